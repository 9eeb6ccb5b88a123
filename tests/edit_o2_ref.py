"""What the batch encoders do not return, for the tests of include/mh.h "ORDER 2 IN EDITING AND SPLICING" (a helper module):
the dropped count of a message under a destination of any order, and the destination context a chunk's lane must start in
after a table splice.  Plain Python over byte strings; tests/test_edit_o2_ref.py proves both against string slicing.

The expected output of the calls themselves is the composition, as everywhere in this family: edit_ref.apply or
splice_table_ref.apply on the original messages, then the batch encoder under dst."""
import numpy as np


def contexts(message, prev0, order):
    """The context of every byte of `message` as the encoder of that order has it: 0 (order 0), y[p - 1] (order 1) or
    (y[p - 2] << 8) | y[p - 1] (order 2), with prev0 standing for every position in front of 0."""
    d = np.frombuffer(bytes(message), dtype=np.uint8).astype(np.int64)
    p1 = np.concatenate([[prev0], d[:-1]])[:d.size]
    p2 = np.concatenate([[prev0, prev0], d[:-2]])[:d.size]
    return [np.zeros(d.size, dtype=np.int64), p1, (p2 << 8) | p1][order]


def dropped(message, live, prev0):
    """The symbols of `message` without a code under a destination whose (context, symbol) pairs with a code are live[(context
    << 8) | symbol] != 0: 256 entries for order 0, 65 536 for order 1, 1 << 24 for order 2 (the model's training counts serve:
    a pair has a code exactly when it was counted).  A dropped symbol still advances the context."""
    live = np.asarray(live).reshape(-1)
    order = {256: 0, 65536: 1, 1 << 24: 2}[live.size]
    d = np.frombuffer(bytes(message), dtype=np.uint8).astype(np.int64)
    return int((live[(contexts(message, prev0, order) << 8) | d] == 0).sum())


def start_context(messages, span_off, spans, tags, reps, F, prev0):
    """Per message: the last two OUTPUT bytes in front of source position F of a table splice, as (earlier << 8) | later, or
    None when the message has no position F (F >= its length) — by brute force: the output of the spans that begin in
    front of F (a span that begins at F, an insertion there included, belongs to what follows), then the source bytes
    between the last of them and F, with prev0 for every position in front of the output's first byte."""
    sp = np.asarray(spans, dtype=np.uint64).reshape(-1, 2).tolist()
    out = []
    for i, msg in enumerate(messages):
        msg = bytes(msg)
        if F >= len(msg):
            out.append(None)
            continue
        y, at = bytearray([prev0, prev0]), 0
        for r in range(int(span_off[i]), int(span_off[i + 1])):
            b, e = sp[r]
            if b >= F:
                break
            y += msg[at:b] + bytes(reps[int(tags[r])])
            at = min(e, len(msg))
        y += msg[at:F]                                   # (empty when the last span reaches over F)
        out.append((y[-2] << 8) | y[-1])
    return out
