"""The reference of splicing re-coding (include/mh.h, "SPLICING BATCHES"): plain Python on the original messages (a helper
module for the tests and tools/splice_rate.py).

A splice while re-coding must give what re-coding the spliced messages gives, so the expected output of a splice is
recode_ref.recode(apply(messages, span_off, spans, rep), dst, chunk): this module only applies a span list and a replacement
to messages.  It builds each message from the pieces between the spans, which is not how the library walks them (a cursor of
three states over the symbols of a chunk)."""
import numpy as np


def apply(messages, span_off, spans, rep):
    """The spliced messages: every span whose begin lies inside the message is replaced by `rep`, its end clipped to the
    message's length; a span that begins at or beyond the length is ignored."""
    rep = bytes(rep)
    sp = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    out = []
    for i, msg in enumerate(messages):
        msg = bytes(msg)
        pieces, at = [], 0
        for b, e in sp[int(span_off[i]):int(span_off[i + 1])].tolist():
            assert at <= b < e, "a malformed list has no spliced message"
            if b >= len(msg):
                break
            pieces += [msg[at:b], rep]
            at = min(e, len(msg))
        pieces.append(msg[at:])
        out.append(b"".join(pieces))
    return out


def offsets(messages):
    """The exclusive scan of the messages' lengths, n + 1 entries."""
    off = np.zeros(len(messages) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    return off
