"""The reference of masked re-coding (include/mh.h, "EDITING BATCHES"): plain Python/numpy on the original messages (a helper
module for the tests and tools/edit_rate.py).

An edit while re-coding must give what re-coding the edited messages gives, so the expected output of an edit is
recode_ref.recode(apply(messages, span_off, spans, map), dst, chunk): this module only merges search records into spans and
applies a span list to messages.  merge_hits sorts a stream's intervals by begin and sweeps them, which is not how the library
merges them (a reverse min-scan over the records in their (end, pattern) order)."""
import numpy as np


def merge_hits(hit_off, hits):
    """The union of every stream's records as maximal spans, overlapping or touching records merged: (span_off[n + 1],
    spans[m, 2]).  hit_off[n + 1]: the exclusive scan of the streams' record counts; hits[k, 3] = (stream, begin, end)."""
    hit_off = np.asarray(hit_off, dtype=np.uint64)
    hits = np.asarray(hits, dtype=np.uint64).reshape(-1, 3)
    n = len(hit_off) - 1
    span_off, spans = np.zeros(n + 1, dtype=np.uint64), []
    for i in range(n):
        span_off[i] = len(spans)
        iv = sorted((int(b), int(e)) for _, b, e in hits[int(hit_off[i]):int(hit_off[i + 1])])
        for b, e in iv:
            if spans and len(spans) > int(span_off[i]) and b <= spans[-1][1]:
                spans[-1][1] = max(spans[-1][1], e)
            else:
                spans.append([b, e])
    span_off[n] = len(spans)
    return span_off, np.array(spans, dtype=np.uint64).reshape(-1, 2)


def apply(messages, span_off, spans, byte_map):
    """The edited messages: byte b at a position inside one of its stream's spans becomes byte_map[b]; the part of a span at or
    beyond the message's length is ignored.  span_off None: every byte of every message is inside."""
    m = np.asarray(bytearray(bytes(byte_map)), dtype=np.uint8)
    assert m.size == 256
    sp = None if span_off is None else np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    out = []
    for i, msg in enumerate(messages):
        d = np.frombuffer(bytes(msg), dtype=np.uint8).copy()
        if span_off is None:
            d = m[d]
        else:
            for b, e in sp[int(span_off[i]):int(span_off[i + 1])]:
                b, e = min(int(b), d.size), min(int(e), d.size)
                d[b:e] = m[d[b:e]]
        out.append(d.tobytes())
    return out


def mask_map(byte):
    """The map of a mask: every byte becomes `byte`."""
    return bytes([byte]) * 256


IDENTITY = bytes(range(256))
