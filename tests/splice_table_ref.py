"""The reference of the table splice (include/mh.h, "SPLICING WITH A REPLACEMENT TABLE"): plain Python on the original
messages (a helper module for the tests and tools/splice_rate.py).

A table splice while re-coding must give what re-coding the spliced messages gives, so the expected output is
recode_ref.recode(apply(messages, span_off, spans, tags, reps), dst, chunk).  apply() builds each message from the pieces
between the spans; merge_tagged() merges search records with their patterns into tagged spans by sorting the intervals by
begin and sweeping, which is not the library's method (a reverse min-scan over records that ascend by end, then a segmented
minimum)."""
import numpy as np


def apply(messages, span_off, spans, tags, reps):
    """The edited messages: every span (begin <= end) whose begin lies inside the message is replaced by reps[its tag], its
    end clipped to the length; begin == end inserts in front of x[begin]; a span or an insertion that begins at or beyond
    the length is ignored.  Spans take effect in list order."""
    sp = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    tags = [int(t) for t in tags]
    reps = [bytes(r) for r in reps]
    out = []
    for i, msg in enumerate(messages):
        msg = bytes(msg)
        pieces, at = [], 0
        lo, hi = int(span_off[i]), int(span_off[i + 1])
        for (b, e), t in zip(sp[lo:hi].tolist(), tags[lo:hi]):
            assert at <= b <= e, "a malformed list has no spliced message"
            if b >= len(msg):
                break
            pieces += [msg[at:b], reps[t]]
            at = min(e, len(msg))
        pieces.append(msg[at:])
        out.append(b"".join(pieces))
    return out


def well_formed(lst):
    """The span rule of the table splice on one stream's list of (begin, end): begin <= end <= next begin."""
    at = 0
    for b, e in lst:
        if not at <= b <= e:
            return False
        at = e
    return True


def merge_tagged(hit_off, hits, patterns):
    """Records (stream, begin, end) with their pattern numbers merged into maximal spans, overlapping or touching intervals
    together, each span tagged with the lowest pattern number among its records: (span_off[n + 1], spans[m, 2], tags[m])."""
    hit_off = [int(x) for x in hit_off]
    rec = np.asarray(hits, dtype=np.uint64).reshape(-1, 3).tolist()
    pat = [int(p) for p in patterns]
    n = len(hit_off) - 1
    span_off, spans, tags = [0], [], []
    for i in range(n):
        iv = sorted((b, e, pat[r]) for r, (s, b, e) in zip(range(hit_off[i], hit_off[i + 1]), rec[hit_off[i]:hit_off[i + 1]]))
        cur = None
        for b, e, p in iv:
            if cur is not None and b <= cur[1]:
                cur = [cur[0], max(cur[1], e), min(cur[2], p)]
            else:
                if cur is not None:
                    spans.append(cur[:2]); tags.append(cur[2])
                cur = [b, e, p]
        if cur is not None:
            spans.append(cur[:2]); tags.append(cur[2])
        span_off.append(len(spans))
    return (np.asarray(span_off, dtype=np.uint64), np.asarray(spans, dtype=np.uint64).reshape(-1, 2), np.asarray(tags, dtype=np.uint32))


def tagged_lists(per):
    """Per-stream lists of (begin, end, tag) -> (span_off[n + 1], spans[m, 2], tags[m])."""
    off = np.zeros(len(per) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    flat = [x for p in per for x in p]
    spans = np.asarray([(b, e) for b, e, _ in flat], dtype=np.uint64).reshape(-1, 2)
    return off, spans, np.asarray([t for _, _, t in flat], dtype=np.uint32)


def offsets(messages):
    """The exclusive scan of the messages' lengths, n + 1 entries."""
    off = np.zeros(len(messages) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    return off
