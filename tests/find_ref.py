"""The reference of the search in batches (include/mh.h, "SEARCH IN BATCHES"): plain Python on the original messages
(a helper module for the tests and tools/find_rate.py; it never sees a compressed byte).

A hit is (stream, begin, end, pattern number); hits come in the order of the contract: ascending (stream, end, pattern)."""
import numpy as np

_UPPER = bytes(range(ord("A"), ord("Z") + 1))
_LOWER = bytes(range(ord("a"), ord("z") + 1))
_FOLD = bytes.maketrans(_UPPER, _LOWER)


def fold_ascii(b):
    """`b` with 'A'..'Z' lowered; no other byte changes (not bytes.lower() by name, but the same table for ASCII)."""
    return bytes(b).translate(_FOLD)


def occurrences(message, pattern):
    """Start offsets of every occurrence of `pattern` in `message`, overlapping ones included."""
    message, pattern = bytes(message), bytes(pattern)
    out, at = [], message.find(pattern)
    while at >= 0:
        out.append(at)
        at = message.find(pattern, at + 1)
    return out


def find_hits(messages, patterns, fold=False):
    """Every hit of every pattern in every message, nothing across message boundaries: a list of (stream, begin, end, pattern)
    in ascending (stream, end, pattern) order."""
    pats = [fold_ascii(p) if fold else bytes(p) for p in patterns]
    assert all(len(p) > 0 for p in pats)
    hits = []
    for i, m in enumerate(messages):
        m = fold_ascii(m) if fold else bytes(m)
        here = [(at + len(p), j, at) for j, p in enumerate(pats) for at in occurrences(m, p)]
        hits.extend((i, at, end, j) for end, j, at in sorted(here))
    return hits


def hit_arrays(hits, n_streams):
    """(hit_off uint64[n + 1], records uint64[k, 3], pattern uint32[k]) of a list of hits, as the device calls write them."""
    off = np.zeros(n_streams + 1, dtype=np.uint64)
    for i, _, _, _ in hits:
        off[i + 1] += np.uint64(1)
    off = np.cumsum(off, dtype=np.uint64)
    rec = np.array([(i, b, e) for i, b, e, _ in hits], dtype=np.uint64).reshape(-1, 3)
    pat = np.array([j for _, _, _, j in hits], dtype=np.uint32)
    return off, rec, pat


def lines_with(hits, pattern_number):
    """Number of distinct streams that have a hit of pattern `pattern_number`."""
    return len({i for i, _, _, j in hits if j == pattern_number})


def straddles(hits, chunk):
    """Hits whose bytes lie in two chunks of their stream."""
    return sum(1 for _, b, e, _ in hits if b // chunk != (e - 1) // chunk)
