"""The numpy reference of include/mh.h "SELECTING RECORDS OF BATCHES" (a helper module like edit_ref.py; it imports numpy and
batch_ref, never the library): what selecting picks from packed batches gives, built from the sources' batch_ref.Packed
objects stream by stream, and the pick list of a per-stream predicate.  tests/test_select_ref.py holds it against
batch_ref.pack of the picked messages."""
import numpy as np

import batch_ref

NONE = 0xFFFFFFFFFFFFFFFF          # include/mh.h MH_SELECT_NONE
SRC_SHIFT = 56                     # pick = source << 56 | stream
MAX_SOURCES = 8                    # include/mh.h MH_SELECT_MAX_SOURCES
WITHOUT_HITS = 1                   # include/mh.h MH_PICKS_WITHOUT_HITS
MH_OK, MH_ERR_ARG = 0, -1


def pick(source, stream):
    return (source << SRC_SHIFT) | stream


def split(p):
    """(source, stream) of a pick, or None for MH_SELECT_NONE."""
    p = int(p)
    return None if p == NONE else (p >> SRC_SHIFT, p & ((1 << SRC_SHIFT) - 1))


def select(packs, picks, chunk=0):
    """The batch_ref.Packed of the picked streams in pick order: payload, pay_off, nbits, sym_off, dropped and, with a chunk,
    the slices.  `status` (int32 per pick) is MH_ERR_ARG for a pick whose source or stream does not exist or whose nbits do
    not fit its payload bytes; such a pick and MH_SELECT_NONE give an empty stream."""
    out = batch_ref.Packed()
    parts, nbits, syms, dropped, status, out.slices = [], [], [], [], [], []
    for p in picks:
        at = split(p)
        ok = at is not None and at[0] < len(packs) and at[1] < len(packs[at[0]].nbits)
        if ok:
            q, i = packs[at[0]], at[1]
            a, z, nb = int(q.pay_off[i]), int(q.pay_off[i + 1]), int(q.nbits[i])
            ok = nb <= (z - a) * 8
        status.append(MH_OK if ok or at is None else MH_ERR_ARG)
        if not ok:
            parts.append(np.zeros(0, dtype=np.uint8)), nbits.append(0), syms.append(0), dropped.append(0)
            out.slices.append(np.zeros(0, dtype=np.uint64))
            continue
        parts.append(q.payload[a:a + (nb + 7) // 8])
        nbits.append(nb), syms.append(int(q.sym_off[i + 1]) - int(q.sym_off[i])), dropped.append(int(q.dropped[i]))
        out.slices.append(np.asarray(q.slices[i], dtype=np.uint64) if chunk else np.zeros(0, dtype=np.uint64))
    scan = lambda v: np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))]).astype(np.uint64)
    out.payload = np.concatenate(parts + [np.zeros(0, dtype=np.uint8)])
    out.nbits, out.dropped = np.array(nbits, dtype=np.uint64), np.array(dropped, dtype=np.uint64)
    out.pay_off, out.sym_off = scan([(b + 7) // 8 for b in nbits]), scan(syms)
    out.status = np.array(status, dtype=np.int32)
    if not chunk:
        out.slices = []
    return out


def picked_messages(message_lists, picks):
    """The messages a pick list names, b"" for MH_SELECT_NONE."""
    return [b"" if split(p) is None else message_lists[split(p)[0]][split(p)[1]] for p in picks]


def picks_from_hits(hit_off, status, flags=0, n=None, source=0):
    """(picks uint64[n], n_kept): the streams with at least one hit (WITHOUT_HITS: with none; hit_off None: all) whose status
    is MH_OK (status None: all), ascending, then MH_SELECT_NONE up to n."""
    if n is None:
        n = len(hit_off) - 1 if hit_off is not None else len(status)
    keep = np.ones(n, dtype=bool)
    if hit_off is not None:
        keep &= (np.diff(np.asarray(hit_off, dtype=np.uint64).astype(np.int64)) > 0) != bool(flags & WITHOUT_HITS)
    if status is not None:
        keep &= np.asarray(status, dtype=np.int32)[:n] == MH_OK
    kept = np.nonzero(keep)[0].astype(np.uint64)
    picks = np.full(n, NONE, dtype=np.uint64)
    picks[:kept.size] = kept | np.uint64(source << SRC_SHIFT)
    return picks, int(kept.size)
