"""Selecting records of compressed batches on the GPU (include/mh.h, "SELECTING RECORDS OF BATCHES"): mh_dev_select_batch and
mh_dev_picks_from_hits on the shapes of tests/select_cases.py, every output, every byte behind the payload and every index
entry exact against tests/select_ref.py with outputs and workspaces prefilled with 0xA5 and 0xFF; refused picks, both
capacities one short, count-only mode, offsets beyond 2^32, and the closure find -> picks -> select -> decode.  Every
expected value comes from the original messages (batch_ref, find_ref, select_ref), never from another call of the library."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import find_ref
import select_cases
import select_ref

pytestmark = pytest.mark.gpu

PREV0 = batch_ref.PREV0
NONE = select_ref.NONE


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


@pytest.mark.parametrize("name", select_cases.NAMES)
def test_select_matches_the_reference(mhc, name):
    c = select_cases.case(name)
    bad = []
    for what, picks in c.picks.items():
        want = select_ref.select(c.packs, picks, c.chunk)
        r = mhc.dev_select_batch(c.sources(), picks, c.chunk)
        bad += select_cases.differences(r, want, c.chunk, "%s, %s" % (name, what))
    assert not bad, "\n".join(bad)


def test_select_into_buffers_full_of_ones(mhc):
    c = select_cases.case("byte lengths")
    for what in ("each twice", "reverse"):
        want = select_ref.select(c.packs, c.picks[what], c.chunk)
        r = mhc.dev_select_batch(c.sources(), c.picks[what], c.chunk, fill=0xFF)
        assert not select_cases.differences(r, want, c.chunk, what, fill=0xFF)


def test_select_without_index_and_without_symbol_offsets(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    picks = c.picks["random"]
    want = select_ref.select(c.packs, picks, c.chunk)
    r = mhc.dev_select_batch(c.sources(index=False), picks, 0)
    assert r.index is None and not select_cases.differences(r, want, c.chunk, "no index", index=False)
    r = mhc.dev_select_batch(c.sources(sym=False), picks, 0, want_sym=False)
    assert not select_cases.differences(r, want, c.chunk, "no sym_off", index=False, sym=False)
    r = mhc.dev_select_batch(c.sources(), picks, c.chunk, want_index=False)
    assert r.index is None and not select_cases.differences(r, want, c.chunk, "index not wanted", index=False)


def test_a_bad_pick_is_refused_alone(mhc):
    """An out-of-range source, an out-of-range stream and a stream whose nbits exceed its bytes set their own status; the
    neighbours stay exact."""
    c = select_cases.case("two sources, order 1, chunk 1024")
    src, packs = select_cases.spoiled(c)
    picks = select_cases.refused_picks(c)
    want = select_ref.select(packs, picks, c.chunk)
    assert want.status.tolist() == [0, -1, 0, -1, -1, 0, -1, 0]
    r = mhc.dev_select_batch(src, picks, c.chunk)
    assert r.status == mhc.MH_ERR_ARG and not select_cases.differences(r, want, c.chunk, "bad picks")


def test_bad_offsets_stop_the_call(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    src = c.sources()
    for field in (1, 3):                                           # pay_off, sym_off of the second source
        rows = list(src)
        row = list(rows[1])
        row[field] = np.asarray(row[field], dtype=np.uint64).copy()
        row[field][2] = row[field][3] + np.uint64(1)
        rows[1] = tuple(row)
        r = mhc.dev_select_batch(rows, c.picks["identity"], c.chunk)
        assert r.status == mhc.MH_ERR_ARG, field
        assert (r.payload == select_cases.FILL).all() and (r.index == select_cases.FILL64).all() and (r.out_off == select_cases.FILL64).all()


def test_capacity_one_short(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    picks = c.picks["each twice"]
    want = select_ref.select(c.packs, picks, c.chunk)
    n, total = len(picks), int(want.pay_off[-1])
    need = int(want.sym_off[n]) // c.chunk + n + 1
    assert need == mhc.lib().mh_batch_index_capacity(int(want.sym_off[n]), n, c.chunk)
    r = mhc.dev_select_batch(c.sources(), picks, c.chunk, cap=total, index_cap=need)
    assert not select_cases.differences(r, want, c.chunk, "exact caps")
    for kw in (dict(cap=total - 1, index_cap=need), dict(cap=total, index_cap=need - 1)):
        r = mhc.dev_select_batch(c.sources(), picks, c.chunk, **kw)
        assert r.status == mhc.MH_ERR_CAPACITY, kw
        assert np.array_equal(r.out_off, want.pay_off) and np.array_equal(r.nbits, want.nbits) and np.array_equal(r.sym_off, want.sym_off)
        assert not r.pick_status.any()
        assert (r.payload == select_cases.FILL).all() and (r.index == select_cases.FILL64).all(), kw    # nothing, so nothing beyond a cap


def test_count_only(mhc):
    c = select_cases.case("byte lengths")
    picks = c.picks["each twice"]
    want = select_ref.select(c.packs, picks, c.chunk)
    r = mhc.dev_select_batch(c.sources(), picks, c.chunk, count_only=True, want_index=False, cap=0)
    assert r.payload is None and not select_cases.differences(r, want, c.chunk, "count only", index=False, count_only=True)
    r = mhc.dev_select_batch(c.sources(), picks, c.chunk, count_only=True, cap=0)                      # the index by itself
    assert not select_cases.differences(r, want, c.chunk, "count only, with the index", count_only=True)


def test_offsets_beyond_4_gib_without_the_memory(mhc):
    """Four streams of 3 GiB each, described by their offsets alone: count-only, no payload, no index.  Every sum is 64-bit."""
    G = 3 << 30
    pay_off = np.arange(5, dtype=np.uint64) * np.uint64(G)
    nbits = np.array([G * 8, G * 8 - 7, G * 8 - 1, G * 8 - 8 + 1], dtype=np.uint64)
    sym_off = np.array([0, 5 << 30, (5 << 30) + 1, 11 << 30, (11 << 30) + (7 << 30)], dtype=np.uint64)
    picks = [3, 0, 0, NONE, 2, 1, 3, 3]
    r = mhc.dev_select_batch([(None, pay_off, nbits, sym_off, None, 0)], picks, 0, count_only=True, cap=0)
    assert r.status == mhc.MH_OK and not r.pick_status.any()
    nb = np.array([0 if p == NONE else int(nbits[p]) for p in picks], dtype=np.uint64)
    syms = [0 if p == NONE else int(sym_off[p + 1]) - int(sym_off[p]) for p in picks]
    assert np.array_equal(r.nbits, nb)
    assert r.out_off.tolist() == [0] + np.cumsum([(int(b) + 7) // 8 for b in nb], dtype=object).tolist() and int(r.out_off[-1]) == 7 * G
    assert r.sym_off.tolist() == [0] + np.cumsum(syms, dtype=object).tolist() and int(r.sym_off[-1]) > 1 << 34


# ---- closure: find -> picks -> select -> decode ---------------------------------------------------------------------------------

def dev_decode(mhc, fn, ws_fn, handle, r, total, sym_total, chunk):
    """One device batch decode (fn: mh_dev_decode_batch or mh_dev_decode_each) of a selected batch through its relocated index:
    (bytes, per-stream status, mh_dev_status)."""
    l = mhc.lib()
    n = len(r.nbits)
    up = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16), np.ascontiguousarray(a) if a.size else None)
    d_pl, d_po, d_nb, d_so, d_idx = up(r.payload), up(r.out_off), up(r.nbits), up(r.sym_off), up(r.index)
    d_out = mhc.DeviceBuffer(sym_total + 64, np.full(sym_total + 64, 0xA5, dtype=np.uint8))
    wsb = ws_fn(n)
    d_st, d_ws = mhc.DeviceBuffer(max(n, 1) * 4), mhc.DeviceBuffer(wsb)
    rc = fn(handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, total, PREV0, d_out.ptr, sym_total, d_so.ptr, sym_total, d_idx.ptr, chunk, d_st.ptr, d_ws.ptr,
            wsb, None)
    assert rc == mhc.MH_OK
    out = d_out.download()
    assert (out[sym_total:] == 0xA5).all()
    return out[:sym_total].tobytes(), d_st.download(np.int32)[:n], l.mh_dev_status(d_ws.ptr, None)


def test_find_picks_select_decode_closes(mhc):
    n, c = 257, 256
    msgs = select_cases.records(n, 21)
    counts = batch_ref.histogram(msgs, 1, PREV0)
    q = batch_ref.pack(msgs, *batch_ref.oracle_codes(counts, 1), 1, PREV0, c)
    model = mhc.Model.from_counts(counts, 1)
    ps = mhc.PatternSet([b"GPU"])
    w_off, _, _ = find_ref.hit_arrays(find_ref.find_hits(msgs, [b"GPU"]), n)
    with_hits = int((np.diff(w_off.astype(np.int64)) > 0).sum())
    assert n // 4 < with_hits < 3 * n // 4
    ho, _, _, st, rc = model.dev_find_batch(ps, q.payload, q.pay_off, q.nbits, PREV0, q.sym_off, q.index_array(c), c, count_only=True)
    assert rc == mhc.MH_OK and np.array_equal(ho, w_off) and not st.any()
    failing = np.zeros(n, dtype=np.int32)
    failing[[0, 5, 100, 256]] = [mhc.MH_ERR_CORRUPT, mhc.MH_ERR_ARG, mhc.MH_ERR_CORRUPT, mhc.MH_ERR_CAPACITY]
    src = [(q.payload, q.pay_off, q.nbits, q.sym_off, q.index_array(c), c)]
    for hit_off, status, flags in ((ho, None, 0), (ho, None, mhc.PICKS_WITHOUT_HITS), (ho, failing, 0), (None, failing, 0), (None, None, 0)):
        want_picks, want_kept = select_ref.picks_from_hits(None if hit_off is None else w_off, status, flags, n=n)
        picks, kept = mhc.dev_picks_from_hits(hit_off, status, n, flags=flags)
        assert kept == want_kept and np.array_equal(picks, want_picks), (hit_off is None, status is None, flags)
        want = select_ref.select([q], want_picks, c)
        r = mhc.dev_select_batch(src, picks, c)                    # n_picks = n: the tail of the batch is empty streams
        assert not select_cases.differences(r, want, c, "closure")
        kept_msgs = [msgs[int(p)] for p in want_picks[:kept]]
        total, sym_total = int(want.pay_off[-1]), int(want.sym_off[-1])
        r.payload, r.index = r.payload[:total], r.index[:r.index_cap]
        out, sst, rc = dev_decode(mhc, mhc.lib().mh_dev_decode_batch, mhc.lib().mh_dev_decode_batch_workspace, model.handle, r, total, sym_total, c)
        assert rc == mhc.MH_OK and not sst.any() and out == b"".join(kept_msgs)
        # every prefix of n_kept streams is a batch; two lookups into it
        if kept >= 2:
            j = max(range(kept), key=lambda k: len(kept_msgs[k]))
            lookups = [(j, len(kept_msgs[j]) // 3, len(kept_msgs[j])), (kept - 1, 0, len(kept_msgs[kept - 1]))]
            got, lst, rc = model.dev_decode_batch_ranges(r.payload, r.out_off, r.nbits, lookups, PREV0, r.sym_off, r.index, c)
            assert rc == mhc.MH_OK and not np.asarray(lst).any()
            assert got == [kept_msgs[a][b:e] for a, b, e in lookups]


def test_a_bank_batch_selects_with_its_choices(mhc):
    """Side information travels with the pick list: choice[picks] names the bank entry of every selected stream."""
    n, c = 60, 256
    rng = np.random.default_rng(31)
    msgs = [m if i % 2 else bytes(rng.integers(0, 256, len(m) + 3).astype(np.uint8)) for i, m in enumerate(select_cases.records(n, 22))]
    bank, choice, _ = mhc.ModelSet.train_bank(msgs, 3, order=1)
    payload, pay_off, nbits, index, sym_off = mhc.encode_bank(bank, msgs, choice, c)
    keep = np.array([i for i in range(n) if i % 3], dtype=np.uint64)[::-1].copy()
    picks = np.concatenate([keep, np.full(4, NONE, dtype=np.uint64)])
    r = mhc.dev_select_batch([(payload, pay_off, nbits, sym_off, index, c)], picks, c)
    assert r.status == mhc.MH_OK and not r.pick_status.any()
    total, sym_total = int(r.out_off[-1]), int(r.sym_off[-1])
    kept_msgs = [msgs[int(i)] for i in keep]
    assert sym_total == sum(len(m) for m in kept_msgs) and np.array_equal(r.nbits[:keep.size], nbits[keep.astype(np.int64)])
    view = bank.pick(np.concatenate([choice[keep.astype(np.int64)], np.zeros(4, dtype=np.uint32)]))
    r.payload, r.index = r.payload[:total], r.index[:r.index_cap]
    out, sst, rc = dev_decode(mhc, mhc.lib().mh_dev_decode_each, mhc.lib().mh_dev_decode_each_workspace, view.handle, r, total, sym_total, c)
    assert rc == mhc.MH_OK and not sst.any() and out == b"".join(kept_msgs)
