"""The batch call family on dirty and reused device memory: include/mh.h promises "Workspaces: query the size, allocate once,
reuse", and every other GPU test hands every call a fresh allocation as workspace and as output.  Here the fuzz rig of
tests/test_gpu_batch_fuzz.py (every family, compared exactly with the references of tests/batch_ref.py) runs under the
allocation modes of the test binding (device_memory):
  fill      every workspace and every output that the binding does not initialise itself starts as 0xFF or 0xA5 bytes;
  recycle   the case, then its neighbour in the case list, then the case again, on one pool of buffers that is never cleared:
            the third run gets the first run's blocks back, dirtied by the neighbour with valid-looking leftovers of other
            data.  It must be served from the pool entirely, or it could pass on fresh memory.
A counter that is not reset, a ready flag of the last run, a slot that is written only on failure show up here as a difference.

One test per case and mode; the cases are every third one of the fuzz (SUBSET; test_the_subset_keeps_its_coverage pins
what that subset reaches)."""
import gc

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
from test_gpu_batch_fuzz import Rig

CASES = batch_ref.draw_cases()
SUBSET = CASES[::3]
gpu = pytest.mark.gpu


def test_the_subset_keeps_its_coverage():
    assert len(CASES) == 96 and len(SUBSET) == 32
    assert {c.orders for c in SUBSET} == {(a, b) for a in (0, 1, 2) for b in (0, 1, 2)}
    assert {c.src_kind for c in SUBSET} == {"own", "limited", "deep"}
    assert {c.dst_kind for c in SUBSET} == {"own", "foreign", "deep", "limited"}
    assert {c.n_streams for c in SUBSET} == set(batch_ref.STREAM_COUNTS)
    assert {c.chunk for c in SUBSET} == set(batch_ref.CHUNKS)
    assert sum(Rig.eligible(c) for c in SUBSET) == 15


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def device_forms(rig):
    """The rig's encode and decode families go through the host forms, which allocate inside the library, out of the modes'
    reach.  Here mh_dev_encode_batch and mh_dev_decode_batch (or their _o2 forms) run on DeviceBuffers: workspace, payload,
    offsets, lengths, decoded bytes and statuses come from the mode; the index gets zeros (its gaps are left untouched)."""
    mhc, S, rs, n, c, p0 = rig.mhc, rig.S, rig.rs, rig.n, rig.c, rig.p0
    l, B, o2 = mhc.lib(), mhc.DeviceBuffer, rig.so == 2
    data = np.frombuffer(rig.joined, dtype=np.uint8)
    total, pay_total = data.size, int(rs.pay_off[n])
    nidx = int(l.mh_batch_index_capacity(total, n, c))
    cap = l.mh_encode_batch_bound(S.handle, total, n)
    d_data, d_in = B(max(total, 1), data if total else None), B((n + 1) * 8, rs.sym_off)
    d_pl, d_po, d_nb, d_idx = B(cap + 64), B((n + 1) * 8), B(max(n, 1) * 8), B(nidx * 8, np.zeros(nidx, dtype=np.uint64))
    wsb = (l.mh_dev_encode_batch_o2_workspace if o2 else l.mh_dev_encode_batch_workspace)(n, total)
    d_ws = B(wsb)
    rc = (l.mh_dev_encode_batch_o2 if o2 else l.mh_dev_encode_batch)(S.handle, d_data.ptr, d_in.ptr, n, total, p0, d_pl.ptr, cap, d_po.ptr, d_nb.ptr,
                                                                     d_idx.ptr, c, d_ws.ptr, wsb, None)
    rig.check(rc == 0 and l.mh_dev_status(d_ws.ptr, None) == 0, "device encode: status")
    rig.same_batch((d_pl.download()[:pay_total], d_po.download(np.uint64), d_nb.download(np.uint64)[:n], d_idx.download(np.uint64), rs.sym_off), rs,
                   "device encode")
    dec, dec_ws = (l.mh_dev_decode_batch_o2, l.mh_dev_decode_batch_o2_workspace) if o2 else (l.mh_dev_decode_batch, l.mh_dev_decode_batch_workspace)
    for indexed in (True, False):                                  # (reads what the device encode wrote)
        wsb = dec_ws(n)
        d_ws, d_out, d_st = B(wsb), B(total + 64), B(max(n, 1) * 4)
        d_so = d_in if indexed else B((n + 1) * 8)
        rc = dec(S.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, p0, d_out.ptr, total, d_so.ptr, total if indexed else 0,
                 d_idx.ptr if indexed else None, c if indexed else 0, d_st.ptr, d_ws.ptr, wsb, None)
        rig.ok(rc or l.mh_dev_status(d_ws.ptr, None), d_st.download(np.int32)[:n], "device decode indexed=%s" % indexed)
        rig.check(d_out.download()[:total].tobytes() == rig.joined and np.array_equal(d_so.download(np.uint64), rs.sym_off),
                  "device decode indexed=%s" % indexed)


def run(mhc, case):
    """Every family the fuzz runs for this case, and the device forms of encode and decode; the list of what differed.  The rig
    and its buffers are gone on return."""
    rig = Rig(mhc, case)
    rig.run_all()

    def device_encode_decode():
        device_forms(rig)
    rig.family(device_encode_decode)
    bad = rig.bad
    del rig, device_encode_decode
    gc.collect()
    return bad


def report(case, bad):
    return "%s: %d differences:\n  %s" % (case.id, len(bad), "\n  ".join(bad))


@gpu
@pytest.mark.parametrize("byte", [0xFF, 0xA5], ids=["fill-ff", "fill-a5"])
@pytest.mark.parametrize("case", SUBSET, ids=[c.id for c in SUBSET])
def test_every_batch_call_on_filled_memory(mhc, case, byte):
    with mhc.device_memory("fill", byte):
        bad = run(mhc, case)
    assert not bad, report(case, bad)


@gpu
@pytest.mark.parametrize("case", SUBSET, ids=["recycle-" + c.id for c in SUBSET])
def test_every_batch_call_on_recycled_memory(mhc, case):
    neighbour = CASES[(case.index + 1) % len(CASES)]
    gc.collect()
    with mhc.device_memory("recycle") as mem:
        first = run(mhc, case)                                    # stocks the pool with blocks of the case's own sizes
        between = run(mhc, neighbour)                             # dirties them
        served, missed = mem.served, mem.missed
        again = run(mhc, case)
        served, missed = mem.served - served, mem.missed - missed
    assert not first, "first run: " + report(case, first)
    assert not between, "neighbour: " + report(neighbour, between)
    assert not again, "third run, on reused memory: " + report(case, again)
    assert missed == 0 and served > 0, "the third run got fresh memory for %d of its %d requests without init" % (missed, missed + served)


# ---- the modes themselves ----
@gpu
def test_fill_mode_fills_buffers_without_init(mhc):
    with mhc.device_memory("fill", 0x5C):
        plain = mhc.DeviceBuffer(1000)
        given = mhc.DeviceBuffer(1000, np.arange(250, dtype=np.uint32))
        assert (plain.download() == 0x5C).all()
        assert np.array_equal(given.download(np.uint32), np.arange(250, dtype=np.uint32))


@gpu
def test_recycle_mode_hands_back_what_was_left(mhc):
    pattern = (np.arange(4096) * 7 % 251).astype(np.uint8)
    with mhc.device_memory("recycle") as mem:
        a = mhc.DeviceBuffer(4096, pattern)
        small = mhc.DeviceBuffer(100, np.zeros(100, dtype=np.uint8))
        addr = a.ptr.value
        del a, small
        gc.collect()
        assert (mem.served, mem.missed) == (0, 0)                 # (requests with init are not counted)
        b = mhc.DeviceBuffer(4096)                                # best fit: the 4096-byte block, not a fresh one
        assert b.ptr.value == addr and np.array_equal(b.download(), pattern) and (mem.served, mem.missed) == (1, 0)
        c = mhc.DeviceBuffer(64)                                  # the smallest block of at least 64 bytes: the 100-byte one
        assert c.block == 100 and c.nbytes == 64 and (mem.served, mem.missed) == (2, 0)
        d = mhc.DeviceBuffer(8192)                                # nothing that large in the pool
        assert (mem.served, mem.missed) == (2, 1)
        del b
        gc.collect()
        e = mhc.DeviceBuffer(4000, np.full(16, 0xEE, dtype=np.uint8))   # init over the front, the rest as it was left
        got = e.download()
        assert e.ptr.value == addr and (got[:16] == 0xEE).all() and np.array_equal(got[16:], pattern[16:4000])
        assert (mem.served, mem.missed) == (2, 1)
        del c, d, e
    assert not mem.pool, "leaving the mode frees the pool"


@gpu
def test_nothing_changes_outside_the_modes(mhc):
    a = mhc.DeviceBuffer(4096, np.full(4096, 0x11, dtype=np.uint8))
    assert a.block == a.nbytes == 4096
    del a
    gc.collect()
    mem = mhc._memory
    assert mem.mode is None and not mem.pool                      # a buffer freed outside the modes is freed, not pooled
    with mhc.device_memory("fill", 0xFF):
        pass
    b = mhc.DeviceBuffer(4096, np.full(4096, 0x22, dtype=np.uint8))
    assert mem.mode is None and (b.download() == 0x22).all()
    with pytest.raises(ValueError):
        mhc.device_memory("zero")
