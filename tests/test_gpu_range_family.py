"""The random-access kernel family (csrc/mh_range.hip) at the smallest shapes at which its shared code can go wrong: one
boundary table through every model policy of the lookups, more items than a workgroup with runs of empty lookups, and the two
index formats of the single-stream ranges side by side, intact, behind a payload window and with one damaged entry at a time.
Chunks of 256 symbols, the minimum.  Ground truth: numpy slices of the inputs; positions from the CPU oracle's code lengths."""
import numpy as np
import pytest

import __graft_entry__ as entry
import damage
from test_gpu_range import Enc as Enc1, dev_ranges as dev_ranges1, zipf_bytes
from test_gpu_range_o2 import Enc as Enc2, dev_ranges as dev_ranges2

pytestmark = pytest.mark.gpu

CHUNK = 256
PIECE = 64                                               # MH_FINE_SYMBOLS
GUARD = 64
FILL = 0xA5
CTX0 = 0x2020                                            # the start context: (0x20, 0x20), order 0/1 reads its last byte
SIZES = (0, 1, 255, 256, 257, 700)


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    m = entry.load_package()
    if m.device_count() < 1:
        pytest.skip("no GPU")
    return m


# ---- lookups into batches: one boundary table through every policy -----------------------------------------------------------
POLICIES = ["shared_order0", "shared_order1", "set_mixed_orders", "shared_order2"]


@pytest.fixture(scope="module")
def batches(mhc):
    """Six streams of Zipf bytes coded under each policy: name -> (device call, model handle owner, payload, pay_off, nbits,
    sym_off, batch index)."""
    msgs = [zipf_bytes(n, 100 + n).tobytes() for n in SIZES]
    lib = mhc.lib()
    out = {"msgs": msgs}
    for order in (0, 1):
        m = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=order), order)
        pl, po, nb, idx, so = m.encode_batch(msgs, chunk_symbols=CHUNK)
        out["shared_order%d" % order] = (lib.mh_dev_decode_batch_ranges, m, pl, po, nb, so, idx)
    s = mhc.ModelSet.from_models([mhc.Model.from_data(x if x else b"x", order=i % 2) for i, x in enumerate(msgs)])
    pl, po, nb, idx, so, rc = s.encode(msgs, chunk_symbols=CHUNK)
    assert rc == mhc.MH_OK
    out["set_mixed_orders"] = (lib.mh_dev_decode_each_ranges, s, pl, po, nb, so, idx)
    m = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
    pl, po, nb, idx, so = m.encode_batch_o2(msgs, chunk_symbols=CHUNK)
    out["shared_order2"] = (lib.mh_dev_decode_batch_o2_ranges, m, pl, po, nb, so, idx)
    return out


def dev_lookups(mhc, batch, lk, sym_off=True, index=True):
    """One device lookup call on outputs filled with FILL, GUARD bytes around each.  Returns (call status, mh_dev_status,
    per-lookup status, output buffer, out_at)."""
    fn, owner, pl, po, nb, so, idx = batch
    lib = mhc.lib()
    lk = np.ascontiguousarray(lk, dtype=np.uint64).reshape(-1, 3)
    m, n = lk.shape[0], len(po) - 1
    ln = np.where(lk[:, 1] <= lk[:, 2], lk[:, 2] - lk[:, 1], 0).astype(np.int64)
    at = (GUARD + np.concatenate([[0], np.cumsum(ln + GUARD)[:-1]])).astype(np.uint64)
    cap = int(at[-1]) + int(ln[-1]) + GUARD
    d_pl = mhc.DeviceBuffer(pl.size + 64, init=np.concatenate([pl, np.zeros(64, dtype=np.uint8)]))
    d_po, d_nb = mhc.DeviceBuffer(po.nbytes, init=po), mhc.DeviceBuffer(nb.nbytes, init=nb)
    d_so = mhc.DeviceBuffer(so.nbytes, init=np.ascontiguousarray(so, dtype=np.uint64))
    d_idx = mhc.DeviceBuffer(idx.nbytes, init=idx)
    d_lk, d_at = mhc.DeviceBuffer(lk.nbytes, init=lk), mhc.DeviceBuffer(at.nbytes, init=at)
    d_out = mhc.DeviceBuffer(cap, init=np.full(cap, FILL, dtype=np.uint8))
    d_st = mhc.DeviceBuffer(m * 4, init=np.full(m, 77, dtype=np.int32))
    wsb = lib.mh_dev_decode_batch_ranges_workspace(m)
    d_ws = mhc.DeviceBuffer(wsb)
    rc = fn(owner.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, mhc.PREV0, d_so.ptr if sym_off else None, d_idx.ptr if index else None,
            CHUNK if index else 0, d_lk.ptr, m, d_out.ptr, d_at.ptr, cap, d_st.ptr, d_ws.ptr, wsb, None)
    return rc, lib.mh_dev_status(d_ws.ptr, None), d_st.download(np.int32)[:m], d_out.download()[:cap], at.astype(np.int64)


def check_lookups(mhc, msgs, lk, st, out, at):
    """Every good lookup is MH_OK with the source's bytes, every bad one MH_ERR_ARG, and no byte outside the good lookups'
    outputs changed (a refused lookup writes nothing)."""
    untouched = np.ones(out.size, dtype=bool)
    for j, (i, b, e) in enumerate(np.asarray(lk, dtype=np.int64).reshape(-1, 3).tolist()):
        bad = i >= len(msgs) or b > e or e > len(msgs[i])
        assert st[j] == (mhc.MH_ERR_ARG if bad else mhc.MH_OK), (j, i, b, e, st[j])
        if not bad:
            assert out[at[j]:at[j] + e - b].tobytes() == msgs[i][b:e], (j, i, b, e)
            untouched[at[j]:at[j] + e - b] = False
    assert np.all(out[untouched] == FILL), "bytes written outside the outputs of the lookups that passed"


def boundary_lookups(msgs):
    lk = []
    for i, x in enumerate(msgs):
        n = len(x)
        lk += [(i, 0, 0), (i, 0, n), (i, n, n), (i, max(n - 1, 0), n)]
        lk += [(i, b, e if e is not None else n) for b, e in ((255, 256), (255, 257), (256, 512), (256, None), (300, 301))
               if b <= n and (e is None or e <= n)]
        # the three refusals: no such stream, begin behind end, end past the stream (begin at its end: an index-free walk
        # without sym_off finds that out only at the stream's end, and has stored nothing by then)
        lk += [(len(msgs) + i, 0, 0), (i, 2, 1), (i, n, n + 1)]
    return np.array(lk, dtype=np.uint64)[np.random.default_rng(5).permutation(len(lk))]


@pytest.mark.parametrize("policy", POLICIES)
def test_one_boundary_table_through_every_policy(mhc, batches, policy):
    msgs = batches["msgs"]
    lk = boundary_lookups(msgs)
    for sym_off, index in ((True, True), (True, False), (False, False)):
        rc, dst, st, out, at = dev_lookups(mhc, batches[policy], lk, sym_off, index)
        assert rc == mhc.MH_OK and dst == mhc.MH_ERR_ARG, (sym_off, index, rc, dst)
        check_lookups(mhc, msgs, lk, st, out, at)


@pytest.mark.parametrize("policy", ["shared_order1", "set_mixed_orders", "shared_order2"])
def test_more_items_than_a_workgroup_and_items_that_share_a_base(mhc, batches, policy):
    """300 lookups into the 700-symbol stream, each over three chunks (about 600 items after every third became an empty
    lookup): the grid-stride loop, and item_of over runs of equal bases."""
    msgs = batches["msgs"]
    i, n = len(SIZES) - 1, SIZES[-1]
    rng = np.random.default_rng(6)
    b, e = rng.integers(0, CHUNK, 300), rng.integers(2 * CHUNK + 1, n + 1, 300)
    e[::3] = b[::3]
    lk = np.stack([np.full(300, i), b, e], axis=1).astype(np.uint64)
    rc, dst, st, out, at = dev_lookups(mhc, batches[policy], lk)
    assert rc == mhc.MH_OK and dst == mhc.MH_OK
    check_lookups(mhc, msgs, lk, st, out, at)


# ---- ranges of one stream: the two index formats -----------------------------------------------------------------------------
N = 3 * CHUNK + 17


class Stream:
    """One stream of N Zipf bytes under an oracle model of `order`, encoded on the device with both of its indices; `bounds`
    are the oracle's code boundaries (bit offset of every symbol, then nbits)."""

    def __init__(self, mhc, oracle, order):
        self.mhc, self.order = mhc, order
        self.data = zipf_bytes(N, 11)
        om = oracle.Model.from_data(self.data.tobytes(), order)
        self.model = mhc.Model.from_table(om.table_bytes())
        self.enc = (Enc2 if order == 2 else Enc1)(mhc, self.model, self.data, CHUNK)
        self.fine = self.enc.d_fine.download(np.uint32)[:(N + PIECE - 1) // PIECE]
        self.pos_mask = (1 << 48) - 1 if order == 2 else mhc.INDEX_BIT_MASK
        self.bounds = damage.boundaries(om.codes_o2()[0] if order == 2 else om.codes()[0], self.data, order, CTX0)
        assert self.bounds[-1] == self.enc.nbits
        assert np.array_equal(self.enc.index & np.uint64(self.pos_mask), self.bounds[0:N:CHUNK].astype(np.uint64))

    def decode(self, ranges, fine, payload=None, base=0, nbytes=None, d_index=None, d_fine=None):
        """One device call: (call status, mh_dev_status, per-range status, output bytes, out_at).  The callee also checks
        that nothing is written outside the outputs of the ranges that passed the count."""
        e = self.enc
        call = dev_ranges2 if self.order == 2 else dev_ranges1
        r = call(self.mhc, self.model, payload if payload is not None else e.d_payload.ptr, base,
                 nbytes if nbytes is not None else (e.nbits + 7) // 8, e.nbits, (e.d_index if d_index is None else d_index).ptr, CHUNK, N,
                 (e.d_fine if d_fine is None else d_fine).ptr if fine else None, ranges)
        return r[:5]

    def check(self, ranges, st, out, at, want=None):
        """want[j]: the status of range j (default: all MH_OK); a range that is MH_OK has the source's bytes."""
        for j, (b, e) in enumerate(np.asarray(ranges, dtype=np.int64).reshape(-1, 2).tolist()):
            w = 0 if want is None else int(want[j])
            assert st[j] == w, (j, b, e, st[j], w)
            if w == 0:
                assert np.array_equal(out[int(at[j]):int(at[j]) + e - b], self.data[b:e]), (j, b, e)


@pytest.fixture(scope="module")
def stream1(mhc, oracle):
    return Stream(mhc, oracle, 1)


@pytest.fixture(scope="module")
def stream2(mhc, oracle):
    return Stream(mhc, oracle, 2)


@pytest.fixture(params=["stream1", "stream2"], ids=["order1", "order2"])
def stream(request):
    return request.getfixturevalue(request.param)


MARKS = [0, 10, 255, 256, 257, 300, 383, 384, 385, 400, 447, 448, 449, 500, 511, 512, 513, 600, 767, 768, 769, 780, N]
ALL_PAIRS = [(b, e) for b in MARKS for e in MARKS if b < e] + [(0, 0), (256, 256), (N, N)]


@pytest.mark.parametrize("fine", [False, True], ids=["chunk_index", "fine_index"])
def test_ranges_ending_inside_a_piece_on_its_boundary_on_a_chunk_boundary_and_at_the_end(mhc, stream, fine):
    ranges = [(10, 100), (10, 128), (130, 192), (10, 256), (200, 512), (256, 512), (511, 513), (700, N), (767, N), (0, N), (N, N)]
    rc, dst, st, out, at = stream.decode(ranges, fine)
    assert rc == 0 and dst == 0
    stream.check(ranges, st, out, at)
    rc, dst, st, out, at = stream.decode(ALL_PAIRS, fine)
    assert rc == 0 and dst == 0
    stream.check(ALL_PAIRS, st, out, at)


@pytest.mark.parametrize("fine", [False, True], ids=["chunk_index", "fine_index"])
def test_payload_window_over_chunk_1_at_four_byte_offsets(mhc, stream, fine):
    s = stream
    lo, hi = int(s.bounds[CHUNK]) >> 3, (int(s.bounds[2 * CHUNK]) + 7) >> 3
    inside = [(256, 512), (256, 257), (300, 301), (320, 448), (383, 385), (511, 512), (400, 400)]
    outside = [(255, 257), (0, 10), (100, 300), (600, N), (770, 780), (500, N)]         # a unit in front of or behind the window
    for shift in range(4):
        win = np.concatenate([np.full(shift, 0xCC, dtype=np.uint8), s.enc.payload[lo:hi], np.zeros(16, dtype=np.uint8)])
        d_win = mhc.DeviceBuffer(win.size, init=win)
        rc, dst, st, out, at = s.decode(inside + outside, fine, payload=d_win.ptr.value + shift, base=lo, nbytes=hi - lo)
        assert rc == 0 and dst == mhc.MH_ERR_ARG
        s.check(inside + outside, st, out, at, want=[0] * len(inside) + [mhc.MH_ERR_ARG] * len(outside))


@pytest.mark.parametrize("fine", [False, True], ids=["chunk_index", "fine_index"])
def test_window_cut_inside_the_last_unit_is_where_the_formats_differ(mhc, stream, fine):
    """The range [256, 300) ends in the middle of its unit, and the window ends with the byte that holds the range's last bit.
    Order 0/1 wants the whole unit in the window (include/mh.h, mh_dev_decode_ranges: "d_range_status[j]: MH_OK, MH_ERR_ARG
    (begin > end, end > n_symbols, a unit outside the payload window)"), so the range is MH_ERR_ARG.  Order 2 judges what the
    lane read ("A range of mh_dev_decode_ranges_o2 whose decode reads past the payload window is MH_ERR_ARG"): this decode
    stays inside, so the range is MH_OK and exact."""
    s = stream
    b, e = 256, 300
    lo, hi = int(s.bounds[b]) >> 3, (int(s.bounds[e]) + 7) >> 3
    assert hi * 8 < int(s.bounds[320])                    # the unit (chunk or piece) ends behind the window
    win = np.concatenate([s.enc.payload[lo:hi], np.zeros(16, dtype=np.uint8)])
    d_win = mhc.DeviceBuffer(win.size, init=win)
    ranges = [(b, e), (b, b + 1), (280, e)]
    rc, dst, st, out, at = s.decode(ranges, fine, payload=d_win.ptr, base=lo, nbytes=hi - lo)
    assert rc == 0
    if s.order == 2:
        assert dst == 0
        s.check(ranges, st, out, at)
    else:
        assert dst == mhc.MH_ERR_ARG
        s.check(ranges, st, out, at, want=[mhc.MH_ERR_ARG] * 3)


def reads_bad_unit(unit, starts, nbits):
    """The ranges of ALL_PAIRS that touch a unit whose start lies past nbits or behind the start before it, or that end on
    such a unit's start boundary (include/mh.h, "Checks")."""
    bad = {u for u in range(len(starts)) if starts[u] > nbits or (u > 0 and starts[u] < starts[u - 1])}
    return np.array([b < e and (bool(set(range(b // unit, (e - 1) // unit + 1)) & bad) or (e % unit == 0 and e < N and e // unit in bad))
                     for b, e in ALL_PAIRS])


@pytest.mark.parametrize("kind", ["behind_predecessor", "past_nbits"])
def test_damaged_chunk_entry_fails_exactly_the_ranges_that_read_it(mhc, stream, kind):
    s = stream
    nbits = s.enc.nbits
    starts = [int(x) for x in s.bounds[0:N:CHUNK]]
    starts[2] = starts[1] - 9 if kind == "behind_predecessor" else nbits + 12345
    idx = s.enc.index.copy()
    idx[2] = (idx[2] & ~np.uint64(s.pos_mask)) | np.uint64(starts[2])
    want = reads_bad_unit(CHUNK, starts, nbits)
    assert want.any() and not want.all()
    rc, dst, st, out, at = s.decode(ALL_PAIRS, False, d_index=mhc.DeviceBuffer(idx.nbytes, init=idx))
    assert rc == 0 and dst == mhc.MH_ERR_CORRUPT
    s.check(ALL_PAIRS, st, out, at, want=np.where(want, mhc.MH_ERR_CORRUPT, 0))


Q = 6                                                    # a piece inside chunk 1, not its first


def test_damaged_fine_entry_fails_exactly_the_ranges_that_read_it(mhc, stream):
    """Order 0/1: the entry of piece Q lies behind the piece in front.  Order 2: it is usable and lies past the next chunk
    entry."""
    s = stream
    fine = s.fine.copy()
    if s.order == 2:
        span = int(s.bounds[2 * CHUNK] - s.bounds[CHUNK])
        assert span + 9 < 0xFFFF
        fine[Q] = (fine[Q] & np.uint32(0xFFFF0000)) | np.uint32(span + 9)
        want = np.array([b < e and (b // PIECE <= Q <= (e - 1) // PIECE or e == Q * PIECE) for b, e in ALL_PAIRS])
    else:
        starts = [int(x) for x in s.bounds[0:N:PIECE]]
        starts[Q] = starts[Q - 1] - 3
        fine[Q] = (fine[Q] & np.uint32(0xFF000000)) | np.uint32(starts[Q] & 0xFFFFFF)
        want = reads_bad_unit(PIECE, starts, s.enc.nbits)
    assert want.any() and not want.all()
    rc, dst, st, out, at = s.decode(ALL_PAIRS, True, d_fine=mhc.DeviceBuffer(fine.nbytes, init=fine))
    assert rc == 0 and dst == mhc.MH_ERR_CORRUPT
    s.check(ALL_PAIRS, st, out, at, want=np.where(want, mhc.MH_ERR_CORRUPT, 0))


def test_order2_fine_entry_that_does_not_fit_falls_back_to_the_piece_in_front(mhc, stream2):
    """0xFFFF is no error: the lane of piece Q starts at piece Q - 1, a range that ends at Q's start is checked as one that
    ends inside a unit, and every range stays exact."""
    s = stream2
    fine = s.fine.copy()
    fine[Q] |= np.uint32(0xFFFF)
    rc, dst, st, out, at = s.decode(ALL_PAIRS, True, d_fine=mhc.DeviceBuffer(fine.nbytes, init=fine))
    assert rc == 0 and dst == 0
    s.check(ALL_PAIRS, st, out, at)


# ---- the workspace --------------------------------------------------------------------------------------------------------
WORKSPACE = {0: 256, 1: 256, 2: 256, 1000: 8192, 65536: 525056, 1 << 20: 8397056}     # tests/test_range_abi.py pins the functions


def test_every_device_call_refuses_a_workspace_one_byte_short(mhc, batches, stream1, stream2):
    """All six device calls of the family size their workspace alike (mh_dev_decode_each_ranges takes the batch function's
    size) and refuse one byte less before anything is launched: the buffers here hold nothing."""
    lib = mhc.lib()
    d = mhc.DeviceBuffer(1 << 16)
    p = d.ptr
    for n, ws in WORKSPACE.items():
        for policy in POLICIES:
            fn, owner = batches[policy][:2]
            rc = fn(owner.handle, p, p, p, len(SIZES), mhc.PREV0, None, None, 0, p, n, p, p, 64, p, p, ws - 1, None)
            assert rc == mhc.MH_ERR_CAPACITY, (policy, n, rc)
        for s, fn in ((stream1, lib.mh_dev_decode_ranges), (stream2, lib.mh_dev_decode_ranges_o2)):
            rc = fn(s.model.handle, p, 0, 64, 512, p, CHUNK, 400, None, p, n, p, p, 16, p, p, ws - 1, None)
            assert rc == mhc.MH_ERR_CAPACITY, (s.order, n, rc)
