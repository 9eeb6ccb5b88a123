"""Random access into order-2 streams on the GPU (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS"): byte ranges of one
indexed stream, with and without the order-2 fine index, and lookups into batches of mh_encode_batch_o2, indexed and
index-free.  Ground truth: numpy slices of the input; on damaged streams, the contract of tests/damage.py (CPU oracle)."""

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
from conftest import golden
from damage import MH_OK, MH_ERR_CORRUPT

pytestmark = pytest.mark.gpu

GOLDEN5 = ["input_a.txt", "input_b.txt", "input_ipsum.txt", "input_wiki_cpp.html", "input_wiki_cpp.txt"]
GUARD = 64
FILL = 0xA5
POS2 = (1 << 48) - 1
CTX0 = 0x2020


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    m = entry.load_package()
    if m.device_count() < 1:
        pytest.skip("no GPU")
    return m


def zipf_bytes(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def text_like(n, seed, base=1 << 20):
    """Words of a seeded 300-word vocabulary (base bytes of them, tiled to n)."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9)).astype(np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < min(n, base):
        out += words[int(rng.integers(0, 300))] + (b".\n" if rng.random() < 0.05 else b" ")
    a = np.frombuffer(bytes(out[:min(n, base)]), dtype=np.uint8)
    return np.tile(a, (n + a.size - 1) // a.size)[:n].copy()


def model_o2(mhc, data):
    """An order-2 model of `data` built on the device (histogram in context (0x20, 0x20), tree build)."""
    lib = mhc.lib()
    d_data = mhc.DeviceBuffer(data.size + 32, init=np.concatenate([data, np.zeros(32, dtype=np.uint8)]))
    d_counts = mhc.DeviceBuffer((1 << 24) * 8)
    mhc._check(lib.mh_dev_histogram_o2(d_data.ptr, data.size, CTX0, d_counts.ptr, None), "hist2")
    m = mhc.Model.from_device_counts(d_counts.ptr, 2)
    assert m.type == 2
    return m


class Enc:
    """A stream encoded on the device with its order-2 chunk index and, for chunk_symbols <= 1024, its order-2 fine index
    (mh_dev_encode_ctx_fine)."""

    def __init__(self, mhc, model, data, chunk):
        lib = mhc.lib()
        self.mhc, self.model, self.data, self.chunk = mhc, model, data, chunk
        n = self.n = data.size
        d_data = mhc.DeviceBuffer(n + 32, init=np.concatenate([data, np.zeros(32, dtype=np.uint8)]))
        cap = lib.mh_encode_bound(model.handle, n) + 64
        self.d_payload = mhc.DeviceBuffer(cap)
        d_nbits = mhc.DeviceBuffer(8, init=np.zeros(1, dtype=np.uint64))
        self.nidx = (n + chunk - 1) // chunk
        self.d_index = mhc.DeviceBuffer(max(self.nidx, 1) * 8)
        self.d_fine = mhc.DeviceBuffer(max((n + 63) // 64, 1) * 4) if chunk <= 1024 else None
        wsb = lib.mh_dev_encode_workspace(n)
        d_ws = mhc.DeviceBuffer(wsb + 64)
        mhc._check(lib.mh_dev_encode_ctx_fine(model.handle, d_data.ptr, n, CTX0, None, self.d_payload.ptr, cap, d_nbits.ptr,
                                              self.d_index.ptr, chunk, self.d_fine.ptr if self.d_fine else None, d_ws.ptr, wsb, None),
                   "encode_ctx_fine")
        mhc._check(lib.mh_dev_status(d_ws.ptr, None), "encode status")
        self.nbits = int(d_nbits.download(np.uint64)[0])
        self.index = self.d_index.download(np.uint64)[:self.nidx]
        self.fine = self.d_fine.download(np.uint32)[:(n + 63) // 64] if self.d_fine else None
        self.payload = self.d_payload.download()[:(self.nbits + 7) // 8]


def dev_ranges(mhc, model, pl_ptr, base, nbytes, nbits, d_index_ptr, chunk, n, d_fine_ptr, ranges, out_at=None, out_cap=None):
    """One mh_dev_decode_ranges_o2 call.  Returns (call status, mh_dev_status, per-range status, output bytes, out_at) and checks
    that nothing was written outside the outputs of the ranges that passed the count kernel."""
    lib = mhc.lib()
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    k = rg.shape[0]
    b, e = rg[:, 0].astype(np.int64), rg[:, 1].astype(np.int64)
    valid = (b <= e) & (e <= n)
    lens = np.where(valid, e - b, 0)
    if out_at is None:                                    # packed with odd gaps: outputs start at every byte alignment
        out_at = np.concatenate([[0], np.cumsum(lens + 3)[:-1]]).astype(np.uint64) if k else np.zeros(0, np.uint64)
    out_at = np.ascontiguousarray(out_at, dtype=np.uint64)
    if out_cap is None:
        out_cap = int(np.max(out_at.astype(np.int64) + lens)) if k else 0
    d_out = mhc.DeviceBuffer(out_cap + 2 * GUARD + 64, init=np.full(out_cap + 2 * GUARD + 64, FILL, dtype=np.uint8))
    d_rg = mhc.DeviceBuffer(max(rg.nbytes, 16), init=rg if k else None)
    d_at = mhc.DeviceBuffer(max(out_at.nbytes, 16), init=out_at if k else None)
    d_st = mhc.DeviceBuffer(max(k, 1) * 4, init=np.full(max(k, 1), 77, dtype=np.int32))
    wsb = lib.mh_dev_decode_ranges_o2_workspace(k)
    d_ws = mhc.DeviceBuffer(wsb)
    rc = lib.mh_dev_decode_ranges_o2(model.handle, pl_ptr, base, nbytes, nbits, d_index_ptr, chunk, n, d_fine_ptr, d_rg.ptr, k,
                                     d_out.ptr.value + GUARD, d_at.ptr, out_cap, d_st.ptr, d_ws.ptr, wsb, None)
    if rc != 0:
        return rc, None, None, None, out_at
    dst = lib.mh_dev_status(d_ws.ptr, None)
    st = d_st.download(np.int32)[:k]
    full = d_out.download()
    out = full[GUARD:GUARD + out_cap]
    allowed = np.zeros(out_cap, dtype=bool)
    at = out_at.astype(np.int64)
    for j in range(k):
        if valid[j] and at[j] + lens[j] <= out_cap:
            allowed[at[j]:at[j] + lens[j]] = True
    assert np.all(full[:GUARD] == FILL) and np.all(full[GUARD + out_cap:] == FILL), "wrote outside [0, out_cap)"
    assert np.all(out[~allowed] == FILL), "wrote outside the ranges' outputs"
    return rc, dst, st, out, out_at


def check_slices(data, ranges, st, out, out_at, ok_mask=None):
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    for j, (b, e) in enumerate(rg):
        if ok_mask is not None and not ok_mask[j]:
            continue
        assert st[j] == 0, (j, b, e, st[j])
        a = int(out_at[j])
        assert np.array_equal(out[a:a + e - b], data[b:e]), (j, b, e)


def range_set(n, chunk, rng, count=3000, max_len=3000, edges=120):
    """Empty ranges and [n, n); ranges on, either side of and spanning chunk and 64-symbol piece boundaries; long ranges over
    many units; random overlapping ranges; all in random order."""
    r = [(0, 0), (0, min(1, n)), (max(n - 1, 0), n), (n, n), (0, min(n, 1 << 20))]
    marks = sorted(set(list(range(0, n + 1, chunk))[:edges] + list(range(0, n + 1, 64))[:edges] + [n - n % 64, n - n % chunk]))
    for c in marks:
        for d in (-1, 0, 1):
            x = c + d
            if 0 <= x <= n:
                r += [(x, min(x + 1, n)), (max(x - 1, 0), x), (x, min(x + 64, n)), (x, min(x + chunk, n)), (x, min(x + 2 * chunk + 7, n))]
    b = rng.integers(0, n + 1, size=count)
    e = np.minimum(b + rng.integers(0, max_len, size=count), n)
    r += list(zip(b.tolist(), e.tolist()))
    r = np.array(r, dtype=np.uint64)
    return r[rng.permutation(len(r))]


def run_all(mhc, enc, ranges, fine):
    rc, dst, st, out, at = dev_ranges(mhc, enc.model, enc.d_payload.ptr, 0, (enc.nbits + 7) // 8, enc.nbits, enc.d_index.ptr, enc.chunk,
                                      enc.n, enc.d_fine.ptr if fine else None, ranges)
    assert rc == 0 and dst == 0, (rc, dst)
    check_slices(enc.data, ranges, st, out, at)


# ---- call-level checks against an order-2 model ------------------------------------------------------------------------------
def test_device_and_host_calls_refuse_bad_arguments_before_any_launch(mhc):
    data = text_like(20_000, 1)
    m = model_o2(mhc, data)
    lib = mhc.lib()
    ws = int(lib.mh_dev_decode_ranges_o2_workspace(1))
    wbuf = np.zeros(ws + 8192, dtype=np.uint8)
    w = (wbuf.ctypes.data + 255) & ~255                   # host stand-ins: a refusal must come before any is read
    rg = np.array([0, 10], dtype=np.uint64)
    ARG, CAP = mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY
    names = ["m", "pl", "base", "bytes", "nbits", "index", "chunk", "n", "fine", "ranges", "k", "out", "out_at", "cap", "st", "ws",
             "wsb", "stream"]
    ok = [m.handle, w, 0, 64, 512, w, 256, 400, None, rg.ctypes.data, 1, w, w, 16, w, w, ws, None]

    def dev(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.mh_dev_decode_ranges_o2(*a)

    assert dev(pl=None) == ARG and dev(index=None) == ARG and dev(ws=None) == ARG and dev(ranges=None) == ARG
    assert dev(out_at=None) == ARG and dev(st=None) == ARG
    assert dev(out=w + 8) == ARG and dev(ws=w + 4) == ARG                          # misaligned output / workspace
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert dev(chunk=bad_chunk) == ARG, bad_chunk
    assert dev(n=513) == ARG                                                       # n_symbols > nbits
    assert dev(base=60, bytes=8) == ARG                                            # window past the payload
    assert dev(fine=w, chunk=2048) == ARG                                          # no order-2 fine index over 1024 symbols
    assert dev(fine=w + 2) == ARG                                                  # misaligned fine index
    assert dev(wsb=64) == CAP
    # the batch device call
    po, nb, so = np.array([0, 16, 32], dtype=np.uint64), np.array([120, 128], dtype=np.uint64), np.array([0, 100, 200], dtype=np.uint64)
    lk = np.array([0, 0, 10], dtype=np.uint64)
    bnames = ["m", "pl", "po", "nb", "n", "prev0", "so", "index", "chunk", "lk", "k", "out", "out_at", "cap", "st", "ws", "wsb", "stream"]
    bok = [m.handle, w, po.ctypes.data, nb.ctypes.data, 2, 0x20, so.ctypes.data, w, 256, lk.ctypes.data, 1, w, w, 64, w, w, ws, None]

    def bdev(**kw):
        a = list(bok)
        for k, v in kw.items():
            a[bnames.index(k)] = v
        return lib.mh_dev_decode_batch_o2_ranges(*a)

    assert bdev(po=None) == ARG and bdev(pl=None) == ARG and bdev(pl=w + 4) == ARG and bdev(out=w + 8) == ARG
    assert bdev(lk=None) == ARG and bdev(out_at=None) == ARG and bdev(st=None) == ARG and bdev(so=None) == ARG
    for bad_chunk in (0, 100, 128, 16384):
        assert bdev(chunk=bad_chunk) == ARG
    assert bdev(wsb=64) == CAP
    # the host forms: call-level checks, then every lookup against the buffers' lengths
    off, st = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int32)
    assert lib.mh_decode_ranges_o2(m.handle, w, 512, w, 300, 400, rg.ctypes.data, 1, w, 64, off.ctypes.data, st.ctypes.data) == ARG
    assert lib.mh_decode_ranges_o2(m.handle, w, 512, w, 256, 513, rg.ctypes.data, 1, w, 64, off.ctypes.data, st.ctypes.data) == ARG
    assert lib.mh_decode_ranges_o2(m.handle, w, 512, None, 256, 400, rg.ctypes.data, 1, w, 64, off.ctypes.data, st.ctypes.data) == ARG
    pl = np.zeros(32, dtype=np.uint8)
    res, sts = m.decode_batch_o2_ranges(pl, po, nb, [(2, 0, 1), (0, 5, 4), (0, 0, 101), (1, 3, 3)], sym_off=so,
                                        index=np.zeros(4, dtype=np.uint64), chunk_symbols=256)
    assert list(sts) == [ARG, ARG, ARG, MH_OK] and res == [b"", b"", b"", b""]
    res, sts = m.decode_batch_o2_ranges(pl, np.array([0, 16, 40], dtype=np.uint64), nb, [(1, 0, 10)])   # stream 1 past the payload
    assert list(sts) == [ARG]


# ---- byte-exact ranges of one stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN5)
def test_golden_ranges_every_chunk_size(mhc, name):
    data = np.frombuffer(golden()[name]["data"], dtype=np.uint8)
    model = model_o2(mhc, data)
    rng = np.random.default_rng(len(data))
    for chunk in (256, 512, 1024, 4096):
        enc = Enc(mhc, model, data, chunk)
        ranges = range_set(data.size, chunk, rng)
        for fine in ((False, True) if chunk <= 1024 else (False,)):
            run_all(mhc, enc, ranges, fine)


@pytest.mark.parametrize("kind", ["zipf", "uniform", "text64m"])
def test_sources_ranges(mhc, kind):
    data = {"zipf": lambda: zipf_bytes(2 << 20, 3), "uniform": lambda: np.random.default_rng(4).integers(0, 256, 1 << 20).astype(np.uint8),
            "text64m": lambda: text_like(64 << 20, 5)}[kind]()
    model = model_o2(mhc, data)
    rng = np.random.default_rng(7)
    chunks = (1024,) if kind == "text64m" else (256, 1024, 4096)
    for chunk in chunks:
        enc = Enc(mhc, model, data, chunk)
        ranges = range_set(data.size, chunk, rng, count=20_000 if kind == "text64m" else 3000)
        for fine in ((False, True) if chunk <= 1024 else (False,)):
            run_all(mhc, enc, ranges, fine)
    if kind == "text64m":                                 # one range over the whole stream
        run_all(mhc, enc, np.array([[0, data.size]], dtype=np.uint64), True)


@pytest.fixture(scope="module")
def wiki(mhc):
    data = np.frombuffer(golden()["input_wiki_cpp.html"]["data"], dtype=np.uint8)
    model = model_o2(mhc, data)
    return Enc(mhc, model, data, 1024)


def test_payload_window_at_every_alignment(mhc, wiki):
    enc, chunk, data = wiki, 1024, wiki.data
    c0, c1 = 20, 40                                      # chunks whose payload bytes are uploaded
    lo = int(enc.index[c0] & POS2) >> 3
    hi = (int(enc.index[c1 + 1] & POS2) + 7) >> 3
    inside = [(c0 * chunk, (c1 + 1) * chunk), (c0 * chunk + 17, c0 * chunk + 18), ((c0 + 3) * chunk - 5, (c0 + 9) * chunk + 1000),
              (c1 * chunk + 1, (c1 + 1) * chunk), ((c0 + 5) * chunk + 64, (c0 + 5) * chunk + 128), ((c0 + 7) * chunk, (c0 + 7) * chunk)]
    # (the second one reads 40 symbols of chunk c1 + 1: more than the bits of the window's last byte)
    outside = [(c0 * chunk - 1, c0 * chunk + 10), ((c1 + 1) * chunk - 3, (c1 + 1) * chunk + 40), (0, 100)]
    for shift in (0, 1, 2, 3):
        win = np.concatenate([np.full(shift, 0xCC, dtype=np.uint8), enc.payload[lo:hi], np.zeros(16, dtype=np.uint8)])
        d_win = mhc.DeviceBuffer(win.size, init=win)
        for fine in (None, enc.d_fine.ptr):
            rc, dst, st, out, at = dev_ranges(mhc, enc.model, d_win.ptr.value + shift, lo, hi - lo, enc.nbits, enc.d_index.ptr, chunk,
                                              enc.n, fine, inside + outside)
            assert rc == 0
            check_slices(data, inside, st, out, at)
            assert list(st[len(inside):]) == [mhc.MH_ERR_ARG] * len(outside), (shift, fine)
            assert dst == mhc.MH_ERR_ARG


def test_per_range_errors_and_capacity_leave_the_others_exact(mhc, wiki):
    enc = wiki
    n = enc.n
    good = range_set(n, 1024, np.random.default_rng(5), count=1000)
    bad = np.array([(10, 5), (n - 3, n + 1), (0, n + 100)], dtype=np.uint64)
    ranges = np.concatenate([good, bad])
    b, e = ranges[:, 0].astype(np.int64), ranges[:, 1].astype(np.int64)
    lens = np.where((b <= e) & (e <= n), e - b, 0)
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    cap = int(at[-1] + lens[-1])
    ranges = np.concatenate([ranges, np.array([[100, 200]], dtype=np.uint64)])
    at = np.concatenate([at, [cap - 50]]).astype(np.uint64)          # reaches 50 bytes past out_cap
    for fine in (None, enc.d_fine.ptr):
        rc, dst, st, out, at2 = dev_ranges(mhc, enc.model, enc.d_payload.ptr, 0, len(enc.payload), enc.nbits, enc.d_index.ptr, 1024, n,
                                           fine, ranges, out_at=at, out_cap=cap)
        assert rc == 0
        check_slices(enc.data, good, st, out, at2)
        assert list(st[len(good):]) == [mhc.MH_ERR_ARG] * 3 + [mhc.MH_ERR_CAPACITY]
        assert dst in (mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY)


# ---- the fine index ------------------------------------------------------------------------------------------------------------
def test_fine_index_entries_that_do_not_fit_fall_back(mhc, wiki):
    enc = wiki
    ranges = range_set(enc.n, 1024, np.random.default_rng(8), count=2000)
    none = np.full(enc.fine.size, 0xFFFF, dtype=np.uint32) | (enc.fine & np.uint32(0xFFFF0000))
    half = enc.fine.copy()
    half[1::2] = none[1::2]                                # every other piece unusable
    for fine in (none, half):
        d_fine = mhc.DeviceBuffer(fine.nbytes, init=fine)
        rc, dst, st, out, at = dev_ranges(mhc, enc.model, enc.d_payload.ptr, 0, len(enc.payload), enc.nbits, enc.d_index.ptr, 1024,
                                          enc.n, d_fine.ptr, ranges)
        assert rc == 0 and dst == 0
        check_slices(enc.data, ranges, st, out, at)


def test_fine_entry_out_of_its_chunk_fails_exactly_the_ranges_that_read_it(mhc, wiki):
    enc = wiki
    n, chunk = enc.n, 1024
    c = 30
    q = c * 16 + 5                                        # a piece inside chunk c
    span = int(enc.index[c + 1] & POS2) - int(enc.index[c] & POS2)
    assert span + 9 < 0xFFFF
    fine = enc.fine.copy()
    fine[q] = (fine[q] & np.uint32(0xFFFF0000)) | np.uint32(span + 9)    # past the next chunk's entry
    d_fine = mhc.DeviceBuffer(fine.nbytes, init=fine)
    rng = np.random.default_rng(9)
    s = q * 64
    ranges = list(map(tuple, range_set(n, chunk, rng, count=2000).tolist()))
    ranges += [(s, s + 1), (s - 1, s), (s - 64, s), (s + 63, s + 64), (s + 64, s + 65), (s - 10, s + 200), (c * chunk, (c + 1) * chunk),
               (s + 1, s + 1)]
    rg = np.array(ranges, dtype=np.uint64)

    def reads(b, e):
        return b < e and ((b // 64 <= q <= (e - 1) // 64) or e == s)

    want = np.array([reads(int(b), int(e)) for b, e in rg])
    assert want.any() and not want.all()
    rc, dst, st, out, at = dev_ranges(mhc, enc.model, enc.d_payload.ptr, 0, len(enc.payload), enc.nbits, enc.d_index.ptr, chunk, n,
                                      d_fine.ptr, rg)
    assert rc == 0 and dst == mhc.MH_ERR_CORRUPT
    assert np.array_equal(st == mhc.MH_ERR_CORRUPT, want)
    check_slices(enc.data, rg, st, out, at, ok_mask=~want)


# ---- the host form -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_text(mhc):
    data = text_like(64 << 20, 12)
    model = model_o2(mhc, data)
    pl, nbits, idx = model.encode(data, chunk_symbols=1024)
    return model, data, pl, nbits, idx


def test_host_form_one_4k_range_uploads_a_few_chunks(mhc, big_text):
    model, data, pl, nbits, idx = big_text
    b = 40_000_000 + 333
    outs, st = model.decode_ranges_o2(pl, nbits, idx, 1024, data.size, [(b, b + 4096)])
    assert list(st) == [0] and outs[0] == data[b:b + 4096].tobytes()
    up = mhc.lib().mh_last_range_upload_bytes()
    c0, c1 = b // 1024, (b + 4095) // 1024
    span = ((int(idx[c1 + 1] & np.uint64(POS2)) + 7) >> 3) - (int(idx[c0] & np.uint64(POS2)) >> 3)
    assert 0 < up == span and up <= 6 * 1024 and up < len(pl) // 1000


def test_host_form_many_ranges_and_segment_cuts(mhc, big_text, monkeypatch):
    model, data, pl, nbits, idx = big_text
    rng = np.random.default_rng(4)
    n = data.size
    b = rng.integers(0, n, size=5000)
    e = np.minimum(b + rng.integers(0, 5000, size=5000), n)
    ranges = list(zip(b.tolist(), e.tolist())) + [(n, n), (0, 1), (n - 1, n), (n // 3, n // 3 + 3_000_000), (5, 3), (0, n + 1)]
    for seg in (None, 64 << 10):
        if seg:
            monkeypatch.setenv("MH_SEGMENT_BYTES", str(seg))
        outs, st = model.decode_ranges_o2(pl, nbits, idx, 1024, n, ranges)
        assert list(st[-2:]) == [mhc.MH_ERR_ARG] * 2 and outs[-2:] == [b"", b""]
        for j, (x, y) in enumerate(ranges[:-2]):
            assert st[j] == 0 and outs[j] == data[x:y].tobytes(), (seg, j)


# ---- damaged streams -------------------------------------------------------------------------------------------------------
def expect(got, want, what):
    assert got[0] == want[0], "%s: status %d, contract %d" % (what, got[0], want[0])
    if want[0] == MH_OK:
        assert got[1] == want[1], "%s: bytes differ" % what


def test_damaged_stream_ranges_follow_the_contract(mhc, oracle):
    """mh_decode_ranges_o2 with the chunk index alone: every range's status and bytes are damage.verdict_range(order=2)."""
    data = text_like(200_000, 7)
    om = oracle.Model.from_data(data.tobytes(), 2)
    blob, nbits = om.compress(data.tobytes())
    payload = blob[1:]
    m = mhc.Model.from_table(om.table_bytes())
    lens = np.asarray(om.codes_o2()[0])
    chunk, n = 1024, data.size
    bounds = damage.boundaries(lens, data, 2, CTX0)
    code_len = damage.code_lengths(lens, data, 2, CTX0)
    index, _ = damage.expected_entries(lens, data, chunk, CTX0, 2)
    offs = (index & np.uint64(POS2)).astype(np.int64)
    cases = damage.all_damages(payload, nbits, bounds, code_len, offs, seed=3, per_kind=1, kmax=6)
    ranges = [(0, 100), (chunk - 10, chunk + 10), (n // 2, n // 2 + 3 * chunk), (n - 5, n), (n - chunk - 1, n - 1), (n - 1, n), (7, 7),
              (n - chunk, n), (0, n)]
    seen_fail = False
    for name, pl, nb in [("intact", payload, nbits)] + cases:
        if nb < n:                                         # fewer bits than symbols: refused before any decode
            with pytest.raises(mhc.MhError) as e:
                m.decode_ranges_o2(pl, nb, index, chunk, n, ranges)
            assert e.value.status == mhc.MH_ERR_ARG, name
            continue
        res, status = m.decode_ranges_o2(pl, nb, index, chunk, n, ranges)
        for (b, e), got, st in zip(ranges, res, status):
            want = damage.verdict_range(om, pl, nb, index, chunk, n, b, e, order=2)
            seen_fail |= want[0] != MH_OK
            expect((int(st), got), want, "range [%d, %d) %s" % (b, e, name))
    assert seen_fail


# ---- lookups into batches ----------------------------------------------------------------------------------------------------
def lines_of(name):
    """The golden input cut into lines (newline kept), with empty messages in between."""
    data = golden()[name]["data"]
    msgs = []
    for k, line in enumerate(data.split(b"\n")):
        msgs.append(line + b"\n")
        if k % 97 == 0:
            msgs.append(b"")
    return msgs


def lookup_set(msgs, rng, count=3000):
    lk = []
    for i, m in enumerate(msgs[:400]):
        n = len(m)
        lk += [(i, 0, n), (i, n, n), (i, n // 2, n), (i, 0, min(n, 3))]
    ln = np.array([len(m) for m in msgs])
    s = rng.integers(0, len(msgs), size=count)
    b = (rng.random(count) * (ln[s] + 1)).astype(np.int64)
    e = np.minimum(b + rng.integers(0, 300, size=count), ln[s])
    lk += list(zip(s.tolist(), b.tolist(), e.tolist()))
    return np.array(lk, dtype=np.uint64)[rng.permutation(len(lk))]


def check_lookups(msgs, lk, res, st):
    for (i, b, e), got, s in zip(lk.tolist(), res, st):
        assert s == 0 and got == msgs[i][b:e], (i, b, e, s)


@pytest.mark.parametrize("name", GOLDEN5)
def test_golden_lines_lookups(mhc, name):
    msgs = lines_of(name)
    m = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
    chunk = 256
    payload, pay_off, nbits, idx, in_off = m.encode_batch_o2(msgs, chunk_symbols=chunk)
    lk = lookup_set(msgs, np.random.default_rng(len(msgs)))
    for kw in (dict(sym_off=in_off, index=idx, chunk_symbols=chunk), dict(sym_off=in_off), {}):
        res, st, dst = m.dev_decode_batch_o2_ranges(payload, pay_off, nbits, lk, **kw)
        assert dst == 0
        check_lookups(msgs, lk, res, st)
        res, st = m.decode_batch_o2_ranges(payload, pay_off, nbits, lk, **kw)
        check_lookups(msgs, lk, res, st)
    # whole .cm files of compress_batch_o2
    blobs = m.compress_batch_o2(msgs, chunk_symbols=chunk)
    res, st = m.decompress_batch_o2_ranges([b for b, _, _ in blobs], lk, indices=[s for _, _, s in blobs], chunk_symbols=chunk,
                                           lengths=[len(x) for x in msgs])
    check_lookups(msgs, lk, res, st)


def test_index_free_stream_over_the_walk_cap(mhc):
    msgs = [text_like(3000, 1).tobytes(), text_like(4 << 20, 2).tobytes(), b"", text_like(777, 3).tobytes()]
    m = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
    payload, pay_off, nbits, idx, in_off = m.encode_batch_o2(msgs, chunk_symbols=1024)
    assert int(nbits[1]) > mhc.BATCH_WALK_MAX_BITS and int(nbits[0]) < mhc.BATCH_WALK_MAX_BITS
    lk = np.array([(0, 5, 900), (1, 3_000_000, 3_000_300), (3, 0, 777), (1, 10, 10), (2, 0, 0)], dtype=np.uint64)
    res, st, dst = m.dev_decode_batch_o2_ranges(payload, pay_off, nbits, lk)
    assert list(st) == [MH_OK, mhc.MH_ERR_ARG, MH_OK, MH_OK, MH_OK] and dst == mhc.MH_ERR_ARG
    assert res[0] == msgs[0][5:900] and res[2] == msgs[3]
    for kw in ({}, dict(sym_off=in_off), dict(sym_off=in_off, index=idx, chunk_symbols=1024)):
        res, st = m.decode_batch_o2_ranges(payload, pay_off, nbits, lk, **kw)
        check_lookups(msgs, lk, res, st)
        assert mhc.last_batch_range_upload_bytes() > 0


class Batch2:
    """Five order-2 streams of one oracle model (every message counted from its own start context), with their index
    slices; stream `at` replaced by a damage."""

    def __init__(self, mhc, oracle, chunk=1024):
        self.mhc, self.chunk = mhc, chunk
        msgs = [text_like(k, 40 + k) for k in (30_000, 5_000, 60_000, 700, 45_000)]
        self.msgs = [x.tobytes() for x in msgs]
        counts = sum(oracle.histogram_o2(x).astype(np.uint64) for x in self.msgs)
        self.om = oracle.Model.from_counts(counts, 2)
        self.m = mhc.Model.from_table(self.om.table_bytes())
        lens = np.asarray(self.om.codes_o2()[0])
        self.streams = []
        for x in msgs:
            blob, nb = self.om.compress(x.tobytes())
            idx, _ = damage.expected_entries(lens, x, chunk, CTX0, 2)
            self.streams.append((blob[1:], nb, idx, damage.boundaries(lens, x, 2, CTX0), damage.code_lengths(lens, x, 2, CTX0)))

    def pack(self, at, pl, nb):
        pls = [s[0] for s in self.streams]
        nbs = [s[1] for s in self.streams]
        pls[at], nbs[at] = pl, nb
        payload, pay_off = self.mhc.batch_offsets(pls)
        sym_off = np.zeros(len(self.msgs) + 1, dtype=np.uint64)
        sym_off[1:] = np.cumsum([len(x) for x in self.msgs])
        l = self.mhc.lib()
        index = np.zeros(max(l.mh_batch_index_capacity(int(sym_off[-1]), len(self.msgs), self.chunk), 1), dtype=np.uint64)
        for i, s in enumerate(self.streams):
            base = l.mh_batch_index_base(int(sym_off[i]), i, self.chunk)
            index[base:base + s[2].size] = s[2]
        return payload, pay_off, np.array(nbs, dtype=np.uint64), sym_off, index


def walk_verdict(om, pl, nb, n_i, b, e):
    """An index-free lookup with sym_off given: the walk from bit 0 in context (0x20, 0x20) (damage.verdict_free's strict
    decode) must reach `end` without a null entry or a code past nbits; a lookup that ends at n_i must end exactly at nbits;
    a stream that ends before `end` is MH_ERR_ARG."""
    if b == e:
        return MH_OK, b""
    rc, out, ns, _ = om.decode_span(pl, 0, nb, CTX0)
    if rc == 0 and e > ns:
        return -1, None                                     # MH_ERR_ARG: the stream ends before `end`
    if e > ns or (e == n_i and (rc != 0 or ns != n_i)):
        return MH_ERR_CORRUPT, None
    return MH_OK, out[b:e]


def test_damaged_batch_lookups_follow_the_contract(mhc, oracle):
    bt = Batch2(mhc, oracle)
    assert mhc.MH_ERR_ARG == -1
    for j, at in enumerate((0, 2, 4)):
        pl0, nb0, idx0, bounds, cl = bt.streams[at]
        offs = (idx0 & np.uint64(POS2)).astype(np.int64)
        for name, pl, nb in damage.all_damages(pl0, nb0, bounds, cl, offs, seed=30 + j, per_kind=1, kmax=6):
            payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
            lookups = []
            for i, msg in enumerate(bt.msgs):
                n = len(msg)
                lookups += [(i, 0, n), (i, 0, min(10, n)), (i, n // 2, n), (i, max(n - 3, 0), n - 1), (i, min(1500, n), min(1600, n))]
            lk = np.array(lookups, dtype=np.uint64)
            # indexed, through the host form and the device form
            res, st = bt.m.decode_batch_o2_ranges(payload, pay_off, nbits, lk, sym_off=sym_off, index=index, chunk_symbols=bt.chunk)
            dres, dst_, _ = bt.m.dev_decode_batch_o2_ranges(payload, pay_off, nbits, lk, sym_off=sym_off, index=index, chunk_symbols=bt.chunk)
            for (i, b, e), got, s, dgot, ds in zip(lookups, res, st, dres, dst_):
                spl, snb, sidx = (pl, nb, idx0) if i == at else bt.streams[i][:3]
                want = damage.verdict_range(bt.om, spl, snb, sidx, bt.chunk, len(bt.msgs[i]), b, e, order=2)
                expect((int(s), got), want, "indexed lookup (%d, %d, %d) %s" % (i, b, e, name))
                expect((int(ds), dgot), want, "device indexed lookup (%d, %d, %d) %s" % (i, b, e, name))
            # index-free, with the lengths
            dres, dst_, _ = bt.m.dev_decode_batch_o2_ranges(payload, pay_off, nbits, lk, sym_off=sym_off)
            for (i, b, e), dgot, ds in zip(lookups, dres, dst_):
                spl, snb = (pl, nb) if i == at else bt.streams[i][:2]
                want = walk_verdict(bt.om, spl, snb, len(bt.msgs[i]), b, e)
                expect((int(ds), dgot), want, "index-free lookup (%d, %d, %d) %s" % (i, b, e, name))
