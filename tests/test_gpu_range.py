"""Byte ranges of one indexed stream on the GPU (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM").  Ground truth:
the golden inputs, sliced with numpy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT, expected_file, golden

pytestmark = pytest.mark.gpu

GOLDEN5 = ["input_a.txt", "input_b.txt", "input_ipsum.txt", "input_wiki_cpp.html", "input_wiki_cpp.txt"]
GUARD = 64
FILL = 0xA5


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


class Enc:
    """A stream encoded on the device with its chunk index and fine index (mh_dev_encode_fine)."""

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
        self.d_fine = mhc.DeviceBuffer(max((n + 63) // 64, 1) * 4)
        wsb = lib.mh_dev_encode_workspace(n)
        d_ws = mhc.DeviceBuffer(wsb)
        mhc._check(lib.mh_dev_encode_fine(model.handle, d_data.ptr, n, 0x20, None, self.d_payload.ptr, cap, d_nbits.ptr,
                                          self.d_index.ptr, chunk, self.d_fine.ptr, None, 0, d_ws.ptr, wsb, None), "encode_fine")
        mhc._check(lib.mh_dev_status(d_ws.ptr, None), "encode status")
        self.nbits = int(d_nbits.download(np.uint64)[0])
        self.index = self.d_index.download(np.uint64)[:self.nidx]
        self.payload = self.d_payload.download()[:(self.nbits + 7) // 8]


def dev_ranges(mhc, model, pl_ptr, base, nbytes, nbits, d_index_ptr, chunk, n, d_fine_ptr, ranges, out_at=None, out_cap=None):
    """One mh_dev_decode_ranges call.  Returns (call status, mh_dev_status, per-range status, output bytes, out_at, out_cap)
    and checks that nothing was written outside the outputs of the ranges that passed the count kernel."""
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
    wsb = lib.mh_dev_decode_ranges_workspace(k)
    d_ws = mhc.DeviceBuffer(wsb)
    rc = lib.mh_dev_decode_ranges(model.handle, pl_ptr, base, nbytes, nbits, d_index_ptr, chunk, n, d_fine_ptr, d_rg.ptr, k,
                                  d_out.ptr.value + GUARD, d_at.ptr, out_cap, d_st.ptr, d_ws.ptr, wsb, None)
    if rc != 0:
        return rc, None, None, None, out_at, out_cap
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
    return rc, dst, st, out, out_at, out_cap


def check_slices(data, ranges, st, out, out_at, ok_mask=None):
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    for j, (b, e) in enumerate(rg):
        if ok_mask is not None and not ok_mask[j]:
            continue
        assert st[j] == 0, (j, b, e, st[j])
        a = int(out_at[j])
        assert np.array_equal(out[a:a + e - b], data[b:e]), (j, b, e)


def range_set(n, chunk, rng, count=10_000):
    """Edge ranges, chunk boundaries +-1, ranges over 1, 2 and many chunks, and random overlapping ranges in random order."""
    r = [(0, 0), (0, min(1, n)), (max(n - 1, 0), n), (n, n), (0, n)]
    for c in range(0, n + 1, chunk)[:250]:
        for d in (-1, 0, 1):
            x = c + d
            if 0 <= x <= n:
                r += [(x, min(x + 1, n)), (max(x - 1, 0), x), (x, min(x + chunk, n)), (x, min(x + 2 * chunk, n))]
    for span in (1, 2, 7):
        b = min(n // 3, n)
        r.append((b, min(b + span * chunk + 5, n)))
    b = rng.integers(0, n + 1, size=count)
    ln = np.where(rng.random(count) < 0.8, rng.integers(0, 300, size=count), rng.integers(0, max(n // 4, 1) + 1, size=count))
    e = np.minimum(b + ln, n)
    r += list(zip(b.tolist(), e.tolist()))
    r = np.array(r, dtype=np.uint64)
    return r[rng.permutation(len(r))]


def run_all(mhc, model, enc, ranges, fine):
    rc, dst, st, out, at, _ = dev_ranges(mhc, model, enc.d_payload.ptr, 0, (enc.nbits + 7) // 8, enc.nbits, enc.d_index.ptr,
                                         enc.chunk, enc.n, enc.d_fine.ptr if fine else None, ranges)
    assert rc == 0 and dst == 0
    check_slices(enc.data, ranges, st, out, at)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("name", GOLDEN5)
def test_golden_ranges_every_chunk_size(mhc, name, order):
    data = np.frombuffer(golden()[name]["data"], dtype=np.uint8)
    model = mhc.Model.from_table(expected_file(name, "e" if order else "eh"))
    assert model.type == order
    rng = np.random.default_rng(len(data) + order)
    for chunk in (256, 1024, 8192):
        enc = Enc(mhc, model, data, chunk)
        ranges = range_set(data.size, chunk, rng)
        for fine in (False, True):
            run_all(mhc, model, enc, ranges, fine)


def test_long_codes_in_skipped_and_stored_symbols(mhc):
    """Fibonacci-weighted counts: codes well over 12 and 16 bits, so the second table level and the tree walk run inside the
    symbols a lane skips and the ones it stores."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    row = np.ones(256, dtype=np.uint64)
    row[:40] = np.array(fib[::-1], dtype=np.uint64)
    model = mhc.Model.from_counts(np.tile(row, 256), 1)
    assert model.max_code_len > 16
    rng = np.random.default_rng(3)
    data = np.concatenate([rng.integers(0, 256, size=150_000), rng.integers(0, 40, size=50_000)]).astype(np.uint8)
    lens = np.frombuffer(model.image(1), dtype=np.uint8)
    assert lens[data[1:].astype(np.int64)].max() > 16                               # long codes occur in the stream
    for chunk in (256, 4096):
        enc = Enc(mhc, model, data, chunk)
        ranges = range_set(data.size, chunk, rng, count=3000)
        for fine in (False, True):
            run_all(mhc, model, enc, ranges, fine)


@pytest.mark.parametrize("name", ["input_ipsum.txt", "input_wiki_cpp.html"])
def test_reference_stream_without_index_gets_one_first(mhc, name):
    data = np.frombuffer(golden()[name]["data"], dtype=np.uint8)
    cm = expected_file(name, "cm")
    lib = mhc.lib()
    model = mhc.Model.from_table(expected_file(name, "e"))
    nb = ctypes.c_uint64()
    mhc._check(lib.mh_stream_parse_header(model.handle, cm[0], len(cm), ctypes.byref(nb)), "header")
    nbits, pl = nb.value, np.frombuffer(cm[1:], dtype=np.uint8)
    d_pl = mhc.DeviceBuffer(pl.size + 64, init=np.concatenate([pl, np.zeros(64, dtype=np.uint8)]))
    chunk = 1024
    icap, fcap = nbits // chunk + 2, nbits // 64 + 2
    d_idx, d_fine, d_ns = mhc.DeviceBuffer(icap * 8), mhc.DeviceBuffer(fcap * 4), mhc.DeviceBuffer(8)
    iws = int(lib.mh_dev_build_index_workspace(nbits))
    d_iws = mhc.DeviceBuffer(iws)
    mhc._check(lib.mh_dev_build_index_fine(model.handle, d_pl.ptr, nbits, 0x20, d_idx.ptr, icap, chunk, d_fine.ptr, fcap, d_ns.ptr,
                                           d_iws.ptr, iws, None), "build_index_fine")
    mhc._check(lib.mh_dev_status(d_iws.ptr, None), "build_index status")
    n = int(d_ns.download(np.uint64)[0])
    assert n == data.size
    ranges = range_set(n, chunk, np.random.default_rng(11), count=4000)
    for fine in (None, d_fine.ptr):
        rc, dst, st, out, at, _ = dev_ranges(mhc, model, d_pl.ptr, 0, pl.size, nbits, d_idx.ptr, chunk, n, fine, ranges)
        assert rc == 0 and dst == 0
        check_slices(data, ranges, st, out, at)


def test_payload_window_only_middle_bytes_uploaded(mhc):
    data = np.frombuffer(golden()["input_wiki_cpp.html"]["data"], dtype=np.uint8)
    model = mhc.Model.from_table(expected_file("input_wiki_cpp.html", "e"))
    chunk = 1024
    enc = Enc(mhc, model, data, chunk)
    c0, c1 = 100, 140                                    # chunks whose payload bytes are uploaded
    lo = int(enc.index[c0] & mhc.INDEX_BIT_MASK) >> 3
    hi = (int(enc.index[c1 + 1] & mhc.INDEX_BIT_MASK) + 7) >> 3
    for shift in (0, 3):                                 # the window may start at any alignment
        win = np.concatenate([np.full(shift, 0xCC, dtype=np.uint8), enc.payload[lo:hi], np.zeros(16, dtype=np.uint8)])
        d_win = mhc.DeviceBuffer(win.size, init=win)
        inside = [(c0 * chunk, (c1 + 1) * chunk), (c0 * chunk + 17, c0 * chunk + 18), ((c0 + 3) * chunk - 5, (c0 + 9) * chunk + 1000),
                  (c1 * chunk + 1, (c1 + 1) * chunk), ((c0 + 20) * chunk, (c0 + 20) * chunk)]
        outside = [(c0 * chunk - 1, c0 * chunk + 10), ((c1 + 1) * chunk - 3, (c1 + 1) * chunk + 2), (0, 100)]
        ranges = inside + outside
        for fine in (None, enc.d_fine.ptr):
            rc, dst, st, out, at, _ = dev_ranges(mhc, model, d_win.ptr.value + shift, lo, hi - lo, enc.nbits, enc.d_index.ptr, chunk,
                                                 enc.n, fine, ranges)
            assert rc == 0
            check_slices(data, inside, st, out, at)
            assert list(st[len(inside):]) == [mhc.MH_ERR_ARG] * len(outside)
            assert dst == mhc.MH_ERR_ARG


def test_per_range_errors_leave_the_others_exact(mhc):
    data = np.frombuffer(golden()["input_wiki_cpp.html"]["data"], dtype=np.uint8)
    model = mhc.Model.from_table(expected_file("input_wiki_cpp.html", "e"))
    chunk = 1024
    enc = Enc(mhc, model, data, chunk)
    n, nbits = enc.n, enc.nbits
    rng = np.random.default_rng(5)
    good = range_set(n, chunk, rng, count=2000)
    # argument errors and a capacity error, each for its range only
    bad = np.array([(10, 5), (n - 3, n + 1), (0, n + 100)], dtype=np.uint64)
    ranges = np.concatenate([good, bad])
    k = len(ranges)
    b, e = ranges[:, 0].astype(np.int64), ranges[:, 1].astype(np.int64)
    lens = np.where((b <= e) & (e <= n), e - b, 0)
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    cap = int(at[-1] + lens[-1])
    cap_range = np.array([[100, 200]], dtype=np.uint64)
    ranges = np.concatenate([ranges, cap_range])
    at = np.concatenate([at, [cap - 50]]).astype(np.uint64)          # reaches 50 bytes past out_cap
    rc, dst, st, out, at, _ = dev_ranges(mhc, model, enc.d_payload.ptr, 0, len(enc.payload), nbits, enc.d_index.ptr, chunk, n,
                                         None, ranges, out_at=at, out_cap=cap)
    assert rc == 0
    check_slices(data, good, st, out, at)
    assert list(st[len(good):]) == [mhc.MH_ERR_ARG] * 3 + [mhc.MH_ERR_CAPACITY]
    assert dst in (mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY)


@pytest.mark.parametrize("kind", ["past_nbits", "behind_predecessor"])
def test_corrupt_index_entries_fail_only_the_ranges_on_them(mhc, kind):
    data = np.frombuffer(golden()["input_wiki_cpp.html"]["data"], dtype=np.uint8)
    model = mhc.Model.from_table(expected_file("input_wiki_cpp.html", "e"))
    chunk = 1024
    enc = Enc(mhc, model, data, chunk)
    n, nbits = enc.n, enc.nbits
    idx = enc.index.copy()
    k = 150
    ctx = idx[k] & ~np.uint64(mhc.INDEX_BIT_MASK)
    pos = nbits + 12345 if kind == "past_nbits" else int(idx[k - 1] & mhc.INDEX_BIT_MASK) - 9
    idx[k] = ctx | np.uint64(pos)
    d_idx = mhc.DeviceBuffer(idx.nbytes, init=idx)
    s = (idx & np.uint64(mhc.INDEX_BIT_MASK)).astype(np.int64)
    bad_units = {u for u in range(len(s)) if s[u] > nbits or (u > 0 and s[u] < s[u - 1])}
    assert k in bad_units
    rng = np.random.default_rng(9)
    ranges = list(map(tuple, range_set(n, chunk, rng, count=3000).tolist()))
    ranges += [(k * chunk - 10, k * chunk), ((k - 1) * chunk, k * chunk), (k * chunk, k * chunk + 1), ((k + 1) * chunk, (k + 1) * chunk + 5),
               ((k - 1) * chunk + 1, k * chunk - 1)]
    rg = np.array(ranges, dtype=np.uint64)

    def expect_corrupt(b, e):
        if b >= e:
            return False
        units = set(range(b // chunk, (e - 1) // chunk + 1))
        return bool(units & bad_units) or (e % chunk == 0 and e < n and e // chunk in bad_units)

    want = np.array([expect_corrupt(int(b), int(e)) for b, e in rg])
    assert want.any() and not want.all()
    rc, dst, st, out, at, _ = dev_ranges(mhc, model, enc.d_payload.ptr, 0, len(enc.payload), nbits, d_idx.ptr, chunk, n, None, rg)
    assert rc == 0
    assert np.array_equal(st == mhc.MH_ERR_CORRUPT, want)
    check_slices(data, rg, st, out, at, ok_mask=~want)
    assert dst == mhc.MH_ERR_CORRUPT


def test_batch_stream_through_its_slice(mhc):
    rng = np.random.default_rng(2)
    msgs = [zipf_bytes(int(rng.integers(0, 20_000)), i).tobytes() for i in range(40)]
    model = mhc.Model.from_data(b"".join(msgs), order=1)
    chunk = 256
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=chunk)
    lib = mhc.lib()
    d_pl = mhc.DeviceBuffer(payload.size + 64, init=np.concatenate([payload, np.zeros(64, dtype=np.uint8)]))
    d_idx = mhc.DeviceBuffer(idx.nbytes, init=idx)
    for i in (0, 7, 13, 39):
        m = np.frombuffer(msgs[i], dtype=np.uint8)
        base = lib.mh_batch_index_base(int(in_off[i]), i, chunk)
        ranges = range_set(m.size, chunk, rng, count=500)
        rc, dst, st, out, at, _ = dev_ranges(mhc, model, d_pl.ptr.value + int(out_off[i]), 0, (int(nbits[i]) + 7) // 8, int(nbits[i]),
                                             d_idx.ptr.value + 8 * int(base), chunk, m.size, None, ranges)
        assert rc == 0 and dst == 0
        check_slices(m, ranges, st, out, at)


def test_order2_is_refused(mhc):
    data = b"the order-2 extension has no byte ranges. " * 50
    m2 = mhc.Model.from_data(data, order=2)
    pl, nbits, idx = m2.encode(data, chunk_symbols=1024)
    with pytest.raises(mhc.MhError) as e:
        m2.decode_ranges(pl, nbits, idx, 1024, len(data), [(0, 10)])
    assert e.value.status == mhc.MH_ERR_ARG
    lib = mhc.lib()
    ws = lib.mh_dev_decode_ranges_workspace(1)
    d = mhc.DeviceBuffer(max(ws, 4096))
    assert lib.mh_dev_decode_ranges(m2.handle, d.ptr, 0, 16, nbits, d.ptr, 1024, len(data), None, d.ptr, 1, d.ptr, d.ptr, 16, d.ptr,
                                    d.ptr, ws, None) == mhc.MH_ERR_ARG


@pytest.fixture(scope="module")
def big_stream(mhc):
    data = zipf_bytes(256 << 20, 17)
    model = mhc.Model.from_data(data, order=1)
    pl, nbits, idx = model.encode(data, chunk_symbols=1024)
    return model, data, pl, nbits, idx


def test_host_form_one_small_range_uploads_a_few_chunks(mhc, big_stream):
    model, data, pl, nbits, idx = big_stream
    b = (9 << 20) * 17 + 333
    outs, st = model.decode_ranges(pl, nbits, idx, 1024, data.size, [(b, b + 4096)])
    assert list(st) == [0] and outs[0] == data[b:b + 4096].tobytes()
    up = mhc.lib().mh_last_range_upload_bytes()
    c0, c1 = b // 1024, (b + 4095) // 1024
    span = ((int(idx[c1 + 1] & mhc.INDEX_BIT_MASK) + 7) >> 3) - (int(idx[c0] & mhc.INDEX_BIT_MASK) >> 3)
    assert 0 < up == span and up <= 6 * 1024


def test_host_form_many_ranges(mhc, big_stream):
    model, data, pl, nbits, idx = big_stream
    rng = np.random.default_rng(4)
    n = data.size
    b = rng.integers(0, n, size=10_000)
    e = np.minimum(b + rng.integers(0, 5000, size=10_000), n)
    ranges = list(zip(b.tolist(), e.tolist())) + [(n, n), (0, 1), (n - 1, n), (5, 3), (0, n + 1)]
    outs, st = model.decode_ranges(pl, nbits, idx, 1024, n, ranges)
    assert list(st[-2:]) == [mhc.MH_ERR_ARG] * 2 and outs[-2:] == [b"", b""]
    for j, (x, y) in enumerate(ranges[:-2]):
        assert st[j] == 0 and outs[j] == data[x:y].tobytes(), j
    assert 0 < mhc.lib().mh_last_range_upload_bytes() <= len(pl)


def test_host_form_cuts_windows_at_the_segment_size(mhc, monkeypatch):
    """A small segment puts window edges inside ranges: the pieces are decoded separately and packed back in range order."""
    data = zipf_bytes(3 << 20, 8)
    model = mhc.Model.from_data(data, order=1)
    pl, nbits, idx = model.encode(data, chunk_symbols=512)
    monkeypatch.setenv("MH_SEGMENT_BYTES", str(64 << 10))
    n = data.size
    rng = np.random.default_rng(6)
    ranges = [(0, n), (n // 3, n // 3 + 700_000), (100, 100)] + [(int(x), int(min(x + 3000, n))) for x in rng.integers(0, n, size=300)]
    outs, st = model.decode_ranges(pl, nbits, idx, 512, n, ranges)
    for j, (x, y) in enumerate(ranges):
        assert st[j] == 0 and outs[j] == data[x:y].tobytes(), j
    assert mhc.lib().mh_last_range_upload_bytes() >= len(pl)


def _cli():
    binp = os.path.join(ROOT, "bin", "markovhuffman")
    if not os.path.exists(binp):
        entry.build()
    return binp


def test_cli_range_extract(tmp_path):
    name = "input_wiki_cpp.html"
    data = golden()[name]["data"]
    src = tmp_path / "in"
    src.write_bytes(data)
    cm, table, idx = tmp_path / "in.cm", tmp_path / "in.e", tmp_path / "in.idx"
    r = subprocess.run([_cli(), str(src), "-o", str(cm), "-d", str(table), "--index", str(idx), "--chunk", "1024"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    n = len(data)
    cases = [[(5000, 9000)], [(100, 200), (n - 10, n), (0, 3000)], [(0, n)], [(7, 7)]]
    for k, rs in enumerate(cases):
        out = tmp_path / ("o%d" % k)
        argv = [_cli(), str(cm), "-x", "-e", str(table), "--index", str(idx), "-o", str(out)]
        for b, e in rs:
            argv += ["--range", "%d:%d" % (b, e)]
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == b"".join(data[b:e] for b, e in rs), k
    out = tmp_path / "past"
    r = subprocess.run([_cli(), str(cm), "-x", "-e", str(table), "--index", str(idx), "-o", str(out), "--range", "%d:%d" % (n - 5, n + 1)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and ("%d:%d" % (n - 5, n + 1)).encode() in r.stderr
