"""CPU-side checks of the batch calls (include/mh.h, "BATCHES OF INDEPENDENT STREAMS"): sizes are plain arithmetic, the host
calls refuse bad arguments before touching a device, every compute call refuses to run without one, the closed-form index
layout gives disjoint slices, and the batch kernels leave the committed counter figures of the single-stream kernels valid."""
import ctypes
import json
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data


def test_batch_sizes_are_plain_arithmetic(mhc):
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.arange(1, 65537, dtype=np.uint64), 1)
    L = m.max_code_len
    for total, n in ((0, 0), (1, 1), (4096 * 65536, 65536), (1000, 7)):
        assert lib.mh_encode_batch_bound(m.handle, total, n) == (total * L + 7) // 8 + n + 16
        ws = lib.mh_dev_encode_batch_workspace(n, total)
        assert ws % 256 == 0 and ws >= 64 + 8 * (total // 1024 + n + 1)
        dws = lib.mh_dev_decode_batch_workspace(n)
        assert dws % 256 == 0 and dws >= 64 + 8 * (n + 1)
    assert lib.mh_dev_encode_batch_workspace(10, 1 << 20) < lib.mh_dev_encode_batch_workspace(10, 1 << 21)
    assert lib.mh_dev_histogram_batch_workspace(0) >= 256
    assert lib.mh_batch_index_capacity(10000, 3, 256) == 10000 // 256 + 4
    assert lib.mh_batch_index_base(5000, 7, 1024) == 5000 // 1024 + 7


def test_workspace_sizes_are_pinned(mhc):
    """The encode and decode workspaces of the three batch families (one shared order-0/1 model, one shared order-2 model, a
    model per stream) share two layouts; their sizes are pinned to what the library returned before the decoders became one
    kernel family: (n_streams, total) -> (encode, decode)."""
    lib = mhc.lib()
    pinned = {(0, 0): (256, 256), (1, 1): (256, 256), (7, 1000): (256, 256), (1000, 1 << 20): (16384, 12288),
              (65536, 4096 * 65536): (2624256, 787200), (1024, (1 << 20) - 1): (16640, 12544), (1023, 1 << 20): (16640, 12544)}
    for (n, total), (enc, dec) in pinned.items():
        for f in (lib.mh_dev_encode_batch_workspace, lib.mh_dev_encode_batch_o2_workspace, lib.mh_dev_encode_each_workspace):
            assert f(n, total) == enc, (f.__name__, n, total)
        for f in (lib.mh_dev_decode_batch_workspace, lib.mh_dev_decode_batch_o2_workspace, lib.mh_dev_decode_each_workspace):
            assert f(n) == dec, (f.__name__, n)


def _slices(off, chunk):
    """Python mirror of the closed-form layout: stream i's entries [in_off_i // chunk + i, ... + ceil(n_i / chunk))."""
    out = []
    for i in range(len(off) - 1):
        n = int(off[i + 1] - off[i])
        b = int(off[i]) // chunk + i
        out.append((b, b + (n + chunk - 1) // chunk))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_index_base_gives_disjoint_slices_within_capacity(mhc, seed):
    lib = mhc.lib()
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    kind = seed % 3
    lens = (rng.integers(0, 20000, n) if kind == 0 else rng.choice([0, 0, 1, 255, 256, 257, 8191, 8192, 8193], n) if kind == 1
            else rng.geometric(1 / 700, n) - 1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    for chunk in (256, 1024, 8192):
        cap = total // chunk + n + 1
        assert lib.mh_batch_index_capacity(total, n, chunk) == cap
        sl = _slices(off, chunk)
        for i, (b, e) in enumerate(sl):
            assert lib.mh_batch_index_base(int(off[i]), i, chunk) == b
            assert 0 <= b <= e <= cap
        for (b0, e0), (b1, e1) in zip(sl, sl[1:]):
            assert e0 <= b1                                  # ceil(m/c) <= floor((a+m)/c) - floor(a/c) + 1
        used = np.zeros(cap, dtype=np.int32)
        for b, e in sl:
            used[b:e] += 1
        assert used.max(initial=0) <= 1


def test_batch_host_calls_reject_bad_arguments_before_a_device(mhc):
    """MH_ERR_ARG for decreasing offsets, bad chunk sizes and null pointers — whether or not a device is present."""
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    data = np.frombuffer(b"hello world, hello batch", dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint8)
    out_off, p_oo = _u64(np.zeros(4))
    nbits, p_nb = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    good, p_good = _u64([0, 5, 11, 24])
    bad, p_bad = _u64([0, 11, 5, 24])
    nz, p_nz = _u64([1, 5, 11, 24])
    ARG = mhc.MH_ERR_ARG
    enc = lambda mod, off, cs=0, ix=None, o=out.ctypes.data, cap=out.size, oo=p_oo: lib.mh_encode_batch(
        mod, data.ctypes.data, off, 3, 0x20, o, cap, oo, p_nb, ix, cs)
    assert enc(m.handle, p_bad) == ARG
    assert enc(m.handle, p_nz) == ARG
    assert enc(None, p_good) == ARG
    assert enc(m.handle, None) == ARG
    assert enc(m.handle, p_good, oo=None) == ARG
    assert enc(m.handle, p_good, o=None) == ARG
    for cs in (0, 100, 128, 300, 16384):
        assert enc(m.handle, p_good, cs, p_idx) == ARG
    st = np.zeros(3, dtype=np.int32)
    so, p_so = _u64(np.zeros(4))
    nb_ok, p_nbok = _u64([8, 8, 8])
    dec = lambda mod, poff, nbp=p_nbok, ix=None, cs=0, sop=p_so: lib.mh_decode_batch(
        mod, out.ctypes.data, poff, nbp, 3, 0x20, out.ctypes.data, out.size, sop, ix, cs, st.ctypes.data)
    assert dec(m.handle, p_bad) == ARG
    assert dec(None, p_good) == ARG
    assert dec(m.handle, p_good, sop=None) == ARG
    too_long, p_tl = _u64([8, 49, 8])                          # stream 1 has 6 payload bytes: 49 bits do not fit
    assert dec(m.handle, p_good, p_tl) == ARG
    assert dec(m.handle, p_good, ix=p_idx, cs=3000) == ARG
    sym_bad, p_sb = _u64([0, 9, 3, 12])
    assert dec(m.handle, p_good, ix=p_idx, cs=256, sop=p_sb) == ARG
    # the device calls: argument errors first as well
    ws = np.zeros(4096, dtype=np.uint8)
    assert lib.mh_dev_encode_batch(None, data.ctypes.data, p_good, 3, 24, 0x20, out.ctypes.data, 256, p_oo, p_nb, None, 0,
                                   ws.ctypes.data, ws.size, None) == ARG
    assert lib.mh_dev_decode_batch(m.handle, None, p_good, p_nbok, 3, 24, 0x20, out.ctypes.data, 256, p_so, 0, None, 0, None,
                                   ws.ctypes.data, ws.size, None) == ARG
    assert lib.mh_dev_histogram_o1_batch(data.ctypes.data, None, 3, 24, 0x20, out.ctypes.data, ws.ctypes.data, ws.size, None) == ARG


def test_batch_compute_refuses_without_gpu(mhc):
    """No CPU fallback: without a device every batch compute call, host and device, reports MH_ERR_NO_DEVICE."""
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    NO = mhc.MH_ERR_NO_DEVICE
    with pytest.raises(mhc.MhError) as e:
        m.compress_batch([b"hello", b"", b"world"], chunk_symbols=256)
    assert e.value.status == NO
    with pytest.raises(mhc.MhError) as e:
        m.decompress_batch([b"\x30\x00", b"\x30\xff"])
    assert e.value.status == NO
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    off, p_off = _u64([0, 5, 11])
    nb, p_nb = _u64([8, 8])
    assert lib.mh_dev_histogram_o1_batch(p, p_off, 2, 11, 0x20, p, p, 4096, None) == NO
    assert lib.mh_dev_histogram_o0_batch(p, p_off, 2, 11, p, p, 4096, None) == NO
    wse = int(lib.mh_dev_encode_batch_workspace(2, 11))
    assert lib.mh_dev_encode_batch(m.handle, p, p_off, 2, 11, 0x20, p, 1024, p, p, None, 0, p + 8192, wse, None) == NO
    wsd = int(lib.mh_dev_decode_batch_workspace(2))
    assert lib.mh_dev_decode_batch(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 1024, p, 0, None, 0, None, p + 8192, wsd, None) == NO


def test_single_stream_counter_figures_stay_valid():
    """The batch kernels live in files of their own: every committed counter figure whose kernel sources matched before still
    matches (set_word_kernel's figure was already stale)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mh_prov", os.path.join(ROOT, "markov-huffman-coding_amd", "provenance.py"))
    prov = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prov)
    for fname, want in (("traffic.json", 11), ("secondary.json", 10)):
        blob = json.load(open(os.path.join(ROOT, "profiles", fname)))
        hashes = blob["_csrc_sha256"]
        same = [k for k, h in hashes.items() if h == prov.kernel_hash(k)]
        assert len(same) == want, (fname, sorted(set(hashes) - set(same)))
        assert "set_word_kernel" not in same
