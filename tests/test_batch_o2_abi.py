"""CPU-side checks of the order-2 batch calls (include/mh.h, "BATCHES OF ORDER-2 STREAMS"): every name is declared and
exported, workspace sizes are plain arithmetic, the calls refuse a missing or order-0/1 model and bad arguments before
touching a device, and the batch histogram, which needs no model, refuses to run without one."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NAMES = ["mh_dev_histogram_o2_batch_workspace", "mh_dev_histogram_o2_batch", "mh_dev_encode_batch_o2_workspace", "mh_dev_encode_batch_o2",
         "mh_dev_decode_batch_o2_workspace", "mh_dev_decode_batch_o2", "mh_encode_batch_o2", "mh_decode_batch_o2"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data


def test_names_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = mhc.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in mhc.EXPORTS, name
        assert hasattr(lib, name), name
    for name in ("encode_batch_o2", "compress_batch_o2", "decode_batch_o2", "decompress_batch_o2"):
        assert callable(getattr(mhc.Model, name))
    assert callable(mhc.histogram_o2_batch)


def test_workspaces_grow_with_streams_and_input(mhc):
    lib = mhc.lib()
    for total, n in ((0, 0), (1, 1), (4096 * 65536, 65536), (1000, 7)):
        ws = lib.mh_dev_encode_batch_o2_workspace(n, total)
        assert ws % 256 == 0 and ws >= 64 + 8 * (total // 1024 + n + 1)
        assert ws == lib.mh_dev_encode_batch_workspace(n, total)            # the order-0/1 batch's layout
        dws = lib.mh_dev_decode_batch_o2_workspace(n)
        assert dws % 256 == 0 and dws >= 64 + 8 * (n + 1)
    assert lib.mh_dev_encode_batch_o2_workspace(10, 1 << 20) < lib.mh_dev_encode_batch_o2_workspace(10, 1 << 21)
    assert lib.mh_dev_encode_batch_o2_workspace(10, 1 << 20) < lib.mh_dev_encode_batch_o2_workspace(100000, 1 << 20)
    assert lib.mh_dev_decode_batch_o2_workspace(10) < lib.mh_dev_decode_batch_o2_workspace(100000)
    assert lib.mh_dev_histogram_o2_batch_workspace(0) >= 256
    assert lib.mh_dev_histogram_o2_batch_workspace(1 << 20) <= lib.mh_dev_histogram_o2_batch_workspace(1 << 30)
    assert lib.mh_dev_histogram_o2_batch_workspace(0) < lib.mh_dev_histogram_o2_batch_workspace(1 << 30)


def test_o2_calls_reject_bad_arguments_before_a_device(mhc):
    """MH_ERR_ARG for a null or order-1 model, bad offsets, bad chunk sizes and null pointers — with or without a device."""
    lib = mhc.lib()
    m1 = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    data = np.frombuffer(b"hello world, hello batch", dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint8)
    out_off, p_oo = _u64(np.zeros(4))
    nbits, p_nb = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    good, p_good = _u64([0, 5, 11, 24])
    bad, p_bad = _u64([0, 11, 5, 24])
    nz, p_nz = _u64([1, 5, 11, 24])
    ARG = mhc.MH_ERR_ARG
    for mod in (None, m1.handle):
        enc = lambda off, cs=0, ix=None, o=out.ctypes.data, cap=out.size, oo=p_oo: lib.mh_encode_batch_o2(
            mod, data.ctypes.data, off, 3, 0x20, o, cap, oo, p_nb, ix, cs)
        for off in (p_good, p_bad, p_nz, None):
            assert enc(off) == ARG
        assert enc(p_good, oo=None) == ARG
        assert enc(p_good, o=None) == ARG
        for cs in (0, 100, 128, 300, 16384):
            assert enc(p_good, cs, p_idx) == ARG
        st = np.zeros(3, dtype=np.int32)
        so, p_so = _u64(np.zeros(4))
        nb_ok, p_nbok = _u64([8, 8, 8])
        dec = lambda poff, nbp=p_nbok, ix=None, cs=0, sop=p_so: lib.mh_decode_batch_o2(
            mod, out.ctypes.data, poff, nbp, 3, 0x20, out.ctypes.data, out.size, sop, ix, cs, st.ctypes.data)
        for off in (p_good, p_bad, p_nz):
            assert dec(off) == ARG
        assert dec(p_good, sop=None) == ARG
        assert dec(p_good, ix=p_idx, cs=3000) == ARG
        # the device calls: the model and argument checks come first as well
        ws = np.zeros(8192, dtype=np.uint8)
        p_ws = (ws.ctypes.data + 255) & ~255
        for off in (p_good, p_bad):
            assert lib.mh_dev_encode_batch_o2(mod, data.ctypes.data, off, 3, 24, 0x20, out.ctypes.data, 256, p_oo, p_nb, None, 0,
                                              p_ws, 4096, None) == ARG
            assert lib.mh_dev_decode_batch_o2(mod, out.ctypes.data, off, p_nbok, 3, 24, 0x20, out.ctypes.data, 256, p_so, 0, None, 0,
                                              None, p_ws, 4096, None) == ARG
        assert lib.mh_dev_encode_batch_o2(mod, data.ctypes.data, p_good, 3, 24, 0x20, out.ctypes.data, 256, p_oo, p_nb, p_idx, 300,
                                          p_ws, 4096, None) == ARG
    # the histogram: null pointers, a workspace that is not 256-byte aligned
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    assert lib.mh_dev_histogram_o2_batch(p, None, 3, 24, 0x20, p, p, 4096, None) == ARG
    assert lib.mh_dev_histogram_o2_batch(p, p_good, 3, 24, 0x20, None, p, 4096, None) == ARG
    assert lib.mh_dev_histogram_o2_batch(p, p_good, 3, 24, 0x20, p, None, 4096, None) == ARG
    assert lib.mh_dev_histogram_o2_batch(p, p_good, 3, 24, 0x20, p, p + 16, 4096, None) == ARG
    assert lib.mh_dev_histogram_o2_batch(None, p_good, 3, 24, 0x20, p, p, 4096, None) == ARG


def test_o2_histogram_refuses_without_gpu(mhc):
    """No CPU fallback: the batch histogram needs no model, and with valid arguments and no device it reports
    MH_ERR_NO_DEVICE.  (An order-2 model cannot be built without a device, so the other calls have no such case.)"""
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = mhc.lib()
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    off, p_off = _u64([0, 5, 11])
    assert lib.mh_dev_histogram_o2_batch(p, p_off, 2, 11, 0x20, p, p, 4096, None) == mhc.MH_ERR_NO_DEVICE
    with pytest.raises(mhc.MhError) as e:
        mhc.histogram_o2_batch([b"hello", b"", b"world"])
    assert e.value.status == mhc.MH_ERR_NO_DEVICE
