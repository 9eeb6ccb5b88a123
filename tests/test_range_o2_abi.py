"""CPU-side checks of the order-2 random-access calls (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS"): the symbols are
declared and exported, the workspaces are plain arithmetic, and every call refuses a missing model and order-0/1 models with
MH_ERR_ARG before it touches a device, whatever else it is given.  (An order-2 model is built on the device only, so the
pointer, chunk-size and n_symbols checks against an order-2 model run in tests/test_gpu_range_o2.py.)"""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_decode_ranges_o2_workspace", "mh_dev_decode_ranges_o2", "mh_decode_ranges_o2",
               "mh_dev_decode_batch_o2_ranges_workspace", "mh_dev_decode_batch_o2_ranges", "mh_decode_batch_o2_ranges"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def models(mhc):
    """An order-0 and an order-1 model (both build on the host)."""
    return [mhc.Model.from_counts(np.ones(256, dtype=np.uint64), 0), mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)]


def test_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    sec = header[header.index("RANDOM ACCESS INTO ORDER-2 STREAMS"):]
    assert "MH_INDEX2_BIT_MASK" in sec and "0xFFFF" in sec
    fine_note = header[header.index("FINE INDEX"):header.index("#define MH_FINE_SYMBOLS")]
    assert "mh_dev_decode_ranges_o2" in fine_note


def test_workspaces_are_plain_arithmetic_and_monotone(mhc):
    lib = mhc.lib()
    ns = (0, 1, 2, 1000, 4096, 65536, 1 << 20)
    for ws in (lib.mh_dev_decode_ranges_o2_workspace, lib.mh_dev_decode_batch_o2_ranges_workspace):
        sizes = [ws(n) for n in ns]
        for n, s in zip(ns, sizes):
            assert s % 256 == 0 and s >= 64 + 8 * (n + 1)
            assert s <= 64 + 8 * (n + 1) + 8 * ((n + 1 + 1023) // 1024 + 1) + 256
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


class Host:
    """16-byte aligned host stand-ins for every pointer argument: a refusal must come before any of them is dereferenced on a
    device."""

    def __init__(self, mhc):
        self.ws = int(mhc.lib().mh_dev_decode_ranges_o2_workspace(4))
        self.buf = np.zeros(self.ws + 8192, dtype=np.uint8)
        self.p = (self.buf.ctypes.data + 255) & ~255
        self.off = np.zeros(8, dtype=np.uint64)
        self.st = np.zeros(8, dtype=np.int32)
        self.rg = np.array([0, 10], dtype=np.uint64)
        self.lk = np.array([0, 0, 10], dtype=np.uint64)
        self.po = np.array([0, 16, 32], dtype=np.uint64)
        self.nb = np.array([120, 128], dtype=np.uint64)
        self.so = np.array([0, 100, 200], dtype=np.uint64)


def calls(mhc, h, handle):
    """Every _o2 call with plausible arguments and the given model handle: name -> status."""
    lib, p = mhc.lib(), h.p
    return {
        "dev_ranges": lib.mh_dev_decode_ranges_o2(handle, p, 0, 64, 512, p, 256, 400, None, h.rg.ctypes.data, 1, p, p, 16, p, p, h.ws, None),
        "dev_ranges_fine": lib.mh_dev_decode_ranges_o2(handle, p, 0, 64, 512, p, 256, 400, p, h.rg.ctypes.data, 1, p, p, 16, p, p, h.ws, None),
        "host_ranges": lib.mh_decode_ranges_o2(handle, p, 512, p, 256, 400, h.rg.ctypes.data, 1, p, 64, h.off.ctypes.data,
                                               h.st.ctypes.data),
        "dev_lookups": lib.mh_dev_decode_batch_o2_ranges(handle, p, h.po.ctypes.data, h.nb.ctypes.data, 2, 0x20, h.so.ctypes.data, p, 256,
                                                         h.lk.ctypes.data, 1, p, p, 64, p, p, h.ws, None),
        "dev_lookups_free": lib.mh_dev_decode_batch_o2_ranges(handle, p, h.po.ctypes.data, h.nb.ctypes.data, 2, 0x20, None, None, 0,
                                                              h.lk.ctypes.data, 1, p, p, 64, p, p, h.ws, None),
        "host_lookups": lib.mh_decode_batch_o2_ranges(handle, p, 32, h.po.ctypes.data, h.nb.ctypes.data, 2, 0x20, h.so.ctypes.data, p, 256,
                                                      h.lk.ctypes.data, 1, p, 64, h.off.ctypes.data, h.st.ctypes.data),
    }


def test_every_call_refuses_a_missing_model(mhc):
    h = Host(mhc)
    for name, rc in calls(mhc, h, None).items():
        assert rc == mhc.MH_ERR_ARG, name


@pytest.mark.parametrize("order", [0, 1])
def test_every_call_refuses_order_0_and_1_models(mhc, models, order):
    m = models[order]
    assert m.type == order
    h = Host(mhc)
    for name, rc in calls(mhc, h, m.handle).items():
        assert rc == mhc.MH_ERR_ARG, (order, name)
    assert list(h.st) == [0] * 8                               # the host forms refused before writing a status


@pytest.mark.parametrize("order", [0, 1])
def test_python_forms_refuse_order_0_and_1_models(mhc, models, order):
    m = models[order]
    pl = np.zeros(64, dtype=np.uint8)
    idx = np.zeros(2, dtype=np.uint64)
    po, nb, so = np.array([0, 16, 32], dtype=np.uint64), np.array([120, 128], dtype=np.uint64), np.array([0, 100, 200], dtype=np.uint64)
    attempts = [
        lambda: m.decode_ranges_o2(pl.tobytes(), 512, idx, 256, 400, [(0, 10)]),
        lambda: m.decode_batch_o2_ranges(pl[:32], po, nb, [(0, 0, 10)], sym_off=so, index=idx, chunk_symbols=256),
        lambda: m.dev_decode_batch_o2_ranges(pl[:32], po, nb, [(0, 0, 10)]),
        lambda: m.decompress_batch_o2_ranges([b"\x30" + bytes(16)], [(0, 0, 1)]),
    ]
    for k, f in enumerate(attempts):
        with pytest.raises(mhc.MhError) as e:
            f()
        assert e.value.status == mhc.MH_ERR_ARG, k

