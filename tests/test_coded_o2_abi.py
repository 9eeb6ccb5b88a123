"""CPU-side checks of include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING": the symbols are declared, exported and bound, the
workspace functions are plain arithmetic inside the documented bounds, and every new entry refuses bad arguments before a
device is touched.  An order-2 model cannot be built without a device, so every check that needs one (the argument checks of
mh_dev_find_batch_o2 and mh_dev_recode_batch_o2 and of the host forms) is in tests/test_gpu_coded_o2.py; with an order-2
model there is a device, so MH_ERR_NO_DEVICE is reachable only through the coded histogram of an order-1 source, below."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_find_batch_o2_workspace", "mh_dev_find_batch_o2", "mh_find_batch_o2", "mh_dev_histogram_coded_batch_o2_workspace",
               "mh_dev_histogram_coded_batch_o2", "mh_dev_recode_batch_o2_workspace", "mh_dev_recode_batch_o2", "mh_recode_batch_o2"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


@pytest.fixture(scope="module")
def model0(mhc):
    return mhc.Model.from_counts(np.ones(256, dtype=np.uint64), 0)


@pytest.fixture(scope="module")
def ps(mhc):
    return mhc.PatternSet([b"abc"])


def test_symbols_are_declared_exported_and_bound(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    at = header.index("ORDER 2 IN SEARCH AND RE-CODING (extension")
    assert header.index(" * RE-CODING BATCHES") < at < header.index("SEGMENT STATES OF INDEX-FREE BATCHES")
    section = header[at:header.index("SEGMENT STATES OF INDEX-FREE BATCHES")]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    assert "model sets" in section and "follow-up" in section          # what the family leaves out is said in the header
    for m in ("find_batch_o2", "dev_find_batch_o2", "recode_batch_o2", "dev_recode_batch_o2", "dev_histogram_coded_o2"):
        assert hasattr(mhc.Model, m), m
    assert hasattr(mhc, "histogram_coded_batch_o2")


@pytest.mark.parametrize("n,total,chunk", [(1, 0, 256), (40, 9000, 256), (65536, 1 << 28, 1024)])
def test_workspaces_obey_their_bounds(mhc, n, total, chunk):
    lib = mhc.lib()
    numbers = total // chunk + n + 1
    f, h, r = (fn(n, total, chunk) for fn in (lib.mh_dev_find_batch_o2_workspace, lib.mh_dev_histogram_coded_batch_o2_workspace,
                                             lib.mh_dev_recode_batch_o2_workspace))
    assert f == lib.mh_dev_find_batch_workspace(n, total, chunk)        # search stays at the order-0/1 size
    assert 0 < r <= 24 * numbers + 8 * n + 4096, (r, numbers)
    assert r >= lib.mh_dev_recode_batch_workspace(n, total, chunk)      # the head bits and the closing context come on top
    assert 0 < h <= 8 * n + 4096                                        # nothing per chunk: the caller owns the counters
    assert h == lib.mh_dev_histogram_coded_batch_o2_workspace(n, total * 7 + 1, chunk)
    # no argument is a payload size: the functions cannot depend on pay_total
    for fn in (lib.mh_dev_find_batch_o2_workspace, lib.mh_dev_histogram_coded_batch_o2_workspace, lib.mh_dev_recode_batch_o2_workspace):
        assert len(fn.argtypes) == 3
    if (n, chunk) == (65536, 1024):
        assert r < 8 << 20                                              # against the 256 MiB of decoded bytes it replaces


def _buf():
    w = np.zeros(1 << 14, dtype=np.uint64)
    return w, (w.ctypes.data + 255) & ~255


def _dev_find(mhc, **kw):
    w, p = _buf()
    a = dict(m=None, ps=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             hit_off=p, hits=p, pat=p, cap=4, status=p, ws=p, wsb=1 << 16, stream=None)
    a.update(kw)
    return mhc.lib().mh_dev_find_batch_o2(*[a[k] for k in ("m", "ps", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off",
                                                           "sym_total", "index", "chunk", "hit_off", "hits", "pat", "cap", "status", "ws", "wsb",
                                                           "stream")])


def _dev_recode(mhc, **kw):
    w, p = _buf()
    a = dict(src=None, dst=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             out=p, cap=64, out_off=p, out_nbits=p, out_index=p, dropped=p, status=p, ws=p, wsb=1 << 16, stream=None)
    a.update(kw)
    return mhc.lib().mh_dev_recode_batch_o2(*[a[k] for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off",
                                                             "sym_total", "index", "chunk", "out", "cap", "out_off", "out_nbits", "out_index",
                                                             "dropped", "status", "ws", "wsb", "stream")])


def _dev_hist(mhc, **kw):
    w, p = _buf()
    a = dict(src=None, order=2, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             counts=p, status=p, ws=p, wsb=1 << 16, stream=None)
    a.update(kw)
    return mhc.lib().mh_dev_histogram_coded_batch_o2(*[a[k] for k in ("src", "order", "payload", "pay_off", "nbits", "n", "pay_total", "prev0",
                                                                      "sym_off", "sym_total", "index", "chunk", "counts", "status", "ws", "wsb",
                                                                      "stream")])


def test_find_o2_refuses_a_model_that_is_not_order_2(mhc, model, model0, ps):
    for m in (None, model.handle, model0.handle):
        assert _dev_find(mhc, m=m, ps=ps.handle) == mhc.MH_ERR_ARG
    pay, off, nb = np.zeros(32, dtype=np.uint8), np.array([0, 16, 32], dtype=np.uint64), np.array([120, 128], dtype=np.uint64)
    ho = np.zeros(3, dtype=np.uint64)
    for m in (None, model.handle):
        assert mhc.lib().mh_find_batch_o2(m, ps.handle, pay.ctypes.data, off.ctypes.data, nb.ctypes.data, 2, 0x20, None, None, 0,
                                          ho.ctypes.data, None, None, 0, None) == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        model.find_batch_o2(ps, pay, off, nb)
    assert e.value.status == mhc.MH_ERR_ARG


def test_an_order_2_side_is_required(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    for s in (model, model0):
        for d in (model, model0):
            assert _dev_recode(mhc, src=s.handle, dst=d.handle) == ARG              # mh_dev_recode_batch serves these
        for order in (0, 1):
            assert _dev_hist(mhc, src=s.handle, order=order) == ARG                 # mh_dev_histogram_coded_batch serves these
        for order in (-1, 3, 7):
            assert _dev_hist(mhc, src=s.handle, order=order) == ARG
    assert _dev_recode(mhc, src=None, dst=model.handle) == ARG and _dev_recode(mhc, src=model.handle, dst=None) == ARG
    assert _dev_hist(mhc, src=None) == ARG
    so, pay, off, nb = np.zeros(3, dtype=np.uint64), np.zeros(32, dtype=np.uint8), np.array([0, 16, 32], dtype=np.uint64), np.array([120, 128], dtype=np.uint64)
    oo, onb = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert mhc.lib().mh_recode_batch_o2(model.handle, model0.handle, pay.ctypes.data, off.ctypes.data, nb.ctypes.data, 2, 0x20, so.ctypes.data,
                                        None, 0, None, 0, oo.ctypes.data, onb.ctypes.data, None, None, None) == ARG


def test_coded_histogram_checks_before_any_launch(mhc, model):
    """Order 2 from an order-1 source is a valid pair, so every later check is reachable without a device."""
    ARG, s = mhc.MH_ERR_ARG, model.handle
    for k in ("payload", "pay_off", "nbits", "counts", "sym_off", "ws"):
        assert _dev_hist(mhc, src=s, **{k: None}) == ARG, k
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _dev_hist(mhc, src=s, chunk=bad_chunk) == ARG, bad_chunk
    w, p = _buf()
    for k in ("payload", "ws"):
        assert _dev_hist(mhc, src=s, **{k: p + 8}) == ARG, k
    need = mhc.lib().mh_dev_histogram_coded_batch_o2_workspace(1, 100, 256)
    assert _dev_hist(mhc, src=s, wsb=need - 1) == mhc.MH_ERR_CAPACITY
    if mhc.device_count() == 0:
        assert _dev_hist(mhc, src=s, wsb=need) == mhc.MH_ERR_NO_DEVICE
        assert _dev_hist(mhc, src=s, index=None, sym_off=None, chunk=0, status=None) == mhc.MH_ERR_NO_DEVICE
