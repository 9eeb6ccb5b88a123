"""CPU-side checks of the bank calls (include/mh.h, "BANKS OF SHARED MODELS"): workspaces are plain arithmetic, and every call
refuses a bad bank size, order, offsets, choice or null pointer before it touches a device."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data


def test_bank_constants_and_workspaces(mhc):
    lib = mhc.lib()
    assert mhc.BANK_MAX == 64 and mhc.BANK_NONE == 0xFFFFFFFF
    for k, n, total in ((1, 0, 0), (2, 1, 1), (3, 1000, 70000), (64, 65536, 4096 * 65536)):
        w = lib.mh_dev_bank_select_workspace(k, n, total)
        # status block, K dense 64 KiB length images, nbits per (stream, entry), one uncovered mask per stream
        assert w % 256 == 0 and w >= 256 + 65536 * k + 8 * n * k + 8 * n
        t = lib.mh_dev_bank_train_workspace(n, total, k)
        # the training workspace holds a select workspace, a gathered copy of the input and the batch histogram's workspace
        assert t >= w + total + lib.mh_dev_histogram_batch_workspace(total) + 65536 * 8
    assert lib.mh_dev_bank_train_workspace(10, 100, 1) <= lib.mh_dev_bank_train_workspace(10, 100, 64)


def test_null_bank_and_bound(mhc):
    lib = mhc.lib()
    off, p_off = _u64([0, 5, 9])
    ch = np.zeros(2, dtype=np.uint32)
    assert lib.mh_encode_bank_bound(None, ch.ctypes.data, p_off, 2) == 0
    buf = np.zeros(4096, dtype=np.uint8)
    b = buf.ctypes.data
    h = ctypes.c_void_p()
    assert lib.mh_dev_bank_select(None, b, p_off, 2, 9, 0x20, b, b, b, 1 << 20, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_set_pick(None, b, 2, None, ctypes.byref(h)) == mhc.MH_ERR_ARG and not h.value
    assert lib.mh_dev_model_set_pick(None, b, 2, None, None) == mhc.MH_ERR_ARG
    oo, p_oo = _u64(np.zeros(3))
    nb, p_nb = _u64(np.zeros(2))
    assert lib.mh_encode_bank(None, b, p_off, 2, 0x20, ch.ctypes.data, b, 4096, p_oo, p_nb, None, 0) == mhc.MH_ERR_ARG
    assert lib.mh_decode_bank(None, ch.ctypes.data, b, p_off, p_nb, 2, 0x20, b, 4096, p_oo, None, 0, None) == mhc.MH_ERR_ARG


def test_training_refuses_bad_arguments_without_a_device(mhc):
    lib = mhc.lib()
    data = np.frombuffer(b"abcdefgh" * 4, dtype=np.uint8)
    d = data.ctypes.data
    good, p_good = _u64([0, 8, 16, 32])
    mono, p_mono = _u64([0, 16, 8, 32])
    first, p_first = _u64([4, 8, 16, 32])
    ch = np.zeros(3, dtype=np.uint32)
    it = ctypes.c_int(0)
    h = ctypes.c_void_p()

    def train(p_in=p_good, order=1, k=2, iters=4, dptr=d, choice=ch.ctypes.data, out=ctypes.byref(h)):
        return lib.mh_bank_train(dptr, p_in, 3, order, 0x20, k, iters, choice, ctypes.byref(it), out)

    assert train(k=0) == mhc.MH_ERR_ARG
    assert train(k=65) == mhc.MH_ERR_ARG
    assert train(order=2) == mhc.MH_ERR_ARG
    assert train(iters=0) == mhc.MH_ERR_ARG
    assert train(p_in=p_mono) == mhc.MH_ERR_ARG
    assert train(p_in=p_first) == mhc.MH_ERR_ARG
    assert train(p_in=None) == mhc.MH_ERR_ARG
    assert train(dptr=None) == mhc.MH_ERR_ARG
    assert train(choice=None) == mhc.MH_ERR_ARG
    assert train(out=None) == mhc.MH_ERR_ARG
    assert not h.value
    # the device form checks the same before it launches anything
    ws = np.zeros(1 << 16, dtype=np.uint8)
    wp = (ws.ctypes.data + 15) & ~15
    for order, k, iters in ((2, 2, 1), (1, 0, 1), (1, 65, 1), (0, 3, 0)):
        assert lib.mh_dev_bank_train(d, p_good, 3, 32, order, 0x20, k, iters, ch.ctypes.data, None, wp, 1 << 15, None,
                                     ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_bank_train(d, p_good, 3, 32, 1, 0x20, 2, 1, ch.ctypes.data, None, wp, 1 << 15, None, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_bank_train(d, p_good, 3, 32, 1, 0x20, 2, 1, ch.ctypes.data, None, wp + 8, 1 << 15, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_bank_train(d, p_good, 3, 32, 1, 0x20, 2, 1, ch.ctypes.data, None, wp, 256, None, ctypes.byref(h)) == mhc.MH_ERR_CAPACITY
