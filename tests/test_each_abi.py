"""CPU-side checks of the per-stream-model calls (include/mh.h, "BATCHES OF STREAMS, ONE MODEL EACH"): bounds and workspaces
are plain arithmetic, and the host calls refuse bad arguments before touching a device."""
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


def test_each_bounds_and_workspaces_are_plain_arithmetic(mhc):
    lib = mhc.lib()
    lens = [0, 1, 2, 3, 65, 4096, 0, 100000]
    off, p_off = _u64(np.concatenate([[0], np.cumsum(lens)]))
    tb, pb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mh_compress_each_bounds(p_off, len(lens), ctypes.byref(tb), ctypes.byref(pb)) == mhc.MH_OK
    total = int(off[-1])
    assert tb.value == 33 * len(lens) + (20 * total + 7) // 8 + 16
    want = len(lens) + 16 + sum((k * (min(64, k - 1) if k > 1 else 1) + 7) // 8 for k in lens)
    assert pb.value == want
    for n, total in ((0, 0), (1, 1), (65536, 4096 * 65536), (7, 1000)):
        assert lib.mh_dev_encode_each_workspace(n, total) == lib.mh_dev_encode_batch_workspace(n, total)
        assert lib.mh_dev_decode_each_workspace(n) == lib.mh_dev_decode_batch_workspace(n)
        tw = lib.mh_dev_model_set_train_workspace(n)
        assert tw % 256 == 0 and tw >= 64 + 32 * n + 8 * (n + 1)
    assert lib.mh_encode_each_bound(None, 1000, 3) == (1000 * 64 + 7) // 8 + 3 + 16
    assert lib.mh_model_set_tables_bound(None) == 0 and lib.mh_dev_model_set_tables_workspace(None) == 0
    assert lib.mh_model_set_size(None) == 0 and lib.mh_model_set_slots(None) == 0


def test_host_forms_refuse_bad_offsets_and_pointers_without_a_device(mhc):
    lib = mhc.lib()
    data = np.frombuffer(b"abcdefgh" * 4, dtype=np.uint8)
    buf = np.zeros(4096, dtype=np.uint8)
    tab_off, p_tab = _u64(np.zeros(4))
    out_off, p_out = _u64(np.zeros(4))
    nbits, p_nb = _u64(np.zeros(3))
    good, p_good = _u64([0, 8, 16, 32])
    bad_mono, p_mono = _u64([0, 16, 8, 32])
    bad_first, p_first = _u64([4, 8, 16, 32])
    d, b = data.ctypes.data, buf.ctypes.data

    def comp(p_in, order=1, dptr=d):
        return lib.mh_compress_each(dptr, p_in, 3, order, 0x20, b, 2048, p_tab, b + 2048, 2048, p_out, p_nb, None, 0)

    assert comp(p_mono) == mhc.MH_ERR_ARG
    assert comp(p_first) == mhc.MH_ERR_ARG
    assert comp(p_good, order=2) == mhc.MH_ERR_ARG
    assert comp(p_good, dptr=None) == mhc.MH_ERR_ARG
    assert comp(None) == mhc.MH_ERR_ARG
    assert lib.mh_compress_each(d, p_good, 3, 1, 0x20, b, 2048, None, b + 2048, 2048, p_out, p_nb, None, 0) == mhc.MH_ERR_ARG
    assert lib.mh_compress_each(d, p_good, 3, 1, 0x20, b, 2048, p_tab, b + 2048, 2048, p_out, p_nb, b, 1000) == mhc.MH_ERR_ARG   # chunk not a power of two
    tb = ctypes.c_size_t(0)
    assert lib.mh_compress_each_bounds(p_mono, 3, ctypes.byref(tb), None) == mhc.MH_ERR_ARG

    # decompress: tables and payload offsets, nbits beyond a payload, sym_off with an index
    nb_ok, p_nb_ok = _u64([8, 8, 8])
    nb_big, p_nb_big = _u64([8, 65, 8])
    so, p_so = _u64(np.zeros(4))
    st = np.zeros(3, dtype=np.int32)

    def decomp(pt, pp, pn, idx=None, p_sym=p_so):
        return lib.mh_decompress_each(b, pt, b, pp, pn, 3, 0x20, b + 2048, 2048, p_sym, idx, 256 if idx else 0, st.ctypes.data)

    assert decomp(p_mono, p_good, p_nb_ok) == mhc.MH_ERR_ARG
    assert decomp(p_good, p_first, p_nb_ok) == mhc.MH_ERR_ARG
    assert decomp(p_good, p_good, p_nb_big) == mhc.MH_ERR_ARG
    assert decomp(p_good, p_good, p_nb_ok, idx=b, p_sym=p_mono) == mhc.MH_ERR_ARG
    assert decomp(None, p_good, p_nb_ok) == mhc.MH_ERR_ARG
    assert lib.mh_decompress_each(b, p_good, b, p_good, p_nb_ok, 3, 0x20, b, 16, None, None, 0, None) == mhc.MH_ERR_ARG


def test_device_calls_refuse_bad_arguments_first(mhc):
    lib = mhc.lib()
    h = ctypes.c_void_p()
    off, p_off = _u64([0, 4])
    ws = np.zeros(1024, dtype=np.uint8)
    assert lib.mh_dev_model_set_train(None, p_off, 1, 4, 1, 0x20, ws.ctypes.data, 1024, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_set_train(ws.ctypes.data, p_off, 1, 4, 2, 0x20, ws.ctypes.data, 1024, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_set_train(ws.ctypes.data, p_off, 1, 4, 1, 0x20, ws.ctypes.data, 1024, None, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_set_train(ws.ctypes.data, p_off, 1, 4, 1, 0x20, ws.ctypes.data, 8, None, ctypes.byref(h)) == mhc.MH_ERR_CAPACITY
    assert lib.mh_dev_encode_each(None, ws.ctypes.data, p_off, 1, 4, 0x20, ws.ctypes.data, 16, p_off, p_off, None, 0, ws.ctypes.data, 1024, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_decode_each(None, ws.ctypes.data, p_off, p_off, 1, 4, 0x20, ws.ctypes.data, 16, p_off, 0, None, 0, None, ws.ctypes.data, 1024, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_set_tables(None, ws.ctypes.data, 16, p_off, ws.ctypes.data, 1024, None) == mhc.MH_ERR_ARG
    assert lib.mh_model_set_stream_info(None, 0, None, None) == mhc.MH_ERR_ARG
    assert lib.mh_model_set_from_models(None, 2, ctypes.byref(h)) == mhc.MH_ERR_ARG
    # a malformed table is refused while it is parsed, before any device memory
    bad = np.frombuffer(b"\x80", dtype=np.uint8)               # a Markov table cut after its first bits
    t_off, p_t = _u64([0, 1])
    assert lib.mh_model_set_from_tables(bad.ctypes.data, p_t, 1, ctypes.byref(h)) == mhc.MH_ERR_BADTABLE
    t_mono, p_tm = _u64([0, 1, 0])
    assert lib.mh_model_set_from_tables(bad.ctypes.data, p_tm, 2, ctypes.byref(h)) == mhc.MH_ERR_ARG
