"""CPU-side checks of the segment-state calls (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES"): the symbols are declared
in their own section and exported, the workspace size is plain arithmetic, the host forms refuse bad arguments before
touching a device, and every compute call refuses to run without one."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW = ("mh_dev_batch_states_workspace", "mh_dev_batch_states", "mh_dev_each_states", "mh_dev_batch_index", "mh_dev_each_index",
       "mh_dev_batch_emit", "mh_dev_each_emit", "mh_index_batch", "mh_index_each")
SEG_BITS = 512


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data


def test_symbols_are_declared_in_their_section_and_exported(mhc):
    with open(os.path.join(ROOT, "include", "mh.h")) as f:
        text = f.read()
    at = text.index("SEGMENT STATES OF INDEX-FREE BATCHES")
    section = text[at:]
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(mh_\w+)\(", section, re.M))
    assert declared == set(NEW)
    for name in NEW:
        assert name in mhc.EXPORTS
        assert hasattr(mhc.lib(), name)


def test_workspace_is_plain_arithmetic_and_monotone(mhc):
    lib = mhc.lib()
    prev = 0
    for n, total in ((0, 0), (1, 0), (1, 64), (7, 1000), (400, 1 << 20), (65536, 1 << 28)):
        ws = lib.mh_dev_batch_states_workspace(n, total)
        segs = total * 8 // SEG_BITS + n + 1
        assert ws % 256 == 0
        assert ws >= 256 + 2 * 24 * segs + 8 * segs + 20 * n    # header, two record buffers, counts, per-stream words
        assert ws >= prev
        prev = ws
    assert lib.mh_dev_batch_states_workspace(10, 1 << 20) < lib.mh_dev_batch_states_workspace(10, 1 << 21)
    assert lib.mh_dev_batch_states_workspace(10, 4096) < lib.mh_dev_batch_states_workspace(100, 4096)
    assert lib.mh_dev_batch_states_workspace(3, 4096) == lib.mh_dev_batch_states_workspace(3, 4096)


def test_host_forms_refuse_bad_arguments_before_a_device(mhc):
    """MH_ERR_ARG for decreasing offsets, nbits beyond a payload, a chunk size that is not a power of two (or out of range)
    and null pointers — whether or not a device is present."""
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    ARG = mhc.MH_ERR_ARG
    payload = np.zeros(64, dtype=np.uint8)
    so, p_so = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    st = np.zeros(2, dtype=np.int32)
    good_off, p_good = _u64([0, 5, 11])
    bad_off, p_bad = _u64([0, 7, 5])
    nb, p_nb = _u64([40, 48])
    big_nb, p_big = _u64([41, 48])
    tab = np.zeros(8, dtype=np.uint8)
    t_off, p_t = _u64([0, 4, 8])
    t_bad, p_tb = _u64([0, 5, 4])
    pl = payload.ctypes.data

    def both(off, nbits, chunk, sym_off=p_so, index=p_idx, tables_off=p_t):
        a = lib.mh_index_batch(m.handle, pl, off, nbits, 2, 0x20, chunk, sym_off, index, 64, st.ctypes.data)
        b = lib.mh_index_each(tab.ctypes.data, tables_off, pl, off, nbits, 2, 0x20, chunk, sym_off, index, 64, st.ctypes.data)
        return a, b

    assert both(p_bad, p_nb, 256) == (ARG, ARG)
    assert both(p_good, p_big, 256) == (ARG, ARG)             # 41 bits in a 5-byte payload
    for chunk in (0, 100, 255, 257, 1000, 16384):
        assert both(p_good, p_nb, chunk) == (ARG, ARG)
    assert both(p_good, p_nb, 256, sym_off=None) == (ARG, ARG)
    assert both(p_good, p_nb, 256, index=None) == (ARG, ARG)
    assert both(p_good, None, 256) == (ARG, ARG)
    assert both(None, p_nb, 256) == (ARG, ARG)
    assert lib.mh_index_each(tab.ctypes.data, p_tb, pl, p_good, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG
    assert lib.mh_index_each(tab.ctypes.data, None, pl, p_good, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG
    assert lib.mh_index_batch(None, pl, p_good, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG


def test_device_calls_refuse_bad_arguments_first(mhc):
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    ARG, CAP = mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    off, p_off = _u64([0, 5, 11])
    nb, p_nb = _u64([8, 8])
    ws = int(lib.mh_dev_batch_states_workspace(2, 11))
    w = p + 8192
    assert lib.mh_dev_batch_states(None, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_states(m.handle, p, p_off, p_nb, 2, 11, 0x20, None, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_states(m.handle, p + 1, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG    # misaligned payload
    assert lib.mh_dev_batch_states(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, None, w + 8, ws, None) == ARG    # misaligned workspace
    assert lib.mh_dev_batch_states(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws - 256, None) == CAP
    assert lib.mh_dev_each_states(None, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_index(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, 300, None, w, ws, None) == ARG   # chunk
    assert lib.mh_dev_batch_index(m.handle, p, p_off, p_nb, 2, 11, 0x20, None, 64, 256, None, w, ws, None) == ARG
    assert lib.mh_dev_each_index(None, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_emit(m.handle, p, p_off, p_nb, 2, 11, 0x20, p + 4, 64, None, w, ws, None) == ARG   # misaligned out
    assert lib.mh_dev_batch_emit(m.handle, p, p_off, p_nb, 2, 11, 0x20, None, 64, None, w, ws, None) == ARG
    assert lib.mh_dev_each_emit(None, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == ARG


def test_compute_refuses_without_gpu(mhc):
    """No CPU fallback: without a device every compute call of the section reports MH_ERR_NO_DEVICE."""
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = mhc.lib()
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    NO = mhc.MH_ERR_NO_DEVICE
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    off, p_off = _u64([0, 5, 11])
    nb, p_nb = _u64([8, 8])
    ws = int(lib.mh_dev_batch_states_workspace(2, 11))
    w = p + 8192
    assert lib.mh_dev_batch_states(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == NO
    assert lib.mh_dev_batch_index(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws, None) == NO
    assert lib.mh_dev_batch_emit(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == NO
    so, p_so = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    assert lib.mh_index_batch(m.handle, p, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == NO
    table = m.table_bytes()
    tabs = np.frombuffer(table + table, dtype=np.uint8)
    t_off, p_t = _u64([0, len(table), 2 * len(table)])
    assert lib.mh_index_each(tabs.ctypes.data, p_t, p, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == NO
    with pytest.raises(mhc.MhError) as e:
        mhc.index_each([table, table], [b"\x30\xff", b"\x30\x0f"], 256)
    assert e.value.status == NO
