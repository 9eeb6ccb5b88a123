"""CPU-side checks of include/mh.h, "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES": the symbols are declared in their section,
exported and bound; the workspace size is the twin's plain arithmetic; bad arguments and a model of the wrong order are refused
before a device is touched; without a device every compute call reports MH_ERR_NO_DEVICE.  The order-2 model of these checks
is parsed from a hand-written table file (two live contexts), which needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW = ("mh_dev_batch_states_o2_workspace", "mh_dev_batch_states_o2", "mh_dev_batch_index_o2", "mh_dev_batch_emit_o2", "mh_index_batch_o2",
       "mh_dev_batch_states_stats")
TITLE = "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES (extension, parity unpinned)"
SEG_BITS = 512


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def o2_table():
    """An order-2 table file: the empty order-1 table (a 1 bit, 256 0 bits, zero padded to 33 bytes), the magic, then per
    context a live bit and its tree in pre-order (inner node 0, leaf 1 + the symbol).  Contexts (0x20, 0x20) and (0x20, 'a')
    code the symbols 'a' and 'b' with one bit each."""
    bits = [1] + [0] * 263
    for byte in b"MH2\x01":
        bits += [(byte >> (7 - k)) & 1 for k in range(8)]
    leaf = lambda s: [1] + [(s >> (7 - k)) & 1 for k in range(8)]
    for c in range(65536):
        if c in (0x2020, 0x2061):
            bits += [1, 0] + leaf(ord("a")) + leaf(ord("b"))
        else:
            bits.append(0)
    return np.packbits(np.array(bits, dtype=np.uint8)).tobytes()


@pytest.fixture(scope="module")
def m2(mhc):
    m = mhc.Model.from_table(o2_table())
    assert m.type == 2
    return m


@pytest.fixture(scope="module")
def m1(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data


def test_symbols_are_declared_in_their_section_exported_and_bound(mhc):
    with open(os.path.join(ROOT, "include", "mh.h")) as f:
        text = f.read()
    at = text.index(TITLE)
    end = text.index("SEGMENT STATES OF INDEX-FREE BATCHES")
    assert text.index("ORDER 2 IN SEARCH AND RE-CODING (extension") < at < end     # beside its twins' section, in front of it
    section = text[at:end]
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(mh_\w+)\(", section, re.M))
    assert declared == set(NEW)
    lib = ctypes.CDLL(mhc.LIB_PATH)
    for name in NEW:
        assert name in mhc.EXPORTS and hasattr(lib, name), name
    assert "Synchronises" in section or "synchronises the stream" in section   # the diagnostic says that it waits
    assert "follow-up" in section                                              # what stays on its old fallback is said in the header
    for name in ("index_batch_o2", "decode_batch_segments_o2"):
        assert hasattr(mhc.Model, name), name
    assert hasattr(mhc, "index_batch_host_o2") and hasattr(mhc.SegmentStates, "states_stats")


def test_workspace_is_the_twin_s_plain_arithmetic(mhc):
    lib = mhc.lib()
    prev = 0
    for n, total in ((0, 0), (1, 0), (1, 64), (7, 1000), (400, 1 << 20), (65536, 1 << 28)):
        ws = lib.mh_dev_batch_states_o2_workspace(n, total)
        segs = total * 8 // SEG_BITS + n + 1
        assert ws == lib.mh_dev_batch_states_workspace(n, total)
        assert ws % 256 == 0 and ws >= 256 + 2 * 24 * segs + 8 * segs + 20 * n
        assert ws >= prev
        prev = ws
    assert lib.mh_dev_batch_states_o2_workspace(10, 1 << 20) < lib.mh_dev_batch_states_o2_workspace(10, 1 << 21)
    assert lib.mh_dev_batch_states_o2_workspace(10, 4096) < lib.mh_dev_batch_states_o2_workspace(100, 4096)


def _dev_args():
    buf = (ctypes.c_uint8 * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    off, p_off = _u64([0, 5, 11])
    nb, p_nb = _u64([8, 8])
    return (buf, off, nb), p, p_off, p_nb, p + 8192


def test_device_calls_refuse_bad_arguments_first(mhc, m2, m1):
    lib = mhc.lib()
    ARG, CAP = mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY
    keep, p, p_off, p_nb, w = _dev_args()
    ws = int(lib.mh_dev_batch_states_o2_workspace(2, 11))
    h = m2.handle
    assert lib.mh_dev_batch_states_o2(None, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_states_o2(h, p, p_off, p_nb, 2, 11, 0x20, None, None, w, ws, None) == ARG          # no sym_off
    assert lib.mh_dev_batch_states_o2(h, None, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG          # no payload
    assert lib.mh_dev_batch_states_o2(h, p, None, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG              # no offsets
    assert lib.mh_dev_batch_states_o2(h, p, p_off, None, 2, 11, 0x20, p, None, w, ws, None) == ARG             # no nbits
    assert lib.mh_dev_batch_states_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, None, None, ws, None) == ARG          # no workspace
    assert lib.mh_dev_batch_states_o2(h, p + 1, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG         # misaligned payload
    assert lib.mh_dev_batch_states_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, None, w + 8, ws, None) == ARG         # misaligned workspace
    assert lib.mh_dev_batch_states_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws - 256, None) == CAP
    for chunk in (0, 100, 255, 300, 16384):
        assert lib.mh_dev_batch_index_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, 64, chunk, None, w, ws, None) == ARG, chunk
    assert lib.mh_dev_batch_index_o2(h, p, p_off, p_nb, 2, 11, 0x20, None, 64, 256, None, w, ws, None) == ARG  # no index
    assert lib.mh_dev_batch_index_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws - 256, None) == CAP
    assert lib.mh_dev_batch_emit_o2(h, p, p_off, p_nb, 2, 11, 0x20, p + 4, 64, None, w, ws, None) == ARG       # misaligned out
    assert lib.mh_dev_batch_emit_o2(h, p, p_off, p_nb, 2, 11, 0x20, None, 64, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_emit_o2(None, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == ARG
    passes, walked = ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert lib.mh_dev_batch_states_stats(None, None, ctypes.byref(passes), ctypes.byref(walked)) == ARG
    assert lib.mh_dev_batch_states_stats(w, None, None, ctypes.byref(walked)) == ARG
    assert lib.mh_dev_batch_states_stats(w, None, ctypes.byref(passes), None) == ARG
    assert (passes.value, walked.value) == (7, 7)


def test_the_wrong_order_is_refused_both_ways(mhc, m2, m1):
    """Before any launch, whether or not a device is present: the checks come in front of the device's."""
    lib = mhc.lib()
    ARG = mhc.MH_ERR_ARG
    keep, p, p_off, p_nb, w = _dev_args()
    ws = int(lib.mh_dev_batch_states_o2_workspace(2, 11))
    m0 = mhc.Model.from_counts(np.ones(256, dtype=np.uint64), 0)
    for m in (m1, m0):
        assert lib.mh_dev_batch_states_o2(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG
        assert lib.mh_dev_batch_index_o2(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws, None) == ARG
        assert lib.mh_dev_batch_emit_o2(m.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_states(m2.handle, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_index(m2.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws, None) == ARG
    assert lib.mh_dev_batch_emit(m2.handle, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == ARG
    so, p_so = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    pl = np.zeros(64, dtype=np.uint8)
    assert lib.mh_index_batch_o2(m1.handle, pl.ctypes.data, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG
    assert lib.mh_index_batch_o2(None, pl.ctypes.data, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG
    assert lib.mh_index_batch(m2.handle, pl.ctypes.data, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.index_batch_host_o2(m1, pl[:11], np.array([0, 5, 11], dtype=np.uint64), np.array([8, 8], dtype=np.uint64), 256)
    assert e.value.status == ARG


def test_the_host_form_refuses_bad_arguments_before_a_device(mhc, m2):
    lib = mhc.lib()
    ARG = mhc.MH_ERR_ARG
    payload = np.zeros(64, dtype=np.uint8)
    so, p_so = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    st = np.zeros(2, dtype=np.int32)
    good_off, p_good = _u64([0, 5, 11])
    bad_off, p_bad = _u64([0, 7, 5])
    first_off, p_first = _u64([1, 5, 11])
    nb, p_nb = _u64([40, 48])
    big_nb, p_big = _u64([41, 48])
    pl = payload.ctypes.data

    def host(off, nbits, chunk, sym_off=p_so, index=p_idx, payload=pl):
        return lib.mh_index_batch_o2(m2.handle, payload, off, nbits, 2, 0x20, chunk, sym_off, index, 64, st.ctypes.data)

    assert host(p_bad, p_nb, 256) == ARG                          # decreasing offsets
    assert host(p_first, p_nb, 256) == ARG                        # offsets that do not start at 0
    assert host(p_good, p_big, 256) == ARG                        # 41 bits in a 5-byte payload
    for chunk in (0, 100, 255, 257, 1000, 16384):
        assert host(p_good, p_nb, chunk) == ARG
    assert host(p_good, p_nb, 256, sym_off=None) == ARG
    assert host(p_good, p_nb, 256, index=None) == ARG
    assert host(p_good, None, 256) == ARG
    assert host(None, p_nb, 256) == ARG
    assert host(p_good, p_nb, 256, payload=None) == ARG


def test_compute_refuses_without_gpu(mhc, m2):
    """No CPU fallback: without a device every compute call of the section reports MH_ERR_NO_DEVICE."""
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = mhc.lib()
    NO = mhc.MH_ERR_NO_DEVICE
    keep, p, p_off, p_nb, w = _dev_args()
    ws = int(lib.mh_dev_batch_states_o2_workspace(2, 11))
    h = m2.handle
    assert lib.mh_dev_batch_states_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, None, w, ws, None) == NO
    assert lib.mh_dev_batch_index_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, 64, 256, None, w, ws, None) == NO
    assert lib.mh_dev_batch_emit_o2(h, p, p_off, p_nb, 2, 11, 0x20, p, 64, None, w, ws, None) == NO
    so, p_so = _u64(np.zeros(3))
    idx, p_idx = _u64(np.zeros(64))
    assert lib.mh_index_batch_o2(h, p, p_off, p_nb, 2, 0x20, 256, p_so, p_idx, 64, None) == NO
    passes, walked = ctypes.c_uint32(0), ctypes.c_uint64(0)
    assert lib.mh_dev_batch_states_stats(w, None, ctypes.byref(passes), ctypes.byref(walked)) == NO
    with pytest.raises(mhc.MhError) as e:
        mhc.SegmentStates(m2, np.zeros(11, dtype=np.uint8), np.array([0, 5, 11], dtype=np.uint64), np.array([8, 8], dtype=np.uint64), o2=True)
    assert e.value.status == NO
