"""CPU-side checks of the lookups into batches (include/mh.h, "RANDOM ACCESS INTO BATCHES"): the symbols are declared,
exported and bound, the workspace is plain arithmetic, and both host forms refuse bad arguments before touching a device."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_decode_batch_ranges_workspace", "mh_dev_decode_batch_ranges", "mh_dev_decode_each_ranges",
               "mh_decode_batch_ranges", "mh_decompress_each_ranges", "mh_last_batch_range_upload_bytes"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def test_batch_range_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    section = header[header.index("RANDOM ACCESS INTO BATCHES"):]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name


def test_batch_range_workspace_is_plain_arithmetic(mhc):
    lib = mhc.lib()
    ns = (0, 1, 2, 1000, 65536, 1 << 20, 1 << 24)
    sizes = [lib.mh_dev_decode_batch_ranges_workspace(n) for n in ns]
    for n, s in zip(ns, sizes):
        assert s % 256 == 0 and s >= 64 + 8 * (n + 1)
        assert s <= 64 + 8 * (n + 1) + 8 * ((n + 1 + 1023) // 1024 + 1) + 256
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.mh_last_batch_range_upload_bytes() == 0


class Batch:
    """Two streams of a batch in host memory: 16 payload bytes each, 100 symbols each, an index of chunk 256."""

    def __init__(self):
        self.payload = np.zeros(32, dtype=np.uint8)
        self.pay_off = np.array([0, 16, 32], dtype=np.uint64)
        self.nbits = np.array([120, 128], dtype=np.uint64)
        self.sym_off = np.array([0, 100, 200], dtype=np.uint64)
        self.index = np.zeros(4, dtype=np.uint64)
        self.tables = np.zeros(64, dtype=np.uint8)
        self.tab_off = np.array([0, 0, 0], dtype=np.uint64)


def _call(mhc, fn, b, lk_in, **kw):
    """A host-form call with the arguments of Batch b, any of them replaced through kw (None: a null pointer).  Returns
    (call status, per-lookup status)."""
    lk = np.ascontiguousarray(np.asarray(lk_in, dtype=np.uint64).reshape(-1, 3))
    a = dict(payload=b.payload, payload_bytes=b.payload.size, pay_off=b.pay_off, nbits=b.nbits, n=2, prev0=0x20, sym_off=b.sym_off,
             index=b.index, chunk=256, lookups=lk, n_lookups=lk.shape[0], out=np.zeros(64, dtype=np.uint8), out_cap=64,
             out_off=np.zeros(lk.shape[0] + 1, dtype=np.uint64), tables=b.tables, tables_bytes=b.tables.size, tab_off=b.tab_off)
    a.update(kw)
    lk = a["lookups"] if isinstance(a["lookups"], np.ndarray) else lk
    st = np.full(max(lk.shape[0], 1), 99, dtype=np.int32)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    tail = (p(a["payload"]), a["payload_bytes"], p(a["pay_off"]), p(a["nbits"]), a["n"], a["prev0"], p(a["sym_off"]), p(a["index"]),
            a["chunk"], p(a["lookups"]), a["n_lookups"], p(a["out"]), a["out_cap"], p(a["out_off"]), st.ctypes.data)
    lib = mhc.lib()
    if fn == "batch":
        rc = lib.mh_decode_batch_ranges(a["model"], *tail)
    else:
        rc = lib.mh_decompress_each_ranges(p(a["tables"]), a["tables_bytes"], p(a["tab_off"]), *tail)
    return rc, st[:lk.shape[0]]


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


@pytest.mark.parametrize("fn", ["batch", "each"])
def test_host_forms_refuse_bad_arguments_before_touching_a_device(mhc, model, fn):
    b = Batch()
    h = dict(model=model.handle) if fn == "batch" else {}
    ARG = mhc.MH_ERR_ARG
    one = [[0, 0, 10]]
    if fn == "batch":
        assert _call(mhc, fn, b, one, model=None)[0] == ARG                         # no model
    else:
        assert _call(mhc, fn, b, one, tab_off=None)[0] == ARG
        assert _call(mhc, fn, b, one, tables=None)[0] == ARG                         # tables_bytes > 0 without tables
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(lookups=None), dict(out_off=None), dict(out=None),
               dict(sym_off=None)):                                                   # (an index needs sym_off)
        assert _call(mhc, fn, b, one, **h, **kw)[0] == ARG, kw
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _call(mhc, fn, b, one, **h, chunk=bad_chunk)[0] == ARG, bad_chunk
    # per lookup, before any device: stream id, begin > end, end > n_i, a touched stream's offsets past the buffers
    rc, st = _call(mhc, fn, b, [[2, 0, 1], [0, 5, 4], [0, 0, 101]], **h)
    assert rc == ARG and list(st) == [ARG] * 3
    po = np.array([0, 16, 40], dtype=np.uint64)                                      # stream 1 ends past payload_bytes
    rc, st = _call(mhc, fn, b, [[1, 0, 10]], **h, pay_off=po)
    assert rc == ARG and list(st) == [ARG]
    rc, st = _call(mhc, fn, b, [[1, 0, 10]], **h, pay_off=np.array([0, 16, 8], dtype=np.uint64))   # non-monotone
    assert rc == ARG and list(st) == [ARG]
    rc, st = _call(mhc, fn, b, [[0, 0, 10]], **h, nbits=np.array([129, 128], dtype=np.uint64))     # nbits past its bytes
    assert rc == ARG and list(st) == [ARG]
    rc, st = _call(mhc, fn, b, [[0, 0, 10]], **h, sym_off=np.array([0, 100, 50], dtype=np.uint64), index=None, chunk=0)
    assert rc == mhc.MH_ERR_NO_DEVICE or st[0] != ARG                                 # stream 1's offsets are not read
    rc, st = _call(mhc, fn, b, [[1, 0, 10]], **h, sym_off=np.array([0, 100, 50], dtype=np.uint64))
    assert rc == ARG and list(st) == [ARG]
    rc, st = _call(mhc, fn, b, [[0, 0, 121]], **h, sym_off=None, index=None, chunk=0)  # index-free: end > nbits_i
    assert rc == ARG and list(st) == [ARG]
    if fn == "each":
        rc, st = _call(mhc, fn, b, [[1, 0, 10]], tab_off=np.array([0, 8, 80], dtype=np.uint64))   # tab_off past tables_bytes
        assert rc == ARG and list(st) == [ARG]
        rc, st = _call(mhc, fn, b, [[1, 0, 10]], tab_off=np.array([0, 8, 4], dtype=np.uint64))
        assert rc == ARG and list(st) == [ARG]
        tabs = np.full(64, 0xFF, dtype=np.uint8)                                      # a Markov table that never ends
        rc, st = _call(mhc, fn, b, [[1, 0, 10]], tables=tabs, tab_off=np.array([0, 0, 64], dtype=np.uint64))
        assert rc == mhc.MH_ERR_BADTABLE and list(st) == [mhc.MH_ERR_BADTABLE]
    # only refused and empty lookups: nothing to decode, no device needed
    rc, st = _call(mhc, fn, b, [[0, 7, 7], [1, 100, 100], [5, 0, 0]], **h)
    assert rc == ARG and list(st) == [mhc.MH_OK, mhc.MH_OK, ARG]


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model):
    lib = mhc.lib()
    ws = int(lib.mh_dev_decode_batch_ranges_workspace(1))
    wbuf = np.zeros(ws + 4096, dtype=np.uint8)
    w = (wbuf.ctypes.data + 255) & ~255                                                # 16-byte aligned host stand-ins
    ARG = mhc.MH_ERR_ARG
    ok = [model.handle, w, w, w, 2, 0x20, w, w, 256, w, 1, w, w, 64, w, w, ws, None]

    def call(fn=lib.mh_dev_decode_batch_ranges, **kw):
        names = ["m", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "lookups", "n_lookups", "out", "out_at",
                 "out_cap", "status", "ws", "ws_bytes", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert call(m=None) == ARG
    assert call(pay_off=None) == ARG
    assert call(payload=None) == ARG
    assert call(payload=w + 4) == ARG                                                # unaligned payload
    assert call(out=w + 8) == ARG
    assert call(ws=None) == ARG
    assert call(lookups=None) == ARG
    assert call(out_at=None) == ARG
    assert call(status=None) == ARG
    assert call(sym_off=None) == ARG                                                 # an index needs sym_off
    for bad_chunk in (0, 100, 128, 16384):
        assert call(chunk=bad_chunk) == ARG
    assert call(ws_bytes=64) == mhc.MH_ERR_CAPACITY
    each = lib.mh_dev_decode_each_ranges
    assert call(fn=each, m=None) == ARG                                              # no set
    assert call(fn=each, m=None, n=0) == ARG


def test_host_forms_without_a_gpu_report_no_device(mhc, model):
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    b = Batch()
    for fn, h in (("batch", dict(model=model.handle)), ("each", {})):
        rc, _ = _call(mhc, fn, b, [[0, 0, 10], [1, 5, 5]], **h)
        assert rc == mhc.MH_ERR_NO_DEVICE, fn
        rc, _ = _call(mhc, fn, b, [[0, 0, 10]], **h, sym_off=None, index=None, chunk=0)
        assert rc == mhc.MH_ERR_NO_DEVICE, fn
    with pytest.raises(mhc.MhError) as e:
        model.decode_batch_ranges(b.payload, b.pay_off, b.nbits, [(1, 0, 10)], sym_off=b.sym_off, index=b.index, chunk_symbols=256)
    assert e.value.status == mhc.MH_ERR_NO_DEVICE
    with pytest.raises(mhc.MhError) as e:
        mhc._each_ranges(b.tables, b.tab_off, b.payload, b.pay_off, b.nbits, [(0, 0, 10)])
    assert e.value.status == mhc.MH_ERR_NO_DEVICE
    assert mhc.lib().mh_last_batch_range_upload_bytes() == 0
