"""CPU-side checks of the search in batches (include/mh.h, "SEARCH IN BATCHES"): the symbols are declared, exported and
bound, the pattern set is a host object with the argument errors the header lists, the compute calls refuse bad arguments
before a device is touched, the CLI's --find argument rules, and the Python reference against hand-written cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import find_ref
from conftest import ROOT

NEW_SYMBOLS = ["mh_pattern_set_create", "mh_pattern_set_size", "mh_pattern_set_max_len", "mh_pattern_set_free",
               "mh_dev_find_batch_workspace", "mh_dev_find_batch", "mh_dev_find_each", "mh_find_batch"]
CLI = os.path.join(ROOT, "bin", "markovhuffman")


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


def test_find_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    section = header[header.index("SEARCH IN BATCHES"):]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    assert "#define MH_FIND_MAX_POSITIONS 64" in section and "#define MH_FIND_FOLD_ASCII    1u" in section
    assert mhc.FIND_MAX_POSITIONS == 64 and mhc.FIND_FOLD_ASCII == 1


def _create(mhc, data, off, n, flags=0, out=True):
    h = ctypes.c_void_p()
    b = np.frombuffer(bytes(data), dtype=np.uint8) if data is not None else None
    o = np.asarray(off, dtype=np.uint32) if off is not None else None
    rc = mhc.lib().mh_pattern_set_create(b.ctypes.data if b is not None else None, o.ctypes.data if o is not None else None, n, flags,
                                         ctypes.byref(h) if out else None)
    return rc, h


def test_pattern_set_argument_errors(mhc):
    ARG = mhc.MH_ERR_ARG
    lib = mhc.lib()
    assert _create(mhc, b"abc", [0, 3], 0)[0] == ARG                       # no patterns
    assert _create(mhc, b"abc", [0, 0, 3], 2)[0] == ARG                    # an empty pattern
    assert _create(mhc, b"abc", [0, 3, 3], 2)[0] == ARG
    assert _create(mhc, b"abc", [1, 3], 1)[0] == ARG                       # pat_off[0] != 0
    assert _create(mhc, b"abc", [0, 2, 1], 2)[0] == ARG                    # decreasing
    assert _create(mhc, b"abc", [0, 3], 1, flags=2)[0] == ARG              # unknown flag bits
    assert _create(mhc, b"abc", [0, 3], 1, flags=3)[0] == ARG
    assert _create(mhc, None, [0, 3], 1)[0] == ARG
    assert _create(mhc, b"abc", None, 1)[0] == ARG
    assert _create(mhc, b"abc", [0, 3], 1, out=False)[0] == ARG
    assert _create(mhc, b"x" * 65, [0, 65], 1)[0] == ARG                   # 65 bytes in one pattern
    assert _create(mhc, b"x" * 65, list(range(66)), 65)[0] == ARG          # ... in 65 patterns
    assert _create(mhc, b"x" * 65, [0, 64, 65], 2)[0] == ARG
    for data, off, n in ((b"x" * 64, [0, 64], 1), (bytes(range(64)), list(range(65)), 64), (b"\0\0a", [0, 2, 3], 2), (b"aa", [0, 1, 2], 2)):
        for flags in (0, mhc.FIND_FOLD_ASCII):
            rc, h = _create(mhc, data, off, n, flags)
            assert rc == mhc.MH_OK and h.value
            assert lib.mh_pattern_set_size(h) == n
            assert lib.mh_pattern_set_max_len(h) == max(off[j + 1] - off[j] for j in range(n))
            lib.mh_pattern_set_free(h)
    assert lib.mh_pattern_set_size(None) == 0 and lib.mh_pattern_set_max_len(None) == 0
    lib.mh_pattern_set_free(None)
    ps = mhc.PatternSet([b"href", b"C++"], fold=True)
    assert len(ps) == 2 and ps.max_len == 4
    with pytest.raises(mhc.MhError) as e:
        mhc.PatternSet([b"a", b""])
    assert e.value.status == ARG


def test_find_workspace_is_plain_arithmetic(mhc):
    lib = mhc.lib()
    base = lib.mh_dev_find_batch_workspace(0, 0, 0)
    assert base % 256 == 0 and 64 + 2048 <= base <= 64 + 2048 + 512
    for n, total, chunk in ((1, 1 << 28, 1024), (65536, 1 << 28, 1024), (1000, 10 ** 6, 256), (3, 0, 8192)):
        s = lib.mh_dev_find_batch_workspace(n, total, chunk)
        w = total // chunk + n + 1
        assert s % 256 == 0
        assert s >= 64 + 2048 + 4 * n + 24 * w                             # a few bytes per chunk: state, two counts, the scan
        assert s <= 64 + 2048 + 4 * n + 24 * w + 8 * (w // 1024 + 4) + 1024
        free = lib.mh_dev_find_batch_workspace(n, total, 0)                # index-free: nothing per chunk
        assert free <= base + 4 * n + 8 * (n // 1024 + 4) + 512
    assert lib.mh_dev_find_batch_workspace(8, 1 << 20, 300) == lib.mh_dev_find_batch_workspace(8, 1 << 20, 0)


NAMES = ["m", "ps", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total", "index", "chunk", "hit_off", "hits",
         "pattern", "hit_cap", "status", "ws", "ws_bytes", "stream"]


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model):
    lib = mhc.lib()
    ws = int(lib.mh_dev_find_batch_workspace(2, 200, 256))
    wbuf = np.zeros(ws + 4096, dtype=np.uint8)
    w = (wbuf.ctypes.data + 255) & ~255                                    # 16-byte aligned host stand-ins
    ps = mhc.PatternSet([b"abc"])
    ARG = mhc.MH_ERR_ARG
    ok = [model.handle, ps.handle, w, w, w, 2, 32, 0x20, w, 200, w, 256, w, w, w, 8, w, w, ws, None]

    def call(fn=lib.mh_dev_find_batch, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[NAMES.index(k)] = v
        return fn(*a)

    assert call(m=None) == ARG
    assert call(ps=None) == ARG
    assert call(pay_off=None) == ARG
    assert call(payload=None) == ARG
    assert call(nbits=None) == ARG
    assert call(payload=w + 4) == ARG                                      # unaligned payload
    assert call(ws=None) == ARG
    assert call(ws=w + 8) == ARG
    assert call(hit_off=None) == ARG
    assert call(sym_off=None) == ARG                                       # an index needs sym_off
    for bad_chunk in (0, 100, 128, 16384):
        assert call(chunk=bad_chunk) == ARG
    assert call(ws_bytes=64) == mhc.MH_ERR_CAPACITY
    assert call(ws_bytes=ws - 1) == mhc.MH_ERR_CAPACITY
    each = lib.mh_dev_find_each
    assert call(fn=each, m=None) == ARG                                    # no set
    assert call(fn=each, m=None, n=0) == ARG
    if mhc.device_count() == 0:
        # valid arguments reach the device check: hits and pattern numbers may be NULL (count only), index-free needs no sym_off
        assert call() == mhc.MH_ERR_NO_DEVICE
        assert call(hits=None, pattern=None, status=None) == mhc.MH_ERR_NO_DEVICE
        assert call(index=None, sym_off=None, chunk=0, sym_total=0) == mhc.MH_ERR_NO_DEVICE


def test_order2_model_is_refused_before_any_launch(mhc):
    lib = mhc.lib()
    counts = np.zeros(1 << 24, dtype=np.uint64)
    counts[(0x2020 << 8) | 65] = 3
    counts[(0x2041 << 8) | 66] = 2
    try:
        m2 = mhc.Model.from_counts(counts, 2)
    except mhc.MhError as e:                                               # an order-2 model cannot be built without a device:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0   # tests/test_gpu_find.py has the refusal on the card
        return
    ps = mhc.PatternSet([b"abc"])
    w = np.zeros(8192, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    assert lib.mh_dev_find_batch(m2.handle, ps.handle, p, p, p, 1, 16, 0x20, p, 100, p, 256, p, p, p, 8, p, p, 1 << 15, None) == mhc.MH_ERR_ARG
    assert lib.mh_find_batch(m2.handle, ps.handle, p, p, p, 1, 0x20, p, p, 256, p, p, p, 8, p) == mhc.MH_ERR_ARG


def _host(mhc, model, ps, **kw):
    a = dict(m=model.handle if model is not None else None, ps=ps.handle if ps is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             hit_off=np.zeros(3, dtype=np.uint64), hits=np.zeros(24, dtype=np.uint64), pattern=np.zeros(8, dtype=np.uint32), hit_cap=8,
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_find_batch(*[p(a[k]) for k in ("m", "ps", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk",
                                                       "hit_off", "hits", "pattern", "hit_cap", "status")])


def test_host_form_refuses_bad_arguments_before_touching_a_device(mhc, model):
    ps = mhc.PatternSet([b"abc", b"bc"])
    ARG = mhc.MH_ERR_ARG
    assert _host(mhc, None, ps) == ARG
    assert _host(mhc, model, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(hit_off=None), dict(sym_off=None)):
        assert _host(mhc, model, ps, **kw) == ARG, kw
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, ps, chunk=bad_chunk) == ARG, bad_chunk
    assert _host(mhc, model, ps, pay_off=np.array([1, 16, 32], dtype=np.uint64)) == ARG
    assert _host(mhc, model, ps, pay_off=np.array([0, 16, 8], dtype=np.uint64)) == ARG
    assert _host(mhc, model, ps, nbits=np.array([129, 128], dtype=np.uint64)) == ARG          # nbits past its bytes
    assert _host(mhc, model, ps, sym_off=np.array([0, 100, 50], dtype=np.uint64)) == ARG
    if mhc.device_count() == 0:
        assert _host(mhc, model, ps) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, ps, hits=None, pattern=None, hit_cap=0, status=None) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, ps, sym_off=None, index=None, chunk=0) == mhc.MH_ERR_NO_DEVICE
        with pytest.raises(mhc.MhError) as e:
            model.find_batch(ps, np.zeros(32, dtype=np.uint8), [0, 16, 32], [120, 128])
        assert e.value.status == mhc.MH_ERR_NO_DEVICE


@pytest.mark.parametrize("case", ["no_x", "no_index", "order2", "empty", "too_long", "with_range", "fold_alone"])
def test_cli_find_argument_errors(mhc, tmp_path, case):
    """The rules of --range: checked before anything is opened, so the named files need not exist."""
    cm, table, idx, out = (str(tmp_path / n) for n in ("in.cm", "table", "f.idx", "out"))
    base = [CLI, cm, "-o", out]
    args = {
        "no_x": base + ["-e", table, "--index", idx, "--find", "abc"],
        "no_index": base + ["-x", "-e", table, "--find", "abc"],
        "order2": base + ["-x", "-e", table, "--index", idx, "--order2", "--find", "abc"],
        "empty": base + ["-x", "-e", table, "--index", idx, "--find", ""],
        "too_long": base + ["-x", "-e", table, "--index", idx, "--find", "a" * 40, "--find", "b" * 25],
        "with_range": base + ["-x", "-e", table, "--index", idx, "--find", "abc", "--range", "0:3"],
        "fold_alone": base + ["-x", "-e", table, "--index", idx, "--find-fold"],
    }[case]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    assert b"--find" in r.stderr and b"Error" in r.stderr, r.stderr
    assert b"opening" not in r.stderr                                      # refused before any file is touched
    assert not os.path.exists(out)


# ---- the reference against itself ---------------------------------------------------------------------------------------------

def test_reference_counts_overlapping_occurrences():
    assert find_ref.occurrences(b"aaaa", b"aa") == [0, 1, 2]
    assert find_ref.find_hits([b"aaaa"], [b"aa"]) == [(0, 0, 2, 0), (0, 1, 3, 0), (0, 2, 4, 0)]
    assert len(find_ref.find_hits([b"a" * 300], [b"aaaa"])) == 297
    assert find_ref.find_hits([b"abc"], [b"abcd"]) == [] and find_ref.find_hits([b""], [b"a"]) == []


def test_reference_stops_at_stream_boundaries():
    assert find_ref.find_hits([b"xxab", b"cxx"], [b"abc"]) == []
    assert find_ref.find_hits([b"xxab" + b"cxx"], [b"abc"]) == [(0, 2, 5, 0)]
    assert find_ref.find_hits([b"", b"abc", b"", b"zabc", b""], [b"abc"]) == [(1, 0, 3, 0), (3, 1, 4, 0)]


def test_reference_orders_by_stream_end_pattern():
    # a pattern and its own suffix end together: the lower pattern number first; equal patterns each report their hits
    assert find_ref.find_hits([b"xabcx"], [b"abc", b"bc", b"abc"]) == [(0, 1, 4, 0), (0, 2, 4, 1), (0, 1, 4, 2)]
    assert find_ref.find_hits([b"ab", b"ba"], [b"b", b"a"]) == [(0, 0, 1, 1), (0, 1, 2, 0), (1, 0, 1, 0), (1, 1, 2, 1)]
    off, rec, pat = find_ref.hit_arrays(find_ref.find_hits([b"ab", b"", b"ba"], [b"b", b"a"]), 3)
    assert off.tolist() == [0, 2, 2, 4] and rec.tolist() == [[0, 0, 1], [0, 1, 2], [2, 0, 1], [2, 1, 2]] and pat.tolist() == [1, 0, 0, 1]


def test_reference_folds_ascii_letters_only():
    assert find_ref.fold_ascii(bytes(range(256))) == bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))
    assert len(find_ref.find_hits([b"C++ c++ C+-"], [b"c++"], fold=True)) == 2
    assert len(find_ref.find_hits([b"C++ c++"], [b"c++"])) == 1
    assert find_ref.find_hits([b"\xc4\xe4"], [b"\xe4"], fold=True) == [(0, 1, 2, 0)]      # bytes outside ASCII are not folded
    assert find_ref.find_hits([b"[{"], [b"{"], fold=True) == [(0, 1, 2, 0)]              # '[' + 32 == '{': not a letter
    assert find_ref.straddles([(0, 254, 258, 0), (0, 256, 260, 0), (0, 250, 256, 0)], 256) == 1
    assert find_ref.lines_with([(0, 0, 1, 0), (0, 1, 2, 0), (3, 0, 1, 0), (4, 0, 1, 1)], 0) == 2
