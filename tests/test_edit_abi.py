"""CPU-side checks of masked re-coding (include/mh.h, "EDITING BATCHES"): the symbols are declared, exported and bound, the
compute calls refuse bad arguments before a device is touched, and mh_spans_from_hits (plain C++, no device) against
tests/edit_ref.py, which merges intervals another way (sorted by begin)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import edit_ref
from conftest import ROOT

NEW_SYMBOLS = ["mh_spans_from_hits", "mh_dev_spans_from_hits_workspace", "mh_dev_spans_from_hits", "mh_dev_recode_edit_workspace",
               "mh_dev_recode_edit_batch", "mh_dev_recode_edit_each", "mh_recode_edit_batch"]
CLI = os.path.join(ROOT, "bin", "markovhuffman")


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


def test_edit_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    at = header.index("EDITING BATCHES")
    section = header[at:header.index("SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES")]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    # what the section must say (the issue): order 2 is out, and the one verdict the call adds
    assert "order-2 model" in section and "only verdict this call adds" in section
    for name in ("dev_recode_edit_batch", "recode_edit_batch"):
        assert hasattr(mhc.Model, name), name
    assert hasattr(mhc.ModelSet, "recode_edit") and hasattr(mhc, "spans_from_hits") and hasattr(mhc, "dev_spans_from_hits")


def test_workspaces_are_plain_arithmetic(mhc):
    lib = mhc.lib()
    for a in [(0, 0, 1024), (1, 1, 256), (65536, 65536 * 4096, 1024), (7, 5000, 0), (7, 5000, 300)]:
        assert lib.mh_dev_recode_edit_workspace(*a) == lib.mh_dev_recode_batch_workspace(*a), a      # the edit keeps nothing of its own
    for n, cap in [(0, 0), (1, 1), (5, 1000), (65536, 100000), (3, 1 << 24)]:
        w = lib.mh_dev_spans_from_hits_workspace(n, cap)
        assert 0 < w <= 32 * cap + (64 << 10) and w % 256 == 0 and w == lib.mh_dev_spans_from_hits_workspace(n + 100, cap), (n, cap, w)
    # 65 536 records with two hits each: a few MiB against the 256 MiB buffer of the decoded bytes
    assert lib.mh_dev_spans_from_hits_workspace(65536, 131072) < 4 << 20


def _dev_edit(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, dst=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             span_off=p, spans=p, map=p, out=p, cap=64, out_off=p, out_nbits=p, out_index=p, dropped=p, status=p, ws=p, wsb=1 << 16, stream=None,
             fn="mh_dev_recode_edit_batch")
    a.update(kw)
    return getattr(mhc.lib(), a["fn"])(*[a[k] for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total",
                                                        "index", "chunk", "span_off", "spans", "map", "out", "cap", "out_off", "out_nbits",
                                                        "out_index", "dropped", "status", "ws", "wsb", "stream")])


def _order2(mhc):
    try:
        return mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0
        return None


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    s, d = model.handle, model0.handle
    assert _dev_edit(mhc, src=None, dst=d) == ARG and _dev_edit(mhc, src=s, dst=None) == ARG
    assert _dev_edit(mhc, src=None, dst=d, fn="mh_dev_recode_edit_each") == ARG
    for k in ("payload", "pay_off", "nbits", "out_off", "out_nbits", "sym_off", "ws", "map"):
        assert _dev_edit(mhc, src=s, dst=d, **{k: None}) == ARG, k
    assert _dev_edit(mhc, src=s, dst=d, index=None, sym_off=None) == ARG          # index-free: sym_off is an output
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _dev_edit(mhc, src=s, dst=d, chunk=bad_chunk) == ARG, bad_chunk
    assert _dev_edit(mhc, src=s, dst=d, index=None, chunk=300) == ARG              # the destination index's chunk
    w = np.zeros(64, dtype=np.uint64)
    odd = ((w.ctypes.data + 255) & ~255) + 8
    for k in ("payload", "out", "ws"):
        assert _dev_edit(mhc, src=s, dst=d, **{k: odd}) == ARG, k
    assert _dev_edit(mhc, src=s, dst=d, wsb=64) == mhc.MH_ERR_CAPACITY
    m2 = _order2(mhc)
    if m2 is not None:
        assert _dev_edit(mhc, src=m2.handle, dst=d) == ARG and _dev_edit(mhc, src=s, dst=m2.handle) == ARG
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert _dev_edit(mhc, src=s, dst=d) == NO and _dev_edit(mhc, src=d, dst=s, span_off=None, spans=None) == NO
    # spans from hits
    lib = mhc.lib()
    p = (w.ctypes.data + 255) & ~255
    assert lib.mh_dev_spans_from_hits(None, p, 4, 1, p, p, p, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, None, 4, 1, p, p, p, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, p, 4, 1, None, p, p, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, p, 4, 1, p, None, p, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, p, 4, 1, p, p, None, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, p, 4, 1, p, p, odd, 1 << 16, None) == ARG
    assert lib.mh_dev_spans_from_hits(p, p, 4, 1, p, p, p, 64, None) == mhc.MH_ERR_CAPACITY
    if mhc.device_count() == 0:
        assert lib.mh_dev_spans_from_hits(p, p, 4, 1, p, p, p, 1 << 16, None) == mhc.MH_ERR_NO_DEVICE


def test_a_set_must_have_one_model_per_stream(mhc, model, model0):
    try:
        ms = mhc.ModelSet.from_models([model, model0, model])
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0       # tests/test_gpu_edit.py has the refusal on the card
        return
    for n in (1, 2, 4):
        assert _dev_edit(mhc, src=ms.handle, dst=model.handle, n=n, fn="mh_dev_recode_edit_each") == mhc.MH_ERR_ARG


def _host(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64), map=np.arange(256, dtype=np.uint8),
             out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64),
             out_index=np.zeros(4, dtype=np.uint64), dropped=np.zeros(2, dtype=np.uint64), status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_edit_batch(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk",
                                                              "span_off", "spans", "map", "out", "cap", "out_off", "out_nbits", "out_index",
                                                              "dropped", "status")])


def test_host_form_refuses_bad_arguments_before_touching_a_device(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    assert _host(mhc, None, model) == ARG and _host(mhc, model, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None),
               dict(map=None), dict(spans=None)):
        assert _host(mhc, model, model0, **kw) == ARG, kw
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, model0, chunk=bad_chunk) == ARG, bad_chunk
    assert _host(mhc, model, model0, pay_off=np.array([0, 16, 8], dtype=np.uint64)) == ARG
    assert _host(mhc, model, model0, nbits=np.array([129, 128], dtype=np.uint64)) == ARG    # nbits past its bytes
    assert _host(mhc, model, model0, span_off=np.array([1, 1, 1], dtype=np.uint64)) == ARG
    assert _host(mhc, model, model0, span_off=np.array([0, 1, 0], dtype=np.uint64)) == ARG
    m2 = _order2(mhc)
    if m2 is not None:
        assert _host(mhc, m2, model) == ARG and _host(mhc, model, m2) == ARG
    if mhc.device_count() == 0:
        assert _host(mhc, model, model0) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, model0, span_off=None, spans=None) == mhc.MH_ERR_NO_DEVICE   # no list: every byte


# ---- mh_spans_from_hits against the reference ----------------------------------------------------------------------------------

def records(per_stream):
    """(hit_off, hits[k, 3]) of per-stream lists of (begin, end, pattern) in the library's order, ascending (end, pattern)."""
    off, rows = [0], []
    for i, lst in enumerate(per_stream):
        for b, e, _ in sorted(lst, key=lambda t: (t[1], t[2])):
            rows.append((i, b, e))
        off.append(len(rows))
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=np.uint64).reshape(-1, 3)


def check_merge(mhc, per_stream, want=None):
    hit_off, hits = records(per_stream)
    so, sp, rc = mhc.spans_from_hits(hit_off, hits)
    r_so, r_sp = edit_ref.merge_hits(hit_off, hits)
    assert rc == mhc.MH_OK and np.array_equal(so, r_so) and np.array_equal(sp, r_sp), (per_stream, so, sp, r_so, r_sp)
    if want is not None:
        assert [sp[int(so[i]):int(so[i + 1])].tolist() for i in range(len(per_stream))] == want, (per_stream, sp)


def test_spans_from_hits_on_crafted_lists(mhc):
    check_merge(mhc, [[(2, 10, 0), (4, 6, 1), (5, 8, 2)]], [[[2, 10]]])                          # nested
    check_merge(mhc, [[(3, 7, 0), (5, 7, 1), (6, 7, 2)]], [[[3, 7]]])                            # equal ends, different patterns
    check_merge(mhc, [[(0, 3, 0), (3, 5, 0), (6, 8, 0)]], [[[0, 5], [6, 8]]])                    # touching merges, a gap of one does not
    check_merge(mhc, [[(0, 2, 0), (1, 3, 0), (2, 4, 0)]], [[[0, 4]]])                            # `aa` in `aaaa`
    # a long pattern that ends last and begins first: the records in front of it are no spans of their own
    check_merge(mhc, [[(10, 12, 0), (20, 22, 0), (30, 32, 0), (5, 40, 1), (50, 52, 0)]], [[[5, 40], [50, 52]]])
    check_merge(mhc, [[(10, 12, 0), (20, 22, 0), (15, 30, 1)]], [[[10, 12], [15, 30]]])          # begins go down, the first stays apart
    check_merge(mhc, [[], [(1, 2, 0)], [], [], [(0, 4, 0), (9, 12, 1)], []], [[], [[1, 2]], [], [], [[0, 4], [9, 12]], []])
    # a span never crosses a stream: equal positions in neighbouring streams
    check_merge(mhc, [[(0, 5, 0)], [(3, 9, 0)], [(9, 10, 0)]], [[[0, 5]], [[3, 9]], [[9, 10]]])
    check_merge(mhc, [], [])                                                                    # n = 0
    check_merge(mhc, [[], []], [[], []])


def test_spans_from_hits_on_200_random_lists(mhc):
    rng = np.random.default_rng(2024)
    for trial in range(200):
        n = int(rng.integers(0, 7))
        per_stream = []
        for _ in range(n):
            k = int(rng.integers(0, 40)) if rng.random() < 0.8 else 0
            span = int(rng.integers(8, 400))
            lens = rng.integers(1, [3, 12, 80][trial % 3], k)
            begins = rng.integers(0, span, k)
            per_stream.append([(int(b), int(b + l), int(rng.integers(0, 5))) for b, l in zip(begins, lens)])
        check_merge(mhc, per_stream)


def test_more_records_than_hit_cap_is_a_capacity_error_with_zeroed_offsets(mhc):
    # what a find call leaves when its hits did not fit: the full counts in hit_off, the first hit_cap records
    hit_off, hits = records([[(0, 2, 0), (1, 3, 0)], [(4, 6, 0)], []])
    so, sp, rc = mhc.spans_from_hits(hit_off, hits[:2], hit_cap=2)
    assert rc == mhc.MH_ERR_CAPACITY and so.tolist() == [0, 0, 0, 0] and sp.size == 0
    so, sp, rc = mhc.spans_from_hits(hit_off, hits, hit_cap=3)
    assert rc == mhc.MH_OK and so.tolist() == [0, 1, 2, 2] and sp.tolist() == [[0, 3], [4, 6]]


def test_reference_apply_clips_and_maps():
    msgs = [b"hello world", b"", b"abc"]
    so, sp = np.array([0, 2, 3, 4], dtype=np.uint64), np.array([[0, 1], [6, 99], [0, 4], [1, 2]], dtype=np.uint64)
    assert edit_ref.apply(msgs, so, sp, edit_ref.mask_map(0x2A)) == [b"*ello *****", b"", b"a*c"]
    fold = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))
    assert edit_ref.apply([b"AbC", b"xyZ"], None, None, fold) == [b"abc", b"xyz"]
    assert edit_ref.apply(msgs, so, sp, edit_ref.IDENTITY) == msgs


# ---- CLI rules ----------------------------------------------------------------------------------------------------------------

REDACT_CASES = {
    "no_recode": (["--redact", "abc"], b"Error: --redact needs --recode."),
    "file_no_recode": (["--redact-file", "deny.txt"], b"Error: --redact needs --recode."),
    "both": (["--recode", "NEW", "--redact", "abc", "--redact-file", "deny.txt"], b"Error: --redact and --redact-file cannot be combined."),
    "mask_alone": (["--recode", "NEW", "--mask", "0"], b"Error: --mask and --redact-fold need --redact or --redact-file."),
    "fold_alone": (["--recode", "NEW", "--redact-fold"], b"Error: --mask and --redact-fold need --redact or --redact-file."),
    "mask_big": (["--recode", "NEW", "--redact", "abc", "--mask", "256"], b"Error: --mask takes a byte value, 0 to 255."),
    "mask_text": (["--recode", "NEW", "--redact", "abc", "--mask", "x"], b"Error: --mask takes a byte value, 0 to 255."),
    "find_too": (["--recode", "NEW", "--redact", "abc", "--index", "f.idx", "--find", "abc"], b"Error: --recode cannot be combined with --find or --range."),
    "order2": (["--recode", "NEW", "--redact", "abc", "--order2"], b"Error: --recode does not support --order2."),
    "empty": (["--recode", "NEW", "--redact", ""], b"Error: --redact takes a non-empty string."),
}


@pytest.mark.parametrize("case", sorted(REDACT_CASES))
def test_cli_redact_argument_errors(mhc, tmp_path, case):
    """The rules of --redact: checked before anything is opened, so the named files need not exist."""
    cm, table, new, out = (str(tmp_path / n) for n in ("in.cm", "table", "new", "out.cm"))
    extra, want = REDACT_CASES[case]
    args = [CLI, cm, "-x", "-e", table, "-o", out] + [new if a == "NEW" else a for a in extra]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    assert want in r.stderr, r.stderr
    assert b"opening" not in r.stderr                                      # refused before any file is touched
    assert not os.path.exists(out)
