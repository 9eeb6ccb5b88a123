"""CPU-side checks of splicing re-coding (include/mh.h, "SPLICING BATCHES"): the symbols are declared, exported and bound, the
calls refuse bad arguments before a device is touched, the workspace is plain arithmetic that grows with the spans and the
chunks, and tests/splice_ref.py against hand-written cases."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import splice_ref
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_recode_splice_workspace", "mh_dev_recode_splice_batch", "mh_dev_recode_splice_each", "mh_recode_splice_batch"]


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


def test_splice_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    at = header.index("SPLICING BATCHES (extension")
    section = header[at:header.index("SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES")]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    assert "#define MH_SPLICE_MAX_REP 255u" in section and mhc.SPLICE_MAX_REP == 255
    # what the section must say: what is left out
    assert "order 2; pure insertions (begin == end); a replacement per span or per pattern" in section
    for name in ("dev_recode_splice_batch", "recode_splice_batch"):
        assert hasattr(mhc.Model, name), name
    assert hasattr(mhc.ModelSet, "recode_splice")


def test_the_workspace_grows_with_the_spans_and_the_chunks(mhc):
    ws = mhc.lib().mh_dev_recode_splice_workspace
    for a in [(0, 0, 1024, 0), (1, 1, 256, 1), (65536, 65536 * 4096, 1024, 65536), (7, 5000, 0, 3), (7, 5000, 300, 3)]:
        assert ws(*a) > 0 and ws(*a) % 256 == 0, a
    # four bytes a span, behind everything else
    assert 400000 - 256 < ws(8, 4000, 256, 100000) - ws(8, 4000, 256, 0) < 400000 + 256
    assert ws(8, 4000, 256, 10) <= ws(8, 4000, 256, 1000) < ws(8, 4000, 256, 100000)
    # per chunk number: 8 + 8 + 4 bytes and the scans' block sums
    a, b = ws(8, 1 << 20, 256, 0), ws(8, 1 << 24, 256, 0)
    chunks = ((1 << 24) - (1 << 20)) // 256
    assert 20 * chunks <= b - a <= 21 * chunks
    assert ws(8, 1 << 24, 0, 0) == ws(8, 0, 0, 0) and ws(8, 1 << 24, 300, 0) == ws(8, 0, 0, 0)      # index-free, or no valid chunk size
    # 65 536 records of 4 KiB, chunk 1024, one span each: a few MiB against the 256 MiB buffer of the decoded bytes
    assert ws(65536, 65536 * 4096, 1024, 65536) < 8 << 20


def _dev(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, dst=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             span_off=p, spans=p, rep=p, rep_len=3, out=p, cap=64, out_off=p, out_nbits=p, out_sym_off=p, out_index=p, index_cap=2, dropped=p,
             status=p, ws=p, wsb=1 << 16, stream=None, fn="mh_dev_recode_splice_batch")
    a.update(kw)
    return getattr(mhc.lib(), a["fn"])(*[a[k] for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total",
                                                        "index", "chunk", "span_off", "spans", "rep", "rep_len", "out", "cap", "out_off",
                                                        "out_nbits", "out_sym_off", "out_index", "index_cap", "dropped", "status", "ws", "wsb",
                                                        "stream")])


def _order2(mhc):
    try:
        return mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0
        return None


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    s, d = model.handle, model0.handle
    assert _dev(mhc, src=None, dst=d) == ARG and _dev(mhc, src=s, dst=None) == ARG
    assert _dev(mhc, src=None, dst=d, fn="mh_dev_recode_splice_each") == ARG
    # the replacement and the list: refused whatever else is passed
    assert _dev(mhc, src=s, dst=d, rep_len=256) == ARG and _dev(mhc, src=s, dst=d, rep_len=1 << 20) == ARG
    assert _dev(mhc, src=s, dst=d, rep=None, rep_len=1) == ARG
    assert _dev(mhc, src=s, dst=d, span_off=None) == ARG
    assert _dev(mhc, src=s, dst=d, out_sym_off=None) == ARG
    for k in ("payload", "pay_off", "nbits", "out_off", "out_nbits", "sym_off", "ws"):
        assert _dev(mhc, src=s, dst=d, **{k: None}) == ARG, k
    assert _dev(mhc, src=s, dst=d, index=None, sym_off=None) == ARG             # index-free: sym_off is an output
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _dev(mhc, src=s, dst=d, chunk=bad_chunk) == ARG, bad_chunk
    assert _dev(mhc, src=s, dst=d, index=None, chunk=300) == ARG                 # the destination index's chunk
    w = np.zeros(64, dtype=np.uint64)
    odd = ((w.ctypes.data + 255) & ~255) + 8
    for k in ("payload", "out", "ws"):
        assert _dev(mhc, src=s, dst=d, **{k: odd}) == ARG, k
    assert _dev(mhc, src=s, dst=d, wsb=64) == mhc.MH_ERR_CAPACITY
    m2 = _order2(mhc)
    if m2 is not None:
        assert _dev(mhc, src=m2.handle, dst=d) == ARG and _dev(mhc, src=s, dst=m2.handle) == ARG
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert _dev(mhc, src=s, dst=d) == NO and _dev(mhc, src=d, dst=s, rep=None, rep_len=0) == NO       # a deletion needs no rep


def test_a_set_must_have_one_model_per_stream(mhc, model, model0):
    try:
        ms = mhc.ModelSet.from_models([model, model0, model])
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0       # tests/test_gpu_splice.py has the refusal on the card
        return
    for n in (1, 2, 4):
        assert _dev(mhc, src=ms.handle, dst=model.handle, n=n, fn="mh_dev_recode_splice_each") == mhc.MH_ERR_ARG


def _host(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64), rep=np.frombuffer(b"[X]", dtype=np.uint8),
             rep_len=3, out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64),
             out_sym_off=np.zeros(3, dtype=np.uint64), out_index=np.zeros(4, dtype=np.uint64), index_cap=4, dropped=np.zeros(2, dtype=np.uint64),
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_splice_batch(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk",
                                                                "span_off", "spans", "rep", "rep_len", "out", "cap", "out_off", "out_nbits",
                                                                "out_sym_off", "out_index", "index_cap", "dropped", "status")])


def test_host_form_refuses_bad_arguments_and_has_no_device_here(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    assert _host(mhc, None, model) == ARG and _host(mhc, model, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None),
               dict(out_sym_off=None), dict(span_off=None), dict(spans=None), dict(rep=None), dict(rep_len=256)):
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
        assert _host(mhc, model, model0, rep=None, rep_len=0) == mhc.MH_ERR_NO_DEVICE        # a deletion


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_apply_on_hand_written_cases():
    msgs = [b"hello world", b"", b"abc", b"0123456789"]
    so = np.array([0, 2, 3, 4, 8], dtype=np.uint64)
    sp = np.array([[0, 1], [6, 99], [0, 4], [1, 2], [0, 2], [2, 3], [5, 6], [10, 12]], dtype=np.uint64)
    assert splice_ref.apply(msgs, so, sp, b"[X]") == [b"[X]ello [X]", b"", b"a[X]c", b"[X][X]34[X]6789"]
    assert splice_ref.apply(msgs, so, sp, b"") == [b"ello ", b"", b"ac", b"346789"]
    assert splice_ref.apply(msgs, so, sp, b"#") == [b"#ello #", b"", b"a#c", b"##34#6789"]
    none = np.zeros(5, dtype=np.uint64)
    assert splice_ref.apply(msgs, none, np.zeros((0, 2), dtype=np.uint64), b"zz") == msgs
    # the whole message, and a span from its last byte on
    whole = np.array([0, 1, 1, 2, 3], dtype=np.uint64)
    sp2 = np.array([[0, 11], [0, 3], [9, 50]], dtype=np.uint64)
    assert splice_ref.apply(msgs, whole, sp2, b"") == [b"", b"", b"", b"012345678"]
    assert splice_ref.apply(msgs, whole, sp2, b"--") == [b"--", b"", b"--", b"012345678--"]
    assert splice_ref.offsets([b"ab", b"", b"cde"]).tolist() == [0, 2, 2, 5]


# ---- CLI rules ----------------------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "bin", "markovhuffman")
REPLACE_CASES = {
    "with_mask": (["--recode", "NEW", "--redact", "abc", "--replace", "[X]", "--mask", "0"], b"Error: --replace and --mask cannot be combined."),
    "alone": (["--recode", "NEW", "--replace", "[X]"], b"Error: --replace needs --redact or --redact-file."),
    "alone_empty": (["--recode", "NEW", "--replace", ""], b"Error: --replace needs --redact or --redact-file."),
    "too_long": (["--recode", "NEW", "--redact", "abc", "--replace", "x" * 256], b"Error: --replace takes at most 255 bytes."),
    "no_recode": (["--redact", "abc", "--replace", ""], b"Error: --redact needs --recode."),
}


@pytest.mark.parametrize("case", sorted(REPLACE_CASES))
def test_cli_replace_argument_errors(mhc, tmp_path, case):
    """The rules of --replace: checked before anything is opened, so the named files need not exist."""
    import subprocess
    cm, table, new, out = (str(tmp_path / n) for n in ("in.cm", "table", "new", "out.cm"))
    extra, want = REPLACE_CASES[case]
    args = [CLI, cm, "-x", "-e", table, "-o", out] + [new if a == "NEW" else a for a in extra]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    assert want in r.stderr, r.stderr
    assert b"opening" not in r.stderr                                      # refused before any file is touched
    assert not os.path.exists(out)
