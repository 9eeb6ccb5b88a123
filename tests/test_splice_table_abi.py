"""CPU-side checks of the table splice and the tagged span merge (include/mh.h, "SPLICING WITH A REPLACEMENT TABLE"): the
symbols are declared, exported and bound, the calls refuse bad arguments before a device is touched, the workspace is plain
arithmetic that grows by 8 bytes a replacement, mh_spans_from_hits_tagged against tests/splice_table_ref.py, that reference
against tests/splice_ref.py and hand-written cases, and the rules of --replace-file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import splice_ref
import splice_table_ref as tref
from conftest import ROOT

NEW_SYMBOLS = ["mh_spans_from_hits_tagged", "mh_dev_spans_from_hits_tagged_workspace", "mh_dev_spans_from_hits_tagged",
               "mh_dev_recode_splice_table_workspace", "mh_dev_recode_splice_table_batch", "mh_dev_recode_splice_table_each",
               "mh_recode_splice_table_batch"]


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


def test_symbols_are_declared_exported_and_bound(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    at = header.index("SPLICING WITH A REPLACEMENT TABLE (extension")
    section = header[at:header.index("SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES")]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    # what the section must say: the priority rule of a tag, the launches, what is left out
    assert "LOWEST pattern number" in section
    assert "indexed versus index-free alone" in section
    for left in ("order 2 on either side", "appending at len(x)", "replacements longer than", "back-references"):
        assert left in section[section.index("Left out:"):], left
    for name in ("dev_recode_splice_table_batch", "recode_splice_table_batch"):
        assert hasattr(mhc.Model, name), name
    assert hasattr(mhc.ModelSet, "recode_splice_table")
    assert hasattr(mhc, "dev_spans_from_hits_tagged") and hasattr(mhc, "spans_from_hits_tagged")


def test_the_workspace_grows_by_8_bytes_a_replacement(mhc):
    ws, one = mhc.lib().mh_dev_recode_splice_table_workspace, mhc.lib().mh_dev_recode_splice_workspace
    for a in [(0, 0, 1024, 0), (1, 1, 256, 1), (65536, 65536 * 4096, 1024, 65536), (7, 5000, 0, 3), (7, 5000, 300, 3)]:
        for nr in (0, 1, 5, 65536):
            assert ws(*a, nr) > 0 and ws(*a, nr) % 256 == 0, (a, nr)
            assert ws(*a, nr) >= one(*a), (a, nr)
        assert ws(*a, 1) == one(*a) == ws(*a, 0), a                              # one entry: the single replacement's two words
        grow = ws(*a, 100001) - ws(*a, 1)
        assert 800000 - 256 - 16 < grow < 800000 + 256 + 16, (a, grow)           # (the total is rounded to 256, the table to 16)
    # four bytes a span, as the splice
    assert 400000 - 256 < ws(8, 4000, 256, 100000, 4) - ws(8, 4000, 256, 0, 4) < 400000 + 256
    assert ws(8, 1 << 24, 0, 0, 3) == ws(8, 0, 0, 0, 3)


def _dev(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, dst=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             span_off=p, spans=p, span_tag=p, rep_off=p, rep_bytes=p, n_reps=2, out=p, cap=64, out_off=p, out_nbits=p, out_sym_off=p, out_index=p,
             index_cap=2, dropped=p, status=p, ws=p, wsb=1 << 16, stream=None, fn="mh_dev_recode_splice_table_batch")
    a.update(kw)
    return getattr(mhc.lib(), a["fn"])(*[a[k] for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total",
                                                        "index", "chunk", "span_off", "spans", "span_tag", "rep_off", "rep_bytes", "n_reps", "out",
                                                        "cap", "out_off", "out_nbits", "out_sym_off", "out_index", "index_cap", "dropped", "status",
                                                        "ws", "wsb", "stream")])


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
    assert _dev(mhc, src=None, dst=d, fn="mh_dev_recode_splice_table_each") == ARG
    for k in ("span_off", "span_tag", "rep_off", "out_sym_off", "payload", "pay_off", "nbits", "out_off", "out_nbits", "sym_off", "ws"):
        assert _dev(mhc, src=s, dst=d, **{k: None}) == ARG, k
    assert _dev(mhc, src=s, dst=d, index=None, sym_off=None) == ARG             # index-free: sym_off is an output
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _dev(mhc, src=s, dst=d, chunk=bad_chunk) == ARG, bad_chunk
    w = np.zeros(64, dtype=np.uint64)
    odd = ((w.ctypes.data + 255) & ~255) + 8
    for k in ("payload", "out", "ws"):
        assert _dev(mhc, src=s, dst=d, **{k: odd}) == ARG, k
    assert _dev(mhc, src=s, dst=d, wsb=64) == mhc.MH_ERR_CAPACITY
    need = mhc.lib().mh_dev_recode_splice_table_workspace(1, 100, 256, 0, 5000)
    assert _dev(mhc, src=s, dst=d, n_reps=5000, wsb=need - 256) == mhc.MH_ERR_CAPACITY  # the table's prices are part of the workspace
    m2 = _order2(mhc)
    if m2 is not None:
        assert _dev(mhc, src=m2.handle, dst=d) == ARG and _dev(mhc, src=s, dst=m2.handle) == ARG
    if mhc.device_count() == 0:
        assert _dev(mhc, src=s, dst=d) == mhc.MH_ERR_NO_DEVICE
        assert _dev(mhc, src=s, dst=d, rep_bytes=None) == mhc.MH_ERR_NO_DEVICE   # a table of deletions needs no bytes


def _host(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64), span_tag=np.array([1], dtype=np.uint32),
             rep_off=np.array([0, 0, 3], dtype=np.uint64), rep_bytes=np.frombuffer(b"[X]", dtype=np.uint8), n_reps=2,
             out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64),
             out_sym_off=np.zeros(3, dtype=np.uint64), out_index=np.zeros(4, dtype=np.uint64), index_cap=4, dropped=np.zeros(2, dtype=np.uint64),
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_splice_table_batch(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index",
                                                                      "chunk", "span_off", "spans", "span_tag", "rep_off", "rep_bytes", "n_reps",
                                                                      "out", "cap", "out_off", "out_nbits", "out_sym_off", "out_index", "index_cap",
                                                                      "dropped", "status")])


def test_host_form_refuses_bad_arguments_and_has_no_device_here(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    assert _host(mhc, None, model) == ARG and _host(mhc, model, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None),
               dict(out_sym_off=None), dict(span_off=None), dict(spans=None), dict(span_tag=None), dict(rep_off=None), dict(rep_bytes=None)):
        assert _host(mhc, model, model0, **kw) == ARG, kw
    # the table, before a device is touched: rep_off[0], decreasing offsets, 256 bytes, no entry for a span
    assert _host(mhc, model, model0, rep_off=u64(1, 1, 3)) == ARG
    assert _host(mhc, model, model0, rep_off=u64(0, 3, 2)) == ARG
    assert _host(mhc, model, model0, rep_off=u64(0, 0, 256), rep_bytes=np.zeros(256, dtype=np.uint8)) == ARG
    assert _host(mhc, model, model0, rep_off=u64(0), n_reps=0) == ARG
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, model0, chunk=bad_chunk) == ARG, bad_chunk
    assert _host(mhc, model, model0, span_off=u64(1, 1, 1)) == ARG and _host(mhc, model, model0, span_off=u64(0, 1, 0)) == ARG
    m2 = _order2(mhc)
    if m2 is not None:
        assert _host(mhc, m2, model) == ARG and _host(mhc, model, m2) == ARG
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, model0) == NO
        assert _host(mhc, model, model0, rep_off=u64(0, 0, 255), rep_bytes=np.zeros(255, dtype=np.uint8)) == NO      # the longest entry
        assert _host(mhc, model, model0, rep_off=u64(0, 0, 0), rep_bytes=None) == NO                                 # deletions only
        assert _host(mhc, model, model0, span_off=u64(0, 0, 0), rep_off=u64(0), n_reps=0) == NO                      # no span, no table


# ---- the tagged merge against the reference ------------------------------------------------------------------------------------------

def records(per):
    """Per-stream lists of (begin, end, pattern) -> (hit_off, hits[k, 3], patterns[k]) in the order of the find calls:
    ascending (stream, end, pattern)."""
    off, rec, pat = [0], [], []
    for i, lst in enumerate(per):
        for b, e, p in sorted(lst, key=lambda x: (x[1], x[2], x[0])):
            rec.append((i, b, e)); pat.append(p)
        off.append(len(rec))
    return np.array(off, dtype=np.uint64), np.array(rec, dtype=np.uint64).reshape(-1, 3), np.array(pat, dtype=np.uint32)


def check_merge(mhc, per, want=None):
    off, rec, pat = records(per)
    so, sp, tg, rc = mhc.spans_from_hits_tagged(off, rec, pat)
    r_so, r_sp, r_tg = tref.merge_tagged(off, rec, pat)
    assert rc == mhc.MH_OK and np.array_equal(so, r_so) and np.array_equal(sp, r_sp) and np.array_equal(tg, r_tg), (per, sp, tg, r_sp, r_tg)
    u_so, u_sp, rc = mhc.spans_from_hits(off, rec)
    assert rc == mhc.MH_OK and np.array_equal(u_so, so) and np.array_equal(u_sp, sp), per
    if want is not None:
        assert [(int(b), int(e), int(t)) for (b, e), t in zip(sp, tg)] == want, (per, sp, tg)


def test_tagged_merge_on_crafted_lists(mhc):
    # a longer lower-priority pattern swallows a shorter higher-priority one: the span is the longer one's, the tag the shorter one's
    check_merge(mhc, [[(10, 30, 5), (15, 18, 1)]], [(10, 30, 1)])
    # the reverse: a longer higher-priority pattern over a shorter lower-priority one
    check_merge(mhc, [[(10, 30, 1), (15, 18, 5)]], [(10, 30, 1)])
    # the lower number ends first, or last, or begins first
    check_merge(mhc, [[(0, 5, 7), (3, 9, 2), (8, 12, 4)]], [(0, 12, 2)])
    check_merge(mhc, [[(0, 5, 2), (3, 9, 7), (8, 12, 4)]], [(0, 12, 2)])
    check_merge(mhc, [[(0, 5, 9), (3, 9, 7), (8, 12, 0)]], [(0, 12, 0)])
    # touching records merge; a gap of one byte does not
    check_merge(mhc, [[(0, 5, 3), (5, 9, 1), (10, 12, 2)]], [(0, 9, 1), (10, 12, 2)])
    # the same interval under two patterns; streams apart; an empty stream between two others
    check_merge(mhc, [[(4, 8, 6), (4, 8, 2)], [], [(4, 8, 6)]], [(4, 8, 2), (4, 8, 6)])
    check_merge(mhc, [[], [], []], [])
    # a late long record reaches back over several spans-to-be
    check_merge(mhc, [[(0, 2, 4), (5, 7, 3), (10, 12, 2), (1, 20, 9), (30, 31, 0)]], [(0, 20, 2), (30, 31, 0)])
    # more than one tile of 256 records in a stream, one span over a tile boundary
    per = [[(3 * k, 3 * k + 2, 100 + k % 7) for k in range(600)] + [(700, 900, 50)]]
    check_merge(mhc, per)
    off, rec, pat = records(per)
    assert mhc.spans_from_hits_tagged(off, rec, pat)[2].min() == 50


def test_tagged_merge_on_200_random_lists(mhc):
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 5))
        per = []
        for _ in range(n):
            k = int(rng.integers(0, 40)) if seed % 10 else int(rng.integers(250, 600))
            span = int(rng.choice([50, 400, 5000]))
            per.append([(int(b), int(b) + int(rng.integers(1, 12)), int(rng.integers(0, 6))) for b in rng.integers(0, span, size=k)])
        check_merge(mhc, per)


def test_tagged_merge_refusals(mhc):
    lib = mhc.lib()
    off, rec, pat = records([[(0, 5, 3), (5, 9, 1)], [(1, 2, 0)]])
    so, sp, tg = np.full(3, 7, dtype=np.uint64), np.zeros(6, dtype=np.uint64), np.zeros(3, dtype=np.uint32)
    call = lambda **kw: lib.mh_spans_from_hits_tagged(*[kw.get(k, v) for k, v in (("off", off.ctypes.data), ("rec", rec.ctypes.data),
                                                                                 ("pat", pat.ctypes.data), ("cap", 3), ("n", 2), ("so", so.ctypes.data),
                                                                                 ("sp", sp.ctypes.data), ("tg", tg.ctypes.data))])
    assert call() == mhc.MH_OK and so.tolist() == [0, 1, 2] and tg[:2].tolist() == [1, 0]
    assert call(pat=None) == mhc.MH_ERR_ARG and call(off=None) == mhc.MH_ERR_ARG and call(so=None) == mhc.MH_ERR_ARG and call(tg=None) == mhc.MH_ERR_ARG
    assert call(cap=2) == mhc.MH_ERR_CAPACITY and so.tolist() == [0, 0, 0]                  # the search overflowed: as the untagged call
    bad = np.array([0, 3, 2], dtype=np.uint64)
    assert call(off=bad.ctypes.data) == mhc.MH_ERR_ARG
    w = np.zeros(1 << 10, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    dev = lambda **kw: lib.mh_dev_spans_from_hits_tagged(*[kw.get(k, v) for k, v in (("off", p), ("rec", p), ("pat", p), ("cap", 4), ("n", 2), ("so", p),
                                                                                    ("sp", p), ("tg", p), ("ws", p), ("wsb", 1 << 12), ("st", None))])
    for k in ("off", "rec", "pat", "so", "sp", "tg", "ws"):
        assert dev(**{k: None}) == mhc.MH_ERR_ARG, k
    assert dev(ws=p + 8) == mhc.MH_ERR_ARG and dev(wsb=64) == mhc.MH_ERR_CAPACITY
    assert lib.mh_dev_spans_from_hits_tagged_workspace(2, 1000) == lib.mh_dev_spans_from_hits_workspace(2, 1000)
    if mhc.device_count() == 0:
        assert dev() == mhc.MH_ERR_NO_DEVICE


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_equals_the_single_replacement_reference_at_one_entry():
    msgs = [b"hello world", b"", b"abc", b"0123456789"]
    so = np.array([0, 2, 3, 4, 8], dtype=np.uint64)
    sp = np.array([[0, 1], [6, 99], [0, 4], [1, 2], [0, 2], [2, 3], [5, 6], [10, 12]], dtype=np.uint64)
    zeros = np.zeros(len(sp), dtype=np.uint32)
    for rep in (b"[X]", b"", b"#", bytes(255)):
        assert tref.apply(msgs, so, sp, zeros, [rep]) == splice_ref.apply(msgs, so, sp, rep)
    rng = np.random.default_rng(3)
    for _ in range(50):
        batch = [bytes(rng.integers(97, 123, size=int(rng.integers(0, 60)), dtype=np.uint8)) for _ in range(3)]
        per = []
        for m in batch:
            cuts = sorted(set(int(x) for x in rng.integers(0, 80, size=int(rng.integers(0, 8)) * 2)))
            per.append([(cuts[k], cuts[k + 1]) for k in range(0, len(cuts) - 1, 2)])
        off = np.zeros(4, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in per])
        flat = np.array([x for p in per for x in p], dtype=np.uint64).reshape(-1, 2)
        assert tref.apply(batch, off, flat, np.zeros(len(flat), dtype=np.uint32), [b"<>"]) == splice_ref.apply(batch, off, flat, b"<>")


def test_reference_apply_on_hand_written_cases():
    msgs = [b"hello world", b"", b"abc"]
    reps = [b"", b"#", b"<IP>"]
    off, sp, tg = tref.tagged_lists([[(0, 0, 1), (0, 1, 2), (5, 5, 2), (5, 6, 0), (6, 6, 1), (11, 11, 1)], [(0, 0, 2)],
                                     [(1, 1, 1), (1, 1, 2), (1, 2, 0), (2, 9, 1), (3, 3, 2)]])
    assert tref.apply(msgs, off, sp, tg, reps) == [b"#<IP>ello<IP>#world", b"", b"a#<IP>#"]
    assert tref.well_formed([(0, 0), (0, 3), (3, 3), (3, 4)]) and not tref.well_formed([(2, 5), (2, 2)]) and not tref.well_formed([(4, 3)])
    assert tref.offsets([b"ab", b"", b"cde"]).tolist() == [0, 2, 2, 5]


# ---- CLI rules ----------------------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "bin", "markovhuffman")


def run_cli(tmp_path, extra, files):
    cm, table, new, out = (str(tmp_path / n) for n in ("in.cm", "table", "new", "out.cm"))
    for name, blob in files.items():
        with open(str(tmp_path / name), "wb") as f:
            f.write(blob)
    args = [CLI, cm, "-x", "-e", table, "-o", out] + [str(tmp_path / a[1:]) if a.startswith("@") else a for a in extra]
    r = subprocess.run(args, capture_output=True, timeout=60)
    return r, out


RULES = {
    "with_replace": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps", "--replace", "[X]"], {},
                     b"Error: --replace-file cannot be combined with --replace or --mask."),
    "with_mask": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps", "--mask", "0"], {},
                  b"Error: --replace-file cannot be combined with --replace or --mask."),
    "with_redact_strings": (["--recode", "@new", "--redact", "abc", "--replace-file", "@reps"], {}, b"Error: --replace-file needs --redact-file."),
    "alone": (["--recode", "@new", "--replace-file", "@reps"], {}, b"Error: --replace-file needs --redact-file."),
    "no_recode": (["--redact-file", "@pats", "--replace-file", "@reps"], {}, b"Error: --redact needs --recode."),
    "fewer_lines": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\ndef\nghi\n", "reps": b"A\nB\n"},
                    b"holds 2 lines for 3 patterns."),
    "more_lines": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\ndef\n", "reps": b"A\nB\n\n"},
                   b"holds 3 lines for 2 patterns."),
    # an empty pattern line is skipped, an empty replacement line is kept: three lines here, two patterns
    "empty_lines_are_kept": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\n\ndef\n", "reps": b"A\n\nB"},
                             b"holds 3 lines for 2 patterns."),
    "too_long": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\ndef\n", "reps": b"A\n" + b"x" * 256 + b"\n"},
                 b"Error: a line of the --replace-file takes at most 255 bytes."),
    "missing_file": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\n"}, b"Error: cannot open the --replace-file"),
}


@pytest.mark.parametrize("case", sorted(RULES))
def test_cli_replace_file_argument_errors(mhc, tmp_path, case):
    """The rules of --replace-file: checked before the input, the tables or a device are touched, so those files need not exist."""
    extra, files, want = RULES[case]
    r, out = run_cli(tmp_path, extra, files)
    assert r.returncode == 1 and r.stdout == b""
    assert want in r.stderr, r.stderr
    assert b"opening" not in r.stderr
    assert not os.path.exists(out)


def test_cli_replace_file_keeps_empty_lines_and_a_final_lf_adds_none(mhc, tmp_path):
    """Counts that match pass the rules: the run then fails later, at the input that does not exist.  "A\\n\\nB\\n" is three lines
    (the empty one deletes), "A\\n\\nB" the same three, "\\n\\n\\n" three empty ones."""
    for reps in (b"A\n\nB\n", b"A\n\nB", b"\n\n\n", b"\n\nB"):
        r, out = run_cli(tmp_path, ["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps"], {"pats": b"abc\ndef\nghi\n", "reps": reps})
        later = b"opening" in r.stderr or b"no usable HIP device" in r.stderr    # (without a device the run ends before the input is opened)
        assert r.returncode == 1 and b"--replace-file" not in r.stderr and later, (reps, r.stderr)
