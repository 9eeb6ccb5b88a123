"""CPU-side checks of the span-token calls (include/mh.h, "TOKENS FROM MATCHED BYTES"): the symbols are declared, exported and
bound, the argument block mirrors the header, struct_size is handled as the other blocks handle it, and both forms refuse bad
arguments before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_span_token_digest", "mh_dev_span_tokens_workspace", "mh_dev_span_tokens_batch", "mh_span_tokens_batch"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


def section_of():
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    at = header.index("TOKENS FROM MATCHED BYTES (extension")
    return header, header[at:header.index("SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES")]


def test_symbols_are_declared_exported_and_bound(mhc):
    header, section = section_of()
    lib = C.CDLL(mhc.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    assert "#define MH_TOKEN_FOLD 1u" in section and mhc.TOKEN_FOLD == 1
    assert re.search(r"int mh_dev_span_tokens_batch\(const mh_span_tokens_args \*a, const mh_launch \*launch\);", section)
    for said in ("ONLY THE STREAMS WITH SPANS ARE DECODED", "no allocation and no host synchronisation", "Known limit"):
        assert said in section, said
    for left in ("back-references and capture groups", "tokens over MH_SPLICE_MAX_REP", "de-duplicating equal table entries"):
        assert left in section[section.index("Left out:"):], left
    # the older sections no longer say that nothing is computed from the matched bytes
    assert "any replacement computed from the matched bytes" not in header
    assert hasattr(mhc, "span_tokens_args") and hasattr(mhc, "SpanTokensArgs") and hasattr(mhc, "launch_args")


def test_the_block_mirrors_the_header(mhc):
    _, section = section_of()
    body = re.search(r"typedef struct mh_span_tokens_args \{(.*?)\} mh_span_tokens_args;", section, flags=re.S).group(1)
    names = [re.search(r"(\w+)(\[16\])?;", line).group(1) for line in body.strip().splitlines()]
    assert names == [f[0] for f in mhc.SpanTokensArgs._fields_]
    # 4 + 2 pointers (padded) | the batch | 3 pointers | key 16 | flags (padded) | 3 pointers | 2 sizes | 2 pointers | size | 2 pointers
    assert C.sizeof(mhc.SpanTokensArgs) == 8 + 16 + C.sizeof(mhc.CodedBatchArgs) + 24 + 16 + 8 + 24 + 16 + 16 + 8 + 16


def test_the_workspace_is_plain_arithmetic(mhc):
    ws = mhc.lib().mh_dev_span_tokens_workspace
    for n in (0, 1, 65536):
        for r in (0, 1, 1000, 65536, 1 << 20):
            assert ws(n, r) > 0 and ws(n, r) % 256 == 0 and ws(n, r) == ws(0, r), (n, r)
    grow = ws(8, 100001) - ws(8, 1)
    assert 800000 - 256 < grow < 800000 + 1024 + 256, grow                      # 8 bytes an entry and the scan's block sums


def _dev(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, src_set=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, sym_off=p, sym_total=100, index=p, chunk=256, prev0=0x20,
             span_off=p, spans=p, span_tag=p, key=bytes(16), flags=0, fmt_off=p, fmt_bytes=p, hex_digits=p, n_formats=1, n_reps=2, rep_off=p,
             rep_bytes=p, rep_cap=64, rep_tag=p, status=p, ws=p, wsb=1 << 16, stream=None, size=None, null_block=False, null_launch=False)
    a.update(kw)
    blk = mhc.span_tokens_args(a["src"], a["src_set"], (a["payload"], a["pay_off"], a["nbits"], a["n"], a["pay_total"], a["sym_off"], a["sym_total"],
                                                      a["index"], a["chunk"], a["prev0"]), a["span_off"], a["spans"], a["span_tag"], a["key"],
                               a["flags"], a["fmt_off"], a["fmt_bytes"], a["hex_digits"], a["n_formats"], a["n_reps"], a["rep_off"], a["rep_bytes"],
                               a["rep_cap"], a["rep_tag"], a["status"])
    if a["size"] is not None:
        blk.struct_size = a["size"]
    launch = mhc.launch_args(a["ws"], a["wsb"], a["stream"])
    return mhc.lib().mh_dev_span_tokens_batch(None if a["null_block"] else C.byref(blk), None if a["null_launch"] else C.byref(launch)), w


def dev(mhc, **kw):
    return _dev(mhc, **kw)[0]


def _order2(mhc):
    try:
        return mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0
        return None


def test_device_form_refuses_bad_arguments_before_any_launch(mhc, model):
    ARG = mhc.MH_ERR_ARG
    s = model.handle
    here = mhc.MH_ERR_NO_DEVICE if mhc.device_count() == 0 else None
    assert dev(mhc, src=s, null_block=True) == ARG and dev(mhc, src=s, null_launch=True) == ARG
    # struct_size: exactly sizeof of the struct, as the other blocks
    size = C.sizeof(mhc.SpanTokensArgs)
    for bad in (0, size - 8, size + 8, 4):
        assert dev(mhc, src=s, size=bad) == ARG, bad
    # exactly one of src and src_set
    assert dev(mhc) == ARG and dev(mhc, src=s, src_set=s) == ARG
    assert dev(mhc, src=s, flags=2) == ARG and dev(mhc, src=s, flags=3) == ARG
    for k in ("span_off", "spans", "rep_off", "rep_tag", "status", "fmt_off", "hex_digits", "payload", "pay_off", "nbits", "sym_off", "ws"):
        assert dev(mhc, src=s, **{k: None}) == ARG, k
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert dev(mhc, src=s, chunk=bad_chunk) == ARG, bad_chunk
    w = np.zeros(64, dtype=np.uint64)
    odd = ((w.ctypes.data + 255) & ~255) + 8
    for k in ("payload", "ws"):
        assert dev(mhc, src=s, **{k: odd}) == ARG, k
    assert dev(mhc, src=s, wsb=64) == mhc.MH_ERR_CAPACITY
    need = mhc.lib().mh_dev_span_tokens_workspace(1, 5000)
    assert dev(mhc, src=s, n_reps=5000, wsb=need - 256) == mhc.MH_ERR_CAPACITY
    if here is not None:
        assert dev(mhc, src=s) == here
        assert dev(mhc, src=s, n_reps=5000, wsb=need) == here
        assert dev(mhc, src=s, span_tag=None) == here and dev(mhc, src=s, rep_bytes=None) == here      # format 0; count only
        assert dev(mhc, src=s, index=None, sym_off=None, chunk=0) == here                               # index-free
        assert dev(mhc, src=s, flags=mhc.TOKEN_FOLD) == here
        assert dev(mhc, src=s, n_formats=0, hex_digits=None, n_reps=0, spans=None, rep_tag=None) == here
        m2 = _order2(mhc)
        assert m2 is None or dev(mhc, src=m2.handle) == here


def _host(mhc, src, **kw):
    a = dict(src=src.handle if src is not None else None, payload=np.zeros(32, dtype=np.uint8), pay_off=np.array([0, 16, 32], dtype=np.uint64),
             nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20, sym_off=np.array([0, 100, 200], dtype=np.uint64),
             index=np.zeros(4, dtype=np.uint64), chunk=256, span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64),
             span_tag=np.array([1], dtype=np.uint32), key=np.arange(16, dtype=np.uint8), flags=0, fmt_off=np.array([0, 1, 2, 6, 6], dtype=np.uint64),
             fmt_bytes=np.frombuffer(b"<><IP>", dtype=np.uint8), hex_digits=np.array([16, 0], dtype=np.uint8), n_formats=2,
             rep_off=np.zeros(2, dtype=np.uint64), rep_bytes=np.zeros(64, dtype=np.uint8), rep_cap=64, rep_tag=np.zeros(1, dtype=np.uint32),
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_span_tokens_batch(*[p(a[k]) for k in ("src", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "span_off",
                                                              "spans", "span_tag", "key", "flags", "fmt_off", "fmt_bytes", "hex_digits", "n_formats",
                                                              "rep_off", "rep_bytes", "rep_cap", "rep_tag", "status")])


def test_host_form_checks_every_rule_before_a_device_is_needed(mhc, model):
    ARG = mhc.MH_ERR_ARG
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    u8 = lambda *v: np.array(v, dtype=np.uint8)
    assert _host(mhc, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(span_off=None), dict(spans=None), dict(key=None), dict(fmt_off=None),
               dict(fmt_bytes=None), dict(hex_digits=None), dict(rep_off=None), dict(rep_tag=None), dict(sym_off=None), dict(flags=2)):
        assert _host(mhc, model, **kw) == ARG, kw
    # the formats: fmt_off[0], decreasing offsets, 17 digits, 256 bytes in all, spans and no format
    assert _host(mhc, model, fmt_off=u64(1, 1, 2, 6, 6)) == ARG
    assert _host(mhc, model, fmt_off=u64(0, 2, 1, 6, 6)) == ARG and _host(mhc, model, fmt_off=u64(0, 1, 2, 6, 5)) == ARG
    assert _host(mhc, model, hex_digits=u8(17, 0)) == ARG and _host(mhc, model, hex_digits=u8(16, 255)) == ARG
    long_bytes = np.zeros(256, dtype=np.uint8)
    assert _host(mhc, model, fmt_off=u64(0, 200, 240, 240, 240), fmt_bytes=long_bytes, hex_digits=u8(16, 0)) == ARG        # 256 bytes
    assert _host(mhc, model, fmt_off=u64(0, 0, 0, 100, 256), fmt_bytes=long_bytes, hex_digits=u8(16, 0)) == ARG           # 256 without a digit
    assert _host(mhc, model, fmt_off=u64(0), n_formats=0, hex_digits=None, fmt_bytes=None) == ARG                          # a span and no format
    # the batch and the span offsets
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, chunk=bad_chunk) == ARG, bad_chunk
    assert _host(mhc, model, pay_off=u64(0, 16, 8)) == ARG and _host(mhc, model, nbits=u64(129, 128)) == ARG
    assert _host(mhc, model, span_off=u64(1, 1, 1)) == ARG and _host(mhc, model, span_off=u64(0, 1, 0)) == ARG
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model) == NO
        assert _host(mhc, model, fmt_off=u64(0, 200, 239, 239, 239), fmt_bytes=long_bytes, hex_digits=u8(16, 0)) == NO     # exactly 255 bytes
        assert _host(mhc, model, span_tag=None) == NO and _host(mhc, model, rep_bytes=None) == NO and _host(mhc, model, status=None) == NO
        assert _host(mhc, model, index=None, sym_off=None) == NO and _host(mhc, model, flags=1) == NO
        assert _host(mhc, model, span_off=u64(0, 0, 0), spans=None, rep_tag=None, fmt_off=u64(0), n_formats=0, hex_digits=None, fmt_bytes=None) == NO


def test_the_digest_refuses_null_pointers_quietly(mhc):
    lib = mhc.lib()
    k = np.arange(16, dtype=np.uint8)
    assert lib.mh_span_token_digest(None, k.ctypes.data, 4, 0) == 0 and lib.mh_span_token_digest(k.ctypes.data, None, 4, 0) == 0
    assert lib.mh_span_token_digest(k.ctypes.data, None, 0, 0) == 0x726fdb47dd0e0e31


# ---- CLI rules ----------------------------------------------------------------------------------------------------------------

import subprocess  # noqa: E402

CLI = os.path.join(ROOT, "bin", "markovhuffman")
KEYHEX = "000102030405060708090a0b0c0d0e0f"
RULES = {
    "alone": (["--recode", "@new", "--redact", "abc", "--token-key", KEYHEX], {}, b"Error: --token-key needs --replace or --replace-file."),
    "short_key": (["--recode", "@new", "--redact", "abc", "--replace", "<%H>", "--token-key", KEYHEX[:-1]], {}, b"Error: --token-key takes 32 hex digits."),
    "not_hex": (["--recode", "@new", "--redact", "abc", "--replace", "<%H>", "--token-key", KEYHEX[:-1] + "g"], {}, b"Error: --token-key takes 32 hex digits."),
    "too_long": (["--recode", "@new", "--redact", "abc", "--replace", "x" * 238 + "<%H>", "--token-key", KEYHEX], {},
                 b"Error: --replace takes at most 255 bytes, the token's digits included."),
    "too_long_line": (["--recode", "@new", "--redact-file", "@pats", "--replace-file", "@reps", "--token-key", KEYHEX],
                      {"pats": b"abc\ndef\n", "reps": b"A\n" + b"x" * 252 + b"%4H\n"}, b"Error: a line of the --replace-file takes at most 255 bytes, the token's digits included."),
    "order2": (["--order2", "--recode", "@new", "--redact", "abc", "--replace", "<%H>", "--token-key", KEYHEX], {}, b"Error: --recode does not support --order2."),
}


@pytest.mark.parametrize("case", sorted(RULES))
def test_cli_token_key_argument_errors(mhc, tmp_path, case):
    """The rules of --token-key: checked before the input, the tables or a device are touched, so those files need not exist."""
    extra, files, want = RULES[case]
    for name, blob in files.items():
        with open(str(tmp_path / name), "wb") as f:
            f.write(blob)
    out = str(tmp_path / "out.cm")
    args = [CLI, str(tmp_path / "in.cm"), "-x", "-e", str(tmp_path / "table"), "-o", out] + [str(tmp_path / a[1:]) if a.startswith("@") else a for a in extra]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and want in r.stderr, r.stderr
    assert b"opening" not in r.stderr and not os.path.exists(out)


def test_cli_token_key_lengths_that_fit_pass_the_rules(mhc, tmp_path):
    """237 bytes and <%H>: 255 in all; %0H, %17H and %H without the key are literal text.  The run then fails later, at the input."""
    for rep in ("x" * 237 + "<%H>", "x" * 250 + "%0H", "x" * 250 + "%17H"):
        args = [CLI, str(tmp_path / "in.cm"), "-x", "-e", str(tmp_path / "t"), "-o", str(tmp_path / "o"), "--recode", str(tmp_path / "n"), "--redact", "abc",
                "--replace", rep, "--token-key", KEYHEX]
        r = subprocess.run(args, capture_output=True, timeout=60)
        later = b"opening" in r.stderr or b"no usable HIP device" in r.stderr
        assert r.returncode == 1 and b"--replace" not in r.stderr and b"--token-key" not in r.stderr and later, (rep, r.stderr)
