"""CPU-side checks of re-coding (include/mh.h, "RE-CODING BATCHES"): the symbols are declared, exported and bound, the
workspace functions are plain arithmetic inside the documented cap, the compute calls refuse bad arguments before a device is
touched, and the Python reference (tests/recode_ref.py) against hand-written cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import recode_ref
from conftest import ROOT
from oracle import mh_oracle

NEW_SYMBOLS = ["mh_dev_histogram_coded_workspace", "mh_dev_histogram_coded_batch", "mh_dev_histogram_coded_each",
               "mh_dev_recode_batch_workspace", "mh_dev_recode_batch", "mh_dev_recode_each", "mh_recode_batch"]
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


def test_recode_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    at = header.index("RE-CODING BATCHES")
    assert header.index("SEARCH IN BATCHES") < at < header.index("SEGMENT STATES OF INDEX-FREE BATCHES")
    section = header[at:header.index("SEGMENT STATES OF INDEX-FREE BATCHES")]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name


def test_workspaces_are_plain_arithmetic_inside_the_cap(mhc):
    lib = mhc.lib()
    for n, total, chunk in [(0, 0, 1024), (1, 1, 256), (65536, 65536 * 4096, 1024), (3, 1 << 34, 8192), (1 << 20, 1 << 20, 256), (7, 12345, 0)]:
        w = lib.mh_dev_recode_batch_workspace(n, total, chunk)
        h = lib.mh_dev_histogram_coded_workspace(n, total, chunk)
        cap = 64 * (lib.mh_batch_index_capacity(total, n, chunk) + n) + (64 << 10)
        assert 0 < w <= cap and 0 < h <= cap, (n, total, chunk, w, h, cap)
        assert w == lib.mh_dev_recode_batch_workspace(n, total, chunk) and w % 256 == 0 and h % 256 == 0
    # per chunk number and per stream: grows with both, and a bad chunk size counts as index-free
    assert lib.mh_dev_recode_batch_workspace(100, 1 << 30, 1024) > lib.mh_dev_recode_batch_workspace(100, 1 << 20, 1024)
    assert lib.mh_dev_recode_batch_workspace(100, 1 << 30, 300) == lib.mh_dev_recode_batch_workspace(100, 1 << 30, 0)
    # 65 536 x 4 KiB at chunk 1024: a few MiB against the 256 MiB buffer of the decoded bytes
    assert lib.mh_dev_recode_batch_workspace(65536, 65536 * 4096, 1024) < 8 << 20


# (n_streams, sym_total, chunk_symbols) -> what each workspace function returned before the re-coders of all orders became one
# kernel family: the layouts are part of the ABI (a caller may have sized a pool by them), 300 is not a valid chunk size
PINNED_ARGS = [(0, 0, 256), (1, 1, 256), (7, 5000, 256), (7, 5000, 0), (7, 5000, 300), (65536, 1 << 28, 1024)]
PINNED_WORKSPACES = {
    "mh_dev_recode_batch_workspace": [256, 256, 512, 256, 256, 4197120],
    "mh_dev_recode_batch_o2_workspace": [256, 256, 768, 256, 256, 6818560],
    "mh_dev_histogram_coded_workspace": [256, 256, 256, 256, 256, 262400],
    "mh_dev_histogram_coded_batch_o2_workspace": [256, 256, 256, 256, 256, 262400],
}


def test_workspace_sizes_are_pinned(mhc):
    for name, want in PINNED_WORKSPACES.items():
        fn = getattr(mhc.lib(), name)
        assert [fn(*a) for a in PINNED_ARGS] == want, name


def _dev_recode(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, dst=None, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             out=p, cap=64, out_off=p, out_nbits=p, out_index=p, dropped=p, status=p, ws=p, wsb=1 << 16, stream=None, fn="mh_dev_recode_batch")
    a.update(kw)
    return getattr(mhc.lib(), a["fn"])(*[a[k] for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total",
                                                        "index", "chunk", "out", "cap", "out_off", "out_nbits", "out_index", "dropped", "status",
                                                        "ws", "wsb", "stream")])


def _dev_hist(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = dict(src=None, order=1, payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256,
             counts=p, status=p, ws=p, wsb=1 << 16, stream=None, fn="mh_dev_histogram_coded_batch")
    a.update(kw)
    return getattr(mhc.lib(), a["fn"])(*[a[k] for k in ("src", "order", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total",
                                                        "index", "chunk", "counts", "status", "ws", "wsb", "stream")])


def _order2(mhc):
    try:
        return mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0
        return None


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    s, d = model.handle, model0.handle
    assert _dev_recode(mhc, src=None, dst=d) == ARG and _dev_recode(mhc, src=s, dst=None) == ARG
    assert _dev_recode(mhc, src=None, dst=d, fn="mh_dev_recode_each") == ARG
    assert _dev_hist(mhc, src=None) == ARG and _dev_hist(mhc, src=None, fn="mh_dev_histogram_coded_each") == ARG
    for order in (-1, 2, 7):
        assert _dev_hist(mhc, src=s, order=order) == ARG, order
    for k in ("payload", "pay_off", "nbits", "out_off", "out_nbits", "sym_off", "ws"):
        assert _dev_recode(mhc, src=s, dst=d, **{k: None}) == ARG, k
    for k in ("payload", "pay_off", "nbits", "counts", "sym_off", "ws"):
        assert _dev_hist(mhc, src=s, **{k: None}) == ARG, k
    assert _dev_recode(mhc, src=s, dst=d, index=None, sym_off=None) == ARG        # index-free: sym_off is an output
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _dev_recode(mhc, src=s, dst=d, chunk=bad_chunk) == ARG, bad_chunk
        assert _dev_hist(mhc, src=s, chunk=bad_chunk) == ARG, bad_chunk
    assert _dev_recode(mhc, src=s, dst=d, index=None, chunk=300) == ARG            # the destination index's chunk
    w = np.zeros(64, dtype=np.uint64)
    odd = ((w.ctypes.data + 255) & ~255) + 8
    for k in ("payload", "out", "ws"):
        assert _dev_recode(mhc, src=s, dst=d, **{k: odd}) == ARG, k
    assert _dev_recode(mhc, src=s, dst=d, wsb=64) == mhc.MH_ERR_CAPACITY
    assert _dev_hist(mhc, src=s, wsb=64) == mhc.MH_ERR_CAPACITY
    m2 = _order2(mhc)
    if m2 is not None:
        assert _dev_recode(mhc, src=m2.handle, dst=d) == ARG and _dev_recode(mhc, src=s, dst=m2.handle) == ARG
        assert _dev_hist(mhc, src=m2.handle) == ARG
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert _dev_recode(mhc, src=s, dst=d) == NO and _dev_recode(mhc, src=d, dst=s, out=None, out_index=None, dropped=None, status=None) == NO
        assert _dev_recode(mhc, src=s, dst=d, index=None, chunk=0, out_index=None) == NO
        assert _dev_hist(mhc, src=s) == NO and _dev_hist(mhc, src=d, order=0, index=None, sym_off=None, chunk=0, status=None) == NO


def test_a_set_must_have_one_model_per_stream(mhc, model, model0):
    try:
        ms = mhc.ModelSet.from_models([model, model0, model])
    except mhc.MhError as e:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0       # tests/test_gpu_recode.py has the refusal on the card
        return
    for n in (1, 2, 4):
        assert _dev_recode(mhc, src=ms.handle, dst=model.handle, n=n, fn="mh_dev_recode_each") == mhc.MH_ERR_ARG
        assert _dev_hist(mhc, src=ms.handle, n=n, fn="mh_dev_histogram_coded_each") == mhc.MH_ERR_ARG


def _host(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256, out=np.zeros(64, dtype=np.uint8),
             cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64), out_index=np.zeros(4, dtype=np.uint64),
             dropped=np.zeros(2, dtype=np.uint64), status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_batch(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "out",
                                                         "cap", "out_off", "out_nbits", "out_index", "dropped", "status")])


def test_host_form_refuses_bad_arguments_before_touching_a_device(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    assert _host(mhc, None, model) == ARG and _host(mhc, model, None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None)):
        assert _host(mhc, model, model0, **kw) == ARG, kw
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, model0, chunk=bad_chunk) == ARG, bad_chunk
        assert _host(mhc, model, model0, index=None, chunk=bad_chunk) == ARG, bad_chunk     # the destination index's chunk
    assert _host(mhc, model, model0, pay_off=np.array([1, 16, 32], dtype=np.uint64)) == ARG
    assert _host(mhc, model, model0, pay_off=np.array([0, 16, 8], dtype=np.uint64)) == ARG
    assert _host(mhc, model, model0, nbits=np.array([129, 128], dtype=np.uint64)) == ARG    # nbits past its bytes
    assert _host(mhc, model, model0, sym_off=np.array([0, 100, 50], dtype=np.uint64)) == ARG
    m2 = _order2(mhc)
    if m2 is not None:
        assert _host(mhc, m2, model) == ARG and _host(mhc, model, m2) == ARG
    if mhc.device_count() == 0:
        assert _host(mhc, model, model0) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model0, model, out=None, out_index=None, dropped=None, status=None) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, model0, index=None, out_index=None, chunk=0) == mhc.MH_ERR_NO_DEVICE
        with pytest.raises(mhc.MhError) as e:
            model.recode_batch(model0, np.zeros(32, dtype=np.uint8), [0, 16, 32], [120, 128])
        assert e.value.status == mhc.MH_ERR_NO_DEVICE


@pytest.mark.parametrize("case", ["no_x", "no_e", "no_o", "with_find", "with_range", "order2"])
def test_cli_recode_argument_errors(mhc, tmp_path, case):
    """The rules of --recode: checked before anything is opened, so the named files need not exist."""
    cm, table, new, idx, out = (str(tmp_path / n) for n in ("in.cm", "table", "new", "f.idx", "out.cm"))
    args = {
        "no_x": [CLI, cm, "-e", table, "-o", out, "--recode", new],
        "no_e": [CLI, cm, "-x", "-o", out, "--recode", new],
        "no_o": [CLI, cm, "-x", "-e", table, "--recode", new],
        "with_find": [CLI, cm, "-x", "-e", table, "-o", out, "--recode", new, "--index", idx, "--find", "abc"],
        "with_range": [CLI, cm, "-x", "-e", table, "-o", out, "--recode", new, "--index", idx, "--range", "0:3"],
        "order2": [CLI, cm, "-x", "-e", table, "-o", out, "--recode", new, "--order2"],
    }[case]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    want = {"no_x": b"Error: --recode needs -x, -e and -o.", "no_e": b"Error: --recode needs -x, -e and -o.",
            "no_o": b"Error: --recode needs -x, -e and -o.", "with_find": b"Error: --recode cannot be combined with --find or --range.",
            "with_range": b"Error: --recode cannot be combined with --find or --range.", "order2": b"Error: --recode does not support --order2."}[case]
    assert want in r.stderr, r.stderr
    assert b"opening" not in r.stderr                                      # refused before any file is touched
    assert not os.path.exists(out)


# ---- the reference against hand-written cases -------------------------------------------------------------------------------

def _toy_model():
    """Order 1: after ' ' (prev0) and after 'a': a -> 0, b -> 10, c -> 11 (counts 4, 2, 1... ties aside, checked below);
    after 'b': only 'a'.  No other context has a code."""
    counts = np.zeros(65536, dtype=np.uint64)
    for prev in (0x20, ord("a")):
        counts[prev * 256 + ord("a")] = 5
        counts[prev * 256 + ord("b")] = 2
        counts[prev * 256 + ord("c")] = 1
    counts[ord("b") * 256 + ord("a")] = 3
    return mh_oracle.Model.from_counts(counts, 1)


def test_reference_codes_a_hand_written_message():
    m = _toy_model()
    lens, codes = m.codes()
    assert [int(lens[0x20 * 256 + c]) for c in b"abc"] == [1, 2, 2] and int(lens[ord("b") * 256 + ord("a")]) == 1
    assert int(lens[ord("c") * 256 + ord("a")]) == 0                             # context 'c' has no codes at all
    (payload, nbits, drop, idx), = recode_ref.recode([b"aaba"], m, chunk=256)
    assert (nbits, drop) == (1 + 1 + 2 + 1, 0) and len(payload) == 1
    bits = "".join(format(int(codes[p * 256 + s]), "0%db" % int(lens[p * 256 + s])) for p, s in zip(b" aab", b"aaba"))
    assert format(payload[0], "08b") == bits.ljust(8, "0")
    assert idx.tolist() == [0x20 << 56]


def test_reference_skips_a_pair_without_a_code_and_advances_the_context():
    m = _toy_model()
    lens, _ = m.codes()
    # 'c' 'a': the pair (c, a) has no code, 'a' is skipped, and the next symbol is coded in context 'a' all the same
    (payload, nbits, drop, _), = recode_ref.recode([b"acab"], m)
    assert drop == 1 and nbits == 1 + 2 + 0 + 2
    assert recode_ref.dropped(lens, b"acab", 1) == 1 and recode_ref.dropped(lens, b"xyz", 1) == 3
    assert recode_ref.code_lengths(lens, b"acab", 1).tolist() == [1, 2, 0, 2]
    (p2, n2, d2, _), = recode_ref.recode([b"xyz"], m)
    assert (p2, n2, d2) == (b"", 0, 3)
    pay, off, nb, dr = recode_ref.packed(recode_ref.recode([b"acab", b"", b"xyz", b"ab"], m))
    assert off.tolist() == [0, 1, 1, 1, 2] and nb.tolist() == [5, 0, 0, 3] and dr.tolist() == [1, 0, 3, 0] and pay.size == 2


def test_reference_index_entries_carry_the_byte_in_front_of_the_chunk():
    m = mh_oracle.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)          # every code 8 bits
    msg = bytes(range(256)) * 3
    (_, nbits, drop, idx), = recode_ref.recode([msg], m, chunk=256)
    assert nbits == 8 * 768 and drop == 0
    assert idx.tolist() == [(0x20 << 56), (255 << 56) | 2048, (255 << 56) | 4096]
    m0 = mh_oracle.Model.from_counts(np.ones(256, dtype=np.uint64), 0)
    (_, _, _, idx0), = recode_ref.recode([msg], m0, chunk=512)
    assert idx0.tolist() == [(0x20 << 56), (255 << 56) | 4096]                   # order 0: the entry still names the byte in front
