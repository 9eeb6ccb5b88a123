"""CPU-side checks of the digests of batches (include/mh.h, "DIGESTS OF BATCHES"): the symbols are declared, exported and
bound, the compute calls refuse bad arguments before a device is touched, the workspace sizes are plain arithmetic,
mh_crc32_combine against zlib.crc32, and the CLI's --crc argument rules."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_crc_batch_workspace", "mh_dev_crc_batch", "mh_dev_crc_each", "mh_dev_crc_batch_o2", "mh_crc_batch", "mh_crc_batch_o2",
               "mh_dev_crc_raw_batch_workspace", "mh_dev_crc_raw_batch", "mh_crc32_combine"]
CLI = os.path.join(ROOT, "bin", "markovhuffman")


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


def test_crc_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    section = header[header.index("DIGESTS OF BATCHES"):]
    assert header.index("ORDER 2 IN SEARCH AND RE-CODING") < header.index("DIGESTS OF BATCHES")
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name


def test_workspaces_are_plain_arithmetic_and_monotone(mhc):
    lib = mhc.lib()
    base = lib.mh_dev_crc_batch_workspace(0, 0, 0)
    assert base % 256 == 0 and 64 + 1280 <= base <= 64 + 1280 + 256
    last = 0
    for n in (0, 1, 2, 63, 64, 65, 1000, 65536, 1 << 24):
        s = lib.mh_dev_crc_batch_workspace(n, 1 << 28, 1024)
        assert s % 256 == 0 and base + 4 * n - 256 <= s <= base + 4 * n + 256, n        # the status block, the tables, 4 bytes per stream
        assert s >= last
        last = s
        for total, chunk in ((0, 0), (1 << 20, 256), (1 << 34, 8192), (1 << 20, 300)):   # nothing per chunk or per byte
            assert lib.mh_dev_crc_batch_workspace(n, total, chunk) == s
    # far below the buffer it replaces: 65 536 x 4 KiB decode into 256 MiB
    assert lib.mh_dev_crc_batch_workspace(65536, 65536 * 4096, 1024) < (256 << 20) // 900
    raw = lib.mh_dev_crc_raw_batch_workspace(0, 0)
    assert raw % 256 == 0 and 64 + 1280 <= raw <= 64 + 1280 + 256
    last = 0
    for n, total in ((0, 0), (1, 10), (1000, 10 ** 6), (65536, 1 << 28), (1 << 24, 1 << 36)):
        s = lib.mh_dev_crc_raw_batch_workspace(n, total)
        assert s % 256 == 0 and s >= last and s <= raw + 4 * n + 256
        last = s


NAMES = ["m", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total", "index", "chunk", "crc", "len", "status", "ws",
         "ws_bytes", "stream"]


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, model):
    lib = mhc.lib()
    ws = int(lib.mh_dev_crc_batch_workspace(2, 200, 256))
    wbuf = np.zeros(ws + 4096, dtype=np.uint8)
    w = (wbuf.ctypes.data + 255) & ~255                                    # 16-byte aligned host stand-ins
    ARG = mhc.MH_ERR_ARG
    ok = [model.handle, w, w, w, 2, 32, 0x20, w, 200, w, 256, w, w, w, w, ws, None]

    def call(fn=lib.mh_dev_crc_batch, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[NAMES.index(k)] = v
        return fn(*a)

    for fn in (lib.mh_dev_crc_batch, lib.mh_dev_crc_batch_o2):
        assert call(fn=fn, m=None) == ARG
    assert call(fn=lib.mh_dev_crc_batch_o2) == ARG                         # an order-1 model: refused by the order-2 call
    assert call(pay_off=None) == ARG
    assert call(payload=None) == ARG
    assert call(nbits=None) == ARG
    assert call(crc=None) == ARG
    assert call(payload=w + 4) == ARG                                      # unaligned payload
    assert call(ws=None) == ARG
    assert call(ws=w + 8) == ARG
    assert call(sym_off=None) == ARG                                       # an index needs sym_off
    for bad_chunk in (0, 100, 128, 16384):
        assert call(chunk=bad_chunk) == ARG
    assert call(ws_bytes=64) == mhc.MH_ERR_CAPACITY
    assert call(ws_bytes=ws - 1) == mhc.MH_ERR_CAPACITY
    each = lib.mh_dev_crc_each
    assert call(fn=each, m=None) == ARG                                    # no set
    assert call(fn=each, m=None, n=0) == ARG
    # the raw call: (data, in_off, n, total, crc, ws, ws_bytes, stream)
    rws = int(lib.mh_dev_crc_raw_batch_workspace(2, 100))
    raw = lib.mh_dev_crc_raw_batch
    assert raw(None, w, 2, 100, w, w, rws, None) == ARG
    assert raw(w, None, 2, 100, w, w, rws, None) == ARG
    assert raw(w, w, 2, 100, None, w, rws, None) == ARG
    assert raw(w, w, 2, 100, w, None, rws, None) == ARG
    assert raw(w, w, 2, 100, w, w + 8, rws, None) == ARG
    assert raw(w, w, 2, 100, w, w, rws - 1, None) == mhc.MH_ERR_CAPACITY
    if mhc.device_count() == 0:
        # valid arguments reach the device check: len and the statuses may be NULL, index-free needs no sym_off
        assert call() == mhc.MH_ERR_NO_DEVICE
        assert call(len=None, status=None) == mhc.MH_ERR_NO_DEVICE
        assert call(index=None, sym_off=None, chunk=0, sym_total=0) == mhc.MH_ERR_NO_DEVICE
        assert raw(w + 1, w, 2, 100, w, w, rws, None) == mhc.MH_ERR_NO_DEVICE     # d_data may start anywhere


def test_order2_model_is_refused_before_any_launch(mhc):
    lib = mhc.lib()
    counts = np.zeros(1 << 24, dtype=np.uint64)
    counts[(0x2020 << 8) | 65] = 3
    counts[(0x2041 << 8) | 66] = 2
    try:
        m2 = mhc.Model.from_counts(counts, 2)
    except mhc.MhError as e:                                               # an order-2 model cannot be built without a device:
        assert e.status == mhc.MH_ERR_NO_DEVICE and mhc.device_count() == 0   # tests/test_gpu_crc.py has the refusal on the card
        return
    w = np.zeros(8192, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    assert lib.mh_dev_crc_batch(m2.handle, p, p, p, 1, 16, 0x20, p, 100, p, 256, p, p, p, p, 1 << 15, None) == mhc.MH_ERR_ARG
    assert lib.mh_crc_batch(m2.handle, p, p, p, 1, 0x20, p, p, 256, p, p, p) == mhc.MH_ERR_ARG


def _host(mhc, model, fn=None, **kw):
    a = dict(m=model.handle if model is not None else None, payload=np.zeros(32, dtype=np.uint8), pay_off=np.array([0, 16, 32], dtype=np.uint64),
             nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20, sym_off=np.array([0, 100, 200], dtype=np.uint64),
             index=np.zeros(4, dtype=np.uint64), chunk=256, crc=np.zeros(2, dtype=np.uint32), len=np.zeros(2, dtype=np.uint64),
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return (fn or mhc.lib().mh_crc_batch)(*[p(a[k]) for k in ("m", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "crc",
                                                              "len", "status")])


def test_host_forms_refuse_bad_arguments_before_touching_a_device(mhc, model):
    ARG = mhc.MH_ERR_ARG
    assert _host(mhc, None) == ARG
    assert _host(mhc, None, fn=mhc.lib().mh_crc_batch_o2) == ARG
    assert _host(mhc, model, fn=mhc.lib().mh_crc_batch_o2) == ARG          # an order-1 model
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(crc=None), dict(sym_off=None)):
        assert _host(mhc, model, **kw) == ARG, kw
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host(mhc, model, chunk=bad_chunk) == ARG, bad_chunk
    assert _host(mhc, model, pay_off=np.array([1, 16, 32], dtype=np.uint64)) == ARG
    assert _host(mhc, model, pay_off=np.array([0, 16, 8], dtype=np.uint64)) == ARG
    assert _host(mhc, model, nbits=np.array([129, 128], dtype=np.uint64)) == ARG          # nbits past its bytes
    assert _host(mhc, model, sym_off=np.array([0, 100, 50], dtype=np.uint64)) == ARG
    if mhc.device_count() == 0:
        assert _host(mhc, model) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, len=None, status=None) == mhc.MH_ERR_NO_DEVICE
        assert _host(mhc, model, sym_off=None, index=None, chunk=0) == mhc.MH_ERR_NO_DEVICE
        with pytest.raises(mhc.MhError) as e:
            model.crc_batch(np.zeros(32, dtype=np.uint8), [0, 16, 32], [120, 128])
        assert e.value.status == mhc.MH_ERR_NO_DEVICE


# ---- mh_crc32_combine -------------------------------------------------------------------------------------------------------

def test_combine_equals_zlib_on_the_edge_lengths(mhc):
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    for la in (0, 1, 255, 256, 257):
        for lb in (0, 1, 255, 256, 257):
            b = rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
            assert mhc.crc32_combine(zlib.crc32(a[:la]), zlib.crc32(b), lb) == zlib.crc32(a[:la] + b), (la, lb)
    assert mhc.crc32_combine(0, 0, 0) == 0 and mhc.crc32_combine(0x12345678, 0, 0) == 0x12345678


def test_combine_equals_zlib_on_random_splits(mhc):
    rng = np.random.default_rng(12)
    data = rng.integers(0, 256, 100_000, dtype=np.uint8).tobytes()
    whole = zlib.crc32(data)
    for cut in [0, len(data)] + [int(x) for x in rng.integers(0, len(data) + 1, 60)]:
        assert mhc.crc32_combine(zlib.crc32(data[:cut]), zlib.crc32(data[cut:]), len(data) - cut) == whole, cut
    cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, 9))       # folded left to right over ten pieces
    acc, at = 0, 0
    for c in cuts + [len(data)]:
        acc = mhc.crc32_combine(acc, zlib.crc32(data[at:c]), c - at)
        at = c
    assert acc == whole


def test_combine_with_a_length_over_2_to_the_32(mhc):
    """B = 2^32 + 3 zero bytes, never allocated.  The expected value comes from the identity: over zero bytes the CRC register
    is a linear map, so crc(A || B) and crc(B) follow from the n-th power of the one-zero-byte matrix over GF(2), computed
    here by squaring with plain Python integers (no code shared with the library).  The matrix route is itself checked
    against zlib at a length zlib can go to."""
    n = (1 << 32) + 3
    a = b"digest"
    # independent route: the CRC register as a 32 x 32 matrix over GF(2) acting on one zero byte, raised to the n-th power by
    # squaring (plain Python integers, no code shared with the library)
    poly = 0xEDB88320

    def zero_byte(r):
        for _ in range(8):
            r = (r >> 1) ^ (poly if r & 1 else 0)
        return r

    def apply(mat, v):
        out, k = 0, 0
        while v:
            if v & 1:
                out ^= mat[k]
            v >>= 1
            k += 1
        return out

    mat = [zero_byte(1 << k) for k in range(32)]                           # column k: the image of bit k
    res = [1 << k for k in range(32)]
    e = n
    while e:
        if e & 1:
            res = [apply(mat, c) for c in res]
        mat = [apply(mat, c) for c in mat]
        e >>= 1
    # crc(A || 0^n) = M^n (crc(A) ^ ~0) ^ ~0 for zero bytes: the register runs on, the final XOR is taken off and put back
    want = apply(res, zlib.crc32(a) ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    crc_b = apply(res, 0xFFFFFFFF) ^ 0xFFFFFFFF                            # crc(0^n)
    assert mhc.crc32_combine(zlib.crc32(a), crc_b, n) == want
    # the same matrices agree with zlib where zlib can go: 2^20 + 3 zero bytes
    small = (1 << 20) + 3
    assert mhc.crc32_combine(zlib.crc32(a), zlib.crc32(bytes(small)), small) == zlib.crc32(a + bytes(small))
    # and three more bytes behind B, combined either way round
    three = zlib.crc32(bytes(3))
    assert mhc.crc32_combine(mhc.crc32_combine(zlib.crc32(a), crc_b, n), three, 3) == mhc.crc32_combine(zlib.crc32(a), mhc.crc32_combine(crc_b, three, 3), n + 3)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["no_x", "order2", "with_find", "with_range", "with_recode"])
def test_cli_crc_argument_errors(mhc, tmp_path, case):
    """Checked before anything is opened, so the named files need not exist."""
    cm, table, idx, out = (str(tmp_path / n) for n in ("in.cm", "table", "f.idx", "out"))
    base = [CLI, cm, "-o", out]
    args = {
        "no_x": base + ["-e", table, "--crc"],
        "order2": base + ["-x", "-e", table, "--order2", "--crc"],
        "with_find": base + ["-x", "-e", table, "--index", idx, "--crc", "--find", "abc"],
        "with_range": base + ["-x", "-e", table, "--index", idx, "--crc", "--range", "0:3"],
        "with_recode": base + ["-x", "-e", table, "--crc", "--recode", table],
    }[case]
    r = subprocess.run(args, capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    assert b"--crc" in r.stderr and b"Error" in r.stderr, r.stderr
    assert b"opening" not in r.stderr                                      # refused before any file is touched
    assert not os.path.exists(out)
