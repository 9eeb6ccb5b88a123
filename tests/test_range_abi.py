"""CPU-side checks of the byte-range calls (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM"): the symbols are
exported, the workspace is plain arithmetic, the host form refuses bad arguments before touching a device, and the CLI refuses
bad --range use before opening anything."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_decode_ranges_workspace", "mh_dev_decode_ranges", "mh_decode_ranges", "mh_last_range_upload_bytes"]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def test_range_symbols_are_declared_and_exported(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = ctypes.CDLL(mhc.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    assert "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM" in header
    assert "mh_dev_build_index_fine" in header[header.index("RANDOM ACCESS: BYTE RANGES"):]


def test_range_workspace_is_plain_arithmetic(mhc):
    lib = mhc.lib()
    sizes = [lib.mh_dev_decode_ranges_workspace(n) for n in (0, 1, 2, 1000, 65536, 1 << 20)]
    for n, s in zip((0, 1, 2, 1000, 65536, 1 << 20), sizes):
        assert s % 256 == 0 and s >= 64 + 8 * (n + 1)
        assert s <= 64 + 8 * (n + 1) + 8 * ((n + 1 + 1023) // 1024 + 1) + 256
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.mh_last_range_upload_bytes() == 0


PINNED_N = (0, 1, 2, 1000, 65536, 1 << 20)
PINNED_WORKSPACE = [256, 256, 256, 8192, 525056, 8397056]      # as returned before the kernel families were merged
PINNED_WORKSPACES = ["mh_dev_decode_ranges_workspace", "mh_dev_decode_ranges_o2_workspace", "mh_dev_decode_batch_ranges_workspace",
                     "mh_dev_decode_batch_o2_ranges_workspace"]


def test_workspace_sizes_are_pinned(mhc):
    """The four workspace functions of the random-access family, and that the order-0/1 device calls refuse a byte less on the
    host, before anything is launched (the calls here never get further: the pointers are host stand-ins).  An order-2 model
    and a model set need a device: tests/test_gpu_range_family.py holds the `_o2` calls and mh_dev_decode_each_ranges, which
    takes the batch function's size, to the same six values."""
    lib = mhc.lib()
    for name in PINNED_WORKSPACES:
        assert [getattr(lib, name)(n) for n in PINNED_N] == PINNED_WORKSPACE, name
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    for n, ws in zip(PINNED_N, PINNED_WORKSPACE):
        assert lib.mh_dev_decode_batch_ranges(m.handle, p, p, p, 1, 0x20, None, None, 0, p, n, p, p, 64, p, p, ws - 1, None) == mhc.MH_ERR_CAPACITY, n
        assert lib.mh_dev_decode_ranges(m.handle, p, 0, 64, 512, p, 256, 400, None, p, n, p, p, 16, p, p, ws - 1, None) == mhc.MH_ERR_CAPACITY, n


def _host_call(mhc, m, payload, nbits, index, chunk, n_symbols, ranges, out_cap=64):
    lib = mhc.lib()
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    off = np.zeros(rg.shape[0] + 1, dtype=np.uint64)
    st = np.zeros(max(rg.shape[0], 1), dtype=np.int32)
    return lib.mh_decode_ranges(m.handle if m is not None else None, payload, nbits, index, chunk, n_symbols,
                                rg.ctypes.data if rg.size else None, rg.shape[0], out.ctypes.data, out_cap, off.ctypes.data,
                                st.ctypes.data)


def test_host_form_refuses_bad_arguments_before_touching_a_device(mhc):
    m = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    pl = np.zeros(64, dtype=np.uint8)
    idx = np.zeros(4, dtype=np.uint64)
    p, i = pl.ctypes.data, idx.ctypes.data
    ok = dict(payload=p, nbits=512, index=i, chunk=256, n_symbols=400, ranges=[[0, 10]])
    args = lambda **kw: {**ok, **kw}
    assert _host_call(mhc, None, **ok) == mhc.MH_ERR_ARG                           # no model
    assert _host_call(mhc, m, **args(payload=None)) == mhc.MH_ERR_ARG
    assert _host_call(mhc, m, **args(index=None)) == mhc.MH_ERR_ARG
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert _host_call(mhc, m, **args(chunk=bad_chunk)) == mhc.MH_ERR_ARG
    assert _host_call(mhc, m, **args(n_symbols=513)) == mhc.MH_ERR_ARG             # n_symbols > nbits
    lib = mhc.lib()
    off = np.zeros(2, dtype=np.uint64)
    rg = np.array([0, 10], dtype=np.uint64)
    assert lib.mh_decode_ranges(m.handle, p, 512, i, 256, 400, None, 1, p, 64, off.ctypes.data, None) == mhc.MH_ERR_ARG   # no ranges
    assert lib.mh_decode_ranges(m.handle, p, 512, i, 256, 400, rg.ctypes.data, 1, p, 64, None, None) == mhc.MH_ERR_ARG     # no out_off
    assert lib.mh_decode_ranges(m.handle, p, 512, i, 256, 400, rg.ctypes.data, 1, None, 64, off.ctypes.data, None) == mhc.MH_ERR_ARG
    # the device form: null model / pointers and bad sizes before any launch
    ws = int(lib.mh_dev_decode_ranges_workspace(1))
    wbuf = np.zeros(ws + 256, dtype=np.uint8)
    w = (wbuf.ctypes.data + 255) & ~255
    assert lib.mh_dev_decode_ranges(None, p, 0, 64, 512, i, 256, 400, None, rg.ctypes.data, 1, w, i, 16, w, w, ws, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_decode_ranges(m.handle, p, 0, 64, 512, i, 300, 400, None, rg.ctypes.data, 1, w, i, 16, w, w, ws, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_decode_ranges(m.handle, p, 0, 64, 512, i, 256, 600, None, rg.ctypes.data, 1, w, i, 16, w, w, ws, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_decode_ranges(m.handle, p, 60, 8, 512, i, 256, 400, None, rg.ctypes.data, 1, w, i, 16, w, w, ws, None) == mhc.MH_ERR_ARG   # window past the payload
    assert lib.mh_dev_decode_ranges(m.handle, p, 0, 64, 512, i, 256, 400, None, None, 1, w, i, 16, w, w, ws, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_decode_ranges(m.handle, p, 0, 64, 512, i, 256, 400, None, rg.ctypes.data, 1, w, i, 16, w, w, 64, None) == mhc.MH_ERR_CAPACITY


def test_host_form_without_a_gpu_reports_no_device(mhc):
    if mhc.device_count() > 0:
        pytest.skip("a GPU is present")
    for order in (0, 1):
        m = mhc.Model.from_counts(np.ones(65536 if order else 256, dtype=np.uint64), order)
        pl = np.zeros(64, dtype=np.uint8)
        idx = np.zeros(2, dtype=np.uint64)
        assert _host_call(mhc, m, pl.ctypes.data, 512, idx.ctypes.data, 256, 400, [[0, 10], [5, 5]]) == mhc.MH_ERR_NO_DEVICE
        with pytest.raises(mhc.MhError) as e:
            m.decode_ranges(pl.tobytes(), 512, idx, 256, 400, [(0, 10)])
        assert e.value.status == mhc.MH_ERR_NO_DEVICE


def _cli():
    binp = os.path.join(ROOT, "bin", "markovhuffman")
    if not os.path.exists(binp):
        entry.build()
    return binp


@pytest.mark.parametrize("case", ["no_x", "no_index", "malformed", "no_colon", "reversed", "negative", "order2"])
def test_cli_rejects_bad_range_use_before_touching_a_device(tmp_path, case):
    src = tmp_path / "in.cm"
    src.write_bytes(b"\x30hello")
    table = tmp_path / "t.e"
    table.write_bytes(b"\x80")
    out = tmp_path / "out"
    idx = str(tmp_path / "i")
    base = [_cli(), str(src), "-o", str(out)]
    argv = {
        "no_x": base + ["--index", idx, "--range", "0:3"],
        "no_index": base + ["-x", "-e", str(table), "--range", "0:3"],
        "malformed": base + ["-x", "-e", str(table), "--index", idx, "--range", "1:2x"],
        "no_colon": base + ["-x", "-e", str(table), "--index", idx, "--range", "12"],
        "reversed": base + ["-x", "-e", str(table), "--index", idx, "--range", "9:3"],
        "negative": base + ["-x", "-e", str(table), "--index", idx, "--range", "-1:3"],
        "order2": base + ["-x", "-e", str(table), "--index", idx, "--order2", "--range", "0:3"],
    }[case]
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1, (case, r.stderr)
    assert b"--range" in r.stderr, (case, r.stderr)
    assert not out.exists(), case
    assert b"no usable HIP device" not in r.stderr, case


def test_cli_help_lists_range_and_keeps_its_first_line():
    r = subprocess.run([_cli()], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1
    lines = r.stderr.decode().splitlines()
    assert lines[0] == "markov-huffman <input> [-o output] [options]"
    assert sum("--range" in l for l in lines) == 1
