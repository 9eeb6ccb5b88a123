"""The tile decoder's piece pipeline (mh_tile.hip): a wave fetches its next piece's payload and the fine-index
words of the piece after that while the current piece's output drains.  What is new against test_gpu_tile.py is "a wave takes
a second, third, ... piece": on a 256-CU card no stream under 32 MiB gives a wave more than one.  So the cases here either are
large enough (the shipped library) or run the diagnostic library (libmhc_diag.so), whose MH_TILE_GRID=<g> caps the grid of the
tile kernels: with one or two workgroups a megabyte gives every wave many pieces.

Every case compares the decoded bytes with the input (the encoder's stream is pinned to the oracle elsewhere) and checks the
decoder's status word, mh_dev_decode_path and the guard bytes behind `decoded`."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from test_gpu_tile import Stream, o2_round_trip, text_like, zipf_bytes
import test_gpu_index_tiles as ixt
import test_gpu_stream as gst

pytestmark = pytest.mark.gpu

DEC_PATH_TILE = 1
GUARD = 4096
DIAG_CALLS = ("mh_dev_decode_fine", "mh_dev_decode_path", "mh_dev_status", "mh_dev_build_index_fine", "mh_dev_build_index",
              "mh_dev_index_path", "mh_dev_decode_stream_states", "mh_dev_decode_stream_emit")


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1
    return mod


class _Calls:
    """The product library's calls, those of DIAG_CALLS taken from the diagnostic library."""

    def __init__(self, base, diag):
        self._base, self._diag = base, diag

    def __getattr__(self, name):
        return getattr(self._diag if name in DIAG_CALLS else self._base, name)


class _Package:
    """The package as the helpers of the other tile tests take it, with lib() answering with _Calls."""

    def __init__(self, mod, calls):
        self._mod, self._calls = mod, calls

    def lib(self):
        return self._calls

    def __getattr__(self, name):
        return getattr(self._mod, name)


@pytest.fixture(scope="module")
def diag(mhc):
    """The package with the decode and index calls of libmhc_diag.so (the only library that reads MH_TILE_GRID)."""
    lib = mhc.lib()
    d = C.CDLL(os.path.join(os.path.dirname(mhc.LIB_PATH), "libmhc_diag.so"))
    for name in DIAG_CALLS:
        getattr(d, name).argtypes = getattr(lib, name).argtypes
        getattr(d, name).restype = getattr(lib, name).restype
    return _Package(mhc, _Calls(lib, d))


@pytest.fixture(autouse=True)
def tile_path_and_clean_switches():
    names = ("MH_DECODE_PATH", "MH_TILE_P", "MH_TILE_GRID")
    old = {k: os.environ.get(k) for k in names}
    os.environ["MH_DECODE_PATH"] = "tile"
    os.environ.pop("MH_TILE_P", None)
    os.environ.pop("MH_TILE_GRID", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@functools.lru_cache(maxsize=None)
def zipf_cached(n, seed, s=1.1):
    a = zipf_bytes(n, seed, s=s)
    a.setflags(write=False)
    return a


def decode(pkg, s, dn=False, stream=None, d_ws=None, d_out=None):
    """(status, path, redo count, decoded bytes) of mh_dev_decode_fine on Stream s; the guard bytes behind `decoded` are checked."""
    lib, n = pkg.lib(), s.n
    if d_out is None:
        d_out = pkg.DeviceBuffer(n + GUARD, init=np.full(n + GUARD, 0xAB, dtype=np.uint8))
    dws = int(lib.mh_dev_decode_workspace(s.nbits, n, s.chunk))
    if d_ws is None:
        d_ws = pkg.DeviceBuffer(dws)
    pkg._check(lib.mh_dev_decode_fine(s.model.handle, s.d_payload.ptr, 0 if dn else s.nbits, s.d_nbits.ptr if dn else None,
                                      d_out.ptr, n, s.d_index.ptr, s.chunk, s.d_fine.ptr, d_ws.ptr, dws, stream), "decode_fine")
    rc = lib.mh_dev_status(d_ws.ptr, stream)                   # (waits for the stream)
    path = lib.mh_dev_decode_path(d_ws.ptr, stream)
    redo = int(d_ws.download(np.uint32)[16])                    # the workspace's redo list: its count is the word at byte 64
    out = d_out.download()
    assert np.all(out[n:] == 0xAB), "wrote past the end of the output"
    return rc, path, redo, out[:n]


def check_round_trip(pkg, s, **kw):
    rc, path, redo, out = decode(pkg, s, **kw)
    assert (rc, path) == (0, DEC_PATH_TILE)
    assert np.array_equal(out, s.data)
    return redo


# ---- 1. the shipped library: workgroups take two or three blocks of sixteen pieces, the last block partial, the end ragged

def test_shipped_library_waves_take_several_pieces(mhc):
    import torch
    import bench
    n = (72 << 20) + 5 * 8192 + 77
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    data = bench.generate("zipf", n, 5, 0, dev).cpu().numpy()
    assert data.size == n
    check_round_trip(mhc, Stream(mhc, data, chunk=1024))


# ---- 2. the diagnostic library with one and three workgroups: eight or more pieces per wave, uneven block counts

@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("chunk", [256, 4096])
@pytest.mark.parametrize("tile_p", [5, 6, 7, 8])
@pytest.mark.parametrize("n", [8192 * 16 * 2, (1 << 20) + 77, 3 * (1 << 20) + 4099])
def test_capped_grid_round_trip(diag, n, tile_p, chunk, grid):
    os.environ["MH_TILE_P"] = str(tile_p)
    os.environ["MH_TILE_GRID"] = str(grid)
    s = Stream(diag, zipf_cached(n, n + tile_p), chunk=chunk)
    assert len(s.model.image(8)) == (256 << tile_p) * 2
    check_round_trip(diag, s)


# ---- 3. fewer than sixteen waves kept: the order tj += nw, and pieces larger than the prefetched part

@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("kind", ["non_stationary", "zipf095"])
def test_fewer_than_sixteen_waves_and_pieces_beyond_the_prefetch(diag, kind, grid):
    os.environ["MH_TILE_GRID"] = str(grid)
    n = 1 << 20
    if kind == "non_stationary":        # test_tile_decode_non_stationary_stream's: a third of the pieces takes 8 KiB and more
        data = np.concatenate([np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8), np.full(n, 7, dtype=np.uint8),
                               zipf_bytes(n + 5, 3)])
    else:                               # Zipf(0.95): ~6.45 bits per symbol, 6.6 KiB per piece of 8192 symbols
        data = zipf_cached(2 * n + 333, 41, s=0.95)
    s = Stream(diag, data)
    if kind == "zipf095":
        assert 6.2 * data.size < s.nbits < 6.7 * data.size
    check_round_trip(diag, s)


# ---- 4. skip paths in the middle of a wave's sequence

def test_an_oversized_piece_between_normal_ones_takes_the_redo_pass(diag):
    os.environ["MH_TILE_GRID"] = "1"
    data = zipf_cached(3 * (1 << 20) + 4099, 77).copy()
    data[21 * 8192:22 * 8192] = np.random.default_rng(6).integers(0, 256, 8192, dtype=np.uint8)   # piece 21: wave 5's second
    redo = check_round_trip(diag, Stream(diag, data))
    assert redo > 0


def test_long_codes_send_whole_pieces_to_the_redo_pass(diag):
    """test_tile_decode_long_codes_take_the_redo_pass's source: codes longer than the 5 + 8 bits the tables resolve."""
    os.environ["MH_TILE_GRID"] = "1"
    os.environ["MH_TILE_P"] = "5"
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, 1 << 20, dtype=np.uint8) & rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    s = Stream(diag, x)
    assert s.model.max_code_len > 13
    redo = check_round_trip(diag, s)
    assert redo > 0


# ---- 5. a damaged fine index in a wave's later piece and in the stream's last piece

def test_damaged_fine_index_in_later_pieces_is_reported(diag):
    """Every damaged position lies inside the allocated payload buffer: a wrong implementation shows as a wrong status."""
    os.environ["MH_TILE_GRID"] = "1"
    data = zipf_cached(2 << 20, 33)
    s = Stream(diag, data)
    fine = s.d_fine.download(np.uint32)
    per_piece, npieces = 2 * 64, data.size // 8192
    assert s.cap * 8 > s.nbits + 8192

    def with_pos(f, pos):
        return np.uint32((int(f) & 0xFF000000) | (pos & 0xFFFFFF))

    def pos_of(f):
        return int(f) & 0xFFFFFF

    later, last = 37 * per_piece, (npieces - 1) * per_piece        # piece 37: wave 5's third; the last piece: wave 15's last
    cases = []
    for first in (later, last):
        # an entry past nbits (wave 5's third piece / the stream's last piece)
        cases.append((first + 70, with_pos(fine[first + 70], s.nbits + 4096)))
        # the piece's first entry behind its neighbours: they then lie before the piece's start
        cases.append((first, with_pos(fine[first], pos_of(fine[first]) + 1000)))
        # two entries out of order, both inside the piece
        cases.append((first + 9, with_pos(fine[first + 9], pos_of(fine[first + 12]))))
    for where, value in cases:
        bad = fine.copy()
        bad[where] = value
        diag._check(s.lib.mh_dev_upload(s.d_fine.ptr, bad.ctypes.data, bad.nbytes), "upload")
        rc, path, _, _ = decode(diag, s)
        assert rc == diag.MH_ERR_CORRUPT and path == DEC_PATH_TILE, (where, rc, path)
    diag._check(s.lib.mh_dev_upload(s.d_fine.ptr, fine.ctypes.data, fine.nbytes), "upload")
    check_round_trip(diag, s)


# ---- 6. a pre-shifted shard in another start context, payload length read from the device word

@pytest.mark.parametrize("start_bit", [(1 << 40) + 5, (1 << 40) + (1 << 31) + 5, (1 << 32) - 1_000_003])
def test_pre_shifted_shard(diag, start_bit):
    """Bit positions beyond 2^32, with bit 31 of their low word set, and a stream that crosses a multiple of 2^32 (what a
    16 GiB stream has and no small one): the start bit's low three bits are not zero, the start context is not ' '."""
    os.environ["MH_TILE_GRID"] = "1"
    check_round_trip(diag, Stream(diag, zipf_cached((2 << 20) + 9, 9), start_bit=start_bit, prev0=0x41))


def test_payload_length_read_from_the_device_word(diag):
    os.environ["MH_TILE_GRID"] = "1"
    check_round_trip(diag, Stream(diag, zipf_cached((1 << 20) + 77, 10)), dn=True)


# ---- 7. the order-2 instantiation (extension: parity unpinned)

def test_order2_text_capped_grid_parity_unpinned(diag, oracle):
    os.environ["MH_TILE_GRID"] = "1"
    o2_round_trip(diag, oracle, text_like((3 << 20) + 1234, 11), chunk=1024, expect_tiles=True)


# ---- 8. a dirty, reused workspace and a non-default stream

def test_dirty_reused_workspace_on_a_non_default_stream(diag):
    import torch
    os.environ["MH_TILE_GRID"] = "1"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    assert sp.value, "a non-default stream has a handle"
    a, b = Stream(diag, zipf_cached((1 << 20) + 77, 10)), Stream(diag, zipf_cached(3 * (1 << 20) + 4099, 77))
    torch.cuda.synchronize()
    dws = int(diag.lib().mh_dev_decode_workspace(b.nbits, b.n, b.chunk))
    assert dws >= int(diag.lib().mh_dev_decode_workspace(a.nbits, a.n, a.chunk))
    d_ws = diag.DeviceBuffer(dws, init=np.full(dws, 0xA5, dtype=np.uint8))
    for s in (b, a, b):                                          # the same workspace, never cleared between the calls
        check_round_trip(diag, s, stream=sp, d_ws=d_ws)


# ---- 9. the index-free kernels under a capped grid: many tiles per wave

@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_index_free_kernels_capped_grid(diag, oracle, kind, grid):
    os.environ.pop("MH_DECODE_PATH", None)
    os.environ["MH_TILE_GRID"] = str(grid)
    n = 3 << 20
    data = zipf_cached(n, 19) if kind == "zipf" else ixt.text_like(n, 19)
    om = oracle.Model.from_data(data.tobytes(), 1)
    blob, nbits = om.compress(data.tobytes())
    m = diag.Model.from_table(om.table_bytes())
    lens = np.asarray(om.codes()[0]).astype(np.int64)
    assert nbits >= 1 << 20 and int(lens.max()) <= 15
    st1, path, ns, st2, out = gst.stream_decode(diag, m, blob[1:], nbits)
    assert (st1, path, ns, st2) == (0, gst.PATH_STATES, n, 0)
    assert np.array_equal(out[:n], data) and np.all(out[n:] == 0x5A)
    want_idx, want_fine = ixt.expected_entries(lens, data, 1024)
    st, ipath, ns, idx, fine = ixt.build(diag, m, blob[1:], nbits, 1024)
    assert (st, ipath, ns) == (0, ixt.IDX_TILES, n)
    assert np.array_equal(idx[:want_idx.size], want_idx) and np.array_equal(fine[:want_fine.size], want_fine)
