"""The verdict matrix on damaged streams: every decoder's status, symbol count and bytes on a damaged input equal the contract
of include/mh.h as tests/damage.py computes it from the CPU oracle alone (src/coding.cpp:158, `assert(bi == length)`, made a
status).  Damages (each named in the case): D1 cuts at the end, D2 extensions with zeros and with ones, D3 cuts at and around
352-bit segment, tile, 512-bit batch segment and chunk-entry boundaries, D4 single-bit flips, D5 a null table entry, D6 another
source's table; bits after nbits set to ones must not change a verdict.  The path or variant each decoder took is asserted
from its diagnostics, so the matrix proves its coverage.  No case accepts more than one verdict."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
from damage import MH_OK, MH_ERR_CORRUPT

pytestmark = pytest.mark.gpu

PATH_STATES, IDX_SEGMENTS, IDX_TILES = 6, 1, 5
DEC_TILE, DEC_CHUNK = 1, 2
VARIANTS = {0: "LDS_WIDE", 3: "LDS_TWO_LEVEL_P8", 8: "L2_DIRECT_H8"}
GUARD = 4096


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1
    mod.lib().mh_dev_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    return mod


def zipf_bytes(n, seed, s=1.1, k=256):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, k + 1) ** s
    return rng.choice(k, size=n, p=w / w.sum()).astype(np.uint8)


def text_like(n, seed):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9)).astype(np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 300))] + (b". " if rng.random() < 0.1 else b" ")
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


class Source:
    """A stream of the oracle (= the reference's file) with its model, code positions, index and damages."""

    def __init__(self, mhc, oracle, data, counts=None, order=1, chunk=1024, seed=0, per_kind=2, kmax=10):
        self.data = np.asarray(data, dtype=np.uint8)
        self.order, self.chunk = order, chunk
        self.prev0 = 0x2020 if order == 2 else 0x20
        self.om = oracle.Model.from_counts(counts, order) if counts is not None else oracle.Model.from_data(self.data.tobytes(), order)
        blob, self.nbits = self.om.compress(self.data.tobytes())
        self.payload = blob[1:]
        self.m = mhc.Model.from_table(self.om.table_bytes())
        lens = np.asarray(self.om.codes_o2()[0] if order == 2 else self.om.codes()[0])
        self.bounds = damage.boundaries(lens, self.data, order, self.prev0)
        self.code_len = damage.code_lengths(lens, self.data, order, self.prev0)
        assert int(self.bounds[-1]) == self.nbits
        self.index, self.fine = damage.expected_entries(lens, self.data, chunk, self.prev0, order)
        offs = (self.index & np.uint64((1 << (48 if order == 2 else 56)) - 1)).astype(np.int64)
        self.cases = damage.all_damages(self.payload, self.nbits, self.bounds, self.code_len, offs, seed=seed, per_kind=per_kind,
                                        kmax=kmax)
        self._free, self._idx = {}, {}

    def free(self, name, pl, nb):
        if name not in self._free:
            self._free[name] = damage.verdict_free(self.om, pl, nb, self.prev0)
        return self._free[name]

    def indexed(self, name, pl, nb):
        if name not in self._idx:
            self._idx[name] = damage.verdict_indexed(self.om, pl, nb, self.index, self.chunk, self.data.size, self.order)
        return self._idx[name]


def padded(pl):
    a = np.frombuffer(pl, dtype=np.uint8)
    return np.concatenate([a, np.zeros(64, dtype=np.uint8)])


def expect(got, want, what):
    """got / want: (status, bytes or None); on OK the bytes must match."""
    assert got[0] == want[0], "%s: status %d, contract %d" % (what, got[0], want[0])
    if want[0] == MH_OK:
        assert len(got[1]) == len(want[1]), "%s: %d symbols, contract %d" % (what, len(got[1]), len(want[1]))
        assert got[1] == want[1], "%s: bytes differ" % what


# ---- single-stream decoders ----------------------------------------------------------------------------------------------
def stream_decode(mhc, m, payload, nbits, prev0=0x20):
    """mh_dev_decode_stream_states + _emit: (path, (status, bytes)); guard bytes behind the output checked."""
    lib = mhc.lib()
    d_pl = mhc.DeviceBuffer(len(payload) + 64, init=padded(payload))
    d_ns = mhc.DeviceBuffer(8)
    iws = int(lib.mh_dev_build_index_workspace(nbits))
    d_iws = mhc.DeviceBuffer(iws)
    assert lib.mh_dev_decode_stream_states(m.handle, d_pl.ptr, nbits, prev0, d_ns.ptr, d_iws.ptr, iws, None) == 0
    st1, path = lib.mh_dev_status(d_iws.ptr, None), lib.mh_dev_index_path(d_iws.ptr, None)
    ns = int(d_ns.download(np.uint64)[0])
    if st1 != 0 or path != PATH_STATES:
        return path, (st1, None)
    d_out = mhc.DeviceBuffer(ns + GUARD, init=np.full(ns + GUARD, 0x5A, dtype=np.uint8))
    assert lib.mh_dev_decode_stream_emit(m.handle, d_pl.ptr, nbits, prev0, d_out.ptr, ns, d_iws.ptr, iws, None) == 0
    st2 = lib.mh_dev_status(d_iws.ptr, None)
    out = d_out.download()
    assert np.all(out[ns:] == 0x5A), "wrote at or beyond out_cap"
    return path, (st2, out[:ns].tobytes() if st2 == 0 else None)


def host_decode(mhc, m, payload, nbits, index=None, chunk=0, n=0):
    """mh_decode (the host form): (status, bytes)."""
    try:
        return MH_OK, m.decode(payload, nbits, index=index, chunk_symbols=chunk, n_symbols=n)
    except mhc.MhError as e:
        return e.status, None


def build_index(mhc, m, payload, nbits, chunk, prev0=0x20):
    """mh_dev_build_index_fine: (path, status, n_symbols, index, fine)."""
    lib = mhc.lib()
    d_pl = mhc.DeviceBuffer(len(payload) + 64, init=padded(payload))
    icap, fcap = nbits // chunk + 2, nbits // 64 + 2
    d_idx, d_fine, d_ns = mhc.DeviceBuffer(icap * 8), mhc.DeviceBuffer(fcap * 4), mhc.DeviceBuffer(8)
    iws = int(lib.mh_dev_build_index_workspace(nbits))
    d_iws = mhc.DeviceBuffer(iws)
    assert lib.mh_dev_build_index_fine(m.handle, d_pl.ptr, nbits, prev0, d_idx.ptr, icap, chunk, d_fine.ptr, fcap, d_ns.ptr, d_iws.ptr,
                                       iws, None) == 0
    return (lib.mh_dev_index_path(d_iws.ptr, None), lib.mh_dev_status(d_iws.ptr, None), int(d_ns.download(np.uint64)[0]),
            d_idx.download(np.uint64), d_fine.download(np.uint32))


def chunk_decode(mhc, src, payload, nbits, fine=False):
    """mh_dev_decode (or mh_dev_decode_fine with the stream's fine index): (path, variant, (status, bytes)); guard checked."""
    lib = mhc.lib()
    n = src.data.size
    d_pl = mhc.DeviceBuffer(len(payload) + 64, init=padded(payload))
    d_idx = mhc.DeviceBuffer(src.index.size * 8, init=np.ascontiguousarray(src.index, dtype=np.uint64))
    d_out = mhc.DeviceBuffer(n + GUARD, init=np.full(n + GUARD, 0x5A, dtype=np.uint8))
    wsb = int(lib.mh_dev_decode_workspace(nbits, n, src.chunk))
    d_ws = mhc.DeviceBuffer(wsb)
    if fine:
        d_fine = mhc.DeviceBuffer(src.fine.size * 4, init=src.fine)
        rc = lib.mh_dev_decode_fine(src.m.handle, d_pl.ptr, nbits, None, d_out.ptr, n, d_idx.ptr, src.chunk, d_fine.ptr, d_ws.ptr, wsb, None)
    else:
        rc = lib.mh_dev_decode(src.m.handle, d_pl.ptr, nbits, d_out.ptr, n, d_idx.ptr, src.chunk, d_ws.ptr, wsb, None)
    assert rc == 0
    st = lib.mh_dev_status(d_ws.ptr, None)
    out = d_out.download()
    assert np.all(out[n:] == 0x5A), "wrote at or beyond out_cap"
    return lib.mh_dev_decode_path(d_ws.ptr, None), lib.mh_dev_decode_variant(d_ws.ptr, None), (st, out[:n].tobytes() if st == 0 else None)


# ---- sources ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zipf_src(mhc, oracle):
    """Zipf bytes: over a megabit, codes of at most 15 bits (tiles, two-pass path)."""
    return Source(mhc, oracle, zipf_bytes(400_000, 9), seed=1, per_kind=1, kmax=8)


@pytest.fixture(scope="module")
def long_src(mhc, oracle):
    """The chunk decoder's REDO_LDS recipe (Fibonacci weights: codes of up to 25 bits, some planted), ending in a planted
    code longer than 15 bits: the stream's last 352-bit segment goes to the walk of the two-pass path."""
    from test_gpu_decode_variants import recipe
    counts, data = recipe("REDO_LDS")
    data = data.copy()
    lens = np.asarray(oracle.Model.from_counts(counts.reshape(-1) + oracle.histogram_o1(data.tobytes()).astype(np.uint64), 1).codes()[0])
    p, sym = divmod(int(np.argmax(lens)), 256)
    data[-2:] = (p, sym)                                # the longest code of the model ends the stream
    counts = counts.reshape(-1) + oracle.histogram_o1(data.tobytes()).astype(np.uint64)
    s = Source(mhc, oracle, data, counts=counts, chunk=256, seed=2)
    assert int(s.code_len[-1]) > 15
    return s


def advice_cases(src):
    """The stream cut inside its final (long) code, every bit of it, and at its start."""
    last = int(src.code_len[-1])
    return [("long-%d" % k, damage.cut(src.payload, src.nbits, src.nbits - k), src.nbits - k) for k in range(1, last + 1)]


def test_the_two_pass_path_on_a_final_code_longer_than_the_tile_tables(mhc, long_src):
    """The stream ends in a code of more than 15 bits; nbits cut anywhere inside it must be MH_ERR_CORRUPT from the two-pass path
    (path 6, the last segment walked) and from mh_decode without an index; cut before it, the prefix."""
    s = long_src
    for name, pl, nb in advice_cases(s) + [("valid", s.payload, s.nbits)]:
        want = s.free(name, pl, nb)
        path, got = stream_decode(mhc, s.m, pl, nb)
        assert path == PATH_STATES, (name, path)
        expect(got, want, "states/emit " + name)
        expect(host_decode(mhc, s.m, pl, nb), want, "mh_decode " + name)


@pytest.mark.parametrize("which", ["zipf", "long"])
def test_two_pass_path_and_host_form(mhc, zipf_src, long_src, which):
    """D1-D4 and garbage after nbits through mh_dev_decode_stream_states / _emit (path 6) and mh_decode without an index."""
    s = zipf_src if which == "zipf" else long_src
    for name, pl, nb in s.cases:
        want = s.free(name, pl, nb)
        path, got = stream_decode(mhc, s.m, pl, nb)
        if nb < 1 << 20:                                   # under a megabit: not this path's business
            assert path == 0, (name, path)
            expect(host_decode(mhc, s.m, pl, nb), want, "mh_decode " + name)
            continue
        assert path == PATH_STATES, (name, path)
        expect(got, want, "states/emit " + name)
        expect(stream_decode(mhc, s.m, damage.garbage_after(pl, nb, 1), nb)[1], want, "states/emit ones after " + name)
        expect(host_decode(mhc, s.m, pl, nb), want, "mh_decode " + name)


@pytest.mark.parametrize("switch,path", [(None, IDX_TILES), ("MH_INDEX_NO_TILES", IDX_SEGMENTS)])
def test_index_builder(mhc, zipf_src, monkeypatch, switch, path):
    """mh_dev_build_index_fine on D1-D4: status, symbol count and entries equal the contract; and mh_decode through the index
    builder (MH_DECODE_NO_STREAM) gives the same verdict."""
    s = zipf_src
    monkeypatch.setenv("MH_DECODE_NO_STREAM", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    lens = np.asarray(s.om.codes()[0])
    for name, pl, nb in s.cases:
        want = s.free(name, pl, nb)
        p, st, ns, idx, fine = build_index(mhc, s.m, pl, nb, s.chunk)
        assert p == (path if nb >= 1 << 20 else IDX_SEGMENTS), (name, p)
        assert st == want[0], "build_index %s: status %d, contract %d" % (name, st, want[0])
        if st == MH_OK:
            d = np.frombuffer(want[1], dtype=np.uint8)
            wi, wf = damage.expected_entries(lens, d, s.chunk)
            assert ns == d.size, name
            assert np.array_equal(idx[:wi.size], wi) and np.array_equal(fine[:wf.size], wf), name
        expect(host_decode(mhc, s.m, pl, nb), want, "mh_decode via the index builder " + name)
        assert st != MH_OK or mhc.lib().mh_last_index_path() == p


@pytest.mark.parametrize("kind,path", [("period3", 2), ("runs", 3)])
def test_index_builder_fallback_paths(mhc, oracle, monkeypatch, kind, path):
    """Streams whose segments never re-synchronise (test_gpu_scale.py's sources): "ABCABC..." (one code length: per-group
    context maps, path 2) and runs 0...01...1... (mixed lengths: per-group state maps, path 3).  D1-D4 through
    mh_dev_build_index_fine and mh_decode; the path is asserted wherever the stream keeps (about) its length."""
    n = 2 << 20
    if kind == "period3":
        data = np.tile(np.frombuffer(b"ABC", dtype=np.uint8), n // 3 + 1)[:n]
    else:
        data = (np.arange(n, dtype=np.int64) // 4096 % 256).astype(np.uint8)
    s = Source(mhc, oracle, data, seed=3, per_kind=1, kmax=6)
    monkeypatch.setenv("MH_DECODE_NO_STREAM", "1")
    seen = 0
    for name, pl, nb in s.cases + [("valid", s.payload, s.nbits)]:
        want = s.free(name, pl, nb)
        p, st, ns, _, _ = build_index(mhc, s.m, pl, nb, s.chunk)
        if abs(nb - s.nbits) <= 64:
            assert p == path, (name, p)
            seen += 1
        assert st == want[0], "build_index %s (path %d): status %d, contract %d" % (name, p, st, want[0])
        if st == MH_OK:
            assert ns == len(want[1]), name
        expect(host_decode(mhc, s.m, pl, nb), want, "mh_decode via the index builder " + name)
    assert seen > 10


@pytest.mark.parametrize("kind,variant", [("LDS_WIDE", "LDS_WIDE"), ("REDO_LDS", "LDS_TWO_LEVEL_P8"), ("REDO_L2_DIRECT", "L2_DIRECT_H8")])
def test_chunk_decoder_with_the_encoder_s_index(mhc, oracle, kind, variant):
    """mh_dev_decode with the encoder's index on D1-D4 of the variant recipes (the REDO ones send chunks with long codes to
    the redo pass); the host form mh_decode with the index gives the same verdict."""
    from test_gpu_decode_variants import recipe
    counts, data = recipe(kind)
    if kind == "LDS_WIDE":
        data = data[:(1 << 20) + 4321]
    counts = counts.reshape(-1) + oracle.histogram_o1(data.tobytes()).astype(np.uint64)
    s = Source(mhc, oracle, data, counts=counts, chunk=256, seed=4, per_kind=1, kmax=6)
    for name, pl, nb in s.cases + [("valid", s.payload, s.nbits)]:
        want = s.indexed(name, pl, nb)
        path, var, got = chunk_decode(mhc, s, pl, nb)
        assert path == DEC_CHUNK, (name, path)
        if abs(nb - s.nbits) <= 64:                        # (the launcher picks by the stream's length as well)
            assert VARIANTS.get(var) == variant, (name, var)
        expect(got, want, "chunk decoder %s %s" % (kind, name))
        expect(host_decode(mhc, s.m, pl, nb, s.index, s.chunk, s.data.size), want, "mh_decode indexed " + name)


def test_tile_decoder(mhc, zipf_src, monkeypatch):
    """mh_dev_decode_fine with the stream's fine index, the tile decoder forced (MH_DECODE_PATH=tile)."""
    s = zipf_src
    monkeypatch.setenv("MH_DECODE_PATH", "tile")
    for name, pl, nb in s.cases:
        want = s.indexed(name, pl, nb)
        path, _, got = chunk_decode(mhc, s, pl, nb, fine=True)
        assert path == DEC_TILE, (name, path)
        expect(got, want, "tile decoder " + name)


def test_byte_ranges(mhc, zipf_src):
    """mh_decode_ranges: a range fails iff a chunk it reads fails."""
    s = zipf_src
    n, c = s.data.size, s.chunk
    ranges = [(0, 100), (c - 10, c + 10), (n // 2, n // 2 + 3 * c), (n - 5, n), (n - c - 1, n - 1), (n - 1, n), (7, 7)]
    for name, pl, nb in s.cases:
        if nb < n:                                         # fewer bits than symbols: refused before any decode
            with pytest.raises(mhc.MhError) as e:
                s.m.decode_ranges(pl, nb, s.index, c, n, ranges)
            assert e.value.status == mhc.MH_ERR_ARG, name
            continue
        res, status = s.m.decode_ranges(pl, nb, s.index, c, n, ranges)
        for (b, e), got, st in zip(ranges, res, status):
            want = damage.verdict_range(s.om, pl, nb, s.index, c, n, b, e)
            expect((int(st), got), want, "range [%d, %d) %s" % (b, e, name))
    assert any(nb >= n and nb < (int(s.index[-1]) & ((1 << 56) - 1)) for _, _, nb in s.cases)   # entries past a cut nbits


def test_order2_single_stream(mhc, oracle):
    """An order-2 stream through mh_decode, index-free (the index builder) and with the encoder's index."""
    s = Source(mhc, oracle, text_like(300_000, 7), order=2, chunk=1024, seed=5, per_kind=1, kmax=6)
    assert host_decode(mhc, s.m, s.payload, s.nbits) == (MH_OK, s.data.tobytes())
    assert mhc.lib().mh_last_index_path() == IDX_SEGMENTS          # order 2: no two-pass path, the segment iteration
    for name, pl, nb in s.cases:
        expect(host_decode(mhc, s.m, pl, nb), s.free(name, pl, nb), "order 2 index-free " + name)
        expect(host_decode(mhc, s.m, pl, nb, s.index, s.chunk, s.data.size), s.indexed(name, pl, nb), "order 2 indexed " + name)


def test_null_entry_and_another_source_s_table(mhc, oracle):
    """D5: byte 1 only ends the training data, so context 1 has no table; bits after it meet the null entry.  D6: a stream
    decoded under another source's table (where that decode happens to end exactly at nbits, the contract says OK)."""
    data = np.concatenate([zipf_bytes(600_000, 21, k=200) + 2, [1]]).astype(np.uint8)
    om = oracle.Model.from_data(data.tobytes(), 1)
    m = mhc.Model.from_table(om.table_bytes())
    for extra in (8, 12, 40):
        for fill in (0, 1):
            name, pl, nb = damage.d5_null_entry(om, data, 1, extra, fill)
            want = damage.verdict_free(om, pl, nb)
            assert want[0] == MH_ERR_CORRUPT
            expect(host_decode(mhc, m, pl, nb), want, "mh_decode " + name)
    z = zipf_bytes(300_000, 22)
    oz = oracle.Model.from_data(z.tobytes(), 1)
    blob, nbits = oz.compress(z.tobytes())
    for other in (oracle.Model.from_data(text_like(400_000, 4).tobytes(), 1), oracle.Model.from_data(b"\x00", 1), om):
        want = damage.verdict_free(other, blob[1:], nbits)
        expect(host_decode(mhc, mhc.Model.from_table(other.table_bytes()), blob[1:], nbits), want, "D6 another table")


# ---- batches ------------------------------------------------------------------------------------------------------------
class Batch:
    """Five streams of one source (order 1 or 2) with the encoder's index slices; stream `at` is replaced by a damage."""

    def __init__(self, mhc, oracle, order=1, chunk=256):
        self.mhc, self.order, self.chunk = mhc, order, chunk
        self.prev0 = 0x2020 if order == 2 else 0x20
        msgs = [text_like(k, 40 + k) if order == 2 else zipf_bytes(k, 40 + k) for k in (30_000, 5_000, 60_000, 700, 45_000)]
        self.msgs = [m.tobytes() for m in msgs]
        hist = oracle.histogram_o2 if order == 2 else (lambda d: oracle.histogram_o1(d))
        counts = sum(hist(m).astype(np.uint64) for m in self.msgs)    # every message counted from the start context
        self.om = oracle.Model.from_counts(counts, order)
        self.m = mhc.Model.from_table(self.om.table_bytes())
        lens = np.asarray(self.om.codes_o2()[0] if order == 2 else self.om.codes()[0])
        self.streams = []
        for msg in msgs:
            blob, nb = self.om.compress(msg.tobytes())
            idx, _ = damage.expected_entries(lens, msg, chunk, self.prev0, order)
            b = damage.boundaries(lens, msg, order, self.prev0)
            cl = damage.code_lengths(lens, msg, order, self.prev0)
            assert damage.verdict_free(self.om, blob[1:], nb, self.prev0) == (MH_OK, msg.tobytes())   # every pair has a code
            self.streams.append((blob[1:], nb, idx, b, cl))

    def cases(self, i, seed, per_kind=1, kmax=6):
        pl, nb, idx, b, cl = self.streams[i]
        offs = (idx & np.uint64((1 << (48 if self.order == 2 else 56)) - 1)).astype(np.int64)
        return damage.all_damages(pl, nb, b, cl, offs, seed=seed, per_kind=per_kind, kmax=kmax)

    def pack(self, at, pl, nb):
        """(payload, pay_off, nbits, sym_off, index) with stream `at` replaced."""
        pls = [s[0] for s in self.streams]
        nbs = [s[1] for s in self.streams]
        pls[at], nbs[at] = pl, nb
        payload, pay_off = self.mhc.batch_offsets(pls)
        sym_off = np.zeros(len(self.msgs) + 1, dtype=np.uint64)
        sym_off[1:] = np.cumsum([len(m) for m in self.msgs])
        l = self.mhc.lib()
        index = np.zeros(max(l.mh_batch_index_capacity(int(sym_off[-1]), len(self.msgs), self.chunk), 1), dtype=np.uint64)
        for i, s in enumerate(self.streams):
            base = l.mh_batch_index_base(int(sym_off[i]), i, self.chunk)
            index[base:base + s[2].size] = s[2]
        return payload, pay_off, np.array(nbs, dtype=np.uint64), sym_off, index

    def verdicts(self, at, pl, nb, indexed):
        want = [(MH_OK, m) for m in self.msgs]
        if indexed:
            want[at] = damage.verdict_indexed(self.om, pl, nb, self.streams[at][2], self.chunk, len(self.msgs[at]), self.order)
        else:
            want[at] = damage.verdict_free(self.om, pl, nb, self.prev0)
        return want

    def each_case(self, seed, edge_cases=None):
        """(position, name, payload, nbits): the damaged stream first, in the middle and last in turn.  edge_cases: only that
        many damages, spread evenly over the kinds, where the damaged stream is the first or the last."""
        for j, at in enumerate((0, 2, 4)):
            cases = self.cases(at, seed + j)
            if edge_cases is not None and at != 2:
                cases = cases[::max(1, len(cases) // edge_cases)][:edge_cases]
            for name, pl, nb in cases:
                yield at, "stream %d %s" % (at, name), pl, nb


def expect_batch(out, so, st, want, what, fail_len=None):
    """Per-stream status; OK streams byte-exact at sym_off; a failed stream's sym_off length fail_len when given."""
    for i, (ws, wb) in enumerate(want):
        assert int(st[i]) == ws, "%s: stream %d status %d, contract %d" % (what, i, int(st[i]), ws)
        got_len = int(so[i + 1]) - int(so[i])
        if ws == MH_OK:
            assert got_len == len(wb), "%s: stream %d has %d symbols, contract %d" % (what, i, got_len, len(wb))
            assert out[int(so[i]):int(so[i + 1])] == wb, "%s: stream %d bytes differ" % (what, i)
        elif fail_len is not None:
            assert got_len == fail_len, "%s: failed stream %d has %d symbols" % (what, i, got_len)


@pytest.fixture(scope="module")
def batch1(mhc, oracle):
    return Batch(mhc, oracle, 1)


@pytest.fixture(scope="module")
def batch2(mhc, oracle):
    return Batch(mhc, oracle, 2, chunk=1024)


@pytest.mark.parametrize("indexed", [False, True])
def test_decode_batch(mhc, batch1, indexed):
    bt = batch1
    for at, name, pl, nb in bt.each_case(10):
        payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
        want = bt.verdicts(at, pl, nb, indexed)
        kw = dict(sym_off=sym_off, index=index, chunk_symbols=bt.chunk) if indexed else {}
        out, so, st = bt.m.decode_batch(payload, pay_off, nbits, check=False, **kw)
        expect_batch(out, so, st, want, "decode_batch %s" % name)
        if indexed:
            assert np.array_equal(so, sym_off)


@pytest.mark.parametrize("indexed", [False, True])
def test_decode_batch_o2(mhc, batch2, indexed):
    bt = batch2
    for at, name, pl, nb in bt.each_case(20):
        payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
        want = bt.verdicts(at, pl, nb, indexed)
        kw = dict(sym_off=sym_off, index=index, chunk_symbols=bt.chunk) if indexed else {}
        out, so, st = bt.m.decode_batch_o2(payload, pay_off, nbits, check=False, **kw)
        expect_batch(out, so, st, want, "decode_batch_o2 %s" % name)
        if indexed:
            assert np.array_equal(so, sym_off)


@pytest.mark.parametrize("kind", ["shared", "set", "shared2"])
def test_device_batch_decode_leaves_the_guard_bytes(mhc, batch1, batch2, kind):
    """The device decode call of every model kind (one kernel family: mh_dev_decode_batch under the shared order-0/1 model,
    mh_dev_decode_each under a set that gives every stream that model, mh_dev_decode_batch_o2 under the shared order-2 model),
    index-free and indexed, into a buffer of exactly the valid streams' size plus 0x5A guard bytes: per-stream status as the
    contract says, nothing written at or beyond out_cap.  The shared order-0/1 model takes every damage first, in the middle
    and last; the two kinds whose tables lie in L2 (a lane walks 60 000 symbols in tens of milliseconds there) every damage in
    the middle, where the damaged stream has good neighbours on both sides, and four damages spread over the kinds as the
    first and as the last stream, the i == 0 and i == n - 1 edges of the kernels."""
    bt = batch2 if kind == "shared2" else batch1
    l = mhc.lib()
    if kind == "set":
        models = mhc.ModelSet.from_tables([bt.om.table_bytes()] * len(bt.msgs))
        call, handle, ws_of = l.mh_dev_decode_each, models.handle, l.mh_dev_decode_each_workspace
    elif kind == "shared2":
        call, handle, ws_of = l.mh_dev_decode_batch_o2, bt.m.handle, l.mh_dev_decode_batch_o2_workspace
    else:
        call, handle, ws_of = l.mh_dev_decode_batch, bt.m.handle, l.mh_dev_decode_batch_workspace
    for at, name, pl, nb in bt.each_case(70, None if kind == "shared" else 4):
        payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
        for indexed in (False, True):
            want = bt.verdicts(at, pl, nb, indexed)
            # indexed: the encode's sizes; index-free: a failed stream decodes to 0 symbols, so exactly the good streams' bytes
            cap = int(sym_off[-1]) if indexed else int(sum(len(w[1]) for w in want if w[0] == MH_OK))
            d_pl = mhc.DeviceBuffer(payload.size + 64, init=np.concatenate([payload, np.zeros(64, dtype=np.uint8)]))
            d_po, d_nb = mhc.DeviceBuffer(pay_off.nbytes, init=pay_off), mhc.DeviceBuffer(nbits.nbytes, init=nbits)
            so = sym_off.copy() if indexed else np.zeros_like(sym_off)
            d_so = mhc.DeviceBuffer(so.nbytes, init=so)
            d_idx = mhc.DeviceBuffer(index.nbytes, init=index) if indexed else None
            d_out = mhc.DeviceBuffer(cap + GUARD, init=np.full(cap + GUARD, 0x5A, dtype=np.uint8))
            d_st = mhc.DeviceBuffer(4 * len(bt.msgs))
            wsb = int(ws_of(len(bt.msgs)))
            d_ws = mhc.DeviceBuffer(wsb)
            what = "%s %s %s" % (call.__name__, "indexed" if indexed else "free", name)
            mhc._check(call(handle, d_pl.ptr, d_po.ptr, d_nb.ptr, len(bt.msgs), int(pay_off[-1]), 0x20, d_out.ptr, cap, d_so.ptr,
                            int(sym_off[-1]) if indexed else 0, d_idx.ptr if indexed else None, bt.chunk if indexed else 0, d_st.ptr,
                            d_ws.ptr, wsb, None), what)
            l.mh_dev_status(d_ws.ptr, None)
            out, st, so = d_out.download(), d_st.download(np.int32), d_so.download(np.uint64)
            assert np.all(out[cap:] == 0x5A), "%s wrote at or beyond out_cap" % what
            expect_batch(out[:cap].tobytes(), so, st, want, what)


@pytest.mark.parametrize("indexed", [False, True])
def test_decompress_each(mhc, batch1, indexed):
    """One model per stream (every stream its own table file): mh_decompress_each."""
    bt = batch1
    table = bt.om.table_bytes()
    for at, name, pl, nb in bt.each_case(30):
        want = bt.verdicts(at, pl, nb, indexed)
        blobs = [bytes([mhc.stream_header(1, s[1])]) + s[0] for s in bt.streams]
        blobs[at] = bytes([mhc.stream_header(1, nb)]) + pl
        kw = dict(indices=[s[2] for s in bt.streams], chunk_symbols=bt.chunk, lengths=[len(m) for m in bt.msgs]) if indexed else {}
        msgs, st = mhc.decompress_each([table] * len(blobs), blobs, check=False, **kw)
        for i, (ws, wb) in enumerate(want):
            assert int(st[i]) == ws, "decompress_each %s: stream %d status %d, contract %d" % (name, i, int(st[i]), ws)
            if ws == MH_OK:
                assert msgs[i] == wb, "decompress_each %s: stream %d" % (name, i)


def test_decode_bank(mhc, oracle, batch1):
    """A bank of two models, every stream under the bank's model 1 (= the batch's model)."""
    bt = batch1
    other = mhc.Model.from_table(oracle.Model.from_data(text_like(50_000, 3).tobytes(), 1).table_bytes())
    bank = mhc.ModelSet.from_models([other, bt.m])
    choice = np.ones(len(bt.msgs), dtype=np.uint32)
    for indexed in (False, True):
        for at, name, pl, nb in bt.each_case(40):
            payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
            want = bt.verdicts(at, pl, nb, indexed)
            kw = dict(sym_off=sym_off, index=index, chunk_symbols=bt.chunk) if indexed else {}
            out, so, st = mhc.decode_bank(bank, choice, payload, pay_off, nbits, check=False, **kw)
            expect_batch(out, so, st, want, "decode_bank %s %s" % ("indexed" if indexed else "index-free", name))


@pytest.mark.parametrize("form", ["shared", "set"])
def test_segment_states(mhc, batch1, form):
    """mh_dev_batch_states / _index / _emit (shared model) and mh_dev_each_* (one model per stream): a failed stream decodes to
    0 symbols; index slices of the good streams equal the encoder's; nothing written beyond out_cap or index_cap; and
    mh_index_batch (host form)."""
    bt = batch1
    model = bt.m if form == "shared" else mhc.ModelSet.from_models([bt.m] * len(bt.msgs))
    l = mhc.lib()
    for at, name, pl, nb in bt.each_case(50):
        payload, pay_off, nbits, _, _ = bt.pack(at, pl, nb)
        want = bt.verdicts(at, pl, nb, False)
        ss = mhc.SegmentStates(model, payload, pay_off, nbits)
        assert [int(x) for x in ss.status] == [w[0] for w in want], name
        out, st, _ = ss.emit(guard=64)
        expect_batch(out, ss.sym_off, st, want, "%s emit %s" % (form, name), fail_len=0)
        idx, ist, _ = ss.index(bt.chunk, guard=8)
        assert [int(x) for x in ist] == [w[0] for w in want], name
        for i, (ws, wb) in enumerate(want):
            if ws == MH_OK:
                base = l.mh_batch_index_base(int(ss.sym_off[i]), i, bt.chunk)
                ref, _ = damage.expected_entries(np.asarray(bt.om.codes()[0]), np.frombuffer(wb, dtype=np.uint8), bt.chunk)
                assert np.array_equal(idx[base:base + ref.size], ref), (name, i)
        if form == "shared":
            so, hidx, hst = mhc.index_batch_host(bt.m, payload, pay_off, nbits, bt.chunk, check=False)
            assert [int(x) for x in hst] == [w[0] for w in want], "mh_index_batch " + name
            assert np.array_equal(so, ss.sym_off), name


def test_batch_lookups(mhc, batch1):
    """mh_decode_batch_ranges with the index: a lookup fails iff a chunk of its stream that it reads fails."""
    bt = batch1
    for at, name, pl, nb in bt.each_case(60):
        payload, pay_off, nbits, sym_off, index = bt.pack(at, pl, nb)
        lookups = []
        for i, msg in enumerate(bt.msgs):
            n = len(msg)
            lookups += [(i, 0, n), (i, 0, min(10, n)), (i, n // 2, n), (i, max(n - 3, 0), n - 1)]
        res, status = bt.m.decode_batch_ranges(payload, pay_off, nbits, lookups, sym_off=sym_off, index=index, chunk_symbols=bt.chunk)
        for (i, b, e), got, st in zip(lookups, res, status):
            spl, snb, sidx = (pl, nb, bt.streams[i][2]) if i == at else bt.streams[i][:3]
            want = damage.verdict_range(bt.om, spl, snb, sidx, bt.chunk, len(bt.msgs[i]), b, e)
            expect((int(st), got), want, "lookup (%d, %d, %d) %s" % (i, b, e, name))


def test_per_stream_lookups(mhc, batch1):
    """mh_decompress_each_ranges (one table per stream) with the index: a lookup fails iff a chunk it reads fails."""
    bt = batch1
    table = bt.om.table_bytes()
    for at, name, pl, nb in bt.each_case(80):
        blobs = [bytes([mhc.stream_header(1, s[1])]) + s[0] for s in bt.streams]
        blobs[at] = bytes([mhc.stream_header(1, nb)]) + pl
        lookups = []
        for i, msg in enumerate(bt.msgs):
            n = len(msg)
            lookups += [(i, 0, n), (i, 0, min(10, n)), (i, n // 2, n), (i, max(n - 3, 0), n - 1)]
        res, status = mhc.decompress_each_ranges([table] * len(blobs), blobs, lookups, indices=[s[2] for s in bt.streams],
                                                 chunk_symbols=bt.chunk, lengths=[len(m) for m in bt.msgs])
        for (i, b, e), got, st in zip(lookups, res, status):
            spl, snb, sidx = (pl, nb, bt.streams[i][2]) if i == at else bt.streams[i][:3]
            want = damage.verdict_range(bt.om, spl, snb, sidx, bt.chunk, len(bt.msgs[i]), b, e)
            expect((int(st), got), want, "each lookup (%d, %d, %d) %s" % (i, b, e, name))


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def test_cli_cut_inside_and_on_the_last_code(oracle, tmp_path):
    """`-x` on a `.cm` whose header remainder was raised: inside the last code, exit 1 with "corrupt"; on its start, the
    prefix."""
    from test_cli_gpu import BIN, run
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(entry.PKG_DIR, "host"), "-s"])
    text = text_like(400_000, 11).tobytes()
    om = oracle.Model.from_data(text, 1)
    lens = np.asarray(om.codes()[0])
    found = None
    for n in range(300_000, 300_400):
        cl = damage.code_lengths(lens, np.frombuffer(text[:n], dtype=np.uint8))
        blob, nbits = om.compress(text[:n])
        rem = blob[0] & 7
        if cl[-1] >= 2 and rem + int(cl[-1]) <= 7:
            found = (n, blob, int(cl[-1]), rem)
            break
    assert found
    n, blob, last, rem = found
    (tmp_path / "t.e").write_bytes(om.table_bytes())
    (tmp_path / "in.cm").write_bytes(bytes([blob[0] + 1]) + blob[1:])
    r = run([tmp_path / "in.cm", "-o", tmp_path / "out", "-x", "-e", tmp_path / "t.e"])
    assert r.returncode == 1 and b"corrupt" in r.stderr.lower(), (r.returncode, r.stderr)
    (tmp_path / "on.cm").write_bytes(bytes([blob[0] + last]) + blob[1:])
    r = run([tmp_path / "on.cm", "-o", tmp_path / "out2", "-x", "-e", tmp_path / "t.e"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out2").read_bytes() == text[:n - 1]
