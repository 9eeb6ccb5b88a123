"""The verdict matrix on a damaged chunk index: every reader that takes a compressed batch or stream "with an index" gets the
encoder's payload and a damaged index slice (tests/damage.py X1-X10: positions off by a bit or a symbol, at and past nbits,
behind the predecessor, entry 0 moved, entries swapped and shifted, bits that a 32-bit compare drops, a changed context field,
whole entries zero or ones, and the gaps between slices filled with ones), and must give the verdict, the bytes, the hits,
the digest, the counts and the re-coded stream that the CPU oracle gives for that slice (damage.verdict_indexed /
verdict_range, the oracle's chunk-wise bytes: under X8 they differ from the message).  Payloads, nbits and the intact index
come from the oracle, never from the encoder under test.  No case accepts more than one verdict and none is skipped; the
last test of the module asserts that every (kind, reader) pair ran.

Why every read stays inside the stream's payload dwords and every write inside its output, by reader (read before any of
these cases first went to a device; none of them is meant to make a kernel fault):
  - batch decode (mh_batch.hip dec_idx_kernel, its own copy of chunk_of's steps), search (mh_find.hip), digests (mh_crc.hip),
    coded histogram and re-coding (mh_recode.hip): a chunk is read only after Chunk::entry_ok (start <= end <= nbits_i), and
    nbits_i <= 8 x the stream's payload bytes since check_batch.  The cursor starts at bit0 + start of mhb::stream_src, whose
    BitSrc covers exactly the dwords of the stream's bytes: BitSrc::word returns whole dwords below full_words and single
    bytes b < bytes behind them, zero past the end, so a decode that runs on from a wrong start reads zeros, never memory.
    The context field indexes tables of 256 (order 0/1: one byte; a set's ctx_slot row has 256 entries, NO_SLOT is tested)
    or 65 536 contexts (order 2: two bytes; prim holds 65 536 x 256 entries, DEC16_NULL where no table is).  Writes never
    depend on an entry: decode stores nsym bytes at sym_off[i] + first, the search stores records r < r1 <= hit_off[n] and
    r < hit_cap, the digests one word per stream, the re-coder the bits its length pass counted with the same decode.
  - lookups (mh_range.hip lookup_kernel, range_kernel): an item is decoded only when its entry is <= nbits and not behind the
    entry in front, and an exact item only when the next entry lies in [start, nbits]; the single-stream kernel also needs
    the span inside the payload window (MH_ERR_ARG else).  The source is the same stream_src / BitSrc.
  - single-stream chunk decoder (mh_decode.hip): the interleaved body initialises a lane only when `fine` holds (bitpos <
    nbits, endpos >= bitpos, endpos - bitpos <= 64 bits per symbol), decode_chunk_single returns on bitpos >= nbits in its
    first line, decode2_kernel on pos >= nbits or an end outside [pos, nbits]; LaneStream clamps every granule load to the
    granule of the last payload byte (glast), and the buffers here are padded as the call asks.  Output addresses come from
    the chunk number alone.
  - host forms (mh_decode with an index, mh_decode_ranges): entry 0 and the end must give pos0 <= pos1 <= nbits before a
    byte is uploaded, every entry below pos0 is refused, spans are taken only between entries s <= end <= nbits.
"""
import functools
import os
import re
import zlib

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import damage
import find_ref
from damage import MH_OK, MH_ERR_CORRUPT
from test_gpu_damaged_streams import (DEC_CHUNK, GUARD, VARIANTS, Source, chunk_decode, expect, expect_batch, host_decode, mhc,  # noqa: F401
                                      text_like, zipf_bytes)

pytestmark = pytest.mark.gpu

LENGTHS = (1500, 257, 1024, 0, 700)            # slices of 6, 2, 4, 0 and 3 entries at chunk 256
CHUNK = 256
MODEL_KINDS = ("o0", "o1", "flat", "each", "bank", "o2")
KINDS = tuple("X%d" % k for k in range(1, 11))
RAN = set()                                    # (damage kind, reader) pairs that ran, for the last test


def ran(name, *readers):
    for r in readers:
        RAN.add((name.split("-")[0], r))


def zipf200(n, seed):
    """Zipf over 200 symbols: the contexts 200..255 have no table."""
    return zipf_bytes(n, seed, k=200)


class IBatch:
    """Five streams of LENGTHS symbols at chunk 256 under one model kind, all from the oracle: payloads, nbits, index slices.
    The damaged stream stands first, in the middle and last in turn (`at`), with a damaged slice in place of its own."""

    def __init__(self, mhc, oracle, kind):
        self.mhc, self.kind, self.chunk = mhc, kind, CHUNK
        self.order = 2 if kind == "o2" else (0 if kind == "o0" else 1)
        self.prev0 = 0x2020 if self.order == 2 else 0x20
        n = len(LENGTHS)
        if kind == "o2":
            msgs = [text_like(k, 70 + i) for i, k in enumerate(LENGTHS)]
        elif kind == "flat":
            msgs = [np.random.default_rng(80 + i).integers(0, 256, k).astype(np.uint8) for i, k in enumerate(LENGTHS)]
        else:
            msgs = [zipf200(k, 90 + i) for i, k in enumerate(LENGTHS)]
        self.msgs = [m.tobytes() for m in msgs]
        hist = {0: oracle.histogram_o0, 1: oracle.histogram_o1, 2: oracle.histogram_o2}[self.order]
        total = lambda which: sum(hist(self.msgs[i]).astype(np.uint64) for i in which)
        self.choice = None
        if kind == "each":
            self.oms = [oracle.Model.from_counts(total([i]), 1) for i in range(n)]
            self.model = mhc.ModelSet.from_tables([om.table_bytes() for om in self.oms])
        elif kind == "bank":
            self.choice = np.array([1, 0, 1, 0, 1], dtype=np.uint32)
            oms = [oracle.Model.from_counts(total([1, 3]) + oracle.histogram_o1(zipf200(5000, 5).tobytes()).astype(np.uint64), 1),
                   oracle.Model.from_counts(total([0, 2, 4]), 1)]
            self.oms = [oms[c] for c in self.choice]
            self.bank_models = [mhc.Model.from_table(om.table_bytes()) for om in oms]
            self.bank = mhc.ModelSet.from_models(self.bank_models)
            self.model = self.bank.pick(self.choice)
        else:
            om = oracle.Model.from_counts(damage.flat_counts(3) if kind == "flat" else total(range(n)), self.order)
            self.oms = [om] * n
            self.model = mhc.Model.from_table(om.table_bytes())
        self.lens = [np.asarray(om.codes_o2()[0] if self.order == 2 else om.codes()[0]) for om in (self.oms if kind in ("each", "bank") else self.oms[:1])]
        if len(self.lens) == 1:
            self.lens = self.lens * n
        self.streams = []
        for i, msg in enumerate(msgs):
            blob, nb = self.oms[i].compress(msg.tobytes())
            idx, _ = damage.expected_entries(self.lens[i], msg, CHUNK, self.prev0, self.order)
            b = damage.boundaries(self.lens[i], msg, self.order, self.prev0)
            assert int(b[-1]) == nb and damage.verdict_indexed(self.oms[i], blob[1:], nb, idx, CHUNK, len(msg), self.order) == (MH_OK, msg.tobytes())
            self.streams.append((blob[1:], nb, idx, b))
        assert [s[2].size for s in self.streams] == [6, 2, 4, 0, 3]
        self.payload, self.pay_off = mhc.batch_offsets([s[0] for s in self.streams])
        self.nbits = np.array([s[1] for s in self.streams], dtype=np.uint64)
        self.sym_off = np.zeros(n + 1, dtype=np.uint64)
        self.sym_off[1:] = np.cumsum(LENGTHS)
        l = mhc.lib()
        self.bases = [int(l.mh_batch_index_base(int(self.sym_off[i]), i, CHUNK)) for i in range(n)]
        self.icap = max(int(l.mh_batch_index_capacity(int(self.sym_off[-1]), n, CHUNK)), 1)
        self._cases = None

    def index(self, at=None, sl=None, gaps=False):
        idx = np.zeros(self.icap, dtype=np.uint64)
        for i, s in enumerate(self.streams):
            idx[self.bases[i]:self.bases[i] + s[2].size] = sl if i == at else s[2]
        return damage.x10_gaps(idx, self.bases, [s[2].size for s in self.streams])[1] if gaps else idx

    def args(self, idx):
        return dict(sym_off=self.sym_off, index=idx, chunk_symbols=CHUNK)

    def cases(self):
        """(at, name, batch index, damaged slice, per-stream verdicts, k = the first damaged entry): X1-X9 with the damaged
        stream first, in the middle (every position of the generators) and last (the first and the last entry), then X10."""
        if self._cases is None:
            out = []
            for j, at in enumerate((0, 2, 4)):
                pl, nb, sl0, b = self.streams[at]
                ks = None if at == 2 else (0, sl0.size - 1)
                for name, sl in damage.index_damages(sl0, b, nb, self.order, self.lens[at], seed=11 + j, ks=ks):
                    want = [(MH_OK, m) for m in self.msgs]
                    want[at] = damage.verdict_indexed(self.oms[at], pl, nb, sl, CHUNK, LENGTHS[at], self.order)
                    out.append((at, "%s (stream %d)" % (name, at), self.index(at, sl), sl, want, int(np.flatnonzero(sl != sl0)[0])))
            out.append((2, "X10-gaps", self.index(gaps=True), self.streams[2][2], [(MH_OK, m) for m in self.msgs], 1))
            assert {c[1].split("-")[0] for c in out} == set(KINDS)
            self._cases = out
        return self._cases

    def soft(self, at, sl, want):
        """The damaged stream decodes, but from a slice that is not the encoder's: what a reader takes from an entry's context
        field beside the decode (the context of a chunk's first symbol for a histogram or a destination code) is then only
        bound by the promises of include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING"."""
        return want[at][0] == MH_OK and not np.array_equal(sl, self.streams[at][2])


@functools.lru_cache(None)
def _batch(kind):
    from oracle import mh_oracle
    return IBatch(entry.load_package(), mh_oracle, kind)


@pytest.fixture(scope="module", params=MODEL_KINDS)
def ib(request, mhc):
    return _batch(request.param)


# ---- decode ---------------------------------------------------------------------------------------------------------------
def dev_decode(bt, idx):
    """The device decode call of the model kind into exactly sym_total bytes + guard: (bytes, status per stream)."""
    mhc, l, n = bt.mhc, bt.mhc.lib(), len(LENGTHS)
    if bt.kind in ("each", "bank"):
        out, so, st, _ = bt.model.decode(bt.payload, bt.pay_off, bt.nbits, guard=GUARD, **bt.args(idx))
        assert np.array_equal(so, bt.sym_off)
        return out, st
    call, ws_of = ((l.mh_dev_decode_batch_o2, l.mh_dev_decode_batch_o2_workspace) if bt.kind == "o2"
                   else (l.mh_dev_decode_batch, l.mh_dev_decode_batch_workspace))
    cap = int(bt.sym_off[-1])
    d_pl = mhc.DeviceBuffer(bt.payload.size + 64, init=np.concatenate([bt.payload, np.zeros(64, dtype=np.uint8)]))
    d_po, d_nb = mhc.DeviceBuffer(bt.pay_off.nbytes, init=bt.pay_off), mhc.DeviceBuffer(bt.nbits.nbytes, init=bt.nbits)
    d_so, d_idx = mhc.DeviceBuffer(bt.sym_off.nbytes, init=bt.sym_off), mhc.DeviceBuffer(idx.nbytes, init=idx)
    d_out = mhc.DeviceBuffer(cap + GUARD, init=np.full(cap + GUARD, 0x5A, dtype=np.uint8))
    d_st = mhc.DeviceBuffer(4 * n)
    wsb = int(ws_of(n))
    d_ws = mhc.DeviceBuffer(wsb)
    mhc._check(call(bt.model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(bt.pay_off[-1]), 0x20, d_out.ptr, cap, d_so.ptr, cap, d_idx.ptr,
                    CHUNK, d_st.ptr, d_ws.ptr, wsb, None), call.__name__)
    l.mh_dev_status(d_ws.ptr, None)
    out = d_out.download()
    assert np.all(out[cap:] == 0x5A), "wrote at or beyond out_cap"
    assert np.array_equal(d_so.download(np.uint64), bt.sym_off)
    return out[:cap].tobytes(), d_st.download(np.int32)


def host_decode_batch(bt, idx):
    if bt.kind == "bank":
        return bt.mhc.decode_bank(bt.bank, bt.choice, bt.payload, bt.pay_off, bt.nbits, check=False, **bt.args(idx))
    if bt.kind == "each":
        blobs = [bytes([bt.mhc.stream_header(1, s[1])]) + s[0] for s in bt.streams]
        msgs, st = bt.mhc.decompress_each([om.table_bytes() for om in bt.oms], blobs, check=False, chunk_symbols=CHUNK, lengths=list(LENGTHS),
                                          indices=[idx[bt.bases[i]:bt.bases[i] + s[2].size] for i, s in enumerate(bt.streams)])
        so = bt.sym_off
        return b"".join(m if s == MH_OK else bytes(int(so[i + 1] - so[i])) for i, (m, s) in enumerate(zip(msgs, st))), so, st
    fn = bt.model.decode_batch_o2 if bt.kind == "o2" else bt.model.decode_batch
    return fn(bt.payload, bt.pay_off, bt.nbits, check=False, **bt.args(idx))


def test_decode(ib):
    """mh_dev_decode_batch (orders 0 and 1), mh_dev_decode_each (a set, a picked bank view), mh_dev_decode_batch_o2; every third
    case the host forms as well (mh_decode_batch, mh_decompress_each, mh_decode_bank, mh_decode_batch_o2)."""
    for j, (at, name, idx, sl, want, k) in enumerate(ib.cases()):
        out, st = dev_decode(ib, idx)
        expect_batch(out, ib.sym_off, st, want, "device decode %s %s" % (ib.kind, name))
        ran(name, "decode")
        if j % 3 == 0 or name.startswith("X10"):
            out, so, st = host_decode_batch(ib, idx)
            assert np.array_equal(so, ib.sym_off)
            expect_batch(out, so, st, want, "host decode %s %s" % (ib.kind, name))
            ran(name, "decode-host")


# ---- lookups --------------------------------------------------------------------------------------------------------------
def lookups_of(at, k):
    n, c = LENGTHS[at], CHUNK
    nch = (n + c - 1) // c
    lk = [(at, 0, n)] + [(at, j * c, min((j + 1) * c, n)) for j in range(nch)] + [(at, j * c - 3, min(j * c + 3, n)) for j in range(1, nch)]
    lk.append((at, k * c + 1, min(k * c + 5, n - 1)))                     # ends inside the damaged chunk
    if k:
        lk.append((at, k * c - 5, k * c))                                  # ends on its start boundary
    far = [j for j in range(nch) if abs(j - k) > 1]
    if far:
        lk.append((at, far[-1] * c + 2, far[-1] * c + 9))                  # in an untouched chunk
    lk.append((at, 7, 7))
    other = {0: 1, 2: 1, 4: 2}[at]                                         # a neighbour that is intact
    lk += [(other, 0, LENGTHS[other]), (other, 3, 9)]
    return lk


def test_lookups(ib):
    """mh_dev_decode_batch_ranges, mh_dev_decode_each_ranges, mh_dev_decode_batch_o2_ranges against damage.verdict_range."""
    bt = ib
    call = (bt.model.dev_decode_batch_o2_ranges if bt.kind == "o2" else bt.model.decode_ranges if bt.kind in ("each", "bank")
            else bt.model.dev_decode_batch_ranges)
    for at, name, idx, sl, want, k in bt.cases():
        lk = lookups_of(at, k)
        res, status, _ = call(bt.payload, bt.pay_off, bt.nbits, lk, **bt.args(idx))
        for (i, b, e), got, st in zip(lk, res, status):
            pl, nb, isl, _ = bt.streams[i]
            w = damage.verdict_range(bt.oms[i], pl, nb, sl if i == at else isl, CHUNK, LENGTHS[i], b, e, bt.order)
            expect((int(st), got), w, "lookup (%d, %d, %d) %s %s" % (i, b, e, bt.kind, name))
        ran(name, "lookups")


# ---- digests --------------------------------------------------------------------------------------------------------------
def test_digest(ib):
    """mh_dev_crc_batch, mh_dev_crc_each, mh_dev_crc_batch_o2: zlib's CRC-32 and the length of every stream that decodes, 0 and
    0 for a failed one."""
    bt = ib
    call = bt.model.dev_crc_batch_o2 if bt.kind == "o2" else bt.model.crc if bt.kind in ("each", "bank") else bt.model.dev_crc_batch
    for at, name, idx, sl, want, k in bt.cases():
        crc, ln, st, _ = call(bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
        for i, (ws, wb) in enumerate(want):
            assert int(st[i]) == ws, "crc %s %s: stream %d status %d, contract %d" % (bt.kind, name, i, int(st[i]), ws)
            assert (int(crc[i]), int(ln[i])) == ((zlib.crc32(wb), len(wb)) if ws == MH_OK else (0, 0)), (bt.kind, name, i)
        ran(name, "digest")


# ---- search ---------------------------------------------------------------------------------------------------------------
def patterns_of(bt, at, want, k):
    """From the oracle's bytes: the four bytes across the damaged seam as decode returns them, the four across it in the
    original message (reported only where the decoded bytes hold them), four inside the damaged chunk, and two frequent pairs."""
    msg = bt.msgs[at]
    out = want[at][1] if want[at][0] == MH_OK else msg
    s = max(k, 1) * CHUNK
    pats = [out[s - 2:s + 2], msg[s - 2:s + 2], out[k * CHUNK + 10:k * CHUNK + 14], bt.msgs[0][CHUNK - 1:CHUNK + 1], bt.msgs[2][2 * CHUNK - 1:2 * CHUNK + 1]]
    assert all(len(p) in (2, 4) for p in pats)
    return pats


def test_search(ib):
    """mh_dev_find_batch / mh_dev_find_dict_batch, their _each and _o2 forms, count-only and with records: the hits are those of
    find_ref.find_hits on the bytes the decoders return for the same arguments; a failed stream has none."""
    bt = ib
    m = bt.model
    if bt.kind == "o2":
        calls = [("find", m.dev_find_batch_o2, bt.mhc.PatternSet), ("find-dict", m.dev_find_dict_batch_o2, bt.mhc.Dict)]
    elif bt.kind in ("each", "bank"):
        calls = [("find", m.find, bt.mhc.PatternSet), ("find-dict", m.find_dict, bt.mhc.Dict)]
    else:
        calls = [("find", m.dev_find_batch, bt.mhc.PatternSet), ("find-dict", m.dev_find_dict_batch, bt.mhc.Dict)]
    for at, name, idx, sl, want, k in bt.cases():
        pats = patterns_of(bt, at, want, k)
        hits = find_ref.find_hits([wb if ws == MH_OK else b"" for ws, wb in want], pats)
        r_off, r_rec, r_pat = find_ref.hit_arrays(hits, len(want))
        for reader, call, make in calls:
            ps = make(pats)
            what = "%s %s %s" % (reader, bt.kind, name)
            ho, _, _, st, _ = call(ps, bt.payload, bt.pay_off, bt.nbits, count_only=True, **bt.args(idx))
            assert [int(x) for x in st] == [w[0] for w in want], what
            assert np.array_equal(ho, r_off), "%s count-only: hit_off %s, reference %s" % (what, ho, r_off)
            ho, rec, pat, st, _ = call(ps, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            assert [int(x) for x in st] == [w[0] for w in want], what
            assert np.array_equal(ho, r_off), "%s: hit_off %s, reference %s" % (what, ho, r_off)
            assert np.array_equal(rec, r_rec) and np.array_equal(pat, r_pat), "%s: records differ" % what
            ran(name, reader)


# ---- coded histogram and re-coding ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def dst_model():
    """The destination of every re-code: the flat order-1 model (every pair has an 8-bit code, nothing is dropped)."""
    from oracle import mh_oracle
    om = mh_oracle.Model.from_counts(damage.flat_counts(21), 1)
    lens, codes = om.codes()
    return entry.load_package().Model.from_table(om.table_bytes()), np.asarray(lens).astype(np.int64), np.asarray(codes)


@functools.lru_cache(None)
def packed(msg):
    _, lens, codes = dst_model()
    return batch_ref.pack([msg], lens, codes, 1, chunk=CHUNK)


def test_coded_histogram(ib):
    """mh_dev_histogram_coded_batch (orders 0 and 1), _each and _batch_o2: a failed stream's counts are absent."""
    bt = ib
    for at, name, idx, sl, want, k in bt.cases():
        soft = bt.soft(at, sl, want)
        for order in (0, 1):
            if bt.kind == "o2":
                counts, st, _ = bt.model.dev_histogram_coded_o2(order, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            elif bt.kind in ("each", "bank"):
                counts, st, _ = bt.model.histogram_coded(order, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            else:
                counts, st, _ = bt.model.dev_histogram_coded(order, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            what = "coded histogram order %d %s %s" % (order, bt.kind, name)
            assert [int(x) for x in st] == [w[0] for w in want], what
            good = [wb if ws == MH_OK and not (soft and i == at) else b"" for i, (ws, wb) in enumerate(want)]
            ref = batch_ref.histogram(good, order)
            if not soft:
                assert np.array_equal(counts, ref), what
            else:                                    # the stream's own counts: as many as it has symbols, none negative
                own = counts.astype(np.int64) - ref.astype(np.int64)
                assert own.min() >= 0 and int(own.sum()) == LENGTHS[at], what
                if order == 0:
                    assert np.array_equal(counts, batch_ref.histogram([wb for _, wb in want], 0)), what
        ran(name, "histogram")


def test_recode(ib):
    """mh_dev_recode_batch, mh_dev_recode_each, mh_dev_recode_batch_o2 and their count-only forms."""
    bt = ib
    dst, _, _ = dst_model()
    call = bt.model.dev_recode_batch_o2 if bt.kind == "o2" else bt.model.recode if bt.kind in ("each", "bank") else bt.model.dev_recode_batch
    for at, name, idx, sl, want, k in bt.cases():
        what = "recode %s %s" % (bt.kind, name)
        soft = bt.soft(at, sl, want)
        cnt = call(dst, bt.payload, bt.pay_off, bt.nbits, count_only=True, **bt.args(idx))
        r = call(dst, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
        assert [int(x) for x in r["status"]] == [w[0] for w in want] == [int(x) for x in cnt["status"]], what
        for key in ("out_off", "nbits", "dropped"):
            assert np.array_equal(cnt[key], r[key]), "%s: count-only %s differs" % (what, key)
        assert np.array_equal(cnt["index"], r["index"]), what
        assert int(r["out_off"][-1]) == r["payload"].size and int(r["out_off"][0]) == 0, what
        for i, (ws, wb) in enumerate(want):
            a, e = int(r["out_off"][i]), int(r["out_off"][i + 1])
            got_sl = r["index"][bt.bases[i]:bt.bases[i] + bt.streams[i][2].size]
            if ws != MH_OK:                          # nbits 0, no payload byte, an untouched index slice, dropped 0
                assert (int(r["nbits"][i]), e - a, int(r["dropped"][i])) == (0, 0, 0), (what, i)
                assert np.all(got_sl == np.uint64(bt.mhc.FIND_FILL)), (what, i)
            elif soft and i == at:
                assert e - a == (int(r["nbits"][i]) + 7) // 8 and int(r["dropped"][i]) == 0, (what, i)
                assert int(r["nbits"][i]) == 8 * LENGTHS[i], (what, i)          # (every code of the destination has 8 bits)
            else:
                ref = packed(wb)
                assert (int(r["nbits"][i]), int(r["dropped"][i])) == (int(ref.nbits[0]), 0), (what, i)
                assert r["payload"][a:e].tobytes() == ref.payload.tobytes(), "%s: stream %d payload differs" % (what, i)
                assert np.array_equal(got_sl, ref.slices[0] if ref.slices and len(wb) else np.zeros(0, dtype=np.uint64)), (what, i)
        if soft:                                     # two calls give identical buffers
            r2 = call(dst, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            assert np.array_equal(r2["payload"], r["payload"]) and np.array_equal(r2["index"], r["index"]), what
            assert np.array_equal(r2["out_off"], r["out_off"]) and np.array_equal(r2["nbits"], r["nbits"]), what
        ran(name, "recode")


def test_seam_recode_to_an_order_2_destination(mhc, oracle):
    """mh_dev_recode_batch_o2 with the shared order-1 sources and an order-2 destination: the lane in front codes a chunk's first
    symbol (include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING").  Verdicts as the decoders'; count-only sizes equal the full
    call's; a failed stream gets nothing; every stream decoded from the encoder's own slice is exact."""
    text = text_like(20000, 9).tobytes()
    om2 = oracle.Model.from_data(text, 2)
    dst = mhc.Model.from_table(om2.table_bytes())
    lens, codes = om2.codes_o2()
    lens, codes = np.asarray(lens).astype(np.int64), np.asarray(codes)
    for kind in ("o1", "flat"):
        bt = _batch(kind)
        ref = {i: batch_ref.pack([m], lens, codes, 2, chunk=CHUNK) for i, m in enumerate(bt.msgs)}
        for at, name, idx, sl, want, k in bt.cases():
            what = "seam recode %s %s" % (kind, name)
            cnt = bt.model.dev_recode_batch_o2(dst, bt.payload, bt.pay_off, bt.nbits, count_only=True, **bt.args(idx))
            r = bt.model.dev_recode_batch_o2(dst, bt.payload, bt.pay_off, bt.nbits, **bt.args(idx))
            assert [int(x) for x in r["status"]] == [w[0] for w in want] == [int(x) for x in cnt["status"]], what
            for key in ("out_off", "nbits", "dropped", "index"):
                assert np.array_equal(cnt[key], r[key]), "%s: count-only %s differs" % (what, key)
            assert int(r["out_off"][-1]) == r["payload"].size, what
            for i, (ws, wb) in enumerate(want):
                a, e = int(r["out_off"][i]), int(r["out_off"][i + 1])
                if ws != MH_OK:
                    assert (int(r["nbits"][i]), e - a, int(r["dropped"][i])) == (0, 0, 0), (what, i)
                elif i != at or np.array_equal(sl, bt.streams[at][2]):
                    assert (int(r["nbits"][i]), int(r["dropped"][i])) == (int(ref[i].nbits[0]), int(ref[i].dropped[0])), (what, i)
                    assert r["payload"][a:e].tobytes() == ref[i].payload.tobytes(), (what, i)
                else:
                    assert e - a == (int(r["nbits"][i]) + 7) // 8, (what, i)
            ran(name, "recode-seam")


# ---- single streams -------------------------------------------------------------------------------------------------------
def dec_shape(variant):
    """(k, NT) of a variant of the chunk decoder, read from dec_cfg in csrc/mh_decode.hip: streams per lane, lanes per group."""
    src = open(os.path.join(entry.PKG_DIR, "csrc", "mh_decode.hip")).read()
    m = re.search(r"v == DV_%s\s*\?\s*DecCfg\{\s*\w+,\s*\d+,\s*(\d+)," % variant, src)
    nt = re.search(r"constexpr int DEC_NT = (\d+);", src)
    return int(m.group(1)), int(nt.group(1))


class View:
    """A Source with another index (chunk_decode reads src.index)."""

    def __init__(self, src, index):
        self.__dict__.update(src.__dict__)
        self.index = index


def fast_verdict(s, sl):
    """damage.verdict_indexed, with the chunks whose entry and end are the encoder's taken as decoded (they pass by
    construction: Source asserts the intact stream)."""
    same = sl == s.index
    changed = [int(j) for j in np.flatnonzero(~(same & np.concatenate([same[1:], [True]])))]
    cv = damage.chunk_verdicts(s.om, s.payload, s.nbits, sl, s.chunk, s.data.size, s.order, only=changed)
    if not all(ok for ok, _ in cv):
        return MH_ERR_CORRUPT, None
    b = bytearray(s.data.tobytes())
    for j, (_, by) in zip(changed, cv):
        b[j * s.chunk:j * s.chunk + len(by)] = by
    return MH_OK, bytes(b)


@pytest.mark.parametrize("kind,variant", [("LDS_WIDE", "LDS_WIDE"), ("REDO_LDS", "LDS_TWO_LEVEL_P8"), ("REDO_L2_DIRECT", "L2_DIRECT_H8")])
def test_single_stream_chunk_decoder(mhc, oracle, kind, variant):
    """mh_dev_decode on the variant recipes of test_gpu_damaged_streams.py, the smallest stream that reaches the interleaved
    body (k streams per lane, NT lanes: (k - 1) NT + 4 full chunks put chunks 0..3 + j NT there and every other chunk in the
    end part), with one damaged entry in the body, one in the end part and the last one; every third case mh_decode with the
    index as well."""
    from test_gpu_decode_variants import recipe
    k, nt = dec_shape(variant)
    body = (k - 1) * nt + 1
    counts, data = recipe(kind)
    data = data[:((k - 1) * nt + 4) * 256 + 77]
    counts = counts.reshape(-1) + oracle.histogram_o1(data.tobytes()).astype(np.uint64)
    s = Source(mhc, oracle, data, counts=counts, chunk=256, seed=4, per_kind=1, kmax=2)
    assert s.index.size == (k - 1) * nt + 5
    lens = np.asarray(s.om.codes()[0])
    cases = damage.index_damages(s.index, s.bounds, s.nbits, 1, lens, seed=6, ks=(body, 100, s.index.size - 1))
    for j, (name, sl) in enumerate(cases):
        want = fast_verdict(s, sl)
        path, var, got = chunk_decode(mhc, View(s, sl), s.payload, s.nbits)
        assert path == DEC_CHUNK and VARIANTS.get(var) == variant, (name, path, var)
        expect(got, want, "chunk decoder %s %s" % (kind, name))
        ran(name, "single-dev")
        if j % 3 == 0:
            expect(host_decode(mhc, s.m, s.payload, s.nbits, sl, s.chunk, s.data.size), want, "mh_decode indexed %s %s" % (kind, name))
            ran(name, "single-host")
    # the generators' verdicts through the plain contract on one case of every kind (fast_verdict is a shortcut)
    for name, sl in cases[::7]:
        assert fast_verdict(s, sl) == damage.verdict_indexed(s.om, s.payload, s.nbits, sl, s.chunk, s.data.size), name


def test_single_stream_order_2(mhc, oracle):
    """mh_dev_decode and mh_decode with an order-2 model and a damaged order-2 index."""
    s = Source(mhc, oracle, text_like(3000, 13), order=2, chunk=256, seed=5, per_kind=1, kmax=2)
    lens = np.asarray(s.om.codes_o2()[0])
    for name, sl in damage.index_damages(s.index, s.bounds, s.nbits, 2, lens, seed=8):
        want = damage.verdict_indexed(s.om, s.payload, s.nbits, sl, s.chunk, s.data.size, 2)
        _, _, got = chunk_decode(mhc, View(s, sl), s.payload, s.nbits)
        expect(got, want, "order-2 mh_dev_decode " + name)
        expect(host_decode(mhc, s.m, s.payload, s.nbits, sl, s.chunk, s.data.size), want, "order-2 mh_decode " + name)
        ran(name, "single-o2")


def test_single_stream_ranges(mhc, oracle):
    """mh_decode_ranges and mh_dev_decode_ranges with the chunk index only."""
    from test_gpu_range import dev_ranges
    s = Source(mhc, oracle, zipf200(3000, 17), chunk=256, seed=6, per_kind=1, kmax=2)
    lens = np.asarray(s.om.codes()[0])
    n, c = s.data.size, s.chunk
    d_pl = mhc.DeviceBuffer(len(s.payload) + 64, init=np.concatenate([np.frombuffer(s.payload, dtype=np.uint8), np.zeros(64, dtype=np.uint8)]))
    for name, sl in damage.index_damages(s.index, s.bounds, s.nbits, 1, lens, seed=9):
        k = int(np.flatnonzero(sl != s.index)[0])
        rg = [(0, n), (k * c, min((k + 1) * c, n)), (k * c + 1, min(k * c + 5, n - 1)), (max(k * c - 5, 0), max(k * c, 1)),
              (max(k * c - 3, 0), min(k * c + 3, n)), (7, 7)]
        far = [j for j in range(s.index.size) if abs(j - k) > 1]
        rg.append((far[-1] * c + 2, far[-1] * c + 9))
        want = [damage.verdict_range(s.om, s.payload, s.nbits, sl, c, n, b, e) for b, e in rg]
        res, status = s.m.decode_ranges(s.payload, s.nbits, sl, c, n, rg)
        for (b, e), got, st, w in zip(rg, res, status, want):
            expect((int(st), got), w, "mh_decode_ranges [%d, %d) %s" % (b, e, name))
        d_idx = mhc.DeviceBuffer(sl.nbytes, init=np.ascontiguousarray(sl))
        rc, _, st, out, out_at, _ = dev_ranges(mhc, s.m, d_pl.ptr, 0, len(s.payload), s.nbits, d_idx.ptr, c, n, None, rg)
        assert rc == 0
        for j, ((b, e), w) in enumerate(zip(rg, want)):
            a = int(out_at[j])
            expect((int(st[j]), out[a:a + e - b].tobytes()), w, "mh_dev_decode_ranges [%d, %d) %s" % (b, e, name))
        ran(name, "single-ranges")


# ---- coverage -------------------------------------------------------------------------------------------------------------
def test_every_kind_met_every_reader():
    """Runs last: every damage kind went through every reader (X10 is a damage of a batch: the single-stream readers have no
    gaps)."""
    batch = ("decode", "decode-host", "lookups", "digest", "find", "find-dict", "histogram", "recode", "recode-seam")
    single = ("single-dev", "single-host", "single-o2", "single-ranges")
    missing = [(k, r) for k in KINDS for r in batch + (single if k != "X10" else ()) if (k, r) not in RAN]
    assert not missing, missing
