"""Digests of compressed batches on the GPU (include/mh.h, "DIGESTS OF BATCHES"): the CRC-32 and the length of every stream's
decoded message under a shared model of order 0, 1 and 2, per-stream models and a picked bank, with and without the chunk
index, through the device and the host forms, and the same digest of uncompressed batches.  Every expected value comes from
zlib.crc32 and len of the original messages (for damaged streams: of the bytes the strict CPU oracle decodes), never from
another call of the library.  The device-call wrappers (Model.dev_crc_batch, ModelSet.crc, crc_raw_batch) put guard words
behind crc and len and assert that they kept their fill."""
import ctypes as C
import gc
import os
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import damage
from conftest import ROOT, golden
from oracle import mh_oracle

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "bin", "markovhuffman")


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


def digests(msgs):
    """(crc[n] uint32, len[n] uint64) of the messages by zlib.crc32 and len."""
    return np.array([zlib.crc32(m) for m in msgs], dtype=np.uint32), np.array([len(m) for m in msgs], dtype=np.uint64)


class Packed:
    """A batch of messages under one shared order-`order` model trained on them, encoded with an index of `chunk`."""

    def __init__(self, mhc, msgs, chunk, order=1, model=None):
        self.mhc, self.msgs, self.chunk, self.order = mhc, [bytes(m) for m in msgs], chunk, order
        if model is None:
            counts = mhc.histogram_o2_batch(self.msgs) if order == 2 else mhc.histogram_o1_batch(self.msgs, order=order)
            model = mhc.Model.from_counts(counts, order)
        self.model = model
        enc = model.encode_batch_o2 if order == 2 else model.encode_batch
        self.payload, self.pay_off, self.nbits, self.index, self.sym_off = enc(self.msgs, chunk_symbols=chunk)
        self.want = digests(self.msgs)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else {}

    def crc(self, indexed, **kw):
        fn = self.model.dev_crc_batch_o2 if self.order == 2 else self.model.dev_crc_batch
        return fn(self.payload, self.pay_off, self.nbits, **self.kw(indexed), **kw)

    def host(self, indexed, **kw):
        fn = self.model.crc_batch_o2 if self.order == 2 else self.model.crc_batch
        return fn(self.payload, self.pay_off, self.nbits, **self.kw(indexed), **kw)


def check(mhc, got, want, what=""):
    """A result (crc, len, statuses, status word or return code) against zlib's digests."""
    crc, ln, st, rc = got
    assert rc == mhc.MH_OK and (st == mhc.MH_OK).all(), (what, rc, np.unique(st))
    bad = np.flatnonzero(crc != want[0])
    assert bad.size == 0, "%s: %d CRCs differ, first stream %d" % (what, bad.size, bad[0])
    assert np.array_equal(ln, want[1]), what


def check_all_ways(mhc, b, what=""):
    """Indexed and index-free, the device and the host form: the same answer."""
    for indexed in (True, False):
        check(mhc, b.crc(indexed), b.want, "%s device indexed=%s" % (what, indexed))
        check(mhc, b.host(indexed), b.want, "%s host indexed=%s" % (what, indexed))


@pytest.fixture(scope="module")
def wiki_lines():
    lines = [l for l in golden()["input_wiki_cpp.html"]["data"].split(b"\n") if l]
    assert len(lines) == 1581 and max(len(l) for l in lines) == 21588
    return lines


@pytest.fixture(scope="module")
def wiki_want(wiki_lines):
    return digests(wiki_lines)


# ---- the shapes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("order", [0, 1])
def test_wiki_lines(mhc, wiki_lines, wiki_want, order, chunk):
    b = Packed(mhc, wiki_lines, chunk, order)
    assert np.array_equal(b.want[0], wiki_want[0]) and len(set(wiki_want[0].tolist())) > 1000
    check_all_ways(mhc, b, "wiki lines order %d chunk %d" % (order, chunk))
    crc, ln, st, rc = b.crc(True, want_len=False, want_status=False)       # len and the statuses may be NULL
    assert ln is None and st is None and rc == mhc.MH_OK and np.array_equal(crc, wiki_want[0])


@pytest.mark.parametrize("chunk", [256, 1024])
def test_wiki_as_one_stream(mhc, chunk):
    data = golden()["input_wiki_cpp.html"]["data"]
    assert len(data) // chunk >= 300 and len(data) % chunk                 # hundreds of chunks combine, the last one is ragged
    b = Packed(mhc, [data], chunk)
    assert int(b.nbits[0]) <= mhc.BATCH_WALK_MAX_BITS
    check_all_ways(mhc, b, "wiki as one stream, chunk %d" % chunk)


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("order", [0, 1])
def test_lengths_around_chunk_edges(mhc, order, chunk):
    """The combine's exponents on both sides of a chunk edge: streams that end just before, at and just behind one."""
    data = zipf(5 * 1024 + 1, 31)
    lengths = [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5 * chunk]
    msgs = [data[7 * k:7 * k + n] for k, n in enumerate(lengths)]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs + [data], order=order), order)   # (every stream's first pair has a code)
    check_all_ways(mhc, Packed(mhc, msgs, chunk, order, model=model), "edge lengths")
    for m in msgs:                                                         # and every one alone, as stream 0 of its batch
        check_all_ways(mhc, Packed(mhc, [m], chunk, order, model=model), "length %d alone" % len(m))


def test_empty_streams(mhc):
    data = zipf(4000, 32)
    msgs = [b"", b"", data[:700], b"", data[700:1000], b"", b"", data[1000:], b"", b""]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=1), 1)
    b = Packed(mhc, msgs, 256, model=model)
    assert b.want[0][0] == 0 and zlib.crc32(b"") == 0                      # an empty stream gives 0
    check_all_ways(mhc, b, "empty streams at the start, in the middle, at the end")
    check_all_ways(mhc, Packed(mhc, [b"", b"", b""], 256, model=model), "empty streams only")
    none = Packed(mhc, [], 256, model=model)
    check_all_ways(mhc, none, "n_streams == 0")
    assert none.crc(True)[0].size == 0 and none.host(False)[0].size == 0


def test_large_batch_of_small_streams(mhc):
    """65 536 x 256 B: a wave holds 64 different streams."""
    data = zipf(65536 * 256, 4)
    msgs = [data[i * 256:(i + 1) * 256] for i in range(65536)]
    b = Packed(mhc, msgs, 256)
    assert len(set(b.want[0].tolist())) > 65000
    check(mhc, b.crc(True), b.want, "65536 x 256 B indexed")
    check(mhc, b.crc(False), b.want, "65536 x 256 B index-free")
    crc, rc = mhc.crc_raw_batch(msgs)
    assert rc == mhc.MH_OK and np.array_equal(crc, b.want[0])


def test_waves_that_straddle_stream_boundaries(mhc):
    """Streams of random length 300 .. 3 000 at chunk 256: two to twelve chunks each, so the runs of equal streams inside a
    wave start and end at every lane."""
    rng = np.random.default_rng(33)
    lengths = rng.integers(300, 3001, 1200)
    data = zipf(int(lengths.sum()), 34)
    off = np.concatenate([[0], np.cumsum(lengths)])
    msgs = [data[off[i]:off[i + 1]] for i in range(len(lengths))]
    b = Packed(mhc, msgs, 256)
    check_all_ways(mhc, b, "random lengths")
    crc, rc = mhc.crc_raw_batch(msgs)
    assert rc == mhc.MH_OK and np.array_equal(crc, b.want[0])


def test_large_zipf_stream(mhc):
    """One 8 MiB stream: all lanes of every wave share one stream, 8 192 chunks meet in one word."""
    data = zipf(8 << 20, 3)
    b = Packed(mhc, [data], 1024)
    check(mhc, b.crc(True), b.want, "8 MiB indexed")
    # index-free the stream is over the walk cap: refused by the device call, indexed and digested by the host form
    assert int(b.nbits[0]) > mhc.BATCH_WALK_MAX_BITS
    crc, ln, st, rc = b.crc(False)
    assert st.tolist() == [mhc.MH_ERR_ARG] and rc == mhc.MH_ERR_ARG and crc.tolist() == [0] and ln.tolist() == [0]
    check(mhc, b.host(False), b.want, "8 MiB host form, index-free")
    check(mhc, b.host(True), b.want, "8 MiB host form, indexed")
    crc, rc = mhc.crc_raw_batch([data])
    assert rc == mhc.MH_OK and np.array_equal(crc, b.want[0])


def test_per_stream_models_and_a_picked_bank(mhc, wiki_lines):
    msgs = wiki_lines[:400]
    want = digests(msgs)
    ms = mhc.ModelSet.train(msgs, order=1)
    payload, out_off, nbits, idx, in_off, rc = ms.encode(msgs, chunk_symbols=256)
    assert rc == mhc.MH_OK
    check(mhc, ms.crc(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=256), want, "each indexed")
    check(mhc, ms.crc(payload, out_off, nbits), want, "each index-free")
    bank, choice, _ = mhc.ModelSet.train_bank(msgs, 4, order=1)
    payload, out_off, nbits, idx, in_off = mhc.encode_bank(bank, msgs, choice, chunk_symbols=1024)
    view = bank.pick(choice)
    check(mhc, view.crc(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024), want, "bank indexed")
    check(mhc, view.crc(payload, out_off, nbits), want, "bank index-free")
    wrong = mhc.ModelSet.train(msgs[:10], order=1)
    with pytest.raises(mhc.MhError) as e:                       # n_streams != the set's size
        wrong.crc(payload, out_off, nbits)
    assert e.value.status == mhc.MH_ERR_ARG


@pytest.mark.parametrize("chunk", [256, 1024])
def test_shared_order2_model(mhc, wiki_lines, wiki_want, chunk):
    b = Packed(mhc, wiki_lines, chunk, order=2)
    assert np.array_equal(b.want[0], wiki_want[0])
    check_all_ways(mhc, b, "order 2 chunk %d" % chunk)


def test_each_call_refuses_the_other_family_s_model(mhc):
    data = zipf(50000, 9)
    m2 = mhc.Model.from_counts(mhc.histogram_o2(data), 2)
    b = Packed(mhc, [data[:3000], data[3000:9000]], 256)
    for indexed in (True, False):
        for fn in (m2.dev_crc_batch, m2.crc_batch, b.model.dev_crc_batch_o2, b.model.crc_batch_o2):
            with pytest.raises(mhc.MhError) as e:
                fn(b.payload, b.pay_off, b.nbits, **b.kw(indexed))
            assert e.value.status == mhc.MH_ERR_ARG


# ---- uncompressed batches -------------------------------------------------------------------------------------------------------

def test_raw_batches(mhc, wiki_lines, wiki_want):
    for shift in (0, 1, 3, 7):                                             # d_data at an odd address
        crc, rc = mhc.crc_raw_batch(wiki_lines, shift=shift)
        assert rc == mhc.MH_OK and np.array_equal(crc, wiki_want[0]), shift
    coded = Packed(mhc, wiki_lines, 1024).crc(True)[0]
    assert np.array_equal(mhc.crc_raw_batch(wiki_lines)[0], coded)         # crc(raw) == crc(coded) for every stream
    data = zipf(5 * 1024 + 1, 31)
    msgs = [b"", data[:1], data[:1023], b"", data[:1024], data[:1025], data[:2047], data[:2048], data[:2049], data, b""]
    crc, rc = mhc.crc_raw_batch(msgs, shift=5)
    assert rc == mhc.MH_OK and np.array_equal(crc, digests(msgs)[0])
    whole = golden()["input_wiki_cpp.html"]["data"]
    crc, rc = mhc.crc_raw_batch([whole], shift=1)
    assert rc == mhc.MH_OK and crc.tolist() == [zlib.crc32(whole)]
    for msgs in ([], [b"", b""]):
        crc, rc = mhc.crc_raw_batch(msgs)
        assert rc == mhc.MH_OK and crc.tolist() == [0] * len(msgs)


def test_raw_bad_offsets(mhc):
    l = mhc.lib()
    data = np.frombuffer(zipf(3000, 1), dtype=np.uint8)
    D = mhc.DeviceBuffer
    d_data = D(data.size, data)
    wsb = l.mh_dev_crc_raw_batch_workspace(2, data.size)
    for off in ([1, 1000, 3000], [0, 2000, 1000], [0, 1000, 2999]):
        d_off, d_crc, d_ws = D(24, np.array(off, dtype=np.uint64)), D(8, np.full(2, 0x77777777, dtype=np.uint32)), D(wsb)
        assert l.mh_dev_crc_raw_batch(d_data.ptr, d_off.ptr, 2, data.size, d_crc.ptr, d_ws.ptr, wsb, None) == mhc.MH_OK
        assert l.mh_dev_status(d_ws.ptr, None) == mhc.MH_ERR_ARG, off
        assert d_crc.download(np.uint32).tolist() == [0, 0], off


# ---- damaged batches ----------------------------------------------------------------------------------------------------------

SILENT_FLIPS = {0: (0, 1, 2, 3, 4), 1: (5, 9, 10, 15, 27)}
# Payload bit 9 of the order-1 stream is the whole code of `o` behind `L`, a context with that one symbol: the strict oracle
# (and every decoder) reads either bit value as `o`, so this accepted flip alone decodes to the original bytes.
SAME_BYTES = {(1, 9)}


@pytest.mark.parametrize("order", [0, 1])
def test_silent_damage_changes_the_crc(mhc, order):
    """Single-bit flips that every decoder accepts: the stream re-synchronises and ends at nbits, the verdict is MH_OK and the
    bytes are wrong.  One damaged copy per flip beside intact copies; the verdicts are recomputed with the strict CPU oracle
    (damage.verdict_indexed / verdict_free), so the input cannot drift."""
    chunk = 256
    data = golden()["input_ipsum.txt"]["data"][:8192]
    om = mh_oracle.Model.from_data(data, order)
    blob, nbits = om.compress(data)
    lens = np.asarray(om.codes()[0])
    index, _ = damage.expected_entries(lens, np.frombuffer(data, dtype=np.uint8), chunk, 0x20, order)
    flips = SILENT_FLIPS[order]
    n = 2 * len(flips) + 1
    b = Packed(mhc, [data] * n, chunk, order, model=mhc.Model.from_table(om.table_bytes()))
    assert bytes(b.payload[:int(b.pay_off[1])]) == blob[1:] and int(b.nbits[0]) == nbits
    payload = b.payload.copy()
    want_crc = b.want[0].copy()
    original = zlib.crc32(data)
    for k, f in enumerate(flips):
        i = 2 * k + 1                                                      # damaged copies at the odd places
        pl = damage.flip(blob[1:], f)
        payload[int(b.pay_off[i]) + (f >> 3)] ^= 0x80 >> (f & 7)
        free, indexed = damage.verdict_free(om, pl, nbits), damage.verdict_indexed(om, pl, nbits, index, chunk, len(data), order)
        assert free[0] == damage.MH_OK and indexed[0] == damage.MH_OK and free[1] == indexed[1] and len(free[1]) == len(data), (order, f)
        assert (free[1] == data) == ((order, f) in SAME_BYTES), (order, f)
        want_crc[i] = zlib.crc32(free[1])
        assert (want_crc[i] == original) == ((order, f) in SAME_BYTES), (order, f)
    assert sum(1 for f in flips if (order, f) not in SAME_BYTES) >= 4
    want = (want_crc, b.want[1])
    for indexed in (True, False):
        got = b.model.dev_crc_batch(payload, b.pay_off, b.nbits, **b.kw(indexed))
        check(mhc, got, want, "silent damage, device, indexed=%s" % indexed)       # every status MH_OK, the intact copies keep their CRC
        assert (got[0][0::2] == original).all()
        check(mhc, b.model.crc_batch(payload, b.pay_off, b.nbits, **b.kw(indexed)), want, "silent damage, host, indexed=%s" % indexed)
    ms = mhc.ModelSet.from_tables([om.table_bytes()] * n)                 # the same under per-stream models
    check(mhc, ms.crc(payload, b.pay_off, b.nbits, **b.kw(True)), want, "silent damage, each")


def dev_decode_statuses(mhc, model, payload, pay_off, nbits, sym_off=None, index=None, chunk_symbols=0):
    """Per-stream statuses and the status word of one mh_dev_decode_batch call on these arguments."""
    l = mhc.lib()
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    D = mhc.DeviceBuffer
    d_pl = D(max(payload.size, 1) + 64, payload if payload.size else None)
    d_po, d_nb = D(pay_off.nbytes, pay_off), D(max(nbits.nbytes, 8), nbits)
    if index is not None:
        so = np.ascontiguousarray(sym_off, dtype=np.uint64)
        cap, total = int(so[n]), int(so[n])
        d_idx = D(max(index.nbytes, 8), np.ascontiguousarray(index, dtype=np.uint64))
    else:
        so = np.zeros(n + 1, dtype=np.uint64)
        cap, total, d_idx = int(sum(int(x) for x in nbits)), 0, None
    d_so, d_out, d_st = D(so.nbytes, so), D(max(cap, 1) + 64), D(max(n, 1) * 4)
    wsb = l.mh_dev_decode_batch_workspace(n)
    d_ws = D(wsb)
    rc = l.mh_dev_decode_batch(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), 0x20, d_out.ptr, cap, d_so.ptr, total,
                               d_idx.ptr if d_idx else None, chunk_symbols, d_st.ptr, d_ws.ptr, wsb, None)
    assert rc == mhc.MH_OK
    return d_st.download(np.int32)[:n], l.mh_dev_status(d_ws.ptr, None)


@pytest.mark.parametrize("indexed", [True, False])
def test_detected_damage_gets_the_decoder_s_verdict(mhc, indexed):
    chunk = 256
    msgs = [zipf(k, 40 + k) for k in (30_000, 5_000, 60_000, 700, 45_000)]
    counts = batch_ref.histogram(msgs, 1)
    b = Packed(mhc, msgs, chunk, model=mhc.Model.from_counts(counts, 1))
    lens = batch_ref.oracle_codes(counts, 1)[0]
    streams = [bytes(b.payload[int(b.pay_off[i]):int(b.pay_off[i + 1])]) for i in range(5)]
    failed = 0
    for at in (0, 2, 4):
        pl, nb = streams[at], int(b.nbits[at])
        bounds = damage.boundaries(lens, np.frombuffer(msgs[at], dtype=np.uint8))
        assert int(bounds[-1]) == nb
        long = int(np.flatnonzero(np.diff(bounds) >= 2)[-1])               # the last code of at least two bits: a cut inside it
        inside = int(bounds[long]) + 1
        base = int(mhc.lib().mh_batch_index_base(int(b.sym_off[at]), at, chunk))
        cases = [("cut inside a code", damage.cut(pl, nb, inside), inside, None), ("cut-1", damage.cut(pl, nb, nb - 1), nb - 1, None),
                 ("ext1+13", damage.with_length(pl, nb, nb + 13, 1), nb + 13, None)]
        if indexed:
            cases += [("entry+1", pl, nb, (base + 3, 1)), ("entry-1", pl, nb, (base + 7, -1))]
        for name, dpl, dnb, move in cases:
            pls, nbs = list(streams), [int(x) for x in b.nbits]
            pls[at], nbs[at] = dpl, dnb
            payload, pay_off = mhc.batch_offsets(pls)
            kw = b.kw(indexed)
            if move:
                kw["index"] = b.index.copy()
                kw["index"][move[0]] = np.uint64(int(kw["index"][move[0]]) + move[1])
            want_st, want_rc = dev_decode_statuses(mhc, b.model, payload, pay_off, nbs, **kw)
            crc, ln, st, rc = b.model.dev_crc_batch(payload, pay_off, nbs, **kw)
            what = "stream %d %s indexed=%s" % (at, name, indexed)
            assert st.tolist() == want_st.tolist(), what
            assert (rc == mhc.MH_OK) == (want_rc == mhc.MH_OK), what
            assert name not in ("cut inside a code", "entry+1", "entry-1") or st[at] == mhc.MH_ERR_CORRUPT, what
            for k in range(5):
                if k != at:                                                # the neighbours are exact
                    assert st[k] == mhc.MH_OK and crc[k] == b.want[0][k] and ln[k] == b.want[1][k], what
            if st[at] != mhc.MH_OK:
                failed += 1
                assert crc[at] == 0 and ln[at] == 0, what
            hcrc, hln, hst, hrc = b.model.crc_batch(payload, pay_off, nbs, check=False, **kw)
            assert hst.tolist() == st.tolist() and np.array_equal(hcrc, crc) and np.array_equal(hln, ln), what
            assert hrc == (mhc.MH_OK if st[at] == mhc.MH_OK else int(st[at])), what
    assert failed >= (12 if indexed else 6)
    # nbits beyond the stream's payload bytes: MH_ERR_ARG for that stream alone, as the decoder says
    nbs = [int(x) for x in b.nbits]
    nbs[1] = (int(b.pay_off[2]) - int(b.pay_off[1])) * 8 + 1
    want_st, _ = dev_decode_statuses(mhc, b.model, b.payload, b.pay_off, nbs, **b.kw(indexed))
    crc, ln, st, rc = b.model.dev_crc_batch(b.payload, b.pay_off, nbs, **b.kw(indexed))
    assert st.tolist() == want_st.tolist() and st[1] == mhc.MH_ERR_ARG and rc == mhc.MH_ERR_ARG
    keep = np.arange(5) != 1
    assert crc[1] == 0 and ln[1] == 0 and np.array_equal(crc[keep], b.want[0][keep]) and np.array_equal(ln[keep], b.want[1][keep])


def test_bad_offsets_stop_the_call(mhc):
    b = Packed(mhc, [zipf(3000, 1), zipf(2000, 2)], 256)
    po = b.pay_off.copy()
    po[1] = po[2] + np.uint64(1)                                               # decreasing
    crc, ln, st, rc = b.model.dev_crc_batch(b.payload, po, b.nbits, **b.kw(True))
    assert rc == mhc.MH_ERR_ARG and crc.tolist() == [0, 0] and ln.tolist() == [0, 0]


# ---- what a call clears -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(mhc, wiki_lines):
    """Empty, short and long streams, one with a detected damage: every kind of entry the outputs can hold."""
    msgs = [b""] + wiki_lines[100:180] + [b"", zipf(20000, 5)] + wiki_lines[300:340] + [b""]
    b = Packed(mhc, msgs, 256)
    nbits = b.nbits.copy()
    nbits[7] -= np.uint64(1)
    return b, nbits


def mixed_run(mhc, mixed, indexed):
    b, nbits = mixed
    got = b.model.dev_crc_batch(b.payload, b.pay_off, nbits, **b.kw(indexed))
    raw = mhc.crc_raw_batch(b.msgs, shift=1)
    return got, raw


def same_results(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x[0][:3], y[0][:3])) and x[0][3] == y[0][3] and x[1][0].tobytes() == y[1][0].tobytes()


@pytest.mark.parametrize("indexed", [True, False])
def test_dirty_and_recycled_memory_and_two_calls(mhc, mixed, indexed):
    b, nbits = mixed
    fresh = mixed_run(mhc, mixed, indexed)
    (crc, ln, st, rc), (raw, raw_rc) = fresh
    keep = np.arange(len(b.msgs)) != 7
    assert st[7] == mhc.MH_ERR_CORRUPT and crc[7] == 0 and ln[7] == 0 and not st[keep].any() and rc == mhc.MH_ERR_CORRUPT
    assert np.array_equal(crc[keep], b.want[0][keep]) and np.array_equal(ln[keep], b.want[1][keep])
    assert raw_rc == mhc.MH_OK and np.array_equal(raw, b.want[0])
    assert same_results(mixed_run(mhc, mixed, indexed), fresh), "two calls give identical buffers"
    for byte in (0xFF, 0xA5):
        with mhc.device_memory("fill", byte):
            assert same_results(mixed_run(mhc, mixed, indexed), fresh), "on memory filled with 0x%02X" % byte
    other = Packed(mhc, [zipf(n, 50 + n) for n in (5000, 0, 12000, 300) * 31], 256)     # another batch with as many streams
    assert len(other.msgs) == len(b.msgs)
    gc.collect()
    with mhc.device_memory("recycle") as mem:
        first = mixed_run(mhc, mixed, indexed)
        check(mhc, other.crc(indexed), other.want, "the other batch")
        assert np.array_equal(mhc.crc_raw_batch(other.msgs, shift=1)[0], other.want[0])
        gc.collect()
        served, missed = mem.served, mem.missed
        again = mixed_run(mhc, mixed, indexed)
        served, missed = mem.served - served, mem.missed - missed
    assert same_results(first, fresh) and same_results(again, fresh), "on buffers recycled from another batch"
    assert missed == 0 and served > 0, "the third run got fresh memory for %d of its %d requests without init" % (missed, missed + served)


def test_encode_then_crc_on_one_stream_without_a_host_wait(mhc, wiki_lines):
    """mh_dev_encode_batch -> mh_dev_crc_batch (indexed and index-free) and mh_dev_crc_raw_batch on one non-default stream,
    enqueued back to back behind a blocker, on buffers prefilled with 0xA5: every call reads what an earlier one wrote on the
    device, and none of them may wait for the stream (the blocker's event is still unfinished after the last call returns)."""
    import torch
    lib = mhc.lib()
    msgs = wiki_lines[:300] + [b"", zipf(30000, 6)]
    data, in_off = mhc.batch_offsets(msgs)
    want = digests(msgs)
    n, total, chunk = len(msgs), int(data.size), 256
    counts = batch_ref.histogram(msgs, 1)
    model = mhc.Model.from_counts(counts, 1)
    pay_total = int(batch_ref.pack(msgs, *batch_ref.oracle_codes(counts, 1), 1, 0x20).pay_off[n])   # a host value, not read from the device
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    assert sp.value, "a non-default stream has a handle"
    ptr = lambda t: C.c_void_p(t.data_ptr())
    buf = lambda nbytes: torch.full((max(int(nbytes), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    cap = lib.mh_encode_batch_bound(model.handle, total, n)
    nidx = int(lib.mh_batch_index_capacity(total, n, chunk))
    ews, cws, rws = lib.mh_dev_encode_batch_workspace(n, total), lib.mh_dev_crc_batch_workspace(n, total, chunk), lib.mh_dev_crc_raw_batch_workspace(n, total)
    d_data, d_in = buf(total + 16), torch.zeros((n + 1) * 8, dtype=torch.uint8, device="cuda")
    d_pl, d_po, d_nb, d_idx, d_ews = buf(cap + 64), buf((n + 1) * 8), buf(n * 8), buf(nidx * 8), buf(ews)
    outs = [(buf(n * 4), buf(n * 8), buf(n * 4), buf(cws)) for _ in range(2)]
    d_raw, d_rws = buf(n * 4), buf(rws)
    h_data, h_in = torch.from_numpy(data.copy()).pin_memory(), torch.from_numpy(in_off.view(np.uint8).copy()).pin_memory()
    with torch.cuda.stream(stream):                                        # cycles per millisecond of _sleep
        torch.cuda._sleep(1_000_000)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20_000_000)
        e.record()
    e.synchronize()
    cycles_per_ms = 20_000_000 / a.elapsed_time(e)
    torch.cuda.synchronize()
    rcs = []
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(100 * cycles_per_ms))
        ev = torch.cuda.Event()
        ev.record()
        d_data[:total].copy_(h_data, non_blocking=True)
        d_in.copy_(h_in, non_blocking=True)
        rcs.append(lib.mh_dev_encode_batch(model.handle, ptr(d_data), ptr(d_in), n, total, 0x20, ptr(d_pl), cap, ptr(d_po), ptr(d_nb), ptr(d_idx), chunk,
                                           ptr(d_ews), ews, sp))
        for indexed, (d_crc, d_len, d_st, d_ws) in zip((True, False), outs):
            rcs.append(lib.mh_dev_crc_batch(model.handle, ptr(d_pl), ptr(d_po), ptr(d_nb), n, pay_total, 0x20, ptr(d_in) if indexed else None,
                                            total if indexed else 0, ptr(d_idx) if indexed else None, chunk if indexed else 0, ptr(d_crc), ptr(d_len),
                                            ptr(d_st), ptr(d_ws), cws, sp))
        rcs.append(lib.mh_dev_crc_raw_batch(ptr(d_data), ptr(d_in), n, total, ptr(d_raw), ptr(d_rws), rws, sp))
        waited = ev.query()
    stream.synchronize()
    assert not waited, "a call waited for the stream: the blocker had finished when the last call returned"
    assert rcs == [0, 0, 0, 0]
    get = lambda t, dtype, count: t.cpu().numpy().view(dtype)[:count]
    assert lib.mh_dev_status(ptr(d_ews), sp) == 0 and lib.mh_dev_status(ptr(d_rws), sp) == 0
    for indexed, (d_crc, d_len, d_st, d_ws) in zip((True, False), outs):
        assert lib.mh_dev_status(ptr(d_ws), sp) == 0 and not get(d_st, np.int32, n).any(), indexed
        assert np.array_equal(get(d_crc, np.uint32, n), want[0]) and np.array_equal(get(d_len, np.uint64, n), want[1]), indexed
    assert np.array_equal(get(d_raw, np.uint32, n), want[0])


# ---- seeded fuzz ----------------------------------------------------------------------------------------------------------------

CASES = batch_ref.draw_cases()[::3]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fuzz_case(mhc, case):
    """Every third case of the batch fuzz (tests/batch_ref.py): the reference's payloads and index under the case's source
    model (order 0, 1 or 2; own, limited or deep), and, where sets apply, under one model per stream."""
    w = case.world()
    order, c, p0, msgs = case.orders[0], case.chunk, w.prev0, w.messages
    want = digests(msgs)
    counts, limit = case.counts("src")
    S = mhc.Model.from_counts(counts, order, max_len=limit)
    rs = batch_ref.pack(msgs, *case.codes("src"), order, p0, c)
    assert not rs.dropped.any()
    dev, host = (S.dev_crc_batch_o2, S.crc_batch_o2) if order == 2 else (S.dev_crc_batch, S.crc_batch)
    for indexed in (True, False):
        kw = dict(prev0=p0, sym_off=rs.sym_off, index=rs.index_array(c), chunk_symbols=c) if indexed else dict(prev0=p0)
        check(mhc, dev(rs.payload, rs.pay_off, rs.nbits, **kw), want, "%s device indexed=%s" % (case.id, indexed))
        if case.index % 2 == 0:
            check(mhc, host(rs.payload, rs.pay_off, rs.nbits, **kw), want, "%s host indexed=%s" % (case.id, indexed))
    crc, rc = mhc.crc_raw_batch(msgs, shift=case.index % 4)
    assert rc == mhc.MH_OK and np.array_equal(crc, want[0])
    if order < 2 and case.n_streams <= 65:
        re, tables = batch_ref.pack_each(msgs, order, p0, c)
        ms = mhc.ModelSet.from_tables(tables)
        for indexed in (True, False):
            kw = dict(prev0=p0, sym_off=re.sym_off, index=re.index_array(c), chunk_symbols=c) if indexed else dict(prev0=p0)
            check(mhc, ms.crc(re.payload, re.pay_off, re.nbits, **kw), want, "%s each indexed=%s" % (case.id, indexed))


def test_the_fuzz_subset_keeps_its_coverage():
    assert 24 <= len(CASES) <= 48
    assert {c.orders[0] for c in CASES} == {0, 1, 2}
    assert {"own", "limited", "deep"} <= {c.src_kind for c in CASES}
    assert sum(1 for c in CASES if c.orders[0] < 2 and c.n_streams <= 65) >= 8
    assert {256, 8192} <= {c.chunk for c in CASES}


def test_the_fuzz_reaches_both_places_of_the_byte_table(mhc):
    """The 1 KiB byte table lies in LDS behind a shared model's decode tables when they leave room, else it is read from the
    workspace (csrc/mh_crc.hip, TLDS): the subset has a deep model on either side of that threshold."""
    where = {}
    for c in CASES:
        if c.orders[0] == 2 or c.src_kind != "deep":
            continue
        counts, limit = c.counts("src")
        primary, nsec, in_lds = mhc.Model.from_counts(counts, c.orders[0], max_len=limit).decode_layout()
        tables = 1024 + (256 << primary) * 2 + (((nsec * 2 + 15) & ~15) if in_lds else 0)
        where.setdefault(tables + 1024 <= 160 << 10, []).append((c.id, tables))
    assert where.get(False) and where.get(True), where
    assert max(t for _, t in where[True]) > (160 << 10) - 4096            # one just under the threshold as well


# ---- CLI ----------------------------------------------------------------------------------------------------------------------

def run_cli(args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300)


@pytest.mark.parametrize("name", ["input_wiki_cpp.html", "input_ipsum.txt", "input_a.txt", "empty"])
def test_cli_crc_of_the_golden_files(mhc, tmp_path, name):
    """The `.cm` / `.e` and `.ch` / `.eh` pairs the reference wrote (tests/golden/expected): index-free, no output file."""
    data = golden()[name]["data"]
    line = ("%08x %d\n" % (zlib.crc32(data), len(data))).encode()
    exp = os.path.join(ROOT, "tests", "golden", "expected", name)
    out = tmp_path / "out"
    r = run_cli([exp + ".cm", "-x", "-e", exp + ".e", "--crc", "-o", out])
    assert r.returncode == 0 and r.stdout == line, r.stderr
    assert not out.exists()
    if name != "empty":                                                    # (the empty input's `.eh` is an empty file: no table to load)
        r = run_cli([exp + ".ch", "-x", "-h", "-e", exp + ".eh", "--crc"])
        assert r.returncode == 0 and r.stdout == line, r.stderr


@pytest.mark.parametrize("name", ["input_wiki_cpp.html", "input_ipsum.txt"])
def test_cli_crc_with_an_index(mhc, tmp_path, name):
    src = os.path.join(ROOT, "tests", "golden", "inputs", name)
    data = golden()[name]["data"]
    line = ("%08x %d\n" % (zlib.crc32(data), len(data))).encode()
    cm, table, idx, out = (tmp_path / n for n in ("in.cm", "table", "f.idx", "out"))
    r = run_cli([src, "-o", cm, "-d", table, "--index", idx, "--chunk", "256"])
    assert r.returncode == 0, r.stderr
    assert cm.read_bytes() == open(os.path.join(ROOT, "tests", "golden", "expected", name + ".cm"), "rb").read()
    r = run_cli([cm, "-x", "-e", table, "--crc", "--index", idx, "-o", out])
    assert r.returncode == 0 and r.stdout == line, r.stderr
    assert not out.exists()
    r = run_cli([cm, "-x", "-e", table, "--crc", "--index", tmp_path / "missing.idx"])    # no usable sidecar: the index-free path
    assert r.returncode == 0 and r.stdout == line, r.stderr
