"""Masked re-coding on the GPU (include/mh.h, "EDITING BATCHES"): a batch coded again with map[b] in place of every byte b
inside given spans, the bytes never written, and the spans merged from search records on the device.  The reference is
tests/edit_ref.py on top of tests/recode_ref.py (the CPU oracle's encoder on the edited messages); every comparison is exact.
The device-call wrappers put guards around every output and assert that nothing outside the results changed.

chunk_symbols is 256 (MH_CHUNK_MIN) and the batch ragged, with messages of 0, 1, 2, 255, 256, 257, 3 * 256 + 5 and about 1100
bytes: the smallest shapes at which a chunk seam, an empty stream and the last partial dword all occur."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
import edit_ref
import find_ref
import recode_ref
from conftest import ROOT, expected_file, golden
from oracle import mh_oracle
from test_gpu_stream_order import Batch, Chain, drive, env, ptr, same  # noqa: F401  (env: the fixture of the stream chains)

pytestmark = pytest.mark.gpu

CHUNK = 256
LENGTHS = [0, 1, 2, 255, 256, 257, 3 * 256 + 5]
STAR = edit_ref.mask_map(0x2A)
FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def msgs():
    """Pieces of input_wiki_cpp.txt of the lengths above, then whole lines of it up to about 1100 bytes."""
    text = golden()["input_wiki_cpp.txt"]["data"]
    out, at = [], 4000
    for k in LENGTHS:
        out.append(text[at:at + k])
        at += k + 37
    lines, size = [], 0
    for l in text.split(b"\n")[40:]:
        if size + len(l) + 1 <= 1100:                                           # (a line that does not fit is left out)
            lines.append(l)
            size += len(l) + 1
    out.append(b"\n".join(lines))
    assert [len(m) for m in out[:-1]] == LENGTHS and 1000 <= len(out[-1]) <= 1100
    return out


def model_of(mhc, messages, order):
    return mhc.Model.from_counts(mhc.histogram_o1_batch([bytes(m) for m in messages], order=order), order)


class Source:
    """A batch coded under one shared model, or (each) one model per stream, with an index of CHUNK."""

    def __init__(self, mhc, msgs, order=1, each=False, model=None, chunk=CHUNK):
        self.mhc, self.msgs, self.each, self.chunk = mhc, [bytes(m) for m in msgs], each, chunk
        if each:
            self.model = mhc.ModelSet.train(self.msgs, order=order)
            self.payload, self.pay_off, self.nbits, self.index, self.sym_off, rc = self.model.encode(self.msgs, chunk_symbols=chunk)
            assert rc == mhc.MH_OK
        else:
            self.model = model or model_of(mhc, self.msgs, order)
            self.payload, self.pay_off, self.nbits, self.index, self.sym_off = self.model.encode_batch(self.msgs, chunk_symbols=chunk)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else dict(chunk_symbols=self.chunk)

    def batch(self, payload=None, pay_off=None, nbits=None):
        return (self.payload if payload is None else payload, self.pay_off if pay_off is None else pay_off, self.nbits if nbits is None else nbits)

    def edit(self, dst, byte_map, span_off, spans, indexed, payload=None, pay_off=None, nbits=None, index=None, **kw):
        fn = self.model.recode_edit if self.each else self.model.dev_recode_edit_batch
        k = self.kw(indexed)
        if index is not None:
            k["index"] = index
        return fn(dst, *self.batch(payload, pay_off, nbits), byte_map, span_off, spans, **k, **kw)

    def recode(self, dst, indexed, payload=None, pay_off=None, nbits=None, index=None, **kw):
        fn = self.model.recode if self.each else self.model.dev_recode_batch
        k = self.kw(indexed)
        if index is not None:
            k["index"] = index
        return fn(dst, *self.batch(payload, pay_off, nbits), **k, **kw)


def span_lists(per_stream):
    """(span_off, spans[m, 2]) of per-stream lists of (begin, end)."""
    off = np.zeros(len(per_stream) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in per_stream], dtype=np.uint64)
    return off, np.array([p for s in per_stream for p in s], dtype=np.uint64).reshape(-1, 2)


def slices_of(idx, sym_off, chunk, only=None):
    out = []
    for i in range(len(sym_off) - 1):
        if only is None or i in only:
            b = int(sym_off[i]) // chunk + i
            out.append(np.asarray(idx[b:b + (int(sym_off[i + 1] - sym_off[i]) + chunk - 1) // chunk], dtype=np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


_ORACLES = {}


def oracle_of(dst):
    t = dst.table_bytes()
    if t not in _ORACLES:
        _ORACLES[t] = mh_oracle.Model.from_table(t)
    return _ORACLES[t]


def expect(src, dst, byte_map, span_off, spans):
    """What the edit must give: the oracle's encode, under dst, of the edited messages."""
    edited = edit_ref.apply(src.msgs, span_off, spans, byte_map)
    ref = recode_ref.recode(edited, oracle_of(dst), src.chunk)
    return edited, ref, recode_ref.packed(ref)


def check_exact(mhc, src, got, ref, packed, what, payload=True, index=True):
    r_pay, r_off, r_nb, r_drop = packed
    n = len(src.msgs)
    assert got["rc"] == mhc.MH_OK and (got["status"] == mhc.MH_OK).all(), (what, got["rc"], got["status"])
    assert np.array_equal(got["out_off"], r_off) and np.array_equal(got["nbits"], r_nb), what
    assert np.array_equal(got["dropped"], r_drop), (what, got["dropped"], r_drop)
    assert np.array_equal(got["sym_off"], src.sym_off), what
    if payload:
        assert np.array_equal(got["payload"], r_pay), what
    else:
        assert got["payload"] is None, what
    if index:
        want = np.concatenate([r[3] for r in ref]) if n else np.zeros(0, dtype=np.uint64)
        assert np.array_equal(slices_of(got["index"], src.sym_off, src.chunk), want), what
    else:
        assert got["index"] is None, what


def scattered_spans(msgs, seed):
    """A valid random span list per message: ascending, disjoint, some touching, some past the end."""
    rng = np.random.default_rng(seed)
    per = []
    for m in msgs:
        at, lst = 0, []
        for _ in range(int(rng.integers(0, 6))):
            b = at + int(rng.integers(0, max(len(m) // 3, 2)))
            e = b + 1 + int(rng.integers(0, 300 if rng.random() < 0.3 else 9))
            lst.append((b, e))
            at = e
        per.append(lst)
    return span_lists(per)


# ---- 1. every order pair, model kind, indexed or not, with and without the index, count only -----------------------------------

@pytest.fixture(scope="module")
def sources(mhc, msgs):
    return {(so, each): Source(mhc, msgs, order=so, each=each) for so in (0, 1) for each in (False, True)}


@pytest.fixture(scope="module")
def dsts(mhc, msgs):
    text = golden()["input_wiki_cpp.txt"]["data"]
    return {do: model_of(mhc, [text, b"*" * 40 + b" * "], do) for do in (0, 1)}


@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("so,do", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_every_order_pair_and_model_kind(mhc, sources, dsts, so, do, each, indexed):
    src, dst = sources[(so, each)], dsts[do]
    span_off, spans = scattered_spans(src.msgs, 11)
    assert len(spans) >= 8
    _, ref, packed = expect(src, dst, STAR, span_off, spans)
    what = "%d->%d each=%s indexed=%s" % (so, do, each, indexed)
    check_exact(mhc, src, src.edit(dst, STAR, span_off, spans, indexed), ref, packed, what)
    check_exact(mhc, src, src.edit(dst, STAR, span_off, spans, indexed, want_index=False), ref, packed, what + " no index", index=False)
    check_exact(mhc, src, src.edit(dst, STAR, span_off, spans, indexed, count_only=True, sym_total=None if indexed else int(src.sym_off[-1])),
                ref, packed, what + " count only", payload=False)
    assert do == 0 or packed[3].sum() > 0                                       # order 1: some (prev, '*') pairs have no code under dst


# ---- 2. spans where the lane logic can break ----------------------------------------------------------------------------------

def placements(msgs):
    """name -> per-stream span lists; stream 6 has 773 bytes (chunks at 256, 512, 768), stream 7 about 1100."""
    n, big, last = len(msgs), 6, 7
    L = len(msgs[last])

    def only(i, lst):
        return [lst if k == i else [] for k in range(n)]
    return {
        "first byte": only(big, [(0, 1)]),
        "last byte": only(big, [(772, 773)]),
        "ends at a chunk boundary": only(big, [(250, 256)]),
        "begins at a chunk boundary": only(big, [(512, 520)]),
        "only the byte in front of a chunk": only(big, [(255, 256)]),
        "in front of two chunks": only(big, [(255, 256), (511, 512), (767, 768)]),
        "three whole chunks": only(big, [(0, 768)]),
        "two spans in one chunk": only(big, [(300, 310), (310, 311), (400, 440)]),
        "beyond the length": only(big, [(770, 5000), (6000, 7000)]),
        "wholly beyond the length": only(big, [(773, 900)]),
        "on an empty stream": [[(0, 4), (9, 12)]] + [[] for _ in range(n - 1)],
        "short streams": [[], [(0, 1)], [(1, 2)], [(254, 255)], [(255, 256)], [(255, 257)], [], []],
        "across every seam of the last stream": only(last, [(k - 2, k + 2) for k in range(256, L, 256)] + [(L - 1, L + 1)]),
        "everything, as a list": [[(0, max(len(m), 1))] for m in msgs],
    }


@pytest.mark.parametrize("name", ["first byte", "last byte", "ends at a chunk boundary", "begins at a chunk boundary",
                                  "only the byte in front of a chunk", "in front of two chunks", "three whole chunks", "two spans in one chunk",
                                  "beyond the length", "wholly beyond the length", "on an empty stream", "short streams",
                                  "across every seam of the last stream", "everything, as a list"])
def test_span_placements(mhc, msgs, sources, dsts, name):
    span_off, spans = span_lists(placements(msgs)[name])
    for each in (False, True):
        src = sources[(1, each)]
        for do in (1, 0):
            edited, ref, packed = expect(src, dsts[do], STAR, span_off, spans)
            for indexed in (True, False):
                check_exact(mhc, src, src.edit(dsts[do], STAR, span_off, spans, indexed), ref, packed, (name, each, do, indexed))
    if name == "only the byte in front of a chunk":
        # just the next chunk's destination context and index entry change: its entry names the mask byte
        plain = recode_ref.recode(src.msgs, oracle_of(dsts[1]), CHUNK)
        assert int(ref[6][3][1]) >> 56 == 0x2A and int(plain[6][3][1]) >> 56 == src.msgs[6][255] != 0x2A
    if name == "wholly beyond the length":
        assert edited == src.msgs


def test_no_span_list_translates_the_whole_batch(mhc, msgs, sources, dsts):
    assert any(65 <= c <= 90 for m in msgs for c in m)
    for each in (False, True):
        src = sources[(1, each)]
        for do in (1, 0):
            edited, ref, packed = expect(src, dsts[do], FOLD, None, None)
            assert edited == [m.lower() for m in src.msgs]
            for indexed in (True, False):
                check_exact(mhc, src, src.edit(dsts[do], FOLD, None, None, indexed), ref, packed, ("fold", each, do, indexed))


def test_a_source_whose_tables_fill_the_lds_reads_the_map_from_l2(mhc):
    """The map's 256 bytes lie in LDS behind the source's tables and the destination's image; 98 contexts of 256 Zipf symbols and
    one of 200 leave 144 bytes (163 840 - 163 696), so neither the order-0 image nor the map fits and both come from L2."""
    c = np.zeros((256, 256), dtype=np.uint64)
    row = (np.floor((1 << 20) / np.arange(1, 257) ** 1.1) + 1).astype(np.uint64)
    c[:98] = row
    c[98, :200] = row[:200]
    c[99:, 0] = 1
    model = mhc.Model.from_counts(c.reshape(-1), 1)
    P, nsec, in_lds = model.decode_layout()
    lds = 1024 + (512 << P) + ((2 * nsec + 15) & ~15)
    assert in_lds and 0 <= 163840 - lds < 256, (P, nsec, lds)
    rng = np.random.default_rng(5)
    w = 1.0 / np.arange(1, 99) ** 1.1
    batch = [rng.choice(98, size=k, p=w / w.sum()).astype(np.uint8).tobytes() for k in (0, 1, 255, 256, 257, 1300)]
    src = Source(mhc, batch, model=model)
    shift = bytes((b + 1) % 98 if b < 98 else b for b in range(256))
    span_off, spans = scattered_spans(batch, 61)
    for do in (0, 1):
        dst = model_of(mhc, [rng.choice(98, size=60000, p=w / w.sum()).astype(np.uint8).tobytes()], do)
        for so_sp in ((span_off, spans), (None, None)):
            _, ref, packed = expect(src, dst, shift, *so_sp)
            for indexed in (True, False):
                check_exact(mhc, src, src.edit(dst, shift, *so_sp, indexed), ref, packed, ("map in L2", do, indexed))


# ---- 3. a mask byte that no message holds, dst trained on the messages ------------------------------------------------------------

def test_mask_without_a_code_is_dropped_as_the_reference_drops_it(mhc, msgs, sources):
    assert not any(0x07 in m for m in msgs)
    dst = model_of(mhc, msgs, 1)
    src = sources[(1, False)]
    span_off, spans = span_lists([[], [], [(0, 1)], [(10, 13)], [(253, 255)], [(0, 2), (254, 256)], [(100, 101), (500, 520)], [(5, 6)]])
    edited, ref, packed = expect(src, dst, edit_ref.mask_map(0x07), span_off, spans)
    # every masked byte is a pair (prev, mask) without a code, and so is the pair behind each span (none ends its message)
    masked = [sum(e - b for b, e in spans[int(span_off[i]):int(span_off[i + 1])].tolist()) for i in range(len(msgs))]
    nspans = np.diff(span_off.astype(np.int64))
    assert packed[3].tolist() == [m + k for m, k in zip(masked, nspans)]
    for indexed in (True, False):
        check_exact(mhc, src, src.edit(dst, edit_ref.mask_map(0x07), span_off, spans, indexed), ref, packed, ("no code", indexed))


# ---- 4. nothing to edit: the plain re-code, byte for byte -------------------------------------------------------------------------

@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("indexed", [True, False])
def test_empty_list_and_identity_map_equal_the_plain_recode(mhc, msgs, sources, dsts, indexed, each):
    src, dst = sources[(1, each)], dsts[1]
    plain = src.recode(dst, indexed)
    empty = span_lists([[] for _ in msgs])
    some = scattered_spans(src.msgs, 5)
    for what, got in (("empty list", src.edit(dst, STAR, *empty, indexed)), ("identity in spans", src.edit(dst, edit_ref.IDENTITY, *some, indexed)),
                      ("identity everywhere", src.edit(dst, edit_ref.IDENTITY, None, None, indexed))):
        for k in ("payload", "out_off", "nbits", "dropped", "status", "sym_off", "index"):
            assert np.array_equal(got[k], plain[k]), (what, k)
        assert got["rc"] == plain["rc"] == mhc.MH_OK


# ---- 5. end to end: search, spans, edit, decode, search again, digests ----------------------------------------------------------------

def identifiers(msgs, k=50):
    words = sorted({w for m in msgs for w in bytes(m).replace(b"\n", b" ").split(b" ") if 4 <= len(w) <= 12 and w.isalpha()})
    assert len(words) >= k
    return words[::len(words) // k][:k]


@pytest.mark.parametrize("kind", ["shift-and", "dictionary", "each"])
def test_find_spans_edit_decode(mhc, msgs, kind):
    pats = [b"in", b"ng", b"ing "] if kind != "dictionary" else identifiers(msgs)
    hits = find_ref.find_hits(msgs, pats)
    w_off, w_rec, _ = find_ref.hit_arrays(hits, len(msgs))
    r_so, r_sp = edit_ref.merge_hits(w_off, w_rec)
    assert len(r_sp) >= 10 and (kind == "dictionary" or len(r_sp) < len(hits))   # `ing ` ends last and begins first
    zero = edit_ref.mask_map(0)
    masked = edit_ref.apply(msgs, r_so, r_sp, zero)
    each = kind == "each"
    if each:
        src = Source(mhc, msgs, each=True)
        dst = model_of(mhc, list(msgs) + masked, 1)                              # a shared model with codes for the masked messages
    else:
        src = Source(mhc, msgs, model=model_of(mhc, list(msgs) + masked, 1))
        dst = src.model                                                          # the edit under the source model
    if kind == "dictionary":
        ho, rec, _, st, rc = src.model.dev_find_dict_batch(mhc.Dict(pats), src.payload, src.pay_off, src.nbits, **src.kw(True))
    elif each:
        ho, rec, _, st, rc = src.model.find(mhc.PatternSet(pats), src.payload, src.pay_off, src.nbits, **src.kw(True))
    else:
        ho, rec, _, st, rc = src.model.dev_find_batch(mhc.PatternSet(pats), src.payload, src.pay_off, src.nbits, **src.kw(True))
    assert rc == mhc.MH_OK and np.array_equal(ho, w_off) and np.array_equal(rec, w_rec)
    d_so, d_sp, rc = mhc.dev_spans_from_hits(ho, rec)
    h_so, h_sp, hrc = mhc.spans_from_hits(ho, rec)
    assert rc == hrc == mhc.MH_OK
    assert np.array_equal(d_so, h_so) and np.array_equal(d_sp, h_sp) and np.array_equal(d_so, r_so) and np.array_equal(d_sp, r_sp)
    # more room than records, and too little
    r_so2, r_sp2, rc = mhc.dev_spans_from_hits(ho, rec, hit_cap=len(rec) + 700)
    assert rc == mhc.MH_OK and np.array_equal(r_so2, r_so) and np.array_equal(r_sp2, r_sp)
    z_so, z_sp, rc = mhc.dev_spans_from_hits(ho, rec[:len(rec) - 1], hit_cap=len(rec) - 1)
    assert rc == mhc.MH_ERR_CAPACITY and not z_so.any() and z_sp.size == 0
    for indexed in (True, False):
        got = src.edit(dst, zero, d_so, d_sp, indexed)
        _, ref, packed = expect(src, dst, zero, d_so, d_sp)
        check_exact(mhc, src, got, ref, packed, (kind, indexed))
        assert not got["dropped"].any()
        back, so, st = dst.decode_batch(got["payload"], got["out_off"], got["nbits"], sym_off=src.sym_off, index=got["index"], chunk_symbols=CHUNK)
        assert back == b"".join(masked) and np.array_equal(so, src.sym_off)
        ps = mhc.Dict(pats) if kind == "dictionary" else mhc.PatternSet(pats)
        find = dst.dev_find_dict_batch if kind == "dictionary" else dst.dev_find_batch
        ho2, rec2, _, st2, rc2 = find(ps, got["payload"], got["out_off"], got["nbits"], sym_off=src.sym_off, index=got["index"], chunk_symbols=CHUNK)
        assert rc2 == mhc.MH_OK and not ho2.any() and len(rec2) == 0               # a second search finds nothing
        crc, ln, st3, rc3 = dst.dev_crc_batch(got["payload"], got["out_off"], got["nbits"], sym_off=src.sym_off, index=got["index"],
                                              chunk_symbols=CHUNK)
        raw, rc4 = mhc.crc_raw_batch(masked)
        assert rc3 == rc4 == mhc.MH_OK and np.array_equal(crc, raw) and ln.tolist() == [len(m) for m in msgs]


# ---- 6. damaged inputs: the verdicts of the plain re-code --------------------------------------------------------------------------

@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("indexed", [True, False])
def test_damaged_streams_get_the_plain_recode_s_verdict(mhc, msgs, sources, dsts, indexed, each):
    src, dst = sources[(1, each)], dsts[1]
    n = len(msgs)
    span_off, spans = scattered_spans(src.msgs, 21)
    clean = src.edit(dst, STAR, span_off, spans, indexed)
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    failed = 0
    for at in (6, 7, 4):
        pl, nb = streams[at], int(src.nbits[at])
        for name, dpl, dnb in [("cut-1", damage.cut(pl, nb, nb - 1), nb - 1), ("cut-9", damage.cut(pl, nb, nb - 9), nb - 9),
                               ("ext1+13", damage.with_length(pl, nb, nb + 13, 1), nb + 13), ("flip-first", damage.flip(pl, 5), nb),
                               ("flip-mid", damage.flip(pl, nb // 2), nb), ("flip-last", damage.flip(pl, nb - 3), nb)]:
            pls, nbs = list(streams), [int(x) for x in src.nbits]
            pls[at], nbs[at] = dpl, dnb
            payload, pay_off = mhc.batch_offsets(pls)
            want = src.recode(dst, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
            got = src.edit(dst, STAR, span_off, spans, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
            what = (at, name, indexed, each)
            assert got["status"].tolist() == want["status"].tolist() and (got["rc"] == mhc.MH_OK) == (want["rc"] == mhc.MH_OK), what
            for k in range(n):
                a0, a1 = int(got["out_off"][k]), int(got["out_off"][k + 1])
                if k != at:
                    c0, c1 = int(clean["out_off"][k]), int(clean["out_off"][k + 1])
                    assert got["payload"][a0:a1].tobytes() == clean["payload"][c0:c1].tobytes() and got["nbits"][k] == clean["nbits"][k], what
                    assert got["dropped"][k] == clean["dropped"][k], what
            if got["status"][at] != mhc.MH_OK:
                failed += 1
                assert got["nbits"][at] == 0 and got["out_off"][at + 1] == got["out_off"][at] and got["dropped"][at] == 0, what
    assert failed >= 6
    if indexed:                                                                   # a damaged index entry
        base = int(mhc.lib().mh_batch_index_base(int(src.sym_off[6]), 6, CHUNK))
        sl = np.array(src.index[base:base + 4], dtype=np.uint64)
        bounds = None
        damaged = damage.x1_off_by_one(sl, bounds, int(src.nbits[6]), 1, ks=[2]) + damage.x4_behind_the_predecessor(sl, bounds, int(src.nbits[6]), 1, ks=[2])
        assert len(damaged) >= 4
        for name, dsl in damaged:
            idx = np.array(src.index, dtype=np.uint64)
            idx[base:base + 4] = dsl
            want = src.recode(dst, True, index=idx)
            got = src.edit(dst, STAR, span_off, spans, True, index=idx)
            assert got["status"].tolist() == want["status"].tolist() and got["status"][6] != mhc.MH_OK, name
            assert got["nbits"][6] == 0 and got["out_off"][7] == got["out_off"][6] and got["dropped"][6] == 0, name


# ---- 7. malformed span lists ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [[(5, 5)], [(9, 4)], [(20, 30), (10, 15)], [(10, 20), (19, 25)], [(0, 3), (3, 9), (8, 12)]])
@pytest.mark.parametrize("indexed", [True, False])
def test_malformed_span_lists_fail_their_streams_alone(mhc, msgs, dsts, indexed, bad):
    five = [msgs[6], msgs[7], msgs[5], msgs[7][:300], msgs[4]]
    src, dst = Source(mhc, five), dsts[1]
    good = [[(0, 9), (250, 260)], [], [(1, 2)], [], [(100, 200)]]
    mixed = [good[0], bad, good[2], bad, good[4]]
    span_off, spans = span_lists(mixed)
    got = src.edit(dst, STAR, span_off, spans, indexed)
    assert got["status"].tolist() == [mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_OK] and got["rc"] == mhc.MH_ERR_ARG
    g_off, g_sp = span_lists(good)
    ok = src.edit(dst, STAR, g_off, g_sp, indexed)
    _, ref, packed = expect(src, dst, STAR, g_off, g_sp)
    check_exact(mhc, src, ok, ref, packed, "good lists")
    for i in range(5):
        a0, a1 = int(got["out_off"][i]), int(got["out_off"][i + 1])
        if i in (1, 3):
            assert a0 == a1 and got["nbits"][i] == 0 and got["dropped"][i] == 0
        else:
            b0, b1 = int(ok["out_off"][i]), int(ok["out_off"][i + 1])
            assert got["payload"][a0:a1].tobytes() == ok["payload"][b0:b1].tobytes() and got["nbits"][i] == ok["nbits"][i]
            assert got["dropped"][i] == ok["dropped"][i]
    if indexed:
        assert np.array_equal(slices_of(got["index"], src.sym_off, CHUNK, (0, 2, 4)), slices_of(ok["index"], src.sym_off, CHUNK, (0, 2, 4)))
    else:
        assert got["sym_off"].tolist() == np.concatenate([[0], np.cumsum([len(five[0]), 0, len(five[2]), 0, len(five[4])])]).tolist()


def test_bad_span_offsets_stop_the_call(mhc, msgs, sources, dsts):
    src = sources[(1, False)]
    span_off, spans = span_lists([[(0, 1)] for _ in msgs])
    spans = np.concatenate([spans, spans[:2]])                                  # (as many pairs as the largest offset below names)
    assert len(msgs) == 8
    for bad in (span_off + np.uint64(1), span_off[::-1].copy(), np.array([0, 3, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint64)):
        for indexed in (True, False):
            got = src.edit(dsts[1], STAR, bad, spans, indexed, count_only=True)
            assert got["rc"] == mhc.MH_ERR_ARG and not got["nbits"].any() and not got["out_off"].any()


# ---- 8. capacity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indexed", [True, False])
def test_a_cap_one_byte_short(mhc, msgs, sources, dsts, indexed):
    src, dst = sources[(1, False)], dsts[1]
    span_off, spans = scattered_spans(src.msgs, 31)
    full = src.edit(dst, STAR, span_off, spans, indexed)
    need = int(full["out_off"][-1])
    short = src.edit(dst, STAR, span_off, spans, indexed, cap=need - 1)
    assert short["rc"] == mhc.MH_ERR_CAPACITY and short["payload"].size == 0
    for k in ("out_off", "nbits", "dropped", "status"):
        assert np.array_equal(short[k], full[k]), (indexed, k)
    roomy = src.edit(dst, STAR, span_off, spans, indexed, cap=need + 100)
    assert roomy["rc"] == mhc.MH_OK and np.array_equal(roomy["payload"], full["payload"])


def test_order2_and_a_set_of_the_wrong_size_are_refused(mhc, msgs, sources):
    src = sources[(1, False)]
    m2 = mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    for a, b in ((m2, src.model), (src.model, m2)):
        with pytest.raises(mhc.MhError) as e:
            a.dev_recode_edit_batch(b, src.payload, src.pay_off, src.nbits, STAR, **src.kw(True))
        assert e.value.status == mhc.MH_ERR_ARG
    ms = mhc.ModelSet.train([bytes(m) for m in msgs[:3]], order=1)
    with pytest.raises(mhc.MhError) as e:
        ms.recode_edit(src.model, src.payload, src.pay_off, src.nbits, STAR, **src.kw(True))
    assert e.value.status == mhc.MH_ERR_ARG


def test_host_form(mhc, msgs, sources, dsts):
    src, dst = sources[(1, False)], dsts[1]
    span_off, spans = scattered_spans(src.msgs, 41)
    _, ref, packed = expect(src, dst, STAR, span_off, spans)
    for indexed in (True, False):
        got = src.model.recode_edit_batch(dst, src.payload, src.pay_off, src.nbits, STAR, span_off, spans, **src.kw(indexed))
        assert got["rc"] == mhc.MH_OK and np.array_equal(got["payload"], packed[0]) and np.array_equal(got["out_off"], packed[1])
        assert np.array_equal(got["nbits"], packed[2]) and np.array_equal(got["dropped"], packed[3]) and np.array_equal(got["sym_off"], src.sym_off)
        assert np.array_equal(slices_of(got["index"], src.sym_off, CHUNK), np.concatenate([r[3] for r in ref]))
    _, ref, packed = expect(src, dst, FOLD, None, None)
    got = src.model.recode_edit_batch(dst, src.payload, src.pay_off, src.nbits, FOLD, **src.kw(True))
    assert np.array_equal(got["payload"], packed[0]) and np.array_equal(got["dropped"], packed[3])


def test_host_form_indexes_a_batch_with_a_stream_over_the_walk_cap_first(mhc):
    """Index-free, one stream over MH_BATCH_WALK_MAX_BITS: the host form indexes the batch first, with the chunk size of
    out_index when it writes one and its own when it does not.  A span in the long stream, one in the first stream."""
    long_msg = np.random.default_rng(61).integers(0, 256, 1_200_000 + 77, dtype=np.uint8).tobytes()      # ~8-bit codes under its own model
    src = Source(mhc, [b"a few bytes", long_msg, b""], order=0)
    assert src.model.min_code_len >= 7 and int(src.nbits[1]) > mhc.BATCH_WALK_MAX_BITS
    dst = model_of(mhc, [long_msg, b"*" * 4000], 0)
    span_off, spans = span_lists([[(2, 5)], [(700_001, 700_300)], []])
    _, ref, packed = expect(src, dst, STAR, span_off, spans)
    for want_index in (True, False):
        got = src.model.recode_edit_batch(dst, src.payload, src.pay_off, src.nbits, STAR, span_off, spans, chunk_symbols=CHUNK,
                                          want_index=want_index, check=False)
        check_exact(mhc, src, got, ref, packed, "over the cap, out_index=%s" % want_index, index=want_index)


# ---- 9. dirty workspaces and outputs; a chain on a non-default stream ------------------------------------------------------------------

@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_prefilled_workspace_and_outputs(mhc, msgs, sources, dsts, byte):
    src, dst = sources[(1, False)], dsts[1]
    span_off, spans = scattered_spans(src.msgs, 51)
    _, ref, packed = expect(src, dst, STAR, span_off, spans)
    hits = find_ref.find_hits(msgs, [b"in", b"ng", b"ing "])
    w_off, w_rec, _ = find_ref.hit_arrays(hits, len(msgs))
    with mhc.device_memory("fill", byte):                                       # the workspaces (created without contents) hold `byte`
        for indexed in (True, False):
            check_exact(mhc, src, src.edit(dst, STAR, span_off, spans, indexed), ref, packed, (byte, indexed))
        d_so, d_sp, rc = mhc.dev_spans_from_hits(w_off, w_rec)
    r_so, r_sp = edit_ref.merge_hits(w_off, w_rec)
    assert rc == mhc.MH_OK and np.array_equal(d_so, r_so) and np.array_equal(d_sp, r_sp)


def test_chain_find_spans_edit_decode_on_one_stream(env, msgs):
    """find -> spans -> edit -> decode on a torch stream, enqueued back to back behind a blocker (tests/test_gpu_stream_order.py)."""
    mhc, lib = env.mhc, env.lib
    pats = [b"in", b"ng", b"ing "]
    hits = find_ref.find_hits(msgs, pats)
    n, k = len(msgs), len(hits)
    w_off, w_rec, _ = find_ref.hit_arrays(hits, n)
    r_so, r_sp = edit_ref.merge_hits(w_off, w_rec)
    zero = edit_ref.mask_map(0)
    masked = edit_ref.apply(msgs, r_so, r_sp, zero)
    model = model_of(mhc, list(msgs) + masked, 1)
    src = Source(mhc, msgs, model=model)
    _, ref, packed = expect(src, model, zero, r_so, r_sp)
    total, pay_total = int(src.sym_off[n]), int(src.pay_off[n])
    nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
    ps = mhc.PatternSet(pats)
    ch = Chain(env, "edit chain")
    ch.keep = (model, ps)
    b = Batch(ch.staged(np.concatenate([src.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(src.pay_off), ch.staged(src.nbits), n, pay_total)
    d_in, d_idx, d_map = ch.staged(src.sym_off), ch.staged(np.asarray(src.index, dtype=np.uint64)[:nidx]), ch.staged(np.frombuffer(zero, dtype=np.uint8))
    # find, with room for exactly the reference's hits
    wsb = lib.mh_dev_find_batch_workspace(n, total, CHUNK)
    d_ws, d_ho, d_rec, d_st = ch.work(wsb), ch.words(n + 1), ch.out(k * 24 + 64), ch.status(n, "find")
    ch.call("find_batch", lib.mh_dev_find_batch, model.handle, ps.handle, *b.args(), 0x20, ptr(d_in), total, ptr(d_idx), CHUNK, ptr(d_ho), ptr(d_rec),
            None, k, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("find: records", lambda: same(ch.get(d_rec, np.uint64, 3 * k).reshape(-1, 3), w_rec) and same(ch.get(d_ho, np.uint64, n + 1), w_off))
    # spans
    wsb2 = lib.mh_dev_spans_from_hits_workspace(n, k)
    d_ws2, d_so, d_sp = ch.work(wsb2), ch.words(n + 1), ch.out(k * 16 + 64)
    ch.call("spans_from_hits", lib.mh_dev_spans_from_hits, ptr(d_ho), ptr(d_rec), k, n, ptr(d_so), ptr(d_sp), ptr(d_ws2), wsb2, ws=d_ws2)
    m = len(r_sp)
    ch.expect("spans", lambda: same(ch.get(d_so, np.uint64, n + 1), r_so) and same(ch.get(d_sp, np.uint64, 2 * m).reshape(-1, 2), r_sp)
              and (ch.get(d_sp)[16 * m:] == 0xA5).all())
    # edit under the source model
    cap = int(packed[1][n])
    wsb3 = lib.mh_dev_recode_edit_workspace(n, total, CHUNK)
    d_ws3, d_st3 = ch.work(wsb3), ch.status(n, "edit")
    d_oo, d_onb, d_dr, d_out, d_oi = ch.words(n + 1), ch.words(n), ch.words(n), ch.out(cap + 64), ch.words(nidx)
    ch.call("recode_edit_batch", lib.mh_dev_recode_edit_batch, model.handle, model.handle, *b.args(), 0x20, ptr(d_in), total, ptr(d_idx), CHUNK,
            ptr(d_so), ptr(d_sp), ptr(d_map), ptr(d_out), cap, ptr(d_oo), ptr(d_onb), ptr(d_oi), ptr(d_dr), ptr(d_st3), ptr(d_ws3), wsb3, ws=d_ws3)
    ch.expect("edit: offsets, nbits, dropped", lambda: same(ch.get(d_oo, np.uint64, n + 1), packed[1]) and same(ch.get(d_onb, np.uint64, n), packed[2])
              and same(ch.get(d_dr, np.uint64, n), packed[3]))
    ch.expect("edit: payload", lambda: same(ch.get(d_out, np.uint8, cap), packed[0]) and (ch.get(d_out)[cap:cap + 64] == 0xA5).all())
    ch.expect("edit: index slices", lambda: same(slices_of(ch.get(d_oi, np.uint64, nidx), src.sym_off, CHUNK), np.concatenate([r[3] for r in ref])))
    # decode what the edit wrote, through the index it wrote
    wsb4 = lib.mh_dev_decode_batch_workspace(n)
    d_ws4, d_dec, d_st4 = ch.work(wsb4), ch.out(total + 64), ch.status(n, "decode")
    ch.call("decode_batch", lib.mh_dev_decode_batch, model.handle, ptr(d_out), ptr(d_oo), ptr(d_onb), n, cap, 0x20, ptr(d_dec), total, ptr(d_in), total,
            ptr(d_oi), CHUNK, ptr(d_st4), ptr(d_ws4), wsb4, ws=d_ws4)
    ch.expect("decode: the masked messages", lambda: ch.get(d_dec, np.uint8, total).tobytes() == b"".join(masked))
    drive(ch)


# ---- 10. seeded fuzz ----------------------------------------------------------------------------------------------------------------

def test_fuzz_of_30_small_batches(mhc):
    text = golden()["input_wiki_cpp.txt"]["data"]
    rng = np.random.default_rng(777)
    dsts = {do: model_of(mhc, [text[:20000], bytes(range(97, 123)) * 3], do) for do in (0, 1)}
    for trial in range(30):
        n = int(rng.integers(1, 7))
        lens = [int(rng.choice([0, 1, 2, 255, 256, 257, int(rng.integers(3, 900))])) for _ in range(n)]
        batch = []
        for k in lens:
            at = int(rng.integers(0, len(text) - 1000))
            batch.append(text[at:at + k] if rng.random() < 0.7 else bytes(rng.integers(97, 105, k, dtype=np.uint8)))
        so, do, each, indexed = int(rng.integers(0, 2)), int(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        kind = int(rng.integers(0, 4))
        byte_map = [STAR, FOLD, bytes(rng.permutation(256).astype(np.uint8)), bytes(rng.integers(97, 123, 256, dtype=np.uint8))][kind]
        span_off, spans = (None, None) if rng.random() < 0.2 else scattered_spans(batch, 1000 + trial)
        src = Source(mhc, batch, order=so, each=each)
        dst = dsts[do]
        _, ref, packed = expect(src, dst, byte_map, span_off, spans)
        check_exact(mhc, src, src.edit(dst, byte_map, span_off, spans, indexed), ref, packed, (trial, lens, so, do, each, indexed, kind))


# ---- 11. CLI ----------------------------------------------------------------------------------------------------------------------------

def test_cli_redact(mhc, tmp_path):
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    x, y = "input_wiki_cpp.txt", "input_ipsum.txt"
    data = golden()[x]["data"]
    p = lambda n: str(tmp_path / n)
    for name, blob in (("x", data), ("x.cm", expected_file(x, "cm")), ("x.e", expected_file(x, "e")), ("y.e", expected_file(y, "e"))):
        with open(p(name), "wb") as f:
            f.write(blob)
    run = lambda a: subprocess.run([cli] + a, capture_output=True, timeout=300)

    def masked_by(pats, byte, fold=False):
        hits = find_ref.find_hits([data], pats, fold=fold)
        off, rec, _ = find_ref.hit_arrays(hits, 1)
        so, sp = edit_ref.merge_hits(off, rec)
        return edit_ref.apply([data], so, sp, edit_ref.mask_map(byte))[0], len(sp), int((sp[:, 1] - sp[:, 0]).sum())

    def want_file(table, text):
        blob, _ = mh_oracle.Model.from_table(table).compress(text)
        return blob

    # --redact, the default mask, under another table; index-free, as the reference wrote the file
    text, nspans, nbytes = masked_by([b"language", b"age"], 0x2A)
    assert nspans > 5 and text != data
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("y.e"), "-o", p("out.cm"), "--redact", "language", "--redact", "age"])
    assert r.returncode == 0, r.stderr
    assert open(p("out.cm"), "rb").read() == want_file(expected_file(y, "e"), text) and not os.path.exists(p("out.cm.idx"))
    assert ("Masking %d bytes in %d spans with 0x2A." % (nbytes, nspans)).encode() in r.stderr, r.stderr
    # --redact-file, --redact-fold and --mask under the same table, with the index: the output's own index beside it
    words = [b"Stroustrup", b"template", b"class", b"C++", b"standard library", b"the"]
    with open(p("deny.txt"), "wb") as f:
        f.write(b"\n".join(words) + b"\n\n")
    text, nspans, nbytes = masked_by(words, 0x20, fold=True)
    with open(p("masked"), "wb") as f:
        f.write(text)
    assert run([p("x"), "-e", p("x.e"), "-o", p("x2.cm"), "--index", p("x.idx"), "--chunk", "256"]).returncode == 0
    assert run([p("masked"), "-e", p("x.e"), "-o", p("m.cm"), "--index", p("m.idx"), "--chunk", "256"]).returncode == 0
    r = run([p("x2.cm"), "-x", "-e", p("x.e"), "--recode", p("x.e"), "-o", p("out2.cm"), "--index", p("x.idx"), "--redact-file", p("deny.txt"),
             "--redact-fold", "--mask", "0x20"])
    assert r.returncode == 0, r.stderr
    assert open(p("out2.cm"), "rb").read() == want_file(expected_file(x, "e"), text) == open(p("m.cm"), "rb").read()
    assert open(p("out2.cm.idx"), "rb").read() == open(p("m.idx"), "rb").read()
    assert ("Masking %d bytes in %d spans with 0x20." % (nbytes, nspans)).encode() in r.stderr, r.stderr
    # a pattern that does not occur: the plain re-code
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("y.e"), "-o", p("out3.cm"), "--redact", "zzzzqqqq", "--mask", "7"])
    assert r.returncode == 0 and b"Masking 0 bytes in 0 spans" in r.stderr
    assert open(p("out3.cm"), "rb").read() == want_file(expected_file(y, "e"), data)
    # an order-2 new table is refused by name
    with open(p("o2.e"), "wb") as f:
        f.write(mhc.Model.from_counts(mhc.histogram_o2(data[:4000]), 2).table_bytes())
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("o2.e"), "-o", p("out4.cm"), "--redact", "age"])
    assert r.returncode == 1 and b"--recode does not support an order-2 table" in r.stderr
