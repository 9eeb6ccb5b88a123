"""Pattern search in compressed batches on the GPU (include/mh.h, "SEARCH IN BATCHES"): under a shared model, per-stream
models and a picked bank, with and without the chunk index, count-only and with records.  The reference for every case is
tests/find_ref.py (bytes.find on the original messages); every case asserts that its reference found what the case is about.
The device-call wrappers (Model.dev_find_batch, ModelSet.find) put guard words behind hit_off, the records and the pattern
numbers and assert that they, and every record at or beyond hit_cap, kept their fill."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
import find_ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "bin", "markovhuffman")
WIKI_PATTERNS = [b"href", b'<a href="', b"C++", b"</span>", b"e", b"template", b"zzzz"]
WIKI_HITS = {b"href": (1935, 1029), b'<a href="': (1584, 1009), b"C++": (520, 208), b"</span>": (892, 257), b"e": (21910, 1284),
             b"template": (52, 17), b"zzzz": (0, 0)}


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


class Packed:
    """A batch of messages under one shared order-`order` model trained on them, encoded with an index of `chunk`."""

    def __init__(self, mhc, msgs, chunk, order=1, model=None):
        self.mhc, self.msgs, self.chunk = mhc, [bytes(m) for m in msgs], chunk
        self.model = model or mhc.Model.from_counts(mhc.histogram_o1_batch(self.msgs, order=order), order)
        self.payload, self.pay_off, self.nbits, self.index, self.sym_off = self.model.encode_batch(self.msgs, chunk_symbols=chunk)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else {}

    def find(self, ps, indexed, **kw):
        return self.model.dev_find_batch(ps, self.payload, self.pay_off, self.nbits, **self.kw(indexed), **kw)


def check(mhc, got, hits, n, what=""):
    """A device result (hit_off, records, pattern numbers, statuses, status word) against the reference's hits."""
    ho, rec, pat, st, rc = got
    off, wrec, wpat = find_ref.hit_arrays(hits, n)
    assert rc == mhc.MH_OK and (st == mhc.MH_OK).all(), (what, rc, np.unique(st))
    assert np.array_equal(ho, off), what
    assert np.array_equal(rec, wrec) and np.array_equal(pat, wpat), what


def check_all_ways(mhc, b, patterns, hits, fold=False, what=""):
    """Indexed and index-free, count-only and with records: the same answer."""
    ps = mhc.PatternSet(patterns, fold=fold)
    n = len(b.msgs)
    off = find_ref.hit_arrays(hits, n)[0]
    for indexed in (True, False):
        ho, rec, pat, st, rc = b.find(ps, indexed, count_only=True)
        assert rc == mhc.MH_OK and (st == mhc.MH_OK).all() and np.array_equal(ho, off) and rec.size == 0, (what, indexed)
        check(mhc, b.find(ps, indexed), hits, n, "%s indexed=%s" % (what, indexed))


@pytest.fixture(scope="module")
def wiki_lines():
    lines = [l for l in golden()["input_wiki_cpp.html"]["data"].split(b"\n") if l]
    assert len(lines) == 1581 and max(len(l) for l in lines) == 21588
    return lines


@pytest.fixture(scope="module", params=[256, 1024])
def wiki(request, mhc, wiki_lines):
    return Packed(mhc, wiki_lines, request.param)


@pytest.mark.parametrize("pattern", WIKI_PATTERNS)
def test_wiki_lines_one_pattern(mhc, wiki, pattern):
    hits = find_ref.find_hits(wiki.msgs, [pattern])
    assert (len(hits), find_ref.lines_with(hits, 0)) == WIKI_HITS[pattern]
    check_all_ways(mhc, wiki, [pattern], hits, what=repr(pattern))


def test_wiki_lines_fold(mhc, wiki):
    hits = find_ref.find_hits(wiki.msgs, [b"c++"], fold=True)
    assert len(hits) == 550 and len(find_ref.find_hits(wiki.msgs, [b"c++"])) < 550
    check_all_ways(mhc, wiki, [b"c++"], hits, fold=True, what="fold")


def test_wiki_lines_all_patterns_in_one_set(mhc, wiki):
    assert sum(len(p) for p in WIKI_PATTERNS) == 36
    hits = find_ref.find_hits(wiki.msgs, WIKI_PATTERNS)
    for j, p in enumerate(WIKI_PATTERNS):
        assert sum(1 for h in hits if h[3] == j) == WIKI_HITS[p][0]
    check_all_ways(mhc, wiki, WIKI_PATTERNS, hits, what="union")


@pytest.mark.parametrize("chunk,straddling", [(256, 22), (1024, 6)])
def test_wiki_as_one_stream(mhc, chunk, straddling):
    data = golden()["input_wiki_cpp.html"]["data"]
    hits = find_ref.find_hits([data], [b"</span>"])
    assert len(hits) == 892 and find_ref.straddles(hits, chunk) == straddling
    b = Packed(mhc, [data], chunk)
    ps = mhc.PatternSet([b"</span>"])
    check(mhc, b.find(ps, True), hits, 1)
    check(mhc, b.find(ps, False), hits, 1)


@pytest.mark.parametrize("chunk", [256, 1024])
def test_seams_64_byte_pattern_at_every_offset_behind_a_boundary(mhc, chunk):
    pattern = bytes(range(1, 65))
    assert len(pattern) == mhc.FIND_MAX_POSITIONS
    msgs = []
    for k in range(64):                                        # the pattern ends k bytes behind every chunk boundary
        m = bytearray(b"\xee" * 5000)
        for edge in range(chunk, 5000 - 64, chunk):
            m[edge + k - 64:edge + k] = pattern
        msgs.append(bytes(m))
    hits = find_ref.find_hits(msgs, [pattern])
    per = len(range(chunk, 5000 - 64, chunk))
    assert len(hits) == 64 * per and find_ref.straddles(hits, chunk) == 63 * per
    check_all_ways(mhc, Packed(mhc, msgs, chunk), [pattern], hits, what="seams")


@pytest.mark.parametrize("chunk", [256, 1024])
def test_seams_suffix_patterns_and_runs(mhc, chunk):
    rng = np.random.default_rng(5)
    text = bytes(rng.choice(np.frombuffer(b"abcx", dtype=np.uint8), size=6000))
    pats = [b"abcab", b"cab", b"b", b"abcab", b"ab"]          # a pattern, its suffixes, a duplicate: equal ends, all pattern numbers
    msgs = [text, b"a" * 300, text[::-1], b"abcab" * 700]
    hits = find_ref.find_hits(msgs, pats)
    ends = {}
    for i, _, e, j in hits:
        ends.setdefault((i, e), []).append(j)
    assert any(len(v) >= 4 for v in ends.values()) and find_ref.straddles(hits, chunk) >= 5
    check_all_ways(mhc, Packed(mhc, msgs, chunk), pats, hits, what="suffixes")
    run = find_ref.find_hits(msgs, [b"aaaa"])
    assert len([h for h in run if h[0] == 1]) == 297
    check_all_ways(mhc, Packed(mhc, msgs, chunk), [b"aaaa"], run, what="aaaa")


def test_stream_boundaries_and_empty_streams(mhc):
    msgs = [b"", b"", b"xxxxab", b"cxxxx", b"", b"abc", b"a", b"ab", b"", b"zabcabc", b"", b""]
    pats = [b"abc", b"a", b"abcabcabc"]
    hits = find_ref.find_hits(msgs, pats)
    assert [h for h in hits if h[3] == 0] == [(5, 0, 3, 0), (9, 1, 4, 0), (9, 4, 7, 0)]       # nothing across streams 2 | 3
    assert not [h for h in hits if h[3] == 2]                                                  # longer than every stream
    assert (6, 0, 1, 1) in hits                                                                # the one-byte stream
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs * 3 + [bytes(range(256)) * 2], order=1), 1)
    check_all_ways(mhc, Packed(mhc, msgs, 256, model=model), pats, hits, what="boundaries")
    none = Packed(mhc, [], 256, model=model)
    check_all_ways(mhc, none, pats, [], what="n_streams == 0")
    ho, rec, pat, st, rc = model.find_batch(mhc.PatternSet(pats), none.payload, none.pay_off, none.nbits)
    assert ho.tolist() == [0] and rec.size == 0 and rc == mhc.MH_OK
    only_empty = Packed(mhc, [b"", b"", b""], 256, model=model)
    check_all_ways(mhc, only_empty, pats, [], what="empty streams only")


@pytest.mark.parametrize("order", [0, 1])
def test_large_zipf_stream(mhc, order):
    rng = np.random.default_rng(17)
    data = bytearray(zipf(8 << 20, 3))
    planted = b"\xf0\xf1\xf2\xf3\xf4\xf5\xf6\xf7\xf8\xf9\xfa\xfb"
    places = sorted(int(x) for x in rng.choice((8 << 20) // 64, size=100, replace=False) * 64 + rng.integers(0, 40, 100))
    for at in places:
        data[at:at + 12] = planted
    data = bytes(data)
    pats = [data[1000:1002], data[5000:5003], planted]
    hits = find_ref.find_hits([data], pats)
    assert sum(1 for h in hits if h[3] != 2) > 1000
    assert [h[1] for h in hits if h[3] == 2] == places
    b = Packed(mhc, [data], 1024, order=order)
    ps = mhc.PatternSet(pats)
    check(mhc, b.find(ps, True), hits, 1, "8 MiB indexed")
    # index-free the stream is over the walk cap: refused by the device call, indexed and searched by the host form
    assert int(b.nbits[0]) > mhc.BATCH_WALK_MAX_BITS
    ho, rec, pat, st, rc = b.find(ps, False)
    assert st.tolist() == [mhc.MH_ERR_ARG] and rc == mhc.MH_ERR_ARG and ho.tolist() == [0, 0] and rec.size == 0
    ho, rec, pat, st, rc = b.model.find_batch(ps, b.payload, b.pay_off, b.nbits)
    off, wrec, wpat = find_ref.hit_arrays(hits, 1)
    assert rc == mhc.MH_OK and st.tolist() == [mhc.MH_OK]
    assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat)
    ho, rec, pat, st, rc = b.model.find_batch(ps, b.payload, b.pay_off, b.nbits, **b.kw(True))
    assert rc == mhc.MH_OK and np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat)


def test_large_batch_of_small_streams(mhc):
    rng = np.random.default_rng(23)
    data = bytearray(zipf(65536 * 256, 4))
    planted = b"needle-12-b!"
    where = sorted(int(x) for x in rng.choice(65536, size=100, replace=False))
    for i in where:
        at = i * 256 + int(rng.integers(0, 256 - 12))
        data[at:at + 12] = planted
    msgs = [bytes(data[i * 256:(i + 1) * 256]) for i in range(65536)]
    pats = [bytes(data[777:779]), bytes(data[4000:4003]), planted]
    hits = find_ref.find_hits(msgs, pats)
    assert sum(1 for h in hits if h[3] != 2) > 1000
    assert [h[0] for h in hits if h[3] == 2] == where
    check_all_ways(mhc, Packed(mhc, msgs, 256), pats, hits, what="65536 x 256 B")


def test_per_stream_models_and_a_picked_bank(mhc, wiki_lines):
    msgs = wiki_lines[:400]
    pats = [b"href", b"</span>", b"C++"]
    hits = find_ref.find_hits(msgs, pats)
    assert len(hits) > 300
    n = len(msgs)
    ps = mhc.PatternSet(pats)
    shared = Packed(mhc, msgs, 256)
    check(mhc, shared.find(ps, True), hits, n, "shared")
    ms = mhc.ModelSet.train(msgs, order=1)
    payload, out_off, nbits, idx, in_off, rc = ms.encode(msgs, chunk_symbols=256)
    assert rc == mhc.MH_OK
    check(mhc, ms.find(ps, payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=256), hits, n, "each indexed")
    check(mhc, ms.find(ps, payload, out_off, nbits), hits, n, "each index-free")
    ho, rec, pat, st, rc = ms.find(ps, payload, out_off, nbits, count_only=True)
    assert np.array_equal(ho, find_ref.hit_arrays(hits, n)[0]) and rec.size == 0
    bank, choice, _ = mhc.ModelSet.train_bank(msgs, 4, order=1)
    payload, out_off, nbits, idx, in_off = mhc.encode_bank(bank, msgs, choice, chunk_symbols=1024)
    view = bank.pick(choice)
    check(mhc, view.find(ps, payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024), hits, n, "bank indexed")
    check(mhc, view.find(ps, payload, out_off, nbits), hits, n, "bank index-free")
    wrong = mhc.ModelSet.train(msgs[:10], order=1)
    with pytest.raises(mhc.MhError) as e:                       # n_streams != the set's size
        wrong.find(ps, payload, out_off, nbits, count_only=True)
    assert e.value.status == mhc.MH_ERR_ARG


@pytest.mark.parametrize("indexed", [True, False])
def test_hit_cap(mhc, wiki, indexed):
    ps = mhc.PatternSet([b"href", b"C++"])
    hits = find_ref.find_hits(wiki.msgs, [b"href", b"C++"])
    n, total = len(wiki.msgs), len(hits)
    assert total == 1935 + 520
    off, wrec, wpat = find_ref.hit_arrays(hits, n)
    for cap, want_rc in ((0, mhc.MH_ERR_CAPACITY), (total - 1, mhc.MH_ERR_CAPACITY), (total, mhc.MH_OK), (7, mhc.MH_ERR_CAPACITY)):
        ho, rec, pat, st, rc = wiki.find(ps, indexed, hit_cap=cap)    # (the wrapper asserts the guard words and the records >= cap)
        assert rc == want_rc and (st == mhc.MH_OK).all(), cap
        assert np.array_equal(ho, off), cap                          # complete whether or not the records fit
        assert np.array_equal(rec, wrec[:cap]) and np.array_equal(pat, wpat[:cap]), cap
        ho, rec, pat, st, rc = wiki.model.find_batch(ps, wiki.payload, wiki.pay_off, wiki.nbits, hit_cap=cap, check=False, **wiki.kw(indexed))
        assert rc == want_rc and np.array_equal(ho, off) and np.array_equal(rec, wrec[:cap]) and np.array_equal(pat, wpat[:cap]), cap


@pytest.mark.parametrize("fold", [False, True])
def test_records_are_lookups(mhc, wiki, fold):
    pats = [b"c++", b"HREF", b"</span>"] if fold else [b"C++", b"href", b"</span>"]
    ps = mhc.PatternSet(pats, fold=fold)
    want = len(find_ref.find_hits(wiki.msgs, pats, fold=fold))
    assert want >= (550 if fold else 520) + 1935 + 892          # (folded, `HREF` also finds the one `Href`)
    for indexed in (True, False):
        ho, rec, pat, st, rc = wiki.find(ps, indexed)
        assert rc == mhc.MH_OK and rec.shape[0] == want
        res, lst, lrc = wiki.model.dev_decode_batch_ranges(wiki.payload, wiki.pay_off, wiki.nbits, rec, **wiki.kw(indexed))
        assert lrc == mhc.MH_OK and (lst == mhc.MH_OK).all()
        for r, j in zip(res, pat):
            assert (find_ref.fold_ascii(r) == find_ref.fold_ascii(pats[j])) if fold else (r == pats[j])


def test_two_calls_give_identical_buffers(mhc, wiki):
    ps = mhc.PatternSet(WIKI_PATTERNS)
    for indexed in (True, False):
        a, b = wiki.find(ps, indexed), wiki.find(ps, indexed)
        assert a[1].shape[0] == sum(v[0] for v in WIKI_HITS.values())
        for x, y in zip(a[:4], b[:4]):
            assert x.tobytes() == y.tobytes()


def test_order2_model_is_refused(mhc):
    data = zipf(50000, 9)
    m2 = mhc.Model.from_counts(mhc.histogram_o2(data), 2)
    b = Packed(mhc, [data[:3000], data[3000:9000]], 256)
    ps = mhc.PatternSet([b"ab"])
    for indexed in (True, False):
        with pytest.raises(mhc.MhError) as e:
            m2.dev_find_batch(ps, b.payload, b.pay_off, b.nbits, count_only=True, **b.kw(indexed))
        assert e.value.status == mhc.MH_ERR_ARG
        with pytest.raises(mhc.MhError) as e:
            m2.find_batch(ps, b.payload, b.pay_off, b.nbits, **b.kw(indexed))
        assert e.value.status == mhc.MH_ERR_ARG


# ---- damaged batches ----------------------------------------------------------------------------------------------------------

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
def test_damaged_streams_get_the_decoder_s_verdict(mhc, indexed):
    chunk = 256
    msgs = [zipf(k, 40 + k) for k in (30_000, 5_000, 60_000, 700, 45_000)]
    pats = [msgs[0][100:102], msgs[2][500:503]]
    b = Packed(mhc, msgs, chunk)
    ps = mhc.PatternSet(pats)
    hits = find_ref.find_hits(msgs, pats)
    assert all(any(h[0] == i for h in hits) for i in range(5))
    clean = b.find(ps, indexed)
    check(mhc, clean, hits, 5, "undamaged")
    streams = [bytes(b.payload[int(b.pay_off[i]):int(b.pay_off[i + 1])]) for i in range(5)]
    failed = 0
    for at in (0, 2, 4):
        pl, nb = streams[at], int(b.nbits[at])
        base = int(b.mhc.lib().mh_batch_index_base(int(b.sym_off[at]), at, chunk))
        entry_bit = int(b.index[base + 3]) & mhc.INDEX_BIT_MASK
        cases = [("cut-1", damage.cut(pl, nb, nb - 1), nb - 1), ("cut-9", damage.cut(pl, nb, nb - 9), nb - 9),
                 ("ext0+5", damage.with_length(pl, nb, nb + 5, 0), nb + 5), ("ext1+13", damage.with_length(pl, nb, nb + 13, 1), nb + 13),
                 ("flip-first", damage.flip(pl, 5), nb), ("flip-mid", damage.flip(pl, nb // 2), nb), ("flip-last", damage.flip(pl, nb - 3), nb),
                 ("cut-entry", damage.cut(pl, nb, entry_bit), entry_bit), ("cut-entry+1", damage.cut(pl, nb, entry_bit + 1), entry_bit + 1),
                 ("garbage", damage.garbage_after(pl, nb, 1), nb)]
        for name, dpl, dnb in cases:
            pls, nbs = list(streams), [int(x) for x in b.nbits]
            pls[at], nbs[at] = dpl, dnb
            payload, pay_off = mhc.batch_offsets(pls)
            kw = b.kw(indexed)
            want_st, want_rc = dev_decode_statuses(mhc, b.model, payload, pay_off, nbs, **kw)
            ho, rec, pat, st, rc = b.model.dev_find_batch(ps, payload, pay_off, nbs, **kw)
            what = "stream %d %s indexed=%s" % (at, name, indexed)
            assert st.tolist() == want_st.tolist(), what
            assert (rc == mhc.MH_OK) == (want_rc == mhc.MH_OK), what
            assert all(int(s) == mhc.MH_OK for k, s in enumerate(st) if k != at), what
            if st[at] != mhc.MH_OK:
                failed += 1
                keep = [h for h in hits if h[0] != at]                         # no hits of the failed stream, every other one's
                off, wrec, wpat = find_ref.hit_arrays(keep, 5)
                assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat), what
            else:
                others = [h for h in hits if h[0] != at]
                got = [(int(i), int(x), int(y), int(j)) for (i, x, y), j in zip(rec, pat) if int(i) != at]
                assert got == others, what
    assert failed >= 12                                                        # the damages did fail streams
    # nbits beyond the stream's payload bytes: MH_ERR_ARG for that stream alone, as the decoder says
    nbs = [int(x) for x in b.nbits]
    nbs[1] = (int(b.pay_off[2]) - int(b.pay_off[1])) * 8 + 1
    want_st, _ = dev_decode_statuses(mhc, b.model, b.payload, b.pay_off, nbs, **b.kw(indexed))
    ho, rec, pat, st, rc = b.model.dev_find_batch(ps, b.payload, b.pay_off, nbs, **b.kw(indexed))
    assert st.tolist() == want_st.tolist() and st[1] == mhc.MH_ERR_ARG and rc == mhc.MH_ERR_ARG
    off, wrec, wpat = find_ref.hit_arrays([h for h in hits if h[0] != 1], 5)
    assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat)


def test_bad_offsets_stop_the_call(mhc):
    b = Packed(mhc, [zipf(3000, 1), zipf(2000, 2)], 256)
    ps = mhc.PatternSet([b"\x00"])
    po = b.pay_off.copy()
    po[1] = po[2] + np.uint64(1)                                               # decreasing
    ho, rec, pat, st, rc = b.model.dev_find_batch(ps, b.payload, po, b.nbits, count_only=True, **b.kw(True))
    assert rc == mhc.MH_ERR_ARG and ho.tolist() == [0, 0, 0]


# ---- CLI ----------------------------------------------------------------------------------------------------------------------

def test_cli_find(mhc, tmp_path):
    src = os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.html")
    data = open(src, "rb").read()
    cm, table, idx = (str(tmp_path / n) for n in ("in.cm", "table", "f.idx"))
    r = subprocess.run([CLI, src, "-o", cm, "-d", table, "--index", idx, "--chunk", "256"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    find = [CLI, cm, "-x", "-e", table, "--index", idx]
    r = subprocess.run(find + ["--find", "</span>", "--find", "C++", "--find", "span>"], capture_output=True, timeout=300)
    hits = find_ref.find_hits([data], [b"</span>", b"C++", b"span>"])
    assert len(hits) == 892 + 520 + len(find_ref.occurrences(data, b"span>"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == ["%d %d" % (j, b) for _, b, _, j in hits]
    r = subprocess.run(find + ["--find", "c++", "--find-fold"], capture_output=True, timeout=300)
    want = find_ref.find_hits([data], [b"c++"], fold=True)
    assert len(want) == 550 and r.returncode == 0 and r.stdout.decode().splitlines() == ["0 %d" % b for _, b, _, _ in want]
    r = subprocess.run(find + ["--find", "zzzz", "-o", str(tmp_path / "out")], capture_output=True, timeout=300)
    assert r.returncode == 1 and r.stdout == b"" and not os.path.exists(str(tmp_path / "out"))
