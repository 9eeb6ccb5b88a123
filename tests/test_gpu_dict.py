"""Dictionary search in compressed batches on the GPU (include/mh.h, "DICTIONARY SEARCH IN BATCHES"): thousands of patterns in
one pass of an Aho-Corasick DFA, under a shared model of order 0, 1 and 2, per-stream models and a picked bank, with and
without the chunk index, count-only and with records.  The reference for every case is tests/find_ref.py on the original
messages; equality is exact everywhere.  The device-call wrappers (Model.dev_find_dict_batch, ...) put guard words behind
hit_off, the records and the pattern numbers and assert that they, and every record at or beyond hit_cap, kept their fill.
The expected counts were computed on the CPU from the golden input with find_ref alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
import find_ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "bin", "markovhuffman")
SUFFIXES = [b"abcab", b"cab", b"b", b"abcab", b"ab"]          # a pattern, its suffixes, a duplicate (test_gpu_find's set)
A_FAMILY = [b"a" * k for k in range(1, 256)]


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
        self.mhc, self.msgs, self.chunk, self.order = mhc, [bytes(m) for m in msgs], chunk, order
        if order == 2:
            self.model = model or mhc.Model.from_counts(mhc.histogram_o2_batch(self.msgs), 2)
            enc = self.model.encode_batch_o2
        else:
            self.model = model or mhc.Model.from_counts(mhc.histogram_o1_batch(self.msgs, order=order), order)
            enc = self.model.encode_batch
        self.payload, self.pay_off, self.nbits, self.index, self.sym_off = enc(self.msgs, chunk_symbols=chunk)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else {}

    def find(self, d, indexed, **kw):
        fn = self.model.dev_find_dict_batch_o2 if self.order == 2 else self.model.dev_find_dict_batch
        return fn(d, self.payload, self.pay_off, self.nbits, **self.kw(indexed), **kw)


def check(mhc, got, want, what=""):
    """A device result (hit_off, records, pattern numbers, statuses, status word) against the reference's arrays."""
    ho, rec, pat, st, rc = got
    off, wrec, wpat = want
    assert rc == mhc.MH_OK and (st == mhc.MH_OK).all(), (what, rc, np.unique(st))
    assert np.array_equal(ho, off), what
    assert np.array_equal(rec, wrec) and np.array_equal(pat, wpat), what


def check_all_ways(mhc, find, d, want, what=""):
    """Indexed and index-free, count-only and with records: the same answer.  find(d, indexed, **kw) is the device call."""
    for indexed in (True, False):
        ho, rec, pat, st, rc = find(d, indexed, count_only=True)
        assert rc == mhc.MH_OK and (st == mhc.MH_OK).all() and np.array_equal(ho, want[0]) and rec.size == 0, (what, indexed)
        check(mhc, find(d, indexed), want, "%s indexed=%s" % (what, indexed))


@pytest.fixture(scope="module")
def wiki_data():
    return golden()["input_wiki_cpp.html"]["data"]


@pytest.fixture(scope="module")
def tokens(wiki_data):
    t = sorted(set(re.findall(rb"[A-Za-z_]{4,}", wiki_data)))
    assert len(t) == 3664 and sum(len(x) for x in t) == 33990
    return t


@pytest.fixture(scope="module")
def wiki_lines(wiki_data):
    lines = [l for l in wiki_data.split(b"\n") if l]
    assert len(lines) == 1581
    return lines


@pytest.fixture(scope="module")
def wiki_want(wiki_lines, tokens):
    """The reference's answer for the whole dictionary on the lines, computed once."""
    hits = find_ref.find_hits(wiki_lines, tokens)
    assert len(hits) == 41061
    return find_ref.hit_arrays(hits, len(wiki_lines))


@pytest.fixture(scope="module")
def wiki_dict(mhc, tokens):
    d = mhc.Dict(tokens)
    assert d.states == 19174 and d.classes == 54
    assert d.states * d.classes * 2 > 160 * 1024                  # more rows than any model kind can keep in LDS: both row paths run
    return d


@pytest.fixture(scope="module", params=[256, 1024])
def wiki(request, mhc, wiki_lines):
    return Packed(mhc, wiki_lines, request.param)


# ---- 1, 2: the wiki page ---------------------------------------------------------------------------------------------------

def test_wiki_lines_whole_dictionary(mhc, wiki, wiki_dict, wiki_want):
    assert wiki_want[1].shape[0] == 41061
    check_all_ways(mhc, wiki.find, wiki_dict, wiki_want, what="wiki lines")


def test_wiki_as_one_stream(mhc, wiki_data, tokens):
    pats = tokens[::8]
    assert len(pats) == 458
    hits = find_ref.find_hits([wiki_data], pats)
    assert len(hits) == 7678 and find_ref.straddles(hits, 256) == 124
    b = Packed(mhc, [wiki_data], 256)
    check_all_ways(mhc, b.find, mhc.Dict(pats), find_ref.hit_arrays(hits, 1), what="one stream")


# ---- 3: seams ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [256, 1024])
def test_seams_255_byte_pattern_at_every_offset_behind_a_boundary(mhc, chunk):
    pattern = bytes(range(1, 256))
    assert len(pattern) == mhc.DICT_MAX_LEN
    # its last byte and its last 254 bytes ride along: a tail meets outputs with out_len <= t in a state of depth > t
    pats = [pattern, pattern[-1:], pattern[-254:]]
    msgs = []
    for k in range(255):                                       # the long pattern ends k bytes behind every chunk boundary
        m = bytearray(5000)                                    # (zeros: no byte of the pattern)
        for edge in range(chunk, 5000 - 255, chunk):
            m[edge + k - 255:edge + k] = pattern
        msgs.append(bytes(m))
    hits = find_ref.find_hits(msgs, pats)
    per = len(range(chunk, 5000 - 255, chunk))
    assert len(hits) == 3 * 255 * per
    assert sum(1 for h in hits if h[3] == 0) == 255 * per      # none lost, none twice
    assert find_ref.straddles([h for h in hits if h[3] == 0], chunk) == 254 * per
    assert find_ref.straddles([h for h in hits if h[3] == 2], chunk) == 253 * per
    b = Packed(mhc, msgs, chunk)
    check_all_ways(mhc, b.find, mhc.Dict(pats), find_ref.hit_arrays(hits, 255), what="seams")


# ---- 4: many hits per end ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def runs():
    rng = np.random.default_rng(5)
    text = bytes(rng.choice(np.frombuffer(b"abcx", dtype=np.uint8), size=6000))
    msgs = [b"a" * 6000, text, b"a" * 300, text[::-1], b"abcab" * 700]
    fam = find_ref.find_hits(msgs, A_FAMILY)
    assert sum(1 for h in fam if h[0] == 0) == sum(min(e, 255) for e in range(1, 6001)) == 1497615
    suf = find_ref.find_hits(msgs, SUFFIXES)
    ends = {}
    for i, _, e, j in suf:
        ends.setdefault((i, e), []).append(j)
    assert any(len(v) >= 4 for v in ends.values()) and find_ref.straddles(suf, 1024) >= 5
    return msgs, find_ref.hit_arrays(fam, len(msgs)), find_ref.hit_arrays(suf, len(msgs))


@pytest.mark.parametrize("chunk", [256, 1024])
def test_many_hits_per_end(mhc, runs, chunk):
    msgs, fam, suf = runs
    b = Packed(mhc, msgs, chunk)
    d = mhc.Dict(A_FAMILY)
    assert d.states == 256
    check_all_ways(mhc, b.find, d, fam, what="a-family")       # up to 255 records per end, in pattern order
    check_all_ways(mhc, b.find, mhc.Dict(SUFFIXES), suf, what="suffixes")


# ---- 5: model kinds ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kinds(wiki_lines, tokens):
    msgs, pats = wiki_lines[:400], tokens[::8]
    hits = find_ref.find_hits(msgs, pats)
    assert len(hits) > 1000
    return msgs, pats, find_ref.hit_arrays(hits, len(msgs))


def test_per_stream_models_and_a_picked_bank(mhc, kinds):
    msgs, pats, want = kinds
    d = mhc.Dict(pats)
    ms = mhc.ModelSet.train(msgs, order=1)
    payload, out_off, nbits, idx, in_off, rc = ms.encode(msgs, chunk_symbols=256)
    assert rc == mhc.MH_OK

    def each(dd, indexed, **kw):
        ix = dict(sym_off=in_off, index=idx, chunk_symbols=256) if indexed else {}
        return ms.find_dict(dd, payload, out_off, nbits, **ix, **kw)
    check_all_ways(mhc, each, d, want, what="each")
    bank, choice, _ = mhc.ModelSet.train_bank(msgs, 4, order=1)
    bpl, boff, bnb, bidx, bin_off = mhc.encode_bank(bank, msgs, choice, chunk_symbols=1024)
    view = bank.pick(choice)

    def picked(dd, indexed, **kw):
        ix = dict(sym_off=bin_off, index=bidx, chunk_symbols=1024) if indexed else {}
        return view.find_dict(dd, bpl, boff, bnb, **ix, **kw)
    check_all_ways(mhc, picked, d, want, what="bank view")
    wrong = mhc.ModelSet.train(msgs[:10], order=1)
    with pytest.raises(mhc.MhError) as e:                       # n_streams != the set's size
        wrong.find_dict(d, payload, out_off, nbits, count_only=True)
    assert e.value.status == mhc.MH_ERR_ARG


@pytest.mark.parametrize("order", [0, 2])
def test_shared_models_of_order_0_and_2(mhc, kinds, order):
    msgs, pats, want = kinds
    d = mhc.Dict(pats)
    b = Packed(mhc, msgs, 256, order=order)
    check_all_ways(mhc, b.find, d, want, what="order %d" % order)
    # each call refuses the other family's model before any launch
    wrong = b.model.dev_find_dict_batch if order == 2 else b.model.dev_find_dict_batch_o2
    wrong_host = b.model.find_dict_batch if order == 2 else b.model.find_dict_batch_o2
    for indexed in (True, False):
        with pytest.raises(mhc.MhError) as e:
            wrong(d, b.payload, b.pay_off, b.nbits, count_only=True, **b.kw(indexed))
        assert e.value.status == mhc.MH_ERR_ARG
        with pytest.raises(mhc.MhError) as e:
            wrong_host(d, b.payload, b.pay_off, b.nbits, **b.kw(indexed))
        assert e.value.status == mhc.MH_ERR_ARG


# ---- 6: contract checks --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indexed", [True, False])
def test_hit_cap(mhc, wiki, wiki_dict, wiki_want, indexed):
    off, wrec, wpat = wiki_want
    total = 41061
    for cap, want_rc in ((0, mhc.MH_ERR_CAPACITY), (total - 1, mhc.MH_ERR_CAPACITY), (total, mhc.MH_OK), (7, mhc.MH_ERR_CAPACITY)):
        ho, rec, pat, st, rc = wiki.find(wiki_dict, indexed, hit_cap=cap)   # (the wrapper asserts the guard words and the records >= cap)
        assert rc == want_rc and (st == mhc.MH_OK).all(), cap
        assert np.array_equal(ho, off), cap                          # complete whether or not the records fit
        assert np.array_equal(rec, wrec[:cap]) and np.array_equal(pat, wpat[:cap]), cap
        ho, rec, pat, st, rc = wiki.model.find_dict_batch(wiki_dict, wiki.payload, wiki.pay_off, wiki.nbits, hit_cap=cap, check=False,
                                                          **wiki.kw(indexed))
        assert rc == want_rc and np.array_equal(ho, off) and np.array_equal(rec, wrec[:cap]) and np.array_equal(pat, wpat[:cap]), cap


def test_two_calls_give_identical_buffers(mhc, wiki, wiki_dict):
    for indexed in (True, False):
        a, b = wiki.find(wiki_dict, indexed), wiki.find(wiki_dict, indexed)
        assert a[1].shape[0] == 41061
        for x, y in zip(a[:4], b[:4]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("fold", [False, True])
def test_records_are_lookups(mhc, wiki, tokens, fold):
    pats = [t.upper() for t in tokens[::8]] if fold else tokens[::8]
    d = mhc.Dict(pats, fold=fold)
    want = len(find_ref.find_hits(wiki.msgs, pats, fold=fold))
    assert want > 1000
    for indexed in (True, False):
        ho, rec, pat, st, rc = wiki.find(d, indexed)
        assert rc == mhc.MH_OK and rec.shape[0] == want
        res, lst, lrc = wiki.model.dev_decode_batch_ranges(wiki.payload, wiki.pay_off, wiki.nbits, rec, **wiki.kw(indexed))
        assert lrc == mhc.MH_OK and (lst == mhc.MH_OK).all()
        for r, j in zip(res, pat):
            assert (find_ref.fold_ascii(r) == find_ref.fold_ascii(pats[j])) if fold else (r == pats[j])


def test_wiki_lines_fold(mhc, wiki):
    hits = find_ref.find_hits(wiki.msgs, [b"c++"], fold=True)
    assert len(hits) == 550
    check_all_ways(mhc, wiki.find, mhc.Dict([b"c++"], fold=True), find_ref.hit_arrays(hits, len(wiki.msgs)), what="fold")


def test_stream_boundaries_empty_and_short_streams(mhc):
    msgs = [b"", b"", b"xxxxab", b"cxxxx", b"", b"abc", b"a", b"ab", b"", b"zabcabc", b"", b""]
    pats = [b"abc", b"a", b"abcabcabc"]
    hits = find_ref.find_hits(msgs, pats)
    assert [h for h in hits if h[3] == 0] == [(5, 0, 3, 0), (9, 1, 4, 0), (9, 4, 7, 0)]       # nothing across streams 2 | 3
    assert not [h for h in hits if h[3] == 2]                                                  # longer than every stream
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs * 3 + [bytes(range(256)) * 2], order=1), 1)
    d = mhc.Dict(pats)
    check_all_ways(mhc, Packed(mhc, msgs, 256, model=model).find, d, find_ref.hit_arrays(hits, len(msgs)), what="boundaries")
    none = Packed(mhc, [], 256, model=model)
    check_all_ways(mhc, none.find, d, find_ref.hit_arrays([], 0), what="n_streams == 0")
    ho, rec, pat, st, rc = model.find_dict_batch(d, none.payload, none.pay_off, none.nbits)
    assert ho.tolist() == [0] and rec.size == 0 and rc == mhc.MH_OK
    check_all_ways(mhc, Packed(mhc, [b"", b"", b""], 256, model=model).find, d, find_ref.hit_arrays([], 3), what="empty streams only")
    short = [b"ab", b"a", b"abc", b"ab"]                       # shorter than every pattern (and pairs the model has codes for)
    long_only = mhc.Dict([b"abca", b"abab"])
    check_all_ways(mhc, Packed(mhc, short, 256, model=model).find, long_only, find_ref.hit_arrays([], 4), what="short streams")


def test_bad_offsets_stop_the_call(mhc):
    b = Packed(mhc, [zipf(3000, 1), zipf(2000, 2)], 256)
    d = mhc.Dict([b"\x00", b"\x00\x01"])
    po = b.pay_off.copy()
    po[1] = po[2] + np.uint64(1)                                               # decreasing
    ho, rec, pat, st, rc = b.model.dev_find_dict_batch(d, b.payload, po, b.nbits, count_only=True, **b.kw(True))
    assert rc == mhc.MH_ERR_ARG and ho.tolist() == [0, 0, 0]


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
    pats = [msgs[0][100:102], msgs[2][500:503], msgs[4][7:9], msgs[1][10:12], msgs[3][20:22]]
    b = Packed(mhc, msgs, chunk)
    d = mhc.Dict(pats)
    hits = find_ref.find_hits(msgs, pats)
    assert all(any(h[0] == i for h in hits) for i in range(5))
    check(mhc, b.find(d, indexed), find_ref.hit_arrays(hits, 5), "undamaged")
    streams = [bytes(b.payload[int(b.pay_off[i]):int(b.pay_off[i + 1])]) for i in range(5)]
    failed = 0
    for at in (0, 2, 4):
        pl, nb = streams[at], int(b.nbits[at])
        base = int(mhc.lib().mh_batch_index_base(int(b.sym_off[at]), at, chunk))
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
            ho, rec, pat, st, rc = b.model.dev_find_dict_batch(d, payload, pay_off, nbs, **kw)
            what = "stream %d %s indexed=%s" % (at, name, indexed)
            assert st.tolist() == want_st.tolist(), what
            assert (rc == mhc.MH_OK) == (want_rc == mhc.MH_OK), what
            assert all(int(s) == mhc.MH_OK for k, s in enumerate(st) if k != at), what
            if st[at] != mhc.MH_OK:
                failed += 1
                off, wrec, wpat = find_ref.hit_arrays([h for h in hits if h[0] != at], 5)     # zero hits of the failed stream
                assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat), what
            else:
                others = [h for h in hits if h[0] != at]
                got = [(int(i), int(x), int(y), int(j)) for (i, x, y), j in zip(rec, pat) if int(i) != at]
                assert got == others, what
    assert failed >= 12                                                        # the damages did fail streams


# ---- 7: workspace and stream ---------------------------------------------------------------------------------------------------

def raw_call(mhc, torch, b, d, want, stream, blocker_cycles=0):
    """mh_dev_find_dict_batch count-only and with records, indexed, on `stream`, every output and the workspace prefilled with
    0xFF; behind a torch.cuda._sleep blocker when asked.  Returns whether the blocker's event was still pending after the calls
    were enqueued."""
    l = mhc.lib()
    off, wrec, wpat = want
    n, k = len(b.msgs), int(off[-1])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def filled(nbytes):
        return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")
    pl = torch.zeros(b.payload.size + 64, dtype=torch.uint8, device="cuda")
    pl[:b.payload.size] = dev(b.payload)
    po, nb, so, idx = dev(b.pay_off.astype(np.uint64)), dev(np.asarray(b.nbits, dtype=np.uint64)), dev(b.sym_off.astype(np.uint64)), dev(b.index)
    wsb = l.mh_dev_find_dict_workspace(n, int(b.sym_off[n]), b.chunk)
    ws, ho, rec, pat, st = filled(wsb), filled((n + 1) * 8), filled(k * 24), filled(k * 4), filled(n * 4)
    ho_c = filled((n + 1) * 8)
    torch.cuda.synchronize()
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
    p = lambda t: C.c_void_p(t.data_ptr())
    pending = None
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        if blocker_cycles:
            torch.cuda._sleep(int(blocker_cycles))
            ev = torch.cuda.Event()
            ev.record()
        common = (b.model.handle, d.handle, p(pl), p(po), p(nb), n, int(b.pay_off[n]), 0x20, p(so), int(b.sym_off[n]), p(idx), b.chunk)
        rc1 = l.mh_dev_find_dict_batch(*common, p(ho_c), None, None, 0, p(st), p(ws), wsb, sp)
        rc2 = l.mh_dev_find_dict_batch(*common, p(ho), p(rec), p(pat), k, p(st), p(ws), wsb, sp)
        if blocker_cycles:
            pending = not ev.query()
    assert rc1 == mhc.MH_OK and rc2 == mhc.MH_OK
    assert l.mh_dev_status(p(ws), sp) == mhc.MH_OK
    torch.cuda.synchronize()
    assert np.array_equal(ho_c.cpu().numpy().view(np.uint64)[:n + 1], off)
    assert np.array_equal(ho.cpu().numpy().view(np.uint64)[:n + 1], off)
    assert np.array_equal(rec.cpu().numpy().view(np.uint64)[:3 * k].reshape(-1, 3), wrec)
    assert np.array_equal(pat.cpu().numpy().view(np.uint32)[:k], wpat)
    assert (st.cpu().numpy().view(np.int32)[:n] == mhc.MH_OK).all()
    return pending


def test_prefilled_workspace_and_a_blocked_stream(mhc, kinds):
    import torch
    msgs, pats, want = kinds
    b = Packed(mhc, msgs, 256)
    d = mhc.Dict(pats)
    raw_call(mhc, torch, b, d, want, None)                      # 0xFF everywhere, default stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                             # cycles per millisecond of _sleep, measured once
        torch.cuda._sleep(1_000_000)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20_000_000)
        e.record()
    e.synchronize()
    per_ms = 20_000_000 / a.elapsed_time(e)
    pending = raw_call(mhc, torch, b, d, want, stream, blocker_cycles=100 * per_ms)
    print("torch.cuda._sleep: %.0f cycles per ms; blocker of 100 ms still pending after the enqueue: %s" % (per_ms, pending))
    assert pending, "a call waited for its stream (or the enqueue took longer than the 100 ms blocker)"


# ---- 8: host forms and the CLI -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,size", [(1, 1_700_000), (2, 2_100_000)])
def test_host_form_serves_a_stream_over_the_walk_cap(mhc, order, size):
    big = zipf(size, 3)
    msgs = [big[:3000], big, big[5000:9000]]
    pats = [big[1000:1002], big[5000:5003], big[70000:70004], big[1000:1002] + b"\xfe\xfd"]
    hits = find_ref.find_hits(msgs, pats)
    assert len(hits) > 500 and all(any(h[0] == i for h in hits) for i in range(3))
    want = find_ref.hit_arrays(hits, 3)
    b = Packed(mhc, msgs, 1024, order=order)
    assert int(b.nbits[1]) > mhc.BATCH_WALK_MAX_BITS > int(b.nbits[1]) * 0.7        # just over the cap
    d = mhc.Dict(pats)
    check(mhc, b.find(d, True), want, "indexed")
    # index-free the long stream is refused by the device call alone ...
    ho, rec, pat, st, rc = b.find(d, False)
    assert st.tolist() == [mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_OK] and rc == mhc.MH_ERR_ARG
    off, wrec, wpat = find_ref.hit_arrays([h for h in hits if h[0] != 1], 3)
    assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat)
    # ... and served by the host form
    host = b.model.find_dict_batch_o2 if order == 2 else b.model.find_dict_batch
    for kw in ({}, b.kw(True)):
        ho, rec, pat, st, rc = host(d, b.payload, b.pay_off, b.nbits, **kw)
        assert rc == mhc.MH_OK and st.tolist() == [mhc.MH_OK] * 3
        assert np.array_equal(ho, want[0]) and np.array_equal(rec, want[1]) and np.array_equal(pat, want[2])
    ho, rec, pat, st, rc = host(d, b.payload, b.pay_off, b.nbits, hit_cap=10, check=False)
    assert rc == mhc.MH_ERR_CAPACITY and np.array_equal(ho, want[0]) and np.array_equal(rec, want[1][:10]) and np.array_equal(pat, want[2][:10])


def test_cli_find_file(mhc, tmp_path, tokens):
    src = os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.html")
    data = open(src, "rb").read()
    cm, table, idx, words = (str(tmp_path / n) for n in ("in.cm", "table", "f.idx", "words"))
    r = subprocess.run([CLI, src, "-o", cm, "-d", table, "--index", idx, "--chunk", "256"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pats = tokens[::8] + [b"</span>", b"C++", b"a href=\"/wiki"]
    open(words, "wb").write(b"\n".join(pats[:100]) + b"\n\n\n" + b"\n".join(pats[100:]))      # empty lines, no LF at the end
    find = [CLI, cm, "-x", "-e", table, "--index", idx]
    r = subprocess.run(find + ["--find-file", words], capture_output=True, timeout=300)
    hits = find_ref.find_hits([data], pats)
    assert len(hits) > 7678 + 892 + 520
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == ["%d %d" % (j, b) for _, b, _, j in hits]
    open(words, "wb").write(b"c++\ntemplate\n")
    r = subprocess.run(find + ["--find-file", words, "--find-fold"], capture_output=True, timeout=300)
    want = find_ref.find_hits([data], [b"c++", b"template"], fold=True)
    assert len(want) > 550 and r.returncode == 0 and r.stdout.decode().splitlines() == ["%d %d" % (j, b) for _, b, _, j in want]
    open(words, "wb").write(b"zzzz\nqqqqqqqq\n")
    r = subprocess.run(find + ["--find-file", words, "-o", str(tmp_path / "out")], capture_output=True, timeout=300)
    assert r.returncode == 1 and r.stdout == b"" and not os.path.exists(str(tmp_path / "out"))
    r = subprocess.run(find + ["--find-file", words, "--find", "zzzz"], capture_output=True, timeout=300)
    assert r.returncode == 1 and b"--find-file cannot be combined with --find" in r.stderr
    r = subprocess.run(find + ["--find-file", words, "--order2"], capture_output=True, timeout=300)
    assert r.returncode == 1 and b"--order2" in r.stderr
