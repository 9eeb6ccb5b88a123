"""Order-2 models in batch search, coded histogram and re-coding on the GPU (include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING").
The references are tests/find_ref.py on the original messages, the batch encoders (mh_dev_encode_batch / _o2 under the
destination model) and the batch histograms of the original messages; verdicts are those of the batch decoders on the same
arguments.  Every order-2 model is built once per module; the device-call wrappers put guards around every output."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import bench
import find_ref
from conftest import golden

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1025, 5000]
CHUNKS = (256, 1024)


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


def text(n, seed):
    return bench.lorem_block(max(n, 1), seed)[:n]


NEEDLE = b"GPU-Huffman!"                      # planted so that it straddles the 256-symbol seam at every offset 1..len-1


def make_ragged():
    msgs = []
    for k, n in enumerate(LENS):
        msgs += [text(n, 10 + k), zipf(n, 40 + k)]
    for off in range(1, len(NEEDLE)):           # NEEDLE's byte `off` is symbol 256
        t = bytearray(text(700, 70 + off))
        t[256 - off:256 - off + len(NEEDLE)] = NEEDLE
        msgs.append(bytes(t))
    msgs.append(text(300, 5) + b"e" * 64 + text(300, 6))
    return msgs


class World:
    """The ragged batch, its models of every order (trained on it: every pair has a code) and its coded forms."""

    def __init__(self, mhc, msgs, prev0=0x20):
        self.mhc, self.msgs, self.prev0, self.n = mhc, msgs, prev0, len(msgs)
        self.h = {0: mhc.histogram_o1_batch(msgs, prev0=prev0, order=0), 1: mhc.histogram_o1_batch(msgs, prev0=prev0, order=1),
                  2: mhc.histogram_o2_batch(msgs, prev0=prev0)}
        self.model = {o: mhc.Model.from_counts(self.h[o], o) for o in (0, 1, 2)}
        self.coded = {}

    def enc(self, order, chunk, model=None):
        key = (order, chunk, id(model))
        if key not in self.coded:
            m = model or self.model[order]
            fn = m.encode_batch_o2 if order == 2 else m.encode_batch
            self.coded[key] = fn(self.msgs, prev0=self.prev0, chunk_symbols=chunk)
        return self.coded[key]

    def kw(self, order, chunk, indexed):
        pay, off, nb, idx, so = self.enc(order, chunk)
        kw = dict(prev0=self.prev0, chunk_symbols=chunk)
        if indexed:
            kw.update(sym_off=so, index=idx)
        return (pay, off, nb), kw


@pytest.fixture(scope="module")
def world(mhc):
    return World(mhc, make_ragged())


def slices(idx, sym_off, chunk, only=None):
    out = []
    for i in range(len(sym_off) - 1):
        if only is not None and i not in only:
            continue
        b = int(sym_off[i]) // chunk + i
        out.append(np.asarray(idx[b:b + (int(sym_off[i + 1] - sym_off[i]) + chunk - 1) // chunk], dtype=np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------- search

PATTERN_SETS = {
    "one_byte": ([b"e"], False),
    "seam": ([NEEDLE], False),
    "len64": ([b"e" * 64], False),
    "fifteen": ([b"the ", b"and", b"lor", b"ip", b"um", b"dolor", b"sit", b"amet", b"cons", b"ect", b"etur", b"adip", b"isci", b"elit", b"sed do"
                 b" eiusmod "], False),
    "fold": ([b"gpu-HUFFMAN", b"LOREM"], True),
}


@pytest.mark.parametrize("name", sorted(PATTERN_SETS))
def test_search_equals_reference(mhc, world, name):
    pats, fold = PATTERN_SETS[name]
    if name == "fifteen":
        assert len(pats) == 15 and sum(len(p) for p in pats) == 64
    ps = mhc.PatternSet(pats, fold=fold)
    want = find_ref.find_hits(world.msgs, pats, fold=fold)
    w_off, w_rec, w_pat = find_ref.hit_arrays(want, world.n)
    assert len(want) > 0
    if name == "seam":
        assert find_ref.straddles(want, 256) == len(NEEDLE) - 1
    m2 = world.model[2]
    for chunk, indexed in [(256, True), (1024, True), (256, False)]:
        src, kw = world.kw(2, chunk, indexed)
        ho, rec, pat, st, rc = m2.dev_find_batch_o2(ps, *src, **kw)
        tag = (name, chunk, indexed)
        assert rc == mhc.MH_OK and not st.any(), tag
        assert np.array_equal(ho, w_off) and np.array_equal(rec, w_rec) and np.array_equal(pat, w_pat), tag
        ho_c, _, _, st_c, rc_c = m2.dev_find_batch_o2(ps, *src, count_only=True, **kw)
        assert rc_c == mhc.MH_OK and np.array_equal(ho_c, w_off), tag
        cap = len(want) - 1
        ho_s, rec_s, pat_s, _, rc_s = m2.dev_find_batch_o2(ps, *src, hit_cap=cap, **kw)      # (the wrapper asserts nothing is written past cap)
        assert rc_s == mhc.MH_ERR_CAPACITY and np.array_equal(ho_s, w_off), tag
        assert np.array_equal(rec_s, w_rec[:cap]) and np.array_equal(pat_s, w_pat[:cap]), tag
    if name == "seam":
        (pay, off, nb), kw = world.kw(2, 256, True)
        outs, st, rc = m2.dev_decode_batch_o2_ranges(pay, off, nb, w_rec, **kw)[:3]
        assert rc == mhc.MH_OK and not np.asarray(st).any()
        assert all(bytes(o) == NEEDLE for o in outs)


def check_all_ways_o2(mhc, msgs, chunk, patterns, hits, what=""):
    """test_gpu_find.check_all_ways for order 2: the messages coded by mh_encode_batch_o2 (the host form over
    mh_dev_encode_batch_o2) under an order-2 model trained on them; mh_dev_find_batch_o2 indexed and index-free,
    count-only and with records, against the reference's hits."""
    w = World(mhc, msgs)
    ps = mhc.PatternSet(patterns)
    off, wrec, wpat = find_ref.hit_arrays(hits, w.n)
    for indexed in (True, False):
        src, kw = w.kw(2, chunk, indexed)
        tag = (what, chunk, indexed)
        ho, rec, pat, st, rc = w.model[2].dev_find_batch_o2(ps, *src, count_only=True, **kw)
        assert rc == mhc.MH_OK and (st == mhc.MH_OK).all() and np.array_equal(ho, off) and rec.size == 0, tag
        ho, rec, pat, st, rc = w.model[2].dev_find_batch_o2(ps, *src, **kw)
        assert rc == mhc.MH_OK and (st == mhc.MH_OK).all(), (tag, rc, np.unique(st))
        assert np.array_equal(ho, off) and np.array_equal(rec, wrec) and np.array_equal(pat, wpat), tag


@pytest.mark.parametrize("chunk", CHUNKS)
def test_seams_64_byte_pattern_at_every_offset_behind_a_boundary(mhc, chunk):
    """The order-2 counterpart of test_gpu_find's test: the seam rule (a hit spans at most two chunks, the tail takes no
    new starts) at the smallest shape where it can go wrong, a 64-position automaton against chunks of 256 symbols."""
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
    check_all_ways_o2(mhc, msgs, chunk, [pattern], hits, what="seams")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_seams_suffix_patterns_and_runs(mhc, chunk):
    """The order-2 counterpart of test_gpu_find's test: a pattern, its suffixes and a duplicate end at the same symbol, on
    both sides of a seam; a run of one byte matches at every position."""
    rng = np.random.default_rng(5)
    text = bytes(rng.choice(np.frombuffer(b"abcx", dtype=np.uint8), size=6000))
    pats = [b"abcab", b"cab", b"b", b"abcab", b"ab"]          # a pattern, its suffixes, a duplicate: equal ends, all pattern numbers
    msgs = [text, b"a" * 300, text[::-1], b"abcab" * 700]
    hits = find_ref.find_hits(msgs, pats)
    ends = {}
    for i, _, e, j in hits:
        ends.setdefault((i, e), []).append(j)
    assert any(len(v) >= 4 for v in ends.values()) and find_ref.straddles(hits, chunk) >= 5
    check_all_ways_o2(mhc, msgs, chunk, pats, hits, what="suffixes")
    run = find_ref.find_hits(msgs, [b"aaaa"])
    assert len([h for h in run if h[0] == 1]) == 297
    check_all_ways_o2(mhc, msgs, chunk, [b"aaaa"], run, what="aaaa")


# ---------------------------------------------------------------------------------------------------- re-code

def check_recode(mhc, w, so, do, dst=None, what=""):
    """Indexed (both chunks) and index-free re-code from order `so` to `dst` (order do) against the batch encoder under dst."""
    dst = dst or w.model[do]
    src_model = w.model[so]
    for chunk in CHUNKS:
        fn = dst.encode_batch_o2 if do == 2 else dst.encode_batch
        e_pay, e_off, e_nb, e_idx, e_so = fn(w.msgs, prev0=w.prev0, chunk_symbols=chunk)
        for indexed in (True, False):
            if not indexed and chunk != 256:
                continue
            src, kw = w.kw(so, chunk, indexed)
            got = src_model.dev_recode_batch_o2(dst, *src, **kw)
            tag = (what, so, do, chunk, indexed)
            assert got["rc"] == mhc.MH_OK and not got["status"].any(), tag
            assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb), tag
            assert np.array_equal(got["payload"], e_pay), tag
            assert np.array_equal(got["sym_off"], e_so), tag
            assert np.array_equal(slices(got["index"], e_so, chunk), slices(e_idx, e_so, chunk)), tag
            count = src_model.dev_recode_batch_o2(dst, *src, count_only=True, **kw)
            assert np.array_equal(count["out_off"], got["out_off"]) and np.array_equal(count["dropped"], got["dropped"]), tag
    return got, (e_pay, e_off, e_nb, e_idx, e_so)


@pytest.mark.parametrize("so,do", [(0, 2), (1, 2), (2, 0), (2, 1), (2, 2)])
def test_recode_equals_the_encoder(mhc, world, so, do):
    got, (e_pay, e_off, e_nb, e_idx, e_so) = check_recode(mhc, world, so, do)
    assert not got["dropped"].any()
    dst = world.model[do]
    dec = dst.decode_batch_o2 if do == 2 else dst.decode_batch
    back, _, st = dec(got["payload"], got["out_off"], got["nbits"], prev0=world.prev0)
    assert back == b"".join(world.msgs) and not np.asarray(st).any()


def test_short_streams_under_another_prev0(mhc):
    msgs = [b"", b"a", b"ab", b"z", b"zz", b"", b"abc", text(600, 3), b"a"]
    w = World(mhc, msgs, prev0=0x61)                                   # 'a': (prev0, prev0) and (prev0, s0) are live contexts
    for so, do in [(0, 2), (1, 2), (2, 1), (2, 2)]:
        check_recode(mhc, w, so, do, what="prev0")
    for order, so in [(2, 1), (2, 0), (1, 2), (0, 2), (2, 2)]:
        src, kw = w.kw(so, 256, True)
        counts, st, rc = w.model[so].dev_histogram_coded_o2(order, *src, **kw)
        assert rc == mhc.MH_OK and np.array_equal(counts, w.h[order]), (order, so)


def test_codes_over_56_bits(mhc):
    fib = [1, 1]
    while len(fib) < 62:
        fib.append(fib[-1] + fib[-2])
    syms = list(range(62))
    counts = np.zeros(1 << 24, dtype=np.uint64)
    for b2 in syms + [0x20]:
        for b1 in syms + [0x20]:
            ctx = (b2 << 8) | b1
            counts[(ctx << 8):(ctx << 8) + 62] = fib[::-1] if (b1 + b2) % 2 else fib
    dst = mhc.Model.from_counts(counts, 2)
    assert dst.max_code_len > 56
    rng = np.random.default_rng(16)
    msgs = [bytes(rng.integers(0, 62, int(k)).astype(np.uint8)) for k in (0, 1, 2, 17, 1000, 5000, 3)]
    msgs.append(bytes([0] * 300 + [61] * 300))
    w = World(mhc, msgs)
    got, _ = check_recode(mhc, w, 1, 2, dst=dst, what="fib")
    assert not got["dropped"].any()


def test_zipf_under_a_text_trained_model_drops_what_the_counts_lack(mhc, world):
    tc = mhc.histogram_o2_batch([text(1 << 18, 17)])
    dst = mhc.Model.from_counts(tc, 2)
    msgs = [zipf(k, 18 + k) for k in (1, 2, 100, 257, 1025, 3000)] + [text(500, 19) + zipf(500, 20) + text(500, 21)]
    w = World(mhc, msgs)
    got, _ = check_recode(mhc, w, 1, 2, dst=dst, what="drops")
    want = []
    for m in msgs:
        d = np.frombuffer(m, dtype=np.uint8).astype(np.int64)
        p1 = np.concatenate([[0x20], d[:-1]])[:d.size]
        p2 = np.concatenate([[0x20, 0x20], d[:-2]])[:d.size]
        want.append(int((tc[((p2 << 8 | p1) << 8) | d] == 0).sum()))
    assert got["dropped"].tolist() == want and sum(want) > 0


# ---------------------------------------------------------------------------------------------------- coded histogram

def test_coded_histogram_equals_the_batch_histograms(mhc, world):
    for order, so in [(2, 1), (2, 0), (0, 2), (1, 2), (2, 2)]:
        for chunk, indexed in [(256, True), (1024, True), (256, False)]:
            src, kw = world.kw(so, chunk, indexed)
            counts, st, rc = world.model[so].dev_histogram_coded_o2(order, *src, **kw)
            assert rc == mhc.MH_OK and not st.any(), (order, so, chunk, indexed)
            assert np.array_equal(counts, world.h[order]), (order, so, chunk, indexed)
    src, kw = world.kw(1, 256, True)
    assert np.array_equal(mhc.histogram_coded_batch_o2(world.model[1], 2, *src, **kw), world.h[2])


# ---------------------------------------------------------------------------------------------------- damage

def damaged(w, order, chunk, kind):
    """(payload, pay_off, nbits, index, sym_off, hit stream) of the ragged batch with one stream damaged."""
    pay, off, nb, idx, so = (np.array(a, copy=True) for a in w.enc(order, chunk))
    i = max(range(w.n), key=lambda k: len(w.msgs[k]))                  # the 5 000-symbol text stream: several chunks
    if kind == "cut":
        nb[i] -= np.uint64(3)
    elif kind == "extended":                                           # one more byte behind the stream's payload, counted in nbits
        pay = np.concatenate([pay[:int(off[i + 1])], np.array([0x55], dtype=np.uint8), pay[int(off[i + 1]):]])
        off[i + 1:] += np.uint64(1)
        nb[i] += np.uint64(8)
    elif kind == "flip":
        pay[int(off[i]) + int(nb[i]) // 16] ^= 0x10
    elif kind == "entry":
        idx[int(so[i]) // chunk + i + 1] += np.uint64(1)
    elif kind == "nbits_beyond":
        nb[i] = np.uint64((int(off[i + 1]) - int(off[i])) * 8 + 1)
    return pay, off, nb, idx, so, i


def dev_decode(mhc, model, o2, pay, off, nb, prev0, chunk_symbols, sym_off=None, index=None):
    """One mh_dev_decode_batch / _o2 call: (the decoded message of every stream that passed, b"" for the others; status[n])."""
    lib = mhc.lib()
    n = len(off) - 1
    fn, wsf = (lib.mh_dev_decode_batch_o2, lib.mh_dev_decode_batch_o2_workspace) if o2 else (lib.mh_dev_decode_batch, lib.mh_dev_decode_batch_workspace)
    pay, off, nb = (np.ascontiguousarray(a) for a in (pay, off, nb))
    indexed = index is not None
    cap = int(sym_off[n]) if indexed else sum(int(b) for b in nb) // max(model.min_code_len, 1) + 64
    d_pl, d_po, d_nb = mhc.DeviceBuffer(pay.size + 64, pay), mhc.DeviceBuffer(off.nbytes, off), mhc.DeviceBuffer(nb.nbytes, nb)
    d_o, d_st = mhc.DeviceBuffer(cap + 64), mhc.DeviceBuffer(n * 4)
    d_so = mhc.DeviceBuffer((n + 1) * 8, np.ascontiguousarray(sym_off, dtype=np.uint64) if indexed else None)
    d_idx = mhc.DeviceBuffer(max(index.nbytes, 8), np.ascontiguousarray(index)) if indexed else None
    ws = wsf(n)
    d_ws = mhc.DeviceBuffer(ws)
    assert fn(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(off[n]), prev0, d_o.ptr, cap, d_so.ptr, int(sym_off[n]) if indexed else 0,
              d_idx.ptr if indexed else None, chunk_symbols, d_st.ptr, d_ws.ptr, ws, None) == 0
    st, so, out = d_st.download(np.int32)[:n], d_so.download(np.uint64), d_o.download(np.uint8)
    return [out[int(so[k]):int(so[k + 1])].tobytes() if st[k] == 0 else b"" for k in range(n)], st


@pytest.mark.parametrize("kind", ["cut", "extended", "flip", "entry", "nbits_beyond"])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("so", [0, 1, 2])
def test_damaged_streams_get_the_decoders_verdicts(mhc, world, so, chunk, kind):
    w = world
    src_model = w.model[so]
    dst = w.model[1 if so == 2 else 2]
    ps = mhc.PatternSet([b"e", NEEDLE])
    clean = src_model.dev_recode_batch_o2(dst, *w.kw(so, chunk, True)[0], **w.kw(so, chunk, True)[1])
    for indexed in (True, False):
        if kind == "entry" and not indexed:
            continue
        pay, off, nb, idx, sym, hit = damaged(w, so, chunk, kind)
        kw = dict(prev0=w.prev0, chunk_symbols=chunk)
        if indexed:
            kw.update(sym_off=sym, index=idx)
        good, want = dev_decode(mhc, src_model, so == 2, pay, off, nb, **kw)      # what the batch decoder makes of the same arguments
        if kind == "nbits_beyond":                                      # (the other kinds: whatever the decoder says)
            assert want[hit] == mhc.MH_ERR_ARG, (kind, indexed)
        assert all(good[k] == w.msgs[k] for k in range(w.n) if k != hit), (kind, indexed)
        got = src_model.dev_recode_batch_o2(dst, pay, off, nb, **kw)
        assert np.array_equal(got["status"], want), (kind, indexed)
        for k in range(w.n):
            a, b = int(got["out_off"][k]), int(got["out_off"][k + 1])
            if want[k] != mhc.MH_OK:
                assert a == b and got["nbits"][k] == 0 and got["dropped"][k] == 0
            elif k != hit:                                              # (a damaged stream that still decodes is another message)
                ca = int(clean["out_off"][k])
                assert got["nbits"][k] == clean["nbits"][k] and np.array_equal(got["payload"][a:b], clean["payload"][ca:ca + b - a])
        order = 1 if so == 2 else 2
        counts, st, _ = src_model.dev_histogram_coded_o2(order, pay, off, nb, **kw)
        assert np.array_equal(st, want), (kind, indexed)
        ref = mhc.histogram_o2_batch(good, prev0=w.prev0) if order == 2 else mhc.histogram_o1_batch(good, prev0=w.prev0, order=1)
        assert np.array_equal(counts, ref), (kind, indexed)
        if so == 2:
            ho, rec, pat, st, _ = src_model.dev_find_batch_o2(ps, pay, off, nb, **kw)
            assert np.array_equal(st, want), (kind, indexed)
            w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(good, [b"e", NEEDLE]), w.n)
            assert np.array_equal(ho, w_off) and np.array_equal(rec, w_rec) and np.array_equal(pat, w_pat), (kind, indexed)


@pytest.mark.parametrize("so,order", [(1, 2), (0, 2), (2, 1), (2, 2)])
def test_histogram_without_a_truncated_and_a_flipped_stream(mhc, world, so, order):
    """One stream truncated and another with a flipped bit in the same batch: the counts are those of the messages the
    batch decoder still gives, indexed and index-free."""
    w, chunk = world, 256
    by_len = sorted(range(w.n), key=lambda k: len(w.msgs[k]))
    cut, flip = by_len[-1], by_len[-2]
    for indexed in (True, False):
        pay, off, nb, idx, sym = (np.array(a, copy=True) for a in w.enc(so, chunk))
        nb[cut] -= np.uint64(5)
        pay[int(off[flip]) + int(nb[flip]) // 16] ^= 0x08
        kw = dict(prev0=w.prev0, chunk_symbols=chunk)
        if indexed:
            kw.update(sym_off=sym, index=idx)
        good, want = dev_decode(mhc, w.model[so], so == 2, pay, off, nb, **kw)
        if indexed:
            assert want[cut] != mhc.MH_OK and want[flip] != mhc.MH_OK           # a chunk must end exactly at the next entry
        counts, st, _ = w.model[so].dev_histogram_coded_o2(order, pay, off, nb, **kw)
        assert np.array_equal(st, want), (so, order, indexed)
        ref = mhc.histogram_o2_batch(good, prev0=w.prev0) if order == 2 else mhc.histogram_o1_batch(good, prev0=w.prev0, order=order)
        assert np.array_equal(counts, ref), (so, order, indexed)


# ---------------------------------------------------------------------------------------------------- capacity

def test_recode_capacity_one_byte_short(mhc, world):
    for so, do in [(1, 2), (2, 1)]:
        src, kw = world.kw(so, 256, True)
        full = world.model[so].dev_recode_batch_o2(world.model[do], *src, **kw)
        short = world.model[so].dev_recode_batch_o2(world.model[do], *src, cap=int(full["out_off"][-1]) - 1, **kw)   # (guards checked inside)
        assert short["rc"] == mhc.MH_ERR_CAPACITY and short["payload"].size == 0
        assert np.array_equal(short["out_off"], full["out_off"]) and np.array_equal(short["nbits"], full["nbits"])


# ---------------------------------------------------------------------------------------------------- host forms

def test_host_forms_take_a_stream_over_the_walk_cap(mhc):
    big = np.random.default_rng(9).integers(0, 256, 1 << 21, dtype=np.uint8).tobytes()
    big = big[:1000] + NEEDLE + big[1000:]
    msgs = [b"small one " + NEEDLE, big, text(5000, 1)]
    w = World(mhc, msgs)
    ps = mhc.PatternSet([NEEDLE])
    want = find_ref.hit_arrays(find_ref.find_hits(msgs, [NEEDLE]), 3)
    for so, do in [(2, 1), (1, 2)]:
        pay, off, nb, _, in_off = w.enc(so, 1024)
        assert nb[1] > mhc.BATCH_WALK_MAX_BITS
        if so == 2:
            ho, rec, pat, st, rc = w.model[2].find_batch_o2(ps, pay, off, nb)
            assert rc == mhc.MH_OK and not st.any()
            assert np.array_equal(ho, want[0]) and np.array_equal(rec, want[1]) and np.array_equal(pat, want[2])
        # the device calls refuse the long stream as the batch decoders do, and leave its neighbours alone
        _, refused = dev_decode(mhc, w.model[so], so == 2, pay, off, nb, w.prev0, 0)
        refused = refused.tolist()
        assert refused == [mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_OK]
        dev = w.model[so].dev_recode_batch_o2(w.model[do], pay, off, nb, chunk_symbols=1024, want_index=False)
        assert dev["rc"] == mhc.MH_ERR_ARG and dev["status"].tolist() == refused and dev["nbits"][1] == 0
        counts, st, rc = w.model[so].dev_histogram_coded_o2(do, pay, off, nb)
        ref = mhc.histogram_o2_batch([msgs[0], b"", msgs[2]]) if do == 2 else mhc.histogram_o1_batch([msgs[0], b"", msgs[2]])
        assert rc == mhc.MH_ERR_ARG and st.tolist() == refused and np.array_equal(counts, ref)
        if so == 2:
            ho, rec, _, st, rc = w.model[2].dev_find_batch_o2(ps, pay, off, nb)
            assert rc == mhc.MH_ERR_ARG and st.tolist() == refused and ho.tolist() == [0, 1, 1, 1]
        got = w.model[so].recode_batch_o2(w.model[do], pay, off, nb, chunk_symbols=1024)
        e_pay, e_off, e_nb, e_idx, e_so = w.enc(do, 1024)
        assert got["rc"] == mhc.MH_OK and not got["status"].any(), (so, do)
        assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb), (so, do)
        assert np.array_equal(got["payload"], e_pay) and np.array_equal(got["sym_off"], e_so), (so, do)
        assert np.array_equal(slices(got["index"], e_so, 1024), slices(e_idx, e_so, 1024)), (so, do)
        assert not got["dropped"].any()
        short = w.model[so].recode_batch_o2(w.model[do], pay, off, nb, chunk_symbols=1024, cap=int(e_off[-1]) - 1, check=False)
        assert short["rc"] == mhc.MH_ERR_CAPACITY and np.array_equal(short["out_off"], e_off) and np.array_equal(short["nbits"], e_nb), (so, do)


def test_host_find_splices_a_long_stream_under_a_hit_cap(mhc):
    """The long stream's records come from the host-side automaton: count-only, and a hit_cap that ends inside the long
    stream's records, behind them and in front of them."""
    big = bytearray(np.random.default_rng(11).integers(0, 256, 1 << 21, dtype=np.uint8).tobytes())
    for at in (10, 5000, 1 << 20, (1 << 21) - 100):
        big[at:at + len(NEEDLE)] = NEEDLE
    msgs = [NEEDLE + b" and " + NEEDLE, bytes(big), text(3000, 2) + NEEDLE, NEEDLE]
    w = World(mhc, msgs)
    ps = mhc.PatternSet([NEEDLE, b"!"])
    w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(msgs, [NEEDLE, b"!"]), 4)
    pay, off, nb, _, _ = w.enc(2, 1024)
    assert nb[1] > mhc.BATCH_WALK_MAX_BITS
    ho, rec, pat, st, rc = w.model[2].find_batch_o2(ps, pay, off, nb, hit_cap="count")
    assert rc == mhc.MH_OK and not st.any() and np.array_equal(ho, w_off) and rec.shape[0] == 0
    total = int(w_off[-1])
    for cap in (int(w_off[1]) + 3, int(w_off[2]) + 1, total):
        ho, rec, pat, st, rc = w.model[2].find_batch_o2(ps, pay, off, nb, hit_cap=cap, check=False)
        assert rc == (mhc.MH_OK if cap == total else mhc.MH_ERR_CAPACITY) and not st.any(), cap
        assert np.array_equal(ho, w_off) and np.array_equal(rec, w_rec[:cap]) and np.array_equal(pat, w_pat[:cap]), cap


def test_host_recode_splices_a_long_stream_under_an_order_2_destination(mhc):
    """Order 2 -> order 2 through the splice: mh_encode under an order-2 model that lacks codes for most of the long stream's
    triples, so that its dropped count comes from the host."""
    big = np.random.default_rng(12).integers(0, 256, 1 << 21, dtype=np.uint8).tobytes()
    msgs = [text(700, 3), big, text(5000, 4), b""]
    w = World(mhc, msgs)
    tc = mhc.histogram_o2_batch([text(1 << 16, 5), big[:1 << 16]])
    dst = mhc.Model.from_counts(tc, 2)
    pay, off, nb, _, _ = w.enc(2, 1024)
    assert nb[1] > mhc.BATCH_WALK_MAX_BITS
    e_pay, e_off, e_nb, e_idx, e_so = dst.encode_batch_o2(msgs, chunk_symbols=1024)
    got = w.model[2].recode_batch_o2(dst, pay, off, nb, chunk_symbols=1024)
    assert got["rc"] == mhc.MH_OK and not got["status"].any()
    assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb) and np.array_equal(got["payload"], e_pay)
    assert np.array_equal(got["sym_off"], e_so) and np.array_equal(slices(got["index"], e_so, 1024), slices(e_idx, e_so, 1024))
    want = []
    for m in msgs:
        d = np.frombuffer(m, dtype=np.uint8).astype(np.int64)
        p1 = np.concatenate([[0x20], d[:-1]])[:d.size]
        p2 = np.concatenate([[0x20, 0x20], d[:-2]])[:d.size]
        want.append(int((tc[((p2 << 8 | p1) << 8) | d] == 0).sum()))
    assert got["dropped"].tolist() == want and want[1] > 1 << 20


# ---------------------------------------------------------------------------------------------------- the use case

def test_wiki_lines_migrate_to_order_2_and_back_without_a_decoded_buffer(mhc):
    lines = [ln for ln in golden()["input_wiki_cpp.html"]["data"].split(b"\n") if ln]
    assert len(lines) == 1581
    m1 = mhc.Model.from_counts(mhc.histogram_o1_batch(lines), 1)
    pay1, off1, nb1, idx1, so1 = m1.encode_batch(lines, chunk_symbols=256)
    assert int(off1[-1]) == 162287
    kw = dict(sym_off=so1, index=idx1, chunk_symbols=256)
    counts = mhc.histogram_coded_batch_o2(m1, 2, pay1, off1, nb1, **kw)
    assert np.array_equal(counts, mhc.histogram_o2_batch(lines))
    m2 = mhc.Model.from_counts(counts, 2)
    got = m1.dev_recode_batch_o2(m2, pay1, off1, nb1, **kw)
    e_pay, e_off, e_nb, e_idx, _ = m2.encode_batch_o2(lines, chunk_symbols=256)
    assert got["rc"] == mhc.MH_OK and int(got["out_off"][-1]) == 100419
    assert np.array_equal(got["payload"], e_pay) and np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb)
    assert np.array_equal(slices(got["index"], so1, 256), slices(e_idx, so1, 256))
    k = max(range(len(lines)), key=lambda i: len(lines[i]))
    needle = lines[k][40:72]
    kw2 = dict(sym_off=so1, index=got["index"], chunk_symbols=256)
    ho, rec, pat, st, rc = m2.dev_find_batch_o2(mhc.PatternSet([needle]), got["payload"], got["out_off"], got["nbits"], **kw2)
    assert rc == mhc.MH_OK and k in rec[:, 0].tolist()
    assert [tuple(r) for r in rec.tolist()] == [h[:3] for h in find_ref.find_hits(lines, [needle])]
    back = m2.dev_recode_batch_o2(m1, got["payload"], got["out_off"], got["nbits"], **kw2)
    assert back["rc"] == mhc.MH_OK and int(back["out_off"][-1]) == 162287
    assert np.array_equal(back["payload"], pay1) and np.array_equal(back["nbits"], nb1)
    assert np.array_equal(slices(back["index"], so1, 256), slices(idx1, so1, 256))


# ---------------------------------------------------------------------------------------------------- arguments

def _buf():
    w = np.zeros(1 << 14, dtype=np.uint64)
    return w, (w.ctypes.data + 255) & ~255


def _call(fn, names, defaults, **kw):
    a = dict(defaults)
    a.update(kw)
    return fn(*[a[k] for k in names])


FIND_ARGS = ("m", "ps", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total", "index", "chunk", "hit_off", "hits", "pat",
             "cap", "status", "ws", "wsb", "stream")
RECODE_ARGS = ("src", "dst", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total", "index", "chunk", "out", "cap", "out_off",
               "out_nbits", "out_index", "dropped", "status", "ws", "wsb", "stream")
HIST_ARGS = ("src", "order", "payload", "pay_off", "nbits", "n", "pay_total", "prev0", "sym_off", "sym_total", "index", "chunk", "counts", "status", "ws",
             "wsb", "stream")


def test_device_forms_refuse_bad_arguments_before_any_launch(mhc, world):
    """Host pointers stand in for device pointers: every call below must return before it launches anything."""
    lib, ARG, CAP = mhc.lib(), mhc.MH_ERR_ARG, mhc.MH_ERR_CAPACITY
    m0, m1, m2 = (world.model[o].handle for o in (0, 1, 2))
    ps = mhc.PatternSet([b"abc"])
    keep, p = _buf()
    common = dict(payload=p, pay_off=p, nbits=p, n=1, pay_total=16, prev0=0x20, sym_off=p, sym_total=100, index=p, chunk=256, status=p, ws=p,
                  wsb=1 << 16, stream=None)
    find = lambda **kw: _call(lib.mh_dev_find_batch_o2, FIND_ARGS, dict(common, m=m2, ps=ps.handle, hit_off=p, hits=p, pat=p, cap=4), **kw)
    recode = lambda **kw: _call(lib.mh_dev_recode_batch_o2, RECODE_ARGS,
                                dict(common, src=m1, dst=m2, out=p, cap=64, out_off=p, out_nbits=p, out_index=p, dropped=p), **kw)
    hist = lambda **kw: _call(lib.mh_dev_histogram_coded_batch_o2, HIST_ARGS, dict(common, src=m2, order=1, counts=p), **kw)
    for m in (None, m0, m1):
        assert find(m=m) == ARG
    assert find(ps=None) == ARG
    for k in ("payload", "pay_off", "nbits", "hit_off", "sym_off", "ws"):
        assert find(**{k: None}) == ARG, k
    for k in ("payload", "ws"):
        assert find(**{k: p + 8}) == ARG, k
    assert find(wsb=lib.mh_dev_find_batch_o2_workspace(1, 100, 256) - 1) == CAP
    for s, d in ((m0, m0), (m0, m1), (m1, m0), (m1, m1)):
        assert recode(src=s, dst=d) == ARG                              # no order-2 side: mh_dev_recode_batch serves it
    for s in (m0, m1):
        for order in (0, 1, -1, 3):
            assert hist(src=s, order=order) == ARG
    for order in (-1, 3):
        assert hist(order=order) == ARG
    for s, d in ((m1, m2), (m0, m2), (m2, m1), (m2, m0), (m2, m2)):
        assert recode(src=None, dst=d) == ARG and recode(src=s, dst=None) == ARG
        for k in ("payload", "pay_off", "nbits", "out_off", "out_nbits", "sym_off", "ws"):
            assert recode(src=s, dst=d, **{k: None}) == ARG, k
        for k in ("payload", "out", "ws"):
            assert recode(src=s, dst=d, **{k: p + 8}) == ARG, k
        assert recode(src=s, dst=d, index=None, sym_off=None) == ARG    # index-free: sym_off is an output
        assert recode(src=s, dst=d, index=None, chunk=300) == ARG       # the destination index's chunk
        assert recode(src=s, dst=d, wsb=lib.mh_dev_recode_batch_o2_workspace(1, 100, 256) - 1) == CAP
    for src, order in ((m2, 0), (m2, 1), (m2, 2), (m1, 2), (m0, 2)):
        for k in ("payload", "pay_off", "nbits", "counts", "sym_off", "ws"):
            assert hist(src=src, order=order, **{k: None}) == ARG, k
        for k in ("payload", "ws"):
            assert hist(src=src, order=order, **{k: p + 8}) == ARG, k
        assert hist(src=src, order=order, wsb=lib.mh_dev_histogram_coded_batch_o2_workspace(1, 100, 256) - 1) == CAP
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert find(chunk=bad_chunk) == ARG and recode(chunk=bad_chunk) == ARG and recode(src=m2, dst=m1, chunk=bad_chunk) == ARG
        assert hist(chunk=bad_chunk) == ARG
    assert keep is not None


def test_host_forms_refuse_bad_arguments(mhc, world):
    lib, ARG = mhc.lib(), mhc.MH_ERR_ARG
    m1, m2 = world.model[1].handle, world.model[2].handle
    ps = mhc.PatternSet([b"abc"])
    d = dict(payload=np.zeros(32, dtype=np.uint8), pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2,
             prev0=0x20, sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             status=np.zeros(2, dtype=np.int32))
    raw = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    fargs = ("m", "ps", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "hit_off", "hits", "pat", "cap", "status")
    rargs = ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk", "out", "cap", "out_off", "out_nbits", "out_index",
             "dropped", "status")

    def find(**kw):
        a = dict(d, m=m2, ps=ps.handle, hit_off=np.zeros(3, dtype=np.uint64), hits=np.zeros(12, dtype=np.uint64), pat=np.zeros(4, dtype=np.uint32), cap=4)
        a.update(kw)
        return lib.mh_find_batch_o2(*[raw(a[k]) for k in fargs])

    def recode(**kw):
        a = dict(d, src=m1, dst=m2, out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64),
                 out_nbits=np.zeros(2, dtype=np.uint64), out_index=np.zeros(4, dtype=np.uint64), dropped=np.zeros(2, dtype=np.uint64))
        a.update(kw)
        return lib.mh_recode_batch_o2(*[raw(a[k]) for k in rargs])

    assert find(m=None) == ARG and find(m=m1) == ARG and find(ps=None) == ARG
    for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(hit_off=None), dict(sym_off=None)):
        assert find(**kw) == ARG, kw
    assert recode(src=None) == ARG and recode(dst=None) == ARG and recode(src=m1, dst=m1) == ARG
    for s, t in ((m1, m2), (m2, m1), (m2, m2)):
        for kw in (dict(payload=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None)):
            assert recode(src=s, dst=t, **kw) == ARG, kw
        for bad_chunk in (0, 100, 300, 128, 16384):
            assert recode(src=s, dst=t, chunk=bad_chunk) == ARG and recode(src=s, dst=t, index=None, chunk=bad_chunk) == ARG
        assert recode(src=s, dst=t, pay_off=np.array([1, 16, 32], dtype=np.uint64)) == ARG
        assert recode(src=s, dst=t, nbits=np.array([129, 128], dtype=np.uint64)) == ARG          # nbits past its bytes
        assert recode(src=s, dst=t, sym_off=np.array([0, 100, 50], dtype=np.uint64)) == ARG
    for bad_chunk in (0, 100, 300, 128, 16384):
        assert find(chunk=bad_chunk) == ARG
    assert find(pay_off=np.array([0, 16, 8], dtype=np.uint64)) == ARG and find(nbits=np.array([129, 128], dtype=np.uint64)) == ARG
    assert find(sym_off=np.array([0, 100, 50], dtype=np.uint64)) == ARG
