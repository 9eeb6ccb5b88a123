"""The closed forms of tests/far_ref.py against the plain references on the real concatenation.  With P = 3 and P = 5 periods
the batch is small enough for batch_ref.pack, batch_ref.histogram, batch_ref.select, find_ref and zlib to take the real
messages; every closed form must equal them.  For the full-size P only the scalars are checked: the thresholds that the batch
crosses.  tests/test_gpu_batch_far.py materialises the same closed forms at the full P; without this module it proves nothing."""
import zlib

import numpy as np
import pytest

import batch_ref
import edit_ref
import far_ref
import find_ref
import splice_ref

FAR = far_ref.FAR


@pytest.fixture(scope="module", params=[3, 5])
def small(request):
    f = far_ref.far(request.param)
    return f, f.messages()


@pytest.fixture(scope="module", params=[("far", 3), ("far", 5), ("far2", 3), ("far2", 5)], ids=lambda v: "%s-%d" % v)
def any_small(request):
    """The order-0/1 batch and the order-2 batch (far_ref.Far2), small."""
    f = getattr(far_ref, request.param[0])(request.param[1])
    return f, f.messages()


def test_the_block_fits_its_own_contract():
    f = far_ref.far(3)
    assert len(f.blk) == far_ref.BLOCK and f.blk[-1] == far_ref.PREV0
    assert all(far_ref.BLOCK % c == 0 for c in far_ref.CHUNKS)
    for k in "SD":
        lens, _ = f.codes[k]
        assert lens.min() > 0                                      # no symbol lacks a code
        assert f.block_bits[k] % 8 == 0
    assert len({int(v) for v in f.codes["S"][0]}) > 4 and len({int(v) for v in f.codes["D"][0]}) > 2     # (codes of many lengths)
    assert far_ref.far(5).blk == f.blk and far_ref.far(None).codes["S"][0].tobytes() == f.codes["S"][0].tobytes()


def test_the_layout(any_small):
    f, msgs = any_small
    ln = [len(m) for m in msgs]
    c = far_ref.CHUNKS[0]
    assert ln == f.lengths and ln[f.f] == f.P * far_ref.BLOCK + len(f.streams[f.f].tail) and ln[f.g] == 3 * far_ref.BLOCK
    assert f.f >= 2 and f.g > f.f + 1 and f.n - f.g - 1 >= 30 and ln[-1] == 0
    assert any(ln[i] == 0 and ln[i + 1] == 0 for i in range(f.g, f.n - 1))
    assert {0, 1, c - 1, c, c + 1, 2 * c + 17} <= set(ln) and {255, 256, 257} <= set(ln)
    assert b"".join(msgs) == np.concatenate([np.tile(a, k) for a, k in f.data_parts()]).tobytes()
    assert all(f.read(i, b, e) == msgs[i][b:e] for i, b, e in f.lookups())


@pytest.mark.parametrize("chunk", far_ref.CHUNKS)
def test_pack(any_small, chunk):
    f, msgs = any_small
    for model in f.codes:
        check_pack(f, msgs, model, chunk)


def check_pack(f, msgs, model, chunk):
    ref = batch_ref.pack(msgs, *f.codes[model], f.orders[model], far_ref.PREV0, chunk)
    got = f.pack(model, chunk)
    for name in ("pay_off", "nbits", "sym_off", "dropped"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert np.array_equal(got.payload(), ref.payload)
    assert np.array_equal(got.index_array(), ref.index_array(chunk))
    mask = np.zeros(got.index_entries, dtype=bool)
    for i, sl in enumerate(ref.slices):
        b = int(ref.sym_off[i]) // chunk + i
        mask[b:b + sl.size] = True
    assert np.array_equal(got.index_mask(), mask)
    for i in (f.f, f.g, f.n - 2):                                  # entry_bits: the offsets that marks() searches
        sl = ref.slices[i]
        for j in {0, sl.size // 2, sl.size - 1} if sl.size else ():
            assert f.entry_bits(model, chunk, i, j) == int(sl[j]) & ((1 << 48) - 1)
        assert f.entry_bits(model, chunk, i, sl.size) == int(ref.nbits[i])


@pytest.mark.parametrize("order", [0, 1, 2])
def test_histograms(any_small, order):
    f, msgs = any_small
    assert np.array_equal(f.histogram(order), batch_ref.histogram(msgs, order))


def test_crc(any_small):
    f, msgs = any_small
    crc, ln = f.crcs()
    assert crc.tolist() == [zlib.crc32(m) for m in msgs] and ln.tolist() == [len(m) for m in msgs]


def test_crc_identities():
    rng = np.random.default_rng(1)
    a, b = bytes(rng.integers(0, 256, size=1000, dtype=np.uint8)), bytes(rng.integers(0, 256, size=77, dtype=np.uint8))
    assert far_ref.crc_concat(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    assert far_ref.crc_concat(zlib.crc32(a), zlib.crc32(b""), 0) == zlib.crc32(a)
    for k in (0, 1, 2, 7, 64, 65):
        assert far_ref.crc_repeat(zlib.crc32(b), len(b), k) == zlib.crc32(b * k)


def test_select(small):
    f, msgs = small
    want = batch_ref.select([(f.orders[k], f.codes[k][0]) for k in "SD"], msgs)
    got = f.select()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_hits(any_small):
    f, msgs = any_small
    off, rec, pat = f.hits()
    w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(msgs, f.patterns), f.n)
    assert np.array_equal(off, w_off) and np.array_equal(rec, w_rec) and np.array_equal(pat, w_pat)
    per = np.diff(off.astype(np.int64))
    assert per[f.f] == f.P + 4 and per[f.g] == 3 and sum(per[f.g + 1:]) >= 3 and sum(len(p) for p in f.patterns) <= 64
    tail_at = f.P * far_ref.BLOCK
    in_f = rec[rec[:, 0] == f.f]
    assert int(in_f[-1, 2]) == f.lengths[f.f]                      # a hit up to F's last byte
    assert any(int(b) - tail_at < 2048 < int(e) - tail_at for _, b, e in in_f)      # and one over a chunk seam of the tail


def test_lookups_reach_the_marks(any_small):
    f, msgs = any_small
    m, ch = f.marks(), far_ref.CHUNKS[1]
    ref = batch_ref.pack(msgs, *f.codes[f.src], f.orders[f.src], far_ref.PREV0, ch)
    assert f.lookup_bytes() == [msgs[i][b:e] for i, b, e in f.lookups()]
    for name in ("bit", "byte"):
        assert m[name] % ch == 0 and 0 < m[name] < f.lengths[f.f]
    sl = ref.slices[f.f] & np.uint64((1 << 48) - 1)
    nb = int(ref.nbits[f.f])
    for name, bit in (("bit", nb // 3), ("byte", 2 * nb // 3)):
        j = m[name] // ch
        assert int(sl[j]) <= bit < int(sl[j + 1])
    lk = f.lookups()
    assert any(i == f.f and b < m["symbol"] < e for i, b, e in lk) and any(i == f.f and e == f.lengths[f.f] and b < e for i, b, e in lk)
    assert any(i == f.g and b < e for i, b, e in lk) and any(i > f.g and b < e for i, b, e in lk) and any(b == e for _, b, e in lk)


def test_the_full_size_batch_crosses_every_threshold():
    f = far_ref.far(None)
    s, d = f.pack("S", far_ref.CHUNKS[1]), f.pack("D", far_ref.CHUNKS[0])
    assert f.lengths[f.f] >= FAR + (1 << 26)                       # F's symbols
    for p in (s, d):
        assert int(p.nbits[f.f]) > 8 * FAR                         # F's payload bits, and bytes, under both models
        assert int(p.pay_off[f.f + 1] - p.pay_off[f.f]) > FAR
        assert int(p.pay_off[f.g]) > FAR and int(p.pay_off[f.g]) * 8 > FAR       # G and all behind it wholly beyond all three
    assert int(f.sym_off[f.g]) > FAR and f.n - f.g - 1 >= 30
    assert int(s.nbits[f.g]) <= far_ref.WALK_MAX_BITS < int(s.nbits[f.f])         # G under the walk cap, F over it
    assert all(int(b) <= far_ref.WALK_MAX_BITS for i, b in enumerate(s.nbits) if i != f.f)
    assert int(f.sym_off[f.g]) // far_ref.CHUNKS[1] + f.g > (1 << 24)               # chunk numbers in the millions
    m = f.marks()
    assert m["symbol"] == FAR
    assert f.entry_bits("S", 256, f.f, m["bit"] // 256) <= FAR < f.entry_bits("S", 256, f.f, m["bit"] // 256 + 1)
    assert f.entry_bits("S", 256, f.f, m["byte"] // 256) <= 8 * FAR < f.entry_bits("S", 256, f.f, m["byte"] // 256 + 1)
    off, rec, pat = f.hits()
    in_f = rec[rec[:, 0] == f.f]
    assert int((in_f[:, 1] > FAR).sum()) >= far_ref.FAR_HITS                   # thousands of hit records beyond 2^32 inside F
    assert all(i != f.f or 0 <= b <= e <= f.lengths[f.f] for i, b, e in f.lookups())


def test_the_batch_without_f(small):
    """What the index-free calls must give: F's place taken by an empty stream, every other stream as it was."""
    f, msgs = small
    g = f.without_f()
    msgs = [b"" if i == f.f else m for i, m in enumerate(msgs)]
    assert g.messages() == msgs and g.lengths[f.f] == 0 and f.lengths[f.f] > 0 and g.total == f.total - f.lengths[f.f]
    ref = batch_ref.pack(msgs, *f.codes["D"], 0, far_ref.PREV0, 1024)
    got = g.pack("D", 1024)
    assert np.array_equal(got.payload(), ref.payload) and np.array_equal(got.index_array(), ref.index_array(1024))
    assert np.array_equal(got.pay_off, ref.pay_off) and np.array_equal(got.nbits, ref.nbits)
    off, rec, pat = g.hits()
    w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(msgs, f.patterns), f.n)
    assert np.array_equal(off, w_off) and np.array_equal(rec, w_rec) and np.array_equal(pat, w_pat)
    assert g.crcs()[0].tolist() == [zlib.crc32(m) for m in msgs]
    for order in (0, 1):
        assert np.array_equal(g.histogram(order), batch_ref.histogram(msgs, order))


@pytest.mark.parametrize("chunk", far_ref.CHUNKS)
def test_mix(small, chunk):
    """Stream i under entry choice[i] of the bank [S, D]: batch_ref.merge of every message packed alone."""
    f, msgs = small
    ch = f.choice()
    assert ch[f.f] == 0 and ch[f.g] == 0 and {int(c) for c in ch[f.g + 1:]} == {0, 1}
    ref = batch_ref.merge([batch_ref.pack([m], *f.codes["SD"[k]], f.orders["SD"[k]], far_ref.PREV0, chunk) for m, k in zip(msgs, ch)])
    got = f.mix(ch, chunk)
    assert np.array_equal(got.pay_off, ref.pay_off) and np.array_equal(got.nbits, ref.nbits) and np.array_equal(got.sym_off, ref.sym_off)
    assert np.array_equal(got.payload(), ref.payload) and np.array_equal(got.index_array(), ref.index_array(chunk))


def same_pack(got, ref, chunk):
    assert np.array_equal(got.pay_off, ref.pay_off) and np.array_equal(got.nbits, ref.nbits) and np.array_equal(got.sym_off, ref.sym_off)
    assert np.array_equal(got.payload(), ref.payload) and np.array_equal(got.index_array(), ref.index_array(chunk))
    assert np.array_equal(got.dropped, ref.dropped)


@pytest.mark.parametrize("without_f", [False, True])
def test_edits(small, without_f):
    """The masked and the splicing re-code under D: edit_ref and splice_ref on the real messages, then batch_ref.pack."""
    f, msgs = small
    if without_f:
        f, msgs = f.without_f(), [b"" if i == f.f else m for i, m in enumerate(msgs)]
    off, sp = f.spans()
    chunk = far_ref.CHUNKS[0]
    put = lambda y: batch_ref.pack(y, *f.codes["D"], 0, far_ref.PREV0, chunk)
    want = {"from 0", "to the last byte", "at or past the end", "whole stream", "a stream without spans between two with spans"}
    assert batch_ref.placements(msgs, off, sp, chunk) >= (want if without_f else want | {"past the end", "touching", "over a seam"})
    y = edit_ref.apply(msgs, off, sp, f.byte_map())
    assert y != msgs and [len(m) for m in y] == [len(m) for m in msgs]
    same_pack(f.edited().pack("D", chunk), put(y), chunk)
    for rep in f.reps():
        y = splice_ref.apply(msgs, off, sp, rep)
        got = f.spliced(rep)
        assert np.array_equal(got.sym_off, splice_ref.offsets(y)) and got.messages() == y
        same_pack(got.pack("D", chunk), put(y), chunk)
    assert len(f.reps()[0]) == 0 and len(f.reps()[1]) > 11
    if not without_f:
        assert int((sp[int(off[f.f]):int(off[f.f + 1]), 0] >= f.P * far_ref.BLOCK).all()) and off[f.g] == off[f.g + 1]


def test_the_order_2_block_and_its_full_size_batch():
    f, g = far_ref.far2(3), far_ref.far2(None)
    lens, _ = f.codes["S2"]
    live = f.counts["S2"] > 0
    assert f.blk[-2:] == bytes([far_ref.PREV0] * 2) and len(set(f.blk)) == 16 and f.block_bits["S2"] % 8 == 0
    assert lens[live].min() > 0 and not lens[~live].any() and len({int(v) for v in lens[live]}) > 4
    assert np.array_equal(batch_ref.histogram(f.messages(), 2) > 0, batch_ref.histogram(far_ref.far2(1).messages(), 2) > 0)   # (every triple has a code)
    s = g.pack("S2", far_ref.CHUNKS[1])
    assert g.blk == f.blk and g.lengths[g.f] >= FAR + (1 << 26) and int(s.nbits[g.f]) > FAR and int(g.sym_off[g.g]) > FAR
    assert int(s.pay_off[g.g]) * 8 > FAR and int(s.nbits[g.g]) <= far_ref.WALK_MAX_BITS and g.n - g.g - 1 >= 30
    m = g.marks()
    assert m["symbol"] == FAR and g.entry_bits("S2", 256, g.f, m["bit"] // 256) <= FAR < g.entry_bits("S2", 256, g.f, m["bit"] // 256 + 1)
    off, rec, pat = g.hits()
    assert int(((rec[:, 0] == g.f) & (rec[:, 1] > FAR)).sum()) >= far_ref.FAR_HITS
