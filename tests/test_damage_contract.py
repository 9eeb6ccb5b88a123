"""The damaged-stream contract on the CPU (tests/damage.py): the oracle's strict span decoder (mho_decode_span, a tree walk)
against its lenient mho_decompress on valid streams, and its verdicts on damaged streams against the code boundaries that
follow from the oracle's code lengths, computed independently with numpy.  No GPU."""
import functools

import numpy as np
import pytest

import damage
from conftest import golden, kat_inputs

ORDER_PREV0 = {0: 0x20, 1: 0x20, 2: 0x2020}


def small_text(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 7)).astype(np.uint8)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 40))] + b" "
    return bytes(out[:n])


def lens_of(om, order):
    return np.asarray(om.codes_o2()[0] if order == 2 else om.codes()[0])


@functools.lru_cache(None)
def inputs():
    g = golden()
    out = {k: g[k]["data"] for k in sorted(g)}
    for k in ("kat1", "kat2", "kat3", "kat4"):
        out[k] = kat_inputs()[k]
    return out


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(inputs()))
def test_span_decoder_equals_decompress_on_valid_streams(oracle, name, order):
    data = inputs()[name]
    if order == 2 and len(data) > 200_000:
        data = data[:200_000]                                  # (order-2 models are 16 M contexts: keep the walk short)
    om = oracle.Model.from_data(data, order)
    blob, nbits = om.compress(data)
    assert om.decompress(blob) == data
    st, out, ns, stop = om.decode_span(blob[1:], 0, nbits, ORDER_PREV0[order])
    assert (st, ns, stop) == (0, len(data), nbits)
    assert out == data
    # the same stream in chunks of 100 symbols from the positions the code lengths give
    if data:
        idx, _ = damage.expected_entries(lens_of(om, order), np.frombuffer(data, dtype=np.uint8), 100, ORDER_PREV0[order], order)
        assert damage.verdict_indexed(om, blob[1:], nbits, idx, 100, len(data), order) == (0, data)


def boundary_verdicts(om, data, order=1):
    """Expected index-free verdict of every cut nbits' in [0, nbits], from the code lengths alone."""
    b = damage.boundaries(lens_of(om, order), np.frombuffer(data, dtype=np.uint8), order, ORDER_PREV0[order])
    nbits = int(b[-1])
    at = {int(p): i for i, p in enumerate(b)}
    return nbits, [(0, data[:at[c]]) if c in at else (damage.MH_ERR_CORRUPT, None) for c in range(nbits + 1)]


@pytest.mark.parametrize("name", ["kat1", "text"])
def test_every_cut_gives_the_verdict_of_the_code_boundaries(oracle, name):
    data = kat_inputs()["kat1"] if name == "kat1" else small_text(1500)
    om = oracle.Model.from_data(data, 1)
    blob, nbits = om.compress(data)
    nb, want = boundary_verdicts(om, data)
    assert nb == nbits
    for c in range(nbits + 1):
        assert damage.verdict_free(om, damage.cut(blob[1:], nbits, c), c) == want[c], c


def test_every_cut_of_an_order_2_stream(oracle):
    data = small_text(600, 5)
    om = oracle.Model.from_data(data, 2)
    blob, nbits = om.compress(data)
    nb, want = boundary_verdicts(om, data, 2)
    assert nb == nbits
    for c in range(nbits + 1):
        st, out, _, _ = om.decode_span(damage.cut(blob[1:], nbits, c), 0, c, 0x2020)
        assert (st, out if st == 0 else None) == ((0, want[c][1]) if want[c][0] == 0 else (-1, None)), c


def test_indexed_verdicts_of_cuts_and_extensions(oracle):
    """Indexed: any nbits other than the true one fails the last chunk, boundaries included; the other chunks still pass."""
    data = small_text(3000, 8)
    om = oracle.Model.from_data(data, 1)
    blob, nbits = om.compress(data)
    d = np.frombuffer(data, dtype=np.uint8)
    idx, _ = damage.expected_entries(lens_of(om, 1), d, 256)
    assert damage.verdict_indexed(om, blob[1:], nbits, idx, 256, len(data)) == (0, data)
    b = damage.boundaries(lens_of(om, 1), d)
    for name, pl, nb in damage.d1_end_cuts(blob[1:], nbits, b) + damage.d2_extensions(blob[1:], nbits, 9):
        assert damage.verdict_indexed(om, pl, nb, idx, 256, len(data))[0] == damage.MH_ERR_CORRUPT, name
        cv = damage.chunk_verdicts(om, pl, nb, idx, 256, len(data))
        assert all(ok for ok, _ in cv[:-1]) and not cv[-1][0], name
        # a range that stays in the earlier chunks decodes; one that reads the last chunk to its end fails
        assert damage.verdict_range(om, pl, nb, idx, 256, len(data), 10, 600) == (0, data[10:600]), name
        assert damage.verdict_range(om, pl, nb, idx, 256, len(data), 2900, 3000)[0] == damage.MH_ERR_CORRUPT, name


def test_null_entry_and_wrong_table(oracle):
    """D5: a byte that only ends the training data has no context table; bits after it meet a null entry.  D6: a payload
    under another source's table."""
    data = small_text(2000, 2) + b"\x01"
    om = oracle.Model.from_data(data, 1)
    name, pl, nb = damage.d5_null_entry(om, np.frombuffer(data, dtype=np.uint8), 1, extra=12)
    st, out, ns, stop = om.decode_span(pl, 0, nb, 0x20)
    assert (st, ns) == (-1, len(data)), name
    assert damage.verdict_free(om, pl, nb) == (damage.MH_ERR_CORRUPT, None)
    blob, nbits = om.compress(data)
    assert damage.verdict_free(om, blob[1:], nbits) == (0, data)
    other = oracle.Model.from_data(b"\x00", 1)     # context ' ' holds only byte 0, context 0 no table: the 2nd code is null
    assert damage.verdict_free(other, blob[1:], nbits) == (damage.MH_ERR_CORRUPT, None)
    # an order-2 model: a context never seen has no table
    om2 = oracle.Model.from_data(b"abcabcabd", 2)
    b2, n2 = om2.compress(b"abcabcabd")
    assert om2.decode_span(b2[1:], 0, n2, 0x2020)[0] == 0
    assert om2.decode_span(b2[1:], 0, n2, 0x6262)[0] == -1          # starts in context "bb": no table


def test_bits_after_nbits_never_change_a_verdict(oracle):
    data = small_text(2500, 4)
    om = oracle.Model.from_data(data, 1)
    blob, nbits = om.compress(data)
    d = np.frombuffer(data, dtype=np.uint8)
    b = damage.boundaries(lens_of(om, 1), d)
    cl = damage.code_lengths(lens_of(om, 1), d)
    for name, pl, nb in damage.all_damages(blob[1:], nbits, b, cl, b[::256], seed=1):
        v = damage.verdict_free(om, pl, nb)
        for fill in (0, 1):
            assert damage.verdict_free(om, damage.garbage_after(pl, nb, fill), nb) == v, name
            assert damage.verdict_free(om, damage.garbage_after(pl, nb, fill) + b"\xff\x00", nb) == v, name


def test_span_arguments(oracle):
    data = kat_inputs()["kat1"]
    om = oracle.Model.from_data(data, 1)
    blob, nbits = om.compress(data)
    assert om.decode_span(blob[1:], 0, len(blob) * 8)[0] == oracle.ERR_ARG     # end_bit beyond the payload
    assert om.decode_span(blob[1:], 5, 4)[0] == oracle.ERR_ARG
    assert om.decode_span(blob[1:], 0, 0)[:3] == (0, b"", 0)
    assert om.decode_span(blob[1:], 0, 0, max_symbols=0)[0] == 0
    assert om.decode_span(blob[1:], 0, nbits, max_symbols=len(data) - 1)[0] == -1  # symbols out before end_bit
    assert om.decode_span(blob[1:], 0, nbits, max_symbols=len(data) + 1)[0] == -1  # end_bit before the symbols are out


# ---- index damages (X1-X10) ------------------------------------------------------------------------------------------------
def zipf_small(n, seed, k=200):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, k + 1) ** 1.1
    return rng.choice(k, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


class Indexed:
    """One stream of the oracle at chunk 256 with the entries its code lengths give."""

    def __init__(self, oracle, data, order=1, counts=None, chunk=256):
        self.data, self.order, self.chunk = data, order, chunk
        self.om = oracle.Model.from_counts(counts, order) if counts is not None else oracle.Model.from_data(data, order)
        self.lens = lens_of(self.om, order)
        blob, self.nbits = self.om.compress(data)
        self.payload = blob[1:]
        d = np.frombuffer(data, dtype=np.uint8)
        self.b = damage.boundaries(self.lens, d, order, ORDER_PREV0[order])
        self.index, _ = damage.expected_entries(self.lens, d, chunk, ORDER_PREV0[order], order)

    def verdict(self, sl):
        return damage.verdict_indexed(self.om, self.payload, self.nbits, sl, self.chunk, len(self.data), self.order)


@functools.lru_cache(None)
def indexed_sources():
    from oracle import mh_oracle
    return {"zipf": Indexed(mh_oracle, zipf_small(1500, 31)), "text": Indexed(mh_oracle, small_text(1500, 6)),
            "text2": Indexed(mh_oracle, small_text(1500, 6), order=2), "zipf0": Indexed(mh_oracle, zipf_small(1500, 31), order=0),
            "flat": Indexed(mh_oracle, np.random.default_rng(5).integers(0, 256, 1500).astype(np.uint8).tobytes(),
                            counts=damage.flat_counts(7))}


def test_order_0_entries_carry_the_byte_in_front_of_the_chunk(oracle):
    s = indexed_sources()["zipf0"]
    d = np.frombuffer(s.data, dtype=np.uint8)
    assert [int(e) >> 56 for e in s.index] == [0x20] + [int(d[k - 1]) for k in range(256, 1500, 256)]
    assert s.verdict(s.index) == (0, s.data)


@pytest.mark.parametrize("name", ["zipf", "text", "text2"])
def test_every_position_damage_corrupts_some_stream(oracle, name):
    """X1-X7 and X9: every kind gives at least one MH_ERR_CORRUPT case, no case returns the intact slice, names are unique and
    the generators are deterministic."""
    s = indexed_sources()[name]
    assert s.verdict(s.index) == (0, s.data)
    cases = damage.index_damages(s.index, s.b, s.nbits, s.order, s.lens, seed=3)
    again = damage.index_damages(s.index, s.b, s.nbits, s.order, s.lens, seed=3)
    assert [n for n, _ in cases] == [n for n, _ in again] and all(np.array_equal(a, b) for (_, a), (_, b) in zip(cases, again))
    assert len({n for n, _ in cases}) == len(cases)
    corrupt = {}
    for n, sl in cases:
        assert sl.dtype == np.uint64 and sl.size == s.index.size and not np.array_equal(sl, s.index), n
        kind = n.split("-")[0]
        corrupt[kind] = corrupt.get(kind, 0) + (s.verdict(sl)[0] == damage.MH_ERR_CORRUPT)
    assert set(corrupt) == {"X%d" % k for k in range(1, 10)}
    for kind in ("X1", "X2", "X3", "X4", "X5", "X6", "X7", "X9"):
        assert corrupt[kind] > 0, kind


def test_entries_at_and_behind_are_always_corrupt(oracle):
    """X3, X4 and X7 leave no room for a chunk: every case of them is corrupt, whatever the payload."""
    for name in ("zipf", "text", "text2", "flat", "zipf0"):
        s = indexed_sources()[name]
        for kind in ("X3", "X4", "X7"):
            for n, sl in damage.index_damages(s.index, s.b, s.nbits, s.order, kinds=[kind]):
                assert s.verdict(sl)[0] == damage.MH_ERR_CORRUPT, (name, n)


def test_gap_entries_change_nothing(oracle):
    """X10: the entries between slices belong to nobody."""
    s = indexed_sources()["zipf"]
    u = lambda *v: np.array(v, dtype=np.uint64)
    idx = np.concatenate([u(7), s.index, u(0, 9), s.index, u(1)])
    bases, sizes = [1, 3 + s.index.size], [s.index.size] * 2
    n, dam = damage.x10_gaps(idx, bases, sizes)
    assert n == "X10-gaps" and not np.array_equal(dam, idx)
    for a in bases:
        assert np.array_equal(dam[a:a + s.index.size], s.index)
        assert s.verdict(dam[a:a + s.index.size]) == (0, s.data)
    assert np.all(dam[[0, 1 + s.index.size, 2 + s.index.size, -1]] == np.uint64(0xFFFFFFFFFFFFFFFF))


def test_flat_model_every_context_byte_decodes_to_other_bytes(oracle):
    """Every code of the flat model has 8 bits, so any context byte keeps the chunk on its end bit: MH_OK with other bytes, for
    every changed value of the generator and for all 255 other values at one entry; a position moved by a symbol is corrupt."""
    s = indexed_sources()["flat"]
    assert set(np.unique(s.lens)) == {8}
    cases = damage.x8_context_field(s.index, s.b, s.nbits, 1, s.lens, seed=1)
    assert len(cases) >= 9
    cases += damage.x8_context_field(s.index, s.b, s.nbits, 1, s.lens, values=range(256), entries=[2])
    for n, sl in cases:
        st, out = s.verdict(sl)
        k = int(np.flatnonzero(sl != s.index)[0])
        assert st == 0 and len(out) == len(s.data), n
        assert out[:k * 256] == s.data[:k * 256] and out[(k + 1) * 256:] == s.data[(k + 1) * 256:], n
        assert out[k * 256:(k + 1) * 256] != s.data[k * 256:(k + 1) * 256], n
    for n, sl in damage.x2_other_boundary(s.index, s.b, s.nbits, 1):
        assert s.verdict(sl)[0] == damage.MH_ERR_CORRUPT, n


def test_text_model_context_byte_reaches_both_outcomes(oracle):
    s = indexed_sources()["text"]
    seen = set()
    for n, sl in damage.x8_context_field(s.index, s.b, s.nbits, 1, s.lens, values=range(256), entries=[3]):
        st, out = s.verdict(sl)
        seen.add((st, None if out is None else out == s.data))
    assert (damage.MH_ERR_CORRUPT, None) in seen and any(st == 0 for st, _ in seen), seen
    # a context with no table fails its chunk; the generator names one
    dead = [c for c in damage.x8_context_field(s.index, s.b, s.nbits, 1, s.lens, seed=2) if "dead" in c[0]]
    assert dead and all(s.verdict(sl)[0] == damage.MH_ERR_CORRUPT for _, sl in dead)
    # order 2: the generator gives the high byte, the low byte and a dead pair; the dead pair is corrupt
    s2 = indexed_sources()["text2"]
    c2 = damage.x8_context_field(s2.index, s2.b, s2.nbits, 2, s2.lens, seed=2)
    assert {n.split("e", 1)[1][1:3] for n, _ in c2} == {"hi", "lo", "de"}
    assert all(s2.verdict(sl)[0] == damage.MH_ERR_CORRUPT for n, sl in c2 if "dead" in n)


def test_order_0_ignores_the_context_field(oracle):
    s = indexed_sources()["zipf0"]
    cases = damage.x8_context_field(s.index, s.b, s.nbits, 0, s.lens, seed=4)
    cases += damage.x8_context_field(s.index, s.b, s.nbits, 0, s.lens, values=range(0, 256, 17), entries=[1])
    assert len(cases) > 12
    for n, sl in cases:
        assert s.verdict(sl) == (0, s.data), n


def test_ranges_over_a_damaged_entry(oracle):
    """verdict_range with the rules of include/mh.h: an entry past nbits or behind the one before it fails every range that
    touches its chunk or ends on its start boundary; the others decode."""
    s = indexed_sources()["zipf"]
    n, c = len(s.data), s.chunk
    vr = lambda sl, b, e: damage.verdict_range(s.om, s.payload, s.nbits, sl, c, n, b, e)
    p = [int(e) & damage.pos_mask(1) for e in s.index]
    for b, e in ((0, n), (10, 20), (c - 3, c + 3), (3 * c, 3 * c + 1), (n - 1, n), (5, 5)):
        assert vr(s.index, b, e) == (0, s.data[b:e])
    behind = np.array(s.index)
    behind[3] = (s.index[3] & np.uint64(0xFF << 56)) | np.uint64(p[2] - 1)
    past = np.array(s.index)
    past[3] = (s.index[3] & np.uint64(0xFF << 56)) | np.uint64(s.nbits + 1)
    for sl in (behind, past):
        assert vr(sl, 3 * c + 5, 3 * c + 9)[0] == damage.MH_ERR_CORRUPT          # ends inside the chunk
        assert vr(sl, 3 * c, 4 * c)[0] == damage.MH_ERR_CORRUPT                  # the chunk alone
        assert vr(sl, 2 * c + 7, 3 * c)[0] == damage.MH_ERR_CORRUPT              # ends on its start boundary
        assert vr(sl, 2 * c + 7, 3 * c - 1) == (0, s.data[2 * c + 7:3 * c - 1])  # inside the chunk in front
        assert vr(sl, 5 * c, n) == (0, s.data[5 * c:])
        assert vr(sl, 0, 2 * c) == (0, s.data[:2 * c])
        assert vr(sl, 3 * c, 3 * c) == (0, b"")
    assert vr(behind, 4 * c, n) == (0, s.data[4 * c:])
    assert vr(past, 4 * c + 1, 4 * c + 2)[0] == damage.MH_ERR_CORRUPT               # entry 4 now lies behind entry 3
    # an entry moved back to its predecessor's own position (an empty chunk in front) is not behind it
    on = np.array(s.index)
    on[3] = (s.index[3] & np.uint64(0xFF << 56)) | np.uint64(p[2])
    assert vr(on, 2 * c, 3 * c)[0] == damage.MH_ERR_CORRUPT                      # chunk 2 must use 0 bits for 256 symbols
    assert vr(on, 4 * c, n) == (0, s.data[4 * c:])
