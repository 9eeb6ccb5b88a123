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
