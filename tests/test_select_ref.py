"""tests/select_ref.py against tests/batch_ref.py (no GPU, no library): selecting picks from packed batches must give exactly
what packing the picked messages gives — payload, offsets, bit counts, symbol offsets and the whole index array — for orders
0, 1 and 2, chunks 256 and 1024, one and two sources, under the oracle's codes and under a model per stream (pack_each)."""
import numpy as np
import pytest

import batch_ref
import select_ref

PREV0 = batch_ref.PREV0


def messages(seed, chunk, n_extra=9):
    """Streams of 0, 1, chunk - 1, chunk, chunk + 1 symbols and some of random lengths, over a small skewed alphabet."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3] + [int(k) for k in rng.integers(0, 3 * chunk, n_extra)]
    rng.shuffle(lens)
    w = 1.0 / np.arange(1, 41) ** 1.2
    return [rng.choice(40, size=k, p=w / w.sum()).astype(np.uint8).tobytes() for k in lens]


def pick_lists(rng, sizes):
    """Identity, reverse, every record twice, MH_SELECT_NONE in the middle and trailing, all none, no pick, a random draw."""
    every = [select_ref.pick(s, i) for s, n in enumerate(sizes) for i in range(n)]
    draw = [every[k] for k in rng.integers(0, len(every), 2 * len(every))]
    return [every, every[::-1], [p for p in every for _ in range(2)], every[:3] + [select_ref.NONE] * 2 + every[3:] + [select_ref.NONE],
            [select_ref.NONE] * 4, [], draw]


def same(got, want, chunk):
    assert np.array_equal(got.payload, want.payload)
    assert np.array_equal(got.pay_off, want.pay_off) and np.array_equal(got.nbits, want.nbits)
    assert np.array_equal(got.sym_off, want.sym_off) and np.array_equal(got.dropped, want.dropped)
    assert np.array_equal(got.index_array(chunk), want.index_array(chunk))
    assert len(got.slices) == len(want.slices) and all(np.array_equal(a, b) for a, b in zip(got.slices, want.slices))
    assert not got.status.any()


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n_sources", [1, 2])
def test_select_equals_packing_the_picked_messages(order, chunk, n_sources):
    lists = [messages(100 * order + chunk + s, chunk) for s in range(n_sources)]
    lens, codes = batch_ref.oracle_codes(batch_ref.histogram([m for l in lists for m in l], order, PREV0), order)
    packs = [batch_ref.pack(l, lens, codes, order, PREV0, chunk) for l in lists]
    rng = np.random.default_rng(7)
    for picks in pick_lists(rng, [len(l) for l in lists]):
        want = batch_ref.pack(select_ref.picked_messages(lists, picks), lens, codes, order, PREV0, chunk)
        same(select_ref.select(packs, picks, chunk), want, chunk)


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("order", [0, 1])
def test_select_of_a_batch_with_a_model_per_stream(order, chunk):
    lists = [messages(5 + order, chunk, 3), messages(50 + order, chunk, 2)]
    packs = [batch_ref.pack_each(l, order, PREV0, chunk)[0] for l in lists]
    rng = np.random.default_rng(8)
    for picks in pick_lists(rng, [len(l) for l in lists]):
        want, _ = batch_ref.pack_each(select_ref.picked_messages(lists, picks), order, PREV0, chunk)
        same(select_ref.select(packs, picks, chunk), want, chunk)


def test_a_pick_that_names_nothing_is_refused_alone():
    msgs = messages(3, 256, 2)
    lens, codes = batch_ref.oracle_codes(batch_ref.histogram(msgs, 1, PREV0), 1)
    q = batch_ref.pack(msgs, lens, codes, 1, PREV0, 256)
    picks = [select_ref.pick(0, 1), select_ref.pick(1, 0), select_ref.pick(0, len(msgs)), select_ref.pick(0, 2), select_ref.pick(200, 0)]
    got = select_ref.select([q], picks, 256)
    assert got.status.tolist() == [0, -1, -1, 0, -1]
    want = batch_ref.pack([msgs[1], b"", b"", msgs[2], b""], lens, codes, 1, PREV0, 256)
    assert np.array_equal(got.payload, want.payload) and np.array_equal(got.index_array(256), want.index_array(256))
    q.nbits = q.nbits.copy()
    q.nbits[2] = (int(q.pay_off[3]) - int(q.pay_off[2])) * 8 + 1               # nbits past the stream's bytes
    assert select_ref.select([q], picks, 256).status.tolist() == [0, -1, -1, -1, -1]


def test_picks_from_hits_reference():
    hit_off = np.array([0, 0, 2, 2, 3, 3], dtype=np.uint64)
    status = np.array([0, 0, 0, -4, 0], dtype=np.int32)
    N = select_ref.NONE
    assert select_ref.picks_from_hits(hit_off, None)[0].tolist() == [1, 3, N, N, N]
    assert select_ref.picks_from_hits(hit_off, status)[0].tolist() == [1, N, N, N, N]
    p, k = select_ref.picks_from_hits(hit_off, status, select_ref.WITHOUT_HITS, source=3)
    assert k == 3 and p.tolist() == [(3 << 56) | 0, (3 << 56) | 2, (3 << 56) | 4, N, N]
    assert select_ref.picks_from_hits(None, status)[0].tolist() == [0, 1, 2, 4, N]
    assert select_ref.picks_from_hits(None, None, n=3) [0].tolist() == [0, 1, 2]
