"""Banks of shared models on the GPU (include/mh.h, "BANKS OF SHARED MODELS"): selection equals a numpy brute force over every
entry's code lengths, a stream coded through a view equals the single-stream encoder under its entry (and the oracle with that
entry's table), both decoders and the byte-range lookups give the messages back through a view, and training is deterministic,
covers every stream and never raises the payload."""
import gc
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "markovhuffman")


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


def letters(n, seed, k=16):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, k, n) + ord("a")).astype(np.uint8).tobytes()


def text(n, at=0):
    t = golden()["input_wiki_cpp.txt"]["data"]
    return (t * (n // len(t) + 2))[at % len(t):at % len(t) + n]


EDGE_LENS = [0, 1, 15, 16, 17, 0, 1023, 1024, 1025, 2047, 4096, 3, 0, 1 << 20, 5, 0]


def mixed_messages(seed, n_random=300, lens=EDGE_LENS):
    rng = np.random.default_rng(seed)
    lens = list(lens) + [int(x) for x in rng.integers(0, 3000, n_random)]
    out = []
    for k, n in enumerate(lens):
        src = (k + seed) % 3
        out.append(text(n, 7 * k) if src == 0 else zipf(n, seed * 1000 + k) if src == 1 else letters(n, seed * 1000 + k))
    return out


_LENS = {}


def code_lens(model):
    key = model.table_bytes()
    if key not in _LENS:
        _LENS[key] = model.codes()[0].astype(np.int64)
    return _LENS[key]


def brute_select(models, msgs, prev0=0x20):
    lens = [code_lens(m) for m in models]
    choice, nbits = [], []
    for m in msgs:
        a = np.frombuffer(m, dtype=np.uint8).astype(np.int64)
        prev = np.concatenate([[prev0], a[:-1]]) if a.size else a
        pairs = prev * 256 + a
        best, arg = None, 0xFFFFFFFF
        for k, l in enumerate(lens):
            v = l[pairs]
            if a.size and (v == 0).any():
                continue
            s = int(v.sum())
            if best is None or s < best:
                best, arg = s, k
        choice.append(arg)
        nbits.append(best if best is not None else (1 << 64) - 1)
    return np.array(choice, dtype=np.uint32), np.array(nbits, dtype=np.uint64)


def bank_models(mhc, k):
    """k distinct order-0/1 models over the three sources: text, Zipf bytes and a 16-letter alphabet (the last covers little)."""
    out = []
    for j in range(k):
        src = j % 3
        data = text(20000 + 997 * j, 131 * j) if src == 0 else zipf(5000 + 300 * j, 77 + j) if src == 1 else letters(3000 + 100 * j, 91 + j)
        out.append(mhc.Model.from_data(data, order=0 if j % 4 == 3 else 1))
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 64])
def test_select_equals_brute_force(mhc, k):
    models = bank_models(mhc, k)
    bank = mhc.ModelSet.from_models(models)
    msgs = mixed_messages(5 + k)
    msgs += [letters(50, 3), bytes([0x61] * 40), bytes(range(256)) * 3]          # uncovered by the letter entries
    ch, nb = bank.select(msgs)
    want_c, want_n = brute_select(models, msgs)
    assert np.array_equal(ch, want_c)
    assert np.array_equal(nb, want_n)
    assert (ch[[i for i, m in enumerate(msgs) if not m]] == 0).all()
    if k >= 3:
        assert (ch == mhc.BANK_NONE).any() or k == 64
        assert len(set(ch.tolist()) - {mhc.BANK_NONE}) >= 2


def test_ties_go_to_the_lowest_entry_and_none_when_uncovered(mhc):
    a = mhc.Model.from_data(text(30000), order=1)
    dup = mhc.Model.from_table(a.table_bytes())
    small = mhc.Model.from_data(letters(2000, 1), order=1)
    bank = mhc.ModelSet.from_models([small, a, dup])
    msgs = [text(500, 3), b"", letters(300, 9), b"\x00\xff" * 10]
    ch, nb = bank.select(msgs)
    want_c, want_n = brute_select([small, a, dup], msgs)
    assert np.array_equal(ch, want_c) and np.array_equal(nb, want_n)
    assert ch[0] == 1 and ch[1] == 0 and ch[3] == mhc.BANK_NONE and nb[3] == (1 << 64) - 1


def test_view_codes_every_stream_as_its_entry_alone(mhc, oracle, tmp_path):
    models = bank_models(mhc, 3)
    bank = mhc.ModelSet.from_models(models)
    msgs = [m for m in mixed_messages(11, 200) if m]
    ch, nb = bank.select(msgs)
    keep = [i for i in range(len(msgs)) if ch[i] != mhc.BANK_NONE]
    msgs, ch, nb = [msgs[i] for i in keep], ch[keep], nb[keep]
    view = bank.pick(ch)
    assert len(view) == len(msgs) and view.slots == bank.slots and view.code_lens() == bank.code_lens()
    tables = bank.table_bytes()
    for c in (256, 1024):
        payload, out_off, nbits, idx, off, rc = view.encode(msgs, chunk_symbols=c)
        assert rc == mhc.MH_OK
        assert np.array_equal(nbits, nb)                                        # select's nbits = the encoder's
        lib = mhc.lib()
        for i, m in enumerate(msgs):
            model = models[ch[i]]
            blob, bits, sl = model.compress(m, chunk_symbols=c)
            mine = bytes([lib.mh_stream_header(model.handle, int(nbits[i]))]) + payload[int(out_off[i]):int(out_off[i + 1])].tobytes()
            assert bits == nbits[i] and mine == blob, i
            b = lib.mh_batch_index_base(int(off[i]), i, c)
            assert np.array_equal(idx[b:b + len(sl)], sl), i
            if c == 256 and i % 7 == 0:
                ref_blob, ref_bits = oracle.Model.from_table(tables[ch[i]]).compress(m)
                assert ref_blob == blob and ref_bits == bits, i
    if os.path.exists(REF_BIN):                                                # the genuine binary with -e bank_k.e
        payload, out_off, nbits, _, _, _ = view.encode(msgs)
        for i in range(0, len(msgs), max(1, len(msgs) // 6)):
            t = tmp_path / ("bank_%d.e" % ch[i])
            t.write_bytes(tables[ch[i]])
            f, o = tmp_path / ("m%d" % i), tmp_path / ("m%d.cm" % i)
            f.write_bytes(msgs[i])
            subprocess.run([REF_BIN, str(f), "-e", str(t), "-o", str(o)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            model = models[ch[i]]
            mine = bytes([mhc.lib().mh_stream_header(model.handle, int(nbits[i]))]) + payload[int(out_off[i]):int(out_off[i + 1])].tobytes()
            assert mine == o.read_bytes(), i


def test_round_trips_through_a_view_after_the_bank_is_freed(mhc):
    models = bank_models(mhc, 4)
    bank = mhc.ModelSet.from_models(models)
    msgs = mixed_messages(23, 300)
    ch, _ = bank.select(msgs)
    covered = [i for i in range(len(msgs)) if ch[i] != mhc.BANK_NONE]
    msgs, ch = [msgs[i] for i in covered], ch[covered]
    view = bank.pick(ch)
    with pytest.raises(mhc.MhError) as e:
        view.table_bytes()
    assert e.value.status == mhc.MH_ERR_ARG
    del bank
    gc.collect()
    payload, out_off, nbits, idx, off, rc = view.encode(msgs, chunk_symbols=512)
    assert rc == mhc.MH_OK
    out, so, st, rc = view.decode(payload, out_off, nbits, sym_off=off, index=idx, chunk_symbols=512)
    assert rc == mhc.MH_OK and out == b"".join(msgs) and not st.any()
    out, so, st, rc = view.decode(payload, out_off, nbits)
    assert rc == mhc.MH_OK and out == b"".join(msgs) and np.array_equal(so, off) and not st.any()
    rng = np.random.default_rng(3)
    lookups = []
    for _ in range(400):
        i = int(rng.integers(0, len(msgs)))
        n = len(msgs[i])
        b = int(rng.integers(0, n + 1))
        lookups.append((i, b, int(rng.integers(b, n + 1))))
    for kw in ({}, {"sym_off": off, "index": idx, "chunk_symbols": 512}):
        got, st, rc = view.decode_ranges(payload, out_off, nbits, lookups, **kw)
        assert rc == mhc.MH_OK and not np.asarray(st).any()
        assert [g for g in got] == [msgs[i][b:e] for i, b, e in lookups]


def test_pick_refuses_out_of_range_choices(mhc):
    bank = mhc.ModelSet.from_models(bank_models(mhc, 2))
    for bad in ([0, 2, 1], [mhc.BANK_NONE], [1, 0, 0xFFFFFFFE]):
        with pytest.raises(mhc.MhError) as e:
            bank.pick(bad)
        assert e.value.status == mhc.MH_ERR_ARG
    assert len(bank.pick([])) == 0


def test_select_errors(mhc):
    bank = mhc.ModelSet.from_models(bank_models(mhc, 2))
    data = zipf(3000, 1)
    for off in ([0, 2000, 1000, 3000], [5, 1000, 3000], [0, 1000, 2999]):
        with pytest.raises(mhc.MhError) as e:
            bank.select(data, in_off=off)
        assert e.value.status == mhc.MH_ERR_ARG
    big = mhc.ModelSet.from_models(bank_models(mhc, 3) * 22)                   # 66 entries: not a bank
    with pytest.raises(mhc.MhError) as e:
        big.select([data])
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.ModelSet.train_bank([data], 65)
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.ModelSet.train_bank([data], 2, order=2)
    assert e.value.status == mhc.MH_ERR_ARG


def ipsum(n, at=0):
    t = golden()["input_ipsum.txt"]["data"]
    return (t * (n // len(t) + 2))[at % len(t):at % len(t) + n]


def three_sources(n_each, size, seed):
    """Text, Zipf(1.1) bytes and a 16-letter alphabet, interleaved: about 3.8, 5.7 and 4.3 bits per byte under their shared
    model, so the seed's rate order already separates them."""
    msgs, src = [], []
    for j in range(3 * n_each):
        s = j % 3
        msgs.append(ipsum(size, 389 * j) if s == 0 else zipf(size, seed + j) if s == 1 else letters(size, seed + j))
        src.append(s)
    return msgs, np.array(src)


@pytest.mark.parametrize("order", [0, 1])
def test_k1_is_the_shared_model(mhc, order):
    msgs = mixed_messages(31, 200)
    bank, ch, it = mhc.ModelSet.train_bank(msgs, 1, order=order)
    counts = mhc.histogram_o1_batch(msgs, order=order)
    shared = mhc.Model.from_counts(counts, order)
    assert len(bank) == 1 and (ch == 0).all() and it == 1
    assert bank.table_bytes() == [shared.table_bytes()]
    pay, oo, nb, _, _ = mhc.encode_bank(bank, msgs, ch)
    pay2, oo2, nb2, _, _ = shared.encode_batch(msgs)
    assert np.array_equal(oo, oo2) and np.array_equal(nb, nb2) and np.array_equal(pay, pay2)


def test_training_is_deterministic_covering_and_monotone(mhc):
    msgs = mixed_messages(41, 600)
    shared = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    shared_bits = int(shared.encode_batch(msgs)[2].sum())
    runs = [mhc.ModelSet.train_bank(msgs, 6, max_iters=6) for _ in range(2)]
    runs.append(mhc.ModelSet.train_bank(msgs, 6, max_iters=6, host=True))
    (b0, c0, i0) = runs[0]
    for b, c, i in runs[1:]:
        assert np.array_equal(c, c0) and i == i0 and b.table_bytes() == b0.table_bytes()
    assert 1 <= len(b0) <= 6
    ch, nb = b0.select(msgs)
    assert np.array_equal(ch, c0) and (ch != mhc.BANK_NONE).all()
    prev = None
    for t in range(1, 6):
        b, c, it = mhc.ModelSet.train_bank(msgs, 6, max_iters=t)
        assert it <= t
        total = int(b.select(msgs)[1].sum())
        assert total <= shared_bits
        if prev is not None:
            assert total <= prev
        prev = total
    assert prev < shared_bits


def test_three_sources_separate(mhc):
    msgs, src = three_sources(40, 3000, 7)
    bank, ch, it = mhc.ModelSet.train_bank(msgs, 3, max_iters=10)
    assert len(bank) == 3
    per = [set(ch[src == s].tolist()) for s in range(3)]
    assert all(len(p) == 1 for p in per) and len(set.union(*per)) == 3
    shared = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    shared_bits = int(shared.encode_batch(msgs)[2].sum())
    bits = int(bank.select(msgs)[1].sum())
    assert bits < 0.95 * shared_bits                                           # 0.93 measured


def test_empty_batches_and_k_over_n(mhc):
    bank, ch, it = mhc.ModelSet.train_bank([b"", b"", b""], 4)
    assert len(bank) == 1 and list(ch) == [0, 0, 0]
    bank, ch, it = mhc.ModelSet.train_bank([], 4)
    assert len(bank) == 1 and len(ch) == 0
    msgs = [text(100), zipf(100, 1)]
    bank, ch, it = mhc.ModelSet.train_bank(msgs, 8)
    assert 1 <= len(bank) <= 2 and (ch < len(bank)).all()


def test_host_forms_round_trip_and_long_streams(mhc):
    rng = np.random.default_rng(5)
    msgs = mixed_messages(51, 200) + [rng.integers(0, 256, 1_200_000, dtype=np.uint8).tobytes()]   # over the walk cap
    bank, ch, _ = mhc.ModelSet.train_bank(msgs, 4, max_iters=3, host=True)
    lib = mhc.lib()
    _, off = mhc.batch_offsets(msgs)
    ml = [bank.stream_info(k)[1] for k in range(len(bank))]
    want = len(msgs) + 16 + sum((len(m) * ml[c] + 7) // 8 for m, c in zip(msgs, ch))
    assert mhc.encode_bank_bound(bank, msgs, ch) == want
    assert mhc.encode_bank_bound(bank, msgs, np.full(len(msgs), len(bank), dtype=np.uint32)) == 0
    pay, oo, nb, idx, off = mhc.encode_bank(bank, msgs, ch, chunk_symbols=1024)
    assert nb[-1] > mhc.BATCH_WALK_MAX_BITS
    out, so, st = mhc.decode_bank(bank, ch, pay, oo, nb)
    assert out == b"".join(msgs) and np.array_equal(so, off) and not st.any()
    out, so, st = mhc.decode_bank(bank, ch, pay, oo, nb, sym_off=off, index=idx, chunk_symbols=1024)
    assert out == b"".join(msgs) and not st.any()
    # the bank's K tables are all a decoder needs: a bank rebuilt from them decodes the same payloads
    again = mhc.ModelSet.from_tables(bank.table_bytes())
    out, _, _ = mhc.decode_bank(again, ch, pay, oo, nb)
    assert out == b"".join(msgs)
    bad = ch.copy()
    bad[3] = len(bank)
    with pytest.raises(mhc.MhError) as e:
        mhc.encode_bank(bank, msgs, bad)
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.decode_bank(bank, bad, pay, oo, nb)
    assert e.value.status == mhc.MH_ERR_ARG


def test_scale_65536_streams_of_4k(mhc):
    n, size = 65536, 4096
    src = zipf(n * size // 2, 99)
    t = text(n * size // 4)
    l = letters(n * size // 4, 5)
    msgs = []
    for i in range(n):
        s = i % 4
        pool = src if s < 2 else t if s == 2 else l
        at = (i // 4) * size % (len(pool) - size)
        msgs.append(pool[at:at + size])
    bank, ch, it = mhc.ModelSet.train_bank(msgs, 16, max_iters=4)
    assert 1 <= len(bank) <= 16 and (ch < len(bank)).all()
    ch2, nb = bank.select(msgs)
    assert np.array_equal(ch, ch2)
    view = bank.pick(ch)
    payload, out_off, nbits, idx, off, rc = view.encode(msgs, chunk_symbols=1024)
    assert rc == mhc.MH_OK and np.array_equal(nbits, nb)
    out, so, st, rc = view.decode(payload, out_off, nbits, sym_off=off, index=idx, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not st.any() and out == b"".join(msgs)
    out, so, st, rc = view.decode(payload, out_off, nbits)
    assert rc == mhc.MH_OK and not st.any() and out == b"".join(msgs)
