"""Lookups (stream, begin, end) into a batch on the GPU (include/mh.h, "RANDOM ACCESS INTO BATCHES"), under a shared model
and under per-stream models, with and without the chunk index.  Ground truth: numpy slices of the messages.  The device-call
wrappers (Model.dev_decode_batch_ranges, ModelSet.decode_ranges) put guard bytes around every output and assert that nothing
outside the outputs of the lookups that decoded changed."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import golden

pytestmark = pytest.mark.gpu

GOLDEN5 = ["input_a.txt", "input_b.txt", "input_ipsum.txt", "input_wiki_cpp.html", "input_wiki_cpp.txt"]
CHUNKS = [256, 512, 1024, 2048, 4096, 8192]


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


@pytest.fixture(scope="module")
def messages():
    """The five golden inputs cut into messages of mixed length, empty ones included."""
    rng = np.random.default_rng(11)
    out = []
    for name in GOLDEN5:
        d = golden()[name]["data"]
        p = 0
        while p < len(d):
            n = int(rng.choice([0, 1, 7, int(rng.integers(1, 600)), int(rng.integers(600, 12000))]))
            out.append(d[p:p + n])
            p += n
        out.append(b"")
    return out


def random_lookups(msgs, count, seed, streams=None):
    """Random lookups into msgs: mostly random ranges, plus empty ones, whole streams and stream tails."""
    rng = np.random.default_rng(seed)
    streams = np.arange(len(msgs)) if streams is None else np.asarray(streams)
    lk = []
    for k in range(count):
        i = int(rng.choice(streams))
        n = len(msgs[i])
        kind = k % 8
        if kind == 0:
            b = e = int(rng.integers(0, n + 1))
        elif kind == 1:
            b, e = 0, n
        elif kind == 2:
            b, e = max(0, n - int(rng.integers(1, 40))), n
        else:
            b, e = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        lk.append((i, b, e))
    return np.array(lk, dtype=np.uint64).reshape(-1, 3)


def expect(msgs, lk):
    return [bytes(msgs[int(i)][int(b):int(e)]) for i, b, e in lk]


def check_ok(mhc, res, st, msgs, lk):
    assert (st == mhc.MH_OK).all(), np.unique(st)
    assert res == expect(msgs, lk)


def shared_model(mhc, msgs, order):
    """The shared model of a batch: trained on the messages each starting in context PREV0 (mh_dev_histogram_o1_batch)."""
    return mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=order), order)


def shared_batch(mhc, msgs, order, chunk):
    model = shared_model(mhc, msgs, order)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=chunk)
    return model, payload, out_off, nbits, idx, in_off


# ------------------------------------------------------------------------------------------------ shared model

@pytest.mark.parametrize("order", [0, 1])
def test_golden_shared_model_every_chunk_size_and_index_free(mhc, messages, order):
    lk = random_lookups(messages, 400, 3 + order)
    model = shared_model(mhc, messages, order)
    for chunk in CHUNKS:
        payload, out_off, nbits, idx, in_off = model.encode_batch(messages, chunk_symbols=chunk)
        res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off, index=idx, chunk_symbols=chunk)
        assert rc == mhc.MH_OK
        check_ok(mhc, res, st, messages, lk)
        res, st = model.decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off, index=idx, chunk_symbols=chunk)
        check_ok(mhc, res, st, messages, lk)
    payload, out_off, nbits, _, in_off = model.encode_batch(messages)
    for so in (None, in_off):
        res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=so)
        assert rc == mhc.MH_OK
        check_ok(mhc, res, st, messages, lk)
        res, st = model.decode_batch_ranges(payload, out_off, nbits, lk, sym_off=so)
        check_ok(mhc, res, st, messages, lk)


def test_each_stream_equals_decode_ranges_on_its_slice(mhc, messages):
    chunk = 512
    model, payload, out_off, nbits, idx, in_off = shared_batch(mhc, messages, 1, chunk)
    lib = mhc.lib()
    lk = random_lookups(messages, 300, 21)
    res, st, _ = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off, index=idx, chunk_symbols=chunk)
    for i in sorted(set(int(x) for x in lk[:, 0]))[:40]:
        mine = lk[:, 0] == i
        n = len(messages[i])
        b = lib.mh_batch_index_base(int(in_off[i]), i, chunk)
        sl = idx[b:b + (n + chunk - 1) // chunk]
        one, one_st = model.decode_ranges(payload[int(out_off[i]):int(out_off[i + 1])], int(nbits[i]), sl, chunk, n, lk[mine][:, 1:])
        assert list(one_st) == list(st[mine])
        assert one == [r for r, k in zip(res, mine) if k]


# ------------------------------------------------------------------------------------------------ per-stream models

def _each_batch(blobs):
    payload, pay_off = [], [0]
    for b in blobs:
        payload.append(b[1:])
        pay_off.append(pay_off[-1] + len(b) - 1)
    return np.frombuffer(b"".join(payload), dtype=np.uint8), np.array(pay_off, dtype=np.uint64)


@pytest.mark.parametrize("chunk", [None, 1024])
def test_per_stream_models_from_compress_each(mhc, messages, chunk):
    enc = mhc.compress_each(messages, order=1, chunk_symbols=chunk)
    tables = [t for t, _, _, _ in enc]
    blobs = [b for _, b, _, _ in enc]
    nbits = np.array([nb for _, _, nb, _ in enc], dtype=np.uint64)
    slices = [s for _, _, _, s in enc] if chunk else None
    lengths = [len(m) for m in messages]
    lk = random_lookups(messages, 400, 5)
    res, st = mhc.decompress_each_ranges(tables, blobs, lk, indices=slices, chunk_symbols=chunk or 0, lengths=lengths if chunk else None)
    check_ok(mhc, res, st, messages, lk)
    # whole streams equal decompress_each
    whole = np.array([(i, 0, len(m)) for i, m in enumerate(messages)], dtype=np.uint64)
    res, st = mhc.decompress_each_ranges(tables, blobs, whole, indices=slices, chunk_symbols=chunk or 0, lengths=lengths if chunk else None)
    assert (st == mhc.MH_OK).all()
    assert res == mhc.decompress_each(tables, blobs, indices=slices, chunk_symbols=chunk or 0, lengths=lengths if chunk else None)
    # the device call under the set of those tables
    s = mhc.ModelSet.from_tables(tables)
    payload, pay_off = _each_batch(blobs)
    so = np.array([0] + list(np.cumsum(lengths)), dtype=np.uint64)
    idx = mhc._batch_index(slices, so, chunk) if chunk else None
    res, st, rc = s.decode_ranges(payload, pay_off, nbits, lk, sym_off=so if chunk else None, index=idx, chunk_symbols=chunk or 0)
    assert rc == mhc.MH_OK
    check_ok(mhc, res, st, messages, lk)


def test_mixed_order_model_set(mhc, messages):
    msgs = messages[:300]
    models = [mhc.Model.from_data(m if m else b"x", order=i % 2) for i, m in enumerate(msgs)]
    s = mhc.ModelSet.from_models(models)
    lk = random_lookups(msgs, 500, 8)
    for chunk in (None, 256, 2048):
        payload, oo, nbits, idx, off, rc = s.encode(msgs, chunk_symbols=chunk)
        assert rc == mhc.MH_OK
        res, st, rc = s.decode_ranges(payload, oo, nbits, lk, sym_off=off if chunk else None, index=idx, chunk_symbols=chunk or 0)
        assert rc == mhc.MH_OK
        check_ok(mhc, res, st, msgs, lk)
        whole = np.array([(i, 0, len(m)) for i, m in enumerate(msgs)], dtype=np.uint64)
        res, st, _ = s.decode_ranges(payload, oo, nbits, whole, sym_off=off if chunk else None, index=idx, chunk_symbols=chunk or 0)
        dec, _, _, _ = s.decode(payload, oo, nbits, sym_off=off if chunk else None, index=idx, chunk_symbols=chunk or 0)
        assert b"".join(res) == dec == b"".join(msgs)


def test_decompress_batch_ranges_over_whole_files(mhc, messages):
    model = shared_model(mhc, messages, 1)
    files = model.compress_batch(messages, chunk_symbols=1024)
    lk = random_lookups(messages, 200, 9)
    res, st = model.decompress_batch_ranges([f for f, _, _ in files], lk, indices=[s for _, _, s in files], chunk_symbols=1024,
                                            lengths=[len(m) for m in messages])
    check_ok(mhc, res, st, messages, lk)
    res, st = model.decompress_batch_ranges([f for f, _, _ in files], lk)
    check_ok(mhc, res, st, messages, lk)


# ------------------------------------------------------------------------------------------------ per-lookup errors

def _long_streams(messages, n_chunks=4, chunk=256):
    return [i for i, m in enumerate(messages) if len(m) >= n_chunks * chunk]


@pytest.mark.parametrize("indexed", [True, False])
def test_per_lookup_errors_leave_the_others_exact(mhc, messages, indexed):
    chunk = 256 if indexed else None
    model, payload, out_off, nbits, idx, in_off = shared_batch(mhc, messages, 1, chunk)
    n = len(messages)
    good = random_lookups(messages, 200, 13)
    i = _long_streams(messages)[0]
    ni = len(messages[i])
    bad = np.array([(n, 0, 1), (n + 5, 0, 0), (i, 10, 9), (i, 0, ni + 1)], dtype=np.uint64)
    lk = np.concatenate([good[:100], bad, good[100:]])
    for so in ((in_off,) if indexed else (None, in_off)):
        res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=so, index=idx, chunk_symbols=chunk or 0)
        assert list(st[100:104]) == [mhc.MH_ERR_ARG] * 4
        assert rc == mhc.MH_ERR_ARG
        keep = np.r_[0:100, 104:len(lk)]
        check_ok(mhc, [res[k] for k in keep], st[keep], messages, lk[keep])
        hres, hst = model.decode_batch_ranges(payload, out_off, nbits, lk, sym_off=so, index=idx, chunk_symbols=chunk or 0)
        assert list(hst) == list(st) and hres == res
    # capacity: the outputs past out_cap are refused and not written (the wrapper checks the guard bytes)
    res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, good, sym_off=in_off if indexed else None, index=idx,
                                                chunk_symbols=chunk or 0, out_cap=2000)
    assert rc == mhc.MH_ERR_CAPACITY and (st == mhc.MH_ERR_CAPACITY).any()
    fit = st == mhc.MH_OK
    assert fit.any()
    assert [r for r, f in zip(res, fit) if f] == expect(messages, good[fit])


def test_index_entry_behind_its_predecessor(mhc, messages):
    chunk = 256
    model, payload, out_off, nbits, idx, in_off = shared_batch(mhc, messages, 1, chunk)
    lib = mhc.lib()
    i = _long_streams(messages)[1]
    base = lib.mh_batch_index_base(int(in_off[i]), i, chunk)
    bad_idx = idx.copy()
    ent1 = int(idx[base + 1])
    bad_idx[base + 2] = np.uint64((int(idx[base + 2]) & ~mhc.INDEX_BIT_MASK) | ((ent1 & mhc.INDEX_BIT_MASK) - 1))
    lk = np.concatenate([random_lookups(messages, 300, 17, streams=[i]), random_lookups(messages, 200, 18)])
    res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off, index=bad_idx, chunk_symbols=chunk)
    c2 = 2 * chunk
    hit = (lk[:, 0] == i) & (lk[:, 1] < lk[:, 2]) & (((lk[:, 1] < c2 + chunk) & (lk[:, 2] > c2)) | (lk[:, 2] == c2))
    assert hit.any() and (~hit).any()
    assert (st[hit] == mhc.MH_ERR_CORRUPT).all()
    assert rc == mhc.MH_ERR_CORRUPT
    check_ok(mhc, [r for r, h in zip(res, hit) if not h], st[~hit], messages, lk[~hit])


@pytest.mark.parametrize("indexed", [True, False])
def test_truncated_nbits_fails_only_the_lookups_reaching_the_end(mhc, messages, indexed):
    chunk = 256 if indexed else None
    model, payload, out_off, nbits, idx, in_off = shared_batch(mhc, messages, 1, chunk)
    i = _long_streams(messages, 8)[0]
    ni = len(messages[i])
    nb = nbits.copy()
    nb[i] -= 5
    lk = np.array([(i, 0, 100), (i, 300, 700), (i, ni - 3, ni), (i, 0, ni), (i, ni, ni)] +
                  [tuple(x) for x in random_lookups(messages, 100, 19)], dtype=np.uint64)
    lk = lk[(lk[:, 0] != i) | (lk[:, 2] <= 700) | (lk[:, 2] == ni)]
    end = (lk[:, 0] == i) & (lk[:, 2] == ni) & (lk[:, 1] < lk[:, 2])
    for so in ((in_off,) if indexed else (None, in_off)):
        res, st, _ = model.dev_decode_batch_ranges(payload, out_off, nb, lk, sym_off=so, index=idx, chunk_symbols=chunk or 0)
        assert end.sum() >= 2 and (st[end] != mhc.MH_OK).all()
        check_ok(mhc, [r for r, h in zip(res, end) if not h], st[~end], messages, lk[~end])


def test_long_index_free_stream(mhc):
    msgs = [zipf(3000, 1), zipf(1 << 21, 2), zipf(5000, 3), b""]
    model = shared_model(mhc, msgs, 1)
    payload, out_off, nbits, _, in_off = model.encode_batch(msgs)
    assert int(nbits[1]) > mhc.BATCH_WALK_MAX_BITS
    lk = np.array([(0, 5, 500), (1, 0, 100), (1, 2000000, 2000100), (2, 0, 5000), (3, 0, 0), (1, 7, 7)], dtype=np.uint64)
    res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk)
    assert list(st) == [mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_ERR_ARG, mhc.MH_OK, mhc.MH_OK, mhc.MH_OK]
    assert rc == mhc.MH_ERR_ARG
    assert res[0] == msgs[0][5:500] and res[3] == msgs[2]
    for so in (None, in_off):
        res, st = model.decode_batch_ranges(payload, out_off, nbits, lk, sym_off=so)
        check_ok(mhc, res, st, msgs, lk)


def test_end_past_the_stream_index_free(mhc, messages):
    model, payload, out_off, nbits, _, in_off = shared_batch(mhc, messages, 0, None)
    i = _long_streams(messages)[0]
    ni = len(messages[i])
    lk = np.array([(i, 0, ni + 1), (i, ni, ni + 3), (i, 0, ni), (i, ni, ni)], dtype=np.uint64)
    res, st, _ = model.dev_decode_batch_ranges(payload, out_off, nbits, lk)                # the walk runs past the end
    assert list(st) == [mhc.MH_ERR_ARG, mhc.MH_ERR_ARG, mhc.MH_OK, mhc.MH_OK]
    res, st, _ = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off)   # refused up front
    assert list(st) == [mhc.MH_ERR_ARG, mhc.MH_ERR_ARG, mhc.MH_OK, mhc.MH_OK]
    assert res[2] == messages[i]


# ------------------------------------------------------------------------------------------------ host forms

def test_host_form_uploads_only_the_touched_streams(mhc):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 200, 65536)
    src = zipf(int(lens.sum()), 5)
    off = np.r_[0, np.cumsum(lens)]
    msgs = [src[off[k]:off[k + 1]] for k in range(len(lens))]
    model = shared_model(mhc, msgs, 1)
    for chunk in (None, 1024):
        payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=chunk)
        touched = [int(x) for x in rng.choice(np.nonzero(lens > 20)[0], 10, replace=False)]
        lk = random_lookups(msgs, 50, 6, streams=touched)
        res, st = model.decode_batch_ranges(payload, out_off, nbits, lk, sym_off=in_off if chunk else None, index=idx, chunk_symbols=chunk or 0)
        check_ok(mhc, res, st, msgs, lk)
        used = sorted(set(int(i) for i, b, e in lk if b < e))
        assert mhc.last_batch_range_upload_bytes() == sum(int(out_off[i + 1] - out_off[i]) for i in used)


def test_host_form_never_reads_untouched_streams(mhc, messages):
    enc = mhc.compress_each(messages, order=1, chunk_symbols=1024)
    tables = [t for t, _, _, _ in enc]
    blobs = [b for _, b, _, _ in enc]
    nbits = np.array([nb for _, _, nb, _ in enc], dtype=np.uint64)
    slices = [s for _, _, _, s in enc]
    lengths = [len(m) for m in messages]
    live = [i for i, m in enumerate(messages) if len(m) > 100]
    victim, others = live[0], live[1:40]
    lk = random_lookups(messages, 200, 22, streams=others)
    tab, tab_off = mhc.batch_offsets(tables)
    payload, pay_off = _each_batch(blobs)
    res0, st0 = mhc._each_ranges(tab, tab_off, payload, pay_off, nbits, lk, slices, 1024, lengths)
    check_ok(mhc, res0, st0, messages, lk)
    tab, payload = tab.copy(), payload.copy()
    tab[int(tab_off[victim]):int(tab_off[victim + 1])] = 0xFF                          # malformed table
    payload[int(pay_off[victim]):int(pay_off[victim + 1])] ^= 0x5A                     # scrambled payload
    res1, st1 = mhc._each_ranges(tab, tab_off, payload, pay_off, nbits, lk, slices, 1024, lengths)
    assert res1 == res0 and list(st1) == list(st0)
    # touched, the malformed table fails only that stream's lookups
    lk2 = np.concatenate([lk, np.array([(victim, 0, 10), (victim, 5, 5)], dtype=np.uint64)])
    res2, st2 = mhc._each_ranges(tab, tab_off, payload, pay_off, nbits, lk2, slices, 1024, lengths)
    assert st2[-2] == mhc.MH_ERR_BADTABLE and st2[-1] == mhc.MH_OK
    assert res2[:-2] == res0 and list(st2[:-2]) == list(st0)


def test_order2_is_refused(mhc):
    data = b"the order-2 extension has no lookups into batches. " * 40
    m2 = mhc.Model.from_data(data, order=2)
    payload = np.zeros(64, dtype=np.uint8)
    pay_off = np.array([0, 64], dtype=np.uint64)
    nbits = np.array([512], dtype=np.uint64)
    with pytest.raises(mhc.MhError) as e:
        m2.decode_batch_ranges(payload, pay_off, nbits, [(0, 0, 10)])
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        m2.dev_decode_batch_ranges(payload, pay_off, nbits, [(0, 0, 10)])
    assert e.value.status == mhc.MH_ERR_ARG


def test_a_million_lookups_in_one_call(mhc):
    rng = np.random.default_rng(30)
    lens = rng.integers(0, 120, 65536)
    src = zipf(int(lens.sum()), 31)
    off = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    msgs = [src[int(off[k]):int(off[k + 1])] for k in range(len(lens))]
    model = shared_model(mhc, msgs, 1)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    m = 1 << 20
    s = rng.integers(0, 65536, m).astype(np.uint64)
    n = off[s + 1] - off[s]
    a = (rng.random(m) * (n + 1)).astype(np.uint64)
    b = (rng.random(m) * (n + 1)).astype(np.uint64)
    lk = np.stack([s, np.minimum(a, b), np.maximum(a, b)], axis=1)
    for chunk_args in (dict(sym_off=in_off, index=idx, chunk_symbols=256), dict()):
        res, st, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lk, **chunk_args)
        assert rc == mhc.MH_OK and (st == mhc.MH_OK).all()
        whole = np.frombuffer(src, dtype=np.uint8)
        got = np.frombuffer(b"".join(res), dtype=np.uint8)
        want = np.concatenate([whole[int(off[i] + x):int(off[i] + y)] for i, x, y in lk])
        assert np.array_equal(got, want)
