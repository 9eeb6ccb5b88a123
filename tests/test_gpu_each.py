"""Batches of streams, one model each, on the GPU (include/mh.h, "BATCHES OF STREAMS, ONE MODEL EACH"): every stream's table
file, `.cm` file and index slice are what the single-stream calls give for that message alone — the reference's own per-file
outputs for the golden inputs — and both decoders give the messages back, or report per stream what is wrong."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import check_against_golden, expected_file, golden, golden_names

pytestmark = pytest.mark.gpu


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


EDGE_LENS = [0, 1, 15, 16, 17, 0, 0, 1023, 1024, 1025, 4095, 4096, 4097, 3, 0, 1 << 20, 5, 0]


def edge_messages(seed, n_random=2000):
    rng = np.random.default_rng(seed)
    lens = EDGE_LENS + [int(x) for x in rng.integers(0, 3000, n_random)]
    src = zipf(sum(lens) + 64, seed)
    text = golden()["input_wiki_cpp.txt"]["data"]
    out, p = [], 0
    for k, n in enumerate(lens):
        out.append(src[p:p + n] if k % 3 else (text * (n // max(len(text), 1) + 1))[p % 997:p % 997 + n])
        p += n
    return out


def oracle_outputs(oracle, m, order):
    om = oracle.Model.from_counts(oracle.histogram_o1(m) if order else oracle.histogram_o0(m), order)
    blob, nbits = om.compress(m)
    return om.table_bytes(), blob, nbits


def test_golden_files_in_one_batch(mhc):
    names = golden_names()
    msgs = [golden()[n]["data"] for n in names]
    for order, te, ce in ((1, "e", "cm"), (0, "eh", "ch")):
        res = mhc.compress_each(msgs, order=order)
        for name, (table, blob, _, _) in zip(names, res):
            check_against_golden(name, te, table)              # size, sha256 and, where committed, the bytes
            check_against_golden(name, ce, blob)
        assert mhc.decompress_each([r[0] for r in res], [r[1] for r in res]) == msgs
        # the reference's own files (those committed in full) decode as a batch
        full = [n for n in names if expected_file(n, te) is not None and expected_file(n, ce) is not None]
        assert len(full) >= 8
        back = mhc.decompress_each([expected_file(n, te) for n in full], [expected_file(n, ce) for n in full])
        assert back == [golden()[n]["data"] for n in full]


@pytest.mark.parametrize("order", [0, 1])
def test_edge_lengths_against_oracle(mhc, oracle, order):
    msgs = edge_messages(41 + order)
    ref = [oracle_outputs(oracle, m, order) for m in msgs]
    ms = mhc.ModelSet.train(msgs, order)
    assert len(ms) == len(msgs)
    tables = ms.table_bytes()
    for t, (rt, _, _) in zip(tables, ref):
        assert t == rt
    for c in (256, 1024, 8192):
        res = mhc.compress_each(msgs, order=order, chunk_symbols=c)
        for k, (m, (t, blob, nb, sl), (rt, rblob, rbits)) in enumerate(zip(msgs, res, ref)):
            assert t == rt and nb == rbits and blob == rblob, k
            if c == 1024 or k < 40:
                _, _, idx = mhc.Model.from_table(rt).encode(m, chunk_symbols=c) if rt else (None, None, np.zeros(0, np.uint64))
                assert np.array_equal(sl, idx), k
    # the device call: same payloads
    payload, out_off, nbits, _, in_off, rc = ms.encode(msgs)
    assert rc == mhc.MH_OK
    for i, (_, rblob, rbits) in enumerate(ref):
        assert int(nbits[i]) == rbits and bytes(payload[int(out_off[i]):int(out_off[i + 1])]) == rblob[1:]


@pytest.mark.parametrize("order", [0, 1])
def test_round_trip_trained_and_loaded_sets(mhc, order):
    msgs = edge_messages(7 + order, n_random=300)
    trained = mhc.ModelSet.train(msgs, order)
    tables = trained.table_bytes()
    loaded = mhc.ModelSet.from_tables(tables)
    nonempty = [i for i, t in enumerate(tables) if t]
    models = [mhc.Model.from_table(tables[i]) for i in nonempty]
    from_models = mhc.ModelSet.from_models(models)
    enc = trained.encode(msgs, chunk_symbols=1024)
    for s in (loaded,):
        e2 = s.encode(msgs, chunk_symbols=1024)
        assert bytes(e2[0]) == bytes(enc[0]) and np.array_equal(e2[2], enc[2]) and np.array_equal(e2[3], enc[3])
    sub = [msgs[i] for i in nonempty]
    e3 = from_models.encode(sub)
    e1 = trained.encode(msgs)
    for k, i in enumerate(nonempty):
        assert int(e3[2][k]) == int(e1[2][i])
        assert bytes(e3[0][int(e3[1][k]):int(e3[1][k + 1])]) == bytes(e1[0][int(e1[1][i]):int(e1[1][i + 1])])
    assert from_models.decode(e3[0], e3[1], e3[2])[0] == b"".join(sub)
    payload, out_off, nbits, idx, in_off, _ = enc
    for s in (trained, loaded):
        out, so, st, rc = s.decode(payload, out_off, nbits)
        assert rc == mhc.MH_OK and not st.any() and out == b"".join(msgs) and np.array_equal(so, in_off)
        out, so, st, rc = s.decode(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024)
        assert rc == mhc.MH_OK and not st.any() and out == b"".join(msgs)
    for i in range(0, len(msgs), 97):
        t, ml = trained.stream_info(i)
        assert t == order and ml == (mhc.Model.from_table(tables[i]).max_code_len if tables[i] else 0)


def test_golden_tables_as_a_model_set(mhc):
    names = [n for n in golden_names() if golden()[n]["data"] and expected_file(n, "e") is not None and expected_file(n, "cm") is not None]
    msgs = [golden()[n]["data"] for n in names]
    models = [mhc.Model.from_table(expected_file(n, "e")) for n in names]
    ms = mhc.ModelSet.from_models(models)
    payload, out_off, nbits, idx, in_off, rc = ms.encode(msgs, chunk_symbols=256)
    assert rc == mhc.MH_OK
    for i, n in enumerate(names):
        assert bytes([mhc.stream_header(1, int(nbits[i]))]) + bytes(payload[int(out_off[i]):int(out_off[i + 1])]) == expected_file(n, "cm")
    assert ms.decode(payload, out_off, nbits)[0] == b"".join(msgs)
    assert ms.decode(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=256)[0] == b"".join(msgs)


def test_per_stream_errors(mhc):
    msgs = [zipf(k, 60 + k) for k in (3000, 5000, 7000, 100, 9000)]
    ms = mhc.ModelSet.train(msgs, 1)
    payload, out_off, nbits, idx, in_off, _ = ms.encode(msgs, chunk_symbols=1024)
    good = [0, 1, 3, 4]
    # truncated nbits: that stream alone is corrupt, with and without an index
    cut = nbits.copy()
    cut[2] -= 1
    for kw in ({}, dict(sym_off=in_off, index=idx, chunk_symbols=1024)):
        out, so, st, rc = ms.decode(payload, out_off, cut, guard=64, **kw)
        assert list(st) == [0, 0, mhc.MH_ERR_CORRUPT, 0, 0] and rc == mhc.MH_ERR_CORRUPT
        for i in good:
            assert out[int(so[i]):int(so[i + 1])] == msgs[i]
    # a flipped payload bit
    flip = np.array(payload, dtype=np.uint8).copy()
    flip[int(out_off[2]) + 5] ^= 0x10
    out, so, st, rc = ms.decode(flip, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024, guard=64)
    assert list(st) == [0, 0, mhc.MH_ERR_CORRUPT, 0, 0]
    for i in good:
        assert out[int(so[i]):int(so[i + 1])] == msgs[i]
    # output capacity one byte short: the last stream does not fit, nothing is written at or beyond out_cap
    out, so, st, rc = ms.decode(payload, out_off, nbits, out_cap=int(in_off[-1]) - 1, guard=64)
    assert st[-1] == mhc.MH_ERR_CAPACITY and not st[:-1].any()
    for i in range(4):
        assert out[int(so[i]):int(so[i + 1])] == msgs[i]
    # payload capacity one byte short on the encoder: MH_ERR_CAPACITY, guard bytes untouched
    _, _, _, _, _, rc = ms.encode(msgs, cap=int(out_off[-1]) - 1, guard=64)
    assert rc == mhc.MH_ERR_CAPACITY
    # host form: per-stream statuses for a corrupt stream
    res = mhc.compress_each(msgs)
    blobs = [r[1] for r in res]
    blobs[1] = blobs[1][:-1]
    back, st = mhc.decompress_each([r[0] for r in res], blobs, check=False)
    assert st[1] != 0 and not st[[0, 2, 3, 4]].any()
    assert [back[i] for i in (0, 2, 3, 4)] == [msgs[i] for i in (0, 2, 3, 4)]


def test_stream_over_walk_cap(mhc):
    long_msg = bytes(np.random.default_rng(5).integers(0, 256, (mhc.BATCH_WALK_MAX_BITS // 8) * 5 // 4).astype(np.uint8))
    msgs = [zipf(2000, 1), long_msg, zipf(3000, 2)]
    ms = mhc.ModelSet.train(msgs, 1)
    payload, out_off, nbits, idx, in_off, _ = ms.encode(msgs)
    assert int(nbits[1]) > mhc.BATCH_WALK_MAX_BITS
    out, so, st, rc = ms.decode(payload, out_off, nbits)
    assert list(st) == [0, mhc.MH_ERR_ARG, 0] and rc == mhc.MH_ERR_ARG
    assert out[int(so[0]):int(so[1])] == msgs[0] and out[int(so[2]):int(so[3])] == msgs[2]
    res = mhc.compress_each(msgs)
    assert mhc.decompress_each([r[0] for r in res], [r[1] for r in res]) == msgs


def test_scale_grouping_empty_and_order2(mhc, oracle, monkeypatch):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 257, 65536)
    src = zipf(int(lens.sum()) + 16, 9)
    msgs, p = [], 0
    for n in lens:
        msgs.append(src[p:p + int(n)])
        p += int(n)
    res = mhc.compress_each(msgs, chunk_symbols=256)
    for i in range(0, len(msgs), 331):
        rt, rblob, rbits = oracle_outputs(oracle, msgs[i], 1)
        assert res[i][0] == rt and res[i][1] == rblob and res[i][2] == rbits
    assert mhc.decompress_each([r[0] for r in res], [r[1] for r in res]) == msgs
    assert mhc.decompress_each([r[0] for r in res], [r[1] for r in res], [r[3] for r in res], 256, [len(m) for m in msgs]) == msgs
    # a budget of a few streams per group: the same bytes
    sub = msgs[:3000]
    monkeypatch.setenv("MH_EACH_GROUP_BYTES", str(1 << 21))
    grouped = mhc.compress_each(sub, chunk_symbols=256)
    assert [g[:3] for g in grouped] == [r[:3] for r in res[:3000]]
    assert all(np.array_equal(g[3], r[3]) for g, r in zip(grouped, res[:3000]))
    assert mhc.decompress_each([g[0] for g in grouped], [g[1] for g in grouped]) == sub
    monkeypatch.delenv("MH_EACH_GROUP_BYTES")
    assert mhc.compress_each([]) == [] and mhc.decompress_each([], []) == []
    ms = mhc.ModelSet.train([], 1)
    assert len(ms) == 0 and ms.table_bytes() == []
    with pytest.raises(mhc.MhError) as e:
        mhc.ModelSet.train([b"abc", b"def"], 2)
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.compress_each([b"abc"], order=2)
    assert e.value.status == mhc.MH_ERR_ARG


def test_more_live_contexts_than_one_tree_launch(mhc, oracle):
    """Over 4 M live contexts in one device call: the trees are built in more than one launch (mh_each.hip, TREE_SLICE)."""
    rng = np.random.default_rng(12)
    n, k = 17000, 2048
    data = rng.integers(0, 256, n * k).astype(np.uint8).tobytes()
    msgs = [data[i * k:(i + 1) * k] for i in range(n)]
    ms = mhc.ModelSet.train(msgs, 1)
    assert ms.slots > (1 << 22)
    tables = ms.table_bytes()
    payload, out_off, nbits, idx, in_off, rc = ms.encode(msgs, chunk_symbols=1024)
    assert rc == mhc.MH_OK
    for i in (0, 1, 8191, 16383, 16384, 16500, n - 1):
        rt, rblob, rbits = oracle_outputs(oracle, msgs[i], 1)
        assert tables[i] == rt and int(nbits[i]) == rbits and bytes(payload[int(out_off[i]):int(out_off[i + 1])]) == rblob[1:]
    out, so, st, rc = ms.decode(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not st.any() and out == data
    out, so, st, rc = ms.decode(payload, out_off, nbits)
    assert rc == mhc.MH_OK and not st.any() and out == data
