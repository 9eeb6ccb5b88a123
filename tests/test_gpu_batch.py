"""Batches of independent streams under one shared model on the GPU (include/mh.h, "BATCHES OF INDEPENDENT STREAMS"):
every stream of a batch is the `.cm` file the reference writes for that message alone with the shared table, its index slice
is mh_encode's index of that message, and both decoders give the messages back — or report, per stream, what is wrong."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

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


EDGE_LENS = [0, 1, 15, 16, 17, 0, 0, 1023, 1024, 1025, 4095, 4096, 4097, 3, 0, 1 << 20, 5, 0]


def edge_messages(seed):
    src = zipf(sum(EDGE_LENS) + 64, seed)
    out, p = [], 0
    for n in EDGE_LENS:
        out.append(src[p:p + n])
        p += n
    return out


def check_against_oracle(mhc, oracle, model, msgs, chunks=(256, 1024, 8192)):
    om = oracle.Model.from_table(model.table_bytes())
    ref = [om.compress(m) for m in msgs]
    for c in chunks:
        res = model.compress_batch(msgs, chunk_symbols=c)
        for m, (blob, nb, sl), (rblob, rbits) in zip(msgs, res, ref):
            assert nb == rbits and blob == rblob
            _, _, idx = model.encode(m, chunk_symbols=c)
            assert np.array_equal(sl, idx)


@pytest.mark.parametrize("order", [0, 1])
def test_batch_matches_oracle_streams_and_indices(mhc, oracle, order):
    msgs = edge_messages(11 + order)
    counts = mhc.histogram_o1_batch(msgs, order=order)
    want = sum((oracle.histogram_o1(m) if order else oracle.histogram_o0(m)).astype(np.uint64) for m in msgs)
    assert np.array_equal(counts, want)
    model = mhc.Model.from_counts(counts, order)
    check_against_oracle(mhc, oracle, model, msgs)
    back = model.decompress_batch([b for b, _, _ in model.compress_batch(msgs)])
    assert back == msgs


def test_single_stream_batch_and_empty_batch(mhc, oracle):
    data = zipf(300000, 5)
    model = mhc.Model.from_data(data, 1)
    check_against_oracle(mhc, oracle, model, [data], chunks=(1024,))
    assert model.compress_batch([]) == []
    assert model.decompress_batch([]) == []


def test_hundred_thousand_small_streams(mhc, oracle):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 40, 100000)
    src = zipf(int(lens.sum()) + 1, 4, 1.3)
    msgs, p = [], 0
    for n in lens:
        msgs.append(src[p:p + int(n)])
        p += int(n)
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    res = model.compress_batch(msgs, chunk_symbols=256)
    om = oracle.Model.from_table(model.table_bytes())
    for i in rng.choice(len(msgs), 3000, replace=False):
        assert res[i][0] == om.compress(msgs[i])[0]
    blobs = [b for b, _, _ in res]
    assert model.decompress_batch(blobs) == msgs
    assert model.decompress_batch(blobs, [s for _, _, s in res], 256, [len(m) for m in msgs]) == msgs


def test_round_trip_65536_streams_of_4k_both_decoders(mhc):
    n, size = 65536, 4096
    src = zipf(n * size, 21)
    msgs = [src[i * size:(i + 1) * size] for i in range(n)]
    model = mhc.Model.from_data(src, 1)                    # (a pair the model has no code for is skipped, as the reference does)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=1024)
    out, so, st = model.decode_batch(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=1024)
    assert out == src and np.array_equal(so, in_off) and not st.any()
    out, so, st = model.decode_batch(payload, out_off, nbits)
    assert out == src and np.array_equal(so, in_off) and not st.any()


def test_long_codes_and_single_symbol_contexts(mhc, oracle):
    fib = [1, 1]
    while len(fib) < 48:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(65536, dtype=np.uint64)
    for prev in range(256):
        counts[prev * 256: prev * 256 + 48] = fib[::-1] if prev % 2 else fib
    model = mhc.Model.from_counts(counts, 1)
    assert model.max_code_len > 32
    rng = np.random.default_rng(8)
    msgs = [bytes(rng.integers(0, 48, int(k)).astype(np.uint8)) for k in (0, 1, 17, 1000, 5000, 70000, 3)]
    check_against_oracle(mhc, oracle, model, msgs, chunks=(256,))
    res = model.compress_batch(msgs, chunk_symbols=256)
    blobs = [b for b, _, _ in res]
    assert model.decompress_batch(blobs) == msgs
    assert model.decompress_batch(blobs, [s for _, _, s in res], 256, [len(m) for m in msgs]) == msgs
    # every context has a single symbol: the one after it
    counts = np.zeros(65536, dtype=np.uint64)
    for prev in range(256):
        counts[prev * 256 + (prev + 1) % 256] = 7
    model = mhc.Model.from_counts(counts, 1)
    chain = bytes((0x21 + k) % 256 for k in range(3000))
    msgs = [chain[:k] for k in (0, 1, 2, 255, 256, 257, 3000)]
    check_against_oracle(mhc, oracle, model, msgs, chunks=(256,))
    assert model.decompress_batch([b for b, _, _ in model.compress_batch(msgs)]) == msgs


def test_order2_model_is_refused(mhc):
    data = zipf(50000, 2)
    model = mhc.Model.from_data(data, 2)
    with pytest.raises(mhc.MhError) as e:
        model.compress_batch([data[:100], data[100:200]])
    assert e.value.status == mhc.MH_ERR_ARG


def test_truncated_stream_is_reported_alone(mhc):
    msgs = [zipf(k, 30 + k) for k in (3000, 5000, 7000, 100, 9000)]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=1024)
    cut = nbits.copy()
    cut[2] -= 1
    for kw in ({}, dict(sym_off=in_off, index=idx, chunk_symbols=1024)):
        out, so, st = model.decode_batch(payload, out_off, cut, check=False, **kw)
        assert list(st) == [0, 0, mhc.MH_ERR_CORRUPT, 0, 0]
        for i in (0, 1, 3, 4):
            assert out[int(so[i]):int(so[i + 1])] == msgs[i]


def _dev(mhc, a):
    a = np.ascontiguousarray(a)
    return mhc.DeviceBuffer(max(a.nbytes, 16), a if a.nbytes else None)


@pytest.mark.parametrize("kind", ["shared", "set"])
def test_capacity_one_byte_short_leaves_guard_bytes(mhc, kind):
    """Both order-0/1 encoders (one shared model; a model per stream) on batch_ref.tail_batches: the payload ends 0, 1, 2 and 3
    bytes into a dword, cap is exact and then one byte short.  Under the shared model also, as before: a batch with an empty
    stream one byte short on the encoder, and on the index-free decoder."""
    lib = mhc.lib()
    if kind == "set":
        for msgs, ref in batch_ref.tail_batches(lambda m: batch_ref.pack_each(m, 1)[0], zipf):
            models = mhc.ModelSet.from_tables(batch_ref.pack_each(msgs, 1)[1])
            batch_ref.check_tail_and_capacity(mhc, lib.mh_dev_encode_each, lib.mh_dev_encode_each_workspace, models.handle, msgs, ref,
                                    "mh_dev_encode_each, payload %d bytes" % int(ref.pay_off[-1]))
        return
    counts = batch_ref.histogram([zipf(1 << 16, 5)], 1) + np.uint64(1)      # every pair has a code
    codes, shared = batch_ref.oracle_codes(counts, 1), mhc.Model.from_counts(counts, 1)
    for msgs, ref in batch_ref.tail_batches(lambda m: batch_ref.pack(m, *codes, 1), zipf):
        batch_ref.check_tail_and_capacity(mhc, lib.mh_dev_encode_batch, lib.mh_dev_encode_batch_workspace, shared.handle, msgs, ref,
                                "mh_dev_encode_batch, payload %d bytes" % int(ref.pay_off[-1]))
    msgs = [zipf(k, 50 + k) for k in (1000, 0, 2500, 77)]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    data, in_off = mhc.batch_offsets(msgs)
    payload, out_off, nbits, _, _ = model.encode_batch(msgs)
    n, total, pbytes = len(msgs), int(data.size), int(out_off[-1])
    GUARD = 0xA5
    # encode: payload capacity one byte short
    d_data, d_in = _dev(mhc, data), _dev(mhc, in_off)
    d_out = _dev(mhc, np.full(pbytes + 64, GUARD, dtype=np.uint8))
    d_oo, d_nb = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8)
    wsb = lib.mh_dev_encode_batch_workspace(n, total)
    d_ws = mhc.DeviceBuffer(wsb)
    assert lib.mh_dev_encode_batch(model.handle, d_data.ptr, d_in.ptr, n, total, 0x20, d_out.ptr, pbytes - 1, d_oo.ptr, d_nb.ptr,
                                   None, 0, d_ws.ptr, wsb, None) == 0
    assert lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_ERR_CAPACITY
    assert (d_out.download()[pbytes - 1:] == GUARD).all()
    # index-free decode: output capacity one byte short
    d_pl, d_po, d_nbits = _dev(mhc, payload), _dev(mhc, out_off), _dev(mhc, nbits)
    d_o = _dev(mhc, np.full(total + 64, GUARD, dtype=np.uint8))
    d_so, d_st = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    wsd = lib.mh_dev_decode_batch_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    assert lib.mh_dev_decode_batch(model.handle, d_pl.ptr, d_po.ptr, d_nbits.ptr, n, pbytes, 0x20, d_o.ptr, total - 1, d_so.ptr, 0,
                                   None, 0, d_st.ptr, d_wd.ptr, wsd, None) == 0
    assert lib.mh_dev_status(d_wd.ptr, None) == mhc.MH_ERR_CAPACITY
    got = d_o.download()
    assert (got[total - 1:] == GUARD).all()
    assert list(d_st.download(np.int32)) == [0, 0, 0, mhc.MH_ERR_CAPACITY]
    assert got[:1000 + 2500].tobytes() == msgs[0] + msgs[2]


def test_stream_over_walk_cap(mhc):
    lib = mhc.lib()
    rng = np.random.default_rng(9)
    big = rng.integers(0, 256, 1 << 21, dtype=np.uint8).tobytes()     # ~16 Mbit of payload
    msgs = [b"small one", big, zipf(5000, 1)]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    payload, out_off, nbits, _, in_off = model.encode_batch(msgs)
    assert nbits[1] > mhc.BATCH_WALK_MAX_BITS
    n, total = len(msgs), int(in_off[-1])
    d_pl, d_po, d_nb = _dev(mhc, payload), _dev(mhc, out_off), _dev(mhc, nbits)
    d_o, d_so, d_st = mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    wsd = lib.mh_dev_decode_batch_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    assert lib.mh_dev_decode_batch(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(out_off[-1]), 0x20, d_o.ptr, total, d_so.ptr, 0,
                                   None, 0, d_st.ptr, d_wd.ptr, wsd, None) == 0
    assert lib.mh_dev_status(d_wd.ptr, None) == mhc.MH_ERR_ARG
    assert list(d_st.download(np.int32)) == [0, mhc.MH_ERR_ARG, 0]
    out, so, st = model.decode_batch(payload, out_off, nbits)
    assert out == b"".join(msgs) and np.array_equal(so, in_off) and not st.any()


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/markovhuffman not built (needs the reference at build time)")
def test_streams_equal_the_reference_binary(mhc, tmp_path):
    """Table from the genuine binary (-d) on one golden input; messages cut from it and from another golden file (pairs the
    table has no code for included): each batch stream is byte-identical to `markovhuffman msg -e table -o msg.cm`."""
    train = golden()["input_ipsum.txt"]["data"]
    other = golden()["input_wiki_cpp.html"]["data"]
    src = tmp_path / "train"
    src.write_bytes(train)
    table = tmp_path / "t.e"
    subprocess.run([REF_BIN, str(src), "-d", str(table), "-o", str(tmp_path / "t.cm")], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    model = mhc.Model.from_table(table.read_bytes())
    msgs = [train[:1], train[5:300], b"", train[1000:5000], other[:700], other[3000:3017], train[-100:]]
    res = model.compress_batch(msgs)
    for k, (m, (blob, _, _)) in enumerate(zip(msgs, res)):
        f = tmp_path / ("m%d" % k)
        f.write_bytes(m)
        out = tmp_path / ("m%d.cm" % k)
        subprocess.run([REF_BIN, str(f), "-e", str(table), "-o", str(out)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert blob == out.read_bytes(), k
