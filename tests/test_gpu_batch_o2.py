"""Batches of order-2 streams under one shared order-2 model on the GPU (include/mh.h, "BATCHES OF ORDER-2 STREAMS";
extension, parity unpinned): the batch histogram is the sum of the messages' own order-2 histograms, every stream of a batch
is what mh_encode writes for that message alone with the shared model (and what the CPU oracle writes), its index slice is
mh_encode's index, both decoders give the messages back or report per stream what is wrong, and the order-0/1 and order-2
families refuse each other's models."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import bench
from conftest import golden

pytestmark = pytest.mark.gpu

ENC_CHAIN = 4                                   # mh_dev_encode_path: the one-pass order-2 encoder (needs the hot image)


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


def uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed):
    return bench.lorem_block(n, seed)


def tiled_text(n, seed):
    """n bytes of an 8 MiB text block, tiled (the bench's text workload)."""
    base = text(min(n, 8 << 20), seed)
    return (base * (n // len(base) + 1))[:n]


EDGE_LENS = [1, 0, 1, 2, 3, 1, 1, 1, 1, 0, 1, 1023, 1024, 1025, 17, 16, 0, 4097, 2, 1, 1, 3]   # first stream of length 1


def edge_messages(src_fn, seed):
    src = src_fn(sum(EDGE_LENS) + 64, seed)
    out, p = [], 0
    for n in EDGE_LENS:
        out.append(src[p:p + n])
        p += n
    return out


def _dev(mhc, a):
    a = np.ascontiguousarray(a)
    return mhc.DeviceBuffer(max(a.nbytes, 16), a if a.nbytes else None)


# ---------------------------------------------------------------------------------------------------- 1. histogram

@pytest.mark.parametrize("src_fn", [text, zipf, uniform])
def test_batch_histogram_is_the_sum_of_the_oracle_histograms(mhc, oracle, src_fn):
    msgs = edge_messages(src_fn, 3)
    want = np.zeros(1 << 24, dtype=np.uint64)
    for m in msgs:
        want += oracle.histogram_o2(m)
    got = mhc.histogram_o2_batch(msgs)
    assert int(got.sum()) == sum(len(m) for m in msgs)
    assert np.array_equal(got, want)


def test_batch_histogram_other_prev0_is_the_sum_of_single_stream_histograms(mhc):
    lib = mhc.lib()
    msgs = edge_messages(text, 5)
    for prev0 in (0x00, 0x41, 0xFF):
        want = np.zeros(1 << 24, dtype=np.uint64)
        d_counts = mhc.DeviceBuffer((1 << 24) * 8)
        for m in msgs:
            d = _dev(mhc, np.frombuffer(m, dtype=np.uint8))
            mhc._check(lib.mh_dev_histogram_o2(d.ptr, len(m), prev0 << 8 | prev0, d_counts.ptr, None), "mh_dev_histogram_o2")
            want += d_counts.download(np.uint64)
        assert np.array_equal(mhc.histogram_o2_batch(msgs, prev0=prev0), want)


def test_batch_histogram_bad_offsets(mhc):
    lib = mhc.lib()
    data = np.frombuffer(text(100, 1), dtype=np.uint8)
    d_data = _dev(mhc, data)
    d_counts = mhc.DeviceBuffer((1 << 24) * 8)
    wsb = lib.mh_dev_histogram_o2_batch_workspace(100)
    d_ws = mhc.DeviceBuffer(wsb)
    for off in ([0, 60, 40, 100], [0, 40, 60, 99], [3, 40, 60, 100]):
        d_off = _dev(mhc, np.array(off, dtype=np.uint64))
        assert lib.mh_dev_histogram_o2_batch(d_data.ptr, d_off.ptr, 3, 100, 0x20, d_counts.ptr, d_ws.ptr, wsb, None) == 0
        assert lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_ERR_ARG


# ---------------------------------------------------------------------------------------------------- 2. streams = oracle

def check_streams(mhc, oracle, model, counts, msgs, chunks=(256, 1024, 4096), round_trip=True):
    om = oracle.Model.from_counts(counts, 2)
    for c in chunks:
        res = model.compress_batch_o2(msgs, chunk_symbols=c)
        for m, (blob, nb, sl) in zip(msgs, res):
            rblob, rbits = om.compress(m)
            assert nb == rbits and blob == rblob
            sblob, sbits, _ = model.compress(m)
            assert sbits == nb and sblob == blob
            _, _, idx = model.encode(m, chunk_symbols=c)
            assert np.array_equal(sl, idx)
    if round_trip:                                         # (a skipped pair leaves the decoder in another context)
        blobs = [b for b, _, _ in model.compress_batch_o2(msgs)]
        assert model.decompress_batch_o2(blobs) == [bytes(m) for m in msgs]


def test_text_model_hot_path(mhc, oracle):
    msgs = edge_messages(text, 7) + [text(5000, 8), text(70000, 9)]
    counts = mhc.histogram_o2_batch(msgs + [text(1 << 20, 10)])
    model = mhc.Model.from_counts(counts, 2)
    assert model.tile_layout()[0] > 0                      # the live contexts' slot tables: the image is in LDS
    check_streams(mhc, oracle, model, counts, msgs)


def test_zipf_model_l2_path(mhc, oracle):
    msgs = edge_messages(zipf, 11) + [zipf(30000, 12)]
    counts = mhc.histogram_o2_batch(msgs + [zipf(1 << 20, 13)])
    model = mhc.Model.from_counts(counts, 2)
    assert model.tile_layout()[0] == 0                     # millions of live contexts: no slot tables
    check_streams(mhc, oracle, model, counts, msgs)


def test_hot_image_with_escapes(mhc, oracle):
    """A model whose hot image is handed over although a few contexts have no slot: lookups of those escape to L2."""
    lib = mhc.lib()
    rnd = uniform(32, 99)
    body = tiled_text(16 << 20, 14)
    msgs = [body[:3000] + rnd + body[3000:5000], rnd[:5] + body[:100], body[7000:9000]] + edge_messages(text, 15)
    counts = mhc.histogram_o2_batch([body] + msgs)          # (every pair of the messages has a code)
    model = mhc.Model.from_counts(counts, 2)
    assert model.tile_layout()[0] == 0
    # the single-stream encoder runs its one-pass form, which needs the image
    data = np.frombuffer(body[:1 << 20] + rnd, dtype=np.uint8)
    n = data.size
    wsb = lib.mh_dev_encode_workspace(n)
    cap = lib.mh_encode_bound(model.handle, n)
    d_data, d_pl, d_nb, d_ws = _dev(mhc, data), mhc.DeviceBuffer(cap), mhc.DeviceBuffer(8), mhc.DeviceBuffer(wsb)
    mhc._check(lib.mh_dev_encode(model.handle, d_data.ptr, n, 0x20, d_pl.ptr, cap, d_nb.ptr, None, 0, d_ws.ptr, wsb, None), "mh_dev_encode")
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert lib.mh_dev_encode_path(d_ws.ptr, None) == ENC_CHAIN
    check_streams(mhc, oracle, model, counts, msgs)


def test_codes_over_56_bits(mhc, oracle):
    fib = [1, 1]
    while len(fib) < 62:
        fib.append(fib[-1] + fib[-2])
    syms = list(range(62))
    counts = np.zeros(1 << 24, dtype=np.uint64)
    for b2 in syms + [0x20]:
        for b1 in syms + [0x20]:
            ctx = (b2 << 8) | b1
            counts[(ctx << 8):(ctx << 8) + 62] = fib[::-1] if (b1 + b2) % 2 else fib
    model = mhc.Model.from_counts(counts, 2)
    assert model.max_code_len > 56
    rng = np.random.default_rng(16)
    msgs = [bytes(rng.integers(0, 62, int(k)).astype(np.uint8)) for k in (0, 1, 2, 17, 1000, 5000, 3)]
    msgs.append(bytes([0] * 300 + [61] * 300))             # the longest codes, back to back
    check_streams(mhc, oracle, model, counts, msgs, chunks=(256,))


def test_pairs_without_a_code_are_skipped(mhc, oracle):
    counts = mhc.histogram_o2_batch([text(1 << 20, 17)])
    model = mhc.Model.from_counts(counts, 2)
    msgs = [zipf(k, 18 + k) for k in (1, 2, 100, 1025, 9000)] + [text(500, 19) + zipf(500, 20) + text(500, 21)]
    check_streams(mhc, oracle, model, counts, msgs, round_trip=False)


# ---------------------------------------------------------------------------------------------------- 3. round trips

def round_trip(model, msgs, chunk=1024):
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=chunk)
    src = b"".join(msgs)
    out, so, st = model.decode_batch_o2(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=chunk)
    assert out == src and np.array_equal(so, in_off) and not st.any()
    out, so, st = model.decode_batch_o2(payload, out_off, nbits)
    assert out == src and np.array_equal(so, in_off) and not st.any()


def model_for(mhc, msgs):
    """the shared order-2 model of the messages themselves: every pair has a code, so every stream decodes back"""
    return mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)


@pytest.fixture(scope="module")
def text_model(mhc):
    return model_for(mhc, [text(4 << 20, 22)])


def test_empty_batches_and_empty_streams(mhc, text_model):
    assert text_model.compress_batch_o2([]) == []
    assert text_model.decompress_batch_o2([]) == []
    round_trip(text_model, [b""] * 5)
    res = text_model.compress_batch_o2([b"", b"", b""], chunk_symbols=256)
    assert [nb for _, nb, _ in res] == [0, 0, 0]
    assert text_model.decompress_batch_o2([b for b, _, _ in res]) == [b"", b"", b""]


def test_round_trip_65536_streams_of_4k(mhc):
    n, size = 65536, 4096
    src = tiled_text(n * size, 23)
    msgs = [src[i * size:(i + 1) * size] for i in range(n)]
    round_trip(model_for(mhc, msgs), msgs)


def test_round_trip_million_streams_of_256(mhc):
    n, size = 1 << 20, 256
    src = tiled_text(n * size, 24)
    msgs = [src[i * size:(i + 1) * size] for i in range(n)]
    round_trip(model_for(mhc, msgs), msgs, chunk=256)


def test_decompress_with_index_slices(mhc):
    msgs = edge_messages(text, 25)
    text_model = model_for(mhc, msgs)
    res = text_model.compress_batch_o2(msgs, chunk_symbols=256)
    blobs, slices = [b for b, _, _ in res], [s for _, _, s in res]
    assert text_model.decompress_batch_o2(blobs, slices, 256, [len(m) for m in msgs]) == msgs


# ---------------------------------------------------------------------------------------------------- 4. errors per stream

def test_truncated_stream_is_reported_alone(mhc):
    msgs = [text(k, 30 + k) for k in (3000, 5000, 7000, 100, 9000)]
    text_model = model_for(mhc, msgs)
    payload, out_off, nbits, idx, in_off = text_model.encode_batch_o2(msgs, chunk_symbols=1024)
    cut = nbits.copy()
    cut[2] -= 1
    for kw in ({}, dict(sym_off=in_off, index=idx, chunk_symbols=1024)):
        out, so, st = text_model.decode_batch_o2(payload, out_off, cut, check=False, **kw)
        assert list(st) == [0, 0, mhc.MH_ERR_CORRUPT, 0, 0]
        for i in (0, 1, 3, 4):
            assert out[int(so[i]):int(so[i + 1])] == msgs[i]


def test_capacity_one_byte_short_leaves_guard_bytes(mhc):
    lib = mhc.lib()
    msgs = [text(k, 50 + k) for k in (1000, 0, 2500, 77)]
    model = model_for(mhc, msgs)
    data, in_off = mhc.batch_offsets(msgs)
    payload, out_off, nbits, _, _ = model.encode_batch_o2(msgs)
    n, total, pbytes = len(msgs), int(data.size), int(out_off[-1])
    GUARD = 0xA5
    d_data, d_in = _dev(mhc, data), _dev(mhc, in_off)
    d_out = _dev(mhc, np.full(pbytes + 64, GUARD, dtype=np.uint8))
    d_oo, d_nb = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8)
    wsb = lib.mh_dev_encode_batch_o2_workspace(n, total)
    d_ws = mhc.DeviceBuffer(wsb)
    assert lib.mh_dev_encode_batch_o2(model.handle, d_data.ptr, d_in.ptr, n, total, 0x20, d_out.ptr, pbytes - 1, d_oo.ptr, d_nb.ptr,
                                      None, 0, d_ws.ptr, wsb, None) == 0
    assert lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_ERR_CAPACITY
    assert (d_out.download()[pbytes - 1:] == GUARD).all()
    # index-free decode: output capacity one byte short
    d_pl, d_po, d_nbits = _dev(mhc, payload), _dev(mhc, out_off), _dev(mhc, nbits)
    d_o = _dev(mhc, np.full(total + 64, GUARD, dtype=np.uint8))
    d_so, d_st = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    wsd = lib.mh_dev_decode_batch_o2_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    assert lib.mh_dev_decode_batch_o2(model.handle, d_pl.ptr, d_po.ptr, d_nbits.ptr, n, pbytes, 0x20, d_o.ptr, total - 1, d_so.ptr, 0,
                                      None, 0, d_st.ptr, d_wd.ptr, wsd, None) == 0
    assert lib.mh_dev_status(d_wd.ptr, None) == mhc.MH_ERR_CAPACITY
    got = d_o.download()
    assert (got[total - 1:] == GUARD).all()
    assert list(d_st.download(np.int32)) == [0, 0, 0, mhc.MH_ERR_CAPACITY]
    assert got[:1000 + 2500].tobytes() == msgs[0] + msgs[2]


def test_encode_capacity_small_writes_nothing_past_cap(mhc, text_model):
    lib = mhc.lib()
    msgs = [text(k, 60 + k) for k in (4000, 3, 8000)]
    data, in_off = mhc.batch_offsets(msgs)
    n, total = len(msgs), int(data.size)
    GUARD = 0x5A
    cap = 1024
    d_data, d_in = _dev(mhc, data), _dev(mhc, in_off)
    d_out = _dev(mhc, np.full(cap + 4096, GUARD, dtype=np.uint8))
    d_oo, d_nb = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8)
    wsb = lib.mh_dev_encode_batch_o2_workspace(n, total)
    d_ws = mhc.DeviceBuffer(wsb)
    assert lib.mh_dev_encode_batch_o2(text_model.handle, d_data.ptr, d_in.ptr, n, total, 0x20, d_out.ptr, cap, d_oo.ptr, d_nb.ptr,
                                      None, 0, d_ws.ptr, wsb, None) == 0
    assert lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_ERR_CAPACITY
    assert (d_out.download()[cap:] == GUARD).all()
    # batch_ref.tail_batches: the payload ends 0, 1, 2 and 3 bytes into a dword; cap exact, then one byte short
    counts = batch_ref.histogram([text(1 << 16, 23)], 2)
    codes, model = batch_ref.oracle_codes(counts, 2), mhc.Model.from_counts(counts, 2)
    for msgs, ref in batch_ref.tail_batches(lambda m: batch_ref.pack(m, *codes, 2), text):
        assert int(ref.nbits[-1]) > 1024                           # (the model has codes for the text's triples)
        batch_ref.check_tail_and_capacity(mhc, lib.mh_dev_encode_batch_o2, lib.mh_dev_encode_batch_o2_workspace, model.handle, msgs, ref,
                                "mh_dev_encode_batch_o2, payload %d bytes" % int(ref.pay_off[-1]))


def test_stream_over_walk_cap(mhc):
    lib = mhc.lib()
    big = uniform(1 << 21, 9)                                  # ~16 Mbit of payload
    msgs = [b"small one", big, text(5000, 1)]
    counts = mhc.histogram_o2_batch(msgs)
    model = mhc.Model.from_counts(counts, 2)
    payload, out_off, nbits, _, in_off = model.encode_batch_o2(msgs)
    assert nbits[1] > mhc.BATCH_WALK_MAX_BITS
    n, total = len(msgs), int(in_off[-1])
    d_pl, d_po, d_nb = _dev(mhc, payload), _dev(mhc, out_off), _dev(mhc, nbits)
    d_o, d_so, d_st = mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    wsd = lib.mh_dev_decode_batch_o2_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    assert lib.mh_dev_decode_batch_o2(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(out_off[-1]), 0x20, d_o.ptr, total, d_so.ptr, 0,
                                      None, 0, d_st.ptr, d_wd.ptr, wsd, None) == 0
    assert lib.mh_dev_status(d_wd.ptr, None) == mhc.MH_ERR_ARG
    assert list(d_st.download(np.int32)) == [0, mhc.MH_ERR_ARG, 0]
    out, so, st = model.decode_batch_o2(payload, out_off, nbits)
    assert out == b"".join(msgs) and np.array_equal(so, in_off) and not st.any()


# ---------------------------------------------------------------------------------------------------- 5. the use case

def test_wiki_lines_order2_payload(mhc):
    """The lines of input_wiki_cpp.html under one shared model: order 2 writes 100 419 payload bytes against 162 287 for
    order 1 (the CPU oracle's figures)."""
    lines = [ln for ln in golden()["input_wiki_cpp.html"]["data"].split(b"\n") if ln]
    assert len(lines) == 1581
    m1 = mhc.Model.from_counts(mhc.histogram_o1_batch(lines), 1)
    _, out_off1, _, _, _ = m1.encode_batch(lines)
    m2 = mhc.Model.from_counts(mhc.histogram_o2_batch(lines), 2)
    payload, out_off2, nbits2, _, _ = m2.encode_batch_o2(lines)
    assert int(out_off1[-1]) == 162287
    assert int(out_off2[-1]) == 100419
    out, _, st = m2.decode_batch_o2(payload, out_off2, nbits2)
    assert out == b"".join(lines) and not st.any()


# ---------------------------------------------------------------------------------------------------- 6. the families stay apart

def test_order1_model_is_refused_by_the_o2_calls(mhc):
    lib = mhc.lib()
    msgs = [zipf(100, 1), zipf(200, 2)]
    m1 = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    with pytest.raises(mhc.MhError) as e:
        m1.compress_batch_o2(msgs)
    assert e.value.status == mhc.MH_ERR_ARG
    payload, out_off, nbits, _, in_off = m1.encode_batch(msgs)
    with pytest.raises(mhc.MhError) as e:
        m1.decode_batch_o2(payload, out_off, nbits)
    assert e.value.status == mhc.MH_ERR_ARG
    data, _ = mhc.batch_offsets(msgs)
    d_data, d_in = _dev(mhc, data), _dev(mhc, in_off)
    d_out, d_oo, d_nb = mhc.DeviceBuffer(4096), mhc.DeviceBuffer(24), mhc.DeviceBuffer(16)
    wsb = lib.mh_dev_encode_batch_o2_workspace(2, 300)
    d_ws = mhc.DeviceBuffer(wsb)
    assert lib.mh_dev_encode_batch_o2(m1.handle, d_data.ptr, d_in.ptr, 2, 300, 0x20, d_out.ptr, 4096, d_oo.ptr, d_nb.ptr, None, 0,
                                      d_ws.ptr, wsb, None) == mhc.MH_ERR_ARG
    wsd = lib.mh_dev_decode_batch_o2_workspace(2)
    d_wd = mhc.DeviceBuffer(wsd)
    assert lib.mh_dev_decode_batch_o2(m1.handle, d_out.ptr, d_in.ptr, d_nb.ptr, 2, 300, 0x20, d_out.ptr, 4096, d_oo.ptr, 0, None, 0,
                                      None, d_wd.ptr, wsd, None) == mhc.MH_ERR_ARG
