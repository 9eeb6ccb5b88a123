"""Segment states of index-free batches on the GPU (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES"): states + index must
give the index the encoder wrote, states + emit the messages, for a shared model, a model set, a bank view and the reference's
own files; long streams, fixed-length-code lattices, long codes, errors and edge cases.  Checked against the encoder's outputs
and the inputs, never only against each other."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import expected_file, golden, golden_names

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5A5A5A5A5
CHUNKS = (256, 512, 1024, 2048, 4096, 8192)


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    m = entry.load_package()
    if m.device_count() < 1:
        pytest.skip("no GPU")
    return m


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


def text(n, seed=0):
    """Words and line breaks; a long text repeats a 1 MiB block."""
    words = [b"the", b"segment", b"state", b"of", b"a", b"stream", b"decoder", b"batch", b"index", b"huffman", b"markov"]
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < min(n, 1 << 20):
        out += words[int(rng.integers(len(words)))] + (b"\n" if rng.random() < 0.1 else b" ")
    return (bytes(out) * (n // len(out) + 1))[:n] if out else b""


def messages(seed, chunk=1024, big=65536):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, big, 0, 3]
    lens += [int(x) for x in rng.integers(0, big, 20)]
    src = zipf(sum(lens), seed) if seed % 2 == 0 else text(sum(lens), seed)
    out, at = [], 0
    for k in lens:
        out.append(src[at:at + k])
        at += k
    return out


def shared_model(mhc, msgs, order):
    """The batch's shared model, every message counted from prev0 (so that every pair of every message has a code)."""
    return mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=order), order)


def expected_index(enc_idx, in_off, chunk, cap):
    """The encoder's slices in an index of `cap` sentinel entries."""
    want = np.full(cap, SENT, dtype=np.uint64)
    for i in range(len(in_off) - 1):
        b = int(in_off[i]) // chunk + i
        e = b + (int(in_off[i + 1] - in_off[i]) + chunk - 1) // chunk
        want[b:e] = enc_idx[b:e]
    return want


def check_states(mhc, model, msgs, payload, out_off, nbits, enc_idx_by_chunk):
    st = mhc.SegmentStates(model, payload, out_off, nbits)
    in_off = mhc.batch_offsets(msgs)[1]
    assert st.rc == mhc.MH_OK and not st.status.any()
    assert np.array_equal(st.sym_off, in_off)
    for chunk, enc_idx in enc_idx_by_chunk.items():
        cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), chunk)
        idx, status, rc = st.index(chunk)
        assert rc == mhc.MH_OK and not status.any()
        assert np.array_equal(idx, expected_index(enc_idx, in_off, chunk, cap)), chunk
    out, status, rc = st.emit(guard=64)
    assert rc == mhc.MH_OK and not status.any()
    assert out == b"".join(msgs)
    return st


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("seed", [0, 1])
def test_shared_model_index_and_emit_parity(mhc, order, seed):
    msgs = messages(seed)
    model = shared_model(mhc, msgs, order)
    enc = {}
    for chunk in CHUNKS:
        payload, out_off, nbits, idx, _ = model.encode_batch(msgs, chunk_symbols=chunk)
        enc[chunk] = idx
    check_states(mhc, model, msgs, payload, out_off, nbits, enc)
    # the existing index-free decoder writes the same bytes and offsets
    out, so, st = model.decode_batch(payload, out_off, nbits)
    assert out == b"".join(msgs) and np.array_equal(so, mhc.batch_offsets(msgs)[1])
    # and the built index drives the existing indexed decoder
    sym_off, idx, status = model.index_batch(payload, out_off, nbits, 1024)
    out, _, st = model.decode_batch(payload, out_off, nbits, sym_off=sym_off, index=idx, chunk_symbols=1024)
    assert out == b"".join(msgs) and not st.any() and not status.any()
    out, so, status = model.decode_batch_segments(payload, out_off, nbits)
    assert out == b"".join(msgs) and not status.any()


@pytest.mark.parametrize("order", [0, 1])
def test_model_set_and_bank_view_parity(mhc, order):
    msgs = messages(4 + order, big=20000)
    res = mhc.compress_each(msgs, order=order, chunk_symbols=512)
    tables = [t for t, _, _, _ in res]
    s = mhc.ModelSet.from_tables(tables)
    payload, pay_off = mhc.batch_offsets([b[1:] for _, b, _, _ in res])
    nbits = np.array([nb for _, _, nb, _ in res], dtype=np.uint64)
    in_off = mhc.batch_offsets(msgs)[1]
    enc = np.zeros(mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 512), dtype=np.uint64)
    for i, (_, _, _, sl) in enumerate(res):
        b = int(in_off[i]) // 512 + i
        enc[b:b + len(sl)] = sl
    check_states(mhc, s, msgs, payload, pay_off, nbits, {512: enc})
    out, so, st, rc = s.decode(payload, pay_off, nbits)
    assert out == b"".join(msgs) and rc == mhc.MH_OK
    # a bank view (mh_dev_model_set_pick) is an ordinary set
    bank, choice, _ = mhc.ModelSet.train_bank(msgs, 3, order=order)
    view = bank.pick(choice)
    payload, out_off, nbits, idx, _ = mhc.encode_bank(bank, msgs, choice, chunk_symbols=1024)
    check_states(mhc, view, msgs, payload, out_off, nbits, {1024: idx})


def test_reference_files_through_index_each(mhc):
    tables, blobs, inputs = [], [], []
    for name in golden_names():
        for ext, tab in (("cm", "e"), ("ch", "eh")):
            blob, table = expected_file(name, ext), expected_file(name, tab)
            if blob is None or table is None:
                continue
            tables.append(table)
            blobs.append(blob)
            inputs.append(golden()[name]["data"])
    assert len(blobs) >= 4
    sym_off, idx, status = mhc.index_each(tables, blobs, 256)
    assert not status.any()
    assert np.array_equal(sym_off, mhc.batch_offsets(inputs)[1])
    for i, (t, data) in enumerate(zip(tables, inputs)):
        if not data:
            continue
        m = mhc.Model.from_table(t)
        _, _, own = m.encode(data, chunk_symbols=256)
        b = int(sym_off[i]) // 256 + i
        n = (len(data) + 255) // 256
        assert np.array_equal(idx[b:b + n], np.asarray(own, dtype=np.uint64)[:n]), i
    assert mhc.decompress_each(tables, blobs, [idx[int(sym_off[i]) // 256 + i:int(sym_off[i]) // 256 + i + (len(d) + 255) // 256]
                                               for i, d in enumerate(inputs)], 256, [len(d) for d in inputs]) == inputs
    # the set form on the device decodes them too
    s = mhc.ModelSet.from_tables(tables)
    payload, pay_off = mhc.batch_offsets([b[1:] for b in blobs])
    nbits = np.array([mhc.parse_stream_header(mhc.table_order(t), b) for t, b in zip(tables, blobs)], dtype=np.uint64)
    out, so, st = s.decode_batch_segments(payload, pay_off, nbits)
    assert out == b"".join(inputs) and not st.any()


def dev_decode_batch_status(mhc, model, payload, pay_off, nbits):
    """Per-stream statuses of the existing device index-free decode (mh_dev_decode_batch)."""
    l = mhc.lib()
    n = len(pay_off) - 1
    cap = int(sum(int(b) for b in nbits) // max(model.min_code_len, 1))
    d_pl = mhc.DeviceBuffer(len(payload) + 64, np.frombuffer(payload, dtype=np.uint8) if len(payload) else None)
    d_po, d_nb = mhc.DeviceBuffer(pay_off.nbytes, pay_off), mhc.DeviceBuffer(nbits.nbytes, nbits)
    d_out, d_so, d_st = mhc.DeviceBuffer(cap + 16), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    wsb = l.mh_dev_decode_batch_workspace(n)
    d_ws = mhc.DeviceBuffer(wsb)
    assert l.mh_dev_decode_batch(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), mhc.PREV0, d_out.ptr, cap, d_so.ptr, 0,
                                 None, 0, d_st.ptr, d_ws.ptr, wsb, None) == mhc.MH_OK
    l.mh_dev_status(d_ws.ptr, None)
    return d_st.download(np.int32)[:n]


@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_streams_over_the_walk_cap(mhc, kind):
    gen = zipf if kind == "zipf" else text
    rng = np.random.default_rng(11)
    msgs = [gen(int(k), int(s)) for s, k in enumerate(rng.integers(0, 4096, 300))]
    msgs[17] = gen(2 << 20, 101)
    msgs[150] = gen(64 << 20, 102)
    model = shared_model(mhc, msgs, 1)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=1024)
    payload = payload.tobytes()
    st = dev_decode_batch_status(mhc, model, payload, out_off, nbits)
    assert st[150] == mhc.MH_ERR_ARG and (nbits[17] <= mhc.BATCH_WALK_MAX_BITS or st[17] == mhc.MH_ERR_ARG)
    check_states(mhc, model, msgs, payload, out_off, nbits, {1024: idx})
    sym_off, built, status = model.index_batch(payload, out_off, nbits, 1024)
    assert not status.any()
    out, _, st = model.decode_batch(payload, out_off, nbits, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert out == b"".join(msgs) and not st.any()
    assert dev_decode_batch_indexed(mhc, model, payload, out_off, nbits, sym_off, built, 1024) == b"".join(msgs)
    lookups = [(150, 33 << 20, (33 << 20) + 4096), (17, 0, 100), (150, (64 << 20) - 7, 64 << 20), (3, 0, len(msgs[3]))]
    want = [msgs[i][b:e] for i, b, e in lookups]
    got, lst = model.decode_batch_ranges(payload, out_off, nbits, lookups, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert not lst.any() and got == want
    got, lst, rc = model.dev_decode_batch_ranges(payload, out_off, nbits, lookups, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not lst.any() and got == want
    # the set form (every stream under the same model) builds the same index, which drives mh_dev_decode_each_ranges
    s = mhc.ModelSet.from_models([model] * len(msgs))
    sym_off2, built2, status = s.index_batch(payload, out_off, nbits, 1024)
    assert not status.any() and np.array_equal(sym_off2, in_off) and np.array_equal(built2, built)
    got, lst, rc = s.decode_ranges(payload, out_off, nbits, lookups, sym_off=sym_off2, index=built2, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not lst.any() and got == want


def dev_decode_batch_indexed(mhc, model, payload, pay_off, nbits, sym_off, index, chunk):
    """The bytes the existing device decoder (mh_dev_decode_batch) writes with the index handed in."""
    l = mhc.lib()
    n = len(pay_off) - 1
    total = int(sym_off[n])
    index = np.ascontiguousarray(index, dtype=np.uint64)
    d_pl = mhc.DeviceBuffer(len(payload) + 64, np.frombuffer(payload, dtype=np.uint8) if len(payload) else None)
    d_po, d_nb = mhc.DeviceBuffer(pay_off.nbytes, pay_off), mhc.DeviceBuffer(nbits.nbytes, nbits)
    d_so, d_idx = mhc.DeviceBuffer(sym_off.nbytes, np.ascontiguousarray(sym_off)), mhc.DeviceBuffer(index.nbytes, index)
    d_out, d_st = mhc.DeviceBuffer(total + 16), mhc.DeviceBuffer(n * 4)
    wsb = l.mh_dev_decode_batch_workspace(n)
    d_ws = mhc.DeviceBuffer(wsb)
    assert l.mh_dev_decode_batch(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), mhc.PREV0, d_out.ptr, total, d_so.ptr,
                                 total, d_idx.ptr, chunk, d_st.ptr, d_ws.ptr, wsb, None) == mhc.MH_OK
    assert l.mh_dev_status(d_ws.ptr, None) == mhc.MH_OK and not d_st.download(np.int32)[:n].any()
    return d_out.download()[:total].tobytes()


def test_lattice_streams(mhc):
    """Fixed-length codes: uniform bytes under 8-bit codes (every segment boundary is a code boundary), and uniform symbols
    0..7 under 3-bit codes, where a segment decoded from a guess stays out of phase for good: the walk covers those, and
    one longer than MH_BATCH_WALK_MAX_BITS is refused by the device form but indexed by the host form."""
    model = mhc.Model.from_counts(np.ones(256, dtype=np.uint64), 0)
    assert model.max_code_len == 8 and model.min_code_len == 8
    rng = np.random.default_rng(5)
    msgs = [rng.integers(0, 256, 4096, dtype=np.uint8).tobytes() for _ in range(12)] + [rng.integers(0, 256, 2 << 20, dtype=np.uint8).tobytes()]
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    check_states(mhc, model, msgs, payload, out_off, nbits, {256: idx})
    counts = np.zeros(256, dtype=np.uint64)
    counts[:8] = 1
    model = mhc.Model.from_counts(counts, 0)
    assert model.max_code_len == 3 and model.min_code_len == 3
    msgs = [rng.integers(0, 8, 4096, dtype=np.uint8).tobytes() for _ in range(12)]
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    check_states(mhc, model, msgs, payload, out_off, nbits, {256: idx})
    msgs.insert(5, rng.integers(0, 8, 3 << 20, dtype=np.uint8).tobytes())     # 9.4 Mbit
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    st = mhc.SegmentStates(model, payload, out_off, nbits)
    assert st.rc == mhc.MH_ERR_ARG and st.status[5] == mhc.MH_ERR_ARG
    assert not np.delete(st.status, 5).any()
    out, status, _ = st.emit()
    so = st.sym_off
    for i, m in enumerate(msgs):
        if i != 5:
            assert out[int(so[i]):int(so[i + 1])] == m
    assert so[6] == so[5]
    sym_off, built, status = mhc.index_batch_host(model, payload, out_off, nbits, 256)
    assert not status.any() and np.array_equal(sym_off, in_off)
    cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 256)
    exp = expected_index(idx, in_off, 256, cap)
    mask = exp != SENT
    assert np.array_equal(built[mask], exp[mask])


def test_lattice_streams_under_a_model_set(mhc):
    """The same 3-bit lattice under the set form: the per-stream-model walk (4 KiB streams exact), the device refusal of the
    9.4 Mbit stream, and mh_index_each, which indexes that stream alone under the model parsed from its table file."""
    counts = np.zeros(256, dtype=np.uint64)
    counts[:8] = 1
    model = mhc.Model.from_counts(counts, 0)
    rng = np.random.default_rng(6)
    msgs = [rng.integers(0, 8, int(k), dtype=np.uint8).tobytes() for k in [4096] * 10 + [0, 1, 5000]]
    msgs.insert(4, rng.integers(0, 8, 3 << 20, dtype=np.uint8).tobytes())     # 9.4 Mbit
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    short = [m for i, m in enumerate(msgs) if i != 4]
    p_s, o_s, nb_s, idx_s, _ = model.encode_batch(short, chunk_symbols=256)
    s_short = mhc.ModelSet.from_models([model] * len(short))
    check_states(mhc, s_short, short, p_s, o_s, nb_s, {256: idx_s})
    s = mhc.ModelSet.from_models([model] * len(msgs))
    st = mhc.SegmentStates(s, payload, out_off, nbits)
    assert st.rc == mhc.MH_ERR_ARG and st.status[4] == mhc.MH_ERR_ARG and not np.delete(st.status, 4).any()
    out, status, _ = st.emit()
    for i, m in enumerate(msgs):
        if i != 4:
            assert out[int(st.sym_off[i]):int(st.sym_off[i + 1])] == m
    table = model.table_bytes()
    blobs = [bytes([mhc.stream_header(0, int(nbits[i]))]) + payload[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(len(msgs))]
    sym_off, built, status = mhc.index_each([table] * len(msgs), blobs, 256)
    assert not status.any() and np.array_equal(sym_off, in_off)
    cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 256)
    exp = expected_index(idx, in_off, 256, cap)
    mask = exp != SENT
    assert np.array_equal(built[mask], exp[mask])


def test_codes_longer_than_15_bits(mhc):
    fib = [1, 1]
    while len(fib) < 26:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(65536, dtype=np.uint64)
    for prev in range(256):
        counts[prev * 256: prev * 256 + 26] = fib[::-1] if prev % 2 else fib
    model = mhc.Model.from_counts(counts, 1)
    assert model.max_code_len > 15
    rng = np.random.default_rng(8)
    msgs = [bytes(rng.integers(0, 26, int(k)).astype(np.uint8)) for k in (0, 1, 17, 1000, 5000, 70000, 3)]
    msgs.append(bytes([25, 24, 23] * 3000))                      # the rare, long codes back to back
    enc = {}
    for chunk in (256, 4096):
        payload, out_off, nbits, idx, _ = model.encode_batch(msgs, chunk_symbols=chunk)
        enc[chunk] = idx
    check_states(mhc, model, msgs, payload, out_off, nbits, enc)


def test_errors_stay_in_their_stream(mhc):
    msgs = messages(2, big=30000)
    model = shared_model(mhc, msgs, 1)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
    k = 9                                                       # the `big` stream
    assert len(msgs[k]) > 1000
    # nbits cut inside the stream's final code: MH_ERR_CORRUPT for it alone
    cut = nbits.copy()
    cut[k] -= 1
    st = mhc.SegmentStates(model, payload, out_off, cut)
    assert st.rc == mhc.MH_ERR_CORRUPT and st.status[k] == mhc.MH_ERR_CORRUPT and not np.delete(st.status, k).any()
    out, status, _ = st.emit()
    for i, m in enumerate(msgs):
        if i != k:
            assert out[int(st.sym_off[i]):int(st.sym_off[i + 1])] == m
    # nbits beyond the payload bytes: MH_ERR_ARG
    over = nbits.copy()
    over[k] = (int(out_off[k + 1]) - int(out_off[k])) * 8 + 1
    st2 = mhc.SegmentStates(model, payload, out_off, over)
    assert st2.status[k] == mhc.MH_ERR_ARG and not np.delete(st2.status, k).any()
    # capacities: nothing written at or beyond the caps
    good = mhc.SegmentStates(model, payload, out_off, nbits)
    total = int(good.sym_off[-1])
    cap = mhc.lib().mh_batch_index_capacity(total, len(msgs), 256)
    _, status, rc = good.index(256, index_cap=cap - 1, guard=8)
    assert rc == mhc.MH_ERR_CAPACITY and (status == mhc.MH_ERR_CAPACITY).all()    # a call-wide error reaches every stream
    small = int(good.sym_off[k + 1]) - 1
    out, status, rc = good.emit(out_cap=small, guard=64)
    assert rc == mhc.MH_ERR_CAPACITY and status[k] == mhc.MH_ERR_CAPACITY and not status[:k].any()
    assert out[:int(good.sym_off[k])] == b"".join(msgs[:k])
    # states of another batch: MH_ERR_ARG
    other = mhc.SegmentStates(model, payload, out_off, nbits)
    _, status, rc = good.index(256, ws=st)
    assert rc == mhc.MH_ERR_ARG and (status == mhc.MH_ERR_ARG).all()
    _, status, rc = other.emit(ws=good)
    assert rc == mhc.MH_ERR_ARG and (status == mhc.MH_ERR_ARG).all()
    # offsets out of order: MH_ERR_ARG for the call and every stream
    bad = out_off.copy()
    bad[3], bad[4] = bad[4], bad[3]
    if bad[3] != bad[4]:
        st3 = mhc.SegmentStates(model, payload, bad, nbits)
        assert st3.rc == mhc.MH_ERR_ARG and (st3.status == mhc.MH_ERR_ARG).all()
    idx2, _, rc = good.index(256)                               # its own workspace still holds its states
    assert rc == mhc.MH_OK
    # an order-2 model is refused before any launch
    m2 = mhc.Model.from_data(zipf(50000, 2), 2)
    with pytest.raises(mhc.MhError) as e:
        mhc.SegmentStates(m2, payload, out_off, nbits)
    assert e.value.status == mhc.MH_ERR_ARG


def test_edges_and_determinism(mhc):
    msgs = messages(6)
    model = shared_model(mhc, msgs + [zipf(3000, 4), zipf(1, 5)], 1)
    for msgs in ([], [b""] * 5, [zipf(3000, 4)], [b"", zipf(1, 5), b""]):
        payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=256)
        check_states(mhc, model, msgs, payload, out_off, nbits, {256: idx if idx is not None else np.zeros(1, np.uint64)})
    msgs = messages(6)
    payload, out_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=1024)
    a = mhc.SegmentStates(model, payload, out_off, nbits)
    b = mhc.SegmentStates(model, payload, out_off, nbits)
    assert np.array_equal(a.sym_off, b.sym_off)
    assert np.array_equal(a.index(1024)[0], b.index(1024)[0])
    assert a.emit()[0] == b.emit()[0] == b"".join(msgs)
