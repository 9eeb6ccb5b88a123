"""Segment states of index-free order-2 batches on the GPU (include/mh.h, "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES"):
states + index must give the index mh_dev_encode_batch_o2 wrote, states + emit the messages; streams over the walk cap,
the convergence of the order-2 speculation (through mh_dev_batch_states_stats: exact outputs cannot show a silent one-lane
walk), a lattice that never synchronises, damage, long codes, edges, reused workspaces and a non-default stream.  Checked
against the encoder's outputs, the inputs and the strict CPU oracle, never only against each other.  Models are trained on
the batch with histogram_o2_batch unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import damage
from oracle import mh_oracle
from test_gpu_batch_states import CHUNKS, SENT, expected_index, messages, text, zipf

pytestmark = pytest.mark.gpu

PREV0 = 0x20


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    m = entry.load_package()
    if m.device_count() < 1:
        pytest.skip("no GPU")
    return m


def o2_model(mhc, msgs):
    return mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)


def check_states(mhc, model, msgs, payload, out_off, nbits, enc_idx_by_chunk):
    st = mhc.SegmentStates(model, payload, out_off, nbits, o2=True)
    in_off = mhc.batch_offsets(msgs)[1]
    assert st.rc == mhc.MH_OK and not st.status.any()
    assert np.array_equal(st.sym_off, in_off)
    for chunk, enc_idx in enc_idx_by_chunk.items():
        cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), chunk)
        idx, status, rc = st.index(chunk, guard=8)
        assert rc == mhc.MH_OK and not status.any()
        assert np.array_equal(idx, expected_index(enc_idx, in_off, chunk, cap)), chunk
    out, status, rc = st.emit(guard=64)
    assert rc == mhc.MH_OK and not status.any()
    assert out == b"".join(msgs)
    return st


def dev_decode_o2(mhc, model, pay, off, nb, sym_off=None, index=None, chunk_symbols=0):
    """One mh_dev_decode_batch_o2 call: (the message of every stream that passed, b"" for the others; status[n])."""
    lib = mhc.lib()
    n = len(off) - 1
    pay, off, nb = (np.ascontiguousarray(a) for a in (np.frombuffer(bytes(pay), dtype=np.uint8), off, nb))
    indexed = index is not None
    cap = int(sym_off[n]) if indexed else sum(int(b) for b in nb) // max(model.min_code_len, 1) + 64
    d_pl, d_po, d_nb = mhc.DeviceBuffer(pay.size + 64, pay if pay.size else None), mhc.DeviceBuffer(off.nbytes, off), mhc.DeviceBuffer(max(nb.nbytes, 8), nb if n else None)
    d_o, d_st = mhc.DeviceBuffer(cap + 64), mhc.DeviceBuffer(max(n, 1) * 4)
    d_so = mhc.DeviceBuffer((n + 1) * 8, np.ascontiguousarray(sym_off, dtype=np.uint64) if indexed else None)
    d_idx = mhc.DeviceBuffer(max(index.nbytes, 8), np.ascontiguousarray(index)) if indexed else None
    ws = lib.mh_dev_decode_batch_o2_workspace(n)
    d_ws = mhc.DeviceBuffer(ws)
    assert lib.mh_dev_decode_batch_o2(model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(off[n]), PREV0, d_o.ptr, cap, d_so.ptr,
                                      int(sym_off[n]) if indexed else 0, d_idx.ptr if indexed else None, chunk_symbols, d_st.ptr, d_ws.ptr, ws,
                                      None) == 0
    lib.mh_dev_status(d_ws.ptr, None)
    st, so, out = d_st.download(np.int32)[:n], d_so.download(np.uint64), d_o.download(np.uint8)
    return [out[int(so[k]):int(so[k + 1])].tobytes() if st[k] == 0 else b"" for k in range(n)], st


# ---------------------------------------------------------------------------------------------------- parity

@pytest.mark.parametrize("seed", [0, 1])
def test_index_and_emit_parity(mhc, seed):
    msgs = messages(seed)
    joined = b"".join(msgs)
    model = o2_model(mhc, msgs)
    enc = {}
    for chunk in CHUNKS:
        payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=chunk)
        enc[chunk] = idx
    st = check_states(mhc, model, msgs, payload, out_off, nbits, enc)
    print("seed %d: repair passes that did work, streams walked: %s" % (seed, st.states_stats()))
    # the index-free decoder writes the same bytes and offsets
    out, so, _ = model.decode_batch_o2(payload, out_off, nbits)
    assert out == joined and np.array_equal(so, in_off)
    out, so, status = model.decode_batch_segments_o2(payload, out_off, nbits)
    assert out == joined and np.array_equal(so, in_off) and not status.any()
    # the built index drives the indexed decoder, the lookups and the indexed search
    sym_off, built, status = model.index_batch_o2(payload, out_off, nbits, 1024)
    assert not status.any() and np.array_equal(sym_off, in_off)
    out, _, dst = model.decode_batch_o2(payload, out_off, nbits, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert out == joined and not dst.any()
    got, dst = dev_decode_o2(mhc, model, payload, out_off, nbits, sym_off, built, 1024)
    assert got == msgs and not dst.any()
    big = max(range(len(msgs)), key=lambda i: len(msgs[i]))
    lookups = [(big, 0, 100), (big, 30000, 34096), (big, len(msgs[big]) - 7, len(msgs[big])), (5, 0, len(msgs[5])), (7, 1023, 1024)]
    want = [msgs[i][b:e] for i, b, e in lookups]
    got, lst, rc = model.dev_decode_batch_o2_ranges(payload, out_off, nbits, lookups, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not lst.any() and got == want
    ps = mhc.PatternSet([b"the ", bytes([0, 1]), b"a"])
    free = model.dev_find_batch_o2(ps, payload, out_off, nbits)
    with_index = model.dev_find_batch_o2(ps, payload, out_off, nbits, sym_off=sym_off, index=built, chunk_symbols=1024)
    assert int(free[0][-1]) > 0
    for a, b in zip(free[:4], with_index[:4]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- over the walk cap, convergence

@pytest.fixture(scope="module")
def over_cap(mhc):
    """kind -> the batch of 300 small streams with one long one (16.6 / 11.7 Mbit under its model) and its states."""
    made = {}

    def get(kind):
        if kind not in made:
            gen, size = (zipf, 3 << 20) if kind == "zipf" else (text, 8 << 20)
            rng = np.random.default_rng(11)
            msgs = [gen(int(k), int(s)) for s, k in enumerate(rng.integers(0, 4096, 300))]
            msgs[17] = gen(size, 102)
            model = o2_model(mhc, msgs)
            payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=1024)
            payload = payload.tobytes()
            st = mhc.SegmentStates(model, payload, out_off, nbits, o2=True)
            made[kind] = (msgs, model, payload, out_off, nbits, idx, in_off, st)
        return made[kind]
    return get


@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_streams_over_the_walk_cap(mhc, over_cap, kind):
    msgs, model, payload, out_off, nbits, idx, in_off, st = over_cap(kind)
    assert nbits[17] > mhc.BATCH_WALK_MAX_BITS
    _, free = dev_decode_o2(mhc, model, payload, out_off, nbits)
    assert free[17] == mhc.MH_ERR_ARG and not np.delete(free, 17).any()      # the one-lane decode refuses it
    print("%s: %.2f Mbit, passes that did work %d, streams walked %d" % ((kind, int(nbits[17]) / 1e6) + st.states_stats()))
    assert st.rc == mhc.MH_OK and not st.status.any()                         # the states settle
    assert np.array_equal(st.sym_off, in_off)
    cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 1024)
    built, status, rc = st.index(1024, guard=8)
    assert rc == mhc.MH_OK and not status.any() and np.array_equal(built, expected_index(idx, in_off, 1024, cap))
    out, status, rc = st.emit(guard=64)
    assert rc == mhc.MH_OK and not status.any() and out == b"".join(msgs)
    n17 = len(msgs[17])
    lookups = [(17, 0, 100), (17, n17 // 2, n17 // 2 + 4096), (17, n17 - 7, n17), (3, 0, len(msgs[3]))]
    want = [msgs[i][b:e] for i, b, e in lookups]
    got, lst, rc = model.dev_decode_batch_o2_ranges(payload, out_off, nbits, lookups, sym_off=st.sym_off, index=built, chunk_symbols=1024)
    assert rc == mhc.MH_OK and not lst.any() and got == want


@pytest.mark.parametrize("kind", ["text", "zipf"])
def test_convergence_small_streams(mhc, kind):
    """At most 1 stream in 20 is left to the one-lane walk (the CPU model of tests/states_o2_ref.py: 0 of 30 and 0 of 40; with
    the order-0/1 rule 18 of 30 and 19 of 40)."""
    msgs = [text(8192, s) for s in range(30)] if kind == "text" else [zipf(4096, s) for s in range(40)]
    model = o2_model(mhc, msgs)
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=256)
    st = check_states(mhc, model, msgs, payload, out_off, nbits, {256: idx})
    passes, walked = st.states_stats()
    print("%s: %d streams, passes that did work %d, streams walked %d" % (kind, len(msgs), passes, walked))
    assert walked * 20 <= len(msgs)
    assert passes <= 8


@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_convergence_over_the_cap(mhc, over_cap, kind):
    """A stream over the cap that were left to the walk would be refused: MH_OK for stream 17 is the condition.  (Not pinned to
    the CPU model's figures: bits past the end of a payload are decoded differently by kernel and model.)"""
    msgs, model, payload, out_off, nbits, idx, in_off, st = over_cap(kind)
    passes, walked = st.states_stats()
    assert st.status[17] == mhc.MH_OK
    assert walked * 20 <= len(msgs) and 1 <= passes <= 8


def test_stats_of_the_order_1_call_and_of_no_states(mhc):
    """The walk counter is there for all policies; a workspace without states is MH_ERR_ARG."""
    msgs = [text(8192, s) for s in range(6)]
    m1 = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=1), 1)
    payload, out_off, nbits, idx, in_off = m1.encode_batch(msgs, chunk_symbols=256)
    st = mhc.SegmentStates(m1, payload, out_off, nbits)
    passes, walked = st.states_stats()
    assert 0 <= passes <= 8 and walked <= len(msgs)
    blank = mhc.DeviceBuffer(4096, np.zeros(4096, dtype=np.uint8))
    p, w = C.c_uint32(0), C.c_uint64(0)
    assert mhc.lib().mh_dev_batch_states_stats(blank.ptr, None, C.byref(p), C.byref(w)) == mhc.MH_ERR_ARG


# ---------------------------------------------------------------------------------------------------- lattices

def lattice_counts(rows):
    """Order-2 counts with count 1 for every (context, symbol) of rows: {context: symbols}."""
    counts = np.zeros(1 << 24, dtype=np.uint64)
    for ctx, syms in rows.items():
        counts[ctx * 256 + np.asarray(syms)] = 1
    return counts


def check_lattice(mhc, model, short, long_msg, walked_expected):
    """The short streams alone: exact, walked as expected.  With long_msg at place 5: refused alone by the device form (every
    other stream exact), indexed by the host form."""
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(short, chunk_symbols=256)
    st = check_states(mhc, model, short, payload, out_off, nbits, {256: idx})
    passes, walked = st.states_stats()
    print("lattice: %d short streams, passes that did work %d, streams walked %d" % (len(short), passes, walked))
    assert walked_expected(walked)
    msgs = list(short)
    msgs.insert(5, long_msg)
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=256)
    assert nbits[5] > mhc.BATCH_WALK_MAX_BITS
    return msgs, payload, out_off, nbits, idx, in_off, mhc.SegmentStates(model, payload, out_off, nbits, o2=True)


def check_refused_alone(mhc, model, msgs, payload, out_off, nbits, idx, in_off, st):
    assert st.rc == mhc.MH_ERR_ARG and st.status[5] == mhc.MH_ERR_ARG and not np.delete(st.status, 5).any()
    out, status, _ = st.emit()
    so = st.sym_off
    for i, m in enumerate(msgs):
        if i != 5:
            assert out[int(so[i]):int(so[i + 1])] == m
    assert so[6] == so[5]
    sym_off, built, status = mhc.index_batch_host_o2(model, payload, out_off, nbits, 256)
    assert not status.any() and np.array_equal(sym_off, in_off)
    cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 256)
    exp = expected_index(idx, in_off, 256, cap)
    mask = exp != SENT
    assert np.array_equal(built[mask], exp[mask])


def test_never_synchronising_streams(mhc):
    """An 8-symbol uniform alphabet: 3-bit codes in every context, out of phase with 512.  A segment decoded from a guess that
    is out of phase stays out of phase for good (every 3-bit pattern is a code), and a repair pass hands a wrong end on to the
    next segment even where that one's own guess was right, so each pass mends one segment per stream (the CPU model of
    tests/states_o2_ref.py: 22 wrong entries of 24 segments, 14 after the 8 passes).  Streams under the cap are walked and
    exact; one of 3 MiB (9.4 Mbit) is refused alone by the device form and indexed by mh_index_batch_o2."""
    S = np.arange(8)
    rows = {PREV0 << 8 | PREV0: S}
    for a in S:
        rows[PREV0 << 8 | int(a)] = S
        for b in S:
            rows[int(a) << 8 | int(b)] = S
    model = mhc.Model.from_counts(lattice_counts(rows), 2)
    assert model.type == 2 and model.min_code_len == 3 and model.max_code_len == 3
    rng = np.random.default_rng(5)
    short = [rng.integers(0, 8, 4096, dtype=np.uint8).tobytes() for _ in range(12)]
    args = check_lattice(mhc, model, short, rng.integers(0, 8, 3 << 20, dtype=np.uint8).tobytes(), lambda walked: walked == 12)
    check_refused_alone(mhc, model, *args)


# ---------------------------------------------------------------------------------------------------- damage

@pytest.mark.parametrize("kind", ["flip", "flip_late", "cut", "nbits_beyond"])
def test_damage_gets_the_decoders_and_the_oracles_verdicts(mhc, kind):
    msgs = messages(3, big=30000)
    counts = mhc.histogram_o2_batch(msgs)
    model = mhc.Model.from_counts(counts, 2)
    om = mh_oracle.Model.from_counts(counts, 2)
    pay, off, nb, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=256)
    pay, nb = np.array(pay, copy=True), np.array(nb, copy=True)
    k = 9                                                       # the `big` stream
    assert len(msgs[k]) == 30000
    if kind == "flip":
        pay[int(off[k]) + int(nb[k]) // 16] ^= 0x10
    elif kind == "flip_late":
        pay[int(off[k]) + int(nb[k]) // 8 - 40] ^= 0x01
    elif kind == "cut":                                           # one bit into the last code of two bits or more
        bounds = damage.boundaries(batch_ref.oracle_codes(counts, 2)[0], np.frombuffer(msgs[k], dtype=np.uint8), 2, PREV0 << 8 | PREV0)
        assert bounds[-1] == nb[k]
        nb[k] = np.uint64(bounds[np.flatnonzero(np.diff(bounds) >= 2)[-1]] + 1)
    else:
        nb[k] = np.uint64((int(off[k + 1]) - int(off[k])) * 8 + 1)
    good, want = dev_decode_o2(mhc, model, pay, off, nb)
    st = mhc.SegmentStates(model, pay, off, nb, o2=True)
    assert np.array_equal(st.status, want), (st.status[k], want[k])
    if kind == "nbits_beyond":
        assert want[k] == mhc.MH_ERR_ARG
    else:
        v, data = damage.verdict_free(om, pay[int(off[k]):int(off[k + 1])].tobytes(), int(nb[k]), PREV0 << 8 | PREV0)
        assert want[k] == v
        if v == damage.MH_OK:
            assert good[k] == data
        if kind == "cut":
            assert v == damage.MH_ERR_CORRUPT
    out, status, _ = st.emit(guard=64)
    for i, m in enumerate(msgs):
        a, b = int(st.sym_off[i]), int(st.sym_off[i + 1])
        if i != k:
            assert out[a:b] == m and st.status[i] == mhc.MH_OK
        elif want[k] != mhc.MH_OK:
            assert a == b                                        # a failed stream counts 0 symbols
        else:
            assert out[a:b] == good[k]
    assert np.array_equal(status, want)


def test_a_code_over_15_bits(mhc):
    ctxs = [PREV0 << 8 | PREV0] + [PREV0 << 8 | s for s in range(26)] + [a << 8 | b for a in range(26) for b in range(26)]
    counts = batch_ref.deep_counts(2, 26, ctxs)
    model = mhc.Model.from_counts(counts, 2)
    assert model.max_code_len > 15
    rng = np.random.default_rng(8)
    msgs = [bytes(rng.integers(0, 26, int(k)).astype(np.uint8)) for k in (0, 1, 17, 1000, 5000, 70000, 3)]
    msgs.append(bytes([25, 24, 23] * 3000))                      # rare symbols back to back
    msgs.append(bytes([0, 1] * 4000))
    enc = {}
    for chunk in (256, 4096):
        payload, out_off, nbits, idx, _ = model.encode_batch_o2(msgs, chunk_symbols=chunk)
        enc[chunk] = idx
    lens = batch_ref.oracle_codes(counts, 2)[0]
    assert batch_ref.pack(msgs, lens, lens * 0, 2).used.max() > 15   # a code over 15 bits is in the payload
    check_states(mhc, model, msgs, payload, out_off, nbits, enc)


# ---------------------------------------------------------------------------------------------------- edges

def test_edges_capacities_and_foreign_workspaces(mhc):
    base = messages(6, big=30000)
    model = o2_model(mhc, base + [zipf(3000, 4), zipf(1, 5), bytes([7])])
    for msgs in ([], [b""] * 5, [zipf(3000, 4)], [b"", zipf(1, 5), b""], [bytes([7])] * 3):
        payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=256)
        check_states(mhc, model, msgs, payload, out_off, nbits, {256: idx if idx is not None else np.zeros(1, np.uint64)})
    msgs = base
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=256)
    good = mhc.SegmentStates(model, payload, out_off, nbits, o2=True)
    total, k = int(good.sym_off[-1]), 9
    cap = mhc.lib().mh_batch_index_capacity(total, len(msgs), 256)
    built, status, rc = good.index(256, index_cap=cap - 1, guard=8)
    assert rc == mhc.MH_ERR_CAPACITY and (status == mhc.MH_ERR_CAPACITY).all() and (built == SENT).all()     # nothing written
    small = int(good.sym_off[k + 1]) - 1
    out, status, rc = good.emit(out_cap=small, guard=64)
    assert rc == mhc.MH_ERR_CAPACITY and status[k] == mhc.MH_ERR_CAPACITY and not status[:k].any()
    assert out[:int(good.sym_off[k])] == b"".join(msgs[:k])
    raw = np.frombuffer(out, dtype=np.uint8)
    assert (raw[int(good.sym_off[k]):] == 0xA5).all()           # the stream that does not fit, and those behind it, wrote nothing
    # the states of another batch
    cut = nbits.copy()
    cut[k] -= 1
    other = mhc.SegmentStates(model, payload, out_off, cut, o2=True)
    assert other.rc == mhc.MH_ERR_CORRUPT and other.status[k] == mhc.MH_ERR_CORRUPT
    _, status, rc = good.index(256, ws=other)
    assert rc == mhc.MH_ERR_ARG and (status == mhc.MH_ERR_ARG).all()
    _, status, rc = good.emit(ws=other)
    assert rc == mhc.MH_ERR_ARG and (status == mhc.MH_ERR_ARG).all()
    # the states of the order-1 call on the very same buffers, and the other way round
    m1 = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=1), 1)
    lib = mhc.lib()

    def run(fn, m, *tail):
        rc = fn(m.handle, good.d_pl.ptr, good.d_po.ptr, good.d_nb.ptr, good.n, good.pay_total, PREV0, *tail, good.d_ws.ptr, good.wsb, None)
        assert rc == mhc.MH_OK
        return lib.mh_dev_status(good.d_ws.ptr, None)
    d_idx, d_out, d_st = mhc.DeviceBuffer(cap * 8), mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer(len(msgs) * 4)
    assert run(lib.mh_dev_batch_index, m1, d_idx.ptr, cap, 256, d_st.ptr) == mhc.MH_ERR_ARG          # order-2 states, order-1 call
    assert (d_st.download(np.int32)[:len(msgs)] == mhc.MH_ERR_ARG).all()
    assert run(lib.mh_dev_batch_emit, m1, d_out.ptr, total, d_st.ptr) == mhc.MH_ERR_ARG
    run(lib.mh_dev_batch_states, m1, good.d_so.ptr, d_st.ptr)                                          # now order-1 states (of an order-2 payload: any verdict)
    assert run(lib.mh_dev_batch_index_o2, model, d_idx.ptr, cap, 256, d_st.ptr) == mhc.MH_ERR_ARG
    assert (d_st.download(np.int32)[:len(msgs)] == mhc.MH_ERR_ARG).all()
    assert run(lib.mh_dev_batch_emit_o2, model, d_out.ptr, total, d_st.ptr) == mhc.MH_ERR_ARG
    # the Python wrapper keeps the order-0/1 calls for a model it is not told about
    with pytest.raises(mhc.MhError) as e:
        mhc.SegmentStates(model, payload, out_off, nbits)
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.SegmentStates(m1, payload, out_off, nbits, o2=True)
    assert e.value.status == mhc.MH_ERR_ARG


def test_dirty_and_recycled_workspaces_and_two_runs(mhc):
    msgs = messages(7, big=20000)
    model = o2_model(mhc, msgs)
    payload, out_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=512)
    other = [text(30000, s) for s in range(9)]
    other_model = o2_model(mhc, other)
    p2, o2, n2, _, _ = other_model.encode_batch_o2(other, chunk_symbols=512)
    results = []
    with mhc.device_memory("fill", 0xFF):                         # every fresh device buffer, the workspace included, starts as 0xFF
        a = mhc.SegmentStates(model, payload, out_off, nbits, o2=True)
        results.append((a.sym_off, a.status, a.index(512)[0], a.emit()[0], a.states_stats()))
    b = mhc.SegmentStates(model, payload, out_off, nbits, o2=True)
    results.append((b.sym_off, b.status, b.index(512)[0], b.emit()[0], b.states_stats()))
    # a workspace that held another batch's states (a larger batch under another model): the states call is made again on
    # a's buffers with that workspace
    lib = mhc.lib()
    donor = mhc.SegmentStates(other_model, p2, o2, n2, o2=True)
    assert donor.wsb >= a.wsb and donor.rc == mhc.MH_OK
    assert lib.mh_dev_batch_states_o2(model.handle, a.d_pl.ptr, a.d_po.ptr, a.d_nb.ptr, a.n, a.pay_total, PREV0, a.d_so.ptr, a.d_st.ptr, donor.d_ws.ptr,
                                      donor.wsb, None) == mhc.MH_OK
    assert lib.mh_dev_status(donor.d_ws.ptr, None) == mhc.MH_OK
    a.sym_off, a.status = a.d_so.download(np.uint64), a.d_st.download(np.int32)[:a.n]
    results.append((a.sym_off, a.status, a.index(512, ws=donor)[0], a.emit(ws=donor)[0], donor.states_stats()))
    cap = mhc.lib().mh_batch_index_capacity(int(in_off[-1]), len(msgs), 512)
    for so, status, built, out, stats in results:
        assert np.array_equal(so, in_off) and not status.any()
        assert np.array_equal(built, expected_index(idx, in_off, 512, cap))
        assert out == b"".join(msgs)
        assert stats == results[0][4]


# ---------------------------------------------------------------------------------------------------- a non-default stream

def test_states_index_decode_on_one_stream_without_a_host_wait(mhc):
    """states -> index -> indexed mh_dev_decode_batch_o2, all on one non-default stream behind a blocker, enqueued back to back
    (the harness of tests/test_gpu_stream_order.py): every call reads what the one before wrote on the device."""
    import torch
    import test_gpu_stream_order as so
    env = so.Env()
    env.torch, env.mhc, env.lib = torch, mhc, mhc.lib()
    env.stream = torch.cuda.Stream()
    env.sp = C.c_void_p(env.stream.cuda_stream)
    with torch.cuda.stream(env.stream):
        torch.cuda._sleep(1_000_000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
    b.synchronize()
    env.cycles_per_ms = 20_000_000 / a.elapsed_time(b)
    lib = env.lib
    msgs = messages(9, big=20000)
    joined = b"".join(msgs)
    counts = batch_ref.histogram(msgs, 2, PREV0)
    model = mhc.Model.from_counts(counts, 2)
    c = 1024
    ref = batch_ref.pack(msgs, *batch_ref.oracle_codes(counts, 2), 2, PREV0, c)
    n, total, pay_total = len(msgs), len(joined), int(ref.pay_off[-1])
    nidx = int(lib.mh_batch_index_capacity(total, n, c))
    ch = so.Chain(env, "order-2 states chain")
    ch.keep = model
    bt = so.Batch(ch.staged(np.concatenate([ref.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(ref.pay_off), ch.staged(ref.nbits), n, pay_total)
    wsb = lib.mh_dev_batch_states_o2_workspace(n, pay_total)
    d_ws, d_so, d_idx, d_out = ch.work(wsb), ch.words(n + 1), ch.words(nidx), ch.out(total + 64)
    st = [ch.status(n, "batch_%s_o2" % k) for k in ("states", "index", "emit")]
    ch.call("batch_states_o2", lib.mh_dev_batch_states_o2, model.handle, *bt.args(), PREV0, so.ptr(d_so), so.ptr(st[0]), so.ptr(d_ws), wsb, ws=d_ws)
    ch.call("batch_index_o2", lib.mh_dev_batch_index_o2, model.handle, *bt.args(), PREV0, so.ptr(d_idx), nidx, c, so.ptr(st[1]), so.ptr(d_ws), wsb)
    ch.call("batch_emit_o2", lib.mh_dev_batch_emit_o2, model.handle, *bt.args(), PREV0, so.ptr(d_out), total, so.ptr(st[2]), so.ptr(d_ws), wsb)
    ch.expect("batch_states_o2: sym_off", lambda: so.same(ch.get(d_so, np.uint64, n + 1), ref.sym_off))
    ch.expect("batch_index_o2: slices", lambda: so.same(ref.slices_of(ch.get(d_idx, np.uint64, nidx), c), ref.all_slices()))
    ch.expect("batch_emit_o2: bytes", lambda: ch.get(d_out, np.uint8, total).tobytes() == joined and (ch.get(d_out)[total:total + 64] == so.FILL).all())
    so.add_decode(ch, "decode_batch_o2 through the built index", lib.mh_dev_decode_batch_o2, lib.mh_dev_decode_batch_o2_workspace, model.handle, bt, PREV0,
                  total, d_so, d_idx, c, joined, ref.sym_off)
    so.drive(ch)
