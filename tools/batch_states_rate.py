"""Segment-state rate: index-free batches through states + index / emit (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES").

In one process, device-side timing (HIP events through torch) after warm-up, every result checked against the input:
  (a) 65 536 x 4 KiB, Zipf(1.1) and text, under a shared order-1 model and under per-stream order-1 models: mh_dev_*_states,
      mh_dev_*_index, mh_dev_*_emit, against the existing index-free mh_dev_decode_batch / _each and the indexed decode;
  (b) the mix of 400 streams of 0 B - 4 MiB plus one of 64 MiB (shared model): the same calls;
  (c) 4 096 random 256 B lookups into 4 096 x 64 KiB index-free Zipf records, shared and per-stream models: index-free
      lookups (mh_dev_decode_batch_ranges / _each_ranges without an index) against states + index + indexed lookups.
Prints one JSON line.  The kernel split comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_states_rate.py`.

    python tools/batch_states_rate.py [--reps 5] [--only 4k,mix,lookups]
"""
import argparse
import json
import os
import sys

try:
    import torch                                   # its HIP runtime first (see tests/conftest.py); events for the timing
except Exception:                                  # pragma: no cover
    torch = None
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def text(n, seed):
    words = [b"the", b"segment", b"state", b"of", b"a", b"stream", b"decoder", b"batch", b"index", b"huffman", b"markov", b"lattice"]
    rng = np.random.default_rng(seed)
    block = b" ".join(words[int(k)] for k in rng.integers(0, len(words), 200000))
    return np.frombuffer((block * (n // len(block) + 1))[:n], dtype=np.uint8)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def workload(mhc, data, lens, reps, per_stream):
    lib = mhc.lib()
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum(lens)
    total = int(in_off[-1])
    msgs = [data[int(in_off[i]):int(in_off[i + 1])].tobytes() for i in range(n)]
    chunk = 1024
    if per_stream:
        res = mhc.compress_each(msgs, order=1, chunk_symbols=chunk)
        model = mhc.ModelSet.from_tables([t for t, _, _, _ in res])
        payload, pay_off = mhc.batch_offsets([b[1:] for _, b, _, _ in res])
        nbits = np.array([nb for _, _, nb, _ in res], dtype=np.uint64)
        idx = np.zeros(lib.mh_batch_index_capacity(total, n, chunk), dtype=np.uint64)
        for i, (_, _, _, sl) in enumerate(res):
            b = int(in_off[i]) // chunk + i
            idx[b:b + len(sl)] = sl
        states_fn, index_fn, emit_fn, dec_fn = lib.mh_dev_each_states, lib.mh_dev_each_index, lib.mh_dev_each_emit, lib.mh_dev_decode_each
    else:
        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        payload, pay_off, nbits, idx, _ = model.encode_batch(msgs, chunk_symbols=chunk)
        states_fn, index_fn, emit_fn, dec_fn = lib.mh_dev_batch_states, lib.mh_dev_batch_index, lib.mh_dev_batch_emit, lib.mh_dev_decode_batch
    h = model.handle
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    pay_total = int(pay_off[n])
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16) + 64, a if a.nbytes else None)
    d_pl, d_po, d_nb, d_in, d_idx = D(payload), D(pay_off), D(nbits), D(in_off), D(idx)
    d_so, d_st, d_out = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4 + 4), mhc.DeviceBuffer(total + 64)
    nidx = lib.mh_batch_index_capacity(total, n, chunk)
    d_idx2 = mhc.DeviceBuffer(nidx * 8)
    wss = lib.mh_dev_batch_states_workspace(n, pay_total)
    d_ws = mhc.DeviceBuffer(wss)
    wsd = lib.mh_dev_decode_batch_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    r = {"streams": n, "bytes": total, "payload_bytes": pay_total, "models": "per-stream" if per_stream else "shared"}
    states = lambda: states_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_so.ptr, d_st.ptr, d_ws.ptr, wss, None)
    r["states"] = stats(timed(states, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_so.download(np.uint64), in_off), "states: sym_off"
    index = lambda: index_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_idx2.ptr, nidx, chunk, d_st.ptr, d_ws.ptr, wss, None)
    r["index"] = stats(timed(index, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    got = d_idx2.download(np.uint64)
    for i in range(n):
        b = int(in_off[i]) // chunk + i
        e = b + (int(lens[i]) + chunk - 1) // chunk
        assert np.array_equal(got[b:e], idx[b:e]), "index slice %d" % i
    emit = lambda: emit_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_st.ptr, d_ws.ptr, wss, None)
    r["emit"] = stats(timed(emit, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data[:total]), "emit bytes"
    dec_i = lambda: dec_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_in.ptr, total, d_idx.ptr, chunk,
                           d_st.ptr, d_wd.ptr, wsd, None)
    r["decode_indexed"] = stats(timed(dec_i, reps))
    assert lib.mh_dev_status(d_wd.ptr, None) == 0
    dec_f = lambda: dec_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_so.ptr, 0, None, 0, d_st.ptr,
                           d_wd.ptr, wsd, None)
    r["decode_index_free_walk"] = stats(timed(dec_f, reps))
    st = d_st.download(np.int32)[:n]
    r["walk_refused_over_cap"] = int((st == mhc.MH_ERR_ARG).sum())
    m = lambda k: r[k]["median_ms"]
    r["states_plus_emit_ms"] = round(m("states") + m("emit"), 4)
    r["states_plus_index_plus_indexed_decode_ms"] = round(m("states") + m("index") + m("decode_indexed"), 4)
    r["walk_over_states_plus_emit"] = round(m("decode_index_free_walk") / r["states_plus_emit_ms"], 2)
    return r


def lookups(mhc, reps, per_stream, n=4096, rec=65536, n_lookups=4096, span=256):
    lib = mhc.lib()
    data = zipf(n * rec, 4)
    in_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(rec)
    msgs = [data[i * rec:(i + 1) * rec].tobytes() for i in range(n)]
    chunk = 1024
    if per_stream:
        res = mhc.compress_each(msgs, order=1)
        model = mhc.ModelSet.from_tables([t for t, _, _, _ in res])
        payload, pay_off = mhc.batch_offsets([b[1:] for _, b, _, _ in res])
        nbits = np.array([nb for _, _, nb, _ in res], dtype=np.uint64)
        states_fn, index_fn, ranges_fn = lib.mh_dev_each_states, lib.mh_dev_each_index, lib.mh_dev_decode_each_ranges
    else:
        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        payload, pay_off, nbits, _, _ = model.encode_batch(msgs)
        states_fn, index_fn, ranges_fn = lib.mh_dev_batch_states, lib.mh_dev_batch_index, lib.mh_dev_decode_batch_ranges
    h = model.handle
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    pay_total = int(pay_off[n])
    rng = np.random.default_rng(9)
    st_ = rng.integers(0, n, n_lookups)
    b_ = rng.integers(0, rec - span + 1, n_lookups)
    lk = np.stack([st_, b_, b_ + span], axis=1).astype(np.uint64)
    want = np.concatenate([data[int(in_off[s]) + int(b):int(in_off[s]) + int(b) + span] for s, b, _ in lk])
    at = np.arange(n_lookups, dtype=np.uint64) * np.uint64(span)
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16) + 64, a if a.nbytes else None)
    d_pl, d_po, d_nb, d_lk, d_at = D(payload), D(pay_off), D(nbits), D(lk), D(at)
    d_out, d_lst = mhc.DeviceBuffer(n_lookups * span + 64), mhc.DeviceBuffer(n_lookups * 4)
    d_so, d_st = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4)
    nidx = lib.mh_batch_index_capacity(n * rec, n, chunk)
    d_idx = mhc.DeviceBuffer(nidx * 8)
    wss = lib.mh_dev_batch_states_workspace(n, pay_total)
    d_ws = mhc.DeviceBuffer(wss)
    wsr = lib.mh_dev_decode_batch_ranges_workspace(n_lookups)
    d_wr = mhc.DeviceBuffer(wsr)
    cap = n_lookups * span
    r = {"records": n, "record_bytes": rec, "lookups": n_lookups, "lookup_bytes": span, "models": "per-stream" if per_stream else "shared",
         "payload_bytes": pay_total}

    def check():
        assert lib.mh_dev_status(d_wr.ptr, None) == 0
        assert not d_lst.download(np.int32)[:n_lookups].any()
        assert np.array_equal(d_out.download()[:cap], want), "lookup bytes"

    free = lambda: ranges_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, 0x20, None, None, 0, d_lk.ptr, n_lookups, d_out.ptr, d_at.ptr, cap,
                             d_lst.ptr, d_wr.ptr, wsr, None)
    r["lookups_index_free"] = stats(timed(free, reps))
    check()
    states = lambda: states_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_so.ptr, d_st.ptr, d_ws.ptr, wss, None)
    index = lambda: index_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, 0x20, d_idx.ptr, nidx, chunk, d_st.ptr, d_ws.ptr, wss, None)
    r["states"] = stats(timed(states, reps))
    r["index"] = stats(timed(index, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_so.download(np.uint64), in_off), "states: sym_off"
    indexed = lambda: ranges_fn(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, 0x20, d_so.ptr, d_idx.ptr, chunk, d_lk.ptr, n_lookups, d_out.ptr,
                                d_at.ptr, cap, d_lst.ptr, d_wr.ptr, wsr, None)
    r["lookups_indexed"] = stats(timed(indexed, reps))
    check()
    m = lambda k: r[k]["median_ms"]
    r["states_plus_index_plus_indexed_lookups_ms"] = round(m("states") + m("index") + m("lookups_indexed"), 4)
    r["index_free_over_build_plus_indexed"] = round(m("lookups_index_free") / r["states_plus_index_plus_indexed_lookups_ms"], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="4k,mix,lookups")
    a = ap.parse_args()
    entry.build() if not os.path.exists(os.path.join(ROOT, "markov-huffman-coding_amd", "libmhc.so")) else None
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("batch_states_rate.py needs a GPU (and torch for the event timing)")
    res = {"tool": "batch_states_rate", "chunk_symbols": 1024, "segment_bits": 512, "repair_passes": 8}
    want = a.only.split(",")
    if "4k" in want:
        lens = [4096] * 65536
        res["a_65536x4KiB_zipf_shared"] = workload(mhc, zipf(4096 * 65536, 1), lens, a.reps, False)
        res["a_65536x4KiB_text_shared"] = workload(mhc, text(4096 * 65536, 2), lens, a.reps, False)
        res["a_65536x4KiB_zipf_per_stream"] = workload(mhc, zipf(4096 * 65536, 1), lens, a.reps, True)
        res["a_65536x4KiB_text_per_stream"] = workload(mhc, text(4096 * 65536, 2), lens, a.reps, True)
    if "mix" in want:
        rng = np.random.default_rng(3)
        lens = np.exp(rng.uniform(0, np.log(4 << 20), 400)).astype(np.int64) - 1
        lens[::37] = 0
        lens = list(lens) + [64 << 20]
        res["b_mix_0B_4MiB_plus_64MiB_shared"] = workload(mhc, zipf(int(sum(lens)), 3), lens, a.reps, False)
    if "lookups" in want:
        res["c_lookups_4096x64KiB_shared"] = lookups(mhc, a.reps, False)
        res["c_lookups_4096x64KiB_per_stream"] = lookups(mhc, a.reps, True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
