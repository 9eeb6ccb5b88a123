"""Segment-state rate of order-2 batches: index-free batches under one shared order-2 model through states + index / emit
(include/mh.h, "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES").

In one process, device-side timing (HIP events through torch) after warm-up, medians, every result checked against the input
before the clock:
  (a) 65 536 x 4 KiB, Zipf(1.1) and text: mh_dev_batch_states_o2, _index_o2, _emit_o2;
  (b) a mix of 400 streams of 0 B - 64 KiB plus one Zipf stream of 3 MiB (over MH_BATCH_WALK_MAX_BITS): the same calls;
  (c) 4 096 random 256 B lookups into 4 096 x 64 KiB index-free Zipf records: index-free mh_dev_decode_batch_o2_ranges against
      states + index + indexed lookups.
Yardsticks, timed in the same run: mh_dev_decode_batch_o2 index-free (one lane per stream) and indexed.  Per workload the
diagnostic of mh_dev_batch_states_stats: repair_passes_run, streams_walked.  The model of every workload is trained on it
(mh_dev_histogram_o2_batch).  Prints one JSON line and writes it to --out.

    python tools/batch_states_o2_rate.py [--reps 5] [--only 4k,mix,lookups] [--out profiles/batch_states_o2/batch_states_o2_rate.json]
"""
import argparse
import ctypes as C
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
from tools.batch_states_rate import stats, text, timed, zipf  # noqa: E402

PREV0, CHUNK = 0x20, 1024


def encode(mhc, data, lens):
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum(lens)
    msgs = [data[int(in_off[i]):int(in_off[i + 1])].tobytes() for i in range(n)]
    model = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
    payload, pay_off, nbits, idx, _ = model.encode_batch_o2(msgs, chunk_symbols=CHUNK)
    return model, in_off, np.ascontiguousarray(payload, dtype=np.uint8), pay_off, nbits, idx


def states_stats(lib, d_ws):
    passes, walked = C.c_uint32(0), C.c_uint64(0)
    assert lib.mh_dev_batch_states_stats(d_ws.ptr, None, C.byref(passes), C.byref(walked)) == 0
    return passes.value, walked.value


def workload(mhc, data, lens, reps):
    lib = mhc.lib()
    model, in_off, payload, pay_off, nbits, idx = encode(mhc, data, lens)
    n, total, pay_total, h = len(lens), int(in_off[-1]), int(pay_off[-1]), model.handle
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16) + 64, a if a.nbytes else None)
    d_pl, d_po, d_nb, d_in, d_idx = D(payload), D(pay_off), D(nbits), D(in_off), D(idx)
    d_so, d_st, d_out = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4 + 4), mhc.DeviceBuffer(total + 64)
    nidx = lib.mh_batch_index_capacity(total, n, CHUNK)
    d_idx2 = mhc.DeviceBuffer(nidx * 8)
    wss = lib.mh_dev_batch_states_o2_workspace(n, pay_total)
    d_ws = mhc.DeviceBuffer(wss)
    wsd = lib.mh_dev_decode_batch_o2_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    r = {"streams": n, "bytes": total, "payload_bytes": pay_total, "longest_stream_bits": int(nbits.max()) if n else 0}
    batch = (h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, PREV0)
    states = lambda: lib.mh_dev_batch_states_o2(*batch, d_so.ptr, d_st.ptr, d_ws.ptr, wss, None)
    r["states"] = stats(timed(states, reps))
    r["repair_passes_run"], r["streams_walked"] = states_stats(lib, d_ws)
    sst = d_st.download(np.int32)[:n]
    r["states_refused"] = int((sst == mhc.MH_ERR_ARG).sum())
    assert not sst[sst != mhc.MH_ERR_ARG].any(), "states: a stream failed"
    if r["states_refused"]:                        # (a miss to report, not to hide: the other variants need every stream)
        return r
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_so.download(np.uint64), in_off), "states: sym_off"
    index = lambda: lib.mh_dev_batch_index_o2(*batch, d_idx2.ptr, nidx, CHUNK, d_st.ptr, d_ws.ptr, wss, None)
    r["index"] = stats(timed(index, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    got = d_idx2.download(np.uint64)
    for i in range(n):
        b = int(in_off[i]) // CHUNK + i
        e = b + (int(lens[i]) + CHUNK - 1) // CHUNK
        assert np.array_equal(got[b:e], idx[b:e]), "index slice %d" % i
    emit = lambda: lib.mh_dev_batch_emit_o2(*batch, d_out.ptr, total, d_st.ptr, d_ws.ptr, wss, None)
    r["emit"] = stats(timed(emit, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data[:total]), "emit bytes"
    # indexed decode through the index the states built
    dec_i = lambda: lib.mh_dev_decode_batch_o2(*batch, d_out.ptr, total, d_so.ptr, total, d_idx2.ptr, CHUNK, d_st.ptr, d_wd.ptr, wsd, None)
    r["decode_indexed"] = stats(timed(dec_i, reps))
    assert lib.mh_dev_status(d_wd.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data[:total]), "indexed decode bytes"
    d_so2 = mhc.DeviceBuffer((n + 1) * 8)
    dec_f = lambda: lib.mh_dev_decode_batch_o2(*batch, d_out.ptr, total, d_so2.ptr, 0, None, 0, d_st.ptr, d_wd.ptr, wsd, None)
    r["decode_index_free_one_lane"] = stats(timed(dec_f, reps))
    st = d_st.download(np.int32)[:n]
    r["one_lane_refused_over_cap"] = int((st == mhc.MH_ERR_ARG).sum())
    if not st.any():
        assert np.array_equal(d_out.download()[:total], data[:total]), "index-free decode bytes"
    m = lambda k: r[k]["median_ms"]
    r["states_plus_emit_ms"] = round(m("states") + m("emit"), 4)
    r["states_plus_index_plus_indexed_decode_ms"] = round(m("states") + m("index") + m("decode_indexed"), 4)
    r["one_lane_over_states_plus_emit"] = round(m("decode_index_free_one_lane") / r["states_plus_emit_ms"], 2)
    return r


def lookups(mhc, reps, n=4096, rec=65536, n_lookups=4096, span=256):
    lib = mhc.lib()
    data = zipf(n * rec, 4)
    model, in_off, payload, pay_off, nbits, _ = encode(mhc, data, [rec] * n)
    h, pay_total = model.handle, int(pay_off[-1])
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
    nidx = lib.mh_batch_index_capacity(n * rec, n, CHUNK)
    d_idx = mhc.DeviceBuffer(nidx * 8)
    wss = lib.mh_dev_batch_states_o2_workspace(n, pay_total)
    d_ws = mhc.DeviceBuffer(wss)
    wsr = lib.mh_dev_decode_batch_o2_ranges_workspace(n_lookups)
    d_wr = mhc.DeviceBuffer(wsr)
    cap = n_lookups * span
    r = {"records": n, "record_bytes": rec, "lookups": n_lookups, "lookup_bytes": span, "payload_bytes": pay_total}

    def check():
        assert lib.mh_dev_status(d_wr.ptr, None) == 0
        assert not d_lst.download(np.int32)[:n_lookups].any()
        assert np.array_equal(d_out.download()[:cap], want), "lookup bytes"

    ranges = lib.mh_dev_decode_batch_o2_ranges
    free = lambda: ranges(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, PREV0, None, None, 0, d_lk.ptr, n_lookups, d_out.ptr, d_at.ptr, cap, d_lst.ptr,
                          d_wr.ptr, wsr, None)
    r["lookups_index_free"] = stats(timed(free, reps))
    check()
    batch = (h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, PREV0)
    states = lambda: lib.mh_dev_batch_states_o2(*batch, d_so.ptr, d_st.ptr, d_ws.ptr, wss, None)
    index = lambda: lib.mh_dev_batch_index_o2(*batch, d_idx.ptr, nidx, CHUNK, d_st.ptr, d_ws.ptr, wss, None)
    r["states"] = stats(timed(states, reps))
    r["repair_passes_run"], r["streams_walked"] = states_stats(lib, d_ws)
    r["index"] = stats(timed(index, reps))
    assert lib.mh_dev_status(d_ws.ptr, None) == 0
    assert np.array_equal(d_so.download(np.uint64), in_off), "states: sym_off"
    indexed = lambda: ranges(h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, PREV0, d_so.ptr, d_idx.ptr, CHUNK, d_lk.ptr, n_lookups, d_out.ptr, d_at.ptr, cap,
                             d_lst.ptr, d_wr.ptr, wsr, None)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_states_o2", "batch_states_o2_rate.json"))
    a = ap.parse_args()
    entry.build() if not os.path.exists(os.path.join(ROOT, "markov-huffman-coding_amd", "libmhc.so")) else None
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("batch_states_o2_rate.py needs a GPU (and torch for the event timing)")
    res = {"tool": "batch_states_o2_rate", "chunk_symbols": CHUNK, "segment_bits": 512, "warmup_bits": 512, "repair_passes": 8, "reps": a.reps}
    want = a.only.split(",")
    if "4k" in want:
        lens = [4096] * 65536
        res["a_65536x4KiB_zipf"] = workload(mhc, zipf(4096 * 65536, 1), lens, a.reps)
        res["a_65536x4KiB_text"] = workload(mhc, text(4096 * 65536, 2), lens, a.reps)
    if "mix" in want:
        rng = np.random.default_rng(3)
        lens = np.exp(rng.uniform(0, np.log(64 << 10), 400)).astype(np.int64) - 1
        lens[::37] = 0
        lens = list(lens) + [3 << 20]
        res["b_mix_0B_64KiB_plus_3MiB_zipf"] = workload(mhc, zipf(int(sum(lens)), 3), lens, a.reps)
    if "lookups" in want:
        res["c_lookups_4096x64KiB_zipf"] = lookups(mhc, a.reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
