"""Batch rate: many small streams under one shared model (include/mh.h, "BATCHES OF INDEPENDENT STREAMS").

In one process, device-side timing (HIP events through torch) after warm-up:
  (a) the batch device calls: mh_dev_encode_batch, mh_dev_decode_batch with the index, mh_dev_decode_batch without;
  (b) a loop of the single-stream device calls over the same messages (mh_dev_encode + mh_dev_decode with an index; the
      loop is timed over at most --loop-max messages and given per message).
Workloads: 65 536 x 4 KiB, 1 M x 256 B, and a mix of sizes from 0 B to 4 MiB with one 64 MiB stream.  Prints one JSON line.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_rate.py` run.

    python tools/batch_rate.py [--reps 5] [--loop-max 8192] [--only 4k,256,mix]
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


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


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


def workload(mhc, name, lens, seed, reps, loop_max):
    lib = mhc.lib()
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    data = zipf(total, seed)
    model = mhc.Model.from_data(data, 1)           # every pair of the input has a code: the round trips are checked
    h, chunk = model.handle, 1024
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16), a if a.nbytes else None)
    d_data, d_off = D(data), D(off)
    cap = lib.mh_encode_batch_bound(h, total, n)
    d_pay, d_oo, d_nb = mhc.DeviceBuffer(cap + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8 + 8)
    nidx = lib.mh_batch_index_capacity(total, n, chunk)
    d_idx = mhc.DeviceBuffer(nidx * 8)
    wse = lib.mh_dev_encode_batch_workspace(n, total)
    d_we = mhc.DeviceBuffer(wse)
    enc = lambda: lib.mh_dev_encode_batch(h, d_data.ptr, d_off.ptr, n, total, 0x20, d_pay.ptr, cap, d_oo.ptr, d_nb.ptr, d_idx.ptr, chunk,
                                          d_we.ptr, wse, None)
    r = {"streams": n, "bytes": total}
    r["batch_encode"] = stats(timed(enc, reps))
    assert lib.mh_dev_status(d_we.ptr, None) == 0
    out_off = mhc.DeviceBuffer.download(d_oo, np.uint64)
    pay_total = int(out_off[n])
    r["payload_bytes"] = pay_total
    d_out, d_so, d_st = mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4 + 4)
    wsd = lib.mh_dev_decode_batch_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    dec_i = lambda: lib.mh_dev_decode_batch(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_off.ptr, total,
                                            d_idx.ptr, chunk, d_st.ptr, d_wd.ptr, wsd, None)
    r["batch_decode_indexed"] = stats(timed(dec_i, reps))
    assert lib.mh_dev_status(d_wd.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data), "indexed round trip"
    dec_f = lambda: lib.mh_dev_decode_batch(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_so.ptr, 0,
                                            None, 0, d_st.ptr, d_wd.ptr, wsd, None)
    r["batch_decode_index_free"] = stats(timed(dec_f, reps))
    st = d_st.download(np.int32)[:n]
    r["index_free_refused_over_walk_cap"] = int((st == mhc.MH_ERR_ARG).sum())
    assert ((st == 0) | (st == mhc.MH_ERR_ARG)).all()
    best = r["batch_encode"]["median_ms"] + r["batch_decode_indexed"]["median_ms"]
    r["batch_enc_plus_indexed_dec_GBps"] = round(total / best / 1e6, 2)
    r["batch_enc_plus_index_free_dec_GBps"] = round(total / (r["batch_encode"]["median_ms"] + r["batch_decode_index_free"]["median_ms"]) / 1e6, 2)
    # (b) the single-stream calls, one message at a time (each message copied to a 16-byte aligned start)
    k = min(n, loop_max)
    sel = list(range(k))
    starts = np.zeros(k, dtype=np.uint64)
    p = 0
    for j, i in enumerate(sel):
        starts[j] = p
        p += (int(lens[i]) + 15) & ~15
    al = np.zeros(max(p, 16), dtype=np.uint8)
    for j, i in enumerate(sel):
        al[int(starts[j]):int(starts[j]) + int(lens[i])] = data[int(off[i]):int(off[i + 1])]
    d_al = D(al)
    maxn = int(lens[:k].max()) if k else 0
    scap = lib.mh_encode_bound(h, maxn) + 64
    d_sp, d_snb = mhc.DeviceBuffer(scap), mhc.DeviceBuffer(8)
    d_sidx = mhc.DeviceBuffer((maxn // chunk + 2) * 8)
    sws = lib.mh_dev_encode_workspace(maxn)
    d_sws = mhc.DeviceBuffer(sws)
    dws = lib.mh_dev_decode_workspace(0, maxn, chunk)
    d_dws = mhc.DeviceBuffer(max(dws, 64))
    d_sout = mhc.DeviceBuffer(maxn + 64)
    nbits_host = mhc.DeviceBuffer.download(d_nb, np.uint64)[:n]
    base = d_al.ptr.value

    def loop():
        for j, i in enumerate(sel):
            ln = int(lens[i])
            lib.mh_dev_encode(h, C.c_void_p(base + int(starts[j])), ln, 0x20, d_sp.ptr, scap, d_snb.ptr, d_sidx.ptr, chunk, d_sws.ptr, sws, None)
            lib.mh_dev_decode_dn(h, d_sp.ptr, d_snb.ptr, int(nbits_host[i]), d_sout.ptr, ln, d_sidx.ptr, chunk, d_dws.ptr, dws, None)
    ms = timed(loop, max(2, reps // 2), warm=1)
    per = float(np.median(ms)) / k
    r["loop_messages_timed"] = k
    r["loop_enc_plus_indexed_dec_us_per_message"] = round(per * 1e3, 3)
    r["loop_extrapolated_ms"] = round(per * n, 3)
    r["speedup_batch_vs_loop"] = round(per * n / best, 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=8192)
    ap.add_argument("--only", default="4k,256,mix")
    a = ap.parse_args()
    entry.build() if not os.path.exists(os.path.join(ROOT, "markov-huffman-coding_amd", "libmhc.so")) else None
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("batch_rate.py needs a GPU (and torch for the event timing)")
    res = {"tool": "batch_rate", "chunk_symbols": 1024}
    want = a.only.split(",")
    if "4k" in want:
        res["65536x4KiB"] = workload(mhc, "4k", [4096] * 65536, 1, a.reps, a.loop_max)
    if "256" in want:
        res["1Mx256B"] = workload(mhc, "256", [256] * (1 << 20), 2, a.reps, a.loop_max)
    if "mix" in want:
        rng = np.random.default_rng(3)
        lens = np.exp(rng.uniform(0, np.log(4 << 20), 400)).astype(np.int64) - 1
        lens[::37] = 0
        lens = list(lens) + [64 << 20]
        res["mix_0B_4MiB_plus_64MiB"] = workload(mhc, "mix", lens, 3, a.reps, min(a.loop_max, 401))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
