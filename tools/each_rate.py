"""Per-stream-model batch rate (include/mh.h, "BATCHES OF STREAMS, ONE MODEL EACH").

In one process, after warm-up:
  (a) the device calls, timed with HIP events (torch): mh_dev_model_set_train (it synchronises twice inside),
      mh_dev_model_set_tables, mh_dev_encode_each, mh_dev_decode_each with the index and without;
  (b) the host forms mh_compress_each / mh_decompress_each, wall clock (uploads and downloads included);
  (c) the reference's per-file flow as a loop of single-stream calls, wall clock, over at most --loop-max messages and given
      per message: histogram -> model -> table -> encode (mh_histogram_o1, mh_model_from_counts, mh_model_write_table,
      mh_encode), then table load -> decode (mh_model_from_table_bits, mh_decode).
Workloads: 65 536 x 4 KiB Zipf(1.1), 65 536 x 4 KiB tiled text, and a mix of sizes from 0 B to 4 MiB.  Every output of (a)
is checked against (b) and the round trips against the input.  Prints one JSON line.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/each_rate.py` run.

    python tools/each_rate.py [--reps 5] [--loop-max 256] [--only zipf,text,mix] [--device-only]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def text(n):
    with open(os.path.join(ROOT, "tests", "golden", "inputs", "input_ipsum.txt"), "rb") as f:
        t = np.frombuffer(f.read(), dtype=np.uint8)
    return np.resize(t, n)


def timed(fn, reps, warm=1):
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


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def workload(mhc, lens, data, reps, loop_max, host_forms=True):
    lib = mhc.lib()
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    data = data[:total]
    chunk = 1024
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16), a if a.nbytes else None)
    d_data, d_off = D(data), D(off)
    r = {"streams": n, "bytes": total}

    # (a) device calls
    wst = lib.mh_dev_model_set_train_workspace(n)
    d_wt = mhc.DeviceBuffer(wst)
    sets = []

    def train():
        h = C.c_void_p()
        assert lib.mh_dev_model_set_train(d_data.ptr, d_off.ptr, n, total, 1, 0x20, d_wt.ptr, wst, None, C.byref(h)) == 0
        if sets:
            lib.mh_model_set_free(sets.pop())
        sets.append(h)
    r["train"] = stats(timed(train, reps))
    h = sets[0]
    r["live_contexts"] = lib.mh_model_set_slots(h)
    tcap = lib.mh_model_set_tables_bound(h)
    wtab = lib.mh_dev_model_set_tables_workspace(h)
    d_tab, d_toff, d_wtab = mhc.DeviceBuffer(tcap + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(wtab)
    tabs = lambda: lib.mh_dev_model_set_tables(h, d_tab.ptr, tcap, d_toff.ptr, d_wtab.ptr, wtab, None)
    r["tables"] = stats(timed(tabs, reps))
    assert lib.mh_dev_status(d_wtab.ptr, None) == 0
    r["table_bytes"] = int(d_toff.download(np.uint64)[n])
    cap = lib.mh_encode_each_bound(h, total, n)
    d_pay, d_oo, d_nb = mhc.DeviceBuffer(cap + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8 + 8)
    d_idx = mhc.DeviceBuffer(lib.mh_batch_index_capacity(total, n, chunk) * 8)
    wse = lib.mh_dev_encode_each_workspace(n, total)
    d_we = mhc.DeviceBuffer(wse)
    enc = lambda: lib.mh_dev_encode_each(h, d_data.ptr, d_off.ptr, n, total, 0x20, d_pay.ptr, cap, d_oo.ptr, d_nb.ptr, d_idx.ptr, chunk,
                                         d_we.ptr, wse, None)
    r["encode"] = stats(timed(enc, reps))
    assert lib.mh_dev_status(d_we.ptr, None) == 0
    pay_total = int(d_oo.download(np.uint64)[n])
    r["payload_bytes"] = pay_total
    d_out, d_so, d_st = mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4 + 4)
    wsd = lib.mh_dev_decode_each_workspace(n)
    d_wd = mhc.DeviceBuffer(wsd)
    dec_i = lambda: lib.mh_dev_decode_each(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_off.ptr, total,
                                           d_idx.ptr, chunk, d_st.ptr, d_wd.ptr, wsd, None)
    r["decode_indexed"] = stats(timed(dec_i, reps))
    assert lib.mh_dev_status(d_wd.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data), "indexed round trip"
    dec_f = lambda: lib.mh_dev_decode_each(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_so.ptr, 0,
                                           None, 0, d_st.ptr, d_wd.ptr, wsd, None)
    r["decode_index_free"] = stats(timed(dec_f, reps))
    st = d_st.download(np.int32)[:n]
    r["index_free_refused_over_walk_cap"] = int((st == mhc.MH_ERR_ARG).sum())
    assert ((st == 0) | (st == mhc.MH_ERR_ARG)).all()
    dev = sum(r[k]["median_ms"] for k in ("train", "tables", "encode", "decode_indexed"))
    r["device_train_tables_enc_dec_ms"] = round(dev, 3)
    r["device_GBps"] = round(total / dev / 1e6, 3)
    tab_dev = d_tab.download()[:r["table_bytes"]].tobytes()
    pay_dev = d_pay.download()[:pay_total].tobytes()
    lib.mh_model_set_free(h)
    del d_tab, d_pay, d_out, d_idx, d_we, d_wd, d_wt

    msgs = [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    if not host_forms:
        return r
    # (b) host forms
    res = []
    comp = lambda: res.append(mhc.compress_each(msgs, order=1)) if not res else mhc.compress_each(msgs, order=1)
    r["host_compress_each"] = stats(wall(comp, max(2, reps // 2)))
    assert b"".join(t for t, _, _, _ in res[0]) == tab_dev and b"".join(b[1:] for _, b, _, _ in res[0]) == pay_dev
    tables, blobs = [t for t, _, _, _ in res[0]], [b for _, b, _, _ in res[0]]
    back = []
    dec = lambda: back.append(mhc.decompress_each(tables, blobs)) if not back else mhc.decompress_each(tables, blobs)
    r["host_decompress_each"] = stats(wall(dec, max(2, reps // 2)))
    assert back[0] == msgs
    host = r["host_compress_each"]["median_ms"] + r["host_decompress_each"]["median_ms"]

    # (c) the per-file loop of single-stream calls
    k = min(n, loop_max)

    def loop():
        for i in range(k):
            m = msgs[i]
            model = mhc.Model.from_counts(mhc.histogram_o1(m), 1)
            t = model.table_bytes()
            payload, nb, _ = model.encode(m)
            back_model = mhc.Model.from_table(t)
            assert back_model.decode(payload, nb) == m
    ms = wall(loop, 2)
    per = float(np.median(ms)) / k
    r["loop_messages_timed"] = k
    r["loop_ms_per_message"] = round(per, 4)
    r["loop_extrapolated_ms"] = round(per * n, 1)
    r["speedup_device_vs_loop"] = round(per * n / dev, 1)
    r["speedup_host_forms_vs_loop"] = round(per * n / host, 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--only", default="zipf,text,mix")
    ap.add_argument("--device-only", action="store_true", help="time (a) alone (the kernel-trace run)")
    a = ap.parse_args()
    entry.build() if not os.path.exists(os.path.join(ROOT, "markov-huffman-coding_amd", "libmhc.so")) else None
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("each_rate.py needs a GPU (and torch for the event timing)")
    res = {"tool": "each_rate", "order": 1, "chunk_symbols": 1024}
    want = a.only.split(",")
    if "zipf" in want:
        res["65536x4KiB_zipf1.1"] = workload(mhc, [4096] * 65536, zipf(4096 * 65536, 1), a.reps, a.loop_max, not a.device_only)
    if "text" in want:
        res["65536x4KiB_text"] = workload(mhc, [4096] * 65536, text(4096 * 65536), a.reps, a.loop_max, not a.device_only)
    if "mix" in want:
        rng = np.random.default_rng(3)
        lens = np.exp(rng.uniform(0, np.log(4 << 20), 400)).astype(np.int64) - 1
        lens[::37] = 0
        res["mix_0B_4MiB"] = workload(mhc, lens, zipf(int(lens.sum()), 3), a.reps, min(a.loop_max, 400), not a.device_only)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
