"""Order-2 batch rate: many small streams under one shared order-2 model (include/mh.h, "BATCHES OF ORDER-2 STREAMS";
extension, parity unpinned), against the order-1 batch on the same messages.

In one process, device-side timing (HIP events through torch) after warm-up, per workload:
  (a) the order-1 batch (model from mh_dev_histogram_o1_batch): payload bytes, mh_dev_encode_batch, mh_dev_decode_batch with
      the index;
  (b) the order-2 batch (model from mh_dev_histogram_o2_batch): payload bytes, mh_dev_encode_batch_o2, mh_dev_decode_batch_o2
      with the index and without;
  (c) a loop of the single-stream order-2 device calls over the same messages (mh_dev_encode + mh_dev_decode_dn with an index;
      timed over at most --loop-max messages and extrapolated to the whole batch).
Workloads: 65 536 x 4 KiB of text (the bench's text generator: an 8 MiB lorem block, tiled), 1 M x 256 B of text, and
65 536 x 4 KiB of Zipf(1.1) (millions of live order-2 contexts: no hot table).  Every round trip is checked.  Prints one
JSON line.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_o2_rate.py --reps 1` run.

    python tools/batch_o2_rate.py [--reps 5] [--loop-max 8192] [--only text4k,text256,zipf4k]
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
import bench  # noqa: E402


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def text(n, seed):
    base = np.frombuffer(bench.lorem_block(8 << 20, seed), dtype=np.uint8)
    return np.tile(base, n // base.size + 1)[:n].copy()


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


def train(mhc, fn, ws_fn, ncounts, order, d_data, d_off, n, total):
    lib = mhc.lib()
    d_counts = mhc.DeviceBuffer(ncounts * 8)
    wsb = getattr(lib, ws_fn)(total)
    d_ws = mhc.DeviceBuffer(wsb)
    mhc._check(getattr(lib, fn)(d_data.ptr, d_off.ptr, n, total, 0x20, d_counts.ptr, d_ws.ptr, wsb, None), fn)
    mhc._check(lib.mh_dev_status(d_ws.ptr, None), fn)
    return mhc.Model.from_device_counts(d_counts.ptr, order)


def batch(mhc, model, o2, d_data, d_off, data, n, total, reps, chunk, index_free):
    """(results, d_nbits, d_index) of one family's batch calls on the messages already on the device"""
    lib = mhc.lib()
    h = model.handle
    sfx = "_o2" if o2 else ""
    enc_fn, dec_fn = getattr(lib, "mh_dev_encode_batch" + sfx), getattr(lib, "mh_dev_decode_batch" + sfx)
    cap = lib.mh_encode_batch_bound(h, total, n)
    d_pay, d_oo, d_nb = mhc.DeviceBuffer(cap + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8 + 8)
    d_idx = mhc.DeviceBuffer(lib.mh_batch_index_capacity(total, n, chunk) * 8)
    wse = getattr(lib, "mh_dev_encode_batch%s_workspace" % sfx)(n, total)
    d_we = mhc.DeviceBuffer(wse)
    enc = lambda: enc_fn(h, d_data.ptr, d_off.ptr, n, total, 0x20, d_pay.ptr, cap, d_oo.ptr, d_nb.ptr, d_idx.ptr, chunk, d_we.ptr, wse, None)
    r = {"batch_encode": stats(timed(enc, reps))}
    assert lib.mh_dev_status(d_we.ptr, None) == 0
    pay_total = int(d_oo.download(np.uint64)[n])
    r["payload_bytes"] = pay_total
    r["payload_ratio"] = round(pay_total / total, 4)
    d_out, d_so, d_st = mhc.DeviceBuffer(total + 64), mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 4 + 4)
    wsd = getattr(lib, "mh_dev_decode_batch%s_workspace" % sfx)(n)
    d_wd = mhc.DeviceBuffer(wsd)
    dec_i = lambda: dec_fn(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_off.ptr, total, d_idx.ptr, chunk,
                           d_st.ptr, d_wd.ptr, wsd, None)
    r["batch_decode_indexed"] = stats(timed(dec_i, reps))
    assert lib.mh_dev_status(d_wd.ptr, None) == 0
    assert np.array_equal(d_out.download()[:total], data), "indexed round trip"
    if index_free:
        dec_f = lambda: dec_fn(h, d_pay.ptr, d_oo.ptr, d_nb.ptr, n, pay_total, 0x20, d_out.ptr, total, d_so.ptr, 0, None, 0,
                               d_st.ptr, d_wd.ptr, wsd, None)
        r["batch_decode_index_free"] = stats(timed(dec_f, reps))
        assert lib.mh_dev_status(d_wd.ptr, None) == 0
        assert np.array_equal(d_out.download()[:total], data), "index-free round trip"
    return r, d_nb, d_idx


def single_loop(mhc, model, data, lens, off, nbits_host, reps, loop_max, chunk):
    """the single-stream order-2 calls, one message at a time (each message copied to a 16-byte aligned start)"""
    lib = mhc.lib()
    h = model.handle
    n = len(lens)
    k = min(n, loop_max)
    starts = np.zeros(k, dtype=np.uint64)
    p = 0
    for i in range(k):
        starts[i] = p
        p += (int(lens[i]) + 15) & ~15
    al = np.zeros(max(p, 16), dtype=np.uint8)
    for i in range(k):
        al[int(starts[i]):int(starts[i]) + int(lens[i])] = data[int(off[i]):int(off[i + 1])]
    d_al = mhc.DeviceBuffer(al.nbytes, al)
    maxn = int(lens[:k].max()) if k else 0
    scap = lib.mh_encode_bound(h, maxn) + 64
    d_sp, d_snb = mhc.DeviceBuffer(scap), mhc.DeviceBuffer(8)
    d_sidx = mhc.DeviceBuffer((maxn // chunk + 2) * 8)
    sws = lib.mh_dev_encode_workspace(maxn)
    d_sws = mhc.DeviceBuffer(sws)
    dws = lib.mh_dev_decode_workspace(0, maxn, chunk)
    d_dws = mhc.DeviceBuffer(max(dws, 64))
    d_sout = mhc.DeviceBuffer(maxn + 64)
    base = d_al.ptr.value

    def loop():
        for i in range(k):
            ln = int(lens[i])
            lib.mh_dev_encode(h, C.c_void_p(base + int(starts[i])), ln, 0x20, d_sp.ptr, scap, d_snb.ptr, d_sidx.ptr, chunk, d_sws.ptr, sws, None)
            lib.mh_dev_decode_dn(h, d_sp.ptr, d_snb.ptr, int(nbits_host[i]), d_sout.ptr, ln, d_sidx.ptr, chunk, d_dws.ptr, dws, None)
    ms = timed(loop, max(2, reps // 2), warm=1)
    assert lib.mh_dev_status(d_dws.ptr, None) == 0
    assert np.array_equal(d_sout.download()[:int(lens[k - 1])], data[int(off[k - 1]):int(off[k])]), "loop round trip"
    per = float(np.median(ms)) / k
    return {"loop_messages_timed": k, "loop_enc_plus_indexed_dec_us_per_message": round(per * 1e3, 3),
            "loop_extrapolated_ms": round(per * n, 3)}


def workload(mhc, gen, size, count, seed, reps, loop_max, chunk=1024):
    lens = np.full(count, size, dtype=np.uint64)
    n = count
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    data = gen(total, seed)
    D = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16), a if a.nbytes else None)
    d_data, d_off = D(data), D(off)
    r = {"streams": n, "bytes": total}
    m1 = train(mhc, "mh_dev_histogram_o1_batch", "mh_dev_histogram_batch_workspace", 65536, 1, d_data, d_off, n, total)
    r1, _, _ = batch(mhc, m1, False, d_data, d_off, data, n, total, reps, chunk, index_free=False)
    del m1
    m2 = train(mhc, "mh_dev_histogram_o2_batch", "mh_dev_histogram_o2_batch_workspace", 1 << 24, 2, d_data, d_off, n, total)
    lay = m2.tile_layout()
    r["order2_model"] = {"max_code_len": m2.max_code_len, "slot_tables": lay[0] > 0}
    r2, d_nb2, _ = batch(mhc, m2, True, d_data, d_off, data, n, total, reps, chunk, index_free=True)
    r["order1_batch"] = r1
    r["order2_batch"] = r2
    r["order2_vs_order1"] = {
        "payload": round(r2["payload_bytes"] / r1["payload_bytes"], 4),
        "encode_time": round(r2["batch_encode"]["median_ms"] / r1["batch_encode"]["median_ms"], 3),
        "indexed_decode_time": round(r2["batch_decode_indexed"]["median_ms"] / r1["batch_decode_indexed"]["median_ms"], 3),
    }
    best = r2["batch_encode"]["median_ms"] + r2["batch_decode_indexed"]["median_ms"]
    r2["batch_enc_plus_indexed_dec_GBps"] = round(total / best / 1e6, 2)
    loop = single_loop(mhc, m2, data, lens, off, d_nb2.download(np.uint64)[:n], reps, loop_max, chunk)
    loop["speedup_batch_vs_loop"] = round(loop["loop_extrapolated_ms"] / best, 2)
    r["order2_single_stream_loop"] = loop
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=8192)
    ap.add_argument("--only", default="text4k,text256,zipf4k")
    a = ap.parse_args()
    entry.build() if not os.path.exists(os.path.join(ROOT, "markov-huffman-coding_amd", "libmhc.so")) else None
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("batch_o2_rate.py needs a GPU (and torch for the event timing)")
    res = {"tool": "batch_o2_rate", "chunk_symbols": 1024}
    want = a.only.split(",")
    if "text4k" in want:
        res["text_65536x4KiB"] = workload(mhc, text, 4096, 65536, 1, a.reps, a.loop_max)
    if "text256" in want:
        res["text_1Mx256B"] = workload(mhc, text, 256, 1 << 20, 2, a.reps, a.loop_max)
    if "zipf4k" in want:
        res["zipf_65536x4KiB"] = workload(mhc, zipf, 4096, 65536, 3, a.reps, a.loop_max)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
