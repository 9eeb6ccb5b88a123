"""Random-access rate into order-2 streams (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS").

In one process, after warm-up, with HIP events (medians with min and max):
  (a) one stream: 4 GiB of text (bench.py's Lorem-Ipsum-style text, tiled) under its order-2 model, chunk 1024, encoded with
      the chunk index and the order-2 fine index (mh_dev_encode_ctx_fine); 65 536 random 256-byte ranges through
      mh_dev_decode_ranges_o2 with and without the fine index, against mh_dev_decode_fine of the whole stream followed by a
      gather of the same bytes (torch indexing);
  (b) a batch: 65 536 x 4 KiB messages of that text under one shared order-2 model (mh_encode_batch_o2, chunk 1024); 4 096
      random 256-byte lookups through mh_dev_decode_batch_o2_ranges, indexed and index-free, against mh_dev_decode_batch_o2 of
      the whole batch followed by the gather;
  (c) the host form, wall clock: one 4 KiB range of the stream of (a) through mh_decode_ranges_o2 from host memory, with
      mh_last_range_upload_bytes, against mh_decode of the whole stream.
Every output is checked against the input.  Prints one JSON line.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/range_o2_rate.py` run.

    python tools/range_o2_rate.py [--gib 4] [--ranges 65536] [--streams 65536] [--lookups 4096] [--reps 5]
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
import bench  # noqa: E402

CHUNK = 1024
LEN = 256
CTX0 = 0x2020


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


def p(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda")


def check(mhc, rc, what):
    if rc != mhc.MH_OK:
        raise mhc.MhError(rc, what)


def gather_index(starts, length):
    return (starts.view(-1, 1) + torch.arange(length, device="cuda", dtype=torch.int64).view(1, -1)).reshape(-1)


def one_stream(mhc, args, text):
    lib = mhc.lib()
    n = args.gib << 30
    base = torch.from_numpy(text).to("cuda")
    data = base.repeat((n + base.numel() - 1) // base.numel())[:n].contiguous()
    del base
    counts = torch.zeros(1 << 24, dtype=torch.int64, device="cuda")
    check(mhc, lib.mh_dev_histogram_o2(p(data), n, CTX0, p(counts), None), "mh_dev_histogram_o2")
    model = mhc.Model.from_device_counts(p(counts), 2)
    del counts
    cap = lib.mh_encode_bound(model.handle, n) + 64
    payload = torch.empty(cap, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    nidx = (n + CHUNK - 1) // CHUNK
    index = torch.empty(nidx, dtype=torch.int64, device="cuda")
    fine = torch.empty((n + 63) // 64, dtype=torch.int32, device="cuda")
    wsb = lib.mh_dev_encode_workspace(n)
    ws = torch.empty(wsb + 64, dtype=torch.uint8, device="cuda")
    check(mhc, lib.mh_dev_encode_ctx_fine(model.handle, p(data), n, CTX0, None, p(payload), cap, p(nb), p(index), CHUNK, p(fine), p(ws),
                                          wsb, None), "mh_dev_encode_ctx_fine")
    check(mhc, lib.mh_dev_status(p(ws), None), "encode status")
    del ws
    nbits = int(nb.item())
    usable = float((fine & 0xFFFF).ne(0xFFFF).float().mean().item())
    rng = np.random.default_rng(1)
    b = rng.integers(0, n - LEN + 1, args.ranges).astype(np.uint64)
    rg = dev(np.stack([b, b + np.uint64(LEN)], axis=1))
    at = dev(np.arange(args.ranges, dtype=np.uint64) * np.uint64(LEN))
    out = torch.empty(args.ranges * LEN, dtype=torch.uint8, device="cuda")
    st = torch.empty(args.ranges, dtype=torch.int32, device="cuda")
    rws_b = lib.mh_dev_decode_ranges_o2_workspace(args.ranges)
    rws = torch.empty(rws_b, dtype=torch.uint8, device="cuda")
    gidx = gather_index(torch.from_numpy(b.astype(np.int64)).to("cuda"), LEN)
    want = data[gidx]
    res = {"n_bytes": n, "payload_bytes": (nbits + 7) // 8, "chunk": CHUNK, "ranges": args.ranges, "range_bytes": LEN,
           "fine_entries_usable": round(usable, 6)}
    for name, f in (("ranges_chunk_index", None), ("ranges_fine_index", fine)):
        def call(f=f):
            check(mhc, lib.mh_dev_decode_ranges_o2(model.handle, p(payload), 0, (nbits + 7) // 8, nbits, p(index), CHUNK, n,
                                                   p(f) if f is not None else None, p(rg), args.ranges, p(out), p(at), out.numel(), p(st),
                                                   p(rws), rws_b, None), "mh_dev_decode_ranges_o2")
        out.fill_(0)
        res[name] = stats(timed(call, args.reps))
        assert lib.mh_dev_status(p(rws), None) == 0 and int(st.abs().sum().item()) == 0, name
        assert torch.equal(out, want), name
    del data
    full = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    dws_b = lib.mh_dev_decode_workspace(nbits, n, CHUNK)
    dws = torch.empty(dws_b, dtype=torch.uint8, device="cuda")

    def whole():
        check(mhc, lib.mh_dev_decode_fine(model.handle, p(payload), nbits, None, p(full), n, p(index), CHUNK, p(fine), p(dws), dws_b, None),
              "mh_dev_decode_fine")
        out.copy_(full[gidx])
    res["whole_decode_fine_and_gather"] = stats(timed(whole, args.reps))
    assert lib.mh_dev_status(p(dws), None) == 0 and torch.equal(out, want)
    res["decode_path"] = int(lib.mh_dev_decode_path(p(dws), None))
    for name in ("ranges_chunk_index", "ranges_fine_index"):
        res["speedup_" + name] = round(res["whole_decode_fine_and_gather"]["median_ms"] / res[name]["median_ms"], 2)
    # (c) the host form on host copies of the payload and index
    h_pl = payload[:(nbits + 7) // 8].cpu().numpy()
    h_idx = index.cpu().numpy().view(np.uint64)
    del full, dws, payload, fine
    torch.cuda.empty_cache()
    hb = int(b[0]) % (n - 4096)
    host = {}

    def one():
        outs, hst = model.decode_ranges_o2(h_pl, nbits, h_idx, CHUNK, n, [(hb, hb + 4096)])
        assert list(hst) == [0] and len(outs[0]) == 4096
        host["bytes"] = outs[0]
    res["host_one_4k_range"] = stats(wall(one, args.reps))
    res["host_one_4k_range_upload_bytes"] = int(lib.mh_last_range_upload_bytes())
    assert host["bytes"] == np.take(text, np.arange(hb, hb + 4096) % text.size).tobytes()

    def all_of():
        host["all"] = model.decode(h_pl, nbits, index=h_idx, chunk_symbols=CHUNK, n_symbols=n)
    res["host_decode_whole_stream"] = stats(wall(all_of, max(1, args.reps // 2), warm=0))
    assert host["all"][hb:hb + 4096] == host["bytes"]
    res["speedup_host_one_4k_range"] = round(res["host_decode_whole_stream"]["median_ms"] / res["host_one_4k_range"]["median_ms"], 1)
    return res


def batch(mhc, args, text):
    lib = mhc.lib()
    per, ns = 4096, args.streams
    total = per * ns
    data = np.tile(text, (total + text.size - 1) // text.size)[:total]
    msgs = [data[i * per:(i + 1) * per].tobytes() for i in range(ns)]
    model = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
    payload, pay_off, nbits, idx, in_off = model.encode_batch_o2(msgs, chunk_symbols=CHUNK)
    d_pl = dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)]))
    d_po, d_nb, d_so, d_idx = dev(pay_off), dev(nbits), dev(in_off), dev(idx)
    d_data = torch.from_numpy(data).to("cuda")
    rng = np.random.default_rng(2)
    s = rng.integers(0, ns, args.lookups).astype(np.uint64)
    b = rng.integers(0, per - LEN + 1, args.lookups).astype(np.uint64)
    lk = dev(np.stack([s, b, b + np.uint64(LEN)], axis=1))
    at = dev(np.arange(args.lookups, dtype=np.uint64) * np.uint64(LEN))
    out = torch.empty(args.lookups * LEN, dtype=torch.uint8, device="cuda")
    st = torch.empty(args.lookups, dtype=torch.int32, device="cuda")
    lws_b = lib.mh_dev_decode_batch_o2_ranges_workspace(args.lookups)
    lws = torch.empty(lws_b, dtype=torch.uint8, device="cuda")
    gidx = gather_index(torch.from_numpy((s * np.uint64(per) + b).astype(np.int64)).to("cuda"), LEN)
    want = d_data[gidx]
    res = {"streams": ns, "stream_bytes": per, "payload_bytes": int(pay_off[-1]), "lookups": args.lookups, "lookup_bytes": LEN}
    for name, so, ix in (("lookups_indexed", d_so, d_idx), ("lookups_index_free", None, None)):
        def call(so=so, ix=ix):
            check(mhc, lib.mh_dev_decode_batch_o2_ranges(model.handle, p(d_pl), p(d_po), p(d_nb), ns, 0x20, p(so) if so is not None else None,
                                                         p(ix) if ix is not None else None, CHUNK, p(lk), args.lookups, p(out), p(at),
                                                         out.numel(), p(st), p(lws), lws_b, None), "mh_dev_decode_batch_o2_ranges")
        out.fill_(0)
        res[name] = stats(timed(call, args.reps))
        assert lib.mh_dev_status(p(lws), None) == 0 and int(st.abs().sum().item()) == 0, name
        assert torch.equal(out, want), name
    full = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    sst = torch.empty(ns, dtype=torch.int32, device="cuda")
    dws_b = lib.mh_dev_decode_batch_o2_workspace(ns)
    dws = torch.empty(dws_b, dtype=torch.uint8, device="cuda")
    so_free = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    for name, so, ix in (("whole_batch_indexed_and_gather", d_so, d_idx), ("whole_batch_index_free_and_gather", so_free, None)):
        def whole(so=so, ix=ix):
            check(mhc, lib.mh_dev_decode_batch_o2(model.handle, p(d_pl), p(d_po), p(d_nb), ns, int(pay_off[-1]), 0x20, p(full), full.numel(),
                                                  p(so), total, p(ix) if ix is not None else None, CHUNK, p(sst), p(dws), dws_b, None),
                  "mh_dev_decode_batch_o2")
            out.copy_(full[gidx])
        res[name] = stats(timed(whole, args.reps))
        assert lib.mh_dev_status(p(dws), None) == 0 and torch.equal(out, want), name
    res["speedup_lookups_indexed"] = round(res["whole_batch_indexed_and_gather"]["median_ms"] / res["lookups_indexed"]["median_ms"], 2)
    res["speedup_lookups_index_free"] = round(res["whole_batch_index_free_and_gather"]["median_ms"] / res["lookups_index_free"]["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--ranges", type=int, default=65536)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--lookups", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    mhc = entry.load_package()
    mhc.lib()
    text = np.frombuffer(bench.lorem_block(8 << 20, 1), dtype=np.uint8)
    out = {"tool": "range_o2_rate", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    out["batch"] = batch(mhc, args, text)
    torch.cuda.empty_cache()
    out["stream"] = one_stream(mhc, args, text)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
