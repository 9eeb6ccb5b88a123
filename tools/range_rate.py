"""Random-access rate (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM").

In one process, after warm-up, on one large Zipf(1.1) stream (order 1, chunk 1024; 256 MiB of Zipf tiled to --gib GiB):
  (a) 65 536 random 256-byte ranges with mh_dev_decode_ranges, HIP events: with the chunk index only, then with the fine
      index; against mh_dev_decode_fine of the whole stream followed by a gather of the same ranges (torch indexing);
  (b) one 4 KiB range with the host form mh_decode_ranges, wall clock, and mh_last_range_upload_bytes; against mh_decode of
      the whole stream with its index (host buffers, wall clock);
  (c) one range covering the whole stream with mh_dev_decode_ranges (fine index) against mh_dev_decode (reported, not gated).
Every output is checked against the input.  Prints one JSON line; medians with min and max.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/range_rate.py` run.

    python tools/range_rate.py [--gib 4] [--reps 5] [--ranges 65536]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=65536)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("range_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    chunk = 1024
    dev = "cuda"
    tile = zipf(256 << 20, 1)
    n = int(args.gib * (1 << 30)) // tile.size * tile.size
    d_data = torch.from_numpy(tile).to(dev).repeat(n // tile.size)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    # model, then payload + chunk index + fine index on the device
    hws = lib.mh_dev_histogram_workspace(n)
    d_hws = torch.empty(hws, dtype=torch.uint8, device=dev)
    d_counts = torch.empty(65536, dtype=torch.int64, device=dev)
    mhc._check(lib.mh_dev_histogram_o1(ptr(d_data), n, 0x20, ptr(d_counts), ptr(d_hws), hws, None), "histogram")
    model = mhc.Model.from_device_counts(ptr(d_counts), 1)
    cap = lib.mh_encode_bound(model.handle, n) + 64
    d_pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_nbits = torch.zeros(1, dtype=torch.int64, device=dev)
    nidx, nfine = (n + chunk - 1) // chunk, (n + 63) // 64
    d_idx = torch.empty(nidx, dtype=torch.int64, device=dev)
    d_fine = torch.empty(nfine, dtype=torch.int32, device=dev)
    ews = lib.mh_dev_encode_workspace(n)
    d_ews = torch.empty(ews, dtype=torch.uint8, device=dev)
    mhc._check(lib.mh_dev_encode_fine(model.handle, ptr(d_data), n, 0x20, None, ptr(d_pl), cap, ptr(d_nbits), ptr(d_idx), chunk,
                                      ptr(d_fine), ptr(d_hws), hws, ptr(d_ews), ews, None), "encode")
    mhc._check(lib.mh_dev_status(ptr(d_ews), None), "encode status")
    del d_ews, d_hws
    nbits = int(d_nbits.item())
    pbytes = (nbits + 7) // 8
    res = {"tool": "range_rate", "stream_bytes": n, "payload_bytes": pbytes, "chunk": chunk, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    # (a) random 256-byte ranges
    rng = np.random.default_rng(2)
    k = args.ranges
    b = rng.integers(0, n - 256, size=k).astype(np.uint64)
    rg = np.stack([b, b + np.uint64(256)], axis=1)
    d_rg = torch.from_numpy(rg.view(np.int64)).to(dev)
    d_at = torch.arange(k, dtype=torch.int64, device=dev) * 256
    d_out = torch.empty(k * 256, dtype=torch.uint8, device=dev)
    d_st = torch.empty(k, dtype=torch.int32, device=dev)
    rws = lib.mh_dev_decode_ranges_workspace(k)
    d_rws = torch.empty(rws, dtype=torch.uint8, device=dev)
    want = d_data[torch.from_numpy(rg[:, :1].astype(np.int64)).to(dev) + torch.arange(256, device=dev)].reshape(-1)

    def ranges_call(fine, rg_t=d_rg, at_t=d_at, kk=k, out=d_out, cap_out=k * 256):
        mhc._check(lib.mh_dev_decode_ranges(model.handle, ptr(d_pl), 0, pbytes, nbits, ptr(d_idx), chunk, n,
                                            ptr(d_fine) if fine else None, ptr(rg_t), kk, ptr(out), ptr(at_t), cap_out, ptr(d_st),
                                            ptr(d_rws), rws, None), "decode_ranges")

    a = {}
    for name, fine in (("chunk_index", False), ("fine_index", True)):
        d_out.fill_(0)
        ms = timed(lambda: ranges_call(fine), args.reps)
        assert lib.mh_dev_status(ptr(d_rws), None) == 0 and torch.equal(d_out, want), name
        a[name] = stats(ms)
    dws = lib.mh_dev_decode_workspace(nbits, n, chunk)
    d_dws = torch.empty(dws, dtype=torch.uint8, device=dev)
    d_all = torch.empty(n, dtype=torch.uint8, device=dev)
    gidx = (torch.from_numpy(rg[:, :1].astype(np.int64)).to(dev) + torch.arange(256, device=dev)).reshape(-1)
    gathered = {}

    def whole_and_gather():
        mhc._check(lib.mh_dev_decode_fine(model.handle, ptr(d_pl), nbits, None, ptr(d_all), n, ptr(d_idx), chunk, ptr(d_fine),
                                          ptr(d_dws), dws, None), "decode_fine")
        gathered["g"] = d_all[gidx]

    ms = timed(whole_and_gather, args.reps)
    assert lib.mh_dev_status(ptr(d_dws), None) == 0 and torch.equal(gathered["g"], want)
    a["whole_decode_fine_plus_gather"] = stats(ms)
    a["decode_path"] = lib.mh_dev_decode_path(ptr(d_dws), None)
    a["ranges"], a["range_bytes"] = k, 256
    a["speedup_fine_vs_whole"] = round(a["whole_decode_fine_plus_gather"]["median_ms"] / a["fine_index"]["median_ms"], 2)
    a["speedup_chunk_vs_whole"] = round(a["whole_decode_fine_plus_gather"]["median_ms"] / a["chunk_index"]["median_ms"], 2)
    res["a_random_256B_ranges"] = a
    del gathered["g"]

    # (b) one 4 KiB range from the host, against the whole stream from the host
    h_pl = d_pl[:pbytes].cpu().numpy()
    h_idx = d_idx.cpu().numpy().view(np.uint64)
    x = (n // 5 * 3) | 1
    one = [(x, x + 4096)]
    outs = {}
    ms = wall(lambda: outs.__setitem__("r", model.decode_ranges(h_pl, nbits, h_idx, chunk, n, one)), args.reps)
    assert outs["r"][0][0] == d_data[x:x + 4096].cpu().numpy().tobytes()
    bb = {"one_4KiB_range_host_form": stats(ms), "upload_bytes": int(lib.mh_last_range_upload_bytes())}
    h_out = np.empty(n, dtype=np.uint8)
    nb = C.c_size_t(0)

    def whole_host():
        mhc._check(lib.mh_decode(model.handle, h_pl.ctypes.data, nbits, 0x20, h_out.ctypes.data, n, C.byref(nb), h_idx.ctypes.data,
                                 chunk, n), "mh_decode")

    ms = wall(whole_host, max(1, min(args.reps, 3)))
    assert nb.value == n and h_out[x:x + 4096].tobytes() == outs["r"][0][0]
    bb["whole_stream_mh_decode"] = stats(ms)
    bb["whole_upload_bytes"] = pbytes
    res["b_one_range_host"] = bb
    del h_out

    # (c) one range covering the whole stream
    rg1 = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
    at1 = torch.zeros(1, dtype=torch.int64, device=dev)
    c = {}
    ms = timed(lambda: ranges_call(True, rg1, at1, 1, d_all, n), args.reps)
    assert lib.mh_dev_status(ptr(d_rws), None) == 0 and torch.equal(d_all, d_data)
    c["whole_range_fine_index"] = stats(ms)
    ms = timed(lambda: mhc._check(lib.mh_dev_decode(model.handle, ptr(d_pl), nbits, ptr(d_all), n, ptr(d_idx), chunk, ptr(d_dws), dws,
                                                    None), "decode"), args.reps)
    assert lib.mh_dev_status(ptr(d_dws), None) == 0 and torch.equal(d_all, d_data)
    c["whole_stream_mh_dev_decode"] = stats(ms)
    res["c_whole_range_device"] = c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
