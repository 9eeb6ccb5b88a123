"""What a length limit buys and costs (include/mh.h, mh_*_from_counts_limited).

In one process, after warm-up, on two sources (order 1, chunk 1024):
  zipf   --mib MiB of the benchmark's Zipf(1.1) stream (bench.py, seed 2);
  html   tests/golden/inputs/input_wiki_cpp.html tiled to --mib MiB, with its own histogram;
and for no limit and L = 12, 11, 10 each:
  longest code of the model, exact payload bits (mh_model_payload_bits) and their growth over no limit;
  model build: mh_dev_model_from_counts_limited_ws on the device counts (HIP events around the call, which ends in its
      one synchronisation), and how many contexts the limit re-codes;
  encode: mh_dev_encode_fine priced from the histogram workspace, with mh_dev_encode_path;
  decode: mh_dev_decode_fine with the fine index (mh_dev_decode_path) and mh_dev_decode with the chunk index alone
      (mh_dev_decode_variant).
The limits are measured in turn inside every repetition (unlimited first), so they share whatever else the machine is doing.
Every decode is checked against the input.  Prints one JSON line; medians with min and max.  Kernel times (tree_build_kernel,
limit_recode_kernel) come from a separate `rocprofv3 --kernel-trace --stats -- python tools/limit_rate.py --build-only` run;
--build-only also runs on a commit without the limited calls (then only L = 0 is built), for the comparison with it.

    python tools/limit_rate.py [--mib 256] [--reps 7] [--build-only]
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
import bench  # noqa: E402

LIMITS = (0, 12, 11, 10)
CHUNK = 1024


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Source:
    def __init__(self, mhc, name, data):
        lib = mhc.lib()
        self.name, self.n = name, data.size
        self.host = data
        self.d_data = mhc.DeviceBuffer(self.n + 32, init=np.concatenate([data, np.zeros(32, dtype=np.uint8)]))
        self.d_counts = mhc.DeviceBuffer(65536 * 8)
        self.hws = int(lib.mh_dev_histogram_workspace(self.n))
        self.d_hws = mhc.DeviceBuffer(self.hws)
        mhc._check(lib.mh_dev_histogram_o1(self.d_data.ptr, self.n, 0x20, self.d_counts.ptr, self.d_hws.ptr, self.hws, None), "hist")
        self.counts = self.d_counts.download(np.uint64)
        self.mws = int(lib.mh_dev_model_workspace(1))


def build(mhc, src, d_ws, L, limited_calls):
    if limited_calls:
        return mhc.Model.from_device_counts_ws(src.d_counts.ptr, 1, d_ws.ptr, src.mws, max_len=L)
    return mhc.Model.from_device_counts_ws(src.d_counts.ptr, 1, d_ws.ptr, src.mws)


def measure_builds(mhc, src, reps, limits, limited_calls):
    d_ws = {L: mhc.DeviceBuffer(src.mws) for L in limits}
    ms = {L: [] for L in limits}
    for L in limits:                                        # warm-up: code objects, the pinned landing place
        build(mhc, src, d_ws[L], L, limited_calls)
    for _ in range(reps):
        for L in limits:
            ms[L].append(event_ms(lambda: build(mhc, src, d_ws[L], L, limited_calls)))
    return {L: stats(ms[L]) for L in limits}


def measure_coding(mhc, src, models, reps):
    lib = mhc.lib()
    n = src.n
    nidx, nfine = (n + CHUNK - 1) // CHUNK, (n + 63) // 64
    cap = max(int(lib.mh_encode_bound(m.handle, n)) for m in models.values()) + 64
    ews = int(lib.mh_dev_encode_workspace(n))
    st = {}
    for L in models:
        st[L] = dict(d_payload=mhc.DeviceBuffer(cap), d_nbits=mhc.DeviceBuffer(8), d_index=mhc.DeviceBuffer(nidx * 8),
                     d_fine=mhc.DeviceBuffer(nfine * 4), d_ews=mhc.DeviceBuffer(ews + 64), d_out=mhc.DeviceBuffer(n + 64),
                     enc=[], dec_fine=[], dec_chunk=[])

    def encode(L):
        s = st[L]
        mhc._check(lib.mh_dev_encode_fine(models[L].handle, src.d_data.ptr, n, 0x20, None, s["d_payload"].ptr, cap, s["d_nbits"].ptr,
                                          s["d_index"].ptr, CHUNK, s["d_fine"].ptr, src.d_hws.ptr, src.hws, s["d_ews"].ptr, ews, None), "encode")

    def decode(L, fine):
        s = st[L]
        if fine:
            mhc._check(lib.mh_dev_decode_fine(models[L].handle, s["d_payload"].ptr, s["nbits"], None, s["d_out"].ptr, n, s["d_index"].ptr,
                                              CHUNK, s["d_fine"].ptr, s["d_dws"].ptr, s["dws"], None), "decode_fine")
        else:
            mhc._check(lib.mh_dev_decode_fine(models[L].handle, s["d_payload"].ptr, s["nbits"], None, s["d_out"].ptr, n, s["d_index"].ptr,
                                              CHUNK, None, s["d_dws"].ptr, s["dws"], None), "decode")

    out = {}
    for L in models:                                        # warm-up + the facts that do not vary
        s = st[L]
        encode(L)
        mhc._check(lib.mh_dev_status(s["d_ews"].ptr, None), "encode status")
        s["nbits"] = int(s["d_nbits"].download(np.uint64)[0])
        s["dws"] = int(lib.mh_dev_decode_workspace(s["nbits"], n, CHUNK))
        s["d_dws"] = mhc.DeviceBuffer(s["dws"])
        out[L] = {"encode_path": lib.mh_dev_encode_path(s["d_ews"].ptr, None), "nbits": s["nbits"]}
        for fine in (True, False):
            decode(L, fine)
            mhc._check(lib.mh_dev_status(s["d_dws"].ptr, None), "decode status")
            assert np.array_equal(s["d_out"].download()[:n], src.host), "decode differs from the input"
            key = "decode_fine" if fine else "decode_chunk"
            out[L][key + "_path"] = lib.mh_dev_decode_path(s["d_dws"].ptr, None)
            out[L][key + "_variant"] = lib.mh_dev_decode_variant(s["d_dws"].ptr, None)
    for _ in range(reps):
        for L in models:
            st[L]["enc"].append(event_ms(lambda: encode(L)))
        for L in models:
            st[L]["dec_fine"].append(event_ms(lambda: decode(L, True)))
        for L in models:
            st[L]["dec_chunk"].append(event_ms(lambda: decode(L, False)))
    for L in models:
        out[L].update(encode=stats(st[L]["enc"]), decode_fine=stats(st[L]["dec_fine"]), decode_chunk=stats(st[L]["dec_chunk"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("limit_rate.py needs a GPU (and torch for the event timing)")
    limited_calls = "mh_dev_model_from_counts_limited_ws" in mhc.EXPORTS
    limits = LIMITS if limited_calls else (0,)
    n = args.mib << 20
    with open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.html"), "rb") as f:
        one = np.frombuffer(f.read(), dtype=np.uint8)
    sources = [Source(mhc, "zipf", bench.synth_slice("zipf", 2, 0, n, device="cuda").cpu().numpy()), Source(mhc, "html", np.tile(one, n // one.size + 1)[:n].copy())]
    res = {"tool": "limit_rate", "mib": args.mib, "reps": args.reps, "chunk": CHUNK, "limited_calls": limited_calls, "sources": {}}
    for src in sources:
        builds = measure_builds(mhc, src, args.reps * 3, limits, limited_calls)
        d_ws = {L: mhc.DeviceBuffer(src.mws) for L in limits}
        models = {L: build(mhc, src, d_ws[L], L, limited_calls) for L in limits}
        free_lens = np.frombuffer(models[0].image(1), dtype=np.uint8).reshape(256, 256)
        rows = {}
        for L in limits:
            bits = models[L].payload_bits(src.counts) if hasattr(models[L], "payload_bits") else None
            rows[L] = {"max_code_len": models[L].max_code_len, "payload_bits": bits, "build": builds[L],
                       "contexts_recoded": int((free_lens.max(axis=1) > L).sum()) if L else 0,
                       "tile_layout": list(models[L].tile_layout()), "decode_layout": list(models[L].decode_layout())}
            if bits is not None and rows[0]["payload_bits"]:
                rows[L]["payload_growth_percent"] = round(100.0 * (bits - rows[0]["payload_bits"]) / rows[0]["payload_bits"], 5)
        if not args.build_only:
            for L, r in measure_coding(mhc, src, models, args.reps).items():
                assert rows[L]["payload_bits"] in (None, r["nbits"])
                rows[L].update(r)
        res["sources"][src.name] = {"bytes": src.n, "limits": {str(L): rows[L] for L in limits}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
