"""Lookup rate into batches (include/mh.h, "RANDOM ACCESS INTO BATCHES").

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), each coded under a shared order-1 model and under per-stream order-1 models (chunk 1024):
  (a) 4 096 random 256-byte lookups with mh_dev_decode_batch_ranges / mh_dev_decode_each_ranges, HIP events, with the chunk
      index and index-free; against mh_dev_decode_batch / mh_dev_decode_each of the whole batch followed by a gather of the
      same bytes (torch indexing);
  (b) the host forms, wall clock: one lookup and 4 096 lookups (shared model, indexed), with mh_last_batch_range_upload_bytes;
      against a loop of mh_decode_ranges over the same lookups, one call per lookup (256 calls timed, scaled to 4 096);
  (c) the crossover: lookup counts 2^10 ... 2^18 against the whole-batch decode plus gather (reported, not gated).
Every output is checked against the input.  Prints one JSON line; medians with min and max.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/batch_range_rate.py` run.

    python tools/batch_range_rate.py [--streams 65536] [--bytes 4096] [--reps 5] [--lookups 4096] [--max-log2 18]
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

CHUNK = 1024
LEN = 256
PREV0 = 0x20


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


def ptr(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to("cuda")


class Coded:
    """One batch on the device: payloads, pay_off, nbits, sym_off (= in_off), index; plus the shared model or the set."""

    def __init__(self, mhc, data, n_streams, per, kind):
        self.mhc, self.kind, self.n, self.per = mhc, kind, n_streams, per
        msgs = [data[i * per:(i + 1) * per].tobytes() for i in range(n_streams)]
        if kind == "shared":
            self.model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)     # every message starts in context PREV0
            payload, pay_off, nbits, idx, in_off = self.model.encode_batch(msgs, chunk_symbols=CHUNK)
            self.handle = self.model.handle
        else:
            self.set = mhc.ModelSet.train(msgs, order=1)
            payload, pay_off, nbits, idx, in_off, rc = self.set.encode(msgs, chunk_symbols=CHUNK)
            assert rc == mhc.MH_OK
            self.handle = self.set.handle
        self.h_payload, self.h_pay_off, self.h_nbits, self.h_idx, self.h_in_off = payload, pay_off, nbits, idx, in_off
        self.d_payload = dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)]))
        self.d_pay_off, self.d_nbits, self.d_in_off, self.d_idx = dev(pay_off), dev(nbits), dev(in_off), dev(idx)
        self.d_data = dev(data[:n_streams * per])
        self.total = n_streams * per


def lookups(n_streams, per, k, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, n_streams, k).astype(np.uint64)
    b = rng.integers(0, per - LEN + 1, k).astype(np.uint64)
    return np.stack([s, b, b + np.uint64(LEN)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lookups", type=int, default=4096)
    ap.add_argument("--max-log2", type=int, default=18)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("batch_range_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total)}
    res = {"tool": "batch_range_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "lookup_bytes": LEN, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        out = {}
        for kind in ("shared", "each"):
            cd = Coded(mhc, data, n, per, kind)
            r = {"payload_bytes": int(cd.h_pay_off[-1])}
            dev_fn = lib.mh_dev_decode_batch_ranges if kind == "shared" else lib.mh_dev_decode_each_ranges

            def run(lk_t, at_t, m, out_t, st_t, ws_t, indexed):
                mhc._check(dev_fn(cd.handle, ptr(cd.d_payload), ptr(cd.d_pay_off), ptr(cd.d_nbits), n, PREV0,
                                  ptr(cd.d_in_off) if indexed else None, ptr(cd.d_idx) if indexed else None, CHUNK if indexed else 0,
                                  ptr(lk_t), m, ptr(out_t), ptr(at_t), m * LEN, ptr(st_t), ptr(ws_t), ws_t.numel(), None), kind)

            def setup(m, seed):
                lk = lookups(n, per, m, seed)
                gidx = (torch.from_numpy((lk[:, 0] * np.uint64(per) + lk[:, 1]).astype(np.int64)).to("cuda")[:, None]
                        + torch.arange(LEN, device="cuda")).reshape(-1)
                return (lk, dev(lk), torch.arange(m, dtype=torch.int64, device="cuda") * LEN, torch.empty(m * LEN, dtype=torch.uint8, device="cuda"),
                        torch.empty(m, dtype=torch.int32, device="cuda"),
                        torch.empty(lib.mh_dev_decode_batch_ranges_workspace(m), dtype=torch.uint8, device="cuda"), gidx)

            # whole-batch decode + gather (the alternative)
            wsb = (lib.mh_dev_decode_batch_workspace if kind == "shared" else lib.mh_dev_decode_each_workspace)(n)
            d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
            d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            whole_fn = lib.mh_dev_decode_batch if kind == "shared" else lib.mh_dev_decode_each
            pay_total = int(cd.h_pay_off[-1])

            def whole(indexed):
                if indexed:
                    d_so.copy_(cd.d_in_off)
                mhc._check(whole_fn(cd.handle, ptr(cd.d_payload), ptr(cd.d_pay_off), ptr(cd.d_nbits), n, pay_total, PREV0, ptr(d_all), total,
                                    ptr(d_so), total, ptr(cd.d_idx) if indexed else None, CHUNK if indexed else 0, None, ptr(d_ws), wsb,
                                    None), "whole")

            # (a)
            lk, d_lk, d_at, d_out, d_st, d_rws, gidx = setup(args.lookups, 2)
            want = cd.d_data[gidx]
            a = {}
            for mode, indexed in (("indexed", True), ("index_free", False)):
                d_out.zero_()
                ms = timed(lambda: run(d_lk, d_at, args.lookups, d_out, d_st, d_rws, indexed), args.reps)
                assert lib.mh_dev_status(ptr(d_rws), None) == 0 and torch.equal(d_out, want), (dname, kind, mode)
                a[mode] = stats(ms)
                g = {}
                ms = timed(lambda: (whole(indexed), g.__setitem__("g", d_all[gidx])), args.reps)
                assert lib.mh_dev_status(ptr(d_ws), None) == 0 and torch.equal(g["g"], want), (dname, kind, "whole", mode)
                a["whole_plus_gather_" + mode] = stats(ms)
                a["speedup_" + mode] = round(a["whole_plus_gather_" + mode]["median_ms"] / a[mode]["median_ms"], 2)
            r["a_device"] = a

            # (c) crossover, indexed and index-free
            c = {}
            for mode, indexed in (("indexed", True), ("index_free", False)):
                sweep, cross = [], None
                for lg in range(10, args.max_log2 + 1):
                    m = 1 << lg
                    lk2, d_lk2, d_at2, d_out2, d_st2, d_rws2, gidx2 = setup(m, 100 + lg)
                    ms = timed(lambda: run(d_lk2, d_at2, m, d_out2, d_st2, d_rws2, indexed), max(3, args.reps // 2))
                    assert lib.mh_dev_status(ptr(d_rws2), None) == 0 and torch.equal(d_out2, cd.d_data[gidx2]), (dname, kind, mode, m)
                    g = {}
                    msw = timed(lambda: (whole(indexed), g.__setitem__("g", d_all[gidx2])), max(3, args.reps // 2))
                    assert torch.equal(g["g"], cd.d_data[gidx2])
                    lk_ms, w_ms = float(np.median(ms)), float(np.median(msw))
                    sweep.append({"lookups": m, "lookup_ms": round(lk_ms, 4), "whole_plus_gather_ms": round(w_ms, 4)})
                    if cross is None and w_ms <= lk_ms:
                        cross = m
                    del d_out2, d_lk2, d_at2, d_st2, d_rws2, gidx2, g
                c[mode] = {"sweep": sweep, "whole_cheaper_from": cross}
            r["c_crossover"] = c

            # (b) host forms, shared model only for the loop comparison
            if kind == "shared":
                b = {}
                one = lk[:1]
                outs = {}
                ms = wall(lambda: outs.__setitem__("r", cd.model.decode_batch_ranges(cd.h_payload, cd.h_pay_off, cd.h_nbits, one, sym_off=cd.h_in_off,
                                                                                     index=cd.h_idx, chunk_symbols=CHUNK)), args.reps)
                s0, b0, e0 = (int(x) for x in one[0])
                assert outs["r"][0][0] == data[s0 * per + b0:s0 * per + e0].tobytes()
                b["one_lookup"] = stats(ms)
                b["one_lookup_upload_bytes"] = int(lib.mh_last_batch_range_upload_bytes())
                ms = wall(lambda: outs.__setitem__("r", cd.model.decode_batch_ranges(cd.h_payload, cd.h_pay_off, cd.h_nbits, lk, sym_off=cd.h_in_off,
                                                                                     index=cd.h_idx, chunk_symbols=CHUNK)), args.reps)
                got = np.frombuffer(b"".join(outs["r"][0]), dtype=np.uint8)
                assert np.array_equal(got, cd.d_data[gidx].cpu().numpy())
                b["lookups_%d" % args.lookups] = stats(ms)
                b["lookups_upload_bytes"] = int(lib.mh_last_batch_range_upload_bytes())
                loop_n = min(256, args.lookups)

                def loop():
                    for s, x, y in lk[:loop_n]:
                        s = int(s)
                        base = lib.mh_batch_index_base(int(cd.h_in_off[s]), s, CHUNK)
                        r1, st1 = cd.model.decode_ranges(cd.h_payload[int(cd.h_pay_off[s]):int(cd.h_pay_off[s + 1])], int(cd.h_nbits[s]),
                                                         cd.h_idx[base:base + (per + CHUNK - 1) // CHUNK], CHUNK, per, [(int(x), int(y))])
                        assert st1[0] == 0 and r1[0] == data[s * per + int(x):s * per + int(y)].tobytes()

                ms = wall(loop, max(1, args.reps // 2))
                b["decode_ranges_loop_%d_calls" % loop_n] = stats(ms)
                b["decode_ranges_loop_scaled_to_%d_ms" % args.lookups] = round(float(np.median(ms)) * args.lookups / loop_n, 3)
                b["speedup_host_form_vs_loop"] = round(b["decode_ranges_loop_scaled_to_%d_ms" % args.lookups] / b["lookups_%d" % args.lookups]["median_ms"], 1)
                r["b_host"] = b
            out[kind] = r
            del cd, d_all, d_ws
            torch.cuda.empty_cache()
        res[dname] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
