"""Rate of re-coding compressed batches (include/mh.h, "RE-CODING BATCHES") against what a caller did before: decode the
batch into a buffer, then histogram or encode that buffer.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), coded under a shared order-1 model with chunk 1024, HIP events, every variant run once per
repetition in turn (interleaved), medians with min and max:
  1. the yardsticks: mh_dev_decode_batch + mh_dev_histogram_o1_batch, and mh_dev_decode_batch + mh_dev_encode_batch(dst);
  2. mh_dev_histogram_coded_batch (shared source) and mh_dev_histogram_coded_each (per-stream models), indexed;
  3. mh_dev_recode_batch indexed: shared -> shared, per-stream models -> shared, shared -> its L = 12 limited form;
  4. mh_dev_recode_batch index-free, and count-only (indexed).
The uniform-bytes batch (every pair cold for the histogram's cache) is measured once and reported whatever it shows.
Every result is checked against the composition's output before the clock.  Prints one JSON line; `ratio` is the variant's
median over its yardstick's.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python
tools/recode_rate.py --reps 1` run.

    python tools/recode_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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

CHUNK = 1024
PREV0 = 0x20


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to("cuda")


def interleaved(fns, reps, warm=1):
    """name -> list of ms: every function once per repetition, in turn."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("recode_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy(),
                "uniform": np.random.default_rng(3).integers(0, 256, total, dtype=np.uint8)}
    res = {"tool": "recode_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        once = dname == "uniform"
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        counts = mhc.histogram_o1_batch(msgs)
        src = mhc.Model.from_counts(counts, 1)
        half = mhc.histogram_o1_batch(msgs[::2])
        dst = mhc.Model.from_counts(half + np.uint64(1), 1)                  # another model that covers every pair
        lim = mhc.Model.from_counts(counts, 1, max_len=12)
        payload, pay_off, nbits, idx, in_off = src.encode_batch(msgs, chunk_symbols=CHUNK)
        pay_total = int(pay_off[-1])
        d = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off),
                 idx=dev(idx))
        e = None
        if not once:
            ms_set = mhc.ModelSet.train(msgs, order=1)
            e_payload, e_pay_off, e_nbits, e_idx, e_in_off, rc = ms_set.encode(msgs, chunk_symbols=CHUNK)
            assert rc == mhc.MH_OK
            e = dict(payload=dev(np.concatenate([e_payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(e_pay_off), nbits=dev(e_nbits),
                     in_off=dev(e_in_off), idx=dev(e_idx), pay_total=int(e_pay_off[-1]))
        cap = int(max(lib.mh_encode_batch_bound(m.handle, total, n) for m in (dst, lim)))
        nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
        wsb = max(lib.mh_dev_recode_batch_workspace(n, total, CHUNK), lib.mh_dev_histogram_coded_workspace(n, total, CHUNK),
                  lib.mh_dev_decode_batch_workspace(n), lib.mh_dev_encode_batch_workspace(n, total), lib.mh_dev_histogram_batch_workspace(total))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_counts = torch.empty(65536, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(nidx, dtype=torch.int64, device="cuda")) for k in ("ref", "got")}
        d_drop = torch.empty(n, dtype=torch.int64, device="cuda")

        def decode():
            d_so.copy_(d["in_off"])
            mhc._check(lib.mh_dev_decode_batch(src.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0, ptr(d_all),
                                               total, ptr(d_so), total, ptr(d["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def decode_hist():
            decode()
            mhc._check(lib.mh_dev_histogram_o1_batch(ptr(d_all), ptr(d["in_off"]), n, total, PREV0, ptr(d_counts), ptr(d_ws), wsb, None), "hist")

        def decode_encode(m=dst):
            decode()
            o = out["ref"]
            mhc._check(lib.mh_dev_encode_batch(m.handle, ptr(d_all), ptr(d["in_off"]), n, total, PREV0, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                               CHUNK, ptr(d_ws), wsb, None), "encode")

        def hist_coded(each=False):
            b = e if each else d
            fn = lib.mh_dev_histogram_coded_each if each else lib.mh_dev_histogram_coded_batch
            mhc._check(fn(ms_set.handle if each else src.handle, 1, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n,
                          b["pay_total"] if each else pay_total, PREV0, ptr(b["in_off"]), total, ptr(b["idx"]), CHUNK, ptr(d_counts), None, ptr(d_ws), wsb,
                          None), "histogram_coded")

        def recode(m=dst, each=False, indexed=True, count_only=False):
            b = e if each else d
            o = out["got"]
            fn = lib.mh_dev_recode_each if each else lib.mh_dev_recode_batch
            so = b["in_off"] if indexed else d_so
            mhc._check(fn(ms_set.handle if each else src.handle, m.handle, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n,
                          b["pay_total"] if each else pay_total, PREV0, ptr(so), total, ptr(b["idx"]) if indexed else None, CHUNK,
                          None if count_only else ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), None if count_only else ptr(o[3]), ptr(d_drop), None,
                          ptr(d_ws), wsb, None), "recode")

        def same(what, payload_too=True):
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, what)
            r, g = out["ref"], out["got"]
            assert torch.equal(r[1], g[1]) and torch.equal(r[2], g[2]), (dname, what)
            if payload_too:
                k = int(r[1][-1].item())
                assert torch.equal(r[0][:k], g[0][:k]) and torch.equal(r[3], g[3]), (dname, what)

        # every variant's result against the composition's, before the clock
        decode_hist()
        want_counts = d_counts.clone()
        assert np.array_equal(want_counts.cpu().numpy().view(np.uint64), counts)
        for each in ((False,) if once else (False, True)):
            d_counts.zero_()
            hist_coded(each)
            assert lib.mh_dev_status(ptr(d_ws), None) == 0 and torch.equal(d_counts, want_counts), (dname, each)
        if not once:
            for m, name in ((dst, "dst"), (lim, "limited")):
                decode_encode(m)
                for kw in (dict(), dict(indexed=False)) + ((dict(each=True),) if m is dst else ()):
                    for t in out["got"]:
                        t.zero_()
                    recode(m, **kw)
                    same((name, kw))
                recode(m, count_only=True)
                same((name, "count"), payload_too=False)
            assert int(d_drop.sum().item()) == 0
            decode_encode(dst)

        if once:
            fns = {"decode_then_histogram": decode_hist, "histogram_coded": hist_coded}
            ms = interleaved(fns, 1)
        else:
            fns = {"decode_then_histogram": decode_hist, "decode_then_encode": decode_encode, "decode_then_encode_limited": lambda: decode_encode(lim),
                   "histogram_coded": hist_coded, "histogram_coded_each": lambda: hist_coded(True),
                   "recode": recode, "recode_each": lambda: recode(each=True), "recode_limited": lambda: recode(lim),
                   "recode_index_free": lambda: recode(indexed=False), "recode_count_only": lambda: recode(count_only=True)}
            ms = interleaved(fns, args.reps)
        o = {k: stats(v) for k, v in ms.items()}
        for k in [k for k in o if not k.startswith("decode_")]:
            base = "decode_then_histogram" if k.startswith("histogram") else ("decode_then_encode_limited" if k.endswith("limited") else "decode_then_encode")
            if base in o:
                o[k]["ratio"] = round(o[k]["median_ms"] / o[base]["median_ms"], 3)
        o["payload_bytes"] = pay_total
        o["workspace_bytes"] = {"recode": int(lib.mh_dev_recode_batch_workspace(n, total, CHUNK)),
                                "histogram_coded": int(lib.mh_dev_histogram_coded_workspace(n, total, CHUNK)), "decoded_buffer": total}
        if not once:
            o["recode_bound_1.0"] = bool(o["recode"]["ratio"] <= 1.0)
            o["histogram_bound_1.0"] = bool(o["histogram_coded"]["ratio"] <= 1.0)
        res[dname] = o
        del d, e, d_all, d_ws, out
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
