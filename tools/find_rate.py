"""Search rate in compressed batches (include/mh.h, "SEARCH IN BATCHES") against the decode of the same batch.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), coded under a shared order-1 model with chunk 1024, HIP events, every variant run once per
repetition in turn (interleaved), medians with min and max:
  1. mh_dev_decode_batch, indexed: the yardstick, measured beside the search;
  2. mh_dev_find_batch count-only, indexed: a rare pattern (12 bytes planted 100 times) and a frequent one (a two-byte pair
     with over 100 000 hits), as one pattern and inside a full set of 64 positions;
  3. the same with records;
  4. index-free, count-only and with records;
  5. mh_dev_find_each (per-stream models), indexed, count-only and with records;
  6. what a caller does without the search: (1) followed by a search of the decoded buffer, with torch on the device and with
     bytes.find on the host after the copy (reported, not gated).
Every result is checked against tests/find_ref.py.  Prints one JSON line; `ratio` is the variant's median over the decode's.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/find_rate.py --reps 1` run.

    python tools/find_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import find_ref  # noqa: E402

CHUNK = 1024
PREV0 = 0x20
PLANTED = b"\xf0needle\xf1-12\xf2"


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


def frequent_pair(data, per, lo=100_000):
    """A two-byte pair with a little over `lo` occurrences inside the messages."""
    d = data.astype(np.int32)
    pairs = d[:-1] * 256 + d[1:]
    pairs = np.delete(pairs, np.arange(per - 1, pairs.size, per))       # the pairs across message boundaries
    h = np.bincount(pairs, minlength=65536)
    cand = np.flatnonzero(h > lo * 1.2)
    p = int(cand[np.argmin(h[cand])])
    return bytes([p >> 8, p & 255])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("find_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "find_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        rng = np.random.default_rng(9)
        for i in rng.choice(n, size=100, replace=False):                 # the rare pattern: 100 known places
            at = int(i) * per + int(rng.integers(0, per - len(PLANTED)))
            data[at:at + len(PLANTED)] = np.frombuffer(PLANTED, dtype=np.uint8)
        pair = frequent_pair(data, per)
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        cands = sorted({raw[int(at):int(at) + 4] for at in rng.integers(0, total - 4, 100)})    # four-byte strings of the data for the
        cands.sort(key=lambda g: len(find_ref.occurrences(raw[:1 << 24], g)))                   # full set: the less frequent ones
        grams = cands[:12]
        full = [PLANTED, pair] + grams + [raw[5:7]]
        assert sum(len(p) for p in full) == mhc.FIND_MAX_POSITIONS
        sets = {"rare": [PLANTED], "frequent": [pair], "full64": full}
        want = {}
        for k, pats in sets.items():
            t0 = time.perf_counter()
            want[k] = find_ref.hit_arrays(find_ref.find_hits(msgs, pats), n)
            print("[find_rate] %s %s: %d reference hits (%.1f s)" % (dname, k, want[k][1].shape[0], time.perf_counter() - t0), file=sys.stderr)
        assert want["rare"][1].shape[0] == 100 and want["frequent"][1].shape[0] > 100_000
        ps = {k: mhc.PatternSet(p) for k, p in sets.items()}

        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        payload, pay_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=CHUNK)
        ms_set = mhc.ModelSet.train(msgs, order=1)
        e_payload, e_pay_off, e_nbits, e_idx, e_in_off, rc = ms_set.encode(msgs, chunk_symbols=CHUNK)
        assert rc == mhc.MH_OK
        pay_total = int(pay_off[-1])
        d = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off), idx=dev(idx))
        e = dict(payload=dev(np.concatenate([e_payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(e_pay_off), nbits=dev(e_nbits), in_off=dev(e_in_off),
                 idx=dev(e_idx))
        d_data = dev(data)
        wsb = max(lib.mh_dev_find_batch_workspace(n, total, CHUNK), lib.mh_dev_decode_batch_workspace(n))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        cap = max(w[1].shape[0] for w in want.values())
        d_hits = torch.empty(cap * 3, dtype=torch.int64, device="cuda")
        d_pat = torch.empty(cap, dtype=torch.int32, device="cuda")

        def decode():
            d_so.copy_(d["in_off"])
            mhc._check(lib.mh_dev_decode_batch(model.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0, ptr(d_all),
                                               total, ptr(d_so), total, ptr(d["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def find(which, records, indexed=True, each=False):
            b = e if each else d
            fn = lib.mh_dev_find_each if each else lib.mh_dev_find_batch
            h = ms_set.handle if each else model.handle
            mhc._check(fn(h, ps[which].handle, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n, int((e_pay_off if each else pay_off)[-1]),
                          PREV0, ptr(b["in_off"]) if indexed else None, total, ptr(b["idx"]) if indexed else None, CHUNK if indexed else 0,
                          ptr(d_ho), ptr(d_hits) if records else None, ptr(d_pat) if records else None, cap, None, ptr(d_ws), wsb, None), "find")

        def verify(which, records, **kw):
            d_ho.zero_(); d_hits.zero_(); d_pat.zero_()
            find(which, records, **kw)
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, which, records, kw)
            off, rec, pat = want[which]
            assert np.array_equal(d_ho.cpu().numpy().view(np.uint64), off), (dname, which, records, kw)
            if records:
                k = rec.shape[0]
                assert np.array_equal(d_hits.cpu().numpy().view(np.uint64)[:3 * k].reshape(-1, 3), rec), (dname, which, kw)
                assert np.array_equal(d_pat.cpu().numpy().view(np.uint32)[:k], pat), (dname, which, kw)

        a, b2 = int(pair[0]), int(pair[1])
        seen = {}

        def decode_then_torch():
            decode()
            m = (d_all[:-1] == a) & (d_all[1:] == b2)
            seen["torch"] = int(m.sum().item())                          # (pairs across message boundaries included: a caller masks them)

        fns = {"decode_indexed": decode}
        for which in ("rare", "frequent", "full64"):
            fns["count_" + which] = lambda w=which: find(w, False)
            fns["records_" + which] = lambda w=which: find(w, True)
        for which in ("rare", "frequent"):
            fns["index_free_count_" + which] = lambda w=which: find(w, False, indexed=False)
            fns["index_free_records_" + which] = lambda w=which: find(w, True, indexed=False)
            fns["each_count_" + which] = lambda w=which: find(w, False, each=True)
            fns["each_records_" + which] = lambda w=which: find(w, True, each=True)
        fns["decode_then_torch_pair"] = decode_then_torch
        for which in sets:                                               # every variant's result against the reference, before the clock
            for records in (False, True):
                verify(which, records)
                if which != "full64":
                    verify(which, records, indexed=False)
                    verify(which, records, each=True)
        decode()
        assert torch.equal(d_all, d_data)
        ms = interleaved(fns, args.reps)
        out = {k: stats(v) for k, v in ms.items()}
        base = out["decode_indexed"]["median_ms"]
        for k in out:
            out[k]["ratio"] = round(out[k]["median_ms"] / base, 3)
        boundary = sum(1 for i in range(1, n) if raw[i * per - 1] == a and raw[i * per] == b2)
        assert seen["torch"] == want["frequent"][1].shape[0] + boundary
        t0 = time.perf_counter()
        decode()
        host = d_all.cpu().numpy().tobytes()
        t1 = time.perf_counter()
        k = sum(len(find_ref.occurrences(host[i * per:(i + 1) * per], pair)) for i in range(n))
        t2 = time.perf_counter()
        assert k == want["frequent"][1].shape[0]
        out["decode_copy_then_bytes_find_pair"] = {"decode_and_copy_ms": round((t1 - t0) * 1e3, 1), "bytes_find_ms": round((t2 - t1) * 1e3, 1)}
        out["hits"] = {k: int(w[1].shape[0]) for k, w in want.items()}
        out["payload_bytes"] = pay_total
        out["workspace_bytes"] = int(lib.mh_dev_find_batch_workspace(n, total, CHUNK))
        out["count_only_bound_1.25"] = bool(max(out["count_" + w]["ratio"] for w in sets) <= 1.25)
        res[dname] = out
        del d, e, d_data, d_all, d_hits, d_pat, d_ws
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
