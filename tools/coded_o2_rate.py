"""Rate of the order-2 family of search, coded histogram and re-coding (include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING")
against what a caller did before: decode the batch into a buffer, then search, histogram or encode that buffer.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), coded under a shared order-1 and a shared order-2 model with chunk 1024, HIP events, every variant
run once per repetition in turn (interleaved), medians with min and max:
  1. the yardsticks: mh_dev_decode_batch_o2 (indexed and index-free), mh_dev_decode_batch + mh_dev_encode_batch_o2,
     mh_dev_decode_batch_o2 + mh_dev_encode_batch, mh_dev_decode_batch + mh_dev_histogram_o2_batch;
  2. mh_dev_find_batch_o2 count-only and with records, indexed and index-free;
  3. mh_dev_recode_batch_o2 order 1 -> 2 and order 2 -> 1, indexed;
  4. mh_dev_histogram_coded_batch_o2, order 2 from the order-1 batch.
Order 2 -> order 2 is left out: its yardstick would be the length-limited form of the same counts, and no length-limited
order-2 model exists.  The uniform-bytes batch (every triple cold for the histogram's cache) is measured once for the
histogram and reported whatever it shows.  Every result is checked before the clock: hits against tests/find_ref.py on the
messages, re-coded batches and counts against the composition's output.  Prints one JSON line; `ratio` is the variant's
median over its yardstick's.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python
tools/coded_o2_rate.py --reps 1` run.

    python tools/coded_o2_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import find_ref  # noqa: E402

CHUNK = 1024
PREV0 = 0x20
PATTERNS = {"zipf1.1": bytes([0, 1, 0]), "text": b"language"}


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


YARDSTICK = {"find_count_indexed": "decode_o2_indexed", "find_records_indexed": "decode_o2_indexed",
             "find_count_index_free": "decode_o2_index_free", "find_records_index_free": "decode_o2_index_free",
             "recode_o1_to_o2": "decode_o1_then_encode_o2", "recode_o2_to_o1": "decode_o2_then_encode_o1",
             "histogram_coded_o2_from_o1": "decode_o1_then_histogram_o2"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("coded_o2_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy(),
                "uniform": np.random.default_rng(3).integers(0, 256, total, dtype=np.uint8)}
    res = {"tool": "coded_o2_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        once = dname == "uniform"
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        c1 = mhc.histogram_o1_batch(msgs)
        c2 = mhc.histogram_o2_batch(msgs)
        m1 = mhc.Model.from_counts(c1, 1)
        p1, po1, nb1, idx1, in_off = m1.encode_batch(msgs, chunk_symbols=CHUNK)
        b1 = dict(payload=dev(np.concatenate([p1, np.zeros(64, dtype=np.uint8)])), pay_off=dev(po1), nbits=dev(nb1), idx=dev(idx1), total=int(po1[-1]))
        d_in_off = dev(in_off)
        m2, b2 = None, None
        if not once:
            m2 = mhc.Model.from_counts(c2, 2)
            p2, po2, nb2, idx2, _ = m2.encode_batch_o2(msgs, chunk_symbols=CHUNK)
            b2 = dict(payload=dev(np.concatenate([p2, np.zeros(64, dtype=np.uint8)])), pay_off=dev(po2), nbits=dev(nb2), idx=dev(idx2),
                      total=int(po2[-1]))
        models = [m for m in (m1, m2) if m is not None]
        cap = int(max(lib.mh_encode_batch_bound(m.handle, total, n) for m in models))
        nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
        wsb = max(lib.mh_dev_recode_batch_o2_workspace(n, total, CHUNK), lib.mh_dev_histogram_coded_batch_o2_workspace(n, total, CHUNK),
                  lib.mh_dev_find_batch_o2_workspace(n, total, CHUNK), lib.mh_dev_decode_batch_workspace(n), lib.mh_dev_decode_batch_o2_workspace(n),
                  lib.mh_dev_encode_batch_workspace(n, total), lib.mh_dev_encode_batch_o2_workspace(n, total),
                  lib.mh_dev_histogram_o2_batch_workspace(total))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_counts = torch.empty(1 << 24, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(nidx, dtype=torch.int64, device="cuda")) for k in ("ref", "got")}
        d_drop = torch.empty(n, dtype=torch.int64, device="cuda")

        def decode(o2, indexed=True):
            m, b = (m2, b2) if o2 else (m1, b1)
            fn = lib.mh_dev_decode_batch_o2 if o2 else lib.mh_dev_decode_batch
            if indexed:
                d_so.copy_(d_in_off)
            mhc._check(fn(m.handle, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n, b["total"], PREV0, ptr(d_all), total, ptr(d_so),
                          total if indexed else 0, ptr(b["idx"]) if indexed else None, CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def encode(o2):
            m = m2 if o2 else m1
            fn = lib.mh_dev_encode_batch_o2 if o2 else lib.mh_dev_encode_batch
            o = out["ref"]
            mhc._check(fn(m.handle, ptr(d_all), ptr(d_in_off), n, total, PREV0, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]), CHUNK, ptr(d_ws), wsb,
                          None), "encode")

        def decode_hist2():
            decode(False)
            mhc._check(lib.mh_dev_histogram_o2_batch(ptr(d_all), ptr(d_in_off), n, total, PREV0, ptr(d_counts), ptr(d_ws), wsb, None), "hist2")

        def hist_coded():
            mhc._check(lib.mh_dev_histogram_coded_batch_o2(m1.handle, 2, ptr(b1["payload"]), ptr(b1["pay_off"]), ptr(b1["nbits"]), n, b1["total"], PREV0,
                                                           ptr(d_in_off), total, ptr(b1["idx"]), CHUNK, ptr(d_counts), None, ptr(d_ws), wsb, None),
                       "histogram_coded_o2")

        def recode(src2):
            s, dm, b = (m2, m1, b2) if src2 else (m1, m2, b1)
            o = out["got"]
            mhc._check(lib.mh_dev_recode_batch_o2(s.handle, dm.handle, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n, b["total"], PREV0,
                                                  ptr(d_in_off), total, ptr(b["idx"]), CHUNK, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                                  ptr(d_drop), None, ptr(d_ws), wsb, None), "recode_o2")

        def same(what):
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, what)
            r, g = out["ref"], out["got"]
            k = int(r[1][-1].item())
            assert torch.equal(r[1], g[1]) and torch.equal(r[2], g[2]) and torch.equal(r[0][:k], g[0][:k]) and torch.equal(r[3], g[3]), (dname, what)
            assert int(d_drop.sum().item()) == 0, (dname, what)

        # every variant's result against the composition's, before the clock
        decode_hist2()
        assert lib.mh_dev_status(ptr(d_ws), None) == 0
        want_counts = d_counts.clone()
        assert np.array_equal(want_counts.cpu().numpy().view(np.uint64), c2)
        d_counts.zero_()
        hist_coded()
        assert lib.mh_dev_status(ptr(d_ws), None) == 0 and torch.equal(d_counts, want_counts), dname

        if once:
            ms = interleaved({"decode_o1_then_histogram_o2": decode_hist2, "histogram_coded_o2_from_o1": hist_coded}, 1)
        else:
            for src2 in (False, True):
                decode(src2)
                encode(not src2)
                for t in out["got"]:
                    t.zero_()
                recode(src2)
                same("recode src2=%s" % src2)
            pat = PATTERNS[dname]
            ps = mhc.PatternSet([pat])
            w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(msgs, [pat]), n)
            hit_total = int(w_off[-1])
            assert hit_total > 0
            d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_hits = torch.empty(3 * hit_total, dtype=torch.int64, device="cuda")
            d_pat = torch.empty(hit_total, dtype=torch.int32, device="cuda")

            def find(records, indexed):
                mhc._check(lib.mh_dev_find_batch_o2(m2.handle, ps.handle, ptr(b2["payload"]), ptr(b2["pay_off"]), ptr(b2["nbits"]), n, b2["total"], PREV0,
                                                    ptr(d_in_off) if indexed else None, total if indexed else 0, ptr(b2["idx"]) if indexed else None,
                                                    CHUNK, ptr(d_ho), ptr(d_hits) if records else None, ptr(d_pat) if records else None,
                                                    hit_total if records else 0, None, ptr(d_ws), wsb, None), "find_o2")

            for indexed in (True, False):
                for records in (False, True):
                    d_ho.zero_(); d_hits.zero_(); d_pat.zero_()
                    find(records, indexed)
                    assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, records, indexed)
                    assert np.array_equal(d_ho.cpu().numpy().view(np.uint64), w_off), (dname, records, indexed)
                    if records:
                        assert np.array_equal(d_hits.cpu().numpy().view(np.uint64).reshape(-1, 3), w_rec), (dname, indexed)
                        assert np.array_equal(d_pat.cpu().numpy().view(np.uint32), w_pat), (dname, indexed)
            decode(True)
            assert bytes(d_all[:per].cpu().numpy()) == msgs[0]
            fns = {"decode_o2_indexed": lambda: decode(True), "decode_o2_index_free": lambda: decode(True, False),
                   "decode_o1_then_encode_o2": lambda: (decode(False), encode(True)), "decode_o2_then_encode_o1": lambda: (decode(True), encode(False)),
                   "decode_o1_then_histogram_o2": decode_hist2,
                   "find_count_indexed": lambda: find(False, True), "find_records_indexed": lambda: find(True, True),
                   "find_count_index_free": lambda: find(False, False), "find_records_index_free": lambda: find(True, False),
                   "recode_o1_to_o2": lambda: recode(False), "recode_o2_to_o1": lambda: recode(True), "histogram_coded_o2_from_o1": hist_coded}
            ms = interleaved(fns, args.reps)
        o = {k: stats(v) for k, v in ms.items()}
        for k, base in YARDSTICK.items():
            if k in o and base in o:
                o[k]["ratio"] = round(o[k]["median_ms"] / o[base]["median_ms"], 3)
                o[k]["ratio_min_max"] = [round(o[k]["min_ms"] / o[base]["max_ms"], 3), round(o[k]["max_ms"] / o[base]["min_ms"], 3)]
        o["payload_bytes"] = {"order1": b1["total"], "order2": b2["total"] if b2 else None}
        o["workspace_bytes"] = {"find": int(lib.mh_dev_find_batch_o2_workspace(n, total, CHUNK)),
                                "recode": int(lib.mh_dev_recode_batch_o2_workspace(n, total, CHUNK)),
                                "histogram_coded": int(lib.mh_dev_histogram_coded_batch_o2_workspace(n, total, CHUNK)),
                                "histogram_counters": (1 << 24) * 8, "decoded_buffer": total}
        if not once:
            o["hits"] = hit_total
            o["count_only_search_within_decode"] = bool(o["find_count_indexed"]["ratio"] <= 1.0)
        res[dname] = o
        del b1, b2, d_all, d_ws, out, d_counts
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
