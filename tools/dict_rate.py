"""Dictionary search rate in compressed batches (include/mh.h, "DICTIONARY SEARCH IN BATCHES") against the decode of the same
batch and against the Shift-And passes a dictionary replaces.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), coded under a shared order-1 model with chunk 1024, indexed, HIP events, every variant run once
per repetition in turn (interleaved), medians with min and max of 7:
  1. mh_dev_decode_batch: the yardstick, measured beside the search;
  2. one mh_dev_find_batch pass with one pattern: a dictionary of P pattern bytes replaces ceil(P / 64) such passes;
  3. mh_dev_find_dict_batch, count-only and with records, for dictionaries of 16, 1 024 and 3 664 patterns (the identifiers of
     four or more letters of input_wiki_cpp.html, in a fixed shuffled order, so the smaller sets are prefixes of the larger);
  4. the same under a model set (mh_dev_find_dict_each);
  5. with --lib-b PATH (a library built by `make -C markov-huffman-coding_amd/csrc exp TAG=nohot
     EXPFLAGS=-DMH_EXP_DICT_NO_HOT_ROWS`): the count-only variants of 3 again through that library, in the same interleaved
     loop: the A/B of the transition rows kept in LDS.
Before the clock every variant's result is checked: hit_off and the records of the first --check-streams streams against
tests/find_ref.py, exactly (find_ref on all 256 MiB with 3 664 patterns is hours of bytes.find), and every stream's count
against the host matcher mh_dict_find_bytes, which tests/test_dict_abi.py pins to find_ref.
Prints one JSON line: `ratio` is a variant's median over the decode's, `vs_shift_and` its median over ceil(P / 64) single
passes, `break_even` the smallest measured dictionary at which one DFA pass beats the passes it replaces.

    python tools/dict_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--check-streams 1024] [--lib-b PATH] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
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
from find_rate import dev, interleaved, ptr, stats, zipf  # noqa: E402

CHUNK = 1024
PREV0 = 0x20
SIZES = (16, 1024, 3664)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check-streams", type=int, default=1024)
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("dict_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    lib_b = None
    if args.lib_b:
        lib_b = C.CDLL(os.path.abspath(args.lib_b))
        lib_b.mh_dev_find_dict_batch.argtypes = lib.mh_dev_find_dict_batch.argtypes
    n, per = args.streams, args.bytes
    total, nchk = n * per, min(args.check_streams, n)
    golden = os.path.join(ROOT, "tests", "golden", "inputs")
    html = open(os.path.join(golden, "input_wiki_cpp.html"), "rb").read()
    tokens = sorted(set(re.findall(rb"[A-Za-z_]{4,}", html)))
    assert len(tokens) == SIZES[-1]
    order = np.random.default_rng(11).permutation(len(tokens))
    tokens = [tokens[i] for i in order]
    single = b"template"
    text = np.frombuffer(open(os.path.join(golden, "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "dict_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "check_streams": nchk,
           "device": torch.cuda.get_device_name(0), "lib_b": os.path.basename(args.lib_b) if args.lib_b else None}

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        dicts = {p: mhc.Dict(tokens[:p]) for p in SIZES}
        ps1 = mhc.PatternSet([single])
        want, counts = {}, {}
        for p, dc in dicts.items():
            t0 = time.perf_counter()
            want[p] = find_ref.hit_arrays(find_ref.find_hits(msgs[:nchk], tokens[:p]), nchk)
            t1 = time.perf_counter()
            c = np.zeros(n + 1, dtype=np.uint64)
            tot = C.c_uint64(0)
            for i, m in enumerate(msgs):
                lib.mh_dict_find_bytes(dc.handle, m, len(m), None, None, 0, C.byref(tot))
                c[i + 1] = tot.value
            counts[p] = np.cumsum(c, dtype=np.uint64)
            assert np.array_equal(counts[p][:nchk + 1], want[p][0])
            print("[dict_rate] %s %d patterns: %d hits (%d in the %d checked streams; find_ref %.1f s, host matcher %.1f s)"
                  % (dname, p, int(counts[p][-1]), want[p][1].shape[0], nchk, t1 - t0, time.perf_counter() - t1), file=sys.stderr)
        want1 = find_ref.hit_arrays(find_ref.find_hits(msgs, [single]), n)

        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        payload, pay_off, nbits, idx, in_off = model.encode_batch(msgs, chunk_symbols=CHUNK)
        ms_set = mhc.ModelSet.train(msgs, order=1)
        e_payload, e_pay_off, e_nbits, e_idx, e_in_off, rc = ms_set.encode(msgs, chunk_symbols=CHUNK)
        assert rc == mhc.MH_OK
        pay_total = int(pay_off[-1])
        pad = np.zeros(64, dtype=np.uint8)
        d = dict(payload=dev(np.concatenate([payload, pad])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off), idx=dev(idx))
        e = dict(payload=dev(np.concatenate([e_payload, pad])), pay_off=dev(e_pay_off), nbits=dev(e_nbits), in_off=dev(e_in_off), idx=dev(e_idx))
        wsb = max(lib.mh_dev_find_dict_workspace(n, total, CHUNK), lib.mh_dev_decode_batch_workspace(n))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        cap = max(int(max(c[-1] for c in counts.values())), want1[1].shape[0], 1)
        d_hits = torch.empty(cap * 3, dtype=torch.int64, device="cuda")
        d_pat = torch.empty(cap, dtype=torch.int32, device="cuda")

        def decode():
            d_so.copy_(d["in_off"])
            mhc._check(lib.mh_dev_decode_batch(model.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0, ptr(d_all),
                                               total, ptr(d_so), total, ptr(d["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def find(fn, h, what, b, b_total, records):
            mhc._check(fn(h, what, ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), n, b_total, PREV0, ptr(b["in_off"]), total, ptr(b["idx"]),
                          CHUNK, ptr(d_ho), ptr(d_hits) if records else None, ptr(d_pat) if records else None, cap, None, ptr(d_ws), wsb, None), "find")

        def shift_and(records=False):
            find(lib.mh_dev_find_batch, model.handle, ps1.handle, d, pay_total, records)

        def dict_find(p, records, each=False, l=lib):
            if each:
                find(l.mh_dev_find_dict_each, ms_set.handle, dicts[p].handle, e, int(e_pay_off[-1]), records)
            else:
                find(l.mh_dev_find_dict_batch, model.handle, dicts[p].handle, d, pay_total, records)

        def verify(p, records, **kw):
            d_ho.zero_(); d_hits.zero_(); d_pat.zero_()
            dict_find(p, records, **kw)
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, p, records, kw)
            assert np.array_equal(d_ho.cpu().numpy().view(np.uint64), counts[p]), (dname, p, records, kw)
            if records:
                off, rec, pat = want[p]
                k = rec.shape[0]
                assert np.array_equal(d_hits[:3 * k].cpu().numpy().view(np.uint64).reshape(-1, 3), rec), (dname, p, kw)
                assert np.array_equal(d_pat[:k].cpu().numpy().view(np.uint32), pat), (dname, p, kw)

        fns = {"decode_indexed": decode, "shift_and_1_pattern_count": shift_and, "shift_and_1_pattern_records": lambda: shift_and(True)}
        for p in SIZES:
            fns["dict_%d_count" % p] = lambda p=p: dict_find(p, False)
            fns["dict_%d_records" % p] = lambda p=p: dict_find(p, True)
            fns["each_dict_%d_count" % p] = lambda p=p: dict_find(p, False, each=True)
            fns["each_dict_%d_records" % p] = lambda p=p: dict_find(p, True, each=True)
            if lib_b is not None:
                fns["dict_%d_count_lib_b" % p] = lambda p=p: dict_find(p, False, l=lib_b)
        for p in SIZES:                                                  # every variant's result against the reference, before the clock
            for records in (False, True):
                verify(p, records)
                verify(p, records, each=True)
            if lib_b is not None:
                verify(p, False, l=lib_b)
        d_ho.zero_()
        shift_and(True)
        k = want1[1].shape[0]
        assert np.array_equal(d_ho.cpu().numpy().view(np.uint64), want1[0])
        assert np.array_equal(d_hits[:3 * k].cpu().numpy().view(np.uint64).reshape(-1, 3), want1[1])
        decode()
        assert torch.equal(d_all, dev(data))
        ms = interleaved(fns, args.reps)
        out = {k: stats(v) for k, v in ms.items()}
        base = out["decode_indexed"]["median_ms"]
        one = out["shift_and_1_pattern_count"]["median_ms"]
        for k in out:
            out[k]["ratio"] = round(out[k]["median_ms"] / base, 3)
        out["break_even"] = None
        for p in SIZES:
            passes = -(-sum(len(t) for t in tokens[:p]) // mhc.FIND_MAX_POSITIONS)
            v = out["dict_%d_count" % p]
            v["pattern_bytes"], v["shift_and_passes"] = sum(len(t) for t in tokens[:p]), passes
            v["vs_shift_and"] = round(v["median_ms"] / (passes * one), 4)
            if out["break_even"] is None and v["median_ms"] < passes * one:
                out["break_even"] = p
            if lib_b is not None:
                a, b = v, out["dict_%d_count_lib_b" % p]
                spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
                b["lib_b_minus_lib_ms"], b["spread_ms"] = round(b["median_ms"] - a["median_ms"], 4), round(spread, 4)
                b["lib_faster_by_more_than_the_spread"] = bool(b["median_ms"] - a["median_ms"] > spread)
        out["hits"] = {str(p): int(counts[p][-1]) for p in SIZES}
        out["dict"] = {str(p): {"states": dicts[p].states, "classes": dicts[p].classes, "device_bytes": dicts[p].device_bytes} for p in SIZES}
        out["payload_bytes"] = pay_total
        res[dname] = out
        del d, e, d_all, d_hits, d_pat, d_ws
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
