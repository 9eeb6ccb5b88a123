"""Rate of masked re-coding (include/mh.h, "EDITING BATCHES") against the plain re-code and against what a caller did before:
decode the batch into a buffer, patch the buffer, encode it again.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text input_wiki_cpp.txt
tiled), coded under a shared order-1 model with chunk 1024, indexed, HIP events, every variant run once per repetition in turn
(interleaved), medians with min and max:
  recode              mh_dev_recode_batch on the same batch: the yardstick of the edit kernels;
  edit_spans          mh_dev_recode_edit_batch with the span list of a real search (mh_dev_find_batch of one two-byte pattern chosen
                      for about one hit per record, merged by mh_dev_spans_from_hits), mask 0x2A;
  edit_all            mh_dev_recode_edit_batch with d_span_off == NULL and a case-folding map;
  spans_from_hits     mh_dev_spans_from_hits alone;
  decode_mask_encode  mh_dev_decode_batch + a torch masked assignment on the decoded buffer + mh_dev_encode_batch: the yardstick of
                      the feature (the mask tensor is built outside the clock).
Every result is checked against the composition's output before the clock; the spans against tests/edit_ref.py.  Prints one JSON
line; `ratio_recode` is a variant's median over the plain re-code's, `ratio_composition` over the composition's.

    python tools/edit_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
import edit_ref  # noqa: E402
from recode_rate import CHUNK, PREV0, dev, interleaved, ptr, stats, zipf  # noqa: E402

MASK = 0x2A
FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def pattern_for(data, per):
    """The two-byte string whose count in the first 16 MiB is nearest to one per record."""
    s = data[:1 << 24].astype(np.uint32)
    pairs = np.bincount((s[:-1] << 8) | s[1:], minlength=65536)
    p = int(np.argmin(np.abs(pairs.astype(np.int64) - s.size // per)))
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
        raise SystemExit("edit_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "edit_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        counts = mhc.histogram_o1_batch(msgs)
        src = mhc.Model.from_counts(counts, 1)
        dst = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs[::2]) + np.uint64(1), 1)     # another model that covers every pair
        payload, pay_off, nbits, idx, in_off = src.encode_batch(msgs, chunk_symbols=CHUNK)
        pay_total = int(pay_off[-1])
        d = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off),
                 idx=dev(idx))
        cap = int(lib.mh_encode_batch_bound(dst.handle, total, n))
        nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
        pat = pattern_for(data, per)
        ps = mhc.PatternSet([pat])
        fwsb = lib.mh_dev_find_batch_workspace(n, total, CHUNK)
        wsb = max(lib.mh_dev_recode_edit_workspace(n, total, CHUNK), lib.mh_dev_recode_batch_workspace(n, total, CHUNK),
                  lib.mh_dev_decode_batch_workspace(n), lib.mh_dev_encode_batch_workspace(n, total), fwsb)
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(nidx, dtype=torch.int64, device="cuda")) for k in ("ref", "got")}
        d_drop = torch.empty(n, dtype=torch.int64, device="cuda")

        # the search, outside the clock: count, then the records
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")

        def find(d_rec, hit_cap):
            mhc._check(lib.mh_dev_find_batch(src.handle, ps.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                             ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_ho), ptr(d_rec), None, hit_cap, None, ptr(d_ws), wsb,
                                             None), "find")
        find(None, 0)
        hit_cap = int(d_ho[-1].item())
        d_rec = torch.empty(max(hit_cap, 1) * 3, dtype=torch.int64, device="cuda")
        find(d_rec, hit_cap)
        swsb = lib.mh_dev_spans_from_hits_workspace(n, hit_cap)
        d_sws = torch.empty(swsb, dtype=torch.uint8, device="cuda")
        d_span_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_spans = torch.empty(max(hit_cap, 1) * 2, dtype=torch.int64, device="cuda")

        def spans_from_hits():
            mhc._check(lib.mh_dev_spans_from_hits(ptr(d_ho), ptr(d_rec), hit_cap, n, ptr(d_span_off), ptr(d_spans), ptr(d_sws), swsb, None), "spans")
        spans_from_hits()
        assert lib.mh_dev_status(ptr(d_sws), None) == 0
        span_off = d_span_off.cpu().numpy().view(np.uint64)
        nspans = int(span_off[-1])
        spans = d_spans.cpu().numpy().view(np.uint64)[:2 * nspans].reshape(-1, 2)
        r_so, r_sp = edit_ref.merge_hits(d_ho.cpu().numpy().view(np.uint64), d_rec.cpu().numpy().view(np.uint64)[:3 * hit_cap].reshape(-1, 3))
        assert np.array_equal(span_off, r_so) and np.array_equal(spans, r_sp), dname
        # the composition's patch: a mask over the decoded buffer, built once
        stream_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(span_off.astype(np.int64)))
        delta = np.zeros(total + 1, dtype=np.int8)
        np.add.at(delta, stream_of * per + spans[:, 0].astype(np.int64), 1)
        np.add.at(delta, stream_of * per + spans[:, 1].astype(np.int64), -1)
        d_mask = dev(np.cumsum(delta[:total], dtype=np.int8) > 0)
        d_fold = dev(np.frombuffer(FOLD, dtype=np.uint8))
        d_maps = {"mask": dev(np.full(256, MASK, dtype=np.uint8)), "fold": d_fold}

        def decode():
            d_so.copy_(d["in_off"])
            mhc._check(lib.mh_dev_decode_batch(src.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0, ptr(d_all),
                                               total, ptr(d_so), total, ptr(d["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def encode():
            o = out["ref"]
            mhc._check(lib.mh_dev_encode_batch(dst.handle, ptr(d_all), ptr(d["in_off"]), n, total, PREV0, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                               CHUNK, ptr(d_ws), wsb, None), "encode")

        def decode_mask_encode():
            decode()
            d_all.masked_fill_(d_mask, MASK)
            encode()

        def decode_fold_encode():
            decode()
            d_all.copy_(torch.index_select(d_fold, 0, d_all.to(torch.int32)))
            encode()

        def decode_encode():
            decode()
            encode()

        def recode():
            o = out["got"]
            mhc._check(lib.mh_dev_recode_batch(src.handle, dst.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                               ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(d_drop),
                                               None, ptr(d_ws), wsb, None), "recode")

        def edit(which):
            o = out["got"]
            lists = (ptr(d_span_off), ptr(d_spans)) if which == "mask" else (None, None)
            mhc._check(lib.mh_dev_recode_edit_batch(src.handle, dst.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                                    ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, *lists, ptr(d_maps[which]), ptr(o[0]), cap, ptr(o[1]),
                                                    ptr(o[2]), ptr(o[3]), ptr(d_drop), None, ptr(d_ws), wsb, None), "edit")

        def same(what):
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, what)
            r, g = out["ref"], out["got"]
            k = int(r[1][-1].item())
            assert torch.equal(r[1], g[1]) and torch.equal(r[2], g[2]) and torch.equal(r[0][:k], g[0][:k]) and torch.equal(r[3], g[3]), (dname, what)

        # every variant's result against the composition's, before the clock
        for ref, got, what in ((decode_encode, recode, "recode"), (decode_mask_encode, lambda: edit("mask"), "edit_spans"),
                               (decode_fold_encode, lambda: edit("fold"), "edit_all")):
            ref()
            for t in out["got"]:
                t.zero_()
            got()
            same(what)

        fns = {"recode": recode, "edit_spans": lambda: edit("mask"), "edit_all": lambda: edit("fold"), "spans_from_hits": spans_from_hits,
               "decode_mask_encode": decode_mask_encode}
        o = {k: stats(v) for k, v in interleaved(fns, args.reps).items()}
        for k in ("edit_spans", "edit_all"):
            o[k]["ratio_recode"] = round(o[k]["median_ms"] / o["recode"]["median_ms"], 3)
            o[k]["ratio_composition"] = round(o[k]["median_ms"] / o["decode_mask_encode"]["median_ms"], 3)
        o["recode"]["spread_ms"] = round(o["recode"]["max_ms"] - o["recode"]["min_ms"], 4)
        o["pattern"] = pat.hex()
        o["hits"], o["spans"] = hit_cap, nspans
        o["masked_bytes"] = int((spans[:, 1] - spans[:, 0]).sum())
        o["workspace_bytes"] = {"edit": int(lib.mh_dev_recode_edit_workspace(n, total, CHUNK)), "spans_from_hits": int(swsb), "find": int(fwsb),
                                "decoded_buffer": total}
        res[dname] = o
        del d, d_all, d_ws, out, d_mask
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
