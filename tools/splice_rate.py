"""Rate of splicing re-coding (include/mh.h, "SPLICING BATCHES") against the masked re-code with the same spans and against
what a caller did before: decode the batch into a buffer, splice the buffer on the device, encode it again.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text input_wiki_cpp.txt
tiled), coded under a shared order-1 model with chunk 1024, indexed, HIP events, every variant run once per repetition in turn
(interleaved), medians with min and max.  The spans are those of a real search (mh_dev_find_batch of one two-byte pattern chosen
for about one hit per record, merged by mh_dev_spans_from_hits), as tools/edit_rate.py takes them:
  edit_spans            mh_dev_recode_edit_batch with the same spans, mask 0x2A: the parent's kernels, the yardstick of the kernels;
  splice_delete         mh_dev_recode_splice_batch, rep_len 0 (with the look-back pre-pass);
  splice_marker         mh_dev_recode_splice_batch, the 10 bytes `[REDACTED]`;
  decode_delete_encode, decode_marker_encode
                        mh_dev_decode_batch + one torch.index_select that gathers the spliced plaintext (the int32 gather index
                        and the new offsets are built outside the clock) + mh_dev_encode_batch: the yardstick of the feature.
The look-back pre-pass of a deletion cannot be launched alone through the C ABI; its time is in the kernel statistics of a
separate profiler run (profiles/splice/splice_kernel_stats.csv).  Every result is checked against the composition's output before
the clock.  Prints one JSON line; `ratio_edit` is a variant's median over the masked re-code's, `ratio_composition` over its
composition's.

    python tools/splice_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
from edit_rate import MASK, pattern_for  # noqa: E402
from recode_rate import CHUNK, PREV0, dev, interleaved, ptr, stats, zipf  # noqa: E402

REPS = {"delete": b"", "marker": b"[REDACTED]"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("splice_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "splice_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    maxr = max(len(r) for r in REPS.values())

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        src = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        dst = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs[::2]) + np.uint64(1), 1)     # another model that covers every pair
        payload, pay_off, nbits, idx, in_off = src.encode_batch(msgs, chunk_symbols=CHUNK)
        pay_total = int(pay_off[-1])
        d = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off),
                 idx=dev(idx))
        pat = pattern_for(data, per)
        ps = mhc.PatternSet([pat])
        fwsb = lib.mh_dev_find_batch_workspace(n, total, CHUNK)
        d_fws = torch.empty(fwsb, dtype=torch.uint8, device="cuda")
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")

        def find(d_rec, hit_cap):
            mhc._check(lib.mh_dev_find_batch(src.handle, ps.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                             ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_ho), ptr(d_rec), None, hit_cap, None, ptr(d_fws), fwsb,
                                             None), "find")
        find(None, 0)
        hit_cap = int(d_ho[-1].item())
        d_rec = torch.empty(max(hit_cap, 1) * 3, dtype=torch.int64, device="cuda")
        find(d_rec, hit_cap)
        swsb = lib.mh_dev_spans_from_hits_workspace(n, hit_cap)
        d_sws = torch.empty(swsb, dtype=torch.uint8, device="cuda")
        d_span_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_spans = torch.empty(max(hit_cap, 1) * 2, dtype=torch.int64, device="cuda")
        mhc._check(lib.mh_dev_spans_from_hits(ptr(d_ho), ptr(d_rec), hit_cap, n, ptr(d_span_off), ptr(d_spans), ptr(d_sws), swsb, None), "spans")
        assert lib.mh_dev_status(ptr(d_sws), None) == 0
        span_off = d_span_off.cpu().numpy().view(np.uint64).astype(np.int64)
        nspans = int(span_off[-1])
        spans = d_spans.cpu().numpy().view(np.uint64)[:2 * nspans].reshape(-1, 2).astype(np.int64)
        assert nspans and (spans[:, 1] <= per).all()                             # hits of a search: inside their messages
        stream_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(span_off))
        removed = np.bincount(stream_of, weights=spans[:, 1] - spans[:, 0], minlength=n).astype(np.int64)
        per_stream = np.diff(span_off)

        ototal_max = total + maxr * nspans
        cap = int(lib.mh_encode_batch_bound(dst.handle, ototal_max, n))
        nidx = int(lib.mh_batch_index_capacity(ototal_max, n, CHUNK))
        wsb = max(lib.mh_dev_recode_splice_workspace(n, total, CHUNK, nspans), lib.mh_dev_recode_edit_workspace(n, total, CHUNK),
                  lib.mh_dev_decode_batch_workspace(n), lib.mh_dev_encode_batch_workspace(n, ototal_max))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total + maxr, dtype=torch.uint8, device="cuda")      # the decoded bytes, the replacement behind them
        d_y = torch.empty(ototal_max, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(nidx, dtype=torch.int64, device="cuda")) for k in ("ref", "got")}
        d_drop = torch.empty(n, dtype=torch.int64, device="cuda")
        d_oso = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_mask = dev(np.full(256, MASK, dtype=np.uint8))
        d_reps = {k: dev(np.frombuffer(v + b"\0" * 16, dtype=np.uint8).copy()) for k, v in REPS.items()}

        # the composition's gather, built once per replacement on the device: source position p gives count[p] output bytes (a
        # kept byte 1, a span's begin rep_len, the rest of a span 0); an output byte of a replacement reads behind the decoded bytes
        g_begin = torch.from_numpy(stream_of * per + spans[:, 0]).cuda()
        g_end = torch.from_numpy(stream_of * per + spans[:, 1]).cuda()
        plan = {}
        for k, rep in REPS.items():
            R = len(rep)
            delta = torch.zeros(total + 1, dtype=torch.int32, device="cuda")
            delta.index_add_(0, g_begin, torch.ones(nspans, dtype=torch.int32, device="cuda"))
            delta.index_add_(0, g_end, -torch.ones(nspans, dtype=torch.int32, device="cuda"))
            count = (torch.cumsum(delta[:total], 0) == 0).to(torch.int32)
            del delta
            count[g_begin] = R
            srcpos = torch.repeat_interleave(torch.arange(total, dtype=torch.int32, device="cuda"), count)
            if R:
                start = torch.cumsum(count, 0, dtype=torch.int64) - count
                is_rep = torch.zeros(total, dtype=torch.bool, device="cuda")
                is_rep[g_begin] = True
                o = torch.arange(srcpos.numel(), dtype=torch.int64, device="cuda")
                sp64 = srcpos.to(torch.int64)
                within = (o - start[sp64]).to(torch.int32)
                srcpos = torch.where(is_rep[sp64], within + total, srcpos)
                del start, is_rep, o, sp64, within
            del count
            ylen = per - removed + R * per_stream
            yoff = np.concatenate([[0], np.cumsum(ylen)]).astype(np.uint64)
            assert srcpos.numel() == int(yoff[-1])
            plan[k] = (srcpos, dev(yoff), int(yoff[-1]))
            torch.cuda.empty_cache()

        def decode():
            d_so.copy_(d["in_off"])
            mhc._check(lib.mh_dev_decode_batch(src.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0, ptr(d_all),
                                               total, ptr(d_so), total, ptr(d["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def composition(k):
            srcpos, d_yoff, ytotal = plan[k]
            decode()
            d_all[total:total + len(REPS[k])] = d_reps[k][:len(REPS[k])]
            torch.index_select(d_all, 0, srcpos, out=d_y[:ytotal])
            o = out["ref"]
            mhc._check(lib.mh_dev_encode_batch(dst.handle, ptr(d_y), ptr(d_yoff), n, ytotal, PREV0, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                               CHUNK, ptr(d_ws), wsb, None), "encode")

        def splice(k):
            o = out["got"]
            mhc._check(lib.mh_dev_recode_splice_batch(src.handle, dst.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                                      ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_span_off), ptr(d_spans),
                                                      ptr(d_reps[k]) if REPS[k] else None, len(REPS[k]), ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(d_oso),
                                                      ptr(o[3]), nidx, ptr(d_drop), None, ptr(d_ws), wsb, None), "splice")

        def edit():
            o = out["got"]
            mhc._check(lib.mh_dev_recode_edit_batch(src.handle, dst.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                                    ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_span_off), ptr(d_spans), ptr(d_mask), ptr(o[0]),
                                                    cap, ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(d_drop), None, ptr(d_ws), wsb, None), "edit")

        # every splice against its composition, before the clock
        for k in REPS:
            for t in out["ref"] + out["got"]:
                t.zero_()
            composition(k)
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, k, "composition")
            splice(k)
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, k, "splice")
            r, g = out["ref"], out["got"]
            nb = int(r[1][-1].item())
            assert torch.equal(r[1], g[1]) and torch.equal(r[2], g[2]) and torch.equal(r[0][:nb], g[0][:nb]) and torch.equal(r[3], g[3]), (dname, k)
            assert torch.equal(d_oso, plan[k][1]), (dname, k, "out_sym_off")

        fns = {"edit_spans": edit}
        for k in REPS:
            fns["splice_" + k] = lambda k=k: splice(k)
            fns["decode_%s_encode" % k] = lambda k=k: composition(k)
        o = {k: stats(v) for k, v in interleaved(fns, args.reps).items()}
        for k in REPS:
            s = o["splice_" + k]
            s["ratio_edit"] = round(s["median_ms"] / o["edit_spans"]["median_ms"], 3)
            s["ratio_composition"] = round(s["median_ms"] / o["decode_%s_encode" % k]["median_ms"], 3)
        o["pattern"] = pat.hex()
        o["hits"], o["spans"] = hit_cap, nspans
        o["removed_bytes"] = int(removed.sum())
        o["workspace_bytes"] = {"splice": int(lib.mh_dev_recode_splice_workspace(n, total, CHUNK, nspans)),
                                "edit": int(lib.mh_dev_recode_edit_workspace(n, total, CHUNK)), "decoded_buffer": total}
        res[dname] = o
        del d, d_all, d_y, d_ws, out, plan
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
