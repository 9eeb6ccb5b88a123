"""Rate of the masked re-code and the table splice with an order-2 model on a side (include/mh.h, "ORDER 2 IN EDITING AND
SPLICING") against the plain order-2 re-code and against what a caller did before: decode the batch into a buffer, patch the
buffer, encode it again.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text input_wiki_cpp.txt
tiled), chunk 1024, indexed, HIP events, every variant run once per repetition in turn (interleaved), medians with min and max.
The destination is an order-2 model of every other message; the sources are an order-2 and an order-1 model of the batch:
  recode22, recode12    mh_dev_recode_batch_o2 on the same batches: the yardstick of the kernels;
  edit22, edit12        mh_dev_recode_edit_batch_o2 with the span list of a real search (mh_dev_find_batch_o2 of one two-byte
                        pattern chosen for about one hit per record, merged by mh_dev_spans_from_hits), mask 0x2A;
  compose22, compose12  mh_dev_decode_batch_o2 / mh_dev_decode_batch + a torch masked assignment on the decoded buffer +
                        mh_dev_encode_batch_o2: the yardstick of the feature (the mask tensor is built outside the clock);
  splice22              mh_dev_recode_splice_table_batch_o2, three tagged spans per record over a four-entry table (lengths 0, 1,
                        2 and 12; the spans lie across the chunk boundaries at 1024 and 2048 and inside the third chunk);
  compose_splice22      its composition: decode + one torch gather through an index built outside the clock + encode.
Every variant's output is compared with its composition's before the clock.  Prints one JSON line; `ratio_recode` is a variant's
median over the plain re-code's of the same orders, `ratio_composition` over its composition's.

    python tools/edit_o2_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
from edit_rate import MASK, pattern_for  # noqa: E402
from recode_rate import CHUNK, PREV0, dev, interleaved, ptr, stats, zipf  # noqa: E402

REPS = [b"", b"#", b"<>", b"[[REDACTED]]"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("edit_o2_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "edit_o2_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    # the table splice: the same three spans in every record, tags 1, 0, 3 (one byte, deleted, twelve bytes)
    cuts = [(CHUNK - 3, CHUNK + 5, 1), (2 * CHUNK - 9, 2 * CHUNK, 0), (2 * CHUNK + 700, 2 * CHUNK + 707, 3)]
    assert per > cuts[-1][1]
    rep_off = np.concatenate([[0], np.cumsum([len(r) for r in REPS])]).astype(np.uint64)
    rep_bytes = np.frombuffer(b"".join(REPS), dtype=np.uint8)

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        src = {2: mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2), 1: mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)}
        # another order-2 model: every other message, and 4 096 of them with a run of the mask byte (a triple without a code is
        # dropped by the calls and by the composition's encoder alike; the count is reported)
        train = msgs[::2]
        marked = [m[:CHUNK - 3] + b"*" * 8 + m[CHUNK + 5:] for m in train[:4096]]
        dst = mhc.Model.from_counts(mhc.histogram_o2_batch(train) + mhc.histogram_o2_batch(marked), 2)
        coded = {2: src[2].encode_batch_o2(msgs, chunk_symbols=CHUNK), 1: src[1].encode_batch(msgs, chunk_symbols=CHUNK)}
        d = {o: dict(payload=dev(np.concatenate([c[0], np.zeros(64, dtype=np.uint8)])), pay_off=dev(c[1]), nbits=dev(c[2]), idx=dev(c[3]), in_off=dev(c[4]),
                     pay_total=int(c[1][-1])) for o, c in coded.items()}
        out_total = total + n * sum(len(REPS[t]) - (e - b) for b, e, t in cuts)
        cap = int(lib.mh_encode_batch_bound(dst.handle, max(total, out_total), n))
        nidx = int(lib.mh_batch_index_capacity(max(total, out_total), n, CHUNK))
        nspl = 3 * n
        ws_edit = int(lib.mh_dev_recode_edit_batch_o2_workspace(n, total, CHUNK))
        ws_splice = int(lib.mh_dev_recode_splice_table_batch_o2_workspace(n, total, CHUNK, nspl, len(REPS)))
        fwsb = int(lib.mh_dev_find_batch_o2_workspace(n, total, CHUNK))
        wsb = max(ws_edit, ws_splice, fwsb, lib.mh_dev_recode_batch_o2_workspace(n, total, CHUNK), lib.mh_dev_decode_batch_workspace(n),
                  lib.mh_dev_decode_batch_o2_workspace(n), lib.mh_dev_encode_batch_o2_workspace(n, max(total, out_total)))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(cap + 64, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(nidx, dtype=torch.int64, device="cuda")) for k in ("ref", "got")}
        d_drop = torch.empty(n, dtype=torch.int64, device="cuda")
        d_oso = torch.empty(n + 1, dtype=torch.int64, device="cuda")

        # the search in the order-2 batch, outside the clock: count, then the records, merged into spans
        pat = pattern_for(data, per)
        ps = mhc.PatternSet([pat])
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        s2 = d[2]

        def find(d_rec, hit_cap):
            mhc._check(lib.mh_dev_find_batch_o2(src[2].handle, ps.handle, ptr(s2["payload"]), ptr(s2["pay_off"]), ptr(s2["nbits"]), n, s2["pay_total"],
                                                PREV0, ptr(s2["in_off"]), total, ptr(s2["idx"]), CHUNK, ptr(d_ho), ptr(d_rec), None, hit_cap, None,
                                                ptr(d_ws), wsb, None), "find")
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
        span_off = d_span_off.cpu().numpy().view(np.uint64)
        nspans = int(span_off[-1])
        spans = d_spans.cpu().numpy().view(np.uint64)[:2 * nspans].reshape(-1, 2)
        r_so, r_sp = edit_ref.merge_hits(d_ho.cpu().numpy().view(np.uint64), d_rec.cpu().numpy().view(np.uint64)[:3 * hit_cap].reshape(-1, 3))
        assert np.array_equal(span_off, r_so) and np.array_equal(spans, r_sp), dname
        stream_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(span_off.astype(np.int64)))
        delta = np.zeros(total + 1, dtype=np.int8)
        np.add.at(delta, stream_of * per + spans[:, 0].astype(np.int64), 1)
        np.add.at(delta, stream_of * per + spans[:, 1].astype(np.int64), -1)
        d_mask = dev(np.cumsum(delta[:total], dtype=np.int8) > 0)
        d_map = dev(np.full(256, MASK, dtype=np.uint8))
        # the table splice's lists and the composition's gather: positions in [decoded bytes | table bytes]
        d_tso = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(3))
        d_tsp = dev(np.tile(np.array([(b, e) for b, e, _ in cuts], dtype=np.uint64).reshape(-1), n))
        d_ttg = dev(np.tile(np.array([t for _, _, t in cuts], dtype=np.uint32), n))
        d_roff, d_rb = dev(rep_off), dev(np.concatenate([rep_bytes, np.zeros(16, dtype=np.uint8)]))
        one, at = [], 0
        for b, e, t in cuts:
            one += [np.arange(at, b), -1 - np.arange(int(rep_off[t]), int(rep_off[t + 1]))]     # (negative: a byte of the table)
            at = e
        one = np.concatenate(one + [np.arange(at, per)]).astype(np.int64)
        assert one.size * n == out_total
        g = one[None, :] + (np.arange(n, dtype=np.int64) * per)[:, None]
        g = np.where(one[None, :] < 0, total + (-1 - one)[None, :], g).reshape(-1).astype(np.int32)
        d_gather = dev(g)
        d_spliced = torch.empty(out_total, dtype=torch.uint8, device="cuda")
        d_out_in = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(one.size))
        d_cat = torch.empty(total + rep_bytes.size, dtype=torch.uint8, device="cuda")
        d_cat[total:] = d_rb[:rep_bytes.size]

        def decode(o):
            s = d[o]
            d_so.copy_(s["in_off"])
            fn = lib.mh_dev_decode_batch_o2 if o == 2 else lib.mh_dev_decode_batch
            mhc._check(fn(src[o].handle, ptr(s["payload"]), ptr(s["pay_off"]), ptr(s["nbits"]), n, s["pay_total"], PREV0, ptr(d_all), total, ptr(d_so),
                          total, ptr(s["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def encode(d_data, d_in, size):
            r = out["ref"]
            mhc._check(lib.mh_dev_encode_batch_o2(dst.handle, ptr(d_data), ptr(d_in), n, size, PREV0, ptr(r[0]), cap, ptr(r[1]), ptr(r[2]), ptr(r[3]),
                                                  CHUNK, ptr(d_ws), wsb, None), "encode")

        def compose(o, mask):
            decode(o)
            if mask:
                d_all.masked_fill_(d_mask, MASK)
            encode(d_all, d[o]["in_off"], total)

        def compose_splice():
            decode(2)
            d_cat[:total] = d_all
            torch.index_select(d_cat, 0, d_gather, out=d_spliced)
            encode(d_spliced, d_out_in, out_total)

        def batch_args(o):
            s = d[o]
            return (src[o].handle, dst.handle, ptr(s["payload"]), ptr(s["pay_off"]), ptr(s["nbits"]), n, s["pay_total"], PREV0, ptr(s["in_off"]), total,
                    ptr(s["idx"]), CHUNK)

        def recode(o):
            r = out["got"]
            mhc._check(lib.mh_dev_recode_batch_o2(*batch_args(o), ptr(r[0]), cap, ptr(r[1]), ptr(r[2]), ptr(r[3]), ptr(d_drop), None, ptr(d_ws), wsb, None),
                       "recode")

        def edit(o):
            r = out["got"]
            blk = mhc.args_block(mhc.RecodeEditO2Args, *batch_args(o), ptr(d_span_off), ptr(d_spans), ptr(d_map), ptr(r[0]), cap, ptr(r[1]), ptr(r[2]),
                                 ptr(r[3]), ptr(d_drop), None, ptr(d_ws), wsb, None)
            mhc._check(lib.mh_dev_recode_edit_batch_o2(C.byref(blk)), "edit")

        def splice():
            r = out["got"]
            blk = mhc.args_block(mhc.RecodeSpliceO2Args, *batch_args(2), ptr(d_tso), ptr(d_tsp), ptr(d_ttg), ptr(d_roff), ptr(d_rb), len(REPS), ptr(r[0]),
                                 cap, ptr(r[1]), ptr(r[2]), ptr(d_oso), ptr(r[3]), nidx, ptr(d_drop), None, ptr(d_ws), wsb, None)
            mhc._check(lib.mh_dev_recode_splice_table_batch_o2(C.byref(blk)), "splice")

        def same(what):
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, what)
            r, got = out["ref"], out["got"]
            k = int(r[1][-1].item())
            assert torch.equal(r[1], got[1]) and torch.equal(r[2], got[2]) and torch.equal(r[0][:k], got[0][:k]) and torch.equal(r[3], got[3]), (dname, what)
            drops[what] = int(d_drop.sum().item())

        # every variant's result against the composition's, before the clock
        drops = {}
        for ref, got, what in ((lambda: compose(2, False), lambda: recode(2), "recode22"), (lambda: compose(1, False), lambda: recode(1), "recode12"),
                               (lambda: compose(2, True), lambda: edit(2), "edit22"), (lambda: compose(1, True), lambda: edit(1), "edit12"),
                               (compose_splice, splice, "splice22")):
            for t in out["ref"] + out["got"]:
                t.zero_()
            ref()
            got()
            same(what)
        assert torch.equal(d_oso, d_out_in), dname

        fns = {"recode22": lambda: recode(2), "recode12": lambda: recode(1), "edit22": lambda: edit(2), "edit12": lambda: edit(1),
               "compose22": lambda: compose(2, True), "compose12": lambda: compose(1, True), "splice22": splice, "compose_splice22": compose_splice}
        o = {k: stats(v) for k, v in interleaved(fns, args.reps).items()}
        for k in ("edit22", "edit12"):
            o[k]["ratio_recode"] = round(o[k]["median_ms"] / o["recode" + k[4:]]["median_ms"], 3)
            o[k]["ratio_composition"] = round(o[k]["median_ms"] / o["compose" + k[4:]]["median_ms"], 3)
        o["splice22"]["ratio_recode"] = round(o["splice22"]["median_ms"] / o["recode22"]["median_ms"], 3)
        o["splice22"]["ratio_composition"] = round(o["splice22"]["median_ms"] / o["compose_splice22"]["median_ms"], 3)
        o["pattern"] = pat.hex()
        o["hits"], o["spans"], o["splice_spans"] = hit_cap, nspans, nspl
        o["dropped"] = drops
        o["masked_bytes"] = int((spans[:, 1] - spans[:, 0]).sum())
        o["coded_bytes"] = {"order2": d[2]["pay_total"], "order1": d[1]["pay_total"]}
        o["workspace_bytes"] = {"edit_o2": ws_edit, "splice_table_o2": ws_splice, "find_o2": fwsb, "decoded_buffer": total, "gather_index": int(g.nbytes)}
        res[dname] = o
        del d, d_all, d_ws, out, d_mask, d_gather, d_spliced, d_cat
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
