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

The table splice (include/mh.h, "SPLICING WITH A REPLACEMENT TABLE"; --no-table leaves these out), same batches, same method:
  table_one_delete, table_one_marker
                        mh_dev_recode_splice_table_batch on the same spans, every tag 0 and a one-entry table, interleaved with
                        splice_delete / splice_marker (`ratio_splice`: over that call's median); its look-back pre-pass always runs;
  spans_untagged, spans_tagged
                        mh_dev_spans_from_hits against mh_dev_spans_from_hits_tagged on the records of a dictionary search
                        (mh_dev_find_dict_batch) of four patterns, two of which overlap in the text (`ratio_untagged`);
  table_mixed           the table splice on those tagged spans with the table `<A>`, empty, `[REDACTED]`, `#`;
  decode_mixed_encode   its composition: decode + gather + encode, the gather index built outside the clock (`ratio_composition`).

    python tools/splice_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE] [--no-table]
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
MIXED = [b"<A>", b"", b"[REDACTED]", b"#"]         # the table of table_mixed, one entry per pattern of patterns_for


def patterns_for(data, per):
    """Four patterns for the dictionary search: the three two-byte strings whose counts in the first 16 MiB are nearest to one
    per record, and in front of them (the highest priority) the first of these with its most frequent follower, which overlaps
    every one of its hits."""
    s = data[:1 << 24].astype(np.uint32)
    pairs = np.bincount((s[:-1] << 8) | s[1:], minlength=65536)
    near = np.argsort(np.abs(pairs.astype(np.int64) - s.size // per), kind="stable")[:3]
    two = [bytes([int(p) >> 8, int(p) & 255]) for p in near]
    at = np.flatnonzero(((s[:-2] << 8) | s[1:-1]) == int(near[0]))
    follower = int(np.bincount(s[at + 2].astype(np.int64), minlength=256).argmax())
    return [two[0] + bytes([follower])] + two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-table", action="store_true", help="the single-replacement variants alone")
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("splice_rate.py needs a GPU (and torch for the event timing)")
    table = not args.no_table
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

        # the table splice's spans: a dictionary search of four patterns with their pattern numbers, merged with tags
        mixed = None
        if table:
            pats = patterns_for(data, per)
            dc = mhc.Dict(pats)
            dwsb = lib.mh_dev_find_dict_workspace(n, total, CHUNK)
            d_dws = torch.empty(dwsb, dtype=torch.uint8, device="cuda")
            d_ho2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")

            def find_dict(d_rec, d_pat, hit_cap):
                mhc._check(lib.mh_dev_find_dict_batch(src.handle, dc.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total, PREV0,
                                                      ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_ho2), ptr(d_rec), ptr(d_pat), hit_cap, None,
                                                      ptr(d_dws), dwsb, None), "find_dict")
            find_dict(None, None, 0)
            hit_cap2 = int(d_ho2[-1].item())
            d_rec2 = torch.empty(max(hit_cap2, 1) * 3, dtype=torch.int64, device="cuda")
            d_pat2 = torch.empty(max(hit_cap2, 1), dtype=torch.int32, device="cuda")
            find_dict(d_rec2, d_pat2, hit_cap2)
            del d_dws
            swsb2 = max(lib.mh_dev_spans_from_hits_workspace(n, hit_cap2), lib.mh_dev_spans_from_hits_tagged_workspace(n, hit_cap2))
            d_sws2 = torch.empty(swsb2, dtype=torch.uint8, device="cuda")
            d_span_off2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_spans2 = torch.empty(max(hit_cap2, 1) * 2, dtype=torch.int64, device="cuda")
            d_tags2 = torch.empty(max(hit_cap2, 1), dtype=torch.int32, device="cuda")
            d_span_off_u = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_spans_u = torch.empty(max(hit_cap2, 1) * 2, dtype=torch.int64, device="cuda")

            def spans_untagged():
                mhc._check(lib.mh_dev_spans_from_hits(ptr(d_ho2), ptr(d_rec2), hit_cap2, n, ptr(d_span_off_u), ptr(d_spans_u), ptr(d_sws2), swsb2, None),
                           "spans")

            def spans_tagged():
                mhc._check(lib.mh_dev_spans_from_hits_tagged(ptr(d_ho2), ptr(d_rec2), ptr(d_pat2), hit_cap2, n, ptr(d_span_off2), ptr(d_spans2),
                                                             ptr(d_tags2), ptr(d_sws2), swsb2, None), "spans_tagged")
            spans_untagged()
            assert lib.mh_dev_status(ptr(d_sws2), None) == 0
            spans_tagged()
            assert lib.mh_dev_status(ptr(d_sws2), None) == 0
            span_off2 = d_span_off2.cpu().numpy().view(np.uint64).astype(np.int64)
            nspans2 = int(span_off2[-1])
            assert torch.equal(d_span_off2, d_span_off_u) and torch.equal(d_spans2[:2 * nspans2], d_spans_u[:2 * nspans2]), (dname, "tagged spans")
            spans2 = d_spans2.cpu().numpy().view(np.uint64)[:2 * nspans2].reshape(-1, 2).astype(np.int64)
            tags2 = d_tags2.cpu().numpy().view(np.uint32)[:nspans2].astype(np.int64)
            # the tags against the host form on the same records
            h = mhc.spans_from_hits_tagged(d_ho2.cpu().numpy().view(np.uint64), d_rec2.cpu().numpy().view(np.uint64)[:3 * hit_cap2],
                                           d_pat2.cpu().numpy().view(np.uint32)[:hit_cap2])
            assert h[3] == 0 and np.array_equal(h[1].astype(np.int64), spans2) and np.array_equal(h[2].astype(np.int64), tags2), (dname, "tags")
            assert nspans2 and (spans2[:, 1] <= per).all() and len(set(tags2.tolist())) >= 3
            mixed = dict(pats=pats, hits=hit_cap2, nspans=nspans2, span_off=span_off2, spans=spans2, tags=tags2)
        nspans_max = max(nspans, mixed["nspans"] if mixed else 0)

        ototal_max = total + maxr * nspans_max
        cap = int(lib.mh_encode_batch_bound(dst.handle, ototal_max, n))
        nidx = int(lib.mh_batch_index_capacity(ototal_max, n, CHUNK))
        wsb = max(lib.mh_dev_recode_splice_workspace(n, total, CHUNK, nspans), lib.mh_dev_recode_edit_workspace(n, total, CHUNK),
                  lib.mh_dev_decode_batch_workspace(n), lib.mh_dev_encode_batch_workspace(n, ototal_max))
        if table:
            wsb = max(wsb, lib.mh_dev_recode_splice_table_workspace(n, total, CHUNK, nspans_max, len(MIXED)))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total + 64, dtype=torch.uint8, device="cuda")        # the decoded bytes, the replacements behind them
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

        # the table splice: one entry and every tag 0 on the same spans, then the mixed table on the tagged spans
        def table_call(d_soff, d_sp, d_tg, d_roff, d_rbytes, nreps):
            o = out["got"]
            mhc._check(lib.mh_dev_recode_splice_table_batch(src.handle, dst.handle, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total,
                                                            PREV0, ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_soff), ptr(d_sp), ptr(d_tg),
                                                            ptr(d_roff), ptr(d_rbytes), nreps, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(d_oso),
                                                            ptr(o[3]), nidx, ptr(d_drop), None, ptr(d_ws), wsb, None), "splice_table")

        def same_as_ref(what, d_yoff):
            r, g = out["ref"], out["got"]
            nb = int(r[1][-1].item())
            assert torch.equal(r[1], g[1]) and torch.equal(r[2], g[2]) and torch.equal(r[0][:nb], g[0][:nb]) and torch.equal(r[3], g[3]), what
            assert torch.equal(d_oso, d_yoff), (what, "out_sym_off")

        fns2 = {}
        if table:
            d_zero = torch.zeros(max(nspans, 1), dtype=torch.int32, device="cuda")
            d_roff1 = {k: dev(np.array([0, len(v)], dtype=np.uint64)) for k, v in REPS.items()}
            for k in REPS:
                for t in out["ref"] + out["got"]:
                    t.zero_()
                composition(k)
                table_call(d_span_off, d_spans, d_zero, d_roff1[k], d_reps[k], 1)
                assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, k, "table, one entry")
                same_as_ref((dname, k, "table, one entry"), plan[k][1])
            # the mixed table's composition: the gather of the single replacement with a length and a source per span
            sp2, tg2, so2 = mixed["spans"], mixed["tags"], mixed["span_off"]
            rlen_of = np.array([len(r) for r in MIXED], dtype=np.int64)
            roff_of = np.concatenate([[0], np.cumsum(rlen_of)]).astype(np.int64)
            stream2 = np.repeat(np.arange(n, dtype=np.int64), np.diff(so2))
            m_begin = torch.from_numpy(stream2 * per + sp2[:, 0]).cuda()
            m_end = torch.from_numpy(stream2 * per + sp2[:, 1]).cuda()
            ones = torch.ones(len(sp2), dtype=torch.int32, device="cuda")
            delta = torch.zeros(total + 1, dtype=torch.int32, device="cuda")
            delta.index_add_(0, m_begin, ones)
            delta.index_add_(0, m_end, -ones)
            count = (torch.cumsum(delta[:total], 0) == 0).to(torch.int32)
            del delta
            count[m_begin] = torch.from_numpy(rlen_of[tg2]).to(torch.int32).cuda()
            m_src = torch.repeat_interleave(torch.arange(total, dtype=torch.int32, device="cuda"), count)
            start = torch.cumsum(count, 0, dtype=torch.int64) - count
            rep_at = torch.full((total,), -1, dtype=torch.int32, device="cuda")
            rep_at[m_begin] = torch.from_numpy(roff_of[tg2]).to(torch.int32).cuda()
            sp64 = m_src.to(torch.int64)
            within = (torch.arange(m_src.numel(), dtype=torch.int64, device="cuda") - start[sp64]).to(torch.int32)
            m_src = torch.where(rep_at[sp64] >= 0, within + rep_at[sp64] + total, m_src)
            del start, rep_at, sp64, within, count
            removed2 = np.bincount(stream2, weights=sp2[:, 1] - sp2[:, 0], minlength=n).astype(np.int64)
            added2 = np.bincount(stream2, weights=rlen_of[tg2], minlength=n).astype(np.int64)
            m_yoff = np.concatenate([[0], np.cumsum(per - removed2 + added2)]).astype(np.uint64)
            assert m_src.numel() == int(m_yoff[-1])
            d_myoff, m_total = dev(m_yoff), int(m_yoff[-1])
            d_mbytes = dev(np.frombuffer(b"".join(MIXED) + b"\0" * 16, dtype=np.uint8).copy())
            d_mroff = dev(roff_of.astype(np.uint64))
            nb_table = int(roff_of[-1])
            torch.cuda.empty_cache()

            def composition_mixed():
                decode()
                d_all[total:total + nb_table] = d_mbytes[:nb_table]
                torch.index_select(d_all, 0, m_src, out=d_y[:m_total])
                o = out["ref"]
                mhc._check(lib.mh_dev_encode_batch(dst.handle, ptr(d_y), ptr(d_myoff), n, m_total, PREV0, ptr(o[0]), cap, ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                                   CHUNK, ptr(d_ws), wsb, None), "encode")

            def table_mixed():
                table_call(d_span_off2, d_spans2, d_tags2, d_mroff, d_mbytes, len(MIXED))
            for t in out["ref"] + out["got"]:
                t.zero_()
            composition_mixed()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, "mixed composition")
            table_mixed()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, "table, mixed")
            same_as_ref((dname, "table, mixed"), d_myoff)
            fns2 = {"spans_untagged": spans_untagged, "spans_tagged": spans_tagged, "table_mixed": table_mixed, "decode_mixed_encode": composition_mixed}

        fns = {"edit_spans": edit}
        for k in REPS:
            fns["splice_" + k] = lambda k=k: splice(k)
            if table:
                fns["table_one_" + k] = lambda k=k: table_call(d_span_off, d_spans, d_zero, d_roff1[k], d_reps[k], 1)
            fns["decode_%s_encode" % k] = lambda k=k: composition(k)
        o = {k: stats(v) for k, v in interleaved(fns, args.reps).items()}
        for k in REPS:
            s = o["splice_" + k]
            s["ratio_edit"] = round(s["median_ms"] / o["edit_spans"]["median_ms"], 3)
            s["ratio_composition"] = round(s["median_ms"] / o["decode_%s_encode" % k]["median_ms"], 3)
            if table:
                t = o["table_one_" + k]
                t["ratio_splice"] = round(t["median_ms"] / s["median_ms"], 3)
                t["ratio_composition"] = round(t["median_ms"] / o["decode_%s_encode" % k]["median_ms"], 3)
        if table:
            o.update({k: stats(v) for k, v in interleaved(fns2, args.reps).items()})
            o["spans_tagged"]["ratio_untagged"] = round(o["spans_tagged"]["median_ms"] / o["spans_untagged"]["median_ms"], 3)
            o["table_mixed"]["ratio_composition"] = round(o["table_mixed"]["median_ms"] / o["decode_mixed_encode"]["median_ms"], 3)
            o["dictionary"] = {"patterns": [p.hex() for p in mixed["pats"]], "table": [r.decode() for r in MIXED], "hits": mixed["hits"],
                               "spans": mixed["nspans"], "spans_per_tag": np.bincount(mixed["tags"], minlength=len(MIXED)).tolist(),
                               "removed_bytes": int(removed2.sum()), "inserted_bytes": int(added2.sum())}
        o["pattern"] = pat.hex()
        o["hits"], o["spans"] = hit_cap, nspans
        o["removed_bytes"] = int(removed.sum())
        o["workspace_bytes"] = {"splice": int(lib.mh_dev_recode_splice_workspace(n, total, CHUNK, nspans)),
                                "edit": int(lib.mh_dev_recode_edit_workspace(n, total, CHUNK)), "decoded_buffer": total}
        if table:
            o["workspace_bytes"]["splice_table"] = int(lib.mh_dev_recode_splice_table_workspace(n, total, CHUNK, mixed["nspans"], len(MIXED)))
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
