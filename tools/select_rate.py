"""Rate of selecting records of compressed batches (include/mh.h, "SELECTING RECORDS OF BATCHES") against its floor and
against what a caller did before.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text input_wiki_cpp.txt
tiled), coded under a shared order-1 model with chunk 1024, HIP events, every variant and its two yardsticks run once per
repetition in turn (interleaved), medians with min and max.  The variants of mh_dev_select_batch:
  identity      every record, in place order;
  permutation   every record, in a random order;
  grep          the records that a two-byte pattern hits (chosen for about half of the records), the picks made on the device
                by mh_dev_picks_from_hits from the hit_off of mh_dev_find_batch; n_picks = n, the tail of the output is empty;
  concat        two half batches, encoded apart, appended.
The yardsticks of each variant:
  copy          hipMemcpyAsync, device to device, of as many payload bytes and as many index bytes as the variant writes: the
                floor of any select;
  composition   what a caller does today: mh_dev_decode_batch, a torch gather of the records, mh_dev_encode_batch.
Every variant's output (offsets, bit counts, payload, index slices) is checked against the composition's before the clock.
Prints one JSON line; `ratio_copy` is a variant's median over its copy's, `ratio_composition` over its composition's.

    python tools/select_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
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
from recode_rate import CHUNK, PREV0, dev, interleaved, ptr, stats, zipf  # noqa: E402


def pattern_for(data, per, share=0.5):
    """The two-byte string that, were its occurrences spread evenly, would hit `share` of the records (Poisson: ln(1 / (1 - share))
    occurrences per record), counted in the first 16 MiB."""
    s = data[:1 << 24].astype(np.uint32)
    pairs = np.bincount((s[:-1] << 8) | s[1:], minlength=65536)
    want = int(s.size // per * np.log(1.0 / (1.0 - share)))
    p = int(np.argmin(np.abs(pairs.astype(np.int64) - want)))
    return bytes([p >> 8, p & 255])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select", "select_rate.json"))
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("select_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    hip_copy = C.CDLL(mhc.LIB_PATH).hipMemcpyAsync                # the HIP runtime libmhc.so is linked against
    hip_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n, per = args.streams, args.bytes
    half, total = n // 2, n * per
    assert n % 2 == 0
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "select_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda")

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)

        def encoded(part):
            payload, pay_off, nbits, idx, in_off = model.encode_batch(part, chunk_symbols=CHUNK)
            b = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off),
                     idx=dev(idx), n=len(part), pay_total=int(pay_off[-1]), total=len(part) * per)
            b["row"] = (ptr(b["payload"]), ptr(b["pay_off"]), ptr(b["nbits"]), b["n"], b["pay_total"], ptr(b["in_off"]), b["total"], ptr(b["idx"]), CHUNK)
            return b
        whole, first, second = encoded(msgs), encoded(msgs[:half]), encoded(msgs[half:])
        cap = int(lib.mh_encode_batch_bound(model.handle, total, n))
        nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
        wsb = max(lib.mh_dev_select_batch_workspace(n, n), lib.mh_dev_picks_from_hits_workspace(n), lib.mh_dev_decode_batch_workspace(n),
                  lib.mh_dev_encode_batch_workspace(n, total), lib.mh_dev_find_batch_workspace(n, total, CHUNK))
        d_ws = u8(wsb)
        out = {k: dict(payload=u8(cap + 64), off=i64(n + 1), nbits=i64(n), sym=i64(n + 1), idx=torch.zeros(nidx, dtype=torch.int64, device="cuda"))
               for k in ("ref", "got", "copy")}
        d_all, d_sel = u8(total), u8(total)
        d_so = i64(n + 1)

        # the grep variant's picks, made on the device outside the clock
        pat = pattern_for(data, per)
        ps = mhc.PatternSet([pat])
        d_ho, d_grep, d_kept = i64(n + 1), i64(n), i64(1)
        mhc._check(lib.mh_dev_find_batch(model.handle, ps.handle, *whole["row"][:5], PREV0, ptr(whole["in_off"]), total, ptr(whole["idx"]), CHUNK,
                                         ptr(d_ho), None, None, 0, None, ptr(d_ws), wsb, None), "find")
        assert lib.mh_dev_status(ptr(d_ws), None) == 0

        def picks_from_hits():
            mhc._check(lib.mh_dev_picks_from_hits(C.byref(mhc.picks_args(ptr(d_ho), None, n, 0, 0, ptr(d_grep), ptr(d_kept), ptr(d_ws), wsb, None))),
                       "picks_from_hits")
        picks_from_hits()
        kept = int(d_kept.item())
        grep = d_grep.cpu().numpy().view(np.uint64)
        assert (grep[kept:] == mhc.SELECT_NONE).all() and (np.diff(grep[:kept].astype(np.int64)) > 0).all()
        rng = np.random.default_rng(3)
        lists = {"identity": ([whole], np.arange(n, dtype=np.uint64), n),
                 "permutation": ([whole], rng.permutation(n).astype(np.uint64), n),
                 "grep": ([whole], grep, kept),
                 "concat": ([first, second], np.concatenate([np.arange(half, dtype=np.uint64),
                                                             np.arange(half, dtype=np.uint64) | np.uint64(1 << 56)]), n)}
        fns, sizes = {}, {}
        for vname, (batches, picks, k) in lists.items():
            d_picks = dev(picks)
            rows = np.array([(int(p) & ((1 << 56) - 1)) + (half if int(p) >> 56 else 0) for p in picks[:k]], dtype=np.int64)
            d_rows = dev(rows)
            d_in_sel = dev(np.arange(k + 1, dtype=np.uint64) * np.uint64(per))
            sources = mhc.coded_batches([b["row"] for b in batches])

            def select(batches=batches, sources=sources, d_picks=d_picks):
                o = out["got"]
                blk = mhc.select_args(sources, len(batches), ptr(d_picks), n, ptr(o["payload"]), cap, ptr(o["off"]), ptr(o["nbits"]), ptr(o["sym"]),
                                      ptr(o["idx"]), nidx, CHUNK, None, ptr(d_ws), wsb, None)
                mhc._check(lib.mh_dev_select_batch(C.byref(blk)), "select")

            def composition(batches=batches, d_rows=d_rows, d_in_sel=d_in_sel, k=k):
                at = 0
                for b in batches:                                  # decode every source into its place of d_all
                    d_so[:b["n"] + 1].copy_(b["in_off"])
                    mhc._check(lib.mh_dev_decode_batch(model.handle, *b["row"][:5], PREV0, C.c_void_p(d_all.data_ptr() + at), b["total"], ptr(d_so),
                                                       b["total"], ptr(b["idx"]), CHUNK, None, ptr(d_ws), wsb, None), "decode")
                    at += b["total"]
                torch.index_select(d_all.view(n, per), 0, d_rows, out=d_sel.view(n, per)[:k])
                o = out["ref"]
                mhc._check(lib.mh_dev_encode_batch(model.handle, ptr(d_sel), ptr(d_in_sel), k, k * per, PREV0, ptr(o["payload"]), cap, ptr(o["off"]),
                                                   ptr(o["nbits"]), ptr(o["idx"]), CHUNK, ptr(d_ws), wsb, None), "encode")

            # the variant's result against the composition's, before the clock
            for o in out.values():
                for t in o.values():
                    t.zero_()
            composition()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, vname)
            select()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, vname)
            r, g = out["ref"], out["got"]
            pay = int(r["off"][k].item())
            ents = k * per // CHUNK + k
            assert torch.equal(r["off"][:k + 1], g["off"][:k + 1]) and torch.equal(r["nbits"][:k], g["nbits"][:k]), (dname, vname)
            assert bool((g["off"][k:] == pay).all()) and bool((g["nbits"][k:] == 0).all()), (dname, vname)
            assert torch.equal(r["payload"][:pay], g["payload"][:pay]) and torch.equal(r["idx"][:ents], g["idx"][:ents]), (dname, vname)
            assert torch.equal(g["sym"][:k + 1], d_in_sel), (dname, vname)

            def copy(pay=pay, ents=ents, src=batches[0]):
                hip_copy(ptr(out["copy"]["payload"]), ptr(whole["payload"]), pay, 3, None)               # 3: hipMemcpyDeviceToDevice
                hip_copy(ptr(out["copy"]["idx"]), ptr(whole["idx"]), ents * 8, 3, None)
            fns[vname], fns[vname + ".copy"], fns[vname + ".composition"] = select, copy, composition
            sizes[vname] = {"records": k, "payload_bytes": pay, "index_bytes": ents * 8}
        fns["picks_from_hits"] = picks_from_hits
        o = {k: stats(v) for k, v in interleaved(fns, args.reps).items()}
        for vname in lists:
            o[vname].update(sizes[vname])
            o[vname]["ratio_copy"] = round(o[vname]["median_ms"] / o[vname + ".copy"]["median_ms"], 3)
            o[vname]["ratio_composition"] = round(o[vname]["median_ms"] / o[vname + ".composition"]["median_ms"], 4)
            o[vname]["GBps_written"] = round((sizes[vname]["payload_bytes"] + sizes[vname]["index_bytes"]) / o[vname]["median_ms"] / 1e6, 1)
        o["pattern"], o["kept_share"] = pat.hex(), round(kept / n, 4)
        o["workspace_bytes"] = {"select": int(lib.mh_dev_select_batch_workspace(n, n)), "picks_from_hits": int(lib.mh_dev_picks_from_hits_workspace(n)),
                                "decoded_buffer": total}
        res[dname] = o
        del whole, first, second, d_all, d_sel, d_ws, out
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
