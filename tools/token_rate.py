"""Rate of the span tokens (include/mh.h, "TOKENS FROM MATCHED BYTES") against the lookups that decode the same (stream, begin,
end) into memory, and of the scrubber chain with tokens against the chain with a constant table.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text input_wiki_cpp.txt
tiled), coded under a shared order-1 model with chunk 1024, indexed, HIP events, every variant run once per repetition in turn
(interleaved), medians with min and max.  The spans are those of a real search of one two-byte pattern chosen for about one and
about three hits per record, merged by mh_spans_from_hits_tagged:
  tokens          mh_dev_span_tokens_batch, format `<T:` 16 digits `>`, a table with one entry per span;
  lookups         mh_dev_decode_batch_ranges (order 2: mh_dev_decode_batch_o2_ranges) on the same (stream, begin, end): the same decode with stores instead of the hash
                  (`ratio_lookups`: tokens over lookups).  --baseline-lib PATH times it with another build of the library (the
                  parent commit's), its model built there from the same counts;
  chain_const     mh_dev_find_batch + mh_dev_spans_from_hits_tagged + mh_dev_recode_splice_table_batch with the one-entry table
                  `<T>`: the chain as it was;
  chain_tokens    the same with mh_dev_span_tokens_batch between the spans and the splice, which takes its table
                  (`ratio_chain`: chain_tokens over chain_const).
`spread` is (max - min) / median of a variant's own repetitions.  The first 200 entries of the token table are checked against
tests/token_ref.py before the clock.  `long_span`: the token call on one stream with one span of 64 KiB (one lane, serial).
Prints one JSON line.

    python tools/token_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE] [--baseline-lib PATH]
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
import token_ref  # noqa: E402
from edit_rate import pattern_for  # noqa: E402
from recode_rate import CHUNK, PREV0, interleaved, ptr, stats, zipf  # noqa: E402

FORMAT = (b"<T:", 16, b">")
KEY = token_ref.KEY


def dev(a):
    """Any array on the device, as bytes."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def spread(s):
    return round((s["max_ms"] - s["min_ms"]) / s["median_ms"], 4) if s["median_ms"] else 0.0


LAST_SPANS = {}                                    # the (span_off, spans) of the last searched measure(): positions, model-free


def baseline(path, counts, order):
    """Another build of the library and its own model of the same counts: (lib, model handle)."""
    lb = C.CDLL(path)
    h = C.c_void_p()
    lb.mh_model_from_counts.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    rc = lb.mh_model_from_counts(counts.ctypes.data, order, C.byref(h))
    assert rc == 0, rc
    vp, sz, u8, u32, u64 = C.c_void_p, C.c_size_t, C.c_uint8, C.c_uint32, C.c_uint64
    for name in ("mh_dev_decode_batch_ranges", "mh_dev_decode_batch_o2_ranges"):
        getattr(lb, name).argtypes = [vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, vp, u64, vp, vp, sz, vp]
        getattr(lb, name + "_workspace").argtypes = [sz]
        getattr(lb, name + "_workspace").restype = sz
    lb.mh_dev_status.argtypes = [vp, vp]
    return lb, h


def measure(mhc, lib, msgs, per_record, reps, base_path, check=200, chain=True, order=1):
    n = len(msgs)
    total = sum(len(m) for m in msgs)
    counts = mhc.histogram_o2_batch(msgs) if order == 2 else mhc.histogram_o1_batch(msgs)
    src = mhc.Model.from_counts(counts, order)
    dst = mhc.Model.from_counts(counts + np.uint64(1), 1) if order == 1 else None   # covers every pair of a scrubbed message
    payload, pay_off, nbits, idx, in_off = (src.encode_batch_o2 if order == 2 else src.encode_batch)(msgs, chunk_symbols=CHUNK)
    pay_total = int(pay_off[-1])
    d = dict(payload=dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)])), pay_off=dev(pay_off), nbits=dev(nbits), in_off=dev(in_off), idx=dev(idx))
    batch = (ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, pay_total)
    if isinstance(per_record, tuple):                                        # given spans: (span_off, spans)
        pat, (so, sp) = None, per_record
        tg = np.zeros(len(sp), dtype=np.uint32)
    else:
        data = np.frombuffer(b"".join(msgs[:4096]), dtype=np.uint8)
        pat = pattern_for(data, max(len(msgs[0]) // per_record, 1))
        ho, rec, hp, _, rc = src.dev_find_batch(mhc.PatternSet([pat]), payload, pay_off, nbits, sym_off=in_off, index=idx, chunk_symbols=CHUNK)
        assert rc == mhc.MH_OK
        so, sp, tg, rc = mhc.spans_from_hits_tagged(ho, rec, hp)
        assert rc == mhc.MH_OK
        LAST_SPANS["spans"] = (so, sp)
    k = m = len(sp)
    assert m > 0
    ps = mhc.PatternSet([pat]) if pat else None
    # device buffers
    empty = lambda nbytes: torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")
    d_so, d_sp, d_tg = dev(so), dev(np.ascontiguousarray(sp).reshape(-1)), dev(tg)
    f_off, f_bytes, f_hex = token_ref.format_arrays([FORMAT])
    d_foff, d_fb, d_hex = dev(f_off), dev(f_bytes), dev(f_hex)
    tok_len = len(FORMAT[0]) + FORMAT[1] + len(FORMAT[2])
    rep_cap = m * tok_len
    d_roff, d_rb, d_rtag, d_st = empty((m + 1) * 8), empty(rep_cap + 64), empty(m * 4), empty(n * 4)
    wsb_t = lib.mh_dev_span_tokens_workspace(n, m)
    d_wst = empty(wsb_t)
    launch = mhc.launch_args(ptr(d_wst), wsb_t, None)

    def tokens(spans=(d_so, d_sp, d_tg)):
        blk = mhc.span_tokens_args(src.handle, None, (*batch, ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, PREV0), ptr(spans[0]), ptr(spans[1]),
                                   ptr(spans[2]), KEY, 0, ptr(d_foff), ptr(d_fb), ptr(d_hex), 1, m, ptr(d_roff), ptr(d_rb), rep_cap, ptr(d_rtag), ptr(d_st))
        mhc._check(lib.mh_dev_span_tokens_batch(C.byref(blk), C.byref(launch)), "span_tokens")

    # the lookups of the same spans
    stream_of = np.repeat(np.arange(n, dtype=np.uint64), np.diff(so).astype(np.int64))
    lk = np.stack([stream_of, sp[:, 0], sp[:, 1]], axis=1).astype(np.uint64)
    ln = (sp[:, 1] - sp[:, 0]).astype(np.uint64)
    at = np.zeros(m, dtype=np.uint64)
    at[1:] = np.cumsum(ln)[:-1]
    size = int(ln.sum())
    d_lk, d_at, d_lout, d_lst = dev(lk.reshape(-1)), dev(at), empty(size + 64), empty(m * 4)
    lb, hb = (lib, src.handle) if not base_path else baseline(base_path, counts, order)
    lookup_call = "mh_dev_decode_batch_o2_ranges" if order == 2 else "mh_dev_decode_batch_ranges"
    wsb_l = getattr(lb, lookup_call + "_workspace")(m)
    d_wsl = empty(wsb_l)

    def lookups():
        rc = getattr(lb, lookup_call)(hb, ptr(d["payload"]), ptr(d["pay_off"]), ptr(d["nbits"]), n, PREV0, ptr(d["in_off"]), ptr(d["idx"]), CHUNK,
                                           ptr(d_lk), m, ptr(d_lout), ptr(d_at), size, ptr(d_lst), ptr(d_wsl), wsb_l, None)
        assert rc == 0, rc

    # before the clock: both calls pass, and the first entries are the reference's
    tokens()
    lookups()
    torch.cuda.synchronize()
    assert lib.mh_dev_status(ptr(d_wst), None) == 0 and lb.mh_dev_status(ptr(d_wsl), None) == 0
    roff, rb = d_roff.cpu().numpy().view(np.uint64)[:m + 1], d_rb.cpu().numpy()
    assert np.array_equal(roff, np.arange(m + 1, dtype=np.uint64) * np.uint64(tok_len))
    for r in range(min(check, m)):
        i = int(stream_of[r])
        assert rb[r * tok_len:(r + 1) * tok_len].tobytes() == token_ref.token(FORMAT, KEY, msgs[i][int(sp[r, 0]):int(sp[r, 1])]), r
    fns = {"tokens": tokens, "lookups": lookups}
    if chain and ps is not None and order == 1:
        cap = int(lib.mh_encode_batch_bound(dst.handle, total + m * tok_len, n))
        nidx = int(lib.mh_batch_index_capacity(total + m * tok_len, n, CHUNK))
        wsb = max(lib.mh_dev_find_batch_workspace(n, total, CHUNK), lib.mh_dev_spans_from_hits_tagged_workspace(n, k),
                  lib.mh_dev_recode_splice_table_workspace(n, total, CHUNK, k, k))
        d_ws = empty(wsb)
        d_ho, d_rec, d_pat = empty((n + 1) * 8), empty(k * 24 + 64), empty(k * 4 + 64)
        c_so, c_sp, c_tg = empty((n + 1) * 8), empty(k * 16 + 64), empty(k * 4 + 64)
        o_pl, o_off, o_nb, o_so, o_idx, o_dr = empty(cap + 64), empty((n + 1) * 8), empty(n * 8), empty((n + 1) * 8), empty(nidx * 8), empty(n * 8)
        one_off, one_bytes = dev(np.array([0, 3], dtype=np.uint64)), dev(np.frombuffer(b"<T>", dtype=np.uint8).copy())

        def find_and_spans():
            mhc._check(lib.mh_dev_find_batch(src.handle, ps.handle, *batch, PREV0, ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(d_ho), ptr(d_rec),
                                             ptr(d_pat), k, None, ptr(d_ws), wsb, None), "find")
            mhc._check(lib.mh_dev_spans_from_hits_tagged(ptr(d_ho), ptr(d_rec), ptr(d_pat), k, n, ptr(c_so), ptr(c_sp), ptr(c_tg), ptr(d_ws), wsb, None),
                       "spans")

        def splice(tag, roff_, rbytes, nreps):
            mhc._check(lib.mh_dev_recode_splice_table_batch(src.handle, dst.handle, *batch, PREV0, ptr(d["in_off"]), total, ptr(d["idx"]), CHUNK, ptr(c_so),
                                                            ptr(c_sp), ptr(tag), ptr(roff_), ptr(rbytes), nreps, ptr(o_pl), cap, ptr(o_off), ptr(o_nb),
                                                            ptr(o_so), ptr(o_idx), nidx, ptr(o_dr), None, ptr(d_ws), wsb, None), "splice")

        def chain_const():
            find_and_spans()
            splice(c_tg, one_off, one_bytes, 1)

        def chain_tokens():
            find_and_spans()
            tokens((c_so, c_sp, c_tg))
            splice(d_rtag, d_roff, d_rb, m)

        for fn in (chain_const, chain_tokens):
            fn()
            torch.cuda.synchronize()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0 and lib.mh_dev_status(ptr(d_wst), None) == 0, fn.__name__
        fns.update(chain_const=chain_const, chain_tokens=chain_tokens)
    ms = {name: stats(v) for name, v in interleaved(fns, reps).items()}
    out = {"spans": m, "span_bytes": size, "pattern": pat.hex() if pat else None}
    for name, s in ms.items():
        out[name] = dict(s, spread=spread(s))
    out["ratio_lookups"] = round(ms["tokens"]["median_ms"] / ms["lookups"]["median_ms"], 4)
    if "chain_const" in ms:
        out["ratio_chain"] = round(ms["chain_tokens"]["median_ms"] / ms["chain_const"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's) for the lookups")
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("token_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "token_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "lookups_library": "baseline" if args.baseline_lib else "this build"}
    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        for density in (1, 3):
            res["%s_%d_per_record" % (dname, density)] = measure(mhc, lib, msgs, density, args.reps, args.baseline_lib)
            if density == 1:                                      # the same spans under a shared order-2 model, against the _o2 lookups
                try:
                    r = measure(mhc, lib, msgs, LAST_SPANS["spans"], args.reps, args.baseline_lib, chain=False, order=2)
                    res["%s_1_per_record_order2" % dname] = {k: r[k] for k in ("spans", "span_bytes", "tokens", "lookups", "ratio_lookups")}
                except Exception as e:                            # (recorded, so that the other rows survive)
                    res["%s_1_per_record_order2" % dname] = {"error": "%s: %s" % (type(e).__name__, e)}
    # one lane, one span of 64 KiB
    long_msg = [zipf(1 << 17, 9).tobytes()]
    spans = (np.array([0, 1], dtype=np.uint64), np.array([[100, 100 + (1 << 16)]], dtype=np.uint64))
    r = measure(mhc, lib, long_msg, spans, args.reps, args.baseline_lib, check=1, chain=False)
    res["long_span"] = {"span_bytes": 1 << 16, "tokens": r["tokens"], "lookups": r["lookups"], "ratio_lookups": r["ratio_lookups"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
