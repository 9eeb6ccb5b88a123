"""The device call of include/mh.h "TOKENS FROM MATCHED BYTES" on a non-default stream.  It takes an argument block and, as a
second parameter, a `const mh_launch *`: a shape of its own, which none of the three counts that
tests/test_gpu_stream_order.py, tests/test_gpu_stream_order_o2_edit.py and tests/test_gpu_stream_order_select.py pin sees.  This
module counts the declarations of that shape and drives the call with the harness of the first (Chain, drive, the fixtures)
under the same rules: one torch.cuda.Stream(), no host wait between calls, every host-side size from the references, the models
and the dictionary built beforehand, a second run behind the blocker.

  chain T   dictionary search -> tagged spans -> tokens (count only, then in full) -> table splice under another model ->
            indexed decode of the scrubbed batch, every call reading what the one before wrote on the device

Every expected value comes from the original messages (find_ref, splice_table_ref, token_ref, batch_ref and the oracle's codes),
never from another call of the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import batch_ref
import find_ref
import select_cases
import splice_table_ref
import token_ref
from conftest import ROOT
from test_gpu_stream_order import FILL, Batch, Chain, add_decode, drive, env, gpu, ptr, same  # noqa: F401 (env: the fixture of the stream chains)
from test_gpu_stream_order_edit import add_edit, clear_behind, zeros

TWO_PARAMETER_CALLS = 1             # the mh_dev_* declarations of include/mh.h that take (const mh_*_args *, const mh_launch *)


def two_parameter_calls():
    with open(os.path.join(ROOT, "include", "mh.h")) as f:
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    return [m.group(1) for m in re.finditer(r"\b(mh_dev_\w+)\s*\(\s*const\s+mh_\w+_args\s*\*\s*\w+\s*,\s*const\s+mh_launch\s*\*\s*\w+\s*\)\s*;", text)]


def test_the_calls_that_take_a_block_and_a_launch_are_one_and_it_is_driven_here():
    calls = two_parameter_calls()
    assert calls == ["mh_dev_span_tokens_batch"] and len(calls) == TWO_PARAMETER_CALLS, calls
    source = inspect.getsource(test_chain_t_pseudonymise)
    for c in calls:
        assert re.search(r"\blib\.%s\b(?!\w)" % c, source), "%s: no stream-order chain drives it" % c


@gpu
def test_chain_t_pseudonymise(env):
    mhc, lib = env.mhc, env.lib
    n, c, p0 = 129, 256, batch_ref.PREV0
    msgs = select_cases.records(n, 43)
    total = sum(len(m) for m in msgs)
    pats = [b"the", b"GPU", b"was"]                                 # folded: `The` hits too, and has the token of `the`
    formats = [(b"<W:", 16, b">"), (b"<GPU>", 0, b""), (b"", 0, b"")]
    key, flags = token_ref.KEY, token_ref.FOLD
    # the references: records, tagged spans, the token table, the scrubbed messages and their batch under the other model
    w_off, w_rec, w_pat = find_ref.hit_arrays(find_ref.find_hits(msgs, pats, fold=True), n)
    k = len(w_rec)
    t_off, t_spans, t_tags = splice_table_ref.merge_tagged(w_off, w_rec, w_pat)
    m = len(t_spans)
    entries = token_ref.table(msgs, t_off, t_spans, t_tags, formats, key, flags)
    r_off, r_bytes, r_tag = token_ref.table_arrays(entries, k)
    scrubbed = token_ref.apply(msgs, t_off, t_spans, t_tags, formats, key, flags)
    assert m > 200 and {0, 1, 2} <= set(t_tags.tolist()) and any(b"The" in x for x in msgs) and r_bytes.size > 1000
    counts = batch_ref.histogram(msgs, 1, p0)
    q = batch_ref.pack(msgs, *batch_ref.oracle_codes(counts, 1), 1, p0, c)
    dcounts = batch_ref.histogram(msgs + scrubbed, 1, p0)
    want = batch_ref.pack(scrubbed, *batch_ref.oracle_codes(dcounts, 1), 1, p0, c)
    assert not want.dropped.any()
    S, D = mhc.Model.from_counts(counts, 1), mhc.Model.from_counts(dcounts, 1)
    dic = mhc.Dict(pats, fold=True)
    ch = Chain(env, "chain T")
    ch.keep = (S, D, dic)
    b = Batch(ch.staged(np.concatenate([q.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(q.pay_off), ch.staged(q.nbits), n, int(q.pay_off[n]))
    d_in, d_idx = ch.staged(q.sym_off), ch.staged(q.index_array(c))
    # 1. the dictionary search, with exactly the reference's number of records
    wsb = lib.mh_dev_find_dict_workspace(n, total, c)
    d_ws, d_ho, d_rec, d_pat, d_fst = ch.work(wsb), zeros(ch, (n + 1) * 8), zeros(ch, k * 24 + 64), zeros(ch, k * 4 + 64), ch.status(n, "find_dict_batch")
    ch.call("find_dict_batch", lib.mh_dev_find_dict_batch, S.handle, dic.handle, *b.args(), p0, ptr(d_in), total, ptr(d_idx), c, ptr(d_ho), ptr(d_rec),
            ptr(d_pat), k, ptr(d_fst), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("find_dict_batch: hit_off, records, patterns", lambda: same(ch.get(d_ho, np.uint64, n + 1), w_off)
              and same(ch.get(d_rec, np.uint64, 3 * k).reshape(-1, 3), w_rec) and same(ch.get(d_pat, np.uint32, k), w_pat))
    # 2. tagged spans: at most k of them
    wsb = lib.mh_dev_spans_from_hits_tagged_workspace(n, k)
    d_ws, d_so, d_sp, d_tg = ch.work(wsb), zeros(ch, (n + 1) * 8), zeros(ch, k * 16 + 64), zeros(ch, k * 4 + 64)
    ch.call("spans_from_hits_tagged", lib.mh_dev_spans_from_hits_tagged, ptr(d_ho), ptr(d_rec), ptr(d_pat), k, n, ptr(d_so), ptr(d_sp), ptr(d_tg),
            ptr(d_ws), wsb, ws=d_ws)
    ch.expect("spans_from_hits_tagged: span_off, spans, tags", lambda: same(ch.get(d_so, np.uint64, n + 1), t_off)
              and same(ch.get(d_sp, np.uint64, 2 * m).reshape(-1, 2), t_spans) and same(ch.get(d_tg, np.uint32, m), t_tags))
    # 3. the tokens: a table of k entries (the caller's bound on the spans), count only and in full with exactly the reference's bytes
    f_off, f_bytes, f_hex = token_ref.format_arrays(formats)
    d_foff, d_fb, d_hex = ch.staged(f_off), ch.staged(f_bytes), ch.staged(f_hex)

    def span_tokens(d_roff, d_rb, cap, d_rtag, d_st, d_ws, wsb, stream):
        blk = mhc.span_tokens_args(S.handle, None, (ptr(b.pl), ptr(b.po), ptr(b.nb), n, b.pay_total, ptr(d_in), total, ptr(d_idx), c, p0), ptr(d_so),
                                   ptr(d_sp), ptr(d_tg), key, flags, ptr(d_foff), ptr(d_fb), ptr(d_hex), len(formats), k, ptr(d_roff), ptr(d_rb), cap,
                                   ptr(d_rtag), ptr(d_st))
        return lib.mh_dev_span_tokens_batch(C.byref(blk), C.byref(mhc.launch_args(ptr(d_ws), wsb, stream)))

    wsb = lib.mh_dev_span_tokens_workspace(n, k)
    cap = int(r_bytes.size)
    for full in (False, True):
        t = "span_tokens_batch" + ("" if full else " count only")
        d_ws, d_roff, d_rtag, d_st = ch.work(wsb), zeros(ch, (k + 1) * 8 + 64), zeros(ch, k * 4 + 64), ch.status(n, t)
        d_rb = ch.out(cap + 64) if full else None
        ch.call(t, span_tokens, d_roff, d_rb, cap, d_rtag, d_st, d_ws, wsb, ws=d_ws)
        ch.expect(t + ": rep_off, rep_tag", lambda d_roff=d_roff, d_rtag=d_rtag: same(ch.get(d_roff, np.uint64, k + 1), r_off)
                  and clear_behind(ch, d_roff, (k + 1) * 8) and same(ch.get(d_rtag, np.uint32, k), r_tag) and clear_behind(ch, d_rtag, k * 4))
    ch.expect("span_tokens_batch: rep_bytes", lambda: same(ch.get(d_rb, np.uint8, cap), r_bytes) and (ch.get(d_rb)[cap:cap + 64] == FILL).all())
    # 4. the table splice under the other model, on the device's spans with the table the tokens call wrote
    wsb = lib.mh_dev_recode_splice_table_workspace(n, total, c, k, k)
    mid = (ptr(d_so), ptr(d_sp), ptr(d_rtag), ptr(d_roff), ptr(d_rb), k)
    tb, d_oi, d_oso = add_edit(ch, "recode_splice_table_batch", lib.mh_dev_recode_splice_table_batch, wsb, S.handle, D.handle, b, p0, total, q.sym_off,
                               d_in, d_idx, c, mid, want, splice=True)
    # 5. the scrubbed batch decodes, through the index the splice wrote, to the reference's messages
    out_total = int(want.sym_off[n])
    add_decode(ch, "decode_batch of the scrubbed", lib.mh_dev_decode_batch, lib.mh_dev_decode_batch_workspace, D.handle, tb, p0, out_total, d_oso, d_oi, c,
               b"".join(scrubbed), want.sym_off)
    drive(ch)
