"""The two device calls of include/mh.h "SELECTING RECORDS OF BATCHES" on a non-default stream.  They take an argument block
whose workspace and stream are a nested `mh_launch`, so neither the count of positional `void *stream` declarations that
tests/test_gpu_stream_order.py pins nor the count of blocks with a `void *stream` member that
tests/test_gpu_stream_order_o2_edit.py pins sees them; this module keeps their promise for these calls, with the harness of the
first (Chain, drive, the fixtures) under the same rules: one torch.cuda.Stream(), no host wait between calls, every host-side
size from the references, the model and the pattern set built beforehand, a second run behind the blocker.

  chain S   search -> pick list of the records with a hit -> select (count only, then in full with its index) -> indexed
            decode of the selected batch, every call reading what the one before wrote on the device

Every expected value comes from the original messages (find_ref, select_ref, batch_ref and the oracle's codes), never from
another call of the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import batch_ref
import find_ref
import select_cases
import select_ref
from conftest import ROOT
from test_gpu_stream_order import FILL, Batch, Chain, add_decode, drive, env, gpu, ptr, same  # noqa: F401 (env: the fixture of the stream chains)

LAUNCH_CALLS = 2                    # the mh_dev_* declarations of include/mh.h that take a block with an `mh_launch` member


def launch_calls():
    """The mh_dev_* declarations whose one parameter is a `const mh_*_args *` to a struct with an `mh_launch` member."""
    with open(os.path.join(ROOT, "include", "mh.h")) as f:
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    structs = {m.group(3) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text)
               if re.search(r"\bmh_launch\s+\w+\s*;", m.group(2))}
    return [m.group(1) for m in re.finditer(r"\b(mh_dev_\w+)\s*\(\s*const\s+(mh_\w+_args)\s*\*\s*\w+\s*\)\s*;", text) if m.group(2) in structs]


def test_the_calls_that_take_a_launch_block_are_the_two_and_both_are_driven_here():
    calls = launch_calls()
    assert sorted(calls) == ["mh_dev_picks_from_hits", "mh_dev_select_batch"] and len(calls) == LAUNCH_CALLS, calls
    source = inspect.getsource(test_chain_s_grep_with_compressed_output)
    for c in calls:
        assert re.search(r"\blib\.%s\b(?!\w)" % c, source), "%s: no stream-order chain drives it" % c


@gpu
def test_chain_s_grep_with_compressed_output(env):
    mhc, lib = env.mhc, env.lib
    n, c, p0 = 257, 256, batch_ref.PREV0
    msgs = select_cases.records(n, 41)
    total = sum(len(m) for m in msgs)
    counts = batch_ref.histogram(msgs, 1, p0)
    q = batch_ref.pack(msgs, *batch_ref.oracle_codes(counts, 1), 1, p0, c)
    S = mhc.Model.from_counts(counts, 1)
    ps = mhc.PatternSet([b"GPU"])
    # the references: hit counts, the pick list, the selected batch and its messages
    w_off, _, _ = find_ref.hit_arrays(find_ref.find_hits(msgs, [b"GPU"]), n)
    picks, kept = select_ref.picks_from_hits(w_off, None, 0)
    want = select_ref.select([q], picks, c)
    kept_msgs = [msgs[int(p)] for p in picks[:kept]]
    cap, sym_total = int(want.pay_off[n]), int(want.sym_off[n])
    nidx = int(lib.mh_batch_index_capacity(sym_total, n, c))
    assert n // 4 < kept < 3 * n // 4 and cap > 4096
    ch = Chain(env, "chain S")
    ch.keep = (S, ps)
    b = Batch(ch.staged(q.payload), ch.staged(q.pay_off), ch.staged(q.nbits), n, int(q.pay_off[n]))
    d_in, d_idx = ch.staged(q.sym_off), ch.staged(q.index_array(c))
    # 1. the search, count only: hit_off
    wsb = lib.mh_dev_find_batch_workspace(n, total, c)
    d_ws, d_ho, d_fst = ch.work(wsb), ch.words(n + 1), ch.status(n, "find_batch")
    ch.call("find_batch", lib.mh_dev_find_batch, S.handle, ps.handle, *b.args(), p0, ptr(d_in), total, ptr(d_idx), c, ptr(d_ho), None, None, 0,
            ptr(d_fst), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("find_batch: hit_off", lambda: same(ch.get(d_ho, np.uint64, n + 1), w_off))
    # 2. the records with a hit and an MH_OK verdict, as picks
    pick_list = lambda *a: lib.mh_dev_picks_from_hits(C.byref(mhc.picks_args(*a)))
    wsb = lib.mh_dev_picks_from_hits_workspace(n)
    d_ws, d_picks, d_kept = ch.work(wsb), ch.words(n), ch.words(1)
    ch.call("picks_from_hits", pick_list, ptr(d_ho), ptr(d_fst), n, 0, 0, ptr(d_picks), ptr(d_kept), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("picks_from_hits: picks and n_kept", lambda: same(ch.get(d_picks, np.uint64, n), picks) and int(ch.get(d_kept, np.uint64, 1)[0]) == kept)
    # 3. select with n_picks = n, count only and in full, with exactly the reference's room
    select = lambda *a: lib.mh_dev_select_batch(C.byref(mhc.select_args(*a)))
    sources = mhc.coded_batches([(ptr(b.pl), ptr(b.po), ptr(b.nb), n, b.pay_total, ptr(d_in), total, ptr(d_idx), c)])
    wsb = lib.mh_dev_select_batch_workspace(n, n)
    for full in (False, True):
        t = "select_batch" + ("" if full else " count only")
        d_ws, d_pst = ch.work(wsb), ch.status(n, t)
        d_oo, d_onb, d_oso = ch.words(n + 1), ch.words(n), ch.words(n + 1)
        d_out, d_oi = (ch.out(cap + 64), ch.words(nidx)) if full else (None, None)
        ch.call(t, select, sources, 1, ptr(d_picks), n, ptr(d_out), cap, ptr(d_oo), ptr(d_onb), ptr(d_oso), ptr(d_oi), nidx, c, ptr(d_pst),
                ptr(d_ws), wsb, ws=d_ws)
        ch.expect(t + ": offsets, nbits, sym_off", lambda d_oo=d_oo, d_onb=d_onb, d_oso=d_oso: same(ch.get(d_oo, np.uint64, n + 1), want.pay_off)
                  and same(ch.get(d_onb, np.uint64, n), want.nbits) and same(ch.get(d_oso, np.uint64, n + 1), want.sym_off))
    ch.expect("select_batch: payload", lambda: same(ch.get(d_out, np.uint8, cap), want.payload) and (ch.get(d_out)[cap:cap + 64] == FILL).all())
    ch.expect("select_batch: the index, gaps included", lambda: same(ch.get(d_oi, np.uint64, nidx), want.index_array(c)))
    # 4. the selected batch decodes, through its relocated index, to the kept records
    add_decode(ch, "decode_batch of the selected", lib.mh_dev_decode_batch, lib.mh_dev_decode_batch_workspace, S.handle,
               Batch(d_out, d_oo, d_onb, n, cap), p0, sym_total, d_oso, d_oi, c, b"".join(kept_msgs), want.sym_off)
    drive(ch)
