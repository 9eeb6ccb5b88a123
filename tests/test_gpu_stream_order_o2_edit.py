"""The two device calls of include/mh.h "ORDER 2 IN EDITING AND SPLICING" on a non-default stream.  They take an argument block
(`const mh_*_args *`) with a `void *stream` member, not a positional `void *stream`, so the count that
tests/test_gpu_stream_order.py pins does not see them; this module keeps that module's promise for them, with its harness
(Chain, drive, the fixtures) and the chain pieces of tests/test_gpu_stream_order_edit.py, under the same rules: one
torch.cuda.Stream(), no host wait between calls, every host-side size from the references, models, dictionary and table built
beforehand, a second run behind the blocker.

  chain H   order 2 (case 088): dictionary search -> tagged spans -> masked re-code -> table-splicing re-code, each re-code
            indexed (count only and in full) and index-free, under an order-2 destination

Every expected value comes from the original messages (find_ref, edit_ref, splice_table_ref, batch_ref and the oracle's
codes), never from another call of the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import batch_ref
import edit_ref
import splice_table_ref
from conftest import ROOT
from test_gpu_stream_order import Chain, drive, env, gpu, ptr, same  # noqa: F401 (env: the fixture of the stream chains)
from test_gpu_stream_order_edit import Order2, add_edit, add_find_dict, add_spans, replacement_table

BLOCK_CALLS = 2                     # the mh_dev_* declarations of include/mh.h that take a block with a `void *stream` member


def block_calls():
    """The mh_dev_* declarations whose one parameter is a `const mh_*_args *` to a struct with a `void *stream` member."""
    with open(os.path.join(ROOT, "include", "mh.h")) as f:
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    structs = {m.group(3) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text)
               if re.search(r"\bvoid\s*\*\s*stream\s*;", m.group(2))}
    return [m.group(1) for m in re.finditer(r"\b(mh_dev_\w+)\s*\(\s*const\s+(mh_\w+_args)\s*\*\s*\w+\s*\)\s*;", text) if m.group(2) in structs]


def test_the_calls_that_take_a_block_are_the_two_and_both_are_driven_here():
    calls = block_calls()
    assert sorted(calls) == ["mh_dev_recode_edit_batch_o2", "mh_dev_recode_splice_table_batch_o2"] and len(calls) == BLOCK_CALLS, calls
    source = inspect.getsource(test_chain_h_order_2_scrubber)
    for c in calls:
        assert re.search(r"\blib\.%s\b(?!\w)" % c, source), "%s: no stream-order chain drives it" % c


@gpu
def test_chain_h_order_2_scrubber(env):
    mhc, lib = env.mhc, env.lib
    g = Order2(env, "chain H")
    ch, S, b, rs, e, msgs, n, total, c, p0 = g.ch, g.S, g.b, g.rs, g.e, g.msgs, g.n, g.total, g.c, g.p0
    edit = lambda *a: lib.mh_dev_recode_edit_batch_o2(C.byref(mhc.args_block(mhc.RecodeEditO2Args, *a)))
    table = lambda *a: lib.mh_dev_recode_splice_table_batch_o2(C.byref(mhc.args_block(mhc.RecodeSpliceO2Args, *a)))
    # the references: the tagged merge of all the dictionary's hits, the masked messages, a table and the spliced messages
    t_off, t_spans, t_tags = splice_table_ref.merge_tagged(e.hit_off, e.records, e.hit_pattern)
    edited = edit_ref.apply(msgs, t_off, t_spans, e.byte_map)
    rep_lens, rep_off, rep_bytes = replacement_table(g.case, t_tags, np.unique(np.frombuffer(g.joined, dtype=np.uint8)))
    reps = [rep_bytes[int(a):int(z)].tobytes() for a, z in zip(rep_off[:-1], rep_off[1:])]
    tabled = splice_table_ref.apply(msgs, t_off, t_spans, t_tags, reps)
    assert len(t_spans) > 100 and edited != msgs and tabled != msgs
    # an order-2 destination with a code for every triple of the three forms
    counts = batch_ref.histogram(msgs + edited + tabled, 2, p0)
    codes = batch_ref.oracle_codes(counts, 2)
    D = mhc.Model.from_counts(counts, 2)
    dic = mhc.Dict(e.dictionary, fold=e.fold)
    ch.keep += (D, dic)
    x_edit, x_table = batch_ref.pack(edited, *codes, 2, p0, c), batch_ref.pack(tabled, *codes, 2, p0, c)
    assert not x_edit.dropped.any() and not x_table.dropped.any()
    # 1. order-2 dictionary search, 2. its records merged into tagged spans
    hits = add_find_dict(ch, "find_dict_batch_o2", lib.mh_dev_find_dict_batch_o2, S.handle, dic, b, p0, total, g.d_in, g.d_idx, c, e)
    (d_mo, d_ms, d_mt), _ = add_spans(ch, "spans_from_hits", hits, len(e.hits), n, e)
    # 3. the masked re-code on the device spans
    d_map = ch.staged(np.frombuffer(e.byte_map, dtype=np.uint8))
    common = (S.handle, D.handle, b, p0, total, rs.sym_off)
    ws = lambda chunk: lib.mh_dev_recode_edit_batch_o2_workspace(n, total, chunk)
    mid = (ptr(d_mo), ptr(d_ms), ptr(d_map))
    add_edit(ch, "recode_edit_batch_o2 count only", edit, ws(c), *common, g.d_in, g.d_idx, c, mid, x_edit, full=False)
    add_edit(ch, "recode_edit_batch_o2", edit, ws(c), *common, g.d_in, g.d_idx, c, mid, x_edit)
    add_edit(ch, "recode_edit_batch_o2 index-free", edit, ws(0), *common, None, None, c, mid, x_edit)
    # 4. the table splice on the device spans and tags
    nt, nr = len(t_spans), len(rep_lens)
    ws = lambda chunk: lib.mh_dev_recode_splice_table_batch_o2_workspace(n, total, chunk, nt, nr)
    d_roff, d_rb = ch.staged(rep_off), ch.staged(rep_bytes)
    mid = (ptr(d_mo), ptr(d_ms), ptr(d_mt), ptr(d_roff), ptr(d_rb), nr)
    add_edit(ch, "recode_splice_table_batch_o2 count only", table, ws(c), *common, g.d_in, g.d_idx, c, mid, x_table, splice=True, full=False)
    add_edit(ch, "recode_splice_table_batch_o2", table, ws(c), *common, g.d_in, g.d_idx, c, mid, x_table, splice=True)
    add_edit(ch, "recode_splice_table_batch_o2 index-free", table, ws(0), *common, None, None, c, mid, x_table, splice=True)
    drive(ch)
