"""The rest of the stream-taking device calls on a non-default stream: tests/test_gpu_stream_order.py drives the older half of
include/mh.h's mh_dev_* family; this module drives the calls that came after it, with that module's harness (Chain, drive, Batch,
the add_* helpers, the env and one_stream fixtures) and under its rules: one torch.cuda.Stream(), no host wait between calls,
every host-side size from the references, models, dictionaries and tables built beforehand, a second run behind the blocker.

  chain E   the scrubber under a shared order-0/1 model (case 032): digests, dictionary search, spans from hits (plain and
            tagged), masked, splicing and table-splicing re-code, decode and digest of the spliced batch
  chain F   one model per stream (case 032, batch_ref.pack_each): encode, table files, segment states, and the _each forms of
            digest, dictionary search, masked, splicing and table-splicing re-code; bank selection
  chain G   order 2 (case 088): digest, dictionary search, segment states / index / emit, the two single-stream order-2
            histograms, byte ranges of one stream of the batch
  chain D2  one stream of 300 000 bytes: the order-0 histogram, every single-stream encoder, the decode forms with a fine index
            and with the payload length on the device

Every expected value comes from the original messages (batch_ref, find_ref, edit_ref, splice_ref, splice_table_ref, recode_ref,
zlib.crc32, the oracle), never from another call of the library.

In these chains search records, their patterns, span offsets, spans and span tags written by one call are the positions and
stream numbers of the next, so they are allocated with zeros (zeros() below), not with the 0xA5 fill: a record read before it
exists must stay in bounds.  Payloads, decoded bytes, replacement bytes, the byte map, digests, statuses and workspaces keep
the fill; a replacement table's offsets are uint64 and get zeros like every staged uint64 array.

mh_dev_batch_states_stats says that it synchronises: it is in the first module's EXEMPT and runs here once, without a blocker."""
import ctypes as C
import zlib

import numpy as np

import batch_ref
import edit_ref
import recode_ref
import splice_table_ref
import states_o2_ref
from oracle import mh_oracle
from test_gpu_stream_order import (CASES, FILL, Batch, Chain, add_decode_of_recoded, drive, env, gpu, one_stream,  # noqa: F401 (fixtures)
                                   packed_out_at, ptr, same)


def zeros(ch, nbytes):
    """Bytes written by one call of a chain and read by the next as positions, stream numbers or table numbers (hit offsets,
    records, patterns, span offsets, spans, tags; a fine index): prefilled with zeros, as Chain.words does for uint64 arrays."""
    return ch._alloc(nbytes, True)


def clear_behind(ch, d, used):
    """The 64 bytes behind the `used` bytes of a zeros() buffer are still zero."""
    return not ch.get(d)[used:used + 64].any()


def crcs(msgs):
    return np.array([zlib.crc32(m) & 0xFFFFFFFF for m in msgs], dtype=np.uint32), np.array([len(m) for m in msgs], dtype=np.uint64)


# ---- the pieces of the chains ---------------------------------------------------------------------------------------------
def add_crc(ch, tag, fn, handle, b, p0, total, d_sym_off, d_index, chunk, msgs):
    """Digests of a coded batch, indexed (d_index given) or index-free: zlib.crc32 and the length of every message."""
    lib, n = ch.env.lib, b.n
    want_crc, want_len = crcs(msgs)
    indexed = d_index is not None
    wsb = lib.mh_dev_crc_batch_workspace(n, total, chunk if indexed else 0)
    d_ws, d_crc, d_len, d_st = ch.work(wsb), ch.out(n * 4 + 64), ch.out(n * 8 + 64), ch.status(n, tag)
    ch.call(tag, fn, handle, *b.args(), p0, ptr(d_sym_off) if indexed else None, total if indexed else 0, ptr(d_index), chunk if indexed else 0,
            ptr(d_crc), ptr(d_len), ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": crc", lambda: same(ch.get(d_crc, np.uint32, n), want_crc) and (ch.get(d_crc)[n * 4:n * 4 + 64] == FILL).all())
    ch.expect(tag + ": len", lambda: same(ch.get(d_len, np.uint64, n), want_len) and (ch.get(d_len)[n * 8:n * 8 + 64] == FILL).all())


def add_find_dict(ch, tag, fn, handle, dic, b, p0, total, d_sym_off, d_index, chunk, e):
    """Dictionary search, count only and then with records; the hit capacity is the reference's number of hits.  Returns the
    device hit offsets, records and patterns of the second call, all three prefilled with zeros."""
    lib, n, k = ch.env.lib, b.n, len(e.hits)
    wsb = lib.mh_dev_find_dict_workspace(n, total, chunk)
    res = None
    for records in (False, True):
        t = tag + (" records" if records else " count only")
        d_ws, d_ho, d_st = ch.work(wsb), zeros(ch, (n + 1) * 8), ch.status(n, t)
        d_rec, d_pat = (zeros(ch, k * 24 + 64), zeros(ch, k * 4 + 64)) if records else (None, None)
        ch.call(t, fn, handle, dic.handle, *b.args(), p0, ptr(d_sym_off), total, ptr(d_index), chunk, ptr(d_ho), ptr(d_rec), ptr(d_pat),
                k if records else 0, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
        ch.expect(t + ": hit_off", lambda d_ho=d_ho: same(ch.get(d_ho, np.uint64, n + 1), e.hit_off))
        if records:
            ch.expect(t + ": records", lambda d_rec=d_rec: same(ch.get(d_rec, np.uint64, 3 * k).reshape(-1, 3), e.records) and clear_behind(ch, d_rec, k * 24))
            ch.expect(t + ": patterns", lambda d_pat=d_pat: same(ch.get(d_pat, np.uint32, k), e.hit_pattern) and clear_behind(ch, d_pat, k * 4))
            res = d_ho, d_rec, d_pat
    return res


def add_spans(ch, tag, hits, k, n, e):
    """mh_dev_spans_from_hits and _tagged on the device records of a search (hits = add_find_dict's result, k its hit_cap):
    edit_ref.merge_hits and splice_table_ref.merge_tagged of the reference records.  Returns the tagged call's span offsets,
    spans and tags (device, zeros) and the reference's (span_off, spans, tags)."""
    lib = ch.env.lib
    d_ho, d_rec, d_pat = hits
    want_off, want = edit_ref.merge_hits(e.hit_off, e.records)
    t_off, t_spans, t_tags = splice_table_ref.merge_tagged(e.hit_off, e.records, e.hit_pattern)
    m = len(want)
    assert same(want_off, t_off) and same(want, t_spans), "the two reference merges give the same spans"
    wsb = lib.mh_dev_spans_from_hits_workspace(n, k)
    d_ws, d_so, d_sp = ch.work(wsb), zeros(ch, (n + 1) * 8), zeros(ch, k * 16 + 64)
    ch.call(tag, lib.mh_dev_spans_from_hits, ptr(d_ho), ptr(d_rec), k, n, ptr(d_so), ptr(d_sp), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": span_off", lambda: same(ch.get(d_so, np.uint64, n + 1), want_off))
    ch.expect(tag + ": spans", lambda: same(ch.get(d_sp, np.uint64, 2 * m).reshape(-1, 2), want) and clear_behind(ch, d_sp, m * 16))
    wsb = lib.mh_dev_spans_from_hits_tagged_workspace(n, k)
    d_ws, d_so2, d_sp2, d_tg = ch.work(wsb), zeros(ch, (n + 1) * 8), zeros(ch, k * 16 + 64), zeros(ch, k * 4 + 64)
    ch.call(tag + " tagged", lib.mh_dev_spans_from_hits_tagged, ptr(d_ho), ptr(d_rec), ptr(d_pat), k, n, ptr(d_so2), ptr(d_sp2), ptr(d_tg),
            ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + " tagged: span_off", lambda: same(ch.get(d_so2, np.uint64, n + 1), t_off))
    ch.expect(tag + " tagged: spans", lambda: same(ch.get(d_sp2, np.uint64, 2 * m).reshape(-1, 2), t_spans) and clear_behind(ch, d_sp2, m * 16))
    ch.expect(tag + " tagged: tags", lambda: same(ch.get(d_tg, np.uint32, m), t_tags) and clear_behind(ch, d_tg, m * 4))
    return (d_so2, d_sp2, d_tg), (t_off, t_spans, t_tags)


def add_edit(ch, tag, fn, wsb, src, dst, b, p0, total, src_sym_off, d_sym_off, d_index, chunk, mid, ref, splice=False, full=True):
    """One masked (splice False), splicing or table-splicing (splice True) re-code: the arguments that the three share around
    `mid`, the call's own (span list and map, replacement or table).  ref: batch_ref.Packed of the edited messages under the
    destination model.  Indexed (d_index given; d_sym_off is input) or index-free (d_sym_off None: the source's sym_off is
    written and compared).  full: exactly the reference's payload bytes of room and the index; else count only.  Returns the
    re-coded batch, its index and (splice) its out_sym_off on the device."""
    lib, n = ch.env.lib, b.n
    indexed = d_index is not None
    cap, out_total = int(ref.pay_off[n]), int(ref.sym_off[n])
    nidx = int(lib.mh_batch_index_capacity(out_total, n, chunk))
    d_ws, d_st = ch.work(wsb), ch.status(n, tag)
    d_so = d_sym_off if indexed else ch.words(n + 1)
    d_oo, d_onb, d_dr = ch.words(n + 1), ch.words(n), ch.words(n)
    d_out, d_oi = (ch.out(cap + 64), ch.words(nidx)) if full else (None, None)
    d_oso = ch.words(n + 1) if splice else None
    tail = (ptr(d_out), cap, ptr(d_oo), ptr(d_onb)) + ((ptr(d_oso), ptr(d_oi), nidx if full else 0) if splice else (ptr(d_oi),))
    ch.call(tag, fn, src, dst, *b.args(), p0, ptr(d_so), total, ptr(d_index), chunk, *mid, *tail, ptr(d_dr), ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": offsets, nbits, dropped", lambda: same(ch.get(d_oo, np.uint64, n + 1), ref.pay_off) and same(ch.get(d_onb, np.uint64, n), ref.nbits)
              and same(ch.get(d_dr, np.uint64, n), ref.dropped))
    if splice:
        ch.expect(tag + ": out_sym_off", lambda: same(ch.get(d_oso, np.uint64, n + 1), ref.sym_off))
    if not indexed:
        ch.expect(tag + ": sym_off of the source", lambda: same(ch.get(d_so, np.uint64, n + 1), src_sym_off))
    if full:
        ch.expect(tag + ": payload", lambda: same(ch.get(d_out, np.uint8, cap), ref.payload) and (ch.get(d_out)[cap:cap + 64] == FILL).all())
        ch.expect(tag + ": index slices", lambda: same(ref.slices_of(ch.get(d_oi, np.uint64, nidx), chunk), ref.all_slices()))
    return Batch(d_out, d_oo, d_onb, n, cap), d_oi, d_oso


def replacement_table(case, tags, alphabet):
    """A replacement table with an entry for every tag of the reference merge, from a generator of its own: (lengths, offsets,
    bytes).  Most entries have 0 to 3 bytes; the four lengths 0, 1, a mid-size one and 255 go to the four used tags with the
    fewest spans (a 255-byte entry at a frequent tag would only make the reference slow).  The bytes are bytes of the messages,
    so the destination model of the case has a code for every pair of a spliced message that it has for the messages."""
    rng = np.random.default_rng([case.seed, 2])
    n_reps = max(4, int(tags.max()) + 1 if tags.size else 0)
    lens = rng.integers(0, 4, size=n_reps)
    used, count = np.unique(tags, return_counts=True)
    four = used[np.argsort(count, kind="stable")][:4] if used.size >= 4 else np.arange(4)
    lens[four] = (0, 1, int(rng.integers(16, 129)), 255)
    off = np.zeros(n_reps + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    data = rng.choice(alphabet, size=int(off[-1])).astype(np.uint8)
    assert {0, 1, 255} <= set(lens.tolist()) and any(16 <= v <= 128 for v in lens.tolist()) and lens.max() <= 255
    return lens, off, data


class Scrub:
    """What chains E and F share: case 032's world, edits, expectations, destination model and the table splice's inputs."""

    def __init__(self, env):
        mhc = env.mhc
        self.case = case = CASES[32]
        assert case.id == "032-uniform-deep1-deep0-c1024-n65"
        self.w, self.e, self.x = case.world(), case.edits(), case.expected()
        self.order, self.do = case.orders
        w = self.w
        self.msgs, self.p0, self.c = w.messages, w.prev0, case.chunk
        self.n, self.joined = len(w.messages), b"".join(w.messages)
        self.total = len(self.joined)
        dc, dl = case.counts("dst")
        self.D = mhc.Model.from_counts(dc, self.do, max_len=dl)
        self.D_oracle = mh_oracle.Model.from_counts(dc, self.do)
        self.dic = mhc.Dict(self.e.dictionary, fold=self.e.fold)
        # the table splice: the reference's tagged merge of all the dictionary's hits, a table with an entry for every tag
        self.t_off, self.t_spans, self.t_tags = splice_table_ref.merge_tagged(self.e.hit_off, self.e.records, self.e.hit_pattern)
        self.rep_lens, self.rep_off, self.rep_bytes = replacement_table(case, self.t_tags, np.unique(np.frombuffer(self.joined, dtype=np.uint8)))
        reps = [self.rep_bytes[int(a):int(b)].tobytes() for a, b in zip(self.rep_off[:-1], self.rep_off[1:])]
        self.tabled = splice_table_ref.apply(self.msgs, self.t_off, self.t_spans, self.t_tags, reps)
        self.table = batch_ref.pack(self.tabled, *case.codes("dst"), self.do, self.p0, self.c)
        if self.p0 == recode_ref.PREV0 and not dl:                # the same from the oracle's own encoder (it starts in PREV0)
            pl, off, nb, dr = recode_ref.packed(recode_ref.recode(self.tabled, self.D_oracle, self.c))
            assert same(pl, self.table.payload) and same(off, self.table.pay_off) and same(nb, self.table.nbits) and same(dr, self.table.dropped)
        self.same_spans = same(self.t_off, self.e.span_off) and same(self.t_spans, self.e.spans)
        print("case 032: %d hits, %d merged spans with %d tags, a table of %d entries (%d bytes); the edit and the splice take %s" % (
            len(self.e.hits), len(self.t_spans), len(set(self.t_tags.tolist())), len(self.rep_lens), self.rep_bytes.size,
            "the device spans of the merge" if self.same_spans else "the case's own span list, staged (it is not the merge of all hits)"))

    def add_recodes(self, ch, kind, src, b, d_in, d_idx, spans, merged, fns):
        """Masked, splicing and table-splicing re-code of the source batch b (kind: "batch" or "each"): each indexed, count
        only and in full, and one of each kind index-free.  spans: the device (span_off, spans) of the case's list; merged: the
        device (span_off, spans, tags) of the tagged merge.  Returns the table splice's batch, index and out_sym_off."""
        lib, e, x, n, total, c, p0, D = ch.env.lib, self.e, self.x, self.n, self.total, self.c, self.p0, self.D.handle
        edit, splice, table = fns
        d_so, d_sp = spans
        d_map = ch.staged(np.frombuffer(e.byte_map, dtype=np.uint8))
        rs_sym_off = splice_table_ref.offsets(self.msgs)
        ns, nt, nr = len(e.spans), len(self.t_spans), len(self.rep_lens)
        ws_edit = lambda chunk: lib.mh_dev_recode_edit_workspace(n, total, chunk)
        ws_splice = lambda chunk: lib.mh_dev_recode_splice_workspace(n, total, chunk, ns)
        ws_table = lambda chunk: lib.mh_dev_recode_splice_table_workspace(n, total, chunk, nt, nr)
        common = (src, D, b, p0, total, rs_sym_off)
        # masked re-code: count only, in full, everywhere (span_off NULL), index-free
        mid = (ptr(d_so), ptr(d_sp), ptr(d_map))
        add_edit(ch, "recode_edit_%s count only" % kind, edit, ws_edit(c), *common, d_in, d_idx, c, mid, x.edit, full=False)
        add_edit(ch, "recode_edit_%s" % kind, edit, ws_edit(c), *common, d_in, d_idx, c, mid, x.edit)
        add_edit(ch, "recode_edit_%s everywhere" % kind, edit, ws_edit(c), *common, d_in, d_idx, c, (None, None, ptr(d_map)), x.edit_all)
        add_edit(ch, "recode_edit_%s index-free" % kind, edit, ws_edit(0), *common, None, None, c, mid, x.edit)
        # splicing re-code with the deletion and the replacement: count only and in full; the replacement index-free as well
        for k, rep in enumerate(e.reps):
            d_rep = ch.staged(np.frombuffer(rep, dtype=np.uint8)) if rep else None
            mid = (ptr(d_so), ptr(d_sp), ptr(d_rep), len(rep))
            t = "recode_splice_%s of %d bytes" % (kind, len(rep))
            assert same(x.splice[k].sym_off, x.out_sym_off[k])
            add_edit(ch, t + " count only", splice, ws_splice(c), *common, d_in, d_idx, c, mid, x.splice[k], splice=True, full=False)
            add_edit(ch, t, splice, ws_splice(c), *common, d_in, d_idx, c, mid, x.splice[k], splice=True)
            if rep:
                add_edit(ch, t + " index-free", splice, ws_splice(0), *common, None, None, c, mid, x.splice[k], splice=True)
        # table-splicing re-code on the merge's device spans and tags
        d_mo, d_ms, d_mt = merged
        d_roff, d_rb = ch.staged(self.rep_off), ch.staged(self.rep_bytes)
        mid = (ptr(d_mo), ptr(d_ms), ptr(d_mt), ptr(d_roff), ptr(d_rb), nr)
        t = "recode_splice_table_%s" % kind
        add_edit(ch, t + " count only", table, ws_table(c), *common, d_in, d_idx, c, mid, self.table, splice=True, full=False)
        res = add_edit(ch, t, table, ws_table(c), *common, d_in, d_idx, c, mid, self.table, splice=True)
        add_edit(ch, t + " index-free", table, ws_table(0), *common, None, None, c, mid, self.table, splice=True)
        return res


# ---- chain E: the scrubber under a shared order-0/1 model -------------------------------------------------------------------
@gpu
def test_chain_e_scrubber_shared_order_0_1(env):
    mhc, lib = env.mhc, env.lib
    s = Scrub(env)
    case, e, msgs, n, total, c, p0 = s.case, s.e, s.msgs, s.n, s.total, s.c, s.p0
    sc, sl = case.counts("src")
    S = mhc.Model.from_counts(sc, s.order, max_len=sl)
    rs = batch_ref.pack(msgs, *case.codes("src"), s.order, p0, c)
    ch = Chain(env, "chain E")
    ch.keep = (S, s)
    d_data, d_in = ch.staged(np.frombuffer(s.joined, dtype=np.uint8)), ch.staged(rs.sym_off)
    b = Batch(ch.staged(np.concatenate([rs.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(rs.pay_off), ch.staged(rs.nbits), n, int(rs.pay_off[n]))
    d_idx = ch.staged(rs.index_array(c))
    # 1. digests: of the messages, and of the coded batch with and without its index
    wsb = lib.mh_dev_crc_raw_batch_workspace(n, total)
    d_ws, d_crc = ch.work(wsb), ch.out(n * 4 + 64)
    ch.call("crc_raw_batch", lib.mh_dev_crc_raw_batch, ptr(d_data), ptr(d_in), n, total, ptr(d_crc), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("crc_raw_batch", lambda: same(ch.get(d_crc, np.uint32, n), crcs(msgs)[0]) and (ch.get(d_crc)[n * 4:n * 4 + 64] == FILL).all())
    add_crc(ch, "crc_batch indexed", lib.mh_dev_crc_batch, S.handle, b, p0, total, d_in, d_idx, c, msgs)
    add_crc(ch, "crc_batch index-free", lib.mh_dev_crc_batch, S.handle, b, p0, total, None, None, 0, msgs)
    # 2. dictionary search, 3. its records merged into spans and tagged spans
    hits = add_find_dict(ch, "find_dict_batch", lib.mh_dev_find_dict_batch, S.handle, s.dic, b, p0, total, d_in, d_idx, c, e)
    merged, _ = add_spans(ch, "spans_from_hits", hits, len(e.hits), n, e)
    # 4. - 6. the three re-codes; the edit and the splice on the case's span list (see Scrub), the table splice on the merge
    spans = merged[:2] if s.same_spans else (ch.staged(e.span_off), ch.staged(e.spans))
    fns = (lib.mh_dev_recode_edit_batch, lib.mh_dev_recode_splice_batch, lib.mh_dev_recode_splice_table_batch)
    tb, d_oi, d_oso = s.add_recodes(ch, "batch", S.handle, b, d_in, d_idx, spans, merged, fns)
    # 7. the table splice's output decoded under the destination model through the index it wrote, and digested
    out_total = int(s.table.sym_off[n])
    add_decode_of_recoded(ch, "decode_batch of the table splice", env, s.D, s.D_oracle, tb, d_oi, d_oso, p0, out_total, c, s.table, s.tabled)
    if not s.table.dropped.any():                                  # (a stream that dropped a symbol does not decode to its message)
        add_crc(ch, "crc_batch of the table splice", lib.mh_dev_crc_batch, s.D.handle, tb, p0, out_total, d_oso, d_oi, c, s.tabled)
    drive(ch)


# ---- chain F: one model per stream -------------------------------------------------------------------------------------------
@gpu
def test_chain_f_scrubber_one_model_per_stream(env):
    mhc, lib = env.mhc, env.lib
    s = Scrub(env)
    case, e, msgs, n, total, c, p0, order = s.case, s.e, s.msgs, s.n, s.total, s.c, s.p0, s.order
    re, tables = batch_ref.pack_each(msgs, order, p0, c)
    ms = mhc.ModelSet.from_tables(tables)                          # (mh_dev_encode_each takes a set: built beforehand by the host form)
    ch = Chain(env, "chain F")
    ch.keep = (ms, s)
    d_data, d_in = ch.staged(np.frombuffer(s.joined, dtype=np.uint8)), ch.staged(re.sym_off)
    pay_total, nidx = int(re.pay_off[n]), int(lib.mh_batch_index_capacity(total, n, c))
    # encode every message under its own model: the batch that the rest of the chain reads
    cap = lib.mh_encode_each_bound(ms.handle, total, n)
    assert cap >= pay_total
    wsb = lib.mh_dev_encode_each_workspace(n, total)
    d_ws, d_pl, d_po, d_nb, d_idx = ch.work(wsb), ch.out(cap + 64), ch.words(n + 1), ch.words(n), ch.words(nidx)
    ch.call("encode_each", lib.mh_dev_encode_each, ms.handle, ptr(d_data), ptr(d_in), n, total, p0, ptr(d_pl), cap, ptr(d_po), ptr(d_nb), ptr(d_idx), c,
            ptr(d_ws), wsb, ws=d_ws)
    ch.expect("encode_each: offsets, nbits", lambda: same(ch.get(d_po, np.uint64, n + 1), re.pay_off) and same(ch.get(d_nb, np.uint64, n), re.nbits))
    ch.expect("encode_each: payload", lambda: same(ch.get(d_pl, np.uint8, pay_total), re.payload) and (ch.get(d_pl)[cap:] == FILL).all())
    ch.expect("encode_each: index slices", lambda: same(re.slices_of(ch.get(d_idx, np.uint64, nidx), c), re.all_slices()))
    b = Batch(d_pl, d_po, d_nb, n, pay_total)
    # the set's table files
    tcap, wsb = lib.mh_model_set_tables_bound(ms.handle), lib.mh_dev_model_set_tables_workspace(ms.handle)
    tab_off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.uint64)
    assert tcap >= int(tab_off[n])
    d_ws, d_tab, d_to = ch.work(wsb), ch.out(tcap + 64), ch.words(n + 1)
    ch.call("model_set_tables", lib.mh_dev_model_set_tables, ms.handle, ptr(d_tab), tcap, ptr(d_to), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("model_set_tables: offsets", lambda: same(ch.get(d_to, np.uint64, n + 1), tab_off))
    ch.expect("model_set_tables: tables", lambda: ch.get(d_tab, np.uint8, int(tab_off[n])).tobytes() == b"".join(tables) and (ch.get(d_tab)[tcap:] == FILL).all())
    # segment states of the batch taken as index-free, then its index and bytes from them
    wsb = lib.mh_dev_batch_states_workspace(n, pay_total)
    d_ws, d_so, d_idx2, d_out = ch.work(wsb), ch.words(n + 1), ch.words(nidx), ch.out(total + 64)
    st = [ch.status(n, "each_" + k) for k in ("states", "index", "emit")]
    ch.call("each_states", lib.mh_dev_each_states, ms.handle, *b.args(), p0, ptr(d_so), ptr(st[0]), ptr(d_ws), wsb, ws=d_ws)
    ch.call("each_index", lib.mh_dev_each_index, ms.handle, *b.args(), p0, ptr(d_idx2), nidx, c, ptr(st[1]), ptr(d_ws), wsb)
    ch.call("each_emit", lib.mh_dev_each_emit, ms.handle, *b.args(), p0, ptr(d_out), total, ptr(st[2]), ptr(d_ws), wsb)
    ch.expect("each_states: sym_off", lambda: same(ch.get(d_so, np.uint64, n + 1), re.sym_off))
    ch.expect("each_index: slices", lambda: same(re.slices_of(ch.get(d_idx2, np.uint64, nidx), c), re.all_slices()))
    ch.expect("each_emit: bytes", lambda: ch.get(d_out, np.uint8, total).tobytes() == s.joined and (ch.get(d_out)[total:total + 64] == FILL).all())
    # the scrubber on the per-stream-model batch: the expectations of chain E
    add_crc(ch, "crc_each indexed", lib.mh_dev_crc_each, ms.handle, b, p0, total, d_in, d_idx, c, msgs)
    add_crc(ch, "crc_each index-free", lib.mh_dev_crc_each, ms.handle, b, p0, total, None, None, 0, msgs)
    hits = add_find_dict(ch, "find_dict_each", lib.mh_dev_find_dict_each, ms.handle, s.dic, b, p0, total, d_in, d_idx, c, e)
    merged, _ = add_spans(ch, "spans_from_hits (of find_dict_each)", hits, len(e.hits), n, e)
    spans = merged[:2] if s.same_spans else (ch.staged(e.span_off), ch.staged(e.spans))
    fns = (lib.mh_dev_recode_edit_each, lib.mh_dev_recode_splice_each, lib.mh_dev_recode_splice_table_each)
    s.add_recodes(ch, "each", ms.handle, b, d_in, d_idx, spans, merged, fns)
    # bank selection of the messages: the bank that the fuzz rig's bank() draws
    drawn = [(1, msgs[:(n + 1) // 2]), (0, s.w.foreign), (order, msgs[::3]), (order, msgs)]
    counts = [(o, batch_ref.histogram(m, o, p0)) for o, m in drawn]
    bank = mhc.ModelSet.from_models([mhc.Model.from_counts(h, o) for o, h in counts])
    ch.keep += (bank,)
    want_c, want_n = batch_ref.select([(o, batch_ref.oracle_codes(h, o)[0]) for o, h in counts], msgs, p0)
    wsb = lib.mh_dev_bank_select_workspace(len(drawn), n, total)
    d_ws, d_choice, d_bits = ch.work(wsb), ch.out(n * 4 + 64), ch.out(n * 8 + 64)
    ch.call("bank_select", lib.mh_dev_bank_select, bank.handle, ptr(d_data), ptr(d_in), n, total, p0, ptr(d_choice), ptr(d_bits), ptr(d_ws), wsb, ws=d_ws)
    ch.expect("bank_select: choices", lambda: same(ch.get(d_choice, np.uint32, n), want_c) and (ch.get(d_choice)[n * 4:n * 4 + 64] == FILL).all())
    ch.expect("bank_select: nbits", lambda: same(ch.get(d_bits, np.uint64, n), want_n) and (ch.get(d_bits)[n * 8:n * 8 + 64] == FILL).all())
    drive(ch)


# ---- chain G: order 2 ------------------------------------------------------------------------------------------------------
class Order2:
    """Case 088 under its shared order-2 source model: the reference's batch, staged."""

    def __init__(self, env, name):
        mhc = env.mhc
        self.case = case = CASES[88]
        assert case.id == "088-text-own2-foreign1-c1024-n257" and case.orders[0] == 2
        self.w, self.e = case.world(), case.edits()
        w = self.w
        self.msgs, self.p0, self.c = w.messages, w.prev0, case.chunk
        self.n, self.joined = len(w.messages), b"".join(w.messages)
        self.total = len(self.joined)
        sc, _ = case.counts("src")
        self.S = mhc.Model.from_counts(sc, 2)
        self.rs = rs = batch_ref.pack(self.msgs, *case.codes("src"), 2, self.p0, self.c)
        self.ch = ch = Chain(env, name)
        ch.keep = (self.S,)
        self.d_in, self.d_idx = ch.staged(rs.sym_off), ch.staged(rs.index_array(self.c))
        self.b = Batch(ch.staged(np.concatenate([rs.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(rs.pay_off), ch.staged(rs.nbits), self.n,
                       int(rs.pay_off[self.n]))

    def add_states(self):
        """mh_dev_batch_states_o2 on the batch taken as index-free: sym_off of the reference.  Returns the workspace."""
        ch, lib, b, n = self.ch, self.ch.env.lib, self.b, self.n
        self.wsb = lib.mh_dev_batch_states_o2_workspace(n, b.pay_total)
        d_ws, d_so, d_st = ch.work(self.wsb), ch.words(n + 1), ch.status(n, "batch_states_o2")
        ch.call("batch_states_o2", lib.mh_dev_batch_states_o2, self.S.handle, *b.args(), self.p0, ptr(d_so), ptr(d_st), ptr(d_ws), self.wsb, ws=d_ws)
        ch.expect("batch_states_o2: sym_off", lambda: same(ch.get(d_so, np.uint64, n + 1), self.rs.sym_off))
        return d_ws


@gpu
def test_chain_g_order_2(env):
    mhc, lib = env.mhc, env.lib
    g = Order2(env, "chain G")
    ch, S, b, rs, e, msgs, n, total, c, p0 = g.ch, g.S, g.b, g.rs, g.e, g.msgs, g.n, g.total, g.c, g.p0
    # digests and dictionary search of the order-2 batch
    add_crc(ch, "crc_batch_o2 indexed", lib.mh_dev_crc_batch_o2, S.handle, b, p0, total, g.d_in, g.d_idx, c, msgs)
    add_crc(ch, "crc_batch_o2 index-free", lib.mh_dev_crc_batch_o2, S.handle, b, p0, total, None, None, 0, msgs)
    dic = mhc.Dict(e.dictionary, fold=e.fold)
    ch.keep += (dic,)
    add_find_dict(ch, "find_dict_batch_o2", lib.mh_dev_find_dict_batch_o2, S.handle, dic, b, p0, total, g.d_in, g.d_idx, c, e)
    # segment states, then index and emit from them
    d_ws = g.add_states()
    nidx = int(lib.mh_batch_index_capacity(total, n, c))
    d_idx2, d_out = ch.words(nidx), ch.out(total + 64)
    st = [ch.status(n, "batch_%s_o2" % k) for k in ("index", "emit")]
    ch.call("batch_index_o2", lib.mh_dev_batch_index_o2, S.handle, *b.args(), p0, ptr(d_idx2), nidx, c, ptr(st[0]), ptr(d_ws), g.wsb)
    ch.call("batch_emit_o2", lib.mh_dev_batch_emit_o2, S.handle, *b.args(), p0, ptr(d_out), total, ptr(st[1]), ptr(d_ws), g.wsb)
    ch.expect("batch_index_o2: slices", lambda: same(rs.slices_of(ch.get(d_idx2, np.uint64, nidx), c), rs.all_slices()))
    ch.expect("batch_emit_o2: bytes", lambda: ch.get(d_out, np.uint8, total).tobytes() == g.joined and (ch.get(d_out)[total:total + 64] == FILL).all())
    # the single-stream order-2 histograms of the concatenated messages, without and with the workspace
    d_data = ch.staged(np.frombuffer(g.joined, dtype=np.uint8))
    want = batch_ref.histogram([g.joined], 2, p0)
    ctx0 = p0 << 8 | p0
    d_c1, d_c2 = ch.out(want.size * 8), ch.out(want.size * 8)
    ch.call("histogram_o2", lib.mh_dev_histogram_o2, ptr(d_data), total, ctx0, ptr(d_c1))
    wsb = lib.mh_dev_histogram_o2_workspace(total)
    d_hws = ch.work(wsb)
    ch.call("histogram_o2_ws", lib.mh_dev_histogram_o2_ws, ptr(d_data), total, ctx0, ptr(d_c2), ptr(d_hws), wsb)
    ch.expect("histogram_o2", lambda: same(ch.get(d_c1, np.uint64, want.size), want))
    ch.expect("histogram_o2_ws", lambda: same(ch.get(d_c2, np.uint64, want.size), want))
    # byte ranges of one stream of the batch: the stream that most of the case's lookups name, its payload and index slice
    # inside the batch (host arithmetic on the reference's offsets)
    named = [i for i, _, _ in g.w.lookups]
    i = max(set(named), key=lambda k: (named.count(k), -k))
    ranges = np.array([(a, t) for k, a, t in g.w.lookups if k == i], dtype=np.uint64)
    assert len(ranges) >= 2 and len(msgs[i]) > c, "ranges in a stream of more than one chunk"
    ln = ranges[:, 1] - ranges[:, 0]
    size = int(ln.sum())
    d_rg, d_at = ch.staged(ranges), ch.staged(packed_out_at(ln))
    wsb = lib.mh_dev_decode_ranges_o2_workspace(len(ranges))
    d_ws, d_rout, d_st = ch.work(wsb), ch.out(size + 64), ch.status(len(ranges), "decode_ranges_o2")
    at, end = int(rs.pay_off[i]), int(rs.pay_off[i + 1])
    base = int(rs.sym_off[i]) // c + i
    ch.call("decode_ranges_o2", lib.mh_dev_decode_ranges_o2, S.handle, C.c_void_p(b.pl.data_ptr() + at), 0, end - at, int(rs.nbits[i]),
            C.c_void_p(g.d_idx.data_ptr() + 8 * base), c, len(msgs[i]), None, ptr(d_rg), len(ranges), ptr(d_rout), ptr(d_at), size, ptr(d_st),
            ptr(d_ws), wsb, ws=d_ws)
    want_bytes = b"".join(msgs[i][int(a):int(t)] for a, t in ranges)
    ch.expect("decode_ranges_o2", lambda: ch.get(d_rout, np.uint8, size).tobytes() == want_bytes and (ch.get(d_rout)[size:size + 64] == FILL).all())
    drive(ch)


@gpu
def test_exempt_states_stats_on_the_stream(env):
    """mh_dev_batch_states_stats (it says that it synchronises: EXEMPT of tests/test_gpu_stream_order.py) once on the stream,
    without a blocker, behind mh_dev_batch_states_o2 of case 088.  The figures depend on how the kernel decodes the bits past a
    payload's end, so they are not pinned to the CPU model of tests/states_o2_ref.py, which is printed beside them; the bounds
    are the repair launches there are and tests/test_gpu_batch_states_o2.py's "at most 1 stream in 20 left to the walk"."""
    lib = env.lib
    g = Order2(env, "states for the stats")
    d_ws = g.add_states()
    g.ch.run()
    g.ch.verify("the states call")
    passes, walked = C.c_uint32(99), C.c_uint64(1 << 40)
    assert lib.mh_dev_batch_states_stats(ptr(d_ws), env.sp, C.byref(passes), C.byref(walked)) == 0, "mh_dev_batch_states_stats"
    model = states_o2_ref.run(g.msgs, "recover", g.p0)
    print("case 088: %d streams, repair passes that did work %d, streams walked %d (the CPU model: wrong entries %s, walked %d)" % (
        g.n, passes.value, walked.value, model["wrong"], model["walked"]))
    assert passes.value <= states_o2_ref.REPAIR_PASSES and walked.value * 20 <= g.n
    # a workspace without states is refused
    blank = env.torch.zeros(4096, dtype=env.torch.uint8, device="cuda")
    env.torch.cuda.synchronize()
    assert lib.mh_dev_batch_states_stats(ptr(blank), env.sp, C.byref(passes), C.byref(walked)) == env.mhc.MH_ERR_ARG


# ---- chain D2: the other single-stream calls -----------------------------------------------------------------------------------
@gpu
def test_chain_d2_one_stream(env, one_stream):
    lib, o = env.lib, one_stream
    m, data, n, nbits, c, p0 = o["model"], o["data"], o["data"].size, o["nbits"], 1024, batch_ref.PREV0
    pay_bytes, n_idx, n_fine = (nbits + 7) // 8, (n + c - 1) // c, (n + 63) // 64
    lens = batch_ref.oracle_codes(o["counts"], 1)[0]
    sym = data.astype(np.int64)
    prev = np.concatenate([[p0], sym[:-1]])
    pos = np.concatenate([[0], np.cumsum(lens[prev * 256 + sym])[:-1]])
    at = np.arange(0, n, 64)
    fine = ((prev[at] << 24) | (pos[at] & 0xFFFFFF)).astype(np.uint32)      # (mh.h, FINE INDEX: context << 24 | low 24 bits of the offset)
    ch = Chain(env, "chain D2")
    d_data = ch.staged(data)
    # the order-0 histogram
    d_c0 = ch.out(256 * 8 + 64)
    ch.call("histogram_o0", lib.mh_dev_histogram_o0, ptr(d_data), n, ptr(d_c0), None, 0)
    ch.expect("histogram_o0", lambda: same(ch.get(d_c0, np.uint64, 256), np.bincount(data, minlength=256)) and (ch.get(d_c0)[2048:] == FILL).all())
    # the order-1 histogram with its full workspace: what mh_dev_encode_fine prices its regions from
    hwsb = lib.mh_dev_histogram_workspace(n)
    d_hws, d_counts = ch.work(hwsb), ch.out(65536 * 8)
    ch.call("histogram_o1", lib.mh_dev_histogram_o1, ptr(d_data), n, p0, ptr(d_counts), ptr(d_hws), hwsb, ws=d_hws)
    ch.expect("histogram_o1", lambda: same(ch.get(d_counts, np.uint64, 65536), o["counts"]))
    # every encoder: the oracle's payload, bit count and chunk index, and the fine index where the call writes one
    cap, wsb = lib.mh_encode_bound(m.handle, n), lib.mh_dev_encode_workspace(n)
    assert cap >= pay_bytes
    made = {}

    def encode(tag, fn, head, with_fine, tail=()):
        d_ws, d_pl, d_nb, d_idx = ch.work(wsb), ch.out(cap + 64), ch.words(1), ch.words(n_idx)
        d_fine = zeros(ch, n_fine * 4 + 64) if with_fine else None
        ch.call(tag, fn, m.handle, ptr(d_data), n, *head, ptr(d_pl), cap, ptr(d_nb), ptr(d_idx), c, *((ptr(d_fine),) if with_fine else ()), *tail,
                ptr(d_ws), wsb, ws=d_ws)
        ch.expect(tag + ": nbits", lambda: int(ch.get(d_nb, np.uint64, 1)[0]) == nbits)
        ch.expect(tag + ": payload", lambda: same(ch.get(d_pl, np.uint8, pay_bytes), o["payload"]) and (ch.get(d_pl)[cap:] == FILL).all())
        ch.expect(tag + ": index", lambda: same(ch.get(d_idx, np.uint64, n_idx), o["index"]))
        if with_fine:
            ch.expect(tag + ": fine index", lambda: same(ch.get(d_fine, np.uint32, n_fine), fine) and clear_behind(ch, d_fine, n_fine * 4))
        made[tag] = d_pl, d_nb, d_idx, d_fine

    encode("encode", lib.mh_dev_encode, (p0,), False)
    encode("encode_at", lib.mh_dev_encode_at, (p0, None), False)
    encode("encode_ctx", lib.mh_dev_encode_ctx, (p0, None), False)
    encode("encode_fine", lib.mh_dev_encode_fine, (p0, None), True, (ptr(d_hws), hwsb))
    encode("encode_fine without a histogram", lib.mh_dev_encode_fine, (p0, None), True, (None, 0))
    encode("encode_ctx_fine", lib.mh_dev_encode_ctx_fine, (p0, None), True)
    # decode with the fine index (payload length as a host value, then read on the device), and with the length on the device
    dwsb = lib.mh_dev_decode_workspace(nbits, n, c)

    def decode(tag, call):
        d_ws, d_out = ch.work(dwsb), ch.out(n + 64)
        call(d_ws, d_out)
        ch.expect(tag, lambda: ch.get(d_out, np.uint8, n).tobytes() == o["raw"] and (ch.get(d_out)[n:n + 64] == FILL).all())

    d_pl, d_nb, d_idx, d_fine = made["encode_fine"]
    decode("decode_fine", lambda d_ws, d_out: ch.call("decode_fine", lib.mh_dev_decode_fine, m.handle, ptr(d_pl), nbits, None, ptr(d_out), n, ptr(d_idx), c,
                                                       ptr(d_fine), ptr(d_ws), dwsb, ws=d_ws))
    d_pl, d_nb, d_idx, d_fine = made["encode_ctx_fine"]
    decode("decode_fine, the length on the device", lambda d_ws, d_out: ch.call(
        "decode_fine, the length on the device", lib.mh_dev_decode_fine, m.handle, ptr(d_pl), 0, ptr(d_nb), ptr(d_out), n, ptr(d_idx), c, ptr(d_fine),
        ptr(d_ws), dwsb, ws=d_ws))
    d_pl, d_nb, d_idx, _ = made["encode"]
    decode("decode_dn", lambda d_ws, d_out: ch.call("decode_dn", lib.mh_dev_decode_dn, m.handle, ptr(d_pl), ptr(d_nb), nbits, ptr(d_out), n, ptr(d_idx), c,
                                                     ptr(d_ws), dwsb, ws=d_ws))
    d_pl, d_nb, d_idx, _ = made["encode_at"]
    decode("decode_dn without a hint", lambda d_ws, d_out: ch.call("decode_dn without a hint", lib.mh_dev_decode_dn, m.handle, ptr(d_pl), ptr(d_nb), 0,
                                                                    ptr(d_out), n, ptr(d_idx), c, ptr(d_ws), dwsb, ws=d_ws))
    drive(ch)
