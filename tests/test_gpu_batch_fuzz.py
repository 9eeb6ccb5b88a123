"""Seeded differential fuzz of the batch call family on the GPU: every case of tests/batch_ref.py goes through every batch call
of include/mh.h — encode, histograms, decode (indexed, index-free, segment states), lookups, search, coded histogram, re-code,
per-stream models and banks, dictionary search, spans from hits (plain and tagged), masked and splicing re-code, the table
splice (a replacement per span, insertions) and their order-2 forms — and every result is compared exactly with the references
of tests/batch_ref.py: the CPU oracle's code tables and plain numpy on the original messages, never another call of the library.
tests/test_batch_ref.py pins those references and the edges that the case list reaches.

The 64 cases without an order-2 side run edit, splice and splice_table; the 32 with one run edit_o2 (all five pairs of orders) and
splice_table_o2: the 17 with an order-2 source splice, the 15 with an order-0 / 1 source under an order-2 destination must be
refused with MH_ERR_ARG.  The order-2 forms are compared under the case's destination and under a covering one, trained on the
originals and every edited form: nothing is dropped there, so every byte at the edge of a span has a code that depends on its
exact context, and a wrong look-back cannot hide behind a drop.

One test per case; its id names the case.  A case runs every family and then reports all that differed, so one failure does
not hide the next.  The decoders read the reference's payloads and index, not the encoder's output."""
import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import edit_ref
import find_ref
from oracle import mh_oracle

pytestmark = pytest.mark.gpu

CASES = batch_ref.draw_cases()
FEEDBACK = 256                     # hit records fed back as lookups: all of them, or this many evenly spaced ones (first and last included)


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


class Rig:
    """One case on the device: the models, the reference forms of the batch and a list of what differed."""

    def __init__(self, mhc, case):
        self.mhc, self.case, self.w = mhc, case, case.world()
        self.so, self.do = case.orders
        self.c, self.p0, self.msgs = case.chunk, self.w.prev0, self.w.messages
        self.n = len(self.msgs)
        self.joined = b"".join(self.msgs)
        self.bad, self.set, self.cover = [], None, None
        (sc, sl), (dc, dl) = case.counts("src"), case.counts("dst")
        self.S, self.D = mhc.Model.from_counts(sc, self.so, max_len=sl), mhc.Model.from_counts(dc, self.do, max_len=dl)
        self.rs = batch_ref.pack(self.msgs, *case.codes("src"), self.so, self.p0, self.c)
        self.rd = batch_ref.pack(self.msgs, *case.codes("dst"), self.do, self.p0, self.c)

    def check(self, ok, what):
        if not ok:
            self.bad.append(what)

    def ok(self, rc, st, what):
        self.check(rc == self.mhc.MH_OK and not np.asarray(st).any(), what + ": status")

    def family(self, fn):
        try:
            fn()
        except Exception as e:                                    # (a call that raises is a finding of this family; the others still run)
            self.bad.append("%s: %s: %s" % (fn.__name__, type(e).__name__, e))

    def source(self, ref, indexed):
        """(payload, pay_off, nbits), keywords of a reader of the reference's batch."""
        kw = dict(prev0=self.p0, chunk_symbols=self.c)
        if indexed:
            kw.update(sym_off=ref.sym_off, index=ref.index_array(self.c))
        return (ref.payload, ref.pay_off, ref.nbits), kw

    def same_batch(self, got, ref, what):
        pay, off, nb, idx, so = got
        self.check(same(off, ref.pay_off) and same(nb, ref.nbits) and same(so, ref.sym_off), what + ": offsets, nbits")
        self.check(same(pay, ref.payload), what + ": payload")
        self.check(same(ref.slices_of(idx, self.c), ref.all_slices()), what + ": index slices")

    # ---- encode ----
    def encode(self):
        enc = lambda m, o: (m.encode_batch_o2 if o == 2 else m.encode_batch)(self.msgs, prev0=self.p0, chunk_symbols=self.c)
        self.same_batch(enc(self.S, self.so), self.rs, "encode (source)")
        self.same_batch(enc(self.D, self.do), self.rd, "encode (destination, %s)" % self.case.dst_kind)
        if self.case.dst_kind != "foreign" and self.so < 2:       # encode-only under a model that lacks pairs of the batch
            counts = batch_ref.histogram(self.w.foreign, self.so, self.p0)
            ref = batch_ref.pack(self.msgs, *batch_ref.oracle_codes(counts, self.so), self.so, self.p0, self.c)
            self.same_batch(enc(self.mhc.Model.from_counts(counts, self.so), self.so), ref, "encode (foreign)")
        for order in (0, 1):
            got = self.mhc.histogram_o1_batch(self.msgs, prev0=self.p0, order=order)
            self.check(same(got, batch_ref.histogram(self.msgs, order, self.p0)), "histogram_o1_batch order %d" % order)
        self.check(same(self.mhc.histogram_o2_batch(self.msgs, prev0=self.p0), batch_ref.histogram(self.msgs, 2, self.p0)), "histogram_o2_batch")

    # ---- decode ----
    def decode(self):
        S, rs = self.S, self.rs
        dec = S.decode_batch_o2 if self.so == 2 else S.decode_batch
        for indexed in (True, False):
            src, kw = self.source(rs, indexed)
            if not indexed:
                kw.pop("chunk_symbols")
            out, so, st = dec(*src, check=False, **kw)
            self.check(not st.any() and out == self.joined and same(so, rs.sym_off), "decode indexed=%s" % indexed)
        if self.so < 2:
            src = (rs.payload, rs.pay_off, rs.nbits)
            out, so, st = S.decode_batch_segments(*src, prev0=self.p0)
            self.check(not st.any() and out == self.joined and same(so, rs.sym_off), "decode_batch_segments")
            so, idx, st = S.index_batch(*src, self.c, prev0=self.p0)
            self.check(not st.any() and same(so, rs.sym_off) and same(rs.slices_of(idx, self.c), rs.all_slices()), "index_batch")

    # ---- lookups ----
    def lookups(self):
        S, rs, w = self.S, self.rs, self.w
        dev = S.dev_decode_batch_o2_ranges if self.so == 2 else S.dev_decode_batch_ranges
        host = S.decode_batch_o2_ranges if self.so == 2 else S.decode_batch_ranges
        for indexed in (True, False):
            src, kw = self.source(rs, indexed)
            got, st, rc = dev(*src, w.lookups, **kw)
            self.ok(rc, st, "lookups indexed=%s" % indexed)
            self.check(got == w.lookup_bytes, "lookups indexed=%s" % indexed)
            if self.case.index % 4 == 0:
                got, st = host(*src, w.lookups, **kw)
                self.check(not st.any() and got == w.lookup_bytes, "lookups (host form) indexed=%s" % indexed)

    # ---- search ----
    def search(self, find=None, ref=None, what="search", ps=None, hits=None):
        w, cap_error = self.w, self.mhc.MH_ERR_CAPACITY
        find = find or (self.S.dev_find_batch_o2 if self.so == 2 else self.S.dev_find_batch)
        ref = ref or self.rs
        ps = ps or self.mhc.PatternSet(w.patterns, fold=w.fold)
        hits = find_ref.find_hits(self.msgs, w.patterns, fold=w.fold) if hits is None else hits
        w_off, w_rec, w_pat = find_ref.hit_arrays(hits, self.n)
        for indexed in (True, False):
            tag = "%s indexed=%s" % (what, indexed)
            src, kw = self.source(ref, indexed)
            ho, rec, pat, st, rc = find(ps, *src, **kw)
            self.ok(rc, st, tag)
            self.check(same(ho, w_off) and same(rec, w_rec) and same(pat, w_pat), tag + ": records")
            ho, _, _, st, rc = find(ps, *src, count_only=True, **kw)
            self.ok(rc, st, tag + " count only")
            self.check(same(ho, w_off), tag + ": count only")
            cap = len(hits) - 1
            ho, rec, pat, st, rc = find(ps, *src, hit_cap=cap, **kw)
            self.check(rc == cap_error and not st.any() and same(ho, w_off) and same(rec, w_rec[:cap]) and same(pat, w_pat[:cap]), tag + ": hit_cap")
        return w_rec, w_pat

    def feed_back(self, w_rec, w_pat, patterns, what):
        pick = np.unique(np.linspace(0, len(w_rec) - 1, min(len(w_rec), FEEDBACK)).astype(np.int64))
        dev = self.S.dev_decode_batch_o2_ranges if self.so == 2 else self.S.dev_decode_batch_ranges
        src, kw = self.source(self.rs, True)
        got, st, rc = dev(*src, w_rec[pick], **kw)
        self.ok(rc, st, what)
        fold = find_ref.fold_ascii if self.w.fold else bytes
        self.check([fold(g) for g in got] == [fold(patterns[int(j)]) for j in w_pat[pick]], what)

    def search_and_feed_back(self):
        w_rec, w_pat = self.search()
        self.feed_back(w_rec, w_pat, self.w.patterns, "hit records as lookups")

    # ---- coded histogram ----
    def coded_histogram(self):
        for order in (0, 1, 2):
            fn = self.S.dev_histogram_coded_o2 if 2 in (order, self.so) else self.S.dev_histogram_coded
            want = batch_ref.histogram(self.msgs, order, self.p0)
            for indexed in (True, False):
                src, kw = self.source(self.rs, indexed)
                counts, st, rc = fn(order, *src, **kw)
                self.ok(rc, st, "coded histogram order %d indexed=%s" % (order, indexed))
                self.check(same(counts, want), "coded histogram order %d indexed=%s" % (order, indexed))

    # ---- re-code ----
    def recode(self, fn=None, ref=None, what="recode"):
        fn = fn or (self.S.dev_recode_batch_o2 if 2 in self.case.orders else self.S.dev_recode_batch)
        rd = self.rd
        for indexed in (True, False):
            tag = "%s indexed=%s" % (what, indexed)
            src, kw = self.source(ref or self.rs, indexed)
            got = fn(self.D, *src, **kw)
            self.ok(got["rc"], got["status"], tag)
            self.check(same(got["out_off"], rd.pay_off) and same(got["nbits"], rd.nbits) and same(got["sym_off"], rd.sym_off), tag + ": offsets, nbits")
            self.check(same(got["payload"], rd.payload), tag + ": payload")
            self.check(same(got["dropped"], rd.dropped), tag + ": dropped")
            self.check(same(rd.slices_of(got["index"], self.c), rd.all_slices()), tag + ": index slices")
            count = fn(self.D, *src, count_only=True, **kw)
            self.ok(count["rc"], count["status"], tag + " count only")
            self.check(same(count["out_off"], got["out_off"]) and same(count["nbits"], got["nbits"]) and same(count["dropped"], got["dropped"]),
                       tag + ": count only")

    # ---- per-stream models ----
    def model_set(self):
        """(the reference's batch with every stream under the oracle's model of its own histogram, the table files, the set)."""
        if self.set is None:
            re, tables = batch_ref.pack_each(self.msgs, self.so, self.p0, self.c)
            self.set = (re, tables, self.mhc.ModelSet.from_tables(tables))
        return self.set

    def each(self):
        mhc, c, p0 = self.mhc, self.c, self.p0
        re, tables, ms = self.model_set()
        got = mhc.compress_each(self.msgs, order=self.so, chunk_symbols=c, prev0=p0)
        self.check([g[0] for g in got] == tables, "compress_each: tables")
        self.check([g[2] for g in got] == re.nbits.tolist(), "compress_each: nbits")
        self.check(b"".join(g[1][1:] for g in got) == re.payload.tobytes(), "compress_each: payloads")
        self.check(same(np.concatenate([g[3] for g in got]), re.all_slices()), "compress_each: index slices")
        if p0 == batch_ref.PREV0:                                 # the oracle's own stream of every message alone
            blobs = [mh_oracle.Model.from_data(m, self.so).compress(m)[0] for m in self.msgs]
            self.check([g[1] for g in got] == blobs, "compress_each: the oracle's files")
        for indexed in (True, False):
            src, kw = self.source(re, indexed)
            if not indexed:
                kw.pop("chunk_symbols")
            out, so, st, rc = ms.decode(*src, **kw)
            self.ok(rc, st, "each decode indexed=%s" % indexed)
            self.check(out == self.joined and same(so, re.sym_off), "each decode indexed=%s" % indexed)
            src, kw = self.source(re, indexed)
            res, st, rc = ms.decode_ranges(*src, self.w.lookups, **kw)
            self.ok(rc, st, "each lookups indexed=%s" % indexed)
            self.check(res == self.w.lookup_bytes, "each lookups indexed=%s" % indexed)
            for order in (0, 1):
                counts, st, rc = ms.histogram_coded(order, *src, **kw)
                self.ok(rc, st, "each coded histogram")
                self.check(same(counts, batch_ref.histogram(self.msgs, order, p0)), "each coded histogram order %d indexed=%s" % (order, indexed))
        self.search(ms.find, re, "each search")
        self.recode(ms.recode, re, "each recode")

    # ---- banks ----
    def bank(self):
        mhc, p0, msgs = self.mhc, self.p0, self.msgs
        drawn = [(1, msgs[:(self.n + 1) // 2]), (0, self.w.foreign), (self.so, msgs[::3]), (self.so, msgs)]
        counts = [(o, batch_ref.histogram(m, o, p0)) for o, m in drawn]
        codes = [(o, batch_ref.oracle_codes(h, o)) for o, h in counts]
        bank = mhc.ModelSet.from_models([mhc.Model.from_counts(h, o) for o, h in counts])
        choice, nbits = bank.select(msgs, prev0=p0)
        want_c, want_n = batch_ref.select([(o, lc[0]) for o, lc in codes], msgs, p0)
        self.check(same(choice, want_c) and same(nbits, want_n), "bank select")
        ref = batch_ref.merge([batch_ref.pack([m], *codes[k][1], codes[k][0], p0, self.c) for m, k in zip(msgs, want_c)])
        self.same_batch(mhc.encode_bank(bank, msgs, want_c, chunk_symbols=self.c, prev0=p0), ref, "encode_bank")
        out, so, st = mhc.decode_bank(bank, want_c, ref.payload, ref.pay_off, ref.nbits, prev0=p0, check=False)
        self.check(not st.any() and out == self.joined and same(so, ref.sym_off), "decode_bank index-free")
        out, so, st = mhc.decode_bank(bank, want_c, ref.payload, ref.pay_off, ref.nbits, sym_off=ref.sym_off, index=ref.index_array(self.c),
                                      chunk_symbols=self.c, prev0=p0, check=False)
        self.check(not st.any() and out == self.joined, "decode_bank indexed")

    # ---- dictionary search ----
    def dictionary_search(self):
        mhc, S, e = self.mhc, self.S, self.case.edits()
        d = mhc.Dict(e.dictionary, fold=e.fold)
        self.check((d.states, d.classes) == (e.states, e.classes), "dictionary: states, classes")
        if self.so < 2:                                           # what test_batch_ref.py takes for the LDS that the matcher gets
            P, nsec, in_lds = S.decode_layout()
            lds = 1024 + (512 << P) + (((2 * nsec + 15) & ~15) if in_lds else 0)
            self.check(lds == batch_ref.tables_lds(*self.case.codes("src"), self.so), "dictionary: the source's tables in LDS")
        w_rec, w_pat = self.search(S.dev_find_dict_batch_o2 if self.so == 2 else S.dev_find_dict_batch, None, "dictionary search", d, e.hits)
        if self.case.index % 4 == 0:
            host = S.find_dict_batch_o2 if self.so == 2 else S.find_dict_batch
            for indexed in (True, False):
                src, kw = self.source(self.rs, indexed)
                ho, rec, pat, st, rc = host(d, *src, **kw)
                self.ok(rc, st, "dictionary search (host form) indexed=%s" % indexed)
                self.check(same(ho, e.hit_off) and same(rec, w_rec) and same(pat, w_pat), "dictionary search (host form) indexed=%s" % indexed)
        if self.eligible(self.case):
            self.search(self.model_set()[2].find_dict, self.model_set()[0], "each dictionary search", d, e.hits)
        self.feed_back(w_rec, w_pat, e.dictionary, "dictionary hits as lookups")

    # ---- spans from hits ----
    def spans(self):
        e = self.case.edits()
        want_off, want = edit_ref.merge_hits(e.hit_off, e.records)
        for fn in (self.mhc.spans_from_hits, self.mhc.dev_spans_from_hits):
            span_off, spans, rc = fn(e.hit_off, e.records)
            self.check(rc == self.mhc.MH_OK and same(span_off, want_off) and same(spans, want), fn.__name__)

    # ---- masked and splicing re-code ----
    def same_recode(self, got, ref, tag, out_sym_off=None):
        self.ok(got["rc"], got["status"], tag)
        self.check(same(got["out_off"], ref.pay_off) and same(got["nbits"], ref.nbits) and same(got["sym_off"], self.rs.sym_off), tag + ": offsets, nbits")
        self.check(same(got["payload"], ref.payload), tag + ": payload")
        self.check(same(got["dropped"], ref.dropped), tag + ": dropped")
        if out_sym_off is not None:
            self.check(same(got["out_sym_off"], out_sym_off), tag + ": out_sym_off")
        self.check(same(ref.slices_of(got["index"], self.c), ref.all_slices()), tag + ": index slices")

    def same_counts(self, count, got, tag):
        self.ok(count["rc"], count["status"], tag + " count only")
        self.check(all(same(count[k], got[k]) for k in ("out_off", "nbits", "dropped", "out_sym_off") if k in got), tag + ": count only")

    def edit_with(self, fn, ref, what, dst=None, want=None):
        """fn: a device form of the masked re-code, reading the reference's batch `ref`; want: (with the span list, everywhere)
        under dst, by default the case's destination."""
        e, x = self.case.edits(), self.case.expected()
        dst, (edit, edit_all) = dst or self.D, want or (x.edit, x.edit_all)
        for indexed in (True, False):
            tag = "%s indexed=%s" % (what, indexed)
            src, kw = self.source(ref, indexed)
            got = fn(dst, *src, e.byte_map, e.span_off, e.spans, **kw)
            self.same_recode(got, edit, tag)
            self.same_counts(fn(dst, *src, e.byte_map, e.span_off, e.spans, count_only=True, **kw), got, tag)
        src, kw = self.source(ref, self.case.index % 2 == 0)
        self.same_recode(fn(dst, *src, e.byte_map, None, None, **kw), edit_all, what + " everywhere")

    def edit(self):
        e, x = self.case.edits(), self.case.expected()
        self.edit_with(self.S.dev_recode_edit_batch, self.rs, "edit (%s)" % e.map_kind)
        if self.case.index % 4 == 0:
            for indexed in (True, False):
                src, kw = self.source(self.rs, indexed)
                self.same_recode(self.S.recode_edit_batch(self.D, *src, e.byte_map, e.span_off, e.spans, **kw), x.edit,
                                 "edit (host form) indexed=%s" % indexed)
        if self.eligible(self.case):
            self.edit_with(self.model_set()[2].recode_edit, self.model_set()[0], "each edit")

    def splice_with(self, fn, ref, what):
        """fn: a device form of the splicing re-code, reading the reference's batch `ref`; both replacements."""
        e, x = self.case.edits(), self.case.expected()
        for k, rep in enumerate(e.reps):
            for indexed in (True, False):
                tag = "%s of %d bytes indexed=%s" % (what, len(rep), indexed)
                src, kw = self.source(ref, indexed)
                got = fn(self.D, *src, rep, e.span_off, e.spans, **kw)
                self.same_recode(got, x.splice[k], tag, x.out_sym_off[k])
                self.same_counts(fn(self.D, *src, rep, e.span_off, e.spans, count_only=True, **kw), got, tag)

    def splice(self):
        e, x = self.case.edits(), self.case.expected()
        self.splice_with(self.S.dev_recode_splice_batch, self.rs, "splice")
        if self.case.index % 4 == 0:
            for k, rep in enumerate(e.reps):
                for indexed in (True, False):
                    src, kw = self.source(self.rs, indexed)
                    self.same_recode(self.S.recode_splice_batch(self.D, *src, rep, e.span_off, e.spans, **kw), x.splice[k],
                                     "splice (host form) of %d bytes indexed=%s" % (len(rep), indexed), x.out_sym_off[k])
        if self.eligible(self.case):
            self.splice_with(self.model_set()[2].recode_splice, self.model_set()[0], "each splice")

    # ---- tagged spans from hits ----
    def spans_tagged(self):
        e, t = self.case.edits(), self.case.table()
        want_off, want, want_tag = t.merged
        plain_off, plain = edit_ref.merge_hits(e.hit_off, e.records)
        self.check(same(want_off, plain_off) and same(want, plain), "spans_tagged: the two references' spans")
        for fn in (self.mhc.spans_from_hits_tagged, self.mhc.dev_spans_from_hits_tagged):
            span_off, spans, tags, rc = fn(e.hit_off, e.records, e.hit_pattern)
            self.check(rc == self.mhc.MH_OK and same(span_off, want_off) and same(spans, want), fn.__name__ + ": spans")
            self.check(same(tags, want_tag), fn.__name__ + ": tags")

    # ---- the table splice ----
    def covering(self):
        """The covering destination's model."""
        if self.cover is None:
            self.cover = self.mhc.Model.from_counts(self.case.cover_counts(), self.do)
        return self.cover

    def table_with(self, fn, ref, what, dst, want, out_sym_off, tags, reps, span_off, spans, counts=True):
        """fn: a device form of the table splice, reading the reference's batch `ref`; want: batch_ref.Packed under dst."""
        for indexed in (True, False):
            tag = "%s indexed=%s" % (what, indexed)
            src, kw = self.source(ref, indexed)
            got = fn(dst, *src, tags, reps, span_off, spans, **kw)
            self.same_recode(got, want, tag, out_sym_off)
            if counts:
                self.same_counts(fn(dst, *src, tags, reps, span_off, spans, count_only=True, **kw), got, tag)

    def one_entry_tables(self, fn, what):
        """A table of one entry, every span of the untagged list under tag 0: the single replacement's expectation."""
        e, x = self.case.edits(), self.case.expected()
        for k, rep in enumerate(e.reps):
            self.table_with(fn, self.rs, "%s, one entry of %d bytes" % (what, len(rep)), self.D, x.splice[k], x.out_sym_off[k],
                            np.zeros(len(e.spans), dtype=np.uint32), [rep], e.span_off, e.spans, counts=False)

    def table_host(self, fn, what, dst, want, out_sym_off):
        t = self.case.table()
        for indexed in (True, False):
            src, kw = self.source(self.rs, indexed)
            self.same_recode(fn(dst, *src, t.tags, t.reps, t.span_off, t.spans, **kw), want, "%s (host form) indexed=%s" % (what, indexed), out_sym_off)

    def splice_table(self):
        t, x = self.case.table(), self.case.expected_table()
        mine = (t.tags, t.reps, t.span_off, t.spans)
        self.table_with(self.S.dev_recode_splice_table_batch, self.rs, "splice_table", self.D, x.packed, x.out_sym_off, *mine)
        self.one_entry_tables(self.S.dev_recode_splice_table_batch, "splice_table")
        if self.case.index % 4 == 0:
            self.table_host(self.S.recode_splice_table_batch, "splice_table", self.D, x.packed, x.out_sym_off)
        if self.eligible(self.case):
            self.table_with(self.model_set()[2].recode_splice_table, self.model_set()[0], "each splice_table", self.D, x.packed, x.out_sym_off, *mine)

    # ---- order 2 in editing and splicing ----
    def edit_o2(self):
        e, x = self.case.edits(), self.case.expected()
        fn = self.S.dev_recode_edit_batch_o2
        self.edit_with(fn, self.rs, "edit_o2 (%s)" % e.map_kind)
        self.edit_with(fn, self.rs, "edit_o2 (%s), covering" % e.map_kind, self.covering(), (x.edit_cover, x.edit_all_cover))
        if self.case.index % 4 == 0:
            for indexed in (True, False):
                src, kw = self.source(self.rs, indexed)
                self.same_recode(self.S.recode_edit_batch_o2(self.D, *src, e.byte_map, span_off=e.span_off, spans=e.spans, **kw), x.edit,
                                 "edit_o2 (host form) indexed=%s" % indexed)

    def splice_table_o2(self):
        t = self.case.table()
        mine = (t.tags, t.reps, t.span_off, t.spans)
        fn = self.S.dev_recode_splice_table_batch_o2
        if self.so < 2:                                           # an order-0 / 1 source under an order-2 destination: refused
            for call, what in ((fn, "device"), (self.S.recode_splice_table_batch_o2, "host")):
                src, kw = self.source(self.rs, True)
                try:
                    call(self.D, *src, *mine, **kw)
                    self.check(False, "splice_table_o2 (%s form): no refusal of an order-%d source" % (what, self.so))
                except self.mhc.MhError as err:
                    self.check(err.status == self.mhc.MH_ERR_ARG, "splice_table_o2 (%s form): refused with %d" % (what, err.status))
            return
        x = self.case.expected_table()
        self.table_with(fn, self.rs, "splice_table_o2", self.D, x.packed, x.out_sym_off, *mine)
        self.table_with(fn, self.rs, "splice_table_o2, covering", self.covering(), x.cover, x.out_sym_off, *mine)
        self.one_entry_tables(fn, "splice_table_o2")
        if self.case.index % 4 == 0:
            self.table_host(self.S.recode_splice_table_batch_o2, "splice_table_o2", self.D, x.packed, x.out_sym_off)
            self.table_host(self.S.recode_splice_table_batch_o2, "splice_table_o2, covering", self.covering(), x.cover, x.out_sym_off)


    # ---- all of them ----
    @staticmethod
    def eligible(case):
        """Whether a case runs the per-stream-model and bank families (sets are order 0 / 1; a set grows with its streams)."""
        return 2 not in case.orders and case.n_streams <= 65

    def families(self):
        """Every family that runs for this case, in order."""
        fams = [self.encode, self.decode, self.lookups, self.search_and_feed_back, self.coded_histogram, self.recode]
        fams += [self.each, self.bank] if self.eligible(self.case) else []
        fams += [self.dictionary_search, self.spans, self.spans_tagged]
        return fams + ([self.edit, self.splice, self.splice_table] if 2 not in self.case.orders else [self.edit_o2, self.splice_table_o2])

    def run_all(self):
        for fn in self.families():
            self.family(fn)
        return self.bad


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_batch_call_equals_the_references(mhc, case):
    rig = Rig(mhc, case)
    rig.run_all()
    assert not rig.bad, "%s: %d differences:\n  %s" % (case.id, len(rig.bad), "\n  ".join(rig.bad))
