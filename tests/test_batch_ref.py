"""The references of the batch-family fuzz (tests/batch_ref.py) pinned to the CPU oracle and the golden fixtures, and the
coverage that the fixed case list of tests/test_gpu_batch_fuzz.py must keep.  No GPU, no library call: everything here is the
oracle, numpy and the committed files."""
import functools
import hashlib
import os

import numpy as np
import pytest

import batch_ref
import edit_o2_ref
import find_ref
import recode_ref
import splice_table_ref
from conftest import GOLDEN_DIR, expected_file, golden, golden_names
from oracle import mh_oracle

TEXTS = ["input_ipsum.txt", "input_wiki_cpp.html", "input_wiki_cpp.txt"]


def lines_of(name, limit=400):
    data = golden()[name]["data"]
    return ([ln for ln in data.split(b"\n")][:limit] + [b""]) if len(data) < (1 << 19) else [data]


# ---------------------------------------------------------------------------------------------------- the packer
@pytest.mark.parametrize("name", golden_names())
@pytest.mark.parametrize("order", [0, 1, 2])
def test_pack_equals_the_oracle_s_compress_of_every_line(name, order):
    msgs = lines_of(name)
    o = mh_oracle.Model.from_data(golden()[name]["data"], order)
    lens, codes = (o.codes_o2() if order == 2 else o.codes())
    p = batch_ref.pack(msgs, lens, codes, order, 0x20, 256)
    assert p.pay_off[0] == 0                                     # (a line's first pair may lack a code: the oracle skips it too)
    for i, m in enumerate(msgs):
        blob, nbits = o.compress(m)
        assert int(p.nbits[i]) == nbits, (name, i)
        assert p.payload[int(p.pay_off[i]):int(p.pay_off[i + 1])].tobytes() == blob[1:], (name, i)
        if order < 2:
            assert np.array_equal(p.slices[i], recode_ref.index_slice(lens, m, order, 256)), (name, i)


def test_order_2_index_entries_carry_both_bytes_in_front():
    msgs = [b"abcdefgh" * 40, b"", b"x", b"xy" * 128, b"q" * 257]
    o = mh_oracle.Model.from_counts(batch_ref.histogram(msgs, 2, 0x61), 2)
    lens, codes = o.codes_o2()
    p = batch_ref.pack(msgs, lens, codes, 2, 0x61, 256)
    assert [s.size for s in p.slices] == [2, 0, 1, 1, 2]
    assert int(p.slices[0][0]) == 0x6161 << 48 and int(p.slices[2][0]) == 0x6161 << 48
    rel = int(lens[batch_ref.keys([msgs[0][:256]], 2, 0x61)[0]].sum())
    assert int(p.slices[0][1]) == (ord("g") << 56) | (ord("h") << 48) | rel
    assert int(p.slices[4][1]) == (ord("q") << 56) | (ord("q") << 48) | int(p.nbits[4]) - int(lens[(0x7171 << 8) | 0x71])
    assert np.array_equal(p.slices_of(p.index_array(256), 256), p.all_slices())


@pytest.mark.parametrize("x,y", [("input_wiki_cpp.txt", "input_wiki_cpp.html"), ("input_ipsum.txt", "input_wiki_cpp.html"),
                                 ("input_wiki_cpp.html", "input_ipsum.txt")])
@pytest.mark.parametrize("order", [0, 1])
def test_pack_equals_recode_ref_under_a_destination_with_drops(x, y, order):
    msgs = lines_of(x)
    dst = mh_oracle.Model.from_data(golden()[y]["data"], order)
    lens, codes = dst.codes()
    p = batch_ref.pack(msgs, lens, codes, order, 0x20, 512)
    want = recode_ref.recode(msgs, dst, 512)
    payload, off, nbits, dropped = recode_ref.packed(want)
    assert dropped.sum() > 0 or (order == 0 and y != "input_ipsum.txt")      # (the html has every byte value of the texts)
    assert np.array_equal(p.payload, payload) and np.array_equal(p.pay_off, off)
    assert np.array_equal(p.nbits, nbits) and np.array_equal(p.dropped, dropped)
    assert all(np.array_equal(a, w[3]) for a, w in zip(p.slices, want))


@pytest.mark.parametrize("order", [0, 1, 2])
def test_pack_under_the_covering_destination_equals_the_oracle_s_compress_of_every_spliced_message(order):
    """The first case with an order-2 source, a destination of this order and the oracle's own prev0: its table-spliced messages
    under the covering destination, message by message."""
    case = next(c for c in batch_ref.draw_cases() if c.orders == (2, order) and c.world().prev0 == recode_ref.PREV0)
    x = case.expected_table()
    o = mh_oracle.Model.from_counts(case.cover_counts(), order)
    lens, _ = o.codes_o2() if order == 2 else o.codes()
    p = x.cover
    assert len(x.spliced) == case.n_streams and x.spliced != case.world().messages and not p.dropped.any()
    for i, m in enumerate(x.spliced):
        blob, nbits = o.compress(m)
        assert int(p.nbits[i]) == nbits, (case.id, i)
        assert p.payload[int(p.pay_off[i]):int(p.pay_off[i + 1])].tobytes() == blob[1:], (case.id, i)
        if order < 2:
            assert np.array_equal(p.slices[i], recode_ref.index_slice(lens, m, order, case.chunk)), (case.id, i)


@pytest.mark.parametrize("x,y", [("input_a.txt", "input_b.txt"), ("input_ipsum.txt", "union_ipsum_wiki"), ("input_wiki_cpp.txt", "union_ipsum_wiki"),
                                 ("input_wiki_cpp.txt", "input_wiki_cpp.html"), ("input_ipsum.txt", "input_wiki_cpp.html"),
                                 ("input_wiki_cpp.html", "input_ipsum.txt")])
def test_pack_equals_the_files_the_reference_program_wrote(x, y):
    table = expected_file(y, "e")
    if table is None:
        with open(os.path.join(GOLDEN_DIR, "recode", y + ".e"), "rb") as f:
            table = f.read()
    with open(os.path.join(GOLDEN_DIR, "recode", "%s__%s.cm" % (x, y)), "rb") as f:
        want = f.read()
    lens, codes = mh_oracle.Model.from_table(table).codes()
    p = batch_ref.pack([golden()[x]["data"]], lens, codes, 1, 0x20)
    assert p.payload.tobytes() == want[1:] and (8 - int(p.nbits[0]) % 8) % 8 == want[0] & 7


@pytest.mark.parametrize("name", golden_names())
def test_histograms_equal_the_oracle_s(name):
    data = golden()[name]["data"][:200000]
    assert np.array_equal(batch_ref.histogram([data], 0), mh_oracle.histogram_o0(data))
    for prev0 in (0x20, 0x65):
        assert np.array_equal(batch_ref.histogram([data], 1, prev0), mh_oracle.histogram_o1(data, prev0))
    assert np.array_equal(batch_ref.histogram([data], 2), mh_oracle.histogram_o2(data))
    if name in TEXTS:                                                # a batch is the sum of its messages
        msgs = lines_of(name, 50)
        for order, fn in ((0, mh_oracle.histogram_o0), (1, mh_oracle.histogram_o1), (2, mh_oracle.histogram_o2)):
            assert np.array_equal(batch_ref.histogram(msgs, order), sum(fn(m) for m in msgs))


@pytest.mark.parametrize("limit", [8, 12])
def test_limited_codes_equal_the_rule_s_table_read_by_the_oracle(limit):
    from test_limit_abi import limited_model
    counts = mh_oracle.histogram_o1(golden()["input_wiki_cpp.html"]["data"])
    table, recoded = limited_model(counts, 1, limit, mh_oracle.Model.from_counts(counts, 1).table_bytes())
    assert any(r is not None for r in recoded)
    lens, codes = mh_oracle.Model.from_table(table).codes()
    got_l, got_c = batch_ref.limited_codes(counts, 1, limit)
    assert got_l.max() == limit and np.array_equal(got_l, lens) and np.array_equal(got_c[lens > 0], codes[lens > 0])


def test_select_takes_the_cheapest_entry_that_covers_the_stream():
    msgs = [b"aaaa", b"", b"abab", b"zz", b"ab"]
    a = batch_ref.oracle_codes(batch_ref.histogram([b"aaaaaaab"], 0), 0)[0]
    b = batch_ref.oracle_codes(batch_ref.histogram([b"abababab" * 4 + b"aa"], 1, 0x20), 1)[0]
    choice, nbits = batch_ref.select([(0, a), (1, b), (0, a)], msgs)
    assert choice.tolist() == [0, 0, 0, batch_ref.BANK_NONE, 0] and nbits.tolist()[:3] == [4, 0, 4] and nbits[3] == 2 ** 64 - 1
    choice, _ = batch_ref.select([(1, b), (0, a)], msgs)
    assert choice.tolist() == [0, 0, 0, batch_ref.BANK_NONE, 0]       # ties go to the lowest entry


# ---------------------------------------------------------------------------------------------------- coverage
@functools.lru_cache(maxsize=1)
def stats():
    out = []
    for case in batch_ref.draw_cases():
        w = case.world()
        so, do = case.orders
        c = case.chunk
        src = batch_ref.pack(w.messages, *case.codes("src"), so, w.prev0, c)
        dst = batch_ref.pack(w.messages, *case.codes("dst"), do, w.prev0, c)
        ln = np.diff(src.sym_off.astype(np.int64))
        hits = find_ref.find_hits(w.messages, w.patterns, fold=w.fold)
        heads = np.concatenate([np.arange(int(a) + c, int(b), c) for a, b in zip(src.sym_off[:-1], src.sym_off[1:])] + [np.zeros(0, dtype=np.int64)])
        own = batch_ref.histogram(w.messages, max(so, 1), w.prev0).reshape(-1, 256)
        out.append(dict(case=case, prev0=w.prev0, total=int(ln.sum()), empty=bool((ln == 0).any()), multiple=bool(((ln > 0) & (ln % c == 0)).any()),
                        src_max=int(src.used.max()), dst_max=int(dst.used.max()), one_symbol=bool(((own > 0).sum(axis=1) == 1).any()),
                        straddle=find_ref.straddles(hits, c), at_end=sum(1 for i, _, e, _ in hits if e == ln[i]), hits=len(hits),
                        drops=int(dst.dropped.sum()), head_max=int(dst.used[heads.astype(np.int64)].max()) if heads.size else 0,
                        nowhere=len(set(range(len(w.patterns))) - {h[3] for h in hits})))
    return out


def count(pred):
    return sum(1 for s in stats() if pred(s))


def test_the_case_list_is_fixed_and_sized():
    cases = batch_ref.draw_cases()
    assert [c.id for c in cases] == [c.id for c in batch_ref.draw_cases.__wrapped__(batch_ref.SEED)]
    assert len(set(c.id for c in cases)) == len(cases) == 96
    assert sum(1 for c in cases if 2 not in c.orders) == 64
    for s in stats():
        case, w = s["case"], s["case"].world()
        assert 0 < s["total"] <= (batch_ref.DEEP_BYTES if case.deep else batch_ref.CASE_BYTES), case.id
        assert len(w.messages) == case.n_streams and len(w.lookups) == 32, case.id
        assert 1 <= len(w.patterns) <= 15 and sum(len(p) for p in w.patterns) <= 64 and all(w.patterns), case.id
        assert s["straddle"] >= 1 and s["at_end"] >= 1 and s["nowhere"] >= 1, case.id
        assert any(b == e for _, b, e in w.lookups) and any(b == 0 and e == len(w.messages[i]) for i, b, e in w.lookups), case.id
        assert any(b // case.chunk != (e - 1) // case.chunk for _, b, e in w.lookups if e > b), case.id
        assert case.src_kind != "foreign" and (s["drops"] == 0 or case.dst_kind == "foreign"), case.id


def test_coverage_of_the_fixed_case_list():
    """What the fuzz must keep reaching, computed from the references alone."""
    for c in batch_ref.CHUNKS:
        assert count(lambda s: s["case"].chunk == c) >= 4, c
    for n in batch_ref.STREAM_COUNTS:
        assert count(lambda s: s["case"].n_streams == n) >= 3, n
    assert count(lambda s: s["prev0"] != 0x20) >= 10
    assert count(lambda s: s["empty"]) >= 10
    assert count(lambda s: s["multiple"]) >= 10
    deep = lambda s: s["case"].deep
    assert count(lambda s: deep(s) and max(s["src_max"], s["dst_max"]) > 32) >= 8
    assert count(lambda s: deep(s) and max(s["src_max"], s["dst_max"]) > 56) >= 3
    n_deep = count(deep)
    assert 3 * count(lambda s: deep(s) and s["case"].alphabet > 57) >= n_deep       # the longest code is over 56 bits
    assert count(lambda s: max(s["src_max"], s["dst_max"]) > 12) >= 10
    assert count(lambda s: s["one_symbol"]) >= 10
    assert count(lambda s: s["straddle"] > 0) >= 10 and count(lambda s: s["at_end"] > 0) >= 10
    assert count(lambda s: s["drops"] > 0) >= 10
    for so in (0, 1, 2):
        for do in (0, 1, 2):
            assert count(lambda s: s["case"].orders == (so, do)) >= 4, (so, do)
    assert count(lambda s: s["case"].orders == (1, 2) and s["head_max"] > 32) >= 3
    # the lookups with two seams inside, the [0, 0) of an empty stream, an index-free lookup that ends at the stream's end
    assert count(lambda s: any((e - 1) // s["case"].chunk - b // s["case"].chunk >= 2 for _, b, e in s["case"].world().lookups if e > b)) >= 10
    assert count(lambda s: any(e == 0 and not s["case"].world().messages[i] for i, b, e in s["case"].world().lookups)) >= 10


# ---------------------------------------------------------------------------------------------------- the second part of a case
WORLDS_DIGEST = "ba1c99016e4c9bbb9896ab9ba67396fbcba1497cce2c0f5d290131458ecdf7fc"


def test_no_world_moved_when_the_edits_were_added():
    """SHA-256 over every case's id, seed, prev0, chunk, fold, lookups, messages, patterns, foreign text and lookup bytes, computed
    at the commit before Case.edits() existed: the second part of a case draws from a generator of its own."""
    h = hashlib.sha256()
    for case in batch_ref.draw_cases():
        w = case.world()
        case.edits()                                                # (building it must not move anything either)
        h.update(repr((case.id, case.seed, w.prev0, w.chunk, w.fold, [tuple(int(v) for v in lk) for lk in w.lookups])).encode())
        for part in (w.messages, w.patterns, w.foreign, w.lookup_bytes):
            h.update(len(part).to_bytes(8, "little"))
            for m in part:
                h.update(len(m).to_bytes(8, "little") + bytes(m))
    assert h.hexdigest() == WORLDS_DIGEST


@functools.lru_cache(maxsize=1)
def edit_stats():
    out = []
    for case in batch_ref.draw_cases():
        w, e = case.world(), case.edits()
        c, ln = case.chunk, [len(m) for m in w.messages]
        folded = [find_ref.fold_ascii(p) if e.fold else p for p in e.dictionary]
        known = set(folded)
        s = dict(case=case, e=e, hits=len(e.hits), placements=batch_ref.placements(w.messages, e.span_off, e.spans, c),
                 seam255=any(t - b == 255 and b // c != (t - 1) // c for _, b, t, _ in e.hits), at_end=any(t == ln[i] for i, _, t, _ in e.hits),
                 nowhere=len(set(range(len(folded))) - {h[3] for h in e.hits}), duplicates=len(folded) - len(known),
                 family=any(len(p) >= 4 and all(p[k:] in known for k in range(1, len(p))) and any(p[:k] in known for k in range(1, len(p)))
                            for p in known),
                 rarest=min(np.bincount(np.frombuffer(b"".join(w.messages), dtype=np.uint8), minlength=256)[sorted(set(b"".join(w.messages)))]),
                 rows=batch_ref.dict_rows_in_lds(case, e.states, e.classes))
        x = case.expected()
        per = batch_ref.span_lists(e.span_off, e.spans)
        src = batch_ref.pack(w.messages, *case.codes("src"), case.orders[0], w.prev0, c)
        mask = batch_ref.span_mask(w.messages, e.span_off, e.spans)
        chunks = lambda k: (k + c - 1) // c
        s.update(spliced=sum(len(m) for m in x.spliced[1]),
                 emptied=any(l and not len(y) for l, y in zip(ln, x.spliced[0])),
                 first_chunk=any(b == 0 and c <= t < ln[i] for i, lst in enumerate(per) for b, t in lst),
                 grows=any(chunks(len(y)) > chunks(l) for l, y in zip(ln, x.spliced[1])),
                 drops=max(int(p.dropped.sum()) for p in [x.edit, x.edit_all] + x.splice),
                 near=max(int(src.used[mask].max()), int(x.edit.used[mask].max())) if mask.any() else 0,
                 cover_drops=sum(int(p.dropped.sum()) for p in (x.edit_cover, x.edit_all_cover)) if 2 in case.orders else 0)
        s.update(table_stats(case, src))
        out.append(s)
    return out


def splices(case):
    """Whether the case runs a table splice: no order-2 side, or an order-2 source."""
    return case.orders[0] == 2 or 2 not in case.orders


def table_stats(case, src):
    """The third part of a case (src: the packer's form of the messages under the source model)."""
    w, t = case.world(), case.table()
    c, ln = case.chunk, [len(m) for m in w.messages]
    per = batch_ref.tagged_span_lists(t.span_off, t.spans, t.tags)
    s = dict(t=t, well_formed=all(splice_table_ref.well_formed([p[:2] for p in lst]) for lst in per),
             insertions=batch_ref.insertions(w.messages, t.span_off, t.spans, t.tags, t.reps, c),
             output_seams=batch_ref.output_seams(w.messages, t.span_off, t.spans, t.tags, t.reps, c))
    if not splices(case):
        return s
    x = case.expected_table()
    # a lane that starts at source position c or 2 c: the two OUTPUT bytes in front of it are not the two source bytes there
    moved = 0
    for F in (c, 2 * c):
        ctx = edit_o2_ref.start_context(w.messages, t.span_off, t.spans, t.tags, t.reps, F, w.prev0)
        moved += sum(1 for m, v in zip(w.messages, ctx) if v is not None and v != (m[F - 2] << 8) | m[F - 1])
    # a span that ends one byte in front of a seam F and x[F - 1] in no span (the look-back's F = end + 1): the earlier of the two
    # output bytes in front of F is not x[F - 2]
    stops = [{min(end, ln[i]) for b, end, _ in lst if b < ln[i]} for i, lst in enumerate(per)]
    ends = 0
    for F in sorted({p + 1 for i, st in enumerate(stops) for p in st if (p + 1) % c == 0 and p + 1 < ln[i]}):
        ctx = edit_o2_ref.start_context(w.messages, t.span_off, t.spans, t.tags, t.reps, F, w.prev0)
        ends += sum(1 for i, (m, v) in enumerate(zip(w.messages, ctx)) if v is not None and F - 1 in stops[i] and v >> 8 != m[F - 2]
                    and not any(b < F <= end for b, end, _ in per[i]))
    # the codes within two symbols of a span: of the source symbols around it, and of the output symbols in and around what it put in
    in_off, out_off = np.concatenate([[0], np.cumsum(ln)]), x.out_sym_off.astype(np.int64)
    near_in, near_out = np.zeros(int(in_off[-1]), dtype=bool), np.zeros(int(out_off[-1]), dtype=bool)
    for i, lst in enumerate(per):
        for b, end, _ in lst:
            if b < ln[i]:
                near_in[in_off[i] + max(b - 2, 0):in_off[i] + b] = True
                near_in[in_off[i] + min(end, ln[i]):in_off[i] + min(end + 2, ln[i])] = True
        for what, o, n, _, _ in batch_ref.splice_pieces(ln[i], lst, t.reps):
            if what == "rep":
                near_out[max(out_off[i] + o - 2, out_off[i]):min(out_off[i] + o + n + 2, out_off[i + 1])] = True
    used = [src.used[near_in], x.packed.used[near_out], x.cover.used[near_out]]
    s.update(table_spliced=sum(len(m) for m in x.spliced), table_cover_drops=int(x.cover.dropped.sum()), moved=moved, ends=ends,
             table_near=max(int(u.max()) for u in used if u.size))
    return s


def test_every_case_s_dictionary_spans_map_and_replacements():
    for s in edit_stats():
        case, e, w = s["case"], s["e"], s["case"].world()
        ln = [len(m) for m in w.messages]
        # the dictionary: within the automaton's and the hit budget, the named patterns in it
        assert 100 <= len(e.dictionary) <= 2000 and all(1 <= len(p) <= batch_ref.DICT_MAX_LEN for p in e.dictionary), case.id
        assert e.states <= batch_ref.DICT_MAX_STATES and 1 <= s["hits"] <= batch_ref.HIT_CAP, (case.id, e.states, s["hits"])
        assert s["seam255"] and s["nowhere"] >= 1 and s["duplicates"] >= 1, case.id
        if not s["at_end"]:      # one symbol nearly everywhere: the last 255 bytes of any stream, or all of it, hit too often
            hit = batch_ref._Counter(w.messages, e.fold)
            assert all(hit.count(m[-batch_ref.DICT_MAX_LEN:], batch_ref.HIT_CAP) > batch_ref.HIT_CAP for m in w.messages if m), case.id
        if case.source not in ("one", "two") and s["rarest"] <= 2000:    # (else the pattern's last byte alone is over the budget)
            assert s["family"] and e.special["family_whole"], case.id
        # the span list: valid, and no more spans than keep the spliced messages small
        for i, lst in enumerate(batch_ref.span_lists(e.span_off, e.spans)):
            assert all(b < t for b, t in lst) and all(lst[k][1] <= lst[k + 1][0] for k in range(len(lst) - 1)), (case.id, i)
        assert len(e.span_off) == len(ln) + 1 and int(e.span_off[-1]) == len(e.spans) <= batch_ref.SPAN_CAP, case.id
        # the map and the replacements
        assert e.map_kind in (batch_ref.MAP_KINDS[case.index % 6], "random") and len(e.byte_map) == 256, case.id
        assert e.reps[0] == b"" and 1 <= len(e.reps[1]) <= 255, case.id
        here = set(b"".join(w.messages))
        assert e.lacking is None or e.lacking not in here, case.id
        assert set(e.reps[1]) - here == ({e.lacking} if e.rep_lacks else set()), case.id
        if e.map_kind == "lacking":
            assert set(e.byte_map) - here == {e.lacking}, case.id
        if "spliced" in s:
            assert s["spliced"] <= batch_ref.SPLICED_BYTES, case.id
    assert count_edits(lambda s: s["at_end"]) >= 95
    assert count_edits(lambda s: s["family"] and s["e"].special["family_whole"]) >= 48
    for kind in batch_ref.MAP_KINDS:
        assert count_edits(lambda s: s["e"].map_kind == kind) >= 10, kind
    for k in (1, 2, 3, 64, 255):
        assert count_edits(lambda s: len(s["e"].reps[1]) == k) >= 5, k
    assert count_edits(lambda s: s["e"].rep_lacks) >= 10


def count_edits(pred, cases=lambda s: True):
    return sum(1 for s in edit_stats() if cases(s) and pred(s))


EDITS_DIGEST = "7688c5f6e1108deb796419bbe4d0073da90388920da09e93200d51b0e73f2acd"


def test_no_edits_moved_when_the_tables_were_added():
    """SHA-256 over every case's dictionary, replacements, byte map and span list, computed at the commit before Case.table()
    existed: the third part of a case draws from a generator of its own."""
    h = hashlib.sha256()
    for case in batch_ref.draw_cases():
        e = case.edits()
        case.table()                                                # (building it must not move anything either)
        h.update(repr((case.id, e.fold, e.map_kind, e.lacking, e.rep_lacks)).encode())
        for part in (e.dictionary, e.reps, [e.byte_map]):
            h.update(len(part).to_bytes(8, "little"))
            for m in part:
                h.update(len(m).to_bytes(8, "little") + bytes(m))
        for a in (e.span_off, e.spans):
            a = np.ascontiguousarray(a, dtype=np.uint64)
            h.update(a.size.to_bytes(8, "little") + a.tobytes())
    assert h.hexdigest() == EDITS_DIGEST


def test_every_case_s_table_and_tagged_list():
    for s in edit_stats():
        case, t, e = s["case"], s["t"], s["e"]
        here = set(b"".join(case.world().messages))
        assert 2 <= len(t.reps) <= 8 and t.reps[t.empty] == b"" and e.reps[1] in t.reps, case.id
        assert all(len(r) <= batch_ref.DICT_MAX_LEN for r in t.reps), case.id
        assert set(b"".join(t.reps)) - here <= ({e.lacking} if e.lacking is not None else set()), case.id
        assert s["well_formed"], case.id
        assert len(t.span_off) == case.n_streams + 1 and int(t.span_off[-1]) == len(t.spans) == len(t.tags) <= batch_ref.SPAN_CAP, case.id
        assert int(t.tags.max()) < len(t.reps), case.id
        want = splice_table_ref.merge_tagged(e.hit_off, e.records, e.hit_pattern)
        assert all(np.array_equal(a, b) for a, b in zip(t.merged, want)), case.id
        assert s["cover_drops"] == 0, case.id                       # the masked messages under the covering destination
        if splices(case):
            assert s["table_spliced"] <= batch_ref.SPLICED_BYTES and s["table_cover_drops"] == 0, case.id
    for k in (2, 8):
        assert count_edits(lambda s: len(s["t"].reps) == k) >= 5, k
    assert count_edits(lambda s: len(set(s["t"].reps)) < len(s["t"].reps)) >= 10                 # two equal entries
    assert count_edits(lambda s: s["e"].lacking is not None and any(s["e"].lacking in r for r in s["t"].reps)) >= 10
    assert count_edits(lambda s: s["t"].tags.size and len(set(s["t"].tags.tolist())) == len(s["t"].reps)) >= 48   # every entry in use


def test_coverage_of_the_tables_of_the_fixed_case_list():
    """What the table-splice families of the fuzz must keep reaching, from the references alone: every kind of insertion under
    both kernel families, and, under an order-2 source, the starts of output chunks and of lanes that the look-back has to get
    right."""
    plain = lambda s: 2 not in s["case"].orders
    o2 = lambda s: s["case"].orders[0] == 2
    assert count_edits(plain) == 64 and count_edits(o2) == 17
    assert count_edits(lambda s: s["case"].orders[1] == 2 and not o2(s)) == 15                  # the refusals
    for name in batch_ref.INSERTIONS:
        assert count_edits(lambda s: name in s["insertions"], plain) >= 10, name
        assert count_edits(lambda s: name in s["insertions"], o2) >= 4, name
    for name in batch_ref.OUTPUT_SEAMS:
        assert count_edits(lambda s: name in s["output_seams"], o2) >= 3, name
    assert count_edits(lambda s: s["case"].deep and s["table_near"] > 32, o2) >= 3
    assert count_edits(lambda s: s["moved"] > 0, o2) >= 12
    # the earlier of the two bytes reaches the output only through an order-2 destination (an order-0 / 1 one reads the later)
    assert count_edits(lambda s: s["ends"] > 0, o2) >= 8
    assert count_edits(lambda s: s["ends"] > 0, lambda s: s["case"].orders == (2, 2)) >= 4


def test_coverage_of_the_edits_of_the_fixed_case_list():
    """What the dictionary, span, edit and splice families of the fuzz must keep reaching, from the references alone."""
    plain = lambda s: 2 not in s["case"].orders                     # the cases that edit and splice (no order-2 side)
    assert count_edits(plain) == 64
    for name in batch_ref.PLACEMENTS:
        assert count_edits(lambda s: name in s["placements"], plain) >= 10, name
    assert count_edits(lambda s: s["emptied"], plain) >= 10         # a deletion empties a stream
    assert count_edits(lambda s: s["first_chunk"], plain) >= 10     # a deletion removes a first chunk: prev0 meets the byte behind
    assert count_edits(lambda s: s["grows"], plain) >= 10           # a replacement raises a chunk count
    assert count_edits(lambda s: s["drops"] > 0 and s["case"].dst_kind != "foreign", plain) >= 10
    assert count_edits(lambda s: s["case"].deep and s["near"] > 32, plain) >= 8
    assert count_edits(lambda s: s["case"].deep and s["near"] > 56, plain) >= 3
    # The matcher keeps the class map and as many rows of the transition table (csrc/mh_dict.h: trans u16[states x ncls]) as fit
    # into what the source's decode tables leave of the 160 KiB of LDS (csrc/mh_find.hip, launch_find_dict and launch_dict;
    # batch_ref.dict_rows_in_lds): both sides of that threshold under sources with deep codes
    deep = lambda s: s["case"].src_kind == "deep"
    assert count_edits(lambda s: s["rows"] < s["e"].states, deep) >= 6
    assert count_edits(lambda s: s["rows"] == s["e"].states, deep) >= 6
    assert count_edits(lambda s: s["rows"] == 0, deep) >= 1          # (tables that fill the LDS: no row, the class map from L2)


def test_the_new_files_leave_no_test_out():
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("batch_ref.py", "test_batch_ref.py", "test_gpu_batch_fuzz.py", "test_dict_abi.py", "edit_ref.py", "splice_ref.py", "find_ref.py",
                 "splice_table_ref.py", "edit_o2_ref.py", "test_edit_o2_ref.py", "test_gpu_workspace_reuse.py"):
        with open(os.path.join(here, name)) as f:
            text = f.read()
        for word in ("pytest.sk", "mark.sk", "importorsk", "xfa"):
            assert word + ("ip" if word.endswith("k") else "il") not in text, (name, word)
