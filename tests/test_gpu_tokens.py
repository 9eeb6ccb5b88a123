"""Tokens from matched bytes on the GPU (include/mh.h, "TOKENS FROM MATCHED BYTES"): the replacement table that
mh_dev_span_tokens_batch computes from the spans of a compressed batch, against tests/token_ref.py on the original messages.
Every comparison is exact.  The device-call wrapper (dev_span_tokens) puts guards behind every output, fills the workspace
with 0xFF beforehand and asserts that nothing outside the results changed.

The batch is that of tests/test_gpu_splice.py: messages of 0, 1, 2, 255, 256, 257, 3 * 256 + 5 and about 1100 bytes, chunk 256,
under a shared order-0 model, a shared order-1 model, a model set and a shared order-2 model, each indexed and index-free."""
import os
import subprocess

import numpy as np
import pytest

import damage
import splice_table_ref
import token_ref
from conftest import ROOT, golden
from test_gpu_edit import CHUNK, Source, mhc, model_of, msgs  # noqa: F401  (mhc, msgs: fixtures)
from test_gpu_splice import BIG, LAST

pytestmark = pytest.mark.gpu

KEY = token_ref.KEY
KEY2 = bytes(range(1, 17))
EMAIL, IP, GONE = (b"<EMAIL:", 16, b">"), (b"<IP>", 0, b""), (b"", 0, b"")
FORMATS = [EMAIL, IP, GONE, (b"", 4, b"#")]
KINDS = ["o0", "o1", "set", "o2"]


class Source2:
    """The batch under a shared order-2 model, with the fields of test_gpu_edit.Source."""

    def __init__(self, mhc, msgs, chunk=CHUNK):
        self.mhc, self.msgs, self.each, self.chunk = mhc, [bytes(m) for m in msgs], False, chunk
        self.model = mhc.Model.from_counts(mhc.histogram_o2_batch(self.msgs), 2)
        self.payload, self.pay_off, self.nbits, self.index, self.sym_off = self.model.encode_batch_o2(self.msgs, chunk_symbols=chunk)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else dict(chunk_symbols=self.chunk)


@pytest.fixture(scope="module")
def sources(mhc, msgs):
    return {"o0": Source(mhc, msgs, order=0), "o1": Source(mhc, msgs, order=1), "set": Source(mhc, msgs, order=1, each=True),
            "o2": Source2(mhc, msgs)}


def tokens(src, indexed, off, sp, tg, formats=FORMATS, key=KEY, flags=0, payload=None, pay_off=None, nbits=None, **kw):
    return src.mhc.dev_span_tokens(src.model, src.payload if payload is None else payload, src.pay_off if pay_off is None else pay_off,
                                   src.nbits if nbits is None else nbits, off, sp, tg, formats, key, flags, **src.kw(indexed), **kw)


def check_table(mhc, got, entries, what, n_reps=None, with_bytes=True, status=None):
    w_off, w_bytes, w_tag = token_ref.table_arrays(entries, n_reps)
    assert np.array_equal(got["rep_off"], w_off), (what, got["rep_off"], w_off)
    assert np.array_equal(got["rep_tag"], w_tag), what
    if with_bytes:
        assert got["rep_bytes"].tobytes() == w_bytes.tobytes(), (what, got["rep_bytes"].tobytes(), w_bytes.tobytes())
    else:
        assert got["rep_bytes"] is None, what
    if status is None:
        assert got["rc"] == mhc.MH_OK and not got["status"].any(), (what, got["rc"], got["status"])
    else:
        assert got["status"].tolist() == status and got["rc"] != mhc.MH_OK, (what, got["status"], status)


def everywhere(mhc, sources, per, formats=FORMATS, key=KEY, flags=0, tags=True, kinds=KINDS):
    """The lists (per stream: (begin, end, tag)) through every source kind, indexed and index-free: the reference's table."""
    off, sp, tg = splice_table_ref.tagged_lists(per)
    entries = token_ref.table(sources["o1"].msgs, off, sp, tg if tags else None, formats, key, flags)
    for s in kinds:
        for indexed in (True, False):
            check_table(mhc, tokens(sources[s], indexed, off, sp, tg if tags else None, formats, key, flags), entries, (s, indexed))
    return entries


def only(n, i, lst):
    return [lst if k == i else [] for k in range(n)]


# ---- 1. span lengths: the SipHash word edges and the length byte ---------------------------------------------------------------------

def test_span_lengths_0_to_255(mhc, msgs, sources):
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 255]
    at, lst = 3, []
    for k in lens:
        lst.append((at, at + k, 0))
        at += k + 2
    assert at < len(msgs[LAST]) and [e - b for b, e, _ in lst] == lens
    entries = everywhere(mhc, sources, only(len(msgs), LAST, lst))
    assert len(set(entries)) == len(lens) and all(len(e) == 24 for e in entries)


# ---- 2. where a span lies -------------------------------------------------------------------------------------------------------------

def test_at_the_start_across_a_seam_and_over_a_whole_three_chunk_message(mhc, msgs, sources):
    n = len(msgs)
    assert len(msgs[BIG]) == 773 and 250 // CHUNK != 259 // CHUNK
    everywhere(mhc, sources, [[], [(0, 1, 0)], [(0, 2, 0)], [(0, 5, 0)], [(0, 5, 3)], [(0, 256, 0)], [(250, 260, 0)], [(0, 7, 0)]])
    everywhere(mhc, sources, only(n, BIG, [(0, 773, 0)]))                       # two seams, and the end of the message
    everywhere(mhc, sources, only(n, BIG, [(256, 512, 0), (512, 768, 0)]))      # from a boundary to a boundary
    everywhere(mhc, sources, only(n, LAST, [(k - 2, k + 2, 0) for k in range(256, len(msgs[LAST]), 256)]))


def test_ends_at_the_length_clipped_by_it_and_beyond_it(mhc, msgs, sources):
    n, L = len(msgs), len(msgs[LAST])
    e = everywhere(mhc, sources, [[(0, 4, 0), (9, 12, 0)], [(0, 1, 0), (1, 1, 0), (1, 9, 0)], [], [(250, 255, 0)], [(250, 256, 0)], [(250, 300, 0)],
                                  [(770, 773, 0), (773, 900, 0)], [(L - 3, L + 5000, 0), (L + 5000, L + 5001, 0)]])
    empty = token_ref.token(EMAIL, KEY, b"")
    assert e[0] == e[1] == e[3] == e[4] == e[9] == e[11] == empty               # begin >= len(x): the digest of the empty string
    assert e[6] == token_ref.token(EMAIL, KEY, msgs[4][250:256]) and e[7] == token_ref.token(EMAIL, KEY, msgs[5][250:257])


def test_two_spans_in_one_chunk_and_several_insertions_at_one_position(mhc, msgs, sources):
    n = len(msgs)
    everywhere(mhc, sources, only(n, BIG, [(300, 310, 0), (320, 333, 3), (333, 340, 0)]))
    e = everywhere(mhc, sources, only(n, BIG, [(10, 10, 1), (10, 10, 0), (10, 10, 3), (10, 12, 0), (12, 12, 1), (256, 256, 0), (256, 257, 0)]))
    assert e[0] == b"<IP>" and e[1] == token_ref.token(EMAIL, KEY, b"") and e[4] == b"<IP>"


# ---- 3. formats -----------------------------------------------------------------------------------------------------------------------

def test_formats_of_0_1_15_and_16_digits_empty_parts_and_255_bytes(mhc, msgs, sources):
    n = len(msgs)
    fm = [(b"", 0, b""), (b"", 1, b""), (b"p", 15, b""), (b"", 16, b"s"), (b"x" * 200, 16, b"y" * 39), (b"", 0, b"z" * 255), (b"q" * 255, 0, b"")]
    assert token_ref.formats_ok(fm) and [len(p) + h + len(s) for p, h, s in fm][4:] == [255, 255, 255]
    lst = [(20 + 10 * k, 25 + 10 * k, k) for k in range(len(fm))]
    e = everywhere(mhc, sources, only(n, LAST, lst), formats=fm)
    assert [len(x) for x in e] == [0, 1, 16, 17, 255, 255, 255]
    # 256 bytes: MH_ERR_ARG through mh_dev_status, nothing written
    off, sp, tg = splice_table_ref.tagged_lists(only(n, LAST, [(20, 25, 0)]))
    for bad in ([(b"x" * 200, 16, b"y" * 40)], [(b"", 0, b"z" * 256)], [(b"", 17, b"")], [EMAIL, (b"a" * 250, 6, b"")]):
        assert not token_ref.formats_ok(bad)
        for s, indexed in (("o1", True), ("o2", False)):
            got = tokens(sources[s], indexed, off, sp, tg, formats=bad, rep_cap=300)
            assert got["rc"] == mhc.MH_ERR_ARG and got["rep_bytes"].size == 0 and (got["rep_off"] == mhc.FIND_FILL).all(), (bad, s)
    # the offsets' own rules: fmt_off[0] != 0, a decreasing pair; and spans with no format
    hexd = np.array([16], dtype=np.uint8)
    for foff in ([1, 8, 9], [0, 8, 7]):
        got = tokens(sources["o1"], True, off, sp, tg, fmt_arrays=(np.array(foff, dtype=np.uint64), np.frombuffer(b"<EMAIL:>>", dtype=np.uint8), hexd), rep_cap=300)
        assert got["rc"] == mhc.MH_ERR_ARG and got["rep_bytes"].size == 0, foff
    got = tokens(sources["o1"], True, off, sp, None, formats=[], rep_cap=300)
    assert got["rc"] == mhc.MH_ERR_ARG and got["rep_bytes"].size == 0


def test_a_null_tag_array_means_format_0(mhc, msgs, sources):
    e = everywhere(mhc, sources, only(len(msgs), BIG, [(5, 9, 1), (254, 258, 2)]), tags=False, kinds=["o1", "o2"])
    assert all(x.startswith(b"<EMAIL:") for x in e)


# ---- 4. the digest's properties -----------------------------------------------------------------------------------------------------

def mixed_case_span(msg):
    for b in range(0, len(msg) - 12):
        w = msg[b:b + 12]
        if any(65 <= c <= 90 for c in w) and any(97 <= c <= 122 for c in w):
            return b
    raise AssertionError("no span of mixed case")


def test_fold_on_and_off_over_a_span_of_mixed_case(mhc, msgs, sources):
    b = mixed_case_span(msgs[LAST])
    per = only(len(msgs), LAST, [(b, b + 12, 0)])
    plain = everywhere(mhc, sources, per, flags=0)
    folded = everywhere(mhc, sources, per, flags=token_ref.FOLD)
    assert plain != folded
    assert folded[0] == token_ref.token(EMAIL, KEY, msgs[LAST][b:b + 12].lower()) and "%016x" % mhc.span_token_digest(KEY, msgs[LAST][b:b + 12], 1) in folded[0].decode()


def test_equal_bytes_give_equal_tokens_in_two_records_and_at_two_phases_and_another_key_gives_another(mhc, msgs, sources):
    word = b"the"
    where = [(i, m.find(word)) for i, m in enumerate(msgs) if m.find(word) >= 0]
    a = msgs[LAST].find(word)
    b = msgs[LAST].find(word, max(a + 3, 300))
    assert len(where) >= 2 and 0 <= a < b and a % 8 != b % 8 and a // CHUNK != b // CHUNK
    per = [[(m.find(word), m.find(word) + 3, 0)] if m.find(word) >= 0 and i != LAST else [] for i, m in enumerate(msgs)]
    per[LAST] = [(a, a + 3, 0), (b, b + 3, 0)]
    e = everywhere(mhc, sources, per)
    assert len(e) >= 3 and len(set(e)) == 1 and ("%016x" % mhc.span_token_digest(KEY, word)).encode() in e[0]
    other = everywhere(mhc, sources, per, key=KEY2, kinds=["o1"])
    assert len(set(other)) == 1 and other[0] != e[0]


# ---- 5. room --------------------------------------------------------------------------------------------------------------------------

def test_count_only_one_byte_short_and_more_spans_than_room(mhc, msgs, sources):
    n = len(msgs)
    per = only(n, BIG, [(0, 4, 0), (250, 260, 1), (300, 300, 3), (500, 773, 0)])
    off, sp, tg = splice_table_ref.tagged_lists(per)
    entries = token_ref.table(msgs, off, sp, tg, FORMATS, KEY)
    total = sum(len(e) for e in entries)
    for s in KINDS:
        for indexed in (True, False):
            src, what = sources[s], (s, indexed)
            check_table(mhc, tokens(src, indexed, off, sp, tg, count_only=True), entries, what, with_bytes=False)
            check_table(mhc, tokens(src, indexed, off, sp, tg, rep_cap=total), entries, what)
            check_table(mhc, tokens(src, indexed, off, sp, tg, rep_cap=total + 7, n_reps=9), entries, what, n_reps=9)   # a table with room to spare
            short = tokens(src, indexed, off, sp, tg, rep_cap=total - 1)
            assert short["rc"] == mhc.MH_ERR_CAPACITY and short["rep_bytes"].size == 0, what
            assert np.array_equal(short["rep_off"], token_ref.table_arrays(entries)[0]) and not short["status"].any(), what
            # more spans than table entries: the call stops
            few = tokens(src, indexed, off, sp, tg, rep_cap=total, n_reps=3)
            assert few["rc"] == mhc.MH_ERR_CAPACITY and few["rep_bytes"].size == 0, what
    # a workspace sized for fewer entries than the table has is refused before any launch
    with pytest.raises(mhc.MhError) as e:
        tokens(sources["o1"], True, off, sp, tg, n_reps=5000, ws_n_reps=3)
    assert e.value.status == mhc.MH_ERR_CAPACITY


# ---- 6. verdicts ----------------------------------------------------------------------------------------------------------------------

def test_a_malformed_list_and_a_tag_without_a_format_each_fail_their_stream_alone(mhc, msgs, sources):
    n = len(msgs)
    good = [[(0, 4, 0)], [(0, 1, 1)], [], [(3, 9, 0)], [(250, 256, 3)], [(0, 2, 0), (254, 257, 0)], [(100, 101, 0), (250, 520, 0)], [(5, 6, 0)]]
    for bad_at, bad in ((BIG, [(5, 4, 0)]), (BIG, [(20, 30, 0), (10, 15, 0)]), (BIG, [(0, 3, 0), (3, 9, 0), (8, 12, 0)]), (BIG, [(2, 5, 0), (2, 2, 0)]),
                        (3, [(3, 9, len(FORMATS))]), (LAST, [(5, 6, 0), (7, 8, 0xFFFFFFFF)])):
        per = list(good)
        per[bad_at] = bad
        off, sp, tg = splice_table_ref.tagged_lists(per)
        ok = list(per)
        ok[bad_at] = [(0, 0, 0)] * len(bad)                                      # (a stand-in of the same length; its entries are empty)
        o2, s2, t2 = splice_table_ref.tagged_lists(ok)
        entries = token_ref.table(msgs, o2, s2, t2, FORMATS, KEY, failed={bad_at})
        status = [mhc.MH_OK] * n
        status[bad_at] = mhc.MH_ERR_ARG
        for s in KINDS:
            for indexed in (True, False):
                check_table(mhc, tokens(sources[s], indexed, off, sp, tg), entries, (bad, s, indexed), status=status)


def decoder_status(src, indexed, payload, pay_off, nbits):
    """What the source's batch decoder says about every stream of the batch."""
    if src.each:
        return src.model.decode(payload, pay_off, nbits, **src.kw(indexed))[2].tolist()
    fn = src.model.decode_batch_o2 if isinstance(src, Source2) else src.model.decode_batch
    return fn(payload, pay_off, nbits, check=False, **src.kw(indexed))[2].tolist()


@pytest.mark.parametrize("s", KINDS)
def test_a_stream_cut_inside_a_code_has_the_decoders_verdict_and_empty_entries(mhc, msgs, sources, s):
    src, n = sources[s], len(msgs)
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    nb = int(src.nbits[BIG])
    per = [[(0, 4, 0)], [(0, 1, 1)], [], [(3, 9, 0)], [(250, 256, 3)], [(0, 2, 0)], [(3, 9, 0), (700, 773, 0)], [(5, 6, 0), (300, 310, 0)]]
    off, sp, tg = splice_table_ref.tagged_lists(per)
    entries = token_ref.table(msgs, off, sp, tg, FORMATS, KEY, failed={BIG})
    for indexed in (True, False):
        # the shortest cut that the decoder refuses: one that ends inside a code (a cut on a code boundary is a valid shorter
        # stream for the index-free decoder)
        for k in range(1, 16):
            pls, nbs = list(streams), [int(x) for x in src.nbits]
            pls[BIG], nbs[BIG] = damage.cut(streams[BIG], nb, nb - k), nb - k
            payload, pay_off = mhc.batch_offsets(pls)
            want = decoder_status(src, indexed, payload, pay_off, nbs)
            if want[BIG] != mhc.MH_OK:
                break
        assert want[BIG] == mhc.MH_ERR_CORRUPT and [w for i, w in enumerate(want) if i != BIG] == [mhc.MH_OK] * (n - 1), (s, indexed, want)
        got = tokens(src, indexed, off, sp, tg, payload=payload, pay_off=pay_off, nbits=nbs)
        check_table(mhc, got, entries, (s, indexed, k), status=want)


def test_streams_without_spans_are_not_decoded(mhc, msgs, sources):
    """The header says so: a damaged stream that no span names keeps MH_OK."""
    src, n = sources["o1"], len(msgs)
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    nb = int(src.nbits[BIG])
    streams[BIG] = damage.flip(streams[BIG], nb // 2)
    payload, pay_off = mhc.batch_offsets(streams)
    per = only(n, LAST, [(5, 9, 0)])
    off, sp, tg = splice_table_ref.tagged_lists(per)
    for indexed in (True, False):
        check_table(mhc, tokens(src, indexed, off, sp, tg, payload=payload, pay_off=pay_off), token_ref.table(msgs, off, sp, tg, FORMATS, KEY), indexed)


def test_damage_in_a_chunk_that_no_span_touches_is_not_seen_under_an_index(mhc, msgs, sources):
    """The header: an indexed stream with spans is judged on the chunks its spans touch.  A flipped bit in the third chunk of
    the 773-byte stream, a span in its first: the batch decoder refuses the stream, the token call does not see the damage."""
    src, n = sources["o1"], len(msgs)
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    base = int(src.sym_off[BIG]) // CHUNK + BIG
    third = int(src.index[base + 2]) & mhc.INDEX_BIT_MASK
    assert int(src.index[base + 1]) & mhc.INDEX_BIT_MASK < third < int(src.nbits[BIG]) - 8
    per = only(n, BIG, [(3, 9, 0), (200, 256, 0)])
    off, sp, tg = splice_table_ref.tagged_lists(per)
    entries = token_ref.table(msgs, off, sp, tg, FORMATS, KEY)
    refused = 0
    for bit in range(third + 1, third + 6):
        pls = list(streams)
        pls[BIG] = damage.flip(streams[BIG], bit)
        payload, pay_off = mhc.batch_offsets(pls)
        refused += decoder_status(src, True, payload, pay_off, src.nbits)[BIG] == mhc.MH_ERR_CORRUPT
        check_table(mhc, tokens(src, True, off, sp, tg, payload=payload, pay_off=pay_off), entries, bit)
    assert refused >= 1                                                        # (the damage is real: the decoder sees it)


def long_batch(mhc):
    """Two streams under one order-1 model, the second over MH_BATCH_WALK_MAX_BITS: (model, messages, coded batch)."""
    text = golden()["input_wiki_cpp.txt"]["data"]
    recs = [text[:3000], (text * (2_600_000 // len(text) + 1))[:2_600_000]]
    model = model_of(mhc, recs, 1)
    payload, pay_off, nbits, index, sym_off = model.encode_batch(recs, chunk_symbols=1024)
    assert int(nbits[1]) > mhc.BATCH_WALK_MAX_BITS > int(nbits[0])
    return model, recs, (payload, pay_off, nbits)


def test_the_host_form_indexes_an_over_long_index_free_stream_first(mhc):
    model, recs, (payload, pay_off, nbits) = long_batch(mhc)
    L = len(recs[1])
    per = [[(5, 9, 0), (100, 100, 1)], [(0, 4, 0), (1023, 1030, 0), (L // 2, L // 2 + 255, 3), (L - 3, L + 9, 0), (L + 9, L + 10, 1)]]
    off, sp, tg = splice_table_ref.tagged_lists(per)
    w_off, w_bytes, w_tag = token_ref.table_arrays(token_ref.table(recs, off, sp, tg, FORMATS, KEY))
    roff, rb, rtag, st, rc = mhc.span_tokens_batch(model, payload, pay_off, nbits, off, sp, tg, FORMATS, KEY)
    assert rc == mhc.MH_OK and not st.any() and np.array_equal(roff, w_off) and rb.tobytes() == w_bytes.tobytes() and np.array_equal(rtag, w_tag)
    # the long stream cut inside a code: the indexing fails it, its entries are empty, its neighbour's are untouched
    streams = [bytes(payload[int(pay_off[i]):int(pay_off[i + 1])]) for i in range(2)]
    for k in range(1, 16):
        cut = [streams[0], damage.cut(streams[1], int(nbits[1]), int(nbits[1]) - k)]
        p2, o2 = mhc.batch_offsets(cut)
        nb2 = np.array([int(nbits[0]), int(nbits[1]) - k], dtype=np.uint64)
        roff, rb, rtag, st, rc = mhc.span_tokens_batch(model, p2, o2, nb2, off, sp, tg, FORMATS, KEY)
        if rc != mhc.MH_OK:
            break
    w_off, w_bytes, _ = token_ref.table_arrays(token_ref.table(recs, off, sp, tg, FORMATS, KEY, failed={1}))
    assert rc == mhc.MH_ERR_CORRUPT and st.tolist() == [mhc.MH_OK, mhc.MH_ERR_CORRUPT], (k, rc, st)
    assert np.array_equal(roff, w_off) and rb.tobytes() == w_bytes.tobytes(), (roff, w_off)


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", KINDS)
def test_tokens_then_the_table_splice_under_another_model_then_decode(mhc, msgs, sources, s):
    src, n = sources[s], len(msgs)
    per = [[(0, 4, 0)], [(0, 1, 1)], [(1, 1, 0)], [(3, 9, 0), (9, 9, 1)], [(250, 256, 3)], [(0, 2, 2), (254, 257, 0)], [(100, 101, 0), (250, 520, 0), (770, 5000, 0)],
           [(5, 6, 1), (255, 257, 0), (600, 600, 0)]]
    off, sp, tg = splice_table_ref.tagged_lists(per)
    want = token_ref.apply(msgs, off, sp, tg, FORMATS, KEY, token_ref.FOLD)
    dst = model_of(mhc, list(msgs) + want, 1)                                   # codes for every pair of the scrubbed messages
    for indexed in (True, False):
        t = tokens(src, indexed, off, sp, tg, flags=token_ref.FOLD)
        assert t["rc"] == mhc.MH_OK
        reps = [t["rep_bytes"][int(a):int(b)].tobytes() for a, b in zip(t["rep_off"][:-1], t["rep_off"][1:])]
        args = (dst, src.payload, src.pay_off, src.nbits, t["rep_tag"], reps, off, sp)
        if s == "set":
            got = src.model.recode_splice_table(*args, **src.kw(indexed))
        elif s == "o2":
            got = src.model.dev_recode_splice_table_batch_o2(*args, **src.kw(indexed))
        else:
            got = src.model.dev_recode_splice_table_batch(*args, **src.kw(indexed))
        assert got["rc"] == mhc.MH_OK and not got["status"].any() and not got["dropped"].any(), (s, indexed)
        back, so, st = dst.decode_batch(got["payload"], got["out_off"], got["nbits"], sym_off=got["out_sym_off"], index=got["index"], chunk_symbols=CHUNK)
        assert back == b"".join(want) and np.array_equal(so, splice_table_ref.offsets(want)), (s, indexed)


# ---- 8. the host form and the CLI -----------------------------------------------------------------------------------------------------

def test_the_host_form_on_a_golden_text(mhc):
    text = golden()["input_wiki_cpp.txt"]["data"]
    recs = [l for l in text.split(b"\n") if l][:60]
    model = model_of(mhc, recs, 1)
    word = b"the"
    per = []
    for m in recs:
        lst, at = [], m.find(word)
        while at >= 0:
            lst.append((at, at + 3, 0))
            at = m.find(word, at + 3)
        per.append(lst + [(len(m) + 2, len(m) + 4, 1)])
    off, sp, tg = splice_table_ref.tagged_lists(per)
    assert len(sp) > 80
    entries = token_ref.table(recs, off, sp, tg, FORMATS, KEY)
    w_off, w_bytes, w_tag = token_ref.table_arrays(entries)
    for chunk in (256, 0):
        payload, pay_off, nbits, index, sym_off = model.encode_batch(recs, chunk_symbols=256)
        kw = dict(sym_off=sym_off, index=index, chunk_symbols=256) if chunk else {}
        roff, rb, rtag, st, rc = mhc.span_tokens_batch(model, payload, pay_off, nbits, off, sp, tg, FORMATS, KEY, **kw)
        assert rc == mhc.MH_OK and not st.any() and np.array_equal(roff, w_off) and rb.tobytes() == w_bytes.tobytes() and np.array_equal(rtag, w_tag), chunk
        roff, rb, rtag, st, rc = mhc.span_tokens_batch(model, payload, pay_off, nbits, off, sp, tg, FORMATS, KEY, rep_cap=len(w_bytes) - 1, **kw)
        assert rc == mhc.MH_ERR_CAPACITY and np.array_equal(roff, w_off), chunk


def test_the_cli_with_a_token_key_on_a_golden_text(mhc, tmp_path):
    from conftest import expected_file
    from oracle import mh_oracle
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    x = "input_wiki_cpp.txt"
    data = golden()[x]["data"]
    p = lambda name: str(tmp_path / name)
    pats = [b"language", b"age", b"the ", b"C++"]
    lines = [b"<L:%H>", b"", b"<the %4H %H> ", b"<CPP>"]                         # a full token, a deletion, four digits (a later %H is literal), a constant
    formats = [(b"<L:", 16, b">"), (b"", 0, b""), (b"<the ", 4, b" %H> "), (b"<CPP>", 0, b"")]
    for name, blob in (("x", data), ("x.e", expected_file(x, "e")), ("pats", b"\n".join(pats) + b"\n"), ("reps", b"\n".join(lines) + b"\n")):
        with open(p(name), "wb") as f:
            f.write(blob)
    run = lambda a: subprocess.run([cli] + a, capture_output=True, timeout=300)
    rows = sorted((at + len(pt), j, at) for j, pt in enumerate(pats) for at in range(len(data)) if data.lower().startswith(pt.lower(), at))
    off = np.array([0, len(rows)], dtype=np.uint64)
    so, sp, tg = splice_table_ref.merge_tagged(off, [(0, b, e) for e, _, b in rows], [j for _, j, _ in rows])
    text = token_ref.apply([data], so, sp, tg, formats, KEY, token_ref.FOLD)[0]
    literal = splice_table_ref.apply([data], so, sp, tg, lines)[0]
    assert len(sp) > 20 and len(set(tg.tolist())) == 4 and b"<L:%H>" in literal and b"%H" not in text.replace(b" %H> ", b"")
    both = model_of(mhc, [data, text, literal], 1).table_bytes()
    with open(p("both.e"), "wb") as f:
        f.write(both)
    assert run([p("x"), "-e", p("x.e"), "-o", p("x.cm"), "--index", p("x.idx"), "--chunk", "256"]).returncode == 0
    common = [p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("both.e"), "--redact-file", p("pats"), "--redact-fold", "--replace-file", p("reps")]
    for indexed in (True, False):
        more = ["--index", p("x.idx")] if indexed else []
        r = run(common + more + ["-o", p("out.cm"), "--token-key", KEY.hex()])
        assert r.returncode == 0 and b"skipped" not in r.stderr, r.stderr
        assert open(p("out.cm"), "rb").read() == mh_oracle.Model.from_table(both).compress(text)[0], indexed
        removed, inserted = int((sp[:, 1] - sp[:, 0]).sum()), len(text) - len(data) + int((sp[:, 1] - sp[:, 0]).sum())
        assert ("Replacing %d bytes in %d spans with %d bytes." % (removed, len(sp), inserted)).encode() in r.stderr, r.stderr
        # without the key every string stays literal, byte for byte as before
        r = run(common + more + ["-o", p("lit.cm")])
        assert r.returncode == 0 and open(p("lit.cm"), "rb").read() == mh_oracle.Model.from_table(both).compress(literal)[0], (indexed, r.stderr)
    # one --replace string with the key: every span under one format
    one = token_ref.apply([data], so, sp, None, [(b"[", 8, b"]")], KEY, token_ref.FOLD)[0]
    with open(p("one.e"), "wb") as f:
        f.write(model_of(mhc, [data, one], 1).table_bytes())
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("one.e"), "--redact-file", p("pats"), "--redact-fold", "--replace", "[%8H]", "-o", p("one.cm"),
             "--token-key", KEY.hex().upper()])
    assert r.returncode == 0 and open(p("one.cm"), "rb").read() == mh_oracle.Model.from_table(open(p("one.e"), "rb").read()).compress(one)[0], r.stderr
