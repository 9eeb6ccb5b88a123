"""Splicing re-coding on the GPU (include/mh.h, "SPLICING BATCHES"): a batch coded again with every span deleted or replaced by
one string of another length, the bytes never written.  The reference is tests/splice_ref.py on top of tests/recode_ref.py (the
CPU oracle's encoder on the spliced messages); every comparison is exact.  The device-call wrappers put guards around every
output and assert that nothing outside the results changed.

chunk_symbols is 256 (MH_CHUNK_MIN) and the batch that of tests/test_gpu_edit.py: messages of 0, 1, 2, 255, 256, 257,
3 * 256 + 5 and about 1100 bytes.  Replacements of 0, 1, 10 and 255 bytes: a deletion, the shortest, a marker, the longest."""
import os
import subprocess

import numpy as np
import pytest

import damage
import edit_ref
import find_ref
import recode_ref
import splice_ref
from conftest import ROOT, expected_file, golden
from oracle import mh_oracle
from test_gpu_edit import CHUNK, Source, mhc, model_of, msgs, oracle_of, slices_of, span_lists  # noqa: F401  (mhc, msgs: fixtures)
from test_gpu_stream_order import Batch, Chain, drive, env, ptr, same  # noqa: F401  (env: the fixture of the stream chains)

pytestmark = pytest.mark.gpu

BIG, LAST = 6, 7                                                                # the 773-byte message (chunks at 256, 512, 768), the long one


def reps():
    text = golden()["input_wiki_cpp.txt"]["data"]
    r = {0: b"", 1: b"#", 10: b"[REDACTED]", 255: text[9000:9255]}
    assert [len(v) for v in r.values()] == [0, 1, 10, 255]
    return r


REPS = reps()


@pytest.fixture(scope="module")
def sources(mhc, msgs):
    """Shared order 0, shared order 1 and a model set."""
    return {"o0": Source(mhc, msgs, order=0), "o1": Source(mhc, msgs, order=1), "set": Source(mhc, msgs, order=1, each=True)}


@pytest.fixture(scope="module")
def dsts(mhc, msgs, sources):
    """The source model itself and another model that covers the text and the replacements."""
    text = golden()["input_wiki_cpp.txt"]["data"]
    return {"same": sources["o1"].model, "other": model_of(mhc, [text, b" [REDACTED] # [REDACTED]#"], 1), "other0": model_of(mhc, [text, b"[REDACTED]#"], 0)}


def splice(src, dst, rep, span_off, spans, indexed, payload=None, pay_off=None, nbits=None, index=None, **kw):
    fn = src.model.recode_splice if src.each else src.model.dev_recode_splice_batch
    k = src.kw(indexed)
    if index is not None:
        k["index"] = index
    return fn(dst, *src.batch(payload, pay_off, nbits), rep, span_off, spans, **k, **kw)


def expect(src, dst, rep, span_off, spans):
    """What the splice must give: the oracle's encode, under dst, of the spliced messages."""
    y = splice_ref.apply(src.msgs, span_off, spans, rep)
    ref = recode_ref.recode(y, oracle_of(dst), src.chunk)
    return y, ref, recode_ref.packed(ref)


def check_exact(mhc, src, got, y, ref, packed, what, payload=True, index=True):
    r_pay, r_off, r_nb, r_drop = packed
    oso = splice_ref.offsets(y)
    assert got["rc"] == mhc.MH_OK and (got["status"] == mhc.MH_OK).all(), (what, got["rc"], got["status"])
    assert np.array_equal(got["out_sym_off"], oso), (what, got["out_sym_off"], oso)
    assert np.array_equal(got["out_off"], r_off) and np.array_equal(got["nbits"], r_nb), what
    assert np.array_equal(got["dropped"], r_drop), (what, got["dropped"], r_drop)
    assert np.array_equal(got["sym_off"], src.sym_off), what
    if payload:
        assert np.array_equal(got["payload"], r_pay), what
    else:
        assert got["payload"] is None, what
    if index:
        want = np.concatenate([r[3] for r in ref]) if ref else np.zeros(0, dtype=np.uint64)
        assert np.array_equal(slices_of(got["index"], oso, src.chunk), want), what        # the slots computed from len(y)
    else:
        assert got["index"] is None, what


# ---- 1. the span placements of the issue, at every replacement length ----------------------------------------------------------------

def placements(msgs):
    """name -> (per-stream span lists, a check on the geometry: the case really occurs)."""
    n, L = len(msgs), len(msgs[LAST])
    ln = [len(m) for m in msgs]

    def only(i, lst):
        return [lst if k == i else [] for k in range(n)]
    assert ln[:7] == [0, 1, 2, 255, 256, 257, 773] and L > 1024
    C = CHUNK
    return {
        "inside one chunk": (only(BIG, [(300, 310)]), lambda: 300 // C == 309 // C),
        "across a seam": (only(BIG, [(250, 260)]), lambda: 250 // C != 259 // C),
        # the lane of chunk 1 produces nothing, the lane of chunk 2 starts inside a span whose begin is mid-chunk
        "one lane produces nothing": (only(BIG, [(200, 600)]), lambda: 200 % C and 200 <= 1 * C and 2 * C <= 600 and (2 * C - 1) in range(200, 600)),
        "touching on a chunk boundary": (only(BIG, [(250, 256), (256, 300)]), lambda: 256 % C == 0),
        # the lane of chunk 2 starts behind a run of three touching spans that begins mid-chunk; in the last stream one run
        # begins at 0 (prev0) and one span begins on a boundary and reaches over the next (the entry's byte)
        "runs of touching spans": ([[] for _ in range(BIG)] + [[(200, 256), (256, 512), (512, 600)], [(0, 256), (256, 300), (512, 800)]],
                                   lambda: 600 > 2 * C and 300 > C and 512 % C == 0 and 800 > 3 * C),
        "from 0": (only(BIG, [(0, 5)]), lambda: True),
        "to exactly the length": (only(BIG, [(770, 773)]), lambda: ln[BIG] == 773),
        "clipped by the length": (only(BIG, [(770, 5000)]), lambda: ln[BIG] < 5000),
        "wholly beyond the length": ([[(0, 4), (9, 12)]] + [[] for _ in range(BIG - 1)] + [[(773, 900)], [(L, L + 1)]], lambda: ln[0] == 0 and ln[BIG] == 773),
        "every message whole": ([[(0, max(k, 1))] for k in ln], lambda: True),
        "the 1- and 2-byte messages": ([[], [(0, 1)], [(1, 2)]] + [[] for _ in range(n - 3)], lambda: ln[1] == 1 and ln[2] == 2),
        "the 2-byte message, first byte": ([[], [], [(0, 1)]] + [[] for _ in range(n - 3)], lambda: ln[2] == 2),
        # 255 + 10 - 1 bytes: one chunk becomes two; 256 bytes with 16 one-byte spans: at 255 bytes each, one chunk becomes 17
        "growth across a chunk count": ([[], [], [], [(100, 101)], [(k, k + 1) for k in range(0, 256, 16)]] + [[] for _ in range(n - 5)],
                                        lambda: (255 - 1 + 10) > C and (256 - 16 + 16 * 255) // C == 16),
        "across every seam of the last stream": (only(LAST, [(k - 2, k + 2) for k in range(256, L, 256)] + [(L - 1, L + 1)]), lambda: L > 4 * C),
    }


PLACEMENTS = ["inside one chunk", "across a seam", "one lane produces nothing", "touching on a chunk boundary", "runs of touching spans", "from 0",
              "to exactly the length", "clipped by the length", "wholly beyond the length", "every message whole", "the 1- and 2-byte messages",
              "the 2-byte message, first byte", "growth across a chunk count", "across every seam of the last stream"]


@pytest.mark.parametrize("rep_len", [0, 1, 10, 255])
@pytest.mark.parametrize("name", PLACEMENTS)
def test_span_placements(mhc, msgs, sources, dsts, name, rep_len):
    per, occurs = placements(msgs)[name]
    assert occurs(), name
    span_off, spans = span_lists(per)
    rep = REPS[rep_len]
    for s in ("o0", "o1", "set"):
        src = sources[s]
        for d in ("same", "other") if s != "o0" else ("other", "other0"):
            y, ref, packed = expect(src, dsts[d], rep, span_off, spans)
            for indexed in (True, False):
                check_exact(mhc, src, splice(src, dsts[d], rep, span_off, spans, indexed), y, ref, packed, (name, rep_len, s, d, indexed))
    ln = [len(m) for m in y]
    if name == "one lane produces nothing":
        assert ln[BIG] == 773 - 400 + rep_len
    if name == "every message whole":
        assert ln == [0] + [rep_len] * 7 and (rep_len or not packed[2].any())       # a deletion: every stream becomes empty
    if name == "wholly beyond the length":
        assert y == src.msgs
    if name == "growth across a chunk count" and rep_len >= 10:
        assert (ln[3] + CHUNK - 1) // CHUNK == 2 and (rep_len < 255 or (ln[4] + CHUNK - 1) // CHUNK == 17)
        assert len(ref[3][3]) == 2


def test_a_replacement_with_a_pair_without_a_code_is_dropped_as_the_reference_drops_it(mhc, msgs, sources, dsts):
    assert not any(0x07 in m for m in msgs)
    rep = b"a\x07\x07b"
    span_off, spans = span_lists([[], [(0, 1)], [(1, 2)], [(10, 13)], [(253, 256)], [(0, 2), (254, 257)], [(100, 101), (250, 520)], [(5, 6)]])
    for s, d in (("o1", "same"), ("o1", "other"), ("set", "other"), ("o0", "other")):
        src = sources[s]
        y, ref, packed = expect(src, dsts[d], rep, span_off, spans)
        assert (packed[3][1:] >= 3).all()                                       # (a, 7), (7, 7), (7, b) of every replacement
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, dsts[d], rep, span_off, spans, indexed), y, ref, packed, ("no code", s, d, indexed))


# ---- 2. nothing to splice: the plain re-code, byte for byte ---------------------------------------------------------------------------

@pytest.mark.parametrize("s", ["o0", "o1", "set"])
@pytest.mark.parametrize("indexed", [True, False])
def test_the_empty_list_equals_the_plain_recode(mhc, msgs, sources, dsts, indexed, s):
    src, dst = sources[s], dsts["other"]
    plain = src.recode(dst, indexed)
    empty = span_lists([[] for _ in msgs])
    for rep_len in (0, 10):
        got = splice(src, dst, REPS[rep_len], *empty, indexed)
        for k in ("payload", "out_off", "nbits", "dropped", "status", "sym_off"):
            assert np.array_equal(got[k], plain[k]), (rep_len, k)
        assert np.array_equal(got["out_sym_off"], src.sym_off) and got["rc"] == plain["rc"] == mhc.MH_OK
        assert np.array_equal(got["index"], plain["index"][:len(got["index"])]), rep_len


# ---- 3. round trip, hits to spans to splice, count only -------------------------------------------------------------------------------

def hit_spans(msgs, pats):
    hits = find_ref.find_hits(msgs, pats)
    w_off, w_rec, _ = find_ref.hit_arrays(hits, len(msgs))
    return w_off, w_rec, edit_ref.merge_hits(w_off, w_rec)


@pytest.mark.parametrize("rep_len", [0, 10])
def test_find_spans_splice_decode(mhc, msgs, rep_len):
    pats = [b"in", b"ng", b"ing "]
    rep = REPS[rep_len]
    w_off, w_rec, (r_so, r_sp) = hit_spans(msgs, pats)
    assert len(r_sp) >= 10
    y = splice_ref.apply(msgs, r_so, r_sp, rep)
    model = model_of(mhc, list(msgs) + y, 1)                                    # codes for every pair of y: nothing is dropped
    src = Source(mhc, msgs, model=model)
    ho, rec, _, st, rc = model.dev_find_batch(mhc.PatternSet(pats), src.payload, src.pay_off, src.nbits, **src.kw(True))
    assert rc == mhc.MH_OK and np.array_equal(ho, w_off) and np.array_equal(rec, w_rec)
    d_so, d_sp, rc = mhc.dev_spans_from_hits(ho, rec)
    assert rc == mhc.MH_OK and np.array_equal(d_so, r_so) and np.array_equal(d_sp, r_sp)
    y2, ref, packed = expect(src, model, rep, d_so, d_sp)
    assert y2 == y and not packed[3].any()
    for indexed in (True, False):
        got = splice(src, model, rep, d_so, d_sp, indexed)
        check_exact(mhc, src, got, y, ref, packed, (rep_len, indexed))
        back, so, st = model.decode_batch(got["payload"], got["out_off"], got["nbits"], sym_off=got["out_sym_off"], index=got["index"],
                                          chunk_symbols=CHUNK)
        assert back == b"".join(y) and np.array_equal(so, got["out_sym_off"])
        ho2, rec2, _, st2, rc2 = model.dev_find_batch(mhc.PatternSet(pats), got["payload"], got["out_off"], got["nbits"], sym_off=got["out_sym_off"],
                                                      index=got["index"], chunk_symbols=CHUNK)
        want2 = find_ref.hit_arrays(find_ref.find_hits(y, pats), len(y))
        assert rc2 == mhc.MH_OK and np.array_equal(ho2, want2[0]) and np.array_equal(rec2, want2[1])


@pytest.mark.parametrize("s", ["o1", "set"])
def test_count_only_gives_the_sizes_of_the_full_call(mhc, msgs, sources, dsts, s):
    src, dst = sources[s], dsts["other"]
    per, _ = placements(msgs)["runs of touching spans"]
    span_off, spans = span_lists(per)
    for rep_len in (0, 255):
        for indexed in (True, False):
            full = splice(src, dst, REPS[rep_len], span_off, spans, indexed)
            y, ref, packed = expect(src, dst, REPS[rep_len], span_off, spans)
            check_exact(mhc, src, full, y, ref, packed, (rep_len, indexed))
            count = splice(src, dst, REPS[rep_len], span_off, spans, indexed, count_only=True, want_index=False)
            check_exact(mhc, src, count, y, ref, packed, (rep_len, indexed, "count only"), payload=False, index=False)
            nidx = int(full["out_sym_off"][-1]) // CHUNK + len(msgs)
            count = splice(src, dst, REPS[rep_len], span_off, spans, indexed, count_only=True, index_cap=nidx)
            check_exact(mhc, src, count, y, ref, packed, (rep_len, indexed, "count only, index"), payload=False)


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indexed", [True, False])
def test_a_cap_one_byte_short_and_an_index_one_entry_short(mhc, msgs, sources, dsts, indexed):
    src, dst = sources["o1"], dsts["other"]
    per, _ = placements(msgs)["growth across a chunk count"]
    span_off, spans = span_lists(per)
    rep = REPS[255]
    full = splice(src, dst, rep, span_off, spans, indexed)
    need, nidx = int(full["out_off"][-1]), int(full["out_sym_off"][-1]) // CHUNK + len(msgs)
    assert full["rc"] == mhc.MH_OK and len(full["index"]) == nidx
    for what, kw in (("cap", dict(cap=need - 1, index_cap=nidx)), ("index_cap", dict(cap=need, index_cap=nidx - 1))):
        short = splice(src, dst, rep, span_off, spans, indexed, **kw)               # (the wrapper asserts the guards and the fills)
        assert short["rc"] == mhc.MH_ERR_CAPACITY and short["payload"].size == 0, what
        assert (short["index"] == mhc.FIND_FILL).all(), what
        for k in ("out_off", "nbits", "dropped", "status", "out_sym_off", "sym_off"):
            assert np.array_equal(short[k], full[k]), (what, indexed, k)
    roomy = splice(src, dst, rep, span_off, spans, indexed, cap=need + 100, index_cap=nidx + 3)
    assert roomy["rc"] == mhc.MH_OK and np.array_equal(roomy["payload"], full["payload"]) and np.array_equal(roomy["index"][:nidx], full["index"])
    # a deletion whose workspace was sized for fewer spans than the list holds
    many = splice(src, dst, b"", span_off, spans, True, n_spans=len(spans))
    few = splice(src, dst, b"", span_off, spans, True, n_spans=0, count_only=True, want_index=False)
    assert many["rc"] == mhc.MH_OK
    ws = mhc.lib().mh_dev_recode_splice_workspace
    if ws(len(msgs), int(src.sym_off[-1]), CHUNK, 0) == ws(len(msgs), int(src.sym_off[-1]), CHUNK, len(spans)):
        assert few["rc"] == mhc.MH_OK                                             # (the rounding of the workspace left room)
    else:
        assert few["rc"] == mhc.MH_ERR_CAPACITY and not few["nbits"].any()


# ---- 5. failed streams ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rep_len", [0, 10])
@pytest.mark.parametrize("indexed", [True, False])
def test_a_malformed_list_and_a_damaged_stream_fail_alone(mhc, msgs, sources, dsts, indexed, rep_len):
    src, dst, rep = sources["o1"], dsts["other"], REPS[rep_len]
    n = len(msgs)
    good = [[], [(0, 1)], [(1, 2)], [(10, 13)], [(250, 256)], [(0, 2), (254, 257)], [(200, 600)], [(5, 6), (250, 300), (300, 520)]]
    g_off, g_sp = span_lists(good)
    clean = splice(src, dst, rep, g_off, g_sp, indexed)
    y, ref, packed = expect(src, dst, rep, g_off, g_sp)
    check_exact(mhc, src, clean, y, ref, packed, "good lists")
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    nb5 = int(src.nbits[5])
    cases = []
    for bad in ([(5, 5)], [(20, 30), (10, 15)], [(0, 3), (3, 9), (8, 12)]):
        for name, dpl, dnb in (("cut-9", damage.cut(streams[5], nb5, nb5 - 9), nb5 - 9), ("flip-mid", damage.flip(streams[5], nb5 // 2), nb5)):
            cases.append((bad, name, dpl, dnb))
    for bad, name, dpl, dnb in cases:
        lists = list(good)
        lists[BIG] = bad
        span_off, spans = span_lists(lists)
        pls, nbs = list(streams), [int(x) for x in src.nbits]
        pls[5], nbs[5] = dpl, dnb
        payload, pay_off = mhc.batch_offsets(pls)
        want = src.recode(dst, indexed, payload=payload, pay_off=pay_off, nbits=nbs)       # the decoder's verdict on stream 5
        got = splice(src, dst, rep, span_off, spans, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
        what = (bad, name, indexed)
        st = want["status"].tolist()
        st[BIG] = mhc.MH_ERR_ARG
        assert got["status"].tolist() == st and got["rc"] != mhc.MH_OK, what
        failed = [i for i in range(n) if st[i] != mhc.MH_OK]
        assert BIG in failed and (name != "cut-9" or 5 in failed), what
        lens = [0 if i in failed else len(y[i]) for i in range(n)]
        sure = [i for i in range(n) if i != 5 or i in failed]                     # (a flip the decoder accepts may change the length)
        assert got["out_sym_off"][0] == 0 and [int(x) for x in np.diff(got["out_sym_off"].astype(np.int64))[sure]] == [lens[i] for i in sure], what
        for i in range(n):
            a0, a1 = int(got["out_off"][i]), int(got["out_off"][i + 1])
            if i in failed:
                assert a0 == a1 and got["nbits"][i] == 0 and got["dropped"][i] == 0, what
            elif i != 5:                                                          # (a flip the decoder accepts gives another message)
                c0, c1 = int(clean["out_off"][i]), int(clean["out_off"][i + 1])
                assert got["payload"][a0:a1].tobytes() == clean["payload"][c0:c1].tobytes() and got["nbits"][i] == clean["nbits"][i], what
                assert got["dropped"][i] == clean["dropped"][i], what
        ok = [i for i in range(n) if i not in failed and i != 5]
        assert np.array_equal(slices_of(got["index"], got["out_sym_off"], CHUNK, ok), slices_of(clean["index"], clean["out_sym_off"], CHUNK, ok)), what


@pytest.mark.parametrize("rep_len", [0, 10])
@pytest.mark.parametrize("indexed", [True, False])
def test_an_empty_span_fails_its_stream_alone(mhc, msgs, sources, dsts, indexed, rep_len):
    """begin == end is the one rule by which this call differs from the table's, where it inserts: here it is malformed.  An
    undamaged batch, the empty span between two good ones in the middle stream: that stream alone is MH_ERR_ARG and gives
    what an empty message gives, nothing; every other stream is the reference's, exactly."""
    src, dst, rep = sources["o1"], dsts["other"], REPS[rep_len]
    n, mid = len(msgs), 4
    lists = [[], [(0, 1)], [(1, 2)], [(10, 13)], [(0, 2), (100, 100), (254, 256)], [(0, 2), (254, 257)], [(200, 600)], [(5, 6), (250, 300), (300, 520)]]
    assert len(msgs[mid]) == 256 and mid == n // 2
    got = splice(src, dst, rep, *span_lists(lists), indexed)
    what = (indexed, rep_len)
    assert got["status"].tolist() == [mhc.MH_ERR_ARG if i == mid else mhc.MH_OK for i in range(n)] and got["rc"] != mhc.MH_OK, (what, got["status"])
    lists[mid] = []
    y = splice_ref.apply(src.msgs, *span_lists(lists), rep)
    y[mid] = b""
    ref = recode_ref.recode(y, oracle_of(dst), src.chunk)
    r_pay, r_off, r_nb, r_drop = recode_ref.packed(ref)
    oso = splice_ref.offsets(y)
    assert np.array_equal(got["out_sym_off"], oso), (what, got["out_sym_off"], oso)
    assert np.array_equal(got["out_off"], r_off) and np.array_equal(got["nbits"], r_nb) and np.array_equal(got["dropped"], r_drop), what
    assert np.array_equal(got["payload"], r_pay), what
    assert np.array_equal(slices_of(got["index"], oso, CHUNK), np.concatenate([r[3] for r in ref])), what


def test_bad_span_offsets_stop_the_call(mhc, msgs, sources, dsts):
    src = sources["o1"]
    span_off, spans = span_lists([[(0, 1)] for _ in msgs])
    spans = np.concatenate([spans, spans[:2]])
    for bad in (span_off + np.uint64(1), span_off[::-1].copy(), np.array([0, 3, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint64)):
        for indexed in (True, False):
            got = splice(src, dsts["other"], b"#", bad, spans, indexed, count_only=True, want_index=False)
            assert got["rc"] == mhc.MH_ERR_ARG and not got["nbits"].any() and not got["out_off"].any() and not got["out_sym_off"].any()


def test_order2_and_a_set_of_the_wrong_size_are_refused(mhc, msgs, sources):
    src = sources["o1"]
    m2 = mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    none = span_lists([[] for _ in msgs])
    for a, b in ((m2, src.model), (src.model, m2)):
        with pytest.raises(mhc.MhError) as e:
            a.dev_recode_splice_batch(b, src.payload, src.pay_off, src.nbits, b"#", *none, **src.kw(True))
        assert e.value.status == mhc.MH_ERR_ARG
    ms = mhc.ModelSet.train([bytes(m) for m in msgs[:3]], order=1)
    with pytest.raises(mhc.MhError) as e:
        ms.recode_splice(src.model, src.payload, src.pay_off, src.nbits, b"#", *none, **src.kw(True))
    assert e.value.status == mhc.MH_ERR_ARG


# ---- 6. dirty workspaces and outputs, the same workspace twice; the host form ------------------------------------------------------------

@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_prefilled_workspace_and_outputs(mhc, msgs, sources, dsts, byte):
    src, dst = sources["o1"], dsts["other"]
    per, _ = placements(msgs)["runs of touching spans"]
    span_off, spans = span_lists(per)
    with mhc.device_memory("fill", byte):                                       # the workspaces (created without contents) hold `byte`
        for rep_len in (0, 10):
            y, ref, packed = expect(src, dst, REPS[rep_len], span_off, spans)
            for indexed in (True, False):
                check_exact(mhc, src, splice(src, dst, REPS[rep_len], span_off, spans, indexed), y, ref, packed, (byte, rep_len, indexed))


@pytest.mark.parametrize("indexed", [True, False])
def test_a_deletion_fits_a_prefilled_workspace_of_exactly_the_stated_size(mhc, msgs, sources, dsts, indexed):
    """rep_len = 0 on the runs of touching spans, the call with the look-back pre-pass and its per-span contexts at the end of
    the workspace: mh_dev_recode_splice_workspace bytes, every one 0xFF, and not a byte more.  The results are the reference's
    and the guard behind the workspace is intact."""
    lib, D = mhc.lib(), mhc.DeviceBuffer
    src, dst = sources["o1"], dsts["other"]
    per, _ = placements(msgs)["runs of touching spans"]
    span_off, spans = span_lists(per)
    y, ref, packed = expect(src, dst, b"", span_off, spans)
    oso = splice_ref.offsets(y)
    n, total, G = len(msgs), int(src.sym_off[-1]) if indexed else 0, 256
    pl = np.concatenate([src.payload, np.zeros(64, dtype=np.uint8)])
    d_pl, d_po, d_nb = D(pl.nbytes, pl), D(src.pay_off.nbytes, src.pay_off), D(src.nbits.nbytes, src.nbits)
    d_so = D(src.sym_off.nbytes, src.sym_off if indexed else np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    idx = np.asarray(src.index, dtype=np.uint64)
    d_idx, d_sof, d_sp = D(idx.nbytes, idx), D(span_off.nbytes, span_off), D(spans.nbytes, spans)
    wsb = lib.mh_dev_recode_splice_workspace(n, total, CHUNK if indexed else 0, len(spans))
    d_ws = D(wsb + G, np.concatenate([np.full(wsb, 0xFF, dtype=np.uint8), np.full(G, 0x5A, dtype=np.uint8)]))
    cap, nidx = int(packed[1][n]), int(oso[n]) // CHUNK + n
    d_out = D(cap + 64, np.full(cap + 64, 0xA5, dtype=np.uint8))
    d_oo, d_onb, d_oso, d_oi, d_dr = [D(k * 8, np.full(k, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)) for k in (n + 1, n, n + 1, nidx, n)]
    d_st = D(n * 4, np.full(n, 99, dtype=np.int32))
    rc = lib.mh_dev_recode_splice_batch(src.model.handle, dst.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(src.pay_off[-1]), 0x20, d_so.ptr, total,
                                        d_idx.ptr if indexed else None, CHUNK, d_sof.ptr, d_sp.ptr, None, 0, d_out.ptr, cap, d_oo.ptr, d_onb.ptr,
                                        d_oso.ptr, d_oi.ptr, nidx, d_dr.ptr, d_st.ptr, d_ws.ptr, wsb, None)
    assert rc == mhc.MH_OK and lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_OK and not d_st.download(np.int32)[:n].any()
    assert (d_ws.download(np.uint8)[wsb:wsb + G] == 0x5A).all(), "bytes written behind the workspace"
    assert np.array_equal(d_oo.download(np.uint64)[:n + 1], packed[1]) and np.array_equal(d_onb.download(np.uint64)[:n], packed[2])
    assert np.array_equal(d_dr.download(np.uint64)[:n], packed[3]) and np.array_equal(d_oso.download(np.uint64)[:n + 1], oso)
    assert np.array_equal(d_so.download(np.uint64)[:n + 1], src.sym_off)
    assert np.array_equal(d_out.download(np.uint8)[:cap], packed[0]) and (d_out.download(np.uint8)[cap:] == 0xA5).all()
    assert np.array_equal(slices_of(d_oi.download(np.uint64)[:nidx], oso, CHUNK), np.concatenate([r[3] for r in ref]))


def test_host_form(mhc, msgs, sources, dsts):
    src, dst = sources["o1"], dsts["other"]
    per, _ = placements(msgs)["runs of touching spans"]
    span_off, spans = span_lists(per)
    for rep_len in (0, 10):
        y, ref, packed = expect(src, dst, REPS[rep_len], span_off, spans)
        oso = splice_ref.offsets(y)
        for indexed in (True, False):
            got = src.model.recode_splice_batch(dst, src.payload, src.pay_off, src.nbits, REPS[rep_len], span_off, spans, **src.kw(indexed))
            assert got["rc"] == mhc.MH_OK and np.array_equal(got["payload"], packed[0]) and np.array_equal(got["out_off"], packed[1])
            assert np.array_equal(got["nbits"], packed[2]) and np.array_equal(got["dropped"], packed[3]) and np.array_equal(got["sym_off"], src.sym_off)
            assert np.array_equal(got["out_sym_off"], oso)
            assert np.array_equal(slices_of(got["index"], oso, CHUNK), np.concatenate([r[3] for r in ref]))


def test_host_form_indexes_a_batch_with_a_stream_over_the_walk_cap_first(mhc):
    """Index-free, one stream over MH_BATCH_WALK_MAX_BITS: the host form indexes the batch first, with the chunk size of
    out_index when it writes one and its own when it does not.  A span in the long stream, one in the first stream."""
    long_msg = np.random.default_rng(61).integers(0, 256, 1_200_000 + 77, dtype=np.uint8).tobytes()      # ~8-bit codes under its own model
    src = Source(mhc, [b"a few bytes", long_msg, b""], order=0)
    assert src.model.min_code_len >= 7 and int(src.nbits[1]) > mhc.BATCH_WALK_MAX_BITS
    dst = model_of(mhc, [long_msg, b"[REDACTED]" * 400], 0)
    span_off, spans = span_lists([[(2, 5)], [(700_001, 700_300)], []])
    for rep in (b"", b"[REDACTED]"):
        y, ref, packed = expect(src, dst, rep, span_off, spans)
        oso = splice_ref.offsets(y)
        for want_index in (True, False):
            got = src.model.recode_splice_batch(dst, src.payload, src.pay_off, src.nbits, rep, span_off, spans, chunk_symbols=CHUNK,
                                                want_index=want_index, check=False)
            what = "over the cap, rep_len=%d out_index=%s" % (len(rep), want_index)
            assert got["rc"] == mhc.MH_OK and not got["status"].any(), what
            assert np.array_equal(got["payload"], packed[0]) and np.array_equal(got["out_off"], packed[1]) and np.array_equal(got["nbits"], packed[2]), what
            assert np.array_equal(got["dropped"], packed[3]) and np.array_equal(got["sym_off"], src.sym_off) and np.array_equal(got["out_sym_off"], oso), what
            if want_index:
                assert np.array_equal(slices_of(got["index"], oso, CHUNK), np.concatenate([r[3] for r in ref])), what


def test_chain_find_spans_splice_decode_on_one_stream_twice_on_one_workspace(env, msgs):
    """find -> spans -> splice -> splice again on the same workspace and outputs -> decode, on a torch stream, enqueued back to
    back behind a blocker (tests/test_gpu_stream_order.py): no host copy and no host wait between the calls."""
    mhc, lib = env.mhc, env.lib
    pats = [b"in", b"ng", b"ing "]
    w_off, w_rec, (r_so, r_sp) = hit_spans(msgs, pats)
    n, k, m = len(msgs), len(w_rec), len(r_sp)
    rep = b""
    y = splice_ref.apply(msgs, r_so, r_sp, rep)
    model = model_of(mhc, list(msgs) + y, 1)
    src = Source(mhc, msgs, model=model)
    ref = recode_ref.recode(y, oracle_of(model), CHUNK)
    packed = recode_ref.packed(ref)
    oso = splice_ref.offsets(y)
    total, pay_total, ototal = int(src.sym_off[n]), int(src.pay_off[n]), int(oso[n])
    nidx = int(lib.mh_batch_index_capacity(total, n, CHUNK))
    onidx = ototal // CHUNK + n
    ps = mhc.PatternSet(pats)
    ch = Chain(env, "splice chain")
    ch.keep = (model, ps)
    b = Batch(ch.staged(np.concatenate([src.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(src.pay_off), ch.staged(src.nbits), n, pay_total)
    d_in, d_idx = ch.staged(src.sym_off), ch.staged(np.asarray(src.index, dtype=np.uint64)[:nidx])
    wsb = lib.mh_dev_find_batch_workspace(n, total, CHUNK)
    d_ws, d_ho, d_rec, d_st = ch.work(wsb), ch.words(n + 1), ch.out(k * 24 + 64), ch.status(n, "find")
    ch.call("find_batch", lib.mh_dev_find_batch, model.handle, ps.handle, *b.args(), 0x20, ptr(d_in), total, ptr(d_idx), CHUNK, ptr(d_ho), ptr(d_rec),
            None, k, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    wsb2 = lib.mh_dev_spans_from_hits_workspace(n, k)
    d_ws2, d_so, d_sp = ch.work(wsb2), ch.words(n + 1), ch.out(k * 16 + 64)
    ch.call("spans_from_hits", lib.mh_dev_spans_from_hits, ptr(d_ho), ptr(d_rec), k, n, ptr(d_so), ptr(d_sp), ptr(d_ws2), wsb2, ws=d_ws2)
    ch.expect("spans", lambda: same(ch.get(d_so, np.uint64, n + 1), r_so) and same(ch.get(d_sp, np.uint64, 2 * m).reshape(-1, 2), r_sp))
    cap = int(packed[1][n])
    wsb3 = lib.mh_dev_recode_splice_workspace(n, total, CHUNK, k)                 # sized from the hit capacity: at most one span a record
    d_ws3, d_st3 = ch.work(wsb3), ch.status(n, "splice")
    d_oo, d_onb, d_dr, d_out, d_oi, d_oso = ch.words(n + 1), ch.words(n), ch.words(n), ch.out(cap + 64), ch.words(onidx), ch.words(n + 1)
    for turn in ("splice_batch", "splice_batch again"):
        ch.call(turn, lib.mh_dev_recode_splice_batch, model.handle, model.handle, *b.args(), 0x20, ptr(d_in), total, ptr(d_idx), CHUNK,
                ptr(d_so), ptr(d_sp), None, 0, ptr(d_out), cap, ptr(d_oo), ptr(d_onb), ptr(d_oso), ptr(d_oi), onidx, ptr(d_dr), ptr(d_st3), ptr(d_ws3),
                wsb3, ws=d_ws3)
    ch.expect("splice: offsets, nbits, dropped, out_sym_off", lambda: same(ch.get(d_oo, np.uint64, n + 1), packed[1])
              and same(ch.get(d_onb, np.uint64, n), packed[2]) and same(ch.get(d_dr, np.uint64, n), packed[3]) and same(ch.get(d_oso, np.uint64, n + 1), oso))
    ch.expect("splice: payload", lambda: same(ch.get(d_out, np.uint8, cap), packed[0]) and (ch.get(d_out)[cap:cap + 64] == 0xA5).all())
    ch.expect("splice: index slices", lambda: same(slices_of(ch.get(d_oi, np.uint64, onidx), oso, CHUNK), np.concatenate([r[3] for r in ref])))
    wsb4 = lib.mh_dev_decode_batch_workspace(n)
    d_ws4, d_dec, d_st4 = ch.work(wsb4), ch.out(ototal + 64), ch.status(n, "decode")
    ch.call("decode_batch", lib.mh_dev_decode_batch, model.handle, ptr(d_out), ptr(d_oo), ptr(d_onb), n, cap, 0x20, ptr(d_dec), ototal, ptr(d_oso), ototal,
            ptr(d_oi), CHUNK, ptr(d_st4), ptr(d_ws4), wsb4, ws=d_ws4)
    ch.expect("decode: the spliced messages", lambda: ch.get(d_dec, np.uint8, ototal).tobytes() == b"".join(y))
    drive(ch)


def test_the_same_workspace_twice_gives_identical_results(mhc, msgs, sources, dsts):
    """Two calls on one workspace and one set of outputs, neither cleared in between, a replacement first and a deletion second:
    the second call's results are those of a call on fresh buffers."""
    lib = mhc.lib()
    src, dst = sources["o1"], dsts["other"]
    per, _ = placements(msgs)["runs of touching spans"]
    span_off, spans = span_lists(per)
    n, total = len(msgs), int(src.sym_off[-1])
    D = mhc.DeviceBuffer
    pl = np.concatenate([src.payload, np.zeros(64, dtype=np.uint8)])
    d_pl, d_po, d_nb, d_so = D(pl.nbytes, pl), D(src.pay_off.nbytes, src.pay_off), D(src.nbits.nbytes, src.nbits), D(src.sym_off.nbytes, src.sym_off)
    idx = np.asarray(src.index, dtype=np.uint64)
    d_idx, d_sof, d_sp = D(idx.nbytes, idx), D(span_off.nbytes, span_off), D(spans.nbytes, spans)
    rep = np.frombuffer(REPS[255] + b"\0", dtype=np.uint8)
    d_rep = D(rep.nbytes, rep)
    wsb = lib.mh_dev_recode_splice_workspace(n, total, CHUNK, len(spans))
    cap, nidx = 1 << 16, 64
    d_ws = D(wsb, np.full(wsb, 0xFF, dtype=np.uint8))
    outs = [D(cap, np.full(cap, 0xA5, dtype=np.uint8))] + [D(k * 8, np.full(k, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)) for k in (n + 1, n, n + 1, nidx, n)]
    d_out, d_oo, d_onb, d_oso, d_oi, d_dr = outs
    d_st = D(n * 4, np.full(n, 99, dtype=np.int32))
    for rep_len in (255, 0, 255, 0):
        rc = lib.mh_dev_recode_splice_batch(src.model.handle, dst.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(src.pay_off[-1]), 0x20, d_so.ptr, total,
                                            d_idx.ptr, CHUNK, d_sof.ptr, d_sp.ptr, d_rep.ptr, rep_len, d_out.ptr, cap, d_oo.ptr, d_onb.ptr, d_oso.ptr,
                                            d_oi.ptr, nidx, d_dr.ptr, d_st.ptr, d_ws.ptr, wsb, None)
        assert rc == mhc.MH_OK and lib.mh_dev_status(d_ws.ptr, None) == mhc.MH_OK
        y, ref, packed = expect(src, dst, REPS[rep_len], span_off, spans)
        oso = splice_ref.offsets(y)
        need = int(packed[1][n])
        assert np.array_equal(d_oo.download(np.uint64)[:n + 1], packed[1]) and np.array_equal(d_onb.download(np.uint64)[:n], packed[2]), rep_len
        assert np.array_equal(d_dr.download(np.uint64)[:n], packed[3]) and np.array_equal(d_oso.download(np.uint64)[:n + 1], oso), rep_len
        assert np.array_equal(d_out.download(np.uint8)[:need], packed[0]) and not d_st.download(np.int32)[:n].any(), rep_len
        assert np.array_equal(slices_of(d_oi.download(np.uint64), oso, CHUNK), np.concatenate([r[3] for r in ref])), rep_len


# (every source reads the replacement from L2 since the splice is one kernel family; here the destination's image does too)
def test_a_source_whose_tables_fill_the_lds_reads_the_replacement_from_l2(mhc):
    """The source model of tests/test_gpu_edit.py whose tables leave 144 bytes of LDS: neither the order-0 image nor the
    replacement's 256 bytes fit, and both come from L2."""
    c = np.zeros((256, 256), dtype=np.uint64)
    row = (np.floor((1 << 20) / np.arange(1, 257) ** 1.1) + 1).astype(np.uint64)
    c[:98] = row
    c[98, :200] = row[:200]
    c[99:, 0] = 1
    model = mhc.Model.from_counts(c.reshape(-1), 1)
    P, nsec, in_lds = model.decode_layout()
    lds = 1024 + (512 << P) + ((2 * nsec + 15) & ~15)
    assert in_lds and 0 <= 163840 - lds < 256, (P, nsec, lds)
    rng = np.random.default_rng(5)
    w = 1.0 / np.arange(1, 99) ** 1.1
    batch = [rng.choice(98, size=k, p=w / w.sum()).astype(np.uint8).tobytes() for k in (0, 1, 255, 256, 257, 1300)]
    src = Source(mhc, batch, model=model)
    span_off, spans = span_lists([[], [(0, 1)], [(100, 101)], [(250, 256)], [(0, 2), (254, 257)], [(200, 600), (600, 700), (1024, 1030)]])
    for do in (0, 1):
        dst = model_of(mhc, [rng.choice(98, size=60000, p=w / w.sum()).astype(np.uint8).tobytes()], do)
        for rep in (b"", bytes(range(10)), bytes(rng.choice(98, size=255).astype(np.uint8))):
            y, ref, packed = expect(src, dst, rep, span_off, spans)
            for indexed in (True, False):
                check_exact(mhc, src, splice(src, dst, rep, span_off, spans, indexed), y, ref, packed, ("rep in L2", do, len(rep), indexed))


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------------------------

def test_cli_replace(mhc, tmp_path):
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    x, yf = "input_wiki_cpp.txt", "input_ipsum.txt"
    data = golden()[x]["data"]
    p = lambda n: str(tmp_path / n)
    for name, blob in (("x", data), ("x.cm", expected_file(x, "cm")), ("x.e", expected_file(x, "e")), ("y.e", expected_file(yf, "e"))):
        with open(p(name), "wb") as f:
            f.write(blob)
    run = lambda a: subprocess.run([cli] + a, capture_output=True, timeout=300)

    def spliced_by(pats, rep):
        off, rec, (so, sp) = hit_spans([data], pats)
        return splice_ref.apply([data], so, sp, rep)[0], len(sp), int((sp[:, 1] - sp[:, 0]).sum())

    def want_file(table, text):
        blob, _ = mh_oracle.Model.from_table(table).compress(text)
        return blob

    # --replace "[X]" under another table; index-free, as the reference wrote the file
    text, nspans, nbytes = spliced_by([b"language", b"age"], b"[X]")
    assert nspans > 5 and len(text) != len(data)
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("y.e"), "-o", p("out.cm"), "--redact", "language", "--redact", "age", "--replace", "[X]"])
    assert r.returncode == 0, r.stderr
    assert open(p("out.cm"), "rb").read() == want_file(expected_file(yf, "e"), text) and not os.path.exists(p("out.cm.idx"))
    assert ("Replacing %d bytes in %d spans with %d bytes." % (nbytes, nspans, 3 * nspans)).encode() in r.stderr, r.stderr
    # --replace "" and "[X]" with the index, under a table with codes for every pair of the spliced texts (nothing is dropped):
    # the output's own index, for the new length, beside it; -x of the output through that index gives the reference bytes
    texts = [spliced_by([b"language", b"age"], rep)[0] for rep in (b"", b"[X]")]
    both = model_of(mhc, [data] + texts, 1).table_bytes()
    with open(p("both.e"), "wb") as f:
        f.write(both)
    assert run([p("x"), "-e", p("x.e"), "-o", p("x2.cm"), "--index", p("x.idx"), "--chunk", "256"]).returncode == 0
    for rep, tag in ((b"", "del"), (b"[X]", "rep")):
        text, nspans, nbytes = spliced_by([b"language", b"age"], rep)
        with open(p("spliced"), "wb") as f:
            f.write(text)
        assert run([p("spliced"), "-e", p("both.e"), "-o", p("m.cm"), "--index", p("m.idx"), "--chunk", "256"]).returncode == 0
        out = p("out_%s.cm" % tag)
        r = run([p("x2.cm"), "-x", "-e", p("x.e"), "--recode", p("both.e"), "-o", out, "--index", p("x.idx"), "--redact", "language", "--redact", "age",
                 "--replace", rep.decode()])
        assert r.returncode == 0 and b"skipped" not in r.stderr, r.stderr
        assert open(out, "rb").read() == want_file(both, text) == open(p("m.cm"), "rb").read()
        assert open(out + ".idx", "rb").read() == open(p("m.idx"), "rb").read()
        assert ("Replacing %d bytes in %d spans with %d bytes." % (nbytes, nspans, len(rep) * nspans)).encode() in r.stderr, r.stderr
        r = run([out, "-x", "-e", p("both.e"), "-o", p("back"), "--index", out + ".idx"])
        assert r.returncode == 0 and open(p("back"), "rb").read() == text, r.stderr
