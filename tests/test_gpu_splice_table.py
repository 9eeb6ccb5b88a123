"""The table splice on the GPU (include/mh.h, "SPLICING WITH A REPLACEMENT TABLE"): a batch coded again with every span replaced
by the table entry its tag names, insertions included, the bytes never written.  The reference is tests/splice_table_ref.py on
top of tests/recode_ref.py (the CPU oracle's encoder on the edited messages); every comparison is exact.  The device-call
wrappers put guards around every output and assert that nothing outside the results changed.

chunk_symbols is 256 (MH_CHUNK_MIN) and the batch that of tests/test_gpu_splice.py: messages of 0, 1, 2, 255, 256, 257,
3 * 256 + 5 and about 1100 bytes."""
import os
import subprocess
import time

import numpy as np
import pytest

import damage
import find_ref
import recode_ref
import splice_ref
import splice_table_ref as tref
from conftest import ROOT, expected_file, golden
from oracle import mh_oracle
from test_gpu_edit import CHUNK, Source, mhc, model_of, msgs, oracle_of, slices_of, span_lists  # noqa: F401  (mhc, msgs: fixtures)
from test_gpu_splice import BIG, LAST, PLACEMENTS, REPS, check_exact, placements, dsts, sources  # noqa: F401  (dsts, sources: fixtures)
from test_gpu_splice import splice as splice_one

pytestmark = pytest.mark.gpu

TEXT = golden()["input_wiki_cpp.txt"]["data"]
# lengths {0, 1, 3, 10, 255}: a deletion, the shortest, a short one, a marker, the longest
TABLE = [b"", b"#", b"<I>", b"[REDACTED]", TEXT[9000:9255]]
assert [len(r) for r in TABLE] == [0, 1, 3, 10, 255]


def splice(src, dst, tags, reps, span_off, spans, indexed, payload=None, pay_off=None, nbits=None, **kw):
    fn = src.model.recode_splice_table if src.each else src.model.dev_recode_splice_table_batch
    return fn(dst, *src.batch(payload, pay_off, nbits), tags, reps, span_off, spans, **src.kw(indexed), **kw)


def expect(src, dst, tags, reps, span_off, spans):
    """What the table splice must give: the oracle's encode, under dst, of the edited messages."""
    y = tref.apply(src.msgs, span_off, spans, tags, reps)
    ref = recode_ref.recode(y, oracle_of(dst), src.chunk)
    return y, ref, recode_ref.packed(ref)


def cycle(per, start=0, k=len(TABLE)):
    """Per-stream lists of (begin, end) with tags cycling along the spans of the batch."""
    out, t = [], start
    for lst in per:
        row = []
        for b, e in lst:
            row.append((b, e, t % k))
            t += 1
        out.append(row)
    return out


def run_all(mhc, sources, dsts, per, reps, what, pairs=(("o0", "other"), ("o0", "other0"), ("o1", "same"), ("o1", "other"), ("set", "other"))):
    """per: per-stream lists of (begin, end, tag).  Every source and destination, indexed and index-free, against the
    reference; returns the edited messages."""
    span_off, spans, tags = tref.tagged_lists(per)
    y = None
    for s, d in pairs:
        src = sources[s]
        y, ref, packed = expect(src, dsts[d], tags, reps, span_off, spans)
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, dsts[d], tags, reps, span_off, spans, indexed), y, ref, packed, (what, s, d, indexed))
    return y


# ---- 1. one entry, every tag 0, no insertion: the single-replacement call ----------------------------------------------------------

@pytest.mark.parametrize("rep_len", [0, 1, 10, 255])
@pytest.mark.parametrize("name", PLACEMENTS)
def test_one_entry_equals_the_single_replacement_call(mhc, msgs, sources, dsts, name, rep_len):
    per, occurs = placements(msgs)[name]
    assert occurs(), name
    span_off, spans = span_lists(per)
    tags = np.zeros(len(spans), dtype=np.uint32)
    rep = REPS[rep_len]
    for s in ("o0", "o1", "set"):
        src = sources[s]
        for d in ("same", "other") if s != "o0" else ("other", "other0"):
            y, ref, packed = expect(src, dsts[d], tags, [rep], span_off, spans)
            assert y == splice_ref.apply(src.msgs, span_off, spans, rep)
            for indexed in (True, False):
                what = (name, rep_len, s, d, indexed)
                got = splice(src, dsts[d], tags, [rep], span_off, spans, indexed)
                check_exact(mhc, src, got, y, ref, packed, what)
                one = splice_one(src, dsts[d], rep, span_off, spans, indexed)
                for k in ("payload", "out_off", "nbits", "dropped", "status", "sym_off", "out_sym_off", "index"):
                    assert np.array_equal(got[k], one[k]), (what, k)
                assert got["rc"] == one["rc"]


# ---- 2. a mixed table, tags cycling along the spans -----------------------------------------------------------------------------------

def mixed_placements(msgs):
    """name -> (per-stream lists of (begin, end, tag), a check that the case occurs).  Tags index TABLE: 0 deletes."""
    n, L = len(msgs), len(msgs[LAST])
    C = CHUNK

    def only(i, lst):
        return [lst if k == i else [] for k in range(n)]
    return {
        # the lane of chunk 1 starts inside a deleted span whose touching predecessor is replaced: rep's last byte
        "deleted over a seam behind a replaced span": (only(BIG, [(240, 250, 3), (250, 260, 0)]), lambda: 250 // C != 259 // C),
        "deleted, deleted, replaced in front": (only(BIG, [(230, 235, 2), (235, 240, 0), (240, 250, 0), (250, 300, 0)]), lambda: 300 > C > 250),
        "an empty insertion inside the run": (only(BIG, [(230, 235, 4), (235, 235, 0), (235, 250, 0), (250, 250, 0), (250, 300, 0)]), lambda: True),
        "deleted run from 0": (only(BIG, [(0, 100, 0), (100, 256, 0), (256, 300, 0)]) , lambda: True),
        "deleted run from 0, last stream": (only(LAST, [(0, 0, 0), (0, 200, 0), (200, 520, 0)]), lambda: L > 520),
        "a run beginning on a chunk boundary": (only(BIG, [(256, 300, 0), (300, 520, 0), (520, 530, 1)]), lambda: 256 % C == 0 and 520 > 2 * C),
        "a chunk whose lane produces nothing": (only(BIG, [(200, 600, 0)]), lambda: 200 < C and 600 > 2 * C),
        "a chunk whose lane produces nothing, replaced": (only(BIG, [(200, 600, 4)]), lambda: True),
        "a replaced span ending exactly at first": (only(BIG, [(250, 256, 3), (500, 512, 1), (512, 513, 0)]), lambda: 256 % C == 0 == 512 % C),
        "a deleted span ending exactly at first": (only(BIG, [(250, 256, 0), (300, 512, 0)]), lambda: True),
        "mixed over every stream": (cycle(placements(msgs)["every message whole"][0], 1), lambda: True),
        "mixed across every seam of the last stream": (cycle(placements(msgs)["across every seam of the last stream"][0]), lambda: True),
        "mixed runs of touching spans": (cycle(placements(msgs)["runs of touching spans"][0]), lambda: True),
        "mixed runs of touching spans, shifted": (cycle(placements(msgs)["runs of touching spans"][0], 3), lambda: True),
    }


MIXED = ["deleted over a seam behind a replaced span", "deleted, deleted, replaced in front", "an empty insertion inside the run",
         "deleted run from 0", "deleted run from 0, last stream", "a run beginning on a chunk boundary", "a chunk whose lane produces nothing",
         "a chunk whose lane produces nothing, replaced", "a replaced span ending exactly at first", "a deleted span ending exactly at first",
         "mixed over every stream", "mixed across every seam of the last stream", "mixed runs of touching spans",
         "mixed runs of touching spans, shifted"]


@pytest.mark.parametrize("name", MIXED)
def test_mixed_table(mhc, msgs, sources, dsts, name):
    per, occurs = mixed_placements(msgs)[name]
    assert occurs(), name
    y = run_all(mhc, sources, dsts, per, TABLE, name)
    if name == "a chunk whose lane produces nothing":
        assert len(y[BIG]) == 773 - 400


# ---- 3. insertions -------------------------------------------------------------------------------------------------------------------

def insertion_cases(msgs):
    n, L = len(msgs), len(msgs[LAST])

    def only(i, lst):
        return [lst if k == i else [] for k in range(n)]
    return {
        "at 0, 255, 256 and mid-chunk": only(BIG, [(0, 0, 3), (255, 255, 1), (256, 256, 2), (400, 400, 3), (512, 512, 4)]),
        "two at one position": only(BIG, [(100, 100, 1), (100, 100, 3), (256, 256, 3), (256, 256, 2), (256, 256, 1)]),
        "touching a deleted span over a seam, front and back": only(BIG, [(250, 250, 3), (250, 260, 0), (260, 260, 2)]),
        "touching a deleted span that ends on a boundary": only(BIG, [(200, 200, 1), (200, 256, 0), (256, 256, 3), (256, 300, 0), (300, 300, 2)]),
        "touching a replaced span": only(BIG, [(10, 10, 1), (10, 20, 3), (20, 20, 2)]),
        "at len and into the empty message": [[(0, 0, 3)], [(1, 1, 3)], [(2, 2, 1)], [(255, 255, 2)], [(256, 256, 3)], [], [(773, 773, 4)], [(L, L, 1)]],
        "into the 1-byte message at 0": [[], [(0, 0, 3)], [(0, 0, 1), (1, 1, 2)]] + [[] for _ in range(n - 3)],
        "16 of 255 bytes into the 256-byte message": [[], [], [], [], [(k, k, 4) for k in range(0, 256, 16)]] + [[] for _ in range(n - 5)],
    }


@pytest.mark.parametrize("name", sorted(insertion_cases([b""] * 8)))
def test_insertions(mhc, msgs, sources, dsts, name):
    per = insertion_cases(msgs)[name]
    y = run_all(mhc, sources, dsts, per, TABLE, name)
    ln = [len(m) for m in y]
    if name == "at len and into the empty message":
        assert y == [bytes(m) for m in msgs]
    if name == "into the 1-byte message at 0":
        assert y[1] == TABLE[3] + msgs[1] and y[2] == TABLE[1] + msgs[2][:1] + TABLE[2] + msgs[2][1:]
    if name == "16 of 255 bytes into the 256-byte message":
        assert ln[4] == 256 + 16 * 255 and (ln[4] + CHUNK - 1) // CHUNK == 17
    if name == "two at one position":
        assert y[BIG][100:111] == b"#[REDACTED]" and y[BIG][256 + 11:256 + 11 + 14] == b"[REDACTED]<I>#"


def test_an_insertion_with_an_empty_replacement_is_a_no_op(mhc, msgs, sources, dsts):
    n = len(msgs)
    base = [(240, 250, 3), (250, 260, 0), (300, 300, 2)]
    with_empty = [(0, 0, 0), (240, 240, 0), (240, 250, 3), (250, 250, 0), (250, 260, 0), (260, 260, 0), (300, 300, 2), (300, 300, 0), (512, 512, 0)]
    src, dst = sources["o1"], dsts["other"]
    res = []
    for lst in (base, with_empty):
        span_off, spans, tags = tref.tagged_lists([lst if k == BIG else [] for k in range(n)])
        y, ref, packed = expect(src, dst, tags, TABLE, span_off, spans)
        for indexed in (True, False):
            got = splice(src, dst, tags, TABLE, span_off, spans, indexed)
            check_exact(mhc, src, got, y, ref, packed, (len(lst), indexed))
            res.append(got)
    for a, b in ((res[0], res[2]), (res[1], res[3])):
        for k in ("payload", "out_off", "nbits", "dropped", "out_sym_off", "index"):
            assert np.array_equal(a[k], b[k]), k


# ---- 4. codes missing under dst ---------------------------------------------------------------------------------------------------------

def test_drops_are_counted_per_replacement(mhc, msgs, sources, dsts):
    assert not any(0x07 in m for m in msgs)
    reps = [b"a\x07\x07b", b"[REDACTED]", b"", b"\x07"]
    per = [[], [(0, 1, 0)], [(1, 2, 1), (2, 2, 0)], [(10, 13, 0), (20, 20, 3)], [(253, 256, 1)], [(0, 2, 0), (254, 257, 3)],
           [(100, 101, 0), (250, 520, 2), (520, 520, 0), (600, 601, 1)], [(5, 6, 1), (255, 256, 0), (256, 256, 0)]]
    span_off, spans, tags = tref.tagged_lists(per)
    for s, d in (("o1", "same"), ("o1", "other"), ("set", "other"), ("o0", "other")):
        src = sources[s]
        y, ref, packed = expect(src, dsts[d], tags, reps, span_off, spans)
        drops = packed[3]
        # (a, 7), (7, 7), (7, b) of entry 0; (x, 7), (7, x) around entry 3: stream 3 has both, stream 1 entry 0 alone
        assert drops[1] >= 3 and drops[3] >= 5 and drops[0] == 0
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, dsts[d], tags, reps, span_off, spans, indexed), y, ref, packed, ("no code", s, d, indexed))


# ---- 5. failures stay local; a bad table stops the call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("indexed", [True, False])
def test_a_bad_tag_a_malformed_list_and_a_damaged_stream_fail_alone(mhc, msgs, sources, dsts, indexed):
    src, dst = sources["o1"], dsts["other"]
    n = len(msgs)
    good = [[], [(0, 1, 1)], [(1, 2, 2)], [(10, 13, 3)], [(250, 256, 0)], [(0, 2, 4), (254, 257, 0)], [(200, 600, 0)],
            [(5, 6, 1), (250, 300, 0), (300, 300, 2), (300, 520, 0)]]
    g_off, g_sp, g_tg = tref.tagged_lists(good)
    clean = splice(src, dst, g_tg, TABLE, g_off, g_sp, indexed)
    y, ref, packed = expect(src, dst, g_tg, TABLE, g_off, g_sp)
    check_exact(mhc, src, clean, y, ref, packed, "good lists")
    streams = [bytes(src.payload[int(src.pay_off[i]):int(src.pay_off[i + 1])]) for i in range(n)]
    nb5 = int(src.nbits[5])
    for bad in ([(5, 9, len(TABLE))], [(5, 9, 1), (20, 20, 0xFFFFFFFF)], [(30, 20, 0)], [(20, 30, 0), (10, 15, 0)], [(3, 9, 1), (3, 3, 1)],
                [(0, 3, 1), (3, 9, 1), (8, 12, 1)]):
        assert bad[0][2] >= len(TABLE) or bad[-1][2] >= len(TABLE) or not tref.well_formed([(b, e) for b, e, _ in bad])
        for name, dpl, dnb in (("cut-9", damage.cut(streams[5], nb5, nb5 - 9), nb5 - 9), ("flip-mid", damage.flip(streams[5], nb5 // 2), nb5)):
            lists = list(good)
            lists[BIG] = bad
            span_off, spans, tags = tref.tagged_lists(lists)
            pls, nbs = list(streams), [int(x) for x in src.nbits]
            pls[5], nbs[5] = dpl, dnb
            payload, pay_off = mhc.batch_offsets(pls)
            want = src.recode(dst, indexed, payload=payload, pay_off=pay_off, nbits=nbs)       # the decoder's verdict on stream 5
            got = splice(src, dst, tags, TABLE, span_off, spans, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
            what = (bad, name, indexed)
            st = want["status"].tolist()
            st[BIG] = mhc.MH_ERR_ARG
            assert got["status"].tolist() == st and got["rc"] != mhc.MH_OK, what
            failed = [i for i in range(n) if st[i] != mhc.MH_OK]
            assert BIG in failed and (name != "cut-9" or 5 in failed), what
            for i in range(n):
                a0, a1 = int(got["out_off"][i]), int(got["out_off"][i + 1])
                if i in failed:
                    assert a0 == a1 and got["nbits"][i] == 0 and got["dropped"][i] == 0, what
                    assert got["out_sym_off"][i + 1] == got["out_sym_off"][i], what
                elif i != 5:                                                      # (a flip the decoder accepts gives another message)
                    c0, c1 = int(clean["out_off"][i]), int(clean["out_off"][i + 1])
                    assert got["payload"][a0:a1].tobytes() == clean["payload"][c0:c1].tobytes() and got["nbits"][i] == clean["nbits"][i], what
                    assert got["dropped"][i] == clean["dropped"][i], what
                    assert int(got["out_sym_off"][i + 1] - got["out_sym_off"][i]) == len(y[i]), what
            ok = [i for i in range(n) if i not in failed and i != 5]
            assert np.array_equal(slices_of(got["index"], got["out_sym_off"], CHUNK, ok), slices_of(clean["index"], clean["out_sym_off"], CHUNK, ok)), what


def test_a_bad_table_stops_the_call(mhc, msgs, sources, dsts):
    src, dst = sources["o1"], dsts["other"]
    span_off, spans, tags = tref.tagged_lists([[(0, 1, 0)] if len(m) else [] for m in msgs])
    long_entry = (np.array([0, 3, 259, 260], dtype=np.uint64), np.zeros(260, dtype=np.uint8) + 65)
    decreasing = (np.array([0, 5, 3, 8], dtype=np.uint64), np.zeros(8, dtype=np.uint8) + 65)
    not_from_0 = (np.array([1, 2, 3, 4], dtype=np.uint64), np.zeros(8, dtype=np.uint8) + 65)
    no_table = (np.array([0], dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    for what, table in (("256 bytes", long_entry), ("decreasing", decreasing), ("rep_off[0]", not_from_0), ("n_reps 0", no_table)):
        for indexed in (True, False):
            got = splice(src, dst, tags, table, span_off, spans, indexed, count_only=True, want_index=False)
            assert got["rc"] == mhc.MH_ERR_ARG, what
            assert not got["nbits"].any() and not got["out_off"].any() and not got["out_sym_off"].any(), what
    # no table and no span: nothing to refuse, the plain re-code
    none = tref.tagged_lists([[] for _ in msgs])
    for indexed in (True, False):
        got = splice(src, dst, none[2], no_table, none[0], none[1], indexed)
        plain = src.recode(dst, indexed)
        assert got["rc"] == mhc.MH_OK and np.array_equal(got["payload"], plain["payload"]) and np.array_equal(got["nbits"], plain["nbits"])


def test_order2_and_a_set_of_the_wrong_size_are_refused(mhc, msgs, sources):
    src = sources["o1"]
    m2 = mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    none = tref.tagged_lists([[] for _ in msgs])
    for a, b in ((m2, src.model), (src.model, m2)):
        with pytest.raises(mhc.MhError) as e:
            a.dev_recode_splice_table_batch(b, src.payload, src.pay_off, src.nbits, none[2], TABLE, none[0], none[1], **src.kw(True))
        assert e.value.status == mhc.MH_ERR_ARG
    ms = mhc.ModelSet.train([bytes(m) for m in msgs[:3]], order=1)
    with pytest.raises(mhc.MhError) as e:
        ms.recode_splice_table(src.model, src.payload, src.pay_off, src.nbits, none[2], TABLE, none[0], none[1], **src.kw(True))
    assert e.value.status == mhc.MH_ERR_ARG


# ---- 6. sizes and buffers -------------------------------------------------------------------------------------------------------------

def busy_lists(msgs):
    return mixed_placements(msgs)["mixed runs of touching spans"][0]


@pytest.mark.parametrize("s", ["o1", "set"])
def test_count_only_gives_the_sizes_of_the_full_call(mhc, msgs, sources, dsts, s):
    src, dst = sources[s], dsts["other"]
    span_off, spans, tags = tref.tagged_lists(busy_lists(msgs))
    y, ref, packed = expect(src, dst, tags, TABLE, span_off, spans)
    for indexed in (True, False):
        full = splice(src, dst, tags, TABLE, span_off, spans, indexed)
        check_exact(mhc, src, full, y, ref, packed, indexed)
        count = splice(src, dst, tags, TABLE, span_off, spans, indexed, count_only=True, want_index=False)
        check_exact(mhc, src, count, y, ref, packed, (indexed, "count only"), payload=False, index=False)
        nidx = int(full["out_sym_off"][-1]) // CHUNK + len(msgs)
        count = splice(src, dst, tags, TABLE, span_off, spans, indexed, count_only=True, index_cap=nidx)
        check_exact(mhc, src, count, y, ref, packed, (indexed, "count only, index"), payload=False)


@pytest.mark.parametrize("indexed", [True, False])
def test_a_cap_one_byte_short_and_an_index_one_entry_short(mhc, msgs, sources, dsts, indexed):
    src, dst = sources["o1"], dsts["other"]
    per = insertion_cases(msgs)["16 of 255 bytes into the 256-byte message"]
    span_off, spans, tags = tref.tagged_lists(per)
    full = splice(src, dst, tags, TABLE, span_off, spans, indexed)
    need, nidx = int(full["out_off"][-1]), int(full["out_sym_off"][-1]) // CHUNK + len(msgs)
    assert full["rc"] == mhc.MH_OK and len(full["index"]) == nidx
    for what, kw in (("cap", dict(cap=need - 1, index_cap=nidx)), ("index_cap", dict(cap=need, index_cap=nidx - 1))):
        short = splice(src, dst, tags, TABLE, span_off, spans, indexed, **kw)       # (the wrapper asserts the guards and the fills)
        assert short["rc"] == mhc.MH_ERR_CAPACITY and short["payload"].size == 0, what
        assert (short["index"] == mhc.FIND_FILL).all(), what
        for k in ("out_off", "nbits", "dropped", "status", "out_sym_off", "sym_off"):
            assert np.array_equal(short[k], full[k]), (what, indexed, k)
    roomy = splice(src, dst, tags, TABLE, span_off, spans, indexed, cap=need + 100, index_cap=nidx + 3)
    assert roomy["rc"] == mhc.MH_OK and np.array_equal(roomy["payload"], full["payload"]) and np.array_equal(roomy["index"][:nidx], full["index"])


def test_more_spans_than_the_workspace_was_sized_for(mhc, msgs, sources, dsts):
    src, dst = sources["o1"], dsts["other"]
    per = [[(k, k + 1, 0) for k in range(0, len(m) - 1, 2)] for m in msgs]       # a deletion of every other byte
    span_off, spans, tags = tref.tagged_lists(per)
    assert len(spans) > 1000
    many = splice(src, dst, tags, TABLE, span_off, spans, True, n_spans=len(spans))
    y, ref, packed = expect(src, dst, tags, TABLE, span_off, spans)
    check_exact(mhc, src, many, y, ref, packed, "sized for the spans")
    few = splice(src, dst, tags, TABLE, span_off, spans, True, n_spans=0, count_only=True, want_index=False)
    ws = mhc.lib().mh_dev_recode_splice_table_workspace
    a = (len(msgs), int(src.sym_off[-1]), CHUNK)
    assert ws(*a, len(spans), len(TABLE)) > ws(*a, 0, len(TABLE)) + 256          # (more than the rounding of the workspace leaves)
    assert few["rc"] == mhc.MH_ERR_CAPACITY and not few["nbits"].any()


@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_prefilled_workspace_and_outputs(mhc, msgs, sources, dsts, byte):
    src, dst = sources["o1"], dsts["other"]
    span_off, spans, tags = tref.tagged_lists(busy_lists(msgs))
    y, ref, packed = expect(src, dst, tags, TABLE, span_off, spans)
    with mhc.device_memory("fill", byte):                                       # the workspaces (created without contents) hold `byte`
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, dst, tags, TABLE, span_off, spans, indexed), y, ref, packed, (byte, indexed))


class Raw:
    """The device buffers of raw mh_dev_recode_splice_table_batch calls on one workspace and one set of outputs."""

    def __init__(self, mhc, src, n_spans, n_reps, cap=1 << 16, nidx=96):
        D = mhc.DeviceBuffer
        self.mhc, self.src, self.cap, self.nidx = mhc, src, cap, nidx
        n = self.n = len(src.msgs)
        self.total = int(src.sym_off[-1])
        pl = np.concatenate([src.payload, np.zeros(64, dtype=np.uint8)])
        idx = np.asarray(src.index, dtype=np.uint64)
        self.ins = [D(pl.nbytes, pl), D(src.pay_off.nbytes, src.pay_off), D(src.nbits.nbytes, src.nbits), D(src.sym_off.nbytes, src.sym_off),
                    D(idx.nbytes, idx)]
        self.wsb = mhc.lib().mh_dev_recode_splice_table_workspace(n, self.total, CHUNK, n_spans, n_reps)
        self.d_ws = D(self.wsb, np.full(self.wsb, 0xFF, dtype=np.uint8))
        self.outs = [D(cap, np.full(cap, 0xA5, dtype=np.uint8))] + [D(k * 8, np.full(k, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
                                                                    for k in (n + 1, n, n + 1, nidx, n)]
        self.d_st = D(n * 4, np.full(n, 99, dtype=np.int32))

    def call(self, dst, span_off, spans, tags, reps):
        mhc, D, n = self.mhc, self.mhc.DeviceBuffer, self.n
        roff = np.zeros(len(reps) + 1, dtype=np.uint64)
        roff[1:] = np.cumsum([len(r) for r in reps])
        rb = np.frombuffer(b"".join(reps) + b"\0" * 16, dtype=np.uint8)
        sp = np.concatenate([np.asarray(spans, dtype=np.uint64).reshape(-1), np.zeros(2, dtype=np.uint64)])
        tg = np.concatenate([np.asarray(tags, dtype=np.uint32), np.zeros(4, dtype=np.uint32)])
        bufs = [D(span_off.nbytes, span_off), D(sp.nbytes, sp), D(tg.nbytes, tg), D(roff.nbytes, roff), D(rb.nbytes, rb)]
        d_pl, d_po, d_nb, d_so, d_idx = self.ins
        d_out, d_oo, d_onb, d_oso, d_oi, d_dr = self.outs
        lib = mhc.lib()
        rc = lib.mh_dev_recode_splice_table_batch(self.src.model.handle, dst.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(self.src.pay_off[-1]), 0x20,
                                                  d_so.ptr, self.total, d_idx.ptr, CHUNK, *[b.ptr for b in bufs], len(reps), d_out.ptr, self.cap,
                                                  d_oo.ptr, d_onb.ptr, d_oso.ptr, d_oi.ptr, self.nidx, d_dr.ptr, self.d_st.ptr, self.d_ws.ptr,
                                                  self.wsb, None)
        assert rc == mhc.MH_OK and lib.mh_dev_status(self.d_ws.ptr, None) == mhc.MH_OK

    def check(self, y, ref, packed, what):
        n = self.n
        d_out, d_oo, d_onb, d_oso, d_oi, d_dr = self.outs
        oso = tref.offsets(y)
        need = int(packed[1][n])
        assert need <= self.cap and int(oso[n]) // CHUNK + n <= self.nidx, what
        assert np.array_equal(d_oo.download(np.uint64)[:n + 1], packed[1]) and np.array_equal(d_onb.download(np.uint64)[:n], packed[2]), what
        assert np.array_equal(d_dr.download(np.uint64)[:n], packed[3]) and np.array_equal(d_oso.download(np.uint64)[:n + 1], oso), what
        assert np.array_equal(d_out.download(np.uint8)[:need], packed[0]) and not self.d_st.download(np.int32)[:n].any(), what
        assert np.array_equal(slices_of(d_oi.download(np.uint64), oso, CHUNK), np.concatenate([r[3] for r in ref])), what
        return d_out.download(np.uint8)[:need], d_oo.download(np.uint64)[:n + 1], d_onb.download(np.uint64)[:n], d_oso.download(np.uint64)[:n + 1], \
            d_oi.download(np.uint64)


def test_the_same_workspace_twice_gives_identical_results(mhc, msgs, sources, dsts):
    """Calls on one workspace and one set of outputs, neither cleared in between, two lists and two tables in turn: each
    call's results are those of a call on fresh buffers."""
    src, dst = sources["o1"], dsts["other"]
    a = tref.tagged_lists(busy_lists(msgs))
    b = tref.tagged_lists(insertion_cases(msgs)["touching a deleted span over a seam, front and back"])
    raw = Raw(mhc, src, max(len(a[1]), len(b[1])), len(TABLE))
    for turn, ((span_off, spans, tags), reps) in enumerate(((a, TABLE), (b, TABLE), (a, TABLE[::-1]), (b, TABLE), (a, TABLE))):
        raw.call(dst, span_off, spans, tags, reps)
        raw.check(*expect(src, dst, tags, reps, span_off, spans), turn)


# ---- 7. a source whose tables fill the LDS ----------------------------------------------------------------------------------------------

def test_a_source_whose_tables_fill_the_lds(mhc):
    """The source model of tests/test_gpu_splice.py whose tables leave 144 bytes of LDS: the destination's order-0 image does
    not fit and comes from L2, like the table."""
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
    reps = [b"", bytes(range(10)), bytes(rng.choice(98, size=255).astype(np.uint8)), b"\x01"]
    per = [[(0, 0, 1)], [(0, 1, 1)], [(100, 101, 2), (101, 101, 3)], [(250, 256, 0)], [(0, 2, 3), (254, 257, 0)],
           [(200, 600, 0), (600, 700, 1), (700, 700, 3), (700, 1024, 0), (1024, 1030, 2), (1100, 1100, 1)]]
    span_off, spans, tags = tref.tagged_lists(per)
    for do in (0, 1):
        dst = model_of(mhc, [rng.choice(98, size=60000, p=w / w.sum()).astype(np.uint8).tobytes()], do)
        y, ref, packed = expect(src, dst, tags, reps, span_off, spans)
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, dst, tags, reps, span_off, spans, indexed), y, ref, packed, ("tables fill the LDS", do, indexed))


# ---- 8. the chain: dictionary search -> tagged spans -> table splice -> decode -------------------------------------------------------------

PATS = [b"ing ", b"in", b"ng", b"the", b"he "]                                      # "in" / "ng" / "ing " and "the" / "he " overlap in the text
CHAIN_REPS = [b"<ING>", b"", b"<NG>", b"<THE>", b"#"]


def dict_hits(msgs):
    """The records of a dictionary search in the documented order, ascending (stream, end, pattern), with their patterns."""
    rows = []
    for i, m in enumerate(msgs):
        m = bytes(m)
        for j, p in enumerate(PATS):
            at = m.find(p)
            while at >= 0:
                rows.append((i, at + len(p), j, at))
                at = m.find(p, at + 1)
    rows.sort()
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    for i, _, _, _ in rows:
        off[i + 1] += 1
    off = np.cumsum(off).astype(np.uint64)
    rec = np.array([(i, b, e) for i, e, _, b in rows], dtype=np.uint64).reshape(-1, 3)
    return off, rec, np.array([j for _, _, j, _ in rows], dtype=np.uint32)


def test_chain_dictionary_tagged_spans_table_splice_decode(mhc, msgs):
    w_off, w_rec, w_pat = dict_hits(msgs)
    r_so, r_sp, r_tg = tref.merge_tagged(w_off, w_rec, w_pat)
    assert len(r_sp) >= 10 and len(set(r_tg.tolist())) >= 3 and len(r_sp) < len(w_rec)            # records were merged
    y = tref.apply(msgs, r_so, r_sp, r_tg, CHAIN_REPS)
    model = model_of(mhc, list(msgs) + y, 1)                                    # codes for every pair of y: nothing is dropped
    src = Source(mhc, msgs, model=model)
    d = mhc.Dict(PATS)
    ho, rec, pat, st, rc = model.dev_find_dict_batch(d, src.payload, src.pay_off, src.nbits, **src.kw(True))
    assert rc == mhc.MH_OK and np.array_equal(ho, w_off) and np.array_equal(rec, w_rec) and np.array_equal(pat, w_pat)
    h_so, h_sp, h_tg, rc = mhc.spans_from_hits_tagged(ho, rec, pat)
    assert rc == mhc.MH_OK and np.array_equal(h_so, r_so) and np.array_equal(h_sp, r_sp) and np.array_equal(h_tg, r_tg)
    d_so, d_sp, d_tg, rc = mhc.dev_spans_from_hits_tagged(ho, rec, pat)
    assert rc == mhc.MH_OK and np.array_equal(d_so, r_so) and np.array_equal(d_sp, r_sp) and np.array_equal(d_tg, r_tg)
    u_so, u_sp, rc = mhc.dev_spans_from_hits(ho, rec)
    assert rc == mhc.MH_OK and np.array_equal(u_so, d_so) and np.array_equal(u_sp, d_sp)
    # an overflowed search: MH_ERR_CAPACITY, no span, no tag (the wrapper asserts the fills)
    o_so, o_sp, o_tg, rc = mhc.dev_spans_from_hits_tagged(ho, rec[:5], pat[:5], hit_cap=5)
    assert rc == mhc.MH_ERR_CAPACITY and not o_so.any() and len(o_sp) == 0
    y2, ref, packed = expect(src, model, d_tg, CHAIN_REPS, d_so, d_sp)
    assert y2 == y and not packed[3].any()
    raw = Raw(mhc, src, len(w_rec), len(CHAIN_REPS))
    for turn in range(2):                                                       # a reused workspace
        raw.call(model, d_so, d_sp, d_tg, CHAIN_REPS)
        pay, oo, onb, oso, oi = raw.check(y, ref, packed, turn)
    back, so, st = model.decode_batch(pay, oo, onb, sym_off=oso, index=oi[:int(oso[-1]) // CHUNK + len(msgs)], chunk_symbols=CHUNK)
    assert back == b"".join(y) and np.array_equal(so, oso)
    for indexed in (True, False):
        check_exact(mhc, src, splice(src, model, d_tg, CHAIN_REPS, d_so, d_sp, indexed), y, ref, packed, ("chain", indexed))


# ---- 9. seeded fuzz ---------------------------------------------------------------------------------------------------------------------

def random_case(rng, text):
    n = int(rng.integers(1, 7))
    lens = [int(rng.choice([0, 1, 2, 255, 256, 257, 300, 511, 512, 600, 900])) for _ in range(n)]
    at = int(rng.integers(0, len(text) - 1000))
    batch = [text[at + 7 * i:at + 7 * i + k] for i, k in enumerate(lens)]
    nrep = int(rng.integers(1, 7))
    reps = []
    for _ in range(nrep):
        k = int(rng.choice([0, 0, 0, 255, 255, 1, 2, 3, 10, 40]))
        a = int(rng.integers(0, len(text) - 300))
        reps.append(text[a:a + k])
    per = []
    for k in lens:
        lst, pos = [], 0
        for _ in range(int(rng.integers(0, 12))):
            kind = int(rng.integers(0, 4))
            b = pos if kind == 0 else pos + int(rng.integers(0, max(k // 4, 2)))            # touching the span in front, or behind a gap
            if rng.integers(0, 4) == 0:
                b = (b + CHUNK - 1) // CHUNK * CHUNK                                       # on a chunk boundary
            e = b if kind == 1 else b + int(rng.choice([1, 2, 10, 256, 300]))                # an insertion, or a span
            lst.append((b, e, int(rng.integers(0, nrep))))
            pos = e
        per.append(lst)
    return batch, reps, per


def test_fuzz_of_40_seeds(mhc):
    text = TEXT
    dst = model_of(mhc, [text], 1)
    dst0 = model_of(mhc, [text[:20000]], 0)
    t0 = time.perf_counter()
    spent = 0.0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        batch, reps, per = random_case(rng, text)
        assert all(tref.well_formed([(b, e) for b, e, _ in lst]) for lst in per)
        src = Source(mhc, batch, order=int(seed % 2), each=seed % 5 == 4)
        d = dst0 if seed % 3 == 0 else dst
        span_off, spans, tags = tref.tagged_lists(per)
        y, ref, packed = expect(src, d, tags, reps, span_off, spans)
        t1 = time.perf_counter()
        for indexed in (True, False):
            check_exact(mhc, src, splice(src, d, tags, reps, span_off, spans, indexed), y, ref, packed, (seed, indexed))
        spent += time.perf_counter() - t1
    print("fuzz: %.2f s in the table splice calls, %.2f s in all" % (spent, time.perf_counter() - t0))
    assert time.perf_counter() - t0 < 10.0


# ---- 10. the host form and the CLI ---------------------------------------------------------------------------------------------------------

def test_host_form(mhc, msgs, sources, dsts):
    src, dst = sources["o1"], dsts["other"]
    for per in (busy_lists(msgs), insertion_cases(msgs)["touching a deleted span over a seam, front and back"]):
        span_off, spans, tags = tref.tagged_lists(per)
        y, ref, packed = expect(src, dst, tags, TABLE, span_off, spans)
        oso = tref.offsets(y)
        for indexed in (True, False):
            got = src.model.recode_splice_table_batch(dst, src.payload, src.pay_off, src.nbits, tags, TABLE, span_off, spans, **src.kw(indexed))
            assert got["rc"] == mhc.MH_OK and np.array_equal(got["payload"], packed[0]) and np.array_equal(got["out_off"], packed[1])
            assert np.array_equal(got["nbits"], packed[2]) and np.array_equal(got["dropped"], packed[3]) and np.array_equal(got["sym_off"], src.sym_off)
            assert np.array_equal(got["out_sym_off"], oso)
            assert np.array_equal(slices_of(got["index"], oso, CHUNK), np.concatenate([r[3] for r in ref]))
    # a tag that is no entry fails its stream alone
    per = [[] for _ in msgs]
    per[BIG] = [(5, 9, len(TABLE))]
    per[LAST] = [(5, 9, 1)]
    span_off, spans, tags = tref.tagged_lists(per)
    got = src.model.recode_splice_table_batch(dst, src.payload, src.pay_off, src.nbits, tags, TABLE, span_off, spans, check=False, **src.kw(True))
    assert got["rc"] == mhc.MH_ERR_ARG and [int(s) for s in got["status"]] == [mhc.MH_ERR_ARG if i == BIG else mhc.MH_OK for i in range(len(msgs))]


def test_cli_replace_file(mhc, tmp_path):
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    x = "input_wiki_cpp.txt"
    data = TEXT
    p = lambda n: str(tmp_path / n)
    pats = [b"language", b"age", b"the ", b"C++"]
    reps = [b"<LANG>", b"", b"", b"<CPP>"]                                       # an empty line in the middle, one at the end
    for name, blob in (("x", data), ("x.e", expected_file(x, "e")), ("pats", b"\n".join(pats) + b"\n"), ("reps", b"\n".join(reps) + b"\n")):
        with open(p(name), "wb") as f:
            f.write(blob)
    run = lambda a: subprocess.run([cli] + a, capture_output=True, timeout=300)
    rows = sorted((at + len(pt), j, at) for j, pt in enumerate(pats) for at in range(len(data)) if data.startswith(pt, at))
    off = np.array([0, len(rows)], dtype=np.uint64)
    so, sp, tg = tref.merge_tagged(off, [(0, b, e) for e, _, b in rows], [j for _, j, _ in rows])
    text = tref.apply([data], so, sp, tg, reps)[0]
    assert len(sp) > 20 and len(set(tg.tolist())) == 4
    both = model_of(mhc, [data, text], 1).table_bytes()
    with open(p("both.e"), "wb") as f:
        f.write(both)
    with open(p("spliced"), "wb") as f:
        f.write(text)
    assert run([p("x"), "-e", p("x.e"), "-o", p("x.cm"), "--index", p("x.idx"), "--chunk", "256"]).returncode == 0
    assert run([p("spliced"), "-e", p("both.e"), "-o", p("m.cm"), "--index", p("m.idx"), "--chunk", "256"]).returncode == 0
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("both.e"), "-o", p("out.cm"), "--index", p("x.idx"), "--redact-file", p("pats"),
             "--replace-file", p("reps")])
    assert r.returncode == 0 and b"skipped" not in r.stderr, r.stderr
    blob, _ = mh_oracle.Model.from_table(both).compress(text)
    assert open(p("out.cm"), "rb").read() == blob == open(p("m.cm"), "rb").read()
    assert open(p("out.cm.idx"), "rb").read() == open(p("m.idx"), "rb").read()
    removed = int((sp[:, 1] - sp[:, 0]).sum())
    inserted = sum(len(reps[t]) for t in tg.tolist())
    assert ("Replacing %d bytes in %d spans with %d bytes." % (removed, len(sp), inserted)).encode() in r.stderr, r.stderr
    r = run([p("out.cm"), "-x", "-e", p("both.e"), "-o", p("back"), "--index", p("out.cm.idx")])
    assert r.returncode == 0 and open(p("back"), "rb").read() == text, r.stderr
