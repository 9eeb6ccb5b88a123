"""The table splice of an order-2 source on the GPU (include/mh.h, "ORDER 2 IN EDITING AND SPLICING"): 2 -> 2, 2 -> 1 and 2 -> 0.
The reference is the composition: splice_table_ref.apply on the original messages, then the batch encoder under dst
(encode_batch_o2 / encode_batch); tests/edit_o2_ref.py names, in a failure, the two output bytes a chunk's lane had to start
from.  Every comparison is exact.  The device-call wrappers put guards around every output.

The enumerated batches hold one stream of 700 text bytes per case, so that every case meets the chunk boundaries at 256 and 512
of its own stream in one call; the ragged batch is tests/test_gpu_edit_o2.py's."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import edit_o2_ref
import splice_table_ref
from test_gpu_coded_o2 import World, slices, text
from test_gpu_edit_o2 import SHAPES, ragged

pytestmark = pytest.mark.gpu

DSTS = [2, 1, 0]
F = 256
REPS = [b"", b"R", b"ST", b"UVWXY"]                                           # by length: 0, 1, 2, 5


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def encoder(dst, do, edited, prev0, chunk):
    return (dst.encode_batch_o2 if do == 2 else dst.encode_batch)(edited, prev0=prev0, chunk_symbols=chunk)


def check(mhc, got, enc, edited, chunk, tag, name=None, payload=True):
    """Every output against the encoder's for the edited messages; name(i): what to say about stream i when it differs."""
    e_pay, e_off, e_nb, e_idx, e_so = enc
    assert got["rc"] == mhc.MH_OK and not got["status"].any(), (tag, got["rc"], got["status"])
    assert np.array_equal(got["out_sym_off"], splice_table_ref.offsets(edited)), tag
    for i in range(len(edited)):
        a, b = int(e_off[i]), int(e_off[i + 1])
        g0, g1 = int(got["out_off"][i]), int(got["out_off"][i + 1])
        same = int(got["nbits"][i]) == int(e_nb[i]) and (not payload or np.array_equal(got["payload"][g0:g1], e_pay[a:b]))
        assert same, (tag, i, name(i) if name else None)
    assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb), tag
    if payload:
        assert np.array_equal(got["payload"], e_pay), tag
    if not payload:
        assert got["payload"] is None and got["index"] is None, tag            # count only
        return
    for i in range(len(edited)):                                              # the index laid out by output positions
        assert np.array_equal(slices(got["index"], e_so, chunk, only=[i]), slices(e_idx, e_so, chunk, only=[i])), (tag, i, name(i) if name else None)


class Batch:
    """Messages with per-stream lists of (begin, end, tag) over `reps`, the source world and a destination world trained on
    the originals and the spliced messages."""

    def __init__(self, mhc, msgs, lists, reps, prev0=0x20):
        self.mhc, self.msgs, self.lists, self.reps, self.prev0 = mhc, msgs, lists, reps, prev0
        self.span_off, self.spans, self.tags = splice_table_ref.tagged_lists(lists)
        self.edited = splice_table_ref.apply(msgs, self.span_off, self.spans, self.tags, reps)
        self.w = World(mhc, msgs, prev0=prev0)
        self.d = World(mhc, msgs + self.edited, prev0=prev0)

    def name(self, i):
        ctx = {f: edit_o2_ref.start_context([self.msgs[i]], [0, len(self.lists[i])], [p[:2] for p in self.lists[i]], [p[2] for p in self.lists[i]],
                                            self.reps, f, self.prev0)[0] for f in (256, 512, 1024, 2048)}
        return "spans %s; the lanes start from %s" % (self.lists[i], {f: "%04x" % c for f, c in ctx.items() if c is not None})

    def run(self, do, chunk, indexed, dst=None, **more):
        src, kw = self.w.kw(2, chunk, indexed)
        return self.w.model[2].dev_recode_splice_table_batch_o2(dst or self.d.model[do], *src, self.tags, self.reps, self.span_off, self.spans,
                                                                **kw, **more)

    def check_all(self, do, shapes=SHAPES):
        for chunk, indexed in shapes:
            enc = encoder(self.d.model[do], do, self.edited, self.prev0, chunk)
            check(self.mhc, self.run(do, chunk, indexed), enc, self.edited, chunk, (do, chunk, indexed), self.name)


# ---- 1. enumerated boundary cases -----------------------------------------------------------------------------------------------

def boundary_lists():
    out = []
    for b in range(F - 3, F + 4):
        for e in range(b, F + 4):
            for t in range(4):
                me = (b, e, t)
                out.append([me])
                out.append([(b - 4, b, 0), me])                                # a deleted span that ends at begin
                out.append([(b - 4, b, 1), me])                                # a one-byte-replaced span that ends at begin
                out.append([(b - 9, b - 6, 0), (b - 6, b - 2, 1), (b - 2, b, 0), me])   # a chain of three
                out.append([(b - 7, b - 3, 0), (b - 3, b - 3, 0), (b - 3, b, 0), me])   # a chain of three, all empty, an insertion in it
                out.append([(b - 5, b - 1, 0), me])                            # one byte apart: x[begin - 1] stands between two deletions
    return out


@pytest.fixture(scope="module")
def boundary(mhc):
    lists = boundary_lists()
    assert len(lists) == 28 * 4 * 6
    return Batch(mhc, [text(700, 7)] * len(lists), lists, REPS)


@pytest.mark.parametrize("do", DSTS)
def test_enumerated_boundary_cases(mhc, boundary, do):
    """One stream per (begin, end, rep_len) with F - 3 <= begin <= end <= F + 3 around F = 256 and rep_len in {0, 1, 2, 5}, alone
    and with a touching neighbour in front, in one batch and one call."""
    starts = {edit_o2_ref.start_context([boundary.msgs[0]], [0, len(l)], [p[:2] for p in l], [p[2] for p in l], REPS, F, 0x20)[0] for l in boundary.lists}
    x = boundary.msgs[0]
    for pair in [(x[F - 2], x[F - 1]), (ord("X"), ord("Y")), (ord("S"), ord("T")), (x[F - 4], ord("R")), (ord("R"), x[F - 1]), (x[F - 3], x[F - 1]),
                 (ord("R"), ord("R")), (x[F - 8], ord("R"))]:                    # the entry, a tail, a tail and a byte, a look-back, a chain
        assert (pair[0] << 8) | pair[1] in starts, pair
    boundary.check_all(do, [(256, True), (256, False)])


# ---- 2. position 0 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("do", DSTS)
def test_position_0_whole_chunks_and_insertions_at_one_position(mhc, do):
    lists = [[(0, 5, 0)], [(0, 1, 0)], [(0, 1, 1)], [(0, F, 0)], [(0, F, 1)], [(0, F + 1, 0)], [(0, F - 1, 0)], [(0, 2 * F, 0)], [(0, 700, 0)],
             [(0, 9000, 0)], [(0, 700, 3)], [(0, 0, 3)], [(0, 0, 1), (0, 0, 2)], [(0, 0, 1), (0, F, 0)], [(0, 0, 0), (0, F, 0), (F, F, 1)],
             [(F, F, 1), (F, F, 2), (F, F, 0), (F, F, 3)], [(F - 1, F - 1, 1), (F - 1, F - 1, 2)], [(F - 1, F - 1, 1), (F - 1, F - 1, 0), (F - 1, F, 0)],
             [(F - 1, F - 1, 1), (F, F, 1)], [(F - 2, F - 2, 1), (F - 2, F - 1, 0), (F - 1, F - 1, 1), (F - 1, F, 0), (F, F, 1)],
             [(1, F, 0)], [(2, F, 0)], [(1, F - 1, 0)], [(0, 1, 0), (1, F, 1)], [(699, 700, 0)], [(699, 699, 2)], [(700, 700, 2)], [(700, 800, 2)]]
    b = Batch(mhc, [text(700, 9)] * len(lists), lists, REPS)
    assert b.edited[8] == b"" and b.edited[9] == b"" and b.edited[3] == b.msgs[3][F:] and b.edited[-1] == b.msgs[0] and b.edited[-2] == b.msgs[0]
    b.check_all(do, [(256, True), (256, False)])


# ---- 3. a mixed table from a dictionary search ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prev0", [0x20, 0x65])
@pytest.mark.parametrize("do", DSTS)
def test_tagged_spans_of_a_dictionary_search_under_a_mixed_table(mhc, do, prev0):
    msgs = ragged()
    w = World(mhc, msgs, prev0=prev0)
    pats = [b"or", b"e ", b"um", b"\x00", b"it a", b"lor"]
    absent = np.flatnonzero(w.h[0] == 0)                                        # a byte the batch lacks: without a code under any order
    assert absent.size, "the ragged batch uses every byte value"
    reps = [b"<OR>", b"", bytes([int(absent[0])]), b"[a longer replacement]"]
    src, kw = w.kw(2, 256, True)
    ho, rec, pat, st, rc = w.model[2].dev_find_dict_batch_o2(mhc.Dict(pats), *src, **kw)
    assert rc == mhc.MH_OK and not st.any()
    span_off, spans, tags, rc = mhc.dev_spans_from_hits_tagged(ho, rec, pat)
    assert rc == mhc.MH_OK and len(spans) > 100
    tags = tags % 4                                                             # six patterns onto four entries, one of them empty
    assert set(tags.tolist()) == {0, 1, 2, 3}
    lists = [[(int(spans[r][0]), int(spans[r][1]), int(tags[r])) for r in range(int(span_off[i]), int(span_off[i + 1]))] for i in range(len(msgs))]
    b = Batch(mhc, msgs, lists, reps, prev0=prev0)
    b.check_all(do)
    enc = encoder(b.d.model[do], do, b.edited, prev0, 1024)
    count = b.run(do, 1024, True, count_only=True)
    check(mhc, count, enc, b.edited, 1024, (do, "count only"), payload=False)
    dst = b.d.model[do]
    got = b.run(do, 256, False)
    back, _, st = (dst.decode_batch_o2 if do == 2 else dst.decode_batch)(got["payload"], got["out_off"], got["nbits"], prev0=prev0)
    assert back == b"".join(b.edited) and not np.asarray(st).any()
    # the destination trained on the originals alone: the replacements' bytes and both of their edges are dropped and counted
    lean = b.w.model[do]
    want = [edit_o2_ref.dropped(m, b.w.h[do], prev0) for m in b.edited]
    got = b.run(do, 256, True, dst=lean)
    assert got["dropped"].tolist() == want
    assert sum(want) > (50 if do else 0)                                        # (order 0 has one context: the absent byte alone is dropped)
    assert np.array_equal(got["payload"], encoder(lean, do, b.edited, prev0, 256)[0])


# ---- 4. equivalence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("do", DSTS)
def test_a_one_entry_table_with_the_identity_replacement_is_the_plain_recode(mhc, do):
    msgs = ragged()
    word = b"dolor"
    lists = []
    for m in msgs:
        at, lst = 0, []
        while (at := m.find(word, at)) >= 0:
            lst.append((at, at + len(word), 0))
            at += len(word)
        lists.append(lst)
    assert sum(len(l) for l in lists) > 20
    b = Batch(mhc, msgs, lists, [word])
    assert b.edited == msgs
    for chunk, indexed in SHAPES:
        src, kw = b.w.kw(2, chunk, indexed)
        plain = b.w.model[2].dev_recode_batch_o2(b.d.model[do], *src, **kw)
        got = b.run(do, chunk, indexed)
        for k in ("rc", "status", "out_off", "nbits", "payload", "dropped", "sym_off"):
            assert np.array_equal(got[k], plain[k]), (do, chunk, indexed, k)
        assert np.array_equal(got["out_sym_off"], plain["sym_off"])
        assert np.array_equal(slices(got["index"], got["sym_off"], chunk), slices(plain["index"], plain["sym_off"], chunk)), (do, chunk, indexed)


# ---- 5. the remaining rules -------------------------------------------------------------------------------------------------------

def test_an_order_01_source_under_an_order_2_destination_is_refused(mhc, boundary):
    w = boundary.w
    for so, do in [(1, 2), (0, 2), (1, 1), (0, 0)]:
        src, kw = w.kw(so, 256, True)
        with pytest.raises(mhc.MhError) as e:
            w.model[so].dev_recode_splice_table_batch_o2(w.model[do], *src, boundary.tags, REPS, boundary.span_off, boundary.spans, **kw)
        assert e.value.status == mhc.MH_ERR_ARG, (so, do)


def test_more_spans_than_the_workspace_was_sized_for(mhc, boundary):
    assert len(boundary.spans) > 1000                                          # far more than the rounding of the workspace leaves
    got = boundary.run(2, 256, True, cap=1 << 20, index_cap=4096, n_spans=0)
    assert got["rc"] == mhc.MH_ERR_CAPACITY


@pytest.mark.parametrize("do", [2, 1])
def test_a_tag_out_of_range_fails_its_stream_alone(mhc, do):
    msgs = ragged()
    n, bad = len(msgs), 23
    lists = [[(3, 9, 1)] if len(m) > 3 else [] for m in msgs]
    b = Batch(mhc, msgs, lists, REPS)
    tags = b.tags.copy()
    tags[int(b.span_off[bad])] = 4
    for chunk, indexed in SHAPES:
        src, kw = b.w.kw(2, chunk, indexed)
        got = b.w.model[2].dev_recode_splice_table_batch_o2(b.d.model[do], *src, tags, REPS, b.span_off, b.spans, **kw)
        enc = encoder(b.d.model[do], do, b.edited, 0x20, chunk)
        assert got["rc"] == mhc.MH_ERR_ARG and got["status"][bad] == mhc.MH_ERR_ARG and not np.delete(got["status"], bad).any()
        assert got["nbits"][bad] == 0 and got["out_off"][bad + 1] == got["out_off"][bad]
        for i in range(n):
            if i != bad:
                a, e = int(enc[1][i]), int(enc[1][i + 1])
                assert np.array_equal(got["payload"][int(got["out_off"][i]):int(got["out_off"][i + 1])], enc[0][a:e]), (do, chunk, indexed, i)


# ---- 6. the host form -------------------------------------------------------------------------------------------------------------

def host_check(mhc, got, enc, edited, src_sym_off, chunk, tag, index=True):
    e_pay, e_off, e_nb, e_idx, e_so = enc
    assert got["rc"] == mhc.MH_OK and not got["status"].any(), (tag, got["rc"], got["status"])
    assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb), tag
    assert np.array_equal(got["out_sym_off"], splice_table_ref.offsets(edited)) and np.array_equal(got["sym_off"], src_sym_off), tag
    assert np.array_equal(got["payload"], e_pay) and not got["dropped"].any(), tag
    if index:
        assert np.array_equal(slices(got["index"], e_so, chunk), slices(e_idx, e_so, chunk)), tag
    else:
        assert got["index"] is None, tag


@pytest.mark.parametrize("do", DSTS)
def test_the_host_form_equals_the_encoder(mhc, boundary, do):
    """mh_recode_splice_table_batch_o2 through Model.recode_splice_table_batch_o2 on the enumerated boundary cases, indexed and
    index-free, with and without the destination index."""
    b = boundary
    for chunk, indexed in SHAPES:
        (pay, off, nb), kw = b.w.kw(2, chunk, indexed)
        enc = encoder(b.d.model[do], do, b.edited, b.prev0, chunk)
        sym = b.w.enc(2, chunk)[4]
        got = b.w.model[2].recode_splice_table_batch_o2(b.d.model[do], pay, off, nb, b.tags, b.reps, b.span_off, b.spans, **kw)
        host_check(mhc, got, enc, b.edited, sym, chunk, (do, chunk, indexed))
        got = b.w.model[2].recode_splice_table_batch_o2(b.d.model[do], pay, off, nb, b.tags, b.reps, b.span_off, b.spans, want_index=False, **kw)
        host_check(mhc, got, enc, b.edited, sym, chunk, (do, chunk, indexed, "no index"), index=False)
    src, kw = b.w.kw(1, 256, True)
    with pytest.raises(mhc.MhError) as e:                                       # left out: an order-0/1 source
        b.w.model[1].recode_splice_table_batch_o2(b.d.model[2], *src, b.tags, b.reps, b.span_off, b.spans, **kw)
    assert e.value.status == mhc.MH_ERR_ARG


@pytest.mark.parametrize("do", [2, 1])
def test_the_host_form_indexes_a_batch_with_a_stream_over_the_walk_cap_first(mhc, do):
    """Index-free, one stream over MH_BATCH_WALK_MAX_BITS under an order-2 source: indexed first by mh_index_batch_o2, never
    refused.  In the long stream a deletion across a chunk boundary, a one-byte replacement that ends in front of one and an
    insertion; a span in the first stream."""
    from test_gpu_edit_o2 import skewed_model
    long_msg = np.random.default_rng(61).integers(0, 256, 1_000_000 + 77, dtype=np.uint8).tobytes()
    msgs = [b"a few bytes", long_msg, b""]
    src, dst = skewed_model(mhc, 2), skewed_model(mhc, do)
    pay, off, nb, _, sym = src.encode_batch_o2(msgs, chunk_symbols=256)
    assert int(nb[1]) > mhc.BATCH_WALK_MAX_BITS
    F = 700_160                                                                 # a multiple of 256
    lists = [[(2, 5, 1)], [(F - 40, F + 3, 0), (F + 250, F + 255, 1), (F + 512, F + 512, 3), (900_000, 900_100, 2)], []]
    span_off, spans, tags = splice_table_ref.tagged_lists(lists)
    edited = splice_table_ref.apply(msgs, span_off, spans, tags, REPS)
    enc = encoder(dst, do, edited, 0x20, 256)
    for want_index in (True, False):
        got = src.recode_splice_table_batch_o2(dst, pay, off, nb, tags, REPS, span_off, spans, chunk_symbols=256, want_index=want_index, check=False)
        host_check(mhc, got, enc, edited, sym, 256, (do, want_index), index=want_index)
