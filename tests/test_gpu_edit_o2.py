"""Masked re-coding with an order-2 model on a side, on the GPU (include/mh.h, "ORDER 2 IN EDITING AND SPLICING"): source ->
destination 2 -> 2, 2 -> 1, 2 -> 0, 1 -> 2 and 0 -> 2.  The reference is the composition: edit_ref.apply on the original messages,
then the batch encoder under dst (encode_batch_o2 / encode_batch, which other modules pin to the oracle); the dropped counts
come from tests/edit_o2_ref.py.  Every comparison is exact.  The device-call wrappers put guards around every output.

Chunks 256 and 1024 indexed, 256 index-free.  The ragged batch has lengths 0, 1, 2, 3, 255, 256, 257, 258, 511, 512, 513, 700 and
3 000 as text and as Zipf: an empty stream, streams shorter than a context, one symbol on either side of one and two chunk
boundaries, and a stream of several chunks of both sizes; once under prev0 = 0x20 and once under a prev0 that is a live symbol."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import edit_o2_ref
import edit_ref
from test_gpu_coded_o2 import World, damaged, dev_decode, slices, text, zipf

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 3, 255, 256, 257, 258, 511, 512, 513, 700, 3000]
PAIRS = [(2, 2), (2, 1), (2, 0), (1, 2), (0, 2)]
SHAPES = [(256, True), (1024, True), (256, False)]
STAR = edit_ref.mask_map(0x2A)
FOLD = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))          # to upper case: moves most bytes of the text
IDENT = bytes(range(256))
NEXT = bytes((c + 1) & 0xFF for c in range(256))                             # moves every byte
PATTERNS = [b"or", b"e ", b"um", b"\x00\x01", b"\x01", b"it a"]


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def ragged():
    msgs = []
    for k, n in enumerate(LENS):
        msgs += [text(n, 110 + k), zipf(n, 140 + k)]
    return msgs


def span_lists(per_stream):
    off = np.zeros(len(per_stream) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in per_stream], dtype=np.uint64)
    return off, np.array([p for s in per_stream for p in s], dtype=np.uint64).reshape(-1, 2)


class Case:
    """A world (the batch, its models, its coded forms), the span lists of a real order-2 search in it, and a destination
    world trained on the originals and on every edited form the tests code, so that no pair of those lacks a code."""

    def __init__(self, mhc, msgs, prev0):
        self.mhc, self.w = mhc, World(mhc, msgs, prev0=prev0)
        src, kw = self.w.kw(2, 256, True)
        ho, rec, _, st, rc = self.w.model[2].dev_find_batch_o2(mhc.PatternSet(PATTERNS), *src, **kw)
        assert rc == mhc.MH_OK and not st.any()
        self.span_off, self.spans, rc = mhc.dev_spans_from_hits(ho, rec)
        assert rc == mhc.MH_OK and len(self.spans) > 100
        self.edits = {"mask": (STAR, self.span_off, self.spans), "fold": (FOLD, self.span_off, self.spans), "fold all": (FOLD, None, None),
                      "mask all": (STAR, None, None)}
        self.edited = {k: edit_ref.apply(msgs, so, sp, m) for k, (m, so, sp) in self.edits.items()}
        self.d = World(mhc, msgs + [m for e in self.edited.values() for m in e], prev0=prev0)
        self.enc = {}

    def expect(self, what, do, chunk, dst=None):
        """The batch encoder's output under dst (default: the destination world's model of order do) for an edited form."""
        key = (what, do, chunk, id(dst))
        if key not in self.enc:
            m = dst or self.d.model[do]
            fn = m.encode_batch_o2 if do == 2 else m.encode_batch
            self.enc[key] = fn(self.edited[what], prev0=self.w.prev0, chunk_symbols=chunk)
        return self.enc[key]

    def run(self, what, so, do, chunk, indexed, dst=None, **more):
        byte_map, span_off, spans = self.edits[what]
        src, kw = self.w.kw(so, chunk, indexed)
        return self.w.model[so].dev_recode_edit_batch_o2(dst or self.d.model[do], *src, byte_map, span_off, spans, **kw, **more)


@pytest.fixture(scope="module")
def cases(mhc):
    msgs = ragged()
    return {p0: Case(mhc, msgs, p0) for p0 in (0x20, 0x65)}                   # 'e': (prev0, prev0) and (prev0, y0) are live contexts


def check(mhc, got, enc, chunk, drops, tag, payload=True):
    e_pay, e_off, e_nb, e_idx, e_so = enc
    assert got["rc"] == mhc.MH_OK and not got["status"].any(), (tag, got["rc"], got["status"])
    assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb), tag
    assert np.array_equal(got["sym_off"], e_so), tag
    assert got["dropped"].tolist() == drops, (tag, got["dropped"].tolist(), drops)
    if payload:
        assert np.array_equal(got["payload"], e_pay), tag
    assert np.array_equal(slices(got["index"], e_so, chunk), slices(e_idx, e_so, chunk)), tag


# ---- 1. equals the encoder ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prev0", [0x20, 0x65])
@pytest.mark.parametrize("so,do", PAIRS)
def test_equals_the_encoder(mhc, cases, so, do, prev0):
    c = cases[prev0]
    none = [0] * c.w.n
    for chunk, indexed in SHAPES:
        for what in ("mask", "fold", "fold all"):
            tag = (so, do, prev0, chunk, indexed, what)
            enc = c.expect(what, do, chunk)
            got = c.run(what, so, do, chunk, indexed)
            check(mhc, got, enc, chunk, none, tag)
            if what == "mask":
                count = c.run(what, so, do, chunk, indexed, count_only=True, sym_total=None if indexed else int(enc[4][-1]))
                check(mhc, count, enc, chunk, none, tag + ("count only",), payload=False)
                assert count["payload"] is None
        dst = c.d.model[do]
        back, _, st = (dst.decode_batch_o2 if do == 2 else dst.decode_batch)(got["payload"], got["out_off"], got["nbits"], prev0=prev0)
        assert back == b"".join(c.edited["fold all"]) and not np.asarray(st).any(), tag
    assert c.edited["mask"] != c.w.msgs and c.edited["fold"] != c.edited["fold all"]


# ---- 2. every alignment at a boundary -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,do", PAIRS)
def test_every_alignment_at_a_boundary(mhc, so, do):
    """One stream per (begin, end) with F - 3 <= begin < end <= F + 3 around F = 256 and F = 512; NEXT moves every byte, so each of
    y[F - 2], y[F - 1], y[F], y[F + 1] is edited or not in every combination: the seam's close and head and an order-2 entry's two
    bytes each come out right only when every one of them is mapped at its own position."""
    base = text(700, 7)
    per = [[(b, e)] for F in (256, 512) for b in range(F - 3, F + 3) for e in range(b + 1, F + 4)]
    assert len(per) == 2 * 21
    combos = {tuple(b <= p < e for p in (F - 2, F - 1, F, F + 1)) for F in (256,) for (b, e), in per[:21]}
    assert len(combos) >= 9
    msgs = [base] * len(per)
    span_off, spans = span_lists(per)
    edited = edit_ref.apply(msgs, span_off, spans, NEXT)
    w = World(mhc, msgs)
    d = World(mhc, msgs + edited)
    dst = d.model[do]
    enc = (dst.encode_batch_o2 if do == 2 else dst.encode_batch)(edited, prev0=w.prev0, chunk_symbols=256)
    for indexed in (True, False):
        src, kw = w.kw(so, 256, indexed)
        got = w.model[so].dev_recode_edit_batch_o2(dst, *src, NEXT, span_off, spans, **kw)
        assert got["rc"] == mhc.MH_OK and not got["status"].any()
        for i, lst in enumerate(per):                                          # name the alignment that went wrong
            a, b = int(enc[1][i]), int(enc[1][i + 1])
            assert int(got["nbits"][i]) == int(enc[2][i]) and np.array_equal(got["payload"][int(got["out_off"][i]):int(got["out_off"][i + 1])],
                                                                             enc[0][a:b]), (so, do, indexed, lst)
        check(mhc, got, enc, 256, [0] * len(per), (so, do, indexed))


# ---- 3. drops, codes over 56 bits -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,do", PAIRS)
def test_a_mask_byte_without_a_code_in_some_contexts_is_dropped_and_counted(mhc, cases, so, do):
    """The destination is trained on the ORIGINAL messages: '*' follows few contexts there, so most masked pairs have no code."""
    c = cases[0x20]
    dst = c.w.model[do]
    what = "mask"
    if do == 0:                                                                 # one context: a byte has a code or has none, so a byte the batch lacks
        absent = np.flatnonzero(c.w.h[0] == 0)
        assert absent.size, "the ragged batch uses every byte value"
        what = "mask with an absent byte"
        if what not in c.edits:
            c.edits[what] = (edit_ref.mask_map(int(absent[0])), c.span_off, c.spans)
            c.edited[what] = edit_ref.apply(c.w.msgs, c.span_off, c.spans, c.edits[what][0])
    want = [edit_o2_ref.dropped(m, c.w.h[do], 0x20) for m in c.edited[what]]
    assert sum(want) > 100
    for chunk, indexed in SHAPES:
        check(mhc, c.run(what, so, do, chunk, indexed, dst=dst), c.expect(what, do, chunk, dst=dst), chunk, want, (so, do, chunk, indexed))


def fib_model(mhc):
    """test_gpu_coded_o2's destination: Fibonacci counts over 62 symbols in every context of them and of prev0: codes of up to 61 bits."""
    fib = [1, 1]
    while len(fib) < 62:
        fib.append(fib[-1] + fib[-2])
    syms = list(range(62))
    counts = np.zeros(1 << 24, dtype=np.uint64)
    for b2 in syms + [0x20]:
        for b1 in syms + [0x20]:
            ctx = (b2 << 8) | b1
            counts[(ctx << 8):(ctx << 8) + 62] = fib[::-1] if (b1 + b2) % 2 else fib
    return mhc.Model.from_counts(counts, 2)


def test_codes_over_56_bits_in_an_order_2_destination(mhc):
    dst = fib_model(mhc)
    assert dst.max_code_len > 56
    rng = np.random.default_rng(16)
    msgs = [bytes(rng.integers(0, 62, int(k)).astype(np.uint8)) for k in (0, 1, 2, 17, 1000, 3000, 3)]
    msgs.append(bytes([0] * 300 + [61] * 300))
    rot = bytes((c + 31) % 62 if c < 62 else c for c in range(256))            # stays inside the 62 symbols
    per = [[(0, 1), (3, 9), (250, 260), (500, 520), (1020, 1030)] for _ in msgs]
    span_off, spans = span_lists(per)
    edited = edit_ref.apply(msgs, span_off, spans, rot)
    assert edited != msgs
    w = World(mhc, msgs)
    for chunk, indexed in SHAPES:
        enc = dst.encode_batch_o2(edited, prev0=0x20, chunk_symbols=chunk)
        for so in (1, 2):
            src, kw = w.kw(so, chunk, indexed)
            got = w.model[so].dev_recode_edit_batch_o2(dst, *src, rot, span_off, spans, **kw)
            check(mhc, got, enc, chunk, [0] * len(msgs), ("fib", so, chunk, indexed))


# ---- 4. equivalence -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,do", PAIRS)
def test_the_identity_map_and_an_empty_list_equal_the_plain_recode(mhc, cases, so, do):
    c = cases[0x65]
    dst = c.d.model[do]
    empty = np.zeros(c.w.n + 1, dtype=np.uint64)
    for chunk, indexed in SHAPES:
        src, kw = c.w.kw(so, chunk, indexed)
        plain = c.w.model[so].dev_recode_batch_o2(dst, *src, **kw)
        for byte_map, span_off, spans in [(IDENT, None, None), (IDENT, c.span_off, c.spans), (STAR, empty, None)]:
            got = c.w.model[so].dev_recode_edit_batch_o2(dst, *src, byte_map, span_off, spans, **kw)
            for k in ("rc", "status", "out_off", "nbits", "payload", "index", "dropped", "sym_off"):
                assert np.array_equal(got[k], plain[k]), (so, do, chunk, indexed, k)


# ---- 5. malformed lists, damaged streams ------------------------------------------------------------------------------------------

def streams_equal(got, enc, only, tag):
    for i in only:
        a, b = int(enc[1][i]), int(enc[1][i + 1])
        assert int(got["nbits"][i]) == int(enc[2][i]), (tag, i)
        assert np.array_equal(got["payload"][int(got["out_off"][i]):int(got["out_off"][i + 1])], enc[0][a:b]), (tag, i)


@pytest.mark.parametrize("so,do", [(2, 2), (1, 2), (2, 1)])
def test_a_malformed_list_fails_its_stream_alone(mhc, cases, so, do):
    c = cases[0x20]
    n, bad = c.w.n, 23                                                          # a 700-byte stream in the middle of the batch
    for name, lst in [("overlap", [(10, 20), (19, 30)]), ("empty span", [(5, 5)]), ("descending", [(300, 310), (100, 110)])]:
        per = [[(3, 9)] if i != bad else lst for i in range(n)]
        span_off, spans = span_lists(per)
        good = span_lists([[(3, 9)] if i != bad else [] for i in range(n)])
        edited = edit_ref.apply(c.w.msgs, good[0], good[1], STAR)
        for chunk, indexed in SHAPES:
            dst = c.d.model[do]
            enc = (dst.encode_batch_o2 if do == 2 else dst.encode_batch)(edited, prev0=0x20, chunk_symbols=chunk)
            src, kw = c.w.kw(so, chunk, indexed)
            got = c.w.model[so].dev_recode_edit_batch_o2(dst, *src, STAR, span_off, spans, **kw)
            tag = (name, so, do, chunk, indexed)
            assert got["rc"] == mhc.MH_ERR_ARG and got["status"][bad] == mhc.MH_ERR_ARG and not np.delete(got["status"], bad).any(), tag
            assert got["nbits"][bad] == 0 and got["out_off"][bad + 1] == got["out_off"][bad] and got["dropped"][bad] == 0, tag
            streams_equal(got, enc, [i for i in range(n) if i != bad], tag)


@pytest.mark.parametrize("kind", ["flip", "cut", "extended"])
@pytest.mark.parametrize("so,do", [(2, 2), (1, 2), (2, 0)])
def test_damaged_streams_get_the_batch_decoders_verdicts(mhc, cases, so, do, kind):
    c = cases[0x20]
    w, dst = c.w, c.d.model[do]
    for chunk, indexed in SHAPES:
        pay, off, nb, idx, sym, hit = damaged(w, so, chunk, kind)
        kw = dict(prev0=0x20, chunk_symbols=chunk)
        if indexed:
            kw.update(sym_off=sym, index=idx)
        _, want = dev_decode(mhc, w.model[so], so == 2, pay, off, nb, **kw)     # what the batch decoder makes of the same arguments
        got = w.model[so].dev_recode_edit_batch_o2(dst, pay, off, nb, STAR, c.span_off, c.spans, **kw)
        tag = (kind, so, do, chunk, indexed)
        assert np.array_equal(got["status"], want) and not np.delete(want, hit).any(), (tag, want)
        if indexed and kind != "flip":
            assert want[hit] != mhc.MH_OK, tag                                  # the last chunk must end exactly at nbits
        if want[hit] != mhc.MH_OK:
            assert got["nbits"][hit] == 0 and got["out_off"][hit + 1] == got["out_off"][hit] and got["dropped"][hit] == 0, tag
        streams_equal(got, c.expect("mask", do, chunk), [i for i in range(w.n) if i != hit], tag)   # (a damaged stream that still decodes is another message)


# ---- 6. capacity, workspace, refusals -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,do", [(2, 2), (0, 2)])
def test_one_byte_short_is_a_capacity_error_with_nothing_written(mhc, cases, so, do):
    c = cases[0x20]
    for chunk, indexed in SHAPES:
        enc = c.expect("mask", do, chunk)
        total = int(enc[1][-1])
        st = None if indexed else int(enc[4][-1])
        got = c.run("mask", so, do, chunk, indexed, cap=total - 1, sym_total=st)       # (the wrapper asserts: nothing at or past cap)
        assert got["rc"] == mhc.MH_ERR_CAPACITY and np.array_equal(got["out_off"], enc[1]), (so, do, chunk, indexed)
        assert np.array_equal(c.run("mask", so, do, chunk, indexed, cap=total, sym_total=st)["payload"], enc[0])


class Raw:
    """One mh_dev_recode_edit_batch_o2 call assembled by hand on an indexed batch: every buffer the caller's own."""

    def __init__(self, mhc, c, so, do, chunk, guard=4096):
        self.mhc, self.lib = mhc, mhc.lib()
        (pay, off, nb), kw = c.w.kw(so, chunk, True)
        n = self.n = c.w.n
        enc = c.expect("mask", do, chunk)
        self.total = int(enc[1][-1])
        sym, idx = np.ascontiguousarray(kw["sym_off"]), np.ascontiguousarray(kw["index"])
        D = mhc.DeviceBuffer
        self.wsb = self.lib.mh_dev_recode_edit_batch_o2_workspace(n, int(sym[n]), chunk)
        self.guard = guard
        self.bufs = dict(pay=D(pay.size + 64, pay), off=D(off.nbytes, off), nb=D(nb.nbytes, nb), sym=D(sym.nbytes, sym), idx=D(idx.nbytes, idx),
                         sof=D(c.span_off.nbytes, c.span_off), sp=D(c.spans.nbytes, c.spans), map=D(256, np.frombuffer(STAR, dtype=np.uint8)),
                         ws=D(self.wsb + guard, np.full(self.wsb + guard, 0xFF, dtype=np.uint8)))
        self.outs = dict(out=D(self.total + 64, np.full(self.total + 64, 0xA5, dtype=np.uint8)), oo=D((n + 1) * 8, np.full(n + 1, 7, dtype=np.uint64)),
                         onb=D(n * 8, np.full(n, 7, dtype=np.uint64)), oi=D(idx.nbytes, np.full(idx.size, 7, dtype=np.uint64)),
                         dr=D(n * 8, np.full(n, 7, dtype=np.uint64)), st=D(n * 4, np.full(n, 99, dtype=np.int32)))
        b, o = self.bufs, self.outs
        self.positional = [c.w.model[so].handle, c.d.model[do].handle, b["pay"].ptr, b["off"].ptr, b["nb"].ptr, n, int(off[n]), 0x20, b["sym"].ptr,
                           int(sym[n]), b["idx"].ptr, chunk, b["sof"].ptr, b["sp"].ptr, b["map"].ptr, o["out"].ptr, self.total, o["oo"].ptr,
                           o["onb"].ptr, o["oi"].ptr, o["dr"].ptr, o["st"].ptr, b["ws"].ptr, self.wsb, None]
        self.enc, self.chunk = enc, chunk

    def block(self, **change):
        blk = self.mhc.args_block(self.mhc.RecodeEditO2Args, *self.positional)
        for k, v in change.items():
            setattr(blk, k, v)
        return blk

    def untouched(self):
        o, n = self.outs, self.n
        return ((o["out"].download() == 0xA5).all() and (o["oo"].download(np.uint64) == 7).all() and (o["onb"].download(np.uint64) == 7).all()
                and (o["oi"].download(np.uint64) == 7).all() and (o["dr"].download(np.uint64) == 7).all() and (o["st"].download(np.int32) == 99).all())


@pytest.mark.parametrize("so,do", [(2, 2), (1, 2)])
def test_a_workspace_of_exactly_the_stated_size(mhc, cases, so, do):
    """Prefilled with 0xFF, a guard behind it that must come back untouched; one byte less is MH_ERR_CAPACITY before any launch."""
    c = cases[0x20]
    r = Raw(mhc, c, so, do, 256)
    assert r.lib.mh_dev_recode_edit_batch_o2(C.byref(r.block(ws_bytes=r.wsb - 1))) == mhc.MH_ERR_CAPACITY and r.untouched()
    assert r.lib.mh_dev_recode_edit_batch_o2(C.byref(r.block())) == mhc.MH_OK
    assert r.lib.mh_dev_status(r.bufs["ws"].ptr, None) == mhc.MH_OK
    ws = r.bufs["ws"].download()
    assert (ws[r.wsb:] == 0xFF).all(), "bytes written behind the stated workspace"
    assert np.array_equal(r.outs["out"].download()[:r.total], r.enc[0]) and np.array_equal(r.outs["oo"].download(np.uint64), r.enc[1])
    assert not r.outs["st"].download(np.int32).any()


def test_refusals_come_before_any_launch(mhc, cases):
    c = cases[0x20]
    r = Raw(mhc, c, 2, 2, 256)
    call = r.lib.mh_dev_recode_edit_batch_o2
    m = c.w.model
    size = C.sizeof(mhc.RecodeEditO2Args)
    for what, blk in [("order 1 -> 1", r.block(src=m[1].handle.value, dst=m[1].handle.value)),
                      ("order 0 -> 1", r.block(src=m[0].handle.value, dst=m[1].handle.value)),
                      ("struct_size one less", r.block(struct_size=size - 1)), ("struct_size eight more", r.block(struct_size=size + 8)),
                      ("struct_size 0", r.block(struct_size=0)), ("NULL map", r.block(d_map=None)), ("NULL src", r.block(src=None)),
                      ("NULL dst", r.block(dst=None)), ("NULL out_off", r.block(d_out_off=None))]:
        assert call(C.byref(blk)) == mhc.MH_ERR_ARG, what
        assert r.untouched(), what
    assert call(None) == mhc.MH_ERR_ARG and r.untouched()
    # the order-0/1 calls keep refusing order 2, and an order-0/1 pair keeps working through them
    with pytest.raises(mhc.MhError):
        src, kw = c.w.kw(2, 256, True)
        m[2].dev_recode_edit_batch(m[2], *src, STAR, c.span_off, c.spans, **kw)


# ---- 7. the host forms ------------------------------------------------------------------------------------------------------------

def host_check(mhc, got, enc, chunk, tag, index=True):
    """A host form's dict against the encoder's output: every array, the index slices by the source's lengths, no drops."""
    e_pay, e_off, e_nb, e_idx, e_so = enc
    assert got["rc"] == mhc.MH_OK and not got["status"].any(), (tag, got["rc"], got["status"])
    assert np.array_equal(got["out_off"], e_off) and np.array_equal(got["nbits"], e_nb) and np.array_equal(got["sym_off"], e_so), tag
    assert np.array_equal(got["payload"], e_pay) and not got["dropped"].any(), tag
    if index:
        assert np.array_equal(slices(got["index"], e_so, chunk), slices(e_idx, e_so, chunk)), tag
    else:
        assert got["index"] is None, tag


@pytest.mark.parametrize("so,do", [(2, 2), (1, 2), (2, 1)])
def test_the_host_form_equals_the_encoder(mhc, cases, so, do):
    """mh_recode_edit_batch_o2 through Model.recode_edit_batch_o2, indexed and index-free, searched spans and the NULL list."""
    c = cases[0x65]
    for chunk, indexed in SHAPES:
        (pay, off, nb), kw = c.w.kw(so, chunk, indexed)
        for what in ("mask", "fold all"):
            byte_map, span_off, spans = c.edits[what]
            got = c.w.model[so].recode_edit_batch_o2(c.d.model[do], pay, off, nb, byte_map, span_off=span_off, spans=spans, **kw)
            host_check(mhc, got, c.expect(what, do, chunk), chunk, (so, do, chunk, indexed, what))
        got = c.w.model[so].recode_edit_batch_o2(c.d.model[do], pay, off, nb, STAR, span_off=c.span_off, spans=c.spans, want_index=False, **kw)
        host_check(mhc, got, c.expect("mask", do, chunk), chunk, (so, do, chunk, indexed, "no index"), index=False)


def skewed_model(mhc, order):
    """The same Zipf(1.1) counts in every context: every pair and triple has a code, of 3 to 13 bits, and the codes
    re-synchronise (no lattice); uniform bytes cost about 9 bits each under it."""
    row = (np.floor((1 << 20) / np.arange(1, 257) ** 1.1) + 1).astype(np.uint64)
    return mhc.Model.from_counts(np.tile(row, 256 ** order), order)


@pytest.fixture(scope="module")
def over_cap(mhc):
    """Three streams, the second over MH_BATCH_WALK_MAX_BITS under the skewed models of order 1 and 2, and those models."""
    long_msg = np.random.default_rng(61).integers(0, 256, 1_000_000 + 77, dtype=np.uint8).tobytes()
    msgs = [b"a few bytes", long_msg, b""]
    model = {o: skewed_model(mhc, o) for o in (1, 2)}
    coded = {o: (model[o].encode_batch_o2 if o == 2 else model[o].encode_batch)(msgs, chunk_symbols=256) for o in (1, 2)}
    for o in (1, 2):
        assert int(coded[o][2][1]) > mhc.BATCH_WALK_MAX_BITS, o
    return msgs, model, coded


@pytest.mark.parametrize("so,do", [(2, 2), (1, 2), (2, 1)])
def test_the_host_form_indexes_a_batch_with_a_stream_over_the_walk_cap_first(mhc, over_cap, so, do):
    """Index-free, one stream over MH_BATCH_WALK_MAX_BITS: the device call refuses that stream alone, the host form indexes the
    batch first (mh_index_batch_o2 for the order-2 source, mh_index_batch for the order-1 source) and never refuses it.  A span
    in the long stream across a chunk boundary, one in the first stream."""
    msgs, model, coded = over_cap
    pay, off, nb, _, sym = coded[so]
    span_off, spans = span_lists([[(2, 5)], [(700_150, 700_420)], []])
    edited = edit_ref.apply(msgs, span_off, spans, STAR)
    dst = model[do]
    enc = (dst.encode_batch_o2 if do == 2 else dst.encode_batch)(edited, chunk_symbols=256)
    for want_index in (True, False):
        got = model[so].recode_edit_batch_o2(dst, pay, off, nb, STAR, span_off=span_off, spans=spans, chunk_symbols=256, want_index=want_index,
                                             check=False)
        host_check(mhc, got, enc, 256, (so, do, want_index), index=want_index)
    dev = model[so].dev_recode_edit_batch_o2(dst, pay, off, nb, STAR, span_off, spans, chunk_symbols=256, count_only=True, want_index=False)
    assert dev["status"].tolist() == [mhc.MH_OK, mhc.MH_ERR_ARG, mhc.MH_OK]


def test_the_host_forms_check_their_arguments_with_an_order_2_side(mhc):
    """The argument checks of the two host forms that need an order-2 model, which lives on a device alone (the checks with
    order-0/1 models are in tests/test_edit_o2_abi.py): each is MH_ERR_ARG, and the same arguments without the fault pass."""
    from test_edit_o2_abi import _host_edit, _host_splice
    ARG = mhc.MH_ERR_ARG
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    m2, m1, m0 = (mhc.Model.from_counts(np.ones(256 ** (o + 1), dtype=np.uint64), o) for o in (2, 1, 0))
    assert _host_splice(mhc, m1, m2) == ARG and _host_splice(mhc, m0, m2) == ARG                # left out: order 0/1 -> order 2
    assert _host_edit(mhc, m1, m0) == ARG and _host_edit(mhc, m0, m1) == ARG                    # order 0/1 on both sides
    for kw in (dict(map=None), dict(pay_off=None), dict(nbits=None), dict(out_off=None), dict(out_nbits=None), dict(sym_off=None),
               dict(spans=None), dict(span_off=u64(1, 1, 1)), dict(span_off=u64(0, 1, 0)), dict(chunk=100), dict(chunk=0)):
        assert _host_edit(mhc, m2, m1, **kw) == ARG and _host_edit(mhc, m1, m2, **kw) == ARG and _host_edit(mhc, m2, m2, **kw) == ARG, kw
    for kw in (dict(span_off=None), dict(span_tag=None), dict(rep_off=None), dict(rep_bytes=None), dict(out_sym_off=None), dict(spans=None),
               dict(rep_off=u64(1, 1, 3)), dict(rep_off=u64(0, 3, 2)), dict(rep_off=u64(0, 0, 256), rep_bytes=np.zeros(256, dtype=np.uint8)),
               dict(rep_off=u64(0), n_reps=0), dict(chunk=300), dict(span_off=u64(0, 1, 0))):
        assert _host_splice(mhc, m2, m1, **kw) == ARG and _host_splice(mhc, m2, m2, **kw) == ARG and _host_splice(mhc, m2, m0, **kw) == ARG, kw
    # the same arguments without a fault get through the checks: the zero payloads decode or are corrupt, never MH_ERR_ARG
    for s, d in [(m2, m2), (m2, m1), (m1, m2)]:
        assert _host_edit(mhc, s, d) in (mhc.MH_OK, mhc.MH_ERR_CORRUPT), (s.type, d.type)
    for d in (m2, m1, m0):
        assert _host_splice(mhc, m2, d) in (mhc.MH_OK, mhc.MH_ERR_CORRUPT), d.type
