"""The batch calls of include/mh.h on offsets and positions beyond 2^32 (run with -m gpu on an MI355X; about 30 GiB of device
memory).  One batch of tests/far_ref.py at its full size: a filler stream F of more than 2^32 symbols, payload bits and payload
bytes, a stream G and about 30 small streams wholly behind it, so every in_off, pay_off, sym_off, out_off, chunk number, hit
record and lookup position of the far streams needs its upper 32 bits.  The expected values are far_ref's closed forms (the CPU
oracle's code tables and batch_ref.pack on one period; tests/test_far_ref.py proves them on the real concatenation at small
sizes), materialised here with torch; never another call of the library.

The batch is built once on the device.  The calls go through mhc.lib() with data_ptr(): the binding's dev_* helpers upload and
download whole batches.  Workspaces and outputs are pre-filled with 0xA5, the gaps of an index buffer with a sentinel that
must survive.  Chunk 1024 for the encoders and the re-code, 256 for decode, lookups, search and digests.  The readers read the
reference's payload and index, not the encoder's output.  Every comparison is exact.

Index-free, the device calls refuse F alone (MH_ERR_ARG: it is over MH_BATCH_WALK_MAX_BITS) and must serve every other
stream, G and the far small streams included: far_ref.Far.without_f() is that expectation.

The per-stream-model calls (mh_dev_*_each) read the same batch with stream i under entry choice[i] of the bank [S, D],
through a mh_dev_model_set_pick view: F and G under S, the small streams in turn under S and D.

Segment states: F is refused (MH_ERR_ARG), as mh.h says of a stream whose unsettled segments lie further apart than
MH_BATCH_WALK_MAX_BITS.  S is close to a lattice: the block is near-uniform, so most of its codes have 7 to 9
bits, and a decoder that starts off the true path drifts back slowly.  Replayed on the CPU from far_ref's tables, the guessed
entries of csrc/mh_batch_states.hip (256 bits of warm-up) were wrong for 98 % of the first 69 000 segments of F, and from a
wrong entry the median distance to the true path was 8 758 bits; the eight repair launches settle 8 x 512.  Unsettled
segments therefore remain all along F, the one-lane walk between the first and the last of them is over the cap, and F
decodes to no symbol.  G (6.2 Mbit, under the cap) and every small stream are walked or settled and must be exact.

Not covered here: the host forms (they stage through host memory, and their offset arithmetic is host C++), damage (the
damage matrices own that) and the order-2 forms of re-coding and dictionary search."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
import edit_ref
import far_ref

pytestmark = pytest.mark.gpu

FAR, PREV0 = far_ref.FAR, far_ref.PREV0
MAIN, FINE = far_ref.CHUNKS
FILL = 0xA5
SENTINEL = np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0]
GUARD = 64


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


class Source:
    """One reference form of the batch on the device: payload (GUARD bytes of padding behind it), pay_off, nbits, sym_off, the
    index of one chunk size (SENTINEL in the gaps) and the closed form `ref` they come from."""


class Rig:
    def __init__(self, mhc, torch, f):
        self.mhc, self.torch, self.lib = mhc, torch, mhc.lib()
        self.dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        self.far, self.free = f, f.without_f()
        self.n, self.total = f.n, f.total
        self.models = {k: mhc.Model.from_counts(f.counts[k], f.orders[k]) for k in f.codes}
        if "D" in self.models:
            self.S, self.D = self.models["S"], self.models["D"]
            self.bank = mhc.ModelSet.from_models([self.S, self.D])
            self.models["mix"] = self.view = self.bank.pick(f.choice())
        self.data = self.tile(f.data_parts())
        self.in_off = self.u64(f.sym_off)
        self.sources = {}

    # ---- tensors ----
    def tile(self, parts, pad=GUARD):
        t = self.torch
        pieces = [t.from_numpy(np.array(a)).to(self.dev).repeat(k) for a, k in parts]
        return t.cat(pieces + [t.zeros(pad, dtype=t.uint8, device=self.dev)])

    def u64(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(self.dev)

    def host(self, t, dtype=np.uint64):
        return t.cpu().numpy().view(dtype)

    def fill(self, nbytes):
        return self.torch.full((max(int(nbytes), 256),), FILL, dtype=self.torch.uint8, device=self.dev)

    def words(self, n):
        return self.torch.full((max(int(n), 1),), int(SENTINEL), dtype=self.torch.int64, device=self.dev)

    def ints(self, n):
        return self.torch.full((max(int(n), 1),), 99, dtype=self.torch.int32, device=self.dev)

    def index(self, ref):
        """ref.index_array(SENTINEL) on the device, GUARD sentinels behind it."""
        t = self.torch
        idx = self.words(ref.index_entries + GUARD)
        for at, a, k, step in ref.index_parts:
            rows = self.u64(a)[None, :] + (t.arange(k, dtype=t.int64, device=self.dev) * int(step))[:, None]
            idx[at:at + a.size * k] = rows.reshape(-1)
        return idx

    def source(self, model, chunk, far=None, keep=True):
        """The reference form of `far` (default: the batch) under 'S', 'D' or 'mix' (the bank view's choice) with the index of
        `chunk`; forms of one batch under one model share their payload.  keep=False: not remembered (the caller drops it)."""
        f = far or self.far
        key = (model, chunk, id(f))
        if key in self.sources:
            return self.sources[key]
        s, ref = Source(), f.mix(f.choice(), chunk) if model == "mix" else f.pack(model, chunk)
        same = [v for k, v in self.sources.items() if k[0] == model and k[2] == id(f)]
        s.far, s.ref, s.chunk, s.pay_total, s.sym_total = f, ref, chunk, int(ref.pay_off[-1]), f.total
        s.payload = same[0].payload if same else self.tile(ref.payload_parts)
        s.pay_off, s.nbits, s.sym_off = self.u64(ref.pay_off), self.u64(ref.nbits), self.u64(ref.sym_off)
        s.index = self.index(ref)
        if keep:
            self.sources[key] = s
        return s

    def status(self, ws):
        return self.lib.mh_dev_status(ws.data_ptr(), None)

    def batch(self, s):
        """The arguments that every reader takes behind its handles: payload .. prev0."""
        return (s.payload.data_ptr(), s.pay_off.data_ptr(), s.nbits.data_ptr(), self.n, s.pay_total, PREV0)

    def refused(self, st, rc):
        """Index-free verdicts: F alone is MH_ERR_ARG."""
        want = np.zeros(self.n, dtype=np.int32)
        want[self.far.f] = self.mhc.MH_ERR_ARG
        assert rc == self.mhc.MH_ERR_ARG and np.array_equal(self.host(st, np.int32)[:self.n], want)


@pytest.fixture(scope="module")
def rig(mhc):
    import torch
    r = Rig(mhc, torch, far_ref.far(None))
    yield r
    r.sources.clear()
    del r.data
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def rig2(mhc):
    """The order-2 batch (far_ref.Far2) under its one model S2."""
    import torch
    r = Rig(mhc, torch, far_ref.far2(None))
    yield r
    r.sources.clear()
    del r.data
    torch.cuda.empty_cache()


def p(t):
    return None if t is None else t.data_ptr()


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------------------- the preconditions
def test_the_batch_lies_beyond_2_pow_32(rig):
    """Read from the references that the tests below use: F's symbols, payload bits and payload bytes beyond 2^32, G and 30
    streams wholly beyond all three, chunk numbers in the millions, hit records and lookups beyond 2^32."""
    f = rig.far
    assert f.lengths[f.f] >= FAR + (1 << 26) and int(f.sym_off[f.g]) > FAR and f.n - f.g - 1 >= 30
    for key in (("S", MAIN), ("D", MAIN), ("S", FINE)):
        ref = rig.source(*key).ref
        assert int(ref.nbits[f.f]) > 8 * FAR and int(ref.pay_off[f.f + 1] - ref.pay_off[f.f]) > FAR and int(ref.pay_off[f.g]) > FAR
    assert int(f.sym_off[f.g]) // FINE + f.g > (1 << 24)
    assert int(rig.source("S", FINE).ref.nbits[f.g]) <= far_ref.WALK_MAX_BITS
    off, rec, pat = f.hits()
    assert int(((rec[:, 0] == f.f) & (rec[:, 1] > FAR)).sum()) >= far_ref.FAR_HITS and int((rec[:, 0] > f.g).sum()) >= 3
    assert sum(1 for i, b, e in f.lookups() if i == f.f and b > FAR) >= 4 and f.marks()["symbol"] == FAR
    assert rig.data.numel() == f.total + GUARD and int(rig.data[f.total - 1]) == f.read(f.n - 2, f.lengths[-2] - 1, f.lengths[-2])[0]


# ------------------------------------------------------------------------------------------------------- encode and training
@pytest.mark.parametrize("model", ["S", "D"])
def test_encode_batch(rig, model):
    check_encode(rig, model, "mh_dev_encode_batch")


def check_encode(rig, model, name):
    s, lib, n = rig.source(model, MAIN), rig.lib, rig.n
    m = rig.models[model]
    out, out_off, nbits, index = rig.fill(s.pay_total + GUARD), rig.words(n + 1 + 8), rig.words(n + 8), rig.words(s.index.numel())
    wsb = getattr(lib, name + "_workspace")(n, rig.total)
    ws = rig.fill(wsb)
    assert getattr(lib, name)(m.handle, p(rig.data), p(rig.in_off), n, rig.total, PREV0, p(out), s.pay_total, p(out_off), p(nbits),
                                   p(index), MAIN, p(ws), wsb, None) == 0
    assert rig.status(ws) == 0
    oo, nb = rig.host(out_off), rig.host(nbits)
    assert same(oo[:n + 1], s.ref.pay_off) and same(nb[:n], s.ref.nbits) and (oo[n + 1:] == SENTINEL.view(np.uint64)).all()
    assert (nb[n:] == SENTINEL.view(np.uint64)).all()
    assert rig.torch.equal(out[:s.pay_total], s.payload[:s.pay_total]), "payload"
    assert bool((out[s.pay_total:] == FILL).all()), "bytes written at or beyond cap"
    assert rig.torch.equal(index, s.index), "index slices, or a gap entry written"


def test_training_histograms(rig):
    lib, n, f = rig.lib, rig.n, rig.far
    for order, nc in ((0, 256), (1, 65536), (2, 1 << 24)):
        counts = rig.words(nc + 8)
        if order == 2:
            wsb = lib.mh_dev_histogram_o2_batch_workspace(rig.total)
            ws = rig.fill(wsb)
            rc = lib.mh_dev_histogram_o2_batch(p(rig.data), p(rig.in_off), n, rig.total, PREV0, p(counts), p(ws), wsb, None)
        else:
            wsb = lib.mh_dev_histogram_batch_workspace(rig.total)
            ws = rig.fill(wsb)
            rc = lib.mh_dev_histogram_o1_batch(p(rig.data), p(rig.in_off), n, rig.total, PREV0, p(counts), p(ws), wsb, None) if order else \
                lib.mh_dev_histogram_o0_batch(p(rig.data), p(rig.in_off), n, rig.total, p(counts), p(ws), wsb, None)
        assert rc == 0 and rig.status(ws) == 0, order
        got = rig.host(counts)
        assert same(got[:nc], f.histogram(order)) and (got[nc:] == SENTINEL.view(np.uint64)).all(), "order %d" % order


def test_bank_select(rig):
    lib, n = rig.lib, rig.n
    bank = rig.bank
    choice, nbits = rig.ints(n + 8), rig.words(n + 8)
    wsb = lib.mh_dev_bank_select_workspace(2, n, rig.total)
    ws = rig.fill(wsb)
    assert lib.mh_dev_bank_select(bank.handle, p(rig.data), p(rig.in_off), n, rig.total, PREV0, p(choice), p(nbits), p(ws), wsb, None) == 0
    assert rig.status(ws) == 0
    want_c, want_n = rig.far.select()
    assert same(rig.host(choice, np.uint32)[:n], want_c) and same(rig.host(nbits)[:n], want_n)
    assert int(want_n[rig.far.f]) > 8 * FAR


# ------------------------------------------------------------------------------------------------------- decode
def kind(rig, name):
    """(the source form, the call, its handle) of a reader family under the shared model S or under the view of the bank."""
    each = name.endswith("_each") or name.endswith("each_ranges")
    model = "S2" if "_o2" in name else "mix" if each else "S"
    return rig.source(model, FINE), getattr(rig.lib, name), rig.models[model].handle


@pytest.mark.parametrize("name", ["mh_dev_decode_batch", "mh_dev_decode_each"])
def test_decode_indexed(rig, name):
    check_decode_indexed(rig, name)


def check_decode_indexed(rig, name):
    (s, fn, h), lib, n = kind(rig, name), rig.lib, rig.n
    out, st, so = rig.fill(rig.total + GUARD), rig.ints(n), s.sym_off.clone()
    wsb = getattr(lib, name + "_workspace")(n)
    ws = rig.fill(wsb)
    assert fn(h, *rig.batch(s), p(out), rig.total, p(so), rig.total, p(s.index), FINE, p(st), p(ws), wsb, None) == 0
    assert rig.status(ws) == 0 and not rig.host(st, np.int32)[:n].any()
    assert rig.torch.equal(out[:rig.total], rig.data[:rig.total]) and bool((out[rig.total:] == FILL).all())
    assert rig.torch.equal(so, s.sym_off)


@pytest.mark.parametrize("name", ["mh_dev_decode_batch", "mh_dev_decode_each"])
def test_decode_index_free(rig, name):
    """F is refused (MH_ERR_ARG) and takes no symbol in d_sym_off; every other stream, G included, decodes to its bytes."""
    (s, fn, h), lib, n, f = kind(rig, name), rig.lib, rig.n, rig.far
    cap = rig.free.total
    out, st, so = rig.fill(cap + GUARD), rig.ints(n), rig.words(n + 1 + 8)
    wsb = (lib.mh_dev_decode_each_workspace if "each" in name else lib.mh_dev_decode_batch_workspace)(n)
    ws = rig.fill(wsb)
    assert fn(h, *rig.batch(s), p(out), cap, p(so), 0, None, 0, p(st), p(ws), wsb, None) == 0
    rig.refused(st, rig.status(ws))
    got = rig.host(so)
    assert same(got[:n + 1], rig.free.sym_off) and (got[n + 1:] == SENTINEL.view(np.uint64)).all()
    a, b = int(f.sym_off[f.f]), int(f.sym_off[f.f + 1])
    assert rig.torch.equal(out[:a], rig.data[:a]) and rig.torch.equal(out[a:cap], rig.data[b:rig.total])
    assert bool((out[cap:] == FILL).all())


# ------------------------------------------------------------------------------------------------------- segment states
def test_segment_states(rig):
    """mh_dev_batch_states, mh_dev_batch_index, mh_dev_batch_emit and mh_dev_batch_states_stats on the index-free batch: F is
    refused (the module's docstring says why) and takes no symbol; for every other stream the built index is the reference's
    and the emitted bytes are the input."""
    s, w, lib, n, f = rig.source("S", FINE), rig.source("S", FINE, rig.free, keep=False), rig.lib, rig.n, rig.far
    args = (rig.S.handle,) + rig.batch(s)
    wsb = lib.mh_dev_batch_states_workspace(n, s.pay_total)
    ws, so, st = rig.fill(wsb), rig.words(n + 1 + 8), rig.ints(n)
    assert lib.mh_dev_batch_states(*args, p(so), p(st), p(ws), wsb, None) == 0
    rig.refused(st, rig.status(ws))
    got = rig.host(so)
    assert same(got[:n + 1], w.ref.sym_off) and (got[n + 1:] == SENTINEL.view(np.uint64)).all()
    passes, walked = C.c_uint32(99), C.c_uint64(99)
    assert lib.mh_dev_batch_states_stats(p(ws), None, C.byref(passes), C.byref(walked)) == 0
    assert 2 <= walked.value <= n and passes.value <= 8                # F (until it is refused) and G at the least
    index, st = rig.words(w.index.numel()), rig.ints(n)
    assert lib.mh_dev_batch_index(*args, p(index), w.ref.index_entries, FINE, p(st), p(ws), wsb, None) == 0
    rig.refused(st, rig.status(ws))
    assert rig.torch.equal(index, w.index), "index slices, or a gap entry written"
    cap = rig.free.total
    out, st = rig.fill(cap + GUARD), rig.ints(n)
    assert lib.mh_dev_batch_emit(*args, p(out), cap, p(st), p(ws), wsb, None) == 0
    rig.refused(st, rig.status(ws))
    a, b = int(f.sym_off[f.f]), int(f.sym_off[f.f + 1])
    assert rig.torch.equal(out[:a], rig.data[:a]) and rig.torch.equal(out[a:cap], rig.data[b:rig.total])
    assert bool((out[cap:] == FILL).all())


# ------------------------------------------------------------------------------------------------------- lookups
def run_lookups(rig, name, lookups, indexed):
    """One mh_dev_decode_batch_ranges / _each_ranges call with GUARD bytes of FILL around every output: ([bytes per lookup],
    status[m], rc)."""
    (s, fn, h), lib, m = kind(rig, name), rig.lib, len(lookups)
    lk = np.array(lookups, dtype=np.uint64).reshape(-1, 3)
    ln = (lk[:, 2] - lk[:, 1]).astype(np.int64)
    at = GUARD + np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(ln[:-1] + GUARD)])
    size = int(at[-1] + ln[-1]) + GUARD
    out, st = rig.fill(size), rig.ints(m)
    wsb = (lib.mh_dev_decode_batch_o2_ranges_workspace if "_o2" in name else lib.mh_dev_decode_batch_ranges_workspace)(m)
    ws = rig.fill(wsb)
    d_lk, d_at = rig.u64(lk), rig.u64(at)
    assert fn(h, p(s.payload), p(s.pay_off), p(s.nbits), rig.n, PREV0, p(s.sym_off), p(s.index) if indexed else None,
              s.chunk if indexed else 0, p(d_lk), m, p(out), p(d_at), size, p(st), p(ws), wsb, None) == 0
    rc = rig.status(ws)
    got = rig.host(out, np.uint8)[:size]
    mine = np.zeros(size, dtype=bool)
    for j in range(m):
        mine[int(at[j]):int(at[j]) + int(ln[j])] = True
    assert (got[~mine] == FILL).all(), "bytes written outside the outputs"
    return [got[int(at[j]):int(at[j]) + int(ln[j])].tobytes() for j in range(m)], rig.host(st, np.int32)[:m], rc


@pytest.mark.parametrize("name", ["mh_dev_decode_batch_ranges", "mh_dev_decode_each_ranges"])
def test_lookups(rig, name):
    check_lookups(rig, name)


def check_lookups(rig, name):
    f = rig.far
    lk, want = f.lookups(), f.lookup_bytes()
    got, st, rc = run_lookups(rig, name, lk, True)
    assert rc == 0 and not st.any() and got == want
    outside = [j for j, (i, _, _) in enumerate(lk) if i != f.f]
    got, st, rc = run_lookups(rig, name, [lk[j] for j in outside], False)
    assert rc == 0 and not st.any() and got == [want[j] for j in outside]


# ------------------------------------------------------------------------------------------------------- search
FINDERS = ["mh_dev_find_batch", "mh_dev_find_each", "mh_dev_find_dict_batch", "mh_dev_find_dict_each"]


def run_find(rig, name, indexed, cap, records=True):
    """One call of a search family: (hit_off[n + 1], records[cap + 8, 3] or None, pattern[cap + 8] or None, status tensor, rc)."""
    (s, fn, h), lib, n = kind(rig, name), rig.lib, rig.n
    ps = (rig.mhc.Dict if "dict" in name else rig.mhc.PatternSet)(rig.far.patterns)
    ho, st = rig.words(n + 1 + 8), rig.ints(n)
    hits = rig.words(3 * (cap + 8)) if records else None
    pat = rig.torch.full((cap + 8,), 0x5A5A5A5A, dtype=rig.torch.int32, device=rig.dev) if records else None
    ws_fn = lib.mh_dev_find_dict_workspace if "dict" in name else lib.mh_dev_find_batch_o2_workspace if "_o2" in name else \
        lib.mh_dev_find_batch_workspace
    wsb = ws_fn(n, s.sym_total if indexed else 0, s.chunk if indexed else 0)
    ws = rig.fill(wsb)
    assert fn(h, ps.handle, *rig.batch(s), p(s.sym_off) if indexed else None, s.sym_total if indexed else 0, p(s.index) if indexed else None,
              s.chunk if indexed else 0, p(ho), p(hits), p(pat), cap, p(st), p(ws), wsb, None) == 0
    rc = rig.status(ws)
    got = rig.host(ho)
    assert (got[n + 1:] == SENTINEL.view(np.uint64)).all(), "words written behind hit_off"
    return (got[:n + 1], rig.host(hits).reshape(-1, 3) if records else None, rig.host(pat, np.uint32) if records else None, st, rc)


def check_records(rec, pat, w_rec, w_pat, k):
    assert same(rec[:k], w_rec[:k]) and same(pat[:k], w_pat[:k]), "records"
    assert (rec[k:] == SENTINEL.view(np.uint64)).all() and (pat[k:] == 0x5A5A5A5A).all(), "records written at or beyond the hits / hit_cap"


@pytest.mark.parametrize("name", FINDERS)
def test_find_indexed(rig, name):
    check_find_indexed(rig, name)


def check_find_indexed(rig, name):
    f, n = rig.far, rig.n
    w_off, w_rec, w_pat = f.hits()
    k = int(w_off[n])
    ho, _, _, st, rc = run_find(rig, name, True, 0, records=False)
    assert rc == 0 and not rig.host(st, np.int32)[:n].any() and same(ho, w_off), "count only"
    ho, rec, pat, st, rc = run_find(rig, name, True, k)
    assert rc == 0 and not rig.host(st, np.int32)[:n].any() and same(ho, w_off)
    check_records(rec, pat, w_rec, w_pat, k)
    ho, rec, pat, st, rc = run_find(rig, name, True, k - 1)
    assert rc == rig.mhc.MH_ERR_CAPACITY and not rig.host(st, np.int32)[:n].any() and same(ho, w_off), "hit_cap"
    check_records(rec, pat, w_rec, w_pat, k - 1)


@pytest.mark.parametrize("name", FINDERS)
def test_find_index_free(rig, name):
    check_find_index_free(rig, name)


def check_find_index_free(rig, name):
    n = rig.n
    w_off, w_rec, w_pat = rig.free.hits()
    k = int(w_off[n])
    assert k >= 6 and int(w_rec[-1, 0]) > rig.far.g
    ho, rec, pat, st, rc = run_find(rig, name, False, k)
    rig.refused(st, rc)
    assert same(ho, w_off)
    check_records(rec, pat, w_rec, w_pat, k)


def test_spans_from_hits_and_hit_records_as_lookups(rig):
    """The reference's records, far ones included, through mh_dev_spans_from_hits; and records with begin > 2^32 fed back as
    lookups give the pattern's bytes."""
    f, lib, n = rig.far, rig.lib, rig.n
    w_off, w_rec, w_pat = f.hits()
    k = int(w_off[n])
    want_off, want = edit_ref.merge_hits(w_off, w_rec)
    d_ho, d_rec = rig.u64(w_off), rig.u64(w_rec.reshape(-1))
    so, sp = rig.words(n + 1 + 8), rig.words(2 * k + 8)
    wsb = lib.mh_dev_spans_from_hits_workspace(n, k)
    ws = rig.fill(wsb)
    assert lib.mh_dev_spans_from_hits(p(d_ho), p(d_rec), k, n, p(so), p(sp), p(ws), wsb, None) == 0
    assert rig.status(ws) == 0
    got_off, got = rig.host(so), rig.host(sp)
    m = int(want_off[n])
    assert same(got_off[:n + 1], want_off) and same(got[:2 * m].reshape(-1, 2), want)
    assert (got_off[n + 1:] == SENTINEL.view(np.uint64)).all() and (got[2 * m:] == SENTINEL.view(np.uint64)).all()
    assert int((np.asarray(want)[:, 0] > FAR).sum()) >= far_ref.FAR_HITS
    far_hits = np.flatnonzero((w_rec[:, 0] == f.f) & (w_rec[:, 1] > FAR))
    pick = far_hits[np.unique(np.linspace(0, far_hits.size - 1, 256).astype(np.int64))]
    pick = np.concatenate([pick, far_hits[-6:], np.flatnonzero(w_rec[:, 0] > f.g)])
    for name in ("mh_dev_decode_batch_ranges", "mh_dev_decode_each_ranges"):
        res, st, rc = run_lookups(rig, name, w_rec[pick].tolist(), True)
        assert rc == 0 and not st.any() and res == [f.patterns[int(j)] for j in w_pat[pick]], name


# ------------------------------------------------------------------------------------------------------- digests, coded histograms
@pytest.mark.parametrize("name", ["mh_dev_crc_batch", "mh_dev_crc_each"])
def test_crc(rig, name):
    check_crc(rig, name)


def check_crc(rig, name):
    (s, fn, h), lib, n = kind(rig, name), rig.lib, rig.n
    for indexed in (True, False):
        crc, ln, st = rig.ints(n + 8), rig.words(n + 8), rig.ints(n)
        wsb = lib.mh_dev_crc_batch_workspace(n, s.sym_total if indexed else 0, s.chunk if indexed else 0)
        ws = rig.fill(wsb)
        assert fn(h, *rig.batch(s), p(s.sym_off) if indexed else None, s.sym_total if indexed else 0, p(s.index) if indexed else None,
                  s.chunk if indexed else 0, p(crc), p(ln), p(st), p(ws), wsb, None) == 0
        rc = rig.status(ws)
        got_c, got_l = rig.host(crc, np.uint32), rig.host(ln)
        assert (got_c[n:] == 99).all() and (got_l[n:] == SENTINEL.view(np.uint64)).all(), "words written behind crc / len"
        if indexed:
            assert rc == 0 and not rig.host(st, np.int32)[:n].any()
        else:
            rig.refused(st, rc)
        w_crc, w_len = (rig.far if indexed else rig.free).crcs()
        assert same(got_c[:n], w_crc) and same(got_l[:n], w_len), "indexed=%s" % indexed


def test_crc_raw_batch(rig):
    lib, n = rig.lib, rig.n
    crc = rig.ints(n + 8)
    wsb = lib.mh_dev_crc_raw_batch_workspace(n, rig.total)
    ws = rig.fill(wsb)
    assert lib.mh_dev_crc_raw_batch(p(rig.data), p(rig.in_off), n, rig.total, p(crc), p(ws), wsb, None) == 0
    assert rig.status(ws) == 0
    got = rig.host(crc, np.uint32)
    assert same(got[:n], rig.far.crcs()[0]) and (got[n:] == 99).all()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", ["mh_dev_histogram_coded_batch", "mh_dev_histogram_coded_each"])
def test_histogram_coded(rig, name, order):
    check_histogram_coded(rig, name, order)


def check_histogram_coded(rig, name, order):
    (s, fn, h), lib, n = kind(rig, name), rig.lib, rig.n
    nc = {0: 256, 1: 65536, 2: 1 << 24}[order]
    ws_fn = lib.mh_dev_histogram_coded_batch_o2_workspace if "_o2" in name else lib.mh_dev_histogram_coded_workspace
    for indexed in (True, False):
        counts, st = rig.words(nc + 8), rig.ints(n)
        wsb = ws_fn(n, s.sym_total if indexed else 0, s.chunk if indexed else 0)
        ws = rig.fill(wsb)
        assert fn(h, order, *rig.batch(s), p(s.sym_off) if indexed else None, s.sym_total if indexed else 0, p(s.index) if indexed else None,
                  s.chunk if indexed else 0, p(counts), p(st), p(ws), wsb, None) == 0
        rc = rig.status(ws)
        if indexed:
            assert rc == 0 and not rig.host(st, np.int32)[:n].any()
        else:
            rig.refused(st, rc)
        got = rig.host(counts)
        assert same(got[:nc], (rig.far if indexed else rig.free).histogram(order)), "indexed=%s" % indexed
        assert (got[nc:] == SENTINEL.view(np.uint64)).all()


# ------------------------------------------------------------------------------------------------------- re-coding S -> D
def run_recode(rig, name, indexed, full, edit=None):
    """One call of a re-coding family into D, chunk MAIN.  edit: None (mh_dev_recode_*), "map" (mh_dev_recode_edit_*: the
    span list and byte map of far_ref) or a replacement (mh_dev_recode_splice_*).  Every output is compared with the closed
    form of the batch after the edit (index-free: of the batch without F); returns (status tensor, rc)."""
    each = name.endswith("_each")
    base = rig.far if indexed else rig.free
    after = base if edit is None else base.edited() if edit == "map" else base.spliced(edit)
    s, d = rig.source("mix" if each else "S", MAIN), rig.source("D", MAIN, after, keep=edit is None)
    fn, h, lib, n = getattr(rig.lib, name), rig.models["mix" if each else "S"].handle, rig.lib, rig.n
    cap = d.pay_total
    out = rig.fill(cap + GUARD) if full else None
    oo, onb, dr, st = rig.words(n + 1 + 8), rig.words(n + 8), rig.words(n + 8), rig.ints(n)
    oi = rig.words(d.index.numel())
    so = s.sym_off.clone() if indexed else rig.words(n + 1)
    sym_total = s.sym_total if indexed else d.sym_total
    head = (h, rig.D.handle) + rig.batch(s) + (p(so), sym_total, p(s.index) if indexed else None, MAIN)
    tail = (p(dr), p(st))
    if edit is None:
        wsb = lib.mh_dev_recode_batch_workspace(n, sym_total, MAIN if indexed else 0)
        ws = rig.fill(wsb)
        assert fn(*head, p(out), cap, p(oo), p(onb), p(oi), *tail, p(ws), wsb, None) == 0
    else:
        span_off, spans = rig.far.spans()
        d_off, d_sp = rig.u64(span_off), rig.u64(spans.reshape(-1))
        if edit == "map":
            d_map = rig.torch.from_numpy(np.frombuffer(rig.far.byte_map(), dtype=np.uint8).copy()).to(rig.dev)
            wsb = lib.mh_dev_recode_edit_workspace(n, sym_total, MAIN if indexed else 0)
            ws = rig.fill(wsb)
            assert fn(*head, p(d_off), p(d_sp), p(d_map), p(out), cap, p(oo), p(onb), p(oi), *tail, p(ws), wsb, None) == 0
        else:
            d_rep = rig.torch.from_numpy(np.frombuffer(edit + bytes(16), dtype=np.uint8).copy()).to(rig.dev)
            oso = rig.words(n + 1 + 8)
            wsb = lib.mh_dev_recode_splice_workspace(n, sym_total, MAIN if indexed else 0, spans.shape[0])
            ws = rig.fill(wsb)
            assert fn(*head, p(d_off), p(d_sp), p(d_rep) if edit else None, len(edit), p(out), cap, p(oo), p(onb), p(oso), p(oi),
                      d.ref.index_entries, *tail, p(ws), wsb, None) == 0
    rc = rig.status(ws)
    got_oo, got_nb, got_dr = rig.host(oo), rig.host(onb), rig.host(dr)
    sent = SENTINEL.view(np.uint64)
    assert (got_oo[n + 1:] == sent).all() and (got_nb[n:] == sent).all() and (got_dr[n:] == sent).all(), "words written behind an output"
    assert same(got_oo[:n + 1], d.ref.pay_off) and same(got_nb[:n], d.ref.nbits) and not got_dr[:n].any(), "offsets, nbits, dropped"
    assert same(rig.host(so)[:n + 1], base.sym_off), "sym_off"
    if edit not in (None, "map"):
        got = rig.host(oso)
        assert same(got[:n + 1], after.sym_off) and (got[n + 1:] == sent).all(), "out_sym_off"
    assert rig.torch.equal(oi, d.index), "index slices, or a gap entry written"
    if full:
        assert rig.torch.equal(out[:cap], d.payload[:cap]), "payload"
        assert bool((out[cap:] == FILL).all()), "bytes written at or beyond out_off[n]"
    return st, rc


def recode_all(rig, name, indexed, edit=None):
    """Count-only and in full (index-free: in full; F is refused there)."""
    for full in ((False, True) if indexed else (True,)):
        st, rc = run_recode(rig, name, indexed, full, edit)
        if indexed:
            assert rc == 0 and not rig.host(st, np.int32)[:rig.n].any(), "full=%s" % full
        else:
            rig.refused(st, rc)


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "index-free"])
@pytest.mark.parametrize("name", ["mh_dev_recode_batch", "mh_dev_recode_each"])
def test_recode(rig, name, indexed):
    """Index-free, F is refused: nbits 0, no payload byte, no symbol; the streams behind it move up in the payload and index."""
    recode_all(rig, name, indexed)


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "index-free"])
@pytest.mark.parametrize("name", ["mh_dev_recode_edit_batch", "mh_dev_recode_edit_each"])
def test_recode_edit(rig, name, indexed):
    """Spans beyond 2^32 of F (its tail) and in the far small streams; the edited F is blk x P + the edited tail."""
    off, sp = rig.far.spans()
    assert int((sp[int(off[rig.far.f]):int(off[rig.far.f + 1]), 0] > FAR).sum()) >= 5 and int(off[-1] - off[rig.far.g]) >= 5
    recode_all(rig, name, indexed, "map")


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "index-free"])
@pytest.mark.parametrize("rep", [0, 1], ids=["deletion", "replacement"])
@pytest.mark.parametrize("name", ["mh_dev_recode_splice_batch", "mh_dev_recode_splice_each"])
def test_recode_splice(rig, name, rep, indexed):
    """The tail's length changes, so out_sym_off and every offset behind F move."""
    rep = rig.far.reps()[rep]
    after = rig.far.spliced(rep)
    assert int(after.sym_off[rig.far.g]) != int(rig.far.sym_off[rig.far.g]) and int(after.sym_off[rig.far.g]) > FAR
    recode_all(rig, name, indexed, rep)


# ------------------------------------------------------------------------------------------------------- order 2
def test_o2_batch_lies_beyond_2_pow_32(rig2):
    f, ref = rig2.far, rig2.source("S2", FINE).ref
    assert f.lengths[f.f] >= FAR + (1 << 26) and int(ref.nbits[f.f]) > FAR and int(f.sym_off[f.g]) > FAR and int(ref.pay_off[f.g]) * 8 > FAR
    assert int(ref.nbits[f.g]) <= far_ref.WALK_MAX_BITS and f.n - f.g - 1 >= 30
    off, rec, pat = f.hits()
    assert int(((rec[:, 0] == f.f) & (rec[:, 1] > FAR)).sum()) >= far_ref.FAR_HITS
    assert rig2.data.numel() == f.total + GUARD


def test_o2_encode_batch(rig2):
    check_encode(rig2, "S2", "mh_dev_encode_batch_o2")


def test_o2_decode_batch_indexed(rig2):
    check_decode_indexed(rig2, "mh_dev_decode_batch_o2")


def test_o2_lookups(rig2):
    check_lookups(rig2, "mh_dev_decode_batch_o2_ranges")


def test_o2_find_batch(rig2):
    check_find_indexed(rig2, "mh_dev_find_batch_o2")
    check_find_index_free(rig2, "mh_dev_find_batch_o2")


def test_o2_crc_batch(rig2):
    check_crc(rig2, "mh_dev_crc_batch_o2")


def test_o2_histogram_coded_batch(rig2):
    check_histogram_coded(rig2, "mh_dev_histogram_coded_batch_o2", 2)
