"""The device calls on a non-default stream: include/mh.h promises that every mh_dev_* call is stream-ordered and neither
allocates nor synchronises, and every other GPU test passes NULL as the stream, where everything serialises whatever a call does.

Here chains of device calls are driven with ctypes on torch tensors, all on one torch.cuda.Stream() (which does not wait for the
null stream), enqueued back to back without a host wait; one stream synchronisation ends a chain.  Every later call of a chain
reads what an earlier one wrote on the device.  All host-side sizes (totals, capacities, the hit capacity) come from the
references of tests/batch_ref.py, never from the device, and the models are built beforehand.  Each chain runs twice:

  first run    no blocker; compared like the second, and its host time to enqueue gives the blocker's length;
  second run   every buffer is prefilled and synchronised (offsets, lengths, lookups and index arrays with zeros, so that a
               premature read stays in bounds; every byte buffer - inputs, payloads, outputs, statuses, workspaces - with 0xA5),
               then the stream gets a torch.cuda._sleep blocker with an event behind it, then the staging of all inputs
               (copies from pinned host memory), then the chain.  After every call is enqueued the event must still be
               unfinished: a call that waited for the stream would have waited for the blocker.  A kernel or a memset
               launched off the stream runs before its inputs exist, and shows up as a difference.

Blocker length: 10 times the first run's enqueue time (the factor covers enqueue jitter on a shared machine), at least
50 ms; a need of more than 2 s fails the test as inconclusive.  _sleep's cycles per millisecond are measured once with events.
Both figures are printed.

EXEMPT lists the calls whose declaration says that they synchronise, with the sentence of include/mh.h that says so; they run
once on the stream without a blocker and are compared."""
import ctypes as C
import time

import numpy as np
import pytest

import __graft_entry__ as entry
import batch_ref
import damage
import find_ref
from oracle import mh_oracle

gpu = pytest.mark.gpu

CASES = batch_ref.draw_cases()
FILL = 0xA5
BLOCKER_FACTOR, BLOCKER_MIN_MS, BLOCKER_MAX_MS = 10, 50.0, 2000.0

# call -> the sentence of include/mh.h that exempts it from "no allocation, no synchronisation" (compared with the header, comment
# markers and line breaks aside, by test_the_exempt_list_quotes_the_header_and_is_run)
_LIMITED = "The device calls follow their unlimited twins (order 0 takes the host route; _ws: order 1 only, no allocation, one synchronisation)."
EXEMPT = {
    "mh_dev_model_from_counts": "mh_dev_model_from_counts allocates and synchronises once",
    "mh_dev_model_from_counts_ws": "mh_dev_model_from_counts_ws only synchronises once",
    "mh_dev_model_from_counts_limited": _LIMITED,
    "mh_dev_model_from_counts_limited_ws": _LIMITED,
    "mh_dev_model2_finish": "mh_dev_model2_finish derives every table from them (one stream synchronisation)",
    "mh_dev_build_index": "Unlike the other device calls this one synchronises `stream` between batches of passes",
    "mh_dev_build_index_fine": "Synchronises `stream` as mh_dev_build_index does.",
    "mh_dev_decode_stream_states": "Synchronises `stream` between its passes.",
    "mh_dev_decode_stream_emit": "No allocation; synchronises `stream` once, before its launch",
    "mh_dev_index_path": "0 nothing ran. Synchronises `stream`.",
    "mh_dev_encode_path": "so a wait is only ever for a workgroup that is running). Synchronises.",
    "mh_dev_decode_path": "2 the chunk decoder. Synchronises.",
    "mh_dev_decode_variant": "uses variant 9 REDO_LDS or 10 REDO_L2_DIRECT of the same layout. Synchronises.",
    "mh_dev_status": "Synchronises `stream` and returns the device-side status word of a workspace",
    "mh_dev_model_set_train": "synchronises `stream` twice: once to size the set (its live-context count), once at the end for the status.",
    "mh_dev_model_set_pick": "Allocates the view and synchronises `stream` once",
    "mh_dev_bank_train": "Allocates the bank and synchronises `stream` a number of times that depends on K and the iterations, not on n.",
    "mh_dev_batch_states_stats": "mh_dev_batch_states_stats (read-only, any order; synchronises the stream) says how the last states call in d_ws settled",
}


def test_the_exempt_list_quotes_the_header_and_is_run():
    import inspect
    import os
    import re
    import test_gpu_stream_order_edit as more                     # (the second module of these tests; it imports this one)
    with open(os.path.join(entry.ROOT, "include", "mh.h")) as f:
        header = re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", f.read()))
    run = inspect.getsource(test_exempt_calls_on_the_stream) + inspect.getsource(test_chain_d_one_stream) + \
        inspect.getsource(more.test_exempt_states_stats_on_the_stream)
    for call, sentence in EXEMPT.items():
        assert re.sub(r"\s+", " ", sentence) in header, "%s: not a sentence of include/mh.h: %s" % (call, sentence)
        assert header.count(call + "("), call
        assert "lib.%s(" % call in run, "%s is listed and never run on the stream" % call


STREAM_CALLS = 82                  # the declarations of include/mh.h that take `void *stream`, as stream_taking_calls() finds them
UNDRIVEN = {}                      # call -> why it cannot be driven on the stream; three entries at the most, each named in the pull request


def stream_taking_calls(header):
    """The names of the mh_dev_* declarations of a header whose argument list holds `void *stream`, comments stripped."""
    import re
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    return [m.group(1) for m in re.finditer(r"\b(mh_dev_\w+)\s*\(([^()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]


def test_every_stream_taking_call_is_driven_on_the_stream():
    """Every mh_dev_* call of include/mh.h that takes a stream appears as `lib.NAME` in the source of the stream-order modules
    (tests/test_gpu_stream_order*.py), in a chain or in an exempt test: a new call in the header fails this until a chain drives
    it.  `lib.NAME` followed by `(` or, where a chain hands the function to Chain.call or to an add_* helper, by `,` or `)`:
    never a longer name (`lib.NAME_workspace`).  The count is pinned so that a parser that finds nothing cannot pass."""
    import glob
    import os
    import re
    with open(os.path.join(entry.ROOT, "include", "mh.h")) as f:
        calls = stream_taking_calls(f.read())
    assert len(calls) == len(set(calls)) == STREAM_CALLS, "include/mh.h declares %d stream-taking device calls, this test pins %d" % (len(calls), STREAM_CALLS)
    source = ""
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_stream_order*.py"))):
        with open(path) as f:
            source += f.read()
    assert len(UNDRIVEN) <= 3 and set(UNDRIVEN) <= set(calls)
    missing = [c for c in calls if c not in UNDRIVEN and not re.search(r"\blib\.%s\b(?!\w)" % c, source)]
    assert not missing, "stream-taking calls of include/mh.h that no stream-order chain drives: %s" % ", ".join(missing)
    assert set(EXEMPT) <= set(calls), "an exempt call takes a stream"


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    import torch
    mhc = entry.load_package()
    e = Env()
    e.torch, e.mhc, e.lib = torch, mhc, mhc.lib()
    assert mhc.device_count() >= 1 and torch.cuda.is_available(), "GPU tests need a device; the codec has no CPU fallback"
    e.stream = torch.cuda.Stream()
    e.sp = C.c_void_p(e.stream.cuda_stream)
    assert e.sp.value, "a non-default stream has a handle"
    with torch.cuda.stream(e.stream):                             # cycles per millisecond of _sleep, measured once
        torch.cuda._sleep(1_000_000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
    b.synchronize()
    e.cycles_per_ms = 20_000_000 / a.elapsed_time(b)
    print("torch.cuda._sleep: %.0f cycles per ms" % e.cycles_per_ms)
    return e


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


class Chain:
    """The buffers, calls and expectations of one chain."""

    def __init__(self, env, name):
        self.env, self.name = env, name
        self.inputs, self.zeroed, self.filled, self.calls, self.spaces, self.statuses, self.expects = [], [], [], [], [], [], []

    def _alloc(self, nbytes, zero):
        d = self.env.torch.empty(max(int(nbytes), 16), dtype=self.env.torch.uint8, device="cuda")
        (self.zeroed if zero else self.filled).append(d)
        return d

    def staged(self, a):
        """An input: staged from pinned host memory on the stream.  Arrays of uint64 (offsets, lengths, lookups, index) are
        prefilled with zeros, bytes with FILL."""
        a = np.ascontiguousarray(a)
        host = self.env.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).pin_memory()
        d = self._alloc(host.numel(), a.dtype == np.uint64)
        if host.numel():
            self.inputs.append((d[:host.numel()], host))
        return d

    def words(self, n):
        """uint64[n] written by the chain (offsets, lengths, sym_off, index): prefilled with zeros."""
        return self._alloc(n * 8, True)

    def out(self, nbytes):
        """Bytes written by the chain (payloads, decoded bytes, counts, records): prefilled with FILL."""
        return self._alloc(nbytes, False)

    def work(self, nbytes):
        return self._alloc(nbytes, False)

    def status(self, n, what):
        d = self._alloc(max(n, 1) * 4, False)
        self.statuses.append((what, d, n))
        return d

    def call(self, name, fn, *args, ws=None):
        sp = self.env.sp
        self.calls.append((name, lambda: fn(*args, sp)))
        if ws is not None:
            self.spaces.append((name, ws))

    def expect(self, what, fn):
        self.expects.append((what, fn))

    def get(self, d, dtype=np.uint8, count=None):
        a = d.cpu().numpy().view(dtype)
        return a if count is None else a[:count]

    def run(self, blocker_ms=None):
        """Prefill, (blocker,) staging, the calls back to back, one synchronisation: (host ms to enqueue, the first step after
        which the blocker's event had finished or None)."""
        torch, stream = self.env.torch, self.env.stream
        for d in self.zeroed:
            d.zero_()
        for d in self.filled:
            d.fill_(FILL)
        torch.cuda.synchronize()
        self.rcs, early, ev = [], None, None
        with torch.cuda.stream(stream):
            if blocker_ms is not None:
                torch.cuda._sleep(int(blocker_ms * self.env.cycles_per_ms))
                ev = torch.cuda.Event()
                ev.record()
            t0 = time.perf_counter()
            for d, host in self.inputs:
                d.copy_(host, non_blocking=True)
            if ev is not None and ev.query():
                early = "the staging of the inputs"
            for name, thunk in self.calls:
                self.rcs.append((name, thunk()))
                if ev is not None and early is None and ev.query():
                    early = name
            ms = (time.perf_counter() - t0) * 1e3
        stream.synchronize()
        if blocker_ms is not None:                                # (the blocker ran for what it was sized for, or nothing was proved)
            waited = (time.perf_counter() - t0) * 1e3
            assert waited >= 0.8 * blocker_ms, "%s: the blocker of %.0f ms was over after %.1f ms" % (self.name, blocker_ms, waited)
        return ms, early

    def verify(self, run):
        """Return codes, workspace statuses, per-stream statuses and every output against its reference: all that differs."""
        lib, bad = self.env.lib, []
        bad += ["%s returned %d" % (name, rc) for name, rc in self.rcs if rc != 0]
        for name, ws in self.spaces:
            rc = lib.mh_dev_status(ptr(ws), self.env.sp)
            if rc != 0:
                bad.append("%s: mh_dev_status %d" % (name, rc))
        for what, d, n in self.statuses:
            if self.get(d, np.int32, n).any():
                bad.append("%s: per-stream statuses %s" % (what, np.unique(self.get(d, np.int32, n)).tolist()))
        for what, fn in self.expects:
            try:
                if not fn():
                    bad.append(what)
            except Exception as e:                                # (a comparison that cannot be made is a difference)
                bad.append("%s: %s: %s" % (what, type(e).__name__, e))
        assert not bad, "%s, %s: %d differences:\n  %s" % (self.name, run, len(bad), "\n  ".join(bad))


def drive(chain):
    ms, _ = chain.run()
    chain.verify("first run (no blocker)")
    blocker = max(BLOCKER_MIN_MS, BLOCKER_FACTOR * ms)
    print("%s: %d calls enqueued in %.2f ms, blocker %.0f ms" % (chain.name, len(chain.calls), ms, blocker))
    if blocker > BLOCKER_MAX_MS:
        pytest.fail("%s: inconclusive: enqueueing took %.1f ms, a blocker of %.0f ms would be needed" % (chain.name, ms, blocker))
    ms2, early = chain.run(blocker)
    print("%s: blocked run enqueued in %.2f ms" % (chain.name, ms2))
    assert early is None, ("%s: the blocker (%.0f ms) had finished after %s was enqueued (%.1f ms for the whole chain): that call "
                           "waited for the stream, or the blocker was too short" % (chain.name, blocker, early, ms2))
    chain.verify("second run (behind the blocker)")


# ---- the pieces of the chains -------------------------------------------------------------------------------------------
class Batch:
    """A batch on the device: payload, pay_off, nbits (device buffers), n, pay_total (host values of the reference)."""

    def __init__(self, pl, po, nb, n, pay_total):
        self.pl, self.po, self.nb, self.n, self.pay_total = pl, po, nb, n, pay_total

    def args(self):
        return ptr(self.pl), ptr(self.po), ptr(self.nb), self.n, self.pay_total


def packed_out_at(lengths):
    at = np.zeros(max(len(lengths), 1), dtype=np.uint64)
    at[1:len(lengths)] = np.cumsum(lengths, dtype=np.uint64)[:-1]
    return at


def add_decode(ch, tag, fn, ws_fn, handle, b, p0, total, d_sym_off, d_index, chunk, want_bytes, want_sym_off):
    """Indexed (d_index given; d_sym_off is input) or index-free (d_sym_off is written) batch decode of the whole batch."""
    lib = ch.env.lib
    wsb = ws_fn(b.n)
    d_ws, d_out, d_st = ch.work(wsb), ch.out(total + 64), ch.status(b.n, tag)
    d_so = d_sym_off if d_index is not None else ch.words(b.n + 1)
    ch.call(tag, fn, handle, *b.args(), p0, ptr(d_out), total, ptr(d_so), total if d_index is not None else 0, ptr(d_index),
            chunk if d_index is not None else 0, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": bytes", lambda: ch.get(d_out, np.uint8, total).tobytes() == want_bytes and (ch.get(d_out)[total:total + 64] == FILL).all())
    ch.expect(tag + ": sym_off", lambda: same(ch.get(d_so, np.uint64, b.n + 1), want_sym_off))


def add_lookups(ch, tag, fn, ws_fn, handle, b, p0, d_sym_off, d_index, chunk, lookups, lookup_bytes):
    lk = np.asarray(lookups, dtype=np.uint64).reshape(-1, 3)
    m = lk.shape[0]
    ln = (lk[:, 2] - lk[:, 1]).astype(np.uint64)
    at = packed_out_at(ln)
    size = int(ln.sum())
    d_lk, d_at = ch.staged(lk), ch.staged(at)
    wsb = ws_fn(m)
    d_ws, d_out, d_st = ch.work(wsb), ch.out(size + 64), ch.status(m, tag)
    ch.call(tag, fn, handle, ptr(b.pl), ptr(b.po), ptr(b.nb), b.n, p0, ptr(d_sym_off), ptr(d_index), chunk, ptr(d_lk), m, ptr(d_out),
            ptr(d_at), size, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": bytes", lambda: ch.get(d_out, np.uint8, size).tobytes() == b"".join(lookup_bytes) and (ch.get(d_out)[size:size + 64] == FILL).all())


def add_find(ch, tag, fn, ws_fn, handle, ps, b, p0, total, d_sym_off, d_index, chunk, hits):
    """Count only, then with records; the hit capacity is the reference's number of hits."""
    n = b.n
    w_off, w_rec, w_pat = find_ref.hit_arrays(hits, n)
    k = len(hits)
    wsb = ws_fn(n, total, chunk)
    for records in (False, True):
        t = tag + (" records" if records else " count only")
        d_ws, d_ho, d_st = ch.work(wsb), ch.words(n + 1), ch.status(n, t)
        d_rec, d_pat = (ch.out(k * 24 + 64), ch.out(k * 4 + 64)) if records else (None, None)
        ch.call(t, fn, handle, ps.handle, *b.args(), p0, ptr(d_sym_off), total, ptr(d_index), chunk, ptr(d_ho), ptr(d_rec), ptr(d_pat),
                k if records else 0, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
        ch.expect(t + ": hit_off", lambda d_ho=d_ho: same(ch.get(d_ho, np.uint64, n + 1), w_off))
        if records:
            ch.expect(t + ": records", lambda d_rec=d_rec: same(ch.get(d_rec, np.uint64, 3 * k).reshape(-1, 3), w_rec))
            ch.expect(t + ": patterns", lambda d_pat=d_pat: same(ch.get(d_pat, np.uint32, k), w_pat))


def add_coded_histogram(ch, tag, fn, ws_fn, handle, order, b, p0, total, d_sym_off, d_index, chunk, want):
    nc = want.size
    wsb = ws_fn(b.n, total, chunk)
    d_ws, d_counts, d_st = ch.work(wsb), ch.out(nc * 8 + 64), ch.status(b.n, tag)
    ch.call(tag, fn, handle, order, *b.args(), p0, ptr(d_sym_off), total, ptr(d_index), chunk, ptr(d_counts), ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    ch.expect(tag + ": counts", lambda: same(ch.get(d_counts, np.uint64, nc), want) and (ch.get(d_counts)[nc * 8:] == FILL).all())


def add_recode(ch, tag, fn, ws_fn, src, dst, b, p0, total, d_sym_off, d_index, chunk, rd):
    """Count only, then in full with exactly the reference's payload bytes of room.  Returns the re-coded batch and its index."""
    lib, n = ch.env.lib, b.n
    cap = int(rd.pay_off[n])
    nidx = int(lib.mh_batch_index_capacity(total, n, chunk))
    wsb = ws_fn(n, total, chunk)
    res = None
    for full in (False, True):
        t = tag + ("" if full else " count only")
        d_ws, d_st = ch.work(wsb), ch.status(n, t)
        d_oo, d_onb, d_dr = ch.words(n + 1), ch.words(n), ch.words(n)
        d_out, d_oi = (ch.out(cap + 64), ch.words(nidx)) if full else (None, None)
        ch.call(t, fn, src, dst, *b.args(), p0, ptr(d_sym_off), total, ptr(d_index), chunk, ptr(d_out), cap, ptr(d_oo), ptr(d_onb), ptr(d_oi),
                ptr(d_dr), ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
        ch.expect(t + ": offsets, nbits, dropped", lambda d_oo=d_oo, d_onb=d_onb, d_dr=d_dr: same(ch.get(d_oo, np.uint64, n + 1), rd.pay_off)
                  and same(ch.get(d_onb, np.uint64, n), rd.nbits) and same(ch.get(d_dr, np.uint64, n), rd.dropped))
        if full:
            ch.expect(t + ": payload", lambda d_out=d_out: same(ch.get(d_out, np.uint8, cap), rd.payload) and (ch.get(d_out)[cap:cap + 64] == FILL).all())
            ch.expect(t + ": index slices", lambda d_oi=d_oi: same(rd.slices_of(ch.get(d_oi, np.uint64, nidx), chunk), rd.all_slices()))
            res = Batch(d_out, d_oo, d_onb, n, cap), d_oi
    return res


def add_decode_of_recoded(ch, tag, env, dst, dst_oracle, b, d_index, d_sym_off, p0, total, chunk, rd, msgs):
    """mh_dev_decode_batch of a re-coded batch.  Nothing dropped: indexed, through the index the re-coding wrote, the messages
    come back.  Symbols dropped (a destination that lacks pairs of the batch): the decoder's context differs from the encoder's
    behind a dropped symbol, so the reference is the strict CPU decode of every re-coded stream (damage.verdict_free) and the
    decode is index-free; a failed stream's length is not pinned."""
    lib = env.lib
    if not rd.dropped.any():
        add_decode(ch, tag, lib.mh_dev_decode_batch, lib.mh_dev_decode_batch_workspace, dst.handle, b, p0, total, d_sym_off, d_index, chunk,
                   b"".join(msgs), rd.sym_off)
        return
    n = b.n
    want = [damage.verdict_free(dst_oracle, rd.payload[int(rd.pay_off[i]):int(rd.pay_off[i + 1])], int(rd.nbits[i]), p0) for i in range(n)]
    assert all(w == (damage.MH_OK, m) for w, m, dr in zip(want, msgs, rd.dropped) if not dr), "a stream without a dropped symbol decodes to its message"
    wsb = lib.mh_dev_decode_batch_workspace(n)
    d_ws, d_out, d_so, d_st = ch.work(wsb), ch.out(total + 64), ch.words(n + 1), ch.out(max(n, 1) * 4)
    ch.call(tag, lib.mh_dev_decode_batch, dst.handle, *b.args(), p0, ptr(d_out), total, ptr(d_so), 0, None, 0, ptr(d_st), ptr(d_ws), wsb)

    def check():
        out, so, st = ch.get(d_out), ch.get(d_so, np.uint64, n + 1), ch.get(d_st, np.int32, n)
        for i, (ws, wb) in enumerate(want):
            if int(st[i]) != ws or (ws == damage.MH_OK and out[int(so[i]):int(so[i + 1])].tobytes() != wb):
                return False
        failed = {ws for ws, _ in want if ws != damage.MH_OK}
        return lib.mh_dev_status(ptr(d_ws), env.sp) in (failed or {0}) and (out[total:total + 64] == FILL).all()
    ch.expect(tag + ": statuses and bytes of every stream against the strict CPU decode", check)
    # and indexed, through the index the re-coding wrote: the streams that dropped nothing come back at their places
    d_ws2, d_out2, d_st2 = ch.work(wsb), ch.out(total + 64), ch.out(max(n, 1) * 4)
    ch.call(tag + " (indexed)", lib.mh_dev_decode_batch, dst.handle, *b.args(), p0, ptr(d_out2), total, ptr(d_sym_off), total, ptr(d_index), chunk,
            ptr(d_st2), ptr(d_ws2), wsb)

    def check_indexed():
        out, st, so = ch.get(d_out2), ch.get(d_st2, np.int32, n), rd.sym_off.astype(np.int64)
        whole = [i for i in range(n) if not rd.dropped[i]]
        return all(int(st[i]) == 0 and out[so[i]:so[i + 1]].tobytes() == msgs[i] for i in whole) and (out[total:total + 64] == FILL).all()
    ch.expect(tag + " (indexed): statuses and bytes of the streams that dropped nothing", check_indexed)


def shared_chain(env, name, case_index, case_id):
    """Chains A and B: a case of the fuzz under its shared source model, re-coded under its destination model."""
    mhc, lib = env.mhc, env.lib
    case = CASES[case_index]
    assert case.id == case_id
    w = case.world()
    so, do = case.orders
    msgs, p0, c = w.messages, w.prev0, case.chunk
    n, joined = len(msgs), b"".join(w.messages)
    total = len(joined)
    (sc, sl), (dc, dl) = case.counts("src"), case.counts("dst")
    S, D = mhc.Model.from_counts(sc, so, max_len=sl), mhc.Model.from_counts(dc, do, max_len=dl)
    rs = batch_ref.pack(msgs, *case.codes("src"), so, p0, c)
    rd = batch_ref.pack(msgs, *case.codes("dst"), do, p0, c)
    o2 = so == 2
    ch = Chain(env, name)
    d_data = ch.staged(np.frombuffer(joined, dtype=np.uint8))
    d_in = ch.staged(rs.sym_off)
    pay_total, nidx = int(rs.pay_off[n]), int(lib.mh_batch_index_capacity(total, n, c))

    # 1. training histograms of the messages
    for order in ((2,) if o2 else (1, 0)):
        want = batch_ref.histogram(msgs, order, p0)
        fn = {0: lib.mh_dev_histogram_o0_batch, 1: lib.mh_dev_histogram_o1_batch, 2: lib.mh_dev_histogram_o2_batch}[order]
        wsb = (lib.mh_dev_histogram_o2_batch_workspace if order == 2 else lib.mh_dev_histogram_batch_workspace)(total)
        d_ws, d_counts = ch.work(wsb), ch.out(want.size * 8)
        args = (ptr(d_data), ptr(d_in), n, total) + ((p0,) if order else ()) + (ptr(d_counts), ptr(d_ws), wsb)
        ch.call("histogram_o%d_batch" % order, fn, *args, ws=d_ws)
        ch.expect("histogram_o%d_batch" % order, lambda d_counts=d_counts, want=want: same(ch.get(d_counts, np.uint64, want.size), want))

    # 2. encode with index
    cap = lib.mh_encode_batch_bound(S.handle, total, n)
    assert cap >= pay_total
    wsb = (lib.mh_dev_encode_batch_o2_workspace if o2 else lib.mh_dev_encode_batch_workspace)(n, total)
    d_ws, d_pl, d_po, d_nb, d_idx = ch.work(wsb), ch.out(cap + 64), ch.words(n + 1), ch.words(n), ch.words(nidx)
    ch.call("encode_batch", lib.mh_dev_encode_batch_o2 if o2 else lib.mh_dev_encode_batch, S.handle, ptr(d_data), ptr(d_in), n, total, p0,
            ptr(d_pl), cap, ptr(d_po), ptr(d_nb), ptr(d_idx), c, ptr(d_ws), wsb, ws=d_ws)
    ch.expect("encode_batch: offsets, nbits", lambda: same(ch.get(d_po, np.uint64, n + 1), rs.pay_off) and same(ch.get(d_nb, np.uint64, n), rs.nbits))
    ch.expect("encode_batch: payload", lambda: same(ch.get(d_pl, np.uint8, pay_total), rs.payload) and (ch.get(d_pl)[cap:] == FILL).all())
    ch.expect("encode_batch: index slices", lambda: same(rs.slices_of(ch.get(d_idx, np.uint64, nidx), c), rs.all_slices()))
    b = Batch(d_pl, d_po, d_nb, n, pay_total)

    # 3. decode, indexed and index-free
    dec, dec_ws = (lib.mh_dev_decode_batch_o2, lib.mh_dev_decode_batch_o2_workspace) if o2 else (lib.mh_dev_decode_batch, lib.mh_dev_decode_batch_workspace)
    add_decode(ch, "decode_batch indexed", dec, dec_ws, S.handle, b, p0, total, d_in, d_idx, c, joined, rs.sym_off)
    add_decode(ch, "decode_batch index-free", dec, dec_ws, S.handle, b, p0, total, None, None, 0, joined, rs.sym_off)

    # 4. segment states, then index and emit from them (order 0 / 1)
    if not o2:
        wsb = lib.mh_dev_batch_states_workspace(n, pay_total)
        d_ws, d_so, d_idx2, d_out = ch.work(wsb), ch.words(n + 1), ch.words(nidx), ch.out(total + 64)
        st = [ch.status(n, "batch_" + k) for k in ("states", "index", "emit")]
        ch.call("batch_states", lib.mh_dev_batch_states, S.handle, *b.args(), p0, ptr(d_so), ptr(st[0]), ptr(d_ws), wsb, ws=d_ws)
        ch.call("batch_index", lib.mh_dev_batch_index, S.handle, *b.args(), p0, ptr(d_idx2), nidx, c, ptr(st[1]), ptr(d_ws), wsb)
        ch.call("batch_emit", lib.mh_dev_batch_emit, S.handle, *b.args(), p0, ptr(d_out), total, ptr(st[2]), ptr(d_ws), wsb)
        ch.expect("batch_states: sym_off", lambda: same(ch.get(d_so, np.uint64, n + 1), rs.sym_off))
        ch.expect("batch_index: slices", lambda: same(rs.slices_of(ch.get(d_idx2, np.uint64, nidx), c), rs.all_slices()))
        ch.expect("batch_emit: bytes", lambda: ch.get(d_out, np.uint8, total).tobytes() == joined and (ch.get(d_out)[total:total + 64] == FILL).all())

    # 5. lookups, indexed and index-free
    lk, lk_ws = (lib.mh_dev_decode_batch_o2_ranges, lib.mh_dev_decode_batch_o2_ranges_workspace) if o2 else \
        (lib.mh_dev_decode_batch_ranges, lib.mh_dev_decode_batch_ranges_workspace)
    add_lookups(ch, "decode_batch_ranges indexed", lk, lk_ws, S.handle, b, p0, d_in, d_idx, c, w.lookups, w.lookup_bytes)
    if not o2:
        add_lookups(ch, "decode_batch_ranges index-free", lk, lk_ws, S.handle, b, p0, None, None, c, w.lookups, w.lookup_bytes)

    # 6. search
    ps = mhc.PatternSet(w.patterns, fold=w.fold)
    ch.keep = (S, D, ps)
    hits = find_ref.find_hits(msgs, w.patterns, fold=w.fold)
    add_find(ch, "find_batch", lib.mh_dev_find_batch_o2 if o2 else lib.mh_dev_find_batch,
             lib.mh_dev_find_batch_o2_workspace if o2 else lib.mh_dev_find_batch_workspace, S.handle, ps, b, p0, total, d_in, d_idx, c, hits)

    # 7. coded histograms
    for order in ((2,) if o2 else (0, 1)):
        add_coded_histogram(ch, "histogram_coded_batch order %d" % order,
                            lib.mh_dev_histogram_coded_batch_o2 if o2 else lib.mh_dev_histogram_coded_batch,
                            lib.mh_dev_histogram_coded_batch_o2_workspace if o2 else lib.mh_dev_histogram_coded_workspace,
                            S.handle, order, b, p0, total, d_in, d_idx, c, batch_ref.histogram(msgs, order, p0))

    # 8. re-code under the destination model, 9. decode the result under it
    two = 2 in case.orders
    rb, d_oi = add_recode(ch, "recode_batch", lib.mh_dev_recode_batch_o2 if two else lib.mh_dev_recode_batch,
                          lib.mh_dev_recode_batch_o2_workspace if two else lib.mh_dev_recode_batch_workspace,
                          S.handle, D.handle, b, p0, total, d_in, d_idx, c, rd)
    assert do < 2
    add_decode_of_recoded(ch, "decode_batch of the re-coded batch", env, D, mh_oracle.Model.from_counts(dc, do), rb, d_oi, d_in, p0, total, c, rd, msgs)
    return ch


@gpu
def test_chain_a_shared_order_0_1(env):
    drive(shared_chain(env, "chain A", 32, "032-uniform-deep1-deep0-c1024-n65"))


@gpu
def test_chain_b_order_2(env):
    drive(shared_chain(env, "chain B", 88, "088-text-own2-foreign1-c1024-n257"))


@gpu
def test_chain_c_one_model_per_stream(env):
    mhc, lib = env.mhc, env.lib
    case = CASES[32]
    assert case.id == "032-uniform-deep1-deep0-c1024-n65"
    w = case.world()
    order, do = case.orders
    msgs, p0, c = w.messages, w.prev0, case.chunk
    n, joined = len(msgs), b"".join(w.messages)
    total = len(joined)
    re, tables = batch_ref.pack_each(msgs, order, p0, c)
    ms = mhc.ModelSet.from_tables(tables)
    dc, dl = case.counts("dst")
    D = mhc.Model.from_counts(dc, do, max_len=dl)
    rd = batch_ref.pack(msgs, *case.codes("dst"), do, p0, c)
    ch = Chain(env, "chain C")
    pay_total = int(re.pay_off[n])
    b = Batch(ch.staged(np.concatenate([re.payload, np.zeros(64, dtype=np.uint8)])), ch.staged(re.pay_off), ch.staged(re.nbits), n, pay_total)
    d_in, d_idx = ch.staged(re.sym_off), ch.staged(re.index_array(c))
    ps = mhc.PatternSet(w.patterns, fold=w.fold)
    ch.keep = (ms, D, ps)
    add_decode(ch, "decode_each indexed", lib.mh_dev_decode_each, lib.mh_dev_decode_each_workspace, ms.handle, b, p0, total, d_in, d_idx, c, joined, re.sym_off)
    add_decode(ch, "decode_each index-free", lib.mh_dev_decode_each, lib.mh_dev_decode_each_workspace, ms.handle, b, p0, total, None, None, 0, joined,
               re.sym_off)
    add_lookups(ch, "decode_each_ranges", lib.mh_dev_decode_each_ranges, lib.mh_dev_decode_batch_ranges_workspace, ms.handle, b, p0, d_in, d_idx, c,
                w.lookups, w.lookup_bytes)
    add_find(ch, "find_each", lib.mh_dev_find_each, lib.mh_dev_find_batch_workspace, ms.handle, ps, b, p0, total, d_in, d_idx, c,
             find_ref.find_hits(msgs, w.patterns, fold=w.fold))
    add_coded_histogram(ch, "histogram_coded_each", lib.mh_dev_histogram_coded_each, lib.mh_dev_histogram_coded_workspace, ms.handle, 1, b, p0, total,
                        d_in, d_idx, c, batch_ref.histogram(msgs, 1, p0))
    add_recode(ch, "recode_each", lib.mh_dev_recode_each, lib.mh_dev_recode_batch_workspace, ms.handle, D.handle, b, p0, total, d_in, d_idx, c, rd)
    drive(ch)


# ---- chain D: one stream ----------------------------------------------------------------------------------------------------
def zipf_stream(n=300_000, seed=7, s=1.1):
    w = 1.0 / np.arange(1, 257) ** s
    return np.random.default_rng(seed).choice(256, size=n, p=w / w.sum()).astype(np.uint8)


@pytest.fixture(scope="module")
def one_stream(env):
    """300 000 bytes of Zipf(1.1) with the oracle's counts, model, stream and chunk index (chunk 1024)."""
    data = zipf_stream()
    raw = data.tobytes()
    counts = mh_oracle.histogram_o1(raw)
    om = mh_oracle.Model.from_counts(counts, 1)
    blob, nbits = om.compress(raw)
    ref = batch_ref.pack([raw], *batch_ref.oracle_codes(counts, 1), 1, batch_ref.PREV0, 1024)
    assert ref.payload.tobytes() == blob[1:] and int(ref.nbits[0]) == nbits
    return dict(data=data, raw=raw, counts=np.asarray(counts, dtype=np.uint64), payload=np.frombuffer(blob[1:], dtype=np.uint8), nbits=nbits,
                index=ref.slices[0], model=env.mhc.Model.from_counts(counts, 1))


@gpu
def test_chain_d_one_stream(env, one_stream):
    lib, o = env.lib, one_stream
    m, data, n, nbits, c, p0 = o["model"], o["data"], o["data"].size, o["nbits"], 1024, batch_ref.PREV0
    pay_bytes, n_idx = (nbits + 7) // 8, (n + c - 1) // c
    ch = Chain(env, "chain D")
    d_data = ch.staged(data)
    # 1. histogram with its full workspace (which keeps what mh_dev_encode_hist needs)
    hwsb = lib.mh_dev_histogram_workspace(n)
    d_hws, d_counts = ch.work(hwsb), ch.out(65536 * 8)
    ch.call("histogram_o1", lib.mh_dev_histogram_o1, ptr(d_data), n, p0, ptr(d_counts), ptr(d_hws), hwsb, ws=d_hws)
    ch.expect("histogram_o1", lambda: same(ch.get(d_counts, np.uint64, 65536), o["counts"]))
    # 2. encode from that histogram
    cap, wsb = lib.mh_encode_bound(m.handle, n), lib.mh_dev_encode_workspace(n)
    assert cap >= pay_bytes
    d_ws, d_pl, d_nb, d_idx = ch.work(wsb), ch.out(cap + 64), ch.words(1), ch.words(n_idx)
    d_ews = d_ws
    ch.call("encode_hist", lib.mh_dev_encode_hist, m.handle, ptr(d_data), n, p0, None, ptr(d_pl), cap, ptr(d_nb), ptr(d_idx), c, ptr(d_hws), hwsb,
            ptr(d_ws), wsb, ws=d_ws)
    ch.expect("encode_hist: nbits", lambda: int(ch.get(d_nb, np.uint64, 1)[0]) == nbits)
    ch.expect("encode_hist: payload", lambda: same(ch.get(d_pl, np.uint8, pay_bytes), o["payload"]) and (ch.get(d_pl)[cap:] == FILL).all())
    ch.expect("encode_hist: index", lambda: same(ch.get(d_idx, np.uint64, n_idx), o["index"]))
    # 3. the payload bits from the device counts
    d_bits = ch.words(1)
    ch.call("payload_bits", lib.mh_dev_payload_bits, m.handle, ptr(d_counts), ptr(d_bits))
    ch.expect("payload_bits", lambda: int(ch.get(d_bits, np.uint64, 1)[0]) == nbits)
    # 4. decode with the index
    wsb = lib.mh_dev_decode_workspace(nbits, n, c)
    d_ws, d_out = ch.work(wsb), ch.out(n + 64)
    d_dws = d_ws
    ch.call("decode", lib.mh_dev_decode, m.handle, ptr(d_pl), nbits, ptr(d_out), n, ptr(d_idx), c, ptr(d_ws), wsb, ws=d_ws)
    ch.expect("decode", lambda: ch.get(d_out, np.uint8, n).tobytes() == o["raw"] and (ch.get(d_out)[n:n + 64] == FILL).all())
    # 5. seven ranges: across one and two chunk seams, on a seam, empty, the whole first chunk, up to the last byte
    ranges = np.array([(c - 1, c + 1), (c - 40, 2 * c + 40), (5 * c, 6 * c), (7 * c + 3, 7 * c + 3), (0, c), (n - 1500, n), (n - 1, n)], dtype=np.uint64)
    ln = ranges[:, 1] - ranges[:, 0]
    size = int(ln.sum())
    d_rg, d_at = ch.staged(ranges), ch.staged(packed_out_at(ln))
    wsb = lib.mh_dev_decode_ranges_workspace(len(ranges))
    d_ws, d_rout, d_st = ch.work(wsb), ch.out(size + 64), ch.status(len(ranges), "decode_ranges")
    ch.call("decode_ranges", lib.mh_dev_decode_ranges, m.handle, ptr(d_pl), 0, pay_bytes, nbits, ptr(d_idx), c, n, None, ptr(d_rg), len(ranges),
            ptr(d_rout), ptr(d_at), size, ptr(d_st), ptr(d_ws), wsb, ws=d_ws)
    want = b"".join(o["raw"][int(a):int(e)] for a, e in ranges)
    ch.expect("decode_ranges", lambda: ch.get(d_rout, np.uint8, size).tobytes() == want and (ch.get(d_rout)[size:size + 64] == FILL).all())
    drive(ch)
    # the path diagnostics (they synchronise: after the chain).  Encoder: priced from the histogram, with the escape variant
    # when the model has a code over 12 bits.  Decoder: no fine index, so the chunk decoder, in the variant of mh.h's table.
    longest = int(batch_ref.oracle_codes(o["counts"], 1)[0].max())
    assert m.max_code_len == longest
    assert lib.mh_dev_encode_path(ptr(d_ews), env.sp) == (3 if longest > 12 else 1), "mh_dev_encode_path"
    assert lib.mh_dev_decode_path(ptr(d_dws), env.sp) == 2, "mh_dev_decode_path"
    primary, secondary, in_lds = m.decode_layout()
    if in_lds:
        short = secondary == 0 and primary == 8
        variant = (0 if nbits * 10 > n * 8 * 6 else 1) if short else 3 if primary == 8 else 2
    else:
        variant = {10: 5, 11: 6, 12: 7}.get(longest, 8 if longest >= 16 else 4)
    assert lib.mh_dev_decode_variant(ptr(d_dws), env.sp) == variant, "mh_dev_decode_variant"


# ---- the calls that say they synchronise: once on the stream, no blocker, compared -----------------------------------------
@gpu
def test_exempt_calls_on_the_stream(env, one_stream):
    torch, mhc, lib, o, sp = env.torch, env.mhc, env.lib, one_stream, env.sp
    n, nbits, c, p0 = o["data"].size, o["nbits"], 1024, batch_ref.PREV0
    om = mh_oracle.Model.from_counts(o["counts"], 1)

    def dev(a):
        a = np.ascontiguousarray(a)
        with torch.cuda.stream(env.stream):
            t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda")
        env.stream.synchronize()
        return t

    def empty(nbytes):
        return torch.full((max(int(nbytes), 16),), FILL, dtype=torch.uint8, device="cuda")

    def model(fn, *args):
        h = C.c_void_p()
        assert fn(*args, sp, C.byref(h)) == 0, fn.__name__
        return mhc.Model(h)

    torch.cuda.synchronize()
    # the model builders: the table the oracle writes for these counts; limited: the host-built limited model's table
    d_counts = dev(o["counts"])
    wsb = lib.mh_dev_model_workspace(1)
    d_mws, d_mws2 = empty(wsb), empty(wsb)
    m1 = model(lambda *a: lib.mh_dev_model_from_counts(*a), ptr(d_counts), 1)
    m2 = model(lambda *a: lib.mh_dev_model_from_counts_ws(*a), ptr(d_counts), 1, ptr(d_mws), wsb)
    m3 = model(lambda *a: lib.mh_dev_model_from_counts_limited(*a), ptr(d_counts), 1, 12)
    m4 = model(lambda *a: lib.mh_dev_model_from_counts_limited_ws(*a), ptr(d_counts), 1, 12, ptr(d_mws2), wsb)
    limited = batch_ref.limited_codes(o["counts"], 1, 12)[0]
    assert int(batch_ref.oracle_codes(o["counts"], 1)[0].max()) > 12, "the limit binds"
    assert m1.table_bytes() == om.table_bytes() and m2.table_bytes() == om.table_bytes(), "mh_dev_model_from_counts, _ws"
    for m in (m3, m4):
        assert m.table_bytes() == mhc.Model.from_counts(o["counts"], 1, max_len=12).table_bytes(), "mh_dev_model_from_counts_limited, _ws"
        assert same(np.frombuffer(m.image(1), dtype=np.uint8)[:65536], limited), "limited code lengths against package-merge"
    del m2, m3, m4, m

    # mh_dev_model2_finish: the order-2 model of case 088's messages, all contexts built in one slice
    case2 = CASES[88]
    assert case2.orders[0] == 2 and case2.src_kind == "own"
    counts2, _ = case2.counts("src")
    d_counts2 = dev(counts2)
    wsb2 = lib.mh_dev_model2_workspace()
    d_ws2 = torch.empty(wsb2, dtype=torch.uint8, device="cuda")
    assert lib.mh_dev_model2_build_slice(ptr(d_counts2), 0, 65536, ptr(d_ws2), wsb2, sp) == 0
    mo2 = model(lambda *a: lib.mh_dev_model2_finish(*a), ptr(d_ws2), wsb2)
    lens2, codes2 = case2.codes("src")
    got_l, got_c = mo2.codes_o2()
    assert mo2.type == 2 and same(got_l, lens2) and same(got_c[lens2 > 0], codes2[lens2 > 0]), "mh_dev_model2_finish"
    assert mo2.table_bytes() == mh_oracle.Model.from_counts(counts2, 2).table_bytes(), "mh_dev_model2_finish: table"
    del mo2, d_ws2, d_counts2

    # mh_dev_build_index and _fine: the chunk index, the fine index and the symbol count of the oracle's stream (which
    # carries none); a model with tile tables and a stream of over a megabit: the tile path (5)
    d_pl = dev(np.concatenate([o["payload"], np.zeros(64, dtype=np.uint8)]))
    n_idx, n_fine, fcap = (n + c - 1) // c, (n + 63) // 64, nbits // 64 + 2
    assert nbits >= 1 << 20 and m1.tile_layout()[0] > 0
    wsb = lib.mh_dev_build_index_workspace(nbits)
    d_ws, d_idx, d_ns, d_fine = empty(wsb), empty((n_idx + 8) * 8), empty(8), empty(fcap * 4)
    rc = lib.mh_dev_build_index(m1.handle, ptr(d_pl), nbits, p0, ptr(d_idx), n_idx + 8, c, ptr(d_ns), ptr(d_ws), wsb, sp)
    assert rc == 0 and lib.mh_dev_status(ptr(d_ws), sp) == 0 and lib.mh_dev_index_path(ptr(d_ws), sp) == 5
    assert int(d_ns.cpu().numpy().view(np.uint64)[0]) == n and same(d_idx.cpu().numpy().view(np.uint64)[:n_idx], o["index"]), "mh_dev_build_index"
    d_idx.fill_(FILL)
    d_ns.fill_(FILL)
    torch.cuda.synchronize()
    rc = lib.mh_dev_build_index_fine(m1.handle, ptr(d_pl), nbits, p0, ptr(d_idx), n_idx + 8, c, ptr(d_fine), fcap, ptr(d_ns), ptr(d_ws), wsb, sp)
    assert rc == 0 and lib.mh_dev_status(ptr(d_ws), sp) == 0 and lib.mh_dev_index_path(ptr(d_ws), sp) == 5
    lens = batch_ref.oracle_codes(o["counts"], 1)[0]
    sym = o["data"].astype(np.int64)
    prev = np.concatenate([[p0], sym[:-1]])
    pos = np.concatenate([[0], np.cumsum(lens[prev * 256 + sym])[:-1]])
    at = np.arange(0, n, 64)
    fine = ((prev[at] << 24) | (pos[at] & 0xFFFFFF)).astype(np.uint32)      # (mh.h, FINE INDEX: context << 24 | low 24 bits of the offset)
    assert int(d_ns.cpu().numpy().view(np.uint64)[0]) == n and same(d_idx.cpu().numpy().view(np.uint64)[:n_idx], o["index"]), "mh_dev_build_index_fine"
    assert same(d_fine.cpu().numpy().view(np.uint32)[:n_fine], fine), "mh_dev_build_index_fine: fine index"

    # mh_dev_decode_stream_states / _emit: the two-pass decode of the same stream, which takes that path (6) as it takes 5 above
    d_out = empty(n + 64)
    d_ns.fill_(FILL)
    torch.cuda.synchronize()
    rc = lib.mh_dev_decode_stream_states(m1.handle, ptr(d_pl), nbits, p0, ptr(d_ns), ptr(d_ws), wsb, sp)
    assert rc == 0 and lib.mh_dev_index_path(ptr(d_ws), sp) == 6 and lib.mh_dev_status(ptr(d_ws), sp) == 0, "mh_dev_decode_stream_states"
    assert int(d_ns.cpu().numpy().view(np.uint64)[0]) == n, "mh_dev_decode_stream_states"
    rc = lib.mh_dev_decode_stream_emit(m1.handle, ptr(d_pl), nbits, p0, ptr(d_out), n, ptr(d_ws), wsb, sp)
    assert rc == 0 and lib.mh_dev_status(ptr(d_ws), sp) == 0
    got = d_out.cpu().numpy()
    assert got[:n].tobytes() == o["raw"] and (got[n:n + 64] == FILL).all(), "mh_dev_decode_stream_emit"

    # mh_dev_model_set_train: one model per stream of case 032, the oracle's table of every message
    case = CASES[32]
    w = case.world()
    _, tables = batch_ref.pack_each(w.messages, 1, w.prev0, case.chunk)
    data, off = mhc.batch_offsets(w.messages)
    d_data, d_off = dev(data), dev(off)
    nst = len(w.messages)
    wsb = lib.mh_dev_model_set_train_workspace(nst)
    d_tws = empty(wsb)
    h = C.c_void_p()
    rc = lib.mh_dev_model_set_train(ptr(d_data), ptr(d_off), nst, int(data.size), 1, w.prev0, ptr(d_tws), wsb, sp, C.byref(h))
    assert rc == 0, "mh_dev_model_set_train"
    trained = mhc.ModelSet(h)
    assert trained.table_bytes() == tables, "mh_dev_model_set_train"
    # mh_dev_model_set_pick: the view of a bank of two shared models (order 1, order 0), entries taken in turn
    bank = mhc.ModelSet.from_models([m1, mhc.Model.from_counts(batch_ref.histogram(w.messages, 0, w.prev0), 0)])
    choice = (np.arange(nst) % 2).astype(np.uint32)
    d_choice = dev(choice)
    h = C.c_void_p()
    rc = lib.mh_dev_model_set_pick(bank.handle, ptr(d_choice), nst, sp, C.byref(h))
    assert rc == 0, "mh_dev_model_set_pick"
    view = mhc.ModelSet(h)
    assert len(view) == nst and [view.stream_info(i)[0] for i in range(4)] == [1, 0, 1, 0], "mh_dev_model_set_pick"

    # mh_dev_bank_train: three shared models for those messages; the host form (its own run of the same training) gives the same
    # bank, choices and iteration count, and the choices are batch_ref's selection under the bank's own tables
    k, iters = 3, C.c_int(0)
    wsb = lib.mh_dev_bank_train_workspace(nst, int(data.size), k)
    d_bws, d_ch = empty(wsb), empty(nst * 4)
    h = C.c_void_p()
    rc = lib.mh_dev_bank_train(ptr(d_data), ptr(d_off), nst, int(data.size), 1, w.prev0, k, 4, ptr(d_ch), C.byref(iters), ptr(d_bws), wsb, sp, C.byref(h))
    assert rc == 0, "mh_dev_bank_train"
    trained_bank = mhc.ModelSet(h)
    got_choice = d_ch.cpu().numpy().view(np.uint32)[:nst]
    host_bank, host_choice, host_iters = mhc.ModelSet.train_bank(w.messages, k, order=1, max_iters=4, prev0=w.prev0, host=True)
    tabs = trained_bank.table_bytes()
    assert tabs == host_bank.table_bytes() and same(got_choice, host_choice) and iters.value == host_iters, "mh_dev_bank_train"
    entries = [(1, mh_oracle.Model.from_table(t).codes()[0].astype(np.int64)) for t in tabs]
    assert same(got_choice, batch_ref.select(entries, w.messages, w.prev0)[0]), "mh_dev_bank_train: choices against the selection rule"
