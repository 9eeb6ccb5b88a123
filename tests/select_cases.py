"""The shapes of the select tests (tests/test_select_abi.py for the host form, tests/test_gpu_select.py for the device call):
small batches packed by tests/batch_ref.py, pick lists, and the comparison of what a call wrote with tests/select_ref.py.
A helper module: numpy, batch_ref and select_ref only, never the library (the binding is handed in).

The smallest shapes at which the gather can go wrong: payloads of 0, 1, 2, 3, 15, 16, 17, 1023, 1024 and 1025 bytes (the lane
word and the wave window, each one less, exact and one more) and one of 70 001 bytes (many windows), runs of 1 .. 3-byte
payloads (a 16-byte output word with up to six owners), every pair of source and output offset modulo 16, two and eight
sources, an order-2 index, a model per stream, chunks 256 and 1024 with streams of 0, 1, chunk - 1, chunk and chunk + 1
symbols.  Under the `flat` table (order 0, 256 equal counts: every code has 8 bits) a message of k bytes has a payload of k
bytes, which is how the byte lengths are hit; the other tables give bit counts that are no multiple of 8."""
import copy
import functools

import numpy as np

import batch_ref
import select_ref

PREV0 = batch_ref.PREV0
FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
BYTE_LENGTHS = (0, 1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 70001)


class Case:
    """name, lists (the messages of every source), packs (their batch_ref.Packed), chunk, picks (name -> pick list)."""

    def sources(self, index=True, sym=True):
        """The (payload, pay_off, nbits, sym_off, index, chunk) tuples the binding's select wrappers take."""
        return [(q.payload, q.pay_off, q.nbits, q.sym_off if sym else None, q.index_array(self.chunk) if index and sym else None,
                 self.chunk if index and sym else 0) for q in self.packs]


def _draw(rng, k, alphabet=256, skew=0.0):
    if not skew:
        return rng.integers(0, alphabet, k).astype(np.uint8).tobytes()
    w = 1.0 / np.arange(1, alphabet + 1) ** skew
    return rng.choice(alphabet, size=k, p=w / w.sum()).astype(np.uint8).tobytes()


def _standard_picks(rng, sizes):
    every = [select_ref.pick(s, i) for s, n in enumerate(sizes) for i in range(n)]
    mid = len(every) // 2
    return {"identity": every, "reverse": every[::-1], "each twice": [p for p in every for _ in range(2)],
            "none in the middle and trailing": every[:mid] + [select_ref.NONE] * 3 + every[mid:] + [select_ref.NONE] * 2,
            "all none": [select_ref.NONE] * 5, "no pick": [],
            "random": [every[k] for k in rng.integers(0, len(every), len(every) + 7)]}


def _case(name, lists, packs, chunk, picks):
    c = Case()
    c.name, c.lists, c.packs, c.chunk, c.picks = name, lists, packs, chunk, picks
    return c


@functools.lru_cache(maxsize=None)
def flat_codes():
    return batch_ref.oracle_codes(np.ones(256, dtype=np.uint64), 0)


def _lengths():
    rng = np.random.default_rng(11)
    lens = list(BYTE_LENGTHS) + [1 + k % 3 for k in range(40)] + [2, 0, 3, 0, 0, 1]
    msgs = [_draw(rng, k) for k in lens]
    q = batch_ref.pack(msgs, *flat_codes(), 0, PREV0, 256)
    assert np.diff(q.pay_off.astype(np.int64)).tolist() == lens                  # the flat table: a byte per symbol
    return _case("byte lengths", [msgs], [q], 256, _standard_picks(rng, [len(msgs)]))


def _phases():
    """Streams of 33 .. 80 bytes among 1 .. 3-byte ones, picked until every (source offset, output offset) pair modulo 16 has
    been a stream of more than two lane words."""
    rng = np.random.default_rng(12)
    lens = [int(rng.integers(33, 81)) if k % 2 else int(rng.integers(1, 4)) for k in range(96)]
    msgs = [_draw(rng, k) for k in lens]
    q = batch_ref.pack(msgs, *flat_codes(), 0, PREV0, 256)
    picks, seen, at = [], set(), 0
    while len(seen) < 256 and len(picks) < 20000:
        i = int(rng.integers(0, len(msgs)))
        picks.append(select_ref.pick(0, i))
        if lens[i] >= 33:
            seen.add((int(q.pay_off[i]) % 16, at % 16))
        at += lens[i]
    assert len(seen) == 256, len(seen)
    return _case("every offset pair modulo 16", [msgs], [q], 256, {"phases": picks})


def _chunk_lengths(rng, chunk, extra):
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 5] + [int(k) for k in rng.integers(0, 2 * chunk, extra)]
    rng.shuffle(lens)
    return lens


def _shared(name, seed, order, chunk, n_sources, extra):
    rng = np.random.default_rng(seed)
    lists = [[_draw(rng, k, 48, 1.1) for k in _chunk_lengths(rng, chunk, extra)] for _ in range(n_sources)]
    codes = batch_ref.oracle_codes(batch_ref.histogram([m for l in lists for m in l], order, PREV0), order)
    packs = [batch_ref.pack(l, *codes, order, PREV0, chunk) for l in lists]
    c = _case(name, lists, packs, chunk, _standard_picks(rng, [len(l) for l in lists]))
    c.order, c.codes = order, codes
    return c


def _each():
    rng = np.random.default_rng(16)
    lists = [[_draw(rng, k, 30, 1.3) for k in _chunk_lengths(rng, 1024, 2)] for _ in range(2)]
    packs = [batch_ref.pack_each(l, 1, PREV0, 1024)[0] for l in lists]
    return _case("a model per stream", lists, packs, 1024, _standard_picks(rng, [len(l) for l in lists]))


def records(n, seed):
    """n short text-like records; about half hold the word `GPU`."""
    rng = np.random.default_rng(seed)
    words = [b"the", b"of", b"and", b"to", b"in", b"a", b"is", b"that", b"for", b"it", b"as", b"was", b"with", b"be", b"The", b"stream"]
    out = []
    for i in range(n):
        k = int(rng.integers(0, 120)) if i % 9 else (0, 1, 255, 256, 257, 700, 1024, 1500, 30)[i // 9 % 9]
        ws = [words[j] for j in rng.integers(0, len(words), k)]
        if rng.random() < 0.5 and ws:
            ws[int(rng.integers(0, len(ws)))] = b"GPU"
        out.append(b" ".join(ws))
    return out


def refused_picks(c):
    """A pick list with an out-of-range source, an out-of-range stream and (once `spoiled` has raised nbits of stream 2) a stream
    whose bits do not fit its bytes, between good picks."""
    n = len(c.lists[0])
    return [select_ref.pick(0, 1), select_ref.pick(len(c.lists), 0), select_ref.pick(0, 3), select_ref.pick(0, n), select_ref.pick(0, 2),
            select_ref.pick(0, 4), select_ref.pick(select_ref.MAX_SOURCES, 1), select_ref.pick(0, 0)]


def spoiled(c):
    """The case with nbits of stream 2 of its first source one bit past the stream's payload bytes: (sources for the binding's
    wrappers, packs for the reference).  The case itself is not changed."""
    q = copy.copy(c.packs[0])
    q.nbits = q.nbits.copy()
    q.nbits[2] = (int(q.pay_off[3]) - int(q.pay_off[2])) * 8 + 1
    src = c.sources()
    src[0] = (src[0][0], src[0][1], q.nbits) + src[0][3:]
    return src, [q] + c.packs[1:]


BUILDERS = {
    "byte lengths": _lengths,
    "every offset pair modulo 16": _phases,
    "two sources, order 1, chunk 1024": lambda: _shared("two sources, order 1, chunk 1024", 13, 1, 1024, 2, 4),
    "eight sources, order 0, chunk 256": lambda: _shared("eight sources, order 0, chunk 256", 14, 0, 256, 8, 1),
    "order 2, chunk 256": lambda: _shared("order 2, chunk 256", 15, 2, 256, 1, 5),
    "a model per stream": _each,
}
NAMES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once and shared; nothing changes a case."""
    return BUILDERS[name]()


def differences(r, want, chunk, what, index=True, sym=True, count_only=False, fill=FILL):
    """What a select call wrote (the binding's Selected, buffers prefilled with `fill`) against select_ref.select's `want`:
    a list of the differences.  Exact: offsets, bit counts, symbol offsets, statuses, every payload byte, every byte behind the
    payload and every index entry, gaps and the words behind the index included."""
    bad = []
    fill64 = int.from_bytes(bytes([fill]) * 8, "little")
    n, total = len(want.nbits), int(want.pay_off[-1])
    if not np.array_equal(r.out_off, want.pay_off):
        bad.append("out_off")
    if not np.array_equal(r.nbits, want.nbits):
        bad.append("out_nbits")
    if not np.array_equal(r.pick_status, want.status):
        bad.append("pick_status %s" % r.pick_status.tolist())
    if sym and not np.array_equal(r.sym_off, want.sym_off):
        bad.append("out_sym_off")
    if not count_only:
        if not np.array_equal(r.payload[:total], want.payload):
            bad.append("payload: first difference at byte %d of %d" % (int(np.nonzero(r.payload[:total] != want.payload)[0][0]), total))
        if not (r.payload[total:] == fill).all():
            bad.append("bytes written behind the payload, first at %d (payload %d)" % (total + int(np.nonzero(r.payload[total:] != fill)[0][0]), total))
    if index and sym:
        exp = np.full(r.index.size, fill64, dtype=np.uint64)
        for j, sl in enumerate(want.slices):
            b = int(want.sym_off[j]) // chunk + j
            exp[b:b + sl.size] = sl
        assert int(want.sym_off[n]) // chunk + n + 1 <= r.index_cap
        if not np.array_equal(r.index, exp):
            bad.append("index: first difference at entry %d" % int(np.nonzero(r.index != exp)[0][0]))
    expect = select_ref.MH_ERR_ARG if want.status.any() else select_ref.MH_OK
    if r.status != expect:
        bad.append("status %d, expected %d" % (r.status, expect))
    return ["%s: %s" % (what, b) for b in bad]
