"""Generator and references of the batch-family fuzz (tests/test_batch_ref.py, tests/test_gpu_batch_fuzz.py): seeded small
batches, and what every batch call of include/mh.h must give for them, from the CPU oracle's code tables and plain numpy on
the original messages (a helper module like find_ref.py and recode_ref.py; it imports numpy and the oracle, never the library).

A case is drawn in two steps: draw_cases(seed) fixes every case's parameters (and its own seed) from one generator, and
Case.world() builds the messages, patterns, lookups and model counts of one case when a test needs them.  Case.edits() is a
second such part, from a generator of its own: a dictionary, a span list, a byte map and two replacements for dictionary
search, span merging, masked and splicing re-code (find_ref.py, edit_ref.py, splice_ref.py), and Case.expected() what the
edit and the splices must give.  Case.table() is a third, again from a generator of its own: a replacement table, the span
list with a tag per span and insertions put in by craft, and the tagged merge of the dictionary's hits (splice_table_ref.py);
Case.expected_table() is what the table splice must give.  Both expectations come under the case's destination and under a
covering one, trained on the originals and on every edited form, under which nothing is dropped."""
import bisect
import functools

import numpy as np

import edit_ref
import find_ref
import splice_ref
import splice_table_ref
from oracle import mh_oracle as oracle

PREV0 = 0x20
STREAM_COUNTS = (1, 2, 3, 63, 64, 65, 257, 1000)
CHUNKS = (256, 512, 1024, 2048, 4096, 8192)
SOURCES = ("uniform", "zipf", "runs", "markov", "two", "one", "text")
CASE_BYTES = 256 << 10            # cap of one case's messages
DEEP_BYTES = 32 << 10             # cap of a case with a deep model (codes of up to 61 bits)
MAX_STREAM = 20000
BANK_NONE = 0xFFFFFFFF
N_CONTEXTS = {0: 1, 1: 256, 2: 65536}
SEED = 20261017


# ---------------------------------------------------------------------------------------------------- contexts and keys
def concat(messages):
    """(all symbols int64, in_off int64[n + 1]) of a list of byte strings."""
    off = np.zeros(len(messages) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(m) for m in messages])
    return np.frombuffer(b"".join(bytes(m) for m in messages), dtype=np.uint8).astype(np.int64), off


def contexts(d, off, order, prev0):
    """The context of every symbol of a batch (include/mh.h): 0 (order 0), the byte in front (order 1; prev0 in front of every
    stream) or (byte two in front) << 8 | byte in front (order 2; prev0 stands for both bytes in front of a stream)."""
    if order == 0 or d.size == 0:
        return np.zeros(d.size, dtype=np.int64)
    ln = np.diff(off)
    first = off[:-1][ln > 0]
    p1 = np.concatenate([[prev0], d[:-1]])
    p1[first] = prev0
    if order == 1:
        return p1
    p2 = np.concatenate([[prev0, prev0], d[:-2]])[:d.size]
    p2[first] = prev0
    p2[off[:-1][ln > 1] + 1] = prev0
    return (p2 << 8) | p1


def keys(messages, order, prev0=PREV0):
    d, off = concat(messages)
    return contexts(d, off, order, prev0) * 256 + d, off


def histogram(messages, order, prev0=PREV0):
    """Summed counts[context * 256 + symbol] of independent messages: 256, 65 536 or 1 << 24 uint64."""
    k, _ = keys(messages, order, prev0)
    return np.bincount(k, minlength=256 * N_CONTEXTS[order]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------- code tables
def oracle_codes(counts, order):
    """(len int64, code uint64) per context * 256 + symbol of the oracle's model of these counts; 0 bits = no code."""
    m = oracle.Model.from_counts(counts, order)
    lens, codes = m.codes_o2() if order == 2 else m.codes()
    n = 256 * N_CONTEXTS[order]
    return lens[:n].astype(np.int64), codes[:n].copy()


def _package_merge(row, limit):
    """Lengths of the optimal code of at most `limit` bits: leaves by (count, symbol); on equal weight a
    leaf precedes a package and packages keep their order."""
    leaves = sorted((int(c), s) for s, c in enumerate(row) if c)
    n = len(leaves)
    level = [(w, (s,)) for w, s in leaves]
    for _ in range(limit - 1):
        packs = [(level[i][0] + level[i + 1][0], level[i][1] + level[i + 1][1]) for i in range(0, len(level) - 1, 2)]
        level = sorted([(w, (s,)) for w, s in leaves] + packs, key=lambda t: t[0])[:2 * n - 2]
    out = {}
    for _, syms in level:
        for s in syms:
            out[s] = out.get(s, 0) + 1
    return out


def limited_codes(counts, order, limit):
    """oracle_codes under the rule of length-limited models: a context whose reference tree is deeper than `limit` gets
    package-merge lengths and canonical codewords (length, then symbol; the first all zero bits), the others stay."""
    lens, codes = oracle_codes(counts, order)
    rows = np.asarray(counts, dtype=np.uint64).reshape(-1, 256)
    for c in np.nonzero(lens.reshape(-1, 256).max(axis=1) > limit)[0]:
        code, last = 0, None
        lens[c * 256:(c + 1) * 256] = 0
        for l, s in sorted((l, s) for s, l in _package_merge(rows[c], limit).items()):
            code = 0 if last is None else (code + 1) << (l - last)
            lens[c * 256 + s], codes[c * 256 + s], last = l, code, l
    return lens, codes


def deep_counts(order, k, contexts_of):
    """Fibonacci-weighted counts over the symbols 0 .. k - 1 in every context of `contexts_of` (context numbers of `order`):
    ascending or descending by the parity of the context's bytes, so the longest code (k - 1 bits) moves about."""
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(256 * N_CONTEXTS[order], dtype=np.uint64)
    for ctx in contexts_of:
        counts[ctx * 256:ctx * 256 + k] = fib[::-1] if ((ctx & 255) + (ctx >> 8)) % 2 else fib
    return counts


# ---------------------------------------------------------------------------------------------------- the packer
class Packed:
    """What encoding `messages` under a code table gives: payload uint8, pay_off / nbits / dropped / sym_off uint64, the index
    slices (one uint64 array per stream) and `used`, the code length of every symbol (0: dropped)."""

    def index_array(self, chunk):
        """The batch index: slice i at sym_off[i] / chunk + i, 0 in the gaps, total / chunk + n + 1 entries."""
        n = len(self.slices)
        idx = np.zeros(int(self.sym_off[n]) // chunk + n + 1, dtype=np.uint64)
        for i, sl in enumerate(self.slices):
            b = int(self.sym_off[i]) // chunk + i
            idx[b:b + sl.size] = sl
        return idx

    def slices_of(self, idx, chunk):
        """The slices of a batch index array, concatenated (what lies in the gaps is not compared)."""
        out = [np.asarray(idx[int(self.sym_off[i]) // chunk + i:][:sl.size], dtype=np.uint64) for i, sl in enumerate(self.slices)]
        return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)

    def all_slices(self):
        return np.concatenate(self.slices) if self.slices else np.zeros(0, dtype=np.uint64)


def pack(messages, lens, codes, order, prev0=PREV0, chunk=0):
    """The vectorised bit packer.  A symbol without a code is skipped and counted, and the context advances (the reference's
    NDEBUG rule, recode_ref.py); codes go MSB first, streams are packed byte-aligned; index entries are (context in front of the
    chunk) << 56 | bit offset in the stream's own payload (recode_ref.index_slice), order 2: (two context bytes) << 48."""
    d, off = concat(messages)
    n = len(messages)
    ctx = contexts(d, off, order, prev0)
    L = np.asarray(lens, dtype=np.int64)[ctx * 256 + d]
    cs = np.concatenate([[0], np.cumsum(L)])
    nbits = cs[off[1:]] - cs[off[:-1]]
    pay_off = np.concatenate([[0], np.cumsum((nbits + 7) // 8)])
    stream = np.repeat(np.arange(n), np.diff(off))
    rel = cs[:-1] - cs[off[:-1]][stream]                         # bit offset of every symbol in its stream's payload
    at = pay_off[:-1][stream] * 8 + rel
    sym = np.repeat(np.arange(d.size), L)
    k = np.arange(int(cs[-1])) - np.repeat(cs[:-1], L)           # bit number inside the code, 0 = first written
    c = np.asarray(codes, dtype=np.uint64)[ctx * 256 + d]
    bits = np.zeros(int(pay_off[-1]) * 8, dtype=np.uint8)
    bits[at[sym] + k] = (c[sym] >> (L[sym] - 1 - k).astype(np.uint64)) & np.uint64(1)
    p = Packed()
    p.payload = np.packbits(bits)
    p.pay_off, p.nbits, p.sym_off = pay_off.astype(np.uint64), nbits.astype(np.uint64), off.astype(np.uint64)
    zero = np.concatenate([[0], np.cumsum(L == 0)])
    p.dropped = (zero[off[1:]] - zero[off[:-1]]).astype(np.uint64)
    p.used = L
    p.slices = []
    if chunk:
        before = contexts(d, off, max(order, 1), prev0)          # (an order-0 entry carries the byte in front as well)
        shift = np.uint64(48 if order == 2 else 56)
        entry = (before.astype(np.uint64) << shift) | rel.astype(np.uint64)
        p.slices = [entry[off[i]:off[i + 1]:chunk] for i in range(n)]
    return p


def merge(packs):
    """Packed of several one-after-the-other batches as one batch (every stream under a model of its own)."""
    p = Packed()
    p.payload = np.concatenate([q.payload for q in packs] + [np.zeros(0, dtype=np.uint8)])
    scan = lambda parts: np.concatenate([[0], np.cumsum(np.concatenate(parts + [np.zeros(0, dtype=np.uint64)]).astype(np.int64))]).astype(np.uint64)
    p.pay_off, p.sym_off = scan([np.diff(q.pay_off) for q in packs]), scan([np.diff(q.sym_off) for q in packs])
    p.nbits = np.concatenate([q.nbits for q in packs] + [np.zeros(0, dtype=np.uint64)])
    p.dropped = np.concatenate([q.dropped for q in packs] + [np.zeros(0, dtype=np.uint64)])
    p.slices = [sl for q in packs for sl in q.slices]
    return p


def pack_each(messages, order, prev0=PREV0, chunk=0):
    """Every message under the oracle's model of its own histogram: (Packed of the batch, [table file per message])."""
    packs, tables = [], []
    for m in messages:
        counts = histogram([m], order, prev0)
        tables.append(oracle.Model.from_counts(counts, order).table_bytes())
        packs.append(pack([m], *oracle_codes(counts, order), order, prev0, chunk))
    return merge(packs), tables


TAIL_LENS = (0, 1, 15, 16, 1025)   # an empty stream, one lane, a lane boundary, one byte past a 1 KiB unit


def tail_batches(packer, draw):
    """Four batches of five streams of TAIL_LENS bytes whose packed payloads are 0, 1, 2 and 3 bytes long modulo 4 (the
    encoders write whole dwords and finish the last, partial one apart): [(messages, Packed)].  packer(messages) is the
    reference Packed, draw(n, seed) gives n bytes; the last stream is drawn again until the total has the wanted remainder."""
    out = []
    for r in range(4):
        head = [draw(k, 100 + 10 * r + i) for i, k in enumerate(TAIL_LENS[:-1])]
        for seed in range(200):
            msgs = head + [draw(TAIL_LENS[-1], 1000 * (r + 1) + seed)]
            ref = packer(msgs)
            if int(ref.pay_off[-1]) % 4 == r:
                break
        assert int(ref.pay_off[-1]) % 4 == r and [len(m) for m in msgs] == list(TAIL_LENS)
        out.append((msgs, ref))
    return out


def check_tail_and_capacity(mhc, encode, workspace, handle, msgs, ref, what):
    """For the GPU tests of the three batch encoders (mhc: the binding, handed in; this module never imports it).
    One device encode call of the batch family (encode / workspace: the mh_dev_encode_* pair, handle: its model or set) on
    msgs, whose packed form is ref (batch_ref.Packed).  With cap exactly the payload size: MH_OK, the reference's bytes, offsets
    and bit counts, and the 64 bytes behind cap untouched.  With cap one byte short: MH_ERR_CAPACITY and nothing written at
    or beyond cap."""
    lib = mhc.lib()
    dev = lambda a: mhc.DeviceBuffer(max(a.nbytes, 16), np.ascontiguousarray(a) if a.nbytes else None)
    data, in_off = mhc.batch_offsets(msgs)
    n, total, pbytes = len(msgs), int(data.size), int(ref.pay_off[-1])
    GUARD = 0xA5
    d_data, d_in = dev(data), dev(in_off)
    wsb = workspace(n, total)
    for cap, want in ((pbytes, mhc.MH_OK), (pbytes - 1, mhc.MH_ERR_CAPACITY)):
        d_out = dev(np.full(pbytes + 64, GUARD, dtype=np.uint8))
        d_oo, d_nb, d_ws = mhc.DeviceBuffer((n + 1) * 8), mhc.DeviceBuffer(n * 8), mhc.DeviceBuffer(wsb)
        assert encode(handle, d_data.ptr, d_in.ptr, n, total, 0x20, d_out.ptr, cap, d_oo.ptr, d_nb.ptr, None, 0, d_ws.ptr, wsb, None) == 0, what
        assert lib.mh_dev_status(d_ws.ptr, None) == want, "%s: cap %d of %d" % (what, cap, pbytes)
        out = d_out.download()
        assert (out[cap:] == GUARD).all(), "%s: bytes written at or beyond cap %d of %d" % (what, cap, pbytes)
        if want == mhc.MH_OK:
            assert np.array_equal(out[:pbytes], ref.payload), what
            assert np.array_equal(d_oo.download(np.uint64), ref.pay_off) and np.array_equal(d_nb.download(np.uint64)[:n], ref.nbits), what


def select(tables, messages, prev0=PREV0):
    """Bank selection: tables = [(order, lens)] per entry.  (choice uint32[n], nbits uint64[n]): the entry that has a code for
    every pair of the stream and gives the fewest bits, ties to the lowest entry; an empty stream: entry 0; none: BANK_NONE
    and UINT64_MAX."""
    n = len(messages)
    best = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    choice = np.full(n, BANK_NONE, dtype=np.uint32)
    for e, (order, lens) in enumerate(tables):
        k, off = keys(messages, order, prev0)
        L = np.asarray(lens, dtype=np.int64)[k]
        cs, zero = np.concatenate([[0], np.cumsum(L)]), np.concatenate([[0], np.cumsum(L == 0)])
        bits, missing = cs[off[1:]] - cs[off[:-1]], zero[off[1:]] - zero[off[:-1]]
        better = (missing == 0) & (bits < best)
        best[better], choice[better] = bits[better], e
    return choice, np.where(choice == BANK_NONE, np.uint64(0xFFFFFFFFFFFFFFFF), best.astype(np.uint64))


# ---------------------------------------------------------------------------------------------------- sources
_WORDS = [b"the", b"of", b"and", b"to", b"in", b"a", b"is", b"that", b"for", b"it", b"as", b"was", b"with", b"be", b"The", b"GPU"]


def draw_source(rng, kind, n, k):
    """n symbols of a source of the kinds of test_gpu_differential.draw_source, over k symbol values where that applies."""
    if kind == "uniform":
        d = rng.integers(0, k, size=n)
    elif kind == "zipf":
        w = 1.0 / np.arange(1, k + 1) ** float(rng.uniform(0.7, 2.5))
        d = rng.permutation(256)[:k][rng.choice(k, size=n, p=w / w.sum())]
    elif kind == "runs":
        ln = rng.geometric(0.05, size=n // 8 + 2)
        d = np.repeat(rng.integers(0, k, size=ln.size), ln)[:n]
        d = np.concatenate([d, np.zeros(n - d.size, dtype=d.dtype)])
    elif kind == "markov":                                       # every symbol has two likely successors
        nxt = rng.integers(0, k, size=(k, 2)).tolist()
        coin, jump = rng.random(n).tolist(), rng.integers(0, k, size=n).tolist()
        d, s = [0] * n, 0
        for i in range(n):
            s = nxt[s][0] if coin[i] < 0.6 else nxt[s][1] if coin[i] < 0.95 else jump[i]
            d[i] = s
    elif kind == "two":
        d = rng.integers(0, 2, size=n) * 255
    elif kind == "one":
        d = np.full(n, int(rng.integers(0, 256)))
    else:
        out = bytearray()
        while len(out) < n:
            out += _WORDS[int(rng.integers(len(_WORDS)))] + (b".\n" if rng.random() < 0.07 else b" ")
        d = np.frombuffer(bytes(out[:n]), dtype=np.uint8)
    return np.asarray(d, dtype=np.int64).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- cases
class World:
    """One case, built: messages, prev0, patterns, fold, lookups and the counts that the source and destination models (and the
    bank's entries) are trained on."""


class Case:
    def __init__(self, index, rng, orders, src_kind, dst_kind):
        self.index, self.orders, self.src_kind, self.dst_kind = index, orders, src_kind, dst_kind
        self.source = str(rng.choice(SOURCES))
        self.chunk = int(rng.choice(CHUNKS))
        self.n_streams = int(rng.choice(STREAM_COUNTS))
        self.live_prev0 = bool(rng.random() < 0.25)
        self.fold = bool(rng.random() < 0.25)
        self.limit = {k: int(rng.choice([8, 12])) for k in ("src", "dst")}
        self.alphabet = int(rng.choice([36, 44, 58, 60, 62]))      # deep: the longest code has alphabet - 1 bits
        self.seam_first = bool(rng.random() < 0.5)
        self.seed = int(rng.integers(1 << 62))
        self.deep = "deep" in (src_kind, dst_kind)

    @property
    def id(self):
        return "%03d-%s-%s%d-%s%d-c%d-n%d" % (self.index, self.source, self.src_kind, self.orders[0], self.dst_kind, self.orders[1],
                                              self.chunk, self.n_streams)

    def lengths(self, rng):
        c, n = self.chunk, self.n_streams
        budget = DEEP_BYTES if self.deep else int(min(CASE_BYTES, max(4 * c + 8, np.exp(rng.uniform(np.log(4096), np.log(CASE_BYTES))))))
        if self.source in ("one", "two"):                        # (every short pattern hits everywhere: fewer bytes, as many edges)
            budget = min(budget, max(4 * c + 8, 16 << 10))
        seams = [c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1]
        ln = [int(rng.choice([c, 2 * c]))] if self.seam_first else [int(rng.choice(seams[2:]))]
        left = budget - max(ln[0], 2 * c)
        for _ in range(n - 1):
            u = rng.random()
            want = int(rng.integers(0, 4)) if u < 0.3 else int(rng.choice(seams)) if u < 0.55 else \
                int(min(MAX_STREAM, np.exp(rng.uniform(0, np.log(MAX_STREAM)))))
            if want > left:                                       # the cap binds: the short lengths remain
                want = min(int(rng.integers(0, 4)), left)
            ln.append(want)
            left -= want
        if max(ln) <= c:                                          # a seam needs a stream longer than the chunk
            ln[0] = 2 * c
        return [ln[i] for i in rng.permutation(len(ln))]

    @functools.lru_cache(maxsize=2)
    def world(self):
        rng = np.random.default_rng(self.seed)
        w = World()
        ln = self.lengths(rng)
        k = self.alphabet if self.deep else int(rng.choice([2, 3, 5, 17, 64, 200, 256]))
        d = draw_source(rng, self.source, sum(ln), k)
        off = np.concatenate([[0], np.cumsum(ln)])
        if self.deep:                                             # the rarest symbol of either weighting opens every other chunk
            d = d % np.uint8(k)
            for i in range(len(ln)):
                d[off[i] + self.chunk:off[i + 1]:2 * self.chunk] = 0
                d[off[i] + 2 * self.chunk:off[i + 1]:2 * self.chunk] = k - 1
        raw = d.tobytes()
        w.messages = [raw[off[i]:off[i + 1]] for i in range(len(ln))]
        w.prev0 = int(d[int(rng.integers(d.size))]) if self.live_prev0 else PREV0
        w.chunk, w.fold = self.chunk, self.fold
        other = draw_source(rng, self.source, max(sum(ln) // 2, 64), k)                      # the foreign model's training text
        w.foreign = [(other % np.uint8(k) if self.deep else other).tobytes()]
        self._patterns(rng, w)
        self._lookups(rng, w)
        return w

    def counts(self, which):
        """(counts, max_len) of the source ('src') or destination ('dst') model."""
        w = self.world()
        order = self.orders[0 if which == "src" else 1]
        kind = self.src_kind if which == "src" else self.dst_kind
        if kind == "deep":
            d, off = concat(w.messages)
            live = np.unique(np.concatenate([contexts(d, off, order, w.prev0), contexts(*concat(w.foreign), order, w.prev0)]))
            return deep_counts(order, self.alphabet, live.tolist()), 0
        if kind == "foreign":
            return histogram(w.foreign, order, w.prev0), 0
        return histogram(w.messages, order, w.prev0), self.limit[which] if kind == "limited" else 0

    @functools.lru_cache(maxsize=4)
    def codes(self, which):
        counts, limit = self.counts(which)
        order = self.orders[0 if which == "src" else 1]
        return limited_codes(counts, order, limit) if limit else oracle_codes(counts, order)

    def _patterns(self, rng, w):
        """1 to 15 substrings of the messages, 64 bytes at most: one across a chunk seam, one up to a stream's last byte, one that
        occurs nowhere (a one-symbol source: a byte it lacks), the rest anywhere."""
        c, msgs = self.chunk, w.messages
        long = [i for i, m in enumerate(msgs) if len(m) > c]
        i = long[int(rng.integers(len(long)))]
        seam = c * int(rng.integers(1, (len(msgs[i]) - 1) // c + 1))
        a = int(rng.integers(1, 7))
        pats = [msgs[i][seam - a:min(seam + int(rng.integers(1, 7)), len(msgs[i]))]]
        full = [m for m in msgs if m]
        m = full[int(rng.integers(len(full)))]
        pats.append(m[-int(rng.integers(1, min(len(m), 6) + 1)):])
        have = find_ref.fold_ascii(b"\0".join(msgs)) if self.fold else b"\0".join(msgs)
        while True:
            p = bytes(rng.integers(1, 256, size=int(rng.integers(1, 4)), dtype=np.uint8))
            if (find_ref.fold_ascii(p) if self.fold else p) not in have:
                break
        pats.append(p)
        room, hits = 64 - sum(len(p) for p in pats), 0
        for _ in range(int(rng.integers(0, 13))):
            m = full[int(rng.integers(len(full)))]
            a = int(rng.integers(len(m)))
            p = m[a:a + int(rng.integers(1, 10))]
            hits += have.count(find_ref.fold_ascii(p) if self.fold else p)
            if len(p) <= room and hits <= 20000:                  # (a byte of a two-symbol source is half the batch)
                pats.append(p)
                room -= len(p)
        if self.fold:
            pats = [p.swapcase() if j % 2 else p for j, p in enumerate(pats)]
        w.patterns = [pats[j] for j in rng.permutation(len(pats))]

    def _lookups(self, rng, w):
        """32 lookups (stream, begin, end): empty ones, whole streams, one and two seams crossed, up to the stream's end, and
        [0, 0) of an empty stream where there is one."""
        c, ln = self.chunk, [len(m) for m in w.messages]
        full = [i for i, l in enumerate(ln) if l]
        long = [i for i, l in enumerate(ln) if l > c]
        longer = [i for i, l in enumerate(ln) if l > 2 * c]
        empty = [i for i, l in enumerate(ln) if l == 0]
        pick = lambda xs: xs[int(rng.integers(len(xs)))]
        lk = []
        i = pick(long)
        lk += [(i, c - 1, c + 1), (i, max(c - 40, 0), min(c + 40, ln[i])), (i, c, ln[i]), (i, 0, ln[i]), (i, ln[i], ln[i])]
        if longer:
            i = pick(longer)
            lk += [(i, c - 1, 2 * c + 1), (i, c, 2 * c), (i, 0, ln[i])]
        if empty:
            lk += [(pick(empty), 0, 0)]
        while len(lk) < 32:
            i = pick(full)
            u, b = rng.random(), int(rng.integers(ln[i] + 1))
            e = b if u < 0.15 else ln[i] if u < 0.4 else min(ln[i], b + int(np.exp(rng.uniform(0, np.log(4 * c)))))
            lk.append((i, 0, ln[i]) if u > 0.9 else (i, b, e))
        w.lookups = [lk[j] for j in rng.permutation(32)]
        w.lookup_bytes = [w.messages[i][b:e] for i, b, e in w.lookups]

    # ---- the second part of a case: a dictionary, a span list, a byte map and two replacements ----
    @functools.lru_cache(maxsize=2)
    def edits(self):
        """The inputs of dictionary search, span merging, masked and splicing re-code, from the messages alone.  A generator of
        its own, seeded from the case's seed: no draw of world() moves."""
        rng = np.random.default_rng([self.seed, 1])
        w, e = self.world(), Edits()
        e.fold = w.fold
        _draw_dictionary(rng, self, w, e)
        e.states, e.classes = trie_counts(e.dictionary, e.fold)
        e.hits = find_ref.find_hits(w.messages, e.dictionary, fold=e.fold)
        e.hit_off, e.records, e.hit_pattern = find_ref.hit_arrays(e.hits, len(w.messages))
        _draw_replacements(rng, w, e)
        _draw_spans(rng, self, w, e)
        _draw_map(rng, self, w, e)
        return e

    @functools.lru_cache(maxsize=2)
    def expected(self):
        """What the masked and the splicing re-code must give under the destination model: the packer on the edited messages.
        A case with an order-2 side: the edit under the covering destination as well."""
        w, e, x = self.world(), self.edits(), Expected()
        do = self.orders[1]
        put = lambda msgs: pack(msgs, *self.codes("dst"), do, w.prev0, self.chunk)
        x.edited, x.edited_all, x.spliced = self._edited()
        x.edit, x.edit_all = put(x.edited), put(x.edited_all)
        x.splice = [put(y) for y in x.spliced]
        x.out_sym_off = [splice_ref.offsets(y) for y in x.spliced]
        if 2 in self.orders:
            x.edit_cover, x.edit_all_cover = self.put_cover(x.edited), self.put_cover(x.edited_all)
        return x

    def _edited(self):
        """(the masked messages, the messages masked everywhere, [the messages with every span deleted, ... replaced])."""
        w, e = self.world(), self.edits()
        return (edit_ref.apply(w.messages, e.span_off, e.spans, e.byte_map), edit_ref.apply(w.messages, None, None, e.byte_map),
                [splice_ref.apply(w.messages, e.span_off, e.spans, rep) for rep in e.reps])

    # ---- the third part of a case: a replacement table, a tagged span list with insertions, the tagged merge ----
    @functools.lru_cache(maxsize=2)
    def table(self):
        """The inputs of the tagged span merge and the table splice.  A generator of its own, seeded from the case's seed: no draw
        of world() or edits() moves."""
        rng = np.random.default_rng([self.seed, 2])
        w, e, t = self.world(), self.edits(), Table()
        _draw_table(rng, w, e, t)
        _draw_tagged(rng, self, w, e, t)
        t.merged = splice_table_ref.merge_tagged(e.hit_off, e.records, e.hit_pattern)
        return t

    def _table_spliced(self):
        t = self.table()
        return splice_table_ref.apply(self.world().messages, t.span_off, t.spans, t.tags, t.reps)

    @functools.lru_cache(maxsize=2)
    def cover_counts(self):
        """The counts of the covering destination: the originals and every edited form of the case (masked, masked everywhere,
        both splices, the table splice) under the destination's order."""
        w = self.world()
        edited, edited_all, spliced = self._edited()
        return histogram(w.messages + edited + edited_all + spliced[0] + spliced[1] + self._table_spliced(), self.orders[1], w.prev0)

    @functools.lru_cache(maxsize=2)
    def cover_codes(self):
        return oracle_codes(self.cover_counts(), self.orders[1])

    def put_cover(self, msgs):
        return pack(msgs, *self.cover_codes(), self.orders[1], self.world().prev0, self.chunk)

    @functools.lru_cache(maxsize=2)
    def expected_table(self):
        """What the table splice must give: splice_table_ref.apply on the original messages, packed under the case's destination
        and under the covering one, where no symbol is dropped."""
        w, x = self.world(), ExpectedTable()
        x.spliced = self._table_spliced()
        x.out_sym_off = splice_table_ref.offsets(x.spliced)
        x.packed = pack(x.spliced, *self.codes("dst"), self.orders[1], w.prev0, self.chunk)
        x.cover = self.put_cover(x.spliced)
        assert not x.cover.dropped.any(), "the covering destination drops a symbol"
        return x


# (source order, destination order) -> cases; every pair of orders appears, the pairs with an order-2 side less often
_PAIRS = [((0, 0), 14), ((0, 1), 16), ((1, 0), 16), ((1, 1), 18), ((0, 2), 6), ((1, 2), 9), ((2, 0), 5), ((2, 1), 6), ((2, 2), 6)]
_SRC_KINDS = ("own", "limited", "deep", "own")
_DST_KINDS = ("own", "foreign", "deep", "limited", "foreign", "own", "deep")


@functools.lru_cache(maxsize=2)
def draw_cases(seed=SEED):
    """The fixed list of cases of a seed: 64 with orders 0 / 1 on both sides and 32 with an order-2 side.  The kinds of the models
    go round fixed lists (of coprime lengths, so every combination comes up), everything else is drawn."""
    rng = np.random.default_rng(seed)
    cases = []
    for orders, count in _PAIRS:
        for j in range(count):
            sk, dk = _SRC_KINDS[j % 4], _DST_KINDS[j % 7]
            if orders[0] == 2 and sk == "limited":                 # (length-limited models are order 0 / 1)
                sk = "deep"
            if orders[1] == 2 and dk == "limited":
                dk = "deep"
            cases.append(Case(len(cases), rng, orders, sk, dk))
    return cases


# ---------------------------------------------------------------------------------------------------- dictionaries, spans, maps
HIT_CAP = 20000                    # hits of a case's dictionary, at most
SPLICED_BYTES = 1 << 20            # a case's spliced messages, at most
DICT_MAX_STATES = 32768            # include/mh.h MH_DICT_MAX_STATES (trie nodes, root included)
DICT_MAX_LEN = 255                 # include/mh.h MH_DICT_MAX_LEN, and MH_SPLICE_MAX_REP
SPAN_CAP = 1000                    # spans of a case, at most (every one may grow by a replacement of 255 bytes)
MAP_KINDS = ("identity", "mask", "fold", "permutation", "random", "lacking")
PLACEMENTS = ("from 0", "to the last byte", "past the end", "at or past the end", "touching", "over a seam", "whole chunks",
              "whole stream", "a stream without spans between two with spans")
LDS_BYTES = 163840                 # csrc/mh_find.hip, launch_find_dict: the 160 KiB of a workgroup
DICT_PER_CU = 8                    # csrc/mh_symdec_dev.hpp, Dec<Set>::PER_CU and Dec<Shared2>::PER_CU
DEC_LDS_ENTRIES = (LDS_BYTES - 1024) // 2       # csrc/mh_model.hpp
DEC_SEC_MAX_PER_CTX = 4096                      # csrc/mh_model.hpp


class Edits:
    """The second part of a case, built: dictionary (a list of patterns) and fold, the trie's states and classes, the
    dictionary's hits (find_ref's list and the three arrays of a device call), special (what the named patterns are: pattern
    numbers), span_off / spans, byte_map and map_kind, reps (the deletion and one replacement), lacking (a byte the messages
    do not hold, or None) and rep_lacks (the replacement holds it)."""


class Expected:
    """The expected outputs of a case's edit and splices: edit, edit_all (no span list: everywhere), splice[k] (batch_ref.Packed
    under the destination model), spliced[k] (the messages) and out_sym_off[k], k = 0 the deletion, 1 the replacement; edited and
    edited_all (the messages); with an order-2 side edit_cover and edit_all_cover, the edit under the covering destination."""


class Table:
    """The third part of a case, built: reps (the replacement table) and empty (the number of its empty entry), span_off /
    spans / tags (the tagged list, insertions included) and merged (span_off, spans, tags of the tagged merge of the
    dictionary's hits)."""


class ExpectedTable:
    """The expected output of a case's table splice: spliced (the messages), out_sym_off, packed (batch_ref.Packed under the
    destination model) and cover (under the covering destination)."""


def _fold(b, fold):
    return find_ref.fold_ascii(b) if fold else bytes(b)


def trie_counts(patterns, fold):
    """(states, classes) of a plain trie of the patterns: its nodes, the root included, and the distinct bytes on its edges plus
    one, the class of the bytes of no pattern (a class number is a byte: 256 distinct bytes leave none for that class, and
    nothing in it)."""
    root, states, seen = {}, 1, set()
    for p in patterns:
        node = root
        for b in _fold(p, fold):
            seen.add(b)
            if b not in node:
                node[b] = {}
                states += 1
            node = node[b]
    return states, min(len(seen) + 1, 256)


class _Counter:
    """Exact hit counts of one pattern in the messages (overlapping hits, none across two messages), up to a limit."""

    def __init__(self, messages, fold):
        self.fold, self.have = fold, _fold(b"".join(messages), fold)
        self.off = [0]
        for m in messages:
            self.off.append(self.off[-1] + len(m))

    def stream_of(self, at):
        return bisect.bisect_right(self.off, at) - 1

    def count(self, p, limit):
        """The hits of p, or some number above `limit` once there are more."""
        p = _fold(p, self.fold)
        k, at = 0, self.have.find(p)
        while at >= 0:
            if at + len(p) <= self.off[self.stream_of(at) + 1]:
                k += 1
                if k > limit:
                    break
            at = self.have.find(p, at + 1)
        return k


def _draw_dictionary(rng, case, w, e):
    """A hundred to about 2000 patterns of 1 to 255 bytes, within HIT_CAP hits and DICT_MAX_STATES states.  In this order: a
    255-byte pattern across a chunk seam, one that ends on a stream's last byte, one with all its suffixes and some of its
    prefixes (a one- or two-symbol source: the runs a, aa, ... of its bytes), patterns that occur nowhere, one duplicate,
    substrings of the messages; then shuffled.  A pattern that would take the hits over the budget is left out, the named ones
    included: a byte of a small alphabet alone hits more often than HIT_CAP, and so does any run in a one-symbol source, where
    little but the seam pattern fits.  e.special says which of the named ones are in (their pattern numbers)."""
    msgs, c, fold = w.messages, case.chunk, w.fold
    cnt = _Counter(msgs, fold)
    ln = [len(m) for m in msgs]
    full = [i for i, l in enumerate(ln) if l]
    pats, folded, special = [], set(), {}
    room = {"hits": HIT_CAP - 1000, "states": DICT_MAX_STATES - 768}

    def add(p, limit, name=None, k=None, nodes=None):
        k = cnt.count(p, min(limit, room["hits"])) if k is None else k
        nodes = len(p) if nodes is None else nodes                 # (an upper bound of the nodes it adds)
        if not p or len(p) > DICT_MAX_LEN or k > min(limit, room["hits"]) or nodes > room["states"]:
            return False
        if name:
            special[name] = len(pats)
        pats.append(bytes(p))
        folded.add(_fold(p, fold))
        room["hits"] -= k
        room["states"] -= nodes
        return True

    joined, total = b"".join(msgs), cnt.off[-1]
    here = sorted(set(joined))
    present = set(cnt.have)
    lack = [b for b in range(256) if _fold(bytes([b]), fold)[0] not in present]
    lack = [lack[int(rng.integers(len(lack)))]] if lack else []   # (one such byte: it is a class of its own in the automaton)
    # 255 bytes across a chunk seam of a stream longer than the chunk
    long = [i for i, l in enumerate(ln) if l > c]
    for i in [long[int(j)] for j in rng.permutation(len(long))[:4]]:
        seam = c * int(rng.integers(1, (ln[i] - 1) // c + 1))
        a = int(rng.integers(max(0, seam - 254), min(seam - 1, ln[i] - 255) + 1))
        if add(msgs[i][a:a + 255], HIT_CAP, "seam"):
            assert a < seam < a + 255
            break
    # up to a stream's last byte
    for i in [full[int(j)] for j in rng.permutation(len(full))[:64]]:
        k = int(rng.integers(1, min(ln[i], 24) + 1))
        if add(msgs[i][-k:], 2000, "end") or (ln[i] > k and add(msgs[i][-DICT_MAX_LEN:], 2000, "end")):
            break
    else:                                                          # (one symbol nearly everywhere: the shortest stream's whole text)
        i = min(full, key=lambda i: (-min(ln[i], DICT_MAX_LEN), ln[i]))
        add(msgs[i][-DICT_MAX_LEN:], HIT_CAP, "end")
    # every suffix and some prefixes of one pattern; a one- or two-symbol source: the runs of two of its bytes and of one it lacks
    if case.source in ("one", "two"):
        top = int(rng.integers(100, 256))
        whole = [0]
        for v in [here[int(j)] for j in rng.permutation(len(here))[:2]] + lack[:1]:
            key = np.where(np.frombuffer(cnt.have, dtype=np.uint8) == _fold(bytes([v]), fold)[0], np.repeat(np.arange(len(ln)), ln) + 1, 0)
            edges = np.flatnonzero(np.diff(np.concatenate([[0], key, [0]])))
            runs = np.diff(edges)[key[edges[:-1]] > 0] if edges.size else edges      # the runs of v, none across two messages
            took = []
            for k in range(1, top + 1):                            # (a run behind the next shorter one is one more node)
                took.append(add(bytes([v]) * k, 3000, "family", int(np.maximum(runs - k + 1, 0).sum()), 1 if took and took[-1] else k))
            whole.append(took.index(False) if False in took else top)
        special["family_whole"] = max(whole[:-1]) >= 4
    else:
        have = np.frombuffer(cnt.have, dtype=np.uint8)
        seen = np.bincount(have, minlength=256)
        rare = int(np.argmin(np.where(seen > 0, seen, 1 << 62)))
        at = int(rng.choice(np.flatnonzero(have == rare)))
        p = joined[max(cnt.off[cnt.stream_of(at)], at + 1 - int(rng.integers(4, 9))):at + 1]
        took = [add(p[k:], 2000) for k in range(len(p) - 1, 0, -1)]
        for k in sorted(set(int(v) for v in rng.integers(1, max(len(p), 2), size=2))):
            if k < len(p):
                add(p[:k], 2000)
        took.append(add(p, 2000, "family"))
        special["family_whole"] = all(took)
    # patterns that occur nowhere: substrings with one byte changed, to a byte the messages lack where there is one
    small = case.source in ("one", "two")
    target = int(rng.integers(300, 601 if small else 2001 if case.n_streams <= 65 else 801))
    nowhere = 0
    for _ in range(4 * max(target // 20, 3)):
        if nowhere >= max(target // 20, 3):
            break
        m = msgs[full[int(rng.integers(len(full)))]]
        a = int(rng.integers(len(m)))
        p = bytearray(m[a:a + int(rng.integers(1, 20))])
        p[int(rng.integers(len(p)))] = lack[int(rng.integers(len(lack)))] if lack and rng.random() < 0.5 else here[int(rng.integers(len(here)))]
        if cnt.count(p, 0) == 0 and _fold(p, fold) not in folded and add(bytes(p), 0):
            nowhere += 1
    special["nowhere"] = nowhere
    # a duplicate, of a pattern that hits where the budget allows
    for j in sorted(range(len(pats)), key=lambda j: (cnt.count(pats[j], 0) == 0, j)):
        if add(pats[j], 2000, "duplicate"):
            break
    # substrings of the messages; one that hits too often is drawn again at twice the length
    for _ in range(3 * target):
        if len(pats) >= target or room["states"] < 256:
            break
        at = int(rng.integers(total))
        end = cnt.off[cnt.stream_of(at) + 1]
        k = int(min(rng.geometric(0.15), DICT_MAX_LEN))
        while True:
            p = joined[at:min(at + k, end)]
            if _fold(p, fold) not in folded and add(p, 64):
                break
            if at + k >= end or k >= DICT_MAX_LEN:
                break
            k = min(2 * k, DICT_MAX_LEN)
    if fold:
        pats = [p.swapcase() if j % 2 else p for j, p in enumerate(pats)]
    order = rng.permutation(len(pats)).tolist()
    where = {j: k for k, j in enumerate(order)}
    e.dictionary = [pats[j] for j in order]
    e.special = {k: (where[v] if k in ("seam", "end", "family", "duplicate") else v) for k, v in special.items()}


def _draw_replacements(rng, w, e):
    """The deletion, and one replacement of 1, 2, 3, 64, 255 or 4 .. 254 bytes of the source alphabet; in about a quarter of the
    cases one of its bytes is a byte the messages lack."""
    here = np.unique(np.frombuffer(b"".join(w.messages), dtype=np.uint8))
    lack = np.setdiff1d(np.arange(256), here)
    e.lacking = int(rng.choice(lack)) if lack.size else None
    k = [1, 2, 3, 64, 255, int(rng.integers(4, 255))][int(rng.integers(6))]
    rep = rng.choice(here, size=k).astype(np.uint8)
    e.rep_lacks = bool(rng.random() < 0.25) and e.lacking is not None
    if e.rep_lacks:
        rep[int(rng.integers(k))] = e.lacking
    e.reps = [b"", rep.tobytes()]


def _craft(rng, L, c):
    """A valid span list of one stream of L bytes that reaches the edges: candidates at 0, over a seam, over whole chunks, a
    touching pair and at the end, of which those that do not overlap stay."""
    if L == 0:
        b = int(rng.integers(0, 3))
        return [(b, b + int(rng.integers(1, 4)))]
    if rng.random() < 0.2:
        return [(0, L + int(rng.choice([0, 0, 1, 9])))]            # the whole stream
    units = []
    if rng.random() < 0.6:
        units.append([(0, c + int(rng.integers(0, 6)) if L > c and rng.random() < 0.5 else int(rng.integers(1, 5)))])
    if L > c and rng.random() < 0.7:
        s = c * int(rng.integers(1, (L - 1) // c + 1))
        units.append([(s - int(rng.integers(1, 6)), s + int(rng.integers(1, 6)))])
    if L >= 3 * c and rng.random() < 0.6:
        j = int(rng.integers(1, L // c - 1))
        units.append([(j * c - int(rng.integers(0, 3)), (j + int(rng.integers(1, 3))) * c + int(rng.integers(0, 3)))])
    b = int(rng.integers(0, L))
    m = b + int(rng.integers(1, 9))
    units.append([(b, m), (m, m + int(rng.integers(1, 9)))])
    u, k = rng.random(), int(rng.integers(1, 6))
    if u < 0.3:
        units.append([(max(L - k, 0), L)])
    elif u < 0.55:
        units.append([(max(L - k, 0), L + int(rng.integers(1, 300)))])
    elif u < 0.8:
        b = L + int(rng.integers(0, 3))
        units.append([(b, b + k)])
    out, at = [], 0
    for unit in sorted(units):
        if unit[0][0] >= at:
            out += unit
            at = unit[-1][1]
    return out


def _draw_spans(rng, case, w, e):
    """The redaction pipeline, merge_hits over the records of a drawn subset of the dictionary's hits, with crafted spans put
    into up to ten streams (the longest among them; the merged spans that lie clear of them stay) and one stream in the middle
    left without spans.  At most SPAN_CAP spans, and no more than keep the spliced messages within SPLICED_BYTES."""
    msgs, c, n = w.messages, case.chunk, len(w.messages)
    ln = [len(m) for m in msgs]
    cap = min(SPAN_CAP, (SPLICED_BYTES - sum(ln)) // max(len(e.reps[1]), 1))
    k = int(rng.integers(1, max(min(len(e.hits), cap - 100), 1) + 1))
    pick = np.sort(rng.choice(len(e.hits), size=min(k, len(e.hits)), replace=False))
    rec = e.records[pick]
    off = np.concatenate([[0], np.cumsum(np.bincount(rec[:, 0].astype(np.int64), minlength=n))])
    so, sp = edit_ref.merge_hits(off, rec)
    per = [[(int(b), int(t)) for b, t in sp[int(so[i]):int(so[i + 1])]] for i in range(n)]
    crafted = {int(np.argmax(ln))} | set(int(i) for i in rng.integers(0, n, size=int(rng.integers(2, 10))))
    for i in sorted(crafted):                                     # (the merged spans that lie clear of the crafted ones stay)
        made = _craft(rng, ln[i], c)
        per[i] = sorted(made + [(b, t) for b, t in per[i] if all(t <= cb or b >= ct for cb, ct in made)])
    if n >= 3:
        i = int(rng.integers(1, n - 1))
        per[i] = []
        for j in (i - 1, i + 1):
            per[j] = per[j] or _craft(rng, ln[j], c)
    e.span_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint64)
    e.spans = np.array([s for p in per for s in p], dtype=np.uint64).reshape(-1, 2)


def _draw_map(rng, case, w, e):
    """One kind per case, going round MAP_KINDS by the case's number.  'lacking' (a random map into the source alphabet, but
    one byte of it goes to a byte the messages lack) is 'random' where the messages hold every byte value."""
    here = np.unique(np.frombuffer(b"".join(w.messages), dtype=np.uint8))
    kind = MAP_KINDS[case.index % len(MAP_KINDS)]
    m = np.arange(256, dtype=np.uint8)
    if kind == "mask":
        m[:] = rng.choice(here)
    elif kind == "fold":
        m = np.frombuffer(find_ref.fold_ascii(bytes(range(256))), dtype=np.uint8).copy()
    elif kind == "permutation":
        m[here] = rng.permutation(here)
    elif kind in ("random", "lacking"):
        m[:] = rng.choice(here, size=256)
        if kind == "lacking" and e.lacking is not None:
            m[rng.choice(here)] = e.lacking
        elif kind == "lacking":
            kind = "random"
    e.byte_map, e.map_kind = m.tobytes(), kind


# ---------------------------------------------------------------------------------------------------- tables and tagged lists
TABLE_ROOM = 250                   # entries of SPAN_CAP that the crafted insertions of a case may take
INSERTIONS = ("at 0", "at a seam", "one byte in front of a seam", "one byte behind a seam", "at the end of a span", "at the begin of a span",
              "several at one position", "the empty entry", "at len - 1", "at len or beyond", "in an empty stream", "a chain to a seam")
OUTPUT_SEAMS = ("inside a replacement", "one byte behind a replacement", "two bytes behind a replacement", "behind three touching spans")


def _draw_table(rng, w, e, t):
    """2 to 8 entries: the empty one, the case's replacement, and entries of 1, 2, 3, 64, 255 or 4 .. 254 bytes of the source
    alphabet; in about a quarter of the cases an entry gets a byte the messages lack, in about a third two entries are equal;
    then shuffled."""
    here = np.unique(np.frombuffer(b"".join(w.messages), dtype=np.uint8))
    k = int(rng.integers(2, 9))
    reps = [b"", e.reps[1]]
    while len(reps) < k:
        ln = [1, 2, 3, 64, 255, int(rng.integers(4, 255))][int(rng.integers(6))]
        reps.append(rng.choice(here, size=ln).astype(np.uint8).tobytes())
    lacks = int(rng.integers(2, k)) if k >= 3 and e.lacking is not None and rng.random() < 0.25 else None
    if lacks is not None:
        r = bytearray(reps[lacks])
        r[int(rng.integers(len(r)))] = e.lacking
        reps[lacks] = bytes(r)
    if k >= 4 and rng.random() < 0.35:                             # (the twin of an entry, not over the one that got the lacking byte)
        b = int(rng.choice([j for j in range(2, k) if j != lacks]))
        reps[b] = reps[int(rng.choice([j for j in range(1, k) if j != b]))]
    t.reps = [reps[int(j)] for j in rng.permutation(k)]
    t.empty = t.reps.index(b"")


def _insert(lst, p, tag):
    """Puts the insertion (p, p, tag) into one stream's well-formed list of (begin, end, tag): behind everything that ends at or
    in front of p, the insertions at p included; a span that holds p strictly inside is split in two at p."""
    for k, (b, end, g) in enumerate(lst):
        if b < p < end:
            lst[k:k + 1] = [(b, p, g), (p, end, g)]
            break
    lst.insert(sum(1 for _, end, _ in lst if end <= p), (p, p, tag))


def _put_unit(lst, unit, keep=0):
    """Puts touching spans into one stream's list; what they overlap gives way: a span is clipped, an insertion strictly
    between the unit's ends is dropped.  keep: as many source bytes behind the unit are cleared of spans as well."""
    lo, hi = unit[0][0], unit[-1][1] + keep
    out = []
    for b, end, g in lst:
        if end <= lo or b >= hi:
            out.append((b, end, g))
            continue
        if b < lo:
            out.append((b, lo, g))
        if end > hi:
            out.append((hi, end, g))
    at = sum(1 for _, end, _ in out if end <= lo)
    lst[:] = out[:at] + list(unit) + out[at:]


def splice_pieces(L, lst, reps):
    """One spliced stream of L source bytes as pieces in output order: ('src', output begin, length, source begin, None) and
    ('rep', output begin, length, source position, number of the span in lst)."""
    out, at, o = [], 0, 0
    for r, (b, end, g) in enumerate(lst):
        if b >= L:
            break
        if b > at:
            out.append(("src", o, b - at, at, None))
            o += b - at
        out.append(("rep", o, len(reps[g]), b, r))
        o += len(reps[g])
        at = min(end, L)
    if L > at:
        out.append(("src", o, L - at, at, None))
    return out


def _craft_insertions(rng, lst, L, c, k, empty, every, head=False):
    """Insertions of every kind of INSERTIONS that one stream of L bytes admits (every: all of them, else each with
    probability 1 / 2), and spans that end one byte in front of a seam (head: one of them from 0 up to the first seam)."""
    tag = lambda: int(rng.integers(k))
    other = lambda g: (g + 1 + int(rng.integers(k - 1))) % k
    go = lambda: every or rng.random() < 0.5
    if L == 0:
        for p in (0, int(rng.integers(0, 3))):
            _insert(lst, p, tag())
        return
    seams = list(range(c, L, c))
    seam = lambda: seams[int(rng.integers(len(seams)))]
    if head and seams:                                             # all but one byte in front of the first seam deleted: prev0 meets it
        _put_unit(lst, [(0, c - 1, empty)], keep=1)
    free = [s for s in seams if not (head and s == c)]            # (a single seam: the chain or a span that ends in front of it)
    chain = free[int(rng.integers(len(free)))] if free and go() and (len(free) > 1 or rng.random() < 0.5) else None
    if chain:                                                      # deletion, insertion, deletion up to a seam
        d1, d2 = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        a = chain - d1 - d2
        _put_unit(lst, [(a, a + d1, empty), (a + d1, a + d1, other(empty)), (a + d1, chain, empty)])
    for s in seams[:8]:                                            # a span that ends one byte in front of a seam, and x[seam - 1]
        if s != chain and not (head and s == c) and go():          # in no span: it follows what the span left, not x[seam - 2]
            _put_unit(lst, [(s - 1 - int(rng.integers(1, 4)), s - 1, tag())], keep=1)
    if go():
        _insert(lst, 0, tag())
    if seams:
        for d in (0, -1, 1):
            s = seam()
            if go() and s + d < L:
                _insert(lst, s + d, tag() if d >= 0 else other(empty))
    real = [(b, end) for b, end, _ in lst if b < end < L]
    if real and go():
        _insert(lst, real[int(rng.integers(len(real)))][1], tag())
    if real and go():
        _insert(lst, real[int(rng.integers(len(real)))][0], tag())
    if go():
        p, g = int(rng.integers(L)), tag()
        _insert(lst, p, g)
        _insert(lst, p, other(g))
    if go():
        _insert(lst, int(rng.integers(L)), empty)
    if go():
        _insert(lst, L - 1, tag())
    if go():
        _insert(lst, L, tag())
    if go():
        _insert(lst, L + int(rng.integers(1, 300)), tag())


def _craft_output_seams(rng, lst, L, c, reps, first):
    """At every seam of the OUTPUT of one stream, in ascending order (what is put in at one seam moves no earlier one), one of
    OUTPUT_SEAMS, going round them from `first`: the unit goes into a run of source bytes that no span touches, where there is
    one at the right distance in front of the seam."""
    k, Q, turn = len(reps), c, first
    while Q <= 6 * c:                                              # (the first six seams: a short chunk has many)
        pieces = splice_pieces(L, lst, reps)
        if not pieces or Q >= pieces[-1][1] + pieces[-1][2]:
            return
        kind = OUTPUT_SEAMS[turn % len(OUTPUT_SEAMS)]
        for _ in range(8):                                         # (other tags, other lengths: another distance)
            g = [int(v) for v in rng.integers(k, size=3)]
            r = [len(reps[v]) for v in g]
            if kind == "inside a replacement":
                if r[0] < 2:
                    continue
                T, width, make = Q - int(rng.integers(1, r[0])), 1, lambda p: [(p, p + int(rng.integers(0, 2)), g[0])]
            elif kind == "behind three touching spans":
                T, width, make = Q - sum(r), 4, lambda p: [(p, p + 1, g[0]), (p + 1, p + 2, g[1]), (p + 2, p + 3, g[2])]
            else:
                if r[0] < 1:
                    continue
                behind = 1 if kind == "one byte behind a replacement" else 2
                T, width, make = Q - r[0] - behind, 1 + behind + 1, lambda p: [(p, p + 1, g[0])]
            run = [(o, n, sb) for what, o, n, sb, _ in pieces if what == "src" and o < T and T + width < o + n]
            if run:
                o, n, sb = run[0]
                _put_unit(lst, make(sb + T - o))
                break
        Q, turn = Q + c, turn + 1


def _draw_tagged(rng, case, w, e, t):
    """The span list of edits() with a tag per span, drawn over the table, and insertions put in by craft: into the longest
    stream every kind it admits, into up to four more streams, one longer than a chunk and one empty among them where there
    are such, about half of them, and spans that end one byte in front of a seam (in the second long stream one that deletes
    everything up to there from 0); then units at the seams of the OUTPUT of the streams longer than a chunk.  A span that holds a
    crafted insertion is split there; where a crafted unit of touching spans overlaps spans of the list, they are clipped.
    The insertions get TABLE_ROOM entries of SPAN_CAP: a list with less room first loses spans, drawn evenly."""
    c, ln = case.chunk, [len(m) for m in w.messages]
    n, k = len(ln), len(t.reps)
    tags = rng.integers(k, size=len(e.spans))
    keep = np.ones(len(e.spans), dtype=bool)
    if len(e.spans) > SPAN_CAP - TABLE_ROOM:
        keep[rng.choice(len(e.spans), size=len(e.spans) - (SPAN_CAP - TABLE_ROOM), replace=False)] = False
    per, r = [], 0
    for lst in span_lists(e.span_off, e.spans):
        per.append([(int(b), int(end), int(tags[r + j])) for j, (b, end) in enumerate(lst) if keep[r + j]])
        r += len(lst)
    longest = int(np.argmax(ln))
    long = [i for i in range(n) if ln[i] > c and i != longest]
    empty = [i for i in range(n) if ln[i] == 0]
    more = [int(i) for i in rng.integers(0, n, size=int(rng.integers(1, 3)))]
    more += [long[int(rng.integers(len(long)))]] if long else []
    more += [empty[int(rng.integers(len(empty)))]] if empty else []
    room = lambda: SPAN_CAP - sum(len(p) for p in per)
    for j, i in enumerate([longest] + sorted(set(more) - {longest})):
        if room() >= 48:
            _craft_insertions(rng, per[i], ln[i], c, k, t.empty, j == 0, bool(long) and i == more[-1 - bool(empty)])
    for j, i in enumerate([longest] + sorted(set(long) & set(more))):
        if room() >= 16:
            _craft_output_seams(rng, per[i], ln[i], c, t.reps, case.index + j)
    t.span_off, t.spans, t.tags = splice_table_ref.tagged_lists(per)


def tagged_span_lists(span_off, spans, tags):
    """[[(begin, end, tag)] per stream] of a tagged span list."""
    tags = [int(g) for g in tags]
    out, r = [], 0
    for lst in span_lists(span_off, spans):
        out.append([(b, end, tags[r + j]) for j, (b, end) in enumerate(lst)])
        r += len(lst)
    return out


def insertions(messages, span_off, spans, tags, reps, chunk):
    """Which of INSERTIONS a tagged list reaches on these messages (a set of names), from the list alone.  A span next to an
    insertion is the nearest entry of the list that is no insertion; a chain is a deletion, one or more insertions where it
    ends, one of them not empty, and a deletion from there up to a seam inside the stream."""
    c, got = chunk, set()
    for m, lst in zip(messages, tagged_span_lists(span_off, spans, tags)):
        L = len(m)
        for j, (b, end, g) in enumerate(lst):
            if b != end:
                continue
            if L == 0 or b >= L:
                got.add("in an empty stream" if L == 0 else "at len or beyond")
                continue
            got.add("at 0" if b == 0 else "at a seam" if b % c == 0 else "")
            got.add("one byte in front of a seam" if (b + 1) % c == 0 and b + 1 < L else "one byte behind a seam" if b % c == 1 and b > c else "")
            got.add("at len - 1" if b == L - 1 else "")
            got.add("the empty entry" if not reps[g] else "")
            front = [x for x in lst[:j] if x[0] < x[1]][-1:]
            behind = [x for x in lst[j + 1:] if x[0] < x[1]][:1]
            got.add("at the end of a span" if front and front[0][1] == b else "")
            got.add("at the begin of a span" if behind and behind[0][0] == b else "")
            if any(x[0] == x[1] == b and x[2] != g for x in lst[j + 1:j + 4]):
                got.add("several at one position")
        for j, (b, end, g) in enumerate(lst):                      # a chain
            if b < end and not reps[g]:
                k = j + 1
                while k < len(lst) and lst[k][0] == lst[k][1] == end:
                    k += 1
                if k > j + 1 and k < len(lst) and any(reps[x[2]] for x in lst[j + 1:k]):
                    b2, e2, g2 = lst[k]
                    if b2 == end < e2 < L and e2 % c == 0 and not reps[g2]:
                        got.add("a chain to a seam")
    return got - {""}


def output_seams(messages, span_off, spans, tags, reps, chunk):
    """Which of OUTPUT_SEAMS a tagged list reaches: where the chunks of the spliced messages start, from splice_pieces.  A
    replacement here has at least one byte; touching spans are entries of the list, insertions included, each of which begins
    where the one in front ends."""
    got = set()
    for m, lst in zip(messages, tagged_span_lists(span_off, spans, tags)):
        L = len(m)
        pieces = splice_pieces(L, lst, reps)
        if not pieces:
            continue
        total = pieces[-1][1] + pieces[-1][2]
        run = {}                                                   # number of a span in lst -> the touching spans up to it
        for r, (b, end, g) in enumerate(lst):
            run[r] = run[r - 1] + 1 if r and b < L and lst[r - 1][1] == b else 1
        for what, o, n, sb, r in pieces:
            if what != "rep":
                continue
            stop, at = o + n, min(lst[r][1], L)                    # where it ends in the output and in the source
            nxt = lst[r + 1][0] if r + 1 < len(lst) and lst[r + 1][0] < L else L + 1
            if n and any(o < q < stop for q in range((o // chunk + 1) * chunk, stop, chunk)):
                got.add("inside a replacement")
            for d, name in ((1, "one byte behind a replacement"), (2, "two bytes behind a replacement")):
                if n and (stop + d) % chunk == 0 and stop + d < total and at + d <= min(nxt, L):
                    got.add(name)
            if run[r] >= 3 and stop and stop % chunk == 0 and stop < total and nxt > at:
                got.add("behind three touching spans")
    return got


def span_lists(span_off, spans):
    """[[(begin, end)] per stream] of a span list."""
    sp = np.asarray(spans, dtype=np.uint64).reshape(-1, 2).tolist()
    return [[tuple(s) for s in sp[int(span_off[i]):int(span_off[i + 1])]] for i in range(len(span_off) - 1)]


def placements(messages, span_off, spans, chunk):
    """Which of PLACEMENTS a span list reaches on these messages (a set of names).  'whole chunks': a span covers a full chunk
    of its stream, from its first byte to its last; 'over a seam': the bytes a span covers lie in two chunks."""
    per, c, got = span_lists(span_off, spans), chunk, set()
    for i, (m, lst) in enumerate(zip(messages, per)):
        L = len(m)
        for k, (b, t) in enumerate(lst):
            if b >= L:
                got.add("at or past the end")
                continue
            if b == 0:
                got.add("from 0")
            got.add("to the last byte" if t == L else "past the end" if t > L else "")
            if b // c != (min(t, L) - 1) // c:
                got.add("over a seam")
            if (b + c - 1) // c * c + c <= min(t, L):
                got.add("whole chunks")
            if b == 0 and t >= L:
                got.add("whole stream")
            if k + 1 < len(lst) and lst[k + 1][0] == t < L:
                got.add("touching")
        if not lst and 0 < i < len(per) - 1 and per[i - 1] and per[i + 1]:
            got.add("a stream without spans between two with spans")
    return got - {""}


def span_mask(messages, span_off, spans):
    """One flag per byte of the concatenated messages: inside a span, or the byte in front of one or behind one."""
    off = np.concatenate([[0], np.cumsum([len(m) for m in messages])])
    mask = np.zeros(int(off[-1]), dtype=bool)
    for i, lst in enumerate(span_lists(span_off, spans)):
        L = len(messages[i])
        for b, t in lst:
            if b < L:
                mask[off[i] + max(b - 1, 0):off[i] + min(t + 1, L)] = True
    return mask


def tables_lds(lens, codes, order):
    """LDS bytes of the decode tables of a shared order-0 / 1 model with these code tables (csrc/mh_batch.h, mhb::tables_lds): the
    1 KiB of bases, 256 first-level tables of 2^P entries of two bytes and the second level, P the largest of 8 .. 4 with which
    both fit (csrc/mh_api_model.cpp).  A second-level table hangs at every P-bit prefix of a longer code and has 2^(its longest
    code's bits behind the prefix, 8 at most) entries.  (first level alone when no P fits: the second level then stays in L2)"""
    L = np.asarray(lens, dtype=np.int64).reshape(-1, 256)
    cd = np.asarray(codes, dtype=np.uint64).reshape(-1, 256)
    for P in range(8, 3, -1):
        total = worst = 0
        for ctx in np.flatnonzero(L.max(axis=1) > P):
            tables = {}
            for s in np.flatnonzero(L[ctx] > P):
                pre = int(cd[ctx, s]) >> (int(L[ctx, s]) - P)
                tables[pre] = max(tables.get(pre, 0), min(int(L[ctx, s]) - P, 8))
            here = sum(1 << h for h in tables.values())
            total, worst = total + here, max(worst, here)
        if worst <= DEC_SEC_MAX_PER_CTX and (256 << P) + total <= DEC_LDS_ENTRIES:
            return 1024 + (512 << P) + ((2 * total + 15) & ~15)
    return 1024 + (512 << 8)


def dict_rows_in_lds(case, states, classes):
    """How many of the transition table's `states` rows the matcher keeps in LDS under the case's source (csrc/mh_find.hip,
    launch_find_dict and launch_dict): a shared order-0 / 1 source leaves what its decode tables do not take of LDS_BYTES, an
    order-2 source or a model set reads its tables from L2 and gets LDS_BYTES / DICT_PER_CU; 256 bytes of that hold the class
    map, rows of 2 * classes bytes the rest (csrc/mh_dict.h: trans u16[states x ncls]); with less than 256 bytes no row."""
    room = LDS_BYTES // DICT_PER_CU if case.orders[0] == 2 else LDS_BYTES - tables_lds(*case.codes("src"), case.orders[0])
    return 0 if room < 256 else min(states, (room - 256) // (2 * classes))
