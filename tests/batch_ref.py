"""Generator and references of the batch-family fuzz (tests/test_batch_ref.py, tests/test_gpu_batch_fuzz.py): seeded small
batches, and what every batch call of include/mh.h must give for them, from the CPU oracle's code tables and plain numpy on
the original messages (a helper module like find_ref.py and recode_ref.py; it imports numpy and the oracle, never the library).

A case is drawn in two steps: draw_cases(seed) fixes every case's parameters (and its own seed) from one generator, and
Case.world() builds the messages, patterns, lookups and model counts of one case when a test needs them."""
import functools

import numpy as np

import find_ref
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
