"""Generator and references of the far-batch tests (tests/test_far_ref.py, tests/test_gpu_batch_far.py): one batch whose
offsets and in-stream positions lie beyond 2^32, and what the batch calls of include/mh.h must give for it, in closed form
(a helper module like batch_ref.py; it uses numpy and, through batch_ref, the oracle's code tables, never the library).

The construction is a periodic filler.  `blk` is one block of BLOCK bytes whose last byte is PREV0, so a block that follows a
block starts in the same order-1 context as a block that starts a stream; and its bit length is a multiple of 8 under both
models, the source model S (order 1) and the destination model D (order 0), so a block's code bits start on a byte wherever
the block lies.  The filler stream F is blk x P followed by `tail`.  Then

  * F's payload is pack(blk) tiled P times, followed by pack(tail) (tail starts in context PREV0 as a stream does);
  * F's index slice is the block's slice + k * nbits(blk) in period k, then the tail's slice + P * nbits(blk)
    (BLOCK is a multiple of every chunk size);
  * its histograms, its CRC-32, its hit records and the bytes of any lookup follow from one block, the tail and P.

So everything comes from batch_ref.pack on a few hundred KiB, for any P: tests/test_far_ref.py compares every closed form with
batch_ref, find_ref and zlib on the real concatenation at P = 3 and P = 5, and the GPU test materialises the same closed
forms at the full P with torch.  S and D are the oracle's models of (the histogram of the batch at P = 1) + 1 in every cell:
the code tables do not depend on P, so the tables that the CPU test proves are the tables of the full-size run.

The batch, in order: three small streams, F, two small streams, G (blk x 3, no tail: wholly behind F and under
MH_BATCH_WALK_MAX_BITS) and about 30 small streams, the last one empty.  Everything is drawn from one seed.

Far.mix() is the same batch with every stream under its own entry of the bank [S, D]; Far.without_f() the batch as the
index-free device calls see it, which refuse F alone; Far.edited() and Far.spliced() the batch after the masked and the
splicing re-code of Far.spans(), which touch tails and small streams only, so the edited F is again blk x P + a tail.  Far2 is
the same layout for an order-2 source model."""
import copy
import functools
import zlib

import numpy as np

import batch_ref
import edit_ref
import find_ref
import splice_ref

PREV0 = batch_ref.PREV0
BLOCK = 256 << 10                  # bytes of the block: a multiple of every chunk size used
CHUNKS = (1024, 256)               # the main run; decode, lookups and search (four times the chunk numbers)
SUFFIX = 63                        # bytes in front of the block's last byte that the search redraws
SEED = 20261020
WALK_MAX_BITS = 1 << 23            # include/mh.h MH_BATCH_WALK_MAX_BITS
G_PERIODS = 3
FAR = 1 << 32
FAR_HITS = 2048                    # periods of F that begin beyond symbol 2^32: as many hit records of the once-per-period pattern


# ---------------------------------------------------------------------------------------------------- CRC-32 of A || B
def _gf2_times(mat, vec):
    out, i = 0, 0
    while vec:
        if vec & 1:
            out ^= mat[i]
        vec >>= 1
        i += 1
    return out


def _gf2_square(mat):
    return [_gf2_times(mat, row) for row in mat]


def crc_shift(crc, nbytes):
    """The CRC-32 register `crc` after nbytes zero bytes went through it: the operator of one zero bit (a 32 x 32 matrix over
    GF(2), one uint32 per column) is squared up to x^(8 * nbytes), one squaring per bit of nbytes."""
    mat = [0xEDB88320] + [1 << (k - 1) for k in range(1, 32)]     # one zero bit
    for _ in range(3):
        mat = _gf2_square(mat)                                     # one zero byte
    while nbytes:
        if nbytes & 1:
            crc = _gf2_times(mat, crc)
        nbytes >>= 1
        if nbytes:
            mat = _gf2_square(mat)
    return crc


def crc_concat(crc_a, crc_b, len_b):
    """zlib's CRC-32 of A || B from those of A and B (the shift identity: the pre- and post-inversions cancel)."""
    return crc_shift(crc_a, len_b) ^ crc_b


def crc_repeat(crc_one, length, times):
    """CRC-32 of a string of `length` bytes repeated `times` times, by doubling."""
    out, out_len = 0, 0                                            # of the empty string
    unit, unit_len = crc_one, length
    while times:
        if times & 1:
            out, out_len = crc_concat(out, unit, unit_len), out_len + unit_len
        times >>= 1
        if times:
            unit, unit_len = crc_concat(unit, unit, unit_len), 2 * unit_len
    return out


# ---------------------------------------------------------------------------------------------------- the batch
class Stream:
    """`reps` copies of the block followed by `tail` (a small stream: reps == 0)."""

    def __init__(self, reps, tail):
        self.reps, self.tail = int(reps), bytes(tail)

    def __len__(self):
        return self.reps * BLOCK + len(self.tail)


class FarPacked:
    """The closed form of batch_ref.Packed: pay_off / nbits / sym_off / dropped uint64, and the big arrays as parts.
    payload_parts: [(bytes uint8, repeat count)] in order.  index_parts: [(first entry's position in the batch index,
    entries uint64, repeat count, what every repeat adds)]; the entries of one part lie back to back."""

    def payload(self):
        return np.concatenate([np.tile(a, k) for a, k in self.payload_parts] + [np.zeros(0, dtype=np.uint8)])

    def index_array(self, fill=0):
        """The batch index, `fill` in the gaps."""
        idx = np.full(self.index_entries, fill, dtype=np.uint64)
        for at, a, k, step in self.index_parts:
            idx[at:at + a.size * k] = (a[None, :] + (np.arange(k, dtype=np.uint64) * np.uint64(step))[:, None]).reshape(-1)
        return idx

    def index_mask(self):
        """True where a slice lies."""
        m = np.zeros(self.index_entries, dtype=bool)
        for at, a, k, _ in self.index_parts:
            m[at:at + a.size * k] = True
        return m


def _draw_block(rng, others):
    """The block and the two code tables.  BLOCK near-uniform bytes; the SUFFIX bytes in front of the last one (PREV0) are drawn
    again until the block's bit length is 0 modulo 8 under S and under D, the models of (counts of block + others) + 1.  Half
    of the suffix comes from symbols whose order-0 code is not 8 bits long: those lengths hardly vary, and a uniform suffix
    never moves the order-0 length off its residue."""
    blk = rng.integers(0, 256, size=BLOCK, dtype=np.uint8)
    blk[-1] = PREV0
    base = [batch_ref.histogram(others, o) for o in (0, 1)]
    odd = np.arange(256)
    for draw in range(20000):
        msg = [blk.tobytes()]
        h0, h1 = batch_ref.histogram(msg, 0), batch_ref.histogram(msg, 1)
        c0, c1 = h0 + base[0] + np.uint64(1), h1 + base[1] + np.uint64(1)
        l0, _ = batch_ref.oracle_codes(c0, 0)
        l1, _ = batch_ref.oracle_codes(c1, 1)
        if int((h0.astype(np.int64) * l0).sum()) % 8 == 0 and int((h1.astype(np.int64) * l1).sum()) % 8 == 0:
            assert l0.min() > 0 and l1.min() > 0
            return blk.tobytes(), c0, c1, draw
        odd = np.flatnonzero(l0 != 8) if (l0 != 8).any() else np.arange(256)
        blk[-1 - SUFFIX:-1] = rng.integers(0, 256, size=SUFFIX)
        blk[-1 - SUFFIX:-1:2] = rng.choice(odd, size=(SUFFIX + 1) // 2)
    raise AssertionError("no block found")


class Far:
    """The batch of one seed with P periods in F (None: the full size, from the block's measured lengths)."""

    def __init__(self, P=None, seed=SEED):
        self.seed = seed
        rng = np.random.default_rng(seed)
        zipf = lambda n: batch_ref.draw_source(rng, "zipf", n, 256).tobytes()
        c = CHUNKS[0]
        # patterns that occur only in the tail and in far small streams
        self.pat_a = bytes(rng.integers(0, 256, size=8, dtype=np.uint8))
        self.pat_b = bytes(rng.integers(0, 256, size=5, dtype=np.uint8))
        tail = bytearray(zipf(4 * c + 37))
        tail[100:108] = self.pat_a
        tail[2 * c - 3:2 * c + 5] = self.pat_a                     # over a chunk seam of both chunk sizes
        tail[c - 2:c + 3] = self.pat_b
        tail[-5:] = self.pat_b                                     # up to F's last byte
        head = [zipf(3000), b"", zipf(1)]
        mid = [zipf(c - 1), zipf(c)]
        lens = [0, 0, 1, c - 1, c, c + 1, 2 * c + 17, 3001, 255, 256, 257, 2 * 256 + 17, 4999]
        far = [bytearray(zipf(lens[j % len(lens)])) for j in range(30)]
        far[7][1000:1008] = self.pat_a
        far[12][-5:] = self.pat_b
        far[19][5:10] = self.pat_b
        far = [bytes(m) for m in far] + [b""]
        smalls = head + mid + far
        self.blk, c0, c1, self.draws = _draw_block(rng, [bytes(tail)] + smalls)
        self.counts = {"S": c1, "D": c0}
        self.orders = {"S": 1, "D": 0}
        self.codes = {k: batch_ref.oracle_codes(self.counts[k], self.orders[k]) for k in "SD"}
        self.block_bits = {k: int(batch_ref.pack([self.blk], *self.codes[k], self.orders[k], PREV0).nbits[0]) for k in "SD"}
        if P is None:
            P = max(-(-(FAR + FAR_HITS * BLOCK) // BLOCK), *(int(8 * FAR // int(b)) + 1 for b in self.block_bits.values()))
        self.P = int(P)
        self.streams = [Stream(0, m) for m in head] + [Stream(self.P, tail)] + [Stream(0, m) for m in mid] + [Stream(G_PERIODS, b"")] + \
            [Stream(0, m) for m in far]
        self.f, self.g = len(head), len(head) + 1 + len(mid)
        self.tail_f = bytes(tail)
        self.src = "S"
        self._finish()

    def _finish(self):
        self._lay_out()
        self.pat_p_at = next(o for o in range(100003, BLOCK - 100) if self.blk.count(self.blk[o:o + 12]) == 1)
        self.pat_p = self.blk[self.pat_p_at:self.pat_p_at + 12]      # once per period
        self.patterns = [self.pat_b, self.pat_p, self.pat_a]
        assert all(BLOCK % ch == 0 for ch in CHUNKS) and self.blk[-1] == PREV0

    def _lay_out(self):
        self.n = len(self.streams)
        self.lengths = [len(s) for s in self.streams]
        self.sym_off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.uint64)
        self.total = int(self.sym_off[-1])

    def without_f(self):
        """The same batch with an empty stream in F's place: what the index-free device calls, which refuse F alone (it is over
        MH_BATCH_WALK_MAX_BITS), must give for every other stream; a refused stream has no symbol, bit, hit or digest."""
        other = copy.copy(self)
        other.streams = [Stream(0, b"") if i == self.f else s for i, s in enumerate(self.streams)]
        other._lay_out()
        return other

    # ---- edits ----
    def spans(self):
        """(span_off uint64[n + 1], spans uint64[m, 2]) of the masked and the splicing re-code.  In F every span lies in the
        tail, so beyond 2^32 of F at the full size and clear of every period's last byte (the edited F is blk x P + the edited
        tail): one over a planted pattern, a touching pair, one over a chunk seam of both chunk sizes and one that runs past
        F's end.  In the far small streams: from 0, a pattern, up to the last byte, a whole stream (the deletion empties it),
        a stream without spans between two with spans, one at or past the end and one on an empty stream.  G has none."""
        per = [[] for _ in range(self.n)]
        t, lf, c, far = self.streams[self.f].reps * BLOCK, self.lengths[self.f], CHUNKS[0], self.g + 1
        if lf:
            per[self.f] = [(t + 50, t + 60), (t + 100, t + 108), (t + 108, t + 111), (t + 2 * c - 3, t + 2 * c + 5), (lf - 5, lf + 3)]
        per[far] = [(0, 2)]
        per[far + 7] = [(0, 4), (1000, 1008), (2990, 3001)]
        per[far + 9] = [(0, 256)]
        per[far + 12] = [(4994, 4999), (5000, 5003)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.uint64)
        return off, np.array([x for lst in per for x in lst], dtype=np.uint64).reshape(-1, 2)

    def byte_map(self):
        """A random map of the bytes (every byte has a code under both models)."""
        return np.random.default_rng([self.seed, 7]).integers(0, 256, size=256, dtype=np.uint8).tobytes()

    def reps(self):
        """The deletion and one replacement longer than every span but one."""
        return [b"", bytes(np.random.default_rng([self.seed, 8]).integers(0, 256, size=23, dtype=np.uint8))]

    def _with_tails(self, fn):
        """The batch whose tails are fn(tails, span_off, spans counted from each tail's first byte)."""
        off, sp = self.spans()
        shift = np.repeat(np.array([s.reps * BLOCK for s in self.streams], dtype=np.uint64), np.diff(off.astype(np.int64)))
        assert (sp[:, 0] >= shift).all()
        tails = fn([s.tail for s in self.streams], off, sp - shift[:, None])
        other = copy.copy(self)
        other.streams = [Stream(s.reps, t) for s, t in zip(self.streams, tails)]
        other._lay_out()
        return other

    def edited(self):
        """The batch after the masked re-code: the bytes inside the spans mapped."""
        return self._with_tails(lambda tails, off, sp: edit_ref.apply(tails, off, sp, self.byte_map()))

    def spliced(self, rep):
        """The batch after the splicing re-code: every span replaced by rep; its sym_off is the call's out_sym_off."""
        return self._with_tails(lambda tails, off, sp: splice_ref.apply(tails, off, sp, rep))

    # ---- the messages ----
    def messages(self):
        """The real messages (small P only)."""
        assert self.P <= 8
        return [self.blk * s.reps + s.tail for s in self.streams]

    def data_parts(self):
        """[(bytes uint8, repeat count)] of the concatenated messages."""
        u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
        return [p for s in self.streams for p in ((u8(self.blk), s.reps), (u8(s.tail), 1)) if p[1] and p[0].size]

    def read(self, i, begin, end):
        """Bytes [begin, end) of stream i."""
        s, out = self.streams[i], bytearray()
        assert 0 <= begin <= end <= len(s)
        at = begin
        while at < end:
            if at < s.reps * BLOCK:
                o = at % BLOCK
                take = min(end - at, BLOCK - o)
                out += self.blk[o:o + take]
            else:
                o = at - s.reps * BLOCK
                take = end - at
                out += s.tail[o:o + take]
            at += take
        return bytes(out)

    # ---- the packer ----
    @functools.lru_cache(maxsize=8)
    def _unit(self, model, chunk):
        """batch_ref.pack of [blk] + every stream's tail: all that the closed forms need."""
        u = batch_ref.pack([self.blk] + [s.tail for s in self.streams], *self.codes[model], self.orders[model], PREV0, chunk)
        assert not u.dropped.any()
        return u

    def pack(self, model, chunk):
        """FarPacked of the batch under model 'S' or 'D'."""
        u = self._unit(model, chunk)
        nb = int(u.nbits[0])
        assert nb % 8 == 0 and nb == int(self.block_bits[model])
        piece = lambda j: u.payload[int(u.pay_off[j]):int(u.pay_off[j + 1])]
        p = FarPacked()
        p.block_bits = nb
        p.nbits = np.array([s.reps * nb + int(u.nbits[1 + i]) for i, s in enumerate(self.streams)], dtype=np.uint64)
        p.pay_off = np.concatenate([[0], np.cumsum((p.nbits.astype(np.int64) + 7) // 8)]).astype(np.uint64)
        p.sym_off = self.sym_off.copy()
        p.dropped = np.zeros(self.n, dtype=np.uint64)
        p.chunk = chunk
        p.index_entries = self.total // chunk + self.n + 1 if chunk else 0
        p.stream_payload, p.stream_index = [], []
        for i, s in enumerate(self.streams):
            p.stream_payload.append([q for q in ((piece(0), s.reps), (piece(1 + i), 1)) if q[1] and q[0].size])
            at, parts = (int(self.sym_off[i]) // chunk + i if chunk else 0), []
            if chunk and s.reps:
                parts.append((at, u.slices[0], s.reps, nb))
            if chunk and s.tail:
                parts.append((at + s.reps * (BLOCK // chunk), u.slices[1 + i] + np.uint64(s.reps * nb), 1, 0))
            p.stream_index.append(parts)
        p.payload_parts = [q for parts in p.stream_payload for q in parts]
        p.index_parts = [q for parts in p.stream_index for q in parts]
        return p

    def choice(self):
        """A choice of the bank [S, D] per stream: F and G under S, the small streams in turn under S and D."""
        return np.array([0 if i in (self.f, self.g) else i % 2 for i in range(self.n)], dtype=np.uint32)

    def mix(self, choice, chunk):
        """FarPacked of the batch with stream i under entry choice[i] of the bank [S, D]: a stream's payload and index slice
        do not depend on the streams around it, and its slice lies where its symbols put it."""
        packs = [self.pack("S", chunk), self.pack("D", chunk)]
        p = FarPacked()
        p.nbits = np.array([packs[int(c)].nbits[i] for i, c in enumerate(choice)], dtype=np.uint64)
        p.pay_off = np.concatenate([[0], np.cumsum((p.nbits.astype(np.int64) + 7) // 8)]).astype(np.uint64)
        p.sym_off, p.dropped, p.chunk, p.index_entries = self.sym_off.copy(), np.zeros(self.n, dtype=np.uint64), chunk, packs[0].index_entries
        p.payload_parts = [q for i, c in enumerate(choice) for q in packs[int(c)].stream_payload[i]]
        p.index_parts = [q for i, c in enumerate(choice) for q in packs[int(c)].stream_index[i]]
        return p

    def entry_bits(self, model, chunk, i, j):
        """Bit offset, in stream i's own payload, of its chunk j (j == its chunk count: its nbits)."""
        u, s = self._unit(model, chunk), self.streams[i]
        per = BLOCK // chunk
        mask = np.uint64((1 << 48) - 1)
        if j < s.reps * per:
            return (j // per) * int(u.nbits[0]) + int(u.slices[0][j % per] & mask)
        j -= s.reps * per
        sl = u.slices[1 + i]
        return s.reps * int(u.nbits[0]) + (int(sl[j] & mask) if j < sl.size else int(u.nbits[1 + i]))

    # ---- training histograms ----
    def histogram(self, order):
        """Summed counts of the batch's streams, each from context PREV0.  Orders 0 and 1: a block counts the same wherever it
        lies (its first byte follows PREV0 in a stream's front and behind a block alike).  Order 2: the first symbol of a block
        behind a block, and of a tail behind a block, has (the block's last two bytes) in front of it, not (PREV0, PREV0)."""
        one = batch_ref.histogram([self.blk], order).astype(np.int64)
        out = batch_ref.histogram([s.tail for s in self.streams], order).astype(np.int64)
        reps = sum(s.reps for s in self.streams)
        out += reps * one
        if order == 2:
            seam = (self.blk[-2] << 8 | self.blk[-1]) * 256
            start = (PREV0 << 8 | PREV0) * 256
            for s in self.streams:
                if s.reps:
                    firsts = [self.blk[0]] * (s.reps - 1) + ([s.tail[0]] if s.tail else [])
                    for b in firsts:
                        out[start + b] -= 1
                        out[seam + b] += 1
        return out.astype(np.uint64)

    # ---- digests ----
    def crcs(self):
        """(zlib CRC-32 uint32[n], length uint64[n]) of every stream."""
        one = zlib.crc32(self.blk)
        crc = [crc_concat(crc_repeat(one, BLOCK, s.reps), zlib.crc32(s.tail), len(s.tail)) for s in self.streams]
        return np.array(crc, dtype=np.uint32), np.array(self.lengths, dtype=np.uint64)

    # ---- bank selection ----
    def select(self):
        """(choice uint32[n], nbits uint64[n]) of the bank [S, D]: the fewer bits, ties and empty streams to entry 0 (both
        models have a code for every pair)."""
        s, d = self.pack("S", 0).nbits, self.pack("D", 0).nbits
        return (d < s).astype(np.uint32), np.minimum(s, d)

    # ---- search ----
    def hits(self):
        """(hit_off uint64[n + 1], records uint64[k, 3], pattern uint32[k]) of self.patterns, in (stream, end, pattern) order.
        One block holds pat_p once and no other pattern, neither do two blocks or a block and a tail across their seam
        (asserted here on blk + blk + tail): a stream's hits are those of its periods, begin = k * BLOCK + o, then its tail's."""
        pats = self.patterns
        tail_f = self.tail_f
        seen = find_ref.find_hits([self.blk + self.blk + tail_f], pats)
        want = [(0, k * BLOCK + self.pat_p_at, k * BLOCK + self.pat_p_at + 12, 1) for k in (0, 1)] + \
            [(0, 2 * BLOCK + b, 2 * BLOCK + e, j) for _, b, e, j in find_ref.find_hits([tail_f], pats)]
        assert seen == want, "the block repeats a pattern, or a pattern lies across a seam"
        rec, pat, off = [], [], [0]
        for i, s in enumerate(self.streams):
            k = np.arange(s.reps, dtype=np.uint64) * np.uint64(BLOCK) + np.uint64(self.pat_p_at)
            t = find_ref.find_hits([s.tail], pats)
            tb = np.array([[b, e] for _, b, e, _ in t], dtype=np.uint64).reshape(-1, 2) + np.uint64(s.reps * BLOCK)
            be = np.concatenate([np.stack([k, k + np.uint64(12)], axis=1), tb])
            rec.append(np.concatenate([np.full((be.shape[0], 1), i, dtype=np.uint64), be], axis=1))
            pat.append(np.concatenate([np.full(s.reps, 1, dtype=np.uint32), np.array([j for _, _, _, j in t], dtype=np.uint32)]))
            off.append(off[-1] + be.shape[0])
        return np.array(off, dtype=np.uint64), np.concatenate(rec), np.concatenate(pat)

    # ---- lookups ----
    def marks(self):
        """Positions inside F that the lookups straddle: symbol 2^32, and the chunks (of CHUNKS[1] symbols, under the source model) whose payload
        spans hold bit 2^32 and byte 2^32 of F's own payload.  A batch too small for one of them takes a position in the
        middle of F instead, so the same code runs at every P."""
        ch, ln = CHUNKS[1], self.lengths[self.f]
        nb = int(self.pack(self.src, ch).nbits[self.f])
        out = {"symbol": FAR if ln > FAR + ch else ln // 2 + 5}
        for name, bit in (("bit", FAR), ("byte", 8 * FAR)):
            bit = bit if nb > bit + 64 else nb // 3 if name == "bit" else 2 * nb // 3
            lo, hi = 0, -(-ln // ch)                                # the last chunk that starts at or before `bit`
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if self.entry_bits(self.src, ch, self.f, mid) <= bit else (lo, mid)
            assert self.entry_bits(self.src, ch, self.f, lo) <= bit < self.entry_bits(self.src, ch, self.f, lo + 1)
            out[name] = lo * ch
        return out

    def lookups(self):
        """[(stream, begin, end)]: inside F over the marks, at F's last byte, in the tail, in G, in the far small streams, and
        empty ones."""
        f, g, ch = self.f, self.g, CHUNKS[1]
        lf, m = self.lengths[f], self.marks()
        lk = [(f, m["symbol"] - 40, m["symbol"] + 40), (f, m["symbol"], m["symbol"] + 1),
              (f, m["bit"] - 3, m["bit"] + ch + 3), (f, m["byte"] - 3, m["byte"] + ch + 3), (f, m["byte"], m["byte"] + ch),
              (f, lf - 1, lf), (f, lf, lf), (f, lf - 3000, lf), (f, self.P * BLOCK - 7, self.P * BLOCK + 9), (f, 0, 300),
              (g, 0, 0), (g, BLOCK - 5, BLOCK + 5), (g, 2 * BLOCK + 1000, 2 * BLOCK + 3000), (g, 3 * BLOCK - 1, 3 * BLOCK)]
        for i in range(self.g + 1, self.n):
            ln = self.lengths[i]
            lk.append((i, 0, ln) if i % 3 == 0 else (i, ln // 3, ln) if i % 3 == 1 else (i, ln // 2, ln // 2))
        return lk

    def lookup_bytes(self):
        return [self.read(i, b, e) for i, b, e in self.lookups()]


@functools.lru_cache(maxsize=2)
def _draw2(seed):
    """Everything of Far2 but P: (patterns a and b, head, tail, mid, far streams, block, counts, code lengths, codes, draws)."""
    rng = np.random.default_rng([seed, 2])
    alpha = np.concatenate([[PREV0], rng.permutation(np.setdiff1d(np.arange(256), [PREV0]))[:15]]).astype(np.uint8)
    w = 1.0 / np.arange(1, 17) ** 1.2
    text = lambda n: alpha[rng.choice(16, size=n, p=w / w.sum())].tobytes()
    rare = lambda n: alpha[rng.integers(8, 16, size=n)].tobytes()
    c = CHUNKS[0]
    pat_a, pat_b = rare(8), rare(6)
    tail = bytearray(text(4 * c + 37))
    tail[100:108] = pat_a
    tail[2 * c - 3:2 * c + 5] = pat_a
    tail[c - 2:c + 4] = pat_b
    tail[-6:] = pat_b
    head, mid = [text(3000), b"", text(1)], [text(c - 1), text(c)]
    lens = [0, 0, 1, c - 1, c, c + 1, 2 * c + 17, 3001, 255, 256, 257, 2 * 256 + 17, 4999]
    far = [bytearray(text(lens[j % len(lens)])) for j in range(30)]
    far[7][1000:1008] = pat_a
    far[12][-6:] = pat_b
    far[19][5:11] = pat_b
    far = [bytes(m) for m in far] + [b""]
    base = batch_ref.histogram([bytes(tail)] + head + mid + far, 2)
    blk = np.frombuffer(text(BLOCK), dtype=np.uint8).copy()
    blk[-2:] = PREV0
    for draws in range(2000):
        h = batch_ref.histogram([blk.tobytes()], 2)
        counts = h + base
        counts[counts > 0] += np.uint64(1)
        lens2, codes2 = batch_ref.oracle_codes(counts, 2)
        if int((h.astype(np.int64) * lens2).sum()) % 8 == 0:
            break
        blk[-2 - SUFFIX:-2] = np.frombuffer(text(SUFFIX), dtype=np.uint8)
    else:
        raise AssertionError("no block found")
    assert lens2[counts > 0].min() > 0
    return pat_a, pat_b, head, bytes(tail), mid, far, blk.tobytes(), counts, lens2, codes2, draws


class Far2(Far):
    """The same layout for an order-2 source model 'S2' alone.  The block is Zipf text over 16 symbols (codes of many lengths;
    PREV0 is one of them) and ends in two bytes PREV0, so the block behind it, and the tail, start in context (PREV0, PREV0) as
    a stream does: the closed forms of Far hold word for word.  S2 is the oracle's order-2 model of (the histogram of the batch
    at P = 1) + 1 on the live triples only, so every triple of the batch has a code; the SUFFIX bytes in front of the last
    two are drawn again until the block's bit length is 0 modulo 8.  The patterns are made of the rarest symbols."""

    def __init__(self, P=None, seed=SEED):
        self.seed = seed
        self.pat_a, self.pat_b, head, tail, mid, far, self.blk, counts, lens2, codes2, self.draws = _draw2(seed)
        self.counts, self.orders, self.codes, self.src = {"S2": counts}, {"S2": 2}, {"S2": (lens2, codes2)}, "S2"
        self.block_bits = {"S2": int(batch_ref.pack([self.blk], lens2, codes2, 2, PREV0).nbits[0])}
        if P is None:
            P = max(-(-(FAR + FAR_HITS * BLOCK) // BLOCK), FAR // self.block_bits["S2"] + 1)
        self.P = int(P)
        self.streams = [Stream(0, m) for m in head] + [Stream(self.P, tail)] + [Stream(0, m) for m in mid] + [Stream(G_PERIODS, b"")] + \
            [Stream(0, m) for m in far]
        self.f, self.g, self.tail_f = len(head), len(head) + 1 + len(mid), bytes(tail)
        self._finish()
        assert self.blk[-2] == PREV0


@functools.lru_cache(maxsize=4)
def far(P=None, seed=SEED):
    return Far(P, seed)


@functools.lru_cache(maxsize=4)
def far2(P=None, seed=SEED):
    return Far2(P, seed)
