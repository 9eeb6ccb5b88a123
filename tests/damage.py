"""The damaged-stream contract of include/mh.h, computed from the CPU oracle alone (a plain helper module for the tests).

The contract is the reference's `assert(bi == length)` (src/coding.cpp:158) made a status:
  - index-free: the decode from bit 0 in context prev0 must end exactly at nbits, and no context on the way may lack a
    table (a null entry); anything else is MH_ERR_CORRUPT;
  - indexed: every chunk, decoded from its entry, must give chunk_symbols symbols (the last chunk the remainder) and end
    exactly at the next entry's offset, the last one at nbits;
  - lookups / ranges into an indexed stream fail iff a chunk they read fails, where a read that ends inside a chunk is only
    checked for null entries and for running past nbits.
The oracle's mho_decompress is the reference's NDEBUG reading (no end check) and stays as it is; the verdicts here come from
mho_decode_span, which walks the tree bit by bit.  The damage generators are deterministic in their seed and name every case:
D1-D6 damage a payload or its nbits and leave the index alone; X1-X10 damage the chunk index (a sidecar file of its own) and
leave the payload alone.  The verdict functions take the index as an argument and judge either.
"""
import numpy as np

MH_OK, MH_ERR_CORRUPT = 0, -4
IX_SEG_BITS = 352                  # the index builder's segment (csrc/mh_index.hip)
IX_TILE_BITS = 128 * IX_SEG_BITS   # a tile of 128 segments (csrc/mh_tile.hip)
BATCH_SEG_BITS = 512               # the batch segment states' segment (csrc/mh_batch_states.hip)


# ---- positions ------------------------------------------------------------------------------------------------------------
def contexts(data, order=1, prev0=0x20):
    """Context of every symbol of `data`: the previous byte (order 1; prev0 first) or the previous two bytes (order 2)."""
    d = np.asarray(data, dtype=np.uint8).astype(np.int64)
    if order == 0:
        return np.zeros(d.size, dtype=np.int64)
    p1 = np.concatenate([[prev0 & 255], d[:-1]]) if d.size else d
    if order == 1:
        return p1
    p2 = np.concatenate([[(prev0 >> 8) & 255, prev0 & 255], d[:-2]])[:d.size] if d.size else d
    return (p2 << 8) | p1


def code_lengths(lens, data, order=1, prev0=0x20):
    """Length in bits of every symbol's code, lens = the oracle's len8 (ctx * 256 + sym; order 0: row 0)."""
    d = np.asarray(data, dtype=np.uint8).astype(np.int64)
    return np.asarray(lens).astype(np.int64)[contexts(d, order, prev0) * 256 + d]


def boundaries(lens, data, order=1, prev0=0x20):
    """Bit offset of every code boundary: 0, end of symbol 0, ..., nbits (data.size + 1 entries)."""
    return np.concatenate([[0], np.cumsum(code_lengths(lens, data, order, prev0))]).astype(np.int64)


def expected_entries(lens, data, chunk, prev0=0x20, order=1):
    """(chunk index, fine index) of the stream of `data` under code lengths lens[ctx * 256 + sym]: the entries the encoder
    writes (orders 0 and 1: prev << 56 | bit, the byte in front of the chunk also where the model ignores it; order 2:
    ctx << 48 | bit) and the fine index (prev << 24 | bit & 0xFFFFFF, order 1)."""
    d = np.asarray(data, dtype=np.uint8)
    ctx = contexts(d, order, prev0)
    field = contexts(d, 1, prev0) if order == 0 else ctx
    pos = boundaries(lens, d, order, prev0)[:-1]
    j = np.arange(0, d.size, chunk)
    shift = np.uint64(48 if order == 2 else 56)
    index = (field[j].astype(np.uint64) << shift) | pos[j].astype(np.uint64)
    f = np.arange(0, d.size, 64)
    fine = ((ctx[f] << 24) | (pos[f] & 0xFFFFFF)).astype(np.uint32)
    return index, fine


# ---- verdicts ---------------------------------------------------------------------------------------------------------------
def verdict_free(om, payload, nbits, prev0=0x20):
    """Index-free verdict: (MH_OK, bytes) when the decode from bit 0 ends exactly at nbits, else (MH_ERR_CORRUPT, None)."""
    st, out, _, _ = om.decode_span(payload, 0, nbits, prev0)
    assert st in (0, -1), st
    return (MH_OK, out) if st == 0 else (MH_ERR_CORRUPT, None)


def _entry(e, order):
    shift = 48 if order == 2 else 56
    return int(e) & ((1 << shift) - 1), int(e) >> shift


def chunk_verdicts(om, payload, nbits, index, chunk, n_symbols, order=1, only=None):
    """Per chunk (only: of these chunk numbers, in their order): (ok, bytes) of the chunk decoded from its entry with the
    contract's checks."""
    res = []
    nchunks = (n_symbols + chunk - 1) // chunk
    for j in (range(nchunks) if only is None else only):
        bit0, ctx = _entry(index[j], order)
        end = _entry(index[j + 1], order)[0] if j + 1 < nchunks else nbits
        count = min(chunk, n_symbols - j * chunk)
        if bit0 > end or end > nbits:
            res.append((False, None))
            continue
        st, out, _, _ = om.decode_span(payload, bit0, end, ctx, max_symbols=count)
        res.append((st == 0, out if st == 0 else None))
    return res


def verdict_indexed(om, payload, nbits, index, chunk, n_symbols, order=1):
    """Indexed verdict: (MH_OK, bytes) when every chunk passes, else (MH_ERR_CORRUPT, None)."""
    cv = chunk_verdicts(om, payload, nbits, index, chunk, n_symbols, order)
    if all(ok for ok, _ in cv):
        return MH_OK, b"".join(b for _, b in cv)
    return MH_ERR_CORRUPT, None


def verdict_range(om, payload, nbits, index, chunk, n_symbols, begin, end, order=1):
    """A range [begin, end) of an indexed stream: (MH_OK, bytes) iff every chunk it reads passes.  A chunk whose entry lies
    past nbits or behind the entry before it fails every range that touches it (and, through the end check of the chunk in
    front, every range that ends on its start boundary).  A chunk read to its end takes the full chunk check; a read that
    ends inside a chunk decodes end - chunk start symbols from the entry and fails only on a null entry or on running past
    nbits."""
    if begin == end:
        return MH_OK, b""
    nchunks = (n_symbols + chunk - 1) // chunk
    out = b""
    for j in range(begin // chunk, (end - 1) // chunk + 1):
        bit0, ctx = _entry(index[j], order)
        if bit0 > nbits or (j > 0 and bit0 < _entry(index[j - 1], order)[0]):
            return MH_ERR_CORRUPT, None
        cs, ce = j * chunk, min((j + 1) * chunk, n_symbols)
        if end >= ce:
            nxt = _entry(index[j + 1], order)[0] if j + 1 < nchunks else nbits
            if bit0 > nxt or nxt > nbits:
                return MH_ERR_CORRUPT, None
            st, b, _, _ = om.decode_span(payload, bit0, nxt, ctx, max_symbols=ce - cs)
            if st != 0:
                return MH_ERR_CORRUPT, None
        else:
            if bit0 > nbits:
                return MH_ERR_CORRUPT, None
            st, b, ns, _ = om.decode_span(payload, bit0, nbits, ctx, max_symbols=end - cs)
            if ns != end - cs:                      # a null entry or a code past nbits before the last symbol
                return MH_ERR_CORRUPT, None
        out += b[max(begin - cs, 0):end - cs]
    return MH_OK, out


# ---- bits -------------------------------------------------------------------------------------------------------------------
def bits_of(payload):
    return np.unpackbits(np.frombuffer(bytes(payload), dtype=np.uint8))


def with_length(payload, nbits, new_nbits, fill=0):
    """The payload of a stream of new_nbits bits: the original bits up to min(nbits, new_nbits), bits [nbits, new_nbits) set
    to `fill`, then ceil(new_nbits / 8) bytes whose bits after new_nbits are `fill` as well."""
    b = bits_of(payload)[:nbits]
    keep = min(nbits, new_nbits)
    nbytes = (new_nbits + 7) // 8
    out = np.full(nbytes * 8, fill, dtype=np.uint8)
    out[:keep] = b[:keep]
    return np.packbits(out).tobytes()


def cut(payload, nbits, new_nbits):
    """Cut (or extend) to new_nbits, the original bits kept where they exist (what a wrong header remainder gives)."""
    b = bits_of(payload)
    nbytes = (new_nbits + 7) // 8
    out = np.zeros(nbytes * 8, dtype=np.uint8)
    m = min(b.size, out.size)
    out[:m] = b[:m]
    return np.packbits(out).tobytes()


def garbage_after(payload, nbits, fill):
    """The same stream with every bit after nbits (to the end of its bytes) set to `fill`."""
    b = bits_of(payload).copy()
    b[nbits:] = fill
    return np.packbits(b).tobytes()


def flip(payload, bit):
    b = bytearray(payload)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


# ---- damage generators: lists of (name, payload, nbits) ----------------------------------------------------------------------
def d1_end_cuts(payload, nbits, bounds):
    """nbits - k for k = 1 .. (the last three codes' lengths + 1): code boundaries and cuts inside codes."""
    span = int(nbits - bounds[max(len(bounds) - 4, 0)]) + 1
    return [("D1-%d" % k, cut(payload, nbits, nbits - k), nbits - k) for k in range(1, min(span, nbits) + 1)]


def d2_extensions(payload, nbits, kmax=16):
    """nbits + k, the bits after the original end zeros, then ones."""
    out = []
    for fill in (0, 1):
        for k in range(1, kmax + 1):
            out.append(("D2-%s%d" % ("01"[fill], k), with_length(payload, nbits, nbits + k, fill), nbits + k))
    return out


def d3_spread_cuts(payload, nbits, chunk_offsets=(), deltas=(-3, -2, -1, 0, 1, 2, 3), per_kind=2, seed=0):
    """Cuts at and around 352-bit segment, tile, 512-bit batch segment and chunk-entry boundaries, a few of each kind
    spread through the stream (seeded)."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    kinds = [("seg", IX_SEG_BITS), ("tile", IX_TILE_BITS), ("bseg", BATCH_SEG_BITS)]
    for name, step in kinds:
        m = (nbits - 1) // step
        if m < 1:
            continue
        picks = sorted(set([1, m] + [int(x) for x in rng.integers(1, m + 1, per_kind)]))[:per_kind + 1]
        for q in picks:
            for d in deltas:
                c = q * step + d
                if 0 < c < nbits and c not in seen:
                    seen.add(c)
                    out.append(("D3-%s%d%+d" % (name, q, d), cut(payload, nbits, c), c))
    offs = [int(o) for o in chunk_offsets][1:]
    if offs:
        sel = sorted(set([offs[0], offs[-1]] + [offs[int(i)] for i in rng.integers(0, len(offs), per_kind)]))
        for o in sel:
            for d in deltas:
                c = o + d
                if 0 < c < nbits and c not in seen:
                    seen.add(c)
                    out.append(("D3-entry%d%+d" % (o, d), cut(payload, nbits, c), c))
    return out


def d4_flips(payload, nbits, bounds, code_len, n=4, seed=0):
    """Single-bit flips: in the first and in the last 352-bit segment, inside the first code longer than 15 bits (when there
    is one), and at n seeded positions."""
    rng = np.random.default_rng(seed)
    pos = {"first": min(5, nbits - 1), "last": max(nbits - 200, 0)}
    long = np.flatnonzero(code_len > 15)
    if long.size:
        pos["long"] = int(bounds[long[0]]) + int(code_len[long[0]]) // 2
    for i, b in enumerate(rng.integers(0, nbits, n)):
        pos["rnd%d" % i] = int(b)
    return [("D4-%s@%d" % (k, b), flip(payload, b), nbits) for k, b in pos.items()]


def d5_null_entry(om, data, x, extra=12, fill=1):
    """A model in which byte `x` only ends the training data has no table for context x: the stream of data (which ends in
    x) extended by `extra` bits must meet that null entry.  Returns (name, payload, nbits)."""
    assert data[-1] == x and x not in data[:-1]
    blob, nbits = om.compress(bytes(data))
    return ("D5-null+%d" % extra, with_length(blob[1:], nbits, nbits + extra, fill), nbits + extra)


def all_damages(payload, nbits, bounds, code_len, chunk_offsets=(), seed=0, per_kind=2, kmax=16):
    """D1-D4 of one stream, each a (name, payload, nbits)."""
    return (d1_end_cuts(payload, nbits, bounds) + d2_extensions(payload, nbits, kmax)
            + d3_spread_cuts(payload, nbits, chunk_offsets, per_kind=per_kind, seed=seed)
            + d4_flips(payload, nbits, bounds, code_len, seed=seed))


# ---- index damages: lists of (name, damaged slice) ---------------------------------------------------------------------------
# One stream's index slice `sl` (m entries: positions p[k], context fields c[k]), its code boundaries `b`, nbits and the order.
# Where k is free, the first, a middle and the last entry.  A damage that would leave the slice as it is is not returned.
def pos_shift(order):
    return 48 if order == 2 else 56


def pos_mask(order):
    return (1 << pos_shift(order)) - 1


def _split(sl, order):
    sh, mk = pos_shift(order), pos_mask(order)
    return [int(e) & mk for e in sl], [int(e) >> sh for e in sl]


def _join(p, c, order):
    sh, mk = pos_shift(order), pos_mask(order)
    return np.array([((ci << sh) | (pi & mk)) & 0xFFFFFFFFFFFFFFFF for pi, ci in zip(p, c)], dtype=np.uint64)


def _picks(m, first=0, ks=None):
    """The entries a damage is placed on: the first, a middle and the last one, or those of `ks` that exist."""
    return sorted({k for k in ((first, m // 2, m - 1) if ks is None else ks) if first <= k < m})


def _moved(sl, order, name, k, new_pos, out):
    p, c = _split(sl, order)
    if 0 <= new_pos <= pos_mask(order) and new_pos != p[k]:
        p[k] = new_pos
        out.append((name, _join(p, c, order)))


def x1_off_by_one(sl, b, nbits, order, ks=None):
    """p[k] +- 1."""
    out, (p, _) = [], _split(sl, order)
    for k in _picks(len(p), 0, ks):
        for d in (-1, 1):
            _moved(sl, order, "X1-e%d%+d" % (k, d), k, p[k] + d, out)
    return out


def x2_other_boundary(sl, b, nbits, order, ks=None):
    """p[k] moved to the code boundary one symbol earlier and one symbol later."""
    out, (p, _) = [], _split(sl, order)
    bl = [int(x) for x in b]
    for k in _picks(len(p), 0, ks):
        j = bl.index(p[k])
        for d in (-1, 1):
            if 0 <= j + d < len(bl):
                _moved(sl, order, "X2-e%d%+dsym" % (k, d), k, bl[j + d], out)
    return out


def x3_at_and_past_the_end(sl, b, nbits, order, ks=None):
    """p[k] = nbits, nbits + 1 and the mask itself, for inner entries and for the last one."""
    out = []
    for k in _picks(len(sl), 1, ks) or [0]:
        for what, v in (("nbits", nbits), ("nbits+1", nbits + 1), ("mask", pos_mask(order))):
            _moved(sl, order, "X3-e%d=%s" % (k, what), k, v, out)
    return out


def x4_behind_the_predecessor(sl, b, nbits, order, ks=None):
    """p[k] = p[k-1] - 1, p[k] = p[k-1] (an empty chunk k - 1) and p[k] = 0, k >= 1."""
    out, (p, _) = [], _split(sl, order)
    for k in _picks(len(p), 1, ks):
        for what, v in (("pred-1", p[k - 1] - 1), ("pred", p[k - 1]), ("0", 0)):
            _moved(sl, order, "X4-e%d=%s" % (k, what), k, v, out)
    return out


def x5_entry_0(sl, b, nbits, order, ks=None):
    """p[0] = 1 and p[0] = p[1]."""
    out, (p, _) = [], _split(sl, order)
    if p:
        _moved(sl, order, "X5-e0=1", 0, 1, out)
    if len(p) > 1:
        _moved(sl, order, "X5-e0=e1", 0, p[1], out)
    return out


def x6_swapped_and_shifted(sl, b, nbits, order, ks=None):
    """Neighbours swapped; the whole slice shifted by one entry, either way."""
    out, m = [], len(sl)
    for k in _picks(m - 1, 0, ks):
        s = np.array(sl, dtype=np.uint64)
        s[k], s[k + 1] = sl[k + 1], sl[k]
        out.append(("X6-swap%d,%d" % (k, k + 1), s))
    if m > 1:
        out.append(("X6-shift-1", np.concatenate([sl[1:], sl[-1:]]).astype(np.uint64)))
        out.append(("X6-shift+1", np.concatenate([sl[:1], sl[:-1]]).astype(np.uint64)))
    return [(n, s) for n, s in out if not np.array_equal(s, sl)]


def x7_bits_a_32_bit_compare_drops(sl, b, nbits, order, ks=None):
    """p[k] + 2^32, and the top position bit set."""
    out, (p, _) = [], _split(sl, order)
    for k in _picks(len(p), 0, ks):
        _moved(sl, order, "X7-e%d+2^32" % k, k, p[k] + (1 << 32), out)
        _moved(sl, order, "X7-e%d|top" % k, k, p[k] | (1 << (pos_shift(order) - 1)), out)
    return out


def live_contexts(lens, order):
    """Context numbers with a table (some symbol has a code) under code lengths lens[ctx * 256 + sym]."""
    n = {0: 1, 1: 256, 2: 65536}[order]
    return np.flatnonzero(np.asarray(lens)[:n * 256].reshape(n, 256).max(axis=1) > 0)


def x8_context_field(sl, b, nbits, order, lens=None, seed=0, n_live=3, values=None, entries=None):
    """The context field changed, the position kept.  Orders 0 and 1: a context with no table (when the model has one), n_live
    live contexts, entry 0's context.  Order 2: the high byte alone, the low byte alone (each to a byte that some live context
    carries there), and a pair with no table.  values: these field values instead; entries: these entries instead of the picks."""
    rng = np.random.default_rng(seed)
    out, (p, c) = [], _split(sl, order)
    ks = _picks(len(p), 0, entries)
    live = live_contexts(lens, order) if lens is not None else np.zeros(0, dtype=np.int64)
    for k in ks:
        if values is not None:
            cand = [("=%#x" % v, int(v)) for v in values]
        elif order == 2:
            lv = set(int(x) for x in live)
            dead = [v for v in (int(x) for x in rng.integers(0, 65536, 64)) if v not in lv]
            hi = int(live[int(rng.integers(0, live.size))]) >> 8 if live.size else (c[k] >> 8) ^ 1
            lo = int(live[int(rng.integers(0, live.size))]) & 255 if live.size else (c[k] & 255) ^ 1
            if hi == c[k] >> 8:
                hi ^= 1
            if lo == c[k] & 255:
                lo ^= 1
            cand = [("hi=%#x" % hi, (hi << 8) | (c[k] & 255)), ("lo=%#x" % lo, (c[k] & 0xFF00) | lo)]
            if dead:
                cand.append(("dead=%#x" % dead[0], dead[0]))
        else:
            nctx = 256
            lv = set(int(x) for x in live) if order == 1 else set(range(256))
            dead = [v for v in range(nctx) if v not in lv]
            cand = [("dead=%#x" % dead[len(dead) // 2], dead[len(dead) // 2])] if dead else []
            pool = sorted(lv - {c[k]})
            for v in (rng.choice(pool, size=min(n_live, len(pool)), replace=False) if pool else []):
                cand.append(("live=%#x" % int(v), int(v)))
            cand.append(("e0ctx=%#x" % c[0], c[0]))
        for what, v in cand:
            if v != c[k]:
                cc = list(c)
                cc[k] = v
                out.append(("X8-e%d%s" % (k, what), _join(p, cc, order)))
    return out


def x9_whole_entry(sl, b, nbits, order, ks=None):
    """The whole entry zero, and all ones."""
    out = []
    for k in _picks(len(sl), 0, ks):
        for what, v in (("zero", 0), ("ones", 0xFFFFFFFFFFFFFFFF)):
            if int(sl[k]) != v:
                s = np.array(sl, dtype=np.uint64)
                s[k] = np.uint64(v)
                out.append(("X9-e%d=%s" % (k, what), s))
    return out


def x10_gaps(index, bases, sizes):
    """A batch index with every entry between the slices (slice i: index[bases[i] : bases[i] + sizes[i]]) all ones: still a
    valid batch.  Returns (name, index)."""
    keep = np.zeros(len(index), dtype=bool)
    for a, m in zip(bases, sizes):
        keep[int(a):int(a) + int(m)] = True
    out = np.array(index, dtype=np.uint64)
    out[~keep] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return "X10-gaps", out


INDEX_KINDS = {"X1": x1_off_by_one, "X2": x2_other_boundary, "X3": x3_at_and_past_the_end, "X4": x4_behind_the_predecessor,
               "X5": x5_entry_0, "X6": x6_swapped_and_shifted, "X7": x7_bits_a_32_bit_compare_drops, "X8": x8_context_field,
               "X9": x9_whole_entry}


def index_damages(sl, b, nbits, order, lens=None, seed=0, kinds=None, ks=None):
    """X1-X9 of one stream's slice, each a (name, damaged slice); the kind is the name up to the first '-'.  ks: the entries to
    damage instead of the first, a middle and the last one."""
    out = []
    for kind in kinds or sorted(INDEX_KINDS, key=lambda s: int(s[1:])):
        fn = INDEX_KINDS[kind]
        out += fn(sl, b, nbits, order, lens, seed, entries=ks) if kind == "X8" else fn(sl, b, nbits, order, ks)
    return out


def flat_counts(seed=0):
    """Order-1 counts drawn uniformly in [100, 200) for all 65 536 pairs: every context has a table and every code 8 bits, so
    a chunk decoded from any other context byte still ends on its end bit, with other bytes."""
    return np.random.default_rng(seed).integers(100, 200, 65536).astype(np.uint64)
