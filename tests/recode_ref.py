"""The reference of re-coding (include/mh.h, "RE-CODING BATCHES"): plain Python/numpy on the original messages, on top of the
CPU oracle (a helper module for the tests and tools/recode_rate.py; it never sees a compressed byte of the source).

Re-coding a batch under `dst` must give what encoding the original messages under `dst` gives, so the reference is the
oracle's encoder (oracle.Model.compress, the reference's NDEBUG reading: a (prev, sym) pair without a code is skipped and the
context advances) plus the oracle's length table for the dropped symbols and the index entries."""
import numpy as np

PREV0 = 0x20


def contexts(message, order, prev0=PREV0):
    """The context of every symbol: the byte in front of it (order 1; prev0 first), or 0 (order 0)."""
    d = np.frombuffer(bytes(message), dtype=np.uint8).astype(np.int64)
    if order == 0 or d.size == 0:
        return np.zeros(d.size, dtype=np.int64)
    return np.concatenate([[prev0 & 255], d[:-1]])


def code_lengths(lens, message, order, prev0=PREV0):
    """Bits of every symbol's code under the oracle's len8 (prev * 256 + sym; an order-0 model: row 0); 0 = no code."""
    d = np.frombuffer(bytes(message), dtype=np.uint8).astype(np.int64)
    return np.asarray(lens).astype(np.int64)[contexts(message, order, prev0) * 256 + d]


def dropped(lens, message, order, prev0=PREV0):
    """Symbols of `message` without a code under the model."""
    return int((code_lengths(lens, message, order, prev0) == 0).sum())


def index_slice(lens, message, order, chunk, prev0=PREV0):
    """The chunk index of the message's stream: (byte in front of the chunk) << 56 | bit offset of its first symbol."""
    d = np.frombuffer(bytes(message), dtype=np.uint8).astype(np.int64)
    if d.size == 0:
        return np.zeros(0, dtype=np.uint64)
    pos = np.concatenate([[0], np.cumsum(code_lengths(lens, message, order, prev0))])[:-1]
    before = np.concatenate([[prev0 & 255], d[:-1]])
    j = np.arange(0, d.size, chunk)
    return (before[j].astype(np.uint64) << np.uint64(56)) | pos[j].astype(np.uint64)


def recode(messages, dst, chunk=0):
    """What a re-code of `messages` under the oracle model `dst` must give: a list of (payload bytes, nbits, dropped, index
    slice or None) per message.  The oracle starts every message in context PREV0."""
    lens, _ = dst.codes()
    order = dst.type
    out = []
    for m in messages:
        m = bytes(m)
        blob, nbits = dst.compress(m)
        assert (nbits + 7) // 8 == len(blob) - 1
        assert nbits == int(code_lengths(lens, m, order).sum())
        out.append((blob[1:], nbits, dropped(lens, m, order), index_slice(lens, m, order, chunk) if chunk else None))
    return out


def packed(ref):
    """(payload, out_off[n + 1], nbits[n], dropped[n]) of recode()'s result, packed as a batch."""
    off = np.zeros(len(ref) + 1, dtype=np.uint64)
    if ref:
        off[1:] = np.cumsum([len(r[0]) for r in ref], dtype=np.uint64)
    return (np.frombuffer(b"".join(r[0] for r in ref), dtype=np.uint8), off, np.array([r[1] for r in ref], dtype=np.uint64),
            np.array([r[2] for r in ref], dtype=np.uint64))
