"""The reference of the span tokens (include/mh.h, "TOKENS FROM MATCHED BYTES"): plain Python on the original messages (a
helper module for the tests and tools/token_rate.py).

siphash24 is the published algorithm, a word at a time on the whole byte string; the library absorbs a byte at a time from a
decoder.  table() builds the replacement table the device call must write, entry r for span r; apply() is
splice_table_ref.apply with that table: the scrubbed messages."""
import struct

import numpy as np

import splice_table_ref

M64 = (1 << 64) - 1
FOLD = 1                                   # include/mh.h MH_TOKEN_FOLD
MAX_TOKEN = 255                            # include/mh.h MH_SPLICE_MAX_REP
KEY = bytes(range(16))                     # the key of the published test vectors


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash24(key, data):
    k0, k1 = struct.unpack("<QQ", bytes(key))
    v = [k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573]

    def sipround():
        v[0] = (v[0] + v[1]) & M64; v[1] = _rotl(v[1], 13); v[1] ^= v[0]; v[0] = _rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64; v[3] = _rotl(v[3], 16); v[3] ^= v[2]
        v[0] = (v[0] + v[3]) & M64; v[3] = _rotl(v[3], 21); v[3] ^= v[0]
        v[2] = (v[2] + v[1]) & M64; v[1] = _rotl(v[1], 17); v[1] ^= v[2]; v[2] = _rotl(v[2], 32)

    data = bytes(data)
    n = len(data)
    words = [int.from_bytes(data[k:k + 8], "little") for k in range(0, n - n % 8, 8)]
    words.append(int.from_bytes(data[n - n % 8:], "little") | ((n & 0xff) << 56))
    for m in words:
        v[3] ^= m
        sipround(); sipround()
        v[0] ^= m
    v[2] ^= 0xff
    for _ in range(4):
        sipround()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def fold(data):
    return bytes(c | 0x20 if 0x41 <= c <= 0x5a else c for c in bytes(data))


def digest(key, data, flags=0):
    return siphash24(key, fold(data) if flags & FOLD else data)


def token(fmt, key, data, flags=0):
    """fmt: (prefix, hex_digits, suffix)."""
    prefix, hexd, suffix = fmt
    return bytes(prefix) + ("%016x" % digest(key, data, flags))[:hexd].encode() + bytes(suffix)


def format_arrays(formats):
    """(fmt_off[2 n + 1], fmt_bytes, hex_digits[n]) as the library takes a list of (prefix, hex_digits, suffix)."""
    off, blob = [0], b""
    for prefix, _, suffix in formats:
        blob += bytes(prefix); off.append(len(blob))
        blob += bytes(suffix); off.append(len(blob))
    return (np.asarray(off, dtype=np.uint64), np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(0, dtype=np.uint8),
            np.asarray([h for _, h, _ in formats], dtype=np.uint8))


def formats_ok(formats):
    return all(0 <= h <= 16 and len(p) + h + len(s) <= MAX_TOKEN for p, h, s in formats)


def table(messages, span_off, spans, tags, formats, key, flags=0, failed=()):
    """The table the call writes: entry r is the token of span r (begin >= len: of the empty string), empty for every span of a
    stream in `failed`.  tags None: format 0.  Returns the list of entries."""
    sp = np.asarray(spans, dtype=np.uint64).reshape(-1, 2).tolist()
    out = []
    for i, msg in enumerate(messages):
        msg = bytes(msg)
        for r in range(int(span_off[i]), int(span_off[i + 1])):
            b, e = sp[r]
            f = 0 if tags is None else int(tags[r])
            out.append(b"" if i in failed else token(formats[f], key, msg[b:e], flags))
    return out


def table_arrays(entries, n_reps=None):
    """(rep_off[n_reps + 1], rep_bytes, rep_tag[n_reps]) of a list of entries, padded with empty entries to n_reps."""
    n_reps = len(entries) if n_reps is None else n_reps
    off = np.zeros(n_reps + 1, dtype=np.uint64)
    lens = [len(e) for e in entries] + [0] * (n_reps - len(entries))
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    blob = b"".join(entries)
    return off, np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(0, dtype=np.uint8), np.arange(n_reps, dtype=np.uint32)


def apply(messages, span_off, spans, tags, formats, key, flags=0):
    """The scrubbed messages: every span that begins inside its message replaced by its token."""
    entries = table(messages, span_off, spans, tags, formats, key, flags)
    return splice_table_ref.apply(messages, span_off, spans, range(len(entries)), entries)
