"""A plain Python model of the segment-state speculation for order-2 batches (kernels: mh_batch_states.hip):
the speculation, the 8 Jacobi repair passes over ping-pong records and the mark pass, on the oracle's order-2 codes of a model
trained on the batch.  It answers one question without a GPU: how many segment entries are still wrong after the
speculation and after each pass, and how many streams are left to the one-lane walk.  Two rules:

  today     the order-0/1 rule: 256 warm-up bits from (prev0, prev0), no recovery (a null entry: the guess is (prev0, prev0) at
            the segment start)
  recover   the order-2 rule: the whole predecessor segment (512 bits) from (prev0, prev0); in a context without codes go on in
            rep[b], the heaviest live context ending in the same byte, at the same bit (none: (prev0, prev0), one bit on); a
            live context whose codes the bits do not match skips one bit

Bits past the end of a payload read as zeros.  A helper module like batch_ref.py: numpy and the oracle, never the library.

As a script it runs the two long inputs of DESIGN 3.20 (about a minute each):  python tests/states_o2_ref.py"""
import os
import sys

import numpy as np

SEG_BITS = 512
WARMUP_TODAY = 256
REPAIR_PASSES = 8
PREV0 = 0x20
BAD = None


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


def text(n, seed=0):
    """Words and line breaks; a long text repeats a 1 MiB block (the generator of tests/test_gpu_batch_states.py)."""
    words = [b"the", b"segment", b"state", b"of", b"a", b"stream", b"decoder", b"batch", b"index", b"huffman", b"markov"]
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < min(n, 1 << 20):
        out += words[int(rng.integers(len(words)))] + (b"\n" if rng.random() < 0.1 else b" ")
    return (bytes(out) * (n // len(out) + 1))[:n] if out else b""


class Tables:
    """Per live context: its code lengths in ascending order and {bit string: symbol}; rep[256] as the model build defines it
    (weight = the context's total count, ties to the smaller first byte; 0xFFFF: none)."""

    def __init__(self, counts, lens, codes):
        lens2 = np.asarray(lens).reshape(65536, 256)
        codes2 = np.asarray(codes).reshape(65536, 256)
        self.ctx = {}
        for c in np.nonzero(lens2.any(axis=1))[0]:
            by = {}
            for s in np.nonzero(lens2[c])[0]:
                l = int(lens2[c, s])
                by[format(int(codes2[c, s]), "0%db" % l)] = int(s)
            self.ctx[int(c)] = (sorted({len(k) for k in by}), by)
        weight = np.asarray(counts, dtype=np.uint64).reshape(65536, 256).sum(axis=1)
        self.rep = [0xFFFF] * 256
        best = [0] * 256
        for c in sorted(self.ctx):
            b = c & 255
            if self.rep[b] == 0xFFFF or int(weight[c]) > best[b]:
                self.rep[b], best[b] = c, int(weight[c])

    def step(self, bits, pos, ctx):
        """(next context, code length), "dead" (no codes in ctx) or "nomatch"."""
        t = self.ctx.get(ctx)
        if t is None:
            return "dead"
        for l in t[0]:
            s = t[1].get(bits[pos:pos + l])
            if s is not None:
                return ((ctx << 8) | s) & 0xFFFF, l
        return "nomatch"


def decode_seg(tab, bits, entry, lim):
    """(entry, end, count): decodes from entry while the position is below lim; end BAD on a null entry."""
    ctx, pos = entry
    n = 0
    while pos < lim:
        r = tab.step(bits, pos, ctx)
        if isinstance(r, str):
            return entry, BAD, n
        ctx, pos, n = r[0], pos + r[1], n + 1
    return entry, (ctx, pos), n


def guess_today(tab, bits, ctx0, at, stats):
    _, end, _ = decode_seg(tab, bits, (ctx0, at - WARMUP_TODAY), at)
    if end is BAD:
        stats["null_warmups"] += 1
        return ctx0, at
    return end


def guess_recover(tab, bits, ctx0, at, stats, warmup=SEG_BITS):
    ctx, pos = ctx0, max(at - warmup, 0)
    while pos < at:
        r = tab.step(bits, pos, ctx)
        if r == "dead":
            rb = tab.rep[ctx & 255]
            if rb != 0xFFFF and rb != ctx:
                ctx = rb
            else:
                ctx, pos = ctx0, pos + 1
        elif r == "nomatch":
            pos += 1
        else:
            ctx, pos = r[0], pos + r[1]
    return ctx, pos


def stream_states(tab, payload, nbits, prev0, guess, stats):
    """Wrong entries of one stream after the speculation and after each repair pass (REPAIR_PASSES + 1 figures), its number
    of segments, and whether the mark pass leaves it to the walk."""
    bits = (np.unpackbits(np.asarray(payload, dtype=np.uint8)) + np.uint8(ord("0"))).tobytes().decode("ascii") + "0" * 128
    ctx0 = (prev0 << 8) | prev0
    nseg = (nbits + SEG_BITS - 1) // SEG_BITS if nbits else 1
    lim = lambda k: min((k + 1) * SEG_BITS, nbits)
    rec = [decode_seg(tab, bits, (ctx0, 0) if k == 0 else guess(tab, bits, ctx0, k * SEG_BITS, stats), lim(k)) for k in range(nseg)]
    wrong = lambda r: sum(1 for k in range(1, nseg) if r[k - 1][1] is BAD or r[k - 1][1] != r[k][0])
    hist = [wrong(rec)]
    for _ in range(REPAIR_PASSES):
        new = list(rec)
        for k in range(1, nseg):
            pe = rec[k - 1][1]
            if pe is not BAD and pe != rec[k][0]:
                new[k] = decode_seg(tab, bits, pe, lim(k))
        rec = new
        hist.append(wrong(rec))
    return hist, nseg, hist[-1] != 0


def run(messages, rule, prev0=PREV0, train_extra=()):
    """The model of one batch: {"segments", "wrong" (after the speculation and each pass), "walked" (streams left to the walk),
    "streams", "null_warmups" (today's rule), "nbits"}.  The model is trained on the batch (and on train_extra)."""
    import batch_ref
    counts = batch_ref.histogram(list(messages) + list(train_extra), 2, prev0)
    lens, codes = batch_ref.oracle_codes(counts, 2)
    p = batch_ref.pack(messages, lens, codes, 2, prev0)
    tab = Tables(counts, lens, codes)
    guess = {"today": guess_today, "recover": guess_recover}[rule]
    stats = {"null_warmups": 0}
    total = np.zeros(REPAIR_PASSES + 1, dtype=np.int64)
    segs = walked = 0
    for i in range(len(messages)):
        pl = p.payload[int(p.pay_off[i]):int(p.pay_off[i + 1])]
        hist, nseg, left = stream_states(tab, pl, int(p.nbits[i]), prev0, guess, stats)
        total += hist
        segs += nseg
        walked += left
    return {"segments": segs, "wrong": total.tolist(), "walked": walked, "streams": len(messages), "null_warmups": stats["null_warmups"],
            "nbits": p.nbits}


def wiki_lines():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "inputs", "input_wiki_cpp.html"), "rb") as f:
        return [ln for ln in f.read().split(b"\n") if ln]


def text_batch():
    return [text(8192, s) for s in range(30)]


def zipf_batch():
    return [zipf(4096, s) for s in range(40)]


def long_batch(gen, size):
    """One long stream among 20 small ones (the shape of the GPU test's over-the-cap batches)."""
    rng = np.random.default_rng(11)
    msgs = [gen(int(k), int(s)) for s, k in enumerate(rng.integers(0, 4096, 21))]
    msgs[17] = gen(size, 102)
    return msgs


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, msgs in (("one 8 MiB text stream + 20 small", long_batch(text, 8 << 20)), ("one 3 MiB Zipf stream + 20 small", long_batch(zipf, 3 << 20))):
        r = run(msgs, "recover")
        print("%s: %.2f Mbit in stream 17, %d segments, wrong %s, %d of %d streams walked" % (
            name, int(r["nbits"][17]) / 1e6, r["segments"], r["wrong"], r["walked"], r["streams"]), flush=True)
