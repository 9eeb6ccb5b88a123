"""Re-coding compressed batches on the GPU (include/mh.h, "RE-CODING BATCHES"): the histogram of a compressed batch and the
batch coded again under another model, under a shared source model and per-stream models, with and without the chunk index.
The references are mh_encode_batch(dst) of the original messages, tests/recode_ref.py (the CPU oracle's encoder) and, through
files, the bytes the reference program wrote (tests/golden/recode/X__Y.cm = input X under table Y.e).  The device-call
wrappers put guards around every output and assert that nothing outside the results changed."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
import recode_ref
from conftest import GOLDEN_DIR, ROOT, expected_file, golden
from oracle import mh_oracle

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


def shared_model(mhc, msgs, order):
    return mhc.Model.from_counts(mhc.histogram_o1_batch(msgs, order=order), order)


class Source:
    """A batch coded under one shared model, or (each=True) one model per stream, with an index of `chunk`."""

    def __init__(self, mhc, msgs, chunk, order=1, each=False, model=None):
        self.mhc, self.msgs, self.chunk, self.each = mhc, [bytes(m) for m in msgs], chunk, each
        if each:
            self.model = mhc.ModelSet.train(self.msgs, order=order)
            self.payload, self.pay_off, self.nbits, self.index, self.sym_off, rc = self.model.encode(self.msgs, chunk_symbols=chunk)
            assert rc == mhc.MH_OK
        else:
            self.model = model or shared_model(mhc, self.msgs, order)
            self.payload, self.pay_off, self.nbits, self.index, self.sym_off = self.model.encode_batch(self.msgs, chunk_symbols=chunk)

    def kw(self, indexed):
        return dict(sym_off=self.sym_off, index=self.index, chunk_symbols=self.chunk) if indexed else dict(chunk_symbols=self.chunk)

    def recode(self, dst, indexed, payload=None, pay_off=None, nbits=None, **kw):
        fn = self.model.recode if self.each else self.model.dev_recode_batch
        return fn(dst, self.payload if payload is None else payload, self.pay_off if pay_off is None else pay_off,
                  self.nbits if nbits is None else nbits, **self.kw(indexed), **kw)

    def histogram(self, order, indexed, payload=None, pay_off=None, nbits=None):
        fn = self.model.histogram_coded if self.each else self.model.dev_histogram_coded
        kw = self.kw(indexed) if indexed else {}
        return fn(order, self.payload if payload is None else payload, self.pay_off if pay_off is None else pay_off,
                  self.nbits if nbits is None else nbits, **kw)


def slices(mhc, idx, sym_off, chunk, only=None):
    """The index entries of every stream (or of the streams in `only`), concatenated."""
    out = []
    for i in range(len(sym_off) - 1):
        if only is not None and i not in only:
            continue
        b = int(sym_off[i]) // chunk + i
        out.append(np.asarray(idx[b:b + (int(sym_off[i + 1] - sym_off[i]) + chunk - 1) // chunk], dtype=np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def check_parity(mhc, src, dst, dst_order, what, oracle=True):
    """Indexed and index-free re-code of `src` under `dst` against mh_encode_batch(dst) of the messages, the oracle and a decode."""
    msgs, chunk, n = src.msgs, src.chunk, len(src.msgs)
    w_pay, w_off, w_nb, w_idx, w_so = dst.encode_batch(msgs, chunk_symbols=chunk)
    om = mh_oracle.Model.from_table(dst.table_bytes())
    lens, _ = om.codes()
    w_drop = [recode_ref.dropped(lens, m, dst_order) for m in msgs]
    if oracle:
        r_pay, r_off, r_nb, r_drop = recode_ref.packed(recode_ref.recode(msgs, om))
        assert np.array_equal(r_pay, w_pay) and np.array_equal(r_off, w_off) and np.array_equal(r_nb, w_nb), what
    for indexed in (True, False):
        tag = "%s indexed=%s" % (what, indexed)
        got = src.recode(dst, indexed)
        assert got["rc"] == mhc.MH_OK and (got["status"] == mhc.MH_OK).all(), (tag, got["rc"], np.unique(got["status"]))
        assert np.array_equal(got["out_off"], w_off) and np.array_equal(got["nbits"], w_nb), tag
        assert np.array_equal(got["payload"], w_pay), tag
        assert got["dropped"].tolist() == w_drop, tag
        assert np.array_equal(got["sym_off"], w_so), tag
        assert np.array_equal(slices(mhc, got["index"], w_so, chunk), slices(mhc, w_idx, w_so, chunk)), tag
        count = src.recode(dst, indexed, count_only=True)
        for k in ("out_off", "nbits", "dropped", "status", "sym_off"):
            assert np.array_equal(count[k], got[k]), (tag, k)
        assert count["payload"] is None and count["rc"] == mhc.MH_OK
    if not any(w_drop):
        back, so, st = dst.decode_batch(got["payload"], got["out_off"], got["nbits"], sym_off=w_so, index=got["index"], chunk_symbols=chunk)
        assert back == b"".join(msgs), what


@pytest.fixture(scope="module")
def golden_lines():
    lines = []
    for name in ("input_a.txt", "input_b.txt", "input_ipsum.txt", "input_wiki_cpp.html", "input_wiki_cpp.txt"):
        lines += [l for l in golden()[name]["data"].split(b"\n")]
    assert len(lines) == 2377 and lines.count(b"") == 283 and max(len(l) for l in lines) == 21588
    return lines


@pytest.mark.parametrize("each", [False, True])
def test_golden_lines_recode_as_the_encoder_codes_them(mhc, golden_lines, each):
    src = Source(mhc, golden_lines, 256, each=each)
    wiki = [l for l in golden()["input_wiki_cpp.html"]["data"].split(b"\n")]
    check_parity(mhc, src, shared_model(mhc, golden_lines[::2], 1), 1, "half-trained dst each=%s" % each)      # some pairs have no code
    check_parity(mhc, src, shared_model(mhc, golden_lines, 1), 1, "covering dst each=%s" % each)
    check_parity(mhc, src, shared_model(mhc, wiki, 0), 0, "order-0 dst each=%s" % each, oracle=False)


@pytest.fixture(scope="module")
def ragged():
    lens = [0, 1, 5000, 0, 256, 257, 1, 70001, 1024, 3, 0]
    msgs = [zipf(k, 100 + i) for i, k in enumerate(lens)]
    assert 70001 % 256 != 0
    return msgs


@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("so,do", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_ragged_batch_all_order_pairs(mhc, ragged, so, do, each):
    src = Source(mhc, ragged, 1024, order=so, each=each)
    dst = mhc.Model.from_counts(mhc.histogram_o1_batch([zipf(200000, 7)], order=do), do)
    check_parity(mhc, src, dst, do, "ragged %d->%d each=%s" % (so, do, each))


def test_limited_form_of_the_same_counts(mhc, ragged):
    counts = mhc.histogram_o1_batch(ragged)
    src = Source(mhc, ragged, 512, model=mhc.Model.from_counts(counts, 1))
    dst = mhc.Model.from_counts(counts, 1, max_len=12)
    assert dst.max_code_len <= 12 < src.model.max_code_len
    check_parity(mhc, src, dst, 1, "to the L=12 form")


@pytest.mark.parametrize("indexed", [True, False])
def test_identity(mhc, ragged, indexed):
    src = Source(mhc, ragged, 256)
    got = src.recode(src.model, indexed)
    assert got["rc"] == mhc.MH_OK and not got["dropped"].any()
    assert np.array_equal(got["payload"], src.payload) and np.array_equal(got["out_off"], src.pay_off) and np.array_equal(got["nbits"], src.nbits)
    assert np.array_equal(slices(mhc, got["index"], src.sym_off, 256), slices(mhc, src.index, src.sym_off, 256))


# (input X, table Y, Y covers X).  union_ipsum_wiki.e is the table the reference program trained on input_ipsum.txt followed by
# input_wiki_cpp.txt (tests/golden/recode/): it covers both, so full coverage is checked on 40 KB files, not only on 11 bits.
PAIRS = [("input_a.txt", "input_b.txt", True), ("input_ipsum.txt", "union_ipsum_wiki", True), ("input_wiki_cpp.txt", "union_ipsum_wiki", True),
         ("input_wiki_cpp.txt", "input_wiki_cpp.html", False), ("input_ipsum.txt", "input_wiki_cpp.html", False),
         ("input_wiki_cpp.html", "input_ipsum.txt", False)]


def table_of(y):
    t = expected_file(y, "e")
    if t is None:
        with open(os.path.join(GOLDEN_DIR, "recode", y + ".e"), "rb") as f:
            t = f.read()
    return t


@pytest.mark.parametrize("x,y,covered", PAIRS)
def test_golden_cm_recoded_equals_the_reference_s_file(mhc, x, y, covered):
    data = golden()[x]["data"]
    src_cm, src_tab, dst_tab = expected_file(x, "cm"), expected_file(x, "e"), table_of(y)
    with open(os.path.join(GOLDEN_DIR, "recode", "%s__%s.cm" % (x, y)), "rb") as f:
        want = f.read()
    src, dst = mhc.Model.from_table(src_tab), mhc.Model.from_table(dst_tab)
    lens, _ = mh_oracle.Model.from_table(dst_tab).codes()
    drop = recode_ref.dropped(lens, data, 1)
    assert (drop == 0) == covered
    nb = mhc.parse_stream_header(1, src_cm)
    nbits = nb[0] if isinstance(nb, tuple) else nb
    payload = np.frombuffer(src_cm[1:], dtype=np.uint8)
    got = src.dev_recode_batch(dst, payload, [0, payload.size], [nbits], chunk_symbols=1024)          # index-free: what the reference wrote
    assert got["rc"] == mhc.MH_OK and got["status"].tolist() == [mhc.MH_OK] and got["dropped"].tolist() == [drop]
    assert int(got["sym_off"][1]) == len(data)
    blob = bytes([mhc.lib().mh_stream_header(dst.handle, int(got["nbits"][0]))]) + got["payload"].tobytes()
    assert blob == want
    host = src.recode_batch(dst, payload, [0, payload.size], [nbits], chunk_symbols=1024)
    assert bytes(host["payload"]) == want[1:] and host["dropped"].tolist() == [drop] and host["rc"] == mhc.MH_OK
    # the index it came with serves the indexed path, which gives the same bytes
    again = src.dev_recode_batch(src, payload, [0, payload.size], [nbits], chunk_symbols=1024)
    got2 = src.dev_recode_batch(dst, payload, [0, payload.size], [nbits], sym_off=again["sym_off"], index=again["index"], chunk_symbols=1024)
    assert got2["payload"].tobytes() == want[1:] and np.array_equal(got2["index"], got["index"])


@pytest.mark.parametrize("x,y,covered", PAIRS)
def test_cli_recode_writes_the_reference_s_file(mhc, tmp_path, x, y, covered):
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    data = golden()[x]["data"]
    with open(os.path.join(GOLDEN_DIR, "recode", "%s__%s.cm" % (x, y)), "rb") as f:
        want = f.read()
    p = lambda n: str(tmp_path / n)
    for n, b in (("x", data), ("x.cm", expected_file(x, "cm")), ("x.e", expected_file(x, "e")), ("y.e", table_of(y))):
        with open(p(n), "wb") as f:
            f.write(b)
    run = lambda a: subprocess.run([cli] + a, capture_output=True, timeout=300)
    r = run([p("x.cm"), "-x", "-e", p("x.e"), "--recode", p("y.e"), "-o", p("out.cm")])
    assert r.returncode == 0, r.stderr
    assert open(p("out.cm"), "rb").read() == want and not os.path.exists(p("out.cm.idx"))
    assert (b"no code in the new table" in r.stderr) == (not covered)
    # with the index the encoder writes: the indexed path, the same bytes, and the output's own index beside it
    assert run([p("x"), "-e", p("x.e"), "-o", p("x2.cm"), "--index", p("x.idx")]).returncode == 0
    assert run([p("x"), "-e", p("y.e"), "-o", p("y2.cm"), "--index", p("y.idx")]).returncode == 0
    r = run([p("x2.cm"), "-x", "-e", p("x.e"), "--recode", p("y.e"), "-o", p("out2.cm"), "--index", p("x.idx")])
    assert r.returncode == 0, r.stderr
    assert open(p("out2.cm"), "rb").read() == want
    assert open(p("out2.cm.idx"), "rb").read() == open(p("y.idx"), "rb").read()


@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("indexed", [True, False])
def test_histogram_of_a_compressed_batch(mhc, ragged, golden_lines, indexed, each):
    for msgs, chunk in ((ragged, 256), (golden_lines, 1024)):
        src = Source(mhc, msgs, chunk, each=each)
        for order in (0, 1):
            counts, st, rc = src.histogram(order, indexed)
            assert rc == mhc.MH_OK and (st == mhc.MH_OK).all()
            assert np.array_equal(counts, mhc.histogram_o1_batch(msgs, order=order)), (indexed, each, order)
    counts, _, _ = src.histogram(1, indexed)
    d_counts = mhc.DeviceBuffer(counts.nbytes, counts)
    assert mhc.Model.from_device_counts(d_counts.ptr, 1).table_bytes() == shared_model(mhc, golden_lines, 1).table_bytes()


def test_histogram_counts_past_two_to_the_32(mhc):
    """One pair more than 2^32 times without a multi-GiB buffer: after 'a' only 'a' follows, a one-bit code, so a stream of
    2^23 zero bits is 2^23 times (a, a); 520 such streams are 4.36e9 pairs in 545 MB of zero payload."""
    counts = np.zeros(65536, dtype=np.uint64)
    counts[ord("a") * 256 + ord("a")] = 9
    model = mhc.Model.from_counts(counts, 1)
    per, n = 1 << 23, 520
    payload = np.zeros(n * per // 8, dtype=np.uint8)
    pay_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(per // 8)
    got, st, rc = model.dev_histogram_coded(1, payload, pay_off, np.full(n, per, dtype=np.uint64), prev0=ord("a"))
    assert rc == mhc.MH_OK and (st == mhc.MH_OK).all()
    assert int(got[ord("a") * 256 + ord("a")]) == n * per > 1 << 32 and int(got.sum()) == n * per


def dev_decode_statuses(mhc, src, payload, pay_off, nbits, sym_off=None, index=None, chunk_symbols=0):
    """Per-stream statuses and the status word of one mh_dev_decode_batch / mh_dev_decode_each call on these arguments."""
    l = mhc.lib()
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    D = mhc.DeviceBuffer
    d_pl = D(max(payload.size, 1) + 64, payload if payload.size else None)
    d_po, d_nb = D(pay_off.nbytes, pay_off), D(max(nbits.nbytes, 8), nbits)
    if index is not None:
        so = np.ascontiguousarray(sym_off, dtype=np.uint64)
        cap, total = int(so[n]), int(so[n])
        d_idx = D(max(index.nbytes, 8), np.ascontiguousarray(index, dtype=np.uint64))
    else:
        so = np.zeros(n + 1, dtype=np.uint64)
        cap, total, d_idx = int(sum(int(x) for x in nbits)), 0, None
    d_so, d_out, d_st = D(so.nbytes, so), D(max(cap, 1) + 64), D(max(n, 1) * 4)
    fn, ws = (l.mh_dev_decode_each, l.mh_dev_decode_each_workspace) if src.each else (l.mh_dev_decode_batch, l.mh_dev_decode_batch_workspace)
    wsb = ws(n)
    d_ws = D(wsb)
    rc = fn(src.model.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), 0x20, d_out.ptr, cap, d_so.ptr, total,
            d_idx.ptr if d_idx else None, chunk_symbols, d_st.ptr, d_ws.ptr, wsb, None)
    assert rc == mhc.MH_OK
    return d_st.download(np.int32)[:n], l.mh_dev_status(d_ws.ptr, None)


@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("indexed", [True, False])
def test_damaged_streams_get_the_decoder_s_verdict(mhc, indexed, each):
    chunk = 256
    msgs = [zipf(k, 40 + k) for k in (30_000, 5_000, 60_000, 700, 45_000)]
    b = Source(mhc, msgs, chunk, each=each)
    dst = shared_model(mhc, [zipf(100000, 3)], 1)
    clean = b.recode(dst, indexed)
    clean_hist = b.histogram(1, indexed)[0]
    per = [mhc.histogram_o1_batch([m]) for m in msgs]
    assert np.array_equal(clean_hist, sum(per))
    streams = [bytes(b.payload[int(b.pay_off[i]):int(b.pay_off[i + 1])]) for i in range(5)]
    cpay = [clean["payload"][int(clean["out_off"][i]):int(clean["out_off"][i + 1])].tobytes() for i in range(5)]
    failed = 0
    for at in (0, 2, 4):
        pl, nb = streams[at], int(b.nbits[at])
        base = int(mhc.lib().mh_batch_index_base(int(b.sym_off[at]), at, chunk))
        entry_bit = int(b.index[base + 3]) & mhc.INDEX_BIT_MASK
        cases = [("cut-1", damage.cut(pl, nb, nb - 1), nb - 1), ("cut-9", damage.cut(pl, nb, nb - 9), nb - 9),
                 ("ext0+5", damage.with_length(pl, nb, nb + 5, 0), nb + 5), ("ext1+13", damage.with_length(pl, nb, nb + 13, 1), nb + 13),
                 ("flip-first", damage.flip(pl, 5), nb), ("flip-mid", damage.flip(pl, nb // 2), nb), ("flip-last", damage.flip(pl, nb - 3), nb),
                 ("cut-entry", damage.cut(pl, nb, entry_bit), entry_bit), ("cut-entry+1", damage.cut(pl, nb, entry_bit + 1), entry_bit + 1),
                 ("garbage", damage.garbage_after(pl, nb, 1), nb)]
        for name, dpl, dnb in cases:
            pls, nbs = list(streams), [int(x) for x in b.nbits]
            pls[at], nbs[at] = dpl, dnb
            payload, pay_off = mhc.batch_offsets(pls)
            kw = b.kw(indexed) if indexed else {}
            want_st, want_rc = dev_decode_statuses(mhc, b, payload, pay_off, nbs, **kw)
            got = b.recode(dst, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
            hist, hst, hrc = b.histogram(1, indexed, payload=payload, pay_off=pay_off, nbits=nbs)
            what = "stream %d %s indexed=%s each=%s" % (at, name, indexed, each)
            assert got["status"].tolist() == want_st.tolist() == hst.tolist(), what
            assert (got["rc"] == mhc.MH_OK) == (want_rc == mhc.MH_OK) == (hrc == mhc.MH_OK), what
            for k in range(5):
                a0, a1 = int(got["out_off"][k]), int(got["out_off"][k + 1])
                if k != at:
                    assert got["payload"][a0:a1].tobytes() == cpay[k] and got["nbits"][k] == clean["nbits"][k], what
                    assert got["dropped"][k] == clean["dropped"][k], what
            if got["status"][at] != mhc.MH_OK:
                failed += 1
                assert got["nbits"][at] == 0 and got["out_off"][at + 1] == got["out_off"][at] and got["dropped"][at] == 0, what
                assert np.array_equal(hist, clean_hist - per[at]), what
                if indexed:
                    ok = [k for k in range(5) if k != at]
                    assert np.array_equal(slices(mhc, got["index"], b.sym_off, chunk, ok), slices(mhc, clean["index"], b.sym_off, chunk, ok)), what
    assert failed >= 12                                                        # the damages did fail streams


def test_capacity_and_the_walk_cap(mhc, ragged):
    src = Source(mhc, ragged, 256)
    dst = shared_model(mhc, [zipf(200000, 7)], 1)
    for indexed in (True, False):
        full = src.recode(dst, indexed)
        need = int(full["out_off"][-1])
        short = src.recode(dst, indexed, cap=need - 1)
        assert short["rc"] == mhc.MH_ERR_CAPACITY and short["payload"].size == 0
        for k in ("out_off", "nbits", "dropped", "status"):
            assert np.array_equal(short[k], full[k]), (indexed, k)
        roomy = src.recode(dst, indexed, cap=need + 100)
        assert roomy["rc"] == mhc.MH_OK and np.array_equal(roomy["payload"], full["payload"])
    # an index-free stream over MH_BATCH_WALK_MAX_BITS: refused by the device call, served by the host form
    big = zipf(2_000_000, 5)
    msgs = [big, zipf(3000, 6)]
    b = Source(mhc, msgs, 1024)
    assert int(b.nbits[0]) > mhc.BATCH_WALK_MAX_BITS
    got = b.recode(dst, False, count_only=True)
    assert got["status"].tolist() == [mhc.MH_ERR_ARG, mhc.MH_OK] and got["nbits"][0] == 0
    w_pay, w_off, w_nb, w_idx, w_so = dst.encode_batch(msgs, chunk_symbols=1024)
    host = b.model.recode_batch(dst, b.payload, b.pay_off, b.nbits, chunk_symbols=1024)
    assert host["rc"] == mhc.MH_OK and np.array_equal(host["payload"], w_pay) and np.array_equal(host["nbits"], w_nb)
    assert np.array_equal(host["sym_off"], w_so)
    assert np.array_equal(slices(mhc, host["index"], w_so, 1024), slices(mhc, w_idx, w_so, 1024))


def test_order2_and_wrong_set_size_are_refused_on_the_card(mhc, ragged):
    src = Source(mhc, ragged, 256)
    m2 = mhc.Model.from_counts(np.ones(1 << 24, dtype=np.uint64), 2)
    for a, b in ((m2, src.model), (src.model, m2)):
        with pytest.raises(mhc.MhError) as e:
            a.dev_recode_batch(b, src.payload, src.pay_off, src.nbits, **src.kw(True))
        assert e.value.status == mhc.MH_ERR_ARG
    ms = mhc.ModelSet.train(ragged[:3], order=1)
    with pytest.raises(mhc.MhError) as e:
        ms.recode(src.model, src.payload, src.pay_off, src.nbits, **src.kw(True))
    assert e.value.status == mhc.MH_ERR_ARG


# ---- every branch of the two launchers -----------------------------------------------------------------------------------------
# Which kernels a call runs depends on the LDS the shared source model's decode tables take (mhb::tables_lds): the destination's
# code lengths come from an LDS image behind the tables when it fits into the 160 KiB, else from L2, and the histogram's counter
# cache takes 12 << log2n bytes of what the tables leave (none when less than 3 KiB are left).  A model set keeps its tables in
# L2: an order-0 image, lengths of an order-1 destination from L2, 1 << 10 counters.

LDS_MAX = 163840
BRANCH_LENS = [0, 1, 255, 256, 257, 1300]      # at chunk 256: empty, a short chunk, a chunk that ends on the boundary, one past, several


def zipf_counts(s, k=256, scale=1 << 20):
    return (np.floor(scale / np.arange(1, k + 1) ** s) + 1).astype(np.uint64)


def zipf_below(k, n, seed):
    """n iid Zipf symbols below k."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, k + 1) ** 1.1
    return rng.choice(k, size=n, p=w / w.sum()).astype(np.uint8).tobytes()


def deep_context_source(seed_base):
    """P = 7 with a small second level.  Context 0 has seventeen subtrees at depth 8, each a chain of eight more levels (the
    weights are dyadic, scaled apart by a thousandth per chain so that no tie lets the tree builder balance them): their
    second-level tables at P = 8 would take 17 * 256 entries, more than one context may have, while at P = 7 they pair up into nine
    tables.  Every other context has 128 symbols of 7 bits and no second level."""
    row = []
    for j in range(17):
        row += [(1 << (16 - d)) * (1000 + j) for d in (9, 10, 11, 12, 13, 14, 15, 16, 16)]
    row += [(1 << (16 - d)) * 1008 for d in (1, 2, 3, 5, 6, 7, 8)]
    c = np.zeros((256, 256), dtype=np.uint64)
    c[:, :128] = 1
    c[0, :] = 0
    c[0, :len(row)] = row
    msgs = []
    for i, n in enumerate(BRANCH_LENS):
        rng = np.random.default_rng(seed_base + i)
        m = rng.integers(1, 128, n, dtype=np.uint8)                    # contexts 1..127: any symbol below 128 has a code
        at = np.arange(3, n - 1, 7)
        m[at] = 0                                                      # context 0: all 160 symbols, the 16-bit ones among them
        m[at + 1] = rng.integers(0, len(row), at.size, dtype=np.uint8)
        msgs.append(m.tobytes())                                       # (behind a symbol >= 128 comes one below 128 again)
    return c, msgs


def branch_source(kind):
    """(counts of the source model, messages, (P, table bytes in LDS)) for one launcher branch."""
    c = np.zeros((256, 256), dtype=np.uint64)
    if kind == "P7_SMALL":
        c, msgs = deep_context_source(900)
        return c, msgs, (7, 1024 + (512 << 7) + 2 * 9 * 256)
    if kind == "P8":                              # forty symbols, codes up to 9 bits: a small second level beside a full first level
        c[:40, :40] = zipf_counts(1.5, 40)
        k, want = 40, (8, None)
    elif kind == "P7_FULL":                       # 96 contexts of 256 Zipf symbols: the tables leave less than 3 KiB
        c[:96] = zipf_counts(1.1)
        c[96:, 0] = 1
        k, want = 96, (7, None)
    else:
        raise ValueError(kind)
    return c, [zipf_below(k, n, 910 + i) for i, n in enumerate(BRANCH_LENS)], want


def tables_lds(model):
    P, nsec, in_lds = model.decode_layout()
    return P, 1024 + (512 << P) + (((2 * nsec + 15) & ~15) if in_lds else 0)


def counter_log2n(room):
    return max([k for k in range(8, 13) if (12 << k) <= room], default=0)


@pytest.fixture(scope="module")
def branch_dsts(mhc):
    train = [zipf(200000, 7)]
    return {do: mhc.Model.from_counts(mhc.histogram_o1_batch(train, order=do), do) for do in (0, 1)}


@pytest.mark.parametrize("kind,img1_in_lds,img0_in_lds,log2n", [("P7_SMALL", True, True, 12), ("P8", False, True, 11), ("P7_FULL", False, True, 0)])
def test_every_launcher_branch_of_a_shared_source(mhc, branch_dsts, kind, img1_in_lds, img0_in_lds, log2n):
    counts, msgs, (want_p, want_lds) = branch_source(kind)
    assert [len(m) for m in msgs] == BRANCH_LENS
    model = mhc.Model.from_counts(counts.reshape(-1), 1)
    P, lds = tables_lds(model)
    assert P == want_p and model.decode_layout()[2] and (want_lds is None or lds == want_lds), (kind, model.decode_layout())
    # the recipe is on its branch
    assert (lds + 65536 <= LDS_MAX) == img1_in_lds and (lds + 256 <= LDS_MAX) == img0_in_lds and counter_log2n(LDS_MAX - lds) == log2n, (kind, lds)
    src = Source(mhc, msgs, 256, model=model)
    for do in (1, 0):
        check_parity(mhc, src, branch_dsts[do], do, "%s -> order %d" % (kind, do), oracle=False)
    for order in (0, 1):
        want = mhc.histogram_o1_batch(msgs, order=order)
        for indexed in (True, False):
            got, st, rc = src.histogram(order, indexed)
            assert rc == mhc.MH_OK and (st == mhc.MH_OK).all() and np.array_equal(got, want), (kind, order, indexed)


def test_every_launcher_branch_of_a_model_set(mhc, branch_dsts):
    msgs = [zipf(n, 930 + i) for i, n in enumerate(BRANCH_LENS)]
    src = Source(mhc, msgs, 256, each=True)
    for do in (1, 0):
        check_parity(mhc, src, branch_dsts[do], do, "set -> order %d" % do, oracle=False)
    for order in (0, 1):
        want = mhc.histogram_o1_batch(msgs, order=order)
        for indexed in (True, False):
            got, st, rc = src.histogram(order, indexed)
            assert rc == mhc.MH_OK and (st == mhc.MH_OK).all() and np.array_equal(got, want), (order, indexed)
