"""Length-limited models on the device (include/mh.h): limit_recode_kernel against the host build, what a limit
of 12 bits changes on a real input (no escape launch, a second table level that resolves every code), every reader on a
limited model's stream, and the genuine reference binary on our limited table.  The rule itself is pinned, on the host,
by tests/test_limit_abi.py against a model in plain Python; here the device has to give the host's bytes."""
import os
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as entry
import damage
from conftest import ROOT, golden
from test_limit_abi import limited_model, random_histograms, synthetic_histograms

pytestmark = pytest.mark.gpu

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "markovhuffman")
CLI = os.path.join(ROOT, "bin", "markovhuffman")
ENC_REGIONS, ENC_REGIONS_ESC = 1, 3
DEC_TILE, DEC_CHUNK = 1, 2
PATH_STATES = 6


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    mod.lib()
    assert mod.device_count() >= 1
    return mod


@pytest.fixture(scope="module")
def ds(mhc):
    import test_gpu_damaged_streams as mod          # its helpers drive the device decoders and check the guard bytes
    return mod


def build_ws(mhc, counts, max_len):
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    d_counts = mhc.DeviceBuffer(65536 * 8, init=counts)
    wsb = int(mhc.lib().mh_dev_model_workspace(1))
    d_ws = mhc.DeviceBuffer(wsb)
    m = mhc.Model.from_device_counts_ws(d_counts.ptr, 1, d_ws.ptr, wsb, max_len=max_len)
    m._keep = (d_counts, d_ws)                       # the model borrows the workspace
    return m


def same_model(dev, host):
    assert dev.max_code_len == host.max_code_len
    assert dev.decode_layout() == host.decode_layout() and dev.tile_layout() == host.tile_layout()
    for which in range(10):
        assert dev.image(which) == host.image(which), "image %d differs" % which
    assert dev.table_bytes() == host.table_bytes()


def stacked_histograms():
    """Models of 256 contexts whose rows are the histograms of tests/test_limit_abi.py (the synthetic ones in every model, 250
    of the tie-heavy random ones each): 8 models, 2 000 random rows."""
    syn = synthetic_histograms()
    rnd = [c for c, _ in random_histograms()]
    out = []
    for k in range(0, len(rnd) - 249, 250):
        rows = [syn[name] for name in sorted(syn)] + rnd[k:k + 250]
        out.append(np.stack(rows[:256]).reshape(-1))
    return out


# ---- 1. device = host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 9, 10, 12, 14, 33, 64])
def test_device_build_equals_host_build_on_tied_histograms(mhc, L):
    models = stacked_histograms()
    assert len(models) >= 8
    for counts in models if L <= 12 else models[:3]:
        host = mhc.Model.from_counts(counts, 1, max_len=L)
        assert host.max_code_len <= L
        same_model(build_ws(mhc, counts, L), host)


@pytest.mark.parametrize("name", ["input_wiki_cpp.html", "input_wiki_cpp.txt", "kat4"])
@pytest.mark.parametrize("L", [8, 9, 10, 12, 14])
def test_device_build_equals_host_build_on_golden_inputs(mhc, oracle, name, L):
    counts = np.asarray(oracle.histogram_o1(golden()[name]["data"]), dtype=np.uint64)
    host = mhc.Model.from_counts(counts, 1, max_len=L)
    same_model(build_ws(mhc, counts, L), host)
    d_counts = mhc.DeviceBuffer(65536 * 8, init=counts)
    same_model(mhc.Model.from_device_counts(d_counts.ptr, 1, max_len=L), host)          # the allocating twin
    table, _ = limited_model(counts, 1, L, oracle.Model.from_counts(counts, 1).table_bytes())
    assert host.table_bytes() == table


def test_a_limit_that_binds_nowhere_gives_the_unlimited_images(mhc, oracle):
    for name, L in (("input_wiki_cpp.html", 15), ("input_ipsum.txt", 12), ("kat4", 64)):
        counts = np.asarray(oracle.histogram_o1(golden()[name]["data"]), dtype=np.uint64)
        same_model(build_ws(mhc, counts, L), build_ws(mhc, counts, 0))
    counts = stacked_histograms()[0]                                                      # fibonacci60: depth 59
    same_model(build_ws(mhc, counts, 64), build_ws(mhc, counts, 0))


def test_device_refuses_a_context_of_2_to_56_symbols_that_would_be_recoded(mhc):
    counts = stacked_histograms()[1].copy()
    counts[7 * 256:8 * 256] = 0
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    counts[7 * 256:7 * 256 + 40] = fib
    counts[7 * 256 + 40] = 1 << 56
    with pytest.raises(mhc.MhError) as e:
        build_ws(mhc, counts, 12)
    assert e.value.status == mhc.MH_ERR_ARG
    with pytest.raises(mhc.MhError) as e:
        mhc.Model.from_counts(counts, 1, max_len=12)
    assert e.value.status == mhc.MH_ERR_ARG


# ---- 2. what it is for ----------------------------------------------------------------------------------------------------
def encode_hist(mhc, model, data, chunk):
    """mh_dev_encode_hist of `data` with its own histogram workspace: (nbits, payload, index, fine index, encode path)."""
    lib = mhc.lib()
    n = data.size
    d_data = mhc.DeviceBuffer(n + 32, init=np.concatenate([data, np.zeros(32, dtype=np.uint8)]))
    d_counts = mhc.DeviceBuffer(65536 * 8)
    hws = int(lib.mh_dev_histogram_workspace(n))
    d_hws = mhc.DeviceBuffer(hws)
    mhc._check(lib.mh_dev_histogram_o1(d_data.ptr, n, 0x20, d_counts.ptr, d_hws.ptr, hws, None), "hist")
    cap = lib.mh_encode_bound(model.handle, n) + 64
    nidx = (n + chunk - 1) // chunk
    wsb = lib.mh_dev_encode_workspace(n)
    d_payload = mhc.DeviceBuffer(cap, init=np.zeros(cap, dtype=np.uint8))
    d_nbits = mhc.DeviceBuffer(8, init=np.zeros(1, dtype=np.uint64))
    d_index = mhc.DeviceBuffer(nidx * 8, init=np.zeros(nidx, dtype=np.uint64))
    d_ws = mhc.DeviceBuffer(wsb + 64)
    mhc._check(lib.mh_dev_encode_hist(model.handle, d_data.ptr, n, 0x20, None, d_payload.ptr, cap, d_nbits.ptr, d_index.ptr, chunk,
                                      d_hws.ptr, hws, d_ws.ptr, wsb, None), "mh_dev_encode_hist")
    mhc._check(lib.mh_dev_status(d_ws.ptr, None), "encode status")
    nbits = int(d_nbits.download(np.uint64)[0])
    return nbits, d_payload.download()[:(nbits + 7) // 8].tobytes(), d_index.download(np.uint64)[:nidx], lib.mh_dev_encode_path(d_ws.ptr, None)


@pytest.fixture(scope="module")
def tiled(mhc, oracle):
    """input_wiki_cpp.html tiled past 8 MiB, its own histogram, the unlimited model and the model limited to 12 bits with
    that model's stream from mh_dev_encode_hist."""
    one = np.frombuffer(golden()["input_wiki_cpp.html"]["data"], dtype=np.uint8)
    data = np.tile(one, (9 << 20) // one.size + 1)
    counts = np.asarray(oracle.histogram_o1(data.tobytes()), dtype=np.uint64)
    t = types.SimpleNamespace(data=data, counts=counts, chunk=1024)
    t.free = build_ws(mhc, counts, 0)
    t.m = build_ws(mhc, counts, 12)
    t.table = t.m.table_bytes()
    t.om = oracle.Model.from_table(t.table)
    t.nbits, t.payload, t.index, t.enc_path = encode_hist(mhc, t.m, data, t.chunk)
    return t


def test_limit_12_takes_the_plain_encoder_and_a_resolving_second_level(mhc, oracle, tiled):
    t = tiled
    assert t.free.max_code_len > 12
    assert encode_hist(mhc, t.free, t.data, t.chunk)[3] == ENC_REGIONS_ESC
    assert t.m.max_code_len == 12
    assert t.enc_path == ENC_REGIONS
    P, H, _ = t.m.tile_layout()
    assert P > 0 and H <= 12 - P
    want_table, recoded = limited_model(t.counts, 1, 12, oracle.Model.from_counts(t.counts, 1).table_bytes())
    assert any(r is not None for r in recoded) and t.table == want_table
    blob, ref_bits = t.om.compress(t.data.tobytes())
    assert t.nbits == ref_bits and t.payload == blob[1:]
    lens = np.asarray(t.om.codes()[0]).astype(object)
    assert t.nbits == int((lens * t.counts.astype(object)).sum()) == t.m.payload_bits(t.counts)      # the optimum: test_limit_abi.py


# ---- 3. every reader --------------------------------------------------------------------------------------------------------
def test_every_single_stream_reader_takes_the_limited_stream(mhc, ds, tiled):
    t = tiled
    want = t.data.tobytes()
    path, status, ns, index, fine = ds.build_index(mhc, t.m, t.payload, t.nbits, t.chunk)
    assert status == 0 and ns == t.data.size
    nidx = (t.data.size + t.chunk - 1) // t.chunk
    assert np.array_equal(index[:nidx], t.index)
    src = types.SimpleNamespace(m=t.m, data=t.data, index=t.index, chunk=t.chunk, fine=fine[:(t.data.size + 63) // 64].copy())
    cpath, variant, got = ds.chunk_decode(mhc, src, t.payload, t.nbits)
    assert cpath == DEC_CHUNK and variant != 8 and got == (0, want)
    fpath, fvariant, got = ds.chunk_decode(mhc, src, t.payload, t.nbits, fine=True)
    assert fvariant != 8 and got == (0, want)
    assert fpath == DEC_TILE
    spath, got = ds.stream_decode(mhc, t.m, t.payload, t.nbits)
    assert spath == PATH_STATES and got == (0, want)
    assert t.m.decode(t.payload, t.nbits) == want                                    # mh_decode without an index
    rng = np.random.default_rng(12)
    b = rng.integers(0, t.data.size - 5000, size=200)
    ranges = [(int(x), int(x + l)) for x, l in zip(b, rng.integers(0, 5000, size=200))] + [(0, 1), (t.data.size - 1, t.data.size)]
    res, st = t.m.decode_ranges(t.payload, t.nbits, t.index, t.chunk, t.data.size, ranges)
    assert not st.any()
    for (lo, hi), r in zip(ranges, res):
        assert r == want[lo:hi]


def test_one_damaged_copy_gets_the_strict_oracles_verdict(mhc, ds, tiled):
    t = tiled
    src = types.SimpleNamespace(m=t.m, data=t.data, index=t.index, chunk=t.chunk)
    for name, pl, nb in (("flip", damage.flip(t.payload, t.nbits // 3), t.nbits), ("cut", damage.cut(t.payload, t.nbits, t.nbits - 5), t.nbits - 5)):
        want = damage.verdict_free(t.om, pl, nb)
        ds.expect(ds.stream_decode(mhc, t.m, pl, nb)[1], want, "states/emit " + name)
        ds.expect(ds.host_decode(mhc, t.m, pl, nb), want, "mh_decode " + name)
        wanti = damage.verdict_indexed(t.om, pl, nb, t.index, t.chunk, t.data.size)
        ds.expect(ds.chunk_decode(mhc, src, pl, nb)[2], wanti, "chunk decoder " + name)


def test_batches_under_a_shared_limited_model(mhc, oracle):
    """The lines of the file as independent streams (each starts in context prev0) under one model trained on them all."""
    lines = golden()["input_wiki_cpp.html"]["data"].split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + [lines[-1]]
    assert len(lines) > 500
    counts = mhc.histogram_o1_batch(lines)
    assert mhc.Model.from_counts(counts, 1).max_code_len > 12
    t = types.SimpleNamespace(m=mhc.Model.from_counts(counts, 1, max_len=12))
    assert t.m.max_code_len == 12
    t.om = oracle.Model.from_table(t.m.table_bytes())
    payload, out_off, nbits, idx, in_off = t.m.encode_batch(lines, chunk_symbols=256)
    lens = np.asarray(t.om.codes()[0])
    for k in (0, 1, len(lines) // 2, len(lines) - 1):
        assert int(nbits[k]) == int(damage.code_lengths(lens, np.frombuffer(lines[k], dtype=np.uint8)).sum())
    out, so, st = t.m.decode_batch(payload, out_off, nbits, sym_off=in_off, index=idx, chunk_symbols=256)
    assert out == b"".join(lines) and not st.any()
    out, so, st = t.m.decode_batch(payload, out_off, nbits)                                # index-free
    assert out == b"".join(lines) and not st.any() and np.array_equal(so, in_off)
    rng = np.random.default_rng(3)
    lookups = []
    for s in rng.integers(0, len(lines), size=300):
        n = len(lines[int(s)])
        lo = int(rng.integers(0, n + 1))
        lookups.append((int(s), lo, int(rng.integers(lo, n + 1))))
    for kw in (dict(sym_off=in_off, index=idx, chunk_symbols=256), dict()):
        res, st = t.m.decode_batch_ranges(payload, out_off, nbits, lookups, **kw)
        assert not st.any()
        for (s, lo, hi), r in zip(lookups, res):
            assert r == lines[s][lo:hi]


def test_a_set_from_limited_tables_reports_the_limited_lengths(mhc, oracle):
    """(mh_model_set_from_tables uploads its models: it needs a device, so this check lives here.)"""
    names = ("input_wiki_cpp.html", "kat4", "input_ipsum.txt")
    counts = [oracle.histogram_o1(golden()[n]["data"]) for n in names]
    limited = [mhc.Model.from_counts(c, 1, max_len=L) for c, L in zip(counts, (12, 10, 0))]
    s = mhc.ModelSet.from_tables([m.table_bytes() for m in limited])
    free = mhc.ModelSet.from_tables([mhc.Model.from_counts(c, 1).table_bytes() for c in counts])
    assert len(s) == 3
    assert s.code_lens()[0] == 12 and free.code_lens()[0] == 15
    assert [s.stream_info(i)[1] for i in range(3)] == [12, 10, 10]
    s2 = mhc.ModelSet.from_models(limited)
    assert s2.code_lens() == s.code_lens()


# ---- 4. the genuine reference -------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/markovhuffman not built (needs the reference at build time)")
def test_the_reference_binary_agrees_on_a_limited_table(mhc, oracle, tmp_path):
    data = golden()["input_wiki_cpp.html"]["data"]
    src = tmp_path / "in.html"
    src.write_bytes(data)
    run = dict(check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    subprocess.run([CLI, str(src), "--max-code-len", "12", "-d", str(tmp_path / "t.e"), "-o", str(tmp_path / "out.cm")], **run)
    table = (tmp_path / "t.e").read_bytes()
    counts = oracle.histogram_o1(data)
    assert table == limited_model(counts, 1, 12, oracle.Model.from_counts(counts, 1).table_bytes())[0]
    assert mhc.Model.from_table(table).max_code_len == 12
    subprocess.run([REF_BIN, str(src), "-e", str(tmp_path / "t.e"), "-o", str(tmp_path / "ref.cm")], **run)
    assert (tmp_path / "ref.cm").read_bytes() == (tmp_path / "out.cm").read_bytes()
    subprocess.run([REF_BIN, str(tmp_path / "out.cm"), "-x", "-e", str(tmp_path / "t.e"), "-o", str(tmp_path / "back")], **run)
    assert (tmp_path / "back").read_bytes() == data
