"""The device tree build (tree_build_kernel's lane-parallel heap) against the host build, on histograms chosen for
their ties: every heap movement of the reference (src/min_pq.tpp) depends on the keys alone, and equal keys are
where a heap that is not the reference's would place an entry differently.  Each case fills all 256 contexts of
one order-1 model; the device images, code lengths and codewords must equal the host twin's
(mh_model_from_counts), and the table file the CPU oracle's."""
import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    import os
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    mod.lib()
    assert mod.device_count() >= 1, "GPU tests need a device; the codec has no CPU fallback"
    return mod


def _check(mhc, oracle, counts):
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(65536)
    host = mhc.Model.from_counts(counts, 1)
    d_counts = mhc.DeviceBuffer(65536 * 8, counts)
    dev = mhc.Model.from_device_counts(d_counts.ptr, 1)
    assert dev.decode_layout() == host.decode_layout()
    assert dev.max_code_len == host.max_code_len
    for which in range(8):
        assert dev.image(which) == host.image(which), "image %d differs" % which
    ld, cd = dev.codes()
    lh, ch = host.codes()
    assert np.array_equal(ld, lh) and np.array_equal(cd, ch)
    assert dev.table_bytes() == oracle.Model.from_counts(counts, 1).table_bytes()


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return np.array(f[:n], dtype=np.uint64)


def _cases():
    rng = np.random.default_rng(20261016)
    z = np.zeros((256, 256), dtype=np.uint64)
    out = {}
    out["all_ones"] = np.ones((256, 256), dtype=np.uint64)
    c = z.copy()                                   # runs of equal rare counts under a few distinct common ones
    for p in range(256):
        c[p] = rng.choice([1, 2, 3], 256)
        c[p, rng.choice(256, 8, replace=False)] = rng.integers(1000, 1004, 8)
    out["equal_rare_runs"] = c
    c = z.copy()                                   # powers of two: merged sums tie with leaves all the way up
    for p in range(256):
        c[p] = np.uint64(1) << rng.integers(0, 12, 256).astype(np.uint64)
    out["powers_of_two"] = c
    c = z.copy()                                   # pairs of equal counts whose sums tie the next pair
    for p in range(256):
        base = np.repeat(np.uint64(1) << np.arange(128, dtype=np.uint64) % np.uint64(20), 2)
        c[p] = base[rng.permutation(256)]
    out["sums_tie_leaves"] = c
    c = z.copy()                                   # 1, 2, 3 and 256 live symbols (and empty contexts)
    for p in range(256):
        k = [0, 1, 2, 3, 256][p % 5]
        c[p, rng.choice(256, k, replace=False)] = rng.integers(1, 4, k)
    out["few_live"] = c
    c = z.copy()                                   # context totals at and above 2^32: 64-bit keys
    for p in range(256):
        c[p] = rng.integers(1, 5, 256)
        c[p, p] = (1 << 32) - int(c[p].sum()) + int(c[p, p]) + (p % 3)
    out["total_2_32"] = c
    c = z.copy()                                   # code lengths over 12 and over 15 bits (Fibonacci weights)
    for p in range(256):
        n = 14 + p % 40
        c[p, rng.choice(256, n, replace=False)] = _fib(n)[rng.permutation(n)]
    out["long_codes"] = c
    # the flagship's histogram: the expected counts of 16 GiB of the bench's Zipf(1.1) stream (i.i.d. symbols, so
    # count(prev, sym) = n * P(prev) * P(sym), with P from the bench's 32-bit thresholds)
    w = 1.0 / np.arange(1, 257, dtype=np.float64) ** 1.1
    t = np.minimum(np.rint(np.cumsum(w / w.sum())[:255] * 4294967296.0), 4294967295.0)
    pr = np.diff(np.concatenate([[0.0], t, [4294967296.0]])) / 4294967296.0
    out["zipf_16g"] = np.rint(np.outer(pr, pr) * float(16 << 30)).astype(np.uint64)
    return out


CASES = _cases()


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_heap_equals_host_heap(mhc, oracle, case):
    _check(mhc, oracle, CASES[case])


@pytest.mark.parametrize("seed", range(12))
def test_device_heap_random_ties(mhc, oracle, seed):
    """256 seeded random histograms per model (3 072 in all), small alphabets of counts so that ties are the rule."""
    rng = np.random.default_rng(seed)
    c = np.zeros((256, 256), dtype=np.uint64)
    for p in range(256):
        live = int(rng.integers(1, 257))
        hi = int(rng.choice([2, 3, 5, 9, 40, 1 << 20]))
        c[p, rng.choice(256, live, replace=False)] = rng.integers(1, hi, live)
    if seed % 4 == 3:
        c[seed] *= np.uint64(1 << 24)              # one context over 2^32 in every fourth model
    _check(mhc, oracle, c)
