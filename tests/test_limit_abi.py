"""Length-limited models on the host (include/mh.h): mh_model_from_counts_limited against a model of the
rule written here in plain Python, against the golden tables where the limit does not bind, and through the CPU oracle,
which reads a limited table like any other.  No GPU.

The rule, per context: the reference tree stays when its depth is <= L; otherwise lengths come from package-merge (leaves
by count, then symbol; on equal weight a leaf precedes a package) and the codewords are canonical (length, then symbol).
`limited_model` below applies the list form of that rule; the product implements the flag form, on the host and in a kernel.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import check_against_golden, golden, golden_names


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


# ---- the rule, in plain Python --------------------------------------------------------------------------------------------
def package_merge(counts, L):
    """{symbol: length} of the optimal code of at most L bits for the live symbols of `counts` (list form)."""
    leaves = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(leaves)
    assert n >= 2 and (1 << L) >= n
    level = [(w, (s,)) for w, s in leaves]
    for _ in range(L - 1):
        packages = [(level[i][0] + level[i + 1][0], level[i][1] + level[i + 1][1]) for i in range(0, len(level) - 1, 2)]
        # stable sort on the weight alone, leaves listed first: a leaf precedes a package of its weight, packages keep their order
        level = sorted([(w, (s,)) for w, s in leaves] + packages, key=lambda t: t[0])[:2 * n - 2]
    lens = {}
    for _, syms in level[:2 * n - 2]:
        for s in syms:
            lens[s] = lens.get(s, 0) + 1
    return lens


def canonical_codes(lens):
    """{symbol: (length, code)}: consecutive values in the order (length, symbol), the first one all zero bits."""
    out, code, prev = {}, 0, None
    for l, s in sorted((l, s) for s, l in lens.items()):
        code = 0 if prev is None else (code + 1) << (l - prev)
        out[s], prev = (l, code), l
    return out


def trie_of(codes):
    """Nested [left, right] lists with symbols at the leaves."""
    root = [None, None]
    for s, (l, code) in codes.items():
        node = root
        for i in range(l - 1, 0, -1):
            b = (code >> i) & 1
            if node[b] is None:
                node[b] = [None, None]
            node = node[b]
        node[code & 1] = s
    return root


def tree_bits(node, out):
    """Pre-order: inner -> 0, leaf -> 1 + the symbol's 8 bits (the table file's tree)."""
    stack = [node]
    while stack:
        n = stack.pop()
        if isinstance(n, list):
            out.append(0)
            stack.append(n[1])
            stack.append(n[0])
        else:
            out.append(1)
            out.extend((n >> i) & 1 for i in range(7, -1, -1))


def parse_tree(bits, pos):
    if bits[pos]:
        s = 0
        for b in bits[pos + 1:pos + 9]:
            s = (s << 1) | int(b)
        return s, pos + 9
    left, pos = parse_tree(bits, pos + 1)
    right, pos = parse_tree(bits, pos)
    return [left, right], pos


def tree_depth(node):
    return 0 if not isinstance(node, list) else 1 + max(tree_depth(node[0]), tree_depth(node[1]))


def parse_table(table, order):
    """Per-context trees (None = empty context) of a table file."""
    bits = np.unpackbits(np.frombuffer(table, dtype=np.uint8))
    if order == 0:
        return [parse_tree(bits, 0)[0]]
    assert bits[0] == 1
    pos, trees = 1, []
    for _ in range(256):
        pos += 1
        if bits[pos - 1]:
            t, pos = parse_tree(bits, pos)
            trees.append(t)
        else:
            trees.append(None)
    return trees


def write_table(trees, order):
    out = []
    if order == 0:
        tree_bits(trees[0], out)
    else:
        out.append(1)
        for t in trees:
            out.append(0 if t is None else 1)
            if t is not None:
                tree_bits(t, out)
    return np.packbits(np.array(out, dtype=np.uint8)).tobytes()


def limited_model(counts, order, L, unlimited_table):
    """The rule applied to a whole model.  Returns (table bytes, [per context: None = kept, else {sym: (len, code)}])."""
    counts = np.asarray(counts, dtype=np.uint64).reshape(-1, 256)
    trees = parse_table(unlimited_table, order)
    recoded = []
    for c, t in enumerate(trees):
        if t is None or tree_depth(t) <= L:
            recoded.append(None)
            continue
        codes = canonical_codes(package_merge([int(v) for v in counts[c]], L))
        trees[c] = trie_of(codes)
        recoded.append(codes)
    return write_table(trees, order), recoded


# ---- histograms ---------------------------------------------------------------------------------------------------------------
def synthetic_histograms():
    """name -> 256 counts (one context each)."""
    h = {}
    fib = [1, 1]
    while len(fib) < 60:
        fib.append(fib[-1] + fib[-2])
    h["fibonacci60"] = fib + [0] * 196                                  # reference depth 59
    h["equal256"] = [7] * 256
    h["ones_and_2^40"] = [1] * 255 + [1 << 40]
    h["geometric3"] = [3 ** i for i in range(34)] + [0] * 222
    h["geometric2_ties"] = [1 << (i // 3) for i in range(120)] + [0] * 136
    near = [(1 << 55) - 12345] + [fib[i] << 12 for i in range(59)]      # total just under 2^56
    assert sum(near) < (1 << 56)
    h["near_2^55"] = [0] * 100 + near + [0] * (156 - len(near))
    return {k: np.array(v, dtype=np.uint64) for k, v in h.items()}


def random_histograms(count=2200, seed=20251016):
    """Seeded histograms with heavy ties: few distinct weights, most of them powers of two, any number of live symbols."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(2, 257)) if rng.random() < 0.3 else int(rng.integers(2, 48))
        kind = rng.integers(0, 4)
        if kind == 0:
            w = 1 << rng.integers(0, 31, size=n)
        elif kind == 1:
            w = rng.integers(1, 6, size=n) * (1 << rng.integers(0, 24, size=n))
        elif kind == 2:
            w = np.sort(1 << np.minimum(rng.geometric(0.15, size=n), 40))
        else:
            w = np.where(rng.random(n) < 0.5, 1, rng.integers(1, 10 ** 6, size=n))
        counts = np.zeros(256, dtype=np.uint64)
        counts[rng.permutation(256)[:n]] = np.asarray(w, dtype=np.uint64)
        out.append((counts, int(rng.choice([8, 8, 9, 10, 11, 12, 14, 16, 20]))))
    return out


def codes_of(mhc, model, prev=0):
    l, c = ctypes.c_int(), ctypes.c_uint64()
    out = {}
    for s in range(256):
        assert mhc.lib().mh_model_get_code(model.handle, prev, s, ctypes.byref(l), ctypes.byref(c)) == 0
        if l.value:
            out[s] = (l.value, c.value)
    return out


def check_context(counts, L, got, kept_codes, expect):
    """One context of a limited model: `got` {sym: (len, code)} from the product, `kept_codes` the unlimited build's codes,
    `expect` None (kept) or the rule's codes.  Returns the context's cost in bits."""
    assert max(l for l, _ in got.values()) <= L
    if expect is None:
        assert got == kept_codes
    else:
        assert sum(Fraction(1, 1 << l) for l, _ in got.values()) == 1
        optimum = sum(int(counts[s]) * l for s, (l, _) in expect.items())
        assert sum(int(counts[s]) * l for s, (l, _) in got.items()) == optimum
        assert got == expect
    return sum(int(counts[s]) * l for s, (l, _) in got.items())


# ---- 1. a limit that does not bind gives the reference's table --------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
@pytest.mark.parametrize("order", [0, 1])
def test_limit_64_gives_the_golden_tables(mhc, oracle, name, order):
    data = golden()[name]["data"]
    counts = oracle.histogram_o1(data) if order else oracle.histogram_o0(data)
    m = mhc.Model.from_counts(counts, order, max_len=64)
    check_against_golden(name, "e" if order else "eh", m.table_bytes())
    assert m.type == order


@pytest.mark.parametrize("name,L", [("input_ipsum.txt", 12), ("input_wiki_cpp.html", 15)])
def test_limit_at_the_longest_code_gives_the_golden_table(mhc, oracle, name, L):
    counts = oracle.histogram_o1(golden()[name]["data"])
    assert int(oracle.Model.from_counts(counts, 1).codes()[0].max()) <= L
    check_against_golden(name, "e", mhc.Model.from_counts(counts, 1, max_len=L).table_bytes())


# ---- 2. a limit that binds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["input_wiki_cpp.html", "input_wiki_cpp.txt", "kat4"])
@pytest.mark.parametrize("L", [8, 9, 10, 12, 14])
def test_binding_limit_on_golden_inputs(mhc, oracle, name, L):
    data = golden()[name]["data"]
    counts = np.asarray(oracle.histogram_o1(data), dtype=np.uint64)
    ref = oracle.Model.from_counts(counts, 1)
    table, recoded = limited_model(counts, 1, L, ref.table_bytes())
    # (input_wiki_cpp.txt's longest code has 13 bits: a limit of 14 must leave it alone)
    assert any(r is not None for r in recoded) == (int(ref.codes()[0].max()) > L)
    m = mhc.Model.from_counts(counts, 1, max_len=L)
    assert m.table_bytes() == table
    assert m.max_code_len <= L
    lens, codes = m.codes()
    rl, rc = ref.codes()
    total = 0
    for c in range(256):
        row = counts[c * 256:(c + 1) * 256]
        got = {s: (int(lens[c * 256 + s]), int(codes[c * 256 + s])) for s in range(256) if lens[c * 256 + s]}
        kept = {s: (int(rl[c * 256 + s]), int(rc[c * 256 + s])) for s in range(256) if rl[c * 256 + s]}
        if not got:
            assert not kept and recoded[c] is None
            continue
        total += check_context(row, L, got, kept, recoded[c])
    # 3. the oracle reads the table: same codes and LUT, round trip, and the exact payload size
    o = oracle.Model.from_table(table)
    ol, oc = o.codes()
    assert np.array_equal(ol, lens) and np.array_equal(oc, codes)
    for prev in (0x20, ord("e"), ord("<"), 0):
        for w in range(256):
            assert m.lut(prev, w) == o.lut(prev, w)
    blob, nbits = o.compress(data)
    assert o.decompress(blob) == data
    assert m.payload_bits(counts) == total == nbits
    unlimited = int((counts.astype(object) * np.asarray(rl).astype(object)).sum())
    print("%s L=%d: %d payload bits, unlimited %d (+%.4f %%)" % (name, L, total, unlimited, 100.0 * (total - unlimited) / unlimited))
    assert total >= unlimited


@pytest.mark.parametrize("name", sorted(synthetic_histograms()))
@pytest.mark.parametrize("L", [8, 9, 10, 12, 14, 33, 64])
def test_binding_limit_on_synthetic_histograms(mhc, oracle, name, L):
    counts = synthetic_histograms()[name]
    ref = oracle.Model.from_counts(counts, 0)
    table, recoded = limited_model(counts, 0, L, ref.table_bytes())
    m = mhc.Model.from_counts(counts, 0, max_len=L)
    assert m.table_bytes() == table
    rl, rc = ref.codes()
    kept = {s: (int(rl[s]), int(rc[s])) for s in range(256) if rl[s]}
    cost = check_context(counts, L, codes_of(mhc, m), kept, recoded[0])
    assert m.payload_bits(counts) == cost
    o = oracle.Model.from_table(table)
    assert np.array_equal(o.codes()[0][:256], m.codes()[0][:256])
    if name == "fibonacci60":
        assert (recoded[0] is not None) == (L < 59)
    if name == "equal256":
        assert recoded[0] is None
    if name == "ones_and_2^40" and L == 8:
        assert recoded[0] is not None and all(l == 8 for l, _ in recoded[0].values())


def test_binding_limit_on_random_tied_histograms(mhc, oracle):
    cases = random_histograms()
    assert len(cases) >= 2000
    bound = 0
    for counts, L in cases:
        ref = oracle.Model.from_counts(counts, 0)
        table, recoded = limited_model(counts, 0, L, ref.table_bytes())
        m = mhc.Model.from_counts(counts, 0, max_len=L)
        assert m.table_bytes() == table
        rl, rc = ref.codes()
        kept = {s: (int(rl[s]), int(rc[s])) for s in range(256) if rl[s]}
        got = codes_of(mhc, m)
        check_context(counts, L, got, kept, recoded[0])
        if recoded[0] is not None:
            bound += 1
            order = sorted(got, key=lambda s: (int(counts[s]), s))        # lengths never grow with the count
            assert all(got[a][0] >= got[b][0] for a, b in zip(order, order[1:]))
    assert bound >= 500, "only %d of the random histograms are deeper than their limit" % bound


def test_package_merge_is_optimal_on_small_alphabets():
    """The test's own optimum against an exhaustive search: every multiset of lengths <= L with Kraft sum 1, longest codes to
    the rarest symbols."""
    def all_profiles(n, L, depth=1, open_nodes=2):
        # number of leaves at each depth of a full binary tree with n leaves and depth <= L
        if depth > L:
            return
        for leaves in range(0, min(open_nodes, n) + 1):
            rest, inner = n - leaves, open_nodes - leaves
            if rest == 0 and inner == 0:
                yield [leaves]
            elif rest > 0 and inner > 0:
                for tail in all_profiles(rest, L, depth + 1, 2 * inner):
                    yield [leaves] + tail
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(2, 10))
        L = int(rng.integers(max(1, (n - 1).bit_length()), 7))
        w = sorted((int(x) for x in rng.integers(1, 40, size=n)), reverse=True)
        best = None
        for prof in all_profiles(n, L):
            lens = [d + 1 for d, k in enumerate(prof) for _ in range(k)]
            cost = sum(a * b for a, b in zip(w, lens))
            best = cost if best is None else min(best, cost)
        pm = package_merge(w, L)
        assert sum(w[s] * l for s, l in pm.items()) == best


# ---- 4. contract ------------------------------------------------------------------------------------------------------------
def test_limited_calls_check_their_arguments_before_a_device(mhc, oracle):
    lib = mhc.lib()
    h = ctypes.c_void_p()
    counts = np.asarray(oracle.histogram_o1(golden()["input_wiki_cpp.txt"]["data"]), dtype=np.uint64)
    p = counts.ctypes.data
    buf = (ctypes.c_uint8 * 64)()
    d = ctypes.addressof(buf)                 # stands for a device pointer: never read, the arguments are refused first
    for bad in list(range(1, 8)) + [65, 100, -1, 1 << 20]:
        assert lib.mh_model_from_counts_limited(p, 1, bad, ctypes.byref(h)) == mhc.MH_ERR_ARG
        assert lib.mh_model_from_counts_limited(p, 0, bad, ctypes.byref(h)) == mhc.MH_ERR_ARG
        assert lib.mh_dev_model_from_counts_limited(d, 1, bad, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
        assert lib.mh_dev_model_from_counts_limited_ws(d, 1, bad, d, 1 << 30, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_model_from_counts_limited(p, 2, 12, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited(d, 2, 12, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited_ws(d, 2, 12, d, 1 << 30, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited_ws(d, 0, 12, d, 1 << 30, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_model_from_counts_limited(None, 1, 12, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_model_from_counts_limited(p, 1, 12, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited(None, 1, 12, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited(d, 1, 12, None, None) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited_ws(None, 1, 12, d, 1 << 30, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited_ws(d, 1, 12, None, 1 << 30, None, ctypes.byref(h)) == mhc.MH_ERR_ARG
    assert lib.mh_dev_model_from_counts_limited_ws(d, 1, 12, d, 1 << 30, None, None) == mhc.MH_ERR_ARG
    if mhc.device_count() == 0:
        assert lib.mh_dev_model_from_counts_limited(d, 1, 12, None, ctypes.byref(h)) == mhc.MH_ERR_NO_DEVICE


def test_limit_0_is_the_unlimited_call(mhc, oracle):
    for name, order in (("input_wiki_cpp.html", 1), ("kat4", 1), ("input_wiki_cpp.txt", 0)):
        data = golden()[name]["data"]
        counts = np.asarray(oracle.histogram_o1(data) if order else oracle.histogram_o0(data), dtype=np.uint64)
        h = ctypes.c_void_p()
        assert mhc.lib().mh_model_from_counts_limited(counts.ctypes.data, order, 0, ctypes.byref(h)) == 0
        a, b = mhc.Model(h), mhc.Model.from_counts(counts, order)
        assert a.table_bytes() == b.table_bytes() and a.max_code_len == b.max_code_len
        check_against_golden(name, "e" if order else "eh", a.table_bytes())


def test_context_of_2_to_56_symbols_is_refused_only_when_it_has_to_be_recoded(mhc):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(256, dtype=np.uint64)
    counts[:40] = fib
    counts[40] = 1 << 56
    h = ctypes.c_void_p()
    assert mhc.lib().mh_model_from_counts_limited(counts.ctypes.data, 0, 12, ctypes.byref(h)) == mhc.MH_ERR_ARG
    m = mhc.Model.from_counts(counts, 0, max_len=64)             # depth 40: kept as it is
    assert m.table_bytes() == mhc.Model.from_counts(counts, 0).table_bytes()


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def test_the_cli_refuses_a_limit_where_no_table_is_trained(tmp_path):
    """Checked at parse time, before a device is looked for.  (A set from limited tables, mh_model_set_from_tables, uploads its
    models and needs a device: that check is in tests/test_gpu_limit.py.)"""
    import os
    import subprocess
    from conftest import ROOT
    cli = os.path.join(ROOT, "bin", "markovhuffman")
    if not os.path.exists(cli):
        entry.build()
    src = tmp_path / "in"
    src.write_bytes(b"hello hello")
    for extra, msg in ((["--max-code-len", "7"], b"between 8 and 64"), (["--max-code-len", "65"], b"between 8 and 64"),
                       (["--max-code-len", "12", "-e", str(src)], b"cannot be combined"),
                       (["--max-code-len", "12", "--order2"], b"cannot be combined"),
                       (["--max-code-len", "12", "-x", "-e", str(src)], b"cannot be combined")):
        r = subprocess.run([cli, str(src), "-o", str(tmp_path / "o")] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and msg in r.stderr, extra
