"""CPU-side checks of selecting records (include/mh.h, "SELECTING RECORDS OF BATCHES"): the symbols are declared, exported and
bound, the host forms mh_select_batch and mh_picks_from_hits (plain C++, no device) against tests/select_ref.py on the shapes
of tests/select_cases.py, and every refusal of the four calls before a device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import select_cases
import select_ref
from conftest import ROOT

NEW_SYMBOLS = ["mh_dev_select_batch_workspace", "mh_dev_select_batch", "mh_dev_picks_from_hits_workspace", "mh_dev_picks_from_hits",
               "mh_select_batch", "mh_picks_from_hits"]
FILL64 = select_cases.FILL64


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def test_select_symbols_are_declared_exported_and_bound(mhc):
    header = open(os.path.join(ROOT, "include", "mh.h")).read()
    lib = C.CDLL(mhc.LIB_PATH)
    section = header[header.index("SELECTING RECORDS OF BATCHES"):]
    for name in NEW_SYMBOLS:
        assert name + "(" in section, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    # what the section must say (the issue): what is left out, who gathers side information, why the launch context is nested
    for words in ("Left out: the CLI", "re-indexes its set", "selecting in place", "index chunk sizes differ", "gathered by the caller",
                  "nested mh_launch"):
        assert words in section, words
    assert "#define MH_SELECT_MAX_SOURCES 8u" in section and "typedef struct mh_launch" in section
    for name in ("Launch", "SelectArgs", "PicksArgs", "select_batch", "dev_select_batch", "picks_from_hits", "dev_picks_from_hits"):
        assert hasattr(mhc, name), name
    assert (mhc.SELECT_NONE, mhc.SELECT_MAX_SOURCES, mhc.PICKS_WITHOUT_HITS) == (select_ref.NONE, select_ref.MAX_SOURCES, select_ref.WITHOUT_HITS)


def test_workspaces_are_plain_arithmetic(mhc):
    lib = mhc.lib()
    for n in (0, 1, 257, 65536):
        w = lib.mh_dev_select_batch_workspace(3 * n, n)
        assert 0 < w <= 48 * n + 4096 and w % 256 == 0 and w == lib.mh_dev_select_batch_workspace(0, n), (n, w)
        w = lib.mh_dev_picks_from_hits_workspace(n)
        assert 0 < w <= 9 * n + 4096 and w % 256 == 0, (n, w)


# ---- the host forms against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", select_cases.NAMES)
def test_host_select_matches_the_reference(mhc, name):
    c = select_cases.case(name)
    bad = []
    for what, picks in c.picks.items():
        want = select_ref.select(c.packs, picks, c.chunk)
        r = mhc.select_batch(c.sources(), picks, c.chunk)
        bad += select_cases.differences(r, want, c.chunk, "%s, %s" % (name, what))
    assert not bad, "\n".join(bad)


def test_host_select_without_index_and_without_symbol_offsets(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    picks = c.picks["random"]
    want = select_ref.select(c.packs, picks, c.chunk)
    r = mhc.select_batch(c.sources(index=False), picks, 0)
    assert r.index is None and not select_cases.differences(r, want, c.chunk, "no index", index=False)
    r = mhc.select_batch(c.sources(sym=False), picks, 0, want_sym=False)
    assert not select_cases.differences(r, want, c.chunk, "no sym_off", index=False, sym=False)
    # an index in the sources, none asked for
    r = mhc.select_batch(c.sources(), picks, c.chunk, want_index=False)
    assert r.index is None and not select_cases.differences(r, want, c.chunk, "index not wanted", index=False)


def test_host_select_refuses_a_bad_pick_alone(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    src, packs = select_cases.spoiled(c)
    picks = select_cases.refused_picks(c)
    want = select_ref.select(packs, picks, c.chunk)
    assert want.status.tolist() == [0, -1, 0, -1, -1, 0, -1, 0]
    r = mhc.select_batch(src, picks, c.chunk)
    assert r.status == mhc.MH_ERR_ARG and not select_cases.differences(r, want, c.chunk, "bad picks")


def test_host_select_capacity_one_short(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    picks = c.picks["each twice"]
    want = select_ref.select(c.packs, picks, c.chunk)
    n, total = len(picks), int(want.pay_off[-1])
    need = int(want.sym_off[n]) // c.chunk + n + 1
    r = mhc.select_batch(c.sources(), picks, c.chunk, cap=total, index_cap=need)
    assert not select_cases.differences(r, want, c.chunk, "exact caps")
    for kw in (dict(cap=total - 1, index_cap=need), dict(cap=total, index_cap=need - 1)):
        r = mhc.select_batch(c.sources(), picks, c.chunk, **kw)
        assert r.status == mhc.MH_ERR_CAPACITY, kw
        assert np.array_equal(r.out_off, want.pay_off) and np.array_equal(r.nbits, want.nbits) and np.array_equal(r.sym_off, want.sym_off)
        assert (r.payload == select_cases.FILL).all() and (r.index == FILL64).all(), kw       # neither payload nor index


def test_host_picks_match_the_reference(mhc):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 64, 65, 257, 1000):
        counts = rng.integers(0, 3, n) * (rng.random(n) < 0.6)
        hit_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        status = np.where(rng.random(n) < 0.2, rng.choice([-1, -4, -8], n), 0).astype(np.int32)
        for ho in (hit_off, None):
            for st in (status, None):
                for flags in (0, select_ref.WITHOUT_HITS):
                    want, kept = select_ref.picks_from_hits(ho, st, flags, n=n, source=5)
                    got, k = mhc.picks_from_hits(ho, st, n, source=5, flags=flags)
                    assert k == kept and np.array_equal(got, want), (n, ho is None, st is None, flags)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _room():
    w = np.zeros(1 << 14, dtype=np.uint64)
    return w, (w.ctypes.data + 255) & ~255


def _select(mhc, form, p, **kw):
    """One select call on made-up addresses (nothing is ever read: every call here is refused, or there is no device)."""
    a = dict(struct_size=None, n_sources=1, sources="own", payload=p, pay_off=p, nbits=p, n=1, pay_total=16, sym_off=p, sym_total=100, index=p,
             src_chunk=256, picks=p, n_picks=1, out=p, cap=64, out_off=p, out_nbits=p, out_sym_off=p, out_index=p, index_cap=8, chunk=256,
             status=p, ws=p, wsb=1 << 16, second=None)
    a.update(kw)
    rows = [(a["payload"], a["pay_off"], a["nbits"], a["n"], a["pay_total"], a["sym_off"], a["sym_total"], a["index"], a["src_chunk"])]
    if a["second"] is not None:
        rows.append(a["second"])
    src = mhc.coded_batches(rows) if a["sources"] == "own" else a["sources"]
    if form == "host":
        return mhc.lib().mh_select_batch(src, a["n_sources"], a["picks"], a["n_picks"], a["out"], a["cap"], a["out_off"], a["out_nbits"],
                                         a["out_sym_off"], a["out_index"], a["index_cap"], a["chunk"], a["status"])
    blk = mhc.select_args(src, a["n_sources"], a["picks"], a["n_picks"], a["out"], a["cap"], a["out_off"], a["out_nbits"], a["out_sym_off"],
                          a["out_index"], a["index_cap"], a["chunk"], a["status"], a["ws"], a["wsb"], None)
    if a["struct_size"] is not None:
        blk.struct_size = a["struct_size"]
    return mhc.lib().mh_dev_select_batch(C.byref(blk))


@pytest.mark.parametrize("form", ["dev", "host"])
def test_select_refuses_bad_arguments_before_any_launch(mhc, form):
    ARG = mhc.MH_ERR_ARG
    w, p = _room()
    sel = lambda **kw: _select(mhc, form, p, **kw)
    assert sel(n_sources=0) == ARG and sel(n_sources=9) == ARG and sel(sources=None) == ARG
    for k in ("pay_off", "nbits", "picks", "out_off", "out_nbits", "payload"):
        assert sel(**{k: None}) == ARG, k
    # an index is written only when every source has one with the block's chunk size, and symbol offsets
    assert sel(index=None) == ARG and sel(src_chunk=1024) == ARG and sel(sym_off=None) == ARG
    for bad_chunk in (0, 100, 128, 300, 16384):
        assert sel(chunk=bad_chunk, src_chunk=bad_chunk) == ARG, bad_chunk
    other = (p, p, p, 1, 16, p, 100, None, 0)                   # a second source without an index
    assert sel(n_sources=2, second=other) == ARG
    other = (p, p, p, 1, 16, p, 100, p, 1024)                   # ... with another chunk size
    assert sel(n_sources=2, second=other) == ARG
    other = (p, p, p, 1, 16, None, 0, None, 0)                  # ... without symbol offsets: out_sym_off must be NULL
    assert sel(n_sources=2, second=other, out_index=None) == ARG
    if form == "dev":
        assert _select(mhc, "dev", p, struct_size=0) == ARG and _select(mhc, "dev", p, struct_size=C.sizeof(mhc.SelectArgs) + 8) == ARG
        assert mhc.lib().mh_dev_select_batch(None) == ARG
        assert sel(ws=None) == ARG and sel(ws=p + 8) == ARG and sel(out=p + 8) == ARG
        assert sel(wsb=64) == mhc.MH_ERR_CAPACITY
        if mhc.device_count() == 0:
            NO = mhc.MH_ERR_NO_DEVICE
            assert sel() == NO and sel(out=None) == NO and sel(out_index=None, out_sym_off=None, sym_off=None, index=None) == NO
            assert sel(n_picks=0, picks=None, out_nbits=None) == NO and sel(status=None) == NO


def test_host_select_refuses_bad_offsets(mhc):
    c = select_cases.case("two sources, order 1, chunk 1024")
    picks = c.picks["identity"]
    src = c.sources()
    assert mhc.select_batch(src, picks, c.chunk).status == mhc.MH_OK
    def broken(field, change):
        rows = list(src)
        row = list(rows[1])
        row[field] = np.asarray(row[field], dtype=np.uint64).copy()
        change(row[field])
        rows[1] = tuple(row)
        return mhc.select_batch(rows, picks, c.chunk).status

    def first_not_zero(a):
        a += np.uint64(1)

    def decreasing(a):
        a[2] = a[3] + np.uint64(1)
    for field in (1, 3):                                                                           # pay_off, sym_off
        assert broken(field, first_not_zero) == mhc.MH_ERR_ARG and broken(field, decreasing) == mhc.MH_ERR_ARG, field
    # [n] != total: the description says 16 bytes more than the offsets
    rows, keep = mhc._select_sources(src, lambda a: a)
    rows[0].pay_total += 16
    out = np.zeros(1 << 16, dtype=np.uint64)
    pk = np.ascontiguousarray(picks, dtype=np.uint64)
    at = out.ctypes.data
    assert mhc.lib().mh_select_batch(rows, 2, pk.ctypes.data, pk.size, None, 0, at, at + 8192, None, None, 0, 0, None) == mhc.MH_ERR_ARG
    rows[0].pay_total -= 16
    assert mhc.lib().mh_select_batch(rows, 2, pk.ctypes.data, pk.size, None, 0, at, at + 8192, None, None, 0, 0, None) == mhc.MH_OK
    rows[1].sym_total += 1
    assert mhc.lib().mh_select_batch(rows, 2, pk.ctypes.data, pk.size, None, 0, at, at + 8192, None, None, 0, 0, None) == mhc.MH_ERR_ARG


def test_picks_refuse_bad_arguments_before_any_launch(mhc):
    ARG = mhc.MH_ERR_ARG
    lib = mhc.lib()
    w, p = _room()
    assert lib.mh_picks_from_hits(p, p, 4, 0, 0, None, p) == ARG and lib.mh_picks_from_hits(p, p, 4, 0, 0, p, None) == ARG
    assert lib.mh_picks_from_hits(p, p, 4, 8, 0, p, p) == ARG and lib.mh_picks_from_hits(p, p, 4, 0, 2, p, p) == ARG

    def dev(**kw):
        a = dict(hit_off=p, status=p, n=4, source=0, flags=0, picks=p, kept=p, ws=p, wsb=1 << 16, struct_size=None)
        a.update(kw)
        blk = mhc.picks_args(a["hit_off"], a["status"], a["n"], a["source"], a["flags"], a["picks"], a["kept"], a["ws"], a["wsb"], None)
        if a["struct_size"] is not None:
            blk.struct_size = a["struct_size"]
        return lib.mh_dev_picks_from_hits(C.byref(blk))
    assert lib.mh_dev_picks_from_hits(None) == ARG and dev(struct_size=4) == ARG
    assert dev(picks=None) == ARG and dev(kept=None) == ARG and dev(source=8) == ARG and dev(flags=2) == ARG and dev(flags=3) == ARG
    assert dev(ws=None) == ARG and dev(ws=p + 8) == ARG and dev(wsb=64) == mhc.MH_ERR_CAPACITY
    if mhc.device_count() == 0:
        NO = mhc.MH_ERR_NO_DEVICE
        assert dev() == NO and dev(hit_off=None) == NO and dev(status=None) == NO and dev(flags=1) == NO and dev(n=0, picks=None) == NO
