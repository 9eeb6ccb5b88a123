"""CPU-side checks of the arguments every call that reads a compressed batch shares (payload, pay_off, nbits, n_streams,
pay_total, prev0, sym_off, sym_total, index, chunk_symbols): one table of bad-argument cases, run over every entry point that
takes the tuple, with the expected codes written here.  No call gets as far as a launch: a refused call returns before it
touches the device, and a valid one is made only where there is no device, where it returns MH_ERR_NO_DEVICE, which is what
shows the precedence of the checks.  A (call, case) pair that does not apply is listed with its reason, and the test asserts
that every pair ran or is listed."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry

ARG, CAPACITY, NO_DEVICE = "MH_ERR_ARG", "MH_ERR_CAPACITY", "MH_ERR_NO_DEVICE"
N, PAY_TOTAL, SYM_TOTAL, CHUNK, PREV0 = 2, 32, 200, 256, 0x20

# ---- the cases: what is changed in a valid call, and the code the call must return --------------------------------------------
# device calls: every pointer is a 256-aligned stand-in W (nothing reads it before the checks are over); "W+4": misaligned
DEV_CASES = {
    "null pay_off": (dict(pay_off=None), ARG),
    "null nbits, n > 0": (dict(nbits=None), ARG),
    "null payload, pay_total > 0": (dict(payload=None), ARG),
    "misaligned payload": (dict(payload="W+4"), ARG),
    "misaligned workspace": (dict(ws="W+8"), ARG),
    "index, chunk_symbols 0": (dict(chunk=0), ARG),
    "index, chunk_symbols not a power of two": (dict(chunk=300), ARG),
    "index, chunk_symbols under MH_CHUNK_MIN": (dict(chunk=128), ARG),
    "index, chunk_symbols over MH_CHUNK_MAX": (dict(chunk=16384), ARG),
    "index, no sym_off": (dict(sym_off=None), ARG),
    "workspace one byte short": (dict(ws_short=1), CAPACITY),                   # ... and the rest valid: not MH_ERR_NO_DEVICE
    "misaligned payload + short workspace": (dict(payload="W+4", ws_short=1), ARG),
    "valid, indexed": (dict(), NO_DEVICE),
    "valid, index-free": (dict(index=None, chunk=0, sym_total=0), NO_DEVICE),
}
# host forms: real arrays (two streams of 16 bytes, 120 and 128 bits, 100 symbols each)
HOST_CASES = {
    "null pay_off": (dict(pay_off=None), ARG),
    "null nbits, n > 0": (dict(nbits=None), ARG),
    "null payload, pay_total > 0": (dict(payload=None), ARG),
    "index, chunk_symbols 0": (dict(chunk=0), ARG),
    "index, chunk_symbols not a power of two": (dict(chunk=300), ARG),
    "index, chunk_symbols under MH_CHUNK_MIN": (dict(chunk=128), ARG),
    "index, chunk_symbols over MH_CHUNK_MAX": (dict(chunk=16384), ARG),
    "index, no sym_off": (dict(sym_off=None), ARG),
    "pay_off[0] != 0": (dict(pay_off=[1, 16, 32]), ARG),
    "decreasing pay_off": (dict(pay_off=[0, 16, 8]), ARG),
    "nbits one bit over its bytes": (dict(nbits=[129, 128]), ARG),
    "decreasing sym_off under an index": (dict(sym_off=[0, 100, 50]), ARG),
    "valid, indexed": (dict(), NO_DEVICE),
    "valid, index-free": (dict(index=None, chunk=0), NO_DEVICE),
}
VALID = ("valid, indexed", "valid, index-free")
INDEX_CASES = [c for c in DEV_CASES if c.startswith("index, ")]

NO_INDEX_PART = "the call takes no index: the batch is index-free by definition"
INDEX_IS_OUTPUT = "index and sym_off are outputs of the call, both required: there is no index-free form and sym_off is not read"
NEEDS_DEVICE = "the call's model (an order-2 model, a model set, a bank) can only be built on a device"
WOULD_LAUNCH = "with a device a valid call would launch kernels on the stand-in pointers"


class Call:
    def __init__(self, name, kind, needs, args, ws=None, na=None):
        self.name, self.kind, self.needs, self.args, self.ws, self.na = name, kind, needs, args, ws, dict(na or {})


def _calls():
    """Every entry point that takes the tuple.  args(t, x): the argument list from the tuple's fields t and the handles x."""
    c = []
    # --- device calls
    dec = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0, t["W"], 4096, t["sym_off"], t["sym_total"],
                                   t["index"], t["chunk"], t["W"], t["ws"], t["ws_bytes"], None])
    dec_ws = lambda l, t: l.mh_dev_decode_batch_workspace(N)
    c.append(Call("mh_dev_decode_batch", "dev", "o1", dec("o1"), dec_ws))
    c.append(Call("mh_dev_decode_batch_o2", "dev", "o2", dec("o2"), dec_ws))
    c.append(Call("mh_dev_decode_each", "dev", "set", dec("set"), dec_ws))
    find = lambda m, s: (lambda t, x: [x[m], x[s], t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0, t["sym_off"], t["sym_total"],
                                       t["index"], t["chunk"], t["W"], t["W"], t["W"], 16, t["W"], t["ws"], t["ws_bytes"], None])
    find_ws = lambda l, t: l.mh_dev_find_batch_workspace(N, t["sym_total"], t["chunk"] if t["index"] else 0)
    for name, m, s in (("mh_dev_find_batch", "o1", "ps"), ("mh_dev_find_batch_o2", "o2", "ps"), ("mh_dev_find_each", "set", "ps"),
                       ("mh_dev_find_dict_batch", "o1", "dict"), ("mh_dev_find_dict_batch_o2", "o2", "dict"), ("mh_dev_find_dict_each", "set", "dict")):
        c.append(Call(name, "dev", m, find(m, s), find_ws))
    crc = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0, t["sym_off"], t["sym_total"], t["index"],
                                   t["chunk"], t["W"], t["W"], t["W"], t["ws"], t["ws_bytes"], None])
    crc_ws = lambda l, t: l.mh_dev_crc_batch_workspace(N, t["sym_total"], t["chunk"])
    for name, m in (("mh_dev_crc_batch", "o1"), ("mh_dev_crc_batch_o2", "o2"), ("mh_dev_crc_each", "set")):
        c.append(Call(name, "dev", m, crc(m), crc_ws))
    hist = lambda m, order: (lambda t, x: [x[m], order, t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0, t["sym_off"], t["sym_total"],
                                           t["index"], t["chunk"], t["W"], t["W"], t["ws"], t["ws_bytes"], None])
    hist_ws = lambda l, t: l.mh_dev_histogram_coded_workspace(N, t["sym_total"], t["chunk"])
    c.append(Call("mh_dev_histogram_coded_batch", "dev", "o1", hist("o1", 1), hist_ws))
    c.append(Call("mh_dev_histogram_coded_each", "dev", "set", hist("set", 1), hist_ws))
    c.append(Call("mh_dev_histogram_coded_batch_o2", "dev", "o1", hist("o1", 2), hist_ws))   # an order-0/1 source counted in order 2
    rec = lambda m, edit: (lambda t, x: [x[m], x["o1"], t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0, t["sym_off"], t["sym_total"],
                                         t["index"], t["chunk"]] + ([t["W"], t["W"], t["W"]] if edit else []) +
                           [t["W"], 4096, t["W"], t["W"], None, t["W"], t["W"], t["ws"], t["ws_bytes"], None])
    rec_ws = lambda l, t: l.mh_dev_recode_batch_workspace(N, t["sym_total"], t["chunk"] if t["index"] else 0)
    rec_o2_ws = lambda l, t: l.mh_dev_recode_batch_o2_workspace(N, t["sym_total"], t["chunk"] if t["index"] else 0)
    c.append(Call("mh_dev_recode_batch", "dev", "o1", rec("o1", False), rec_ws))
    c.append(Call("mh_dev_recode_each", "dev", "set", rec("set", False), rec_ws))
    c.append(Call("mh_dev_recode_batch_o2", "dev", "o2", rec("o2", False), rec_o2_ws))
    c.append(Call("mh_dev_recode_edit_batch", "dev", "o1", rec("o1", True), rec_ws))
    c.append(Call("mh_dev_recode_edit_each", "dev", "set", rec("set", True), rec_ws))
    look = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["sym_off"], t["index"], t["chunk"], t["W"], 3, t["W"],
                                    t["W"], 4096, t["W"], t["ws"], t["ws_bytes"], None])
    look_ws = lambda l, t: l.mh_dev_decode_batch_ranges_workspace(3)
    for name, m in (("mh_dev_decode_batch_ranges", "o1"), ("mh_dev_decode_batch_o2_ranges", "o2"), ("mh_dev_decode_each_ranges", "set")):
        c.append(Call(name, "dev", m, look(m), look_ws))
    # the segment-state calls: no sym_off or index is read; mh_dev_*_index writes an index, so its chunk size is checked
    st_ws = lambda l, t: l.mh_dev_batch_states_workspace(N, PAY_TOTAL)
    head = lambda m, t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PAY_TOTAL, PREV0]
    tail = lambda t: [t["W"], t["ws"], t["ws_bytes"], None]
    no_index = {k: NO_INDEX_PART for k in INDEX_CASES}
    for suffix, m in (("batch", "o1"), ("each", "set"), ("batch", "o2")):
        o2 = "_o2" if m == "o2" else ""
        c.append(Call("mh_dev_%s_states%s" % (suffix, o2), "dev", m, (lambda m: lambda t, x: head(m, t, x) + [t["W"]] + tail(t))(m), st_ws,
                      dict(no_index, **{"valid, index-free": "the one valid form is listed as 'valid, indexed'"})))
        c.append(Call("mh_dev_%s_index%s" % (suffix, o2), "dev", m, (lambda m: lambda t, x: head(m, t, x) + [t["W"], 64, t["chunk"]] + tail(t))(m),
                      st_ws, {"index, no sym_off": INDEX_IS_OUTPUT, "valid, index-free": INDEX_IS_OUTPUT}))
        c.append(Call("mh_dev_%s_emit%s" % (suffix, o2), "dev", m, (lambda m: lambda t, x: head(m, t, x) + [t["W"], 4096] + tail(t))(m), st_ws,
                      dict(no_index, **{"valid, index-free": "the one valid form is listed as 'valid, indexed'"})))
    # --- host forms
    hdec = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["out"], 4096, t["sym_off"], t["index"], t["chunk"], t["st"]])
    c.append(Call("mh_decode_batch", "host", "o1", hdec("o1")))
    c.append(Call("mh_decode_batch_o2", "host", "o2", hdec("o2")))
    c.append(Call("mh_decode_bank", "host", "set", lambda t, x: [x["set"], t["choice"], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["out"], 4096,
                                                                 t["sym_off"], t["index"], t["chunk"], t["st"]]))
    c.append(Call("mh_decompress_each", "host", "o1", lambda t, x: [x["tables"], x["tab_off"], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["out"],
                                                                     4096, t["sym_off"], t["index"], t["chunk"], t["st"]]))
    hfind = lambda m, s: (lambda t, x: [x[m], x[s], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["sym_off"], t["index"], t["chunk"], t["hit_off"],
                                        t["out"], t["out"], 16, t["st"]])
    for name, m, s in (("mh_find_batch", "o1", "ps"), ("mh_find_batch_o2", "o2", "ps"), ("mh_find_dict_batch", "o1", "dict"),
                       ("mh_find_dict_batch_o2", "o2", "dict")):
        c.append(Call(name, "host", m, hfind(m, s)))
    hcrc = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["sym_off"], t["index"], t["chunk"], t["out"], t["out"], t["st"]])
    c.append(Call("mh_crc_batch", "host", "o1", hcrc("o1")))
    c.append(Call("mh_crc_batch_o2", "host", "o2", hcrc("o2")))
    hrec = lambda m, edit: (lambda t, x: [x[m], x["o1"], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["sym_off"], t["index"], t["chunk"]] +
                            ([None, None, t["map"]] if edit else []) + [t["out"], 4096, t["hit_off"], t["out"], None, t["out"], t["st"]])
    c.append(Call("mh_recode_batch", "host", "o1", hrec("o1", False)))
    c.append(Call("mh_recode_batch_o2", "host", "o2", hrec("o2", False)))
    c.append(Call("mh_recode_edit_batch", "host", "o1", hrec("o1", True)))
    hidx = lambda m: (lambda t, x: [x[m], t["payload"], t["pay_off"], t["nbits"], N, PREV0, t["chunk"], t["sym_off"], t["out"], 64, t["st"]])
    idx_na = {"decreasing sym_off under an index": INDEX_IS_OUTPUT, "valid, index-free": INDEX_IS_OUTPUT}
    c.append(Call("mh_index_batch", "host", "o1", hidx("o1"), na=idx_na))
    c.append(Call("mh_index_batch_o2", "host", "o2", hidx("o2"), na=idx_na))
    return c


@pytest.fixture(scope="module")
def mhc():
    mod = entry.load_package()
    if not os.path.exists(mod.LIB_PATH):
        entry.build()
    return mod


@pytest.fixture(scope="module")
def handles(mhc):
    """What the calls take beside the tuple; the keys a machine cannot build are missing."""
    o1 = mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)
    table = np.frombuffer(o1.table_bytes(), dtype=np.uint8)
    tabs, tab_off = np.concatenate([table, table]), np.array([0, table.size, 2 * table.size], dtype=np.uint64)
    ps, dic = mhc.PatternSet([b"ab", b"c"]), mhc.Dict([b"ab", b"c"])
    keep = [o1, tabs, tab_off, ps, dic]
    x = {"o1": o1.handle, "ps": ps.handle, "dict": dic.handle, "tables": tabs.ctypes.data, "tab_off": tab_off.ctypes.data, "_keep": keep}
    if mhc.device_count() > 0:
        counts = np.zeros(1 << 24, dtype=np.uint64)
        counts[(0x2020 << 8) | 65] = 3
        counts[(0x2041 << 8) | 66] = 2
        o2 = mhc.Model.from_counts(counts, 2)
        s = mhc.ModelSet.from_models([o1, o1])
        keep.extend([o2, s])
        x["o2"], x["set"] = o2.handle, s.handle
    return x


def _dev_tuple(lib, call, over):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    W = (buf.ctypes.data + 255) & ~255
    sym = {"W": W, "W+4": W + 4, "W+8": W + 8, None: None}
    t = dict(W=W, payload=W, pay_off=W, nbits=W, sym_off=W, sym_total=SYM_TOTAL, index=W, chunk=CHUNK, ws=W, _buf=buf)
    for k, v in over.items():
        if k != "ws_short":
            t[k] = sym[v] if k in ("payload", "pay_off", "nbits", "sym_off", "index", "ws") else v
    t["ws_bytes"] = int(call.ws(lib, t)) - over.get("ws_short", 0)
    return t


def _host_tuple(over):
    a = dict(payload=np.zeros(32, dtype=np.uint8), pay_off=[0, 16, 32], nbits=[120, 128], sym_off=[0, 100, 200], index=np.zeros(8, dtype=np.uint64),
             chunk=CHUNK)
    a.update(over)
    keep = []

    def ptr(v):
        if v is None:
            return None
        arr = np.ascontiguousarray(v, dtype=np.uint64) if isinstance(v, list) else v
        keep.append(arr)
        return arr.ctypes.data

    t = {k: ptr(a[k]) for k in ("payload", "pay_off", "nbits", "sym_off", "index")}
    t["chunk"] = a["chunk"]
    for k, arr in (("out", np.zeros(4096, dtype=np.uint8)), ("st", np.zeros(2, dtype=np.int32)), ("hit_off", np.zeros(3, dtype=np.uint64)),
                   ("choice", np.zeros(2, dtype=np.uint32)), ("map", np.arange(256, dtype=np.uint8))):
        t[k] = ptr(arr)
    t["_keep"] = keep
    return t


def test_every_reader_refuses_the_same_bad_batch_with_the_same_code(mhc, handles):
    lib = mhc.lib()
    code = {ARG: mhc.MH_ERR_ARG, CAPACITY: mhc.MH_ERR_CAPACITY, NO_DEVICE: mhc.MH_ERR_NO_DEVICE}
    have_device = mhc.device_count() > 0
    ran, listed = set(), {}
    for call in _calls():
        cases = DEV_CASES if call.kind == "dev" else HOST_CASES
        for case, (over, want) in cases.items():
            key = (call.name, case)
            if case in call.na:
                listed[key] = call.na[case]
            elif call.needs not in handles:
                listed[key] = NEEDS_DEVICE
            elif case in VALID and have_device:
                listed[key] = WOULD_LAUNCH
            else:
                over = dict(over)
                if case == "valid, index-free" and call.name.startswith(("mh_dev_decode", "mh_dev_recode", "mh_decode", "mh_recode", "mh_decompress")):
                    pass                                        # (sym_off stays: these calls write it when index-free)
                elif case == "valid, index-free":
                    over["sym_off"] = None
                t = _dev_tuple(lib, call, over) if call.kind == "dev" else _host_tuple(over)
                got = getattr(lib, call.name)(*call.args(t, handles))
                assert got == code[want], (call.name, case, got, want)
                ran.add(key)
    every = {(call.name, case) for call in _calls() for case in (DEV_CASES if call.kind == "dev" else HOST_CASES)}
    assert ran | set(listed) == every and not ran & set(listed)
    assert all(isinstance(r, str) and r for r in listed.values())
    # what runs everywhere: every case of the calls under an order-0/1 model (264 pairs); with a device the refusals of the
    # order-2, set and bank calls join in, and only the valid calls stay out
    assert len(ran) >= 264, (len(ran), len(listed))
    if have_device:
        assert NEEDS_DEVICE not in listed.values()
        assert {case for (_, case), r in listed.items() if r == WOULD_LAUNCH} == set(VALID)
