"""CPU-side checks of include/mh.h "ORDER 2 IN EDITING AND SPLICING": the entry points and sizing calls are declared, exported
and bound; the argument blocks have the layout of the ctypes structures; the workspaces are the stated arithmetic; the block
rules and the host forms' argument checks come before a device is touched; the section says what is left out.  An order-2
model lives on a device alone: without a device the device calls answer MH_ERR_NO_DEVICE behind the block's own checks, and
the host forms' checks that need an order-2 model are in tests/test_gpu_edit_o2.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import ROOT

ENTRY_POINTS = ["mh_dev_recode_edit_batch_o2", "mh_dev_recode_splice_table_batch_o2", "mh_recode_edit_batch_o2", "mh_recode_splice_table_batch_o2"]
SIZING = ["mh_dev_recode_edit_batch_o2_workspace", "mh_dev_recode_splice_table_batch_o2_workspace"]
HEADER = os.path.join(ROOT, "include", "mh.h")


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


@pytest.fixture(scope="module")
def model(mhc):
    return mhc.Model.from_counts(np.ones(65536, dtype=np.uint64), 1)


@pytest.fixture(scope="module")
def model0(mhc):
    return mhc.Model.from_counts(np.ones(256, dtype=np.uint64), 0)


def section():
    header = open(HEADER).read()
    at = header.index("ORDER 2 IN EDITING AND SPLICING (extension, parity unpinned)")
    return header[at:header.index("SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES")]


def test_entry_points_and_sizing_calls_are_declared_exported_and_bound(mhc):
    s = section()
    lib = C.CDLL(mhc.LIB_PATH)
    for name in ENTRY_POINTS + SIZING:
        assert name + "(" in s, name
        assert hasattr(lib, name), name
        assert name in mhc.EXPORTS, name
    for name in ("dev_recode_edit_batch_o2", "dev_recode_splice_table_batch_o2", "recode_edit_batch_o2", "recode_splice_table_batch_o2"):
        assert hasattr(mhc.Model, name), name
    # the section stands behind the table splice's, whose text is as it was
    header = open(HEADER).read()
    assert header.index("SPLICING WITH A REPLACEMENT TABLE (extension") < header.index("ORDER 2 IN EDITING AND SPLICING (extension")
    assert "order 2 is MH_ERR_ARG before any launch" in header[:header.index("ORDER 2 IN EDITING AND SPLICING (extension")]


def test_the_section_names_what_is_left_out_and_why_the_calls_take_a_block():
    s = re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", section()))
    left = s[s.index("Left out:"):]
    for what in ("the CLI", "model sets", "the table splice of an order-0/1 source under an order-2 destination", "appending at len(x)",
                 "replacements longer than MH_SPLICE_MAX_REP", "back-references"):
        assert what in left, what
    for what in ("2 -> 2, 2 -> 1, 2 -> 0, 1 -> 2, 0 -> 2", "Shared models only", "struct_size must equal sizeof of the struct",
                 "a NULL block is MH_ERR_ARG", "MH_ERR_NO_DEVICE", "indexed versus index-free alone", "no separate single-replacement call",
                 "more than thirty positional pointers", "positional `void *stream`"):
        assert what in s, what


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mh.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m))
int main(void) {
    printf("mh_coded_batch_args sizeof %zu\n", sizeof(mh_coded_batch_args));
    printf("mh_recode_edit_o2_args sizeof %zu\n", sizeof(mh_recode_edit_o2_args));
    printf("mh_recode_splice_o2_args sizeof %zu\n", sizeof(mh_recode_splice_o2_args));
@MEMBERS@
    return 0;
}
"""


def test_sizeof_and_member_offsets_equal_the_ctypes_structures(mhc, tmp_path):
    """The header compiled as C: sizeof and every member's offset against the binding's structures, member names included."""
    pairs = [("mh_coded_batch_args", mhc.CodedBatchArgs), ("mh_recode_edit_o2_args", mhc.RecodeEditO2Args),
             ("mh_recode_splice_o2_args", mhc.RecodeSpliceO2Args)]
    lines = "".join("    F(%s, %s);\n" % (cname, f[0]) for cname, cls in pairs for f in cls._fields_)
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE.replace("@MEMBERS@", lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls in pairs:
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for f in cls._fields_:
            assert got[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])
    # the members are the positional calls' parameters under the same names, in the same order
    header = re.sub(r"\s+", " ", open(HEADER).read())
    for twin, cls in [("mh_dev_recode_edit_batch", mhc.RecodeEditO2Args), ("mh_dev_recode_splice_table_batch", mhc.RecodeSpliceO2Args)]:
        params = re.search(r"int %s\(([^()]*)\);" % twin, header).group(1)
        names = [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")]
        flat = [g[0] for f in cls._fields_[1:] for g in (mhc.CodedBatchArgs._fields_ if f[0] == "batch" else [f])]
        assert flat == names, (twin, flat, names)
    assert mhc.RecodeEditO2Args._fields_[0][0] == "struct_size" and mhc.RecodeSpliceO2Args._fields_[-1][0] == "stream"


def test_the_workspaces_are_the_stated_arithmetic(mhc):
    l = mhc.lib()
    for a in [(0, 0, 1024), (1, 1, 256), (65536, 65536 * 4096, 1024), (7, 5000, 0), (7, 5000, 300), (26, 20000, 256)]:
        assert l.mh_dev_recode_edit_batch_o2_workspace(*a) == l.mh_dev_recode_batch_o2_workspace(*a), a
        assert l.mh_dev_recode_edit_batch_o2_workspace(*a) >= l.mh_dev_recode_edit_workspace(*a), a
        for ns, nr in [(0, 0), (1, 1), (100000, 4), (5, 65536)]:
            assert l.mh_dev_recode_splice_table_batch_o2_workspace(*a, ns, nr) == l.mh_dev_recode_splice_table_workspace(*a, ns, nr), (a, ns, nr)
    # the seam: a closing context and a head, 4 bytes each, per chunk number (the totals are rounded to 256 bytes)
    n, total, c = 65536, 65536 * 4096, 1024
    nwork = total // c + n
    grow = l.mh_dev_recode_edit_batch_o2_workspace(n, total, c) - l.mh_dev_recode_edit_workspace(n, total, c)
    assert 8 * nwork - 256 - 16 <= grow <= 8 * nwork + 256 + 16, grow
    assert l.mh_dev_recode_edit_batch_o2_workspace(n, total, 0) == l.mh_dev_recode_edit_workspace(n, total, 0)   # index-free: no chunk, no seam


def _edit_block(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = [None, None, p, p, p, 1, 16, 0x20, p, 100, p, 256, p, p, p, p, 64, p, p, p, p, p, p, 1 << 16, None]
    blk = mhc.args_block(mhc.RecodeEditO2Args, *a)
    for k, v in kw.items():
        setattr(blk, k, v)
    return blk, w


def _splice_block(mhc, **kw):
    w = np.zeros(1 << 14, dtype=np.uint64)
    p = (w.ctypes.data + 255) & ~255
    a = [None, None, p, p, p, 1, 16, 0x20, p, 100, p, 256, p, p, p, p, p, 2, p, 64, p, p, p, p, 2, p, p, p, 1 << 16, None]
    blk = mhc.args_block(mhc.RecodeSpliceO2Args, *a)
    for k, v in kw.items():
        setattr(blk, k, v)
    return blk, w


def test_the_block_rules_come_first_and_a_call_without_a_device_says_so(mhc, model, model0):
    l = mhc.lib()
    ARG = mhc.MH_ERR_ARG
    assert l.mh_dev_recode_edit_batch_o2(None) == ARG and l.mh_dev_recode_splice_table_batch_o2(None) == ARG
    for fn, make, cls in [(l.mh_dev_recode_edit_batch_o2, _edit_block, mhc.RecodeEditO2Args),
                          (l.mh_dev_recode_splice_table_batch_o2, _splice_block, mhc.RecodeSpliceO2Args)]:
        size = C.sizeof(cls)
        for bad in (0, 8, size - 1, size + 1, size + 8):
            blk, keep = make(mhc, src=model.handle.value, dst=model0.handle.value, struct_size=bad)
            assert fn(C.byref(blk)) == ARG, (cls.__name__, bad)
        blk, keep = make(mhc, src=model.handle.value, dst=model0.handle.value)
        assert blk.struct_size == size
        # order 0/1 on both sides stays with the existing calls: MH_ERR_ARG here, behind the device test
        assert fn(C.byref(blk)) == (mhc.MH_ERR_NO_DEVICE if mhc.device_count() == 0 else ARG), cls.__name__
        blk, keep = make(mhc)                                                  # no models at all
        assert fn(C.byref(blk)) == (mhc.MH_ERR_NO_DEVICE if mhc.device_count() == 0 else ARG), cls.__name__
    for count in (26, 24, 0):                                                  # one too many, one too few, none
        with pytest.raises(TypeError):
            mhc.args_block(mhc.RecodeEditO2Args, *([None] * count))
    with pytest.raises(TypeError):
        mhc.args_block(mhc.RecodeSpliceO2Args, *([None] * 29))


def _host_edit(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64), map=np.arange(256, dtype=np.uint8),
             out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64),
             out_index=np.zeros(4, dtype=np.uint64), dropped=np.zeros(2, dtype=np.uint64), status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_edit_batch_o2(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index", "chunk",
                                                                 "span_off", "spans", "map", "out", "cap", "out_off", "out_nbits", "out_index",
                                                                 "dropped", "status")])


def _host_splice(mhc, src, dst, **kw):
    a = dict(src=src.handle if src is not None else None, dst=dst.handle if dst is not None else None, payload=np.zeros(32, dtype=np.uint8),
             pay_off=np.array([0, 16, 32], dtype=np.uint64), nbits=np.array([120, 128], dtype=np.uint64), n=2, prev0=0x20,
             sym_off=np.array([0, 100, 200], dtype=np.uint64), index=np.zeros(4, dtype=np.uint64), chunk=256,
             span_off=np.array([0, 1, 1], dtype=np.uint64), spans=np.array([3, 5], dtype=np.uint64), span_tag=np.array([1], dtype=np.uint32),
             rep_off=np.array([0, 0, 3], dtype=np.uint64), rep_bytes=np.frombuffer(b"[X]", dtype=np.uint8), n_reps=2,
             out=np.zeros(64, dtype=np.uint8), cap=64, out_off=np.zeros(3, dtype=np.uint64), out_nbits=np.zeros(2, dtype=np.uint64),
             out_sym_off=np.zeros(3, dtype=np.uint64), out_index=np.zeros(4, dtype=np.uint64), index_cap=4, dropped=np.zeros(2, dtype=np.uint64),
             status=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return mhc.lib().mh_recode_splice_table_batch_o2(*[p(a[k]) for k in ("src", "dst", "payload", "pay_off", "nbits", "n", "prev0", "sym_off", "index",
                                                                         "chunk", "span_off", "spans", "span_tag", "rep_off", "rep_bytes", "n_reps",
                                                                         "out", "cap", "out_off", "out_nbits", "out_sym_off", "out_index",
                                                                         "index_cap", "dropped", "status")])


def test_the_host_forms_check_their_arguments_before_a_device_is_touched(mhc, model, model0):
    ARG = mhc.MH_ERR_ARG
    # the order rules: no model, and order 0/1 on both sides (an order-0/1 source under the splice whatever the destination)
    for host in (_host_edit, _host_splice):
        assert host(mhc, None, model) == ARG and host(mhc, model, None) == ARG
        for s, d in [(model, model), (model, model0), (model0, model), (model0, model0)]:
            assert host(mhc, s, d) == ARG, host.__name__
    # the checks that need an order-2 model, which lives on a device alone, run on the device:
    # tests/test_gpu_edit_o2.py::test_the_host_forms_check_their_arguments_with_an_order_2_side
