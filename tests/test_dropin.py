"""The coding.h face as a drop-in for the reference's own caller.

oracle/Makefile (`make dropin`, part of __graft_entry__.build() when /root/reference is present) compiles
the reference's src/main.cpp WHERE IT LIES against markov-huffman-coding_amd/host/ (its quoted includes
"bitbuffer.h", "coding.h", "huffman.h", "markov_huffman.h", "utils.h" resolve to the product's headers)
and links it with host/coding.cpp + libmhc.so into oracle/_ref/markovhuffman_refmain.  Nothing of the
reference is copied into the repo; the binary is a built artefact like oracle/_ref/markovhuffman.

CPU: build() made the binary (compile and link succeeded) and it starts (argc < 2 -> help text, exit 1, src/main.cpp:42-45).
GPU: the reference's main() drives the HIP path: its outputs equal the golden files of the genuine reference.
"""
import os
import subprocess

import pytest

from conftest import ROOT, check_against_golden, golden, golden_names

BIN = os.path.join(ROOT, "oracle", "_ref", "markovhuffman_refmain")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "markovhuffman")


def test_reference_main_compiles_and_links_against_the_host_face():
    """build() (oracle/Makefile `all`) compiles the drop-in whenever the reference checkout is there, the same condition
    under which it compiles the reference itself: oracle/_ref/markovhuffman is the sign that it was."""
    if not os.path.exists(REF_BIN):
        pytest.skip("no reference checkout at build time (oracle/_ref/markovhuffman not built)")
    assert os.path.exists(BIN), "build() compiled the reference but not the drop-in oracle/_ref/markovhuffman_refmain"
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1
    assert b"markov-huffman <input> [-o output] [options]" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names())
def test_reference_main_runs_on_the_hip_path(tmp_path, name):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/markovhuffman_refmain not built (needs /root/reference at build time)")
    data = golden()[name]["data"]
    src = tmp_path / "in"
    src.write_bytes(data)
    run = lambda a: subprocess.run([BIN] + [str(x) for x in a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p = lambda ext: tmp_path / ("out." + ext)
    assert run([src, "-o", p("cm"), "-d", p("e")]).returncode == 0
    assert run([src, "-o", p("ch"), "-h", "-d", p("eh")]).returncode == 0
    for ext in ("cm", "e", "ch", "eh"):
        check_against_golden(name, ext, p(ext).read_bytes())
    assert run([p("cm"), "-o", p("dm"), "-x", "-e", p("e")]).returncode == 0
    assert p("dm").read_bytes() == data
