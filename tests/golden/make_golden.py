#!/usr/bin/env python3
"""Regenerate tests/golden/ with the GENUINE reference binary (oracle/_ref/markovhuffman).

Runs only in the build container (needs /root/reference to build oracle/_ref; see oracle/Makefile).
What is committed is DATA: the inputs (the reference's own test/input files and formula-defined
known-answer inputs) and the reference's outputs on them:
    X.cm / X.e   Markov stream / table      (markovhuffman X -o X.cm -d X.e)
    X.ch / X.eh  Huffman stream / table     (markovhuffman X -o X.ch -h -d X.eh)
plus golden.json with sizes and sha256 of everything.  Both decodes are run and compared with the
input before anything is written (the round trip of test/main.py:17-50,77).

differential.json: the reference on the seeded random inputs of tests/test_oracle_golden.py's differential
test (input, stream and table pinned by size and sha256; the tables in full as differential/diff_s<seed>_o<order>.e).
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "markovhuffman")
REF_INPUTS = "/root/reference/test/input"


def kat_inputs():
    """Formula-defined inputs; regenerable anywhere without the reference."""
    out = {}
    out["kat1"] = b"aaaabbcd"
    out["kat2"] = bytes((i * i + 7 * i) % 251 for i in range(100000))
    out["kat3"] = bytes(range(256)) * 64
    x = 12345
    buf = bytearray()
    for _ in range(1 << 20):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        buf.append(((x >> 16) & 0xFF) & ((x >> 8) & 0xFF))
    out["kat4"] = bytes(buf)
    out["empty"] = b""
    out["one_Z"] = b"Z"
    out["nine_Z"] = b"Z" * 9
    return out


def differential_input(seed):
    """Seeded random inputs (same formulas as tests/test_oracle_golden.py); regenerable anywhere without the reference."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1000, 200000))
    kind = seed % 3
    if kind == 0:
        data = rng.integers(0, 256, n, dtype=np.uint8)
    elif kind == 1:
        data = np.minimum(rng.geometric(0.08, n) - 1, 255).astype(np.uint8)
    else:
        w = 1.0 / np.arange(1, 257) ** 1.1
        data = rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)
    return data.tobytes()


def sha(b):
    return hashlib.sha256(b).hexdigest()


def run(args):
    subprocess.run([REF_BIN] + args, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("oracle/_ref/markovhuffman missing: run `make -C oracle ref` in the build container")
    inputs = {}
    for name in sorted(os.listdir(REF_INPUTS)):
        with open(os.path.join(REF_INPUTS, name), "rb") as f:
            inputs[name] = f.read()
    inputs.update(kat_inputs())

    in_dir = os.path.join(HERE, "inputs")
    exp_dir = os.path.join(HERE, "expected")
    for d in (in_dir, exp_dir):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)

    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in inputs.items():
            src = os.path.join(tmp, name)
            with open(src, "wb") as f:
                f.write(data)
            p = lambda ext: os.path.join(tmp, name + ext)
            run([src, "-o", p(".cm"), "-d", p(".e")])
            run([src, "-o", p(".ch"), "-h", "-d", p(".eh")])
            entry = {"size": len(data), "sha256": sha(data), "formula": name in kat_inputs()}
            # round trips (Huffman decode of an empty table crashes in the reference: skip it)
            run([p(".cm"), "-o", p(".dm"), "-x", "-e", p(".e")])
            assert open(p(".dm"), "rb").read() == data, name
            if len(data):
                run([p(".ch"), "-o", p(".dh"), "-xh", "-e", p(".eh")])
                assert open(p(".dh"), "rb").read() == data, name
            for ext in (".cm", ".e", ".ch", ".eh"):
                b = open(p(ext), "rb").read()
                entry[ext[1:]] = {"size": len(b), "sha256": sha(b)}
                # large formula-defined cases are pinned by hash only (regenerable); the rest in full
                if not (entry["formula"] and len(data) > 1000):
                    with open(os.path.join(exp_dir, name + ext), "wb") as f:
                        f.write(b)
            # -g debug dumps (stdout of print_table + print_tree, src/main.cpp:186-190) for small cases
            if name in ("input_a.txt", "input_b.txt", "input_ipsum.txt", "one_Z", "nine_Z"):
                for ext, extra in ((".g", []), (".gh", ["-h"])):
                    r = subprocess.run([REF_BIN, src, "-o", os.devnull, "-g"] + extra, check=True,
                                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
                    entry[ext[1:]] = {"size": len(r.stdout), "sha256": sha(r.stdout)}
                    with open(os.path.join(exp_dir, name + ext), "wb") as f:
                        f.write(r.stdout)
            # the reference's own inputs are committed as data; formula inputs are regenerated
            if not entry["formula"]:
                with open(os.path.join(in_dir, name), "wb") as f:
                    f.write(data)
            meta[name] = entry
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", len(meta), "golden entries")
    differential()


def differential():
    out_dir = os.path.join(HERE, "differential")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in (1, 2, 3):
            data = differential_input(seed)
            src = os.path.join(tmp, "in.bin")
            with open(src, "wb") as f:
                f.write(data)
            for order in (0, 1):
                c, e, d = (os.path.join(tmp, "out" + x) for x in (".c", ".e", ".d"))
                run([src] + (["-h"] if order == 0 else []) + ["-o", c, "-d", e])
                run([c, "-o", d] + (["-xh"] if order == 0 else ["-x"]) + ["-e", e])
                assert open(d, "rb").read() == data, (seed, order)
                stream, table = open(c, "rb").read(), open(e, "rb").read()
                name = "diff_s%d_o%d" % (seed, order)
                meta[name] = {"seed": seed, "order": order, "size": len(data), "sha256": sha(data),
                              "c": {"size": len(stream), "sha256": sha(stream)},
                              "e": {"size": len(table), "sha256": sha(table)}}
                with open(os.path.join(out_dir, name + ".e"), "wb") as f:
                    f.write(table)
    with open(os.path.join(HERE, "differential.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", len(meta), "differential entries")


if __name__ == "__main__":
    main()
