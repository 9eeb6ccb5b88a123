"""The token of a span without a GPU (include/mh.h, "TOKENS FROM MATCHED BYTES"): the published SipHash-2-4 answers on the
reference (tests/token_ref.py), mh_span_token_digest against that reference on every length 0 .. 64 and on 255 bytes with and
without the fold, the reference's apply against the table splice's reference, and the stand-alone sanitizer fuzz."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import splice_table_ref
import token_ref
from conftest import ROOT

KNOWN = [(0, 0x726fdb47dd0e0e31), (8, 0x93f5f5799a932462), (15, 0xa129ca6149be45e5), (63, 0x958a324ceb064572)]


@pytest.fixture(scope="module")
def mhc():
    entry.build()
    return entry.load_package()


def lib_digest(mhc, key, data, flags=0):
    k, d = np.frombuffer(bytes(key), dtype=np.uint8), np.frombuffer(bytes(data), dtype=np.uint8)
    return int(mhc.lib().mh_span_token_digest(k.ctypes.data, d.ctypes.data if len(d) else None, len(d), flags))


def test_known_answers_of_the_reference():
    for n, want in KNOWN:
        assert token_ref.siphash24(token_ref.KEY, bytes(range(n))) == want, n


def test_known_answers_of_the_library(mhc):
    for n, want in KNOWN:
        assert lib_digest(mhc, token_ref.KEY, bytes(range(n))) == want, n


def test_digest_equals_the_reference_on_every_length_to_64_and_on_255_bytes(mhc):
    rng = np.random.default_rng(5)
    for n in list(range(65)) + [255]:
        for trial in range(3):
            key = bytes(rng.integers(0, 256, size=16, dtype=np.uint8))
            # bytes of every class: letters of both cases and their neighbours '@', '[', '`', '{', and anything
            data = bytes(rng.choice(np.frombuffer(b"@AZ[`az{Mm\x00\xff", dtype=np.uint8), size=n)) if trial else bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
            for flags in (0, token_ref.FOLD):
                assert lib_digest(mhc, key, data, flags) == token_ref.digest(key, data, flags), (n, trial, flags)
    mixed = b"Alice.Smith@Example.COM"
    assert lib_digest(mhc, token_ref.KEY, mixed, token_ref.FOLD) == lib_digest(mhc, token_ref.KEY, mixed.lower(), 0)
    assert lib_digest(mhc, token_ref.KEY, mixed, 0) != lib_digest(mhc, token_ref.KEY, mixed.lower(), 0)
    assert lib_digest(mhc, token_ref.KEY, b"@[`{", token_ref.FOLD) == lib_digest(mhc, token_ref.KEY, b"@[`{", 0)   # the neighbours of A-Z stay


def test_reference_token_formats():
    d = token_ref.digest(token_ref.KEY, b"abc")
    full = ("%016x" % d).encode()
    assert token_ref.token((b"<EMAIL:", 16, b">"), token_ref.KEY, b"abc") == b"<EMAIL:" + full + b">"
    assert token_ref.token((b"", 1, b""), token_ref.KEY, b"abc") == full[:1]
    assert token_ref.token((b"<IP>", 0, b""), token_ref.KEY, b"abc") == b"<IP>"
    assert token_ref.token((b"", 0, b""), token_ref.KEY, b"abc") == b""
    assert token_ref.token((b"x", 15, b"yz"), token_ref.KEY, b"abc") == b"x" + full[:15] + b"yz"
    off, blob, hexd = token_ref.format_arrays([(b"<EMAIL:", 16, b">"), (b"<IP>", 0, b""), (b"", 4, b"#")])
    assert off.tolist() == [0, 7, 8, 12, 12, 12, 13] and blob.tobytes() == b"<EMAIL:><IP>#" and hexd.tolist() == [16, 0, 4]
    assert token_ref.formats_ok([(b"a" * 239, 16, b"")]) and not token_ref.formats_ok([(b"a" * 239, 16, b"b")])


def test_reference_apply_is_the_table_splice_with_the_token_table():
    msgs = [b"mail alice@example.com or ALICE@EXAMPLE.COM from 10.0.0.1", b"", b"bob@example.com", b"short"]
    formats = [(b"<EMAIL:", 16, b">"), (b"<IP>", 0, b""), (b"", 0, b"")]
    off, sp, tg = splice_table_ref.tagged_lists([[(0, 0, 1), (5, 22, 0), (26, 43, 0), (49, 57, 1)], [(0, 0, 0)], [(0, 15, 0), (15, 15, 1)],
                                                 [(1, 3, 2), (4, 99, 0), (7, 9, 0)]])
    for flags in (0, token_ref.FOLD):
        entries = token_ref.table(msgs, off, sp, tg, formats, token_ref.KEY, flags)
        assert len(entries) == len(sp)
        got = token_ref.apply(msgs, off, sp, tg, formats, token_ref.KEY, flags)
        assert got == splice_table_ref.apply(msgs, off, sp, np.arange(len(sp)), entries)
        a, b = entries[1], entries[2]
        assert (a == b) == bool(flags) and a.startswith(b"<EMAIL:") and len(a) == 24
        assert got[0] == b"<IP>mail " + a + b" or " + b + b" from <IP>"
        assert got[1] == b"" and got[2] == entries[5]                       # (an insertion at len(x) is ignored)
        assert got[3] == b"s" + b"r" + token_ref.token(formats[0], token_ref.KEY, b"t", flags)
        # a span that begins at or beyond the length has the empty string's token in the table, and the splice ignores it
        assert entries[9] == token_ref.token(formats[0], token_ref.KEY, b"", flags)
    off1, bytes1, tag1 = token_ref.table_arrays([b"ab", b"", b"cde"], 5)
    assert off1.tolist() == [0, 2, 2, 5, 5, 5] and bytes1.tobytes() == b"abcde" and tag1.tolist() == [0, 1, 2, 3, 4]
    assert token_ref.table(msgs, off, sp, tg, formats, token_ref.KEY, failed={0})[:4] == [b""] * 4


def test_the_sanitizer_fuzz_of_the_digest_and_the_format_rules(mhc):
    """csrc/sanitize/fuzz_tokens.cpp: a stand-alone program over mh_token_host.cpp, the sanitizer runtimes linked in."""
    csrc = os.path.join(ROOT, "markov-huffman-coding_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "fuzz_tokens"])
    r = subprocess.run([os.path.join(csrc, "build", "fuzz_tokens"), "4000", "11"], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"4000 cases, 0 mismatches" in r.stdout, (r.stdout[-400:], r.stderr[-2000:])
