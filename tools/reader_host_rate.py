#!/usr/bin/env python3
"""Wall-clock time of the host forms that read a compressed batch (mh_decode_batch, mh_decode_bank, mh_decompress_each,
mh_find_batch, mh_crc_batch, mh_recode_batch, mh_recode_edit_batch, mh_index_batch), indexed and index-free, through the
Python wrappers: upload, one device call, download.  The other *_rate tools time the device calls; this one times what the
host side of the C ABI adds around them (csrc/mh_api_reader.hpp).  MH_LIB selects the library, for parent / change / parent runs.

    python tools/reader_host_rate.py [--streams 16384] [--bytes 4096] [--reps 7] [--only decode_batch,crc_batch]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

CHUNK = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated variant name prefixes (default: all)")
    args = ap.parse_args()
    only = [o for o in args.only.split(",") if o]
    mhc = entry.load_package()
    if mhc.device_count() < 1:
        raise SystemExit("reader_host_rate.py needs a GPU")
    n, per = args.streams, args.bytes
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    raw = np.resize(text, n * per).tobytes()
    msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
    model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
    payload, pay_off, nbits, index, in_off = model.encode_batch(msgs, chunk_symbols=CHUNK)
    ps = mhc.PatternSet([b"template", b"class "])
    star = bytes([0x2A]) * 256
    span_off = np.arange(n + 1, dtype=np.uint64)
    spans = np.tile(np.array([[100, 164]], dtype=np.uint64), (n, 1))
    bank = mhc.ModelSet.from_models([model, model])
    choice = (np.arange(n) & 1).astype(np.uint32)
    each = mhc.compress_each(msgs[:n // 8], chunk_symbols=CHUNK)
    tables, blobs = [e[0] for e in each], [e[1] for e in each]
    idx_kw = dict(sym_off=in_off, index=index, chunk_symbols=CHUNK)
    calls = {
        "decode_batch": lambda kw: model.decode_batch(payload, pay_off, nbits, **kw),
        "decode_bank": lambda kw: mhc.decode_bank(bank, choice, payload, pay_off, nbits, **kw),
        "find_batch": lambda kw: model.find_batch(ps, payload, pay_off, nbits, **kw),
        "crc_batch": lambda kw: model.crc_batch(payload, pay_off, nbits, **kw),
        "recode_batch": lambda kw: model.recode_batch(model, payload, pay_off, nbits, **(kw or dict(chunk_symbols=CHUNK))),
        "recode_edit_batch": lambda kw: model.recode_edit_batch(model, payload, pay_off, nbits, star, span_off, spans,
                                                                **(kw or dict(chunk_symbols=CHUNK))),
    }
    res = {"tool": "reader_host_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "lib": mhc.LIB_PATH, "variants": {}}

    def timed(name, fn):
        if only and not any(name.startswith(o) for o in only):
            return
        fn()                                                    # warm-up: the staging ring, the first hipMalloc of each size
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["variants"][name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    for name, fn in calls.items():
        timed(name + "/indexed", lambda: fn(idx_kw))
        timed(name + "/index_free", lambda: fn({}))
    timed("index_batch", lambda: model.index_batch(payload, pay_off, nbits, CHUNK))
    timed("decompress_each/index_free (%d streams)" % len(blobs), lambda: mhc.decompress_each(tables, blobs))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
