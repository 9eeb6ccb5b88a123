"""Digest rate of compressed batches (include/mh.h, "DIGESTS OF BATCHES") against the decode and the search of the same batch.

In one process, after warm-up, for two batches of 65 536 x 4 KiB messages (Zipf(1.1), and the golden text
input_wiki_cpp.txt tiled), chunk 1024, HIP events, every variant run once per repetition in turn (interleaved), medians
with min and max.  The variants:
  crc_indexed, crc_index_free   mh_dev_crc_batch under a shared order-1 model, with and without the index;
  crc_each_indexed              mh_dev_crc_each (one model per stream);
  crc_o2_indexed                mh_dev_crc_batch_o2 (a shared order-2 model);
  crc_raw                       mh_dev_crc_raw_batch on the uncompressed messages.
The yardsticks, existing calls measured in the same run:
  decode_indexed                mh_dev_decode_batch into a buffer of the batch's size (`ratio` is over this one);
  find_count_1byte              count-only mh_dev_find_batch of one 1-byte pattern: the same decode with a matcher in the
                                CRC's place (`vs_find` is over this one);
  decode_then_crc_raw           what a caller does without the call: decode_indexed, then crc_raw of the buffer.
Every CRC and length is checked against zlib.crc32 before the clock.  Prints one JSON line.

    python tools/crc_rate.py [--streams 65536] [--bytes 4096] [--reps 7] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

try:
    import torch                                   # its HIP runtime first (see tests/conftest.py); events for the timing
except Exception:                                  # pragma: no cover
    torch = None
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

CHUNK = 1024
PREV0 = 0x20


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to("cuda")


def interleaved(fns, reps, warm=1):
    """name -> list of ms: every function once per repetition, in turn."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


class Batch:
    """A coded batch on the device: payload, pay_off, nbits, in_off, index, and pay_total as a host value."""

    def __init__(self, enc):
        payload, pay_off, nbits, idx, in_off = enc
        self.pay_total = int(pay_off[-1])
        self.payload = dev(np.concatenate([payload, np.zeros(64, dtype=np.uint8)]))
        self.pay_off, self.nbits, self.in_off, self.idx = dev(pay_off), dev(nbits), dev(in_off), dev(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mhc = entry.load_package()
    if torch is None or not torch.cuda.is_available() or mhc.device_count() < 1:
        raise SystemExit("crc_rate.py needs a GPU (and torch for the event timing)")
    lib = mhc.lib()
    n, per = args.streams, args.bytes
    total = n * per
    text = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "inputs", "input_wiki_cpp.txt"), "rb").read(), dtype=np.uint8)
    datasets = {"zipf1.1": zipf(total, 1), "text": np.resize(text, total).copy()}
    res = {"tool": "crc_rate", "streams": n, "stream_bytes": per, "chunk": CHUNK, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    for dname, data in datasets.items():
        raw = data.tobytes()
        msgs = [raw[i * per:(i + 1) * per] for i in range(n)]
        want_crc = np.array([zlib.crc32(m) for m in msgs], dtype=np.uint32)
        want_len = np.full(n, per, dtype=np.uint64)
        model = mhc.Model.from_counts(mhc.histogram_o1_batch(msgs), 1)
        shared = Batch(model.encode_batch(msgs, chunk_symbols=CHUNK))
        ms_set = mhc.ModelSet.train(msgs, order=1)
        e_payload, e_pay_off, e_nbits, e_idx, e_in_off, rc = ms_set.encode(msgs, chunk_symbols=CHUNK)
        assert rc == mhc.MH_OK
        each = Batch((e_payload, e_pay_off, e_nbits, e_idx, e_in_off))
        model2 = mhc.Model.from_counts(mhc.histogram_o2_batch(msgs), 2)
        second = Batch(model2.encode_batch_o2(msgs, chunk_symbols=CHUNK))
        ps = mhc.PatternSet([raw[5:6]])
        d_data = dev(data)
        cws = lib.mh_dev_crc_batch_workspace(n, total, CHUNK)
        wsb = max(cws, lib.mh_dev_find_batch_workspace(n, total, CHUNK), lib.mh_dev_decode_batch_workspace(n),
                  lib.mh_dev_crc_raw_batch_workspace(n, total))
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d_all = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_so = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_ho = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_crc = torch.empty(n, dtype=torch.int32, device="cuda")
        d_len = torch.empty(n, dtype=torch.int64, device="cuda")
        d_st = torch.empty(n, dtype=torch.int32, device="cuda")

        def decode():
            d_so.copy_(shared.in_off)
            mhc._check(lib.mh_dev_decode_batch(model.handle, ptr(shared.payload), ptr(shared.pay_off), ptr(shared.nbits), n, shared.pay_total, PREV0,
                                               ptr(d_all), total, ptr(d_so), total, ptr(shared.idx), CHUNK, None, ptr(d_ws), wsb, None), "decode")

        def find():
            mhc._check(lib.mh_dev_find_batch(model.handle, ps.handle, ptr(shared.payload), ptr(shared.pay_off), ptr(shared.nbits), n, shared.pay_total,
                                             PREV0, ptr(shared.in_off), total, ptr(shared.idx), CHUNK, ptr(d_ho), None, None, 0, None, ptr(d_ws), wsb,
                                             None), "find")

        def crc(fn, handle, b, indexed=True):
            mhc._check(fn(handle, ptr(b.payload), ptr(b.pay_off), ptr(b.nbits), n, b.pay_total, PREV0, ptr(b.in_off) if indexed else None, total,
                          ptr(b.idx) if indexed else None, CHUNK if indexed else 0, ptr(d_crc), ptr(d_len), ptr(d_st), ptr(d_ws), wsb, None), "crc")

        def crc_raw(src):
            mhc._check(lib.mh_dev_crc_raw_batch(ptr(src), ptr(shared.in_off), n, total, ptr(d_crc), ptr(d_ws), wsb, None), "crc_raw")

        def decode_then_crc_raw():
            decode()
            crc_raw(d_all)

        fns = {
            "decode_indexed": decode,
            "find_count_1byte": find,
            "crc_indexed": lambda: crc(lib.mh_dev_crc_batch, model.handle, shared),
            "crc_index_free": lambda: crc(lib.mh_dev_crc_batch, model.handle, shared, indexed=False),
            "crc_each_indexed": lambda: crc(lib.mh_dev_crc_each, ms_set.handle, each),
            "crc_o2_indexed": lambda: crc(lib.mh_dev_crc_batch_o2, model2.handle, second),
            "crc_raw": lambda: crc_raw(d_data),
            "decode_then_crc_raw": decode_then_crc_raw,
        }
        for k, fn in fns.items():                                        # every variant's result against zlib, before the clock
            d_crc.fill_(0x5A5A5A5A); d_len.fill_(-1); d_st.fill_(-1); d_ho.fill_(-1)
            fn()
            assert lib.mh_dev_status(ptr(d_ws), None) == 0, (dname, k)
            if k == "decode_indexed":
                assert torch.equal(d_all, d_data), (dname, k)
            elif k == "find_count_1byte":
                ho = d_ho.cpu().numpy().view(np.uint64)
                assert int(ho[n]) == raw.count(raw[5:6]), (dname, k)
            else:
                assert np.array_equal(d_crc.cpu().numpy().view(np.uint32), want_crc), (dname, k)
                if "raw" not in k:
                    assert np.array_equal(d_len.cpu().numpy().view(np.uint64), want_len) and not d_st.cpu().numpy().any(), (dname, k)
        ms = interleaved(fns, args.reps)
        out = {k: stats(v) for k, v in ms.items()}
        base, fnd = out["decode_indexed"]["median_ms"], out["find_count_1byte"]["median_ms"]
        for k in out:
            out[k]["ratio"] = round(out[k]["median_ms"] / base, 3)
            out[k]["vs_find"] = round(out[k]["median_ms"] / fnd, 3)
        out["payload_bytes"] = shared.pay_total
        out["workspace_bytes"] = int(cws)
        out["decoded_buffer_bytes"] = total
        res[dname] = out
        del shared, each, second, d_data, d_all, d_ws
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
