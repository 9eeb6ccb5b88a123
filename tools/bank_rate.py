"""Bank-of-shared-models rate and size (include/mh.h, "BANKS OF SHARED MODELS").

For each workload (65 536 x 4 KiB of Zipf(1.1), of tiled text, and of a mixed corpus: text, Zipf(1.1), Zipf(1.6) and a
16-letter alphabet interleaved), in one process after warm-up, wall clock around calls that end in a synchronisation:
  - mh_dev_bank_train with K entries (total, iterations run, per iteration = total / (iterations + 1 for the seed));
  - mh_dev_bank_select under the trained bank, mh_dev_model_set_pick, mh_dev_encode_each and mh_dev_decode_each (indexed and
    index-free) through the view;
  - bytes: the bank's K tables + payload, against one shared model (table + mh_encode_batch payload) and against one model
    per stream (mh_compress_each: tables + payload).
The round trips are checked against the input.  Prints one JSON line (--out: also writes it).  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/bank_rate.py` run.

    python tools/bank_rate.py [--k 8] [--reps 3] [--iters 8] [--only zipf,text,mixed] [--no-each] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

N, SIZE = 65536, 4096


def zipf(n, seed, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 257) ** s
    return rng.choice(256, size=n, p=w / w.sum()).astype(np.uint8)


def text(n):
    with open(os.path.join(ROOT, "tests", "golden", "inputs", "input_ipsum.txt"), "rb") as f:
        t = np.frombuffer(f.read(), dtype=np.uint8)
    return np.resize(t, n)


def workload(name):
    if name == "zipf":
        return zipf(N * SIZE, 1)
    if name == "text":
        return text(N * SIZE)
    parts = [text(N * SIZE // 4), zipf(N * SIZE // 4, 2), zipf(N * SIZE // 4, 3, 1.6),
             (np.random.default_rng(4).integers(0, 16, N * SIZE // 4) + ord("a")).astype(np.uint8)]
    return np.stack([p.reshape(-1, SIZE) for p in parts], axis=1).reshape(-1)      # message i from source i % 4


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


def run(mhc, name, k, reps, iters, each):
    l = mhc.lib()
    data = workload(name)
    off = np.arange(N + 1, dtype=np.uint64) * SIZE
    total = int(data.size)
    D = mhc.DeviceBuffer
    d_data, d_off = D(total, data), D(off.nbytes, off)
    d_ch, d_nb = D(N * 4), D(N * 8)
    r = {"workload": name, "streams": N, "stream_bytes": SIZE, "input_bytes": total, "k": k}

    wt = l.mh_dev_bank_train_workspace(N, total, k)
    d_wt = D(wt)
    state = {}

    def train():
        if "bank" in state:
            l.mh_model_set_free(state.pop("bank"))
        h, it = C.c_void_p(), C.c_int(0)
        assert l.mh_dev_bank_train(d_data.ptr, d_off.ptr, N, total, 1, 0x20, k, iters, d_ch.ptr, C.byref(it), d_wt.ptr, wt, None, C.byref(h)) == 0
        state["bank"], state["iters"] = h, it.value
    r["train_ms"] = wall(train, reps)
    r["train_iters"] = state["iters"]
    r["train_ms_per_iter"] = r["train_ms"] / (state["iters"] + 1)
    bank = mhc.ModelSet(state.pop("bank"))
    K = len(bank)
    r["k_trained"] = K
    ch_train = d_ch.download(np.uint32)

    ws = l.mh_dev_bank_select_workspace(K, N, total)
    d_ws = D(ws)

    def select():
        assert l.mh_dev_bank_select(bank.handle, d_data.ptr, d_off.ptr, N, total, 0x20, d_ch.ptr, d_nb.ptr, d_ws.ptr, ws, None) == 0
        assert l.mh_dev_status(d_ws.ptr, None) == 0
    r["select_ms"] = wall(select, reps)
    r["select_GBps"] = total / r["select_ms"] / 1e6
    ch, nb = d_ch.download(np.uint32), d_nb.download(np.uint64)
    assert np.array_equal(ch, ch_train)
    r["entries_used"] = int(np.unique(ch).size)

    views = []

    def pick():
        h = C.c_void_p()
        assert l.mh_dev_model_set_pick(bank.handle, d_ch.ptr, N, None, C.byref(h)) == 0
        views.append(mhc.ModelSet(h))
        if len(views) > 1:
            views.pop(0)
    r["pick_ms"] = wall(pick, reps)
    view = views[-1]

    cap = l.mh_encode_each_bound(view.handle, total, N)
    chunk = 1024
    nidx = l.mh_batch_index_capacity(total, N, chunk)
    d_pay, d_po, d_nbe, d_idx = D(cap), D((N + 1) * 8), D(N * 8), D(nidx * 8)
    we = l.mh_dev_encode_each_workspace(N, total)
    d_we = D(we)

    def encode():
        assert l.mh_dev_encode_each(view.handle, d_data.ptr, d_off.ptr, N, total, 0x20, d_pay.ptr, cap, d_po.ptr, d_nbe.ptr, d_idx.ptr, chunk,
                                    d_we.ptr, we, None) == 0
        assert l.mh_dev_status(d_we.ptr, None) == 0
    r["encode_ms"] = wall(encode, reps)
    po = d_po.download(np.uint64)
    assert np.array_equal(d_nbe.download(np.uint64), nb)
    pay_total = int(po[N])

    wd = l.mh_dev_decode_each_workspace(N)
    d_wd, d_out, d_so, d_st = D(wd), D(total), D((N + 1) * 8, off), D(N * 4)

    def decode_idx():
        assert l.mh_dev_decode_each(view.handle, d_pay.ptr, d_po.ptr, d_nbe.ptr, N, pay_total, 0x20, d_out.ptr, total, d_so.ptr, total,
                                    d_idx.ptr, chunk, d_st.ptr, d_wd.ptr, wd, None) == 0
        assert l.mh_dev_status(d_wd.ptr, None) == 0
    r["decode_indexed_ms"] = wall(decode_idx, reps)
    assert np.array_equal(d_out.download(), data)
    minl = max(view.code_lens()[1], 1)
    dcap = int(sum(int(b) // minl for b in nb))
    d_out2, d_so2 = D(dcap), D((N + 1) * 8)

    def decode_free():
        assert l.mh_dev_decode_each(view.handle, d_pay.ptr, d_po.ptr, d_nbe.ptr, N, pay_total, 0x20, d_out2.ptr, dcap, d_so2.ptr, 0,
                                    None, 0, d_st.ptr, d_wd.ptr, wd, None) == 0
        assert l.mh_dev_status(d_wd.ptr, None) == 0
    r["decode_index_free_ms"] = wall(decode_free, reps)
    assert np.array_equal(d_out2.download()[:total], data)

    tables = bank.table_bytes()
    r["bank"] = {"tables_bytes": sum(len(t) for t in tables), "payload_bytes": pay_total,
                 "total_bytes": sum(len(t) for t in tables) + pay_total + N}       # + one entry byte per stream
    msgs_off = off
    counts = np.zeros(65536, dtype=np.uint64)
    d_c = D(65536 * 8)
    wh = l.mh_dev_histogram_batch_workspace(total)
    d_wh = D(wh)
    assert l.mh_dev_histogram_o1_batch(d_data.ptr, d_off.ptr, N, total, 0x20, d_c.ptr, d_wh.ptr, wh, None) == 0
    counts = d_c.download(np.uint64)
    shared = mhc.Model.from_counts(counts, 1)
    sb = l.mh_encode_batch_bound(shared.handle, total, N)
    out = np.zeros(sb, dtype=np.uint8)
    oo, nbs = np.zeros(N + 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
    assert l.mh_encode_batch(shared.handle, data.ctypes.data, msgs_off.ctypes.data, N, 0x20, out.ctypes.data, sb, oo.ctypes.data,
                             nbs.ctypes.data, None, 0) == 0
    r["shared"] = {"tables_bytes": len(shared.table_bytes()), "payload_bytes": int(oo[N]),
                   "total_bytes": len(shared.table_bytes()) + int(oo[N])}
    if each:
        tb, pb = C.c_size_t(0), C.c_size_t(0)
        assert l.mh_compress_each_bounds(msgs_off.ctypes.data, N, C.byref(tb), C.byref(pb)) == 0
        t = np.zeros(tb.value, dtype=np.uint8)
        p = np.zeros(pb.value, dtype=np.uint8)
        to, po2, nbe = np.zeros(N + 1, dtype=np.uint64), np.zeros(N + 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        t0 = time.perf_counter()
        assert l.mh_compress_each(data.ctypes.data, msgs_off.ctypes.data, N, 1, 0x20, t.ctypes.data, tb.value, to.ctypes.data, p.ctypes.data,
                                  pb.value, po2.ctypes.data, nbe.ctypes.data, None, 0) == 0
        r["each"] = {"tables_bytes": int(to[N]), "payload_bytes": int(po2[N]), "total_bytes": int(to[N] + po2[N]),
                     "compress_each_s": time.perf_counter() - t0}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--only", default="zipf,text,mixed")
    ap.add_argument("--no-each", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    mhc = entry.load_package()
    res = {"tool": "bank_rate", "results": [run(mhc, w, a.k, a.reps, a.iters, not a.no_each) for w in a.only.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
