#!/usr/bin/env python3
"""Batched Write on the MI355X (bcw_write_records_async: field arrays -> the active WAL's bytes -> the index, in HBM).

One batch of --records records of the config-B shape (ns 20, key 100, value 4096; no etag, expire or meta), inputs
device-resident, written at file position 40 into a device buffer and applied to an index that already holds the
batch's keys after the first call (every timed call replaces 1 M values, as a steady-state writer does). Every call
is timed with HIP events on the codec stream; --warmup calls first, then --reps. Reported: the whole-call median, the
per-kernel split from bcw_ctx_set_profiling in a pass of its own, (bytes read + bytes written) / time as a fraction
of the HBM peak, and the single-core rate of the CPU oracle's record_encode + Writer.write + Index.set on the first
--cpu-records records of the same batch. One JSON line on stdout.

  python tools/bench_put.py [--records 1000000] [--reps 7] [--warmup 2] [--cpu-records 20000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from bitcaskdb_amd import Context, Index  # noqa: E402
from bitcaskdb_amd import _lib as L  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
BASE_TIME = 1_700_000_000
NS, KEY, VAL, ETAG = 20, 100, 4096, 20
FID = 1


def ptr(t: torch.Tensor):
    return t.data_ptr()


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-records", type=int, default=20000)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_put: no HIP device")
    n = args.records
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    ix = Index(ctx, keys=2 * n + 1024, arena_bytes=(16 + 128) * n + (1 << 20))

    g = torch.Generator(device="cuda").manual_seed(7)
    mk = NS + KEY
    d_keys = torch.randint(0, 256, (n * mk,), dtype=torch.uint8, device="cuda", generator=g)
    d_vals = torch.randint(0, 256, (n * VAL,), dtype=torch.uint8, device="cuda", generator=g)
    i64 = lambda a: torch.from_numpy(a.astype(np.int64)).cuda()  # noqa: E731  (offsets as bit-identical u64)
    d_koff = i64(np.arange(n + 1, dtype=np.int64) * mk)
    d_voff = i64(np.arange(n + 1, dtype=np.int64) * VAL)
    d_moff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_exp = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    keys_len, vals_len = n * mk, n * VAL
    cap = int(L.lib.bcw_write_bound(n, keys_len, vals_len, 0, ETAG, 40))
    d_wal = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off, d_size, d_ffid, d_fbytes = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(4))
    d_found = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(C.sizeof(L.WriteResult), dtype=torch.uint8, device="cuda")
    ba = L.WriteBatchArrays(n, ptr(d_keys), ptr(d_koff), keys_len, ptr(d_vals), ptr(d_voff), vals_len, None,
                            ptr(d_moff), 0, None, ptr(d_exp), ptr(d_flags))
    p = L.WriteParams(FID, BASE_TIME, 40, NS, ETAG)
    out = L.WriteOut(ptr(d_wal), cap, ptr(d_off), ptr(d_size), ptr(d_found), ptr(d_ffid), ptr(d_fbytes))

    def call():
        rc = L.lib.bcw_write_records_async(ix.handle, C.byref(p), C.byref(ba), C.byref(out), C.c_void_p(ptr(d_res)))
        assert rc == 0, rc

    def result() -> L.WriteResult:
        stream.synchronize()
        return L.WriteResult.from_buffer_copy(d_res.cpu().numpy().tobytes())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    ev = []
    for rep in range(args.warmup + args.reps):
        ms = timed(call)
        if rep >= args.warmup:
            ev.append(ms)
    r = result()
    assert r.fits == 1 and r.err_class == 0 and r.idx_err == 0 and r.n_written == n, (r.fits, r.err_class, r.n_written)
    need = int(r.wal_need)

    # per-kernel split, in a pass of its own (events around each kernel)
    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
    L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
    for _ in range(args.reps):
        call()
    tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
    L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
    L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
    split = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk) if cnt[k]}

    # the CPU oracle on the same records, one core: Record.Encode + WriteRecord + the index op
    import _oracle as O
    m = min(args.cpu_records, n)
    hk = d_keys[:m * mk].cpu().numpy().tobytes()
    hv = d_vals[:m * VAL].cpu().numpy().tobytes()
    w, oix = O.Writer(BASE_TIME, BASE_TIME, at=40), O.Index()
    t0 = time.perf_counter()
    for i in range(m):
        k = hk[i * mk:(i + 1) * mk]
        rec = O.record_encode(k[:NS], k[NS:], hv[i * VAL:(i + 1) * VAL], b"", 0, False, b"", BASE_TIME)
        off = w.write(rec)
        oix.set(k[:NS], k[NS:], 0, FID, off, len(rec))
    cpu_s = time.perf_counter() - t0
    # the first m records of the device output are the oracle's bytes
    stream.synchronize()
    assert d_wal[:w.size() - 40].cpu().numpy().tobytes() == w.data()

    med = statistics.median(ev)
    moved = keys_len + vals_len + need  # every input byte read once, every output byte written once
    gbs = moved / (med * 1e-3) / 1e9
    cpu_rps = m / cpu_s
    print(json.dumps({"bench": "put", "records": n, "record_shape": {"ns": NS, "key": KEY, "value": VAL},
                      "wal_bytes": need, "input_bytes": keys_len + vals_len, "event_ms": stats(ev),
                      "kernel_ms": split, "records_per_s": round(n / (med * 1e-3)), "moved_gbs": round(gbs, 1),
                      "moved_frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                      "cpu_oracle": {"records": m, "records_per_s": round(cpu_rps),
                                     "mb_per_s": round(cpu_rps * (mk + VAL) / 1e6, 1)},
                      "gpu_over_cpu_one_core": round(n / (med * 1e-3) / cpu_rps, 1)}))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
