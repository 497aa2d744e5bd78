#!/usr/bin/env python3
"""Retiring WAL files from the device index on the MI355X (bcw_index_drop_fids_async).

The table of tools/bench_usage.py: 2^22 slots at load 0.7 (2,936,012 keys of 28 bytes), the values spread over --fids
distinct fids (default: 4 and 1024, one index each). Every timed call works on the full table, all keys live, and
concerns one quarter of the fids. Per repetition, interleaved, in one process, HIP events on the codec stream around
the calls:
  (a) bcw_index_drop_fids_async(BCW_DROP_IN) of those fids
  (b) the only route without it: bcw_index_export_fids of those fids to the host plus bcw_index_apply of
      BCW_IDX_DELETE ops for the exported keys. The table is full, so the Delete batch does not fit the host's slot
      bound and the apply grows the table first (b_grew_table); the two halves are also timed on the host clock
  (c) bcw_index_fid_usage_async on the same table: the read-only pass that streams the same bytes
After (a) and after (b) the dropped keys are put back and the table is rebuilt at 2^22 slots, untimed. In a pass of
its own, the kernel split of (a). --warmup calls first, then --reps; median [min, max]. One JSON line on stdout.

  python tools/bench_drop.py [--keys 2936012] [--fids 4,1024] [--reps 7] [--warmup 2]
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
import torch  # noqa: E402

from bitcaskdb_amd import Context, Index  # noqa: E402
from bitcaskdb_amd import _lib as L  # noqa: E402

NS = 20
ROW = C.sizeof(L.FidUsageRow)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def u64p(a):
    return a.ctypes.data_as(L.u64p)


def put_keys(ix: Index, idx: np.ndarray, nfids: int):
    """Put of the keys ns(20) || counter(8) for the counters in idx, value (1 + i % nfids, 40 + 128 i, 100 + i % 4000),
    in chunks (bench_usage.py's fill)"""
    chunk = 1 << 19
    for a in range(0, idx.size, chunk):
        i = np.ascontiguousarray(idx[a:a + chunk], dtype=np.uint64)
        m = int(i.size)
        keys = np.zeros((m, NS + 8), dtype=np.uint8)
        keys[:, :NS] = 0x41
        keys[:, NS:] = i.view(np.uint8).reshape(m, 8)
        koff = np.arange(m + 1, dtype=np.uint64) * (NS + 8)
        ops = np.zeros(m, dtype=np.uint8)
        one = np.uint64(1)
        fid, off, size = one + i % np.uint64(nfids), np.uint64(40) + np.uint64(128) * i, \
            np.uint64(100) + i % np.uint64(4000)
        rc = L.lib.bcw_index_apply(ix.handle, m, keys.ctypes.data_as(C.c_void_p), u64p(koff),
                                   ops.ctypes.data_as(L.u8p), u64p(fid), u64p(off), u64p(size))
        assert rc == 0, rc


def bench(ctx, stream, n: int, nfids: int, reps: int, warmup: int) -> dict:
    ix = Index(ctx, keys=n, arena_bytes=48 * n + (1 << 20))
    every = np.arange(n, dtype=np.uint64)
    put_keys(ix, every, nfids)
    st0 = ix.stats()
    nq = max(nfids // 4, 1)
    listed = np.arange(1, nq + 1, dtype=np.uint64)  # fid = 1 + i % nfids
    dropped = every[every % np.uint64(nfids) < np.uint64(nq)]
    nd = int(dropped.size)
    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    cap = nfids
    d_rows = torch.zeros(cap * ROW, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(C.sizeof(L.UsageResult), dtype=torch.uint8, device="cuda")
    # (b)'s host arrays, allocated once
    h_keys = np.zeros((NS + 8) * nd, dtype=np.uint8)
    h_koff = np.zeros(nd + 1, dtype=np.uint64)
    h_fid, h_off, h_size = (np.zeros(nd, dtype=np.uint64) for _ in range(3))
    h_del = np.full(nd, L.IDX_DELETE, dtype=np.uint8)

    def restore():
        """the dropped keys back, the table rebuilt at its first capacity, every key live"""
        put_keys(ix, dropped, nfids)
        ix.compact(shrink=True)
        s = ix.stats()
        assert (s.live, s.slots_used, s.slot_capacity) == (n, n, st0.slot_capacity), s

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def a_drop():
        rc = L.lib.bcw_index_drop_fids_async(ix.handle, L.DROP_IN, u64p(listed), nq, C.c_void_p(d_rows.data_ptr()), cap,
                                             C.c_void_p(d_res.data_ptr()))
        assert rc == 0, rc

    split_b = []

    def b_export_delete():
        t0 = time.perf_counter()
        no, kb = C.c_uint64(), C.c_uint64()
        rc = L.lib.bcw_index_export_fids(ix.handle, u64p(listed), nq, h_keys.ctypes.data_as(C.c_void_p), h_keys.size,
                                         u64p(h_koff), u64p(h_fid), u64p(h_off), u64p(h_size), nd, C.byref(no),
                                         C.byref(kb))
        assert rc == 0 and no.value == nd, (rc, no.value)
        t1 = time.perf_counter()
        rc = L.lib.bcw_index_apply(ix.handle, nd, h_keys.ctypes.data_as(C.c_void_p), u64p(h_koff),
                                   h_del.ctypes.data_as(L.u8p), u64p(h_fid), u64p(h_off), u64p(h_size))
        assert rc == 0, rc
        split_b.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))

    def c_usage():
        rc = L.lib.bcw_index_fid_usage_async(ix.handle, C.c_void_p(d_rows.data_ptr()), cap,
                                             C.c_void_p(d_res.data_ptr()))
        assert rc == 0, rc

    def result():
        return L.UsageResult.from_buffer_copy(d_res.cpu().numpy().tobytes())

    ta, tb, tc = [], [], []
    grew = False
    for rep in range(warmup + reps):
        a = timed(a_drop)
        res = result()
        assert (res.fits, res.overflow, res.n_fids, res.count) == (1, 0, nq, nd), (res.n_fids, res.count)
        assert ix.stats().live == n - nd
        restore()
        c = timed(c_usage)
        assert result().count == n
        b = timed(b_export_delete)
        s = ix.stats()
        assert s.live == n - nd
        grew = grew or s.slot_capacity > st0.slot_capacity
        restore()
        if rep >= warmup:
            ta.append(a)
            tb.append(b)
            tc.append(c)
    # the kernel split of (a), in a pass of its own
    L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
    for _ in range(3):
        L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
        a_drop()
        stream.synchronize()
        L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
        restore()
    tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
    L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
    split = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk)
             if cnt[k] and names[k] in ("k_ix_drop", "k_usage_final")}
    ma, mb, mc = (statistics.median(x) for x in (ta, tb, tc))
    table_bytes = st0.slot_capacity * 64
    out = {"fids": nfids, "listed_fids": nq, "keys": n, "dropped_keys": nd, "slots": st0.slot_capacity,
           "table_bytes": table_bytes, "a_drop_event_ms": stats(ta), "b_export_delete_event_ms": stats(tb),
           "b_export_host_ms": stats([x[0] for x in split_b[warmup:]]),
           "b_delete_apply_host_ms": stats([x[1] for x in split_b[warmup:]]), "b_grew_table": grew,
           "c_fid_usage_event_ms": stats(tc), "a_kernel_ms": split, "a_over_b": round(ma / mb, 5),
           "a_over_c": round(ma / mc, 3), "a_table_gbs": round(table_bytes / (ma * 1e-3) / 1e9, 1)}
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_936_012)
    ap.add_argument("--fids", default="4,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_drop: no HIP device")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    res = {"bench": "drop",
           "index": [bench(ctx, stream, args.keys, int(f), args.reps, args.warmup) for f in args.fids.split(",") if f]}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
