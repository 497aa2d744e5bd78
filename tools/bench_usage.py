#!/usr/bin/env python3
"""Per-WAL space accounting on the MI355X (bcw_index_fid_usage_async, bcw_freed_by_fid_async).

Index: the reclaim measurement's shape, 2^22 slots at load 0.7 (2,936,012 keys of 28 bytes), the values spread over
--fids distinct fids (default: 4 and 1024, one index each). Per repetition, interleaved, in one process:
  (a) bcw_index_fid_usage_async, HIP events on the codec stream around the call
  (b) what the library offered before it: bcw_index_export of every entry to the host plus the host's grouped sum
      (numpy: count and bytes per fid; the span is left out, in (b)'s favour), host clock around both
  (c) the floor, a plain pass over the same table: k_ix_live_bytes (bcw_index_compact(shrink) runs it first), its
      kernel time from bcw_ctx_set_profiling
and, in a pass of its own, the kernel split of (a). (a)'s rows are checked against (b)'s sums.

Write: the batch of tools/bench_put.py (--records records, ns 20, key 100, value 4096, device-resident inputs) into an
index that already holds its keys, timed on the host clock from the call to the finished writeStats dict: with the
two WriteStat columns downloaded and summed on the host (write_batch's default), and with bcw_freed_by_fid_async
(stats_on_device). --warmup calls first, then --reps; median [min, max]. One JSON line on stdout.

  python tools/bench_usage.py [--keys 2936012] [--fids 4,1024] [--records 1000000] [--reps 7] [--warmup 2]
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
from bitcaskdb_amd.usage import freed_by_fid  # noqa: E402

BASE_TIME = 1_700_000_000
NS, KEY, VAL, ETAG = 20, 100, 4096, 20
ROW = C.sizeof(L.FidUsageRow)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def u64p(a):
    return a.ctypes.data_as(L.u64p)


def fill_index(ix: Index, n: int, nfids: int):
    """n keys ns(20) || counter(8), value (1 + i % nfids, 40 + 128 i, 100 + i % 4000), applied in chunks"""
    chunk = 1 << 19
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        i = np.arange(a, a + m, dtype=np.uint64)
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


def bench_index(ctx, stream, n: int, nfids: int, reps: int, warmup: int) -> dict:
    ix = Index(ctx, keys=n, arena_bytes=48 * n + (1 << 20))
    fill_index(ix, n, nfids)
    st = ix.stats()
    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    cap = max(nfids, 1)
    d_rows = torch.zeros(cap * ROW, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(C.sizeof(L.UsageResult), dtype=torch.uint8, device="cuda")
    # (b)'s host arrays, allocated once
    h_keys = np.zeros((NS + 8) * n, dtype=np.uint8)
    h_koff = np.zeros(n + 1, dtype=np.uint64)
    h_fid, h_off, h_size = (np.zeros(n, dtype=np.uint64) for _ in range(3))

    def usage_call():
        rc = L.lib.bcw_index_fid_usage_async(ix.handle, C.c_void_p(d_rows.data_ptr()), cap,
                                             C.c_void_p(d_res.data_ptr()))
        assert rc == 0, rc

    def a_event() -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        usage_call()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def b_export_sum():
        t0 = time.perf_counter()
        no, kb = C.c_uint64(), C.c_uint64()
        rc = L.lib.bcw_index_export(ix.handle, h_keys.ctypes.data_as(C.c_void_p), h_keys.size, u64p(h_koff),
                                    u64p(h_fid), u64p(h_off), u64p(h_size), n, C.byref(no), C.byref(kb))
        assert rc == 0 and no.value == n, (rc, no.value)
        fids, inv = np.unique(h_fid, return_inverse=True)
        count = np.bincount(inv, minlength=fids.size)
        nbytes = np.bincount(inv, weights=h_size.astype(np.float64), minlength=fids.size)  # exact below 2^53
        return (time.perf_counter() - t0) * 1e3, dict(zip(fids.tolist(), zip(count.tolist(),
                                                                            nbytes.astype(np.uint64).tolist())))

    def c_floor() -> float:
        kid = names.index("k_ix_live_bytes")
        L.lib.bcw_ctx_set_profiling(ctx.handle, 1 << kid)
        L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
        ix.compact(shrink=True)  # nothing is dead: the same table again
        tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
        L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
        L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
        assert cnt[kid] == 1
        return tot[kid]

    ta, tb, tc = [], [], []
    sums = None
    for rep in range(warmup + reps):
        a = a_event()
        b, sums = b_export_sum()
        c = c_floor()
        if rep >= warmup:
            ta.append(a)
            tb.append(b)
            tc.append(c)
    assert ix.stats().slot_capacity == st.slot_capacity
    # (a)'s rows against (b)'s sums
    usage_call()
    stream.synchronize()
    res = L.UsageResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    rows = d_rows.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert res.fits == 1 and res.overflow == 0 and res.n_fids == nfids == len(sums), (res.fits, res.n_fids)
    assert {int(r[0]): (int(r[1]), int(r[2])) for r in rows[:nfids]} == sums
    # the kernel split of (a), in a pass of its own
    L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
    L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
    for _ in range(reps):
        usage_call()
    tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
    L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
    L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
    split = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk) if cnt[k]}
    ma, mb, mc = (statistics.median(x) for x in (ta, tb, tc))
    table_bytes = st.slot_capacity * 64
    out = {"fids": nfids, "keys": n, "slots": st.slot_capacity, "table_bytes": table_bytes,
           "a_fid_usage_event_ms": stats(ta), "b_export_host_sum_ms": stats(tb), "c_live_bytes_kernel_ms": stats(tc),
           "a_kernel_ms": split, "a_over_b": round(ma / mb, 5), "a_over_c": round(ma / mc, 3),
           "a_table_gbs": round(table_bytes / (ma * 1e-3) / 1e9, 1)}
    ix.close()
    return out


def bench_write(ctx, stream, n: int, reps: int, warmup: int) -> dict:
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
    ba = L.WriteBatchArrays(n, d_keys.data_ptr(), d_koff.data_ptr(), keys_len, d_vals.data_ptr(), d_voff.data_ptr(),
                            vals_len, None, d_moff.data_ptr(), 0, None, d_exp.data_ptr(), d_flags.data_ptr())
    out = L.WriteOut(d_wal.data_ptr(), cap, d_off.data_ptr(), d_size.data_ptr(), d_found.data_ptr(),
                     d_ffid.data_ptr(), d_fbytes.data_ptr())

    def write(fid: int):
        p = L.WriteParams(fid, BASE_TIME, 40, NS, ETAG)
        rc = L.lib.bcw_write_records_async(ix.handle, C.byref(p), C.byref(ba), C.byref(out),
                                           C.c_void_p(d_res.data_ptr()))
        assert rc == 0, rc

    def host_stats(fid: int):  # write_batch's default: the two columns over the bus, a loop over n Python ints
        stream.synchronize()
        t0 = time.perf_counter()
        write(fid)
        stream.synchronize()
        ffid = d_ffid.cpu().numpy().view(np.uint64)
        fbytes = d_fbytes.cpu().numpy().view(np.uint64)
        st: dict = {}
        for f, b in zip(ffid.tolist(), fbytes.tolist()):
            st[f] = st.get(f, 0) + b
        return (time.perf_counter() - t0) * 1e3, st

    def device_stats(fid: int):  # stats_on_device: the grouped rows only
        stream.synchronize()
        t0 = time.perf_counter()
        write(fid)
        st = freed_by_fid(ix, n, d_found.data_ptr(), d_ffid.data_ptr(), d_fbytes.data_ptr(), d_res.data_ptr())
        return (time.perf_counter() - t0) * 1e3, st

    th, td = [], []
    fid = 1
    for rep in range(warmup + reps):  # every call replaces the previous call's n values (a new fid each time)
        h, sh = host_stats(fid)
        d, sd = device_stats(fid + 1)
        # the first call of all finds nothing ({0: 0}); every later one frees the previous call's values
        assert list(sd) == [fid] and (rep == 0 or sh == {fid - 1: sd[fid]}), (sh, sd)
        fid += 2
        if rep >= warmup:
            th.append(h)
            td.append(d)
    r = L.WriteResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert r.fits == 1 and r.err_class == 0 and r.n_written == n
    mh, md = statistics.median(th), statistics.median(td)
    res = {"records": n, "host_stats_ms": stats(th), "device_stats_ms": stats(td),
           "device_over_host": round(md / mh, 4)}
    ix.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_936_012)
    ap.add_argument("--fids", default="4,1024")
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_usage: no HIP device")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    res = {"bench": "usage",
           "index": [bench_index(ctx, stream, args.keys, int(f), args.reps, args.warmup)
                     for f in args.fids.split(",") if f],
           "write": bench_write(ctx, stream, args.records, args.reps, args.warmup) if args.records else None}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
