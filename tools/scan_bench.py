#!/usr/bin/env python3
"""Scan of the device index by key prefix on the MI355X (bcw_index_scan_async) beside the only enumeration there was,
bcw_index_export.

An index of --keys keys in 16 namespaces of 20 bytes (user keys of 24 bytes, every value file-backed), nothing else
resident. In one process, HIP events on the codec stream around the calls, --warmup calls first, then --reps:
  scan_all   bcw_index_scan_async with n_prefix == 0 into device buffers with room for every entry and all four columns
  scan_ns    the same with one namespace as the prefix (a sixteenth of the keys)
  export     bcw_index_export of every entry into host arrays: synchronous, so a host clock around the call
and, in a pass of its own, the kernel split of the two scans (events around each kernel). The bytes a scan must move
are the slot table once, a verdict byte per slot written and read, and the listed keys (read from the arena, written
packed), their offsets and columns; the share of HBM bandwidth is those bytes over the median time. One JSON line on
stdout.

  python tools/scan_bench.py [--keys 1048576] [--reps 20] [--warmup 3]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bitcaskdb_amd import Context, Index  # noqa: E402
from bitcaskdb_amd import _lib as L  # noqa: E402

NS, KEY, NNS = 20, 24, 16
HBM_GBS = 8000.0  # MI355X peak


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--export-reps", type=int, default=5)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("scan_bench: no HIP device")

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    n = args.keys
    ix = Index(ctx, keys=n, arena_bytes=n * 64)
    rng = np.random.default_rng(11)
    nss = rng.integers(0, 256, size=(NNS, NS), dtype=np.uint8)
    step = 1 << 16
    for a in range(0, n, step):  # key i: namespace i % 16, then 24 bytes that hold i
        m = min(step, n - a)
        idx = np.arange(a, a + m, dtype=np.uint64)
        keys = np.zeros((m, NS + KEY), dtype=np.uint8)
        keys[:, :NS] = nss[(idx % NNS).astype(np.int64)]
        keys[:, NS:NS + 8] = idx.view(np.uint8).reshape(m, 8)
        keys[:, NS + 8:] = rng.integers(0, 256, size=(m, KEY - 8), dtype=np.uint8)
        koff = np.arange(m + 1, dtype=np.uint64) * (NS + KEY)
        ops = np.zeros(m, dtype=np.uint8)
        fid, off, size = idx % 7 + 1, 40 + idx * 4200, np.full(m, 4200, dtype=np.uint64)
        rc = L.lib.bcw_index_apply(ix.handle, m, keys.ctypes.data_as(C.c_void_p), koff.ctypes.data_as(L.u64p),
                                   ops.ctypes.data_as(L.u8p), fid.ctypes.data_as(L.u64p), off.ctypes.data_as(L.u64p),
                                   size.ctypes.data_as(L.u64p))
        assert rc == 0, rc
    st = ix.stats()
    assert st.live == n, (st.live, n)
    kb = n * (NS + KEY)

    u8 = lambda m: torch.zeros(max(m, 1), dtype=torch.uint8, device="cuda")  # noqa: E731
    d = {"keys": u8(kb + 16), "key_off": u8(8 * (n + 1)), "fid": u8(8 * n), "off": u8(8 * n), "size": u8(8 * n),
         "prefix_id": u8(n), "groups": u8(32), "res": u8(C.sizeof(L.ScanResult))}
    out = L.ScanOut(d["keys"].data_ptr(), kb, d["key_off"].data_ptr(), d["fid"].data_ptr(), d["off"].data_ptr(),
                    d["size"].data_ptr(), d["prefix_id"].data_ptr(), n, d["groups"].data_ptr())
    p_all = L.ScanParams(0, 0, None, None)
    pfx = np.ascontiguousarray(nss[3])
    poff = np.array([0, NS], dtype=np.uint32)
    p_ns = L.ScanParams(0, 1, pfx.ctypes.data, poff.ctypes.data)

    def scan(p):
        rc = L.lib.bcw_index_scan_async(ix.handle, C.byref(p), C.byref(out), C.c_void_p(d["res"].data_ptr()))
        assert rc == 0, rc

    def result():
        stream.synchronize()
        return L.ScanResult.from_buffer_copy(d["res"].cpu().numpy().tobytes())

    h_keys = np.zeros(kb, dtype=np.uint8)
    h_koff = np.zeros(n + 1, dtype=np.uint64)
    h_fid, h_off, h_size = (np.zeros(n, dtype=np.uint64) for _ in range(3))

    def export():
        no, nkb = C.c_uint64(), C.c_uint64()
        rc = L.lib.bcw_index_export(ix.handle, h_keys.ctypes.data_as(C.c_void_p), kb, h_koff.ctypes.data_as(L.u64p),
                                    h_fid.ctypes.data_as(L.u64p), h_off.ctypes.data_as(L.u64p),
                                    h_size.ctypes.data_as(L.u64p), n, C.byref(no), C.byref(nkb))
        assert rc == 0 and no.value == n and nkb.value == kb, (rc, no.value, nkb.value)

    # the two routes list the same entries (checked once, before anything is timed)
    scan(p_all)
    r_all = result()
    assert (r_all.n_listed, r_all.key_bytes, r_all.n_live, r_all.fits) == (n, kb, n, 1), (r_all.n_listed, r_all.fits)
    s_keys = d["keys"].cpu().numpy()[:kb].reshape(n, NS + KEY)
    s_fid = d["fid"].cpu().numpy().view(np.uint64)
    export()
    e_keys = h_keys.reshape(n, NS + KEY)
    so, eo = np.lexsort(s_keys.T[::-1]), np.lexsort(e_keys.T[::-1])
    assert (s_keys[so] == e_keys[eo]).all() and (s_fid[so] == h_fid[eo]).all()
    scan(p_ns)
    r_ns = result()
    n_ns = len(range(3, n, NNS))
    assert (r_ns.n_listed, r_ns.key_bytes, r_ns.fits) == (n_ns, n_ns * (NS + KEY), 1), (r_ns.n_listed, n_ns)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    t_all, t_ns, t_x = [], [], []
    for rep in range(args.warmup + args.reps):  # interleaved
        a = timed(lambda: scan(p_all))[0]
        b = timed(lambda: scan(p_ns))[0]
        if rep >= args.warmup:
            t_all.append(a)
            t_ns.append(b)
    for rep in range(1 + args.export_reps):
        x = timed(export)[1]
        if rep >= 1:
            t_x.append(x)

    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    split = {}
    for name, p in (("scan_all", p_all), ("scan_ns", p_ns)):
        L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
        L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
        for _ in range(args.reps):
            scan(p)
        tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
        L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
        L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
        split[name] = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk) if cnt[k]}

    slots = st.slot_capacity

    def must_move(listed, key_bytes):  # slot table, verdict bytes out and in, tile columns, keys in and out, columns
        entry = 16 + ((NS + KEY + 15) & ~15)
        return 64 * slots + 2 * slots + 4 * 8 * (slots // 256) + listed * entry + key_bytes + listed * (8 * 4 + 1 + 64)

    def share(b, ms):
        gbs = b / (ms * 1e-3) / 1e9
        return {"bytes": b, "gbs": round(gbs, 1), "hbm_share": round(gbs / HBM_GBS, 3)}

    m_all, m_ns = statistics.median(t_all), statistics.median(t_ns)
    print(json.dumps({"bench": "scan", "keys": n, "slots": slots, "namespaces": NNS, "key_bytes": NS + KEY,
                      "scan_all_event_ms": stats(t_all), "scan_ns_event_ms": stats(t_ns),
                      "export_host_ms": stats(t_x), "kernel_ms": split,
                      "scan_all_traffic": share(must_move(n, kb), m_all),
                      "scan_ns_traffic": share(must_move(n_ns, n_ns * (NS + KEY)), m_ns),
                      "scan_all_over_export": round(m_all / statistics.median(t_x), 4)}))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
