#!/usr/bin/env python3
"""Batched Get by key on the MI355X: the fused path (bcw_get_records_async: keys -> index -> record bytes in HBM)
against the composed path a caller had before it (bcw_index_get, host grouping by fid, one bcw_read_records_async
per resident image), interleaved in one process.

Four resident WALs of the config-B record shape (ns 20, key 100, value 4096; the product writer, one seed each) and
an index over them; a get of --gets uniformly drawn keys, device-resident, with verify off and on. Every call is
timed with HIP events on the codec stream (the composed path, which has host work between its launches, also with a
host clock around its final synchronise); --warmup calls first, then --reps repetitions per variant, round-robin.
Reported: median, min and max per variant, the fused path's payload rate (payload_need bytes over the call time, as
a fraction of the HBM peak; the call also reads the same bytes out of the WAL images), and the fused path's
per-kernel split from bcw_ctx_set_profiling in a pass of its own. One JSON line on stdout.

  python tools/bench_get.py [--wal-mib 1024] [--gets 1000000] [--reps 7] [--warmup 2]
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

from bitcaskdb_amd import Context, Index, WalSet  # noqa: E402
from bitcaskdb_amd import _lib as L  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
BASE_TIME = 1_700_000_000
NS, KEY, VAL, ETAG = 20, 100, 4096, 20


def synth(seg_bytes: int, seed: int) -> np.ndarray:
    n, r = C.c_uint64(), C.c_uint64()
    assert L.lib.bcw_synth_segment(seg_bytes, 0, seed, NS, KEY, VAL, 0, BASE_TIME, None, 0, C.byref(n),
                                   C.byref(r)) == 0
    buf = np.zeros(n.value, dtype=np.uint8)
    assert L.lib.bcw_synth_segment(seg_bytes, 0, seed, NS, KEY, VAL, 0, BASE_TIME, C.c_void_p(buf.ctypes.data),
                                   buf.size, C.byref(n), C.byref(r)) == 0
    return buf


def export_keys(ix: Index):
    """every live merged key as rows of a (n, NS + KEY) array (all keys have one length here)"""
    n, kb = C.c_uint64(), C.c_uint64()
    rc = L.lib.bcw_index_export_fids(ix.handle, None, 0, None, 0, None, None, None, None, 0, C.byref(n), C.byref(kb))
    assert rc in (0, L.E_CAPACITY)
    cap, kcap = int(n.value), int(kb.value)
    assert kcap == cap * (NS + KEY)
    keys = np.zeros(kcap, dtype=np.uint8)
    koff = np.zeros(cap + 1, dtype=np.uint64)
    fid, off, size = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    rc = L.lib.bcw_index_export_fids(ix.handle, None, 0, keys.ctypes.data_as(C.c_void_p), kcap,
                                     koff.ctypes.data_as(L.u64p), fid.ctypes.data_as(L.u64p),
                                     off.ctypes.data_as(L.u64p), size.ctypes.data_as(L.u64p), cap, C.byref(n),
                                     C.byref(kb))
    assert rc == 0
    return keys.reshape(cap, NS + KEY)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def ptr(t: torch.Tensor, ty=None):
    p = C.c_void_p(t.data_ptr())
    return C.cast(p, ty) if ty is not None else p


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wal-mib", type=int, default=1024, help="size of each of the four WALs")
    ap.add_argument("--gets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_get: no HIP device")

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    fids = (1, 2, 3, 4)
    ix, ws = Index(ctx, keys=1 << 16), WalSet(ctx)
    d_img, img_len = {}, {}
    for fid in fids:
        seg = synth(args.wal_mib << 20, 100 + fid)
        dres, ires = ix.recover_segment(seg, L.MODE_RECORD, fid, 40, BASE_TIME, NS, ETAG)
        assert dres.err_class == 0 and ires.err_class == 0 and ires.n_in == dres.n_records
        d_img[fid], img_len[fid] = dev(seg), int(seg.size)
        ws.put_device(fid, d_img[fid].data_ptr(), img_len[fid], BASE_TIME)
        del seg
    allkeys = export_keys(ix)
    n_keys, n = int(allkeys.shape[0]), args.gets
    rng = np.random.default_rng(1)
    draw = rng.integers(0, n_keys, n)
    h_keys = np.ascontiguousarray(allkeys[draw]).reshape(-1)
    h_koff = (np.arange(n + 1, dtype=np.uint64) * (NS + KEY))
    d_keys, d_koff = dev(h_keys), dev(h_koff)

    # outputs of the fused path (sized by a first call that reports payload_need)
    u8 = lambda m: torch.zeros(max(m, 1), dtype=torch.uint8, device="cuda")  # noqa: E731
    col = {k: u8(n * w) for k, w in (("get_status", 1), ("rd_status", 1), ("fid", 8), ("off", 8), ("size", 8),
                                     ("pay_off", 8))}
    tcols = {name: u8(n * int(dt[1])) for name, dt in L.TABLE_COLUMNS if name not in ("aux0", "aux1")}
    ptr_t = {"u8": L.u64p, "u4": L.u32p, "u1": L.u8p}
    table = L.RecordTable(n, *[ptr(tcols[name], ptr_t[dt]) if name in tcols else None for name, dt in L.TABLE_COLUMNS])
    d_res = u8(C.sizeof(L.GetResult))

    def fused(verify: int, d_pay, cap: int):
        out = L.GetOut(ptr(col["get_status"], L.u8p), ptr(col["rd_status"], L.u8p), ptr(col["fid"], L.u64p),
                       ptr(col["off"], L.u64p), ptr(col["size"], L.u64p), ptr(col["pay_off"], L.u64p),
                       ptr(d_pay, L.u8p) if cap else None, cap, table)
        p = L.GetParams(NS, ETAG, verify, 0)
        rc = L.lib.bcw_get_records_async(ix.handle, ws.handle, C.byref(p), n, ptr(d_keys), ptr(d_koff), C.byref(out),
                                         ptr(d_res))
        assert rc == 0, rc

    def result() -> L.GetResult:
        stream.synchronize()
        return L.GetResult.from_buffer_copy(d_res.cpu().numpy().tobytes())

    fused(0, None, 0)
    need = int(result().payload_need)
    d_pay = u8(need)
    fused(1, d_pay, need)
    r = result()
    assert r.fits == 1 and r.n_ok == n == r.n_found, (r.fits, r.n_ok, r.n_found)

    # the composed path's buffers: the index values come back to the host, are grouped by fid there, and go out again
    # as one request list per image; payload slots as the fused path lays them out (16-byte aligned), per group
    h_fid, h_off, h_size = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    h_st = np.zeros(n, dtype=np.uint8)
    d_off, d_size, d_po, d_rst = u8(8 * n), u8(8 * n), u8(8 * n), u8(n)
    d_pay2 = u8(need)

    def composed(verify: int):
        rc = L.lib.bcw_index_get(ix.handle, n, h_keys.ctypes.data_as(C.c_void_p), h_koff.ctypes.data_as(L.u64p),
                                 h_fid.ctypes.data_as(L.u64p), h_off.ctypes.data_as(L.u64p),
                                 h_size.ctypes.data_as(L.u64p), h_st.ctypes.data_as(L.u8p))
        assert rc == 0
        order = np.argsort(h_fid, kind="stable")
        g_fid = h_fid[order]
        slots = (h_size[order] + np.uint64(15)) & ~np.uint64(15)
        po = np.zeros(n, dtype=np.uint64)
        np.cumsum(slots[:-1], out=po[1:])
        with torch.cuda.stream(stream):
            d_off.copy_(torch.from_numpy(h_off[order].view(np.uint8)), non_blocking=False)
            d_size.copy_(torch.from_numpy(h_size[order].view(np.uint8)), non_blocking=False)
            d_po.copy_(torch.from_numpy(po.view(np.uint8)), non_blocking=False)
        bounds = np.searchsorted(g_fid, np.array(fids + (fids[-1] + 1,), dtype=np.uint64))
        for k, fid in enumerate(fids):
            a, b = int(bounds[k]), int(bounds[k + 1])
            if a == b:
                continue
            p = L.ReadParams(img_len[fid], BASE_TIME, NS, ETAG, verify, 0)
            rc = L.lib.bcw_read_records_async(ctx.handle, ptr(d_img[fid]), C.byref(p), b - a,
                                              C.c_void_p(d_off.data_ptr() + 8 * a),
                                              C.c_void_p(d_size.data_ptr() + 8 * a),
                                              C.c_void_p(d_po.data_ptr() + 8 * a), ptr(d_pay2),
                                              C.c_void_p(d_rst.data_ptr() + a), None)
            assert rc == 0
        return order

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    # the composed path returns the same bytes (checked once, on a sample, before anything is timed)
    order = composed(1)
    stream.synchronize()
    assert int(d_rst.cpu().max()) == 0
    po_f = col["pay_off"].cpu().numpy().view(np.uint64)
    po_c = np.zeros(n, dtype=np.uint64)
    po_c[order] = d_po.cpu().numpy().view(np.uint64)
    for i in rng.integers(0, n, 64):
        z = int(h_size[i])
        a, b = int(po_f[i]), int(po_c[i])
        assert torch.equal(d_pay[a:a + z], d_pay2[b:b + z]), int(i)

    variants = {"fused_verify0": lambda: fused(0, d_pay, need), "composed_verify0": lambda: composed(0),
                "fused_verify1": lambda: fused(1, d_pay, need), "composed_verify1": lambda: composed(1)}
    ev = {k: [] for k in variants}
    host = {k: [] for k in variants}
    for rep in range(args.warmup + args.reps):
        for name, fn in variants.items():  # interleaved
            e, h = timed(fn)
            if rep >= args.warmup:
                ev[name].append(e)
                host[name].append(h)

    # the fused path's kernels, in a pass of its own (events around each kernel)
    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    split = {}
    for verify in (0, 1):
        L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
        L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
        for _ in range(args.reps):
            fused(verify, d_pay, need)
        tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
        L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
        L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
        split[f"verify{verify}"] = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk) if cnt[k]}

    out = {"bench": "get", "gets": n, "keys": n_keys, "wals": len(fids), "wal_bytes": img_len[fids[0]],
           "payload_bytes": need, "record_shape": {"ns": NS, "key": KEY, "value": VAL},
           "event_ms": {k: stats(v) for k, v in ev.items()}, "host_ms": {k: stats(v) for k, v in host.items()},
           "kernel_ms": split}
    for v in (0, 1):
        ms = statistics.median(ev[f"fused_verify{v}"])
        gbs = need / (ms * 1e-3) / 1e9
        out[f"fused_verify{v}_payload_gbs"] = round(gbs, 1)
        out[f"fused_verify{v}_payload_frac_of_hbm_peak"] = round(gbs / HBM_PEAK_GBS, 4)
        out[f"composed_over_fused_verify{v}"] = round(statistics.median(host[f"composed_verify{v}"]) /
                                                       statistics.median(host[f"fused_verify{v}"]), 2)
    print(json.dumps(out))
    ws.close()
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
