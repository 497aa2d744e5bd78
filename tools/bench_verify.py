#!/usr/bin/env python3
"""Scrub of the device index against the resident WALs on the MI355X (bcw_index_verify_async).

The database of tools/bench_get.py: four resident WALs of the config-B record shape (ns 20, key 100, value 4096; the
product writer, one seed each) and an index over them, every entry intact. Per repetition, interleaved, in one process,
HIP events on the codec stream around the calls:
  (a) bcw_index_verify_async with verify = 1: every entry read, CRC-checked, parsed and its key compared, in HBM
  (b) the only route without it: bcw_index_export of every key to the host (b_export), then bcw_get_records_async of
      all of them with verify = 1 into a payload buffer as large as the live data (b_get). The two halves are timed
      separately: the export is synchronous host work (host clock), the get is device-resident (events; the upload of
      the exported keys is untimed). The route cannot see an entry that points at another key's intact record.
In a pass of its own, the kernel split of (a) and of (b)'s get. --warmup calls first, then --reps; median [min, max].
One JSON line on stdout.

  python tools/bench_verify.py [--wal-mib 1024] [--reps 7] [--warmup 2]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_verify: no HIP device")

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
    n = ix.stats().live
    kb = n * (NS + KEY)
    u8 = lambda m: torch.zeros(max(m, 1), dtype=torch.uint8, device="cuda")  # noqa: E731

    # (a): room for a few bad entries (there are none)
    d_bad, d_bkeys, d_rows = u8(64 * 48), u8(64 * 256), u8(8 * 32)
    d_vres = u8(C.sizeof(L.VerifyResult))
    vout = L.VerifyOut(d_bad.data_ptr(), 64, d_bkeys.data_ptr(), 64 * 256, d_rows.data_ptr(), 8, 0)
    vp = L.GetParams(NS, ETAG, 1, 0)

    def a_verify():
        rc = L.lib.bcw_index_verify_async(ix.handle, ws.handle, C.byref(vp), C.byref(vout), ptr(d_vres))
        assert rc == 0, rc

    # (b): the export's host arrays, and the get's device arrays with a payload buffer for every record
    h_keys = np.zeros(kb, dtype=np.uint8)
    h_koff = np.zeros(n + 1, dtype=np.uint64)
    h_fid, h_off, h_size = (np.zeros(n, dtype=np.uint64) for _ in range(3))

    def b_export():
        no, nkb = C.c_uint64(), C.c_uint64()
        rc = L.lib.bcw_index_export(ix.handle, h_keys.ctypes.data_as(C.c_void_p), kb, h_koff.ctypes.data_as(L.u64p),
                                    h_fid.ctypes.data_as(L.u64p), h_off.ctypes.data_as(L.u64p),
                                    h_size.ctypes.data_as(L.u64p), n, C.byref(no), C.byref(nkb))
        assert rc == 0 and no.value == n and nkb.value == kb, (rc, no.value, nkb.value)

    b_export()
    d_keys, d_koff = dev(h_keys), dev(h_koff)
    col = {k: u8(n * w) for k, w in (("get_status", 1), ("rd_status", 1), ("fid", 8), ("off", 8), ("size", 8),
                                     ("pay_off", 8))}
    d_gres = u8(C.sizeof(L.GetResult))
    need = int(((h_size + np.uint64(15)) & ~np.uint64(15)).sum())
    d_pay = u8(need)
    gout = L.GetOut(ptr(col["get_status"], L.u8p), ptr(col["rd_status"], L.u8p), ptr(col["fid"], L.u64p),
                    ptr(col["off"], L.u64p), ptr(col["size"], L.u64p), ptr(col["pay_off"], L.u64p),
                    ptr(d_pay, L.u8p), need, L.RecordTable())

    def b_get():
        rc = L.lib.bcw_get_records_async(ix.handle, ws.handle, C.byref(vp), n, ptr(d_keys), ptr(d_koff), C.byref(gout),
                                         ptr(d_gres))
        assert rc == 0, rc

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    # both routes find the database whole (checked once, before anything is timed)
    a_verify()
    b_get()
    stream.synchronize()
    vres = L.VerifyResult.from_buffer_copy(d_vres.cpu().numpy().tobytes())
    gres = L.GetResult.from_buffer_copy(d_gres.cpu().numpy().tobytes())
    assert (vres.n_checked, vres.by_class[L.VFY_OK], vres.n_bad, vres.fits) == (n, n, 0, 1), (vres.n_checked, vres.n_bad)
    assert (gres.n_ok, gres.fits, gres.payload_need) == (n, 1, need), (gres.n_ok, gres.fits)

    ta, tg, tx = [], [], []
    for rep in range(args.warmup + args.reps):  # interleaved
        a = timed(a_verify)[0]
        x = timed(b_export)[1]
        g = timed(b_get)[0]
        if rep >= args.warmup:
            ta.append(a)
            tx.append(x)
            tg.append(g)

    # the kernels of (a) and of (b)'s get, in a pass of its own (events around each kernel)
    nk = int(L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, 0))
    names = [L.lib.bcw_kernel_name(k).decode() for k in range(nk)]
    split = {}
    for name, fn in (("a_verify", a_verify), ("b_get", b_get)):
        L.lib.bcw_ctx_set_profiling(ctx.handle, -1)
        L.lib.bcw_ctx_kernel_times(ctx.handle, None, None, nk)
        for _ in range(args.reps):
            fn()
        tot, cnt = (C.c_double * nk)(), (C.c_uint64 * nk)()
        L.lib.bcw_ctx_kernel_times(ctx.handle, tot, cnt, nk)
        L.lib.bcw_ctx_set_profiling(ctx.handle, 0)
        split[name] = {names[k]: round(tot[k] / cnt[k], 4) for k in range(nk) if cnt[k]}

    wal_bytes = sum(img_len.values())
    ma = statistics.median(ta)
    out = {"bench": "verify", "keys": n, "slots": ix.stats().slot_capacity, "wals": len(fids), "wal_bytes": wal_bytes,
           "record_shape": {"ns": NS, "key": KEY, "value": VAL}, "payload_bytes_of_b": need,
           "a_verify_event_ms": stats(ta), "b_export_host_ms": stats(tx), "b_get_event_ms": stats(tg),
           "kernel_ms": split, "a_min_below_b_get_min": min(ta) < min(tg),
           "a_over_b_get": round(ma / statistics.median(tg), 3),
           "a_over_b": round(ma / (statistics.median(tg) + statistics.median(tx)), 3),
           "a_wal_gbs": round(wal_bytes / (ma * 1e-3) / 1e9, 1)}
    print(json.dumps(out))
    ws.close()
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
