#!/usr/bin/env python3
"""The device compaction filter (doFilter, bcw_compact_filter_async) on the MI355X, without and with compaction filter
rules (bcw_index_set_compact_rules), over one decoded segment of the config-B record shape (ns 20, key 100, value
4096) whose every row is live in the index.

The segment holds TTL records written through the batched Write (two namespaces, alternating; every record expires
in the future), decoded once, device-resident. Four cases, each the filter launch alone:
  a  no rules                                   the filter as it was before rules existed
  b  expired + tombstone rules, nothing matches the two column reads per kept row
  c  64 prefixes of 64 bytes, nothing matches   each a namespace of the data followed by key bytes no record has
  d  one 1-byte namespace prefix                half the live rows dropped
A window is --iters back-to-back launches between two HIP events on the codec stream (one launch is tens of
microseconds: a single one would time the event pair); --warmup windows per case first, then --reps windows per case,
round-robin over the cases. Reported per case: the median, min and max time per launch over the windows, and rows/s.
The rules are set outside the windows. Against a library without bcw_index_set_compact_rules only case a runs, so
the same script times the filter of an older build. One JSON line on stdout.

  python tools/bench_filter.py [--seg-mib 1024] [--iters 1000] [--reps 9] [--warmup 2]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bitcaskdb_amd import Context, Index  # noqa: E402
from bitcaskdb_amd import _lib as L  # noqa: E402

BASE_TIME = 1_700_000_000
NOW = BASE_TIME + 1000
NS, KEY, VAL, ETAG = 20, 100, 4096, 20
FID = 7
RULE_EXPIRED, RULE_TOMBSTONE, RULE_PREFIX = 1, 2, 4


class Rules(C.Structure):  # bcw_compact_rules (declared here: the script also runs against builds without it)
    _fields_ = [("mask", C.c_uint32), ("n_prefix", C.c_uint32), ("now", C.c_uint64), ("prefixes", C.c_void_p),
                ("prefix_off", C.c_void_p)]


def write_segment(ctx, ix, stream, n: int, dev):
    """n TTL records of the config-B shape (ns 20 -- 'A'... for even records, 'B'... for odd ones --, key 100 = the
    record index and random bytes, value 4096, expire an hour after NOW, no etag) appended to a fresh WAL image in HBM
    by the batched Write (bcw_write_records_async), which also puts every record into the index: the state a database
    is in when compaction meets the file. Returns (device image, file size)."""
    rng = np.random.default_rng(42)
    keys = rng.integers(0, 256, (n, NS + KEY), dtype=np.uint8)
    keys[:, :NS] = np.frombuffer(bytes(66 + j for j in range(NS)), dtype=np.uint8)
    keys[0::2, 0] = 65
    keys[:, NS:NS + 8] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    vals = np.frombuffer(rng.bytes(n * VAL), dtype=np.uint8)
    koff = np.arange(n + 1, dtype=np.uint64) * (NS + KEY)
    voff = np.arange(n + 1, dtype=np.uint64) * VAL
    moff = np.zeros(n + 1, dtype=np.uint64)
    expire = np.full(n, NOW + 3600, dtype=np.uint64)
    flags = np.zeros(n, dtype=np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d = [up(x) for x in (keys, koff, vals, voff, moff, expire, flags, np.zeros(16, dtype=np.uint8))]
    d_keys, d_koff, d_vals, d_voff, d_moff, d_expire, d_flags, d_metas = d  # no record has an app meta
    need = int(L.lib.bcw_write_bound(n, keys.size, vals.size, 0, ETAG, 40))
    image = torch.zeros(40 + need, dtype=torch.uint8, device=dev)
    sb = (C.c_uint8 * 40)()
    L.lib.bcw_write_super_block(sb, BASE_TIME, BASE_TIME)
    image[:40] = torch.frombuffer(bytearray(bytes(sb)), dtype=torch.uint8).to(dev)
    d_off = torch.zeros(n, dtype=torch.int64, device=dev)
    d_size = torch.zeros(n, dtype=torch.int64, device=dev)
    d_res = torch.zeros(C.sizeof(L.WriteResult), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    arr = L.WriteBatchArrays(n, d_keys.data_ptr(), d_koff.data_ptr(), keys.size, d_vals.data_ptr(), d_voff.data_ptr(),
                             vals.size, d_metas.data_ptr(), d_moff.data_ptr(), 0, None, d_expire.data_ptr(), d_flags.data_ptr())
    p = L.WriteParams(FID, BASE_TIME, 40, NS, ETAG)
    out = L.WriteOut(image.data_ptr() + 40, need, d_off.data_ptr(), d_size.data_ptr(), None, None, None)
    assert L.lib.bcw_write_records_async(ix.handle, C.byref(p), C.byref(arr), C.byref(out),
                                         C.c_void_p(d_res.data_ptr())) == 0
    stream.synchronize()
    r = L.WriteResult.from_buffer_copy(bytes(d_res.cpu().numpy()))
    assert (r.err_class, r.idx_err, r.fits, r.n_written) == (0, 0, 1, n), (r.err_class, r.idx_err, r.fits, r.n_written)
    return image, int(r.wal_end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seg-mib", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=1000, help="filter launches per timed window")
    ap.add_argument("--reps", type=int, default=9, help="timed windows per case")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per case")
    args = ap.parse_args()
    if L.lib.bcw_device_count() < 1:
        sys.exit("bench_filter: no HIP device")
    try:
        set_rules = L.lib.bcw_index_set_compact_rules
        set_rules.restype, set_rules.argtypes = C.c_int, [C.c_void_p, C.POINTER(Rules)]
    except AttributeError:
        set_rules = None

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(stream.cuda_stream)
    n_rec = (args.seg_mib << 20) // (VAL + KEY + NS + 16)
    ix = Index(ctx, keys=n_rec + (n_rec >> 2), arena_bytes=n_rec * 160 + (1 << 20))
    d_seg, seg_len = write_segment(ctx, ix, stream, n_rec, dev)
    cap = n_rec + 64
    tdt = {"u8": torch.int64, "u4": torch.int32, "u1": torch.uint8}
    ptr_t = {"u8": L.u64p, "u4": L.u32p, "u1": L.u8p}
    cols = {name: torch.zeros(cap, dtype=tdt[dt], device=dev) for name, dt in L.TABLE_COLUMNS}
    table = L.RecordTable(cap, *[C.cast(C.c_void_p(cols[nm].data_ptr()), ptr_t[dt]) for nm, dt in L.TABLE_COLUMNS])
    d_res = torch.zeros(C.sizeof(L.DecodeResult), dtype=torch.uint8, device=dev)
    d_ir = torch.zeros(C.sizeof(L.IndexResult), dtype=torch.uint8, device=dev)
    keep = torch.zeros(cap, dtype=torch.uint8, device=dev)
    p = L.DecodeParams(seg_len, BASE_TIME, 40, NS, ETAG, L.MODE_RECORD)
    torch.cuda.synchronize()

    def decode() -> L.DecodeResult:
        for _ in range(2):  # a result with retry_frag_capacity != 0 is invalid: reserve and decode again
            assert L.lib.bcw_decode_segment_async(ctx.handle, C.c_void_p(d_seg.data_ptr()), C.byref(p),
                                                  C.byref(table), C.c_void_p(d_res.data_ptr())) == 0
            stream.synchronize()
            r = L.DecodeResult.from_buffer_copy(bytes(d_res.cpu().numpy()))
            if not r.retry_frag_capacity:
                return r
            assert L.lib.bcw_ctx_reserve_fragments(ctx.handle, r.retry_frag_capacity + 64) == 0
        sys.exit("bench_filter: decode retry failed")

    dres = decode()
    assert dres.err_class == 0 and dres.n_records == n_rec and dres.first_bad_record == -1
    assert ix.stats().live == n_rec

    def filt():
        assert L.lib.bcw_compact_filter_async(ix.handle, C.c_void_p(d_seg.data_ptr()), C.byref(p), C.byref(table),
                                              C.c_void_p(d_res.data_ptr()), FID, C.c_void_p(keep.data_ptr()),
                                              C.c_void_p(d_ir.data_ptr())) == 0

    def rules_of(mask, prefixes=()):
        flat = np.frombuffer(b"".join(prefixes) or b"\0", dtype=np.uint8).copy()
        off = np.zeros(len(prefixes) + 1, dtype=np.uint32)
        np.cumsum([len(q) for q in prefixes], out=off[1:])
        return Rules(mask, len(prefixes), NOW, flat.ctypes.data, off.ctypes.data), (flat, off)

    ns_even, ns_odd = bytes([65]) + bytes(66 + j for j in range(1, NS)), bytes(66 + j for j in range(NS))
    cases = {"a_no_rules": (None, n_rec)}
    if set_rules is not None:
        cases["b_column_rules_no_match"] = (rules_of(RULE_EXPIRED | RULE_TOMBSTONE), n_rec)
        cases["c_64_prefixes_no_match"] = (rules_of(RULE_PREFIX, [(ns_odd if j % 2 else ns_even) + bytes([0xFF, j]) * 22
                                                                 for j in range(64)]), n_rec)
        cases["d_half_rows_match"] = (rules_of(RULE_PREFIX, [b"A"]), n_rec // 2)
    def select(name):
        ru = cases[name][0]
        if set_rules is not None:
            assert set_rules(ix.handle, C.byref(ru[0]) if ru else None) == 0

    def window(name) -> float:
        select(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        for _ in range(args.iters):
            filt()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / args.iters

    # every case keeps what it should (checked once, before anything is timed)
    for name, (_, want) in cases.items():
        select(name)
        keep.fill_(0xFF)
        torch.cuda.synchronize()
        filt()
        stream.synchronize()
        r = L.IndexResult.from_buffer_copy(bytes(d_ir.cpu().numpy()))
        assert (r.err_class, r.n_in, r.n_done) == (0, n_rec, want), (name, r.err_class, r.n_in, r.n_done, want)
        assert int(keep[:n_rec].sum().item()) == want and int(keep[n_rec:].sum().item()) == 0, name

    ms = {k: [] for k in cases}
    for rep in range(args.warmup + args.reps):
        for name in cases:  # interleaved
            t = window(name)
            if rep >= args.warmup:
                ms[name].append(t)
    out = {"bench": "filter", "rows": n_rec, "seg_bytes": seg_len, "record_shape": {"ns": NS, "key": KEY, "value": VAL},
           "iters_per_window": args.iters, "windows": args.reps, "rules_supported": set_rules is not None,
           "launch_us": {k: {"median": round(1e3 * statistics.median(v), 2), "min": round(1e3 * min(v), 2),
                             "max": round(1e3 * max(v), 2)} for k, v in ms.items()},
           "rows_per_s": {k: round(n_rec / (statistics.median(v) * 1e-3)) for k, v in ms.items()},
           "kept": {k: w for k, (_, w) in cases.items()}}
    print(json.dumps(out))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
