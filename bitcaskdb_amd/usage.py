"""Per-WAL space accounting: what the compaction picker reads, summed on the device (csrc/bcw_usage.hip).

  fid_usage                  live keys, value bytes and framed footprint per fid, from one pass over the index
  freed_by_fid               writeIndex's writeStats map (db_impl.go:434-454) from a write's device columns
  default_compaction_picker  DefaultCompactionPicker                          db.go:200-224
  wal_garbage                wal.size - 40 - span per WAL: the exact reclaimable bytes of every file
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

from . import _lib as L
from ._hip import DevMem


class FidUsage(NamedTuple):
    count: int  # keys whose value lives in the file
    bytes: int  # the sum of their valueSize (the unit of WriteStat.FreeBytes)
    span: int   # the sum of WalRecordSize(off, size): fragment headers and leading pads included


class FidUsageMap(dict):
    """{fid: FidUsage}, ascending by fid, plus what the pass saw besides: soft_deleted (present keys with off == 0)
    and invalid (present keys with 0 < off < 40, which no writer produces)"""
    soft_deleted = 0
    invalid = 0
    overflow = False  # drop_fids only: more distinct fids than the accounting holds, the rows are void


class PickerWalInfo(NamedTuple):  # compaction.go:135-150
    fid: int
    wal_size: int
    free_bytes: int


def _rows(mem: DevMem, n: int) -> list:
    if n == 0:
        return []
    raw = mem.download(n * C.sizeof(L.FidUsageRow)).tobytes()
    return list((L.FidUsageRow * n).from_buffer_copy(raw))


def fid_usage(index) -> FidUsageMap:
    """bcw_index_fid_usage_async on the index's stream: asked again with n_fids rows when the first table was too
    small; raises when the index holds more than BCW_USAGE_MAX_FIDS distinct fids"""
    cap = 64
    while True:
        d_rows, d_res = DevMem(cap * C.sizeof(L.FidUsageRow)), DevMem(C.sizeof(L.UsageResult))
        try:
            rc = L.lib.bcw_index_fid_usage_async(index.handle, C.c_void_p(d_rows.ptr), cap, C.c_void_p(d_res.ptr))
            if rc != 0:
                raise RuntimeError(f"bcw_index_fid_usage_async: {L.lib.bcw_strerror(rc).decode()}")
            index.ctx.sync()
            res = L.UsageResult.from_buffer_copy(d_res.download(C.sizeof(L.UsageResult)).tobytes())
            if res.overflow:
                raise RuntimeError(f"the index holds more than {L.USAGE_MAX_FIDS} distinct fids")
            if not res.fits:
                cap = int(res.n_fids)
                continue
            out = FidUsageMap((int(r.fid), FidUsage(int(r.count), int(r.bytes), int(r.span)))
                              for r in _rows(d_rows, int(res.n_fids)))
            out.soft_deleted, out.invalid = int(res.soft_deleted), int(res.invalid)
            return out
        finally:
            d_rows.free()
            d_res.free()


def drop_fids(index, fids, mode: int = L.DROP_IN) -> FidUsageMap:
    """bcw_index_drop_fids: remove every file-backed entry whose fid is in `fids` (DROP_IN: the files that were
    deleted) or is not in it (DROP_NOT_IN: keep only the files that exist), in one pass over the slot table on the
    index's stream. Returns what was dropped as fid_usage reports it, {fid: FidUsage} ascending, with .invalid (dropped
    entries with 0 < off < 40) and .soft_deleted (soft-deleted entries, which always stay). The call cannot be
    repeated, so the row buffer holds the most rows it can return; where a DROP_NOT_IN call met more than
    BCW_USAGE_MAX_FIDS distinct dead fids the drop is still complete and the map comes back empty with .overflow set.
    ValueError for a list of more than BCW_USAGE_MAX_FIDS distinct fids or an unknown mode (the index is untouched)."""
    import numpy as np
    fa = np.ascontiguousarray([int(f) for f in fids], dtype=np.uint64)
    nf = int(fa.size)
    cap = max(min(nf, L.USAGE_MAX_FIDS), 1) if mode == L.DROP_IN else L.USAGE_MAX_FIDS
    rows, res = (L.FidUsageRow * cap)(), L.UsageResult()
    rc = L.lib.bcw_index_drop_fids(index.handle, mode, fa.ctypes.data_as(L.u64p) if nf else None, nf, rows, cap,
                                   C.byref(res))
    if rc == L.E_INVAL:
        raise ValueError(f"bcw_index_drop_fids: mode {mode} or more than {L.USAGE_MAX_FIDS} distinct fids")
    if rc != 0:
        raise RuntimeError(f"bcw_index_drop_fids: {L.lib.bcw_strerror(rc).decode()}")
    out = FidUsageMap()
    out.soft_deleted, out.invalid, out.overflow = int(res.soft_deleted), int(res.invalid), bool(res.overflow)
    if not res.overflow:
        assert res.fits, "the row buffer holds every row a drop can return"
        for r in rows[:int(res.n_fids)]:
            out[int(r.fid)] = FidUsage(int(r.count), int(r.bytes), int(r.span))
    return out


def freed_by_fid(index, n: int, d_found: int, d_free_fid: int, d_free_bytes: int, d_gate: int | None = None) -> dict:
    """writeStats {FreeWalFid: FreeBytes} of a write's n ops from its WriteStat columns on the device
    (bcw_freed_by_fid_async, queued behind the write on the index's stream): only the grouped rows are downloaded"""
    cap = 64
    while True:
        d_rows, d_res = DevMem(cap * C.sizeof(L.FidUsageRow)), DevMem(C.sizeof(L.UsageResult))
        try:
            rc = L.lib.bcw_freed_by_fid_async(index.handle, n, C.c_void_p(d_found), C.c_void_p(d_free_fid),
                                              C.c_void_p(d_free_bytes), C.c_void_p(d_gate) if d_gate else None,
                                              C.c_void_p(d_rows.ptr), cap, C.c_void_p(d_res.ptr))
            if rc != 0:
                raise RuntimeError(f"bcw_freed_by_fid_async: {L.lib.bcw_strerror(rc).decode()}")
            index.ctx.sync()
            res = L.UsageResult.from_buffer_copy(d_res.download(C.sizeof(L.UsageResult)).tobytes())
            if res.overflow:
                raise RuntimeError(f"the batch freed values of more than {L.USAGE_MAX_FIDS} distinct fids")
            if not res.fits:
                cap = int(res.n_fids)
                continue
            return {int(r.fid): int(r.bytes) for r in _rows(d_rows, int(res.n_fids))}
        finally:
            d_rows.free()
            d_res.free()


def default_compaction_picker(infos, ratio: float) -> list:
    """DefaultCompactionPicker (db.go:200-224): the WALs by FreeBytes descending, stop at the first whose FreeBytes /
    WalSize is below `ratio` (gOpts.CompactionPickerRatio), at most 2 fids. infos: PickerWalInfo or (fid, wal_size,
    free_bytes) tuples. Go's sort.Slice is not stable, so the reference's order among equal FreeBytes is unspecified:
    here ties are broken by ascending fid."""
    wals = sorted((PickerWalInfo(*w) for w in infos), key=lambda w: (-w.free_bytes, w.fid))
    res = []
    for w in wals:
        # float64 division as in Go: x / 0 is +Inf and 0 / 0 is NaN, and neither is below the ratio
        if w.wal_size != 0 and float(w.free_bytes) / float(w.wal_size) < ratio:
            break
        res.append(w.fid)
        if len(res) >= 2:
            break
    return res


def wal_garbage(index, wals) -> dict:
    """{fid: wal.size - 40 - span}: the bytes of each WAL file that no live key's record occupies (super block
    excluded), from one fid_usage pass. wals: {fid: file size} or objects with .fid and .size (write.ActiveWal)."""
    sizes = dict(wals) if isinstance(wals, dict) else {int(w.fid): int(w.size) for w in wals}
    use = fid_usage(index)
    return {fid: int(sz) - L.SUPER_BLOCK_SIZE - (use[fid].span if fid in use else 0) for fid, sz in sizes.items()}


__all__ = ["FidUsage", "FidUsageMap", "PickerWalInfo", "fid_usage", "drop_fids", "freed_by_fid",
           "default_compaction_picker", "wal_garbage"]
