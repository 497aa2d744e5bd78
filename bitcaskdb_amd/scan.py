"""Scan of the device index by key prefix (csrc/bcw_index.hip, bcw_scan.h): list and fold a namespace in HBM.

  scan_index   bcw_index_scan: the live entries whose merged key ns || key starts with one of the prefixes (all of them
               without prefixes), with one row of counts per prefix -- classical Bitcask's list_keys
  fold_index   bcw_index_scan_async, then bcw_get_records_async on the very keys the scan left in HBM: every record
               under the prefixes -- classical Bitcask's fold

The reference has no counterpart: its hash map gives it no better way than a full walk.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import _lib as L
from ._hip import DevMem


class ScanGroup(NamedTuple):
    """the entries whose first matching prefix is this row's (bcw_scan_group)"""
    count: int         # file-backed entries (off != 0)
    bytes: int         # the sum of their sizes (wrapping uint64)
    key_bytes: int     # the sum of their key lengths
    soft_deleted: int  # entries with off == 0 (not in the three above)


@dataclass
class ScanReport:
    entries: dict = field(default_factory=dict)   # {merged key: (fid, off, size)} of the listed entries
    groups: list = field(default_factory=list)    # ScanGroup per prefix, in the order given (one row without prefixes)
    keys: list = field(default_factory=list)      # the listed keys in output (ascending slot) order
    prefix_id: list = field(default_factory=list)  # per listed key, the row it counts in
    result: L.ScanResult = field(default_factory=L.ScanResult)  # the raw bcw_scan_result

    @property
    def n_listed(self) -> int:
        return int(self.result.n_listed)

    @property
    def n_soft_deleted(self) -> int:
        return int(self.result.n_soft_deleted)


def _params(prefixes, soft_deleted: bool):
    """bcw_scan_params over `prefixes`, and the arrays it points into (kept alive by the caller)"""
    from .index import _pack
    prefixes = [bytes(p) for p in (prefixes or ())]
    flat, off = _pack(prefixes)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    p = L.ScanParams(L.SCAN_SOFT_DELETED if soft_deleted else 0, len(prefixes), flat.ctypes.data, off.ctypes.data)
    return p, (flat, off), max(len(prefixes), 1)


def scan_index(index, prefixes=None, soft_deleted: bool = False) -> ScanReport:
    """bcw_index_scan of `index`: the live, file-backed entries under `prefixes` (at most 64, of 1..64 bytes each; None
    or empty: every entry), and with soft_deleted also the soft-deleted ones (value (0, 0, 0)). An entry counts in the
    row of the first prefix it starts with. Asks first for the totals alone and, when anything is listed, once more
    with room for it (BCW_E_CAPACITY); nothing changes in between unless the caller changes it. Read-only. ValueError
    for prefixes the library refuses."""
    p, keep, rows = _params(prefixes, soft_deleted)
    groups = (L.ScanGroup * rows)()
    res = L.ScanResult()
    out = L.ScanOut(None, 0, None, None, None, None, None, 0, C.cast(groups, C.c_void_p))
    arrays = None
    for attempt in range(2):
        rc = L.lib.bcw_index_scan(index.handle, C.byref(p), C.byref(out), C.byref(res))
        if rc == L.E_INVAL:
            raise ValueError("bcw_index_scan: invalid prefixes")
        if rc == L.E_CAPACITY and attempt == 0:
            n, kb = int(res.n_listed), int(res.key_bytes)
            keys = np.zeros(max(kb, 1), dtype=np.uint8)
            koff = np.zeros(n + 1, dtype=np.uint64)
            fid, off, size = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
            pid = np.zeros(max(n, 1), dtype=np.uint8)
            arrays = (keys, koff, fid, off, size, pid)
            out = L.ScanOut(keys.ctypes.data, kb, koff.ctypes.data, fid.ctypes.data, off.ctypes.data, size.ctypes.data,
                            pid.ctypes.data, n, C.cast(groups, C.c_void_p))
            continue
        if rc != 0:
            raise RuntimeError(f"bcw_index_scan: {L.lib.bcw_strerror(rc).decode()}")
        break
    rep = ScanReport(result=res)
    rep.groups = [ScanGroup(int(g.count), int(g.bytes), int(g.key_bytes), int(g.soft_deleted)) for g in groups]
    n = int(res.n_listed)
    if n:
        keys, koff, fid, off, size, pid = arrays
        kbytes = keys.tobytes()
        rep.keys = [kbytes[int(koff[i]):int(koff[i + 1])] for i in range(n)]
        rep.prefix_id = [int(v) for v in pid[:n]]
        rep.entries = {k: (int(fid[i]), int(off[i]), int(size[i])) for i, k in enumerate(rep.keys)}
    del keep
    return rep


def _dev_table(n: int):
    """a device record table of n rows (no hint columns, no fragment ids): the bcw_record_table and its buffers"""
    mems, ptrs = {}, {}
    for name, dt in L.TABLE_COLUMNS:
        if name in ("aux0", "aux1", "first_frag", "emit_frag"):
            ptrs[name] = None
            continue
        mems[name] = DevMem(n * np.dtype(dt).itemsize)
        ty = L.u8p if dt == "u1" else (L.u32p if dt == "u4" else L.u64p)
        ptrs[name] = C.cast(C.c_void_p(mems[name].ptr), ty)
    return L.RecordTable(n, *[ptrs[name] for name, _ in L.TABLE_COLUMNS]), mems


def fold_index(index, walset, prefixes, verify: bool = False, ns_size: int = 20, etag_size: int = 20,
               soft_deleted: bool = False):
    """every record under `prefixes`: (keys, items), items as Index.get_records returns them (a wal.Record, or the
    error instance the reference's Get returns for that key), in the scan's order. The keys do not visit the host on
    their way from the index to the Get: bcw_index_scan_async leaves them and their offsets in device buffers sized
    from the index's live count and arena use, its 48-byte result is read back, and bcw_get_records_async takes those
    same two buffers with n = n_listed; the keys are copied out at the end, with the records. With soft_deleted the
    soft-deleted keys come too, each with ErrKeySoftDeleted."""
    from .index import GetBatch, _get_items
    if index.ctx is not walset.ctx:
        raise ValueError("the index and the walset belong to different contexts")
    p, keep, _ = _params(prefixes, soft_deleted)
    st = index.stats()
    ecap, kcap = st.live, st.arena_used  # every live entry, every key byte the arena holds: nothing larger can come
    d_keys, d_koff, d_sres = DevMem(kcap + 16), DevMem(8 * (ecap + 1)), DevMem(C.sizeof(L.ScanResult))
    out = L.ScanOut(d_keys.ptr, kcap, d_koff.ptr, None, None, None, None, ecap, None)
    rc = L.lib.bcw_index_scan_async(index.handle, C.byref(p), C.byref(out), C.c_void_p(d_sres.ptr))
    if rc == L.E_INVAL:
        raise ValueError("bcw_index_scan_async: invalid prefixes")
    if rc != 0:
        raise RuntimeError(f"bcw_index_scan_async: {L.lib.bcw_strerror(rc).decode()}")
    index.ctx.sync()
    del keep
    sres = L.ScanResult.from_buffer_copy(d_sres.download(C.sizeof(L.ScanResult)).tobytes())
    if not sres.fits:
        raise RuntimeError("bcw_index_scan_async: the index changed under the scan")
    n = int(sres.n_listed)
    if n == 0:
        return [], []
    gp = L.GetParams(ns_size, etag_size, 1 if verify else 0, 0)
    cols = {name: DevMem(n * w) for name, w in (("get_status", 1), ("rd_status", 1), ("fid", 8), ("off", 8),
                                                ("size", 8), ("pay_off", 8))}
    tab, tmem = _dev_table(n)
    d_gres = DevMem(C.sizeof(L.GetResult))
    cap = min(int(sres.bytes) + 15 * n, 1 << 26)  # the sizes are the index's word: a too small guess is retried
    for attempt in range(2):
        d_pay = DevMem(cap + 16)
        u8 = lambda m: C.cast(C.c_void_p(m.ptr), L.u8p)  # noqa: E731
        u64 = lambda m: C.cast(C.c_void_p(m.ptr), L.u64p)  # noqa: E731
        gout = L.GetOut(u8(cols["get_status"]), u8(cols["rd_status"]), u64(cols["fid"]), u64(cols["off"]),
                        u64(cols["size"]), u64(cols["pay_off"]), u8(d_pay), cap, tab)
        rc = L.lib.bcw_get_records_async(index.handle, walset.handle, C.byref(gp), n, C.c_void_p(d_keys.ptr),
                                         C.c_void_p(d_koff.ptr), C.byref(gout), C.c_void_p(d_gres.ptr))
        if rc != 0:
            raise RuntimeError(f"bcw_get_records_async: {L.lib.bcw_strerror(rc).decode()}")
        index.ctx.sync()
        gres = L.GetResult.from_buffer_copy(d_gres.download(C.sizeof(L.GetResult)).tobytes())
        if gres.fits or attempt == 1:
            break
        cap = int(gres.payload_need)
    if not gres.fits:
        raise RuntimeError("bcw_get_records_async: the payload did not fit the size the first call reported")
    table = {name: (tmem[name].download(n * np.dtype(dt).itemsize, dtype=np.dtype(dt)) if name in tmem
                    else np.zeros(n, dtype=dt)) for name, dt in L.TABLE_COLUMNS}
    b = GetBatch(0, gres, cols["get_status"].download(n), cols["rd_status"].download(n),
                 cols["fid"].download(8 * n, dtype=np.uint64), cols["off"].download(8 * n, dtype=np.uint64),
                 cols["size"].download(8 * n, dtype=np.uint64), cols["pay_off"].download(8 * n, dtype=np.uint64),
                 d_pay.download(cap), table)
    koff = d_koff.download(8 * (n + 1), dtype=np.uint64)
    kbytes = d_keys.download(int(sres.key_bytes)).tobytes()
    keys = [kbytes[int(koff[i]):int(koff[i + 1])] for i in range(n)]
    return keys, _get_items(b, n, ns_size, etag_size)


__all__ = ["ScanGroup", "ScanReport", "scan_index", "fold_index"]
