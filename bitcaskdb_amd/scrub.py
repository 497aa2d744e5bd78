"""Scrub: every live, file-backed entry of the device index against the resident WALs (csrc/bcw_verify.hip).

  verify_index   bcw_index_verify: what DBImpl.Get (db_impl.go:567-587) of every key would run into, plus the check Get
                 does not make -- that the record at (fid, off, size) carries the entry's key
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import NamedTuple

from . import _lib as L
from .usage import FidUsage, FidUsageMap


class BadEntry(NamedTuple):
    key: bytes       # the entry's merged key ns || key
    fid: int
    off: int
    size: int
    cls: int         # VFY_NO_WAL, VFY_READ, VFY_RECORD or VFY_KEY
    rd_status: int   # RD_* when cls == VFY_READ, else 0
    rec_status: int  # ST_* when cls == VFY_RECORD, else 0


@dataclass
class ScrubReport:
    n_checked: int = 0       # live entries with off != 0
    n_soft_deleted: int = 0  # live entries with off == 0: not checked
    by_class: tuple = (0,) * 5   # by VFY_*; sums to n_checked
    by_rd: tuple = (0,) * 8      # the READ class by RD_*
    n_bad: int = 0
    bad: list = field(default_factory=list)              # BadEntry, in no particular order
    per_fid: FidUsageMap = field(default_factory=FidUsageMap)  # what a Delete of the bad keys frees, per file

    @property
    def clean(self) -> bool:
        return self.n_bad == 0


def verify_index(index, walset, ns_size: int = 20, etag_size: int = 20, verify: bool = True) -> ScrubReport:
    """bcw_index_verify of `index` against `walset` (both of one Context; ValueError otherwise). verify: compute the
    fragment CRCs (ReadOptions.VerifyChecksum). Read-only. Asks first for the totals alone and, when there are bad
    entries, again with room for them; nothing changes in between unless the caller changes it."""
    p = L.GetParams(ns_size, etag_size, 1 if verify else 0, 0)
    res = L.VerifyResult()
    bad = keys = rows = None
    out = L.VerifyOut()
    for _ in range(3):
        rc = L.lib.bcw_index_verify(index.handle, walset.handle, C.byref(p), C.byref(out), C.byref(res))
        if rc == L.E_INVAL:
            raise ValueError("bcw_index_verify: the index and the walset belong to different contexts")
        if rc == L.E_CAPACITY:
            if res.per_fid.overflow:
                raise RuntimeError(f"bad entries in more than {L.USAGE_MAX_FIDS} distinct fids")
            nb, kb, nr = int(res.n_bad), int(res.bad_key_bytes), int(res.per_fid.n_fids)
            bad, keys, rows = (L.VerifyBad * max(nb, 1))(), (C.c_uint8 * max(kb, 1))(), (L.FidUsageRow * max(nr, 1))()
            out = L.VerifyOut(C.cast(bad, C.c_void_p), nb, C.cast(keys, C.c_void_p), kb, C.cast(rows, C.c_void_p), nr,
                              0)
            continue
        if rc != 0:
            raise RuntimeError(f"bcw_index_verify: {L.lib.bcw_strerror(rc).decode()}")
        break
    else:
        raise RuntimeError("bcw_index_verify: the index changed between the calls")
    rep = ScrubReport(int(res.n_checked), int(res.n_soft_deleted), tuple(int(v) for v in res.by_class),
                      tuple(int(v) for v in res.by_rd), int(res.n_bad))
    if rep.n_bad:
        kb = bytes(keys)
        rep.bad = [BadEntry(kb[int(b.key_pos):int(b.key_pos) + int(b.key_len)], int(b.fid), int(b.off), int(b.size),
                            int(b.cls), int(b.rd_status), int(b.rec_status)) for b in bad[:rep.n_bad]]
        for r in rows[:int(res.per_fid.n_fids)]:
            rep.per_fid[int(r.fid)] = FidUsage(int(r.count), int(r.bytes), int(r.span))
    rep.per_fid.soft_deleted, rep.per_fid.invalid = int(res.per_fid.soft_deleted), int(res.per_fid.invalid)
    return rep


__all__ = ["BadEntry", "ScrubReport", "verify_index"]
