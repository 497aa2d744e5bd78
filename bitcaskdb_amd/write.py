"""Host mirror of the write path, backed by bcw_write_records_async (csrc/bcw_put.hip).

  WriteBatch            Batch                          batch.go
  ActiveWal             manifest.active (the Wal DBImpl.Write appends to), its image resident in HBM
  write_batch           DBImpl.writeWal + writeIndex   db_impl.go:434-480   (Index.write calls it)
The group commit (buildBatchGroup, db_impl.go:482-...) stays with the caller: merge batches with WriteBatch.append.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._hip import DevMem
from .wal import Context, Meta, WalError, _ENC_ERRORS, default_context


class WriteBatch:
    """Batch (batch.go): records in call order; byte_size sums Record.ApproximateSize (record.go:50-55)."""

    def __init__(self):
        self.records = []  # (ns, key, value, etag, expire, app_meta bytes, flags)
        self._byte_size = 0

    @staticmethod
    def _approx(ns, key, val, etag, app_meta_size) -> int:
        # 1B header size + len(ns) + 1B flags + 2B varint * 3 + len(etag) + 2B expire
        return 1 + len(ns) + 1 + 2 * 3 + len(etag) + 2 + len(key) + len(val) + app_meta_size

    def put(self, ns: bytes, key: bytes, val: bytes, meta: Meta | None = None, app_meta_size: int | None = None):
        """Batch.Put. meta (wal.Meta): expire, etag, the tombstone flag and app_meta, the msgpack bytes of
        Meta.AppMeta -- empty when AppMetaSize == 0 (Record.Encode drops the meta then, record.go:82-86);
        app_meta_size: AppMetaSize (the sum of the map's key and value lengths, meta.go:38-49) when the caller knows
        it, else len(app_meta)."""
        etag = bytes(meta.etag) if meta is not None and meta.etag else b""
        expire = int(meta.expire) if meta is not None else 0
        app_meta = bytes(meta.app_meta) if meta is not None else b""
        fl = (L.WR_TOMBSTONE if meta is not None and meta.is_tombstone() else 0) | (L.WR_ETAG if etag else 0)
        self.records.append((bytes(ns), bytes(key), bytes(val), etag, expire, bytes(app_meta), fl))
        self._byte_size += self._approx(ns, key, val, etag, len(app_meta) if app_meta_size is None else app_meta_size)

    def delete(self, ns: bytes, key: bytes):
        """Batch.Delete: a tombstone record that also removes the key from the index (Record.Deleted)."""
        self.records.append((bytes(ns), bytes(key), b"", b"", 0, b"", L.WR_TOMBSTONE | L.WR_DELETED))
        self._byte_size += self._approx(ns, key, b"", b"", 0)

    def clear(self):
        self.records = []
        self._byte_size = 0

    def append(self, other: "WriteBatch | None"):
        if other is None:
            return
        self.records.extend(other.records)
        self._byte_size += other._byte_size

    def size(self) -> int:
        return len(self.records)

    def byte_size(self) -> int:
        return self._byte_size

    def arrays(self, etag_size: int):
        """the field arrays of bcw_write_batch (host, numpy): keys (ns || key), values, metas with their offsets,
        etags (n x etag_size), expire, flags"""
        n = len(self.records)

        def pack(parts):
            off = np.zeros(n + 1, dtype=np.uint64)
            if n:
                np.cumsum([len(p) for p in parts], out=off[1:])
            return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off

        keys, koff = pack([r[0] + r[1] for r in self.records])
        vals, voff = pack([r[2] for r in self.records])
        metas, moff = pack([r[5] for r in self.records])
        etags = np.zeros(n * etag_size, dtype=np.uint8)
        for i, r in enumerate(self.records):
            if r[6] & L.WR_ETAG:
                if len(r[3]) != etag_size:
                    raise ValueError(f"record {i}: etag of {len(r[3])} bytes, EtagSize is {etag_size}")
                etags[i * etag_size:(i + 1) * etag_size] = np.frombuffer(r[3], dtype=np.uint8)
        expire = np.array([r[4] for r in self.records], dtype=np.uint64)
        flags = np.array([r[6] for r in self.records], dtype=np.uint8)
        return keys, koff, vals, voff, metas, moff, etags, expire, flags


class ActiveWal:
    """The active WAL's image in HBM: `capacity` bytes of device memory holding the file's first `size` bytes (the
    super block written at creation). Index.write appends to it; with a WalSet given, the image is registered under
    its fid and re-registered with the new length after every write, so later gets see the new records."""

    def __init__(self, fid: int, base_time: int, capacity: int, create_time: int | None = None,
                 ctx: Context | None = None, walset=None):
        if capacity < L.SUPER_BLOCK_SIZE:
            raise ValueError("capacity below the super block size")
        self.ctx = ctx or default_context()
        self.fid, self.base_time, self.capacity = fid, base_time, int(capacity)
        self._mem = DevMem(self.capacity)
        sb = (C.c_uint8 * 40)()
        L.lib.bcw_write_super_block(sb, base_time if create_time is None else create_time, base_time)
        self._mem.upload(bytes(sb))
        self.size = L.SUPER_BLOCK_SIZE
        self.walset = None
        if walset is not None:
            self.register(walset)

    @property
    def ptr(self) -> int:
        return self._mem.ptr

    def register(self, walset):
        """make the image resident in `walset` under its fid (bcw_walset_put with the current size)"""
        self.walset = walset
        walset.put_device(self.fid, self.ptr, self.size, self.base_time)

    def grow(self, capacity: int):
        """a larger image with the same bytes (the old one is freed once copied)"""
        if capacity <= self.capacity:
            return
        self.ctx.sync()
        old = self._mem.download(self.size)
        mem = DevMem(capacity)
        mem.upload(old)
        if self.walset is not None:
            self.walset.put_device(self.fid, mem.ptr, self.size, self.base_time)
            self.ctx.sync()
        self._mem.free()
        self._mem, self.capacity = mem, int(capacity)

    def bytes(self) -> bytes:
        """the file image [0, size)"""
        self.ctx.sync()
        return self._mem.download(self.size).tobytes()

    def close(self):
        if self.walset is not None and self.walset.handle:
            self.walset.remove(self.fid)
            self.ctx.sync()
        self.walset = None
        self._mem.free()


def write_batch(index, active: ActiveWal, batch: WriteBatch, walset=None, ns_size: int = 20, etag_size: int = 20,
                stats_on_device: bool = False):
    """DBImpl.Write's writeWal + writeIndex (db_impl.go:434-480) on the device: the batch's records are encoded and
    framed into `active`'s image at its current size, the index receives Put / Delete / SoftDelete with the offsets
    the writer returned. Returns (locs [(off, size)], write_stats {FreeWalFid: FreeBytes}) as the reference's locs
    and writeStats. Raises WalError("invalid expire") / RefPanic as Record.Encode does, with nothing written and the
    index untouched; grows the image and retries when the bytes do not fit.
    stats_on_device: the WriteStat columns stay in HBM and write_stats comes from bcw_freed_by_fid_async (the same
    dict: one row per fid instead of two columns of n entries over the bus and a host loop over them)."""
    if index.ctx is not active.ctx:
        raise ValueError("the index and the active WAL belong to different contexts")
    ws = walset if walset is not None else active.walset
    if ws is not None and active.walset is not ws:
        active.register(ws)
    n = batch.size()
    if n == 0:
        return [], {}
    keys, koff, vals, voff, metas, moff, etags, expire, flags = batch.arrays(etag_size)
    host = [keys, koff, vals, voff, metas, moff, etags, expire, flags]
    dev = [DevMem(a.nbytes).upload(a) for a in host]
    outs = [DevMem(8 * n), DevMem(8 * n), DevMem(n), DevMem(8 * n), DevMem(8 * n), DevMem(C.sizeof(L.WriteResult))]
    d_off, d_size, d_found, d_ffid, d_fbytes, d_res = outs
    arr = L.WriteBatchArrays(n, dev[0].ptr, dev[1].ptr, keys.nbytes, dev[2].ptr, dev[3].ptr, vals.nbytes, dev[4].ptr,
                             dev[5].ptr, metas.nbytes, dev[6].ptr if etag_size else None, dev[7].ptr, dev[8].ptr)
    need = int(L.lib.bcw_write_bound(n, keys.nbytes, vals.nbytes, metas.nbytes, etag_size, active.size))
    if active.size + need > active.capacity:
        active.grow(max(2 * active.capacity, active.size + need))
    while True:
        p = L.WriteParams(active.fid, active.base_time, active.size, ns_size, etag_size)
        out = L.WriteOut(active.ptr + active.size, active.capacity - active.size, d_off.ptr, d_size.ptr, d_found.ptr,
                         d_ffid.ptr, d_fbytes.ptr)
        rc = L.lib.bcw_write_records_async(index.handle, C.byref(p), C.byref(arr), C.byref(out), C.c_void_p(d_res.ptr))
        if rc != 0:
            raise RuntimeError(f"bcw_write_records_async: {L.lib.bcw_strerror(rc).decode()}")
        index.ctx.sync()
        res = L.WriteResult.from_buffer_copy(d_res.download(C.sizeof(L.WriteResult)).tobytes())
        if res.err_class == L.ENC_ERR_BATCH:
            raise ValueError(f"record {res.err_record}: a key shorter than NsSize or a payload of 2^32 bytes or more")
        if res.err_class in _ENC_ERRORS:
            raise _ENC_ERRORS[res.err_class]()
        if not res.fits:  # BCW_E_CAPACITY of the sync call: a larger image, then once more
            active.grow(active.size + int(res.wal_need))
            continue
        break
    if res.idx_err:
        raise RuntimeError(f"index put failed: {res.idx_err}")
    active.size = int(res.wal_end)
    if active.walset is not None:
        active.walset.put_device(active.fid, active.ptr, active.size, active.base_time)
    off = d_off.download(8 * n, dtype=np.uint64)
    size = d_size.download(8 * n, dtype=np.uint64)
    if stats_on_device:
        from .usage import freed_by_fid
        return list(zip(off.tolist(), size.tolist())), freed_by_fid(index, n, d_found.ptr, d_ffid.ptr, d_fbytes.ptr,
                                                                    d_res.ptr)
    ffid = d_ffid.download(8 * n, dtype=np.uint64)
    fbytes = d_fbytes.download(8 * n, dtype=np.uint64)
    stats: dict = {}
    for f, b in zip(ffid.tolist(), fbytes.tolist()):  # writeStats[stat.FreeWalFid] += stat.FreeBytes
        stats[f] = stats.get(f, 0) + b
    return list(zip(off.tolist(), size.tolist())), stats


__all__ = ["WriteBatch", "ActiveWal", "write_batch", "WalError"]
