"""GPU tests of retiring WAL files from the device index (bcw_index_drop_fids*, k_ix_drop in csrc/bcw_index.hip):
every outcome is compared with a host dict model of the index, key -> (fid, off, size, seq), from which a drop removes
the selected entries (test_drop_host.py checks that predicate against a set model). The span of a row comes from
bcw_wal_record_size, the reference's loop. Shapes: the smallest table (1024 slots), a table of 2^21 slots whose
workgroups take more than one round, 4096 fids (the accounting's LDS table overflows into the global one, and the fid
list fills its 32 KiB of LDS), one fid for every lane of a wave, and the fids 0 and 2^64 - 1."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import _devmem as D
import _oracle as O
from bitcaskdb_amd import ActiveWal, ErrKeyNotFound, FidUsage, Index, WalSet, WriteBatch
from bitcaskdb_amd import _lib as L
from test_gpu_index_reclaim import _entry_bytes, _RoomReplay

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
BASE = 1_700_000_000
SENT = 0x5A5A5A5A5A5A5A5A
ROW = C.sizeof(L.FidUsageRow)
U64 = 2 ** 64 - 1


def key_of(i: int) -> bytes:
    return (b"ns-%03d-" % (i % 7) * 4)[:NS] + b"key-%06d" % i


def span(off: int, size: int) -> int:
    return int(L.lib.bcw_wal_record_size(off, size))


class Model:
    """the index as a dict: key -> (fid, off, size, seq); ops in order on a logical clock"""

    def __init__(self):
        self.d = {}
        self.t = 0
        self.seen = {}  # every key ever applied, in order

    def apply(self, ix: Index, ops, keys, fid=None, off=None, size=None):
        n = len(keys)
        z = [0] * n
        fid, off, size = fid or z, off or z, size or z
        ix.apply(ops, keys, fid, off, size)
        for op, k, f, o, s in zip(ops, keys, fid, off, size):
            self.t += 1
            self.seen.setdefault(k)
            if op == L.IDX_DELETE:
                self.d.pop(k, None)
            elif op == L.IDX_SOFT_DELETE:
                self.d[k] = (0, 0, 0, self.t)
            else:
                self.d[k] = (f, o, s, self.t)

    def drop(self, mode: int, fids):
        """remove what the call selects: ({fid: FidUsage} of the dropped entries, invalid, soft_deleted kept, dropped)"""
        fids = set(fids)
        rows, inv, n = {}, 0, 0
        soft = sum(1 for v in self.d.values() if v[1] == 0)
        for k, (f, o, s, _) in list(self.d.items()):
            if o == 0 or (f in fids) != (mode == L.DROP_IN):
                continue
            del self.d[k]
            n += 1
            if o < 40:
                inv += 1
            else:
                c, b, sp = rows.get(f, (0, 0, 0))
                rows[f] = (c + 1, (b + s) & U64, (sp + span(o, s)) & U64)
        return {f: FidUsage(*rows[f]) for f in sorted(rows)}, inv, soft, n

    def export(self):
        return {k: v[:3] for k, v in self.d.items()}


def check_state(ix: Index, m: Model):
    """get_many of every key ever applied and export() are the model's"""
    keys = list(m.seen)
    st, fid, off, size = ix.get_many(keys)
    for i, k in enumerate(keys):
        v = m.d.get(k)
        if v is None:
            assert st[i] == L.IDX_NOT_FOUND, (i, k)
        elif v[1] == 0:
            assert st[i] == L.IDX_SOFT_DELETED, (i, k)
        else:
            assert (int(st[i]), int(fid[i]), int(off[i]), int(size[i])) == (L.IDX_FOUND, v[0], v[1], v[2]), (i, k)
    assert ix.export() == m.export()


def drop_sync(ix: Index, mode: int, fids, cap: int, null_list: bool = False, n_fids: int | None = None):
    """bcw_index_drop_fids with the row buffer pre-filled: (rc, result, rows as an n x 4 array)"""
    fa = np.ascontiguousarray(list(fids), dtype=np.uint64)
    rows = np.full(4 * max(cap, 1), SENT, dtype=np.uint64)
    res = L.UsageResult()
    n = int(fa.size) if n_fids is None else n_fids
    rc = L.lib.bcw_index_drop_fids(ix.handle, mode, None if null_list or fa.size == 0 else fa.ctypes.data_as(L.u64p), n,
                                   C.cast(rows.ctypes.data, C.POINTER(L.FidUsageRow)) if cap else None, cap,
                                   C.byref(res))
    return rc, res, rows.reshape(-1, 4)


def rows_of(got, n):
    return {int(r[0]): FidUsage(int(r[1]), int(r[2]), int(r[3])) for r in got[:n]}


def small_table(ctx, seed=1):
    """1024 slots: 300 keys over the fids 3, 5, 7, 9, then 12 of them soft-deleted, 12 deleted, and four entries
    inside the super block (off 1 and 39, one of each under fid 5 and under fid 3)"""
    rng = random.Random(seed)
    ix = Index(ctx, keys=1024)
    ix.compact(shrink=True)
    assert ix.stats().slot_capacity == 1024
    m = Model()
    keys = [key_of(i) for i in range(300)]
    fids = [(3, 5, 7, 9)[i % 4] for i in range(300)]
    offs = [40 + rng.randrange(1 << 32) for _ in range(300)]
    sizes = [rng.choice([0, 1, 100, 4096, 32761, 70000]) for _ in range(300)]
    m.apply(ix, [L.IDX_PUT] * 300, keys, fids, offs, sizes)
    m.apply(ix, [L.IDX_SOFT_DELETE] * 12, keys[20:32])
    m.apply(ix, [L.IDX_DELETE] * 12, keys[40:52])
    m.apply(ix, [L.IDX_PUT] * 4, [key_of(1000 + i) for i in range(4)], [5, 5, 3, 3], [1, 39, 1, 39], [10, 20, 30, 40])
    assert ix.stats().slot_capacity == 1024
    return ix, m


def do_drop(ix: Index, m: Model, mode: int, fids):
    """one drop through the Python layer against the model: rows, counters, stats; returns (map, dropped)"""
    st0, before = ix.stats(), ix.fid_usage()
    got = ix.drop_fids(fids) if mode == L.DROP_IN else ix.retain_fids(fids)
    rows, inv, soft, n = m.drop(mode, fids)
    assert list(got) == sorted(got) and dict(got) == rows
    assert (got.invalid, got.soft_deleted, got.overflow) == (inv, soft, False)
    assert dict(got) == {f: before[f] for f in rows}  # the rows fid_usage gave for those fids just before the call
    st = ix.stats()
    assert st.live == st0.live - n and st.slots_used == st0.slots_used and st.slot_capacity == st0.slot_capacity
    after = ix.fid_usage()
    assert not set(rows) & set(after)
    assert dict(after) == {f: before[f] for f in before if f not in rows}
    return got, n


# 1. the smallest table ----------------------------------------------------------------------------------------
def test_smallest_table(ctx):
    ix, m = small_table(ctx)
    got, n = do_drop(ix, m, L.DROP_IN, [9, 5, 5])
    assert list(got) == [5, 9] and n > 100 and got.invalid == 2 and got.soft_deleted == 12
    check_state(ix, m)
    ix.close()


# 2. BCW_DROP_NOT_IN -------------------------------------------------------------------------------------------
def test_drop_not_in(ctx):
    a, ma = small_table(ctx)
    b, mb = small_table(ctx)
    ga, na = do_drop(a, ma, L.DROP_IN, [5, 9])
    gb, nb = do_drop(b, mb, L.DROP_NOT_IN, [3, 7])
    assert dict(ga) == dict(gb) and (ga.invalid, ga.soft_deleted, na) == (gb.invalid, gb.soft_deleted, nb)
    assert a.export() == b.export() and a.stats() == b.stats()
    check_state(b, mb)
    soft = [k for k, v in mb.d.items() if v[1] == 0]
    assert len(soft) == 12 and (b.get_many(soft)[0] == L.IDX_SOFT_DELETED).all()
    # the empty list: every file-backed key goes (the entries inside the super block too), the soft-deleted ones stay
    got, n = do_drop(b, mb, L.DROP_NOT_IN, [])
    assert list(got) == [3, 7] and got.invalid == 2 and got.soft_deleted == 12
    assert b.export() == {k: (0, 0, 0) for k in soft} and b.stats().live == 12
    check_state(b, mb)
    a.close()
    b.close()


# 3. lists that change nothing -----------------------------------------------------------------------------------
def test_lists_that_change_nothing(ctx):
    ix, m = small_table(ctx)
    before, st = ix.export(), ix.stats()
    # fids no key holds; fid 0 is what a soft-deleted entry stores, and names no file
    for fids in ([100, 4, 6, U64, 0], []):
        rc, res, got = drop_sync(ix, L.DROP_IN, fids, 8)
        assert rc == 0 and (res.n_fids, res.fits, res.overflow, res.count, res.bytes, res.span) == (0, 1, 0, 0, 0, 0)
        assert (res.invalid, res.soft_deleted) == (0, 12)
        assert (got == SENT).all()
        assert ix.export() == before and ix.stats() == st
    rc, res, got = drop_sync(ix, L.DROP_NOT_IN, [9, 7, 5, 3, 3], 8)  # every file that exists is kept
    assert rc == 0 and (res.n_fids, res.fits, res.invalid, res.soft_deleted) == (0, 1, 0, 12)
    assert ix.export() == before and ix.stats() == st
    check_state(ix, m)
    ix.close()


# 4. more than one round per workgroup -----------------------------------------------------------------------------
def test_grid_stride(ctx):
    ix = Index(ctx, keys=1 << 20)
    assert ix.stats().slot_capacity >= 2 ** 20  # above the grid's 8 workgroups per CU of 256 slots each
    rng = random.Random(4)
    m = Model()
    n = 20000
    keys = [key_of(i) for i in range(n)]
    m.apply(ix, [L.IDX_PUT] * n, keys, [(11, 12, 13, 14)[i % 4] for i in range(n)],
            [40 + rng.randrange(1 << 32) for _ in range(n)], [rng.randrange(1 << 16) for _ in range(n)])
    m.apply(ix, [L.IDX_SOFT_DELETE] * 100, keys[500:600])
    got, dropped = do_drop(ix, m, L.DROP_IN, [12, 14])
    assert dropped == sum(r.count for r in got.values()) > 9000
    check_state(ix, m)
    ix.close()


# 5. the accumulator's paths -----------------------------------------------------------------------------------
def _many_fids(k: int, seed: int):
    rng = random.Random(seed)
    out = set()
    while len(out) < k:
        out.add(rng.choice([rng.randrange(1, 5000), rng.randrange(1, 2 ** 64)]))
    return sorted(out)


@pytest.mark.parametrize("shape", ["4096_fids", "one_fid", "fid_0_and_max"])
def test_accumulator_paths(ctx, shape):
    ix = Index(ctx, keys=1 << 12)
    m = Model()
    rng = random.Random(5)
    if shape == "4096_fids":  # one key each, all dropped: rows past the LDS table's 512 slots and 8 probes
        fids = _many_fids(L.USAGE_MAX_FIDS, 6)
        n = len(fids)
        order = fids[:]
        rng.shuffle(order)
        m.apply(ix, [L.IDX_PUT] * n, [key_of(i) for i in range(n)], order, [40 + 100 * i for i in range(n)],
                [1 + i % 500 for i in range(n)])
        listed = order[::-1]
    elif shape == "one_fid":  # whole waves share a fid
        n = 3000
        m.apply(ix, [L.IDX_PUT] * n, [key_of(i) for i in range(n)], [77] * n, [40 + 100 * i for i in range(n)],
                [rng.randrange(1 << 20) for _ in range(n)])
        listed = [77]
    else:
        n = 2000
        m.apply(ix, [L.IDX_PUT] * n, [key_of(i) for i in range(n)], [(0, U64, 8)[i % 3] for i in range(n)],
                [40 + rng.randrange(1 << 30) for _ in range(n)], [rng.randrange(1 << 12) for _ in range(n)])
        listed = [U64, 0]
    got, dropped = do_drop(ix, m, L.DROP_IN, listed)
    assert list(got) == sorted(set(listed))
    assert dropped == sum(r.count for r in got.values())
    if shape == "4096_fids":
        assert len(got) == 4096 and all(r.count == 1 for r in got.values()) and ix.stats().live == 0
    elif shape == "fid_0_and_max":
        assert list(ix.fid_usage()) == [8]
    check_state(ix, m)
    ix.close()


# 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_untouched(ctx):
    ix, m = small_table(ctx)
    before, st = ix.export(), ix.stats()
    too_many = list(range(1, L.USAGE_MAX_FIDS + 2))  # 4097 distinct, the index's own fids among them
    for rc, res, got in (drop_sync(ix, L.DROP_IN, too_many, 8), drop_sync(ix, L.DROP_NOT_IN, too_many, 8),
                         drop_sync(ix, 2, [5, 9], 8), drop_sync(ix, -1, [5, 9], 8),
                         drop_sync(ix, L.DROP_IN, [5, 9], 8, null_list=True, n_fids=2),
                         drop_sync(ix, L.DROP_NOT_IN, [5], 8, null_list=True, n_fids=3)):
        assert rc == L.E_INVAL
        assert (got == SENT).all()
        assert ix.export() == before and ix.stats() == st
    with pytest.raises(ValueError):
        ix.drop_fids(too_many)
    with pytest.raises(ValueError):
        ix.retain_fids(too_many)
    assert ix.export() == before and ix.stats() == st
    # 5000 entries with only 4096 distinct fids are accepted
    rng = random.Random(7)
    distinct = list(range(1, L.USAGE_MAX_FIDS + 1))
    listed = distinct + [rng.choice(distinct) for _ in range(5000 - len(distinct))]
    rng.shuffle(listed)
    rc, res, got = drop_sync(ix, L.DROP_IN, listed, 8)
    rows, inv, soft, n = m.drop(L.DROP_IN, listed)
    assert rc == 0 and (res.n_fids, res.fits, res.overflow) == (4, 1, 0) and list(rows) == [3, 5, 7, 9]
    assert rows_of(got, 4) == rows and (got[4:] == SENT).all()
    assert (res.invalid, res.soft_deleted) == (inv, soft) == (4, 12)
    assert ix.stats().live == st.live - n == 12
    check_state(ix, m)
    ix.close()


# 7. row capacity ----------------------------------------------------------------------------------------------
def test_row_capacity_never_limits_the_drop(ctx):
    ix, m = small_table(ctx)
    st = ix.stats()
    rc, res, got = drop_sync(ix, L.DROP_IN, [3, 5, 7], 2)
    rows, inv, soft, n = m.drop(L.DROP_IN, [3, 5, 7])
    assert rc == 0 and (res.fits, res.overflow, res.n_fids) == (0, 0, 3)
    assert (got == SENT).all()
    assert (res.count, res.bytes, res.span) == tuple(sum(r[i] for r in rows.values()) & U64 for i in range(3))
    assert (res.invalid, res.soft_deleted) == (inv, soft)
    assert ix.stats().live == st.live - n
    check_state(ix, m)
    # totals only: no row buffer at all
    rc, res, got = drop_sync(ix, L.DROP_IN, [9], 0)
    rows, inv, soft, n9 = m.drop(L.DROP_IN, [9])
    assert rc == 0 and (res.fits, res.overflow, res.n_fids) == (0, 0, 1)
    assert (res.count, res.bytes, res.span) == tuple(rows[9])
    assert ix.stats().live == st.live - n - n9 == 12
    check_state(ix, m)
    # an index with nothing to report fits a NULL row buffer
    rc, res, got = drop_sync(ix, L.DROP_IN, [9], 0)
    assert rc == 0 and (res.fits, res.n_fids, res.soft_deleted) == (1, 0, 12)
    ix.close()


# 8. stream order --------------------------------------------------------------------------------------------------
def test_stream_order(ctx):
    ix = Index(ctx, keys=1 << 12)
    m = Model()
    n = 1000
    keys = [key_of(i) for i in range(n)]
    d_rows, d_res = D.DevBuf(8 * ROW, fill=0x5A), D.DevBuf(C.sizeof(L.UsageResult), fill=0x5A)
    fa = np.array([6], dtype=np.uint64)
    m.apply(ix, [L.IDX_PUT] * n, keys, [(6, 8)[i % 2] for i in range(n)], [40 + 10 * i for i in range(n)], [9] * n)
    rc = L.lib.bcw_index_drop_fids_async(ix.handle, L.DROP_IN, fa.ctypes.data_as(L.u64p), 1, d_rows.vp(), 8,
                                         d_res.vp())
    fa[0] = 8  # the list was copied before the call returned
    rows, inv, soft, dropped = m.drop(L.DROP_IN, [6])
    m.apply(ix, [L.IDX_PUT], [keys[10]], [6], [4040], [17])  # a dropped key, back into the dropped fid
    assert rc == 0
    ctx.sync()
    res = L.UsageResult.from_buffer_copy(d_res.download().tobytes()[:C.sizeof(L.UsageResult)])
    got = d_rows.download().view(np.uint64).reshape(-1, 4)
    assert (res.n_fids, res.fits, res.overflow, res.count) == (1, 1, 0, 500) and rows_of(got, 1) == rows
    assert (got[1:] == SENT).all()
    assert m.d[keys[10]][:3] == (6, 4040, 17) and dropped == 500
    check_state(ix, m)
    assert ix.stats().live == 501 and ix.export(fids=[6]) == {keys[10]: (6, 4040, 17)}
    ix.close()


# 9. the space comes back ------------------------------------------------------------------------------------------
def test_reclaim_after_a_drop(ctx):
    ix = Index(ctx, keys=1024)
    ix.compact(shrink=True)  # 1024 slots, 1 MiB of arena, host bounds at zero: _RoomReplay's start
    m = Model()
    rp, grown = _RoomReplay(), _RoomReplay()
    keys = [key_of(i) for i in range(800)]
    kb, eb = sum(len(k) for k in keys[:600]), sum(_entry_bytes(k) for k in keys[:600])
    m.apply(ix, [L.IDX_PUT] * 600, keys[:600], [1 if i < 400 else 2 for i in range(600)],
            [40 + i for i in range(600)], [5] * 600)
    for r in (rp, grown):
        r.batch(600, kb, 600, eb, 0, 0)
    assert rp.cap == 1024 and ix.stats().slot_capacity == 1024
    got, dropped = do_drop(ix, m, L.DROP_IN, [1])
    assert dropped == 400  # at least half of the 600 claimed slots
    # 200 new keys do not fit the host bounds (800 > 0.7 * 1024): the counters are read, half the claimed slots are
    # dead, the index is rebuilt at its capacity and does not grow. Without the drop the same batch doubles the table.
    kb2, eb2 = sum(len(k) for k in keys[600:]), sum(_entry_bytes(k) for k in keys[600:])
    live_bytes = sum(_entry_bytes(k) for k in m.d)
    rp.batch(200, kb2, 200, eb2, 200, live_bytes)
    grown.batch(200, kb2, 200, eb2, 600, eb)
    assert (rp.cap, rp.rebuilds) == (1024, 1) and (grown.cap, grown.rebuilds) == (2048, 0)
    m.apply(ix, [L.IDX_PUT] * 200, keys[600:], [3] * 200, [40 + i for i in range(200)], [6] * 200)
    s = ix.stats()
    assert (s.slot_capacity, s.arena_capacity) == (rp.cap, rp.arena_cap) == (1024, 1 << 20)
    assert s.live == s.slots_used == 400 == rp.slots and s.arena_used == rp.arena
    check_state(ix, m)
    # an explicit rebuild after a drop
    do_drop(ix, m, L.DROP_IN, [3])
    assert ix.stats().slots_used == 400 and ix.stats().live == 200
    ix.compact(shrink=True)
    s = ix.stats()
    assert s.slots_used == s.live == 200 and s.arena_used == sum(_entry_bytes(k) for k in m.d)
    check_state(ix, m)
    ix.close()


# 10. the bound stops paying for unreadable keys -----------------------------------------------------------------------
class BoundModel(Model):
    """k_ix_evict's policy on top of the dict model: after every batch each of the 16 shards (murmur3 Sum64 % 16)
    holding more than limited / 16 keys evicts its entries of least seq first"""

    def __init__(self, limited):
        super().__init__()
        self.lim = limited // 16
        self.evicted = 0

    def shards(self):
        by = {s: [] for s in range(16)}
        for k, v in self.d.items():
            by[O.murmur3_sum64(k) & 15].append((v[3], k))
        return by

    def bound(self):
        out = []
        for lst in self.shards().values():
            for _, k in sorted(lst)[:max(len(lst) - self.lim, 0)]:
                self.evicted += 1
                out.append(k)
                del self.d[k]
        return out


def test_bounded_index_after_a_drop(ctx):
    limited = 16 * 8
    ix = Index(ctx, keys=1 << 12)
    ix.set_limit(limited)
    m = BoundModel(limited)
    keys = [key_of(i) for i in range(700)]
    m.apply(ix, [L.IDX_PUT] * 600, keys[:600], [(1, 2)[i % 2] for i in range(600)], [40 + i for i in range(600)],
            [7] * 600)
    m.bound()
    assert all(len(v) == 8 for v in m.shards().values())  # all 16 shards full
    dead = [k for k, v in m.d.items() if v[0] == 1]
    assert 40 <= len(dead) <= 88  # about half the keys under the dead fid
    assert ix.export() == m.export() and ix.stats().evicted == m.evicted
    got, dropped = do_drop(ix, m, L.DROP_IN, [1])
    assert dropped == len(dead)
    readable = dict(m.d)
    room = {s: 8 - len(v) for s, v in m.shards().items()}
    # new keys, no more per shard than the drop made room for: nothing readable has to go
    fresh = []
    for k in keys[600:]:
        s = O.murmur3_sum64(k) & 15
        if room[s] > 0:
            room[s] -= 1
            fresh.append(k)
    assert len(fresh) >= 20
    ev0 = m.evicted
    m.apply(ix, [L.IDX_PUT] * len(fresh), fresh, [3] * len(fresh), [40 + i for i in range(len(fresh))],
            [9] * len(fresh))
    assert m.bound() == [] and m.evicted == ev0
    exp = ix.export()
    assert exp == m.export() and all(exp[k] == v[:3] for k, v in readable.items())
    assert ix.stats().evicted == ev0 and ix.stats().live == len(readable) + len(fresh)
    # a batch past the room: the policy's victims are the model's, least seq first in every shard
    more = [key_of(5000 + i) for i in range(100)]
    m.apply(ix, [L.IDX_PUT] * 100, more, [3] * 100, [40 + i for i in range(100)], [9] * 100)
    assert len(m.bound()) > 0
    assert ix.export() == m.export() and ix.stats().evicted == m.evicted
    ix.close()


# 11. consumers ----------------------------------------------------------------------------------------------------
def _write_async(ix: Index, active: ActiveWal, batch: WriteBatch):
    """bcw_write_records_async with device arrays: (buffers to keep, n, outs)"""
    n = batch.size()
    keys, koff, vals, voff, metas, moff, etags, expire, flags = host = batch.arrays(ETAG)
    dev = [D.upload(a) for a in host]
    outs = [D.DevBuf(8 * n), D.DevBuf(8 * n), D.DevBuf(n), D.DevBuf(8 * n), D.DevBuf(8 * n),
            D.DevBuf(C.sizeof(L.WriteResult))]
    arr = L.WriteBatchArrays(n, dev[0].ptr, dev[1].ptr, keys.nbytes, dev[2].ptr, dev[3].ptr, vals.nbytes, dev[4].ptr,
                             dev[5].ptr, metas.nbytes, dev[6].ptr, dev[7].ptr, dev[8].ptr)
    p = L.WriteParams(active.fid, active.base_time, active.size, NS, ETAG)
    out = L.WriteOut(active.ptr + active.size, active.capacity - active.size, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                     outs[3].ptr, outs[4].ptr)
    rc = L.lib.bcw_write_records_async(ix.handle, C.byref(p), C.byref(arr), C.byref(out), C.c_void_p(outs[5].ptr))
    assert rc == 0
    return dev, n, outs


def test_write_stat_of_dropped_and_kept_keys(ctx):
    ix = Index(ctx, keys=1 << 12)
    m = Model()
    keys = [key_of(i) for i in range(200)]
    m.apply(ix, [L.IDX_PUT] * 200, keys, [3] * 100 + [5] * 100, [40 + 64 * i for i in range(200)],
            [10 + i for i in range(200)])
    do_drop(ix, m, L.DROP_IN, [5])
    active = ActiveWal(11, BASE, 1 << 20, ctx=ctx)
    b = WriteBatch()
    for i in range(90, 110):  # ten kept keys of fid 3, ten dropped keys of fid 5
        b.put(keys[i][:NS], keys[i][NS:], b"v" * 8)
    keep, n, outs = _write_async(ix, active, b)
    ctx.sync()
    wres = L.WriteResult.from_buffer_copy(outs[5].download(C.sizeof(L.WriteResult)).tobytes())
    assert wres.n_written == n == 20 and wres.fits == 1
    found = outs[2].download(n)
    ffid, fbytes = outs[3].download(8 * n).view(np.uint64), outs[4].download(8 * n).view(np.uint64)
    assert found.tolist() == [1] * 10 + [0] * 10
    assert ffid.tolist() == [3] * 10 + [0] * 10
    assert fbytes.tolist() == [10 + i for i in range(90, 100)] + [0] * 10
    assert len(ix.export(fids=[11])) == 20
    active.close()
    ix.close()


def test_get_and_filter_of_a_dropped_file(ctx):
    ix = Index(ctx, keys=1 << 12)
    ws = WalSet(ctx)
    active = ActiveWal(11, BASE, 1 << 20, ctx=ctx)
    other = ActiveWal(12, BASE, 1 << 20, ctx=ctx)
    b, b2 = WriteBatch(), WriteBatch()
    keys = [key_of(i) for i in range(60)]
    for i, k in enumerate(keys):
        (b if i < 50 else b2).put(k[:NS], k[NS:], b"value-%04d" % i)
    ix.write(active, b, walset=ws, ns_size=NS, etag_size=ETAG)
    ix.write(other, b2, walset=ws, ns_size=NS, etag_size=ETAG)
    assert all(not isinstance(r, Exception) for r in ix.get_records(ws, keys, ns_size=NS, etag_size=ETAG))

    def filter_rows(src: ActiveWal):
        """bcw_compact_filter_async over the file's resident image: (keep bytes of the decoded rows, n_done)"""
        cap = 64
        table = D.DevTable(cap)
        d_res, d_ir = D.DevBuf(C.sizeof(L.DecodeResult)), D.DevBuf(C.sizeof(L.IndexResult))
        d_keep = D.DevBuf(cap, fill=0xFF)
        p = L.DecodeParams(src.size, BASE, 40, NS, ETAG, L.MODE_RECORD)
        assert L.lib.bcw_decode_segment_async(ctx.handle, C.c_void_p(src.ptr), C.byref(p), C.byref(table.t),
                                              d_res.vp()) == 0
        assert L.lib.bcw_compact_filter_async(ix.handle, C.c_void_p(src.ptr), C.byref(p), C.byref(table.t), d_res.vp(),
                                              src.fid, d_keep.vp(), d_ir.vp()) == 0
        ctx.sync()
        dres = L.DecodeResult.from_buffer_copy(d_res.download().tobytes()[:C.sizeof(L.DecodeResult)])
        r = L.IndexResult.from_buffer_copy(d_ir.download().tobytes()[:C.sizeof(L.IndexResult)])
        assert r.err_class == 0 and r.n_in == dres.n_records
        return d_keep.download(int(dres.n_records)), int(r.n_done)

    keep, done = filter_rows(active)
    assert done == 50 and (keep == 1).all()
    # the file is deleted: first from the set of resident WALs, then from the index
    ws.remove(11)
    active.walset = None
    g = ix.get_batch(ws, keys, ns_size=NS, etag_size=ETAG)
    assert g.get_status.tolist() == [L.GET_NO_WAL] * 50 + [L.GET_OK] * 10
    recs = ix.get_records(ws, keys, ns_size=NS, etag_size=ETAG)
    assert all(isinstance(r, ErrKeyNotFound) for r in recs[:50]) and recs[55].value == b"value-0055"
    got = ix.drop_fids([11])
    assert list(got) == [11] and got[11].count == 50
    g = ix.get_batch(ws, keys, ns_size=NS, etag_size=ETAG)
    assert g.get_status.tolist() == [L.GET_NOT_FOUND] * 50 + [L.GET_OK] * 10
    recs = ix.get_records(ws, keys, ns_size=NS, etag_size=ETAG)
    assert all(isinstance(r, ErrKeyNotFound) for r in recs[:50]) and recs[55].value == b"value-0055"
    keep, done = filter_rows(active)
    assert done == 0 and len(keep) == 50 and (keep == 0).all()
    keep, done = filter_rows(other)
    assert done == 10 and (keep == 1).all()
    active.close()
    other.close()
    ws.close()
    ix.close()
