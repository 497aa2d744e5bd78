"""GPU tests of the per-WAL space accounting (bcw_index_fid_usage*, bcw_freed_by_fid_async, csrc/bcw_usage.hip and
k_ix_usage): every result is compared with a Python dict built from Index.export(), the span from
bcw_wal_record_size (the reference's loop, oracle-tested in test_capi.py). The index here is a few thousand keys in a
table of several workgroups; the fid counts walk the reduction's paths: one fid for every lane, a handful (wave
rounds), more than a wave holds, more than a workgroup's LDS table holds (rows go to the global table directly), the
cap itself, and one more than the cap. No size above 2^20 reaches the device (tools/usage_check.cpp covers those)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import _devmem as D
from bitcaskdb_amd import ActiveWal, FidUsage, Index, WriteBatch, load_wal, recover_from_wals, wal_garbage
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W
from bitcaskdb_amd._hip import DevMem

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
BASE = 1_700_000_000
BLOCK = 32768
SENT = 0x5A5A5A5A5A5A5A5A
ROW = C.sizeof(L.FidUsageRow)


def span(off: int, size: int) -> int:
    return int(L.lib.bcw_wal_record_size(off, size))


def model(ix: Index):
    """({fid: FidUsage}, soft_deleted, invalid) of the index's live entries"""
    rows, soft, inv = {}, 0, 0
    for fid, off, size in ix.export().values():
        if off == 0:
            soft += 1
        elif off < 40:
            inv += 1
        else:
            c, b, s = rows.get(fid, (0, 0, 0))
            rows[fid] = (c + 1, (b + size) & (2 ** 64 - 1), (s + span(off, size)) & (2 ** 64 - 1))
    return {f: FidUsage(*v) for f, v in rows.items()}, soft, inv


def check(ix: Index):
    """fid_usage equals the model, rows ascending, and the call leaves the index as it was"""
    before, st = ix.export(), ix.stats()
    rows, soft, inv = model(ix)
    u = ix.fid_usage()
    assert list(u) == sorted(u)
    assert dict(u) == rows
    assert (u.soft_deleted, u.invalid) == (soft, inv)
    assert ix.export() == before and ix.stats() == st
    return u


def usage_sync(ix: Index, cap: int):
    """bcw_index_fid_usage with the row buffer pre-filled"""
    rows = np.full(4 * max(cap, 1), SENT, dtype=np.uint64)
    res = L.UsageResult()
    rc = L.lib.bcw_index_fid_usage(ix.handle, C.cast(rows.ctypes.data, C.POINTER(L.FidUsageRow)) if cap else None,
                                   cap, C.byref(res))
    return rc, res, rows.reshape(-1, 4)


def key_of(i: int) -> bytes:
    return (b"ns-%03d-" % (i % 7) * 4)[:NS] + b"key-%06d" % i


def fill(ix: Index, n: int, fids, seed: int, churn: bool = True):
    """n keys, key i in fids[i % len(fids)], random offsets and sizes; then (churn) random Delete / SoftDelete / Put
    over the keys beyond the first len(fids), so that every fid keeps at least one counted key"""
    rng = random.Random(seed)
    keys = [key_of(i) for i in range(n)]

    def val():
        return 40 + rng.randrange(1 << 32), rng.choice([0, 1, 100, 4096, 32761, 70000, rng.randrange(1 << 20)])
    vals = [val() for _ in range(n)]
    ix.apply([L.IDX_PUT] * n, keys, [fids[i % len(fids)] for i in range(n)], [v[0] for v in vals],
             [v[1] for v in vals])
    if churn and n > len(fids):
        m = n // 2
        pick = [rng.randrange(len(fids), n) for _ in range(m)]
        ops = [rng.choice([L.IDX_PUT, L.IDX_PUT, L.IDX_DELETE, L.IDX_SOFT_DELETE]) for _ in range(m)]
        vals = [val() for _ in range(m)]
        ix.apply(ops, [keys[i] for i in pick], [fids[rng.randrange(len(fids))] for _ in range(m)],
                 [v[0] for v in vals], [v[1] for v in vals])
    return keys


def some_fids(k: int, seed: int):
    rng = random.Random(seed)
    out = set()
    while len(out) < k:
        out.add(rng.choice([rng.randrange(1, 5000), rng.randrange(1, 2 ** 64)]))
    return sorted(out)


@pytest.fixture()
def ix(ctx):
    x = Index(ctx, keys=1 << 12)
    yield x
    x.close()


# 1. random Put / Delete / SoftDelete, by number of distinct fids -----------------------------------------
@pytest.mark.parametrize("nfids", [1, 3, 70, 300, 600, 1500, 4096])
def test_random_ops(ix, nfids):
    fill(ix, 6000, some_fids(nfids, nfids), seed=nfids)
    u = check(ix)
    assert len(u) == nfids and u.soft_deleted > 0
    assert ix.stats().slot_capacity >= 4 * 256  # more than one workgroup round


# 2. the extreme fids --------------------------------------------------------------------------------------
def test_fid_zero_and_max(ix):
    fill(ix, 3000, [0, 2 ** 64 - 1, 7], seed=2)
    u = check(ix)
    assert list(u) == [0, 7, 2 ** 64 - 1]
    ix.clear()
    fill(ix, 500, [0], seed=3)
    assert list(check(ix)) == [0]
    ix.clear()
    fill(ix, 500, [2 ** 64 - 1], seed=4)
    assert list(check(ix)) == [2 ** 64 - 1]


# 3. span geometry -----------------------------------------------------------------------------------------
def test_span_geometry(ix):
    keys, fid, off, size = [], [], [], []
    for left in range(0, 9):  # bytes the record's offset leaves in its block (0: the block's first byte)
        o = 40 + 3 * BLOCK - left
        lo = BLOCK if left < 7 else left
        for s in (0, 1, lo - 7, lo - 6, 32761, 32762, 100000):
            keys.append(key_of(len(keys)))
            fid.append(5 + left % 2)
            off.append(o)
            size.append(s)
    keys.append(key_of(len(keys)))  # a present entry inside the super block: no writer produces it
    fid.append(5)
    off.append(17)
    size.append(100)
    ix.apply([L.IDX_PUT] * len(keys), keys, fid, off, size)
    u = check(ix)
    assert u.invalid == 1 and u.soft_deleted == 0
    assert sum(r.count for r in u.values()) == len(keys) - 1
    # the pad is counted: 3 bytes left in the block, one payload byte
    assert span(40 + BLOCK - 3, 1) == 3 + 7 + 1


# 4. index states ------------------------------------------------------------------------------------------
def test_empty_and_all_deleted(ix):
    u = check(ix)
    assert dict(u) == {} and (u.soft_deleted, u.invalid) == (0, 0)
    keys = fill(ix, 2000, [3, 4], seed=5, churn=False)
    assert len(check(ix)) == 2
    ix.apply([L.IDX_DELETE] * len(keys), keys)
    u = check(ix)
    assert dict(u) == {} and ix.stats().live == 0


def test_after_compact_shrink_and_growth(ctx):
    x = Index(ctx, keys=1024)  # 2048 slots: 6000 keys grow it twice
    cap0 = x.stats().slot_capacity
    keys = fill(x, 6000, some_fids(9, 1), seed=6)
    assert x.stats().slot_capacity > cap0
    u = check(x)
    x.apply([L.IDX_DELETE] * 5000, keys[1000:])
    x.compact(shrink=True)
    assert x.stats().slot_capacity < 8192
    u2 = check(x)
    assert sum(r.count for r in u2.values()) < sum(r.count for r in u.values())
    x.close()


def test_bounded_index_counts_no_evicted_key(ix):
    ix.set_limit(1600)
    fill(ix, 6000, some_fids(5, 2), seed=7)
    st = ix.stats()
    assert st.evicted > 0
    u = check(ix)
    assert sum(r.count for r in u.values()) + u.soft_deleted + u.invalid == st.live


# 5. capacity ----------------------------------------------------------------------------------------------
def test_row_capacity(ix):
    fill(ix, 3000, some_fids(40, 3), seed=8)
    rows, soft, inv = model(ix)
    rc, res, got = usage_sync(ix, 39)
    assert rc == L.E_CAPACITY and res.fits == 0 and res.overflow == 0 and res.n_fids == 40
    assert (got == SENT).all()
    assert (res.count, res.bytes, res.span) == tuple(sum(r[i] for r in rows.values()) for i in range(3))
    rc, res, got = usage_sync(ix, 0)
    assert rc == L.E_CAPACITY and res.fits == 0 and res.n_fids == 40
    rc, res, got = usage_sync(ix, int(res.n_fids))
    assert rc == 0 and res.fits == 1 and res.n_fids == 40 and (res.soft_deleted, res.invalid) == (soft, inv)
    assert {int(r[0]): FidUsage(int(r[1]), int(r[2]), int(r[3])) for r in got} == rows
    assert got[:, 0].tolist() == sorted(rows)


def test_more_fids_than_the_cap(ix):
    keys = fill(ix, 5000, some_fids(L.USAGE_MAX_FIDS + 1, 4), seed=9, churn=False)
    before = ix.get_many(keys)
    rc, res, got = usage_sync(ix, L.USAGE_MAX_FIDS + 1)
    assert rc == L.E_CAPACITY and res.overflow == 1 and res.fits == 0
    assert (got == SENT).all()
    with pytest.raises(RuntimeError, match="distinct fids"):
        ix.fid_usage()
    after = ix.get_many(keys)
    assert all((a == b).all() for a, b in zip(before, after))
    # one key less and the same index fits again
    ix.apply([L.IDX_DELETE], [keys[L.USAGE_MAX_FIDS]])
    assert len(check(ix)) == L.USAGE_MAX_FIDS


# 6. ordering: queued behind a write on the same stream, no synchronisation in between ------------------------
def _write_async(ix: Index, active: ActiveWal, batch: WriteBatch):
    """bcw_write_records_async with device arrays, not synchronised: (buffers to keep, n, outs)"""
    n = batch.size()
    keys, koff, vals, voff, metas, moff, etags, expire, flags = host = batch.arrays(ETAG)
    dev = [DevMem(a.nbytes).upload(a) for a in host]
    outs = [DevMem(8 * n), DevMem(8 * n), DevMem(n), DevMem(8 * n), DevMem(8 * n), DevMem(C.sizeof(L.WriteResult))]
    arr = L.WriteBatchArrays(n, dev[0].ptr, dev[1].ptr, keys.nbytes, dev[2].ptr, dev[3].ptr, vals.nbytes, dev[4].ptr,
                             dev[5].ptr, metas.nbytes, dev[6].ptr, dev[7].ptr, dev[8].ptr)
    p = L.WriteParams(active.fid, active.base_time, active.size, NS, ETAG)
    out = L.WriteOut(active.ptr + active.size, active.capacity - active.size, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                     outs[3].ptr, outs[4].ptr)
    rc = L.lib.bcw_write_records_async(ix.handle, C.byref(p), C.byref(arr), C.byref(out), C.c_void_p(outs[5].ptr))
    assert rc == 0
    return dev, n, outs


def test_async_after_write_sees_the_batch(ctx):
    x = Index(ctx, keys=1024)
    active = ActiveWal(11, BASE, 4 << 20, ctx=ctx)
    x.apply([L.IDX_PUT] * 300, [key_of(i) for i in range(300)], [4] * 300, [40 + 50 * i for i in range(300)],
            [30] * 300)
    cap0 = x.stats().slot_capacity
    b = WriteBatch()
    for i in range(200, 3200):  # 100 overwrites of fid 4's keys, 2900 new keys: the index grows inside the call
        b.put(key_of(i)[:NS], key_of(i)[NS:], b"v" * (i % 50))
    d_rows, d_res = D.DevBuf(64 * ROW, fill=0x5A), D.DevBuf(C.sizeof(L.UsageResult))
    keep, n, outs = _write_async(x, active, b)
    rc = L.lib.bcw_index_fid_usage_async(x.handle, d_rows.vp(), 64, d_res.vp())
    assert rc == 0
    ctx.sync()
    wres = L.WriteResult.from_buffer_copy(outs[5].download(C.sizeof(L.WriteResult)).tobytes())
    assert wres.n_written == n and wres.fits == 1
    res = L.UsageResult.from_buffer_copy(d_res.download().tobytes()[:C.sizeof(L.UsageResult)])
    assert res.fits == 1 and res.overflow == 0 and res.n_fids == 2
    got = d_rows.download().view(np.uint64).reshape(-1, 4)
    rows, _, _ = model(x)
    assert x.stats().slot_capacity > cap0
    assert {int(r[0]): FidUsage(int(r[1]), int(r[2]), int(r[3])) for r in got[:2]} == rows
    assert rows[4].count == 200 and rows[11].count == 3000
    assert (got[2:] == SENT).all()
    active.close()
    x.close()


# 7. the freed-bytes map of a write ------------------------------------------------------------------------
def _three_batches():
    rng = random.Random(12)
    out = []
    for k in range(3):
        b = WriteBatch()
        for j in range(400):
            i = rng.randrange(700)  # repeated keys inside a batch and across batches
            ns, key = key_of(i)[:NS], key_of(i)[NS:]
            r = rng.randrange(10)
            if r == 0:
                b.delete(ns, key)
            elif r == 1:
                b.put(ns, key, b"", W.Meta(flags=1))  # a tombstone: SoftDelete
            else:
                b.put(ns, key, rng.randbytes(rng.choice([0, 5, 300, 40000 if j % 97 == 0 else 64])))
        out.append(b)
    return out


def test_stats_on_device_equal_the_host_loop(ctx):
    twins = []
    for on in (False, True):
        x = Index(ctx, keys=1 << 12)
        # keys that live under other fids before the first batch
        x.apply([L.IDX_PUT] * 300, [key_of(i) for i in range(300)], [20 + i % 6 for i in range(300)],
                [40 + 100 * i for i in range(300)], [10 + i for i in range(300)])
        active = ActiveWal(9, BASE, 1 << 16, ctx=ctx)
        res = [x.write(active, b, ns_size=NS, etag_size=ETAG, stats_on_device=on) for b in _three_batches()]
        twins.append((res, active.bytes(), x.export()))
        assert x.write(active, WriteBatch(), stats_on_device=on) == ([], {})
        bad = WriteBatch()
        bad.put(key_of(1)[:NS], b"k", b"v", W.Meta(expire=BASE - 1))
        with pytest.raises(W.WalError, match="invalid expire"):
            x.write(active, bad, ns_size=NS, etag_size=ETAG, stats_on_device=on)
        assert x.export() == twins[-1][2]
        active.close()
        x.close()
    (res_a, img_a, ent_a), (res_b, img_b, ent_b) = twins
    assert res_a == res_b and img_a == img_b and ent_a == ent_b
    stats = [s for _, s in res_a]
    assert all(0 in s for s in stats)  # the ops that freed nothing: fid 0
    assert any(f >= 20 for f in stats[0]) and 9 in stats[1]  # values under other fids, then under the active WAL


def test_freed_map_of_a_rejected_batch_is_empty(ctx):
    x = Index(ctx, keys=1 << 12)
    active = ActiveWal(9, BASE, 1 << 20, ctx=ctx)
    bad = WriteBatch()
    for i in range(500):
        bad.put(key_of(i)[:NS], key_of(i)[NS:], b"v", W.Meta(expire=BASE - 1 if i == 250 else 0))
    keep, n, outs = _write_async(x, active, bad)
    d_rows, d_res = D.DevBuf(8 * ROW, fill=0x5A), D.DevBuf(C.sizeof(L.UsageResult), fill=0x5A)
    # the rejected batch left its WriteStat columns unwritten: the gate keeps them from being read
    rc = L.lib.bcw_freed_by_fid_async(x.handle, n, C.c_void_p(outs[2].ptr), C.c_void_p(outs[3].ptr),
                                      C.c_void_p(outs[4].ptr), C.c_void_p(outs[5].ptr), d_rows.vp(), 8, d_res.vp())
    assert rc == 0
    ctx.sync()
    wres = L.WriteResult.from_buffer_copy(outs[5].download(C.sizeof(L.WriteResult)).tobytes())
    assert wres.n_written == 0 and wres.err_class == L.ENC_ERR_EXPIRE and wres.err_record == 250
    res = L.UsageResult.from_buffer_copy(d_res.download().tobytes()[:C.sizeof(L.UsageResult)])
    assert (res.n_fids, res.fits, res.overflow, res.count, res.bytes, res.span) == (0, 1, 0, 0, 0, 0)
    assert (d_rows.download().view(np.uint64) == SENT).all()
    # without a gate, and with columns that hold something, the same call groups all n ops
    found, ffid, fbytes = np.ones(n, np.uint8), np.arange(n, dtype=np.uint64) % 3, np.full(n, 7, np.uint64)
    found[::5] = 0
    bufs = [D.upload(a) for a in (found, ffid, fbytes)]
    rc = L.lib.bcw_freed_by_fid_async(x.handle, n, bufs[0].vp(), bufs[1].vp(), bufs[2].vp(), None, d_rows.vp(), 8,
                                      d_res.vp())
    assert rc == 0
    ctx.sync()
    res = L.UsageResult.from_buffer_copy(d_res.download().tobytes()[:C.sizeof(L.UsageResult)])
    got = d_rows.download().view(np.uint64).reshape(-1, 4)
    assert (res.n_fids, res.fits, res.count, res.bytes, res.span) == (3, 1, int(found.sum()), 7 * n, 0)
    for f in range(3):
        assert got[f].tolist() == [f, int(found[ffid == f].sum()), 7 * int((ffid == f).sum()), 0]
    active.close()
    x.close()


# 8. end to end: the garbage of two WAL files, and again after recovery ------------------------------------
def test_wal_garbage_and_recovery(ctx):
    x = Index(ctx, keys=1 << 12)
    rng = random.Random(13)
    wals = []
    for fid in (3, 4):
        active = ActiveWal(fid, BASE, 1 << 16, ctx=ctx)
        for _ in range(2):
            b = WriteBatch()
            for j in range(300):
                i = rng.randrange(400)  # overwrites inside a batch, across batches and across the two files
                b.put(key_of(i)[:NS], key_of(i)[NS:], rng.randbytes(rng.choice([1, 200, 3000, 33000])))
            x.write(active, b, ns_size=NS, etag_size=ETAG)
        wals.append(active)
    g = wal_garbage(x, wals)
    assert g == wal_garbage(x, {w.fid: w.size for w in wals})
    rows, _, _ = model(x)
    assert g == {w.fid: w.size - 40 - rows[w.fid].span for w in wals}
    assert all(0 < g[w.fid] < w.size - 40 for w in wals)  # overwritten records and pads; live records remain
    # every record of file 3 that a later write replaced is garbage there: the live spans of both files together
    # are the footprints of the keys' last records
    assert sum(r.count for r in rows.values()) == len(x.export())
    y = Index(ctx, keys=1 << 12)
    recover_from_wals(y, {w.fid: (load_wal(w.bytes(), w.fid), None) for w in wals}, NS, ETAG)
    assert y.export() == x.export()
    assert wal_garbage(y, wals) == g
    for w in wals:
        w.close()
    x.close()
    y.close()
