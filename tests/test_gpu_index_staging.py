"""GPU tests of the index's host side: the staging layouts of the synchronous entry points at their edges, the
staging buffer's regrow, the export in both phases, the growth of the table, the arena, the walset's device array and
the lookup's block sums, and the drop list's buffers, which are allocated on first use.

Expected values come from a plain dict model of the index (merged key -> (fid, off, size), None for a soft-deleted
key) and, for Get, from the bytes the test itself wrote into the WAL; WalRecordSize comes from the oracle. Calls go
through the C ABI directly where the Python wrappers cannot make the shape (keys passed as a slice whose first offset
is not 0, NULL keys, offsets that run backwards, a caller capacity that is too small)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _oracle as O
import cases
from bitcaskdb_amd import Index, WalSet
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
BASE = cases.BASE
NS_EDGE = (1, 2, 255, 256, 257)   # around k_ix_get's and the batch kernels' 256-key workgroups
KEY_BYTES = (0, 1, 15, 16, 17)    # around the 16-byte padding of the staged key bytes


# ---- the model -----------------------------------------------------------------------------------------------------
class Model(dict):
    """the index's Put / Delete / SoftDelete on a dict, ops applied in order: a Put stores the value, a SoftDelete
    keeps the key with no value, a Delete removes it; each reports what the key held before (WriteStat)"""

    def apply(self, ops, keys, fid, off, size):
        """returns every op's WriteStat: (found, free_fid, free_bytes)"""
        stats = []
        for op, k, f, o, z in zip(ops, keys, fid, off, size):
            old = self.get(k, "absent")
            stats.append((0, 0, 0) if old == "absent" else (1, 0, 0) if old is None else (1, old[0], old[2]))
            if op == L.IDX_PUT:
                self[k] = (int(f), int(o), int(z))
            elif op == L.IDX_SOFT_DELETE:
                self[k] = None
            else:
                self.pop(k, None)
        return stats

    def answer(self, k):
        """Index.Get: (status, value or None)"""
        if k not in self:
            return L.IDX_NOT_FOUND, None
        return (L.IDX_SOFT_DELETED, None) if self[k] is None else (L.IDX_FOUND, self[k])

    def exported(self):
        """what an export holds: every present key, a soft-deleted one with the zero value SoftDelete stores"""
        return {k: v or (0, 0, 0) for k, v in self.items()}


def edge_keys(n: int, total: int):
    """n keys whose lengths add up to `total` bytes: the empty key, and repeated keys, included"""
    lens = [0] * n
    for j in range(total):
        lens[j % n] += 1
    return [bytes(65 + (i * 7 + q) % 50 for q in range(lens[i])) for i in range(n)]


# ---- the C ABI, with keys as a slice of a larger buffer --------------------------------------------------------------
def flat(keys, lead=0):
    """(bytes, offsets): the keys inside a larger buffer, the first offset `lead`"""
    buf = np.frombuffer(b"\xee" * lead + b"".join(keys) + b"\xee" * 3, dtype=np.uint8).copy()
    off = np.full(len(keys) + 1, lead, dtype=np.uint64)
    off[1:] += np.cumsum([len(k) for k in keys], dtype=np.uint64)
    return buf, off


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def raw_apply(ix, ops, keys, fid, off, size, stats=False, lead=0, null_keys=False, koff=None):
    n = len(keys)
    buf, ko = flat(keys, lead)
    koff = ko if koff is None else koff
    ops, fid, off, size = np.ascontiguousarray(ops, dtype=np.uint8), u64(fid), u64(off), u64(size)
    found, ffid, fbytes = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    rc = L.lib.bcw_index_apply_stat(ix.handle, n, None if null_keys else buf.ctypes.data_as(C.c_void_p),
                                    koff.ctypes.data_as(L.u64p), ops.ctypes.data_as(L.u8p), fid.ctypes.data_as(L.u64p),
                                    off.ctypes.data_as(L.u64p), size.ctypes.data_as(L.u64p),
                                    found.ctypes.data_as(L.u8p) if stats else None,
                                    ffid.ctypes.data_as(L.u64p) if stats else None,
                                    fbytes.ctypes.data_as(L.u64p) if stats else None)
    return rc, list(zip(found.tolist(), ffid.tolist(), fbytes.tolist()))


def raw_get(ix, keys, lead=0, null_keys=False, koff=None):
    n = len(keys)
    buf, ko = flat(keys, lead)
    koff = ko if koff is None else koff
    st = np.full(n, 0xAA, dtype=np.uint8)
    fid, off, size = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    rc = L.lib.bcw_index_get(ix.handle, n, None if null_keys else buf.ctypes.data_as(C.c_void_p),
                             koff.ctypes.data_as(L.u64p), fid.ctypes.data_as(L.u64p), off.ctypes.data_as(L.u64p),
                             size.ctypes.data_as(L.u64p), st.ctypes.data_as(L.u8p))
    return rc, st, fid, off, size


def check_get(ix, model, keys, lead=0):
    rc, st, fid, off, size = raw_get(ix, keys, lead)
    assert rc == 0
    for i, k in enumerate(keys):
        want, val = model.answer(k)
        assert int(st[i]) == want, (i, k, int(st[i]), want)
        if val is not None:
            assert (int(fid[i]), int(off[i]), int(size[i])) == val, (i, k)


def raw_get_records(ix, ws, keys, lead=0, cap=1 << 16, null_keys=False, koff=None, buf=None):
    n = len(keys) if koff is None else len(koff) - 1
    if buf is None:
        buf, ko = flat(keys, lead)
        koff = ko if koff is None else koff
    gst, rst = np.full(n, 0xAA, np.uint8), np.zeros(n, np.uint8)
    fid, off, size, pay_off = (np.zeros(n, np.uint64) for _ in range(4))
    pay = np.zeros(max(cap, 1), dtype=np.uint8)
    out = L.GetOut(gst.ctypes.data_as(L.u8p), rst.ctypes.data_as(L.u8p), fid.ctypes.data_as(L.u64p),
                   off.ctypes.data_as(L.u64p), size.ctypes.data_as(L.u64p), pay_off.ctypes.data_as(L.u64p),
                   pay.ctypes.data_as(L.u8p), cap, L.RecordTable())
    p, res = L.GetParams(20, 20, 0, 0), L.GetResult()
    rc = L.lib.bcw_get_records(ix.handle, ws.handle, C.byref(p), n,
                               None if null_keys else buf.ctypes.data_as(C.c_void_p), koff.ctypes.data_as(L.u64p),
                               C.byref(out), C.byref(res))
    return rc, res, gst, fid, off, size, pay_off, pay


def raw_export(ix, fids=(), ecap=None, kcap=None):
    """bcw_index_export_fids once with the given capacities (None: asked for first): (rc, n_out, key_bytes, entries,
    key_off[0])"""
    fa = u64(sorted(set(fids)))
    fp, nf = (fa.ctypes.data_as(L.u64p), int(fa.size)) if fa.size else (None, 0)
    n, kb = C.c_uint64(), C.c_uint64()
    if ecap is None:
        rc = L.lib.bcw_index_export_fids(ix.handle, fp, nf, None, 0, None, None, None, None, 0, C.byref(n), C.byref(kb))
        assert rc in (0, L.E_CAPACITY)
        ecap, kcap = int(n.value), int(kb.value)
    keys = np.zeros(max(kcap, 1), dtype=np.uint8)
    koff = np.full(ecap + 1, 0xFFFF, dtype=np.uint64)
    fid, off, size = (np.zeros(max(ecap, 1), dtype=np.uint64) for _ in range(3))
    rc = L.lib.bcw_index_export_fids(ix.handle, fp, nf, keys.ctypes.data_as(C.c_void_p), kcap,
                                     koff.ctypes.data_as(L.u64p), fid.ctypes.data_as(L.u64p),
                                     off.ctypes.data_as(L.u64p), size.ctypes.data_as(L.u64p), ecap, C.byref(n),
                                     C.byref(kb))
    ent = {}
    if rc == 0:
        kbytes = keys.tobytes()
        ent = {kbytes[int(koff[i]):int(koff[i + 1])]: (int(fid[i]), int(off[i]), int(size[i]))
               for i in range(int(n.value))}
        assert len(ent) == int(n.value), "an exported key came out twice"
    return rc, int(n.value), int(kb.value), ent, int(koff[0])


# ---- staging edges of the sync entry points -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ix(ctx):
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    yield x
    x.close()


@pytest.mark.parametrize("n", NS_EDGE)
def test_apply_and_get_staging_edges(ix, n):
    """bcw_index_apply_stat with and without the WriteStat outputs and bcw_index_get, n keys of 0, 1, 15, 16 and 17 key
    bytes in all, the keys once from offset 0 and once as a slice of a larger buffer"""
    for total in KEY_BYTES:
        keys = edge_keys(n, total)
        assert sum(map(len, keys)) == total
        ix.clear()
        m = Model()
        r = np.arange(n)
        # every key Put, with the WriteStat outputs: repeated keys report the earlier op of the batch
        args = ([L.IDX_PUT] * n, keys, 1 + r % 3, 40 + 8 * r, 10 + r)
        rc, stats = raw_apply(ix, *args, stats=True)
        assert rc == 0 and stats == m.apply(*args), (n, total)
        check_get(ix, m, keys + [b"absent"])
        # a mix of ops without them, the keys as a slice
        args = ([(L.IDX_PUT, L.IDX_DELETE, L.IDX_SOFT_DELETE, L.IDX_PUT, L.IDX_PUT)[i % 5] for i in range(n)], keys,
                5 + r % 2, 1000 + 16 * r, 77 + r)
        rc, _ = raw_apply(ix, *args, lead=5)
        m.apply(*args)
        assert rc == 0
        check_get(ix, m, keys, lead=3)
        check_get(ix, m, keys)
        # and with them again, as a slice: what the mix left is what is found
        args = ([L.IDX_SOFT_DELETE if i % 7 == 3 else L.IDX_PUT for i in range(n)], keys, 9 + r % 4, 40 + r, 1 + r)
        rc, stats = raw_apply(ix, *args, stats=True, lead=17)
        assert rc == 0 and stats == m.apply(*args), (n, total)
        check_get(ix, m, keys, lead=16)
        assert ix.stats().live == len(m), (n, total)


def test_flat_key_refusals_keep_their_codes(ix):
    """NULL keys with key bytes and an offset that runs backwards: BCW_E_INVAL from all three entry points, the index
    unchanged"""
    ix.clear()
    m = Model()
    keys = [b"alpha", b"be", b"gamma-gamma"]
    args = ([L.IDX_PUT] * 3, keys, [1, 2, 3], [40, 80, 120], [11, 12, 13])
    assert raw_apply(ix, *args)[0] == 0
    m.apply(*args)
    before = ix.stats()
    back = flat(keys)[1]
    back[1], back[2] = back[2], back[1]  # 0, 7, 5, 18: runs backwards, first and last as they were
    assert back.tolist() == [0, 7, 5, 18]
    for stats in (False, True):
        assert raw_apply(ix, [L.IDX_DELETE] * 3, keys, [0] * 3, [0] * 3, [0] * 3, stats, null_keys=True)[0] == L.E_INVAL
        assert raw_apply(ix, [L.IDX_DELETE] * 3, keys, [0] * 3, [0] * 3, [0] * 3, stats, koff=back)[0] == L.E_INVAL
    assert raw_get(ix, keys, null_keys=True)[0] == L.E_INVAL
    assert raw_get(ix, keys, koff=back)[0] == L.E_INVAL
    ws = WalSet(ix.ctx)
    try:
        assert raw_get_records(ix, ws, keys, null_keys=True)[0] == L.E_INVAL
        assert raw_get_records(ix, ws, keys, koff=back)[0] == L.E_INVAL
    finally:
        ws.close()
    # NULL keys without key bytes are fine: three times the empty key
    zero = np.zeros(4, dtype=np.uint64)
    rc, st, *_ = raw_get(ix, [b""] * 3, null_keys=True, koff=zero)
    assert rc == 0 and st.tolist() == [L.IDX_NOT_FOUND] * 3
    assert ix.stats() == before
    check_get(ix, m, keys)


@pytest.fixture(scope="module")
def one_file(ctx):
    """a one-file walset: six small records at the head of fid 4, and where each lies"""
    wr = O.Writer(BASE, BASE)
    recs = []
    for i in range(6):
        p = cases.rec(i, 5 + 9 * i)
        recs.append((wr.write(p), p))
    img = wr.data()
    assert len(img) < 32768, "every record in the first block: one fragment each"
    ws = WalSet(ctx)
    ws.add(W.Wal(np.frombuffer(img, dtype=np.uint8), 4, 40, BASE))
    yield ws, recs
    ws.close()


@pytest.mark.parametrize("n", NS_EDGE)
def test_get_records_staging_edges(ix, one_file, n):
    """bcw_get_records with the same key shapes against a one-file walset, two keys in three pointing at a record:
    the n keys alone (n keys, 0 / 1 / 15 / 16 / 17 key bytes), from offset 0 and as a slice, and once with a longer
    absent key after them"""
    ws, recs = one_file
    for total in KEY_BYTES:
        keys = edge_keys(n, total)
        ix.clear()
        m = Model()
        put = [i for i in range(n) if i % 3 != 2]
        args = ([L.IDX_PUT] * len(put), [keys[i] for i in put], [4] * len(put), [recs[i % 6][0] for i in put],
                [len(recs[i % 6][1]) for i in put])
        assert raw_apply(ix, *args)[0] == 0
        m.apply(*args)
        for query, lead in ((keys, 0), (keys, 9), (keys + [b"absent"], 0)):
            rc, res, gst, fid, off, size, pay_off, pay = raw_get_records(ix, ws, query, lead)
            assert rc == 0
            pos = n_found = 0
            for i, k in enumerate(query):
                want, val = m.answer(k)
                assert int(pay_off[i]) == pos, (n, total, i)
                if val is None:
                    assert int(gst[i]) == L.GET_NOT_FOUND, (n, total, i)
                    continue
                assert int(gst[i]) == L.GET_OK and (int(fid[i]), int(off[i]), int(size[i])) == val, (n, total, i)
                rec = next(p for o, p in recs if o == val[1])
                assert pay[pos:pos + val[2]].tobytes() == rec, (n, total, i)
                pos += (val[2] + 15) & ~15
                n_found += 1
            assert (int(res.payload_need), res.fits, int(res.n_found), int(res.n_ok)) == (pos, 1, n_found, n_found)


# ---- staging regrow --------------------------------------------------------------------------------------------------
def test_staging_regrow(ctx):
    """one index, its staging buffer growing under it: get n = 1, apply_stat n = 257, export, get n = 1"""
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    try:
        m = Model()
        check_get(x, m, [b"first"])
        keys = [b"regrow-%04d-" % i + bytes(i % 40) for i in range(257)]
        r = np.arange(257)
        args = ([L.IDX_PUT] * 257, keys, 1 + r % 5, 40 + 100 * r, 60 + r)
        rc, stats = raw_apply(x, *args, stats=True)
        assert rc == 0 and stats == m.apply(*args)
        rc, n, kb, ent, _ = raw_export(x)
        assert rc == 0 and ent == m.exported() and (n, kb) == (257, sum(map(len, keys)))
        check_get(x, m, [keys[200]])
        check_get(x, m, [b"first"])
    finally:
        x.close()


# ---- export ----------------------------------------------------------------------------------------------------------
def test_export_empty_index(ctx):
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    try:
        for fids in ((), (1, 2)):
            rc, n, kb, ent, koff0 = raw_export(x, fids, ecap=4, kcap=64)
            assert (rc, n, kb, ent, koff0) == (0, 0, 0, {}, 0)
    finally:
        x.close()


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_export_live_entries(ctx, n):
    """n entries with a value, one soft-deleted key (exported with the zero value, so n + 1 entries without a fid list
    and n with the list of every fid) and one deleted key (k_ix_count's blocks are 256 slots, so the entries sit on
    their edge by count, not by slot); a fid list that selects none, some and all of them; a caller capacity one entry
    or one key byte short"""
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    try:
        m = Model()
        keys = [b"exp-%05d" % i + b"x" * (i % 19) for i in range(n)] + [b"soft-deleted", b"deleted"]
        r = np.arange(n + 2)
        args = ([L.IDX_PUT] * (n + 2), keys, 1 + r % 3, 40 + 64 * r, 20 + r)
        assert raw_apply(x, *args)[0] == 0
        m.apply(*args)
        args = ([L.IDX_SOFT_DELETE, L.IDX_DELETE], keys[n:], [0, 0], [0, 0], [0, 0])
        assert raw_apply(x, *args)[0] == 0
        m.apply(*args)
        live = m.exported()
        assert len(live) == n + 1 and live[b"soft-deleted"] == (0, 0, 0)
        for fids in ((), (99,), (0,), (1,), (2, 3), (1, 2, 3), (3, 2, 1, 99, 1), (0, 1, 2, 3)):
            want = {k: v for k, v in live.items() if not fids or v[0] in fids}
            assert len(want) == {(): n + 1, (99,): 0, (0,): 1, (1, 2, 3): n, (0, 1, 2, 3): n + 1}.get(fids, len(want))
            rc, cnt, kb, ent, _ = raw_export(x, fids)
            assert rc == 0 and ent == want, (n, fids)
            assert (cnt, kb) == (len(want), sum(map(len, want))), (n, fids)
            assert x.export(fids or None) == want
        total = sum(map(len, live))
        for ecap, kcap in ((n, total), (n + 1, total - 1), (0, 0)):
            rc, cnt, kb, _, _ = raw_export(x, (), ecap=ecap, kcap=kcap)
            assert (rc, cnt, kb) == (L.E_CAPACITY, n + 1, total), (n, ecap, kcap)
        rc, cnt, kb, ent, _ = raw_export(x, (), ecap=n + 1, kcap=total)  # exactly enough
        assert rc == 0 and ent == live
    finally:
        x.close()


# ---- growth ----------------------------------------------------------------------------------------------------------
def test_growth_from_the_minimum_size(ctx):
    """1 024 keys and 1 MiB of arena hold one batch of 1 000 keys of 600 bytes, not two: at a load of 0.7 the table
    (2 048 slots) doubles for the second and for the third batch, and the arena (16 + 608 bytes an entry) for the
    second"""
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    try:
        m = Model()
        caps = []
        for b in range(3):
            keys = [b"grow-%d-%04d-" % (b, i) + bytes((i + q) & 0xff for q in range(588)) for i in range(1000)]
            assert all(len(k) == 600 for k in keys)
            r = np.arange(1000)
            args = ([L.IDX_PUT] * 1000, keys, [b + 1] * 1000, 40 + 700 * r, 650 + r % 7)
            assert raw_apply(x, *args)[0] == 0
            m.apply(*args)
            s = x.stats()
            caps.append((s.slot_capacity, s.arena_capacity))
            assert s.live == len(m) == 1000 * (b + 1) and s.overflow == 0
            check_get(x, m, list(m) + [b"grow-absent"])
        assert caps == [(2048, 1 << 20), (4096, 2 << 20), (8192, 2 << 20)]
        x.compact(shrink=True)
        s = x.stats()
        assert s.live == 3000 and s.slot_capacity == 8192 and s.arena_capacity < 2 << 20
        check_get(x, m, list(m) + [b"grow-absent"])
        assert x.export() == m.exported()
    finally:
        x.close()


# ---- walset growth ---------------------------------------------------------------------------------------------------
def test_walset_growth(ctx):
    """17 files, past the 16 entries the set's device array begins with; then one get of 256 * 1024 + 1 keys, past the
    1 024 lookup blocks the set's block sums begin with"""
    x, ws = Index(ctx, keys=1024, arena_bytes=1 << 20), WalSet(ctx)
    try:
        m, recs = Model(), {}
        for fid in range(1, 18):
            wr = O.Writer(BASE, BASE)
            p = cases.rec(fid, 10 + fid)
            recs[fid] = (wr.write(p), p)
            ws.add(W.Wal(np.frombuffer(wr.data(), dtype=np.uint8), fid, 40, BASE))
        assert len(ws) == 17
        keys = [b"file-%02d" % fid for fid in recs]
        args = ([L.IDX_PUT] * 17, keys, list(recs), [recs[f][0] for f in recs], [len(recs[f][1]) for f in recs])
        assert raw_apply(x, *args)[0] == 0
        m.apply(*args)
        rc, res, gst, fid, off, size, pay_off, pay = raw_get_records(x, ws, [keys[0], keys[16], b"absent"])
        assert rc == 0 and gst.tolist() == [L.GET_OK, L.GET_OK, L.GET_NOT_FOUND] and fid.tolist()[:2] == [1, 17]
        for i, f in enumerate((1, 17)):
            assert (int(off[i]), int(size[i])) == (recs[f][0], len(recs[f][1]))
            assert pay[int(pay_off[i]):int(pay_off[i]) + int(size[i])].tobytes() == recs[f][1]
        n = 256 * 1024 + 1
        buf, koff = np.full(n, ord("?"), dtype=np.uint8), np.arange(n + 1, dtype=np.uint64)
        rc, res, gst, *_ = raw_get_records(x, ws, None, koff=koff, buf=buf, cap=16)
        assert rc == 0 and (gst == L.GET_NOT_FOUND).all()
        assert (int(res.payload_need), res.fits, int(res.n_found), int(res.n_ok)) == (0, 1, 0, 0)
        rc, res, gst, *_ = raw_get_records(x, ws, [keys[16]])  # the grown buffers serve the next get
        assert rc == 0 and gst.tolist() == [L.GET_OK]
    finally:
        ws.close()
        x.close()


# ---- the buffers allocated on first use ---------------------------------------------------------------------------
# (the rules' table and counters: test_gpu_rules.py::test_rules_clear_and_reset sets, clears and sets them again)
def test_two_drops_in_a_row(ctx):
    """the drop list's pinned buffer, device copy and event are allocated by the first drop; the second call waits for
    the first one's copy out of the pinned list. Both report, and leave, what the model says"""
    x = Index(ctx, keys=1024, arena_bytes=1 << 20)
    try:
        m = Model()
        keys = [b"drop-%03d" % i for i in range(300)]
        r = np.arange(300)
        args = ([L.IDX_PUT] * 300, keys, 1 + r % 3, 40 + 50 * r, 20 + r % 9)
        assert raw_apply(x, *args)[0] == 0
        m.apply(*args)
        for fids in ((2,), (3, 7)):
            gone = {k: v for k, v in m.items() if v[0] in fids}
            want = {f: (sum(v[0] == f for v in gone.values()), sum(v[2] for v in gone.values() if v[0] == f),
                        sum(O.wal_record_size(v[1], v[2]) for v in gone.values() if v[0] == f))
                    for f in fids if any(v[0] == f for v in gone.values())}
            got = x.drop_fids(fids)
            assert {f: tuple(u) for f, u in got.items()} == want and (got.soft_deleted, got.invalid) == (0, 0)
            for k in gone:
                del m[k]
            check_get(x, m, keys)
            assert x.stats().live == len(m)
        assert len(m) == 100
    finally:
        x.close()
