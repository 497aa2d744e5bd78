"""GPU parity of the batched Write (bcw_write_records*, DBImpl.Write's writeWal + writeIndex, db_impl.go:434-480)
against the oracle: O.record_encode (Record.Encode) fed to O.Writer(at=wal_pos) (Wal.WriteRecord) for the bytes and the
locs, O.Index / O.SMap.index_op for the index and the WriteStat columns, O.decode and the library's own decode and
Get for the round trip.

One batch of ~400 records carries every shape: values of 0 .. 200 000 bytes (the last in Middle fragments), values
that fill their block exactly and that length +-1, user keys of 0 .. 300 bytes, with and without etag, expire and
meta, tombstones and Batch.Delete records. It is rebuilt for every start position, since the exact fills depend on it."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import _devmem as D
import _oracle as O
from bitcaskdb_amd import ActiveWal, ErrKeyNotFound, ErrKeySoftDeleted, Index, WalSet, WriteBatch
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
BASE = 1_700_000_000
BLOCK = 32768
FID = 9
FILL = 0xA5
SENT = 0x5A5A5A5A5A5A5A5A
VAL_LENS = [0, 1, 15, 16, 17, 127, 128, 4096]
BIG = {40: 40000, 110: 70000, 180: 200000, 260: 40000, 330: 70000}
KEY_LENS = [0, 1, 127, 128, 300]
META = b"\x81\xa3foo\xa3bar"
# start positions: a fresh file, and positions that leave 0, 3, 6, 7, 8 and 20 bytes in the block
POSITIONS = [40] + [40 + 2 * BLOCK - left for left in (0, 3, 6, 7, 8, 20)]


class Built:
    """a WriteBatch and what the oracle makes of it from file position pos"""

    def __init__(self, pos: int, ns_size: int = NS, etag_size: int = ETAG):
        self.pos, self.ns_size, self.etag_size = pos, ns_size, etag_size
        self.batch = WriteBatch()
        self.w = O.Writer(BASE, BASE, at=pos)
        self.locs = []
        self.ops = []  # (ns, key, op) in batch order

    def left(self) -> int:
        return BLOCK - (self.w.size() - 40) % BLOCK

    def put(self, ns, key, val, etag=b"", expire=0, tomb=False, meta=b""):
        p = O.record_encode(ns, key, val, etag, expire, tomb, meta, BASE)
        self.locs.append((self.w.write(p), len(p)))
        self.batch.put(ns, key, val, W.Meta(expire=expire, etag=etag or None, flags=1 if tomb else 0, app_meta=meta))
        self.ops.append((ns, key, L.IDX_SOFT_DELETE if tomb else L.IDX_PUT))

    def delete(self, ns, key):
        p = O.record_encode(ns, key, b"", b"", 0, True, b"", BASE)
        self.locs.append((self.w.write(p), len(p)))
        self.batch.delete(ns, key)
        self.ops.append((ns, key, L.IDX_DELETE))

    def put_filling(self, ns, key, delta: int):
        """a Put whose payload is the room of the current block + delta"""
        if self.left() < 7 + 400:
            self.put(ns, b"spacer" + key, bytes(1000))
        target = self.left() - 7 + delta
        vl = target - len(O.record_encode(ns, key, b"", b"", 0, False, b"", BASE))
        for _ in range(4):  # the value varint's own length moves the payload length
            vl += target - len(O.record_encode(ns, key, bytes(vl), b"", 0, False, b"", BASE))
        self.put(ns, key, bytes(random.Random(vl).randbytes(vl)))
        assert self.locs[-1][1] == target

    def expect(self):
        return self.w.data(), self.w.size()


def ns_of(i: int, ns_size: int) -> bytes:
    return (b"ns-%03d-" % (i % 7) * 40)[:ns_size]


def full_batch(pos: int, ns_size: int = NS, etag_size: int = ETAG, n: int = 400, big=BIG) -> Built:
    rng = random.Random(pos * 131 + ns_size)
    b = Built(pos, ns_size, etag_size)
    for i in range(n):
        ns = ns_of(i, ns_size)
        key = (b"k%05d-" % i + rng.randbytes(300))[:KEY_LENS[i % 5]] if KEY_LENS[i % 5] else b""
        if i in (30, 150, 250):
            for j, delta in enumerate((0, 1, -1)):  # fills the block exactly; one more; one less
                b.put_filling(ns, b"fill%d-%d" % (i, j), delta)
            continue
        if i % 17 == 16:
            b.delete(ns, key)
            continue
        vl = big.get(i, VAL_LENS[rng.randrange(len(VAL_LENS))])
        variant = rng.randrange(8)
        etag = rng.randbytes(etag_size) if variant & 1 else b""
        expire = BASE + rng.choice([0, 1, 128, 3600, (1 << 35) - 1]) if variant & 2 else 0
        meta = META if variant & 4 else b""
        b.put(ns, key, rng.randbytes(vl), etag, expire, tomb=(i % 23 == 5), meta=meta)
    return b


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


class Out:
    pass


def write_sync(ix: Index, batch: WriteBatch, pos: int, cap: int | None = None, ns_size=NS, etag_size=ETAG, fid=FID,
               stat: bool = True):
    """bcw_write_records with every output pre-filled (0xA5 bytes, sentinel words); stat False: without the WriteStat
    columns (found, free_fid, free_bytes)"""
    keys, koff, vals, voff, metas, moff, etags, expire, flags = arrs = batch.arrays(etag_size)
    n = batch.size()
    if cap is None:
        cap = int(L.lib.bcw_write_bound(n, keys.size, vals.size, metas.size, etag_size, pos))
    o = Out()
    o.wal = np.full(max(cap, 1), FILL, dtype=np.uint8)
    o.rec_off, o.rec_size = np.full(max(n, 1), SENT, np.uint64), np.full(max(n, 1), SENT, np.uint64)
    o.found = np.full(max(n, 1), FILL, np.uint8)
    o.ffid, o.fbytes = np.full(max(n, 1), SENT, np.uint64), np.full(max(n, 1), SENT, np.uint64)
    ba = L.WriteBatchArrays(n, _vp(keys), _vp(koff), keys.size, _vp(vals), _vp(voff), vals.size, _vp(metas), _vp(moff),
                            metas.size, _vp(etags), _vp(expire), _vp(flags))
    p = L.WriteParams(fid, BASE, pos, ns_size, etag_size)
    out = L.WriteOut(_vp(o.wal), cap, _vp(o.rec_off), _vp(o.rec_size),
                     *((_vp(o.found), _vp(o.ffid), _vp(o.fbytes)) if stat else (None, None, None)))
    o.res = L.WriteResult()
    o.rc = L.lib.bcw_write_records(ix.handle, C.byref(p), C.byref(ba), C.byref(out), C.byref(o.res))
    o.keep = arrs
    return o


def assert_written(o: Out, b: Built):
    data, end = b.expect()
    n = b.batch.size()
    assert o.rc == 0 and o.res.err_class == 0 and o.res.err_record == -1 and o.res.fits == 1 and o.res.idx_err == 0
    assert o.res.n_written == n and o.res.wal_end == end and o.res.wal_need == end - b.pos == len(data)
    assert o.rec_off[:n].tolist() == [l[0] for l in b.locs]
    assert o.rec_size[:n].tolist() == [l[1] for l in b.locs]
    got = o.wal[:len(data)].tobytes()
    if got != data:
        bad = next(i for i in range(len(data)) if got[i] != data[i])
        pytest.fail(f"appended bytes differ first at +{bad} (file offset {b.pos + bad}) of {len(data)}")
    assert (o.wal[len(data):] == FILL).all()  # nothing past wal_need (pad bytes inside are the oracle's zeros)


def assert_untouched(o: Out, n: int):
    assert (o.wal == FILL).all()
    assert (o.rec_off[:n] == SENT).all() and (o.rec_size[:n] == SENT).all()


def merged(ops):
    return [ns + k for ns, k, _ in ops]


def oracle_index(b: Built, oix: O.Index | None = None) -> O.Index:
    oix = oix or O.Index()
    for (ns, k, op), (off, size) in zip(b.ops, b.locs):
        oix.set(ns, k, op, FID, off, size)
    return oix


def assert_index(ix: Index, oix: O.Index, ops):
    keys = sorted(set((ns, k) for ns, k, _ in ops))
    st, fid, off, size = ix.get_many([ns + k for ns, k in keys])
    for i, (ns, k) in enumerate(keys):
        est, (ef, eo, ez) = oix.get(ns, k)
        assert st[i] == est, (ns, k)
        if est != L.IDX_NOT_FOUND:
            assert (int(fid[i]), int(off[i]), int(size[i])) == (ef, eo, ez), (ns, k)


@pytest.fixture()
def ix(ctx):
    x = Index(ctx, keys=1 << 12)
    yield x
    x.close()


# 1. byte parity at every start position --------------------------------------------------------------
@pytest.mark.parametrize("pos", POSITIONS)
def test_bytes_match_the_writer(ix, pos):
    b = full_batch(pos)
    assert b.batch.size() >= 400
    o = write_sync(ix, b.batch, pos)
    assert_written(o, b)
    assert_index(ix, oracle_index(b), b.ops)


def test_batch_has_the_shapes():
    """the batch of case 1 holds what it claims (the writer's arithmetic on the oracle's locs): Middle fragments, a
    zero-length First, exact fills, pads"""
    b = full_batch(40 + 2 * BLOCK - 7)
    room = [BLOCK - (o - 40) % BLOCK - 7 for o, _ in b.locs]  # payload bytes the record's first block takes
    assert room[0] == 0 and b.locs[0][0] == b.pos                               # the zero-length First
    assert sum(1 for r, (_, s) in zip(room, b.locs) if s - r > 2 * (BLOCK - 7)) >= 1  # Middle fragments
    assert sum(1 for r, (_, s) in zip(room, b.locs) if s == r) >= 3               # ends its block exactly
    ends = [int(O.wal_record_size(o, s)) + o for o, s in b.locs]
    assert sum(1 for (o, _), e in zip(b.locs[1:], ends) if 0 < o - e < 7) >= 3     # pads before a record


# 2. index parity and WriteStat ---------------------------------------------------------------------------
def test_index_and_write_stats(ix):
    rng = random.Random(2)
    ns = ns_of(0, NS)
    old = [b"old-%03d" % i for i in range(60)]
    ix.apply([L.IDX_PUT] * 60, [ns + k for k in old], [3] * 60, [1000 + 50 * i for i in range(60)],
             [40 + i for i in range(60)])
    ix.apply([L.IDX_SOFT_DELETE], [ns + old[5]])
    om = O.SMap(1 << 20, 1 << 19, 32, 5)
    oix = O.Index()
    for i, k in enumerate(old):
        om.index_op(ns, k, L.IDX_PUT, 3, 1000 + 50 * i, 40 + i)
        oix.set(ns, k, L.IDX_PUT, 3, 1000 + 50 * i, 40 + i)
    om.index_op(ns, old[5], L.IDX_SOFT_DELETE)
    oix.set(ns, old[5], L.IDX_SOFT_DELETE)
    b = Built(40)
    b.put(ns, b"one", b"v1")
    b.put(ns, b"one", b"v2" * 50)
    b.delete(ns, b"one")
    b.put(ns, b"one", b"v4" * 9)
    for i in range(300):
        r = rng.random()
        k = rng.choice(old) if r < 0.5 else b"new-%03d" % rng.randrange(80)
        if r < 0.1 or 0.5 <= r < 0.6:
            b.delete(ns, k)
        else:
            b.put(ns, k, rng.randbytes(rng.randrange(200)), tomb=(i % 9 == 0))
    want, present = [], []
    for (n_, k, op), (off, size) in zip(b.ops, b.locs):
        present.append(om.index_get(n_, k)[0] != L.IDX_NOT_FOUND)
        want.append(om.index_op(n_, k, op, FID, off, size))
    o = write_sync(ix, b.batch, 40)
    assert_written(o, b)
    n = b.batch.size()
    assert o.found[:n].tolist() == [int(p) for p in present]
    assert o.ffid[:n].tolist() == [w[0] for w in want]
    assert o.fbytes[:n].tolist() == [w[1] for w in want]
    assert want[1] == (FID, b.locs[0][1]) and want[2] == (FID, b.locs[1][1]) and want[3] == (0, 0)
    assert any(w[0] == 3 for w in want)  # values of the other fid were freed
    assert_index(ix, oracle_index(b, oix), b.ops + [(ns, k, 0) for k in old])
    assert ix.stats().overflow == 0


# 3. round trip through the resident image -----------------------------------------------------------------
def test_round_trip_get_and_decode(ctx):
    ix, ws = Index(ctx, keys=1 << 12), WalSet(ctx)
    b = full_batch(40, n=230, big={40: 40000, 110: 70000, 180: 200000})
    active = ActiveWal(FID, BASE, 1 << 16, ctx=ctx, walset=ws)  # too small: Index.write grows it
    locs, stats = ix.write(active, b.batch, ws, NS, ETAG)
    data, end = b.expect()
    assert locs == b.locs and active.size == end and len(ws) == 1
    img = active.bytes()
    assert img[40:] == data and W.load_wal(img, FID).base_time == BASE
    # Get: the last op of every key decides
    last = {}
    for i, (ns, k, op) in enumerate(b.ops):
        last[(ns, k)] = i
    keys = sorted(last)
    got = ix.get_records(ws, [ns + k for ns, k in keys], verify=True, ns_size=NS, etag_size=ETAG)
    for (ns, k), g in zip(keys, got):
        i = last[(ns, k)]
        op = b.ops[i][2]
        if op == L.IDX_DELETE:
            assert isinstance(g, ErrKeyNotFound)
        elif op == L.IDX_SOFT_DELETE:
            assert isinstance(g, ErrKeySoftDeleted)
        else:
            assert isinstance(g, W.Record) and g.value == b.batch.records[i][2] and g.key == k and g.ns == ns
    # the library's decode of the image: exactly the batch's records, no error (CRCs and framing, independently)
    dec = ctx.decode(np.frombuffer(img, dtype=np.uint8), 40, BASE, NS, ETAG)
    n = b.batch.size()
    assert dec.result.err_class == L.ERR_NONE and dec.n_records == n
    assert (dec.table["status"][:n] == L.ST_OK).all()
    assert dec.table["size"][:n].tolist() == [l[1] for l in b.locs]
    ref = O.decode(img, 40, BASE, NS, ETAG)
    assert ref.err_class == 0 and len(ref.recs) == n
    assert ref.payloads == [O.record_encode(r[0], r[1], r[2], r[3], r[4], bool(r[6] & L.WR_TOMBSTONE), r[5], BASE)
                            for r in b.batch.records]
    # a second write lands behind the first and is visible at once
    b2 = Built(end)
    b2.put(ns_of(0, NS), b"later", b"x" * 5000)
    locs2, _ = ix.write(active, b2.batch, ns_size=NS, etag_size=ETAG)
    assert locs2 == b2.locs
    g = ix.get_records(ws, [ns_of(0, NS) + b"later"], verify=True, ns_size=NS, etag_size=ETAG)[0]
    assert isinstance(g, W.Record) and g.value == b"x" * 5000
    # Record.Encode's errors surface as the existing error types, with nothing appended
    bad = WriteBatch()
    bad.put(ns_of(0, NS), b"k", b"v", W.Meta(expire=BASE - 1))
    with pytest.raises(W.WalError, match="invalid expire"):
        ix.write(active, bad, ns_size=NS, etag_size=ETAG)
    bad.clear()
    bad.put(ns_of(0, NS), b"k", b"v", W.Meta(expire=BASE + 2 ** 35))
    with pytest.raises(W.RefPanic):
        ix.write(active, bad, ns_size=NS, etag_size=ETAG)
    assert active.size == b2.w.size()
    active.close()
    ws.close()
    ix.close()


# 4. chaining ---------------------------------------------------------------------------------------------
def test_three_batches_chain(ix):
    pos = 40 + 2 * BLOCK - 3
    one = O.Writer(BASE, BASE, at=pos)
    got = b""
    at = pos
    oix = O.Index()
    ops = []
    for r in range(3):
        b = full_batch(at, n=90, big={40: 40000, 70: 70000})
        for rec in b.batch.records:
            one.write(O.record_encode(rec[0], rec[1], rec[2], rec[3], rec[4], bool(rec[6] & 1), rec[5], BASE))
        o = write_sync(ix, b.batch, at)
        assert_written(o, b)
        got += o.wal[:o.res.wal_need].tobytes()
        at = int(o.res.wal_end)
        oracle_index(b, oix)
        ops += b.ops
    assert at == one.size() and got == one.data()
    assert_index(ix, oix, ops)


# 5. rejection: all or nothing ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["expire", "panic", "short_key"])
def test_rejected_batch_writes_nothing(ix, kind):
    ns = ns_of(0, NS)
    pre = Built(40)
    for i in range(50):
        pre.put(ns, b"pre-%02d" % i, b"v" * i)
    assert_written(write_sync(ix, pre.batch, 40), pre)
    before = ix.stats()
    b = full_batch(pre.w.size(), n=120, big={})
    k, j = 37, 90
    recs = b.batch.records
    for i in (k, j):
        r = list(recs[i])
        r[6] &= ~L.WR_DELETED
        if kind == "expire":
            r[4] = BASE - 1
        elif kind == "panic":
            r[4] = BASE + 2 ** 35
        else:
            r[0], r[1] = b"", b"short"  # a merged key of 5 bytes under NsSize 20
        recs[i] = tuple(r)
    o = write_sync(ix, b.batch, b.pos)
    want = {"expire": L.ENC_ERR_EXPIRE, "panic": L.ENC_ERR_PANIC, "short_key": L.ENC_ERR_BATCH}[kind]
    assert o.rc == 0 and o.res.err_class == want and o.res.err_record == k
    assert o.res.n_written == 0 and o.res.wal_end == b.pos and o.res.wal_need == 0
    assert_untouched(o, b.batch.size())
    after = ix.stats()
    assert (after.live, after.slots_used, after.arena_used) == (before.live, before.slots_used, before.arena_used)
    assert_index(ix, oracle_index(pre), pre.ops + [op for op in b.ops])


# 6. capacity ---------------------------------------------------------------------------------------------
def test_capacity_one_byte_short(ix):
    pos = 40 + 2 * BLOCK - 8
    b = full_batch(pos, n=150, big={40: 40000})
    data, end = b.expect()
    need = end - pos
    before = ix.stats()
    o = write_sync(ix, b.batch, pos, cap=need - 1)
    assert o.rc == L.E_CAPACITY and o.res.fits == 0 and o.res.wal_need == need and o.res.err_class == 0
    assert o.res.n_written == 0
    assert_untouched(o, b.batch.size())
    after = ix.stats()
    assert (after.live, after.slots_used, after.arena_used) == (before.live, before.slots_used, before.arena_used)
    st, _, _, _ = ix.get_many(merged(b.ops))
    assert (st == L.IDX_NOT_FOUND).all()
    o = write_sync(ix, b.batch, pos, cap=need)
    assert_written(o, b)
    assert_index(ix, oracle_index(b), b.ops)


# 7. async API, inputs at awkward addresses --------------------------------------------------------------
def test_async_unaligned_inputs_equal_sync(ctx):
    pos = 40 + 2 * BLOCK - 20
    b = full_batch(pos, n=200, big={40: 40000, 110: 70000})
    n = b.batch.size()
    ix_s, ix_a = Index(ctx, keys=1 << 12), Index(ctx, keys=1 << 12)
    s = write_sync(ix_s, b.batch, pos)
    assert_written(s, b)
    # the sync call without the WriteStat columns: the same bytes, offsets and index, the three columns untouched
    ix_n = Index(ctx, keys=1 << 12)
    bare = write_sync(ix_n, b.batch, pos, stat=False)
    assert_written(bare, b)
    assert (bare.found == FILL).all() and (bare.ffid == SENT).all() and (bare.fbytes == SENT).all()
    for f, _ in L.WriteResult._fields_:
        assert getattr(bare.res, f) == getattr(s.res, f), f
    assert_index(ix_n, oracle_index(b), b.ops)
    ix_n.close()
    keys, koff, vals, voff, metas, moff, etags, expire, flags = b.batch.arrays(ETAG)
    d_keys = D.DevBuf(1 + keys.size).upload(keys, 1)
    d_vals = D.DevBuf(7 + vals.size).upload(vals, 7)  # the values end exactly at the allocation's end
    d_metas = D.DevBuf(13 + metas.size + 3).upload(metas, 13)
    d_etags = D.DevBuf(7 + etags.size).upload(etags, 7)
    d_flags = D.DevBuf(13 + n).upload(flags, 13)
    d_koff, d_voff, d_moff, d_exp = (D.upload(a) for a in (koff, voff, moff, expire))
    cap = len(s.wal)
    d_wal = D.DevBuf(13 + cap, fill=FILL)
    d_roff, d_rsize, d_ffid, d_fbytes = (D.DevBuf(8 * n, fill=0x5A) for _ in range(4))
    d_found = D.DevBuf(1 + n, fill=FILL)
    d_res = D.DevBuf(C.sizeof(L.WriteResult))
    ba = L.WriteBatchArrays(n, d_keys.ptr + 1, d_koff.ptr, keys.size, d_vals.ptr + 7, d_voff.ptr, vals.size,
                            d_metas.ptr + 13, d_moff.ptr, metas.size, d_etags.ptr + 7, d_exp.ptr, d_flags.ptr + 13)
    p = L.WriteParams(FID, BASE, pos, NS, ETAG)
    out = L.WriteOut(d_wal.ptr + 13, cap, d_roff.ptr, d_rsize.ptr, d_found.ptr + 1, d_ffid.ptr, d_fbytes.ptr)
    rc = L.lib.bcw_write_records_async(ix_a.handle, C.byref(p), C.byref(ba), C.byref(out), d_res.vp())
    assert rc == 0
    ctx.sync()
    res = L.WriteResult.from_buffer_copy(d_res.download(C.sizeof(L.WriteResult)).tobytes())
    for f, _ in L.WriteResult._fields_:
        assert getattr(res, f) == getattr(s.res, f), f
    whole = d_wal.download()
    assert (whole[:13] == FILL).all() and (whole[13:] == s.wal).all()
    assert (d_roff.download().view(np.uint64) == s.rec_off[:n]).all()
    assert (d_rsize.download().view(np.uint64) == s.rec_size[:n]).all()
    assert (d_found.download()[1:] == s.found[:n]).all()
    assert (d_ffid.download().view(np.uint64) == s.ffid[:n]).all()
    assert (d_fbytes.download().view(np.uint64) == s.fbytes[:n]).all()
    assert_index(ix_a, oracle_index(b), b.ops)
    ix_s.close()
    ix_a.close()


# 8. the empty batch and other NsSize / EtagSize ------------------------------------------------------------
def test_empty_batch(ix):
    for pos in (40, 40 + BLOCK - 3):
        o = write_sync(ix, WriteBatch(), pos)
        assert o.rc == 0 and o.res.wal_end == pos and o.res.wal_need == 0 and o.res.n_written == 0
        assert o.res.fits == 1 and o.res.err_class == 0 and (o.wal == FILL).all()
        o = write_sync(ix, WriteBatch(), pos, stat=False)
        assert o.rc == 0 and o.res.wal_end == pos and o.res.wal_need == 0 and o.res.n_written == 0 and o.res.fits == 1


@pytest.mark.parametrize("ns_size,etag_size", [(0, 0), (8, 16)])
def test_other_ns_and_etag_sizes(ix, ns_size, etag_size):
    pos = 40 + 2 * BLOCK - 6
    b = full_batch(pos, ns_size, etag_size, n=120, big={40: 40000})
    o = write_sync(ix, b.batch, pos, ns_size=ns_size, etag_size=etag_size)
    assert_written(o, b)
    assert_index(ix, oracle_index(b), b.ops)
