"""GPU parity of the batched Get by key (bcw_get_records / bcw_walset, DBImpl.Get db_impl.go:567-587) against the
oracle: O.Index.get (Index.Get), the fid's image when it is in the set (getWalRef), O.read_record on that image
(Wal.ReadRecord + WalParseRecord) and O.record_parse (RecordFromBytes).

The database: three WALs (fids 3, 7, 12, a baseTime each) of ~300 records of every shape plus values that cross one
and two block boundaries, ~50 keys present in two consecutive files, a first record that leaves 3 bytes in its block
(the next record starts after the padding: an index value pointing at the padding has it inside its span, the only
way padding gets there -- the writer never pads inside a record), payloads RecordFromBytes rejects, deletes, soft
deletes and Puts with tampered values."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import _devmem as D
import _oracle as O
import cases
from bitcaskdb_amd import Context, Index, WalSet
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import index as IX
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
NSB = cases.sha1("ns")[:NS]
FIDS = (3, 7, 12)
BASES = {3: cases.BASE, 7: cases.BASE + 1000, 12: cases.BASE + 50000}
REC_FIELDS = ("expire", "key_len", "val_len", "meta_len", "hdr_size", "flags", "etag_off", "status")
BIG = (5000, 32761 - 60, 40000, 70000)
CORRUPT_ID = 900 + 10 * 2 + 2  # the 40 000-byte value of fid 12


def ukey(i: int) -> bytes:
    return b"key-%06d" % i


def shaped(i: int, base: int) -> bytes:
    """the shapes of cases.case_records_mixed, against the WAL's own baseTime"""
    etag = cases.sha1("etag")
    k = i % 4
    if k == 0:
        return cases.rec(i, 11, etag=etag, expire=base + 60, tomb=True, meta=b"\x81\xa3foo\xa3bar", base=base)
    if k == 1:
        return cases.rec(i, 11, etag=etag, expire=base + 61, base=base)
    if k == 2:
        return cases.rec(i, 0, etag=etag, expire=base + 62, tomb=True, meta=b"\x81\xa3foo\xa3bar", base=base)
    return cases.rec(i, 0, base=base)


class DB:
    pass


@pytest.fixture(scope="module")
def db(ctx):
    d = DB()
    d.img, d.offs = {}, {}
    d.ix, d.oix = Index(ctx, keys=1 << 12), O.Index()
    for w, fid in enumerate(FIDS):
        base = BASES[fid]
        wr = O.Writer(base, base)
        offs = {}
        first = 800 + w
        offs[first] = (wr.write(cases.filler(first, 32768 - 7 - 3)), 32768 - 7 - 3)  # leaves 3 bytes: padding follows
        for i in list(range(250 * w, 250 * w + 300)) + [900 + 10 * w + j for j in range(len(BIG))]:
            p = cases.rec(i, BIG[i % 10], base=base) if i >= 900 else shaped(i, base)
            offs[i] = (wr.write(p), len(p))
        if fid == 3:  # payloads RecordFromBytes rejects, last: IterateRecord stops at them
            junk = bytearray(cases.rec(0, 0))
            junk[1 + NS] = 0  # etag and expire flagged present, beyond the data: the reference panics
            offs["invalid"] = (wr.write(bytes(range(60))), 60)
            offs["panic"] = (wr.write(bytes(junk)), len(junk))
        d.img[fid], d.offs[fid] = wr.data(), offs
        d.ix.recover_segment(d.img[fid], L.MODE_RECORD, fid, 40, base, NS, ETAG)
        d.oix.put_segment(d.img[fid], 40, base, NS, ETAG, 0, fid)
    assert d.offs[3][800][0] + 7 + 32758 + 3 == 40 + 32768 == d.offs[3][0][0]  # the padding is where it is meant
    n3, n12 = len(d.img[3]), len(d.img[12])
    o5, z5 = d.offs[3][5]
    o9, z9 = d.offs[12][509]
    ops = [(ukey(10), L.IDX_DELETE, 0, 0, 0), (ukey(260), L.IDX_DELETE, 0, 0, 0), (ukey(700), L.IDX_DELETE, 0, 0, 0),
           (ukey(11), L.IDX_SOFT_DELETE, 0, 0, 0), (ukey(511), L.IDX_SOFT_DELETE, 0, 0, 0),
           (ukey(20), L.IDX_PUT, 3, d.offs[3][20][0], d.offs[3][20][1] + 1),
           (ukey(21), L.IDX_PUT, 3, d.offs[3][21][0], d.offs[3][21][1] - 1),
           (ukey(22), L.IDX_PUT, 3, d.offs[3][22][0], 0),
           (ukey(23), L.IDX_PUT, 3, o5 + 13, z5),                       # into the middle of a record
           (ukey(24), L.IDX_PUT, 3, n3 - 5, 11),                        # near the end of the file
           (ukey(25), L.IDX_PUT, 3, d.offs[3][25][0], n3 + 1),          # size = seg_len + 1
           (ukey(26), L.IDX_PUT, 12, d.offs[12][922][0], d.offs[12][922][1] - 1),
           (ukey(27), L.IDX_PUT, 12, d.offs[12][500][0] - 3, d.offs[12][500][1]),  # the padding inside the span
           (ukey(28), L.IDX_PUT, 12, o9, z9),                           # another key's record: a plain read
           (ukey(29), L.IDX_PUT, 12, n12 - 20, 70000),
           (ukey(30), L.IDX_PUT, 5, 40, 11),                            # a fid that was never resident
           (b"junk-a", L.IDX_PUT, 3, *d.offs[3]["invalid"]), (b"junk-b", L.IDX_PUT, 3, *d.offs[3]["panic"]),
           (b"", L.IDX_PUT, 7, *d.offs[7][300])]                        # the empty user key
    d.ix.apply([o[1] for o in ops], [NSB + o[0] for o in ops], [o[2] for o in ops], [o[3] for o in ops],
               [o[4] for o in ops])
    for k, op, f, o, z in ops:
        d.oix.set(NSB, k, op, f, o, z)
    d.ukeys = sorted({ukey(i) for offs in d.offs.values() for i in offs if isinstance(i, int)}
                     | {o[0] for o in ops})
    d.absent = [b"absent-%03d" % i for i in range(40)]
    q = d.ukeys + d.absent + [ukey(7)] * 5
    random.Random(11).shuffle(q)
    d.query = q
    d.ws = walset_of(ctx, d)
    yield d
    d.ws.close()
    d.ix.close()


def walset_of(ctx, d, img=None) -> WalSet:
    ws = WalSet(ctx)
    for fid in reversed(FIDS):  # any order: the set sorts
        ws.add(W.Wal(np.frombuffer((img or d.img)[fid], dtype=np.uint8), fid, 40, BASES[fid]))
    assert len(ws) == len(FIDS)
    return ws


def expected(d, keys, verify, resident=FIDS, img=None):
    """the oracle's DBImpl.Get per key: (get_status, rd_status, fid, off, size, slot, payload, row)"""
    img = img or d.img
    out = []
    for k in keys:
        st, (f, o, z) = d.oix.get(NSB, k)
        if st == 1:
            out.append((L.GET_NOT_FOUND, 0, 0, 0, 0, 0, None, None))
        elif st == 2:
            out.append((L.GET_SOFT_DELETED, 0, f, o, z, 0, None, None))
        elif f not in resident:
            out.append((L.GET_NO_WAL, 0, f, o, z, 0, None, None))
        else:
            rst, pay = O.read_record(img[f], o, z, verify)
            slot = 0 if rst == L.RD_BEYOND else (z + 15) & ~15
            if rst != 0:
                out.append((L.GET_READ, rst, f, o, z, slot, None, None))
            else:
                row = O.record_parse(pay, BASES[f], NS, ETAG)
                out.append((L.GET_OK if row["status"] == 0 else L.GET_RECORD, 0, f, o, z, slot, pay, row))
    return out


def check(b, exp):
    """every column of a GetBatch against the oracle's results"""
    pos = 0
    for i, (gs, rst, f, o, z, slot, pay, row) in enumerate(exp):
        assert (int(b.get_status[i]), int(b.rd_status[i])) == (gs, rst), (i, b.get_status[i], b.rd_status[i], gs, rst)
        assert (int(b.fid[i]), int(b.off[i]), int(b.size[i])) == (f, o, z), i
        assert int(b.pay_off[i]) == pos and pos % 16 == 0, (i, int(b.pay_off[i]), pos)
        if pay is not None:
            assert b.record_bytes(i) == pay, i
            assert int(b.table["status"][i]) == int(row["status"]), i
        if gs == L.GET_OK:
            for fld in REC_FIELDS:
                assert int(b.table[fld][i]) == int(row[fld]), (i, fld, int(b.table[fld][i]), int(row[fld]))
            assert int(b.table["foff"][i]) == o + 7 and int(b.table["size"][i]) == z
            h, kl, vl = int(row["hdr_size"]), int(row["key_len"]), int(row["val_len"])
            assert b.record_bytes(i)[h + kl:h + kl + vl] == pay[h + kl:h + kl + vl]
        pos += slot
    r = b.result
    assert int(r.payload_need) == pos and r.fits == 1
    assert int(r.n_ok) == sum(e[0] == L.GET_OK for e in exp)
    assert int(r.n_found) == sum(e[0] != L.GET_NOT_FOUND for e in exp)


@pytest.mark.parametrize("verify", [False, True])
def test_get_parity(ctx, db, verify):
    exp = expected(db, db.query, verify)
    seen = {e[0] for e in exp}
    assert {L.GET_OK, L.GET_NOT_FOUND, L.GET_SOFT_DELETED, L.GET_NO_WAL, L.GET_READ, L.GET_RECORD} <= seen
    assert {L.RD_BEYOND, L.RD_SIZE, L.RD_PANIC} <= {e[1] for e in exp if e[0] == L.GET_READ}
    assert {1, 2} <= {int(e[7]["status"]) for e in exp if e[0] == L.GET_RECORD}
    # the later fid won for the keys two files hold, and each file's baseTime shows in its expires
    k = db.query.index(ukey(253))
    assert exp[k][2] == 7 and int(exp[k][7]["expire"]) == BASES[7] + 60 + 253 % 4
    for n in (0, 1, 5, 257, len(db.query)):
        b = db.ix.get_batch(db.ws, [NSB + k for k in db.query[:n]], verify, NS, ETAG)
        assert b.rc == 0
        check(b, exp[:n])


def test_get_missing_wal(ctx, db):
    keys = [NSB + k for k in db.query]
    full = expected(db, db.query, True)
    ws = walset_of(ctx, db)
    ws.remove(7)
    ws.remove(99)  # not present: BCW_OK
    assert len(ws) == 2
    exp = expected(db, db.query, True, resident=(3, 12))
    turned = [i for i, (a, e) in enumerate(zip(full, exp)) if a != e]
    assert turned and all(exp[i][0] == L.GET_NO_WAL and full[i][2] == 7 for i in turned)
    assert len(turned) == sum(e[2] == 7 for e in full)
    check(db.ix.get_batch(ws, keys, True, NS, ETAG), exp)
    dev = D.upload(db.img[7])  # caller-owned image
    ws.put_device(7, dev.ptr, len(db.img[7]), BASES[7])
    check(db.ix.get_batch(ws, keys, True, NS, ETAG), full)
    ws.close()
    dev.free()


def test_get_corruption(ctx, db):
    o, z = db.offs[12][CORRUPT_ID]
    bad = bytearray(db.img[12])
    bad[o + 7 + 20000] ^= 0x20  # inside the 40 000-byte value (its first fragment)
    img = dict(db.img)
    img[12] = bytes(bad)
    ws = walset_of(ctx, db, img)
    keys = [ukey(CORRUPT_ID), ukey(CORRUPT_ID + 1), ukey(5)]
    for verify in (True, False):
        exp = expected(db, keys, verify, img=img)
        assert (exp[0][0], exp[0][1]) == ((L.GET_READ, L.RD_CRC) if verify else (L.GET_OK, L.RD_OK))
        b = db.ix.get_batch(ws, [NSB + k for k in keys], verify, NS, ETAG)
        check(b, exp)
        if not verify:
            assert b.record_bytes(0) == O.read_record(img[12], o, z, False)[1] != O.read_record(db.img[12], o, z)[1]
    ws.close()


def test_get_capacity(ctx, db):
    keys = [NSB + k for k in db.query]
    exp = expected(db, db.query, False)
    need = sum(e[5] for e in exp)
    b = db.ix.get_batch(db.ws, keys, False, NS, ETAG, payload_cap=need - 1, fill=0xAB)
    assert b.rc == L.E_CAPACITY and b.result.fits == 0 and int(b.result.payload_need) == need
    assert (b.payload == 0xAB).all()
    pos = 0
    for i, e in enumerate(exp):  # the lookup columns
        assert (int(b.fid[i]), int(b.off[i]), int(b.size[i]), int(b.pay_off[i])) == (e[2], e[3], e[4], pos), i
        if e[0] in (L.GET_NOT_FOUND, L.GET_SOFT_DELETED, L.GET_NO_WAL) or e[1] == L.RD_BEYOND:
            assert (int(b.get_status[i]), int(b.rd_status[i])) == (e[0], e[1]), i
        pos += e[5]
    assert (b.table["status"] == 0).all() and (b.table["foff"] == 0).all()  # no table row either
    b = db.ix.get_batch(db.ws, keys, False, NS, ETAG, payload_cap=int(b.result.payload_need), fill=0xAB)
    assert b.rc == 0
    check(b, exp)
    b = db.ix.get_batch(db.ws, keys, False, NS, ETAG)  # the retry inside get_batch
    assert b.rc == 0 and int(b.result.payload_need) == need
    # the sync call's device layout on both sides of a lookup workgroup (256 keys), with and without the optional
    # table, and a payload buffer too small at each
    first = next(i for i, e in enumerate(exp) if e[0] == L.GET_OK)  # the batch of one key has a payload
    many = (db.query[first:] + db.query[:first])[:257]
    assert len(many) == 257
    for n in (1, 256, 257):
        exp_n = expected(db, many[:n], False)
        need_n = sum(e[5] for e in exp_n)
        assert need_n > 16
        with_tab = db.ix.get_batch(db.ws, [NSB + k for k in many[:n]], False, NS, ETAG)
        check(with_tab, exp_n)
        bare = db.ix.get_batch(db.ws, [NSB + k for k in many[:n]], False, NS, ETAG, table=False)
        assert bare.rc == 0 and all(not col.any() for col in bare.table.values())
        for c in ("get_status", "rd_status", "fid", "off", "size", "pay_off"):
            np.testing.assert_array_equal(getattr(bare, c), getattr(with_tab, c), err_msg=c)
        assert bare.payload[:need_n].tobytes() == with_tab.payload[:need_n].tobytes()
        for f in ("n_found", "n_ok", "payload_need", "fits"):
            assert getattr(bare.result, f) == getattr(with_tab.result, f), f
        short = db.ix.get_batch(db.ws, [NSB + k for k in many[:n]], False, NS, ETAG, payload_cap=need_n - 1, fill=0xAB,
                                table=False)
        assert short.rc == L.E_CAPACITY and short.result.fits == 0 and int(short.result.payload_need) == need_n
        assert (short.payload == 0xAB).all()
        np.testing.assert_array_equal(short.pay_off, with_tab.pay_off)


def test_get_leaves_index_untouched(ctx, db):
    before = (db.ix.stats(), sorted(db.ix.export().items()))
    db.ix.get_batch(db.ws, [NSB + k for k in db.query], True, NS, ETAG)
    assert (db.ix.stats(), sorted(db.ix.export().items())) == before


def test_get_after_growth(ctx, db):
    """an index that grew several times since it was created: the get reads the buffers of its own launch"""
    ix = Index(ctx, keys=16)
    cap0 = ix.stats().slot_capacity
    ids = list(range(250, 550))
    for r in range(10):  # 3 000 keys, ten batches; the first 300 are fid 7's records
        ks = [NSB + (ukey(i) if r == 0 else b"grow-%d-%d" % (r, i)) for i in ids]
        ix.apply([L.IDX_PUT] * len(ks), ks, [7] * len(ks), [db.offs[7][i][0] for i in ids],
                 [db.offs[7][i][1] for i in ids])
    assert ix.stats().slot_capacity >= 4 * cap0 and ix.stats().live == 3000
    keys = [NSB + (ukey(i) if r == 0 else b"grow-%d-%d" % (r, i)) for r in range(10) for i in ids]
    b = ix.get_batch(db.ws, keys, True, NS, ETAG)
    assert b.rc == 0 and int(b.result.n_found) == 3000 == int(b.result.n_ok)
    for j in (0, 299, 300, 1234, 2999):
        o, z = db.offs[7][ids[j % 300]]
        assert (int(b.fid[j]), int(b.off[j]), int(b.size[j])) == (7, o, z)
        assert b.record_bytes(j) == O.read_record(db.img[7], o, z)[1]
    ix.close()


def test_get_async_device_resident(ctx, db):
    """device arrays in and out on the context's stream, one sync at the end: the sync call's answers"""
    keys = [NSB + k for k in db.query]
    n = len(keys)
    ref = db.ix.get_batch(db.ws, keys, True, NS, ETAG)
    flat, koff = IX._pack(keys)
    d_keys, d_koff = D.upload(flat), D.upload(koff.view(np.uint8))
    col = {name: D.DevBuf(n * w) for name, w in (("get_status", 1), ("rd_status", 1), ("fid", 8), ("off", 8),
                                                 ("size", 8), ("pay_off", 8))}
    cap = int(ref.result.payload_need)
    d_pay, d_res, tab = D.DevBuf(cap, fill=0xAB), D.DevBuf(C.sizeof(L.GetResult)), D.DevTable(n)
    out = L.GetOut(C.cast(col["get_status"].vp(), L.u8p), C.cast(col["rd_status"].vp(), L.u8p),
                   C.cast(col["fid"].vp(), L.u64p), C.cast(col["off"].vp(), L.u64p), C.cast(col["size"].vp(), L.u64p),
                   C.cast(col["pay_off"].vp(), L.u64p), C.cast(d_pay.vp(), L.u8p), cap, tab.t)
    p = L.GetParams(NS, ETAG, 1, 0)
    D.sync()
    rc = L.lib.bcw_get_records_async(db.ix.handle, db.ws.handle, C.byref(p), n, d_keys.vp(), d_koff.vp(), C.byref(out),
                                     d_res.vp())
    assert rc == 0
    ctx.sync()
    res = L.GetResult.from_buffer_copy(d_res.download(C.sizeof(L.GetResult)).tobytes())
    assert (res.n_found, res.n_ok, res.payload_need, res.fits) == (ref.result.n_found, ref.result.n_ok, cap, 1)
    for name, w in (("get_status", 1), ("rd_status", 1), ("fid", 8), ("off", 8), ("size", 8), ("pay_off", 8)):
        got = col[name].download(n * w).view(np.uint8 if w == 1 else np.uint64)
        assert (got == getattr(ref, name)).all(), name
    pay = d_pay.download(cap)
    for i in range(n):
        if ref.get_status[i] in (L.GET_OK, L.GET_RECORD):
            o = int(ref.pay_off[i])
            assert bytes(pay[o:o + int(ref.size[i])]) == ref.record_bytes(i), i
    for name, _ in L.TABLE_COLUMNS:
        if name not in ("aux0", "aux1"):
            assert (tab.column(name, n) == ref.table[name]).all(), name
    for b in [d_keys, d_koff, d_pay, d_res, *col.values()]:
        b.free()


def test_get_wrong_pairing(ctx, db):
    other = Context(0)
    ws = WalSet(other)
    gst = np.zeros(1, np.uint8)
    u = np.zeros(1, np.uint64)
    out = L.GetOut(gst.ctypes.data_as(L.u8p), gst.ctypes.data_as(L.u8p), u.ctypes.data_as(L.u64p),
                   u.ctypes.data_as(L.u64p), u.ctypes.data_as(L.u64p), u.ctypes.data_as(L.u64p), None, 0,
                   L.RecordTable())
    key, koff = np.frombuffer(NSB, dtype=np.uint8), np.array([0, NS], dtype=np.uint64)
    p, res = L.GetParams(NS, ETAG, 0, 0), L.GetResult()
    assert L.lib.bcw_get_records(db.ix.handle, ws.handle, C.byref(p), 1, key.ctypes.data_as(C.c_void_p),
                                 koff.ctypes.data_as(L.u64p), C.byref(out), C.byref(res)) == L.E_INVAL
    d_res = D.DevBuf(C.sizeof(L.GetResult))
    assert L.lib.bcw_get_records_async(db.ix.handle, ws.handle, C.byref(p), 0, None, None, C.byref(out),
                                       d_res.vp()) == L.E_INVAL
    d_res.free()
    ws.close()
    other.close()


def test_get_python_layer(ctx, db):
    exp = expected(db, db.query, True)
    got = db.ix.get_records(db.ws, [NSB + k for k in db.query], verify=True)
    assert len(got) == len(exp)
    rd_err = {L.RD_BEYOND: W.WalError, L.RD_CORRUPTED: W.ErrWalCorruptedData, L.RD_CRC: W.ErrWalMismatchCRC,
              L.RD_SIZE: W.ErrWalMismatchSize, L.RD_TYPE: W.ErrWalUnknownRecordType,
              L.RD_INCOMPLETE: W.ErrWalIncompleteRecord, L.RD_PANIC: W.RefPanic}
    for k, g, (gs, rst, f, o, z, slot, pay, row) in zip(db.query, got, exp):
        if gs == L.GET_OK:
            h, kl, vl, ml = (int(row[c]) for c in ("hdr_size", "key_len", "val_len", "meta_len"))
            assert isinstance(g, W.Record) and g.ns == pay[1:1 + NS] and g.key == pay[h:h + kl]
            assert g.value == pay[h + kl:h + kl + vl]
            assert g.meta.expire == int(row["expire"]) and g.meta.app_meta == pay[h + kl + vl:h + kl + vl + ml]
            assert g.meta.flags == (1 if int(row["flags"]) & 4 else 0)
            eo = int(row["etag_off"])
            assert g.meta.etag == (b"" if int(row["flags"]) & 1 else pay[eo:eo + ETAG])
        elif gs in (L.GET_NOT_FOUND, L.GET_NO_WAL):
            assert type(g) is IX.ErrKeyNotFound, k
        elif gs == L.GET_SOFT_DELETED:
            assert type(g) is IX.ErrKeySoftDeleted, k
        elif gs == L.GET_READ:
            assert type(g) is rd_err[rst], (k, rst, g)
        else:
            assert type(g) is (W.ErrInvalidData if int(row["status"]) == 1 else W.RefPanic), k


def test_get_many_requests(ctx):
    """a batch large enough that every loop of the get takes another pass: k_get_scan carries its running sum over
    more than one chunk of 1024 workgroup sums (n > 262 144), k_get_read's waves stride over the requests
    (n > 128 x CUs), and k_get_offsets meets 256-key workgroups whose slots are all zero, at the chunk edge too.
    The oracle answers once per distinct key; every column is compared for every request."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(262144 + 256 + 3, 128 * cus + 777)
    assert n > 1024 * 256 and n > 128 * cus
    d = DB()
    d.img, d.oix = {}, O.Index()
    ix = Index(ctx, keys=1 << 12)
    offs = {}
    for fid in (3, 7):
        wr = O.Writer(BASES[fid], BASES[fid])
        for i in range(1000 * fid, 1000 * fid + 1000):
            p = cases.rec(i, i % 53, base=BASES[fid])  # payloads of 35..87 bytes
            offs[i] = (fid, wr.write(p), len(p))
        d.img[fid] = wr.data()
        ix.recover_segment(d.img[fid], L.MODE_RECORD, fid, 40, BASES[fid], NS, ETAG)
        d.oix.put_segment(d.img[fid], 40, BASES[fid], NS, ETAG, 0, fid)
    ops = [(ukey(3000 + i), L.IDX_DELETE, 0, 0, 0) for i in range(20)]
    ops += [(ukey(3100 + i), L.IDX_SOFT_DELETE, 0, 0, 0) for i in range(20)]
    ops += [(ukey(3200 + i), L.IDX_PUT, 5, offs[3200 + i][1], offs[3200 + i][2]) for i in range(20)]      # no WAL
    ops += [(ukey(3300 + i), L.IDX_PUT, 3, len(d.img[3]) + 1 + i, offs[3300 + i][2]) for i in range(20)]  # BEYOND
    ops += [(ukey(7000 + i), L.IDX_PUT, 7, offs[7000 + i][1], offs[7000 + i][2] + (1 if i % 2 else -1))
            for i in range(20)]                                                                          # SIZE
    ix.apply([o[1] for o in ops], [NSB + o[0] for o in ops], [o[2] for o in ops], [o[3] for o in ops],
             [o[4] for o in ops])
    for k, op, f, o, z in ops:
        d.oix.set(NSB, k, op, f, o, z)
    ukeys = [ukey(i) for i in offs] + [b"absent-%03d" % i for i in range(40)]
    ws = WalSet(ctx)
    for fid in (3, 7):
        ws.add(W.Wal(np.frombuffer(d.img[fid], dtype=np.uint8), fid, 40, BASES[fid]))
    nb = (n + 255) // 256
    rng = np.random.default_rng(5)
    try:
        for verify in (True, False):
            exp = expected(d, ukeys, verify, resident=(3, 7))
            assert {L.GET_OK, L.GET_NOT_FOUND, L.GET_SOFT_DELETED, L.GET_NO_WAL, L.GET_READ} <= {e[0] for e in exp}
            assert {L.RD_BEYOND, L.RD_SIZE} <= {e[1] for e in exp if e[0] == L.GET_READ}
            col = {c: np.array([e[j] for e in exp], dtype=np.uint64) for j, c in
                   enumerate(("get_status", "rd_status", "fid", "off", "size", "slot"))}
            zero = np.nonzero(col["slot"] == 0)[0]
            assert len(zero) >= 100
            pick = rng.integers(0, len(ukeys), n)
            for b in (0, 7, 1023, 1024, nb - 2):  # workgroups whose slots are all zero, two at the scan's chunk edge
                pick[256 * b:256 * b + 256] = rng.choice(zero, 256)
            keys = [NSB + ukeys[i] for i in pick]
            slot = col["slot"][pick]
            pay_off = np.concatenate([[0], np.cumsum(slot)[:-1]]).astype(np.uint64)
            need = int(slot.sum())
            assert need > 0 and int(slot[256 * 1024:].sum()) > 0  # the second chunk's workgroups have bytes to place
            g = ix.get_batch(ws, keys, verify, NS, ETAG, payload_cap=need, fill=0xAB)
            assert g.rc == 0 and g.result.fits == 1 and int(g.result.payload_need) == need
            for c in ("get_status", "rd_status", "fid", "off", "size"):
                np.testing.assert_array_equal(getattr(g, c).astype(np.uint64), col[c][pick], err_msg=c)
            np.testing.assert_array_equal(g.pay_off, pay_off, err_msg="pay_off")
            gs = col["get_status"][pick]
            assert int(g.result.n_found) == int((gs != L.GET_NOT_FOUND).sum())
            assert int(g.result.n_ok) == int((gs == L.GET_OK).sum())
            ok = np.nonzero(gs == L.GET_OK)[0]
            assert len(ok) > n // 2
            np.testing.assert_array_equal(g.table["foff"][ok], g.off[ok] + 7)
            np.testing.assert_array_equal(g.table["size"][ok], g.size[ok])
            pay = g.payload.tobytes()
            for r in ok.tolist():
                o, want = int(pay_off[r]), exp[pick[r]][6]
                assert pay[o:o + len(want)] == want, r
        # one byte short of a slot: nothing but the lookup columns is written
        g = ix.get_batch(ws, keys, False, NS, ETAG, payload_cap=need - 16, fill=0xAB)
        assert g.rc == L.E_CAPACITY and g.result.fits == 0 and int(g.result.payload_need) == need
        assert (g.payload == 0xAB).all()
        np.testing.assert_array_equal(g.pay_off, pay_off)
    finally:
        ws.close()
        ix.close()
