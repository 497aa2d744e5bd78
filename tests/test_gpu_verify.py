"""GPU parity of the scrub (bcw_index_verify*, csrc/bcw_verify.hip) against the oracle, key by key: O.Index.get
(Index.Get) -> is the fid resident (getWalRef) -> O.read_record on that image (Wal.ReadRecord + WalParseRecord) ->
O.record_parse (RecordFromBytes) -> the key compare, done here in Python on the payload. Every entry is compared, none
is sampled: counts, by_rd, per_fid and the sorted bad list with its key bytes are equal integer for integer.

The one place the expectation does not ask the oracle is the rule bcw.h states for an index value that is not trusted
(bcw_get_records*' rule): size > seg_len, off < 40 or off > seg_len is READ / BEYOND before WalRecordSize is walked,
where the reference's uint64 arithmetic wraps.

The database: three WALs (fids 3, 7, 12, a baseTime each) of ~150 records of the four shapes (50 keys present in two consecutive files) plus values of 5 000,
32 701, 40 000 and 70 000 bytes, a first record that leaves 3 bytes in its block, in fid 7 a record placed by a filler
so that its header ends and its key begins across a block boundary, user keys of 0, 1, 15, 16, 17 and 200 bytes,
deletes, soft deletes and Puts with tampered values: ~400 keys in a table of at least 1 024 slots (256 per workgroup
round), so the select pass spans several workgroups."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _devmem as D
import _oracle as O
import cases
from bitcaskdb_amd import Context, Index, WalSet, verify_index
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
NSB = cases.sha1("ns")[:NS]
NSX = bytes([NSB[0] ^ 0x40]) + NSB[1:]  # another namespace: one byte differs
FIDS = (3, 7, 12)
BASES = {3: cases.BASE, 7: cases.BASE + 1000, 12: cases.BASE + 50000}
BIG = (5000, 32761 - 60, 40000, 70000)
KLENS = (0, 1, 15, 16, 17, 200)
BLOCK = 32768
U64 = 2 ** 64 - 1


def ukey(i: int) -> bytes:
    return b"key-%06d" % i


def lkey(n: int) -> bytes:
    return bytes((37 * n + 11 * k + 1) & 0xff for k in range(n))


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
    def put(self, merged: bytes, op: int, f: int = 0, o: int = 0, z: int = 0):
        """one op on the device index and on the oracle's"""
        self.ix.apply([op], [merged], [f], [o], [z])
        self.oix.set(merged[:NS], merged[NS:], op, f, o, z)
        self.keys.add(merged)

    def close(self):
        self.ws.close()
        self.ix.close()


def build_db(ctx) -> DB:
    d = DB()
    d.img, d.offs, d.keys = {}, {}, set()
    d.ix, d.oix = Index(ctx, keys=1 << 10), O.Index()
    for w, fid in enumerate(FIDS):
        base = BASES[fid]
        wr = O.Writer(base, base)
        offs = {}
        first = 800 + w
        offs[first] = (wr.write(cases.filler(first, BLOCK - 7 - 3)), BLOCK - 7 - 3)  # leaves 3 bytes: padding follows
        d.keys.add(NSB + ukey(first))
        if fid == 7:  # a record whose fragment ends with its header: the key begins in the next block
            p = O.record_encode(NSB, b"straddle-k", bytes(range(50)), base_time=base)
            hdr = p[0]
            fill = BLOCK - 14 - hdr
            offs[810] = (wr.write(cases.filler(810, fill)), fill)
            offs["straddle"] = (wr.write(p), len(p))
            assert (offs["straddle"][0] + 7 + hdr - 40) % BLOCK == 0 and hdr > 1 + NS
            d.keys |= {NSB + ukey(810), NSB + b"straddle-k"}
        for i in list(range(100 * w, 100 * w + 150)) + [900 + 10 * w + j for j in range(len(BIG))]:
            p = cases.rec(i, BIG[i % 10], base=base) if i >= 900 else shaped(i, base)
            offs[i] = (wr.write(p), len(p))
            d.keys.add(NSB + ukey(i))
        if fid == 12:
            for n in KLENS:
                p = O.record_encode(NSB, lkey(n), bytes(range(n % 7 + 3)), base_time=base)
                offs[("len", n)] = (wr.write(p), len(p))
                d.keys.add(NSB + lkey(n))
        if fid == 3:  # payloads RecordFromBytes rejects, last: IterateRecord stops at them
            junk = bytearray(cases.rec(0, 0))
            junk[1 + NS] = 0  # etag and expire flagged present, beyond the data: the reference panics
            offs["invalid"] = (wr.write(bytes(range(60))), 60)
            offs["panic"] = (wr.write(bytes(junk)), len(junk))
        d.img[fid], d.offs[fid] = wr.data(), offs
        d.ix.recover_segment(d.img[fid], L.MODE_RECORD, fid, 40, base, NS, ETAG)
        d.oix.put_segment(d.img[fid], 40, base, NS, ETAG, 0, fid)
    assert d.offs[12][200][0] == 40 + BLOCK  # the padding is where it is meant
    d.ws = walset_of(ctx, d)
    assert set(d.ix.export()) == d.keys and len(d.keys) >= 350
    return d


def tamper(d: DB):
    """the list test_gpu_get.py applies, plus off = 17 and the wrong-key entries"""
    n3, n12 = len(d.img[3]), len(d.img[12])
    o5, z5 = d.offs[3][5]
    P, DEL, SOFT = L.IDX_PUT, L.IDX_DELETE, L.IDX_SOFT_DELETE
    ops = [(ukey(10), DEL, 0, 0, 0), (ukey(150), DEL, 0, 0, 0), (ukey(300), DEL, 0, 0, 0),
           (ukey(11), SOFT, 0, 0, 0), (ukey(301), SOFT, 0, 0, 0),
           (ukey(20), P, 3, d.offs[3][20][0], d.offs[3][20][1] + 1),
           (ukey(21), P, 3, d.offs[3][21][0], d.offs[3][21][1] - 1),
           (ukey(22), P, 3, d.offs[3][22][0], 0),
           (ukey(23), P, 3, o5 + 13, z5),                       # into the middle of a record
           (ukey(24), P, 3, n3 - 5, 11),                        # near the end of the file
           (ukey(25), P, 3, d.offs[3][25][0], n3 + 1),          # size = seg_len + 1
           (ukey(26), P, 12, d.offs[12][922][0], d.offs[12][922][1] - 1),
           (ukey(27), P, 12, d.offs[12][200][0] - 3, d.offs[12][200][1]),  # the padding inside the span
           (ukey(29), P, 12, n12 - 20, 70000),
           (ukey(30), P, 5, 40, 11),                            # a fid that was never resident
           (ukey(31), P, 3, 17, 11),                            # inside the super block
           (ukey(32), P, 5, 17, 11),                            # the same, of a file that is gone
           (b"junk-a", P, 3, *d.offs[3]["invalid"]), (b"junk-b", P, 3, *d.offs[3]["panic"])]
    for k, op, f, o, z in ops:
        d.put(NSB + k, op, f, o, z)
    # wrong keys: each points at an intact record of another key
    d.wrong = [NSB + ukey(28), NSB + b"key-00025Z", NSX + ukey(252), NSB + ukey(253)[:-1], NSB + b"straddle-x",
               NSB + lkey(200)[:-1] + b"\x00"]
    d.put(d.wrong[0], P, 12, *d.offs[12][250])            # another key's (fid, off, size)
    d.put(d.wrong[1], P, 12, *d.offs[12][251])            # differs in its last byte only
    d.put(d.wrong[2], P, 12, *d.offs[12][252])            # differs in the namespace only
    d.put(d.wrong[3], P, 12, *d.offs[12][253])            # a proper prefix of the record's key
    d.put(d.wrong[4], P, 7, *d.offs[7]["straddle"])       # the straddling record under a tampered key
    d.put(d.wrong[5], P, 12, *d.offs[12][("len", 200)])   # byte 199 of 200 differs
    return d


def walset_of(ctx, d, img=None, fids=FIDS) -> WalSet:
    ws = WalSet(ctx)
    for fid in reversed(fids):  # any order: the set sorts
        ws.add(W.Wal(np.frombuffer((img or d.img)[fid], dtype=np.uint8), fid, 40, BASES[fid]))
    return ws


@pytest.fixture(scope="module")
def clean(ctx):
    d = build_db(ctx)
    yield d
    d.close()


@pytest.fixture(scope="module")
def db(ctx):
    d = tamper(build_db(ctx))
    yield d
    d.close()


class Expect:
    pass


def expected(d, verify, resident=FIDS, img=None, memo=None) -> Expect:
    """the oracle's answer for every key the test ever put: what bcw_verify_result and the list must hold"""
    img = img or d.img
    e = Expect()
    e.checked = e.soft = e.invalid = 0
    e.by_class, e.by_rd, e.bad, e.per_fid = [0] * 5, [0] * 8, [], {}
    for mk in sorted(d.keys):
        st, (f, o, z) = d.oix.get(mk[:NS], mk[NS:])
        if st == 1:
            continue
        if st == 2:
            assert o == 0
            e.soft += 1
            continue
        e.checked += 1
        rst = rec = 0
        if f not in resident:
            cls = L.VFY_NO_WAL
        else:
            n = len(img[f])
            hit = memo.get((f, o, z)) if memo is not None else None
            if hit is None:
                if z > n or o < 40 or o > n:  # bcw.h: not trusted, BEYOND before WalRecordSize is walked
                    hit = (L.RD_BEYOND, 0, None)
                else:
                    r, pay = O.read_record(img[f], o, z, verify)
                    if r != 0:
                        hit = (r, 0, None)
                    else:
                        row = O.record_parse(pay, BASES[f], NS, ETAG)
                        h, kl = int(row["hdr_size"]), int(row["key_len"])
                        hit = (0, int(row["status"]), pay[1:1 + NS] + pay[h:h + kl])
                if memo is not None:
                    memo[(f, o, z)] = hit
            rst, rec, rkey = hit
            cls = L.VFY_READ if rst else L.VFY_RECORD if rec else L.VFY_OK if rkey == mk else L.VFY_KEY
            if cls != L.VFY_RECORD:
                rec = 0
        e.by_class[cls] += 1
        if cls == L.VFY_READ:
            e.by_rd[rst] += 1
        if cls != L.VFY_OK:
            e.bad.append((mk, f, o, z, cls, rst, rec))
            if o >= 40:
                c, b, s = e.per_fid.get(f, (0, 0, 0))
                e.per_fid[f] = (c + 1, b + z, (s + O.wal_record_size(o, z)) & U64)
            else:
                e.invalid += 1
    e.bad.sort()
    e.key_bytes = sum(len(b[0]) for b in e.bad)
    return e


def raw_verify(d, ws, verify, bad_cap, keys_cap, rows_cap, ix=None):
    """one bcw_index_verify call with host arrays of the given caps (0: NULL) -> (rc, result, bad, keys, rows)"""
    bad = (L.VerifyBad * max(bad_cap, 1))()
    keys = (C.c_uint8 * max(keys_cap, 1))(*([0xAB] * max(keys_cap, 1)))
    rows = (L.FidUsageRow * max(rows_cap, 1))()
    out = L.VerifyOut(C.cast(bad, C.c_void_p) if bad_cap else None, bad_cap,
                      C.cast(keys, C.c_void_p) if keys_cap else None, keys_cap,
                      C.cast(rows, C.c_void_p) if rows_cap else None, rows_cap, 0)
    p, res = L.GetParams(NS, ETAG, int(verify), 0), L.VerifyResult()
    rc = L.lib.bcw_index_verify((ix or d.ix).handle, ws.handle, C.byref(p), C.byref(out), C.byref(res))
    return rc, res, bad, bytes(keys), rows


def check_counts(res, e):
    assert (int(res.n_checked), int(res.n_soft_deleted)) == (e.checked, e.soft)
    assert [int(v) for v in res.by_class] == e.by_class and sum(e.by_class) == e.checked
    assert [int(v) for v in res.by_rd] == e.by_rd and e.by_rd[0] == 0
    assert (int(res.n_bad), int(res.bad_key_bytes)) == (len(e.bad), e.key_bytes)
    pf = res.per_fid
    assert (int(pf.n_fids), int(pf.soft_deleted), int(pf.invalid), pf.overflow) == (len(e.per_fid), e.soft, e.invalid, 0)
    assert (int(pf.count), int(pf.bytes), int(pf.span)) == tuple(
        sum(v[j] for v in e.per_fid.values()) & U64 for j in range(3))


def check_lists(res, bad, keys, rows, e):
    got = sorted((keys[int(b.key_pos):int(b.key_pos) + int(b.key_len)], int(b.fid), int(b.off), int(b.size),
                  int(b.cls), int(b.rd_status), int(b.rec_status)) for b in bad[:int(res.n_bad)])
    assert got == e.bad
    for b in bad[:int(res.n_bad)]:  # the hash is the index's, and the key slices tile the key bytes
        mk = keys[int(b.key_pos):int(b.key_pos) + int(b.key_len)]
        assert int(b.hash) == O.murmur3_sum64(mk) and b._pad == 0
    spans = sorted((int(b.key_pos), int(b.key_len)) for b in bad[:int(res.n_bad)])
    pos = 0
    for kp, kl in spans:
        assert kp == pos
        pos += kl
    assert pos == e.key_bytes
    got_rows = [(int(r.fid), (int(r.count), int(r.bytes), int(r.span))) for r in rows[:int(res.per_fid.n_fids)]]
    assert got_rows == sorted(e.per_fid.items())


def verify_whole(d, ws, verify, e, ix=None):
    rc, res, bad, keys, rows = raw_verify(d, ws, verify, len(e.bad), e.key_bytes, len(e.per_fid), ix)
    assert rc == 0 and res.fits == 1
    check_counts(res, e)
    check_lists(res, bad, keys, rows, e)
    return res


@pytest.mark.parametrize("verify", [0, 1])
def test_clean_database(ctx, clean, verify):
    e = expected(clean, verify)
    live = clean.ix.stats().live
    assert e.bad == [] and e.soft == 0 and e.by_class[L.VFY_OK] == e.checked == live == len(clean.keys)
    rc, res, *_ = raw_verify(clean, clean.ws, verify, 0, 0, 0)
    assert rc == 0 and res.fits == 1 and int(res.n_bad) == 0 and int(res.per_fid.n_fids) == 0
    assert int(res.by_class[L.VFY_OK]) == int(res.n_checked) == live - int(res.n_soft_deleted)
    check_counts(res, e)


@pytest.mark.parametrize("verify", [0, 1])
def test_tampered_values_and_wrong_keys(ctx, db, verify):
    e = expected(db, verify)
    assert e.soft == 2 and e.checked == db.ix.stats().live - 2
    assert min(e.by_class) > 0 and e.by_class[L.VFY_KEY] == len(db.wrong)
    assert all(e.by_rd[s] > 0 for s in (L.RD_BEYOND, L.RD_SIZE, L.RD_PANIC))
    assert {1, 2} <= {b[6] for b in e.bad if b[4] == L.VFY_RECORD}
    cls_of = {b[0]: (b[4], b[5]) for b in e.bad}
    assert all(cls_of[k] == (L.VFY_KEY, 0) for k in db.wrong)
    assert cls_of[NSB + ukey(31)] == (L.VFY_READ, L.RD_BEYOND) and cls_of[NSB + ukey(32)] == (L.VFY_NO_WAL, 0)
    assert e.invalid == 2 and e.per_fid[5][0] == 1  # ukey(30) names fid 5 with off >= 40: a row; off = 17 is invalid
    # the untampered straddling record, every key length and the values of every size are OK
    for k in [b"straddle-k"] + [lkey(n) for n in KLENS] + [ukey(900 + 10 * w + j) for w in range(3) for j in range(4)]:
        assert NSB + k not in cls_of and db.oix.get(NSB, k)[0] == 0, k
    verify_whole(db, db.ws, verify, e)


def test_image_corruption(ctx, db):
    img = dict(db.img)
    bad = bytearray(db.img[12])
    o, z = db.offs[12][922]                      # the 40 000-byte value
    l1 = BLOCK - (o - 40) % BLOCK - 7            # its first fragment's data
    assert 0 < l1 < z - 200
    bad[o + 7 + l1 + 7 + 100] ^= 0x20            # in its second fragment
    o2, z2 = db.offs[12][230]                    # a small record in one fragment: a byte of its key
    assert (o2 - 40) % BLOCK + 7 + z2 <= BLOCK
    hdr = db.img[12][o2 + 7]
    bad[o2 + 7 + hdr + 3] ^= 0x01
    img[12] = bytes(bad)
    ws = walset_of(ctx, db, img)
    try:
        for verify in (1, 0):
            e = expected(db, verify, img=img)
            cls_of = {b[0]: (b[4], b[5]) for b in e.bad}
            assert cls_of.get(NSB + ukey(922)) == ((L.VFY_READ, L.RD_CRC) if verify else None)
            assert cls_of[NSB + ukey(230)] == ((L.VFY_READ, L.RD_CRC) if verify else (L.VFY_KEY, 0))
            verify_whole(db, ws, verify, e)
    finally:
        ws.close()


def test_caps(ctx, db):
    e = expected(db, 1)
    nb, kb, nr = len(e.bad), e.key_bytes, len(e.per_fid)
    assert nb > 10 and nr >= 2
    rc, res, *_ = raw_verify(db, db.ws, 1, 0, 0, 0)  # NULL arrays: the totals only
    assert rc == L.E_CAPACITY and res.fits == 0
    check_counts(res, e)
    for caps in ((nb - 1, kb, nr), (nb, kb - 1, nr), (nb, kb, nr - 1)):
        rc, res, bad, keys, rows = raw_verify(db, db.ws, 1, *caps)
        assert rc == L.E_CAPACITY and res.fits == 0, caps
        check_counts(res, e)
        assert all(b.fid == 0 and b.key_len == 0 for b in bad) and set(keys) == {0xAB}, caps  # nothing copied
    rc, res, bad, keys, rows = raw_verify(db, db.ws, 1, int(res.n_bad), int(res.bad_key_bytes),
                                          int(res.per_fid.n_fids))
    assert rc == 0 and res.fits == 1
    check_counts(res, e)
    check_lists(res, bad, keys, rows, e)
    rc, res, bad, keys, rows = raw_verify(db, db.ws, 1, nb + 5, kb + 100, nr + 3)  # room to spare
    assert rc == 0
    check_lists(res, bad, keys, rows, e)


def test_empty_walset_empty_index_and_wrong_pairing(ctx, db):
    ws = WalSet(ctx)
    e = expected(db, 1, resident=())
    assert e.by_class[L.VFY_NO_WAL] == e.checked == len(e.bad) and e.by_rd == [0] * 8
    verify_whole(db, ws, 1, e)
    ix = Index(ctx, keys=16)
    rc, res, *_ = raw_verify(db, db.ws, 1, 0, 0, 0, ix=ix)
    assert rc == 0 and res.fits == 1
    none = Expect()
    none.checked = none.soft = none.invalid = none.key_bytes = 0
    none.by_class, none.by_rd, none.bad, none.per_fid = [0] * 5, [0] * 8, [], {}
    check_counts(res, none)
    ix.close()
    ws.close()
    other = Context(0)
    ws2 = WalSet(other)
    p, res, out = L.GetParams(NS, ETAG, 1, 0), L.VerifyResult(), L.VerifyOut()
    assert L.lib.bcw_index_verify(db.ix.handle, ws2.handle, C.byref(p), C.byref(out), C.byref(res)) == L.E_INVAL
    d_res = D.DevBuf(C.sizeof(L.VerifyResult))
    assert L.lib.bcw_index_verify_async(db.ix.handle, ws2.handle, C.byref(p), C.byref(out), d_res.vp()) == L.E_INVAL
    d_res.free()
    ws2.close()
    other.close()


def test_read_only(ctx, db):
    before = (db.ix.stats(), sorted(db.ix.export().items()))
    for verify in (0, 1):
        raw_verify(db, db.ws, verify, 64, 4096, 8)
    assert (db.ix.stats(), sorted(db.ix.export().items())) == before


def async_verify(d, ws, verify, e):
    """the device-resident form with room for the expectation: (result, bad, keys, rows) after one sync"""
    nb, kb, nr = max(len(e.bad), 1), max(e.key_bytes, 1), max(len(e.per_fid), 1)
    d_bad, d_keys = D.DevBuf(nb * 48), D.DevBuf(kb)
    d_rows, d_res = D.DevBuf(nr * 32), D.DevBuf(C.sizeof(L.VerifyResult), fill=0xEE)
    out = L.VerifyOut(d_bad.ptr, len(e.bad), d_keys.ptr, e.key_bytes, d_rows.ptr, len(e.per_fid), 0)
    p = L.GetParams(NS, ETAG, int(verify), 0)
    return out, p, (d_bad, d_keys, d_rows, d_res), (nb, kb, nr)


def test_async_sees_the_batch_queued_before_it_and_compact_changes_nothing(ctx):
    d = tamper(build_db(ctx))
    try:
        ws = d.ws
        D.sync()
        # ops applied, then the scrub queued at once on the same stream: it sees them
        d.put(NSB + ukey(40), L.IDX_PUT, 3, d.offs[3][41][0], d.offs[3][41][1])  # now another key's record
        d.put(NSB + ukey(42), L.IDX_DELETE)
        d.put(NSB + b"fresh", L.IDX_PUT, 9, 4000, 12)
        e = expected(d, 1)
        cls_of = {b[0]: b[4] for b in e.bad}
        assert cls_of[NSB + ukey(40)] == L.VFY_KEY and cls_of[NSB + b"fresh"] == L.VFY_NO_WAL
        out, p, bufs, (nb, kb, nr) = async_verify(d, ws, 1, e)
        d_bad, d_keys, d_rows, d_res = bufs
        assert L.lib.bcw_index_verify_async(d.ix.handle, ws.handle, C.byref(p), C.byref(out), d_res.vp()) == 0
        ctx.sync()
        res = L.VerifyResult.from_buffer_copy(d_res.download(C.sizeof(L.VerifyResult)).tobytes())
        assert res.fits == 1 and res._pad == 0
        check_counts(res, e)
        bad = (L.VerifyBad * nb).from_buffer_copy(d_bad.download(nb * 48).tobytes())
        rows = (L.FidUsageRow * nr).from_buffer_copy(d_rows.download(nr * 32).tobytes())
        check_lists(res, bad, d_keys.download(kb).tobytes(), rows, e)
        for b in bufs:
            b.free()
        # a rebuild from the live keys: the dead entries stay unseen, the report is the same
        st = d.ix.stats()
        assert st.slots_used > st.live
        d.ix.compact()
        st = d.ix.stats()
        assert st.slots_used == st.live
        verify_whole(d, ws, 1, e)
    finally:
        d.close()


def test_python_verify_index(ctx, db, clean):
    for verify in (False, True):
        e = expected(db, verify)
        rep = verify_index(db.ix, db.ws, NS, ETAG, verify=verify)
        assert (rep.n_checked, rep.n_soft_deleted, rep.n_bad) == (e.checked, e.soft, len(e.bad)) and not rep.clean
        assert list(rep.by_class) == e.by_class and list(rep.by_rd) == e.by_rd
        assert sorted(tuple(b) for b in rep.bad) == e.bad
        assert {f: tuple(u) for f, u in rep.per_fid.items()} == e.per_fid and list(rep.per_fid) == sorted(e.per_fid)
        assert (rep.per_fid.soft_deleted, rep.per_fid.invalid) == (e.soft, e.invalid)
    rep = verify_index(clean.ix, clean.ws, NS, ETAG)
    assert rep.clean and rep.bad == [] and rep.per_fid == {} and rep.by_class[L.VFY_OK] == rep.n_checked > 0
    other = Context(0)
    ws2 = WalSet(other)
    with pytest.raises(ValueError):
        verify_index(db.ix, ws2, NS, ETAG)
    ws2.close()
    other.close()


def test_many_entries_every_loop_strides(ctx, clean):
    """a table of 2^20 slots (the select pass has more rounds than workgroups) holding 40 000 checked entries (more
    work items than k_vfy_read has waves): each points at one of fid 7's records, under the record's own key for 100
    of them and under a key of its own otherwise, so the list takes 39 900 entries. The oracle answers once per
    distinct (fid, off, size)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 40000
    ix = Index(ctx, keys=600_000, arena_bytes=4 << 20)
    cap = ix.stats().slot_capacity
    assert cap // 256 > 8 * cus and n > 4 * 32 * cus  # rounds per select workgroup > 1, items per read wave > 1
    d = DB()
    d.ix, d.oix, d.keys, d.img = ix, O.Index(), set(), clean.img
    ids = list(range(100, 200))
    keys = [NSB + ukey(i) for i in ids] + [NSB + b"many-%05d" % j for j in range(n - len(ids))]
    fo = [clean.offs[7][ids[j % 100]] for j in range(n)]
    ix.apply([L.IDX_PUT] * n, keys, [7] * n, [o for o, _ in fo], [z for _, z in fo])
    for k, (o, z) in zip(keys, fo):
        d.oix.set(k[:NS], k[NS:], L.IDX_PUT, 7, o, z)
    d.keys = set(keys)
    try:
        e = expected(d, 1, memo={})
        assert e.by_class[L.VFY_OK] == 100 and e.by_class[L.VFY_KEY] == n - 100 == len(e.bad)
        verify_whole(d, clean.ws, 1, e, ix=ix)
    finally:
        ix.close()
