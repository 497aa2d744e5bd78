"""GPU tests of the scan of the device index by key prefix (bcw_index_scan*, csrc/bcw_index.hip: k_ix_scan_select,
k_ix_scan_offsets, k_ix_scan_emit; Index.scan / Index.fold) against a Python dict driven by the same ops as the device
index and bytes.startswith. Entries are compared as sorted lists, group rows and totals integer for integer; nothing is
sampled.

The database, built once: three namespaces of 20 bytes (the second differs from the first in byte 0 only, the third in
byte 19 only), user keys of 0, 1, 15, 16, 17, 43, 44, 45 and 200 bytes (merged keys of 63, 64 and 65 bytes sit around
the 64-byte prefix limit; the key of n + 1 bytes continues the key of n bytes), one 3-byte merged key, and over them
deletes, soft deletes, keys overwritten in a later batch, keys deleted and put again, and two entries with 0 < off < 40:
about 390 keys in Index(ctx, keys=1 << 10), a table of at least 1,024 slots and so at least 4 tiles of 256."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _devmem as D
import _oracle as O
import cases
from bitcaskdb_amd import ActiveWal, ErrKeyNotFound, ErrKeySoftDeleted, Index, WalSet, WriteBatch
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W
from bitcaskdb_amd._hip import DevMem

pytestmark = pytest.mark.gpu
NS, ETAG = 20, 20
NSA = cases.sha1("ns")[:NS]
NSB = bytes([NSA[0] ^ 0x40]) + NSA[1:]        # differs in byte 0 only
NSC = NSA[:19] + bytes([NSA[19] ^ 0x01])      # differs in byte 19 only
KLENS = (0, 1, 15, 16, 17, 43, 44, 45, 200)
U64 = 2 ** 64 - 1
SENT = 0xAB
SENT64 = int.from_bytes(bytes([SENT]) * 8, "little")
P, DEL, SOFT = L.IDX_PUT, L.IDX_DELETE, L.IDX_SOFT_DELETE
SHORT = b"abc"  # a merged key shorter than most prefixes


def ukey(n: int, j: int) -> bytes:
    """user key j of n bytes; ukey(n + 1, j) continues ukey(n, j)"""
    return bytes((31 * j + 7 * k + 1) & 0xff for k in range(n))


class DB:
    """a device index and the dict that models it, driven by the same ops"""

    def __init__(self, ctx, keys: int):
        self.ix, self.m = Index(ctx, keys=keys), {}

    def apply(self, ops):
        """ops: (op, merged key, fid, off, size), applied in order"""
        if not ops:
            return
        self.ix.apply([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], [o[3] for o in ops],
                      [o[4] for o in ops])
        for op, k, f, o, z in ops:
            if op == P:
                self.m[k] = (f, o, z)
            elif op == DEL:
                self.m.pop(k, None)
            else:
                self.m[k] = (0, 0, 0)  # SoftDelete stores IndexValue{} whether or not the key was there

    def close(self):
        self.ix.close()


def build_db(ctx) -> DB:
    d = DB(ctx, 1 << 10)
    keys = [ns + ukey(n, j) for ns in (NSA, NSB, NSC) for n in KLENS for j in range(16 if n else 1)]
    assert len(set(keys)) == len(keys) == 3 * (1 + 8 * 16)
    d.apply([(P, k, (1, 2, 9)[i % 3], 40 + 97 * i, 10 + i) for i, k in enumerate(keys)])
    ops = [(P, SHORT, 2, 4040, 3), (P, keys[1], 1, 1, 77), (P, keys[2], 9, 39, 78)]  # two entries with 0 < off < 40
    for i, k in enumerate(keys):
        if i % 7 == 0:
            ops.append((P, k, 12, 100000 + i, 7 * i + 1))  # overwritten in a later batch
        if i % 11 == 3:
            ops.append((DEL, k, 0, 0, 0))
        if i % 13 == 5:
            ops.append((SOFT, k, 0, 0, 0))
    d.apply(ops)
    d.apply([(P, k, 15, 5000 + i, 2 ** 40 + i) for i, k in enumerate(keys) if i % 22 == 3] +  # deleted, put again
            [(DEL, NSB + b"never-there", 0, 0, 0), (SOFT, NSC + b"soft-only", 0, 0, 0)])
    d.keys = keys
    st = d.ix.stats()
    assert st.live == len(d.m) and st.slot_capacity >= 1024
    assert sum(1 for v in d.m.values() if v[1] == 0) >= 25 and sum(1 for v in d.m.values() if 0 < v[1] < 40) == 2
    return d


@pytest.fixture(scope="module")
def db(ctx):
    d = build_db(ctx)
    yield d
    d.close()


class Expect:
    pass


def expected(m: dict, prefixes, soft: bool) -> Expect:
    """the issue's words over the dict: first matching prefix, off != 0 listed and counted, off == 0 a SoftDelete"""
    e = Expect()
    e.entries, e.pid, e.n_soft = {}, {}, 0
    e.groups = [[0, 0, 0, 0] for _ in range(max(len(prefixes), 1))]
    for k, (f, o, z) in m.items():
        g = 0 if not prefixes else next((i for i, p in enumerate(prefixes) if k.startswith(p)), None)
        if g is None:
            continue
        if o != 0:
            e.groups[g][0] += 1
            e.groups[g][1] = (e.groups[g][1] + z) & U64
            e.groups[g][2] += len(k)
        else:
            e.groups[g][3] += 1
            e.n_soft += 1
        if o != 0 or soft:
            e.entries[k] = (f, o, z)
            e.pid[k] = g
    e.groups = [tuple(g) for g in e.groups]
    e.n_listed, e.key_bytes = len(e.entries), sum(len(k) for k in e.entries)
    e.bytes = sum(g[1] for g in e.groups) & U64
    e.n_live = len(m)
    return e


def check_report(rep, e: Expect):
    r = rep.result
    assert (int(r.n_listed), int(r.key_bytes), int(r.bytes), int(r.n_soft_deleted), int(r.n_live), int(r.fits)) == \
        (e.n_listed, e.key_bytes, e.bytes, e.n_soft, e.n_live, 1)
    assert [tuple(g) for g in rep.groups] == e.groups
    assert len(rep.keys) == len(set(rep.keys)) == e.n_listed
    assert sorted(rep.entries.items()) == sorted(e.entries.items())
    assert {k: g for k, g in zip(rep.keys, rep.prefix_id)} == e.pid


def scan_params(prefixes, flags: int = 0):
    prefixes = [bytes(p) for p in prefixes]
    flat = np.frombuffer(b"".join(prefixes) or b"\0", dtype=np.uint8).copy()
    off = np.zeros(len(prefixes) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) for p in prefixes], dtype=np.uint32)
    return L.ScanParams(flags, len(prefixes), flat.ctypes.data, off.ctypes.data), (flat, off)


COLS = ("fid", "off", "size", "prefix_id")
SLACK = 4  # entries (and 8 x SLACK key bytes) of every device array beyond its cap: they keep the sentinel


class DevScan:
    """one bcw_index_scan_async into device buffers pre-filled with the sentinel, downloaded after a synchronise.
    key_shift: the keys array starts that many bytes into its allocation (an odd alignment); null: the columns left
    NULL; totals_only: keys and key_off NULL too (caps 0)"""

    def __init__(self, ix, prefixes, flags, entries_cap, keys_cap, null=(), totals_only=False, key_shift=0,
                 groups=True, run=True):
        self.ix, self.ecap, self.kcap, self.shift = ix, entries_cap, keys_cap, key_shift
        self.rows = max(len(prefixes), 1)
        self.p, self.keep = scan_params(prefixes, flags)
        self.b = {"keys": D.DevBuf(keys_cap + key_shift + 8 * SLACK, fill=SENT),
                  "key_off": D.DevBuf(8 * (entries_cap + 1 + SLACK), fill=SENT),
                  "prefix_id": D.DevBuf(entries_cap + SLACK, fill=SENT),
                  "groups": D.DevBuf(32 * self.rows + 32, fill=SENT), "res": D.DevBuf(C.sizeof(L.ScanResult), fill=SENT)}
        for c in ("fid", "off", "size"):
            self.b[c] = D.DevBuf(8 * (entries_cap + SLACK), fill=SENT)
        ptr = lambda c: None if c in null or totals_only else self.b[c].ptr  # noqa: E731
        self.out = L.ScanOut(None if totals_only else self.b["keys"].ptr + key_shift, keys_cap, ptr("key_off"),
                             ptr("fid"), ptr("off"), ptr("size"), ptr("prefix_id"), entries_cap,
                             self.b["groups"].ptr if groups else None)
        self.null = set(null) | ({"keys", "key_off", *COLS} if totals_only else set())
        if run:
            assert self.launch() == 0
            self.fetch()

    def launch(self) -> int:
        return L.lib.bcw_index_scan_async(self.ix.handle, C.byref(self.p), C.byref(self.out), self.b["res"].vp())

    def fetch(self):
        D.sync()
        self.raw = {c: self.b[c].download().tobytes() for c in self.b}
        self.res = L.ScanResult.from_buffer_copy(self.raw["res"])
        self.key_off = np.frombuffer(self.raw["key_off"], dtype=np.uint64)
        self.col = {c: np.frombuffer(self.raw[c], dtype=np.uint64) for c in ("fid", "off", "size")}
        self.col["prefix_id"] = np.frombuffer(self.raw["prefix_id"], dtype=np.uint8)
        g = np.frombuffer(self.raw["groups"], dtype=np.uint64)
        self.groups = [tuple(int(v) for v in g[4 * r:4 * r + 4]) for r in range(self.rows)]
        self.groups_tail = g[4 * self.rows:]

    def untouched(self, c: str) -> bool:
        return self.raw[c] == bytes([SENT]) * len(self.raw[c])

    def check_listing(self, e: Expect):
        """the layout, the entries against the model, and the sentinel behind everything written"""
        n, kb = e.n_listed, e.key_bytes
        assert (int(self.res.n_listed), int(self.res.key_bytes), int(self.res.fits)) == (n, kb, 1)
        ko = [int(v) for v in self.key_off[:n + 1]]
        assert ko[0] == 0 and ko[n] == kb and all(a <= b for a, b in zip(ko, ko[1:]))
        assert all(int(v) == SENT64 for v in self.key_off[n + 1:])
        kbytes = self.raw["keys"]
        assert kbytes[:self.shift] == bytes([SENT]) * self.shift
        assert kbytes[self.shift + kb:] == bytes([SENT]) * (len(kbytes) - self.shift - kb)
        keys = [kbytes[self.shift + ko[i]:self.shift + ko[i + 1]] for i in range(n)]
        assert sorted(keys) == sorted(e.entries)
        for j, c in enumerate(("fid", "off", "size")):
            if c in self.null:
                assert self.untouched(c)
                continue
            assert [int(v) for v in self.col[c][:n]] == [e.entries[k][j] for k in keys]
            assert all(int(v) == SENT64 for v in self.col[c][n:])
        if "prefix_id" in self.null:
            assert self.untouched("prefix_id")
        else:
            assert [int(v) for v in self.col["prefix_id"][:n]] == [e.pid[k] for k in keys]
            assert all(int(v) == SENT for v in self.col["prefix_id"][n:])
        return keys

    def check_totals(self, e: Expect):
        r = self.res
        assert (int(r.n_listed), int(r.key_bytes), int(r.bytes), int(r.n_soft_deleted), int(r.n_live), r._pad) == \
            (e.n_listed, e.key_bytes, e.bytes, e.n_soft, e.n_live, 0)
        assert self.groups == e.groups and all(int(v) == SENT64 for v in self.groups_tail)


# ---- 1. prefix shapes ----
K64 = NSA + ukey(44, 3)  # a 64-byte merged key; NSA + ukey(45, 3) continues it, NSA + ukey(43, 3) is one byte short
PREFIX_SETS = {
    "one_byte": [NSA[:1]],
    "namespace": [NSB],
    "namespace_plus_7": [NSA + ukey(7, 5)],
    "64_bytes": [K64],
    "overlap_short_first": [NSA, NSA + ukey(7, 5)],
    "overlap_long_first": [NSA + ukey(7, 5), NSA],
    "duplicate": [NSC, NSC, NSA[:19]],
    "nothing": [b"\xff\xfe-no-such-prefix", NSA + b"\xff" * 44],
    "sixty_four": [NSA + ukey(1, j) for j in range(16)] + [NSB + bytes([x]) for x in range(40)] +
                  [NSC + ukey(16, 2), NSC, NSA, NSB, SHORT + b"d", SHORT, b"ab", K64],
}


@pytest.mark.parametrize("name", list(PREFIX_SETS))
def test_prefix_shapes(db, name):
    prefixes = PREFIX_SETS[name]
    e = expected(db.m, prefixes, False)
    check_report(db.ix.scan(prefixes), e)
    if name == "64_bytes":  # equals the 64-byte key, starts the 65- and the 220-byte one; the 63-byte key is too short
        assert set(e.entries) == {K64, NSA + ukey(45, 3), NSA + ukey(200, 3)} and db.m[NSA + ukey(43, 3)][1] != 0
    if name in ("overlap_short_first", "overlap_long_first"):  # the first one wins and moves the counts
        both = [g[0] for g in e.groups]
        assert min(both) == 0 if name == "overlap_short_first" else min(both) > 0
        assert sum(both) == expected(db.m, [NSA], False).groups[0][0]
    if name == "duplicate":
        assert e.groups[1] == (0, 0, 0, 0) and e.groups[0][0] > 0 and e.groups[2][0] > 0
    if name == "nothing":
        assert e.n_listed == 0 and e.groups == [(0, 0, 0, 0)] * 2
    if name == "sixty_four":
        assert len(prefixes) == 64 and sum(1 for g in e.groups if g[0]) >= 20 and e.groups[60][0] == 0


def test_no_prefix_equals_export(db):
    rep = db.ix.scan()
    e = expected(db.m, [], False)
    check_report(rep, e)
    assert rep.entries == {k: v for k, v in db.ix.export().items() if v[1] != 0}
    assert rep.n_listed == db.ix.stats().live - rep.n_soft_deleted and rep.n_soft_deleted >= 25
    with_soft = db.ix.scan(soft_deleted=True)
    assert with_soft.entries == db.ix.export() == db.m
    # the two entries inside the super block are listed: Get finds those too
    assert sum(1 for v in rep.entries.values() if 0 < v[1] < 40) == 2


# ---- 2. the soft-deleted flag ----
@pytest.mark.parametrize("prefixes", [[], [NSC], [NSA + ukey(1, 5), NSA, NSC[:10]]], ids=["all", "ns", "three"])
def test_soft_deleted_flag(db, prefixes):
    off, on = db.ix.scan(prefixes), db.ix.scan(prefixes, soft_deleted=True)
    check_report(off, expected(db.m, prefixes, False))
    check_report(on, expected(db.m, prefixes, True))
    soft = {k for k, v in db.m.items() if v[1] == 0 and (not prefixes or any(k.startswith(p) for p in prefixes))}
    assert soft and set(on.entries) - set(off.entries) == soft and set(off.entries) <= set(on.entries)
    assert all(on.entries[k] == (0, 0, 0) for k in soft)
    assert on.groups == off.groups and on.n_soft_deleted == off.n_soft_deleted == len(soft)


# ---- 3. layout ----
def test_layout_and_determinism(db):
    prefixes = [NSA + ukey(1, 5), NSB, NSA]
    e = expected(db.m, prefixes, True)
    runs = [DevScan(db.ix, prefixes, L.SCAN_SOFT_DELETED, e.n_listed, e.key_bytes, key_shift=s) for s in (0, 0, 5)]
    orders = [r.check_listing(e) for r in runs]
    for r in runs:
        r.check_totals(e)
    for c in ("keys", "key_off", "groups", "res", *COLS):  # two scans of the unchanged index: identical bytes
        assert runs[0].raw[c] == runs[1].raw[c], c
    assert orders[0] == orders[2] and runs[0].raw["key_off"] == runs[2].raw["key_off"]  # whatever the alignment


def test_unchanged_by_compact(ctx):
    d = build_db(ctx)
    try:
        prefixes = [NSC, NSA[:3]]
        before = [d.ix.scan(), d.ix.scan(prefixes, soft_deleted=True)]
        d.ix.compact()
        after = [d.ix.scan(), d.ix.scan(prefixes, soft_deleted=True)]
        for b, a, e in zip(before, after, (expected(d.m, [], False), expected(d.m, prefixes, True))):
            check_report(a, e)
            assert a.entries == b.entries and a.groups == b.groups
            assert bytes(a.result) == bytes(b.result)
    finally:
        d.close()


# ---- 4. caps ----
def raw_scan(ix, prefixes, flags, entries_cap, keys_cap, null_keys=False, null_off=False):
    """one bcw_index_scan with host arrays pre-filled with the sentinel -> (rc, result, groups, keys, key_off, fid)"""
    p, keep = scan_params(prefixes, flags)
    keys = np.full(max(keys_cap, 1), SENT, dtype=np.uint8)
    koff = np.full(entries_cap + 1, SENT64, dtype=np.uint64)
    fid = np.full(max(entries_cap, 1), SENT64, dtype=np.uint64)
    groups = (L.ScanGroup * max(len(prefixes), 1))()
    out = L.ScanOut(None if null_keys else keys.ctypes.data, keys_cap, None if null_off else koff.ctypes.data,
                    None if null_keys or null_off else fid.ctypes.data, None, None, None, entries_cap,
                    C.cast(groups, C.c_void_p))
    res = L.ScanResult()
    rc = L.lib.bcw_index_scan(ix.handle, C.byref(p), C.byref(out), C.byref(res))
    del keep
    return rc, res, [(int(g.count), int(g.bytes), int(g.key_bytes), int(g.soft_deleted)) for g in groups], keys, koff, fid


@pytest.mark.parametrize("short", ["entries", "keys", "both_null"])
def test_caps_too_small(db, short):
    prefixes = [NSB, NSA]
    e = expected(db.m, prefixes, False)
    ecap = {"entries": e.n_listed - 1, "keys": e.n_listed, "both_null": 0}[short]
    kcap = {"entries": e.key_bytes, "keys": e.key_bytes - 1, "both_null": 0}[short]
    s = DevScan(db.ix, prefixes, 0, ecap, kcap, totals_only=short == "both_null")
    assert s.res.fits == 0
    s.check_totals(e)  # the result and the groups are exact
    for c in ("keys", "key_off", *COLS):  # and nothing else was written
        assert s.untouched(c), c
    rc, res, groups, keys, koff, fid = raw_scan(db.ix, prefixes, 0, ecap, kcap, null_keys=short == "both_null",
                                                null_off=short == "both_null")
    assert rc == L.E_CAPACITY and res.fits == 0 and groups == e.groups
    assert (int(res.n_listed), int(res.key_bytes), int(res.bytes), int(res.n_live)) == \
        (e.n_listed, e.key_bytes, e.bytes, e.n_live)
    assert (keys == SENT).all() and (koff == SENT64).all() and (fid == SENT64).all()
    # the retry with the reported sizes succeeds
    rc, res2, groups, keys, koff, fid = raw_scan(db.ix, prefixes, 0, int(res.n_listed), int(res.key_bytes))
    assert rc == 0 and res2.fits == 1 and groups == e.groups and int(koff[e.n_listed]) == e.key_bytes
    kb = keys.tobytes()
    got = {kb[int(koff[i]):int(koff[i + 1])]: int(fid[i]) for i in range(e.n_listed)}
    assert got == {k: v[0] for k, v in e.entries.items()}
    DevScan(db.ix, prefixes, 0, e.n_listed, e.key_bytes).check_listing(e)


@pytest.mark.parametrize("null", [("fid",), ("off",), ("size",), ("prefix_id",), COLS], ids=lambda n: "+".join(n))
def test_optional_columns_null(db, null):
    prefixes = [NSC + ukey(1, 2), NSC]
    e = expected(db.m, prefixes, False)
    s = DevScan(db.ix, prefixes, 0, e.n_listed + 2, e.key_bytes + 3, null=null)
    s.check_listing(e)
    s.check_totals(e)
    g = DevScan(db.ix, prefixes, 0, e.n_listed, e.key_bytes, groups=False)  # no group rows wanted
    g.check_listing(e)
    assert g.untouched("groups")


# ---- 5. refusals ----
def test_refusals(db):
    a = NSA[:3]
    e = expected(db.m, [a], False)
    n, kb = e.n_listed, e.key_bytes

    def refused(prefixes, flags=0, fix=None, **kw):
        s = DevScan(db.ix, prefixes, flags, kw.pop("ecap", n), kw.pop("kcap", kb), run=False, **kw)
        if fix:
            fix(s)
        assert s.launch() == L.E_INVAL
        h = L.ScanOut(None, 0, None, None, None, None, None, 0, None) if not kw else s.out
        assert L.lib.bcw_index_scan(db.ix.handle, C.byref(s.p), C.byref(h), C.byref(L.ScanResult())) == L.E_INVAL
        s.fetch()
        for c in s.b:  # nothing launched
            assert s.untouched(c), c

    refused([a], flags=2)                                      # an unknown flag
    refused([a], flags=0x80000000 | L.SCAN_SOFT_DELETED)
    refused([a] * 65)                                          # n_prefix > 64
    refused([a, b"", a])                                       # an empty prefix
    refused([b"\x07" * 65])                                    # one longer than 64 bytes

    def descend(s):
        s.keep[1][2] = 1  # 0, 3, 1, 9
    refused([a, a, a], fix=descend)                            # offsets that descend

    def null_bytes(s):
        s.p.prefixes = None

    def null_offsets(s):
        s.p.prefix_off = None
    refused([a], fix=null_bytes)                               # n_prefix > 0 with a NULL array
    refused([a], fix=null_offsets)

    def no_keys(s):
        s.out.keys = None

    def no_key_off(s):
        s.out.key_off = None
    refused([a], fix=no_keys, null=("fid",))                   # entries_cap > 0 with keys NULL
    refused([a], fix=no_key_off, null=("fid",))                # ... or key_off NULL
    assert L.lib.bcw_index_scan_async(db.ix.handle, None, None, None) == L.E_INVAL
    # a following scan is still correct, and the accepted edges are accepted
    DevScan(db.ix, [a], 0, n, kb).check_listing(e)
    check_report(db.ix.scan([b"\x07" * 64, a]), expected(db.m, [b"\x07" * 64, a], False))
    with pytest.raises(ValueError):
        db.ix.scan([b""])


# ---- 6. empty and cleared index ----
def test_empty_and_cleared(ctx):
    d = DB(ctx, 1 << 10)
    try:
        for prefixes in ([], [NSA, NSB]):
            rep = d.ix.scan(prefixes, soft_deleted=True)
            check_report(rep, expected({}, prefixes, True))
            assert rep.entries == {} and all(g == (0, 0, 0, 0) for g in rep.groups) and rep.result.fits == 1
        s = DevScan(d.ix, [], 0, 0, 0, null=COLS)  # key_off of one entry: key_off[0] == 0
        assert (int(s.res.n_listed), int(s.res.fits), int(s.key_off[0])) == (0, 1, 0) and s.untouched("keys")
        d.apply([(P, NSA + ukey(16, j), 1, 40 + j, j) for j in range(300)] + [(SOFT, NSB + b"x", 0, 0, 0)])
        check_report(d.ix.scan([NSA]), expected(d.m, [NSA], False))
        d.ix.clear()
        d.m.clear()
        for prefixes in ([], [NSA]):
            rep = d.ix.scan(prefixes, soft_deleted=True)
            check_report(rep, expected({}, prefixes, True))
            assert rep.n_listed == 0 and rep.result.n_live == 0 and rep.result.fits == 1
    finally:
        d.close()


# ---- 7. stream order ----
def test_scan_queued_behind_a_write_batch(ctx):
    """bcw_write_records_async, then bcw_index_scan_async with no synchronise in between: the scan sees the batch"""
    d = DB(ctx, 1 << 10)
    act = ActiveWal(4, cases.BASE, 1 << 20, ctx=ctx)
    try:
        d.apply([(P, NSA + ukey(15, j), 1, 40 + j, 5) for j in range(40)] + [(P, NSB + ukey(15, 1), 1, 99, 5)])
        batch = WriteBatch()
        for j in range(60):
            batch.put(NSA, b"new-%03d" % j, b"v" * (j + 1))
        batch.delete(NSA, ukey(15, 3))
        batch.put(NSA, ukey(15, 4), b"again")
        n = batch.size()
        host = list(batch.arrays(ETAG))
        keys, koff, vals, voff, metas, moff, etags, expire, flags = host
        dev = [DevMem(a.nbytes).upload(a) for a in host]
        d_off, d_size, d_res = DevMem(8 * n), DevMem(8 * n), DevMem(C.sizeof(L.WriteResult))
        arr = L.WriteBatchArrays(n, dev[0].ptr, dev[1].ptr, keys.nbytes, dev[2].ptr, dev[3].ptr, vals.nbytes,
                                 dev[4].ptr, dev[5].ptr, metas.nbytes, dev[6].ptr, dev[7].ptr, dev[8].ptr)
        wp = L.WriteParams(act.fid, act.base_time, act.size, NS, ETAG)
        wout = L.WriteOut(act.ptr + act.size, act.capacity - act.size, d_off.ptr, d_size.ptr, None, None, None)
        live0, export0 = d.ix.stats().live, d.ix.export()
        cap_n, cap_k = live0 + n, sum(len(k) for k in export0) + keys.nbytes
        DevScan(d.ix, [NSA], 0, 0, 0, totals_only=True)  # the index's scan scratch exists: the next scan allocates nothing
        s = DevScan(d.ix, [NSA], 0, cap_n, cap_k, run=False)
        assert L.lib.bcw_write_records_async(d.ix.handle, C.byref(wp), C.byref(arr), C.byref(wout),
                                             C.c_void_p(d_res.ptr)) == 0
        assert s.launch() == 0  # queued directly behind the batch
        s.fetch()
        wres = L.WriteResult.from_buffer_copy(d_res.download(C.sizeof(L.WriteResult)).tobytes())
        assert wres.fits == 1 and wres.err_class == 0 and wres.idx_err == 0 and wres.n_written == n
        off, size = d_off.download(8 * n, dtype=np.uint64), d_size.download(8 * n, dtype=np.uint64)
        for i, r in enumerate(batch.records):
            if r[6] & L.WR_DELETED:
                d.m.pop(r[0] + r[1], None)
            else:
                d.m[r[0] + r[1]] = (act.fid, int(off[i]), int(size[i]))
        e = expected(d.m, [NSA], False)
        assert e.n_listed == 40 - 1 + 60
        s.check_listing(e)
        s.check_totals(e)
        # the scan modified nothing
        live1, export1 = d.ix.stats().live, d.ix.export()
        s2 = DevScan(d.ix, [NSA], 0, cap_n, cap_k)
        assert (d.ix.stats().live, d.ix.export()) == (live1, export1) and export1 == d.m
        assert live1 == live0 + 60 - 1 and s2.raw == s.raw
    finally:
        act.close()
        d.close()


# ---- 8. fold ----
FOLD_FIDS = (3, 8)
FOLD_BASE = {3: cases.BASE, 8: cases.BASE + 777}


@pytest.fixture(scope="module")
def fold_db(ctx):
    """two small resident WALs of records under NSA and NSB (values of 0 to 40,000 bytes, one with an etag and an
    expire, one tombstone), an entry whose fid is not resident, a soft-deleted key and one with a tampered size"""
    d = DB(ctx, 1 << 10)
    d.ws = WalSet(ctx)
    etag = cases.sha1("etag")
    for fid in FOLD_FIDS:
        base = FOLD_BASE[fid]
        wr = O.Writer(base, base)
        ops = []
        for j in range(40):
            ns = NSA if j % 3 else NSB
            key = ukey((1, 16, 17, 45, 200)[j % 5], j % 16) + b"-%d-%d" % (fid, j)
            val = bytes((j * 13 + k) & 0xff for k in range((0, 11, 300, 5000, 40000)[j % 5]))
            p = O.record_encode(ns, key, val, etag=etag if j % 7 == 2 else b"", expire=base + 60 if j % 7 == 2 else 0,
                                tombstone=j % 9 == 4, base_time=base)
            ops.append((P, ns + key, fid, wr.write(p), len(p)))
        d.ws.add(W.Wal(np.frombuffer(wr.data(), dtype=np.uint8), fid, 40, base))
        d.apply(ops)
    some = [k for k in d.m if k.startswith(NSA)]
    d.apply([(P, NSA + b"gone-file", 5, 40, 11), (SOFT, some[0], 0, 0, 0), (DEL, some[1], 0, 0, 0),
             (P, some[2], d.m[some[2]][0], d.m[some[2]][1], d.m[some[2]][2] + 1)])
    yield d
    d.ws.close()
    d.close()


@pytest.mark.parametrize("verify", [False, True], ids=["noverify", "verify"])
def test_fold(fold_db, verify):
    d = fold_db
    single = {}  # Index.get_records(ws, [key])[0] per key, asked once

    def get_one(k):
        if k not in single:
            single[k] = d.ix.get_records(d.ws, [k], verify=verify, ns_size=NS, etag_size=ETAG)[0]
        return single[k]

    for prefixes, soft in (([NSA], False), ([NSB, NSA], True), (None, False)):
        keys, items = d.ix.fold(d.ws, prefixes, verify=verify, ns_size=NS, etag_size=ETAG, soft_deleted=soft)
        rep = d.ix.scan(prefixes, soft_deleted=soft)
        assert keys == rep.keys and sorted(keys) == sorted(expected(d.m, prefixes or [], soft).entries)
        assert len(items) == len(keys) > 20
        kinds = set()
        for k, it in zip(keys, items):
            want = get_one(k)
            kinds.add(type(want))
            if isinstance(want, W.Record):
                assert it == want and it.ns + it.key == k
            else:
                assert type(it) is type(want)
        assert {W.Record, ErrKeyNotFound} <= kinds and len(kinds) >= 3  # the tampered size is a read error
        if soft:
            assert ErrKeySoftDeleted in kinds
        assert isinstance(items[keys.index(NSA + b"gone-file")], ErrKeyNotFound)  # the fid that is not resident
    assert d.ix.fold(d.ws, [b"\xff-none"]) == ([], [])


# ---- 9. many tiles ----
def test_many_tiles(ctx):
    """Index(ctx, keys=360_000): 2^19 slots, 2,048 tiles of 256 -- two rounds of the offsets kernel's one workgroup of
    1,024 threads, and two rounds per workgroup of the select pass, whose grid is capped at 4 workgroups per CU
    (1,024 on the 256 CUs of an MI355X; the emit pass, capped at 8 per CU, takes one tile per workgroup)."""
    d = DB(ctx, 360_000)
    try:
        assert d.ix.stats().slot_capacity == 1 << 19
        ops = [(P, (NSA if j % 3 else NSC) + b"k%05d" % j + ukey(j % 23, j), 1 + j % 5, 40 + 11 * j, j)
               for j in range(5000)]
        ops += [(SOFT, ops[j][1], 0, 0, 0) for j in range(0, 5000, 41)] + [(DEL, ops[j][1], 0, 0, 0)
                                                                          for j in range(7, 5000, 53)]
        d.apply(ops)
        assert d.ix.stats().slot_capacity == 1 << 19 and d.ix.stats().live == len(d.m)
        for prefixes in ([], [NSC]):
            check_report(d.ix.scan(prefixes), expected(d.m, prefixes, False))
        e = expected(d.m, [NSA, NSC], True)
        s = DevScan(d.ix, [NSA, NSC], L.SCAN_SOFT_DELETED, e.n_listed, e.key_bytes)
        s.check_listing(e)
        s.check_totals(e)
    finally:
        d.close()
