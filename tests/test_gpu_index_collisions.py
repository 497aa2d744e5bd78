"""The device index on keys whose murmur3 Sum64 collide (tests/_collide.py; test_collide_host.py shows that every
family key has its target hash). With random keys no two keys share a hash, so the comparisons behind the hash --
stored length and 16 B key chunks in find_slot, arena_matches and keys_match (k_ix_claim), key_chunk's fragment path --
are never what decides. Here they decide every probe: 21 keys of one hash form one chain, among them keys that differ
in their first chunk only, in their last chunk only, inside a ragged last chunk only, and a key that is a proper
prefix of another. Two targets: H_WRAP starts the chain in the table's last slot (it wraps at every capacity), H_ZERO
is the hash a table might take for "empty".

Every expectation comes from the oracle, which compares whole keys: O.Index, O.SMap.index_op, O.Writer,
O.compact_append, O.read_record, O.record_parse. The capacity bound's policy (least recently set first) is
the one exception: the reference's sampled eviction has no deterministic oracle."""
from __future__ import annotations

import random

import numpy as np
import pytest

import _collide as K
import _oracle as O
import cases
import test_gpu_get as TG
import test_gpu_put as TP
import test_gpu_rules as TR
import test_gpu_usage as TU
from bitcaskdb_amd import Index, WalSet
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
NS, ETAG, BASE, FID = TP.NS, TP.ETAG, TP.BASE, TP.FID
PUT, DELETE, SOFT = L.IDX_PUT, L.IDX_DELETE, L.IDX_SOFT_DELETE
TARGET_IDS = ["wrap", "zero"]
targets = pytest.mark.parametrize("target", K.TARGETS, ids=TARGET_IDS)


def val_of(i: int, gen: int = 0):
    """a value of its own for key i (of generation gen)"""
    return 3 + (i + gen) % 4, 40 + 1000 * i + 7 * gen, 30 + i + 100 * gen


def assert_equal(ix: Index, oc: O.Index, keys):
    """Get of every key, export() and the live count against the oracle; keys: every key the index was ever given,
    and any others. Returns the oracle's live set {merged key: value}."""
    keys = list(keys)
    st, fid, off, size = ix.get_many(keys)
    live = {}
    for i, k in enumerate(keys):
        est, ev = oc.get(b"", k)
        assert int(st[i]) == est, (k.hex(), int(st[i]), est)
        if est != L.IDX_NOT_FOUND:
            assert (int(fid[i]), int(off[i]), int(size[i])) == ev, k.hex()
            live[k] = ev
    assert ix.export() == live  # whole keys, each with its own value
    s = ix.stats()
    assert s.live == len(live) == oc.live() and s.overflow == 0
    return live


class Pair:
    """a device index and the oracle's, given the same ops"""

    def __init__(self, ctx, keys: int = 1024):
        self.ix, self.oc, self.seen = Index(ctx, keys=keys), O.Index(), set()

    def apply(self, ops, keys, vals=None):
        vals = vals or [(0, 0, 0)] * len(keys)
        self.ix.apply(ops, keys, [v[0] for v in vals], [v[1] for v in vals], [v[2] for v in vals])
        for op, k, v in zip(ops, keys, vals):
            self.oc.set(b"", k, op, *v)
        self.seen.update(keys)

    def check(self, extra=()):
        return assert_equal(self.ix, self.oc, sorted(self.seen) + list(extra))

    def close(self):
        self.ix.close()


# 1. apply and Get ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_batch", "three_batches", "twice_in_one_batch"])
@targets
def test_apply_and_get(ctx, target, mode):
    """one batch: every key claims its slot past provisional slots of the same hash (keys_match decides); three
    batches: past committed ones too (arena_matches decides); each key twice: the second op must find its own key's
    slot in the chain, and the last op wins"""
    fam = K.family(target)
    n = len(fam)
    p = Pair(ctx)
    if mode == "one_batch":  # last key first: the extension A || X is an earlier op than its prefix A
        p.apply([PUT] * n, fam[::-1], [val_of(i) for i in range(n)][::-1])
    elif mode == "three_batches":
        for r in (2, 1, 0):  # the extension pair's A || X (index 13) goes in before its prefix A (index 12)
            part = list(range(r, n, 3))
            p.apply([PUT] * len(part), [fam[i] for i in part], [val_of(i) for i in part])
    else:
        again = random.Random(1).sample(range(n), n)
        p.apply([PUT] * (2 * n), fam + [fam[i] for i in again],
                [val_of(i) for i in range(n)] + [val_of(i, 1) for i in again])
    rng = random.Random(2)
    never = K.outsider(target)
    live = p.check([rng.randbytes(rng.choice([16, 28, 47, 48])) for _ in range(20)] + [never])
    assert set(live) == set(fam) and never not in live
    s = p.ix.stats()
    assert s.live == n and s.slots_used == n and s.overflow == 0
    cap = s.slot_capacity
    assert cap & (cap - 1) == 0 and cap > n
    if target == K.H_WRAP:  # the chain starts in the last slot and goes on in slot 0: it wrapped
        assert target & (cap - 1) == cap - 1
    else:
        assert target & (cap - 1) == 0
    p.close()


# 2. removal inside a chain -------------------------------------------------------------------------------
@targets
def test_removal_inside_a_chain(ctx, target):
    """a dead slot in the middle of the chain: the keys behind it are still found, the removed key is not; then the
    live-only rebuild, the shrinking one and growth re-insert the chain, and the removed key comes back"""
    fam = K.family(target)
    n = len(fam)
    new, never = K.outsider(target, 2), K.outsider(target)
    p = Pair(ctx)
    p.apply([PUT] * n, fam, [val_of(i) for i in range(n)])
    p.apply([DELETE, SOFT, PUT], [fam[2], fam[4], new], [(0, 0, 0), (0, 0, 0), (7, 5000, 77)])

    def step():
        live = p.check([never])
        TU.check(p.ix)  # fid_usage() equals the dict built from export()
        return live

    live = step()
    assert fam[2] not in live and live[fam[4]] == (0, 0, 0) and live[new] == (7, 5000, 77) and len(live) == n
    s = p.ix.stats()
    assert s.slots_used == n + 1 == s.live + 1  # the deleted key keeps its slot, mid-chain
    p.ix.compact()
    assert p.ix.stats().slots_used == n
    step()
    p.ix.compact(shrink=True)
    step()
    cap0 = p.ix.stats().slot_capacity
    other = [TU.key_of(i) for i in range(6000)]
    p.apply([PUT] * 6000, other, [(11, 40 + 64 * i, 20 + i % 50) for i in range(6000)])
    assert p.ix.stats().slot_capacity > cap0
    step()
    p.apply([PUT, DELETE], [fam[2], fam[0]], [(8, 6000, 88), (0, 0, 0)])
    live = step()
    assert live[fam[2]] == (8, 6000, 88) and fam[0] not in live
    p.close()


# 3. the write batch ----------------------------------------------------------------------------------------
class Written:
    pass


@pytest.fixture(scope="module", params=K.TARGETS, ids=TARGET_IDS)
def written(ctx, request):
    """one write batch over the family (ns = key[:20]) into an index that holds some of its keys under another fid:
    the device's outputs, the oracle's, and the WAL file image. Cases 3 to 6 read it."""
    d = Written()
    d.target = request.param
    d.fam = fam = K.family(d.target)
    d.never, d.elsewhere = K.outsider(d.target), K.outsider(d.target, 3)
    d.ix, d.oix = Index(ctx, keys=1024), O.Index()
    om = O.SMap(1 << 20, 1 << 19, 32, 5)
    # the extension A || X is there before the batch brings A: the longer key sits earlier in the chain than its
    # prefix, so a lookup of A meets an entry whose first 32 bytes are A's and only the length tells them apart
    old = [fam.unrelated[0], fam.unrelated[1], fam.ext[1], fam.twins[1], fam.last_chunk[1], fam.ragged[2], d.elsewhere]
    d.ix.apply([PUT] * len(old), old, [3] * len(old), [1000 + 50 * i for i in range(len(old))],
               [40 + i for i in range(len(old))])
    d.ix.apply([SOFT], [old[1]])
    for i, k in enumerate(old):
        om.index_op(k[:NS], k[NS:], PUT, 3, 1000 + 50 * i, 40 + i)
        d.oix.set(k[:NS], k[NS:], PUT, 3, 1000 + 50 * i, 40 + i)
    om.index_op(old[1][:NS], old[1][NS:], SOFT)
    d.oix.set(old[1][:NS], old[1][NS:], SOFT)
    rng = random.Random(3)
    b = TP.Built(40)

    def put(k, vlen, tomb=False):
        b.put(k[:NS], k[NS:], rng.randbytes(vlen), tomb=tomb)

    def delete(k):
        b.delete(k[:NS], k[NS:])

    for i, k in enumerate(fam.ns20):
        put(k, 10 + i)
    a, ax = fam.ext
    t0, t1 = fam.twins
    for step in (lambda: put(a, 50), lambda: put(ax, 60), lambda: delete(a), lambda: put(ax, 61), lambda: put(a, 51),
                 lambda: put(t0, 70), lambda: put(t1, 71), lambda: put(t0, 0, True), lambda: put(t1, 72),
                 lambda: put(t0, 73)):
        step()  # the extension pair and the tail twins, back to back
    delete(fam.unrelated[2])
    put(fam.unrelated[4], 0, True)
    delete(d.never)  # a Delete that finds nothing, its hash shared by every slot of the chain
    put(fam.last_chunk[0], 300)
    delete(fam.chunk0[1])
    put(fam.unrelated[1], 33)  # soft-deleted before the batch
    d.want, d.present = [], []
    for (ns, k, op), (off, size) in zip(b.ops, b.locs):
        d.present.append(om.index_get(ns, k)[0] != L.IDX_NOT_FOUND)
        d.want.append(om.index_op(ns, k, op, FID, off, size))
    d.o = TP.write_sync(d.ix, b.batch, 40)
    TP.oracle_index(b, d.oix)
    d.b = b
    d.img = O.Writer(BASE, BASE).data()[:40] + b.expect()[0]
    d.keys = sorted(set(TP.merged(b.ops))) + [d.elsewhere]  # every key the index was given (d.never among them)
    yield d
    d.ix.close()


def test_write_batch(written):
    """found / free_fid / free_bytes against O.SMap.index_op replayed in order (k_put_link / k_put_stat: several keys
    per hash, each with an op list of its own), the WAL bytes against O.Writer, the index against O.Index"""
    d = written
    n = d.b.batch.size()
    assert n == len(d.fam.ns20) + 16
    TP.assert_written(d.o, d.b)
    assert d.o.found[:n].tolist() == [int(p) for p in d.present]
    assert d.o.ffid[:n].tolist() == [w[0] for w in d.want]
    assert d.o.fbytes[:n].tolist() == [w[1] for w in d.want]
    assert {True, False} <= set(d.present)
    assert any(w[0] == 3 for w in d.want) and any(w[0] == FID for w in d.want)
    live = assert_equal(d.ix, d.oix, d.keys)
    a, ax = d.fam.ext
    t0, t1 = d.fam.twins
    assert all(live[k][0] == FID for k in (a, ax, t0, t1)) and len({live[k] for k in (a, ax, t0, t1)}) == 4
    assert d.never not in live and live[d.elsewhere][0] == 3


# 4. recovery from tables -------------------------------------------------------------------------------------
def recover_both(ctx, data, keys, mode, fid, ns_size, etag_size, use_record_fid=False, into=None):
    """bcw_index_recover_segment and O.Index.put_segment of one source into fresh indexes (or into the pair `into`);
    the device index must equal the oracle's"""
    ix, oc = into or (Index(ctx, keys=1024), O.Index())
    ec, nput = oc.put_segment(data, 40, BASE, ns_size, etag_size, mode, fid, use_record_fid)
    dres, ires = ix.recover_segment(data, mode, fid, 40, BASE, ns_size, etag_size, use_record_fid)
    assert ec == 0 and dres.err_class == 0 and ires.err_class == 0
    assert ires.n_in == ires.n_done == nput > 0
    live = assert_equal(ix, oc, keys)
    return ix, oc, live


@pytest.mark.parametrize("source", ["record", "hint", "hint_record_fid"])
def test_recover_from_tables(ctx, written, source):
    """the data WAL of case 3 and its hint: every row's key is gathered from the segment, hashed, and claimed against
    the other rows of the same hash"""
    d = written
    if source == "record":
        ix, _, live = recover_both(ctx, d.img, d.keys, L.MODE_RECORD, FID, NS, ETAG)
        assert {v[0] for v in live.values()} == {FID}
    else:
        ec, _, nin, hint = O.hint_by_wal(d.img, FID, 40, BASE, NS, ETAG)
        assert ec == 0 and nin == d.b.batch.size()
        rec_fid = source == "hint_record_fid"
        ix, _, live = recover_both(ctx, hint, d.keys, L.MODE_HINT, 5, NS, 0, use_record_fid=rec_fid)
        assert {v[0] for v in live.values()} == {FID if rec_fid else 5}
    assert set(d.fam.ns20) <= set(live)  # recovery Puts every record, Batch.Delete's too
    ix.close()


@targets
def test_recover_keys_that_straddle_blocks(ctx, target):
    """a family record whose first fragment holds 3 bytes (its namespace spans two blocks) and one whose key does,
    among the other family records: key_chunk's byte-wise path on either side of a colliding compare -- against
    provisional slots (first recovery), against the arena (second recovery, another fid), and in the filter's
    find_slot"""
    fam = K.family(target)
    ka, kb = fam.last_chunk[0], fam.ragged[2]
    a = TR.R(ka[:NS], ka[NS:], vlen=60)
    b = TR.R(kb[:NS], kb[NS:], vlen=50)
    hb = b[0]
    f1 = cases.filler(1, 32768 - 7 - (7 + 3))  # leaves a header and 3 bytes in block 0
    used = 7 + (len(a) - 3)                    # a's Last fragment in block 1
    f2 = cases.filler(2, 32768 - used - 7 - (7 + hb + 40))  # b's First fragment: its header and 40 key bytes
    rest = [k for k in fam.ns20 if k not in (ka, kb)]
    ps = [f1, a, f2, b] + [TR.R(k[:NS], k[NS:], vlen=20 + i) for i, k in enumerate(rest)]
    s = TR.Src(ps, fid=1)
    fr, rc = s.dec.frags, s.dec.recs
    ia, ib = 1, 3
    assert s.mkey(ia) == ka and s.mkey(ib) == kb
    assert int(fr["len"][rc["first_frag"][ia]]) == 3 and rc["first_frag"][ia] != rc["emit_frag"][ia]
    assert int(fr["len"][rc["first_frag"][ib]]) == hb + 40 and rc["first_frag"][ib] != rc["emit_frag"][ib]
    keys = [s.mkey(i) for i in range(s.n)] + [K.outsider(target)]
    ix, oc, live = recover_both(ctx, s.data, keys, L.MODE_RECORD, 2, NS, ETAG)
    assert len(live) == s.n and ix.stats().slots_used == s.n
    arena = ix.stats().arena_used
    recover_both(ctx, s.data, keys, L.MODE_RECORD, 1, NS, ETAG, into=(ix, oc))
    assert ix.stats().arena_used == arena and ix.stats().slots_used == s.n  # every key was found, none added
    base, mask, _, nv = TR._model(s, oc, None)
    assert nv == s.n and int(base.sum()) == s.n
    TR._compact_vs_oracle(ix, s, mask)
    ix.apply([DELETE, SOFT], [fam.last_chunk[1], kb])
    oc.set(b"", fam.last_chunk[1], DELETE)
    oc.set(b"", kb, SOFT)
    base, mask, _, _ = TR._model(s, oc, None)
    assert int(base.sum()) == s.n - 2 and base[ia] == 1 and base[ib] == 0
    TR._compact_vs_oracle(ix, s, mask)
    ix.close()


@targets
def test_recover_ns_size_zero(ctx, target):
    """NsSize 0: the whole family as user keys, the 16- and 17-byte keys among them, from a data WAL and its hint"""
    fam = K.family(target)
    ps = [O.record_encode(b"", k, bytes(range(5 + i)), b"", 0, False, b"", BASE) for i, k in enumerate(fam)]
    s = TR.Src(ps, ns=0, etag=0, fid=4)
    assert s.n == len(fam) and [s.mkey(i) for i in range(s.n)] == list(fam)
    keys = list(fam) + [K.outsider(target)]
    ix, oc, live = recover_both(ctx, s.data, keys, L.MODE_RECORD, 4, 0, 0)
    assert set(live) == set(fam)
    base, mask, _, _ = TR._model(s, oc, None)
    assert int(base.sum()) == s.n
    TR._compact_vs_oracle(ix, s, mask)
    ix.close()
    ec, _, nin, hint = O.hint_by_wal(s.data, 4, 40, BASE, 0, 0)
    assert ec == 0 and nin == s.n
    ix, _, live = recover_both(ctx, hint, keys, L.MODE_HINT, 6, 0, 0)
    assert set(live) == set(fam)
    ix.close()


# 5. the compaction filter, without and with rules ----------------------------------------------------------------
def test_compaction_filter(written):
    """compactOneWal of case 3's WAL against case 3's index: only each key's last record in the file is kept, and
    find_slot picks that key out of its chain. Then a prefix rule of 33 bytes: one byte more than the extension
    pair's A, so it drops A || X and keeps A."""
    d = written
    s = TR.Src(data=d.img, fid=FID)
    assert s.n == d.b.batch.size() and all(s.ok(i) for i in range(s.n))
    base, mask, _, nv = TR._model(s, d.oix, None)
    live = {k for k in d.keys if d.oix.get(b"", k)[0] == L.IDX_FOUND and d.oix.get(b"", k)[1][0] == FID}
    assert nv == s.n and int(base.sum()) == len(live) and 0 < len(live) < s.n
    TR._compact_vs_oracle(d.ix, s, mask)
    a, ax = d.fam.ext
    ra = [i for i in range(s.n) if s.mkey(i) == a and base[i]]
    rax = [i for i in range(s.n) if s.mkey(i) == ax and base[i]]
    assert len(ra) == len(rax) == 1
    try:
        _, mask, counts = TR._run(d.ix, d.oix, s, TR.rules(prefixes=[ax[:33]]))
        assert counts == [0, 0, 1] and mask[ra[0]] == 1 and mask[rax[0]] == 0
        assert int(mask.sum()) == int(base.sum()) - 1
    finally:
        d.ix.clear_compact_rules()


# 6. Get by key ---------------------------------------------------------------------------------------------
def expected_get(d, keys, verify):
    """the oracle's DBImpl.Get per key, in the columns of test_gpu_get.check"""
    out = []
    for k in keys:
        st, (f, o, z) = d.oix.get(b"", k)
        if st == L.IDX_NOT_FOUND:
            out.append((L.GET_NOT_FOUND, 0, 0, 0, 0, 0, None, None))
        elif st == L.IDX_SOFT_DELETED:
            out.append((L.GET_SOFT_DELETED, 0, f, o, z, 0, None, None))
        elif f != FID:
            out.append((L.GET_NO_WAL, 0, f, o, z, 0, None, None))
        else:
            rst, pay = O.read_record(d.img, o, z, verify)
            assert rst == 0
            row = O.record_parse(pay, BASE, NS, ETAG)
            assert row["status"] == 0
            out.append((L.GET_OK, 0, f, o, z, (z + 15) & ~15, pay, row))
    return out


@pytest.mark.parametrize("verify", [False, True])
def test_get_by_key(ctx, written, verify):
    """bcw_get_records of every family key and of the colliding key that was never inserted: k_get_lookup's
    find_slot, then the read of the value it found -- each twin's payload is its own record"""
    d = written
    ws = WalSet(ctx)
    ws.add(W.Wal(np.frombuffer(d.img, dtype=np.uint8), FID, 40, BASE))
    keys = d.fam.ns20 + [d.never, d.elsewhere]
    exp = expected_get(d, keys, verify)
    assert {e[0] for e in exp} == {L.GET_OK, L.GET_NOT_FOUND, L.GET_SOFT_DELETED, L.GET_NO_WAL}
    b = d.ix.get_batch(ws, keys, verify, NS, ETAG)
    assert b.rc == 0
    TG.check(b, exp)
    last = {ns + k: i for i, (ns, k, _) in enumerate(d.b.ops)}
    for i, (k, e) in enumerate(zip(keys, exp)):
        if e[0] != L.GET_OK:
            continue
        pay, row = b.record_bytes(i), e[7]
        h, kl, vl = int(row["hdr_size"]), int(row["key_len"]), int(row["val_len"])
        assert pay[1:1 + NS] + pay[h:h + kl] == k                           # the record is this key's
        assert pay[h + kl:h + kl + vl] == d.b.batch.records[last[k]][2]     # and holds the value of its last Put
    assert all(exp[keys.index(t)][0] == L.GET_OK for t in d.fam.twins + d.fam.ext)
    ws.close()


# 7. the capacity bound -------------------------------------------------------------------------------------------
@targets
def test_capacity_bound_within_one_hash(ctx, target):
    """IndexLimited 128: 8 keys per shard, and the whole family lives in one shard (hash % 16). One key per batch:
    the survivors are the 8 set last (least recently set first), told apart from the evicted keys of the
    same hash only by their bytes"""
    fam = K.family(target)
    n = len(fam)
    ix = Index(ctx, keys=1024)
    ix.set_limit(16 * 8)
    for i, k in enumerate(fam):
        v = val_of(i)
        ix.apply([PUT], [k], [v[0]], [v[1]], [v[2]])
    want = {fam[i]: val_of(i) for i in range(n - 8, n)}
    assert ix.export() == want
    s = ix.stats()
    assert (s.live, s.evicted, s.overflow) == (8, n - 8, 0)
    assert s.evicted_bytes == sum(val_of(i)[2] for i in range(n - 8))
    st, fid, off, size = ix.get_many(list(fam))
    assert st.tolist() == [L.IDX_NOT_FOUND] * (n - 8) + [L.IDX_FOUND] * 8
    assert [(int(fid[i]), int(off[i]), int(size[i])) for i in range(n - 8, n)] == [val_of(i) for i in range(n - 8, n)]
    ix.close()
