"""One database through its whole life on the device, compared with the oracle chain after every step.

tests/_lifecycle.py holds the seeded workload and RefDB, the reference's chain restated with tests/_oracle.py and plain
Python (test_lifecycle_host.py checks on the CPU that the run has the shapes it is there for). Here DevDB takes the
same steps through the Python layer -- Index.write into an ActiveWal, rotation, fid_usage / wal_garbage and the picker,
compact_wals_filtered, the hint replay (recover_segment with use_record_fid), drop_fids, WalSet.remove, verify_index,
scan / fold, a restart through recover_from_wals, and a recovery of what is left at the end -- on ONE index, ONE WalSet
and the images the steps themselves produced. After every step check_state compares the index (get_many, export, scan,
stats), a Get of every key ever written, the accounting (fid_usage, wal_garbage, the per-fid conservation identity of
test_lifecycle_host.py) and the scrub with the oracle, integer for integer and byte for byte. No expected value comes
from the library."""
from __future__ import annotations

import pytest

import _lifecycle as LC
import _oracle as O
from bitcaskdb_amd import (ActiveWal, Context, ErrKeyNotFound, ErrKeySoftDeleted, FidUsage, Index, PickerWalInfo, WalSet,
                           WriteBatch, default_compaction_picker, recover_from_wals, verify_index, wal_garbage)
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import index as IX
from bitcaskdb_amd import wal as W

pytestmark = pytest.mark.gpu
BASE = LC.BASE


def usage_map(rows: dict) -> dict:
    return {f: FidUsage(*r) for f, r in rows.items()}


class DevDB:
    """the device side: an index of 1024 slots, the resident set, the active WAL, and the file images as the steps
    left them (a rotated WAL's bytes are read back from HBM, a compaction's output is what the call appended)"""

    def __init__(self, ctx, peer, ns_size: int, etag_size: int, first_fid: int):
        self.ctx, self.peer, self.ns, self.etag = ctx, peer, ns_size, etag_size
        self.ix = Index(ctx, keys=1 << 10)
        self.ws = WalSet(ctx)
        self.wals = {}    # fid -> ActiveWal of every written WAL that still exists (its image stays in HBM)
        self.images = {}  # fid -> bytes of the files that are no longer written
        self.hints = {}   # fid -> bytes of a compaction output's hint file
        self.active = None
        self.scrub_b = self.retain_b = None
        self.rotate(first_fid)

    def close(self):
        for w in self.wals.values():
            w.close()
        self.wals = {}
        self.ws.close()
        self.ix.close()

    def rotate(self, fid: int):
        if self.active is not None:
            self.images[self.active.fid] = self.active.bytes()
        self.active = self.wals[fid] = ActiveWal(fid, BASE, 1 << 16, ctx=self.ctx, walset=self.ws)  # grows as it fills

    def all_sizes(self) -> dict:
        return {**{f: len(b) for f, b in self.images.items()}, self.active.fid: self.active.size}

    def files(self) -> dict:
        """what is on disk, as recover_from_wals takes it: outputs with their hints, written WALs without"""
        imgs = {**self.images, self.active.fid: self.active.bytes()}
        return {f: (W.load_wal(b, f), W.load_wal(self.hints[f], f) if f in self.hints else None)
                for f, b in imgs.items()}

    def remove(self, fids):
        for f in fids:
            self.ws.remove(f)
            if f in self.wals:
                self.wals.pop(f).close()
            self.images.pop(f)
            self.hints.pop(f, None)


def expect_named(ref: LC.RefDB, dangling: dict):
    """the rows of the entries in `dangling`, {fid: FidUsage}, by the oracle's WalRecordSize"""
    rows = {}
    for f, o, s in dangling.values():
        c, b, sp = rows.get(f, (0, 0, 0))
        rows[f] = (c + 1, b + s, sp + O.wal_record_size(o, s))
    return usage_map({f: rows[f] for f in sorted(rows)})


def check_state(dev: DevDB, ref: LC.RefDB, where: str):
    ix, ws, ns, etag = dev.ix, dev.ws, ref.ns, ref.etag
    pairs = list(ref.keys)
    keys = [n + k for n, k in pairs]
    # 2. the index
    st, fid, off, size = ix.get_many(keys)
    for i, (n, k) in enumerate(pairs):
        est, ev = ref.oix.get(n, k)
        assert st[i] == est, (where, keys[i])
        if est == LC.FOUND:
            assert (int(fid[i]), int(off[i]), int(size[i])) == ev, (where, keys[i])
    ent = ref.entries()
    backed = {k: v for k, v in ent.items() if v[1] != 0}
    soft = len(ent) - len(backed)
    assert ix.export() == ent, where
    stats = ix.stats()
    assert stats.live == len(ent) and stats.overflow == 0, where
    rep = ix.scan()
    assert rep.entries == backed and rep.n_soft_deleted == soft and rep.n_listed == len(backed), where
    assert ix.scan(soft_deleted=True).entries == ent, where
    # 3. Get of every key ever written
    got = ix.get_records(ws, keys, verify=True, ns_size=ns, etag_size=etag)
    for (n, k), g in zip(pairs, got):
        want = ref.expect_get(n, k)
        if want == LC.NOT_FOUND:
            assert isinstance(g, ErrKeyNotFound), (where, n + k, g)
        elif want == LC.SOFT_DELETED:
            assert isinstance(g, ErrKeySoftDeleted), (where, n + k, g)
        else:
            assert isinstance(g, W.Record), (where, n + k, g)
            assert g.value == want and g.ns == n and g.key == k, (where, n + k)
    prefix = LC.namespaces(ns)[1] + b"a"
    fkeys, items = ix.fold(ws, [prefix], verify=True, ns_size=ns, etag_size=etag)
    assert sorted(fkeys) == sorted(k for k in backed if k.startswith(prefix)), where
    for k, g in zip(fkeys, items):
        want = ref.expect_get(k[:ns], k[ns:])
        assert isinstance(g, ErrKeyNotFound) if want == LC.NOT_FOUND else g.value == want, (where, k)
    # 4. the accounting, three ways
    rows, rsoft = ref.usage()
    u = ix.fid_usage()
    assert list(u) == sorted(u) and dict(u) == usage_map(rows) and (u.soft_deleted, u.invalid) == (rsoft, 0), where
    sizes = dev.all_sizes()
    assert sizes == ref.sizes(), where
    assert wal_garbage(ix, sizes) == ref.garbage(sizes), where
    for f in set(ref.put_bytes) | set(ref.freed) | set(ref.retired) | set(u):
        if f != 0:  # fid 0 collects the WriteStats that freed nothing
            assert ref.put_bytes[f] - ref.freed[f] - ref.retired[f] == (u[f].bytes if f in u else 0), (where, f)
    # 5. the scrub, whenever every file the index names is resident
    assert len(ws) == len(ref.files), where
    if {v[0] for v in backed.values()} <= set(ref.files):
        s = verify_index(ix, ws, ns, etag)
        assert s.clean and s.bad == [] and not s.per_fid, where
        assert s.n_checked == len(backed) and s.n_soft_deleted == soft and sum(s.by_class) == s.n_checked, where
        assert s.by_class[L.VFY_OK] == s.n_checked, where


def do_write(dev: DevDB, ref: LC.RefDB, step):
    batch = WriteBatch()
    for op in step.ops:
        if op.deleted:
            batch.delete(op.ns, op.key)
        else:
            batch.put(op.ns, op.key, op.val, W.Meta(expire=op.expire, etag=op.etag or None, flags=1 if op.tomb else 0,
                                                    app_meta=op.meta))
    assert dev.active.fid == step.fid
    locs, stats = dev.ix.write(dev.active, batch, dev.ws, ref.ns, ref.etag, stats_on_device=step.stats_on_device)
    assert locs == step.locs, f"batch {step.b}"
    assert stats == step.stats, f"batch {step.b}"
    assert dev.active.bytes() == ref.image(step.fid), f"batch {step.b}"


def do_compact(dev: DevDB, ref: LC.RefDB, step):
    sizes = {f: len(b) for f, b in sorted(dev.images.items())}
    assert sizes == step.sizes
    garbage = wal_garbage(dev.ix, sizes)
    assert garbage == step.garbage
    picked = default_compaction_picker([PickerWalInfo(f, sizes[f], garbage[f]) for f in sizes], LC.PICK_RATIO)
    assert picked == step.picked
    if step.rule is not None:
        dev.ix.set_compact_rules(**step.rule)
    dst, hint = W.WalFile(step.dst, BASE), W.WalFile(step.dst, BASE)
    srcs = [W.load_wal(dev.images[f], f) for f in picked]
    # the later compactions fan out over the database's context and the suite's
    res = IX.compact_wals_filtered(dst, hint, srcs, dev.ix, ref.ns, ref.etag,
                                   contexts=[dev.ctx, dev.peer] if step.fanout else None)
    assert len(res) == len(step.srcs)
    for (offs, kept), s in zip(res, step.srcs):
        assert kept == s.kept, s.fid
        assert offs.tolist() == s.offs.tolist(), s.fid
    assert bytes(dst.data) == ref.image(step.dst) and bytes(hint.data) == ref.hint_image(step.dst)
    if step.rule is not None:
        c = dev.ix.compact_rule_counts()
        assert [c["expired"], c["tombstone"], c["prefix"]] == step.counts
        dev.ix.clear_compact_rules()
    c = dev.ix.compact_rule_counts()
    assert [c["expired"], c["tombstone"], c["prefix"]] == [0, 0, 0]
    dev.images[step.dst], dev.hints[step.dst] = bytes(dst.data), bytes(hint.data)
    dev.ws.add(dst.as_wal())


def do_one_phase(dev: DevDB, ref: LC.RefDB, step):
    dres, ires = dev.ix.recover_segment(dev.hints[step.dst], L.MODE_HINT, step.dst, 40, BASE, ref.ns, 0,
                                        use_record_fid=True)
    assert dres.err_class == 0 and ires.err_class == 0
    assert ires.n_in == ires.n_done == step.n == dres.n_records
    # the hint's own fid is the call's fid here, so the line above cannot tell use_record_fid from its absence: the same
    # replay into an empty index under another fid argument must still put every row under the fid the hint carries
    probe = Index(dev.ctx, keys=1 << 10)
    try:
        probe.recover_segment(dev.hints[step.dst], L.MODE_HINT, step.dst + 100, 40, BASE, ref.ns, 0, use_record_fid=True)
        rows = LC.hint_rows(ref.hint_image(step.dst), ref.ns)
        assert probe.export() == {n + k: (f, o, s) for n, k, f, o, s in rows} and {r[2] for r in rows} == {step.dst}
    finally:
        probe.close()


def do_remove(dev: DevDB, ref: LC.RefDB, step):
    dev.remove(step.picked)
    if step.order == "A":
        return
    # order B: the files are gone and the index still names them. The scrub lists exactly those entries
    s = verify_index(dev.ix, dev.ws, ref.ns, ref.etag)
    assert s.n_bad == len(step.dangling)
    assert all(b.cls == L.VFY_NO_WAL and b.rd_status == 0 and b.rec_status == 0 for b in s.bad)
    assert {b.key: (b.fid, b.off, b.size) for b in s.bad} == step.dangling and len(s.bad) == len(step.dangling)
    assert s.by_class[L.VFY_NO_WAL] == s.n_bad and sum(s.by_class) == s.n_checked
    assert dict(s.per_fid) == expect_named(ref, step.dangling) and list(s.per_fid) == sorted(s.per_fid)
    dev.scrub_b = s.per_fid
    # 12. a snapshot of this very state, resynced to the files that exist
    snap = Index(dev.ctx, keys=1 << 10)
    try:
        snap.load_snapshot(step.snapshot)
        dev.retain_b = snap.retain_fids(step.surviving)
        assert snap.export() == {k: v for k, v in step.snapshot.items() if v[1] == 0 or v[0] in step.surviving}
    finally:
        snap.close()


def do_retire(dev: DevDB, ref: LC.RefDB, step):
    m = dev.ix.drop_fids(step.picked)
    assert dict(m) == usage_map(step.rows) == expect_named(ref, step.dangling) and list(m) == sorted(m)
    assert (m.soft_deleted, m.invalid, m.overflow) == (step.soft, 0, False)
    if step.order == "B":
        assert dict(dev.scrub_b) == dict(m)
        assert dict(dev.retain_b) == dict(m) and dev.retain_b.soft_deleted == m.soft_deleted


def do_restart(dev: DevDB, ref: LC.RefDB, step):
    dev.ix.clear()
    recover_from_wals(dev.ix, dev.files(), ref.ns, ref.etag)


def do_recover(dev: DevDB, ref: LC.RefDB, step):
    live = dev.ix.export()
    files = dev.files()
    assert sorted(files) == sorted(ref.files)
    for fanout in (False, True):
        ix2 = Index(dev.ctx, keys=1 << 10)
        try:
            recover_from_wals(ix2, files, ref.ns, ref.etag, contexts=[dev.ctx, dev.peer] if fanout else None)
            got = ix2.export()
            assert got == step.entries, f"fanout {fanout}"
            differ = {k for k in set(live) | set(got) if live.get(k) != got.get(k)}
            print(f"recovered against live: {len(differ)} of {len(ref.keys)} keys differ (fanout {fanout})")
            assert differ == set(step.differ)
            for k in step.must_agree:
                assert live[k] == got[k] and live[k][1] != 0, k
            m = ix2.retain_fids(sorted(files))
            assert dict(m) == {} and m.invalid == 0 and ix2.export() == got
        finally:
            ix2.close()


STEPS = {"write": do_write, "compact": do_compact, "one_phase": do_one_phase, "remove": do_remove, "retire": do_retire,
         "restart": do_restart, "recover": do_recover, "rotate": lambda dev, ref, step: dev.rotate(step.fid)}


def run(ctx, seed: int, ns_size: int = 20, etag_size: int = 20, **kw):
    """the run on a context of its own, opened and closed here; the suite's `ctx` is the second context of the
    fan-outs. A call into the index reserves one slot per row of its context's decode table, which only grows: on the
    suite's context, whether a call fits the index's bounds -- and with that, where the index grows and where it
    reclaims -- would depend on which tests ran before this one."""
    own = Context(0)
    ref = LC.RefDB(ns_size, etag_size)
    dev = None
    try:
        dev = DevDB(own, ctx, ns_size, etag_size, ref.active)
        first = prev = dev.ix.stats()
        check_state(dev, ref, "empty")
        n, purged, reclaim = 0, False, None
        for step in LC.lifecycle(ref, seed, **kw):
            STEPS[step.kind](dev, ref, step)
            n += 1
            where = f"step {n} ({step.kind}{' ' + str(step.b) if step.kind == 'write' else ''})"
            st = dev.ix.stats()
            print(f"{where}: {st.slot_capacity} slots, {st.slots_used} used, {st.live} live")
            if purged and reclaim is None and st.slots_used < prev.slots_used:
                # the automatic reclaim: this call did not fit, found at least half of the claimed slots dead and
                # rebuilt the index from its live keys before it ran. What is dead now, this step's Deletes left
                reclaim = where
                deletes = sum(op.kind == LC.DELETE for op in step.ops) if step.kind == "write" else 0
                assert st.live <= st.slots_used <= st.live + deletes, (where, prev, st)
            if step.kind == "write" and step.b == LC.PURGE_BATCH:
                purged = True
                assert 2 * st.live < st.slots_used, (where, st)  # more than half of the claimed slots are dead
            check_state(dev, ref, where)  # exact right after every step, the reclaiming one included
            prev = st
        print(f"{n} steps, {len(ref.keys)} keys, reclaim at {reclaim}")
        assert prev.slot_capacity > first.slot_capacity  # the index of 1024 keys grew under the run
        assert reclaim is not None or not purged
    finally:
        if dev is not None:
            dev.close()
        own.close()


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_lifecycle(ctx, seed):
    """ten batches (the ninth a purge), three compactions (the later ones over two contexts, the second with rules),
    both retirement orders, one restart, an automatic reclaim of the index, the recovery at the end"""
    run(ctx, seed)


@pytest.mark.parametrize("ns_size,etag_size", [(0, 0), (8, 16)])
def test_lifecycle_other_sizes(ctx, ns_size, etag_size):
    """four batches and one compaction at NsSize / EtagSize (0, 0) and (8, 16)"""
    run(ctx, LC.SEEDS[0], ns_size, etag_size, n_batches=4, compact_after=(4,), ruled_after=(), restart_after=())
