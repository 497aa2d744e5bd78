"""CPU checks of the lifecycle run (tests/_lifecycle.py) that test_gpu_lifecycle.py drives the device through: the
workload has the shapes it is there for, for every committed seed, and the oracle chain is self-consistent -- vals, the
O.Index, the O.SMap and golden/pyref.py's PyIndex (a second restatement of index.go:81-165) agree on every key after
every step, and the per-fid conservation identity holds at every step:
    bytes Put under the fid (writes and the hint replay) - WriteStat bytes freed in it - bytes retired from it
        == the bytes of the live entries that point into it
A SoftDelete and a Delete free what they replace (index.go:134-137, 157-160) and put nothing, which is why the left
side counts IDX_PUT sizes only."""
from __future__ import annotations

import pytest

import _lifecycle as LC
import _oracle as O
from golden import pyref

BLOCK = LC.BLOCK


def _same(ref: LC.RefDB, py: pyref.PyIndex, step):
    for ns, key in ref.keys:
        st, v = ref.oix.get(ns, key)
        pst, pv = py.get(ns, key)
        assert st == pst and (st != LC.FOUND or v == pv), (step.kind, ns + key)


def _mirror(ref: LC.RefDB, py: pyref.PyIndex, step) -> pyref.PyIndex:
    """the step on the second restatement of the index"""
    if step.kind == "write":
        for op, (off, size) in zip(step.ops, step.locs):
            if op.kind == LC.PUT:
                py.put(op.ns, op.key, step.fid, off, size)
            elif op.kind == LC.DELETE:
                py.delete(op.ns, op.key)
            else:
                py.soft_delete(op.ns, op.key)
    elif step.kind == "one_phase":
        for ns, key, fid, off, size in LC.hint_rows(ref.hint_image(step.dst), ref.ns):
            py.put(ns, key, fid, off, size)
    elif step.kind == "retire":
        for mk in step.dangling:
            py.delete(mk[:ref.ns], mk[ref.ns:])
    elif step.kind == "restart":
        py = pyref.PyIndex()
        for ns, key, fid, off, size in ref.recovery_puts():
            py.put(ns, key, fid, off, size)
    return py


def _shapes(writes):
    """test_gpu_put.py::test_batch_has_the_shapes' arithmetic over every file's locs: (zero-length Firsts, records with
    Middle fragments, records that end their block exactly, records written after a pad)"""
    by_fid = {}
    for st in writes:
        by_fid.setdefault(st.fid, []).extend(st.locs)
    zero = middle = exact = pad = 0
    for locs in by_fid.values():
        room = [BLOCK - (o - 40) % BLOCK - 7 for o, _ in locs]
        zero += sum(1 for r in room if r == 0)
        middle += sum(1 for r, (_, s) in zip(room, locs) if s - r > 2 * (BLOCK - 7))
        exact += sum(1 for r, (_, s) in zip(room, locs) if s == r)
        ends = [O.wal_record_size(o, s) + o for o, s in locs]
        pad += sum(1 for (o, _), e in zip(locs[1:], ends) if 0 < o - e < 7)
    return zero, middle, exact, pad


def _run(seed, ns_size=20, etag_size=20, **kw):
    ref, py, steps = LC.RefDB(ns_size, etag_size), pyref.PyIndex(), []
    for step in LC.lifecycle(ref, seed, **kw):
        py = _mirror(ref, py, step)
        _same(ref, py, step)
        ref.self_consistent()
        if step.kind == "compact":  # what only this moment shows: the state between the compaction and the retirement
            quirk = LC.namespaces(ns_size)[0] + LC.QUIRK_KEY
            step.quirk_row = [(int(s.base[i]), ref.vals.get(quirk)) for s in step.srcs
                              for i, k in enumerate(s.keys) if k == quirk]
        steps.append(step)
    return ref, steps


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_workload_has_the_shapes(seed):
    ref, steps = _run(seed)
    writes = [s for s in steps if s.kind == "write"]
    compacts = [s for s in steps if s.kind == "compact"]
    assert [s.b for s in writes] == list(range(1, 11))
    purge = writes.pop(LC.PURGE_BATCH - 1)
    assert all(150 <= len(s.ops) <= 250 + 5 for s in writes)
    assert len({s.fid for s in writes[:8]}) >= 4
    assert sum(sum(sz for _, sz in s.locs) for s in writes) < 2 << 20
    assert len({op.mkey for s in writes for op in s.ops}) <= 600 + 8
    assert {len(op.key) for s in writes for op in s.ops} >= set(LC.KEY_LENS)
    # the later batches' mix: about 50 % re-Puts, 10 % Deletes and 10 % tombstone Puts of earlier keys. Of ~1 500 draws
    # the standard deviation of a 10 % share is 0.8 points and of the 50 % share 1.3: the bands are over three wide
    roles = [op.role for s in writes[1:] for op in s.ops if op.role != "placed"]
    assert len(roles) > 1200
    share = {r: roles.count(r) / len(roles) for r in ("redo", "delete", "soft", "fresh")}
    assert 0.45 <= share["redo"] <= 0.55 and 0.07 <= share["delete"] <= 0.13 and 0.07 <= share["soft"] <= 0.13, share
    for s in writes[1:]:
        first = {}
        for i, op in enumerate(s.ops):
            first.setdefault(op.mkey, i)
        earlier = {op.mkey for w in writes if w.b < s.b for op in w.ops}
        assert all(op.mkey in earlier or first[op.mkey] < i for i, op in enumerate(s.ops)
                   if op.role in ("redo", "delete", "soft"))
    # the purge leaves more than half of the slots claimed since the restart dead
    assert all(op.role == "purge" and op.kind == LC.DELETE for op in purge.ops) and len(purge.ops) > 100
    assert 2 * purge.live < purge.claimed
    # every compaction picks, one of the first two picks two files
    assert [c.b for c in compacts] == [4, 8, 9] and all(c.picked for c in compacts)
    assert any(len(c.picked) == 2 for c in compacts[:2])
    assert [c.rule is not None for c in compacts] == [False, True, False]
    # the zero-length First: one in the whole run, dropped by the first compaction's index check while its key is live
    zero, middle, exact, pad = _shapes(writes)
    assert zero == 1 and middle >= 1 and exact >= 1 and pad >= 1
    assert compacts[0].quirk_row == [(0, compacts[0].quirk_row[0][1])] and isinstance(compacts[0].quirk_row[0][1], bytes)
    assert compacts[1].quirk_row == [] and compacts[2].quirk_row == []
    # every rule drops rows, and some of them still hold their key's index entry until the retirement
    assert all(c > 0 for c in compacts[1].counts) and compacts[0].counts == [0, 0, 0]
    assert len(compacts[1].rule_dropped) == sum(compacts[1].counts) and compacts[1].rule_dropped_backed
    # order B's scrub has something to find, and the second write into a survivor frees bytes of the dst fid
    removes = [s for s in steps if s.kind == "remove"]
    assert [r.order for r in removes] == ["A", "B", "B"] and removes[1].dangling
    assert writes[4].stats.get(compacts[0].dst, 0) > 0 and purge.stats.get(compacts[1].dst, 0) > 0
    assert writes[-1].b == 10 and writes[-1].stats.get(compacts[2].dst, 0) > 0
    # the recovery at the end: the keys the run says must agree do, and some keys differ (a Delete's record is Put)
    rec = steps[-1]
    assert rec.kind == "recover" and rec.must_agree and not set(rec.must_agree) & set(rec.differ)
    assert len(rec.must_agree) > 100


@pytest.mark.parametrize("ns_size,etag_size", [(0, 0), (8, 16)])
def test_other_sizes_run(ns_size, etag_size):
    ref, steps = _run(LC.SEEDS[0], ns_size, etag_size, n_batches=4, compact_after=(4,), ruled_after=(), restart_after=())
    compacts = [s for s in steps if s.kind == "compact"]
    assert len(compacts) == 1 and compacts[0].picked
    zero, middle, exact, pad = _shapes([s for s in steps if s.kind == "write"])
    assert zero == 1 and middle >= 1 and exact >= 1 and pad >= 1
    (keep, val), = compacts[0].quirk_row  # the zero-length First is in a picked file: dropped while its key is live
    assert keep == 0 and isinstance(val, bytes)
    rec = steps[-1]
    assert rec.must_agree and not set(rec.must_agree) & set(rec.differ)


def test_write_replays():
    """RefDB.write of a step's recorded ops on a second database gives the same locs, stats and bytes"""
    ref, other = LC.RefDB(), LC.RefDB()
    step = next(LC.lifecycle(ref, LC.SEEDS[0]))
    locs, stats = other.write(step.ops)
    assert (locs, stats) == (step.locs, step.stats) and other.image(other.active) == ref.image(step.fid)
