"""The device index gives back what removed keys used: the live-only rebuild (k_ix_compact) behind
Index.compact() / bcw_index_compact and behind the automatic policy of a batch that does not fit (rebuild at the
current capacities once half the claimed slots are dead, grow only if the batch still does not fit). Checked against
the index oracle (O.Index) and the capacity-bound policy model (_BoundModel); every index starts from a 1024-slot
table."""
from __future__ import annotations

import random

import pytest

import _oracle as O
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import index as IX
from test_gpu_index import _BoundModel, _keyset, check_against_oracle

pytestmark = pytest.mark.gpu

MAX_LOAD = 0.7  # kMaxLoad


@pytest.fixture
def new_index(ctx):
    """Index(ctx, ...) factory; the indexes are closed when the test ends, failed or not (an index must not outlive
    the session's context)"""
    made = []

    def make(**kw):
        made.append(IX.Index(ctx, **kw))
        return made[-1]

    yield make
    for ix in made:
        ix.close()


def _entry_bytes(mk: bytes) -> int:
    """one key's arena entry: 16 B header + the merged key padded to 16 (k_ix_commit's layout)"""
    return 16 + ((len(mk) + 15) & ~15)


def _pow2_at_least(v: int) -> int:
    p = 1024
    while p < v:
        p <<= 1
    return p


class _RoomReplay:
    """ix_room / ix_grow restated on the host, for the capacity bounds the churn tests assert: the host's upper bounds
    (every op of a batch may claim a slot and 31 B + its key in the arena), the counter sync when a batch does not
    fit them, the rebuild when half the claimed slots are dead, then the growth."""

    def __init__(self, cap=1024, arena_cap=1 << 20):
        self.cap, self.arena_cap = cap, arena_cap
        self.slots_ub = self.arena_ub = 0
        self.slots = self.arena = 0  # the device counters
        self.rebuilds = 0

    def _fits(self, n, ab):
        return self.slots_ub + n <= MAX_LOAD * self.cap and self.arena_ub + ab <= self.arena_cap

    def batch(self, n, key_bytes, claims, claim_bytes, live_before, live_bytes_before):
        """a batch of n ops (key_bytes of keys) that claims `claims` new slots / `claim_bytes` of arena, on an index
        holding live_before live keys whose entries take live_bytes_before"""
        ab = 31 * n + key_bytes
        if not self._fits(n, ab):
            self.slots_ub, self.arena_ub = self.slots, self.arena
            if self.slots > 0 and self.slots - live_before >= self.slots // 2:
                self.slots = self.slots_ub = live_before
                self.arena = self.arena_ub = live_bytes_before
                self.rebuilds += 1
            if not self._fits(n, ab):
                need_a = self.arena_ub + ab
                if need_a > self.arena_cap:
                    self.arena_cap = max(need_a, 2 * self.arena_cap)
                self.cap = max(self.cap, _pow2_at_least(int((self.slots_ub + n) / MAX_LOAD) + 1))
        self.slots_ub += n
        self.arena_ub += ab
        self.slots += claims
        self.arena += claim_bytes


def _random_batch(rng, keys, n, oc):
    ops, ks, fids, offs, sizes = [], [], [], [], []
    for _ in range(n):
        ns, k = rng.choice(keys)  # duplicates inside a batch: the last op wins
        op = rng.choice([0, 0, 0, 1, 1, 2])
        f, o, z = rng.randrange(1, 50), rng.randrange(40, 1 << 40), rng.randrange(5, 1 << 20)
        ops.append(op)
        ks.append(ns + k)
        fids.append(f)
        offs.append(o)
        sizes.append(z)
        oc.set(ns, k, op, f, o, z)
    return ops, ks, fids, offs, sizes


def _check_export(ix, oc):
    exp = ix.export()
    assert len(exp) == oc.live()
    for mk, v in exp.items():
        st, ov = oc.get(mk[:20], mk[20:])
        assert st != 1 and ov == v
    return exp


def test_compact_keeps_every_answer(new_index):
    """random Put / Delete / SoftDelete batches, then compact(): every Get (deleted keys not found, soft-deleted ones
    status 2 with their value), the export and the counters are the live set's; the index goes on working"""
    rng = random.Random(11)
    keys = _keyset(rng, 3000)  # merged lengths over every 16 B chunk edge (20 + 0, 1, 7, 8, 15, 16, 17, ... + digits)
    probe = keys + _keyset(random.Random(99), 50)
    ix = new_index(keys=1024, arena_bytes=1 << 16)
    oc = O.Index()
    for batch in range(10):
        ix.apply(*_random_batch(rng, keys, rng.choice([50, 2000, 2000, 9000]), oc))
    before = ix.stats()
    assert before.slots_used > before.live  # there is something dead to reclaim
    ix.compact()
    check_against_oracle(ix, oc, probe)
    st, _, off, _ = ix.get_many([ns + k for ns, k in keys])
    assert (st == 1).any() and (st == 2).any() and (off[st == 2] == 0).all()
    exp = _check_export(ix, oc)
    s = ix.stats()
    assert s.slots_used == s.live == oc.live()
    assert s.arena_used == sum(_entry_bytes(mk) for mk in exp)
    assert s.overflow == 0
    assert (s.slot_capacity, s.arena_capacity) == (before.slot_capacity, before.arena_capacity)
    for batch in range(3):
        ix.apply(*_random_batch(rng, keys, 2000, oc))
        check_against_oracle(ix, oc, probe)
    _check_export(ix, oc)
    assert ix.stats().overflow == 0


def test_compact_edge_tables(new_index):
    rng = random.Random(12)
    keys = [ns + k for ns, k in _keyset(rng, 700)]
    vals = [(1 + i % 7, 40 + i, 5 + i) for i in range(700)]
    f, o, z = zip(*vals)
    # an empty index
    ix = new_index(keys=1024)
    ix.compact()
    ix.compact(shrink=True)
    s = ix.stats()
    assert (s.live, s.slots_used, s.arena_used, s.slot_capacity, s.overflow) == (0, 0, 0, 1024, 0)
    # all live: 700 keys in 1024 slots (probe chains wrap past the end of the table); nothing changes
    ix.apply([L.IDX_PUT] * 700, keys, f, o, z)
    s0 = ix.stats()
    assert s0.slot_capacity == 1024 and s0.live == s0.slots_used == 700
    got0 = [a.copy() for a in ix.get_many(keys)]
    ix.compact()
    assert ix.stats() == s0
    for a, b in zip(got0, ix.get_many(keys)):
        assert (a == b).all()
    assert ix.export() == dict(zip(keys, vals))
    # all dead
    ix.apply([L.IDX_DELETE] * 700, keys)
    assert ix.stats().live == 0 and ix.stats().slots_used == 700
    ix.compact()
    s = ix.stats()
    assert (s.live, s.slots_used, s.arena_used, s.overflow) == (0, 0, 0, 0)
    assert (ix.get_many(keys)[0] == 1).all() and ix.export() == {}
    # the same keys again: they fit the table as it is
    ix.apply([L.IDX_PUT] * 700, keys, f, o, z)
    s1 = ix.stats()
    assert (s1.live, s1.slots_used, s1.arena_used, s1.slot_capacity) == (700, 700, s0.arena_used, s.slot_capacity)
    assert ix.export() == dict(zip(keys, vals))


def test_compact_shrink(new_index):
    rng = random.Random(13)
    keys = _keyset(rng, 20000)
    ix = new_index(keys=1024)
    oc = O.Index()
    mks = [ns + k for ns, k in keys]
    for i, (ns, k) in enumerate(keys):
        oc.set(ns, k, 0, 3, 40 + i, 9)
    ix.apply([L.IDX_PUT] * 20000, mks, [3] * 20000, [40 + i for i in range(20000)], [9] * 20000)
    assert ix.stats().slot_capacity >= 32768
    keep = set(rng.sample(range(20000), 300))
    gone = [i for i in range(20000) if i not in keep]
    for i in gone:
        oc.set(*keys[i], 1)
    ix.apply([L.IDX_DELETE] * len(gone), [mks[i] for i in gone])
    ix.compact(shrink=True)
    s = ix.stats()
    assert (s.slot_capacity, s.arena_capacity) == (1024, 1 << 20)
    assert s.live == s.slots_used == 300 and s.overflow == 0
    assert s.arena_used == sum(_entry_bytes(mks[i]) for i in keep)
    check_against_oracle(ix, oc, keys)
    # the shrunk table grows again
    more = [(b"Z" * 20, b"new%05d" % i) for i in range(2000)]
    for i, (ns, k) in enumerate(more):
        oc.set(ns, k, 0, 5, 77 + i, 11)
    ix.apply([L.IDX_PUT] * 2000, [ns + k for ns, k in more], [5] * 2000, [77 + i for i in range(2000)], [11] * 2000)
    s = ix.stats()
    assert s.live == oc.live() == 2300 and s.slot_capacity == 4096 and s.overflow == 0
    check_against_oracle(ix, oc, more)
    check_against_oracle(ix, oc, keys)


def test_bounded_index_churn_stays_bounded(new_index):
    """IndexLimited = 1024 under 40 batches of 500 never-seen keys: the index equals the policy model after every batch
    (the eviction order survives the rebuilds) and its HBM stays bounded.
    A growth happens only when fewer than half the claimed slots are dead, i.e. slots_used < 2 L at that moment, so
    slot_capacity <= pow2_at_least((2 L + n) / 0.7 + 1) = 4096, arena_used < 2 L E there, and ix_grow at most
    doubles what the batch needs: arena_capacity <= 2 (2 L E + 31 n + key bytes of a batch). The host replay of
    ix_room / ix_grow (_RoomReplay) confirms both caps before the device is asked."""
    limited, n, nb = 16 * 64, 500, 40
    E = _entry_bytes(bytes(270))
    assert E == 288
    slot_cap_max = _pow2_at_least(int((2 * limited + n) / MAX_LOAD) + 1)
    arena_cap_max = 2 * (2 * limited * E + 31 * n + 270 * n)
    assert slot_cap_max == 4096
    rng = random.Random(15)
    ix = new_index(keys=1024, arena_bytes=1 << 20)
    ix.set_limit(limited)
    m = _BoundModel(limited)
    rp = _RoomReplay()
    used, dropped = 0, False
    for batch in range(nb):
        ks = [bytes([65 + batch % 5]) * 20 + rng.randbytes(242) + b"%08d" % (batch * n + i) for i in range(n)]
        assert all(len(k) == 270 for k in ks)
        live_before = len(m.d)
        fs, os_, zs = [1 + batch] * n, [40 + i for i in range(n)], [rng.randrange(5, 1 << 20) for _ in range(n)]
        for k, f, o, z in zip(ks, fs, os_, zs):
            m.op(L.IDX_PUT, k, f, o, z)
        ix.apply([L.IDX_PUT] * n, ks, fs, os_, zs)
        m.bound()
        rp.batch(n, 270 * n, n, E * n, live_before, E * live_before)
        assert rp.cap <= slot_cap_max and rp.arena_cap <= arena_cap_max
        assert ix.export() == m.export(), batch
        s = ix.stats()
        assert (s.live, s.evicted, s.evicted_bytes, s.overflow) == (len(m.d), m.evicted, m.evicted_bytes, 0), batch
        assert s.slot_capacity <= slot_cap_max, (batch, s)
        assert s.arena_capacity <= arena_cap_max, (batch, s)
        dropped = dropped or s.slots_used < used
        used = s.slots_used
    assert dropped and rp.rebuilds > 0  # an automatic rebuild ran
    assert m.evicted > 0


def test_unbounded_delete_churn_stays_bounded(new_index):
    """20 rounds of 2000 new keys Put, then Deleted in a second batch. The live count is at most 2000 whenever ix_room
    reads the counters, so slots_used < 4000 at any growth and the capacity is at most pow2_at_least((4000 + 2000) /
    0.7 + 1) = 16384; the host replay shows 8192 to be tight (the first Delete batch reserves 2000 more slots on top
    of 2000 live ones, every later batch finds at least half the slots dead), and that is asserted."""
    n, rounds = 2000, 20
    rp = _RoomReplay()
    kb = 0
    for r in range(rounds):
        kb = sum(len(b"%c" % (65 + r % 5) * 20 + b"round%02d-%05d" % (r, i)) for i in range(n))
        eb = n * _entry_bytes(bytes(20 + 13))
        rp.batch(n, kb, n, eb, 0, 0)
        rp.batch(n, kb, 0, 0, n, eb)
    assert rp.cap == 8192 and rp.rebuilds > 0
    ix = new_index(keys=1024, arena_bytes=1 << 20)
    sample = []
    for r in range(rounds):
        ks = [bytes([65 + r % 5]) * 20 + b"round%02d-%05d" % (r, i) for i in range(n)]
        ix.apply([L.IDX_PUT] * n, ks, [1 + r] * n, [40 + i for i in range(n)], [7] * n)
        s = ix.stats()
        assert s.live == n and s.slot_capacity <= 8192 and s.overflow == 0, (r, s)
        ix.apply([L.IDX_DELETE] * n, ks)
        s = ix.stats()
        assert s.live == 0 and s.slot_capacity <= 8192 and s.overflow == 0, (r, s)
        sample += ks[::100]
    s = ix.stats()
    assert s.live == 0 and s.slot_capacity == rp.cap and s.arena_capacity == rp.arena_cap
    assert (ix.get_many(sample)[0] == 1).all()
    assert ix.export() == {}


def test_compact_between_bounded_batches(new_index):
    """test_index_capacity_bound_batches's loop (limited = 16 * 8) with an explicit compact() after every fifth batch:
    the index equals the policy model after every batch"""
    limited = 16 * 8
    rng = random.Random(limited)
    keys = [ns + k for ns, k in _keyset(rng, 4 * limited)]
    ix = new_index(keys=1024)
    ix.set_limit(limited)
    m = _BoundModel(limited)
    for batch in range(25):
        n = rng.choice([1, 7, 60, 400])
        ops, ks, fs, os_, zs = [], [], [], [], []
        for _ in range(n):
            op = rng.choice([0, 0, 0, 0, 0, 1, 2])
            k = rng.choice(keys)
            f, o, z = rng.randrange(1, 50), rng.randrange(40, 1 << 40), rng.randrange(5, 1 << 20)
            ops.append(op)
            ks.append(k)
            fs.append(f)
            os_.append(o)
            zs.append(z)
            m.op(op, k, f, o, z)
        ix.apply(ops, ks, fs, os_, zs)
        m.bound()
        if batch % 5 == 4:
            ix.compact()
            s = ix.stats()
            assert s.slots_used == s.live
        exp = ix.export()
        assert exp == m.export(), batch
        s = ix.stats()
        assert (s.live, s.limited, s.evicted, s.evicted_bytes, s.overflow) == (len(exp), limited, m.evicted,
                                                                              m.evicted_bytes, 0), batch
    assert m.evicted > 0
