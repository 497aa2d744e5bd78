"""One database's life, device-free: a seeded workload and the oracle-side database it runs on. TEST INFRASTRUCTURE ONLY.
Nothing here imports the library under test.

RefDB is the reference's chain restated with tests/_oracle.py (the C restatement) and plain Python, nothing of the
library under test:
  write       DBImpl.writeWal + writeIndex     db_impl.go:434-480   O.record_encode, O.Writer.write, O.Index.set and
                                                                    O.SMap.index_op for the WriteStat columns
  rotate      Manifest.RotateWal               manifest.go:249-273  a new active fid from GenFid (manifest.go:426-431)
  compact     doCompactionWork's loop          compaction.go:201-211, compactOneWal + doFilter compaction.go:294-348,
                                                                    the rules as rule_model() below states them
  one_phase   the hint replay                  compaction.go:248-251
  restart     recoverFromWals                  db_impl.go:268-314
  usage       what maybeScheduleCompaction (compaction.go:135-150) feeds the picker, exact instead of the manifest's
              freed-bytes estimate
and one operation the reference does not have:
  retire      bcw_index_drop_fids: every entry that still points into a deleted file becomes what a Delete leaves. The
              reference keeps such entries until its sampled eviction meets them; Get answers ErrKeyNotFound for them
              either way (getWalRef(fid) == nil, db_impl.go:574-577).

lifecycle() is the run: it applies one step to the RefDB and yields it, so whoever drives a second database through the
same steps compares the two after every step. Three things in the run are not in the reference's own schedule and are
there for a reason:
  * the active WAL is rotated after every compaction. The reference gives the merge output the next fid, above the
    active file's, and recovers in ascending fid (db_impl.go:274-281): a key kept in the output and rewritten later in
    the still-active, lower-numbered file recovers to the older record. With the rotation fid order is write order, so
    "recovered == live" is a property the run can assert for the keys it names.
  * the database restarts once between the two compactions. writeIndex never points the index at a tombstone record
    (db_impl.go:441-448: Delete / SoftDelete), so doFilter's index check drops every tombstone before a rule sees it;
    only recovery, which Puts every record it iterates (db_impl.go:307-313), leaves entries on tombstones. Without
    the restart the tombstone rule's counter is 0 for every seed.
  * batch 9 is a purge: a Delete of about 70 % of the live keys, followed by a third compaction and one more batch.
    A device index rebuilds itself from its live keys only when at least half of its claimed slots are dead at the
    moment a call does not fit its bounds; a mix of 10 % Deletes never gets there, and the restart starts the count of
    claimed slots afresh. After the purge more than half of the slots claimed since the restart are dead (RefDB counts
    them in `claimed`), so the next call that has to make room reclaims them.
"""
from __future__ import annotations

import random
from collections import defaultdict
from types import SimpleNamespace

import numpy as np

import _oracle as O
from golden import pyref
from test_usage_host import _picker_model

BASE = 1_700_000_000
BLOCK = 32768
PUT, DELETE, SOFT_DELETE = O.Index.PUT, O.Index.DELETE, O.Index.SOFT_DELETE
FOUND, NOT_FOUND, SOFT_DELETED = 0, 1, 2
MODE_RECORD, MODE_HINT = 0, 1
SOFT = "soft-deleted"  # vals' mark of a key whose last op is a tombstone Put
ROTATE_AT = 192 << 10
PICK_RATIO = 0.2
RULE_NOW = BASE + 100
META = b"\x81\xa3foo\xa3bar"
KEY_LENS = (0, 1, 9, 127, 300)
SEEDS = (11, 27, 58)
FIRST_FID = 2  # manifest.go:79
TOMB = 1 << 2  # tombstoneFieldBit (record.go:44-48)
PURGE_BATCH, PURGE_SHARE = 9, 0.7


class Op(SimpleNamespace):
    """one record of a batch: ns, key, val, etag, expire, tomb (a tombstone Put), deleted (Batch.Delete), meta"""

    @property
    def kind(self) -> int:
        return DELETE if self.deleted else SOFT_DELETE if self.tomb else PUT

    @property
    def mkey(self) -> bytes:
        return self.ns + self.key


def put_op(ns, key, val, etag=b"", expire=0, tomb=False, meta=b"", role="placed") -> Op:
    """role: what the workload meant by the record -- "fresh" (a key drawn from the whole key space), "redo" (a Put of
    an earlier key), "soft" (a tombstone Put of an earlier key), "delete", "placed" (sized by the file position)"""
    return Op(ns=ns, key=key, val=val, etag=etag, expire=expire, tomb=tomb, deleted=False, meta=meta, role=role)


def delete_op(ns, key, role="delete") -> Op:
    return Op(ns=ns, key=key, val=b"", etag=b"", expire=0, tomb=True, deleted=True, meta=b"", role=role)


class Source:
    """one source WAL of a compaction and the oracle's decode of it"""

    def __init__(self, data: bytes, ns_size: int, etag_size: int, fid: int):
        self.data, self.ns, self.etag, self.fid = data, ns_size, etag_size, fid
        self.dec = O.decode(data, 40, BASE, ns_size, etag_size)
        self.n = len(self.dec.recs)
        assert self.dec.err_class == 0 and (self.dec.recs["status"] == 0).all()

    def mkey(self, i: int) -> bytes:
        pay, r = self.dec.payloads[i], self.dec.recs[i]
        h, kl = int(r["hdr_size"]), int(r["key_len"])
        return pay[1:1 + self.ns] + pay[h:h + kl]


def first_rule(rule: dict, expire: int, flags: int, mkey: bytes):
    """the rule that drops a row, in the order the device counts them: 0 expired (meta.Expire != 0 && meta.Expire <=
    now), 1 tombstone (meta.IsTombstone()), 2 prefix (bytes.HasPrefix(MergedKey(ns, key), p)), None"""
    if rule["drop_expired"] and expire != 0 and expire <= rule["now"]:
        return 0
    if rule["drop_tombstones"] and flags & TOMB:
        return 1
    if any(mkey.startswith(p) for p in rule["prefixes"]):
        return 2
    return None


def rule_model(s: Source, oix, rule: dict | None):
    """doFilter (compaction.go:329-348) over a source: (the index-check mask, the mask after the user filter that
    `rule` stands for, rows dropped per rule). The callback is asked only about rows that passed the index check
    (compaction.go:339-345), and a row counts for the first rule that matches."""
    base, nv = oix.compact_filter(s.data, 40, BASE, s.ns, s.etag, s.fid, s.n)
    assert nv == s.n
    mask, counts = base.copy(), [0, 0, 0]
    for i in range(s.n):
        if base[i] and rule is not None:
            r = first_rule(rule, int(s.dec.recs["expire"][i]), int(s.dec.recs["flags"][i]), s.mkey(i))
            if r is not None:
                mask[i] = 0
                counts[r] += 1
    return base, np.asarray(mask), counts


def hint_rows(image: bytes, ns_size: int):
    """(ns, key, fid, off, size) of every row of a hint file (HintRecord.Decode, hint.go:50-84)"""
    dec = O.decode(image, 40, BASE, ns_size, 0, MODE_HINT)
    assert dec.err_class == 0 and (dec.recs["status"] == 0).all()
    out = []
    for pay in dec.payloads:
        st, f = pyref.hint_decode(pay, ns_size)
        assert st == 0
        h = f["hdr_size"]
        out.append((pay[:ns_size], pay[h:h + f["key_len"]], f["fid"], f["off"], f["size"]))
    return out


def data_rows(image: bytes, ns_size: int, etag_size: int):
    """(ns, key, foff - 7, size) of every row IterateRecord delivers (record.go:242-266)"""
    dec = O.decode(image, 40, BASE, ns_size, etag_size, MODE_RECORD)
    assert dec.err_class == 0 and (dec.recs["status"] == 0).all()
    out = []
    for r, pay in zip(dec.recs, dec.payloads):
        h, kl = int(r["hdr_size"]), int(r["key_len"])
        out.append((pay[1:1 + ns_size], pay[h:h + kl], int(r["foff"]) - 7, int(r["size"])))
    return out


class RefDB:
    def __init__(self, ns_size: int = 20, etag_size: int = 20):
        self.ns, self.etag = ns_size, etag_size
        self.files, self.hints = {}, {}  # fid -> O.Writer: the data WALs and the hint files
        self.oix = O.Index()
        self.om = O.SMap(1 << 20, 1 << 19, 32, 5)  # Limited above the key count: no eviction, the WriteStat source
        self.vals = {}      # merged key -> the last Put's value | SOFT; absent after a Delete
        self.keys = {}      # every (ns, key) ever written, in order
        self.last_op = {}   # merged key -> the kind of its last op
        self.lost = set()   # keys retire() took out of the index though vals calls them live
        self.claimed = set()  # keys that have held an index entry since the index was last built from nothing
        self.next_fid = FIRST_FID
        self.active = None
        # conservation columns, per fid: bytes Put under it, WriteStat bytes freed in it, bytes retired from it
        self.put_bytes, self.freed, self.retired = defaultdict(int), defaultdict(int), defaultdict(int)
        self._locs, self._stats = [], {}
        self.rotate()

    # ---- files ----
    def new_fid(self) -> int:
        self.next_fid += 1
        return self.next_fid - 1

    def rotate(self) -> int:
        self.active = self.new_fid()
        self.files[self.active] = O.Writer(BASE, BASE)
        return self.active

    def image(self, fid: int) -> bytes:
        return self.files[fid].data()

    def hint_image(self, fid: int) -> bytes:
        return self.hints[fid].data()

    def sizes(self, with_active: bool = True) -> dict:
        return {f: w.size() for f, w in sorted(self.files.items()) if with_active or f != self.active}

    def left(self) -> int:
        """bytes left in the active file's current block"""
        return BLOCK - (self.files[self.active].size() - 40) % BLOCK

    # ---- DBImpl.Write ----
    def write_op(self, op: Op):
        p = O.record_encode(op.ns, op.key, op.val, op.etag, op.expire, op.tomb, op.meta, BASE)
        off = self.files[self.active].write(p)
        kind, fid, size = op.kind, self.active, len(p)
        self.oix.set(op.ns, op.key, kind, fid, off, size)
        ff, fb = self.om.index_op(op.ns, op.key, kind, fid, off, size)
        self._stats[ff] = self._stats.get(ff, 0) + fb  # writeStats[stat.FreeWalFid] += stat.FreeBytes
        self.freed[ff] += fb
        if kind == PUT:
            self.put_bytes[fid] += size
            self.vals[op.mkey] = op.val
        elif kind == SOFT_DELETE:
            self.vals[op.mkey] = SOFT
        else:
            self.vals.pop(op.mkey, None)
        self.keys.setdefault((op.ns, op.key))
        if kind != DELETE:
            self.claimed.add(op.mkey)
        self.last_op[op.mkey] = kind
        self.lost.discard(op.mkey)
        self._locs.append((off, size))

    def end_batch(self):
        locs, stats = self._locs, self._stats
        self._locs, self._stats = [], {}
        return locs, stats

    def write(self, ops):
        """one batch: (locs, {FreeWalFid: FreeBytes})"""
        for op in ops:
            self.write_op(op)
        return self.end_batch()

    # ---- compaction ----
    def compact(self, src_fids, dst_fid: int, rule: dict | None):
        """the sources, in order, into a new dst / hint pair: per source the index-check mask, the mask after the
        rules, the dst offsets and the rows kept; the rule counters summed; the keys the rules dropped"""
        dst, hint = O.Writer(BASE, BASE), O.Writer(BASE, BASE)
        out, total, dropped = [], [0, 0, 0], []
        for fid in src_fids:
            s = Source(self.image(fid), self.ns, self.etag, fid)
            base, mask, counts = rule_model(s, self.oix, rule)
            ec, _, nin, offs = O.compact_append(dst, hint, dst_fid, s.data, 40, BASE, BASE, self.ns, self.etag, mask)
            assert ec == 0 and nin == s.n
            out.append(SimpleNamespace(fid=fid, base=base, mask=mask, offs=offs[:nin], kept=int(mask.sum()),
                                       keys=[s.mkey(i) for i in range(s.n)],
                                       foff=[int(v) - 7 for v in s.dec.recs["foff"]]))
            total = [a + b for a, b in zip(total, counts)]
            dropped += [s.mkey(i) for i in range(s.n) if base[i] and not mask[i]]
        self.files[dst_fid], self.hints[dst_fid] = dst, hint
        return out, total, dropped

    def one_phase(self, dst_fid: int) -> int:
        """onePhase's replay of the new hint file: Put(ns, key, h.fid, h.off, h.size)"""
        img = self.hint_image(dst_fid)
        rows = hint_rows(img, self.ns)
        for ns, key, fid, off, size in rows:
            assert fid == dst_fid
            ff, fb = self.om.index_op(ns, key, PUT, fid, off, size)
            self.freed[ff] += fb
            self.put_bytes[fid] += size
        ec, n = self.oix.put_segment(img, 40, BASE, self.ns, 0, MODE_HINT, dst_fid, use_rec_fid=True)
        assert ec == 0 and n == len(rows)
        return n

    def dangling(self, fids) -> dict:
        """the entries that point into `fids`: {merged key: (fid, off, size)}"""
        fids, out = set(fids), {}
        for ns, key in self.keys:
            st, v = self.oix.get(ns, key)
            if st == FOUND and v[0] in fids:
                out[ns + key] = v
        return out

    def remove_files(self, fids):
        for f in fids:
            self.files.pop(f, None)
            self.hints.pop(f, None)

    def retire(self, fids):
        """drop_fids: ({fid: (count, bytes, span)} ascending, soft-deleted entries that stay)"""
        rows = {}
        for mk, (f, o, s) in self.dangling(fids).items():
            ns, key = mk[:self.ns], mk[self.ns:]
            self.oix.set(ns, key, DELETE)
            self.om.index_op(ns, key, DELETE)
            c, b, sp = rows.get(f, (0, 0, 0))
            rows[f] = (c + 1, b + s, sp + O.wal_record_size(o, s))
            self.retired[f] += s
            self.lost.add(mk)
        return {f: rows[f] for f in sorted(rows)}, self.usage()[1]

    # ---- state ----
    def entries(self) -> dict:
        """every live entry, a soft-deleted one as (0, 0, 0)"""
        out = {}
        for ns, key in self.keys:
            st, v = self.oix.get(ns, key)
            if st != NOT_FOUND:
                out[ns + key] = v
        return out

    def usage(self):
        """({fid: (count, bytes, span)} ascending over the file-backed entries, soft-deleted count)"""
        rows, soft = {}, 0
        for f, o, s in self.entries().values():
            if o == 0:
                soft += 1
                continue
            c, b, sp = rows.get(f, (0, 0, 0))
            rows[f] = (c + 1, b + s, sp + O.wal_record_size(o, s))
        return {f: rows[f] for f in sorted(rows)}, soft

    def garbage(self, sizes: dict) -> dict:
        use = self.usage()[0]
        return {f: sz - 40 - (use[f][2] if f in use else 0) for f, sz in sizes.items()}

    def conserved(self) -> bool:
        """per fid: bytes Put under it - WriteStat bytes freed in it - bytes retired from it == its live bytes"""
        use = self.usage()[0]
        fids = set(self.put_bytes) | set(self.freed) | set(self.retired) | set(use)
        return all(self.put_bytes[f] - self.freed[f] - self.retired[f] == (use[f][1] if f in use else 0)
                   for f in fids if f != 0)

    def recovered(self, index=None):
        """recoverFromWals over the files as they are: a fresh O.Index (or `index`: an O.Index / O.SMap)"""
        x = index if index is not None else O.Index()
        for fid in sorted(self.files):
            if fid in self.hints:
                ec, _ = x.put_segment(self.hint_image(fid), 40, BASE, self.ns, 0, MODE_HINT, fid)
            else:
                ec, _ = x.put_segment(self.image(fid), 40, BASE, self.ns, self.etag, MODE_RECORD, fid)
            assert ec == 0
        return x

    def recovery_puts(self):
        """the Put stream of that recovery, for a second restatement of the index: (ns, key, fid, off, size)"""
        for fid in sorted(self.files):
            if fid in self.hints:
                yield from ((ns, k, fid, o, s) for ns, k, _, o, s in hint_rows(self.hint_image(fid), self.ns))
            else:
                yield from ((ns, k, fid, o, s) for ns, k, o, s in data_rows(self.image(fid), self.ns, self.etag))

    def restart(self):
        """the process ends and the database is opened again: the index is what recovery makes of the files, and Get
        answers from it -- a deleted or soft-deleted key whose tombstone record is still on disk is found again"""
        self.oix = self.recovered()
        self.om = self.recovered(O.SMap(1 << 20, 1 << 19, 32, 5))
        self.lost = set()
        self.claimed = set(self.entries())
        for ns, key in self.keys:
            st, (f, o, s) = self.oix.get(ns, key)
            if st == NOT_FOUND:
                self.vals.pop(ns + key, None)
                continue
            assert st == FOUND
            rd, pay = O.read_record(self.image(f), o, s)
            assert rd == 0, "a recovered entry that cannot be read: a zero-length First survived to the restart"
            r = O.record_parse(pay, BASE, self.ns, self.etag)
            h, kl, vl = int(r["hdr_size"]), int(r["key_len"]), int(r["val_len"])
            self.vals[ns + key] = pay[h + kl:h + kl + vl]
        use = self.usage()[0]
        self.put_bytes = defaultdict(int, {f: u[1] for f, u in use.items()})
        self.freed, self.retired = defaultdict(int), defaultdict(int)

    def expect_get(self, ns: bytes, key: bytes):
        """what DBImpl.Get answers: NOT_FOUND, SOFT_DELETED, or the value's bytes"""
        st, (f, _, _) = self.oix.get(ns, key)
        if st != FOUND:
            return st
        if f not in self.files:
            return NOT_FOUND  # getWalRef(fid) == nil
        return self.vals[ns + key]

    def self_consistent(self):
        """vals, the two restatements of the index and the conservation columns tell one story"""
        for ns, key in self.keys:
            mk = ns + key
            st, v = self.oix.get(ns, key)
            mst, mv = self.om.index_get(ns, key)
            assert st == mst and (st != FOUND or v == mv), mk
            want = self.vals.get(mk)
            if mk in self.lost:
                assert st == NOT_FOUND and want is not None, mk
            elif want is None:
                assert st == NOT_FOUND, mk
            elif want is SOFT:
                assert st == SOFT_DELETED, mk
            else:
                assert st == FOUND, mk
        assert self.conserved()


# ---- the workload -------------------------------------------------------------------------------------------------
def namespaces(ns_size: int):
    return [(b"ns-%d-lifecycle-padding-" % i)[:ns_size] for i in range(3)]


def key_space(ns_size: int):
    """600 (ns, key): user keys of 0, 1, 9, 127 and 300 bytes; the first byte of a key cycles through 'a'..'e'"""
    rng = random.Random(600)
    out = []
    for j in range(200):
        kl = 0 if j == 0 else 1 if j <= 40 else KEY_LENS[2 + j % 3]
        body = bytes([0x40 + j]) if kl == 1 else (b"abcde"[j % 5:j % 5 + 1] + b"%05d-" % j + rng.randbytes(300))[:kl]
        out += [(ns, body) for ns in namespaces(ns_size)]
    return out


def rules_of(ns_size: int) -> dict:
    """the second compaction's rules: one namespace plus a 1-byte key prefix"""
    return dict(now=RULE_NOW, drop_expired=True, drop_tombstones=True, prefixes=(namespaces(ns_size)[1] + b"c",))


BIG = {(2, 50): 40000, (3, 60): 70000, (5, 40): 40000}
BIG_LATE = ((3, 60),)  # the large values placed late in their block
QUIRK_KEY, EXACT_KEY, PAD_KEY = b"zero-length-first", b"fill-exact", b"fill-pad3"


class Workload:
    def __init__(self, seed: int, ns_size: int, etag_size: int):
        self.rng = random.Random(seed)
        self.ns_size, self.etag_size = ns_size, etag_size
        self.space = key_space(ns_size)
        self.ns0 = namespaces(ns_size)[0]
        self.seen = []  # keys written so far (the placed records' keys are not among them: never overwritten)
        self.spacers = 0

    def _fill(self, ref: RefDB, key: bytes, delta: int):
        """a Put whose payload is the room of the active file's current block + delta, as
        test_gpu_put.py::Built.put_filling places it"""
        if ref.left() < 7 + 400:
            self.spacers += 1
            yield put_op(self.ns0, b"spacer-%d" % self.spacers, bytes(1000))
        target = ref.left() - 7 + delta
        vl = target - len(O.record_encode(self.ns0, key, b"", b"", 0, False, b"", BASE))
        for _ in range(4):  # the value varint's own length moves the payload length
            vl += target - len(O.record_encode(self.ns0, key, bytes(vl), b"", 0, False, b"", BASE))
        yield put_op(self.ns0, key, random.Random(vl).randbytes(vl))

    def _value_len(self) -> int:
        r = self.rng.random()
        if r < 0.4:
            return self.rng.choice([0, 1, 15, 16, 17, 127, 128])
        return self.rng.randrange(4097) if r < 0.65 else self.rng.randrange(600)

    def batch(self, b: int, ref: RefDB):
        """the ops of batch b, one at a time: the caller writes each into `ref` before it asks for the next, since a
        placed record is sized by the active file's position"""
        rng = self.rng
        if b == PURGE_BATCH:
            for ns, key in list(ref.keys):
                if isinstance(ref.vals.get(ns + key), bytes) and ns + key not in ref.lost and rng.random() < PURGE_SHARE:
                    yield delete_op(ns, key, role="purge")
            return
        redo, dele, soft = (0.5, 0.6, 0.7) if b > 1 else (0.15, 0.2, 0.25)
        for i in range(rng.randint(150, 250)):
            if (b, i) == (1, 20):    # exactly 7 bytes remain in the block: the next record's First holds no byte
                yield from self._fill(ref, b"before-" + QUIRK_KEY, -7)
                assert ref.left() == 7
                yield put_op(self.ns0, QUIRK_KEY, rng.randbytes(100))
            elif (b, i) == (2, 30):  # ends its block exactly
                yield from self._fill(ref, EXACT_KEY, 0)
            elif (b, i) == (3, 30):  # leaves 3 bytes: the next record starts after a pad
                yield from self._fill(ref, PAD_KEY, -3)
            elif (b, i) in BIG_LATE:  # leaves 2000 bytes: the large value after it goes through Middle fragments
                yield from self._fill(ref, b"before-big-%d" % b, -2000)
            r = rng.random()
            old = bool(self.seen) and r < soft
            ns, key = rng.choice(self.seen) if old else self.space[rng.randrange(len(self.space))]
            if old and redo <= r < dele and (b, i) not in BIG:
                yield delete_op(ns, key)
                continue
            variant = rng.randrange(8)
            etag = rng.randbytes(self.etag_size) if variant & 1 and self.etag_size else b""
            expire = BASE + rng.choice([1, 3600]) if variant & 2 else 0
            meta = META if variant & 4 else b""
            vl = BIG.get((b, i), self._value_len())
            tomb = old and r >= dele and (b, i) not in BIG
            if not old:
                self.seen.append((ns, key))
            yield put_op(ns, key, rng.randbytes(vl), etag, expire, tomb, meta,
                         role="soft" if tomb else "redo" if old else "fresh")


def lifecycle(ref: RefDB, seed: int, n_batches: int = 10, compact_after=(4, 8, 9), ruled_after=(8,),
              restart_after=(6,)):
    """the run. Every step has been applied to `ref` when it is yielded, and carries what the reference chain returned
    for it; the last step, "recover", changes nothing. Retirement order A (first compaction): the index drops the
    picked fids, then their images go; order B (any later one): the images go first."""
    assert PURGE_BATCH not in restart_after
    wl = Workload(seed, ref.ns, ref.etag)
    rounds = 0
    for b in range(1, n_batches + 1):
        fid, ops = ref.active, []
        for op in wl.batch(b, ref):
            ref.write_op(op)
            ops.append(op)
        locs, stats = ref.end_batch()
        yield SimpleNamespace(kind="write", b=b, fid=fid, ops=ops, locs=locs, stats=stats, stats_on_device=bool(b & 1),
                              claimed=len(ref.claimed), live=len(ref.entries()))
        if ref.files[ref.active].size() > ROTATE_AT:
            yield SimpleNamespace(kind="rotate", fid=ref.rotate())
        if b in compact_after:
            rounds += 1
            sizes = ref.sizes(with_active=False)
            garbage = ref.garbage(sizes)
            picked = _picker_model([(f, sizes[f], garbage[f]) for f in sizes], PICK_RATIO)
            rule = rules_of(ref.ns) if b in ruled_after else None
            dst = ref.new_fid()
            srcs, counts, dropped = ref.compact(picked, dst, rule)
            backed = ref.dangling(picked)
            yield SimpleNamespace(kind="compact", b=b, round=rounds, sizes=sizes, garbage=garbage, picked=picked,
                                  rule=rule, dst=dst, srcs=srcs, counts=counts, rule_dropped=dropped,
                                  rule_dropped_backed=[k for k in dropped if k in backed], fanout=rounds > 1)
            yield SimpleNamespace(kind="one_phase", dst=dst, n=ref.one_phase(dst))
            dangling = ref.dangling(picked)
            if rounds == 1:
                rows, soft = ref.retire(picked)
                yield SimpleNamespace(kind="retire", order="A", picked=picked, rows=rows, soft=soft, dangling=dangling)
                ref.remove_files(picked)
                yield SimpleNamespace(kind="remove", order="A", picked=picked, dangling={})
            else:
                snapshot = ref.entries()
                ref.remove_files(picked)
                yield SimpleNamespace(kind="remove", order="B", picked=picked, dangling=dangling, snapshot=snapshot,
                                      surviving=sorted(ref.files))
                rows, soft = ref.retire(picked)
                yield SimpleNamespace(kind="retire", order="B", picked=picked, rows=rows, soft=soft, dangling=dangling)
            yield SimpleNamespace(kind="rotate", fid=ref.rotate())
        if b in restart_after:
            ref.restart()
            yield SimpleNamespace(kind="restart")
    rec = ref.recovered()
    differ, must_agree = [], []
    for ns, key in ref.keys:
        a, c = ref.oix.get(ns, key), rec.get(ns, key)
        if (a[0], a[1] if a[0] == FOUND else None) != (c[0], c[1] if c[0] == FOUND else None):
            differ.append(ns + key)
        mk = ns + key
        if ref.last_op[mk] == PUT and isinstance(ref.vals.get(mk), bytes) and mk not in ref.lost:
            must_agree.append(mk)
    entries = {}
    for ns, key in ref.keys:
        st, v = rec.get(ns, key)
        if st != NOT_FOUND:
            entries[ns + key] = v
    yield SimpleNamespace(kind="recover", entries=entries, differ=differ, must_agree=must_agree)
