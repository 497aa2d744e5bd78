"""WAL test inputs mirroring the reference tests plus the branch fixtures SURVEY.md 4 asks for.
Built with the oracle writer (tests only). Each builder returns (file_bytes, params dict)."""
from __future__ import annotations

import hashlib
import random
import struct

import numpy as np

import _oracle as O

BASE = 1_700_000_000


def sha1(s: str) -> bytes:
    return hashlib.sha1(s.encode()).digest()


def params(ns=20, etag=20, start_off=40, base=BASE, mode=0):
    return dict(ns_size=ns, etag_size=etag, start_off=start_off, base_time=base, mode=mode)


def wal_of(payloads, base=BASE, create=None):
    w = O.Writer(create if create is not None else base, base)
    offs = [w.write(p) for p in payloads]
    return w.data(), offs


def rec(i, vlen=11, ns=20, etag=b"", expire=0, tomb=False, meta=b"", base=BASE, klen=None):
    key = (b"key-%06d" % i) if klen is None else bytes((i * 7 + k) & 0xff for k in range(klen))
    rng = random.Random(i)
    val = bytes(rng.getrandbits(8) for _ in range(vlen))
    return O.record_encode(sha1("ns")[:ns] if ns <= 20 else bytes(ns), key, val, etag, expire, tomb, meta, base)


# --- reference test scenarios (restated) ---
def case_iterator_basic():
    """wal_iterator_test.go:11-40: 1000 tiny payloads "0".."999" (not valid records: invalid data)."""
    data, _ = wal_of([str(i).encode() for i in range(1000)])
    return data, params()


def case_iterator_large():
    """wal_iterator_test.go:42-74: 1024 x 5 KiB payloads (spanning records)."""
    blob = (b"01234567" * 128) * 5
    data, _ = wal_of([blob] * 1024)
    return data, params()


def case_large_record():
    """wal_test.go:73-94: one 64 KiB record -> First/Middle/Last."""
    data, _ = wal_of([bytes(i % 256 for i in range(65536))])
    return data, params()


def case_records_mixed():
    """record_test.go:43-147 shapes (etag, expire, tombstone, meta, empty value) inside a WAL."""
    etag = sha1("etag")
    ps = []
    for i in range(300):
        k = i % 4
        if k == 0:
            ps.append(rec(i, 11, etag=etag, expire=BASE + 60, tomb=True, meta=b"\x81\xa3foo\xa3bar"))
        elif k == 1:
            ps.append(rec(i, 11, etag=etag, expire=BASE + 61))
        elif k == 2:
            ps.append(rec(i, 0, etag=etag, expire=BASE + 62, tomb=True, meta=b"\x81\xa3foo\xa3bar"))
        else:
            ps.append(rec(i, 0))
    data, _ = wal_of(ps)
    return data, params()


def case_config_shape(n=400, vlen=4096):
    """config A/B shape: ns 20, key 100, value 4096, no etag/expire/meta."""
    data, _ = wal_of([rec(i, vlen, klen=100) for i in range(n)])
    return data, params()


# --- branch fixtures ---
def case_padding():
    """leftover < 7 at a block end (wal.go:507-512): first record leaves 3 bytes in block 0."""
    first = bytes(32768 - 7 - 3)  # 32758 B record -> 32765 bytes used, 3 left -> padding
    data, _ = wal_of([first, rec(1, 100), rec(2, 50000), rec(3, 10)])
    return data, params()


def case_zero_first():
    """leftover == 7 (wal.go:518-519): a zero-length First fragment, offset re-captured."""
    first = bytes(32768 - 7 - 7)  # leaves exactly 7 bytes
    data, _ = wal_of([first, rec(1, 200), rec(2, 10)])
    return data, params()


def case_zipf(n=600, seed=42):
    rng = np.random.default_rng(seed)
    ps = [rec(i, int(128 * min(rng.zipf(1.1), 512)), klen=100) for i in range(n)]
    data, _ = wal_of(ps)
    return data, params()


def case_sparse_multi(n=6000, seed=7):
    """Long runs of single-window fragments between rare multi-window ones: a 64-fragment window
    can hold few body windows, so one CRC pass spans many fragment windows."""
    rng = np.random.default_rng(seed)
    ps = []
    for i in range(n):
        r = rng.random()
        v = int(rng.integers(200, 70000)) if r < 0.03 else int(rng.integers(1, 60))
        ps.append(rec(i, v, klen=int(rng.integers(1, 40))))
    data, _ = wal_of(ps)
    return data, params()


def case_tail_garbage():
    """file with < 7 trailing bytes after the last fragment (ignored) and a truncated last block."""
    data, _ = wal_of([rec(i, 300) for i in range(20)])
    return data + b"\x01\x02\x03", params()


def case_truncated_record():
    """a First fragment at EOF without its Last: silently dropped (ErrWalIteratorEOF)."""
    data, _ = wal_of([rec(0, 100), rec(1, 40000)])
    return data[:40 + 32768 + 100], params()


def case_zero_tail():
    """an all-zero region after valid data: masked CRC of empty != 0 -> CRC error."""
    data, _ = wal_of([rec(i, 100) for i in range(5)])
    return data + bytes(64), params()


def case_bad_type():
    """valid CRC, unknown type byte 9 (ErrWalUnknownRecordType)."""
    data, _ = wal_of([rec(i, 100) for i in range(5)])
    b = bytearray(data)
    # rewrite the 3rd fragment's type: header offsets follow Full records of equal size
    flen = len(rec(0, 100))
    h = 40 + 2 * (7 + flen)
    b[h + 6] = 9
    return bytes(b), params()


def case_out_of_order():
    """Middle/Last without First, Full after First, First after First (crafted, valid CRCs)."""
    w = O.Writer(BASE, BASE)
    # hand-frame fragments: use the writer on pieces then patch types
    pieces = [rec(0, 50), rec(1, 60), rec(2, 70), rec(3, 80), rec(4, 90), rec(5, 30)]
    offs = [w.write(p) for p in pieces]
    b = bytearray(w.data())
    b[offs[0] + 6] = 4   # Last with no First: emitted alone
    b[offs[1] + 6] = 2   # First ...
    b[offs[2] + 6] = 1   # ... then Full: Full's data with First's offset
    b[offs[3] + 6] = 2   # First
    b[offs[4] + 6] = 2   # First again (appended)
    b[offs[5] + 6] = 4   # Last: concatenation of 3 fragments -> invalid data
    return bytes(b), params()


def case_clamped():
    """a length field larger than the block: clamped (wal_iterator.go:75), then CRC fails."""
    data, _ = wal_of([rec(i, 100) for i in range(3)])
    b = bytearray(data)
    b[40 + 4] = 0xff
    b[40 + 5] = 0xff
    return bytes(b), params()


def case_start_off(delta):
    data, _ = wal_of([rec(i, 500) for i in range(100)])
    return data, params(start_off=40 + delta)


def case_panic_records():
    """records that make RecordFromBytes panic or fail validation."""
    ns = 20
    good = rec(0, 10)
    # expire flag clear but etag field extends beyond the data
    p1 = bytearray(good)
    p1[1 + ns] = 0  # flags: etag present, expire present
    # keyLen huge so that the uint64 sum wraps
    hdr = bytes([0]) + sha1("ns")[:ns] + bytes([3])
    big = O.put_uvarint(1 << 63) + O.put_uvarint(1 << 63) + O.put_uvarint(0)
    body = hdr + big
    p2 = bytearray(body)
    p2[0] = len(body) & 0xff
    # length exactly min header (1+ns+1+3) with mismatching header size
    p3 = bytes([9]) + bytes(ns) + bytes([3, 0, 0, 0])
    data, _ = wal_of([good, bytes(p1), bytes(p2), p3, bytes(4), rec(5, 10)])
    return data, params()


def case_hint(n=500):
    """a hint WAL rebuilt from a data WAL (hint.go:123-161)."""
    data, p = case_config_shape(n, 300)
    ec, _, _, hint = O.hint_by_wal(data, 7, 40, BASE, 20, 20)
    assert ec == 0
    return hint, params(mode=1)


def filler(i: int, total: int) -> bytes:
    """a valid record of exactly `total` payload bytes"""
    v = total - len(rec(i, 0))
    for _ in range(4):
        r = rec(i, v)
        if len(r) == total:
            return r
        v -= len(r) - total
    raise AssertionError("no record of that size")


# --- hand-framed sources: fragment sequences WalIterator.Next accepts and the writer never produces ---
BLOCK, HDR = 32768, 7
FULL, FIRST, MIDDLE, LAST = 1, 2, 3, 4


class Framer:
    """A WAL image laid out fragment by fragment as WalIterator.Next walks it (wal_iterator.go:40-100): 32 KiB
    blocks counted from start_off, a 7-byte header (masked CRC of the data, u16 length, type) per fragment, zero fill
    when fewer than 7 bytes are left in a block. The bytes between the super block and start_off are zero."""

    def __init__(self, start_off=40, base=BASE):
        self.start = start_off
        self.buf = bytearray(O.Writer(base, base).data()[:40]) + bytes(start_off - 40)

    @property
    def pos(self) -> int:
        return len(self.buf)

    def room(self) -> int:
        """data bytes the next fragment can hold (after the zero fill of a block end too short for a header)"""
        left = BLOCK - (len(self.buf) - self.start) % BLOCK
        if left < HDR:
            self.buf += bytes(left)
            left = BLOCK
        return left - HDR

    def put(self, typ: int, data: bytes) -> int:
        """one fragment; returns the file offset of its header"""
        assert len(data) <= self.room(), "a fragment never crosses a block"
        off = len(self.buf)
        self.buf += struct.pack("<IHB", O.compute_crc32(data), len(data), typ) + data
        return off

    def record(self, payload: bytes, cuts=()) -> int:
        """payload cut at `cuts` and wherever a block ends, typed First / Middle.. / Last (Full when it is one
        fragment). Without cuts this is the writer's framing (wal.go:490-553). Returns the first header's offset."""
        offs = []
        for _, piece in split(payload, cuts):
            while len(piece) > self.room():
                r = self.room()
                offs.append(self.put(MIDDLE, piece[:r]))
                piece = piece[r:]
            offs.append(self.put(MIDDLE, piece))
        if len(offs) == 1:
            self.buf[offs[0] + 6] = FULL
        else:
            self.buf[offs[0] + 6], self.buf[offs[-1] + 6] = FIRST, LAST
        return offs[0]

    def data(self) -> bytes:
        return bytes(self.buf)


def split(payload: bytes, cuts):
    """payload cut at the positions `cuts` (repeats give zero-length pieces) -> [(type, data)]"""
    edges = [0] + sorted(cuts) + [len(payload)]
    assert 0 <= edges[1] and edges[-2] <= len(payload)
    pieces = [payload[a:b] for a, b in zip(edges, edges[1:])]
    if len(pieces) == 1:
        return [(FULL, pieces[0])]
    return [(FIRST, pieces[0])] + [(MIDDLE, p) for p in pieces[1:-1]] + [(LAST, pieces[-1])]


def frame(frags, start_off=40) -> bytes:
    """the file image of the (type, data) fragments `frags`, in order, from start_off on"""
    f = Framer(start_off)
    for typ, data in frags:
        f.put(typ, data)
    return f.data()


def rec_any(rng, i, vlen=None, base=BASE):
    """a valid record of a random kind: etag, expire, tombstone, meta (AppMetaSize 0 ones too), key lengths with
    one- and two-byte varints"""
    etag = sha1("etag%d" % i) if rng.random() < 0.4 else b""
    expire = base + rng.choice([0, 1, 127, 128, 100000, 1 << 30]) if rng.random() < 0.4 else 0
    meta = rng.choice([b"", b"", b"", b"\x81\xa3foo\xa3bar", b"\x80", b"\x81\xa0\xa0"])
    klen = rng.choice([None, None, 0, 1, 40, 130, 300])
    v = vlen if vlen is not None else rng.choice([0, 1, 13, 60, 200, 1000])
    return rec(i, v, etag=etag, expire=expire, tomb=rng.random() < 0.2, meta=meta, base=base, klen=klen)


def _checked(data, p, payloads=None, last_invalid=False):
    """a builder's own preconditions, from the oracle: no fragment error, every row OK (but a deliberate last one)"""
    d = O.decode(data, p["start_off"], p["base_time"], p["ns_size"], p["etag_size"], p["mode"])
    assert d.err_class == 0
    st = d.recs["status"]
    assert (st[:-1] == 0).all() and st[-1] == (1 if last_invalid else 0)
    if payloads is not None:
        assert d.payloads == payloads
    return d


def case_irregular_shapes():
    """every fragment sequence the iterator accepts and the writer never writes, then writer-framed records and one
    deliberately invalid last row (it pins n_in of the consumers)"""
    etag, meta = sha1("etag"), b"\x81\xa3foo\xa3bar"
    f, ps = Framer(), []

    def R(i, vlen, **kw):
        ps.append(rec(i, vlen, **kw))
        return ps[-1]

    f.record(R(0, 60, etag=etag, expire=BASE + 60), cuts=[30])          # First + Last in one block
    p = R(1, 40, tomb=True, meta=meta)
    f.record(p, cuts=[0, 0, 25, 25, len(p)])                            # zero-length First, Middle and Last
    f.put(FIRST, b"dangling-first")
    f.put(FULL, R(2, 33, meta=b"\x80"))                                 # Full after First; AppMetaSize 0
    f.put(LAST, R(3, 0))                                                # a lone Last
    f.record(R(4, 80, etag=etag, klen=30), cuts=range(1, 97))           # 96 one-byte fragments
    a = f.room() - 3                                                    # a First that leaves 3 bytes in its block,
    f.record(R(5, a + 32762 + 50, expire=BASE + 61), cuts=[a, a + 32761, a + 32762])  # a full-block Middle, 1 byte
    p = R(6, 34000, etag=etag, tomb=True, meta=meta)
    f.record(p, cuts=[20, 21, 21, 48, 300, len(p) - 600, len(p) - 599, len(p) - 590])  # multi-block, short Middles
    for i in range(7, 13):
        f.record(R(i, (0, 11, 300, 5000)[i % 4], etag=etag if i % 2 else b"", expire=BASE + 62 if i % 3 else 0,
                   meta=meta if i % 5 == 0 else b""))
    ps.append(b"\x05garbage-bytes")
    f.put(FULL, ps[-1])
    data, p = f.data(), params()
    d = _checked(data, p, ps, last_invalid=True)
    fr = d.frags
    assert int(d.recs["foff"][2]) == int(fr["data_off"][d.recs["first_frag"][2] - 1])  # the dangling First's offset
    assert (fr["len"] == 32761).any() and (fr["len"] == 0).sum() >= 4
    return data, p


def _random_cuts(rng, f, payload, big=False):
    if big:  # irregular Middles: clusters of short pieces anywhere in the value
        cuts = []
        for _ in range(rng.randrange(2, 6)):
            c = rng.randrange(0, len(payload))
            cuts += [c, min(len(payload), c + rng.choice([0, 1, 6, 7, 100]))]
        return f.record(payload, cuts)
    if rng.random() < 0.25:
        return f.record(payload)  # the writer's framing
    return f.record(payload, [rng.randrange(0, len(payload) + 1) for _ in range(rng.randrange(0, 5))])


def case_irregular_random(n=300, nbig=20, seed=5):
    """records of every kind cut at 0-4 random points (inside the header, namespace, key, varints, meta), ~20 of
    33-120 KB cut into irregular Middles (>= 3 destination fragments from an irregular source), writer-framed ones
    interleaved"""
    rng = random.Random(seed)
    f, ps = Framer(), []
    big = set(rng.sample(range(n), nbig))
    for i in range(n):
        ps.append(rec_any(rng, i, rng.randrange(33000, 120000) if i in big else None))
        _random_cuts(rng, f, ps[-1], i in big)
    data, p = f.data(), params()
    d = _checked(data, p, ps)
    f0, f1 = d.recs["first_frag"], d.recs["emit_frag"]
    blk = (d.frags["data_off"] - 40) // BLOCK
    assert int(((f0 != f1) & (blk[f0] == blk[f1])).sum()) >= 100
    return data, p


def case_irregular_hint(n=300, seed=6):
    """a hint WAL (hint.go:32-48 records) framed as case_irregular_random frames records"""
    rng = random.Random(seed)
    f, ps = Framer(), []
    for i in range(n):
        klen = rng.randrange(33000, 40000) if i % 75 == 7 else rng.choice([0, 1, 8, 40, 121, 122, 300])
        key = b"%06d" % i + bytes((i * 7 + k) & 0xff for k in range(klen))
        ps.append(O.hint_encode(sha1("ns")[:20], key, rng.randrange(1, 1 << 20), rng.randrange(40, 1 << 40),
                                rng.randrange(5, 1 << 20)))
        _random_cuts(rng, f, ps[-1], klen > 30000)
    data, p = f.data(), params(mode=1)
    d = _checked(data, p, ps)
    assert int((d.recs["first_frag"] != d.recs["emit_frag"]).sum()) >= 100
    return data, p


def shifted(data: bytes, p: dict, delta: int):
    """`delta` zero bytes after the super block and start_off moved with them: the same fragments, every offset
    `delta` higher"""
    q = dict(p)
    q["start_off"] = p["start_off"] + delta
    return data[:40] + bytes(delta) + data[40:], q


def corrupt(data: bytes, rng: random.Random, nflips: int = 1) -> bytes:
    b = bytearray(data)
    for _ in range(nflips):
        i = rng.randrange(40, len(b))
        b[i] ^= 1 << rng.randrange(8)
    return bytes(b)


ALL = {
    "iterator_basic": case_iterator_basic,
    "iterator_large": case_iterator_large,
    "large_record": case_large_record,
    "records_mixed": case_records_mixed,
    "config_shape": case_config_shape,
    "padding": case_padding,
    "zero_first": case_zero_first,
    "zipf": case_zipf,
    "sparse_multi": case_sparse_multi,
    "sparse_multi_dense": lambda: case_sparse_multi(4000, 11),
    "tail_garbage": case_tail_garbage,
    "truncated_record": case_truncated_record,
    "zero_tail": case_zero_tail,
    "bad_type": case_bad_type,
    "out_of_order": case_out_of_order,
    "clamped": case_clamped,
    "start_off_plus4": lambda: case_start_off(4),
    "start_off_plus7": lambda: case_start_off(7),
    "start_off_minus40": lambda: case_start_off(-40),
    "start_off_beyond": lambda: case_start_off(10_000_000),
    "panic_records": case_panic_records,
    "hint": case_hint,
    "irregular_shapes": case_irregular_shapes,
    "irregular_random": case_irregular_random,
    "irregular_hint": case_irregular_hint,
}
