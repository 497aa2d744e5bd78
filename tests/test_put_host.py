"""CPU tests of the batched Write's host helpers (include/bcw.h): bcw_record_encode against the oracle's
Record.Encode (record.go:57-138) and bcw_write_bound against the oracle writer's growth (wal.go:490-553). No device."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
from bitcaskdb_amd import _lib as L

BASE = 1_700_000_000
BLOCK = 32768


def _ptr(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).ctypes.data_as(C.c_void_p) if b else None


def lib_encode(ns, key, val, etag=b"", expire=0, tombstone=False, meta=b"", base=BASE, etag_size=None, cap=None):
    mk = ns + key
    n = len(mk) + len(val) + len(etag) + len(meta) + 64 if cap is None else cap
    out = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    flags = (L.WR_TOMBSTONE if tombstone else 0) | (L.WR_ETAG if etag else 0)
    r = L.lib.bcw_record_encode(out.ctypes.data_as(C.c_void_p), n, _ptr(mk), len(mk), _ptr(val), len(val), _ptr(meta),
                                len(meta), _ptr(etag), expire, flags, len(etag) if etag_size is None else etag_size,
                                base, len(ns))
    return int(r), (bytes(out[:r]) if r >= 0 else None)


VAL_LENS = [0, 1, 15, 16, 17, 127, 128, 4096, 40000, 70000, 200000]
KEY_LENS = [0, 1, 127, 128, 300]


@pytest.mark.parametrize("ns_size", [0, 8, 20, 250])
def test_record_encode_matches_oracle(ns_size):
    rng = random.Random(ns_size)
    ns = bytes(rng.randrange(256) for _ in range(ns_size))
    n = 0
    for vl in VAL_LENS:
        for kl in KEY_LENS:
            for variant in range(6):
                key, val = rng.randbytes(kl), rng.randbytes(vl)
                etag = rng.randbytes(20) if variant & 1 else b""
                expire = BASE + rng.choice([0, 1, 127, 128, 3600, (1 << 35) - 1]) if variant & 2 else 0
                meta = rng.randbytes(rng.choice([1, 40, 300])) if variant >= 4 else b""
                tomb = variant == 3
                ref = O.record_encode(ns, key, val, etag, expire, tomb, meta, BASE)
                r, got = lib_encode(ns, key, val, etag, expire, tomb, meta)
                assert r == len(ref) and got == ref, (ns_size, vl, kl, variant)
                n += 1
    assert n == len(VAL_LENS) * len(KEY_LENS) * 6


def test_record_encode_header_size_truncates():
    ns = bytes(range(250))
    ref = O.record_encode(ns, b"k" * 300, b"v" * 128, b"e" * 20, BASE + 5, False, b"", BASE)
    r, got = lib_encode(ns, b"k" * 300, b"v" * 128, b"e" * 20, BASE + 5)
    assert got == ref
    hn = 2 + 250 + (2 + 2 + 1) + 20 + 1  # flags and size bytes, ns, three varints, etag, expire varint
    assert hn >= 256 and got[0] == hn & 0xFF  # byte(headerSize), record.go:109


def test_record_encode_errors():
    ns, key, val = b"n" * 20, b"key", b"value"
    assert O.record_encode(ns, key, val, b"", BASE - 1, False, b"", BASE) is None
    assert lib_encode(ns, key, val, expire=BASE - 1)[0] == -L.ENC_ERR_EXPIRE
    assert O.record_encode(ns, key, val, b"", BASE + 2 ** 35, False, b"", BASE) is None
    assert lib_encode(ns, key, val, expire=BASE + 2 ** 35)[0] == -L.ENC_ERR_PANIC
    assert lib_encode(ns, key, val, expire=BASE + 2 ** 35 - 1)[0] > 0
    assert lib_encode(ns, key, val, expire=BASE)[0] > 0  # a delta of 0 is encoded (one byte)
    # a merged key shorter than NsSize cannot be expressed
    out = np.zeros(64, dtype=np.uint8)
    r = L.lib.bcw_record_encode(out.ctypes.data_as(C.c_void_p), 64, _ptr(b"abc"), 3, None, 0, None, 0, None, 0, 0, 20,
                                BASE, 20)
    assert r == -L.ENC_ERR_BATCH
    # a buffer one byte short: nothing written
    full, _ = lib_encode(ns, key, val)
    r, _ = lib_encode(ns, key, val, cap=full - 1)
    assert r == -L.ENC_ERR_TABLE


def _random_batch(rng, ns_size, etag_size):
    recs = []
    for _ in range(rng.randrange(1, 40)):
        kl = rng.choice([0, 1, 16, 100, 127, 128, 300])
        vl = rng.choice([0, 1, 17, 128, 1000, 4096, 32700, 32761, 40000, 70000])
        etag = bytes(etag_size) if rng.random() < 0.5 else b""
        expire = BASE + rng.randrange(1, 1 << 34) if rng.random() < 0.5 else 0
        meta = bytes(rng.randrange(1, 200)) if rng.random() < 0.3 else b""
        recs.append((bytes(ns_size), bytes(kl), bytes(vl), etag, expire, meta))
    return recs


def test_write_bound_covers_the_writer():
    rng = random.Random(5)
    leftovers = list(range(0, 9)) + [32768]
    for it in range(200):
        ns_size, etag_size = rng.choice([(20, 20), (0, 0), (8, 16)])
        recs = _random_batch(rng, ns_size, etag_size)
        left = leftovers[it % len(leftovers)]
        # `left` bytes remain in the block at wal_pos (0: wal_pos is a block start written as a full block before it)
        wal_pos = 40 + (1 + it % 3) * BLOCK - left if left != 32768 else 40 + (it % 3) * BLOCK
        assert (BLOCK - (wal_pos - 40) % BLOCK) % BLOCK == left % BLOCK
        w = O.Writer(BASE, BASE, at=wal_pos)
        kb = vb = mb = 0
        for ns, key, val, etag, expire, meta in recs:
            w.write(O.record_encode(ns, key, val, etag, expire, False, meta, BASE))
            kb += len(ns) + len(key)
            vb += len(val)
            mb += len(meta)
        growth = w.size() - wal_pos
        bound = int(L.lib.bcw_write_bound(len(recs), kb, vb, mb, etag_size, wal_pos))
        assert bound >= growth, (it, wal_pos, bound, growth)


def test_write_batch_mirrors_batch_go():
    """WriteBatch: Put / Delete / Append / Size / ByteSize with Record.ApproximateSize (batch.go, record.go:50-55)"""
    from bitcaskdb_amd import WriteBatch
    from bitcaskdb_amd.wal import Meta
    ns = b"n" * 20

    def approx(key, val, etag=b"", app=0):  # 1 + len(ns) + 1 + 2 * 3 + len(etag) + 2 + key + value + AppMetaSize
        return 1 + len(ns) + 1 + 6 + len(etag) + 2 + len(key) + len(val) + app

    a, b = WriteBatch(), WriteBatch()
    a.put(ns, b"k1", b"v" * 100)
    a.put(ns, b"k2", b"w" * 7, Meta(expire=BASE + 5, etag=b"e" * 20, app_meta=b"\x81\xa1a\xa1b"), app_meta_size=2)
    a.delete(ns, b"k1")
    assert a.size() == 3
    assert a.byte_size() == approx(b"k1", b"v" * 100) + approx(b"k2", b"w" * 7, b"e" * 20, 2) + approx(b"k1", b"")
    b.put(ns, b"k3", b"", Meta(flags=1))
    a.append(b)
    a.append(None)
    assert a.size() == 4 and a.byte_size() == approx(b"k1", b"v" * 100) + approx(b"k2", b"w" * 7, b"e" * 20, 2) + \
        approx(b"k1", b"") + approx(b"k3", b"")
    keys, koff, vals, voff, metas, moff, etags, expire, flags = a.arrays(20)
    assert koff.tolist() == [0, 22, 44, 66, 88] and voff.tolist() == [0, 100, 107, 107, 107]
    assert moff.tolist() == [0, 0, 5, 5, 5] and expire.tolist() == [0, BASE + 5, 0, 0]
    assert flags.tolist() == [0, L.WR_ETAG, L.WR_TOMBSTONE | L.WR_DELETED, L.WR_TOMBSTONE]
    assert etags[20:40].tobytes() == b"e" * 20 and not etags[:20].any()
    a.clear()
    assert a.size() == 0 and a.byte_size() == 0
