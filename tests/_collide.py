"""Keys with a chosen murmur3 Sum64 (MurmurHash3_x64_128, seed 0, first word): TEST INFRASTRUCTURE ONLY.

The hash is a chain of bijections on its state (h1, h2): every multiplier is odd, x ^= x >> 33 is its own inverse on 64
bits, and a body block, the tail and the finish can each be undone when the key bytes they consumed are known. So for
a wanted Sum64 and any 64-bit `salt` taken as the final h2 the state before the finish is determined; walking back over
the known tail and the known blocks behind the free one gives the state that block must produce, and its two words
follow from the state the prefix leaves. Pure Python, no GPU; test_collide_host.py checks every key it makes against
the oracle's and the library's murmur3."""
from __future__ import annotations

import random
import struct

M = (1 << 64) - 1
C1, C2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
N1, N2 = 0x52dce729, 0x38495ab5
F1, F2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53

H_WRAP = 0x9E3779B9FFFFFFFF  # h & mask is the table's last slot at every capacity (the chain wraps); h % 16 == 15
H_ZERO = 0                   # a hash of zero is a hash like any other
TARGETS = (H_WRAP, H_ZERO)


def _inv(c: int) -> int:
    return pow(c, -1, 1 << 64)


I5, IC1, IC2, IF1, IF2 = _inv(5), _inv(C1), _inv(C2), _inv(F1), _inv(F2)


def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (64 - r))) & M


def _rotr(x: int, r: int) -> int:
    return ((x >> r) | (x << (64 - r))) & M


def _m1(k: int) -> int:
    return _rotl(k * C1 & M, 31) * C2 & M


def _m2(k: int) -> int:
    return _rotl(k * C2 & M, 33) * C1 & M


def _m1_inv(x: int) -> int:
    return _rotr(x * IC2 & M, 31) * IC1 & M


def _m2_inv(x: int) -> int:
    return _rotr(x * IC1 & M, 33) * IC2 & M


def _fmix(k: int) -> int:
    k ^= k >> 33
    k = k * F1 & M
    k ^= k >> 33
    k = k * F2 & M
    return k ^ (k >> 33)


def _fmix_inv(k: int) -> int:
    k ^= k >> 33
    k = k * IF2 & M
    k ^= k >> 33
    k = k * IF1 & M
    return k ^ (k >> 33)


def _block(h1: int, h2: int, k1: int, k2: int):
    h1 = ((_rotl(h1 ^ _m1(k1), 27) + h2) * 5 + N1) & M
    h2 = ((_rotl(h2 ^ _m2(k2), 31) + h1) * 5 + N2) & M
    return h1, h2


def _unblock(h1: int, h2: int, k1: int, k2: int):
    """the state before a body block of known words, from the state after it"""
    p2 = _rotr(((h2 - N2) * I5 - h1) & M, 31) ^ _m2(k2)
    p1 = _rotr(((h1 - N1) * I5 - p2) & M, 27) ^ _m1(k1)
    return p1, p2


def _solve(p1: int, p2: int, h1: int, h2: int):
    """the words of the body block that takes the state (p1, p2) to (h1, h2)"""
    k1 = _m1_inv(_rotr(((h1 - N1) * I5 - p2) & M, 27) ^ p1)
    k2 = _m2_inv(_rotr(((h2 - N2) * I5 - h1) & M, 31) ^ p2)
    return k1, k2


def _words(b: bytes):
    """(k1, k2) of up to 16 bytes, little endian, absent bytes 0"""
    return int.from_bytes(b[:8], "little"), int.from_bytes(b[8:16], "little")


def _body(b: bytes, h1: int = 0, h2: int = 0):
    assert len(b) % 16 == 0
    for o in range(0, len(b), 16):
        h1, h2 = _block(h1, h2, *_words(b[o:o + 16]))
    return h1, h2


def _finish(h1: int, h2: int, n: int):
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M
    h2 = (h2 + h1) & M
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & M
    h2 = (h2 + h1) & M
    return h1, h2


def _unfinish(h1: int, h2: int, n: int):
    """the state after the tail of a key of n bytes whose 128-bit hash is (h1, h2)"""
    h2 = (h2 - h1) & M
    h1 = (h1 - h2) & M
    h1, h2 = _fmix_inv(h1), _fmix_inv(h2)
    h2 = (h2 - h1) & M
    h1 = (h1 - h2) & M
    return h1 ^ n, h2 ^ n


def sum128(b: bytes):
    nb = len(b) & ~15
    h1, h2 = _body(b[:nb])
    k1, k2 = _words(b[nb:])  # m(0) == 0: an absent tail half changes nothing
    return _finish(h1 ^ _m1(k1), h2 ^ _m2(k2), len(b))


def sum64(b: bytes) -> int:
    return sum128(b)[0]


def collide(prefix: bytes, tail: bytes, target: int, salt: int, after: bytes = b"") -> bytes:
    """prefix || 16 solved bytes || after || tail with Sum64 == target. len(prefix) and len(after) are multiples of 16
    (`after`: further body blocks behind the solved one), len(tail) < 16. Different salts give different solved bytes."""
    assert len(prefix) % 16 == 0 and len(after) % 16 == 0 and len(tail) < 16
    n = len(prefix) + 16 + len(after) + len(tail)
    h1, h2 = _unfinish(target & M, salt & M, n)
    k1, k2 = _words(tail)
    h1, h2 = h1 ^ _m1(k1), h2 ^ _m2(k2)
    for o in range(len(after) - 16, -1, -16):
        h1, h2 = _unblock(h1, h2, *_words(after[o:o + 16]))
    k1, k2 = _solve(*_body(prefix), h1, h2)
    return prefix + struct.pack("<QQ", k1, k2) + after + tail


def tail_twins(body: bytes, target: int):
    """two keys body || 15-byte tail, tails different, both with Sum64 == target: they differ only inside their last,
    ragged chunk. The tail's words are solved as a block's are; its second word has 7 bytes, so salts are tried until
    the solved word's top byte is zero (about one in 256)."""
    assert len(body) % 16 == 0
    p1, p2 = _body(body)
    n = len(body) + 15
    out = []
    salt = 0
    while len(out) < 2:
        salt = (salt + 0x9E3779B97F4A7C15) & M
        h1, h2 = _unfinish(target & M, salt, n)
        k2 = _m2_inv(h2 ^ p2)
        if k2 >> 56:
            continue
        key = body + struct.pack("<Q", _m1_inv(h1 ^ p1)) + struct.pack("<Q", k2)[:7]
        if key not in out:
            out.append(key)
    return out[0], out[1]


class Family(list):
    """the merged keys of one target, in chain order, with the groups by name:
    unrelated (8 x 48 B), last_chunk (2 x 48 B), chunk0 (2 x 32 B), ext (A of 32 B, A || X of 48 B), twins (2 x 47 B),
    ragged (28, 44 and 116 B), ns0 (16 and 17 B: shorter than a 20-byte namespace)"""

    def __init__(self, target: int, groups: dict):
        super().__init__(k for g in groups.values() for k in g)
        self.target, self.groups = target, groups

    def __getattr__(self, name):
        try:
            return self.__dict__["groups"][name]
        except KeyError:
            raise AttributeError(name) from None

    @property
    def ns20(self):
        """every key of at least 20 bytes (ns = key[:20])"""
        return [k for k in self if len(k) >= 20]


def family(target: int, seed: int = 1) -> Family:
    rng = random.Random(seed * 1_000_003 + (target & 0xFFFF))

    def salt():
        return rng.getrandbits(64)

    g = {}
    g["unrelated"] = [collide(rng.randbytes(32), b"", target, salt()) for _ in range(8)]
    p = rng.randbytes(32)
    g["last_chunk"] = [collide(p, b"", target, salt()) for _ in range(2)]
    tail16 = rng.randbytes(16)
    g["chunk0"] = [collide(b"", b"", target, salt(), after=tail16) for _ in range(2)]
    a = collide(rng.randbytes(16), b"", target, salt())
    g["ext"] = [a, collide(a, b"", target, salt())]
    g["twins"] = list(tail_twins(rng.randbytes(32), target))
    g["ragged"] = [collide(b"", rng.randbytes(12), target, salt()),
                   collide(rng.randbytes(16), rng.randbytes(12), target, salt()),
                   collide(rng.randbytes(96), rng.randbytes(4), target, salt())]
    g["ns0"] = [collide(b"", b"", target, salt()), collide(b"", rng.randbytes(1), target, salt())]
    return Family(target, g)


def outsider(target: int, seed: int = 1) -> bytes:
    """a 48-byte key with Sum64 == target that is in no family"""
    rng = random.Random(seed * 7_000_003 + 99 + (target & 0xFFFF))
    return collide(rng.randbytes(32), b"", target, rng.getrandbits(64))


LENGTHS = [48] * 8 + [48, 48] + [32, 32] + [32, 48] + [47, 47] + [28, 44, 116] + [16, 17]
