"""The colliding-key construction of tests/_collide.py, on the CPU: every key of both families has the wanted Sum64
under the oracle's murmur3 and under the library's host one, and the families have the shapes the device tests
(test_gpu_index_collisions.py) rely on. Those tests assume all of this and do not derive it again."""
from __future__ import annotations

import random

import pytest

import _collide as K
import _oracle as O
from bitcaskdb_amd import murmur3_sum64


@pytest.mark.parametrize("target", K.TARGETS)
def test_family_hashes_to_the_target(target):
    fam = K.family(target)
    for k in list(fam) + [K.outsider(target)]:
        assert K.sum64(k) == target, k.hex()
        assert O.murmur3_sum64(k) == target, k.hex()
        assert murmur3_sum64(k) == target, k.hex()


@pytest.mark.parametrize("target", K.TARGETS)
def test_family_shapes(target):
    fam = K.family(target)
    assert [len(k) for k in fam] == K.LENGTHS
    assert len(set(fam)) == len(fam) == 21 and K.outsider(target) not in fam
    assert fam == K.family(target)  # a fixed list
    assert [len(k) for k in fam.ns0] == [16, 17] and sorted(set(fam) - set(fam.ns20)) == sorted(fam.ns0)
    assert len(fam.unrelated) == 8 and len({k[:16] for k in fam.unrelated}) == 8
    a, b = fam.last_chunk
    assert a[:32] == b[:32] and a[32:] != b[32:]
    a, b = fam.chunk0
    assert a[:16] != b[:16] and a[16:] == b[16:]
    a, ax = fam.ext
    assert len(a) == 32 and len(ax) == 48 and ax[:32] == a
    a, b = fam.twins
    assert len(a) == len(b) == 47 and a[:32] == b[:32] and a[32:] != b[32:]
    assert [len(k) for k in fam.ragged] == [28, 44, 116]


def test_targets():
    assert K.H_WRAP & 0xFFFFFFFF == 0xFFFFFFFF and K.H_WRAP % 16 == 15 and K.H_ZERO == 0
    assert not set(K.family(K.H_WRAP)) & set(K.family(K.H_ZERO))


def test_python_murmur3_matches_the_oracle():
    rng = random.Random(3)
    for n in list(range(0, 70)) + [116, 255]:
        b = rng.randbytes(n)
        assert K.sum64(b) == O.murmur3_sum64(b), n
        assert K.sum128(b) == O.murmur3_128(b), n


def test_collide_random_triples():
    rng = random.Random(4)
    for i in range(200):
        prefix = rng.randbytes(16 * rng.randrange(0, 6))
        tail = rng.randbytes(rng.randrange(0, 16))
        after = rng.randbytes(16 * rng.randrange(0, 3)) if i % 4 == 0 else b""
        target = rng.choice([rng.getrandbits(64), K.H_WRAP, K.H_ZERO, 2 ** 64 - 1])
        k = K.collide(prefix, tail, target, rng.getrandbits(64), after=after)
        assert len(k) == len(prefix) + 16 + len(after) + len(tail)
        assert k[:len(prefix)] == prefix and k[len(k) - len(tail):] == tail
        assert O.murmur3_sum64(k) == target, (i, k.hex())


def test_tail_twins_random_bodies():
    rng = random.Random(5)
    for nb in (0, 16, 32, 64):
        body = rng.randbytes(nb)
        target = rng.getrandbits(64)
        a, b = K.tail_twins(body, target)
        assert a != b and len(a) == len(b) == nb + 15 and a[:nb] == b[:nb] == body
        assert O.murmur3_sum64(a) == O.murmur3_sum64(b) == target
