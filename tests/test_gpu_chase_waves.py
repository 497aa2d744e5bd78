"""k_chase's several-wave workgroup (bcw_decode.hip: wave 0 chases and sums, the helper waves compute the held
headers' check words and resolve the wave boundaries, then every wave stores): the smallest shapes at which the
split between the waves, between the held headers and a block's tail, and between the boundaries resolved from LDS
and those left to the tail can go wrong. Every case is compared with the CPU oracle column by column
(_parity.full_parity) on a context of its own, with the direct predecessor sum and with the look-back, with the
per-XCD weights on (three decodes in a row: the weights, and with them every boundary, move between decodes) and
off."""
from __future__ import annotations

import numpy as np
import pytest

import _oracle as O
import cases
from _parity import full_parity
from bitcaskdb_amd import _lib as L

pytestmark = pytest.mark.gpu

BLOCK = 32768
# (BCW_OPT_CHASE_DIRECT 0: the look-back; None: its default), BCW_OPT_XCD_BALANCE
SETTINGS = [(None, 1), (None, 0), (0, 1), (0, 0)]
SETTING_IDS = ["direct-xbal", "direct-equal", "lookback-xbal", "lookback-equal"]


def check(data, direct, xbal, name):
    from bitcaskdb_amd import Context
    c = Context(0)
    try:
        if direct is not None:
            c.set_option(L.OPT_CHASE_DIRECT, direct)
        c.set_option(L.OPT_XCD_BALANCE, xbal)
        got = ref = None
        for i in range(3 if xbal else 1):
            got, ref = full_parity(c, data, cases.params(), f"{name} decode {i}")
        return got, ref
    finally:
        c.close()


def headers_per_block(data):
    """header count of every 32 KiB block (the oracle's fragment table)"""
    ref = O.decode(data, 40, cases.BASE, 20, 20, 0, want_bytes=False)
    blk = (ref.frags["data_off"].astype(np.int64) - 7 - 40) // BLOCK
    return np.bincount(blk)


@pytest.fixture(scope="module")
def hold_edge():
    """blocks with 64 (ending exactly at the block's end: the next block's first fragment is adjacent), 65, 66 and 63
    headers, in one segment"""
    sizes = [505] * 64 + [497] * 64 + [505] + [497] * 65 + [513] * 63
    rng = np.random.default_rng(7)
    data, _ = cases.wal_of([rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes])
    return data


@pytest.fixture(scope="module")
def config_b_shape():
    return O.synth(3 << 20, 0, 42)


@pytest.mark.parametrize("direct,xbal", SETTINGS, ids=SETTING_IDS)
def test_hold_edge(hold_edge, direct, xbal):
    """the held / tail split on each side of kChaseHold = 64"""
    n = headers_per_block(hold_edge)
    assert n.tolist() == [64, 65, 66, 63], n
    check(hold_edge, direct, xbal, "hold edge")


@pytest.mark.parametrize("direct,xbal", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("size,vlen,per_block", [(300 << 10, 0, 249), (3 << 20, 10, 231)],
                         ids=["300k", "3m-two-workgroups"])
def test_boundaries_in_tails(size, vlen, per_block, direct, xbal):
    """249 (value length 0) and 231-232 (value length 10) headers per block and hundreds of wave boundaries per block:
    most boundaries lie past the 64th header, and a workgroup has many batches of boundaries"""
    data = O.synth(size, 0, 11, 20, 100, vlen, 0)
    n = headers_per_block(data)
    assert n[:-1].min() == per_block and n[:-1].max() <= per_block + 1, n
    assert (len(n) > 64) == (size > (2 << 20)), n
    check(data, direct, xbal, f"tails {size}")


@pytest.mark.parametrize("direct,xbal", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("length", [40 + 1 * BLOCK, 40 + 2 * BLOCK, 40 + 64 * BLOCK, 40 + 65 * BLOCK,
                                    40 + 65 * BLOCK - 3, 40 + 65 * BLOCK + 3])
def test_block_multiples(config_b_shape, length, direct, xbal):
    """exact multiples of the block (P_nwaves = L lies at the last block's end), one full workgroup, a second
    workgroup with one block, a last block cut 3 bytes short (its last fragment fails its CRC) and a last block of 3
    bytes, shorter than a header (the panic class)"""
    data = config_b_shape[:length]
    assert len(data) == length
    got, ref = check(data, direct, xbal, f"multiple {length}")
    want = {40 + 65 * BLOCK - 3: L.ERR_CRC, 40 + 65 * BLOCK + 3: L.ERR_PANIC}.get(length, L.ERR_NONE)
    assert ref.err_class == want == got.result.err_class


@pytest.mark.parametrize("direct,xbal", SETTINGS, ids=SETTING_IDS)
def test_tiny(direct, xbal):
    """30 records: every one of the 4,097 boundaries falls in one block"""
    data = cases.wal_of([cases.rec(i, vlen=100 + i) for i in range(30)])[0]
    check(data, direct, xbal, "tiny")
