"""Bit-exact parity of one device encode against the CPU oracle (test infrastructure): the compaction re-encode
against oc_compact_append and the hint rebuild against oc_hint_by_wal, on the appended bytes, the offsets and the
error outcome. Shared by tests/test_gpu_encode.py and tests/test_gpu_consumers.py."""
from __future__ import annotations

import random

import numpy as np

import _oracle as O
import cases
from bitcaskdb_amd import _lib as L

BASE = cases.BASE
U64MAX = np.iinfo(np.uint64).max


def prefill(rng, w, nbytes):
    while w.size() < nbytes:
        w.write(bytes(rng.getrandbits(8) for _ in range(rng.randrange(5, 3000))))


def run_compact(ctx, src, keep, ns=20, etag=20, dst_base=BASE, fid=9, pre_wal=0, pre_hint=0, seed=0, start_off=40,
                full=False):
    """full: return (EncodeResult, appended WAL bytes, appended hint bytes, rec_off) instead of the result alone"""
    rng = random.Random(seed)
    dst, hint = O.Writer(dst_base, dst_base), O.Writer(dst_base, dst_base)
    prefill(rng, dst, pre_wal)
    prefill(rng, hint, pre_hint)
    wal_pos, hint_pos = dst.size(), hint.size()
    ec, er, nin, offs = O.compact_append(dst, hint, fid, src, start_off, BASE, dst_base, ns, etag, keep)
    res, wal, hb, goffs = ctx.encode(src, L.ENC_COMPACT, start_off, dst_base, fid, wal_pos, hint_pos, ns, etag, keep)
    assert res.err_class == ec, (res.err_class, ec, res.err_record, er)
    if ec in (L.ENC_ERR_EXPIRE, L.ENC_ERR_PANIC) or (ec == L.ENC_ERR_SRC and er >= 0):
        assert res.err_record == er
    assert res.n_in == nin
    ref_wal, ref_hint = dst.data()[wal_pos:], hint.data()[hint_pos:]
    assert res.wal_end == dst.size() and res.hint_end == hint.size()
    assert len(wal) == len(ref_wal)
    if wal != ref_wal:
        d = next(i for i in range(len(wal)) if wal[i] != ref_wal[i])
        raise AssertionError(f"dst WAL differs at file offset {wal_pos + d} (appended byte {d} of {len(wal)})")
    if hb != ref_hint:
        d = next((i for i in range(min(len(hb), len(ref_hint))) if hb[i] != ref_hint[i]), min(len(hb), len(ref_hint)))
        raise AssertionError(f"hint WAL differs at appended byte {d} ({len(hb)} vs {len(ref_hint)})")
    np.testing.assert_array_equal(goffs[:nin], offs[:nin])
    assert res.n_written == int((offs[:nin] != U64MAX).sum())
    return (res, wal, hb, goffs) if full else res


def run_hint(ctx, src, ns=20, etag=20, fid=5, start_off=40):
    ec, er, nin, ref = O.hint_by_wal(src, fid, start_off, BASE, ns, etag)
    res, _, hb, _ = ctx.encode(src, L.ENC_HINT, start_off, BASE, fid, 40, 40, ns, etag)
    assert res.err_class == ec and res.n_in == nin
    assert hb == ref[40:], "hint WAL bytes differ"
    return res
