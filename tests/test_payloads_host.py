"""CPU pin of the enumerated payload sources (tests/_payloads.py) that test_gpu_parse.py judges the device by: on
every source the oracle (tests/_oracle.py) equals the independent restatement (golden/pyref.py) on the error class, the
fragment table and every column of every row, the partial fields of rejected rows included; and the sources reach what
they are built to reach, counted from the oracle's tables alone -- every status class a family can produce at that
size, and enough valid rows on each side of the windows of the decode's byte reader (RegReader, bcw_decode.hip: a 64 B
head clipped to the first fragment, a 32 B second window, walk_byte for the rest). These are conditions, not
measurements: a source that stops meeting one fails here, before a GPU test silently checks less."""
from __future__ import annotations

import collections
import os
import sys

import numpy as np
import pytest

import _oracle as O
import _payloads as PL

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref as P  # noqa: E402

OK, INVALID, PANIC = 0, 1, 2
MIN_ROWS = 8


def oracle_equals_pyref(src):
    """err_class, the fragment table, every row column and the payload bytes (test_irregular_oracle_vs_pyref's
    mapping); returns the oracle's decode"""
    p = src.params
    mode, ns, etag = p["mode"], p["ns_size"], p["etag_size"]
    a = PL.decode(src)
    b = P.iterate(src.data, p["start_off"], p["base_time"], ns, etag, mode)
    assert a.err_class == b["err_class"] == 0
    assert len(a.frags) == len(b["frags"])
    for k in ("data_off", "len", "stored_crc", "type", "crc_ok"):
        assert [int(x) for x in a.frags[k]] == [f[k] for f in b["frags"]], k
    assert len(a.recs) == len(b["recs"]) == len(src.rows)
    cols = {"foff": "foff", "size": "size", "status": "status", "first_frag": "first_frag", "emit_frag": "emit_frag",
            "key_len": "key_len", "hdr_size": "hdr_size"}
    cols.update({"flags": "flags", "etag_off": "etag_off", "val_len": "val_len", "meta_len": "meta_len",
                 "expire": "expire"} if mode == 0 else {"expire": "fid", "val_len": "off", "meta_len": "hint_size"})
    for i, (got, want) in enumerate(zip(a.recs, b["recs"])):
        for k, pk in cols.items():
            assert int(got[k]) == want[pk], (src.rows[i], k, int(got[k]), want[pk])
        assert a.payloads[i] == want["payload"] == src.payloads[i], src.rows[i]
    return a


def by_family(src, d):
    seen = collections.defaultdict(set)
    for row, st in zip(src.rows, d.recs["status"]):
        seen[row[0]].add(int(st))
    return seen


def frag_lens(d):
    """per row: the length of its first fragment, of its second (None for a one-fragment row) and of its last"""
    fl = d.frags["len"].astype(np.int64)
    f0, f1 = d.recs["first_frag"].astype(np.int64), d.recs["emit_frag"].astype(np.int64)
    multi = f0 != f1
    second = np.where(multi, fl[np.minimum(f0 + 1, len(fl) - 1)], -1)
    return fl[f0], second, fl[f1], multi


def record_expectation(ns, etag):
    """the statuses each family must show at this size. A row can only be valid when its header size fits the header
    byte (byte(headerSize), record.go:109): 1 + ns + 1 + three varint bytes, + etag + an expire varint where flagged.
    R2 and R8 carry an etag and an expire (ns + etag + 6, one more padded); R6's valid row has no expire byte; R7's
    two ten-byte varints need ns + 23; R4 and R6 panic in the etag slice only when there is an etag to slice."""
    fits = lambda h: {OK} if h <= 255 else {INVALID}  # noqa: E731
    return {"R1": fits(ns + 5), "R2": fits(ns + etag + 7), "R3": {INVALID},
            "R4": {INVALID, PANIC} if etag else {INVALID}, "R5": {INVALID},
            "R6": fits(ns + etag + 5) | ({PANIC} if etag else set()),
            "R7": {INVALID, PANIC} if ns + 23 <= 255 else {INVALID}, "R8": fits(ns + etag + 6), "R9": fits(ns + 5)}


HINT_EXPECTATION = {"H1": {OK}, "H2": {OK}, "H3": {INVALID}, "H4": {INVALID, PANIC}, "H5": {OK, PANIC},
                    "H6": {INVALID}}


@pytest.mark.parametrize("ns,etag", PL.REC_SIZES)
def test_record_source(ns, etag):
    src = PL.record_source(ns, etag)
    assert len(src.data) < PL.MAX_SOURCE
    d = oracle_equals_pyref(src)
    seen = by_family(src, d)
    for fam, want in record_expectation(ns, etag).items():
        assert want <= seen[fam], (fam, want, seen[fam])
    st = d.recs["status"]
    ok = st == OK
    hdr = d.recs["hdr_size"].astype(np.int64)
    first, second, _, multi = frag_lens(d)
    framings = {r[2][:2] for r in src.rows}
    assert {"F1", "F2", "F4"} <= framings
    if ns >= 251:
        assert not ok.any()  # byte(headerSize) cannot hold 1 + ns + 1 + 3
        return
    if ns <= 230:
        win2 = ok & (first < np.minimum(hdr, 64))
        walk = ok & multi & (first + np.minimum(32, second) < hdr)
        assert int(win2.sum()) >= MIN_ROWS and int(walk.sum()) >= MIN_ROWS, (int(win2.sum()), int(walk.sum()))
    if ns >= 63:
        assert (hdr[ok] > 64).all()
    if ns in (62, 63):  # the flag byte (offset 1 + ns) is the head's last byte, then the first one outside it
        assert ok.sum() >= 50 and 1 + ns == (63 if ns == 62 else 64)


@pytest.mark.parametrize("ns", PL.HINT_NS)
def test_hint_source(ns):
    src = PL.hint_source(ns)
    assert len(src.data) < PL.MAX_SOURCE
    d = oracle_equals_pyref(src)
    seen = by_family(src, d)
    for fam, want in HINT_EXPECTATION.items():
        assert want <= seen[fam], (fam, want, seen[fam])
    assert {"F1", "F2", "F3", "F4"} <= {r[2][:2] for r in src.rows}
    ok = d.recs["status"] == OK
    first, _, last, multi = frag_lens(d)
    # hdr_size is the key's offset as a byte: ns + the 1..10 bytes of the keyLen varint
    key_off = ns + ((d.recs["hdr_size"].astype(np.int64) - ns) & 0xff)
    trailing = d.recs["size"].astype(np.int64) - key_off - d.recs["key_len"].astype(np.int64)
    assert (trailing[ok] >= 0).all() and (trailing[ok] <= 30).all()  # 0: the key runs to the end (H5), all (0, 0)
    tail = ok & multi & (last < trailing)
    assert int(tail.sum()) >= MIN_ROWS, int(tail.sum())
    if ns >= 64:
        assert int((ok & (first > 64)).sum()) >= MIN_ROWS


@pytest.mark.parametrize("ns,etag", [(0, 0), (17, 4), (63, 20), (100, 4), (230, 0)])
def test_valid_builders_match_the_encoders(ns, etag):
    """R1 and H1 assemble their bytes by hand; where Record.Encode and HintRecord.Encode can express the same row
    (an etag flagged present has bytes) both restatements of the encoders give the same payload"""
    nsb = PL.ns_of(ns)
    i = 0
    for e in (0, 1):
        for x in (0, 1):
            for t in (0, 1):
                for klen in PL.KLENS:
                    got, _ = PL._valid(nsb, etag, i, e, x, t, klen)
                    if not (e and etag == 0):
                        args = (nsb, PL.blob(i, klen), PL.blob(i + 100, PL.VLENS[i % 4]),
                                PL.etag_of(etag, i) if e else b"", PL.BASE + PL.DELTAS[i % 4] if x else 0, bool(t),
                                PL.METAS[i % 3], PL.BASE)
                        assert got == O.record_encode(*args) == P.record_encode(*args), i
                    i += 1
    for p in PL.hint_payloads(ns):
        if p.tag[0] == "H1":
            st, f = P.hint_decode(p.data, ns)
            assert st == 0
            key = p.data[p.hdr:p.hdr + f["key_len"]]
            assert p.data == O.hint_encode(nsb, key, f["fid"], f["off"], f["size"]) == P.hint_encode(
                nsb, key, f["fid"], f["off"], f["size"]), p.tag


def test_sizes_and_cycles():
    """every ns_size with two etag sizes, every etag size with small, mid and large namespaces; over all sources the F4
    placements put the first fragment at every one of the last 1..70 bytes of a block"""
    assert len(PL.REC_SIZES) == 2 * len(PL.REC_NS) and all(len(PL.etags_of(n)) == 2 for n in PL.REC_NS)
    for e in PL.ETAGS:
        sizes = [n for n, x in PL.REC_SIZES if x == e]
        assert min(sizes) <= 16 and max(sizes) >= 250 and any(41 <= n <= 100 for n in sizes)
    ks = collections.Counter()
    for src in [PL.record_source(*s) for s in PL.REC_SIZES] + [PL.hint_source(n) for n in PL.HINT_NS]:
        ks.update(int(r[2][3:]) for r in src.rows if r[2].startswith("F4k"))
    assert set(ks) == set(range(1, 71)), sorted(set(range(1, 71)) - set(ks))


@pytest.mark.parametrize("mode,ns,etag", PL.SEAM_SIZES)
def test_seam_sources(mode, ns, etag):
    """the index-seam sources: valid rows only (the F4 fillers included), distinct keys, the merged length ns + key on
    16k - 1, 16k and 16k + 1, and both the namespace and the key straddling two fragments"""
    for gen in (0, 1):
        src = PL.seam_source(ns, etag, mode, gen)  # asserts every row valid
        d = PL.decode(src)
        merged = d.recs["key_len"].astype(np.int64) + ns
        seam = [int(m) for m, r in zip(merged, src.rows) if r[0] != "filler"]
        lo = -(-ns // 16) * 16 + 16
        assert {lo - 1, lo, lo + 1} <= set(seam)
        first, _, _, multi = frag_lens(d)
        key_off = d.recs["hdr_size"].astype(np.int64) if mode == 0 else ns + 1
        ns_off = 1 if mode == 0 else 0
        klen = d.recs["key_len"].astype(np.int64)
        if ns >= 2:
            assert int((multi & (first > ns_off) & (first < ns_off + ns)).sum()) >= 2  # the namespace straddles
        assert int((multi & (first > key_off) & (first < key_off + klen)).sum()) >= 2   # the key straddles
        assert any(r[2].startswith("F4k") for r in src.rows)
