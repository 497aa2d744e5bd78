"""GPU parity of everything that consumes the decode's record and fragment tables -- the compaction re-encode
(ENC_COMPACT), the hint rebuild (ENC_HINT), the index Put loops (recover_segment) and the compaction filter fused
with the encode -- on sources the writer never produces and at source offsets the other suites never pass:

  * hand-framed WALs (cases.Framer): First + Last in one block, zero-length fragments, Full after First, a lone
    Last, runs of one-byte fragments, short Middles around block ends, random cuts inside the header, the
    namespace, the key, the varints and the meta;
  * writer-framed WALs in which a record's first fragment holds exactly L0 bytes, for every L0 that puts the
    fragment boundary inside the header, the key or the value (record mode) and inside the namespace, the key-length
    varint or the key (hint mode, NsSize 20 and 300);
  * sources whose first block starts at start_off = 40 + delta.

Every assertion is bit-exact against the CPU oracle (pinned against the independent restatement on these very
sources in test_oracle.py::test_irregular_oracle_vs_pyref)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import _oracle as O
import cases
from _encode_parity import prefill, run_compact, run_hint
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import index as IX
from bitcaskdb_amd import wal as W
from test_gpu_decode import assert_parity

pytestmark = pytest.mark.gpu
BASE = cases.BASE
NS, ETAG = 20, 20
SRC_FID = 3
META = b"\x81\xa3foo\xa3bar"
RECORD_CASES = ("irregular_shapes", "irregular_random")


class Source:
    """one source image with the oracle's decode of it, built once per module"""

    def __init__(self, data, p):
        self.data, self.p = data, p
        self.so, self.mode, self.ns = p["start_off"], p["mode"], p["ns_size"]
        self.ref = O.decode(data, self.so, BASE, self.ns, ETAG, self.mode)
        st = self.ref.recs["status"]
        bad = np.nonzero(st != 0)[0]
        self.n_ok = int(bad[0]) if len(bad) else len(st)  # rows the iteration delivers


_SOURCES = {}


def source(name, delta=0) -> Source:
    if (name, delta) not in _SOURCES:
        if name == "zipf60":
            data, p = cases.case_zipf(60)
        elif name == "sweep_records":
            data, p = sweep_records()
        else:
            data, p = cases.ALL[name]()
        if delta:
            data, p = cases.shifted(data, p, delta)
        _SOURCES[(name, delta)] = Source(data, p)
    return _SOURCES[(name, delta)]


def oracle_compact(src, keep, dst_base, pre_wal, seed, start_off):
    """what run_compact compares against, for another source: (err_class, n_in, appended WAL, hint, offsets)"""
    rng = random.Random(seed)
    dst, hint = O.Writer(dst_base, dst_base), O.Writer(dst_base, dst_base)
    prefill(rng, dst, pre_wal)
    prefill(rng, hint, 0)
    wp, hp = dst.size(), hint.size()
    ec, _, nin, offs = O.compact_append(dst, hint, 9, src, start_off, BASE, dst_base, NS, ETAG, keep)
    return ec, nin, dst.data()[wp:], hint.data()[hp:], offs[:nin]


def reencoded(pay: bytes, r, dst_base: int) -> bytes:
    """Record.Encode of the parsed row against dst_base (compaction.go:313-316): an AppMetaSize-0 meta is dropped"""
    h, kl, vl, ml, fl, eo = (int(r[c]) for c in ("hdr_size", "key_len", "val_len", "meta_len", "flags", "etag_off"))
    meta = pay[h + kl + vl:h + kl + vl + ml]
    return O.record_encode(pay[1:1 + NS], pay[h:h + kl], pay[h + kl:h + kl + vl], b"" if fl & 1 else pay[eo:eo + ETAG],
                           int(r["expire"]), bool(fl & 4), b"" if O.meta_app_size_zero(meta) else meta, dst_base)


def compact_checks(ctx, s: Source, combos, twin=None):
    """ENC_COMPACT against oc_compact_append for every (keep, dst_base, pre_wal); twin: a source with the same payload
    sequence at start_off 40 (the writer's framing of it, or the unshifted image) -- the output must equal the
    oracle's for the twin too, because it depends on the payload sequence only; then the GPU decode of the output
    returns the kept rows' re-encoded payloads at the returned offsets"""
    n = len(s.ref.recs)
    for k, (keep, dst_base, pre_wal) in enumerate(combos):
        keep = np.ascontiguousarray(keep[:n], dtype=np.uint8)
        res, wal, hb, offs = run_compact(ctx, s.data, keep, dst_base=dst_base, pre_wal=pre_wal, seed=k,
                                         start_off=s.so, full=True)
        assert res.n_in == s.n_ok
        assert res.err_class == (L.ENC_ERR_SRC if s.n_ok < n else 0)
        if twin is not None:
            ec, nin, twal, thint, toffs = oracle_compact(twin, keep, dst_base, pre_wal, k, 40)
            assert (ec, nin) == (res.err_class, res.n_in)
            assert wal == twal and hb == thint, "the output depends on the framing / offset of the source"
            np.testing.assert_array_equal(offs[:nin], toffs)
        if pre_wal == 0:  # the round trip needs the file from its super block on
            image = O.Writer(dst_base, dst_base).data()[:40] + wal
            dec = ctx.decode(np.frombuffer(image, dtype=np.uint8), 40, dst_base, NS, ETAG, with_frags=True)
            rows = [i for i in range(s.n_ok) if keep[i]]
            assert dec.result.err_class == 0 and dec.n_records == len(rows)
            # WriteRecord returns the First's header; behind a zero-length First (7 bytes were left in the block) the
            # iterator re-captures the offset at the next fragment
            hdr = dec.table["foff"] - 7
            f0 = dec.table["first_frag"]
            prev = np.maximum(f0, 1) - 1
            zf = (f0 > 0) & (dec.frags["len"][prev] == 0) & (dec.frags["type"][prev] == cases.FIRST)
            hdr[zf] = dec.frags["data_off"][prev[zf]] - 7
            np.testing.assert_array_equal(hdr, offs[rows])
            for j, i in enumerate(rows):
                assert dec.record_bytes(j) == reencoded(s.ref.payloads[i], s.ref.recs[i], dst_base), (j, i)


def masks(n, seed):
    rng = random.Random(seed)
    return np.ones(n, dtype=np.uint8), np.array([rng.random() < 0.7 for _ in range(n)], dtype=np.uint8)


def put_checks(ctx, s: Source, fid=SRC_FID):
    """recover_segment's Put loop against oc_index_put_segment: the exported index and the row counts"""
    for use_fid in (False, True):
        ix, oc = IX.Index(ctx), O.Index()
        _, n_put = oc.put_segment(s.data, s.so, BASE, s.ns, 0 if s.mode else ETAG, s.mode, fid, use_fid)
        assert n_put == s.n_ok
        dres, ires = ix.recover_segment(s.data, s.mode, fid, s.so, BASE, s.ns, 0 if s.mode else ETAG,
                                        use_record_fid=use_fid)
        assert ires.err_class == 0 and (ires.n_in, ires.n_done) == (n_put, n_put)
        assert (dres.err_class, dres.n_records) == (s.ref.err_class, len(s.ref.recs))
        exp = ix.export()
        assert len(exp) == oc.live() == ix.stats().live
        for mk, v in exp.items():
            assert oc.get(mk[:s.ns], mk[s.ns:]) == (0, v), mk[s.ns:s.ns + 12]
        ix.close()


def row_keys(s: Source):
    """(ns, key) of every delivered row"""
    out = []
    for r, pay in zip(s.ref.recs[:s.n_ok], s.ref.payloads):
        h, kl = int(r["hdr_size"]), int(r["key_len"])
        out.append((pay[1:1 + NS], pay[h:h + kl]))
    return out


def filter_checks(ctx, s: Source, seed=0, pins=(), expect=None, dst_base=BASE):
    """the device doFilter fused with the encode: the index is filled from the source, ~20 % of its keys are deleted
    or soft-deleted and ~10 % re-pointed (another fid, or another offset of this fid), `pins` [(row, off)] re-point
    rows at chosen offsets last. kept, the dst and hint bytes and the offsets equal oc_compact_append's with
    oc_compact_filter's mask. A source whose iteration ends in an error raises it after the appends.
    expect: {row: keep} asserted on the oracle's mask."""
    ix, oc = IX.Index(ctx), O.Index()
    ix.recover_segment(s.data, L.MODE_RECORD, SRC_FID, s.so, BASE, NS, ETAG)
    oc.put_segment(s.data, s.so, BASE, NS, ETAG, 0, SRC_FID)
    keys = row_keys(s)
    uniq = sorted(set(keys))
    rng = random.Random(seed)
    ops = []
    for ns, k in uniq:
        r = rng.random()
        if r < 0.2:
            ops.append((rng.choice([L.IDX_DELETE, L.IDX_SOFT_DELETE]), ns, k, 0, 0, 0))
        elif r < 0.3:
            st, (f, o, z) = oc.get(ns, k)
            ops.append((L.IDX_PUT, ns, k, SRC_FID + 1, o, z) if rng.random() < 0.5 else
                       (L.IDX_PUT, ns, k, SRC_FID, o + rng.choice([-7, 7, 1]), z))
    for row, off in pins:
        ops.append((L.IDX_PUT, *keys[row], SRC_FID, off, int(s.ref.recs["size"][row])))
    ix.apply([o[0] for o in ops], [o[1] + o[2] for o in ops], [o[3] for o in ops], [o[4] for o in ops],
             [o[5] for o in ops])
    for op, ns, k, f, o, z in ops:
        oc.set(ns, k, op, f, o, z)
    n = len(s.ref.recs)
    keep_ref, nv = oc.compact_filter(s.data, s.so, BASE, NS, ETAG, SRC_FID, n)
    assert nv == s.n_ok and 0 < int(keep_ref.sum()) < s.n_ok
    for row, want in (expect or {}).items():
        assert int(keep_ref[row]) == want, (row, want)
    rd, rh = O.Writer(dst_base, dst_base), O.Writer(dst_base, dst_base)
    ec, _, nin, roffs = O.compact_append(rd, rh, 9, s.data, s.so, BASE, dst_base, NS, ETAG, keep_ref)
    dst, hint = W.WalFile(9, dst_base), W.WalFile(9, dst_base)
    src = W.Wal(np.frombuffer(s.data, dtype=np.uint8), SRC_FID, s.so, BASE)
    if ec == 0:
        offs, kept = IX.compact_one_wal_filtered(dst, hint, src, ix)
        assert kept == int(keep_ref.sum()) and len(offs) == nin
        np.testing.assert_array_equal(offs, roffs[:nin])
    else:
        assert s.n_ok < n and ec == L.ENC_ERR_SRC
        with pytest.raises(W.ErrInvalidData):
            IX.compact_one_wal_filtered(dst, hint, src, ix)
    assert bytes(dst.data) == rd.data(), "dst WAL bytes differ"
    assert bytes(hint.data) == rh.data(), "hint WAL bytes differ"
    ix.close()


def valid_prefix(s: Source) -> Source:
    """the image cut before the row that ends the iteration"""
    if s.n_ok == len(s.ref.recs):
        return s
    f = int(s.ref.recs["first_frag"][s.n_ok])
    return Source(s.data[:int(s.ref.frags["data_off"][f]) - 7], s.p)


# ---- 2. irregular framing ----
def test_irregular_decode_is_what_the_consumers_see(ctx):
    """the tables the consumers below read: decode parity on the session context they run on"""
    for name in RECORD_CASES + ("irregular_hint",):
        s = source(name)
        assert_parity(ctx, s.data, s.p, name)


@pytest.mark.parametrize("name", RECORD_CASES)
def test_irregular_hint_by_wal(ctx, name):
    s = source(name)
    res = run_hint(ctx, s.data)
    assert res.n_in == s.n_ok
    if name == "irregular_shapes":  # what the rows must carry, read from the oracle's (equal) output
        h = O.decode(O.hint_by_wal(s.data, 5, 40, BASE, NS, ETAG)[3], 40, BASE, NS, 0, 1).recs
        fr, rc = s.ref.frags, s.ref.recs
        first_hdr = int(fr["data_off"][rc["first_frag"][2] - 1]) - 7  # the dangling First before the Full of row 2
        assert fr["type"][rc["first_frag"][2] - 1] == cases.FIRST and fr["type"][rc["emit_frag"][2]] == cases.FULL
        assert (int(h["val_len"][2]), int(h["meta_len"][2])) == (first_hdr, int(fr["len"][rc["emit_frag"][2]]))
        f = int(rc["first_frag"][1])  # row 1: zero-length First and Middle, then the first fragment with data
        assert fr["len"][f] > 0 and (fr["len"][f - 2:f] == 0).all()
        assert int(h["val_len"][1]) == int(fr["data_off"][f]) - 7


@pytest.mark.parametrize("name", RECORD_CASES)
def test_irregular_compact(ctx, name):
    s = source(name)
    ones, some = masks(len(s.ref.recs), 17)
    twin = cases.wal_of(s.ref.payloads)[0]
    combos = [(m, b, pre) for m in (ones, some) for b in (BASE, BASE - 5) for pre in (0, 32768 - 50)]
    compact_checks(ctx, s, combos, twin)


@pytest.mark.parametrize("name", RECORD_CASES + ("irregular_hint",))
def test_irregular_index_put(ctx, name):
    put_checks(ctx, source(name))


@pytest.mark.parametrize("name", RECORD_CASES)
def test_irregular_filter_fused(ctx, name):
    s = source(name)
    filter_checks(ctx, s, seed=1)  # irregular_shapes: the invalid last row ends the iteration with its error
    if name == "irregular_shapes":
        v = valid_prefix(s)
        fr, rc = v.ref.frags, v.ref.recs
        f = int(rc["first_frag"][1])
        assert int(rc["foff"][1]) == int(fr["data_off"][f]) and fr["len"][f - 2] == 0  # foff re-captured
        zero_first_hdr = int(fr["data_off"][f - 2]) - 7
        filter_checks(ctx, v, seed=2, pins=[(1, int(rc["foff"][1]) - 7)], expect={1: 1})
        filter_checks(ctx, v, seed=2, pins=[(1, zero_first_hdr)], expect={1: 0})


# ---- 3. first-fragment-length sweeps on writer-framed sources ----
def _sweep(targets, make_filler, min_filler):
    """a writer-framed WAL in which target j = (payload, L0) has exactly L0 bytes in its first fragment: a filler of
    exact size before each target leaves 7 + L0 bytes in the block. Returns (image, rows of the targets)."""
    w = O.Writer(BASE, BASE)
    rows, n = [], 0
    for j, (p, l0) in enumerate(targets):
        while True:
            left = 32768 - (w.size() - 40) % 32768
            left = 32768 if left < 7 else left  # the writer pads such a block end
            room = left - (7 + l0) - 7          # filler payload bytes that leave 7 + L0
            if room >= min_filler:
                break
            w.write(make_filler(1000 + n, max(min_filler, left - 7)))  # burn the block
            n += 1
        w.write(make_filler(1000 + n, room))
        w.write(p)
        rows.append(n + 1 + j)
        n += 1
    return w.data(), rows


def sweep_records():
    etag = cases.sha1("etag")
    targets = [(cases.rec(i, 60, etag=etag, expire=BASE + 300, meta=META, klen=40), i) for i in range(110)]
    assert all(p[0] == 47 for p, _ in targets)  # hdr_size: L0 up to 109 reaches through the key into the value
    data, rows = _sweep(targets, cases.filler, 40)
    d = O.decode(data, 40, BASE, NS, ETAG, want_bytes=False)
    assert d.err_class == 0 and (d.recs["status"] == 0).all()
    f0, f1 = d.recs["first_frag"][rows], d.recs["emit_frag"][rows]
    span = f0 != f1
    assert set(int(x) for x in d.frags["len"][f0[span]]) == set(range(1, 110)) and int(span.sum()) == 109
    z = rows[0]  # L0 = 0: the zero-length First; the iterator re-captures the offset in the next block
    assert not span[0] and (int(d.recs["foff"][z]) - 7 - 40) % 32768 == 0
    assert d.frags["len"][f0[0] - 1] == 0 and d.frags["type"][f0[0] - 1] == cases.FIRST
    return data, cases.params()


def test_sweep_records_encode(ctx):
    s = source("sweep_records")
    n = len(s.ref.recs)
    drop7 = np.ones(n, dtype=np.uint8)
    drop7[::7] = 0
    compact_checks(ctx, s, [(np.ones(n, dtype=np.uint8), BASE - 5, 0), (drop7, BASE, 32768 - 50)])
    run_hint(ctx, s.data)


def test_sweep_records_index(ctx):
    s = source("sweep_records")
    put_checks(ctx, s)
    filter_checks(ctx, s, seed=3)


def hint_filler(ns: bytes):
    def make(i: int, total: int) -> bytes:
        klen = total - len(ns) - 12
        for _ in range(4):
            key = b"%06d" % i + bytes((i + k) & 0xff for k in range(klen - 6))
            h = O.hint_encode(ns, key, 4, 1000 + i, 77)
            if len(h) == total:
                return h
            klen -= len(h) - total
        raise AssertionError("no hint of that size")
    return make


@pytest.mark.parametrize("ns_size,klen,l0s", [(20, 60, range(0, 80)), (300, 200, (0, 1, 150, 299, 300, 301, 302, 305))],
                         ids=["ns20", "ns300"])
def test_sweep_hint_index(ctx, ns_size, klen, l0s):
    """hint records whose first fragment ends inside the namespace, the key-length varint (two bytes at NsSize 300:
    make_key counts them through the fragment boundary) or the key"""
    ns = bytes((7 * i + 1) & 0xff for i in range(ns_size))
    targets = [(O.hint_encode(ns, b"t%03d" % l0 + bytes((l0 + k) & 0xff for k in range(klen - 4)), 9, 5000 + l0,
                              60 + l0), l0) for l0 in l0s]
    data, rows = _sweep(targets, hint_filler(ns), ns_size + 24)
    s = Source(data, cases.params(ns=ns_size, mode=1))
    assert s.ref.err_class == 0 and s.n_ok == len(s.ref.recs)
    f0 = s.ref.recs["first_frag"][rows]
    want = set(l0s) - {0}
    assert set(int(x) for x in s.ref.frags["len"][f0[f0 != s.ref.recs["emit_frag"][rows]]]) == want
    assert_parity(ctx, data, s.p, f"hint sweep ns={ns_size}")
    put_checks(ctx, s, fid=4)


# ---- 4. start_off = 40 + delta through the consumers ----
@pytest.mark.parametrize("delta", [4, 9, 16])
@pytest.mark.parametrize("name", ["records_mixed", "zipf60", "irregular_random"])
def test_shifted_start_off(ctx, name, delta):
    s0, s = source(name), source(name, delta)
    assert s.so == 40 + delta and s.ref.err_class == 0 and s.n_ok == s0.n_ok == len(s.ref.recs)
    np.testing.assert_array_equal(s.ref.recs["foff"], s0.ref.recs["foff"] + delta)
    assert_parity(ctx, s.data, s.p, f"{name}+{delta}")
    ones, some = masks(len(s.ref.recs), delta)
    compact_checks(ctx, s, [(ones, BASE, 0), (some, BASE - 5, 32768 - 50)], twin=s0.data)
    run_hint(ctx, s.data, start_off=s.so)
    put_checks(ctx, s)
    filter_checks(ctx, s, seed=delta)


@pytest.mark.parametrize("delta", [4, -40])
def test_failing_start_off(ctx, delta):
    """a start_off the fragments do not begin at: the iteration fails at once. The consumers stop where the oracle
    stops and write nothing"""
    data, p = cases.case_start_off(delta)
    so = p["start_off"]
    ref = O.decode(data, so, BASE, NS, ETAG)
    assert ref.err_class != 0 and len(ref.recs) < 100
    n = len(ref.recs)
    res, wal, hb, offs = run_compact(ctx, data, np.ones(100, dtype=np.uint8), start_off=so, pre_wal=500, full=True)
    assert res.err_class == L.ENC_ERR_SRC and res.src_err_class == ref.err_class
    assert res.n_in == n and len(offs) == n
    if n == 0:
        assert wal == b"" and hb == b""
    hres = run_hint(ctx, data, start_off=so)
    assert hres.src_err_class == ref.err_class
    ix, oc = IX.Index(ctx), O.Index()
    _, n_put = oc.put_segment(data, so, BASE, NS, ETAG, 0, SRC_FID)
    dres, ires = ix.recover_segment(data, L.MODE_RECORD, SRC_FID, so, BASE, NS, ETAG)
    assert dres.err_class == ref.err_class and (ires.n_in, ires.n_done) == (n_put, n_put)
    assert ix.export() == {} if n_put == 0 else len(ix.export()) == oc.live()
    ix.close()
