"""GPU parity of the payload parsers (csrc/bcw_parse.h: uvarint, parse_record) under each of their three byte readers,
at every NsSize / EtagSize of tests/_payloads.py and on every reject branch with valid framing:

  RegReader (bcw_decode.hip)        the decode's record table, record and hint mode, also with every offset shifted
  rd::FragReader (bcw_read_body.h)  the point reads, and through the index the Get and the scrub
  make_key / key_chunk (bcw_index.hip)  ns || key stitched in 16 B chunks: recover, overwrite, filter, Get, scrub
  k_recdesc_w (bcw_encode.hip)      the two choices of the source range no other test selects

The reference of every assertion is the oracle (tests/_oracle.py); test_payloads_host.py pins it against the
independent restatement on these very sources and asserts what the sources reach."""
from __future__ import annotations

import random

import numpy as np
import pytest

import _encode_parity as EP
import _oracle as O
import _payloads as PL
import cases
from bitcaskdb_amd import Index, WalSet, verify_index
from bitcaskdb_amd import _lib as L
from bitcaskdb_amd import index as IX
from bitcaskdb_amd import wal as W
from test_gpu_decode import assert_parity
from test_gpu_read import REC_FIELDS
from test_gpu_read import check as check_reads

pytestmark = pytest.mark.gpu
BASE = cases.BASE
U64MAX = np.iinfo(np.uint64).max


def tagged(src, fn):
    """run fn; a mismatch names the rows of the source by (family, variant, framing)"""
    try:
        return fn()
    except AssertionError as e:
        p = src.params
        raise AssertionError(f"ns_size {p['ns_size']} etag_size {p['etag_size']} mode {p['mode']}: {e}\nrows: "
                             + " ".join(f"{i}:{'/'.join(r)}" for i, r in enumerate(src.rows))[:6000]) from e


# ---- the decode: RegReader ----
@pytest.mark.parametrize("ns,etag", PL.REC_SIZES)
def test_decode_records(ctx_path, ns, etag):
    src = PL.record_source(ns, etag)
    tagged(src, lambda: assert_parity(ctx_path, src.data, src.params, f"records {ns}/{etag}"))


@pytest.mark.parametrize("ns", PL.HINT_NS)
def test_decode_hints(ctx_path, ns):
    src = PL.hint_source(ns)
    tagged(src, lambda: assert_parity(ctx_path, src.data, src.params, f"hints {ns}"))


@pytest.mark.parametrize("delta", [3, 13])
@pytest.mark.parametrize("mode,ns", [(0, 17), (0, 63), (0, 100), (1, 64), (1, 246)])
def test_decode_shifted(ctx_path, mode, ns, delta):
    """every fragment `delta` bytes later: each unaligned 16 B load of the head and tail windows moves"""
    srcs = [PL.record_source(ns, e) for e in PL.etags_of(ns)] if mode == 0 else [PL.hint_source(ns)]
    for src in srcs:
        data, p = cases.shifted(src.data, src.params, delta)
        tagged(src, lambda: assert_parity(ctx_path, data, p, f"shifted {mode}/{ns}+{delta}"))


# ---- the point reads: rd::FragReader ----
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("ns,etag", [(n, e) for n in (0, 17, 63, 64, 100, 250) for e in PL.etags_of(n)])
def test_point_reads(ctx, ns, etag, verify):
    """R1-R9 in the writer's framing (a filler first, so that records cross the block end), read back by (offset,
    size): status, payload and every row column per request, the rejected rows' partial fields included"""
    ps = PL.record_payloads(ns, etag)
    w = O.Writer(BASE, BASE)
    w.write(PL.raw_filler(32768 - 7 - 150 - ns, 0)[0])
    offs = [w.write(p.data) for p in ps]
    data = w.data()
    st = O.decode(data, 40, BASE, ns, etag).recs["status"]
    assert {0, 1} <= set(st.tolist()) and (etag == 0 or 2 in st)
    try:
        got = check_reads(ctx, data, offs, [len(p.data) for p in ps], verify, ns, etag)
    except AssertionError as e:
        raise AssertionError(f"ns_size {ns} etag_size {etag} verify {verify}: {e}\nrequests: "
                             + " ".join(f"{i}:{'/'.join(p.tag)}" for i, p in enumerate(ps))[:6000]) from e
    assert int((got == L.RD_OK).sum()) >= len(ps) - 2  # all but the empty payload read


# ---- the index's key reader: make_key / key_chunk, and the consumers that follow it ----
def merged_keys(src, d):
    ns, mode = src.params["ns_size"], src.params["mode"]
    out = []
    for r, p in zip(d.recs, d.payloads):
        h = int(r["hdr_size"]) if mode == 0 else ns + ((int(r["hdr_size"]) - ns) & 0xff)  # the key's offset as a byte
        a = 1 if mode == 0 else 0
        out.append(p[a:a + ns] + p[h:h + int(r["key_len"])])
    return out


def expect_get(oc, imgs, ns, etag, mk, verify):
    """DBImpl.Get of one merged key by the oracle: (get_status, rd_status, fid, off, size, payload, row)"""
    st, (f, o, z) = oc.get(mk[:ns], mk[ns:])
    if st == 1:
        return (L.GET_NOT_FOUND, 0, 0, 0, 0, None, None)
    if st == 2:
        return (L.GET_SOFT_DELETED, 0, f, o, z, None, None)
    if f not in imgs:
        return (L.GET_NO_WAL, 0, f, o, z, None, None)
    rst, pay = O.read_record(imgs[f], o, z, verify)
    if rst != 0:
        return (L.GET_READ, rst, f, o, z, None, None)
    row = O.record_parse(pay, BASE, ns, etag)
    return (L.GET_OK if row["status"] == 0 else L.GET_RECORD, 0, f, o, z, pay, row)


@pytest.mark.parametrize("mode,ns,etag", PL.SEAM_SIZES)
def test_index_key_seam(ctx, mode, ns, etag):
    """valid rows whose key lengths walk 0..40 (ns + key on every residue mod 16 around each chunk edge), the
    namespace and the key each cut across two fragments: recovery, a second file that overwrites every third key,
    then in record mode the compaction filter, the Get and the scrub, each against the oracle"""
    a = PL.seam_source(ns, etag, mode, 0)
    b = PL.seam_source(ns, etag, mode, 1, klens=range(0, 41, 3), force_f4=(2,))
    ix, oc = Index(ctx, keys=1 << 9), O.Index()
    imgs, known = {3: a.data, 7: b.data}, set()
    try:
        for fid, src in ((3, a), (7, b)):
            dres, ires = ix.recover_segment(src.data, mode, fid, 40, BASE, ns, etag)
            ec, n = oc.put_segment(src.data, 40, BASE, ns, etag, mode, fid)
            assert ec == 0 and n == len(src.rows)
            assert (dres.err_class, ires.err_class, int(ires.n_in), int(ires.n_done)) == (0, 0, n, n)
            known |= set(merged_keys(src, PL.decode(src)))
            exp = ix.export()
            assert set(exp) == known and len(exp) == oc.live() == ix.stats().live, (fid, len(exp), oc.live())
            for mk, v in exp.items():
                st, ov = oc.get(mk[:ns], mk[ns:])
                assert st == 0 and ov == v, (fid, mk, v, ov)
        assert {v[0] for v in exp.values()} == {3, 7}
        if mode == 1:
            return
        # the compaction filter over the first file: the rows the index still points at
        keep_ref, nv = oc.compact_filter(a.data, 40, BASE, ns, etag, 3, len(a.rows))
        assert nv == len(a.rows) and 0 < int(keep_ref.sum()) < len(a.rows)
        dst, hint = W.WalFile(9, BASE), W.WalFile(9, BASE)
        offs, kept = IX.compact_one_wal_filtered(dst, hint, W.load_wal(a.data, 3), ix, ns, etag)
        np.testing.assert_array_equal(offs[:nv] != U64MAX, keep_ref.astype(bool))
        assert kept == int(keep_ref.sum())
        rd, rh = O.Writer(BASE, BASE), O.Writer(BASE, BASE)
        ec, _, nin, roffs = O.compact_append(rd, rh, 9, a.data, 40, BASE, BASE, ns, etag, keep_ref)
        assert ec == 0 and bytes(dst.data) == rd.data() and bytes(hint.data) == rh.data()
        np.testing.assert_array_equal(offs[:nin], roffs[:nin])
        # wrong entries for the scrub: a key that differs in its last byte, one that differs in the namespace's last
        # byte, one that is a byte longer -- each pointing at another key's readable record
        readable = [k for k in sorted(known) if expect_get(oc, imgs, ns, etag, k, True)[0] == L.GET_OK]
        assert len(readable) >= 20 and len(known) - len(readable) >= 10  # the cut framings do not read back
        some = [k for k in readable if len(k) > ns + 1][::5]
        wrong = [k[:-1] + bytes([k[-1] ^ 1]) for k in some] + [k + b"\x00" for k in some[:3]]
        if ns:
            wrong += [k[:ns - 1] + bytes([k[ns - 1] ^ 0x80]) + k[ns:] for k in some]
        src_of = dict(zip(wrong, some + some[:3] + some))
        wrong = sorted(set(wrong) - known)
        vals = [oc.get(src_of[k][:ns], src_of[k][ns:])[1] for k in wrong]
        ix.apply([L.IDX_PUT] * len(wrong), wrong, [v[0] for v in vals], [v[1] for v in vals], [v[2] for v in vals])
        for k, v in zip(wrong, vals):
            oc.put(k[:ns], k[ns:], *v)
        ws = WalSet(ctx)
        for fid, img in imgs.items():
            ws.add(W.Wal(np.frombuffer(img, dtype=np.uint8), fid, 40, BASE))
        try:
            absent = [PL.ns_of(ns) + b"absent-%d" % i for i in range(5)]
            query = sorted(known) + wrong + absent
            random.Random(ns).shuffle(query)
            for verify in (False, True):
                exp = [expect_get(oc, imgs, ns, etag, mk, verify) for mk in query]
                assert {L.GET_OK, L.GET_READ, L.GET_NOT_FOUND} == {e[0] for e in exp}
                g = ix.get_batch(ws, query, verify, ns, etag)
                assert g.rc == 0 and int(g.result.n_ok) == sum(e[0] == L.GET_OK for e in exp)
                for i, (gs, rst, f, o, z, pay, row) in enumerate(exp):
                    assert (int(g.get_status[i]), int(g.rd_status[i])) == (gs, rst), (i, query[i])
                    assert (int(g.fid[i]), int(g.off[i]), int(g.size[i])) == (f, o, z), (i, query[i])
                    if pay is not None:
                        assert g.record_bytes(i) == pay, (i, query[i])
                        for fld in REC_FIELDS:
                            assert int(g.table[fld][i]) == int(row[fld]), (i, query[i], fld)
                        assert int(g.table["foff"][i]) == o + 7 and int(g.table["size"][i]) == z
                # the scrub: what the Get of every entry runs into, and whether the record carries the entry's key
                rep = verify_index(ix, ws, ns, etag, verify)
                bad_ref, by_class, by_rd = [], [0] * 5, [0] * 8
                for mk, (gs, rst, f, o, z, pay, row) in zip(query, exp):
                    if gs == L.GET_NOT_FOUND:
                        continue
                    assert gs in (L.GET_OK, L.GET_READ)
                    if gs == L.GET_READ:
                        cls = L.VFY_READ
                        by_rd[rst] += 1
                    else:
                        h, kl = int(row["hdr_size"]), int(row["key_len"])
                        cls = L.VFY_OK if pay[1:1 + ns] + pay[h:h + kl] == mk else L.VFY_KEY
                    by_class[cls] += 1
                    if cls != L.VFY_OK:
                        bad_ref.append((mk, f, o, z, cls, rst, 0))
                assert sorted(b[0] for b in bad_ref if b[4] == L.VFY_KEY) == wrong
                assert rep.n_checked == len(known) + len(wrong) and rep.n_soft_deleted == 0
                assert list(rep.by_class) == by_class and list(rep.by_rd) == by_rd and rep.n_bad == len(bad_ref)
                assert sorted(tuple(b) for b in rep.bad) == sorted(bad_ref)
        finally:
            ws.close()
    finally:
        ix.close()


# ---- the encode's source range: k_recdesc_w's longest source piece ----
def _encode_both(ctx, src, ns, etag):
    rng = random.Random(ns * 100 + etag)
    keep = np.array([rng.random() < 0.7 for _ in src.rows], dtype=np.uint8)
    res = EP.run_compact(ctx, src.data, keep, ns=ns, etag=etag, dst_base=BASE + 3)
    assert res.err_class == 0 and res.n_written == int(keep.sum())
    res = EP.run_hint(ctx, src.data, ns=ns, etag=etag)
    assert res.err_class == 0 and res.n_in == len(src.rows)


def test_encode_etag_is_the_source_range(ctx):
    """ns_size 8, etag_size 32 with short keys and values: the etag is the longest source piece of a record"""
    ns, etag = 8, 32
    src = PL.seam_source(ns, etag, 0, klens=range(0, 12), force_f4=(4,))
    r = PL.decode(src).recs
    body = r["key_len"] + r["val_len"] + r["meta_len"]
    assert int((((r["flags"] & 1) == 0) & (body < etag)).sum()) >= 8
    _encode_both(ctx, src, ns, etag)


@pytest.mark.parametrize("ns", [66, 67, 68])
def test_encode_literal_prefix_at_the_limit(ctx, ns):
    """ns_size 66, 67, 68 with etag_size 20: header byte, namespace, flags, etag and the varints are 91, 92 and 93
    literal bytes and more, on both sides of the 92 the fast writers hold (k_write / k_wcopy against k_write_general)"""
    etag = 20
    src = PL.seam_source(ns, etag, 0)
    r = PL.decode(src).recs
    with_etag = (r["flags"] & 3) == 2  # an etag and no expire: the shortest header with an etag
    assert int(with_etag.sum()) >= 8 and set(r["hdr_size"][with_etag].tolist()) == {ns + 25}
    _encode_both(ctx, src, ns, etag)
