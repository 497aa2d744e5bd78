"""Enumerated record and hint payloads for the payload parsers (csrc/bcw_parse.h: uvarint, parse_record) and the
framings that move them through every window of the three byte readers (TEST INFRASTRUCTURE ONLY).

Nothing here is sampled: every family below is built variant by variant, so each class of payload occurs by
construction, and every payload carries a tag (family, variant) that the assertion messages print. The payloads are
assembled from raw varint bytes, not through the oracle's encoder, so padded and overflowing varints, wrong header bytes
and truncations are expressible. What the parser must answer for them comes from the oracle (tests/_oracle.py), pinned
against the independent restatement (golden/pyref.py) in test_payloads_host.py.

Record mode (RecordFromBytes, record.go:140-239), for one (ns_size, etag_size):
  R1 valid records, R2 padded varints, R3 overflowing varints, R4 truncations, R5 off-by-one header byte and length,
  R6 the etag slice boundary, R7 length sums, R8 expire deltas, R9 unknown flag bits.
Hint mode (HintRecord.Decode, hint.go:50-84), for one ns_size:
  H1 valid hints, H2 padded varints, H3 overflowing varints, H4 truncations, H5 re-written key lengths,
  H6 a continuation bit on the last byte.
Framings (cases.Framer), each payload placed once per framing:
  F1 one Full; F2 a first fragment of L0 bytes and a second of d bytes; F3 (hint) a last fragment of t bytes;
  F4 behind a filler fragment that leaves the record's first fragment the last k bytes of its 32 KiB block. F4 costs the
  rest of a block, so it is placed where the image reaches a block end anyway (and where a caller forces it): once per
  block, which keeps a source under 256 KiB. k cycles over 1..70 from a start that differs per size.
L0, d and t cycle per family, so the valid families walk every position themselves."""
from __future__ import annotations

from collections import namedtuple

import _oracle as O
import cases

BASE = cases.BASE
MAX_SOURCE = 256 << 10

# record mode: every ns_size with two of the etag sizes, cycling
REC_NS = (0, 1, 15, 16, 17, 31, 32, 33, 41, 42, 43, 59, 60, 61, 62, 63, 64, 65, 100, 200, 230, 231, 250, 251, 300)
ETAGS = (0, 4, 20, 32)
REC_SIZES = tuple((ns, ETAGS[(2 * i + j) % 4]) for i, ns in enumerate(REC_NS) for j in (0, 1))
HINT_NS = (0, 1, 15, 16, 17, 20, 31, 32, 33, 59, 62, 63, 64, 65, 100, 245, 246, 300)


# the index-seam sources (mode, ns_size, etag_size): every residue of ns_size mod 16, then the sizes around the chunk
# and head edges and the largest ones
SEAM_SIZES = tuple((0, n, dict(REC_SIZES).get(n, ETAGS[n % 4])) for n in list(range(18)) + [31, 32, 33, 63, 64, 65, 100,
                                                                                          250]) \
    + tuple((1, n, 0) for n in list(range(18)) + [100, 245, 246, 300])


def etags_of(ns_size: int):
    return tuple(e for n, e in REC_SIZES if n == ns_size)


# a payload: tag = (family, variant), the bytes, and the header size it was built with (where the key starts; the
# truncations keep their source's), which bounds the F2 cuts
Payload = namedtuple("Payload", "tag data hdr")
# a source: the file image, the decode parameters, and per expected row (family, variant, framing)
Source = namedtuple("Source", "data params rows payloads")

META11 = b"\x81\xa4foo1\xa4bar2"
METAS = (b"", META11, b"\x81\xa0\xa0")  # absent, 11 B, an AppMetaSize-0 form
KLENS = (0, 1, 127, 128, 300)
VLENS = (0, 1, 33, 300)
HKLENS = (0, 1, 5, 31, 32, 33, 64, 127, 128, 300)
DELTAS = (60, 128, 1 << 20, (1 << 35) - 1)
OVERFLOWS = (("ff9_01", b"\xff" * 9 + b"\x01"),   # 2^64 - 1: accepted, >= 2^63
             ("ff9_02", b"\xff" * 9 + b"\x02"),   # overflow: (0, 0)
             ("cont11", b"\x80" * 11))            # eleven continuation bytes: (0, 0)
U64S = (0, 1, 127, 128, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)


def uv(v: int) -> bytes:
    """binary.PutUvarint"""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def pad_uv(v: int, n: int) -> bytes:
    """v in n bytes, more than PutUvarint writes: every byte continues but the last, which is 0x00 (Uvarint accepts
    it; at n == 10 the last byte is <= 1)"""
    c = uv(v)
    assert n > len(c)
    return bytes(b | 0x80 for b in c) + b"\x80" * (n - len(c) - 1) + b"\x00"


def ns_of(ns_size: int) -> bytes:
    return bytes((11 * i + ns_size + 1) & 0xff for i in range(ns_size))


def blob(seed: int, n: int) -> bytes:
    return bytes((seed * 31 + 7 * k + 3) & 0xff for k in range(n))


def etag_of(etag_size: int, seed: int = 0) -> bytes:
    return bytes((0xe0 + seed + 5 * k) & 0xff for k in range(etag_size))


def record(ns: bytes, flag: int, klb: bytes, vlb: bytes, mlb: bytes, etag: bytes, expb: bytes, body: bytes,
           hdr: int | None = None):
    """header byte | ns | flag | three varints | etag | expire varint | key value meta -> (bytes, header size)"""
    head = ns + bytes([flag]) + klb + vlb + mlb + etag + expb
    h = 1 + len(head)
    return bytes([(h if hdr is None else hdr) & 0xff]) + head + body, h


def _valid(ns, etag_size, i, e, x, t, klen, vlen=None, meta=None):
    """valid record i: etag present e, expire present x, tombstone t"""
    meta = METAS[i % 3] if meta is None else meta
    vlen = VLENS[i % 4] if vlen is None else vlen
    flag = (0 if e else 1) | (0 if x else 2) | (4 if t else 0)
    key, val = blob(i, klen), blob(i + 100, vlen)
    return record(ns, flag, uv(klen), uv(vlen), uv(len(meta)), etag_of(etag_size, i) if e else b"",
                  uv(DELTAS[i % 4]) if x else b"", key + val + meta)


def _base(ns, etag_size, over=None, **kw):
    """the record the mutated families start from: etag and expire present, key 5, value 9, meta 11 B; `over` replaces
    the raw bytes of one varint (k, v, m, x)"""
    f = dict(k=uv(5), v=uv(9), m=uv(11), x=uv(60))
    f.update(over or {})
    return record(ns, 0, f["k"], f["v"], f["m"], etag_of(etag_size), f["x"], blob(1, 5) + blob(2, 9) + META11, **kw)


def record_payloads(ns_size: int, etag_size: int):
    ns, out = ns_of(ns_size), []

    def add(fam, var, built):
        out.append(Payload((fam, var), built[0], built[1]))

    i = 0
    for e in (0, 1):
        for x in (0, 1):
            for t in (0, 1):
                for klen in KLENS:
                    add("R1", f"e{e}x{x}t{t}k{klen}m{i % 3}v{VLENS[i % 4]}", _valid(ns, etag_size, i, e, x, t, klen))
                    i += 1
    vals = dict(k=5, v=9, m=11, x=60)
    for pos in "kvmx":
        for n in (2, 3, 10):
            add("R2", f"{pos}pad{n}", _base(ns, etag_size, {pos: pad_uv(vals[pos], n)}))
    for pos in "kvmx":
        for name, raw in OVERFLOWS:
            add("R3", f"{pos}{name}", _base(ns, etag_size, {pos: raw}))
    full, h = _base(ns, etag_size)
    for n in range(0, h + 3):
        add("R4", f"cut{n}", (full[:n], h))
    add("R5", "hdr-1", _base(ns, etag_size, hdr=h - 1))
    add("R5", "hdr+1", _base(ns, etag_size, hdr=h + 1))
    add("R5", "len+1", (full + b"\x00", h))
    add("R5", "len-1", (full[:-1], h))
    # etag and expire flagged present, no key, value or meta: o = 1 + ns + 1 + 3, the slice data[o + etag_len:] panics
    # one byte short, is empty at len == o + etag_len (an expire of (0, 0): the row is valid) and holds one byte after
    o = ns_size + 5
    for d in (-1, 0, 1):
        hd = o + etag_size + (1 if d == 1 else 0)
        p, _ = record(ns, 0, uv(0), uv(0), uv(0), etag_of(etag_size), b"\x05", b"", hdr=hd)
        add("R6", f"len=o+etag{d:+d}", (p[:o + etag_size + d], hd))
    big = 1 << 63
    for var, kl, vl, ml in (("k2^63", big, 0, 0), ("wrap_total_ok", big, big, 0), ("wrap_total_bad", big, big, 1),
                            ("kmax_wrap_total_ok", (1 << 64) - 1, 1, 0), ("kmax_wrap_total_bad", (1 << 64) - 1, 3, 0)):
        add("R7", var, record(ns, 3, uv(kl), uv(vl), uv(ml), b"", b"", b""))
    for dl in (0, (1 << 35) - 1, 1 << 35, 1 << 63, (1 << 64) - 1):
        add("R8", f"delta{dl:#x}", record(ns, 0, uv(3), uv(4), uv(0), etag_of(etag_size), uv(dl), blob(3, 7)))
    for fl in (0x83, 0xfb, 0x80, 0xf8):
        present = not fl & 1
        add("R9", f"flag{fl:#x}", record(ns, fl, uv(3), uv(4), uv(0), etag_of(etag_size) if present else b"",
                                          uv(60) if present else b"", blob(4, 7)))
    return out


def hint(ns: bytes, klb: bytes, key: bytes, fb: bytes, ob: bytes, sb: bytes):
    """ns | keyLen varint | key | fid, off, size varints -> (bytes, key offset)"""
    return ns + klb + key + fb + ob + sb, len(ns) + len(klb)


def hint_payloads(ns_size: int):
    ns, out = ns_of(ns_size), []

    def add(fam, var, built):
        out.append(Payload((fam, var), built[0], built[1]))

    # 45 hints: every key length at least four times, every value nine times in each of fid, off and size
    for i in range(45):
        klen = HKLENS[i % 10]
        f, o, s = U64S[i % 9], U64S[(i + 3 + i // 9) % 9], U64S[(i + 6 + 2 * (i // 9)) % 9]
        add("H1", f"k{klen}f{f:#x}o{o:#x}s{s:#x}", hint(ns, uv(klen), blob(i, klen), uv(f), uv(o), uv(s)))
    vals = dict(k=5, f=7, o=100, s=50)

    def base(over=None):
        f = {p: uv(v) for p, v in vals.items()}
        f.update(over or {})
        return hint(ns, f["k"], blob(5, 5), f["f"], f["o"], f["s"])

    for pos in "kfos":
        for n in (2, 3, 10):
            add("H2", f"{pos}pad{n}", base({pos: pad_uv(vals[pos], n)}))
    for pos in "kfos":
        for name, raw in OVERFLOWS:
            add("H3", f"{pos}{name}", base({pos: raw}))
    full, h = hint(ns, uv(33), blob(6, 33), uv(1 << 32), uv(1 << 63), uv(300))
    for n in range(len(full)):
        add("H4", f"cut{n}", (full[:n], h))
    add("H4", "len+1", (full + b"\x00", h))
    # keyLen re-written over a 5-byte key and three one-byte varints (8 bytes after the keyLen varint)
    for var, kl in (("end=len", 8), ("end=len+1", 9), ("2^62", 1 << 62), ("2^63", 1 << 63), ("2^64-1", (1 << 64) - 1)):
        add("H5", var, hint(ns, uv(kl), blob(7, 5), uv(7), uv(100), uv(50)))
    # keyLen 2^64 - 1 steps back onto its varint's last byte (fid 1); two more varints end the payload exactly, which
    # leaves the negative keyLen for the make() that panics
    add("H5", "2^64-1,o==len", hint(ns, uv((1 << 64) - 1), b"", b"", b"\x05", b"\x06"))
    p, h = base()
    add("H6", "last|0x80", (p[:-1] + bytes([p[-1] | 0x80]), h))
    return out


D_CYCLE = (0, 1, 7, 31, 32, 33)


def raw_filler(space: int, row: int):
    """one Full fragment of raw bytes that takes `space` bytes of the image, header included"""
    return [bytes((0xa5 + 3 * k) & 0xff for k in range(space - cases.HDR))] if space >= cases.HDR else None


def frame_source(payloads, params, force_f4=(), filler=raw_filler, k0=0, framings=("F1", "F2", "F3", "F4"),
                 extra=None) -> Source:
    """every payload under each framing. force_f4: indices of payloads that get an F4 placement wherever the image
    stands (each costs the rest of a block). filler(space, row_index) -> the data of the Full fragments that take up
    `space` bytes of the image with their headers, or None when it cannot. extra(index, payload) -> further
    placements [(name, cuts)] of that payload."""
    mode = params["mode"]
    f = cases.Framer(params["start_off"])
    rows, placed = [], []
    cyc = {}
    kk = [k0]

    def nxt(fam, what, mod):
        c = cyc.get((fam, what), 0)
        cyc[(fam, what)] = c + 1
        return c % mod

    def put(p, framing, cuts):
        f.record(p.data, cuts)
        rows.append(p.tag + (framing,))
        placed.append(p.data)

    def f4(p):
        """filler, then the record framed as the writer frames it: its first fragment is the block's last k bytes"""
        k = 1 + kk[0] % 70
        fills = filler(f.room() - k, len(rows))
        if fills is None:
            return False
        kk[0] += 1
        for fill in fills:
            f.put(cases.FULL, fill)
            rows.append(("filler", str(len(fill)), "F4"))
            placed.append(fill)
        assert f.room() == k
        put(p, f"F4k{k}", ())
        return True

    def place(p, fr, forced):
        fam, n = p.tag[0], len(p.data)
        # the image would leave this block within this placement: spend the block end on an F4 first
        if "F4" in framings and not forced and f.room() < n + 3 * cases.HDR + 80:
            f4(p)
        if fr == "F1":
            put(p, "F1", ())
        elif fr == "F2":
            l0 = nxt(fam, "l0", min(n, p.hdr + 2) + 1)
            d = D_CYCLE[nxt(fam, "d", len(D_CYCLE))]
            put(p, f"F2L{l0}d{d}", (l0, min(n, l0 + d)))
        else:
            t = min(n, nxt(fam, "t", 34))
            put(p, f"F3t{t}", (n - t,))

    for idx, p in enumerate(payloads):
        n = len(p.data)
        todo = [fr for fr in framings if fr in ("F1", "F2") or (fr == "F3" and mode == 1)]
        if p.tag[0] == "H4" and n < params["ns_size"]:
            todo.remove("F1")  # rejected on its length alone, whatever the bytes: F2 and F3 only (the source's size)
        forced = "F4" in framings and idx in force_f4 and f4(p)
        ex = list(extra(idx, p)) if extra else []
        if ex and idx % 2:
            todo, ex = [], ex + [(fr, None) for fr in todo[::-1]]  # the cuts first and the Full last: see seam_source
        for fr in todo:
            place(p, fr, forced)
        for name, cuts in ex:
            if cuts is None:
                place(p, name, forced)
            else:
                put(p, name, cuts)
    data = f.data()
    assert len(data) < MAX_SOURCE, len(data)
    return Source(data, params, rows, placed)


_cache = {}


def _forced(ps, ns_size, m):
    """the payloads that get an F4 placement of their own, a block each: valid rows first, then a padded varint, a
    truncation inside the header and an overflowing varint; fewer where the namespace makes the source large"""
    want = [(m + "1", 3), (m + "1", 22), (m + "2", 5), (m + "4", ns_size // 2 + 4), (m + "1", 37), (m + "3", 1)]
    idx = []
    for fam, nth in want[:6 if ns_size < 128 else 0 if m == "H" and ns_size >= 200 else 2]:
        idx.append([i for i, p in enumerate(ps) if p.tag[0] == fam][nth])
    return tuple(idx)


def record_source(ns_size: int, etag_size: int) -> Source:
    key = (0, ns_size, etag_size)
    if key not in _cache:
        ps = record_payloads(ns_size, etag_size)
        _cache[key] = frame_source(ps, cases.params(ns_size, etag_size), force_f4=_forced(ps, ns_size, "R"),
                                   k0=7 * ns_size + etag_size)
    return _cache[key]


def hint_source(ns_size: int) -> Source:
    key = (1, ns_size)
    if key not in _cache:
        ps = hint_payloads(ns_size)
        _cache[key] = frame_source(ps, cases.params(ns_size, 20, mode=1), force_f4=_forced(ps, ns_size, "H"),
                                   k0=11 * ns_size)
    return _cache[key]


def decode(src: Source):
    p = src.params
    return O.decode(src.data, p["start_off"], p["base_time"], p["ns_size"], p["etag_size"], p["mode"])


# ---- R1 / H1 rows only, with distinct keys: what the consumers (index, filter, Get, scrub, encode) can read, since
# they stop at the first rejected row ----
def valid_filler(ns: bytes, etag_size: int, mode: int):
    """F4 fillers that are valid rows themselves: records (hints) with keys of their own whose values (keys) take up
    the space. Where the namespace leaves the header byte no room for a longer value varint, many short records."""
    nn = len(ns)

    def piece(t, row, j):
        """a valid payload of exactly t bytes, or None"""
        for kx in (0, 1):
            key = b"filler-%06d-%04d" % (row, j) + b"+" * kx
            if mode == 0:
                for vlv in (1, 2, 3):
                    vl = t - (nn + 4 + vlv) - len(key)
                    if vl >= 0 and len(uv(vl)) == vlv and nn + 4 + vlv <= 255:
                        return record(ns, 3, uv(len(key)), uv(vl), uv(0), b"", b"", key + blob(row + j, vl))[0]
            else:
                for klv in (1, 2, 3):
                    kl = t - nn - klv - 3
                    if kl >= len(key) and len(uv(kl)) == klv:
                        return hint(ns, uv(kl), key + blob(row + j, kl - len(key)), uv(1), uv(2), uv(3))[0]
        return None

    small = nn + 5 + 18                                     # the shortest piece
    large = 1 << 20 if mode == 1 or nn + 7 <= 255 else small + (16000 if nn + 6 <= 255 else 100)

    def fill(space, row):
        out = []
        while space > 0:
            t = space - cases.HDR
            if t > large:
                t = min(large, t - cases.HDR - small - 2)  # leave a last piece that can be valid
            p = piece(t, row, len(out)) if t >= small else None
            if p is None:
                return None
            out.append(p)
            space -= cases.HDR + len(p)
        return out
    return fill


def seam_records(ns_size: int, etag_size: int, gen: int = 0, klens=range(41)):
    """valid records whose key lengths walk 0..40, so ns || key passes 16k - 1, 16k and 16k + 1 at every ns_size; a
    key is its length's own (one byte value per length, then a counter), so every key is distinct; gen varies the
    value, the flags and with them the offsets of a second file"""
    ns, out = ns_of(ns_size), []
    for i, klen in enumerate(klens):
        key = bytes((klen * 5 + 1 + k) & 0xff for k in range(klen))
        j = i + gen
        e, x, t = j & 1, (j >> 1) & 1, int(j % 5 == 4)
        if ns_size + etag_size + 10 > 255:  # the header byte has no room for an etag and an expire
            e = x = 0
        flag = (0 if e else 1) | (0 if x else 2) | (4 if t else 0)
        val, meta = blob(j, (0, 3, 40, 17)[j % 4] + gen), METAS[j % 3]
        built = record(ns, flag, uv(klen), uv(len(val)), uv(len(meta)), etag_of(etag_size, j) if e else b"",
                       uv(DELTAS[j % 4]) if x else b"", key + val + meta)
        out.append(Payload(("R1", f"seam k{klen}g{gen}"), built[0], built[1]))
    return out


def seam_hints(ns_size: int, gen: int = 0, klens=range(41)):
    ns, out = ns_of(ns_size), []
    for i, klen in enumerate(klens):
        key = bytes((klen * 5 + 1 + k) & 0xff for k in range(klen))
        built = hint(ns, uv(klen), key, uv(3 + gen), uv(200 + 100 * i + gen), uv(30 + i))  # >= ns + 5 bytes
        out.append(Payload(("H1", f"seam k{klen}g{gen}"), built[0], built[1]))
    return out


def seam_source(ns_size: int, etag_size: int, mode: int, gen: int = 0, klens=range(41), force_f4=(5, 23)) -> Source:
    """F1, F2 (F3) and forced F4 placements of the seam rows, and a cut inside the namespace and one inside the key:
    the namespace, and separately the key, straddles two fragments. Every row is valid, the fillers included. Every
    other key's last placement is its Full one, which Wal.ReadRecord can read back (the cut framings are ones the
    iterator accepts and the writer never writes: a point read of them fails, in the reference as on the device)."""
    ps = seam_records(ns_size, etag_size, gen, klens) if mode == 0 else seam_hints(ns_size, gen, klens)
    ns_off = 1 if mode == 0 else 0

    def inside(i, p):
        """one cut inside the namespace and one inside the key, walking with i"""
        klen = 0 if p.hdr >= len(p.data) else (p.data[p.hdr - 1] if mode == 1 else p.data[ns_off + ns_size + 1])
        out = []
        if ns_size >= 2:
            out.append(("Cns", (ns_off + 1 + i % (ns_size - 1),)))
        if klen >= 2:
            out.append(("Ckey", (p.hdr + 1 + i % (klen - 1),)))
        return out

    src = frame_source(ps, cases.params(ns_size, etag_size, mode=mode), force_f4=force_f4,
                       filler=valid_filler(ns_of(ns_size), etag_size, mode), k0=3 * ns_size + gen, extra=inside)
    d = decode(src)
    assert d.err_class == 0 and (d.recs["status"] == 0).all() and len(d.recs) == len(src.rows)
    return src
