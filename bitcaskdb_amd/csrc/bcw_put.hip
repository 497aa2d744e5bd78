// bcw_put.hip -- MI355X (gfx950) kernels and entry points of the batched Write (DBImpl.Write, db_impl.go:343-431):
// records that arrive as field arrays are encoded (Record.Encode, record.go:57-138), framed into the active WAL
// (Wal.WriteRecord, wal.go:490-553) and applied to the device index (writeIndex, db_impl.go:434-454) without leaving
// HBM. bcw_encode.hip re-encodes rows of a decoded WAL through that decode's fragment table; here the payload is
// gathered from the caller's arrays.
//
// Pipeline (the index's context stream, no host synchronisation; DESIGN.md "Batched Write"):
//   k_put_prep    per record: validation, the header literal (headerSize | ns | flags | 3 varints | etag | expire),
//                 the payload size into EncScratch::sz, the first error as min (record << 2 | class)
//   enc_layout_run  the writer's layout recurrence: bcw_encode.hip's scan, event scan and k_recoff, unchanged
//   k_put_plan    one thread: the "accepted" word (no error and the bytes fit wal_cap) and bcw_write_result
//   k_put_frags   per record: rec_off / rec_size and the record's output fragments (blk_end arithmetic) appended to
//                 a fragment list
//   k_put_write   one wave per output fragment: 16 B output units gathered from the header literal, key, value and
//                 meta, stored, and folded into the fragment's CRC-32C; the record's first fragment zeroes the pad
//                 before it
//   ix_put_batch  the index ops (bcw_index.hip, SRC_BATCH) reading rec_off / rec_size and the accepted op count
// Every store of k_put_frags / k_put_write and every index op is predicated on the accepted word: a rejected batch
// leaves the output buffer, rec_off / rec_size and the index as they were (writeWal's ResetBuffer, db_impl.go:465-473).
#include <algorithm>
#include <cstring>
#include <vector>

#include "bcw_crc_dev.h"
#include "bcw_frame.h"
#include "bcw_host.h"

namespace bcw {
namespace put {

using namespace frame;  // the writer's framing rules (bcw_frame.h)

// emisc slots of the write (after the layouts' slots)
enum { P_ACC = kXPut, P_NIN = kXPut + 1, P_NFRAG = kXPut + 2, P_FOVER = kXPut + 3 };
// k_put_prep's error classes in the two low bits of emisc[kXErr]: BCW_ENC_ERR_EXPIRE (2) and BCW_ENC_ERR_PANIC (3) as
// k_enc_prep packs them, and 1 for BCW_ENC_ERR_BATCH
constexpr uint32_t kClsBatch = 1;

struct PutDev {
  uint64_t n;
  const uint8_t *keys, *vals, *metas, *etags, *flags;
  const uint64_t *koff, *voff, *moff, *expire;
  uint64_t keys_len, vals_len, metas_len;
  uint64_t base_time, wal_pos, wal_cap;
  uint8_t* out;
  uint64_t* rec_off;
  uint64_t* rec_size;
  uint32_t ns, etag, lstride;
};

// one output fragment (wal.go:519-546): header at file offset hp, flen payload bytes from payload offset x0
struct PFrag {
  uint64_t hp;
  uint32_t rec, x0, flen, type;
};
static_assert(sizeof(PFrag) == 24, "PFrag layout");

// ------------------------------------------------------------------------------------------
// k_put_prep: Record.Encode's header and size per record (record.go:57-138). The literal (record_header_put,
// bcw_frame.h; at most 2 + ns + 15 + etag + 5 bytes) is kept at lit + i * lstride for the writer.
__global__ __launch_bounds__(256) void k_put_prep(PutDev d, uint32_t* __restrict__ sz, uint8_t* __restrict__ lit,
                                                   uint32_t* __restrict__ hlen, uint64_t* __restrict__ emisc) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i == 0) emisc[kXNin] = d.n;
  if (i >= d.n) return;
  auto fail = [&](uint32_t cls) {
    atomicMin((unsigned long long*)&emisc[kXErr], (unsigned long long)(i << 2 | cls));
    sz[i] = 0;
  };
  const uint64_t k0 = d.koff[i], k1 = d.koff[i + 1], v0 = d.voff[i], v1 = d.voff[i + 1], m0 = d.moff[i],
                 m1 = d.moff[i + 1];
  // a record whose ranges do not lie inside the arrays is never read
  if (k0 > k1 || k1 > d.keys_len || v0 > v1 || v1 > d.vals_len || m0 > m1 || m1 > d.metas_len) return fail(kClsBatch);
  const uint64_t klm = k1 - k0, vl = v1 - v0, ml = m1 - m0;
  const int64_t hn = record_header_put(lit + i * (uint64_t)d.lstride, d.keys + k0, klm, d.ns, vl, ml,
                                       d.etags ? d.etags + i * (uint64_t)d.etag : nullptr, d.etag, d.expire[i],
                                       d.base_time, d.flags[i]);
  if (hn < 0) return fail(hn == -BCW_ENC_ERR_BATCH ? kClsBatch : (uint32_t)-hn);
  hlen[i] = (uint32_t)hn;
  sz[i] = (uint32_t)((uint64_t)hn + klm - d.ns + vl + ml);
}

// ------------------------------------------------------------------------------------------
// k_put_plan: the accepted word and the result. The layout ran over the records before the first error; a batch with
// an error appends nothing (wal_end = wal_pos).
__global__ void k_put_plan(PutDev d, uint64_t* __restrict__ emisc, bcw_write_result* __restrict__ r) {
  const uint64_t err = emisc[kXErr];
  const bool bad = (err >> 2) < d.n;
  const uint64_t end = (bad || d.n == 0) ? d.wal_pos : emisc[kXLayEnd];
  bcw_write_result o{};
  o.wal_end = end;
  o.wal_need = end - d.wal_pos;
  o.fits = o.wal_need <= d.wal_cap ? 1u : 0u;
  o.err_record = -1;
  if (bad) {
    const uint32_t cls = (uint32_t)(err & 3u);
    o.err_class = cls == kClsBatch ? BCW_ENC_ERR_BATCH : (int32_t)cls;
    o.err_record = (int64_t)(err >> 2);
  }
  const bool acc = !bad && o.fits;
  o.n_written = acc ? d.n : 0;
  emisc[P_ACC] = acc ? 1 : 0;
  emisc[P_NIN] = acc ? d.n : 0;
  *r = o;
}

// ------------------------------------------------------------------------------------------
// k_put_frags: per accepted record, locs (rec_off, rec_size: db_impl.go:475-476) and its output fragments: the
// writer's loop (wal.go:505-549) from the record's first header, one fragment per block it touches (a block with
// exactly 7 bytes left takes the zero-length First). The list's order is arbitrary: a fragment is self-contained.
__global__ __launch_bounds__(256) void k_put_frags(PutDev d, const uint32_t* __restrict__ sz,
                                                    const uint64_t* __restrict__ dpos, uint64_t* __restrict__ emisc,
                                                    PFrag* __restrict__ frags, uint64_t fcap) {
  const uint64_t j = blockIdx.x * 256ull + threadIdx.x;
  const bool on = emisc[P_ACC] != 0 && j < d.n;
  uint64_t P = 0, len = 0, cnt = 0;
  if (on) {
    P = dpos[j];
    len = sz[j];
    cnt = frag_count(P, len);
  }
  uint64_t f = wave_alloc(&emisc[P_NFRAG], cnt);
  if (!on) return;
  d.rec_off[j] = P;
  d.rec_size[j] = len;
  if (f + cnt > fcap) {  // the host sizes the list from bcw_write_bound: never expected
    atomicOr(reinterpret_cast<unsigned long long*>(&emisc[P_FOVER]), 1ull);
    return;
  }
  uint64_t hp = P, x0 = 0;
  for (bool first = true;; first = false) {
    const FragStep s = next_frag(hp, len - x0, first);
    frags[f++] = PFrag{hp, (uint32_t)j, (uint32_t)x0, (uint32_t)s.flen, s.type};
    x0 += s.flen;
    if (s.last) break;
    hp = s.be;
  }
}

// ------------------------------------------------------------------------------------------
// k_put_write. One wave per output fragment; lane l takes the fragment's 16 B output units l, l + 64, ... (units
// aligned to the output address, so interior units are one aligned 16 B store; the first and last unit of a fragment
// may be partial and are stored bytewise). A unit's bytes come from up to four inputs -- the record's header literal,
// key, value and meta -- each at its own byte alignment: per input an aligned pair of 16 B loads and a byte shift
// (shift16), where a granule of an input is loaded only when it holds a byte the unit needs, so no load touches a
// granule without a byte of the record's own range and none goes past an input's end (a boundary unit's unused load
// slots read the record's own literal slot in the scratch, gather_unit).
// CRC: each lane keeps a Horner chain c = A_{8*1024}(c) ^ R(unit) over its units (R: raw CRC-32C, init 0, bytes
// outside the fragment read as 0: leading zeros do not change R), the chains are shifted to the end of the last unit
// (A_{8*16*dn}, dn < 64 units follow the lane's last one), XOR-ed over the wave, the zero bytes after the fragment's
// end are undone by A_{8t}^-1, and A_{8 flen}(~0) (initc) supplies the init value. Lanes 0-6 store the header:
// ComputeCRC32 (utils.go:24-29), length, type.
// LDS (32.5 KiB per workgroup of 8 waves, 2 workgroups per CU at the kernel's registers): the slice-by-8 byte tables
// t8, the round operator A_{8*1024} as byte images, and the nibble-image operators of the final shift. Every table
// read is a ds_read_b32: 32 banks of 4 bytes, a wave
// served as two halves of 32 lanes. Operator tables are kOpStride = 144 words apart, i.e. 16 banks apart, and one
// nibble row is 16 words, so lanes applying different operators (different dn) in the final shift collide only on
// equal nibbles. The byte-table reads are data-dependent: 32 lanes on random banks of 32, a few ways of conflict
// on average, which no static layout removes; replicating the 8 KiB table per lane group would, at the price of the
// occupancy the gather's loads need, and is not done here.
constexpr int kPT = 512;
constexpr int kOpStride = 144;
#ifndef BCW_PUT_ROUNDS
#define BCW_PUT_ROUNDS 2
#endif
constexpr int kPutRounds = BCW_PUT_ROUNDS;  // units per lane whose source loads are in flight together
constexpr int kNOps = 21;  // A_{8*16*n} (n < 16), A_{8*256*n} (n < 5): [20] = A_{8*1024}, one round of the wave

struct WArgs {
  PutDev d;
  const uint64_t* emisc;
  const PFrag* frags;
  uint64_t fcap;
  const uint32_t* sz;
  const uint64_t* dpos;
  const uint8_t* lit;
  const uint32_t* hlen;
  const uint32_t* wops;   // enc_ops (layout in bcw_crc_consts.h)
  const uint32_t* initc;  // A_{8L}(0xFFFFFFFF)
};

// the 16 bytes at address a, of which only bytes [lo, hi) are needed (0 <= lo < hi <= 16) and known to lie inside
// the input: the aligned granule at a & ~15 is loaded when it holds one of them, and so is the next one
__device__ __forceinline__ uint4 load_unit(uint64_t a, int32_t lo, int32_t hi) {
  const uint32_t sh = (uint32_t)(a & 15u);
  const uint4* g = reinterpret_cast<const uint4*>((uintptr_t)(a & ~15ull));
  const uint4 z = make_uint4(0, 0, 0, 0);
  const uint4 v0 = (int32_t)sh + lo < 16 ? g[0] : z;
  const uint4 v1 = (int32_t)sh + hi > 16 ? g[1] : z;
  return shift16(v0, v1, sh);
}

// a record's payload as four inputs: input s covers payload offsets [z[s], z[s + 1]) and starts at address a[s]
struct Rec4 {
  int64_t z[5];
  uint64_t a[4];
};
// bytes [b0, b1) of the unit whose byte 0 is payload offset zb (the other bytes 0)
__device__ __forceinline__ uint4 gather_unit(const Rec4& R, int64_t zb, int32_t b0, int32_t b1) {
  const int64_t lo = zb + b0, hi = zb + b1;
  // the usual unit lies inside the value
  if (lo >= R.z[2] && hi <= R.z[3]) {
    const uint4 q = load_unit(R.a[2] + (uint64_t)(zb - R.z[2]), b0, b1);
    if (b1 - b0 == 16) return q;
    uint4 v = make_uint4(0, 0, 0, 0);
    or_masked(v, q, range_mask(b0, b1));
    return v;
  }
  // a unit at an input boundary: the loads of all four inputs are issued before any is used (one memory latency,
  // not four). An input the unit does not touch loads the record's literal slot instead, which is always there.
  uint4 g0[4], g1[4];
  int32_t u0[4], u1[4];
  uint32_t sh[4];
  const uint64_t spare = R.a[0] & ~15ull;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t s0 = max(lo, R.z[s]), s1 = min(hi, R.z[s + 1]);
    const bool need = s0 < s1;
    u0[s] = need ? (int32_t)(s0 - zb) : 0;
    u1[s] = need ? (int32_t)(s1 - zb) : 0;
    const uint64_t a = R.a[s] + (uint64_t)(zb - R.z[s]);
    sh[s] = (uint32_t)(a & 15u);
    const uint64_t Ba = a & ~15ull;
    const bool n0 = need && (int32_t)sh[s] + u0[s] < 16, n1 = need && (int32_t)sh[s] + u1[s] > 16;
    g0[s] = *reinterpret_cast<const uint4*>((uintptr_t)(n0 ? Ba : spare));
    g1[s] = *reinterpret_cast<const uint4*>((uintptr_t)(n1 ? Ba + 16 : spare));
  }
  uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int s = 0; s < 4; ++s) or_masked(v, shift16(g0[s], g1[s], sh[s]), range_mask(u0[s], u1[s]));
  return v;
}

__global__ __launch_bounds__(kPT) void k_put_write(WArgs A) {
  const PutDev& d = A.d;
  const uint64_t nfr = A.emisc[P_ACC] ? (A.emisc[P_NFRAG] < A.fcap ? A.emisc[P_NFRAG] : A.fcap) : 0;
  if ((uint64_t)blockIdx.x * (kPT / 64) >= nfr) return;  // rejected batch, or no fragment for this workgroup
  __shared__ uint32_t t8[8 * 256];
  __shared__ uint32_t sop[kNOps * kOpStride];
  __shared__ uint32_t sinv[16 * 128];  // A_{8t}^-1
  __shared__ uint32_t hopb[4 * 256];   // A_{8*1024} as byte images: the Horner step of every unit in 4 lookups, not 8
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  crc_byte_table(t8, tid, kPT);
  for (uint32_t i = tid; i < kNOps * 128; i += kPT) sop[(i >> 7) * kOpStride + (i & 127u)] = A.wops[i];
  for (uint32_t i = tid; i < 16 * 128; i += kPT) sinv[i] = A.wops[kOpInv * 128 + i];
  __syncthreads();
  crc_slice_tables<8>(t8, tid, kPT);
  __syncthreads();
  {
    const uint32_t* hop = sop + 20 * kOpStride;  // A_{8*1024}, nibble images
    for (uint32_t i = tid; i < 4 * 256; i += kPT) {
      const uint32_t k = i >> 8, b = i & 255u;
      hopb[i] = hop[(2 * k) * 16 + (b & 15u)] ^ hop[(2 * k + 1) * 16 + (b >> 4)];
    }
  }
  __syncthreads();
  const uint64_t nw = (uint64_t)gridDim.x * (kPT / 64);
  const uint64_t obase = (uint64_t)(uintptr_t)d.out;
  // the wave's index as a scalar: the fragment descriptor and the record's offsets are then wave-uniform (scalar
  // loads into SGPRs, not 64 copies in VGPRs)
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (uint64_t f = (uint64_t)blockIdx.x * (kPT / 64) + wv; f < nfr; f += nw) {
    const PFrag F = A.frags[f];
    const uint64_t i = F.rec, hp = F.hp, flen = F.flen;
    // defensive: the fragment lies inside the output (the layout and the plan guarantee it)
    if (hp < d.wal_pos || hp + kHdr + flen - d.wal_pos > d.wal_cap) continue;
    // zero pad before a record that starts a block (wal.go:509-512; at most 6 bytes)
    if (F.x0 == 0 && (F.type == BCW_RECORD_FULL || F.type == BCW_RECORD_FIRST) && starts_block(hp)) {
      const uint64_t prev = pad_start(i, d.wal_pos, [&] { return rec_end(A.dpos[i - 1], A.sz[i - 1]); });
      if (lane < kHdr && prev + lane < hp) d.out[prev + lane - d.wal_pos] = 0;
    }
    uint32_t acc = 0;
    if (flen) {
      Rec4 R;
      const uint64_t k0 = d.koff[i], k1 = d.koff[i + 1], v0 = d.voff[i], v1 = d.voff[i + 1], m0 = d.moff[i],
                     m1 = d.moff[i + 1];
      R.z[0] = 0;
      R.z[1] = A.hlen[i];
      R.z[2] = R.z[1] + (int64_t)(k1 - k0 - d.ns);
      R.z[3] = R.z[2] + (int64_t)(v1 - v0);
      R.z[4] = R.z[3] + (int64_t)(m1 - m0);
      R.a[0] = (uint64_t)(uintptr_t)(A.lit + i * (uint64_t)d.lstride);
      R.a[1] = (uint64_t)(uintptr_t)d.keys + k0 + d.ns;
      R.a[2] = (uint64_t)(uintptr_t)d.vals + v0;
      R.a[3] = (uint64_t)(uintptr_t)d.metas + m0;
      const uint64_t as = obase + (hp + kHdr - d.wal_pos), ae = as + flen;  // output addresses of the data
      const uint64_t uf = as >> 4, ul = (ae - 1) >> 4;
      const uint32_t nunits = (uint32_t)(ul - uf + 1);
      uint32_t c = 0;
      // kPutRounds units per lane are in flight together: first the aligned loads of the units that lie whole inside
      // the value (the usual unit), then, unit by unit, the byte shift (or the general gather), the store and the CRC
      for (uint32_t r0 = lane; r0 < nunits; r0 += 64 * kPutRounds) {
        uint4 g0[kPutRounds], g1[kPutRounds];
        uint32_t shv[kPutRounds];
        bool fast[kPutRounds];
#pragma unroll
        for (int q = 0; q < kPutRounds; ++q) {
          const uint32_t r = r0 + 64 * q;
          const uint64_t ua = (uf + r) << 4;
          const int64_t zb = (int64_t)F.x0 + ((int64_t)ua - (int64_t)as);  // payload offset of unit byte 0
          fast[q] = r < nunits && ua >= as && ua + 16 <= ae && zb >= R.z[2] && zb + 16 <= R.z[3];
          shv[q] = 0;
          g0[q] = g1[q] = make_uint4(0, 0, 0, 0);
          if (fast[q]) {
            const uint64_t a = R.a[2] + (uint64_t)(zb - R.z[2]);
            const uint4* g = reinterpret_cast<const uint4*>((uintptr_t)(a & ~15ull));
            shv[q] = (uint32_t)(a & 15u);
            g0[q] = g[0];
            if (shv[q]) g1[q] = g[1];  // 16 bytes from an unaligned address end in the next granule
          }
        }
#pragma unroll
        for (int q = 0; q < kPutRounds; ++q) {
          const uint32_t r = r0 + 64 * q;
          if (r >= nunits) continue;
          const uint64_t ua = (uf + r) << 4;
          const int32_t b0 = ua < as ? (int32_t)(as - ua) : 0;
          const int32_t b1 = ua + 16 > ae ? (int32_t)(ae - ua) : 16;
          const int64_t zb = (int64_t)F.x0 + ((int64_t)ua - (int64_t)as);
          const uint4 v = fast[q] ? shift16(g0[q], g1[q], shv[q]) : gather_unit(R, zb, b0, b1);
          uint8_t* q8 = reinterpret_cast<uint8_t*>((uintptr_t)ua);
          if (b1 - b0 == 16) {
            __builtin_nontemporal_store(v.x, reinterpret_cast<uint32_t*>(q8));
            __builtin_nontemporal_store(v.y, reinterpret_cast<uint32_t*>(q8) + 1);
            __builtin_nontemporal_store(v.z, reinterpret_cast<uint32_t*>(q8) + 2);
            __builtin_nontemporal_store(v.w, reinterpret_cast<uint32_t*>(q8) + 3);
          } else {
            for (int32_t b = b0; b < b1; ++b) q8[b] = (uint8_t)sel_byte(v, (uint32_t)b);
          }
          c = op_apply_b(hopb, c) ^ crc_step16(t8, 0u, v);
        }
      }
      // shift each lane's chain to the end of the fragment's last unit (dn < 64 units follow the lane's last one)
      if (lane < nunits) {
        const uint32_t dn = (nunits - 1 - lane) & 63u;
        if (dn & 15u) c = op_apply(sop + (dn & 15u) * kOpStride, c);
        if (dn >> 4) c = op_apply(sop + (16u + (dn >> 4)) * kOpStride, c);
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) c ^= __shfl_xor(c, m, 64);
      const uint32_t t = (uint32_t)(((ul + 1) << 4) - ae);
      acc = t ? op_apply(sinv + t * 128, c) : c;
    }
    if (lane < kHdr) {
      const uint32_t masked = mask_crc(~(acc ^ A.initc[flen]));
      d.out[hp - d.wal_pos + lane] = (uint8_t)frag_header_byte(masked, flen, F.type, lane);
    }
  }
}

}  // namespace put

namespace {

int put_scratch_reserve(bcw_ctx* c, uint64_t rows, uint64_t lit_bytes, uint64_t nfrags) {
  PutScratch& s = c->ps;
  if (rows <= s.rows_cap && lit_bytes <= s.lit_cap && nfrags <= s.frag_cap) return BCW_OK;
  (void)hipStreamSynchronize(c->cur);
  const uint64_t r = std::max(rows, s.rows_cap), l = std::max(lit_bytes, s.lit_cap), f = std::max(nfrags, s.frag_cap);
  const int wr = s.write_resident;
  s = PutScratch{};  // frees the three arrays
  if (!s.lit.alloc(l) || !s.hlen.alloc(r * 4) || !s.frags.alloc(f * sizeof(put::PFrag))) {
    s = PutScratch{};
    return BCW_E_NOMEM;
  }
  s.write_resident = wr;
  s.rows_cap = r;
  s.lit_cap = l;
  s.frag_cap = f;
  return BCW_OK;
}

// payload bytes Record.Encode adds to a record's key, value and meta: headerSize, flags, three varints of at most
// 5 bytes, the etag, the expire varint (ns is part of the merged key)
uint64_t enc_overhead(uint32_t etag_size) { return 2 + 15 + (uint64_t)etag_size + 5; }

}  // namespace
}  // namespace bcw

using namespace bcw;

extern "C" {

uint64_t bcw_write_bound(uint64_t n, uint64_t keys_len, uint64_t vals_len, uint64_t metas_len, uint32_t etag_size,
                         uint64_t wal_pos) {
  (void)wal_pos;  // the bound holds for every phase of wal_pos in the block grid
  // payloads + per record one header (7) and one pad (<= 6) + the leading pad (<= 6). With B bytes appended over nb
  // blocks: B <= raw + 7 nb (one continuation or zero-length-First header per block) and nb <= B / 32768 + 2, so
  // B <= (raw + 14) * 32768 / 32761.
  const uint64_t raw = keys_len + vals_len + metas_len + n * (enc_overhead(etag_size) + 13) + 6 + 14;
  return raw + (raw / (kBlock - kHdr) + 1) * kHdr;
}

int64_t bcw_record_encode(uint8_t* out, uint64_t cap, const uint8_t* merged_key, uint64_t key_len, const uint8_t* val,
                          uint64_t val_len, const uint8_t* meta, uint64_t meta_len, const uint8_t* etag,
                          uint64_t expire, uint32_t flags, uint32_t etag_size, uint64_t base_time, uint32_t ns_size) {
  // the header's length (or the error class) first: nothing is written into a buffer that is too small
  const int64_t hn = frame::record_header_put(nullptr, merged_key, key_len, ns_size, val_len, meta_len, etag, etag_size,
                                              expire, base_time, flags);
  if (hn < 0) return hn;
  const uint64_t kl = key_len - ns_size, total = (uint64_t)hn + kl + val_len + meta_len;
  if (total > cap || !out) return -BCW_ENC_ERR_TABLE;
  frame::record_header_put(out, merged_key, key_len, ns_size, val_len, meta_len, etag, etag_size, expire, base_time, flags);
  uint64_t o = (uint64_t)hn;
  auto app = [&](const uint8_t* p, uint64_t n) {
    if (n) memcpy(out + o, p, n);
    o += n;
  };
  app(merged_key + ns_size, kl);
  app(val, val_len);
  app(meta, meta_len);
  return (int64_t)o;
}

int bcw_write_records_async(bcw_index* ix, const bcw_write_params* p, const bcw_write_batch* b, const bcw_write_out* o,
                            bcw_write_result* d_result) {
  if (!ix || !p || !b || !o || !d_result) return BCW_E_INVAL;
  if (p->wal_pos < BCW_SUPER_BLOCK_SIZE || p->ns_size > 0xffffu || p->etag_size > 0xffffu) return BCW_E_INVAL;
  const uint64_t n = b->n;
  if (n >= 0xffffff00ull) return BCW_E_INVAL;  // u32 record ids
  if (n && (!b->key_off || !b->val_off || !b->meta_off || !b->expire || !b->flags || !o->rec_off || !o->rec_size))
    return BCW_E_INVAL;
  if ((b->keys_len && !b->keys) || (b->vals_len && !b->vals) || (b->metas_len && !b->metas) || (o->wal_cap && !o->wal))
    return BCW_E_INVAL;
  const bool stat = o->found || o->free_fid || o->free_bytes;
  if (stat && !(o->found && o->free_fid && o->free_bytes)) return BCW_E_INVAL;
  bcw_ctx* c = index_ctx(ix);
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  const uint32_t lstride = (uint32_t)((enc_overhead(p->etag_size) + p->ns_size + 15) & ~15ull);
  const uint64_t bound = bcw_write_bound(n, b->keys_len, b->vals_len, b->metas_len, p->etag_size, p->wal_pos);
  const uint64_t fcap = n + bound / kBlock + 2;  // every fragment after a record's first one starts a block
  int rc = enc_scratch_reserve(c, std::max<uint64_t>(n, 1));
  if (rc == BCW_OK) rc = put_scratch_reserve(c, std::max<uint64_t>(n, 1), std::max<uint64_t>(n, 1) * lstride, fcap);
  if (rc != BCW_OK) return rc;
  hipStream_t st = c->cur;
  EncScratch& es = c->es;
  PutScratch& ps = c->ps;
  Prof& pr = c->prof;
  hipEvent_t ev = nullptr;

  put::PutDev d{};
  d.n = n;
  d.keys = b->keys;
  d.vals = b->vals;
  d.metas = b->metas;
  d.etags = b->etags;
  d.flags = b->flags;
  d.koff = b->key_off;
  d.voff = b->val_off;
  d.moff = b->meta_off;
  d.expire = b->expire;
  d.keys_len = b->keys_len;
  d.vals_len = b->vals_len;
  d.metas_len = b->metas_len;
  d.base_time = p->base_time;
  d.wal_pos = p->wal_pos;
  d.wal_cap = o->wal_cap;
  d.out = o->wal;
  d.rec_off = o->rec_off;
  d.rec_size = o->rec_size;
  d.ns = p->ns_size;
  d.etag = p->etag_size;
  d.lstride = lstride;
  const uint32_t grid = (uint32_t)((n + 255) / 256);

  enc_layout_reset(es, st);
  if (n) {
    pr.begin(K_PUT_PREP, st, ev);
    put::k_put_prep<<<grid, 256, 0, st>>>(d, es.sz.get(), ps.lit.get(), ps.hlen.get(), es.emisc.get());
    pr.end(K_PUT_PREP, st, ev);
    pr.begin(K_PUT_LAYOUT, st, ev);
    if (enc_layout_run(es, n, p->wal_pos, st) != hipSuccess) return BCW_E_HIP;
    pr.end(K_PUT_LAYOUT, st, ev);
  }
  pr.begin(K_PUT_FRAGS, st, ev);
  put::k_put_plan<<<1, 1, 0, st>>>(d, es.emisc.get(), d_result);
  if (n) put::k_put_frags<<<grid, 256, 0, st>>>(d, es.sz.get(), es.dpos.get(), es.emisc.get(),
                                           static_cast<put::PFrag*>(ps.frags.get()), fcap);
  pr.end(K_PUT_FRAGS, st, ev);
  if (n) {
    put::WArgs W{};
    W.d = d;
    W.emisc = es.emisc.get();
    W.frags = static_cast<const put::PFrag*>(ps.frags.get());
    W.fcap = fcap;
    W.sz = es.sz.get();
    W.dpos = es.dpos.get();
    W.lit = ps.lit.get();
    W.hlen = ps.hlen.get();
    W.wops = c->tabs.enc_ops;
    W.initc = c->tabs.initc;
    // a grid of resident workgroups: each wave walks the fragment list with the grid's stride, and the tables are
    // built a bounded number of times however long the list is
    const uint64_t want = (fcap + put::kPT / 64 - 1) / (put::kPT / 64);
    if (ps.write_resident == 0 &&
        (hipOccupancyMaxActiveBlocksPerMultiprocessor(&ps.write_resident, put::k_put_write, put::kPT, 0) != hipSuccess ||
         ps.write_resident < 1))
      ps.write_resident = 2;
    const uint32_t wgrid =
        (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->num_cus * ps.write_resident));
    pr.begin(K_PUT_WRITE, st, ev);
    put::k_put_write<<<wgrid, put::kPT, 0, st>>>(W);
    pr.end(K_PUT_WRITE, st, ev);
  }
  if (hipGetLastError() != hipSuccess) return BCW_E_HIP;
  PutIx q{};
  q.n = n;
  q.keys = b->keys;
  q.koff = b->key_off;
  q.keys_len = b->keys_len;
  q.n_in = es.emisc.get() + put::P_NIN;
  q.rec_off = o->rec_off;
  q.rec_size = o->rec_size;
  q.flags = b->flags;
  q.fid = p->fid;
  q.found = o->found;
  q.free_fid = o->free_fid;
  q.free_bytes = o->free_bytes;
  q.idx_err = &d_result->idx_err;
  pr.begin(K_PUT_INDEX, st, ev);
  rc = ix_put_batch(ix, q);
  pr.end(K_PUT_INDEX, st, ev);
  return rc;
}

int bcw_write_records(bcw_index* ix, const bcw_write_params* p, const bcw_write_batch* hb, const bcw_write_out* ho,
                      bcw_write_result* h_result) {
  if (!ix || !p || !hb || !ho || !h_result) return BCW_E_INVAL;
  const uint64_t n = hb->n;
  if (n && (!hb->key_off || !hb->val_off || !hb->meta_off || !hb->expire || !hb->flags || !ho->rec_off || !ho->rec_size))
    return BCW_E_INVAL;
  if (ho->wal_cap && !ho->wal) return BCW_E_INVAL;
  const bool stat = ho->found || ho->free_fid || ho->free_bytes;
  if (stat && !(ho->found && ho->free_fid && ho->free_bytes)) return BCW_E_INVAL;
  *h_result = bcw_write_result{};
  uint64_t kb = 0, vb = 0, mb = 0;
  bool any_etag = false;
  if (n) {
    for (uint64_t i = 0; i < n; ++i) {
      if (hb->key_off[i + 1] < hb->key_off[i] || hb->val_off[i + 1] < hb->val_off[i] ||
          hb->meta_off[i + 1] < hb->meta_off[i])
        return BCW_E_INVAL;
      any_etag = any_etag || (hb->flags[i] & BCW_WR_ETAG);
    }
    kb = hb->key_off[n] - hb->key_off[0];
    vb = hb->val_off[n] - hb->val_off[0];
    mb = hb->meta_off[n] - hb->meta_off[0];
    if ((kb && !hb->keys) || (vb && !hb->vals) || (mb && !hb->metas)) return BCW_E_INVAL;
    if (any_etag && p->etag_size && !hb->etags) return BCW_E_INVAL;
  }
  bcw_ctx* c = index_ctx(ix);
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  const uint64_t eb = (any_etag && hb->etags) ? n * (uint64_t)p->etag_size : 0;
  DevBuf<> mem;
  PutLayout L;
  if (int rc = carve_alloc(mem, [&](Carver& cv) { L = carve_put(cv, kb, vb, mb, eb, ho->wal_cap, n, stat); })) return rc;
  const bcw_write_out& d = L.out;
  bcw_write_batch db{};
  db.n = n;
  db.keys = kb ? L.keys : nullptr;
  db.key_off = L.offs;
  db.keys_len = kb;
  db.vals = vb ? L.vals : nullptr;
  db.val_off = L.offs + (n + 1);
  db.vals_len = vb;
  db.metas = mb ? L.metas : nullptr;
  db.meta_off = L.offs + 2 * (n + 1);
  db.metas_len = mb;
  db.etags = eb ? L.etags : nullptr;
  db.expire = L.expire;
  db.flags = L.flags;
  hipStream_t st = c->cur;
  std::vector<uint64_t> off(3 * (n + 1));
  for (uint64_t i = 0; n && i <= n; ++i) {
    off[i] = hb->key_off[i] - hb->key_off[0];
    off[n + 1 + i] = hb->val_off[i] - hb->val_off[0];
    off[2 * (n + 1) + i] = hb->meta_off[i] - hb->meta_off[0];
  }
  bool ok = true;
  if (n)
    ok = copy_up(L.keys, kb ? hb->keys + hb->key_off[0] : nullptr, kb, st) &&
         copy_up(L.vals, vb ? hb->vals + hb->val_off[0] : nullptr, vb, st) &&
         copy_up(L.metas, mb ? hb->metas + hb->meta_off[0] : nullptr, mb, st) && copy_up(L.etags, hb->etags, eb, st) &&
         copy_up(L.offs, off.data(), 3 * 8 * (n + 1), st) && copy_up(L.expire, hb->expire, 8 * n, st) &&
         copy_up(L.flags, hb->flags, n, st);
  int rc = ok ? bcw_write_records_async(ix, p, &db, &d, L.res) : BCW_E_HIP;
  if (rc == BCW_OK) {
    ok = copy_down(h_result, L.res, sizeof(bcw_write_result), st) && hipStreamSynchronize(st) == hipSuccess;
    rc = !ok ? BCW_E_HIP : h_result->fits ? BCW_OK : BCW_E_CAPACITY;
  }
  if (rc == BCW_OK && h_result->n_written) {
    ok = copy_down(ho->wal, d.wal, h_result->wal_need, st) && copy_down(ho->rec_off, d.rec_off, 8 * n, st) &&
         copy_down(ho->rec_size, d.rec_size, 8 * n, st);
    if (ok && stat)
      ok = copy_down(ho->found, d.found, n, st) && copy_down(ho->free_fid, d.free_fid, 8 * n, st) &&
           copy_down(ho->free_bytes, d.free_bytes, 8 * n, st);
    if (!ok) rc = BCW_E_HIP;
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == BCW_OK) rc = BCW_E_HIP;  // before mem goes
  return rc;
}

}  // extern "C"
