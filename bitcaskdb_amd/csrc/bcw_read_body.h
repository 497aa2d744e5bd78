// bcw_read_body.h -- the per-request body of a point read, shared by k_read_records (bcw_read.hip: one WAL image,
// caller-given payload offsets), k_get_read (bcw_get.hip: each request against the image its index value names) and
// k_vfy_read (bcw_verify.hip: every index entry against its image, nothing copied):
// WalRecordSize (wal.go:61-86), WalParseRecord (wal.go:121-173: the fragment walk over the record's physical span,
// optional CRC verify, size check) and RecordFromBytes (record.go:140-239). The mapping to the reference's errors
// (BCW_RD_*, BCW_ST_*) lives here only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bcw_crc_dev.h"
#include "bcw_frame.h"
#include "bcw_internal.h"
#include "bcw_parse.h"

namespace bcw {

namespace rd {

constexpr int kMaxF = 64;  // fragments recorded for the header parse (the header lies in the first ones)

// WalRecordSize (wal.go:61-86), uint64 arithmetic. The loop runs size / 32761 + 1 times: a caller that takes `size`
// from an index (k_get_lookup) bounds it by the image's length first.
__device__ __forceinline__ uint64_t wal_record_size(uint64_t offset, uint64_t size) {
  uint64_t left = size, phy = 0;
  offset -= 40;
  while (left > 0) {
    uint64_t leftover = kBlock - (offset % kBlock);
    if (leftover < kHdr) {
      phy += leftover;
      offset += leftover;
      leftover = kBlock;
    }
    const uint64_t frag = left < leftover - kHdr ? left : leftover - kHdr;
    phy += kHdr + frag;
    offset += kHdr + frag;
    left -= frag;
  }
  return phy;
}

__device__ __forceinline__ uint32_t byte_at(const uint8_t* __restrict__ seg, uint64_t n, uint64_t a) {
  return a < n ? seg[a] : 0u;
}

// the payload's bytes through the fragment list recorded in LDS
struct FragReader {
  const uint8_t* seg;
  uint64_t seg_len;
  const uint64_t* fo;  // segment offset of each fragment's data
  const uint32_t* fl;  // its length
  uint32_t nf;
  __device__ __forceinline__ uint32_t operator()(uint64_t pos) const {
    for (uint32_t f = 0; f < nf; ++f) {
      if (pos < fl[f]) return byte_at(seg, seg_len, fo[f] + pos);
      pos -= fl[f];
    }
    return 0;
  }
};

// what a request reads from: the WAL image, the verify tables in LDS (t0: the CRC-32C byte table, sp2: kPow2Ops
// nibble images of A_{8 * 2^k}) and in HBM (initc), and the wave's fragment list in LDS (kMaxF entries each)
struct ReadEnv {
  const uint8_t* seg;
  uint64_t seg_len;
  uint32_t verify;
  const uint32_t* t0;
  const uint32_t* sp2;
  const uint32_t* initc;
  uint64_t* fo;
  uint32_t* fl;
};

// cl bytes of the image at ds -> dst, by all lanes of the wave, one 16 B unit per lane and round
// kWide = false: a unit is sixteen guarded byte loads and up to sixteen byte stores
// kWide = true:  the units are aligned to the destination; each is two aligned 16 B loads of the image (shift16 takes
//                the unit out of them) and one 16 B store, while the 32 B window lies inside the image; the ragged
//                head (up to the destination's first 16 B boundary), the tail and a window that leaves the image
//                keep the byte path
template <bool kWide>
__device__ __forceinline__ void copy_fragment(const ReadEnv& E, uint64_t ds, uint8_t* __restrict__ dst, uint64_t cl,
                                              uint32_t lane) {
  const uint8_t* __restrict__ seg = E.seg;
  const uint64_t n = E.seg_len;
  uint64_t head = 0;
  if (kWide) {
    head = (0 - reinterpret_cast<uintptr_t>(dst)) & 15u;
    if (head > cl) head = cl;
    if (lane < head) dst[lane] = (uint8_t)byte_at(seg, n, ds + lane);
    const uint64_t units = (cl - head) / 16;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(seg), s1 = s0 + n;
    for (uint64_t u = lane; u < units; u += 64) {
      const uint64_t b = head + 16 * u;
      const uintptr_t a = s0 + ds + b, q = a & ~(uintptr_t)15;
      const uint32_t sh = (uint32_t)(a & 15u);
      uint4 v;
      if (ds + b + 16 <= n && q >= s0 && q + (sh ? 32 : 16) <= s1) {
        const uint4 v0 = *reinterpret_cast<const uint4*>(q);
        v = sh ? shift16(v0, *reinterpret_cast<const uint4*>(q + 16), sh) : v0;
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k >> 2] |= byte_at(seg, n, ds + b + k) << (8 * (k & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *reinterpret_cast<uint4*>(dst + b) = v;
    }
    head += 16 * units;
    if (head + lane < cl) dst[head + lane] = (uint8_t)byte_at(seg, n, ds + head + lane);  // < 16 bytes left
    return;
  }
  for (uint64_t b = (uint64_t)lane * 16; b < cl; b += 64 * 16) {
    uint8_t tmp[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tmp[k] = (uint8_t)byte_at(seg, n, ds + b + k);
    const uint64_t m = cl - b < 16 ? cl - b : 16;
    for (uint64_t k = 0; k < m; ++k) dst[b + k] = tmp[k];
  }
}

// WalParseRecord(size, 0, [][]byte{buffer}, verify) with buffer = the image's [off, off + rs), rs = WalRecordSize(off,
// size) and off + rs inside the image (the caller reports BCW_RD_BEYOND otherwise). All lanes of one wave; every
// argument but `lane` is wave-uniform. Copies the record into out[0, size), records the first kMaxF fragments in E.fo /
// E.fl (visible to the wave after the caller's wave barrier) and returns BCW_RD_*; nf: fragments walked.
// kCopy = false (the scrub, k_vfy_read): the same walk with no byte stored; `out` is not read.
template <bool kWide, bool kCopy = true>
__device__ __forceinline__ uint32_t read_walk(const ReadEnv& E, uint64_t off, uint64_t size, uint64_t rs,
                                              uint8_t* __restrict__ out, uint32_t lane, uint32_t& nf) {
  const uint8_t* seg = E.seg;
  const uint64_t n = E.seg_len;
  uint32_t st = BCW_RD_OK;
  uint64_t bo = 0, got = 0;
  nf = 0;
  for (;;) {
    if (bo + kHdr > rs) { st = BCW_RD_PANIC; break; }  // header := blks[0][blkOff:blkOff+7] out of range
    const uint64_t ha = off + bo;
    const uint32_t crc = byte_at(seg, n, ha) | byte_at(seg, n, ha + 1) << 8 | byte_at(seg, n, ha + 2) << 16 |
                         byte_at(seg, n, ha + 3) << 24;
    const uint64_t len = byte_at(seg, n, ha + 4) | byte_at(seg, n, ha + 5) << 8;
    const uint32_t type = byte_at(seg, n, ha + 6);
    bo += kHdr;
    if (len > rs - bo) { st = BCW_RD_CORRUPTED; break; }  // ErrWalCorruptedData
    const uint64_t ds = off + bo;  // the fragment's data in the segment
    bo += len;
    if (nf < (uint32_t)kMaxF && lane == 0) { E.fo[nf] = ds; E.fl[nf] = (uint32_t)len; }
    ++nf;
    // copy what fits the payload slot (record = append(record, data...); a longer record is a size error)
    const uint64_t cl = got < size ? (len < size - got ? len : size - got) : 0;
    if (kCopy) copy_fragment<kWide>(E, ds, out + got, cl, lane);
    if (E.verify) {
      // lane l: raw CRC-32C (init 0) of its chunk [l*c, min((l+1)*c, len)), shifted to the data end
      const uint64_t c = (len + 63) / 64;
      const uint64_t a0 = (uint64_t)lane * c, a1 = a0 + c < len ? a0 + c : len;
      uint32_t x = 0;
      for (uint64_t q = a0; q < a1; ++q) x = (x >> 8) ^ E.t0[(x ^ byte_at(seg, n, ds + q)) & 0xffu];
      if (a0 < a1) {
        uint64_t dsh = len - a1;  // zero bytes after the chunk
        for (int k = 0; dsh; ++k, dsh >>= 1)
          if (dsh & 1u) x = op_apply(E.sp2 + k * 128, x);
      } else {
        x = 0;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) x ^= (uint32_t)__shfl_xor((int)x, d, 64);
      // the init contribution A_{8L}(~0): the table up to one block, beyond (crafted lengths) by shifts
      uint32_t ic = E.initc[len <= kBlock ? len : kBlock];
      for (uint64_t dsh = len > kBlock ? len - kBlock : 0, k = 0; dsh; ++k, dsh >>= 1)
        if (dsh & 1u) ic = op_apply(E.sp2 + k * 128, ic);
      // CRC-32C = ~crc_update(~0, data)
      if (frame::mask_crc(~(x ^ ic)) != crc) { st = BCW_RD_CRC; break; }
    }
    got += len;
    if (type == BCW_RECORD_FULL || type == BCW_RECORD_LAST) {
      if (got != size) st = BCW_RD_SIZE;  // ErrWalMismatchSize
      break;
    }
    if (type != BCW_RECORD_FIRST && type != BCW_RECORD_MIDDLE) { st = BCW_RD_TYPE; break; }
    if (rs - bo <= kHdr) { st = BCW_RD_INCOMPLETE; break; }  // leftover <= 7: the block loop ends
  }
  return st;
}

// fill the LDS verify tables of a workgroup of `threads` threads (the caller's __syncthreads follows)
__device__ __forceinline__ void load_verify_tables(uint32_t* t0, uint32_t* sp2, const uint32_t* __restrict__ pow2,
                                                   uint32_t tid, uint32_t threads) {
  crc_byte_table(t0, tid, threads);
  for (uint32_t i = tid; i < kPow2Ops * 128; i += threads) sp2[i] = pow2[i];
}

// RecordFromBytes' fields of one request (zeros unless the read succeeded)
struct ReadRow {
  uint8_t status = BCW_ST_OK, hdr = 0, flags = 0, etag_off = 0;
  uint64_t kl = 0, vl = 0, ml = 0, expire = 0;
};

// one lane, after the wave barrier that follows read_walk: RecordFromBytes (record.go:140-239) of a request whose
// read gave BCW_RD_OK, straight from the image through the recorded fragment list
__device__ __forceinline__ ReadRow read_parse(const ReadEnv& E, uint64_t base_time, uint32_t ns_size,
                                              uint32_t etag_size, uint64_t size, uint32_t nf) {
  bcw_decode_params dp{};
  dp.seg_len = E.seg_len;
  dp.base_time = base_time;
  dp.ns_size = ns_size;
  dp.etag_size = etag_size;
  dp.mode = BCW_MODE_RECORD;
  ReadRow R;
  uint64_t x0 = 0, x1 = 0;
  FragReader fr{E.seg, E.seg_len, E.fo, E.fl, nf < (uint32_t)kMaxF ? nf : (uint32_t)kMaxF};
  parse_record(dp, fr, size, R.status, R.hdr, R.flags, R.etag_off, R.kl, R.vl, R.ml, R.expire, x0, x1);
  return R;
}

// row r of the request table (bcw_read_records_async's meaning: foff = offset + 7)
__device__ __forceinline__ void write_row(const bcw_record_table& t, uint64_t r, uint64_t off, uint64_t size,
                                          uint32_t nf, const ReadRow& R) {
  if (r >= t.capacity) return;
  t.foff[r] = off + kHdr;
  t.size[r] = size;
  t.expire[r] = R.expire;
  t.key_len[r] = (uint32_t)R.kl;
  t.val_len[r] = (uint32_t)R.vl;
  t.meta_len[r] = (uint32_t)R.ml;
  if (t.first_frag) t.first_frag[r] = 0;
  if (t.emit_frag) t.emit_frag[r] = nf ? nf - 1 : 0;
  t.hdr_size[r] = R.hdr;
  t.flags[r] = R.flags;
  t.etag_off[r] = R.etag_off;
  t.status[r] = R.status;
}

}  // namespace rd
}  // namespace bcw
