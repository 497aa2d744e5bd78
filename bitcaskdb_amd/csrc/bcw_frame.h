// bcw_frame.h -- the WAL writer's framing rules (Wal.WriteRecord, wal.go:490-553), ComputeCRC32's mask
// (utils.go:24-29), Go's PutUvarint and Record.Encode's header (record.go:57-138): the single home of these rules.
// Plain inline functions compiled by the host (bcw_api.cpp, bcw_put.hip's host entry points), by the writer kernels
// (bcw_encode.hip, bcw_put.hip, bcw_read_body.h) and by the stand-alone host check (tools/frame_check.cpp), as
// bcw_rules.h and bcw_usage.h are: one text for all three. No device calls here.
#pragma once
#include "bcw.h"

#if defined(__HIPCC__)
#define BCW_FRAME_FN __host__ __device__ __forceinline__
#else
#define BCW_FRAME_FN inline
#endif

namespace bcw {
namespace frame {

constexpr uint32_t kB = BCW_BLOCK_SIZE;                    // 32768
constexpr uint32_t kH = BCW_HEADER_SIZE;                   // 7
constexpr uint32_t kD = BCW_BLOCK_SIZE - BCW_HEADER_SIZE;  // 32761: the data of a whole block

// Go binary.PutUvarint: its length, and the bytes
BCW_FRAME_FN uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) { v >>= 7; ++n; }
  return n;
}
BCW_FRAME_FN uint32_t uvarint_put(uint8_t* p, uint64_t v) {
  uint32_t n = 0;
  while (v >= 0x80) { p[n++] = (uint8_t)(v | 0x80); v >>= 7; }
  p[n++] = (uint8_t)v;
  return n;
}

// ComputeCRC32 (utils.go:24-29) of a fragment's CRC-32C c
BCW_FRAME_FN uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// first file offset past the block that holds P
BCW_FRAME_FN uint64_t blk_end(uint64_t P) { return P + kB - (P - BCW_SUPER_BLOCK_SIZE) % kB; }
// payload bytes the block of a header at P holds after it
BCW_FRAME_FN uint64_t frag_room(uint64_t P) { return blk_end(P) - (P + kH); }
// fragments of a record whose first header is at P, with a payload of len > 0 bytes
BCW_FRAME_FN uint64_t frag_count(uint64_t P, uint64_t len) {
  const uint64_t x1 = frag_room(P);
  return len <= x1 ? 1 : 1 + (len - x1 + kD - 1) / kD;
}
// file offset just past that record
BCW_FRAME_FN uint64_t rec_end(uint64_t P, uint64_t len) {
  const uint64_t be = blk_end(P), ds = P + kH;
  if (ds + len <= be) return ds + len;
  const uint64_t rem = len - (be - ds);
  const uint64_t q = (rem - 1) / kD;  // whole continuation blocks before the last fragment
  return be + q * kB + kH + (rem - q * kD);
}

// One step of the writer's loop (wal.go:505-549): the fragment whose header is at hp when rem payload bytes are
// left. Its data [ds, ds + flen) runs to the end of the block at the most, the next header is at be. A block with
// exactly 7 bytes left takes a zero-length First.
struct FragStep {
  uint64_t be, ds, flen;
  uint32_t type;  // BCW_RECORD_*
  bool last;
};
BCW_FRAME_FN FragStep next_frag(uint64_t hp, uint64_t rem, bool first) {
  FragStep s;
  s.be = blk_end(hp);
  s.ds = hp + kH;
  s.flen = rem < s.be - s.ds ? rem : s.be - s.ds;
  s.last = s.flen == rem;
  s.type = first ? (s.last ? BCW_RECORD_FULL : BCW_RECORD_FIRST) : (s.last ? BCW_RECORD_LAST : BCW_RECORD_MIDDLE);
  return s;
}

// byte i of a fragment header (its low 8 bits): masked CRC (LE32), length (LE16), type
BCW_FRAME_FN uint32_t frag_header_byte(uint32_t masked, uint64_t flen, uint32_t type, uint32_t i) {
  return i < 4 ? (masked >> (8 * i)) : i == 4 ? (uint32_t)flen : i == 5 ? (uint32_t)(flen >> 8) : type;
}
BCW_FRAME_FN void store_frag_header(uint8_t* h, uint32_t masked, uint64_t flen, uint32_t type) {
  for (uint32_t i = 0; i < kH; ++i) h[i] = (uint8_t)frag_header_byte(masked, flen, type, i);
}

// The zero pad (wal.go:509-512). Only a record whose first header P starts a block can have one: the previous block
// ended with fewer than 7 bytes left. The pad runs from pad_start to P: from where the previous record ended, or for
// record 0 from pos, where the write started. prev_end() gives the previous record's end and is called only when
// there is one, so it may read element j - 1 of the writer's arrays.
BCW_FRAME_FN bool starts_block(uint64_t P) { return (P - BCW_SUPER_BLOCK_SIZE) % kB == 0; }
template <class PrevEnd>
BCW_FRAME_FN uint64_t pad_start(uint64_t j, uint64_t pos, PrevEnd prev_end) {
  return j == 0 ? pos : prev_end();
}

// Record.Encode's header (record.go:57-138): headerSize | ns | flags | uvarint(len(key)) | uvarint(len(value)) |
// uvarint(len(meta)) | etag | uvarint(expire - baseTime), at most 2 + ns_size + 15 + etag_size + 5 bytes, into out
// (NULL: nothing is written, the return value is the same). merged_key = ns || key, of which only the ns_size bytes
// of ns are read; flags = BCW_WR_* (the etag is read only with BCW_WR_ETAG). Returns the header's length, or minus the
// BCW_ENC_ERR_* class with nothing written: what the batch cannot express, then "invalid expire" (record.go:74), then
// the panic of a delta the 5-byte varint array cannot hold. headerSize is truncated to a byte (record.go:109).
BCW_FRAME_FN int64_t record_header_put(uint8_t* out, const uint8_t* merged_key, uint64_t merged_len, uint32_t ns_size,
                                       uint64_t val_len, uint64_t meta_len, const uint8_t* etag, uint32_t etag_size,
                                       uint64_t expire, uint64_t base_time, uint32_t flags) {
  if (merged_len < ns_size || (merged_len | val_len | meta_len) >> 32) return -BCW_ENC_ERR_BATCH;
  const uint32_t el = (flags & BCW_WR_ETAG) ? etag_size : 0u;
  if (el && !etag) return -BCW_ENC_ERR_BATCH;
  const uint64_t kl = merged_len - ns_size;
  uint32_t flag = (el == 0 ? 1u : 0u) | ((flags & BCW_WR_TOMBSTONE) ? 4u : 0u);
  uint64_t delta = 0;
  uint32_t ve = 0;
  if (expire == 0) {
    flag |= 2u;
  } else {
    if (expire < base_time) return -BCW_ENC_ERR_EXPIRE;
    delta = expire - base_time;
    if (delta >= (1ull << 35)) return -BCW_ENC_ERR_PANIC;
    ve = uvarint_len(delta);
  }
  const uint64_t hn = 2ull + ns_size + uvarint_len(kl) + uvarint_len(val_len) + uvarint_len(meta_len) + el + ve;
  if ((hn + kl + val_len + meta_len) >> 32) return -BCW_ENC_ERR_BATCH;
  if (!out) return (int64_t)hn;
  uint32_t o = 0;
  out[o++] = (uint8_t)hn;
  for (uint32_t b = 0; b < ns_size; ++b) out[o++] = merged_key[b];
  out[o++] = (uint8_t)flag;
  o += uvarint_put(out + o, kl);
  o += uvarint_put(out + o, val_len);
  o += uvarint_put(out + o, meta_len);
  for (uint32_t b = 0; b < el; ++b) out[o++] = etag[b];
  if (ve) o += uvarint_put(out + o, delta);
  return (int64_t)hn;
}

}  // namespace frame
}  // namespace bcw
