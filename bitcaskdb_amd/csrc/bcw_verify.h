// bcw_verify.h -- the scrub of the device index against the resident WALs (bcw_index_verify*; bcw.h): what DBImpl.Get
// (db_impl.go:567-587) of every live, file-backed entry would run into, plus the one check Get does not make -- that
// the record at (fid, off, size) carries the entry's key.
//
// Two parts. The decisions -- the class of an entry from (wal found, rd_status, rec_status, key equal), the span
// pre-check that keeps an untrusted size out of WalRecordSize's loop, and the `fits` rule -- are plain inline
// functions compiled by the host, the kernels (k_ix_vfy_select and k_get_lookup in bcw_index.hip, k_vfy_read in
// bcw_verify.hip) and the stand-alone host check (tools/verify_check.cpp), as bcw_drop.h and bcw_rules.h are: one
// text for all three. The rest is the device side both kernels share (HIP only): the work item, the call's counters
// and the one function that emits a bad entry.
#pragma once
#include <cstdint>

#include "bcw.h"

#if defined(__HIPCC__)
#define BCW_VFY_FN __host__ __device__ __forceinline__
#else
#define BCW_VFY_FN inline
#endif

namespace bcw {
namespace vfy {

// Get's order (db_impl.go:567-587): getWalRef, Wal.ReadRecord, RecordFromBytes; then the key compare. Each later
// argument is read only when the earlier ones passed.
BCW_VFY_FN uint32_t classify(bool wal_found, uint32_t rd_status, uint32_t rec_status, bool key_equal) {
  if (!wal_found) return BCW_VFY_NO_WAL;
  if (rd_status != BCW_RD_OK) return BCW_VFY_READ;
  if (rec_status != BCW_ST_OK) return BCW_VFY_RECORD;
  return key_equal ? BCW_VFY_OK : BCW_VFY_KEY;
}

// An index value is not trusted: a size beyond the image, an off inside the super block (the reference's
// WalRecordSize wraps there) or beyond the image is "read beyond file size" (wal.go:562-564) before WalRecordSize's
// loop (size / 32761 rounds) is entered. false: the loop is bounded by seg_len and off + WalRecordSize cannot wrap.
BCW_VFY_FN bool span_untrusted(uint64_t off, uint64_t size, uint64_t seg_len) {
  return size > seg_len || off < BCW_SUPER_BLOCK_SIZE || off > seg_len;
}

// ReadRecord's own test, for a span that passed span_untrusted: rs = WalRecordSize(off, size)
BCW_VFY_FN bool span_beyond(uint64_t off, uint64_t rs, uint64_t seg_len) { return off + rs > seg_len; }

// the list, the key bytes and the rows are whole only when every one of them had room
BCW_VFY_FN bool fits(uint64_t n_bad, uint64_t bad_cap, uint64_t key_bytes, uint64_t keys_cap, uint64_t n_fids,
                     uint64_t rows_cap, bool rows_overflow) {
  return n_bad <= bad_cap && key_bytes <= keys_cap && n_fids <= rows_cap && !rows_overflow;
}

}  // namespace vfy
}  // namespace bcw

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace bcw {
namespace vfy {

// One entry k_ix_vfy_select leaves to k_vfy_read: the index value, what names the entry's key in the arena, and the
// position of its fid in the resident set (48 bytes).
struct Item {
  uint64_t fid, off, size;
  uint64_t hash;
  uint64_t kref;  // 1 + arena offset of the key entry (16 B header, then the key)
  uint32_t wal;   // index into the set's device array
  uint32_t key_len;
};
static_assert(sizeof(Item) == 48, "Item layout");

// the call's counters (device words, zeroed by every call on its stream): V_QUEUE work items reserved, V_CLASS + c
// entries of class c, V_RD + s entries of the READ class with rd_status s. The soft-deleted and the invalid (0 < off <
// 40) counts go to the accounting table's auxiliary words, which usage_finish reports.
enum { V_QUEUE = 0, V_CHECKED = 1, V_NBAD = 2, V_KEY_BYTES = 3, V_CLASS = 8, V_RD = 16, V_NUM = 24 };

// what both kernels write besides the accounting table
struct Sink {
  bcw_verify_out out;       // the caller's arrays (device)
  unsigned long long* cnt;  // V_NUM words
  const uint8_t* arena;     // the index's key arena
};

// One bad entry, by one lane: a reservation in the list and in the key bytes (the two totals stay exact whatever the
// caps), a write only inside the caps. The list is whole only when everything had room (vfy::fits), so an entry whose
// key bytes found none is simply not written.
__device__ __forceinline__ void emit_bad(const Sink& S, uint64_t fid, uint64_t off, uint64_t size, uint64_t hash,
                                         uint64_t kref, uint32_t key_len, uint32_t cls, uint32_t rd, uint32_t rec) {
  const uint64_t i = atomicAdd(&S.cnt[V_NBAD], 1ull);
  const uint64_t kp = atomicAdd(&S.cnt[V_KEY_BYTES], (unsigned long long)key_len);
  if (i >= S.out.bad_cap || kp + key_len > S.out.keys_cap) return;
  bcw_verify_bad b;
  b.fid = fid;
  b.off = off;
  b.size = size;
  b.hash = hash;
  b.key_pos = kp;
  b.key_len = key_len;
  b.cls = (uint8_t)cls;
  b.rd_status = (uint8_t)rd;
  b.rec_status = (uint8_t)rec;
  b._pad = 0;
  S.out.bad[i] = b;
  const uint8_t* __restrict__ src = S.arena + (kref - 1) + 16;
  for (uint32_t q = 0; q < key_len; ++q) S.out.keys[kp + q] = src[q];
}

}  // namespace vfy
}  // namespace bcw
#endif  // __HIPCC__
