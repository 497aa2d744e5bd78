// bcw_usage.h -- per-WAL space accounting (bcw_index_fid_usage*, bcw_freed_by_fid_async; bcw.h): the grouped sum of
// rows {fid, counted, bytes, span} by fid that turns the index, or the WriteStat columns of a write, into the numbers
// the compaction picker reads (writeIndex db_impl.go:434-454 -> manifest.Apply manifest.go:505-512 ->
// maybeScheduleCompaction compaction.go:135-150 -> DefaultCompactionPicker db.go:200-224).
//
// Two parts. wal_record_size_closed is a plain inline function compiled by the host, the device and the stand-alone
// host check (tools/usage_check.cpp), as bcw_rules.h is: one text for all three. The rest is the device side of the
// reduction (HIP only): every workgroup of a pass groups its rows in an LDS table and flushes it into one global
// table, and a final one-workgroup kernel (bcw_usage.hip) sorts the occupied slots into the result.
#pragma once
#include <cstdint>

#include "bcw.h"

#if defined(__HIPCC__)
#define BCW_USAGE_FN __host__ __device__ __forceinline__
#else
#define BCW_USAGE_FN inline
#endif

namespace bcw {
namespace usage {

// WalRecordSize (wal.go:61-86) in constant time: the footprint of a `size`-byte payload whose first header is at file
// offset `off` -- the pad that ends a block with fewer than 7 bytes left, the first fragment up to the end of its
// block, whole blocks of 7 + 32761 bytes, and a last partial fragment. rd::wal_record_size (bcw_read_body.h) walks
// one iteration per fragment, size / 32761 of them, and the size an index holds is not trusted (a loaded snapshot, a
// tampered value): the accounting pass never enters that loop. uint64 arithmetic wraps as the reference's does
// (off < 40 included); equal to the loop wherever the loop's own sums do not wrap.
BCW_USAGE_FN uint64_t wal_record_size_closed(uint64_t off, uint64_t size) {
  if (size == 0) return 0;
  const uint64_t kB = BCW_BLOCK_SIZE, kH = BCW_HEADER_SIZE, kData = kB - kH;
  const uint64_t o = off - BCW_SUPER_BLOCK_SIZE;
  uint64_t lo = kB - o % kB;  // bytes left in the block, 1..32768
  uint64_t total = 0;
  if (lo < kH) {  // the writer pads the block's end and starts the record at the next block
    total = lo;
    lo = kB;
  }
  const uint64_t first = size < lo - kH ? size : lo - kH;
  total += kH + first;
  const uint64_t rem = size - first;
  if (rem) {
    total += (rem / kData) * kB;
    if (rem % kData) total += kH + rem % kData;
  }
  return total;
}

}  // namespace usage
}  // namespace bcw

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace bcw {
namespace usage {

// The global table (one per context, zeroed by every call on its stream): kSlots open-addressing slots plus one
// entry, index kSlots, for fid 0. A slot's tag is its fid, and 0 marks an empty slot, so fid 0 never probes: it has
// the extra entry, whose tag word is a presence flag. Every other uint64 is an ordinary tag.
constexpr uint32_t kSlots = 8192;
constexpr uint32_t kEntries = kSlots + 1;
// the three tuning constants can be set on the compile line (A/B builds of the same library, as BCW_CRC_WAVES):
// the values here are the measured choice
#ifndef BCW_USAGE_LDS
#define BCW_USAGE_LDS 512
#endif
#ifndef BCW_USAGE_PROBES
#define BCW_USAGE_PROBES 8
#endif
#ifndef BCW_USAGE_ROUNDS
#define BCW_USAGE_ROUNDS 1
#endif
constexpr uint32_t kLds = BCW_USAGE_LDS;           // slots of a workgroup's LDS table (+ 1 entry for fid 0)
constexpr uint32_t kLdsProbes = BCW_USAGE_PROBES;  // probes into it before a row goes to the global table directly
constexpr uint32_t kRounds = BCW_USAGE_ROUNDS;     // wave-level match-and-reduce rounds before the tables
constexpr uint32_t kLdsBits = kLds == 256 ? 8 : kLds == 512 ? 9 : 10;
static_assert((1u << kLdsBits) == kLds, "the LDS table holds 256, 512 or 1024 slots");
constexpr uint32_t kThreads = 256;    // workgroup size of every pass that uses Accum
// auxiliary words behind the four columns
enum { A_CLAIMED = 0, A_OVERFLOW = 1, A_SOFT = 2, A_INVALID = 3, A_NUM = 8 };
constexpr uint64_t kScratchWords = 4ull * kEntries + A_NUM;

struct Table {  // views into the context's scratch
  unsigned long long* tag;
  unsigned long long* cnt;
  unsigned long long* bytes;
  unsigned long long* span;
  unsigned long long* aux;
};
__host__ __device__ __forceinline__ Table table_of(uint64_t* scratch) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(scratch);
  return Table{p, p + kEntries, p + 2ull * kEntries, p + 3ull * kEntries, p + 4ull * kEntries};
}

__device__ __forceinline__ uint32_t slot_hash(uint64_t fid, uint32_t bits) {
  return (uint32_t)((fid * 0x9E3779B97F4A7C15ull) >> (64u - bits));
}

// one row (already summed over the lanes that share it) into the global table. Bounded: at most kSlots probes, and
// none once the call is known to hold more than BCW_USAGE_MAX_FIDS fids (the result is void then).
__device__ __forceinline__ void global_add(const Table& g, uint64_t fid, uint64_t c, uint64_t b, uint64_t s) {
  uint32_t j = kSlots;
  if (fid == 0) {
    if (g.tag[kSlots] == 0) atomicOr(&g.tag[kSlots], 1ull);
  } else {
    if (__hip_atomic_load(&g.aux[A_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    j = slot_hash(fid, 13);
    uint32_t probe = 0;
    for (; probe < kSlots; ++probe, j = (j + 1) & (kSlots - 1)) {
      unsigned long long t = __hip_atomic_load(&g.tag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == 0) {
        t = atomicCAS(&g.tag[j], 0ull, (unsigned long long)fid);
        if (t == 0) {  // claimed: one more distinct fid (fid 0's entry is not counted here)
          if (atomicAdd(&g.aux[A_CLAIMED], 1ull) + 1 > BCW_USAGE_MAX_FIDS) atomicOr(&g.aux[A_OVERFLOW], 1ull);
          break;
        }
      }
      if (t == fid) break;
    }
    if (probe == kSlots) {  // no slot: only with more than kSlots fids
      atomicOr(&g.aux[A_OVERFLOW], 1ull);
      return;
    }
  }
  if (c) atomicAdd(&g.cnt[j], (unsigned long long)c);
  if (b) atomicAdd(&g.bytes[j], (unsigned long long)b);
  if (s) atomicAdd(&g.span[j], (unsigned long long)s);
}

// A workgroup's accumulator. Use: init() by every thread, add() once per row round by every thread of the workgroup
// (whole waves call it together; a lane without a row passes valid = false), flush() by every thread at the end.
struct Accum {
  unsigned long long tag[kLds + 1], cnt[kLds + 1], bytes[kLds + 1], span[kLds + 1];

  __device__ __forceinline__ void init() {
    for (uint32_t i = threadIdx.x; i < kLds + 1; i += blockDim.x) tag[i] = cnt[i] = bytes[i] = span[i] = 0;
    __syncthreads();
  }

  __device__ __forceinline__ void row(const Table& g, uint64_t fid, uint64_t c, uint64_t b, uint64_t s) {
    uint32_t j = kLds;
    if (fid == 0) {
      tag[kLds] = 1;
    } else {
      j = slot_hash(fid, kLdsBits);
      uint32_t probe = 0;
      for (; probe < kLdsProbes; ++probe, j = (j + 1) & (kLds - 1)) {
        unsigned long long t = tag[j];
        if (t == 0) t = atomicCAS(&tag[j], 0ull, (unsigned long long)fid);  // 64-bit LDS compare-and-swap claim
        if (t == 0 || t == fid) break;
      }
      if (probe == kLdsProbes) {  // this neighbourhood of the table is taken by other fids
        global_add(g, fid, c, b, s);
        return;
      }
    }
    if (c) atomicAdd(&cnt[j], (unsigned long long)c);
    if (b) atomicAdd(&bytes[j], (unsigned long long)b);
    if (s) atomicAdd(&span[j], (unsigned long long)s);
  }

  // kRounds times: the first unserved lane's fid, the lanes that hold it, their sums by one lane; what is left goes
  // lane by lane. One round is what measurement kept: it turns a wave whose rows all share a fid (a
  // database with one WAL file, a write that replaced one file's values) into a single add, and on the 4-fid bench
  // shape every further round cost more in cross-lane traffic than the LDS adds it saved (the pass streams the table
  // at HBM rate with the adds left to the LDS unit).
  __device__ __forceinline__ void add(const Table& g, bool valid, uint64_t fid, bool counted, uint64_t b, uint64_t s) {
    const uint32_t lane = threadIdx.x & 63u;
    bool act = valid, mine = act;  // mine: this lane adds a row (its own, unless a round made it a group's)
    uint64_t rc = counted ? 1 : 0, rb = b, rs = s;
#pragma unroll 1
    for (uint32_t r = 0; r < kRounds; ++r) {
      const uint64_t m = __ballot(act);
      if (m == 0) break;
      const int lead = __ffsll((unsigned long long)m) - 1;
      const uint64_t f = __shfl(fid, lead, 64);
      const bool eq = act && fid == f;
      const uint64_t c = (uint64_t)__popcll(__ballot(eq && counted));
      uint64_t sb = eq ? b : 0, ss = eq ? s : 0;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        sb += __shfl_xor(sb, d, 64);
        ss += __shfl_xor(ss, d, 64);
      }
      if (eq) {  // the group's first lane carries its sums, the others are served
        mine = lane == (uint32_t)lead;
        rc = c;
        rb = sb;
        rs = ss;
      }
      act = act && !eq;
    }
    if (mine) row(g, fid, rc, rb, rs);
  }

  __device__ __forceinline__ void flush(const Table& g) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kLds + 1; i += blockDim.x)
      if (tag[i]) global_add(g, i == kLds ? 0ull : (uint64_t)tag[i], cnt[i], bytes[i], span[i]);
  }
};

}  // namespace usage

// The context's table, allocated on first use and zeroed on `st`; then the rows of the caller's pass go in, and
// usage_finish queues the final kernel: rows ascending by fid into d_rows (cap entries), the result into d_res.
// index_pass: soft_deleted / invalid are reported from the table's auxiliary words (else 0).
int usage_begin(bcw_ctx* c, hipStream_t st, uint64_t** scratch);
int usage_finish(bcw_ctx* c, hipStream_t st, bcw_fid_usage* d_rows, uint32_t cap, bcw_usage_result* d_res,
                 int index_pass);

}  // namespace bcw
#endif  // __HIPCC__
