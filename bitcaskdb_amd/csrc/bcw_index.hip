// bcw_index.hip -- the bitcaskDB index (index.go) resident in HBM, for the two callers of the WAL
// codec that consult it: the compaction filter (doFilter, compaction.go:329-348) and
// the index rebuild from hint / data WALs (recoverFromWal db_impl.go:286-313, onePhase
// compaction.go:248-251; §8 f2).
//
// What is restated is the index's observable behaviour (index.go:81-165 over map.go's ShardMap): a map
// from MergedKey(ns, key) = ns || key (utils.go:133-139) to IndexValue{fid, valueOff, valueSize}, keyed by
// IndexOperator.Hash = murmur3 Sum64 (index.go:15-19, spaolacci/murmur3 v1.1.0); Put replaces, Delete
// removes, SoftDelete stores {0, 0, 0}, Get reports ErrKeyNotFound / ErrKeySoftDeleted (valueOff == 0).
// Bucket placement is unobservable; the reference's sampled approximate-LRU eviction (random slots,
// map.go:395-420) is not restated -- the device index holds every key (capacity grows instead).
//
// Layout (HBM): an open-addressing slot table (64 B slots, power-of-two capacity, linear probing from
// the hash) and a key arena of {hash, length, key bytes padded to 16} entries. Between rebuilds both only fill
// up: a removed key (Delete, or an eviction by the capacity bound) leaves a dead slot and a dead arena entry, and
// a live-only rebuild (k_ix_compact: off the batch path, run by the host when half the claimed slots are dead, or
// on request, bcw_index_compact) gives both back.
// A batch of operations (host-supplied, or every delivered row of a decoded record / hint table) runs
// as five stream-ordered launches, so every cross-workgroup hand-off is a kernel boundary:
//   k_ix_keys   one lane per op: murmur3 over the merged key's 16 B chunks (gathered from the WAL segment
//               when the ops come from a decoded table)
//   k_ix_claim  probe from the hash: find the slot holding the key (arena compare), or claim an empty
//               slot with a 64-bit CAS of a provisional reference to the op itself (ops of the batch
//               compare their keys straight from the source); an op that finds its key records the
//               value it replaces (WriteStat)
//   k_ix_seq    atomicMax of the op's sequence number into its slot: the last op of a key wins, as
//               in the reference's sequential loop
//   k_ix_commit the op that claimed a slot copies its key into the arena and makes the slot's reference
//               permanent: only keys new to the index take arena space (a rebuild over existing keys
//               takes none)
//   k_ix_write  the winning op writes the value / presence
// Lookups (Get, the compaction filter) are one launch: hash, probe, compare.
// The passes over the whole slot table (usage, drop, the scrub's select, the scan by key prefix) share one coalesced,
// LDS-staged round of 256 slots (usage_round).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "bcw_crc_dev.h"
#include "bcw_drop.h"
#include "bcw_host.h"
#include "bcw_murmur.h"
#include "bcw_read_body.h"
#include "bcw_rules.h"
#include "bcw_scan.h"
#include "bcw_usage.h"
#include "bcw_verify.h"

namespace bcw {
namespace ix {

struct Slot {
  uint64_t kref;  // 0: empty; 1 + arena offset of the key entry; kProv | op: claimed by op of the running batch
  uint64_t seq;   // sequence number of the last op applied to this key
  uint64_t hash;  // murmur3 Sum64 of the merged key
  uint64_t fid, off, size;
  uint64_t live;  // 1: present (Put, SoftDelete); 0: absent (Delete)
  uint64_t pad;   // 0 between batches; inside a write batch the head of the key's op list (k_put_link)
};
static_assert(sizeof(Slot) == 64, "Slot layout");

constexpr uint64_t kProv = 1ull << 63;  // provisional slot reference (claim -> commit inside one batch)

// device counters (C_NEED: arena bytes the rows of a decoded table would take, k_ix_need)
// C_EVICTED / C_EVICTED_BYTES: keys evicted by the capacity bound (k_ix_evict) and the sum of their value sizes
// C_R_*: the counters of a live-only rebuild in progress (k_ix_compact): arena bytes and slots of the new table,
// and its failure flag; k_ix_adopt makes them the index's once the rebuild is known to be whole
enum { C_ARENA = 0, C_SLOTS = 1, C_LIVE = 2, C_OVERFLOW = 3, C_NIN = 4, C_DONE = 5, C_FAIL = 6, C_NEED = 7,
       C_EVICTED = 8, C_EVICTED_BYTES = 9, C_R_ARENA = 10, C_R_SLOTS = 11, C_R_FAIL = 12, C_NUM = 13 };
// a call's own counters C_NIN .. C_FAIL and a rebuild's C_R_ARENA .. C_R_FAIL are each zeroed at once (zero_group)
static_assert(C_DONE == C_NIN + 1 && C_FAIL == C_NIN + 2, "C_NIN, C_DONE, C_FAIL are adjacent");
static_assert(C_R_SLOTS == C_R_ARENA + 1 && C_R_FAIL == C_R_ARENA + 2, "C_R_ARENA, C_R_SLOTS, C_R_FAIL are adjacent");

// op sources
// SRC_BATCH: a write batch (bcw_write_records*): flat merged keys as SRC_FLAT, but the number of ops is read from a
// device word (as the table kinds read cnt[C_NIN]), the op comes from the record's BCW_WR_* flags and the Put value
// from the device rec_off / rec_size columns the writer produced
enum { SRC_FLAT = 0, SRC_RECORD = 1, SRC_HINT = 2, SRC_BATCH = 3 };

struct Src {
  int kind;
  // flat: merged keys concatenated, key i = keys[koff[i], koff[i+1])
  const uint8_t* keys;
  const uint64_t* koff;
  uint64_t keys_len;
  uint64_t kbias;  // added to every key offset (SRC_BATCH: `keys` is the array's address rounded down to 16 bytes)
  // write batch
  const uint64_t* b_nin;  // device word: ops to apply (0: the batch was rejected)
  const uint64_t* b_off;
  const uint64_t* b_size;
  const uint8_t* b_flags;
  uint64_t b_fid;
  // decoded table: the segment, its fragment table and record table
  const uint8_t* seg;
  uint64_t seg_len;
  const Frag* frags;
  bcw_record_table t;
  uint32_t start_off, ns;
};

__device__ __forceinline__ bool flat_keys(const Src& s) { return s.kind == SRC_FLAT || s.kind == SRC_BATCH; }

// 16 bytes of buf at signed offset a; bytes outside [0, n) read as 0
__device__ __forceinline__ uint4 load16u(const uint8_t* __restrict__ buf, uint64_t n, int64_t a) {
  if (a >= 0 && (uint64_t)(a & ~15ll) + 32 <= n) {
    const uint8_t* p = buf + (a & ~15ll);
    return shift16(*reinterpret_cast<const uint4*>(p), *reinterpret_cast<const uint4*>(p + 16), (uint32_t)(a & 15));
  }
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int i = 0; i < 16; ++i) {
    const int64_t q = a + i;
    const uint32_t by = (q >= 0 && (uint64_t)q < n) ? buf[q] : 0u;
    w[i >> 2] |= by << (8 * (i & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// bytes [lo, hi) of a 16 B unit
__device__ __forceinline__ uint4 keep_bytes(uint4 v, int32_t lo, int32_t hi) {
  const uint4 m = range_mask(lo, hi);
  return make_uint4(v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w);
}
__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }

// One op's merged key: up to two byte ranges (ns, key) of a flat buffer or of a record payload.
struct Key {
  uint32_t la, lb;   // range lengths (merged key = A || B)
  int64_t a0, b0;    // start of A / B: flat -> buffer offset; payload -> file offset when contiguous
  bool ca, cb;       // the range is contiguous in the buffer (always, for flat keys)
  uint32_t pa, pb;   // payload offsets of A / B (slow path)
  uint32_t f0, f1;   // the payload's fragments
  bool ok;           // false: the row is not a delivered OK record (no key)
  __device__ __forceinline__ uint32_t len() const { return la + lb; }
};

// payload offset z of a record whose bytes are the data of fragments [f0, f1]
__device__ uint8_t payload_byte(const Src& s, uint32_t f0, uint32_t f1, uint64_t z) {
  uint32_t f = f0;
  for (;;) {
    const Frag F = s.frags[f];
    if (z < F.len || f >= f1) {
      const uint64_t a = (uint64_t)s.start_off + (uint64_t)F.blk * kBlock + F.start + z;
      return a < s.seg_len ? s.seg[a] : 0;
    }
    z -= F.len;
    ++f;
  }
}

__device__ __forceinline__ Key make_key(const Src& s, uint64_t i) {
  Key k{};
  k.ok = true;
  if (flat_keys(s)) {
    const uint64_t a = s.koff[i] + s.kbias, b = s.koff[i + 1] + s.kbias;
    k.la = (uint32_t)(b - a);
    k.lb = 0;
    k.a0 = (int64_t)a;
    k.b0 = (int64_t)b;
    k.ca = k.cb = true;
    return k;
  }
  const bcw_record_table& t = s.t;
  k.f1 = t.emit_frag[i];
  k.f0 = t.first_frag[i];
  const Frag F0 = s.frags[k.f0];
  const Frag F1 = s.frags[k.f1];
  if (F1.type == BCW_RECORD_FULL) k.f0 = k.f1;  // a Full emission carries only its own data
  const Frag Fa = k.f0 == k.f1 ? F1 : F0;
  const uint64_t d0 = (uint64_t)s.start_off + (uint64_t)Fa.blk * kBlock + Fa.start;
  const uint32_t l0 = Fa.len;
  k.la = s.ns;
  k.pa = s.kind == SRC_RECORD ? 1u : 0u;  // RecordFromBytes: data[1:1+NsSize]; HintRecord: data[0:NsSize]
  k.lb = t.key_len[i];
  k.pb = t.hdr_size[i];                   // record: headerSize (key offset); hint: key offset mod 256
  if (s.kind == SRC_HINT && s.ns > 245u) {
    // the hint key offset NsSize + len(uvarint keyLen) (hint.go:62-66) no longer fits the table's u8 column:
    // count the varint's bytes in the payload (HintRecord.Decode accepted it, so it ends within 10 bytes)
    uint32_t u = 1;
    while (u < 10u && (payload_byte(s, k.f0, k.f1, (uint64_t)s.ns + u - 1) & 0x80u)) ++u;
    k.pb = s.ns + u;
  }
  k.ca = (uint64_t)k.pa + k.la <= l0;
  k.cb = (uint64_t)k.pb + k.lb <= l0;
  k.a0 = (int64_t)(d0 + k.pa);
  k.b0 = (int64_t)(d0 + k.pb);
  return k;
}

// chunk c (merged bytes [16c, 16c + 16), zero beyond the key) of op i's key
__device__ __forceinline__ uint4 key_chunk(const Src& s, const Key& k, uint32_t c) {
  const int32_t m0 = (int32_t)(16 * c);
  const int32_t L = (int32_t)k.len();
  uint4 v = make_uint4(0, 0, 0, 0);
  const uint8_t* buf = flat_keys(s) ? s.keys : s.seg;
  const uint64_t n = flat_keys(s) ? s.keys_len : s.seg_len;
  if (m0 < (int32_t)k.la) {  // part of A: merged [m0, min(la, m0 + 16))
    const int32_t hi = min((int32_t)k.la - m0, 16);
    if (k.ca) {
      v = keep_bytes(load16u(buf, n, k.a0 + m0), 0, hi);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (int32_t b = 0; b < hi; ++b)
        w[b >> 2] |= (uint32_t)payload_byte(s, k.f0, k.f1, k.pa + (uint64_t)(m0 + b)) << (8 * (b & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  if (m0 + 16 > (int32_t)k.la && m0 < L) {  // part of B: merged [max(la, m0), min(L, m0 + 16))
    const int32_t lo = max((int32_t)k.la - m0, 0), hi = min(L - m0, 16);
    if (k.cb) {
      v = or4(v, keep_bytes(load16u(buf, n, k.b0 + (m0 - (int32_t)k.la)), lo, hi));
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (int32_t b = lo; b < hi; ++b)
        w[b >> 2] |= (uint32_t)payload_byte(s, k.f0, k.f1, k.pb + (uint64_t)(m0 + b - (int32_t)k.la)) << (8 * (b & 3));
      v = or4(v, make_uint4(w[0], w[1], w[2], w[3]));
    }
  }
  return v;
}

__device__ __forceinline__ uint64_t key_hash(const Src& s, const Key& k) {
  murmur::State m;  // fed 16-byte blocks
  const uint32_t L = k.len(), nb = L / 16, t = L & 15u;
  for (uint32_t c = 0; c < nb; ++c) {
    const uint4 v = key_chunk(s, k, c);
    m.block((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32));
  }
  uint4 v = make_uint4(0, 0, 0, 0);
  if (t) v = key_chunk(s, k, nb);
  return m.finish((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32), t, L);
}

// rows of a decoded table that IterateRecord / IterateHint deliver to the callback: those before the
// first row RecordFromBytes / HintRecord.Decode rejects (record.go:246-263, hint.go:174-185)
__device__ __forceinline__ uint64_t delivered_rows(const bcw_decode_result* R) {
  const uint64_t nrec = R->n_records;
  return (R->first_bad_record >= 0 && (uint64_t)R->first_bad_record < nrec) ? (uint64_t)R->first_bad_record : nrec;
}

// the table source is usable: the context's latest decode (its fragment table), not truncated, and not a decode
// that gave up on an internal wait (BCW_ERR_INTERNAL: its rows, if any, are not to be applied)
__device__ __forceinline__ uint32_t table_fail(const bcw_decode_result* R, uint64_t gen, uint64_t rows) {
  return R->generation != gen ? BCW_ENC_ERR_STALE
         : (R->n_records > rows || R->err_class == BCW_ERR_INTERNAL) ? BCW_ENC_ERR_TABLE : 0u;
}

// An arena entry is a 16 B header {hash, key length, 0} and the key padded to 16 B (k_ix_commit lays it out):
// the length word of the entry a slot's kref names, and the bytes an entry of a len-byte key takes
__device__ __forceinline__ uint32_t entry_len(const uint8_t* __restrict__ arena, uint64_t kref) {
  return *reinterpret_cast<const uint32_t*>(arena + (kref - 1) + 8);
}
__device__ __forceinline__ uint64_t entry_bytes(uint64_t len) { return 16ull + ((len + 15) & ~15ull); }

// ---- batch launch 1: key hashes ----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ix_keys(Src s, uint64_t n, const bcw_decode_result* __restrict__ R,
                                                 uint64_t gen, uint64_t* __restrict__ cnt,
                                                 uint64_t* __restrict__ op_kref, uint64_t* __restrict__ op_hash) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  uint64_t nin = n;
  if (s.kind == SRC_BATCH) {
    nin = *s.b_nin < n ? *s.b_nin : n;
    if (i == 0) { cnt[C_NIN] = nin; cnt[C_FAIL] = 0; }
  } else if (s.kind != SRC_FLAT) {
    const uint32_t fail = table_fail(R, gen, n);
    nin = fail ? 0 : delivered_rows(R);
    if (i == 0) { cnt[C_NIN] = nin; cnt[C_FAIL] = fail; }
  }
  if (i >= nin) return;
  const Key k = make_key(s, i);
  op_hash[i] = key_hash(s, k);
  op_kref[i] = kProv | i;  // the op's own provisional reference (its key is read from the source)
}

// the arena entry at offset a holds op k's key (length L)
__device__ __forceinline__ bool arena_matches(const Src& s, const Key& k, const uint8_t* __restrict__ arena,
                                              uint64_t a, uint32_t L) {
  const uint4* q = reinterpret_cast<const uint4*>(arena + a + 16);
  for (uint32_t c = 0; c < (L + 15) / 16; ++c) {
    const uint4 x = key_chunk(s, k, c), y = q[c];
    if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) return false;
  }
  return true;
}
// ops k and kj of the batch have the same key (lengths equal)
__device__ __forceinline__ bool keys_match(const Src& s, const Key& k, const Key& kj, uint32_t L) {
  for (uint32_t c = 0; c < (L + 15) / 16; ++c) {
    const uint4 x = key_chunk(s, k, c), y = key_chunk(s, kj, c);
    if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) return false;
  }
  return true;
}

// ---- batch launch 2: find or claim each op's slot --------------------------------------------------
// old_*: per op, the value the slot held before the batch when the key existed (WriteStat of the key's first
// op in the batch; the host composes the later ones, bcw_index_apply_stat)
__global__ __launch_bounds__(256) void k_ix_claim(Src s, uint64_t n, const uint64_t* __restrict__ cnt_in,
                                                  Slot* __restrict__ slots, uint64_t mask,
                                                  const uint8_t* __restrict__ arena, uint64_t* __restrict__ cnt,
                                                  const uint64_t* __restrict__ op_kref,
                                                  const uint64_t* __restrict__ op_hash, uint64_t* __restrict__ op_slot,
                                                  uint8_t* __restrict__ old_found, uint64_t* __restrict__ old_fid,
                                                  uint64_t* __restrict__ old_size) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t nin = s.kind == SRC_FLAT ? n : cnt_in[C_NIN];
  bool claimed = false;
  if (i < nin) {
    uint64_t slot = ~0ull;
    uint8_t found = 0;
    uint64_t ofid = 0, osize = 0;
    if (op_kref[i]) {
      const uint64_t h = op_hash[i];
      const Key k = make_key(s, i);
      const uint32_t L = k.len();
      uint64_t j = h & mask;
      for (uint64_t probe = 0; probe <= mask; ++probe, j = (j + 1) & mask) {
        uint64_t c = __hip_atomic_load(&slots[j].kref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) {
          c = atomicCAS(reinterpret_cast<unsigned long long*>(&slots[j].kref), 0ull, (unsigned long long)(kProv | i));
          if (c == 0) { slot = j; claimed = true; break; }
        }
        if (c & kProv) {  // claimed by another op of this batch: compare with its key at the source
          const uint64_t o = c & ~kProv;
          if (op_hash[o] != h) continue;
          const Key ko = make_key(s, o);
          if (ko.len() == L && keys_match(s, k, ko, L)) { slot = j; break; }
        } else {
          const uint4 hd = *reinterpret_cast<const uint4*>(arena + (c - 1));
          if (((uint64_t)hd.x | ((uint64_t)hd.y << 32)) == h && hd.z == L && arena_matches(s, k, arena, c - 1, L)) {
            slot = j;
            const Slot S = slots[j];  // values are only written by k_ix_write, after this launch
            if (S.live) { found = 1; ofid = S.fid; osize = S.size; }
            break;
          }
        }
      }
      if (slot == ~0ull) atomicOr(reinterpret_cast<unsigned long long*>(&cnt[C_OVERFLOW]), 2ull);
    }
    op_slot[i] = slot;
    if (old_found) { old_found[i] = found; old_fid[i] = ofid; old_size[i] = osize; }
  }
  (void)wave_alloc(&cnt[C_SLOTS], claimed ? 1ull : 0ull);
}

// ---- batch launch 3: the last op of each key wins ----------------------------------------------------
__global__ __launch_bounds__(256) void k_ix_seq(uint64_t n, const uint64_t* __restrict__ cnt_in, int flat,
                                                Slot* __restrict__ slots, const uint64_t* __restrict__ op_slot,
                                                uint64_t seq_base) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t nin = flat ? n : cnt_in[C_NIN];
  if (i >= nin) return;
  const uint64_t s = op_slot[i];
  if (s == ~0ull) return;
  atomicMax(reinterpret_cast<unsigned long long*>(&slots[s].seq), (unsigned long long)(seq_base + i));
}

// ---- batch launch 4: the claiming op copies its key into the arena ------------------------------------
__global__ __launch_bounds__(256) void k_ix_commit(Src s, uint64_t n, uint64_t* __restrict__ cnt,
                                                   Slot* __restrict__ slots, uint8_t* __restrict__ arena,
                                                   uint64_t arena_cap, const uint64_t* __restrict__ op_hash,
                                                   const uint64_t* __restrict__ op_slot) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t nin = s.kind == SRC_FLAT ? n : cnt[C_NIN];
  bool own = false;
  uint64_t sl = ~0ull;
  Key k{};
  if (i < nin) {
    sl = op_slot[i];
    own = sl != ~0ull && slots[sl].kref == (kProv | i);
    if (own) k = make_key(s, i);
  }
  const uint64_t esz = own ? entry_bytes(k.len()) : 0;
  const uint64_t a = wave_alloc(&cnt[C_ARENA], esz);
  if (!own) return;
  if (a + esz > arena_cap) {  // the host sizes the arena before the launch; never expected
    atomicOr(reinterpret_cast<unsigned long long*>(&cnt[C_OVERFLOW]), 1ull);
    slots[sl].kref = 0;
    return;
  }
  uint8_t* e = arena + a;
  const uint32_t L = k.len();
  for (uint32_t c = 0; c < (L + 15) / 16; ++c) *reinterpret_cast<uint4*>(e + 16 + 16 * c) = key_chunk(s, k, c);
  const uint64_t h = op_hash[i];
  *reinterpret_cast<uint4*>(e) = make_uint4((uint32_t)h, (uint32_t)(h >> 32), L, 0u);
  slots[sl].hash = h;
  slots[sl].kref = a + 1;
}

// arena bytes the delivered rows of a decoded table would take if every key were new (the exact bound the
// host reads when its cheap bound does not fit the arena)
__global__ __launch_bounds__(256) void k_ix_need(Src s, uint64_t rows, const bcw_decode_result* __restrict__ R,
                                                 uint64_t gen, uint64_t* __restrict__ cnt) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t nin = table_fail(R, gen, rows) ? 0 : delivered_rows(R);
  uint64_t b = 0;
  if (i < nin) b = entry_bytes((uint64_t)s.ns + s.t.key_len[i]);
  (void)wave_alloc(&cnt[C_NEED], b);
}

// ---- batch launch 5: values ---------------------------------------------------------------------------
struct OpVals {
  // flat ops (host arrays copied to the device): op code and value per op
  const uint8_t* op;
  const uint64_t* fid;
  const uint64_t* off;
  const uint64_t* size;
  // table ops: value columns (PUT of every delivered row)
  uint64_t file_fid;
  int use_rec_fid;
};

// the op of record i of a write batch, from its BCW_WR_* flags (db_impl.go:441-448)
__device__ __forceinline__ uint32_t batch_op(const Src& s, uint64_t i) {
  const uint32_t fl = s.b_flags[i];
  return (fl & BCW_WR_DELETED) ? BCW_IDX_DELETE : (fl & BCW_WR_TOMBSTONE) ? BCW_IDX_SOFT_DELETE : BCW_IDX_PUT;
}

__global__ __launch_bounds__(256) void k_ix_write(Src s, uint64_t n, uint64_t* __restrict__ cnt, OpVals v,
                                                  Slot* __restrict__ slots, const uint64_t* __restrict__ op_slot,
                                                  uint64_t seq_base) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const bool flat = s.kind == SRC_FLAT;
  const uint64_t nin = flat ? n : cnt[C_NIN];
  int64_t dlive = 0;
  uint64_t done = 0;
  if (i < nin) {
    const uint64_t sl = op_slot[i];
    if (sl != ~0ull &&
        __hip_atomic_load(&slots[sl].seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq_base + i) {
      Slot& S = slots[sl];
      uint32_t op = BCW_IDX_PUT;
      uint64_t fid = 0, off = 0, size = 0;
      if (flat) {
        op = v.op[i];
        fid = v.fid[i];
        off = v.off[i];
        size = v.size[i];
      } else if (s.kind == SRC_BATCH) {      // db_impl.go:441-448
        op = batch_op(s, i);
        fid = s.b_fid;
        off = s.b_off[i];
        size = s.b_size[i];
      } else if (s.kind == SRC_RECORD) {
        fid = v.file_fid;                       // db_impl.go:307-313: Put(ns, key, wal.Fid(), foff - 7, size)
        off = s.t.foff[i] - kHdr;
        size = s.t.size[i];
      } else {
        fid = v.use_rec_fid ? s.t.expire[i] : v.file_fid;  // compaction.go:250 (record.fid) / db_impl.go:297 (fid)
        off = s.t.aux0[i];
        size = s.t.aux1[i];
      }
      const uint64_t was = S.live;
      if (op == BCW_IDX_DELETE) {
        S.live = 0;
      } else {
        if (op == BCW_IDX_SOFT_DELETE) fid = off = size = 0;  // IndexValue{valueOff: 0} (index.go:128-130)
        S.fid = fid;
        S.off = off;
        S.size = size;
        S.live = 1;
      }
      dlive = (int64_t)S.live - (int64_t)was;
    }
    done = 1;
  }
  (void)wave_alloc(&cnt[C_LIVE], (uint64_t)dlive);
  (void)wave_alloc(&cnt[C_DONE], done);
}

// ---- WriteStat of a write batch, composed on the device -----------------------------------------------
// k_ix_claim reported, per op, the value the key held before the batch. An op preceded by another op on the same key
// in this batch replaces that op's value instead (Put: the batch's fid and its size, SoftDelete: IndexValue{} with
// fid 0 / size 0, Delete: nothing -- index.go:108-165; the host composition of bcw_index_apply_stat, here without a
// round trip). The ops of one key are those of one slot: k_put_link chains them through the slot's spare word (an
// unordered list: link[i] = the previous head), k_put_stat walks its key's list for the latest op before its own (the
// list is as long as the key's ops in this batch), k_put_unlink clears the word again.
__global__ __launch_bounds__(256) void k_put_link(const uint64_t* __restrict__ cnt, Slot* __restrict__ slots,
                                                  const uint64_t* __restrict__ op_slot, uint64_t* __restrict__ link) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= cnt[C_NIN]) return;
  const uint64_t sl = op_slot[i];
  link[i] = sl == ~0ull ? 0 : atomicExch(reinterpret_cast<unsigned long long*>(&slots[sl].pad), (unsigned long long)(i + 1));
}
__global__ __launch_bounds__(256) void k_put_stat(Src s, const uint64_t* __restrict__ cnt, const Slot* __restrict__ slots,
                                                  const uint64_t* __restrict__ op_slot, const uint64_t* __restrict__ link,
                                                  uint8_t* __restrict__ found, uint64_t* __restrict__ free_fid,
                                                  uint64_t* __restrict__ free_bytes) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= cnt[C_NIN]) return;
  const uint64_t sl = op_slot[i];
  uint64_t best = 0;  // 1 + the latest earlier op on this key
  if (sl != ~0ull)
    for (uint64_t p = slots[sl].pad; p != 0; p = link[p - 1])
      if (p - 1 < i && p > best) best = p;
  uint32_t f = found[i];
  uint64_t ff = free_fid[i], fb = free_bytes[i];
  if (best) {
    const uint32_t op = batch_op(s, best - 1);
    f = op != BCW_IDX_DELETE;
    ff = op == BCW_IDX_PUT ? s.b_fid : 0;
    fb = op == BCW_IDX_PUT ? s.b_size[best - 1] : 0;
  }
  if (!f) ff = fb = 0;
  found[i] = (uint8_t)f;
  free_fid[i] = ff;
  free_bytes[i] = fb;
}
__global__ __launch_bounds__(256) void k_put_unlink(const uint64_t* __restrict__ cnt, Slot* __restrict__ slots,
                                                    const uint64_t* __restrict__ op_slot) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= cnt[C_NIN]) return;
  const uint64_t sl = op_slot[i];
  if (sl != ~0ull) slots[sl].pad = 0;
}
__global__ void k_put_idx_err(const uint64_t* __restrict__ cnt, int32_t* __restrict__ idx_err) {
  *idx_err = cnt[C_OVERFLOW] ? BCW_IDX_ERR_FULL : 0;
}

// ---- lookups -----------------------------------------------------------------------------------------
// hash, probe, compare: the slot holding key k, or ~0. A lookup (Index.Get, index.go:81-98) is this and the slot's
// `live`; its callers spell that test out, because a helper that returns "found" made their kernels longer.
__device__ __forceinline__ uint64_t find_slot(const Src& s, const Key& k, const Slot* __restrict__ slots,
                                              uint64_t mask, const uint8_t* __restrict__ arena) {
  const uint64_t h = key_hash(s, k);
  const uint32_t L = k.len();
  uint64_t j = h & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe, j = (j + 1) & mask) {
    const uint64_t kr = slots[j].kref;
    if (kr == 0) return ~0ull;
    if (slots[j].hash != h) continue;
    const uint4 hd = *reinterpret_cast<const uint4*>(arena + (kr - 1));
    if (hd.z != L) continue;
    // arena_matches' compare, written out: calling it here was tried and made every lookup kernel's body longer
    const uint4* q = reinterpret_cast<const uint4*>(arena + (kr - 1) + 16);
    bool eq = true;
    for (uint32_t c = 0; c < (L + 15) / 16 && eq; ++c) {
      const uint4 x = key_chunk(s, k, c), y = q[c];
      eq = x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
    }
    if (eq) return j;
  }
  return ~0ull;
}

// Index.Get (index.go:81-98) of flat keys
__global__ __launch_bounds__(256) void k_ix_get(Src s, uint64_t n, const Slot* __restrict__ slots, uint64_t mask,
                                                const uint8_t* __restrict__ arena, uint64_t* __restrict__ fid,
                                                uint64_t* __restrict__ off, uint64_t* __restrict__ size,
                                                uint8_t* __restrict__ status) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= n) return;
  const Key k = make_key(s, i);
  const uint64_t j = find_slot(s, k, slots, mask, arena);
  uint8_t st = BCW_IDX_NOT_FOUND;
  uint64_t f = 0, o = 0, z = 0;
  if (j != ~0ull && slots[j].live) {
    f = slots[j].fid;
    o = slots[j].off;
    z = slots[j].size;
    st = o == 0 ? BCW_IDX_SOFT_DELETED : BCW_IDX_FOUND;
  }
  fid[i] = f;
  off[i] = o;
  size[i] = z;
  status[i] = st;
}

// getWalRef (db_impl.go:589-593) and ReadRecord's span check (wal.go:562-564) of an index value (f, o, z), the one
// text k_get_lookup and k_ix_vfy_select compile: the position of f in the resident set (ascending fid; n_wals: not
// resident) and, when it is resident, *beyond. The value is not trusted: vfy::span_untrusted (bcw_verify.h) comes
// before WalRecordSize's loop, which then runs at most seg_len / 32761 rounds and whose sum cannot wrap.
__device__ __forceinline__ uint32_t wal_span(const WalEnt* __restrict__ wals, uint32_t n_wals, uint64_t f, uint64_t o,
                                             uint64_t z, bool* beyond) {
  uint32_t lo = 0, hi = n_wals;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (wals[m].fid < f) lo = m + 1; else hi = m;
  }
  *beyond = false;
  if (lo >= n_wals || wals[lo].fid != f) return n_wals;
  const uint64_t len = wals[lo].seg_len;
  bool b = vfy::span_untrusted(o, z, len);
  if (!b) b = vfy::span_beyond(o, rd::wal_record_size(o, z), len);  // no wrap: both terms are O(seg_len)
  *beyond = b;
  return lo;
}

// The lookup of a batched Get (DBImpl.Get, db_impl.go:567-577), one lane per flat key as k_ix_get: Index.Get, then
// getWalRef -- the value's fid in the resident set, a binary search -- then ReadRecord's span check off +
// WalRecordSize(off, size) > seg_len (wal.go:562-564). size comes out of the index and is not trusted: size > seg_len
// or an off outside [40, seg_len] is BEYOND before WalRecordSize's loop (size / 32761 rounds) is entered. A request
// that will be read takes a payload slot of size rounded up to 16 bytes; the slot sizes go to out.pay_off and their
// sum per workgroup to bsum (bfound: keys found) for the scan that lays the slots out in request order.
__global__ __launch_bounds__(kGetLookupKeys) void k_get_lookup(Src s, GetLookup g, const Slot* __restrict__ slots,
                                                               uint64_t mask, const uint8_t* __restrict__ arena) {
  __shared__ uint64_t s_sum[kGetLookupKeys / 64], s_found[kGetLookupKeys / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kGetLookupKeys + threadIdx.x;
  uint64_t slot = 0, found = 0;
  if (i < g.n) {
    s.keys_len = s.koff[g.n];
    const Key k = make_key(s, i);
    const uint64_t j = find_slot(s, k, slots, mask, arena);
    uint8_t gs = BCW_GET_NOT_FOUND, rs = BCW_RD_OK;
    uint64_t f = 0, o = 0, z = 0;
    if (j != ~0ull && slots[j].live) {
      found = 1;
      f = slots[j].fid;
      o = slots[j].off;
      z = slots[j].size;
      if (o == 0) {
        gs = BCW_GET_SOFT_DELETED;
      } else {
        bool beyond;
        if (wal_span(g.wals, g.n_wals, f, o, z, &beyond) >= g.n_wals) {
          gs = BCW_GET_NO_WAL;
        } else if (beyond) {
          gs = BCW_GET_READ;
          rs = BCW_RD_BEYOND;
        } else {
          gs = BCW_GET_OK;  // so far: k_get_read decides
          slot = (z + 15) & ~15ull;
        }
      }
    }
    g.out.get_status[i] = gs;
    g.out.rd_status[i] = rs;
    g.out.fid[i] = f;
    g.out.off[i] = o;
    g.out.size[i] = z;
    g.out.pay_off[i] = slot;
  }
  uint64_t sum = slot, nf = found;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {  // two wave_sums, interleaved: one after the other waits twice as often
    sum += __shfl_xor(sum, d, 64);
    nf += __shfl_xor(nf, d, 64);
  }
  if ((threadIdx.x & 63u) == 0) { s_sum[threadIdx.x >> 6] = sum; s_found[threadIdx.x >> 6] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0, b = 0;
    for (int w = 0; w < kGetLookupKeys / 64; ++w) { a += s_sum[w]; b += s_found[w]; }
    g.bsum[blockIdx.x] = a;
    g.bfound[blockIdx.x] = b;
  }
}

// compactOneWal's doFilter (compaction.go:329-348, without the user CompactionFilter) of every delivered
// row of a decoded data WAL: keep = Get succeeds (not deleted / soft-deleted) and still points at
// (src fid, foff - 7) (compaction.go:302); rows the iteration does not deliver get 0
//
// With the index's compaction filter rules (bcw_index_set_compact_rules, bcw_rules.h; kRules): the same index
// check first, then, only for a row that is still kept, the rules in their order -- the two column rules from the
// table's expire / flags, the prefix rule over the merged key's first 16 B chunks (key_chunk, as the lookup reads
// them: a namespace or key that straddles fragments takes its slow path) against the prefix table pt, which the
// workgroup has staged into LDS. A row counts for the first rule that matches it (one wave-aggregated add per rule and
// wave). One text, two kernels: k_ix_filter compiles none of the rules, k_ix_filter_rules is launched only when rules
// are set.
struct Rules {
  uint32_t mask, n_prefix, longest;  // n_prefix: 0 unless BCW_RULE_PREFIX is set
  uint64_t now;
  const rules::PrefixTable* table;   // device
  uint64_t* cnt;                     // device: rows dropped by {expired, tombstone, prefix}
};

template <bool kRules>
__device__ __forceinline__ void filter_rows(const Src& s, uint64_t rows, const bcw_decode_result* __restrict__ R,
                                            uint64_t gen, const Slot* __restrict__ slots, uint64_t mask,
                                            const uint8_t* __restrict__ arena, uint64_t src_fid,
                                            uint8_t* __restrict__ keep, uint64_t* __restrict__ cnt, const Rules& ru,
                                            const rules::PrefixTable* pt) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint32_t fail = table_fail(R, gen, rows);
  const uint64_t nin = fail ? 0 : delivered_rows(R);
  if (i == 0) { cnt[C_NIN] = nin; cnt[C_FAIL] = fail; }
  uint8_t kp = 0;
  uint32_t hit = rules::kNone;
  if (i < nin) {
    const Key k = make_key(s, i);
    const uint64_t j = find_slot(s, k, slots, mask, arena);
    if (j != ~0ull && slots[j].live && slots[j].off != 0)
      kp = (slots[j].fid == src_fid && slots[j].off == s.t.foff[i] - kHdr) ? 1 : 0;
    if constexpr (kRules) {
      if (kp) {
        hit = rules::first_match(ru.mask, ru.now, s.t.expire[i], s.t.flags[i], k.len(), pt->w, pt->len, ru.n_prefix,
                                 ru.longest, [&](uint32_t* kw, uint32_t n) {
#pragma unroll
                                   for (uint32_t c = 0; c < rules::kKeyChunks; ++c) {
                                     if (c >= n) break;
                                     const uint4 x = key_chunk(s, k, c);
                                     kw[4 * c] = x.x;
                                     kw[4 * c + 1] = x.y;
                                     kw[4 * c + 2] = x.z;
                                     kw[4 * c + 3] = x.w;
                                   }
                                 });
        if (hit != rules::kNone) kp = 0;
      }
    }
  }
  if (i < rows) keep[i] = kp;
  (void)wave_alloc(&cnt[C_DONE], kp ? 1ull : 0ull);
  if constexpr (kRules) {
#pragma unroll
    for (uint32_t r = rules::kExpired; r <= rules::kPrefix; ++r) {
      const uint64_t b = __ballot(hit == r);
      if ((threadIdx.x & 63u) == 0 && b)
        atomicAdd(reinterpret_cast<unsigned long long*>(&ru.cnt[r - 1]), (unsigned long long)__popcll(b));
    }
  }
}

__global__ __launch_bounds__(256) void k_ix_filter(Src s, uint64_t rows, const bcw_decode_result* __restrict__ R,
                                                   uint64_t gen, const Slot* __restrict__ slots, uint64_t mask,
                                                   const uint8_t* __restrict__ arena, uint64_t src_fid,
                                                   uint8_t* __restrict__ keep, uint64_t* __restrict__ cnt) {
  filter_rows<false>(s, rows, R, gen, slots, mask, arena, src_fid, keep, cnt, Rules{}, nullptr);
}

__global__ __launch_bounds__(256) void k_ix_filter_rules(Src s, uint64_t rows, const bcw_decode_result* __restrict__ R,
                                                         uint64_t gen, const Slot* __restrict__ slots, uint64_t mask,
                                                         const uint8_t* __restrict__ arena, uint64_t src_fid,
                                                         uint8_t* __restrict__ keep, uint64_t* __restrict__ cnt,
                                                         Rules ru) {
  __shared__ __align__(16) rules::PrefixTable pt;
  {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(ru.table->w);
    uint4* dst = reinterpret_cast<uint4*>(pt.w);
    for (uint32_t q = threadIdx.x; q < ru.n_prefix * (rules::kPrefixWords / 4); q += 256) dst[q] = src[q];
    if (threadIdx.x < ru.n_prefix) pt.len[threadIdx.x] = ru.table->len[threadIdx.x];
  }
  __syncthreads();
  filter_rows<true>(s, rows, R, gen, slots, mask, arena, src_fid, keep, cnt, ru, &pt);
}

// the rule counts of a synchronous compaction whose output is final join the cumulative ones (rule counters:
// [0, 3) cumulative, [3, 6) the compaction in progress)
__global__ void k_ix_rule_commit(uint64_t* __restrict__ rc) {
  for (int r = 0; r < 3; ++r) {
    rc[r] += rc[3 + r];
    rc[3 + r] = 0;
  }
}

__global__ void k_ix_result(const uint64_t* __restrict__ cnt, bcw_index_result* __restrict__ r) {
  bcw_index_result o{};
  o.n_in = cnt[C_NIN];
  o.n_done = cnt[C_DONE];
  o.err_class = (int32_t)cnt[C_FAIL];
  if (!o.err_class && cnt[C_OVERFLOW]) o.err_class = BCW_IDX_ERR_FULL;
  *r = o;
}

// ---- growth: re-insert every claimed slot into a larger table ---------------------------------------
// slot S of an old table into the first empty slot of the fresh table nw from its hash, under the reference kref and
// the presence `live`; false: no empty slot
__device__ __forceinline__ bool insert_slot(Slot* __restrict__ nw, uint64_t mask, const Slot& S, uint64_t kref,
                                            uint64_t live) {
  uint64_t j = S.hash & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe, j = (j + 1) & mask) {
    if (atomicCAS(reinterpret_cast<unsigned long long*>(&nw[j].kref), 0ull, (unsigned long long)kref) == 0) {
      nw[j].seq = S.seq;
      nw[j].hash = S.hash;
      nw[j].fid = S.fid;
      nw[j].off = S.off;
      nw[j].size = S.size;
      nw[j].live = live;
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(256) void k_ix_rehash(const Slot* __restrict__ old, uint64_t old_cap,
                                                   Slot* __restrict__ nw, uint64_t mask) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= old_cap) return;
  const Slot S = old[i];
  if (S.kref == 0) return;
  (void)insert_slot(nw, mask, S, S.kref, S.live);  // the larger table has room
}

// ---- reclaim: rebuild the table and the arena from the live keys only ---------------------------------
// A removed key (Delete, k_ix_evict) keeps its slot and its arena entry: k_ix_claim only claims empty slots, and the
// arena only appends. This pass gives both back. One lane per old slot; a live slot (soft-deleted keys are live)
// takes a fresh arena entry (wave_alloc on the rebuild's own counter: arena order is unobservable), copies its
// {hash, length, padded key} entry as 16 B chunks and inserts itself into the zeroed new table as k_ix_rehash does,
// with its sequence number (the clock of the capacity bound) and value unchanged. Dead slots are dropped, so the
// new probe chains hold live keys only. The counters go to C_R_*; the host adopts them (k_ix_adopt) after it has
// seen that nothing failed, and keeps the old buffers otherwise.

// arena bytes the live keys' entries take (16 B header + the key padded to 16, as k_ix_commit lays them out)
__global__ __launch_bounds__(256) void k_ix_live_bytes(const Slot* __restrict__ slots, uint64_t cap,
                                                       const uint8_t* __restrict__ arena, uint64_t arena_cap,
                                                       uint64_t* __restrict__ out) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  uint64_t b = 0;
  if (i < cap && slots[i].kref && slots[i].live && slots[i].kref - 1 + 16 <= arena_cap)
    b = entry_bytes(entry_len(arena, slots[i].kref));
  b = wave_sum(b);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)b);
}

__global__ __launch_bounds__(256) void k_ix_compact(const Slot* __restrict__ old, uint64_t old_cap,
                                                    const uint8_t* __restrict__ old_arena, uint64_t old_arena_cap,
                                                    Slot* __restrict__ nw, uint64_t mask, uint8_t* __restrict__ arena,
                                                    uint64_t arena_cap, uint64_t* __restrict__ cnt) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  Slot S{};
  if (i < old_cap) S = old[i];
  bool act = S.kref != 0 && S.live != 0;
  uint64_t esz = 0;
  if (act) {
    // the entry lies inside the old arena (always, for a consistent index: checked, not assumed, before it is read)
    const uint64_t src = S.kref - 1;
    bool in = (S.kref & kProv) == 0 && (src & 15u) == 0 && src + 16 <= old_arena_cap;
    if (in) {
      esz = entry_bytes(entry_len(old_arena, S.kref));
      in = src + esz <= old_arena_cap;
    }
    if (!in) {
      atomicOr(reinterpret_cast<unsigned long long*>(&cnt[C_R_FAIL]), 1ull);
      act = false;
      esz = 0;
    }
  }
  const uint64_t a = wave_alloc(&cnt[C_R_ARENA], esz);
  (void)wave_alloc(&cnt[C_R_SLOTS], act ? 1ull : 0ull);
  if (!act) return;
  if (a + esz > arena_cap) {  // the host sizes the new arena for the live entries; never expected
    atomicOr(reinterpret_cast<unsigned long long*>(&cnt[C_R_FAIL]), 1ull);
    return;
  }
  const uint4* __restrict__ s = reinterpret_cast<const uint4*>(old_arena + (S.kref - 1));
  uint4* __restrict__ d = reinterpret_cast<uint4*>(arena + a);
  for (uint64_t c = 0; c < esz / 16; ++c) d[c] = s[c];
  if (!insert_slot(nw, mask, S, a + 1, 1))
    atomicOr(reinterpret_cast<unsigned long long*>(&cnt[C_R_FAIL]), 2ull);  // no empty slot; never expected
}

// the rebuilt table's counters become the index's: every claimed slot is live
__global__ void k_ix_adopt(uint64_t* __restrict__ cnt) {
  cnt[C_ARENA] = cnt[C_R_ARENA];
  cnt[C_SLOTS] = cnt[C_R_SLOTS];
  cnt[C_LIVE] = cnt[C_R_SLOTS];
}

// ---- export of the live entries (the Go shim loads them into its ShardMap after a GPU rebuild) --------
// fids (sorted, nf > 0): only entries whose value fid is one of them (the slice of the index that points into
// a set of WAL files: the compaction fan-out's filter snapshot); nf == 0: every entry. The membership test is
// bcw_drop.h's.
__device__ __forceinline__ bool slot_exported(const Slot& S, const uint64_t* __restrict__ fids, uint32_t nf) {
  return S.kref && S.live && (nf == 0 || drop::fid_in(fids, nf, S.fid));
}

__global__ __launch_bounds__(256) void k_ix_count(const Slot* __restrict__ slots, uint64_t cap,
                                                  const uint8_t* __restrict__ arena, const uint64_t* __restrict__ fids,
                                                  uint32_t nf, uint64_t* __restrict__ blk_n,
                                                  uint64_t* __restrict__ blk_b) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  uint64_t c = 0, b = 0;
  if (i < cap && slot_exported(slots[i], fids, nf)) {
    c = 1;
    b = entry_len(arena, slots[i].kref);
  }
  c = wave_sum(c);
  b = wave_sum(b);
  __shared__ uint64_t sc[4], sb[4];
  if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = c; sb[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_n[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
    blk_b[blockIdx.x] = sb[0] + sb[1] + sb[2] + sb[3];
  }
}

__global__ __launch_bounds__(256) void k_ix_export(const Slot* __restrict__ slots, uint64_t cap,
                                                   const uint8_t* __restrict__ arena, const uint64_t* __restrict__ fids,
                                                   uint32_t nf, const uint64_t* __restrict__ blk_n,
                                                   const uint64_t* __restrict__ blk_b, uint8_t* __restrict__ keys,
                                                   uint64_t* __restrict__ koff, uint64_t* __restrict__ fid,
                                                   uint64_t* __restrict__ off, uint64_t* __restrict__ size) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  uint64_t c = 0, b = 0;
  Slot S{};
  if (i < cap) S = slots[i];
  const bool act = i < cap && slot_exported(S, fids, nf);
  if (act) {
    c = 1;
    b = entry_len(arena, S.kref);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t ic = c, ib = b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t tc = __shfl_up(ic, d, 64), tb = __shfl_up(ib, d, 64);
    if (lane >= (uint32_t)d) { ic += tc; ib += tb; }
  }
  __shared__ uint64_t wc[4], wb[4];
  if (lane == 63) { wc[wave] = ic; wb[wave] = ib; }
  __syncthreads();
  uint64_t pc = blk_n[blockIdx.x], pb = blk_b[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) { pc += wc[w]; pb += wb[w]; }
  pc += ic - c;
  pb += ib - b;
  if (!act) return;
  koff[pc] = pb;
  koff[pc + 1] = pb + b;  // the next entry writes the same value (or this is the last entry)
  fid[pc] = S.fid;
  off[pc] = S.off;
  size[pc] = S.size;
  const uint8_t* src = arena + (S.kref - 1) + 16;
  for (uint64_t q = 0; q < b; ++q) keys[pb + q] = src[q];
}

// ---- the capacity bound (bcw_index_set_limit): map.go's ShardMap keeps 16 shards (hash % 16) of Limited / 16 keys
// each and, when an insert would exceed a shard's limit, evicts the entry of minimum expire among sampled ones
// (SimpleMap.Set map.go:185-187, evict map.go:395-420, evictMinExpireEntry map.go:319). The device restates the
// bound with a deterministic policy: an entry's expire is the sequence number of the last op that set it (the
// index's logical clock in place of genExpire's wall seconds), and at the end of every batch each shard holding more
// than its limit evicts its entries of smallest sequence number (exact LRU order, every entry sampled) until it holds
// its limit. One workgroup per shard: count its live keys, radix-select (11-bit digits over npass passes) the
// (n - limit)-th smallest sequence number T (sequence numbers are unique), then evict every entry with seq <= T (live
// = 0, as Delete: the slot and the key's arena entry stay dead until the next live-only rebuild, k_ix_compact, which
// the host runs once half the claimed slots are dead, so the bound limits HBM use too). The evicted keys and their value sizes are counted (C_EVICTED*), the
// WriteStat of an eviction (index.go:144-165 reports the evicted value from Set's eviction path).
__global__ __launch_bounds__(1024) void k_ix_evict(Slot* __restrict__ slots, uint64_t cap, uint64_t lim,
                                                   uint64_t* __restrict__ cnt, uint32_t npass) {
  __shared__ uint32_t hist[2048];
  __shared__ unsigned long long s_acc[3];
  __shared__ uint64_t s_sel[2];  // prefix so far, rank left
  const uint32_t shard = blockIdx.x, tid = threadIdx.x;
  if (tid < 3) s_acc[tid] = 0;
  __syncthreads();
  uint64_t n = 0;
  for (uint64_t i = tid; i < cap; i += blockDim.x) n += (slots[i].live != 0 && (slots[i].hash & 15u) == shard) ? 1 : 0;
  atomicAdd(&s_acc[0], (unsigned long long)n);
  __syncthreads();
  const uint64_t total = s_acc[0];
  if (total <= lim) return;
  if (tid == 0) { s_sel[0] = 0; s_sel[1] = total - lim; }
  for (int p = (int)npass - 1; p >= 0; --p) {
    const uint32_t sh = 11u * (uint32_t)p;
    const uint64_t hi = (uint32_t)p + 1u >= npass ? 0ull : ~((1ull << (sh + 11u)) - 1ull);  // digits already chosen
    for (uint32_t b = tid; b < 2048u; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    const uint64_t pre = s_sel[0];
    for (uint64_t i = tid; i < cap; i += blockDim.x) {
      const Slot& q = slots[i];
      if (q.live != 0 && (q.hash & 15u) == shard && (q.seq & hi) == (pre & hi))
        atomicAdd(&hist[(q.seq >> sh) & 2047u], 1u);
    }
    __syncthreads();
    if (tid == 0) {  // the digit holding the rank-th smallest (a serial scan: evictions are rare)
      uint64_t rank = s_sel[1], c = 0;
      uint32_t b = 0;
      for (; b < 2047u && c + hist[b] < rank; ++b) c += hist[b];
      s_sel[0] = pre | ((uint64_t)b << sh);
      s_sel[1] = rank - c;
    }
    __syncthreads();
  }
  const uint64_t T = s_sel[0];
  uint64_t ev = 0, evb = 0;
  for (uint64_t i = tid; i < cap; i += blockDim.x) {
    Slot& q = slots[i];
    if (q.live != 0 && (q.hash & 15u) == shard && q.seq <= T) {
      q.live = 0;
      ++ev;
      evb += q.size;
    }
  }
  atomicAdd(&s_acc[1], (unsigned long long)ev);
  atomicAdd(&s_acc[2], (unsigned long long)evb);
  __syncthreads();
  if (tid == 0 && s_acc[1]) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[C_EVICTED]), s_acc[1]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[C_EVICTED_BYTES]), s_acc[2]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[C_LIVE]), (unsigned long long)(0ull - s_acc[1]));
  }
}

// ---- live usage per fid (bcw_index_fid_usage*, bcw_usage.h): one read-only pass over the slot table ----------
// A workgroup takes 256 slots per round: their 16 KiB go through LDS as 1024 contiguous 16 B loads (every lane's load
// next to its neighbour's; a slot's four chunks land rotated by its index so that the lanes' 16 B reads of one field
// pair spread over all banks), then each lane reads {fid}, {off, size}, {live} of its own slot (usage_round: the one
// text of that round, compiled by this pass and by its writing twin, k_ix_drop). A slot is counted iff live and
// off >= 40; its span is WalRecordSize in closed form (the size is not trusted). Rows go to the workgroup's
// accumulator; soft-deleted (live, off == 0) and invalid (live, 0 < off < 40) slots are only counted.
constexpr uint32_t kUsageSlots = usage::kThreads;  // slots per workgroup round
__device__ __forceinline__ uint32_t usage_chunk_pos(uint32_t slot, uint32_t q) { return slot * 4 + (q ^ ((slot >> 2) & 3u)); }

struct UsageLane {  // what a lane holds of its slot after a round; live is false for a lane past the table's end
  bool live;
  uint64_t fid, off, size;
  uint64_t kref, hash;  // kKey rounds only (the scrub names the entry's key)
};

// one round: slots [base, base + 256) of the table (fewer at its end) through `stage` (kUsageSlots * 4 chunks), every
// thread of the workgroup calls it; the lane's slot is base + threadIdx.x
template <bool kKey = false>
__device__ __forceinline__ UsageLane usage_round(const Slot* __restrict__ slots, uint64_t cap, uint64_t base,
                                                 uint4* __restrict__ stage) {
  const uint32_t tid = threadIdx.x;
  const uint64_t left = cap - base;
  const uint32_t nslots = left < kUsageSlots ? (uint32_t)left : kUsageSlots;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(slots + base);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t j = k * usage::kThreads + tid;  // chunk j of the round: slot j / 4, 16 B part j % 4
    if (j < nslots * 4) stage[usage_chunk_pos(j >> 2, j & 3u)] = src[j];
  }
  __syncthreads();
  const bool valid = tid < nslots;
  const uint4 hf = stage[usage_chunk_pos(tid, 1)], os = stage[usage_chunk_pos(tid, 2)],
              lp = stage[usage_chunk_pos(tid, 3)];
  uint4 ks = make_uint4(0, 0, 0, 0);
  if (kKey) ks = stage[usage_chunk_pos(tid, 0)];
  __syncthreads();  // the next round overwrites the staging buffer
  UsageLane r;
  r.kref = (uint64_t)ks.x | ((uint64_t)ks.y << 32);
  r.hash = (uint64_t)hf.x | ((uint64_t)hf.y << 32);
  r.fid = (uint64_t)hf.z | ((uint64_t)hf.w << 32);
  r.off = (uint64_t)os.x | ((uint64_t)os.y << 32);
  r.size = (uint64_t)os.z | ((uint64_t)os.w << 32);
  r.live = valid && (lp.x | lp.y) != 0;
  return r;
}

__global__ __launch_bounds__(usage::kThreads) void k_ix_usage(const Slot* __restrict__ slots, uint64_t cap,
                                                              uint64_t* __restrict__ scratch) {
  __shared__ usage::Accum acc;
  __shared__ uint4 stage[kUsageSlots * 4];
  acc.init();
  const usage::Table g = usage::table_of(scratch);
  const uint32_t tid = threadIdx.x;
  uint64_t n_soft = 0, n_inv = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kUsageSlots; base < cap; base += (uint64_t)gridDim.x * kUsageSlots) {
    const UsageLane r = usage_round(slots, cap, base, stage);
    const bool counted = r.live && r.off >= BCW_SUPER_BLOCK_SIZE;
    n_soft += (r.live && r.off == 0) ? 1 : 0;
    n_inv += (r.live && r.off != 0 && r.off < BCW_SUPER_BLOCK_SIZE) ? 1 : 0;
    const uint64_t span = counted ? usage::wal_record_size_closed(r.off, r.size) : 0;
    acc.add(g, counted, r.fid, true, r.size, span);
  }
  acc.flush(g);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_soft += __shfl_xor(n_soft, d, 64);
    n_inv += __shfl_xor(n_inv, d, 64);
  }
  if ((tid & 63u) == 0) {
    if (n_soft) atomicAdd(&g.aux[usage::A_SOFT], (unsigned long long)n_soft);
    if (n_inv) atomicAdd(&g.aux[usage::A_INVALID], (unsigned long long)n_inv);
  }
}

// ---- retiring WAL files (bcw_index_drop_fids*, bcw_drop.h): the writing twin of k_ix_usage -------------------------
// The same rounds. The fid list (ascending, distinct, at most BCW_USAGE_MAX_FIDS) is searched from dynamic LDS sized
// to the list, so a list of the one to three files of a compaction leaves the workgroup's LDS, and with it the
// occupancy, at k_ix_usage's; the [min, max] range test comes before the search. A wave in which no lane is selected
// (the ballot) does no accumulator work and stores nothing. A selected lane stores the 8 bytes of its slot's `live`
// (every slot belongs to one lane of one workgroup: no other thread of the pass reads or writes it) and feeds the
// accumulator by k_ix_usage's counting rule; each wave adds its dropped count to a word of LDS and the workgroup takes
// the sum off C_LIVE with one atomic at the end (one atomic per wave was measured: 8,192 adds to one address took
// longer than the pass itself).
// The stores and the C_LIVE count do not depend on the accounting table (an overflow voids only rows and totals).
__global__ __launch_bounds__(usage::kThreads) void k_ix_drop(Slot* __restrict__ slots, uint64_t cap,
                                                             const uint64_t* __restrict__ d_fids, uint32_t nf,
                                                             int mode, uint64_t* __restrict__ scratch,
                                                             uint64_t* __restrict__ cnt) {
  __shared__ usage::Accum acc;
  __shared__ uint4 stage[kUsageSlots * 4];
  extern __shared__ uint64_t s_fids[];  // nf entries
  __shared__ unsigned long long s_drop;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_drop = 0;
  for (uint32_t i = tid; i < nf; i += usage::kThreads) s_fids[i] = d_fids[i];
  acc.init();  // ends with the barrier that publishes the list too
  const usage::Table g = usage::table_of(scratch);
  uint64_t n_soft = 0, n_inv = 0, n_drop = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kUsageSlots; base < cap; base += (uint64_t)gridDim.x * kUsageSlots) {
    const UsageLane r = usage_round(slots, cap, base, stage);
    n_soft += (r.live && r.off == 0) ? 1 : 0;
    const bool file = r.live && r.off != 0;  // only these are searched
    const bool sel = drop::selected(mode, r.live, r.off, file && drop::fid_in_range(s_fids, nf, r.fid));
    if (__ballot(sel) == 0) continue;  // wave-uniform
    const bool counted = sel && r.off >= BCW_SUPER_BLOCK_SIZE;
    n_drop += sel ? 1 : 0;
    n_inv += (sel && !counted) ? 1 : 0;
    if (sel) slots[base + tid].live = 0;  // sel implies a lane inside the table
    const uint64_t span = counted ? usage::wal_record_size_closed(r.off, r.size) : 0;
    acc.add(g, counted, r.fid, true, r.size, span);
  }
  acc.flush(g);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_soft += __shfl_xor(n_soft, d, 64);
    n_inv += __shfl_xor(n_inv, d, 64);
    n_drop += __shfl_xor(n_drop, d, 64);
  }
  if ((tid & 63u) == 0) {
    if (n_soft) atomicAdd(&g.aux[usage::A_SOFT], (unsigned long long)n_soft);
    if (n_inv) atomicAdd(&g.aux[usage::A_INVALID], (unsigned long long)n_inv);
    if (n_drop) atomicAdd(&s_drop, (unsigned long long)n_drop);
  }
  __syncthreads();
  if (tid == 0 && s_drop) atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[C_LIVE]), 0ull - s_drop);
}

// ---- scrub, the select pass (bcw_index_verify*, bcw_verify.h): the reading twin that names keys ----------------------
// The same rounds, with the slot's kref and hash. A live slot with off != 0 is checked: wal_span decides NO_WAL and
// READ / BEYOND here (such an entry is emitted as bad, vfy::emit_bad, and feeds the accumulator by k_ix_usage's
// counting rule), every other checked entry becomes a work item for k_vfy_read. The items of a wave are compacted by
// ballot into the wave's own 64-item buffer in LDS; a buffer that cannot take a round's items goes to the queue first,
// behind one reservation per wave (V_QUEUE), as 64 adjacent items. One reservation per wave and round was built
// first and measured: at one key per 33 slots nearly every wave-round has an item, and the adds to the
// one address took ten times the pass. A write past queue_cap, which the slot capacity never reaches, is dropped.
// Order in the queue is unobservable and no workgroup waits for another. Index values are data here, never addresses:
// only kref, which the index itself wrote, is followed. Counters are summed per lane, reduced per wave and added into
// LDS; the workgroup adds each to its global word once, at the end (k_ix_drop's note).
// the first n items of a wave's buffer to the queue, by the whole wave (n is wave-uniform)
__device__ __forceinline__ void vfy_flush(const vfy::Item* __restrict__ buf, uint32_t n, unsigned long long* q_count,
                                          vfy::Item* __restrict__ queue, uint64_t queue_cap, uint32_t lane) {
  if (n == 0) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  unsigned long long q0 = 0;
  if (lane == 0) q0 = atomicAdd(q_count, (unsigned long long)n);
  const uint64_t pos = __shfl(q0, 0, 64) + lane;
  if (lane < n && pos < queue_cap) queue[pos] = buf[lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the buffer is rewritten next
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(usage::kThreads) void k_ix_vfy_select(const Slot* __restrict__ slots, uint64_t cap,
                                                                   const WalEnt* __restrict__ wals, uint32_t n_wals,
                                                                   vfy::Sink S, vfy::Item* __restrict__ queue,
                                                                   uint64_t queue_cap, uint64_t* __restrict__ scratch) {
  __shared__ usage::Accum acc;
  __shared__ uint4 stage[kUsageSlots * 4];
  __shared__ unsigned long long s_cnt[5];  // checked, soft-deleted, invalid, NO_WAL, BEYOND
  __shared__ __align__(16) vfy::Item s_q[usage::kThreads / 64][64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  vfy::Item* const wq = s_q[tid >> 6];
  if (tid < 5) s_cnt[tid] = 0;
  acc.init();
  const usage::Table g = usage::table_of(scratch);
  uint64_t n_chk = 0, n_soft = 0, n_inv = 0, n_nowal = 0, n_beyond = 0;
  uint32_t nq = 0;  // items in the wave's buffer (wave-uniform)
  for (uint64_t base = (uint64_t)blockIdx.x * kUsageSlots; base < cap; base += (uint64_t)gridDim.x * kUsageSlots) {
    const UsageLane r = usage_round<true>(slots, cap, base, stage);
    n_soft += (r.live && r.off == 0) ? 1 : 0;
    const bool chk = r.live && r.off != 0;
    if (__ballot(chk) == 0) continue;  // wave-uniform
    uint32_t cls = BCW_VFY_OK, wal = 0, klen = 0;
    if (chk) {
      bool beyond;
      wal = wal_span(wals, n_wals, r.fid, r.off, r.size, &beyond);
      cls = vfy::classify(wal < n_wals, beyond ? BCW_RD_BEYOND : BCW_RD_OK, BCW_ST_OK, true);
      klen = entry_len(S.arena, r.kref);
      n_chk += 1;
      n_nowal += cls == BCW_VFY_NO_WAL ? 1 : 0;
      n_beyond += cls == BCW_VFY_READ ? 1 : 0;
    }
    const bool work = chk && cls == BCW_VFY_OK, bad = chk && cls != BCW_VFY_OK;
    const uint64_t m = __ballot(work);
    if (m) {
      const uint32_t k = (uint32_t)__popcll(m);  // <= 64: an empty buffer always takes a round
      if (nq + k > 64) {
        vfy_flush(wq, nq, &S.cnt[vfy::V_QUEUE], queue, queue_cap, lane);
        nq = 0;
      }
      if (work)
        wq[nq + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] =
            vfy::Item{r.fid, r.off, r.size, r.hash, r.kref, wal, klen};
      nq += k;
    }
    if (__ballot(bad) == 0) continue;
    const bool counted = bad && r.off >= BCW_SUPER_BLOCK_SIZE;
    n_inv += (bad && !counted) ? 1 : 0;
    if (bad)
      vfy::emit_bad(S, r.fid, r.off, r.size, r.hash, r.kref, klen, cls, cls == BCW_VFY_READ ? BCW_RD_BEYOND : BCW_RD_OK,
                    BCW_ST_OK);
    const uint64_t span = counted ? usage::wal_record_size_closed(r.off, r.size) : 0;
    acc.add(g, counted, r.fid, true, r.size, span);
  }
  vfy_flush(wq, nq, &S.cnt[vfy::V_QUEUE], queue, queue_cap, lane);
  acc.flush(g);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_chk += __shfl_xor(n_chk, d, 64);
    n_soft += __shfl_xor(n_soft, d, 64);
    n_inv += __shfl_xor(n_inv, d, 64);
    n_nowal += __shfl_xor(n_nowal, d, 64);
    n_beyond += __shfl_xor(n_beyond, d, 64);
  }
  if (lane == 0) {
    if (n_chk) atomicAdd(&s_cnt[0], (unsigned long long)n_chk);
    if (n_soft) atomicAdd(&s_cnt[1], (unsigned long long)n_soft);
    if (n_inv) atomicAdd(&s_cnt[2], (unsigned long long)n_inv);
    if (n_nowal) atomicAdd(&s_cnt[3], (unsigned long long)n_nowal);
    if (n_beyond) atomicAdd(&s_cnt[4], (unsigned long long)n_beyond);
  }
  __syncthreads();
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&S.cnt[vfy::V_CHECKED], s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&g.aux[usage::A_SOFT], s_cnt[1]);
    if (s_cnt[2]) atomicAdd(&g.aux[usage::A_INVALID], s_cnt[2]);
    if (s_cnt[3]) atomicAdd(&S.cnt[vfy::V_CLASS + BCW_VFY_NO_WAL], s_cnt[3]);
    if (s_cnt[4]) {
      atomicAdd(&S.cnt[vfy::V_CLASS + BCW_VFY_READ], s_cnt[4]);
      atomicAdd(&S.cnt[vfy::V_RD + BCW_RD_BEYOND], s_cnt[4]);
    }
  }
}

// ---- scan by key prefix (bcw_index_scan*, bcw_scan.h): list and fold a namespace ------------------------------------
// Three stream-ordered launches, so every hand-off between workgroups is a kernel boundary:
//   k_ix_scan_select   the usage rounds with the slot's kref: a live lane reads its arena entry's length and the key
//                      chunks a prefix can reach, scan::decide names its group; out go a verdict byte per slot, each
//                      256-slot tile's listed entries and key bytes, and the group rows
//   k_ix_scan_offsets  one workgroup: the exclusive prefix sums of the two tile columns, in place, 1024 tiles a round
//                      with a carry (any tile count), then the result, `fits` and the caller's group rows
//   k_ix_scan_emit     a workgroup per tile: the verdict bytes, coalesced; slots and arena only for listed lanes; the
//                      rank inside the tile by ballot and popcount over its waves; offsets, columns, keys
// An entry's place in the output is the number of listed slots before its own, so the layout is in slot order and the
// same bytes come out whatever the scheduling. Nothing here writes the index.
// workgroups per CU the select and emit grids are capped at (both stride over the tiles beyond that): the select pass
// holds 22.6 KiB of LDS and 16 KiB of loads in flight per workgroup, the emit pass next to nothing
constexpr uint32_t kScanSelectPerCu = 4, kScanEmitPerCu = 8;

struct ScanArgs {
  const rules::PrefixTable* table;  // device; read only when n_prefix > 0
  uint32_t n_prefix, longest, flags;
  uint8_t* verdict;                 // [slots] 0: not listed, 1 + group
  uint64_t *tile_n, *tile_b;        // [tiles] listed entries, their key bytes
  unsigned long long* acc;          // [scan::kAccWords] the group rows and the live count, zeroed by the call
};

// the entry a slot's kref names lies inside the arena (always, for a consistent index: checked, not assumed, before
// it is read, as k_ix_compact does); *len: the key's length
__device__ __forceinline__ bool scan_entry(const uint8_t* __restrict__ arena, uint64_t arena_cap, uint64_t kref,
                                           uint32_t* len) {
  const uint64_t a = kref - 1;
  if (kref == 0 || (kref & kProv) || (a & 15u) || a + 16 > arena_cap) return false;
  *len = entry_len(arena, kref);
  return a + entry_bytes(*len) <= arena_cap;
}

// The group rows go through a per-workgroup accumulator in LDS: the lanes of a wave that share a group (all of them,
// when one namespace is scanned) are summed by ballot and butterfly and added by one lane, one round of the loop per
// distinct group in the wave; the workgroup adds each non-zero word to its global word once, at the end (k_ix_drop's
// note on measured contention). The tile columns are plain stores: every tile belongs to one round of one workgroup.
// A wave with no live lane loads nothing and matches nothing; it still stores its 64 verdict bytes, which nothing
// else zeroes.
__global__ __launch_bounds__(usage::kThreads) void k_ix_scan_select(const Slot* __restrict__ slots, uint64_t cap,
                                                                    const uint8_t* __restrict__ arena,
                                                                    uint64_t arena_cap, ScanArgs A) {
  static_assert(kUsageSlots == scan::kTileSlots, "a tile is one usage round");
  __shared__ __align__(16) rules::PrefixTable pt;
  __shared__ uint4 stage[kUsageSlots * 4];
  __shared__ unsigned long long s_acc[scan::kAccWords];
  __shared__ uint64_t s_tile[usage::kThreads / 64][2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (A.n_prefix) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(A.table->w);
    uint4* dst = reinterpret_cast<uint4*>(pt.w);
    for (uint32_t q = tid; q < A.n_prefix * (rules::kPrefixWords / 4); q += usage::kThreads) dst[q] = src[q];
    if (tid < A.n_prefix) pt.len[tid] = A.table->len[tid];
  }
  for (uint32_t q = tid; q < scan::kAccWords; q += usage::kThreads) s_acc[q] = 0;
  __syncthreads();
  uint64_t n_live = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kUsageSlots; base < cap; base += (uint64_t)gridDim.x * kUsageSlots) {
    const UsageLane r = usage_round<true>(slots, cap, base, stage);
    n_live += r.live ? 1 : 0;
    uint32_t verdict = 0;
    uint64_t kb = 0;
    if (__ballot(r.live) != 0) {  // wave-uniform
      scan::Hit h{};
      uint32_t klen = 0;
      if (r.live && scan_entry(arena, arena_cap, r.kref, &klen)) {
        uint32_t kw[4 * rules::kKeyChunks] = {};
        if (A.n_prefix) {
          const uint32_t n = rules::key_chunks(klen, A.longest);
          const uint4* __restrict__ q = reinterpret_cast<const uint4*>(arena + (r.kref - 1) + 16);
#pragma unroll
          for (uint32_t c = 0; c < rules::kKeyChunks; ++c) {
            if (c >= n) break;
            const uint4 x = q[c];
            kw[4 * c] = x.x;
            kw[4 * c + 1] = x.y;
            kw[4 * c + 2] = x.z;
            kw[4 * c + 3] = x.w;
          }
        }
        h = scan::decide(true, r.off, r.size, kw, klen, pt.w, pt.len, A.n_prefix, A.flags);
      }
      for (uint64_t m = __ballot(h.match); m != 0;) {  // one round per distinct group in the wave
        const int lead = __ffsll((unsigned long long)m) - 1;
        const uint32_t g = __shfl(h.group, lead, 64);
        const bool mine = h.match && h.group == g;
        const uint64_t cnt = (uint64_t)__popcll(__ballot(mine && !h.soft));
        const uint64_t soft = (uint64_t)__popcll(__ballot(mine && h.soft));
        const uint64_t by = wave_sum(mine ? h.bytes : 0), kby = wave_sum(mine ? h.key_bytes : 0);
        if ((int)lane == lead) {
          unsigned long long* row = &s_acc[g * scan::G_WORDS];
          if (cnt) atomicAdd(&row[scan::G_COUNT], (unsigned long long)cnt);
          if (by) atomicAdd(&row[scan::G_BYTES], (unsigned long long)by);
          if (kby) atomicAdd(&row[scan::G_KEY_BYTES], (unsigned long long)kby);
          if (soft) atomicAdd(&row[scan::G_SOFT], (unsigned long long)soft);
        }
        m &= ~__ballot(mine);
      }
      verdict = scan::verdict_of(h);
      kb = verdict ? klen : 0;
    }
    if (base + tid < cap) A.verdict[base + tid] = (uint8_t)verdict;
    const uint64_t lm = __ballot(verdict != 0);
    if (lm) kb = wave_sum(kb);  // wave-uniform
    if (lane == 0) {
      s_tile[wave][0] = (uint64_t)__popcll(lm);
      s_tile[wave][1] = kb;
    }
    __syncthreads();  // the next writes of s_tile come behind the two barriers of the next round
    if (tid == 0) {
      uint64_t n = 0, b = 0;
      for (uint32_t w = 0; w < usage::kThreads / 64; ++w) { n += s_tile[w][0]; b += s_tile[w][1]; }
      A.tile_n[scan::tile_of(base)] = n;
      A.tile_b[scan::tile_of(base)] = b;
    }
  }
  n_live = wave_sum(n_live);
  if (lane == 0 && n_live) atomicAdd(&s_acc[scan::kLiveWord], (unsigned long long)n_live);
  __syncthreads();
  for (uint32_t q = tid; q < scan::kAccWords; q += usage::kThreads)
    if (s_acc[q]) atomicAdd(&A.acc[q], s_acc[q]);
}

// One workgroup of 1024 threads: a thread per tile and round, the wave's inclusive scan by shuffles, the waves' totals
// through LDS, the carry of the rounds before in every thread. Then the totals (bytes and n_soft_deleted are the sums
// of the rows' columns), `fits`, the caller's group rows, and -- when the outputs are whole -- the last offset,
// key_off[n_listed] = key_bytes (key_off[0] = 0 of an empty listing included); the emit pass writes the others.
constexpr uint32_t kScanOffsetsThreads = 1024;
__global__ __launch_bounds__(kScanOffsetsThreads) void k_ix_scan_offsets(uint64_t* __restrict__ tile_n,
                                                                         uint64_t* __restrict__ tile_b, uint64_t tiles,
                                                                         const unsigned long long* __restrict__ acc,
                                                                         uint32_t rows, bcw_scan_out out,
                                                                         bcw_scan_result* __restrict__ res) {
  constexpr uint32_t kWaves = kScanOffsetsThreads / 64;
  __shared__ uint64_t s_w[kWaves][2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t cn = 0, cb = 0;  // listed entries and key bytes of the rounds before
  for (uint64_t t0 = 0; t0 < tiles; t0 += kScanOffsetsThreads) {
    const uint64_t i = t0 + tid;
    const uint64_t n = i < tiles ? tile_n[i] : 0, b = i < tiles ? tile_b[i] : 0;
    uint64_t in = n, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t tn = __shfl_up(in, d, 64), tb = __shfl_up(ib, d, 64);
      if (lane >= (uint32_t)d) { in += tn; ib += tb; }
    }
    if (lane == 63) { s_w[wave][0] = in; s_w[wave][1] = ib; }
    __syncthreads();
    uint64_t pn = cn, pb = cb;
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint64_t wn = s_w[w][0], wb = s_w[w][1];
      if (w < wave) { pn += wn; pb += wb; }
      cn += wn;
      cb += wb;
    }
    if (i < tiles) {
      tile_n[i] = pn + in - n;
      tile_b[i] = pb + ib - b;
    }
    __syncthreads();  // the next round overwrites s_w
  }
  if (out.groups && tid < rows * scan::G_WORDS) reinterpret_cast<uint64_t*>(out.groups)[tid] = acc[tid];
  if (tid != 0) return;
  bcw_scan_result o{};
  o.n_listed = cn;
  o.key_bytes = cb;
  for (uint32_t r = 0; r < rows; ++r) {
    o.bytes += acc[r * scan::G_WORDS + scan::G_BYTES];
    o.n_soft_deleted += acc[r * scan::G_WORDS + scan::G_SOFT];
  }
  o.n_live = acc[scan::kLiveWord];
  o.fits = scan::fits(cn, out.entries_cap, cb, out.keys_cap) ? 1u : 0u;
  *res = o;
  if (o.fits && out.key_off) out.key_off[cn] = cb;
}

// len key bytes from src (an arena key: 16-byte aligned, padded to 16) to dst (any alignment), in 16-byte granules
// aligned to the destination. Neighbouring keys share destination granules, and those keys may be written by other
// waves or workgroups at the same time, so no granule that holds another key's bytes is read or written whole: the
// bytes before the first granule that lies inside this key, and those behind the last one, are byte stores; every
// 16-byte store covers only bytes of this key. A whole granule is bytes [o, o + 16) of the key, unaligned in the
// arena by the head's length: the two-chunk funnel (shift16), each chunk loaded once. Chunk c + 1 is read only when a
// byte of it is needed, so never past the entry.
__device__ __forceinline__ void scan_copy_key(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                              uint32_t len) {
  const uint32_t lead = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  const uint32_t head = lead < len ? lead : len;
  for (uint32_t q = 0; q < head; ++q) dst[q] = src[q];
  uint32_t o = head;
  if (len - o >= 16) {
    const uint4* __restrict__ s = reinterpret_cast<const uint4*>(src);
    const uint32_t sh = head;  // o % 16 of every granule
    uint32_t c = 0;
    uint4 v0 = s[0];
    for (; len - o >= 16; o += 16, ++c) {
      uint4 v = v0;
      if (sh) {
        const uint4 v1 = s[c + 1];  // holds key byte 16 c + 16 <= o + 15 < len
        v = shift16(v0, v1, sh);
        v0 = v1;
      } else if (len - o >= 32) {
        v0 = s[c + 1];
      }
      *reinterpret_cast<uint4*>(dst + o) = v;
    }
  }
  for (; o < len; ++o) dst[o] = src[o];
}

// Bounds: a listed lane's entry passed scan_entry in the select pass of the same call, on the same buffers; its place
// (pc, pb) is a prefix sum of the very counts `fits` was decided from, and is checked against the caps all the same
// before anything is stored.
__global__ __launch_bounds__(scan::kTileSlots) void k_ix_scan_emit(const Slot* __restrict__ slots, uint64_t cap,
                                                                   const uint8_t* __restrict__ arena,
                                                                   const uint8_t* __restrict__ verdict,
                                                                   const uint64_t* __restrict__ tile_n,
                                                                   const uint64_t* __restrict__ tile_b, uint64_t tiles,
                                                                   bcw_scan_out out,
                                                                   const bcw_scan_result* __restrict__ res) {
  constexpr uint32_t kWaves = scan::kTileSlots / 64;
  __shared__ uint64_t s_w[kWaves][2];
  if (res->fits == 0) return;
  const uint64_t n_listed = res->n_listed;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t t0 = tile_n[tile], t1 = tile + 1 < tiles ? tile_n[tile + 1] : n_listed;
    if (t1 == t0) continue;  // nothing listed in this tile (uniform over the workgroup)
    const uint64_t i = scan::tile_base(tile) + tid;
    const uint32_t v = i < cap ? verdict[i] : 0u;
    const bool listed = v != 0;
    uint64_t kref = 0, fid = 0, off = 0, size = 0;
    uint32_t klen = 0;
    if (listed) {
      const Slot& S = slots[i];
      kref = S.kref;
      fid = S.fid;
      off = S.off;
      size = S.size;
      klen = entry_len(arena, kref);
    }
    const uint64_t lm = __ballot(listed);
    uint64_t ib = klen;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t tb = __shfl_up(ib, d, 64);
      if (lane >= (uint32_t)d) ib += tb;
    }
    if (lane == 63) { s_w[wave][0] = (uint64_t)__popcll(lm); s_w[wave][1] = ib; }
    __syncthreads();
    uint64_t pc = t0 + (uint64_t)__popcll(lm & ((1ull << lane) - 1ull)), pb = tile_b[tile] + ib - klen;
    for (uint32_t w = 0; w < wave; ++w) { pc += s_w[w][0]; pb += s_w[w][1]; }
    __syncthreads();  // the next tile overwrites s_w
    if (!listed || pc >= out.entries_cap || pb + klen > out.keys_cap) continue;
    out.key_off[pc] = pb;
    if (out.fid) out.fid[pc] = fid;
    if (out.off) out.off[pc] = off;
    if (out.size) out.size[pc] = size;
    if (out.prefix_id) out.prefix_id[pc] = (uint8_t)scan::verdict_group(v);
    scan_copy_key(out.keys + pb, arena + (kref - 1) + 16, klen);
  }
}

}  // namespace ix
}  // namespace bcw

using namespace bcw;
using namespace bcw::ix;

struct bcw_index {
  bcw_ctx* ctx = nullptr;
  DevBuf<Slot> slots;
  uint64_t cap = 0;  // slots (power of two)
  DevBuf<uint8_t> arena;  // the key arena; arena.bytes() is its capacity
  DevBuf<uint64_t> cnt;  // device counters
  uint64_t slots_ub = 0, arena_ub = 0;  // host upper bounds of the device counters
  uint64_t seq_base = 1;                // sequence number of the next op
  uint64_t limited = 0;                 // the capacity bound (bcw_index_set_limit; 0: none)
  // per-op scratch: one allocation, three arrays of op_cap entries
  DevBuf<> op_mem;
  struct { uint64_t *kref, *hash, *slot; } op{};
  uint64_t op_cap = 0;
  // host-batch staging (device copies), carved anew by every call (bcw_devmem.h)
  DevBuf<> stage;
  // compaction filter rules (bcw_index_set_compact_rules): the host copy (mask 0: none; the prefix arrays point into
  // the two vectors), the packed prefix table and the counters on the device (allocated with the first rules: three
  // cumulative words, then the three of a synchronous compaction in progress, k_ix_rule_commit), and the counts
  // bcw_compact_wals' workers took per source, added on the host for the sources whose output is final
  bcw_compact_rules rules{};
  std::vector<uint8_t> rule_bytes;
  std::vector<uint32_t> rule_off;
  uint32_t rule_longest = 0;
  DevBuf<rules::PrefixTable> d_rule_tab;
  DevBuf<uint64_t> d_rule_cnt;
  uint64_t rule_host[3] = {0, 0, 0};
  // the fid list of bcw_index_drop_fids* (allocated with the first drop, BCW_USAGE_MAX_FIDS entries each): the
  // normalised list in pinned host memory, its device copy, and the event behind the last copy out of the pinned
  // buffer, which the next call waits for before it overwrites the buffer (the copy alone, not the stream)
  uint64_t* drop_h = nullptr;
  DevBuf<uint64_t> drop_d;
  hipEvent_t drop_ev = nullptr;
  // the scrub's counters and work queue (bcw_index_verify*; grow-only, allocated with the first scrub), carved for
  // the vfy_q_cap slots of the largest table a scrub has met (carve_vfy_queue)
  DevBuf<> vfy_q;
  uint64_t vfy_q_cap = 0;
  // the scan's scratch (bcw_index_scan*; grow-only, allocated with the first scan), carved for the scan_cap slots of
  // the largest table a scan has met (carve_ix_scan), and the packed prefix table in pinned host memory with the event
  // behind its last copy to the device, as for the drop's fid list
  DevBuf<> scan_mem;
  uint64_t scan_cap = 0;
  rules::PrefixTable* scan_h = nullptr;
  hipEvent_t scan_ev = nullptr;
};

namespace {
// flat merged keys on the device: key i = keys[koff[i], koff[i + 1])
Src flat_src(const uint8_t* keys, const uint64_t* koff, uint64_t keys_len) {
  Src s{};
  s.kind = SRC_FLAT;
  s.keys = keys;
  s.koff = koff;
  s.keys_len = keys_len;
  return s;
}
}  // namespace

namespace bcw {
bcw_ctx* index_ctx(const bcw_index* ix) { return ix ? ix->ctx : nullptr; }

hipError_t ix_launch_get_lookup(bcw_index* x, const GetLookup& g, hipStream_t st) {
  if (g.n == 0) return hipSuccess;
  const Src s = flat_src(g.keys, g.koff, 0);  // keys_len: the kernel reads koff[n]
  k_get_lookup<<<(uint32_t)((g.n + kGetLookupKeys - 1) / kGetLookupKeys), kGetLookupKeys, 0, st>>>(
      s, g, x->slots.get(), x->cap - 1, x->arena.get());
  return hipGetLastError();
}
}  // namespace bcw

namespace {

constexpr double kMaxLoad = 0.7;

uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 1024;
  while (p < v) p <<= 1;
  return p;
}

int ix_sync_counters(bcw_index* x, uint64_t* out) {
  hipStream_t st = x->ctx->cur;
  const bool ok = copy_down(out, x->cnt.get(), C_NUM * sizeof(uint64_t), st) && hipStreamSynchronize(st) == hipSuccess;
  return ok ? BCW_OK : BCW_E_HIP;
}

// the host's upper bounds, made exact from counters just read (c: ix_sync_counters)
void ix_refresh_bounds(bcw_index* x, const uint64_t* c) {
  x->slots_ub = c[C_SLOTS];
  x->arena_ub = c[C_ARENA];
}

// three adjacent counters from `first` (cnt + C_NIN, cnt + C_R_ARENA, or the rules' three) to zero
hipError_t zero_group(uint64_t* first, hipStream_t st) { return hipMemsetAsync(first, 0, 3 * sizeof(uint64_t), st); }

// grow the slot table to hold `slots` claimed slots at kMaxLoad and the arena to `arena` bytes. The larger buffer is
// built in a local on the stream and adopted once the stream has drained (DevBuf::adopt): queued work reads the old
// one until then, and a failure returns with the index as it was.
int ix_grow(bcw_index* x, uint64_t slots, uint64_t arena) {
  hipStream_t st = x->ctx->cur;
  if (arena > x->arena.bytes()) {
    const uint64_t na = std::max(arena, x->arena.bytes() * 2);
    DevBuf<uint8_t> a;
    if (!a.alloc(na)) return BCW_E_NOMEM;
    if (x->arena && hipMemcpyAsync(a.get(), x->arena.get(), std::min(x->arena_ub, x->arena.bytes()),
                                   hipMemcpyDeviceToDevice, st) != hipSuccess)
      return BCW_E_HIP;
    x->arena.adopt(std::move(a), st);
  }
  const uint64_t want = pow2_at_least((uint64_t)((double)slots / kMaxLoad) + 1);
  if (want > x->cap) {
    DevBuf<Slot> ns;
    if (!ns.alloc(want * sizeof(Slot))) return BCW_E_NOMEM;
    if (hipMemsetAsync(ns.get(), 0, want * sizeof(Slot), st) != hipSuccess) return BCW_E_HIP;
    if (x->slots && x->cap)
      k_ix_rehash<<<(uint32_t)((x->cap + 255) / 256), 256, 0, st>>>(x->slots.get(), x->cap, ns.get(), want - 1);
    if (hipStreamSynchronize(st) != hipSuccess) return BCW_E_HIP;
    x->slots.adopt(std::move(ns), st);  // the stream is empty by now: adopt's own synchronise returns at once
    x->cap = want;
  }
  return BCW_OK;
}

// rebuild the index from its live keys only (k_ix_compact) into a table of ncap slots and an arena of narena bytes,
// both large enough for them; the new buffers are adopted after the stream sync, as in ix_grow. On an error the index
// is left as it was: the rebuild counts in the C_R_* counters, which k_ix_adopt moves over only when it succeeded.
int ix_compact(bcw_index* x, uint64_t ncap, uint64_t narena) {
  hipStream_t st = x->ctx->cur;
  DevBuf<Slot> ns;
  DevBuf<uint8_t> na;
  if (!ns.alloc(ncap * sizeof(Slot)) || !na.alloc(narena)) return BCW_E_NOMEM;
  uint64_t c[C_NUM];
  bool ok = hipMemsetAsync(ns.get(), 0, ncap * sizeof(Slot), st) == hipSuccess &&
            zero_group(x->cnt.get() + C_R_ARENA, st) == hipSuccess;
  if (ok)
    k_ix_compact<<<(uint32_t)((x->cap + 255) / 256), 256, 0, st>>>(x->slots.get(), x->cap, x->arena.get(),
                                                                   x->arena.bytes(), ns.get(), ncap - 1, na.get(),
                                                                   narena, x->cnt.get());
  ok = ok && hipGetLastError() == hipSuccess && ix_sync_counters(x, c) == BCW_OK && c[C_R_FAIL] == 0;
  if (ok) {
    k_ix_adopt<<<1, 1, 0, st>>>(x->cnt.get());
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  }
  if (!ok) return BCW_E_HIP;
  // the stream is empty by now (the checked synchronise above): the synchronise inside each adopt returns at once
  x->slots.adopt(std::move(ns), st);
  x->arena.adopt(std::move(na), st);
  x->cap = ncap;
  x->slots_ub = c[C_R_SLOTS];
  x->arena_ub = c[C_R_ARENA];
  return BCW_OK;
}

// make room for a batch of n ops whose arena entries total at most `arena_bytes`. When the batch does not fit the
// host bounds, the counters are read; if at least half the claimed slots are dead by then, the index is first rebuilt
// from its live keys at the capacities it has (ix_compact: O(capacity), paid for by the >= 0.35 * capacity removals
// since the last rebuild or growth -- amortised constant work per removal, as doubling is per insert), and it grows
// only if the batch still does not fit. A batch that fits costs no sync and no launch here.
int ix_room(bcw_index* x, uint64_t n, uint64_t arena_bytes) {
  const auto fits = [&] {
    return (double)(x->slots_ub + n) <= kMaxLoad * (double)x->cap && x->arena_ub + arena_bytes <= x->arena.bytes();
  };
  if (!fits()) {
    uint64_t c[C_NUM];
    int rc = ix_sync_counters(x, c);
    if (rc != BCW_OK) return rc;
    if (c[C_OVERFLOW]) return BCW_E_CAPACITY;  // a previous batch overflowed: the index is inconsistent
    ix_refresh_bounds(x, c);
    if (c[C_SLOTS] > 0 && c[C_SLOTS] - c[C_LIVE] >= c[C_SLOTS] / 2) {
      rc = ix_compact(x, x->cap, x->arena.bytes());
      if (rc != BCW_OK) return rc;
    }
    if (!fits()) {
      rc = ix_grow(x, x->slots_ub + n, x->arena_ub + arena_bytes);
      if (rc != BCW_OK) return rc;
    }
  }
  if (n > x->op_cap) {
    const uint64_t c = std::max<uint64_t>(n, 1024);
    const int rc = carve_reserve(x->op_mem, x->ctx->cur, [&](Carver& cv) {
      x->op = {cv.take<uint64_t>(c), cv.take<uint64_t>(c), cv.take<uint64_t>(c)};
    });
    x->op_cap = rc == BCW_OK ? c : 0;
    if (rc != BCW_OK) return rc;
  }
  x->slots_ub += n;
  x->arena_ub += arena_bytes;
  return BCW_OK;
}

// x->stage carved by a layout that begins with the flat keys of a host call (carve_ix_apply, carve_ix_get: *L), and
// the copies of the keys queued (flat_keys_ok, upload_flat_keys: bcw_host.h). *koff lives until the caller's sync.
template <class Layout>
int stage_flat_keys(bcw_index* x, uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off,
                    Layout (*carve)(Carver&, uint64_t, uint64_t), Layout* L, std::vector<uint64_t>* koff) {
  hipStream_t st = x->ctx->cur;
  const int rc = carve_reserve(x->stage, st, [&](Carver& cv) { *L = carve(cv, h_key_off[n] - h_key_off[0], n); });
  if (rc != BCW_OK) return rc;
  return upload_flat_keys(n, h_keys, h_key_off, L->k, st, koff) ? BCW_OK : BCW_E_HIP;
}

// the capacity bound after a batch (k_ix_evict), when one is set
void ix_bound(bcw_index* x) {
  if (!x->limited) return;
  uint32_t npass = 1;
  while (npass < 6 && (x->seq_base >> (11u * npass)) != 0) ++npass;  // digits of the largest sequence number
  k_ix_evict<<<16, 1024, 0, x->ctx->cur>>>(x->slots.get(), x->cap, x->limited / 16, x->cnt.get(), npass);
}

// the five launches of a batch (ops [0, n) of src); old_*: optional WriteStat outputs of k_ix_claim
void ix_batch(bcw_index* x, const Src& s, uint64_t n, const bcw_decode_result* R, uint64_t gen, const OpVals& v,
              uint8_t* old_found = nullptr, uint64_t* old_fid = nullptr, uint64_t* old_size = nullptr) {
  hipStream_t st = x->ctx->cur;
  const uint32_t grid = (uint32_t)((n + 255) / 256);
  (void)zero_group(x->cnt.get() + C_NIN, st);
  if (!grid) return;
  k_ix_keys<<<grid, 256, 0, st>>>(s, n, R, gen, x->cnt.get(), x->op.kref, x->op.hash);
  k_ix_claim<<<grid, 256, 0, st>>>(s, n, x->cnt.get(), x->slots.get(), x->cap - 1, x->arena.get(), x->cnt.get(),
                                   x->op.kref, x->op.hash, x->op.slot, old_found, old_fid, old_size);
  k_ix_seq<<<grid, 256, 0, st>>>(n, x->cnt.get(), s.kind == SRC_FLAT, x->slots.get(), x->op.slot, x->seq_base);
  k_ix_commit<<<grid, 256, 0, st>>>(s, n, x->cnt.get(), x->slots.get(), x->arena.get(), x->arena.bytes(), x->op.hash,
                                    x->op.slot);
  k_ix_write<<<grid, 256, 0, st>>>(s, n, x->cnt.get(), v, x->slots.get(), x->op.slot, x->seq_base);
  x->seq_base += n;
  ix_bound(x);
}

Src table_src(bcw_ctx* c, const uint8_t* d_seg, const bcw_decode_params* p, const bcw_record_table* t, int kind) {
  Src s{};
  s.kind = kind;
  s.seg = d_seg;
  s.seg_len = p->seg_len;
  s.frags = c->s.frags.get();
  s.t = *t;
  s.start_off = p->start_off;
  s.ns = p->ns_size;
  return s;
}
// c's latest decode left a fragment table, and the table has the columns every table source reads (need_size: and
// the one the index rebuild takes its values from)
bool table_ok(const bcw_ctx* c, const bcw_record_table* t, bool need_size) {
  return c->s.frags && t->foff && (!need_size || t->size) && t->key_len && t->first_frag && t->emit_frag &&
         t->hdr_size;
}

// doFilter of every row of a decoded table on stream st, counters in cnt: with no rules set the filter without
// rules (k_ix_filter, as it always was), else the rules variant, which counts the rows each rule drops into
// rule_cnt (three device words). A table the rules cannot read is refused.
int ix_launch_filter(bcw_index* x, const Src& s, uint64_t rows, const bcw_decode_result* d_result, uint64_t gen,
                     uint64_t src_fid, uint8_t* d_keep, uint64_t* cnt, uint64_t* rule_cnt, hipStream_t st) {
  if (!rows) return BCW_OK;
  const uint32_t grid = (uint32_t)((rows + 255) / 256);
  if (!x->rules.mask) {
    k_ix_filter<<<grid, 256, 0, st>>>(s, rows, d_result, gen, x->slots.get(), x->cap - 1, x->arena.get(), src_fid,
                                      d_keep, cnt);
    return BCW_OK;
  }
  if (!s.t.expire || !s.t.flags) return BCW_E_INVAL;
  const bool pfx = (x->rules.mask & BCW_RULE_PREFIX) != 0;
  const Rules ru{x->rules.mask, pfx ? x->rules.n_prefix : 0u, pfx ? x->rule_longest : 0u, x->rules.now,
                 x->d_rule_tab.get(), rule_cnt};
  k_ix_filter_rules<<<grid, 256, 0, st>>>(s, rows, d_result, gen, x->slots.get(), x->cap - 1, x->arena.get(), src_fid,
                                          d_keep, cnt, ru);
  return BCW_OK;
}

// The one filter call behind ix_filter_on, ix_filter_pending and bcw_compact_filter_async: c is the context whose
// decode made the table and whose stream runs the filter, cnt the counter block the call counts in (the index's own,
// or a caller's, which first takes a copy of the index's, its overflow flag included), rule_cnt the three words the
// rules count in, zeroed first when the call owns them (zero_rules).
int ix_filter(bcw_index* x, bcw_ctx* c, const uint8_t* d_seg, const bcw_decode_params* p,
              const bcw_record_table* d_table, const bcw_decode_result* d_result, uint64_t src_fid, uint8_t* d_keep,
              uint64_t* cnt, uint64_t* rule_cnt, bool zero_rules, bcw_index_result* d_out) {
  if (!p || !d_table || !d_result || !d_keep || p->mode != BCW_MODE_RECORD || !table_ok(c, d_table, false))
    return BCW_E_INVAL;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  if (cnt != x->cnt.get())
    (void)hipMemcpyAsync(cnt, x->cnt.get(), C_NUM * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
  (void)zero_group(cnt + C_NIN, st);
  if (zero_rules) (void)zero_group(rule_cnt, st);
  const Src s = table_src(c, d_seg, p, d_table, SRC_RECORD);
  const int rc =
      ix_launch_filter(x, s, d_table->capacity, d_result, c->frag_gen, src_fid, d_keep, cnt, rule_cnt, st);
  if (rc != BCW_OK) return rc;
  if (d_out) k_ix_result<<<1, 1, 0, st>>>(cnt, d_out);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

// A usage-shaped pass over the slot table (k_ix_usage, k_ix_drop) on stream st: launch(grid) queues the kernel. The
// buffers are taken as they are now: a batch queued before this call has already grown them.
template <class Launch>
int ix_usage_pass(bcw_index* x, int kid, hipStream_t st, Launch&& launch) {
  if (!x->slots.get() || !x->cap) return BCW_OK;
  bcw_ctx* c = x->ctx;
  const uint64_t wgs = (x->cap + kUsageSlots - 1) / kUsageSlots;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)c->num_cus * 8);
  hipEvent_t ev = nullptr;
  c->prof.begin(kid, st, ev);
  launch(grid);
  c->prof.end(kid, st, ev);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

// The synchronous form of bcw_index_fid_usage_async / bcw_index_drop_fids_async: one device allocation for the
// result and cap rows (carve_usage), async(d_rows, d_res), the result read back, then the rows when they are whole.
// must_fit: rows that are not whole (fits == 0, or an overflow) are BCW_E_CAPACITY; otherwise they are the caller's to
// read.
template <class Async>
int ix_usage_sync(bcw_index* x, bcw_fid_usage* h_rows, uint32_t cap, bcw_usage_result* h_res, bool must_fit,
                  Async&& async) {
  if (!x || !h_res || (cap && !h_rows)) return BCW_E_INVAL;
  bcw_ctx* c = x->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  DevBuf<> mem;
  UsageLayout L;
  int rc = carve_alloc(mem, [&](Carver& cv) { L = carve_usage(cv, cap); });
  if (rc != BCW_OK) return rc;
  rc = async(L.rows, L.res);
  if (rc == BCW_OK &&
      (!copy_down(h_res, L.res, sizeof *h_res, c->cur) || hipStreamSynchronize(c->cur) != hipSuccess))
    rc = BCW_E_HIP;
  const bool whole = rc == BCW_OK && h_res->fits && !h_res->overflow;
  if (rc == BCW_OK && !whole && must_fit) rc = BCW_E_CAPACITY;
  if (whole && (!copy_down(h_rows, L.rows, h_res->n_fids * sizeof(bcw_fid_usage), c->cur) ||
                hipStreamSynchronize(c->cur) != hipSuccess))
    rc = BCW_E_HIP;
  (void)hipStreamSynchronize(c->cur);  // before mem goes
  return rc;
}

}  // namespace

namespace bcw {
int ix_launch_verify_select(bcw_index* x, VerifySelect& v, hipStream_t st) {
  // grow-only: a table that shrank since keeps the queue, and the capacity, of the largest one
  const uint64_t cap = std::max(x->cap, x->vfy_q_cap);
  VfyQueueLayout Q;
  const auto layout = [&](Carver& cv) { Q = carve_vfy_queue(cv, vfy::V_NUM, cap, sizeof(vfy::Item)); };
  const int rc = carve_reserve(x->vfy_q, st, layout);
  x->vfy_q_cap = rc == BCW_OK ? cap : 0;
  if (rc != BCW_OK) return rc;
  v.cnt = Q.cnt;
  v.queue = Q.queue;
  v.queue_cap = cap;
  v.arena = x->arena.get();
  if (hipMemsetAsync(v.cnt, 0, vfy::V_NUM * sizeof *v.cnt, st) != hipSuccess) return BCW_E_HIP;
  const vfy::Sink S{v.out, v.cnt, v.arena};
  return ix_usage_pass(x, K_VFY_SELECT, st, [&](uint32_t grid) {
    k_ix_vfy_select<<<grid, usage::kThreads, 0, st>>>(x->slots.get(), x->cap, v.wals, v.n_wals, S,
                                                      static_cast<vfy::Item*>(v.queue), v.queue_cap, v.scratch);
  });
}

int ix_put_batch(bcw_index* x, const PutIx& p) {
  hipStream_t st = x->ctx->cur;
  if (p.n) {
    const int rc = ix_room(x, p.n, 31 * p.n + p.keys_len);
    if (rc != BCW_OK) return rc;
    Src s{};
    s.kind = SRC_BATCH;
    // every 16-byte granule a key load touches holds a byte of the keys array, whatever the array's alignment
    s.kbias = (uint64_t)((uintptr_t)p.keys & 15u);
    s.keys = p.keys - s.kbias;
    s.koff = p.koff;
    s.keys_len = p.keys_len + s.kbias;
    s.b_nin = p.n_in;
    s.b_off = p.rec_off;
    s.b_size = p.rec_size;
    s.b_flags = p.flags;
    s.b_fid = p.fid;
    const OpVals v{nullptr, nullptr, nullptr, nullptr, 0, 0};
    ix_batch(x, s, p.n, nullptr, 0, v, p.found, p.free_fid, p.free_bytes);
    if (p.found) {
      const uint32_t grid = (uint32_t)((p.n + 255) / 256);
      uint64_t* link = x->op.kref;  // free again once k_ix_claim has run
      k_put_link<<<grid, 256, 0, st>>>(x->cnt.get(), x->slots.get(), x->op.slot, link);
      k_put_stat<<<grid, 256, 0, st>>>(s, x->cnt.get(), x->slots.get(), x->op.slot, link, p.found, p.free_fid,
                                       p.free_bytes);
      k_put_unlink<<<grid, 256, 0, st>>>(x->cnt.get(), x->slots.get(), x->op.slot);
    }
  }
  if (p.idx_err) k_put_idx_err<<<1, 1, 0, st>>>(x->cnt.get(), p.idx_err);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int ix_export(bcw_index* x, const uint64_t* h_fids, uint64_t n_fids, IxSink& sink, uint64_t* n_out,
              uint64_t* key_bytes) {
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = x->ctx->cur;
  std::vector<uint64_t> fids(h_fids, h_fids + n_fids);
  std::sort(fids.begin(), fids.end());
  fids.erase(std::unique(fids.begin(), fids.end()), fids.end());
  if (fids.size() > 0xffffffffull) return BCW_E_INVAL;
  const uint32_t nf = (uint32_t)fids.size();
  const uint64_t nblk = (x->cap + 255) / 256;
  // staging (carve_ix_export): fids | per-block entry counts | per-block key bytes (then their exclusive prefixes) |
  // outputs
  IxExportLayout L;
  const auto stage = [&](uint64_t tn, uint64_t tb) {
    return carve_reserve(x->stage, st, [&](Carver& cv) { L = carve_ix_export(cv, nf, nblk, tn, tb); });
  };
  int rc = stage(0, 0);
  if (rc != BCW_OK) return rc;
  if (!copy_up(L.fids, fids.data(), 8 * (uint64_t)nf, st)) return BCW_E_HIP;
  k_ix_count<<<(uint32_t)nblk, 256, 0, st>>>(x->slots.get(), x->cap, x->arena.get(), L.fids, nf, L.blk_n, L.blk_b);
  std::vector<uint64_t> hn(nblk), hb(nblk);
  if (hipGetLastError() != hipSuccess || !copy_down(hn.data(), L.blk_n, nblk * 8, st) ||
      !copy_down(hb.data(), L.blk_b, nblk * 8, st) || hipStreamSynchronize(st) != hipSuccess)
    return BCW_E_HIP;
  uint64_t tn = 0, tb = 0;
  for (uint64_t b = 0; b < nblk; ++b) {
    const uint64_t a = hn[b], k = hb[b];
    hn[b] = tn;
    hb[b] = tb;
    tn += a;
    tb += k;
  }
  *n_out = tn;
  *key_bytes = tb;
  rc = sink.room(tn, tb);
  if (rc != BCW_OK || tn == 0) return rc;
  rc = stage(tn, tb);  // a regrow drops the contents: the fids go up again, with the prefixes
  if (rc != BCW_OK) return rc;
  bool ok = copy_up(L.fids, fids.data(), 8 * (uint64_t)nf, st) && copy_up(L.blk_n, hn.data(), nblk * 8, st) &&
            copy_up(L.blk_b, hb.data(), nblk * 8, st);
  if (ok)
    k_ix_export<<<(uint32_t)nblk, 256, 0, st>>>(x->slots.get(), x->cap, x->arena.get(), L.fids, nf, L.blk_n, L.blk_b,
                                                  L.k.keys, L.k.key_off, L.fid, L.off, L.size);
  ok = ok && hipGetLastError() == hipSuccess && copy_down(sink.keys, L.k.keys, tb, st) &&
       copy_down(sink.koff, L.k.key_off, 8 * (tn + 1), st) && copy_down(sink.fid, L.fid, 8 * tn, st) &&
       copy_down(sink.off, L.off, 8 * tn, st) && copy_down(sink.size, L.size, 8 * tn, st) &&
       hipStreamSynchronize(st) == hipSuccess;
  return ok ? BCW_OK : BCW_E_HIP;
}

int ix_filter_on(bcw_index* x, bcw_ctx* c, const uint8_t* d_seg, const bcw_decode_params* p,
                 const bcw_record_table* d_table, const bcw_decode_result* d_result, uint64_t src_fid, uint8_t* d_keep,
                 uint64_t* d_cnt, bcw_index_result* d_out) {
  static_assert(C_NUM <= kIxRuleCnt && kIxRuleCnt + 3 <= kIxCounters,
                "the per-call counters hold every index counter and the three rule counts");
  if (!x || !c || !d_cnt || c->device != x->ctx->device) return BCW_E_INVAL;
  // the index's counters, then this call's own zeroed; the rule counts of this call alone
  return ix_filter(x, c, d_seg, p, d_table, d_result, src_fid, d_keep, d_cnt, d_cnt + kIxRuleCnt, x->rules.mask != 0,
                   d_out);
}

bool ix_has_rules(const bcw_index* x) { return x->rules.mask != 0; }

int ix_forward_rules(bcw_index* to, const bcw_index* from) {
  return from->rules.mask ? bcw_index_set_compact_rules(to, &from->rules) : BCW_OK;
}

void ix_add_rule_counts(bcw_index* to, const uint64_t c[3]) {
  for (int r = 0; r < 3; ++r) to->rule_host[r] += c[r];
}

int ix_rule_commit(bcw_index* x) {
  if (!x->rules.mask) return BCW_OK;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  k_ix_rule_commit<<<1, 1, 0, x->ctx->cur>>>(x->d_rule_cnt.get());
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

// bcw_compact_filter_async, with the rows the rules drop counted apart, for ix_rule_commit
int ix_filter_pending(bcw_index* x, const uint8_t* d_seg, const bcw_decode_params* p, const bcw_record_table* d_table,
                      const bcw_decode_result* d_result, uint64_t src_fid, uint8_t* d_keep, bcw_index_result* d_out) {
  if (!x) return BCW_E_INVAL;
  const bool apart = x->rules.mask != 0;  // rule counters [3, 6): the compaction in progress
  return ix_filter(x, x->ctx, d_seg, p, d_table, d_result, src_fid, d_keep, x->cnt.get(),
                   x->d_rule_cnt.get() + (apart ? 3 : 0), apart, d_out);
}
}  // namespace bcw

extern "C" {

int bcw_index_create(bcw_ctx* c, uint64_t keys, uint64_t arena_bytes, bcw_index** out) {
  if (!c || !out) return BCW_E_INVAL;
  *out = nullptr;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  bcw_index* x = new (std::nothrow) bcw_index();
  if (!x) return BCW_E_NOMEM;
  x->ctx = c;
  const bool ok = x->cnt.alloc(C_NUM * sizeof(uint64_t)) &&
                  hipMemsetAsync(x->cnt.get(), 0, C_NUM * sizeof(uint64_t), c->cur) == hipSuccess;
  const int rc =
      ok ? ix_grow(x, std::max<uint64_t>(keys, 1024), std::max<uint64_t>(arena_bytes, 1 << 20)) : BCW_E_NOMEM;
  if (rc != BCW_OK) bcw_index_destroy(x);  // whatever it holds by now goes with it
  else *out = x;
  return rc;
}

int bcw_index_destroy(bcw_index* x) {
  if (!x) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  (void)hipStreamSynchronize(x->ctx->cur);
  if (x->drop_h) (void)hipHostFree(x->drop_h);
  if (x->drop_ev) (void)hipEventDestroy(x->drop_ev);
  if (x->scan_h) (void)hipHostFree(x->scan_h);
  if (x->scan_ev) (void)hipEventDestroy(x->scan_ev);
  delete x;  // the device buffers go here (DevBuf), on the index's device: inside dg's scope
  return BCW_OK;
}

int bcw_index_reserve(bcw_index* x, uint64_t keys, uint64_t arena_bytes) {
  if (!x) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  uint64_t c[C_NUM];
  int rc = ix_sync_counters(x, c);
  if (rc != BCW_OK) return rc;
  ix_refresh_bounds(x, c);
  return ix_grow(x, std::max(keys, x->slots_ub), std::max(arena_bytes, x->arena_ub));
}

int bcw_index_stats(bcw_index* x, bcw_index_info* out) {
  if (!x || !out) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  uint64_t c[C_NUM];
  const int rc = ix_sync_counters(x, c);
  if (rc != BCW_OK) return rc;
  out->live = c[C_LIVE];
  out->slots_used = c[C_SLOTS];
  out->slot_capacity = x->cap;
  out->arena_used = c[C_ARENA];
  out->arena_capacity = x->arena.bytes();
  out->overflow = c[C_OVERFLOW];
  out->limited = x->limited;
  out->evicted = c[C_EVICTED];
  out->evicted_bytes = c[C_EVICTED_BYTES];
  return BCW_OK;
}

int bcw_index_set_limit(bcw_index* x, uint64_t limited) {
  if (!x || (limited != 0 && limited < 16)) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  x->limited = limited;
  ix_bound(x);  // an index already past the new bound is brought within it at once
  return hipGetLastError() == hipSuccess && hipStreamSynchronize(x->ctx->cur) == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_index_compact(bcw_index* x, int shrink) {
  if (!x) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = x->ctx->cur;
  uint64_t ncap = x->cap, narena = x->arena.bytes();
  if (shrink && hipMemsetAsync(x->cnt.get() + C_R_ARENA, 0, sizeof(uint64_t), st) != hipSuccess) return BCW_E_HIP;
  if (shrink) {
    hipEvent_t ev = nullptr;
    x->ctx->prof.begin(K_IX_LIVE_BYTES, st, ev);
    k_ix_live_bytes<<<(uint32_t)((x->cap + 255) / 256), 256, 0, st>>>(x->slots.get(), x->cap, x->arena.get(),
                                                                      x->arena.bytes(), x->cnt.get() + C_R_ARENA);
    x->ctx->prof.end(K_IX_LIVE_BYTES, st, ev);
  }
  uint64_t c[C_NUM];
  const int rc = hipGetLastError() == hipSuccess ? ix_sync_counters(x, c) : BCW_E_HIP;
  if (rc != BCW_OK) return rc;
  if (c[C_OVERFLOW]) return BCW_E_CAPACITY;  // the index is inconsistent
  if (shrink) {
    ncap = std::min(ncap, pow2_at_least((uint64_t)((double)c[C_LIVE] / kMaxLoad) + 1));
    narena = std::min(narena, std::max<uint64_t>(c[C_R_ARENA], 1 << 20));
  }
  return ix_compact(x, ncap, narena);
}

int bcw_index_apply_stat(bcw_index* x, uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off,
                         const uint8_t* h_ops, const uint64_t* h_fid, const uint64_t* h_off, const uint64_t* h_size,
                         uint8_t* h_found, uint64_t* h_free_fid, uint64_t* h_free_bytes) {
  if (!x || (n && (!h_key_off || !h_ops || !h_fid || !h_off || !h_size))) return BCW_E_INVAL;
  const bool stat = h_found || h_free_fid || h_free_bytes;
  if (stat && !(h_found && h_free_fid && h_free_bytes)) return BCW_E_INVAL;
  if (n == 0) return BCW_OK;
  int rc = flat_keys_ok(n, h_keys, h_key_off);
  if (rc != BCW_OK) return rc;
  for (uint64_t i = 0; i < n; ++i)
    if (h_ops[i] > BCW_IDX_SOFT_DELETE) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  const uint64_t arena_b = 16 * n + (h_key_off[n] - h_key_off[0]) + 15 * n;
  rc = ix_room(x, n, arena_b);
  if (rc != BCW_OK) return rc;
  IxApplyLayout L;
  std::vector<uint64_t> koff;
  rc = stage_flat_keys(x, n, h_keys, h_key_off, carve_ix_apply, &L, &koff);
  if (rc != BCW_OK) return rc;
  hipStream_t st = x->ctx->cur;
  bool ok = copy_up(L.fid, h_fid, 8 * n, st) && copy_up(L.off, h_off, 8 * n, st) &&
            copy_up(L.size, h_size, 8 * n, st) && copy_up(L.ops, h_ops, n, st);
  if (!ok) return BCW_E_HIP;
  OpVals v{L.ops, L.fid, L.off, L.size, 0, 0};
  ix_batch(x, flat_src(L.k.keys, L.k.key_off, koff[n]), n, nullptr, 0, v, stat ? L.found : nullptr, L.free_fid,
           L.free_bytes);
  if (stat)
    ok = copy_down(h_found, L.found, n, st) && copy_down(h_free_fid, L.free_fid, 8 * n, st) &&
         copy_down(h_free_bytes, L.free_bytes, 8 * n, st);
  if (!ok || hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return BCW_E_HIP;
  if (stat) {
    // the device reported, per op, the value the key held before the batch; an op preceded by another op on the
    // same key in this batch replaces that op's value instead (Put: its fid / size, SoftDelete: IndexValue{} with
    // fid 0 / size 0, Delete: nothing -- index.go:108-165)
    std::unordered_map<std::string_view, uint64_t> last;
    last.reserve(n * 2);
    const char* kbase = reinterpret_cast<const char*>(h_keys);
    for (uint64_t i = 0; i < n; ++i) {
      const std::string_view key(kbase ? kbase + h_key_off[i] : "", h_key_off[i + 1] - h_key_off[i]);
      auto it = last.find(key);
      if (it != last.end()) {
        const uint64_t p = it->second;
        h_found[i] = h_ops[p] != BCW_IDX_DELETE;
        h_free_fid[i] = h_ops[p] == BCW_IDX_PUT ? h_fid[p] : 0;
        h_free_bytes[i] = h_ops[p] == BCW_IDX_PUT ? h_size[p] : 0;
        it->second = i;
      } else {
        last.emplace(key, i);
      }
      if (!h_found[i]) h_free_fid[i] = h_free_bytes[i] = 0;
    }
  }
  uint64_t c[C_NUM];
  rc = ix_sync_counters(x, c);
  if (rc != BCW_OK) return rc;
  return c[C_OVERFLOW] ? BCW_E_CAPACITY : BCW_OK;
}

int bcw_index_apply(bcw_index* x, uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off, const uint8_t* h_ops,
                    const uint64_t* h_fid, const uint64_t* h_off, const uint64_t* h_size) {
  return bcw_index_apply_stat(x, n, h_keys, h_key_off, h_ops, h_fid, h_off, h_size, nullptr, nullptr, nullptr);
}

int bcw_index_clear(bcw_index* x) {
  if (!x) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = x->ctx->cur;
  if (hipMemsetAsync(x->slots.get(), 0, x->cap * sizeof(Slot), st) != hipSuccess ||
      hipMemsetAsync(x->cnt.get(), 0, C_NUM * sizeof(uint64_t), st) != hipSuccess)
    return BCW_E_HIP;
  x->slots_ub = 0;
  x->arena_ub = 0;
  return BCW_OK;
}

int bcw_index_get(bcw_index* x, uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off, uint64_t* h_fid,
                  uint64_t* h_off, uint64_t* h_size, uint8_t* h_status) {
  if (!x || (n && (!h_key_off || !h_fid || !h_off || !h_size || !h_status))) return BCW_E_INVAL;
  if (n == 0) return BCW_OK;
  int rc = flat_keys_ok(n, h_keys, h_key_off);
  if (rc != BCW_OK) return rc;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  IxGetLayout L;
  std::vector<uint64_t> koff;
  rc = stage_flat_keys(x, n, h_keys, h_key_off, carve_ix_get, &L, &koff);
  if (rc != BCW_OK) return rc;
  hipStream_t st = x->ctx->cur;
  k_ix_get<<<(uint32_t)((n + 255) / 256), 256, 0, st>>>(flat_src(L.k.keys, L.k.key_off, koff[n]), n, x->slots.get(),
                                                         x->cap - 1, x->arena.get(), L.fid, L.off, L.size, L.status);
  const bool ok = hipGetLastError() == hipSuccess && copy_down(h_fid, L.fid, 8 * n, st) &&
                  copy_down(h_off, L.off, 8 * n, st) && copy_down(h_size, L.size, 8 * n, st) &&
                  copy_down(h_status, L.status, n, st) && hipStreamSynchronize(st) == hipSuccess;
  return ok ? BCW_OK : BCW_E_HIP;
}

int bcw_index_put_decoded_async(bcw_index* x, const uint8_t* d_seg, const bcw_decode_params* p,
                                const bcw_record_table* d_table, const bcw_decode_result* d_result, uint64_t fid,
                                int use_record_fid, bcw_index_result* d_out) {
  if (!x || !p || !d_table || !d_result) return BCW_E_INVAL;
  if (p->mode != BCW_MODE_RECORD && p->mode != BCW_MODE_HINT) return BCW_E_INVAL;
  bcw_ctx* c = x->ctx;
  if (!table_ok(c, d_table, true)) return BCW_E_INVAL;
  if (p->mode == BCW_MODE_HINT && (!d_table->aux0 || !d_table->aux1 || !d_table->expire)) return BCW_E_INVAL;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  const uint64_t rows = d_table->capacity;
  const Src s = table_src(c, d_seg, p, d_table, p->mode == BCW_MODE_RECORD ? SRC_RECORD : SRC_HINT);
  // arena bound: a merged key is at most its record's payload (ns + key <= size), all payloads fit the segment.
  // When that cheap bound does not fit the arena (a large segment), the exact need of the delivered rows is
  // read back instead (one small launch and a sync): only keys new to the index take arena space, so an
  // index rebuilt over keys it already holds does not grow.
  uint64_t arena_b = p->seg_len + 32 * rows;
  if (x->arena_ub + arena_b > x->arena.bytes() && rows) {
    if (hipMemsetAsync(x->cnt.get() + C_NEED, 0, sizeof(uint64_t), c->cur) != hipSuccess) return BCW_E_HIP;
    k_ix_need<<<(uint32_t)((rows + 255) / 256), 256, 0, c->cur>>>(s, rows, d_result, c->frag_gen, x->cnt.get());
    uint64_t cc[C_NUM];
    int rc0 = ix_sync_counters(x, cc);
    if (rc0 != BCW_OK) return rc0;
    if (cc[C_OVERFLOW]) return BCW_E_CAPACITY;
    ix_refresh_bounds(x, cc);
    arena_b = cc[C_NEED];
  }
  int rc = ix_room(x, rows, arena_b);
  if (rc != BCW_OK) return rc;
  OpVals v{nullptr, nullptr, nullptr, nullptr, fid, use_record_fid};
  ix_batch(x, s, rows, d_result, c->frag_gen, v);
  if (d_out) k_ix_result<<<1, 1, 0, c->cur>>>(x->cnt.get(), d_out);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_compact_filter_async(bcw_index* x, const uint8_t* d_seg, const bcw_decode_params* p,
                             const bcw_record_table* d_table, const bcw_decode_result* d_result, uint64_t src_fid,
                             uint8_t* d_keep, bcw_index_result* d_out) {
  if (!x) return BCW_E_INVAL;
  return ix_filter(x, x->ctx, d_seg, p, d_table, d_result, src_fid, d_keep, x->cnt.get(), x->d_rule_cnt.get(), false,
                   d_out);
}

int bcw_index_set_compact_rules(bcw_index* x, const bcw_compact_rules* r) {
  if (!x || rules::validate(r) != BCW_OK) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = x->ctx->cur;
  const bool on = r && r->mask;
  if (on && !x->d_rule_tab) {
    DevBuf<rules::PrefixTable> t;
    DevBuf<uint64_t> cnt;
    if (!t.alloc(sizeof(rules::PrefixTable)) || !cnt.alloc(6 * sizeof(uint64_t))) return BCW_E_NOMEM;
    x->d_rule_tab = std::move(t);
    x->d_rule_cnt = std::move(cnt);
  }
  // the copy of the caller's arrays, made before anything of the index changes
  std::vector<uint8_t> bytes;
  std::vector<uint32_t> off(1, 0u);
  rules::PrefixTable tab;
  uint32_t longest = 0;
  if (on) {
    for (uint32_t i = 0; i < r->n_prefix; ++i) {
      bytes.insert(bytes.end(), r->prefixes + r->prefix_off[i], r->prefixes + r->prefix_off[i + 1]);
      off.push_back((uint32_t)bytes.size());
    }
    longest = rules::pack(*r, &tab);
    // ordered on the stream after the filters queued so far; the sync below keeps `tab` alive for the copy
    if (hipMemcpyAsync(x->d_rule_tab.get(), &tab, sizeof tab, hipMemcpyHostToDevice, st) != hipSuccess)
      return BCW_E_HIP;
  }
  if (x->d_rule_cnt && hipMemsetAsync(x->d_rule_cnt.get(), 0, 6 * sizeof(uint64_t), st) != hipSuccess) return BCW_E_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return BCW_E_HIP;
  x->rule_bytes.swap(bytes);
  x->rule_off.swap(off);
  x->rules = bcw_compact_rules{};
  if (on) {
    x->rules.mask = r->mask;
    x->rules.n_prefix = r->n_prefix;
    x->rules.now = r->now;
    x->rules.prefixes = x->rule_bytes.data();
    x->rules.prefix_off = x->rule_off.data();
  }
  x->rule_longest = longest;
  x->rule_host[0] = x->rule_host[1] = x->rule_host[2] = 0;
  return BCW_OK;
}

int bcw_index_compact_rule_counts(bcw_index* x, uint64_t out[3]) {
  if (!x || !out) return BCW_E_INVAL;
  DeviceGuard dg(x->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = x->ctx->cur;
  uint64_t c[3] = {0, 0, 0};
  if (x->d_rule_cnt && hipMemcpyAsync(c, x->d_rule_cnt.get(), sizeof c, hipMemcpyDeviceToHost, st) != hipSuccess)
    return BCW_E_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return BCW_E_HIP;
  for (int r = 0; r < 3; ++r) out[r] = c[r] + x->rule_host[r];
  return BCW_OK;
}

int bcw_index_export(bcw_index* x, uint8_t* h_keys, uint64_t keys_cap, uint64_t* h_key_off, uint64_t* h_fid,
                     uint64_t* h_off, uint64_t* h_size, uint64_t entries_cap, uint64_t* n_out, uint64_t* key_bytes) {
  return bcw_index_export_fids(x, nullptr, 0, h_keys, keys_cap, h_key_off, h_fid, h_off, h_size, entries_cap, n_out,
                               key_bytes);
}

int bcw_index_export_fids(bcw_index* x, const uint64_t* h_fids, uint64_t n_fids, uint8_t* h_keys, uint64_t keys_cap,
                          uint64_t* h_key_off, uint64_t* h_fid, uint64_t* h_off, uint64_t* h_size,
                          uint64_t entries_cap, uint64_t* n_out, uint64_t* key_bytes) {
  if (!x || !n_out || !key_bytes || (n_fids && !h_fids)) return BCW_E_INVAL;
  struct Fixed : IxSink {
    uint64_t ecap, kcap;
    int room(uint64_t n, uint64_t kb) override {
      if (n > ecap || kb > kcap) return BCW_E_CAPACITY;
      return n == 0 || (keys && koff && fid && off && size) ? BCW_OK : BCW_E_INVAL;
    }
  } sink;
  sink.ecap = entries_cap;
  sink.kcap = keys_cap;
  sink.keys = h_keys;
  sink.koff = h_key_off;
  sink.fid = h_fid;
  sink.off = h_off;
  sink.size = h_size;
  const int rc = ix_export(x, h_fids, n_fids, sink, n_out, key_bytes);
  if (rc == BCW_OK && *n_out == 0 && h_key_off) h_key_off[0] = 0;
  return rc;
}

int bcw_index_fid_usage_async(bcw_index* x, bcw_fid_usage* d_rows, uint32_t cap, bcw_usage_result* d_res) {
  if (!x || !d_res || (cap && !d_rows)) return BCW_E_INVAL;
  bcw_ctx* c = x->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  uint64_t* scratch = nullptr;
  const int rc = usage_begin(c, st, &scratch);
  if (rc != BCW_OK) return rc;
  const int rp = ix_usage_pass(x, K_USAGE_INDEX, st, [&](uint32_t grid) {
    k_ix_usage<<<grid, usage::kThreads, 0, st>>>(x->slots.get(), x->cap, scratch);
  });
  return rp != BCW_OK ? rp : usage_finish(c, st, d_rows, cap, d_res, 1);
}

int bcw_index_fid_usage(bcw_index* x, bcw_fid_usage* h_rows, uint32_t cap, bcw_usage_result* h_res) {
  return ix_usage_sync(x, h_rows, cap, h_res, true, [&](bcw_fid_usage* d_rows, bcw_usage_result* d_res) {
    return bcw_index_fid_usage_async(x, d_rows, cap, d_res);
  });
}

int bcw_index_drop_fids_async(bcw_index* x, int mode, const uint64_t* h_fids, uint32_t n_fids, bcw_fid_usage* d_rows,
                              uint32_t cap, bcw_usage_result* d_res) {
  if (!x || !d_res || (cap && !d_rows)) return BCW_E_INVAL;
  std::vector<uint64_t> fids;
  int rc = drop::normalise(mode, h_fids, n_fids, &fids);  // nothing has touched the index or the stream yet
  if (rc != BCW_OK) return rc;
  const uint32_t nf = (uint32_t)fids.size();
  bcw_ctx* c = x->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  if (!x->drop_d) {
    const size_t bytes = (size_t)BCW_USAGE_MAX_FIDS * sizeof(uint64_t);
    // the list alone can pass 64 KiB of LDS per workgroup together with the kernel's static 32 KiB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ix_drop), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
    (void)hipGetLastError();
    if (!x->drop_d.alloc(bytes)) return BCW_E_NOMEM;
    if (hipHostMalloc(&x->drop_h, bytes, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&x->drop_ev, hipEventDisableTiming) != hipSuccess) {
      if (x->drop_h) (void)hipHostFree(x->drop_h);
      x->drop_d.reset();
      x->drop_h = nullptr;
      x->drop_ev = nullptr;
      return BCW_E_NOMEM;
    }
  } else if (hipEventSynchronize(x->drop_ev) != hipSuccess) {  // the previous call's copy has read the pinned list
    return BCW_E_HIP;
  }
  if (nf) {
    memcpy(x->drop_h, fids.data(), (size_t)nf * sizeof(uint64_t));
    if (hipMemcpyAsync(x->drop_d.get(), x->drop_h, (size_t)nf * sizeof(uint64_t), hipMemcpyHostToDevice, st) !=
        hipSuccess)
      return BCW_E_HIP;
  }
  if (hipEventRecord(x->drop_ev, st) != hipSuccess) return BCW_E_HIP;
  uint64_t* scratch = nullptr;
  rc = usage_begin(c, st, &scratch);
  if (rc != BCW_OK) return rc;
  rc = ix_usage_pass(x, K_IX_DROP, st, [&](uint32_t grid) {
    k_ix_drop<<<grid, usage::kThreads, (size_t)nf * sizeof(uint64_t), st>>>(x->slots.get(), x->cap, x->drop_d.get(), nf,
                                                                           mode, scratch, x->cnt.get());
  });
  return rc != BCW_OK ? rc : usage_finish(c, st, d_rows, cap, d_res, 1);
}

int bcw_index_drop_fids(bcw_index* x, int mode, const uint64_t* h_fids, uint32_t n_fids, bcw_fid_usage* h_rows,
                        uint32_t cap, bcw_usage_result* h_res) {
  // fits == 0 and overflow are the caller's to read: the drop has happened either way
  return ix_usage_sync(x, h_rows, cap, h_res, false, [&](bcw_fid_usage* d_rows, bcw_usage_result* d_res) {
    return bcw_index_drop_fids_async(x, mode, h_fids, n_fids, d_rows, cap, d_res);
  });
}

int bcw_index_scan_async(bcw_index* x, const bcw_scan_params* p, const bcw_scan_out* d_out, bcw_scan_result* d_res) {
  if (!x || !d_res || scan::validate(p, d_out) != BCW_OK) return BCW_E_INVAL;  // nothing has touched the stream yet
  bcw_ctx* c = x->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  // grow-only: a table that shrank since keeps the scratch, and the capacity, of the largest one
  const uint64_t cap = std::max(x->cap, x->scan_cap);
  IxScanLayout L;
  const auto layout = [&](Carver& cv) {
    L = carve_ix_scan(cv, sizeof(rules::PrefixTable), scan::kAccWords, scan::tiles(cap), cap);
  };
  int rc = carve_reserve(x->scan_mem, st, layout);
  x->scan_cap = rc == BCW_OK ? cap : 0;
  if (rc != BCW_OK) return rc;
  if (!x->scan_h) {
    if (hipHostMalloc(reinterpret_cast<void**>(&x->scan_h), sizeof(rules::PrefixTable), hipHostMallocDefault) !=
            hipSuccess ||
        hipEventCreateWithFlags(&x->scan_ev, hipEventDisableTiming) != hipSuccess) {
      if (x->scan_h) (void)hipHostFree(x->scan_h);
      (void)hipGetLastError();
      x->scan_h = nullptr;
      x->scan_ev = nullptr;
      return BCW_E_NOMEM;
    }
  } else if (hipEventSynchronize(x->scan_ev) != hipSuccess) {  // the previous call's copy has read the pinned table
    return BCW_E_HIP;
  }
  ScanArgs A{};
  A.table = static_cast<const rules::PrefixTable*>(L.table);
  A.n_prefix = p->n_prefix;
  A.flags = p->flags;
  A.verdict = L.verdict;
  A.tile_n = L.tile_n;
  A.tile_b = L.tile_b;
  A.acc = L.acc;
  if (p->n_prefix) {
    A.longest = scan::pack(*p, x->scan_h);
    if (hipMemcpyAsync(L.table, x->scan_h, sizeof(rules::PrefixTable), hipMemcpyHostToDevice, st) != hipSuccess)
      return BCW_E_HIP;
  }
  if (hipEventRecord(x->scan_ev, st) != hipSuccess ||
      hipMemsetAsync(L.acc, 0, scan::kAccWords * sizeof *L.acc, st) != hipSuccess)
    return BCW_E_HIP;
  // the buffers are taken as they are now: a batch queued before this call has already grown them
  const uint64_t tiles = scan::tiles(x->cap);
  const uint32_t wgs = (uint32_t)std::min<uint64_t>(tiles, 0x7fffffffull);
  hipEvent_t ev = nullptr;
  c->prof.begin(K_SCAN_SELECT, st, ev);
  k_ix_scan_select<<<std::min(wgs, (uint32_t)c->num_cus * kScanSelectPerCu), usage::kThreads, 0, st>>>(
      x->slots.get(), x->cap, x->arena.get(), x->arena.bytes(), A);
  c->prof.end(K_SCAN_SELECT, st, ev);
  c->prof.begin(K_SCAN_OFFSETS, st, ev);
  k_ix_scan_offsets<<<1, kScanOffsetsThreads, 0, st>>>(L.tile_n, L.tile_b, tiles, L.acc,
                                                        scan::group_rows(p->n_prefix), *d_out, d_res);
  c->prof.end(K_SCAN_OFFSETS, st, ev);
  c->prof.begin(K_SCAN_EMIT, st, ev);
  k_ix_scan_emit<<<std::min(wgs, (uint32_t)c->num_cus * kScanEmitPerCu), scan::kTileSlots, 0, st>>>(
      x->slots.get(), x->cap, x->arena.get(), L.verdict, L.tile_n, L.tile_b, tiles, *d_out, d_res);
  c->prof.end(K_SCAN_EMIT, st, ev);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_index_scan(bcw_index* x, const bcw_scan_params* p, const bcw_scan_out* h_out, bcw_scan_result* h_res) {
  if (!x || !h_res || scan::validate(p, h_out) != BCW_OK) return BCW_E_INVAL;
  const bcw_scan_out& h = *h_out;
  bcw_ctx* c = x->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  const uint32_t rows = scan::group_rows(p->n_prefix);
  DevBuf<> mem;
  bcw_scan_out d{};
  bcw_scan_result* d_res = nullptr;
  if (const int rc = carve_alloc(mem, [&](Carver& cv) {
        d_res = cv.take<bcw_scan_result>(1, 16);
        d.groups = h.groups ? cv.take<bcw_scan_group>(rows, 16) : nullptr;
        d.keys = h.keys ? cv.take_bytes16(h.keys_cap) : nullptr;
        d.key_off = h.key_off ? cv.take<uint64_t>(h.entries_cap + 1) : nullptr;
        d.fid = h.fid ? cv.take<uint64_t>(h.entries_cap) : nullptr;
        d.off = h.off ? cv.take<uint64_t>(h.entries_cap) : nullptr;
        d.size = h.size ? cv.take<uint64_t>(h.entries_cap) : nullptr;
        d.prefix_id = h.prefix_id ? cv.take<uint8_t>(h.entries_cap) : nullptr;
        cv.take<uint8_t>(kTailSlack);
      }))
    return rc;
  d.keys_cap = h.keys ? h.keys_cap : 0;
  d.entries_cap = h.entries_cap;
  int rc = bcw_index_scan_async(x, p, &d, d_res);
  if (rc == BCW_OK)
    rc = copy_down(h_res, d_res, sizeof *h_res, st) && copy_down(h.groups, d.groups, rows * sizeof(bcw_scan_group), st) &&
                 hipStreamSynchronize(st) == hipSuccess
             ? BCW_OK
             : BCW_E_HIP;
  if (rc == BCW_OK && !h_res->fits) rc = BCW_E_CAPACITY;
  if (rc == BCW_OK) {
    const uint64_t n = h_res->n_listed;
    const bool ok = copy_down(h.keys, d.keys, h_res->key_bytes, st) &&
                    copy_down(h.key_off, d.key_off, 8 * (n + 1), st) && copy_down(h.fid, d.fid, 8 * n, st) &&
                    copy_down(h.off, d.off, 8 * n, st) && copy_down(h.size, d.size, 8 * n, st) &&
                    copy_down(h.prefix_id, d.prefix_id, n, st) && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) rc = BCW_E_HIP;
  }
  (void)hipStreamSynchronize(st);  // before mem goes
  return rc;
}

// the hash of the index (bcw_murmur.h: the text the kernels compile), over a byte pointer
uint64_t bcw_murmur3_sum64(const uint8_t* p, uint64_t n) { return murmur::sum64(p, n); }

}  // extern "C"
