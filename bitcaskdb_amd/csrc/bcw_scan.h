// bcw_scan.h -- the scan of the device index by key prefix (bcw_index_scan*, bcw.h): which live entries a call lists,
// the group each one counts in, what it adds to that group's row, and when the outputs are whole.
// Plain inline functions shared by the host (argument check, packing the prefix table), the kernels (bcw_index.hip:
// k_ix_scan_select decides with scan::decide, k_ix_scan_offsets with scan::fits; all three use the tile arithmetic)
// and the stand-alone host check (tools/scan_check.cpp): one text, compiled by all three, as bcw_rules.h is -- whose
// prefix validation, packed table and chunked match this header takes over rather than restating. No device calls here.
#pragma once
#include <cstdint>

#include "bcw.h"
#include "bcw_rules.h"

#if defined(__HIPCC__)
#define BCW_SCAN_FN __host__ __device__ __forceinline__
#else
#define BCW_SCAN_FN inline
#endif

namespace bcw {
namespace scan {

constexpr uint32_t kKnownFlags = BCW_SCAN_SOFT_DELETED;

// ---- the tile arithmetic: a tile is the 256 slots one workgroup round takes (usage_round) ----
constexpr uint32_t kTileSlots = 256;
BCW_SCAN_FN uint64_t tiles(uint64_t slots) { return (slots + kTileSlots - 1) / kTileSlots; }
BCW_SCAN_FN uint64_t tile_of(uint64_t slot) { return slot / kTileSlots; }
BCW_SCAN_FN uint64_t tile_base(uint64_t tile) { return tile * kTileSlots; }

// ---- the group rows: bcw_scan_group as four words, BCW_RULE_MAX_PREFIXES rows, then the live entries the pass saw ----
enum { G_COUNT = 0, G_BYTES = 1, G_KEY_BYTES = 2, G_SOFT = 3, G_WORDS = 4 };
static_assert(sizeof(bcw_scan_group) == G_WORDS * sizeof(uint64_t), "bcw_scan_group is four words");
constexpr uint32_t kGroupWords = BCW_RULE_MAX_PREFIXES * G_WORDS;
constexpr uint32_t kLiveWord = kGroupWords;  // the word behind the rows
constexpr uint32_t kAccWords = kGroupWords + 1;
BCW_SCAN_FN uint32_t group_rows(uint32_t n_prefix) { return n_prefix ? n_prefix : 1u; }

// ---- arguments ----
// the prefixes of a scan as the rules header takes them: validated and packed by its text
inline bcw_compact_rules as_rules(const bcw_scan_params& p) {
  bcw_compact_rules r{};
  r.mask = BCW_RULE_PREFIX;
  r.n_prefix = p.n_prefix;
  r.prefixes = p.prefixes;
  r.prefix_off = p.prefix_off;
  return r;
}

// bcw_index_scan*'s argument check: an unknown flag; more than 64 prefixes, an empty or too long one, offsets that
// descend, a NULL array with n_prefix > 0 (rules::validate); room for entries with nowhere to put their keys
inline int validate(const bcw_scan_params* p, const bcw_scan_out* o) {
  if (!p || !o) return BCW_E_INVAL;
  if (p->flags & ~kKnownFlags) return BCW_E_INVAL;
  const bcw_compact_rules r = as_rules(*p);
  if (rules::validate(&r) != BCW_OK) return BCW_E_INVAL;
  if (o->entries_cap > 0 && (!o->keys || !o->key_off)) return BCW_E_INVAL;
  return BCW_OK;
}

// the prefixes of validated parameters, packed; returns the longest prefix (0: none)
inline uint32_t pack(const bcw_scan_params& p, rules::PrefixTable* t) { return rules::pack(as_rules(p), t); }

// ---- the rule ----
constexpr uint32_t kNoGroup = 0xffffffffu;

// the first prefix, in the order given, the merged key starts with (BCW_RULE_PREFIX's rule: a prefix longer than the
// key never matches); n_prefix == 0: every key, group 0. kw: as rules::starts_with takes it
BCW_SCAN_FN uint32_t first_group(const uint32_t* kw, uint32_t key_len, const uint32_t (*pw)[rules::kPrefixWords],
                                 const uint32_t* plen, uint32_t n_prefix) {
  if (n_prefix == 0) return 0;
  for (uint32_t i = 0; i < n_prefix; ++i)
    if (rules::starts_with(kw, key_len, pw[i], plen[i])) return i;
  return kNoGroup;
}

// What one slot is to a scan. A slot that is not live is nothing. A live entry matches when its key is under a prefix;
// a matching entry with off != 0 is listed and adds {1, size, key_len} to its group's {count, bytes, key_bytes}
// (0 < off < 40 included: Get finds those too); one with off == 0 is a SoftDelete, adds 1 to soft_deleted and is
// listed only with BCW_SCAN_SOFT_DELETED (its group's count, bytes and key_bytes stay as they are).
struct Hit {
  bool match, listed, soft;
  uint32_t group;               // valid when match
  uint64_t bytes, key_bytes;    // what the entry adds to its group's row (count: match && !soft)
};

BCW_SCAN_FN Hit decide(bool live, uint64_t off, uint64_t size, const uint32_t* kw, uint32_t key_len,
                       const uint32_t (*pw)[rules::kPrefixWords], const uint32_t* plen, uint32_t n_prefix,
                       uint32_t flags) {
  Hit h{};
  if (!live) return h;
  const uint32_t g = first_group(kw, key_len, pw, plen, n_prefix);
  if (g == kNoGroup) return h;
  h.match = true;
  h.group = g;
  h.soft = off == 0;
  h.listed = !h.soft || (flags & BCW_SCAN_SOFT_DELETED) != 0;
  h.bytes = h.soft ? 0 : size;
  h.key_bytes = h.soft ? 0 : key_len;
  return h;
}

// the verdict byte of a slot: 0 not listed, 1 + group (group < 64)
BCW_SCAN_FN uint32_t verdict_of(const Hit& h) { return h.listed ? 1u + h.group : 0u; }
BCW_SCAN_FN uint32_t verdict_group(uint32_t verdict) { return verdict - 1u; }

// the keys, the offsets and the columns are whole only when both the entries and the key bytes had room
BCW_SCAN_FN bool fits(uint64_t n_listed, uint64_t entries_cap, uint64_t key_bytes, uint64_t keys_cap) {
  return n_listed <= entries_cap && key_bytes <= keys_cap;
}

}  // namespace scan
}  // namespace bcw
