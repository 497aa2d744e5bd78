// bcw_rules.h -- the compaction filter rules (bcw_compact_rules, bcw.h): the pure predicates a user CompactionFilter
// (doFilter, compaction.go:339-345) nearly always is, evaluated on the device for rows that passed the index check.
// Plain inline functions shared by the host (validation, packing the prefix table), the filter kernel
// (bcw_index.hip, k_ix_filter<true>) and the stand-alone host check (tools/rules_check.cpp): one text, compiled by
// all three. No device calls here.
#pragma once
#include <cstdint>
#include <cstring>

#include "bcw.h"

#if defined(__HIPCC__)
#define BCW_RULES_FN __host__ __device__ __forceinline__
#else
#define BCW_RULES_FN inline
#endif

namespace bcw {
namespace rules {

constexpr uint32_t kKnown = BCW_RULE_EXPIRED | BCW_RULE_TOMBSTONE | BCW_RULE_PREFIX;
constexpr uint32_t kTombstone = 1u << 2;                         // tombstoneFieldBit (record.go:44-48)
constexpr uint32_t kPrefixWords = BCW_RULE_MAX_PREFIX_LEN / 4;   // a prefix as little-endian words, zero padded
constexpr uint32_t kKeyChunks = BCW_RULE_MAX_PREFIX_LEN / 16;    // 16 B chunks of a merged key a prefix can reach

// the rule that dropped a row; the values are the order the rules are tried in, and 1 + the counter's index
enum { kNone = 0, kExpired = 1, kTombstoneHit = 2, kPrefix = 3 };

// The prefix table as the kernel reads it: prefix i is w[i] (zero beyond len[i] bytes).
struct PrefixTable {
  uint32_t w[BCW_RULE_MAX_PREFIXES][kPrefixWords];
  uint32_t len[BCW_RULE_MAX_PREFIXES];
};

// bcw_index_set_compact_rules' argument check. NULL or mask == 0 clears the rules, whatever else the struct says.
inline int validate(const bcw_compact_rules* r) {
  if (!r || r->mask == 0) return BCW_OK;
  if (r->mask & ~kKnown) return BCW_E_INVAL;
  if (r->n_prefix > BCW_RULE_MAX_PREFIXES) return BCW_E_INVAL;
  if (r->n_prefix == 0) return BCW_OK;  // BCW_RULE_PREFIX with no prefix matches nothing
  if (!r->prefixes || !r->prefix_off) return BCW_E_INVAL;
  for (uint32_t i = 0; i < r->n_prefix; ++i) {
    const uint32_t a = r->prefix_off[i], b = r->prefix_off[i + 1];
    if (b <= a || b - a > BCW_RULE_MAX_PREFIX_LEN) return BCW_E_INVAL;  // descending, empty or too long
  }
  return BCW_OK;
}

// the prefixes of validated rules, packed; returns the longest prefix (0: none)
inline uint32_t pack(const bcw_compact_rules& r, PrefixTable* t) {
  std::memset(t, 0, sizeof *t);
  uint32_t longest = 0;
  for (uint32_t i = 0; i < r.n_prefix; ++i) {
    const uint32_t a = r.prefix_off[i], n = r.prefix_off[i + 1] - a;
    for (uint32_t b = 0; b < n; ++b) t->w[i][b >> 2] |= (uint32_t)r.prefixes[a + b] << (8 * (b & 3));
    t->len[i] = n;
    if (n > longest) longest = n;
  }
  return longest;
}

// Does the merged key of key_len bytes start with the prefix pw of pl bytes (1..64)? kw: the key's first kKeyChunks
// 16 B chunks as little-endian words, zero beyond the key (and beyond the chunks the caller loaded: it loads every
// chunk that holds a byte below min(key_len, the longest prefix)). A prefix longer than the key never matches.
BCW_RULES_FN bool starts_with(const uint32_t* kw, uint32_t key_len, const uint32_t* pw, uint32_t pl) {
  if (pl > key_len) return false;
#pragma unroll
  for (uint32_t w = 0; w < kPrefixWords; ++w) {
    if (4 * w >= pl) break;
    const uint32_t nb = pl - 4 * w;
    const uint32_t m = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
    if ((kw[w] ^ pw[w]) & m) return false;
  }
  return true;
}

// 16 B chunks of a key that a prefix comparison can read
BCW_RULES_FN uint32_t key_chunks(uint32_t key_len, uint32_t longest) {
  const uint32_t n = key_len < longest ? key_len : longest;
  return (n + 15) / 16;
}

// The first rule that matches a row, in the order EXPIRED, TOMBSTONE, PREFIX, or kNone. expire: the record table's
// column (absolute, 0: MetaNoExpire); flags: the record's flag byte. load(kw, n) fills kw[0, 4 n) with the merged
// key's first n chunks; it is called only when the prefix rule is reached (kw beyond stays zero).
template <class Load>
BCW_RULES_FN uint32_t first_match(uint32_t mask, uint64_t now, uint64_t expire, uint32_t flags, uint32_t key_len,
                                  const uint32_t (*pw)[kPrefixWords], const uint32_t* plen, uint32_t n_prefix,
                                  uint32_t longest, Load load) {
  if ((mask & BCW_RULE_EXPIRED) && expire != 0 && expire <= now) return kExpired;
  if ((mask & BCW_RULE_TOMBSTONE) && (flags & kTombstone)) return kTombstoneHit;
  if ((mask & BCW_RULE_PREFIX) && n_prefix) {
    uint32_t kw[4 * kKeyChunks] = {};
    load(kw, key_chunks(key_len, longest));
    for (uint32_t i = 0; i < n_prefix; ++i)
      if (starts_with(kw, key_len, pw[i], plen[i])) return kPrefix;
  }
  return kNone;
}

}  // namespace rules
}  // namespace bcw
