// murmur_check.cpp -- the index's hash (csrc/bcw_murmur.h: what k_ix_keys and every lookup kernel compile, and what
// bcw_murmur3_sum64 calls) as a stand-alone program. No device, no library. Keys of every length 0 .. 80 at several
// alignments, their bytes drawn to include 0x80 and above (the sign-extension hazard of the tail), go through
//   the block-at-a-time path, fed zero-padded 16-byte chunks as four 32-bit words, as key_hash feeds it,
//   the byte-pointer path (murmur::sum64), and
//   a naive restatement written here: one byte at a time into a 128-bit state, after spaolacci/murmur3's
//   Write / bmix / Sum128 (what index.go:15-19 calls),
// and all three must agree; then the known answers tests/test_index_oracle.py pins against the oracle.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/murmur_check.cpp -o /tmp/murmur_check && /tmp/murmur_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "bcw_murmur.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "murmur_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the naive restatement: nothing shared with the header but the algorithm's published constants
namespace naive {
struct Digest {
  uint64_t h1 = 0, h2 = 0, len = 0;
  uint8_t buf[16];
  unsigned fill = 0;
};
static uint64_t rotl(uint64_t x, unsigned r) { return (x << r) | (x >> (64 - r)); }
static void byte(Digest& d, uint8_t b) {
  d.buf[d.fill++] = b;
  ++d.len;
  if (d.fill < 16) return;
  uint64_t k1 = 0, k2 = 0;
  for (int i = 7; i >= 0; --i) { k1 = (k1 << 8) | d.buf[i]; k2 = (k2 << 8) | d.buf[8 + i]; }
  k1 *= 0x87c37b91114253d5ull; k1 = rotl(k1, 31); k1 *= 0x4cf5ad432745937full; d.h1 ^= k1;
  d.h1 = rotl(d.h1, 27); d.h1 += d.h2; d.h1 = d.h1 * 5 + 0x52dce729;
  k2 *= 0x4cf5ad432745937full; k2 = rotl(k2, 33); k2 *= 0x87c37b91114253d5ull; d.h2 ^= k2;
  d.h2 = rotl(d.h2, 31); d.h2 += d.h1; d.h2 = d.h2 * 5 + 0x38495ab5;
  d.fill = 0;
}
static uint64_t fmix(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
static void sum128(const Digest& d, uint64_t* o1, uint64_t* o2) {
  uint64_t h1 = d.h1, h2 = d.h2, k1 = 0, k2 = 0;
  for (unsigned i = d.fill; i-- > 8;) k2 ^= (uint64_t)d.buf[i] << (8 * (i - 8));
  if (d.fill > 8) { k2 *= 0x4cf5ad432745937full; k2 = rotl(k2, 33); k2 *= 0x87c37b91114253d5ull; h2 ^= k2; }
  for (unsigned i = d.fill < 8 ? d.fill : 8; i-- > 0;) k1 ^= (uint64_t)d.buf[i] << (8 * i);
  if (d.fill > 0) { k1 *= 0x87c37b91114253d5ull; k1 = rotl(k1, 31); k1 *= 0x4cf5ad432745937full; h1 ^= k1; }
  h1 ^= d.len; h2 ^= d.len;
  h1 += h2; h2 += h1;
  h1 = fmix(h1); h2 = fmix(h2);
  h1 += h2; h2 += h1;
  *o1 = h1;
  *o2 = h2;
}
static uint64_t sum64(const uint8_t* p, uint64_t n) {
  Digest d;
  for (uint64_t i = 0; i < n; ++i) byte(d, p[i]);
  uint64_t h1, h2;
  sum128(d, &h1, &h2);
  return h1;
}
}  // namespace naive

// the header fed as the kernels feed it: chunk c = bytes [16c, 16c + 16) of the key, zero beyond it, as four
// little-endian 32-bit words
static uint64_t by_chunks(const uint8_t* p, uint64_t n) {
  bcw::murmur::State m;
  const uint64_t nb = n / 16;
  const uint32_t t = (uint32_t)(n & 15);
  uint64_t k1 = 0, k2 = 0;
  for (uint64_t c = 0; c <= nb; ++c) {
    uint8_t chunk[16] = {0};
    if (c < nb) std::memcpy(chunk, p + 16 * c, 16);
    else if (t) std::memcpy(chunk, p + 16 * c, t);
    uint32_t w[4];
    for (int q = 0; q < 4; ++q)
      w[q] = (uint32_t)chunk[4 * q] | ((uint32_t)chunk[4 * q + 1] << 8) | ((uint32_t)chunk[4 * q + 2] << 16) |
             ((uint32_t)chunk[4 * q + 3] << 24);
    k1 = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    k2 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    if (c < nb) m.block(k1, k2);
  }
  return m.finish(k1, k2, t, n);
}

int main() {
  unsigned long long n_keys = 0;
  // every length 0 .. 80, each with several byte patterns, the key at every offset 0 .. 3 of its buffer
  for (uint64_t n = 0; n <= 80; ++n)
    for (int pat = 0; pat < 6; ++pat)
      for (uint64_t shift = 0; shift < 4; ++shift) {
        std::vector<uint8_t> buf(shift + n + 1);
        for (uint64_t i = 0; i < n; ++i) {
          const uint8_t r = (uint8_t)rnd();
          buf[shift + i] = pat == 0 ? 0xff : pat == 1 ? 0x80 : pat == 2 ? (uint8_t)(r | 0x80) : pat == 3 ? 0 : r;
        }
        const uint8_t* p = buf.data() + shift;
        const uint64_t want = naive::sum64(p, n);
        CHECK(bcw::murmur::sum64(p, n) == want);
        CHECK(by_chunks(p, n) == want);
        ++n_keys;
      }
  CHECK(bcw::murmur::sum64(nullptr, 0) == 0);
  // known answers (spaolacci/murmur3 murmur3_test.go, seed 0: h1 = Sum64, h2), as tests/test_index_oracle.py has them
  static const struct { const char* s; uint64_t h1, h2; } kKnown[] = {
      {"", 0x0000000000000000ull, 0x0000000000000000ull},
      {"hello", 0xcbd8a7b341bd9b02ull, 0x5b1e906a48ae1d19ull},
      {"hello, world", 0x342fac623a5ebc8eull, 0x4cdcbc079642414dull},
      {"19 Jan 2038 at 3:14:07 AM", 0xb89e5988b737affcull, 0x664fc2950231b2cbull},
      {"The quick brown fox jumps over the lazy dog.", 0xcd99481f9ee902c9ull, 0x695da1a38987b6e7ull},
  };
  for (const auto& k : kKnown) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(k.s);
    const uint64_t n = std::strlen(k.s);
    naive::Digest d;
    for (uint64_t i = 0; i < n; ++i) naive::byte(d, p[i]);
    uint64_t h1, h2;
    naive::sum128(d, &h1, &h2);
    CHECK(h1 == k.h1 && h2 == k.h2);  // the restatement itself, on both halves
    CHECK(bcw::murmur::sum64(p, n) == k.h1);
    CHECK(by_chunks(p, n) == k.h1);
  }
  std::printf("murmur_check ok: %llu keys\n", n_keys);
  return 0;
}
