// usage_check.cpp -- the closed form of WalRecordSize (csrc/bcw_usage.h, wal_record_size_closed: the text the index's
// accounting pass compiles) as a stand-alone program. No device, no library. It is checked against the reference's
// plain loop (wal.go:61-86) at every offset of two blocks and the sizes around the fragment boundaries, on random
// pairs, and at sizes no loop could walk (2^40, 2^62) against the same formula in 128-bit arithmetic.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/usage_check.cpp -o /tmp/usage_check && /tmp/usage_check
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "bcw_usage.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "usage_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

// WalRecordSize as the reference writes it: one iteration per fragment
static uint64_t loop_size(uint64_t offset, uint64_t size) {
  const uint64_t kB = BCW_BLOCK_SIZE, kH = BCW_HEADER_SIZE;
  uint64_t left = size, phy = 0;
  offset -= BCW_SUPER_BLOCK_SIZE;
  while (left > 0) {
    uint64_t leftover = kB - (offset % kB);
    if (leftover < kH) {
      phy += leftover;
      offset += leftover;
      leftover = kB;
    }
    const uint64_t frag = left < leftover - kH ? left : leftover - kH;
    phy += kH + frag;
    offset += kH + frag;
    left -= frag;
  }
  return phy;
}

// the closed form with every intermediate in 128 bits, truncated at the end
static uint64_t wide_size(uint64_t off, uint64_t size) {
  typedef unsigned __int128 u128;
  if (size == 0) return 0;
  const u128 kB = BCW_BLOCK_SIZE, kH = BCW_HEADER_SIZE, kData = kB - kH;
  const u128 o = (u128)(off - BCW_SUPER_BLOCK_SIZE);
  u128 lo = kB - o % kB, total = 0;
  if (lo < kH) { total = lo; lo = kB; }
  const u128 first = (u128)size < lo - kH ? (u128)size : lo - kH;
  total += kH + first;
  const u128 rem = (u128)size - first;
  if (rem) {
    total += (rem / kData) * kB;
    if (rem % kData) total += kH + rem % kData;
  }
  return (uint64_t)total;
}

int main() {
  using bcw::usage::wal_record_size_closed;
  const uint64_t sizes[] = {0, 1, 6, 7, 8, 100, 32760, 32761, 32762, 65522, 65523, 100000};
  uint64_t n = 0;
  for (uint64_t off = 40; off <= 40 + 2 * 32768 + 16; ++off)
    for (uint64_t s : sizes) {
      CHECK(wal_record_size_closed(off, s) == loop_size(off, s));
      ++n;
    }
  // every size that fills the first block exactly, one less and one more, at the offsets around a block's end
  for (uint64_t left = 0; left <= 16; ++left) {
    const uint64_t off = 40 + 32768 - left;
    const uint64_t lo = left < 7 ? 32768 : left;
    for (int64_t d : {-1, 0, 1, 32761, 32762}) {
      const int64_t s = (int64_t)lo - 7 + d;
      if (s < 0) continue;
      CHECK(wal_record_size_closed(off, (uint64_t)s) == loop_size(off, (uint64_t)s));
      ++n;
    }
  }
  for (int i = 0; i < 8000; ++i) {
    const uint64_t off = 40 + rnd() % (1ull << 34), s = rnd() % (1ull << (1 + rnd() % 24));
    CHECK(wal_record_size_closed(off, s) == loop_size(off, s));
    CHECK(wal_record_size_closed(off, s) == wide_size(off, s));
    ++n;
  }
  // sizes the loop would walk for minutes or years: constant time here, equal to the wide evaluation
  for (uint64_t s : {1ull << 40, (1ull << 40) + 12345, 1ull << 62, (1ull << 62) + 32761, ~0ull})
    for (uint64_t off : {40ull, 41ull, 40ull + 32768 - 3, 40ull + 32768 - 7, 1ull << 33, (1ull << 50) + 17}) {
      CHECK(wal_record_size_closed(off, s) == wide_size(off, s));
      ++n;
    }
  std::printf("usage_check ok: %llu pairs\n", (unsigned long long)n);
  return 0;
}
