// bcw_murmur.h -- MurmurHash3_x64_128 with seed 0, of which the index keeps h1: IndexOperator.Hash (index.go:15-19,
// spaolacci/murmur3 v1.1.0 New64().Sum64()). The hash every slot placement depends on, and the single home of its
// block step, its tail / finish step and fmix64. Plain inline functions compiled by the kernels (bcw_index.hip feeds
// 16-byte chunks of a merged key), by the host (bcw_murmur3_sum64 walks a byte pointer) and by the stand-alone host
// check (tools/murmur_check.cpp), as bcw_frame.h and bcw_drop.h are: one text for all three. No device calls here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BCW_MURMUR_FN __host__ __device__ __forceinline__
#else
#define BCW_MURMUR_FN inline
#endif

namespace bcw {
namespace murmur {

constexpr uint64_t kC1 = 0x87c37b91114253d5ull, kC2 = 0x4cf5ad432745937full;

BCW_MURMUR_FN uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
BCW_MURMUR_FN uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
// what a block's (or the tail's) low / high word contributes to h1 / h2
BCW_MURMUR_FN uint64_t mix_k1(uint64_t k1) { k1 *= kC1; k1 = rotl64(k1, 31); k1 *= kC2; return k1; }
BCW_MURMUR_FN uint64_t mix_k2(uint64_t k2) { k2 *= kC2; k2 = rotl64(k2, 33); k2 *= kC1; return k2; }

struct State {
  uint64_t h1 = 0, h2 = 0;
  // one 16-byte block: k1 = bytes 0-7, k2 = bytes 8-15, little-endian
  BCW_MURMUR_FN void block(uint64_t k1, uint64_t k2) {
    h1 ^= mix_k1(k1);
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    h2 ^= mix_k2(k2);
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  // the tail of t = n & 15 bytes, zero-padded into k1 (bytes 0-7) and k2 (bytes 8-15), then the finish over the
  // whole length n; returns Sum64
  BCW_MURMUR_FN uint64_t finish(uint64_t k1, uint64_t k2, uint32_t t, uint64_t n) {
    if (t > 8) h2 ^= mix_k2(k2);
    if (t > 0) h1 ^= mix_k1(k1);
    h1 ^= n; h2 ^= n;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    h1 += h2;
    return h1;
  }
};

// up to 8 bytes at p as a little-endian word, zero above them (each byte widened unsigned before it is shifted)
BCW_MURMUR_FN uint64_t le_word(const uint8_t* p, uint32_t nbytes) {
  uint64_t w = 0;
  for (uint32_t i = 0; i < nbytes; ++i) w |= (uint64_t)p[i] << (8 * i);
  return w;
}

// Sum64 of the n bytes at p
BCW_MURMUR_FN uint64_t sum64(const uint8_t* p, uint64_t n) {
  State m;
  const uint64_t nb = n / 16;
  for (uint64_t i = 0; i < nb; ++i) m.block(le_word(p + 16 * i, 8), le_word(p + 16 * i + 8, 8));
  const uint32_t t = (uint32_t)(n & 15);
  const uint8_t* tail = p + 16 * nb;
  return m.finish(le_word(tail, t < 8 ? t : 8), t > 8 ? le_word(tail + 8, t - 8) : 0, t, n);
}

}  // namespace murmur
}  // namespace bcw
