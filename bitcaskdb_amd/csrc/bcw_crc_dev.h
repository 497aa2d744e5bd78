// bcw_crc_dev.h -- the device primitives the kernels that write or read framed WAL bytes share (bcw_encode.hip,
// bcw_put.hip, bcw_read_body.h, bcw_index.hip): the CRC-32C tables a workgroup builds in LDS, the steps and shift
// operators applied to a raw CRC state, the 16 B unit helpers of the copy loops, the wave-aggregated counter add and
// the wave sum. The single home of each. What a kernel stages, its LDS layout and its launch bounds stay in the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcw {

// entry b of the CRC-32C byte table (reflected polynomial 0x82F63B78, Go crc32.Castagnoli)
__device__ __forceinline__ uint32_t crc_byte_entry(uint32_t c) {
  for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
  return c;
}
// the raw state c after one more zero byte
__device__ __forceinline__ uint32_t crc_zero_step(const uint32_t* t0, uint32_t c) { return (c >> 8) ^ t0[c & 0xffu]; }
// The byte table into t0[256] by the workgroup's `threads` threads; the caller's __syncthreads follows. (A workgroup
// of exactly 256 threads stores t0[tid] = crc_byte_entry(tid) itself, without the loop.)
__device__ __forceinline__ void crc_byte_table(uint32_t* t0, uint32_t tid, uint32_t threads) {
  for (uint32_t i = tid; i < 256; i += threads) t0[i] = crc_byte_entry(i);
}
// slice-by-K extension of a finished byte table: t[256 k + b] = CRC of byte b and k zero bytes, 1 <= k < K
template <int K>
__device__ __forceinline__ void crc_slice_tables(uint32_t* t, uint32_t tid, uint32_t threads) {
  for (uint32_t i = tid; i < 256; i += threads) {
    uint32_t c = t[i];
    for (int k = 1; k < K; ++k) { c = crc_zero_step(t, c); t[256 * k + i] = c; }
  }
}
// CRC-32C state after 16 more bytes (raw, slice-by-8: t8[256 k + b] = CRC of byte b and k zeros)
__device__ __forceinline__ uint32_t crc_step16(const uint32_t* __restrict__ t8, uint32_t c, uint4 v) {
  uint32_t x = c ^ v.x, y = v.y;
  c = t8[1792 + (x & 0xffu)] ^ t8[1536 + ((x >> 8) & 0xffu)] ^ t8[1280 + ((x >> 16) & 0xffu)] ^ t8[1024 + (x >> 24)] ^
      t8[768 + (y & 0xffu)] ^ t8[512 + ((y >> 8) & 0xffu)] ^ t8[256 + ((y >> 16) & 0xffu)] ^ t8[y >> 24];
  x = c ^ v.z;
  y = v.w;
  return t8[1792 + (x & 0xffu)] ^ t8[1536 + ((x >> 8) & 0xffu)] ^ t8[1280 + ((x >> 16) & 0xffu)] ^ t8[1024 + (x >> 24)] ^
         t8[768 + (y & 0xffu)] ^ t8[512 + ((y >> 8) & 0xffu)] ^ t8[256 + ((y >> 16) & 0xffu)] ^ t8[y >> 24];
}

// a shift operator A_{8m} (m zero bytes appended to a raw CRC-32C state) applied to x: nibble images (8 x 16 words)
__device__ __forceinline__ uint32_t op_apply(const uint32_t* __restrict__ op, uint32_t x) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r ^= op[i * 16 + ((x >> (4 * i)) & 15u)];
  return r;
}
// the same with byte images (4 x 256 words)
__device__ __forceinline__ uint32_t op_apply_b(const uint32_t* __restrict__ op, uint32_t x) {
  return op[x & 0xffu] ^ op[256 + ((x >> 8) & 0xffu)] ^ op[512 + ((x >> 16) & 0xffu)] ^ op[768 + (x >> 24)];
}

// bytes [sh, sh + 16) of the 32 bytes v0 || v1: 16 bytes at an arbitrary address from two aligned 16 B loads (the
// caller checks bounds)
__device__ __forceinline__ uint4 shift16(uint4 v0, uint4 v1, uint32_t sh) {
  // named scalars and two select stages: an array indexed by w would be lowered to a scratch round trip
  const bool s2 = (sh & 8u) != 0, s1 = (sh & 4u) != 0;
  const uint32_t b0 = s2 ? v0.z : v0.x, b1 = s2 ? v0.w : v0.y, b2 = s2 ? v1.x : v0.z, b3 = s2 ? v1.y : v0.w,
                 b4 = s2 ? v1.z : v1.x, b5 = s2 ? v1.w : v1.y;
  const uint32_t c0 = s1 ? b1 : b0, c1 = s1 ? b2 : b1, c2 = s1 ? b3 : b2, c3 = s1 ? b4 : b3, c4 = s1 ? b5 : b4;
  const uint32_t b = sh & 3u;
  return make_uint4(__builtin_amdgcn_alignbyte(c1, c0, b), __builtin_amdgcn_alignbyte(c2, c1, b),
                    __builtin_amdgcn_alignbyte(c3, c2, b), __builtin_amdgcn_alignbyte(c4, c3, b));
}
// byte b of a 16 B unit
__device__ __forceinline__ uint32_t sel_byte(uint4 v, uint32_t b) {
  const uint32_t w = (b & 8u) ? ((b & 4u) ? v.w : v.z) : ((b & 4u) ? v.y : v.x);
  return (w >> (8 * (b & 3u))) & 0xffu;
}
// bytes [lo, hi) of a 16 B unit
__device__ __forceinline__ uint4 range_mask(int32_t lo, int32_t hi) {
  uint32_t m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t a = min(max(lo - 4 * k, 0), 4), b = min(max(hi - 4 * k, 0), 4);
    m[k] = (uint32_t)(((1ull << (8 * b)) - 1) & ~((1ull << (8 * a)) - 1));
  }
  return make_uint4(m[0], m[1], m[2], m[3]);
}
__device__ __forceinline__ void or_masked(uint4& v, uint4 q, uint4 m) {
  v.x |= q.x & m.x;
  v.y |= q.y & m.y;
  v.z |= q.z & m.z;
  v.w |= q.w & m.w;
}

// wave-aggregated add of v to *ctr; returns this lane's exclusive offset
__device__ __forceinline__ uint64_t wave_alloc(uint64_t* ctr, uint64_t v) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += t;
  }
  const uint64_t tot = __shfl(incl, 63, 64);
  uint64_t base = 0;
  if (lane == 63 && tot) base = atomicAdd(reinterpret_cast<unsigned long long*>(ctr), (unsigned long long)tot);
  base = __shfl(base, 63, 64);
  return base + incl - v;
}
// the sum of v over the wave's 64 lanes, in every lane (a butterfly: every lane of the wave calls it)
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

}  // namespace bcw
