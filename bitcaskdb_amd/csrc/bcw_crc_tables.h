// bcw_crc_tables.h -- the CRC-32C constant tables (reflected polynomial 0x82F63B78, Go crc32.Castagnoli) every
// context uploads once: they decide each CRC verdict of the decode and each CRC the writers emit. Plain C++, no HIP:
// bcw_ctx_create builds and uploads them, tools/crc_tables_check.cpp checks them on the CPU. Shapes: bcw_crc_consts.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bcw.h"
#include "bcw_crc_consts.h"

namespace bcw {
namespace crc {

inline void byte_table(uint32_t* t0) {
  for (uint32_t b = 0; b < 256; ++b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
    t0[b] = c;
  }
}

inline uint32_t zero_step(const uint32_t* t0, uint32_t s) { return (s >> 8) ^ t0[s & 0xffu]; }

// images of the 32 basis vectors under "advance over n zero bytes"
inline void shift_basis(const uint32_t* t0, uint64_t n, uint32_t* img) {
  for (int i = 0; i < 32; ++i) {
    uint32_t v = 1u << i;
    for (uint64_t k = 0; k < n; ++k) v = zero_step(t0, v);
    img[i] = v;
  }
}
inline uint32_t apply_basis(const uint32_t* img, uint32_t x) {
  uint32_t r = 0;
  for (int i = 0; x; ++i, x >>= 1)
    if (x & 1u) r ^= img[i];
  return r;
}

// basis images of the inverse of a (bijective) GF(2)-linear map given by its basis images
inline void invert_basis(const uint32_t* img, uint32_t* inv) {
  uint32_t out[32], in[32];
  for (int i = 0; i < 32; ++i) { out[i] = img[i]; in[i] = 1u << i; }
  for (int bit = 0; bit < 32; ++bit) {
    int p = bit;
    while (p < 32 && !((out[p] >> bit) & 1u)) ++p;  // x^8n mod P is invertible: a pivot always exists
    std::swap(out[bit], out[p]);
    std::swap(in[bit], in[p]);
    for (int r = 0; r < 32; ++r)
      if (r != bit && ((out[r] >> bit) & 1u)) { out[r] ^= out[bit]; in[r] ^= in[bit]; }
  }
  for (int bit = 0; bit < 32; ++bit) inv[bit] = in[bit];
}

inline void nibble_image(const uint32_t* img, uint32_t* t) {
  for (int i = 0; i < 8; ++i)
    for (uint32_t n = 0; n < 16; ++n) t[i * 16 + n] = apply_basis(img, n << (4 * i));
}

// the ladder A_{8*2^k}, k < n, as basis images ladder[k][32]: A_8, then repeated squaring
// (A_{8*2^(k+1)} = A_{8*2^k} o A_{8*2^k})
inline void pow2_ladder(const uint32_t* t0, int n, uint32_t (*ladder)[32]) {
  shift_basis(t0, 1, ladder[0]);
  for (int k = 1; k < n; ++k)
    for (int i = 0; i < 32; ++i) ladder[k][i] = apply_basis(ladder[k - 1], ladder[k - 1][i]);
}

// encode shift operators (nibble images, 128 words each; layout in bcw_crc_consts.h): A_{8*16*n}, A_{8*256*n},
// A_{8*4096*n} (k_write's lane chains), A_{8t}^-1 (t < 16), and A_{8*2^k} / A_{8*2^k}^-1 for shifts by arbitrary
// distances (the CRC combine of re-encoded records)
inline void build_enc_ops(const uint32_t* t0, const uint32_t (*ladder)[32], uint32_t* ops) {
  uint32_t img[32], inv[32];
  for (int n = 0; n < 16; ++n) { shift_basis(t0, 16ull * n, img); nibble_image(img, ops + n * 128); }
  for (int n = 0; n < 16; ++n) { shift_basis(t0, 256ull * n, img); nibble_image(img, ops + (16 + n) * 128); }
  for (int n = 0; n < 8; ++n) { shift_basis(t0, 4096ull * n, img); nibble_image(img, ops + (32 + n) * 128); }
  for (int t = 0; t < 16; ++t) {
    shift_basis(t0, (uint64_t)t, img);
    invert_basis(img, inv);
    nibble_image(inv, ops + (kOpInv + t) * 128);
  }
  for (int k = 0; k < 32; ++k) {
    nibble_image(ladder[k], ops + (kOpPow2 + k) * 128);
    if (k < 15) {
      invert_basis(ladder[k], inv);
      nibble_image(inv, ops + (kOpPow2Inv + k) * 128);
    }
  }
}

// initc[L] = A_{8L}(0xFFFFFFFF), L <= BCW_BLOCK_SIZE: the contribution of the CRC init value after L data bytes
inline void build_initc(const uint32_t* t0, uint32_t* initc) {
  uint32_t v = 0xffffffffu;
  for (uint32_t L = 0; L <= BCW_BLOCK_SIZE; ++L) {
    initc[L] = v;
    v = zero_step(t0, v);
  }
}

// the stream verify's LDS image (bcw_crc_consts.h kS2*): slice rows with the shifted tables, lane operators, split
// operators, the byte-select tables of the fragment-end masks
inline void build_stream_image(const uint32_t* t0, uint32_t* image2) {
  uint32_t tk[4][256], img[32], nib[128], step[32], m[32];
  memcpy(tk[0], t0, sizeof tk[0]);
  for (int k = 1; k < 4; ++k)
    for (int e = 0; e < 256; ++e) tk[k][e] = (tk[k - 1][e] >> 8) ^ t0[tk[k - 1][e] & 0xffu];
  uint32_t sh[32];
  shift_basis(t0, kSChunk - kSPiece, sh);
  for (int e = 0; e < 256; ++e)
    for (int s = 0; s < 4; ++s)
      for (int cp = 0; cp < 8; ++cp) {
        image2[kS2SliceOff + e * 64 + s * 8 + cp] = tk[3 - s][e];
        image2[kS2SliceOff + e * 64 + 32 + s * 8 + cp] = apply_basis(sh, tk[3 - s][e]);
      }
  shift_basis(t0, kSPiece, step);
  for (int i = 0; i < 32; ++i) m[i] = 1u << i;  // identity for lane 63
  for (int l = 63; l >= 0; --l) {
    nibble_image(m, nib);
    for (int k = 0; k < 128; ++k) image2[kS2LopOff + k * 64 + l] = nib[k];
    for (int i = 0; i < 32; ++i) m[i] = apply_basis(step, m[i]);
  }
  for (int k = 0; k < kSPW; ++k) {  // split operators as byte tables: [k][t][e] = A(e << 8t)
    shift_basis(t0, 4u * (kSPW - k) + (kSChunk - kSPiece), img);
    for (int t = 0; t < 4; ++t)
      for (uint32_t e = 0; e < 256; ++e)
        image2[kS2KopOff + (k * 4 + t) * 256 + e] = apply_basis(img, e << (8 * t));
  }
  auto put_bytes = [&](int at, const uint8_t (&b)[16]) {
    for (int w = 0; w < 4; ++w)
      image2[at + w] = b[4 * w] | b[4 * w + 1] << 8 | b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
  };
  for (int n = 0; n < kS2GeN; ++n) {  // GE[n]: bytes q >= n
    uint8_t b[16];
    for (int q = 0; q < 16; ++q) b[q] = q >= n ? 0xff : 0x00;
    put_bytes(kS2Ge + 4 * n, b);
  }
  for (int m = 0; m < kS2JselN; ++m) {  // JSEL[m]: perm selectors, J byte q - o at q in [o, o + 4) (o = m - 3), else 0
    uint8_t b[16];
    for (int q = 0; q < 16; ++q) {
      const int p = q - (m - 3);
      b[q] = (m < kS2JselN - 1 && p >= 0 && p < 4) ? (uint8_t)(4 + p) : 0x0c;
    }
    put_bytes(kS2Jsel + 4 * m, b);
  }
  for (int g = 0; g < kS2GapN; ++g) {  // GAP[g]: J at [o, o + 4) (o = g - 6), zeros at [o + 4, o + 7), else the byte
    uint8_t b[16];
    for (int q = 0; q < 16; ++q) {
      const int p = q - (g - 6);
      b[q] = g == kS2GapN - 1 ? (uint8_t)(q & 3) : (p >= 0 && p < 4) ? (uint8_t)(4 + p) : (p >= 4 && p < 7) ? 0x0c
                                                                                          : (uint8_t)(q & 3);
    }
    put_bytes(kS2Gap + 4 * g, b);
  }
}

// the four tables of a context, from one byte table and one ladder (the image's pad words stay 0)
struct Tables {
  std::vector<uint32_t> initc, enc_ops, pow2, lds_image2;
};
inline Tables build_tables() {
  uint32_t t0[256], ladder[32][32];
  byte_table(t0);
  pow2_ladder(t0, 32, ladder);
  using V = std::vector<uint32_t>;
  Tables T{V(BCW_BLOCK_SIZE + 1), V(kEncOpsWords), V(kPow2Ops * 128), V(kS2Image)};
  build_initc(t0, T.initc.data());
  build_enc_ops(t0, ladder, T.enc_ops.data());
  for (int k = 0; k < kPow2Ops; ++k) nibble_image(ladder[k], T.pow2.data() + k * 128);  // = enc_ops[kOpPow2 + k]
  build_stream_image(t0, T.lds_image2.data());
  return T;
}

}  // namespace crc
}  // namespace bcw
