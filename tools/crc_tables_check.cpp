// crc_tables_check.cpp -- the CRC-32C constant tables every context uploads (csrc/bcw_crc_tables.h: initc, enc_ops,
// pow2 and the stream verify's LDS image) as a stand-alone program. No device, no library. Each table is checked
// against a bit-at-a-time CRC-32C restated here, which shares nothing with the header but the polynomial:
//   initc[L] is the register after L zero bytes from 0xFFFFFFFF;
//   every enc_ops operator, applied through its nibble image to kWords fixed pseudo-random words, is "step that many
//   zero bytes" (the shifts up to 2^16 bytes directly, A_{8*2^k} beyond as two steps of the checked A_{8*2^(k-1)}), and
//   the inverses undo their operators;
//   pow2[k] is enc_ops[kOpPow2 + k];
//   in the LDS image: the slice rows are T0..T3 and their 1008-byte shifts, lane operator l is A_{8*16*(63-l)}, the
//   split operators and the GE / JSEL / GAP selector rows follow their definitions (bcw_crc_consts.h);
//   CRC-32C("123456789") = 0xE3069283, masked 0xC78AB0E5, through byte_table.
// Then a 64-bit FNV-1a of each table against the values of the builders this header replaced (the tables are the
// same bytes as before the move).
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/crc_tables_check.cpp -o /tmp/crc_tables_check && /tmp/crc_tables_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "bcw_crc_tables.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "crc_tables_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace bcw;

// the restatement: one bit at a time
namespace naive {
static uint32_t byte(uint32_t reg, uint8_t b) {
  reg ^= b;
  for (int k = 0; k < 8; ++k) reg = (reg & 1u) ? (reg >> 1) ^ 0x82F63B78u : reg >> 1;
  return reg;
}
static uint32_t zeros(uint32_t reg, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) reg = byte(reg, 0);
  return reg;
}
}  // namespace naive

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// an operator through its nibble image [8][16], as the kernels apply it; stride: words between entries (64 in the
// LDS image's transposed lane operators)
static uint32_t nib_apply(const uint32_t* t, uint32_t x, int stride = 1) {
  uint32_t r = 0;
  for (int i = 0; i < 8; ++i) r ^= t[(i * 16 + ((x >> (4 * i)) & 15u)) * stride];
  return r;
}

static unsigned long long fnv1a(const std::vector<uint32_t>& v) {
  unsigned long long h = 0xcbf29ce484222325ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * 4; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}

int main() {
  const crc::Tables T = crc::build_tables();
  CHECK(T.initc.size() == BCW_BLOCK_SIZE + 1 && T.enc_ops.size() == (size_t)kEncOpsWords);
  CHECK(T.pow2.size() == (size_t)kPow2Ops * 128 && T.lds_image2.size() == (size_t)kS2Image);
  constexpr int kWords = 256;
  uint32_t words[kWords];
  for (int i = 0; i < kWords; ++i) words[i] = i < 32 ? 1u << i : (uint32_t)rnd();  // the basis, then random words

  // initc
  for (uint32_t L : {0u, 1u, 2u, 7u, 32761u, 32768u}) CHECK(T.initc[L] == naive::zeros(0xffffffffu, L));

  // enc_ops: the operators of the lane chains and the power-of-two ladder up to 2^16 bytes, stepped directly
  const uint32_t* ops = T.enc_ops.data();
  auto is_shift = [&](int op, uint64_t nbytes) {
    for (uint32_t x : words)
      if (nib_apply(ops + op * 128, x) != naive::zeros(x, nbytes)) return false;
    return true;
  };
  for (int n = 0; n < 16; ++n) CHECK(is_shift(n, 16ull * n));
  for (int n = 0; n < 16; ++n) CHECK(is_shift(16 + n, 256ull * n));
  for (int n = 0; n < 8; ++n) CHECK(is_shift(32 + n, 4096ull * n));
  for (int k = 0; k <= 16; ++k) CHECK(is_shift(kOpPow2 + k, 1ull << k));
  // beyond: 2^k zero bytes are 2^(k-1) zero bytes twice
  for (int k = 17; k < 32; ++k)
    for (uint32_t x : words) {
      const uint32_t* half = ops + (kOpPow2 + k - 1) * 128;
      CHECK(nib_apply(ops + (kOpPow2 + k) * 128, x) == nib_apply(half, nib_apply(half, x)));
    }
  // the inverses: op^-1(op(x)) == x
  for (int t = 0; t < 16; ++t)
    for (uint32_t x : words) CHECK(nib_apply(ops + (kOpInv + t) * 128, naive::zeros(x, (uint64_t)t)) == x);
  for (int k = 0; k < 15; ++k)
    for (uint32_t x : words)
      CHECK(nib_apply(ops + (kOpPow2Inv + k) * 128, nib_apply(ops + (kOpPow2 + k) * 128, x)) == x);

  // pow2
  for (int k = 0; k < kPow2Ops; ++k)
    CHECK(std::memcmp(T.pow2.data() + k * 128, ops + (kOpPow2 + k) * 128, 128 * sizeof(uint32_t)) == 0);

  // the LDS image
  const uint32_t* img = T.lds_image2.data();
  constexpr uint64_t kTail = kSChunk - kSPiece;  // 1008: the bytes of a chunk after a lane's piece
  for (int e = 0; e < 256; ++e)
    for (int s = 0; s < 4; ++s) {
      const uint32_t tk = naive::zeros(naive::byte(0, (uint8_t)e), (uint64_t)(3 - s));  // T_{3-s}[e]
      const uint32_t shifted = naive::zeros(tk, kTail);
      for (int cp = 0; cp < 8; ++cp) {
        CHECK(img[kS2SliceOff + e * 64 + s * 8 + cp] == tk);
        CHECK(img[kS2SliceOff + e * 64 + 32 + s * 8 + cp] == shifted);
      }
    }
  for (int l = 0; l < 64; ++l)
    for (uint32_t x : words) CHECK(nib_apply(img + kS2LopOff + l, x, 64) == naive::zeros(x, 16ull * (63 - l)));
  for (int k = 0; k < kSPW; ++k)
    for (int t = 0; t < 4; ++t)
      for (uint32_t e = 0; e < 256; ++e)
        CHECK(img[kS2KopOff + (k * 4 + t) * 256 + e] == naive::zeros(e << (8 * t), 4ull * (kSPW - k) + kTail));
  auto sel = [&](int at, int q) { return (uint8_t)(img[at + q / 4] >> (8 * (q % 4))); };
  // selector bytes (v_perm): 0..3 the data word's bytes, 4..7 the check word's, 0x0c a zero byte
  for (int n = 0; n < kS2GeN; ++n)
    for (int q = 0; q < 16; ++q) CHECK(sel(kS2Ge + 4 * n, q) == (q >= n ? 0xff : 0x00));
  for (int m = 0; m < kS2JselN; ++m)
    for (int q = 0; q < 16; ++q) {
      const int p = q - (m - 3);  // the check word at piece offset m - 3; the last entry selects nothing
      const uint8_t want = (m != kS2JselN - 1 && p >= 0 && p < 4) ? (uint8_t)(4 + p) : 0x0c;
      CHECK(sel(kS2Jsel + 4 * m, q) == want);
    }
  for (int g = 0; g < kS2GapN; ++g)
    for (int q = 0; q < 16; ++q) {
      const int p = q - (g - 6);  // the check word at piece offset g - 6, then 3 zero bytes; the last entry: no gap
      uint8_t want = (uint8_t)(q & 3);
      if (g != kS2GapN - 1 && p >= 0 && p < 4) want = (uint8_t)(4 + p);
      if (g != kS2GapN - 1 && p >= 4 && p < 7) want = 0x0c;
      CHECK(sel(kS2Gap + 4 * g, q) == want);
    }
  for (int i = kS2Gap + 4 * kS2GapN; i < kS2Image; ++i) CHECK(img[i] == 0);  // the pad

  // known answers through byte_table
  uint32_t t0[256];
  crc::byte_table(t0);
  uint32_t reg = 0xffffffffu, bits = 0xffffffffu;
  for (const char* p = "123456789"; *p; ++p) {
    reg = (reg >> 8) ^ t0[(reg ^ (uint8_t)*p) & 0xffu];
    bits = naive::byte(bits, (uint8_t)*p);
  }
  CHECK(~reg == 0xE3069283u && ~bits == 0xE3069283u);
  const uint32_t c = ~reg;
  CHECK((uint32_t)(((c >> 15) | (c << 17)) + 0xa282ead8u) == 0xC78AB0E5u);  // ComputeCRC32's mask

  // the same bytes as the builders this header replaced
  const unsigned long long h_initc = fnv1a(T.initc), h_ops = fnv1a(T.enc_ops), h_pow2 = fnv1a(T.pow2),
                           h_img = fnv1a(T.lds_image2);
  std::printf("initc %016llx enc_ops %016llx pow2 %016llx lds_image2 %016llx\n", h_initc, h_ops, h_pow2, h_img);
  CHECK(h_initc == 0x7399ab11d26bbe4bull);
  CHECK(h_ops == 0xfa51dde36c908235ull);
  CHECK(h_pow2 == 0x6935f69e9e68844dull);
  CHECK(h_img == 0xe146d2c6341da25dull);
  std::printf("crc_tables_check ok\n");
  return 0;
}
