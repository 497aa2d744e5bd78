// verify_check.cpp -- the decisions of bcw_index_verify* (csrc/bcw_verify.h: classify, span_untrusted, span_beyond,
// fits -- what k_ix_vfy_select, k_get_lookup, k_vfy_read and k_vfy_final compile) as a stand-alone program. No device,
// no library. They are checked against brute-force models: the class against Get's order written as a chain of early
// returns over every (wal found, rd_status, rec_status, key equal); the span pre-check against the reference's
// WalRecordSize loop (wal.go:61-86) run in 128-bit arithmetic, on offsets around the super block, block ends and the
// image's end, sizes from 0 to past the image and the wrapping values near 2^64 -- wherever the pre-check lets a
// span through, the loop must be bounded by the image and its sum must not wrap; and the `fits` rule against the
// conjunction of its three caps on their edges.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/verify_check.cpp -o /tmp/verify_check && /tmp/verify_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bcw_usage.h"
#include "bcw_verify.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "verify_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint64_t n_checks = 0;
typedef unsigned __int128 u128;

// Get's order, db_impl.go:567-587, then the key compare
static uint32_t model_class(bool wal, uint32_t rd, uint32_t rec, bool eq) {
  if (!wal) return 1;
  if (rd != 0) return 2;
  if (rec != 0) return 3;
  if (!eq) return 4;
  return 0;
}

// WalRecordSize (wal.go:61-86) for off >= 40 without wrapping, counting the loop's rounds
static u128 model_record_size(uint64_t off, uint64_t size, uint64_t* rounds) {
  const u128 kB = BCW_BLOCK_SIZE, kH = BCW_HEADER_SIZE;
  u128 left = size, phy = 0, o = (u128)off - 40;
  *rounds = 0;
  while (left > 0) {
    u128 leftover = kB - (o % kB);
    if (leftover < kH) {
      phy += leftover;
      o += leftover;
      leftover = kB;
    }
    const u128 frag = left < leftover - kH ? left : leftover - kH;
    phy += kH + frag;
    o += kH + frag;
    left -= frag;
    ++*rounds;
  }
  return phy;
}

// the model of ReadRecord's test for an untrusted value: beyond iff the span does not lie inside [40, seg_len]
static bool model_beyond(uint64_t off, uint64_t size, uint64_t len) {
  if (off < 40 || off > len || size > len) return true;
  uint64_t rounds;
  return (u128)off + model_record_size(off, size, &rounds) > (u128)len;
}

static int check_span(uint64_t off, uint64_t size, uint64_t len) {
  using namespace bcw;
  const bool pre = vfy::span_untrusted(off, size, len);
  bool beyond = pre;
  if (!pre) {
    // the loop the kernels enter now: bounded by the image, and nothing wraps
    uint64_t rounds;
    const u128 rs = model_record_size(off, size, &rounds);
    CHECK(rounds <= len / (BCW_BLOCK_SIZE - BCW_HEADER_SIZE) + 2);  // a ragged first and last fragment
    CHECK(rs < ((u128)1 << 63) && (u128)off + rs < ((u128)1 << 64));
    CHECK((u128)usage::wal_record_size_closed(off, size) == rs);  // the accounting's closed form agrees there
    beyond = vfy::span_beyond(off, (uint64_t)rs, len);
  }
  CHECK(beyond == model_beyond(off, size, len));
  ++n_checks;
  return 0;
}

int main() {
  using namespace bcw::vfy;
  // the class: every combination, the sub-statuses over their whole ranges
  for (int wal = 0; wal < 2; ++wal)
    for (uint32_t rd = 0; rd < 8; ++rd)
      for (uint32_t rec = 0; rec < 4; ++rec)
        for (int eq = 0; eq < 2; ++eq) {
          CHECK(classify(wal != 0, rd, rec, eq != 0) == model_class(wal != 0, rd, rec, eq != 0));
          ++n_checks;
        }
  CHECK(classify(true, BCW_RD_OK, BCW_ST_OK, true) == BCW_VFY_OK);
  CHECK(classify(false, BCW_RD_CRC, BCW_ST_PANIC, false) == BCW_VFY_NO_WAL);
  CHECK(classify(true, BCW_RD_BEYOND, BCW_ST_PANIC, false) == BCW_VFY_READ);
  CHECK(classify(true, BCW_RD_OK, BCW_ST_INVALID, false) == BCW_VFY_RECORD);
  CHECK(classify(true, BCW_RD_OK, BCW_ST_OK, false) == BCW_VFY_KEY);
  CHECK(BCW_VFY_OK == 0 && BCW_VFY_NO_WAL == 1 && BCW_VFY_READ == 2 && BCW_VFY_RECORD == 3 && BCW_VFY_KEY == 4);
  CHECK(sizeof(bcw_verify_bad) == 48);

  // the span: images of a few sizes, offsets and sizes on every edge
  const uint64_t kB = BCW_BLOCK_SIZE, kMax = ~0ull;
  for (uint64_t len : std::vector<uint64_t>{0, 39, 40, 47, 48, kB, 40 + kB - 1, 40 + kB, 40 + kB + 1, 40 + 3 * kB + 17,
                                            40 + 40 * kB + 5}) {
    std::vector<uint64_t> offs = {0, 1, 17, 39, 40, 41, 47, kMax, kMax - 39, 1ull << 63};
    for (uint64_t b = 0; b <= 3; ++b)
      for (int64_t d = -9; d <= 9; ++d) offs.push_back(40 + b * kB + (uint64_t)d);
    for (int64_t d = -9; d <= 9; ++d) offs.push_back(len + (uint64_t)d);
    std::vector<uint64_t> sizes = {0, 1, 2, 11, kB - 8, kB - 7, kB - 6, kB, 2 * kB, 70000, kMax, kMax - 6, 1ull << 63};
    for (int64_t d = -9; d <= 9; ++d) sizes.push_back(len + (uint64_t)d);
    for (uint64_t off : offs)
      for (uint64_t size : sizes)
        if (check_span(off, size, len)) return 1;
    for (int i = 0; i < 4000; ++i) {
      const uint64_t off = (i & 1) ? rnd() % (len + 50) : rnd();
      const uint64_t size = (i & 2) ? rnd() % (len + 50) : rnd();
      if (check_span(off, size, len)) return 1;
    }
  }
  CHECK(span_untrusted(39, 1, 1000) && span_untrusted(1001, 1, 1000) && span_untrusted(40, 1001, 1000));
  CHECK(!span_untrusted(40, 1000, 1000) && !span_untrusted(1000, 0, 1000));

  // fits: each cap on its edge, alone and together
  for (uint64_t nb : {0ull, 1ull, 7ull})
    for (uint64_t kb : {0ull, 5ull, 300ull})
      for (uint64_t nf : {0ull, 1ull, 3ull})
        for (int dq = -1; dq <= 1; ++dq)
          for (int dk = -1; dk <= 1; ++dk)
            for (int dr = -1; dr <= 1; ++dr)
              for (int ovf = 0; ovf < 2; ++ovf) {
                if ((nb == 0 && dq < 0) || (kb == 0 && dk < 0) || (nf == 0 && dr < 0)) continue;
                const uint64_t bc = nb + (uint64_t)dq, kc = kb + (uint64_t)dk, rc = nf + (uint64_t)dr;
                const bool want = dq >= 0 && dk >= 0 && dr >= 0 && !ovf;
                CHECK(fits(nb, bc, kb, kc, nf, rc, ovf != 0) == want);
                ++n_checks;
              }
  CHECK(fits(0, 0, 0, 0, 0, 0, false));  // NULL arrays with cap 0 and nothing bad: totals only, whole

  std::printf("verify_check ok: %llu checks\n", (unsigned long long)n_checks);
  return 0;
}
