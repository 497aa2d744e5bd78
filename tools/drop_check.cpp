// drop_check.cpp -- the fid-list text of bcw_index_drop_fids* (csrc/bcw_drop.h: fid_in, fid_in_range, selected,
// normalise -- what k_ix_drop, k_ix_count and k_ix_export compile) as a stand-alone program. No device, no library.
// It is checked against a std::set model: random lists of 0 .. 5000 entries with duplicates, drawn from narrow and
// full-width ranges, the edge fids 0 and 2^64 - 1, the list sizes 0, 1, 4096 and 4097 distinct, both modes and the
// offsets 0, 1, 39, 40.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/drop_check.cpp -o /tmp/drop_check && /tmp/drop_check
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "bcw_drop.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "drop_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static const uint64_t kMax = ~0ull;
static const uint64_t kOffs[] = {0, 1, 39, 40};
static uint64_t n_checks = 0;

// the model: a live entry with off != 0 is dropped iff its fid's membership in the set is what the mode asks for
static bool model(int mode, bool live, uint64_t off, const std::set<uint64_t>& s, uint64_t fid) {
  if (!live || off == 0) return false;
  const bool in = s.count(fid) != 0;
  return mode == BCW_DROP_IN ? in : !in;
}

// one list against the model, probed at its members, their neighbours, the edges and random fids
static int check_list(const std::vector<uint64_t>& raw) {
  using namespace bcw::drop;
  const std::set<uint64_t> s(raw.begin(), raw.end());
  std::vector<uint64_t> norm;
  for (int mode : {BCW_DROP_IN, BCW_DROP_NOT_IN}) {
    const int rc = normalise(mode, raw.empty() ? nullptr : raw.data(), (uint32_t)raw.size(), &norm);
    if (s.size() > BCW_USAGE_MAX_FIDS) {
      CHECK(rc == BCW_E_INVAL);
      return 0;
    }
    CHECK(rc == BCW_OK);
    CHECK(norm.size() == s.size());
    CHECK(std::equal(norm.begin(), norm.end(), s.begin()));  // ascending and distinct
  }
  const uint32_t nf = (uint32_t)norm.size();
  std::vector<uint64_t> probes = {0, 1, 2, kMax, kMax - 1, 1ull << 63, (1ull << 63) - 1};
  for (uint64_t f : s) {
    probes.push_back(f);
    probes.push_back(f + 1);  // wraps at 2^64 - 1
    probes.push_back(f - 1);  // wraps at 0
  }
  for (int i = 0; i < 64; ++i) probes.push_back(rnd());
  for (uint64_t f : probes) {
    const bool in = s.count(f) != 0;
    CHECK(fid_in(norm.data(), nf, f) == in);
    CHECK(fid_in_range(norm.data(), nf, f) == in);
    for (int mode : {BCW_DROP_IN, BCW_DROP_NOT_IN})
      for (uint64_t off : kOffs)
        for (bool live : {false, true}) {
          CHECK(selected(mode, live, off, fid_in_range(norm.data(), nf, f)) == model(mode, live, off, s, f));
          ++n_checks;
        }
  }
  return 0;
}

int main() {
  using namespace bcw::drop;
  std::vector<uint64_t> out;
  // refusals
  const uint64_t one[] = {7};
  CHECK(normalise(2, one, 1, &out) == BCW_E_INVAL);
  CHECK(normalise(-1, one, 1, &out) == BCW_E_INVAL);
  CHECK(normalise(BCW_DROP_IN, nullptr, 1, &out) == BCW_E_INVAL);
  CHECK(normalise(BCW_DROP_NOT_IN, nullptr, 0, &out) == BCW_OK && out.empty());
  CHECK(known_mode(BCW_DROP_IN) && known_mode(BCW_DROP_NOT_IN) && !known_mode(2));
  // the empty list: BCW_DROP_IN selects nothing, BCW_DROP_NOT_IN every file-backed entry
  if (check_list({})) return 1;
  CHECK(!selected(BCW_DROP_IN, true, 40, fid_in_range(nullptr, 0, 5)));
  CHECK(selected(BCW_DROP_NOT_IN, true, 40, fid_in_range(nullptr, 0, 5)));
  CHECK(selected(BCW_DROP_NOT_IN, true, 1, fid_in_range(nullptr, 0, 5)));
  CHECK(!selected(BCW_DROP_NOT_IN, true, 0, fid_in_range(nullptr, 0, 5)));
  // single entries and the edge fids
  for (uint64_t f : std::vector<uint64_t>{0, 1, 5, kMax - 1, kMax})
    if (check_list({f})) return 1;
  if (check_list({0, kMax})) return 1;
  if (check_list({kMax, 0, kMax, 0, 3, 3})) return 1;
  // the cap: 4096 distinct is accepted (also as 5000 entries with duplicates), 4097 is refused
  std::vector<uint64_t> big;
  for (uint64_t i = 0; i < BCW_USAGE_MAX_FIDS; ++i) big.push_back(kMax - 3 * i);
  if (check_list(big)) return 1;
  std::vector<uint64_t> dup = big;
  for (int i = 0; i < 904; ++i) dup.push_back(big[rnd() % big.size()]);
  CHECK(dup.size() == 5000);
  if (check_list(dup)) return 1;
  CHECK(normalise(BCW_DROP_IN, dup.data(), (uint32_t)dup.size(), &out) == BCW_OK && out.size() == BCW_USAGE_MAX_FIDS);
  big.push_back(1);
  if (check_list(big)) return 1;
  CHECK(normalise(BCW_DROP_IN, big.data(), (uint32_t)big.size(), &out) == BCW_E_INVAL);
  // random lists: sizes 0 .. 5000, values from a narrow range (many duplicates, dense neighbours) or all 64 bits
  for (int it = 0; it < 300; ++it) {
    const uint32_t n = (uint32_t)(rnd() % (it % 10 == 0 ? 5001 : 200));
    const uint64_t range = (it & 1) ? 0 : 1 + rnd() % 6000;
    const uint64_t base = (it & 2) ? kMax - 6000 : rnd() % 3;
    std::vector<uint64_t> raw(n);
    for (auto& v : raw) v = range ? base + rnd() % range : rnd();
    if (check_list(raw)) return 1;
  }
  std::printf("drop_check ok: %llu predicate checks\n", (unsigned long long)n_checks);
  return 0;
}
