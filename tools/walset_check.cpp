// walset_check.cpp -- the host side of the resident WAL set (csrc/bcw_walset.h: sorted insert, replace, remove and
// the hand-back of owned images) against a std::map model, as a stand-alone program for a CPU sanitizer run. No
// device is needed: images are plain heap blocks the program frees as the library frees device images.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Ibitcaskdb_amd/csrc \
//       tools/walset_check.cpp -o /tmp/walset_check && /tmp/walset_check
#include <cstdio>
#include <cstdlib>
#include <map>

#include "bcw_walset.h"

using bcw::WalEnt;
using bcw::WalTable;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "walset_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

struct Model { uint64_t len, base; void* own; };

static int same(const WalTable& t, const std::map<uint64_t, Model>& m) {
  CHECK(t.ents.size() == m.size() && t.owned.size() == m.size());
  size_t i = 0;
  for (const auto& kv : m) {  // std::map iterates in ascending fid: the table's order
    CHECK(t.ents[i].fid == kv.first && t.ents[i].seg_len == kv.second.len && t.ents[i].base_time == kv.second.base);
    CHECK(t.owned[i] == kv.second.own);
    CHECK(kv.second.own == nullptr || t.ents[i].seg == (const uint8_t*)kv.second.own);
    CHECK(t.has(kv.first) && t.lower(kv.first) == i);
    ++i;
  }
  return 0;
}

int main() {
  WalTable t;
  std::map<uint64_t, Model> m;
  bool found = true;
  CHECK(t.remove(5, &found) == nullptr && !found && !t.has(5) && t.lower(5) == 0);
  static const uint8_t caller_image[64] = {};
  for (int step = 0; step < 20000; ++step) {
    const uint64_t fid = rnd() % 48 == 0 ? ~0ull - rnd() % 3 : rnd() % 40;  // a small fid range: many replaces
    const uint64_t op = rnd() % 4;
    if (op < 3) {
      const bool own = op != 0;  // upload (owned) or put (caller-owned)
      void* img = own ? std::malloc(32) : nullptr;
      const Model nm{rnd() % 100000, rnd(), img};
      void* old = t.put(WalEnt{fid, own ? (const uint8_t*)img : caller_image, nm.len, nm.base}, img);
      auto it = m.find(fid);
      CHECK(old == (it == m.end() ? nullptr : it->second.own));
      std::free(old);
      m[fid] = nm;
    } else {
      void* old = t.remove(fid, &found);
      auto it = m.find(fid);
      CHECK(found == (it != m.end()) && old == (found ? it->second.own : nullptr));
      std::free(old);
      if (found) m.erase(it);
    }
    if (same(t, m)) return 1;
  }
  for (void* img : t.owned) std::free(img);  // destroy
  std::printf("walset_check ok: %zu entries at the end\n", t.ents.size());
  return 0;
}
