// scan_check.cpp -- the scan by key prefix's shared text (csrc/bcw_scan.h: the argument check of bcw_index_scan*, the
// match / list / count rule, the `fits` rule and the tile arithmetic) as a stand-alone program, the same text the host
// and the scan kernels compile. No device, no library. The rule is checked against a byte-wise memcmp model.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/scan_check.cpp -o /tmp/scan_check && /tmp/scan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bcw_scan.h"

namespace S = bcw::scan;
namespace R = bcw::rules;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "scan_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using Bytes = std::vector<uint8_t>;

// scan parameters over `prefixes` (each a byte string), as a caller lays them out
struct Built {
  Bytes bytes;
  std::vector<uint32_t> off;
  bcw_scan_params p{};
  Built(uint32_t flags, const std::vector<Bytes>& prefixes) {
    off.push_back(0);
    for (const auto& x : prefixes) {
      bytes.insert(bytes.end(), x.begin(), x.end());
      off.push_back((uint32_t)bytes.size());
    }
    bytes.push_back(0);  // never read: data() stays non-null for an empty set
    p.flags = flags;
    p.n_prefix = (uint32_t)prefixes.size();
    p.prefixes = bytes.data();
    p.prefix_off = off.data();
  }
};

// the key's chunk c as the kernel loads it from the arena: bytes [16c, 16c + 16), zero beyond the key
static void chunk_of(const Bytes& key, uint32_t c, uint32_t* w) {
  w[0] = w[1] = w[2] = w[3] = 0;
  for (uint32_t b = 0; b < 16; ++b) {
    const size_t q = 16 * (size_t)c + b;
    if (q < key.size()) w[b >> 2] |= (uint32_t)key[q] << (8 * (b & 3));
  }
}

static bool model_starts_with(const Bytes& key, const Bytes& p) {
  return p.size() <= key.size() && std::memcmp(key.data(), p.data(), p.size()) == 0;
}

// scan::decide as the select kernel calls it: the packed table, and only the chunks a prefix can reach
static S::Hit decide(const bcw_scan_params& p, bool live, uint64_t off, uint64_t size, const Bytes& key) {
  R::PrefixTable t;
  const uint32_t longest = S::pack(p, &t);
  uint32_t kw[4 * R::kKeyChunks] = {};
  if (p.n_prefix) {
    const uint32_t n = R::key_chunks((uint32_t)key.size(), longest);
    for (uint32_t c = 0; c < n; ++c) chunk_of(key, c, kw + 4 * c);
  }
  return S::decide(live, off, size, kw, (uint32_t)key.size(), t.w, t.len, p.n_prefix, p.flags);
}

// the same by the issue's words, byte-wise
static S::Hit model(const std::vector<Bytes>& prefixes, uint32_t flags, bool live, uint64_t off, uint64_t size,
                    const Bytes& key) {
  S::Hit h{};
  if (!live) return h;
  uint32_t g = prefixes.empty() ? 0u : S::kNoGroup;
  for (size_t i = 0; i < prefixes.size() && g == S::kNoGroup; ++i)
    if (model_starts_with(key, prefixes[i])) g = (uint32_t)i;
  if (g == S::kNoGroup) return h;
  h.match = true;
  h.group = g;
  h.soft = off == 0;
  h.listed = off != 0 || (flags & BCW_SCAN_SOFT_DELETED);
  h.bytes = off != 0 ? size : 0;
  h.key_bytes = off != 0 ? key.size() : 0;
  return h;
}

static bool same(const S::Hit& a, const S::Hit& b) {
  return a.match == b.match && a.listed == b.listed && a.soft == b.soft && (!a.match || a.group == b.group) &&
         a.bytes == b.bytes && a.key_bytes == b.key_bytes;
}

static Bytes random_bytes(size_t n, uint32_t alphabet) {
  Bytes v(n);
  for (auto& b : v) b = (uint8_t)(rnd() % alphabet);
  return v;
}

static int check_validation() {
  const Bytes a{1, 2, 3};
  uint8_t kbuf[4];
  uint64_t obuf[4];
  bcw_scan_out none{};  // NULL arrays with caps 0: the totals only
  bcw_scan_out some{};
  some.keys = kbuf;
  some.keys_cap = sizeof kbuf;
  some.key_off = obuf;
  some.entries_cap = 3;
  {
    Built b(0, {a, a});
    CHECK(S::validate(nullptr, &none) == BCW_E_INVAL);
    CHECK(S::validate(&b.p, nullptr) == BCW_E_INVAL);
    CHECK(S::validate(&b.p, &none) == BCW_OK);
    CHECK(S::validate(&b.p, &some) == BCW_OK);  // every optional column NULL
    b.p.flags = BCW_SCAN_SOFT_DELETED;
    CHECK(S::validate(&b.p, &some) == BCW_OK);
    b.p.flags = 2u;  // an unknown flag
    CHECK(S::validate(&b.p, &some) == BCW_E_INVAL);
    b.p.flags = 0x80000000u | BCW_SCAN_SOFT_DELETED;
    CHECK(S::validate(&b.p, &some) == BCW_E_INVAL);
  }
  {
    Built b(0, {});  // n_prefix == 0: every live entry, whatever the arrays say
    CHECK(S::validate(&b.p, &none) == BCW_OK);
    b.p.prefixes = nullptr;
    b.p.prefix_off = nullptr;
    CHECK(S::validate(&b.p, &some) == BCW_OK);
  }
  {
    std::vector<Bytes> p64(64, a), p65(65, a);
    Built ok(0, p64), bad(0, p65);
    CHECK(S::validate(&ok.p, &none) == BCW_OK);  // 64 prefixes, duplicates of one another
    CHECK(S::validate(&bad.p, &none) == BCW_E_INVAL);  // n_prefix > 64
  }
  {
    Built e(0, {a, {}, a});  // an empty prefix
    CHECK(S::validate(&e.p, &none) == BCW_E_INVAL);
    Built l64(0, {Bytes(64, 7)}), l65(0, {Bytes(65, 7)}), one(0, {{9}});
    CHECK(S::validate(&l64.p, &none) == BCW_OK);
    CHECK(S::validate(&l65.p, &none) == BCW_E_INVAL);  // longer than 64 bytes
    CHECK(S::validate(&one.p, &none) == BCW_OK);
  }
  {
    Built d(0, {a, a, a});
    d.off[2] = 1;  // 0, 3, 1, 9: descends
    CHECK(S::validate(&d.p, &none) == BCW_E_INVAL);
  }
  {
    Built n(0, {a}), m(0, {a});
    n.p.prefixes = nullptr;
    m.p.prefix_off = nullptr;
    CHECK(S::validate(&n.p, &none) == BCW_E_INVAL);  // n_prefix > 0 with a NULL array
    CHECK(S::validate(&m.p, &none) == BCW_E_INVAL);
  }
  {
    Built b(0, {a});
    bcw_scan_out o = some;
    o.keys = nullptr;
    CHECK(S::validate(&b.p, &o) == BCW_E_INVAL);  // entries_cap > 0 with keys NULL
    o = some;
    o.key_off = nullptr;
    CHECK(S::validate(&b.p, &o) == BCW_E_INVAL);  // ... or key_off NULL
    o.entries_cap = 0;
    CHECK(S::validate(&b.p, &o) == BCW_OK);
  }
  return 0;
}

static int check_edges() {
  const Bytes key = random_bytes(64, 256);
  // n_prefix == 0: every live entry, group 0; the key is not looked at
  {
    Built b(0, {});
    const S::Hit h = decide(b.p, true, 40, 7, key);
    CHECK(h.match && h.listed && !h.soft && h.group == 0 && h.bytes == 7 && h.key_bytes == 64);
    CHECK(!decide(b.p, false, 40, 7, key).match);
    const S::Hit e = decide(b.p, true, 40, 7, {});  // the empty key
    CHECK(e.match && e.listed && e.key_bytes == 0);
  }
  // a duplicate of an earlier prefix collects nothing; the first of two overlapping prefixes wins, in either order
  {
    const Bytes ns(key.begin(), key.begin() + 20), ns7(key.begin(), key.begin() + 27);
    Built dup(0, {ns, ns}), ab(0, {ns, ns7}), ba(0, {ns7, ns});
    CHECK(decide(dup.p, true, 40, 1, key).group == 0);
    CHECK(decide(ab.p, true, 40, 1, key).group == 0 && decide(ba.p, true, 40, 1, key).group == 0);
    Bytes other = key;
    other[23] ^= 1;  // under ns, not under ns7
    CHECK(decide(ab.p, true, 40, 1, other).group == 0 && decide(ba.p, true, 40, 1, other).group == 1);
  }
  // a 64-byte prefix equals a 64-byte key and starts a 65-byte one; the 63-byte key is shorter than it
  {
    Built b(0, {key});
    Bytes k65 = key, k63(key.begin(), key.begin() + 63);
    k65.push_back(0);
    CHECK(decide(b.p, true, 40, 1, key).match && decide(b.p, true, 40, 1, k65).match);
    CHECK(!decide(b.p, true, 40, 1, k63).match);
    Bytes off63 = key;
    off63[63] ^= 0x80;  // the last byte of the prefix counts
    CHECK(!decide(b.p, true, 40, 1, off63).match);
  }
  // a prefix longer than the key never matches, the key's zero padding included
  {
    const Bytes k3{5, 6, 7};
    Built b(0, {{5, 6, 7, 0}, {5, 6, 7}, {5}});
    const S::Hit h = decide(b.p, true, 40, 1, k3);
    CHECK(h.match && h.group == 1);
  }
  // off: 0 is a SoftDelete, 0 < off < 40 is listed as any other
  {
    Built off_(0, {}), on(BCW_SCAN_SOFT_DELETED, {});
    const S::Hit a = decide(off_.p, true, 0, 9, key), b = decide(on.p, true, 0, 9, key);
    CHECK(a.match && a.soft && !a.listed && a.bytes == 0 && a.key_bytes == 0 && S::verdict_of(a) == 0);
    CHECK(b.match && b.soft && b.listed && b.bytes == 0 && b.key_bytes == 0 && S::verdict_of(b) == 1);
    const S::Hit c = decide(off_.p, true, 1, 9, key), d = decide(off_.p, true, 39, ~0ull, key);
    CHECK(c.listed && !c.soft && c.bytes == 9 && d.listed && d.bytes == ~0ull);
  }
  // the verdict byte names the group, 63 included
  {
    std::vector<Bytes> ps(63, Bytes{0xEE});
    ps.push_back(Bytes(key.begin(), key.begin() + 5));
    Built b(0, ps);
    const S::Hit h = decide(b.p, true, 40, 1, key);
    CHECK(h.group == 63 && S::verdict_of(h) == 64 && S::verdict_group(64) == 63);
  }
  return 0;
}

static int check_rule_against_model() {
  static const uint32_t klens[] = {0, 1, 3, 15, 16, 17, 20, 21, 35, 36, 37, 63, 64, 65, 120, 220};
  static const uint64_t offs[] = {0, 1, 39, 40, 123456, ~0ull};
  uint64_t cases = 0, listed = 0, soft = 0, missed = 0, later = 0;
  for (int rep = 0; rep < 4000; ++rep, ++cases) {
    const uint32_t kl = klens[rnd() % 16];
    const Bytes key = random_bytes(kl, rep & 1 ? 2 : 256);
    // a prefix set cut out of the key, some damaged, some longer than the key, some unrelated; sometimes none
    std::vector<Bytes> ps;
    const uint32_t np = rnd() % 5 == 0 ? 0 : 1 + (uint32_t)(rnd() % (rep % 50 == 0 ? 64 : 6));
    for (uint32_t i = 0; i < np; ++i) {
      const uint32_t pl = 1 + (uint32_t)(rnd() % 64);
      Bytes p = random_bytes(pl, rep & 1 ? 2 : 256);
      const int how = (int)(rnd() % 4);
      if (how != 0)
        for (uint32_t b = 0; b < pl && b < kl; ++b) p[b] = key[b];
      if (how == 2) p[rnd() % pl] ^= (uint8_t)(1u << (rnd() % 8));
      if (how == 3 && pl > 1) p.resize(1 + rnd() % (pl - 1));
      ps.push_back(p);
    }
    const uint32_t flags = (uint32_t)(rnd() & 1);
    const bool live = rnd() % 8 != 0;
    const uint64_t off = offs[rnd() % 6], size = rnd() % 3 ? rnd() % 100000 : rnd();
    Built b(flags, ps);
    CHECK(S::validate(&b.p, nullptr) == BCW_E_INVAL);
    bcw_scan_out none{};
    CHECK(S::validate(&b.p, &none) == BCW_OK);
    const S::Hit got = decide(b.p, live, off, size, key), want = model(ps, flags, live, off, size, key);
    CHECK(same(got, want));
    CHECK(S::verdict_of(got) == (want.listed ? 1u + want.group : 0u));
    listed += want.listed;
    soft += want.soft;
    missed += live && !want.match;
    later += want.match && want.group > 0;
  }
  CHECK(cases >= 4000 && listed > 500 && soft > 100 && missed > 300 && later > 100);
  return 0;
}

static int check_fits_and_tiles() {
  CHECK(S::fits(0, 0, 0, 0) && S::fits(5, 5, 9, 9) && S::fits(5, 6, 9, 10));
  CHECK(!S::fits(6, 5, 9, 9) && !S::fits(5, 5, 10, 9) && !S::fits(1, 0, 0, 0) && !S::fits(0, 0, 1, 0));
  CHECK(S::kTileSlots == 256);
  CHECK(S::tiles(0) == 0 && S::tiles(1) == 1 && S::tiles(256) == 1 && S::tiles(257) == 2);
  CHECK(S::tiles(1024) == 4 && S::tiles(1ull << 19) == 2048 && S::tiles(1ull << 23) == 32768);
  for (uint64_t s : {0ull, 255ull, 256ull, 1000ull, (1ull << 23) - 1}) {
    CHECK(S::tile_base(S::tile_of(s)) <= s && s < S::tile_base(S::tile_of(s) + 1));
    CHECK(S::tile_of(s) < S::tiles(s + 1));
  }
  CHECK(S::group_rows(0) == 1 && S::group_rows(1) == 1 && S::group_rows(64) == 64);
  CHECK(S::kGroupWords == 256 && S::kLiveWord == 256 && S::kAccWords == 257);
  // the layouts the ctypes binding restates
  static_assert(sizeof(bcw_scan_params) == 24 && sizeof(bcw_scan_group) == 32 && sizeof(bcw_scan_out) == 72 &&
                    sizeof(bcw_scan_result) == 48,
                "the scan's C-ABI structs");
  return 0;
}

int main() {
  if (check_validation() || check_edges() || check_rule_against_model() || check_fits_and_tiles()) return 1;
  std::printf("scan_check ok\n");
  return 0;
}
