// frame_check.cpp -- the writer's framing rules, varints, CRC mask and Record.Encode header (csrc/bcw_frame.h: the text
// the host and the writer kernels compile) as a stand-alone program. No device, no library. Every function is checked
// against a model written here from the reference's own loops (WriteRecord wal.go:490-553, PutUvarint, ComputeCRC32
// utils.go:24-29, Record.Encode record.go:57-138), at every header position of two blocks and the lengths around the
// fragment boundaries, and on random pairs.
//   c++ -std=c++17 -O1 -Iinclude -Ibitcaskdb_amd/csrc tools/frame_check.cpp -o /tmp/frame_check && /tmp/frame_check
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/frame_check.cpp -o /tmp/frame_check && /tmp/frame_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "bcw_frame.h"
#include "bcw_usage.h"

using namespace bcw::frame;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "frame_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

// ---- framing: WriteRecord as the reference writes it, on a writer whose file ends at offset `pos` ----
struct Frag {
  uint64_t hp, flen;
  uint32_t type;
};
struct Written {
  uint64_t pad_from, offset, end;  // the zero pad is [pad_from, offset), the record [offset, end)
  std::vector<Frag> frags;
};
static Written write_record(uint64_t pos, uint64_t n) {
  const uint64_t kBlock = 32768, kHeader = 7;
  Written w{pos, 0, 0, {}};
  uint64_t left = n;
  bool begin = true;
  while (left > 0) {
    uint64_t leftover = kBlock - ((pos - 40) % kBlock);
    if (leftover < kHeader) {
      pos += leftover;  // padding[:leftover]
      leftover = kBlock;
    }
    if (begin) w.offset = pos;
    const uint64_t avail = leftover - kHeader;
    const uint64_t frag = left < avail ? left : avail;
    const bool end = left == frag;
    const uint32_t type = (begin && end) ? 1 : begin ? 2 : end ? 4 : 3;  // Full, First, Last, Middle
    w.frags.push_back(Frag{pos, frag, type});
    pos += kHeader + frag;
    left -= frag;
    begin = false;
  }
  w.end = pos;
  return w;
}

static uint64_t n_walks = 0;
// a record of len bytes whose first header is at P (a position the writer can produce: at least 7 bytes left)
static int check_walk(uint64_t P, uint64_t len) {
  const Written w = write_record(P, len);
  CHECK(w.offset == P && w.pad_from == P);
  uint64_t hp = P, rem = len;
  size_t k = 0;
  for (bool first = true;; first = false, ++k) {
    CHECK(k < w.frags.size());
    const FragStep s = next_frag(hp, rem, first);
    CHECK(hp == w.frags[k].hp && s.flen == w.frags[k].flen && s.type == w.frags[k].type);
    CHECK(s.ds == hp + 7 && s.be == blk_end(hp) && (s.be - 40) % 32768 == 0 && s.be > hp && s.be - hp <= 32768);
    CHECK(s.last == (k + 1 == w.frags.size()));
    rem -= s.flen;
    if (s.last) break;
    hp = s.be;
  }
  CHECK(rem == 0);
  CHECK(frag_count(P, len) == w.frags.size());
  CHECK(frag_room(P) == 32768 - (P - 40) % 32768 - 7);
  CHECK(rec_end(P, len) == w.end);
  CHECK(rec_end(P, len) - P == bcw::usage::wal_record_size_closed(P, len));
  ++n_walks;
  return 0;
}

// the zero pad before a record whose header the writer puts at the block start P, after `pad` bytes of padding: as the
// first record of a write that starts at P - pad, and after a one-byte record that ends there
static int check_pad(uint64_t P, uint64_t pad, uint64_t len) {
  const uint64_t pos = P - pad;
  const Written w = write_record(pos, len);
  CHECK(w.offset == P && w.pad_from == pos);
  bool called = false;
  CHECK(pad_start(0, pos, [&] { called = true; return (uint64_t)0; }) == w.pad_from && !called);
  const uint64_t PA = pos - 8;  // header + one byte; at least 8 bytes are left in its block
  const Written a = write_record(PA, 1);
  CHECK(a.offset == PA && a.end == pos);
  CHECK(pad_start(1, PA, [&] { return rec_end(PA, 1); }) == w.pad_from);
  return 0;
}

static int check_framing() {
  for (uint64_t P = 40; P < 40 + 2 * 32768; ++P) {
    const uint64_t ph = (P - 40) % 32768;
    CHECK(starts_block(P) == (ph == 0));
    if (ph > 32761) continue;  // fewer than 7 bytes left: the writer pads and starts the record at the next block
    for (uint64_t len = 1; len <= 40; ++len)
      if (check_walk(P, len)) return 1;
    for (int64_t d = -8; d <= 8; ++d) {
      if (check_walk(P, (uint64_t)(32761 + d)) || check_walk(P, (uint64_t)(2 * 32761 + d))) return 1;
      const int64_t l = (int64_t)frag_room(P) + d;  // room 0: the zero-length First
      if (l >= 1 && check_walk(P, (uint64_t)l)) return 1;
    }
    if (ph == 0 && P > 40)
      for (uint64_t pad = 0; pad <= 6; ++pad)
        for (uint64_t len : {1ull, 100ull, 32761ull, 32762ull})
          if (check_pad(P, pad, len)) return 1;
  }
  for (int i = 0; i < 10000; ++i) {
    uint64_t P;
    do P = 40 + rnd() % (1ull << 34); while ((P - 40) % 32768 > 32761);
    if (check_walk(P, 1 + rnd() % ((1ull << 20) - 1))) return 1;
  }
  // the header's bytes: masked CRC little-endian, length little-endian, type
  uint8_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0xee};
  store_frag_header(h, 0x04030201u, 0x0605u, 7);
  for (uint32_t i = 0; i < 7; ++i) CHECK(h[i] == i + 1 && (uint8_t)frag_header_byte(0x04030201u, 0x0605u, 7, i) == i + 1);
  CHECK(h[7] == 0xee);
  return 0;
}

// ---- varints: byte i holds bits [7i, 7i + 7), the continuation bit on all but the last ----
static std::vector<uint8_t> model_uvarint(uint64_t v) {
  int bits = 0;
  while (bits < 64 && (v >> bits) != 0) ++bits;
  const int n = bits == 0 ? 1 : (bits + 6) / 7;
  std::vector<uint8_t> out;
  for (int i = 0; i < n; ++i) out.push_back((uint8_t)(((v >> (7 * i)) & 0x7f) | (i + 1 < n ? 0x80 : 0)));
  return out;
}
// Go binary.Uvarint
static uint64_t model_uvarint_decode(const uint8_t* p, size_t n, size_t* used) {
  uint64_t x = 0;
  for (size_t i = 0; i < n; ++i) {
    x |= (uint64_t)(p[i] & 0x7f) << (7 * i);
    if (p[i] < 0x80) { *used = i + 1; return x; }
  }
  *used = 0;
  return 0;
}
static uint64_t n_varints = 0;
static int check_varint(uint64_t v) {
  uint8_t buf[12];
  memset(buf, 0xee, sizeof buf);
  const std::vector<uint8_t> m = model_uvarint(v);
  const uint32_t n = uvarint_put(buf + 1, v);
  CHECK(n == m.size() && uvarint_len(v) == n && n <= 10);
  CHECK(memcmp(buf + 1, m.data(), n) == 0 && buf[0] == 0xee && buf[1 + n] == 0xee);
  size_t used = 0;
  CHECK(model_uvarint_decode(buf + 1, n, &used) == v && used == n);
  ++n_varints;
  return 0;
}
static int check_varints() {
  if (check_varint(0) || check_varint(~0ull)) return 1;
  for (int k = 1; k <= 9; ++k) {
    const uint64_t p = 1ull << (7 * k);
    if (check_varint(p - 1) || check_varint(p) || check_varint(p + 1)) return 1;
  }
  for (int i = 0; i < 10000; ++i)
    if (check_varint(rnd() >> (rnd() % 64))) return 1;
  return 0;
}

// ---- Record.Encode's header, byte by byte; the classes in the order the batched Write reports them ----
struct HeaderCase {
  std::vector<uint8_t> ns, etag;
  bool etag_null;
  uint64_t kl, vl, ml, expire, base;
  uint32_t flags;
};
static int64_t model_header(const HeaderCase& c, std::vector<uint8_t>& out) {
  const uint64_t merged = c.ns.size() + c.kl;
  if ((merged | c.vl | c.ml) >> 32) return -BCW_ENC_ERR_BATCH;
  const bool etag_on = (c.flags & BCW_WR_ETAG) && !c.etag.empty();
  if (etag_on && c.etag_null) return -BCW_ENC_ERR_BATCH;
  uint8_t flag = 0;
  if (!etag_on) flag |= 1 << 0;                       // noEtagFieldBit
  if (c.flags & BCW_WR_TOMBSTONE) flag |= 1 << 2;     // tombstoneFieldBit
  std::vector<uint8_t> expire;
  if (c.expire == 0) {
    flag |= 1 << 1;                                   // noExpireFieldBit
  } else if (c.expire < c.base) {
    return -BCW_ENC_ERR_EXPIRE;
  } else {
    expire = model_uvarint(c.expire - c.base);
    if (expire.size() > 5) return -BCW_ENC_ERR_PANIC;  // [binary.MaxVarintLen32]byte
  }
  std::vector<uint8_t> tmp;
  for (uint64_t v : {c.kl, c.vl, c.ml})
    for (uint8_t b : model_uvarint(v)) tmp.push_back(b);
  const uint64_t header = tmp.size() + expire.size() + c.ns.size() + (etag_on ? c.etag.size() : 0) + 2;
  if ((header + c.kl + c.vl + c.ml) >> 32) return -BCW_ENC_ERR_BATCH;
  out.clear();
  out.push_back((uint8_t)header);  // byte(headerSize)
  out.insert(out.end(), c.ns.begin(), c.ns.end());
  out.push_back(flag);
  out.insert(out.end(), tmp.begin(), tmp.end());
  if (etag_on) out.insert(out.end(), c.etag.begin(), c.etag.end());
  out.insert(out.end(), expire.begin(), expire.end());
  return (int64_t)header;
}
static uint64_t n_headers = 0;
static int check_header(const HeaderCase& c) {
  std::vector<uint8_t> want;
  const int64_t m = model_header(c, want);
  const uint64_t merged = c.ns.size() + c.kl;
  const uint8_t* etag = c.etag_null ? nullptr : c.etag.data();
  const uint32_t es = (uint32_t)c.etag.size(), nsz = (uint32_t)c.ns.size();
  CHECK(record_header_put(nullptr, c.ns.data(), merged, nsz, c.vl, c.ml, etag, es, c.expire, c.base, c.flags) == m);
  std::vector<uint8_t> got(2 + c.ns.size() + 15 + c.etag.size() + 5 + 1, 0xee);
  CHECK(record_header_put(got.data(), c.ns.data(), merged, nsz, c.vl, c.ml, etag, es, c.expire, c.base, c.flags) == m);
  if (m < 0) {
    for (uint8_t b : got) CHECK(b == 0xee);  // nothing written
  } else {
    CHECK((uint64_t)m == want.size() && want.size() < got.size());
    CHECK(memcmp(got.data(), want.data(), want.size()) == 0);
    for (size_t i = want.size(); i < got.size(); ++i) CHECK(got[i] == 0xee);
  }
  ++n_headers;
  return 0;
}
static int check_headers() {
  const uint64_t base = 1700000000ull;
  const uint64_t lens[] = {0, 1, 127, 128, 16383, 16384};
  const uint64_t expires[] = {0, base, base + 1, base + (1ull << 35) - 1, base + (1ull << 35), base - 1};
  auto bytes = [](size_t n, uint8_t seed) {
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)(seed + 7 * i);
    return v;
  };
  for (size_t ns : {0, 1, 16, 20, 64, 300})  // 300: a header longer than 255 bytes, headerSize truncated
    for (size_t es : {0, 20})
      for (uint64_t kl : lens)
        for (uint64_t vl : lens)
          for (uint64_t ml : lens)
            for (uint64_t ex : expires)
              for (uint32_t flags : {0u, (uint32_t)BCW_WR_TOMBSTONE, (uint32_t)BCW_WR_ETAG,
                                     (uint32_t)(BCW_WR_ETAG | BCW_WR_TOMBSTONE | BCW_WR_DELETED)})
                for (bool etag_null : {false, true}) {
                  if (etag_null && !(flags & BCW_WR_ETAG) && ex != 0) continue;  // the etag is not looked at
                  if (check_header(HeaderCase{bytes(ns, 0x41), bytes(es, 0x90), etag_null, kl, vl, ml, ex, base, flags}))
                    return 1;
                }
  // what the batch cannot express: a merged key shorter than the namespace, a length or a payload of 2^32 bytes
  std::vector<uint8_t> out(64, 0xee);
  CHECK(record_header_put(out.data(), out.data(), 3, 4, 0, 0, nullptr, 0, 0, base, 0) == -BCW_ENC_ERR_BATCH);
  CHECK(record_header_put(nullptr, nullptr, 1ull << 32, 0, 0, 0, nullptr, 0, 0, base, 0) == -BCW_ENC_ERR_BATCH);
  CHECK(record_header_put(nullptr, nullptr, 0, 0, 1ull << 32, 0, nullptr, 0, 0, base, 0) == -BCW_ENC_ERR_BATCH);
  CHECK(record_header_put(nullptr, nullptr, 0, 0, 0, 1ull << 32, nullptr, 0, 0, base, 0) == -BCW_ENC_ERR_BATCH);
  CHECK(record_header_put(nullptr, nullptr, 0, 0, (1ull << 32) - 9, 0, nullptr, 0, 0, base, 0) == -BCW_ENC_ERR_BATCH);
  CHECK(record_header_put(nullptr, nullptr, 0, 0, (1ull << 32) - 10, 0, nullptr, 0, 0, base, 0) == 2 + 1 + 5 + 1);
  // a batch error comes before the expire errors
  CHECK(record_header_put(nullptr, nullptr, 3, 4, 0, 0, nullptr, 0, base - 1, base, 0) == -BCW_ENC_ERR_BATCH);
  return 0;
}

int main() {
  if (check_framing() || check_varints() || check_headers()) return 1;
  // the public known answers: CRC-32C("123456789"), and the empty fragment's CRC-32C of 0
  if (mask_crc(0xE3069283u) != 0xC78AB0E5u || mask_crc(0) != 0xA282EAD8u) {
    std::fprintf(stderr, "frame_check: mask_crc known answers failed\n");
    return 1;
  }
  std::printf("frame_check ok: %llu walks, %llu varints, %llu headers\n", (unsigned long long)n_walks,
              (unsigned long long)n_varints, (unsigned long long)n_headers);
  return 0;
}
