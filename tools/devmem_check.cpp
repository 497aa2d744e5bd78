// devmem_check.cpp -- the host's device-memory types, column list and layouts (csrc/bcw_devmem.h) as a
// stand-alone program. No device, no library: the few HIP names the header uses are stand-ins defined here
// (BCW_DEVMEM_NO_HIP), a "device allocation" is host memory, and the stand-ins keep a log of what was called.
//   the carver: for the twelve layouts (fragments, read, get, put, encode outputs, the record table; the index's flat
//   keys, apply, get, export in both phases, usage rows, scrub queue) at n = 0, 1, 2, 255, 256, 257, with and without
//   the optional parts, byte counts 0, 1, 15, 16, 17 -- the measured total is where the carve pass ends, every pointer
//   is aligned to its element (16 B for payload, hint WAL and the result structs), the arrays do not overlap and stay
//   inside the allocation; a take past the end is refused, for good; get, index apply and index get begin with the
//   flat-key layout, export's second phase with its first;
//   the column list: the required-column sets of decode / encode and of read / get, the carve with and without the
//   hint columns, the copy that skips columns either side lacks;
//   the owner: reserve's order (synchronise, free, allocate), its fast path without a call, null / 0 and no error left
//   behind after a failed allocation, one free per allocation across moves and destruction; adopt's order (the new
//   allocation, synchronise, free of the old one), and a pair whose second allocation fails leaks nothing and leaves
//   what is held alone; carve_reserve keeps a buffer that is large enough without a call and refuses a layout whose
//   carve pass asks for more than its measure pass, however large the buffer.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ibitcaskdb_amd/csrc \
//       tools/devmem_check.cpp -o /tmp/devmem_check && /tmp/devmem_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

// ---- stand-ins for the HIP names bcw_devmem.h uses ----
typedef int hipError_t;
typedef void* hipStream_t;
constexpr hipError_t hipSuccess = 0;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
static std::string g_log;         // 'S' synchronise, 'F' free of a live pointer, 'M' allocate, 'C' copy
static int g_live = 0;            // allocations not yet freed
static bool g_fail_next = false;  // the next allocation fails
static hipError_t g_err = hipSuccess;  // the error a failed call leaves on the thread until it is read
static hipError_t hipGetLastError() { return std::exchange(g_err, hipSuccess); }
static hipError_t hipMalloc(void** p, size_t n) {
  if (g_fail_next) { g_fail_next = false; *p = reinterpret_cast<void*>(0x1); return g_err = 2; }  // garbage, as a failed call may leave
  *p = std::aligned_alloc(256, (n + 255) / 256 * 256 + 256);
  ++g_live;
  g_log += 'M';
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  if (p) { std::free(p); --g_live; g_log += 'F'; }
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t) { g_log += 'S'; return hipSuccess; }
static hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  std::memcpy(d, s, n);
  g_log += 'C';
  return hipSuccess;
}
#define BCW_DEVMEM_NO_HIP
#include "bcw_devmem.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "devmem_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace bcw;

// the arrays a layout handed out: [p, p + bytes), aligned to `align`
struct Span { const void* p; uint64_t bytes, align; };
struct Spans {
  std::vector<Span> v;
  template <class T>
  void add(const T* p, uint64_t n, uint64_t align = sizeof(T)) { v.push_back({p, n * sizeof(T), align}); }
  void add_table(const bcw_record_table& t, bool aux) {
    each_column(t, t, [&](auto* col, auto*, unsigned kind) {
      if (aux || !(kind & kColAux)) add(col, t.capacity);
      return true;
    });
  }
};
// every array aligned, inside [base, base + total), none overlapping another
static bool spans_ok(std::vector<Span> v, const void* base, uint64_t total) {
  const uintptr_t b = (uintptr_t)base;
  for (const Span& s : v)
    if (!s.p || (uintptr_t)s.p % s.align || (uintptr_t)s.p < b || (uintptr_t)s.p + s.bytes > b + total) return false;
  std::sort(v.begin(), v.end(), [](const Span& x, const Span& y) {  // empty arrays first where two begin together
    return std::make_pair((uintptr_t)x.p, x.bytes) < std::make_pair((uintptr_t)y.p, y.bytes);
  });
  for (size_t i = 1; i < v.size(); ++i)
    if ((uintptr_t)v[i - 1].p + v[i - 1].bytes > (uintptr_t)v[i].p) return false;
  return true;
}

static bool g_bad = false;  // a layout's own fields (capacities, which optional parts exist) were wrong
// one layout, both passes: the measured total is the carve's end, the pointers hold; one byte less is refused
template <class Layout>
static bool both_passes(Layout layout) {
  Carver measure;
  { Spans ignore; layout(measure, ignore); }
  const uint64_t total = measure.total();
  if (!measure.ok()) return false;
  void* base = std::aligned_alloc(256, total / 256 * 256 + 256);
  Carver cv(base, total);
  Spans sp;
  layout(cv, sp);
  bool ok = cv.ok() && cv.total() == total && spans_ok(sp.v, base, total) && !g_bad;
  if (total) {
    Carver tight(base, total - 1);
    Spans ignore;
    layout(tight, ignore);
    ok = ok && !tight.ok();
  }
  std::free(base);
  return ok;
}

// k is where the flat-key layout of (key_bytes, n) puts it when that layout begins the allocation (k.keys is the base)
static bool flat_prefix(const Carver& cv, const FlatKeys& k, uint64_t key_bytes, uint64_t n) {
  if (!k.keys || !cv.ok()) return true;  // the measuring pass, or a carve that was refused
  Carver ref(k.keys, ~0ull);
  const FlatKeys f = carve_flat_keys(ref, key_bytes, n);
  return f.keys == k.keys && f.key_off == k.key_off;
}

int main() {
  const uint64_t kN[] = {0, 1, 2, 255, 256, 257}, kBytes[] = {0, 1, 15, 16, 17};
  unsigned long long layouts = 0;
  for (uint64_t n : kN) {
    // the index's layouts: usage rows (cap = n, 0 included), the scrub queue (24 counter words, 48-byte items)
    CHECK(both_passes([&](Carver& cv, Spans& sp) {
      const UsageLayout L = carve_usage(cv, n);
      sp.add(L.res, 1, 16);
      if (n) sp.add(L.rows, n, 16);
      if (L.res && cv.ok()) g_bad |= (L.rows != nullptr) != (n != 0);
    }));
    CHECK(both_passes([&](Carver& cv, Spans& sp) {
      const VfyQueueLayout L = carve_vfy_queue(cv, 24, n, 48);
      sp.add(L.cnt, 24, 16); sp.add(static_cast<const uint8_t*>(L.queue), n * 48, 16);
    }));
    layouts += 2;
    for (uint64_t a : kBytes) {
      CHECK(both_passes([&](Carver& cv, Spans& sp) {
        const FlatKeys k = carve_flat_keys(cv, a, n);
        sp.add(k.keys, a, 16); sp.add(k.key_off, n + 1);
      }));
      CHECK(both_passes([&](Carver& cv, Spans& sp) {
        const IxApplyLayout L = carve_ix_apply(cv, a, n);
        sp.add(L.k.keys, a, 16); sp.add(L.k.key_off, n + 1); sp.add(L.fid, n); sp.add(L.off, n); sp.add(L.size, n);
        sp.add(L.free_fid, n); sp.add(L.free_bytes, n); sp.add(L.ops, n); sp.add(L.found, n);
        g_bad |= !flat_prefix(cv, L.k, a, n);
      }));
      CHECK(both_passes([&](Carver& cv, Spans& sp) {
        const IxGetLayout L = carve_ix_get(cv, a, n);
        sp.add(L.k.keys, a, 16); sp.add(L.k.key_off, n + 1); sp.add(L.fid, n); sp.add(L.off, n); sp.add(L.size, n);
        sp.add(L.status, n);
        g_bad |= !flat_prefix(cv, L.k, a, n);
      }));
      layouts += 3;
      // the export: nf selected fids (none included), n blocks; phase one, and phase two with n entries of a key
      // bytes, whose first part lies where phase one put it
      for (uint64_t nf : {0, 1, 3})
        for (bool two : {false, true}) {
          if (two && !n) continue;  // no entries: the export ends after phase one
          CHECK(both_passes([&](Carver& cv, Spans& sp) {
            const IxExportLayout L = carve_ix_export(cv, nf, n, two ? n : 0, two ? a : 0);
            sp.add(L.fids, nf, 16); sp.add(L.blk_n, n, 16); sp.add(L.blk_b, n);
            if (two) {
              sp.add(L.k.keys, a, 16); sp.add(L.k.key_off, n + 1); sp.add(L.fid, n); sp.add(L.off, n); sp.add(L.size, n);
            }
            if (!L.fids || !cv.ok()) return;  // the measuring pass, or a carve that was refused
            g_bad |= two != (L.k.keys != nullptr) || two != (L.k.key_off != nullptr) || two != (L.size != nullptr);
            Carver ref(L.fids, ~0ull);
            const IxExportLayout P = carve_ix_export(ref, nf, n, 0, 0);
            g_bad |= P.fids != L.fids || P.blk_n != L.blk_n || P.blk_b != L.blk_b;
          }));
          ++layouts;
        }
    }
    CHECK(both_passes([&](Carver& cv, Spans& sp) {
      const bcw_frag_table d = carve_frags(cv, n);
      sp.add(d.data_off, n); sp.add(d.len, n); sp.add(d.stored_crc, n); sp.add(d.type, n); sp.add(d.crc_ok, n);
    }));
    for (bool aux : {false, true})
      CHECK(both_passes([&](Carver& cv, Spans& sp) {
        const bcw_record_table t = carve_table(cv, n, aux);
        if (t.foff && cv.ok()) g_bad |= t.capacity != n || aux != (t.aux0 != nullptr) || aux != (t.aux1 != nullptr);
        sp.add_table(t, aux);
      }));
    layouts += 3;
    for (bool tab : {false, true})
      for (uint64_t a : kBytes)
        for (uint64_t b : kBytes) {
          CHECK(both_passes([&](Carver& cv, Spans& sp) {
            const ReadLayout L = carve_read(cv, a, b, n, tab);
            sp.add(L.seg, a, 16); sp.add(L.payload, b, 16); sp.add(L.off, n); sp.add(L.size, n);
            sp.add(L.pay_off, n + 1); sp.add(L.rd_status, n);
            if (tab) sp.add_table(L.tab, false);
            if (L.seg && cv.ok()) g_bad |= (L.tab.status != nullptr) != tab || L.tab.aux0 != nullptr;
          }));
          CHECK(both_passes([&](Carver& cv, Spans& sp) {
            const GetLayout L = carve_get(cv, a, b, n, tab);
            sp.add(L.k.keys, a, 16); sp.add(L.out.payload, b, 16); sp.add(L.k.key_off, n + 1); sp.add(L.out.fid, n);
            sp.add(L.out.off, n); sp.add(L.out.size, n); sp.add(L.out.pay_off, n); sp.add(L.out.get_status, n);
            sp.add(L.out.rd_status, n); sp.add(L.res, 1, 16);
            if (tab) sp.add_table(L.out.table, false);
            if (L.k.keys && cv.ok()) g_bad |= (L.out.table.status != nullptr) != tab || L.out.payload_cap != b;
            g_bad |= !flat_prefix(cv, L.k, a, n);
          }));
          CHECK(both_passes([&](Carver& cv, Spans& sp) {
            const bcw_encode_out d = carve_encode_out(cv, n, a, b);
            sp.add(d.rec_off, n); sp.add(d.wal, a, 16); sp.add(d.hint, b, 16);
            g_bad |= d.rec_off_cap != n || d.wal_cap != a || d.hint_cap != b;
          }));
          layouts += 3;
          // the write: its optional part is the WriteStat columns; key / value bytes a, b, the rest from both
          CHECK(both_passes([&](Carver& cv, Spans& sp) {
            const PutLayout L = carve_put(cv, a, b, (a + b) % 18, b ? 8 * n : 0, a * 7 + b, n, tab);
            sp.add(L.keys, a, 16); sp.add(L.vals, b, 16); sp.add(L.metas, (a + b) % 18, 16);
            sp.add(L.etags, b ? 8 * n : 0, 16); sp.add(L.out.wal, a * 7 + b, 16); sp.add(L.offs, 3 * (n + 1));
            sp.add(L.expire, n); sp.add(L.out.rec_off, n); sp.add(L.out.rec_size, n); sp.add(L.flags, n, 16);
            sp.add(L.res, 1, 16);
            if (tab) { sp.add(L.out.free_fid, n); sp.add(L.out.free_bytes, n); sp.add(L.out.found, n, 16); }
            if (L.keys && cv.ok())
              g_bad |= L.out.wal_cap != a * 7 + b || (tab != (L.out.found != nullptr)) || (tab != (L.out.free_fid != nullptr));
          }));
          ++layouts;
        }
  }
  {  // a take past the end is refused: null, nothing handed out afterwards either, a measuring carver never refuses
    alignas(16) uint8_t buf[64];
    Carver cv(buf, 40);
    CHECK(cv.take<uint64_t>(4) == (uint64_t*)buf && cv.ok());
    CHECK(cv.take<uint8_t>(1) == buf + 32);
    CHECK(cv.take<uint32_t>(1) == (uint32_t*)(buf + 36) && cv.total() == 40 && cv.ok());  // to the very end
    CHECK(cv.take<uint8_t>(0) == buf + 40 && cv.ok());
    CHECK(cv.take<uint8_t>(1) == nullptr && !cv.ok());
    CHECK(cv.take<uint8_t>(0) == nullptr && !cv.ok() && cv.total() == 40);
    Carver al(buf, 40);  // the alignment gap counts: 33 rounds up to 48
    CHECK(al.take<uint8_t>(33) == buf && al.take<uint8_t>(1, 16) == nullptr && !al.ok());
    Carver m;
    CHECK(m.take<uint64_t>(1ull << 40) == nullptr && m.ok() && m.total() == 8ull << 40);
    CHECK(m.take_bytes16(17) == nullptr && m.total() == (8ull << 40) + 32);
  }
  {  // the column list
    uint64_t a8[4] = {1, 2, 3, 4};
    uint32_t a4[4] = {5, 6, 7, 8};
    uint8_t a1[4] = {9, 10, 11, 12};
    bcw_record_table t{4, a8, a8, a8, nullptr, nullptr, a4, a4, a4, a4, a4, a1, a1, a1, a1};
    int cols = 0;
    each_column(t, t, [&](auto* c, auto*, unsigned) { cols += (int)sizeof *c; return true; });
    CHECK(cols == 5 * 8 + 5 * 4 + 4);  // 14 columns, 64 B a row
    CHECK(table_has(t, kColAux) && !table_has(t, 0) && read_table_ok(t));
    bcw_record_table u = t;
    u.first_frag = nullptr;
    CHECK(!table_has(u, kColAux) && read_table_ok(u));  // decode and encode need the fragment ids, read and get do not
    u.emit_frag = nullptr;
    u.flags = nullptr;
    CHECK(!read_table_ok(u));
    u = bcw_record_table{};
    CHECK(read_table_ok(u) && !table_has(u, kColAux | kColFrag));  // status == NULL: no table
    // the copy: k rows of the columns both sides have
    uint64_t h8[4] = {0, 0, 0, 0}, h8b[4] = {0, 0, 0, 0};
    uint8_t h1[4] = {0, 0, 0, 0};
    bcw_record_table h{};
    h.foff = h8;
    h.aux0 = h8b;  // the device side has none
    h.status = h1;
    g_log.clear();
    CHECK(table_copy_down(h, t, 3, nullptr) && g_log == "CC");
    CHECK(h8[0] == 1 && h8[2] == 3 && h8[3] == 0 && h8b[0] == 0 && h1[2] == 11 && h1[3] == 0);
    g_log.clear();
    CHECK(table_copy_down(h, t, 0, nullptr) && g_log.empty());
  }
  {  // the owner
    g_log.clear();
    {
      DevBuf<uint32_t> b;
      CHECK(!b && b.get() == nullptr && b.bytes() == 0);
      CHECK(b.reserve(0, nullptr) && g_log.empty() && !b);  // nothing asked, nothing done
      CHECK(b.reserve(100, nullptr) && g_log == "SM" && b && b.bytes() == 100);
      uint32_t* p = b.get();
      CHECK(b.reserve(100, nullptr) && b.reserve(7, nullptr) && g_log == "SM" && b.get() == p);  // the fast path
      CHECK(b.reserve(101, nullptr) && g_log == "SMSFM" && b.bytes() == 101);  // synchronise, free, allocate
      g_fail_next = true;
      CHECK(!b.reserve(200, nullptr) && g_log == "SMSFMSF" && !b && b.get() == nullptr && b.bytes() == 0);
      CHECK(g_err == hipSuccess);  // the failed call's error does not wait for a later check of a launch
      CHECK(b.reserve(1, nullptr) && g_log == "SMSFMSFSM" && g_live == 1);
      DevBuf<uint32_t> c(std::move(b));
      CHECK(!b && b.bytes() == 0 && c && c.bytes() == 1 && g_live == 1);
      DevBuf<uint32_t> d;
      CHECK(d.alloc(8) && g_live == 2);
      d = std::move(c);  // frees what d held
      CHECK(g_live == 1 && !c && d.bytes() == 1);
      struct Two { DevBuf<> x; DevBuf<uint8_t> y; int keep = 3; } two;
      CHECK(two.x.alloc(1) && two.y.alloc(1) && g_live == 3);
      two = Two{};  // how the scratch structs drop everything
      CHECK(g_live == 1 && !two.x && !two.y);
      DevBuf<> mem;
      bcw_frag_table ft{};
      CHECK(carve_alloc(mem, [&](Carver& cv) { ft = carve_frags(cv, 3); }) == BCW_OK && mem.bytes() == 54 && ft.crc_ok);
      g_fail_next = true;
      CHECK(carve_alloc(mem, [&](Carver& cv) { ft = carve_frags(cv, 3); }) == BCW_E_NOMEM && !mem);
    }
    CHECK(g_live == 0);  // every allocation freed once
  }
  {  // adopt: the larger buffer of ix_grow / ix_compact / the walset's growth
    {
      DevBuf<uint32_t> held, other;
      CHECK(held.alloc(8) && other.alloc(8) && g_live == 2);
      const uint32_t *h0 = held.get(), *o0 = other.get();
      g_log.clear();
      {
        DevBuf<uint32_t> nw;
        CHECK(nw.alloc(16));
        const uint32_t* pn = nw.get();
        held.adopt(std::move(nw), nullptr);
        CHECK(!nw && held.get() == pn && held.bytes() == 16 && pn != h0);
      }
      CHECK(g_log == "MSF" && g_live == 2);  // the new allocation, the synchronise, the free of the old one: once
      DevBuf<uint32_t> empty, nw;
      CHECK(nw.alloc(4));
      g_log.clear();
      empty.adopt(std::move(nw), nullptr);
      CHECK(g_log == "S" && empty && !nw && g_live == 3);  // nothing was held: nothing freed
      const uint32_t* h1 = held.get();
      g_log.clear();
      {  // a pair whose second allocation fails: the caller returns before any adopt
        DevBuf<uint32_t> na, nb;
        CHECK(na.alloc(32) && g_live == 4);
        g_fail_next = true;
        CHECK(!nb.alloc(32) && !nb && g_err == hipSuccess);
      }
      CHECK(g_log == "MF" && g_live == 3 && held.get() == h1 && held.bytes() == 16 && other.get() == o0);
    }
    CHECK(g_live == 0);
  }
  {  // carve_reserve
    {
      DevBuf<> st;
      FlatKeys k{};
      g_log.clear();
      CHECK(carve_reserve(st, nullptr, [&](Carver& cv) { k = carve_flat_keys(cv, 17, 2); }) == BCW_OK);
      CHECK(g_log == "SM" && st.bytes() == 32 + 24 && k.keys == st.get() && k.key_off);
      void* p = st.get();
      CHECK(carve_reserve(st, nullptr, [&](Carver& cv) { k = carve_flat_keys(cv, 1, 1); }) == BCW_OK);
      CHECK(g_log == "SM" && st.get() == p && st.bytes() == 56 && k.keys == p);  // large enough: kept, no call
      int pass = 0;  // 9 bytes fit the buffer, not the 8 that were measured
      CHECK(carve_reserve(st, nullptr, [&](Carver& cv) { cv.take<uint8_t>(pass++ ? 9 : 8); }) == BCW_E_INVAL);
      CHECK(g_log == "SM" && st.get() == p);
      g_fail_next = true;
      CHECK(carve_reserve(st, nullptr, [&](Carver& cv) { k = carve_flat_keys(cv, 64, 2); }) == BCW_E_NOMEM);
      CHECK(g_log == "SMSF" && !st && st.bytes() == 0 && g_err == hipSuccess);
    }
    CHECK(g_live == 0);
  }
  std::printf("devmem_check ok: %llu layouts\n", layouts);
  return 0;
}
