// bcw_devmem.h -- host only: who owns a device allocation (DevBuf), how one allocation is cut into arrays (Carver), and
// what is cut with it: the record table's column list, written once, and the layouts of the synchronous entry points.
// The two types each hold one condition: an allocation is freed exactly once; the bytes allocated are the end of the
// very walk that hands out the pointers. tools/devmem_check.cpp compiles this against stand-ins (BCW_DEVMEM_NO_HIP).
#pragma once
#ifndef BCW_DEVMEM_NO_HIP
#include <hip/hip_runtime.h>
#endif
#include <cstdint>
#include <type_traits>
#include <utility>

#include "bcw.h"

namespace bcw {

// One device allocation. Move-only (no copy operations beside the move ones); the destructor frees.
template <class T = void>
class DevBuf {
 public:
  DevBuf() = default;
  ~DevBuf() { reset(); }
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  T* get() const { return p_; }
  uint64_t bytes() const { return bytes_; }  // the size asked for (0: nothing held)
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // frees what is held, then allocates `bytes` (> 0). false: nothing is held.
  bool alloc(uint64_t bytes) {
    reset();
    if (hipMalloc(reinterpret_cast<void**>(&p_), bytes) != hipSuccess) p_ = nullptr;
    bytes_ = p_ ? bytes : 0;
    return p_ != nullptr;
  }
  // grow-only: enough already (0 bytes of nothing included) -> true without a HIP call. Otherwise work queued on `st`
  // may still use the old allocation: synchronise, free, allocate. false: nothing is held (pointer null, size 0).
  bool reserve(uint64_t bytes, hipStream_t st) {
    if (bytes <= bytes_) return true;
    (void)hipStreamSynchronize(st);
    return alloc(bytes);
  }

 private:
  T* p_ = nullptr;
  uint64_t bytes_ = 0;
};

// Cuts one allocation into arrays. The same layout function runs twice: on a Carver() it only adds up (takes return
// null, total() is the bytes to allocate), on a Carver(base, total) it hands out the pointers. A take past the end is
// refused: null, and ok() is false for good. Offsets are aligned from the base (hipMalloc aligns that to 256 B).
class Carver {
 public:
  Carver() = default;
  Carver(void* base, uint64_t limit) : base_(static_cast<uint8_t*>(base)), limit_(limit) {}
  // n elements of T, the first aligned to `align` bytes (a power of two, sizeof(T) at least)
  template <class T>
  T* take(uint64_t n, uint64_t align = sizeof(T)) {
    const uint64_t at = (off_ + align - 1) & ~(align - 1), end = at + n * sizeof(T);
    if (base_ && end > limit_) ok_ = false;
    if (!ok_) return nullptr;
    off_ = end;
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  // bytes padded to a multiple of 16: the 16-byte units the copy kernels move stay inside their own region
  uint8_t* take_bytes16(uint64_t n) { return take<uint8_t>((n + 15) & ~15ull, 16); }
  uint64_t total() const { return off_; }
  bool ok() const { return ok_; }

 private:
  uint8_t* base_ = nullptr;
  uint64_t limit_ = 0, off_ = 0;
  bool ok_ = true;
};

// ---- the record table's columns ----
enum : unsigned { kColAux = 1, kColFrag = 2 };  // aux0 / aux1 (hint mode only); first_frag / emit_frag (decode's)
// f(a's column, b's column, kind) for every column, in struct order, until one returns false. The columns are typed
// pointers (8, 4 and 1 byte elements): f is a generic lambda and reads the element size off the pointer.
template <class A, class B, class F>
bool each_column(A& a, B& b, F&& f) {
  return f(a.foff, b.foff, 0u) && f(a.size, b.size, 0u) && f(a.expire, b.expire, 0u) && f(a.aux0, b.aux0, kColAux) &&
         f(a.aux1, b.aux1, kColAux) && f(a.key_len, b.key_len, 0u) && f(a.val_len, b.val_len, 0u) &&
         f(a.meta_len, b.meta_len, 0u) && f(a.first_frag, b.first_frag, kColFrag) &&
         f(a.emit_frag, b.emit_frag, kColFrag) && f(a.hdr_size, b.hdr_size, 0u) && f(a.flags, b.flags, 0u) &&
         f(a.etag_off, b.etag_off, 0u) && f(a.status, b.status, 0u);
}

// every column is there, but for the kinds in `optional`
inline bool table_has(const bcw_record_table& t, unsigned optional) {
  return each_column(t, t, [&](const void* col, const void*, unsigned kind) { return col || (kind & optional); });
}
// the table of a read or a get: none (status == NULL), or everything but the hint columns and the fragment ids
inline bool read_table_ok(const bcw_record_table& t) { return !t.status || table_has(t, kColAux | kColFrag); }

// a device table of n rows, with or without aux0 / aux1
inline bcw_record_table carve_table(Carver& cv, uint64_t n, bool aux) {
  bcw_record_table t{};
  t.capacity = n;
  each_column(t, t, [&](auto*& col, auto*&, unsigned kind) {
    if (aux || !(kind & kColAux)) col = cv.take<std::remove_reference_t<decltype(*col)>>(n);
    return true;
  });
  return t;
}

// rows [0, k) of every column both tables have, device -> host on `st`
inline bool table_copy_down(const bcw_record_table& h, const bcw_record_table& d, uint64_t k, hipStream_t st) {
  return each_column(h, d, [&](auto* dst, auto* src, unsigned) {
    return !dst || !src || k == 0 ||
           hipMemcpyAsync(dst, src, k * sizeof *dst, hipMemcpyDeviceToHost, st) == hipSuccess;
  });
}

// ---- the layouts ----
constexpr uint64_t kTailSlack = 64;  // headroom past the last array of a staging allocation

// measure with layout(Carver&), allocate, carve with the same layout
template <class Layout>
int carve_alloc(DevBuf<>& mem, Layout&& layout) {
  Carver measure;
  layout(measure);
  if (!mem.alloc(measure.total())) return BCW_E_NOMEM;
  Carver cv(mem.get(), measure.total());
  layout(cv);
  return cv.ok() ? BCW_OK : BCW_E_INVAL;
}

// bcw_decode_fragments: the export of n fragments
inline bcw_frag_table carve_frags(Carver& cv, uint64_t n) {
  bcw_frag_table d{};
  d.capacity = n;
  d.data_off = cv.take<uint64_t>(n);
  d.len = cv.take<uint32_t>(n);
  d.stored_crc = cv.take<uint32_t>(n);
  d.type = cv.take<uint8_t>(n);
  d.crc_ok = cv.take<uint8_t>(n);
  return d;
}

// bcw_read_records: the image, the payload slots, the requests, the optional table, the read status
struct ReadLayout {
  uint8_t *seg, *payload;
  uint64_t *off, *size, *pay_off;  // pay_off: n + 1
  bcw_record_table tab;
  uint8_t* rd_status;
};
inline ReadLayout carve_read(Carver& cv, uint64_t seg_len, uint64_t pay_bytes, uint64_t n, bool tab) {
  ReadLayout L{};
  L.seg = cv.take_bytes16(seg_len);
  L.payload = cv.take_bytes16(pay_bytes);
  L.off = cv.take<uint64_t>(n);
  L.size = cv.take<uint64_t>(n);
  L.pay_off = cv.take<uint64_t>(n + 1);
  if (tab) L.tab = carve_table(cv, n, false);
  L.rd_status = cv.take<uint8_t>(n);
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// bcw_get_records: the keys, the outputs (payload, lookup columns, optional table, the two status columns), the result
struct GetLayout {
  uint8_t* keys;
  uint64_t* key_off;  // n + 1
  bcw_get_out out;
  bcw_get_result* res;
};
inline GetLayout carve_get(Carver& cv, uint64_t key_bytes, uint64_t payload_cap, uint64_t n, bool tab) {
  GetLayout L{};
  L.keys = cv.take_bytes16(key_bytes);
  L.out.payload = cv.take_bytes16(payload_cap);
  L.out.payload_cap = payload_cap;
  L.key_off = cv.take<uint64_t>(n + 1);
  L.out.fid = cv.take<uint64_t>(n);
  L.out.off = cv.take<uint64_t>(n);
  L.out.size = cv.take<uint64_t>(n);
  L.out.pay_off = cv.take<uint64_t>(n);
  if (tab) L.out.table = carve_table(cv, n, false);
  L.out.get_status = cv.take<uint8_t>(n);
  L.out.rd_status = cv.take<uint8_t>(n);
  L.res = cv.take<bcw_get_result>(1, 16);
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// bcw_write_records: the batch, the outputs (WAL, per-record columns, the WriteStat columns if asked for), the result
struct PutLayout {
  uint8_t *keys, *vals, *metas, *etags, *flags;
  uint64_t* offs;  // key, value and meta offsets, n + 1 each, one after the other (one upload)
  uint64_t* expire;
  bcw_write_out out;
  bcw_write_result* res;
};
inline PutLayout carve_put(Carver& cv, uint64_t key_bytes, uint64_t val_bytes, uint64_t meta_bytes, uint64_t etag_bytes,
                           uint64_t wal_cap, uint64_t n, bool stat) {
  PutLayout L{};
  L.keys = cv.take_bytes16(key_bytes);
  L.vals = cv.take_bytes16(val_bytes);
  L.metas = cv.take_bytes16(meta_bytes);
  L.etags = cv.take_bytes16(etag_bytes);
  L.out.wal = cv.take_bytes16(wal_cap);
  L.out.wal_cap = wal_cap;
  L.offs = cv.take<uint64_t>(3 * (n + 1));
  L.expire = cv.take<uint64_t>(n);
  L.out.rec_off = cv.take<uint64_t>(n);
  L.out.rec_size = cv.take<uint64_t>(n);
  L.flags = cv.take_bytes16(n);
  if (stat) {
    L.out.free_fid = cv.take<uint64_t>(n);
    L.out.free_bytes = cv.take<uint64_t>(n);
    L.out.found = cv.take_bytes16(n);
  }
  L.res = cv.take<bcw_write_result>(1, 16);
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// the synchronous encode's device outputs: the record offsets of `rows` source rows, the dst WAL, the hint WAL
inline bcw_encode_out carve_encode_out(Carver& cv, uint64_t rows, uint64_t wal_cap, uint64_t hint_cap) {
  bcw_encode_out d{};
  d.rec_off = cv.take<uint64_t>(rows);
  d.rec_off_cap = rows;
  d.wal = cv.take_bytes16(wal_cap);
  d.wal_cap = wal_cap;
  d.hint = cv.take_bytes16(hint_cap);
  d.hint_cap = hint_cap;
  cv.take<uint8_t>(kTailSlack);
  return d;
}

}  // namespace bcw
