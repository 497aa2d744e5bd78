// bcw_devmem.h -- host only: who owns a device allocation (DevBuf), how one allocation is cut into arrays (Carver), and
// what is cut with it: the record table's column list, written once, and every layout of the library: the synchronous
// entry points' (fragments, read, get, put, encode outputs) and the index's (flat keys, apply, get, export, usage
// rows, scrub queue, scan scratch).
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
  // frees what is held, then allocates `bytes` (> 0). false: nothing is held, and the failed call's error is taken
  // off the thread, so that it is not found by a later check of a launch.
  bool alloc(uint64_t bytes) {
    reset();
    if (hipMalloc(reinterpret_cast<void**>(&p_), bytes) != hipSuccess) {
      (void)hipGetLastError();
      p_ = nullptr;
    }
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
  // replace: `nw` was allocated (and filled on `st`) while work queued on `st` could still read what is held, so the
  // old allocation goes only once the stream has drained. Until the call nothing of *this has changed: a caller that
  // fails before it simply returns, and its local `nw` frees itself.
  void adopt(DevBuf&& nw, hipStream_t st) {
    (void)hipStreamSynchronize(st);
    *this = std::move(nw);
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
// the same for a grow-only buffer (DevBuf::reserve on `st`). The limit of the carve is the measured total, not what
// the buffer happens to hold: a layout whose second pass asks for more than its first is refused, not absorbed.
template <class Layout>
int carve_reserve(DevBuf<>& mem, hipStream_t st, Layout&& layout) {
  Carver measure;
  layout(measure);
  if (!mem.reserve(measure.total(), st)) return BCW_E_NOMEM;
  Carver cv(mem.get(), measure.total());
  layout(cv);
  return cv.ok() ? BCW_OK : BCW_E_INVAL;
}

// b bytes device -> host on `st`, unless there is nowhere to put them or nothing to copy; host -> device likewise
inline bool copy_down(void* dst, const void* src, uint64_t b, hipStream_t st) {
  return !dst || b == 0 || hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, st) == hipSuccess;
}
inline bool copy_up(void* dst, const void* src, uint64_t b, hipStream_t st) {
  return b == 0 || hipMemcpyAsync(dst, src, b, hipMemcpyHostToDevice, st) == hipSuccess;
}

// the flat keys of a host call: key i = keys[key_off[i], key_off[i + 1])
struct FlatKeys {
  uint8_t* keys;
  uint64_t* key_off;  // n + 1
};
inline FlatKeys carve_flat_keys(Carver& cv, uint64_t key_bytes, uint64_t n) {
  return {cv.take_bytes16(key_bytes), cv.take<uint64_t>(n + 1)};  // a braced list: in this order
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
  FlatKeys k;
  bcw_get_out out;
  bcw_get_result* res;
};
inline GetLayout carve_get(Carver& cv, uint64_t key_bytes, uint64_t payload_cap, uint64_t n, bool tab) {
  GetLayout L{};
  L.k = carve_flat_keys(cv, key_bytes, n);
  L.out.payload = cv.take_bytes16(payload_cap);
  L.out.payload_cap = payload_cap;
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

// ---- the index's layouts (bcw_index.hip) ----
// bcw_index_apply_stat: the keys, the values, the two WriteStat columns (old fid, old size), the ops, found
struct IxApplyLayout {
  FlatKeys k;
  uint64_t *fid, *off, *size, *free_fid, *free_bytes;
  uint8_t *ops, *found;
};
inline IxApplyLayout carve_ix_apply(Carver& cv, uint64_t key_bytes, uint64_t n) {
  IxApplyLayout L{};
  L.k = carve_flat_keys(cv, key_bytes, n);
  L.fid = cv.take<uint64_t>(n);
  L.off = cv.take<uint64_t>(n);
  L.size = cv.take<uint64_t>(n);
  L.free_fid = cv.take<uint64_t>(n);
  L.free_bytes = cv.take<uint64_t>(n);
  L.ops = cv.take<uint8_t>(n);
  L.found = cv.take<uint8_t>(n);
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// bcw_index_get: the keys, the values, the status
struct IxGetLayout {
  FlatKeys k;
  uint64_t *fid, *off, *size;
  uint8_t* status;
};
inline IxGetLayout carve_ix_get(Carver& cv, uint64_t key_bytes, uint64_t n) {
  IxGetLayout L{};
  L.k = carve_flat_keys(cv, key_bytes, n);
  L.fid = cv.take<uint64_t>(n);
  L.off = cv.take<uint64_t>(n);
  L.size = cv.take<uint64_t>(n);
  L.status = cv.take<uint8_t>(n);
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// ix_export: the nf selected fids, then per 256-slot block the entry count and the key bytes (phase one: tn = tb = 0;
// phase two holds their exclusive prefixes there), then the tn entries with tb key bytes (phase two). The phase-one
// part of both phases is the same, whatever follows it.
struct IxExportLayout {
  uint64_t *fids, *blk_n, *blk_b;
  FlatKeys k;  // tn + 1 offsets
  uint64_t *fid, *off, *size;
};
inline IxExportLayout carve_ix_export(Carver& cv, uint64_t nf, uint64_t nblk, uint64_t tn, uint64_t tb) {
  IxExportLayout L{};
  L.fids = cv.take<uint64_t>(nf, 16);
  L.blk_n = cv.take<uint64_t>(nblk, 16);
  L.blk_b = cv.take<uint64_t>(nblk);
  if (tn) {
    L.k = carve_flat_keys(cv, tb, tn);
    L.fid = cv.take<uint64_t>(tn);
    L.off = cv.take<uint64_t>(tn);
    L.size = cv.take<uint64_t>(tn);
  }
  cv.take<uint8_t>(kTailSlack);
  return L;
}

// bcw_index_fid_usage / bcw_index_drop_fids: the result, then cap rows (cap == 0: none)
struct UsageLayout {
  bcw_usage_result* res;
  bcw_fid_usage* rows;
};
inline UsageLayout carve_usage(Carver& cv, uint64_t cap) {
  return {cv.take<bcw_usage_result>(1, 16), cap ? cv.take<bcw_fid_usage>(cap, 16) : nullptr};
}

// the scrub: `words` counter words (vfy::V_NUM), then one work item of item_bytes (vfy::Item) per slot
struct VfyQueueLayout {
  unsigned long long* cnt;
  void* queue;
};
inline VfyQueueLayout carve_vfy_queue(Carver& cv, uint64_t words, uint64_t slots, uint64_t item_bytes) {
  return {cv.take<unsigned long long>(words, 16), cv.take<uint8_t>(slots * item_bytes, 16)};
}

// the scan by prefix: the packed prefix table (table_bytes: rules::PrefixTable), `words` accumulator words (the group
// rows and the live count, scan::kAccWords), per tile of 256 slots its listed entries and their key bytes (then their
// exclusive prefixes), and a verdict byte per slot
struct IxScanLayout {
  void* table;
  unsigned long long* acc;
  uint64_t *tile_n, *tile_b;
  uint8_t* verdict;
};
inline IxScanLayout carve_ix_scan(Carver& cv, uint64_t table_bytes, uint64_t words, uint64_t tiles, uint64_t slots) {
  return {cv.take<uint8_t>(table_bytes, 16), cv.take<unsigned long long>(words, 16), cv.take<uint64_t>(tiles, 16),
          cv.take<uint64_t>(tiles), cv.take_bytes16(slots)};  // a braced list: in this order
}

}  // namespace bcw
