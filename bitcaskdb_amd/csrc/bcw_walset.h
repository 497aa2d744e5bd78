// bcw_walset.h -- the host side of the resident WAL set (bcw_walset, bcw_get.hip): fid -> (device image, seg_len,
// base_time), sorted by fid, the image the device kernels binary-search (manifest.ToWalWithRef, db_impl.go:589-593).
// No device calls here: the table hands back the images it owned for the caller to free, so that the insert /
// replace / remove logic builds and runs without a GPU (tools/walset_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bcw {

// one resident WAL, as the kernels read it (32 bytes)
struct WalEnt {
  uint64_t fid;
  const uint8_t* seg;  // device image of the whole file (super block included)
  uint64_t seg_len;
  uint64_t base_time;
};
static_assert(sizeof(WalEnt) == 32, "WalEnt layout");

struct WalTable {
  std::vector<WalEnt> ents;  // ascending fid, no duplicates
  std::vector<void*> owned;  // parallel to ents: the image when the set allocated it (upload), else nullptr

  // index of the first entry with fid >= f
  size_t lower(uint64_t f) const {
    size_t lo = 0, hi = ents.size();
    while (lo < hi) {
      const size_t m = lo + (hi - lo) / 2;
      if (ents[m].fid < f) lo = m + 1; else hi = m;
    }
    return lo;
  }
  bool has(uint64_t f) const {
    const size_t i = lower(f);
    return i < ents.size() && ents[i].fid == f;
  }
  // insert e, or replace the entry of its fid; own: the image if the set allocated it. Returns the image the
  // replaced entry owned (nullptr: none), which the caller frees.
  void* put(const WalEnt& e, void* own) {
    const size_t i = lower(e.fid);
    if (i < ents.size() && ents[i].fid == e.fid) {
      void* old = owned[i];
      ents[i] = e;
      owned[i] = own;
      return old;
    }
    ents.reserve(ents.size() + 1);  // both or neither: an allocation failure leaves the table as it was
    owned.reserve(owned.size() + 1);
    ents.insert(ents.begin() + (std::ptrdiff_t)i, e);
    owned.insert(owned.begin() + (std::ptrdiff_t)i, own);
    return nullptr;
  }
  // remove f's entry when present (*found says so). Returns the image it owned (nullptr: none).
  void* remove(uint64_t f, bool* found) {
    const size_t i = lower(f);
    *found = i < ents.size() && ents[i].fid == f;
    if (!*found) return nullptr;
    void* old = owned[i];
    ents.erase(ents.begin() + (std::ptrdiff_t)i);
    owned.erase(owned.begin() + (std::ptrdiff_t)i);
    return old;
  }
};

}  // namespace bcw
