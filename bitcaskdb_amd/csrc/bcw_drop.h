// bcw_drop.h -- which index entries a set of WAL fids selects (bcw_index_drop_fids*, bcw_index_export_fids; bcw.h):
// the membership test over a sorted fid list, the drop's selection predicate (mode, soft-delete exemption) and the
// normalisation of a caller's list with its validation. Plain inline functions shared by the host (bcw_index.hip's
// entry points), the kernels that walk the slot table (k_ix_drop, k_ix_count, k_ix_export) and the stand-alone host
// check (tools/drop_check.cpp), as bcw_rules.h and bcw_usage.h are: one text, compiled by all three. No device calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "bcw.h"

#if defined(__HIPCC__)
#define BCW_DROP_FN __host__ __device__ __forceinline__
#else
#define BCW_DROP_FN inline
#endif

namespace bcw {
namespace drop {

// f is one of fids[0, nf): ascending, distinct. An empty list holds nothing (callers whose empty list means "all"
// say so themselves).
BCW_DROP_FN bool fid_in(const uint64_t* fids, uint32_t nf, uint64_t f) {
  uint32_t lo = 0, hi = nf;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (fids[m] < f) lo = m + 1; else hi = m;
  }
  return lo < nf && fids[lo] == f;
}

// the same answer with the list's [min, max] range tried first: an entry of a file outside it costs no search
BCW_DROP_FN bool fid_in_range(const uint64_t* fids, uint32_t nf, uint64_t f) {
  if (nf == 0 || f < fids[0] || f > fids[nf - 1]) return false;
  return fid_in(fids, nf, f);
}

BCW_DROP_FN bool known_mode(int mode) { return mode == BCW_DROP_IN || mode == BCW_DROP_NOT_IN; }

// An entry is dropped iff it is live, names a file (off != 0: a soft-deleted entry names none and always stays) and
// its fid's membership in the list is what the mode asks for. 0 < off < 40 is selected like any other offset.
BCW_DROP_FN bool selected(int mode, bool live, uint64_t off, bool member) {
  return live && off != 0 && member == (mode == BCW_DROP_IN);
}

// A caller's list (any order, duplicates allowed, any uint64) as the kernels read it: ascending and distinct.
// BCW_E_INVAL for an unknown mode, a NULL list with n > 0, or more than BCW_USAGE_MAX_FIDS distinct fids.
inline int normalise(int mode, const uint64_t* h_fids, uint32_t n, std::vector<uint64_t>* out) {
  out->clear();
  if (!known_mode(mode) || (n && !h_fids)) return BCW_E_INVAL;
  if (n) out->assign(h_fids, h_fids + n);
  std::sort(out->begin(), out->end());
  out->erase(std::unique(out->begin(), out->end()), out->end());
  return out->size() > BCW_USAGE_MAX_FIDS ? BCW_E_INVAL : BCW_OK;
}

}  // namespace drop
}  // namespace bcw
