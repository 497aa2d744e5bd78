// bcw_usage.hip -- the reduction core of the per-WAL space accounting (bcw_usage.h): the context's global table, the
// final kernel that turns it into sorted rows, and the pass over the WriteStat columns of a write
// (bcw_freed_by_fid_async). The pass over the index lives with the slot table (bcw_index.hip, k_ix_usage).
//
// No workgroup waits for another: every pass only adds into the table (compare-and-swap claims and 64-bit adds), and
// the final kernel is a launch of its own behind them on the stream. Integer sums and sorted rows make the output
// the same from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bcw_host.h"
#include "bcw_usage.h"

namespace bcw {
namespace usage {

// rows {free_fid[i], found[i] != 0, free_bytes[i], 0} of ops [0, n), or none when the gate says the batch was rejected
__global__ __launch_bounds__(kThreads) void k_usage_rows(uint64_t n, const uint8_t* __restrict__ found,
                                                         const uint64_t* __restrict__ ffid,
                                                         const uint64_t* __restrict__ fbytes,
                                                         const bcw_write_result* __restrict__ gate,
                                                         uint64_t* __restrict__ scratch) {
  __shared__ Accum acc;
  acc.init();
  const Table g = table_of(scratch);
  const uint64_t ne = (gate && gate->n_written == 0) ? 0 : n;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < ne; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t i = base + threadIdx.x;
    const bool valid = i < ne;
    uint64_t f = 0, b = 0;
    bool hit = false;
    if (valid) {
      f = ffid[i];
      b = fbytes[i];
      hit = found[i] != 0;
    }
    acc.add(g, valid, f, hit, b, 0);
  }
  acc.flush(g);
}

constexpr uint32_t kFinalThreads = 1024;
constexpr uint16_t kPad = 0xffffu;  // no table entry (kEntries <= 0xffff)

// One workgroup: the occupied entries of the table into LDS, a bitonic sort by fid (distinct keys; the pads of the
// power-of-two tail compare above every fid), then rows, totals and result.
__global__ __launch_bounds__(kFinalThreads) void k_usage_final(uint64_t* __restrict__ scratch,
                                                               bcw_fid_usage* __restrict__ rows, uint32_t cap,
                                                               bcw_usage_result* __restrict__ res, int index_pass) {
  __shared__ uint64_t key[BCW_USAGE_MAX_FIDS];
  __shared__ uint16_t idx[BCW_USAGE_MAX_FIDS];
  __shared__ uint32_t s_n;
  __shared__ unsigned long long s_tot[3];
  const Table g = table_of(scratch);
  const uint32_t tid = threadIdx.x;
  if (tid == 0) { s_n = 0; s_tot[0] = s_tot[1] = s_tot[2] = 0; }
  __syncthreads();
  const bool ovf = g.aux[A_OVERFLOW] != 0;
  if (!ovf)
    for (uint32_t e = tid; e < kEntries; e += kFinalThreads)
      if (g.tag[e]) {
        const uint32_t p = atomicAdd(&s_n, 1u);
        if (p < BCW_USAGE_MAX_FIDS) {
          key[p] = e == kSlots ? 0ull : (uint64_t)g.tag[e];
          idx[p] = (uint16_t)e;
        }
      }
  __syncthreads();
  const uint32_t n = s_n;
  bcw_usage_result o{};
  if (index_pass) {
    o.soft_deleted = g.aux[A_SOFT];
    o.invalid = g.aux[A_INVALID];
  }
  if (ovf || n > BCW_USAGE_MAX_FIDS) {  // the cap is the design: nothing but the result is written
    if (tid == 0) {
      o.n_fids = ovf ? (uint64_t)g.aux[A_CLAIMED] + (g.tag[kSlots] ? 1 : 0) : n;
      o.overflow = 1;
      *res = o;
    }
    return;
  }
  uint32_t m = 1;
  while (m < n) m <<= 1;
  for (uint32_t i = n + tid; i < m; i += kFinalThreads) { key[i] = 0; idx[i] = kPad; }
  __syncthreads();
  for (uint32_t k = 2; k <= m; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < m; i += kFinalThreads) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t ka = key[i], kb = key[l];
          const uint16_t ia = idx[i], ib = idx[l];
          const bool a_lt_b = ia != kPad && (ib == kPad || ka < kb);
          const bool b_lt_a = ib != kPad && (ia == kPad || kb < ka);
          if ((i & k) == 0 ? b_lt_a : a_lt_b) {
            key[i] = kb; key[l] = ka;
            idx[i] = ib; idx[l] = ia;
          }
        }
      }
      __syncthreads();
    }
  const bool fits = n <= cap;
  uint64_t tc = 0, tb = 0, ts = 0;
  for (uint32_t i = tid; i < n; i += kFinalThreads) {
    const uint32_t e = idx[i];
    const bcw_fid_usage r{key[i], g.cnt[e], g.bytes[e], g.span[e]};
    tc += r.count;
    tb += r.bytes;
    ts += r.span;
    if (fits) rows[i] = r;
  }
  if (tc) atomicAdd(&s_tot[0], (unsigned long long)tc);
  if (tb) atomicAdd(&s_tot[1], (unsigned long long)tb);
  if (ts) atomicAdd(&s_tot[2], (unsigned long long)ts);
  __syncthreads();
  if (tid == 0) {
    o.n_fids = n;
    o.count = s_tot[0];
    o.bytes = s_tot[1];
    o.span = s_tot[2];
    o.fits = fits ? 1u : 0u;
    *res = o;
  }
}

}  // namespace usage

int usage_begin(bcw_ctx* c, hipStream_t st, uint64_t** scratch) {
  if (!c->usage && !c->usage.alloc(usage::kScratchWords * sizeof(uint64_t))) return BCW_E_NOMEM;
  if (hipMemsetAsync(c->usage.get(), 0, usage::kScratchWords * sizeof(uint64_t), st) != hipSuccess) return BCW_E_HIP;
  *scratch = c->usage.get();
  return BCW_OK;
}

int usage_finish(bcw_ctx* c, hipStream_t st, bcw_fid_usage* d_rows, uint32_t cap, bcw_usage_result* d_res,
                 int index_pass) {
  hipEvent_t ev = nullptr;
  c->prof.begin(K_USAGE_FINAL, st, ev);
  usage::k_usage_final<<<1, usage::kFinalThreads, 0, st>>>(c->usage.get(), d_rows, cap, d_res, index_pass);
  c->prof.end(K_USAGE_FINAL, st, ev);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

}  // namespace bcw

using namespace bcw;

extern "C" {

int bcw_freed_by_fid_async(bcw_index* ix, uint64_t n, const uint8_t* d_found, const uint64_t* d_free_fid,
                           const uint64_t* d_free_bytes, const bcw_write_result* d_gate, bcw_fid_usage* d_rows,
                           uint32_t cap, bcw_usage_result* d_res) {
  if (!ix || !d_res || (cap && !d_rows)) return BCW_E_INVAL;
  if (n && (!d_found || !d_free_fid || !d_free_bytes)) return BCW_E_INVAL;
  bcw_ctx* c = index_ctx(ix);
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  uint64_t* scratch = nullptr;
  const int rc = usage_begin(c, st, &scratch);
  if (rc != BCW_OK) return rc;
  if (n) {
    const uint64_t wgs = (n + usage::kThreads - 1) / usage::kThreads;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)c->num_cus * 8);
    hipEvent_t ev = nullptr;
    c->prof.begin(K_USAGE_ROWS, st, ev);
    usage::k_usage_rows<<<grid, usage::kThreads, 0, st>>>(n, d_found, d_free_fid, d_free_bytes, d_gate, scratch);
    c->prof.end(K_USAGE_ROWS, st, ev);
    if (hipGetLastError() != hipSuccess) return BCW_E_HIP;
  }
  return usage_finish(c, st, d_rows, cap, d_res, 0);
}

}  // extern "C"
