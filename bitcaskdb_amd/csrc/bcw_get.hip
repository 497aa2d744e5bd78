// bcw_get.hip -- batched Get by key (DBImpl.Get, db_impl.go:567-587): keys -> index -> record bytes without leaving
// HBM. The resident WAL set (bcw_walset) is manifest.ToWalWithRef (getWalRef, db_impl.go:589-593): fid -> (device
// image, seg_len, base_time) as a device array sorted by fid.
//
// A get is four stream-ordered launches:
//   k_get_lookup   (bcw_index.hip) one lane per key: murmur3, probe, the fid in the set, ReadRecord's span check;
//                  the request's payload slot size and each 256-key workgroup's slot sum
//   k_get_scan     one workgroup: exclusive scan of the workgroup sums, payload_need, fits, n_found
//   k_get_offsets  each 256-key workgroup scans its slot sizes from its base: pay_off, in request order (no atomic
//                  allocation: the layout never depends on scheduling)
//   k_get_read     one wave per request (waves stride over the requests): the body of k_read_records
//                  (bcw_read_body.h) against the request's own image and base time, the copy in 16 B units
// When the payload does not fit (fits == 0) k_get_read returns at once: nothing but the lookup columns is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "bcw_host.h"
#include "bcw_read_body.h"

struct bcw_walset {
  bcw_ctx* ctx = nullptr;
  bcw::WalTable t;
  bcw::DevBuf<bcw::WalEnt> d_ents;  // the device copy of t.ents ([d_cap])
  uint64_t d_cap = 0;
  bcw::DevBuf<uint64_t> d_blk;      // [2 * blk_cap] per lookup workgroup: slot sums, then found counts
  uint64_t blk_cap = 0;
};

namespace bcw {
namespace get {

constexpr int kScanThreads = 1024;
constexpr int kWaves = 4;

// wave-inclusive scan
__device__ __forceinline__ uint64_t wave_incl(uint64_t v, uint32_t lane) {
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += t;
  }
  return incl;
}

// exclusive scan of v over the workgroup's `waves` waves; *total: the workgroup's sum. s_w: `waves` LDS words. Ends
// with a barrier, so s_w may be reused at once.
__device__ __forceinline__ uint64_t block_excl(uint64_t v, uint64_t* s_w, uint32_t waves, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_incl(v, lane);
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
  for (uint32_t w = 0; w < waves; ++w) {
    if (w < wave) pre += s_w[w];
    tot += s_w[w];
  }
  __syncthreads();
  *total = tot;
  return pre + incl - v;
}

__global__ __launch_bounds__(kScanThreads) void k_get_scan(uint64_t* __restrict__ bsum,
                                                           const uint64_t* __restrict__ bfound, uint64_t nb,
                                                           uint64_t payload_cap, bcw_get_result* __restrict__ res) {
  __shared__ uint64_t s_w[kScanThreads / 64];
  const uint32_t tid = threadIdx.x;
  uint64_t carry = 0, found = 0;
  for (uint64_t base = 0; base < nb; base += kScanThreads) {
    const uint64_t i = base + tid;
    const uint64_t v = i < nb ? bsum[i] : 0;
    found += i < nb ? bfound[i] : 0;
    uint64_t tot;
    const uint64_t ex = block_excl(v, s_w, kScanThreads / 64, &tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
  }
  uint64_t nfound;
  (void)block_excl(found, s_w, kScanThreads / 64, &nfound);
  if (tid == 0) {
    bcw_get_result r{};
    r.n_found = nfound;
    r.n_ok = 0;  // k_get_read counts
    r.payload_need = carry;
    r.fits = carry <= payload_cap ? 1u : 0u;
    *res = r;
  }
}

__global__ __launch_bounds__(kGetLookupKeys) void k_get_offsets(uint64_t* __restrict__ pay_off, uint64_t n,
                                                                const uint64_t* __restrict__ bsum) {
  __shared__ uint64_t s_w[kGetLookupKeys / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kGetLookupKeys + threadIdx.x;
  const uint64_t v = i < n ? pay_off[i] : 0;
  uint64_t tot;
  const uint64_t ex = block_excl(v, s_w, kGetLookupKeys / 64, &tot);
  if (i < n) pay_off[i] = bsum[blockIdx.x] + ex;
}

struct ReadArgs {
  const WalEnt* wals;
  uint32_t n_wals;
  bcw_get_params p;
  uint64_t n;
  bcw_get_out out;
  bcw_get_result* res;
  const uint32_t* pow2;   // [kPow2Ops][8][16] nibble images of A_{8 * 2^k}
  const uint32_t* initc;  // A_{8L}(0xFFFFFFFF)
};

__global__ __launch_bounds__(64 * kWaves) void k_get_read(ReadArgs A) {
  __shared__ uint32_t t0[256];
  __shared__ uint32_t sp2[kPow2Ops * 128];
  __shared__ uint64_t s_fo[kWaves][rd::kMaxF];
  __shared__ uint32_t s_fl[kWaves][rd::kMaxF];
  if (!A.res->fits) return;  // the whole grid: no payload byte, no table row
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (A.p.verify) rd::load_verify_tables(t0, sp2, A.pow2, tid, 64 * kWaves);
  __syncthreads();
  const bool tab = A.out.table.status != nullptr;
  uint64_t n_ok = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < A.n; r += (uint64_t)gridDim.x * kWaves) {
    const uint64_t off = A.out.off[r], size = A.out.size[r];
    uint32_t gs = A.out.get_status[r];
    if (gs != BCW_GET_OK) {  // decided by the lookup
      if (tab && lane == 0) rd::write_row(A.out.table, r, off, size, 0, rd::ReadRow{});
      continue;
    }
    const uint64_t fid = A.out.fid[r];
    uint32_t lo = 0, hi = A.n_wals;
    while (lo < hi) {
      const uint32_t m = (lo + hi) >> 1;
      if (A.wals[m].fid < fid) lo = m + 1; else hi = m;
    }
    const WalEnt W = A.wals[lo < A.n_wals ? lo : 0];  // the lookup found fid in this same set
    const rd::ReadEnv E{W.seg, W.seg_len, A.p.verify, t0, sp2, A.initc, s_fo[wave], s_fl[wave]};
    uint32_t nf = 0;
    // size <= seg_len and off in [40, seg_len] (k_get_lookup): WalRecordSize's loop is bounded by the image
    const uint32_t st = rd::read_walk<true>(E, off, size, rd::wal_record_size(off, size),
                                            A.out.payload + A.out.pay_off[r], lane, nf);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane != 0) continue;
    rd::ReadRow R;
    if (st == BCW_RD_OK) R = rd::read_parse(E, W.base_time, A.p.ns_size, A.p.etag_size, size, nf);
    gs = st != BCW_RD_OK ? BCW_GET_READ : R.status != BCW_ST_OK ? BCW_GET_RECORD : BCW_GET_OK;
    A.out.rd_status[r] = (uint8_t)st;
    A.out.get_status[r] = (uint8_t)gs;
    if (tab) rd::write_row(A.out.table, r, off, size, nf, R);
    n_ok += gs == BCW_GET_OK ? 1 : 0;
  }
  if (lane == 0 && n_ok) atomicAdd(reinterpret_cast<unsigned long long*>(&A.res->n_ok), (unsigned long long)n_ok);
}

}  // namespace get
}  // namespace bcw

namespace bcw {
bcw_ctx* walset_ctx(const bcw_walset* ws) { return ws ? ws->ctx : nullptr; }
const WalEnt* walset_device(const bcw_walset* ws, uint32_t* n_wals) {
  *n_wals = (uint32_t)ws->t.ents.size();
  return ws->d_ents.get();
}
}  // namespace bcw

using namespace bcw;

namespace {

// the device copy of the set follows the host table, after the gets already queued
int ws_publish(bcw_walset* ws) {
  hipStream_t st = ws->ctx->cur;
  const uint64_t n = ws->t.ents.size();
  if (n > ws->d_cap) {
    const uint64_t cap = std::max<uint64_t>(16, std::max(n, ws->d_cap * 2));
    DevBuf<WalEnt> d;  // the new one first: the old copy stays valid when there is no room
    if (!d.alloc(cap * sizeof(WalEnt))) return BCW_E_NOMEM;
    ws->d_ents.adopt(std::move(d), st);
    ws->d_cap = cap;
  }
  if (n && hipMemcpyAsync(ws->d_ents.get(), ws->t.ents.data(), n * sizeof(WalEnt), hipMemcpyHostToDevice, st) != hipSuccess)
    return BCW_E_HIP;
  // the host table may change again as soon as this returns
  return hipStreamSynchronize(st) == hipSuccess ? BCW_OK : BCW_E_HIP;
}

// an image the set owned, once no queued get can read it
void ws_free_image(bcw_walset* ws, void* img) {
  if (!img) return;
  (void)hipStreamSynchronize(ws->ctx->cur);
  (void)hipFree(img);
}

int ws_put(bcw_walset* ws, const WalEnt& e, void* own) {
  void* old = nullptr;
  try {
    old = ws->t.put(e, own);
  } catch (const std::bad_alloc&) {
    return BCW_E_NOMEM;
  }
  const int rc = ws_publish(ws);
  ws_free_image(ws, old);
  return rc;
}

}  // namespace

extern "C" {

int bcw_walset_create(bcw_ctx* c, bcw_walset** out) {
  if (!c || !out) return BCW_E_INVAL;
  *out = nullptr;
  bcw_walset* ws = new (std::nothrow) bcw_walset();
  if (!ws) return BCW_E_NOMEM;
  ws->ctx = c;
  *out = ws;
  return BCW_OK;
}

int bcw_walset_destroy(bcw_walset* ws) {
  if (!ws) return BCW_E_INVAL;
  DeviceGuard dg(ws->ctx->device);
  (void)hipStreamSynchronize(ws->ctx->cur);
  for (void* img : ws->t.owned) (void)hipFree(img);
  delete ws;
  return BCW_OK;
}

int bcw_walset_put(bcw_walset* ws, uint64_t fid, const uint8_t* d_seg, uint64_t seg_len, uint64_t base_time) {
  if (!ws || (seg_len && !d_seg)) return BCW_E_INVAL;
  DeviceGuard dg(ws->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  return ws_put(ws, WalEnt{fid, d_seg, seg_len, base_time}, nullptr);
}

int bcw_walset_upload(bcw_walset* ws, uint64_t fid, const uint8_t* h_seg, uint64_t seg_len, uint64_t base_time) {
  if (!ws || (seg_len && !h_seg)) return BCW_E_INVAL;
  DeviceGuard dg(ws->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  void* img = nullptr;
  if (hipMalloc(&img, std::max<uint64_t>(seg_len, 16)) != hipSuccess) return BCW_E_NOMEM;
  if (seg_len && (hipMemcpyAsync(img, h_seg, seg_len, hipMemcpyHostToDevice, ws->ctx->cur) != hipSuccess ||
                  hipStreamSynchronize(ws->ctx->cur) != hipSuccess)) {
    (void)hipFree(img);
    return BCW_E_HIP;
  }
  const int rc = ws_put(ws, WalEnt{fid, (const uint8_t*)img, seg_len, base_time}, img);
  if (rc == BCW_E_NOMEM && !ws->t.has(fid)) (void)hipFree(img);  // the table did not take it
  return rc;
}

int bcw_walset_remove(bcw_walset* ws, uint64_t fid) {
  if (!ws) return BCW_E_INVAL;
  DeviceGuard dg(ws->ctx->device);
  if (!dg.ok) return BCW_E_HIP;
  bool found = false;
  void* old = ws->t.remove(fid, &found);
  if (!found) return BCW_OK;
  const int rc = ws_publish(ws);
  ws_free_image(ws, old);
  return rc;
}

uint64_t bcw_walset_count(bcw_walset* ws) { return ws ? ws->t.ents.size() : 0; }

int bcw_get_records_async(bcw_index* ix, bcw_walset* ws, const bcw_get_params* p, uint64_t n, const uint8_t* d_keys,
                          const uint64_t* d_key_off, const bcw_get_out* d_out, bcw_get_result* d_result) {
  if (!ix || !ws || !p || !d_out || !d_result || index_ctx(ix) != ws->ctx) return BCW_E_INVAL;
  const bcw_get_out& o = *d_out;
  if (n && (!d_key_off || !o.get_status || !o.rd_status || !o.fid || !o.off || !o.size || !o.pay_off))
    return BCW_E_INVAL;
  if ((o.payload_cap && !o.payload) || !read_table_ok(o.table)) return BCW_E_INVAL;
  bcw_ctx* c = ws->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  const uint64_t nb = (n + kGetLookupKeys - 1) / kGetLookupKeys;
  if (nb > ws->blk_cap) {
    const uint64_t cap = std::max<uint64_t>(1024, std::max(nb, ws->blk_cap * 2));
    DevBuf<uint64_t> d;
    if (!d.alloc(2 * cap * sizeof(uint64_t))) return BCW_E_NOMEM;
    ws->d_blk.adopt(std::move(d), st);
    ws->blk_cap = cap;
  }
  uint64_t* bsum = ws->d_blk.get();
  uint64_t* bfound = bsum + ws->blk_cap;
  Prof* prof = &c->prof;
  hipEvent_t ev = nullptr;

  GetLookup g{};
  g.wals = ws->d_ents.get();
  g.n_wals = (uint32_t)ws->t.ents.size();
  g.n = n;
  g.keys = d_keys;
  g.koff = d_key_off;
  g.out = o;
  g.bsum = bsum;
  g.bfound = bfound;
  prof->begin(K_GET_LOOKUP, st, ev);
  if (ix_launch_get_lookup(ix, g, st) != hipSuccess) return BCW_E_HIP;
  prof->end(K_GET_LOOKUP, st, ev);

  prof->begin(K_GET_SCAN, st, ev);
  get::k_get_scan<<<1, get::kScanThreads, 0, st>>>(bsum, bfound, nb, o.payload_cap, d_result);
  if (nb) get::k_get_offsets<<<(uint32_t)nb, kGetLookupKeys, 0, st>>>(o.pay_off, n, bsum);
  prof->end(K_GET_SCAN, st, ev);
  if (hipGetLastError() != hipSuccess) return BCW_E_HIP;
  if (n == 0) return BCW_OK;

  get::ReadArgs A{};
  A.wals = ws->d_ents.get();
  A.n_wals = g.n_wals;
  A.p = *p;
  A.n = n;
  A.out = o;
  A.res = d_result;
  A.pow2 = c->tabs.pow2;
  A.initc = c->tabs.initc;
  const uint64_t want = (n + get::kWaves - 1) / get::kWaves;
  // a few rounds of resident workgroups (4 per CU at the kernel's registers): the dispatcher evens out requests of
  // unequal size, and the verify tables are filled a bounded number of times however large n is
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)c->num_cus * 32);
  prof->begin(K_GET_READ, st, ev);
  get::k_get_read<<<grid, 64 * get::kWaves, 0, st>>>(A);
  prof->end(K_GET_READ, st, ev);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_get_records(bcw_index* ix, bcw_walset* ws, const bcw_get_params* p, uint64_t n, const uint8_t* h_keys,
                    const uint64_t* h_key_off, const bcw_get_out* h_out, bcw_get_result* h_result) {
  if (!ix || !ws || !p || !h_out || !h_result || index_ctx(ix) != ws->ctx) return BCW_E_INVAL;
  const bcw_get_out& h = *h_out;
  if (n && (!h_key_off || !h.get_status || !h.rd_status || !h.fid || !h.off || !h.size || !h.pay_off))
    return BCW_E_INVAL;
  if ((h.payload_cap && !h.payload) || !read_table_ok(h.table)) return BCW_E_INVAL;
  *h_result = bcw_get_result{};
  h_result->fits = 1;
  if (n == 0) return BCW_OK;
  if (const int rc = flat_keys_ok(n, h_keys, h_key_off)) return rc;
  bcw_ctx* c = ws->ctx;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  const bool tab = h.table.status != nullptr;
  DevBuf<> mem;
  GetLayout L;
  const uint64_t kb = h_key_off[n] - h_key_off[0];
  if (const int rc = carve_alloc(mem, [&](Carver& cv) { L = carve_get(cv, kb, h.payload_cap, n, tab); })) return rc;
  const bcw_get_out& d = L.out;
  hipStream_t st = c->cur;
  std::vector<uint64_t> koff;  // alive until the synchronise below
  bool ok = upload_flat_keys(n, h_keys, h_key_off, L.k, st, &koff);
  int rc = ok ? bcw_get_records_async(ix, ws, p, n, L.k.keys, L.k.key_off, &d, L.res) : BCW_E_HIP;
  if (rc == BCW_OK) {
    ok = copy_down(h_result, L.res, sizeof(bcw_get_result), st) && copy_down(h.get_status, d.get_status, n, st) &&
         copy_down(h.rd_status, d.rd_status, n, st) && copy_down(h.fid, d.fid, 8 * n, st) &&
         copy_down(h.off, d.off, 8 * n, st) && copy_down(h.size, d.size, 8 * n, st) &&
         copy_down(h.pay_off, d.pay_off, 8 * n, st) && hipStreamSynchronize(st) == hipSuccess;
    rc = !ok ? BCW_E_HIP : h_result->fits ? BCW_OK : BCW_E_CAPACITY;
  }
  if (rc == BCW_OK) {
    ok = copy_down(h.payload, d.payload, h_result->payload_need, st);
    if (ok && tab) ok = table_copy_down(h.table, d.table, std::min(n, h.table.capacity), st);
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) rc = BCW_E_HIP;
  }
  (void)hipStreamSynchronize(st);  // before mem goes
  return rc;
}

}  // extern "C"
