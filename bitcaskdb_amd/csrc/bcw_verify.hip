// bcw_verify.hip -- scrub: every live, file-backed index entry against the resident WALs (bcw_index_verify*; bcw.h,
// bcw_verify.h). What DBImpl.Get (db_impl.go:567-587) of each key would run into, and whether the record found at
// (fid, off, size) carries that key, without a payload byte being copied and without the keys leaving HBM.
//
// A scrub is four stream-ordered launches, so every hand-off is a kernel boundary:
//   k_ix_vfy_select (bcw_index.hip) one pass over the slot table: soft-deleted entries counted, NO_WAL and READ /
//                   BEYOND decided, every other checked entry queued as a 48-byte work item
//   k_vfy_read      one wave per work item (waves stride over the queue): the body of k_get_read (bcw_read_body.h)
//                   with no copy -- the fragment walk with its optional CRC verify, RecordFromBytes on lane 0 -- then
//                   the wave compares the entry's key in the arena with the record's namespace and key ranges
//   k_usage_final   (bcw_usage.hip) the bad entries' rows per fid, ascending
//   k_vfy_final     one thread: the counters into the result, and `fits`
// Both kernels emit a bad entry through vfy::emit_bad and feed it to the workgroup's usage::Accum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bcw_host.h"
#include "bcw_read_body.h"
#include "bcw_usage.h"
#include "bcw_verify.h"

namespace bcw {
namespace vfy {

constexpr int kWaves = usage::kThreads / 64;  // the accumulator's workgroup size

struct ReadArgs {
  const WalEnt* wals;
  uint32_t n_wals;
  bcw_get_params p;
  const Item* queue;
  uint64_t queue_cap;
  Sink S;
  uint64_t* scratch;      // the context's accounting table
  const uint32_t* pow2;   // [kPow2Ops][8][16] nibble images of A_{8 * 2^k}
  const uint32_t* initc;  // A_{8L}(0xFFFFFFFF)
};

// Bounds: the image is read only through byte_at's bound (read_walk with kCopy = false has no wide path, FragReader
// reads through byte_at); the arena is read over the entry's own key length; the walk's loop is bounded by rs <=
// seg_len (k_ix_vfy_select queued only spans inside their image) and the compare by the arena key's length.
__global__ __launch_bounds__(64 * kWaves) void k_vfy_read(ReadArgs A) {
  __shared__ usage::Accum acc;
  __shared__ uint32_t t0[256];
  __shared__ uint32_t sp2[kPow2Ops * 128];
  __shared__ uint64_t s_fo[kWaves][rd::kMaxF];
  __shared__ uint32_t s_fl[kWaves][rd::kMaxF];
  __shared__ unsigned long long s_cnt[V_NUM];  // V_CLASS + c, V_RD + s of this workgroup
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t queued = A.S.cnt[V_QUEUE];  // written by the launch before this one
  const uint64_t n = queued < A.queue_cap ? queued : A.queue_cap;
  if ((uint64_t)blockIdx.x * kWaves >= n) return;  // the whole workgroup: the grid is sized from the slot capacity
  if (tid < V_NUM) s_cnt[tid] = 0;
  acc.init();
  if (A.p.verify) rd::load_verify_tables(t0, sp2, A.pow2, tid, 64 * kWaves);
  __syncthreads();
  const usage::Table g = usage::table_of(A.scratch);
  uint64_t n_ok = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < n; r += (uint64_t)gridDim.x * kWaves) {
    const Item it = A.queue[r];
    const WalEnt W = A.wals[it.wal < A.n_wals ? it.wal : 0];  // the select pass found the fid at this position
    const rd::ReadEnv E{W.seg, W.seg_len, A.p.verify, t0, sp2, A.initc, s_fo[wave], s_fl[wave]};
    uint32_t nf = 0;
    // size <= seg_len and off in [40, seg_len] (wal_span): WalRecordSize's loop is bounded by the image
    const uint32_t st = rd::read_walk<false, false>(E, it.off, it.size, rd::wal_record_size(it.off, it.size), nullptr,
                                                    lane, nf);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t rec = BCW_ST_OK, hdr = 0;
    uint64_t kl = 0;
    if (st == BCW_RD_OK) {
      if (lane == 0) {
        const rd::ReadRow R = rd::read_parse(E, W.base_time, A.p.ns_size, A.p.etag_size, it.size, nf);
        rec = R.status;
        hdr = R.hdr;
        kl = R.kl;
      }
      rec = __shfl(rec, 0, 64);
      hdr = __shfl(hdr, 0, 64);
      kl = __shfl(kl, 0, 64);
    }
    bool equal = false;
    if (st == BCW_RD_OK && rec == BCW_ST_OK) {
      // the record's merged key is payload[1, 1 + ns) || payload[hdr, hdr + kl): lanes stride the arena key's bytes
      const uint64_t ns = A.p.ns_size;
      bool diff = ns + kl != (uint64_t)it.key_len;
      if (!diff) {
        const rd::FragReader fr{E.seg, E.seg_len, E.fo, E.fl, nf < (uint32_t)rd::kMaxF ? nf : (uint32_t)rd::kMaxF};
        const uint8_t* __restrict__ key = A.S.arena + (it.kref - 1) + 16;
        for (uint32_t i = lane; i < it.key_len; i += 64)
          diff |= fr(i < ns ? 1 + (uint64_t)i : (uint64_t)hdr + (i - ns)) != (uint32_t)key[i];
      }
      equal = __ballot(diff) == 0;
    }
    if (lane != 0) continue;
    const uint32_t cls = classify(true, st, rec, equal);
    if (cls == BCW_VFY_OK) {
      ++n_ok;
      continue;
    }
    atomicAdd(&s_cnt[V_CLASS + cls], 1ull);
    if (cls == BCW_VFY_READ) atomicAdd(&s_cnt[V_RD + (st & 7u)], 1ull);
    emit_bad(A.S, it.fid, it.off, it.size, it.hash, it.kref, it.key_len, cls, cls == BCW_VFY_READ ? st : BCW_RD_OK,
             cls == BCW_VFY_RECORD ? rec : BCW_ST_OK);
    // off >= 40 here (wal_span): the entry counts, by k_ix_usage's rule
    acc.row(g, it.fid, 1, it.size, usage::wal_record_size_closed(it.off, it.size));
  }
  if (lane == 0 && n_ok) atomicAdd(&s_cnt[V_CLASS + BCW_VFY_OK], (unsigned long long)n_ok);
  acc.flush(g);  // begins with the barrier that completes s_cnt too
  if (tid >= V_CLASS && tid < V_NUM && s_cnt[tid]) atomicAdd(&A.S.cnt[tid], s_cnt[tid]);
}

// one thread, behind usage_finish (which wrote res->per_fid): the counters into the result, and `fits`
__global__ void k_vfy_final(const unsigned long long* __restrict__ cnt, bcw_verify_out out,
                            bcw_verify_result* __restrict__ res) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bcw_usage_result pf = res->per_fid;
  res->n_checked = cnt[V_CHECKED];
  res->n_soft_deleted = pf.soft_deleted;
  for (int c = 0; c < 5; ++c) res->by_class[c] = cnt[V_CLASS + c];
  for (int s = 0; s < 8; ++s) res->by_rd[s] = cnt[V_RD + s];
  res->n_bad = cnt[V_NBAD];
  res->bad_key_bytes = cnt[V_KEY_BYTES];
  const bool ok = fits(cnt[V_NBAD], out.bad_cap, cnt[V_KEY_BYTES], out.keys_cap, pf.n_fids, out.rows_cap,
                       pf.overflow != 0 || pf.fits == 0);
  res->fits = ok ? 1u : 0u;
  res->_pad = 0;
}

}  // namespace vfy
}  // namespace bcw

using namespace bcw;

extern "C" {

int bcw_index_verify_async(bcw_index* ix, bcw_walset* ws, const bcw_get_params* p, const bcw_verify_out* d_out,
                           bcw_verify_result* d_res) {
  if (!ix || !ws || !p || !d_out || !d_res || index_ctx(ix) != walset_ctx(ws)) return BCW_E_INVAL;
  const bcw_verify_out& o = *d_out;
  if ((o.bad_cap && !o.bad) || (o.keys_cap && !o.keys) || (o.rows_cap && !o.rows)) return BCW_E_INVAL;
  bcw_ctx* c = index_ctx(ix);
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  uint64_t* scratch = nullptr;
  int rc = usage_begin(c, st, &scratch);
  if (rc != BCW_OK) return rc;

  VerifySelect v{};
  v.wals = walset_device(ws, &v.n_wals);
  v.out = o;
  v.scratch = scratch;
  rc = ix_launch_verify_select(ix, v, st);
  if (rc != BCW_OK) return rc;

  vfy::ReadArgs A{};
  A.wals = v.wals;
  A.n_wals = v.n_wals;
  A.p = *p;
  A.queue = static_cast<const vfy::Item*>(v.queue);
  A.queue_cap = v.queue_cap;
  A.S = vfy::Sink{o, v.cnt, v.arena};
  A.scratch = scratch;
  A.pow2 = c->tabs.pow2;
  A.initc = c->tabs.initc;
  if (v.n_wals && v.queue_cap) {  // an empty set queues nothing: every checked entry is NO_WAL
    // the queue's length is on the device: the grid is k_get_read's for as many requests as the table has slots, and
    // a workgroup whose first item lies past the queue's end returns before it fills a table
    const uint64_t want = (v.queue_cap + vfy::kWaves - 1) / vfy::kWaves;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)c->num_cus * 32);
    hipEvent_t ev = nullptr;
    c->prof.begin(K_VFY_READ, st, ev);
    vfy::k_vfy_read<<<grid, 64 * vfy::kWaves, 0, st>>>(A);
    c->prof.end(K_VFY_READ, st, ev);
    if (hipGetLastError() != hipSuccess) return BCW_E_HIP;
  }
  rc = usage_finish(c, st, o.rows, o.rows_cap, &d_res->per_fid, 1);
  if (rc != BCW_OK) return rc;
  vfy::k_vfy_final<<<1, 1, 0, st>>>(v.cnt, o, d_res);
  return hipGetLastError() == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_index_verify(bcw_index* ix, bcw_walset* ws, const bcw_get_params* p, const bcw_verify_out* h_out,
                     bcw_verify_result* h_res) {
  if (!ix || !ws || !p || !h_out || !h_res || index_ctx(ix) != walset_ctx(ws)) return BCW_E_INVAL;
  const bcw_verify_out& h = *h_out;
  if ((h.bad_cap && !h.bad) || (h.keys_cap && !h.keys) || (h.rows_cap && !h.rows)) return BCW_E_INVAL;
  bcw_ctx* c = index_ctx(ix);
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  hipStream_t st = c->cur;
  DevBuf<> mem;
  bcw_verify_out d{};
  bcw_verify_result* d_res = nullptr;
  if (const int rc = carve_alloc(mem, [&](Carver& cv) {
        d_res = cv.take<bcw_verify_result>(1, 16);
        d.bad = cv.take<bcw_verify_bad>(h.bad_cap, 16);
        d.rows = cv.take<bcw_fid_usage>(h.rows_cap, 16);
        d.keys = cv.take<uint8_t>(h.keys_cap, 16);
      }))
    return rc;
  d.bad_cap = h.bad_cap;
  d.keys_cap = h.keys_cap;
  d.rows_cap = h.rows_cap;
  if (!h.bad_cap) d.bad = nullptr;
  if (!h.keys_cap) d.keys = nullptr;
  if (!h.rows_cap) d.rows = nullptr;
  int rc = bcw_index_verify_async(ix, ws, p, &d, d_res);
  if (rc == BCW_OK)
    rc = copy_down(h_res, d_res, sizeof *h_res, st) && hipStreamSynchronize(st) == hipSuccess ? BCW_OK : BCW_E_HIP;
  if (rc == BCW_OK && !h_res->fits) rc = BCW_E_CAPACITY;
  if (rc == BCW_OK) {
    const bool ok = copy_down(h.bad, d.bad, h_res->n_bad * sizeof(bcw_verify_bad), st) &&
                    copy_down(h.keys, d.keys, h_res->bad_key_bytes, st) &&
                    copy_down(h.rows, d.rows, h_res->per_fid.n_fids * sizeof(bcw_fid_usage), st) &&
                    hipStreamSynchronize(st) == hipSuccess;
    if (!ok) rc = BCW_E_HIP;
  }
  (void)hipStreamSynchronize(st);  // before mem goes
  return rc;
}

}  // extern "C"
