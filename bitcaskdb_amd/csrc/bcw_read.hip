// bcw_read.hip -- batched point reads: Get / GetV2's record fetch (db_impl.go:567-631)
// = Wal.ReadRecord (wal.go:556-573: WalRecordSize, one read of the record's physical span) +
// WalParseRecord (wal.go:121-173: the fragment walk over that one buffer, optional CRC verify, size
// check) + RecordFromBytes (record.go:140-239), for many (offset, size) requests at once against a WAL
// image resident in HBM.
//
// One wave per request. The fragment headers of a record are walked in order (a record has
// ceil(size / 32761) + 1 of them at most); each fragment's data is copied to the request's payload slot
// by all lanes (16 B units aligned to the destination) and, with verifyChecksum, its CRC-32C is the
// XOR of the lanes' chunk CRCs shifted to the fragment end (shift operators A_{8*2^k}, nibble tables
// in LDS). The record header is then parsed by one lane straight from the segment, through the
// recorded fragment list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bcw_host.h"
#include "bcw_read_body.h"

namespace bcw {
namespace rd {

constexpr int kWaves = 4;

struct ReadArgs {
  const uint8_t* seg;
  bcw_read_params p;
  uint64_t n;
  const uint64_t* off;
  const uint64_t* size;
  const uint64_t* pay_off;
  uint8_t* payload;
  uint8_t* rd_status;
  bcw_record_table tab;
  const uint32_t* pow2;   // [kPow2Ops][8][16] nibble images of A_{8 * 2^k}
  const uint32_t* initc;  // A_{8L}(0xFFFFFFFF)
};

__global__ __launch_bounds__(64 * kWaves) void k_read_records(ReadArgs A) {
  __shared__ uint32_t t0[256];
  __shared__ uint32_t sp2[kPow2Ops * 128];  // a fragment is < 2^16 bytes: shifts by up to 65535
  __shared__ uint64_t s_fo[kWaves][kMaxF];
  __shared__ uint32_t s_fl[kWaves][kMaxF];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  load_verify_tables(t0, sp2, A.pow2, tid, 64 * kWaves);
  __syncthreads();
  const uint64_t r = (uint64_t)blockIdx.x * kWaves + wave;
  if (r >= A.n) return;
  const ReadEnv E{A.seg, A.p.seg_len, A.p.verify, t0, sp2, A.initc, s_fo[wave], s_fl[wave]};
  const uint64_t n = A.p.seg_len;
  const uint64_t off = A.off[r], size = A.size[r];
  uint32_t st = BCW_RD_OK;
  const uint64_t rs = wal_record_size(off, size);
  uint32_t nf = 0;
  if (off + rs > n || off + rs < off)
    st = BCW_RD_BEYOND;  // "read beyond file size" (wal.go:562-564)
  else
    st = read_walk<false>(E, off, size, rs, A.payload + A.pay_off[r], lane, nf);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane != 0) return;
  A.rd_status[r] = (uint8_t)st;
  if (!A.tab.status) return;
  ReadRow R;
  if (st == BCW_RD_OK) R = read_parse(E, A.p.base_time, A.p.ns_size, A.p.etag_size, size, nf);
  write_row(A.tab, r, off, size, nf, R);
}

}  // namespace rd

hipError_t launch_read_records(const rd::ReadArgs& A, hipStream_t st) {
  if (A.n == 0) return hipSuccess;
  rd::k_read_records<<<(uint32_t)((A.n + rd::kWaves - 1) / rd::kWaves), 64 * rd::kWaves, 0, st>>>(A);
  return hipGetLastError();
}

}  // namespace bcw

using namespace bcw;

extern "C" {

int bcw_read_records_async(bcw_ctx* c, const uint8_t* d_seg, const bcw_read_params* p, uint64_t n,
                           const uint64_t* d_off, const uint64_t* d_size, const uint64_t* d_pay_off, uint8_t* d_payload,
                           uint8_t* d_rd_status, const bcw_record_table* d_table) {
  if (!c || !p || (n && (!d_seg || !d_off || !d_size || !d_pay_off || !d_payload || !d_rd_status))) return BCW_E_INVAL;
  if (d_table && !read_table_ok(*d_table)) return BCW_E_INVAL;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  rd::ReadArgs A{};
  A.seg = d_seg;
  A.p = *p;
  A.n = n;
  A.off = d_off;
  A.size = d_size;
  A.pay_off = d_pay_off;
  A.payload = d_payload;
  A.rd_status = d_rd_status;
  if (d_table) A.tab = *d_table;
  A.pow2 = c->tabs.pow2;
  A.initc = c->tabs.initc;
  return launch_read_records(A, c->cur) == hipSuccess ? BCW_OK : BCW_E_HIP;
}

int bcw_read_records(bcw_ctx* c, const uint8_t* h_seg, const bcw_read_params* p, uint64_t n, const uint64_t* h_off,
                     const uint64_t* h_size, uint8_t* h_payload, uint8_t* h_rd_status, const bcw_record_table* h_table) {
  if (!c || !p || (n && (!h_off || !h_size || !h_payload || !h_rd_status)) || (p->seg_len && !h_seg))
    return BCW_E_INVAL;
  if (n == 0) return BCW_OK;
  DeviceGuard dg(c->device);
  if (!dg.ok) return BCW_E_HIP;
  std::vector<uint64_t> pay(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) pay[i + 1] = pay[i] + h_size[i];
  const bool tab = h_table && h_table->status;
  DevBuf<> mem;
  ReadLayout d;
  if (const int rc = carve_alloc(mem, [&](Carver& cv) { d = carve_read(cv, p->seg_len, pay[n], n, tab); })) return rc;
  hipStream_t st = c->cur;
  bool ok = (p->seg_len == 0 || hipMemcpyAsync(d.seg, h_seg, p->seg_len, hipMemcpyHostToDevice, st) == hipSuccess) &&
            hipMemcpyAsync(d.off, h_off, 8 * n, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.size, h_size, 8 * n, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.pay_off, pay.data(), 8 * (n + 1), hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && bcw_read_records_async(c, d.seg, p, n, d.off, d.size, d.pay_off, d.payload, d.rd_status,
                                    tab ? &d.tab : nullptr) == BCW_OK;
  ok = ok && (pay[n] == 0 || hipMemcpyAsync(h_payload, d.payload, pay[n], hipMemcpyDeviceToHost, st) == hipSuccess) &&
       hipMemcpyAsync(h_rd_status, d.rd_status, n, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (ok && tab) ok = table_copy_down(*h_table, d.tab, std::min(n, h_table->capacity), st);
  ok = ok && hipStreamSynchronize(st) == hipSuccess;  // any failure of the async half is reported as BCW_E_HIP
  return ok ? BCW_OK : BCW_E_HIP;
}

}  // extern "C"
