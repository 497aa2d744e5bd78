// Internal definitions of the decode pipeline, shared by its kernels (bcw_decode.hip) and the host API: nothing the
// decode does not read lives here (the rest of the host plumbing is bcw_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "bcw.h"
#include "bcw_crc_consts.h"
#include "bcw_devmem.h"

namespace bcw {

constexpr uint32_t kBlock = BCW_BLOCK_SIZE;  // wal.go:46
constexpr uint32_t kHdr = BCW_HEADER_SIZE;   // wal.go:53
constexpr uint32_t kWin = 128;               // CRC window per lane (bytes)
constexpr int kWaveLanes = 64;

// k_crc's stream balanced per XCD (bcw_decode.hip): workgroup r streams range r of the segment, and the dispatcher
// places workgroup r on XCD (r + s) % 8 with the same s every decode (both kernels' grids are multiples of 8), so each
// class r % 8 is one XCD. The ranges of class y are sized in proportion to its weight, the rate measured by the
// previous decode on the context (the XCDs of an MI355X stream up to ~6 % apart, kbench per-XCD timelines). Only the
// work split depends on it, never a result.
struct XBal {
  uint32_t w[8];    // byte weight of a range of class y (65536: equal)
  uint32_t pad0[8];
  uint64_t t[8];    // k_crc: summed stream times (wall_clock64 ticks) of class y's waves (the finalize resets them)
  uint64_t n[8];    // their count
  uint32_t on;      // k_chase used the weights (BCW_OPT_XCD_BALANCE): the finalize updates them only then
  uint32_t pad[7];
};
// One parsed fragment header (wal_iterator.go:62-77), 16 bytes.
struct Frag {
  uint32_t blk;    // block index within the segment
  uint16_t start;  // block-relative offset of the data (header + 7)
  uint16_t len;    // data length after the clamp of wal_iterator.go:75
  uint32_t chk;    // check word J = ~unmask(stored CRC) ^ A_{8 len}(0xFFFFFFFF) (bcw_decode.hip, k_crc): the
                   // fragment's data passes ComputeCRC32 iff its raw CRC-32C equals this (stored CRC recoverable)
  uint8_t type;    // header byte 6
  uint8_t ok;      // CRC verified
  uint16_t pad;
};
static_assert(sizeof(Frag) == 16, "Frag layout");

// Device-side constant tables, built on the host once per context.
struct Tables {
  uint32_t* initc;   // [kBlock+1] A_{8L}(0xFFFFFFFF)
  uint32_t* lds_image2; // the stream verify's LDS image (kS2Image)
  uint32_t* enc_ops;    // [kEncOpsWords] encode shift operators (nibble images, see build_enc_ops)
  uint32_t* pow2;       // [kPow2Ops][8][16] A_{8 * 2^k} (nibble images), k < 16: shifts by any distance < 64 KiB
};
#ifndef BCW_CRC_WAVES
#define BCW_CRC_WAVES 16
#endif
constexpr int kCrcWaves = BCW_CRC_WAVES;  // waves per k_crc workgroup (one workgroup per CU)
constexpr int kCrcThreads = kCrcWaves * 64;

struct Scratch {
  uint64_t nblocks_cap = 0;
  uint64_t frag_cap = 0;
  DevBuf<uint32_t> fbase;      // [nblocks+1] global index of each block's first fragment
  DevBuf<uint32_t> rbase;      // [nblocks+1] Full/Last fragments before each block (its first record row)
  DevBuf<uint2> bsum;          // [nblocks] record-state summary of each block (bcw_decode.hip, kSumHasE)
  DevBuf<uint64_t> lb;         // [nblocks/64+2] k_chase look-back words (zeroed at allocation)
  DevBuf<uint64_t> lbe;        // [nblocks/64+2] k_chase look-back words of the Full/Last counts (> kDirect groups)
  uint64_t nlb = 0;
  uint64_t epoch = 1;          // look-back epoch of the next launch
  DevBuf<Frag> frags;          // [frag_cap]
  DevBuf<uint4> srec;          // [frag_cap + 4] stream record per fragment (k_chase -> k_crc, bcw_decode.hip kRecUsual)
  DevBuf<uint8_t> fok;         // [frag_cap] CRC verdict per fragment (k_crc; dense: 64 verdicts are one 64 B store)
  DevBuf<uint32_t> wstart;     // [CUs x kCrcWaves + 1] each k_crc wave's first fragment (byte-balanced, k_chase)
  DevBuf<XBal> xbal;           // the per-XCD split of k_crc's stream (persists across decodes)
  uint32_t xbal_on = 1;        // BCW_OPT_XCD_BALANCE
  DevBuf<uint64_t> misc;       // [16] device counters (see bcw_decode.hip)
  uint32_t chase_direct = BCW_CHASE_DIRECT_MAX;  // k_chase: direct predecessor sum up to this many workgroups
  uint64_t test_abort_wg = 0;  // BCW_OPT_TEST_ABORT_WAIT for the next launch only (k_chase workgroup + 1; 0: none)
};

// Optional per-kernel HIP-event timing (bcw_ctx_set_profiling): events recorded on the launch
// stream around every kernel of the pipeline.
enum KernelId { K_CHASE = 0, K_CRC, K_RETIRED, K_ENC_PREP, K_ENC_SCAN, K_ENC_EVENTS, K_ENC_WRITE, K_ENC_HINT_LAYOUT,
                K_ENC_EVENTS_HINT, K_GET_LOOKUP, K_GET_SCAN, K_GET_READ, K_PUT_PREP, K_PUT_LAYOUT, K_PUT_FRAGS,
                K_PUT_WRITE, K_PUT_INDEX, K_USAGE_INDEX, K_USAGE_ROWS, K_USAGE_FINAL, K_IX_LIVE_BYTES, K_IX_DROP,
                K_VFY_SELECT, K_VFY_READ, K_SCAN_SELECT, K_SCAN_OFFSETS, K_SCAN_EMIT, K_NUM };
struct Prof {
  uint32_t mask = 0;   // bit k: time kernel id k
  uint32_t every = 1;  // time every `every`-th launch of a selected kernel
  uint32_t seq[K_NUM] = {};
  bool open[K_NUM] = {};
  struct Mark { int kid; hipEvent_t a, b; };
  std::vector<Mark> marks;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  bool on(int kid) const { return (mask >> kid) & 1u; }
  void begin(int kid, hipStream_t s, hipEvent_t& a) {
    open[kid] = on(kid) && (seq[kid]++ % every) == 0;
    if (open[kid]) { a = get(); (void)hipEventRecord(a, s); }
  }
  void end(int kid, hipStream_t s, hipEvent_t a) {
    if (!open[kid]) return;
    open[kid] = false;
    hipEvent_t b = get();
    (void)hipEventRecord(b, s);
    marks.push_back({kid, a, b});
  }
};

// Launch the full decode pipeline on `stream`. Defined in bcw_decode.hip.
hipError_t launch_decode(const uint8_t* d_seg, const bcw_decode_params& p, const bcw_record_table& t,
                         bcw_decode_result* d_result, const Tables& tabs, Scratch& s, uint64_t nblocks,
                         uint64_t gen, hipStream_t stream, int num_cus, Prof* prof);
hipError_t launch_export_frags(const Scratch& s, const bcw_frag_table& out, uint32_t start_off, hipStream_t stream,
                               uint64_t n, const uint32_t* initc);

}  // namespace bcw
