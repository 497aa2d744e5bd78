// Host-side plumbing of libbcw.so that the decode kernels never read: the context behind the C-ABI handle, the encode
// and put scratch, and the steps the translation units share (encode, index, get, put, the sync API).
#pragma once
#include "bcw_internal.h"
#include "bcw_walset.h"

namespace bcw {

// Encode scratch (grow-only, per context). rows: source table rows.
struct EncScratch {
  uint64_t rows_cap = 0;
  DevBuf<uint32_t> sz;        // [rows] payload size per source row (0: not written)
  DevBuf<uint8_t> mflag;      // [rows] meta dropped by Record.Encode
  DevBuf<uint32_t> dsrc;      // [rows] dense record -> source row
  DevBuf<uint64_t> da;        // [rows+1] dst WAL y-coordinates
  DevBuf<uint64_t> hda;       // [rows+1] hint WAL y-coordinates
  DevBuf<uint32_t> hsz;       // [rows] hint payload sizes (compaction)
  DevBuf<uint64_t> dpos;      // [rows] dst record offsets
  DevBuf<uint64_t> hpos;      // [rows] hint record offsets (compaction)
  DevBuf<> tiles;             // scan tile sums
  DevBuf<> ev;                // [rows+2] layout events
  DevBuf<uint32_t> evb;       // [rows/win+2] governing event per event-scan window
  DevBuf<uint64_t> evt;       // [rows/win+2][32768] per-window entry tables (k_ev_win)
  DevBuf<uint16_t> hnl;       // [rows] next event inside the window (k_ev_win)
  DevBuf<uint32_t> evw;       // [rows/win+2][3] window entries (k_ev_walk)
  DevBuf<> recdesc;           // [rows] 128 B payload descriptors (k_recdesc_w -> k_write), dst WAL
  DevBuf<uint32_t> wl;        // [rows] dst records k_wcopy leaves to k_write<16> / k_write_general
  DevBuf<uint64_t> emisc;     // [64] counters
  int wcopy_resident = 0;     // k_wcopy workgroups resident per CU (occupancy query on the context's device, once)
};
// the payload descriptors are built on an auxiliary stream while the serial layout scans run (context lifetime)
struct EncAux {
  hipStream_t aux = nullptr;
  hipEvent_t ev_scan = nullptr, ev_hscan = nullptr, ev_desc = nullptr;
};

struct EncLaunch {
  const uint8_t* d_src;
  bcw_encode_params p;
  bcw_record_table table;
  uint64_t rows;
  const bcw_decode_result* d_src_result;
  const uint8_t* d_keep;
  bcw_encode_out out;
  bcw_encode_result* d_result;
  const Frag* frags;
  const uint32_t* crc_ops;
  const uint32_t* initc;
  int num_cus;
  uint64_t gen;  // generation of the context's latest decode (the owner of `frags`)
};

hipError_t launch_encode(const EncLaunch& L, EncScratch& s, EncAux& a, hipStream_t stream, Prof* prof);
// The writer's layout for a caller that filled s.sz itself (bcw_put.hip): enc_layout_reset clears the counters
// (before the caller's own prep kernel, which sets emisc[kXNin] and min-reduces emisc[kXErr] as k_enc_prep does);
// enc_layout_run is launch_encode's dst WAL layout -- the scan of s.sz over rows [0, first error), the event scan from
// wal_pos and k_recoff -- and leaves s.da (y-coordinates), s.dpos (the offsets WriteRecord returns) and the layout's
// counters emisc[kXLay + ...] (kXLayEnd: the file size after the append).
constexpr int kXNin = 0, kXErr = 1, kXNDense = 3, kXLay = 8, kXLayEnd = kXLay + 3, kXPut = 32;
void enc_layout_reset(EncScratch& s, hipStream_t stream);
hipError_t enc_layout_run(EncScratch& s, uint64_t rows, uint64_t wal_pos, hipStream_t stream);
// grow the context's encode scratch to `rows` records (bcw_api.cpp)
int enc_scratch_reserve(bcw_ctx* c, uint64_t rows);
size_t enc_sizeof_ev();
size_t enc_sizeof_recdesc();
size_t enc_sizeof_tile();
int enc_tile_items();
int enc_ev_win();

// Every C-ABI entry point that touches the device selects the context's device on the calling thread
// and restores the caller's current device when it returns.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The flat keys of a host call, key i = h_keys[h_key_off[i], h_key_off[i + 1]), n > 0 (bcw_index_apply_stat,
// bcw_index_get, bcw_get_records). flat_keys_ok refuses offsets that run backwards and a NULL h_keys with key bytes.
// upload_flat_keys queues the two copies into d (carve_flat_keys): the key bytes from the first key on, and the
// offsets rebased to it, which *koff holds until the caller has synchronised `st`.
inline int flat_keys_ok(uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off) {
  if (h_key_off[n] != h_key_off[0] && !h_keys) return BCW_E_INVAL;
  for (uint64_t i = 0; i < n; ++i)
    if (h_key_off[i + 1] < h_key_off[i]) return BCW_E_INVAL;
  return BCW_OK;
}
inline bool upload_flat_keys(uint64_t n, const uint8_t* h_keys, const uint64_t* h_key_off, const FlatKeys& d,
                             hipStream_t st, std::vector<uint64_t>* koff) {
  const uint64_t kb = h_key_off[n] - h_key_off[0];
  koff->resize(n + 1);
  for (uint64_t i = 0; i <= n; ++i) (*koff)[i] = h_key_off[i] - h_key_off[0];
  return copy_up(d.keys, kb ? h_keys + h_key_off[0] : nullptr, kb, st) &&
         copy_up(d.key_off, koff->data(), 8 * (n + 1), st);
}

// The context an index was created on (bcw_index.hip): the sync entry points refuse an index of another context.
bcw_ctx* index_ctx(const bcw_index* ix);
// doFilter (bcw_compact_filter_async) of context c's latest decode against index x, on c's stream, with the call's
// counters in d_cnt (kIxCounters words of c's device): another context on the index's device filters against the
// index itself, read-only, while no call modifies it (bcw_compact_wals).
constexpr int kIxCounters = 16;
constexpr int kIxRuleCnt = 13;  // d_cnt[kIxRuleCnt, +3): the rows the index's compaction filter rules dropped in the call
int ix_filter_on(bcw_index* x, bcw_ctx* c, const uint8_t* d_seg, const bcw_decode_params* p,
                 const bcw_record_table* d_table, const bcw_decode_result* d_result, uint64_t src_fid, uint8_t* d_keep,
                 uint64_t* d_cnt, bcw_index_result* d_out);
// The compaction filter rules' counters across the synchronous compactions. bcw_compact_filter_async counts into the
// index's cumulative counters; a compaction that may be refused for capacity and run again counts a source only when
// its output is final. bcw_compact_segment: ix_filter_pending (bcw_compact_filter_async with the counts held apart),
// then ix_rule_commit once the encode's outputs are out. bcw_compact_wals: ix_filter_on leaves the call's counts in
// d_cnt[kIxRuleCnt, +3); a staging index gets the main index's rules (ix_forward_rules) and counts for itself; the
// caller adds the counts of the final sources on the host (ix_add_rule_counts). Without rules (ix_has_rules) none of
// this runs: no launch, copy or synchronisation is added to a compaction.
int ix_filter_pending(bcw_index* x, const uint8_t* d_seg, const bcw_decode_params* p, const bcw_record_table* d_table,
                      const bcw_decode_result* d_result, uint64_t src_fid, uint8_t* d_keep, bcw_index_result* d_out);
int ix_rule_commit(bcw_index* x);
bool ix_has_rules(const bcw_index* x);
int ix_forward_rules(bcw_index* to, const bcw_index* from);
void ix_add_rule_counts(bcw_index* to, const uint64_t c[3]);

// The lookup step of a batched Get (bcw_get.hip drives it; the kernel lives with the index, bcw_index.hip): one lane
// per key. Writes get_status / rd_status / fid / off / size, the request's slot size into out.pay_off (the scan
// turns the column into offsets), and per workgroup of kGetLookupKeys keys the sum of its slots (bsum) and its found
// keys (bfound). The index's buffers are taken when the call is made, on the index's context.
constexpr int kGetLookupKeys = 256;
struct GetLookup {
  const WalEnt* wals;  // device, ascending fid
  uint32_t n_wals;
  uint64_t n;
  const uint8_t* keys;
  const uint64_t* koff;
  bcw_get_out out;
  uint64_t* bsum;
  uint64_t* bfound;
};
hipError_t ix_launch_get_lookup(bcw_index* x, const GetLookup& g, hipStream_t st);

// The resident set as the kernels take it (bcw_get.hip): its context, and its device array (ascending fid) with
// the number of entries, as of this call.
bcw_ctx* walset_ctx(const bcw_walset* ws);
const WalEnt* walset_device(const bcw_walset* ws, uint32_t* n_wals);

// The select step of a scrub (bcw_verify.hip drives it; the kernel lives with the index, bcw_index.hip): one pass over
// the slot table decides NO_WAL and READ / BEYOND, counts, and queues every other checked entry as a 48-byte work item
// (vfy::Item, bcw_verify.h) for k_vfy_read. The launch grows the index's queue to its slot capacity, zeroes the call's
// counters (cnt: vfy::V_NUM device words in front of the queue) and fills the last four fields: the index's buffers
// are taken when the call is made, on the index's context.
struct VerifySelect {
  const WalEnt* wals;  // device, ascending fid
  uint32_t n_wals;
  bcw_verify_out out;  // the caller's arrays (device)
  uint64_t* scratch;   // the context's accounting table (usage_begin)
  // filled by the launch
  unsigned long long* cnt;
  void* queue;
  uint64_t queue_cap;  // items; also the most the pass can queue
  const uint8_t* arena;
};
int ix_launch_verify_select(bcw_index* x, VerifySelect& v, hipStream_t st);

// The index half of a batched Write (bcw_put.hip drives it; the kernels live with the index, bcw_index.hip): the ops
// of a write batch through the index's batch launches. Keys are the batch's merged keys; the number of ops is read
// from the device word *n_in (n, or 0 when the batch was rejected), off / size from the device rec_off / rec_size, the
// op from the BCW_WR_* flags. found / free_fid / free_bytes (all or none): the WriteStat of every op, an earlier op of
// the batch on the same key included. idx_err (device, may be NULL) receives 0 or BCW_IDX_ERR_FULL.
struct PutIx {
  uint64_t n;
  const uint8_t* keys;
  const uint64_t* koff;
  uint64_t keys_len;
  const uint64_t* n_in;
  const uint64_t* rec_off;
  const uint64_t* rec_size;
  const uint8_t* flags;
  uint64_t fid;
  uint8_t* found;
  uint64_t* free_fid;
  uint64_t* free_bytes;
  int32_t* idx_err;
};
int ix_put_batch(bcw_index* x, const PutIx& p);

// Scratch of the batched Write (grow-only, per context; bcw_put.hip)
struct PutScratch {
  uint64_t rows_cap = 0, lit_cap = 0, frag_cap = 0;
  DevBuf<uint8_t> lit;       // [rows x stride] header literal per record (k_put_prep -> k_put_write)
  DevBuf<uint32_t> hlen;     // [rows] its length
  DevBuf<> frags;            // [frag_cap] output fragments (k_put_frags -> k_put_write)
  int write_resident = 0;    // k_put_write workgroups resident per CU (occupancy query on the context's device, once)
};

// The sync API's steps (bcw_api.cpp), shared with the multi-context fan-out (bcw_fanout.cpp): upload + decode into
// the context's device table; the keep mask's scratch; the decode parameters of a source WAL file; the encode of
// the context's decoded source with its keep mask, outputs copied to the host.
int sync_decode(bcw_ctx* c, const uint8_t* h_src, const bcw_decode_params& dp, bcw_decode_result& dres);
int ensure_keep(bcw_ctx* c, uint64_t rows);
bcw_decode_params src_params(const uint8_t* h_src, const bcw_encode_params* p);
int encode_to_host(bcw_ctx* c, const bcw_encode_params* p, const bcw_encode_out* h, bcw_encode_result* h_result,
                   const bcw_decode_result& dres);
// encode_to_host in two steps (bcw_compact_wals): the encode and its result (the dst / hint ends the next source
// starts from), then the copies of the outputs to the host. *d_out: the device-side outputs between the two.
int encode_run(bcw_ctx* c, const bcw_encode_params* p, const bcw_encode_out* h, bcw_encode_result* h_result,
               bcw_encode_out* d_out);
int encode_copy_out(bcw_ctx* c, const bcw_encode_params* p, const bcw_encode_out* h, const bcw_encode_result& r,
                    const bcw_encode_out& d, const bcw_decode_result& dres);

// Export of an index's live entries (bcw_index.hip) into host arrays the sink provides once the sizes are known:
// room(n, key_bytes) fills the five pointers (koff has n + 1 entries) or refuses (BCW_E_CAPACITY). h_fids / n_fids
// (n_fids > 0): only entries whose value fid is one of them.
struct IxSink {
  virtual ~IxSink() = default;
  virtual int room(uint64_t n, uint64_t key_bytes) = 0;
  uint8_t* keys = nullptr;
  uint64_t* koff = nullptr;
  uint64_t* fid = nullptr;
  uint64_t* off = nullptr;
  uint64_t* size = nullptr;
};
int ix_export(bcw_index* x, const uint64_t* h_fids, uint64_t n_fids, IxSink& sink, uint64_t* n_out,
              uint64_t* key_bytes);

}  // namespace bcw

// The context behind the C-ABI handle (bcw.h): one device, one launch stream, constant tables and
// grow-only scratch. Defined here so every translation unit of libbcw.so can reach its stream,
// device and the fragment table of its latest decode.
struct bcw_ctx {
  int device = 0;
  uint64_t id = 0;         // unique per context (high half of every decode generation)
  uint64_t gen_seq = 0;    // decodes issued on this context
  uint64_t frag_gen = 0;   // generation of the decode whose fragment table the scratch holds
  int num_cus = 256;
  hipStream_t own = nullptr;
  hipStream_t cur = nullptr;
  bcw::DevBuf<uint32_t> d_initc, d_image2, d_enc_ops, d_pow2;  // the constant tables (bcw_crc_tables.h) ...
  bcw::Tables tabs{};                                          // ... as the kernels take them
  bcw::Scratch s{};
  bcw::EncScratch es{};
  bcw::EncAux ea;
  bcw::PutScratch ps{};
  // sync encode staging (grow-only)
  bcw::DevBuf<uint8_t> d_keep;
  bcw::DevBuf<> d_eout;
  bcw::DevBuf<bcw_encode_result> d_eres;
  uint64_t frag_hint = 0;  // capacity requested by a retry
  // sync-API staging (grow-only)
  bcw::DevBuf<uint8_t> d_seg;
  bcw::DevBuf<> d_tab_mem;
  bcw_record_table d_tab{};  // carved from d_tab_mem (capacity 0: none)
  bcw::DevBuf<bcw_decode_result> d_result;
  bcw::DevBuf<bcw_index_result> d_ires;  // sync index calls
  bcw::DevBuf<uint64_t> usage;           // the space accounting's global table (bcw_usage.h), allocated on first use
  uint32_t last_start_off = 0;
  uint32_t chase_direct = BCW_CHASE_DIRECT_MAX;  // BCW_OPT_CHASE_DIRECT
  uint64_t test_abort_wg = 0;                    // BCW_OPT_TEST_ABORT_WAIT (one-shot)
  bool filter_snapshot = false;                  // BCW_OPT_FILTER_SNAPSHOT (bcw_compact_wals)
  bcw::Prof prof;
};
