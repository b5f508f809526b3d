// mmf_host.h — host-side plumbing of libmmf_hg.so: error reporting, per-(device,stream)
// grow-only workspaces, launch checks, and the internal kernel-launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <optional>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/mmf_hg.h"
#include "../../include/mmf_hg_topk.h"
#include "../../include/mmf_hg_topk16.h"
#include "../../include/ext/mmf_hg_topk16_seg.h"
#include "../../include/ext/mmf_hg_topk_xy.h"
#include "../../include/ext/mmf_hg_seg_exact.h"
#include "../../include/ext/mmf_hg_topk_anyk.h"
#include "../../include/ext/mmf_hg_kmeans_ragged.h"
#include "../../include/ext/mmf_hg_cross_seg.h"
#include "../../include/ext/mmf_hg_cross_seg16.h"
#include "../../include/ext/mmf_hg_cross_segw.h"
#include "../../include/ext/mmf_hg_fast_anyk.h"
#include "../../include/ext/mmf_hg_wide_anyk.h"
#include "../../include/ext/mmf_hg_seg_anyk.h"
#include "../../include/ext/mmf_hg_cross_seg_anyk.h"
#include "../../include/ext/mmf_hg_cross_segw_anyk.h"
#include "../../include/ext/mmf_hg_segw_anyk.h"
#include "../../include/ext/mmf_hg_topk16_anyk.h"
#include "../../include/ext/mmf_hg_topk16_xy_anyk.h"
#include "../../include/ext/mmf_hg_hgconv.h"
#include "../../include/ext/mmf_hg_readout.h"
#include "../../include/ext/mmf_hg_hgpair.h"
#include "../../include/ext/mmf_hg_hg16.h"
#include "../../include/mmf_hg_wide.h"
#include "../../include/mmf_hg_wide_seg.h"

namespace mmf {

void set_error(const char* fmt, ...);

#define MMF_HIP(call)                                                                      \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess) {                                                                \
      mmf::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      return MMF_E_HIP;                                                                    \
    }                                                                                      \
  } while (0)

#define MMF_LAUNCH_CHECK()                                                                 \
  do {                                                                                     \
    hipError_t _e = hipGetLastError();                                                     \
    if (_e != hipSuccess) {                                                                \
      mmf::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
      return MMF_E_HIP;                                                                    \
    }                                                                                      \
  } while (0)

#define MMF_TRY(expr)            \
  do {                           \
    int _rc = (expr);            \
    if (_rc != MMF_OK) return _rc; \
  } while (0)

// What a cached workspace still holds from the previous call on its stream and a later call may use as it is (one thing:
// the work tables of the symmetric scan, which depend on the row-block count, G, the direction, the phase count and the
// antipodal switch alone).  Handing the
// workspace out forgets it — whoever takes the buffer may overwrite every byte — and gives the taker what was kept until
// then (Workspace::kept); a call that finds or writes the same content at the same place files it again (*Workspace::keep).
struct WsKept {
  const void* where = nullptr;
  int64_t row_blocks = 0;
  int group = 0, forward = 0, phases = 0, antipodal = 0;
  bool operator==(const WsKept& o) const {
    return where == o.where && row_blocks == o.row_blocks && group == o.group && forward == o.forward && phases == o.phases &&
           antipodal == o.antipodal;
  }
};

// Bump allocator over one cached device buffer per (device, stream).
struct Workspace {
  char* base = nullptr;
  size_t cap = 0;
  size_t off = 0;
  WsKept kept;              // what the buffer held when it was handed out
  WsKept* keep = nullptr;   // where to file what it holds now (nullptr: nowhere)
  void reset() { off = 0; }
  template <typename T>
  T* take(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base + off);
    off += bytes;
    return p;
  }
};
inline size_t ws_bytes(size_t count, size_t elem) { return (count * elem + 255) & ~size_t(255); }

// A host table (the caller's ptr_host, a local std::vector) on its way to the device, for entries that return without
// synchronising: the bytes are copied AT CALL TIME into pinned memory that the library owns, and the copy to `dst` is
// enqueued on `s` from there.  The caller's memory may die as soon as the call returns, and the call never waits for the
// stream (hipMemcpyAsync out of pageable memory does, from tables of about 1 MiB on: tests/test_gpu_stream_contract.py).
// The pinned blocks are kept per (current device, stream), each guarded by an event recorded behind its copy, and are
// handed out again once the stream has passed that event; mmf_release_workspaces frees them.
int upload_table(hipStream_t s, void* dst, const void* src_host, size_t bytes);

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    // a refused device is reported through the entry's status; HIP also keeps it as the thread's last error, where the next
    // launch check of this process — the library's or the caller's framework's — would find it and blame an unrelated call
    else (void)hipGetLastError();
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// mmf_api.hip: a workspace of at least `bytes` for (device, stream), slot 0 or 1 (Call::workspace)
int get_workspace_slot(int device, hipStream_t stream, int slot, size_t bytes, Workspace* out);

// The prologue of every entry that takes (device_id, hip_stream), in the order it has to run.  on_device() is the entry's first
// check.  Then come its checks of the host arguments: with device_id = 0 on a machine without a GPU they still answer
// MMF_E_INVALID, not MMF_E_HIP.  Then begin(): it sets the device (restored when the Call goes) and only then gives out the
// caller's stream and a workspace, so neither can be had past a refused device or ahead of the host checks.
struct Call {
  const char* who;           // the entry, for error messages
  hipStream_t s = nullptr;   // the caller's stream, from begin()
  Workspace ws;              // the call's slot-0 workspace, from begin(bytes)
  Call(const char* who_, int device_id, void* hip_stream) : who(who_), device(device_id), stream(static_cast<hipStream_t>(hip_stream)) {}
  int on_device() const {
    if (device >= 0) return MMF_OK;
    set_error("%s: device_id %d: no CPU path (the CPU restatement is oracle/, tests only)", who, device);
    return MMF_E_UNSUPPORTED;
  }
  int begin() {
    MMF_TRY(on_device());
    guard.emplace(device);
    if (!guard->ok) { set_error("hipSetDevice(%d) failed", device); return MMF_E_HIP; }
    s = stream;
    return MMF_OK;
  }
  int begin(size_t bytes) {
    MMF_TRY(begin());
    return workspace(bytes, &ws);
  }
  // after begin(): a workspace whose size only work behind begin() settles, or (slot 1) what a rare branch needs on top
  int workspace(size_t bytes, Workspace* out, int slot = 0) const {
    if (!guard) { set_error("%s: workspace before begin() (internal invariant)", who); return MMF_E_INTERNAL; }
    return get_workspace_slot(device, stream, slot, bytes, out);
  }

 private:
  int device; hipStream_t stream;
  std::optional<DeviceGuard> guard;
};


// The host offsets ptr[n_seg + 1] of a segmented entry (mmf_api.hip): n_seg >= min_seg segments, start at 0, never decrease, at
// least min_rows per segment, end at `rows` (kAnyRows: wherever they end).  MMF_E_INVALID names the first bad segment.
constexpr int64_t kAnyRows = -1;
int check_offsets(const char* who, const char* name, const int64_t* ptr, int64_t n_seg, int64_t min_seg, int64_t min_rows, int64_t rows);

inline size_t dtype_size(int dt) { return dt == MMF_F32 ? 4 : 2; }

// ------------------------------------------------------------------------------------------------
// kernel launchers (one translation unit each)
// ------------------------------------------------------------------------------------------------

// mmf_prep.hip: canonical squared norms (or clamped norms for cosine) of every row.
// max_n (optional, device u32 holding float bits, zeroed by the caller) receives the largest n_i.
int launch_row_scalars(const void* X, int64_t n, int64_t d, int dtype, int metric, float* out,
                       uint32_t* max_n, hipStream_t s);

// candidate lists written by the scan kernels and read by the select kernel:
//   cnt[(row * lists + l)]            number of ids in list l of the row
//   ids[(row * lists + l) * cap + e]  LOCAL column index (0..m-1)
struct CandLists {
  uint32_t* cnt;
  uint32_t* ids;
  uint32_t* overflow;  // [n] nonzero when a list of the row overflowed
  int lists;           // lists per row = 2 * col_splits
  int cap;
  // 16-bit scan only (else nullptr): the entries' approximate keys and the row's error margin — with several
  // lists per row, select drops what the union of the lists proves irrelevant before the exact re-rank
  float* keys = nullptr;
  float* margin = nullptr;   // [n]
  int slot_ulp = 16;         // stored keys carry an id-slot number in their low mantissa bits: 16 (4 bits) or 32 (5 bits)
  // 16-bit scan only: per-row overflow lists (SpillSink, mmf_dev.h) — what the lane lists could not hold
  uint32_t* spill_cnt = nullptr;   // [n], zeroed before the first launch
  uint32_t* spill_ids = nullptr;   // [n][spill_cap], GLOBAL-mapped local column ids like `ids`
  int spill_cap = 0;
  int spill_stacks = 0;            // lists == 2: the row's two lanes fill its slots from both ends; spill_cnt[row] = front | back << 16
  // symmetric 16-bit scan only (else nullptr): the columns a row received from the scans of OTHER rows (launch_scan_b16_sym),
  // with their approximate keys (no slot bits) — select treats them as one more list
  uint32_t* sym_cnt = nullptr;     // [n] entries offered (may pass sym_cap: the row is then flagged for the exact rescan)
  uint2* sym_ent = nullptr;        // [n][sym_cap] (id, key bits): one 8-byte store files an entry, one 8-byte load reads it
  int sym_cap = 0;
};

// mmf_scan_bf16.hip: the symmetric schedule of a scan of X against itself.  nb row blocks of 256 rows in
// nb / G super-blocks of G (the last one also takes the nb % G left-over row blocks); launch 0 does the plain pairs (own and, for an even count, antipodal super-block), launch 1 the
// symmetric ones.  The table has sym_schedule_grid() entries of 8 ints: row block (-1: idle), first tile and tile count of
// two column ranges, the entry's list pair within its launch and its phase.  phases == 2: the symmetric launch's wrap-around
// pairs run behind all others (phase B, block ids of their own); antipodal: launch 0 does the own super-block alone and the
// antipodal pairs are symmetric ones.  The look-ahead table (forward) has neither.
constexpr int kSymListPairs = 3;        // list pairs of a row in the symmetric scan: launch 0, phase A, phase B
int64_t sym_schedule_grid(int64_t nb, int G);
int64_t sym_schedule_phase_b_begin(int64_t nb, int G);   // first block id of phase B (they run to the end of the grid)
void sym_schedule_table(int64_t nb, int G, int launch, int32_t* out, bool forward = false, int phases = 1, bool antipodal = false);
int sym_default_group(int64_t nb);
constexpr int kSymCap = 512;            // entries per row of CandLists::sym_ent (1.66 x the largest count on the bench rows, bf16 leg)
constexpr int kSymLogPerWave = 2304;    // 64-byte hit records of a wave's append log (DESIGN.md §4.1 "Capacity and memory": the fullest on the bench rows x 1.5, up to a multiple of 256)
int scan_b16_sym_log_cap();             // ... as this call uses it: MMF_SYMMETRIC_LOG_CAP (read per call) lowers it, for tests of the full-log path
struct SymBuffers {
  float* thr = nullptr;            // [n_pad] thresholds, then [n_pad / 8] group minima (four per 32-row tile), one allocation: one buffer resource
  uint32_t* log = nullptr;         // [grid * 8][kSymLogPerWave][16]
  uint32_t* log_cnt = nullptr;     // [3][grid * 8] per wave: records in its log, wave-tiles that passed the group test, wave-tiles with a hit
  uint32_t* val_cnt = nullptr;     // [grid * 8] values of each log's records that passed their recorded threshold (sym_scatter_kernel)
  int32_t* sched = nullptr;        // [2][grid][8]
  uint32_t* none_cnt = nullptr;    // [4] real rows that reached the symmetric launch without a threshold
  static size_t bytes(int64_t n_pad, int64_t grid) {
    return ws_bytes(n_pad + n_pad / 8, 4) + ws_bytes((size_t)grid * 8 * kSymLogPerWave * 16, 4) + ws_bytes((size_t)grid * 24, 4) +
           ws_bytes((size_t)grid * 8, 4) + ws_bytes((size_t)grid * 16, 4) + ws_bytes(4, 4);
  }
  void carve(Workspace& ws, int64_t n_pad, int64_t grid) {
    thr = ws.take<float>(n_pad + n_pad / 8); log = ws.take<uint32_t>((size_t)grid * 8 * kSymLogPerWave * 16);
    log_cnt = ws.take<uint32_t>((size_t)grid * 24); val_cnt = ws.take<uint32_t>((size_t)grid * 8); sched = ws.take<int32_t>((size_t)grid * 16); none_cnt = ws.take<uint32_t>(4);
  }
};

// Where a launch of the 16-bit scan sits inside a paneled scan (all zero: the whole problem in one launch).
struct ScanB16Panel {
  int list_base = 0;                                   // first of the row's list slots this launch writes
  uint32_t seg_len = 0, seg_stride = 0, id_off = 0;    // operand column i -> id_off + (i / seg_len) * seg_stride + i % seg_len
  int32_t* seed = nullptr;                             // [2][seed_stride]: best proven threshold / best dropped key per query
  int64_t seed_stride = 0;                             //   (ordered-int encoding), memset to 0x80 before the first launch
  int share = 0;                                       // more than one workgroup / launch scans each query
  int32_t* sunk = nullptr;                             // wide scan with overflow lists in the counter form: [seed_stride] best key
                                                       //   written to the row's overflow list (same encoding and memset), or nullptr
};

// mmf_prep.hip: the f32 operand image of mmf_scan_f32.hip — [prep_f32_rows(n)][prep_f32_dim(d)] floats, zero padded,
// de-interleaved inside every group of eight k (k0 k2 k4 k6 | k1 k3 k5 k7).  row_ids: optional gather of the rows.
int64_t prep_f32_rows(int64_t n);
int64_t prep_f32_dim(int64_t d);
size_t prep_f32_bytes(int64_t n, int64_t d);
int launch_prep_f32(const void* X, int64_t n, int64_t d, int dtype, const int32_t* row_ids, float* out, hipStream_t s);

struct ScanProblem {
  const void* X; int64_t n;       // query rows
  const void* Y; int64_t m;       // candidate rows (columns of the similarity matrix)
  const float* Xp = nullptr;      // f32 images (launch_prep_f32) of the rows to scan — gathered when row_ids is set —
  const float* Yp = nullptr;      //   and of the candidate rows: what the exact scan reads
  int64_t d;
  int dtype;
  int metric;
  float lambda;
  int kk;                         // entries to retain per query (k, +1 when self is excluded later)
  const float* rx;                // per-row scalar of X  (launch_row_scalars)
  const float* cy;                // per-row scalar of Y
  const int32_t* row_ids;         // optional: scan only these rows of X (fallback), else nullptr
  int64_t n_rows;                 // number of rows to scan (== n when row_ids == nullptr)
  int col_splits;
  const float* floor_key = nullptr;     // exact scan only: per query, offer only what ranks strictly after (floor_key, floor_id)
  const uint32_t* floor_id = nullptr;   //   in the total order — the later passes of a call with k + self > 44
  // exact scan only, optional (Pc set): rank by the exponent of K_h * K_g (mmf_simtopk_combined) — positions [rows][dp] f32 of
  // the query and candidate rows, chain(p, p) of each (launch_row_scalars), and lambda_g; metric MMF_RBF, lambda = lambda_h
  const float *Pq = nullptr, *Pc = nullptr, *pnq = nullptr, *pnc = nullptr;
  int dp = 0;
  float lambda_g = 0.0f;
};

// mmf_scan_f32.hip: exact scan on v_mfma_f32_32x32x2_f32 (any d, f32/bf16/f16 inputs).
int scan_f32_cap(int kk);  // list capacity the kernel will use for kk (0 = unsupported)
int launch_scan_f32(const ScanProblem& p, const CandLists& L, hipStream_t s, int* grid_out);

// the segmented exact scan: the host work table ([entries][8] int64) over the segments x_ptr / y_ptr [S + 1] with
// at least k admissible columns (*served_out), `col_splits` forced column ranges per segment (0: the runs of
// sim_dense_combined_seg_table), *ranges_out the largest range count; and ONE launch over its device copy, images / scalars /
// floors / lists covering all rows, ids = rows of Y, L.lists = 2 * ranges, counts zeroed by the caller
std::vector<int64_t> seg_exact_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int k, int exclude_self, int col_splits,
                                     int* ranges_out, std::vector<char>* served_out);
// the cross-segment scan: the table of the complement — per block of 128 rows of a segment, runs of the 128-row
// tiles of ALL of Y that do not lie wholly inside the segment's own rows y_ptr[s] .. y_ptr[s + 1]; the two bounds ride in the
// words seg_exact_table gives to the segment's first row and column count; *ranges_out the largest range count of a block
std::vector<int64_t> cross_seg_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int k, int col_splits, int* ranges_out);
// the 16-bit cross-segment scan: its [entries][8] int32 work table over row blocks of qt rows of X and the 32-row
// tiles of the plain image of Y (mmf_scan_f32.hip, beside cross_seg_table); *lists_out 2 x the largest entry count of a block, -1
// when a run cannot be kept inside the tile DMA's 32-bit offsets
std::vector<int32_t> cross_seg16_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int qt, int dp, int cap, int cand_budget,
                                       int col_splits, int* lists_out);
// the wide 16-bit cross-segment scan: the same rule over row blocks of 128 rows of X and the 128-row tiles of the
// plain image of Y, in the wide scan's entry layout; automatic runs fill 256 workgroups and are at least 8 tiles long
std::vector<int32_t> cross_segw_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int cap, int cand_budget, int col_splits,
                                      int* lists_out);
// cross: `sched` is a cross_seg_table, the kernel masks each entry's excluded range (no combined key); p.row_ids may then name
// gathered rows (the table's rows are positions of p.Xp and of the lists)
int launch_scan_f32_seg(const ScanProblem& p, const CandLists& L, const int64_t* sched, int64_t grid, hipStream_t s, bool cross = false);

// mmf_select.hip: canonical keys of the candidates, self dropped, top-k by (key desc, id asc).
struct SelectProblem {
  const void* X; int64_t n; const void* Y; int64_t m; int64_t d; int dtype; int metric; float lambda;
  int k; int exclude_self; int64_t row_offset; int64_t col_offset;
  const float* rx; const float* cy;
  const int32_t* row_ids; int64_t n_rows;
  int64_t* out_idx; float* out_val;
  int32_t* fail_rows; uint32_t* fail_count;   // rows whose lists overflowed (or came up short)
  uint32_t* cand_total;                        // optional accumulated candidate count
  bool two_pass = false;   // rows with overflow-list entries are handled by a second launch that has LDS room for them
  int out_stride = 0, out_off = 0;       // out_idx / out_val rows are out_stride wide (0: k) and this call fills columns out_off .. out_off + k
  float* floor_key_out = nullptr;        // optional: key and LOCAL column id of the last entry emitted per row (the next pass's floor),
                                         //   indexed by list position (two_pass with `perm`: by row — positions are only the scan's order)
  uint32_t* floor_id_out = nullptr;
  float* key_out = nullptr;              // optional (launch_select): the canonical key of every entry emitted, laid out like out_val
  void* order_scratch = nullptr;   // select_order_bytes(n_rows): that second launch walks its rows ordered by their smallest candidate id
  const int32_t* perm = nullptr;   // optional (row_ids must be null): list position -> row of X, a permutation of 0 .. n_rows - 1 — the scan
                                   // took its queries in that order (mmf_order.hip); X, rx, the outputs and fail_rows stay in row order
  // launch_rerank_combined only: the position fields of ScanProblem
  const float *Pq = nullptr, *Pc = nullptr, *pnq = nullptr, *pnc = nullptr;
  int dp = 0;
  float lambda_g = 0.0f;
};
size_t select_order_bytes(int64_t n);
// mmf_order.hip: the order in which the 16-bit scan takes its query rows (near-duplicate rows next to each other)
size_t query_order_bytes(int64_t n);
int query_order_pivots();
int query_order_last(int32_t* out_host, int64_t n);
void query_order_forget();   // the recorded permutation is gone (a new fast-path call has begun, or the workspaces were released)
int launch_query_order_probe(const uint16_t* ZQ, const float* q_zn, int64_t n, int dp, bool f16, void* scratch, int64_t* near, hipStream_t s);
int launch_query_order_apply(const uint16_t* ZQ, const float* q_zn, const float* q_rn, const float* q_un, int64_t n, int64_t n_pad,
                             int dp, bool f16, void* scratch, uint16_t* Zo, float* zno, float* rno, float* uno, const int32_t** perm,
                             hipStream_t s);
int launch_select(const SelectProblem& p, const CandLists& L, hipStream_t s);
// mmf_topk.hip: the re-rank of the combined key over the exact scan's lists (f32 rows, no row_ids / perm): key and value
// recomputed with fmaf chains over F and P, ranked by counting under better(); k entries per row from column out_off on, then
// -1 / -inf up to out_stride.  One pass of several (out_off != 0 or floor_key_out set): the columns before
// out_off are left alone, the entry of rank k - 1 leaves its key and LOCAL id in floor_key_out / floor_id_out, and only the
// last pass (no floor_key_out) pads
int launch_rerank_combined(const SelectProblem& p, const CandLists& L, hipStream_t s);
// mmf_topk_anyk.hip: the same re-rank with launch_select's `row_ids` (gathered rows: lists, overflow words and floor slots by list
// position, F, P, chains, self, outputs and the fail list by row) and `key_out` (the canonical key of every emitted entry) — the
// passes of mmf_simtopk_combined_fast_anyk; always the pass form: only a call without floor_key_out pads
int launch_rerank_combined_ext(const SelectProblem& p, const CandLists& L, hipStream_t s);
// mmf_api.hip: mmf_simtopk_combined behind its host checks (ptr: host offsets of n_seg >= 1 segments) — ExactPass over the segments
int run_simtopk_combined(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g,
                         int k, int exclude_self, const int64_t* ptr, int64_t n_seg, int64_t* out_idx, float* out_val,
                         const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream);
// exact top-k of a few rows (p.row_ids) against every column, no candidate lists; keys: p.n_rows * p.m floats
int launch_rows_exact(const SelectProblem& p, float* keys, hipStream_t s);
int launch_topk_merge(const int64_t* ia, const float* va, const int64_t* ib, const float* vb,
                      int64_t n, int k, int64_t* io, float* vo, hipStream_t s);
// w_e = max(0, cos(x_i, x_j)) of every edge; nrm: the rows' clamped norms (launch_row_scalars, MMF_COSINE)
int launch_edge_cosine_impl(const void* X, int64_t d, int dtype, const float* nrm, const int64_t* ei, int64_t E,
                            float* out, hipStream_t s);

// mmf_scan_bf16.hip: the 16-bit scan (fast path) — what it supports, its operand images, its launches and their scratch
int scan_bf16_supported(int64_t d, int kk, int dtype);
int scan_bf16_cap(int kk, int dp);
int scan_bf16_dp(int64_t d);
// The 16-bit operand image of one side: what launch_prep_half writes and the scan reads.  Z [n_pad][dp] operands, zn / rn / un
// [n_pad] norms of the rounded row, of the rounding residual and of the row, cb [n_pad] per-candidate bias (-inf: padding),
// maxima [4] float bits (max zn, max rn, max un, max |cb|; zeroed by the caller before the prep).
struct HalfImage {
  uint16_t* Z = nullptr;
  float *zn = nullptr, *rn = nullptr, *un = nullptr, *cb = nullptr;
  uint32_t* maxima = nullptr;
  int64_t n_pad = 0;
  static size_t bytes(int64_t n_pad, int dp) { return ws_bytes((size_t)n_pad * dp, 2) + 4 * ws_bytes(n_pad, 4) + ws_bytes(4, 4); }
  void carve(Workspace& ws, int64_t n_pad_, int dp) {
    n_pad = n_pad_;
    Z = ws.take<uint16_t>((size_t)n_pad * dp);
    zn = ws.take<float>(n_pad); rn = ws.take<float>(n_pad); un = ws.take<float>(n_pad); cb = ws.take<float>(n_pad);
    maxima = ws.take<uint32_t>(4);
  }
  // rows r0 .. of this image as an image of their own (the queries of a row slice; they share the maxima)
  HalfImage from_row(int64_t r0, int dp) const { return {Z + (size_t)r0 * dp, zn + r0, rn + r0, un + r0, cb + r0, maxima, n_pad - r0}; }
  // a side the caller prepared (mmf_prep_rows): only ever read through the image
  static HalfImage of(const mmf_prepared_side& p, const float* maxima, int64_t n_pad) {
    return {static_cast<uint16_t*>(const_cast<void*>(p.Z)), const_cast<float*>(p.zn), const_cast<float*>(p.rn), const_cast<float*>(p.un),
            const_cast<float*>(p.cb), reinterpret_cast<uint32_t*>(const_cast<float*>(maxima)), n_pad};
  }
};
// the rows an image is made of: scal their canonical row scalars (launch_row_scalars), max_n the float bits of the largest
// squared norm over both sides (unused for cosine)
struct PrepRows { const void* X; int64_t n, d; int dtype, metric; const float* scal; const uint32_t* max_n; };
int launch_prep_half(const PrepRows& r, const HalfImage& out, int dp, bool f16, hipStream_t s);
// positions [0, n_pos) of the image are rows gather[pos] of X (-1: padding), positions [n_pos, n_pad) padding
int launch_prep_half_gather(const PrepRows& r, const int32_t* gather, int64_t n_pos, const HalfImage& out, int dp, bool f16, hipStream_t s);

// What every launch of the 16-bit scan needs: the query image (the scan reads Z / zn / rn / un of it), Z / cb / maxima of the
// candidate side, and the shape.  m_pad: candidate rows covered by tiles (multiple of 256).
struct ScanB16Problem {
  const void* ZQ; const float *q_zn, *q_rn, *q_un;
  const void* ZC; const float* cb; const uint32_t* maxima;
  int64_t n_rows, m, m_pad;
  int dp; int64_t d; bool f16; int metric, kk;
  ScanB16Problem(const HalfImage& q, const HalfImage& c, int64_t n_rows_, int64_t m_, int64_t m_pad_, int dp_, int64_t d_, bool f16_,
                 int metric_, int kk_)
      : ZQ(q.Z), q_zn(q.zn), q_rn(q.rn), q_un(q.un), ZC(c.Z), cb(c.cb), maxima(c.maxima), n_rows(n_rows_), m(m_), m_pad(m_pad_),
        dp(dp_), d(d_), f16(f16_), metric(metric_), kk(kk_) {}
};
// col_splits must be a power of two.  Lists are indexed by query position.
int launch_scan_b16(const ScanB16Problem& p, int col_splits, const CandLists& L, void* scratch, const ScanB16Panel& pn, hipStream_t s,
                    int* grid_out);
int launch_scan_b16_audit(const ScanB16Panel& pn, uint32_t* overflow, int64_t n_rows, hipStream_t s);
// The later passes of mmf_simtopk_fast_anyk: the plain launch with a ceiling per query row — a scanned value above
// ceil[row] ([n_pad], the kernel's units, +inf for padding rows) reaches no list, overflow list or threshold — and the kernel that
// turns the rows' floors (canonical keys, [p.n_rows]) into those ceilings: rx the rows' canonical scalars, max_n the word the
// operand images took their scale from, cap the lane lists' capacity of the launch that follows
int launch_scan_b16_ceil(const ScanB16Problem& p, int col_splits, const CandLists& L, void* scratch, const ScanB16Panel& pn, const float* ceil,
                         hipStream_t s, int* grid_out);
int launch_scan_b16_ceilings(const ScanB16Problem& p, int cap, const float* floor_key, const float* rx, const uint32_t* max_n, float lambda,
                             int64_t n_pad, float* ceil, hipStream_t s);
size_t scan_b16_sym_scratch_bytes(int64_t n_rows, int G);
// G: row blocks per super-block; live / forward / prune: MMF_SYMMETRIC_LIVE and MMF_SYMMETRIC_PRUNE as read by the caller;
// phases / antipodal: MMF_SYMMETRIC_PHASES and MMF_SYMMETRIC_ANTIPODAL (sym_schedule_table);
// tables: build and upload the two work tables (false: SymBuffers::sched still holds them)
struct SymLaunch { int G; bool live, forward, prune, tables; int phases = 2; bool antipodal = false; };
int launch_scan_b16_sym(const ScanB16Problem& p, const SymLaunch& y, const CandLists& L, void* scratch, const SymBuffers& sb,
                        const ScanB16Panel& pn, hipStream_t s, int* grid_out);
size_t scan_b16_scratch_bytes(int64_t n_rows, int col_splits, int dp, int cap);
int scan_bf16_slot_ulp(int cap);
int scan_b16_queries_per_block(int dp);
size_t scan_b16_seg_scratch_bytes(int64_t grid, int dp, int cap);
int launch_scan_b16_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const CandLists& L, void* scratch,
                        const ScanB16Panel& pn, hipStream_t s);
// The later passes of mmf_simtopk_segmented_fast_anyk: the table-driven launch with a ceiling per OPERAND POSITION
// (ceil [nq_pad], positions of the segment-padded query image; +inf for padding) — full-depth lists only (32 entries at d <= 512, the
// split-k pair kernel at d <= 1024) — and the ceilings of those positions: gather [n_pos] is the row of X at each position (-1:
// padding), floor_key and rx are indexed by row of X, the margin's maxima are those of the whole padded candidate image
int launch_scan_b16_seg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const CandLists& L, void* scratch,
                             const ScanB16Panel& pn, const float* ceil, hipStream_t s);
int launch_scan_b16_ceilings_gather(const ScanB16Problem& p, int cap, const int32_t* gather, int64_t n_pos, const float* floor_key, const float* rx,
                                    const uint32_t* max_n, float lambda, int64_t nq_pad, float* ceil, hipStream_t s);
// the cross-segment flavour: plain images on both sides, `sched` a device copy of cross_seg16_table, `bounds`
// [n_pad][2] the excluded column range (first, count) of every query row, L.lists = the table's list count, pn.share as the table says
int launch_scan_b16_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, const CandLists& L,
                         void* scratch, const ScanB16Panel& pn, hipStream_t s);
// the later passes of mmf_simtopk_cross_segments_fast_anyk: the same launch under a ceiling per query row (ceil
// [n_pad] by row of X, what launch_scan_b16_ceilings leaves: the plain images' positions are rows) — full-depth lists only
int launch_scan_b16_xseg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, const CandLists& L,
                              void* scratch, const ScanB16Panel& pn, const float* ceil, hipStream_t s);

// mmf_fast_anyk.hip: the per-row bookkeeping of mmf_simtopk_fast_anyk's later passes.  The re-rank of such a pass
// fills a staging row per query: `depth` entries in the final order (ids with col_offset added, values, canonical keys).
struct AnykStage { const int64_t* idx; const float* val; const float* key; int64_t n; int depth; int64_t col_offset; };
// certified [n]: -1 for the rows of the re-rank's fail list, else the staged entries that rank strictly after the row's floor;
// hist [depth + 3]: rows per certified count, then the flagged rows, then the largest number of entries dropped for a row
int launch_anyk_count(const AnykStage& st, const int32_t* fail_rows, const uint32_t* fail_count, const float* floor_key, const uint32_t* floor_id,
                      int32_t* certified, uint32_t* hist, hipStream_t s);
// rows with certified >= t: t entries to columns done .. of the out_stride-wide outputs, and the new floor; the others: listed for the
// exact rescan (rescan_rows [n], *rescan_count)
int launch_anyk_emit(const AnykStage& st, const int32_t* certified, int t, int done, int out_stride, int64_t* out_idx, float* out_val,
                     float* floor_key, uint32_t* floor_id, int32_t* rescan_rows, uint32_t* rescan_count, hipStream_t s);
int launch_anyk_iota(int32_t* rows, int64_t n, hipStream_t s);
// floors of the gathered rows rows[0 .. cnt): from their row-indexed home to a position-indexed block, or (back) home again
int launch_floor_move(const int32_t* rows, int64_t cnt, float* row_key, uint32_t* row_id, float* pos_key, uint32_t* pos_id, bool back,
                      hipStream_t s);
// mmf_simtopk_segmented_fast_anyk keeps the floors' ids as rows of Y; an exact pass over the gathered rows of one
// segment reads and leaves ids local to that segment's columns.  floor_id[rows[i]] -= col0[rows[i]] (add: +=) for i < cnt, col0 [n] the
// first row of Y of each row's segment
int launch_floor_rebase(const int32_t* rows, int64_t cnt, uint32_t* floor_id, const int32_t* col0, bool add, hipStream_t s);

// mmf_scan_b16w.hip: the wide 16-bit scan (1024 < d <= 4096, k + self <= 20) — both operands streamed through
// LDS in k-chunks.  Same operand images (dp = d rounded up to 128), lists, threshold buffers and audit as launch_scan_b16; no
// id scratch, no overflow lists, no panels, no shared thresholds.  col_splits must be a power of two, L.lists == 2 * col_splits.
int scan_b16w_supported(int64_t d, int kk);
int scan_b16w_cap(int kk);
int scan_b16w_dp(int64_t d);
int scan_b16w_queries_per_block();
int scan_b16w_col_tile();
int launch_scan_b16w(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, hipStream_t s, int* grid_out);
// The later passes of mmf_simtopk_wide_anyk, as launch_scan_b16_ceil / launch_scan_b16_ceilings serve
// mmf_simtopk_fast_anyk: the plain launch with a ceiling per query row — a scanned value above ceil[row] ([n_pad], the kernel's
// units, +inf for padding rows; n_pad covers whole 128-row blocks) reaches no list, overflow list or threshold — and the kernel
// that turns the rows' floors (canonical keys, [p.n_rows]) into those ceilings with the wide scan's margin: rx the rows' canonical
// scalars, max_n the word the operand images took their scale from
int launch_scan_b16w_ceil(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s,
                          int* grid_out);
int launch_scan_b16w_ceilings(const ScanB16Problem& p, const float* floor_key, const float* rx, const uint32_t* max_n, float lambda, int64_t n_pad,
                              float* ceil, hipStream_t s);
// Segmented form: one workgroup per entry of the device work table `sched` ([grid][8] int32: query position in the
// query image, row of X, real queries, first / end tile in the candidate image, id offset, list slot).  p.n_rows: rows of X (lists,
// thresholds and margins are indexed by them); both images are padded per segment to 128 rows.  lists == L.lists == 2 x the
// largest number of column ranges of a segment (a power of two).
int launch_scan_b16w_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                         hipStream_t s);
// The later passes of mmf_simtopk_segmented_wide_anyk: the same launch with a ceiling per OPERAND POSITION (ceil
// [nq_pad], positions of the segment-padded query image; +inf for padding) — full-depth lists only — and the ceilings of those
// positions: gather [n_pos] is the row of X at each position (-1: padding), floor_key and rx are indexed by row of X, the norms by
// position, the margin's maxima are those of the whole padded candidate image
int launch_scan_b16w_seg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                              const float* ceil, hipStream_t s);
int launch_scan_b16w_ceilings_gather(const ScanB16Problem& p, const int32_t* gather, int64_t n_pos, const float* floor_key, const float* rx,
                                     const uint32_t* max_n, float lambda, int64_t nq_pad, float* ceil, hipStream_t s);
// Cross-segment form: plain images on both sides, `sched` a device copy of cross_segw_table, `bounds` [n_pad][2]
// the excluded column range (first, count) of every query row, lists == L.lists == the table's list count (any even number).
int launch_scan_b16w_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                          const ScanB16Panel& pn, hipStream_t s);
// the later passes of mmf_simtopk_cross_segments_wide_anyk: the same launch under a ceiling per query row (ceil
// [n_pad] by row of X, what launch_scan_b16w_ceilings leaves: the plain images' positions are rows) — full-depth lists only
int launch_scan_b16w_xseg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                               const ScanB16Panel& pn, const float* ceil, hipStream_t s);

// mmf_scan_b16c.hip: the 16-bit scan of the combined key eh + eg (mmf_simtopk_combined_fast), 1 <= d <= 4096,
// k + self <= 20: the wide scan's structure with the position term formed in the epilogue.  One MMF_RBF operand image scanned
// against itself (p.ZQ == p.ZC, p.n_rows == p.m, dp = d rounded up to 128); lists, threshold buffers and audit as launch_scan_b16w,
// L.margin receives m0_i of margin_i(t) = m0_i + m1 |t|.
struct ScanB16Comb {
  const float* P; const float* pn;    // positions [n][dp] and chain(p, p) of every row (launch_row_scalars)
  const float* nf;                    // chain(f, f) of every row
  const uint32_t* max_nf;             // float bits of the largest nf: the word the prep took its scale from
  const uint32_t* max_pn;             // float bits of the largest pn
  int dp; float lambda_h, lambda_g;
};
int scan_b16c_supported(int64_t d, int kk);
int scan_b16c_cap(int kk);
int scan_b16c_dp(int64_t d);
int launch_scan_b16c(const ScanB16Problem& p, const ScanB16Comb& c, int col_splits, const CandLists& L, const ScanB16Panel& pn, hipStream_t s,
                     int* grid_out);
// the same scan over a ragged batch: one workgroup per entry of the device work table `sched` ([grid][8] int32);
// p.m_pad: positions of the one image, every segment padded to whole tiles of 128; `lists` = 2 x the largest range count
int launch_scan_b16c_seg(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, const CandLists& L,
                         const ScanB16Panel& pn, hipStream_t s);
// The later passes of mmf_simtopk_combined_fast_anyk: the same launch with a ceiling per row of F — an approximate
// key above ceil[row] reaches no list, threshold or seed (32-entry lists only) — and the kernel that turns the rows' floors (canonical
// combined keys, by row of F; -inf: no column left) into ceilings: gather [n_pos] maps an image position to its row of F (-1: padding)
int launch_scan_b16c_seg_ceil(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, const CandLists& L,
                              const ScanB16Panel& pn, const float* ceil, hipStream_t s);
int launch_scan_b16c_ceilings(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* gather, int64_t n_pos, const float* floor_key,
                              float* ceil, hipStream_t s);
// the same scan for queries that are not the candidates, or only some of them (mmf_simtopk_combined_xy): the table
// names, per workgroup, a block of 128 queries anywhere in the one image and a range of CANDIDATE tiles.  c.P / c.pn / c.nf are in
// the joint numbering of the table (candidates first); the lists, threshold buffers and margins hold only the p.n_rows queries,
// whose first one is row `list_row0` of that numbering; p.m: candidate rows, p.m_pad: positions of the image
int launch_scan_b16c_xy(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, int64_t list_row0,
                        const CandLists& L, const ScanB16Panel& pn, hipStream_t s);
// The later passes of mmf_simtopk_combined_xy_fast_anyk: launch_scan_b16c_xy under a ceiling per QUERY (ceil
// [p.n_rows], its base moved back like the lists'; 32-entry lists only), and the ceilings of the queries of such an image from their
// floors (floor_key / ceil [p.n_rows] by query; -inf: no column left): query i sits at image position q_pos0 + i and is row
// q_row0 + i of the joint numbering; iota [p.n_rows] = 0, 1, ... (launch_anyk_iota) is the kernel's position -> row table
int launch_scan_b16c_xy_ceil(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, int64_t list_row0,
                             const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s);
int launch_scan_b16c_xy_ceilings(const ScanB16Problem& p, const ScanB16Comb& c, int64_t q_pos0, int64_t q_row0, const int32_t* iota,
                                 const float* floor_key, float* ceil, hipStream_t s);
// mmf_api.hip: mmf_simtopk_combined_xy behind its host checks — the exact pass over the queries against the candidates, or the
// table-driven 16-bit scan, audit, re-rank and the exact pass over the row blocks of flagged rows
int run_simtopk_combined_xy(const char* who, const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                            int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self, int64_t row_offset,
                            int64_t col_offset, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                            int device_id, void* hip_stream);
// mmf_api.hip: mmf_simtopk_combined_fast behind its host checks (one graph) — 16-bit scan, audit, re-rank of the combined key,
// exact pass over the row blocks of flagged rows; MMF_PREC_EXACT (and AUTO where the fast path does not pay): run_simtopk_combined
int run_simtopk_combined_fast(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                              float lambda_g, int k, int exclude_self, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                              mmf_simtopk_stats* stats, int device_id, void* hip_stream);
// mmf_api.hip: mmf_simtopk_combined_fast_segmented behind its host checks (ptr: host offsets of n_seg >= 0 segments) — one table-driven
// launch of the 16-bit scan for every segment with at least k admissible columns, the exact pass for the others and for flagged rows
int run_simtopk_combined_fast_segmented(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                        float lambda_g, int k, int exclude_self, const int64_t* ptr, int64_t n_seg, int64_t* out_idx,
                                        float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream);

// mmf_dense.hip
// Xp / Yp: f32 images of X and Y (launch_prep_f32; unused — may be null — for d <= 8 and MMF_RBF_DIRECT)
bool sim_dense_needs_images(int64_t d, int metric);
int launch_sim_dense(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int dtype,
                     int metric, float lambda, const float* rx, const float* cy, const float* Xp, const float* Yp,
                     float* out, hipStream_t s);
// rows [row0, row0 + rows) of the combined n x n similarity; out [rows, n].  Fp: f32 image of all n rows of F.
int launch_sim_dense_combined(const float* Fp, const float* P, int64_t n, int64_t d, int64_t dp,
                              float lambda_h, float lambda_g, const float* nf, int64_t row0, int64_t rows, float* out,
                              hipStream_t s);
// segmented (mmf_sim_dense_combined_segmented): the host-built work table over the segments ptr[0..S] ([entries][8] int64,
// block s of the output at sum_{t<s} n_t^2), and the launch over its device copy; Fp / nf / P cover all rows of the batch
std::vector<int64_t> sim_dense_combined_seg_table(const int64_t* ptr, int64_t S);
int launch_sim_dense_combined_seg(const float* Fp, const float* P, int64_t d, int64_t dp, float lambda_h, float lambda_g,
                                  const float* nf, const int64_t* sched, int64_t grid, float* out, hipStream_t s);

// mmf_edges.hip
// Lower medians (torch.median: element (count - 1) / 2).  A population of 4 M values or more is first tried in ONE sweep
// (sampled bracket, exact counts, select among the ~3 % inside the bracket; one host sync for the verdict); the four-pass
// radix select is the fallback and the small-size path.  MMF_MEDIAN_RADIX=1 forces the latter.
using MedianConsume = std::function<int(const float* data, int64_t cols, int64_t row0, int64_t rows)>;
using MedianSweep = std::function<int(const MedianConsume&)>;      // streams the whole population once through `consume`
using MedianSampler = std::function<int(float* sample, int s)>;   // s values at hashed positions (device)
size_t median_scratch_bytes(unsigned long long count);
int64_t median_no_diagonal_row();                                  // row0 for data without a diagonal to skip
// A sweep whose rows are never all in memory (mmf_stream_stats.hip): the statistic partials of lower_median_of's one sweep are
// those of ONE launch of `grid` workgroups over all the whole rows, the lanes' running sums kept in `lanes` between the runs.
// The sweep sets row0 before every consume(): the index of the run's first row among all rows, or -1 for the ragged last row.
struct SweepCarry {
  void* lanes;          // stat_lanes_bytes(grid)
  int64_t grid;         // workgroups of that one launch: min((rows + 3) / 4, 2040)
  int64_t row0;
};
int lower_median_of(unsigned long long count, const MedianSampler& sampler, const MedianSweep& sweep, float* out, void* scratch,
                    hipStream_t s, void* stat_part = nullptr, const float* stat_pivot = nullptr, int64_t* stat_nparts = nullptr,
                    SweepCarry* carry = nullptr);
bool median_one_sweep(unsigned long long count);                   // does lower_median_of try its one sweep for this population?
size_t stat_lanes_bytes(int64_t grid);
int launch_stat_lanes_init(void* lanes, int64_t grid, hipStream_t s);
int launch_stat_lanes_finish(void* lanes, int64_t grid, void* part /* [grid] partials */, hipStream_t s);
// stats_partial_kernel's assignment, run by run: its grid for `count` values, and one run of the array (v = values
// [4 group0, 4 group0 + count) of it; only the array's last run may have count % 4 != 0; pivot[0] = the array's first value)
int64_t stats_partial_grid(int64_t count);
int launch_stats_partial_carry(const float* v, int64_t count, int64_t group0, const float* pivot, void* lanes, int64_t grid, hipStream_t s);
int launch_sample_gather(const float* data, int64_t n_sq, unsigned long long count, float* sample, int s_count, hipStream_t s);
int launch_sample_pairs(const void* A, const void* B, int64_t nb, int64_t d, int dtype, float lambda, const float* P, int dp,
                        float lambda_g, int offdiag, unsigned long long count, float* sample, int s_count, hipStream_t s);
int launch_offdiag_lower_median(const float* K, int64_t n, float* out, void* scratch /* median_scratch_bytes(n (n - 1)) */,
                                hipStream_t s);
// the radix select in pieces (matrices recomputed panel by panel): begin; for pass 0..3 { accumulate panels; next }
int launch_median_accumulate(const float* K, int64_t n, int64_t row0, int64_t rows, void* state, int pass, hipStream_t s);
int launch_median_next(void* state, int pass, float* out, hipStream_t s);
int launch_median_begin_count(void* state, unsigned long long count, hipStream_t s);
// lower median of a flat array (scratch: median_scratch_bytes(count)); mean / std / min / max / median of a flat array
int launch_lower_median(const float* v, int64_t count, float* out, void* scratch, hipStream_t s);
int launch_stats_finish(const void* part, int64_t nparts, const float* pivot, int64_t count, double* out, hipStream_t s);
int launch_stats_set_median(const float* med, double* out, hipStream_t s);
size_t stat_partial_bytes();
// mmf_direct.hip: register-tiled direct-difference RBF with optional per-workgroup statistic partials
int64_t rbf_direct_blocks(int64_t n, int64_t m);
int launch_rbf_direct_pivot(const void* X, const void* Y, int64_t d, int dtype, float lambda, float* pivot, hipStream_t s);
int launch_rbf_direct(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int dtype, float lambda, float* out,
                      void* part, const float* pivot, hipStream_t s);
size_t array_stats_scratch_bytes(int64_t count);
int launch_array_stats(const float* v, int64_t count, double* out /*[5] device*/, void* scratch, hipStream_t s);
int launch_threshold_edges_panel(const float* K, int64_t n, int64_t row0, int64_t rows, float thr, int64_t* ei_row,
                                 int64_t* ei_col, float* ew, int64_t capacity, int64_t* out_count, uint32_t* scratch,
                                 size_t scratch_u32, hipStream_t s);
int launch_threshold_edges(const float* K, int64_t n, float thr, int64_t* ei, float* ew,
                           int64_t capacity, int64_t* out_count, uint32_t* scratch, size_t scratch_u32,
                           hipStream_t s);

int launch_threshold_count(const float* K, int64_t n, float thr, unsigned long long* row_off, int64_t* out_count, uint32_t* row_cnt,
                           hipStream_t s);
int launch_threshold_fill(const float* K, int64_t n, float thr, const unsigned long long* row_off, int64_t* ei, float* ew,
                          int64_t capacity, hipStream_t s);
// segmented: the blocks K_s (n_s x n_s) stored one after the other from kptr[s] = sum_{t<s} n_t^2.  ptr: HOST offsets (every
// n_s >= 2) for the median, which uploads its own tables into `scratch`; device copies d_ptr / d_kptr for the edges.
size_t offdiag_lower_median_seg_scratch_bytes(const int64_t* ptr, int64_t S);
int launch_offdiag_lower_median_seg(const float* K, const int64_t* ptr, int64_t S, float* out, void* scratch, hipStream_t s);
// flat blocks v[bptr[s] .. bptr[s+1]) (HOST offsets, every block >= 1 value): mmf_lower_median of every block, no synchronisation
size_t lower_median_seg_scratch_bytes(const int64_t* bptr, int64_t S);
int launch_lower_median_seg(const float* v, const int64_t* bptr, int64_t S, float* out, void* scratch, hipStream_t s);
// per-segment merge of statistic partials (part[pbase[s] .. pbase[s+1]), pivot[s], count = n_s m_s -> out[s][0..3]) and out[s][4] = med[s]
int launch_stats_finish_seg(const void* part, const int64_t* d_pbase, const float* pivot, const int64_t* d_xptr, const int64_t* d_yptr,
                            int64_t S, double* out, hipStream_t s);
int launch_stats_set_median_seg(const float* med, int64_t S, double* out, hipStream_t s);
// mmf_direct.hip, segmented: work table ([entries][3]: segment, tile row, tile column) + first partial of every segment; pivots;
// the launch over the device copies of the tables
std::vector<int64_t> rbf_direct_seg_table(const int64_t* xptr, const int64_t* yptr, int64_t S, std::vector<int64_t>* pbase);
int launch_rbf_direct_pivot_seg(const void* X, const void* Y, int64_t d, int dtype, float lambda, const int64_t* d_xptr,
                                const int64_t* d_yptr, int64_t S, float* pivot, hipStream_t s);
int launch_rbf_direct_seg(const void* X, const void* Y, int64_t d, int dtype, float lambda, float* out, void* part, const float* pivot,
                          const int64_t* d_tab, int64_t grid, const int64_t* d_xptr, const int64_t* d_yptr, const int64_t* d_optr,
                          const int64_t* d_pbase, hipStream_t s);
int launch_threshold_count_seg(const float* K, const int64_t* d_ptr, const int64_t* d_kptr, int64_t S, int64_t n, const float* thr,
                               unsigned long long* row_off, int64_t* out_count, uint32_t* row_cnt, hipStream_t s);
int launch_threshold_fill_seg(const float* K, const int64_t* d_ptr, const int64_t* d_kptr, int64_t S, int64_t n, const float* thr,
                              const unsigned long long* row_off, int64_t* ei, float* ew, int64_t capacity, hipStream_t s);

// rows of a panel of a recomputed n x n matrix: the caller's panel_rows, or about 1 GiB of f32 (at least 128 rows, at most n)
inline int64_t pick_panel_rows(int64_t n, int64_t panel_rows) {
  if (panel_rows <= 0) panel_rows = (int64_t(1) << 30) / (4 * n);
  if (panel_rows < 128) panel_rows = 128;
  if (panel_rows > n) panel_rows = n;
  return panel_rows;
}

// mmf_segments.hip: cluster-shaped steps (labels -> members, per-cluster means, cliques, k-NN pair dedup)
int segment_max_segments();
size_t segment_sort_scratch_bytes(int64_t n, int64_t S);
int launch_segment_sort(const int64_t* labels, int64_t n, int64_t S, int64_t* counts, int64_t* offsets, int64_t* order,
                        void* scratch, uint32_t* bad, hipStream_t s);
int launch_segment_mean(const float* X, int64_t d, const int64_t* order, const int64_t* offsets, int64_t S, float* out, hipStream_t s);
size_t segment_offdiag_scratch_bytes(int64_t n);
int launch_segment_offdiag_mean(const float* K, int64_t n, const int64_t* order, const int64_t* offsets, int64_t S,
                                double* out_mean, void* scratch, hipStream_t s);
int launch_segment_member_clusters(const int64_t* offsets, int64_t S, int32_t* seg_of /* [n] */, hipStream_t s);
int launch_segment_offdiag_final(const double* row_sum, const int64_t* offsets, int64_t S, double* out_mean, hipStream_t s);
size_t clique_scratch_bytes(int64_t n, int64_t S);
int launch_clique_pairs(const int64_t* order, const int64_t* offsets, int64_t n, int64_t S, int64_t* lo, int64_t* hi,
                        int64_t capacity, int64_t* out_count, void* scratch, hipStream_t s);
// mmf_knn_clique.hip: the ordered k-NN + clique edge list of every segment (mmf_knn_clique_edges_count / _fill).  ptr: HOST
// offsets, uploaded into `scratch` (knn_clique_scratch_bytes) by both; labels local to the segment, nullptr = no cliques.
size_t knn_clique_scratch_bytes(int64_t n, int64_t n_seg, int64_t H, bool with_labels);
int launch_knn_clique_count(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t H, const int64_t* ptr, int64_t n_seg,
                            unsigned long long* row_off, int64_t* edge_ptr, int64_t* out_count, void* scratch, hipStream_t s);
int launch_knn_clique_fill(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t H, const int64_t* ptr, int64_t n_seg,
                           const unsigned long long* row_off, int64_t* edge_index, int64_t capacity, void* scratch, hipStream_t s);
// mmf_kmeans.hip: scikit-learn's KMeans fit, decision for decision, all restarts in lockstep (host-synchronous).
// Groups of consecutive segments [bounds[i], bounds[i + 1]) that fit one lockstep (n_seg n_init k <= segment_max_segments(),
// n_init rows < 2^31, bounded scratch); *max_bytes = the largest group's scratch.  The plain fit is ptr = {0, n}, one segment.
std::vector<int64_t> kmeans_segment_groups(const int64_t* ptr, int64_t n_seg, int64_t d, int64_t k, int64_t n_init, int trials, size_t* max_bytes);
// segmented: mmf_kmeans_fit_segmented (first_h [n_seg][n_init], info per segment, seeds as row ids of the batch); otherwise
// mmf_kmeans_fit on its one group
int launch_kmeans_fit(const float* X, int64_t d, const int64_t* ptr, const std::vector<int64_t>& groups, int64_t k, int64_t n_init, int trials,
                      const int64_t* first_h, const double* u_h, int max_iter, double tol, int64_t* out_labels, float* out_centres,
                      int64_t* out_seeds, double* info_h, void* scratch, hipStream_t s, bool segmented);
// The ragged fit (mmf_kmeans_fit_ragged): segment q is rows[q] x width[q] at element xoff[q] of the flat buffer V.  Groups as above,
// plus the padding rule: sum rows * km_ds(widest) <= 2 sum rows * km_ds(width) per group; ds_out (optional, [n_seg]) receives the
// internal width of each segment's group.  Labels in call order, centres [k][width] per segment back to back, seeds local rows.
std::vector<int64_t> kmeans_ragged_groups(const int64_t* rows, const int64_t* width, int64_t n_seg, int64_t k, int64_t n_init, int trials,
                                          size_t* max_bytes, int64_t* ds_out);
int launch_kmeans_fit_ragged(const float* V, const int64_t* xoff, const int64_t* rows, const int64_t* width, const std::vector<int64_t>& groups,
                             int64_t k, int64_t n_init, int trials, const int64_t* first_h, const double* u_h, int max_iter, double tol,
                             int64_t* out_labels, float* out_centres, int64_t* out_seeds, double* info_h, void* scratch, hipStream_t s);
int launch_knn_pairs(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t* lo, int64_t* hi, int64_t* out_count,
                     hipStream_t s);

}  // namespace mmf
