// mmf_api.hip — the C ABI of include/mmf_hg.h.  Host code only: validation, workspace layout,
// kernel sequencing.  No CPU compute path exists here (device_id < 0 is an error).
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <optional>
#include <utility>
#include <vector>

#include "mmf_host.h"

namespace mmf {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

struct WsEntry { char* base = nullptr; size_t cap = 0; WsKept kept; };
static std::mutex g_ws_mu;
static std::map<std::pair<int, hipStream_t>, WsEntry> g_ws[2];

// A workspace of at least `bytes` for (device, stream); reallocates (after a stream sync) when it has to grow.
// slot 0: the call's working set.  slot 1: what only a rare branch of a call needs on top of it (the f32 operand
// images of an exact rescan inside the 16-bit path), so that every call does not carry it.
int get_workspace_slot(int device, hipStream_t stream, int slot, size_t bytes, Workspace* out) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  WsEntry& e = g_ws[slot][std::make_pair(device, stream)];
  if (e.cap < bytes) {
    if (e.base) {
      MMF_HIP(hipStreamSynchronize(stream));
      MMF_HIP(hipFree(e.base));
      e.base = nullptr;
      e.cap = 0;
      e.kept = WsKept{};
    }
    size_t want = bytes + (bytes >> 3) + (1u << 20);
    void* p = nullptr;
    hipError_t rc = hipMalloc(&p, want);
    if (rc != hipSuccess) {
      set_error("workspace allocation of %zu bytes failed: %s", want, hipGetErrorString(rc));
      return MMF_E_NOMEM;
    }
    e.base = static_cast<char*>(p);
    e.cap = want;
  }
  out->base = e.base;
  out->cap = e.cap;
  out->off = 0;
  out->kept = e.kept;       // (a buffer that was just reallocated kept nothing: `where` cannot match)
  e.kept = WsKept{};
  out->keep = &e.kept;      // map nodes do not move
  return MMF_OK;
}

struct StageBlock { char* host = nullptr; size_t cap = 0; hipEvent_t passed = nullptr; bool in_flight = false; };
static std::map<std::pair<int, hipStream_t>, std::vector<StageBlock>> g_stage;

int upload_table(hipStream_t s, void* dst, const void* src_host, size_t bytes) {
  if (bytes == 0) return MMF_OK;
  int device = 0;
  MMF_HIP(hipGetDevice(&device));
  std::lock_guard<std::mutex> lk(g_ws_mu);
  std::vector<StageBlock>& blocks = g_stage[std::make_pair(device, s)];
  StageBlock* b = nullptr;
  for (StageBlock& c : blocks) {
    if (c.cap < bytes) continue;
    if (c.in_flight) {
      const hipError_t q = hipEventQuery(c.passed);
      if (q != hipSuccess) { (void)hipGetLastError(); continue; }      // hipErrorNotReady is not a failure of a later launch
      c.in_flight = false;
    }
    b = &c;
    break;
  }
  if (!b) {                                                              // nothing free: the stream is busy, take a new block, never wait
    StageBlock nb;
    nb.cap = (std::max(bytes, (size_t)1 << 16) + 4095) & ~size_t(4095);
    void* h = nullptr;
    hipError_t rc = hipHostMalloc(&h, nb.cap, hipHostMallocDefault);
    if (rc != hipSuccess) { set_error("pinned staging of %zu bytes failed: %s", nb.cap, hipGetErrorString(rc)); return MMF_E_NOMEM; }
    nb.host = static_cast<char*>(h);
    rc = hipEventCreateWithFlags(&nb.passed, hipEventDisableTiming);
    if (rc != hipSuccess) { (void)hipHostFree(h); set_error("hipEventCreate failed: %s", hipGetErrorString(rc)); return MMF_E_HIP; }
    blocks.push_back(nb);
    b = &blocks.back();
  }
  memcpy(b->host, src_host, bytes);
  MMF_HIP(hipMemcpyAsync(dst, b->host, bytes, hipMemcpyHostToDevice, s));
  MMF_HIP(hipEventRecord(b->passed, s));
  b->in_flight = true;
  return MMF_OK;
}

// The first checks of an entry that takes rows of features: the device, then shapes and dtype.
static int check_common(const Call& c, const void* X, int64_t n, int64_t m, int64_t d, int in_dtype) {
  MMF_TRY(c.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("bad shape n=%lld m=%lld d=%lld", (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("bad in_dtype %d", in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("X is NULL"); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("n and m must be < 2^31"); return MMF_E_UNSUPPORTED; }
  return MMF_OK;
}

// The host offsets ptr[n_seg + 1] of a segmented entry (`name`: the array as the caller knows it): n_seg >= min_seg segments,
// start at 0, never decrease, at least min_rows per segment, end at `rows` (kAnyRows: wherever they end).
int check_offsets(const char* who, const char* name, const int64_t* ptr, int64_t n_seg, int64_t min_seg, int64_t min_rows,
                         int64_t rows) {
  if (n_seg < min_seg || !ptr) {
    set_error("%s: need n_seg >= %lld and host offsets %s[n_seg + 1]", who, (long long)min_seg, name);
    return MMF_E_INVALID;
  }
  if (ptr[0] != 0) { set_error("%s: %s must start at 0 (got %lld)", who, name, (long long)ptr[0]); return MMF_E_INVALID; }
  for (int64_t g = 0; g < n_seg; ++g) {
    const int64_t ns = ptr[g + 1] - ptr[g];
    if (ns < 0) { set_error("%s: %s decreases at segment %lld", who, name, (long long)g); return MMF_E_INVALID; }
    if (ns < min_rows) {
      set_error("%s: segment %lld has %lld rows in %s, need at least %lld", who, (long long)g, (long long)ns, name, (long long)min_rows);
      return MMF_E_INVALID;
    }
  }
  if (rows != kAnyRows && ptr[n_seg] != rows) {
    set_error("%s: %s must end at %lld (got %lld)", who, name, (long long)rows, (long long)ptr[n_seg]);
    return MMF_E_INVALID;
  }
  return MMF_OK;
}

// HIP events are kept between calls (per device): creating and destroying eight of them per step showed up next to
// an 8 ms per-rank step.  An EventTimer borrows two from the pool and hands them back when it goes out of scope.
struct EventPool {
  std::mutex mu;
  std::map<int, std::vector<hipEvent_t>> idle;
  hipEvent_t get(int dev) {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto& v = idle[dev];
      if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  void put(int dev, hipEvent_t e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    idle[dev].push_back(e);
  }
};
static EventPool g_events;

struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  int dev = 0;
  int start(bool enable, hipStream_t s) {
    on = enable;
    if (!on) return MMF_OK;
    MMF_HIP(hipGetDevice(&dev));
    a = g_events.get(dev);
    b = g_events.get(dev);
    if (!a || !b) { set_error("hipEventCreate failed"); return MMF_E_HIP; }
    MMF_HIP(hipEventRecord(a, s));
    return MMF_OK;
  }
  int stop(hipStream_t s) {
    if (!on) return MMF_OK;
    MMF_HIP(hipEventRecord(b, s));
    return MMF_OK;
  }
  float ms() {
    float t = 0.f;
    if (on && a && b && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&t, a, b);
    return t;
  }
  ~EventTimer() {
    g_events.put(dev, a);
    g_events.put(dev, b);
  }
};

static int pick_splits(int64_t row_blocks, int64_t col_tiles, int cap, int forced) {
  int64_t s = forced > 0 ? forced : (768 + row_blocks - 1) / row_blocks;
  if (s > col_tiles) s = col_tiles;
  const int64_t max_lists = 1024 / cap;  // select kernel capacity per row
  if (2 * s > max_lists) s = max_lists / 2;
  if (s < 1) s = 1;
  return (int)s;
}

// Columns a row of rows [r0, r0 + n) may take from columns [c0, c0 + m): all m, minus one when self is excluded and a row's
// own id may lie among them (any overlap of the two ranges).
static int64_t admissible_columns(int64_t r0, int64_t n, int64_t c0, int64_t m, int exclude_self, bool* overlap = nullptr) {
  const bool o = exclude_self && r0 < c0 + m && r0 + n > c0;
  if (overlap) *overlap = o;
  return m - (o ? 1 : 0);
}

// What MMF_PREC_AUTO does where only the wide 16-bit scan applies (1024 < d <= 4096, k + self <= 20): it takes it.  Measured
// (profiles/wide_scan_timing.txt): the whole call is 4.6x / 4.3x faster than the exact scan at N = 16384 /
// 65536, d = 1536 — 125 and 431 times the exact arm's spread, where the rule asks for three.
static bool wide_scan_auto() { return true; }

// Whether the segmented wide scan splits its segments' columns on its own (FastTail's rule applied to the call).  It does not:
// measured at 4 segments of 4096 rows, d = 1536 (profiles/wide_segmented_timing.txt) the rule's two ranges took
// 1.090 ms against 1.411 ms for one — 2.9 times the spread of the one-range arm, where the project's rule asks for more than
// three.  opts->col_splits forces a count either way.
static bool wide_seg_auto_splits() { return false; }

// One simtopk call: its prologue (`call`), its arguments, and what check() derives from them.
struct Request {
  Call call;
  const void* X; int64_t n; const void* Y; int64_t m; int64_t d; int dtype, metric; float lambda;
  int k, exclude_self; int64_t row_offset, col_offset;   // ids reported: row_offset + row of X, col_offset + row of Y
  int64_t* out_idx; float* out_val; mmf_simtopk_stats* stats; bool profile;
  int kk = 0;                       // entries a row's lists keep: k, + 1 when self is excluded
  int precision = MMF_PREC_AUTO;    // resolved: MMF_PREC_EXACT, _FAST or _FAST_BF16
  bool wide_ok = false;             // the entry has the wide 16-bit scan (mmf_scan_b16w.hip) behind it: mmf_simtopk / _ex only
  bool wide = false;                // resolved: the 16-bit scan of this call is the wide one (1024 < d <= 4096)

  // The checks every simtopk entry makes, in this order: device / shapes / dtype, metric, lambda, k, the entry's own
  // (`entry_checks`); stats zeroed; then, when there are rows: outputs, admissible columns (of the whole block unless
  // `per_segment`), device, precision (`prec`: requested, or fixed by the operands; AUTO: the 16-bit scan if it applies).
  template <class F>
  int check(int prec, bool per_segment, F&& entry_checks) {
    const char* who = call.who;
    MMF_TRY(check_common(call, X, n, m, d, dtype));
    if (metric < MMF_DOT || metric > MMF_RBF) { set_error("%s: bad metric %d", who, metric); return MMF_E_INVALID; }
    if (metric == MMF_RBF && !(lambda > 0.0f)) { set_error("%s: MMF_RBF needs lambda > 0 (got %g)", who, lambda); return MMF_E_INVALID; }
    if (k < 1) { set_error("%s: k must be >= 1 (got %d)", who, k); return MMF_E_INVALID; }
    kk = k + (exclude_self ? 1 : 0);
    MMF_TRY(entry_checks());
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MMF_OK;
    if (!out_idx || !out_val) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    bool overlap = false;
    const int64_t adm = admissible_columns(row_offset, n, col_offset, m, exclude_self, &overlap);
    if (!per_segment && k > adm) {
      set_error("%s: k = %d exceeds the %lld admissible columns (m = %lld%s)", who, k, (long long)adm, (long long)m, overlap ? ", self excluded" : "");
      return MMF_E_INVALID;
    }
    MMF_TRY(call.begin());
    const bool narrow = scan_bf16_supported(d, kk, dtype);
    const bool b16 = narrow || (wide_ok && scan_b16w_supported(d, kk));
    // AUTO: the register-resident 16-bit scan where it applies; the wide one only where wide_scan_auto() says it pays
    precision = prec == MMF_PREC_AUTO ? ((narrow || (b16 && wide_scan_auto())) ? MMF_PREC_FAST : MMF_PREC_EXACT) : prec;
    if (precision != MMF_PREC_EXACT && precision != MMF_PREC_FAST && precision != MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", who, precision); return MMF_E_INVALID; }
    wide = precision != MMF_PREC_EXACT && !narrow && b16;
    if (precision != MMF_PREC_EXACT && !b16) {
      set_error("%s: MMF_PREC_FAST does not support d = %lld, k = %d (AUTO takes the exact scan there)", who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }

  // The re-rank of the whole call: operands, metric, k, id offsets, outputs.  The caller adds the row scalars, the flag block
  // and what its lists need.
  SelectProblem select() const {
    SelectProblem q{};
    q.X = X; q.n = n; q.Y = Y; q.m = m; q.d = d; q.dtype = dtype; q.metric = metric; q.lambda = lambda;
    q.k = k; q.exclude_self = exclude_self; q.row_offset = row_offset; q.col_offset = col_offset;
    q.n_rows = n; q.out_idx = out_idx; q.out_val = out_val;
    return q;
  }
};

// What a simtopk call reports (check() zeroed the rest).  h_tot: the re-rank's candidate counters.
static void fill_stats(mmf_simtopk_stats* st, int precision, int splits, int grid, float prep_ms, float scan_ms, float rerank_ms,
                       float fallback_ms, int64_t fallback_rows, int64_t overflow_rows, int64_t short_rows,
                       const std::vector<uint32_t>& h_tot, int64_t near_rows = -1) {
  if (!st) return;
  st->precision_used = precision; st->col_splits = splits; st->scan_grid = grid;
  st->prep_ms = prep_ms; st->scan_ms = scan_ms; st->rerank_ms = rerank_ms; st->fallback_ms = fallback_ms;
  st->fallback_rows = fallback_rows; st->overflow_rows = overflow_rows; st->short_rows = short_rows;
  for (uint32_t v : h_tot) st->candidates += v;
  st->near_rows = near_rows;
}

// overflow slots per row of the 16-bit scan for the columns a row's lane lists cannot hold (near-duplicate data); a row
// that fills them as well is redone exactly
static constexpr int kSpillCap = 192;

// one list pair per row: its two lanes fill the row's overflow slots from both ends (MMF_SPILL_COUNTER: one counter instead)
static int spill_stacks_for(int lists) { return (lists == 2 && !getenv("MMF_SPILL_COUNTER")) ? 1 : 0; }

// The 16-bit scan's candidate lists of n rows: `lists` lists of bcap entries per row, and the overflow lists.
static size_t b16_lists_bytes(int64_t n, int lists, int bcap) {
  const size_t e = (size_t)n * lists;
  return ws_bytes(e, 4) + ws_bytes(e * bcap, 4) + (lists > 2 ? ws_bytes(e * bcap, 4) + ws_bytes(n, 4) : 0) + 2 * ws_bytes(n, 4) +
         ws_bytes((size_t)n * kSpillCap, 4);
}
static CandLists carve_b16_lists(Workspace& ws, int64_t n, int lists, int bcap) {
  CandLists L{};
  L.lists = lists; L.cap = bcap; L.slot_ulp = scan_bf16_slot_ulp(bcap); L.spill_cap = kSpillCap;
  L.cnt = ws.take<uint32_t>((size_t)n * lists); L.ids = ws.take<uint32_t>((size_t)n * lists * bcap);
  if (lists > 2) { L.keys = ws.take<float>((size_t)n * lists * bcap); L.margin = ws.take<float>(n); }   // one pair: nothing to prune against
  L.overflow = ws.take<uint32_t>(n); L.spill_cnt = ws.take<uint32_t>(n); L.spill_ids = ws.take<uint32_t>((size_t)n * kSpillCap);
  L.spill_stacks = spill_stacks_for(lists);
  return L;
}

// What the re-rank of a 16-bit scan leaves for the host: the rows it could not certify (fail_rows; their count in word 0 of
// fail_count, word 1: of them, those whose lists overflowed, word 2: those that came up short) and its candidate counters.
struct FlagBlock {
  int32_t* fail_rows = nullptr; uint32_t *fail_count = nullptr, *cand_total = nullptr;
  uint32_t h_fail4[4] = {0, 0, 0, 0};
  std::vector<uint32_t> h_tot;   // read() with totals: the 256 counters, else empty
  static size_t bytes(int64_t n) { return ws_bytes(n, 4) + ws_bytes(4, 4) + ws_bytes(256, 4); }
  void carve(Workspace& ws, int64_t n) { fail_rows = ws.take<int32_t>(n); fail_count = ws.take<uint32_t>(4); cand_total = ws.take<uint32_t>(256); }
  int zero(hipStream_t s) const {
    MMF_HIP(hipMemsetAsync(fail_count, 0, 16, s)); MMF_HIP(hipMemsetAsync(cand_total, 0, 1024, s));
    return MMF_OK;
  }
  int read(bool totals, hipStream_t s) {   // synchronises the stream
    MMF_HIP(hipMemcpyAsync(h_fail4, fail_count, 16, hipMemcpyDeviceToHost, s));
    h_tot.assign(totals ? 256 : 0, 0);
    if (totals) MMF_HIP(hipMemcpyAsync(h_tot.data(), cand_total, 1024, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    return MMF_OK;
  }
};

// The symmetric 16-bit scan (launch_scan_b16_sym) applies to X against itself with equal id offsets, cosine or dot (no
// per-candidate bias), padded dim 512, 15-entry lists, no forced column splits, and an operand image inside the 32-bit tile
// offsets.  MMF_SYMMETRIC (read per call): 0 = never, 1 = whenever it applies, unset = from kSymMinRows rows on — below that
// its first launch (own + antipodal super-block only) leaves compute units idle (profiles/r04_symmetric_ab.txt).
// MMF_SYMMETRIC_G: row blocks per super-block (default: 32, more when that would make more than 32 super-blocks).
// MMF_SYMMETRIC_LIVE (read per call): unset / 1 = the candidate rows' thresholds keep rising while the symmetric launch runs
// and its schedule looks back, 0 = the image frozen after the first launch and the schedule looking ahead;
// for measurements, 2 = live image with the schedule looking ahead, 3 = frozen image with the schedule looking back.
static void symmetric_live_mode(bool* live, bool* forward) {
  const char* e = getenv("MMF_SYMMETRIC_LIVE");
  const int v = e ? atoi(e) : 1;
  *live = (v == 1 || v == 2);
  *forward = (v == 0 || v == 2);
}
// MMF_SYMMETRIC_PHASES (read per call): unset / 2 = the symmetric launch looks back in two phases, the wrap-around pairs behind all
// others (sym_schedule_table), 1 = the single cyclic look-back.  MMF_SYMMETRIC_ANTIPODAL (read per call): 1 = with an even number
// of super-blocks (four or more) the antipodal pairs are multiplied once, in the symmetric launch, 0 = twice, in the first launch;
// unset = 1 with two phases and super-blocks of at least kSymAntipodalMinGroup row blocks (every default G: launch 0 then gives a
// row its threshold from its own super-block alone, and with the 256 columns of a forced G = 1 rows with crowded margin bands drop
// keys they would not have dropped — tests/test_gpu_scan16_adversarial.py flags 3 rows instead of 1), else 0
// (MMF_SYMMETRIC_PHASES=1 alone is the schedule before both; with one phase the
// antipodal pairs fill the wave logs on the benchmark rows in bf16 — profiles/r09_symmetric_schedule.txt — so that pair is for
// measurements only).  Neither applies to the look-ahead table (MMF_SYMMETRIC_LIVE=0 / 2).  Results are the same.
// `schedule_default`: what an unset MMF_SYMMETRIC_PHASES means — 2 for a scan; mmf_debug_symmetric_schedule passes 1, so that
// it shows the tables with phases or without the antipodal range only where it is asked for them.
static constexpr int kSymAntipodalMinGroup = 32;
static void symmetric_schedule_mode(int* phases, bool* antipodal, int G, int schedule_default = 2) {
  const char* e = getenv("MMF_SYMMETRIC_PHASES");
  const int v = e ? atoi(e) : schedule_default;
  *phases = v == 1 ? 1 : (v == 2 ? 2 : schedule_default);
  const char* a = getenv("MMF_SYMMETRIC_ANTIPODAL");
  *antipodal = a ? atoi(a) == 1 : (*phases == 2 && G >= kSymAntipodalMinGroup);
}
// MMF_SYMMETRIC_PRUNE (read per call): unset / 1 = the logs' entries are filed into the rows' received lists only if select could
// still keep them (sym_scatter_kernel), 0 = every entry is filed.  Results are the same; for measurements and tests.
static bool symmetric_prune_mode() {
  const char* e = getenv("MMF_SYMMETRIC_PRUNE");
  return !e || atoi(e) != 0;
}
// MMF_WIDE_SINK (read per call): unset / 1 = the wide scan's crowded lists write to the rows' overflow lists (mmf_scan_b16w.hip,
// DESIGN.md §4.21), 0 = the kernels without them: a crowded row is flagged and rescanned exactly.  Results are the same; for
// measurements and tests.
static bool wide_sink_mode() {
  const char* e = getenv("MMF_WIDE_SINK");
  return !e || atoi(e) != 0;
}
static constexpr int64_t kSymMinRows = 131072;
static bool symmetric_scan_wanted(int64_t n, int dp, int bcap, int metric, int forced_splits, bool same_ids, int* G) {
  if (!same_ids || dp != 512 || bcap != scan_bf16_cap(1, 512) || forced_splits != 0) return false;
  if (metric != MMF_DOT && metric != MMF_COSINE) return false;
  const int64_t nb = (n + 255) / 256;
  if (nb * 256 * 1024 >= (int64_t(1) << 32)) return false;
  const char* e = getenv("MMF_SYMMETRIC");
  const int mode = e ? atoi(e) : -1;
  if (mode == 0 || (mode < 0 && n < kSymMinRows)) return false;
  int g = sym_default_group(nb);
  if (const char* ge = getenv("MMF_SYMMETRIC_G")) { const int v = atoi(ge); if (v >= 1 && v <= 65536) g = v; }
  *G = g;
  return true;
}

// ---- the exact f32 pass -----------------------------------------------------------------------------------------------
// The exact scan (mmf_scan_f32.hip) and the re-rank over groups of rows: all of X in the plain exact call, the rows the
// 16-bit path flagged (gathered), and in the segmented call the whole segments it sends there (slices) and the flagged
// rows of each segment.  Each group is one scan and one re-rank on the stream (one of each per pass of at most 44 entries
// when k + self is larger); one fail-count readback ends the pass.

// Candidate lists, overflow words and fail list of an exact pass, for `rows` rows at a time.
struct ExactLists {
  CandLists L{};                 // cnt / ids: list_words (x cap) words; overflow: one word per row
  int32_t* fail_rows = nullptr; uint32_t* fail_count = nullptr;
  float* floor_key = nullptr; uint32_t* floor_id = nullptr;   // k + self > 44: where each row's previous pass ended
  int64_t rows = 0;
  static size_t bytes(int64_t rows, size_t list_words, int cap, bool floors) {
    return ws_bytes(list_words, 4) + ws_bytes(list_words * cap, 4) + (floors ? 4 : 2) * ws_bytes(rows, 4) + ws_bytes(4, 4);
  }
  void carve(Workspace& ws, int64_t rows_, size_t list_words, int cap, bool floors) {
    rows = rows_;
    L.cnt = ws.take<uint32_t>(list_words); L.ids = ws.take<uint32_t>(list_words * cap); L.overflow = ws.take<uint32_t>(rows);
    fail_rows = ws.take<int32_t>(rows); fail_count = ws.take<uint32_t>(4);
    if (floors) { floor_key = ws.take<float>(rows); floor_id = ws.take<uint32_t>(rows); }
  }
  int zero(hipStream_t s) const {   // fail count and overflow words
    MMF_HIP(hipMemsetAsync(fail_count, 0, 16, s)); MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)rows * 4, s));
    return MMF_OK;
  }
};

struct ExactGroup {
  int64_t row0, rows;   // rows [row0, row0 + rows) of X, or (gathered) entries [row0, row0 + rows) of ExactPass::row_ids
  bool gathered;
  int64_t col0, cols;   // ranked against rows [col0, col0 + cols) of Y
  int k;                // entries per row (the output rows stay r.k wide)
};

struct ExactPass {
  static constexpr int64_t kBatch = 4096;   // gathered rows that have an f32 image at a time
  const Request& r;
  const float *rx, *cy;                     // row scalars of X and Y
  bool same = false;                        // X is Y: one f32 image serves both
  int forced_splits = 0;                    // (set before add())
  const int32_t* row_ids = nullptr;         // device: the rows of X that gathered groups name
  int64_t n_ids = 0;
  uint32_t* cand_total = nullptr;           // optional: the re-rank counts its candidates here
  const float *P = nullptr, *pn = nullptr;  // optional: rank by the exponent of K_h * K_g — positions [n][dp] of the rows of
  int dp = 0; float lambda_g = 0.0f;        //   X and their chains; r.metric MMF_RBF, r.lambda = lambda_h (mmf_simtopk_combined)
  const float *Pc = nullptr, *pnc = nullptr;   // ... and of the rows of Y (mmf_simtopk_combined_xy); null: P / pn, X against itself
  int64_t out_row0 = 0;                     // the outputs' first row is row out_row0 of X (the caller holds a row slice of X's rows)
  // One pass of several for gathered rows (mmf_simtopk_fast_anyk): the output rows are out_stride wide (0: r.k) and
  // already hold out_off0 entries; the rows' floors live in row_floor_key / row_floor_id, indexed by row of X — read before a piece's
  // first scan (floors_in) and left behind its last re-rank (floors_out)
  int out_stride = 0, out_off0 = 0;
  bool floors_in = false, floors_out = false;
  float* row_floor_key = nullptr; uint32_t* row_floor_id = nullptr;
  std::vector<ExactGroup> pieces;           // the groups, gathered ones in pieces of at most kBatch rows
  int64_t rows_total = 0; size_t list_words = 0; bool slices = false;
  int grid = 0;                             // out: scan workgroups (of each piece's last pass)

  ExactPass(const Request& r_, const float* rx_, const float* cy_) : r(r_), rx(rx_), cy(cy_) {}
  int cap() const { return scan_f32_cap(std::min(r.kk, 44)); }
  bool floors() const { return r.kk > 44 || floors_in || floors_out; }
  int splits(const ExactGroup& G) const { return pick_splits((G.rows + 127) / 128, (G.cols + 127) / 128, cap(), forced_splits); }
  void add(ExactGroup G) {
    const int64_t end = G.row0 + G.rows;
    for (; G.row0 < end; G.row0 += G.rows) {
      G.rows = G.gathered ? std::min(kBatch, end - G.row0) : end - G.row0;
      pieces.push_back(G);
      rows_total += G.rows; slices |= !G.gathered;
      list_words = std::max(list_words, (size_t)G.rows * 2 * splits(G));
    }
  }
  // f32 images: all of Y, all of X when a piece is a slice of it (and X is not Y), one batch of gathered rows
  size_t image_bytes() const {
    return ws_bytes(prep_f32_bytes(r.m, r.d), 1) + (slices && !same ? ws_bytes(prep_f32_bytes(r.n, r.d), 1) : 0) +
           (n_ids > 0 ? ws_bytes(prep_f32_bytes(std::min(n_ids, kBatch), r.d), 1) : 0);
  }
  size_t list_bytes() const { return ExactLists::bytes(rows_total, list_words, cap(), floors()); }

  int read_fails(const ExactLists& B, std::vector<uint32_t>* h_tot) const {
    uint32_t h_fail = 0;
    MMF_HIP(hipMemcpyAsync(&h_fail, B.fail_count, 4, hipMemcpyDeviceToHost, r.call.s));
    if (h_tot) MMF_HIP(hipMemcpyAsync(h_tot->data(), cand_total, 1024, hipMemcpyDeviceToHost, r.call.s));
    MMF_HIP(hipStreamSynchronize(r.call.s));
    if (h_fail != 0) { set_error("%s: %u rows failed in the exact scan (internal invariant)", r.call.who, h_fail); return MMF_E_INTERNAL; }
    return MMF_OK;
  }

  // Images from ws; lists from B (zeroed by the caller), which holds B.rows rows: when the next piece does not fit, the
  // fail count is read back and B starts over.  t: the plain exact call's timers (prep, started by the caller; scan; re-rank), else null.
  // h_tot: the candidate counters (cand_total), read back with the fail count.
  int run(Workspace& ws, const ExactLists& B, EventTimer* t = nullptr, std::vector<uint32_t>* h_tot = nullptr) {
    const hipStream_t s = r.call.s;
    const int64_t dpad = prep_f32_dim(r.d);
    const size_t row_bytes = (size_t)r.d * dtype_size(r.dtype);
    auto image = [&](int64_t rows) { return reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(rows, r.d))); };
    float* Yp = image(r.m);
    float* Xp = same ? Yp : (slices ? image(r.n) : nullptr);
    float* Xe = n_ids > 0 ? image(std::min(n_ids, kBatch)) : nullptr;
    MMF_TRY(launch_prep_f32(r.Y, r.m, r.d, r.dtype, nullptr, Yp, s));
    if (Xp && Xp != Yp) MMF_TRY(launch_prep_f32(r.X, r.n, r.d, r.dtype, nullptr, Xp, s));
    const int self1 = r.exclude_self ? 1 : 0, k_pass_max = 44 - self1;   // entries one pass can emit
    const bool one_pass = r.k <= k_pass_max;   // timers: scan and re-rank apart for one pass, the whole loop as "scan" otherwise
    if (t) { MMF_TRY(t[0].stop(s)); MMF_TRY(t[1].start(r.profile, s)); }
    int64_t batch0 = -1, used = 0;   // first entry of row_ids in Xe; rows of B in use
    for (const ExactGroup& G : pieces) {
      if (used + G.rows > B.rows) { MMF_TRY(read_fails(B, nullptr)); MMF_TRY(B.zero(s)); used = 0; }
      if (G.gathered && (batch0 < 0 || G.row0 + G.rows > batch0 + kBatch)) {   // next batch of gathered rows
        batch0 = G.row0;
        MMF_TRY(launch_prep_f32(r.X, std::min(kBatch, n_ids - batch0), r.d, r.dtype, row_ids + batch0, Xe, s));
      }
      const int64_t r0 = G.gathered ? 0 : G.row0;   // a slice: X, its scalars, its image and the outputs from row r0 on
      CandLists L = B.L;
      L.lists = 2 * splits(G); L.cap = scan_f32_cap(std::min(G.k + self1, 44)); L.overflow = B.L.overflow + used;
      ScanProblem sp{};
      sp.X = static_cast<const char*>(r.X) + r0 * row_bytes; sp.n = G.gathered ? r.n : G.rows;
      sp.Y = static_cast<const char*>(r.Y) + G.col0 * row_bytes; sp.m = G.cols;
      sp.d = r.d; sp.dtype = r.dtype; sp.metric = r.metric; sp.lambda = r.lambda;
      sp.Xp = G.gathered ? Xe + (G.row0 - batch0) * dpad : Xp + r0 * dpad; sp.Yp = Yp + G.col0 * dpad;
      sp.rx = rx + r0; sp.cy = cy + G.col0; sp.row_ids = G.gathered ? row_ids + G.row0 : nullptr; sp.n_rows = G.rows;
      sp.col_splits = L.lists / 2;
      SelectProblem q = r.select();   // this piece of it (exact lists have no overflow lists: nothing for a second select launch)
      q.X = sp.X; q.n = sp.n; q.Y = sp.Y; q.m = sp.m; q.row_offset += r0; q.col_offset += G.col0;
      q.rx = sp.rx; q.cy = sp.cy; q.row_ids = sp.row_ids; q.n_rows = G.rows;
      q.out_stride = out_stride > 0 ? out_stride : r.k;
      q.out_idx += (r0 - out_row0) * q.out_stride; q.out_val += (r0 - out_row0) * q.out_stride;
      q.fail_rows = B.fail_rows; q.fail_count = B.fail_count; q.cand_total = cand_total;
      if (P) {
        sp.Pq = q.Pq = P + r0 * dp; sp.Pc = q.Pc = (Pc ? Pc : P) + G.col0 * dp;
        sp.pnq = q.pnq = pn + r0; sp.pnc = q.pnc = (pnc ? pnc : pn) + G.col0;
        sp.dp = q.dp = dp; sp.lambda_g = q.lambda_g = lambda_g;
      }
      // k + self beyond 44: several passes, each offering only what ranks after the previous pass's last entry
      // (scikit-learn's n_neighbors is uncapped, preprocess_hypergraph.py:379)
      int g = 0;
      const bool row_floors = G.gathered && (floors_in || floors_out);
      if (row_floors && floors_in) MMF_TRY(launch_floor_move(row_ids + G.row0, G.rows, row_floor_key, row_floor_id, B.floor_key, B.floor_id, false, s));
      for (int done = 0; done < G.k; done += k_pass_max) {
        const int kp = std::min(G.k - done, k_pass_max);
        const bool more = done + kp < G.k || (row_floors && floors_out);
        sp.kk = kp + self1;
        if (done > 0 || (row_floors && floors_in)) { sp.floor_key = B.floor_key; sp.floor_id = B.floor_id; }
        MMF_TRY(launch_scan_f32(sp, L, s, &g));
        if (t && one_pass) { MMF_TRY(t[1].stop(s)); MMF_TRY(t[2].start(r.profile, s)); }
        q.k = kp; q.out_off = out_off0 + done;
        q.floor_key_out = more ? B.floor_key : nullptr; q.floor_id_out = more ? B.floor_id : nullptr;
        // (the combined key over gathered rows: the passes of mmf_simtopk_combined_fast_anyk)
        MMF_TRY(P ? (q.row_ids ? launch_rerank_combined_ext(q, L, s) : launch_rerank_combined(q, L, s)) : launch_select(q, L, s));
      }
      if (row_floors && floors_out) MMF_TRY(launch_floor_move(row_ids + G.row0, G.rows, row_floor_key, row_floor_id, B.floor_key, B.floor_id, true, s));
      grid += g;
      used += G.rows;
    }
    if (t && one_pass) MMF_TRY(t[2].stop(s));
    if (t && !one_pass) { MMF_TRY(t[1].stop(s)); MMF_TRY(t[2].start(r.profile, s)); MMF_TRY(t[2].stop(s)); }
    return read_fails(B, h_tot);
  }
};

// Everything of the fast path after the 16-bit operands exist: candidate lists, scan, (optional event
// wait), exact re-rank, exact rescan of flagged rows, stats.  Shared by mmf_simtopk_ex,
// mmf_simtopk_prepared and mmf_simtopk_panels.
struct FastOperands {
  HalfImage q, c;        // the 16-bit images of the queries and of the candidates (c: Z / cb / maxima are read)
  const float* rx; const float* cy;
  int64_t m_pad_tiles;   // candidate rows covered by tiles (multiple of 256)
  int dp; bool f16;
  // paneled scan (mmf_simtopk_panels): the candidate operands come as n_panels separate blocks, each scanned by
  // its own launch once its event has fired; c.Z / c.cb / m_pad_tiles above are then unused
  const mmf_panel* panels = nullptr; int n_panels = 0;
  // q holds the queries in scan order: position p is row perm[p] (mmf_order.hip); null: row order
  const int32_t* perm = nullptr;
};

struct FastTail {
  int64_t n, m; int kk, cap, bcap, splits, lists, fb_splits; int64_t FB;
  CandLists L;
  ExactLists XL;   // the exact rescan of flagged rows, FB rows at a time
  FlagBlock flags;
  char* scan_scratch = nullptr;
  char* order_scratch = nullptr;
  // query order of the scan (mmf_order.hip): near-duplicate rows next to each other.  Tried when forced, or (auto) at sizes where
  // the scan dominates; applied when the rows have near-duplicates among themselves (decided from the data, one host sync).
  int order_mode = MMF_QUERY_ORDER_OFF; bool order_try = false;
  char* qo_scratch = nullptr; uint16_t* qo_Z = nullptr; float *qo_zn = nullptr, *qo_rn = nullptr, *qo_un = nullptr;
  int64_t n_pad_q() const { return (n + 255) / 256 * 256; }
  int set_query_order(int mode) {   // before bytes() / carve()
    if (mode < MMF_QUERY_ORDER_AUTO || mode > MMF_QUERY_ORDER_ON) { set_error("simtopk: bad query_order %d", mode); return MMF_E_INVALID; }
    order_mode = mode;
    order_try = !wide && (mode == MMF_QUERY_ORDER_ON || (mode == MMF_QUERY_ORDER_AUTO && n >= 32768 && m >= 32768));
    return MMF_OK;
  }

  // Symmetric scan (launch_scan_b16_sym): tried when the call qualifies (set_symmetric), taken unless the query
  // order is applied (scan positions are then not rows, and near-duplicate bands would flood the rows' received lists).  The
  // buffers hold whichever path runs: the lists are carved for the larger list count and used through view().
  bool sym_try = false; int sym_G = 32; int lists_alloc = 0;
  SymBuffers sym;
  WsKept sym_kept; WsKept* sym_keep = nullptr;   // the work tables the workspace came with, and where to file the ones it leaves with
  uint32_t* sym_cnt = nullptr; uint2* sym_ent = nullptr;
  int64_t sym_grid() const { return sym_schedule_grid((n + 255) / 256, sym_G); }
  void set_symmetric(int G) {   // before bytes() / carve()
    sym_try = true; sym_G = G;
    if (lists_alloc < 2 * kSymListPairs) lists_alloc = 2 * kSymListPairs;
  }
  CandLists view(bool symmetric) const {
    CandLists v = L;
    v.lists = symmetric ? 2 * kSymListPairs : lists;
    if (v.lists <= 2) { v.keys = nullptr; v.margin = nullptr; }
    v.spill_stacks = spill_stacks_for(v.lists);
    if (symmetric) { v.sym_cnt = sym_cnt; v.sym_ent = sym_ent; v.sym_cap = kSymCap; }
    return v;
  }

  int dp, panels;
  bool wide = false;   // dp > 1024: launch_scan_b16w takes the slot of launch_scan_b16 (no query order, symmetric scan or panels);
                       // it writes the same overflow lists (L.spill_*) unless MMF_WIDE_SINK=0
  int panel_splits[16]; int max_splits = 1;
  int64_t n_seed;
  int32_t* seed = nullptr;
  int64_t seed_stripes() const { return wide ? 3 : 2; }   // thresholds, dropped keys; wide: the overflow lists' best keys (ScanB16Panel::sunk)
  // a handful of flagged rows skips the matrix-core rescan: all their keys, then a block-wide top-k
  static constexpr int64_t kRowsExactMax = 48;
  int64_t rows_exact_cap = 0;
  float* row_keys = nullptr;
  // The first pass of mmf_simtopk_fast_anyk (set before bytes() / carve()): the output rows are out_stride wide
  // (0: r.k) and every row — the flagged ones too, which then all take the matrix-core rescan — leaves the key and local id of its
  // last entry in floor_key_out / floor_id_out [n]
  bool leave_floors = false; int out_stride = 0;
  float* floor_key_out = nullptr; uint32_t* floor_id_out = nullptr;
  int64_t failed_rows = 0;   // out: rows the last run() sent to the exact rescan
  // m_panel_min: columns of the smallest panel (== m_ when the scan is one launch); `splits` is per launch
  FastTail(int64_t n_, int64_t m_, int kk_, int forced_splits, int dp_, int panels_ = 1, int64_t m_panel_min = -1,
           int64_t m_panel_max = -1)
      : n(n_), m(m_), kk(kk_), cap(scan_f32_cap(kk_)), dp(dp_), panels(panels_) {
    wide = dp > 1024;   // the wide kernel's sizes: its list capacity, 128 queries per workgroup, column tiles of 128, no id scratch
    bcap = wide ? scan_b16w_cap(kk) : scan_bf16_cap(kk, dp);
    const int qt = wide ? scan_b16w_queries_per_block() : scan_b16_queries_per_block(dp);
    if (m_panel_min < 0) m_panel_min = m;
    const int64_t row_blocks = (n + qt - 1) / qt;
    const int64_t col_tiles = wide ? (m_panel_min + scan_b16w_col_tile() - 1) / scan_b16w_col_tile() : ((m_panel_min + 255) / 256 * 256) / 32;
    n_seed = row_blocks * qt;
    splits = 1;
    if (forced_splits > 0) { while (splits < forced_splits) splits <<= 1; }
    else { while (row_blocks * splits < 256 && splits < 32) splits <<= 1; }
    while (splits > 1 && (splits > col_tiles || 2 * splits * panels * bcap > 1024 - kSpillCap)) splits >>= 1;
    // the tile DMA addresses a workgroup's column range with 32-bit offsets: a range stays under 4 GiB of 16-bit operands
    // (N = 4 M rows at d = 1024 is 8 GiB: at least four splits), whatever the caller forced
    {
      const int64_t m_big = (m_panel_max > 0 ? m_panel_max : m);
      const int64_t range_bytes = ((m_big + 255) / 256 * 256) * (int64_t)dp * 2;
      while ((range_bytes + splits - 1) / splits >= (int64_t(1) << 32) && 2 * (2 * splits) * panels * bcap <= 1024 - kSpillCap) splits <<= 1;
    }
    // The first half of the panels runs while the rest of the exchange is still on the wire and its kernel
    // holds compute units.  MMF_PANEL_FRONT_FACTOR = 2 or 4 gives those launches that many times the workgroups
    // (shorter ones), which shortens the tail the late-joining units leave — measured with a stand-in kernel
    // (scripts/overlap_sim.py) it trades 0.6 ms without contention for 0.9 ms with it, so the default stays 1.
    int front = 1;
    if (const char* e = getenv("MMF_PANEL_FRONT_FACTOR")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) front = v; }
    int total_splits = 0;
    for (int p = 0; p < panels && p < 16; ++p) {
      int sp = splits * ((panels > 1 && p < panels / 2) ? front : 1);
      while (sp > 1 && sp > col_tiles) sp >>= 1;
      panel_splits[p] = sp;
      total_splits += sp;
    }
    if (2 * total_splits * bcap > 1024 - kSpillCap) { // too many lists for the select kernel: uniform
      total_splits = splits * panels;
      for (int p = 0; p < panels && p < 16; ++p) panel_splits[p] = splits;
    }
    max_splits = 1;
    for (int p = 0; p < panels && p < 16; ++p) if (panel_splits[p] > max_splits) max_splits = panel_splits[p];
    lists = 2 * total_splits;
    lists_alloc = lists;
    rows_exact_cap = (int64_t(64) << 20) / (4 * (m > 0 ? m : 1));
    if (rows_exact_cap > kRowsExactMax) rows_exact_cap = kRowsExactMax;
    if (rows_exact_cap < 1) rows_exact_cap = 1;
    FB = n < ExactPass::kBatch ? n : ExactPass::kBatch;   // exact rescans are done in batches of at most FB rows
    fb_splits = pick_splits((FB + 127) / 128, (m + 127) / 128, cap, 0);
  }
  size_t scan_scratch_bytes() const {
    if (wide) return 256;
    const size_t a = scan_b16_scratch_bytes(n, max_splits, dp, bcap), b = sym_try ? scan_b16_sym_scratch_bytes(n, sym_G) : 0;
    return a > b ? a : b;
  }
  size_t bytes() const {
    return b16_lists_bytes(n, lists_alloc, bcap) + FlagBlock::bytes(n) +
           ExactLists::bytes(FB, (size_t)FB * 2 * fb_splits, cap, leave_floors) + ws_bytes(scan_scratch_bytes(), 1) +
           (sym_try ? ws_bytes(n, 4) + ws_bytes((size_t)n * kSymCap, 8) + SymBuffers::bytes(n_pad_q(), sym_grid()) : 0) +
           ws_bytes(seed_stripes() * n_seed, 4) + ws_bytes((size_t)rows_exact_cap * m, 4) + ws_bytes(select_order_bytes(n), 1) +
           (order_try ? ws_bytes(query_order_bytes(n), 1) + ws_bytes((size_t)n_pad_q() * dp, 2) + 3 * ws_bytes(n_pad_q(), 4) : 0);
  }
  void carve(Workspace& ws) {
    L = carve_b16_lists(ws, n, lists_alloc, bcap);
    if (sym_try) {
      sym_cnt = ws.take<uint32_t>(n); sym_ent = ws.take<uint2>((size_t)n * kSymCap);
      sym.carve(ws, n_pad_q(), sym_grid());
      sym_kept = ws.kept; sym_keep = ws.keep;
    }
    flags.carve(ws, n);
    XL.carve(ws, FB, (size_t)FB * 2 * fb_splits, cap, leave_floors);
    scan_scratch = ws.take<char>(scan_scratch_bytes());
    seed = ws.take<int32_t>(seed_stripes() * n_seed);
    row_keys = ws.take<float>((size_t)rows_exact_cap * m);
    order_scratch = ws.take<char>(select_order_bytes(n));
    if (order_try) {
      qo_scratch = ws.take<char>(query_order_bytes(n));
      qo_Z = ws.take<uint16_t>((size_t)n_pad_q() * dp);
      qo_zn = ws.take<float>(n_pad_q()); qo_rn = ws.take<float>(n_pad_q()); qo_un = ws.take<float>(n_pad_q());
    }
  }
  int run(const Request& r, const FastOperands& fo_in, void* select_wait_event) {
    const hipStream_t s = r.call.s;
    const bool profile = r.profile;
    FastOperands fo = fo_in;
    query_order_forget();
    EventTimer t_order;
    int64_t near_rows = -1;
    if (order_try) {
      MMF_TRY(t_order.start(profile, s));
      MMF_TRY(launch_query_order_probe(fo.q.Z, fo.q.zn, n, fo.dp, fo.f16, qo_scratch, &near_rows, s));
      if (order_mode == MMF_QUERY_ORDER_ON || near_rows >= 8 * (int64_t)query_order_pivots()) {
        MMF_TRY(launch_query_order_apply(fo.q.Z, fo.q.zn, fo.q.rn, fo.q.un, n, n_pad_q(), fo.dp, fo.f16, qo_scratch, qo_Z, qo_zn, qo_rn, qo_un, &fo.perm, s));
        fo.q.Z = qo_Z; fo.q.zn = qo_zn; fo.q.rn = qo_rn; fo.q.un = qo_un;
      }
      MMF_TRY(t_order.stop(s));
    }
    const bool symmetric = sym_try && !fo.perm && fo.n_panels == 0;
    const CandLists L = view(symmetric);   // (shadows the member: the lists as this call's path uses them)
    MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
    MMF_TRY(flags.zero(s));
    EventTimer t_scan, t_sel, t_fb;
    EventTimer t_panel[16];
    int grid = 0;
    MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)n_seed * 4 * seed_stripes(), s));   // kSeedNone, thresholds and dropped keys
    MMF_HIP(hipMemsetAsync(L.spill_cnt, 0, (size_t)n * 4, s));
    MMF_TRY(t_scan.start(profile, s));
    ScanB16Panel pn;
    pn.seed = seed; pn.seed_stride = n_seed;
    pn.share = (splits > 1 || fo.n_panels > 1) ? 1 : 0;
    ScanB16Problem sp(fo.q, fo.c, n, m, fo.m_pad_tiles, fo.dp, r.d, fo.f16, r.metric, kk);
    if (symmetric) {
      bool live, forward;
      symmetric_live_mode(&live, &forward);
      int phases; bool antipodal;
      symmetric_schedule_mode(&phases, &antipodal, sym_G);
      const WsKept tables{sym.sched, (n + 255) / 256, sym_G, forward ? 1 : 0, phases, antipodal ? 1 : 0};
      MMF_TRY(launch_scan_b16_sym(sp, SymLaunch{sym_G, live, forward, symmetric_prune_mode(), !(sym_kept == tables), phases, antipodal}, L,
                                  scan_scratch, sym, pn, s, &grid));
      if (sym_keep) *sym_keep = tables;
    } else if (fo.n_panels == 0) {
      if (wide) {
        CandLists Lw = L;   // without the sink the overflow lists stay zeroed: select reads them as empty
        if (!wide_sink_mode()) { Lw.spill_cnt = nullptr; Lw.spill_ids = nullptr; Lw.spill_cap = 0; Lw.spill_stacks = 0; }
        pn.sunk = seed + 2 * n_seed;
        MMF_TRY(launch_scan_b16w(sp, splits, Lw, pn, s, &grid));
      }
      else MMF_TRY(launch_scan_b16(sp, splits, L, scan_scratch, pn, s, &grid));
    } else {
      // one launch per panel, each behind its own arrival event; the launches share the lists (disjoint
      // slots), the id scratch (they run one after the other) and the per-query thresholds
      int list_base = 0;
      for (int p = 0; p < fo.n_panels; ++p) {
        const mmf_panel& P = fo.panels[p];
        if (P.ready_event) MMF_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(P.ready_event), 0));
        MMF_TRY(t_panel[p].start(profile, s));       // behind the wait: launch-only time of this panel
        pn.list_base = list_base;
        list_base += 2 * panel_splits[p];
        pn.seg_len = (uint32_t)P.seg_len; pn.seg_stride = (uint32_t)P.seg_stride; pn.id_off = (uint32_t)P.id_base;
        sp.ZC = P.Z; sp.cb = P.cb; sp.m = P.m; sp.m_pad = P.m_pad;
        MMF_TRY(launch_scan_b16(sp, panel_splits[p], L, scan_scratch, pn, s, &grid));
        MMF_TRY(t_panel[p].stop(s));
      }
    }
    MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
    if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {   // test hook: send the first rows down the exact paths
      const int64_t f = atoll(e);
      if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < n ? f : n) * 4, s));
    }
    MMF_TRY(t_scan.stop(s));
    if (symmetric && getenv("MMF_SYMMETRIC_DEBUG")) {   // diagnosis: what the candidate direction carried
      MMF_HIP(hipStreamSynchronize(s));
      // hr: the hit records in each wave's log; hl: the values of those records that pass the thresholds recorded with them — the
      // "logged entries", counted by sym_scatter_kernel before its pruning test
      // hr continues with the waves' coarse visits (wave-tiles whose group test passed) and their wave-tiles with a hit
      std::vector<uint32_t> hc((size_t)n), hl((size_t)sym_grid() * 8), hr((size_t)sym_grid() * 24);
      uint32_t none = 0;
      MMF_HIP(hipMemcpy(hc.data(), sym_cnt, hc.size() * 4, hipMemcpyDeviceToHost));
      MMF_HIP(hipMemcpy(hl.data(), sym.val_cnt, hl.size() * 4, hipMemcpyDeviceToHost));
      MMF_HIP(hipMemcpy(hr.data(), sym.log_cnt, hr.size() * 4, hipMemcpyDeviceToHost));
      MMF_HIP(hipMemcpy(&none, sym.none_cnt, 4, hipMemcpyDeviceToHost));
      unsigned long long tot = 0, logged = 0, records = 0, coarse = 0, hit_tiles = 0; uint32_t mx = 0, lmx = 0;
      for (uint32_t v : hc) { tot += v; if (v > mx) mx = v; }
      for (uint32_t v : hl) logged += v;
      const size_t waves = hl.size();
      for (size_t i = 0; i < waves; ++i) { records += hr[i]; if (hr[i] > lmx) lmx = hr[i]; coarse += hr[waves + i]; hit_tiles += hr[2 * waves + i]; }
      bool live, forward;
      symmetric_live_mode(&live, &forward);
      int phases; bool antipodal;
      symmetric_schedule_mode(&phases, &antipodal, sym_G);
      // logged entries by the phase of the workgroup that logged them (sym_schedule_grid: phase B's block ids follow phase A's)
      const size_t first_b = (size_t)sym_schedule_phase_b_begin((n + 255) / 256, sym_G) * 8;
      unsigned long long logged_b = 0;
      for (size_t i = first_b; i < hl.size(); ++i) logged_b += hl[i];
      fprintf(stderr, "[mmf symmetric] G %d grid %lld %s %s: rows without a threshold %u, received entries %llu (%.1f per row, largest %u of %d), fullest wave log %u of %d, logged entries %llu (%.1f per row, filing %s), records %llu, phases %d antipodal %d, logged by phase B %llu (%.1f per row), coarse visits %llu, hit wave-tiles %llu\n",
              sym_G, (long long)sym_grid(), live ? "live" : "frozen", forward ? "ahead" : "back", none, tot, (double)tot / (double)n, mx,
              kSymCap, lmx, scan_b16_sym_log_cap(), logged, (double)logged / (double)n, symmetric_prune_mode() ? "pruned" : "complete", records,
              forward ? 1 : phases, (antipodal && !forward) ? 1 : 0, logged_b, (double)logged_b / (double)n, coarse, hit_tiles);
    }
    // the f32 rows are first touched here: a caller that is still receiving them (overlapped
    // all-gather) hands in the event that marks their arrival
    if (select_wait_event) MMF_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(select_wait_event), 0));

    SelectProblem q = r.select();
    q.rx = fo.rx; q.cy = fo.cy; q.perm = fo.perm;
    q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = r.stats ? flags.cand_total : nullptr;
    q.two_pass = true;
    q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
    q.out_stride = out_stride;
    if (leave_floors) { q.floor_key_out = floor_key_out; q.floor_id_out = floor_id_out; }
    MMF_TRY(t_sel.start(profile, s));
    MMF_TRY(launch_select(q, L, s));
    MMF_TRY(t_sel.stop(s));

    MMF_TRY(flags.read(r.stats != nullptr, s));
    const uint32_t* h_fail4 = flags.h_fail4;
    const uint32_t h_fail = h_fail4[0];
    failed_rows = h_fail;
    if (h_fail > 0 && getenv("MMF_DEBUG_PRINT_FLAGGED")) {   // diagnosis: which rows, and the threshold / dropped key that flagged them
      const uint32_t nshow = h_fail < 8 ? h_fail : 8;
      int32_t rows[8];
      MMF_HIP(hipMemcpy(rows, flags.fail_rows, nshow * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < nshow; ++i) {
        int32_t enc[2] = {0, 0};
        MMF_HIP(hipMemcpy(&enc[0], seed + rows[i], 4, hipMemcpyDeviceToHost));
        MMF_HIP(hipMemcpy(&enc[1], seed + n_seed + rows[i], 4, hipMemcpyDeviceToHost));
        auto dec = [](int32_t o) { int32_t b = o >= 0 ? o : (o ^ 0x7fffffff); float f; memcpy(&f, &b, 4); return f; };
        fprintf(stderr, "[mmf flagged] row %d: best threshold %.9g (enc %d)  best dropped key %.9g (enc %d)  overflow %u short %u\n",
                rows[i], dec(enc[0]), enc[0], dec(enc[1]), enc[1], h_fail4[1], h_fail4[2]);
      }
    }

    MMF_TRY(t_fb.start(profile && h_fail > 0, s));
    if (h_fail > 0 && (int64_t)h_fail <= kRowsExactMax && !leave_floors) {
      for (int64_t off = 0; off < (int64_t)h_fail; off += rows_exact_cap) {
        SelectProblem fq = q;
        fq.perm = nullptr;
        fq.row_ids = flags.fail_rows + off;
        fq.n_rows = ((int64_t)h_fail - off < rows_exact_cap) ? ((int64_t)h_fail - off) : rows_exact_cap;
        MMF_TRY(launch_rows_exact(fq, row_keys, s));
      }
    } else if (h_fail > 0) {   // the exact pass over the flagged rows; its f32 images in the second workspace slot
      ExactPass ex(r, fo.rx, fo.cy);
      ex.row_ids = flags.fail_rows; ex.n_ids = h_fail; ex.forced_splits = fb_splits;
      ex.out_stride = out_stride;
      if (leave_floors) { ex.floors_out = true; ex.row_floor_key = floor_key_out; ex.row_floor_id = floor_id_out; }
      ex.add(ExactGroup{0, (int64_t)h_fail, true, 0, m, r.k});
      Workspace aux;
      MMF_TRY(r.call.workspace(ex.image_bytes(), &aux, 1));
      MMF_TRY(XL.zero(s));
      MMF_TRY(ex.run(aux, XL));
    }
    MMF_TRY(t_fb.stop(s));
    fill_stats(r.stats, r.precision, symmetric ? 1 : splits, grid, 0.f, t_scan.ms(), t_sel.ms(), t_fb.ms(), h_fail, h_fail4[1], h_fail4[2], flags.h_tot,
               near_rows);
    if (r.stats) {
      if (profile && fo.n_panels > 0) {     // what the scan stream spent waiting for panels to arrive
        float launches = 0.f;
        for (int p = 0; p < fo.n_panels; ++p) launches += t_panel[p].ms();
        const float w = r.stats->scan_ms - launches;
        r.stats->scan_wait_ms = w > 0.f ? w : 0.f;
      }
      r.stats->order_ms = t_order.ms();
      r.stats->query_order = fo.perm ? 1 : 0;
    }
    return MMF_OK;
  }
};

// mmf_simtopk_combined (include/mmf_hg_topk.h; entry and host checks in mmf_topk.hip): every segment is a slice of F against
// itself through the exact pass, two launches per segment on the stream (DESIGN.md §4.7 "Exact rows", §4.14), one fail-count
// readback at the end.  A segment with fewer than k admissible columns is ranked for what it has; the re-rank pads its rows.
int run_simtopk_combined(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                         float lambda_g, int k, int exclude_self, const int64_t* ptr, int64_t n_seg, int64_t* out_idx, float* out_val,
                         const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  const int self1 = exclude_self ? 1 : 0;
  r.kk = k + self1;
  r.precision = MMF_PREC_EXACT;
  if (stats) memset(stats, 0, sizeof(*stats));
  MMF_TRY(r.call.begin());
  const hipStream_t s = r.call.s;
  ExactPass ex(r, nullptr, nullptr);
  ex.same = true;
  ex.forced_splits = opts ? opts->col_splits : 0;
  ex.P = P; ex.dp = (int)dp; ex.lambda_g = lambda_g;
  std::vector<int64_t> bare;   // segments without an admissible column (one row, self excluded): -1 / -inf
  for (int64_t g = 0; g < n_seg; ++g) {
    const int64_t ng = ptr[g + 1] - ptr[g];
    if (ng == 0) continue;
    const int64_t ks = std::min<int64_t>(k, ng - self1);
    if (ks > 0) ex.add(ExactGroup{ptr[g], ng, false, ptr[g], ng, (int)ks});
    else bare.push_back(g);
  }
  const size_t need = 2 * ws_bytes(n, 4) + ws_bytes(256, 4) + (ex.pieces.empty() ? 0 : ex.image_bytes() + ex.list_bytes());
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(n);
  float* pn = ws.take<float>(n);
  uint32_t* cand_total = ws.take<uint32_t>(256);
  ex.rx = nf; ex.cy = nf; ex.pn = pn;
  ex.cand_total = stats ? cand_total : nullptr;
  for (int64_t g : bare) {
    const int64_t ng = ptr[g + 1] - ptr[g];
    MMF_HIP(hipMemsetAsync(out_idx + ptr[g] * k, 0xff, (size_t)ng * k * 8, s));
    MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_val + ptr[g] * k), (int)0xff800000u, (size_t)ng * k, s));
  }
  if (ex.pieces.empty()) return MMF_OK;
  ExactLists B;
  B.carve(ws, ex.rows_total, ex.list_words, ex.cap(), ex.floors());   // floors: the passes of the any-k entries (k + self > 44)
  MMF_TRY(B.zero(s));
  MMF_HIP(hipMemsetAsync(cand_total, 0, 1024, s));

  // timers: prep (row scalars, f32 image), scan, re-rank for one graph; with several segments the launches alternate, and
  // "scan" is the image and every segment's two launches
  const bool one = ex.pieces.size() == 1;
  EventTimer t[3];
  MMF_TRY(t[0].start(r.profile, s));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_row_scalars(P, n, dp, MMF_F32, MMF_RBF, pn, nullptr, s));
  if (!one) { MMF_TRY(t[0].stop(s)); MMF_TRY(t[1].start(r.profile, s)); }
  std::vector<uint32_t> h_tot(stats ? 256 : 0);
  MMF_TRY(ex.run(ws, B, one ? t : nullptr, stats ? &h_tot : nullptr));
  if (!one) MMF_TRY(t[1].stop(s));
  fill_stats(stats, MMF_PREC_EXACT, ex.splits(ex.pieces[0]), ex.grid, t[0].ms(), t[1].ms(), t[2].ms(), 0.f, 0, 0, 0, h_tot);
  return MMF_OK;
}

// What MMF_PREC_AUTO does in mmf_simtopk_combined_fast: the 16-bit scan only for the (d, k) range where the whole call beat the
// exact one by more than three times the exact arm's spread at every measured N (DESIGN.md §4.17,
// profiles/simtopk_combined_fast_timing.txt): k = 5 (16-entry lists), d = 512 at N = 16384 / 65536 / 262144 — 2.87x / 3.36x /
// 3.83x, the difference 23 / 92 / 542 times that spread — and d = 1536 at N = 65536 — 3.84x, 117 times.  Between the two measured
// dims the epilogue's share only falls; outside 512 <= d <= 1536, or with the 32-entry lists of k + self > 11, nothing is
// measured and AUTO stays exact (precision = MMF_PREC_FAST is served everywhere).
static bool combined_fast_auto(int64_t d, int kk) { return d >= 512 && d <= 1536 && kk <= 11; }

// mmf_simtopk_combined_fast (include/mmf_hg_topk16.h; entry and host checks in mmf_scan_b16c.hip), one graph, DESIGN.md §4.17:
// row scalars of F and P, the 16-bit image of F, the scan of the combined key (launch_scan_b16c), the audit, the re-rank of the
// combined key over the 16-bit lists, one readback.  The rows the audit or the re-rank flagged are answered by the exact pass
// over slices of F against itself: their 128-row blocks, adjacent blocks merged into runs — all of F when more than a quarter
// of the blocks hold a flagged row.  The values are the same bits by contract, so overwriting a block's clean rows changes nothing.
int run_simtopk_combined_fast(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                              float lambda_g, int k, int exclude_self, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                              mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const int self1 = exclude_self ? 1 : 0;
  int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec == MMF_PREC_AUTO) prec = combined_fast_auto(d, k + self1) ? MMF_PREC_FAST : MMF_PREC_EXACT;
  const int ks = (int)std::min<int64_t>(k, n - self1);   // entries a row can have; the re-rank pads the rest with -1 / -inf
  if (prec == MMF_PREC_EXACT || ks <= 0) {                // (one row, self excluded: nothing to scan)
    const int64_t one_graph[2] = {0, n};
    return run_simtopk_combined(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, one_graph, 1, out_idx, out_val, opts, stats,
                                device_id, hip_stream);
  }
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.kk = ks + self1;
  r.precision = prec;
  if (stats) memset(stats, 0, sizeof(*stats));
  MMF_TRY(r.call.begin());
  const hipStream_t s = r.call.s;
  const bool f16 = prec == MMF_PREC_FAST;
  const int dpf = scan_b16c_dp(d), bcap = scan_b16c_cap(r.kk);
  const int64_t n_pad = (n + 255) / 256 * 256, row_blocks = (n + 127) / 128, n_seed = row_blocks * 128;
  // column splits: a power of two; enough workgroups for the device, no more ranges than column tiles, and no more lists than
  // the re-rank gathers (launch_rerank_combined: lists x cap <= 1024)
  int splits = 1;
  const int forced = opts ? opts->col_splits : 0;
  if (forced > 0) { while (splits < forced && splits < 32) splits <<= 1; }
  else { while (row_blocks * splits < 256 && splits < 32) splits <<= 1; }
  while (splits > 1 && (splits > row_blocks || 2 * splits * bcap > 1024)) splits >>= 1;
  const int lists = 2 * splits;
  constexpr int64_t kFailPeek = 1024;   // flagged row ids that come back with the fail count
  const int64_t peek = std::min(n, kFailPeek);

  const size_t need = 2 * ws_bytes(n, 4) + ws_bytes(8, 4) + HalfImage::bytes(n_pad, dpf) + b16_lists_bytes(n, lists, bcap) +
                      FlagBlock::bytes(n) + ws_bytes(2 * n_seed, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(n);
  float* pn = ws.take<float>(n);
  uint32_t* maxw = ws.take<uint32_t>(8);   // word 0: largest chain(f, f), word 4: largest chain(p, p)
  HalfImage C;
  C.carve(ws, n_pad, dpf);
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  FlagBlock flags;
  flags.carve(ws, n);
  int32_t* seed = ws.take<int32_t>(2 * n_seed);
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(maxw, 0, 32, s));
  MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
  MMF_TRY(flags.zero(s));
  MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)n_seed * 8, s));   // kSeedNone, thresholds and dropped keys

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(r.profile, s));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, maxw, s));
  MMF_TRY(launch_row_scalars(P, n, dp, MMF_F32, MMF_RBF, pn, maxw + 4, s));
  MMF_TRY(launch_prep_half({F, n, d, MMF_F32, MMF_RBF, nf, maxw}, C, dpf, f16, s));
  MMF_TRY(t_prep.stop(s));

  int grid = 0;
  MMF_TRY(t_scan.start(r.profile, s));
  ScanB16Panel pnl;
  pnl.seed = seed; pnl.seed_stride = n_seed;
  const ScanB16Problem sp(C, C, n, n, n_pad, dpf, d, f16, MMF_RBF, r.kk);
  const ScanB16Comb sc{P, pn, nf, maxw, maxw + 4, (int)dp, lambda_h, lambda_g};
  MMF_TRY(launch_scan_b16c(sp, sc, splits, L, pnl, s, &grid));
  MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, n, s));
  if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {   // test hook: send the first rows down the exact pass (FastTail::run's)
    const int64_t f = atoll(e);
    if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < n ? f : n) * 4, s));
  }
  MMF_TRY(t_scan.stop(s));

  SelectProblem q = r.select();
  q.k = ks; q.out_stride = k;
  q.rx = nf; q.cy = nf; q.Pq = P; q.Pc = P; q.pnq = pn; q.pnc = pn; q.dp = (int)dp; q.lambda_g = lambda_g;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = stats ? flags.cand_total : nullptr;
  MMF_TRY(t_sel.start(r.profile, s));
  MMF_TRY(launch_rerank_combined(q, L, s));
  MMF_TRY(t_sel.stop(s));

  std::vector<int32_t> h_rows((size_t)peek);
  MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)peek * 4, hipMemcpyDeviceToHost, s));
  MMF_TRY(flags.read(stats != nullptr, s));   // the call's synchronisation
  const int64_t h_fail = flags.h_fail4[0];
  MMF_TRY(t_fb.start(r.profile && h_fail > 0, s));
  if (h_fail > 0) {
    h_rows.resize((size_t)h_fail);
    if (h_fail > peek) {
      MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)h_fail * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
    }
    std::vector<char> hit((size_t)row_blocks, 0);
    int64_t n_hit = 0;
    for (int32_t row : h_rows) {
      if (row < 0 || row >= n) { set_error("%s: flagged row %d outside the %lld rows (internal invariant)", who, row, (long long)n); return MMF_E_INTERNAL; }
      if (!hit[(size_t)(row / 128)]) { hit[(size_t)(row / 128)] = 1; ++n_hit; }
    }
    ExactPass ex(r, nf, nf);
    ex.same = true;
    ex.P = P; ex.pn = pn; ex.dp = (int)dp; ex.lambda_g = lambda_g;
    if (4 * n_hit > row_blocks) {
      ex.add(ExactGroup{0, n, false, 0, n, ks});
    } else {
      for (int64_t b = 0; b < row_blocks; ++b) {
        if (!hit[(size_t)b]) continue;
        int64_t e = b;
        while (e + 1 < row_blocks && hit[(size_t)(e + 1)]) ++e;
        const int64_t row0 = b * 128, end = std::min(n, (e + 1) * 128);
        ex.add(ExactGroup{row0, end - row0, false, 0, n, ks});
        b = e;
      }
    }
    Workspace aux;   // the f32 image and the exact lists, in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), false);
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
  }
  MMF_TRY(t_fb.stop(s));
  fill_stats(stats, prec, splits, grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), h_fail, flags.h_fail4[1], flags.h_fail4[2], flags.h_tot);
  return MMF_OK;
}

// What MMF_PREC_AUTO does in mmf_simtopk_combined_fast_segmented: the 16-bit scan only for the (d, k) range where the whole call
// beat combined_topk.simtopk_combined(ptr=...) by more than three times that arm's spread at EVERY measured batch of the range
// (profiles/simtopk_combined_fast_segmented_timing.txt): k = 5 (16-entry lists), d = 512 at 2048 x 128, 1000
// ragged 100..300, 64 x 4096 and 16 x 16384 rows — 46.5x / 26.0x / 5.0x / 3.6x, the difference 605 / 489 / 167 / 381 times that
// spread — and d = 1536 at 64 x 4096 — 5.8x, 168 times.  Outside 512 <= d <= 1536, or with the 32-entry lists of k + self > 11,
// nothing is measured and AUTO stays exact, as in the one-graph entry (precision = MMF_PREC_FAST is served everywhere).
static bool combined_fast_seg_auto(int64_t d, int kk) { return d >= 512 && d <= 1536 && kk <= 11; }

// The column ranges the segmented combined scan takes on its own: FastTail's rule applied to the call (double while the served
// segments' row blocks x ranges stay below 256), capped at the one count that was measured — two.  At 4 segments of 4096 rows,
// d = 512 (128 row blocks) two ranges took 0.801 ms against 0.956 ms for one, 11.4 times the spread of the
// one-range arm, where the project's rule asks for more than three; four ranges (0.923 ms) already give some of it back, and no
// smaller batch was measured.  opts->col_splits forces a count either way.
static int combined_fast_seg_auto_splits() { return 2; }

// mmf_simtopk_combined_fast_segmented (include/ext/mmf_hg_topk16_seg.h; entry and host checks in mmf_scan_b16c.hip), DESIGN.md
// §4.18.  Every segment with at least k admissible columns is copied into ONE 16-bit image, padded to whole tiles of 128, and
// scanned by one table-driven launch (launch_scan_b16c_seg); audit, re-rank of the combined key over all rows, one readback.  The
// other segments — and every segment under MMF_PREC_EXACT — are slices of the exact pass, as run_simtopk_combined ranks them; the
// rows the audit or the re-rank flagged are answered per segment by the same pass over their 128-row blocks (counted from the
// segment's first row, adjacent blocks merged into runs; the whole segment when more than a quarter of its blocks hold one).
int run_simtopk_combined_fast_segmented(const char* who, const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                        float lambda_g, int k, int exclude_self, const int64_t* ptr, int64_t n_seg, int64_t* out_idx,
                                        float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const int self1 = exclude_self ? 1 : 0;
  const int64_t S = n_seg;
  int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec == MMF_PREC_AUTO) prec = combined_fast_seg_auto(d, k + self1) ? MMF_PREC_FAST : MMF_PREC_EXACT;
  // segments the 16-bit scan serves: at least k admissible columns (the others are ranked exactly for what they have)
  std::vector<char> served((size_t)S, 0);
  int64_t R = 0, n_pos = 0;   // row blocks and image positions of the served segments
  for (int64_t g = 0; g < S && prec != MMF_PREC_EXACT; ++g) {
    const int64_t ng = ptr[g + 1] - ptr[g];
    if (ng - self1 < k || ng == 0) continue;
    served[(size_t)g] = 1;
    R += (ng + 127) / 128;
    n_pos += (ng + 127) / 128 * 128;
  }
  if (R == 0)   // MMF_PREC_EXACT, or nothing to scan
    return run_simtopk_combined(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, ptr, S, out_idx, out_val, opts, stats, device_id,
                                hip_stream);
  if (n_pos >= (int64_t(1) << 31)) { set_error("%s: the padded image of %lld positions is too large", who, (long long)n_pos); return MMF_E_UNSUPPORTED; }
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.kk = k + self1;
  r.precision = prec;
  if (stats) memset(stats, 0, sizeof(*stats));
  MMF_TRY(r.call.begin());
  const hipStream_t s = r.call.s;
  const bool f16 = prec == MMF_PREC_FAST;
  const int dpf = scan_b16c_dp(d), bcap = scan_b16c_cap(r.kk);
  // Column ranges (DESIGN.md §4.16's rule): the call's count is a power of two bounded by the re-rank's gather (2 x ranges x cap
  // <= 1024); every segment takes at most that many, and at most one per tile of its own, rounded down to a power of two
  int call_splits = 1, max_splits = 1;
  {
    const int forced = opts ? opts->col_splits : 0;
    const auto fits = [&](int sp) { return 2 * sp * bcap <= 1024; };
    if (forced > 0) { while (call_splits < forced && fits(2 * call_splits)) call_splits <<= 1; }
    else { while (R * call_splits < 256 && 2 * call_splits <= combined_fast_seg_auto_splits() && fits(2 * call_splits)) call_splits <<= 1; }
  }
  // the work table (one entry per row block and column range) and the gather table (image position -> row of F, -1: padding)
  std::vector<int32_t> sched, gather((size_t)n_pos, -1);
  {
    int64_t pos = 0;
    for (int64_t g = 0; g < S; ++g) {
      if (!served[(size_t)g]) continue;
      const int64_t ng = ptr[g + 1] - ptr[g], tiles = (ng + 127) / 128, t0 = pos / 128;
      int sp = 1;
      while (2 * sp <= call_splits && 2 * sp <= tiles) sp <<= 1;
      if (sp > max_splits) max_splits = sp;
      const int64_t tps = (tiles + sp - 1) / sp;
      for (int64_t b = 0; b < ng; b += 128) {
        for (int c = 0; c < sp; ++c) {
          const int64_t tb = std::min(t0 + c * tps, t0 + tiles), te = std::min(tb + tps, t0 + tiles);
          const int32_t e[8] = {(int32_t)(pos + b), (int32_t)(ptr[g] + b), (int32_t)std::min<int64_t>(ng - b, 128), (int32_t)tb, (int32_t)te,
                                (int32_t)(uint32_t)(ptr[g] - pos), 2 * c, (int32_t)(ptr[g + 1] - 1)};
          sched.insert(sched.end(), e, e + 8);
        }
      }
      for (int64_t i = 0; i < ng; ++i) gather[(size_t)(pos + i)] = (int32_t)(ptr[g] + i);
      pos += tiles * 128;
    }
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  const int lists = 2 * max_splits;
  const int64_t n_img = (n_pos + 255) / 256 * 256;
  constexpr int64_t kFailPeek = 1024;   // flagged row ids that come back with the fail count
  const int64_t peek = std::min(n, kFailPeek);

  const size_t need = 2 * ws_bytes(n, 4) + ws_bytes(8, 4) + HalfImage::bytes(n_img, dpf) + ws_bytes(sched.size(), 4) + ws_bytes(n_pos, 4) +
                      b16_lists_bytes(n, lists, bcap) + FlagBlock::bytes(n) + ws_bytes(2 * (size_t)n, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(n);
  float* pn = ws.take<float>(n);
  uint32_t* maxw = ws.take<uint32_t>(8);   // word 0: largest chain(f, f) of the batch, word 4: largest chain(p, p)
  HalfImage C;
  C.carve(ws, n_img, dpf);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  int32_t* d_gather = ws.take<int32_t>(n_pos);
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  FlagBlock flags;
  flags.carve(ws, n);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)n);
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(maxw, 0, 32, s));
  // rows of segments the scan does not serve, and the unused ranges of a segment with fewer than max_splits, keep empty lists
  MMF_HIP(hipMemsetAsync(L.cnt, 0, (size_t)n * lists * 4, s));
  MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
  MMF_HIP(hipMemsetAsync(L.spill_cnt, 0, (size_t)n * 4, s));
  MMF_TRY(flags.zero(s));
  MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)n * 8, s));   // kSeedNone, thresholds and dropped keys

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(r.profile, s));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, maxw, s));
  MMF_TRY(launch_row_scalars(P, n, dp, MMF_F32, MMF_RBF, pn, maxw + 4, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(upload_table(s, d_gather, gather.data(), (size_t)n_pos * 4));
  MMF_TRY(launch_prep_half_gather({F, n, d, MMF_F32, MMF_RBF, nf, maxw}, d_gather, n_pos, C, dpf, f16, s));
  MMF_TRY(t_prep.stop(s));

  MMF_TRY(t_scan.start(r.profile, s));
  ScanB16Panel pnl;
  pnl.seed = seed; pnl.seed_stride = n;
  const ScanB16Problem sp(C, C, n, n, n_img, dpf, d, f16, MMF_RBF, r.kk);
  const ScanB16Comb sc{P, pn, nf, maxw, maxw + 4, (int)dp, lambda_h, lambda_g};
  MMF_TRY(launch_scan_b16c_seg(sp, sc, d_sched, grid, lists, L, pnl, s));
  MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, n, s));
  if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {   // test hook: send the first rows down the exact pass (FastTail::run's)
    const int64_t f = atoll(e);
    if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < n ? f : n) * 4, s));
  }
  MMF_TRY(t_scan.stop(s));

  SelectProblem q = r.select();
  q.out_stride = k;
  q.rx = nf; q.cy = nf; q.Pq = P; q.Pc = P; q.pnq = pn; q.pnc = pn; q.dp = (int)dp; q.lambda_g = lambda_g;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = stats ? flags.cand_total : nullptr;
  MMF_TRY(t_sel.start(r.profile, s));
  MMF_TRY(launch_rerank_combined(q, L, s));   // all rows: those of unserved segments come back flagged and are redone below
  MMF_TRY(t_sel.stop(s));

  std::vector<int32_t> h_rows((size_t)peek);
  MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)peek * 4, hipMemcpyDeviceToHost, s));
  MMF_TRY(flags.read(stats != nullptr, s));   // the call's synchronisation
  const int64_t h_fail = flags.h_fail4[0];
  h_rows.resize((size_t)h_fail);
  if (h_fail > peek) {
    MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)h_fail * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
  }
  std::sort(h_rows.begin(), h_rows.end());
  if (h_fail > 0 && (h_rows.front() < 0 || h_rows.back() >= n)) {
    set_error("%s: flagged row outside the %lld rows (internal invariant)", who, (long long)n);
    return MMF_E_INTERNAL;
  }

  // ---- exact pass: the segments the scan did not serve, and per served segment the blocks of its flagged rows ---------------
  ExactPass ex(r, nf, nf);
  ex.same = true;
  ex.P = P; ex.pn = pn; ex.dp = (int)dp; ex.lambda_g = lambda_g;
  int64_t fallback_rows = 0;
  size_t e = 0;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = ptr[g + 1] - ptr[g];
    const size_t e0 = e;
    while (e < h_rows.size() && h_rows[e] < ptr[g + 1]) ++e;
    if (ng == 0) continue;
    if (!served[(size_t)g]) {
      const int64_t ks = std::min<int64_t>(k, ng - self1);
      if (ks > 0) { ex.add(ExactGroup{ptr[g], ng, false, ptr[g], ng, (int)ks}); continue; }
      // one row, self excluded: -1 / -inf
      MMF_HIP(hipMemsetAsync(out_idx + ptr[g] * k, 0xff, (size_t)ng * k * 8, s));
      MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_val + ptr[g] * k), (int)0xff800000u, (size_t)ng * k, s));
      continue;
    }
    if (e == e0) continue;
    fallback_rows += (int64_t)(e - e0);
    const int64_t nb = (ng + 127) / 128;
    std::vector<char> hit((size_t)nb, 0);
    int64_t n_hit = 0;
    for (size_t i = e0; i < e; ++i) {
      const int64_t b = (h_rows[i] - ptr[g]) / 128;
      if (!hit[(size_t)b]) { hit[(size_t)b] = 1; ++n_hit; }
    }
    if (4 * n_hit > nb) { ex.add(ExactGroup{ptr[g], ng, false, ptr[g], ng, k}); continue; }
    for (int64_t b = 0; b < nb; ++b) {
      if (!hit[(size_t)b]) continue;
      int64_t l = b;
      while (l + 1 < nb && hit[(size_t)(l + 1)]) ++l;
      const int64_t row0 = ptr[g] + b * 128, end = std::min(ptr[g + 1], ptr[g] + (l + 1) * 128);
      ex.add(ExactGroup{row0, end - row0, false, ptr[g], ng, k});
      b = l;
    }
  }
  MMF_TRY(t_fb.start(r.profile && !ex.pieces.empty(), s));
  if (!ex.pieces.empty()) {
    Workspace aux;   // the f32 image and the exact lists, in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), false);
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
  }
  MMF_TRY(t_fb.stop(s));
  const int64_t overflow_rows = std::min<int64_t>(flags.h_fail4[1], fallback_rows);
  fill_stats(stats, prec, max_splits, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback_rows, overflow_rows,
             fallback_rows - overflow_rows, flags.h_tot);
  return MMF_OK;
}

// ---- mmf_simtopk_combined_xy (include/ext/mmf_hg_topk_xy.h; entry and host checks in mmf_scan_b16c.hip) --------

// What MMF_PREC_AUTO does in mmf_simtopk_combined_xy: the 16-bit scan only for the (d, k) range where the whole call beat this
// entry's own exact arm by more than three times that arm's spread at every measured shape (the rule of DESIGN.md §4.17; §4.19,
// profiles/simtopk_combined_xy_timing.txt): k = 5 (16-entry lists) at d = 512 and d = 1536, for a row panel of one eighth of
// N = 65536 and, at d = 512, of N = 262144, and for 16384 queries against 65536 distinct candidates — 3.05x / 3.83x / 3.22x at
// d = 512 and 3.48x / 3.41x at d = 1536, the difference 79 / 312 / 39 and 44 / 121 times that spread.  Outside
// 512 <= d <= 1536, or with the 32-entry lists of k + self > 11, nothing is measured and AUTO stays exact, as in the self
// entries (precision = MMF_PREC_FAST is served wherever the scan applies).
static bool combined_xy_auto(int64_t d, int kk) { return d >= 512 && d <= 1536 && kk <= 11; }

// Queries [a, b) and the entries each of them can have: all nc candidates, minus one where self is excluded and the query's own
// id lies among the candidates' ids.  Adjacent ranges with the same count are one.
struct XYRange { int64_t a, b; int ks; };
static std::vector<XYRange> xy_ranges(int64_t nq, int64_t nc, int k, int exclude_self, int64_t row_offset, int64_t col_offset) {
  int64_t o0 = 0, o1 = 0;   // the queries whose id is a candidate's
  if (exclude_self) {
    o0 = std::min(std::max<int64_t>(col_offset - row_offset, 0), nq);
    o1 = std::min(std::max<int64_t>(col_offset + nc - row_offset, o0), nq);
  }
  const XYRange three[3] = {{0, o0, (int)std::min<int64_t>(k, nc)}, {o0, o1, (int)std::min<int64_t>(k, nc - 1)}, {o1, nq, (int)std::min<int64_t>(k, nc)}};
  std::vector<XYRange> out;
  for (const XYRange& g : three) {
    if (g.a >= g.b) continue;
    if (!out.empty() && out.back().ks == g.ks) out.back().b = g.b;
    else out.push_back(g);
  }
  return out;
}

// rows without an admissible candidate: -1 / -inf
static int xy_fill_none(int64_t* out_idx, float* out_val, int64_t row0, int64_t rows, int k, hipStream_t s) {
  MMF_HIP(hipMemsetAsync(out_idx + row0 * k, 0xff, (size_t)rows * k * 8, s));
  MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_val + row0 * k), (int)0xff800000u, (size_t)rows * k, s));
  return MMF_OK;
}

// The 16-bit path of run_simtopk_combined_xy, behind r.call.begin(): nc >= k + self candidates, so every query has k entries.
// r is the call as the exact pass wants it (X = the candidates for a slice, whose row slice0 is query 0; else the queries).
// One image (candidates, then — unless the queries are rows of them — the queries), chains and positions in the joint numbering
// of mmf_scan_b16c.hip's "Two-set form", a work table of one entry per query block and column range, launch_scan_b16c_xy, audit,
// the two-sided re-rank, one readback; flagged rows as in run_simtopk_combined_fast.
static int xy_fast(Request& r, const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc, int64_t slice0,
                   int64_t dp, float lambda_g, int64_t row_offset, const mmf_simtopk_opts* opts) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const bool slice = slice0 >= 0, f16 = r.precision == MMF_PREC_FAST;
  const int64_t d = r.d, x0 = slice ? slice0 : 0;
  const int k = r.k;
  const float lambda_h = r.lambda;
  const int dpf = scan_b16c_dp(d), bcap = scan_b16c_cap(r.kk);
  const int64_t ncp = (nc + 127) / 128 * 128, tiles = ncp / 128, row_blocks = (nq + 127) / 128;
  const int64_t J = slice ? nc : nc + nq;           // rows of the joint numbering: candidates, then the queries unless they are among them
  const int64_t q_row0 = slice ? slice0 : nc;       // the first query's row in it
  const int64_t q_pos0 = slice ? slice0 : ncp;      // ... and its image position
  // a slice's last query block reads up to 127 rows behind its last query: one spare block of padding keeps them inside the image
  const int64_t n_img = ncp + (slice ? 128 : row_blocks * 128);
  if (n_img >= (int64_t(1) << 31) || J >= (int64_t(1) << 31)) { set_error("%s: the padded image of %lld positions is too large", who, (long long)n_img); return MMF_E_UNSUPPORTED; }
  // column splits: run_simtopk_combined_fast's rule, bounded by the candidate tiles
  int splits = 1;
  const int forced = opts ? opts->col_splits : 0;
  if (forced > 0) { while (splits < forced && splits < 32) splits <<= 1; }
  else { while (row_blocks * splits < 256 && splits < 32) splits <<= 1; }
  while (splits > 1 && (splits > tiles || 2 * splits * bcap > 1024)) splits >>= 1;
  const int lists = 2 * splits;
  const int64_t tps = (tiles + splits - 1) / splits;
  std::vector<int32_t> sched;
  sched.reserve((size_t)row_blocks * splits * 8);
  for (int64_t b = 0; b < nq; b += 128) {
    for (int c = 0; c < splits; ++c) {
      const int64_t tb = std::min(c * tps, tiles), te = std::min(tb + tps, tiles);
      const int32_t e[8] = {(int32_t)(q_pos0 + b), (int32_t)(q_row0 + b), (int32_t)std::min<int64_t>(nq - b, 128), (int32_t)tb, (int32_t)te, 0,
                            2 * c, (int32_t)(nc - 1)};
      sched.insert(sched.end(), e, e + 8);
    }
  }
  const int64_t grid = row_blocks * splits;
  constexpr int64_t kFailPeek = 1024;   // flagged row ids that come back with the fail count
  const int64_t peek = std::min(nq, kFailPeek);

  const size_t need = 2 * ws_bytes(J, 4) + ws_bytes(8, 4) + (slice ? 0 : ws_bytes((size_t)J * dp, 4)) + HalfImage::bytes(n_img, dpf) +
                      ws_bytes(sched.size(), 4) + b16_lists_bytes(nq, lists, bcap) + FlagBlock::bytes(nq) + ws_bytes(2 * (size_t)nq, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(J);
  float* pn = ws.take<float>(J);
  uint32_t* maxw = ws.take<uint32_t>(8);   // word 0: largest chain(f, f) of both sides, word 4: largest chain(p, p)
  float* Pj = slice ? nullptr : ws.take<float>((size_t)J * dp);   // both sides' positions in the joint numbering
  HalfImage C;
  C.carve(ws, n_img, dpf);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  const CandLists L = carve_b16_lists(ws, nq, lists, bcap);
  FlagBlock flags;
  flags.carve(ws, nq);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)nq);
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(maxw, 0, 32, s));
  MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)nq * 4, s));
  MMF_TRY(flags.zero(s));
  MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)nq * 8, s));   // kSeedNone, thresholds and dropped keys

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(r.profile, s));
  MMF_TRY(launch_row_scalars(Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw, s));
  MMF_TRY(launch_row_scalars(Pc, nc, dp, MMF_F32, MMF_RBF, pn, maxw + 4, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  if (slice) {
    MMF_TRY(launch_prep_half({Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw}, C, dpf, f16, s));
  } else {
    // scale and maxima over both sides: the queries' scalars join the same words before either image is written
    MMF_TRY(launch_row_scalars(Fq, nq, d, MMF_F32, MMF_RBF, nf + nc, maxw, s));
    MMF_TRY(launch_row_scalars(Pq, nq, dp, MMF_F32, MMF_RBF, pn + nc, maxw + 4, s));
    MMF_HIP(hipMemcpyAsync(Pj, Pc, (size_t)nc * dp * 4, hipMemcpyDeviceToDevice, s));
    MMF_HIP(hipMemcpyAsync(Pj + nc * dp, Pq, (size_t)nq * dp * 4, hipMemcpyDeviceToDevice, s));
    HalfImage Cc = C;
    Cc.n_pad = ncp;
    MMF_TRY(launch_prep_half({Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw}, Cc, dpf, f16, s));
    MMF_TRY(launch_prep_half({Fq, nq, d, MMF_F32, MMF_RBF, nf + nc, maxw}, C.from_row(ncp, dpf), dpf, f16, s));
  }
  MMF_TRY(t_prep.stop(s));

  MMF_TRY(t_scan.start(r.profile, s));
  ScanB16Panel pnl;
  pnl.seed = seed; pnl.seed_stride = nq;
  const ScanB16Problem sp(C, C, nq, nc, n_img, dpf, d, f16, MMF_RBF, r.kk);
  const ScanB16Comb sc{slice ? Pc : Pj, pn, nf, maxw, maxw + 4, (int)dp, lambda_h, lambda_g};
  MMF_TRY(launch_scan_b16c_xy(sp, sc, d_sched, grid, lists, q_row0, L, pnl, s));
  MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, nq, s));
  if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {   // test hook: send the first queries down the exact pass (FastTail::run's)
    const int64_t f = atoll(e);
    if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < nq ? f : nq) * 4, s));
  }
  MMF_TRY(t_scan.stop(s));

  SelectProblem q = r.select();
  q.X = Fq; q.n = nq; q.n_rows = nq; q.row_offset = row_offset; q.out_stride = k;
  q.rx = nf + q_row0; q.cy = nf; q.Pq = Pq; q.Pc = Pc; q.pnq = pn + q_row0; q.pnc = pn; q.dp = (int)dp; q.lambda_g = lambda_g;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = r.stats ? flags.cand_total : nullptr;
  MMF_TRY(t_sel.start(r.profile, s));
  MMF_TRY(launch_rerank_combined(q, L, s));
  MMF_TRY(t_sel.stop(s));

  std::vector<int32_t> h_rows((size_t)peek);
  MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)peek * 4, hipMemcpyDeviceToHost, s));
  MMF_TRY(flags.read(r.stats != nullptr, s));   // the call's synchronisation
  const int64_t h_fail = flags.h_fail4[0];
  MMF_TRY(t_fb.start(r.profile && h_fail > 0, s));
  if (h_fail > 0) {
    h_rows.resize((size_t)h_fail);
    if (h_fail > peek) {
      MMF_HIP(hipMemcpyAsync(h_rows.data(), flags.fail_rows, (size_t)h_fail * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
    }
    std::vector<char> hit((size_t)row_blocks, 0);
    int64_t n_hit = 0;
    for (int32_t row : h_rows) {
      if (row < 0 || row >= nq) { set_error("%s: flagged row %d outside the %lld queries (internal invariant)", who, row, (long long)nq); return MMF_E_INTERNAL; }
      if (!hit[(size_t)(row / 128)]) { hit[(size_t)(row / 128)] = 1; ++n_hit; }
    }
    // the exact pass over the flagged queries' 128-row blocks against all candidates: rows x0 + ... of r.X
    ExactPass ex(r, nf + (slice ? 0 : nc), nf);
    ex.same = slice;
    ex.P = slice ? Pc : Pq; ex.pn = pn + (slice ? 0 : nc); ex.dp = (int)dp; ex.lambda_g = lambda_g; ex.out_row0 = x0;
    if (!slice) { ex.Pc = Pc; ex.pnc = pn; }
    if (4 * n_hit > row_blocks) {
      ex.add(ExactGroup{x0, nq, false, 0, nc, k});
    } else {
      for (int64_t b = 0; b < row_blocks; ++b) {
        if (!hit[(size_t)b]) continue;
        int64_t e = b;
        while (e + 1 < row_blocks && hit[(size_t)(e + 1)]) ++e;
        const int64_t row0 = b * 128, end = std::min(nq, (e + 1) * 128);
        ex.add(ExactGroup{x0 + row0, end - row0, false, 0, nc, k});
        b = e;
      }
    }
    Workspace aux;   // the f32 images and the exact lists, in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), false);
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
  }
  MMF_TRY(t_fb.stop(s));
  fill_stats(r.stats, r.precision, splits, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), h_fail, flags.h_fail4[1], flags.h_fail4[2],
             flags.h_tot);
  return MMF_OK;
}

// Queries against candidates.  A row slice (Fq / Pq point at the same row of Fc / Pc, nq rows inside nc) is a slice of the
// candidates against themselves: one image, one set of chains, and the groups the self entries run for those rows — so their bits.
// Exact: one ExactGroup of all queries against all candidates (up to three when self is excluded, some queries' ids lie among the
// candidates' and there are fewer than k + 1 candidates: the queries then differ in how many entries they can have).
int run_simtopk_combined_xy(const char* who, const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                            int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self, int64_t row_offset,
                            int64_t col_offset, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                            int device_id, void* hip_stream) {
  const int self1 = exclude_self ? 1 : 0, kk = k + self1;
  int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec == MMF_PREC_AUTO) prec = (scan_b16c_supported(d, kk) && combined_xy_auto(d, kk)) ? MMF_PREC_FAST : MMF_PREC_EXACT;
  if (nc < kk) prec = MMF_PREC_EXACT;   // fewer candidates than a row's lists keep: nothing for a candidate scan to narrow down
  int64_t slice0 = -1;
  if (nc > 0) {
    const uintptr_t fq = reinterpret_cast<uintptr_t>(Fq), fc = reinterpret_cast<uintptr_t>(Fc);
    const size_t row_bytes = (size_t)d * 4;
    if (fq >= fc && (fq - fc) % row_bytes == 0) {
      const int64_t r0 = (int64_t)((fq - fc) / row_bytes);
      if (r0 <= nc - nq && Pq == Pc + r0 * dp) slice0 = r0;
    }
  }
  const bool slice = slice0 >= 0;
  const int64_t x0 = slice ? slice0 : 0;   // query 0 is row x0 of r.X
  Request r{Call(who, device_id, hip_stream), slice ? Fc : Fq, slice ? nc : nq, Fc, nc, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self,
            row_offset - x0, col_offset, out_idx, out_val, stats, opts && opts->profile};
  r.kk = kk;
  r.precision = prec;
  if (stats) memset(stats, 0, sizeof(*stats));
  MMF_TRY(r.call.begin());
  const hipStream_t s = r.call.s;
  if (stats) stats->precision_used = prec;
  if (nc == 0) return xy_fill_none(out_idx, out_val, 0, nq, k, s);
  if (prec != MMF_PREC_EXACT) return xy_fast(r, Fq, Pq, nq, Fc, Pc, nc, slice0, dp, lambda_g, row_offset, opts);

  ExactPass ex(r, nullptr, nullptr);
  ex.same = slice;
  ex.forced_splits = opts ? opts->col_splits : 0;
  ex.dp = (int)dp; ex.lambda_g = lambda_g; ex.out_row0 = x0;
  std::vector<XYRange> bare;   // queries without an admissible candidate (one candidate, and it is the query itself)
  for (const XYRange& g : xy_ranges(nq, nc, k, exclude_self, row_offset, col_offset)) {
    if (g.ks > 0) ex.add(ExactGroup{x0 + g.a, g.b - g.a, false, 0, nc, g.ks});
    else bare.push_back(g);
  }
  const size_t need = 2 * ws_bytes(nc, 4) + (slice ? 0 : 2 * ws_bytes(nq, 4)) + ws_bytes(256, 4) +
                      (ex.pieces.empty() ? 0 : ex.image_bytes() + ex.list_bytes());
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nfc = ws.take<float>(nc);
  float* pnc = ws.take<float>(nc);
  float* nfq = slice ? nfc : ws.take<float>(nq);
  float* pnq = slice ? pnc : ws.take<float>(nq);
  uint32_t* cand_total = ws.take<uint32_t>(256);
  ex.rx = nfq; ex.cy = nfc; ex.P = slice ? Pc : Pq; ex.pn = pnq;
  if (!slice) { ex.Pc = Pc; ex.pnc = pnc; }
  ex.cand_total = stats ? cand_total : nullptr;
  for (const XYRange& g : bare) MMF_TRY(xy_fill_none(out_idx, out_val, g.a, g.b - g.a, k, s));
  if (ex.pieces.empty()) return MMF_OK;
  ExactLists B;
  B.carve(ws, ex.rows_total, ex.list_words, ex.cap(), ex.floors());   // floors: the passes of the any-k entries (k + self > 44)
  MMF_TRY(B.zero(s));
  MMF_HIP(hipMemsetAsync(cand_total, 0, 1024, s));

  // timers as run_simtopk_combined: prep (row scalars, f32 images), scan, re-rank for one group; with several, "scan" is all of it
  const bool one = ex.pieces.size() == 1;
  EventTimer t[3];
  MMF_TRY(t[0].start(r.profile, s));
  MMF_TRY(launch_row_scalars(Fc, nc, d, MMF_F32, MMF_RBF, nfc, nullptr, s));
  MMF_TRY(launch_row_scalars(Pc, nc, dp, MMF_F32, MMF_RBF, pnc, nullptr, s));
  if (!slice) {
    MMF_TRY(launch_row_scalars(Fq, nq, d, MMF_F32, MMF_RBF, nfq, nullptr, s));
    MMF_TRY(launch_row_scalars(Pq, nq, dp, MMF_F32, MMF_RBF, pnq, nullptr, s));
  }
  if (!one) { MMF_TRY(t[0].stop(s)); MMF_TRY(t[1].start(r.profile, s)); }
  std::vector<uint32_t> h_tot(stats ? 256 : 0);
  MMF_TRY(ex.run(ws, B, one ? t : nullptr, stats ? &h_tot : nullptr));
  if (!one) MMF_TRY(t[1].stop(s));
  fill_stats(stats, MMF_PREC_EXACT, ex.splits(ex.pieces[0]), ex.grid, t[0].ms(), t[1].ms(), t[2].ms(), 0.f, 0, 0, 0, h_tot);
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_version(void) { return MMF_ABI_VERSION; }
int mmf_debug_query_order(int32_t* perm_host, int64_t n) { return query_order_last(perm_host, n); }
int64_t mmf_debug_symmetric_schedule(int64_t row_blocks, int group, int launch, int32_t* table_host, int64_t capacity) {
  if (row_blocks < 1 || group < 1 || launch < 0 || launch > 1) { set_error("debug_symmetric_schedule: bad argument"); return MMF_E_INVALID; }
  const int64_t grid = sym_schedule_grid(row_blocks, group);
  if (table_host) {
    if (capacity < grid) { set_error("debug_symmetric_schedule: table of %lld entries needed", (long long)grid); return MMF_E_INVALID; }
    bool live, forward;
    symmetric_live_mode(&live, &forward);
    int phases; bool antipodal;
    symmetric_schedule_mode(&phases, &antipodal, group, 1);
    sym_schedule_table(row_blocks, group, launch, table_host, forward, phases, antipodal);
  }
  return grid;
}
const char* mmf_last_error(void) { return g_err; }

int mmf_release_workspaces(void) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  query_order_forget();
  for (auto& slot : g_ws) {
    for (auto& kv : slot) {
      if (kv.second.base) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(kv.first.first);
        (void)hipDeviceSynchronize();
        (void)hipFree(kv.second.base);
        if (prev >= 0) (void)hipSetDevice(prev);
      }
    }
    slot.clear();
  }
  for (auto& kv : g_stage) {                      // the pinned staging blocks of upload_table, once their device is idle
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(kv.first.first);
    (void)hipDeviceSynchronize();
    for (StageBlock& b : kv.second) {
      (void)hipEventDestroy(b.passed);
      (void)hipHostFree(b.host);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  g_stage.clear();
  return MMF_OK;
}

// The 16-bit operands of a fast call: both images and both scalar vectors, shared or not, and max_n.  X a row-slice of Y (the
// row-sharded multi-GPU case passes full[lo:hi] and full): every query-side buffer is then a view into the candidate-side one
// and only Y is prepared.
struct FastPrep {
  int64_t n, m; int dp; bool f16;
  bool same, shared; int64_t slice0 = -1, n_pad, m_pad;
  float *rx = nullptr, *cy = nullptr; HalfImage Q, C;
  uint32_t* max_n = nullptr;   // largest squared row norm over X and Y -> common scale
  FastPrep(const Request& r, int dp_, bool f16_) : n(r.n), m(r.m), dp(dp_), f16(f16_) {
    same = (r.Y == r.X) && (m == n);
    const size_t row_bytes = (size_t)r.d * dtype_size(r.dtype);
    if (!same) {
      const char* xb = static_cast<const char*>(r.X);
      const char* yb = static_cast<const char*>(r.Y);
      if (xb >= yb && xb + (size_t)n * row_bytes <= yb + (size_t)m * row_bytes && ((size_t)(xb - yb) % row_bytes) == 0)
        slice0 = (int64_t)((size_t)(xb - yb) / row_bytes);
    }
    shared = same || slice0 >= 0;
    n_pad = (n + 255) / 256 * 256; m_pad = (m + 255) / 256 * 256 + (slice0 >= 0 ? 256 : 0);
  }
  size_t bytes() const { return ws_bytes(n, 4) + ws_bytes(m, 4) + HalfImage::bytes(n_pad, dp) + HalfImage::bytes(m_pad, dp) + ws_bytes(4, 4); }
  // the candidate side is always carved; the query side is rows r0 .. of it (shared) or a carve of its own
  void carve(Workspace& ws) {
    const int64_t r0 = same ? 0 : slice0;
    rx = shared ? nullptr : ws.take<float>(n);
    cy = ws.take<float>(m);
    if (!shared) Q.carve(ws, n_pad, dp);
    C.carve(ws, m_pad, dp);
    if (shared) { rx = cy + r0; Q = C.from_row(r0, dp); }
    max_n = ws.take<uint32_t>(4);
  }
  int run(const Request& r, EventTimer* t_prep) const {
    const hipStream_t s = r.call.s;
    MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
    MMF_HIP(hipMemsetAsync(max_n, 0, 16, s));
    if (!shared) MMF_HIP(hipMemsetAsync(Q.maxima, 0, 16, s));
    MMF_TRY(t_prep->start(r.profile, s));
    MMF_TRY(launch_row_scalars(r.Y, m, r.d, r.dtype, r.metric, cy, max_n, s));
    if (!shared) MMF_TRY(launch_row_scalars(r.X, n, r.d, r.dtype, r.metric, rx, max_n, s));
    MMF_TRY(launch_prep_half({r.Y, m, r.d, r.dtype, r.metric, cy, max_n}, C, dp, f16, s));
    if (!shared) MMF_TRY(launch_prep_half({r.X, n, r.d, r.dtype, r.metric, rx, max_n}, Q, dp, f16, s));
    return t_prep->stop(s);
  }
  FastOperands operands() const { return FastOperands{Q, C, rx, cy, (m + 255) / 256 * 256, dp, f16}; }
};

// mmf_simtopk_ex behind its checks (and mmf_simtopk_fast_anyk where one pass serves): the fast path or the exact path, as r.precision says
static int simtopk_run(Request& r, const mmf_simtopk_opts* opts) {
  const void* X = r.X; const void* Y = r.Y;
  const int64_t n = r.n, m = r.m, d = r.d, row_offset = r.row_offset, col_offset = r.col_offset;
  const int in_dtype = r.dtype, metric = r.metric, k = r.k;
  mmf_simtopk_stats* stats = r.stats;
  if (n == 0) return MMF_OK;
  const hipStream_t s = r.call.s;
  const int forced_splits = opts ? opts->col_splits : 0;
  const bool same = (Y == X) && (m == n);

  if (r.precision != MMF_PREC_EXACT) {
    // ---- fast path: f16/bf16 MFMA scan -> exact re-rank -> exact rescan of overflowed rows -------
    const int dp = r.wide ? scan_b16w_dp(d) : scan_bf16_dp(d);
    const bool f16 = (r.precision == MMF_PREC_FAST);   // operand type of the scan, not of the input
    FastPrep fp(r, dp, f16);
    FastTail ft(n, m, r.kk, forced_splits, dp);
    MMF_TRY(ft.set_query_order(opts ? opts->query_order : MMF_QUERY_ORDER_AUTO));
    {
      int G = 0;
      if (symmetric_scan_wanted(n, dp, ft.bcap, metric, forced_splits, same && row_offset == col_offset, &G)) ft.set_symmetric(G);
    }
    Workspace ws;
    MMF_TRY(r.call.workspace(fp.bytes() + ft.bytes(), &ws));
    fp.carve(ws);
    ft.carve(ws);
    EventTimer t_prep;
    MMF_TRY(fp.run(r, &t_prep));

    MMF_TRY(ft.run(r, fp.operands(), opts ? opts->select_wait_event : nullptr));
    if (stats) stats->prep_ms = t_prep.ms();
    return MMF_OK;
  }

  // ---- exact path: everything in the call's workspace ---------------------------------------------------------------
  ExactPass ex(r, nullptr, nullptr);
  ex.same = same;
  ex.forced_splits = forced_splits;
  ex.add(ExactGroup{0, n, false, 0, m, k});
  const size_t need = ws_bytes(n, 4) + (same ? 0 : ws_bytes(m, 4)) + ws_bytes(256, 4) + ex.image_bytes() + ex.list_bytes();
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = same ? rx : ws.take<float>(m);
  uint32_t* cand_total = ws.take<uint32_t>(256);
  ExactLists B;
  B.carve(ws, n, ex.list_words, ex.cap(), ex.floors());
  ex.rx = rx; ex.cy = cy;
  ex.cand_total = stats ? cand_total : nullptr;
  MMF_TRY(B.zero(s));
  MMF_HIP(hipMemsetAsync(cand_total, 0, 1024, s));

  EventTimer t[3];   // prep (row scalars and f32 images), scan, re-rank
  MMF_TRY(t[0].start(r.profile, s));
  MMF_TRY(launch_row_scalars(X, n, d, in_dtype, metric, rx, nullptr, s));
  if (!same) MMF_TRY(launch_row_scalars(Y, m, d, in_dtype, metric, cy, nullptr, s));
  std::vector<uint32_t> h_tot(stats ? 256 : 0);
  MMF_TRY(ex.run(ws, B, t, stats ? &h_tot : nullptr));
  fill_stats(stats, MMF_PREC_EXACT, ex.splits(ex.pieces[0]), ex.grid, t[0].ms(), t[1].ms(), t[2].ms(), 0.f, 0, 0, 0, h_tot);
  return MMF_OK;
}

int mmf_simtopk_ex(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                   float lambda, int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx,
                   float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id,
                   void* hip_stream) {
  if (!Y) { Y = X; m = n; }
  Request r{Call("simtopk", device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset, col_offset,
            out_idx, out_val, stats, opts && opts->profile};
  r.wide_ok = true;
  MMF_TRY(r.check(opts ? opts->precision : MMF_PREC_AUTO, false, [] { return MMF_OK; }));
  return simtopk_run(r, opts);
}

// ---- mmf_simtopk_fast_anyk (include/ext/mmf_hg_fast_anyk.h) ---------------------------------------------------
// The depth of a pass of the 16-bit scan, self's slot included: the largest k + self scan_bf16_supported serves at d.
static int anyk_depth(int64_t d) { return d <= 512 ? 44 : 20; }

// What every *_anyk_plan reports behind its own checks.  one: a single pass at k + self serves the call; else pass 0 at the full
// depth and later passes of at most depth - self entries each.  Returns 0 / 1 for one / several passes.
static int anyk_plan(int64_t d, int k, int self1, bool one, int* scan_kk, int* first_yield, int* min_passes) {
  const int depth = one ? k + self1 : anyk_depth(d), per = anyk_depth(d) - self1;
  if (scan_kk) *scan_kk = depth;
  if (first_yield) *first_yield = depth - self1;
  if (min_passes) *min_passes = one ? 1 : 1 + (k - (depth - self1) + per - 1) / per;
  return one ? 0 : 1;
}

int mmf_fast_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes) {
  if (d < 1 || k < 1) { set_error("fast_anyk_plan: need d >= 1 and k >= 1 (got d = %lld, k = %d)", (long long)d, k); return MMF_E_INVALID; }
  const int self1 = exclude_self ? 1 : 0, kk = k + self1;
  const bool one = d <= 1024 ? scan_bf16_supported(d, kk, MMF_F32) != 0 : scan_b16w_supported(d, kk) != 0;
  if (!one && d > 1024) {
    set_error("fast_anyk_plan: d = %lld, k = %d is beyond one pass of the wide 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
              (long long)d, k);
    return MMF_E_UNSUPPORTED;
  }
  return anyk_plan(d, k, self1, one, scan_kk, first_yield, min_passes);
}

// MMF_ANYK_SHORT_DIV (read per call): a later pass may leave n / div unflagged rows short of its yield (they take the exact rescan).
// An operating point, not a correctness condition (profiles/fast_anyk_timing.txt).
static int64_t anyk_short_div() {
  const char* e = getenv("MMF_ANYK_SHORT_DIV");
  const long v = e ? atol(e) : 0;
  return (v >= 1 && v <= 65536) ? v : 64;
}

static void anyk_record(mmf_fast_anyk_info* info, int pass, int yield, int ghost_max, int64_t exact_rows) {
  if (!info) return;
  info->passes = pass + 1;
  if (pass >= MMF_FAST_ANYK_MAX_PASSES) return;
  info->yield[pass] = yield; info->ghost_max[pass] = ghost_max; info->exact_rows[pass] = exact_rows;
}

// The yield of a later pass: the largest t <= t_max that leaves at most `budget` unflagged rows short of it (0: none does).
// h: launch_anyk_count's histogram, rows per certified count; *short_rows: the unflagged rows with fewer than t certified entries.
static int anyk_yield(const uint32_t* h, int t_max, int64_t budget, int64_t* short_rows) {
  int t = 0;
  int64_t below = 0;
  *short_rows = 0;
  for (int tq = 1; tq <= t_max; ++tq) {
    below += h[tq - 1];
    if (below > budget) break;
    t = tq; *short_rows = below;
  }
  return t;
}

// The re-rank of a later pass: K entries per row into the K-wide staging rows with their keys, flagged rows into `flags`.
static SelectProblem anyk_stage_select(const Request& r, int K, int64_t* sidx, float* sval, float* skey, const float* rx, const float* cy,
                                       const FlagBlock& flags, char* order_scratch) {
  SelectProblem q = r.select();
  q.k = K; q.out_idx = sidx; q.out_val = sval; q.key_out = skey; q.out_stride = K;
  q.rx = rx; q.cy = cy;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count;
  q.two_pass = true;
  q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
  return q;
}

// What a table-driven 16-bit scan of the segmented and cross-segment runners needs reset before every launch: list counts (the slots
// a block's entries do not use stay empty), overflow marks, overflow-list counts (the wide scan has no such lists: select reads them
// as empty) and the thresholds' seeds.
static int reset_b16_lists(const CandLists& L, int64_t n, int lists, int32_t* seed, int64_t n_seed, hipStream_t s) {
  MMF_HIP(hipMemsetAsync(L.cnt, 0, (size_t)n * lists * 4, s));
  MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
  MMF_HIP(hipMemsetAsync(L.spill_cnt, 0, (size_t)n * 4, s));
  MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)n_seed * 8, s));
  return MMF_OK;
}

// The passes (r.precision MMF_PREC_FAST or _FAST_BF16, k + self beyond one pass; d <= 1024: mmf_simtopk_fast_anyk, above it the wide
// scan's launches take the narrow ones' slots: mmf_simtopk_wide_anyk).  Pass 0 is the fast call at the full
// depth (FastTail::run), leaving every row's floor.  A later pass: ceilings from the floors, the plain scan under them at the full
// depth, the re-rank into the staging rows, the count of each row's certified entries (one host synchronisation: histogram and
// flagged rows), the yield t, the emit of t entries per row, and the exact rescan with floors of the rows that could not.
static int fast_anyk_run(Request& r, const mmf_simtopk_opts* opts, mmf_fast_anyk_info* info) {
  const int64_t n = r.n, m = r.m;
  const hipStream_t s = r.call.s;
  const int k = r.k, self1 = r.exclude_self ? 1 : 0, depth = anyk_depth(r.d), K = depth - self1;
  const bool wide = r.d > 1024;   // launch_scan_b16w_ceilings / _ceil for launch_scan_b16_ceilings / _ceil; no query order (FastTail)
  const int dp = wide ? scan_b16w_dp(r.d) : scan_bf16_dp(r.d);
  FastPrep fp(r, dp, r.precision == MMF_PREC_FAST);
  // (the symmetric scan needs the 15-entry lists of k + self <= 11: it never applies at the full depth)
  FastTail ft(n, m, depth, opts ? opts->col_splits : 0, dp);
  MMF_TRY(ft.set_query_order(opts ? opts->query_order : MMF_QUERY_ORDER_AUTO));
  ft.leave_floors = true; ft.out_stride = k;
  // the exact rescans of the later passes, FB rows at a time: lists for the deepest exact pass, with floors
  const int xcap = scan_f32_cap(44), xsplits = pick_splits((ft.FB + 127) / 128, (m + 127) / 128, xcap, 0);
  const size_t xwords = (size_t)ft.FB * 2 * xsplits;
  const size_t stage = (size_t)n * K;
  const size_t extra = 4 * ws_bytes(n, 4) + ws_bytes(fp.n_pad, 4) + ws_bytes(64, 4) + ws_bytes(4, 4) + ws_bytes(stage, 8) + 2 * ws_bytes(stage, 4) +
                       ExactLists::bytes(ft.FB, xwords, xcap, true);
  Workspace ws;
  MMF_TRY(r.call.workspace(fp.bytes() + ft.bytes() + extra, &ws));
  fp.carve(ws);
  ft.carve(ws);
  float* fkey = ws.take<float>(n); uint32_t* fid = ws.take<uint32_t>(n);
  int32_t* certified = ws.take<int32_t>(n); int32_t* rescan_rows = ws.take<int32_t>(n);
  float* ceil = ws.take<float>(fp.n_pad);
  uint32_t* hist = ws.take<uint32_t>(64); uint32_t* rescan_count = ws.take<uint32_t>(4);
  int64_t* sidx = ws.take<int64_t>(stage); float* sval = ws.take<float>(stage); float* skey = ws.take<float>(stage);
  ExactLists XB;
  XB.carve(ws, ft.FB, xwords, xcap, true);
  ft.floor_key_out = fkey; ft.floor_id_out = fid;
  EventTimer t_prep;
  MMF_TRY(fp.run(r, &t_prep));

  // pass 0: K entries per row, r.k wide rows
  r.k = K; r.kk = depth;
  const int rc0 = ft.run(r, fp.operands(), nullptr);
  r.k = k; r.kk = k + self1;
  MMF_TRY(rc0);
  if (r.stats) r.stats->prep_ms = t_prep.ms();
  anyk_record(info, 0, K, 0, ft.failed_rows);

  const int64_t budget = n / anyk_short_div();
  const CandLists L = ft.view(false);
  ScanB16Panel pn;
  pn.seed = ft.seed; pn.seed_stride = ft.n_seed; pn.share = ft.splits > 1 ? 1 : 0;
  const ScanB16Problem sp(fp.Q, fp.C, n, m, (m + 255) / 256 * 256, dp, r.d, fp.f16, r.metric, depth);
  const AnykStage st{sidx, sval, skey, n, K, r.col_offset};
  CandLists Lw = L;   // wide: what the scan writes — without the sink the overflow lists stay zeroed and select reads them as empty
  if (wide) {
    if (!wide_sink_mode()) { Lw.spill_cnt = nullptr; Lw.spill_ids = nullptr; Lw.spill_cap = 0; Lw.spill_stacks = 0; }
    pn.sunk = ft.seed + 2 * ft.n_seed;
  }
  int done = K;
  // kq more entries, from the floors on, for `cnt` rows by the exact scan; floors left unless these are the call's last entries
  auto exact_rows = [&](const int32_t* rows, int64_t cnt, int kq) -> int {
    ExactPass ex(r, fp.rx, fp.cy);
    ex.row_ids = rows; ex.n_ids = cnt; ex.forced_splits = xsplits;
    ex.out_off0 = done; ex.floors_in = true; ex.floors_out = done + kq < k;
    ex.row_floor_key = fkey; ex.row_floor_id = fid;
    ex.add(ExactGroup{0, cnt, true, 0, m, kq});
    Workspace aux;
    MMF_TRY(r.call.workspace(ex.image_bytes(), &aux, 1));
    MMF_TRY(XB.zero(s));
    MMF_TRY(ex.run(aux, XB));
    if (r.stats) r.stats->fallback_rows += cnt;
    return MMF_OK;
  };
  auto finish_exact = [&](int pass) -> int {   // every row, everything that is left
    MMF_TRY(launch_anyk_iota(rescan_rows, n, s));
    MMF_TRY(exact_rows(rescan_rows, n, k - done));
    anyk_record(info, pass, k - done, 0, n);
    return MMF_OK;
  };
  for (int pass = 1; done < k; ++pass) {
    if (pass >= MMF_FAST_ANYK_MAX_PASSES - 1) return finish_exact(pass);
    if (wide) MMF_TRY(launch_scan_b16w_ceilings(sp, fkey, fp.rx, fp.max_n, r.lambda, fp.n_pad, ceil, s));
    else MMF_TRY(launch_scan_b16_ceilings(sp, L.cap, fkey, fp.rx, fp.max_n, r.lambda, fp.n_pad, ceil, s));
    MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
    MMF_TRY(ft.flags.zero(s));
    MMF_HIP(hipMemsetAsync(ft.seed, 0x80, (size_t)ft.n_seed * 4 * ft.seed_stripes(), s));
    MMF_HIP(hipMemsetAsync(L.spill_cnt, 0, (size_t)n * 4, s));
    if (wide) MMF_TRY(launch_scan_b16w_ceil(sp, ft.splits, Lw, pn, ceil, s, nullptr));
    else MMF_TRY(launch_scan_b16_ceil(sp, ft.splits, L, ft.scan_scratch, pn, ceil, s, nullptr));
    MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
    MMF_TRY(launch_select(anyk_stage_select(r, K, sidx, sval, skey, fp.rx, fp.cy, ft.flags, ft.order_scratch), L, s));
    MMF_TRY(launch_anyk_count(st, ft.flags.fail_rows, ft.flags.fail_count, fkey, fid, certified, hist, s));
    uint32_t h[64];
    MMF_HIP(hipMemcpyAsync(h, hist, (size_t)(K + 3) * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    int64_t short_rows = 0;
    const int t = anyk_yield(h, std::min(K, k - done), budget, &short_rows);
    if (t < 1) return finish_exact(pass);
    MMF_TRY(launch_anyk_emit(st, certified, t, done, k, r.out_idx, r.out_val, fkey, fid, rescan_rows, rescan_count, s));
    const int64_t rescan = (int64_t)h[K + 1] + short_rows;
    if (rescan > 0) MMF_TRY(exact_rows(rescan_rows, rescan, t));
    anyk_record(info, pass, t, (int)h[K + 2], rescan);
    done += t;
  }
  return MMF_OK;
}

int mmf_simtopk_fast_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                          int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                          const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                          mmf_fast_anyk_info* info) {
  if (!Y) { Y = X; m = n; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call("simtopk_fast_anyk", device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset, col_offset,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the 16-bit scan serves d but not k + self (the checks below refuse what makes this meaningless)
  const bool multi = fast && d >= 1 && d <= 1024 && k >= 1 && !scan_bf16_supported(d, k + (exclude_self ? 1 : 0), in_dtype);
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, false, [&] {
    if (asked < MMF_PREC_AUTO || asked > MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", r.call.who, asked); return MMF_E_INVALID; }
    if (opts && opts->select_wait_event) {
      set_error("%s: select_wait_event is not supported (every pass reads the rows; wait on the stream before the call)", r.call.who);
      return MMF_E_UNSUPPORTED;
    }
    if (fast && d > 1024 && r.kk > 20) {
      set_error("%s: d = %lld, k = %d is beyond one pass of the wide 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
                r.call.who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }));
  if (n == 0) return MMF_OK;
  if (!multi) {
    MMF_TRY(simtopk_run(r, opts));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return fast_anyk_run(r, opts, info);
}

// ---- mmf_simtopk_wide_anyk (include/ext/mmf_hg_wide_anyk.h) ---------------------------------------------------
int mmf_wide_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes) {
  if (d < 1 || k < 1) { set_error("wide_anyk_plan: need d >= 1 and k >= 1 (got d = %lld, k = %d)", (long long)d, k); return MMF_E_INVALID; }
  if (d <= 1024) { set_error("wide_anyk_plan: d = %lld is served by mmf_fast_anyk_plan (this one: 1024 < d <= 4096)", (long long)d); return MMF_E_UNSUPPORTED; }
  if (d > 4096) { set_error("wide_anyk_plan: d = %lld is beyond the wide 16-bit scan (1024 < d <= 4096)", (long long)d); return MMF_E_UNSUPPORTED; }
  const int self1 = exclude_self ? 1 : 0;
  return anyk_plan(d, k, self1, scan_b16w_supported(d, k + self1) != 0, scan_kk, first_yield, min_passes);
}

int mmf_simtopk_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                          int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                          const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                          mmf_fast_anyk_info* info) {
  if (!Y) { Y = X; m = n; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call("simtopk_wide_anyk", device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset, col_offset,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the wide scan serves d but not k + self (the checks below refuse what makes this meaningless)
  const bool multi = fast && d > 1024 && d <= 4096 && k >= 1 && !scan_b16w_supported(d, k + (exclude_self ? 1 : 0));
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, false, [&] {
    if (asked < MMF_PREC_AUTO || asked > MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", r.call.who, asked); return MMF_E_INVALID; }
    if (opts && opts->select_wait_event) {
      set_error("%s: select_wait_event is not supported (every pass reads the rows; wait on the stream before the call)", r.call.who);
      return MMF_E_UNSUPPORTED;
    }
    if (d <= 1024) {
      set_error("%s: d = %lld is not above 1024: call mmf_simtopk_fast_anyk, which serves d <= 1024 for any k", r.call.who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    if (fast && d > 4096) {
      set_error("%s: d = %lld is beyond the wide 16-bit scan (1024 < d <= 4096; MMF_PREC_EXACT serves it)", r.call.who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }));
  if (n == 0) return MMF_OK;
  if (!multi) {
    MMF_TRY(simtopk_run(r, opts));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return fast_anyk_run(r, opts, info);
}

int mmf_simtopk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                int k, int exclude_self, int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                int device_id, void* hip_stream) {
  return mmf_simtopk_ex(X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset, col_offset, out_idx,
                        out_val, nullptr, nullptr, device_id, hip_stream);
}

int64_t mmf_padded_dim(int64_t d) { return (int64_t)scan_bf16_dp(d); }

int mmf_wide_scan_supported(int64_t d, int k, int exclude_self) {
  if (d < 1 || k < 1) return 0;
  return scan_b16w_supported(d, k + (exclude_self ? 1 : 0));
}

int mmf_wide_scan_list_capacity(int k, int exclude_self) {
  const int kk = k + (exclude_self ? 1 : 0);
  return (k >= 1 && kk <= 20) ? scan_b16w_cap(kk) : 0;
}

int mmf_fast_scan_supported(int64_t d, int k, int exclude_self) {
  if (d < 1 || k < 1) return 0;
  return scan_bf16_supported(d, k + (exclude_self ? 1 : 0), MMF_F32);
}

int mmf_row_scalars(const void* X, int64_t n, int64_t d, int in_dtype, int metric, float* scal, float* max_sq_norm,
                    int device_id, void* hip_stream) {
  Call c("row_scalars", device_id, hip_stream);
  MMF_TRY(check_common(c, X, n, n, d, in_dtype));
  if (metric < MMF_DOT || metric > MMF_RBF) { set_error("row_scalars: bad metric %d", metric); return MMF_E_INVALID; }
  if (n == 0) return MMF_OK;
  if (!scal) { set_error("row_scalars: NULL output"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_row_scalars(X, n, d, in_dtype, metric, scal, reinterpret_cast<uint32_t*>(max_sq_norm), c.s);
}

int mmf_prep_rows(const void* X, int64_t n, int64_t d, int in_dtype, int metric, int operand, const float* scal,
                  const float* max_sq_norm, void* Z, int64_t n_pad, float* zn, float* rn, float* un, float* cb,
                  float* maxima, int device_id, void* hip_stream) {
  Call c("prep_rows", device_id, hip_stream);
  MMF_TRY(check_common(c, X, n, n, d, in_dtype));
  if (metric < MMF_DOT || metric > MMF_RBF) { set_error("prep_rows: bad metric %d", metric); return MMF_E_INVALID; }
  if (operand != MMF_F16 && operand != MMF_BF16) { set_error("prep_rows: operand must be MMF_F16 or MMF_BF16"); return MMF_E_INVALID; }
  const int dp = scan_bf16_dp(d);
  if (dp == 0) { set_error("prep_rows: d = %lld is not supported by the 16-bit scan", (long long)d); return MMF_E_UNSUPPORTED; }
  if (n_pad < n) { set_error("prep_rows: n_pad < n"); return MMF_E_INVALID; }
  if (n_pad == 0) return MMF_OK;
  if (!scal || !Z || !zn || !rn || !un || !cb || !maxima || (metric != MMF_COSINE && !max_sq_norm)) {
    set_error("prep_rows: NULL pointer"); return MMF_E_INVALID;
  }
  MMF_TRY(c.begin());
  const HalfImage out{static_cast<uint16_t*>(Z), zn, rn, un, cb, reinterpret_cast<uint32_t*>(maxima), n_pad};
  return launch_prep_half({X, n, d, in_dtype, metric, scal, reinterpret_cast<const uint32_t*>(max_sq_norm)}, out, dp, operand == MMF_F16, c.s);
}

int mmf_simtopk_prepared(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                         float lambda, int k, int exclude_self, int64_t row_offset, int64_t col_offset,
                         const mmf_prepared_side* q, const mmf_prepared_side* c, int64_t m_pad, const float* maxima,
                         int operand, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                         mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  Request r{Call("simtopk_prepared", device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset,
            col_offset, out_idx, out_val, stats, opts && opts->profile};
  MMF_TRY(r.check(operand == MMF_F16 ? MMF_PREC_FAST : MMF_PREC_FAST_BF16, false, [&] {
    if (!Y || !q || !c || !maxima) { set_error("simtopk_prepared: NULL pointer"); return MMF_E_INVALID; }
    if (operand != MMF_F16 && operand != MMF_BF16) { set_error("simtopk_prepared: bad operand"); return MMF_E_INVALID; }
    if (m_pad < m || (m_pad % 256) != 0) { set_error("simtopk_prepared: m_pad must be a multiple of 256 and >= m"); return MMF_E_INVALID; }
    return MMF_OK;
  }));
  if (n == 0) return MMF_OK;
  FastTail ft(n, m, r.kk, opts ? opts->col_splits : 0, scan_bf16_dp(d));
  MMF_TRY(ft.set_query_order(opts ? opts->query_order : MMF_QUERY_ORDER_AUTO));
  Workspace ws;
  MMF_TRY(r.call.workspace(ft.bytes(), &ws));
  ft.carve(ws);
  FastOperands fo{HalfImage::of(*q, nullptr, ft.n_pad_q()), HalfImage::of(*c, maxima, m_pad), q->scal, c->scal, m_pad, scan_bf16_dp(d),
                  operand == MMF_F16};
  return ft.run(r, fo, opts ? opts->select_wait_event : nullptr);
}

int mmf_simtopk_panels(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                       float lambda, int k, int exclude_self, int64_t row_offset, int64_t col_offset,
                       const mmf_prepared_side* q, const float* c_scal, const mmf_panel* panels, int n_panels,
                       const float* maxima, int operand, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                       mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  Request r{Call("simtopk_panels", device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, row_offset,
            col_offset, out_idx, out_val, stats, opts && opts->profile};
  int64_t m_min = m, m_max = 0;
  MMF_TRY(r.check(operand == MMF_F16 ? MMF_PREC_FAST : MMF_PREC_FAST_BF16, false, [&] {
    if (!Y || !q || !c_scal || !panels || !maxima) { set_error("simtopk_panels: NULL pointer"); return MMF_E_INVALID; }
    if (operand != MMF_F16 && operand != MMF_BF16) { set_error("simtopk_panels: bad operand"); return MMF_E_INVALID; }
    if (n_panels < 1 || n_panels > 16) { set_error("simtopk_panels: n_panels must be in 1..16"); return MMF_E_INVALID; }
    int64_t covered = 0;
    for (int p = 0; p < n_panels; ++p) {
      const mmf_panel& P = panels[p];
      if (!P.Z || !P.cb || P.m < 1 || P.m_pad < P.m || (P.m_pad % 256) != 0 || P.seg_len < 0 || P.id_base < 0 ||
          (P.seg_len > 0 && (P.seg_stride < P.seg_len || (P.m % P.seg_len) != 0))) {
        set_error("simtopk_panels: panel %d is malformed", p); return MMF_E_INVALID;
      }
      const int64_t last = P.seg_len ? P.id_base + (P.m / P.seg_len - 1) * P.seg_stride + P.seg_len - 1 : P.id_base + P.m - 1;
      if (last >= m) { set_error("simtopk_panels: panel %d maps past column %lld", p, (long long)m); return MMF_E_INVALID; }
      covered += P.m;
      if (P.m < m_min) m_min = P.m;
      if (P.m_pad > m_max) m_max = P.m_pad;
    }
    if (covered != m) { set_error("simtopk_panels: panels cover %lld columns, Y has %lld", (long long)covered, (long long)m); return MMF_E_INVALID; }
    return MMF_OK;
  }));
  if (n == 0) return MMF_OK;
  FastTail ft(n, m, r.kk, opts ? opts->col_splits : 0, scan_bf16_dp(d), n_panels, m_min, m_max);
  MMF_TRY(ft.set_query_order(opts ? opts->query_order : MMF_QUERY_ORDER_AUTO));
  if ((int64_t)ft.lists * ft.bcap + kSpillCap > 1024) {
    set_error("simtopk_panels: %d panels x %d-entry lists exceed the 1024 candidates a row can hand to the re-rank (k = %d): use fewer panels", n_panels, ft.bcap, k);
    return MMF_E_UNSUPPORTED;
  }
  Workspace ws;
  MMF_TRY(r.call.workspace(ft.bytes(), &ws));
  ft.carve(ws);
  const HalfImage none = HalfImage::of(mmf_prepared_side{}, maxima, 0);   // the candidate operands are the panels'; the maxima are those of all of them
  FastOperands fo{HalfImage::of(*q, nullptr, ft.n_pad_q()), none, q->scal, c_scal, 0, scan_bf16_dp(d), operand == MMF_F16};
  fo.panels = panels; fo.n_panels = n_panels;
  return ft.run(r, fo, opts ? opts->select_wait_event : nullptr);
}

int mmf_topk_merge(const int64_t* ia, const float* va, const int64_t* ib, const float* vb, int64_t n, int k,
                   int64_t* io, float* vo, int device_id, void* hip_stream) {
  Call c("topk_merge", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || k < 1) { set_error("topk_merge: bad n/k"); return MMF_E_INVALID; }
  if (n == 0) return MMF_OK;
  if (!ia || !va || !ib || !vb || !io || !vo) { set_error("topk_merge: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_topk_merge(ia, va, ib, vb, n, k, io, vo, c.s);
}

int mmf_edge_cosine(const void* X, int64_t n, int64_t d, int in_dtype, const int64_t* edge_index, int64_t E,
                    float* out_w, int device_id, void* hip_stream) {
  Call c("edge_cosine", device_id, hip_stream);
  MMF_TRY(check_common(c, X, n, n, d, in_dtype));
  if (E < 0) { set_error("edge_cosine: E < 0"); return MMF_E_INVALID; }
  if (E == 0) return MMF_OK;
  if (!edge_index || !out_w) { set_error("edge_cosine: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin(ws_bytes(n, 4)));
  float* nrm = c.ws.take<float>(n);
  MMF_TRY(launch_row_scalars(X, n, d, in_dtype, MMF_COSINE, nrm, nullptr, c.s));
  return launch_edge_cosine_impl(X, d, in_dtype, nrm, edge_index, E, out_w, c.s);
}

int mmf_sim_dense(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                  float lambda, float* out, int device_id, void* hip_stream) {
  if (!Y) { Y = X; m = n; }
  Call c("sim_dense", device_id, hip_stream);
  MMF_TRY(check_common(c, X, n, m, d, in_dtype));
  if (metric < MMF_DOT || metric > MMF_RBF_DIRECT) { set_error("sim_dense: bad metric %d", metric); return MMF_E_INVALID; }
  if (n == 0 || m == 0) return MMF_OK;
  if (!out) { set_error("sim_dense: NULL output"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  const bool same = (Y == X) && (m == n);
  float *rx = nullptr, *cy = nullptr, *Xp = nullptr, *Yp = nullptr;
  if (metric != MMF_RBF_DIRECT) {
    const bool img = sim_dense_needs_images(d, metric);
    Workspace ws;
    MMF_TRY(c.workspace(ws_bytes(n, 4) + ws_bytes(m, 4) +
                        (img ? ws_bytes(prep_f32_bytes(m, d), 1) + (same ? 0 : ws_bytes(prep_f32_bytes(n, d), 1)) : 0), &ws));
    rx = ws.take<float>(n);
    cy = same ? rx : ws.take<float>(m);
    MMF_TRY(launch_row_scalars(X, n, d, in_dtype, metric, rx, nullptr, s));
    if (!same) MMF_TRY(launch_row_scalars(Y, m, d, in_dtype, metric, cy, nullptr, s));
    if (img) {
      Yp = reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(m, d)));
      Xp = same ? Yp : reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(n, d)));
      MMF_TRY(launch_prep_f32(Y, m, d, in_dtype, nullptr, Yp, s));
      if (!same) MMF_TRY(launch_prep_f32(X, n, d, in_dtype, nullptr, Xp, s));
    }
  }
  return launch_sim_dense(X, n, Y, m, d, in_dtype, metric, lambda, rx, cy, Xp, Yp, out, s);
}

int mmf_sim_dense_stats(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                        float* out, double* out_stats, int64_t panel_rows, int device_id, void* hip_stream) {
  if (!Y) { Y = X; m = n; }
  Call c("sim_dense_stats", device_id, hip_stream);
  MMF_TRY(check_common(c, X, n, m, d, in_dtype));
  if (metric < MMF_DOT || metric > MMF_RBF_DIRECT) { set_error("sim_dense_stats: bad metric %d", metric); return MMF_E_INVALID; }
  if (n < 1 || m < 1) { set_error("sim_dense_stats: empty matrix"); return MMF_E_INVALID; }
  if (!out_stats) { set_error("sim_dense_stats: NULL out_stats"); return MMF_E_INVALID; }
  if (!out && metric != MMF_RBF_DIRECT) { set_error("sim_dense_stats: out == NULL is supported for MMF_RBF_DIRECT only"); return MMF_E_UNSUPPORTED; }
  const int64_t count = n * m;
  if (metric != MMF_RBF_DIRECT) {        // matrix-core dense kernels, then one reduction pass + the radix select
    MMF_TRY(mmf_sim_dense(X, n, Y, m, d, in_dtype, metric, lambda, out, device_id, hip_stream));
    return mmf_array_stats(out, count, out_stats, device_id, hip_stream);
  }
  int64_t R = n;
  if (!out) {                            // nothing stored: rows recomputed in panels for each radix pass
    R = panel_rows > 0 ? panel_rows : (int64_t(1) << 30) / (4 * m);
    R = (R + 127) / 128 * 128;
    if (R < 128) R = 128;
    if (R > n) R = n;
  }
  int64_t blocks = 0;
  for (int64_t r0 = 0; r0 < n; r0 += R) blocks += rbf_direct_blocks((n - r0 < R) ? (n - r0) : R, m);
  const size_t mneed = median_scratch_bytes((unsigned long long)count);
  MMF_TRY(c.begin(ws_bytes((size_t)blocks * stat_partial_bytes(), 1) + ws_bytes(64, 4) + ws_bytes(mneed, 1) +
                          (out ? 0 : ws_bytes((size_t)R * m, 4))));
  const hipStream_t s = c.s;
  char* part = c.ws.take<char>((size_t)blocks * stat_partial_bytes());
  float* pivot = c.ws.take<float>(64);
  float* med = pivot + 8;
  void* mscratch = c.ws.take<char>(mneed);
  MMF_TRY(launch_rbf_direct_pivot(X, Y, d, in_dtype, lambda, pivot, s));
  if (out) {
    MMF_TRY(launch_rbf_direct(X, n, Y, m, d, in_dtype, lambda, out, part, pivot, s));
    MMF_TRY(launch_lower_median(out, count, med, mscratch, s));
  } else {
    // the matrix is never stored: every sweep of the median recomputes it panel by panel (one sweep when the sampled
    // bracket holds, four radix passes otherwise); the first sweep also leaves the statistic partials
    float* panel = c.ws.take<float>((size_t)R * m);
    bool partials_done = false;
    const MedianSweep sweep = [&](const MedianConsume& consume) -> int {
      int64_t b0 = 0;
      for (int64_t r0 = 0; r0 < n; r0 += R) {
        const int64_t rows = (n - r0 < R) ? (n - r0) : R;
        const void* Xr = static_cast<const char*>(X) + (size_t)r0 * d * dtype_size(in_dtype);
        MMF_TRY(launch_rbf_direct(Xr, rows, Y, m, d, in_dtype, lambda, panel,
                                  partials_done ? nullptr : part + (size_t)b0 * stat_partial_bytes(), pivot, s));
        MMF_TRY(consume(panel, m, median_no_diagonal_row(), rows));
        b0 += rbf_direct_blocks(rows, m);
      }
      partials_done = true;
      return MMF_OK;
    };
    MMF_TRY(lower_median_of((unsigned long long)count,
                            [&](float* sample, int sc) {
                              return launch_sample_pairs(X, Y, m, d, in_dtype, lambda, nullptr, 0, 0.0f, 0, (unsigned long long)count, sample, sc, s);
                            },
                            sweep, med, mscratch, s));
  }
  MMF_TRY(launch_stats_finish(part, blocks, pivot, count, out_stats, s));
  return launch_stats_set_median(med, out_stats, s);
}

int mmf_sim_dense_combined(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                           float lambda_g, float* out, int device_id, void* hip_stream) {
  Call c("sim_dense_combined", device_id, hip_stream);
  MMF_TRY(check_common(c, F, n, n, d, MMF_F32));
  if (dp < 1) { set_error("sim_dense_combined: dp < 1"); return MMF_E_INVALID; }
  if (n == 0) return MMF_OK;
  if (!P || !out) { set_error("sim_dense_combined: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin(ws_bytes(n, 4) + ws_bytes(prep_f32_bytes(n, d), 1)));
  const hipStream_t s = c.s;
  float* nf = c.ws.take<float>(n);
  float* Fp = reinterpret_cast<float*>(c.ws.take<char>(prep_f32_bytes(n, d)));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_prep_f32(F, n, d, MMF_F32, nullptr, Fp, s));
  return launch_sim_dense_combined(Fp, P, n, d, dp, lambda_h, lambda_g, nf, 0, n, out, s);
}

int mmf_offdiag_lower_median(const float* K, int64_t n, float* out_median, int device_id, void* hip_stream) {
  Call c("offdiag_lower_median", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 2) { set_error("offdiag_lower_median: need n >= 2 (got %lld)", (long long)n); return MMF_E_INVALID; }
  if (!K || !out_median) { set_error("offdiag_lower_median: NULL pointer"); return MMF_E_INVALID; }
  const size_t need = median_scratch_bytes((unsigned long long)n * (unsigned long long)(n - 1));
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_offdiag_lower_median(K, n, out_median, c.ws.take<char>(need), c.s);
}

// ---- cluster-shaped steps (mmf_segments.hip) ----------------------------------------------------------------------
static int check_cluster_counts(const Call& c, int64_t n, int64_t S) {
  MMF_TRY(c.on_device());
  if (n < 0 || S < 1) { set_error("%s: bad n / n_segments", c.who); return MMF_E_INVALID; }
  if (S > segment_max_segments()) { set_error("%s: at most %d segments are supported (got %lld)", c.who, segment_max_segments(), (long long)S); return MMF_E_UNSUPPORTED; }
  return MMF_OK;
}

int mmf_segment_sort(const int64_t* labels, int64_t n, int64_t n_segments, int64_t* counts, int64_t* offsets, int64_t* order,
                     int device_id, void* hip_stream) {
  Call c("segment_sort", device_id, hip_stream);
  MMF_TRY(check_cluster_counts(c, n, n_segments));
  if (!counts || !offsets || (n > 0 && (!labels || !order))) { set_error("segment_sort: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  if (n == 0) {
    MMF_HIP(hipMemsetAsync(counts, 0, (size_t)n_segments * 8, s));
    MMF_HIP(hipMemsetAsync(offsets, 0, (size_t)(n_segments + 1) * 8, s));
    return MMF_OK;
  }
  Workspace ws;
  MMF_TRY(c.workspace(ws_bytes(segment_sort_scratch_bytes(n, n_segments), 1) + ws_bytes(4, 4), &ws));
  char* scratch = ws.take<char>(segment_sort_scratch_bytes(n, n_segments));
  uint32_t* bad = ws.take<uint32_t>(4);
  MMF_TRY(launch_segment_sort(labels, n, n_segments, counts, offsets, order, scratch, bad, s));
  uint32_t h_bad = 0;
  MMF_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, s));
  MMF_HIP(hipStreamSynchronize(s));
  if (h_bad) { set_error("segment_sort: %u labels lie outside [0, %lld)", h_bad, (long long)n_segments); return MMF_E_INVALID; }
  return MMF_OK;
}

int mmf_segment_mean(const float* X, int64_t n, int64_t d, const int64_t* order, const int64_t* offsets, int64_t n_segments,
                     float* out, int device_id, void* hip_stream) {
  Call c("segment_mean", device_id, hip_stream);
  MMF_TRY(check_cluster_counts(c, n, n_segments));
  if (d < 1) { set_error("segment_mean: d < 1"); return MMF_E_INVALID; }
  if (!X || !order || !offsets || !out) { set_error("segment_mean: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_segment_mean(X, d, order, offsets, n_segments, out, c.s);
}

int mmf_segment_offdiag_mean(const float* K, int64_t n, const int64_t* order, const int64_t* offsets, int64_t n_segments,
                             double* out_mean, int device_id, void* hip_stream) {
  Call c("segment_offdiag_mean", device_id, hip_stream);
  MMF_TRY(check_cluster_counts(c, n, n_segments));
  if (n < 1 || !K || !order || !offsets || !out_mean) { set_error("segment_offdiag_mean: NULL pointer / empty matrix"); return MMF_E_INVALID; }
  MMF_TRY(c.begin(segment_offdiag_scratch_bytes(n)));
  return launch_segment_offdiag_mean(K, n, order, offsets, n_segments, out_mean, c.ws.take<char>(segment_offdiag_scratch_bytes(n)), c.s);
}

int mmf_clique_pairs(const int64_t* order, const int64_t* offsets, int64_t n, int64_t n_segments, int64_t* pair_lo,
                     int64_t* pair_hi, int64_t capacity, int64_t* out_count, int device_id, void* hip_stream) {
  Call c("clique_pairs", device_id, hip_stream);
  MMF_TRY(check_cluster_counts(c, n, n_segments));
  if (capacity < 0 || !offsets || !out_count || (n > 0 && !order) || (capacity > 0 && (!pair_lo || !pair_hi))) {
    set_error("clique_pairs: NULL pointer / bad capacity"); return MMF_E_INVALID;
  }
  MMF_TRY(c.begin(clique_scratch_bytes(n, n_segments)));
  return launch_clique_pairs(order, offsets, n, n_segments, pair_lo, pair_hi, capacity, out_count,
                             c.ws.take<char>(clique_scratch_bytes(n, n_segments)), c.s);
}

int mmf_knn_pairs(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t* pair_lo, int64_t* pair_hi,
                  int64_t* out_count, int device_id, void* hip_stream) {
  Call c("knn_pairs", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || k < 1) { set_error("knn_pairs: bad n / k"); return MMF_E_INVALID; }
  if (!out_count || (n > 0 && (!nbr || !pair_lo || !pair_hi))) { set_error("knn_pairs: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_knn_pairs(nbr, n, k, labels, pair_lo, pair_hi, out_count, c.s);
}

// both KMeans entries after their own argument checks: the plain fit is the one segment ptr = {0, n}
static int kmeans_fit_run(const float* X, int64_t d, const int64_t* ptr, int64_t n_seg, int64_t k, int64_t n_init, int trials,
                          const int64_t* first_centres, const double* uniforms, int max_iter, double tol, int64_t* labels, float* centres,
                          int64_t* seeds, double* info, bool segmented, Call& c) {
  size_t need = 0;
  const std::vector<int64_t> groups = kmeans_segment_groups(ptr, n_seg, d, k, n_init, trials, &need);
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_kmeans_fit(X, d, ptr, groups, k, n_init, trials, first_centres, uniforms, max_iter, tol, labels, centres, seeds, info,
                           c.ws.take<char>(need), c.s, segmented);
}

int mmf_kmeans_fit(const float* X, int64_t n, int64_t d, int64_t n_clusters, int64_t n_init, int trials, const int64_t* first_centres,
                   const double* uniforms, int max_iter, double tol, int64_t* labels, float* centres, int64_t* seeds, double* info,
                   int device_id, void* hip_stream) {
  Call c("kmeans_fit", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 1 || d < 1 || n_clusters < 1 || n_clusters > n || n_init < 1 || trials < 1 || trials > 64 || max_iter < 1 || !(tol >= 0.0)) {
    set_error("kmeans_fit: need 1 <= n_clusters <= n, n_init >= 1, 1 <= trials <= 64, max_iter >= 1, tol >= 0 (n = %lld, n_clusters = %lld, "
              "n_init = %lld, trials = %d, max_iter = %d)", (long long)n, (long long)n_clusters, (long long)n_init, trials, max_iter);
    return MMF_E_INVALID;
  }
  if (n_init * n_clusters > segment_max_segments()) {
    set_error("kmeans_fit: n_init * n_clusters = %lld above the supported %d", (long long)(n_init * n_clusters), segment_max_segments());
    return MMF_E_UNSUPPORTED;
  }
  if (n_init * n >= ((int64_t)1 << 31)) { set_error("kmeans_fit: n_init * n must be < 2^31"); return MMF_E_UNSUPPORTED; }
  if (!X || !first_centres || (n_clusters > 1 && !uniforms) || !labels) { set_error("kmeans_fit: NULL pointer"); return MMF_E_INVALID; }
  for (int64_t i = 0; i < n_init; ++i)
    if (first_centres[i] < 0 || first_centres[i] >= n) { set_error("kmeans_fit: first_centres[%lld] outside [0, n)", (long long)i); return MMF_E_INVALID; }
  const int64_t ptr[2] = {0, n};
  return kmeans_fit_run(X, d, ptr, 1, n_clusters, n_init, trials, first_centres, uniforms, max_iter, tol, labels, centres, seeds, info, false, c);
}

int mmf_kmeans_fit_segmented(const float* X, int64_t n, int64_t d, const int64_t* ptr, int64_t n_seg, int64_t n_clusters, int64_t n_init,
                             int trials, const int64_t* first_centres, const double* uniforms, int max_iter, double tol, int64_t* labels,
                             float* centres, int64_t* seeds, double* info, int device_id, void* hip_stream) {
  Call c("kmeans_fit_segmented", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 1 || d < 1 || n_seg < 1 || n_clusters < 1 || n_init < 1 || trials < 1 || max_iter < 1 || !(tol >= 0.0)) {
    set_error("kmeans_fit_segmented: need n >= 1, d >= 1, n_seg >= 1, n_clusters >= 1, n_init >= 1, trials >= 1, max_iter >= 1, tol >= 0 "
              "(n = %lld, d = %lld, n_seg = %lld, n_clusters = %lld, n_init = %lld, trials = %d, max_iter = %d)", (long long)n, (long long)d,
              (long long)n_seg, (long long)n_clusters, (long long)n_init, trials, max_iter);
    return MMF_E_INVALID;
  }
  if (!X || !ptr || !first_centres || (n_clusters > 1 && !uniforms) || !labels) { set_error("kmeans_fit_segmented: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(c.who, "ptr", ptr, n_seg, 1, 0, n));
  for (int64_t s = 0; s < n_seg; ++s) {   // scikit-learn's sentence, not the shared one
    const int64_t ns = ptr[s + 1] - ptr[s];
    if (ns < n_clusters) {
      set_error("kmeans_fit_segmented: segment %lld: n_samples=%lld should be >= n_clusters=%lld.", (long long)s, (long long)ns, (long long)n_clusters);
      return MMF_E_INVALID;
    }
  }
  // the plain entry's limits, per segment
  if (n_init * n_clusters > segment_max_segments()) {
    set_error("kmeans_fit_segmented: n_init * n_clusters = %lld above the supported %d", (long long)(n_init * n_clusters), segment_max_segments());
    return MMF_E_UNSUPPORTED;
  }
  if (trials > 64) { set_error("kmeans_fit_segmented: trials = %d above the supported 64", trials); return MMF_E_UNSUPPORTED; }
  for (int64_t s = 0; s < n_seg; ++s)
    if (n_init * (ptr[s + 1] - ptr[s]) >= ((int64_t)1 << 31)) {
      set_error("kmeans_fit_segmented: segment %lld: n_init * n_samples must be < 2^31", (long long)s);
      return MMF_E_UNSUPPORTED;
    }
  for (int64_t s = 0; s < n_seg; ++s)
    for (int64_t i = 0; i < n_init; ++i) {
      const int64_t f = first_centres[s * n_init + i];
      if (f < 0 || f >= ptr[s + 1] - ptr[s]) {
        set_error("kmeans_fit_segmented: segment %lld: first_centres[%lld] outside [0, n_samples)", (long long)s, (long long)i);
        return MMF_E_INVALID;
      }
    }
  return kmeans_fit_run(X, d, ptr, n_seg, n_clusters, n_init, trials, first_centres, uniforms, max_iter, tol, labels, centres, seeds, info, true, c);
}

// ---- ragged-width segmented KMeans (include/ext/mmf_hg_kmeans_ragged.h) --------------------------------
// the checks both entries share: the shapes of the table and the limits one segment alone can break
static int kmeans_ragged_check(const char* who, const int64_t* rows, const int64_t* width, int64_t n_seg, int64_t n_clusters, int64_t n_init,
                               int trials) {
  if (n_seg < 1 || n_clusters < 1 || n_init < 1 || trials < 1) {
    set_error("%s: need n_seg >= 1, n_clusters >= 1, n_init >= 1, trials >= 1 (n_seg = %lld, n_clusters = %lld, n_init = %lld, trials = %d)", who,
              (long long)n_seg, (long long)n_clusters, (long long)n_init, trials);
    return MMF_E_INVALID;
  }
  if (!rows || !width) { set_error("%s: NULL pointer", who); return MMF_E_INVALID; }
  for (int64_t s = 0; s < n_seg; ++s) {
    if (rows[s] < n_clusters) {      // scikit-learn's sentence
      set_error("%s: segment %lld: n_samples=%lld should be >= n_clusters=%lld.", who, (long long)s, (long long)rows[s], (long long)n_clusters);
      return MMF_E_INVALID;
    }
    if (width[s] < 1) { set_error("%s: segment %lld: width %lld must be >= 1", who, (long long)s, (long long)width[s]); return MMF_E_INVALID; }
  }
  if (n_init * n_clusters > segment_max_segments()) {
    set_error("%s: n_init * n_clusters = %lld above the supported %d", who, (long long)(n_init * n_clusters), segment_max_segments());
    return MMF_E_UNSUPPORTED;
  }
  if (trials > 64) { set_error("%s: trials = %d above the supported 64", who, trials); return MMF_E_UNSUPPORTED; }
  for (int64_t s = 0; s < n_seg; ++s)
    if (n_init * rows[s] >= ((int64_t)1 << 31)) {
      set_error("%s: segment %lld: n_init * n_samples must be < 2^31", who, (long long)s);
      return MMF_E_UNSUPPORTED;
    }
  return MMF_OK;
}

int mmf_kmeans_fit_ragged(const float* V, int64_t n_values, const int64_t* xoff, const int64_t* rows, const int64_t* width, int64_t n_seg,
                          int64_t n_clusters, int64_t n_init, int trials, const int64_t* first_centres, const double* uniforms, int max_iter,
                          double tol, int64_t* labels, float* centres, int64_t* seeds, double* info, int device_id, void* hip_stream) {
  Call c("kmeans_fit_ragged", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (max_iter < 1 || !(tol >= 0.0)) { set_error("kmeans_fit_ragged: need max_iter >= 1, tol >= 0 (max_iter = %d)", max_iter); return MMF_E_INVALID; }
  if (!V || !xoff || !first_centres || (n_clusters > 1 && !uniforms) || !labels) { set_error("kmeans_fit_ragged: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(kmeans_ragged_check(c.who, rows, width, n_seg, n_clusters, n_init, trials));
  for (int64_t s = 0; s < n_seg; ++s) {
    // (rows < 2^31 / n_init was checked; the product is taken in 128 bits against a width near 2^63)
    if (xoff[s] < 0 || (__int128)xoff[s] + (__int128)rows[s] * width[s] > (__int128)n_values) {
      set_error("kmeans_fit_ragged: segment %lld: block [%lld, %lld + %lld x %lld) outside the %lld values of V", (long long)s, (long long)xoff[s],
                (long long)xoff[s], (long long)rows[s], (long long)width[s], (long long)n_values);
      return MMF_E_INVALID;
    }
    for (int64_t i = 0; i < n_init; ++i) {
      const int64_t f = first_centres[s * n_init + i];
      if (f < 0 || f >= rows[s]) {
        set_error("kmeans_fit_ragged: segment %lld: first_centres[%lld] outside [0, n_samples)", (long long)s, (long long)i);
        return MMF_E_INVALID;
      }
    }
  }
  size_t need = 0;
  const std::vector<int64_t> groups = kmeans_ragged_groups(rows, width, n_seg, n_clusters, n_init, trials, &need, nullptr);
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_kmeans_fit_ragged(V, xoff, rows, width, groups, n_clusters, n_init, trials, first_centres, uniforms, max_iter, tol, labels, centres,
                                  seeds, info, c.ws.take<char>(need), c.s);
}

int64_t mmf_kmeans_ragged_groups(const int64_t* rows, const int64_t* width, int64_t n_seg, int64_t n_clusters, int64_t n_init, int trials,
                                 int64_t* bounds, int64_t* ds) {
  const int rc = kmeans_ragged_check("kmeans_ragged_groups", rows, width, n_seg, n_clusters, n_init, trials);
  if (rc != MMF_OK) return rc;
  if (!bounds) { set_error("kmeans_ragged_groups: NULL pointer"); return MMF_E_INVALID; }
  const std::vector<int64_t> b = kmeans_ragged_groups(rows, width, n_seg, n_clusters, n_init, trials, nullptr, ds);
  for (size_t i = 0; i < b.size(); ++i) bounds[i] = b[i];
  return (int64_t)b.size() - 1;
}

int mmf_lower_median(const float* v, int64_t count, float* out_median, int device_id, void* hip_stream) {
  Call c("lower_median", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (count < 1) { set_error("lower_median: need count >= 1 (got %lld)", (long long)count); return MMF_E_INVALID; }
  if (!v || !out_median) { set_error("lower_median: NULL pointer"); return MMF_E_INVALID; }
  const size_t need = median_scratch_bytes((unsigned long long)count);
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_lower_median(v, count, out_median, c.ws.take<char>(need), c.s);
}

int mmf_array_stats(const float* v, int64_t count, double* out_stats, int device_id, void* hip_stream) {
  Call c("array_stats", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (count < 1) { set_error("array_stats: need count >= 1 (got %lld)", (long long)count); return MMF_E_INVALID; }
  if (!v || !out_stats) { set_error("array_stats: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin(ws_bytes(array_stats_scratch_bytes(count), 1)));
  return launch_array_stats(v, count, out_stats, c.ws.take<char>(array_stats_scratch_bytes(count)), c.s);
}

int mmf_threshold_edges(const float* K, int64_t n, float threshold, int64_t* edge_index, float* edge_w,
                        int64_t capacity, int64_t* out_count, int device_id, void* hip_stream) {
  Call c("threshold_edges", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || capacity < 0) { set_error("threshold_edges: bad n/capacity"); return MMF_E_INVALID; }
  if (!out_count) { set_error("threshold_edges: NULL out_count"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  MMF_HIP(hipMemsetAsync(out_count, 0, 8, c.s));
  if (n == 0) return MMF_OK;
  if (!K || (capacity > 0 && (!edge_index || !edge_w))) { set_error("threshold_edges: NULL pointer"); return MMF_E_INVALID; }
  const size_t rows_u32 = (size_t)n * 2 + 64;
  Workspace ws;
  MMF_TRY(c.workspace(ws_bytes(rows_u32, 8), &ws));
  return launch_threshold_edges(K, n, threshold, edge_index, edge_w, capacity, out_count,
                                reinterpret_cast<uint32_t*>(ws.take<uint64_t>(rows_u32)), rows_u32 * 2, c.s);
}

int mmf_threshold_edges_count(const float* K, int64_t n, float threshold, uint64_t* row_offsets, int64_t* out_count, int device_id,
                              void* hip_stream) {
  Call c("threshold_edges_count", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0) { set_error("threshold_edges_count: bad n"); return MMF_E_INVALID; }
  if (!out_count || !row_offsets) { set_error("threshold_edges_count: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  MMF_HIP(hipMemsetAsync(out_count, 0, 8, s));
  if (n == 0) { MMF_HIP(hipMemsetAsync(row_offsets, 0, 8, s)); return MMF_OK; }
  if (!K) { set_error("threshold_edges_count: NULL pointer"); return MMF_E_INVALID; }
  Workspace ws;
  MMF_TRY(c.workspace(ws_bytes((size_t)n, 4), &ws));
  return launch_threshold_count(K, n, threshold, reinterpret_cast<unsigned long long*>(row_offsets), out_count, ws.take<uint32_t>((size_t)n), s);
}

int mmf_threshold_edges_fill(const float* K, int64_t n, float threshold, const uint64_t* row_offsets, int64_t* edge_index, float* edge_w,
                             int64_t capacity, int device_id, void* hip_stream) {
  Call c("threshold_edges_fill", device_id, hip_stream);
  MMF_TRY(c.on_device());
  if (n < 0 || capacity < 0) { set_error("threshold_edges_fill: bad n/capacity"); return MMF_E_INVALID; }
  if (n == 0 || capacity == 0) return MMF_OK;
  if (!K || !row_offsets || !edge_index || !edge_w) { set_error("threshold_edges_fill: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  return launch_threshold_fill(K, n, threshold, reinterpret_cast<const unsigned long long*>(row_offsets), edge_index, edge_w, capacity, c.s);
}

// ---- the same two steps for an N whose K = K_h * K_g does not fit: K is recomputed in row panels -----------------

int mmf_combined_offdiag_median(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                float lambda_g, int64_t panel_rows, float* out_median, int device_id, void* hip_stream) {
  Call c("combined_offdiag_median", device_id, hip_stream);
  MMF_TRY(check_common(c, F, n, n, d, MMF_F32));
  if (dp < 1 || n < 2) { set_error("combined_offdiag_median: need dp >= 1 and n >= 2"); return MMF_E_INVALID; }
  if (!P || !out_median) { set_error("combined_offdiag_median: NULL pointer"); return MMF_E_INVALID; }
  const int64_t R = pick_panel_rows(n, panel_rows);
  const unsigned long long count = (unsigned long long)n * (unsigned long long)(n - 1);
  const size_t mneed = median_scratch_bytes(count);
  MMF_TRY(c.begin(ws_bytes(n, 4) + ws_bytes((size_t)R * n, 4) + ws_bytes(mneed, 1) + ws_bytes(prep_f32_bytes(n, d), 1)));
  const hipStream_t s = c.s;
  float* nf = c.ws.take<float>(n);
  float* Kp = c.ws.take<float>((size_t)R * n);
  void* mscratch = c.ws.take<char>(mneed);
  float* Fp = reinterpret_cast<float*>(c.ws.take<char>(prep_f32_bytes(n, d)));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_prep_f32(F, n, d, MMF_F32, nullptr, Fp, s));
  // one sweep over the recomputed matrix when the sampled bracket holds (four otherwise)
  return lower_median_of(
      count,
      [&](float* sample, int sc) { return launch_sample_pairs(F, F, n, d, MMF_F32, lambda_h, P, (int)dp, lambda_g, 1, count, sample, sc, s); },
      [&](const MedianConsume& consume) -> int {
        for (int64_t r0 = 0; r0 < n; r0 += R) {
          const int64_t rows = (n - r0 < R) ? (n - r0) : R;
          MMF_TRY(launch_sim_dense_combined(Fp, P, n, d, dp, lambda_h, lambda_g, nf, r0, rows, Kp, s));
          MMF_TRY(consume(Kp, n, r0, rows));
        }
        return MMF_OK;
      },
      out_median, mscratch, s);
}

int mmf_combined_threshold_edges(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                 float lambda_g, float threshold, int64_t panel_rows, int64_t* edge_index, float* edge_w,
                                 int64_t capacity, int64_t* out_count, int device_id, void* hip_stream) {
  Call c("combined_threshold_edges", device_id, hip_stream);
  MMF_TRY(check_common(c, F, n, n, d, MMF_F32));
  if (dp < 1 || capacity < 0) { set_error("combined_threshold_edges: bad dp / capacity"); return MMF_E_INVALID; }
  if (!out_count) { set_error("combined_threshold_edges: NULL out_count"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  MMF_HIP(hipMemsetAsync(out_count, 0, 8, s));
  if (n == 0) return MMF_OK;
  if (!P || (capacity > 0 && (!edge_index || !edge_w))) { set_error("combined_threshold_edges: NULL pointer"); return MMF_E_INVALID; }
  const int64_t R = pick_panel_rows(n, panel_rows);
  const size_t rows_u32 = (size_t)R * 2 + 64;
  Workspace ws;
  MMF_TRY(c.workspace(ws_bytes(n, 4) + ws_bytes((size_t)R * n, 4) + ws_bytes(rows_u32, 8) + ws_bytes(prep_f32_bytes(n, d), 1), &ws));
  float* nf = ws.take<float>(n);
  float* Kp = ws.take<float>((size_t)R * n);
  uint32_t* scratch = reinterpret_cast<uint32_t*>(ws.take<uint64_t>(rows_u32));
  float* Fp = reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(n, d)));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_prep_f32(F, n, d, MMF_F32, nullptr, Fp, s));
  for (int64_t r0 = 0; r0 < n; r0 += R) {            // panels in row order: the running count keeps the edges row-major
    const int64_t rows = (n - r0 < R) ? (n - r0) : R;
    MMF_TRY(launch_sim_dense_combined(Fp, P, n, d, dp, lambda_h, lambda_g, nf, r0, rows, Kp, s));
    MMF_TRY(launch_threshold_edges_panel(Kp, n, r0, rows, threshold, edge_index, edge_index ? edge_index + capacity : nullptr,
                                         edge_w, capacity, out_count, scratch, rows_u32 * 2, s));
  }
  return MMF_OK;
}

// ---- segmented simtopk (block-diagonal k-NN over a ragged batch) ------------------------------------------------
// DESIGN.md §4.7.  One call: row scalars, a segment-padded 16-bit image of each side (gathered prep), ONE scan launch
// driven by a host-built work table (a workgroup = one row block of one segment against that segment's tiles), the
// audit and the exact re-rank over all rows, then one host synchronisation.  Rows the 16-bit path cannot certify, and
// every row of a segment with fewer than k admissible columns (or of every segment under MMF_PREC_EXACT), go through the
// exact pass (ExactPass) segment by segment: two launches per segment, not a work table ("Exact rows").
//
// One body for mmf_simtopk_segmented (`who` "simtopk_segmented", wide_allowed false) and mmf_simtopk_segmented_wide
// (include/mmf_hg_wide_seg.h).  wide_allowed: for 1024 < d <= 4096, k + self <= 20 the 16-bit candidates come
// from the wide scan (launch_scan_b16w_seg) — 128-row tiles on both sides, its list capacity, no id scratch, column splits per
// segment — and MMF_PREC_AUTO takes it; everything around the scan launch is the narrow path's.  The body keeps the name of
// the entry it was written for: mmf::mmf_simtopk_segmented(who, wide_allowed, ...) is the overload the two C entries call.
}  // extern "C"

namespace mmf {

int mmf_simtopk_segmented(const char* who, bool wide_allowed, const void* X, int64_t n, const void* Y, int64_t m, int64_t d,
                          int in_dtype, int metric, float lambda, int k, int exclude_self, const int64_t* x_ptr_host,
                          const int64_t* y_ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                          const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.wide_ok = wide_allowed;
  const int prec_asked = opts ? opts->precision : MMF_PREC_AUTO;
  MMF_TRY(r.check(prec_asked, true, [&] {
    MMF_TRY(check_offsets(r.call.who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(r.call.who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    // (lifting this is a matter of letting the exact pass take such segments: it runs the passes k + self > 44 needs)
    if (r.kk > 44) { set_error("%s: k + self = %d > 44 is not supported", who, r.kk); return MMF_E_UNSUPPORTED; }
    // the shapes the wide scan serves take col_splits (0 or a power of two); everywhere else the options are the narrow entry's
    const bool wide_shape = wide_allowed && prec_asked != MMF_PREC_EXACT && scan_b16w_supported(d, r.kk);
    if (wide_shape) {
      if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
      const int cs = opts ? opts->col_splits : 0;
      if (cs < 0 || (cs & (cs - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, cs); return MMF_E_INVALID; }
    } else if (opts && (opts->col_splits != 0 || opts->select_wait_event)) {
      set_error("%s: col_splits and select_wait_event are not supported", who);
      return MMF_E_UNSUPPORTED;
    }
    // the wide entry settles the precision before any device call (Request::check repeats this behind Call::begin)
    if (wide_allowed && (prec_asked == MMF_PREC_FAST || prec_asked == MMF_PREC_FAST_BF16) && !scan_bf16_supported(d, r.kk, in_dtype) &&
        !scan_b16w_supported(d, r.kk)) {
      set_error("%s: MMF_PREC_FAST does not support d = %lld, k = %d (AUTO takes the exact scan there)", who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }));
  if (stats) stats->near_rows = -1;   // the query order is never probed here
  if (n == 0) return MMF_OK;
  const hipStream_t s = r.call.s;
  const int precision = r.precision;
  const bool profile = r.profile;
  const int64_t S = n_segments;
  const int64_t* xp = x_ptr_host;
  const int64_t* yp = y_ptr_host;
  std::vector<int64_t> adm(S);
  for (int64_t g = 0; g < S; ++g) adm[g] = admissible_columns(xp[g], xp[g + 1] - xp[g], yp[g], yp[g + 1] - yp[g], exclude_self);
  const bool fast = precision != MMF_PREC_EXACT;
  const bool wide = r.wide;                       // the 16-bit scan of this call is the wide one (wide_allowed entries only)
  const int dp = !fast ? 0 : wide ? scan_b16w_dp(d) : scan_bf16_dp(d);
  const int qt = !fast ? 1 : wide ? scan_b16w_queries_per_block() : scan_b16_queries_per_block(dp);
  const int kTile = wide ? scan_b16w_col_tile() : 32;   // candidate rows per tile of the 16-bit scan (W_CT / B_CT)
  const int bcap = !fast ? 0 : wide ? scan_b16w_cap(r.kk) : scan_bf16_cap(r.kk, dp);
  // Column ranges per segment (wide only): FastTail's rule applied to the call — with R row blocks over the
  // served segments, double while R x splits < 256 and select's capacity per row holds 2 x splits lists; a forced value takes
  // the same bound; each segment caps its count at its own tile count, rounded down to a power of two.
  int call_splits = 1, max_splits = 1;
  if (wide) {
    int64_t R = 0;
    for (int64_t g = 0; g < S; ++g)
      if (xp[g + 1] > xp[g] && adm[g] >= k) R += (xp[g + 1] - xp[g] + qt - 1) / qt;
    const int forced = opts ? opts->col_splits : 0;
    const auto fits = [&](int sp) { return 2 * sp * bcap <= 1024 - kSpillCap; };
    if (forced > 0) { while (call_splits < forced && fits(2 * call_splits)) call_splits <<= 1; }
    else if (wide_seg_auto_splits()) { while (R > 0 && R * call_splits < 256 && fits(2 * call_splits)) call_splits <<= 1; }
  }
  // segments the 16-bit scan serves: rows present and at least k admissible columns (the others are done exactly)
  std::vector<char> on_fast(S, 0);
  int64_t nq_pos = 0, mc_pos = 0;
  std::vector<int32_t> sched;
  if (fast) {
    for (int64_t g = 0; g < S; ++g) {
      const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
      if (ng == 0 || adm[g] < k) continue;
      const int64_t tiles = (mg + kTile - 1) / kTile;
      // 32-bit offsets of the tile DMA (the wide kernel moves a tile through the buffer base: no such limit)
      if (!wide && tiles * kTile * (int64_t)dp * 2 >= (int64_t(1) << 32)) {
        set_error("%s: segment %lld has %lld candidate rows, over 4 GiB of 16-bit operands", who, (long long)g, (long long)mg);
        return MMF_E_UNSUPPORTED;
      }
      on_fast[g] = 1;
      const int64_t t0 = mc_pos / kTile;
      int sp = 1;                                   // column ranges of this segment: one table entry and one list pair each
      while (2 * sp <= call_splits && 2 * sp <= tiles) sp <<= 1;
      if (sp > max_splits) max_splits = sp;
      const int64_t tps = (tiles + sp - 1) / sp;
      for (int64_t b = 0; b < ng; b += qt) {
        for (int c = 0; c < sp; ++c) {
          const int64_t tb = std::min(t0 + c * tps, t0 + tiles), te = std::min(tb + tps, t0 + tiles);
          const int32_t e[8] = {(int32_t)(nq_pos + b), (int32_t)(xp[g] + b), (int32_t)(ng - b < qt ? ng - b : qt), (int32_t)tb,
                                (int32_t)te, (int32_t)(uint32_t)(yp[g] - t0 * kTile), 2 * c, 0};
          sched.insert(sched.end(), e, e + 8);
        }
      }
      nq_pos += (ng + qt - 1) / qt * qt;
      mc_pos += tiles * kTile;
    }
    if (nq_pos >= (int64_t(1) << 31) || mc_pos >= (int64_t(1) << 31)) { set_error("%s: padded images too large", who); return MMF_E_UNSUPPORTED; }
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  std::vector<int32_t> qgather(nq_pos, -1), cgather(mc_pos, -1);
  {
    int64_t qpos = 0, cpos = 0;
    for (int64_t g = 0; g < S && grid > 0; ++g) {
      if (!on_fast[g]) continue;
      const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
      for (int64_t i = 0; i < ng; ++i) qgather[qpos + i] = (int32_t)(xp[g] + i);
      for (int64_t j = 0; j < mg; ++j) cgather[cpos + j] = (int32_t)(yp[g] + j);
      qpos += (ng + qt - 1) / qt * qt;
      cpos += (mg + kTile - 1) / kTile * kTile;
    }
  }

  // ---- workspace (slot 0): row scalars, the 16-bit images, tables, lists -------------------------------------------
  const int64_t nq_pad = (nq_pos + 255) / 256 * 256, mc_pad = (mc_pos + 255) / 256 * 256;
  const int lists = 2 * max_splits;               // per row; narrow scan: one pair
  const size_t scratch_bytes = wide ? 256 : scan_b16_seg_scratch_bytes(grid, dp, bcap);   // the wide kernel keeps no id scratch
  const int64_t n_seed = n;
  size_t need = ws_bytes(n, 4) + ws_bytes(m, 4) + FlagBlock::bytes(n);
  if (grid > 0)
    need += HalfImage::bytes(nq_pad, dp) + HalfImage::bytes(mc_pad, dp) + ws_bytes(4, 4) + ws_bytes(sched.size(), 4) +
            ws_bytes(nq_pos, 4) + ws_bytes(mc_pos, 4) + b16_lists_bytes(n, lists, bcap) +
            ws_bytes(scratch_bytes, 1) + ws_bytes(2 * (size_t)n_seed, 4) + ws_bytes(select_order_bytes(n), 1);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = self ? rx : ws.take<float>(m);
  FlagBlock flags;
  flags.carve(ws, n);
  MMF_TRY(flags.zero(s));

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  uint32_t* max_n = nullptr;
  if (grid > 0) { max_n = ws.take<uint32_t>(4); MMF_HIP(hipMemsetAsync(max_n, 0, 16, s)); }
  MMF_TRY(launch_row_scalars(X, n, d, in_dtype, metric, rx, max_n, s));
  if (!self && m > 0) MMF_TRY(launch_row_scalars(Y, m, d, in_dtype, metric, cy, max_n, s));

  const uint32_t* h_fail4 = flags.h_fail4;
  std::vector<int32_t> h_fail_rows;
  if (grid > 0) {
    const bool f16 = (precision == MMF_PREC_FAST);
    HalfImage Q, C;
    Q.carve(ws, nq_pad, dp);
    C.carve(ws, mc_pad, dp);
    int32_t* d_sched = ws.take<int32_t>(sched.size());
    int32_t* d_qg = ws.take<int32_t>(nq_pos);
    int32_t* d_cg = ws.take<int32_t>(mc_pos);
    const CandLists L = carve_b16_lists(ws, n, lists, bcap);
    char* scan_scratch = ws.take<char>(scratch_bytes);
    int32_t* seed = ws.take<int32_t>(2 * (size_t)n_seed);
    char* order_scratch = ws.take<char>(select_order_bytes(n));
    MMF_HIP(hipMemcpyAsync(d_sched, sched.data(), sched.size() * 4, hipMemcpyHostToDevice, s));
    MMF_HIP(hipMemcpyAsync(d_qg, qgather.data(), (size_t)nq_pos * 4, hipMemcpyHostToDevice, s));
    MMF_HIP(hipMemcpyAsync(d_cg, cgather.data(), (size_t)mc_pos * 4, hipMemcpyHostToDevice, s));
    MMF_HIP(hipMemsetAsync(Q.maxima, 0, 16, s));
    MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
    MMF_TRY(launch_prep_half_gather({Y, m, d, in_dtype, metric, cy, max_n}, d_cg, mc_pos, C, dp, f16, s));
    MMF_TRY(launch_prep_half_gather({X, n, d, in_dtype, metric, rx, max_n}, d_qg, nq_pos, Q, dp, f16, s));
    MMF_TRY(t_prep.stop(s));

    // rows of segments the scan does not serve keep empty lists: the re-rank reports them, the exact pass below redoes them
    MMF_HIP(hipMemsetAsync(L.cnt, 0, (size_t)n * lists * 4, s));
    MMF_HIP(hipMemsetAsync(L.overflow, 0, (size_t)n * 4, s));
    MMF_HIP(hipMemsetAsync(L.spill_cnt, 0, (size_t)n * 4, s));
    MMF_HIP(hipMemsetAsync(seed, 0x80, (size_t)n_seed * 8, s));
    ScanB16Panel pn;
    pn.seed = seed; pn.seed_stride = n_seed; pn.share = 0;
    MMF_TRY(t_scan.start(profile, s));
    const ScanB16Problem sp(Q, C, n, m, mc_pad, dp, d, f16, metric, r.kk);
    if (wide) MMF_TRY(launch_scan_b16w_seg(sp, d_sched, grid, lists, L, pn, s));
    else MMF_TRY(launch_scan_b16_seg(sp, d_sched, grid, L, scan_scratch, pn, s));
    MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
    MMF_TRY(t_scan.stop(s));

    SelectProblem q = r.select();
    q.rx = rx; q.cy = cy;
    q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = stats ? flags.cand_total : nullptr;
    q.two_pass = true;
    q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
    MMF_TRY(t_sel.start(profile, s));
    MMF_TRY(launch_select(q, L, s));
    MMF_TRY(t_sel.stop(s));
    MMF_TRY(flags.read(stats != nullptr, s));
    h_fail_rows.resize(h_fail4[0]);
    if (h_fail4[0] > 0) MMF_HIP(hipMemcpy(h_fail_rows.data(), flags.fail_rows, (size_t)h_fail4[0] * 4, hipMemcpyDeviceToHost));
  } else {
    MMF_TRY(t_prep.stop(s));
  }

  // ---- exact pass: per segment, the rows the scan did not certify or did not serve ----------------------------------
  // whole segments (short of admissible columns, or every segment under MMF_PREC_EXACT) as slices of X and Y; the rows
  // the 16-bit path flagged gathered per segment
  ExactPass ex(r, rx, cy);
  ex.same = self;
  std::vector<int32_t> ex_rows;   // flagged rows of the segments the scan served, ascending: grouped by segment
  for (int32_t row : h_fail_rows) {
    const int64_t g = (int64_t)(std::upper_bound(xp, xp + S + 1, (int64_t)row) - xp) - 1;
    if (g >= 0 && g < S && on_fast[g]) ex_rows.push_back(row);
  }
  std::sort(ex_rows.begin(), ex_rows.end());
  const int64_t fallback_rows = (int64_t)ex_rows.size();
  for (int64_t g = 0, e = 0; g < S; ++g) {
    const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g], e0 = e;
    if (on_fast[g]) {
      while (e < fallback_rows && ex_rows[e] < xp[g + 1]) ++e;
      if (e > e0) ex.add(ExactGroup{e0, e - e0, true, yp[g], mg, k});
    } else if (ng > 0) {
      int ks = k;
      if (adm[g] < k) {   // a segment short of admissible columns: its top-(m_g - self) first, then -1 / -inf
        MMF_HIP(hipMemsetAsync(out_idx + xp[g] * k, 0xff, (size_t)ng * k * 8, s));
        MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_val + xp[g] * k), (int)0xff800000u, (size_t)ng * k, s));
        ks = (int)(adm[g] > 0 ? adm[g] : 0);
      }
      if (ks > 0) ex.add(ExactGroup{xp[g], ng, false, yp[g], mg, ks});
    }
  }
  MMF_TRY(t_fb.start(profile && !ex.pieces.empty(), s));
  if (!ex.pieces.empty()) {   // lists and f32 images in the second workspace slot
    ex.n_ids = fallback_rows;
    Workspace aux;
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes() + ws_bytes(ex.n_ids, 4), &aux, 1));
    int32_t* d_rows = aux.take<int32_t>(ex.n_ids);
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), false);
    ex.row_ids = d_rows;
    if (ex.n_ids > 0) MMF_HIP(hipMemcpyAsync(d_rows, ex_rows.data(), (size_t)ex.n_ids * 4, hipMemcpyHostToDevice, s));
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
  }
  MMF_TRY(t_fb.stop(s));
  MMF_HIP(hipStreamSynchronize(s));
  const int64_t overflow_rows = h_fail4[1] < (uint32_t)fallback_rows ? h_fail4[1] : fallback_rows;
  fill_stats(stats, grid > 0 ? precision : MMF_PREC_EXACT, max_splits, grid > 0 ? (int)grid : ex.grid, t_prep.ms(),
             grid > 0 ? t_scan.ms() : t_fb.ms(), t_sel.ms(), grid > 0 ? t_fb.ms() : 0.f, fallback_rows, overflow_rows,
             fallback_rows - overflow_rows, flags.h_tot);
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

int mmf_simtopk_segmented(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                          float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                          int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                          mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  return mmf::mmf_simtopk_segmented("simtopk_segmented", false, X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, x_ptr_host,
                                    y_ptr_host, n_segments, out_idx, out_val, opts, stats, device_id, hip_stream);
}

// include/mmf_hg_wide_seg.h, DESIGN.md §4.16
int mmf_simtopk_segmented_wide(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                               float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                               int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                               mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  return mmf::mmf_simtopk_segmented("simtopk_segmented_wide", true, X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, x_ptr_host,
                                    y_ptr_host, n_segments, out_idx, out_val, opts, stats, device_id, hip_stream);
}


// ---- segmented weighted hypergraph (the blocks K_s of a ragged batch) -------------------------------------------
// DESIGN.md §4.9.  Segment s is rows ptr[s] .. ptr[s+1]-1 (host int64 offsets); its block K_s (n_s x n_s, row-major) sits at
// kptr[s] = sum_{t<s} n_t^2 of one flat f32 buffer.  Every argument is checked here, before any device work.
// n < 2^31 keeps sum n_s^2 <= n^2 below 2^62: every block offset fits int64
static int check_block_rows(const char* who, int64_t n) {
  if (n >= ((int64_t)1 << 31)) { set_error("%s: %lld rows, must be < 2^31", who, (long long)n); return MMF_E_UNSUPPORTED; }
  return MMF_OK;
}

static std::vector<int64_t> block_offsets(const int64_t* ptr, int64_t n_seg) {
  std::vector<int64_t> kptr((size_t)n_seg + 1, 0);
  for (int64_t g = 0; g < n_seg; ++g) kptr[g + 1] = kptr[g] + (ptr[g + 1] - ptr[g]) * (ptr[g + 1] - ptr[g]);
  return kptr;
}

// compute_combined_similarity of every segment (build_hypergraph/similarity_kernel.py:88-124; :171 inside
// build_weighted_hypergraph, and the K_wsi of every slide, preprocess_hypergraph.py:136-138): row scalars and the f32 image of all n rows, then ONE scan launch over a host-built work
// table (mmf_scan_f32.hip, SEG).  Block s is bit for bit mmf_sim_dense_combined(F_s, P_s).
int mmf_sim_dense_combined_segmented(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, const int64_t* ptr_host,
                                     int64_t n_seg, float lambda_h, float lambda_g, float* out, int device_id, void* hip_stream) {
  Call c("sim_dense_combined_segmented", device_id, hip_stream);
  MMF_TRY(check_common(c, F, n, n, d, MMF_F32));   // (n < 2^31: the limit of check_block_rows)
  if (dp < 1) { set_error("sim_dense_combined_segmented: dp < 1"); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 0, n));
  if (n == 0) return MMF_OK;
  if (!P || !out) { set_error("sim_dense_combined_segmented: NULL pointer"); return MMF_E_INVALID; }
  const std::vector<int64_t> tab = sim_dense_combined_seg_table(ptr_host, n_seg);
  const int64_t grid = (int64_t)tab.size() / 8;
  if (grid >= ((int64_t)1 << 31)) { set_error("sim_dense_combined_segmented: %lld workgroups", (long long)grid); return MMF_E_UNSUPPORTED; }
  MMF_TRY(c.begin(ws_bytes(n, 4) + ws_bytes(prep_f32_bytes(n, d), 1) + ws_bytes(tab.size(), 8)));
  const hipStream_t s = c.s;
  float* nf = c.ws.take<float>(n);
  float* Fp = reinterpret_cast<float*>(c.ws.take<char>(prep_f32_bytes(n, d)));
  int64_t* d_tab = c.ws.take<int64_t>(tab.size());
  MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_prep_f32(F, n, d, MMF_F32, nullptr, Fp, s));
  return launch_sim_dense_combined_seg(Fp, P, d, dp, lambda_h, lambda_g, nf, d_tab, grid, out, s);
}

// The off-diagonal lower median of every block: K[~eye] + torch.median per slide, build_hypergraph/similarity_kernel.py:183-186.
// The four-pass radix select of mmf_offdiag_lower_median with a select state per segment (mmf_edges.hip): a fixed number of
// launches for any n_seg, no host synchronisation.
int mmf_offdiag_lower_median_segmented(const float* K, const int64_t* ptr_host, int64_t n_seg, float* out_median, int device_id,
                                       void* hip_stream) {
  Call c("offdiag_lower_median_segmented", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 2, kAnyRows));
  MMF_TRY(check_block_rows(c.who, ptr_host[n_seg]));
  if (!K || !out_median) { set_error("offdiag_lower_median_segmented: NULL pointer"); return MMF_E_INVALID; }
  const size_t need = offdiag_lower_median_seg_scratch_bytes(ptr_host, n_seg);
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_offdiag_lower_median_seg(K, ptr_host, n_seg, out_median, c.ws.take<char>(need), c.s);
}

// The threshold edges of every block against its own threshold (thresholds: device f32 [n_seg]): the per-slide double loop
// of build_hypergraph/similarity_kernel.py:193-202, in the two calls of mmf_threshold_edges_count / _fill.  Edges are global
// row ids (ptr[s] + i, ptr[s] + j), segment-major and row-major inside a segment; segment s's start at row_offsets[ptr[s]].
int mmf_threshold_edges_segmented_count(const float* K, const int64_t* ptr_host, int64_t n_seg, const float* thresholds,
                                        uint64_t* row_offsets, int64_t* out_count, int device_id, void* hip_stream) {
  Call c("threshold_edges_segmented_count", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 0, kAnyRows));
  const int64_t n = ptr_host[n_seg];
  MMF_TRY(check_block_rows(c.who, n));
  if (!out_count || !row_offsets || (n > 0 && (!K || !thresholds))) { set_error("threshold_edges_segmented_count: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  MMF_HIP(hipMemsetAsync(out_count, 0, 8, s));
  if (n == 0) { MMF_HIP(hipMemsetAsync(row_offsets, 0, 8, s)); return MMF_OK; }
  const std::vector<int64_t> kptr = block_offsets(ptr_host, n_seg);
  Workspace ws;
  MMF_TRY(c.workspace(2 * ws_bytes((size_t)n_seg + 1, 8) + ws_bytes((size_t)n, 4), &ws));
  int64_t* d_ptr = ws.take<int64_t>((size_t)n_seg + 1);
  int64_t* d_kptr = ws.take<int64_t>((size_t)n_seg + 1);
  uint32_t* row_cnt = ws.take<uint32_t>((size_t)n);
  MMF_TRY(upload_table(s, d_ptr, ptr_host, (size_t)(n_seg + 1) * 8));
  MMF_TRY(upload_table(s, d_kptr, kptr.data(), (size_t)(n_seg + 1) * 8));
  return launch_threshold_count_seg(K, d_ptr, d_kptr, n_seg, n, thresholds, reinterpret_cast<unsigned long long*>(row_offsets), out_count,
                                    row_cnt, s);
}

int mmf_threshold_edges_segmented_fill(const float* K, const int64_t* ptr_host, int64_t n_seg, const float* thresholds,
                                       const uint64_t* row_offsets, int64_t* edge_index, float* edge_w, int64_t capacity, int device_id,
                                       void* hip_stream) {
  Call c("threshold_edges_segmented_fill", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 0, kAnyRows));
  const int64_t n = ptr_host[n_seg];
  MMF_TRY(check_block_rows(c.who, n));
  if (capacity < 0) { set_error("threshold_edges_segmented_fill: bad capacity"); return MMF_E_INVALID; }
  if (n == 0 || capacity == 0) return MMF_OK;
  if (!K || !thresholds || !row_offsets || !edge_index || !edge_w) { set_error("threshold_edges_segmented_fill: NULL pointer"); return MMF_E_INVALID; }
  const std::vector<int64_t> kptr = block_offsets(ptr_host, n_seg);
  MMF_TRY(c.begin(2 * ws_bytes((size_t)n_seg + 1, 8)));
  const hipStream_t s = c.s;
  int64_t* d_ptr = c.ws.take<int64_t>((size_t)n_seg + 1);
  int64_t* d_kptr = c.ws.take<int64_t>((size_t)n_seg + 1);
  MMF_TRY(upload_table(s, d_ptr, ptr_host, (size_t)(n_seg + 1) * 8));
  MMF_TRY(upload_table(s, d_kptr, kptr.data(), (size_t)(n_seg + 1) * 8));
  return launch_threshold_fill_seg(K, d_ptr, d_kptr, n_seg, n, thresholds, reinterpret_cast<const unsigned long long*>(row_offsets),
                                   edge_index, edge_w, capacity, s);
}

// ---- segmented WSI x TMA similarity and the flat ragged median ----------------------------------
// compute_wsi_tma_similarity of every slide of a cohort (build_hypergraph/preprocess_hypergraph.py:248-265): the pivots, ONE tiled
// launch over a host-built work table, the per-segment merge of the partials, the flat ragged median over the stored blocks.
// Block s and its five statistics are bit for bit mmf_sim_dense_stats(X_s, Y_s, MMF_RBF_DIRECT).
int mmf_sim_dense_stats_segmented(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                                  const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_seg, float* out, double* out_stats,
                                  int device_id, void* hip_stream) {
  Call c("sim_dense_stats_segmented", device_id, hip_stream);
  const char* what = c.who;
  MMF_TRY(check_common(c, X, n, m, d, in_dtype));
  if (metric < MMF_DOT || metric > MMF_RBF_DIRECT) { set_error("%s: bad metric %d", what, metric); return MMF_E_INVALID; }
  if (metric != MMF_RBF_DIRECT) { set_error("%s: only MMF_RBF_DIRECT is supported (got metric %d)", what, metric); return MMF_E_UNSUPPORTED; }
  MMF_TRY(check_offsets(what, "x_ptr", x_ptr_host, n_seg, 1, 1, n));
  MMF_TRY(check_offsets(what, "y_ptr", y_ptr_host, n_seg, 1, 1, m));
  if (!Y || !out_stats) { set_error("%s: NULL pointer", what); return MMF_E_INVALID; }
  if (!out) { set_error("%s: out == NULL is not supported (the median reads the stored blocks)", what); return MMF_E_UNSUPPORTED; }
  std::vector<int64_t> optr((size_t)n_seg + 1, 0), pbase;
  for (int64_t g = 0; g < n_seg; ++g)      // n, m < 2^31: sum n_s m_s <= n m < 2^62
    optr[g + 1] = optr[g] + (x_ptr_host[g + 1] - x_ptr_host[g]) * (y_ptr_host[g + 1] - y_ptr_host[g]);
  const std::vector<int64_t> tab = rbf_direct_seg_table(x_ptr_host, y_ptr_host, n_seg, &pbase);
  const int64_t grid = pbase[n_seg];
  if (grid >= ((int64_t)1 << 31)) { set_error("%s: %lld workgroups", what, (long long)grid); return MMF_E_UNSUPPORTED; }
  const size_t S1 = (size_t)n_seg + 1, mneed = lower_median_seg_scratch_bytes(optr.data(), n_seg);
  MMF_TRY(c.begin(ws_bytes((size_t)grid * stat_partial_bytes(), 1) + 2 * ws_bytes((size_t)n_seg, 4) + 4 * ws_bytes(S1, 8) +
                          ws_bytes(tab.size(), 8) + ws_bytes(mneed, 1)));
  const hipStream_t s = c.s;
  char* part = c.ws.take<char>((size_t)grid * stat_partial_bytes());
  float* pivot = c.ws.take<float>((size_t)n_seg);
  float* med = c.ws.take<float>((size_t)n_seg);
  int64_t* d_xptr = c.ws.take<int64_t>(S1);
  int64_t* d_yptr = c.ws.take<int64_t>(S1);
  int64_t* d_optr = c.ws.take<int64_t>(S1);
  int64_t* d_pbase = c.ws.take<int64_t>(S1);
  int64_t* d_tab = c.ws.take<int64_t>(tab.size());
  void* mscratch = c.ws.take<char>(mneed);
  MMF_TRY(upload_table(s, d_xptr, x_ptr_host, S1 * 8));
  MMF_TRY(upload_table(s, d_yptr, y_ptr_host, S1 * 8));
  MMF_TRY(upload_table(s, d_optr, optr.data(), S1 * 8));
  MMF_TRY(upload_table(s, d_pbase, pbase.data(), S1 * 8));
  MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
  MMF_TRY(launch_rbf_direct_pivot_seg(X, Y, d, in_dtype, lambda, d_xptr, d_yptr, n_seg, pivot, s));
  MMF_TRY(launch_rbf_direct_seg(X, Y, d, in_dtype, lambda, out, part, pivot, d_tab, grid, d_xptr, d_yptr, d_optr, d_pbase, s));
  MMF_TRY(launch_stats_finish_seg(part, d_pbase, pivot, d_xptr, d_yptr, n_seg, out_stats, s));
  MMF_TRY(launch_lower_median_seg(out, optr.data(), n_seg, med, mscratch, s));
  return launch_stats_set_median_seg(med, n_seg, out_stats, s);
}

// torch.median of every block v[ptr[s]:ptr[s+1]] of a flat ragged array: the similarity blocks above, and the edge-weight median
// filter of the rebuild (preprocess_hypergraph.py:885-897) for every slide of a cohort's edge list.
int mmf_lower_median_segmented(const float* v, const int64_t* ptr_host, int64_t n_seg, float* out_median, int device_id, void* hip_stream) {
  Call c("lower_median_segmented", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(check_offsets(c.who, "ptr", ptr_host, n_seg, 1, 1, kAnyRows));
  if (!v || !out_median) { set_error("%s: NULL pointer", c.who); return MMF_E_INVALID; }
  const size_t need = lower_median_seg_scratch_bytes(ptr_host, n_seg);
  MMF_TRY(c.begin(ws_bytes(need, 1)));
  return launch_lower_median_seg(v, ptr_host, n_seg, out_median, c.ws.take<char>(need), c.s);
}

// ---- ordered k-NN + clique edges of a ragged batch (mmf_knn_clique.hip) -----------------------------
// The edge list that build_hypergraph_knn_kmeans assembles per slide (preprocess_hypergraph.py:386-404), for every segment at
// once and already in its documented order.  Count, one host read of *out_count by the caller, fill.
static int knn_clique_check(const Call& c, const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t n_clusters,
                            const int64_t* ptr_host, int64_t n_seg) {
  const char* what = c.who;
  MMF_TRY(c.on_device());
  MMF_TRY(check_offsets(what, "ptr", ptr_host, n_seg, 1, 0, n));
  MMF_TRY(check_block_rows(what, n));
  if (k < 1) { set_error("%s: k must be >= 1 (got %d)", what, k); return MMF_E_INVALID; }
  if (n > 0 && !nbr) { set_error("%s: NULL pointer", what); return MMF_E_INVALID; }
  if (labels) {
    if (n_clusters < 1) { set_error("%s: n_clusters must be >= 1 (got %lld)", what, (long long)n_clusters); return MMF_E_INVALID; }
    if (n_clusters >= ((int64_t)1 << 31) || n_seg * n_clusters >= ((int64_t)1 << 31)) {
      set_error("%s: n_seg * n_clusters = %lld x %lld, must be < 2^31", what, (long long)n_seg, (long long)n_clusters);
      return MMF_E_UNSUPPORTED;
    }
  }
  return MMF_OK;
}

int mmf_knn_clique_edges_count(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t n_clusters, const int64_t* ptr_host,
                               int64_t n_seg, uint64_t* row_offsets, int64_t* edge_ptr, int64_t* out_count, int device_id,
                               void* hip_stream) {
  Call c("knn_clique_edges_count", device_id, hip_stream);
  MMF_TRY(knn_clique_check(c, nbr, n, k, labels, n_clusters, ptr_host, n_seg));
  if (!row_offsets || !edge_ptr || !out_count) { set_error("knn_clique_edges_count: NULL pointer"); return MMF_E_INVALID; }
  MMF_TRY(c.begin());
  const hipStream_t s = c.s;
  if (n == 0) {
    MMF_HIP(hipMemsetAsync(out_count, 0, 8, s));
    MMF_HIP(hipMemsetAsync(row_offsets, 0, 8, s));
    MMF_HIP(hipMemsetAsync(edge_ptr, 0, (size_t)(n_seg + 1) * 8, s));
    return MMF_OK;
  }
  const size_t need = knn_clique_scratch_bytes(n, n_seg, n_clusters, labels != nullptr);
  Workspace ws;
  MMF_TRY(c.workspace(need, &ws));
  return launch_knn_clique_count(nbr, n, k, labels, n_clusters, ptr_host, n_seg, reinterpret_cast<unsigned long long*>(row_offsets),
                                 edge_ptr, out_count, ws.take<char>(need), s);
}

int mmf_knn_clique_edges_fill(const int64_t* nbr, int64_t n, int k, const int64_t* labels, int64_t n_clusters, const int64_t* ptr_host,
                              int64_t n_seg, const uint64_t* row_offsets, int64_t* edge_index, int64_t capacity, int device_id,
                              void* hip_stream) {
  Call c("knn_clique_edges_fill", device_id, hip_stream);
  MMF_TRY(knn_clique_check(c, nbr, n, k, labels, n_clusters, ptr_host, n_seg));
  if (capacity < 0) {      // what the count entry reports instead of a count when a label is out of range
    set_error("knn_clique_edges_fill: capacity %lld: a label lies outside [0, %lld)", (long long)capacity, (long long)n_clusters);
    return MMF_E_INVALID;
  }
  if (n == 0 || capacity == 0) return MMF_OK;
  if (!row_offsets || !edge_index) { set_error("knn_clique_edges_fill: NULL pointer"); return MMF_E_INVALID; }
  const size_t need = knn_clique_scratch_bytes(n, n_seg, n_clusters, labels != nullptr);
  MMF_TRY(c.begin(need));
  return launch_knn_clique_fill(nbr, n, k, labels, n_clusters, ptr_host, n_seg, reinterpret_cast<const unsigned long long*>(row_offsets),
                                edge_index, capacity, c.ws.take<char>(need), c.s);
}


}  // extern "C"

// ---- segmented exact scan (include/ext/mmf_hg_seg_exact.h) -----------------------------------------------
// One table-driven launch of the exact scan for every segment with rows and at least k admissible columns, one re-rank over all
// rows with ids that are rows of Y, one fail-count readback.  The segments short of columns keep the launch loop (ExactPass
// slices).  P set: the combined key of mmf_simtopk_combined (r.X == r.Y == F, MMF_RBF, r.lambda = lambda_h).
namespace mmf {

static int check_pow2_splits(const char* who, const mmf_simtopk_opts* opts) {
  const int cs = opts ? opts->col_splits : 0;
  if (cs < 0 || (cs & (cs - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, cs); return MMF_E_INVALID; }
  return MMF_OK;
}

// r: checked, begun, n > 0.  xp / yp: host offsets of the S segments on the two sides (the same array for a self call).
// cross (mmf_simtopk_cross_segments): the complement — the table is cross_seg_table's, the kernel masks each
// block's own segment of Y; the entry has refused every segment short of k admissible columns, so the table serves every row.
static int run_segmented_exact(Request& r, bool self, const int64_t* xp, const int64_t* yp, int64_t S, const mmf_simtopk_opts* opts,
                               const float* P, int dp, float lambda_g, bool cross = false) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const int k = r.k, self1 = r.exclude_self ? 1 : 0;
  const int cap = scan_f32_cap(std::min(r.kk, 44));
  int ranges = 1;
  std::vector<char> served;
  const std::vector<int64_t> tab = cross ? cross_seg_table(xp, yp, S, k, opts ? opts->col_splits : 0, &ranges)
                                         : seg_exact_table(xp, yp, S, k, r.exclude_self, opts ? opts->col_splits : 0, &ranges, &served);
  if (cross) served.assign((size_t)S, 1);
  const int64_t grid = (int64_t)tab.size() / 8;
  if (grid >= ((int64_t)1 << 31)) { set_error("%s: %lld workgroups", who, (long long)grid); return MMF_E_UNSUPPORTED; }
  const int lists = 2 * ranges;
  const int k_pass_max = 44 - self1;
  const int passes = (k + k_pass_max - 1) / k_pass_max;
  const bool floors = passes > 1;

  // the segments the table does not serve: the launch loop, for what they have
  ExactPass ex(r, nullptr, nullptr);
  ex.same = self;
  ex.P = P; ex.dp = dp; ex.lambda_g = lambda_g;
  int64_t unserved_rows = 0;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
    if (ng == 0 || served[g]) continue;
    unserved_rows += ng;
    MMF_HIP(hipMemsetAsync(r.out_idx + xp[g] * k, 0xff, (size_t)ng * k * 8, s));
    MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.out_val + xp[g] * k), (int)0xff800000u, (size_t)ng * k, s));
    const int64_t adm = admissible_columns(xp[g], ng, yp[g], mg, r.exclude_self);
    if (adm > 0) ex.add(ExactGroup{xp[g], ng, false, yp[g], mg, (int)adm});
  }

  const int64_t n = r.n, m = r.m;
  const size_t list_words = (size_t)n * lists;
  size_t need = ws_bytes(n, 4) + ws_bytes(m, 4) + 2 * ws_bytes(n, 4) + ws_bytes(256, 4) + ws_bytes(4 * (size_t)passes, 4);
  if (grid > 0)
    need += ws_bytes(prep_f32_bytes(m, r.d), 1) + (self ? 0 : ws_bytes(prep_f32_bytes(n, r.d), 1)) + ws_bytes(tab.size(), 8) +
            ExactLists::bytes(n, list_words, cap, floors);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = self ? rx : ws.take<float>(m);
  float* pn = P ? ws.take<float>(n) : nullptr;
  uint32_t* cand_total = ws.take<uint32_t>(256);
  uint32_t* fail_counts = ws.take<uint32_t>(4 * (size_t)passes);   // one block per pass: the rows outside the table fail in each
  ex.rx = rx; ex.cy = cy; ex.pn = pn;

  EventTimer t[3];   // prep (row scalars, f32 images, table), scan, re-rank; several passes: the whole loop is "scan"
  MMF_TRY(t[0].start(r.profile, s));
  MMF_TRY(launch_row_scalars(r.X, n, r.d, r.dtype, r.metric, rx, nullptr, s));
  if (!self && m > 0) MMF_TRY(launch_row_scalars(r.Y, m, r.d, r.dtype, r.metric, cy, nullptr, s));
  if (P) MMF_TRY(launch_row_scalars(P, n, dp, MMF_F32, MMF_RBF, pn, nullptr, s));
  std::vector<uint32_t> h_fail(4 * (size_t)passes, 0), h_tot(r.stats && grid > 0 ? 256 : 0);
  if (grid > 0) {
    float* Yp = reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(m, r.d)));
    float* Xp = self ? Yp : reinterpret_cast<float*>(ws.take<char>(prep_f32_bytes(n, r.d)));
    int64_t* d_tab = ws.take<int64_t>(tab.size());
    ExactLists B;
    B.carve(ws, n, list_words, cap, floors);
    MMF_TRY(launch_prep_f32(r.Y, m, r.d, r.dtype, nullptr, Yp, s));
    if (!self) MMF_TRY(launch_prep_f32(r.X, n, r.d, r.dtype, nullptr, Xp, s));
    MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
    // the slots of ranges a segment does not use, and every slot of a row outside the table, stay empty
    MMF_HIP(hipMemsetAsync(B.L.cnt, 0, list_words * 4, s));
    MMF_HIP(hipMemsetAsync(B.L.overflow, 0, (size_t)n * 4, s));
    MMF_HIP(hipMemsetAsync(fail_counts, 0, 16 * (size_t)passes, s));
    MMF_HIP(hipMemsetAsync(cand_total, 0, 1024, s));
    MMF_TRY(t[0].stop(s));

    CandLists L = B.L;
    L.lists = lists; L.cap = cap;
    ScanProblem sp{};
    sp.X = r.X; sp.n = n; sp.Y = r.Y; sp.m = m; sp.Xp = Xp; sp.Yp = Yp; sp.d = r.d; sp.dtype = r.dtype; sp.metric = r.metric;
    sp.lambda = r.lambda; sp.rx = rx; sp.cy = cy; sp.row_ids = nullptr; sp.n_rows = n; sp.col_splits = ranges;
    SelectProblem q = r.select();   // all rows, ids are rows of Y: no offsets
    q.rx = rx; q.cy = cy; q.out_stride = k;
    q.fail_rows = B.fail_rows; q.cand_total = r.stats ? cand_total : nullptr;
    if (P) {
      sp.Pq = sp.Pc = q.Pq = q.Pc = P; sp.pnq = sp.pnc = q.pnq = q.pnc = pn;
      sp.dp = q.dp = dp; sp.lambda_g = q.lambda_g = lambda_g;
    }
    MMF_TRY(t[1].start(r.profile, s));
    int pass = 0;
    for (int done = 0; done < k; done += k_pass_max, ++pass) {
      const int kp = std::min(k - done, k_pass_max);
      const bool more = done + kp < k;
      sp.kk = kp + self1;
      if (done > 0) { sp.floor_key = B.floor_key; sp.floor_id = B.floor_id; }
      MMF_TRY(launch_scan_f32_seg(sp, L, d_tab, grid, s, cross));
      if (passes == 1) { MMF_TRY(t[1].stop(s)); MMF_TRY(t[2].start(r.profile, s)); }
      q.k = kp; q.out_off = done;
      q.fail_count = fail_counts + 4 * pass;
      q.floor_key_out = more ? B.floor_key : nullptr; q.floor_id_out = more ? B.floor_id : nullptr;
      MMF_TRY(P ? launch_rerank_combined(q, L, s) : launch_select(q, L, s));
    }
    MMF_TRY(t[passes == 1 ? 2 : 1].stop(s));
    MMF_HIP(hipMemcpyAsync(h_fail.data(), fail_counts, 16 * (size_t)passes, hipMemcpyDeviceToHost, s));
    if (!h_tot.empty()) MMF_HIP(hipMemcpyAsync(h_tot.data(), cand_total, 1024, hipMemcpyDeviceToHost, s));
  } else {
    MMF_TRY(t[0].stop(s));
  }
  if (!ex.pieces.empty()) {   // images and lists of the launch loop in the second workspace slot
    Workspace aux;
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), ex.floors());
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
  }
  MMF_HIP(hipStreamSynchronize(s));
  for (int p = 0; p < passes && grid > 0; ++p)
    if (h_fail[4 * p] != (uint32_t)unserved_rows) {
      set_error("%s: %lld rows failed in the exact scan (internal invariant)", who, (long long)h_fail[4 * p] - (long long)unserved_rows);
      return MMF_E_INTERNAL;
    }
  fill_stats(r.stats, MMF_PREC_EXACT, grid > 0 ? ranges : (ex.pieces.empty() ? 1 : ex.splits(ex.pieces[0])), grid > 0 ? (int)grid : ex.grid,
             t[0].ms(), t[1].ms(), t[2].ms(), 0.f, 0, 0, 0, h_tot);
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

int mmf_simtopk_segmented_exact(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_segmented_exact";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  // check_common's refusals, under this entry's name
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  MMF_TRY(r.check(MMF_PREC_EXACT, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    const int prec = opts ? opts->precision : MMF_PREC_AUTO;
    if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT) {
      set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (the 16-bit scans are mmf_simtopk_segmented_wide's)", who, prec);
      return prec == MMF_PREC_FAST || prec == MMF_PREC_FAST_BF16 ? MMF_E_UNSUPPORTED : MMF_E_INVALID;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    return MMF_OK;
  }));
  if (stats) stats->near_rows = -1;
  if (n == 0) return MMF_OK;
  return run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f);
}

// ---- cross-segment top-k (include/ext/mmf_hg_cross_seg.h) -------------------------------------------------------
// The complement of the entry above from the same driver: every row against the rows of Y outside its own segment.  A row's self
// lies inside its segment, so nothing is excluded by identity (kk = k); a segment short of k admissible columns is refused here,
// on the host, so the driver's launch loop for unserved segments never runs.
int mmf_simtopk_cross_segments(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                               int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t* out_idx,
                               float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_cross_segments";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, 0, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  MMF_TRY(r.check(MMF_PREC_EXACT, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    const int prec = opts ? opts->precision : MMF_PREC_AUTO;
    if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT) {
      set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (no 16-bit scan serves the cross-segment entry yet)", who, prec);
      return prec == MMF_PREC_FAST || prec == MMF_PREC_FAST_BF16 ? MMF_E_UNSUPPORTED : MMF_E_INVALID;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    for (int64_t g = 0; g < n_segments; ++g) {
      const int64_t own = y_ptr_host[g + 1] - y_ptr_host[g];
      if (x_ptr_host[g + 1] > x_ptr_host[g] && m - own < k) {
        set_error("%s: segment %lld has %lld admissible columns (m = %lld minus its own %lld rows of Y), k = %d needs at least %d", who,
                  (long long)g, (long long)(m - own), (long long)m, (long long)own, k, k);
        return MMF_E_INVALID;
      }
    }
    return MMF_OK;
  }));
  if (stats) stats->near_rows = -1;
  if (n == 0) return MMF_OK;
  return run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true);
}

int64_t mmf_cross_segments_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int k, int col_splits,
                                 int64_t* table_host, int64_t capacity, int* lists_out) {
  const char* who = "cross_segments_table";
  if (!y_ptr_host) y_ptr_host = x_ptr_host;
  MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, kAnyRows));
  MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, kAnyRows));
  if (k < 1) { set_error("%s: k must be >= 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (col_splits < 0 || (col_splits & (col_splits - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, col_splits); return MMF_E_INVALID; }
  int ranges = 1;
  const std::vector<int64_t> tab = cross_seg_table(x_ptr_host, y_ptr_host, n_segments, k, col_splits, &ranges);
  const int64_t grid = (int64_t)tab.size() / 8;
  if (table_host) {
    if (capacity < grid) { set_error("%s: table of %lld entries needed", who, (long long)grid); return MMF_E_INVALID; }
    if (grid > 0) memcpy(table_host, tab.data(), tab.size() * 8);
  }
  if (lists_out) *lists_out = 2 * ranges;
  return grid;
}

// ---- cross-segment top-k on the 16-bit scan (include/ext/mmf_hg_cross_seg16.h) -----------------------------------
// The plain 16-bit images of both sides (launch_prep_half: column = row of Y), ONE table-driven scan launch whose epilogue masks,
// per query row, the columns of the row's own segment (launch_scan_b16_xseg), the audit, one re-rank over all rows, one host
// synchronisation.  Rows the re-rank reports go through the exact cross-segment scan, all of them in one launch (cross_flagged).
}  // extern "C"

namespace mmf {

// what the re-rank takes per row beside the overflow list: bounds the entries of a row block (cross_seg16_table)
static constexpr int kCross16Budget = 1024 - kSpillCap;

// The flagged rows of the 16-bit cross-segment call, `rows` ascending (so grouped by segment): the exact cross driver in its
// two-sided form over the gathered rows — x_ptr' counts the flagged rows per segment, y_ptr is the call's — as ONE exact scan
// launch and one re-rank, the rows handed over the way ExactPass hands gathered rows (an f32 image of the gathered rows,
// ScanProblem::row_ids, SelectProblem::row_ids).  k <= 44 here: one pass.  Images and lists live in the second workspace slot.
static int cross_flagged(const Request& r, const float* rx, const float* cy, const std::vector<int32_t>& rows, const int64_t* xp,
                         const int64_t* yp, int64_t S) {
  const hipStream_t s = r.call.s;
  const int64_t F = (int64_t)rows.size();
  std::vector<int64_t> fp((size_t)S + 1, 0);
  for (int64_t g = 0, e = 0; g < S; ++g) {
    while (e < F && rows[e] < xp[g + 1]) ++e;
    fp[g + 1] = e;
  }
  int ranges = 1;
  const std::vector<int64_t> tab = cross_seg_table(fp.data(), yp, S, r.k, 0, &ranges);
  const int64_t grid = (int64_t)tab.size() / 8;
  const int cap = scan_f32_cap(r.kk), lists = 2 * ranges;
  const size_t list_words = (size_t)F * lists;
  Workspace aux;
  MMF_TRY(r.call.workspace(ws_bytes(prep_f32_bytes(r.m, r.d), 1) + ws_bytes(prep_f32_bytes(F, r.d), 1) + ws_bytes(F, 4) +
                               ws_bytes(tab.size(), 8) + ExactLists::bytes(F, list_words, cap, false),
                           &aux, 1));
  float* Yp = reinterpret_cast<float*>(aux.take<char>(prep_f32_bytes(r.m, r.d)));
  float* Xe = reinterpret_cast<float*>(aux.take<char>(prep_f32_bytes(F, r.d)));
  int32_t* d_rows = aux.take<int32_t>(F);
  int64_t* d_tab = aux.take<int64_t>(tab.size());
  ExactLists B;
  B.carve(aux, F, list_words, cap, false);
  MMF_TRY(upload_table(s, d_rows, rows.data(), (size_t)F * 4));
  MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
  MMF_TRY(launch_prep_f32(r.Y, r.m, r.d, r.dtype, nullptr, Yp, s));
  MMF_TRY(launch_prep_f32(r.X, F, r.d, r.dtype, d_rows, Xe, s));
  MMF_TRY(B.zero(s));
  MMF_HIP(hipMemsetAsync(B.L.cnt, 0, list_words * 4, s));   // the slots of ranges a block does not use stay empty
  CandLists L = B.L;
  L.lists = lists; L.cap = cap;
  ScanProblem sp{};
  sp.X = r.X; sp.n = r.n; sp.Y = r.Y; sp.m = r.m; sp.Xp = Xe; sp.Yp = Yp; sp.d = r.d; sp.dtype = r.dtype; sp.metric = r.metric;
  sp.lambda = r.lambda; sp.rx = rx; sp.cy = cy; sp.row_ids = d_rows; sp.n_rows = F; sp.col_splits = ranges; sp.kk = r.kk;
  MMF_TRY(launch_scan_f32_seg(sp, L, d_tab, grid, s, true));
  SelectProblem q = r.select();
  q.rx = rx; q.cy = cy; q.row_ids = d_rows; q.n_rows = F; q.out_stride = r.k;
  q.fail_rows = B.fail_rows; q.fail_count = B.fail_count; q.cand_total = nullptr;
  MMF_TRY(launch_select(q, L, s));
  uint32_t h_fail = 0;
  MMF_HIP(hipMemcpyAsync(&h_fail, B.fail_count, 4, hipMemcpyDeviceToHost, s));
  MMF_HIP(hipStreamSynchronize(s));
  if (h_fail != 0) { set_error("%s: %u rows failed in the exact scan (internal invariant)", r.call.who, h_fail); return MMF_E_INTERNAL; }
  return MMF_OK;
}

// r: checked, begun, n > 0, precision MMF_PREC_FAST or _FAST_BF16, (d, k) served by the 16-bit scan — the wide one under `wide`
// (1024 < d <= 4096): the images at its padded dim, cross_segw_table, its list capacity, no id scratch, no shared
// thresholds, launch_scan_b16w_xseg; the overflow lists stay zeroed and unused there (select reads them as empty).
static int run_cross_segments16(Request& r, bool self, const int64_t* xp, const int64_t* yp, int64_t S, const mmf_simtopk_opts* opts,
                                bool wide) {
  const hipStream_t s = r.call.s;
  const int64_t n = r.n, m = r.m;
  const bool profile = r.profile, f16 = (r.precision == MMF_PREC_FAST);
  const int dp = wide ? scan_b16w_dp(r.d) : scan_bf16_dp(r.d), bcap = wide ? scan_b16w_cap(r.kk) : scan_bf16_cap(r.kk, dp);
  const int forced = opts ? opts->col_splits : 0;
  int lists = 2;
  const std::vector<int32_t> sched = wide ? cross_segw_table(xp, yp, S, bcap, kCross16Budget, forced, &lists)
                                          : cross_seg16_table(xp, yp, S, scan_b16_queries_per_block(dp), dp, bcap, kCross16Budget, forced, &lists);
  if (!wide && lists < 0) {
    set_error("%s: a column run of the %lld rows of Y exceeds 4 GiB of 16-bit operands at padded dim %d", r.call.who, (long long)m, dp);
    return MMF_E_UNSUPPORTED;
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  const int64_t n_pad = (n + 255) / 256 * 256, m_pad = (m + 255) / 256 * 256;
  // per row of X: first row and row count of the columns it may not take; padding rows exclude nothing
  std::vector<uint32_t> bounds((size_t)n_pad * 2, 0u);
  for (int64_t g = 0; g < S; ++g)
    for (int64_t i = xp[g]; i < xp[g + 1]; ++i) { bounds[2 * i] = (uint32_t)yp[g]; bounds[2 * i + 1] = (uint32_t)(yp[g + 1] - yp[g]); }

  const size_t scratch_bytes = wide ? 0 : scan_b16_seg_scratch_bytes(grid, dp, bcap);   // 0 bytes: nothing is carved
  const size_t need = ws_bytes(n, 4) + (self ? 0 : ws_bytes(m, 4)) + FlagBlock::bytes(n) + ws_bytes(4, 4) + HalfImage::bytes(n_pad, dp) +
                      (self ? 0 : HalfImage::bytes(m_pad, dp)) + ws_bytes(sched.size(), 4) + ws_bytes(bounds.size(), 4) +
                      b16_lists_bytes(n, lists, bcap) + ws_bytes(scratch_bytes, 1) + ws_bytes(2 * (size_t)n, 4) +
                      ws_bytes(select_order_bytes(n), 1);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = self ? rx : ws.take<float>(m);
  FlagBlock flags;
  flags.carve(ws, n);
  MMF_TRY(flags.zero(s));
  uint32_t* max_n = ws.take<uint32_t>(4);
  HalfImage Q, C;
  Q.carve(ws, n_pad, dp);
  if (self) C = Q; else C.carve(ws, m_pad, dp);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  uint32_t* d_bounds = ws.take<uint32_t>(bounds.size());
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  char* scan_scratch = ws.take<char>(scratch_bytes);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)n);
  char* order_scratch = ws.take<char>(select_order_bytes(n));

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  MMF_HIP(hipMemsetAsync(max_n, 0, 16, s));
  MMF_TRY(launch_row_scalars(r.X, n, r.d, r.dtype, r.metric, rx, max_n, s));
  if (!self) MMF_TRY(launch_row_scalars(r.Y, m, r.d, r.dtype, r.metric, cy, max_n, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(upload_table(s, d_bounds, bounds.data(), bounds.size() * 4));
  MMF_HIP(hipMemsetAsync(Q.maxima, 0, 16, s));
  if (!self) MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_TRY(launch_prep_half({r.Y, m, r.d, r.dtype, r.metric, cy, max_n}, C, dp, f16, s));
  if (!self) MMF_TRY(launch_prep_half({r.X, n, r.d, r.dtype, r.metric, rx, max_n}, Q, dp, f16, s));
  MMF_TRY(t_prep.stop(s));

  MMF_TRY(reset_b16_lists(L, n, lists, seed, n, s));
  ScanB16Panel pn;
  pn.seed = seed; pn.seed_stride = n; pn.share = (!wide && lists > 2) ? 1 : 0;
  MMF_TRY(t_scan.start(profile, s));
  const ScanB16Problem sp(Q, C, n, m, m_pad, dp, r.d, f16, r.metric, r.kk);
  if (wide) MMF_TRY(launch_scan_b16w_xseg(sp, d_sched, grid, d_bounds, lists, L, pn, s));
  else MMF_TRY(launch_scan_b16_xseg(sp, d_sched, grid, d_bounds, L, scan_scratch, pn, s));
  MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
  MMF_TRY(t_scan.stop(s));

  SelectProblem q = r.select();
  q.rx = rx; q.cy = cy;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = r.stats ? flags.cand_total : nullptr;
  q.two_pass = true;
  q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
  MMF_TRY(t_sel.start(profile, s));
  MMF_TRY(launch_select(q, L, s));
  MMF_TRY(t_sel.stop(s));
  MMF_TRY(flags.read(r.stats != nullptr, s));   // the call's one synchronisation when no row is flagged
  const uint32_t* h_fail4 = flags.h_fail4;
  const int64_t fallback_rows = h_fail4[0];
  MMF_TRY(t_fb.start(profile && fallback_rows > 0, s));
  if (fallback_rows > 0) {
    std::vector<int32_t> rows((size_t)fallback_rows);
    MMF_HIP(hipMemcpyAsync(rows.data(), flags.fail_rows, (size_t)fallback_rows * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));               // only on this branch: the fail list, now that its length is known
    std::sort(rows.begin(), rows.end());
    MMF_TRY(cross_flagged(r, rx, cy, rows, xp, yp, S));
  }
  MMF_TRY(t_fb.stop(s));
  const int64_t overflow_rows = h_fail4[1] < (uint32_t)fallback_rows ? h_fail4[1] : fallback_rows;
  fill_stats(r.stats, r.precision, lists / 2, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback_rows, overflow_rows,
             fallback_rows - overflow_rows, flags.h_tot);
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

int mmf_simtopk_cross_segments_fast(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                                    int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t* out_idx,
                                    float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id,
                                    void* hip_stream) {
  const char* who = "simtopk_cross_segments_fast";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, 0, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  // AUTO means FAST where the 16-bit scan serves (d, k) and the exact driver elsewhere; settled here, before any device call
  int prec = opts ? opts->precision : MMF_PREC_AUTO;
  const bool served = k >= 1 && scan_bf16_supported(d, k, in_dtype);
  if (prec == MMF_PREC_AUTO) prec = served ? MMF_PREC_FAST : MMF_PREC_EXACT;
  MMF_TRY(r.check(prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    if (prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
      set_error("%s: bad precision %d", who, prec);
      return MMF_E_INVALID;
    }
    if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
    if (prec != MMF_PREC_EXACT && !served) {
      set_error("%s: MMF_PREC_FAST does not support d = %lld, k = %d (AUTO takes the exact scan there)", who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    for (int64_t g = 0; g < n_segments; ++g) {
      const int64_t own = y_ptr_host[g + 1] - y_ptr_host[g];
      if (x_ptr_host[g + 1] > x_ptr_host[g] && m - own < k) {
        set_error("%s: segment %lld has %lld admissible columns (m = %lld minus its own %lld rows of Y), k = %d needs at least %d", who,
                  (long long)g, (long long)(m - own), (long long)m, (long long)own, k, k);
        return MMF_E_INVALID;
      }
    }
    return MMF_OK;
  }));
  if (stats) stats->near_rows = -1;
  if (n == 0) return MMF_OK;
  if (r.precision == MMF_PREC_EXACT) return run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true);
  return run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, false);
}

int64_t mmf_cross_segments_fast_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t d, int k,
                                      int col_splits, int32_t* table_host, int64_t capacity, int* lists_out) {
  const char* who = "cross_segments_fast_table";
  if (!y_ptr_host) y_ptr_host = x_ptr_host;
  MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, kAnyRows));
  MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, kAnyRows));
  if (k < 1) { set_error("%s: k must be >= 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (col_splits < 0 || (col_splits & (col_splits - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, col_splits); return MMF_E_INVALID; }
  if (d < 1 || !scan_bf16_supported(d, k, MMF_F32)) {
    set_error("%s: the 16-bit scan does not serve d = %lld, k = %d", who, (long long)d, k);
    return MMF_E_UNSUPPORTED;
  }
  if ((n_segments > 0 ? x_ptr_host[n_segments] : 0) >= (int64_t)1 << 31 || (n_segments > 0 ? y_ptr_host[n_segments] : 0) >= (int64_t)1 << 31) {
    set_error("%s: n and m must be < 2^31", who);
    return MMF_E_UNSUPPORTED;
  }
  const int dp = scan_bf16_dp(d);
  int lists = 2;
  const std::vector<int32_t> tab = cross_seg16_table(x_ptr_host, y_ptr_host, n_segments, scan_b16_queries_per_block(dp), dp,
                                                     scan_bf16_cap(k, dp), kCross16Budget, col_splits, &lists);
  if (lists < 0) { set_error("%s: a column run exceeds 4 GiB of 16-bit operands at padded dim %d", who, dp); return MMF_E_UNSUPPORTED; }
  const int64_t grid = (int64_t)tab.size() / 8;
  if (table_host) {
    if (capacity < grid) { set_error("%s: table of %lld entries needed", who, (long long)grid); return MMF_E_INVALID; }
    if (grid > 0) memcpy(table_host, tab.data(), tab.size() * 4);
  }
  if (lists_out) *lists_out = lists;
  return grid;
}

// ---- cross-segment top-k on the wide 16-bit scan (include/ext/mmf_hg_cross_segw.h) -------------------------------
// run_cross_segments16 under `wide`, 1024 < d <= 4096: the plain 16-bit images at the wide scan's padded dim, ONE table-driven
// launch of the wide scan whose epilogue masks, per query row, the columns of the row's own segment (launch_scan_b16w_xseg; its
// threshold union when a block has several entries), the audit, one re-rank over all rows, one host synchronisation.  Flagged
// rows: cross_flagged.
int mmf_simtopk_cross_segments_wide(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric, float lambda,
                                    int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t* out_idx,
                                    float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id,
                                    void* hip_stream) {
  const char* who = "simtopk_cross_segments_wide";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, 0, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.wide_ok = true;
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  // AUTO means FAST where the WIDE scan serves (d, k) and the exact driver elsewhere — also where the narrow 16-bit scan would
  // serve: routing between the two 16-bit entries is the caller's; settled here, before any device call
  int prec = opts ? opts->precision : MMF_PREC_AUTO;
  const bool served = k >= 1 && scan_b16w_supported(d, k);
  if (prec == MMF_PREC_AUTO) prec = served ? MMF_PREC_FAST : MMF_PREC_EXACT;
  MMF_TRY(r.check(prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    if (prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
      set_error("%s: bad precision %d", who, prec);
      return MMF_E_INVALID;
    }
    if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
    if (prec != MMF_PREC_EXACT && !served) {
      set_error("%s: MMF_PREC_FAST does not support d = %lld, k = %d (the wide scan serves 1024 < d <= 4096 with k <= 20)", who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    for (int64_t g = 0; g < n_segments; ++g) {
      const int64_t own = y_ptr_host[g + 1] - y_ptr_host[g];
      if (x_ptr_host[g + 1] > x_ptr_host[g] && m - own < k) {
        set_error("%s: segment %lld has %lld admissible columns (m = %lld minus its own %lld rows of Y), k = %d needs at least %d", who,
                  (long long)g, (long long)(m - own), (long long)m, (long long)own, k, k);
        return MMF_E_INVALID;
      }
    }
    return MMF_OK;
  }));
  if (stats) stats->near_rows = -1;
  if (n == 0) return MMF_OK;
  if (r.precision == MMF_PREC_EXACT) return run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true);
  return run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, true);
}

int64_t mmf_cross_segments_wide_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int64_t d, int k,
                                      int col_splits, int32_t* table_host, int64_t capacity, int* lists_out) {
  const char* who = "cross_segments_wide_table";
  if (!y_ptr_host) y_ptr_host = x_ptr_host;
  MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, kAnyRows));
  MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, kAnyRows));
  if (k < 1) { set_error("%s: k must be >= 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (col_splits < 0 || (col_splits & (col_splits - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, col_splits); return MMF_E_INVALID; }
  if (d < 1 || !scan_b16w_supported(d, k)) {
    set_error("%s: the wide 16-bit scan does not serve d = %lld, k = %d", who, (long long)d, k);
    return MMF_E_UNSUPPORTED;
  }
  if ((n_segments > 0 ? x_ptr_host[n_segments] : 0) >= (int64_t)1 << 31 || (n_segments > 0 ? y_ptr_host[n_segments] : 0) >= (int64_t)1 << 31) {
    set_error("%s: n and m must be < 2^31", who);
    return MMF_E_UNSUPPORTED;
  }
  int lists = 2;
  const std::vector<int32_t> tab = cross_segw_table(x_ptr_host, y_ptr_host, n_segments, scan_b16w_cap(k), kCross16Budget, col_splits, &lists);
  const int64_t grid = (int64_t)tab.size() / 8;
  if (table_host) {
    if (capacity < grid) { set_error("%s: table of %lld entries needed", who, (long long)grid); return MMF_E_INVALID; }
    if (grid > 0) memcpy(table_host, tab.data(), tab.size() * 4);
  }
  if (lists_out) *lists_out = lists;
  return grid;
}

int mmf_simtopk_combined_segmented_exact(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                                         float lambda_g, int k, int exclude_self, const int64_t* ptr_host, int64_t n_segments,
                                         int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats,
                                         int device_id, void* hip_stream) {
  const char* who = "simtopk_combined_segmented_exact";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !std::isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !std::isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(who, "ptr_host", ptr_host, n_segments, 0, 0, n));
  MMF_TRY(check_pow2_splits(who, opts));
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int kk = k + (exclude_self ? 1 : 0);
  if (kk > 44) { set_error("%s: k + self = %d > 44 is not supported (the combined re-rank has no floors)", who, kk); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT) {
    set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (the 16-bit scan is mmf_simtopk_combined_fast_segmented)", who, prec);
    return MMF_E_UNSUPPORTED;
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n == 0) return MMF_OK;
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.kk = kk;
  r.precision = MMF_PREC_EXACT;
  MMF_TRY(r.call.begin());
  return run_segmented_exact(r, true, ptr_host, ptr_host, n_segments, opts, P, (int)dp, lambda_g);
}

// ---- the combined top-k for any k (include/ext/mmf_hg_topk_anyk.h) ---------------------------------------
// The drivers of the entries above without their k + self > 44 refusal: ExactPass::run and run_segmented_exact loop over passes of
// at most 44 - self entries, and launch_rerank_combined (mmf_topk.hip) now writes a pass's columns and the next pass's floors.

int mmf_simtopk_combined_anyk(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                              int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                              const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_combined_anyk";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !std::isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !std::isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const bool segmented = ptr_host != nullptr || n_segments != 0;
  if (segmented) {
    MMF_TRY(check_offsets(who, "ptr_host", ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_pow2_splits(who, opts));
  }
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT) {
    set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (the 16-bit combined scans stop at k + self = 20)", who, prec);
    return MMF_E_UNSUPPORTED;
  }
  if (opts && opts->col_splits < 0) { set_error("%s: col_splits must be >= 0 (got %d)", who, opts->col_splits); return MMF_E_INVALID; }
  if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  if (!segmented) {
    const int64_t one_graph[2] = {0, n};
    return run_simtopk_combined(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, one_graph, 1, out_idx, out_val, opts, stats,
                                device_id, hip_stream);
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0,
            out_idx, out_val, stats, opts && opts->profile};
  r.kk = k + (exclude_self ? 1 : 0);
  r.precision = MMF_PREC_EXACT;
  MMF_TRY(r.call.begin());
  return run_segmented_exact(r, true, ptr_host, ptr_host, n_segments, opts, P, (int)dp, lambda_g);
}

int mmf_simtopk_combined_xy_anyk(const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                                 int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self,
                                 int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                                 const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_combined_xy_anyk";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (nq < 0) { set_error("%s: nq must be >= 0 (got %lld)", who, (long long)nq); return MMF_E_INVALID; }
  if (nc < 0) { set_error("%s: nc must be >= 0 (got %lld)", who, (long long)nc); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (row_offset < 0) { set_error("%s: row_offset must be >= 0 (got %lld)", who, (long long)row_offset); return MMF_E_INVALID; }
  if (col_offset < 0) { set_error("%s: col_offset must be >= 0 (got %lld)", who, (long long)col_offset); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !std::isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !std::isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (nq > 0 && !Fq) { set_error("%s: Fq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !Pq) { set_error("%s: Pq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Fc) { set_error("%s: Fc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Pc) { set_error("%s: Pc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO or MMF_PREC_EXACT", who, prec);
    return MMF_E_INVALID;
  }
  if (opts && opts->col_splits < 0) { set_error("%s: col_splits must be >= 0 (got %d)", who, opts->col_splits); return MMF_E_INVALID; }
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  if (prec == MMF_PREC_FAST || prec == MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: only MMF_PREC_AUTO and MMF_PREC_EXACT (the 16-bit combined scans stop at k + self = 20)", who, prec);
    return MMF_E_UNSUPPORTED;
  }
  if (nq >= ((int64_t)1 << 31) - row_offset) { set_error("%s: row_offset + nq must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (nc >= ((int64_t)1 << 31) - col_offset) { set_error("%s: col_offset + nc must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (nq == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  mmf_simtopk_opts exact{};   // AUTO means the exact scan here, whatever the (d, k) range
  if (opts) exact = *opts;
  exact.precision = MMF_PREC_EXACT;
  return run_simtopk_combined_xy(who, Fq, Pq, nq, Fc, Pc, nc, d, dp, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, out_idx,
                                 out_val, &exact, stats, device_id, hip_stream);
}

int64_t mmf_segmented_exact_table(const int64_t* x_ptr_host, const int64_t* y_ptr_host, int64_t n_segments, int k, int exclude_self,
                                  int col_splits, int64_t* table_host, int64_t capacity, int* lists_out) {
  const char* who = "segmented_exact_table";
  if (!y_ptr_host) y_ptr_host = x_ptr_host;
  MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, kAnyRows));
  MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, kAnyRows));
  if (k < 1) { set_error("%s: k must be >= 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (col_splits < 0 || (col_splits & (col_splits - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, col_splits); return MMF_E_INVALID; }
  int ranges = 1;
  const std::vector<int64_t> tab = seg_exact_table(x_ptr_host, y_ptr_host, n_segments, k, exclude_self, col_splits, &ranges, nullptr);
  const int64_t grid = (int64_t)tab.size() / 8;
  if (table_host) {
    if (capacity < grid) { set_error("%s: table of %lld entries needed", who, (long long)grid); return MMF_E_INVALID; }
    if (grid > 0) memcpy(table_host, tab.data(), tab.size() * 8);
  }
  if (lists_out) *lists_out = 2 * ranges;
  return grid;
}

}  // extern "C"

// ---- mmf_simtopk_segmented_fast_anyk (include/ext/mmf_hg_seg_anyk.h) ------------------------------------------
// The passes of fast_anyk_run over the images and the work table of the segmented body (mmf::mmf_simtopk_segmented); d <= 1024 the
// narrow scan, above it (mmf_simtopk_segmented_wide_anyk) `wide`: the wide scan's padded dim, 128-row tiles and
// 32-entry lists, a forced opts->col_splits under the body's bounds (automatic: one range per segment) with one table entry and one
// list pair per range, no id scratch, its launches in the narrow ones' slots and no overflow lists (a crowded row is flagged).
// r: checked, begun, n > 0, r.precision MMF_PREC_FAST or _FAST_BF16, k + self beyond one pass.  A segment is
// SERVED when it has rows and at least k admissible columns; the others go through the exact launch loop in pass 0, as in the body.
// Pass 0: the body's launches at the full depth, K entries into the k-wide output rows, every served row's floor left behind (the
// flagged ones by the exact pass, gathered per segment).  A later pass: ceilings by operand position, the same device work table
// under them, the re-rank into staging rows, count, one yield for the whole call, emit, and the exact rescan — one gathered group
// per segment — of the served rows that were flagged or short.  The floors' ids are rows of Y (what the call-wide re-rank leaves and
// anyk_count compares); an exact pass over one segment's columns reads and leaves ids local to them: launch_floor_rebase on both sides.
// A served segment that runs out of unemitted columns (adm - done < K) stays in the work table: its lists come up short, the re-rank
// flags its rows and they take the rescan.
namespace mmf {

static int segmented_anyk_run(Request& r, bool self, const int64_t* xp, const int64_t* yp, int64_t S, const mmf_simtopk_opts* opts,
                              mmf_fast_anyk_info* info) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const int64_t n = r.n, m = r.m, d = r.d;
  const int k = r.k, self1 = r.exclude_self ? 1 : 0, depth = anyk_depth(d), K = depth - self1;
  const bool f16 = r.precision == MMF_PREC_FAST, profile = r.profile;
  const bool wide = d > 1024;   // the wide scan's sizes and launches, column ranges per segment, no id scratch
  mmf_simtopk_stats* stats = r.stats;
  const int dp = wide ? scan_b16w_dp(d) : scan_bf16_dp(d), qt = wide ? scan_b16w_queries_per_block() : scan_b16_queries_per_block(dp);
  const int kTile = wide ? scan_b16w_col_tile() : 32, bcap = wide ? scan_b16w_cap(depth) : scan_bf16_cap(depth, dp);

  // ---- the body's tables: column ranges, work table, position -> row gathers; and per row the first row of Y of its segment -------
  std::vector<int64_t> adm(S);
  std::vector<char> on_fast(S, 0);
  int64_t unserved_rows = 0, n_served = 0;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
    adm[g] = admissible_columns(xp[g], ng, yp[g], mg, r.exclude_self);
    if (ng == 0) continue;
    if (adm[g] < k) { unserved_rows += ng; continue; }
    if (!wide && (mg + kTile - 1) / kTile * kTile * (int64_t)dp * 2 >= (int64_t(1) << 32)) {   // the narrow tile DMA's 32-bit offsets
      set_error("%s: segment %lld has %lld candidate rows, over 4 GiB of 16-bit operands", who, (long long)g, (long long)mg);
      return MMF_E_UNSUPPORTED;
    }
    on_fast[g] = 1;
    n_served += ng;
  }
  // wide, the body's rule: a forced count is taken while select's capacity per row holds 2 x splits lists; each
  // segment caps its count at its own tile count, rounded down to a power of two.  Narrow: one range per segment.
  int call_splits = 1, max_splits = 1;
  if (wide) {
    int64_t R = 0;
    for (int64_t g = 0; g < S; ++g)
      if (on_fast[g]) R += (xp[g + 1] - xp[g] + qt - 1) / qt;
    const int forced = opts ? opts->col_splits : 0;
    const auto fits = [&](int sp) { return 2 * sp * bcap <= 1024 - kSpillCap; };
    if (forced > 0) { while (call_splits < forced && fits(2 * call_splits)) call_splits <<= 1; }
    else if (wide_seg_auto_splits()) { while (R > 0 && R * call_splits < 256 && fits(2 * call_splits)) call_splits <<= 1; }
  }
  std::vector<int32_t> sched, col0(n, 0), served_rows;
  served_rows.reserve((size_t)n_served);
  int64_t nq_pos = 0, mc_pos = 0;
  for (int64_t g = 0; g < S; ++g) {
    if (!on_fast[g]) continue;
    const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
    const int64_t tiles = (mg + kTile - 1) / kTile;
    const int64_t t0 = mc_pos / kTile;
    int sp = 1;                                   // column ranges of this segment: one table entry and one list pair each
    while (2 * sp <= call_splits && 2 * sp <= tiles) sp <<= 1;
    if (sp > max_splits) max_splits = sp;
    const int64_t tps = (tiles + sp - 1) / sp;
    for (int64_t b = 0; b < ng; b += qt) {
      for (int c = 0; c < sp; ++c) {
        const int64_t tb = std::min(t0 + c * tps, t0 + tiles), te = std::min(tb + tps, t0 + tiles);
        const int32_t e[8] = {(int32_t)(nq_pos + b), (int32_t)(xp[g] + b), (int32_t)(ng - b < qt ? ng - b : qt), (int32_t)tb,
                              (int32_t)te, (int32_t)(uint32_t)(yp[g] - t0 * kTile), 2 * c, 0};
        sched.insert(sched.end(), e, e + 8);
      }
    }
    for (int64_t i = 0; i < ng; ++i) { col0[xp[g] + i] = (int32_t)yp[g]; served_rows.push_back((int32_t)(xp[g] + i)); }
    nq_pos += (ng + qt - 1) / qt * qt;
    mc_pos += tiles * kTile;
    if (nq_pos >= (int64_t(1) << 31) || mc_pos >= (int64_t(1) << 31)) { set_error("%s: padded images too large", who); return MMF_E_UNSUPPORTED; }
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  std::vector<int32_t> qgather(nq_pos, -1), cgather(mc_pos, -1);
  {
    int64_t qpos = 0, cpos = 0;
    for (int64_t g = 0; g < S; ++g) {
      if (!on_fast[g]) continue;
      const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g];
      for (int64_t i = 0; i < ng; ++i) qgather[qpos + i] = (int32_t)(xp[g] + i);
      for (int64_t j = 0; j < mg; ++j) cgather[cpos + j] = (int32_t)(yp[g] + j);
      qpos += (ng + qt - 1) / qt * qt;
      cpos += (mg + kTile - 1) / kTile * kTile;
    }
  }

  // ---- workspace (slot 0): the body's, then floors, bookkeeping, ceilings and the staging rows -----------------------------------
  const int64_t nq_pad = (nq_pos + 255) / 256 * 256, mc_pad = (mc_pos + 255) / 256 * 256;
  const int lists = 2 * max_splits;   // (narrow: 2)
  const size_t scratch_bytes = wide ? 0 : scan_b16_seg_scratch_bytes(grid, dp, bcap);   // 0 bytes: nothing is carved
  const int64_t n_seed = n;
  const size_t stage = (size_t)n * K;
  size_t need = ws_bytes(n, 4) + ws_bytes(m, 4) + FlagBlock::bytes(n);
  if (grid > 0)
    need += HalfImage::bytes(nq_pad, dp) + HalfImage::bytes(mc_pad, dp) + ws_bytes(4, 4) + ws_bytes(sched.size(), 4) +
            ws_bytes(nq_pos, 4) + ws_bytes(mc_pos, 4) + b16_lists_bytes(n, lists, bcap) +
            ws_bytes(scratch_bytes, 1) + ws_bytes(2 * (size_t)n_seed, 4) + ws_bytes(select_order_bytes(n), 1) +
            5 * ws_bytes(n, 4) + ws_bytes(nq_pad, 4) + ws_bytes(64, 4) + ws_bytes(4, 4) + ws_bytes(stage, 8) + 2 * ws_bytes(stage, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = self ? rx : ws.take<float>(m);
  FlagBlock flags;
  flags.carve(ws, n);
  MMF_TRY(flags.zero(s));

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  uint32_t* max_n = nullptr;
  if (grid > 0) { max_n = ws.take<uint32_t>(4); MMF_HIP(hipMemsetAsync(max_n, 0, 16, s)); }
  MMF_TRY(launch_row_scalars(r.X, n, d, r.dtype, r.metric, rx, max_n, s));
  if (!self && m > 0) MMF_TRY(launch_row_scalars(r.Y, m, d, r.dtype, r.metric, cy, max_n, s));

  // kq entries per row from column out_off0 on for `rows` (served rows, ascending: grouped by segment) by the exact pass, one
  // gathered group per segment; `whole`: also the unserved segments, for what they have (pass 0 only).  Does not synchronise.
  int32_t* d_rows = nullptr; int32_t* d_col0 = nullptr;
  float* fkey = nullptr; uint32_t* fid = nullptr;
  auto exact_rows = [&](const std::vector<int32_t>& rows, int kq, int out_off0, bool floors_in, bool floors_out, bool whole) -> int {
    ExactPass ex(r, rx, cy);
    ex.same = self;
    ex.out_stride = k; ex.out_off0 = out_off0;
    ex.floors_in = floors_in; ex.floors_out = floors_out;
    ex.row_floor_key = fkey; ex.row_floor_id = fid;
    const int64_t cnt = (int64_t)rows.size();
    for (int64_t g = 0, e = 0; g < S; ++g) {
      const int64_t ng = xp[g + 1] - xp[g], mg = yp[g + 1] - yp[g], e0 = e;
      if (on_fast[g]) {
        while (e < cnt && rows[e] < xp[g + 1]) ++e;
        if (e > e0) ex.add(ExactGroup{e0, e - e0, true, yp[g], mg, kq});
      } else if (whole && ng > 0) {   // short of k admissible columns: its top-(m_g - self) first, then -1 / -inf
        MMF_HIP(hipMemsetAsync(r.out_idx + xp[g] * k, 0xff, (size_t)ng * k * 8, s));
        MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.out_val + xp[g] * k), (int)0xff800000u, (size_t)ng * k, s));
        if (adm[g] > 0) ex.add(ExactGroup{xp[g], ng, false, yp[g], mg, (int)adm[g]});
      }
    }
    if (ex.pieces.empty()) return MMF_OK;
    if (!wide && getenv("MMF_SEG_ANYK_DEBUG"))   // diagnosis: what the exact pass is asked for (two launches per piece and internal pass of 44)
      fprintf(stderr, "[mmf segmented anyk] exact pass behind column %d: %lld gathered rows, %zu pieces, %d entries each\n", out_off0,
              (long long)cnt, ex.pieces.size(), kq);
    ex.n_ids = cnt; ex.row_ids = d_rows;
    Workspace aux;   // lists and f32 images in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), ex.floors());
    if (cnt > 0) MMF_TRY(upload_table(s, d_rows, rows.data(), (size_t)cnt * 4));
    if (floors_in) MMF_TRY(launch_floor_rebase(d_rows, cnt, fid, d_col0, false, s));
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
    if (floors_out) MMF_TRY(launch_floor_rebase(d_rows, cnt, fid, d_col0, true, s));
    return MMF_OK;
  };

  if (grid == 0) {   // no segment is served: the launch loop answers the call
    MMF_TRY(t_prep.stop(s));
    MMF_TRY(t_fb.start(profile, s));
    MMF_TRY(exact_rows({}, 0, 0, false, false, true));
    MMF_TRY(t_fb.stop(s));
    MMF_HIP(hipStreamSynchronize(s));
    fill_stats(stats, MMF_PREC_EXACT, 1, 0, t_prep.ms(), t_fb.ms(), 0.f, 0.f, 0, 0, 0, flags.h_tot);
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }

  HalfImage Q, C;
  Q.carve(ws, nq_pad, dp);
  C.carve(ws, mc_pad, dp);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  int32_t* d_qg = ws.take<int32_t>(nq_pos);
  int32_t* d_cg = ws.take<int32_t>(mc_pos);
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  char* scan_scratch = ws.take<char>(scratch_bytes);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)n_seed);
  char* order_scratch = ws.take<char>(select_order_bytes(n));
  fkey = ws.take<float>(n); fid = ws.take<uint32_t>(n);
  int32_t* certified = ws.take<int32_t>(n); int32_t* rescan_rows = ws.take<int32_t>(n);
  d_col0 = ws.take<int32_t>(n); d_rows = rescan_rows;   // (a pass's rescan list is read to the host before the sorted rows take its place)
  float* ceil = ws.take<float>(nq_pad);
  uint32_t* hist = ws.take<uint32_t>(64); uint32_t* rescan_count = ws.take<uint32_t>(4);
  int64_t* sidx = ws.take<int64_t>(stage); float* sval = ws.take<float>(stage); float* skey = ws.take<float>(stage);
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(upload_table(s, d_qg, qgather.data(), (size_t)nq_pos * 4));
  MMF_TRY(upload_table(s, d_cg, cgather.data(), (size_t)mc_pos * 4));
  MMF_TRY(upload_table(s, d_col0, col0.data(), (size_t)n * 4));
  MMF_HIP(hipMemsetAsync(Q.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_TRY(launch_prep_half_gather({r.Y, m, d, r.dtype, r.metric, cy, max_n}, d_cg, mc_pos, C, dp, f16, s));
  MMF_TRY(launch_prep_half_gather({r.X, n, d, r.dtype, r.metric, rx, max_n}, d_qg, nq_pos, Q, dp, f16, s));
  MMF_TRY(t_prep.stop(s));

  ScanB16Panel pn;
  pn.seed = seed; pn.seed_stride = n_seed; pn.share = 0;
  const ScanB16Problem sp(Q, C, n, m, mc_pad, dp, d, f16, r.metric, depth);
  // the served rows among `cnt` device rows, ascending (one more synchronisation)
  auto served_of = [&](const int32_t* dev_rows, int64_t cnt, std::vector<int32_t>* out) -> int {
    std::vector<int32_t> h((size_t)cnt);
    if (cnt > 0) {
      MMF_HIP(hipMemcpyAsync(h.data(), dev_rows, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
    }
    out->clear();
    for (int32_t row : h) {
      const int64_t g = (int64_t)(std::upper_bound(xp, xp + S + 1, (int64_t)row) - xp) - 1;
      if (g >= 0 && g < S && on_fast[g]) out->push_back(row);
    }
    std::sort(out->begin(), out->end());
    return MMF_OK;
  };

  // ---- pass 0: K entries per row, k-wide rows, floors left ----------------------------------------------------------------------
  // (every scan starts from the body's reset; rows of unserved segments keep empty lists: the re-rank reports them every pass)
  MMF_TRY(reset_b16_lists(L, n, lists, seed, n_seed, s));
  MMF_TRY(t_scan.start(profile, s));
  if (wide) MMF_TRY(launch_scan_b16w_seg(sp, d_sched, grid, lists, L, pn, s));
  else MMF_TRY(launch_scan_b16_seg(sp, d_sched, grid, L, scan_scratch, pn, s));
  MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
  MMF_TRY(t_scan.stop(s));
  SelectProblem q = r.select();
  q.k = K; q.out_stride = k;
  q.rx = rx; q.cy = cy;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = stats ? flags.cand_total : nullptr;
  q.two_pass = true;
  q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
  q.floor_key_out = fkey; q.floor_id_out = fid;
  MMF_TRY(t_sel.start(profile, s));
  MMF_TRY(launch_select(q, L, s));
  MMF_TRY(t_sel.stop(s));
  MMF_TRY(flags.read(stats != nullptr, s));
  std::vector<int32_t> ex_rows;
  MMF_TRY(served_of(flags.fail_rows, flags.h_fail4[0], &ex_rows));
  const int64_t fallback0 = (int64_t)ex_rows.size();
  MMF_TRY(t_fb.start(profile && (fallback0 > 0 || unserved_rows > 0), s));
  MMF_TRY(exact_rows(ex_rows, K, 0, false, true, true));
  MMF_TRY(t_fb.stop(s));
  if (!wide) MMF_HIP(hipStreamSynchronize(s));   // (the narrow entry has always waited for pass 0's exact rows here)
  {
    const int64_t overflow_rows = flags.h_fail4[1] < (uint32_t)fallback0 ? flags.h_fail4[1] : fallback0;
    fill_stats(stats, r.precision, max_splits, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback0, overflow_rows,
               fallback0 - overflow_rows, flags.h_tot);
  }
  anyk_record(info, 0, K, 0, fallback0);

  // ---- later passes ---------------------------------------------------------------------------------------------------------------
  const int64_t budget = n_served / anyk_short_div();
  const AnykStage st{sidx, sval, skey, n, K, 0};
  int done = K;
  auto finish_exact = [&](int pass) -> int {   // every served row, everything that is left
    MMF_TRY(exact_rows(served_rows, k - done, done, true, false, false));
    if (stats) stats->fallback_rows += n_served;
    anyk_record(info, pass, k - done, 0, n_served);
    return MMF_OK;
  };
  for (int pass = 1; done < k; ++pass) {
    if (pass >= MMF_FAST_ANYK_MAX_PASSES - 1) return finish_exact(pass);
    if (wide) MMF_TRY(launch_scan_b16w_ceilings_gather(sp, d_qg, nq_pos, fkey, rx, max_n, r.lambda, nq_pad, ceil, s));
    else MMF_TRY(launch_scan_b16_ceilings_gather(sp, L.cap, d_qg, nq_pos, fkey, rx, max_n, r.lambda, nq_pad, ceil, s));
    MMF_TRY(reset_b16_lists(L, n, lists, seed, n_seed, s));
    MMF_TRY(flags.zero(s));
    if (wide) MMF_TRY(launch_scan_b16w_seg_ceil(sp, d_sched, grid, lists, L, pn, ceil, s));
    else MMF_TRY(launch_scan_b16_seg_ceil(sp, d_sched, grid, L, scan_scratch, pn, ceil, s));
    MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
    MMF_TRY(launch_select(anyk_stage_select(r, K, sidx, sval, skey, rx, cy, flags, order_scratch), L, s));
    MMF_TRY(launch_anyk_count(st, flags.fail_rows, flags.fail_count, fkey, fid, certified, hist, s));
    uint32_t h[64];
    MMF_HIP(hipMemcpyAsync(h, hist, (size_t)(K + 3) * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    int64_t short_rows = 0;   // (unserved rows are always flagged, never short)
    const int t = anyk_yield(h, std::min(K, k - done), budget, &short_rows);
    if (t < 1) return finish_exact(pass);
    MMF_TRY(launch_anyk_emit(st, certified, t, done, k, r.out_idx, r.out_val, fkey, fid, rescan_rows, rescan_count, s));
    const int64_t listed = (int64_t)h[K + 1] + short_rows;   // the emit kernel's list: flagged rows (the unserved ones among them) and short rows
    int64_t rescan = 0;
    if (listed > unserved_rows) {
      MMF_TRY(served_of(rescan_rows, listed, &ex_rows));
      rescan = (int64_t)ex_rows.size();
      MMF_TRY(exact_rows(ex_rows, t, done, true, done + t < k, false));
      if (stats) stats->fallback_rows += rescan;
    }
    anyk_record(info, pass, t, (int)h[K + 2], rescan);
    done += t;
  }
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

int mmf_segmented_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes) {
  if (d < 1 || k < 1) { set_error("segmented_anyk_plan: need d >= 1 and k >= 1 (got d = %lld, k = %d)", (long long)d, k); return MMF_E_INVALID; }
  if (d <= 1024) return mmf_fast_anyk_plan(d, k, exclude_self, scan_kk, first_yield, min_passes);
  const int self1 = exclude_self ? 1 : 0, kk = k + self1;
  if (!scan_b16w_supported(d, kk)) {
    set_error("segmented_anyk_plan: d = %lld, k = %d is beyond one pass of the wide segmented 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
              (long long)d, k);
    return MMF_E_UNSUPPORTED;
  }
  return anyk_plan(d, k, self1, true, scan_kk, first_yield, min_passes);
}

int mmf_simtopk_segmented_fast_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                    int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                    mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info) {
  const char* who = "simtopk_segmented_fast_anyk";
  const void* Y_in = Y; const int64_t m_in = m; const int64_t* y_ptr_in = y_ptr_host;
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, 0, 0,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the 16-bit scan serves d but not k + self (the checks below refuse what makes this meaningless)
  const bool multi = fast && d >= 1 && d <= 1024 && k >= 1 && !scan_bf16_supported(d, k + (exclude_self ? 1 : 0), in_dtype);
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    if (asked < MMF_PREC_AUTO || asked > MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", who, asked); return MMF_E_INVALID; }
    if (opts && (opts->col_splits != 0 || opts->select_wait_event)) {
      set_error("%s: col_splits and select_wait_event are not supported", who);
      return MMF_E_UNSUPPORTED;
    }
    if (fast && d > 1024 && r.kk > 20) {
      set_error("%s: d = %lld, k = %d is beyond one pass of the wide segmented 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
                who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }));
  if (r.stats) r.stats->near_rows = -1;   // the query order is never probed here
  if (n == 0) return MMF_OK;
  if (!fast) {   // mmf_simtopk_segmented_exact behind its checks
    MMF_TRY(run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f));
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (!multi) {   // one pass serves: the call IS mmf_simtopk_segmented (above 1024: the wide segmented scan)
    mmf_simtopk_opts one{};
    if (opts) one = *opts;
    one.precision = prec;
    MMF_TRY(mmf::mmf_simtopk_segmented(who, true, X, n, Y_in, m_in, d, in_dtype, metric, lambda, k, exclude_self, x_ptr_host, y_ptr_in,
                                       n_segments, out_idx, out_val, &one, r.stats, device_id, hip_stream));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return segmented_anyk_run(r, self, x_ptr_host, y_ptr_host, n_segments, opts, info);
}

}  // extern "C"

// ---- mmf_simtopk_cross_segments_fast_anyk (include/ext/mmf_hg_cross_seg_anyk.h) --------------------------------
// The passes of fast_anyk_run over the images, the work table and the per-row mask of run_cross_segments16; d <= 1024 the narrow
// scan, above it (mmf_simtopk_cross_segments_wide_anyk) `wide`: the wide scan's padded dim, cross_segw_table, 32-entry
// lists, no id scratch, no shared thresholds, its launches in the narrow ones' slots and no overflow lists (a crowded row is flagged).
// r: checked, begun, n > 0, r.precision MMF_PREC_FAST or _FAST_BF16, k beyond one pass; the entry has refused every
// segment short of k columns outside itself, so every row is served.  Nothing is excluded by identity (a row's self lies inside its
// masked segment), so a pass is K = 44 / 20 entries deep.  Prep happens once: row scalars, the plain 16-bit images, the work table
// at the full depth and the rows' bounds.  Pass 0: the one-pass call's launches at depth K into the k-wide rows, every row's floor
// left behind (the flagged ones by the exact cross scan).  A later pass: ceilings by row, the same device work table under them
// (launch_scan_b16_xseg_ceil / launch_scan_b16w_xseg_ceil), the audit, the re-rank into staging rows, count, one yield for the whole
// call, emit, and the exact rescan of the rows that were flagged or short.  Floor ids are rows of all of Y on both sides: no rebase.
// A row that runs out of unemitted columns outside its segment stays in the table: its lists come up short, the re-rank flags it
// and it takes the rescan.
namespace mmf {

// cross_flagged with a depth, an output column offset and floors: kq entries per row from column out_off on for the gathered rows
// `rows` (ascending, so grouped by segment — they may lie in every segment of the call), each row from its floor (floors_in) and
// leaving its new one (floors_out); row_floor_key / row_floor_id are indexed by row of X, ids are rows of all of Y.  ONE table-driven
// launch of the exact cross kernel and one re-rank per 44 entries (launch_scan_f32_seg reads the floors by launch position:
// launch_floor_move before and after).  Images, table, lists and floors live in the second workspace slot.  No synchronisation:
// the re-rank adds the rows it cannot certify (an internal invariant: none) to *fail_word, which the caller reads at its next one.
static int cross_flagged_from(const Request& r, const float* rx, const float* cy, const std::vector<int32_t>& rows, const int64_t* xp,
                              const int64_t* yp, int64_t S, int kq, int out_off, bool floors_in, bool floors_out, float* row_floor_key,
                              uint32_t* row_floor_id, uint32_t* fail_word) {
  const hipStream_t s = r.call.s;
  const int64_t F = (int64_t)rows.size();
  if (F == 0 || kq < 1) return MMF_OK;
  std::vector<int64_t> fp((size_t)S + 1, 0);
  for (int64_t g = 0, e = 0; g < S; ++g) {
    while (e < F && rows[e] < xp[g + 1]) ++e;
    fp[g + 1] = e;
  }
  const int k_pass_max = 44, k_tab = std::min(kq, k_pass_max);
  int ranges = 1;
  const std::vector<int64_t> tab = cross_seg_table(fp.data(), yp, S, k_tab, 0, &ranges);
  const int64_t grid = (int64_t)tab.size() / 8;
  const int cap = scan_f32_cap(k_tab), lists = 2 * ranges;
  const size_t list_words = (size_t)F * lists;
  Workspace aux;
  MMF_TRY(r.call.workspace(ws_bytes(prep_f32_bytes(r.m, r.d), 1) + ws_bytes(prep_f32_bytes(F, r.d), 1) + ws_bytes(F, 4) +
                               ws_bytes(tab.size(), 8) + ExactLists::bytes(F, list_words, cap, true),
                           &aux, 1));
  float* Yp = reinterpret_cast<float*>(aux.take<char>(prep_f32_bytes(r.m, r.d)));
  float* Xe = reinterpret_cast<float*>(aux.take<char>(prep_f32_bytes(F, r.d)));
  int32_t* d_rows = aux.take<int32_t>(F);
  int64_t* d_tab = aux.take<int64_t>(tab.size());
  ExactLists B;
  B.carve(aux, F, list_words, cap, true);
  MMF_TRY(upload_table(s, d_rows, rows.data(), (size_t)F * 4));
  MMF_TRY(upload_table(s, d_tab, tab.data(), tab.size() * 8));
  MMF_TRY(launch_prep_f32(r.Y, r.m, r.d, r.dtype, nullptr, Yp, s));
  MMF_TRY(launch_prep_f32(r.X, F, r.d, r.dtype, d_rows, Xe, s));
  MMF_TRY(B.zero(s));
  MMF_HIP(hipMemsetAsync(B.L.cnt, 0, list_words * 4, s));   // the slots of ranges a block does not use stay empty
  if (floors_in) MMF_TRY(launch_floor_move(d_rows, F, row_floor_key, row_floor_id, B.floor_key, B.floor_id, false, s));
  CandLists L = B.L;
  L.lists = lists; L.cap = cap;
  ScanProblem sp{};
  sp.X = r.X; sp.n = r.n; sp.Y = r.Y; sp.m = r.m; sp.Xp = Xe; sp.Yp = Yp; sp.d = r.d; sp.dtype = r.dtype; sp.metric = r.metric;
  sp.lambda = r.lambda; sp.rx = rx; sp.cy = cy; sp.row_ids = d_rows; sp.n_rows = F; sp.col_splits = ranges;
  SelectProblem q = r.select();
  q.rx = rx; q.cy = cy; q.row_ids = d_rows; q.n_rows = F; q.out_stride = r.k;
  q.fail_rows = B.fail_rows; q.fail_count = fail_word; q.cand_total = nullptr;
  for (int done = 0; done < kq; done += k_pass_max) {   // more than 44 entries (the finishing case): passes of 44 from floor to floor
    const int kp = std::min(kq - done, k_pass_max);
    const bool more = done + kp < kq || floors_out;
    sp.kk = kp;
    if (done > 0 || floors_in) { sp.floor_key = B.floor_key; sp.floor_id = B.floor_id; }
    MMF_TRY(launch_scan_f32_seg(sp, L, d_tab, grid, s, true));
    q.k = kp; q.out_off = out_off + done;
    q.floor_key_out = more ? B.floor_key : nullptr; q.floor_id_out = more ? B.floor_id : nullptr;
    MMF_TRY(launch_select(q, L, s));
  }
  if (floors_out) MMF_TRY(launch_floor_move(d_rows, F, row_floor_key, row_floor_id, B.floor_key, B.floor_id, true, s));
  return MMF_OK;
}

static int cross_anyk_run(Request& r, bool self, const int64_t* xp, const int64_t* yp, int64_t S, const mmf_simtopk_opts* opts,
                          mmf_fast_anyk_info* info) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const int64_t n = r.n, m = r.m;
  const int k = r.k, depth = anyk_depth(r.d), K = depth;
  const bool profile = r.profile, f16 = (r.precision == MMF_PREC_FAST);
  const bool wide = r.d > 1024;   // run_cross_segments16's wide pieces, launch_scan_b16w_ceilings / _xseg_ceil under the ceilings
  mmf_simtopk_stats* stats = r.stats;
  const int dp = wide ? scan_b16w_dp(r.d) : scan_bf16_dp(r.d), bcap = wide ? scan_b16w_cap(depth) : scan_bf16_cap(depth, dp);
  const int forced = opts ? opts->col_splits : 0;
  int lists = 2;
  const std::vector<int32_t> sched = wide ? cross_segw_table(xp, yp, S, bcap, kCross16Budget, forced, &lists)
                                          : cross_seg16_table(xp, yp, S, scan_b16_queries_per_block(dp), dp, bcap, kCross16Budget, forced, &lists);
  if (!wide && lists < 0) {
    set_error("%s: a column run of the %lld rows of Y exceeds 4 GiB of 16-bit operands at padded dim %d", who, (long long)m, dp);
    return MMF_E_UNSUPPORTED;
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  const int64_t n_pad = (n + 255) / 256 * 256, m_pad = (m + 255) / 256 * 256;
  // per row of X: first row and row count of the columns it may not take; padding rows exclude nothing
  std::vector<uint32_t> bounds((size_t)n_pad * 2, 0u);
  for (int64_t g = 0; g < S; ++g)
    for (int64_t i = xp[g]; i < xp[g + 1]; ++i) { bounds[2 * i] = (uint32_t)yp[g]; bounds[2 * i + 1] = (uint32_t)(yp[g + 1] - yp[g]); }

  // ---- workspace (slot 0): the one-pass call's at the pass depth, then floors, bookkeeping, ceilings and the staging rows ---------
  const size_t scratch_bytes = wide ? 0 : scan_b16_seg_scratch_bytes(grid, dp, bcap);   // 0 bytes: nothing is carved
  const size_t stage = (size_t)n * K;
  const size_t need = ws_bytes(n, 4) + (self ? 0 : ws_bytes(m, 4)) + FlagBlock::bytes(n) + ws_bytes(4, 4) + HalfImage::bytes(n_pad, dp) +
                      (self ? 0 : HalfImage::bytes(m_pad, dp)) + ws_bytes(sched.size(), 4) + ws_bytes(bounds.size(), 4) +
                      b16_lists_bytes(n, lists, bcap) + ws_bytes(scratch_bytes, 1) + ws_bytes(2 * (size_t)n, 4) +
                      ws_bytes(select_order_bytes(n), 1) +
                      4 * ws_bytes(n, 4) + ws_bytes(n_pad, 4) + ws_bytes(64, 4) + 2 * ws_bytes(4, 4) + ws_bytes(stage, 8) + 2 * ws_bytes(stage, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* rx = ws.take<float>(n);
  float* cy = self ? rx : ws.take<float>(m);
  FlagBlock flags;
  flags.carve(ws, n);
  MMF_TRY(flags.zero(s));
  uint32_t* max_n = ws.take<uint32_t>(4);
  HalfImage Q, C;
  Q.carve(ws, n_pad, dp);
  if (self) C = Q; else C.carve(ws, m_pad, dp);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  uint32_t* d_bounds = ws.take<uint32_t>(bounds.size());
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  char* scan_scratch = ws.take<char>(scratch_bytes);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)n);
  char* order_scratch = ws.take<char>(select_order_bytes(n));
  float* fkey = ws.take<float>(n); uint32_t* fid = ws.take<uint32_t>(n);
  int32_t* certified = ws.take<int32_t>(n); int32_t* rescan_rows = ws.take<int32_t>(n);
  float* ceil = ws.take<float>(n_pad);
  uint32_t* hist = ws.take<uint32_t>(64); uint32_t* rescan_count = ws.take<uint32_t>(4);
  uint32_t* xfail = ws.take<uint32_t>(4);   // rows the exact rescans could not certify (an internal invariant: none)
  int64_t* sidx = ws.take<int64_t>(stage); float* sval = ws.take<float>(stage); float* skey = ws.take<float>(stage);

  // ---- prep, once ---------------------------------------------------------------------------------------------------------------------
  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  MMF_HIP(hipMemsetAsync(max_n, 0, 16, s));
  MMF_HIP(hipMemsetAsync(xfail, 0, 16, s));
  MMF_TRY(launch_row_scalars(r.X, n, r.d, r.dtype, r.metric, rx, max_n, s));
  if (!self) MMF_TRY(launch_row_scalars(r.Y, m, r.d, r.dtype, r.metric, cy, max_n, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(upload_table(s, d_bounds, bounds.data(), bounds.size() * 4));
  MMF_HIP(hipMemsetAsync(Q.maxima, 0, 16, s));
  if (!self) MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_TRY(launch_prep_half({r.Y, m, r.d, r.dtype, r.metric, cy, max_n}, C, dp, f16, s));
  if (!self) MMF_TRY(launch_prep_half({r.X, n, r.d, r.dtype, r.metric, rx, max_n}, Q, dp, f16, s));
  MMF_TRY(t_prep.stop(s));

  ScanB16Panel pn;
  pn.seed = seed; pn.seed_stride = n; pn.share = (!wide && lists > 2) ? 1 : 0;
  const ScanB16Problem sp(Q, C, n, m, m_pad, dp, r.d, f16, r.metric, depth);
  // `cnt` device rows on the host, ascending (one more synchronisation)
  auto sorted_rows = [&](const int32_t* dev_rows, int64_t cnt, std::vector<int32_t>* out) -> int {
    out->resize((size_t)cnt);
    if (cnt > 0) {
      MMF_HIP(hipMemcpyAsync(out->data(), dev_rows, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
      std::sort(out->begin(), out->end());
    }
    return MMF_OK;
  };
  bool xfail_pending = false;   // an exact rescan has run since *xfail was last read
  auto xfail_check = [&](uint32_t v) -> int {
    xfail_pending = false;
    if (v != 0) { set_error("%s: %u rows failed in the exact scan (internal invariant)", who, v); return MMF_E_INTERNAL; }
    return MMF_OK;
  };

  // ---- pass 0: K entries per row, k-wide rows, floors left ----------------------------------------------------------------------
  MMF_TRY(reset_b16_lists(L, n, lists, seed, n, s));
  MMF_TRY(t_scan.start(profile, s));
  if (wide) MMF_TRY(launch_scan_b16w_xseg(sp, d_sched, grid, d_bounds, lists, L, pn, s));
  else MMF_TRY(launch_scan_b16_xseg(sp, d_sched, grid, d_bounds, L, scan_scratch, pn, s));
  MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
  MMF_TRY(t_scan.stop(s));
  SelectProblem q = r.select();
  q.k = K; q.out_stride = k;
  q.rx = rx; q.cy = cy;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count; q.cand_total = stats ? flags.cand_total : nullptr;
  q.two_pass = true;
  q.order_scratch = getenv("MMF_SELECT_UNORDERED") ? nullptr : order_scratch;
  q.floor_key_out = fkey; q.floor_id_out = fid;
  MMF_TRY(t_sel.start(profile, s));
  MMF_TRY(launch_select(q, L, s));
  MMF_TRY(t_sel.stop(s));
  MMF_TRY(flags.read(stats != nullptr, s));
  std::vector<int32_t> ex_rows;
  const int64_t fallback0 = flags.h_fail4[0];
  MMF_TRY(t_fb.start(profile && fallback0 > 0, s));
  if (fallback0 > 0) {
    MMF_TRY(sorted_rows(flags.fail_rows, fallback0, &ex_rows));
    MMF_TRY(cross_flagged_from(r, rx, cy, ex_rows, xp, yp, S, K, 0, false, true, fkey, fid, xfail));
    xfail_pending = true;
  }
  MMF_TRY(t_fb.stop(s));
  {
    const int64_t overflow_rows = flags.h_fail4[1] < (uint32_t)fallback0 ? flags.h_fail4[1] : fallback0;
    fill_stats(stats, r.precision, lists / 2, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback0, overflow_rows,
               fallback0 - overflow_rows, flags.h_tot);
  }
  anyk_record(info, 0, K, 0, fallback0);

  // ---- later passes ---------------------------------------------------------------------------------------------------------------
  const int64_t budget = n / anyk_short_div();
  const AnykStage st{sidx, sval, skey, n, K, 0};
  int done = K;
  auto finish = [&]() -> int {   // the exact rescans' fail count, when none of the call's synchronisations has read it yet
    if (!xfail_pending) return MMF_OK;
    uint32_t v = 0;
    MMF_HIP(hipMemcpyAsync(&v, xfail, 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    return xfail_check(v);
  };
  auto finish_exact = [&](int pass) -> int {   // every row, everything that is left, from the floors
    ex_rows.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) ex_rows[(size_t)i] = (int32_t)i;
    MMF_TRY(cross_flagged_from(r, rx, cy, ex_rows, xp, yp, S, k - done, done, true, false, fkey, fid, xfail));
    xfail_pending = true;
    if (stats) stats->fallback_rows += n;
    anyk_record(info, pass, k - done, 0, n);
    return finish();
  };
  for (int pass = 1; done < k; ++pass) {
    if (pass >= MMF_FAST_ANYK_MAX_PASSES - 1) return finish_exact(pass);
    if (wide) MMF_TRY(launch_scan_b16w_ceilings(sp, fkey, rx, max_n, r.lambda, n_pad, ceil, s));
    else MMF_TRY(launch_scan_b16_ceilings(sp, L.cap, fkey, rx, max_n, r.lambda, n_pad, ceil, s));
    MMF_TRY(reset_b16_lists(L, n, lists, seed, n, s));
    MMF_TRY(flags.zero(s));
    if (wide) MMF_TRY(launch_scan_b16w_xseg_ceil(sp, d_sched, grid, d_bounds, lists, L, pn, ceil, s));
    else MMF_TRY(launch_scan_b16_xseg_ceil(sp, d_sched, grid, d_bounds, L, scan_scratch, pn, ceil, s));
    MMF_TRY(launch_scan_b16_audit(pn, L.overflow, n, s));
    MMF_TRY(launch_select(anyk_stage_select(r, K, sidx, sval, skey, rx, cy, flags, order_scratch), L, s));
    MMF_TRY(launch_anyk_count(st, flags.fail_rows, flags.fail_count, fkey, fid, certified, hist, s));
    uint32_t h[64], xf = 0;
    MMF_HIP(hipMemcpyAsync(h, hist, (size_t)(K + 3) * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipMemcpyAsync(&xf, xfail, 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    MMF_TRY(xfail_check(xf));
    int64_t short_rows = 0;
    const int t = anyk_yield(h, std::min(K, k - done), budget, &short_rows);
    if (t < 1) return finish_exact(pass);
    MMF_TRY(launch_anyk_emit(st, certified, t, done, k, r.out_idx, r.out_val, fkey, fid, rescan_rows, rescan_count, s));
    const int64_t rescan = (int64_t)h[K + 1] + short_rows;
    if (rescan > 0) {
      MMF_TRY(sorted_rows(rescan_rows, rescan, &ex_rows));
      MMF_TRY(cross_flagged_from(r, rx, cy, ex_rows, xp, yp, S, t, done, true, done + t < k, fkey, fid, xfail));
      xfail_pending = true;
      if (stats) stats->fallback_rows += rescan;
    }
    anyk_record(info, pass, t, (int)h[K + 2], rescan);
    done += t;
  }
  return finish();
}

}  // namespace mmf

extern "C" {

int mmf_cross_segments_anyk_plan(int64_t d, int k, int* scan_kk, int* first_yield, int* min_passes) {
  if (d < 1 || k < 1) { set_error("cross_segments_anyk_plan: need d >= 1 and k >= 1 (got d = %lld, k = %d)", (long long)d, k); return MMF_E_INVALID; }
  if (d <= 1024) return mmf_fast_anyk_plan(d, k, 0, scan_kk, first_yield, min_passes);
  if (!scan_b16w_supported(d, k)) {
    set_error("cross_segments_anyk_plan: d = %lld, k = %d is beyond one pass of the wide cross-segment 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
              (long long)d, k);
    return MMF_E_UNSUPPORTED;
  }
  return anyk_plan(d, k, 0, true, scan_kk, first_yield, min_passes);
}

int mmf_simtopk_cross_segments_fast_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                         float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                         int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                         mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info) {
  const char* who = "simtopk_cross_segments_fast_anyk";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, 0, 0, 0,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the 16-bit scan serves d but not k (the checks below refuse what makes this meaningless)
  const bool multi = fast && d <= 1024 && k >= 1 && !scan_bf16_supported(d, k, in_dtype);
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    if (asked < MMF_PREC_AUTO || asked > MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", who, asked); return MMF_E_INVALID; }
    if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
    if (fast && d > 1024 && !scan_b16w_supported(d, k)) {
      set_error("%s: d = %lld, k = %d is beyond one pass of the wide cross-segment 16-bit scan, which has no ceilings (d <= 1024 is served for any k)",
                who, (long long)d, k);
      return MMF_E_UNSUPPORTED;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    for (int64_t g = 0; g < n_segments; ++g) {
      const int64_t own = y_ptr_host[g + 1] - y_ptr_host[g];
      if (x_ptr_host[g + 1] > x_ptr_host[g] && m - own < k) {
        set_error("%s: segment %lld has %lld admissible columns (m = %lld minus its own %lld rows of Y), k = %d needs at least %d", who,
                  (long long)g, (long long)(m - own), (long long)m, (long long)own, k, k);
        return MMF_E_INVALID;
      }
    }
    return MMF_OK;
  }));
  if (r.stats) r.stats->near_rows = -1;   // the query order is never probed here
  if (n == 0) return MMF_OK;
  if (!fast) {   // mmf_simtopk_cross_segments behind its checks
    MMF_TRY(run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true));
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (!multi) {   // one pass serves: the call IS mmf_simtopk_cross_segments_fast (above 1024: mmf_simtopk_cross_segments_wide)
    MMF_TRY(run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, d > 1024));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return cross_anyk_run(r, self, x_ptr_host, y_ptr_host, n_segments, opts, info);
}

// ---- mmf_simtopk_cross_segments_wide_anyk (include/ext/mmf_hg_cross_segw_anyk.h) -------------------------------
// cross_anyk_run under `wide`, 1024 < d <= 4096: passes of 20 entries over 32-entry lists.
int mmf_cross_segments_wide_anyk_plan(int64_t d, int k, int* scan_kk, int* first_yield, int* min_passes) {
  return mmf_wide_anyk_plan(d, k, 0, scan_kk, first_yield, min_passes);
}

int mmf_simtopk_cross_segments_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                         float lambda, int k, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                         int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                         mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info) {
  const char* who = "simtopk_cross_segments_wide_anyk";
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, 0, 0, 0,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  MMF_TRY(r.call.on_device());
  if (n < 0 || m < 0 || d < 1) { set_error("%s: bad shape n=%lld m=%lld d=%lld", who, (long long)n, (long long)m, (long long)d); return MMF_E_INVALID; }
  if (in_dtype != MMF_F32 && in_dtype != MMF_BF16 && in_dtype != MMF_F16) { set_error("%s: bad in_dtype %d", who, in_dtype); return MMF_E_INVALID; }
  if (n > 0 && !X) { set_error("%s: X is NULL", who); return MMF_E_INVALID; }
  if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) { set_error("%s: n and m must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the wide scan serves d but not k (the checks below refuse what makes this meaningless)
  const bool multi = fast && d > 1024 && d <= 4096 && k >= 1 && !scan_b16w_supported(d, k);
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    if (prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
      set_error("%s: bad precision %d", who, prec);
      return MMF_E_INVALID;
    }
    if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
    if (d <= 1024) {
      set_error("%s: d = %lld is not above 1024: call mmf_simtopk_cross_segments_fast_anyk, which serves d <= 1024 for any k", who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    if (fast && d > 4096) {
      set_error("%s: d = %lld is beyond the wide 16-bit scan (1024 < d <= 4096; MMF_PREC_EXACT serves it)", who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    if (n > 0 && (!out_idx || !out_val)) { set_error("%s: NULL output", who); return MMF_E_INVALID; }
    for (int64_t g = 0; g < n_segments; ++g) {
      const int64_t own = y_ptr_host[g + 1] - y_ptr_host[g];
      if (x_ptr_host[g + 1] > x_ptr_host[g] && m - own < k) {
        set_error("%s: segment %lld has %lld admissible columns (m = %lld minus its own %lld rows of Y), k = %d needs at least %d", who,
                  (long long)g, (long long)(m - own), (long long)m, (long long)own, k, k);
        return MMF_E_INVALID;
      }
    }
    return MMF_OK;
  }));
  if (r.stats) r.stats->near_rows = -1;   // the query order is never probed here
  if (n == 0) return MMF_OK;
  if (!fast) {   // mmf_simtopk_cross_segments behind its checks
    MMF_TRY(run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f, true));
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (!multi) {   // one pass serves: the call IS mmf_simtopk_cross_segments_wide
    MMF_TRY(run_cross_segments16(r, self, x_ptr_host, y_ptr_host, n_segments, opts, true));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return cross_anyk_run(r, self, x_ptr_host, y_ptr_host, n_segments, opts, info);
}

// ---- mmf_simtopk_segmented_wide_anyk (include/ext/mmf_hg_segw_anyk.h) ------------------------------------------
// segmented_anyk_run under `wide`, 1024 < d <= 4096: passes of 20 entries (self's slot included) over 32-entry lists.
int mmf_segmented_wide_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes) {
  return mmf_wide_anyk_plan(d, k, exclude_self, scan_kk, first_yield, min_passes);
}

int mmf_simtopk_segmented_wide_anyk(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int in_dtype, int metric,
                                    float lambda, int k, int exclude_self, const int64_t* x_ptr_host, const int64_t* y_ptr_host,
                                    int64_t n_segments, int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts,
                                    mmf_simtopk_stats* stats, int device_id, void* hip_stream, mmf_fast_anyk_info* info) {
  const char* who = "simtopk_segmented_wide_anyk";
  const void* Y_in = Y; const int64_t m_in = m; const int64_t* y_ptr_in = y_ptr_host;
  const bool self = (Y == nullptr);
  if (self) { Y = X; m = n; y_ptr_host = x_ptr_host; }
  if (info) memset(info, 0, sizeof(*info));
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  Request r{Call(who, device_id, hip_stream), X, n, Y, m, d, in_dtype, metric, lambda, k, exclude_self, 0, 0,
            out_idx, out_val, stats ? stats : (info ? &own_stats : nullptr), opts && opts->profile};
  r.wide_ok = true;
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const bool fast = prec != MMF_PREC_EXACT;
  // more than one pass: the wide scan serves d but not k + self (the checks below refuse what makes this meaningless)
  const bool multi = fast && d > 1024 && d <= 4096 && k >= 1 && !scan_b16w_supported(d, k + (exclude_self ? 1 : 0));
  MMF_TRY(r.check(multi ? MMF_PREC_EXACT : prec, true, [&] {
    MMF_TRY(check_offsets(who, "x_ptr", x_ptr_host, n_segments, 0, 0, n));
    MMF_TRY(check_offsets(who, "y_ptr", y_ptr_host, n_segments, 0, 0, m));
    if (m > 0 && !Y) { set_error("%s: Y is NULL", who); return MMF_E_INVALID; }
    MMF_TRY(check_pow2_splits(who, opts));
    if (asked < MMF_PREC_AUTO || asked > MMF_PREC_FAST_BF16) { set_error("%s: bad precision %d", who, asked); return MMF_E_INVALID; }
    if (opts && opts->select_wait_event) { set_error("%s: select_wait_event is not supported", who); return MMF_E_UNSUPPORTED; }
    if (d <= 1024) {
      set_error("%s: d = %lld is not above 1024: call mmf_simtopk_segmented_fast_anyk, which serves d <= 1024 for any k", who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    if (fast && d > 4096) {
      set_error("%s: d = %lld is beyond the wide 16-bit scan (1024 < d <= 4096; MMF_PREC_EXACT serves it)", who, (long long)d);
      return MMF_E_UNSUPPORTED;
    }
    return MMF_OK;
  }));
  if (r.stats) r.stats->near_rows = -1;   // the query order is never probed here
  if (n == 0) return MMF_OK;
  if (!fast) {   // mmf_simtopk_segmented_exact behind its checks
    MMF_TRY(run_segmented_exact(r, self, x_ptr_host, y_ptr_host, n_segments, opts, nullptr, 0, 0.0f));
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (!multi) {   // one pass serves: the call IS mmf_simtopk_segmented_wide
    mmf_simtopk_opts one{};
    if (opts) one = *opts;
    one.precision = prec;
    MMF_TRY(mmf::mmf_simtopk_segmented(who, true, X, n, Y_in, m_in, d, in_dtype, metric, lambda, k, exclude_self, x_ptr_host, y_ptr_in,
                                       n_segments, out_idx, out_val, &one, r.stats, device_id, hip_stream));
    anyk_record(info, 0, k, 0, r.stats ? r.stats->fallback_rows : 0);
    return MMF_OK;
  }
  r.precision = prec;
  return segmented_anyk_run(r, self, x_ptr_host, y_ptr_host, n_segments, opts, info);
}

}  // extern "C"

// ---- mmf_simtopk_combined_fast_anyk (include/ext/mmf_hg_topk16_anyk.h) ------------------------------------------
// The passes of segmented_anyk_run over the image and the work table of run_simtopk_combined_fast_segmented, for the combined key;
// one graph is a batch of one segment.  r: begun, n > 0, F against itself (MMF_F32, MMF_RBF, r.lambda = lambda_h), r.precision
// MMF_PREC_FAST or _FAST_BF16, k + self > 20, at least one SERVED segment (rows and at least k admissible columns); the others go
// through the exact launch loop in pass 0, as in the one-pass entry.
// Pass 0: that entry's launches at depth 20, K = 20 - self entries into the k-wide output rows, every served row's floor left behind
// (the PASS re-rank's floor slot; the flagged rows by the exact pass, gathered per segment).  A later pass: ceilings by row from the
// floors (launch_scan_b16c_ceilings), the same device work table under them, the combined re-rank into staging rows with the
// canonical key of every entry, count, one yield for the whole call, emit (the bookkeeping kernels of mmf_fast_anyk.hip, unchanged),
// and the exact rescan — one gathered group per segment, the exact scan of the combined key over gathered rows — of the served rows
// that were flagged or short.  The floors' ids are rows of F (what the call-wide re-rank leaves and anyk_count compares); an exact
// pass over one segment's columns reads and leaves ids local to them: launch_floor_rebase on both sides.
namespace mmf {

static int combined_fast_anyk_run(Request& r, const float* P, int dpos, float lambda_g, const int64_t* ptr, int64_t S,
                                  const mmf_simtopk_opts* opts, mmf_fast_anyk_info* info) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const float* F = static_cast<const float*>(r.X);
  const int64_t n = r.n, d = r.d;
  const int k = r.k, self1 = r.exclude_self ? 1 : 0, depth = 20, K = depth - self1;
  const bool f16 = r.precision == MMF_PREC_FAST, profile = r.profile;
  mmf_simtopk_stats* stats = r.stats;
  const int dpf = scan_b16c_dp(d), bcap = scan_b16c_cap(depth);

  // ---- the one-pass entry's tables: served segments, column ranges, work table, position -> row gather; per row its segment's first row
  std::vector<char> served((size_t)S, 0);
  int64_t R = 0, n_pos = 0, unserved_rows = 0, n_served = 0;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = ptr[g + 1] - ptr[g];
    if (ng == 0) continue;
    if (ng - self1 < k) { unserved_rows += ng; continue; }
    served[(size_t)g] = 1;
    n_served += ng;
    R += (ng + 127) / 128;
    n_pos += (ng + 127) / 128 * 128;
  }
  if (R == 0) { set_error("%s: no served segment (internal invariant)", who); return MMF_E_INTERNAL; }
  if (n_pos >= (int64_t(1) << 31)) { set_error("%s: the padded image of %lld positions is too large", who, (long long)n_pos); return MMF_E_UNSUPPORTED; }
  int call_splits = 1, max_splits = 1;
  {
    const int forced = opts ? opts->col_splits : 0;
    const auto fits = [&](int sp) { return 2 * sp * bcap <= 1024; };
    if (forced > 0) { while (call_splits < forced && fits(2 * call_splits)) call_splits <<= 1; }
    else { while (R * call_splits < 256 && 2 * call_splits <= combined_fast_seg_auto_splits() && fits(2 * call_splits)) call_splits <<= 1; }
  }
  std::vector<int32_t> sched, gather((size_t)n_pos, -1), col0((size_t)n, 0), served_rows;
  served_rows.reserve((size_t)n_served);
  {
    int64_t pos = 0;
    for (int64_t g = 0; g < S; ++g) {
      if (!served[(size_t)g]) continue;
      const int64_t ng = ptr[g + 1] - ptr[g], tiles = (ng + 127) / 128, t0 = pos / 128;
      int sp = 1;
      while (2 * sp <= call_splits && 2 * sp <= tiles) sp <<= 1;
      if (sp > max_splits) max_splits = sp;
      const int64_t tps = (tiles + sp - 1) / sp;
      for (int64_t b = 0; b < ng; b += 128) {
        for (int c = 0; c < sp; ++c) {
          const int64_t tb = std::min(t0 + c * tps, t0 + tiles), te = std::min(tb + tps, t0 + tiles);
          const int32_t e[8] = {(int32_t)(pos + b), (int32_t)(ptr[g] + b), (int32_t)std::min<int64_t>(ng - b, 128), (int32_t)tb, (int32_t)te,
                                (int32_t)(uint32_t)(ptr[g] - pos), 2 * c, (int32_t)(ptr[g + 1] - 1)};
          sched.insert(sched.end(), e, e + 8);
        }
      }
      for (int64_t i = 0; i < ng; ++i) {
        gather[(size_t)(pos + i)] = (int32_t)(ptr[g] + i);
        col0[(size_t)(ptr[g] + i)] = (int32_t)ptr[g];
        served_rows.push_back((int32_t)(ptr[g] + i));
      }
      pos += tiles * 128;
    }
  }
  const int64_t grid = (int64_t)sched.size() / 8;
  const int lists = 2 * max_splits;
  const int64_t n_img = (n_pos + 255) / 256 * 256;

  // ---- workspace (slot 0): the one-pass entry's, then floors, bookkeeping, segment offsets, ceilings and the staging rows ----------
  const size_t stage = (size_t)n * K;
  const size_t need = 2 * ws_bytes(n, 4) + ws_bytes(8, 4) + HalfImage::bytes(n_img, dpf) + ws_bytes(sched.size(), 4) + ws_bytes(n_pos, 4) +
                      b16_lists_bytes(n, lists, bcap) + FlagBlock::bytes(n) + ws_bytes(2 * (size_t)n, 4) + 6 * ws_bytes(n, 4) + ws_bytes(64, 4) +
                      ws_bytes(4, 4) + ws_bytes(stage, 8) + 2 * ws_bytes(stage, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(n);
  float* pn = ws.take<float>(n);
  uint32_t* maxw = ws.take<uint32_t>(8);   // word 0: largest chain(f, f) of the batch, word 4: largest chain(p, p)
  HalfImage C;
  C.carve(ws, n_img, dpf);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  int32_t* d_gather = ws.take<int32_t>(n_pos);
  const CandLists L = carve_b16_lists(ws, n, lists, bcap);
  FlagBlock flags;
  flags.carve(ws, n);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)n);
  float* fkey = ws.take<float>(n); uint32_t* fid = ws.take<uint32_t>(n);
  int32_t* certified = ws.take<int32_t>(n); int32_t* rescan_rows = ws.take<int32_t>(n);
  int32_t* d_col0 = ws.take<int32_t>(n);
  int32_t* d_rows = rescan_rows;   // (a pass's rescan list is read to the host before the sorted rows take its place)
  float* ceil = ws.take<float>(n);
  uint32_t* hist = ws.take<uint32_t>(64); uint32_t* rescan_count = ws.take<uint32_t>(4);
  int64_t* sidx = ws.take<int64_t>(stage); float* sval = ws.take<float>(stage); float* skey = ws.take<float>(stage);
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(maxw, 0, 32, s));
  MMF_TRY(flags.zero(s));

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, maxw, s));
  MMF_TRY(launch_row_scalars(P, n, dpos, MMF_F32, MMF_RBF, pn, maxw + 4, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(upload_table(s, d_gather, gather.data(), (size_t)n_pos * 4));
  MMF_TRY(upload_table(s, d_col0, col0.data(), (size_t)n * 4));
  MMF_TRY(launch_prep_half_gather({F, n, d, MMF_F32, MMF_RBF, nf, maxw}, d_gather, n_pos, C, dpf, f16, s));
  MMF_TRY(t_prep.stop(s));

  // kq entries per row from column out_off0 on for `rows` (served rows, ascending: grouped by segment) by the exact pass, one
  // gathered group per segment; `whole`: also the unserved segments, for what they have (pass 0 only)
  auto exact_rows = [&](const std::vector<int32_t>& rows, int kq, int out_off0, bool floors_in, bool floors_out, bool whole) -> int {
    ExactPass ex(r, nf, nf);
    ex.same = true;
    ex.P = P; ex.pn = pn; ex.dp = dpos; ex.lambda_g = lambda_g;
    ex.out_stride = k; ex.out_off0 = out_off0;
    ex.floors_in = floors_in; ex.floors_out = floors_out;
    ex.row_floor_key = fkey; ex.row_floor_id = fid;
    const int64_t cnt = (int64_t)rows.size();
    for (int64_t g = 0, e = 0; g < S; ++g) {
      const int64_t ng = ptr[g + 1] - ptr[g], e0 = e;
      if (served[(size_t)g]) {
        while (e < cnt && rows[(size_t)e] < ptr[g + 1]) ++e;
        if (e > e0) ex.add(ExactGroup{e0, e - e0, true, ptr[g], ng, kq});
      } else if (whole && ng > 0) {   // short of k admissible columns: its top-(n_g - self) first, then -1 / -inf
        MMF_HIP(hipMemsetAsync(r.out_idx + ptr[g] * k, 0xff, (size_t)ng * k * 8, s));
        MMF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.out_val + ptr[g] * k), (int)0xff800000u, (size_t)ng * k, s));
        if (ng - self1 > 0) ex.add(ExactGroup{ptr[g], ng, false, ptr[g], ng, (int)(ng - self1)});
      }
    }
    if (ex.pieces.empty()) return MMF_OK;
    ex.n_ids = cnt; ex.row_ids = d_rows;
    Workspace aux;   // lists and f32 images in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), ex.floors());
    if (cnt > 0) MMF_TRY(upload_table(s, d_rows, rows.data(), (size_t)cnt * 4));
    if (floors_in) MMF_TRY(launch_floor_rebase(d_rows, cnt, fid, d_col0, false, s));
    MMF_TRY(B.zero(s));
    MMF_TRY(ex.run(aux, B));
    if (floors_out) MMF_TRY(launch_floor_rebase(d_rows, cnt, fid, d_col0, true, s));
    return MMF_OK;
  };
  // the served rows among `cnt` device rows, ascending (one more synchronisation)
  auto served_of = [&](const int32_t* dev_rows, int64_t cnt, std::vector<int32_t>* out) -> int {
    std::vector<int32_t> h((size_t)cnt);
    if (cnt > 0) {
      MMF_HIP(hipMemcpyAsync(h.data(), dev_rows, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
    }
    out->clear();
    for (int32_t row : h) {
      if (row < 0 || row >= n) { set_error("%s: flagged row %d outside the %lld rows (internal invariant)", who, row, (long long)n); return MMF_E_INTERNAL; }
      const int64_t g = (int64_t)(std::upper_bound(ptr, ptr + S + 1, (int64_t)row) - ptr) - 1;
      if (g >= 0 && g < S && served[(size_t)g]) out->push_back(row);
    }
    std::sort(out->begin(), out->end());
    return MMF_OK;
  };
  // test hook, every pass: send the first rows down the exact paths (FastTail::run's)
  auto debug_flag_rows = [&]() -> int {
    if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {
      const int64_t f = atoll(e);
      if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < n ? f : n) * 4, s));
    }
    return MMF_OK;
  };

  ScanB16Panel pnl;
  pnl.seed = seed; pnl.seed_stride = n;
  const ScanB16Problem sp(C, C, n, n, n_img, dpf, d, f16, MMF_RBF, depth);
  const ScanB16Comb sc{P, pn, nf, maxw, maxw + 4, dpos, r.lambda, lambda_g};
  SelectProblem q = r.select();
  q.rx = nf; q.cy = nf; q.Pq = P; q.Pc = P; q.pnq = pn; q.pnc = pn; q.dp = dpos; q.lambda_g = lambda_g;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count;

  // ---- pass 0: K entries per row, k-wide rows, floors left ----------------------------------------------------------------------
  // (every scan starts from the same reset; rows of unserved segments keep empty lists: the re-rank reports them every pass)
  MMF_TRY(reset_b16_lists(L, n, lists, seed, n, s));
  MMF_TRY(t_scan.start(profile, s));
  MMF_TRY(launch_scan_b16c_seg(sp, sc, d_sched, grid, lists, L, pnl, s));
  MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, n, s));
  MMF_TRY(debug_flag_rows());
  MMF_TRY(t_scan.stop(s));
  {
    SelectProblem q0 = q;
    q0.k = K; q0.out_stride = k; q0.cand_total = stats ? flags.cand_total : nullptr;
    q0.floor_key_out = fkey; q0.floor_id_out = fid;
    MMF_TRY(t_sel.start(profile, s));
    MMF_TRY(launch_rerank_combined(q0, L, s));
    MMF_TRY(t_sel.stop(s));
  }
  MMF_TRY(flags.read(stats != nullptr, s));
  std::vector<int32_t> ex_rows;
  MMF_TRY(served_of(flags.fail_rows, flags.h_fail4[0], &ex_rows));
  const int64_t fallback0 = (int64_t)ex_rows.size();
  MMF_TRY(t_fb.start(profile && (fallback0 > 0 || unserved_rows > 0), s));
  MMF_TRY(exact_rows(ex_rows, K, 0, false, true, true));
  MMF_TRY(t_fb.stop(s));
  {
    const int64_t overflow_rows = flags.h_fail4[1] < (uint32_t)fallback0 ? flags.h_fail4[1] : fallback0;
    fill_stats(stats, r.precision, max_splits, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback0, overflow_rows,
               fallback0 - overflow_rows, flags.h_tot);
  }
  anyk_record(info, 0, K, 0, fallback0);

  // ---- later passes ---------------------------------------------------------------------------------------------------------------
  const int64_t budget = n_served / anyk_short_div();
  const AnykStage st{sidx, sval, skey, n, K, 0};
  int done = K;
  auto finish_exact = [&](int pass) -> int {   // every served row, everything that is left
    MMF_TRY(exact_rows(served_rows, k - done, done, true, false, false));
    if (stats) stats->fallback_rows += n_served;
    anyk_record(info, pass, k - done, 0, n_served);
    return MMF_OK;
  };
  for (int pass = 1; done < k; ++pass) {
    if (pass >= MMF_FAST_ANYK_MAX_PASSES - 1) return finish_exact(pass);
    MMF_TRY(launch_scan_b16c_ceilings(sp, sc, d_gather, n_pos, fkey, ceil, s));
    MMF_TRY(reset_b16_lists(L, n, lists, seed, n, s));
    MMF_TRY(flags.zero(s));
    MMF_TRY(launch_scan_b16c_seg_ceil(sp, sc, d_sched, grid, lists, L, pnl, ceil, s));
    MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, n, s));
    MMF_TRY(debug_flag_rows());
    {
      SelectProblem qs = q;   // K entries per row into the K-wide staging rows, with their keys
      qs.k = K; qs.out_idx = sidx; qs.out_val = sval; qs.key_out = skey; qs.out_stride = K;
      MMF_TRY(launch_rerank_combined_ext(qs, L, s));
    }
    MMF_TRY(launch_anyk_count(st, flags.fail_rows, flags.fail_count, fkey, fid, certified, hist, s));
    uint32_t h[64];
    MMF_HIP(hipMemcpyAsync(h, hist, (size_t)(K + 3) * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    int64_t short_rows = 0;   // (unserved rows are always flagged, never short)
    const int t = anyk_yield(h, std::min(K, k - done), budget, &short_rows);
    if (t < 1) return finish_exact(pass);
    MMF_TRY(launch_anyk_emit(st, certified, t, done, k, r.out_idx, r.out_val, fkey, fid, rescan_rows, rescan_count, s));
    const int64_t listed = (int64_t)h[K + 1] + short_rows;   // the emit kernel's list: flagged rows (the unserved ones among them) and short rows
    int64_t rescan = 0;
    if (listed > unserved_rows) {
      MMF_TRY(served_of(rescan_rows, listed, &ex_rows));
      rescan = (int64_t)ex_rows.size();
      MMF_TRY(exact_rows(ex_rows, t, done, true, done + t < k, false));
      if (stats) stats->fallback_rows += rescan;
    }
    anyk_record(info, pass, t, (int)h[K + 2], rescan);
    done += t;
  }
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

int mmf_combined_fast_anyk_plan(int64_t d, int k, int exclude_self, int* scan_kk, int* first_yield, int* min_passes) {
  if (d < 1 || k < 1) { set_error("combined_fast_anyk_plan: need d >= 1 and k >= 1 (got d = %lld, k = %d)", (long long)d, k); return MMF_E_INVALID; }
  if (d > 4096) { set_error("combined_fast_anyk_plan: d = %lld > 4096 is beyond the 16-bit scan of the combined key", (long long)d); return MMF_E_UNSUPPORTED; }
  const int self1 = exclude_self ? 1 : 0, kk = k + self1, per = 20 - self1;
  const bool one = scan_b16c_supported(d, kk) != 0;
  const int depth = one ? kk : 20;
  if (scan_kk) *scan_kk = depth;
  if (first_yield) *first_yield = depth - self1;
  if (min_passes) *min_passes = one ? 1 : 1 + (k - (depth - self1) + per - 1) / per;
  return one ? 0 : 1;
}

int mmf_simtopk_combined_fast_anyk(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                                   int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                                   const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                                   mmf_fast_anyk_info* info) {
  const char* who = "simtopk_combined_fast_anyk";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !std::isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !std::isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const bool segmented = ptr_host != nullptr || n_segments != 0;
  if (segmented) MMF_TRY(check_offsets(who, "ptr_host", ptr_host, n_segments, 0, 0, n));
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  if (d > 4096) { set_error("%s: d = %lld > 4096 is not supported (mmf_simtopk_combined takes any d)", who, (long long)d); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  if (asked != MMF_PREC_AUTO && asked != MMF_PREC_EXACT && asked != MMF_PREC_FAST && asked != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16", who, asked);
    return MMF_E_INVALID;
  }
  MMF_TRY(check_pow2_splits(who, opts));
  if (info) memset(info, 0, sizeof(*info));
  if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }

  const int self1 = exclude_self ? 1 : 0, kk = k + self1;
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  const int64_t one_graph[2] = {0, n};
  const int64_t* ptr = segmented ? ptr_host : one_graph;
  const int64_t S = segmented ? n_segments : 1;
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  mmf_simtopk_stats* st = stats ? stats : (info ? &own_stats : nullptr);
  bool any_served = false;       // a segment with rows and at least k admissible columns
  for (int64_t g = 0; g < S; ++g) any_served |= (ptr[g + 1] - ptr[g] > 0 && ptr[g + 1] - ptr[g] - self1 >= k);
  mmf_simtopk_opts one{};
  if (opts) one = *opts;
  if (prec == MMF_PREC_EXACT || (kk > 20 && !any_served)) {
    // the drivers behind mmf_simtopk_combined_anyk (they also answer a batch in which no segment has k admissible columns: the
    // exact launch loop would take every segment anyway)
    one.precision = MMF_PREC_EXACT;
    if (!segmented) {
      MMF_TRY(run_simtopk_combined(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, one_graph, 1, out_idx, out_val, &one, st, device_id,
                                   hip_stream));
    } else {
      if (st) memset(st, 0, sizeof(*st));
      Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0, out_idx, out_val, st,
                opts && opts->profile};
      r.kk = kk;
      r.precision = MMF_PREC_EXACT;
      MMF_TRY(r.call.begin());
      MMF_TRY(run_segmented_exact(r, true, ptr_host, ptr_host, n_segments, &one, P, (int)dp, lambda_g));
    }
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (kk <= 20) {   // one pass serves: the call IS the one-pass entry
    one.precision = prec;
    if (!segmented) MMF_TRY(run_simtopk_combined_fast(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, out_idx, out_val, &one, st, device_id, hip_stream));
    else MMF_TRY(run_simtopk_combined_fast_segmented(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, ptr_host, n_segments, out_idx, out_val, &one,
                                                     st, device_id, hip_stream));
    anyk_record(info, 0, k, 0, st ? st->fallback_rows : 0);
    return MMF_OK;
  }
  if (st) memset(st, 0, sizeof(*st));
  Request r{Call(who, device_id, hip_stream), F, n, F, n, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self, 0, 0, out_idx, out_val, st,
            opts && opts->profile};
  r.kk = kk;
  r.precision = prec;
  MMF_TRY(r.call.begin());
  return combined_fast_anyk_run(r, P, (int)dp, lambda_g, ptr, S, opts, info);
}

}  // extern "C"

// ---- mmf_simtopk_combined_xy_fast_anyk (include/ext/mmf_hg_topk16_xy_anyk.h) -----------------------------------
// The passes of combined_fast_anyk_run over the image and the work table of xy_fast: queries against candidates, or a row slice of
// the candidates against all of them.  r: begun, as the exact pass wants it (X = the candidates for a slice, whose row slice0 is
// query 0; else the queries), r.precision MMF_PREC_FAST or _FAST_BF16, k + self beyond one pass and nc >= k + self, so every query
// has k admissible candidates and none is unserved.  Pass 0: xy_fast's launches at depth 20, K = 20 - self entries into the k-wide
// output rows, every query's floor left behind (the flagged ones by the exact pass, gathered).  A later pass: ceilings by query
// (launch_scan_b16c_xy_ceilings), the same device work table under them (launch_scan_b16c_xy_ceil), audit, the two-sided re-rank
// into staging rows with canonical keys, count, one yield for the whole call, emit, and the exact two-set scan — one gathered group
// against all candidates — of the queries that were flagged or short, from their floors.
// Numberings.  Lists, thresholds, ceilings, staging rows, floors and the count / emit kernels go by QUERY (0 .. nq - 1); the floors'
// ids are candidate rows (what the re-rank leaves before col_offset, what anyk_count compares after taking col_offset off the staged
// id, and what an exact pass over all candidates reads and leaves: no rebase).  An exact pass goes by row of r.X: query i is row
// x0 + i (x0 = slice0 for a slice, else 0), so it gets the floors' bases moved back by x0 rows and the gathered row ids with x0 added.
namespace mmf {

static int combined_xy_fast_anyk_run(Request& r, const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                                     int64_t slice0, int64_t dp, float lambda_g, int64_t row_offset, const mmf_simtopk_opts* opts,
                                     mmf_fast_anyk_info* info) {
  const char* who = r.call.who;
  const hipStream_t s = r.call.s;
  const bool slice = slice0 >= 0, f16 = r.precision == MMF_PREC_FAST, profile = r.profile;
  const int64_t d = r.d, x0 = slice ? slice0 : 0;
  const int k = r.k, self1 = r.exclude_self ? 1 : 0, depth = 20, K = depth - self1;
  const float lambda_h = r.lambda;
  mmf_simtopk_stats* stats = r.stats;
  const int dpf = scan_b16c_dp(d), bcap = scan_b16c_cap(depth);

  // ---- xy_fast's image and work table at depth 20 ---------------------------------------------------------------------------------
  const int64_t ncp = (nc + 127) / 128 * 128, tiles = ncp / 128, row_blocks = (nq + 127) / 128;
  const int64_t J = slice ? nc : nc + nq;           // rows of the joint numbering: candidates, then the queries unless they are among them
  const int64_t q_row0 = slice ? slice0 : nc;       // the first query's row in it
  const int64_t q_pos0 = slice ? slice0 : ncp;      // ... and its image position
  const int64_t n_img = ncp + (slice ? 128 : row_blocks * 128);
  if (n_img >= (int64_t(1) << 31) || J >= (int64_t(1) << 31)) { set_error("%s: the padded image of %lld positions is too large", who, (long long)n_img); return MMF_E_UNSUPPORTED; }
  int splits = 1;
  const int forced = opts ? opts->col_splits : 0;
  if (forced > 0) { while (splits < forced && splits < 32) splits <<= 1; }
  else { while (row_blocks * splits < 256 && splits < 32) splits <<= 1; }
  while (splits > 1 && (splits > tiles || 2 * splits * bcap > 1024)) splits >>= 1;
  const int lists = 2 * splits;
  const int64_t tps = (tiles + splits - 1) / splits;
  std::vector<int32_t> sched;
  sched.reserve((size_t)row_blocks * splits * 8);
  for (int64_t b = 0; b < nq; b += 128) {
    for (int c = 0; c < splits; ++c) {
      const int64_t tb = std::min(c * tps, tiles), te = std::min(tb + tps, tiles);
      const int32_t e[8] = {(int32_t)(q_pos0 + b), (int32_t)(q_row0 + b), (int32_t)std::min<int64_t>(nq - b, 128), (int32_t)tb, (int32_t)te, 0,
                            2 * c, (int32_t)(nc - 1)};
      sched.insert(sched.end(), e, e + 8);
    }
  }
  const int64_t grid = row_blocks * splits;

  // ---- workspace (slot 0): xy_fast's, then floors (by row of r.X: x0 rows ahead of the first query's), bookkeeping, the identity
  // table, ceilings and the staging rows ---------------------------------------------------------------------------------------------
  const size_t stage = (size_t)nq * K;
  const size_t need = 2 * ws_bytes(J, 4) + ws_bytes(8, 4) + (slice ? 0 : ws_bytes((size_t)J * dp, 4)) + HalfImage::bytes(n_img, dpf) +
                      ws_bytes(sched.size(), 4) + b16_lists_bytes(nq, lists, bcap) + FlagBlock::bytes(nq) + ws_bytes(2 * (size_t)nq, 4) +
                      2 * ws_bytes(x0 + nq, 4) + 4 * ws_bytes(nq, 4) + ws_bytes(64, 4) + ws_bytes(4, 4) + ws_bytes(stage, 8) + 2 * ws_bytes(stage, 4);
  Workspace ws;
  MMF_TRY(r.call.workspace(need, &ws));
  float* nf = ws.take<float>(J);
  float* pn = ws.take<float>(J);
  uint32_t* maxw = ws.take<uint32_t>(8);   // word 0: largest chain(f, f) of both sides, word 4: largest chain(p, p)
  float* Pj = slice ? nullptr : ws.take<float>((size_t)J * dp);   // both sides' positions in the joint numbering
  HalfImage C;
  C.carve(ws, n_img, dpf);
  int32_t* d_sched = ws.take<int32_t>(sched.size());
  const CandLists L = carve_b16_lists(ws, nq, lists, bcap);
  FlagBlock flags;
  flags.carve(ws, nq);
  int32_t* seed = ws.take<int32_t>(2 * (size_t)nq);
  float* fkey_x = ws.take<float>(x0 + nq); uint32_t* fid_x = ws.take<uint32_t>(x0 + nq);   // by row of r.X
  float* fkey = fkey_x + x0; uint32_t* fid = fid_x + x0;                                   // by query
  int32_t* certified = ws.take<int32_t>(nq); int32_t* rescan_rows = ws.take<int32_t>(nq);
  int32_t* d_rows = rescan_rows;   // (a pass's rescan list is read to the host before the sorted rows take its place)
  int32_t* d_iota = ws.take<int32_t>(nq);
  float* ceil = ws.take<float>(nq);
  uint32_t* hist = ws.take<uint32_t>(64); uint32_t* rescan_count = ws.take<uint32_t>(4);
  int64_t* sidx = ws.take<int64_t>(stage); float* sval = ws.take<float>(stage); float* skey = ws.take<float>(stage);
  MMF_HIP(hipMemsetAsync(C.maxima, 0, 16, s));
  MMF_HIP(hipMemsetAsync(maxw, 0, 32, s));
  MMF_TRY(flags.zero(s));

  EventTimer t_prep, t_scan, t_sel, t_fb;
  MMF_TRY(t_prep.start(profile, s));
  MMF_TRY(launch_row_scalars(Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw, s));
  MMF_TRY(launch_row_scalars(Pc, nc, dp, MMF_F32, MMF_RBF, pn, maxw + 4, s));
  MMF_TRY(upload_table(s, d_sched, sched.data(), sched.size() * 4));
  MMF_TRY(launch_anyk_iota(d_iota, nq, s));
  if (slice) {
    MMF_TRY(launch_prep_half({Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw}, C, dpf, f16, s));
  } else {
    // scale and maxima over both sides: the queries' scalars join the same words before either image is written
    MMF_TRY(launch_row_scalars(Fq, nq, d, MMF_F32, MMF_RBF, nf + nc, maxw, s));
    MMF_TRY(launch_row_scalars(Pq, nq, dp, MMF_F32, MMF_RBF, pn + nc, maxw + 4, s));
    MMF_HIP(hipMemcpyAsync(Pj, Pc, (size_t)nc * dp * 4, hipMemcpyDeviceToDevice, s));
    MMF_HIP(hipMemcpyAsync(Pj + nc * dp, Pq, (size_t)nq * dp * 4, hipMemcpyDeviceToDevice, s));
    HalfImage Cc = C;
    Cc.n_pad = ncp;
    MMF_TRY(launch_prep_half({Fc, nc, d, MMF_F32, MMF_RBF, nf, maxw}, Cc, dpf, f16, s));
    MMF_TRY(launch_prep_half({Fq, nq, d, MMF_F32, MMF_RBF, nf + nc, maxw}, C.from_row(ncp, dpf), dpf, f16, s));
  }
  MMF_TRY(t_prep.stop(s));

  // kq entries per query from column out_off0 on for `rows` (rows of r.X, ascending) by the exact two-set pass: one gathered group
  // against all candidates
  auto exact_rows = [&](const std::vector<int32_t>& rows, int kq, int out_off0, bool floors_in, bool floors_out) -> int {
    const int64_t cnt = (int64_t)rows.size();
    if (cnt == 0) return MMF_OK;
    ExactPass ex(r, nf + (slice ? 0 : nc), nf);
    ex.same = slice;
    ex.P = slice ? Pc : Pq; ex.pn = pn + (slice ? 0 : nc); ex.dp = (int)dp; ex.lambda_g = lambda_g; ex.out_row0 = x0;
    if (!slice) { ex.Pc = Pc; ex.pnc = pn; }
    ex.out_stride = k; ex.out_off0 = out_off0;
    ex.floors_in = floors_in; ex.floors_out = floors_out;
    ex.row_floor_key = fkey_x; ex.row_floor_id = fid_x;
    ex.add(ExactGroup{0, cnt, true, 0, nc, kq});
    ex.n_ids = cnt; ex.row_ids = d_rows;
    Workspace aux;   // lists and f32 images in the second workspace slot
    MMF_TRY(r.call.workspace(ex.image_bytes() + ex.list_bytes(), &aux, 1));
    ExactLists B;
    B.carve(aux, ex.rows_total, ex.list_words, ex.cap(), ex.floors());
    MMF_TRY(upload_table(s, d_rows, rows.data(), (size_t)cnt * 4));
    MMF_TRY(B.zero(s));
    return ex.run(aux, B);
  };
  // `cnt` device queries as rows of r.X, ascending (one more synchronisation)
  auto rows_of = [&](const int32_t* dev_rows, int64_t cnt, std::vector<int32_t>* out) -> int {
    out->assign((size_t)cnt, 0);
    if (cnt > 0) {
      MMF_HIP(hipMemcpyAsync(out->data(), dev_rows, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
      MMF_HIP(hipStreamSynchronize(s));
    }
    for (int32_t& row : *out) {
      if (row < 0 || row >= nq) { set_error("%s: flagged row %d outside the %lld queries (internal invariant)", who, row, (long long)nq); return MMF_E_INTERNAL; }
      row += (int32_t)x0;
    }
    std::sort(out->begin(), out->end());
    return MMF_OK;
  };
  // test hook, every pass: send the first queries down the exact paths (FastTail::run's)
  auto debug_flag_rows = [&]() -> int {
    if (const char* e = getenv("MMF_DEBUG_FLAG_ROWS")) {
      const int64_t f = atoll(e);
      if (f > 0) MMF_HIP(hipMemsetAsync(L.overflow, 1, (size_t)(f < nq ? f : nq) * 4, s));
    }
    return MMF_OK;
  };

  ScanB16Panel pnl;
  pnl.seed = seed; pnl.seed_stride = nq;
  const ScanB16Problem sp(C, C, nq, nc, n_img, dpf, d, f16, MMF_RBF, depth);
  const ScanB16Comb sc{slice ? Pc : Pj, pn, nf, maxw, maxw + 4, (int)dp, lambda_h, lambda_g};
  SelectProblem q = r.select();   // the call-wide re-ranks go by query, as xy_fast's
  q.X = Fq; q.n = nq; q.n_rows = nq; q.row_offset = row_offset;
  q.rx = nf + q_row0; q.cy = nf; q.Pq = Pq; q.Pc = Pc; q.pnq = pn + q_row0; q.pnc = pn; q.dp = (int)dp; q.lambda_g = lambda_g;
  q.fail_rows = flags.fail_rows; q.fail_count = flags.fail_count;

  // ---- pass 0: K entries per query, k-wide rows, floors left ------------------------------------------------------------------------
  MMF_TRY(reset_b16_lists(L, nq, lists, seed, nq, s));
  MMF_TRY(t_scan.start(profile, s));
  MMF_TRY(launch_scan_b16c_xy(sp, sc, d_sched, grid, lists, q_row0, L, pnl, s));
  MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, nq, s));
  MMF_TRY(debug_flag_rows());
  MMF_TRY(t_scan.stop(s));
  {
    SelectProblem q0 = q;
    q0.k = K; q0.out_stride = k; q0.cand_total = stats ? flags.cand_total : nullptr;
    q0.floor_key_out = fkey; q0.floor_id_out = fid;
    MMF_TRY(t_sel.start(profile, s));
    MMF_TRY(launch_rerank_combined(q0, L, s));
    MMF_TRY(t_sel.stop(s));
  }
  MMF_TRY(flags.read(stats != nullptr, s));
  std::vector<int32_t> ex_rows;
  MMF_TRY(rows_of(flags.fail_rows, flags.h_fail4[0], &ex_rows));
  const int64_t fallback0 = (int64_t)ex_rows.size();
  MMF_TRY(t_fb.start(profile && fallback0 > 0, s));
  MMF_TRY(exact_rows(ex_rows, K, 0, false, true));
  MMF_TRY(t_fb.stop(s));
  fill_stats(stats, r.precision, splits, (int)grid, t_prep.ms(), t_scan.ms(), t_sel.ms(), t_fb.ms(), fallback0, flags.h_fail4[1], flags.h_fail4[2],
             flags.h_tot);
  anyk_record(info, 0, K, 0, fallback0);

  // ---- later passes ---------------------------------------------------------------------------------------------------------------
  const int64_t budget = nq / anyk_short_div();
  const AnykStage st{sidx, sval, skey, nq, K, r.col_offset};
  int done = K;
  auto finish_exact = [&](int pass) -> int {   // every query, everything that is left
    std::vector<int32_t> all((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) all[(size_t)i] = (int32_t)(x0 + i);
    MMF_TRY(exact_rows(all, k - done, done, true, false));
    if (stats) stats->fallback_rows += nq;
    anyk_record(info, pass, k - done, 0, nq);
    return MMF_OK;
  };
  for (int pass = 1; done < k; ++pass) {
    if (pass >= MMF_FAST_ANYK_MAX_PASSES - 1) return finish_exact(pass);
    MMF_TRY(launch_scan_b16c_xy_ceilings(sp, sc, q_pos0, q_row0, d_iota, fkey, ceil, s));
    MMF_TRY(reset_b16_lists(L, nq, lists, seed, nq, s));
    MMF_TRY(flags.zero(s));
    MMF_TRY(launch_scan_b16c_xy_ceil(sp, sc, d_sched, grid, lists, q_row0, L, pnl, ceil, s));
    MMF_TRY(launch_scan_b16_audit(pnl, L.overflow, nq, s));
    MMF_TRY(debug_flag_rows());
    {
      SelectProblem qs = q;   // K entries per query into the K-wide staging rows, with their keys
      qs.k = K; qs.out_idx = sidx; qs.out_val = sval; qs.key_out = skey; qs.out_stride = K;
      MMF_TRY(launch_rerank_combined_ext(qs, L, s));
    }
    MMF_TRY(launch_anyk_count(st, flags.fail_rows, flags.fail_count, fkey, fid, certified, hist, s));
    uint32_t h[64];
    MMF_HIP(hipMemcpyAsync(h, hist, (size_t)(K + 3) * 4, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    int64_t short_rows = 0;
    const int t = anyk_yield(h, std::min(K, k - done), budget, &short_rows);
    if (t < 1) return finish_exact(pass);
    MMF_TRY(launch_anyk_emit(st, certified, t, done, k, r.out_idx, r.out_val, fkey, fid, rescan_rows, rescan_count, s));
    const int64_t listed = (int64_t)h[K + 1] + short_rows;   // the emit kernel's list: flagged queries and short ones
    if (listed > 0) {
      MMF_TRY(rows_of(rescan_rows, listed, &ex_rows));
      MMF_TRY(exact_rows(ex_rows, t, done, true, done + t < k));
      if (stats) stats->fallback_rows += listed;
    }
    anyk_record(info, pass, t, (int)h[K + 2], listed);
    done += t;
  }
  return MMF_OK;
}

}  // namespace mmf

extern "C" {

// The checks of mmf_simtopk_combined_xy (mmf_scan_b16c.hip) in their order and wording under this entry's name, without its
// k + self refusals; col_splits as the any-k 16-bit entries check it.
int mmf_simtopk_combined_xy_fast_anyk(const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc,
                                      int64_t d, int64_t dp, float lambda_h, float lambda_g, int k, int exclude_self,
                                      int64_t row_offset, int64_t col_offset, int64_t* out_idx, float* out_val,
                                      const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream,
                                      mmf_fast_anyk_info* info) {
  const char* who = "simtopk_combined_xy_fast_anyk";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (nq < 0) { set_error("%s: nq must be >= 0 (got %lld)", who, (long long)nq); return MMF_E_INVALID; }
  if (nc < 0) { set_error("%s: nc must be >= 0 (got %lld)", who, (long long)nc); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (row_offset < 0) { set_error("%s: row_offset must be >= 0 (got %lld)", who, (long long)row_offset); return MMF_E_INVALID; }
  if (col_offset < 0) { set_error("%s: col_offset must be >= 0 (got %lld)", who, (long long)col_offset); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !std::isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !std::isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (nq > 0 && !Fq) { set_error("%s: Fq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !Pq) { set_error("%s: Pq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Fc) { set_error("%s: Fc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Pc) { set_error("%s: Pc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const int asked = opts ? opts->precision : MMF_PREC_AUTO;
  if (asked != MMF_PREC_AUTO && asked != MMF_PREC_EXACT && asked != MMF_PREC_FAST && asked != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16", who, asked);
    return MMF_E_INVALID;
  }
  MMF_TRY(check_pow2_splits(who, opts));
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int prec = asked == MMF_PREC_AUTO ? MMF_PREC_FAST : asked;
  if (prec != MMF_PREC_EXACT && d > 4096) { set_error("%s: d = %lld > 4096 is not supported (MMF_PREC_EXACT takes any d)", who, (long long)d); return MMF_E_UNSUPPORTED; }
  if (nq >= ((int64_t)1 << 31) - row_offset) { set_error("%s: row_offset + nq must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (nc >= ((int64_t)1 << 31) - col_offset) { set_error("%s: col_offset + nc must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (info) memset(info, 0, sizeof(*info));
  if (nq == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }

  const int self1 = exclude_self ? 1 : 0, kk = k + self1;
  mmf_simtopk_stats own_stats;   // info reports the first pass's flagged rows, which the call counts in its stats
  mmf_simtopk_stats* st = stats ? stats : (info ? &own_stats : nullptr);
  mmf_simtopk_opts one{};
  if (opts) one = *opts;
  if (prec == MMF_PREC_EXACT || nc < kk) {
    // the driver behind mmf_simtopk_combined_xy_anyk; fewer candidates than a query's lists keep (none at all: the fill) are served
    // exactly, as mmf_simtopk_combined_xy serves them
    one.precision = MMF_PREC_EXACT;
    MMF_TRY(run_simtopk_combined_xy(who, Fq, Pq, nq, Fc, Pc, nc, d, dp, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, out_idx,
                                    out_val, &one, st, device_id, hip_stream));
    anyk_record(info, 0, k, 0, 0);
    return MMF_OK;
  }
  if (kk <= 20) {   // one pass serves: the call IS mmf_simtopk_combined_xy's 16-bit path
    one.precision = prec;
    MMF_TRY(run_simtopk_combined_xy(who, Fq, Pq, nq, Fc, Pc, nc, d, dp, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, out_idx,
                                    out_val, &one, st, device_id, hip_stream));
    anyk_record(info, 0, k, 0, st ? st->fallback_rows : 0);
    return MMF_OK;
  }
  // a row slice (Fq / Pq point at the same row of Fc / Pc, nq rows inside nc): run_simtopk_combined_xy's recognition
  int64_t slice0 = -1;
  {
    const uintptr_t fq = reinterpret_cast<uintptr_t>(Fq), fc = reinterpret_cast<uintptr_t>(Fc);
    const size_t row_bytes = (size_t)d * 4;
    if (fq >= fc && (fq - fc) % row_bytes == 0) {
      const int64_t r0 = (int64_t)((fq - fc) / row_bytes);
      if (r0 <= nc - nq && Pq == Pc + r0 * dp) slice0 = r0;
    }
  }
  const bool slice = slice0 >= 0;
  const int64_t x0 = slice ? slice0 : 0;   // query 0 is row x0 of r.X
  if (st) memset(st, 0, sizeof(*st));
  Request r{Call(who, device_id, hip_stream), slice ? Fc : Fq, slice ? nc : nq, Fc, nc, d, MMF_F32, MMF_RBF, lambda_h, k, exclude_self,
            row_offset - x0, col_offset, out_idx, out_val, st, opts && opts->profile};
  r.kk = kk;
  r.precision = prec;
  MMF_TRY(r.call.begin());
  return combined_xy_fast_anyk_run(r, Fq, Pq, nq, Fc, Pc, nc, slice0, dp, lambda_g, row_offset, opts, info);
}

}  // extern "C"
