// mmf_scan_b16w.hip — the WIDE 16-bit scan: f16 / bf16 MFMA candidate generation for feature dims above 1024
// (1024 < d <= 4096, k + self <= 20), where the register-resident scan of mmf_scan_bf16.hip stops.  DESIGN.md §4.15.
//
// scan_b16x_kernel keeps a wave's 32 queries in registers (128 VGPRs at d = 512, split-k wave pairs up to 1024); here
// nothing is resident.  The structure is scan_f32_kernel's: a workgroup = 4 waves owns a macro tile of 128 queries x 128
// candidates, BOTH operands stream through LDS in k-chunks of 64 halves (128 bytes per row, 32 KiB per stage), double
// buffered, one barrier per chunk, and the epilogue runs once per macro tile after the whole d — the larger d is, the less
// it weighs.
//   * Operands are the 16-bit images of launch_prep_half, unchanged, with dp = d rounded up to 128 (pad rows: zeros, bias
//     -inf, so a padding column never reaches a list and no column needs a bounds test).
//   * Staging is buffer-form LDS-DMA, 1 KiB (8 rows x 128 B) per wave instruction, 8 per wave and chunk; LDS stays
//     lane-linear and the 16-byte unit u of tile row r is fetched to unit u ^ ((r >> 1) & 7) — the XOR on the SOURCE
//     address — so the 16 lanes of a ds_read_b128 group (16 rows, one unit) hit 16 distinct bank quads.
//   * v_mfma_f32_16x16x32_{f16,bf16}: wave w owns queries 32 w .. 32 w + 31 (B operand, two 16-query blocks) and sweeps the
//     tile's 128 candidates (A operand, eight 16-row blocks): 16 accumulator tiles, 64 VGPRs, initialised with the
//     candidates' bias cb_j (-n_j / 2 for the L2 metrics, -inf for padding).  C layout as in mmf_scan_bf16.hip: lane l holds
//     column l & 15, rows 4 (l >> 4) + {0..3}, i.e. TWO queries x 4 candidates per tile; the list code keeps "one lane = one
//     query, 16 of every 32 candidates": lane l owns query (l & 15) + 16 ((l >> 4) & 1) and, on the rare slow path, swaps
//     with lane l ^ 16 the values they hold for each other's query.  Lanes l and l ^ 32 own the two halves of one query.
//   * Lists (WideList below): approximate key AND column id in LDS, 8 bytes per entry, CAP = 16 (k + self <= 11) or 32
//     (k + self in 12..20) entries per lane.  The plain launches (launch_scan_b16w) give every row an overflow list in global
//     memory (SpillSink, mmf_dev.h; "Overflow lists" below); the segmented launches have none: there a crowded row is flagged
//     and the exact rescan answers it.
//
// Error margin (the formula of mmf_scan_bf16.hip with KS * 16 read as dp; stored keys carry no slot bits here): with u the
// f32 rows (normalised for cosine, scaled by the common power of two), z = round_16(u), the scanned value G = bias_j + z_i.z_j
// differs from the real-number target Q = bias_j + u_i.u_j by at most
//   E1_i = |dz_i| max|z_j| + |u_i| max|dz_j| + (dp + 8) 2^-24 (|z_i| max|z_j| + max|bias|)
// (products of 16-bit values are exact in f32; the last term bounds the f32 accumulation of dp products and the bias in any
// order), and the canonical f32 key (mapped to Q units) differs from Q by at most E2_i (rounding of the chain and of the
// metric's few f32 ops).  margin_i = 2 (E1_i + E2_i): every column that can be in the canonical top-k has
// G >= (k-th best G) - margin_i.
//
// What a list guarantees: it holds its best CAP keys under (G desc, id asc) among the columns that passed its threshold, and
// a key is DROPPED only from a list that then holds CAP entries ranking before it (the best dropped key is remembered).  The
// threshold is max(proven, lost): proven = (kk-th best key the two lists of the query hold) - margin, a lower bound of the
// final one; lost = the best dropped key — anything below it matters only if the row is not flagged, i.e. if the final
// threshold is above it.  After the scan the row is flagged (launch_scan_b16_audit) iff its best dropped key reaches the best
// threshold proven for it.  A row whose margin band — the columns with G >= (kk-th best G over ALL columns) - margin — holds
// at most CAP columns is therefore never flagged: a dropped key has CAP + 1 columns at or above it, so it lies below the
// band, and every column of the band is still in a list when the thresholds are settled (wide_seed_union_kernel settles them
// across column splits).  A band column that is in neither a list nor the row's overflow list at the end has raised `lost` to
// at least its key, so the audit flags the row.
//
// Overflow lists (the SINK instantiations).  A column is offered to one list pair once and ends in a list, in
// the row's overflow list, or below the threshold; select re-ranks the overflow entries exactly, so ANY hit may be written down
// instead of pushed.  A threshold is only ever proven from keys the lists hold (a subset of the row's columns: a lower bound).
// The policy, for a list whose last compaction left it full (`crowded`, so cnt == CAP) with tband = the pair's kk-th best key
// at that compaction:
//   1. a hit below tband + MMF_BAND_SLACK * margin goes straight to the overflow list and does not touch the list (it could
//      raise the threshold by less than the slack);
//   2. any other hit replaces the list's worst entry and the worst of the CAP + 1 goes to the overflow list;
//   3. after kk such replacements the list asks for a compaction.  Each of them left the list with one more key at or above
//      tband + slack (the key itself, or CAP entries that beat it), CAP >= kk, so the pair's kk-th best is then at least
//      tband + slack: every compaction a crowded list asks for raises its proven threshold by at least the slack, and a list
//      costs at most kk overflow slots per slack of threshold it climbs.
// Without rule 3 a crowded list would never compact of its own accord: drops no longer raise `lost`, the threshold would stay
// where a transient crowd early in the scan left it, and every later hit would pour into the overflow list.
// When the overflow list refuses a key (full, or the two stacks met) the old rule applies to that key: lost, thr = max(thr,
// lost), audited.  One column range per row: the two-stack form (the pair's lower lane fills the row's slots from the front,
// the upper one from the back, no counter; the pair writes front | back << 16 when the scan ends, stacks that met flag the
// row).  Column splits: the counter form, slots reserved in chunks of SpillSink::kChunk (at most 7 wasted slots per lane),
// closed with the empty marker.
// What was written down and has since been proven irrelevant is taken back when the thresholds are settled, so that a transient
// crowd early in a scan costs the re-rank nothing: every lane remembers the best key it wrote (`sunk`).  One column range: at
// every compaction a lane whose best written key lies below the pair's proven threshold empties its stack, so a transient
// crowd does not use the slots up either; stacks are taken to have met if their high-water marks add up to more than the
// slots.  Column splits: the lanes leave the row's best written key in ScanB16WArgs::sunk and wide_seed_union_kernel empties
// the row's overflow list if that key lies below the row's settled threshold (the slots stay used while the scan runs).
// Either way every discarded key lies below a proven threshold: outside the band.
//
// Ceilings (the CEIL instantiations).  A call with more neighbours than one pass holds (mmf_simtopk_wide_anyk) runs
// the plain launch again with a ceiling per query row: ceil_i = map_i(floor key) + E1_i + E2_i (wide_ceil_kernel; E1, E2 as above),
// so that no column ranking after the row's floor is scanned above it.  The epilogue's hit branch sets the gathered values above
// the ceiling to -inf before they are offered; everything said above about lists, thresholds and overflow lists then holds for the
// columns at or below the ceiling.  The cross-segment call's later passes (mmf_simtopk_cross_segments_wide_anyk) run
// the masked table-driven launch under the same ceilings; there is no overflow list on that schedule, so a crowded row is flagged.
// The segmented call's later passes (mmf_simtopk_segmented_wide_anyk) run the table-driven launch under ceilings
// indexed by operand position (wide_ceil_kernel<true> reads the rows' floors through the position -> row table); no overflow list either.
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

namespace {

constexpr int W_NT = 256;                        // threads per workgroup
constexpr int W_QT = 128;                        // queries per macro tile
constexpr int W_CT = 128;                        // candidates per macro tile
constexpr int W_KC = 64;                         // halves per staged chunk
constexpr int W_ROWB = W_KC * 2;                 // bytes per LDS row (128)
constexpr int W_OPB = W_QT * W_ROWB;             // bytes per operand tile of a stage (16 KiB)
constexpr int W_STAGEB = 2 * W_OPB;              // queries, then candidates
constexpr int W_UPR = W_ROWB / 16;               // 16-byte units per row (8)
constexpr int W_RPP = 64 / W_UPR;                // rows per 1 KiB DMA piece (8)
constexpr int W_HP = W_QT / W_RPP;               // pieces per operand tile (16)
constexpr int W_PPW = 2 * W_HP / 4;              // pieces per wave and chunk (8): the first half query pieces
constexpr int W_FSH = 1;                         // unit u of tile row r sits at unit u ^ ((r >> W_FSH) & (W_UPR - 1))
// (chunks of 32 halves — 64-byte rows, two workgroups per CU beside 16-entry lists — measured 27 % slower at N = 16384 and
//  5 % faster at N = 65536, d = 1536; 8 % slower at d = 2560: one chunk size)
constexpr int W_CAP_SMALL = 16;                  // list entries per lane, k + self <= 11
constexpr int W_CAP_BIG = 32;                    // ... k + self in 12..20

typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 wf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t wu32x4 __attribute__((ext_vector_type(4)));

// order-preserving float -> int32 map of the threshold buffers (ScanB16Panel::seed; memset 0x80 = none)
__device__ __forceinline__ int32_t wide_enc(float f) {
  const int32_t b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}

struct ScanB16WArgs {
  const void* ZQ;            // [nq_pad][dp] query side
  const void* ZC;            // [m_pad][dp]  candidate side
  const float* cb;           // [m_pad]
  const float* q_zn; const float* q_rn; const float* q_un;
  const uint32_t* maxima;    // candidate-side maxima
  int64_t n_rows;            // queries
  int64_t tiles_total;       // ceil(m / 128) <= m_pad / 128
  int64_t tiles_per_split;
  int col_splits;
  int dp;                    // multiple of 128
  int d;
  int metric;
  int kk;
  int lists_total;           // lists per query row in cand_cnt / cand_ids
  int list_base;
  int32_t* seed;             // [>= n_rows] best proven threshold per query (wide_enc; atomicMax)
  int32_t* lost;             // [>= n_rows] best dropped key per query
  uint32_t* cand_cnt; uint32_t* cand_ids;
  float* cand_keys;          // approximate keys of the entries, or nullptr
  float* margin_out;         // [n_rows], written with cand_keys
  const int32_t* sched;      // SEG kernels only: [grid][WSEG_ENTRY] work table (launch_scan_b16w_seg)
  // SINK kernels only: the rows' overflow lists (CandLists; SpillSink)
  uint32_t* spill_cnt; uint32_t* spill_ids; int spill_cap; int spill_stacks;
  int32_t* sunk;             // counter form: [>= n_rows] best key written to the row's overflow list (wide_enc; atomicMax), or nullptr
  // XSEG kernels only (launch_scan_b16w_xseg): [n_pad][2] per query row, first row and row count of the columns the row may not
  // take (its own segment's rows of Y); rows of the padding exclude nothing
  const uint32_t* bounds;
  // CEIL kernels only (launch_scan_b16w_ceil): [n_pad] per query row, the largest scanned value the row may still take, in the
  // kernel's own units (bias and 2^(2e) scale included); padding rows: +inf.  Indexed by OPERAND POSITION (qpos), like q_zn / q_rn /
  // q_un: the plain schedule's positions are its rows, and so are the cross-segment (XSEG) one's, whose images are the plain ones
  // (launch_scan_b16w_ceilings fills both); the table-driven (SEG) one's are positions of the segment-padded query image ([nq_pad];
  // launch_scan_b16w_ceilings_gather fills them through the position -> row table)
  const float* ceil;
};

// One entry of the segmented work table: a workgroup = one row block of one segment against one column range of that segment.
// Operands, zn / rn / un and the biases are addressed by image position (both images are padded per segment to whole tiles);
// lists, seed, lost and margin_out by the row of X.
enum {
  WSEG_QPOS = 0,    // position of the row block's first query in the query image (a multiple of 128)
  WSEG_ROW0 = 1,    // row of X of that query
  WSEG_NQ = 2,      // real queries of the block (<= 128)
  WSEG_T0 = 3,      // first and end tile of the column range, in the candidate image (tiles of 128)
  WSEG_T1 = 4,
  WSEG_IDOFF = 5,   // y_ptr[s] - first column of the segment's tiles (mod 2^32): lists hold global rows of Y
  WSEG_SLOT = 6,    // first list slot of this range (2 x split)
  WSEG_ENTRY = 8
};
// Work table entry of the cross-segment scan (cross_segw_table; same entry size, words 0 .. 4 and 6 as above): both images are the
// plain ones of launch_prep_half, so the query position IS the row of X (words 0 and 1 are equal), the id offset is zero, and its
// word and the spare one carry the entry's mask window [w0, w1), in tiles of the candidate image: the tiles of [T0, T1) that hold a
// column some row of the block may not take (w0 == w1: none).
enum { WXSEG_W0 = 5, WXSEG_W1 = 7 };

// The lane-private list: entry e of thread t at keys[e * NT + t] / ids[e * NT + t] (LaneList's layout), approximate keys.
template <int CAP, int NT, bool SINK = false>
struct WideList {
  SpillSink sink;  // SINK only: the row's overflow list
  float tband;     // SINK only: the pair's kk-th best key at the last compaction that left this list crowded
  int repl;        // SINK only: hits that went through replace_worst since the last compaction
  float sunk;      // SINK only: best key this lane wrote to the overflow list and has not taken back; -inf: none
  uint32_t high;   // SINK only, two stacks: the most entries this lane's stack held before it was emptied
  float* keys; uint32_t* ids;
  int cnt;
  float thr;       // max(proven, lost): what a column has to reach
  float proven;    // best (kk-th best key of the pair's lists) - margin seen so far; -FLT_MAX: none
  float lost;      // best dropped key; -inf: none
  bool crowded;    // the last compaction left the list full: hits replace its worst entry, no compaction until a partner asks

  __device__ __forceinline__ void init(float* k, uint32_t* i) {
    keys = k; ids = i; cnt = 0; thr = -kFltMax; proven = -kFltMax; lost = kNegInf; crowded = false;
    if constexpr (SINK) { tband = kNegInf; repl = 0; sunk = kNegInf; high = 0; }
  }
  __device__ __forceinline__ void push(float key, uint32_t id) {
    keys[cnt * NT] = key; ids[cnt * NT] = id; ++cnt;
  }
  static __device__ __forceinline__ long long order64(float key, uint32_t id) {   // (key desc, id asc) as one signed compare
    const int b = __float_as_int(key + 0.0f);
    const int e = b >= 0 ? b : (b ^ 0x7fffffff);
    return (long long)(((unsigned long long)(uint32_t)e << 32) | (unsigned long long)(~id));
  }

  // Wave-wide (EXEC full).  Ranks every entry by counting the entries of its own and of the partner lane's list (lane ^ 32,
  // same wave: its LDS writes are ordered before these reads) that beat it, eight entries per sweep (LaneList::compact).
  // The entry of union rank kk - 1 gives the proven threshold; what lies below the threshold leaves the list — that is no
  // drop: a column below (kk-th best of a subset) - margin cannot be in the final top-kk.
  __device__ __forceinline__ void compact(int kk, float margin) {
    constexpr int BLK = 8;
    const int pofs = (int)((threadIdx.x ^ 32u) - threadIdx.x);
    const int pcnt = __shfl_xor(cnt, 32);
    float t_own = kNegInf;
#pragma nounroll
    for (int e0 = 0; e0 < cnt; e0 += BLK) {
      float kf32[BLK]; long long ke[BLK]; int rk[BLK];
#pragma unroll
      for (int i = 0; i < BLK; ++i) {                   // rows beyond cnt: stale but inside the lane's column; masked below
        const int e = (e0 + i < CAP) ? e0 + i : CAP - 1;
        kf32[i] = keys[e * NT]; ke[i] = order64(kf32[i], ids[e * NT]); rk[i] = 0;
      }
#pragma nounroll
      for (int f = 0; f < cnt; ++f) {
        const long long kf = order64(keys[f * NT], ids[f * NT]);
#pragma unroll
        for (int i = 0; i < BLK; ++i) rk[i] += (kf > ke[i]) ? 1 : 0;
      }
#pragma nounroll
      for (int f = 0; f < pcnt; ++f) {
        const long long kf = order64(keys[f * NT + pofs], ids[f * NT + pofs]);
#pragma unroll
        for (int i = 0; i < BLK; ++i) rk[i] += (kf > ke[i]) ? 1 : 0;
      }
#pragma unroll
      for (int i = 0; i < BLK; ++i)
        if (e0 + i < cnt && rk[i] == kk - 1) t_own = kf32[i];
    }
    const float t = fmaxf(t_own, __shfl_xor(t_own, 32));
    if (t != kNegInf) {                                 // fewer than kk entries in the union: keep collecting everything
      const float p = t - margin;
      if (p > proven) proven = p;
      if (proven > thr) thr = proven;
    }
    int w = 0;
#pragma nounroll
    for (int e = 0; e < cnt; ++e) {
      const float ke = keys[e * NT];
      const uint32_t ie = ids[e * NT];
      if (ke >= thr) { keys[w * NT] = ke; ids[w * NT] = ie; ++w; }
    }
    cnt = w;
    crowded = cnt >= CAP;
    if constexpr (SINK) {
      repl = 0;
      if (crowded && t > tband) tband = t;
      if (sink.stacks && sunk < proven) {              // nothing this lane wrote can matter any more: its stack starts over
        high = sink.cpos > high ? sink.cpos : high;
        sink.cpos = 0; sunk = kNegInf;
      }
    }
  }

  // A hit on a full list (lane-private): the worst of the CAP + 1 under (key desc, id asc) is dropped — CAP entries rank
  // before it — and remembered; nothing below it can matter unless the row is flagged.  SINK: it goes to the row's overflow
  // list instead and is lost only if that refuses it.
  __device__ __forceinline__ void replace_worst(float x, uint32_t id) {
    int wpos = 0;
    float wk = keys[0]; uint32_t wi = ids[0];
#pragma nounroll
    for (int e = 1; e < CAP; ++e) {
      const float ke = keys[e * NT]; const uint32_t ie = ids[e * NT];
      if (better(wk, wi, ke, ie)) { wk = ke; wi = ie; wpos = e; }
    }
    float dropped = x;
    uint32_t dropped_id = id;
    if (better(x, id, wk, wi)) { keys[wpos * NT] = x; ids[wpos * NT] = id; dropped = wk; dropped_id = wi; }
    if constexpr (SINK) {
      ++repl;
      if (sink.put(dropped_id, true)) { sunk = fmaxf(sunk, dropped); return; }
    }
    lost = fmaxf(lost, dropped);
    thr = fmaxf(thr, lost);
  }

  // One 32-candidate sub-tile's 16 values of this lane's query; rowof(r): sub-tile row of element r.  Called by the whole
  // wave when any lane has a hit; only the elements that hold a hit in SOME lane run the push code.
  template <class RowOf>
  __device__ __forceinline__ void offer_tile(const f32x16& v, uint32_t id0, RowOf rowof, int kk, float margin) {
    uint32_t rmask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) rmask |= (__any(v[r] >= thr) ? 1u : 0u) << r;
    while (rmask) {
      const int r = __builtin_ctz(rmask);
      rmask &= rmask - 1;
      const float x = v[r];
      bool hit = x >= thr;
      if constexpr (SINK) {
        // rules 1 - 3 of the header; crowded implies cnt == CAP
        bool band = crowded && x < tband + MMF_BAND_SLACK * margin;
        if (__any(hit && !band && cnt >= CAP && (!crowded || repl >= kk))) {
          compact(kk, margin);
          hit = x >= thr;
          band = crowded && x < tband + MMF_BAND_SLACK * margin;
        }
        if (hit) {
          const uint32_t id = id0 + rowof(r);
          if (band) {
            if (sink.put(id, true)) sunk = fmaxf(sunk, x);
            else { lost = fmaxf(lost, x); thr = fmaxf(thr, lost); }
          } else if (cnt < CAP) push(x, id);
          else replace_worst(x, id);
        }
        continue;
      }
      if (__any(hit && cnt >= CAP && !crowded)) {
        compact(kk, margin);
        hit = x >= thr;
      }
      if (hit) {
        const uint32_t id = id0 + rowof(r);
        if (cnt < CAP) push(x, id);
        else replace_worst(x, id);
      }
    }
  }
};

// 64 KiB of stages + 1 KiB of biases + 32 / 64 KiB of lists: one workgroup per CU
constexpr size_t scan_b16w_lds(int cap) { return (size_t)2 * W_STAGEB + (size_t)2 * W_CT * 4 + (size_t)cap * W_NT * 8; }

// SEG (segmented calls, launch_scan_b16w_seg): the workgroup's row block, column range, id offset and list slot come from the
// work table a.sched instead of blockIdx / col_splits; everything else is shared.  SINK (plain launches only): crowded lists
// write to the rows' overflow lists (header, "Overflow lists").
// XSEG (implies SEG, excludes SINK; mmf_simtopk_cross_segments_wide): every row against the columns OUTSIDE its own
// segment, on the plain images.  A row block is 128 consecutive rows of X whatever the segments; the table leaves out the tiles every
// row of the block excludes, and on the tiles of the entry's mask window the epilogue sets the accumulators of a query's excluded
// columns (a.bounds) to -inf before anything reads them: such a value is below every threshold (the first one is -FLT_MAX), so it
// reaches neither the tile maxima's test, nor a list, nor proven / lost / seed — exactly like the -inf bias of a padding column.
// CEIL (the plain schedule only, with or without SINK; mmf_simtopk_wide_anyk): the later passes of a call with more
// neighbours than one pass holds.  Every query row comes with a ceiling a.ceil[row]; a value above it belongs to a column the row has
// already emitted.  Such a value is above the row's threshold by construction, so it takes the epilogue's hit branch anyway: the
// compare sits THERE, on the lane's 16 gathered values before they are offered — the sub-tile's 14 v_max + two compares are
// untouched, and the ceiling is loaded inside the branch, so the k-loop carries no register for it.  A value set to -inf there
// reaches no list, overflow list or sink slot, proven, lost, seed or threshold.
// CEIL with XSEG (mmf_simtopk_cross_segments_wide_anyk): both images of the
// cross form are the plain ones, so the query position is the row of X and a.ceil[qpos] is the row's ceiling.  Mask and ceiling do not
// meet: the mask writes -inf into the accumulators ahead of the tile maxima, the ceiling compare works on the gathered values inside
// the hit branch and leaves a -inf as it is (-inf > ce is false for every ceiling).
// CEIL with the plain SEG (mmf_simtopk_segmented_wide_anyk): qpos is the position in the segment-padded query image
// and lrow the row of X; the hit branch reads a.ceil[qpos], so the ceilings of a segmented pass are indexed by operand position, like
// the norms (launch_scan_b16w_ceilings_gather).  A padding position inside a segment's last block carries +inf and is not valid anyway.
template <bool F16, int CAP, bool SEG = false, bool SINK = false, bool XSEG = false, bool CEIL = false>
__global__ __launch_bounds__(W_NT, 1) void scan_b16w_kernel(ScanB16WArgs a) {
  static_assert(!CEIL || !SEG || !SINK, "per-row ceilings on a table-driven schedule: no overflow lists");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* stages = smem;                                                   // [2][W_STAGEB]
  float* cbs = reinterpret_cast<float*>(smem + 2 * W_STAGEB);            // [2][W_CT] bias of the tile being accumulated / the next
  float* lkeys = cbs + 2 * W_CT;                                         // [CAP][W_NT]
  uint32_t* lids = reinterpret_cast<uint32_t*>(lkeys + CAP * W_NT);      // [CAP][W_NT]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int g = lane >> 4;                      // row group of the C layout: rows 4 g .. 4 g + 3 of each 16-row block
  const int c16 = lane & 15;
  const int ownb = g & 1;                       // the query block (0 / 1) whose list this lane owns
  const int c = c16 + 16 * ownb;                // own query within the wave

  int slot;                                     // first list slot of this workgroup's column range
  int64_t q0, t_begin, t_end;
  int64_t row0 = 0;                             // SEG: row of X of the block's first query
  int nq = W_QT;                                // SEG: real queries of the block
  uint32_t id_off = 0;                          // SEG: column of the candidate image -> row of Y
  int64_t xw0 = 0, xw1 = 0;                     // XSEG: the entry's mask window, in tiles of the candidate image
  static_assert(!XSEG || (SEG && !SINK), "the cross-segment mask rides on the table-driven schedule, without overflow lists");
  if constexpr (SEG) {
    const int32_t* e = a.sched + (size_t)blockIdx.x * WSEG_ENTRY;
    q0 = e[WSEG_QPOS]; row0 = e[WSEG_ROW0]; nq = e[WSEG_NQ];
    t_begin = e[WSEG_T0]; t_end = e[WSEG_T1]; id_off = (uint32_t)e[WSEG_IDOFF]; slot = e[WSEG_SLOT];
    if (t_begin > t_end) t_begin = t_end;
    if constexpr (XSEG) { id_off = 0u; xw0 = e[WXSEG_W0]; xw1 = e[WXSEG_W1]; }
  } else {
    const int split = blockIdx.x % a.col_splits;
    const int64_t rb = blockIdx.x / a.col_splits;
    q0 = rb * W_QT;
    t_begin = (int64_t)split * a.tiles_per_split;
    t_end = t_begin + a.tiles_per_split;
    if (t_end > a.tiles_total) t_end = a.tiles_total;
    if (t_begin > t_end) t_begin = t_end;
    slot = 2 * split;
  }
  const int nkc = a.dp / W_KC;
  const int64_t steps = (t_end - t_begin) * nkc;

  const int64_t qpos = q0 + 32 * wave + c;      // position in the query image
  const int64_t lrow = SEG ? row0 + 32 * wave + c : qpos;   // row of the lists and of the threshold buffers
  const bool qvalid = SEG ? (32 * wave + c < nq) : (qpos < a.n_rows);

  // margin of this lane's query (see the header): 2 (E1 + E2)
  float margin;
  {
    const float ZB = __uint_as_float(a.maxima[0]), RB = __uint_as_float(a.maxima[1]);
    const float UB = __uint_as_float(a.maxima[2]), CB = __uint_as_float(a.maxima[3]);
    const float zn = a.q_zn[qpos], rn = a.q_rn[qpos], un = a.q_un[qpos];   // arrays are padded to whole row blocks
    const float g_acc = (float)(a.dp + 8) * 5.9604645e-8f;
    const float g_chain = (float)(a.d + 2) * 5.9604645e-8f;
    const float e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB);
    float e2;
    if (a.metric == MMF_DOT) e2 = g_chain * un * UB;
    else if (a.metric == MMF_COSINE) e2 = (g_chain + 4.7683716e-7f) * un * UB * 1.01f;
    else e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
    margin = 2.0f * (e1 + e2) * 1.001f + 1e-30f;
  }

  static_assert(!(SEG && SINK), "overflow ids are local columns: no segmented form");
  WideList<CAP, W_NT, SINK> list;
  list.init(lkeys + tid, lids + tid);
  if (!qvalid) list.thr = __builtin_huge_valf();
  if constexpr (SINK) {
    if (qvalid) {   // (a lane without a query keeps cap == 0: its sink refuses everything, and it never has a hit)
      list.sink.cnt = a.spill_cnt; list.sink.ids = a.spill_ids; list.sink.cap = (uint32_t)a.spill_cap; list.sink.row = lrow;
      if (a.spill_stacks) list.sink.stacks = 1 + half;
    }
  }

  // DMA roles (scan_f32_kernel's): piece p = wave + 4 i covers tile rows [(p % W_HP) * 8, + 8) of the query (i < 4) or
  // candidate tile; lane l lands at row l / 8, unit l % 8 of the piece and fetches the unit the swizzle puts there.  The
  // lane's byte offset inside a tile image is loop invariant; the chunk moves through the scalar offset, the tile through
  // the buffer's base.
  uint32_t voff[W_PPW];
#pragma unroll
  for (int i = 0; i < W_PPW; ++i) {
    const int row = ((wave + 4 * i) % W_HP) * W_RPP + lane / W_UPR;
    const int lu = (lane % W_UPR) ^ ((row >> W_FSH) & (W_UPR - 1));
    voff[i] = (uint32_t)(row * a.dp * 2 + 16 * lu);
  }
  const char* zq0 = reinterpret_cast<const char*>(a.ZQ) + q0 * (int64_t)a.dp * 2;
  const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zq0), 0, -1, 0x00020000);
  float rcb = 0.0f;
  // chunk kc of candidate tile ct -> stage `buf`; the tile's 128 biases ride along with its first chunk
  auto stage = [&](int64_t ct, int kc, int buf) {
    if (kc == 0 && tid < W_CT) rcb = a.cb[ct * W_CT + tid];
    const char* zc = reinterpret_cast<const char*>(a.ZC) + ct * W_CT * (int64_t)a.dp * 2;
    const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zc), 0, -1, 0x00020000);
    const int koff = kc * W_ROWB;
    char* sb = stages + buf * W_STAGEB;
#pragma unroll
    for (int i = 0; i < W_PPW; ++i) {
      const int pr = (wave + 4 * i) % W_HP;
      if (i < W_PPW / 2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(qrsrc, (__attribute__((address_space(3))) void*)(sb + pr * 1024), 16, (int)voff[i], koff, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(crsrc, (__attribute__((address_space(3))) void*)(sb + W_OPB + pr * 1024), 16, (int)voff[i], koff, 0, 0);
    }
  };

  f32x4 acc[8][2];                              // [candidate block][query block]
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) { acc[cb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[cb][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  // thresholds of the two queries this lane holds values for: its own list's and its partner's (lane ^ 16)
  float thr_q0, thr_q1;
  auto refresh_thr = [&]() {
    const float mine = list.thr;
    const float theirs = __shfl_xor(mine, 16);
    thr_q0 = ownb ? theirs : mine;
    thr_q1 = ownb ? mine : theirs;
  };
  refresh_thr();

  // operand reads inside a stage: query row 32 wave + c16 (+ 16 qb), candidate row c16 (+ 16 cb); all of them share
  // the swizzle term of row c16 (the other rows differ by multiples of 16), so one term serves every read of the lane
  const int sw = (c16 >> W_FSH) & (W_UPR - 1);
  const int qoff = (32 * wave + c16) * W_ROWB;
  const int coff = W_OPB + c16 * W_ROWB;

  if (steps > 0) {
    stage(t_begin, 0, 0);
    if (tid < W_CT) cbs[tid] = rcb;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int64_t ct = t_begin;        // tile and chunk being multiplied
  int kc = 0;
  for (int64_t s = 0; s < steps; ++s) {
    const int buf = (int)(s & 1);
    int nkcn = kc + 1;
    int64_t nct = ct;
    if (nkcn == nkc) { nkcn = 0; nct = ct + 1; }
    if (s + 1 < steps) stage(nct, nkcn, buf ^ 1);
    const int tpar = (int)((ct - t_begin) & 1);

    if (kc == 0) {             // a new tile: accumulators start from the candidates' bias
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(cbs + tpar * W_CT + 16 * cb + 4 * g);
        acc[cb][0] = b4; acc[cb][1] = b4;
      }
    }

    const char* sb = stages + buf * W_STAGEB;
#pragma unroll
    for (int ks = 0; ks < W_KC / 32; ++ks) {
      const int uo = ((4 * ks + g) ^ sw) * 16;
      const wu32x4 b0 = *reinterpret_cast<const wu32x4*>(sb + qoff + uo);
      const wu32x4 b1 = *reinterpret_cast<const wu32x4*>(sb + qoff + 16 * W_ROWB + uo);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const wu32x4 av = *reinterpret_cast<const wu32x4*>(sb + coff + cb * 16 * W_ROWB + uo);
        if constexpr (F16) {
          acc[cb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(wf16x8, av), __builtin_bit_cast(wf16x8, b0), acc[cb][0], 0, 0, 0);
          acc[cb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(wf16x8, av), __builtin_bit_cast(wf16x8, b1), acc[cb][1], 0, 0, 0);
        } else {
          acc[cb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wbf16x8, av), __builtin_bit_cast(wbf16x8, b0), acc[cb][0], 0, 0, 0);
          acc[cb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wbf16x8, av), __builtin_bit_cast(wbf16x8, b1), acc[cb][1], 0, 0, 0);
        }
      }
    }

    if (kc == nkc - 1) {       // the whole d is in: one epilogue per macro tile, a 32-candidate sub-tile at a time
      if constexpr (XSEG) {
        // The columns a query may not take.  The window test is wave-uniform and almost always false (a block inside one segment
        // meets its mask on the two tiles that straddle the segment's bounds); the bounds of the lane's two queries — c16 and
        // c16 + 16 of the wave — are loaded inside the branch, so the tile loop carries nothing for them.  acc starts from the bias
        // again at the next tile.
        if (__builtin_expect(xw0 <= ct && ct < xw1, 0)) {
          const uint32_t* bq = a.bounds + 2 * (q0 + 32 * wave + c16);
          const uint32_t lo0 = bq[0], len0 = bq[1], lo1 = bq[32], len1 = bq[33];
          const uint32_t col0 = (uint32_t)(ct * W_CT) + 4 * g;
#pragma unroll
          for (int cb = 0; cb < 8; ++cb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t col = col0 + 16 * cb + j;      // acc[cb][qb][j]: candidate 16 cb + 4 g + j of the tile
              if (col - lo0 < len0) acc[cb][0][j] = kNegInf;
              if (col - lo1 < len1) acc[cb][1][j] = kNegInf;
            }
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4& p0 = acc[2 * t][0]; const f32x4& r0 = acc[2 * t + 1][0];
        const f32x4& p1 = acc[2 * t][1]; const f32x4& r1 = acc[2 * t + 1][1];
        const float m0 = fmaxf(fmaxf(fmaxf(p0[0], p0[1]), fmaxf(p0[2], p0[3])), fmaxf(fmaxf(r0[0], r0[1]), fmaxf(r0[2], r0[3])));
        const float m1 = fmaxf(fmaxf(fmaxf(p1[0], p1[1]), fmaxf(p1[2], p1[3])), fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3])));
        if (__builtin_expect(__any((m0 >= thr_q0) || (m1 >= thr_q1)), 0)) {
          // this lane's query gets its 16 candidates together: its own 8 plus the 8 the partner lane holds
          f32x16 v;
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float mine = ownb ? acc[2 * t + cb][1][j] : acc[2 * t + cb][0][j];
              const float give = ownb ? acc[2 * t + cb][0][j] : acc[2 * t + cb][1][j];
              v[4 * cb + j] = mine;
              v[8 + 4 * cb + j] = __shfl_xor(give, 16);
            }
          }
          if constexpr (CEIL) {   // columns the row has already emitted (and nothing that ranks after its floor: §4.28) lie above its ceiling
            const float ce = a.ceil[qpos];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = (v[r] > ce) ? kNegInf : v[r];
          }
          // v[0..7]: rows of this lane's group g, v[8..15]: rows of the partner's group g ^ 1
          const int g4 = 4 * g;
          auto rowof = [g4](int r) -> uint32_t { return (uint32_t)((g4 ^ ((r & 8) >> 1)) + (r & 3) + 16 * ((r >> 2) & 1)); };
          list.offer_tile(v, (uint32_t)(ct * W_CT + 32 * t) + id_off, rowof, a.kk, margin);
          refresh_thr();
        }
      }
    }

    if (s + 1 < steps && nkcn == 0 && tid < W_CT) cbs[(int)((nct - t_begin) & 1) * W_CT + tid] = rcb;
    ct = nct; kc = nkcn;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next chunk have landed
    __syncthreads();
  }

  // Settle: the pair's proven threshold from what the two lists hold, entries below the threshold dropped before they are
  // written (the re-rank gathers about kk rows per list, not CAP).
  list.compact(a.kk, margin);
  if constexpr (SINK) {
    list.sink.close();                    // reserved overflow slots this lane did not use
    if (a.spill_stacks) {                 // two stacks: both counts in one word; stacks that met cost the row its fast path
      const uint32_t mine = qvalid ? list.sink.cpos : 0u;   // (the compaction above has emptied a stack that no longer matters)
      const uint32_t theirs = (uint32_t)__shfl_xor((int)mine, 32);
      const uint32_t mine_high = mine > list.high ? mine : list.high;
      const uint32_t theirs_high = (uint32_t)__shfl_xor((int)mine_high, 32);
      if (qvalid && mine_high + theirs_high > (uint32_t)a.spill_cap) list.lost = kFltMax;
      if (qvalid && half == 0 && (mine | theirs)) a.spill_cnt[lrow] = mine | (theirs << 16);
    } else if (qvalid && a.sunk && list.sunk > kNegInf) {
      atomicMax(a.sunk + lrow, wide_enc(list.sunk));
    }
  }
  if (qvalid) {
    const int64_t lbase = lrow * a.lists_total + a.list_base + slot + half;
    a.cand_cnt[lbase] = (uint32_t)list.cnt;
    for (int e = 0; e < list.cnt; ++e) {
      a.cand_ids[lbase * CAP + e] = list.ids[e * W_NT];
      if (a.cand_keys) a.cand_keys[lbase * CAP + e] = list.keys[e * W_NT];
    }
    if (a.cand_keys && half == 0) a.margin_out[lrow] = margin;
    if (list.proven > -kFltMax) atomicMax(a.seed + lrow, wide_enc(list.proven));
    if (list.lost > kNegInf) atomicMax(a.lost + lrow, wide_enc(list.lost));
  }
}

// Column splits: every pair of lists proves a threshold from ITS columns only, (kk-th best of the split) - margin, which can
// lie far below the row's.  One wave per row takes the kk-th best key of everything the row's lists hold — a subset of the
// row's columns, so a valid lower bound — and raises the row's threshold to it minus the margin.  With that, "band <= CAP
// columns => never flagged" holds for any number of splits (header).  kk rounds of "best entry ranked after the previous
// pick" under (key desc, position asc), as select's pruning does.
// sunk / spill_cnt (plain launches with overflow lists in the counter form, else nullptr): a row whose best written key lies below
// its settled threshold gets its overflow list emptied (header of this file, "Overflow lists").
__global__ __launch_bounds__(256) void wide_seed_union_kernel(const uint32_t* cand_cnt, const float* cand_keys, const float* margin,
                                                              int lists, int cap, int kk, int32_t* seed, int64_t n_rows,
                                                              const int32_t* sunk, uint32_t* spill_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int slots = lists * cap;
  float pk = 0.0f;
  uint32_t pe = 0;
  bool proved = true;
  for (int t = 0; t < kk; ++t) {
    float bk = kNegInf;
    uint32_t be = kNoIdx;
    for (int e = lane; e < slots; e += 64) {
      const int l = e / cap;
      if ((uint32_t)(e - l * cap) >= cand_cnt[row * lists + l]) continue;
      const float ke = cand_keys[row * slots + e];
      if (t > 0 && !better(pk, pe, ke, (uint32_t)e)) continue;
      if (be == kNoIdx || better(ke, (uint32_t)e, bk, be)) { bk = ke; be = (uint32_t)e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o);
      const uint32_t oe = (uint32_t)__shfl_xor((int)be, o);
      if (oe != kNoIdx && (be == kNoIdx || better(ok, oe, bk, be))) { bk = ok; be = oe; }
    }
    if (be == kNoIdx) { proved = false; break; }   // fewer than kk entries: nothing to prove
    pk = bk; pe = be;
  }
  if (lane != 0) return;
  int32_t settled = seed[row];         // what the scan's lists proved (the scan has finished: same stream)
  if (proved) {
    const int32_t p = wide_enc(pk - margin[row]);
    atomicMax(seed + row, p);
    if (p > settled) settled = p;
  }
  if (sunk && sunk[row] < settled) spill_cnt[row] = 0u;   // (no key written: the count is 0 already)
}

// The ceilings of the CEIL kernels (ceil_kernel of mmf_scan_bf16.hip with THIS scan's margin).  Row i has emitted
// everything down to its floor, the canonical key fk_i; a column that ranks after the floor has a key <= fk_i, so its real-number
// target Q is at most map_i(fk_i) + E2_i and its scanned value at most map_i(fk_i) + E1_i + E2_i.  map_i turns a canonical key into
// Q units (Q = bias_j + u_i . u_j, operands scaled by s):
//   dot, cosine: s^2 key;   -|x - y|^2: s^2 (key + n_i) / 2;   rbf (key = -lambda |x - y|^2): s^2 (key / lambda + n_i) / 2.
// E1 + E2 is half the scan's margin — the margin block at the top of scan_b16w_kernel copied term for term (dp = d rounded up to
// 128, no slot-bit term; the kernel keeps its own text so that its instantiations stay the instruction streams they were), the
// scale the block at the top of prep_half_kernel.  2^-21 of the terms' magnitudes covers the f32 rounding of the map itself and of
// the rbf key's product with lambda; the sum is rounded up by one more ulp.
struct WideCeilArgs {
  const float* floor_key; const float* rx;   // [n] the rows' floors and canonical row scalars
  const float *q_zn, *q_rn, *q_un; const uint32_t* maxima; const uint32_t* max_n;
  int64_t n, n_pad; int metric, d, dp; float lambda;
  float* ceil;                               // [n_pad]
  // GATHER (the segmented passes): i is a position of the segment-padded query image, n the positions in use and
  // gather [n] the row of X at each (-1: padding inside a segment's last block, ceiling +inf); floor_key and rx are read through it,
  // the norms by position
  const int32_t* gather;
};
template <bool GATHER>
__global__ void wide_ceil_kernel(WideCeilArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_pad) return;
  if (i >= a.n) { a.ceil[i] = __builtin_huge_valf(); return; }
  int64_t row = i;
  if constexpr (GATHER) {
    row = a.gather[i];
    if (row < 0) { a.ceil[i] = __builtin_huge_valf(); return; }
  }
  // the operands' common power-of-two scale; max_n: float bits of the largest squared norm (unused for cosine)
  float s;
  {
    float mx = (a.metric == MMF_COSINE) ? 1.0f : __builtin_sqrtf(__uint_as_float(a.max_n[0]));
    int ex = 0;
    if (mx > 0.0f && mx < __builtin_huge_valf()) (void)frexpf(mx, &ex); else ex = 9;
    int e = 9 - ex;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    s = ldexpf(1.0f, e);
  }
  const float s2 = s * s;
  const float fk = a.floor_key[row];
  float q, mag;
  if (a.metric == MMF_DOT || a.metric == MMF_COSINE) { q = s2 * fk; mag = fabsf(q); }
  else {
    const float t = (a.metric == MMF_RBF) ? fk / a.lambda : fk, ni = a.rx[row];
    q = 0.5f * s2 * (t + ni); mag = 0.5f * s2 * (fabsf(t) + ni);
  }
  float margin;
  {
    const float ZB = __uint_as_float(a.maxima[0]), RB = __uint_as_float(a.maxima[1]);
    const float UB = __uint_as_float(a.maxima[2]), CB = __uint_as_float(a.maxima[3]);
    const float zn = a.q_zn[i], rn = a.q_rn[i], un = a.q_un[i];
    const float g_acc = (float)(a.dp + 8) * 5.9604645e-8f;
    const float g_chain = (float)(a.d + 2) * 5.9604645e-8f;
    const float e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB);
    float e2;
    if (a.metric == MMF_DOT) e2 = g_chain * un * UB;
    else if (a.metric == MMF_COSINE) e2 = (g_chain + 4.7683716e-7f) * un * UB * 1.01f;
    else e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
    margin = 2.0f * (e1 + e2) * 1.001f + 1e-30f;
  }
  const float c = q + 0.5f * margin + 4.7683716e-7f * mag;
  a.ceil[i] = (c == c) ? nextafterf(c, __builtin_huge_valf()) : __builtin_huge_valf();
}

template <int CAP, bool SEG = false, bool SINK = false, bool XSEG = false, bool CEIL = false>
int launch_b16w_t(const ScanB16WArgs& a, bool f16, int64_t grid, hipStream_t s) {
  const size_t lds = scan_b16w_lds(CAP);
  auto go = [&](auto kern) -> int {
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(W_NT), lds, s, a);
    MMF_LAUNCH_CHECK();
    return MMF_OK;
  };
  if constexpr (XSEG && CEIL) {   // full-depth lists only: the later passes of the cross-segment any-k call
    static_assert(CAP == W_CAP_BIG && !SINK, "ceilings under the cross-segment mask: every pass is 20 deep");
    if (f16) return go(scan_b16w_kernel<true, CAP, true, false, true, true>);
    return go(scan_b16w_kernel<false, CAP, true, false, true, true>);
  }
  if constexpr (SEG && CEIL) {   // full-depth lists only: the later passes of the segmented any-k call
    static_assert(CAP == W_CAP_BIG && !SINK, "ceilings on the table-driven schedule: every pass is 20 deep");
    if (f16) return go(scan_b16w_kernel<true, CAP, true, false, false, true>);
    return go(scan_b16w_kernel<false, CAP, true, false, false, true>);
  }
  if constexpr (CEIL) {
    if (f16) return go(scan_b16w_kernel<true, CAP, false, SINK, false, true>);
    return go(scan_b16w_kernel<false, CAP, false, SINK, false, true>);
  }
  if constexpr (SINK) {
    if (f16) return go(scan_b16w_kernel<true, CAP, SEG, true>);
    return go(scan_b16w_kernel<false, CAP, SEG, true>);
  }
  if constexpr (XSEG) {
    if (f16) return go(scan_b16w_kernel<true, CAP, true, false, true>);
    return go(scan_b16w_kernel<false, CAP, true, false, true>);
  }
  if (f16) return go(scan_b16w_kernel<true, CAP, SEG>);
  return go(scan_b16w_kernel<false, CAP, SEG>);
}

}  // namespace

int scan_b16w_supported(int64_t d, int kk) { return (d > 1024 && d <= 4096 && kk >= 1 && kk <= 20) ? 1 : 0; }
int scan_b16w_cap(int kk) { return kk <= 11 ? W_CAP_SMALL : W_CAP_BIG; }
int scan_b16w_dp(int64_t d) { return (int)((d + 127) / 128 * 128); }
int scan_b16w_queries_per_block() { return W_QT; }
int scan_b16w_col_tile() { return W_CT; }

// Cross-segment scan (mmf_simtopk_cross_segments_wide): one workgroup per entry of `sched`, a device copy of
// cross_segw_table ([grid][8] int32: WSEG_* words 0 .. 4 and 6, WXSEG_W0 / _W1).  Both images are the plain ones of launch_prep_half
// (p.n_rows rows of X, m_pad rows of Y in whole tiles); `bounds` is [n_pad][2], the excluded column range (first, count) of every
// query row, n_pad covering whole 128-row blocks.  `lists` == L.lists == 2 x the largest entry count of a row block — any even
// number: a run cut by a hole is two entries — and a block with fewer entries leaves the rest of its rows' lists empty (the caller
// zeroes the counts).  With more than one pair the lists carry keys and margins and wide_seed_union_kernel settles every row's
// threshold over all of its entries, as in the other launchers.  No overflow lists: a crowded row is flagged.
static int scan_b16w_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                          const ScanB16Panel& pn, const float* ceil, hipStream_t s);
int launch_scan_b16w_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                          const ScanB16Panel& pn, hipStream_t s) {
  return scan_b16w_xseg(p, sched, grid, bounds, lists, L, pn, nullptr, s);
}
// The same launch with a ceiling per query row (mmf_simtopk_cross_segments_wide_anyk): ceil [n_pad] by row of X, what
// launch_scan_b16w_ceilings leaves — the plain images' positions are rows.  Full-depth lists only (every pass of that call is 20 deep).
int launch_scan_b16w_xseg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                               const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (!ceil) { set_error("scan_b16w_xseg_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  if (L.cap != W_CAP_BIG) { set_error("scan_b16w_xseg_ceil: list capacity %d, the ceilings run at the full depth (%d)", L.cap, W_CAP_BIG); return MMF_E_INTERNAL; }
  return scan_b16w_xseg(p, sched, grid, bounds, lists, L, pn, ceil, s);
}
// The launch itself.  ceil: nullptr, or the rows' ceilings (CEIL kernels).
static int scan_b16w_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, int lists, const CandLists& L,
                          const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16w_supported(p.d, p.kk) || p.dp != scan_b16w_dp(p.d)) {
    set_error("scan_b16w_xseg: d = %lld (padded %d), k = %d outside 1024 < d <= 4096, k <= 20", (long long)p.d, p.dp, p.kk);
    return MMF_E_INTERNAL;
  }
  if (lists < 2 || (lists & 1)) { set_error("scan_b16w_xseg: %d lists per row are no whole number of pairs", lists); return MMF_E_INTERNAL; }
  if (!sched || !bounds) { set_error("scan_b16w_xseg: work table or mask bounds missing"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16w_xseg: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (pn.seed_stride < p.n_rows) { set_error("scan_b16w_xseg: threshold buffers shorter than the rows"); return MMF_E_INTERNAL; }
  if (pn.list_base != 0 || pn.seg_len != 0 || pn.id_off != 0) { set_error("scan_b16w_xseg: no paneled form"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16w_xseg: %d lists per row for a table of %d", L.lists, lists); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16w_cap(p.kk)) { set_error("scan_b16w_xseg: list capacity %d, expected %d", L.cap, scan_b16w_cap(p.kk)); return MMF_E_INTERNAL; }
  if (lists > 2 && (!L.keys || !L.margin)) { set_error("scan_b16w_xseg: several entries per block need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % W_CT != 0) { set_error("scan_b16w_xseg: candidate image of %lld rows is no whole number of tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  if (p.m >= (int64_t(1) << 31)) { set_error("scan_b16w_xseg: column ids need m < 2^31"); return MMF_E_INTERNAL; }
  ScanB16WArgs a{};
  a.ZQ = p.ZQ; a.ZC = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.n_rows = p.n_rows; a.kk = p.kk; a.metric = p.metric; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / W_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists; a.list_base = 0;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  a.sched = sched; a.bounds = bounds; a.ceil = ceil;
  if (ceil) MMF_TRY((launch_b16w_t<W_CAP_BIG, true, false, true, true>(a, p.f16, grid, s)));
  else MMF_TRY(L.cap == W_CAP_SMALL ? (launch_b16w_t<W_CAP_SMALL, true, false, true>(a, p.f16, grid, s))
                                    : (launch_b16w_t<W_CAP_BIG, true, false, true>(a, p.f16, grid, s)));
  if (lists > 2) {
    wide_seed_union_kernel<<<dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s>>>(L.cnt, L.keys, L.margin, L.lists, L.cap, p.kk, pn.seed,
                                                                                     p.n_rows, nullptr, nullptr);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// col_splits must be a power of two.  Lists are indexed by query position; pn: the threshold buffers (no panels, no shared
// thresholds on this path).  With more than one split L.keys / L.margin must be set: wide_seed_union_kernel reads them.
// L.spill_cnt (zeroed by the caller) with L.spill_cap > 0: the rows' overflow lists, written by the SINK instantiations in the
// form L.spill_stacks names (two stacks need the one list pair); without them the kernels that lose what a list cannot hold.
// pn.sunk (optional, counter form): the rows' best written keys, memset like pn.seed; with it a row whose overflow entries all
// lie below its settled threshold gets its overflow list emptied.
static int scan_b16w_plain(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s,
                           int* grid_out);
int launch_scan_b16w(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, hipStream_t s, int* grid_out) {
  return scan_b16w_plain(p, col_splits, L, pn, nullptr, s, grid_out);
}
// The launch itself.  ceil: nullptr, or the rows' ceilings (CEIL kernels).
static int scan_b16w_plain(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s,
                           int* grid_out) {
  if (p.n_rows <= 0 || p.m <= 0) return MMF_OK;
  if (!scan_b16w_supported(p.d, p.kk) || p.dp != scan_b16w_dp(p.d)) {
    set_error("scan_b16w: d = %lld (padded %d), k + self = %d outside 1024 < d <= 4096, k + self <= 20", (long long)p.d, p.dp, p.kk);
    return MMF_E_INTERNAL;
  }
  if (col_splits < 1 || (col_splits & (col_splits - 1)) != 0) { set_error("scan_b16w: col_splits %d is no power of two", col_splits); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16w: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (pn.list_base != 0 || pn.seg_len != 0 || pn.id_off != 0) { set_error("scan_b16w: no paneled form"); return MMF_E_INTERNAL; }
  const bool sink = L.spill_cnt != nullptr && L.spill_cap > 0;
  if (sink && (!L.spill_ids || L.spill_cap > 0xffff || (L.spill_stacks && col_splits != 1))) {
    set_error("scan_b16w: overflow lists of %d slots (two stacks: %d) for %d column splits", L.spill_cap, L.spill_stacks, col_splits);
    return MMF_E_INTERNAL;
  }
  if (2 * col_splits != L.lists) { set_error("scan_b16w: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16w_cap(p.kk)) { set_error("scan_b16w: list capacity %d, expected %d", L.cap, scan_b16w_cap(p.kk)); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16w: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  ScanB16WArgs a{};
  a.ZQ = p.ZQ; a.ZC = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.n_rows = p.n_rows; a.kk = p.kk; a.metric = p.metric; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = (p.m + W_CT - 1) / W_CT;
  if (a.tiles_total * W_CT > p.m_pad) { set_error("scan_b16w: candidate image of %lld rows is shorter than its tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  a.col_splits = col_splits;
  a.tiles_per_split = (a.tiles_total + col_splits - 1) / col_splits;
  a.lists_total = L.lists; a.list_base = 0;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  if (sink) {
    a.spill_cnt = L.spill_cnt; a.spill_ids = L.spill_ids; a.spill_cap = L.spill_cap; a.spill_stacks = L.spill_stacks;
    a.sunk = L.spill_stacks ? nullptr : pn.sunk;
  }
  a.ceil = ceil;
  const int64_t row_blocks = (p.n_rows + W_QT - 1) / W_QT;
  const int64_t grid = row_blocks * col_splits;
  if (grid_out) *grid_out = (int)grid;
  if (ceil && sink) MMF_TRY(L.cap == W_CAP_SMALL ? (launch_b16w_t<W_CAP_SMALL, false, true, false, true>(a, p.f16, grid, s)) : (launch_b16w_t<W_CAP_BIG, false, true, false, true>(a, p.f16, grid, s)));
  else if (ceil) MMF_TRY(L.cap == W_CAP_SMALL ? (launch_b16w_t<W_CAP_SMALL, false, false, false, true>(a, p.f16, grid, s)) : (launch_b16w_t<W_CAP_BIG, false, false, false, true>(a, p.f16, grid, s)));
  else if (sink) MMF_TRY(L.cap == W_CAP_SMALL ? (launch_b16w_t<W_CAP_SMALL, false, true>(a, p.f16, grid, s)) : (launch_b16w_t<W_CAP_BIG, false, true>(a, p.f16, grid, s)));
  else MMF_TRY(L.cap == W_CAP_SMALL ? launch_b16w_t<W_CAP_SMALL>(a, p.f16, grid, s) : launch_b16w_t<W_CAP_BIG>(a, p.f16, grid, s));
  if (col_splits > 1) {
    hipLaunchKernelGGL(wide_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows, a.sunk, a.sunk ? a.spill_cnt : nullptr);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// The same launch with a ceiling per query row (mmf_simtopk_wide_anyk): ceil [n_pad] in the kernel's units, n_pad
// covering whole 128-row blocks.
int launch_scan_b16w_ceil(const ScanB16Problem& p, int col_splits, const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s,
                          int* grid_out) {
  if (!ceil) { set_error("scan_b16w_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  return scan_b16w_plain(p, col_splits, L, pn, ceil, s, grid_out);
}
// The ceilings of that launch from the rows' floors (canonical keys, [p.n_rows]): rx the rows' canonical scalars, max_n the word the
// operand images took their scale from; ceil [n_pad], +inf for the padding rows.
int launch_scan_b16w_ceilings(const ScanB16Problem& p, const float* floor_key, const float* rx, const uint32_t* max_n, float lambda, int64_t n_pad,
                              float* ceil, hipStream_t s) {
  if (n_pad < (p.n_rows + W_QT - 1) / W_QT * W_QT) { set_error("scan_b16w_ceilings: %lld ceilings do not cover the row blocks of %lld rows", (long long)n_pad, (long long)p.n_rows); return MMF_E_INTERNAL; }
  WideCeilArgs a{floor_key, rx, p.q_zn, p.q_rn, p.q_un, p.maxima, max_n, p.n_rows, n_pad, p.metric, (int)p.d, p.dp, lambda, ceil, nullptr};
  wide_ceil_kernel<false><<<dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s>>>(a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
// The same for a segment-padded query image (mmf_simtopk_segmented_wide_anyk): ceil [nq_pad] by operand position,
// gather [n_pos] the row of X at each position (-1: padding); floor_key and rx stay indexed by row of X, the norms by position.  The
// margin's maxima are those of the whole padded candidate image (p.maxima), as in the scan that follows.
int launch_scan_b16w_ceilings_gather(const ScanB16Problem& p, const int32_t* gather, int64_t n_pos, const float* floor_key, const float* rx,
                                     const uint32_t* max_n, float lambda, int64_t nq_pad, float* ceil, hipStream_t s) {
  if (!gather) { set_error("scan_b16w_ceilings_gather: position table missing"); return MMF_E_INTERNAL; }
  if (nq_pad <= 0) return MMF_OK;
  if (n_pos < 0 || n_pos > nq_pad || n_pos % W_QT != 0) {
    set_error("scan_b16w_ceilings_gather: %lld positions in an image of %lld are no whole row blocks", (long long)n_pos, (long long)nq_pad);
    return MMF_E_INTERNAL;
  }
  WideCeilArgs a{floor_key, rx, p.q_zn, p.q_rn, p.q_un, p.maxima, max_n, n_pos, nq_pad, p.metric, (int)p.d, p.dp, lambda, ceil, gather};
  wide_ceil_kernel<true><<<dim3((unsigned)((nq_pad + 255) / 256)), dim3(256), 0, s>>>(a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// Segmented scan (mmf_simtopk_segmented_wide): one workgroup per entry of the work table `sched` ([grid][8] int32,
// device; the WSEG_* fields above).  p.n_rows: rows of X — lists, thresholds and margins are indexed by them, the operand images
// by the table's positions.  `lists` = 2 x the largest split count of a segment; a segment with fewer ranges leaves the rest of its
// rows' lists empty (the caller zeroes the counts).  With more than one range per segment the lists carry keys and margins and
// wide_seed_union_kernel settles every row's threshold, as in launch_scan_b16w.
static int scan_b16w_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                         const float* ceil, hipStream_t s);
int launch_scan_b16w_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                         hipStream_t s) {
  return scan_b16w_seg(p, sched, grid, lists, L, pn, nullptr, s);
}
// The same launch with a ceiling per OPERAND POSITION (mmf_simtopk_segmented_wide_anyk): ceil [nq_pad] by position of
// the segment-padded query image, what launch_scan_b16w_ceilings_gather leaves.  Full-depth lists only (every pass of that call is 20 deep).
int launch_scan_b16w_seg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                              const float* ceil, hipStream_t s) {
  if (!ceil) { set_error("scan_b16w_seg_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  if (L.cap != W_CAP_BIG) { set_error("scan_b16w_seg_ceil: list capacity %d, the ceilings run at the full depth (%d)", L.cap, W_CAP_BIG); return MMF_E_INTERNAL; }
  return scan_b16w_seg(p, sched, grid, lists, L, pn, ceil, s);
}
// The launch itself.  ceil: nullptr, or the positions' ceilings (CEIL kernels).
static int scan_b16w_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, int lists, const CandLists& L, const ScanB16Panel& pn,
                         const float* ceil, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16w_supported(p.d, p.kk) || p.dp != scan_b16w_dp(p.d)) {
    set_error("scan_b16w_seg: d = %lld (padded %d), k + self = %d outside 1024 < d <= 4096, k + self <= 20", (long long)p.d, p.dp, p.kk);
    return MMF_E_INTERNAL;
  }
  const int col_splits = lists / 2;
  if (lists < 2 || lists != 2 * col_splits || (col_splits & (col_splits - 1)) != 0) {
    set_error("scan_b16w_seg: %d lists per row are no power-of-two number of pairs", lists);
    return MMF_E_INTERNAL;
  }
  if (!sched) { set_error("scan_b16w_seg: work table missing"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16w_seg: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (pn.seed_stride < p.n_rows) { set_error("scan_b16w_seg: threshold buffers shorter than the rows"); return MMF_E_INTERNAL; }
  if (pn.list_base != 0 || pn.seg_len != 0 || pn.id_off != 0) { set_error("scan_b16w_seg: no paneled form"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16w_seg: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16w_cap(p.kk)) { set_error("scan_b16w_seg: list capacity %d, expected %d", L.cap, scan_b16w_cap(p.kk)); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16w_seg: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % W_CT != 0) { set_error("scan_b16w_seg: candidate image of %lld rows is no whole number of tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  ScanB16WArgs a{};
  a.ZQ = p.ZQ; a.ZC = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.n_rows = p.n_rows; a.kk = p.kk; a.metric = p.metric; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / W_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists; a.list_base = 0;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  a.sched = sched; a.ceil = ceil;
  if (ceil) MMF_TRY((launch_b16w_t<W_CAP_BIG, true, false, false, true>(a, p.f16, grid, s)));
  else MMF_TRY(L.cap == W_CAP_SMALL ? (launch_b16w_t<W_CAP_SMALL, true>(a, p.f16, grid, s)) : (launch_b16w_t<W_CAP_BIG, true>(a, p.f16, grid, s)));
  if (col_splits > 1) {
    hipLaunchKernelGGL(wide_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows, nullptr, nullptr);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

}  // namespace mmf
