// mmf_scan_b16c.hip — the 16-bit scan of the COMBINED key: f16 / bf16 MFMA candidate generation for the top-k of
// K = K_h * K_g (mmf_simtopk_combined_fast, include/mmf_hg_topk16.h), 1 <= d <= 4096, k + self <= 20.
//
// The structure is scan_b16w_kernel's (mmf_scan_b16w.hip), copied rather than shared: a workgroup = 4 waves owns a macro tile of
// 128 queries x 128 candidates, both operands stream through LDS by buffer-form LDS-DMA in k-chunks of 64 halves (XOR swizzle
// on the source address), double buffered, v_mfma_f32_16x16x32_{f16,bf16}, accumulators initialised with the candidates' bias
// cb_j (-inf: padding), lists of whole keys (16 entries for k + self <= 11, 32 for 12..20), column splits in powers of two, a
// seed-union launch when there is more than one split.  Operands are the MMF_RBF images of launch_prep_half, unchanged, with
// dp = d rounded up to 128 — so this kernel also serves d <= 1024.
//
// The key.  The prep scales the rows by s = 2^e (taken from the largest squared norm), so the scanned value is
//   G_ij = cb_j + z_i.z_j,  cb_j = -n_j s^2 / 2,  z = round_16(s f),
// and with a = 2 lambda_h / s^2 (exact in f32) the feature exponent is eh_ij = a Q_ij - lambda_h n_i, Q the real-number
// target of G.  The epilogue, once per macro tile and one 32-candidate sub-tile at a time:
//   (i)  coarse test on the feature term alone.  eg_ij = -lambda_g sq_from(pn_i, pn_j, chain(p_i, p_j)) is not clamped: it can
//        exceed 0, by at most egb_i = lambda_g (2 dp + 4) 2^-24 (pn_i + max pn) 1.01 (the three chains err by at most dp ulps of
//        (pn_i + pn_j) / 2 each, the two adds by one ulp of their results).  fl(fmaf(a, max G, rc_i) + egb_i), rc_i =
//        fl(-lambda_h n_i), bounds every approximate key of the sub-tile from above (fmaf and the add are monotone), so a
//        sub-tile where it lies below both thresholds the lane serves is skipped: 14 v_max, 2 fma, 2 adds, 2 compares.
//   (ii) a sub-tile that passes forms eg_ij with pos_exponent<T> (mmf_dev.h; T in {2, 4, 8}, wave-uniform) from the chains
//        launch_row_scalars gives the exact path — the canonical bits, no approximation in the position term — and the
//        approximate key  A_ij = fl(fl(fmaf(a, G_ij, rc_i)) + eg_ij)  (-inf for a padding column, selected on G == -inf before
//        any arithmetic: lambda_h = 0 makes a = 0 and 0 * -inf would be NaN).  The threshold test and the list code run on A.
//   A candidate tile's positions ([128][8] floats, zero beyond dp, rows clamped at m - 1) and chains ride into LDS with the
//   tile's first chunk, two parities (9 KiB).  A lane holds values of two queries in the C layout, so it keeps both queries'
//   positions, chains, rc and egb.
//
// Error margin.  E1_i and E2_i are the wide scan's (mmf_scan_b16w.hip; E2 its MMF_RBF form, which includes the rounding of
// sq_from's two ops and of the product with -lambda_h), in units of Q:  |a G_ij - lambda_h n_i - eh_ij| <= a (E1_i + E2_i) +
// u lambda_h n_i (u = 2^-24: the rounding of rc_i).  The fmaf rounds once (u |inner|), each of the two adds — the scan's
// inner + eg and the canonical eh + eg — once (u |A|, u |key|).  With inner <= hb_i = a (E1_i + E2_i) 1.01 and eg <= egb_i,
// |inner| <= |A| + hb_i + egb_i, and |key| <= |A| + |A - key|, so
//   |A_ij - key_ij| <= err_i(A_ij) = a (E1_i + E2_i) + u' (3 |A_ij| + lambda_h n_i + pb_i),  pb_i = hb_i + egb_i, u' = 1.01 u.
// Unlike in the feature-only scans |key| is not bounded by the row norms (lambda_g sq_g reaches thousands for pixel
// coordinates), so the margin is a function of the threshold it is subtracted from.  Let T be the kk-th best A of a set of
// columns, j a column of the canonical top-kk with A_j < T, and c one of the kk columns with A_c >= T and key_c <= key_j
// (there is one).  A_c lies in [T, pb_i], so |A_c| <= |T| + pb_i, and |A_j| <= |T| + (T - A_j).  Then
//   T - A_j <= err_i(A_c) + err_i(A_j) <= 2 a (E1_i + E2_i) + 2 u' (lambda_h n_i + pb_i) + 3 u' (2 |T| + pb_i + (T - A_j)),
// i.e. T - A_j <= margin_i(T) with
//   margin_i(t) = m0_i + m1 |t|,  m0_i = 2.002 (a (E1_i + E2_i) + u' (lambda_h n_i + 2 pb_i)) + 1e-30,  m1 = 6.1 * 2^-24
// (2 * 3 * 1.01 u / (1 - 3 u') < 6.1 u).  t - margin_i(t) increases with t, so a threshold proven from a subset of the columns
// is a lower bound of the final one, as in the wide scan.  margin_i(t) is applied wherever the wide kernel uses `margin`:
// compaction, the final settle and the seed union (comb_seed_union_kernel below: the stored per-row word is m0_i).
//
// What a list guarantees is the wide scan's contract word for word, the band defined through margin_i: a row whose band —
// the columns with A >= T - margin_i(T), T the kk-th best A over ALL columns — holds at most CAP columns is never flagged.
// A flagged row is answered by the exact pass.  A scale outside f32's reach (|e| > 60: a would overflow or vanish) flags
// every row.
//
// Segmented form (mmf_simtopk_combined_fast_segmented, include/ext/mmf_hg_topk16_seg.h): the same kernel with
// SEG = true takes its row block, column range, id offset, list slot and clamp rows from a host-built work table, one entry per
// workgroup, over ONE image in which every segment is padded to whole tiles of 128.  Scale and maxima are the batch's — a superset
// of any one segment's rows, so m0_i is at least a per-segment call's — and a row's band is taken inside its own segment.
//
// Two-set form (mmf_simtopk_combined_xy, include/ext/mmf_hg_topk_xy.h): the SEG = true kernel again, unchanged,
// for queries that are not the candidates (or only rows r0 .. of them).  ONE image: the candidates from position 0, padded to
// whole tiles of 128; queries that are no slice of the candidates appended from the next multiple of 128.  nf / P / pn are in the
// joint numbering candidates-then-queries (for a slice: the candidates' own), so CSEG_ROW0 is a query block's row in it,
// CSEG_QPOS its image position (for a slice r0 + 128 b: any position — the query DMA and zn / rn / un only need 128 mapped rows
// behind it, which one spare block of padding behind the image gives), the tile range covers candidate tiles only, CSEG_IDOFF = 0
// and CSEG_LAST = nc - 1: the lists hold candidate rows and the candidate-side reads stay on the candidates.  Lists, threshold
// buffers and margins exist for the queries alone: the launcher hands the kernel their bases moved back by the first query's
// joint row (launch_scan_b16c_xy).
// Why the margin proof carries over.  The proof above uses, for a pair (i, j): one scale s for z_i and z_j; E1_i / E2_i, which
// bound the rounding of row i against ANY row whose zn / rn / un / |cb| lie below the four maxima; egb_i, which needs max pn over
// every row j that i meets; and nothing else that ties i to the set j comes from.  Scale, maxima and the largest pn are taken
// over the UNION of both sides here (both prep launches and both row-scalar launches write the same words), a superset of the
// candidates — all a query's bound needs — so every inequality holds pair by pair with m0_i at least the value a self call over
// the union would use, and a query's band is taken among the candidate columns only.  For a slice the union is the candidates,
// so m0_i, the approximate keys and therefore the flagged rows are those of the self call on the candidates.
//
// Ceilings (mmf_simtopk_combined_fast_anyk, include/ext/mmf_hg_topk16_anyk.h): a later pass of a call with
// k + self > 20 scans for the columns that rank strictly AFTER the row's floor (fk_i, fid_i) — the last entry the row has
// emitted — in the total order (key descending, id ascending).  Call that set S_i.  The CEIL kernel turns every approximate key
// above a per-row ceiling into -inf; the ceiling must never mask a member of S_i.  From the error margin above, with
//   e0_i = a (E1_i + E2_i) + u' (lambda_h n_i + pb_i)   (so that |A_ij - key_ij| <= e0_i + 3 u' |A_ij|; m0_i >= 2.002 e0_i),
// a column j of S_i has key_ij <= fk_i, hence A_ij <= h + 3 u' |A_ij| with h = fk_i + e0_i:
//   A_ij >= 0:      A_ij (1 - 3 u') <= h, so h >= 0 and A_ij <= h / (1 - 3 u') <= h + 3.1 u' h;
//   h < A_ij < 0:   |A_ij| < |h|, so A_ij < h + 3 u' |h|;     A_ij <= h: nothing to show.
// Either way A_ij <= h + 3.1 u' |h| <= h + 3.2 u |h| in real numbers.  comb_ceil_kernel takes e0 = m0_i / 2 (exact halving of the
// word the scan itself uses; m0_i / 2 >= 1.001 e0_i covers the roundings of forming it, as in the scan), hf = fl(fk_i + e0)
// (h <= hf + u |hf|, |h| <= (1 + u) |hf|, so the bound is at most hf + 4.3 u |hf|) and returns the float above
// fl(hf + fl(6 u |hf|)) >= hf + (6 (1 - u) - 1.01) u |hf|.  fk_i = -inf (the row has no column left) gives -inf: everything is
// masked.  The distance from the floor to the ceiling is e0 + 6 u |h| plus two ulps — about half of margin_i(fk_i).
// What gets through without belonging to S_i — a ghost: a column the row has already emitted, or the row itself — has
// key_ij >= fk_i: in the exact order every ghost stands before every member of S_i, so in a re-ranked row the ghosts are a
// prefix; and key_ij <= A_ij + e0_i + 3 u' |A_ij| <= ceiling + e0_i + 3 u' |ceiling|, within about margin_i(fk_i) of the floor.
// The lists' guarantee (the band through margin_i) is a statement about ANY set of columns, here the unmasked ones, so the
// re-rank certifies the best entries among them exactly as in a first pass.  The coarse test (i) still bounds the unmasked keys
// from above (masking only lowers keys), so it stays sound; it is merely less sharp for a row whose best columns are masked.
#include <math.h>
#include <string.h>

#include <type_traits>

#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

namespace {

constexpr int C_NT = 256;                        // threads per workgroup
constexpr int C_QT = 128;                        // queries per macro tile
constexpr int C_CT = 128;                        // candidates per macro tile
constexpr int C_KC = 64;                         // halves per staged chunk
constexpr int C_ROWB = C_KC * 2;                 // bytes per LDS row (128)
constexpr int C_OPB = C_QT * C_ROWB;             // bytes per operand tile of a stage (16 KiB)
constexpr int C_STAGEB = 2 * C_OPB;              // queries, then candidates
constexpr int C_UPR = C_ROWB / 16;               // 16-byte units per row (8)
constexpr int C_RPP = 64 / C_UPR;                // rows per 1 KiB DMA piece (8)
constexpr int C_HP = C_QT / C_RPP;               // pieces per operand tile (16)
constexpr int C_PPW = 2 * C_HP / 4;              // pieces per wave and chunk (8): the first half query pieces
constexpr int C_FSH = 1;                         // unit u of tile row r sits at unit u ^ ((r >> C_FSH) & (C_UPR - 1))
constexpr int C_CAP_SMALL = 16;                  // list entries per lane, k + self <= 11
constexpr int C_CAP_BIG = 32;                    // ... k + self in 12..20
constexpr float C_U = 5.9604645e-8f;             // 2^-24
constexpr float C_M1 = 6.1f * C_U;               // slope of margin_i(t) (header)

typedef __bf16 cbf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 cf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t cu32x4 __attribute__((ext_vector_type(4)));

// order-preserving float -> int32 map of the threshold buffers (ScanB16Panel::seed; memset 0x80 = none)
__device__ __forceinline__ int32_t comb_enc(float f) {
  const int32_t b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}

struct ScanB16CArgs {
  const void* Z;             // [n_pad][dp] the one operand image (X is Y)
  const float* cb;           // [n_pad]
  const float* q_zn; const float* q_rn; const float* q_un;
  const uint32_t* maxima;
  const float* nf;           // [n] canonical chain(f, f)
  const float* P;            // [n][dpp] positions
  const float* pn;           // [n] canonical chain(p, p)
  const uint32_t* max_nf;    // float bits of the largest nf (the prep's scale comes from it)
  const uint32_t* max_pn;    // float bits of the largest pn
  float lambda_h, lambda_g;
  int dpp;                   // position dims, 1..8
  int64_t n_rows;            // queries = candidates
  int64_t tiles_total;
  int64_t tiles_per_split;
  int col_splits;
  int dp;                    // feature dims of the image, multiple of 128
  int d;
  int kk;
  int lists_total;
  int32_t* seed;             // [>= n_rows] best proven threshold per query (comb_enc; atomicMax)
  int32_t* lost;             // [>= n_rows] best dropped key per query
  uint32_t* cand_cnt; uint32_t* cand_ids;
  float* cand_keys;          // approximate keys of the entries, or nullptr
  float* margin_out;         // [n_rows] m0_i, written with cand_keys
  const int32_t* sched;      // SEG kernels only: [grid][CSEG_ENTRY] work table (launch_scan_b16c_seg)
  const float* ceil;         // CEIL kernels only: [n_rows] per-row ceiling of the approximate key, by row of F (comb_ceil_kernel)
};

// One entry of the segmented work table (the layout of mmf_scan_b16w.hip's, plus the clamp row): a workgroup = one row block of
// one segment against one column range of that segment.  There is ONE operand image (X is Y), padded per segment to whole tiles
// of 128: Z, cb and zn / rn / un are addressed by image position; nf, P, pn, the lists and the threshold buffers by row of F.
enum : int {
  CSEG_QPOS = 0,    // position of the row block's first query in the image (a multiple of 128)
  CSEG_ROW0 = 1,    // row of F of that query
  CSEG_NQ = 2,      // real queries of the block (<= 128)
  CSEG_T0 = 3,      // first and end tile of the column range, in the image (tiles of 128)
  CSEG_T1 = 4,
  CSEG_IDOFF = 5,   // ptr[s] - image position of the segment's first column (mod 2^32): lists hold global rows of F
  CSEG_SLOT = 6,    // first list slot of this range (2 x split)
  CSEG_LAST = 7,    // global row of the segment's last row: the clamp of the candidates' position / chain reads
  CSEG_ENTRY = 8
};

__device__ __forceinline__ float comb_margin(float m0, float t) { return m0 + C_M1 * __builtin_fabsf(t); }

// WideList of mmf_scan_b16w.hip with the margin a function of the threshold: margin_i(t) = m0 + C_M1 |t|.
template <int CAP, int NT>
struct CombList {
  float* keys; uint32_t* ids;
  int cnt;
  float thr;       // max(proven, lost): what a column has to reach
  float proven;    // best (kk-th best key of the pair's lists) - margin seen so far; -FLT_MAX: none
  float lost;      // best dropped key; -inf: none
  bool crowded;    // the last compaction left the list full: hits replace its worst entry, no compaction until a partner asks

  __device__ __forceinline__ void init(float* k, uint32_t* i) {
    keys = k; ids = i; cnt = 0; thr = -kFltMax; proven = -kFltMax; lost = kNegInf; crowded = false;
  }
  __device__ __forceinline__ void push(float key, uint32_t id) {
    keys[cnt * NT] = key; ids[cnt * NT] = id; ++cnt;
  }
  static __device__ __forceinline__ long long order64(float key, uint32_t id) {   // (key desc, id asc) as one signed compare
    const int b = __float_as_int(key + 0.0f);
    const int e = b >= 0 ? b : (b ^ 0x7fffffff);
    return (long long)(((unsigned long long)(uint32_t)e << 32) | (unsigned long long)(~id));
  }

  // Wave-wide (EXEC full): WideList::compact.  The entry of union rank kk - 1 gives the proven threshold t - margin_i(t);
  // what lies below the threshold leaves the list — that is no drop.
  __device__ __forceinline__ void compact(int kk, float m0) {
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
      const float p = t - comb_margin(m0, t);
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
  }

  // A hit on a full list (lane-private): the worst of the CAP + 1 under (key desc, id asc) is dropped and remembered.
  __device__ __forceinline__ void replace_worst(float x, uint32_t id) {
    int wpos = 0;
    float wk = keys[0]; uint32_t wi = ids[0];
#pragma nounroll
    for (int e = 1; e < CAP; ++e) {
      const float ke = keys[e * NT]; const uint32_t ie = ids[e * NT];
      if (better(wk, wi, ke, ie)) { wk = ke; wi = ie; wpos = e; }
    }
    float dropped = x;
    if (better(x, id, wk, wi)) { keys[wpos * NT] = x; ids[wpos * NT] = id; dropped = wk; }
    lost = fmaxf(lost, dropped);
    thr = fmaxf(thr, lost);
  }

  // One 32-candidate sub-tile's 16 values of this lane's query; rowof(r): sub-tile row of element r.  Called by the whole
  // wave when any lane has a hit; only the elements that hold a hit in SOME lane run the push code.
  template <class RowOf>
  __device__ __forceinline__ void offer_tile(const f32x16& v, uint32_t id0, RowOf rowof, int kk, float m0) {
    uint32_t rmask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) rmask |= (__any(v[r] >= thr) ? 1u : 0u) << r;
    while (rmask) {
      const int r = __builtin_ctz(rmask);
      rmask &= rmask - 1;
      const float x = v[r];
      bool hit = x >= thr;
      if (__any(hit && cnt >= CAP && !crowded)) {
        compact(kk, m0);
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

// 64 KiB of stages + 1 KiB of biases + 9 KiB of positions and chains + 32 / 64 KiB of lists: one workgroup per CU
constexpr size_t scan_b16c_lds(int cap) {
  return (size_t)2 * C_STAGEB + (size_t)2 * C_CT * 4 + (size_t)2 * C_CT * 9 * 4 + (size_t)cap * C_NT * 8;
}

// SEG (segmented calls, launch_scan_b16c_seg): the workgroup's row block, column range, id offset, list slot and clamp rows come
// from the work table a.sched instead of blockIdx / col_splits; everything else is shared.
// The kernel's body, inlined into the kernels below.  CEIL (scan_b16c_ceil_kernel: a later pass of mmf_simtopk_combined_fast_anyk,
// launch_scan_b16c_seg_ceil): an approximate key above its row's ceiling a.ceil becomes -inf in stage (ii) of the epilogue, before
// anything but the coarse test (i) has seen it; CEIL = false is the kernel as it was.
template <bool F16, int CAP, bool SEG, bool CEIL>
__device__ __forceinline__ void scan_b16c_body(ScanB16CArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* stages = smem;                                                   // [2][C_STAGEB]
  float* cbs = reinterpret_cast<float*>(smem + 2 * C_STAGEB);            // [2][C_CT] bias of the tile being accumulated / the next
  float* pss = cbs + 2 * C_CT;                                           // [2][C_CT][8] candidate positions (zero beyond dpp)
  float* pns = pss + 2 * C_CT * 8;                                       // [2][C_CT] their chains
  float* lkeys = pns + 2 * C_CT;                                         // [CAP][C_NT]
  uint32_t* lids = reinterpret_cast<uint32_t*>(lkeys + CAP * C_NT);      // [CAP][C_NT]

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
  int64_t m;                                    // candidate rows are clamped at m - 1 (SEG: the segment's last row)
  int64_t row0 = 0;                             // SEG: row of F of the block's first query
  int nq = C_QT;                                // SEG: real queries of the block
  uint32_t id_off = 0;                          // SEG: column of the image -> row of F
  if constexpr (SEG) {
    const int32_t* e = a.sched + (size_t)blockIdx.x * CSEG_ENTRY;
    q0 = e[CSEG_QPOS]; row0 = e[CSEG_ROW0]; nq = e[CSEG_NQ];
    t_begin = e[CSEG_T0]; t_end = e[CSEG_T1]; id_off = (uint32_t)e[CSEG_IDOFF]; slot = e[CSEG_SLOT];
    m = (int64_t)e[CSEG_LAST] + 1;
    if (t_begin > t_end) t_begin = t_end;
  } else {
    const int split = blockIdx.x % a.col_splits;
    const int64_t rb = blockIdx.x / a.col_splits;
    q0 = rb * C_QT;
    t_begin = (int64_t)split * a.tiles_per_split;
    t_end = t_begin + a.tiles_per_split;
    if (t_end > a.tiles_total) t_end = a.tiles_total;
    if (t_begin > t_end) t_begin = t_end;
    slot = 2 * split;
    m = a.n_rows;
  }
  const int nkc = a.dp / C_KC;
  const int64_t steps = (t_end - t_begin) * nkc;

  const int64_t qpos = q0 + 32 * wave + c;      // own query: row of the image; without SEG also of the lists and threshold buffers
  const int64_t lrow = SEG ? row0 + 32 * wave + c : qpos;   // row of F: lists, threshold buffers, margins
  const bool qvalid = SEG ? (32 * wave + c < nq) : (qpos < a.n_rows);

  // a = 2 lambda_h / s^2 from the prep's scale (prep_half_kernel's formula on the same word)
  float av;
  bool bad_scale;
  {
    const float mx = __builtin_sqrtf(__uint_as_float(a.max_nf[0]));
    int ex = 0;
    if (mx > 0.0f && mx < __builtin_huge_valf()) (void)frexpf(mx, &ex); else ex = 9;
    int e = 9 - ex;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    bad_scale = e < -60 || e > 60;
    const float inv_s = ldexpf(1.0f, bad_scale ? 0 : -e);
    av = (2.0f * a.lambda_h * inv_s) * inv_s;
    if (bad_scale) av = 0.0f;
  }
  float nlg = -a.lambda_g;
  // uniform, but kept in vector registers: the list code under the epilogue has no scalar register to spare (scan_f32_kernel's
  // COMB epilogue does the same)
  const float* Ppos = a.P; const float* pnc = a.pn;
  asm volatile("" : "+v"(Ppos), "+v"(pnc), "+v"(nlg), "+v"(av));

  // the two queries this lane holds values for (C layout: query block 0 and 1): positions, chains, rc, egb
  float pq0[8], pq1[8], pnq0, pnq1, rc0, rc1, egb0, egb1;
  {
    const float PNB = __uint_as_float(a.max_pn[0]);
    const float ge = a.lambda_g * (float)(2 * a.dpp + 4) * C_U * 1.01f;
    int64_t qa = (SEG ? row0 : q0) + 32 * wave + c16, qb = qa + 16;
    const int64_t qlast = SEG ? row0 + nq - 1 : m - 1;   // SEG: the block's last real query
    if (qa > qlast) qa = qlast;
    if (qb > qlast) qb = qlast;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pq0[e] = (e < a.dpp) ? a.P[qa * a.dpp + e] : 0.0f;
      pq1[e] = (e < a.dpp) ? a.P[qb * a.dpp + e] : 0.0f;
    }
    pnq0 = a.pn[qa]; pnq1 = a.pn[qb];
    rc0 = -a.lambda_h * a.nf[qa]; rc1 = -a.lambda_h * a.nf[qb];
    egb0 = ge * (pnq0 + PNB); egb1 = ge * (pnq1 + PNB);
  }

  // m0 of this lane's own query (header)
  float m0;
  {
    const float ZB = __uint_as_float(a.maxima[0]), RB = __uint_as_float(a.maxima[1]);
    const float UB = __uint_as_float(a.maxima[2]), CB = __uint_as_float(a.maxima[3]);
    const float zn = a.q_zn[qpos], rn = a.q_rn[qpos], un = a.q_un[qpos];   // arrays are padded to whole row blocks
    const float g_acc = (float)(a.dp + 8) * C_U;
    const float g_chain = (float)(a.d + 2) * C_U;
    const float e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB);
    const float e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
    const float ae = av * (e1 + e2);
    const float rc = ownb ? rc1 : rc0, egb = ownb ? egb1 : egb0;
    const float pb = ae * 1.01f + egb;
    m0 = 2.002f * (ae + 1.01f * C_U * (__builtin_fabsf(rc) + 2.0f * pb)) + 1e-30f;
  }

  CombList<CAP, C_NT> list;
  list.init(lkeys + tid, lids + tid);
  if (!qvalid) list.thr = __builtin_huge_valf();

  // DMA roles (scan_b16w_kernel's): piece p = wave + 4 i covers tile rows [(p % C_HP) * 8, + 8) of the query (i < 4) or
  // candidate tile; lane l lands at row l / 8, unit l % 8 of the piece and fetches the unit the swizzle puts there.
  uint32_t voff[C_PPW];
#pragma unroll
  for (int i = 0; i < C_PPW; ++i) {
    const int row = ((wave + 4 * i) % C_HP) * C_RPP + lane / C_UPR;
    const int lu = (lane % C_UPR) ^ ((row >> C_FSH) & (C_UPR - 1));
    voff[i] = (uint32_t)(row * a.dp * 2 + 16 * lu);
  }
  const char* zq0 = reinterpret_cast<const char*>(a.Z) + q0 * (int64_t)a.dp * 2;
  const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zq0), 0, -1, 0x00020000);
  float rcb = 0.0f;
  f32x4 rpp = {0.0f, 0.0f, 0.0f, 0.0f};   // floats 4 (tid & 1) .. + 3 of candidate tid >> 1's position
  float rpn = 0.0f;                       // chain(p, p) of candidate tid
  // chunk kc of candidate tile ct -> stage `buf`; the tile's biases, positions and chains ride along with its first chunk
  auto stage = [&](int64_t ct, int kc, int buf) {
    if (kc == 0) {
      if (tid < C_CT) {
        rcb = a.cb[ct * C_CT + tid];
        int64_t j = SEG ? (int64_t)((uint32_t)(ct * C_CT + tid) + id_off) : ct * C_CT + tid;
        if (j > m - 1) j = m - 1;
        rpn = pnc[j];
      }
      int64_t j = SEG ? (int64_t)((uint32_t)(ct * C_CT + (tid >> 1)) + id_off) : ct * C_CT + (tid >> 1);
      if (j > m - 1) j = m - 1;
      const int e0 = 4 * (tid & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) rpp[i] = (e0 + i < a.dpp) ? Ppos[j * a.dpp + e0 + i] : 0.0f;
    }
    const char* zc = reinterpret_cast<const char*>(a.Z) + ct * C_CT * (int64_t)a.dp * 2;
    const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zc), 0, -1, 0x00020000);
    const int koff = kc * C_ROWB;
    char* sb = stages + buf * C_STAGEB;
#pragma unroll
    for (int i = 0; i < C_PPW; ++i) {
      const int pr = (wave + 4 * i) % C_HP;
      if (i < C_PPW / 2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(qrsrc, (__attribute__((address_space(3))) void*)(sb + pr * 1024), 16, (int)voff[i], koff, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(crsrc, (__attribute__((address_space(3))) void*)(sb + C_OPB + pr * 1024), 16, (int)voff[i], koff, 0, 0);
    }
  };
  auto file_tile = [&](int par) {   // what stage() fetched for a tile's first chunk, into parity `par`
    if (tid < C_CT) { cbs[par * C_CT + tid] = rcb; pns[par * C_CT + tid] = rpn; }
    *reinterpret_cast<f32x4*>(pss + par * C_CT * 8 + 4 * tid) = rpp;
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

  const int sw = (c16 >> C_FSH) & (C_UPR - 1);
  const int qoff = (32 * wave + c16) * C_ROWB;
  const int coff = C_OPB + c16 * C_ROWB;

  if (steps > 0) {
    stage(t_begin, 0, 0);
    file_tile(0);
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
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(cbs + tpar * C_CT + 16 * cb + 4 * g);
        acc[cb][0] = b4; acc[cb][1] = b4;
      }
    }

    const char* sb = stages + buf * C_STAGEB;
#pragma unroll
    for (int ks = 0; ks < C_KC / 32; ++ks) {
      const int uo = ((4 * ks + g) ^ sw) * 16;
      const cu32x4 b0 = *reinterpret_cast<const cu32x4*>(sb + qoff + uo);
      const cu32x4 b1 = *reinterpret_cast<const cu32x4*>(sb + qoff + 16 * C_ROWB + uo);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const cu32x4 cv = *reinterpret_cast<const cu32x4*>(sb + coff + cb * 16 * C_ROWB + uo);
        if constexpr (F16) {
          acc[cb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cf16x8, cv), __builtin_bit_cast(cf16x8, b0), acc[cb][0], 0, 0, 0);
          acc[cb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cf16x8, cv), __builtin_bit_cast(cf16x8, b1), acc[cb][1], 0, 0, 0);
        } else {
          acc[cb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cbf16x8, cv), __builtin_bit_cast(cbf16x8, b0), acc[cb][0], 0, 0, 0);
          acc[cb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cbf16x8, cv), __builtin_bit_cast(cbf16x8, b1), acc[cb][1], 0, 0, 0);
        }
      }
    }

    if (kc == nkc - 1) {       // the whole d is in: one epilogue per macro tile, a 32-candidate sub-tile at a time
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4& p0 = acc[2 * t][0]; const f32x4& r0 = acc[2 * t + 1][0];
        const f32x4& p1 = acc[2 * t][1]; const f32x4& r1 = acc[2 * t + 1][1];
        // (i) the feature term alone; -FLT_MAX keeps an all-padding sub-tile finite (a = 0 times -inf would be NaN)
        const float g0 = fmaxf(fmaxf(fmaxf(fmaxf(p0[0], p0[1]), fmaxf(p0[2], p0[3])), fmaxf(fmaxf(r0[0], r0[1]), fmaxf(r0[2], r0[3]))), -kFltMax);
        const float g1 = fmaxf(fmaxf(fmaxf(fmaxf(p1[0], p1[1]), fmaxf(p1[2], p1[3])), fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3]))), -kFltMax);
        const float u0 = __builtin_fmaf(av, g0, rc0) + egb0;
        const float u1 = __builtin_fmaf(av, g1, rc1) + egb1;
        if (__builtin_expect(__any((u0 >= thr_q0) || (u1 >= thr_q1)), 0)) {
          // (ii) the approximate keys of the sub-tile: this lane's 8 candidates x 2 queries
          float A0[8], A1[8];
          const float* pst = pss + (tpar * C_CT + 32 * t + 4 * g) * 8;
          const float* pnt = pns + tpar * C_CT + 32 * t + 4 * g;
          auto keys = [&](auto terms) {
            constexpr int T = decltype(terms)::value;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const f32x4 n4 = *reinterpret_cast<const f32x4*>(pnt + 16 * cb);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float pj[T];
                if constexpr (T == 2) {
                  const f32x2 v = *reinterpret_cast<const f32x2*>(pst + (16 * cb + j) * 8);
                  pj[0] = v[0]; pj[1] = v[1];
                } else {
#pragma unroll
                  for (int u = 0; u < T; u += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(pst + (16 * cb + j) * 8 + u);
                    pj[u] = v[0]; pj[u + 1] = v[1]; pj[u + 2] = v[2]; pj[u + 3] = v[3];
                  }
                }
                const float G0 = acc[2 * t + cb][0][j], G1 = acc[2 * t + cb][1][j];
                const bool pad0 = G0 == kNegInf, pad1 = G1 == kNegInf;
                const float x0 = __builtin_fmaf(av, pad0 ? 0.0f : G0, rc0) + pos_exponent<T>(pq0, pj, pnq0, n4[j], nlg);
                const float x1 = __builtin_fmaf(av, pad1 ? 0.0f : G1, rc1) + pos_exponent<T>(pq1, pj, pnq1, n4[j], nlg);
                A0[4 * cb + j] = pad0 ? kNegInf : x0;
                A1[4 * cb + j] = pad1 ? kNegInf : x1;
              }
            }
          };
          if (a.dpp <= 2) keys(std::integral_constant<int, 2>{});
          else if (a.dpp <= 4) keys(std::integral_constant<int, 4>{});
          else keys(std::integral_constant<int, 8>{});
          if constexpr (CEIL) {
            // the two queries' ceilings, fetched here — only a sub-tile that passed (i) pays for them — by the clamped rows of
            // F the positions above came from
            int64_t qa = (SEG ? row0 : q0) + 32 * wave + c16, qb = qa + 16;
            const int64_t qlast = SEG ? row0 + nq - 1 : m - 1;
            if (qa > qlast) qa = qlast;
            if (qb > qlast) qb = qlast;
            const float c0 = a.ceil[qa], c1 = a.ceil[qb];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              A0[e] = A0[e] > c0 ? kNegInf : A0[e];
              A1[e] = A1[e] > c1 ? kNegInf : A1[e];
            }
          }
          const float m0k = fmaxf(fmaxf(fmaxf(A0[0], A0[1]), fmaxf(A0[2], A0[3])), fmaxf(fmaxf(A0[4], A0[5]), fmaxf(A0[6], A0[7])));
          const float m1k = fmaxf(fmaxf(fmaxf(A1[0], A1[1]), fmaxf(A1[2], A1[3])), fmaxf(fmaxf(A1[4], A1[5]), fmaxf(A1[6], A1[7])));
          if (__any((m0k >= thr_q0) || (m1k >= thr_q1))) {
            // this lane's query gets its 16 candidates together: its own 8 plus the 8 the partner lane holds
            f32x16 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float mine = ownb ? A1[e] : A0[e];
              const float give = ownb ? A0[e] : A1[e];
              v[e] = mine;
              v[8 + e] = __shfl_xor(give, 16);
            }
            // v[0..7]: rows of this lane's group g, v[8..15]: rows of the partner's group g ^ 1
            const int g4 = 4 * g;
            auto rowof = [g4](int r) -> uint32_t { return (uint32_t)((g4 ^ ((r & 8) >> 1)) + (r & 3) + 16 * ((r >> 2) & 1)); };
            list.offer_tile(v, (uint32_t)(ct * C_CT + 32 * t) + id_off, rowof, a.kk, m0);
            refresh_thr();
          }
        }
      }
    }

    if (s + 1 < steps && nkcn == 0) file_tile((int)((nct - t_begin) & 1));
    ct = nct; kc = nkcn;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next chunk have landed
    __syncthreads();
  }

  // Settle: the pair's proven threshold from what the two lists hold, entries below the threshold dropped before they are
  // written (the re-rank gathers about kk rows per list, not CAP).
  list.compact(a.kk, m0);
  if (qvalid) {
    const int64_t lbase = lrow * a.lists_total + slot + half;
    a.cand_cnt[lbase] = (uint32_t)list.cnt;
    for (int e = 0; e < list.cnt; ++e) {
      a.cand_ids[lbase * CAP + e] = list.ids[e * C_NT];
      if (a.cand_keys) a.cand_keys[lbase * CAP + e] = list.keys[e * C_NT];
    }
    if (a.cand_keys && half == 0) a.margin_out[lrow] = m0;
    if (list.proven > -kFltMax) atomicMax(a.seed + lrow, comb_enc(list.proven));
    if (list.lost > kNegInf) atomicMax(a.lost + lrow, comb_enc(list.lost));
    if (bad_scale && half == 0) atomicMax(a.lost + lrow, comb_enc(kFltMax));   // no usable key: the exact pass answers the row
  }
}

template <bool F16, int CAP, bool SEG = false>
__global__ __launch_bounds__(C_NT, 1) void scan_b16c_kernel(ScanB16CArgs a) {
  scan_b16c_body<F16, CAP, SEG, false>(a);
}

// the table-driven scan with 32-entry lists under per-row ceilings (the header's "Ceilings")
template <bool F16>
__global__ __launch_bounds__(C_NT, 1) void scan_b16c_ceil_kernel(ScanB16CArgs a) {
  scan_b16c_body<F16, C_CAP_BIG, true, true>(a);
}

// Column splits: wide_seed_union_kernel with margin_i(t).  One wave per row takes the kk-th best key pk of everything the
// row's lists hold — a subset of the row's columns, so a valid lower bound — and raises the row's threshold to
// pk - (m0_i + C_M1 |pk|).
__global__ __launch_bounds__(256) void comb_seed_union_kernel(const uint32_t* cand_cnt, const float* cand_keys, const float* m0, int lists,
                                                              int cap, int kk, int32_t* seed, int64_t n_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int slots = lists * cap;
  float pk = 0.0f;
  uint32_t pe = 0;
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
    if (be == kNoIdx) return;          // fewer than kk entries: nothing to prove
    pk = bk; pe = be;
  }
  if (lane == 0) atomicMax(seed + row, comb_enc(pk - comb_margin(m0[row], pk)));
}

template <int CAP, bool SEG = false>
int launch_b16c_t(const ScanB16CArgs& a, bool f16, int64_t grid, hipStream_t s) {
  const size_t lds = scan_b16c_lds(CAP);
  auto go = [&](auto kern) -> int {
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C_NT), lds, s, a);
    MMF_LAUNCH_CHECK();
    return MMF_OK;
  };
  if constexpr (SEG) {
    if (f16) return go(scan_b16c_kernel<true, CAP, true>);
    return go(scan_b16c_kernel<false, CAP, true>);
  }
  if (f16) return go(scan_b16c_kernel<true, CAP>);
  return go(scan_b16c_kernel<false, CAP>);
}

}  // namespace

int scan_b16c_supported(int64_t d, int kk) { return (d >= 1 && d <= 4096 && kk >= 1 && kk <= 20) ? 1 : 0; }
int scan_b16c_cap(int kk) { return kk <= 11 ? C_CAP_SMALL : C_CAP_BIG; }
int scan_b16c_dp(int64_t d) { return (int)((d + 127) / 128 * 128); }

// One operand image scanned against itself (p.ZQ == p.ZC, p.n_rows == p.m, MMF_RBF).  col_splits must be a power of two,
// L.lists == 2 * col_splits; with more than one split L.keys / L.margin must be set: comb_seed_union_kernel reads them.
int launch_scan_b16c(const ScanB16Problem& p, const ScanB16Comb& c, int col_splits, const CandLists& L, const ScanB16Panel& pn, hipStream_t s,
                     int* grid_out) {
  if (p.n_rows <= 0) return MMF_OK;
  if (!scan_b16c_supported(p.d, p.kk) || p.dp != scan_b16c_dp(p.d) || p.metric != MMF_RBF) {
    set_error("scan_b16c: d = %lld (padded %d), k + self = %d, metric %d outside 1 <= d <= 4096, k + self <= 20, MMF_RBF", (long long)p.d, p.dp,
              p.kk, p.metric);
    return MMF_E_INTERNAL;
  }
  if (p.ZQ != p.ZC || p.n_rows != p.m) { set_error("scan_b16c: one image against itself only"); return MMF_E_INTERNAL; }
  if (!c.P || !c.pn || !c.nf || !c.max_nf || !c.max_pn || c.dp < 1 || c.dp > 8) { set_error("scan_b16c: positions, chains and maxima (1 <= dp <= 8) missing"); return MMF_E_INTERNAL; }
  if (col_splits < 1 || (col_splits & (col_splits - 1)) != 0) { set_error("scan_b16c: col_splits %d is no power of two", col_splits); return MMF_E_INTERNAL; }
  if (!pn.seed || pn.seed_stride < p.n_rows) { set_error("scan_b16c: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (2 * col_splits != L.lists) { set_error("scan_b16c: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16c_cap(p.kk)) { set_error("scan_b16c: list capacity %d, expected %d", L.cap, scan_b16c_cap(p.kk)); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16c: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  ScanB16CArgs a{};
  a.Z = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.nf = c.nf; a.P = c.P; a.pn = c.pn; a.max_nf = c.max_nf; a.max_pn = c.max_pn; a.lambda_h = c.lambda_h; a.lambda_g = c.lambda_g; a.dpp = c.dp;
  a.n_rows = p.n_rows; a.kk = p.kk; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = (p.m + C_CT - 1) / C_CT;
  if (a.tiles_total * C_CT > p.m_pad) { set_error("scan_b16c: candidate image of %lld rows is shorter than its tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  const int64_t row_blocks = (p.n_rows + C_QT - 1) / C_QT;
  if (row_blocks * C_QT > p.m_pad) { set_error("scan_b16c: query image of %lld rows is shorter than its row blocks", (long long)p.m_pad); return MMF_E_INTERNAL; }
  // the tile DMA addresses a column range with 32-bit offsets inside a tile image: 128 rows of dp halves, far below 4 GiB
  a.col_splits = col_splits;
  a.tiles_per_split = (a.tiles_total + col_splits - 1) / col_splits;
  a.lists_total = L.lists;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  const int64_t grid = row_blocks * col_splits;
  if (grid_out) *grid_out = (int)grid;
  MMF_TRY(L.cap == C_CAP_SMALL ? launch_b16c_t<C_CAP_SMALL>(a, p.f16, grid, s) : launch_b16c_t<C_CAP_BIG>(a, p.f16, grid, s));
  if (col_splits > 1) {
    hipLaunchKernelGGL(comb_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// Segmented scan (mmf_simtopk_combined_fast_segmented): one workgroup per entry of the work table `sched`
// ([grid][8] int32, device; the CSEG_* fields above).  p.n_rows = p.m: rows of F — lists, thresholds and margins are indexed by
// them; p.m_pad: positions of the one operand image, every segment padded to whole tiles of 128.  `lists` = 2 x the largest range
// count of a segment; a segment with fewer ranges leaves the rest of its rows' lists empty (the caller zeroes the counts).  With
// more than one range per segment the lists carry keys and margins and comb_seed_union_kernel settles every row's threshold.
int launch_scan_b16c_seg(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, const CandLists& L,
                         const ScanB16Panel& pn, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16c_supported(p.d, p.kk) || p.dp != scan_b16c_dp(p.d) || p.metric != MMF_RBF) {
    set_error("scan_b16c_seg: d = %lld (padded %d), k + self = %d, metric %d outside 1 <= d <= 4096, k + self <= 20, MMF_RBF", (long long)p.d,
              p.dp, p.kk, p.metric);
    return MMF_E_INTERNAL;
  }
  if (p.ZQ != p.ZC || p.n_rows != p.m) { set_error("scan_b16c_seg: one image against itself only"); return MMF_E_INTERNAL; }
  if (!c.P || !c.pn || !c.nf || !c.max_nf || !c.max_pn || c.dp < 1 || c.dp > 8) { set_error("scan_b16c_seg: positions, chains and maxima (1 <= dp <= 8) missing"); return MMF_E_INTERNAL; }
  const int col_splits = lists / 2;
  if (lists < 2 || lists != 2 * col_splits || (col_splits & (col_splits - 1)) != 0) {
    set_error("scan_b16c_seg: %d lists per row are no power-of-two number of pairs", lists);
    return MMF_E_INTERNAL;
  }
  if (!sched) { set_error("scan_b16c_seg: work table missing"); return MMF_E_INTERNAL; }
  if (!pn.seed || pn.seed_stride < p.n_rows) { set_error("scan_b16c_seg: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16c_seg: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16c_cap(p.kk)) { set_error("scan_b16c_seg: list capacity %d, expected %d", L.cap, scan_b16c_cap(p.kk)); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16c_seg: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % C_CT != 0) { set_error("scan_b16c_seg: image of %lld positions is no whole number of tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  ScanB16CArgs a{};
  a.Z = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.nf = c.nf; a.P = c.P; a.pn = c.pn; a.max_nf = c.max_nf; a.max_pn = c.max_pn; a.lambda_h = c.lambda_h; a.lambda_g = c.lambda_g; a.dpp = c.dp;
  a.n_rows = p.n_rows; a.kk = p.kk; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / C_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  a.sched = sched;
  MMF_TRY(L.cap == C_CAP_SMALL ? (launch_b16c_t<C_CAP_SMALL, true>(a, p.f16, grid, s)) : (launch_b16c_t<C_CAP_BIG, true>(a, p.f16, grid, s)));
  if (col_splits > 1) {
    hipLaunchKernelGGL(comb_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// The same launch under per-row ceilings (a later pass of mmf_simtopk_combined_fast_anyk; the header's
// "Ceilings"): launch_scan_b16c_seg's checks and arguments, 32-entry lists only, ceil [p.n_rows] by row of F (from
// launch_scan_b16c_ceilings).  The seed union sees masked lists only.
int launch_scan_b16c_seg_ceil(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, const CandLists& L,
                              const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16c_supported(p.d, p.kk) || p.dp != scan_b16c_dp(p.d) || p.metric != MMF_RBF) {
    set_error("scan_b16c_seg_ceil: d = %lld (padded %d), k + self = %d, metric %d outside 1 <= d <= 4096, k + self <= 20, MMF_RBF", (long long)p.d,
              p.dp, p.kk, p.metric);
    return MMF_E_INTERNAL;
  }
  if (p.ZQ != p.ZC || p.n_rows != p.m) { set_error("scan_b16c_seg_ceil: one image against itself only"); return MMF_E_INTERNAL; }
  if (!c.P || !c.pn || !c.nf || !c.max_nf || !c.max_pn || c.dp < 1 || c.dp > 8) { set_error("scan_b16c_seg_ceil: positions, chains and maxima (1 <= dp <= 8) missing"); return MMF_E_INTERNAL; }
  const int col_splits = lists / 2;
  if (lists < 2 || lists != 2 * col_splits || (col_splits & (col_splits - 1)) != 0) {
    set_error("scan_b16c_seg_ceil: %d lists per row are no power-of-two number of pairs", lists);
    return MMF_E_INTERNAL;
  }
  if (!sched || !ceil) { set_error("scan_b16c_seg_ceil: work table or ceilings missing"); return MMF_E_INTERNAL; }
  if (!pn.seed || pn.seed_stride < p.n_rows) { set_error("scan_b16c_seg_ceil: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16c_seg_ceil: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != C_CAP_BIG) { set_error("scan_b16c_seg_ceil: list capacity %d, expected %d", L.cap, C_CAP_BIG); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16c_seg_ceil: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % C_CT != 0) { set_error("scan_b16c_seg_ceil: image of %lld positions is no whole number of tiles", (long long)p.m_pad); return MMF_E_INTERNAL; }
  ScanB16CArgs a{};
  a.Z = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.nf = c.nf; a.P = c.P; a.pn = c.pn; a.max_nf = c.max_nf; a.max_pn = c.max_pn; a.lambda_h = c.lambda_h; a.lambda_g = c.lambda_g; a.dpp = c.dp;
  a.n_rows = p.n_rows; a.kk = p.kk; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / C_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.cand_keys = L.keys; a.margin_out = L.margin;
  a.sched = sched; a.ceil = ceil;
  const size_t lds = scan_b16c_lds(C_CAP_BIG);
  const auto kern = p.f16 ? scan_b16c_ceil_kernel<true> : scan_b16c_ceil_kernel<false>;
  MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C_NT), lds, s, a);
  MMF_LAUNCH_CHECK();
  if (col_splits > 1) {
    hipLaunchKernelGGL(comb_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

namespace {

// One thread per image position (the header's "Ceilings"): position q holds row gather[q] of F (-1: padding).  m0 is the scan's
// own word — the formula of scan_b16c_kernel on the same operands, restated here so that the scan's instantiations stay as they are.
__global__ __launch_bounds__(256) void comb_ceil_kernel(const float* q_zn, const float* q_rn, const float* q_un, const uint32_t* maxima,
                                                        const float* nf, const float* pn, const uint32_t* max_nf, const uint32_t* max_pn,
                                                        float lambda_h, float lambda_g, int dpp, int dp, int d, const int32_t* gather,
                                                        int64_t n_pos, const float* floor_key, float* ceil) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pos) return;
  const int64_t row = gather[q];
  if (row < 0) return;
  float av;
  {
    const float mx = __builtin_sqrtf(__uint_as_float(max_nf[0]));
    int ex = 0;
    if (mx > 0.0f && mx < __builtin_huge_valf()) (void)frexpf(mx, &ex); else ex = 9;
    int e = 9 - ex;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    const bool bad_scale = e < -60 || e > 60;   // such a call's rows are all flagged by the scan: any finite ceiling will do
    const float inv_s = ldexpf(1.0f, bad_scale ? 0 : -e);
    av = (2.0f * lambda_h * inv_s) * inv_s;
    if (bad_scale) av = 0.0f;
  }
  const float ZB = __uint_as_float(maxima[0]), RB = __uint_as_float(maxima[1]);
  const float UB = __uint_as_float(maxima[2]), CB = __uint_as_float(maxima[3]);
  const float zn = q_zn[q], rn = q_rn[q], un = q_un[q];
  const float g_acc = (float)(dp + 8) * C_U;
  const float g_chain = (float)(d + 2) * C_U;
  const float e1 = rn * ZB + un * RB + g_acc * (zn * ZB + CB);
  const float e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
  const float ae = av * (e1 + e2);
  const float rc = -lambda_h * nf[row];
  const float egb = lambda_g * (float)(2 * dpp + 4) * C_U * 1.01f * (pn[row] + __uint_as_float(max_pn[0]));
  const float pb = ae * 1.01f + egb;
  const float m0 = 2.002f * (ae + 1.01f * C_U * (__builtin_fabsf(rc) + 2.0f * pb)) + 1e-30f;
  const float fk = floor_key[row];
  float cl = kNegInf;
  if (fk > kNegInf) {
    const float hf = fk + 0.5f * m0;
    cl = nextafterf(hf + 6.0f * C_U * __builtin_fabsf(hf), __builtin_huge_valf());
  }
  ceil[row] = cl;
}

}  // namespace

// ceil[row] for every row of F an image position holds (gather [n_pos]: position -> row, -1 padding; the others keep what they
// have — the scan never reads them), from the row's floor key; p / c: what launch_scan_b16c_seg_ceil will be given.
int launch_scan_b16c_ceilings(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* gather, int64_t n_pos, const float* floor_key,
                              float* ceil, hipStream_t s) {
  if (n_pos <= 0) return MMF_OK;
  if (!gather || !floor_key || !ceil || n_pos > p.m_pad) { set_error("scan_b16c_ceilings: gather table, floors and ceilings for at most %lld positions", (long long)p.m_pad); return MMF_E_INTERNAL; }
  hipLaunchKernelGGL(comb_ceil_kernel, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, p.q_zn, p.q_rn, p.q_un, p.maxima, c.nf, c.pn,
                     c.max_nf, c.max_pn, c.lambda_h, c.lambda_g, c.dp, p.dp, (int)p.d, gather, n_pos, floor_key, ceil);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// Two-set scan (mmf_simtopk_combined_xy; the header's "Two-set form"): launch_scan_b16c_seg's launch with the
// queries' buffers apart.  The kernel indexes lists, threshold buffers and margins by a query's row in the table's joint
// numbering, CSEG_ROW0 + its place in the block; the p.n_rows queries are rows list_row0 .. of that numbering, so the kernel gets
// the bases moved back by list_row0 rows and only ever forms addresses inside the buffers (it writes for real queries only).  The
// seed union and the caller's audit and re-rank see the buffers as they are: row 0 = the first query.
int launch_scan_b16c_xy(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, int64_t list_row0,
                        const CandLists& L, const ScanB16Panel& pn, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16c_supported(p.d, p.kk) || p.dp != scan_b16c_dp(p.d) || p.metric != MMF_RBF) {
    set_error("scan_b16c_xy: d = %lld (padded %d), k + self = %d, metric %d outside 1 <= d <= 4096, k + self <= 20, MMF_RBF", (long long)p.d,
              p.dp, p.kk, p.metric);
    return MMF_E_INTERNAL;
  }
  if (p.ZQ != p.ZC || p.m < 1 || list_row0 < 0) { set_error("scan_b16c_xy: one image holding both sides, candidates first"); return MMF_E_INTERNAL; }
  if (!c.P || !c.pn || !c.nf || !c.max_nf || !c.max_pn || c.dp < 1 || c.dp > 8) { set_error("scan_b16c_xy: positions, chains and maxima (1 <= dp <= 8) missing"); return MMF_E_INTERNAL; }
  const int col_splits = lists / 2;
  if (lists < 2 || lists != 2 * col_splits || (col_splits & (col_splits - 1)) != 0) {
    set_error("scan_b16c_xy: %d lists per row are no power-of-two number of pairs", lists);
    return MMF_E_INTERNAL;
  }
  if (!sched) { set_error("scan_b16c_xy: work table missing"); return MMF_E_INTERNAL; }
  if (!pn.seed || pn.seed_stride < p.n_rows) { set_error("scan_b16c_xy: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16c_xy: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != scan_b16c_cap(p.kk)) { set_error("scan_b16c_xy: list capacity %d, expected %d", L.cap, scan_b16c_cap(p.kk)); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16c_xy: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % C_CT != 0 || (p.m + C_CT - 1) / C_CT * C_CT > p.m_pad) {
    set_error("scan_b16c_xy: image of %lld positions for %lld candidates", (long long)p.m_pad, (long long)p.m);
    return MMF_E_INTERNAL;
  }
  ScanB16CArgs a{};
  a.Z = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.nf = c.nf; a.P = c.P; a.pn = c.pn; a.max_nf = c.max_nf; a.max_pn = c.max_pn; a.lambda_h = c.lambda_h; a.lambda_g = c.lambda_g; a.dpp = c.dp;
  a.n_rows = p.n_rows; a.kk = p.kk; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / C_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists;
  const int64_t lw = list_row0 * L.lists;   // list words ahead of the first query's
  a.seed = pn.seed - list_row0; a.lost = pn.seed + pn.seed_stride - list_row0;
  a.cand_cnt = L.cnt - lw; a.cand_ids = L.ids - lw * L.cap;
  a.cand_keys = L.keys ? L.keys - lw * L.cap : nullptr; a.margin_out = L.margin ? L.margin - list_row0 : nullptr;
  a.sched = sched;
  MMF_TRY(L.cap == C_CAP_SMALL ? (launch_b16c_t<C_CAP_SMALL, true>(a, p.f16, grid, s)) : (launch_b16c_t<C_CAP_BIG, true>(a, p.f16, grid, s)));
  if (col_splits > 1) {
    hipLaunchKernelGGL(comb_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// The two-set scan under per-query ceilings (a later pass of mmf_simtopk_combined_xy_fast_anyk): launch_scan_b16c_xy's
// checks, arguments and moved-back bases on scan_b16c_ceil_kernel, 32-entry lists only.  ceil [p.n_rows] is indexed by query, like
// the lists: the kernel reads it by the joint row of a (clamped) real query of the block, so its base moves back with theirs.
int launch_scan_b16c_xy_ceil(const ScanB16Problem& p, const ScanB16Comb& c, const int32_t* sched, int64_t grid, int lists, int64_t list_row0,
                             const CandLists& L, const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (grid <= 0 || p.n_rows <= 0) return MMF_OK;
  if (!scan_b16c_supported(p.d, p.kk) || p.dp != scan_b16c_dp(p.d) || p.metric != MMF_RBF) {
    set_error("scan_b16c_xy_ceil: d = %lld (padded %d), k + self = %d, metric %d outside 1 <= d <= 4096, k + self <= 20, MMF_RBF", (long long)p.d,
              p.dp, p.kk, p.metric);
    return MMF_E_INTERNAL;
  }
  if (p.ZQ != p.ZC || p.m < 1 || list_row0 < 0) { set_error("scan_b16c_xy_ceil: one image holding both sides, candidates first"); return MMF_E_INTERNAL; }
  if (!c.P || !c.pn || !c.nf || !c.max_nf || !c.max_pn || c.dp < 1 || c.dp > 8) { set_error("scan_b16c_xy_ceil: positions, chains and maxima (1 <= dp <= 8) missing"); return MMF_E_INTERNAL; }
  const int col_splits = lists / 2;
  if (lists < 2 || lists != 2 * col_splits || (col_splits & (col_splits - 1)) != 0) {
    set_error("scan_b16c_xy_ceil: %d lists per row are no power-of-two number of pairs", lists);
    return MMF_E_INTERNAL;
  }
  if (!sched || !ceil) { set_error("scan_b16c_xy_ceil: work table or ceilings missing"); return MMF_E_INTERNAL; }
  if (!pn.seed || pn.seed_stride < p.n_rows) { set_error("scan_b16c_xy_ceil: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (lists != L.lists) { set_error("scan_b16c_xy_ceil: %d lists per row for %d column splits", L.lists, col_splits); return MMF_E_INTERNAL; }
  if (L.cap != C_CAP_BIG) { set_error("scan_b16c_xy_ceil: list capacity %d, expected %d", L.cap, C_CAP_BIG); return MMF_E_INTERNAL; }
  if (col_splits > 1 && (!L.keys || !L.margin)) { set_error("scan_b16c_xy_ceil: column splits need the lists' keys and margins"); return MMF_E_INTERNAL; }
  if (p.m_pad % C_CT != 0 || (p.m + C_CT - 1) / C_CT * C_CT > p.m_pad) {
    set_error("scan_b16c_xy_ceil: image of %lld positions for %lld candidates", (long long)p.m_pad, (long long)p.m);
    return MMF_E_INTERNAL;
  }
  ScanB16CArgs a{};
  a.Z = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.nf = c.nf; a.P = c.P; a.pn = c.pn; a.max_nf = c.max_nf; a.max_pn = c.max_pn; a.lambda_h = c.lambda_h; a.lambda_g = c.lambda_g; a.dpp = c.dp;
  a.n_rows = p.n_rows; a.kk = p.kk; a.d = (int)p.d; a.dp = p.dp;
  a.tiles_total = p.m_pad / C_CT; a.tiles_per_split = a.tiles_total; a.col_splits = 1;   // unused: the table carries the ranges
  a.lists_total = L.lists;
  const int64_t lw = list_row0 * L.lists;   // list words ahead of the first query's
  a.seed = pn.seed - list_row0; a.lost = pn.seed + pn.seed_stride - list_row0;
  a.cand_cnt = L.cnt - lw; a.cand_ids = L.ids - lw * L.cap;
  a.cand_keys = L.keys ? L.keys - lw * L.cap : nullptr; a.margin_out = L.margin ? L.margin - list_row0 : nullptr;
  a.sched = sched; a.ceil = ceil - list_row0;
  const size_t lds = scan_b16c_lds(C_CAP_BIG);
  const auto kern = p.f16 ? scan_b16c_ceil_kernel<true> : scan_b16c_ceil_kernel<false>;
  MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C_NT), lds, s, a);
  MMF_LAUNCH_CHECK();
  if (col_splits > 1) {
    hipLaunchKernelGGL(comb_seed_union_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, s, L.cnt, L.keys, L.margin, L.lists, L.cap,
                       p.kk, pn.seed, p.n_rows);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

// The ceilings of the p.n_rows queries of a two-sided image: query i sits at image position q_pos0 + i and is row q_row0 + i of the
// joint numbering (c.nf / c.pn), its floor and its ceiling are entry i.  comb_ceil_kernel as it is: `iota` [p.n_rows] holds
// 0, 1, ... (launch_anyk_iota) and stands in for the gather table, over the norms, chains and scalars from the first query on;
// the maxima stay the image's — those of both sides.
int launch_scan_b16c_xy_ceilings(const ScanB16Problem& p, const ScanB16Comb& c, int64_t q_pos0, int64_t q_row0, const int32_t* iota,
                                 const float* floor_key, float* ceil, hipStream_t s) {
  if (p.n_rows <= 0) return MMF_OK;
  if (!iota || !floor_key || !ceil || q_pos0 < 0 || q_row0 < 0 || q_pos0 + p.n_rows > p.m_pad) {
    set_error("scan_b16c_xy_ceilings: identity table, floors and ceilings for %lld queries inside the %lld positions", (long long)p.n_rows, (long long)p.m_pad);
    return MMF_E_INTERNAL;
  }
  hipLaunchKernelGGL(comb_ceil_kernel, dim3((unsigned)((p.n_rows + 255) / 256)), dim3(256), 0, s, p.q_zn + q_pos0, p.q_rn + q_pos0, p.q_un + q_pos0,
                     p.maxima, c.nf + q_row0, c.pn + q_row0, c.max_nf, c.max_pn, c.lambda_h, c.lambda_g, c.dp, p.dp, (int)p.d, iota, p.n_rows,
                     floor_key, ceil);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_simtopk_combined_fast(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g, int k,
                              int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx, float* out_val,
                              const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id, void* hip_stream) {
  const char* who = "simtopk_combined_fast";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  if (ptr_host != nullptr || n_segments != 0) {
    set_error("%s: ptr_host / n_segments: a ragged batch stays on mmf_simtopk_combined (one graph here: NULL and 0)", who);
    return MMF_E_UNSUPPORTED;
  }
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int kk = k + (exclude_self ? 1 : 0);
  if (kk > 20) { set_error("%s: k + self = %d > 20 is not supported (mmf_simtopk_combined takes up to 44)", who, kk); return MMF_E_UNSUPPORTED; }
  if (d > 4096) { set_error("%s: d = %lld > 4096 is not supported (mmf_simtopk_combined takes any d)", who, (long long)d); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16", who, prec);
    return MMF_E_INVALID;
  }
  if (opts && opts->col_splits < 0) { set_error("%s: col_splits must be >= 0 (got %d)", who, opts->col_splits); return MMF_E_INVALID; }
  if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  return run_simtopk_combined_fast(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, out_idx, out_val, opts, stats, device_id,
                                   hip_stream);
}

// include/ext/mmf_hg_topk16_seg.h, DESIGN.md §4.18: a ragged batch in one launch of the combined-key 16-bit scan.  The checks are
// mmf_simtopk_combined_fast's, in its order and wording; the offsets are required and checked as mmf_simtopk_combined checks them.
int mmf_simtopk_combined_fast_segmented(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g,
                                        int k, int exclude_self, const int64_t* ptr_host, int64_t n_segments, int64_t* out_idx,
                                        float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id,
                                        void* hip_stream) {
  const char* who = "simtopk_combined_fast_segmented";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (n < 0) { set_error("%s: n must be >= 0 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (n > 0 && !F) { set_error("%s: F is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !P) { set_error("%s: P is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (n > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  MMF_TRY(check_offsets(who, "ptr_host", ptr_host, n_segments, 0, 0, n));
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int kk = k + (exclude_self ? 1 : 0);
  if (kk > 20) { set_error("%s: k + self = %d > 20 is not supported (mmf_simtopk_combined takes up to 44)", who, kk); return MMF_E_UNSUPPORTED; }
  if (d > 4096) { set_error("%s: d = %lld > 4096 is not supported (mmf_simtopk_combined takes any d)", who, (long long)d); return MMF_E_UNSUPPORTED; }
  if (n >= (int64_t)1 << 31) { set_error("%s: n must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16", who, prec);
    return MMF_E_INVALID;
  }
  const int cs = opts ? opts->col_splits : 0;
  if (cs < 0 || (cs & (cs - 1)) != 0) { set_error("%s: col_splits must be 0 or a power of two (got %d)", who, cs); return MMF_E_INVALID; }
  if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  return run_simtopk_combined_fast_segmented(who, F, P, n, d, dp, lambda_h, lambda_g, k, exclude_self, ptr_host, n_segments, out_idx, out_val,
                                             opts, stats, device_id, hip_stream);
}

// include/ext/mmf_hg_topk_xy.h, DESIGN.md §4.19: queries against candidates.  The checks are the siblings', in their order and
// wording, with two sides and the id offsets of mmf_simtopk.
int mmf_simtopk_combined_xy(const float* Fq, const float* Pq, int64_t nq, const float* Fc, const float* Pc, int64_t nc, int64_t d, int64_t dp,
                            float lambda_h, float lambda_g, int k, int exclude_self, int64_t row_offset, int64_t col_offset,
                            int64_t* out_idx, float* out_val, const mmf_simtopk_opts* opts, mmf_simtopk_stats* stats, int device_id,
                            void* hip_stream) {
  const char* who = "simtopk_combined_xy";
  MMF_TRY(Call(who, device_id, hip_stream).on_device());
  if (nq < 0) { set_error("%s: nq must be >= 0 (got %lld)", who, (long long)nq); return MMF_E_INVALID; }
  if (nc < 0) { set_error("%s: nc must be >= 0 (got %lld)", who, (long long)nc); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (k < 1) { set_error("%s: k must be at least 1 (got %d)", who, k); return MMF_E_INVALID; }
  if (row_offset < 0) { set_error("%s: row_offset must be >= 0 (got %lld)", who, (long long)row_offset); return MMF_E_INVALID; }
  if (col_offset < 0) { set_error("%s: col_offset must be >= 0 (got %lld)", who, (long long)col_offset); return MMF_E_INVALID; }
  if (!(lambda_h >= 0.0f) || !isfinite(lambda_h)) { set_error("%s: lambda_h must be finite and >= 0 (got %g)", who, lambda_h); return MMF_E_INVALID; }
  if (!(lambda_g >= 0.0f) || !isfinite(lambda_g)) { set_error("%s: lambda_g must be finite and >= 0 (got %g)", who, lambda_g); return MMF_E_INVALID; }
  if (nq > 0 && !Fq) { set_error("%s: Fq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !Pq) { set_error("%s: Pq is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Fc) { set_error("%s: Fc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && nc > 0 && !Pc) { set_error("%s: Pc is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_idx) { set_error("%s: out_idx is NULL", who); return MMF_E_INVALID; }
  if (nq > 0 && !out_val) { set_error("%s: out_val is NULL", who); return MMF_E_INVALID; }
  const int prec = opts ? opts->precision : MMF_PREC_AUTO;
  if (prec != MMF_PREC_AUTO && prec != MMF_PREC_EXACT && prec != MMF_PREC_FAST && prec != MMF_PREC_FAST_BF16) {
    set_error("%s: precision %d: MMF_PREC_AUTO, _EXACT, _FAST (f16 operands) or _FAST_BF16", who, prec);
    return MMF_E_INVALID;
  }
  if (opts && opts->col_splits < 0) { set_error("%s: col_splits must be >= 0 (got %d)", who, opts->col_splits); return MMF_E_INVALID; }
  if (dp > 8) { set_error("%s: dp = %lld > 8 is not supported", who, (long long)dp); return MMF_E_UNSUPPORTED; }
  const int kk = k + (exclude_self ? 1 : 0);
  if (kk > 44) { set_error("%s: k + self = %d > 44 is not supported (the multi-pass floors are a follow-up)", who, kk); return MMF_E_UNSUPPORTED; }
  if (prec == MMF_PREC_FAST || prec == MMF_PREC_FAST_BF16) {
    if (kk > 20) { set_error("%s: k + self = %d > 20 is not supported (MMF_PREC_EXACT takes up to 44)", who, kk); return MMF_E_UNSUPPORTED; }
    if (d > 4096) { set_error("%s: d = %lld > 4096 is not supported (MMF_PREC_EXACT takes any d)", who, (long long)d); return MMF_E_UNSUPPORTED; }
  }
  if (nq >= ((int64_t)1 << 31) - row_offset) { set_error("%s: row_offset + nq must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (nc >= ((int64_t)1 << 31) - col_offset) { set_error("%s: col_offset + nc must be < 2^31", who); return MMF_E_UNSUPPORTED; }
  if (nq == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MMF_OK; }
  return run_simtopk_combined_xy(who, Fq, Pq, nq, Fc, Pc, nc, d, dp, lambda_h, lambda_g, k, exclude_self, row_offset, col_offset, out_idx,
                                 out_val, opts, stats, device_id, hip_stream);
}

}  // extern "C"
