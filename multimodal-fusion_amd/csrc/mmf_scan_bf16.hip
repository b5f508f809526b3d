// mmf_scan_bf16.hip — the fast all-pairs scan: f16 / bf16 MFMA candidate generation with a proven
// error margin; the exact f32 re-rank (mmf_select.hip) turns the candidates into the final rows.
//
// Shape of the work: like a flash-attention S = Q K^T pass with head dim d and no
// softmax/PV.  A workgroup = 8 waves owns 256 queries for its whole column range (4 waves / 128 queries for d > 512):
//   * each wave keeps its 32 queries RESIDENT IN REGISTERS as the MFMA B operand
//     (KS x 8 halves = 128 VGPRs at d = 512), loaded once;
//   * candidate tiles of 32 rows x d stream L2/HBM -> LDS by buffer-form LDS-DMA (one 1 KiB piece per wave
//     instruction, scalar tile offset) into a 4-stage ring used as two pairs: an iteration reads one pair — TWO
//     tiles per s_barrier — while the pieces of the next pair are issued inside the MFMA chains; at the top of an
//     iteration a wave's outstanding DMA is exactly what the iteration needs (vmcnt(0), barrier);
//   * the LDS image is the candidates' natural row-major layout with the 16-byte chunk index XORed
//     by (row & 15) — applied on the DMA *source* address, LDS stays lane-linear — so every
//     ds_read_b128 of an A fragment is bank-conflict free;
//   * v_mfma_f32_16x16x32_{f16,bf16}, 2 x 2 tiles per wave (32 candidates x 32 queries), four independent
//     accumulator chains: C rows = candidates, C columns = queries, a lane holds TWO queries x 8 candidates per tile;
//     the accumulators are initialised with the per-candidate bias (-n_j/2 for the L2 metrics, -inf for padding)
//     instead of zero, which costs nothing;
//   * epilogue per tile: 14 v_max + 2 compares, reduced before the barrier, tested behind it; only a hit enters
//     the lane-private list code (SlotList, mmf_dev.h).
// X against itself (cosine / dot, d <= 512 padded to 512): launch_scan_b16_sym multiplies every pair of rows of different
// super-blocks ONCE and serves both rows with the value (template flag SYM, DESIGN.md §4.1 "Symmetric scan").
// Where the time goes (profiles/README.md, r02 ablations): the bare ds_read + MFMA chain alone runs at 0.60 of the
// 2.5 PFLOP/s peak (matrix pipe 73 % busy at the 1.94 GHz the chip holds under this load); the tile DMA adds 6 %
// (instruction issue, not traffic), the list code 10 %.
//
// Error margin: with u the f32 rows (normalised for cosine), z = round_16(u), the scanned value
// G = bias_j + z_i.z_j differs from the real-number target Q = bias_j + u_i.u_j by at most
//   E1_i = |dz_i| max|z_j| + |u_i| max|dz_j| + (DP+8) 2^-24 (|z_i| max|z_j| + max|bias|)
// and the canonical f32 key (mapped to Q units) differs from Q by at most E2_i (rounding of the
// chain and of the metric's few f32 ops).  Every column that can be in the canonical top-k has
// G >= (k-th best G) - 2(E1+E2); the lists keep exactly those, so the re-rank sees a superset.
// A list that cannot hold them hands the surplus to the row's overflow list; a row that fills that too is flagged
// and rescanned by the exact kernel.
#include <stdlib.h>

#include <type_traits>

#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int B_CT = 32;
#ifndef MMF_B_CAP
#define MMF_B_CAP 15
#endif
constexpr int B_CAP = MMF_B_CAP;  // list entries per lane for k + self <= 11: what LDS leaves beside four 32 KiB tile stages
constexpr int B_CAP_BIG = 16;     // ... for k + self in 12..20 (costs the fourth tile stage: TPB = 1); what a lane list
                                  // cannot hold goes to the row's overflow list, so the capacity bounds speed, not k
constexpr int B_CAP_WIDE = 32;    // ... for k + self in 21..44, d <= 512: 5 slot bits, ranks counted out of LDS (64 KiB of lists
                                  // beside two 32 KiB tile stages)

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// prep: z = round(u) in bf16/f16, per-row norms of z, of the rounding residual and of u, bias,
// and the column-side maxima the margins need.  One wave per row.
// ------------------------------------------------------------------------------------------------
struct PrepArgs {
  const void* X; int64_t n; int64_t d; int dtype; int metric;
  const float* scal;        // canonical row scalars (n_i, or clamped norm for cosine)
  const uint32_t* max_n;    // float bits of the largest n over both operands (unused for cosine)
  void* Z; int64_t n_pad; int dp; int z_f16;
  float* zn; float* rn; float* un; float* cb;
  uint32_t* maxima;         // [4] float bits: max zn, max rn, max un, max |cb|
  const int32_t* gather;    // optional: position -> row of X (-1 = padding row); n counts positions, scal is indexed by row
};

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// the operands' common power-of-two scale outside prep_half_kernel (ceil_kernel's copy of the block at its top); max_n: float bits of
// the largest squared norm (unused for cosine)
__device__ __forceinline__ float prep_scale(int metric, const uint32_t* max_n) {
  float mx = (metric == MMF_COSINE) ? 1.0f : __builtin_sqrtf(__uint_as_float(max_n[0]));
  int ex = 0;
  if (mx > 0.0f && mx < __builtin_huge_valf()) (void)frexpf(mx, &ex); else ex = 9;
  int e = 9 - ex;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  return ldexpf(1.0f, e);
}

__global__ __launch_bounds__(256) void prep_half_kernel(PrepArgs a) {
  const int lane = threadIdx.x & 63;
  // Common exact power-of-two scale: the largest row norm lands in [256, 512), so f16 keeps its full
  // 11-bit precision on typical elements and cannot overflow.  Scaling by 2^e is exact, it multiplies
  // every scanned value by 2^(2e) and leaves the ranking untouched; the margins are computed from the
  // scaled norms, so they carry the same factor.
  float scale;
  {
    float mx = (a.metric == MMF_COSINE) ? 1.0f : __builtin_sqrtf(__uint_as_float(a.max_n[0]));
    int ex = 0;
    if (mx > 0.0f && mx < __builtin_huge_valf()) (void)frexpf(mx, &ex); else ex = 9;
    int e = 9 - ex;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    scale = ldexpf(1.0f, e);
  }
  // one wave per row, grid-stride over rows; the four column-side maxima are kept per wave and
  // published once at the end (a same-address atomic per row would serialise the whole kernel)
  float m_zn = 0.f, m_rn = 0.f, m_un = 0.f, m_cb = 0.f;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row = wave0; row < a.n_pad; row += nwaves) {
    uint16_t* zrow = reinterpret_cast<uint16_t*>(a.Z) + row * a.dp;
    const int64_t src = (row < a.n && a.gather) ? (int64_t)a.gather[row] : row;
    if (row >= a.n || src < 0) {  // padding rows: zeros, bias -inf so they can never be candidates
      for (int k = lane; k < a.dp; k += 64) zrow[k] = 0;
      if (lane == 0) { a.zn[row] = 0.f; a.rn[row] = 0.f; a.un[row] = 0.f; a.cb[row] = kNegInf; }
      continue;
    }
    const float sc = a.scal[src];
    float s_z = 0.f, s_r = 0.f, s_u = 0.f;
    const bool vec = (a.dtype == MMF_F32) && ((a.d & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15) == 0);
    const bool vec16 = (a.dtype != MMF_F32) && ((a.d & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 7) == 0);
    for (int k4 = lane * 4; k4 < a.dp; k4 += 256) {       // 4 consecutive k per lane: 16 B in, 8 B out
      float u4[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec) {
        if (k4 < a.d) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.X) + src * a.d + k4);
          u4[0] = x4[0]; u4[1] = x4[1]; u4[2] = x4[2]; u4[3] = x4[3];
        }
      } else if (vec16) {                                   // bf16 / f16 rows: 8 bytes per lane, exact upcasts
        if (k4 < a.d) {
          const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(a.X) + src * a.d + k4);
          if (a.dtype == MMF_BF16) {
            u4[0] = __uint_as_float(h.x << 16); u4[1] = __uint_as_float(h.x & 0xffff0000u);
            u4[2] = __uint_as_float(h.y << 16); u4[3] = __uint_as_float(h.y & 0xffff0000u);
          } else {
            u4[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(h.x & 0xffffu)); u4[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(h.x >> 16));
            u4[2] = (float)__builtin_bit_cast(_Float16, (uint16_t)(h.y & 0xffffu)); u4[3] = (float)__builtin_bit_cast(_Float16, (uint16_t)(h.y >> 16));
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (k4 + i < a.d) u4[i] = ld_elem(a.X, src * a.d + k4 + i, a.dtype);
      }
      uint16_t b4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float u = u4[i];
        if (a.metric == MMF_COSINE) u = u / sc;
        u = u * scale;
        float z;
        if (a.z_f16) {
          const _Float16 hz = (_Float16)u;
          z = (float)hz;
          b4[i] = __builtin_bit_cast(uint16_t, hz);
        } else {
          b4[i] = f32_to_bf16_rne(u);
          z = bf16_bits_to_f32(b4[i]);
        }
        const float r = z - u;
        s_z = __builtin_fmaf(z, z, s_z);
        s_r = __builtin_fmaf(r, r, s_r);
        s_u = __builtin_fmaf(u, u, s_u);
      }
      uint2 pk;
      pk.x = (uint32_t)b4[0] | ((uint32_t)b4[1] << 16);
      pk.y = (uint32_t)b4[2] | ((uint32_t)b4[3] << 16);
      *reinterpret_cast<uint2*>(zrow + k4) = pk;            // dp is a multiple of 128: always in range
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s_z += __shfl_xor(s_z, o);
      s_r += __shfl_xor(s_r, o);
      s_u += __shfl_xor(s_u, o);
    }
    const float up = 1.0f + 1e-4f;  // covers the rounding of these sums and square roots
    const float zn = __builtin_sqrtf(s_z) * up, rn = __builtin_sqrtf(s_r) * up, un = __builtin_sqrtf(s_u) * up;
    const float cb = (a.metric == MMF_NEG_SQ_L2 || a.metric == MMF_RBF) ? (-0.5f * sc * scale * scale) : 0.0f;
    if (lane == 0) { a.zn[row] = zn; a.rn[row] = rn; a.un[row] = un; a.cb[row] = cb; }
    m_zn = fmaxf(m_zn, zn); m_rn = fmaxf(m_rn, rn); m_un = fmaxf(m_un, un); m_cb = fmaxf(m_cb, fabsf(cb));
  }
  // Publish once per WORKGROUP: same-address atomics retire at about 90 per microsecond, so one set per wave
  // (16384 x 4 of them) used to be most of this kernel's time.  Non-negative floats order like their bits.
  __shared__ float wmax[4][4];
  const int w = threadIdx.x >> 6;
  if (lane == 0) { wmax[w][0] = m_zn; wmax[w][1] = m_rn; wmax[w][2] = m_un; wmax[w][3] = m_cb; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const float m = fmaxf(fmaxf(wmax[0][threadIdx.x], wmax[1][threadIdx.x]), fmaxf(wmax[2][threadIdx.x], wmax[3][threadIdx.x]));
    if (m > 0.f) atomicMax(a.maxima + threadIdx.x, __float_as_uint(m));
  }
}

// ------------------------------------------------------------------------------------------------
// scan
// ------------------------------------------------------------------------------------------------
struct ScanB16Args {
  const void* ZQ;            // [nq_pad][DP] query side
  const void* ZC;            // [m_pad][DP]  candidate side
  const float* cb;           // [m_pad]
  const float* q_zn; const float* q_rn; const float* q_un;
  const uint32_t* maxima;    // candidate-side maxima
  int64_t n_rows;            // queries
  int64_t m;                 // real candidates
  int64_t tiles_total;       // m_pad / 32
  int64_t tiles_per_split;
  int64_t row_blocks;
  int col_splits;            // power of two
  int conc_splits;           // splits that run side by side (power of two <= 8); the rest follow in later "rounds" of block ids
  int64_t blocks_per_round;
  int lists_total;           // lists per query row in cand_cnt / cand_ids (>= list_base + 2 * col_splits)
  int list_base;             // first list slot written by this launch
  uint32_t seg_len, seg_stride, id_off;   // column i of ZC is reported as id_off + (i / seg_len) * seg_stride + i % seg_len
                                          // (seg_len == 0: id_off + i)
  int32_t* seed;             // [row_blocks * QT] best threshold published for each query by the workgroups / launches
                             // that scan it (order-preserving int encoding, see seed_enc; memset 0x80 = none)
  int32_t* lost;             // [row_blocks * QT] best key any of them dropped (same encoding); the row is rescanned
                             // exactly iff lost >= seed once every launch has finished (audit_kernel)
  int share;                 // other workgroups scan the same queries: import their thresholds on the way
  int kk;
  int metric;
  int d;
  int debug;                 // MMF_SCAN_DEBUG (instrumented build of the same template; scripts/ablate.py): 1 = skip the filter /
                             // list code, 2 = no tile DMA, 4 = no barrier, 32 = DMA of tile 0 only (1, 2, 4, 32: timing only, the
                             // results are wrong), 8 = count events, 16 = cycle stamps, 64 = instrumented build, nothing removed
  unsigned long long* dbg;   // [8] event counters when debug & 8
  uint32_t* lids;            // lane-private id slots: [grid][16][B_NT] (global, written on push, read once at the end)
  uint32_t* cand_cnt; uint32_t* cand_ids; uint32_t* overflow;
  float* cand_keys;          // approximate keys of the entries (select prunes with them), or nullptr
  float* margin_out;         // [n_rows] the queries' error margins, written with cand_keys
  uint32_t* spill_cnt; uint32_t* spill_ids; int spill_cap;   // per-row overflow lists (SpillSink), or nullptr / 0
  int spill_stacks;          // one list pair per row: the two lanes fill the row's slots from both ends, no counter (SpillSink)
  const int32_t* sched;      // SEG / SYM kernels only: [grid][SEG_ENTRY] work table (launch_scan_b16_seg, launch_scan_b16_sym)
  // SYM == 2 (the symmetric launch of a scan of X against itself, launch_scan_b16_sym): a value G_ij that reaches the
  // threshold of its CANDIDATE row j sends its lane's hit record (thresholds and values of the candidate block) to the wave's private
  // log; sym_scatter_kernel picks the passing values out of the records and files them into the rows' lists afterwards
  float* sym_thr;            // [m_pad] threshold of every candidate row (sym_thr_kernel: seed[] decoded; +inf for padding rows), and behind it
                             // [m_pad / 32][4] group minima: the smallest threshold of the eight rows a lane of row group g holds of a tile
  int sym_live;              // the rows' workgroups keep raising sym_thr[] while the symmetric launch runs (sync_seed)
  uint32_t* sym_log;         // [grid * NW][sym_log_cap][16]: hit records (MMF_SYM_RECORDS=0: [sym_log_cap][4] entries)
  uint32_t* sym_log_cnt;     // [3][grid * NW] records written, wave-tiles that passed the group test, wave-tiles with a hit (zeroed by the host;
                             // an idle workgroup writes nothing)
  int sym_log_cap;
  // XSEG kernels only (launch_scan_b16_xseg): [n_pad][2] per query row, first row and row count of the columns the row may not
  // take (its own segment's rows of Y; padding rows: 0, 0)
  const uint32_t* xbounds;
  // CEIL kernels only (launch_scan_b16_ceil, launch_scan_b16_seg_ceil, launch_scan_b16_xseg_ceil): [n_pad] per query row, the largest
  // scanned value the row may still take, in the kernel's own units (bias and 2^(2e) scale included); padding rows: +inf.  Indexed by
  // OPERAND POSITION (qop), like q_zn / q_rn / q_un: the plain schedule's positions are its rows, and so are the cross-segment (XSEG)
  // one's, whose images are the plain ones (launch_scan_b16_ceilings fills both); the table-driven (SEG) one's are positions of the
  // segment-padded query image ([nq_pad]; launch_scan_b16_ceilings_gather fills them through the position -> row table)
  const float* ceil;
};

// Work table entry of a segmented scan (one per workgroup): the row block's first position in the segment-padded query
// image, the list row (= row of X) of its first query, how many of its QT queries are real, its candidate tile range
// in the segment-padded candidate image, and the id offset that turns an image column into a global row id of Y.
enum { SEG_QPOS = 0, SEG_ROW0 = 1, SEG_NQ = 2, SEG_T0 = 3, SEG_T1 = 4, SEG_IDOFF = 5, SEG_ENTRY = 8 };
// Work table entry of the symmetric schedule (sym_schedule_table; same entry size): the workgroup's row block (-1: idle) and
// its columns — tiles [B1, B1 + N1) followed by [B2, B2 + N2) (a cyclic range that wraps, or own + antipodal super-block).
// N1 and N2 are multiples of 8 tiles; N1 == 0 only when N2 == 0.  SLOT: the entry's list pair within its launch (a row block has
// an entry per phase of the symmetric launch, like XSEG_SLOT); PHASE: 0 = a table without phases, 1 / 2 = phase A / B (host only).
enum { SYM_RB = 0, SYM_B1 = 1, SYM_N1 = 2, SYM_B2 = 3, SYM_N2 = 4, SYM_SLOT = 5, SYM_PHASE = 6 };
// Work table entry of the cross-segment scan (cross_seg16_table; same entry size, SEG's words 0 .. 4): both images are the plain
// ones, so the id offset is zero and its word carries the entry's list-slot number; words 6 and 7 are the entry's mask window,
// the tiles [W0, W1) of its range that hold a column some query of the block may not take (W0 == W1: none).
enum { XSEG_SLOT = 5, XSEG_W0 = 6, XSEG_W1 = 7 };

// Order-preserving float <-> int32 map (an involution) so that thresholds can be merged with atomicMax.
__device__ __forceinline__ int32_t seed_enc(float f) {
  const int32_t b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}
constexpr int32_t kSeedNone = (int32_t)0x80808080;   // hipMemset(0x80) pattern: "no threshold yet"

// The margin 2 (E1 + E2) of a query row (see the header) outside the scan kernel — ceil_kernel's copy of the block at the top of
// scan_b16x_kernel, term for term (the kernel keeps its own so that its instantiations stay the instruction streams they were):
// zn / rn / un the row's norms, maxima the candidate side's, dp the padded dim, cap the lane lists' capacity.
__device__ __forceinline__ float scan_margin(int metric, int d, int dp, int cap, float zn, float rn, float un, const uint32_t* maxima) {
  const float ZB = __uint_as_float(maxima[0]), RB = __uint_as_float(maxima[1]);
  const float UB = __uint_as_float(maxima[2]), CB = __uint_as_float(maxima[3]);
  const float g_acc = (float)(dp + 8) * 5.9604645e-8f;
  const float g_chain = (float)(d + 2) * 5.9604645e-8f;
  // + 2^-19 |G| (2^-18 with 5 slot bits): the slot number a stored key carries in its low mantissa bits (SlotList)
  const float slot_eps = (cap <= 16) ? 1.9073486e-6f : 3.8146973e-6f;
  const float e1 = rn * ZB + un * RB + (g_acc + slot_eps) * (zn * ZB + CB);
  float e2;
  if (metric == MMF_DOT) e2 = g_chain * un * UB;
  else if (metric == MMF_COSINE) e2 = (g_chain + 4.7683716e-7f) * un * UB * 1.01f;
  else e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
  return 2.0f * (e1 + e2) * 1.001f + 1e-30f;
}

// LDS-DMA (global -> LDS, no registers) of the 32 biases of a tile.  LDS address = wave-uniform base + lane * 4.
__device__ __forceinline__ void glds4(const void* gptr, const void* lptr) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr), (__attribute__((address_space(3))) void*)(lptr), 4, 0, 0);
}

// MFMA shape: v_mfma_f32_16x16x32_{f16,bf16}.  The kernel was first written on the 32x32x16 shape (one 32 x 32 tile
// per wave, a lane = one query x 16 candidates); operand bytes, LDS image and cycles per flop are identical, but the
// chip holds a higher clock on 16x16x32 under load (MI355X_MICROARCH.md "DVFS give-back" item 7): 10 % less wall
// time on the same box (profiles/README.md; the 32x32x16 form is in the history, commit "scan on v_mfma_f32_16x16x32").
// C layout per 16x16 tile: lane l -> column l & 15, rows 4 (l >> 4) + {0..3}.  A wave covers its 32 queries x the
// 32 candidates of a tile with 2 x 2 tiles acc[cb][qb]: a lane holds TWO queries (l & 15, + 16) x 8 candidates.
// The list code keeps its "one lane = one query, 16 candidates" form: lane l owns query (l & 15) + 16 ((l >> 4) & 1);
// on the (rare) slow path the lanes l and l ^ 16 swap the 8 values they hold for each other's query.
// NW waves per workgroup (32 queries each), TPB tiles per barrier (2 * TPB tile stages in LDS):
//   d <= 512 : NW = 8 (two waves per SIMD, 256 VGPRs each), TPB = 2
//   d <= 1024: SPLITK — NW = 8, TPB = 1: the waves w and w + 4 share 32 queries and a SIMD; each keeps HALF of every
//              query's k range resident (128 VGPRs), walks that half of every tile, and the upper-half wave hands its
//              partial accumulators to the lower-half wave through LDS (one 16 KiB exchange block, acknowledged per
//              tile), which adds them behind the next barrier and runs the filter / lists.  Two waves per SIMD hide
//              each other's DMA issue, as at d <= 512.
//              (k + self in 12..20 at d <= 1024: NW = 4, one wave per SIMD with all of k — its 16-entry lists leave no
//              room for the exchange block.)
//
// SEG (segmented calls): the workgroup's row block, column range and id offset come from the work table a.sched instead
// of blockIdx / col_splits; one workgroup per row block (split 0), queries past the block's count are idle.  List rows
// (lists, thresholds, margins, overflow lists) are rows of X, operand rows are positions of the padded query image.
//
// SYM (a scan of X against itself split into two launches, launch_scan_b16_sym; DESIGN.md §4.1 "Symmetric scan"): the row
// block and its columns — two tile ranges walked as one — come from the work table a.sched.  SYM == 1 is otherwise the plain
// kernel.  SYM == 2 serves both directions of every pair it multiplies: beside the query-side filter, each value is tested
// against the threshold of its CANDIDATE row (32 floats per tile, DMAed into LDS with the tile's biases), and a value that
// passes makes its lane append a hit record to a log private to the wave — a ballot and a popcount place it: four stores, no atomic, no
// returned value to wait for (the stores retire with the iteration's vmcnt(0), like the tile DMA).
#ifndef MMF_SYM_ABLATE
#define MMF_SYM_ABLATE 0   // timing-only variants of the SYM == 2 kernel's candidate direction (sym_offer below)
#endif
#ifndef MMF_SYM_EARLY_THR
#define MMF_SYM_EARLY_THR 1   // SYM == 2: 1 = ONE 64-lane threshold DMA per iteration for both tiles of the next group, issued between
#endif                        // the iteration's two chains; 0 = one 32-lane DMA behind each chain (the placement before; scripts/ab_build.sh)
#ifndef MMF_SYM_RECORDS
#define MMF_SYM_RECORDS 1     // SYM == 2: 1 = a lane with a hit appends one 64-byte record per candidate block (its four thresholds and eight
#endif                        // values; sym_scatter_kernel does the per-value test), 0 = the per-value entry path before it (scripts/ab_build.sh)
#ifndef MMF_SYM_COARSE
#define MMF_SYM_COARSE 1      // SYM == 2: 1 = behind a chain the candidate side costs ONE compare, the lane's largest value against the minimum of its
#endif                        // eight rows' thresholds (the group minima, sym_offer); the per-row test runs in the cold block behind it.  0 = the
                              // per-row test behind every chain, as before (scripts/ab_build.sh)
#if MMF_SYM_COARSE && !MMF_SYM_EARLY_THR
#error "MMF_SYM_COARSE: the group minima ride on the paired threshold DMA (MMF_SYM_EARLY_THR=1)"
#endif
#ifndef MMF_SYM_CHAIN_WAIT
#define MMF_SYM_CHAIN_WAIT 1  // SYM == 2: 1 = the cold blocks of the hot tests end with lgkmcnt(0), so the chain behind them opens with a counted
#endif                        // wait for its A fragments; 0 = as before, the chain waits for all its leading reads (scripts/ab_build.sh)
#ifndef MMF_SYM_SCALAR_ANY
#define MMF_SYM_SCALAR_ANY 1  // SYM != 0: 1 = the hot tests branch on the ballot's scalar pair, 0 = on __any (scripts/ab_build.sh)
#endif
// The SYM kernels have no instrumented (DBG) build; their query-side list code is measured with two build switches (scripts/ab_build.sh):
#ifndef MMF_SYM_ABLATE_Q
#define MMF_SYM_ABLATE_Q 0    // timing only, the results are WRONG: bit 0 / bit 1 = the SYM == 1 / SYM == 2 kernel never enters the query-side list code
#endif                        // bit 2 = ... and the tile maxima are folded into one value that is stored at the end.  WITHOUT bit 2 nothing reads the
                              // SYM == 1 kernel's accumulators and the compiler drops its MFMA chain: such a build does not time the matrix work
#ifndef MMF_SYM_COUNT
#define MMF_SYM_COUNT 0       // 1 = both SYM launches count wave-tiles, visits, hits and compactions (MMF_SCAN_DEBUG bit 8's counters)
#endif                        //     and launch_scan_b16_sym prints them per launch (it synchronises the stream: not for timing)
//
// XSEG (implies SEG; mmf_simtopk_cross_segments_fast): every row against the columns OUTSIDE its own segment, on the
// plain images of both sides (column = row of Y, no id offset).  The schedule is SEG's plus the entry's list slot (a row block has
// several entries, which share thresholds through a.share) and its mask window.  A tile inside the window goes through a cold,
// wave-uniform branch behind its chain: the lane fetches the excluded column range (first, count) of its two queries from
// a.xbounds and sets each of its 16 values whose column lies inside to -inf — before max_qb, acc_prev and filter, so a masked value
// reaches no list, overflow list, threshold, seed or lost.  SPLITK: only the owner wave masks; -inf survives the partner's partial sums.
//
// CEIL (mmf_simtopk_fast_anyk, DESIGN.md §4.27: the plain schedule; mmf_simtopk_segmented_fast_anyk, §4.29: with SEG, four depth
// shapes — launch_b16_seg_ceil_for; mmf_simtopk_cross_segments_fast_anyk, §4.30: with XSEG, the same four shapes —
// launch_b16_xseg_ceil_for): the later passes of a call with more neighbours than one
// pass holds.  Every query row comes with a ceiling a.ceil[row]; a value above it belongs to a column the row has already emitted.
// Such a value is above the row's threshold by construction, so it enters the list code as a hit anyway: the compare sits THERE, on
// the lane's 16 gathered values before they are offered — the tile loop's v_max + two compares are untouched, and the ceiling is
// loaded inside the branch, so the loop carries no register for it.  A value set to -inf there reaches no list, overflow list,
// threshold, seed or lost.  SPLITK: only the owner wave runs the list code, so only it compares.
// With XSEG the two do not meet: the mask has made a value -inf behind its tile's chain, before the list code gathers it, and the
// ceiling compare leaves -inf alone; a value either of them removes reaches no threshold the entries of a row block share (a.share).
template <int KS, bool F16, bool DBG, int NW, int TPB, int CAP, bool SPLITK = false, bool SEG = false, int SYM = 0, bool XSEG = false,
          bool CEIL = false>
__global__ __launch_bounds__(64 * NW, (NW == 8) ? 2 : 1) void scan_b16x_kernel(ScanB16Args a) {
  static_assert(!CEIL || (SYM == 0 && !DBG), "per-row ceilings: the plain and the table-driven schedules (SEG, XSEG) only");
  static_assert(!SPLITK || (TPB == 1 && NW == 8 && (KS % 8) == 0), "split-k pairs");
  static_assert(SYM == 0 || (!SPLITK && !SEG && !DBG && TPB == 2), "symmetric schedule: the d = 512 kernel only");
  static_assert(!XSEG || (SEG && SYM == 0 && !DBG), "the cross-segment mask rides on the table-driven schedule");
  constexpr int NQW = SPLITK ? NW / 2 : NW;     // waves that own queries and lists
  constexpr int NTL = 64 * NQW;                 // threads that own lists
  constexpr int QT = 32 * NQW;
  constexpr int STAGES = 2 * TPB;
  constexpr int ROWB = KS * 32;                 // bytes per candidate row in LDS (= DP * 2)
  constexpr int TILEB = B_CT * ROWB;            // bytes per tile
  constexpr int PIECES = TILEB / 1024;          // 1 KiB DMA pieces per tile (= KS)
  constexpr int PPW = (PIECES + NW - 1) / NW;
  static_assert(PIECES % NW == 0, "piece distribution");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* tiles = smem;                                                  // [STAGES][TILEB]
  float* cbs = reinterpret_cast<float*>(smem + STAGES * TILEB);      // [STAGES][64]
  // Candidate lists (SlotList, mmf_dev.h): approximate keys in LDS, column ids in a global slot block of
  // this workgroup — leaving most of LDS to the tile ring is what buys the fourth stage.
  float* lkeys = cbs + STAGES * 64;                                  // [CAP][NTL]
  uint32_t* lids = a.lids + (size_t)blockIdx.x * (SlotList<CAP, NTL>::SLOTS * NTL);
  f32x4* xch = reinterpret_cast<f32x4*>(lkeys + CAP * NTL);          // SPLITK: [NQW][4][64] partial accumulators
  volatile int* ack = reinterpret_cast<volatile int*>(xch + NQW * 4 * 64);   // SPLITK: [NQW] last tile the lower wave took
  // SYM == 2: the thresholds of a tile's candidate rows and their group minima take the bias stages (sym_thr_stage below)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int khalf = SPLITK ? wave / NQW : 0;    // which half of k this wave multiplies
  const int qw = SPLITK ? wave % NQW : wave;    // which 32 queries
  const bool owner = khalf == 0;                // bias, filter and lists live in the lower-half wave
  const int half = lane >> 5;
  const int g = lane >> 4;                      // row group of the C layout: rows 4 g .. 4 g + 3 of each 16-row tile
  const int c16 = lane & 15;
  const int ownb = g & 1;                       // the query block (0 / 1) whose list this lane owns
  const int c = c16 + 16 * ownb;                // own query within the wave

  // XCD-aware block -> (row block, split): blocks that share blockIdx % 8 share an XCD (observed
  // round-robin placement; speed only) and are given the same column range, so its tiles are L2 hits.
  // Splits beyond the `conc_splits` that run side by side follow in later rounds of block ids, i.e. later in
  // dispatch order: their workgroups start from the thresholds the earlier ones published (a.seed).
  int64_t rb;
  int split;
  int64_t t_begin, t_end, row0 = 0;
  int nq = 0;
  uint32_t id_off = a.id_off;
  int sym_n1 = 0, sym_skip = 0;   // SYM: tiles of the first range, and how many tiles lie between its end and the second range's start
  int xw0 = 0, xw1 = 0;           // XSEG: the mask window, as tile numbers inside this entry's range
  if constexpr (SYM != 0) {
    const int32_t* e = a.sched + (size_t)blockIdx.x * SEG_ENTRY;
    if (e[SYM_RB] < 0) return;
    rb = e[SYM_RB]; split = SYM == 2 ? e[SYM_SLOT] : 0;
    t_begin = e[SYM_B1]; t_end = t_begin + e[SYM_N1] + e[SYM_N2];      // walked as one range of N1 + N2 tiles
    sym_n1 = e[SYM_N1]; sym_skip = e[SYM_B2] - (e[SYM_B1] + e[SYM_N1]);
  } else if constexpr (SEG) {
    const int32_t* e = a.sched + (size_t)blockIdx.x * SEG_ENTRY;
    rb = e[SEG_QPOS] / QT; row0 = e[SEG_ROW0]; nq = e[SEG_NQ];
    t_begin = e[SEG_T0]; t_end = e[SEG_T1];
    if constexpr (XSEG) {
      id_off = 0u; split = e[XSEG_SLOT];
      xw0 = e[XSEG_W0] - e[SEG_T0]; xw1 = e[XSEG_W1] - e[SEG_T0];
    } else {
      id_off = (uint32_t)e[SEG_IDOFF];
      split = 0;
    }
  } else {
    const int CS = a.conc_splits;
    const int64_t round = blockIdx.x / a.blocks_per_round;
    const int64_t j = blockIdx.x - round * a.blocks_per_round;
    const int64_t q = j >> 3;
    const int x = (int)(j & 7);
    split = (int)round * CS + x % CS;
    rb = q * (8 / CS) + x / CS;
    if (rb >= a.row_blocks) return;
    t_begin = (int64_t)split * a.tiles_per_split;
    t_end = t_begin + a.tiles_per_split;
    if (t_end > a.tiles_total) t_end = a.tiles_total;
    if (t_begin > t_end) t_begin = t_end;
  }
  const int64_t q0 = rb * QT;
  const int64_t T = t_end - t_begin;

  const int64_t qop = q0 + 32 * qw + c;                    // operand position of this lane's query
  const int64_t qpos = SEG ? row0 + 32 * qw + c : qop;     // its list row
  const bool qvalid = (SEG ? (32 * qw + c < nq) : (qpos < a.n_rows)) && owner;

  // margin of this lane's query (see the header): 2 (E1 + E2)
  float margin;
  {
    const float ZB = __uint_as_float(a.maxima[0]), RB = __uint_as_float(a.maxima[1]);
    const float UB = __uint_as_float(a.maxima[2]), CB = __uint_as_float(a.maxima[3]);
    const float zn = a.q_zn[qop], rn = a.q_rn[qop], un = a.q_un[qop];   // arrays are padded
    const float g_acc = (float)(KS * 16 + 8) * 5.9604645e-8f;
    const float g_chain = (float)(a.d + 2) * 5.9604645e-8f;
    // + 2^-19 |G| (2^-18 with 5 slot bits): the slot number a stored key carries in its low mantissa bits (SlotList)
    const float slot_eps = (CAP <= 16) ? 1.9073486e-6f : 3.8146973e-6f;
    const float e1 = rn * ZB + un * RB + (g_acc + slot_eps) * (zn * ZB + CB);
    float e2;
    if (a.metric == MMF_DOT) e2 = g_chain * un * UB;
    else if (a.metric == MMF_COSINE) e2 = (g_chain + 4.7683716e-7f) * un * UB * 1.01f;
    else e2 = g_chain * un * UB + 2.3841858e-7f * (un * un + UB * UB);
    margin = 2.0f * (e1 + e2) * 1.001f + 1e-30f;
  }

  SlotList<CAP, NTL> list;
  list.init(lkeys + (tid & (NTL - 1)), lids + (tid & (NTL - 1)));
  if (!qvalid) list.thr = __builtin_huge_valf();
  else if (a.spill_cnt) {
    list.sink.cnt = a.spill_cnt; list.sink.ids = a.spill_ids; list.sink.cap = (uint32_t)a.spill_cap; list.sink.row = qpos;
    list.sink.seg_len = a.seg_len; list.sink.seg_stride = a.seg_stride; list.sink.id_off = id_off;
    if (DBG) list.sink.ablate = (a.debug & 128) ? 1 : 0;
    if (a.spill_stacks) list.sink.stacks = 1 + half;
  }
  // Thresholds are shared between the workgroups (and launches) that scan different columns for the same
  // queries: any list's threshold bounds the approximate key of every member of the final top-k, whatever
  // columns it sits in.  sync_seed publishes this lane's threshold when it has risen (and is not the product
  // of a dropped key) and adopts the best one published so far; it runs at the start and every 64 tiles.
  float pub = -kFltMax;
  bool seed_rose = false;   // SYM == 2: the last sync_seed published a risen threshold of this lane (sync_tmin)
  auto sync_seed = [&]() {
    if (!qvalid) return;
    bool rose = false;
    if (list.thr > pub && list.thr > list.lost) {
      pub = list.thr;
      atomicMax(a.seed + qpos, seed_enc(pub));
      rose = true;
    }
    if (!a.share) return;
    const int32_t o = __hip_atomic_load(a.seed + qpos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o > kSeedNone) {
      const float t = __int_as_float(o >= 0 ? o : (o ^ 0x7fffffff));
      if (t > list.thr) { list.thr = t; pub = t; }
    }
    // SYM == 2, live image: the risen threshold also goes to the image the OTHER rows' candidate-side tests read (issue_thr).
    // Any value ever published for a row is a valid threshold for it, so neither the order in which the row's two lanes
    // store nor how late a reader sees the store matters; agent scope makes it leave this XCD's L2 while the kernel runs.
    if constexpr (SYM == 2) {
      // (the lane's byte offset is made opaque HERE: left alone the compiler forms the 64-bit address in front of the tile loop, and
      //  that pair of registers, live across the loop, is what the kernel would spill; the image is below 4 GiB, launch_scan_b16_sym)
      if (rose && a.sym_live) {
        uint32_t off = (uint32_t)qpos * 4u;
        asm volatile("" : "+v"(off));
        __hip_atomic_store(reinterpret_cast<float*>(reinterpret_cast<char*>(a.sym_thr) + off), list.thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seed_rose = true;
      }
    }
  };
  // SYM == 2, live image: ... and the group minima follow (the hot test of sym_offer reads them); called behind sync_seed, by the
  // whole wave.  `pub` is a value published for
  // the lane's row (or -FLT_MAX), so the minimum over the 16 lanes that own the lists of a group's eight rows is a minimum of
  // published values: below it a value is below a valid threshold of its own row, whichever of the two images a reader sees newer.
  // A row past n_rows counts as +inf, as in sym_thr_kernel.  Same store as the threshold image's; any order of the stores of the
  // workgroups that share the rows leaves a valid minimum.
  auto sync_tmin = [&]() {
    if (__any(seed_rose)) {
      float v = qvalid ? pub : __builtin_huge_valf();
      v = fminf(v, __shfl_xor(v, 1)); v = fminf(v, __shfl_xor(v, 2));      // the four queries of the group in this lane's query block
      v = fminf(v, __shfl_xor(v, 16)); v = fminf(v, __shfl_xor(v, 32));    // both query blocks, both lists of a row
      if ((lane & 0x33) == 0)
        __hip_atomic_store(a.sym_thr + a.tiles_total * B_CT + ((q0 >> 5) + qw) * 4 + (c16 >> 2), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    seed_rose = false;
  };
  // the wave-uniform branches of the SYM kernels' hot tests: on scalar registers.  __any of an OR of compares goes through a VGPR
  // (v_cndmask 0, 1 + v_cmp_ne on top of the s_or_b64 that already holds the answer), and so does the ballot of such an OR; the
  // ballot of ONE compare is the compare's own SGPR pair, so the tests OR their compares' ballots (sym_hits) and branch on that.
  // (The empty asm keeps the pair where it is: left to itself the compiler folds `ballot != 0` back into the VGPR form.)
  constexpr bool SCALAR_ANY = SYM != 0 && MMF_SYM_SCALAR_ANY != 0;
  auto sym_hits = [&](unsigned long long b) -> bool { asm("" : "+s"(b)); return b != 0ull; };
  if (a.share) sync_seed();
  // a wave whose queries all start from a published threshold skips the cold-start treatment
  const bool seeded = !__any(list.thr == -kFltMax);

  // resident query fragments: B operand of k-step s (32 wide), query block qb: lane holds
  // Z[q0 + 32 w + 16 qb + c16][32 s + 8 g .. +7]
  constexpr int KS2 = SPLITK ? KS / 4 : KS / 2;      // 32-wide k-steps this wave multiplies
  const int kbyte = khalf * KS2 * 64;                // byte offset of its k range inside a row
  u32x4 qf[KS2][2];
  {
    const char* qbase = reinterpret_cast<const char*>(a.ZQ) + (q0 + 32 * qw + c16) * (int64_t)ROWB + g * 16 + kbyte;
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      qf[s][0] = *reinterpret_cast<const u32x4*>(qbase + s * 64);
      qf[s][1] = *reinterpret_cast<const u32x4*>(qbase + 16 * (int64_t)ROWB + s * 64);
    }
    // make the compiler retire these loads HERE: otherwise it cannot prove them complete at their first use
    // inside the tile loop and puts s_waitcnt vmcnt(0) there, which drains the tile DMA in flight every iteration
#pragma unroll
    for (int s = 0; s < KS2; ++s) { asm volatile("" : "+v"(qf[s][0])); asm volatile("" : "+v"(qf[s][1])); }
  }

  // A-fragment read offsets inside a tile: row c16 (+ 16 cb), 16-byte chunk (4 s + g) ^ (row & 15)
  int lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) lo[j] = c16 * ROWB + ((((4 * j + g) ^ c16) & 15) << 4);

  // DMA roles: piece p of a tile covers LDS bytes [1024 p, 1024 p + 1024); lane writes 16 B at l*16.
  // Source = wave-uniform running tile pointer + a loop-invariant 32-bit lane offset.
  uint32_t src_off[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = wave + NW * i;
    const int off = p * 1024 + lane * 16;
    const int r = off / ROWB;
    const int chunk = (off % ROWB) >> 4;
    const int src_chunk = (chunk & ~15) | ((chunk ^ r) & 15);
    src_off[i] = (uint32_t)(r * ROWB + src_chunk * 16);
  }
  // (SYM: the second range may lie BELOW the first, so the buffers start at the image's first tile and zt0 / ct0 point at the
  //  range's; the host has checked that the whole image stays inside the 32-bit offsets)
  const char* zc0 = reinterpret_cast<const char*>(a.ZC) + (SYM != 0 ? 0 : t_begin * (int64_t)TILEB);          // tile 0 of my range
  const char* cb0 = reinterpret_cast<const char*>(a.cb + (SYM != 0 ? 0 : t_begin * B_CT));
  const char* zt0 = SYM != 0 ? zc0 + t_begin * (int64_t)TILEB : zc0;
  const char* ct0 = SYM != 0 ? cb0 + t_begin * B_CT * 4 : cb0;
  // Tile pieces go through the buffer form of the LDS-DMA: the workgroup's column range is one raw buffer
  // (base = its first tile), the running tile position is the scalar offset and the lane's swizzled position
  // the vector offset — no per-piece 64-bit address arithmetic in the MFMA chain, and (unlike the FLAT-encoded
  // global form) it leaves the compiler's counted lgkmcnt waits for the A-fragment ring intact.
  const __amdgpu_buffer_rsrc_t zrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zc0), 0, -1, 0x00020000);
  auto issue_piece = [&](const char* tsrc, int stage, int i) {
    if (DBG && (a.debug & 2)) return;       // timing-only ablation: no tile DMA (the chain runs on whatever LDS holds)
    if (DBG && (a.debug & 32)) tsrc = zc0;  // timing-only ablation: every piece re-fetches tile 0 (issue cost without the traffic)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(zrsrc, (__attribute__((address_space(3))) void*)(tiles + stage * TILEB + (wave + NW * i) * 1024),
                                             16, (int)src_off[i], (int)(uint32_t)(tsrc - zc0), 0, 0);
  };
  // the 32 biases of a tile: one 4-byte DMA by lanes 0..31 of the wave whose turn it is
  // (buffer form like the tile pieces: the FLAT-encoded global form makes the compiler wait lgkmcnt(0) where the
  // A-fragment ring wants counted waits)
  const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(cb0), 0, -1, 0x00020000);
  auto issue_bias = [&](const char* bsrc, int stage) {
    const uint32_t l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // lane id, no live VGPR
    if (l < 32)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(brsrc, (__attribute__((address_space(3))) void*)(cbs + stage * 64), 4, (int)(l * 4u),
                                               (int)(uint32_t)(bsrc - cb0), 0, 0);
  };
  // SYM == 2: the thresholds of the same 32 rows, same form, same place in the iteration, issued by another wave
  // They live in the bias stages, which the SYM kernels leave unused: per stage group, the 64 thresholds of its two tiles and behind
  // them the 2 x 4 group minima — 288 contiguous bytes, what one DMA writes (issue_thr_pair)
  constexpr int SYM_GRP = 2 * B_CT + 8;
  static_assert(SYM != 2 || (2 * SYM_GRP <= STAGES * 64 && TPB == 2), "thresholds and group minima in the bias stages");
  auto sym_thr_stage = [&](int stage) -> float* { return cbs + (stage >> 1) * SYM_GRP + (stage & 1) * B_CT; };
  auto sym_min_stage = [&](int stage) -> float* { return cbs + (stage >> 1) * SYM_GRP + 2 * B_CT + (stage & 1) * 4; };
  // (cache policy 16 = sc1, what the compiler emits for an agent-scope load: the image is rewritten by other XCDs' workgroups
  //  while this kernel runs (sync_seed), and a plain load could be served from a stale line of this XCD's L2 for as long as
  //  it stays there)
  auto issue_thr = [&](const char* bsrc, int stage) {
    const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(a.sym_thr, 0, -1, 0x00020000);
    const uint32_t l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (l < 32)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(trsrc, (__attribute__((address_space(3))) void*)sym_thr_stage(stage), 4, (int)(l * 4u),
                                               (int)(uint32_t)(bsrc - cb0), 0, 16);
  };

  // ... and of the 64 rows of BOTH tiles of a group in one DMA by all 64 lanes: a group's two tiles are consecutive rows (ranges
  // are multiples of 8 tiles and the jump to the second range sits on a group boundary) and its two stages are adjacent
  auto issue_thr_pair = [&](const char* bsrc, int stage) {
    const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(a.sym_thr, 0, -1, 0x00020000);
    const uint32_t l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if constexpr (MMF_SYM_COARSE != 0) {
      // ... 16 bytes a lane: lanes 0..15 carry the 64 thresholds, lanes 16 and 17 the two tiles' group minima, which lie behind the
      // threshold image (4 floats per tile: an eighth of the rows' byte offset), the other lanes nothing
      const uint32_t off = (uint32_t)(bsrc - cb0);
      const uint32_t voff = l < 16u ? off + l * 16u : (uint32_t)a.tiles_total * (B_CT * 4u) + (off >> 3) + (l - 16u) * 16u;
      if (l < 18u)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(trsrc, (__attribute__((address_space(3))) void*)sym_thr_stage(stage), 16, (int)voff, 0, 0, 16);
    } else
    __builtin_amdgcn_raw_ptr_buffer_load_lds(trsrc, (__attribute__((address_space(3))) void*)sym_thr_stage(stage), 4, (int)(l * 4u),
                                             (int)(uint32_t)(bsrc - cb0), 0, 16);
  };

  if (SPLITK && tid < NQW) ack[tid] = -1;
  const int Ti = (int)T;
  if (Ti > 0) {   // first group of TPB tiles -> stages 0 .. TPB-1
#pragma unroll
    for (int u = 0; u < TPB; ++u) {
      const bool real = u < Ti;
#pragma unroll
      for (int i = 0; i < PPW; ++i) issue_piece(real ? zt0 + u * (int64_t)TILEB : zc0, u, i);
      if constexpr (SYM == 0) { if (wave == (u & (NW - 1))) issue_bias(real ? ct0 + u * B_CT * 4 : cb0, u); }
      if constexpr (SYM == 2 && !MMF_SYM_EARLY_THR) { if (wave == ((u + 4) & (NW - 1))) issue_thr(real ? ct0 + u * B_CT * 4 : cb0, u); }
    }
    if constexpr (SYM == 2 && MMF_SYM_EARLY_THR) { if (wave == 4) issue_thr_pair(Ti >= TPB ? ct0 : cb0, 0); }
  }
  // The DMA pieces of tile t+TPB are issued inside the MFMA chain of tile t, one per group of GRP MFMAs.  The
  // chain is straight-line code and the DMA is unconditional — past the end of the range it re-fetches tile 0
  // into a stage nobody reads again — so no branch and no per-tile bookkeeping sits between the MFMAs.
  // (Issuing at different points of the chain for the two waves that share a SIMD used to pay when a piece cost
  // 64-bit address arithmetic; with the buffer form it measures 0.8 % slower than issuing at the same point.)
  constexpr int GRP = KS2 / PPW;                     // k-steps (4 MFMAs each) between two DMA pieces (issuing the SPLITK
                                                     // kernel's pieces in its first k-steps instead measured the same)
  static_assert(KS2 % PPW == 0 && GRP >= 1, "DMA piece placement");
  const char* tsrc = zt0 + TPB * (int64_t)TILEB;     // source of the first tile of the NEXT group
  const char* bsrc = ct0 + TPB * B_CT * 4;
  const uint32_t id_base = (uint32_t)(t_begin * B_CT);

  struct Acc { f32x4 t[2][2]; };                     // [candidate block][query block]
  auto tile_body = [&](const char* tb, const float* cbt, const char* src, int s2) -> Acc {
    Acc acc;
    if constexpr (SYM != 0) {   // cosine / dot only (launch_scan_b16_sym): the bias of every real row is zero — no stage, no read;
                                // padding rows are masked behind the chain (mask_padding)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) { acc.t[cb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc.t[cb][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    } else {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      f32x4 b4 = *reinterpret_cast<const f32x4*>(cbt + 16 * cb + 4 * g);
      if (SPLITK && !owner) b4 = f32x4{0.f, 0.f, 0.f, 0.f};      // the bias is added once, by the lower-half wave
      acc.t[cb][0] = b4; acc.t[cb][1] = b4;
    }
    }
    // A fragments are read PD k-steps ahead of the MFMAs that consume them (explicit register ring)
    constexpr int PD = 2;
    u32x4 af[PD][2];
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      af[s][0] = *reinterpret_cast<const u32x4*>(tb + lo[s & 3] + (s >> 2) * 256);
      af[s][1] = *reinterpret_cast<const u32x4*>(tb + lo[s & 3] + (s >> 2) * 256 + 16 * ROWB);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * PD, 0);   // the leading reads first
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      const u32x4 a0 = af[s % PD][0], a1 = af[s % PD][1];
      if (s + PD < KS2) {
        af[s % PD][0] = *reinterpret_cast<const u32x4*>(tb + lo[(s + PD) & 3] + ((s + PD) >> 2) * 256);
        af[s % PD][1] = *reinterpret_cast<const u32x4*>(tb + lo[(s + PD) & 3] + ((s + PD) >> 2) * 256 + 16 * ROWB);
      }
      if constexpr (F16) {
        acc.t[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a0), __builtin_bit_cast(f16x8_t, qf[s][0]), acc.t[0][0], 0, 0, 0);
        acc.t[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a0), __builtin_bit_cast(f16x8_t, qf[s][1]), acc.t[0][1], 0, 0, 0);
        acc.t[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a1), __builtin_bit_cast(f16x8_t, qf[s][0]), acc.t[1][0], 0, 0, 0);
        acc.t[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a1), __builtin_bit_cast(f16x8_t, qf[s][1]), acc.t[1][1], 0, 0, 0);
      } else {
        acc.t[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a0), __builtin_bit_cast(bf16x8_t, qf[s][0]), acc.t[0][0], 0, 0, 0);
        acc.t[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a0), __builtin_bit_cast(bf16x8_t, qf[s][1]), acc.t[0][1], 0, 0, 0);
        acc.t[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a1), __builtin_bit_cast(bf16x8_t, qf[s][0]), acc.t[1][0], 0, 0, 0);
        acc.t[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a1), __builtin_bit_cast(bf16x8_t, qf[s][1]), acc.t[1][1], 0, 0, 0);
      }
      // one DMA piece of tile t+TPB per GRP k-steps
      if ((s % GRP) == GRP - 1) issue_piece(src, s2, s / GRP);
      // pin the interleave: the two LDS reads of step s+PD, then the four MFMAs of step s
      if (s + PD < KS2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    return acc;
  };
  // per query block: the largest of the 8 values this lane holds for it
  auto max_qb = [&](const Acc& x, int qb) -> float {
    const f32x4& p = x.t[0][qb];
    const f32x4& q = x.t[1][qb];
    return fmaxf(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])), fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3])));
  };
  // SYM: without a bias nothing rejects the padding rows of the image's last row block (zero operands: G = 0, which beats the real
  // candidates of a row whose best cosines are negative).  A wave-uniform test per tile — does it reach past the real rows — sends
  // exactly those tiles through a cold branch that sets the padding rows' values to -inf, what their bias used to make them.
  auto mask_padding = [&](Acc& x, int tt) {
    const int64_t r0 = (int64_t)id_base + (int64_t)tt * B_CT + ((tt >= sym_n1) ? (int64_t)sym_skip * B_CT : 0);   // first row of the tile
    if (__builtin_expect(r0 + B_CT > a.m, 0)) {
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          if (r0 + 16 * cb + 4 * g + jj >= a.m) { x.t[cb][0][jj] = kNegInf; x.t[cb][1][jj] = kNegInf; }
        }
      }
    }
  };
  // XSEG: the columns a query may not take.  The window test is wave-uniform and almost always false (a block inside one segment
  // has at most two such tiles); the four bound words are loaded inside the branch, so the tile loop carries no register for them.
  auto mask_excluded = [&](Acc& x, int tt) {
    if (__builtin_expect(tt >= xw0 && tt < xw1, 0)) {
      if (owner) {
        const uint32_t* bq = a.xbounds + 2 * (q0 + 32 * qw + c16);       // query block 0; block 1 is 16 rows on
        const uint2 b0 = *reinterpret_cast<const uint2*>(bq);
        const uint2 b1 = *reinterpret_cast<const uint2*>(bq + 32);
        const uint32_t j0 = id_base + (uint32_t)tt * B_CT + 4u * (uint32_t)g;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const uint32_t j = j0 + 16u * cb + jj;
            if ((uint32_t)(j - b0.x) < b0.y) x.t[cb][0][jj] = kNegInf;
            if ((uint32_t)(j - b1.x) < b1.y) x.t[cb][1][jj] = kNegInf;
          }
        }
      }
    }
  };
  // thresholds of the two queries this lane holds values for: its own list's and its partner's (lane ^ 16);
  // they change only inside the list code and in sync_seed, and are re-read from the partner there
  float thr_q0, thr_q1;
  auto refresh_thr = [&]() {
    const float mine = list.thr;
    const float theirs = __shfl_xor(mine, 16);
    thr_q0 = ownb ? theirs : mine;
    thr_q1 = ownb ? mine : theirs;
  };
  refresh_thr();

  // The filter of tile t-1 runs AFTER barrier t, ahead of this wave's own MFMA chain: a wave that
  // falls into the (rare) list code then delays only itself while its SIMD partner issues MFMAs;
  // placed before the barrier it would hold all eight waves, and their matrix pipes, at the barrier.
  constexpr bool SYMCNT = SYM != 0 && MMF_SYM_COUNT != 0;
  float ablate_keep = -kFltMax;   // MMF_SYM_ABLATE_Q bit 2: the tile maxima folded into one value, stored once at the end
  auto filter = [&](const Acc& acc, int tt, float m0, float m1) {
    if (SYM != 0 && (MMF_SYM_ABLATE_Q & SYM) != 0 && (MMF_SYM_ABLATE_Q & 4) != 0) ablate_keep = fmaxf(ablate_keep, fmaxf(m0, m1));
    if (__builtin_expect(!(DBG && (a.debug & 1)) && !(SYM != 0 && (MMF_SYM_ABLATE_Q & SYM) != 0) &&
                         (SCALAR_ANY ? sym_hits(__builtin_amdgcn_ballot_w64(m0 >= thr_q0) | __builtin_amdgcn_ballot_w64(m1 >= thr_q1))
                                     : __any((m0 >= thr_q0) || (m1 >= thr_q1)) != 0), 0)) {
      uint32_t id0 = id_base + (uint32_t)tt * B_CT;
      if constexpr (SYM != 0) id0 += (tt >= sym_n1) ? (uint32_t)(sym_skip * B_CT) : 0u;   // behind the first range: sym_skip tiles further on
      // this lane's query gets its 16 candidates together: its own 8 plus the 8 the partner lane holds
      f32x16 v;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float mine = ownb ? acc.t[cb][1][j] : acc.t[cb][0][j];
          const float give = ownb ? acc.t[cb][0][j] : acc.t[cb][1][j];
          v[4 * cb + j] = mine;
          v[8 + 4 * cb + j] = __shfl_xor(give, 16);
        }
      }
      if constexpr (CEIL) {   // columns the row has already emitted (and nothing that ranks after its floor: §4.27) lie above its ceiling
        float ce;
        if constexpr (XSEG) {   // the same word, a.ceil[qop], addressed from the wave's scalar base and a lane id read here: with qop kept
          // live across the tile loop beside the mask's operands the d = 512 kernel spills a VGPR
          const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
          ce = (a.ceil + (q0 + 32 * qw))[(ln & 15) + (ln & 16)];
        } else ce = a.ceil[qop];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = (v[r] > ce) ? kNegInf : v[r];
      }
      // v[0..7]: rows of this lane's group g, v[8..15]: rows of the partner's group g ^ 1 (4 g ^ 4)
      const int g4 = 4 * g;
      auto rowof = [g4](int r) -> uint32_t { return (uint32_t)((g4 ^ ((r & 8) >> 1)) + (r & 3) + 16 * ((r >> 2) & 1)); };
      // robust (never dropping) path while thresholds are still forming: first 32 tiles of the range
      const bool cold = (!seeded && tt < 32) || __any(list.thr == -kFltMax);
      if ((DBG && (a.debug & 8)) || SYMCNT) {
        const bool willc = __any(list.cnt >= CAP - 1);
        int nh = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) nh += (v[r] >= list.thr) ? 1 : 0;
        const int lanes_hit = __popcll(__ballot(nh > 0));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nh += __shfl_xor(nh, o);
        if (lane == 0) {
          atomicAdd(a.dbg + 0, 1ull);                       // slow-path entries
          atomicAdd(a.dbg + 1, cold ? 1ull : 0ull);         // ... of which cold
          atomicAdd(a.dbg + 2, (unsigned long long)nh);     // hits (values >= thr)
          atomicAdd(a.dbg + 3, (!cold && willc) ? 1ull : 0ull);   // warm compactions
          atomicAdd(a.dbg + 4, (unsigned long long)lanes_hit);
        }
      }
      unsigned long long ts0 = 0;
      if (DBG && (a.debug & 16)) ts0 = __builtin_amdgcn_s_memtime();
      // (the instrumented build of the split-k kernel keeps the row loop: with the rounds it spills a VGPR — profiles/r08_scan_variants.txt)
      list.template offer_tile<!(DBG && SPLITK)>(v, id0, rowof, a.kk, margin);
      if (DBG && (a.debug & 16) && lane == 0) {
        const unsigned long long dt = __builtin_amdgcn_s_memtime() - ts0;
        atomicAdd(a.dbg + (cold ? 4 : 5), dt);
        atomicAdd(a.dbg + (cold ? 6 : 7), 1ull);
      }
      refresh_thr();
    }
    if (((DBG && (a.debug & 8)) || SYMCNT) && lane == 0) atomicAdd(a.dbg + 5, 1ull);   // tiles
    if (__builtin_expect(a.share && (tt & 63) == 63, 0)) {
      sync_seed();
      if constexpr (SYM == 2 && MMF_SYM_COARSE != 0) sync_tmin();
      refresh_thr();
    }
  };

  // SYM == 2, the candidate direction: right behind a tile's chain (its stage of thresholds is not refilled before the next
  // barrier), the lane's 16 values against the thresholds of their candidate rows — 8 v_max + 8 compares, two LDS reads.
  // On a hit the wave's log gets hit records (MMF_SYM_RECORDS, below).  The entry path before them (MMF_SYM_RECORDS=0):
  // every passing value goes to the wave's log: position = the wave's running count + the lane's rank in the ballot;
  // a full log flags the candidate row for the exact rescan (audit_kernel).  Almost every hit is ONE value in ONE lane, so
  // the path costs one round: each lane folds its passing values (validity included) into a 16-bit mask, and a round takes
  // the lowest set bit of every lane that has one — one ballot and one store per round, as many rounds as the busiest lane
  // has values.
  // MMF_SYM_ABLATE (scripts/ab_build.sh, timing only, the results are WRONG): 1 = the test without the hit path, 2 = neither
  // the test nor the threshold DMA, 3 = the hit path without its log stores (the logs then read as empty; with records: the ballots and positions without the record stores).
  // MMF_SYM_COARSE (the default): the hot test is ONE compare.  A lane's 16 values belong to eight candidate rows, those of its row
  // group g in the tile's two candidate blocks; tmn is the smallest of their thresholds (the group minima: written with the image
  // by sym_thr_kernel, kept up by sync_seed, fetched with the thresholds by issue_thr_pair and read from LDS BEFORE the chain), mm the
  // largest of the 16 values (the two per-query maxima the query-side filter takes anyway).  mm < tmn: every value is below its row's
  // threshold.  Otherwise the wave enters the cold block, which is the test above, unchanged.  ABLATE 4 = the hot test alone.
  uint32_t sym_wcnt = 0, sym_cvis = 0, sym_htile = 0;   // records; wave-tiles that passed the group test; ... that had a hit
  auto sym_offer = [&](const Acc& x, int tt, const float* th, float tmn, float mm) {
    if constexpr (MMF_SYM_COARSE != 0) {
      if (__builtin_expect(!(SCALAR_ANY ? sym_hits(__builtin_amdgcn_ballot_w64(mm >= tmn)) : __any(mm >= tmn) != 0) ||
                           (MMF_SYM_ABLATE == 4 && a.sym_log_cap >= 0), 1)) return;
      ++sym_cvis;
      if (SYMCNT && lane == 0) atomicAdd(a.dbg + 6, 1ull);   // coarse visits
    }
    const f32x4 th0 = *reinterpret_cast<const f32x4*>(th + 4 * g);
    const f32x4 th1 = *reinterpret_cast<const f32x4*>(th + 16 + 4 * g);
    if constexpr (MMF_SYM_RECORDS != 0) {
      // Hit records: the wave does not need to know WHICH value passed — sym_scatter_kernel tests every value of a record against the
      // thresholds recorded with it (and against the rows' validity), where nobody waits at a barrier.  So the hit path is one ballot
      // per candidate block with a hit and, per lane with a hit, one 64-byte record: header (first of the lane's four candidate rows,
      // first of its two query rows, two reserved words), the block's four thresholds as tested, the lane's eight values of the block.
      // Position = the wave's running count + the lane's rank in the ballot, the second block's records behind the first's.
      bool any0 = false, any1 = false;
      unsigned long long hit0 = 0ull, hit1 = 0ull;     // the ballots of any0 / any1, kept as the compares' own SGPR pairs
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool p0 = fmaxf(x.t[0][0][j], x.t[0][1][j]) >= th0[j], p1 = fmaxf(x.t[1][0][j], x.t[1][1][j]) >= th1[j];
        any0 |= p0; any1 |= p1;
        if constexpr (SCALAR_ANY) { hit0 |= __builtin_amdgcn_ballot_w64(p0); hit1 |= __builtin_amdgcn_ballot_w64(p1); }
      }
      if (__builtin_expect((SCALAR_ANY ? sym_hits(hit0 | hit1) : __any(any0 || any1) != 0) && (MMF_SYM_ABLATE != 1 || a.sym_log_cap < 0), 0)) {
        const uint32_t cj0 = id_base + (uint32_t)tt * B_CT + ((tt >= sym_n1) ? (uint32_t)(sym_skip * B_CT) : 0u) + 4u * (uint32_t)g;
        const uint32_t qi0 = (uint32_t)(q0 + 32 * qw + c16);
        u32x4* lg = reinterpret_cast<u32x4*>(a.sym_log) + ((size_t)blockIdx.x * NW + wave) * (size_t)a.sym_log_cap * 4;
        ++sym_htile;
        if (SYMCNT && lane == 0) atomicAdd(a.dbg + 7, 1ull);   // wave-tiles with a hit
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const bool hit = cb ? any1 : any0;
          const unsigned long long b = SCALAR_ANY ? (cb ? hit1 : hit0) : __ballot(hit);
          if (hit) {
            const uint32_t at = sym_wcnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (at < (uint32_t)a.sym_log_cap) {
              if (MMF_SYM_ABLATE != 3) {
                u32x4 hd;
                hd[0] = cj0 + 16u * cb; hd[1] = qi0; hd[2] = 0u; hd[3] = 0u;
                u32x4* r = lg + (size_t)at * 4;
                r[0] = hd;
                r[1] = __builtin_bit_cast(u32x4, cb ? th1 : th0);
                r[2] = __builtin_bit_cast(u32x4, x.t[cb][0]);
                r[3] = __builtin_bit_cast(u32x4, x.t[cb][1]);
              }
            } else {
              // full log: the record is lost, and nobody knows which of its values passed — every real row among the block's four
              // candidate rows is flagged.  Over-flagging only sends rows to the exact rescan (audit_kernel), which is always right.
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const uint32_t cj = cj0 + 16u * cb + jj;
                if ((int64_t)cj < a.n_rows) atomicMax(a.lost + cj, 0x7fffffff);
              }
            }
          }
          sym_wcnt += (uint32_t)__popcll(b);
        }
      }
      return;
    }
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      any |= fmaxf(x.t[0][0][j], x.t[0][1][j]) >= th0[j];
      any |= fmaxf(x.t[1][0][j], x.t[1][1][j]) >= th1[j];
    }
    if (__builtin_expect(__any(any) && (MMF_SYM_ABLATE != 1 || a.sym_log_cap < 0), 0)) {
      const uint32_t cj0 = id_base + (uint32_t)tt * B_CT + ((tt >= sym_n1) ? (uint32_t)(sym_skip * B_CT) : 0u) + 4u * (uint32_t)g;
      const uint32_t qi0 = (uint32_t)(q0 + 32 * qw + c16);
      const bool sym_qv0 = q0 + 32 * qw + c16 < a.n_rows, sym_qv1 = q0 + 32 * qw + c16 + 16 < a.n_rows;
      uint32_t* lg = a.sym_log + ((size_t)blockIdx.x * NW + wave) * (size_t)a.sym_log_cap * 4;
      ++sym_htile;
      uint32_t m = 0;                                   // bit 8 cb + 2 j + qb: value x.t[cb][qb][j] passes and both rows are real
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float tj = cb ? th1[j] : th0[j];
          const bool cv = (int64_t)(cj0 + 16u * cb + j) < a.n_rows;
          m |= (x.t[cb][0][j] >= tj && sym_qv0 && cv) ? (1u << (8 * cb + 2 * j)) : 0u;
          m |= (x.t[cb][1][j] >= tj && sym_qv1 && cv) ? (2u << (8 * cb + 2 * j)) : 0u;
        }
      }
      unsigned long long busy = __ballot(m != 0u);
      while (busy) {
        if (m != 0u) {
          const uint32_t b = (uint32_t)__builtin_ctz(m);
          m &= m - 1u;
          // value number b = 8 cb + 2 j + qb out of the registers: a tree of selects, one level per bit of b (select16, mmf_dev.h)
          const float v = select16(b, x.t[0][0][0], x.t[0][1][0], x.t[0][0][1], x.t[0][1][1], x.t[0][0][2], x.t[0][1][2], x.t[0][0][3], x.t[0][1][3],
                                   x.t[1][0][0], x.t[1][1][0], x.t[1][0][1], x.t[1][1][1], x.t[1][0][2], x.t[1][1][2], x.t[1][0][3], x.t[1][1][3]);
          const uint32_t cj = cj0 + 16u * (b >> 3) + ((b >> 1) & 3u);
          const uint32_t at = sym_wcnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(busy >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)busy, 0u));
          if (at < (uint32_t)a.sym_log_cap) {
            u32x4 ent;
            ent[0] = cj; ent[1] = qi0 + 16u * (b & 1u); ent[2] = __float_as_uint(v); ent[3] = 0u;
            if (MMF_SYM_ABLATE != 3) *reinterpret_cast<u32x4*>(lg + (size_t)at * 4) = ent;
          } else {
            atomicMax(a.lost + cj, 0x7fffffff);
          }
        }
        sym_wcnt += (uint32_t)__popcll(busy);
        busy = __ballot(m != 0u);
      }
    }
  };

  // Main loop: TPB tiles per barrier.  Iteration j reads the group of stages holding tiles j*TPB ..
  // and fills the other group with the next TPB tiles (DMA pieces issued inside the MFMA chains), so at
  // the top of an iteration everything this wave has in flight is exactly what the iteration needs:
  // vmcnt(0), barrier.  Past the end of the range the DMA re-fetches tile 0 into a stage nobody reads.
  unsigned long long tw = 0, tf = 0, tc = 0, tv = 0, t0s = 0, t1s = 0, t2s = 0, t3s = 0, tvs = 0;
  const bool stamps = DBG && (a.debug & 16) != 0;
  Acc acc_prev;
  float m0_prev = kNegInf, m1_prev = kNegInf;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc_prev.t[cb][0][j] = kNegInf; acc_prev.t[cb][1][j] = kNegInf; }   // "tile -1"
  }
  const int nIter = (Ti + TPB - 1) / TPB;
  for (int j = 0; j < nIter; ++j) {
    if (stamps) tvs = __builtin_amdgcn_s_memtime();
    if constexpr (SYM == 2 && MMF_SYM_CHAIN_WAIT != 0) {
      // ... with lgkmcnt(0) in the same instruction.  On the hot path nothing of that counter is outstanding here, but the compiler
      // carries the cold blocks' possibly outstanding scalar loads and LDS operations across the back edge and then opens the first
      // chain with lgkmcnt(0) behind all six of its leading reads; told here that the counter is empty, it counts (lgkmcnt(5))
      __builtin_amdgcn_s_waitcnt(0x0070);
    } else
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) alone (expcnt 7, lgkmcnt 15 = no wait)
    if (stamps) t0s = __builtin_amdgcn_s_memtime();
    asm volatile("" ::: "memory");
    if (!(DBG && (a.debug & 4)))    // timing-only ablation: no workgroup barrier (races)
    __builtin_amdgcn_s_barrier();   // this group is visible to all; everyone is done READING the other group
    asm volatile("" ::: "memory");
    if (stamps) t1s = __builtin_amdgcn_s_memtime();

    if constexpr (SPLITK) {
      if (owner) {
        if (j > 0) {                 // the partner's half of tile j - 1, written before the barrier just passed
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x4 p = xch[(qw * 4 + i) * 64 + lane];
            acc_prev.t[i >> 1][i & 1] += p;
          }
          m0_prev = max_qb(acc_prev, 0);
          m1_prev = max_qb(acc_prev, 1);
        }
        // the reads of the exchange block above must be ISSUED before the acknowledgement below (LDS operations of a wave
        // complete in order, so issue order is all it takes): keep the compiler from sinking them past the volatile store
        asm volatile("" ::: "memory");
        if (lane == 0) ack[qw] = j;  // the exchange block may be overwritten
      }
    }
    if (owner) filter(acc_prev, j * TPB - 1, m0_prev, m1_prev);  // behind the barrier: only this wave waits for its own list code
    if (stamps) t2s = __builtin_amdgcn_s_memtime();

    const int sg = (j & 1) * TPB, ng = TPB - sg;      // stage group read / filled by this iteration
#pragma unroll
    for (int u = 0; u < TPB; ++u) {
      const int t = j * TPB + u;
      const bool more = (t + TPB < Ti);
      const char* src = more ? tsrc + u * (int64_t)TILEB : zc0;
      // the 32 biases of tile t + TPB go out BEFORE this tile's chain: issued behind it, the wave whose turn it is would
      // reach the vmcnt(0) of the next iteration with a DMA just issued, and seven waves would wait for it at the barrier
      Acc acc;
      // SYM == 2: the tile's group minimum of this lane's row group, read in front of the chain (it landed before the barrier), so that
      // no LDS wait sits behind it
      constexpr bool COARSE = SYM == 2 && MMF_SYM_COARSE != 0 && MMF_SYM_ABLATE != 2;
      float tmn = 0.f, m0 = 0.f, m1 = 0.f;
      if constexpr (COARSE) {
        tmn = sym_min_stage(sg + u)[g];
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      acc = tile_body(tiles + (sg + u) * TILEB + kbyte, cbs + (sg + u) * 64, src, ng + u);
      // (behind the chain: issued in front of it, the same DMA costs +8 %; mid-chain needs a branch inside the chain)
      if constexpr (SYM == 0) { if (wave == ((t + TPB) & (NW - 1))) issue_bias(more ? bsrc + u * B_CT * 4 : cb0, ng + u); }
      else mask_padding(acc, t);
      if constexpr (XSEG) mask_excluded(acc, t);
      if constexpr (SYM == 2 && MMF_SYM_ABLATE != 2) {
        // the next group's thresholds: between the iteration's two chains, far from either barrier (issued behind the LAST chain, a
        // fetch that has not landed holds all eight waves at the next barrier); the issuing wave rotates with the iteration
        if constexpr (MMF_SYM_EARLY_THR) { if (u == 0 && wave == (j & (NW - 1))) issue_thr_pair(more ? bsrc : cb0, ng); }
        else if (wave == ((t + TPB + 4) & (NW - 1))) issue_thr(more ? bsrc + u * B_CT * 4 : cb0, ng + u);
        // (the two per-query maxima serve the group test here and the query-side filter below)
        if constexpr (COARSE) { m0 = max_qb(acc, 0); m1 = max_qb(acc, 1); }
        if (t < Ti) sym_offer(acc, t, sym_thr_stage(sg + u), tmn, fmaxf(m0, m1));
      }
      if (u < TPB - 1) {
        if (TPB == 2 || __builtin_expect(t < Ti, 1))      // (TPB > 2: the ragged last group can hold several dummy tiles)
        filter(acc, t, COARSE ? m0 : max_qb(acc, 0), COARSE ? m1 : max_qb(acc, 1));   // mid-iteration, no barrier nearby
      } else {
        if (__builtin_expect(t >= Ti, 0)) {              // ragged range: the last tile of the last group is a dummy
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) { acc.t[cb][0][jj] = kNegInf; acc.t[cb][1][jj] = kNegInf; }
          }
          m0 = kNegInf; m1 = kNegInf;
        }
        acc_prev = acc;
        if constexpr (COARSE) {
          m0_prev = m0; m1_prev = m1;
        } else if constexpr (!SPLITK) {
          m0_prev = max_qb(acc, 0);     // reduced BEFORE the barrier, in time this wave would otherwise spend waiting
          m1_prev = max_qb(acc, 1);
        } else if (!owner) {
          // hand this tile's partial sums to the lower-half wave once it has taken the previous tile's
          while (ack[qw] < j) __builtin_amdgcn_s_sleep(1);
          asm volatile("" ::: "memory");        // ... and the writes of the next partials stay behind the poll
#pragma unroll
          for (int i = 0; i < 4; ++i) xch[(qw * 4 + i) * 64 + lane] = acc.t[i >> 1][i & 1];
          __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the partials are in LDS before this wave reaches the barrier
        }
      }
    }
    tsrc += TPB * (int64_t)TILEB;
    bsrc += TPB * B_CT * 4;
    if constexpr (SYM != 0) {   // the next group to fetch (tiles (j + 2) TPB ..) is the first of the second range: jump there
      if ((j + 2) * TPB == sym_n1) { tsrc += sym_skip * (int64_t)TILEB; bsrc += sym_skip * (B_CT * 4); }
    }
    if (stamps) {
      asm volatile("" :: "v"(acc_prev.t[0][0][0]));  // the chain's result must exist before the stamp
      t3s = __builtin_amdgcn_s_memtime();
      tw += t1s - t0s; tf += t2s - t1s; tc += t3s - t2s; tv += t0s - tvs;
    }
  }
  if (stamps && lane == 0) {
    atomicAdd(a.dbg + 0, tw); atomicAdd(a.dbg + 1, tf); atomicAdd(a.dbg + 2, tc); atomicAdd(a.dbg + 3, (unsigned long long)Ti);
    atomicAdd(a.dbg + 8, tv);
  }
  if constexpr (SPLITK) {               // the last tile's upper half
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_s_barrier();
    if (owner && Ti > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc_prev.t[i >> 1][i & 1] += xch[(qw * 4 + i) * 64 + lane];
    }
  }
  if (Ti > 0 && owner) filter(acc_prev, nIter * TPB - 1, max_qb(acc_prev, 0), max_qb(acc_prev, 1));
  __builtin_amdgcn_s_waitcnt(0x0F70);   // the dummy tiles still in flight

  list.compact(a.kk, margin);
  list.sink.close();                    // reserved overflow-list slots this lane did not use
  if (a.spill_stacks && a.spill_cnt) {  // two-stack overflow lists: both counts in one word; stacks that met cost the row its fast path
    const uint32_t mine = qvalid ? list.sink.cpos : 0u;
    const uint32_t theirs = (uint32_t)__shfl_xor((int)mine, 32);
    if (mine + theirs > (uint32_t)a.spill_cap) list.lost = kFltMax;
    if (qvalid && half == 0 && (mine | theirs)) a.spill_cnt[qpos] = mine | (theirs << 16);
  }
  sync_seed();
  if constexpr (SYM == 2) {
    if constexpr (MMF_SYM_COARSE != 0) sync_tmin();
    if (MMF_SYM_ABLATE == 3) sym_wcnt = 0;   // nothing was stored: nothing for sym_scatter_kernel to read
    if (lane == 0) {
      uint32_t* lc = a.sym_log_cnt + (size_t)blockIdx.x * NW + wave;
      lc[0] = sym_wcnt < (uint32_t)a.sym_log_cap ? sym_wcnt : (uint32_t)a.sym_log_cap;
      lc[(size_t)gridDim.x * NW] = sym_cvis; lc[2 * (size_t)gridDim.x * NW] = sym_htile;   // MMF_SYMMETRIC_DEBUG's "coarse visits" and "hit wave-tiles"
    }
  }
  if (qvalid) {
    const int64_t lbase = qpos * a.lists_total + a.list_base + 2 * split + half;
    a.cand_cnt[lbase] = (uint32_t)list.cnt;
    for (int e = 0; e < list.cnt; ++e) {
      uint32_t id = list.id_of(e);
      if (a.seg_len) id = (id / a.seg_len) * a.seg_stride + id % a.seg_len;
      a.cand_ids[lbase * CAP + e] = id + id_off;
      if (a.cand_keys) a.cand_keys[lbase * CAP + e] = list.keys[e * NTL];
    }
    // Audited loss, settled after the last launch: a dropped candidate matters only if its key reaches the
    // best threshold ANY list of the row has proven by then.
    if (a.cand_keys && half == 0) a.margin_out[qpos] = margin;
    if (list.lost > kNegInf) atomicMax(a.lost + qpos, seed_enc(list.lost) + SlotList<CAP, NTL>::SLOTS);   // stored keys carry slot bits
  }
  // (behind the last read of the id slots: the workgroup's own scratch, one word per list thread)
  if (SYM != 0 && (MMF_SYM_ABLATE_Q & SYM) != 0 && (MMF_SYM_ABLATE_Q & 4) != 0) lids[tid & (NTL - 1)] = __float_as_uint(ablate_keep);
}

// overflow[row] |= (a key was dropped for the row) && (no list proved a threshold above it)
__global__ void audit_kernel(const int32_t* seed, const int32_t* lost, uint32_t* overflow, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t l = lost[i];
  if (l > kSeedNone && l >= seed[i]) overflow[i] = 1u;
}

// The ceilings of the CEIL kernels.  Row i has emitted everything down to its floor, the canonical key fk_i; a
// column that ranks after the floor has a key <= fk_i, so its real-number target Q is at most map_i(fk_i) + E2_i and its scanned
// value at most map_i(fk_i) + E1_i + E2_i.  map_i turns a canonical key into Q units (Q = bias_j + u_i . u_j, operands scaled by s):
//   dot, cosine: s^2 key;   -|x - y|^2: s^2 (key + n_i) / 2;   rbf (key = -lambda |x - y|^2): s^2 (key / lambda + n_i) / 2.
// E1 + E2 is half the scan's margin; `slack` covers the f32 rounding of the map itself and of the rbf key's product with lambda
// (a few 2^-24 of the terms; 2^-21 of their magnitudes is taken).  The sum is rounded up by one more ulp.
struct CeilArgs {
  const float* floor_key; const float* rx;   // [n] the rows' floors and canonical row scalars
  const float *q_zn, *q_rn, *q_un; const uint32_t* maxima; const uint32_t* max_n;
  int64_t n, n_pad; int metric, d, dp, cap; float lambda;
  float* ceil;                               // [n_pad]
  // GATHER (the segmented passes): i is a position of the segment-padded query image, n the positions in use and
  // gather [n] the row of X at each (-1: padding inside a segment's last block, ceiling +inf); floor_key and rx are read through it,
  // the norms by position
  const int32_t* gather;
};
template <bool GATHER>
__global__ void ceil_kernel(CeilArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_pad) return;
  if (i >= a.n) { a.ceil[i] = __builtin_huge_valf(); return; }
  int64_t row = i;
  if constexpr (GATHER) {
    row = a.gather[i];
    if (row < 0) { a.ceil[i] = __builtin_huge_valf(); return; }
  }
  const float s = prep_scale(a.metric, a.max_n), s2 = s * s;
  const float fk = a.floor_key[row];
  float q, mag;
  if (a.metric == MMF_DOT || a.metric == MMF_COSINE) { q = s2 * fk; mag = fabsf(q); }
  else {
    const float t = (a.metric == MMF_RBF) ? fk / a.lambda : fk, ni = a.rx[row];
    q = 0.5f * s2 * (t + ni); mag = 0.5f * s2 * (fabsf(t) + ni);
  }
  const float half_margin = 0.5f * scan_margin(a.metric, a.d, a.dp, a.cap, a.q_zn[i], a.q_rn[i], a.q_un[i], a.maxima);
  const float c = q + half_margin + 4.7683716e-7f * mag;
  a.ceil[i] = (c == c) ? nextafterf(c, __builtin_huge_valf()) : __builtin_huge_valf();
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int pad_dp(int64_t d) {
  if (d <= 128) return 128;
  if (d <= 256) return 256;
  if (d <= 512) return 512;
  if (d <= 1024) return 1024;
  return 0;
}
static int waves_for_dp(int dp) { return dp <= 512 ? 8 : 4; }   // waves that own queries (d <= 1024: four split-k pairs)

int scan_bf16_supported(int64_t d, int kk, int dtype) {
  (void)dtype;
  const int dp = pad_dp(d);
  if (dp == 0) return 0;
  if (kk <= 20) return 1;                          // two 16-entry lists per query keep 14 each after a compaction
  return (kk <= 44 && dp <= 512) ? 1 : 0;          // two 32-entry lists (their 64 KiB do not fit beside 64 KiB tiles: d <= 512)
}

// d <= 1024 keeps the 15-entry lists up to k + self = 20: the split-k pair kernel has no LDS for 16-entry lists beside its
// exchange block, and the one-wave-per-SIMD kernel that had (380-395 VGPRs, 7-17 of them spilled) is retired.  Two 15-entry
// lists hold 13 each after a compaction: enough for the k-th best of their union; the surplus goes to the overflow list.
int scan_bf16_cap(int kk, int dp) {
  if (dp > 512) return B_CAP;
  return kk <= B_CAP - 4 ? B_CAP : (kk <= 20 ? B_CAP_BIG : B_CAP_WIDE);
}
int scan_bf16_slot_ulp(int cap) { return cap <= 16 ? 16 : 32; }
int scan_bf16_dp(int64_t d) { return pad_dp(d); }

int launch_prep_half(const PrepRows& r, const HalfImage& out, int dp, bool f16, hipStream_t s) {
  return launch_prep_half_gather(r, nullptr, r.n, out, dp, f16, s);
}

int launch_prep_half_gather(const PrepRows& r, const int32_t* gather, int64_t n_pos, const HalfImage& out, int dp, bool f16, hipStream_t s) {
  PrepArgs a{r.X, n_pos, r.d, r.dtype, r.metric, r.scal, r.max_n, out.Z, out.n_pad, dp, f16 ? 1 : 0, out.zn, out.rn, out.un, out.cb,
             out.maxima, gather};
  int64_t grid = (out.n_pad + 3) / 4;
  if (grid > 1024) grid = 1024;          // 16 waves per CU; fewer, longer workgroups keep the final atomics few
  hipLaunchKernelGGL(prep_half_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

static size_t scan_b16_lds(int ks, int nw, int tpb, int cap, bool splitk) {
  const int nqw = splitk ? nw / 2 : nw;
  return (size_t)(2 * tpb) * (B_CT * ks * 32) + (size_t)(2 * tpb) * 64 * 4 + (size_t)cap * (64 * nqw) * 4 +
         (splitk ? (size_t)nqw * 4 * 64 * 16 + 64 : 0);
}

int scan_b16_queries_per_block(int dp) { return 32 * waves_for_dp(dp); }

// splits of a row block that run side by side; the remaining col_splits / conc follow in later rounds
static int conc_splits_for(int64_t row_blocks, int col_splits) {
  int cs = 1;
  while (cs < 8 && cs < col_splits && row_blocks * cs < 256) cs <<= 1;
  return cs;
}
static int64_t scan_b16_round_blocks(int64_t row_blocks, int cs) {
  const int per = 8 / cs;                                 // row blocks per group of 8 block ids
  return ((row_blocks + per - 1) / per) * 8;
}
static int64_t scan_b16_grid(int64_t n_rows, int col_splits, int dp) {
  const int qt = scan_b16_queries_per_block(dp);
  const int64_t row_blocks = (n_rows + qt - 1) / qt;
  const int cs = conc_splits_for(row_blocks, col_splits);
  return scan_b16_round_blocks(row_blocks, cs) * (col_splits / cs);
}

// bytes of the global id-slot scratch ([grid][slots][list threads] u32) a launch needs
size_t scan_b16_scratch_bytes(int64_t n_rows, int col_splits, int dp, int cap) {
  return (size_t)scan_b16_grid(n_rows, col_splits, dp) * (cap <= 16 ? 16 : 32) * (64 * waves_for_dp(dp)) * 4 + 256;
}

// SEG and SYM kernels have no instrumented build
template <int KS, int NW, int TPB, int CAP, bool SPLITK = false, bool SEG = false, int SYM = 0, bool XSEG = false, bool CEIL = false>
static int launch_b16_t(const ScanB16Args& a, bool f16, int64_t grid, hipStream_t s) {
  const size_t lds = scan_b16_lds(KS, NW, TPB, CAP, SPLITK);
  auto go = [&](auto kern) -> int {
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * NW), lds, s, a);
    MMF_LAUNCH_CHECK();
    return MMF_OK;
  };
  if constexpr (SEG || SYM != 0 || CEIL) {
    if (f16) return go(scan_b16x_kernel<KS, true, false, NW, TPB, CAP, SPLITK, SEG, SYM, XSEG, CEIL>);
    return go(scan_b16x_kernel<KS, false, false, NW, TPB, CAP, SPLITK, SEG, SYM, XSEG, CEIL>);
  }
  if (a.debug != 0) {   // instrumented build of the same kernel (MMF_SCAN_DEBUG)
    if (f16) return go(scan_b16x_kernel<KS, true, true, NW, TPB, CAP, SPLITK>);
    return go(scan_b16x_kernel<KS, false, true, NW, TPB, CAP, SPLITK>);
  }
  if (f16) return go(scan_b16x_kernel<KS, true, false, NW, TPB, CAP, SPLITK>);
  return go(scan_b16x_kernel<KS, false, false, NW, TPB, CAP, SPLITK>);
}

// (padded dim, list capacity) -> <KS, NW, TPB, CAP, SPLITK>, for the plain launch, (SEG) the table-driven one and (XSEG) the
// table-driven one with the cross-segment mask; (CEIL) the plain launch with per-row ceilings
template <bool SEG, bool XSEG = false, bool CEIL = false>
static int launch_b16_for(const char* who, int dp, int cap, const ScanB16Args& a, bool f16, int64_t grid, hipStream_t s) {
  const bool big = (cap == B_CAP_BIG);   // k + self in 12..20: 16-entry lists, one tile per barrier
  if (cap == B_CAP_WIDE) {               // k + self in 21..44: 32-entry lists, one tile per barrier, d <= 512
    switch (dp) {
      case 128: return launch_b16_t<8, 8, 1, B_CAP_WIDE, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
      case 256: return launch_b16_t<16, 8, 1, B_CAP_WIDE, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
      case 512: return launch_b16_t<32, 8, 1, B_CAP_WIDE, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
    }
    set_error("%s: 32-entry lists need a padded dim <= 512 (got %d)", who, dp);
    return MMF_E_INTERNAL;
  }
  switch (dp) {
    // d <= 256: the smaller tiles leave room for eight stages — four tiles per barrier (-1.5 % against two at d = 256)
    case 128: return big ? launch_b16_t<8, 8, 2, B_CAP_BIG, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s) : launch_b16_t<8, 8, 4, B_CAP, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
    case 256: return big ? launch_b16_t<16, 8, 2, B_CAP_BIG, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s) : launch_b16_t<16, 8, 4, B_CAP, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
    case 512: return big ? launch_b16_t<32, 8, 1, B_CAP_BIG, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s) : launch_b16_t<32, 8, 2, B_CAP, false, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
    case 1024: return launch_b16_t<64, 8, 1, B_CAP, true, SEG, 0, XSEG, CEIL>(a, f16, grid, s);
  }
  set_error("%s: unsupported padded dim %d", who, dp);
  return MMF_E_INTERNAL;
}

int launch_scan_b16_ceilings(const ScanB16Problem& p, int cap, const float* floor_key, const float* rx, const uint32_t* max_n, float lambda,
                             int64_t n_pad, float* ceil, hipStream_t s) {
  CeilArgs a{floor_key, rx, p.q_zn, p.q_rn, p.q_un, p.maxima, max_n, p.n_rows, n_pad, p.metric, (int)p.d, p.dp, cap, lambda, ceil, nullptr};
  hipLaunchKernelGGL(ceil_kernel<false>, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// The same for a segment-padded query image (mmf_simtopk_segmented_fast_anyk): ceil [nq_pad] by operand position,
// gather [n_pos] the row of X at each position (-1: padding); floor_key and rx stay indexed by row of X.  The margin's maxima are
// those of the whole padded candidate image (p.maxima), as in the scan that follows.
int launch_scan_b16_ceilings_gather(const ScanB16Problem& p, int cap, const int32_t* gather, int64_t n_pos, const float* floor_key, const float* rx,
                                    const uint32_t* max_n, float lambda, int64_t nq_pad, float* ceil, hipStream_t s) {
  if (!gather) { set_error("scan_b16_ceilings_gather: position table missing"); return MMF_E_INTERNAL; }
  if (nq_pad <= 0) return MMF_OK;
  CeilArgs a{floor_key, rx, p.q_zn, p.q_rn, p.q_un, p.maxima, max_n, n_pos, nq_pad, p.metric, (int)p.d, p.dp, cap, lambda, ceil, gather};
  hipLaunchKernelGGL(ceil_kernel<true>, dim3((unsigned)((nq_pad + 255) / 256)), dim3(256), 0, s, a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// Settles the audited losses of all scan launches of a problem (call once, after the last one).
int launch_scan_b16_audit(const ScanB16Panel& pn, uint32_t* overflow, int64_t n_rows, hipStream_t s) {
  hipLaunchKernelGGL(audit_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, pn.seed, pn.seed + pn.seed_stride,
                     overflow, n_rows);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// What every launch shares: operands, shape, lists and threshold buffers.  One column range, the first list slots, no threshold
// sharing, no work table; each launcher sets what is its own.
static ScanB16Args scan_args(const ScanB16Problem& p, const CandLists& L, const ScanB16Panel& pn, void* scratch) {
  ScanB16Args a{};
  a.ZQ = p.ZQ; a.ZC = p.ZC; a.cb = p.cb; a.q_zn = p.q_zn; a.q_rn = p.q_rn; a.q_un = p.q_un; a.maxima = p.maxima;
  a.n_rows = p.n_rows; a.m = p.m; a.kk = p.kk; a.metric = p.metric; a.d = (int)p.d;
  a.col_splits = 1; a.conc_splits = 1;
  a.lists_total = L.lists;
  a.seed = pn.seed; a.lost = pn.seed + pn.seed_stride;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.overflow = L.overflow; a.cand_keys = L.keys; a.margin_out = L.margin;
  a.spill_cnt = L.spill_cnt; a.spill_ids = L.spill_ids; a.spill_cap = L.spill_cap; a.spill_stacks = L.spill_stacks;
  a.lids = reinterpret_cast<uint32_t*>(scratch);
  return a;
}

// col_splits must be a power of two.  Lists are indexed by query position.  ceil: nullptr, or the rows' ceilings (CEIL kernels).
static int scan_b16_plain(const ScanB16Problem& p, int col_splits, const CandLists& L, void* scratch, const ScanB16Panel& pn, const float* ceil,
                          hipStream_t s, int* grid_out) {
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.ceil = ceil;
  a.tiles_total = p.m_pad / B_CT;
  a.tiles_per_split = (a.tiles_total + col_splits - 1) / col_splits;
  if (a.tiles_per_split * (int64_t)B_CT * p.dp * 2 >= (int64_t(1) << 32)) {   // 32-bit scalar offsets of the tile DMA
    set_error("scan_b16: a column range of %lld tiles x %d exceeds 4 GiB of operands; use more col_splits",
              (long long)a.tiles_per_split, p.dp);
    return MMF_E_UNSUPPORTED;
  }
  a.row_blocks = (p.n_rows + scan_b16_queries_per_block(p.dp) - 1) / scan_b16_queries_per_block(p.dp);
  a.col_splits = col_splits;
  a.conc_splits = conc_splits_for(a.row_blocks, col_splits);
  a.blocks_per_round = scan_b16_round_blocks(a.row_blocks, a.conc_splits);
  a.list_base = pn.list_base; a.share = pn.share;
  a.seg_len = pn.seg_len; a.seg_stride = pn.seg_stride; a.id_off = pn.id_off;
  if (!pn.seed) { set_error("scan_b16: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (pn.list_base + 2 * col_splits > L.lists) { set_error("scan_b16: list slots out of range"); return MMF_E_INTERNAL; }
  if (!ceil) {   // (the CEIL kernels have no instrumented build)
    const char* dbg = getenv("MMF_SCAN_DEBUG");
    a.debug = dbg ? atoi(dbg) : 0;
    if (a.debug & (8 | 16)) {
      static unsigned long long* dbuf = nullptr;
      if (!dbuf) MMF_HIP(hipMalloc(&dbuf, 128));
      MMF_HIP(hipMemsetAsync(dbuf, 0, 128, s));
      a.dbg = dbuf;
    }
  }
  const int64_t grid = scan_b16_grid(p.n_rows, col_splits, p.dp);
  if (grid_out) *grid_out = (int)grid;
  const int rc = ceil ? launch_b16_for<false, false, true>("scan_b16_ceil", p.dp, L.cap, a, p.f16, grid, s)
                      : launch_b16_for<false>("scan_b16", p.dp, L.cap, a, p.f16, grid, s);
  if (rc == MMF_OK && (a.debug & 16)) {
    unsigned long long h[16];
    MMF_HIP(hipMemcpyAsync(h, a.dbg, 128, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    const double tiles = (double)h[3];
    fprintf(stderr, "[mmf scan stamps] per wave-tile cycles: dma-wait %.0f  barrier-wait %.0f  filter %.0f  chain(+DMA issue) %.0f  (sum %.0f)\n",
            h[8] / tiles, h[0] / tiles, h[1] / tiles, h[2] / tiles, (h[8] + h[0] + h[1] + h[2]) / tiles);
    fprintf(stderr, "[mmf scan stamps] list code: cold entries %llu x %.0f cycles, warm entries %llu x %.0f cycles\n",
            h[6], h[6] ? (double)h[4] / h[6] : 0.0, h[7], h[7] ? (double)h[5] / h[7] : 0.0);
  }
  if (rc == MMF_OK && (a.debug & 8)) {
    unsigned long long h[8];
    MMF_HIP(hipMemcpyAsync(h, a.dbg, 64, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    fprintf(stderr, "[mmf scan dbg] wave-tiles=%llu slow-entries=%llu (cold %llu) hits=%llu warm-compactions=%llu lanes-with-hit=%llu\n",
            h[5], h[0], h[1], h[2], h[3], h[4]);
  }
  return rc;
}

int launch_scan_b16(const ScanB16Problem& p, int col_splits, const CandLists& L, void* scratch, const ScanB16Panel& pn, hipStream_t s,
                    int* grid_out) {
  return scan_b16_plain(p, col_splits, L, scratch, pn, nullptr, s, grid_out);
}
// The same launch with a ceiling per query row (mmf_simtopk_fast_anyk): ceil [n_pad] in the kernel's units.
int launch_scan_b16_ceil(const ScanB16Problem& p, int col_splits, const CandLists& L, void* scratch, const ScanB16Panel& pn, const float* ceil,
                         hipStream_t s, int* grid_out) {
  if (!ceil) { set_error("scan_b16_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  return scan_b16_plain(p, col_splits, L, scratch, pn, ceil, s, grid_out);
}

// Segmented scan (mmf_simtopk_segmented): one workgroup per entry of the work table `sched` ([grid][SEG_ENTRY] int32,
// device), one list pair per row (L.lists == 2), no threshold sharing.  The tables' tile ranges index the segment-padded
// candidate image; the query image is segment-padded too.  Same kernel as launch_scan_b16 with its schedule read from the
// table (template flag SEG: the production instantiations are untouched).
size_t scan_b16_seg_scratch_bytes(int64_t grid, int dp, int cap) {
  return (size_t)grid * (cap <= 16 ? 16 : 32) * (64 * waves_for_dp(dp)) * 4 + 256;
}

int launch_scan_b16_seg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const CandLists& L, void* scratch,
                        const ScanB16Panel& pn, hipStream_t s) {
  if (grid <= 0) return MMF_OK;
  if (L.lists != 2) { set_error("scan_b16_seg: one list pair per row expected"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16_seg: threshold buffers missing"); return MMF_E_INTERNAL; }
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.sched = sched;
  return launch_b16_for<true>("scan_b16_seg", p.dp, L.cap, a, p.f16, grid, s);
}

// The table-driven launch with a ceiling per operand position (the later passes of mmf_simtopk_segmented_fast_anyk).
// Such a pass runs at the full list depth only — 32-entry lists at d <= 512, the split-k pair kernel at d <= 1024 — so SEG + CEIL is
// instantiated for those four shapes and not for the whole table of launch_b16_for.
static int launch_b16_seg_ceil_for(int dp, int cap, const ScanB16Args& a, bool f16, int64_t grid, hipStream_t s) {
  if (cap == B_CAP_WIDE) {
    switch (dp) {
      case 128: return launch_b16_t<8, 8, 1, B_CAP_WIDE, false, true, 0, false, true>(a, f16, grid, s);
      case 256: return launch_b16_t<16, 8, 1, B_CAP_WIDE, false, true, 0, false, true>(a, f16, grid, s);
      case 512: return launch_b16_t<32, 8, 1, B_CAP_WIDE, false, true, 0, false, true>(a, f16, grid, s);
    }
  } else if (cap == B_CAP && dp == 1024) {
    return launch_b16_t<64, 8, 1, B_CAP, true, true, 0, false, true>(a, f16, grid, s);
  }
  set_error("scan_b16_seg_ceil: no kernel for padded dim %d with %d-entry lists (full-depth passes only)", dp, cap);
  return MMF_E_INTERNAL;
}

// ceil: [nq_pad] by position of the segment-padded query image (launch_scan_b16_ceilings_gather)
int launch_scan_b16_seg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const CandLists& L, void* scratch,
                             const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (grid <= 0) return MMF_OK;
  if (L.lists != 2) { set_error("scan_b16_seg_ceil: one list pair per row expected"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16_seg_ceil: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (!ceil) { set_error("scan_b16_seg_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.sched = sched; a.ceil = ceil;
  return launch_b16_seg_ceil_for(p.dp, L.cap, a, p.f16, grid, s);
}

// Cross-segment scan (mmf_simtopk_cross_segments_fast): one workgroup per entry of `sched` (cross_seg16_table,
// device copy), both operand images the plain ones (column = row of Y), `bounds` the [n_pad][2] excluded ranges of the query rows.
// L.lists = 2 x the largest entry count of a row block (every entry's XSEG_SLOT is below that count); pn.share: the entries of a
// block share thresholds.  Same kernel as launch_scan_b16_seg with the template flag XSEG: the other instantiations are untouched.
int launch_scan_b16_xseg(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, const CandLists& L,
                         void* scratch, const ScanB16Panel& pn, hipStream_t s) {
  if (grid <= 0) return MMF_OK;
  if (L.lists < 2 || (L.lists & 1) || !bounds || !sched) { set_error("scan_b16_xseg: list pairs, a work table and the rows' bounds expected"); return MMF_E_INTERNAL; }
  if (L.lists > 2 && (!L.keys || !L.margin)) { set_error("scan_b16_xseg: several list pairs need keys and margins"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16_xseg: threshold buffers missing"); return MMF_E_INTERNAL; }
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.sched = sched; a.xbounds = bounds; a.share = pn.share;
  return launch_b16_for<true, true>("scan_b16_xseg", p.dp, L.cap, a, p.f16, grid, s);
}

// The cross-segment launch with a ceiling per query row (the later passes of mmf_simtopk_cross_segments_fast_anyk).
// Both images are the plain ones, so a position is a row and `ceil` [n_pad] is what launch_scan_b16_ceilings leaves.  Such a pass
// runs at the full list depth only, so XSEG + CEIL is instantiated for the four shapes of launch_b16_seg_ceil_for.
static int launch_b16_xseg_ceil_for(int dp, int cap, const ScanB16Args& a, bool f16, int64_t grid, hipStream_t s) {
  if (cap == B_CAP_WIDE) {
    switch (dp) {
      case 128: return launch_b16_t<8, 8, 1, B_CAP_WIDE, false, true, 0, true, true>(a, f16, grid, s);
      case 256: return launch_b16_t<16, 8, 1, B_CAP_WIDE, false, true, 0, true, true>(a, f16, grid, s);
      case 512: return launch_b16_t<32, 8, 1, B_CAP_WIDE, false, true, 0, true, true>(a, f16, grid, s);
    }
  } else if (cap == B_CAP && dp == 1024) {
    return launch_b16_t<64, 8, 1, B_CAP, true, true, 0, true, true>(a, f16, grid, s);
  }
  set_error("scan_b16_xseg_ceil: no kernel for padded dim %d with %d-entry lists (full-depth passes only)", dp, cap);
  return MMF_E_INTERNAL;
}

int launch_scan_b16_xseg_ceil(const ScanB16Problem& p, const int32_t* sched, int64_t grid, const uint32_t* bounds, const CandLists& L,
                              void* scratch, const ScanB16Panel& pn, const float* ceil, hipStream_t s) {
  if (grid <= 0) return MMF_OK;
  if (L.lists < 2 || (L.lists & 1) || !bounds || !sched) { set_error("scan_b16_xseg_ceil: list pairs, a work table and the rows' bounds expected"); return MMF_E_INTERNAL; }
  if (L.lists > 2 && (!L.keys || !L.margin)) { set_error("scan_b16_xseg_ceil: several list pairs need keys and margins"); return MMF_E_INTERNAL; }
  if (!pn.seed) { set_error("scan_b16_xseg_ceil: threshold buffers missing"); return MMF_E_INTERNAL; }
  if (!ceil) { set_error("scan_b16_xseg_ceil: ceilings missing"); return MMF_E_INTERNAL; }
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.sched = sched; a.xbounds = bounds; a.share = pn.share; a.ceil = ceil;
  return launch_b16_xseg_ceil_for(p.dp, L.cap, a, p.f16, grid, s);
}

// ------------------------------------------------------------------------------------------------
// Symmetric scan of X against itself (cosine / dot, padded dim 512, 15-entry lists): DESIGN.md §4.1
// ------------------------------------------------------------------------------------------------
// Super-blocks of G row blocks (the last one takes the left-over row blocks too); ns of them.  Launch 0: every row block scans its own super-block and, when ns is even, the
// antipodal one (plain: query direction only).  Launch 1: the super-blocks a - (ns - 1) / 2 .. a - 1 (cyclic; `forward`:
// a + 1 .. a + (ns - 1) / 2), each pair of rows multiplied once and served in both directions.  Every ordered (row, column)
// pair is covered exactly once.  Looking BACK is what the live threshold image (sync_seed) wants: workgroups are dispatched in
// block-id order, so the rows a workgroup tests as candidates mostly belong to workgroups that run or have finished and have
// raised their thresholds; only the pairs of the wrap-around meet rows whose workgroup has not started.
// Block ids: like the plain launch, blocks that share blockIdx % 8 share an XCD; the G row blocks of a super-block take one
// XCD's block ids of one stretch of 8 G ids, so they run together and stream the same columns through that XCD's L2.
int sym_default_group(int64_t nb) {
  int64_t g = (nb + 31) / 32;                   // at most 32 super-blocks: launch 0 samples at least 1/16 of the columns
  return (int)(g < 32 ? 32 : g);                // at least one XCD's worth of workgroups (32 CUs)
}
// ns = nb / G super-blocks; the row blocks left over join the LAST one (G .. 2 G - 1 row blocks), so no super-block is
// short: a short one would give its rows thresholds from a handful of columns in launch 0 and flood their received lists.
static int64_t sym_super_blocks(int64_t nb, int G) { const int64_t ns = nb / G; return ns < 1 ? 1 : ns; }
// Two phases (`phases` == 2, looking back only; the default): the wrap-around pairs leave the cyclic look-back and run LAST.  Phase A,
// the block ids of the single-phase table: super-block b scans max(0, b - h) .. b - 1, so every candidate row belongs to a
// workgroup of an earlier or the same stretch of block ids.  Phase B, the block ids behind ALL of phase A: super-block b < h
// scans what it lost, b + ns - h .. ns - 1, whose rows have all at least started phase A — longest first (b ascending: h - b
// super-blocks), so the launch ends with its short workgroups.  A row block has an entry per phase, each with a list pair of
// its own (SYM_SLOT).  The grid has the stretches of phase B whatever table is built (they are idle in the other tables and
// in launch 0): one grid, one workspace layout and one block count for every switch.
// `antipodal` (ns even and at least 4, looking back only): launch 0 scans the own super-block alone, and the pair (a, a + ns / 2) is
// multiplied once, symmetric, by the later super-block a + ns / 2 as its LAST range (the second one, which lies below the first).
static int64_t sym_phase_a_grid(int64_t nb, int G) {
  const int64_t ns = sym_super_blocks(nb, G);
  return ((ns + 7) / 8 + (nb > ns * G ? 1 : 0)) * 8 * G;      // the left-over row blocks take a stretch of block ids of their own
}
int64_t sym_schedule_phase_b_begin(int64_t nb, int G) { return sym_phase_a_grid(nb, G); }
int64_t sym_schedule_grid(int64_t nb, int G) {
  const int64_t ns = sym_super_blocks(nb, G), h = (ns - 1) / 2;
  if (h == 0) return sym_phase_a_grid(nb, G);
  // (8 idle ids more when phase A's super-blocks fill its stretches to the last id: without them 64 row blocks in 8 super-blocks
  //  come to 128 ids per launch, 256 in all — the plain scan's block count at that size, and stats.scan_grid is how callers and
  //  tests tell which path ran)
  const int64_t pad = (ns % 8 == 0 && nb == ns * G) ? 8 : 0;
  return sym_phase_a_grid(nb, G) + (h + 7) / 8 * 8 * G + pad;
}
void sym_schedule_table(int64_t nb, int G, int launch, int32_t* out, bool forward, int phases, bool antipodal) {
  const int64_t ns = sym_super_blocks(nb, G), grid = sym_schedule_grid(nb, G), grid_a = sym_phase_a_grid(nb, G), tiles = nb * 8;
  const int64_t per = 8 * (int64_t)G, stretches = (ns + 7) / 8;
  const int64_t h = (ns - 1) / 2;
  if (forward) { phases = 1; antipodal = false; }   // the look-ahead arms keep the table they were measured with
  if (ns < 4 || (ns % 2) != 0) antipodal = false;   // (two super-blocks: launch 0 keeps all the pairs and the symmetric launch stays empty)
  auto first_tile = [&](int64_t sb) { return sb * G * 8; };
  auto end_tile = [&](int64_t sb) { return sb == ns - 1 ? tiles : (sb + 1) * G * 8; };
  for (int64_t b = 0; b < grid; ++b) {
    int32_t* e = out + b * SEG_ENTRY;
    for (int i = 0; i < SEG_ENTRY; ++i) e[i] = 0;
    e[SYM_RB] = -1;
    const bool phase_b = b >= grid_a;
    if (phase_b && (launch == 0 || phases != 2)) continue;
    const int64_t bb = phase_b ? b - grid_a : b;
    int64_t sb = (bb / per) * 8 + (bb % 8), rbi = sb * G + (bb % per) / 8;
    if (phase_b) {
      if (sb >= h) continue;
    } else if (bb / per >= stretches) {          // the extra stretch: left-over row blocks, on the XCD of the last super-block
      if (bb % 8 != (ns - 1) % 8) continue;
      sb = ns - 1; rbi = ns * G + (bb % per) / 8;
    } else if (sb >= ns) continue;
    if (rbi >= nb) continue;
    int64_t b1 = 0, n1 = 0, b2 = 0, n2 = 0;
    if (launch == 0) {
      b1 = first_tile(sb); n1 = end_tile(sb) - b1;
      if (ns >= 2 && (ns % 2) == 0 && !antipodal) { const int64_t o = (sb + ns / 2) % ns; b2 = first_tile(o); n2 = end_tile(o) - b2; }
    } else if (phase_b) {
      b1 = first_tile(sb + ns - h); n1 = tiles - b1;
    } else {
      const bool anti = antipodal && sb >= ns / 2;   // (its look-back sb - h .. sb - 1 starts behind the antipodal super-block: no wrap)
      if (h == 0 && !anti) continue;
      if (h > 0) {
        int64_t lo = forward ? sb + 1 : sb - h, hi = lo + h - 1;   // super-blocks lo .. hi, cyclic
        if (phases == 2) { if (lo < 0) lo = 0; }                    // (hi = sb - 1; sb == 0: nothing)
        else {
          if (lo >= ns) { lo -= ns; hi -= ns; }
          if (lo < 0) { lo += ns; hi += ns; }
        }
        if (hi < lo) continue;
        if (hi < ns) { b1 = first_tile(lo); n1 = end_tile(hi) - b1; }
        else { b1 = first_tile(lo); n1 = end_tile(ns - 1) - b1; b2 = 0; n2 = end_tile(hi - ns); }
      }
      if (anti) {
        const int64_t o = sb - ns / 2;
        if (n1 == 0) { b1 = first_tile(o); n1 = end_tile(o) - b1; }
        else { b2 = first_tile(o); n2 = end_tile(o) - b2; }
      }
    }
    if (n2 == 0) b2 = b1 + n1;
    e[SYM_RB] = (int32_t)rbi; e[SYM_B1] = (int32_t)b1; e[SYM_N1] = (int32_t)n1; e[SYM_B2] = (int32_t)b2; e[SYM_N2] = (int32_t)n2;
    e[SYM_SLOT] = phase_b ? 1 : 0;
    e[SYM_PHASE] = launch == 0 || phases != 2 ? 0 : (phase_b ? 2 : 1);
  }
}

// thresholds of the candidate rows for the symmetric launch: seed[] (launch 0's proven thresholds) decoded once.  A real row
// without one accepts everything (and is counted: it does not happen once launch 0 has seen k + self columns of the row);
// padding rows accept nothing.  Behind the image, thr[n_pad + 4 t + g]: the group minima of tile t (32 rows) — the smallest
// threshold of rows 4 g .. 4 g + 3 and 16 + 4 g .. + 3 of the tile, the eight rows whose values a lane of row group g holds
// (scan_b16x_kernel, sym_offer).  Padding rows (+inf) never lower one; a real row without a threshold makes its group pass always.
// One workgroup of 256 threads per 256 rows (n_pad is a multiple of 256): eight tiles.
__global__ __launch_bounds__(256) void sym_thr_kernel(const int32_t* seed, float* thr, int64_t n, int64_t n_pad, uint32_t* none_cnt) {
  __shared__ float sv[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float v = __builtin_huge_valf();
  if (i < n) {
    const int32_t o = seed[i];
    if (o > kSeedNone) v = __int_as_float(o >= 0 ? o : (o ^ 0x7fffffff));
    else { v = -kFltMax; atomicAdd(none_cnt, 1u); }
  }
  if (i < n_pad) thr[i] = v;
  sv[threadIdx.x] = v;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 2);
  if (threadIdx.x < 32 && t * B_CT < n_pad) {
    const float* r = sv + (threadIdx.x >> 2) * B_CT + 4 * (threadIdx.x & 3);
    float m = __builtin_huge_valf();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) m = fminf(m, fminf(r[jj], r[16 + jj]));
    thr[n_pad + 4 * t + (threadIdx.x & 3)] = m;
  }
}

// files the waves' logs into the rows' lists: one workgroup per log.  An entry that finds its row's list full flags the row.
// An entry was logged against the threshold its row had at the time; by now seed[] holds every row's FINAL proven threshold (all scan
// launches have finished), and select's pruning threshold is never below it (DESIGN.md §4.1 "Pruned filing"): an entry that fails
// select's own test — enc(key) + slot_ulp >= threshold — against seed[] would be dropped there, so it is not filed (seed: nullptr =
// file everything, MMF_SYMMETRIC_PRUNE=0).
// The log holds hit records (scan_b16x_kernel, sym_offer): 16 words — candidate row of value 0, query row of query block 0, two reserved
// words; the four thresholds the wave tested against; the lane's 2 x 4 values [query block][candidate row].  Eight threads walk a
// record, one value each, and apply the per-value test the scan kernel left out: the value reaches its candidate row's recorded
// threshold, and both rows are real (records carry the padding rows of a ragged last row block and queries past n_rows).  What
// passes is an "entry"; val_cnt[log] counts them (MMF_SYMMETRIC_DEBUG's "logged entries").
// (MMF_SYM_RECORDS=0: the log holds the entries themselves, (candidate row, query row, key bits, 0), tested by the scan kernel.)
__global__ __launch_bounds__(256) void sym_scatter_kernel(const uint32_t* log, const uint32_t* log_cnt, int log_cap, uint32_t* sym_cnt,
                                                          uint2* sym_ent, int cap, int32_t* lost,
                                                          const int32_t* seed, int slot_ulp, int64_t n_rows, uint32_t* val_cnt) {
  const uint32_t c = log_cnt[blockIdx.x];
#if MMF_SYM_RECORDS
  __shared__ uint32_t passed_all;
  if (c == 0) { if (threadIdx.x == 0) val_cnt[blockIdx.x] = 0u; return; }
  if (threadIdx.x == 0) passed_all = 0u;
  __syncthreads();
  const uint32_t* lg = log + (size_t)blockIdx.x * log_cap * 16;
  uint32_t passed = 0;
  for (uint32_t e = threadIdx.x; e < 8u * c; e += 256) {
    const uint32_t* r = lg + (size_t)(e >> 3) * 16;
    const uint32_t vi = e & 7u, j = vi & 3u;                        // value vi = 4 qb + j of the record
    const uint32_t cj = r[0] + j, qi = r[1] + 16u * (vi >> 2), kb = r[8 + vi];
    if (!(__uint_as_float(kb) >= __uint_as_float(r[4 + j])) || (int64_t)qi >= n_rows || (int64_t)cj >= n_rows) continue;
    ++passed;
    if (seed) {
      const int32_t sd = seed[cj], b = (int32_t)kb;
      if (sd > kSeedNone && (b >= 0 ? b : (b ^ 0x7fffffff)) + slot_ulp < sd) continue;   // (no proven threshold: keep)
    }
    const uint32_t slot = atomicAdd(sym_cnt + cj, 1u);
    if (slot < (uint32_t)cap) {
      sym_ent[(size_t)cj * cap + slot] = make_uint2(qi, kb);           // (id, key bits): one 8-byte store
    } else {
      atomicMax(lost + cj, 0x7fffffff);
    }
  }
  if (passed) atomicAdd(&passed_all, passed);
  __syncthreads();
  if (threadIdx.x == 0) val_cnt[blockIdx.x] = passed_all;
#else
  if (threadIdx.x == 0) val_cnt[blockIdx.x] = c;
  const u32x4* lg = reinterpret_cast<const u32x4*>(log) + (size_t)blockIdx.x * log_cap;
  for (uint32_t e = threadIdx.x; e < c; e += 256) {
    const u32x4 v = lg[e];
    if (seed) {
      const int32_t sd = seed[v[0]], b = (int32_t)v[2];
      if (sd > kSeedNone && (b >= 0 ? b : (b ^ 0x7fffffff)) + slot_ulp < sd) continue;   // (no proven threshold: keep)
    }
    const uint32_t slot = atomicAdd(sym_cnt + v[0], 1u);
    if (slot < (uint32_t)cap) {
      sym_ent[(size_t)v[0] * cap + slot] = make_uint2(v[1], v[2]);      // (id, key bits): one 8-byte store
    } else {
      atomicMax(lost + v[0], 0x7fffffff);
    }
  }
#endif
}

// A wave log's capacity in the units the kernels count in: hit records (64 bytes), or — MMF_SYM_RECORDS=0 — entries (16 bytes, four to
// a record's room).  MMF_SYMMETRIC_LOG_CAP (read per call) only lowers it: a small test reaches the full-log path with it.
int scan_b16_sym_log_cap() {
  int cap = kSymLogPerWave * (MMF_SYM_RECORDS ? 1 : 4);
  if (const char* e = getenv("MMF_SYMMETRIC_LOG_CAP")) {
    const int v = atoi(e);
    if (v >= 1 && v < cap) cap = v;
  }
  return cap;
}

size_t scan_b16_sym_scratch_bytes(int64_t n_rows, int G) {
  const int64_t nb = (n_rows + 255) / 256;
  return (size_t)sym_schedule_grid(nb, G) * 16 * 512 * 4 + 256;
}

// Both launches, the threshold image between them and the filing of the logs behind them, on stream s.  p.ZC is the operand
// image of all rows (queries and candidates), n_pad / 32 tiles.  L has six lists per row (a pair for launch 0 and one per phase of
// the symmetric launch; a pair no entry writes keeps the count 0 it is given here), keys, margins
// and the sym_* lists; pn.seed as for launch_scan_b16.  y.live: the rows' workgroups keep raising the threshold image while the
// symmetric launch runs; y.forward: its schedule looks ahead (sym_schedule_table).  y.tables: build the two work tables and
// upload them to sb.sched — they depend on (row blocks, G, forward, phases, antipodal) alone, so a caller whose sb.sched still holds them from
// an earlier call on this stream passes false.  *grid_out: the sum of the two grids.
int launch_scan_b16_sym(const ScanB16Problem& p, const SymLaunch& y, const CandLists& L, void* scratch, const SymBuffers& sb,
                        const ScanB16Panel& pn, hipStream_t s, int* grid_out) {
  const int64_t n = p.n_rows, nb = (n + 255) / 256, n_pad = nb * 256, grid = sym_schedule_grid(nb, y.G);
  const int log_cap = scan_b16_sym_log_cap();
  // the SYM kernels neither fetch nor add the per-candidate bias: only metrics whose bias is zero for every real row may come here
  if (p.metric != MMF_DOT && p.metric != MMF_COSINE) {
    set_error("scan_b16_sym: metric %d has a per-candidate bias, which the symmetric kernels do not apply", p.metric);
    return MMF_E_INTERNAL;
  }
  if (L.lists != 2 * kSymListPairs || L.cap != B_CAP || !L.keys || !L.margin || !L.sym_cnt || !pn.seed) { set_error("scan_b16_sym: lists missing"); return MMF_E_INTERNAL; }
  if (n_pad * 1024 >= (int64_t(1) << 32)) { set_error("scan_b16_sym: operand image beyond the 32-bit tile offsets"); return MMF_E_INTERNAL; }
  if (y.tables) {
    std::vector<int32_t> tab((size_t)grid * 2 * SEG_ENTRY);
    sym_schedule_table(nb, y.G, 0, tab.data(), y.forward, y.phases, y.antipodal);
    sym_schedule_table(nb, y.G, 1, tab.data() + (size_t)grid * SEG_ENTRY, y.forward, y.phases, y.antipodal);
    MMF_TRY(upload_table(s, sb.sched, tab.data(), tab.size() * 4));
  }
  MMF_HIP(hipMemsetAsync(L.sym_cnt, 0, (size_t)n * 4, s));
  MMF_HIP(hipMemsetAsync(L.cnt, 0, (size_t)n * L.lists * 4, s));   // with one or two super-blocks the second launch has no work and writes no list
  MMF_HIP(hipMemsetAsync(sb.log_cnt, 0, (size_t)3 * grid * 8 * 4, s));   // records, coarse visits, hit wave-tiles
  MMF_HIP(hipMemsetAsync(sb.none_cnt, 0, 16, s));
  ScanB16Args a = scan_args(p, L, pn, scratch);
  a.ZQ = p.ZC;                                          // one image: the rows are queries and candidates
  a.tiles_total = n_pad / B_CT; a.row_blocks = nb;
  a.spill_stacks = 0;
  a.sched = sb.sched;
  a.sym_thr = sb.thr; a.sym_live = y.live ? 1 : 0; a.sym_log = sb.log; a.sym_log_cnt = sb.log_cnt; a.sym_log_cap = log_cap;
#if MMF_SYM_COUNT
  static unsigned long long* dbuf = nullptr;
  if (!dbuf) MMF_HIP(hipMalloc(&dbuf, 128));
  a.dbg = dbuf;
  auto report = [&](int launch) -> int {
    unsigned long long h[16];
    MMF_HIP(hipMemcpyAsync(h, dbuf, 128, hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    fprintf(stderr, "[mmf sym count] launch %d: wave-tiles=%llu visits=%llu (cold %llu) hits=%llu entry-compactions=%llu lanes-with-hit=%llu coarse-visits=%llu hit-wave-tiles=%llu\n",
            launch, h[5], h[0], h[1], h[2], h[3], h[4], h[6], h[7]);
    return MMF_OK;
  };
  MMF_HIP(hipMemsetAsync(dbuf, 0, 128, s));
#endif
  MMF_TRY((launch_b16_t<32, 8, 2, B_CAP, false, false, 1>(a, p.f16, grid, s)));
#if MMF_SYM_COUNT
  MMF_TRY(report(0));
  MMF_HIP(hipMemsetAsync(dbuf, 0, 128, s));
#endif
  hipLaunchKernelGGL(sym_thr_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, pn.seed, sb.thr, n, n_pad, sb.none_cnt);
  MMF_LAUNCH_CHECK();
  a.sched = sb.sched + (size_t)grid * SEG_ENTRY; a.list_base = 2; a.share = 1;
  MMF_TRY((launch_b16_t<32, 8, 2, B_CAP, false, false, 2>(a, p.f16, grid, s)));
#if MMF_SYM_COUNT
  MMF_TRY(report(1));
#endif
  hipLaunchKernelGGL(sym_scatter_kernel, dim3((unsigned)(grid * 8)), dim3(256), 0, s, sb.log, sb.log_cnt, log_cap, L.sym_cnt,
                     L.sym_ent, L.sym_cap, pn.seed + pn.seed_stride, y.prune ? pn.seed : nullptr, L.slot_ulp, n, sb.val_cnt);
  MMF_LAUNCH_CHECK();
  if (grid_out) *grid_out = (int)(2 * grid);
  return MMF_OK;
}

}  // namespace mmf
