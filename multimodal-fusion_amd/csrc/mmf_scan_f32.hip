// mmf_scan_f32.hip — exact all-pairs scan on v_mfma_f32_32x32x2_f32, any d, f32/bf16/f16 inputs.
//
// One kernel template, two epilogues:
//   MODE_SCAN  : fused similarity + per-row top-k candidates (the N x M matrix never leaves the CU)
//   MODE_DENSE : writes the [n,m] similarity for the small-N reference signatures
//
// The f32-input MFMA accumulates D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), i.e. exactly the k-ordered
// fmaf chain of include/mmf_hg.h (cdna_hip_programming.md §3 "FP32-input MFMA"), so the keys formed
// here ARE the canonical keys: lists are truncated by the final total order and cannot overflow.
//
// Tiling: workgroup = 4 waves = 128 queries x 128 candidates per macro tile, K staged through LDS in chunks of
// 16 (scan) / 32 (dense), double buffered, one barrier per chunk.  Wave w owns queries 32w..32w+31 as the MFMA
// column (B operand) and sweeps the 4 candidate sub-tiles as MFMA rows (A operand), so every lane keeps ONE query
// and its candidate list is lane-private (mmf_dev.h).
//
// Operands come from the f32 IMAGES of X and Y (mmf_prep.hip: f32, zero padded to 128 rows / 32 columns, and inside
// every group of eight k de-interleaved to k0 k2 k4 k6 | k1 k3 k5 k7).  A 16-byte unit of the image is what one lane
// half of the MFMA feeds to four consecutive k-steps, so
//   * staging is LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction, 4 or 8 per wave and chunk): no
//     staging registers, no ds_write, no per-chunk address arithmetic (a loop-invariant lane offset + a scalar k offset);
//   * the chain reads ONE ds_read_b128 per operand per four k-steps (5 per 16 MFMAs), the next group's while the
//     current one multiplies.  LDS rows are KC floats, 16-byte units XOR-swizzled by row so that the 16 lanes of a
//     b128 access group hit 16 distinct bank quads.
// Round 2 measured the pieces in a bare loop (scripts/probe/f32_loop.hip, 2 workgroups per CU, of 157.3 TFLOP/s):
// register loop 0.98, + ds_read_b32 operands 0.95, + barrier 0.95, + staging through registers and ds_write_b32 (the
// round-1 kernel) 0.76, 16-byte [row][k] units with a per-half v_cndmask select 0.81 (VALU between the MFMAs is what
// costs), de-interleaved image + LDS-DMA + b128 reads 0.91.
//
// Replaces: torch.mm + 3 elementwise passes, build_hypergraph/similarity_kernel.py:43-52, 79-84, 122;
//           sklearn brute-force kneighbors, build_hypergraph/preprocess_hypergraph.py:379-382.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int F_NT = 256;
constexpr int F_QT = 128;
constexpr int F_CT = 128;
// k per staged chunk (template parameter KC): 16 for the scan — 2 x (128 + 128) rows x 64 B = 32 KB beside 32 KB of
// lists, so two workgroups share a CU — and 32 for the dense outputs (no lists: two workgroups fit anyway, and half
// the barriers measure 7 % faster).

constexpr int MODE_SCAN = 0;
constexpr int MODE_DENSE = 1;

struct ScanF32Args {
  const float* Xp; const float* Yp;     // f32 images: row q of Xp is query position q of this launch
  int64_t n, m, dpad;
  const float* rx; const float* cy;
  const int32_t* row_ids; int64_t n_rows;
  float neg_lambda;
  int metric;
  int kk;
  int col_splits;
  int64_t tiles_per_split;
  uint32_t* cand_cnt; uint32_t* cand_ids; uint32_t* overflow;
  // k beyond one pass (k + self > 44): only columns that rank strictly AFTER (floor_key[q], floor_id[q]) in the total order
  // (key desc, id asc) are offered — the last entry the previous pass emitted for the row (NULL: no floor)
  const float* floor_key; const uint32_t* floor_id;
  // dense epilogue
  float* out;
  const float* P; int dp; float neg_lambda_g;
  int64_t prow0;   // dense combined, panel form: query q of this launch is row prow0 + q of P
  int debug;   // MMF_F32_DEBUG (timing-only ablations): 1 skip epilogue, 2 skip staging
  const int64_t* sched;   // SEG kernels only: [grid][SEGF_ENTRY] work table (launch_sim_dense_combined_seg)
  // COMB kernels only (the scan of K_h * K_g): P / dp / neg_lambda_g above are the CANDIDATES' positions; the queries' positions
  // (row q of Pq is query row q) and chain(p, p) of the query and candidate rows
  const float* Pq; const float* pnq; const float* pnc;
};

// Work table entry of the segmented dense combined similarity (one per workgroup): the segment, the image row of the row
// block's first query and how many of its F_QT queries are real, the segment's first row (candidate base for the image,
// the norms and P), the candidate tile range inside the segment, the output base kptr[s] and the row stride n_s.
enum { SEGF_SEG = 0, SEGF_ROW0 = 1, SEGF_NQ = 2, SEGF_CBASE = 3, SEGF_T0 = 4, SEGF_T1 = 5, SEGF_OUT = 6, SEGF_NS = 7, SEGF_ENTRY = 8 };

// SEG (segmented calls): the row block, tile range, candidate base, output base and row stride come from the
// work table a.sched instead of blockIdx / col_splits.  Tiles start at unaligned segment rows and read up to 127 rows past
// them (the next segment, or the image's unwritten last block): those rows only reach masked outputs.
//
// SEG with MODE_SCAN (mmf_simtopk_segmented_exact): the same table, with the segment's column count in SEGF_NS
// and the number of the workgroup's column range in SEGF_OUT.  q0 is a row of X and rx, the floors, the positions and the
// lists are addressed by it; a lane past the block's SEGF_NQ queries is a !qvalid lane (threshold +inf, nothing written).  The
// candidates are rows cbase + j of Y, j < SEGF_NS, and cbase + j is the id the lists, the floor test and the re-rank see: one
// id space, the rows of all of Y.  The range's list slot is row * 2 col_splits + 2 range + half, a.col_splits being the largest
// range count of any segment.
//
// COMB (MODE_SCAN only, mmf_simtopk_combined): the key is the exponent of K_h * K_g, eh + eg (mmf_dev.h: pos_exponent,
// combined_key).  A lane keeps its query's position (at most 8 floats, zero padded) and chain(p_i, p_i) in registers; the candidate
// tile's positions and their chains ride into LDS beside cys with the tile's first chunk, clamped at m - 1 as cy is.  In the
// epilogue the 32 lanes of a half read the same candidate's position (an LDS broadcast).  The chain, the DMA, the floor test and
// LaneList are those of the plain scan; the other instantiations are untouched.  COMB asks for two workgroups per CU at every
// capacity: that bounds the allocator at 256 registers (204 VGPRs, no AGPRs, nothing spilled); LDS decides how many run.
//
// XSEG (SEG with MODE_SCAN, no COMB; mmf_simtopk_cross_segments): the complement of the segmented scan.  The row
// block is still SEGF_ROW0 / SEGF_NQ of one segment, but the candidates are rows j of ALL of Y (base 0, j < a.m, tiles aligned to
// 128 rows as in the plain scan) and a key whose column lies in the block's excluded range [SEGF_CBASE, SEGF_NS) — the segment's
// own rows of Y, the two table words that would always be 0 and m here — becomes -inf where the m mask is applied, before the floor
// test and before LaneList sees the tile.  Both bounds are workgroup-uniform; a 32-column sub-tile that does not touch the range
// skips the test (wave-uniform branch).  Everything else is the SEG scan's code; the other instantiations are untouched.
template <int MODE, int CAP, int F_KC, bool SEG = false, bool COMB = false, bool XSEG = false>
__global__ __launch_bounds__(F_NT, (MODE == MODE_DENSE || CAP <= 16 || COMB) ? 2 : 1) void scan_f32_kernel(ScanF32Args a) {
  constexpr bool SSEG = SEG && MODE == MODE_SCAN;   // the table-driven scan epilogue (launch_scan_f32_seg)
  static_assert(!COMB || MODE == MODE_SCAN, "the combined key is a scan epilogue");
  static_assert(!XSEG || (SSEG && !COMB), "the cross flavour is the table-driven scan without the combined key");
  constexpr int UPR = F_KC / 4;            // 16-byte units per image row
  constexpr int RPP = 64 / UPR;            // image rows per 1 KiB DMA piece
  constexpr int HP = F_QT / RPP;           // pieces per operand tile (8 / 16)
  constexpr int PPW = 2 * HP / 4;          // pieces per wave: the first half of them query pieces, the rest candidate pieces
  constexpr int FSH = (UPR == 4) ? 2 : 1;  // unit u of row r sits at unit u ^ ((r >> FSH) & (UPR - 1))
  constexpr int NG = F_KC / 8;             // groups of eight k per chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = reinterpret_cast<float*>(smem);   // [2][F_QT][F_KC]
  float* Cs = Qs + 2 * F_QT * F_KC;             // [2][F_CT][F_KC]
  float* cys = Cs + 2 * F_CT * F_KC;            // [2][F_CT] per-candidate scalars of the tile being accumulated
  float* lkeys = cys + 2 * F_CT;                // [CAP][F_NT]
  uint32_t* lids = reinterpret_cast<uint32_t*>(lkeys + CAP * F_NT);
  float* pss = reinterpret_cast<float*>(lids + CAP * F_NT);   // COMB: [2][F_CT][8] candidate positions (zero beyond dp), as cys
  float* pns = pss + 2 * F_CT * 8;                            // COMB: [2][F_CT] their chains

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int c = lane & 31;

  int split = 0;
  int64_t q0, t_begin, t_end;
  int64_t m = a.m, qend = a.n_rows;        // columns of the output row; queries q < qend are real
  int64_t cbase = 0, obase = 0;            // SEG: the segment's first row, its block's first output element
  int ex_lo = 0, ex_len = 0;               // XSEG: first row and row count of the excluded columns (ids below 2^31)
  if constexpr (XSEG) {
    const int64_t* e = a.sched + (size_t)blockIdx.x * SEGF_ENTRY;
    q0 = e[SEGF_ROW0]; qend = q0 + e[SEGF_NQ];
    t_begin = e[SEGF_T0]; t_end = e[SEGF_T1]; split = (int)e[SEGF_OUT];
    ex_lo = (int)e[SEGF_CBASE]; ex_len = (int)(e[SEGF_NS] - e[SEGF_CBASE]);
  } else if constexpr (SEG) {
    const int64_t* e = a.sched + (size_t)blockIdx.x * SEGF_ENTRY;
    q0 = e[SEGF_ROW0]; qend = q0 + e[SEGF_NQ]; cbase = e[SEGF_CBASE];
    t_begin = e[SEGF_T0]; t_end = e[SEGF_T1]; obase = e[SEGF_OUT]; m = e[SEGF_NS];
    if constexpr (SSEG) split = (int)e[SEGF_OUT];   // the scan form keeps its column range's number there: the list slot
  } else {
    split = blockIdx.x % a.col_splits;
    const int64_t rb = blockIdx.x / a.col_splits;
    q0 = rb * F_QT;
    const int64_t total_tiles = (a.m + F_CT - 1) / F_CT;
    t_begin = (int64_t)split * a.tiles_per_split;
    t_end = t_begin + a.tiles_per_split;
    if (t_end > total_tiles) t_end = total_tiles;
    if (t_begin > t_end) t_begin = t_end;
  }
  const int nkc = (int)(a.dpad / F_KC);
  const int64_t steps = (t_end - t_begin) * nkc;

  // this lane's query
  const int64_t qpos = q0 + 32 * wave + c;
  const bool qvalid = SSEG ? (qpos < qend) : (qpos < a.n_rows);
  const int64_t qrow = qvalid ? (a.row_ids ? (int64_t)a.row_ids[qpos] : qpos) : 0;
  const float ri = qvalid ? a.rx[qrow] : 1.0f;
  const int metric = a.metric;
  const bool floored = (MODE == MODE_SCAN) && a.floor_key != nullptr;
  const float fk = (floored && qvalid) ? a.floor_key[qpos] : 0.0f;
  const uint32_t fid = (floored && qvalid) ? a.floor_id[qpos] : 0u;
  // COMB: this lane's position and its chain
  float pq[8], pnq = 0.0f;
  const float* Pc = nullptr; const float* pnc = nullptr; float nlg = 0.0f;
  if constexpr (COMB) {
    // uniform, but kept in vector registers: the list code under the epilogue has no scalar register to spare (in scalar
    // registers these five words cost ten scalar spills inside LaneList::compact)
    Pc = a.P; pnc = a.pnc; nlg = a.neg_lambda_g;
    asm volatile("" : "+v"(Pc), "+v"(pnc), "+v"(nlg));
#pragma unroll
    for (int e = 0; e < 8; ++e) pq[e] = (qvalid && e < a.dp) ? a.Pq[qrow * a.dp + e] : 0.0f;
    if (qvalid) pnq = a.pnq[qrow];
  }

  // DENSE: the 16 query rows this lane's accumulator elements belong to (fixed for the workgroup's lifetime)
  float rq16[16];
  if constexpr (MODE == MODE_DENSE) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t q = q0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
      rq16[r] = (q < qend) ? a.rx[q] : 1.0f;
    }
  }

  LaneList<CAP, F_NT> list;
  if constexpr (MODE == MODE_SCAN) {
    list.init(lkeys + tid, lids + tid);
    if (!qvalid) list.thr = __builtin_huge_valf();
  }

  // DMA roles: piece p = wave + 4 i covers image rows [(p % HP) * RPP, + RPP) of the query (p < HP) or candidate tile;
  // lane l lands at unit l of the piece = row l / UPR, unit l % UPR, and fetches the unit the swizzle puts there.
  // The lane's byte offset inside a tile image is loop invariant; chunk and tile move through scalar offsets.
  uint32_t voff[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int row = ((wave + 4 * i) % HP) * RPP + lane / UPR;
    const int lu = (lane % UPR) ^ ((row >> FSH) & (UPR - 1));
    voff[i] = (uint32_t)(((int64_t)row * a.dpad + 4 * lu) * 4);
  }
  const __amdgpu_buffer_rsrc_t qrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Xp + q0 * a.dpad), 0, -1, 0x00020000);
  float rcy = 0.0f;
  f32x4 rpp = {0.0f, 0.0f, 0.0f, 0.0f};   // COMB: floats 4 (tid & 1) .. + 3 of candidate tid >> 1's position
  float rpn = 0.0f;                       // COMB: chain(p, p) of candidate tid
  // chunk kc of candidate tile ct -> stage `buf`; the tile's 128 per-candidate scalars ride along with its first chunk
  auto stage = [&](int64_t ct, int kc, int buf) {
    if (kc == 0 && tid < F_CT) {
      int64_t j = ct * F_CT + tid;
      if (j > m - 1) j = m - 1;
      rcy = a.cy[cbase + j];
      if constexpr (COMB) rpn = pnc[cbase + j];
    }
    if constexpr (COMB) {
      if (kc == 0) {
        int64_t j = ct * F_CT + (tid >> 1);
        if (j > m - 1) j = m - 1;
        const int e0 = 4 * (tid & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) rpp[i] = (e0 + i < a.dp) ? Pc[(cbase + j) * a.dp + e0 + i] : 0.0f;
      }
    }
    if (a.debug & 2) return;
    const __amdgpu_buffer_rsrc_t crsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Yp + (cbase + ct * F_CT) * a.dpad), 0, -1, 0x00020000);
    const int koff = kc * F_KC * 4;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pr = (wave + 4 * i) % HP;
      if (i < PPW / 2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(qrsrc, (__attribute__((address_space(3))) void*)(Qs + buf * F_QT * F_KC + pr * RPP * F_KC),
                                                 16, (int)voff[i], koff, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(crsrc, (__attribute__((address_space(3))) void*)(Cs + buf * F_CT * F_KC + pr * RPP * F_KC),
                                                 16, (int)voff[i], koff, 0, 0);
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  // this lane's operand rows inside a stage: query row 32 wave + c, candidate rows c + 32 t (same swizzle for all t)
  const int rqrow = 32 * wave + c;
  const int fq = (rqrow >> FSH) & (UPR - 1), fc = (c >> FSH) & (UPR - 1);

  if (steps > 0) {
    stage(t_begin, 0, 0);
    if (tid < F_CT) cys[tid] = rcy;
    if constexpr (COMB) {
      *reinterpret_cast<f32x4*>(pss + 4 * tid) = rpp;
      if (tid < F_CT) pns[tid] = rpn;
    }
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

    const float* Qrow = Qs + buf * F_QT * F_KC + rqrow * F_KC;
    const float* Crow = Cs + buf * F_CT * F_KC + c * F_KC;
    // operands of group g + 1 are read from LDS before the MFMAs of group g issue
    f32x4 bn = *reinterpret_cast<const f32x4*>(Qrow + 4 * (half ^ fq));
    f32x4 avn[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) avn[t] = *reinterpret_cast<const f32x4*>(Crow + t * 32 * F_KC + 4 * (half ^ fc));
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const f32x4 b = bn;
      f32x4 av[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) av[t] = avn[t];
      if (g + 1 < NG) {
        bn = *reinterpret_cast<const f32x4*>(Qrow + 4 * ((2 * (g + 1) + half) ^ fq));
#pragma unroll
        for (int t = 0; t < 4; ++t) avn[t] = *reinterpret_cast<const f32x4*>(Crow + t * 32 * F_KC + 4 * ((2 * (g + 1) + half) ^ fc));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // SCAN: C rows = candidates, columns = queries (a lane owns one query).  DENSE: the transpose — a lane owns
          // one candidate COLUMN of the output, so the 32 lanes of a half store 128 contiguous bytes of one output
          // row.  Products commute, the k order is the same: both orientations give the same bits.
          if constexpr (MODE == MODE_DENSE) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[e], av[t][e], acc[t], 0, 0, 0);
          else acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][e], b[e], acc[t], 0, 0, 0);
        }
      }
    }

    if (kc == nkc - 1 && !(a.debug & 1)) {
      const int tpar = (int)((ct - t_begin) & 1);
      // one 32 x 32 sub-tile at a time (keeping all four key vectors live costs 64 VGPRs and pushes the
      // staging registers of the next chunk into AGPRs, i.e. a vmcnt(0) in front of the MFMA block)
      if constexpr (MODE == MODE_DENSE) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int64_t j = ct * F_CT + 32 * t + c;            // this lane's output column
          const bool jv = j < m;
          const float cj = cys[tpar * F_CT + 32 * t + c];
          const float nl = (metric == MMF_RBF) ? a.neg_lambda : -1.0f;  // (-1)*sq == -sq exactly
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t q = q0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float dot = acc[t][r];
            acc[t][r] = 0.0f;
            if (jv && q < qend) {
              float key;
              if (metric == MMF_DOT) key = dot;
              else if (metric == MMF_COSINE) key = key_from_dot<MMF_COSINE>(dot, rq16[r], cj, 0.0f);
              else key = key_from_dot<MMF_RBF>(dot, rq16[r], cj, nl);
              float v = (metric == MMF_RBF) ? expf(key) : key;
              if (a.P) {
                // K_g from the positions, canonical chains over dp (similarity_kernel.py:79-84, 122)
                float ni = 0.f, nj = 0.f, dp_ = 0.f;
                for (int e = 0; e < a.dp; ++e) {
                  const float pi = a.P[(a.prow0 + q) * a.dp + e], pj = a.P[(cbase + j) * a.dp + e];
                  ni = __builtin_fmaf(pi, pi, ni);
                  nj = __builtin_fmaf(pj, pj, nj);
                  dp_ = __builtin_fmaf(pi, pj, dp_);
                }
                v = v * expf(a.neg_lambda_g * sq_from(ni, nj, dp_));
              }
              a.out[obase + (q - cbase) * m + j] = v;
            }
          }
        }
      } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t cand0 = ct * F_CT + 32 * t;
        const float* cyt = cys + tpar * F_CT + 32 * t + 4 * half;
        f32x16 key;
        // keys in three wave-uniform flavours (no per-element switch): dot | dot/(r*c) | nl*((r+c)-2dot)
        if constexpr (COMB) {
          // nl_h*((r+c)-2dot) + nl_g*((pr+pc)-2pdot); the chain over the positions in 2, 4 or 8 terms (wave-uniform)
          const float* pst = pss + (tpar * F_CT + 32 * t + 4 * half) * 8;
          const float* pnt = pns + tpar * F_CT + 32 * t + 4 * half;
          auto keys = [&](auto terms) {
            constexpr int T = decltype(terms)::value;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const f32x4 c4 = *reinterpret_cast<const f32x4*>(cyt + 8 * g);
              const f32x4 n4 = *reinterpret_cast<const f32x4*>(pnt + 8 * g);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float pj[T];
                if constexpr (T == 2) {
                  const f32x2 v = *reinterpret_cast<const f32x2*>(pst + (8 * g + i) * 8);
                  pj[0] = v[0]; pj[1] = v[1];
                } else {
#pragma unroll
                  for (int u = 0; u < T; u += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(pst + (8 * g + i) * 8 + u);
                    pj[u] = v[0]; pj[u + 1] = v[1]; pj[u + 2] = v[2]; pj[u + 3] = v[3];
                  }
                }
                const float eh = key_from_dot<MMF_RBF>(acc[t][4 * g + i], ri, c4[i], a.neg_lambda);
                key[4 * g + i] = combined_key(eh, pos_exponent<T>(pq, pj, pnq, n4[i], nlg));
              }
            }
          };
          if (a.dp <= 2) keys(std::integral_constant<int, 2>{});
          else if (a.dp <= 4) keys(std::integral_constant<int, 4>{});
          else keys(std::integral_constant<int, 8>{});
        } else if (metric == MMF_DOT) {
#pragma unroll
          for (int r = 0; r < 16; ++r) key[r] = acc[t][r];
        } else if (metric == MMF_COSINE) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cyt + 8 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) key[4 * g + i] = key_from_dot<MMF_COSINE>(acc[t][4 * g + i], ri, c4[i], 0.0f);
          }
        } else {
          const float nl = (metric == MMF_RBF) ? a.neg_lambda : -1.0f;  // (-1)*sq == -sq exactly
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cyt + 8 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) key[4 * g + i] = key_from_dot<MMF_RBF>(acc[t][4 * g + i], ri, c4[i], nl);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool jv = (cand0 + (r & 3) + 8 * (r >> 2) + 4 * half) < (SSEG ? m : a.m);
          key[r] = jv ? key[r] : kNegInf;
          acc[t][r] = 0.0f;
        }
        if constexpr (XSEG) {
          // the row block's own segment: columns ex_lo .. ex_lo + ex_len - 1 (one unsigned compare per key; a sub-tile outside
          // the range, which is every sub-tile of all but the two boundary tiles, takes the branch around it)
          const int c0 = (int)cand0;
          if (c0 < ex_lo + ex_len && c0 > ex_lo - 32) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const uint32_t off = (uint32_t)(c0 + (r & 3) + 8 * (r >> 2) + 4 * half - ex_lo);
              key[r] = off < (uint32_t)ex_len ? kNegInf : key[r];
            }
          }
        }
        if (floored) {                             // wave-uniform: a later pass of a large-k call
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const uint32_t j = (uint32_t)((SSEG ? cbase : 0) + cand0 + (r & 3) + 8 * (r >> 2) + 4 * half);
            const bool after = (key[r] < fk) || (key[r] == fk && j > fid);
            key[r] = after ? key[r] : kNegInf;
          }
        }
        if (__builtin_expect(__any(max16(key) >= list.thr), 0)) list.offer_tile(key, (uint32_t)((SSEG ? cbase : 0) + cand0), half, a.kk);
      }
    }

      }
    if (s + 1 < steps && nkcn == 0 && tid < F_CT) cys[(int)((nct - t_begin) & 1) * F_CT + tid] = rcy;
    if constexpr (COMB) {
      if (s + 1 < steps && nkcn == 0) {
        const int par = (int)((nct - t_begin) & 1);
        *reinterpret_cast<f32x4*>(pss + par * F_CT * 8 + 4 * tid) = rpp;
        if (tid < F_CT) pns[par * F_CT + tid] = rpn;
      }
    }
    ct = nct; kc = nkcn;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next chunk have landed
    __syncthreads();
  }

  if constexpr (MODE == MODE_SCAN) {
    list.compact(a.kk);
    if (qvalid) {
      const int64_t lbase = qpos * (2 * a.col_splits) + 2 * split + half;
      a.cand_cnt[lbase] = (uint32_t)list.cnt;
      for (int e = 0; e < list.cnt; ++e) a.cand_ids[lbase * CAP + e] = list.ids[e * F_NT];
      if (list.overflow) atomicOr(a.overflow + qpos, 1u);
    }
  }
}

// ------------------------------------------------------------------------------------------------
int scan_f32_cap(int kk) {
  if (kk <= 12) return 16;
  if (kk <= 28) return 32;
  if (kk <= 44) return 48;     // 48 x 256 x 8 B of lists + 36 KB of tiles: one workgroup per CU
  return 0;
}

static size_t scan_f32_lds(int cap, int kc) {
  return sizeof(float) * (2 * F_QT * kc + 2 * F_CT * kc + 2 * F_CT) + (size_t)cap * F_NT * 8;
}
constexpr size_t kScanPosLds = sizeof(float) * 2 * F_CT * 9;   // COMB: the tiles' positions and their chains

template <int MODE, int CAP, bool SEG = false, bool COMB = false, bool XSEG = false>
static int launch_f32_t(const ScanF32Args& a, int64_t grid, hipStream_t s) {
  if (a.metric < MMF_DOT || a.metric > MMF_RBF) {
    set_error("scan_f32: unsupported metric %d", a.metric);
    return MMF_E_INVALID;
  }
  if (!a.Xp || !a.Yp || a.dpad <= 0 || (a.dpad & 31) != 0 || a.dpad > (int64_t(1) << 21)) {
    set_error("scan_f32: missing f32 operand images (or padded dim %lld not a multiple of 32 below 2^21)", (long long)a.dpad);
    return MMF_E_INTERNAL;
  }
  constexpr int KC = (MODE == MODE_SCAN) ? 16 : 32;
  const size_t lds = scan_f32_lds(MODE == MODE_SCAN ? CAP : 0, KC) + (COMB ? kScanPosLds : 0);
  auto kern = scan_f32_kernel<MODE, CAP, KC, SEG, COMB, XSEG>;
  MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(F_NT), lds, s, a);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

int launch_scan_f32(const ScanProblem& p, const CandLists& L, hipStream_t s, int* grid_out) {
  if (p.n_rows <= 0 || p.m <= 0) return MMF_OK;
  ScanF32Args a{};
  a.Xp = p.Xp; a.Yp = p.Yp; a.n = p.n; a.m = p.m; a.dpad = prep_f32_dim(p.d);
  a.rx = p.rx; a.cy = p.cy; a.row_ids = p.row_ids; a.n_rows = p.n_rows;
  a.neg_lambda = -p.lambda; a.kk = p.kk; a.col_splits = p.col_splits;
  const int64_t total_tiles = (p.m + F_CT - 1) / F_CT;
  a.tiles_per_split = (total_tiles + p.col_splits - 1) / p.col_splits;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.overflow = L.overflow;
  a.floor_key = p.floor_key; a.floor_id = p.floor_id;
  const int64_t grid = ((p.n_rows + F_QT - 1) / F_QT) * p.col_splits;
  if (grid_out) *grid_out = (int)grid;
  a.metric = p.metric;
  { const char* e = getenv("MMF_F32_DEBUG"); a.debug = e ? atoi(e) : 0; }
  if (p.Pc) {   // the combined key (mmf_simtopk_combined)
    // (gathered rows — p.row_ids — are served: the kernel takes a query's scalar, position and chain by row and its image, floor
    // and lists by position; Pq / pnq are then the whole query side's, as rx is)
    if (!p.Pq || !p.pnq || !p.pnc || p.dp < 1 || p.dp > 8 || p.metric != MMF_RBF) {
      set_error("scan_f32: combined key needs both sides' positions and chains, 1 <= dp <= 8 (got %d) and MMF_RBF", p.dp);
      return MMF_E_INTERNAL;
    }
    a.P = p.Pc; a.Pq = p.Pq; a.pnq = p.pnq; a.pnc = p.pnc; a.dp = p.dp; a.neg_lambda_g = -p.lambda_g;
    if (L.cap == 16) return launch_f32_t<MODE_SCAN, 16, false, true>(a, grid, s);
    if (L.cap == 32) return launch_f32_t<MODE_SCAN, 32, false, true>(a, grid, s);
    if (L.cap == 48) return launch_f32_t<MODE_SCAN, 48, false, true>(a, grid, s);
    set_error("scan_f32: unsupported list capacity %d", L.cap);
    return MMF_E_INTERNAL;
  }
  if (L.cap == 16) return launch_f32_t<MODE_SCAN, 16>(a, grid, s);
  if (L.cap == 32) return launch_f32_t<MODE_SCAN, 32>(a, grid, s);
  if (L.cap == 48) return launch_f32_t<MODE_SCAN, 48>(a, grid, s);
  set_error("scan_f32: unsupported list capacity %d", L.cap);
  return MMF_E_INTERNAL;
}

// The work table of the segmented exact scan ([entries][SEGF_ENTRY] int64, one entry per workgroup): every segment with rows
// and at least k admissible columns ("served") gets, per block of F_QT of its rows, one entry per column range.  A segment of T
// column tiles has R ranges of ceil(T / R) tiles (the empty ones at the end make no entry); R is a power of two, at most T, at
// most `col_splits` when that is forced (> 0), and 2 R cap <= 1024 candidates per row of the re-rank.  col_splits == 0 is the
// automatic rule, sim_dense_combined_seg_table's: runs of `per` tiles, `per` sized so that the call makes about 1024 workgroups —
// a few large segments split their columns and fill the chip, many segments are one range each (measured: DESIGN.md §4.20).
// y_ptr == x_ptr for a self call.  *ranges_out: the largest R.
std::vector<int64_t> seg_exact_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int k, int exclude_self, int col_splits,
                                     int* ranges_out, std::vector<char>* served_out) {
  const int kk = k + (exclude_self ? 1 : 0);
  const int cap = scan_f32_cap(kk < 44 ? kk : 44);
  int max_r = 1;
  while (2 * (2 * max_r) * cap <= 1024) max_r <<= 1;
  std::vector<char> served((size_t)S, 0);
  int64_t pairs = 0;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = x_ptr[g + 1] - x_ptr[g], mg = y_ptr[g + 1] - y_ptr[g];
    const bool overlap = exclude_self && x_ptr[g] < y_ptr[g] + mg && x_ptr[g] + ng > y_ptr[g];
    served[g] = ng > 0 && mg - (overlap ? 1 : 0) >= k;
    if (served[g]) pairs += ((ng + F_QT - 1) / F_QT) * ((mg + F_CT - 1) / F_CT);
  }
  const int64_t per = std::max<int64_t>(1, (pairs + 1023) / 1024);
  std::vector<int64_t> tab;
  int ranges = 1;
  for (int64_t g = 0; g < S; ++g) {
    if (!served[g]) continue;
    const int64_t ng = x_ptr[g + 1] - x_ptr[g], mg = y_ptr[g + 1] - y_ptr[g], tiles = (mg + F_CT - 1) / F_CT;
    const int64_t want = col_splits > 0 ? col_splits : (tiles + per - 1) / per;
    int R = 1;
    while (2 * R <= want && 2 * R <= tiles && 2 * R <= max_r) R <<= 1;
    if (R > ranges) ranges = R;
    const int64_t tps = (tiles + R - 1) / R;
    for (int64_t r = 0; r < ng; r += F_QT)
      for (int c = 0; c < R && c * tps < tiles; ++c) {
        const int64_t e[SEGF_ENTRY] = {g, x_ptr[g] + r, ng - r < F_QT ? ng - r : F_QT, y_ptr[g], c * tps,
                                       std::min<int64_t>((c + 1) * tps, tiles), c, mg};
        tab.insert(tab.end(), e, e + SEGF_ENTRY);
      }
  }
  if (ranges_out) *ranges_out = ranges;
  if (served_out) served_out->swap(served);
  return tab;
}

// The work table of the cross-segment scan (mmf_simtopk_cross_segments), the layout of seg_exact_table with two
// words re-used: entry = segment, first row of X, real queries, ex_lo = y_ptr[s] (SEGF_CBASE), first and end tile, number of the
// column range, ex_hi = y_ptr[s + 1] (SEGF_NS).  The column tiles are the F_CT-row tiles of ALL of Y from row 0, T = ceil(m / F_CT)
// of them.  The segment's hole is the tiles that lie wholly inside [ex_lo, ex_hi) — tiles ceil(ex_lo / F_CT) up to floor(ex_hi /
// F_CT), up to T when ex_hi == m: they appear in no entry; a tile that straddles a bound appears once and the kernel masks it.  The
// A = T - hole admissible tiles, numbered without the hole, are cut into R runs of ceil(A / R) as in seg_exact_table: R a power of
// two, at most A, at most `col_splits` when that is forced (> 0), else ceil(A / per) with `per` sized so that the call makes about
// 1024 workgroups.  A run that spans the hole becomes TWO entries, one on each side of it, with range numbers (and so list slots)
// of their own: the ranges of a block are numbered 0, 1, ... in tile order, at most R + 1 of them, which is why R stops at the
// largest power of two with 2 (R + 1) cap <= 1024, the re-rank's candidates per row.  A segment without rows, or without an
// admissible tile, makes no entry; a segment with no rows of Y excludes nothing.  *ranges_out: the largest range count of a block.
std::vector<int64_t> cross_seg_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int k, int col_splits, int* ranges_out) {
  const int cap = scan_f32_cap(k < 44 ? k : 44);
  int max_r = 1;
  while (2 * (2 * max_r + 1) * cap <= 1024) max_r <<= 1;
  const int64_t m = S > 0 ? y_ptr[S] : 0, T = (m + F_CT - 1) / F_CT;
  auto hole = [&](int64_t g, int64_t* h0, int64_t* h1) {
    *h0 = (y_ptr[g] + F_CT - 1) / F_CT;
    *h1 = y_ptr[g + 1] == m ? T : y_ptr[g + 1] / F_CT;
    if (*h1 < *h0) *h1 = *h0;
  };
  int64_t pairs = 0;
  for (int64_t g = 0; g < S; ++g) {
    int64_t h0, h1;
    hole(g, &h0, &h1);
    pairs += ((x_ptr[g + 1] - x_ptr[g] + F_QT - 1) / F_QT) * (T - (h1 - h0));
  }
  const int64_t per = std::max<int64_t>(1, (pairs + 1023) / 1024);
  std::vector<int64_t> tab;
  int ranges = 1;
  for (int64_t g = 0; g < S; ++g) {
    const int64_t ng = x_ptr[g + 1] - x_ptr[g];
    int64_t h0, h1;
    hole(g, &h0, &h1);
    const int64_t adm = T - (h1 - h0);
    if (ng <= 0 || adm <= 0) continue;
    const int64_t want = col_splits > 0 ? col_splits : (adm + per - 1) / per;
    int R = 1;
    while (2 * R <= want && 2 * R <= adm && 2 * R <= max_r) R <<= 1;
    const int64_t tps = (adm + R - 1) / R;
    for (int64_t r = 0; r < ng; r += F_QT) {
      int number = 0;
      auto entry = [&](int64_t t0, int64_t t1) {
        if (t0 >= t1) return;
        const int64_t e[SEGF_ENTRY] = {g, x_ptr[g] + r, ng - r < F_QT ? ng - r : F_QT, y_ptr[g], t0, t1, number++, y_ptr[g + 1]};
        tab.insert(tab.end(), e, e + SEGF_ENTRY);
      };
      for (int64_t a0 = 0; a0 < adm; a0 += tps) {
        // admissible tile a is tile a below the hole and tile a + (h1 - h0) above it
        const int64_t a1 = std::min(a0 + tps, adm);
        if (h1 == h0 || a1 <= h0) entry(a0, a1);
        else if (a0 >= h0) entry(a0 + (h1 - h0), a1 + (h1 - h0));
        else { entry(a0, h0); entry(h1, a1 + (h1 - h0)); }
      }
      if (number > ranges) ranges = number;
    }
  }
  // Longest run first.  The two sides of a hole are as uneven as the segment's place in the batch makes them (a block of the
  // last segment is one run of nearly all tiles and one of none), and in table order the longest runs would start last: measured
  //  the launch then ends in a tail of a few long workgroups.  Entries are independent, so any order is correct.
  const size_t entries = tab.size() / SEGF_ENTRY;
  std::vector<size_t> order(entries);
  for (size_t i = 0; i < entries; ++i) order[i] = i;
  auto len = [&](size_t i) { return tab[i * SEGF_ENTRY + SEGF_T1] - tab[i * SEGF_ENTRY + SEGF_T0]; };
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return len(a) > len(b); });
  std::vector<int64_t> sorted(tab.size());
  for (size_t i = 0; i < entries; ++i) std::copy_n(tab.begin() + order[i] * SEGF_ENTRY, SEGF_ENTRY, sorted.begin() + i * SEGF_ENTRY);
  if (ranges_out) *ranges_out = ranges;
  return sorted;
}

namespace {

// Row block geometry shared by the two 16-bit cross-segment tables (cross_seg16_table, cross_segw_table): hole [h0, h1) and mask
// window [w0, w1) of every block of qt rows of X, in tiles of `tile` rows of the plain image of Y (T tiles).
struct CrossBlock { int64_t h0, h1, w0, w1; };
std::vector<CrossBlock> cross_blocks(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int qt, int tile, int64_t T) {
  const int64_t n = S > 0 ? x_ptr[S] : 0, m = S > 0 ? y_ptr[S] : 0;
  std::vector<CrossBlock> blocks((size_t)((n + qt - 1) / qt));
  int64_t g = 0;
  for (size_t b = 0; b < blocks.size(); ++b) {
    const int64_t r0 = (int64_t)b * qt, r1 = std::min<int64_t>(r0 + qt, n);
    while (x_ptr[g + 1] <= r0) ++g;                      // segment of the block's first row (empty segments hold no row)
    int64_t gl = g;
    while (x_ptr[gl + 1] <= r1 - 1) ++gl;                // ... and of its last
    const int64_t ulo = y_ptr[g], uhi = y_ptr[gl + 1];
    CrossBlock& B = blocks[b];
    B.h0 = B.h1 = 0;
    if (gl == g) {
      B.h0 = (ulo + tile - 1) / tile;
      B.h1 = uhi == m ? T : uhi / tile;
      if (B.h1 < B.h0) B.h1 = B.h0;
    }
    B.w0 = ulo / tile; B.w1 = uhi > ulo ? (uhi + tile - 1) / tile : B.w0;
  }
  return blocks;
}

// The T - hole admissible tiles of block B cut into R runs of ceil(A / R); a run that spans the hole is two entries.  Calls
// entry(t0, t1, w0, w1) in tile order ([w0, w1): the entry's part of the mask window, w0 == w1 == t0 when it has none) and returns
// the number of entries.
template <class Entry>
int cross_block_runs(const CrossBlock& B, int64_t T, int R, Entry entry) {
  const int64_t hole = B.h1 - B.h0, adm = T - hole, tps = (adm + R - 1) / R;
  int count = 0;
  auto one = [&](int64_t t0, int64_t t1) {
    if (t0 >= t1) return;
    int64_t w0 = std::max(B.w0, t0), w1 = std::min(B.w1, t1);
    if (w0 >= w1) w0 = w1 = t0;
    entry(t0, t1, w0, w1);
    ++count;
  };
  for (int64_t a0 = 0; a0 < adm; a0 += tps) {
    const int64_t a1 = std::min(a0 + tps, adm);          // admissible tile a is tile a below the hole and a + hole above it
    if (hole == 0 || a1 <= B.h0) one(a0, a1);
    else if (a0 >= B.h0) one(a0 + hole, a1 + hole);
    else { one(a0, B.h0); one(B.h1, a1 + hole); }
  }
  return count;
}

// entries of 8 int32 words, first / end tile in words 3 / 4: longest run first (stable)
std::vector<int32_t> longest_run_first(const std::vector<int32_t>& tab) {
  const size_t entries = tab.size() / 8;
  std::vector<size_t> order(entries);
  for (size_t i = 0; i < entries; ++i) order[i] = i;
  auto len = [&](size_t i) { return tab[i * 8 + 4] - tab[i * 8 + 3]; };
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return len(a) > len(b); });
  std::vector<int32_t> sorted(tab.size());
  for (size_t i = 0; i < entries; ++i) std::copy_n(tab.begin() + order[i] * 8, 8, sorted.begin() + i * 8);
  return sorted;
}

}  // namespace

// The work table of the 16-bit cross-segment scan (mmf_simtopk_cross_segments_fast): [entries][8] int32, the
// words of the 16-bit scan's SEG entry with the id-offset word (zero on the plain images) carrying the list slot —
//   first row of the block (operand position = list row), the same again, real queries, first and end tile, list slot, and the
//   mask window [w0, w1) of the entry (w0 == w1: no tile of it needs the mask).
// Row block b is rows [b qt, min((b + 1) qt, n)) of X whatever the segments: with s_first / s_last the segments of its first and
// last row, U = [y_ptr[s_first], y_ptr[s_last + 1]) is the union of its rows' excluded ranges and I their intersection (U for a
// block inside one segment, empty otherwise).  The column tiles are the 32-row tiles of the plain image of Y, T = m_pad / 32 of
// them (m_pad: m rounded up to 256).  The block's hole — in no entry — is the tiles wholly inside I: ceil(I.lo / 32) up to
// floor(I.hi / 32), up to T when I.hi == m (the tiles behind m hold padding only).  Its mask window is the tiles that meet U
// without the hole.  The A = T - hole admissible tiles are cut into R runs of ceil(A / R) by cross_seg_table's rule (R a power of
// two, at most A, `col_splits` when forced, else ceil(A / per) with `per` sized for about 1024 workgroups per call but no run shorter
// than 64 tiles, the cadence of the threshold exchange), R capped at
// the largest power of two with 2 (R + 1) cap <= cand_budget (what the re-rank takes per row beside the overflow list) and raised
// while a run would pass the 32-bit offsets of the tile DMA (run tiles x 32 x dp x 2 bytes < 2^32); a run that spans the hole is
// two entries.  Slots number a block's entries in tile order.  Entries come longest run first.  *lists_out: 2 x the largest entry
// count of a block, or -1 when a run cannot be made short enough (the table is then empty).
std::vector<int32_t> cross_seg16_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int qt, int dp, int cap, int cand_budget,
                                       int col_splits, int* lists_out) {
  const int64_t n = S > 0 ? x_ptr[S] : 0, m = S > 0 ? y_ptr[S] : 0;
  const int64_t T = (m + 255) / 256 * 8;
  int max_r = 1;
  while (2 * (2 * max_r + 1) * cap <= cand_budget) max_r <<= 1;
  const int64_t max_run = (((int64_t)1 << 32) - 1) / ((int64_t)64 * dp);
  const std::vector<CrossBlock> blocks = cross_blocks(x_ptr, y_ptr, S, qt, 32, T);
  int64_t pairs = 0;
  for (const CrossBlock& B : blocks) pairs += T - (B.h1 - B.h0);
  const int64_t per = std::max<int64_t>(1, (pairs + 1023) / 1024);
  std::vector<int32_t> tab;
  int most = 1;
  for (size_t b = 0; b < blocks.size(); ++b) {
    const CrossBlock& B = blocks[b];
    const int64_t r0 = (int64_t)b * qt, adm = T - (B.h1 - B.h0);
    if (adm <= 0) continue;
    // automatic: no run shorter than kMinRun tiles.  The workgroups of a row block exchange thresholds every 64 tiles (sync_seed), so
    // a shorter run never imports one on its way and proves its own from a few hundred columns only: measured at 2001 rows, d = 600,
    // k = 20 with bf16 operands, sixteen runs of four tiles flagged 286 rows for the exact rescan, one run none.
    constexpr int64_t kMinRun = 64;
    const int64_t want = col_splits > 0 ? col_splits : std::min((adm + per - 1) / per, std::max<int64_t>(1, adm / kMinRun));
    int R = 1;
    while (2 * R <= want && 2 * R <= adm && 2 * R <= max_r) R <<= 1;
    while ((adm + R - 1) / R > max_run && 2 * R <= adm && 2 * R <= max_r) R <<= 1;
    if ((adm + R - 1) / R > max_run) { if (lists_out) *lists_out = -1; return {}; }
    int slot = 0;
    const int count = cross_block_runs(B, T, R, [&](int64_t t0, int64_t t1, int64_t w0, int64_t w1) {
      const int32_t e[8] = {(int32_t)r0, (int32_t)r0, (int32_t)std::min<int64_t>(qt, n - r0), (int32_t)t0, (int32_t)t1, slot++, (int32_t)w0, (int32_t)w1};
      tab.insert(tab.end(), e, e + 8);
    });
    if (count > most) most = count;
  }
  if (lists_out) *lists_out = 2 * most;
  return longest_run_first(tab);
}

// The work table of the wide 16-bit cross-segment scan (mmf_simtopk_cross_segments_wide): cross_seg16_table's rule
// with the wide kernel's numbers — row blocks of 128 rows of X, column tiles of 128 rows of the plain image of Y, T = m_pad / 128 of
// them (m_pad: m rounded up to 256) — in the wide scan's entry layout (mmf_scan_b16w.hip, WSEG_* / WXSEG_*):
//   first row of the block (operand position = list row), the same again, real queries, first and end tile, first tile of the mask
//   window, first list slot (2 x the entry's number in its block, in tile order), end tile of the mask window.
// Hole, mask window, runs and the two entries of a run that spans the hole are cross_blocks' and cross_block_runs'.  R is a power of
// two, at most A, at most the largest one with 2 (R + 1) cap <= cand_budget (16 at cap 16, 8 at cap 32: the bounds of §4.16);
// `col_splits` when forced (> 0), else the smallest power of two with (row blocks) x R >= 256 — the wide kernel runs one workgroup
// per CU — but no automatic run shorter than 8 tiles.  The wide kernel moves a tile through the buffer base: no run is too long.
// Entries come longest run first.  *lists_out: 2 x the largest entry count of a block.
std::vector<int32_t> cross_segw_table(const int64_t* x_ptr, const int64_t* y_ptr, int64_t S, int cap, int cand_budget, int col_splits,
                                      int* lists_out) {
  constexpr int kQT = 128, kTile = 128;
  constexpr int64_t kFill = 256, kMinRun = 8;
  const int64_t n = S > 0 ? x_ptr[S] : 0, m = S > 0 ? y_ptr[S] : 0;
  const int64_t T = (m + 255) / 256 * 2;
  int max_r = 1;
  while (2 * (2 * max_r + 1) * cap <= cand_budget) max_r <<= 1;
  const std::vector<CrossBlock> blocks = cross_blocks(x_ptr, y_ptr, S, kQT, kTile, T);
  int64_t fill = 1;
  while ((int64_t)blocks.size() * fill < kFill && fill < max_r) fill <<= 1;
  std::vector<int32_t> tab;
  int most = 1;
  for (size_t b = 0; b < blocks.size(); ++b) {
    const CrossBlock& B = blocks[b];
    const int64_t r0 = (int64_t)b * kQT, adm = T - (B.h1 - B.h0);
    if (adm <= 0) continue;
    const int64_t want = col_splits > 0 ? col_splits : std::min(fill, std::max<int64_t>(1, adm / kMinRun));
    int R = 1;
    while (2 * R <= want && 2 * R <= adm && 2 * R <= max_r) R <<= 1;
    int number = 0;
    const int count = cross_block_runs(B, T, R, [&](int64_t t0, int64_t t1, int64_t w0, int64_t w1) {
      const int32_t e[8] = {(int32_t)r0, (int32_t)r0, (int32_t)std::min<int64_t>(kQT, n - r0), (int32_t)t0, (int32_t)t1, (int32_t)w0,
                            2 * number++, (int32_t)w1};
      tab.insert(tab.end(), e, e + 8);
    });
    if (count > most) most = count;
  }
  if (lists_out) *lists_out = 2 * most;
  return longest_run_first(tab);
}

// One workgroup per entry of the device copy `sched` of that table.  p.Xp / p.Yp: the f32 images of ALL rows of X and Y; p.rx /
// p.cy, the floors, the positions and the lists L (L.lists = 2 x the table's largest range count) cover all rows; p.kk, the
// metric and the floors are those of launch_scan_f32.  Counts of the slots a segment does not use must be zero already.
// cross: `sched` is a cross_seg_table and the kernel is the XSEG flavour (no combined key).
int launch_scan_f32_seg(const ScanProblem& p, const CandLists& L, const int64_t* sched, int64_t grid, hipStream_t s, bool cross) {
  if (grid <= 0) return MMF_OK;
  // (gathered rows — p.row_ids: the table's rows are positions of p.Xp and of the lists, position q is row row_ids[q] of X — go with
  //  the cross flavour only: the flagged rows of mmf_simtopk_cross_segments_fast)
  if ((p.row_ids && !cross) || !sched || L.lists < 2 || (L.lists & 1)) { set_error("scan_f32_seg: needs a work table, list pairs and no gathered rows"); return MMF_E_INTERNAL; }
  ScanF32Args a{};
  a.Xp = p.Xp; a.Yp = p.Yp; a.n = p.n; a.m = p.m; a.dpad = prep_f32_dim(p.d);
  a.rx = p.rx; a.cy = p.cy; a.row_ids = cross ? p.row_ids : nullptr; a.n_rows = p.n;
  a.neg_lambda = -p.lambda; a.kk = p.kk; a.col_splits = L.lists / 2; a.tiles_per_split = 0;
  a.cand_cnt = L.cnt; a.cand_ids = L.ids; a.overflow = L.overflow;
  a.floor_key = p.floor_key; a.floor_id = p.floor_id;
  a.metric = p.metric;
  a.sched = sched;
  if (cross) {
    if (p.Pc || p.m >= ((int64_t)1 << 31)) { set_error("scan_f32_seg: the cross flavour has no combined key and needs m < 2^31"); return MMF_E_INTERNAL; }
    if (L.cap == 16) return launch_f32_t<MODE_SCAN, 16, true, false, true>(a, grid, s);
    if (L.cap == 32) return launch_f32_t<MODE_SCAN, 32, true, false, true>(a, grid, s);
    if (L.cap == 48) return launch_f32_t<MODE_SCAN, 48, true, false, true>(a, grid, s);
  } else if (p.Pc) {
    if (!p.Pq || !p.pnq || !p.pnc || p.dp < 1 || p.dp > 8 || p.metric != MMF_RBF) {
      set_error("scan_f32_seg: combined key needs both sides' positions and chains, 1 <= dp <= 8 (got %d) and MMF_RBF", p.dp);
      return MMF_E_INTERNAL;
    }
    a.P = p.Pc; a.Pq = p.Pq; a.pnq = p.pnq; a.pnc = p.pnc; a.dp = p.dp; a.neg_lambda_g = -p.lambda_g;
    if (L.cap == 16) return launch_f32_t<MODE_SCAN, 16, true, true>(a, grid, s);
    if (L.cap == 32) return launch_f32_t<MODE_SCAN, 32, true, true>(a, grid, s);
    if (L.cap == 48) return launch_f32_t<MODE_SCAN, 48, true, true>(a, grid, s);
  } else {
    if (L.cap == 16) return launch_f32_t<MODE_SCAN, 16, true>(a, grid, s);
    if (L.cap == 32) return launch_f32_t<MODE_SCAN, 32, true>(a, grid, s);
    if (L.cap == 48) return launch_f32_t<MODE_SCAN, 48, true>(a, grid, s);
  }
  set_error("scan_f32_seg: unsupported list capacity %d", L.cap);
  return MMF_E_INTERNAL;
}

// d <= 8 (the spatial similarity of similarity_kernel.py:58-86 has d = 2): no matrix cores, the kernel is pure
// output bandwidth.  A thread owns 4 consecutive output columns (its 4 y vectors stay in registers) and walks 16
// rows; each store is 16 bytes per lane, 1 KiB contiguous per wave.  Same canonical chains and keys as everywhere.
__global__ __launch_bounds__(256) void dense_small_d_kernel(const void* __restrict__ X, int64_t n, const void* __restrict__ Y,
                                                            int64_t m, int d, int dtype, int metric, float neg_lambda,
                                                            const float* __restrict__ rx, const float* __restrict__ cy,
                                                            float* __restrict__ out) {
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t i0 = (int64_t)blockIdx.y * 16;
  if (j0 >= m) return;
  float y[4][8], cj[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int64_t j = (j0 + jj < m) ? (j0 + jj) : (m - 1);
    cj[jj] = cy[j];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[jj][k] = (k < d) ? ld_elem(Y, j * d + k, dtype) : 0.0f;
  }
  const float nl = (metric == MMF_RBF) ? neg_lambda : -1.0f;
  const bool vec = ((m & 3) == 0) && (j0 + 3 < m) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  for (int ii = 0; ii < 16; ++ii) {
    const int64_t i = i0 + ii;
    if (i >= n) break;
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (k < d) ? ld_elem(X, i * d + k, dtype) : 0.0f;
    const float ri = rx[i];
    f32x4 v;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      float dot = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < d) dot = __builtin_fmaf(x[k], y[jj][k], dot);
      float key;
      if (metric == MMF_DOT) key = dot;
      else if (metric == MMF_COSINE) key = key_from_dot<MMF_COSINE>(dot, ri, cj[jj], 0.0f);
      else key = key_from_dot<MMF_RBF>(dot, ri, cj[jj], nl);
      v[jj] = (metric == MMF_RBF) ? expf(key) : key;
    }
    float* o = out + i * m + j0;
    if (vec) *reinterpret_cast<f32x4*>(o) = v;
    else {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        if (j0 + jj < m) o[jj] = v[jj];
    }
  }
}

bool sim_dense_needs_images(int64_t d, int metric) { return d > 8 && metric != MMF_RBF_DIRECT; }

int launch_sim_dense(const void* X, int64_t n, const void* Y, int64_t m, int64_t d, int dtype, int metric,
                     float lambda, const float* rx, const float* cy, const float* Xp, const float* Yp, float* out,
                     hipStream_t s) {
  if (n <= 0 || m <= 0) return MMF_OK;
  if (d <= 8 && metric != MMF_RBF_DIRECT) {
    dim3 grid((unsigned)((m + 1023) / 1024), (unsigned)((n + 15) / 16));
    hipLaunchKernelGGL(dense_small_d_kernel, grid, dim3(256), 0, s, X, n, Y, m, (int)d, dtype, metric, -lambda, rx, cy, out);
    MMF_LAUNCH_CHECK();
    return MMF_OK;
  }
  if (metric == MMF_RBF_DIRECT) return launch_rbf_direct(X, n, Y, m, d, dtype, lambda, out, nullptr, nullptr, s);   // mmf_direct.hip
  ScanF32Args a{};
  a.Xp = Xp; a.Yp = Yp; a.n = n; a.m = m; a.dpad = prep_f32_dim(d);
  a.rx = rx; a.cy = cy; a.row_ids = nullptr; a.n_rows = n;
  a.neg_lambda = -lambda; a.kk = 0;
  const int64_t total_tiles = (m + F_CT - 1) / F_CT;
  const int64_t rbs = (n + F_QT - 1) / F_QT;
  int64_t splits = (1024 + rbs - 1) / rbs;
  if (splits > total_tiles) splits = total_tiles;
  if (splits < 1) splits = 1;
  a.col_splits = (int)splits;
  a.tiles_per_split = (total_tiles + splits - 1) / splits;
  a.out = out;
  a.metric = metric;
  { const char* e = getenv("MMF_F32_DEBUG"); a.debug = e ? atoi(e) : 0; }
  return launch_f32_t<MODE_DENSE, 16>(a, rbs * splits, s);
}

int launch_sim_dense_combined(const float* Fp, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h,
                              float lambda_g, const float* nf, int64_t row0, int64_t rows, float* out, hipStream_t s) {
  if (n <= 0 || rows <= 0) return MMF_OK;
  ScanF32Args a{};
  a.dpad = prep_f32_dim(d);
  a.Xp = Fp + row0 * a.dpad; a.Yp = Fp; a.n = rows; a.m = n;
  a.rx = nf + row0; a.cy = nf; a.row_ids = nullptr; a.n_rows = rows;
  a.neg_lambda = -lambda_h; a.kk = 0;
  const int64_t total_tiles = (n + F_CT - 1) / F_CT;
  const int64_t rbs = (rows + F_QT - 1) / F_QT;
  int64_t splits = (1024 + rbs - 1) / rbs;
  if (splits > total_tiles) splits = total_tiles;
  a.col_splits = (int)splits;
  a.tiles_per_split = (total_tiles + splits - 1) / splits;
  a.out = out; a.P = P; a.dp = (int)dp; a.neg_lambda_g = -lambda_g; a.prow0 = row0;
  a.metric = MMF_RBF;
  return launch_f32_t<MODE_DENSE, 16>(a, rbs * splits, s);
}


// Segmented dense combined similarity (mmf_sim_dense_combined_segmented): the work table over the segments ptr[0..S] of a
// batch, [entries][SEGF_ENTRY] int64.  Each row block of F_QT rows of a segment takes its segment's column tiles in runs of
// at most `per` tiles, `per` chosen so that the batch makes about as many workgroups as one plain call (1024 row block x
// column split pairs): a few large segments split their columns and still fill the chip, thousands of small ones are one
// entry each.  Every tile starts at a row below ptr[S] = n (the invariant that keeps the unbounded tile loads inside the
// image, prep_f32_bytes).
std::vector<int64_t> sim_dense_combined_seg_table(const int64_t* ptr, int64_t S) {
  int64_t pairs = 0;
  for (int64_t sg = 0; sg < S; ++sg) {
    const int64_t b = (ptr[sg + 1] - ptr[sg] + F_QT - 1) / F_QT;
    pairs += b * b;
  }
  int64_t per = (pairs + 1023) / 1024;
  if (per < 1) per = 1;
  std::vector<int64_t> tab;
  int64_t kbase = 0;
  for (int64_t sg = 0; sg < S; ++sg) {
    const int64_t ns = ptr[sg + 1] - ptr[sg], tiles = (ns + F_CT - 1) / F_CT;
    for (int64_t r = 0; r < ns; r += F_QT)
      for (int64_t t0 = 0; t0 < tiles; t0 += per) {
        const int64_t e[SEGF_ENTRY] = {sg, ptr[sg] + r, ns - r < F_QT ? ns - r : F_QT, ptr[sg], t0, t0 + per < tiles ? t0 + per : tiles, kbase, ns};
        tab.insert(tab.end(), e, e + SEGF_ENTRY);
      }
    kbase += ns * ns;
  }
  return tab;
}

// One workgroup per entry of the device copy `sched` of that table (grid entries).  Fp / nf / P: f32 image, norms and
// positions of all rows of the batch; out: the blocks K_s, block s at sched's output base.  The kernel of
// launch_sim_dense_combined with its schedule read from the table (template flag SEG: the other instantiations are untouched).
int launch_sim_dense_combined_seg(const float* Fp, const float* P, int64_t d, int64_t dp, float lambda_h, float lambda_g,
                                  const float* nf, const int64_t* sched, int64_t grid, float* out, hipStream_t s) {
  if (grid <= 0) return MMF_OK;
  ScanF32Args a{};
  a.dpad = prep_f32_dim(d);
  a.Xp = Fp; a.Yp = Fp; a.n = 0; a.m = 0;
  a.rx = nf; a.cy = nf; a.row_ids = nullptr; a.n_rows = 0;
  a.neg_lambda = -lambda_h; a.kk = 0;
  a.col_splits = 1; a.tiles_per_split = 0;
  a.out = out; a.P = P; a.dp = (int)dp; a.neg_lambda_g = -lambda_g; a.prow0 = 0;
  a.metric = MMF_RBF;
  a.sched = sched;
  return launch_f32_t<MODE_DENSE, 16, true>(a, grid, s);
}

}  // namespace mmf
