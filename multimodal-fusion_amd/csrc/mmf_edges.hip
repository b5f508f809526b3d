// mmf_edges.hip — threshold edge builder over a dense [n,n] similarity (row a4 of SURVEY.md §8).
//
//  * lower median of the n(n-1) off-diagonal entries: 4-pass 8-bit radix select on the
//    order-preserving integer image of the floats; HBM-bound (4 reads of K), no sort, no copy.
//    Replaces: K[~eye] gather + torch.median, build_hypergraph/similarity_kernel.py:183-186.
//  * row-major stream compaction of the entries that are NOT below the threshold (self loops
//    kept): count per row -> exclusive scan -> ordered fill with wave ballots.
//    Replaces: the Python double loop with .item(), build_hypergraph/similarity_kernel.py:193-202.
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// a first-row index no column can reach: switches the diagonal skip off (flat arrays, rectangular panels)
constexpr int64_t kNoDiagonal = -(int64_t(1) << 62);
int64_t median_no_diagonal_row() { return kNoDiagonal; }

// The histogram of a pass exists in 16 copies (a workgroup adds to copy blockIdx % 16): similarities are concentrated, so
// every workgroup ends with the same one or two non-empty bins, and thousands of atomics on ONE address queue up at the
// L2 (30 us per pass over 36 MB, measured); the pick sums the copies.
constexpr int kHistCopies = 16;
struct MedianState {
  unsigned long long hist[kHistCopies][256];
  unsigned long long prefix;
  unsigned long long rank;
};

__global__ __launch_bounds__(256) void median_init_kernel(MedianState* st, unsigned long long rank) {
  for (int c = 0; c < kHistCopies; ++c) st->hist[c][threadIdx.x] = 0ull;
  if (threadIdx.x == 0) { st->prefix = 0ull; st->rank = rank; }
}

// One radix pass: histogram of byte (shift) over the entries whose higher bytes equal the prefix found so far.
// A workgroup walks whole rows (no per-element division), 16 bytes per lane when n % 4 == 0.  Similarities are
// concentrated — in the first passes nearly every entry lands in one or two bins — so a lane counts runs of equal
// bins in a register and touches the LDS histogram only when the bin changes.
// K: rows [row0, row0 + rows) of the n x n matrix (row0 = 0, rows = n: all of it).
__global__ __launch_bounds__(256) void median_hist_kernel(const float* __restrict__ K, int64_t n, int64_t row0, int64_t rows,
                                                          MedianState* st, int shift) {
  __shared__ unsigned int lh[256];
  lh[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t prefix = (uint32_t)st->prefix;
  const uint32_t himask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
  const uint32_t want = prefix & himask;
  uint32_t cur = 0xffffffffu, run = 0;
  auto feed = [&](float v) {
    const uint32_t o = f2ord(v);
    if ((o & himask) != want) return;
    const uint32_t bin = (o >> shift) & 255u;
    if (bin == cur) { ++run; return; }
    if (run) atomicAdd(&lh[cur], run);
    cur = bin; run = 1;
  };
  const bool vec = ((n & 3) == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0);
  for (int64_t li = blockIdx.x; li < rows; li += gridDim.x) {
    const float* row = K + li * n;
    const int64_t i = row0 + li;                       // global row: its diagonal entry is skipped
    if (vec) {
      for (int64_t j = (int64_t)threadIdx.x * 4; j < n; j += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j + e != i) feed(v[e]);
      }
    } else {
      for (int64_t j = threadIdx.x; j < n; j += 256)
        if (j != i) feed(row[j]);
    }
  }
  if (run) atomicAdd(&lh[cur], run);
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&st->hist[blockIdx.x % kHistCopies][threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

// the bin that holds the wanted rank: 256 threads, inclusive scan of the histogram in LDS
__global__ __launch_bounds__(256) void median_pick_kernel(MedianState* st, int shift, float* out) {
  __shared__ unsigned long long cum[256];
  const int t = threadIdx.x;
  unsigned long long mine = 0ull;
  for (int c = 0; c < kHistCopies; ++c) { mine += st->hist[c][t]; st->hist[c][t] = 0ull; }
  cum[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long v = (t >= o) ? cum[t - o] : 0ull;
    __syncthreads();
    cum[t] += v;
    __syncthreads();
  }
  const unsigned long long r = st->rank;
  const unsigned long long before = cum[t] - mine;
  // the first bin whose inclusive count exceeds the rank (bin 255 if none does: the serial loop's behaviour)
  const bool here = (r >= before && r < cum[t]) || (t == 255 && r >= cum[255]);
  __syncthreads();
  if (here) {
    st->rank = r - before;
    st->prefix = st->prefix | ((unsigned long long)t << shift);
    if (shift == 0) *out = ord2f((uint32_t)st->prefix);
  }
}

int launch_offdiag_lower_median(const float* K, int64_t n, float* out, void* scratch /* median_scratch_bytes(n (n - 1)) */,
                                hipStream_t s) {
  const unsigned long long count = (unsigned long long)n * (unsigned long long)(n - 1);
  return lower_median_of(
      count, [&](float* sample, int sc) { return launch_sample_gather(K, n, count, sample, sc, s); },
      [&](const MedianConsume& consume) { return consume(K, n, 0, n); }, out, scratch, s);
}

// The same radix select in pieces, for matrices that are recomputed panel by panel instead of stored:
// begin; then for pass 0..3 { accumulate every panel; next }.  `out` is written by next(pass 3).
int launch_median_begin_count(void* state, unsigned long long cnt, hipStream_t s) {
  hipLaunchKernelGGL(median_init_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<MedianState*>(state), (cnt - 1) / 2);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_median_accumulate(const float* K, int64_t n, int64_t row0, int64_t rows, void* state, int pass, hipStream_t s) {
  if (rows <= 0) return MMF_OK;
  int64_t grid = rows < 2048 ? rows : 2048;          // workgroups take whole rows (fewer workgroups: fewer same-address atomics at the end)
  hipLaunchKernelGGL(median_hist_kernel, dim3((unsigned)grid), dim3(256), 0, s, K, n, row0, rows,
                     reinterpret_cast<MedianState*>(state), 24 - 8 * pass);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_median_next(void* state, int pass, float* out, hipStream_t s) {
  hipLaunchKernelGGL(median_pick_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<MedianState*>(state), 24 - 8 * pass, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// ------------------------------------------------------------------------------------------------
// Lower median in ONE sweep over the data (instead of four): a sampled bracket, verified by exact counts.
//
//  1. 32768 entries at hashed positions (uniform over the population, so its quantiles are unbiased whatever the
//     row / column structure of the matrix) go through an in-LDS radix select that returns the sample's quantiles at
//     0.5 -+ 1.66 % (six standard deviations of a sample quantile): the bracket [lo, hi].
//  2. The sweep counts the entries below lo and appends the entries inside [lo, hi] (about 3.3 % of them) to a buffer:
//     a wave compacts its hits through a private LDS stage (ballot ranks, no atomics) and reserves buffer space with one
//     atomicAdd per ~800 entries.
//  3. If  below <= rank < below + inside  (and the buffer held everything), the median is the entry of rank
//     rank - below among the buffered values: a radix select over 3 % of the data.  The result is EXACT — the sample
//     only chose where to look.  Otherwise (an unlucky bracket, or so many equal values that the buffer overflows) the
//     caller falls back to the four-pass radix select; both give the same value.
// The sweep reads the data once, so the matrices that are recomputed panel by panel (mmf_combined_offdiag_median,
// mmf_sim_dense_stats without an output) are recomputed once instead of four times.
// ------------------------------------------------------------------------------------------------
constexpr int kBracketSample = 32768;
constexpr int kBracketHalfWidth = 544;          // ranks either side of the sample's middle: 3 sqrt(32768)

constexpr int kBracketSegs = 64;                 // the buffer is 64 segments with a cursor each: waves that reserve space do not
constexpr int kBracketPad = 16;                  //   queue up on ONE address (cursors and below-counters sit 128 B apart)
struct BracketState {
  unsigned long long rank, seg_cap, inside, pad0;
  float lo, hi;
  uint32_t fail, pad;
  MedianState sel;                               // radix select inside the buffer
  unsigned long long cursor[kBracketSegs * kBracketPad];
  unsigned long long below[kBracketSegs * kBracketPad];
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {      // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// sample entry i of a stored array: flat (n_sq == 0: `count` values) or the off-diagonal of an n_sq x n_sq matrix
__global__ __launch_bounds__(256) void sample_gather_kernel(const float* __restrict__ data, int64_t n_sq, unsigned long long count,
                                                            int s, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= s) return;
  const unsigned long long idx = mix64((unsigned long long)i) % count;
  if (n_sq == 0) { out[i] = data[idx]; return; }
  const unsigned long long r = idx / (unsigned long long)(n_sq - 1);
  unsigned long long c = idx - r * (unsigned long long)(n_sq - 1);
  c += (c >= r) ? 1ull : 0ull;
  out[i] = data[r * (unsigned long long)n_sq + c];
}

// sample entry i of a matrix that is NOT stored: exp(-lambda |a_r - b_c|^2) [* exp(-lambda_g |p_r - p_c|^2)] of a hashed
// pair, one wave per pair, lanes across k (not the canonical chain: the sample only places the bracket).
// offdiag != 0: A == B, pairs (r, c) with r != c.
__global__ __launch_bounds__(256) void sample_pairs_kernel(const void* __restrict__ A, const void* __restrict__ B, int64_t nb, int64_t d,
                                                           int dtype, float neg_lambda, const float* __restrict__ P, int dp,
                                                           float neg_lambda_g, int offdiag, unsigned long long count, int s,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= s) return;
  const unsigned long long idx = mix64((unsigned long long)i) % count;
  const unsigned long long per = (unsigned long long)(offdiag ? nb - 1 : nb);
  const unsigned long long r = idx / per;
  unsigned long long c = idx - r * per;
  if (offdiag) c += (c >= r) ? 1ull : 0ull;
  float acc = 0.0f;
  for (int64_t k = lane; k < d; k += 64) {
    const float t = ld_elem(A, (int64_t)r * d + k, dtype) - ld_elem(B, (int64_t)c * d + k, dtype);
    acc = __builtin_fmaf(t, t, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    float v = expf(neg_lambda * acc);
    if (P) {
      float g = 0.0f;
      for (int e = 0; e < dp; ++e) { const float t = P[r * dp + e] - P[c * dp + e]; g = __builtin_fmaf(t, t, g); }
      v *= expf(neg_lambda_g * g);
    }
    out[i] = v;
  }
}

// one workgroup: the sample's order statistics r_lo and r_hi by radix select out of LDS -> the bracket; state reset.
// A thread owns every 1024th key and counts runs of equal bins in a register (similarities are concentrated: without
// that the first passes are 32768 atomics on one LDS word).
__global__ __launch_bounds__(1024) void bracket_bounds_kernel(const float* __restrict__ sample, int s, int r_lo, int r_hi,
                                                              unsigned long long rank, unsigned long long seg_cap, BracketState* st) {
  extern __shared__ uint32_t bkeys[];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int cum[256];
  __shared__ uint32_t sh_prefix;
  __shared__ int sh_rank;
  const int tid = threadIdx.x;
  for (int i = tid; i < s; i += 1024) bkeys[i] = f2ord(sample[i]);
  for (int i = tid; i < kBracketSegs * kBracketPad; i += 1024) { st->cursor[i] = 0ull; st->below[i] = 0ull; }
  uint32_t found[2] = {0u, 0u};
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
    if (tid == 0) { sh_prefix = 0u; sh_rank = which ? r_hi : r_lo; }
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const uint32_t prefix = sh_prefix;
      const uint32_t himask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
      uint32_t cur = 0xffffffffu, run = 0u;
      for (int i = tid; i < s; i += 1024) {        // interleaved ownership: conflict-free LDS reads
        const uint32_t k = bkeys[i];
        if ((k & himask) != (prefix & himask)) continue;
        const uint32_t bin = (k >> shift) & 255u;
        if (bin == cur) { ++run; continue; }
        if (run) atomicAdd(&hist[cur], run);
        cur = bin; run = 1u;
      }
      if (run) atomicAdd(&hist[cur], run);
      __syncthreads();
      if (tid < 256) cum[tid] = hist[tid];
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {
        unsigned int v = 0u;
        if (tid < 256 && tid >= o) v = cum[tid - o];
        __syncthreads();
        if (tid < 256) cum[tid] += v;
        __syncthreads();
      }
      if (tid < 256) {
        const unsigned int r = (unsigned int)sh_rank, before = cum[tid] - hist[tid];
        if ((r >= before && r < cum[tid]) || (tid == 255 && r >= cum[255])) {
          sh_rank = (int)(r - before);
          sh_prefix = prefix | ((uint32_t)tid << shift);
        }
      }
      __syncthreads();
    }
    found[which] = sh_prefix;
  }
  if (tid == 0) {
    st->lo = ord2f(found[0]); st->hi = ord2f(found[1]);
    st->rank = rank; st->seg_cap = seg_cap; st->inside = 0ull; st->fail = 0u; st->pad = 0u;
  }
}

struct StatPartial { double s1, s2; float mn, mx; };

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}


// K: rows [row0, row0 + rows) of a matrix with n columns; the entry (row0 + li, j == row0 + li) is skipped (pass
// kNoDiagonal as row0 for data without a diagonal).  One wave per row, 16 bytes per lane when n % 4 == 0.
// part != NULL: the sweep also leaves the workgroup's statistic partial (sums around pivot[0], minimum, maximum) over the entries
// it visits — mmf_array_stats then reads its array once instead of twice.
//
// CARRY (mmf_stream_stats.hip): K is a run of rows out of a longer array that one launch of `ln.grid` workgroups
// would sweep — row li here is row ln.row0 + li there — and this launch stands in for that one on these rows.  Workgroup
// blockIdx.x acts as workgroup (ln.block0 + blockIdx.x) % ln.grid of it and takes the rows that one would take; every lane
// starts from the running (s1, s2, min, max) its counterpart left in `ln` and puts it back, so over all the runs a lane adds the
// same values in the same order as in the one launch.  No partial is written: stat_lanes_finish_kernel reduces the lanes once.
struct StatLanes {
  double* s1; double* s2; float* mn; float* mx;      // [grid * 256]
  int64_t grid, row0, block0;
};

static StatLanes stat_lanes_of(void* lanes, int64_t grid, int64_t row0, int64_t block0);

template <bool CARRY>
__global__ __launch_bounds__(256) void bracket_sweep_kernel(const float* __restrict__ K, int64_t n, int64_t row0, int64_t rows,
                                                            BracketState* st, float* __restrict__ buf, StatPartial* __restrict__ part,
                                                            const float* __restrict__ pivot, StatLanes ln) {
  __shared__ float stage[4][1024];
  __shared__ unsigned long long wbelow[4];
  __shared__ StatPartial wstat[4];
  const bool stats = CARRY || part;
  const double pv = stats ? (double)pivot[0] : 0.0;
  double s1 = 0.0, s2 = 0.0;
  float smn = __builtin_huge_valf(), smx = -__builtin_huge_valf();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t li = (int64_t)blockIdx.x * 4 + w, step = (int64_t)gridDim.x * 4;
  int64_t slot = 0;
  if constexpr (CARRY) {
    const int64_t lb = (ln.block0 + (int64_t)blockIdx.x) % ln.grid;
    slot = lb * 256 + threadIdx.x;
    s1 = ln.s1[slot]; s2 = ln.s2[slot]; smn = ln.mn[slot]; smx = ln.mx[slot];
    step = ln.grid * 4;
    const int64_t first = lb * 4 + w;                 // the wave's rows of the long array: first, first + step, ...
    const int64_t skip = ln.row0 > first ? (ln.row0 - first + step - 1) / step : 0;
    li = first + skip * step - ln.row0;
  }
  const float lo = st->lo, hi = st->hi;
  const unsigned long long seg_cap = st->seg_cap;
  const int seg = (int)((blockIdx.x * 4u + (unsigned)w) % (unsigned)kBracketSegs);
  float* sbuf = buf + (size_t)seg * seg_cap;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned long long below = 0ull;
  int cnt = 0;                                   // wave-uniform: entries waiting in this wave's stage
  auto flush = [&]() {
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(&st->cursor[seg * kBracketPad], (unsigned long long)cnt);
    base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), 0) << 32) | (unsigned long long)(uint32_t)__shfl((int)(uint32_t)base, 0);
    for (int i = lane; i < cnt; i += 64)
      if (base + (unsigned long long)i < seg_cap) sbuf[base + (unsigned long long)i] = stage[w][i];
    cnt = 0;
  };
  auto offer = [&](float x, bool valid) {
    const bool in = valid && x >= lo && x <= hi;
    below += (valid && x < lo) ? 1ull : 0ull;
    if (stats && valid) {
      const double dx = (double)x - pv;
      s1 += dx; s2 = __builtin_fma(dx, dx, s2);
      smn = fminf(smn, x); smx = fmaxf(smx, x);
    }
    const unsigned long long mask = __ballot(in);
    if (in) stage[w][cnt + __popcll(mask & lt)] = x;
    cnt += __popcll(mask);
  };
  const bool vec = ((n & 3) == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0);
  for (; li < rows; li += step) {
    const float* row = K + li * n;
    const int64_t i = row0 + li;
    if (vec) {
      for (int64_t j0 = 0; j0 < n; j0 += 256) {          // wave-uniform trip count: the ballots see every lane
        const int64_t j = j0 + (int64_t)lane * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < n) v = *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) offer(v[e], j < n && j + e != i);
        if (cnt > 1024 - 256) flush();
      }
    } else {
      for (int64_t j0 = 0; j0 < n; j0 += 64) {
        const int64_t j = j0 + lane;
        offer(j < n ? row[j] : 0.0f, j < n && j != i);
        if (cnt > 1024 - 64) flush();
      }
    }
  }
  if (cnt > 0) flush();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long hi32 = (unsigned long long)(uint32_t)__shfl_xor((int)(below >> 32), o);
    const unsigned long long lo32 = (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)below, o);
    below += (hi32 << 32) | lo32;
  }
  if constexpr (CARRY) {
    ln.s1[slot] = s1; ln.s2[slot] = s2; ln.mn[slot] = smn; ln.mx[slot] = smx;
  } else if (part) {
    s1 = wave_sum(s1); s2 = wave_sum(s2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { smn = fminf(smn, __shfl_xor(smn, o)); smx = fmaxf(smx, __shfl_xor(smx, o)); }
    if (lane == 0) wstat[w] = StatPartial{s1, s2, smn, smx};
  }
  if (lane == 0) wbelow[w] = below;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = wbelow[0] + wbelow[1] + wbelow[2] + wbelow[3];
    if (t) atomicAdd(&st->below[(blockIdx.x % (unsigned)kBracketSegs) * kBracketPad], t);
    if (!CARRY && part) {
      StatPartial r = wstat[0];
      for (int i = 1; i < 4; ++i) { r.s1 += wstat[i].s1; r.s2 += wstat[i].s2; r.mn = fminf(r.mn, wstat[i].mn); r.mx = fmaxf(r.mx, wstat[i].mx); }
      part[blockIdx.x] = r;
    }
  }
}

// does the bracket hold the wanted rank?  sets up the select inside the buffer
__global__ __launch_bounds__(64) void bracket_begin_kernel(BracketState* st) {
  const int t = threadIdx.x;
  unsigned long long c = st->cursor[t * kBracketPad], b = st->below[t * kBracketPad];
  const bool over = c > st->seg_cap;
  unsigned long long hi32, lo32;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi32 = (unsigned long long)(uint32_t)__shfl_xor((int)(c >> 32), o); lo32 = (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)c, o);
    c += (hi32 << 32) | lo32;
    hi32 = (unsigned long long)(uint32_t)__shfl_xor((int)(b >> 32), o); lo32 = (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)b, o);
    b += (hi32 << 32) | lo32;
  }
  const bool any_over = __any(over);
  for (int c = 0; c < kHistCopies; ++c)
    for (int i = t; i < 256; i += 64) st->sel.hist[c][i] = 0ull;
  if (t == 0) {
    const bool ok = !any_over && st->rank >= b && (st->rank - b) < c;
    st->fail = ok ? 0u : 1u;
    st->inside = c;
    st->sel.prefix = 0ull;
    st->sel.rank = ok ? (st->rank - b) : 0ull;
  }
}

// one radix pass over the buffered values: workgroup -> (segment, slice of it); runs of equal bins counted in a register
__global__ __launch_bounds__(256) void bracket_hist_kernel(const float* __restrict__ buf, BracketState* st, int shift) {
  __shared__ unsigned int lh[256];
  lh[threadIdx.x] = 0u;
  __syncthreads();
  if (st->fail == 0u) {
    const int seg = blockIdx.x % kBracketSegs, part = blockIdx.x / kBracketSegs, parts = gridDim.x / kBracketSegs;
    const unsigned long long count = st->cursor[seg * kBracketPad];
    const float* sbuf = buf + (size_t)seg * st->seg_cap;
    const uint32_t prefix = (uint32_t)st->sel.prefix;
    const uint32_t himask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
    uint32_t cur = 0xffffffffu, run = 0u;
    for (unsigned long long i = (unsigned long long)part * 256 + threadIdx.x; i < count; i += (unsigned long long)parts * 256) {
      const uint32_t o = f2ord(sbuf[i]);
      if ((o & himask) != (prefix & himask)) continue;
      const uint32_t bin = (o >> shift) & 255u;
      if (bin == cur) { ++run; continue; }
      if (run) atomicAdd(&lh[cur], run);
      cur = bin; run = 1u;
    }
    if (run) atomicAdd(&lh[cur], run);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&st->sel.hist[blockIdx.x % kHistCopies][threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

__global__ void bracket_report_kernel(const BracketState* st, uint32_t* flag) { *flag = st->fail; }

size_t bracket_state_bytes() { return (sizeof(BracketState) + 255) & ~size_t(255); }
// buffer entries for a population of `count` (0: the one-sweep path is not used — small or enormous populations)
unsigned long long bracket_capacity(unsigned long long count) {
  if (getenv("MMF_MEDIAN_RADIX")) return 0ull;                   // A/B switch: always the four-pass select
  if (count < (1ull << 22)) return 0ull;
  unsigned long long cap = count / 20ull + 65536ull;             // 5 %: the bracket holds 3.3 % in expectation
  cap = (cap + kBracketSegs * 64 - 1) / (kBracketSegs * 64) * (kBracketSegs * 64);   // 64 segments of whole 256-byte lines
  if (cap * 4ull > (2ull << 30)) return 0ull;
  return cap;
}
size_t median_scratch_bytes(unsigned long long count) {
  return bracket_state_bytes() + kBracketSample * sizeof(float) + 256 + (size_t)bracket_capacity(count) * sizeof(float) + 256 +
         ((sizeof(MedianState) + 255) & ~size_t(255));
}

// out (device): the lower median of `count` values — torch.median's element (count - 1) / 2.
//   sampler(sample, s): fills s sample values (device);  sweep(consume): streams the whole population once through
//   consume(data, cols, row0, rows) (row0: global row of the first row for the diagonal skip, or kNoDiagonalRow).
// One host synchronisation (the bracket's verdict) when the one-sweep path is taken.
// stat_part / stat_pivot / stat_nparts (optional): the one-sweep path leaves statistic partials of the population there (one per
// workgroup of every sweep launch, *stat_nparts of them); *stat_nparts stays 0 when the sweep did not run.
// carry (optional, with stat_part): the sweep hands over a long array of rows in runs (SweepCarry, mmf_host.h) and the partials
// are those of ONE launch over all of it.
int lower_median_of(unsigned long long count, const MedianSampler& sampler, const MedianSweep& sweep, float* out, void* scratch,
                    hipStream_t s, void* stat_part, const float* stat_pivot, int64_t* stat_nparts, SweepCarry* carry) {
  if (stat_nparts) *stat_nparts = 0;
  int64_t parts_used = 0;
  char* base = static_cast<char*>(scratch);
  BracketState* st = reinterpret_cast<BracketState*>(base);
  float* sample = reinterpret_cast<float*>(base + bracket_state_bytes());
  const unsigned long long cap = bracket_capacity(count);
  float* buf = sample + kBracketSample + 64;
  void* radix = reinterpret_cast<char*>(buf) + (((size_t)cap * sizeof(float) + 255) & ~size_t(255));
  const unsigned long long rank = (count - 1ull) / 2ull;
  if (cap != 0ull) {
    MMF_TRY(sampler(sample, kBracketSample));
    MMF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bracket_bounds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kBracketSample * 4));
    hipLaunchKernelGGL(bracket_bounds_kernel, dim3(1), dim3(1024), kBracketSample * 4, s, sample, kBracketSample,
                       kBracketSample / 2 - kBracketHalfWidth, kBracketSample / 2 + kBracketHalfWidth, rank, cap / kBracketSegs, st);
    MMF_LAUNCH_CHECK();
    bool carry_tail = false;
    if (carry && stat_part) MMF_TRY(launch_stat_lanes_init(carry->lanes, carry->grid, s));
    MMF_TRY(sweep([&](const float* data, int64_t cols, int64_t row0, int64_t rows) -> int {
      if (rows <= 0) return MMF_OK;
      if (carry && stat_part) {
        if (carry->row0 >= 0) {                        // a run of whole rows: the workgroups of the one launch that own some of them
          const int64_t w0 = carry->row0 % (carry->grid * 4);
          int64_t nb = (w0 % 4 + rows + 3) / 4;
          if (nb > carry->grid) nb = carry->grid;
          const StatLanes ln = stat_lanes_of(carry->lanes, carry->grid, carry->row0, w0 / 4);
          hipLaunchKernelGGL(bracket_sweep_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, data, cols, row0, rows, st, buf,
                             (StatPartial*)nullptr, stat_pivot, ln);
          MMF_LAUNCH_CHECK();
          return MMF_OK;
        }
        // the ragged last row: the launch of one workgroup it has in the plain sweep, its partial behind the others
        if (rows != 1 || carry_tail) { set_error("median sweep: a carried sweep has one ragged last row"); return MMF_E_INTERNAL; }
        hipLaunchKernelGGL(bracket_sweep_kernel<false>, dim3(1), dim3(256), 0, s, data, cols, row0, rows, st, buf,
                           reinterpret_cast<StatPartial*>(stat_part) + carry->grid, stat_pivot, StatLanes{});
        MMF_LAUNCH_CHECK();
        carry_tail = true;
        return MMF_OK;
      }
      int64_t grid = (rows + 3) / 4;
      if (grid > (stat_part ? 2040 : 2048)) grid = stat_part ? 2040 : 2048;     // a ragged last row adds one launch of one workgroup
      StatPartial* sp = stat_part ? reinterpret_cast<StatPartial*>(stat_part) + parts_used : nullptr;
      if (sp && parts_used + grid > 2048) { set_error("median sweep: more than 2048 statistic partials"); return MMF_E_INTERNAL; }
      hipLaunchKernelGGL(bracket_sweep_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, data, cols, row0, rows, st, buf, sp, stat_pivot,
                         StatLanes{});
      MMF_LAUNCH_CHECK();
      if (sp) parts_used += grid;
      return MMF_OK;
    }));
    if (carry && stat_part) {
      MMF_TRY(launch_stat_lanes_finish(carry->lanes, carry->grid, stat_part, s));
      parts_used = carry->grid + (carry_tail ? 1 : 0);
    }
    if (stat_nparts) *stat_nparts = parts_used;
    hipLaunchKernelGGL(bracket_begin_kernel, dim3(1), dim3(64), 0, s, st);
    MMF_LAUNCH_CHECK();
    MedianState* sel = &st->sel;
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(bracket_hist_kernel, dim3(16 * kBracketSegs), dim3(256), 0, s, buf, st, 24 - 8 * pass);
      MMF_LAUNCH_CHECK();
      hipLaunchKernelGGL(median_pick_kernel, dim3(1), dim3(256), 0, s, sel, 24 - 8 * pass, out);
      MMF_LAUNCH_CHECK();
    }
    uint32_t h_fail = 1;
    MMF_HIP(hipMemcpyAsync(&h_fail, &st->fail, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MMF_HIP(hipStreamSynchronize(s));
    if (h_fail == 0u) return MMF_OK;
  }
  // four-pass radix select over the whole population
  MMF_TRY(launch_median_begin_count(radix, count, s));
  for (int pass = 0; pass < 4; ++pass) {
    MMF_TRY(sweep([&](const float* data, int64_t cols, int64_t row0, int64_t rows) -> int {
      return launch_median_accumulate(data, cols, row0, rows, radix, pass, s);
    }));
    MMF_TRY(launch_median_next(radix, pass, out, s));
  }
  return MMF_OK;
}

int launch_sample_gather(const float* data, int64_t n_sq, unsigned long long count, float* sample, int s_count, hipStream_t s) {
  hipLaunchKernelGGL(sample_gather_kernel, dim3((unsigned)((s_count + 255) / 256)), dim3(256), 0, s, data, n_sq, count, s_count, sample);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_sample_pairs(const void* A, const void* B, int64_t nb, int64_t d, int dtype, float lambda, const float* P, int dp,
                        float lambda_g, int offdiag, unsigned long long count, float* sample, int s_count, hipStream_t s) {
  hipLaunchKernelGGL(sample_pairs_kernel, dim3((unsigned)((s_count + 3) / 4)), dim3(256), 0, s, A, B, nb, d, dtype, -lambda, P, dp,
                     -lambda_g, offdiag, count, s_count, sample);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// flat array as rows of 4096 values plus one ragged row
static int sweep_flat(const float* v, int64_t count, const MedianConsume& consume) {
  const int64_t C = 4096, full = count / C, tail = count - full * C;
  if (full > 0) MMF_TRY(consume(v, C, kNoDiagonal, full));
  if (tail > 0) MMF_TRY(consume(v + full * C, tail, kNoDiagonal, 1));
  return MMF_OK;
}

// Lower median (torch.median semantics: element (count - 1) / 2 of the sorted values) of a flat array — the
// similarity statistics of preprocess_hypergraph.py:190-196, 259-265 and the edge-weight median of :885-897.
// The array is walked as rows of 4096 values (plus one ragged row) by the same histogram kernel; a row0 that no
// column index can reach switches the diagonal skip off.
int launch_lower_median(const float* v, int64_t count, float* out, void* scratch /* median_scratch_bytes(count) */, hipStream_t s) {
  return lower_median_of(
      (unsigned long long)count, [&](float* sample, int sc) { return launch_sample_gather(v, 0, (unsigned long long)count, sample, sc, s); },
      [&](const MedianConsume& consume) { return sweep_flat(v, count, consume); }, out, scratch, s);
}

// ------------------------------------------------------------------------------------------------
// mean / std / min / max of a flat f32 array in ONE pass (f64 accumulation around a pivot), deterministic:
// every workgroup writes its partial, one workgroup merges them in index order.
// Replaces: K.mean(), K.std(), K.min(), K.max() — four passes — at preprocess_hypergraph.py:190-195, 260-263.
// ------------------------------------------------------------------------------------------------
//
// CARRY (mmf_stream_stats.hip): v is a run out of a longer 16-byte aligned array that one launch of `ln.grid`
// workgroups would reduce: ln.row0 is the index there of this run's first group of four values, `count` the run's length, and
// the run ends either on a group boundary or at the end of the array (then its last count % 4 values are the array's scalar
// tail).  Thread t here acts as thread (ln.block0 * 256 + t) % (ln.grid * 256) of that launch, takes the groups it would take,
// starts from the lane's running sums in `ln` and puts them back; pivot[0] is the array's first value.
template <bool CARRY>
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ v, int64_t count, StatPartial* __restrict__ part,
                                                            const float* __restrict__ pivot, StatLanes ln) {
  const double p = CARRY ? (double)pivot[0] : (double)v[0];   // pivot: sums of (x - p) stay small when the values cluster
  double s1 = 0.0, s2 = 0.0;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  auto feed = [&](float x) {
    const double dx = (double)x - p;
    s1 += dx; s2 = __builtin_fma(dx, dx, s2);
    mn = fminf(mn, x); mx = fmaxf(mx, x);
  };
  if constexpr (CARRY) {
    const int64_t nth = ln.grid * 256;
    const int64_t tid = ((ln.block0 + (int64_t)blockIdx.x) % ln.grid) * 256 + threadIdx.x;
    s1 = ln.s1[tid]; s2 = ln.s2[tid]; mn = ln.mn[tid]; mx = ln.mx[tid];
    const int64_t n4 = count >> 2;
    const int64_t skip = ln.row0 > tid ? (ln.row0 - tid + nth - 1) / nth : 0;
    const bool vec = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
    for (int64_t i = tid + skip * nth - ln.row0; i < n4; i += nth) {
      if (vec) {
        const f32x4 x = reinterpret_cast<const f32x4*>(v)[i];
        feed(x[0]); feed(x[1]); feed(x[2]); feed(x[3]);
      } else {
        const float x0 = v[4 * i], x1 = v[4 * i + 1], x2 = v[4 * i + 2], x3 = v[4 * i + 3];
        feed(x0); feed(x1); feed(x2); feed(x3);
      }
    }
    if (n4 * 4 + tid < count) feed(v[n4 * 4 + tid]);     // the array's scalar tail: threads 0 .. 2 of the one launch
    ln.s1[tid] = s1; ln.s2[tid] = s2; ln.mn[tid] = mn; ln.mx[tid] = mx;
    return;
  }
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(v) & 15) == 0) ? (count >> 2) : 0;
  for (int64_t i = tid; i < n4; i += nth) {
    const f32x4 x = reinterpret_cast<const f32x4*>(v)[i];
    feed(x[0]); feed(x[1]); feed(x[2]); feed(x[3]);
  }
  for (int64_t i = n4 * 4 + tid; i < count; i += nth) feed(v[i]);
  s1 = wave_sum(s1); s2 = wave_sum(s2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  __shared__ StatPartial w[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) w[wave] = StatPartial{s1, s2, mn, mx};
  __syncthreads();
  if (threadIdx.x == 0) {
    StatPartial r = w[0];
    for (int i = 1; i < 4; ++i) { r.s1 += w[i].s1; r.s2 += w[i].s2; r.mn = fminf(r.mn, w[i].mn); r.mx = fmaxf(r.mx, w[i].mx); }
    part[blockIdx.x] = r;
  }
}

// The lanes of a carried launch (StatLanes): every lane at the state it has before it adds its first value, and the end both
// producers share — wave butterflies, then the workgroup's four waves in order — once the last run has been added.
__global__ __launch_bounds__(256) void stat_lanes_init_kernel(StatLanes ln) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  ln.s1[i] = 0.0; ln.s2[i] = 0.0; ln.mn[i] = __builtin_huge_valf(); ln.mx[i] = -__builtin_huge_valf();
}

__global__ __launch_bounds__(256) void stat_lanes_finish_kernel(StatLanes ln, StatPartial* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double s1 = ln.s1[i], s2 = ln.s2[i];
  float mn = ln.mn[i], mx = ln.mx[i];
  s1 = wave_sum(s1); s2 = wave_sum(s2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  __shared__ StatPartial w[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) w[wave] = StatPartial{s1, s2, mn, mx};
  __syncthreads();
  if (threadIdx.x == 0) {
    StatPartial r = w[0];
    for (int k = 1; k < 4; ++k) { r.s1 += w[k].s1; r.s2 += w[k].s2; r.mn = fminf(r.mn, w[k].mn); r.mx = fmaxf(r.mx, w[k].mx); }
    part[blockIdx.x] = r;
  }
}

// out[0..3] = mean, std (unbiased, as torch.std), min, max; out[4] is the median's slot.  pivot[0]: the value the
// partial sums were taken around.
__device__ __forceinline__ void stats_final_body(const float* __restrict__ pivot, int64_t count, const StatPartial* __restrict__ part,
                                                 int64_t nparts, double* __restrict__ out) {
  __shared__ StatPartial w[256];
  StatPartial r{0.0, 0.0, __builtin_huge_valf(), -__builtin_huge_valf()};
  for (int64_t i = threadIdx.x; i < nparts; i += 256) {   // fixed assignment, fixed order: bit-reproducible
    r.s1 += part[i].s1; r.s2 += part[i].s2; r.mn = fminf(r.mn, part[i].mn); r.mx = fmaxf(r.mx, part[i].mx);
  }
  w[threadIdx.x] = r;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      w[threadIdx.x].s1 += w[threadIdx.x + o].s1; w[threadIdx.x].s2 += w[threadIdx.x + o].s2;
      w[threadIdx.x].mn = fminf(w[threadIdx.x].mn, w[threadIdx.x + o].mn); w[threadIdx.x].mx = fmaxf(w[threadIdx.x].mx, w[threadIdx.x + o].mx);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = (double)count, p = (double)pivot[0];
    const double mean = p + w[0].s1 / n;
    double var = (w[0].s2 - w[0].s1 * w[0].s1 / n) / (n - 1.0);   // count == 1: 0 / 0 = NaN, as torch.std
    if (var < 0.0) var = 0.0;
    out[0] = mean; out[1] = __builtin_sqrt(var); out[2] = (double)w[0].mn; out[3] = (double)w[0].mx;
  }
}

__global__ __launch_bounds__(256) void stats_final_kernel(const float* __restrict__ pivot, int64_t count, const StatPartial* __restrict__ part,
                                                          int64_t nparts, double* __restrict__ out) {
  stats_final_body(pivot, count, part, nparts, out);
}

__global__ void stats_median_kernel(const float* med, double* out) { out[4] = (double)*med; }

// segmented (mmf_sim_dense_stats_segmented): workgroup s merges the partials pbase[s] .. pbase[s+1]-1 of segment s — the same
// assignment of partials to threads, the same tree — around pivot[s] with count = n_s m_s, into out[s][0..3]
__global__ __launch_bounds__(256) void stats_final_seg_kernel(const float* __restrict__ pivot, const int64_t* __restrict__ xptr,
                                                              const int64_t* __restrict__ yptr, const StatPartial* __restrict__ part,
                                                              const int64_t* __restrict__ pbase, double* __restrict__ out) {
  const int64_t sg = blockIdx.x;
  const int64_t count = (xptr[sg + 1] - xptr[sg]) * (yptr[sg + 1] - yptr[sg]);
  stats_final_body(pivot + sg, count, part + pbase[sg], pbase[sg + 1] - pbase[sg], out + 5 * sg);
}
__global__ __launch_bounds__(256) void stats_median_seg_kernel(const float* __restrict__ med, int64_t S, double* __restrict__ out) {
  const int64_t sg = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (sg < S) out[5 * sg + 4] = (double)med[sg];
}

size_t array_stats_scratch_bytes(int64_t count) { return 2048 * sizeof(StatPartial) + 256 + median_scratch_bytes((unsigned long long)count); }

int launch_array_stats(const float* v, int64_t count, double* out, void* scratch, hipStream_t s) {
  StatPartial* part = reinterpret_cast<StatPartial*>(scratch);
  char* rest = reinterpret_cast<char*>(scratch) + 2048 * sizeof(StatPartial);
  float* med = reinterpret_cast<float*>(rest);
  void* mscratch = rest + 256;
  // large arrays: the median's one sweep also leaves the statistic partials (one read of the array instead of two)
  int64_t nparts = 0;
  MMF_TRY(lower_median_of(
      (unsigned long long)count, [&](float* sample, int sc) { return launch_sample_gather(v, 0, (unsigned long long)count, sample, sc, s); },
      [&](const MedianConsume& consume) { return sweep_flat(v, count, consume); }, med, mscratch, s, part, v, &nparts));
  if (nparts == 0) {
    int64_t grid = (count + 256 * 16 - 1) / (256 * 16);
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(stats_partial_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, v, count, part, (const float*)nullptr, StatLanes{});
    MMF_LAUNCH_CHECK();
    nparts = grid;
  }
  MMF_TRY(launch_stats_finish(part, nparts, v, count, out, s));
  return launch_stats_set_median(med, out, s);
}

// ---- statistics carried across the runs of an array that is never whole in memory (mmf_stream_stats.hip) ----
size_t stat_lanes_bytes(int64_t grid) { return 2 * ws_bytes((size_t)grid * 256, 8) + 2 * ws_bytes((size_t)grid * 256, 4); }
static StatLanes stat_lanes_of(void* lanes, int64_t grid, int64_t row0, int64_t block0) {
  char* b = static_cast<char*>(lanes);
  const size_t d8 = ws_bytes((size_t)grid * 256, 8), d4 = ws_bytes((size_t)grid * 256, 4);
  return StatLanes{reinterpret_cast<double*>(b), reinterpret_cast<double*>(b + d8), reinterpret_cast<float*>(b + 2 * d8),
                   reinterpret_cast<float*>(b + 2 * d8 + d4), grid, row0, block0};
}
int launch_stat_lanes_init(void* lanes, int64_t grid, hipStream_t s) {
  hipLaunchKernelGGL(stat_lanes_init_kernel, dim3((unsigned)grid), dim3(256), 0, s, stat_lanes_of(lanes, grid, 0, 0));
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_stat_lanes_finish(void* lanes, int64_t grid, void* part, hipStream_t s) {
  hipLaunchKernelGGL(stat_lanes_finish_kernel, dim3((unsigned)grid), dim3(256), 0, s, stat_lanes_of(lanes, grid, 0, 0),
                     reinterpret_cast<StatPartial*>(part));
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
bool median_one_sweep(unsigned long long count) { return bracket_capacity(count) != 0ull; }
int64_t stats_partial_grid(int64_t count) {
  int64_t grid = (count + 256 * 16 - 1) / (256 * 16);
  if (grid > 2048) grid = 2048;
  return grid < 1 ? 1 : grid;
}
// values v[0 .. count) = values [group0 * 4, group0 * 4 + count) of the array that stats_partial_kernel would reduce with `grid`
// workgroups; count % 4 != 0 only for the run that ends the array
int launch_stats_partial_carry(const float* v, int64_t count, int64_t group0, const float* pivot, void* lanes, int64_t grid, hipStream_t s) {
  if (count <= 0) return MMF_OK;
  const int64_t nth = grid * 256, t0 = group0 % nth;
  int64_t nb = (t0 % 256 + (count >> 2) + 255) / 256, b0 = t0 / 256;
  if (nb > grid || (count & 3)) { nb = grid; b0 = 0; }          // the scalar tail belongs to threads 0 .. 2
  hipLaunchKernelGGL(stats_partial_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, v, count, (StatPartial*)nullptr, pivot,
                     stat_lanes_of(lanes, grid, group0, b0));
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// the merge of per-workgroup partials (StatPartial: {double s1, s2; float mn, mx}) written by ANY producer kernel
int launch_stats_finish(const void* part, int64_t nparts, const float* pivot, int64_t count, double* out, hipStream_t s) {
  hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(256), 0, s, pivot, count, reinterpret_cast<const StatPartial*>(part), nparts, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_stats_set_median(const float* med, double* out, hipStream_t s) {
  hipLaunchKernelGGL(stats_median_kernel, dim3(1), dim3(1), 0, s, med, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_stats_finish_seg(const void* part, const int64_t* d_pbase, const float* pivot, const int64_t* d_xptr, const int64_t* d_yptr,
                            int64_t S, double* out, hipStream_t s) {
  hipLaunchKernelGGL(stats_final_seg_kernel, dim3((unsigned)S), dim3(256), 0, s, pivot, d_xptr, d_yptr,
                     reinterpret_cast<const StatPartial*>(part), d_pbase, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_stats_set_median_seg(const float* med, int64_t S, double* out, hipStream_t s) {
  hipLaunchKernelGGL(stats_median_seg_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, med, S, out);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
size_t stat_partial_bytes() { return sizeof(StatPartial); }

// ------------------------------------------------------------------------------------------------
// threshold edges
// ------------------------------------------------------------------------------------------------
// One wave counts the entries of row kr[0 .. n) that are not below thr (every lane returns the row's count).
// vec: n % 4 == 0 and kr 16-byte aligned.
__device__ __forceinline__ uint32_t thr_count_row(const float* __restrict__ kr, int64_t n, float thr, bool vec, int lane) {
  uint32_t c = 0;
  if (vec) {                                                                    // 16 bytes per lane, 1 KiB per wave instruction
    for (int64_t j = (int64_t)lane * 4; j < n; j += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(kr + j);
      c += (v[0] < thr ? 0u : 1u) + (v[1] < thr ? 0u : 1u) + (v[2] < thr ? 0u : 1u) + (v[3] < thr ? 0u : 1u);   // skipped iff K < thr (:198)
    }
  } else {
    for (int64_t j = lane; j < n; j += 64) c += (kr[j] < thr) ? 0u : 1u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor((int)c, o);
  return c;
}

// K: `rows` rows of n entries each (a panel of the square matrix, or all of it)
__global__ __launch_bounds__(256) void thr_count_kernel(const float* __restrict__ K, int64_t n, int64_t rows, float thr,
                                                        uint32_t* __restrict__ row_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint32_t c = thr_count_row(K + row * n, n, thr, ((n & 3) == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0), lane);
  if (lane == 0) row_cnt[row] = c;
}

// Exclusive offsets of the rows, starting at the edges already counted (*out_count on entry: 0 for a whole matrix,
// the running total when panels are processed one after the other); *out_count is advanced by this panel's edges.
__global__ __launch_bounds__(1024) void thr_scan_kernel(const uint32_t* __restrict__ row_cnt, int64_t n,
                                                        unsigned long long* __restrict__ row_off,
                                                        int64_t* __restrict__ out_count) {
  __shared__ unsigned long long part[1024];
  const unsigned long long base = (unsigned long long)*out_count;
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t b = (int64_t)t * per;
  int64_t e = b + per;
  if (e > n) e = n;
  unsigned long long sum = 0;
  for (int64_t i = b; i < e; ++i) sum += row_cnt[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    unsigned long long v = (t >= o) ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = base + ((t == 0) ? 0ull : part[t - 1]);
  for (int64_t i = b; i < e; ++i) { row_off[i] = run; run += row_cnt[i]; }
  __syncthreads();                                   // everybody has read the base
  if (t == 1023) { *out_count = (int64_t)(base + part[1023]); row_off[n] = base + part[1023]; }
}

// One wave writes the kept entries of row kr[0 .. n) from edge position pos on: (id_row, col0 + j, kr[j]), j ascending.
__device__ __forceinline__ void thr_fill_row(const float* __restrict__ kr, int64_t n, float thr, unsigned long long pos, int64_t id_row,
                                             int64_t col0, int64_t* __restrict__ ei_row, int64_t* __restrict__ ei_col,
                                             float* __restrict__ ew, int64_t capacity, int lane) {
  // Four 64-column groups per trip: the four loads are in flight together, and every store instruction writes the
  // kept entries of one group to CONSECUTIVE positions (a lane-owns-4-columns layout would make the stores strided).
  int64_t j0 = 0;
  for (; j0 + 256 <= n; j0 += 256) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = kr[j0 + 64 * u + lane];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = !(v[u] < thr);
      const unsigned long long mask = __ballot(keep);
      if (keep) {
        const unsigned long long p = pos + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
        if ((int64_t)p < capacity) { ei_row[p] = id_row; ei_col[p] = col0 + j0 + 64 * u + lane; ew[p] = v[u]; }
      }
      pos += (unsigned long long)__popcll(mask);
    }
  }
  for (; j0 < n; j0 += 64) {
    const int64_t j = j0 + lane;
    const float v = (j < n) ? kr[j] : 0.0f;
    const bool keep = (j < n) && !(v < thr);
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const unsigned long long p = pos + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
      if ((int64_t)p < capacity) { ei_row[p] = id_row; ei_col[p] = col0 + j; ew[p] = v; }
    }
    pos += (unsigned long long)__popcll(mask);
  }
}

__global__ __launch_bounds__(256) void thr_fill_kernel(const float* __restrict__ K, int64_t n, int64_t row0, int64_t rows,
                                                       float thr, const unsigned long long* __restrict__ row_off,
                                                       int64_t* __restrict__ ei_row, int64_t* __restrict__ ei_col,
                                                       float* __restrict__ ew, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  thr_fill_row(K + row * n, n, thr, row_off[row], row0 + row, 0, ei_row, ei_col, ew, capacity, lane);
}

// K: rows [row0, row0 + rows) of the n x n matrix.  Edges are written to (ei_row, ei_col, ew)[0 .. count), row-major.
int launch_threshold_edges_panel(const float* K, int64_t n, int64_t row0, int64_t rows, float thr, int64_t* ei_row,
                                 int64_t* ei_col, float* ew, int64_t capacity, int64_t* out_count, uint32_t* scratch,
                                 size_t scratch_u32, hipStream_t s) {
  if ((size_t)(2 * (rows + 1) + rows) > scratch_u32) { set_error("threshold_edges: scratch too small"); return MMF_E_INTERNAL; }
  unsigned long long* row_off = reinterpret_cast<unsigned long long*>(scratch);
  uint32_t* row_cnt = scratch + 2 * (rows + 1);
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipLaunchKernelGGL(thr_count_kernel, dim3(grid), dim3(256), 0, s, K, n, rows, thr, row_cnt);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(thr_scan_kernel, dim3(1), dim3(1024), 0, s, row_cnt, rows, row_off, out_count);
  MMF_LAUNCH_CHECK();
  if (capacity > 0) {
    hipLaunchKernelGGL(thr_fill_kernel, dim3(grid), dim3(256), 0, s, K, n, row0, rows, thr, row_off, ei_row, ei_col, ew, capacity);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

int launch_threshold_edges(const float* K, int64_t n, float thr, int64_t* ei, float* ew, int64_t capacity,
                           int64_t* out_count, uint32_t* scratch, size_t scratch_u32, hipStream_t s) {
  return launch_threshold_edges_panel(K, n, 0, n, thr, ei, ei ? ei + capacity : nullptr, ew, capacity, out_count, scratch,
                                      scratch_u32, s);
}

// The two halves of the above for a caller that sizes its outputs from the count: the counting pass leaves the rows'
// exclusive offsets (row_off[n + 1], row_off[n] = total), the fill pass takes them — K is read twice, not three times.
int launch_threshold_count(const float* K, int64_t n, float thr, unsigned long long* row_off, int64_t* out_count, uint32_t* row_cnt,
                           hipStream_t s) {
  const unsigned grid = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(thr_count_kernel, dim3(grid), dim3(256), 0, s, K, n, n, thr, row_cnt);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(thr_scan_kernel, dim3(1), dim3(1024), 0, s, row_cnt, n, row_off, out_count);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_threshold_fill(const float* K, int64_t n, float thr, const unsigned long long* row_off, int64_t* ei, float* ew,
                          int64_t capacity, hipStream_t s) {
  const unsigned grid = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(thr_fill_kernel, dim3(grid), dim3(256), 0, s, K, n, (int64_t)0, n, thr, row_off, ei, ei + capacity, ew, capacity);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}


// ------------------------------------------------------------------------------------------------
// segmented: the diagonal blocks K_s (n_s x n_s, row-major) of a ragged batch, stored one after the other from
// kptr[s] = sum_{t<s} n_t^2 (mmf_offdiag_lower_median_segmented, mmf_threshold_edges_segmented_*)
// ------------------------------------------------------------------------------------------------
// The lower median of every block's off-diagonal entries: the four-pass radix select above, one select state per segment.
// A segment's histogram lives in as many copies as the segment has histogram workgroups, at most kHistCopies (a small
// segment is one workgroup and one copy: the copies are what the pick reads and clears, S times over).
struct SegMedianHead {
  unsigned long long prefix, rank;   // as in MedianState
  unsigned long long hoff, copies;   // its copies: hist[hoff + 256 c + bin], c < copies
};
// work table of the histogram passes, one entry per workgroup: segment, first row, rows, histogram copy (flat blocks: segment,
// first element, elements, histogram copy)
enum { SMED_SEG = 0, SMED_ROW0 = 1, SMED_ROWS = 2, SMED_COPY = 3, SMED_ENTRY = 4 };
constexpr int64_t kSegMedianChunk = 65536;     // entries of a block per histogram workgroup (whole rows, at least one)

struct SegMedianPlan {
  std::vector<int64_t> tab;                    // [entries][SMED_ENTRY]
  std::vector<SegMedianHead> heads;            // [S]
  std::vector<int64_t> kptr;                   // [S + 1]
  size_t hist_words = 0;
  SegMedianPlan(const int64_t* ptr, int64_t S) : heads((size_t)S), kptr((size_t)S + 1) {
    kptr[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
      const int64_t ns = ptr[s + 1] - ptr[s];
      kptr[s + 1] = kptr[s] + ns * ns;
      int64_t rpe = kSegMedianChunk / ns;
      if (rpe < 1) rpe = 1;
      int64_t e = 0;
      for (int64_t r0 = 0; r0 < ns; r0 += rpe, ++e) {
        const int64_t ent[SMED_ENTRY] = {s, r0, ns - r0 < rpe ? ns - r0 : rpe, e % kHistCopies};
        tab.insert(tab.end(), ent, ent + SMED_ENTRY);
      }
      const unsigned long long cnt = (unsigned long long)ns * (unsigned long long)(ns - 1);
      heads[s] = SegMedianHead{0ull, (cnt - 1ull) / 2ull, hist_words, (unsigned long long)(e < kHistCopies ? e : kHistCopies)};
      hist_words += 256 * heads[s].copies;
    }
  }
  // flat blocks (mmf_lower_median_segmented): block s is the bptr[s+1] - bptr[s] >= 1 values from bptr[s], no diagonal
  struct Flat {};
  SegMedianPlan(const int64_t* bptr, int64_t S, Flat) : heads((size_t)S), kptr(bptr, bptr + S + 1) {
    for (int64_t s = 0; s < S; ++s) {
      const int64_t cs = bptr[s + 1] - bptr[s];
      int64_t e = 0;
      for (int64_t f0 = 0; f0 < cs; f0 += kSegMedianChunk, ++e) {
        const int64_t ent[SMED_ENTRY] = {s, f0, cs - f0 < kSegMedianChunk ? cs - f0 : kSegMedianChunk, e % kHistCopies};
        tab.insert(tab.end(), ent, ent + SMED_ENTRY);
      }
      heads[s] = SegMedianHead{0ull, ((unsigned long long)cs - 1ull) / 2ull, hist_words, (unsigned long long)(e < kHistCopies ? e : kHistCopies)};
      hist_words += 256 * heads[s].copies;
    }
  }
  int64_t entries() const { return (int64_t)tab.size() / SMED_ENTRY; }
  size_t bytes(int64_t S) const {
    return ws_bytes((size_t)S, sizeof(SegMedianHead)) + 2 * ws_bytes((size_t)S + 1, 8) + ws_bytes(tab.size(), 8) + ws_bytes(hist_words, 8);
  }
};

// One radix pass over the entries of ONE block (the workgroup's table entry: rows [r0, r0 + rows) of K_s) whose higher bytes
// equal the segment's prefix; the diagonal is skipped.  The rows are walked flat, one entry per thread and step, so short rows
// keep every lane busy: (i, j) of the thread's entry advance by 256 entries per step without a division.
// FLAT: the block is kptr[sg+1] - kptr[sg] values without a diagonal (ptr is not read) and the entry is elements [r0, r0 + rows):
// the same walk without the (i, j) bookkeeping.
template <bool FLAT>
__global__ __launch_bounds__(256) void seg_median_hist_kernel(const float* __restrict__ K, const int64_t* __restrict__ ptr,
                                                              const int64_t* __restrict__ kptr, const int64_t* __restrict__ tab,
                                                              SegMedianHead* __restrict__ head, unsigned long long* __restrict__ hist,
                                                              int shift) {
  __shared__ unsigned int lh[256];
  lh[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t* e = tab + (size_t)blockIdx.x * SMED_ENTRY;
  const int64_t sg = e[SMED_SEG], r0 = e[SMED_ROW0], rows = e[SMED_ROWS];
  const int64_t ns = FLAT ? 1 : ptr[sg + 1] - ptr[sg];
  const float* B = K + kptr[sg];
  const uint32_t prefix = (uint32_t)head[sg].prefix;
  const uint32_t himask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
  const uint32_t want = prefix & himask;
  uint32_t cur = 0xffffffffu, run = 0;
  auto feed = [&](float v) {
    const uint32_t o = f2ord(v);
    if ((o & himask) != want) return;
    const uint32_t bin = (o >> shift) & 255u;
    if (bin == cur) { ++run; return; }
    if (run) atomicAdd(&lh[cur], run);
    cur = bin; run = 1;
  };
  const int64_t f1 = (r0 + rows) * ns;
  int64_t f = r0 * ns + threadIdx.x;
  int64_t i = f / ns, j = f - i * ns;
  const int64_t qs = 256 / ns, rs = 256 - qs * ns;
  auto step = [&]() {
    j += rs; i += qs;
    if (j >= ns) { j -= ns; ++i; }
  };
  for (; f + 768 < f1; f += 1024) {                  // four loads in flight
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = B[f + 256 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (FLAT || i != j) feed(v[u]);
      if constexpr (!FLAT) step();
    }
  }
  for (; f < f1; f += 256) {
    if (FLAT || i != j) feed(B[f]);
    if constexpr (!FLAT) step();
  }
  if (run) atomicAdd(&lh[cur], run);
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&hist[head[sg].hoff + 256 * e[SMED_COPY] + threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

// median_pick_kernel for segment blockIdx.x: sums (and clears) its copies, picks the bin of its rank
__global__ __launch_bounds__(256) void seg_median_pick_kernel(SegMedianHead* __restrict__ head, unsigned long long* __restrict__ hist,
                                                              int shift, float* __restrict__ out) {
  __shared__ unsigned long long cum[256];
  SegMedianHead* st = head + blockIdx.x;
  const int t = threadIdx.x;
  unsigned long long* h = hist + st->hoff;
  const int copies = (int)st->copies;
  unsigned long long mine = 0ull;
  for (int c = 0; c < copies; ++c) { mine += h[256 * c + t]; h[256 * c + t] = 0ull; }
  cum[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long v = (t >= o) ? cum[t - o] : 0ull;
    __syncthreads();
    cum[t] += v;
    __syncthreads();
  }
  const unsigned long long r = st->rank;
  const unsigned long long before = cum[t] - mine;
  const bool here = (r >= before && r < cum[t]) || (t == 255 && r >= cum[255]);
  __syncthreads();
  if (here) {
    st->rank = r - before;
    st->prefix = st->prefix | ((unsigned long long)t << shift);
    if (shift == 0) out[blockIdx.x] = ord2f((uint32_t)st->prefix);
  }
}

size_t offdiag_lower_median_seg_scratch_bytes(const int64_t* ptr, int64_t S) { return SegMedianPlan(ptr, S).bytes(S); }

// out[s] (device f32 [S]): the lower median of the n_s (n_s - 1) off-diagonal entries of block s (every n_s >= 2, checked by
// the caller).  Launches: the state's upload and clear, then 4 x (histogram over all blocks, pick per segment), for any S.
template <bool FLAT>
static int run_seg_median(const float* K, const SegMedianPlan& plan, const int64_t* ptr, int64_t S, float* out, void* scratch, hipStream_t s) {
  char* p = static_cast<char*>(scratch);
  SegMedianHead* head = reinterpret_cast<SegMedianHead*>(p);
  p += ws_bytes((size_t)S, sizeof(SegMedianHead));
  int64_t* d_ptr = reinterpret_cast<int64_t*>(p);
  p += ws_bytes((size_t)S + 1, 8);
  int64_t* d_kptr = reinterpret_cast<int64_t*>(p);
  p += ws_bytes((size_t)S + 1, 8);
  int64_t* d_tab = reinterpret_cast<int64_t*>(p);
  p += ws_bytes(plan.tab.size(), 8);
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(p);
  MMF_TRY(upload_table(s, head, plan.heads.data(), (size_t)S * sizeof(SegMedianHead)));      // the plan dies with this call
  if (!FLAT) MMF_TRY(upload_table(s, d_ptr, ptr, (size_t)(S + 1) * 8));
  MMF_TRY(upload_table(s, d_kptr, plan.kptr.data(), (size_t)(S + 1) * 8));
  MMF_TRY(upload_table(s, d_tab, plan.tab.data(), plan.tab.size() * 8));
  MMF_HIP(hipMemsetAsync(hist, 0, plan.hist_words * 8, s));
  const int64_t grid = plan.entries();
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(seg_median_hist_kernel<FLAT>, dim3((unsigned)grid), dim3(256), 0, s, K, d_ptr, d_kptr, d_tab, head, hist, 24 - 8 * pass);
    MMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_median_pick_kernel, dim3((unsigned)S), dim3(256), 0, s, head, hist, 24 - 8 * pass, out);
    MMF_LAUNCH_CHECK();
  }
  return MMF_OK;
}

int launch_offdiag_lower_median_seg(const float* K, const int64_t* ptr, int64_t S, float* out, void* scratch, hipStream_t s) {
  return run_seg_median<false>(K, SegMedianPlan(ptr, S), ptr, S, out, scratch, s);
}

// The lower median of every flat block v[bptr[s] .. bptr[s+1]) (every block with at least one value, checked by the caller):
// the same select without a diagonal.  out[s] = the element of rank (c_s - 1) / 2, what mmf_lower_median returns on the block.
size_t lower_median_seg_scratch_bytes(const int64_t* bptr, int64_t S) { return SegMedianPlan(bptr, S, SegMedianPlan::Flat{}).bytes(S); }
int launch_lower_median_seg(const float* v, const int64_t* bptr, int64_t S, float* out, void* scratch, hipStream_t s) {
  return run_seg_median<true>(v, SegMedianPlan(bptr, S, SegMedianPlan::Flat{}), nullptr, S, out, scratch, s);
}

// Threshold edges of every block: row r of the batch (segment s, local row i = r - ptr[s]) is row i of K_s against
// thr[s]; its edges are (r, ptr[s] + j).  thr_scan_kernel's offsets over all n rows are then segment-major, row-major
// within a segment, and segment s's edges start at row_off[ptr[s]].
__device__ __forceinline__ int64_t seg_of_row(const int64_t* __restrict__ ptr, int64_t S, int64_t row) {
  int64_t lo = 0, hi = S - 1;                        // the last s with ptr[s] <= row: a non-empty segment
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void thr_count_seg_kernel(const float* __restrict__ K, const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ kptr, int64_t S, int64_t n,
                                                            const float* __restrict__ thr, uint32_t* __restrict__ row_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t sg = seg_of_row(ptr, S, row);
  const int64_t ns = ptr[sg + 1] - ptr[sg];
  const float* kr = K + kptr[sg] + (row - ptr[sg]) * ns;
  const uint32_t c = thr_count_row(kr, ns, thr[sg], ((ns & 3) == 0) && ((reinterpret_cast<uintptr_t>(kr) & 15) == 0), lane);
  if (lane == 0) row_cnt[row] = c;
}

__global__ __launch_bounds__(256) void thr_fill_seg_kernel(const float* __restrict__ K, const int64_t* __restrict__ ptr,
                                                           const int64_t* __restrict__ kptr, int64_t S, int64_t n,
                                                           const float* __restrict__ thr, const unsigned long long* __restrict__ row_off,
                                                           int64_t* __restrict__ ei_row, int64_t* __restrict__ ei_col,
                                                           float* __restrict__ ew, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t sg = seg_of_row(ptr, S, row);
  const int64_t ns = ptr[sg + 1] - ptr[sg];
  thr_fill_row(K + kptr[sg] + (row - ptr[sg]) * ns, ns, thr[sg], row_off[row], row, ptr[sg], ei_row, ei_col, ew, capacity, lane);
}

// d_ptr / d_kptr: device copies of the offsets (S + 1 each); n = ptr[S] >= 1.  *out_count must be zero on entry.
int launch_threshold_count_seg(const float* K, const int64_t* d_ptr, const int64_t* d_kptr, int64_t S, int64_t n, const float* thr,
                               unsigned long long* row_off, int64_t* out_count, uint32_t* row_cnt, hipStream_t s) {
  const unsigned grid = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(thr_count_seg_kernel, dim3(grid), dim3(256), 0, s, K, d_ptr, d_kptr, S, n, thr, row_cnt);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(thr_scan_kernel, dim3(1), dim3(1024), 0, s, row_cnt, n, row_off, out_count);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}
int launch_threshold_fill_seg(const float* K, const int64_t* d_ptr, const int64_t* d_kptr, int64_t S, int64_t n, const float* thr,
                              const unsigned long long* row_off, int64_t* ei, float* ew, int64_t capacity, hipStream_t s) {
  const unsigned grid = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(thr_fill_seg_kernel, dim3(grid), dim3(256), 0, s, K, d_ptr, d_kptr, S, n, thr, row_off, ei, ei + capacity, ew,
                     capacity);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf
