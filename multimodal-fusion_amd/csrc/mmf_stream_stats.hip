// mmf_stream_stats.hip — the statistics of aggregate_wsi_super_patches for a slide whose K = K_h * K_g does not fit
// (include/mmf_hg_stream.h): the cluster means of mmf_segment_offdiag_mean and the five numbers of
// mmf_array_stats, from row panels of K that are recomputed and thrown away.
//
//   panel                launch_sim_dense_combined(row0, rows) — the f32-MFMA kernel; a row's bits do not depend on its panel
//   row sums             stream_row_sums_kernel: seg_row_sums_kernel's wave on the members whose rows the panel holds
//   mean/std/min/max     the panel is appended to what the last one left over and walked as flat rows of 4096 values by
//                        bracket_sweep_kernel<true> / stats_partial_kernel<true> (mmf_edges.hip): the plain kernels' assignment
//                        of values to lanes, the lanes' running sums kept on the device between the panels
//   median               lower_median_of over the same flat rows (one sweep, or four radix passes: K recomputed every time)
//
// The panel is bound by the f32 matrix cores (2 n^2 d flop), every reduction by HBM (a panel is written once and read once or
// twice).  No atomics on floats; every f64 sum has the plain kernel's order.
#include "../../include/mmf_hg_stream.h"
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

constexpr int64_t kFlatRow = 4096;                              // sweep_flat's row (mmf_edges.hip)
constexpr int64_t kOneSweepMin = (int64_t)1 << 22;              // values from which mmf_array_stats may take its one sweep

// member position of every row that has one (pos is preset to -1).  order[q] is a row of the slide for every q below
// offsets[n_clusters]; anything else (rows with a bad label leave holes behind the last member) is skipped.
__global__ __launch_bounds__(256) void stream_member_pos_kernel(const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                                int64_t n_clusters, int64_t n, int32_t* __restrict__ pos) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n || q >= offsets[n_clusters]) return;
  const int64_t r = order[q];
  if (r >= 0 && r < n) pos[r] = (int32_t)q;
}

// seg_row_sums_kernel (mmf_segments.hip) for the members whose rows are in the panel: one wave per panel row, the sum over the
// other members of its cluster lane-strided in member order, then the same butterfly.  Kp: rows [row0, row0 + rows) of K.
__global__ __launch_bounds__(256) void stream_row_sums_kernel(const float* __restrict__ Kp, int64_t n, int64_t row0, int64_t rows,
                                                              const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ seg_of, const int32_t* __restrict__ pos,
                                                              double* __restrict__ row_sum) {
  const int lane = threadIdx.x & 63;
  const int64_t li = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= rows) return;
  const int64_t q = pos[row0 + li];
  if (q < 0) return;
  const int c = seg_of[q];
  const int64_t b = offsets[c], e = offsets[c + 1];
  const float* row = Kp + li * n;
  double acc = 0.0;
  for (int64_t p = b + lane; p < e; p += 64)
    if (p != q) acc += (double)row[order[p]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) row_sum[q] = acc;
}

// What the call takes from its workspace, in order.  One function for the entry and for the size query.
struct StreamPlan {
  bool small;            // n * n < 2^22: the block is materialised and goes through the plain routines
  bool one_sweep;        // mmf_array_stats would take its partials from the median's one sweep
  int64_t R, grid;       // panel rows; workgroups of the plain launch whose lanes are carried
  size_t nf, Fp, K, part, scalars, median, lanes, row_sum, seg_of, pos, offdiag, stats;
  size_t total() const { return nf + Fp + K + part + scalars + median + lanes + row_sum + seg_of + pos + offdiag + stats; }
};
static StreamPlan stream_plan(int64_t n, int64_t d, int64_t panel_rows) {
  StreamPlan p{};
  const int64_t count = n * n;
  p.small = count < kOneSweepMin;
  p.nf = ws_bytes((size_t)n, 4);
  p.Fp = ws_bytes(prep_f32_bytes(n, d), 1);
  if (p.small) {
    p.K = ws_bytes((size_t)count, 4);
    p.offdiag = ws_bytes(segment_offdiag_scratch_bytes(n), 1);
    p.stats = ws_bytes(array_stats_scratch_bytes(count), 1);
    return p;
  }
  p.R = pick_panel_rows(n, panel_rows);
  p.one_sweep = median_one_sweep((unsigned long long)count);
  const int64_t full = count / kFlatRow;
  p.grid = p.one_sweep ? ((full + 3) / 4 < 2040 ? (full + 3) / 4 : 2040) : stats_partial_grid(count);
  p.K = ws_bytes((size_t)p.R * (size_t)n + (size_t)kFlatRow, 4);
  p.part = ws_bytes((size_t)2056 * stat_partial_bytes(), 1);
  p.scalars = ws_bytes(64, 4);
  p.median = ws_bytes(median_scratch_bytes((unsigned long long)count), 1);
  p.lanes = ws_bytes(stat_lanes_bytes(p.grid), 1);
  p.row_sum = ws_bytes((size_t)n, 8);
  p.seg_of = ws_bytes((size_t)n, 4);
  p.pos = ws_bytes((size_t)n, 4);
  return p;
}

static int check_shape(const char* who, int64_t n, int64_t d, int64_t dp) {
  if (n < 2) { set_error("%s: n must be at least 2 (got %lld)", who, (long long)n); return MMF_E_INVALID; }
  if (d < 1) { set_error("%s: d must be at least 1 (got %lld)", who, (long long)d); return MMF_E_INVALID; }
  if (dp < 1) { set_error("%s: dp must be at least 1 (got %lld)", who, (long long)dp); return MMF_E_INVALID; }
  if (n >= ((int64_t)1 << 31)) { set_error("%s: n must be < 2^31 (got %lld)", who, (long long)n); return MMF_E_UNSUPPORTED; }
  return MMF_OK;
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int64_t mmf_super_patch_stats_streamed_bytes(int64_t n, int64_t d, int64_t dp, int64_t n_clusters, int64_t panel_rows) {
  (void)n_clusters;                                    // the clusters take nothing: every per-cluster value goes to the caller's buffer
  const int rc = check_shape("super_patch_stats_streamed_bytes", n, d, dp);
  if (rc != MMF_OK) return (int64_t)rc;
  return (int64_t)stream_plan(n, d, panel_rows).total();
}

int mmf_super_patch_stats_streamed(const float* F, const float* P, int64_t n, int64_t d, int64_t dp, float lambda_h, float lambda_g,
                                   const int64_t* order, const int64_t* offsets, int64_t n_clusters, int64_t panel_rows,
                                   double* intra_mean, double* k_stats, int device_id, void* hip_stream) {
  Call c("super_patch_stats_streamed", device_id, hip_stream);
  MMF_TRY(c.on_device());
  MMF_TRY(check_shape(c.who, n, d, dp));
  if (!F) { set_error("%s: F is NULL", c.who); return MMF_E_INVALID; }
  if (!P) { set_error("%s: P is NULL", c.who); return MMF_E_INVALID; }
  if (!k_stats) { set_error("%s: k_stats is NULL", c.who); return MMF_E_INVALID; }
  if (order) {
    if (n_clusters < 1) { set_error("%s: n_clusters must be at least 1 (got %lld)", c.who, (long long)n_clusters); return MMF_E_INVALID; }
    if (!offsets) { set_error("%s: offsets is NULL (order is given)", c.who); return MMF_E_INVALID; }
    if (!intra_mean) { set_error("%s: intra_mean is NULL (order is given)", c.who); return MMF_E_INVALID; }
    if (n_clusters > segment_max_segments()) {
      set_error("%s: at most %d clusters are supported (got %lld)", c.who, segment_max_segments(), (long long)n_clusters);
      return MMF_E_UNSUPPORTED;
    }
  }
  const StreamPlan pl = stream_plan(n, d, panel_rows);
  MMF_TRY(c.begin(pl.total()));
  const hipStream_t s = c.s;
  const int64_t count = n * n;
  float* nf = c.ws.take<float>((size_t)n);
  float* Fp = reinterpret_cast<float*>(c.ws.take<char>(prep_f32_bytes(n, d)));
  MMF_TRY(launch_row_scalars(F, n, d, MMF_F32, MMF_RBF, nf, nullptr, s));
  MMF_TRY(launch_prep_f32(F, n, d, MMF_F32, nullptr, Fp, s));
  if (pl.small) {                                     // at most 16 MiB: the plain routines on the block itself
    float* K = c.ws.take<float>((size_t)count);
    char* od = c.ws.take<char>(segment_offdiag_scratch_bytes(n));
    char* st = c.ws.take<char>(array_stats_scratch_bytes(count));
    MMF_TRY(launch_sim_dense_combined(Fp, P, n, d, dp, lambda_h, lambda_g, nf, 0, n, K, s));
    if (order) MMF_TRY(launch_segment_offdiag_mean(K, n, order, offsets, n_clusters, intra_mean, od, s));
    return launch_array_stats(K, count, k_stats, st, s);
  }
  const int64_t R = pl.R;
  float* Kbuf = c.ws.take<float>((size_t)R * (size_t)n + (size_t)kFlatRow);
  char* part = c.ws.take<char>((size_t)2056 * stat_partial_bytes());
  float* med = c.ws.take<float>(64);
  float* pivot = med + 32;
  char* mscratch = c.ws.take<char>(median_scratch_bytes((unsigned long long)count));
  char* lanes = c.ws.take<char>(stat_lanes_bytes(pl.grid));
  double* row_sum = c.ws.take<double>((size_t)n);
  int32_t* seg_of = c.ws.take<int32_t>((size_t)n);
  int32_t* pos = c.ws.take<int32_t>((size_t)n);
  if (order) {
    MMF_HIP(hipMemsetAsync(pos, 0xff, (size_t)n * 4, s));
    MMF_TRY(launch_segment_member_clusters(offsets, n_clusters, seg_of, s));
    hipLaunchKernelGGL(stream_member_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, order, offsets, n_clusters, n, pos);
    MMF_LAUNCH_CHECK();
  }
  SweepCarry carry{lanes, pl.grid, 0};
  if (!pl.one_sweep) MMF_TRY(launch_stat_lanes_init(lanes, pl.grid, s));
  int sweeps = 0;
  // One pass over K: every panel lands behind the values the last one left over (fewer than one flat row), the whole flat rows
  // go to `consume` (and, without the one sweep, to the partial kernel's assignment on the first pass), the rest moves to the front.
  auto sweep = [&](const MedianConsume& consume) -> int {
    const bool first = sweeps++ == 0;
    int64_t held = 0, done = 0;                        // values waiting at Kbuf[0 .. held); flat rows handed over so far
    for (int64_t r0 = 0; r0 < n; r0 += R) {
      const int64_t rows = (n - r0 < R) ? (n - r0) : R;
      float* panel = Kbuf + held;
      MMF_TRY(launch_sim_dense_combined(Fp, P, n, d, dp, lambda_h, lambda_g, nf, r0, rows, panel, s));
      if (first && r0 == 0) MMF_HIP(hipMemcpyAsync(pivot, panel, 4, hipMemcpyDeviceToDevice, s));      // K[0][0]
      if (first && order) {
        hipLaunchKernelGGL(stream_row_sums_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, panel, n, r0, rows, order, offsets,
                           seg_of, pos, row_sum);
        MMF_LAUNCH_CHECK();
      }
      held += rows * n;
      const int64_t full = held / kFlatRow;
      if (full == 0) continue;
      if (first && !pl.one_sweep) MMF_TRY(launch_stats_partial_carry(Kbuf, full * kFlatRow, done * (kFlatRow / 4), pivot, lanes, pl.grid, s));
      carry.row0 = done;
      MMF_TRY(consume(Kbuf, kFlatRow, median_no_diagonal_row(), full));
      held -= full * kFlatRow;
      done += full;
      // source and destination do not overlap: the source starts at least one flat row in, fewer than one is left
      if (held > 0) MMF_HIP(hipMemcpyAsync(Kbuf, Kbuf + full * kFlatRow, (size_t)held * 4, hipMemcpyDeviceToDevice, s));
    }
    if (held > 0) {                                    // the ragged last row of the flat array
      if (first && !pl.one_sweep) MMF_TRY(launch_stats_partial_carry(Kbuf, held, done * (kFlatRow / 4), pivot, lanes, pl.grid, s));
      carry.row0 = -1;
      MMF_TRY(consume(Kbuf, held, median_no_diagonal_row(), 1));
    }
    return MMF_OK;
  };
  int64_t nparts = 0;
  MMF_TRY(lower_median_of(
      (unsigned long long)count,
      [&](float* sample, int sc) {
        return launch_sample_pairs(F, F, n, d, MMF_F32, lambda_h, P, (int)dp, lambda_g, /*offdiag*/ 0, (unsigned long long)count, sample, sc, s);
      },
      sweep, med, mscratch, s, part, pivot, &nparts, &carry));
  if (nparts == 0) {                                   // no one sweep: the lanes hold stats_partial_kernel's sums
    MMF_TRY(launch_stat_lanes_finish(lanes, pl.grid, part, s));
    nparts = pl.grid;
  }
  if (order) MMF_TRY(launch_segment_offdiag_final(row_sum, offsets, n_clusters, intra_mean, s));
  MMF_TRY(launch_stats_finish(part, nparts, pivot, count, k_stats, s));
  return launch_stats_set_median(med, k_stats, s);
}

}  // extern "C"
