// mmf_fast_anyk.hip — the per-row bookkeeping kernels of mmf_simtopk_fast_anyk (the pass driver is in mmf_api.hip,
// the scan with ceilings in mmf_scan_bf16.hip).  A later pass re-ranks its candidates into a staging row per query: `depth` entries
// in the final order, of which a prefix are ghosts — columns the row has already emitted, which the ceiling let through.  Every
// kernel here is one thread per row.
#include "mmf_dev.h"
#include "mmf_host.h"

namespace mmf {

// floors between their row-indexed home and the position-indexed block an exact pass over gathered rows reads and writes
__global__ void floor_move_kernel(const int32_t* rows, int64_t cnt, float* row_key, uint32_t* row_id, float* pos_key, uint32_t* pos_id, int back) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= cnt) return;
  const int64_t r = rows[p];
  if (back) { row_key[r] = pos_key[p]; row_id[r] = pos_id[p]; }
  else { pos_key[p] = row_key[r]; pos_id[p] = row_id[r]; }
}

int launch_floor_move(const int32_t* rows, int64_t cnt, float* row_key, uint32_t* row_id, float* pos_key, uint32_t* pos_id, bool back,
                      hipStream_t s) {
  if (cnt <= 0) return MMF_OK;
  hipLaunchKernelGGL(floor_move_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, rows, cnt, row_key, row_id, pos_key, pos_id, back ? 1 : 0);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// the segmented call's floors between ids that are rows of Y (their home) and ids local to the row's segment (what an exact pass over
// one segment's columns reads and leaves); uint32 arithmetic, so the two directions undo each other exactly
__global__ void floor_rebase_kernel(const int32_t* rows, int64_t cnt, uint32_t* floor_id, const int32_t* col0, int add) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= cnt) return;
  const int64_t r = rows[p];
  const uint32_t c = (uint32_t)col0[r];
  floor_id[r] = add ? floor_id[r] + c : floor_id[r] - c;
}

int launch_floor_rebase(const int32_t* rows, int64_t cnt, uint32_t* floor_id, const int32_t* col0, bool add, hipStream_t s) {
  if (cnt <= 0) return MMF_OK;
  hipLaunchKernelGGL(floor_rebase_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, rows, cnt, floor_id, col0, add ? 1 : 0);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

__global__ void anyk_iota_kernel(int32_t* rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows[i] = (int32_t)i;
}

int launch_anyk_iota(int32_t* rows, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(anyk_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, n);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// the rows the re-rank could not certify (its fail list) get certified[row] = -1
__global__ void anyk_mark_kernel(const int32_t* fail_rows, const uint32_t* fail_count, int32_t* certified) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)fail_count[0]) certified[fail_rows[i]] = -1;
}

// certified[row]: -1 (flagged), else the staged entries that rank strictly after the row's floor — in the final order they are a
// suffix, so the count is depth minus the ghosts in front.  hist[c] counts the unflagged rows with c such entries, hist[depth + 1]
// the flagged rows, hist[depth + 2] is the largest ghost count.
__global__ void anyk_count_kernel(AnykStage st, const float* floor_key, const uint32_t* floor_id, int32_t* certified, uint32_t* hist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  if (certified[i] < 0) { atomicAdd(hist + st.depth + 1, 1u); return; }
  const float fk = floor_key[i];
  const uint32_t fid = floor_id[i];
  int ghosts = 0;
  for (int j = 0; j < st.depth; ++j) {
    const uint32_t id = (uint32_t)(st.idx[i * st.depth + j] - st.col_offset);
    if (better(fk, fid, st.key[i * st.depth + j], id)) break;
    ++ghosts;
  }
  certified[i] = st.depth - ghosts;
  atomicAdd(hist + (st.depth - ghosts), 1u);
  atomicMax(hist + st.depth + 2, (uint32_t)ghosts);
}

int launch_anyk_count(const AnykStage& st, const int32_t* fail_rows, const uint32_t* fail_count, const float* floor_key, const uint32_t* floor_id,
                      int32_t* certified, uint32_t* hist, hipStream_t s) {
  const unsigned grid = (unsigned)((st.n + 255) / 256);
  MMF_HIP(hipMemsetAsync(certified, 0, (size_t)st.n * 4, s));
  MMF_HIP(hipMemsetAsync(hist, 0, (size_t)(st.depth + 3) * 4, s));
  hipLaunchKernelGGL(anyk_mark_kernel, dim3(grid), dim3(256), 0, s, fail_rows, fail_count, certified);
  MMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(anyk_count_kernel, dim3(grid), dim3(256), 0, s, st, floor_key, floor_id, certified, hist);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

// A row with at least t certified entries copies the first t of them behind the `done` columns it has and moves its floor to the last
// one; any other row joins the list for the exact rescan (rows [*rescan_count], any order).
__global__ void anyk_emit_kernel(AnykStage st, const int32_t* certified, int t, int done, int out_stride, int64_t* out_idx, float* out_val,
                                 float* floor_key, uint32_t* floor_id, int32_t* rescan_rows, uint32_t* rescan_count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  const int c = certified[i];
  if (c < t) { rescan_rows[atomicAdd(rescan_count, 1u)] = (int32_t)i; return; }
  const int64_t src = i * st.depth + (st.depth - c), dst = i * out_stride + done;
  for (int j = 0; j < t; ++j) { out_idx[dst + j] = st.idx[src + j]; out_val[dst + j] = st.val[src + j]; }
  floor_key[i] = st.key[src + t - 1];
  floor_id[i] = (uint32_t)(st.idx[src + t - 1] - st.col_offset);
}

int launch_anyk_emit(const AnykStage& st, const int32_t* certified, int t, int done, int out_stride, int64_t* out_idx, float* out_val,
                     float* floor_key, uint32_t* floor_id, int32_t* rescan_rows, uint32_t* rescan_count, hipStream_t s) {
  MMF_HIP(hipMemsetAsync(rescan_count, 0, 4, s));
  hipLaunchKernelGGL(anyk_emit_kernel, dim3((unsigned)((st.n + 255) / 256)), dim3(256), 0, s, st, certified, t, done, out_stride, out_idx,
                     out_val, floor_key, floor_id, rescan_rows, rescan_count);
  MMF_LAUNCH_CHECK();
  return MMF_OK;
}

}  // namespace mmf
