// IVF cell-scan distance kernels for gfx950 (CDNA4).
//
// Replaces the reference's NumKong SIMD cdist scan
// (/root/reference/tasks/ivf_quant.py:106-147 + tasks/paged_ivf.py:1035:
// per-query thread-pool loop over probed cells, CPU SIMD) with one GPU
// launch: grid = (nprobe, Q); each workgroup scans one probed cell for
// one query, one row per 64-lane wave, lanes striding the dimension
// (coalesced row-major reads), wave shuffle-reduce for the dot/SSD.
//
// Storage dtypes match the reference codec (ivf_quant.py):
//   i8  : vectors scaled by 127, angular only (dot via sdot4, 4 i8/int)
//   f16 : half vectors
//   f32 : float vectors
// Metrics (reference semantics):
//   angular   : 1 - clip(cos(q, v), -1, 1)   (cos in the encoded domain)
//   euclidean : sqrt(sum((v - q)^2))
//   dot       : -sum(v * q)
//
// The cell layout is HBM-resident and packed: data (N, d) sorted by cell,
// cell_off (nlist+1) prefix offsets, row_norm (N) f32 norms of the encoded
// rows (for angular). Candidates are written to a dense per-query buffer
// (prefix offsets precomputed on the host); top-k select happens upstream
// (torch.topk over the candidate buffer).

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cfloat>

namespace audiomuse {

// 16-lane sub-group reductions: each wave scans 4 rows concurrently
// (4x fewer shuffle steps per row than a full-wave reduce, full
// coalescing preserved: 16 lanes x 4 B = one 64 B segment per row).
__device__ __forceinline__ float sub_reduce_sum(float v) {
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
  return v;
}

__device__ __forceinline__ int sub_reduce_sum_i32(int v) {
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
  return v;
}

// torch builds with __HIP_NO_HALF_CONVERSIONS__: convert explicitly
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }

// ---------------------------------------------------------------------------
// i8 angular scan. d must be a multiple of 4 (padded at build time).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_scan_i8_angular(
    const int* __restrict__ qpack,      // (Q, d/4) int32-packed i8 query
    const float* __restrict__ qnorm,    // (Q,) ||q|| in i8 domain
    const int* __restrict__ data,       // (N, d/4) int32-packed i8 rows
    const float* __restrict__ row_norm, // (N,) ||v|| in i8 domain
    const int* __restrict__ probe,      // (Q, nprobe) cell ids (-1 = skip)
    const int* __restrict__ cell_off,   // (nlist+1,)
    const long long* __restrict__ cand_off, // (Q, nprobe) output offsets
    float* __restrict__ out_dist,       // (Q * cap,)
    int* __restrict__ out_row,          // (Q * cap,) packed row index
    int d4, int nprobe, long long cap) {
  const int p = blockIdx.x;
  const int q = blockIdx.y;
  const int cell = probe[(long long)q * nprobe + p];
  if (cell < 0) return;
  const int r0 = cell_off[cell], r1 = cell_off[cell + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int sub = lane >> 4;       // row slot within the wave (0..3)
  const int sl = lane & 15;        // lane within the 16-lane sub-group

  extern __shared__ int qs[];  // d/4 ints
  for (int i = threadIdx.x; i < d4; i += blockDim.x)
    qs[i] = qpack[(long long)q * d4 + i];
  __syncthreads();

  const float qn = qnorm[q];
  const long long base = cand_off[(long long)q * nprobe + p];
  float* dq = out_dist + (long long)q * cap;
  int* rq = out_row + (long long)q * cap;

  for (int r = r0 + wave * 4 + sub; r < r1; r += nwaves * 4) {
    const int* row = data + (long long)r * d4;
    int acc = 0;
    for (int j = sl; j < d4; j += 16)
      acc = __builtin_amdgcn_sdot4(qs[j], row[j], acc, false);
    acc = sub_reduce_sum_i32(acc);
    if (sl == 0) {
      const float denom = qn * row_norm[r] + 1e-12f;
      float cosv = (float)acc / denom;
      cosv = fminf(1.0f, fmaxf(-1.0f, cosv));
      const long long slot = base + (r - r0);
      dq[slot] = 1.0f - cosv;
      rq[slot] = r;
    }
  }
}

// ---------------------------------------------------------------------------
// f16 / f32 scan, all three metrics (METRIC: 0 angular, 1 euclidean, 2 dot).
// ---------------------------------------------------------------------------
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void ivf_scan_float(
    const float* __restrict__ query,    // (Q, d) f32 (pre-normalized if angular)
    const float* __restrict__ qnorm,    // (Q,)
    const T* __restrict__ data,         // (N, d)
    const float* __restrict__ row_norm, // (N,)
    const int* __restrict__ probe, const int* __restrict__ cell_off,
    const long long* __restrict__ cand_off, float* __restrict__ out_dist,
    int* __restrict__ out_row, int d, int nprobe, long long cap) {
  const int p = blockIdx.x;
  const int q = blockIdx.y;
  const int cell = probe[(long long)q * nprobe + p];
  if (cell < 0) return;
  const int r0 = cell_off[cell], r1 = cell_off[cell + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const int sub = lane >> 4;
  const int sl = lane & 15;

  extern __shared__ float qf[];  // d floats
  for (int i = threadIdx.x; i < d; i += blockDim.x)
    qf[i] = query[(long long)q * d + i];
  __syncthreads();

  const float qn = qnorm[q];
  const long long base = cand_off[(long long)q * nprobe + p];
  float* dq = out_dist + (long long)q * cap;
  int* rq = out_row + (long long)q * cap;

  for (int r = r0 + wave * 4 + sub; r < r1; r += nwaves * 4) {
    const T* row = data + (long long)r * d;
    float acc = 0.0f;
    for (int j = sl; j < d; j += 16) {
      const float v = to_f32(row[j]);
      if (METRIC == 1) {
        const float diff = v - qf[j];
        acc += diff * diff;
      } else {
        acc += v * qf[j];
      }
    }
    acc = sub_reduce_sum(acc);
    if (sl == 0) {
      float dist;
      if (METRIC == 0) {
        float cosv = acc / (qn * row_norm[r] + 1e-12f);
        dist = 1.0f - fminf(1.0f, fmaxf(-1.0f, cosv));
      } else if (METRIC == 1) {
        dist = sqrtf(acc);
      } else {
        dist = -acc;
      }
      const long long slot = base + (r - r0);
      dq[slot] = dist;
      rq[slot] = r;
    }
  }
}

// ---------------------------------------------------------------------------
// Row-selection ("scoped") scans. Instead of walking a cell's packed rows
// [cell_off[c], cell_off[c+1]) the workgroup walks an indirection list:
// sel_rows (M,) holds the packed-row indices of the allowed rows, ascending
// (hence grouped by cell), and sel_off (ncells+1,) its per-cell prefix
// offsets. Only allowed rows are read, every sub-group works on an allowed
// row, and candidate slots are dense over the allowed counts. The row index
// is a dependent load in front of every row read, so the index for the next
// pass is fetched before the current row is reduced. Row reads, lane
// striding and the reduce are those of the unscoped kernels above.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_scan_sel_i8_angular(
    const int* __restrict__ qpack, const float* __restrict__ qnorm,
    const int* __restrict__ data, const float* __restrict__ row_norm,
    const int* __restrict__ probe,
    const int* __restrict__ sel_rows,   // (M,) allowed packed rows, ascending
    const int* __restrict__ sel_off,    // (ncells+1,) offsets into sel_rows
    const long long* __restrict__ cand_off, float* __restrict__ out_dist,
    int* __restrict__ out_row, int d4, int nprobe, long long cap) {
  const int p = blockIdx.x;
  const int q = blockIdx.y;
  const int cell = probe[(long long)q * nprobe + p];
  if (cell < 0) return;
  const int s0 = sel_off[cell], s1 = sel_off[cell + 1];
  if (s0 >= s1) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int step = (blockDim.x >> 6) * 4;
  const int sub = lane >> 4;
  const int sl = lane & 15;

  extern __shared__ int qs[];  // d/4 ints
  for (int i = threadIdx.x; i < d4; i += blockDim.x)
    qs[i] = qpack[(long long)q * d4 + i];
  __syncthreads();

  const float qn = qnorm[q];
  const long long base = cand_off[(long long)q * nprobe + p];
  float* dq = out_dist + (long long)q * cap;
  int* rq = out_row + (long long)q * cap;

  // index loads are clamped, not predicated: a branch around the load
  // makes the compiler wait for it on the spot and the prefetch is lost
  int i = s0 + wave * 4 + sub;
  int r = sel_rows[min(i, s1 - 1)];
  for (; i < s1; i += step) {
    const int rnext = sel_rows[min(i + step, s1 - 1)];
    const int* row = data + (long long)r * d4;
    int acc = 0;
    for (int j = sl; j < d4; j += 16)
      acc = __builtin_amdgcn_sdot4(qs[j], row[j], acc, false);
    acc = sub_reduce_sum_i32(acc);
    if (sl == 0) {
      const float denom = qn * row_norm[r] + 1e-12f;
      float cosv = (float)acc / denom;
      cosv = fminf(1.0f, fmaxf(-1.0f, cosv));
      const long long slot = base + (i - s0);
      dq[slot] = 1.0f - cosv;
      rq[slot] = r;
    }
    r = rnext;
  }
}

template <typename T, int METRIC>
__global__ __launch_bounds__(256) void ivf_scan_sel_float(
    const float* __restrict__ query, const float* __restrict__ qnorm,
    const T* __restrict__ data, const float* __restrict__ row_norm,
    const int* __restrict__ probe, const int* __restrict__ sel_rows,
    const int* __restrict__ sel_off, const long long* __restrict__ cand_off,
    float* __restrict__ out_dist, int* __restrict__ out_row, int d, int nprobe,
    long long cap) {
  const int p = blockIdx.x;
  const int q = blockIdx.y;
  const int cell = probe[(long long)q * nprobe + p];
  if (cell < 0) return;
  const int s0 = sel_off[cell], s1 = sel_off[cell + 1];
  if (s0 >= s1) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int step = (blockDim.x >> 6) * 4;
  const int sub = lane >> 4;
  const int sl = lane & 15;

  extern __shared__ float qf[];  // d floats
  for (int i = threadIdx.x; i < d; i += blockDim.x)
    qf[i] = query[(long long)q * d + i];
  __syncthreads();

  const float qn = qnorm[q];
  const long long base = cand_off[(long long)q * nprobe + p];
  float* dq = out_dist + (long long)q * cap;
  int* rq = out_row + (long long)q * cap;

  // index loads are clamped, not predicated: a branch around the load
  // makes the compiler wait for it on the spot and the prefetch is lost
  int i = s0 + wave * 4 + sub;
  int r = sel_rows[min(i, s1 - 1)];
  for (; i < s1; i += step) {
    const int rnext = sel_rows[min(i + step, s1 - 1)];
    const T* row = data + (long long)r * d;
    float acc = 0.0f;
    for (int j = sl; j < d; j += 16) {
      const float v = to_f32(row[j]);
      if (METRIC == 1) {
        const float diff = v - qf[j];
        acc += diff * diff;
      } else {
        acc += v * qf[j];
      }
    }
    acc = sub_reduce_sum(acc);
    if (sl == 0) {
      float dist;
      if (METRIC == 0) {
        float cosv = acc / (qn * row_norm[r] + 1e-12f);
        dist = 1.0f - fminf(1.0f, fmaxf(-1.0f, cosv));
      } else if (METRIC == 1) {
        dist = sqrtf(acc);
      } else {
        dist = -acc;
      }
      const long long slot = base + (i - s0);
      dq[slot] = dist;
      rq[slot] = r;
    }
    r = rnext;
  }
}

void launch_ivf_scan(int dtype_code, int metric, const void* query,
                     const float* qnorm, const void* data,
                     const float* row_norm, const int* probe,
                     const int* cell_off, const long long* cand_off,
                     float* out_dist, int* out_row, int Q, int d, int nprobe,
                     long long cap, hipStream_t stream) {
  dim3 grid(nprobe, Q);
  dim3 block(256);
  if (dtype_code == 2) {  // i8, angular only
    const int d4 = d / 4;
    const size_t lds = (size_t)d4 * sizeof(int);
    hipLaunchKernelGGL(ivf_scan_i8_angular, grid, block, lds, stream,
                       (const int*)query, qnorm, (const int*)data, row_norm,
                       probe, cell_off, cand_off, out_dist, out_row, d4,
                       nprobe, cap);
    return;
  }
  const size_t lds = (size_t)d * sizeof(float);
#define AM_SCAN(T, M)                                                          \
  hipLaunchKernelGGL((ivf_scan_float<T, M>), grid, block, lds, stream,        \
                     (const float*)query, qnorm, (const T*)data, row_norm,    \
                     probe, cell_off, cand_off, out_dist, out_row, d, nprobe, \
                     cap)
  if (dtype_code == 1) {
    if (metric == 0) AM_SCAN(__half, 0);
    else if (metric == 1) AM_SCAN(__half, 1);
    else AM_SCAN(__half, 2);
  } else {
    if (metric == 0) AM_SCAN(float, 0);
    else if (metric == 1) AM_SCAN(float, 1);
    else AM_SCAN(float, 2);
  }
#undef AM_SCAN
}

void launch_ivf_scan_sel(int dtype_code, int metric, const void* query,
                         const float* qnorm, const void* data,
                         const float* row_norm, const int* probe,
                         const int* sel_rows, const int* sel_off,
                         const long long* cand_off, float* out_dist,
                         int* out_row, int Q, int d, int nprobe, long long cap,
                         hipStream_t stream) {
  dim3 grid(nprobe, Q);
  dim3 block(256);
  if (dtype_code == 2) {  // i8, angular only
    const int d4 = d / 4;
    const size_t lds = (size_t)d4 * sizeof(int);
    hipLaunchKernelGGL(ivf_scan_sel_i8_angular, grid, block, lds, stream,
                       (const int*)query, qnorm, (const int*)data, row_norm,
                       probe, sel_rows, sel_off, cand_off, out_dist, out_row,
                       d4, nprobe, cap);
    return;
  }
  const size_t lds = (size_t)d * sizeof(float);
#define AM_SCAN_SEL(T, M)                                                      \
  hipLaunchKernelGGL((ivf_scan_sel_float<T, M>), grid, block, lds, stream,    \
                     (const float*)query, qnorm, (const T*)data, row_norm,    \
                     probe, sel_rows, sel_off, cand_off, out_dist, out_row, d, \
                     nprobe, cap)
  if (dtype_code == 1) {
    if (metric == 0) AM_SCAN_SEL(__half, 0);
    else if (metric == 1) AM_SCAN_SEL(__half, 1);
    else AM_SCAN_SEL(__half, 2);
  } else {
    if (metric == 0) AM_SCAN_SEL(float, 0);
    else if (metric == 1) AM_SCAN_SEL(float, 1);
    else AM_SCAN_SEL(float, 2);
  }
#undef AM_SCAN_SEL
}

}  // namespace audiomuse
