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
// (torch.topk over the candidate buffer). The batch path at the end of
// this file (ivf_scan_topk_kernel) selects inside the scan instead and
// writes only the K best per query.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cfloat>
#include <type_traits>

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

// ---------------------------------------------------------------------------
// Fused probed-cell scan + top-K. Instead of writing every candidate to a
// (Q, cap) buffer, a workgroup keeps the K best of the probe-list slice it
// walks and writes only those: grid = (S, Q), split s of query q walks
// probes [s*nprobe/S, (s+1)*nprobe/S), out (Q, S, K) sorted ascending by
// (distance, row), unused slots +inf / -1. The host merges the S lists.
//
// Order is one 64-bit key: the f32 distance mapped monotonically into the
// high word (sign set: all bits flipped, else only the sign bit), the
// packed row in the low word. Keys are unique, so the result does not
// depend on the order candidates were met in.
//
// One list per workgroup, in LDS: key[0, K) is the sorted best list,
// key[K, 256) padding, key[256, 512) a staging area that sub-group leaders
// append to (LDS atomic counter) when key <= tau, the current K-th best.
// Before a group of 4 passes (at most 64 appends) the workgroup checks that
// the staging area has 64 free slots and otherwise bitonic-sorts all 512
// keys, which tightens tau and empties the staging area.
//
// Every loop that holds a barrier runs a workgroup-uniform number of trips
// (probe entries, cell offsets and the staging count are read alike by all
// threads); rows past the end of a cell are clamped and predicated, not
// skipped. The only return is for an empty slice, before any barrier.
//
// Row reads, lane striding, reduce order and distance expressions are
// those of the scans above. blockDim.x must be 256.
// LDS per workgroup: 512 keys x 8 B + 16 B (tau, count) + query
// (d x 4 B) = 6160 B at d = 512, whatever K is.
// ---------------------------------------------------------------------------
constexpr int TK_KMAX = 256;            // best-list capacity
constexpr int TK_STAGE = 256;           // staging capacity
constexpr int TK_N = TK_KMAX + TK_STAGE;  // keys sorted per flush
constexpr int TK_GROUP = 4;             // passes between overflow checks
constexpr int TK_ROWS = 16;             // rows per pass (4 waves x 4)
constexpr unsigned long long TK_PAD = ~0ull;

__device__ __forceinline__ unsigned long long tk_key(float dist, int row) {
  if (dist == 0.0f) dist = 0.0f;  // -0 and +0 are one distance
  unsigned int u = __float_as_uint(dist);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned int)row;
}

__device__ __forceinline__ float tk_key_dist(unsigned long long key) {
  unsigned int u = (unsigned int)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

// a * b + c with both roundings (no fma contraction)
__device__ __forceinline__ float tk_mul_add_unfused(float a, float b,
                                                    float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p + c;
}

// Sort all TK_N keys ascending, keep the first K, reset the staging area.
// Called by all 256 threads; every barrier is unconditional.
__device__ __forceinline__ void tk_flush(unsigned long long* key, int* count,
                                         unsigned long long* tau, int K) {
  const int t = threadIdx.x;
  for (int k = 2; k <= TK_N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j clear
      const unsigned long long a = key[i], b = key[i + j];
      const bool asc = (i & k) == 0;
      if ((a > b) == asc) {
        key[i] = b;
        key[i + j] = a;
      }
      __syncthreads();
    }
  }
  const unsigned long long kth = key[K - 1];
  if (t >= K) key[t] = TK_PAD;
  key[TK_KMAX + t] = TK_PAD;
  if (t == 0) {
    *count = 0;
    *tau = kth;
  }
  __syncthreads();
}

// DT: 0 f32, 1 f16, 2 i8 (int32-packed, d = dim/4, angular only).
// EXCL: a candidate whose row_label equals the query's q_label is never
// staged (a negative q_label excludes nothing); everything else, staging,
// tau, the flush, key order and padding, is the plain kernel's.
template <int DT, int METRIC, bool SEL, bool EXCL>
__global__ __launch_bounds__(256) void ivf_scan_topk_kernel(
    const void* __restrict__ query_v,   // (Q, d) f32, or (Q, d) packed i8
    const float* __restrict__ qnorm,    // (Q,)
    const void* __restrict__ data_v,    // (N, d)
    const float* __restrict__ row_norm, // (N,)
    const int* __restrict__ probe,      // (Q, nprobe) cell ids (-1 = skip)
    const int* __restrict__ off,        // (ncells+1,) cell_off, or sel_off
    const int* __restrict__ sel_rows,   // (M,) allowed rows (SEL only)
    const int* __restrict__ skip_row,   // (Q,) row never reported, or null
    float* __restrict__ out_dist,       // (Q, S, K)
    int* __restrict__ out_row,          // (Q, S, K)
    int d, int nprobe, int K,
    const int* __restrict__ row_label,  // (N,) packed order (EXCL only)
    const int* __restrict__ q_label) {  // (Q,) (EXCL only)
  const int s = blockIdx.x;
  const int S = gridDim.x;
  const int q = blockIdx.y;
  const int tid = threadIdx.x;
  float* od = out_dist + ((long long)q * S + s) * K;
  int* orow = out_row + ((long long)q * S + s) * K;
  const int p0 = (int)((long long)s * nprobe / S);
  const int p1 = (int)((long long)(s + 1) * nprobe / S);
  if (p0 >= p1) {  // empty slice: padding only (no barrier passed yet)
    if (tid < K) {
      od[tid] = INFINITY;
      orow[tid] = -1;
    }
    return;
  }
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int sub = lane >> 4;
  const int sl = lane & 15;

  extern __shared__ unsigned long long tk_lds[];
  unsigned long long* key = tk_lds;           // TK_N keys
  unsigned long long* tau = tk_lds + TK_N;    // current K-th best key
  int* count = (int*)(tk_lds + TK_N + 1);     // staged keys
  float* qf = (float*)(tk_lds + TK_N + 2);    // d query words
  int* qs = (int*)qf;

  key[tid] = TK_PAD;
  key[TK_KMAX + tid] = TK_PAD;
  if (tid == 0) {
    *tau = TK_PAD;
    *count = 0;
  }
  for (int i = tid; i < d; i += 256)
    qs[i] = ((const int*)query_v)[(long long)q * d + i];
  __syncthreads();

  const float qn = qnorm[q];
  const int skip = skip_row ? skip_row[q] : -1;
  const int qlab = EXCL ? q_label[q] : -1;

  for (int p = p0; p < p1; ++p) {
    const int cell = probe[(long long)q * nprobe + p];
    if (cell < 0) continue;
    const int b0 = off[cell], b1 = off[cell + 1];
    for (int gb = b0; gb < b1; gb += TK_GROUP * TK_ROWS) {
      // all appends of the previous group have landed; everyone reads the
      // count before anyone appends again, so the branch is uniform
      __syncthreads();
      const int staged = *count;
      __syncthreads();
      if (staged + TK_GROUP * TK_ROWS > TK_STAGE) tk_flush(key, count, tau, K);
      const unsigned long long thr = *tau;
      // the group's 4 rows per sub-group are read side by side (4 loads
      // in flight per lane); each row keeps its own accumulator and the
      // j order of the scans above, so its distance does not change
      int r[TK_GROUP];
      bool live[TK_GROUP];
      float dist[TK_GROUP];
#pragma unroll
      for (int g = 0; g < TK_GROUP; ++g) {
        const int i = gb + g * TK_ROWS + wave * 4 + sub;
        live[g] = i < b1;
        const int ic = min(i, b1 - 1);
        r[g] = SEL ? sel_rows[ic] : ic;
      }
      if (DT == 2) {
        const int* row[TK_GROUP];
        int acc[TK_GROUP];
#pragma unroll
        for (int g = 0; g < TK_GROUP; ++g) {
          row[g] = (const int*)data_v + (long long)r[g] * d;
          acc[g] = 0;
        }
        for (int j = sl; j < d; j += 16) {
#pragma unroll
          for (int g = 0; g < TK_GROUP; ++g)
            acc[g] = __builtin_amdgcn_sdot4(qs[j], row[g][j], acc[g], false);
        }
#pragma unroll
        for (int g = 0; g < TK_GROUP; ++g) {
          const int a = sub_reduce_sum_i32(acc[g]);
          // spelled as hipcc contracts it in ivf_scan_i8_angular (one fma)
          const float denom = __fmaf_rn(qn, row_norm[r[g]], 1e-12f);
          float cosv = (float)a / denom;
          cosv = fminf(1.0f, fmaxf(-1.0f, cosv));
          dist[g] = 1.0f - cosv;
        }
      } else {
        typedef typename std::conditional<DT == 1, __half, float>::type T;
        const T* row[TK_GROUP];
        float acc[TK_GROUP];
#pragma unroll
        for (int g = 0; g < TK_GROUP; ++g) {
          row[g] = (const T*)data_v + (long long)r[g] * d;
          acc[g] = 0.0f;
        }
        for (int j = sl; j < d; j += 16) {
#pragma unroll
          for (int g = 0; g < TK_GROUP; ++g) {
            const float v = to_f32(row[g][j]);
            if (METRIC == 1) {
              const float diff = v - qf[j];
              acc[g] += diff * diff;
            } else {
              acc[g] += v * qf[j];
            }
          }
        }
#pragma unroll
        for (int g = 0; g < TK_GROUP; ++g) {
          const float a = sub_reduce_sum(acc[g]);
          if (METRIC == 0) {
            // spelled as hipcc emits it in ivf_scan_float (mul, then add:
            // the add is paired with the reduce and not contracted)
            float cosv =
                a / tk_mul_add_unfused(qn, row_norm[r[g]], 1e-12f);
            dist[g] = 1.0f - fminf(1.0f, fmaxf(-1.0f, cosv));
          } else if (METRIC == 1) {
            dist[g] = sqrtf(a);
          } else {
            dist[g] = -a;
          }
        }
      }
      if (sl == 0) {
#pragma unroll
        for (int g = 0; g < TK_GROUP; ++g) {
          if (live[g] && r[g] != skip &&
              (!EXCL || qlab < 0 || row_label[r[g]] != qlab)) {
            const unsigned long long kv = tk_key(dist[g], r[g]);
            if (kv <= thr) {
              const int slot = atomicAdd(count, 1);  // < TK_STAGE, see above
              key[TK_KMAX + slot] = kv;
            }
          }
        }
      }
    }
  }

  __syncthreads();
  tk_flush(key, count, tau, K);
  if (tid < K) {
    const unsigned long long kv = key[tid];
    const bool pad = kv == TK_PAD;
    od[tid] = pad ? INFINITY : tk_key_dist(kv);
    orow[tid] = pad ? -1 : (int)(unsigned int)kv;
  }
}

// S = gridDim.x splits per query; sel_rows == nullptr selects the unscoped
// walk over cell_off. K must be in [1, TK_KMAX] (checked by the binding).
void launch_ivf_scan_topk(int dtype_code, int metric, const void* query,
                          const float* qnorm, const void* data,
                          const float* row_norm, const int* probe,
                          const int* off, const int* sel_rows,
                          const int* skip_row, float* out_dist, int* out_row,
                          int Q, int S, int K, int d, int nprobe,
                          hipStream_t stream) {
  dim3 grid(S, Q);
  dim3 block(256);
  const int dw = dtype_code == 2 ? d / 4 : d;  // query words in LDS
  const size_t lds = (size_t)(TK_N + 2) * sizeof(unsigned long long) +
                     (size_t)dw * sizeof(float);
#define AM_TOPK(DT, M)                                                         \
  do {                                                                         \
    if (sel_rows)                                                              \
      hipLaunchKernelGGL((ivf_scan_topk_kernel<DT, M, true, false>), grid,    \
                         block, lds, stream, query, qnorm, data, row_norm,    \
                         probe, off, sel_rows, skip_row, out_dist, out_row,   \
                         dw, nprobe, K, nullptr, nullptr);                     \
    else                                                                       \
      hipLaunchKernelGGL((ivf_scan_topk_kernel<DT, M, false, false>), grid,   \
                         block, lds, stream, query, qnorm, data, row_norm,    \
                         probe, off, sel_rows, skip_row, out_dist, out_row,   \
                         dw, nprobe, K, nullptr, nullptr);                     \
  } while (0)
  if (dtype_code == 2) {  // i8, angular only
    AM_TOPK(2, 0);
  } else if (dtype_code == 1) {
    if (metric == 0) AM_TOPK(1, 0);
    else if (metric == 1) AM_TOPK(1, 1);
    else AM_TOPK(1, 2);
  } else {
    if (metric == 0) AM_TOPK(0, 0);
    else if (metric == 1) AM_TOPK(0, 1);
    else AM_TOPK(0, 2);
  }
#undef AM_TOPK
}

// The unscoped walk with label exclusion: row_label (N,) in packed order,
// q_label (Q,). Everything else as launch_ivf_scan_topk without sel_rows.
void launch_ivf_scan_topk_excl(int dtype_code, int metric, const void* query,
                               const float* qnorm, const void* data,
                               const float* row_norm, const int* probe,
                               const int* cell_off, const int* skip_row,
                               const int* row_label, const int* q_label,
                               float* out_dist, int* out_row, int Q, int S,
                               int K, int d, int nprobe, hipStream_t stream) {
  dim3 grid(S, Q);
  dim3 block(256);
  const int dw = dtype_code == 2 ? d / 4 : d;  // query words in LDS
  const size_t lds = (size_t)(TK_N + 2) * sizeof(unsigned long long) +
                     (size_t)dw * sizeof(float);
#define AM_TOPK_EXCL(DT, M)                                                    \
  hipLaunchKernelGGL((ivf_scan_topk_kernel<DT, M, false, true>), grid, block, \
                     lds, stream, query, qnorm, data, row_norm, probe,        \
                     cell_off, nullptr, skip_row, out_dist, out_row, dw,      \
                     nprobe, K, row_label, q_label)
  if (dtype_code == 2) {  // i8, angular only
    AM_TOPK_EXCL(2, 0);
  } else if (dtype_code == 1) {
    if (metric == 0) AM_TOPK_EXCL(1, 0);
    else if (metric == 1) AM_TOPK_EXCL(1, 1);
    else AM_TOPK_EXCL(1, 2);
  } else {
    if (metric == 0) AM_TOPK_EXCL(0, 0);
    else if (metric == 1) AM_TOPK_EXCL(0, 1);
    else AM_TOPK_EXCL(0, 2);
  }
#undef AM_TOPK_EXCL
}

}  // namespace audiomuse
