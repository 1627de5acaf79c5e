// Personalised PageRank over the symmetrised kNN graph for gfx950 (CDNA4).
//
// rank_pull is one sweep of the power iteration for B legs (independent
// seed sets) at once. It is the pull pass of path.hip with another inner
// operation: a gather, a fused multiply-add and a sum where path_relax has
// a gather, an add and a minimum. Every vertex is computed and written by
// one owner lane from the input buffers only, so there are no atomics and
// the results are bit-identical from run to run. The torch statement of the
// same sweep is engines/graph_radio.pull_reference (f64 accumulation; the
// two agree to rounding, not bit for bit).
//
// Candidates of vertex v, in enumeration order:
//   own slots j = 0..k-1   u = idx[v][j] (skipped when u < 0), affinity s[v][j]
//   in-list positions      e = in_edge[q], u = e / k, affinity s.flat[e]
// Each candidate is one f32 FMA acc = s * x[b][u] + acc, from acc = 0.
//
// In-lists of up to LONG_LIST entries are walked by the owner lane; longer
// lists (hub vertices) are walked by the owner's whole wave, 64 entries at
// a time: every lane sums its own positions in ascending order, a fixed
// xor-butterfly adds the 64 partial sums, and the owner adds the total to
// its acc. The adjacency (idx, s, in_edge) is loaded once per vertex and
// reused across the B legs.
//
// SWEEP:   p_out[b][v] = (1 - alpha) * restart[b][v] + alpha * acc
//          q_out[b][v] = p_out[b][v] * inv_deg[v]
// !SWEEP:  p_out[b][v] = acc          (the degree pass: x = ones or the mask)
// Vertices that are not allowed get 0 in both modes.
//
// The (B, n) buffers are leg-major or vertex-major, as in path.hip (legs.h).

#include <hip/hip_runtime.h>

#include "legs.h"

namespace audiomuse {

namespace {

constexpr int LONG_LIST = 64;
constexpr int MAX_LEGS = 8;

template <int B, bool LEGS_INNER, bool SWEEP>
__global__ __launch_bounds__(256) void rank_pull_kernel(
    const float* __restrict__ x_in, float* __restrict__ p_out,
    float* __restrict__ q_out, const float* __restrict__ restart,
    const float* __restrict__ inv_deg, const int* __restrict__ idx,
    const float* __restrict__ s, const int* __restrict__ in_off,
    const int* __restrict__ in_edge, const unsigned char* __restrict__ allowed,
    float alpha, float one_minus_alpha, int n, int k, int n_in) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // lanes past n stay in the kernel: the wave-wide walk below needs them
  const bool live = v < n;
  const unsigned int un = (unsigned int)n, uk = (unsigned int)k;
  const unsigned int n_edges = un * uk;  // < 2^31, checked by the binding
  const size_t sn = (size_t)n;

  float acc[B];
  int beg = 0, end = 0;
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b] = 0.0f;
  if (live) {
    beg = min(max(in_off[v], 0), n_in);
    end = min(max(in_off[v + 1], beg), n_in);

    // ---- own slots ----
    const unsigned int row0 = (unsigned int)v * uk;
    for (unsigned int j = 0; j < uk; ++j) {
      const int u = idx[row0 + j];
      if (u < 0) continue;
      const unsigned int uu = min((unsigned int)u, un - 1u);
      const float wt = s[row0 + j];
      float xu[B];
      load_legs<B, LEGS_INNER>(x_in, sn, uu, xu);
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b] = __builtin_fmaf(wt, xu[b], acc[b]);
    }
  }

  // ---- in-lists: short ones by the owner, ascending ----
  const bool long_list = end - beg > LONG_LIST;
  if (!long_list) {
    for (int q = beg; q < end; ++q) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const unsigned int u = e / uk;
      const float wt = s[e];
      float xu[B];
      load_legs<B, LEGS_INNER>(x_in, sn, u, xu);
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b] = __builtin_fmaf(wt, xu[b], acc[b]);
    }
  }

  // ---- hub in-lists: the owner's whole wave walks them ----
  unsigned long long todo = __ballot(long_list);
  while (todo) {  // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int b0 = __shfl(beg, src);
    const int e0 = __shfl(end, src);
    float part[B];
#pragma unroll
    for (int b = 0; b < B; ++b) part[b] = 0.0f;
    for (int q = b0 + lane; q < e0; q += 64) {  // q ascends within a lane
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const unsigned int u = e / uk;
      const float wt = s[e];
      float xu[B];
      load_legs<B, LEGS_INNER>(x_in, sn, u, xu);
#pragma unroll
      for (int b = 0; b < B; ++b) part[b] = __builtin_fmaf(wt, xu[b], part[b]);
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      // a + b == b + a: every lane ends with the same total
      for (int off = 32; off > 0; off >>= 1)
        part[b] += __shfl_xor(part[b], off);
      if (lane == src) acc[b] += part[b];
    }
  }
  if (!live) return;

  const bool open = allowed == nullptr || allowed[v] != 0;
  if constexpr (SWEEP) {
    float r[B], p[B], qv[B];
    load_legs<B, LEGS_INNER>(restart, sn, (unsigned int)v, r);
    const float inv = inv_deg[v];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      p[b] = open ? __builtin_fmaf(alpha, acc[b], one_minus_alpha * r[b])
                  : 0.0f;
      qv[b] = p[b] * inv;
    }
    store_legs<B, LEGS_INNER>(p_out, sn, (unsigned int)v, p);
    store_legs<B, LEGS_INNER>(q_out, sn, (unsigned int)v, qv);
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b] = open ? acc[b] : 0.0f;
    store_legs<B, LEGS_INNER>(p_out, sn, (unsigned int)v, acc);
  }
}

}  // namespace

// x_in/p_out (B, n), and in a sweep q_out/restart (B, n) and inv_deg (n):
// leg-major or (legs_inner) vertex-major and then 16-byte aligned. q_out,
// restart and inv_deg are all null for the plain sum (p_out = acc). idx/s
// (n, k), in_off (n+1), in_edge (n_in), allowed (n) or null. 1 <= B <= 8
// and n*k < 2^31 are checked by the binding.
void launch_rank_pull(const float* x_in, float* p_out, float* q_out,
                      const float* restart, const float* inv_deg,
                      const int* idx, const float* s, const int* in_off,
                      const int* in_edge, const unsigned char* allowed,
                      float alpha, int B, int n, int k, int n_in,
                      int legs_inner, hipStream_t stream) {
  if (n <= 0 || B < 1 || B > MAX_LEGS) return;
  const bool sweep = restart != nullptr;
  dim3 grid((n + 255) / 256);
  dim3 block(256);
  // The kernel needs few registers (48 VGPRs at B = 8) and would run 8
  // waves per SIMD, but the sweep is bound by its random 32-byte gathers,
  // and with that many waves in flight the 8-leg sweep measured 1.05-1.15 ms
  // at 1M vertices against 0.87-1.01 ms with 3 (what path_relax runs with at
  // B = 8, by its register count). Dynamic LDS the kernel never touches
  // leaves room for 3 blocks per CU (profiles/r9_graph_radio.txt; B = 5..7
  // not measured).
  const size_t lds = B > 4 ? 48 * 1024 : 0;
#define AM_PULL_L(NB, INNER, SWEEP)                                           \
  hipLaunchKernelGGL((rank_pull_kernel<NB, INNER, SWEEP>), grid, block, lds,  \
                     stream, x_in, p_out, q_out, restart, inv_deg, idx, s,    \
                     in_off, in_edge, allowed, alpha, 1.0f - alpha, n, k,     \
                     n_in)
#define AM_PULL(NB)                                                           \
  case NB:                                                                    \
    if (legs_inner) {                                                         \
      if (sweep) AM_PULL_L(NB, true, true);                                   \
      else AM_PULL_L(NB, true, false);                                        \
    } else {                                                                  \
      if (sweep) AM_PULL_L(NB, false, true);                                  \
      else AM_PULL_L(NB, false, false);                                       \
    }                                                                         \
    break
  switch (B) {
    AM_PULL(1);
    AM_PULL(2);
    AM_PULL(3);
    AM_PULL(4);
    AM_PULL(5);
    AM_PULL(6);
    AM_PULL(7);
    AM_PULL(8);
  }
#undef AM_PULL
#undef AM_PULL_L
}

}  // namespace audiomuse
