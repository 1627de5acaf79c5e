// Batched shortest paths over the symmetrised kNN graph for gfx950 (CDNA4).
//
// path_relax is one Jacobi sweep of Bellman-Ford for B legs (independent
// sources) at once. Like the map layout epoch (layout.hip) it is a pull
// pass: every vertex is computed and written by one owner lane from the
// input buffers only, so there are no atomics and distances and
// predecessors are bit-identical from run to run. The torch statement of
// the same sweep is engines/graph_path.relax_reference.
//
// Candidates of vertex v, in enumeration order:
//   own slots s = 0..k-1   u = idx[v][s] (skipped when u < 0), weight w[v][s]
//   in-list positions      e = in_edge[q], u = e / k, weight w.flat[e]
// Each candidate is the single f32 addition dist_in[b][u] + weight; the
// running best starts at dist_in[b][v] / pred_in[b][v] and is replaced only
// by a strictly smaller candidate, so of equal candidates the earliest wins.
//
// In-lists of up to LONG_LIST entries are walked by the owner lane; longer
// lists (hub vertices) are walked by the owner's whole wave, 64 entries at
// a time, and reduced by the lexicographic minimum of (candidate, position),
// which is the same tie rule. The adjacency (idx, w, in_edge) is loaded
// once per vertex and reused across the B legs.
//
// The (B, n) buffers come in one of two memory layouts: leg-major (row b
// is contiguous) or vertex-major (the B values of a vertex are contiguous,
// LEGS_INNER). Vertex-major is what the engine allocates: the B gathers of
// a candidate then fall into one 32-byte run and are read with 8- or
// 16-byte loads (load_legs / store_legs, legs.h).
//
// path_walk follows the predecessors of one leg per lane from the target
// back to the source.

#include <hip/hip_runtime.h>

#include "legs.h"

namespace audiomuse {

namespace {

constexpr int LONG_LIST = 64;
constexpr int MAX_LEGS = 8;

template <int B, bool LEGS_INNER>
__global__ __launch_bounds__(256) void path_relax_kernel(
    const float* __restrict__ dist_in, const int* __restrict__ pred_in,
    float* __restrict__ dist_out, int* __restrict__ pred_out,
    const int* __restrict__ idx, const float* __restrict__ w,
    const int* __restrict__ in_off, const int* __restrict__ in_edge,
    const unsigned char* __restrict__ allowed, int* __restrict__ changed,
    int n, int k, int n_in) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // lanes past n stay in the kernel: the wave-wide walk below needs them
  const bool live = v < n;
  const unsigned int un = (unsigned int)n, uk = (unsigned int)k;
  const unsigned int n_edges = un * uk;  // < 2^31, checked by the binding
  const size_t sn = (size_t)n;

  float best[B], old[B];
  int bp[B];
  int beg = 0, end = 0;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    best[b] = old[b] = __builtin_inff();
    bp[b] = -1;
  }
  if (live) {
    load_legs<B, LEGS_INNER>(dist_in, sn, (unsigned int)v, old);
    load_legs<B, LEGS_INNER>(pred_in, sn, (unsigned int)v, bp);
#pragma unroll
    for (int b = 0; b < B; ++b) best[b] = old[b];
    beg = min(max(in_off[v], 0), n_in);
    end = min(max(in_off[v + 1], beg), n_in);

    // ---- own slots ----
    const unsigned int row0 = (unsigned int)v * uk;
    for (unsigned int s = 0; s < uk; ++s) {
      const int u = idx[row0 + s];
      if (u < 0) continue;
      const unsigned int uu = min((unsigned int)u, un - 1u);
      const float wt = w[row0 + s];
      float du[B];
      load_legs<B, LEGS_INNER>(dist_in, sn, uu, du);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float c = du[b] + wt;
        if (c < best[b]) {
          best[b] = c;
          bp[b] = (int)uu;
        }
      }
    }
  }

  // ---- in-lists: short ones by the owner, ascending ----
  const bool long_list = end - beg > LONG_LIST;
  if (!long_list) {
    for (int q = beg; q < end; ++q) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const unsigned int u = e / uk;
      const float wt = w[e];
      float du[B];
      load_legs<B, LEGS_INNER>(dist_in, sn, u, du);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float c = du[b] + wt;
        if (c < best[b]) {
          best[b] = c;
          bp[b] = (int)u;
        }
      }
    }
  }

  // ---- hub in-lists: the owner's whole wave walks them ----
  unsigned long long todo = __ballot(long_list);
  while (todo) {  // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int b0 = __shfl(beg, src);
    const int e0 = __shfl(end, src);
    float lc[B];
    int lq[B], lu[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      lc[b] = __builtin_inff();
      lq[b] = 0x7FFFFFFF;
      lu[b] = -1;
    }
    for (int q = b0 + lane; q < e0; q += 64) {  // q ascends within a lane
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const unsigned int u = e / uk;
      const float wt = w[e];
      float du[B];
      load_legs<B, LEGS_INNER>(dist_in, sn, u, du);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float c = du[b] + wt;
        if (c < lc[b]) {
          lc[b] = c;
          lq[b] = q;
          lu[b] = (int)u;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      for (int off = 32; off > 0; off >>= 1) {
        const float oc = __shfl_xor(lc[b], off);
        const int oq = __shfl_xor(lq[b], off);
        const int ou = __shfl_xor(lu[b], off);
        if (oc < lc[b] || (oc == lc[b] && oq < lq[b])) {
          lc[b] = oc;
          lq[b] = oq;
          lu[b] = ou;
        }
      }
      // every in-list position comes after the owner's own slots
      if (lane == src && lc[b] < best[b]) {
        best[b] = lc[b];
        bp[b] = lu[b];
      }
    }
  }
  if (!live) return;

  const bool open = allowed == nullptr || allowed[v] != 0;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    if (open) {
      if (best[b] < old[b]) changed[b] = 1;
    } else {
      best[b] = __builtin_inff();
      bp[b] = -1;
    }
  }
  store_legs<B, LEGS_INNER>(dist_out, sn, (unsigned int)v, best);
  store_legs<B, LEGS_INNER>(pred_out, sn, (unsigned int)v, bp);
}

// One lane per leg: out[b][0] = dst[b], then its predecessors, until src[b]
// is written, a predecessor is missing, or T+1 entries are out. The rest of
// the row is -1. count[b] is the number of entries, -1 when dst[b] was not
// reached.
__global__ void path_walk_kernel(const float* __restrict__ dist,
                                 const int* __restrict__ pred,
                                 const int* __restrict__ src,
                                 const int* __restrict__ dst,
                                 int* __restrict__ out, int* __restrict__ count,
                                 int n, int B, int T1, int legs_inner) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  // element (b, v) of dist / pred is at row + v * step
  const size_t row = legs_inner ? (size_t)b : (size_t)b * (size_t)n;
  const size_t step = legs_inner ? (size_t)B : 1;
  int* o = out + (size_t)b * (size_t)T1;
  const int s = src[b];
  int v = dst[b];
  int c = 0;
  const bool ok = v >= 0 && v < n && s >= 0 && s < n &&
                  dist[row + (size_t)min(max(v, 0), n - 1) * step] <
                      __builtin_inff();
  if (ok) {
    while (c < T1) {
      o[c++] = v;
      if (v == s) break;
      const int p = pred[row + (size_t)v * step];
      if (p < 0 || p >= n) break;
      v = p;
    }
  }
  for (int i = c; i < T1; ++i) o[i] = -1;
  count[b] = ok ? c : -1;
}

}  // namespace

// dist_in/pred_in/dist_out/pred_out (B, n), leg-major or (legs_inner)
// vertex-major and then 16-byte aligned; idx/w (n, k), in_off (n+1),
// in_edge (n_in), allowed (n) or null, changed (B). 1 <= B <= 8 and
// n*k < 2^31 are checked by the binding.
void launch_path_relax(const float* dist_in, const int* pred_in,
                       float* dist_out, int* pred_out, const int* idx,
                       const float* w, const int* in_off, const int* in_edge,
                       const unsigned char* allowed, int* changed, int B,
                       int n, int k, int n_in, int legs_inner,
                       hipStream_t stream) {
  if (n <= 0 || B < 1 || B > MAX_LEGS) return;
  dim3 grid((n + 255) / 256);
  dim3 block(256);
#define AM_RELAX_L(NB, INNER)                                                 \
  hipLaunchKernelGGL((path_relax_kernel<NB, INNER>), grid, block, 0, stream,  \
                     dist_in, pred_in, dist_out, pred_out, idx, w, in_off,    \
                     in_edge, allowed, changed, n, k, n_in)
#define AM_RELAX(NB)                                                          \
  case NB:                                                                    \
    if (legs_inner) AM_RELAX_L(NB, true);                                     \
    else AM_RELAX_L(NB, false);                                               \
    break
  switch (B) {
    AM_RELAX(1);
    AM_RELAX(2);
    AM_RELAX(3);
    AM_RELAX(4);
    AM_RELAX(5);
    AM_RELAX(6);
    AM_RELAX(7);
    AM_RELAX(8);
  }
#undef AM_RELAX
#undef AM_RELAX_L
}

void launch_path_walk(const float* dist, const int* pred, const int* src,
                      const int* dst, int* out, int* count, int B, int n,
                      int T1, int legs_inner, hipStream_t stream) {
  if (B <= 0 || n <= 0 || T1 <= 0) return;
  hipLaunchKernelGGL(path_walk_kernel, dim3(1), dim3(64), 0, stream, dist,
                     pred, src, dst, out, count, n, B, T1, legs_inner);
}

}  // namespace audiomuse
