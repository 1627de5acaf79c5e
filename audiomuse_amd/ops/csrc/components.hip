// Connected components of the symmetrised kNN graph for gfx950 (CDNA4).
//
// graph_label_pull is one sweep of min-label propagation with a shortcut.
// Like path_relax (path.hip) and rank_pull (rank.hip) it is a pull pass:
// every vertex is computed and written by one owner lane from the input
// buffer only, so there are no atomics and the output is a pure function of
// the input. The torch statement of the same sweep is
// engines/graph_connect.label_pull_reference; the two agree bit for bit.
//
// For vertex v:
//   m            = min(label_in[v], label_in[u] for every candidate u)
//   label_out[v] = label_in[m]
// Candidates of v, as in the other graph kernels:
//   own slots s = 0..k-1   u = idx[v][s] (skipped when u < 0)
//   in-list positions      e = in_edge[q], u = e / k
// Labels start as label[v] = v. label[x] <= x with label[x] in x's component
// holds from then on, so the shortcut read label_in[m] is in range, never
// raises a label and jumps along the chain of representatives: the labels of
// a path of n vertices numbered in order settle in about log2 n sweeps where
// plain propagation takes n - 1. Numbered at random the same path still
// takes about n / 2 sweeps: the shortcut only helps along runs of falling
// ids, and the bound in general is the diameter, as for plain propagation.
// kNN graphs have small diameters. The fixed point is the smallest vertex id
// of each component.
//
// In-lists of up to LONG_LIST entries are walked by the owner lane; longer
// lists (hub vertices) are walked by the owner's whole wave, 64 entries at
// a time, and min-reduced. Every index read from memory is clamped into
// range, so malformed input gives wrong labels, never a wild read.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

constexpr int LONG_LIST = 64;

__global__ __launch_bounds__(256) void graph_label_pull_kernel(
    const int* __restrict__ label_in, int* __restrict__ label_out,
    const int* __restrict__ idx, const int* __restrict__ in_off,
    const int* __restrict__ in_edge, int* __restrict__ changed, int n, int k,
    int n_in) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // lanes past n stay in the kernel: the wave-wide walk below needs them
  const bool live = v < n;
  const unsigned int un = (unsigned int)n, uk = (unsigned int)k;
  const unsigned int n_edges = un * uk;  // < 2^31, checked by the binding

  int old = 0x7FFFFFFF, m = 0x7FFFFFFF;
  int beg = 0, end = 0;
  if (live) {
    old = m = label_in[v];
    beg = min(max(in_off[v], 0), n_in);
    end = min(max(in_off[v + 1], beg), n_in);

    // ---- own slots ----
    const unsigned int row0 = (unsigned int)v * uk;
    for (unsigned int s = 0; s < uk; ++s) {
      const int u = idx[row0 + s];
      if (u < 0) continue;
      m = min(m, label_in[min((unsigned int)u, un - 1u)]);
    }
  }

  // ---- in-lists: short ones by the owner ----
  const bool long_list = end - beg > LONG_LIST;
  if (!long_list) {
    for (int q = beg; q < end; ++q) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      m = min(m, label_in[e / uk]);
    }
  }

  // ---- hub in-lists: the owner's whole wave walks them ----
  unsigned long long todo = __ballot(long_list);
  while (todo) {  // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int b0 = __shfl(beg, src);
    const int e0 = __shfl(end, src);
    int lm = 0x7FFFFFFF;
    for (int q = b0 + lane; q < e0; q += 64) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      lm = min(lm, label_in[e / uk]);
    }
    for (int off = 32; off > 0; off >>= 1) lm = min(lm, __shfl_xor(lm, off));
    if (lane == src) m = min(m, lm);
  }
  if (!live) return;

  const int out = label_in[min(max(m, 0), n - 1)];
  if (out < old) changed[0] = 1;
  label_out[v] = out;
}

}  // namespace

// label_in/label_out (n), idx (n, k), in_off (n+1), in_edge (n_in), changed
// (1). n*k < 2^31 and the rest of the shapes are checked by the binding.
void launch_graph_label_pull(const int* label_in, int* label_out,
                             const int* idx, const int* in_off,
                             const int* in_edge, int* changed, int n, int k,
                             int n_in, hipStream_t stream) {
  if (n <= 0 || k <= 0) return;
  hipLaunchKernelGGL(graph_label_pull_kernel, dim3((n + 255) / 256), dim3(256),
                     0, stream, label_in, label_out, idx, in_off, in_edge,
                     changed, n, k, n_in);
}

}  // namespace audiomuse
