// Louvain local moving over the symmetrised kNN graph for gfx950 (CDNA4).
//
// community_move is one synchronous sweep: every vertex v is computed and
// written by one owner lane from the sweep's input buffers only, so there
// are no atomics, and because every sum is an integer sum the result equals
// its torch statement (engines/graph_community.move_reference) bit for bit.
//
// Candidates of vertex v, as in rank.hip, without those that are v itself:
//   own slots j = 0..k-1   u = idx[v][j] (skipped when u < 0), weight w[v][j]
//   in-list positions      e = in_edge[q], u = e / k, weight w.flat[e]
// With L = label_in[v], the candidate communities are the labels of the own-
// slot neighbours, K[c] the weight of all candidates whose label is c, and
//   stay     = K[L] * A - g * deg[v] * (tot[L] - deg[v])
//   score[c] = K[c] * A - g * deg[v] * tot[c]                  (all int64)
// label_out[v] is the c != L with score[c] > stay, c > L (up) or c < L
// (down), of highest score, ties to the smallest c; else L.
//
// The (label, sum) pairs of a lane. A lane holds KMAX labels and KMAX sums,
// and every candidate is matched against all of them. Indexed by a runtime
// slot number the two arrays would live in scratch, so they are only ever
// indexed by the counters of fully unrolled loops and stay in registers:
// the labels are filled by an unrolled pass over the own slots, and each
// candidate then costs one label gather and KMAX compare-and-adds. A label
// that fills two slots gets the same sum in both, hence the same score. The
// other way to keep them out of scratch, a per-lane LDS slice of 33 pairs,
// costs 66 KB a block and leaves 2 blocks per CU for a kernel that is bound
// by its random gathers; this one needs no LDS
// (profiles/r13_resource_usage.txt: 0 scratch at both KMAX).
//
// In-lists of up to LONG_LIST entries are walked by the owner lane; longer
// lists (hub vertices) by the owner's whole wave, 64 entries at a time: the
// owner's labels are broadcast, every lane sums the matches of its own
// positions, an xor-butterfly adds the 64 partial sums, and the owner adds
// the totals to its own. Integer addition makes the order irrelevant.
// K fits int32: the driver keeps max(64, g) * max_deg * two_m < 2^62, so
// max_deg < 2^28.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

constexpr int LONG_LIST = 64;

template <int KMAX>
__global__ __launch_bounds__(256) void community_move_kernel(
    const int* __restrict__ label_in, int* __restrict__ label_out,
    const long long* __restrict__ tot, const long long* __restrict__ deg,
    const int* __restrict__ idx, const int* __restrict__ w,
    const int* __restrict__ in_off, const int* __restrict__ in_edge,
    long long A, long long g, int up, int n, int k, int n_in) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // lanes past n stay in the kernel: the wave-wide walk below needs them
  const bool live = v < n;
  const unsigned int un = (unsigned int)n, uk = (unsigned int)k;
  const unsigned int n_edges = un * uk;  // < 2^31, checked by the binding
  const int top = n - 1;

  int lab[KMAX], K[KMAX];
  int L = -1, KL = 0;
  int beg = 0, end = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    lab[j] = -1;  // matches no label: those are clamped into [0, n)
    K[j] = 0;
  }

#define AM_MATCH(LABS, SUMS, HOME, HOME_SUM, lu, wt)                          \
  do {                                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < KMAX; ++i_)                       \
        SUMS[i_] += (LABS[i_] == (lu)) ? (wt) : 0;                            \
    HOME_SUM += ((HOME) == (lu)) ? (wt) : 0;                                  \
  } while (0)

  if (live) {
    L = min(max(label_in[v], 0), top);
    beg = min(max(in_off[v], 0), n_in);
    end = min(max(in_off[v + 1], beg), n_in);

    // ---- own slots: the candidate communities, then their sums ----
    const unsigned int row0 = (unsigned int)v * uk;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < k) {
        const int u = idx[row0 + j];
        const int uu = min(max(u, 0), top);
        if (u >= 0 && uu != v) lab[j] = min(max(label_in[uu], 0), top);
      }
    }
    for (unsigned int j = 0; j < uk; ++j) {
      const int u = idx[row0 + j];
      if (u < 0) continue;
      const int uu = min(u, top);
      if (uu == v) continue;
      const int wt = w[row0 + j];
      const int lu = min(max(label_in[uu], 0), top);
      AM_MATCH(lab, K, L, KL, lu, wt);
    }
  }

  // ---- in-lists: short ones by the owner ----
  const bool long_list = end - beg > LONG_LIST;
  if (!long_list) {
    for (int q = beg; q < end; ++q) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const int u = (int)(e / uk);
      if (u == v) continue;
      const int wt = w[e];
      const int lu = min(max(label_in[u], 0), top);
      AM_MATCH(lab, K, L, KL, lu, wt);
    }
  }

  // ---- hub in-lists: the owner's whole wave walks them ----
  unsigned long long todo = __ballot(long_list);
  while (todo) {  // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int b0 = __shfl(beg, src);
    const int e0 = __shfl(end, src);
    const int v0 = __shfl(v, src);
    const int L0 = __shfl(L, src);
    int lab0[KMAX], part[KMAX];
    int partL = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      lab0[j] = __shfl(lab[j], src);
      part[j] = 0;
    }
    for (int q = b0 + lane; q < e0; q += 64) {
      const unsigned int e =
          min((unsigned int)max(in_edge[q], 0), n_edges - 1u);
      const int u = (int)(e / uk);
      if (u == v0) continue;
      const int wt = w[e];
      const int lu = min(max(label_in[u], 0), top);
      AM_MATCH(lab0, part, L0, partL, lu, wt);
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      for (int off = 32; off > 0; off >>= 1)
        part[j] += __shfl_xor(part[j], off);
      if (lane == src) K[j] += part[j];
    }
    for (int off = 32; off > 0; off >>= 1) partL += __shfl_xor(partL, off);
    if (lane == src) KL += partL;
  }
#undef AM_MATCH
  if (!live) return;

  // ---- the move ----
  const long long dv = deg[v];
  const long long gd = g * dv;
  const long long stay = (long long)KL * A - gd * (tot[L] - dv);
  int best = L;
  long long best_score = stay;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const int c = lab[j];
    if (c >= 0 && c != L && (up ? c > L : c < L)) {
      const long long sc = (long long)K[j] * A - gd * tot[c];
      if (sc > best_score || (sc == best_score && best != L && c < best)) {
        best = c;
        best_score = sc;
      }
    }
  }
  label_out[v] = best;
}

}  // namespace

// label_in/label_out (n) int32, tot/deg (n) int64, idx/w (n, k) int32,
// in_off (n+1), in_edge (n_in). 1 <= k <= 32, n*k < 2^31, A > 0 and g >= 1
// are checked by the binding.
void launch_community_move(const int* label_in, int* label_out,
                           const long long* tot, const long long* deg,
                           const int* idx, const int* w, const int* in_off,
                           const int* in_edge, long long A, long long g,
                           int up, int n, int k, int n_in,
                           hipStream_t stream) {
  if (n <= 0 || k < 1 || k > 32) return;
  dim3 grid((n + 255) / 256);
  dim3 block(256);
  if (k <= 16)
    hipLaunchKernelGGL((community_move_kernel<16>), grid, block, 0, stream,
                       label_in, label_out, tot, deg, idx, w, in_off, in_edge,
                       A, g, up, n, k, n_in);
  else
    hipLaunchKernelGGL((community_move_kernel<32>), grid, block, 0, stream,
                       label_in, label_out, tot, deg, idx, w, in_off, in_edge,
                       A, g, up, n, k, n_in);
}

}  // namespace audiomuse
