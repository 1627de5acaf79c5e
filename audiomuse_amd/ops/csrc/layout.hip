// One epoch of the 2-D map layout optimiser for gfx950 (CDNA4).
//
// Replaces the eager-torch SGD epoch of engines/projection.py (host RNG,
// mask compaction, six gather + index_add_ rounds) with one launch. The
// epoch is a pull formulation: every vertex is computed and written by
// one owner lane, so there are no atomics and the result is bit-identical
// from run to run. The torch statement of the same epoch is
// projection.layout_epoch_reference; the two take the same sampling
// decisions (integer hash below) and differ by float rounding only.
//
//   step 1  tail pulls: for every sampled in-edge (head j -> tail i),
//           acc += attract(E[j] - E[i]); p = E[i] - alpha * acc
//   step 2  own edges, sequential on the running p: for every sampled
//           slot s, p += alpha * attract(p - E[idx[i][s]]), then `neg`
//           times p += alpha * repel(p - E[negative])
//
// Step 1 is the only part with an unbounded trip count. In-edge lists of
// up to LONG_LIST entries are walked by the owner lane; longer lists (hub
// vertices) are walked by the owner's whole wave, 64 entries at a time,
// and reduced with a fixed shuffle tree.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

constexpr int LONG_LIST = 64;

struct Curve {
  float a, b;
  float c_att;  // -2ab
  float c_rep;  // 2b
};

__device__ __forceinline__ unsigned int mix32(unsigned int h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ float clamp4(float v) {
  return fminf(fmaxf(v, -4.0f), 4.0f);
}

__device__ __forceinline__ float2 attract(float dx, float dy, const Curve& c) {
  const float d2 = dx * dx + dy * dy;
  const float g = c.c_att * powf(fmaxf(d2, 1e-12f), c.b - 1.0f) /
                  (1.0f + c.a * powf(d2, c.b));
  return make_float2(clamp4(g * dx), clamp4(g * dy));
}

__device__ __forceinline__ float2 repel(float dx, float dy, const Curve& c) {
  const float d2 = dx * dx + dy * dy;
  const float g = c.c_rep / ((0.001f + d2) * (1.0f + c.a * powf(d2, c.b)));
  return make_float2(clamp4(g * dx), clamp4(g * dy));
}

// In-edge q of the reverse lists: its pull on a tail at (tx, ty), or zero
// when the edge is not sampled this epoch. Every index that addresses
// memory is clamped to its table.
__device__ __forceinline__ float2 tail_pull(const float2* __restrict__ E,
                                            const int* __restrict__ in_edge,
                                            const int* __restrict__ in_thr,
                                            int q, float tx, float ty,
                                            unsigned int base, unsigned int n,
                                            unsigned int k, const Curve& c) {
  const unsigned int e = (unsigned int)in_edge[q];
  const unsigned int t = (unsigned int)in_thr[q];
  if ((mix32(mix32(base + e)) >> 8) >= t) return make_float2(0.0f, 0.0f);
  const unsigned int j = min(e / k, n - 1u);
  const float2 h = E[j];
  return attract(h.x - tx, h.y - ty, c);
}

// NEG >= 0: compile-time count of negative samples; NEG < 0: neg_rt of
// them, loaded four at a time.
template <int NEG>
__global__ __launch_bounds__(256) void umap_epoch_kernel(
    const float2* __restrict__ E, float2* __restrict__ out,
    const int* __restrict__ idx, const int* __restrict__ thr,
    const int* __restrict__ in_off, const int* __restrict__ in_edge,
    const int* __restrict__ in_thr, int n, int k, int n_in, int neg_rt,
    float alpha, Curve c, unsigned int base) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // lanes past n stay in the kernel: the wave-wide walk below needs them
  const bool live = i < n;
  const unsigned int un = (unsigned int)n, uk = (unsigned int)k;

  float2 ei = make_float2(0.0f, 0.0f);
  int beg = 0, end = 0;
  if (live) {
    ei = E[i];
    beg = min(max(in_off[i], 0), n_in);
    end = min(max(in_off[i + 1], beg), n_in);
  }

  // ---- step 1: tail pulls, from the input positions on both ends ----
  const bool long_list = end - beg > LONG_LIST;
  float ax = 0.0f, ay = 0.0f;
  if (!long_list) {
    for (int q = beg; q < end; ++q) {
      const float2 f = tail_pull(E, in_edge, in_thr, q, ei.x, ei.y, base, un,
                                 uk, c);
      ax += f.x;
      ay += f.y;
    }
  }
  unsigned long long todo = __ballot(long_list);
  while (todo) {  // wave-uniform
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int b0 = __shfl(beg, src);
    const int e0 = __shfl(end, src);
    const float tx = __shfl(ei.x, src);
    const float ty = __shfl(ei.y, src);
    float sx = 0.0f, sy = 0.0f;
    for (int q = b0 + lane; q < e0; q += 64) {
      const float2 f = tail_pull(E, in_edge, in_thr, q, tx, ty, base, un, uk,
                                 c);
      sx += f.x;
      sy += f.y;
    }
    for (int off = 32; off > 0; off >>= 1) {
      sx += __shfl_xor(sx, off);
      sy += __shfl_xor(sy, off);
    }
    if (lane == src) {
      ax = sx;
      ay = sy;
    }
  }
  if (!live) return;

  float px = ei.x - alpha * ax;
  float py = ei.y - alpha * ay;

  // ---- step 2: own edges, sequential on the running position ----
  const unsigned int row0 = (unsigned int)i * uk;
  for (unsigned int s = 0; s < uk; ++s) {
    const unsigned int e = row0 + s;
    const unsigned int t = (unsigned int)thr[e];
    const unsigned int h0 = mix32(base + e);
    if ((mix32(h0) >> 8) >= t) continue;
    // none of the addresses depends on p: issue the loads, then the maths
    const unsigned int j = min((unsigned int)idx[e], un - 1u);
    const float2 nb = E[j];
    if constexpr (NEG >= 0) {
      float2 ng[NEG > 0 ? NEG : 1];
#pragma unroll
      for (int u = 0; u < NEG; ++u)
        ng[u] = E[__umulhi(mix32(h0 + 1u + (unsigned int)u), un)];
      const float2 f = attract(px - nb.x, py - nb.y, c);
      px += alpha * f.x;
      py += alpha * f.y;
#pragma unroll
      for (int u = 0; u < NEG; ++u) {
        const float2 r = repel(px - ng[u].x, py - ng[u].y, c);
        px += alpha * r.x;
        py += alpha * r.y;
      }
    } else {
      const float2 f = attract(px - nb.x, py - nb.y, c);
      px += alpha * f.x;
      py += alpha * f.y;
      for (int t0 = 0; t0 < neg_rt; t0 += 4) {
        // a draw past neg_rt is still a valid row: load all four, use
        // what counts
        float2 ng[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          ng[u] = E[__umulhi(mix32(h0 + 1u + (unsigned int)(t0 + u)), un)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (t0 + u < neg_rt) {
            const float2 r = repel(px - ng[u].x, py - ng[u].y, c);
            px += alpha * r.x;
            py += alpha * r.y;
          }
        }
      }
    }
  }
  out[i] = make_float2(px, py);
}

}  // namespace

// E/out (n, 2) f32, idx/thr (n, k) int32, in_off (n+1), in_edge/in_thr
// (n_in) int32: the reverse lists and the thresholds in list order. n*k
// must be below 2^31 (checked by the binding).
void launch_umap_epoch(const float* E, float* out, const int* idx,
                       const int* thr, const int* in_off, const int* in_edge,
                       const int* in_thr, int n, int k, int n_in, int neg,
                       float alpha, float a, float b, unsigned int seed,
                       unsigned int epoch, hipStream_t stream) {
  if (n <= 0) return;
  unsigned int base = seed ^ ((epoch + 1u) * 0x9E3779B9u);
  base ^= base >> 16;
  base *= 0x85EBCA6Bu;
  base ^= base >> 13;
  base *= 0xC2B2AE35u;
  base ^= base >> 16;
  Curve c;
  c.a = a;
  c.b = b;
  c.c_att = (float)(-2.0 * (double)a * (double)b);
  c.c_rep = (float)(2.0 * (double)b);
  dim3 grid((n + 255) / 256);
  dim3 block(256);
#define AM_EPOCH(NEG)                                                         \
  hipLaunchKernelGGL((umap_epoch_kernel<NEG>), grid, block, 0, stream,        \
                     reinterpret_cast<const float2*>(E),                      \
                     reinterpret_cast<float2*>(out), idx, thr, in_off,        \
                     in_edge, in_thr, n, k, n_in, neg, alpha, c, base)
  if (neg == 0) AM_EPOCH(0);
  else if (neg == 5) AM_EPOCH(5);
  else AM_EPOCH(-1);
#undef AM_EPOCH
}

}  // namespace audiomuse
