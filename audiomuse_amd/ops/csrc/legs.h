// Loads and stores of the B per-leg values of one vertex, shared by the
// pull sweeps over the kNN graph (path.hip, rank.hip).
//
// The (B, n) buffers of those sweeps come in one of two memory layouts:
// leg-major (row b is contiguous) or vertex-major (the B values of a vertex
// are contiguous, LEGS_INNER). Vertex-major is what the engines allocate:
// the B gathers of a candidate then fall into one 32-byte run and are read
// with 8- or 16-byte loads.
#pragma once

#include <hip/hip_runtime.h>

namespace audiomuse {

// The B values of vertex v. LEGS_INNER: p[v*B + b], read in the widest
// pieces B allows (the binding checks 16-byte alignment of the buffers);
// otherwise p[b*n + v].
template <int B, bool LEGS_INNER, typename T>
__device__ __forceinline__ void load_legs(const T* __restrict__ p, size_t n,
                                          unsigned int v, T (&out)[B]) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  if constexpr (LEGS_INNER && B % 4 == 0) {
    const int4* q = reinterpret_cast<const int4*>(p + (size_t)v * B);
#pragma unroll
    for (int i = 0; i < B / 4; ++i) {
      const int4 t = q[i];
      out[4 * i + 0] = __builtin_bit_cast(T, t.x);
      out[4 * i + 1] = __builtin_bit_cast(T, t.y);
      out[4 * i + 2] = __builtin_bit_cast(T, t.z);
      out[4 * i + 3] = __builtin_bit_cast(T, t.w);
    }
  } else if constexpr (LEGS_INNER && B % 2 == 0) {
    const int2* q = reinterpret_cast<const int2*>(p + (size_t)v * B);
#pragma unroll
    for (int i = 0; i < B / 2; ++i) {
      const int2 t = q[i];
      out[2 * i + 0] = __builtin_bit_cast(T, t.x);
      out[2 * i + 1] = __builtin_bit_cast(T, t.y);
    }
  } else if constexpr (LEGS_INNER) {
#pragma unroll
    for (int b = 0; b < B; ++b) out[b] = p[(size_t)v * B + b];
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) out[b] = p[b * n + v];
  }
}

template <int B, bool LEGS_INNER, typename T>
__device__ __forceinline__ void store_legs(T* __restrict__ p, size_t n,
                                           unsigned int v, const T (&in)[B]) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  if constexpr (LEGS_INNER && B % 4 == 0) {
    int4* q = reinterpret_cast<int4*>(p + (size_t)v * B);
#pragma unroll
    for (int i = 0; i < B / 4; ++i)
      q[i] = make_int4(__builtin_bit_cast(int, in[4 * i + 0]),
                       __builtin_bit_cast(int, in[4 * i + 1]),
                       __builtin_bit_cast(int, in[4 * i + 2]),
                       __builtin_bit_cast(int, in[4 * i + 3]));
  } else if constexpr (LEGS_INNER && B % 2 == 0) {
    int2* q = reinterpret_cast<int2*>(p + (size_t)v * B);
#pragma unroll
    for (int i = 0; i < B / 2; ++i)
      q[i] = make_int2(__builtin_bit_cast(int, in[2 * i + 0]),
                       __builtin_bit_cast(int, in[2 * i + 1]));
  } else if constexpr (LEGS_INNER) {
#pragma unroll
    for (int b = 0; b < B; ++b) p[(size_t)v * B + b] = in[b];
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) p[b * n + v] = in[b];
  }
}

}  // namespace audiomuse
