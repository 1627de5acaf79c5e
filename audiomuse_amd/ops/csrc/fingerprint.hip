// Batched fingerprint alignment for gfx950 (CDNA4).
//
// The batched form of engines/chromaprint.bit_match_ratio: for every pair
// of fingerprints, slide one over the other by every offset in
// [-max_offset, max_offset], count the differing bits over the overlap
// and keep the alignment with the smallest bits / n. Everything is
// integer: fractions are compared by cross-multiplication in 64 bits and,
// among equal fractions, the lowest offset wins, which is what the
// sequential host scan keeps. The result does not depend on how the
// offsets are spread over waves and is bit-identical from run to run.
//
//   o >= 0 compares a[o:] with b;  o < 0 compares a with b[-o:]
//   n = length of the overlap; alignments with n < min_words are skipped
//   bits = popcount(xor) over all 32 bits of each of the n words
//
// One workgroup per pair. Both fingerprints are staged in LDS once and
// read 2 * max_offset + 1 times. An offset o < 0 of (a, b) is the shift
// d = -o of (b, a), so both signs are "compare X[d + i] with Y[i]". A wave
// takes FP_SHIFTS consecutive shifts at a time and its lanes stride over
// the overlap: consecutive lanes read consecutive LDS words (no bank
// conflicts) and each Y[i] is read once for FP_SHIFTS comparisons. The
// kernel is bound by LDS reads; scoring 1 / 2 / 4 / 8 shifts side by side
// took 27.3 / 19.9 / 17.5 / 16.6 ms for 1.5M pairs of 969 words
// (profiles/r7_fingerprint_align.txt). One shuffle tree per offset, one
// LDS hand-off between waves, plain stores, no atomics.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_SHIFTS = 8;  // shifts a wave scores side by side

// true when (bits, n, off) is a better alignment than (bbits, bn, boff);
// bn == 0 means "none yet". bits <= 32 * 4096 and n <= 4096, so the
// products are far inside 64 bits.
__device__ __forceinline__ bool fp_better(int bits, int n, int off, int bbits,
                                          int bn, int boff) {
  if (n == 0) return false;
  if (bn == 0) return true;
  const long long lhs = (long long)bits * bn;
  const long long rhs = (long long)bbits * n;
  return lhs < rhs || (lhs == rhs && off < boff);
}

__global__ __launch_bounds__(FP_THREADS) void fp_align_kernel(
    const unsigned int* __restrict__ words, const long long* __restrict__ off,
    const int* __restrict__ pairs, int* __restrict__ out, long long W, int F,
    int max_offset, int min_words, int lds_words) {
  extern __shared__ unsigned int fp_smem[];
  unsigned int* sa = fp_smem;
  unsigned int* sb = fp_smem + lds_words;
  int* red = reinterpret_cast<int*>(fp_smem + 2 * lds_words);

  const long long p = blockIdx.x;
  const int tid = threadIdx.x;
  const int ia = pairs[2 * p];
  const int ib = pairs[2 * p + 1];

  // The wrapper validates the bank and the pair indices before the
  // launch; these tests only keep a caller who skipped that from reading
  // outside `words` or writing outside the LDS carve. Every condition is
  // uniform over the workgroup, so the early exit is taken by all threads
  // or by none, ahead of any barrier.
  long long a0 = 0, b0 = 0;
  int la = 0, lb = 0;
  bool ok = ia >= 0 && ia < F && ib >= 0 && ib < F;
  if (ok) {
    a0 = off[ia];
    b0 = off[ib];
    const long long a1 = off[ia + 1];
    const long long b1 = off[ib + 1];
    ok = a0 >= 0 && a1 >= a0 && a1 <= W && a1 - a0 <= lds_words && b0 >= 0 &&
         b1 >= b0 && b1 <= W && b1 - b0 <= lds_words;
    la = ok ? (int)(a1 - a0) : 0;
    lb = ok ? (int)(b1 - b0) : 0;
  }
  if (!ok || la < min_words || lb < min_words) {
    if (tid < 3) out[3 * p + tid] = 0;
    return;
  }

  for (int i = tid; i < la; i += FP_THREADS) sa[i] = words[a0 + i];
  for (int i = tid; i < lb; i += FP_THREADS) sb[i] = words[b0 + i];
  __syncthreads();

  const int wave = tid >> 6;
  const int lane = tid & 63;
  int best_bits = 0, best_n = 0, best_off = 0;  // tracked by lane 0

  // blocks of FP_SHIFTS consecutive shifts d, n = min(lx - d, ly):
  // (X, Y) = (a, b) for o = d >= 0, then (b, a) for o = -d < 0
  // (d = 0 .. max_offset on the first side, 1 .. max_offset on the second)
  const int blocks_pos = (max_offset + FP_SHIFTS) / FP_SHIFTS;
  const int blocks_neg = (max_offset + FP_SHIFTS - 1) / FP_SHIFTS;
  // the first waves get one block more: rotate who is first by workgroup
  const int first = (wave + (int)(p & (FP_WAVES - 1))) & (FP_WAVES - 1);
  for (int blk = first; blk < blocks_pos + blocks_neg; blk += FP_WAVES) {
    const bool neg = blk >= blocks_pos;
    const int d0 =
        neg ? 1 + (blk - blocks_pos) * FP_SHIFTS : blk * FP_SHIFTS;
    const unsigned int* X = neg ? sb : sa;
    const unsigned int* Y = neg ? sa : sb;
    const int lx = neg ? lb : la;
    const int ly = neg ? la : lb;
    // overlap per shift, 0 for a shift that is skipped: n_all words are
    // compared at every shift of the block, the rest under a test per shift
    int n[FP_SHIFTS];
    int n_all = 1 << 30, n_any = 0;
#pragma unroll
    for (int k = 0; k < FP_SHIFTS; ++k) {
      const int d = d0 + k;
      int nk = min(lx - d, ly);
      if (d > max_offset || nk < min_words) nk = 0;
      n[k] = nk;
      n_all = min(n_all, nk);
      n_any = max(n_any, nk);
    }
    if (n_any == 0) continue;  // uniform over the wave
    const unsigned int* Xd = X + d0;
    int acc[FP_SHIFTS];
#pragma unroll
    for (int k = 0; k < FP_SHIFTS; ++k) acc[k] = 0;
    int i = lane;
    for (; i < n_all; i += 64) {
      const unsigned int y = Y[i];
#pragma unroll
      for (int k = 0; k < FP_SHIFTS; ++k) acc[k] += __popc(Xd[i + k] ^ y);
    }
    for (; i < n_any; i += 64) {
      const unsigned int y = Y[i];
#pragma unroll
      for (int k = 0; k < FP_SHIFTS; ++k)
        if (i < n[k]) acc[k] += __popc(Xd[i + k] ^ y);
    }
#pragma unroll
    for (int k = 0; k < FP_SHIFTS; ++k) {
      int v = acc[k];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
      const int o = neg ? -(d0 + k) : d0 + k;
      if (fp_better(v, n[k], o, best_bits, best_n, best_off)) {
        best_bits = v;
        best_n = n[k];
        best_off = o;
      }
    }
  }

  if (lane == 0) {
    red[3 * wave + 0] = best_bits;
    red[3 * wave + 1] = best_n;
    red[3 * wave + 2] = best_off;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < FP_WAVES; ++w) {
      const int bits = red[3 * w], n = red[3 * w + 1], o = red[3 * w + 2];
      if (fp_better(bits, n, o, best_bits, best_n, best_off)) {
        best_bits = bits;
        best_n = n;
        best_off = o;
      }
    }
    out[3 * p + 0] = best_bits;
    out[3 * p + 1] = best_n;
    out[3 * p + 2] = best_n > 0 ? best_off : 0;
  }
}

}  // namespace

// words (W) uint32 bit patterns; off (F + 1) int64; pairs (P, 2) int32;
// out (P, 3) int32. lds_words is the LDS room per fingerprint: no
// fingerprint named by `pairs` may be longer (a longer one scores 0, 0, 0).
void launch_fp_align(const int* words, const long long* off, const int* pairs,
                     int* out, long long W, int F, long long P, int max_offset,
                     int min_words, int lds_words, hipStream_t stream) {
  if (P <= 0) return;
  const size_t smem =
      (2 * (size_t)lds_words + 3 * FP_WAVES) * sizeof(unsigned int);
  hipLaunchKernelGGL(fp_align_kernel, dim3((unsigned int)P), dim3(FP_THREADS),
                     smem, stream,
                     reinterpret_cast<const unsigned int*>(words), off, pairs,
                     out, W, F, max_offset, min_words, lds_words);
}

}  // namespace audiomuse
