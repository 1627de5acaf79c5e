// One-launch 4x4 patch embedding for the HTSAT encoder (gfx950).
//
// Replaces pad/crop -> patchify (permute + reshape copy) -> K = 16 GEMM:
// each output token gathers its 4x4 patch straight from the (B, n_mels, T)
// bf16 mel tensor. Frames T..n_frames read as zero, frames past n_frames are
// never touched. fp32 accumulation in k order, bias added in fp32, one
// rounding to bf16.
//
// The kernel is store-bound (C bf16 per 16 inputs). A workgroup takes one
// (clip, patch row) at a time: it stages the four mel rows in LDS (8 KiB at 1024
// frames; rows are only 2-byte aligned when T is odd, so the staging loads
// are scalar and coalesced), then every lane keeps the 16 x 8 weights of
// its eight channels in registers, as channel pairs for packed fp32 FMAs,
// and writes one 16-byte store per token: C / 8 lanes cover a token, so a
// wave's store instruction is contiguous. A workgroup walks several patch
// rows so the weights are fetched and unpacked once.

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace audiomuse {

__device__ __forceinline__ float pe_bf16_to_f32(unsigned v) {
  return __uint_as_float(v << 16);
}

__device__ __forceinline__ unsigned pe_f32_to_bf16(float f) {  // RNE
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

typedef float pe_f32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void patch_embed_bf16_kernel(
    const uint16_t* __restrict__ mel,     // (B, n_mels, T)
    const uint16_t* __restrict__ weight,  // (C, 16), k = 4 * mel_row + frame
    const uint16_t* __restrict__ bias,    // (C)
    uint16_t* __restrict__ out,           // (B, n_mels/4 * n_frames/4, C)
    int n_rows,                           // B * n_mels / 4 patch rows
    int n_mels, int T, int n_frames, int C) {
  extern __shared__ uint16_t tile[];      // 4 rows x n_frames, zero-padded

  const int tid = threadIdx.x;
  const int H = n_mels >> 2, W = n_frames >> 2;

  const int lanes_per_tok = C >> 3;       // power of two in [1, 256]
  const int tok_per_iter = 256 / lanes_per_tok;
  const int ts = tid / lanes_per_tok;
  const int c0 = (tid - ts * lanes_per_tok) << 3;

  // This lane's eight channels as four pairs: 16 weights each, once per
  // workgroup (a weight row is 32 bytes: two 16-byte loads).
  pe_f32x2 w[4][16], bs[4];
#pragma unroll
  for (int c2 = 0; c2 < 4; ++c2) {
    const int c = c0 + 2 * c2;
    bs[c2] = pe_f32x2{pe_bf16_to_f32(bias[c]), pe_bf16_to_f32(bias[c + 1])};
    const uint4* wr = reinterpret_cast<const uint4*>(weight + c * 16);
    const uint4 q[4] = {wr[0], wr[1], wr[2], wr[3]};   // rows c, c + 1
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
      const unsigned* lo = &q[0].x;
      const unsigned a = lo[k >> 1], d = lo[8 + (k >> 1)];
      w[c2][k] = pe_f32x2{pe_bf16_to_f32(a & 0xffffu),
                          pe_bf16_to_f32(d & 0xffffu)};
      w[c2][k + 1] = pe_f32x2{pe_bf16_to_f32(a >> 16),
                              pe_bf16_to_f32(d >> 16)};
    }
  }

  for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int b = row / H;
    const int h = row - b * H;
    const uint16_t* src = mel + ((long long)b * n_mels + 4 * h) * T;
    for (int i = tid; i < 4 * n_frames; i += 256) {
      const int r = i / n_frames;
      const int f = i - r * n_frames;
      tile[i] = f < T ? src[(long long)r * T + f] : (uint16_t)0;
    }
    __syncthreads();

    uint16_t* dst = out + (long long)row * W * C + c0;
    for (int t = ts; t < W; t += tok_per_iter) {
      float x[16];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint2 v =
            *reinterpret_cast<const uint2*>(&tile[r * n_frames + 4 * t]);
        x[4 * r + 0] = pe_bf16_to_f32(v.x & 0xffffu);
        x[4 * r + 1] = pe_bf16_to_f32(v.x >> 16);
        x[4 * r + 2] = pe_bf16_to_f32(v.y & 0xffffu);
        x[4 * r + 3] = pe_bf16_to_f32(v.y >> 16);
      }
      unsigned o[4];
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2) {
        pe_f32x2 acc = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          acc = __builtin_elementwise_fma(pe_f32x2{x[k], x[k]}, w[c2][k], acc);
        acc += bs[c2];
        o[c2] = pe_f32_to_bf16(acc.x) | (pe_f32_to_bf16(acc.y) << 16);
      }
      *reinterpret_cast<uint4*>(dst + (long long)t * C) =
          make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();                      // tile is restaged for the next row
  }
}

void launch_patch_embed_bf16(const void* mel, const void* weight,
                             const void* bias, void* out, int Bn, int n_mels,
                             int T, int n_frames, int C, hipStream_t stream) {
  const size_t lds = sizeof(uint16_t) * 4 * (size_t)n_frames;
  const int n_rows = Bn * (n_mels / 4);
  // a few patch rows per workgroup: the weights are unpacked once for all
  const int grid = n_rows < 2048 ? n_rows : 2048;
  hipLaunchKernelGGL(patch_embed_bf16_kernel, dim3(grid), dim3(256), lds,
                     stream, static_cast<const uint16_t*>(mel),
                     static_cast<const uint16_t*>(weight),
                     static_cast<const uint16_t*>(bias),
                     static_cast<uint16_t*>(out), n_rows, n_mels, T, n_frames,
                     C);
}

}  // namespace audiomuse
