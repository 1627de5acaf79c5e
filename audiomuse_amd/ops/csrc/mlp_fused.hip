// Fused residual add + LayerNorm + MLP for the C = 128 encoder stage
// (gfx950, CDNA4):
//
//   x2  = x + proj
//   out = x2 + W2 . gelu_tanh(W1 . LN(x2) + b1) + b2
//
// The three-op path (add_layernorm_bf16 -> linear_gelu -> linear_bias_add)
// writes x2, LN(x2) and the 4C-wide hidden activation to HBM and reads
// them back: 15 activation-sized transfers for a computation whose true
// traffic is 3 (read x, read proj, write out). Here the normalised tile
// and the hidden activation never leave the CU.
//
// Rounding points are those of the three-op path: fp32 sum; LN statistics
// from the fp32 sum; x2 rounded to bf16 before it is the residual; LN
// output rounded to bf16; hidden rounded to bf16 after fp32 bias + GELU;
// fp32 MFMA accumulation. Only the summation order differs.
//
// Structure: a 256-thread workgroup owns 128 tokens, each wave 32 of them.
//   * The wave loads its tokens straight into the B-operand layout of
//     mfma_f32_32x32x16_bf16 (lane = token, 8 contiguous channels per
//     k-step), adds, normalises and keeps LN(x2) as 8 operand fragments.
//   * The hidden dimension is walked in chunks of 32. GEMM1 is computed
//     TRANSPOSED, X = W1chunk . LN(x2)^T (hidden unit on accumulator rows,
//     token on the lane), so after bias + GELU the packed accumulator is
//     directly the B operand of GEMM2, Y^T += W2chunk . X, with no LDS
//     round trip. The accumulator's rows reach a k-step in permuted order
//     (row 16s + 8(j>>2) + 4h + (j&3) for element j of lane half h); the
//     permutation is absorbed by assigning W1 rows to accumulator rows
//     with bits 2 and 3 swapped, after which both weight operands read
//     contiguous 16-byte runs.
//   * Y^T (4 tiles of 32 channels x 32 tokens, fp32) lives in registers for
//     the whole kernel, initialised with x2 + b2.
//   * Weight chunks (8 KiB of W1, 8 KiB of W2) are staged once per
//     workgroup through double-buffered, row-padded LDS; one barrier per
//     chunk. The output tile is staged through the same LDS so that rows
//     leave as full 256-byte lines.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MLP_C = 128;         // channels
constexpr int MLP_HID = 512;       // hidden width
constexpr int MLP_BM = 128;        // tokens per workgroup
constexpr int MLP_CHUNK = 32;      // hidden units per step
constexpr int MLP_NCHUNK = MLP_HID / MLP_CHUNK;
// Weight loads are issued this many chunks ahead, into as many register
// sets: one chunk of MFMA work does not cover a loaded L2's latency
// (measured 1.01 ms at distance 1, 0.97 ms at distance 2; a third wave per
// SIMD at 168 registers spills and is no faster at either distance).
constexpr int MLP_PF = 2;
// LDS images, in bf16 elements; rows padded by 16 B against bank conflicts
constexpr int W1_ROW = MLP_C + 8;              // [32 hid][128 c]
constexpr int W2_ROW = MLP_CHUNK + 8;          // [128 c][32 hid]
constexpr int W1_ELEMS = MLP_CHUNK * W1_ROW;   // 4352
constexpr int W2_ELEMS = MLP_C * W2_ROW;       // 5120
constexpr int BUF_ELEMS = W1_ELEMS + W2_ELEMS; // 9472 (18944 B)
constexpr int OUT_ROW = MLP_C + 8;             // output staging row
static_assert(MLP_BM * OUT_ROW <= 2 * BUF_ELEMS, "output staging fits");

// tanh-form GELU, 0.5 u (1 + tanh(z)) with z = 0.79788456 (u + 0.044715 u^3),
// written as u * sigmoid(2z) = u / (1 + 2^t), t = -2z log2(e): one v_exp
// and one v_rcp per element.
__device__ __forceinline__ float gelu_tanh(float u) {
  const float t = u * (-2.3022082f - 0.10294324f * u * u);
  return u * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}

struct WeightRegs {
  bf16x8 w1[2];
  bf16x8 w2[2];
};

// one chunk's weights, global -> registers (16 KiB over 256 threads)
__device__ __forceinline__ void load_chunk(const __bf16* __restrict__ W1,
                                           const __bf16* __restrict__ W2,
                                           int chunk, int tid, WeightRegs& r) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = tid + 256 * i;
    // W1 rows chunk*32 .. +31 are one contiguous 8 KiB run
    r.w1[i] = *(const bf16x8*)(W1 + (long long)chunk * MLP_CHUNK * MLP_C + p * 8);
    // W2[c][chunk*32 .. +31]: 64 B per channel row
    const int c = p >> 2, q = p & 3;
    r.w2[i] = *(const bf16x8*)(W2 + c * MLP_HID + chunk * MLP_CHUNK + q * 8);
  }
}

__device__ __forceinline__ void store_chunk(__bf16* buf, int tid,
                                            const WeightRegs& r) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = tid + 256 * i;
    *(bf16x8*)(buf + (p >> 4) * W1_ROW + (p & 15) * 8) = r.w1[i];
    *(bf16x8*)(buf + W1_ELEMS + (p >> 2) * W2_ROW + (p & 3) * 8) = r.w2[i];
  }
}

// One hidden chunk: prefetch the weights of chunk + MLP_PF into ld_set,
// GEMM1 -> bias + GELU -> GEMM2 from LDS buffer chunk & 1, then park
// st_set (chunk + 1, loaded MLP_PF - 1 steps ago) in the other buffer.
__device__ __forceinline__ void mlp_step(
    int chunk, __bf16* lds, const __bf16* __restrict__ W1,
    const __bf16* __restrict__ W2, const __bf16* __restrict__ b1, int tid,
    int w1row, int tl, int hh, WeightRegs& ld_set, WeightRegs& st_set,
    const bf16x8 (&xn)[8], f32x16 (&acc)[4]) {
  const __bf16* buf = lds + (chunk & 1) * BUF_ELEMS;
  if (chunk + MLP_PF < MLP_NCHUNK)
    load_chunk(W1, W2, chunk + MLP_PF, tid, ld_set);
  // accumulator register r of lane half h is hidden unit
  // chunk*32 + 16(r>>3) + 8h + (r&7)
  const bf16x8 bia0 = *(const bf16x8*)(b1 + chunk * MLP_CHUNK + 8 * hh);
  const bf16x8 bia1 = *(const bf16x8*)(b1 + chunk * MLP_CHUNK + 16 + 8 * hh);

  // ---- GEMM1 (transposed): X[hid][token] = b1 + W1 . LN(x2)^T, K = 128 ----
  f32x16 xacc;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    xacc[r] = (float)bia0[r];
    xacc[8 + r] = (float)bia1[r];
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const bf16x8 a = *(const bf16x8*)(buf + w1row * W1_ROW + 16 * s + 8 * hh);
    xacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xn[s], xacc, 0, 0, 0);
  }

  // ---- GELU, packed as GEMM2's B operand ----
  bf16x8 hb[2];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    hb[0][r] = (__bf16)gelu_tanh(xacc[r]);
    hb[1][r] = (__bf16)gelu_tanh(xacc[8 + r]);
  }

  // ---- GEMM2: Y^T[c][token] += W2[c][hid] X[hid][token] ----
  const __bf16* w2b = buf + W1_ELEMS + tl * W2_ROW + 8 * hh;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 a = *(const bf16x8*)(w2b + ct * 32 * W2_ROW + 16 * s);
      acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[s], acc[ct],
                                                        0, 0, 0);
    }

  if (chunk + 1 < MLP_NCHUNK)
    store_chunk(lds + ((chunk + 1) & 1) * BUF_ELEMS, tid, st_set);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(256, 2) void mlp_fused_c128_kernel(
    const __bf16* __restrict__ x,     // (M, 128)
    const __bf16* __restrict__ proj,  // (M, 128)
    const __bf16* __restrict__ ln_w,  // (128)
    const __bf16* __restrict__ ln_b,  // (128)
    const __bf16* __restrict__ W1,    // (512, 128)
    const __bf16* __restrict__ b1,    // (512)
    const __bf16* __restrict__ W2,    // (128, 512)
    const __bf16* __restrict__ b2,    // (128)
    __bf16* __restrict__ out,         // (M, 128)
    float eps) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BUF_ELEMS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int tl = lane & 31;   // token within the wave's 32
  const int hh = lane >> 5;   // lane half
  const long long tok =
      (long long)blockIdx.x * MLP_BM + wave * 32 + tl;

  // first chunks' weights in flight while the tile is normalised
  WeightRegs wr[MLP_PF];
#pragma unroll
  for (int k = 0; k < MLP_PF; ++k) load_chunk(W1, W2, k, tid, wr[k]);

  // ---- x2 = x + proj, LN(x2): lane (token, half) holds channels
  // 16s + 8h + j, s = 0..7, j = 0..7 (B-operand layout) ----
  bf16x8 xn[8];
  f32x16 acc[4];   // Y^T tiles: channel 32ct + (r&3) + 8(r>>2) + 4h, token tl
  {
    const __bf16* xp = x + tok * MLP_C + 8 * hh;
    const __bf16* pp = proj + tok * MLP_C + 8 * hh;
    bf16x8 xv[8], pv[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      xv[s] = *(const bf16x8*)(xp + 16 * s);
      pv[s] = *(const bf16x8*)(pp + 16 * s);
    }
    // the fp32 sums are recomputed from the packed inputs in each pass
    // rather than held: 64 fewer live registers
    float sum = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += (float)xv[s][j] + (float)pv[s][j];
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / MLP_C;
    float var = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = ((float)xv[s][j] + (float)pv[s][j]) - mean;
        var += d * d;
      }
    var += __shfl_xor(var, 32, 64);
    const float rstd = rsqrtf(var / MLP_C + eps);

    // Accumulator init, x2 (rounded to bf16) + b2, rides the same pass.
    // The accumulator wants, for lane half h, the channels whose bit 2 is
    // h; the operand layout gave this lane those whose bit 3 is h. Each
    // lane keeps the 4-channel group with bit 2 == bit 3 == h and trades
    // the other with lane ^ 32.
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 lw = *(const bf16x8*)(ln_w + 16 * s + 8 * hh);
      const bf16x8 lb = *(const bf16x8*)(ln_b + 16 * s + 8 * hh);
      float x2r[8];   // x2 as the residual: rounded to bf16
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (float)xv[s][j] + (float)pv[s][j];
        const float f = (v - mean) * rstd;
        xn[s][j] = (__bf16)(f * (float)lw[j] + (float)lb[j]);
        x2r[j] = (float)(__bf16)v;
      }
      const int ct = s >> 1;
      const int g0 = 2 * (s & 1);   // accumulator row groups g0, g0 + 1
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // lo = channel 16s + 8h + i, hi = channel 16s + 8h + 4 + i
        const float keep = hh ? x2r[4 + i] : x2r[i];   // 16s + 12h + i
        const float send = hh ? x2r[i] : x2r[4 + i];
        const float recv = __shfl_xor(send, 32, 64);  // 16s + 8(1-h) + 4h + i
        // row group g holds channel bit 3 == (g & 1)
        acc[ct][4 * g0 + i] = hh ? recv : keep;        // bit 3 == 0
        acc[ct][4 * (g0 + 1) + i] = hh ? keep : recv;  // bit 3 == 1
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const bf16x4 bb = *(const bf16x4*)(b2 + 32 * ct + 8 * g + 4 * hh);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[ct][4 * g + i] += (float)bb[i];
      }
  }

  store_chunk(lds, tid, wr[0]);
  __syncthreads();

  // W1 row read by this lane: accumulator row tl <-> hidden unit with
  // bits 2 and 3 of tl swapped
  const int w1row = (tl & 19) | ((tl & 4) << 1) | ((tl & 8) >> 1);

  // step i loads chunk i + 2 into set i % 2 (free: chunk i is already in
  // LDS) and parks set (i + 1) % 2, which holds chunk i + 1
  static_assert(MLP_PF == 2 && MLP_NCHUNK % 2 == 0, "two alternating sets");
  for (int chunk = 0; chunk < MLP_NCHUNK; chunk += 2) {
    mlp_step(chunk, lds, W1, W2, b1, tid, w1row, tl, hh, wr[0], wr[1], xn,
             acc);
    mlp_step(chunk + 1, lds, W1, W2, b1, tid, w1row, tl, hh, wr[1], wr[0],
             xn, acc);
  }

  // ---- output: stage the 128 x 128 bf16 tile, store full rows ----
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (__bf16)acc[ct][4 * g + i];
      *(bf16x4*)(lds + (wave * 32 + tl) * OUT_ROW + 32 * ct + 8 * g + 4 * hh) = o;
    }
  __syncthreads();
  __bf16* ob = out + (long long)blockIdx.x * MLP_BM * MLP_C;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (tid >> 4) + 16 * i;
    const int col = (tid & 15) * 8;
    *(bf16x8*)(ob + row * MLP_C + col) = *(const bf16x8*)(lds + row * OUT_ROW + col);
  }
}

// M must be a multiple of 128 (checked by the binding).
void launch_mlp_fused_c128(const void* x, const void* proj, const void* ln_w,
                           const void* ln_b, const void* W1, const void* b1,
                           const void* W2, const void* b2, void* out,
                           long long M, float eps, hipStream_t stream) {
  hipLaunchKernelGGL(mlp_fused_c128_kernel, dim3((unsigned)(M / MLP_BM)),
                     dim3(256), 0, stream, (const __bf16*)x,
                     (const __bf16*)proj, (const __bf16*)ln_w,
                     (const __bf16*)ln_b, (const __bf16*)W1, (const __bf16*)b1,
                     (const __bf16*)W2, (const __bf16*)b2, (__bf16*)out, eps);
}

}  // namespace audiomuse
