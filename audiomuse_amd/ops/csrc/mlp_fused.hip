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

// ---------------------------------------------------------------------------
// C = 256 (stage 2), hidden 1024: the same computation and rounding points.
//
// The 32-token layout above, widened, needs xn[16], acc[8] and 32 KiB weight
// chunks and spills at two waves per SIMD. Here a wave owns 16 tokens and
// uses mfma_f32_16x16x32_bf16; a 512-thread workgroup owns 128 tokens.
// With lane = (tl = lane & 15, g = lane >> 4):
//   * xn[s], s = 0..7, holds channels 32s + 8g + j of token tl (B operand).
//   * The hidden dimension is walked in chunks of 32. GEMM1 is transposed,
//     two 16-row tiles t = 0, 1. Accumulator row r of tile t is fed W1 row
//     chunk*32 + 8(r >> 2) + 4t + (r & 3), so the lane's eight GELU'd values
//     (t, i) are element j = 4t + i of GEMM2's B operand, hidden unit
//     8g + j of the chunk: no LDS trip. The bias of xacc[t][i] is
//     b1[chunk*32 + 8g + 4t + i].
//   * GEMM2 is 16 tiles acc[ct], channel 16ct + 4g + i of token tl; its A
//     operand is W2[16ct + tl][chunk*32 + 8g .. + 8]. Each accumulator
//     starts as x2 + b2: x and proj are read a second time for this, in
//     accumulator layout (8-byte loads of lines the first read left hot).
//   * Weight chunks (16 KiB of W1, 16 KiB of W2) go through double-buffered
//     LDS, loaded two chunks ahead, one barrier per chunk; b1 sits in LDS
//     whole. The output tile is staged through the same LDS so rows leave
//     as full 512-byte lines.
//   * The LDS images are XOR-swizzled, not padded. ds_read_b128 serves a
//     wave in four groups of 16 lanes, each made of eight lanes of one g and
//     eight of the next: no row padding keeps tl + g (or 5 tl + g) apart in
//     all of them, and every read then costs twice. W1 row h of the chunk
//     sits at LDS row R = 16t + r (its tile and accumulator row) with its
//     16-byte slot cs at cs ^ r; W2 row c keeps its place with slot q at
//     q ^ (-(c >> 2) & 3). Both make the 16 lanes of every group hit 16
//     different slots.
// ---------------------------------------------------------------------------

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int M2_C = 256;
constexpr int M2_HID = 1024;
constexpr int M2_BM = 128;         // tokens per workgroup (8 waves x 16)
constexpr int M2_THREADS = 512;
constexpr int M2_CHUNK = 32;
constexpr int M2_NCHUNK = M2_HID / M2_CHUNK;
constexpr int V1_ROW = M2_C;                   // [32 rows][256 c]
constexpr int V2_ROW = M2_CHUNK;               // [256 c][32 hid]
constexpr int V1_ELEMS = M2_CHUNK * V1_ROW;    // 8192
constexpr int V2_ELEMS = M2_C * V2_ROW;        // 8192
constexpr int VBUF_ELEMS = V1_ELEMS + V2_ELEMS;  // 16384 (32 KiB)
constexpr int LDS2_ELEMS = 2 * VBUF_ELEMS + M2_HID;  // buffers, then b1
constexpr int VOUT_ROW = M2_C + 8;
// the staged output also covers b1's copy, which is dead by then
static_assert(M2_BM * VOUT_ROW <= LDS2_ELEMS, "output staging fits");

// one chunk's weights, global -> registers (32 KiB over 512 threads)
__device__ __forceinline__ void load_chunk2(const __bf16* __restrict__ W1,
                                            const __bf16* __restrict__ W2,
                                            int chunk, int tid,
                                            WeightRegs& r) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = tid + M2_THREADS * i;
    // W1 rows chunk*32 .. +31 are one contiguous 16 KiB run
    r.w1[i] = *(const bf16x8*)(W1 + chunk * M2_CHUNK * M2_C + p * 8);
    // W2[c][chunk*32 .. +31]: 64 B per channel row
    const int c = p >> 2, q = p & 3;
    r.w2[i] = *(const bf16x8*)(W2 + c * M2_HID + chunk * M2_CHUNK + q * 8);
  }
}

__device__ __forceinline__ void store_chunk2(__bf16* buf, int tid,
                                             const WeightRegs& r) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = tid + M2_THREADS * i;
    // W1 row h of the chunk -> tile t = (h >> 2) & 1, accumulator row r
    const int h = p >> 5, cs = p & 31;
    const int r1 = 4 * (h >> 3) + (h & 3);
    const int row = 16 * ((h >> 2) & 1) + r1;
    *(bf16x8*)(buf + row * V1_ROW + (cs ^ r1) * 8) = r.w1[i];
    const int c = p >> 2, q = p & 3;
    *(bf16x8*)(buf + V1_ELEMS + c * V2_ROW + (q ^ (-(c >> 2) & 3)) * 8) =
        r.w2[i];
  }
}

// One hidden chunk, as mlp_step: prefetch chunk + 2 into ld_set, compute
// from LDS buffer chunk & 1, park st_set (chunk + 1) in the other buffer.
// b1 is read from its LDS copy: a global load here would make the wave wait
// for the weight prefetch it has just issued. The operand fragments are
// read four at a time, two batches ahead of the MFMAs that use them, so
// GEMM2's first batches are in flight under the GELU; the scheduling
// barriers keep the compiler from sinking the reads back to their uses.
__device__ __forceinline__ void mlp2_step(
    int chunk, __bf16* lds, const __bf16* __restrict__ W1,
    const __bf16* __restrict__ W2, int tid, int tl, int g,
    WeightRegs& ld_set, WeightRegs& st_set, const bf16x8 (&xn)[8],
    f32x4 (&acc)[16]) {
  const __bf16* buf = lds + (chunk & 1) * VBUF_ELEMS;
  // No branch round the prefetch or the store below: behind one the compiler
  // must assume the older loads are the youngest and waits for every load
  // before the store, the prefetch just issued included. The last two steps
  // load the last chunk again and the last step parks it, unused.
  load_chunk2(W1, W2, chunk + 2 < M2_NCHUNK ? chunk + 2 : M2_NCHUNK - 1, tid,
              ld_set);
  const bf16x8 bia =
      *(const bf16x8*)(lds + 2 * VBUF_ELEMS + chunk * M2_CHUNK + 8 * g);
  const __bf16* w1b = buf + tl * V1_ROW;
  const __bf16* w2b =
      buf + V1_ELEMS + tl * V2_ROW + (g ^ (-(tl >> 2) & 3)) * 8;

  // Operand fragment q = 0..15 of GEMM1 is tile t = q & 1 of k-step q >> 1;
  // fragment q of GEMM2 is channel tile q. Batches of four rotate through
  // three register sets, each read two batches ahead of its MFMAs.
  bf16x8 f[3][4];
  auto read1 = [&](int set, int batch) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = 4 * batch + k;
      f[set][k] = *(const bf16x8*)(w1b + 16 * (q & 1) * V1_ROW +
                                   ((4 * (q >> 1) + g) ^ tl) * 8);
    }
  };
  auto read2 = [&](int set, int batch) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      f[set][k] = *(const bf16x8*)(w2b + (4 * batch + k) * 16 * V2_ROW);
  };
  f32x4 xacc[2];
  auto gemm1 = [&](int set, int batch) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = 4 * batch + k;
      xacc[q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          f[set][k], xn[q >> 1], xacc[q & 1], 0, 0, 0);
    }
  };
  bf16x8 hb;
  auto gemm2 = [&](int set, int batch) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      acc[4 * batch + k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          f[set][k], hb, acc[4 * batch + k], 0, 0, 0);
  };

  // ---- GEMM1 (transposed): X[hid][token] = b1 + W1 . LN(x2)^T, K = 256 ----
  read1(0, 0);
  read1(1, 1);
  read1(2, 2);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) xacc[t][i] = (float)bia[4 * t + i];
  __builtin_amdgcn_sched_barrier(0);
  gemm1(0, 0);
  read1(0, 3);
  __builtin_amdgcn_sched_barrier(0);
  gemm1(1, 1);
  read2(1, 0);
  __builtin_amdgcn_sched_barrier(0);
  gemm1(2, 2);
  read2(2, 1);
  __builtin_amdgcn_sched_barrier(0);
  gemm1(0, 3);
  read2(0, 2);
  __builtin_amdgcn_sched_barrier(0);

  // ---- GELU, packed as GEMM2's B operand (hidden unit 8g + 4t + i) ----
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) hb[4 * t + i] = (__bf16)gelu_tanh(xacc[t][i]);
  __builtin_amdgcn_sched_barrier(0);

  // ---- GEMM2: Y^T[c][token] += W2[c][hid] X[hid][token] ----
  gemm2(1, 0);
  read2(1, 3);
  __builtin_amdgcn_sched_barrier(0);
  gemm2(2, 1);
  gemm2(0, 2);
  gemm2(1, 3);

  store_chunk2(lds + ((chunk + 1) & 1) * VBUF_ELEMS, tid, st_set);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(512, 2) void mlp_fused_c256_kernel(
    const __bf16* __restrict__ x,     // (M, 256)
    const __bf16* __restrict__ proj,  // (M, 256)
    const __bf16* __restrict__ ln_w,  // (256)
    const __bf16* __restrict__ ln_b,  // (256)
    const __bf16* __restrict__ W1,    // (1024, 256)
    const __bf16* __restrict__ b1,    // (1024)
    const __bf16* __restrict__ W2,    // (256, 1024)
    const __bf16* __restrict__ b2,    // (256)
    __bf16* __restrict__ out,         // (M, 256)
    float eps) {
  // two weight buffers, then a copy of b1
  __shared__ __attribute__((aligned(16))) __bf16 lds[LDS2_ELEMS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int tl = lane & 15;   // token within the wave's 16
  const int g = lane >> 4;    // k-group of the operand, row group of C/D
  const long long tok = (long long)blockIdx.x * M2_BM + wave * 16 + tl;

  // b1 -> LDS, 4 bytes per thread (no branch: one between the accumulator
  // init below and the loop lets the compiler sink the init past it, holding
  // the raw inputs instead, and spill); visible after the first barrier
  *(bf16x2*)(lds + 2 * VBUF_ELEMS + 2 * tid) = *(const bf16x2*)(b1 + 2 * tid);

  // first chunks' weights in flight while the tile is normalised
  WeightRegs wr[2];
  load_chunk2(W1, W2, 0, tid, wr[0]);
  load_chunk2(W1, W2, 1, tid, wr[1]);

  bf16x8 xn[8];
  f32x4 acc[16];
  {
    const __bf16* xp = x + tok * M2_C + 8 * g;
    const __bf16* pp = proj + tok * M2_C + 8 * g;
    bf16x8 xv[8], pv[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      xv[s] = *(const bf16x8*)(xp + 32 * s);
      pv[s] = *(const bf16x8*)(pp + 32 * s);
    }
    // a token's 256 channels lie on the four lanes tl, tl + 16, .. + 48
    float sum = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += (float)xv[s][j] + (float)pv[s][j];
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / M2_C;
    float var = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = ((float)xv[s][j] + (float)pv[s][j]) - mean;
        var += d * d;
      }
    var += __shfl_xor(var, 16, 64);
    var += __shfl_xor(var, 32, 64);
    const float rstd = rsqrtf(var / M2_C + eps);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 lw = *(const bf16x8*)(ln_w + 32 * s + 8 * g);
      const bf16x8 lb = *(const bf16x8*)(ln_b + 32 * s + 8 * g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (float)xv[s][j] + (float)pv[s][j];
        const float f = (v - mean) * rstd;
        xn[s][j] = (__bf16)(f * (float)lw[j] + (float)lb[j]);
      }
    }
    // accumulator init: x2 (rounded to bf16) + b2 at channel 16ct + 4g + i;
    // kept behind the normalisation so its loads do not add to the
    // registers the packed inputs hold (hoisted, they spill)
    __builtin_amdgcn_sched_barrier(0);
    const __bf16* xa = x + tok * M2_C + 4 * g;
    const __bf16* pa = proj + tok * M2_C + 4 * g;
#pragma unroll
    for (int ct = 0; ct < 16; ++ct) {
      const bf16x4 xq = *(const bf16x4*)(xa + 16 * ct);
      const bf16x4 pq = *(const bf16x4*)(pa + 16 * ct);
      const bf16x4 bb = *(const bf16x4*)(b2 + 16 * ct + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[ct][i] = (float)(__bf16)((float)xq[i] + (float)pq[i]) +
                     (float)bb[i];
      // four tiles' loads in flight at a time: all 48 at once spill
      if ((ct & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }

  store_chunk2(lds, tid, wr[0]);
  __syncthreads();

  static_assert(M2_NCHUNK % 2 == 0, "two alternating sets");
  for (int chunk = 0; chunk < M2_NCHUNK; chunk += 2) {
    mlp2_step(chunk, lds, W1, W2, tid, tl, g, wr[0], wr[1], xn, acc);
    mlp2_step(chunk + 1, lds, W1, W2, tid, tl, g, wr[1], wr[0], xn, acc);
  }

  // ---- output: stage the 128 x 256 bf16 tile, store full rows ----
#pragma unroll
  for (int ct = 0; ct < 16; ++ct) {
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (__bf16)acc[ct][i];
    *(bf16x4*)(lds + (wave * 16 + tl) * VOUT_ROW + 16 * ct + 4 * g) = o;
  }
  __syncthreads();
  __bf16* ob = out + (long long)blockIdx.x * M2_BM * M2_C;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (tid >> 5) + 16 * i;
    const int col = (tid & 31) * 8;
    *(bf16x8*)(ob + row * M2_C + col) =
        *(const bf16x8*)(lds + row * VOUT_ROW + col);
  }
}

// M must be a multiple of 128 (checked by the binding).
void launch_mlp_fused_c256(const void* x, const void* proj, const void* ln_w,
                           const void* ln_b, const void* W1, const void* b1,
                           const void* W2, const void* b2, void* out,
                           long long M, float eps, hipStream_t stream) {
  hipLaunchKernelGGL(mlp_fused_c256_kernel, dim3((unsigned)(M / M2_BM)),
                     dim3(M2_THREADS), 0, stream, (const __bf16*)x,
                     (const __bf16*)proj, (const __bf16*)ln_w,
                     (const __bf16*)ln_b, (const __bf16*)W1, (const __bf16*)b1,
                     (const __bf16*)W2, (const __bf16*)b2, (__bf16*)out, eps);
}

}  // namespace audiomuse
