// One-launch attention half of a C = 128 encoder block (gfx950, CDNA4):
//
//   proj = Wp . attn(Wqkv . LN(x) + bqkv) + bp        (window 8x8, 4 heads)
//
// The four-launch path (layernorm_bf16 -> QKV GEMM -> window_attn_kernel ->
// proj GEMM) moves 12 activation-sized tensors through HBM for a
// computation whose true traffic is 2 (read x, write proj): everything in
// between is per-window. Here a 256-thread workgroup owns one 8x8 window
// and the normalised tile, q/k/v, P and O never leave the CU.
//
// Rounding points are those of the four-launch path: fp32 LN statistics,
// LN output rounded to bf16; q, k, v rounded to bf16 after the fp32 bias;
// P and O rounded to bf16; proj rounded to bf16 after the fp32 bias; fp32
// MFMA accumulation throughout. Only the summation order differs. The
// kernel writes proj, not x + proj: mlp_fused_c128_kernel takes (x, proj).
//
// Structure (mfma_f32_16x16x32_bf16 everywhere; A and B operands share one
// lane map: row|col = lane&15, k = 8*(lane>>4) + j; C/D: col = lane&15,
// row = 4*(lane>>4) + reg):
//   1. 16 lanes per token row gather x (roll + wrap as window_attn_kernel),
//      LayerNorm it and store the 64 x 128 bf16 tile to LDS (buffer A,
//      16-byte chunks XOR-swizzled by the row).
//   2. Wave h is head h. It reads the whole tile once as 16 operand
//      fragments and multiplies it with its 96 rows of qkv.weight, whose
//      fragments come straight from global/L2 (no weight element is used
//      by two waves).
//        Q^T, K^T = W . LN^T   -> lane holds one token, 4 consecutive d per
//                                 16-wide d tile
//        V        = LN . Wv^T  -> lane holds one d, 4 consecutive tokens per
//                                 16-wide token tile
//      Two accumulator tiles packed together are an operand fragment whose
//      k index is permuted (element j of lane group g is index
//      16*(j>>2) + 4g + (j&3) of a 32-wide k-step). A contraction does not
//      care about the order of its index as long as both operands agree,
//      and they do:  S^T = K . Q^T  contracts d with both operands in the
//      Q^T/K^T form;  O^T = V^T . P^T  contracts the key token with V in
//      the form above and P^T = softmax(S^T) packed the same way. So q, k,
//      v and P go from accumulator to operand without touching LDS, and a
//      softmax row (one query) is 16 registers on each of 4 lanes: two
//      shuffles per reduction.
//   3. O^T (lane = token, 4 consecutive channels) is stored to LDS buffer
//      B; after a barrier wave w computes proj columns 32w .. 32w+31 for
//      all 64 tokens as  proj^T = Wp . O^T  and stores them to buffer A.
//   4. After a barrier every token row leaves as one full 256-byte row at
//      its un-rolled position, written by the 16 lanes that loaded it.

#include <hip/hip_runtime.h>

namespace audiomuse {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AF_C = 128;               // channels
constexpr int AF_T = 64;                // tokens per window
constexpr int AF_TILE = AF_T * AF_C;    // bf16 elements of one LDS tile

// Element offset of 16-byte chunk ch (0..15) of token row `row`. An operand
// read takes rows r0 .. r0+15 at chunks c0 .. c0+3: all 16 chunk slots of
// the 256-byte bank row are hit once per ds_read_b128 lane group.
__device__ __forceinline__ int af_off(int row, int ch) {
  return row * AF_C + ((ch ^ (row & 15)) << 3);
}

// Offset of channel c (a multiple of 4) of token row `row`.
__device__ __forceinline__ int af_off_c4(int row, int c) {
  return af_off(row, c >> 3) + (c & 7);
}

// Two accumulator tiles, rounded to bf16, as one operand fragment.
__device__ __forceinline__ bf16x8 af_pack(const f32x4 lo, const f32x4 hi) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = (__bf16)lo[j];
    r[4 + j] = (__bf16)hi[j];
  }
  return r;
}

__device__ __forceinline__ f32x4 af_mfma(const bf16x8 a, const bf16x8 b,
                                         const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

}  // namespace

__global__ __launch_bounds__(256, 2) void attn_fused_c128_kernel(
    const __bf16* __restrict__ x,        // (B, H, W, 128)
    const __bf16* __restrict__ ln_w,     // (128)
    const __bf16* __restrict__ ln_b,     // (128)
    const __bf16* __restrict__ qkv_w,    // (384, 128)
    const __bf16* __restrict__ qkv_b,    // (384)
    const __bf16* __restrict__ proj_w,   // (128, 128)
    const __bf16* __restrict__ proj_b,   // (128)
    const __bf16* __restrict__ bias,     // (4, 64, 64) relative-position bias
    __bf16* __restrict__ out,            // (B, H, W, 128)
    int H, int W, int shift, float scale, float eps) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * AF_TILE];
  __bf16* bufA = lds;            // LN tile, later the proj tile
  __bf16* bufB = lds + AF_TILE;  // O tile

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;     // head in step 2, column group in step 3
  const int l16 = lane & 15;
  const int g = lane >> 4;

  const int nWw = W >> 3;
  const int nWh = H >> 3;
  const int win = blockIdx.x;
  const int b = win / (nWh * nWw);
  const int wrem = win - b * (nWh * nWw);
  const int wh = wrem / nWw;
  const int ww = wrem - wh * nWw;

  // token t (0..63) -> source coords + wrap bits (shifted windows)
  auto src_of = [&](int t, int& si, int& sj, int& wrap) {
    const int ri = t >> 3, ci = t & 7;
    int gi = wh * 8 + ri + shift;
    int gj = ww * 8 + ci + shift;
    const int wr = gi >= H;
    const int wc = gj >= W;
    si = wr ? gi - H : gi;
    sj = wc ? gj - W : gj;
    wrap = (wr << 1) | wc;
  };

  // wrap bits of all 64 tokens as a pair of 64-bit masks (lane = token)
  unsigned long long wrap_r_mask, wrap_c_mask;
  {
    int si, sj, wrap;
    src_of(lane, si, sj, wrap);
    wrap_r_mask = __ballot(wrap & 2);
    wrap_c_mask = __ballot(wrap & 1);
  }

  // ---- 1. gather + LayerNorm: 16 lanes per row, 4 rows per thread ----
  const int ch = tid & 15;       // this thread's 16-byte chunk of a row
  long long row_off[4];          // global element offset of (row, chunk)
  {
    bf16x8 xv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int si, sj, wrap;
      src_of(16 * i + (tid >> 4), si, sj, wrap);
      row_off[i] = (((long long)b * H + si) * W + sj) * AF_C + ch * 8;
      xv[i] = *(const bf16x8*)(x + row_off[i]);
    }
    const bf16x8 lw = *(const bf16x8*)(ln_w + ch * 8);
    const bf16x8 lb = *(const bf16x8*)(ln_b + ch * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sum = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += (float)xv[i][j];
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) sum += __shfl_xor(sum, d, 64);
      const float mean = sum / AF_C;
      float var = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dv = (float)xv[i][j] - mean;
        var += dv * dv;
      }
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) var += __shfl_xor(var, d, 64);
      const float rstd = rsqrtf(var / AF_C + eps);
      bf16x8 y;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        y[j] = (__bf16)((((float)xv[i][j] - mean) * rstd) * (float)lw[j] +
                        (float)lb[j]);
      *(bf16x8*)(bufA + af_off(16 * i + (tid >> 4), ch)) = y;
    }
  }
  __syncthreads();

  // ---- 2. head `wave`: QKV, attention ----
  const int h = wave;
  bf16x8 xn[4][4];   // [token tile][k-step] fragments of the LN tile
#pragma unroll
  for (int tr = 0; tr < 4; ++tr)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      xn[tr][ks] = *(const bf16x8*)(bufA + af_off(16 * tr + l16, 4 * ks + g));

  // Q^T and K^T: accumulator row = d (4g + reg of d tile dt), col = token
  bf16x8 qk[2][4];   // [q|k][token tile], k index = permuted d
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    f32x4 acc[2][4];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int feat = which * AF_C + h * 32 + dt * 16;
      const __bf16* wrow = qkv_w + (feat + l16) * AF_C + 8 * g;
      bf16x8 wf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) wf[ks] = *(const bf16x8*)(wrow + 32 * ks);
      const bf16x4 bb = *(const bf16x4*)(qkv_b + feat + 4 * g);
#pragma unroll
      for (int tr = 0; tr < 4; ++tr) {
        f32x4 a = {(float)bb[0], (float)bb[1], (float)bb[2], (float)bb[3]};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a = af_mfma(wf[ks], xn[tr][ks], a);
        acc[dt][tr] = a;
      }
    }
#pragma unroll
    for (int tr = 0; tr < 4; ++tr)
      qk[which][tr] = af_pack(acc[0][tr], acc[1][tr]);
  }

  // V: accumulator row = token (4g + reg of token tile tr), col = d
  bf16x8 vf[2][2];   // [d tile][key k-step], k index = permuted key token
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int feat = 2 * AF_C + h * 32 + dt * 16;
    const __bf16* wrow = qkv_w + (feat + l16) * AF_C + 8 * g;
    bf16x8 wf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) wf[ks] = *(const bf16x8*)(wrow + 32 * ks);
    const float bv = (float)qkv_b[feat + l16];
    f32x4 acc[4];
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {
      f32x4 a = {bv, bv, bv, bv};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a = af_mfma(xn[tr][ks], wf[ks], a);
      acc[tr] = a;
    }
    vf[dt][0] = af_pack(acc[0], acc[1]);
    vf[dt][1] = af_pack(acc[2], acc[3]);
  }

  // proj weights for step 3, in flight across the attention
  bf16x8 wp[2][4];   // [column tile][k-step]
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      wp[ct][ks] = *(const bf16x8*)(proj_w +
                                    (32 * wave + 16 * ct + l16) * AF_C +
                                    32 * ks + 8 * g);

  // S^T = K . Q^T: accumulator row = key (4g + reg of tile tc), col = query
  f32x4 st[4][4];    // [key tile][query tile]
#pragma unroll
  for (int tc = 0; tc < 4; ++tc)
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      st[tc][tr] = af_mfma(qk[1][tc], qk[0][tr], z);
    }

  // scale + relative-position bias + shift mask + softmax over the keys of
  // each query: 16 registers on this lane, the rest on lanes ^16, ^32
  bf16x8 pf[4][2];   // [query tile][key k-step]
#pragma unroll
  for (int tr = 0; tr < 4; ++tr) {
    const int tq = 16 * tr + l16;
    const int qwrap = (int)((((wrap_r_mask >> tq) & 1ull) << 1) |
                            ((wrap_c_mask >> tq) & 1ull));
    const __bf16* brow = bias + (h * 64 + tq) * 64 + 4 * g;
    float m = -1e30f;
#pragma unroll
    for (int tc = 0; tc < 4; ++tc) {
      const bf16x4 bb = *(const bf16x4*)(brow + 16 * tc);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int tk = 16 * tc + 4 * g + reg;
        const int kwrap = (int)((((wrap_r_mask >> tk) & 1ull) << 1) |
                                ((wrap_c_mask >> tk) & 1ull));
        float v = st[tc][tr][reg] * scale + (float)bb[reg];
        if (shift && qwrap != kwrap) v = -1e30f;
        st[tc][tr][reg] = v;
        m = fmaxf(m, v);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.0f;
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float e = __expf(st[tc][tr][reg] - m);
        st[tc][tr][reg] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = __frcp_rn(sum + 1e-20f);
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) st[tc][tr][reg] *= inv;
    pf[tr][0] = af_pack(st[0][tr], st[1][tr]);
    pf[tr][1] = af_pack(st[2][tr], st[3][tr]);
  }

  // O^T = V^T . P^T: accumulator row = d (4g + reg of tile dt), col = query
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      o = af_mfma(vf[dt][0], pf[tr][0], o);
      o = af_mfma(vf[dt][1], pf[tr][1], o);
      bf16x4 ob;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) ob[reg] = (__bf16)o[reg];
      *(bf16x4*)(bufB + af_off_c4(16 * tr + l16, 32 * h + 16 * dt + 4 * g)) =
          ob;
    }
  __syncthreads();   // O complete; every wave is done with the LN tile

  // ---- 3. proj^T = Wp . O^T, columns 32 wave .. 32 wave + 31 ----
  bf16x4 pb[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
    pb[ct] = *(const bf16x4*)(proj_b + 32 * wave + 16 * ct + 4 * g);
#pragma unroll
  for (int tr = 0; tr < 4; ++tr) {
    bf16x8 of[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      of[ks] = *(const bf16x8*)(bufB + af_off(16 * tr + l16, 4 * ks + g));
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      f32x4 a = {(float)pb[ct][0], (float)pb[ct][1], (float)pb[ct][2],
                 (float)pb[ct][3]};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a = af_mfma(wp[ct][ks], of[ks], a);
      bf16x4 ob;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) ob[reg] = (__bf16)a[reg];
      *(bf16x4*)(bufA +
                 af_off_c4(16 * tr + l16, 32 * wave + 16 * ct + 4 * g)) = ob;
    }
  }
  __syncthreads();

  // ---- 4. full 256-byte rows out, at the positions they were read from ----
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *(bf16x8*)(out + row_off[i]) =
        *(const bf16x8*)(bufA + af_off(16 * i + (tid >> 4), ch));
}

// H and W must be multiples of 8 and shift 0 or 4 (checked by the binding).
void launch_attn_fused_c128(const void* x, const void* ln_w, const void* ln_b,
                            const void* qkv_w, const void* qkv_b,
                            const void* proj_w, const void* proj_b,
                            const void* bias, void* out, int Bn, int H, int W,
                            int shift, float scale, float eps,
                            hipStream_t stream) {
  const unsigned n_windows = (unsigned)Bn * (H >> 3) * (W >> 3);
  hipLaunchKernelGGL(attn_fused_c128_kernel, dim3(n_windows), dim3(256), 0,
                     stream, (const __bf16*)x, (const __bf16*)ln_w,
                     (const __bf16*)ln_b, (const __bf16*)qkv_w,
                     (const __bf16*)qkv_b, (const __bf16*)proj_w,
                     (const __bf16*)proj_b, (const __bf16*)bias,
                     (__bf16*)out, H, W, shift, scale, eps);
}

}  // namespace audiomuse
