// hipBLASLt GEMMs with fused epilogues (bf16 in/out, fp32 compute).
//
// linear_gelu:     y = gelu(x @ w^T + b)        (epilogue GELU_BIAS)
// linear_bias_add: y = x @ w^T + b + residual   (epilogue BIAS, beta=1)
//
// The encoder MLP is Linear(C,4C) -> GELU -> Linear(4C,C) + residual; an
// eager GELU re-reads and re-writes the 4C-wide activation (measured ~9%
// of step time, profiles/r01_kernel_pmc.md) and the trailing residual
// add re-reads both the GEMM output and the skip tensor. Both ride the
// GEMM epilogue instead. Plain library GEMM use. At C = 128 (stage 1) the
// whole MLP half runs in the hand-written MFMA kernel of mlp_fused.hip
// instead, which keeps the hidden activation on chip; these two GEMMs
// serve the wider stages, where the three-op path is already near the
// fused kernel's compute time, and token counts that are not a multiple
// of its tile.

#include <hipblaslt/hipblaslt.h>
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <mutex>
#include <unordered_map>

namespace {

#define HIPBLASLT_CHECK(expr)                                          \
  do {                                                                 \
    hipblasStatus_t st_ = (expr);                                      \
    TORCH_CHECK(st_ == HIPBLAS_STATUS_SUCCESS, "hipblaslt error ", st_, \
                " at " #expr);                                         \
  } while (0)

hipblasLtHandle_t get_handle() {
  static hipblasLtHandle_t handle = [] {
    hipblasLtHandle_t h;
    TORCH_CHECK(hipblasLtCreate(&h) == HIPBLAS_STATUS_SUCCESS,
                "hipblasLtCreate failed");
    return h;
  }();
  return handle;
}

struct AlgoKey {
  int64_t m, n, k;
  int epi;
  bool operator==(const AlgoKey& o) const {
    return m == o.m && n == o.n && k == o.k && epi == o.epi;
  }
};
struct AlgoKeyHash {
  size_t operator()(const AlgoKey& k) const {
    return std::hash<int64_t>()(k.m * 1315423911 ^ k.n * 2654435761 ^ k.k ^
                                (int64_t)k.epi << 40);
  }
};

// every operand pointer handed to hipBLASLt must live on x's device
bool on_device_of(const torch::Tensor& x, const torch::Tensor& t) {
  return t.is_cuda() && t.get_device() == x.get_device();
}

std::mutex algo_mu;
std::unordered_map<AlgoKey, hipblasLtMatmulAlgo_t, AlgoKeyHash> algo_cache;

// Shared driver: D(M,N) = epilogue(x(M,K) @ w(N,K)^T + bias) + beta*C.
// Col-major framing: D(N,M)cm = op(A=w_rm seen cm (K,N), T) x op(B=x_cm
// (K,M), N); C shares D's layout, so a row-major (M,N) residual is legal.
torch::Tensor lt_linear(torch::Tensor x, torch::Tensor w, torch::Tensor bias,
                        hipblasLtEpilogue_t epi, const torch::Tensor* resid) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  x.is_contiguous(),
              "x must be contiguous bf16 GPU");
  TORCH_CHECK(on_device_of(x, w) && on_device_of(x, bias) &&
                  w.is_contiguous() && bias.is_contiguous() &&
                  w.scalar_type() == at::kBFloat16 &&
                  bias.scalar_type() == at::kBFloat16,
              "w/bias must be contiguous bf16 on x's device");
  TORCH_CHECK(x.numel() > 0 && w.dim() == 2, "x empty or w not (N, K)");
  const int64_t K = x.size(-1);
  const int64_t M = x.numel() / K;
  const int64_t N = w.size(0);
  TORCH_CHECK(w.size(1) == K && bias.numel() == N, "shape mismatch");
  if (resid != nullptr) {
    TORCH_CHECK(on_device_of(x, *resid) && resid->is_contiguous() &&
                    resid->scalar_type() == at::kBFloat16 &&
                    resid->numel() == M * N,
                "residual must be contiguous bf16 of (M, N)");
  }

  auto sizes = x.sizes().vec();
  sizes.back() = N;
  auto y = torch::empty(sizes, x.options());

  hipblasLtMatmulDesc_t desc;
  HIPBLASLT_CHECK(hipblasLtMatmulDescCreate(&desc, HIPBLAS_COMPUTE_32F,
                                            HIP_R_32F));
  hipblasOperation_t opA = HIPBLAS_OP_T, opB = HIPBLAS_OP_N;
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opA, sizeof(opA)));
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opB, sizeof(opB)));
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)));
  const void* bias_ptr = bias.data_ptr();
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias_ptr, sizeof(bias_ptr)));

  hipblasLtMatrixLayout_t la, lb, ld;
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(&la, HIP_R_16BF, K, N, K));
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(&lb, HIP_R_16BF, K, M, K));
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(&ld, HIP_R_16BF, N, M, N));

  auto stream = c10::hip::getCurrentHIPStream();
  static void* workspace = nullptr;
  static size_t workspace_size = 64ull << 20;
  static std::once_flag ws_once;
  std::call_once(ws_once, [] {
    TORCH_CHECK(hipMalloc(&workspace, workspace_size) == hipSuccess,
                "workspace alloc failed");
  });

  hipblasLtMatmulAlgo_t algo;
  bool have_algo = false;
  {
    std::lock_guard<std::mutex> g(algo_mu);
    auto it = algo_cache.find({M, N, K, (int)epi});
    if (it != algo_cache.end()) {
      algo = it->second;
      have_algo = true;
    }
  }
  if (!have_algo) {
    // timed search over the heuristic candidates (first call per shape):
    // the first heuristic is often 15-25% off the best for the skinny
    // K=128 / N=C shapes this encoder runs (profiles/r01_final_profile.md)
    hipblasLtMatmulPreference_t pref;
    HIPBLASLT_CHECK(hipblasLtMatmulPreferenceCreate(&pref));
    HIPBLASLT_CHECK(hipblasLtMatmulPreferenceSetAttribute(
        pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &workspace_size,
        sizeof(workspace_size)));
    hipblasLtMatmulHeuristicResult_t results[8];
    int found = 0;
    HIPBLASLT_CHECK(hipblasLtMatmulAlgoGetHeuristic(
        get_handle(), desc, la, lb, ld, ld, pref, 8, results, &found));
    hipblasLtMatmulPreferenceDestroy(pref);
    TORCH_CHECK(found > 0, "no hipblaslt algo for epilogue ", (int)epi,
                " at ", M, "x", N, "x", K);
    const float alpha_s = 1.0f, beta_s = 0.0f;
    auto stream0 = c10::hip::getCurrentHIPStream().stream();
    hipEvent_t ev0, ev1;
    (void)hipEventCreate(&ev0);
    (void)hipEventCreate(&ev1);
    int best = 0;
    float best_ms = 1e30f;
    for (int i = 0; i < found; ++i) {
      // warm once, then time 2 reps into y (its contents are overwritten
      // by the real call below)
      if (hipblasLtMatmul(get_handle(), desc, &alpha_s, w.data_ptr(), la,
                          x.data_ptr(), lb, &beta_s, y.data_ptr(), ld,
                          y.data_ptr(), ld, &results[i].algo, workspace,
                          workspace_size, stream0) != HIPBLAS_STATUS_SUCCESS)
        continue;
      (void)hipEventRecord(ev0, stream0);
      for (int r = 0; r < 2; ++r)
        (void)hipblasLtMatmul(get_handle(), desc, &alpha_s, w.data_ptr(), la,
                              x.data_ptr(), lb, &beta_s, y.data_ptr(), ld,
                              y.data_ptr(), ld, &results[i].algo, workspace,
                              workspace_size, stream0);
      (void)hipEventRecord(ev1, stream0);
      (void)hipEventSynchronize(ev1);
      float ms = 1e30f;
      (void)hipEventElapsedTime(&ms, ev0, ev1);
      if (ms < best_ms) {
        best_ms = ms;
        best = i;
      }
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    algo = results[best].algo;
    std::lock_guard<std::mutex> g(algo_mu);
    algo_cache[{M, N, K, (int)epi}] = algo;
  }

  const float alpha = 1.0f;
  const float beta = resid != nullptr ? 1.0f : 0.0f;
  const void* c_ptr = resid != nullptr ? resid->data_ptr() : y.data_ptr();
  HIPBLASLT_CHECK(hipblasLtMatmul(
      get_handle(), desc, &alpha, w.data_ptr(), la, x.data_ptr(), lb, &beta,
      c_ptr, ld, y.data_ptr(), ld, &algo, workspace, workspace_size,
      stream.stream()));

  hipblasLtMatrixLayoutDestroy(la);
  hipblasLtMatrixLayoutDestroy(lb);
  hipblasLtMatrixLayoutDestroy(ld);
  hipblasLtMatmulDescDestroy(desc);
  return y;
}

torch::Tensor linear_gelu(torch::Tensor x, torch::Tensor w,
                          torch::Tensor bias) {
  return lt_linear(x, w, bias, HIPBLASLT_EPILOGUE_GELU_BIAS, nullptr);
}

torch::Tensor linear_bias_add(torch::Tensor x, torch::Tensor w,
                              torch::Tensor bias, torch::Tensor resid) {
  return lt_linear(x, w, bias, HIPBLASLT_EPILOGUE_BIAS, &resid);
}

torch::Tensor linear_bias(torch::Tensor x, torch::Tensor w,
                          torch::Tensor bias) {
  return lt_linear(x, w, bias, HIPBLASLT_EPILOGUE_BIAS, nullptr);
}

// fp8 (OCP e4m3) GEMM with per-tensor scales and the same timed algo
// search: D_bf16 = (sa * x_fp8) @ (sb * w_fp8)^T [+ bias]. torch's
// _scaled_mm takes hipBLASLt's first heuristic, which is 2.1x off at
// the encoder's K=128/N=384 shape (scripts/fp8_shapes.py) — this path
// searches instead.
torch::Tensor linear_fp8(torch::Tensor x, torch::Tensor w,
                         torch::Tensor sa, torch::Tensor sb,
                         c10::optional<torch::Tensor> bias,
                         bool gelu,
                         c10::optional<torch::Tensor> resid,
                         c10::optional<torch::Tensor> d_inv_scale,
                         c10::optional<torch::Tensor> amax_d) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat8_e4m3fn &&
                  x.is_contiguous(),
              "x must be contiguous fp8e4m3 GPU");
  TORCH_CHECK(on_device_of(x, w) && w.is_contiguous() &&
                  w.scalar_type() == at::kFloat8_e4m3fn,
              "w must be contiguous fp8e4m3 on x's device");
  TORCH_CHECK(on_device_of(x, sa) && on_device_of(x, sb) &&
                  sa.scalar_type() == at::kFloat &&
                  sb.scalar_type() == at::kFloat && sa.numel() >= 1 &&
                  sb.numel() >= 1,
              "scales must be f32 scalars on x's device");
  TORCH_CHECK(x.numel() > 0 && w.dim() == 2, "x empty or w not (N, K)");
  const int64_t K = x.size(-1);
  const int64_t M = x.numel() / K;
  const int64_t N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "shape mismatch");
  if (bias.has_value()) {
    TORCH_CHECK(on_device_of(x, *bias) && bias->is_contiguous() &&
                    bias->scalar_type() == at::kBFloat16 &&
                    bias->numel() == N,
                "bias must be contiguous bf16 of N elements on x's device");
  }
  const bool out8 = d_inv_scale.has_value();
  if (resid.has_value()) {
    TORCH_CHECK(!out8, "residual add requires bf16 output");
    TORCH_CHECK(on_device_of(x, *resid) && resid->is_contiguous() &&
                    resid->scalar_type() == at::kBFloat16 &&
                    resid->numel() == M * N,
                "residual must be contiguous bf16 of (M, N) on x's device");
  }

  auto sizes = x.sizes().vec();
  sizes.back() = N;
  auto y = torch::empty(sizes, x.options().dtype(
      out8 ? at::kFloat8_e4m3fn : at::kBFloat16));

  hipblasLtMatmulDesc_t desc;
  HIPBLASLT_CHECK(hipblasLtMatmulDescCreate(&desc, HIPBLAS_COMPUTE_32F,
                                            HIP_R_32F));
  hipblasOperation_t opA = HIPBLAS_OP_T, opB = HIPBLAS_OP_N;
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opA, sizeof(opA)));
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opB, sizeof(opB)));
  if (out8) {
    // D = d_inv_scale * acc, cast to e4m3; true amax recorded on device
    const void* ds = d_inv_scale->data_ptr();
    HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
        desc, HIPBLASLT_MATMUL_DESC_D_SCALE_POINTER, &ds, sizeof(ds)));
    if (amax_d.has_value()) {
      const void* ap = amax_d->data_ptr();
      HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
          desc, HIPBLASLT_MATMUL_DESC_AMAX_D_POINTER, &ap, sizeof(ap)));
    }
  }
  // col-major framing: A = w (K, N) cm via T, B = x (K, M) cm; scales
  // swap accordingly (A-scale applies to w)
  const void* a_scale = sb.data_ptr();
  const void* b_scale = sa.data_ptr();
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_A_SCALE_POINTER, &a_scale,
      sizeof(a_scale)));
  HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
      desc, HIPBLASLT_MATMUL_DESC_B_SCALE_POINTER, &b_scale,
      sizeof(b_scale)));
  if (bias.has_value()) {
    hipblasLtEpilogue_t epi =
        gelu ? HIPBLASLT_EPILOGUE_GELU_BIAS : HIPBLASLT_EPILOGUE_BIAS;
    HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
        desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)));
    const void* bp = bias->data_ptr();
    HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
        desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bp, sizeof(bp)));
  } else if (gelu) {
    hipblasLtEpilogue_t epi = HIPBLASLT_EPILOGUE_GELU;
    HIPBLASLT_CHECK(hipblasLtMatmulDescSetAttribute(
        desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)));
  }

  hipblasLtMatrixLayout_t la, lb, ld;
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(&la, HIP_R_8F_E4M3, K, N, K));
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(&lb, HIP_R_8F_E4M3, K, M, K));
  HIPBLASLT_CHECK(hipblasLtMatrixLayoutCreate(
      &ld, out8 ? HIP_R_8F_E4M3 : HIP_R_16BF, N, M, N));

  auto stream = c10::hip::getCurrentHIPStream();
  static void* workspace = nullptr;
  static size_t workspace_size = 64ull << 20;
  static std::once_flag ws_once;
  std::call_once(ws_once, [] {
    TORCH_CHECK(hipMalloc(&workspace, workspace_size) == hipSuccess,
                "workspace alloc failed");
  });

  hipblasLtMatmulAlgo_t algo;
  bool have_algo = false;
  {
    std::lock_guard<std::mutex> g(algo_mu);
    auto it = algo_cache.find({M, N, K, 1000 + (bias.has_value() ? 1 : 0) + (gelu ? 2 : 0) + (out8 ? 4 : 0) + (resid.has_value() ? 8 : 0)});
    if (it != algo_cache.end()) {
      algo = it->second;
      have_algo = true;
    }
  }
  if (!have_algo) {
    hipblasLtMatmulPreference_t pref;
    HIPBLASLT_CHECK(hipblasLtMatmulPreferenceCreate(&pref));
    HIPBLASLT_CHECK(hipblasLtMatmulPreferenceSetAttribute(
        pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &workspace_size,
        sizeof(workspace_size)));
    hipblasLtMatmulHeuristicResult_t results[8];
    int found = 0;
    HIPBLASLT_CHECK(hipblasLtMatmulAlgoGetHeuristic(
        get_handle(), desc, la, lb, ld, ld, pref, 8, results, &found));
    hipblasLtMatmulPreferenceDestroy(pref);
    TORCH_CHECK(found > 0, "no hipblaslt fp8 algo at ", M, "x", N, "x", K);
    const float alpha_s = 1.0f;
    const float beta_s = resid.has_value() ? 1.0f : 0.0f;
    const void* c_s = resid.has_value() ? resid->data_ptr() : y.data_ptr();
    auto stream0 = stream.stream();
    hipEvent_t ev0, ev1;
    (void)hipEventCreate(&ev0);
    (void)hipEventCreate(&ev1);
    int best = 0;
    float best_ms = 1e30f;
    for (int i = 0; i < found; ++i) {
      if (hipblasLtMatmul(get_handle(), desc, &alpha_s, w.data_ptr(), la,
                          x.data_ptr(), lb, &beta_s, c_s, ld,
                          y.data_ptr(), ld, &results[i].algo, workspace,
                          workspace_size, stream0) != HIPBLAS_STATUS_SUCCESS)
        continue;
      (void)hipEventRecord(ev0, stream0);
      for (int r = 0; r < 2; ++r)
        (void)hipblasLtMatmul(get_handle(), desc, &alpha_s, w.data_ptr(), la,
                              x.data_ptr(), lb, &beta_s, c_s, ld,
                              y.data_ptr(), ld, &results[i].algo, workspace,
                              workspace_size, stream0);
      (void)hipEventRecord(ev1, stream0);
      (void)hipEventSynchronize(ev1);
      float ms = 1e30f;
      (void)hipEventElapsedTime(&ms, ev0, ev1);
      if (ms < best_ms) {
        best_ms = ms;
        best = i;
      }
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    algo = results[best].algo;
    std::lock_guard<std::mutex> g(algo_mu);
    algo_cache[{M, N, K, 1000 + (bias.has_value() ? 1 : 0) + (gelu ? 2 : 0) + (out8 ? 4 : 0) + (resid.has_value() ? 8 : 0)}] = algo;
  }

  const float alpha = 1.0f;
  const float beta = resid.has_value() ? 1.0f : 0.0f;
  const void* c_ptr = resid.has_value() ? resid->data_ptr() : y.data_ptr();
  HIPBLASLT_CHECK(hipblasLtMatmul(
      get_handle(), desc, &alpha, w.data_ptr(), la, x.data_ptr(), lb, &beta,
      c_ptr, ld, y.data_ptr(), ld, &algo, workspace, workspace_size,
      stream.stream()));

  hipblasLtMatrixLayoutDestroy(la);
  hipblasLtMatrixLayoutDestroy(lb);
  hipblasLtMatrixLayoutDestroy(ld);
  hipblasLtMatmulDescDestroy(desc);
  return y;
}

}  // namespace

void register_gemm_gelu(pybind11::module_& m) {
  m.def("linear_gelu", &linear_gelu,
        "gelu(x @ w.T + bias) via hipBLASLt epilogue fusion");
  m.def("linear_bias_add", &linear_bias_add,
        "x @ w.T + bias + residual via hipBLASLt beta=1");
  m.def("linear_bias", &linear_bias,
        "x @ w.T + bias via hipBLASLt with timed algo search");
  m.def("linear_fp8", &linear_fp8,
        "fp8 e4m3 GEMM with per-tensor scales + timed algo search",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("sa"),
        pybind11::arg("sb"), pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("gelu") = false,
        pybind11::arg("resid") = pybind11::none(),
        pybind11::arg("d_inv_scale") = pybind11::none(),
        pybind11::arg("amax_d") = pybind11::none());
}
