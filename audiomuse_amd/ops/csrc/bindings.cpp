// PyTorch bindings for the AudioMuse-AMD native kernel library (gfx950).
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <vector>

#include <c10/hip/HIPStream.h>

namespace audiomuse {
void launch_mel_fwd(const float* audio, float* out, const float* window,
                    const float2* twiddle, const int* mel_rowptr,
                    const int* mel_bin, const float* mel_w,
                    const int* band_first, const int* band_len,
                    const int* band_off, const float* band_w, int kmax,
                    int allow_v2, int B, int T, int n_frames, int hop,
                    int n_mels, int n_fft, int center, int log_mode,
                    int quant16, hipStream_t stream);
bool mel_fwd_takes_v2(int n_fft, int hop, int n_mels, int center, int kmax,
                      int allow_v2, bool have_band);
void launch_patch_embed_bf16(const void* mel, const void* weight,
                             const void* bias, void* out, int Bn, int n_mels,
                             int T, int n_frames, int C, hipStream_t stream);
void launch_ivf_scan(int dtype_code, int metric, const void* query,
                     const float* qnorm, const void* data,
                     const float* row_norm, const int* probe,
                     const int* cell_off, const long long* cand_off,
                     float* out_dist, int* out_row, int Q, int d, int nprobe,
                     long long cap, hipStream_t stream);
void launch_ivf_scan_sel(int dtype_code, int metric, const void* query,
                         const float* qnorm, const void* data,
                         const float* row_norm, const int* probe,
                         const int* sel_rows, const int* sel_off,
                         const long long* cand_off, float* out_dist,
                         int* out_row, int Q, int d, int nprobe, long long cap,
                         hipStream_t stream);
void launch_ivf_scan_topk(int dtype_code, int metric, const void* query,
                          const float* qnorm, const void* data,
                          const float* row_norm, const int* probe,
                          const int* off, const int* sel_rows,
                          const int* skip_row, float* out_dist, int* out_row,
                          int Q, int S, int K, int d, int nprobe,
                          hipStream_t stream);
void launch_ivf_scan_topk_excl(int dtype_code, int metric, const void* query,
                               const float* qnorm, const void* data,
                               const float* row_norm, const int* probe,
                               const int* cell_off, const int* skip_row,
                               const int* row_label, const int* q_label,
                               float* out_dist, int* out_row, int Q, int S,
                               int K, int d, int nprobe, hipStream_t stream);
void launch_graph_label_pull(const int* label_in, int* label_out,
                             const int* idx, const int* in_off,
                             const int* in_edge, int* changed, int n, int k,
                             int n_in, hipStream_t stream);
void launch_umap_epoch(const float* E, float* out, const int* idx,
                       const int* thr, const int* in_off, const int* in_edge,
                       const int* in_thr, int n, int k, int n_in, int neg,
                       float alpha, float a, float b, unsigned int seed,
                       unsigned int epoch, hipStream_t stream);
void launch_path_relax(const float* dist_in, const int* pred_in,
                       float* dist_out, int* pred_out, const int* idx,
                       const float* w, const int* in_off, const int* in_edge,
                       const unsigned char* allowed, int* changed, int B,
                       int n, int k, int n_in, int legs_inner,
                       hipStream_t stream);
void launch_path_walk(const float* dist, const int* pred, const int* src,
                      const int* dst, int* out, int* count, int B, int n,
                      int T1, int legs_inner, hipStream_t stream);
void launch_rank_pull(const float* x_in, float* p_out, float* q_out,
                      const float* restart, const float* inv_deg,
                      const int* idx, const float* s, const int* in_off,
                      const int* in_edge, const unsigned char* allowed,
                      float alpha, int B, int n, int k, int n_in,
                      int legs_inner, hipStream_t stream);
void launch_community_move(const int* label_in, int* label_out,
                           const long long* tot, const long long* deg,
                           const int* idx, const int* w, const int* in_off,
                           const int* in_edge, long long A, long long g,
                           int up, int n, int k, int n_in,
                           hipStream_t stream);
void launch_layernorm_bf16(const void* x, void* y, const void* w,
                           const void* b, long long n_rows, int dim, float eps,
                           hipStream_t stream);
void launch_add_layernorm_bf16(const void* x, const void* in2, void* sum_out,
                               void* y, const void* w, const void* b,
                               long long n_rows, int dim, float eps,
                               hipStream_t stream);
void launch_layernorm_bf16_fp8_impl(const void* x, void* y8, const void* w,
                                    const void* b, const void* in2,
                                    void* sum_out, const float* q_scale,
                                    float* q_amax, long long n_rows, int dim,
                                    float eps, hipStream_t stream);
void launch_mfma_probe(const void* A, const void* B, float* D,
                       hipStream_t stream);
void launch_window_attn4(const void* qkv, void* out, const void* bias,
                         int Bn, int H, int W, int C, int heads, int shift,
                         float scale, hipStream_t stream);
void launch_window_attn(const void* qkv, void* out, const void* bias, int Bn,
                        int H, int W, int C, int heads, int shift, float scale,
                        bool xcd_grid, hipStream_t stream);
void launch_merge_layernorm_bf16(const void* x, void* y, const void* w,
                                 const void* b, int Bn, int H, int W, int C,
                                 float eps, hipStream_t stream);
void launch_mlp_fused_c128(const void* x, const void* proj, const void* ln_w,
                           const void* ln_b, const void* W1, const void* b1,
                           const void* W2, const void* b2, void* out,
                           long long M, float eps, hipStream_t stream);
void launch_mlp_fused_c256(const void* x, const void* proj, const void* ln_w,
                           const void* ln_b, const void* W1, const void* b1,
                           const void* W2, const void* b2, void* out,
                           long long M, float eps, hipStream_t stream);
void launch_attn_fused_c128(const void* x, const void* ln_w, const void* ln_b,
                            const void* qkv_w, const void* qkv_b,
                            const void* proj_w, const void* proj_b,
                            const void* bias, void* out, int Bn, int H, int W,
                            int shift, float scale, float eps,
                            hipStream_t stream);
void launch_window_attn_fp8(const void* qkv, void* out, const void* bias,
                            const void* qs_ptr, int Bn, int H, int W, int C,
                            int heads, int shift, float sm_scale,
                            hipStream_t stream);
void launch_fp_align(const int* words, const long long* off, const int* pairs,
                     int* out, long long W, int F, long long P, int max_offset,
                     int min_words, int lds_words, hipStream_t stream);
}

#define AM_CHECK(x, msg) TORCH_CHECK(x, msg)
#define AM_CHECK_GPU_F32_CONTIG(t)                                   \
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&        \
                  t.is_contiguous(),                                 \
              #t " must be a contiguous float32 GPU tensor")

static torch::Tensor mel_fwd(torch::Tensor audio, torch::Tensor window,
                             torch::Tensor twiddle, torch::Tensor mel_rowptr,
                             torch::Tensor mel_bin, torch::Tensor mel_w,
                             int64_t hop, int64_t n_fft, bool center,
                             int64_t log_mode, bool quant16,
                             c10::optional<torch::Tensor> band_first,
                             c10::optional<torch::Tensor> band_len,
                             c10::optional<torch::Tensor> band_off,
                             c10::optional<torch::Tensor> band_w,
                             int64_t kmax, bool allow_v2,
                             c10::optional<torch::Tensor> out_opt) {
  AM_CHECK_GPU_F32_CONTIG(audio);
  AM_CHECK_GPU_F32_CONTIG(window);
  AM_CHECK_GPU_F32_CONTIG(mel_w);
  AM_CHECK(audio.dim() == 2, "audio must be (B, T)");
  AM_CHECK(twiddle.is_cuda() && twiddle.is_contiguous() &&
               twiddle.scalar_type() == at::kFloat &&
               twiddle.numel() == n_fft,  // (n_fft/2, 2) floats
           "twiddle must be (n_fft/2, 2) float32 on GPU");
  AM_CHECK(mel_rowptr.is_cuda() && mel_rowptr.scalar_type() == at::kInt &&
               mel_bin.scalar_type() == at::kInt,
           "CSR index tensors must be int32 on GPU");
  AM_CHECK(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 ||
               n_fft == 4096,
           "n_fft must be a power of two in [256, 4096]");

  const int64_t B = audio.size(0);
  const int64_t T = audio.size(1);
  const int64_t n_mels = mel_rowptr.numel() - 1;
  const int64_t n_frames =
      center ? (1 + T / hop) : (1 + (T - n_fft) / hop);
  AM_CHECK(n_frames >= 1, "audio too short for one frame");
  AM_CHECK(window.numel() == n_fft, "window must have n_fft elements");
  AM_CHECK(hop >= 1 && T >= 1 && B >= 1 && B <= 65535,
           "mel_fwd needs hop >= 1, T >= 1 and 1 <= B <= 65535");

  // Band plan of the multi-frame kernel: all four tensors or none.
  const bool have_band = band_first.has_value() && band_len.has_value() &&
                         band_off.has_value() && band_w.has_value();
  if (have_band) {
    auto ok_i32 = [&](const torch::Tensor& t) {
      return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() &&
             t.numel() == n_mels && t.get_device() == audio.get_device();
    };
    AM_CHECK(ok_i32(*band_first) && ok_i32(*band_len) && ok_i32(*band_off),
             "band_first, band_len, band_off must be (n_mels,) int32 on the "
             "audio's device");
    AM_CHECK_GPU_F32_CONTIG((*band_w));
    AM_CHECK(band_w->get_device() == audio.get_device() && band_w->numel() >= 1,
             "band_w must be a non-empty tensor on the audio's device");
    AM_CHECK(kmax >= 0 && kmax <= n_fft / 2, "kmax must be a bin index");
  }

  torch::Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    AM_CHECK_GPU_F32_CONTIG(out);
    AM_CHECK(out.dim() == 3 && out.size(0) == B && out.size(1) == n_mels &&
                 out.size(2) == n_frames &&
                 out.get_device() == audio.get_device(),
             "out must be (B, n_mels, n_frames) float32 on the audio's device");
  } else {
    out = torch::empty({B, n_mels, n_frames}, audio.options());
  }
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_mel_fwd(
      audio.data_ptr<float>(), out.data_ptr<float>(), window.data_ptr<float>(),
      reinterpret_cast<const float2*>(twiddle.data_ptr<float>()),
      mel_rowptr.data_ptr<int>(), mel_bin.data_ptr<int>(),
      mel_w.data_ptr<float>(),
      have_band ? band_first->data_ptr<int>() : nullptr,
      have_band ? band_len->data_ptr<int>() : nullptr,
      have_band ? band_off->data_ptr<int>() : nullptr,
      have_band ? band_w->data_ptr<float>() : nullptr, (int)kmax,
      allow_v2 ? 1 : 0, (int)B, (int)T, (int)n_frames, (int)hop, (int)n_mels,
      (int)n_fft, center ? 1 : 0, (int)log_mode, quant16 ? 1 : 0,
      stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

static void ivf_scan(int64_t dtype_code, int64_t metric, torch::Tensor query,
                     torch::Tensor qnorm, torch::Tensor data,
                     torch::Tensor row_norm, torch::Tensor probe,
                     torch::Tensor cell_off, torch::Tensor cand_off,
                     torch::Tensor out_dist, torch::Tensor out_row,
                     int64_t dim_pad) {
  AM_CHECK(query.is_cuda() && data.is_cuda(), "ivf_scan needs GPU tensors");
  AM_CHECK(probe.scalar_type() == at::kInt && cell_off.scalar_type() == at::kInt,
           "probe/cell_off must be int32");
  AM_CHECK(cand_off.scalar_type() == at::kLong, "cand_off must be int64");
  AM_CHECK(out_dist.is_contiguous() && out_row.is_contiguous(),
           "outputs must be contiguous");
  const int Q = probe.size(0);
  const int nprobe = probe.size(1);
  const long long cap = out_dist.size(1);
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_ivf_scan(
      (int)dtype_code, (int)metric, query.data_ptr(), qnorm.data_ptr<float>(),
      data.data_ptr(), row_norm.data_ptr<float>(), probe.data_ptr<int>(),
      cell_off.data_ptr<int>(),
      reinterpret_cast<const long long*>(cand_off.data_ptr<int64_t>()),
      out_dist.data_ptr<float>(), out_row.data_ptr<int>(), Q, (int)dim_pad,
      nprobe, cap, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

static void ivf_scan_sel(int64_t dtype_code, int64_t metric,
                         torch::Tensor query, torch::Tensor qnorm,
                         torch::Tensor data, torch::Tensor row_norm,
                         torch::Tensor probe, torch::Tensor sel_rows,
                         torch::Tensor sel_off, torch::Tensor cand_off,
                         torch::Tensor out_dist, torch::Tensor out_row,
                         int64_t dim_pad) {
  AM_CHECK(query.is_cuda() && data.is_cuda(), "ivf_scan_sel needs GPU tensors");
  AM_CHECK(probe.scalar_type() == at::kInt, "probe must be int32");
  AM_CHECK(cand_off.scalar_type() == at::kLong, "cand_off must be int64");
  AM_CHECK(out_dist.is_contiguous() && out_row.is_contiguous(),
           "outputs must be contiguous");
  AM_CHECK(sel_rows.is_cuda() && sel_off.is_cuda() &&
               sel_rows.scalar_type() == at::kInt &&
               sel_off.scalar_type() == at::kInt &&
               sel_rows.is_contiguous() && sel_off.is_contiguous() &&
               sel_rows.dim() == 1 && sel_off.dim() == 1,
           "sel_rows/sel_off must be contiguous 1-D int32 GPU tensors");
  AM_CHECK(sel_off.numel() >= 2, "sel_off must hold ncells+1 offsets");
  const int Q = probe.size(0);
  const int nprobe = probe.size(1);
  const long long cap = out_dist.size(1);
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_ivf_scan_sel(
      (int)dtype_code, (int)metric, query.data_ptr(), qnorm.data_ptr<float>(),
      data.data_ptr(), row_norm.data_ptr<float>(), probe.data_ptr<int>(),
      sel_rows.data_ptr<int>(), sel_off.data_ptr<int>(),
      reinterpret_cast<const long long*>(cand_off.data_ptr<int64_t>()),
      out_dist.data_ptr<float>(), out_row.data_ptr<int>(), Q, (int)dim_pad,
      nprobe, cap, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// Fused scan + top-K: out_dist/out_row are (Q, S, K); S splits per query
// and K are taken from their shape. sel_rows/sel_off and skip_row are
// optional (None: unscoped walk over cell_off / nothing skipped).
// row_label (N,) / q_label (Q,) select the label-excluding kernel
// (ivf_scan_topk_excl below); they do not combine with sel_rows.
static void ivf_scan_topk_impl(int64_t dtype_code, int64_t metric,
                               torch::Tensor query, torch::Tensor qnorm,
                               torch::Tensor data, torch::Tensor row_norm,
                               torch::Tensor probe, torch::Tensor cell_off,
                               c10::optional<torch::Tensor> sel_rows,
                               c10::optional<torch::Tensor> sel_off,
                               c10::optional<torch::Tensor> skip_row,
                               c10::optional<torch::Tensor> row_label,
                               c10::optional<torch::Tensor> q_label,
                               torch::Tensor out_dist, torch::Tensor out_row,
                               int64_t dim_pad) {
  AM_CHECK(query.is_cuda() && data.is_cuda() && qnorm.is_cuda() &&
               row_norm.is_cuda() && probe.is_cuda() && cell_off.is_cuda() &&
               out_dist.is_cuda() && out_row.is_cuda(),
           "ivf_scan_topk needs GPU tensors");
  AM_CHECK(dtype_code >= 0 && dtype_code <= 2 && metric >= 0 && metric <= 2 &&
               (dtype_code != 2 || metric == 0),
           "unknown dtype/metric (i8 is angular only)");
  AM_CHECK(probe.scalar_type() == at::kInt && probe.dim() == 2 &&
               probe.is_contiguous() && cell_off.scalar_type() == at::kInt &&
               cell_off.dim() == 1 && cell_off.is_contiguous() &&
               cell_off.numel() >= 2,
           "probe (Q, nprobe) / cell_off (ncells+1,) must be contiguous int32");
  AM_CHECK(query.is_contiguous() && data.is_contiguous() &&
               qnorm.is_contiguous() && row_norm.is_contiguous() &&
               qnorm.scalar_type() == at::kFloat &&
               row_norm.scalar_type() == at::kFloat,
           "query/data/norms must be contiguous, norms float32");
  AM_CHECK(out_dist.scalar_type() == at::kFloat &&
               out_row.scalar_type() == at::kInt && out_dist.dim() == 3 &&
               out_dist.sizes() == out_row.sizes() &&
               out_dist.is_contiguous() && out_row.is_contiguous(),
           "outputs must be contiguous (Q, S, K) float32 / int32");
  const int64_t Q = probe.size(0);
  const int64_t nprobe = probe.size(1);
  const int64_t S = out_dist.size(1);
  const int64_t K = out_dist.size(2);
  AM_CHECK(out_dist.size(0) == Q && qnorm.numel() == Q && query.size(0) == Q,
           "query, qnorm, probe and outputs must agree on Q");
  AM_CHECK(K >= 1 && K <= 256, "K must be in [1, 256]");
  AM_CHECK(S >= 1 && S <= 65535 && Q <= 65535, "S and Q must be <= 65535");
  AM_CHECK(dim_pad >= 1 && (dtype_code != 2 || dim_pad % 4 == 0) &&
               dim_pad <= 8192,
           "dim_pad must be in [1, 8192] (a multiple of 4 for i8)");
  AM_CHECK(query.numel() == Q * (dtype_code == 2 ? dim_pad / 4 : dim_pad) &&
               data.numel() == row_norm.numel() *
                   (dtype_code == 2 ? dim_pad / 4 : dim_pad),
           "query/data do not match dim_pad");
  AM_CHECK(sel_rows.has_value() == sel_off.has_value(),
           "sel_rows and sel_off go together");
  const int* sel_rows_p = nullptr;
  const int* off_p = cell_off.data_ptr<int>();
  if (sel_rows.has_value()) {
    const torch::Tensor& sr = *sel_rows;
    const torch::Tensor& so = *sel_off;
    AM_CHECK(sr.is_cuda() && so.is_cuda() && sr.scalar_type() == at::kInt &&
                 so.scalar_type() == at::kInt && sr.is_contiguous() &&
                 so.is_contiguous() && sr.dim() == 1 && so.dim() == 1,
             "sel_rows/sel_off must be contiguous 1-D int32 GPU tensors");
    AM_CHECK(so.numel() == cell_off.numel(),
             "sel_off must hold ncells+1 offsets");
    sel_rows_p = sr.data_ptr<int>();
    off_p = so.data_ptr<int>();
  }
  const int* skip_p = nullptr;
  if (skip_row.has_value()) {
    const torch::Tensor& sk = *skip_row;
    AM_CHECK(sk.is_cuda() && sk.scalar_type() == at::kInt &&
                 sk.is_contiguous() && sk.numel() == Q,
             "skip_row must be a contiguous (Q,) int32 GPU tensor");
    skip_p = sk.data_ptr<int>();
  }
  AM_CHECK(row_label.has_value() == q_label.has_value(),
           "row_label and q_label go together");
  if (row_label.has_value()) {
    const torch::Tensor& rl = *row_label;
    const torch::Tensor& ql = *q_label;
    AM_CHECK(!sel_rows.has_value(),
             "label exclusion does not combine with a row selection");
    AM_CHECK(rl.is_cuda() && ql.is_cuda() && rl.scalar_type() == at::kInt &&
                 ql.scalar_type() == at::kInt && rl.is_contiguous() &&
                 ql.is_contiguous() && rl.dim() == 1 && ql.dim() == 1 &&
                 rl.get_device() == data.get_device() &&
                 ql.get_device() == data.get_device(),
             "row_label/q_label must be contiguous 1-D int32 tensors on the "
             "GPU of data");
    AM_CHECK(rl.numel() == row_norm.numel() && ql.numel() == Q,
             "row_label must hold one label per row, q_label one per query");
    if (Q == 0) return;
    auto stream = c10::hip::getCurrentHIPStream();
    audiomuse::launch_ivf_scan_topk_excl(
        (int)dtype_code, (int)metric, query.data_ptr(),
        qnorm.data_ptr<float>(), data.data_ptr(), row_norm.data_ptr<float>(),
        probe.data_ptr<int>(), off_p, skip_p, rl.data_ptr<int>(),
        ql.data_ptr<int>(), out_dist.data_ptr<float>(),
        out_row.data_ptr<int>(), (int)Q, (int)S, (int)K, (int)dim_pad,
        (int)nprobe, stream.stream());
    C10_HIP_CHECK(hipGetLastError());
    return;
  }
  if (Q == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_ivf_scan_topk(
      (int)dtype_code, (int)metric, query.data_ptr(), qnorm.data_ptr<float>(),
      data.data_ptr(), row_norm.data_ptr<float>(), probe.data_ptr<int>(),
      off_p, sel_rows_p, skip_p, out_dist.data_ptr<float>(),
      out_row.data_ptr<int>(), (int)Q, (int)S, (int)K, (int)dim_pad,
      (int)nprobe, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

static void ivf_scan_topk(int64_t dtype_code, int64_t metric,
                          torch::Tensor query, torch::Tensor qnorm,
                          torch::Tensor data, torch::Tensor row_norm,
                          torch::Tensor probe, torch::Tensor cell_off,
                          c10::optional<torch::Tensor> sel_rows,
                          c10::optional<torch::Tensor> sel_off,
                          c10::optional<torch::Tensor> skip_row,
                          torch::Tensor out_dist, torch::Tensor out_row,
                          int64_t dim_pad) {
  ivf_scan_topk_impl(dtype_code, metric, query, qnorm, data, row_norm, probe,
                     cell_off, sel_rows, sel_off, skip_row, c10::nullopt,
                     c10::nullopt, out_dist, out_row, dim_pad);
}

// ivf_scan_topk over all rows of the probed cells, except that query q
// never gets a row whose row_label equals q_label[q] (a negative q_label
// excludes nothing).
static void ivf_scan_topk_excl(int64_t dtype_code, int64_t metric,
                               torch::Tensor query, torch::Tensor qnorm,
                               torch::Tensor data, torch::Tensor row_norm,
                               torch::Tensor probe, torch::Tensor cell_off,
                               c10::optional<torch::Tensor> skip_row,
                               torch::Tensor row_label, torch::Tensor q_label,
                               torch::Tensor out_dist, torch::Tensor out_row,
                               int64_t dim_pad) {
  ivf_scan_topk_impl(dtype_code, metric, query, qnorm, data, row_norm, probe,
                     cell_off, c10::nullopt, c10::nullopt, skip_row, row_label,
                     q_label, out_dist, out_row, dim_pad);
}

// One epoch of the map layout: reads E, writes out (both (n, 2) f32; they
// must not overlap). idx/thr are (n, k); in_off (n+1), in_edge and in_thr
// (n_in) are the reverse lists and the thresholds in list order.
static void umap_epoch(torch::Tensor E, torch::Tensor out, torch::Tensor idx,
                       torch::Tensor thr, torch::Tensor in_off,
                       torch::Tensor in_edge, torch::Tensor in_thr,
                       double alpha, double a, double b, int64_t seed,
                       int64_t epoch, int64_t neg) {
  AM_CHECK(E.is_cuda() && out.is_cuda() && idx.is_cuda() && thr.is_cuda() &&
               in_off.is_cuda() && in_edge.is_cuda() && in_thr.is_cuda(),
           "umap_epoch needs GPU tensors");
  AM_CHECK(E.scalar_type() == at::kFloat && out.scalar_type() == at::kFloat &&
               E.dim() == 2 && E.size(1) == 2 && out.sizes() == E.sizes() &&
               E.is_contiguous() && out.is_contiguous(),
           "E/out must be contiguous (n, 2) float32");
  const int64_t n = E.size(0);
  const int64_t nbytes = n * 2 * (int64_t)sizeof(float);
  const char* pe = static_cast<const char*>(E.data_ptr());
  const char* po = static_cast<const char*>(out.data_ptr());
  AM_CHECK(n == 0 || pe + nbytes <= po || po + nbytes <= pe,
           "E and out must not overlap");
  AM_CHECK(reinterpret_cast<uintptr_t>(pe) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(po) % 8 == 0,
           "E and out must be 8-byte aligned (rows are read as float2)");
  AM_CHECK(idx.scalar_type() == at::kInt && thr.scalar_type() == at::kInt &&
               idx.dim() == 2 && idx.size(0) == n && idx.size(1) >= 1 &&
               thr.sizes() == idx.sizes() && idx.is_contiguous() &&
               thr.is_contiguous(),
           "idx/thr must be contiguous (n, k) int32 with k >= 1");
  const int64_t k = idx.size(1);
  AM_CHECK(n * k < (1ll << 31), "umap_epoch is limited to n*k < 2^31");
  AM_CHECK(in_off.scalar_type() == at::kInt &&
               in_edge.scalar_type() == at::kInt &&
               in_thr.scalar_type() == at::kInt && in_off.dim() == 1 &&
               in_edge.dim() == 1 && in_thr.dim() == 1 &&
               in_off.is_contiguous() && in_edge.is_contiguous() &&
               in_thr.is_contiguous(),
           "in_off/in_edge/in_thr must be contiguous 1-D int32");
  AM_CHECK(in_off.numel() == n + 1 && in_edge.numel() <= n * k &&
               in_thr.numel() == in_edge.numel(),
           "in_off must hold n+1 offsets, in_edge/in_thr at most n*k edges");
  AM_CHECK(neg >= 0 && neg <= 64, "neg must be in [0, 64]");
  AM_CHECK(epoch >= 0 && epoch < (1ll << 32), "epoch must fit 32 bits");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_umap_epoch(
      E.data_ptr<float>(), out.data_ptr<float>(), idx.data_ptr<int>(),
      thr.data_ptr<int>(), in_off.data_ptr<int>(), in_edge.data_ptr<int>(),
      in_thr.data_ptr<int>(), (int)n, (int)k, (int)in_edge.numel(), (int)neg,
      (float)alpha, (float)a, (float)b,
      (unsigned int)((uint64_t)seed & 0xFFFFFFFFull), (unsigned int)epoch,
      stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// The (B, n) buffers of the path ops are dense in one of two layouts:
// leg-major (contiguous) or vertex-major (the transpose of a contiguous
// (n, B) tensor). Returns 0 / 1 for the two, -1 for anything else.
static int path_layout(const torch::Tensor& t) {
  if (t.dim() != 2) return -1;
  if (t.is_contiguous()) return 0;
  if (t.stride(0) == 1 && t.stride(1) == t.size(0)) return 1;
  return -1;
}

// One Bellman-Ford sweep over the symmetrised kNN graph for B legs: reads
// dist_in/pred_in, writes dist_out/pred_out (all (B, n); in and out must not
// overlap). idx/w are (n, k); in_off (n+1) and in_edge are the reverse
// lists; allowed is an optional (n) uint8 mask; changed (B) int32 gets a 1
// for every leg in which some vertex improved.
static void path_relax(torch::Tensor dist_in, torch::Tensor pred_in,
                       torch::Tensor dist_out, torch::Tensor pred_out,
                       torch::Tensor idx, torch::Tensor w,
                       torch::Tensor in_off, torch::Tensor in_edge,
                       c10::optional<torch::Tensor> allowed,
                       torch::Tensor changed) {
  AM_CHECK(dist_in.is_cuda() && pred_in.is_cuda() && dist_out.is_cuda() &&
               pred_out.is_cuda() && idx.is_cuda() && w.is_cuda() &&
               in_off.is_cuda() && in_edge.is_cuda() && changed.is_cuda(),
           "path_relax needs GPU tensors");
  const int layout = path_layout(dist_in);
  AM_CHECK(dist_in.scalar_type() == at::kFloat &&
               dist_out.scalar_type() == at::kFloat && layout >= 0 &&
               dist_out.sizes() == dist_in.sizes() &&
               path_layout(dist_out) == layout,
           "dist_in/dist_out must be (B, n) float32, both contiguous or "
           "both the transpose of a contiguous (n, B) tensor");
  AM_CHECK(pred_in.scalar_type() == at::kInt &&
               pred_out.scalar_type() == at::kInt &&
               pred_in.sizes() == dist_in.sizes() &&
               pred_out.sizes() == dist_in.sizes() &&
               path_layout(pred_in) == layout &&
               path_layout(pred_out) == layout,
           "pred_in/pred_out must be (B, n) int32 in the layout of dist_in");
  const int64_t B = dist_in.size(0);
  const int64_t n = dist_in.size(1);
  AM_CHECK(B >= 1 && B <= 8, "path_relax takes 1 to 8 legs");
  const int64_t nbytes = B * n * 4;
  const char* bufs[4] = {static_cast<const char*>(dist_in.data_ptr()),
                         static_cast<const char*>(pred_in.data_ptr()),
                         static_cast<const char*>(dist_out.data_ptr()),
                         static_cast<const char*>(pred_out.data_ptr())};
  for (int i = 0; i < 4; ++i)
    for (int j = std::max(i + 1, 2); j < 4; ++j)
      AM_CHECK(n == 0 || bufs[i] + nbytes <= bufs[j] ||
                   bufs[j] + nbytes <= bufs[i],
               "path_relax in and out buffers must not overlap");
  for (int i = 0; i < 4; ++i)
    AM_CHECK(layout == 0 || reinterpret_cast<uintptr_t>(bufs[i]) % 16 == 0,
             "vertex-major buffers must be 16-byte aligned");
  AM_CHECK(idx.scalar_type() == at::kInt && w.scalar_type() == at::kFloat &&
               idx.dim() == 2 && idx.size(0) == n && idx.size(1) >= 1 &&
               w.sizes() == idx.sizes() && idx.is_contiguous() &&
               w.is_contiguous(),
           "idx must be contiguous (n, k) int32 and w (n, k) float32, k >= 1");
  const int64_t k = idx.size(1);
  AM_CHECK(n * k < (1ll << 31), "path_relax is limited to n*k < 2^31");
  AM_CHECK(in_off.scalar_type() == at::kInt &&
               in_edge.scalar_type() == at::kInt && in_off.dim() == 1 &&
               in_edge.dim() == 1 && in_off.is_contiguous() &&
               in_edge.is_contiguous(),
           "in_off/in_edge must be contiguous 1-D int32");
  AM_CHECK(in_off.numel() == n + 1 && in_edge.numel() <= n * k,
           "in_off must hold n+1 offsets, in_edge at most n*k edges");
  const unsigned char* allowed_p = nullptr;
  if (allowed.has_value()) {
    const torch::Tensor& a = *allowed;
    AM_CHECK(a.is_cuda() && a.scalar_type() == at::kByte && a.dim() == 1 &&
                 a.numel() == n && a.is_contiguous(),
             "allowed must be a contiguous (n) uint8 GPU tensor");
    allowed_p = a.data_ptr<unsigned char>();
  }
  AM_CHECK(changed.scalar_type() == at::kInt && changed.dim() == 1 &&
               changed.numel() == B && changed.is_contiguous(),
           "changed must be contiguous (B) int32");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_path_relax(
      dist_in.data_ptr<float>(), pred_in.data_ptr<int>(),
      dist_out.data_ptr<float>(), pred_out.data_ptr<int>(),
      idx.data_ptr<int>(), w.data_ptr<float>(), in_off.data_ptr<int>(),
      in_edge.data_ptr<int>(), allowed_p, changed.data_ptr<int>(), (int)B,
      (int)n, (int)k, (int)in_edge.numel(), layout, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// One component-label sweep over the symmetrised kNN graph: reads label_in
// (n), writes label_out (n) (they must not overlap). idx is (n, k); in_off
// (n+1) and in_edge are the reverse lists; changed (1) int32 gets a 1 when
// some label dropped.
static void graph_label_pull(torch::Tensor label_in, torch::Tensor label_out,
                             torch::Tensor idx, torch::Tensor in_off,
                             torch::Tensor in_edge, torch::Tensor changed) {
  AM_CHECK(label_in.is_cuda() && label_out.is_cuda() && idx.is_cuda() &&
               in_off.is_cuda() && in_edge.is_cuda() && changed.is_cuda(),
           "graph_label_pull needs GPU tensors");
  const auto dev = label_in.get_device();
  AM_CHECK(label_out.get_device() == dev && idx.get_device() == dev &&
               in_off.get_device() == dev && in_edge.get_device() == dev &&
               changed.get_device() == dev,
           "graph_label_pull needs all tensors on one device");
  AM_CHECK(label_in.scalar_type() == at::kInt &&
               label_out.scalar_type() == at::kInt && label_in.dim() == 1 &&
               label_out.sizes() == label_in.sizes(),
           "label_in/label_out must be (n) int32");
  const int64_t n = label_in.size(0);
  AM_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 2 &&
               idx.size(0) == n && idx.size(1) >= 1,
           "idx must be (n, k) int32, k >= 1");
  const int64_t k = idx.size(1);
  // by shape alone, before anything is read or assumed about the storage
  AM_CHECK(n < (1ll << 31) && k < (1ll << 31) && n * k < (1ll << 31),
           "graph_label_pull is limited to n*k < 2^31");
  AM_CHECK(label_in.is_contiguous() && label_out.is_contiguous() &&
               idx.is_contiguous(),
           "label_in, label_out and idx must be contiguous");
  const char* pi = static_cast<const char*>(label_in.data_ptr());
  const char* po = static_cast<const char*>(label_out.data_ptr());
  AM_CHECK(n == 0 || pi + n * 4 <= po || po + n * 4 <= pi,
           "label_in and label_out must not overlap");
  AM_CHECK(in_off.scalar_type() == at::kInt &&
               in_edge.scalar_type() == at::kInt && in_off.dim() == 1 &&
               in_edge.dim() == 1 && in_off.is_contiguous() &&
               in_edge.is_contiguous(),
           "in_off/in_edge must be contiguous 1-D int32");
  AM_CHECK(in_off.numel() == n + 1 && in_edge.numel() <= n * k,
           "in_off must hold n+1 offsets, in_edge at most n*k edges");
  AM_CHECK(changed.scalar_type() == at::kInt && changed.dim() == 1 &&
               changed.numel() == 1 && changed.is_contiguous(),
           "changed must be contiguous (1) int32");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_graph_label_pull(
      label_in.data_ptr<int>(), label_out.data_ptr<int>(),
      idx.data_ptr<int>(), in_off.data_ptr<int>(), in_edge.data_ptr<int>(),
      changed.data_ptr<int>(), (int)n, (int)k, (int)in_edge.numel(),
      stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// Follow pred (B, n) from dst[b] back to src[b] into out (B, T+1), target
// first; count (B) is the number of entries, -1 for an unreachable target.
static void path_walk(torch::Tensor dist, torch::Tensor pred,
                      torch::Tensor src, torch::Tensor dst, torch::Tensor out,
                      torch::Tensor count) {
  AM_CHECK(dist.is_cuda() && pred.is_cuda() && src.is_cuda() &&
               dst.is_cuda() && out.is_cuda() && count.is_cuda(),
           "path_walk needs GPU tensors");
  const int layout = path_layout(dist);
  AM_CHECK(dist.scalar_type() == at::kFloat && pred.scalar_type() == at::kInt &&
               layout >= 0 && pred.sizes() == dist.sizes() &&
               path_layout(pred) == layout,
           "dist must be (B, n) float32 and pred (B, n) int32, both "
           "contiguous or both the transpose of a contiguous (n, B) tensor");
  const int64_t B = dist.size(0);
  const int64_t n = dist.size(1);
  AM_CHECK(B >= 1 && B <= 8 && n >= 1 && n < (1ll << 31),
           "path_walk takes 1 to 8 legs over 1 <= n < 2^31 vertices");
  AM_CHECK(src.scalar_type() == at::kInt && dst.scalar_type() == at::kInt &&
               count.scalar_type() == at::kInt && src.dim() == 1 &&
               dst.dim() == 1 && count.dim() == 1 && src.numel() == B &&
               dst.numel() == B && count.numel() == B &&
               src.is_contiguous() && dst.is_contiguous() &&
               count.is_contiguous(),
           "src/dst/count must be contiguous (B) int32");
  AM_CHECK(out.scalar_type() == at::kInt && out.dim() == 2 &&
               out.size(0) == B && out.size(1) >= 1 &&
               out.size(1) < (1ll << 31) && out.is_contiguous(),
           "out must be contiguous (B, T+1) int32");
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_path_walk(dist.data_ptr<float>(), pred.data_ptr<int>(),
                              src.data_ptr<int>(), dst.data_ptr<int>(),
                              out.data_ptr<int>(), count.data_ptr<int>(),
                              (int)B, (int)n, (int)out.size(1), layout,
                              stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// One personalised-PageRank sweep over the symmetrised kNN graph for B legs:
// acc[b][v] = sum of s * x_in[b][u] over v's candidates (own slots, then its
// in-list). With restart (B, n), inv_deg (n) and q_out (B, n):
// p_out = (1 - alpha) * restart + alpha * acc and q_out = p_out * inv_deg.
// With all three absent: p_out = acc (the degree pass). idx/s are (n, k);
// in_off (n+1) and in_edge are the reverse lists; allowed is an optional (n)
// uint8 mask (vertices that are not allowed get 0). Outputs must not overlap
// the inputs or each other.
static void rank_pull(torch::Tensor x_in, torch::Tensor p_out,
                      c10::optional<torch::Tensor> q_out,
                      c10::optional<torch::Tensor> restart,
                      c10::optional<torch::Tensor> inv_deg, torch::Tensor idx,
                      torch::Tensor s, torch::Tensor in_off,
                      torch::Tensor in_edge,
                      c10::optional<torch::Tensor> allowed, double alpha) {
  const bool sweep = restart.has_value();
  AM_CHECK(q_out.has_value() == sweep && inv_deg.has_value() == sweep,
           "rank_pull takes q_out, restart and inv_deg together or not at all");
  AM_CHECK(x_in.is_cuda() && p_out.is_cuda() && idx.is_cuda() && s.is_cuda() &&
               in_off.is_cuda() && in_edge.is_cuda() &&
               (!sweep || (q_out->is_cuda() && restart->is_cuda() &&
                           inv_deg->is_cuda())),
           "rank_pull needs GPU tensors");
  const int layout = path_layout(x_in);
  AM_CHECK(x_in.scalar_type() == at::kFloat &&
               p_out.scalar_type() == at::kFloat && layout >= 0 &&
               p_out.sizes() == x_in.sizes() && path_layout(p_out) == layout,
           "x_in/p_out must be (B, n) float32, both contiguous or both the "
           "transpose of a contiguous (n, B) tensor");
  const int64_t B = x_in.size(0);
  const int64_t n = x_in.size(1);
  AM_CHECK(B >= 1 && B <= 8, "rank_pull takes 1 to 8 legs");
  if (sweep) {
    AM_CHECK(q_out->scalar_type() == at::kFloat &&
                 restart->scalar_type() == at::kFloat &&
                 q_out->sizes() == x_in.sizes() &&
                 restart->sizes() == x_in.sizes() &&
                 path_layout(*q_out) == layout &&
                 path_layout(*restart) == layout,
             "q_out/restart must be (B, n) float32 in the layout of x_in");
    AM_CHECK(inv_deg->scalar_type() == at::kFloat && inv_deg->dim() == 1 &&
                 inv_deg->numel() == n && inv_deg->is_contiguous(),
             "inv_deg must be contiguous (n) float32");
  }
  AM_CHECK(alpha >= 0.0 && (float)alpha < 1.0f,
           "rank_pull needs 0 <= alpha < 1 (in float32)");
  // {start, bytes}: inputs first, then the outputs
  const int64_t nbytes = B * n * 4;
  std::vector<std::pair<const char*, int64_t>> bufs;
  bufs.emplace_back(static_cast<const char*>(x_in.data_ptr()), nbytes);
  if (sweep) {
    bufs.emplace_back(static_cast<const char*>(restart->data_ptr()), nbytes);
    bufs.emplace_back(static_cast<const char*>(inv_deg->data_ptr()), n * 4);
  }
  const size_t first_out = bufs.size();
  bufs.emplace_back(static_cast<const char*>(p_out.data_ptr()), nbytes);
  if (sweep)
    bufs.emplace_back(static_cast<const char*>(q_out->data_ptr()), nbytes);
  for (size_t i = 0; i < bufs.size(); ++i)
    for (size_t j = std::max(i + 1, first_out); j < bufs.size(); ++j)
      AM_CHECK(n == 0 || bufs[i].first + bufs[i].second <= bufs[j].first ||
                   bufs[j].first + bufs[j].second <= bufs[i].first,
               "rank_pull outputs must not overlap the inputs or each other");
  for (size_t i = 0; i < bufs.size(); ++i)
    AM_CHECK(layout == 0 || (sweep && i == 2) ||
                 reinterpret_cast<uintptr_t>(bufs[i].first) % 16 == 0,
             "vertex-major buffers must be 16-byte aligned");
  AM_CHECK(idx.scalar_type() == at::kInt && s.scalar_type() == at::kFloat &&
               idx.dim() == 2 && idx.size(0) == n && idx.size(1) >= 1 &&
               s.sizes() == idx.sizes(),
           "idx must be (n, k) int32 and s (n, k) float32, k >= 1");
  const int64_t k = idx.size(1);
  AM_CHECK(n * k < (1ll << 31), "rank_pull is limited to n*k < 2^31");
  AM_CHECK(idx.is_contiguous() && s.is_contiguous(),
           "idx and s must be contiguous");
  AM_CHECK(in_off.scalar_type() == at::kInt &&
               in_edge.scalar_type() == at::kInt && in_off.dim() == 1 &&
               in_edge.dim() == 1 && in_off.is_contiguous() &&
               in_edge.is_contiguous(),
           "in_off/in_edge must be contiguous 1-D int32");
  AM_CHECK(in_off.numel() == n + 1 && in_edge.numel() <= n * k,
           "in_off must hold n+1 offsets, in_edge at most n*k edges");
  const unsigned char* allowed_p = nullptr;
  if (allowed.has_value()) {
    const torch::Tensor& a = *allowed;
    AM_CHECK(a.is_cuda() && a.scalar_type() == at::kByte && a.dim() == 1 &&
                 a.numel() == n && a.is_contiguous(),
             "allowed must be a contiguous (n) uint8 GPU tensor");
    allowed_p = a.data_ptr<unsigned char>();
  }
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_rank_pull(
      x_in.data_ptr<float>(), p_out.data_ptr<float>(),
      sweep ? q_out->data_ptr<float>() : nullptr,
      sweep ? restart->data_ptr<float>() : nullptr,
      sweep ? inv_deg->data_ptr<float>() : nullptr, idx.data_ptr<int>(),
      s.data_ptr<float>(), in_off.data_ptr<int>(), in_edge.data_ptr<int>(),
      allowed_p, (float)alpha, (int)B, (int)n, (int)k, (int)in_edge.numel(),
      layout, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

// One Louvain local-moving sweep over the symmetrised kNN graph: every
// vertex reads label_in (n) int32, tot (n) int64 (degree sum per community
// id) and deg (n) int64 and writes label_out (n). idx/w are (n, k) int32;
// in_off (n+1) and in_edge are the reverse lists. A = 64 * two_m, g = the
// resolution in 64ths, up the direction of the sweep. label_out must not
// overlap any input. The caller keeps max(64, g) * max_deg * two_m < 2^62.
static void community_move(torch::Tensor label_in, torch::Tensor label_out,
                           torch::Tensor tot, torch::Tensor deg,
                           torch::Tensor idx, torch::Tensor w,
                           torch::Tensor in_off, torch::Tensor in_edge,
                           int64_t A, int64_t g, bool up) {
  AM_CHECK(label_in.is_cuda() && label_out.is_cuda() && tot.is_cuda() &&
               deg.is_cuda() && idx.is_cuda() && w.is_cuda() &&
               in_off.is_cuda() && in_edge.is_cuda(),
           "community_move needs GPU tensors");
  AM_CHECK(label_in.scalar_type() == at::kInt &&
               label_out.scalar_type() == at::kInt && label_in.dim() == 1 &&
               label_out.dim() == 1 && label_in.is_contiguous() &&
               label_out.is_contiguous() &&
               label_out.numel() == label_in.numel(),
           "label_in/label_out must be contiguous (n) int32");
  const int64_t n = label_in.numel();
  AM_CHECK(tot.scalar_type() == at::kLong && deg.scalar_type() == at::kLong &&
               tot.dim() == 1 && deg.dim() == 1 && tot.numel() == n &&
               deg.numel() == n && tot.is_contiguous() && deg.is_contiguous(),
           "tot/deg must be contiguous (n) int64");
  AM_CHECK(idx.scalar_type() == at::kInt && w.scalar_type() == at::kInt &&
               idx.dim() == 2 && idx.size(0) == n && w.sizes() == idx.sizes(),
           "idx and w must be (n, k) int32");
  const int64_t k = idx.size(1);
  AM_CHECK(k >= 1 && k <= 32, "community_move takes 1 <= k <= 32");
  AM_CHECK(n * k < (1ll << 31), "community_move is limited to n*k < 2^31");
  AM_CHECK(idx.is_contiguous() && w.is_contiguous(),
           "idx and w must be contiguous");
  AM_CHECK(in_off.scalar_type() == at::kInt &&
               in_edge.scalar_type() == at::kInt && in_off.dim() == 1 &&
               in_edge.dim() == 1 && in_off.is_contiguous() &&
               in_edge.is_contiguous(),
           "in_off/in_edge must be contiguous 1-D int32");
  AM_CHECK(in_off.numel() == n + 1 && in_edge.numel() <= n * k,
           "in_off must hold n+1 offsets, in_edge at most n*k edges");
  AM_CHECK(A > 0, "community_move needs A > 0");
  AM_CHECK(g >= 1, "community_move needs g >= 1");
  // {start, bytes} of every input against the output
  const char* out0 = static_cast<const char*>(label_out.data_ptr());
  const int64_t out_bytes = n * 4;
  const std::pair<const char*, int64_t> ins[] = {
      {static_cast<const char*>(label_in.data_ptr()), n * 4},
      {static_cast<const char*>(tot.data_ptr()), n * 8},
      {static_cast<const char*>(deg.data_ptr()), n * 8},
      {static_cast<const char*>(idx.data_ptr()), n * k * 4},
      {static_cast<const char*>(w.data_ptr()), n * k * 4},
      {static_cast<const char*>(in_off.data_ptr()), (n + 1) * 4},
      {static_cast<const char*>(in_edge.data_ptr()), in_edge.numel() * 4}};
  for (const auto& in : ins)
    AM_CHECK(n == 0 || in.second == 0 || in.first + in.second <= out0 ||
                 out0 + out_bytes <= in.first,
             "community_move: label_out must not overlap an input");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_community_move(
      label_in.data_ptr<int>(), label_out.data_ptr<int>(),
      reinterpret_cast<const long long*>(tot.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(deg.data_ptr<int64_t>()),
      idx.data_ptr<int>(), w.data_ptr<int>(), in_off.data_ptr<int>(),
      in_edge.data_ptr<int>(), (long long)A, (long long)g, up ? 1 : 0, (int)n,
      (int)k, (int)in_edge.numel(), stream.stream());
  C10_HIP_CHECK(hipGetLastError());
}

static torch::Tensor layernorm_bf16(torch::Tensor x, torch::Tensor w,
                                    torch::Tensor b, double eps) {
  AM_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous(),
           "x must be contiguous bf16 on GPU");
  const int dim = x.size(-1);
  AM_CHECK(dim % 4 == 0 && dim <= 4096,
           "dim must be a multiple of 4 and <= 4096");
  AM_CHECK(w.is_contiguous() && b.is_contiguous() &&
               w.scalar_type() == at::kBFloat16 &&
               b.scalar_type() == at::kBFloat16 && w.numel() == dim &&
               b.numel() == dim,
           "w/b must be contiguous bf16 of size dim");
  auto y = torch::empty_like(x);
  const long long n_rows = x.numel() / dim;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_layernorm_bf16(x.data_ptr(), y.data_ptr(), w.data_ptr(),
                                   b.data_ptr(), n_rows, dim, (float)eps,
                                   stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return y;
}

static torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  AM_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16 &&
               A.is_contiguous() && A.size(0) == 16 && A.size(1) == 32,
           "A must be (16,32) bf16 GPU");
  AM_CHECK(B.is_cuda() && B.scalar_type() == at::kBFloat16 &&
               B.is_contiguous() && B.size(0) == 32 && B.size(1) == 16,
           "B must be (32,16) bf16 GPU");
  auto D = torch::empty({16, 16}, A.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_mfma_probe(A.data_ptr(), B.data_ptr(),
                               D.data_ptr<float>(), stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return D;
}

// xcd_grid picks the block-id mapping only (flat grid, heads of a window 8
// ids apart); the result is the same either way.
static torch::Tensor window_attn_fwd(torch::Tensor qkv, torch::Tensor bias,
                                     int64_t heads, int64_t shift,
                                     double scale, bool xcd_grid,
                                     c10::optional<torch::Tensor> out_opt) {
  AM_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
               qkv.is_contiguous() && qkv.dim() == 4,
           "qkv must be (B, H, W, 3C) bf16 contiguous GPU");
  const int64_t Bn = qkv.size(0), H = qkv.size(1), W = qkv.size(2);
  const int64_t C = qkv.size(3) / 3;
  AM_CHECK(qkv.size(3) == 3 * C && C == heads * 32,
           "C must be heads*32 and last dim 3C");
  AM_CHECK(H % 8 == 0 && W % 8 == 0, "H, W must be multiples of 8");
  AM_CHECK(heads % 2 == 0, "heads must be a multiple of 2");
  AM_CHECK(bias.is_cuda() && bias.scalar_type() == at::kBFloat16 &&
               bias.is_contiguous() && bias.numel() == heads * 64 * 64,
           "bias must be (heads, 64, 64) bf16 contiguous");
  const int64_t n_windows = Bn * (H / 8) * (W / 8);
  AM_CHECK(n_windows > 0 && (n_windows + 7) / 8 * 8 * heads < (1ll << 31),
           "too many windows for one launch");
  torch::Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    AM_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 &&
                 out.is_contiguous() && out.dim() == 4 && out.size(0) == Bn &&
                 out.size(1) == H && out.size(2) == W && out.size(3) == C &&
                 out.get_device() == qkv.get_device(),
             "out must be a contiguous (B, H, W, C) bf16 GPU tensor");
  } else {
    out = torch::empty({Bn, H, W, C}, qkv.options());
  }
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_window_attn(qkv.data_ptr(), out.data_ptr(),
                                bias.data_ptr(), (int)Bn, (int)H,
                                (int)W, (int)C, (int)heads, (int)shift,
                                (float)scale, xcd_grid, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

static torch::Tensor window_attn_fp8_fwd(torch::Tensor qkv,
                                         torch::Tensor bias,
                                         torch::Tensor q_scale,
                                         int64_t heads, int64_t shift,
                                         double sm_scale) {
  AM_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kFloat8_e4m3fn &&
               qkv.is_contiguous() && qkv.dim() == 4,
           "qkv must be (B, H, W, 3C) fp8e4m3 contiguous GPU");
  const int64_t Bn = qkv.size(0), H = qkv.size(1), W = qkv.size(2);
  const int64_t C = qkv.size(3) / 3;
  AM_CHECK(qkv.size(3) == 3 * C && C == heads * 32,
           "C must be heads*32 and last dim 3C");
  AM_CHECK(H % 8 == 0 && W % 8 == 0, "H, W must be multiples of 8");
  AM_CHECK(bias.is_cuda() && bias.scalar_type() == at::kBFloat16 &&
               bias.is_contiguous() && bias.numel() == heads * 64 * 64,
           "bias must be (heads, 64, 64) bf16 contiguous");
  AM_CHECK(q_scale.is_cuda() && q_scale.scalar_type() == at::kFloat &&
               q_scale.numel() == 1,
           "q_scale must be a f32 device scalar");
  auto out = torch::empty({Bn, H, W, C},
                          qkv.options().dtype(at::kBFloat16));
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_window_attn_fp8(
      qkv.data_ptr(), out.data_ptr(), bias.data_ptr(), q_scale.data_ptr(),
      (int)Bn, (int)H, (int)W, (int)C, (int)heads, (int)shift,
      (float)sm_scale, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

static torch::Tensor window_attn4_fwd(torch::Tensor qkv, torch::Tensor bias,
                                      int64_t heads, int64_t shift,
                                      double scale) {
  AM_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
               qkv.is_contiguous() && qkv.dim() == 4,
           "qkv must be (B, H, W, 3C) bf16 contiguous GPU");
  const int64_t Bn = qkv.size(0), H = qkv.size(1), W = qkv.size(2);
  const int64_t C = qkv.size(3) / 3;
  AM_CHECK(qkv.size(3) == 3 * C && C == heads * 32,
           "C must be heads*32 and last dim 3C");
  AM_CHECK(H % 4 == 0 && W % 4 == 0, "H, W must be multiples of 4");
  AM_CHECK(bias.is_cuda() && bias.scalar_type() == at::kBFloat16 &&
               bias.is_contiguous() && bias.numel() == heads * 16 * 16,
           "bias must be (heads, 16, 16) bf16 contiguous");
  auto out = torch::empty({Bn, H, W, C}, qkv.options());
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_window_attn4(qkv.data_ptr(), out.data_ptr(),
                                 bias.data_ptr(), (int)Bn, (int)H,
                                 (int)W, (int)C, (int)heads, (int)shift,
                                 (float)scale, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// Shared argument checks of the add / fp8 LayerNorm bindings: everything
// the kernels index is validated here, before any launch.
static void check_ln_params(const torch::Tensor& x, const torch::Tensor& w,
                            const torch::Tensor& b, int dim) {
  AM_CHECK(x.numel() > 0, "x must not be empty");
  auto ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.get_device() == x.get_device() &&
           t.is_contiguous() && t.scalar_type() == at::kBFloat16 &&
           t.numel() == dim;
  };
  AM_CHECK(ok(w) && ok(b),
           "w/b must be contiguous bf16 of size dim on x's device");
}

static void check_ln_other(const torch::Tensor& x, const torch::Tensor& other) {
  AM_CHECK(other.is_cuda() && other.get_device() == x.get_device() &&
               other.is_contiguous() && other.sizes() == x.sizes() &&
               other.scalar_type() == at::kBFloat16,
           "other must match x and be on its device");
}

// the kernels read scale[0] and write amax[blockIdx.x & 255]
static void check_ln_fp8_state(const torch::Tensor& x,
                               const torch::Tensor& scale,
                               const torch::Tensor& amax) {
  AM_CHECK(scale.is_cuda() && scale.get_device() == x.get_device() &&
               scale.scalar_type() == at::kFloat && scale.numel() >= 1,
           "scale must be f32 with at least 1 element on x's device");
  AM_CHECK(amax.is_cuda() && amax.get_device() == x.get_device() &&
               amax.scalar_type() == at::kFloat && amax.is_contiguous() &&
               amax.numel() >= 256,
           "amax must be contiguous f32 with at least 256 slots on x's device");
}

static std::vector<torch::Tensor> add_layernorm_bf16(torch::Tensor x,
                                                     torch::Tensor other,
                                                     torch::Tensor w,
                                                     torch::Tensor b,
                                                     double eps) {
  AM_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous(),
           "x must be contiguous bf16 on GPU");
  check_ln_other(x, other);
  const int dim = x.size(-1);
  AM_CHECK(dim % 4 == 0 && dim <= 4096, "dim must be /4 and <= 4096");
  check_ln_params(x, w, b, dim);
  auto sum = torch::empty_like(x);
  auto y = torch::empty_like(x);
  const long long n_rows = x.numel() / dim;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_add_layernorm_bf16(
      x.data_ptr(), other.data_ptr(), sum.data_ptr(), y.data_ptr(),
      w.data_ptr(), b.data_ptr(), n_rows, dim, (float)eps, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return {sum, y};
}

static torch::Tensor layernorm_bf16_fp8(torch::Tensor x, torch::Tensor w,
                                        torch::Tensor b, double eps,
                                        torch::Tensor scale,
                                        torch::Tensor amax) {
  AM_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous(),
           "x must be contiguous bf16 on GPU");
  check_ln_fp8_state(x, scale, amax);
  const int dim = x.size(-1);
  AM_CHECK(dim % 4 == 0 && dim <= 4096, "dim must be /4 and <= 4096");
  check_ln_params(x, w, b, dim);
  auto y8 = torch::empty(x.sizes(),
                         x.options().dtype(at::kFloat8_e4m3fn));
  const long long n_rows = x.numel() / dim;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_layernorm_bf16_fp8_impl(
      x.data_ptr(), y8.data_ptr(), w.data_ptr(), b.data_ptr(), nullptr,
      nullptr, scale.data_ptr<float>(), amax.data_ptr<float>(), n_rows, dim,
      (float)eps, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return y8;
}

static std::vector<torch::Tensor> add_layernorm_bf16_fp8(
    torch::Tensor x, torch::Tensor other, torch::Tensor w, torch::Tensor b,
    double eps, torch::Tensor scale, torch::Tensor amax) {
  AM_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous(),
           "x must be contiguous bf16 on GPU");
  check_ln_other(x, other);
  check_ln_fp8_state(x, scale, amax);
  const int dim = x.size(-1);
  AM_CHECK(dim % 4 == 0 && dim <= 4096, "dim must be /4 and <= 4096");
  check_ln_params(x, w, b, dim);
  auto sum = torch::empty_like(x);
  auto y8 = torch::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
  const long long n_rows = x.numel() / dim;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_layernorm_bf16_fp8_impl(
      x.data_ptr(), y8.data_ptr(), w.data_ptr(), b.data_ptr(),
      other.data_ptr(), sum.data_ptr(), scale.data_ptr<float>(),
      amax.data_ptr<float>(), n_rows, dim, (float)eps, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return {sum, y8};
}

static torch::Tensor merge_layernorm_bf16(torch::Tensor x, torch::Tensor w,
                                          torch::Tensor b, double eps) {
  AM_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
               x.is_contiguous() && x.dim() == 4,
           "x must be (B, H, W, C) bf16 contiguous GPU");
  const int64_t Bn = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  AM_CHECK(H % 2 == 0 && W % 2 == 0, "H, W must be even");
  AM_CHECK(C % 4 == 0 && 4 * C > 128 && 4 * C <= 4096,
           "C must be a multiple of 4 with 128 < 4C <= 4096");
  AM_CHECK(w.is_cuda() && b.is_cuda() && w.is_contiguous() &&
               b.is_contiguous() && w.scalar_type() == at::kBFloat16 &&
               b.scalar_type() == at::kBFloat16 && w.numel() == 4 * C &&
               b.numel() == 4 * C,
           "w/b must be contiguous bf16 of size 4C");
  auto y = torch::empty({Bn, (H / 2) * (W / 2), 4 * C}, x.options());
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_merge_layernorm_bf16(x.data_ptr(), y.data_ptr(),
                                         w.data_ptr(), b.data_ptr(), (int)Bn,
                                         (int)H, (int)W, (int)C, (float)eps,
                                         stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return y;
}

static torch::Tensor mlp_fused(torch::Tensor x, torch::Tensor proj,
                               torch::Tensor ln_w, torch::Tensor ln_b,
                               double eps, torch::Tensor w1, torch::Tensor b1,
                               torch::Tensor w2, torch::Tensor b2,
                               c10::optional<torch::Tensor> out_opt) {
  auto ok = [](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
           t.is_contiguous();
  };
  AM_CHECK(ok(x) && ok(proj) && ok(ln_w) && ok(ln_b) && ok(w1) && ok(b1) &&
               ok(w2) && ok(b2),
           "all inputs must be contiguous bf16 GPU tensors");
  AM_CHECK(x.dim() >= 1, "x must have a channel dimension");
  const int64_t C = x.size(-1);
  AM_CHECK(C == 128 || C == 256, "mlp_fused is built for C = 128 and C = 256");
  const int64_t M = x.numel() / C;
  // tokens per workgroup of either kernel (MLP_BM, M2_BM in mlp_fused.hip)
  AM_CHECK(M > 0 && M % 128 == 0, "token count must be a multiple of 128");
  AM_CHECK(M / 128 < (1ll << 31), "too many tokens for one launch");
  AM_CHECK(proj.sizes() == x.sizes(), "proj must match x");
  AM_CHECK(ln_w.numel() == C && ln_b.numel() == C, "LN weight/bias size");
  AM_CHECK(w1.dim() == 2 && w1.size(0) == 4 * C && w1.size(1) == C &&
               b1.numel() == 4 * C,
           "w1 must be (4C, C), b1 (4C)");
  AM_CHECK(w2.dim() == 2 && w2.size(0) == C && w2.size(1) == 4 * C &&
               b2.numel() == C,
           "w2 must be (C, 4C), b2 (C)");
  torch::Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    AM_CHECK(ok(out) && out.sizes() == x.sizes() &&
                 out.get_device() == x.get_device(),
             "out must be a contiguous bf16 GPU tensor shaped like x");
    AM_CHECK(out.data_ptr() != x.data_ptr() &&
                 out.data_ptr() != proj.data_ptr(),
             "out must not alias x or proj");
  } else {
    out = torch::empty_like(x);
  }
  auto stream = c10::hip::getCurrentHIPStream();
  auto launch = C == 128 ? audiomuse::launch_mlp_fused_c128
                         : audiomuse::launch_mlp_fused_c256;
  launch(x.data_ptr(), proj.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
         w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
         out.data_ptr(), (long long)M, (float)eps, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// LN -> QKV -> window attention -> proj of a C = 128, 4-head, window-8
// block in one launch; returns proj (the caller adds the residual).
static torch::Tensor attn_block_fused(
    torch::Tensor x, torch::Tensor ln_w, torch::Tensor ln_b, double eps,
    torch::Tensor qkv_w, torch::Tensor qkv_b, torch::Tensor proj_w,
    torch::Tensor proj_b, torch::Tensor bias, int64_t shift, double scale,
    c10::optional<torch::Tensor> out) {
  auto ok = [](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
           t.is_contiguous();
  };
  AM_CHECK(ok(x) && ok(ln_w) && ok(ln_b) && ok(qkv_w) && ok(qkv_b) &&
               ok(proj_w) && ok(proj_b) && ok(bias),
           "all inputs must be contiguous bf16 GPU tensors");
  AM_CHECK(x.dim() == 4, "x must be (B, H, W, C)");
  const int64_t Bn = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  AM_CHECK(C == 128, "attn_block_fused is built for C = 128");
  AM_CHECK(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
           "H, W must be multiples of 8");
  AM_CHECK(shift == 0 || shift == 4, "shift must be 0 or 4");
  AM_CHECK(Bn > 0 && Bn * (H / 8) * (W / 8) < (1ll << 31) &&
               H < (1 << 30) && W < (1 << 30),
           "too many windows for one launch");
  AM_CHECK(ln_w.numel() == C && ln_b.numel() == C, "LN weight/bias size");
  AM_CHECK(qkv_w.dim() == 2 && qkv_w.size(0) == 3 * C && qkv_w.size(1) == C &&
               qkv_b.numel() == 3 * C,
           "qkv_w must be (3C, C), qkv_b (3C)");
  AM_CHECK(proj_w.dim() == 2 && proj_w.size(0) == C && proj_w.size(1) == C &&
               proj_b.numel() == C,
           "proj_w must be (C, C), proj_b (C)");
  AM_CHECK(bias.dim() == 3 && bias.size(0) == 4 && bias.size(1) == 64 &&
               bias.size(2) == 64,
           "bias must be (4, 64, 64): 4 heads of 32");
  torch::Tensor o;
  if (out.has_value()) {
    o = *out;
    AM_CHECK(ok(o) && o.sizes() == x.sizes() &&
                 o.get_device() == x.get_device(),
             "out must be a contiguous bf16 GPU tensor shaped like x");
    AM_CHECK(o.data_ptr() != x.data_ptr(), "out must not alias x");
  } else {
    o = torch::empty_like(x);
  }
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_attn_fused_c128(
      x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), qkv_w.data_ptr(),
      qkv_b.data_ptr(), proj_w.data_ptr(), proj_b.data_ptr(), bias.data_ptr(),
      o.data_ptr(), (int)Bn, (int)H, (int)W, (int)shift, (float)scale,
      (float)eps, stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return o;
}

// Best alignment of fingerprint pairs: words (W,) int32 bit patterns, off
// (F+1,) int64, pairs (P, 2) int32 -> (P, 3) int32 (bits, n, offset).
// lds_words is the LDS room per fingerprint; the caller keeps longer
// fingerprints away (engines/chromaprint.match_pairs routes them) and has
// checked the contents of off and pairs on the device.
static torch::Tensor fp_align(torch::Tensor words, torch::Tensor off,
                              torch::Tensor pairs, int64_t max_offset,
                              int64_t min_words, int64_t lds_words) {
  AM_CHECK(words.is_cuda() && off.is_cuda() && pairs.is_cuda(),
           "fp_align needs GPU tensors");
  AM_CHECK(words.get_device() == off.get_device() &&
               words.get_device() == pairs.get_device(),
           "words, off and pairs must be on one device");
  AM_CHECK(words.scalar_type() == at::kInt && words.dim() == 1 &&
               words.is_contiguous(),
           "words must be a contiguous (W,) int32 tensor");
  AM_CHECK(off.scalar_type() == at::kLong && off.dim() == 1 &&
               off.is_contiguous() && off.numel() >= 1,
           "off must be a contiguous (F+1,) int64 tensor");
  AM_CHECK(pairs.scalar_type() == at::kInt && pairs.dim() == 2 &&
               pairs.size(1) == 2 && pairs.is_contiguous(),
           "pairs must be a contiguous (P, 2) int32 tensor");
  AM_CHECK(max_offset >= 0 && max_offset <= 1024,
           "max_offset must be in [0, 1024]");
  AM_CHECK(min_words >= 1, "min_words must be >= 1");
  AM_CHECK(lds_words >= 1 && lds_words <= 4096,
           "lds_words must be in [1, 4096]");
  const int64_t F = off.numel() - 1;
  const int64_t P = pairs.size(0);
  AM_CHECK(F < (1ll << 31) && P < (1ll << 31),
           "fp_align is limited to F, P < 2^31");
  auto out = torch::empty({P, 3}, pairs.options());
  if (P == 0) return out;
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_fp_align(
      words.data_ptr<int>(),
      reinterpret_cast<const long long*>(off.data_ptr<int64_t>()),
      pairs.data_ptr<int>(), out.data_ptr<int>(), (long long)words.numel(),
      (int)F, (long long)P, (int)max_offset,
      (int)std::min<int64_t>(min_words, 1 << 30), (int)lds_words,
      stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// Patch embedding of the encoder: pad/crop to n_frames, 4x4 patches, linear.
static torch::Tensor patch_embed_bf16(torch::Tensor mel, torch::Tensor weight,
                                      torch::Tensor bias, int64_t n_frames) {
  auto ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
           t.is_contiguous() && t.get_device() == mel.get_device();
  };
  AM_CHECK(ok(mel) && ok(weight) && ok(bias),
           "mel, weight and bias must be contiguous bf16 tensors on one GPU");
  AM_CHECK(mel.dim() == 3, "mel must be (B, n_mels, T)");
  const int64_t Bn = mel.size(0), M = mel.size(1), T = mel.size(2);
  AM_CHECK(weight.dim() == 2 && weight.size(1) == 16,
           "weight must be (C, 16): 4x4 patches");
  const int64_t C = weight.size(0);
  AM_CHECK(C >= 8 && C <= 2048 && (C & (C - 1)) == 0,
           "C must be a power of two in [8, 2048]");
  AM_CHECK(bias.numel() == C, "bias must have C elements");
  AM_CHECK(reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
           "weight must be 16-byte aligned");
  AM_CHECK(M >= 4 && M % 4 == 0 && n_frames >= 4 && n_frames % 4 == 0 &&
               n_frames <= 8192,
           "n_mels and n_frames must be multiples of 4, n_frames <= 8192");
  AM_CHECK(Bn >= 1 && T >= 1 && T < (1ll << 31) && Bn * (M / 4) < (1ll << 31),
           "patch_embed_bf16: batch too large for one launch");
  auto out = torch::empty({Bn, (M / 4) * (n_frames / 4), C}, mel.options());
  auto stream = c10::hip::getCurrentHIPStream();
  audiomuse::launch_patch_embed_bf16(mel.data_ptr(), weight.data_ptr(),
                                     bias.data_ptr(), out.data_ptr(), (int)Bn,
                                     (int)M, (int)T, (int)n_frames, (int)C,
                                     stream.stream());
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

void register_gemm_gelu(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "AudioMuse-AMD native CDNA4 kernels";
  register_gemm_gelu(m);
  m.def("add_layernorm_bf16", &add_layernorm_bf16,
        "Fused residual add + LayerNorm: returns (x+other, LN(x+other))");
  m.def("layernorm_bf16_fp8", &layernorm_bf16_fp8,
        "LayerNorm with fused e4m3 quantize (delayed scale + amax)");
  m.def("add_layernorm_bf16_fp8", &add_layernorm_bf16_fp8,
        "Residual add + LN with fused e4m3 quantize: (sum bf16, y fp8)");
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
  m.def("window_attn_fp8_fwd", &window_attn_fp8_fwd,
        "fused shifted-window attention, fp8-ingest QKV (e4m3 + device "
        "dequant scale), bf16 MFMAs/out");
  m.def("window_attn_fwd", &window_attn_fwd,
        "Fused shifted-window attention (qkv BHW3C bf16, bias, heads, "
        "shift, scale, xcd_grid=False, out=None) -> (B,H,W,C); xcd_grid "
        "launches the flat grid that keeps a window's heads on one XCD",
        pybind11::arg("qkv"), pybind11::arg("bias"), pybind11::arg("heads"),
        pybind11::arg("shift"), pybind11::arg("scale"),
        pybind11::arg("xcd_grid") = false,
        pybind11::arg("out") = pybind11::none());
  m.def("merge_layernorm_bf16", &merge_layernorm_bf16,
        "LayerNorm over 2x2-merged patches gathered from (B,H,W,C): "
        "(x, w, b, eps) -> (B, H/2*W/2, 4C)");
  m.def("mlp_fused", &mlp_fused,
        "x2 = x + proj; out = x2 + W2 gelu_tanh(W1 LN(x2) + b1) + b2 in one "
        "launch, C = 128 or 256, hidden 4C (x, proj, ln_w, ln_b, eps, w1, b1, "
        "w2, b2, out=None)",
        pybind11::arg("x"), pybind11::arg("proj"), pybind11::arg("ln_w"),
        pybind11::arg("ln_b"), pybind11::arg("eps"), pybind11::arg("w1"),
        pybind11::arg("b1"), pybind11::arg("w2"), pybind11::arg("b2"),
        pybind11::arg("out") = pybind11::none());
  m.def("attn_block_fused", &attn_block_fused,
        "LN -> QKV -> 8x8 window attention -> proj in one launch, C = 128, "
        "4 heads; returns proj (x, ln_w, ln_b, eps, qkv_w, qkv_b, proj_w, "
        "proj_b, bias (4,64,64), shift, scale, out=None) -> (B,H,W,128)",
        pybind11::arg("x"), pybind11::arg("ln_w"), pybind11::arg("ln_b"),
        pybind11::arg("eps"), pybind11::arg("qkv_w"), pybind11::arg("qkv_b"),
        pybind11::arg("proj_w"), pybind11::arg("proj_b"),
        pybind11::arg("bias"), pybind11::arg("shift"), pybind11::arg("scale"),
        pybind11::arg("out") = pybind11::none());
  m.def("window_attn4_fwd", &window_attn4_fwd,
        "Fused 4x4-window attention for stage 4 (qkv BHW3C bf16, "
        "bias (heads,16,16), heads, shift, scale) -> (B,H,W,C)");
  m.def("layernorm_bf16", &layernorm_bf16,
        "Fused LayerNorm forward, bf16 in/out, fp32 stats (x, w, b, eps)");
  m.def("mel_fwd", &mel_fwd,
        "Fused STFT+mel+log spectrogram (audio, window, twiddle, rowptr, "
        "bin, w, hop, n_fft, center, log_mode, quant16, band_first=None, "
        "band_len=None, band_off=None, band_w=None, kmax=0, allow_v2=False, "
        "out=None); with a band plan and allow_v2 the multi-frame kernel "
        "takes the configurations mel_fwd_takes_v2 names",
        pybind11::arg("audio"), pybind11::arg("window"),
        pybind11::arg("twiddle"), pybind11::arg("mel_rowptr"),
        pybind11::arg("mel_bin"), pybind11::arg("mel_w"), pybind11::arg("hop"),
        pybind11::arg("n_fft"), pybind11::arg("center"),
        pybind11::arg("log_mode"), pybind11::arg("quant16"),
        pybind11::arg("band_first") = pybind11::none(),
        pybind11::arg("band_len") = pybind11::none(),
        pybind11::arg("band_off") = pybind11::none(),
        pybind11::arg("band_w") = pybind11::none(),
        pybind11::arg("kmax") = 0, pybind11::arg("allow_v2") = false,
        pybind11::arg("out") = pybind11::none());
  m.def("mel_fwd_takes_v2",
        [](int64_t n_fft, int64_t hop, int64_t n_mels, bool center,
           int64_t kmax) {
          return audiomuse::mel_fwd_takes_v2((int)n_fft, (int)hop, (int)n_mels,
                                             center ? 1 : 0, (int)kmax, 1,
                                             true);
        },
        "whether mel_fwd runs the multi-frame kernel for this configuration "
        "when it is allowed and a band plan is given");
  m.def("patch_embed_bf16", &patch_embed_bf16,
        "4x4 patch embedding in one launch: (mel (B, n_mels, T) bf16, weight "
        "(C, 16) bf16, bias (C) bf16, n_frames) -> (B, n_mels/4 * n_frames/4, "
        "C) bf16; frames T..n_frames read as zero, frames past n_frames are "
        "ignored");
  m.def("ivf_scan", &ivf_scan,
        "IVF probed-cell distance scan (dtype, metric, query, qnorm, data, "
        "row_norm, probe, cell_off, cand_off, out_dist, out_row, dim_pad)");
  m.def("ivf_scan_sel", &ivf_scan_sel,
        "IVF probed-cell scan over a row selection (dtype, metric, query, "
        "qnorm, data, row_norm, probe, sel_rows, sel_off, cand_off, out_dist, "
        "out_row, dim_pad)");
  m.def("ivf_scan_topk", &ivf_scan_topk,
        "IVF probed-cell scan that keeps the K best per (query, split) "
        "(dtype, metric, query, qnorm, data, row_norm, probe, cell_off, "
        "sel_rows|None, sel_off|None, skip_row|None, out_dist (Q,S,K), "
        "out_row (Q,S,K), dim_pad)");
  m.def("ivf_scan_topk_excl", &ivf_scan_topk_excl,
        "ivf_scan_topk without a row selection that never reports a row "
        "whose label is the query's (dtype, metric, query, qnorm, data, "
        "row_norm, probe, cell_off, skip_row|None, row_label (N,), q_label "
        "(Q,), out_dist (Q,S,K), out_row (Q,S,K), dim_pad)");
  m.def("graph_label_pull", &graph_label_pull,
        "One component-label sweep over the symmetrised kNN graph (label_in, "
        "label_out, idx, in_off, in_edge, changed): pull pass with the "
        "shortcut label_out[v] = label_in[min over v and its candidates]");
  m.def("umap_epoch", &umap_epoch,
        "One epoch of the 2-D map layout, one launch (E, out, idx, thr, "
        "in_off, in_edge, in_thr, alpha, a, b, seed, epoch, neg)");
  m.def("path_relax", &path_relax,
        "One Bellman-Ford sweep over the symmetrised kNN graph for up to 8 "
        "legs (pull pass, ping-pong buffers)");
  m.def("path_walk", &path_walk,
        "Follow shortest-path predecessors from each target to its source");
  m.def("rank_pull", &rank_pull,
        "One personalised-PageRank sweep over the symmetrised kNN graph for "
        "up to 8 legs (x_in, p_out, q_out, restart, inv_deg, idx, s, in_off, "
        "in_edge, allowed, alpha); without q_out/restart/inv_deg the plain "
        "weighted sum (the degree pass)");
  m.def("community_move", &community_move,
        "One Louvain local-moving sweep over the symmetrised kNN graph "
        "(label_in, label_out, tot, deg, idx, w, in_off, in_edge, A, g, up): "
        "integer arithmetic, one owner lane per vertex");
  m.def("fp_align", &fp_align,
        "Best alignment of fingerprint pairs (words int32 (W,), off int64 "
        "(F+1,), pairs int32 (P, 2), max_offset, min_words, lds_words) -> "
        "(P, 3) int32 (bits, n, offset)");
  m.attr("gfx_arch") = "gfx950";
}
