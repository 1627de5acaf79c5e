"""One-launch residual add + LayerNorm + MLP kernel (GPU, C = 128).

Reference: fp32 torch evaluation of
    x2 = x + proj;  out = x2 + W2 . gelu_tanh(W1 . LN(x2) + b1) + b2
from the same bf16 inputs. The three-op path (add_layernorm_bf16 ->
linear_gelu -> linear_bias_add) has the same rounding points and differs
only in summation order, so the fused kernel's max-abs and mean-abs
errors must stay within 1.5x of the three-op path's; anything beyond that
is a layout or indexing bug.
"""

import pytest
import torch
import torch.nn.functional as F

BM = 128
C = 128
HID = 512
EPS = 1e-5


def _inputs(M, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    # rows with different means and scales
    row_scale = torch.linspace(0.3, 2.0, M, device="cuda")[:, None]
    row_mean = torch.linspace(-1.0, 1.5, M, device="cuda")[:, None]
    x = (rn(M, C) * row_scale + row_mean).to(torch.bfloat16)
    proj = (rn(M, C) * 0.5 + 0.1).to(torch.bfloat16)
    ln_w = (1.0 + 0.3 * rn(C)).to(torch.bfloat16)
    ln_b = (0.2 * rn(C)).to(torch.bfloat16)
    # asymmetric weights: column- and row-dependent scale
    w1 = (rn(HID, C) * C ** -0.5
          * torch.linspace(0.5, 1.5, C, device="cuda")[None, :]
          * torch.linspace(0.7, 1.3, HID, device="cuda")[:, None]
          ).to(torch.bfloat16)
    b1 = (0.3 * rn(HID)).to(torch.bfloat16)
    w2 = (rn(C, HID) * HID ** -0.5
          * torch.linspace(0.5, 1.5, HID, device="cuda")[None, :]
          * torch.linspace(1.3, 0.7, C, device="cuda")[:, None]
          ).to(torch.bfloat16)
    b2 = (0.3 * rn(C)).to(torch.bfloat16)
    return [t.contiguous() for t in (x, proj, ln_w, ln_b, w1, b1, w2, b2)]


def _fp32_reference(x, proj, ln_w, ln_b, w1, b1, w2, b2):
    x2 = x.float() + proj.float()
    xn = F.layer_norm(x2, (C,), ln_w.float(), ln_b.float(), EPS)
    h = F.gelu(xn @ w1.float().t() + b1.float(), approximate="tanh")
    return x2 + h @ w2.float().t() + b2.float()


def _three_op(ext, x, proj, ln_w, ln_b, w1, b1, w2, b2):
    x2, xn2 = ext.add_layernorm_bf16(x, proj, ln_w, ln_b, EPS)
    hidden = ext.linear_gelu(xn2, w1, b1)
    return ext.linear_bias_add(hidden, w2, b2, x2)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [BM, 3 * BM])
def test_fused_mlp_error_within_three_op_path(M):
    import audiomuse_amd._C as ext

    args = _inputs(M, seed=17 + M)
    ref = _fp32_reference(*args)
    three = _three_op(ext, *args).float()
    x, proj, ln_w, ln_b, w1, b1, w2, b2 = args
    fused = ext.mlp_fused(x, proj, ln_w, ln_b, EPS, w1, b1, w2, b2).float()

    e3 = (three - ref).abs()
    ef = (fused - ref).abs()
    print(f"M={M}: three-op max {float(e3.max()):.5f} mean "
          f"{float(e3.mean()):.6f}; fused max {float(ef.max()):.5f} mean "
          f"{float(ef.mean()):.6f}; ref mean-abs {float(ref.abs().mean()):.4f}")
    assert torch.isfinite(fused).all()
    assert float(ef.max()) <= 1.5 * float(e3.max()), \
        f"fused max-abs {float(ef.max()):.5f} vs three-op {float(e3.max()):.5f}"
    assert float(ef.mean()) <= 1.5 * float(e3.mean()), \
        f"fused mean-abs {float(ef.mean()):.6f} vs three-op {float(e3.mean()):.6f}"


@pytest.mark.gpu
def test_binding_rejects_partial_tile():
    import audiomuse_amd._C as ext

    x, proj, ln_w, ln_b, w1, b1, w2, b2 = _inputs(BM + 64, seed=3)
    with pytest.raises(RuntimeError):
        ext.mlp_fused(x, proj, ln_w, ln_b, EPS, w1, b1, w2, b2)


@pytest.mark.gpu
def test_model_dispatch_falls_back_when_not_tile_multiple():
    """A token count that is not a multiple of BM goes through the model
    dispatch and must give exactly the three-op result."""
    import audiomuse_amd._C as ext
    from audiomuse_amd import config
    from audiomuse_amd.models.htsat import SwinBlock

    assert config.MLP_FUSED_ENABLE
    torch.manual_seed(9)
    blk = SwinBlock(C, 4, window=8, shift=0, mlp_ratio=4.0)
    blk = blk.to("cuda", torch.bfloat16).eval()
    M = BM + 64
    x = torch.randn(1, M, C, device="cuda", dtype=torch.bfloat16)
    attn_out = torch.randn(1, M, C, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        got = blk._mlp_half(ext, x, attn_out)
        want = _three_op(
            ext, x, attn_out,
            blk.norm2.weight.contiguous(), blk.norm2.bias.contiguous(),
            blk.mlp[0].weight.contiguous(), blk.mlp[0].bias.contiguous(),
            blk.mlp[2].weight.contiguous(), blk.mlp[2].bias.contiguous())
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_model_dispatch_uses_fused_kernel_on_tile_multiple():
    import audiomuse_amd._C as ext
    from audiomuse_amd.models.htsat import SwinBlock

    torch.manual_seed(10)
    blk = SwinBlock(C, 4, window=8, shift=0, mlp_ratio=4.0)
    blk = blk.to("cuda", torch.bfloat16).eval()
    x = torch.randn(2, BM, C, device="cuda", dtype=torch.bfloat16)
    attn_out = torch.randn(2, BM, C, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        got = blk._mlp_half(ext, x, attn_out)
        want = ext.mlp_fused(
            x, attn_out, blk.norm2.weight.contiguous(),
            blk.norm2.bias.contiguous(), blk.norm2.eps,
            blk.mlp[0].weight.contiguous(), blk.mlp[0].bias.contiguous(),
            blk.mlp[2].weight.contiguous(), blk.mlp[2].bias.contiguous())
    assert torch.equal(got, want)
