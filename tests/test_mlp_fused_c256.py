"""One-launch residual add + LayerNorm + MLP kernel at C = 256 (GPU).

Reference: fp32 torch evaluation of
    x2 = x + proj;  out = x2 + W2 . gelu_tanh(W1 . LN(x2) + b1) + b2
from the same bf16 inputs. The three-op path (add_layernorm_bf16 ->
linear_gelu -> linear_bias_add) has the same rounding points and differs
only in summation order, so the fused kernel's max-abs and mean-abs
errors must stay within 1.5x of the three-op path's on the same inputs.
Inputs are built as in test_mlp_fused.py: rows with different means and
scales, weights with row- and column-dependent scale, so that a transposed
or permuted layout cannot pass.
"""

import pytest
import torch
import torch.nn.functional as F

BM = 128
C = 256
HID = 1024
EPS = 1e-5


def _inputs(M, seed, C=C, HID=HID):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    row_scale = torch.linspace(0.3, 2.0, M, device="cuda")[:, None]
    row_mean = torch.linspace(-1.0, 1.5, M, device="cuda")[:, None]
    x = (rn(M, C) * row_scale + row_mean).to(torch.bfloat16)
    proj = (rn(M, C) * 0.5 + 0.1).to(torch.bfloat16)
    ln_w = (1.0 + 0.3 * rn(C)).to(torch.bfloat16)
    ln_b = (0.2 * rn(C)).to(torch.bfloat16)
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
    xn = F.layer_norm(x2, (x.shape[-1],), ln_w.float(), ln_b.float(), EPS)
    h = F.gelu(xn @ w1.float().t() + b1.float(), approximate="tanh")
    return x2 + h @ w2.float().t() + b2.float()


def _three_op(ext, x, proj, ln_w, ln_b, w1, b1, w2, b2):
    x2, xn2 = ext.add_layernorm_bf16(x, proj, ln_w, ln_b, EPS)
    hidden = ext.linear_gelu(xn2, w1, b1)
    return ext.linear_bias_add(hidden, w2, b2, x2)


def _fused(ext, args, out=None):
    x, proj, ln_w, ln_b, w1, b1, w2, b2 = args
    return ext.mlp_fused(x, proj, ln_w, ln_b, EPS, w1, b1, w2, b2, out)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [BM, 3 * BM, 512 * BM])
def test_fused_mlp_error_within_three_op_path(M):
    import audiomuse_amd._C as ext

    args = _inputs(M, seed=29 + M)
    ref = _fp32_reference(*args)
    three = _three_op(ext, *args).float()
    fused_bf16 = _fused(ext, args)
    fused = fused_bf16.float()

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

    if M == 512 * BM:
        # more than one workgroup per CU in turn: what the buffer held
        # before must not show in the result
        a = _fused(ext, args, torch.full_like(fused_bf16, float("nan")))
        b = _fused(ext, args, torch.full_like(fused_bf16, 1e30))
        assert torch.equal(a, b)
        assert torch.equal(a, fused_bf16)


@pytest.mark.gpu
def test_binding_rejects_partial_tile():
    import audiomuse_amd._C as ext

    args = _inputs(BM + BM // 2, seed=3)
    with pytest.raises(RuntimeError):
        _fused(ext, args)


@pytest.mark.gpu
def test_binding_rejects_other_widths():
    import audiomuse_amd._C as ext

    args = _inputs(BM, seed=4, C=512, HID=2048)
    with pytest.raises(RuntimeError):
        _fused(ext, args)


@pytest.mark.gpu
def test_binding_rejects_wrong_shaped_out():
    import audiomuse_amd._C as ext

    args = _inputs(BM, seed=5)
    for bad in (torch.empty(2 * BM, C, device="cuda", dtype=torch.bfloat16),
                torch.empty(BM, C, device="cuda", dtype=torch.float32),
                torch.empty(C, BM, device="cuda", dtype=torch.bfloat16).t()):
        with pytest.raises(RuntimeError):
            _fused(ext, args, bad)
    out = torch.empty(BM, C, device="cuda", dtype=torch.bfloat16)
    got = _fused(ext, args, out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, _fused(ext, args))


@pytest.mark.gpu
def test_c128_call_unchanged():
    """The C = 128 kernel through the widened binding: positional call as
    before, same partial-tile error, and out= returns the same values."""
    import audiomuse_amd._C as ext

    args = _inputs(2 * 128, seed=6, C=128, HID=512)
    x, proj, ln_w, ln_b, w1, b1, w2, b2 = args
    got = ext.mlp_fused(x, proj, ln_w, ln_b, EPS, w1, b1, w2, b2)
    ref = _fp32_reference(*args)
    three = _three_op(ext, *args).float()
    assert float((got.float() - ref).abs().max()) <= \
        1.5 * float((three - ref).abs().max())
    out = torch.full_like(got, float("nan"))
    assert torch.equal(_fused(ext, args, out), got)
    with pytest.raises(RuntimeError):
        _fused(ext, _inputs(128 + 64, seed=7, C=128, HID=512))


def _block():
    from audiomuse_amd.models.htsat import SwinBlock

    torch.manual_seed(12)
    blk = SwinBlock(C, 8, window=8, shift=0, mlp_ratio=4.0)
    return blk.to("cuda", torch.bfloat16).eval()


def _block_three_op(ext, blk, x, attn_out):
    return _three_op(
        ext, x, attn_out,
        blk.norm2.weight.contiguous(), blk.norm2.bias.contiguous(),
        blk.mlp[0].weight.contiguous(), blk.mlp[0].bias.contiguous(),
        blk.mlp[2].weight.contiguous(), blk.mlp[2].bias.contiguous())


@pytest.mark.gpu
def test_model_dispatch_at_c256():
    import audiomuse_amd._C as ext
    from audiomuse_amd import config

    assert config.MLP_FUSED_ENABLE and config.MLP_FUSED_C256_ENABLE
    blk = _block()
    g = torch.Generator(device="cuda").manual_seed(13)

    def pair(M):
        return (torch.randn(1, M, C, device="cuda", generator=g).to(
                    torch.bfloat16),
                torch.randn(1, M, C, device="cuda", generator=g).to(
                    torch.bfloat16))

    with torch.inference_mode():
        # tile multiple: the one-launch kernel
        x, a = pair(2 * BM)
        want = ext.mlp_fused(
            x, a, blk.norm2.weight.contiguous(), blk.norm2.bias.contiguous(),
            blk.norm2.eps,
            blk.mlp[0].weight.contiguous(), blk.mlp[0].bias.contiguous(),
            blk.mlp[2].weight.contiguous(), blk.mlp[2].bias.contiguous())
        assert torch.equal(blk._mlp_half(ext, x, a), want)
        # flag off: the three-op path, bit for bit
        saved = config.MLP_FUSED_C256_ENABLE
        try:
            config.MLP_FUSED_C256_ENABLE = False
            got_off = blk._mlp_half(ext, x, a)
        finally:
            config.MLP_FUSED_C256_ENABLE = saved
        assert torch.equal(got_off, _block_three_op(ext, blk, x, a))
        # MLP_FUSED_ENABLE off switches the C = 256 kernel off with it
        saved = config.MLP_FUSED_ENABLE
        try:
            config.MLP_FUSED_ENABLE = False
            got_off = blk._mlp_half(ext, x, a)
        finally:
            config.MLP_FUSED_ENABLE = saved
        assert torch.equal(got_off, _block_three_op(ext, blk, x, a))
        # not a tile multiple: the three-op path, bit for bit
        x, a = pair(BM + BM // 2)
        assert torch.equal(blk._mlp_half(ext, x, a),
                           _block_three_op(ext, blk, x, a))
