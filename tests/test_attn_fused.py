"""One-launch LayerNorm + QKV + window attention + proj kernel (GPU,
C = 128, 4 heads, window 8).

Reference: fp32 torch evaluation of
    LN -> qkv -> scale * q k^T + rel_bias + shift mask -> softmax -> P v -> proj
from the same bf16 inputs. The four-launch path (layernorm_bf16 ->
linear_bias -> window_attn_fwd -> linear_bias) has the same rounding points
(LN out, qkv, P, O and proj are bf16, accumulation fp32) and differs only in
summation order, so the fused kernel's max-abs and mean-abs errors must stay
within 1.5x of the four-launch path's; anything beyond that is a layout or
indexing bug.
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

C = 128
HEADS = 4
WIN = 8
EPS = 1e-5
SCALE = 32 ** -0.5


def _inputs(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    M = B * H * W
    # rows with different means and scales
    row_scale = torch.linspace(0.3, 2.0, M, device="cuda")[:, None]
    row_mean = torch.linspace(-1.0, 1.5, M, device="cuda")[:, None]
    x = (rn(M, C) * row_scale + row_mean).view(B, H, W, C).to(torch.bfloat16)
    ln_w = (1.0 + 0.3 * rn(C)).to(torch.bfloat16)
    ln_b = (0.2 * rn(C)).to(torch.bfloat16)
    # asymmetric weights: column- and row-dependent scale, so a swapped head,
    # a q/k/v mix-up or a transpose changes the result
    qkv_w = (rn(3 * C, C) * C ** -0.5
             * torch.linspace(0.5, 1.5, C, device="cuda")[None, :]
             * torch.linspace(0.6, 1.6, 3 * C, device="cuda")[:, None]
             ).to(torch.bfloat16)
    qkv_b = (0.3 * rn(3 * C)).to(torch.bfloat16)
    proj_w = (rn(C, C) * C ** -0.5
              * torch.linspace(0.5, 1.5, C, device="cuda")[None, :]
              * torch.linspace(1.3, 0.7, C, device="cuda")[:, None]
              ).to(torch.bfloat16)
    proj_b = (0.3 * rn(C)).to(torch.bfloat16)
    rel_bias = (0.5 * rn(HEADS, WIN * WIN, WIN * WIN)).to(torch.bfloat16)
    return [t.contiguous() for t in
            (x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, rel_bias)]


def _fp32_reference(x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, rel_bias,
                    shift):
    from audiomuse_amd.models.htsat import (_shift_mask, window_partition,
                                            window_reverse)
    B, H, W, _ = x.shape
    T = WIN * WIN
    xn = F.layer_norm(x.float(), (C,), ln_w.float(), ln_b.float(), EPS)
    if shift:
        xn = torch.roll(xn, shifts=(-shift, -shift), dims=(1, 2))
    win = window_partition(xn, WIN)                       # (nW, T, C)
    nW = win.shape[0]
    qkv = win @ qkv_w.float().t() + qkv_b.float()
    qkv = qkv.view(nW, T, 3, HEADS, C // HEADS)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)        # (nW, h, T, d)
    s = (q @ k.transpose(-1, -2)) * SCALE + rel_bias.float()[None]
    if shift:
        mask = _shift_mask(H, W, WIN, shift, x.device)    # (groups, T, T)
        groups = mask.shape[0]
        s = (s.view(nW // groups, groups, HEADS, T, T)
             + mask[None, :, None]).view(nW, HEADS, T, T)
    o = torch.softmax(s, dim=-1) @ v
    o = o.transpose(1, 2).reshape(nW, T, C)
    o = window_reverse(o, WIN, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o @ proj_w.float().t() + proj_b.float()


def _four_launch(ext, x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, rel_bias,
                 shift):
    B, H, W, _ = x.shape
    xn = ext.layernorm_bf16(x.view(B, H * W, C), ln_w, ln_b, EPS)
    qkv = ext.linear_bias(xn, qkv_w, qkv_b)
    o = ext.window_attn_fwd(qkv.view(B, H, W, 3 * C), rel_bias, HEADS, shift,
                            SCALE)
    return ext.linear_bias(o.view(B, H * W, C), proj_w, proj_b).view(
        B, H, W, C)


def _fused(ext, x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, rel_bias, shift,
           out=None):
    return ext.attn_block_fused(x, ln_w, ln_b, EPS, qkv_w, qkv_b, proj_w,
                                proj_b, rel_bias, shift, SCALE, out=out)


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    return tuple(_inputs(B, H, W, seed=101 + B * H * W))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,shift", [((1, 8, 8), 0), ((2, 16, 24), 0),
                                         ((2, 16, 24), 4)])
def test_fused_error_within_four_launch_path(shape, shift):
    import audiomuse_amd._C as ext

    args = _case(*shape)
    ref = _fp32_reference(*args, shift)
    four = _four_launch(ext, *args, shift).float()
    fused = _fused(ext, *args, shift).float()

    e4 = (four - ref).abs()
    ef = (fused - ref).abs()
    print(f"{shape} shift {shift}: four-launch max {float(e4.max()):.5f} "
          f"mean {float(e4.mean()):.6f}; fused max {float(ef.max()):.5f} "
          f"mean {float(ef.mean()):.6f}; ref mean-abs "
          f"{float(ref.abs().mean()):.4f}")
    assert fused.shape == ref.shape
    assert torch.isfinite(fused).all()
    assert float(ef.max()) <= 1.5 * float(e4.max()), \
        f"fused max-abs {float(ef.max()):.5f} vs four-launch {float(e4.max()):.5f}"
    assert float(ef.mean()) <= 1.5 * float(e4.mean()), \
        f"fused mean-abs {float(ef.mean()):.6f} vs four-launch {float(e4.mean()):.6f}"


@pytest.mark.gpu
def test_every_element_written_more_windows_than_resident():
    """1024 windows, shift 4: the result must not depend on what the
    destination held before, and must stay within the error bound."""
    import audiomuse_amd._C as ext

    shape, shift = (8, 32, 256), 4
    args = _case(*shape)
    x = args[0]
    out_nan = torch.full_like(x, float("nan"))
    out_big = torch.full_like(x, 1e30)
    r1 = _fused(ext, *args, shift, out=out_nan)
    r2 = _fused(ext, *args, shift, out=out_big)
    assert r1.data_ptr() == out_nan.data_ptr()
    assert torch.isfinite(r1).all() and torch.isfinite(r2).all()
    assert torch.equal(r1, r2)

    ref = _fp32_reference(*args, shift)
    four = _four_launch(ext, *args, shift).float()
    e4 = (four - ref).abs()
    ef = (r1.float() - ref).abs()
    print(f"{shape} shift {shift}: four-launch max {float(e4.max()):.5f} "
          f"mean {float(e4.mean()):.6f}; fused max {float(ef.max()):.5f} "
          f"mean {float(ef.mean()):.6f}")
    assert float(ef.max()) <= 1.5 * float(e4.max())
    assert float(ef.mean()) <= 1.5 * float(e4.mean())


@pytest.mark.gpu
def test_binding_rejects_unsupported_inputs():
    import audiomuse_amd._C as ext

    x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, rel_bias = _case(1, 8, 8)

    def z(*shape):
        return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)

    # C = 256
    with pytest.raises(RuntimeError):
        ext.attn_block_fused(z(1, 8, 8, 256), z(256), z(256), EPS,
                             z(768, 256), z(768), z(256, 256), z(256),
                             z(8, 64, 64), 0, SCALE)
    # H = 12
    with pytest.raises(RuntimeError):
        ext.attn_block_fused(z(1, 12, 8, C), ln_w, ln_b, EPS, qkv_w, qkv_b,
                             proj_w, proj_b, rel_bias, 0, SCALE)
    # wrong-shaped out
    with pytest.raises(RuntimeError):
        ext.attn_block_fused(x, ln_w, ln_b, EPS, qkv_w, qkv_b, proj_w, proj_b,
                             rel_bias, 0, SCALE, out=z(1, 8, 16, C))
    # shift outside {0, 4}
    with pytest.raises(RuntimeError):
        ext.attn_block_fused(x, ln_w, ln_b, EPS, qkv_w, qkv_b, proj_w, proj_b,
                             rel_bias, 2, SCALE)


def _block(dim, heads, shift, seed):
    from audiomuse_amd.models.htsat import SwinBlock

    torch.manual_seed(seed)
    blk = SwinBlock(dim, heads, window=WIN, shift=shift, mlp_ratio=4.0)
    with torch.no_grad():
        # defaults (LN weight 1 / bias 0, rel_bias std 0.02) would hide a
        # dropped LN parameter or a wrong bias index
        blk.norm1.weight.add_(0.3 * torch.randn(dim))
        blk.norm1.bias.add_(0.2 * torch.randn(dim))
        blk.attn.rel_bias.copy_(0.5 * torch.randn_like(blk.attn.rel_bias))
    return blk.to("cuda", torch.bfloat16).eval()


def _four_launch_block(ext, blk, x, H, W):
    B, L, Cd = x.shape
    xn = blk.norm1(x)
    qkv = ext.linear_bias(xn.contiguous(), blk.attn.qkv.weight.contiguous(),
                          blk.attn.qkv.bias.contiguous())
    o = ext.window_attn_fwd(qkv.view(B, H, W, 3 * Cd),
                            blk.attn.full_bias_bf16(), blk.attn.heads,
                            blk.shift, blk.attn.scale)
    proj = ext.linear_bias(o.view(B, L, Cd).contiguous(),
                           blk.attn.proj.weight.contiguous(),
                           blk.attn.proj.bias.contiguous())
    return blk._mlp_half(ext, x, proj)


@pytest.mark.gpu
def test_model_dispatch_stage1_block():
    import audiomuse_amd._C as ext
    from audiomuse_amd import config

    assert config.ATTN_FUSED_ENABLE
    B, H, W = 2, 16, 24
    blk = _block(C, HEADS, shift=4, seed=11)
    x = torch.randn(B, H * W, C, device="cuda", dtype=torch.bfloat16)
    saved = config.ATTN_FUSED_ENABLE
    try:
        with torch.inference_mode():
            got = blk(x, H, W, None)
            proj = ext.attn_block_fused(
                x.view(B, H, W, C), blk.norm1.weight.contiguous(),
                blk.norm1.bias.contiguous(), blk.norm1.eps,
                blk.attn.qkv.weight.contiguous(),
                blk.attn.qkv.bias.contiguous(),
                blk.attn.proj.weight.contiguous(),
                blk.attn.proj.bias.contiguous(), blk.attn.full_bias_bf16(),
                blk.shift, blk.attn.scale)
            want = blk._mlp_half(ext, x, proj.view(B, H * W, C))
            assert torch.equal(got, want)

            config.ATTN_FUSED_ENABLE = False
            got_off = blk(x, H, W, None)
            want_off = _four_launch_block(ext, blk, x, H, W)
            assert torch.equal(got_off, want_off)
    finally:
        config.ATTN_FUSED_ENABLE = saved
    assert torch.isfinite(got).all()


@pytest.mark.gpu
def test_model_dispatch_leaves_c256_block_alone():
    import audiomuse_amd._C as ext
    from audiomuse_amd import config

    B, H, W = 2, 16, 24
    blk = _block(256, 8, shift=4, seed=12)
    x = torch.randn(B, H * W, 256, device="cuda", dtype=torch.bfloat16)
    saved = config.ATTN_FUSED_ENABLE
    try:
        with torch.inference_mode():
            on = blk(x, H, W, None)
            config.ATTN_FUSED_ENABLE = False
            off = blk(x, H, W, None)
            want = _four_launch_block(ext, blk, x, H, W)
    finally:
        config.ATTN_FUSED_ENABLE = saved
    assert torch.equal(on, off)
    assert torch.equal(on, want)


@pytest.mark.gpu
def test_whole_encoder_embedding_error_vs_four_launch_path():
    """Full HTSATConfig, B = 2: embedding max-abs error against the fp32
    eager forward, flag on, at most 1.25x the error with the flag off."""
    from audiomuse_amd import config
    from audiomuse_amd.models.htsat import HTSATConfig, HTSATEncoder

    torch.manual_seed(4321)
    model = HTSATEncoder(HTSATConfig()).to("cuda", torch.bfloat16).eval()
    ref_model = copy.deepcopy(model).float()
    mel = (torch.randn(2, 128, 1001, device="cuda") * 2.0 - 4.0).to(
        torch.bfloat16)
    with torch.no_grad():
        ref = ref_model(mel.float())

    saved = config.ATTN_FUSED_ENABLE
    try:
        config.ATTN_FUSED_ENABLE = True
        with torch.inference_mode():
            new = model(mel).float()
        config.ATTN_FUSED_ENABLE = False
        with torch.inference_mode():
            old = model(mel).float()
    finally:
        config.ATTN_FUSED_ENABLE = saved

    err_new = float((new - ref).abs().max())
    err_old = float((old - ref).abs().max())
    print(f"embedding max-abs err vs fp32 eager: fused attention half "
          f"{err_new:.5f}, four-launch {err_old:.5f}, ref max-abs "
          f"{float(ref.abs().max()):.4f}")
    assert torch.isfinite(new).all()
    assert err_new <= 1.25 * err_old, (err_new, err_old)
