"""window_attn_kernel block-id mappings (GPU): the flat XCD-grouped grid
runs the same code per (window, head) as the (windows, heads) grid, so the
two results must be torch.equal: no tolerance. Window counts cover one
window, a count that is no multiple of 8 (padding blocks return early),
and enough windows for several blocks per CU."""

import pytest
import torch

# (B, H, W): 1, 12, 48 and 2048 windows
GRIDS = [(1, 8, 8), (2, 16, 24), (3, 16, 64), (64, 16, 128)]
WIDTHS = [(128, 4), (256, 8), (512, 16)]


def _cases():
    for (B, H, W) in GRIDS:
        for (C, heads) in WIDTHS:
            # a shifted window needs more than one window along each axis
            for shift in ((0, 4) if min(H, W) > 8 else (0,)):
                yield pytest.param(B, H, W, C, heads, shift,
                                   id=f"b{B}-{H}x{W}-c{C}-s{shift}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C,heads,shift", list(_cases()))
def test_xcd_grid_equals_2d_grid(B, H, W, C, heads, shift):
    import audiomuse_amd._C as ext

    g = torch.Generator(device="cuda").manual_seed(1000 * B + C + shift)
    qkv = torch.randn(B, H, W, 3 * C, device="cuda", generator=g).to(
        torch.bfloat16)
    bias = (torch.randn(heads, 64, 64, device="cuda", generator=g) * 0.5).to(
        torch.bfloat16)
    scale = 32 ** -0.5

    want = ext.window_attn_fwd(qkv, bias, heads, shift, scale)
    assert torch.isfinite(want).all()
    if B * (H // 8) * (W // 8) == 2048:
        out = torch.full((B, H, W, C), 1e30, device="cuda",
                         dtype=torch.bfloat16)
        got = ext.window_attn_fwd(qkv, bias, heads, shift, scale, True, out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.isfinite(got).all()
    else:
        got = ext.window_attn_fwd(qkv, bias, heads, shift, scale, True)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_model_switch_selects_the_grid():
    """config.WINDOW_ATTN_XCD_GRID reaches the launch through SwinBlock and
    does not change a C = 256 block's output."""
    from audiomuse_amd import config
    from audiomuse_amd.models.htsat import SwinBlock

    torch.manual_seed(21)
    blk = SwinBlock(256, 8, window=8, shift=4, mlp_ratio=4.0)
    blk = blk.to("cuda", torch.bfloat16).eval()
    x = torch.randn(2, 16 * 24, 256, device="cuda", dtype=torch.bfloat16)
    saved = config.WINDOW_ATTN_XCD_GRID
    try:
        with torch.inference_mode():
            config.WINDOW_ATTN_XCD_GRID = True
            on = blk(x, 16, 24, None)
            config.WINDOW_ATTN_XCD_GRID = False
            off = blk(x, 16, 24, None)
    finally:
        config.WINDOW_ATTN_XCD_GRID = saved
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)
