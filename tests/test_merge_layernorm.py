"""Patch-merging LayerNorm that gathers its 4C-wide rows from the four
source positions (GPU): bit-identical to LayerNorm over the regrouped
copy, and PatchMerging matches its eager fp32 result."""

import copy

import pytest
import torch

from audiomuse_amd.models.htsat import PatchMerging


def _regroup(x, B, H, W, C):
    x = x.view(B, H // 2, 2, W // 2, 2, C)
    return x.permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [128, 256, 512])
def test_gather_layernorm_equals_copy_plus_layernorm(C):
    import audiomuse_amd._C as ext

    torch.manual_seed(C)
    B, H, W = 2, 4, 6
    # every source position gets its own offset so a wrong gather order shows
    x = torch.randn(B, H, W, C, device="cuda") \
        + torch.arange(B * H * W, device="cuda").view(B, H, W, 1) * 0.05
    x = x.to(torch.bfloat16).contiguous()
    w = torch.randn(4 * C, device="cuda").to(torch.bfloat16)
    b = torch.randn(4 * C, device="cuda").to(torch.bfloat16)
    want = ext.layernorm_bf16(_regroup(x, B, H, W, C).contiguous(), w, b, 1e-5)
    got = ext.merge_layernorm_bf16(x, w, b, 1e-5)
    assert got.shape == want.shape
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_patch_merging_matches_eager_fp32():
    from audiomuse_amd import config

    assert config.MERGE_LN_GATHER
    torch.manual_seed(2)
    B, H, W, C = 2, 4, 6, 128
    pm32 = PatchMerging(C).to("cuda")
    with torch.no_grad():
        pm32.norm.weight.normal_(1.0, 0.3)
        pm32.norm.bias.normal_(0.0, 0.3)
    pm = copy.deepcopy(pm32).to(torch.bfloat16).eval()
    pm32 = copy.deepcopy(pm).float()     # same (bf16-rounded) weights
    x = torch.randn(B, H * W, C, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        assert pm._gather_available(x)
        got = pm(x, H, W)
    with torch.no_grad():
        want = pm32(x.float(), H, W)
    assert got.shape == (B, (H // 2) * (W // 2), 2 * C)
    # tolerance of tests/test_norms.py for the bf16 LayerNorm kernel
    torch.testing.assert_close(got.float(), want, rtol=2e-2, atol=2e-2)
