"""One-launch patch embedding (ops/csrc/patch_embed.hip) against the fp32
evaluation of pad/crop -> 4x4 patchify -> linear from the same bf16 inputs,
and against the three-op path it replaces.

T = 37 (mostly padding, odd, no multiple of 4), 1001 (the CLAP clip: odd,
padded to 1024), 1024 (exact) and 1030 (cropped).
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from audiomuse_amd import config
from audiomuse_amd.ops import _ext

pytestmark = pytest.mark.gpu

B, N_MELS, N_FRAMES, C = 2, 128, 1024, 128
T_CASES = (37, 1001, 1024, 1030)


@functools.lru_cache(maxsize=None)
def _inputs(T: int):
    g = torch.Generator().manual_seed(77 + T)
    mel = (torch.randn(B, N_MELS, T, generator=g) * 2.0 - 4.0).to(
        torch.bfloat16)
    w = (torch.randn(C, 16, generator=g) * 0.25).to(torch.bfloat16)
    b = (torch.randn(C, generator=g) * 0.1).to(torch.bfloat16)
    return mel.cuda(), w.cuda(), b.cuda()


def _patches(mel: torch.Tensor) -> torch.Tensor:
    """pad/crop to N_FRAMES, then (B, H*W, 16) patches, as the encoder does."""
    T = mel.shape[-1]
    if T < N_FRAMES:
        mel = F.pad(mel, (0, N_FRAMES - T))
    elif T > N_FRAMES:
        mel = mel[..., :N_FRAMES]
    H, W = N_MELS // 4, N_FRAMES // 4
    return mel.view(B, H, 4, W, 4).permute(0, 1, 3, 2, 4).reshape(
        B, H * W, 16)


@functools.lru_cache(maxsize=None)
def _ref32(T: int) -> torch.Tensor:
    mel, w, b = _inputs(T)
    return F.linear(_patches(mel.float()), w.float(), b.float())


@pytest.mark.parametrize("T", T_CASES)
def test_fused_error_against_three_op(T):
    mel, w, b = _inputs(T)
    fused = _ext.require().patch_embed_bf16(mel, w, b, N_FRAMES)
    assert fused.shape == (B, (N_MELS // 4) * (N_FRAMES // 4), C)
    assert fused.dtype == torch.bfloat16
    three = F.linear(_patches(mel), w, b)
    ref = _ref32(T)
    ef = (fused.float() - ref).abs()
    e3 = (three.float() - ref).abs()
    print(f"T={T}: fused max/mean abs err {float(ef.max()):.4e}/"
          f"{float(ef.mean()):.4e}  three-op {float(e3.max()):.4e}/"
          f"{float(e3.mean()):.4e}")
    assert torch.isfinite(fused.float()).all()
    assert float(ef.max()) <= 1.5 * float(e3.max())
    assert float(ef.mean()) <= 1.5 * float(e3.mean())


@pytest.mark.parametrize("T", [37, 1001])
def test_padding_tokens_are_the_bias(T):
    mel, w, b = _inputs(T)
    fused = _ext.require().patch_embed_bf16(mel, w, b, N_FRAMES)
    W = N_FRAMES // 4
    first_pad = (T + 3) // 4          # first token column with no frame < T
    tok = fused.view(B, N_MELS // 4, W, C)[:, :, first_pad:, :]
    assert tok.shape[2] > 0
    assert torch.equal(tok, b.expand_as(tok))


def test_whole_encoder_embedding_error_vs_three_op_path():
    """Full HTSATConfig, B = 2: embedding max-abs error against the fp32
    eager forward, switch on, at most 1.25x the error with the switch off."""
    from audiomuse_amd.models.htsat import HTSATConfig, HTSATEncoder

    torch.manual_seed(4321)
    model = HTSATEncoder(HTSATConfig()).to("cuda", torch.bfloat16).eval()
    ref_model = copy.deepcopy(model).float()
    mel = (torch.randn(2, 128, 1001, device="cuda") * 2.0 - 4.0).to(
        torch.bfloat16)
    with torch.no_grad():
        ref = ref_model(mel.float())

    saved = config.PATCH_FUSED_ENABLE
    try:
        config.PATCH_FUSED_ENABLE = True
        with torch.inference_mode():
            new = model(mel).float()
        config.PATCH_FUSED_ENABLE = False
        with torch.inference_mode():
            old = model(mel).float()
    finally:
        config.PATCH_FUSED_ENABLE = saved

    err_new = float((new - ref).abs().max())
    err_old = float((old - ref).abs().max())
    print(f"embedding max-abs err vs fp32 eager: fused patch embed "
          f"{err_new:.5f}, three-op {err_old:.5f}, ref max-abs "
          f"{float(ref.abs().max()):.4f}")
    assert torch.isfinite(new).all()
    assert err_new <= 1.25 * err_old, (err_new, err_old)
