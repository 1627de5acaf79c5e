"""Whole-encoder check of the stage-2 changes (GPU): with the full
HTSATConfig at B = 2 (seed and input recipe of
test_encoder_traffic_model.py), the embedding error against an fp32 eager
forward of the same weights with the C = 256 one-launch MLP kernel and the
XCD-grouped attention grid on may be at most 1.25x the error with both
off."""

import copy

import pytest
import torch

from audiomuse_amd import config
from audiomuse_amd.models.htsat import HTSATConfig, HTSATEncoder

FLAGS = ("MLP_FUSED_C256_ENABLE", "WINDOW_ATTN_XCD_GRID")


@pytest.mark.gpu
def test_embedding_error_vs_flags_off():
    torch.manual_seed(4321)
    model = HTSATEncoder(HTSATConfig()).to("cuda", torch.bfloat16).eval()
    ref_model = copy.deepcopy(model).float()
    mel = (torch.randn(2, 128, 1001, device="cuda") * 2.0 - 4.0).to(
        torch.bfloat16)

    with torch.no_grad():
        ref = ref_model(mel.float())

    saved = {f: getattr(config, f) for f in FLAGS}
    try:
        for f in FLAGS:
            setattr(config, f, True)
        with torch.inference_mode():
            new = model(mel).float()
        for f in FLAGS:
            setattr(config, f, False)
        with torch.inference_mode():
            old = model(mel).float()
    finally:
        for f, v in saved.items():
            setattr(config, f, v)

    err_new = float((new - ref).abs().max())
    err_old = float((old - ref).abs().max())
    print(f"embedding max-abs err vs fp32 eager: flags on {err_new:.5f}, "
          f"flags off {err_old:.5f}, ref max-abs "
          f"{float(ref.abs().max()):.4f}")
    assert torch.isfinite(new).all()
    assert err_new <= 1.25 * err_old, (err_new, err_old)
