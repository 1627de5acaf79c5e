"""The checkers of tests/ln_exact.py, checked on the CPU.

An fp32 emulation of the LayerNorm kernels' arithmetic must pass the bf16
and e4m3 criteria on every input family, and every planted fault must
fail them. This is the evidence that the GPU tests of
tests/test_norms_exact.py can fail.
"""

import pytest
import torch

from tests import ln_exact as X

# every dispatch edge of the kernels plus sizes in between
SELF_DIMS = (4, 8, 32, 96, 128, 132, 256, 384, 768, 1024, 1028, 2052, 4096)
ROWS = 6


def _inputs(dim, family, seed=0):
    gen = torch.Generator().manual_seed(7919 * dim + X.FAMILIES.index(family)
                                        + seed)
    x = X.draw(family, ROWS, dim, gen)
    other = X.draw(family, ROWS, dim, gen)
    w = torch.randn(dim, generator=gen).to(torch.bfloat16)
    b = torch.randn(dim, generator=gen).to(torch.bfloat16)
    return x, other, w, b


@pytest.mark.parametrize("family", X.FAMILIES)
def test_fp32_emulation_passes_both_criteria(family):
    worst16 = worst8 = 0.0
    for dim in SELF_DIMS:
        x, other, w, b = _inputs(dim, family)
        for oth in (None, other):
            out = X.ln_ref64(x, w, b, X.EPS, oth)
            ref, M = out[0], out[1]
            f = X.emulate_f32(x, w, b, X.EPS, oth)
            X.assert_bf16(f.to(torch.bfloat16), ref, M, f"dim {dim}")
            worst16 = max(worst16, X.bf16_excess(f.to(torch.bfloat16), ref,
                                                 M).max().item())
            for scale in X.SCALES:
                q = X.quantize_e4m3(f, scale)
                X.assert_e4m3(q, ref, M, scale, f"dim {dim} scale {scale}")
                worst8 = max(worst8, X.e4m3_excess(q, ref, M,
                                                   scale).max().item())
            if oth is not None:
                assert torch.equal(out[2], (x.float() + other.float())
                                   .to(torch.bfloat16))
    print(f"{family}: worst error/tolerance bf16 {worst16:.3f} "
          f"e4m3 {worst8:.3f}")
    assert worst16 <= 1.0 and worst8 <= 1.0


def test_ulp_helpers_are_exact_at_binade_edges():
    r = torch.tensor([1.0, 1.9921875, 2.0, -0.5, 0.0, 3.0e-3], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0,
                         2.0 ** -16], dtype=torch.float64)
    assert torch.equal(X.ulp_bf16(r), want)
    t = torch.tensor([448.0, 256.0, 255.9, 1.0, 2.0 ** -6, 2.0 ** -7, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([32.0, 32.0, 16.0, 0.125, 2.0 ** -9, 2.0 ** -9,
                         2.0 ** -9], dtype=torch.float64)
    assert torch.equal(X.ulp_e4m3(t), want)
    # every e4m3 byte decodes to a multiple of its own ulp
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn)
    v = X.decode_e4m3(codes)
    v = v[~torch.isnan(v)]
    assert v.numel() == 254
    assert torch.equal(torch.round(v / X.ulp_e4m3(v)) * X.ulp_e4m3(v), v)


def _fails_bf16(got, ref, M):
    return X.bf16_excess(got, ref, M).max().item() > 1.0


def _fails_e4m3(got8, ref, M, scale):
    return X.e4m3_excess(got8, ref, M, scale).max().item() > 1.0


@pytest.mark.parametrize("dim,divisor", [(128, 129), (768, 769), (768, 1024),
                                         (96, 128), (2052, 4096)])
def test_wrong_divisor_fails(dim, divisor):
    """dim + 1, and the padded width of a partial trip."""
    for family in ("normal", "offset", "wide"):
        x, _, w, b = _inputs(dim, family)
        ref, M = X.ln_ref64(x, w, b, X.EPS)
        f = X.emulate_f32(x, w, b, X.EPS, divisor=divisor)
        assert _fails_bf16(f.to(torch.bfloat16), ref, M), family
        assert _fails_e4m3(X.quantize_e4m3(f, X.SCALES[0]), ref, M,
                           X.SCALES[0]), family


@pytest.mark.parametrize("dim", [64, 768])
def test_variance_without_eps_fails(dim):
    """var == 0 on a constant row: 0 * inf is NaN without eps."""
    x, _, w, b = _inputs(dim, "constant")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    f = X.emulate_f32(x, w, b, X.EPS, use_eps=False)
    assert _fails_bf16(f.to(torch.bfloat16), ref, M)
    assert _fails_e4m3(X.quantize_e4m3(f, X.SCALES[0]), ref, M, X.SCALES[0])
    # and on a low-variance row, where eps is a 1e-3 part of var + eps
    x, _, w, b = _inputs(dim, "offset")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    f = X.emulate_f32(x, w, b, X.EPS, use_eps=False)
    assert _fails_bf16(f.to(torch.bfloat16), ref, M)


@pytest.mark.parametrize("dim", [32, 132, 1028])
def test_bias_dropped_on_the_last_four_channels_fails(dim):
    x, _, w, b = _inputs(dim, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    b_bad = b.clone()
    b_bad[-4:] = 0
    f = X.emulate_f32(x, w, b_bad, X.EPS)
    assert _fails_bf16(f.to(torch.bfloat16), ref, M)
    assert _fails_e4m3(X.quantize_e4m3(f, X.SCALES[0]), ref, M, X.SCALES[0])


@pytest.mark.parametrize("dim", [4, 128, 768])
def test_two_bytes_swapped_in_one_pack_fails(dim):
    x, _, w, b = _inputs(dim, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    q = X.quantize_e4m3(X.emulate_f32(x, w, b, X.EPS), X.SCALES[0])
    raw = q.view(torch.uint8).clone()
    pack = dim - 4                      # the last 4-pack of row 0
    assert raw[0, pack + 1] != raw[0, pack + 2]
    raw[0, pack + 1], raw[0, pack + 2] = (raw[0, pack + 2].clone(),
                                          raw[0, pack + 1].clone())
    assert _fails_e4m3(raw.view(torch.float8_e4m3fn), ref, M, X.SCALES[0])


@pytest.mark.parametrize("factor", [1.07, 1 / 1.07])
def test_scale_off_by_seven_percent_fails(factor):
    x, _, w, b = _inputs(256, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    f = X.emulate_f32(x, w, b, X.EPS)
    for scale in X.SCALES:
        assert _fails_e4m3(X.quantize_e4m3(f, scale * factor), ref, M, scale)
    # a scale applied twice
    assert _fails_e4m3(X.quantize_e4m3(f, X.SCALES[0] ** 2), ref, M,
                       X.SCALES[0])


def test_missing_saturation_fails():
    """e4m3fn has no infinity: past +-448 an unclamped convert gives NaN."""
    x, _, w, b = _inputs(256, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    f = X.emulate_f32(x, w, b, X.EPS)
    scale = 0.5 / 448.0
    assert ((ref / scale).abs() > 480).any()
    q = X.quantize_e4m3(f, scale, saturate=False)
    assert torch.isnan(X.decode_e4m3(q)).any()
    assert _fails_e4m3(q, ref, M, scale)
    X.assert_e4m3(X.quantize_e4m3(f, scale), ref, M, scale)


@pytest.mark.parametrize("family", ["normal", "wide"])
def test_truncation_instead_of_rounding_fails(family):
    x, _, w, b = _inputs(512, family)
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    f = X.emulate_f32(x, w, b, X.EPS)
    assert _fails_bf16(X.truncate_bf16(f), ref, M)
    for scale in X.SCALES:
        assert _fails_e4m3(X.truncate_e4m3(f, scale), ref, M, scale)


def test_one_ulp_off_fails_almost_everywhere():
    x, _, w, b = _inputs(1024, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    good = X.emulate_f32(x, w, b, X.EPS).to(torch.bfloat16)
    up = (good.view(torch.int16) + 1).view(torch.bfloat16)
    assert (X.bf16_excess(up, ref, M) > 1.0).float().mean().item() > 0.95


def test_sum_from_rounded_operands_fails():
    """The add variant normalises the fp32 sum. Normalising the bf16 sum_out
    instead, or rounding sum_out toward zero, must both show."""
    x, other, w, b = _inputs(384, "wide")
    ref, M, sum_out = X.ln_ref64(x, w, b, X.EPS, other)
    s32 = x.float() + other.float()
    assert not torch.equal(sum_out.float(), s32)          # it does differ
    f = X.emulate_f32(sum_out, w, b, X.EPS)               # LN of the rounded
    assert _fails_bf16(f.to(torch.bfloat16), ref, M)
    assert _fails_e4m3(X.quantize_e4m3(f, X.SCALES[0]), ref, M, X.SCALES[0])
    assert not torch.equal(X.truncate_bf16(s32), sum_out)
    X.assert_bf16(X.emulate_f32(x, w, b, X.EPS, other).to(torch.bfloat16),
                  ref, M)


def test_nan_output_fails():
    x, _, w, b = _inputs(128, "normal")
    ref, M = X.ln_ref64(x, w, b, X.EPS)
    got = X.emulate_f32(x, w, b, X.EPS).to(torch.bfloat16)
    got[2, 5] = float("nan")
    with pytest.raises(AssertionError):
        X.assert_bf16(got, ref, M)


def test_byte_test_scales_do_what_they_are_there_for():
    """Inputs of the GPU byte tests: at 0.5/448 most of a row saturates,
    at 64/448 some outputs are e4m3 subnormals."""
    c = X.case(4096, 5, "normal")
    assert ((c.ref / X.SCALES[1]).abs() > 448).float().mean() > 0.5
    t = (c.ref / X.SCALES[2]).abs()
    assert ((t < 2.0 ** -6) & (t > 2.0 ** -10)).any()
