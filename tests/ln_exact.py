"""fp64 reference and half-ulp checkers for the LayerNorm kernel family
(ops/csrc/norms.hip) and its e4m3-emitting variants.

The kernels compute ((s - mean) * rsqrt(var + eps)) * w + b in fp32 from
bf16 inputs and round once, to bf16 or to OCP e4m3. A correct kernel is
therefore within half an output ulp of the exact value, plus what fp32
arithmetic can lose before the rounding. That loss is bounded per element
by 2^-16 * M (256 fp32 epsilons of the magnitude M below: room for the
reduction order and the hardware rsqrt), where

    M = (|xhat| + 2^-6 * (1 + max|s| / sigma)) * |w| + |b|

and the second term covers the cancellation in s - mean for rows that sit
on a large offset. tests/test_ln_exact_selftest.py shows that an fp32
emulation of the kernel passes both criteria and that planted faults fail.

Everything here runs on the CPU; GPU results are moved over as raw bytes.
"""

import functools

import torch

EPS = 1e-5
E4M3_MAX = 448.0
SLACK = 2.0 ** -16
SCALES = (8.0 / 448.0, 0.5 / 448.0, 64.0 / 448.0)
FAMILIES = ("normal", "offset", "wide", "constant")
# one per dispatch branch and edge of launch_layernorm_bf16_impl
DIMS = (4, 32, 64, 96, 128,        # two rows per wave: idle lanes, then full
        132, 192, 256,             # NIT=1
        384, 512,                  # NIT=2
        768, 1024,                 # NIT=4: 3 trips and 4
        1028, 2048,                # NIT=8
        2052, 4096)                # NIT=16


def rows_for(dim):
    """One row, and one more than a block holds (8 rows below 129, else 4):
    an odd half-wave / a one-row tail block."""
    return (1, 9) if dim <= 128 else (1, 5)


def draw(family, rows, dim, gen):
    """A (rows, dim) bf16 input of one of the four families."""
    n = torch.randn(rows, dim, generator=gen)
    if family == "normal":
        x = n
    elif family == "offset":
        x = 0.1 * n + 30.0
    elif family == "wide":
        x = 300.0 * n
    elif family == "constant":          # var == 0: the output is b
        x = (3.0 * torch.randn(rows, 1, generator=gen)).expand(rows, dim)
    else:
        raise ValueError(family)
    return x.to(torch.bfloat16).contiguous()


def ln_ref64(x, w, b, eps, other=None):
    """fp64 LayerNorm of bf16 inputs: (ref, M), or (ref, M, sum_out) with
    `other`. With `other` the normalised row is the unrounded fp32 sum
    x.float() + other.float(), as the kernel forms it, and sum_out is that
    sum rounded to bf16."""
    if other is None:
        s32 = x.float()
    else:
        s32 = x.float() + other.float()
    s = s32.double()
    mean = s.mean(-1, keepdim=True)
    var = (s - mean).square().mean(-1, keepdim=True)
    sigma = (var + eps).sqrt()
    xhat = (s - mean) / sigma
    wd, bd = w.double(), b.double()
    ref = xhat * wd + bd
    smax = s.abs().amax(-1, keepdim=True)
    M = (xhat.abs() + 2.0 ** -6 * (1.0 + smax / sigma)) * wd.abs() + bd.abs()
    if other is None:
        return ref, M
    return ref, M, s32.to(torch.bfloat16)


def _floor_log2(a):
    """floor(log2 a) for a > 0, exact (frexp, no transcendental)."""
    _, e = torch.frexp(a)
    return (e - 1).double()


def ulp_bf16(r):
    """2^(floor(log2|r|) - 7); 0 at r == 0."""
    a = r.double().abs()
    u = torch.exp2(_floor_log2(a.clamp(min=2.0 ** -126)) - 7.0)
    return torch.where(a > 0, u, torch.zeros_like(u))


def ulp_e4m3(t):
    """2^(floor(log2 max(|t|, 2^-6)) - 3): subnormal spacing below 2^-6."""
    a = t.double().abs().clamp(min=2.0 ** -6)
    return torch.exp2(_floor_log2(a) - 3.0)


def decode_e4m3(y8):
    """The bytes of an e4m3 tensor as fp64 on the CPU, with no GPU cast
    kernel between the bytes and the check."""
    return y8.view(torch.uint8).cpu().view(torch.float8_e4m3fn).double()


def bf16_excess(got, ref, M):
    """|got - ref| / (1/2 ulp_bf16(ref) + 2^-16 M); NaN counts as inf."""
    tol = 0.5 * ulp_bf16(ref) + SLACK * M
    ratio = (got.double().cpu() - ref).abs() / tol
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")),
                       ratio)


def e4m3_excess(got8, ref, M, scale):
    """The same ratio for e4m3 bytes quantised with `scale`."""
    t = (ref / scale).clamp(-E4M3_MAX, E4M3_MAX)
    tol = 0.5 * ulp_e4m3(t) + SLACK * M / scale
    ratio = (decode_e4m3(got8) - t).abs() / tol
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")),
                       ratio)


def _report(ratio, what):
    worst = ratio.max().item()
    if worst <= 1.0:
        return
    bad = int((ratio > 1.0).sum())
    idx = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
    raise AssertionError(
        f"{what}: {bad} of {ratio.numel()} elements outside 1/2 ulp + slack, "
        f"worst error/tolerance {worst:.3f} at {idx}")


def assert_bf16(got, ref, M, what="bf16 LayerNorm"):
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    _report(bf16_excess(got, ref, M), what)


def assert_e4m3(got8, ref, M, scale, what="e4m3 LayerNorm"):
    assert got8.dtype == torch.float8_e4m3fn and got8.shape == ref.shape
    _report(e4m3_excess(got8, ref, M, scale), what)


class Case:
    """Inputs of one (dim, rows, family) point and their fp64 references,
    all on the CPU. Built once (see case()); nothing here is modified."""

    def __init__(self, dim, rows, family):
        gen = torch.Generator().manual_seed(
            1000003 * dim + 101 * rows + FAMILIES.index(family))
        self.dim, self.rows, self.family = dim, rows, family
        self.x = draw(family, rows, dim, gen)
        self.other = draw(family, rows, dim, gen)
        self.w = torch.randn(dim, generator=gen).to(torch.bfloat16)
        self.b = torch.randn(dim, generator=gen).to(torch.bfloat16)
        self.ref, self.M = ln_ref64(self.x, self.w, self.b, EPS)
        self.add_ref, self.add_M, self.sum_out = ln_ref64(
            self.x, self.w, self.b, EPS, self.other)

    def __repr__(self):
        return f"dim={self.dim} rows={self.rows} {self.family}"


@functools.lru_cache(maxsize=None)
def case(dim, rows, family):
    return Case(dim, rows, family)


def cases(dim):
    return [case(dim, rows, fam) for rows in rows_for(dim) for fam in FAMILIES]


# -- fp32 emulation of the kernel's arithmetic (CPU) -------------------------

def emulate_f32(x, w, b, eps, other=None, divisor=None, use_eps=True):
    """The kernel's value before the final rounding, in float32:
    ((s - mean) * rsqrt(var + eps)) * w + b. `divisor` and `use_eps` plant
    faults for the self-test."""
    s = x.float() if other is None else x.float() + other.float()
    d = float(s.shape[-1] if divisor is None else divisor)
    mean = s.sum(-1, keepdim=True) / d
    diff = s - mean
    var = diff.square().sum(-1, keepdim=True) / d
    rstd = torch.rsqrt(var + eps if use_eps else var)
    return (diff * rstd) * w.float() + b.float()


def quantize_e4m3(f, scale, saturate=True):
    """The kernel's quantiser: multiply by 1/scale in fp32, clamp to +-448,
    round to nearest even. Without the clamp e4m3fn has no infinity, so
    values past 448 become NaN bytes."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(
        scale, dtype=torch.float32)
    q = f.float() * inv
    if saturate:
        q = q.clamp(-E4M3_MAX, E4M3_MAX)
    return q.to(torch.float8_e4m3fn)


def truncate_bf16(f):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    bits = f.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).to(torch.bfloat16)


def truncate_e4m3(f, scale):
    """Quantise toward zero: the e4m3 value of largest magnitude that does
    not exceed |f / scale|."""
    q = (f.double() / scale).clamp(-E4M3_MAX, E4M3_MAX)
    a = q.abs()
    step = ulp_e4m3(a)
    return (torch.sign(q) * torch.floor(a / step) * step).float().to(
        torch.float8_e4m3fn)
