"""The LayerNorm kernel family (ops/csrc/norms.hip) against fp64, to half
an output ulp plus a derived fp32 slack (tests/ln_exact.py), at one dim per
dispatch branch and edge, with row tails, for the bf16 and the e4m3
outputs; the sampled amax of the e4m3 variants; the delayed-scale chain of
ops/fp8.py on top of them; and the argument checks of the bindings."""

import pytest
import torch

from tests import ln_exact as X

pytestmark = pytest.mark.gpu


def _ext():
    import audiomuse_amd._C as ext
    return ext


def _dev(t):
    return t.to("cuda")


def _scale(v):
    return torch.full((), v, dtype=torch.float32, device="cuda")


# -- bf16 outputs -------------------------------------------------------------

@pytest.mark.parametrize("dim", X.DIMS)
def test_layernorm_bf16_within_half_ulp_of_fp64(dim):
    ext = _ext()
    for c in X.cases(dim):
        got = ext.layernorm_bf16(_dev(c.x), _dev(c.w), _dev(c.b), X.EPS)
        X.assert_bf16(got.cpu(), c.ref, c.M, f"layernorm_bf16 {c}")


@pytest.mark.parametrize("dim", X.DIMS)
def test_add_layernorm_bf16_within_half_ulp_of_fp64(dim):
    ext = _ext()
    for c in X.cases(dim):
        s, y = ext.add_layernorm_bf16(_dev(c.x), _dev(c.other), _dev(c.w),
                                      _dev(c.b), X.EPS)
        assert torch.equal(s.cpu(), c.sum_out), f"sum_out {c}"
        X.assert_bf16(y.cpu(), c.add_ref, c.add_M, f"add_layernorm_bf16 {c}")


def _regroup(x, B, H, W, C):
    x = x.view(B, H // 2, 2, W // 2, 2, C)
    return x.permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 4, 6)])
@pytest.mark.parametrize("C", [36, 96, 128, 512, 1024])
def test_merge_layernorm_bf16_within_half_ulp_of_fp64(C, shape):
    ext = _ext()
    B, H, W = shape
    gen = torch.Generator().manual_seed(C * 31 + B)
    # every source position gets its own offset so a wrong gather order shows
    x = torch.randn(B, H, W, C, generator=gen) \
        + torch.arange(B * H * W).view(B, H, W, 1) * 0.05
    x = x.to(torch.bfloat16).contiguous()
    w = torch.randn(4 * C, generator=gen).to(torch.bfloat16)
    b = torch.randn(4 * C, generator=gen).to(torch.bfloat16)
    ref, M = X.ln_ref64(_regroup(x, B, H, W, C), w, b, X.EPS)
    got = ext.merge_layernorm_bf16(_dev(x), _dev(w), _dev(b), X.EPS)
    assert got.shape == ref.shape
    X.assert_bf16(got.cpu(), ref, M, f"merge_layernorm_bf16 C={C} {shape}")


# -- e4m3 outputs -------------------------------------------------------------

@pytest.mark.parametrize("dim", X.DIMS)
def test_layernorm_bf16_fp8_bytes_within_half_ulp_of_fp64(dim):
    ext = _ext()
    for c in X.cases(dim):
        x, w, b = _dev(c.x), _dev(c.w), _dev(c.b)
        for scale in X.SCALES:
            amax = torch.zeros(256, device="cuda")
            y8 = ext.layernorm_bf16_fp8(x, w, b, X.EPS, _scale(scale), amax)
            X.assert_e4m3(y8, c.ref, c.M, scale,
                          f"layernorm_bf16_fp8 {c} scale {scale * 448}/448")


@pytest.mark.parametrize("dim", X.DIMS)
def test_add_layernorm_bf16_fp8_bytes_within_half_ulp_of_fp64(dim):
    ext = _ext()
    for c in X.cases(dim):
        x, o, w, b = _dev(c.x), _dev(c.other), _dev(c.w), _dev(c.b)
        for scale in X.SCALES:
            amax = torch.zeros(256, device="cuda")
            s, y8 = ext.add_layernorm_bf16_fp8(x, o, w, b, X.EPS,
                                               _scale(scale), amax)
            assert torch.equal(s.cpu(), c.sum_out), f"sum_out {c}"
            X.assert_e4m3(y8, c.add_ref, c.add_M, scale,
                          f"add_layernorm_bf16_fp8 {c} scale {scale * 448}/448")


# -- the sampled amax ---------------------------------------------------------

def _amax_inputs(rows, dim, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=gen)
    other = torch.randn(rows, dim, generator=gen)
    w = torch.randn(dim, generator=gen)
    b = 0.1 * torch.randn(dim, generator=gen)
    # block 0's largest |f| is a negative one: a channel with a clearly
    # positive gain is pushed far below its row's mean
    j = int(w.argmax())
    x[0, j] = -60.0
    other[0, j] = -60.0
    return tuple(t.to(torch.bfloat16).contiguous() for t in (x, other, w, b))


def _run_amax(ext, add, x, other, w, b, amax):
    sc = _scale(8.0 / 448.0)
    if add:
        ext.add_layernorm_bf16_fp8(_dev(x), _dev(other), _dev(w), _dev(b),
                                   X.EPS, sc, amax)
    else:
        ext.layernorm_bf16_fp8(_dev(x), _dev(w), _dev(b), X.EPS, sc, amax)
    return amax.cpu().double()


def _check_amax_contract(ext, add, rows, dim, rows_per_block):
    x, other, w, b = _amax_inputs(rows, dim, 5 * rows + dim + add)
    ref, M = X.ln_ref64(x, w, b, X.EPS, other if add else None)[:2]
    f = ref.abs()
    slack = (X.SLACK * M).max().item()
    blk0 = ref[:rows_per_block]
    top = blk0.flatten()[blk0.abs().argmax()].item()
    assert top < 0, "input sanity: block 0's largest |f| must be negative"
    blk0_max = abs(top)

    got = _run_amax(ext, add, x, other, w, b, torch.zeros(256, device="cuda"))
    # never an overestimate
    assert got.max().item() <= f.max().item() + slack
    # block 0 is always sampled, and its negative peak counts by magnitude
    assert got.max().item() >= blk0_max - slack
    assert got[0].item() >= blk0_max - slack
    # slot by slot: every 64th block is sampled into slot (block & 255), so a
    # slot holds the largest |f| over the rows of its blocks, within the
    # slack of those rows alone, and every other slot stays 0. A recorded
    # value is thereby some element's |f|, in the right slot.
    n_blocks = (rows + rows_per_block - 1) // rows_per_block
    want = torch.zeros(256, dtype=torch.float64)
    room = torch.zeros(256, dtype=torch.float64)
    for blk in range(0, n_blocks, 64):
        sl = slice(blk * rows_per_block, (blk + 1) * rows_per_block)
        want[blk & 255] = max(want[blk & 255].item(), f[sl].max().item())
        room[blk & 255] = max(room[blk & 255].item(),
                              (X.SLACK * M[sl]).max().item())
    assert ((got - want).abs() <= room).all(), (got - want).abs().max().item()
    assert not got[want == 0].any()

    # accumulation is by maximum: a larger value stands ...
    big = 2.0 * f.max().item() + 1.0
    kept = _run_amax(ext, add, x, other, w, b,
                     torch.full((256,), big, device="cuda"))
    assert torch.equal(kept, torch.full((256,), big, dtype=torch.float64)
                       .float().double())
    # ... and a smaller one is raised to this call's value
    half = (0.5 * got).float().cuda()
    raised = _run_amax(ext, add, x, other, w, b, half)
    assert torch.equal(raised, got)
    return got


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("rows,dim,rpb", [(2051, 128, 8), (1025, 256, 4)])
def test_fp8_amax_contract_with_a_reused_slot(add, rows, dim, rpb):
    """257 blocks: blocks 0, 64, 128, 192 and 256 are sampled and block 256
    shares slot 0 with block 0."""
    got = _check_amax_contract(_ext(), add, rows, dim, rpb)
    assert int((got > 0).sum()) >= 2          # several sampled blocks


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("dim", [32, 64, 96, 128])
def test_fp8_amax_block0_with_idle_lanes(add, dim):
    """dim < 128 leaves the upper lanes of each 32-lane half idle; they
    take part in the amax reduction with 0."""
    for rows in (1, 5, 8):
        _check_amax_contract(_ext(), add, rows, dim, 8)


# -- the delayed-scale chain of ops/fp8.py ------------------------------------

def _chain_norm():
    from audiomuse_amd.ops.norms import FusedLayerNorm

    torch.manual_seed(11)
    norm = FusedLayerNorm(128).to("cuda", torch.bfloat16)
    with torch.no_grad():
        norm.weight.normal_(1.0, 0.5)
        norm.bias.normal_(0.0, 0.5)
    return norm


@pytest.mark.parametrize("add", [False, True])
def test_fp8_chain_scale_follows_the_recorded_amax(add):
    from audiomuse_amd.ops import fp8

    ext = _ext()
    norm = _chain_norm()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(3, 40, 128, generator=gen).to(torch.bfloat16)
    other = torch.randn(3, 40, 128, generator=gen).to(torch.bfloat16)

    def call():
        with torch.inference_mode():
            if add:
                s, y8, scale = fp8.add_ln_fp8(norm, _dev(x), _dev(other))
                assert torch.equal(s.cpu(), sum_out)
                return y8, scale
            return fp8.ln_fp8(norm, _dev(x))

    def reference():
        out = X.ln_ref64(x, norm.weight.detach().cpu(),
                         norm.bias.detach().cpu(), norm.eps,
                         other if add else None)
        return out

    out = reference()
    ref, M = out[0], out[1]
    sum_out = out[2] if add else None
    y8, scale = call()
    init = torch.tensor(8.0 / 448.0, dtype=torch.float32).item()
    assert scale.item() == init
    X.assert_e4m3(y8, ref, M, init, "first call, init scale")
    _, amax = fp8._weak_get(fp8._ln_state, norm)[0][:2]
    amax1 = amax.clone()
    assert amax1.max().item() > 0
    assert amax1.max().item() <= ref.abs().max().item() + (X.SLACK * M).max().item()

    # a quarter of the gain: the second call must record a smaller amax,
    # which it can only do if the state was zeroed before the kernel ran
    with torch.no_grad():
        norm.weight.mul_(0.25)
        norm.bias.mul_(0.25)
    out = reference()
    ref, M = out[0], out[1]
    y8, scale2 = call()
    assert scale2 is scale
    want = ((amax1.max().clamp(min=1e-6) * 1.05) / 448.0).item()
    assert scale.item() == want
    X.assert_e4m3(y8, ref, M, want, "second call, delayed scale")
    fresh = torch.zeros(256, device="cuda")
    args = [_dev(x)] + ([_dev(other)] if add else []) + [
        norm.weight.detach().contiguous(), norm.bias.detach().contiguous(),
        norm.eps, scale, fresh]
    (ext.add_layernorm_bf16_fp8 if add else ext.layernorm_bf16_fp8)(*args)
    assert torch.equal(amax, fresh)
    assert 0 < amax.max().item() < 0.5 * amax1.max().item()


# -- argument checks of the bindings ------------------------------------------

def _half_strided(t):
    return t.repeat(2)[::2]              # same values, not contiguous


def test_layernorm_bindings_reject_bad_arguments():
    """Every call below is refused by a check that stands before the launch
    in bindings.cpp; the good calls at the end still run."""
    ext = _ext()
    dim = 128

    def args():
        return {"x": torch.randn(5, dim, device="cuda", dtype=torch.bfloat16),
                "other": torch.randn(5, dim, device="cuda",
                                     dtype=torch.bfloat16),
                "w": torch.ones(dim, device="cuda", dtype=torch.bfloat16),
                "b": torch.zeros(dim, device="cuda", dtype=torch.bfloat16),
                "scale": _scale(8.0 / 448.0),
                "amax": torch.zeros(256, device="cuda")}

    def call(fn, a):
        if fn == "add_layernorm_bf16":
            return ext.add_layernorm_bf16(a["x"], a["other"], a["w"], a["b"],
                                          X.EPS)
        if fn == "layernorm_bf16_fp8":
            return ext.layernorm_bf16_fp8(a["x"], a["w"], a["b"], X.EPS,
                                          a["scale"], a["amax"])
        return ext.add_layernorm_bf16_fp8(a["x"], a["other"], a["w"], a["b"],
                                          X.EPS, a["scale"], a["amax"])

    param = [lambda t: t.cpu(), lambda t: t.float(), lambda t: t[:-4],
             lambda t: torch.cat([t, t]), _half_strided]
    bad = {
        "x": [lambda t: t[:0], lambda t: t.cpu()],
        "w": param,
        "b": param,
        "other": [lambda t: t.cpu(), lambda t: t.float(), lambda t: t[:-1]],
        "scale": [lambda t: t.cpu(), lambda t: t.double(),
                  lambda t: t.new_empty(0)],
        # a 0-d amax is what fp8.hidden_state builds for the GEMM side
        "amax": [lambda t: t.cpu(), lambda t: t.double(),
                 lambda t: t.new_zeros(()), lambda t: t[:255],
                 lambda t: t.new_zeros(512)[::2]],
    }
    uses = {"add_layernorm_bf16": ("x", "w", "b", "other"),
            "layernorm_bf16_fp8": ("x", "w", "b", "scale", "amax"),
            "add_layernorm_bf16_fp8": ("x", "w", "b", "other", "scale",
                                       "amax")}
    for fn, names in uses.items():
        for name in names:
            for change in bad[name]:
                a = args()
                a[name] = change(a[name])
                with pytest.raises(RuntimeError):
                    call(fn, a)
    for fn in uses:
        call(fn, args())                                    # the good calls
    torch.cuda.synchronize()
