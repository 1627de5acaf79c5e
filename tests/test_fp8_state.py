"""Delayed-scale bookkeeping of the fp8 serving mode (ops/fp8.py), on the
CPU: _state_for feeds the e4m3 LayerNorm kernels, hidden_state the fp8-D
GEMMs. Both are pure torch."""

import gc

import pytest
import torch

from audiomuse_amd.ops import fp8

CPU = torch.device("cpu")
META = torch.device("meta")      # a second device that needs no hardware


class _Owner(torch.nn.Module):
    pass


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def test_state_for_starts_at_the_init_scale_with_256_zero_slots():
    m = _Owner()
    scale, amax = fp8._state_for(m, CPU)
    assert scale.dtype == torch.float32 and scale.dim() == 0
    assert scale.item() == _f32(8.0 / 448.0).item()
    assert amax.dtype == torch.float32 and amax.shape == (256,)
    assert amax.is_contiguous() and not amax.any()


def test_state_for_rescales_from_the_recorded_amax_and_zeroes_it():
    m = _Owner()
    scale, amax = fp8._state_for(m, CPU)
    amax[3] = 2.5
    amax[200] = 5.25                    # the kernel's slots: the max counts
    scale2, amax2 = fp8._state_for(m, CPU)
    assert scale2 is scale and amax2 is amax      # updated in place
    assert scale.item() == ((_f32(5.25) * 1.05) / 448.0).item()
    assert not amax.any()
    # nothing recorded since: the clamp keeps the scale positive
    scale3, _ = fp8._state_for(m, CPU)
    assert scale3.item() == ((_f32(1e-6) * 1.05) / 448.0).item()
    assert scale3.item() > 0


def test_state_for_keeps_modules_apart():
    a, b = _Owner(), _Owner()
    sa, aa = fp8._state_for(a, CPU)
    sb, ab = fp8._state_for(b, CPU)
    assert sa is not sb and aa is not ab
    aa[0] = 100.0
    ab[0] = 1.0
    assert fp8._state_for(a, CPU)[0].item() == ((_f32(100.0) * 1.05) / 448.0).item()
    assert fp8._state_for(b, CPU)[0].item() == ((_f32(1.0) * 1.05) / 448.0).item()


@pytest.mark.parametrize("table,make", [
    ("_ln_state", lambda m: fp8._state_for(m, CPU)),
    ("_hid_state", lambda m: fp8.hidden_state(m, CPU)),
])
def test_state_dies_with_its_module(table, make):
    m = _Owner()
    make(m)
    key = id(m)
    cache = getattr(fp8, table)
    assert key in cache and cache[key][0]() is m
    del m
    gc.collect()
    assert key not in cache


def test_state_for_reinitialises_on_a_device_change():
    m = _Owner()
    scale, amax = fp8._state_for(m, CPU)
    amax[0] = 50.0
    fp8._state_for(m, CPU)
    assert scale.item() != _f32(8.0 / 448.0).item()
    s_meta, a_meta = fp8._state_for(m, META)
    assert s_meta.device == META and a_meta.device == META
    assert a_meta.shape == (256,)
    # and back: a fresh state at the init scale, not the one left behind
    s_cpu, a_cpu = fp8._state_for(m, CPU)
    assert s_cpu is not scale
    assert s_cpu.item() == _f32(8.0 / 448.0).item() and not a_cpu.any()


def test_stale_entry_of_a_reused_id_is_not_returned():
    m = _Owner()
    fp8._state_for(m, CPU)
    other = _Owner()
    ent = fp8._ln_state[id(m)]
    fp8._ln_state[id(other)] = ent       # as if the id had been reused
    try:
        assert fp8._weak_get(fp8._ln_state, other) is None
        scale, amax = fp8._state_for(other, CPU)
        assert scale.item() == _f32(8.0 / 448.0).item() and not amax.any()
        assert fp8._weak_get(fp8._ln_state, m) is not None
    finally:
        fp8._ln_state.pop(id(other), None)


def test_hidden_state_init_update_and_inverse():
    m = _Owner()
    scale, inv, amax = fp8.hidden_state(m, CPU)
    assert scale.item() == _f32(4.0 / 448.0).item()
    assert inv.item() == _f32(448.0 / 4.0).item()
    assert amax.dim() == 0 and amax.item() == 0.0
    amax.fill_(3.5)
    s2, i2, a2 = fp8.hidden_state(m, CPU)
    assert s2 is scale and i2 is inv and a2 is amax
    want = (_f32(3.5) * 1.05) / 448.0
    assert scale.item() == want.item()
    assert inv.item() == (1.0 / want).item()
    assert amax.item() == 0.0
    # all-zero amax: clamped at 1e-6, inverse still finite and consistent
    fp8.hidden_state(m, CPU)
    want = (_f32(1e-6) * 1.05) / 448.0
    assert scale.item() == want.item() and inv.item() == (1.0 / want).item()
    assert torch.isfinite(inv)


def test_hidden_state_keeps_modules_apart_and_follows_the_device():
    a, b = _Owner(), _Owner()
    sa, _, aa = fp8.hidden_state(a, CPU)
    sb, _, ab = fp8.hidden_state(b, CPU)
    aa.fill_(10.0)
    ab.fill_(0.5)
    fp8.hidden_state(a, CPU)
    fp8.hidden_state(b, CPU)
    assert sa.item() == ((_f32(10.0) * 1.05) / 448.0).item()
    assert sb.item() == ((_f32(0.5) * 1.05) / 448.0).item()
    s_meta, i_meta, a_meta = fp8.hidden_state(a, META)
    assert s_meta.device == META and i_meta.device == META
    s_cpu, i_cpu, a_cpu = fp8.hidden_state(a, CPU)
    assert s_cpu is not sa
    assert s_cpu.item() == _f32(4.0 / 448.0).item()
    assert i_cpu.item() == _f32(448.0 / 4.0).item() and a_cpu.item() == 0.0
