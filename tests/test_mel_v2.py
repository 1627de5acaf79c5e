"""Multi-frame mel kernel (mel_fwd v2, ops/csrc/mel.hip) against a float64
evaluation of the same formula and against the two-frame kernel.

Shapes: T = 4801 / 12000 / 33603 samples give 11 / 26 / 71 frames at hop
480: an odd and an even frame count, remainders 3, 2 and 7 of an 8-frame
run, one odd T (the second row of the batch is then only 4-byte aligned),
and reflection at both ends of every clip.
"""

import functools

import pytest
import torch

from audiomuse_amd import config
from audiomuse_amd.ops import _ext, dsp, hip_ops

pytestmark = pytest.mark.gpu

CLAP_T = (4801, 12000, 33603)
MUSICNN_T = (512, 4000, 16001)


@functools.lru_cache(maxsize=None)
def _audio(T: int, B: int = 2) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + T)
    return (torch.randn(B, T, generator=g) * 0.2).clamp(-1, 1)


@functools.lru_cache(maxsize=None)
def _ref64(cfg_name: str, T: int, quant: bool) -> torch.Tensor:
    """float64 on the CPU: torch.stft with the periodic Hann window and
    reflect padding, dsp.mel_filterbank, the same log."""
    cfg = getattr(dsp, cfg_name)()
    a = _audio(T)
    if quant:
        a = dsp.int16_roundtrip(a)
    power = dsp.power_spectrogram(a.double(), cfg.n_fft, cfg.hop, cfg.center)
    fb = torch.from_numpy(dsp.mel_filterbank(
        cfg.sr, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax)).double()
    return dsp._apply_log(torch.matmul(fb, power), cfg.log_mode)


def _run(cfg, audio, v2: bool, monkeypatch, **kw) -> torch.Tensor:
    monkeypatch.setattr(config, "MEL_V2_ENABLE", v2)
    return hip_ops.mel_spectrogram(audio, cfg, **kw)


def _takes_v2(cfg) -> bool:
    plan = hip_ops._mel_plan(cfg, torch.device("cuda", 0))
    band = plan["band"]
    return band is not None and _ext.require().mel_fwd_takes_v2(
        cfg.n_fft, cfg.hop, cfg.n_mels, cfg.center, band["kmax"])


def _errors(x: torch.Tensor, ref: torch.Tensor):
    d = (x.double().cpu() - ref).abs()
    return float(d.max()), float(d.mean())


def test_clap_configuration_goes_to_v2():
    assert _takes_v2(dsp.clap_mel_config())
    assert not _takes_v2(dsp.musicnn_mel_config())


@pytest.mark.parametrize("quant", [False, True])
@pytest.mark.parametrize("T", CLAP_T)
def test_v2_against_reference_and_float64(T, quant, monkeypatch):
    cfg = dsp.clap_mel_config()
    audio = _audio(T).cuda()
    v1 = _run(cfg, audio, False, monkeypatch, quantize_int16=quant)
    v2 = _run(cfg, audio, True, monkeypatch, quantize_int16=quant)
    assert v2.shape == (2, cfg.n_mels, 1 + T // cfg.hop)
    ref32 = hip_ops.mel_spectrogram(audio, cfg, force_reference=True,
                                    quantize_int16=quant)
    ref64 = _ref64("clap_mel_config", T, quant)
    e1, e2 = _errors(v1, ref64), _errors(v2, ref64)
    print(f"T={T} quant={quant}: v1 max/mean abs err {e1[0]:.3e}/{e1[1]:.3e}"
          f"  v2 {e2[0]:.3e}/{e2[1]:.3e}  v2-v1 max abs "
          f"{float((v2 - v1).abs().max()):.3e}")
    torch.testing.assert_close(v2, ref32, rtol=1e-3, atol=2e-3)
    assert e2[0] <= 1.5 * e1[0]
    assert e2[1] <= 1.5 * e1[1]


@pytest.mark.parametrize("T", CLAP_T)
def test_v2_writes_every_element(T, monkeypatch):
    cfg = dsp.clap_mel_config()
    audio = _audio(T).cuda()
    out = torch.full((2, cfg.n_mels, 1 + T // cfg.hop), float("nan"),
                     device="cuda")
    res = _run(cfg, audio, True, monkeypatch, quantize_int16=True, out=out)
    assert res.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any()
    assert torch.equal(out, _run(cfg, audio, True, monkeypatch,
                                 quantize_int16=True))


@pytest.mark.parametrize("T", CLAP_T)
def test_v2_batch_independence(T, monkeypatch):
    cfg = dsp.clap_mel_config()
    audio = _audio(T, 3).cuda()
    full = _run(cfg, audio, True, monkeypatch, quantize_int16=True)
    for b in range(3):
        one = _run(cfg, audio[b:b + 1].contiguous(), True, monkeypatch,
                   quantize_int16=True)
        assert torch.equal(full[b], one[0])


@pytest.mark.parametrize("T", CLAP_T)
def test_switch_off_is_the_two_frame_kernel(T, monkeypatch):
    cfg = dsp.clap_mel_config()
    audio = _audio(T).cuda()
    off = _run(cfg, audio, False, monkeypatch, quantize_int16=True)
    plan = hip_ops._mel_plan(cfg, audio.device)
    direct = _ext.require().mel_fwd(
        audio, plan["window"], plan["twiddle"], plan["rowptr"], plan["bin"],
        plan["w"], cfg.hop, cfg.n_fft, cfg.center, 0, True)
    assert torch.equal(off, direct)


@pytest.mark.parametrize("T", MUSICNN_T)
def test_configurations_v2_does_not_take(T, monkeypatch):
    cfg = dsp.musicnn_mel_config()
    audio = _audio(T).cuda()
    if _takes_v2(cfg):
        ref64 = _ref64("musicnn_mel_config", T, False)
        e1 = _errors(_run(cfg, audio, False, monkeypatch), ref64)
        e2 = _errors(_run(cfg, audio, True, monkeypatch), ref64)
        print(f"musicnn T={T}: v1 {e1}  v2 {e2}")
        assert e2[0] <= 1.5 * e1[0] and e2[1] <= 1.5 * e1[1]
    else:
        assert torch.equal(_run(cfg, audio, True, monkeypatch),
                           _run(cfg, audio, False, monkeypatch))
