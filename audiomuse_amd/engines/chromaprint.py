"""Acoustic fingerprint (chromaprint-class).

Reference: /root/reference/tasks/chromaprint.py shells out to a vendored
`fpcalc` binary and compares zlib-compressed raw int fingerprints by
alignment/overlap bit-match. No fpcalc binary ships in this image, so
this is a first-party chroma fingerprint with the same role and
comparison semantics: 12-bin chroma frames -> temporal/spectral gradient
binarization -> packed uint32 frames; agreement = best-aligned bit-match
ratio over the overlap (chromaprint.py:67-115 behavior).
"""

from __future__ import annotations

import zlib
from typing import Optional

import numpy as np

from audiomuse_amd import config as C
import torch

from audiomuse_amd.ops.features import chroma_from_stft

FP_SR = 11025
_FRAME_BITS = 24          # 12 temporal + 12 spectral gradient bits


def compute(audio: torch.Tensor, sr: int, max_seconds: float = 120.0
            ) -> bytes:
    """zlib-compressed packed fingerprint of (<= max_seconds of) audio."""
    from audiomuse_amd.ops.audio_io import resample

    audio = audio.float().flatten()[: int(sr * max_seconds)]
    a = resample(audio, sr, FP_SR)
    chroma = chroma_from_stft(a, FP_SR, n_fft=4096, hop=1365)  # ~8 fps
    c = chroma.T.cpu().numpy()                                  # (frames, 12)
    if c.shape[0] < 3:
        return b""
    dt = (c[1:] > c[:-1]).astype(np.uint32)                     # temporal grad
    ds = (c[1:, :] > np.roll(c[1:, :], 1, axis=1)).astype(np.uint32)
    words = np.zeros(dt.shape[0], dtype=np.uint32)
    for b in range(12):
        words |= dt[:, b] << b
        words |= ds[:, b] << (12 + b)
    return zlib.compress(words.tobytes())


def _unpack(fp: bytes) -> Optional[np.ndarray]:
    if not fp:
        return None
    try:
        raw = zlib.decompress(fp)
    except zlib.error:
        return None
    return np.frombuffer(raw, dtype=np.uint32)


def bit_match_ratio(fp_a: bytes, fp_b: bytes,
                    max_offset: Optional[int] = None) -> float:
    """Best aligned per-bit agreement over the overlap (the reference's
    align/overlap/bit-match comparison). Alignment range and minimum
    overlap come from config (CHROMAPRINT_ALIGN_RANGE /
    CHROMAPRINT_MIN_OVERLAP)."""
    if max_offset is None:
        max_offset = C.CHROMAPRINT_ALIGN_RANGE // 2
    a = _unpack(fp_a)
    b = _unpack(fp_b)
    if a is None or b is None or a.size == 0 or b.size == 0:
        return 0.0
    best = 0.0
    for off in range(-max_offset, max_offset + 1):
        if off >= 0:
            aa, bb = a[off:], b
        else:
            aa, bb = a, b[-off:]
        n = min(aa.size, bb.size)
        if n < max(8, C.CHROMAPRINT_MIN_OVERLAP // 8):
            continue
        diff = np.bitwise_xor(aa[:n], bb[:n])
        bits = np.unpackbits(diff.view(np.uint8)).sum()
        ratio = 1.0 - bits / (n * 32.0)
        # only 24 of 32 bits carry signal; rescale agreement over them
        ratio = max(0.0, (ratio * 32.0 - 8.0) / 24.0)
        best = max(best, ratio)
    return best


def chromaprints_agree(fp_a: bytes, fp_b: bytes,
                       threshold: float = 0.85) -> bool:
    return bit_match_ratio(fp_a, fp_b) >= threshold


# -- batched comparison ------------------------------------------------------
#
# bit_match_ratio above answers for one pair per call. The catalogue audit
# (analysis/duplicates.py) asks for millions of pairs, so the fingerprints
# are decompressed once into a FingerprintBank and match_pairs scores a
# whole list of pairs in one call: ops/csrc/fingerprint.hip on the GPU, a
# vectorised torch statement of the same integer arithmetic elsewhere.

FP_LDS_WORDS = 4096      # longest fingerprint the kernel stages in LDS
MAX_ALIGN_OFFSET = 1024  # the kernel binding's bound on max_offset
_FALLBACK_CHUNK_WORDS = 1 << 22


class FingerprintBank:
    """All fingerprints back to back: `words` int32 (W,) holds the bit
    pattern of every packed uint32 frame, fingerprint f is
    words[off[f]:off[f+1]] (`off` int64 (F+1,)). Length 0 means "no usable
    fingerprint" and scores 0.0 against everything."""

    def __init__(self, words: torch.Tensor, off: torch.Tensor):
        if words.dtype != torch.int32 or words.dim() != 1:
            raise ValueError("words must be a 1-D int32 tensor")
        if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1:
            raise ValueError("off must be a 1-D int64 tensor of F+1 entries")
        if off.device != words.device:
            raise ValueError("words and off must be on one device")
        self.words = words.contiguous()
        self.off = off.contiguous()
        self._checked = False

    def __len__(self) -> int:
        return self.off.numel() - 1

    @property
    def device(self) -> torch.device:
        return self.words.device

    @classmethod
    def from_blobs(cls, blobs, device="cpu") -> "FingerprintBank":
        """Decompress each blob once. None, empty and undecodable blobs
        (bad zlib stream, not a whole number of words) become length 0."""
        parts, lens = [], []
        for blob in blobs:
            arr = None
            if blob:
                try:
                    arr = _unpack(bytes(blob))
                except ValueError:
                    arr = None
            if arr is None or arr.size == 0:
                lens.append(0)
            else:
                parts.append(arr)
                lens.append(int(arr.size))
        return cls.from_arrays(parts, lens, device)

    @classmethod
    def from_arrays(cls, parts, lens, device="cpu") -> "FingerprintBank":
        """parts: the non-empty uint32 arrays in order; lens: the length of
        every fingerprint, zeros included."""
        flat = (np.concatenate(parts) if parts
                else np.zeros(0, dtype=np.uint32))
        off = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
        words = torch.from_numpy(
            np.ascontiguousarray(flat, dtype=np.uint32).view(np.int32).copy())
        return cls(words.to(device), torch.from_numpy(off).to(device))

    def check(self) -> None:
        """off must start at 0, never decrease and end at W. Checked once
        per bank, on the bank's device."""
        if self._checked:
            return
        off = self.off
        ok = (off[0] == 0) & (off[-1] == self.words.numel())
        if off.numel() > 1:
            ok = ok & (off[1:] >= off[:-1]).all()
        if not bool(ok):
            raise ValueError("FingerprintBank.off must be non-decreasing "
                             "from 0 to len(words)")
        self._checked = True


def _popcount32(x: torch.Tensor) -> torch.Tensor:
    """Bits set in the low 32 bits of an int64 tensor (values in
    [0, 2^32))."""
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) >> 24) & 0xFF


def _align_torch(bank: FingerprintBank, pairs: torch.Tensor, max_offset: int,
                 min_words: int) -> torch.Tensor:
    """(P, 3) int32 (bits, n, offset) with the kernel's semantics, as
    torch ops on the bank's device. One pass per offset over a padded
    (pairs, words) block; pairs go through in length order so that a block
    is padded to lengths close to its own."""
    dev = bank.device
    P = pairs.shape[0]
    out = torch.zeros((P, 3), dtype=torch.int32, device=dev)
    if P == 0:
        return out
    # uint32 values in int64, with one zero word of padding to gather from
    words = torch.cat([bank.words.to(torch.int64) & 0xFFFFFFFF,
                       torch.zeros(1, dtype=torch.int64, device=dev)])
    pad = words.numel() - 1
    ia, ib = pairs[:, 0].long(), pairs[:, 1].long()
    a0, b0 = bank.off[ia], bank.off[ib]
    la, lb = bank.off[ia + 1] - a0, bank.off[ib + 1] - b0
    order = torch.argsort(torch.minimum(la, lb))
    lmin = torch.minimum(la, lb)[order].cpu()
    start = 0
    while start < P:
        # rows * (the block's longest overlap, its last row's) stays bounded
        stop = min(P, start + _FALLBACK_CHUNK_WORDS // max(int(lmin[start]), 1))
        while stop > start + 1 and \
                (stop - start) * int(lmin[stop - 1]) > _FALLBACK_CHUNK_WORDS:
            stop = start + max(
                1, _FALLBACK_CHUNK_WORDS // int(lmin[stop - 1]))
        sel = order[start:stop]
        start = stop
        sa0, sb0, sla, slb = a0[sel], b0[sel], la[sel], lb[sel]
        L = int(torch.minimum(sla, slb).max())
        if L < min_words:
            continue
        j = torch.arange(L, device=dev)
        best_bits = torch.zeros(sel.numel(), dtype=torch.int64, device=dev)
        best_n = torch.zeros_like(best_bits)
        best_off = torch.zeros_like(best_bits)
        for o in range(-max_offset, max_offset + 1):
            sh_a, sh_b = max(o, 0), max(-o, 0)
            n = torch.minimum(sla - sh_a, slb - sh_b).clamp_(min=0)
            live = n >= min_words
            if not bool(live.any()):
                continue
            mask = j[None, :] < torch.where(live, n, 0)[:, None]
            xa = words[torch.where(mask, (sa0 + sh_a)[:, None] + j, pad)]
            xb = words[torch.where(mask, (sb0 + sh_b)[:, None] + j, pad)]
            bits = _popcount32(xa ^ xb).sum(dim=1)
            # strictly smaller bits / n, by cross-multiplication; offsets
            # ascend, so ties keep the lowest one
            better = live & ((best_n == 0) | (bits * best_n < best_bits * n))
            best_bits = torch.where(better, bits, best_bits)
            best_n = torch.where(better, n, best_n)
            best_off = torch.where(better, o, best_off)
        out[sel] = torch.stack([best_bits, best_n, best_off],
                               dim=1).to(torch.int32)
    return out


def align_pairs(bank: FingerprintBank, pairs, max_offset: Optional[int] = None,
                min_words: Optional[int] = None) -> torch.Tensor:
    """Best alignment of every pair: (P, 3) int32 (bits, n, offset) on the
    bank's device, (0, 0, 0) where no alignment reaches min_words.

    For o in [-max_offset, max_offset], o >= 0 compares a[o:] with b and
    o < 0 compares a with b[-o:]; n is the overlap, bits the differing
    bits over all 32 bits of the n words; the smallest bits / n wins and,
    among equal fractions, the lowest offset.

    The bank and the pair indices are checked on the device before any
    launch (ValueError): an index outside the bank would be a wild read.
    A GPU bank goes to the HIP kernel; pairs with a fingerprint longer
    than FP_LDS_WORDS, and CPU banks, take the torch path."""
    if max_offset is None:
        max_offset = C.CHROMAPRINT_ALIGN_RANGE // 2
    if min_words is None:
        min_words = max(8, C.CHROMAPRINT_MIN_OVERLAP // 8)
    max_offset, min_words = int(max_offset), int(min_words)
    if not 0 <= max_offset <= MAX_ALIGN_OFFSET:
        raise ValueError(f"max_offset must be in [0, {MAX_ALIGN_OFFSET}]")
    if min_words < 1:
        raise ValueError("min_words must be >= 1")
    dev = bank.device
    pairs = torch.as_tensor(pairs)
    if pairs.numel() == 0:
        return torch.zeros((0, 3), dtype=torch.int32, device=dev)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.is_floating_point():
        raise ValueError("pairs must be an integer (P, 2) array")
    pairs = pairs.to(dev)
    bank.check()
    F = len(bank)
    # one reduction, one sync: index range and the longest fingerprint used
    lo, hi = torch.aminmax(pairs)
    idx = pairs.long().clamp(0, max(F - 1, 0))
    lens = (bank.off[1:] - bank.off[:-1]) if F else bank.off[:0]
    longest = lens[idx].max() if F else lo
    lo, hi, longest = torch.stack([lo.long(), hi.long(),
                                   longest.long()]).tolist()
    if lo < 0 or hi >= F:
        raise ValueError(f"pair index outside the bank [0, {F}): "
                         f"min {lo}, max {hi}")
    pairs = pairs.to(torch.int32).contiguous()

    from audiomuse_amd.ops import _ext
    ext = _ext.native_or_none() if dev.type == "cuda" else None
    if ext is None:
        return _align_torch(bank, pairs, max_offset, min_words)
    if longest <= FP_LDS_WORDS:
        return ext.fp_align(bank.words, bank.off, pairs, max_offset,
                            min_words, max(int(longest), 1))
    over = (lens[pairs.long()] > FP_LDS_WORDS).any(dim=1)
    out = torch.empty((pairs.shape[0], 3), dtype=torch.int32, device=dev)
    fit = pairs[~over].contiguous()
    if fit.shape[0]:
        out[~over] = ext.fp_align(bank.words, bank.off, fit, max_offset,
                                  min_words, FP_LDS_WORDS)
    out[over] = _align_torch(bank, pairs[over], max_offset, min_words)
    return out


def ratio_from_alignment(bits: np.ndarray, n: np.ndarray) -> np.ndarray:
    """max(0, 1 - bits / (24 n)) in float64, 0.0 where n = 0: the algebraic
    form of bit_match_ratio's (r * 32 - 8) / 24 with r = 1 - bits / (32 n)."""
    bits = np.asarray(bits, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    ratio = np.zeros(bits.shape, dtype=np.float64)
    np.divide(bits, _FRAME_BITS * n, out=ratio, where=n > 0)
    return np.where(n > 0, np.maximum(0.0, 1.0 - ratio), 0.0)


def match_pairs(bank: FingerprintBank, pairs,
                max_offset: Optional[int] = None,
                min_words: Optional[int] = None):
    """bit_match_ratio for a list of pairs of bank entries: (ratio float64
    (P,), offset int32 (P,)) as numpy. Defaults as in bit_match_ratio."""
    res = align_pairs(bank, pairs, max_offset, min_words).cpu().numpy()
    return (ratio_from_alignment(res[:, 0], res[:, 1]),
            res[:, 2].astype(np.int32))
