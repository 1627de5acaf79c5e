"""Batched fingerprint alignment (engines/chromaprint.match_pairs and the
fp_align kernel) against the one-pair host function bit_match_ratio and a
pure-integer host reference."""

import zlib

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import chromaprint as cp

MAX_REF_OFFSET = 100


def _blob(arr) -> bytes:
    return zlib.compress(np.asarray(arr, dtype=np.uint32).tobytes())


def _small_arrays():
    """The fingerprints every test uses, as uint32 arrays (empty = length
    0), and the positions of the shifted copies by shift."""
    rng = np.random.default_rng(1234)
    arrs = [rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
            for n in (0, 1, 14, 15, 16, 63, 64, 65, 129, 300)]
    base = rng.integers(0, 1 << 24, size=600, dtype=np.uint32)
    shifted = {}
    for s in (-41, -40, -1, 0, 1, 40, 41):
        a = base[100 + s: 500 + s].copy()
        for w in rng.choice(400, size=3, replace=False):
            a[w] ^= np.uint32(1 << int(rng.integers(0, 24)))
        shifted[s] = len(arrs)
        arrs.append(a)
    # top byte set (stored blobs may carry it; nothing masks it) ...
    arrs.append(rng.integers(0, 1 << 32, size=200, dtype=np.uint32)
                | np.uint32(0xFF000000))
    # ... and two that differ in all 32 bits at every alignment: 1 - 32/24
    # is negative and must clamp to 0
    arrs.append(np.full(120, 0xFFFFFFFF, dtype=np.uint32))
    arrs.append(np.zeros(120, dtype=np.uint32))
    return arrs, shifted


@pytest.fixture(scope="module")
def small():
    arrs, shifted = _small_arrays()
    blobs = [_blob(a) for a in arrs] + [b"", None, b"xx"]
    arrs = arrs + [np.zeros(0, dtype=np.uint32)] * 3
    return {"arrs": arrs, "blobs": blobs, "shifted": shifted,
            "bank": cp.FingerprintBank.from_blobs(blobs)}


# -- CPU ---------------------------------------------------------------------

def test_bank_layout(small):
    bank, arrs = small["bank"], small["arrs"]
    assert len(bank) == len(arrs)
    assert bank.words.dtype == torch.int32 and bank.off.dtype == torch.int64
    off = bank.off.tolist()
    assert off[0] == 0 and off[-1] == bank.words.numel()
    for f, a in enumerate(arrs):
        got = bank.words[off[f]:off[f + 1]].numpy().view(np.uint32)
        assert np.array_equal(got, a)


def test_match_pairs_equals_bit_match_ratio(small):
    """abs <= 1e-12: float64 rounding of two divisions is all that
    separates 1 - bits / (24 n) from the host's (r * 32 - 8) / 24."""
    bank, blobs = small["bank"], small["blobs"]
    F = len(bank)
    pairs = [(i, j) for i in range(F) for j in range(F)]   # (i, i) included
    pairs += pairs[5:25] + [(3, 3), (3, 3)]                # repeated pairs
    ratio, offset = cp.match_pairs(bank, np.array(pairs))
    assert ratio.dtype == np.float64 and ratio.shape == (len(pairs),)
    assert offset.dtype == np.int32 and offset.shape == (len(pairs),)
    ref = np.array([cp.bit_match_ratio(blobs[i], blobs[j]) for i, j in pairs])
    err = np.abs(ratio - ref).max()
    print(f"max |match_pairs - bit_match_ratio| = {err:.3g}")
    assert err <= 1e-12
    # the bank really holds matches, misses and clamped pairs
    assert ratio.max() == 1.0 and (ratio == 0.0).any() and \
        ((ratio > 0.2) & (ratio < 0.8)).any()


def test_shifted_copies(small):
    bank, sh = small["bank"], small["shifted"]
    zero = sh[0]
    shifts = sorted(sh)
    ratio, offset = cp.match_pairs(
        bank, np.array([(zero, sh[s]) for s in shifts]))
    for s, r, o in zip(shifts, ratio.tolist(), offset.tolist()):
        if abs(s) <= C.CHROMAPRINT_ALIGN_RANGE // 2:
            # 6 flipped bits (3 when s = 0 compares the copy with itself)
            # over at least 360 words
            assert r > 0.999 and o == s, (s, r, o)
        else:
            assert r < 0.7 and r < C.CHROMAPRINT_MATCH_THRESHOLD, (s, r, o)
    in_range = min(r for s, r in zip(shifts, ratio) if abs(s) <= 40)
    out_of_range = max(r for s, r in zip(shifts, ratio) if abs(s) > 40)
    assert out_of_range < in_range


def test_unusable_blobs_score_zero(small):
    bank = small["bank"]
    F = len(bank)
    dead = [F - 3, F - 2, F - 1, 0]         # b"", None, b"xx", length 0
    pairs = [(d, j) for d in dead for j in range(F)]
    pairs += [(j, d) for d in dead for j in range(F)]
    ratio, offset = cp.match_pairs(bank, np.array(pairs))
    assert not ratio.any() and not offset.any()


def test_clamp_to_zero(small):
    bank = small["bank"]
    ones = len(small["arrs"]) - 5
    zeros = ones + 1
    ratio, _ = cp.match_pairs(bank, np.array([(ones, zeros), (zeros, ones)]))
    assert ratio.tolist() == [0.0, 0.0]
    res = cp.align_pairs(bank, np.array([(ones, zeros)])).tolist()[0]
    assert res[0] == 32 * res[1] and res[1] > 0      # compared, then clamped


def test_single_fingerprint_and_empty_pairs():
    arr = np.random.default_rng(5).integers(0, 1 << 24, size=40,
                                            dtype=np.uint32)
    bank = cp.FingerprintBank.from_blobs([_blob(arr)])
    assert len(bank) == 1
    ratio, offset = cp.match_pairs(bank, np.array([(0, 0)]))
    assert ratio.tolist() == [1.0] and offset.tolist() == [0]
    for empty in (np.zeros((0, 2), dtype=np.int64), []):
        ratio, offset = cp.match_pairs(bank, empty)
        assert ratio.shape == (0,) and ratio.dtype == np.float64
        assert offset.shape == (0,) and offset.dtype == np.int32


@pytest.mark.parametrize("bad", [-1, "F"])
def test_bad_pair_index_raises(small, bad):
    bank = small["bank"]
    bad = len(bank) if bad == "F" else bad
    with pytest.raises(ValueError):
        cp.match_pairs(bank, np.array([(0, 1), (bad, 2)]))
    with pytest.raises(ValueError):
        cp.match_pairs(bank, np.array([(0, 1), (2, bad)]))


def test_scalar_ranges_and_broken_bank(small):
    bank = small["bank"]
    for kw in ({"max_offset": -1}, {"max_offset": 1025}, {"min_words": 0}):
        with pytest.raises(ValueError):
            cp.match_pairs(bank, np.array([(0, 1)]), **kw)
    off = bank.off.clone()
    off[3] = off[4] + 1                                  # decreasing
    with pytest.raises(ValueError):
        cp.match_pairs(cp.FingerprintBank(bank.words, off), np.array([(0, 1)]))
    off = bank.off.clone()
    off[-1] += 1                                         # past the words
    with pytest.raises(ValueError):
        cp.match_pairs(cp.FingerprintBank(bank.words, off), np.array([(0, 1)]))


# -- GPU ---------------------------------------------------------------------

def _popcount(x: np.ndarray) -> int:
    if hasattr(np, "bitwise_count"):
        return int(np.bitwise_count(x).sum())
    return int(np.unpackbits(x.view(np.uint8)).sum())


def _offset_table(a: np.ndarray, b: np.ndarray):
    """(bits, n) of every alignment o in [-MAX_REF_OFFSET, MAX_REF_OFFSET]
    as Python ints; n <= 0 where the two do not overlap."""
    table = {}
    for o in range(-MAX_REF_OFFSET, MAX_REF_OFFSET + 1):
        aa, bb = (a[o:], b) if o >= 0 else (a, b[-o:])
        n = min(aa.size, bb.size)
        table[o] = (_popcount(aa[:n] ^ bb[:n]) if n > 0 else 0, n)
    return table


def _best(table, max_offset: int, min_words: int):
    """The sequential scan in integers: smallest bits / n by
    cross-multiplication, the first (lowest) offset among equals."""
    best = (0, 0, 0)
    for o in range(-max_offset, max_offset + 1):
        bits, n = table[o]
        if n < min_words:
            continue
        if best[1] == 0 or bits * best[1] < best[0] * n:
            best = (bits, n, o)
    return best


@pytest.fixture(scope="module")
def gpu_case():
    """Bank (small set + 969 words + exactly the LDS cap + cap + 1), 1000
    pairs of which fewer than 200 touch a fingerprint of 969 words or more,
    and the host's offset table of every pair, computed once."""
    pytest.importorskip("audiomuse_amd._C")
    rng = np.random.default_rng(99)
    arrs, _ = _small_arrays()
    n_small = len(arrs)
    cap = cp.FP_LDS_WORDS

    def noisy_shift(src, shift, length):
        out = src[200 + shift: 200 + shift + length].copy()
        out[rng.choice(length, size=5, replace=False)] ^= np.uint32(0x10)
        return out

    long_base = rng.integers(0, 1 << 32, size=cap + 500, dtype=np.uint32)
    big = [noisy_shift(long_base, 0, 969), noisy_shift(long_base, 37, 969),
           noisy_shift(long_base, -100, 969),
           noisy_shift(long_base, 0, cap), noisy_shift(long_base, -3, cap),
           noisy_shift(long_base, 1, cap + 1),
           rng.integers(0, 1 << 32, size=cap + 1, dtype=np.uint32)]
    arrs = arrs + big
    F = len(arrs)
    big_ids = list(range(n_small, F))
    pairs = [(big_ids[0], big_ids[1])]
    pairs += [(i, j) for i in big_ids for j in big_ids]            # 49
    pairs += [(i, int(rng.integers(0, n_small))) for i in big_ids
              for _ in range(8)]                                   # 56
    pairs += [(int(rng.integers(0, n_small)), i) for i in big_ids
              for _ in range(8)]                                   # 56
    assert len(pairs) < 200
    rest = rng.integers(0, n_small, size=(1000 - len(pairs), 2)).tolist()
    tail = [tuple(p) for p in rest]
    mixed = pairs[1:] + tail
    order = rng.permutation(len(mixed))
    pairs = [pairs[0]] + [mixed[i] for i in order]
    assert len(pairs) == 1000
    tables = {}
    for i, j in pairs:
        if (i, j) not in tables:
            tables[(i, j)] = _offset_table(arrs[i], arrs[j])
    lens = [a.size for a in arrs]
    bank = cp.FingerprintBank.from_arrays([a for a in arrs if a.size], lens,
                                          "cuda")
    return {"bank": bank, "pairs": np.array(pairs, dtype=np.int64),
            "tables": tables, "n_small": n_small, "F": F}


@pytest.mark.gpu
@pytest.mark.parametrize("min_words", [1, 15])
@pytest.mark.parametrize("max_offset", [0, 1, 40, 100])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_kernel_equals_integer_reference(gpu_case, P, max_offset, min_words):
    pairs = gpu_case["pairs"][:P]
    got = cp.align_pairs(gpu_case["bank"], pairs, max_offset, min_words)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (P, 3)
    got = got.cpu().tolist()
    for (i, j), (bits, n, off) in zip(pairs.tolist(), got):
        rb, rn, ro = _best(gpu_case["tables"][(i, j)], max_offset, min_words)
        assert bits * rn == rb * n and off == ro and n == rn, \
            ((i, j), (bits, n, off), (rb, rn, ro))


@pytest.mark.gpu
def test_kernel_is_the_path_taken(gpu_case):
    """Pairs under the LDS cap go to fp_align and give what the torch
    statement of the same arithmetic gives; the raw binding agrees."""
    from audiomuse_amd.ops import _ext
    bank = gpu_case["bank"]
    sel = (gpu_case["pairs"] < gpu_case["F"] - 2).all(axis=1)  # cap + 1 out
    pairs = torch.from_numpy(gpu_case["pairs"][sel]).to("cuda", torch.int32)
    via = cp.align_pairs(bank, pairs, 40, 15)
    raw = _ext.require().fp_align(bank.words, bank.off, pairs.contiguous(),
                                  40, 15, cp.FP_LDS_WORDS)
    ref = cp._align_torch(bank, pairs, 40, 15)
    assert torch.equal(via, raw) and torch.equal(via, ref)


@pytest.mark.gpu
def test_kernel_repeatable_and_stream(gpu_case):
    bank, pairs = gpu_case["bank"], gpu_case["pairs"]
    first = cp.align_pairs(bank, pairs, 40, 15)
    second = cp.align_pairs(bank, pairs, 40, 15)
    assert torch.equal(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = cp.align_pairs(bank, pairs, 40, 15)
    side.synchronize()
    assert torch.equal(first, third)


@pytest.mark.gpu
def test_kernel_bad_index_raises_before_launch(gpu_case):
    bank = gpu_case["bank"]
    for bad in (-1, gpu_case["F"], 2 ** 31 - 1):
        with pytest.raises(ValueError):
            cp.align_pairs(bank, np.array([(0, 1), (bad, 2)]))
    torch.cuda.synchronize()
    # and the bank is still usable
    assert cp.align_pairs(bank, np.array([(4, 4)]), 40, 15).tolist() \
        == [[0, 16, 0]]


@pytest.mark.gpu
def test_binding_checks(gpu_case):
    from audiomuse_amd.ops import _ext
    ext, bank = _ext.require(), gpu_case["bank"]
    pairs = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    for args in ((bank.words.long(), bank.off, pairs, 40, 15, 4096),
                 (bank.words, bank.off.int(), pairs, 40, 15, 4096),
                 (bank.words, bank.off, pairs.long(), 40, 15, 4096),
                 (bank.words, bank.off, pairs.t(), 40, 15, 4096),
                 (bank.words, bank.off, pairs.flatten(), 40, 15, 4096),
                 (bank.words.cpu(), bank.off, pairs, 40, 15, 4096),
                 (bank.words, bank.off, pairs, 1025, 15, 4096),
                 (bank.words, bank.off, pairs, -1, 15, 4096),
                 (bank.words, bank.off, pairs, 40, 0, 4096),
                 (bank.words, bank.off, pairs, 40, 15, 4097),
                 (bank.words, bank.off, pairs, 40, 15, 0)):
        with pytest.raises(RuntimeError):
            ext.fp_align(*args)
    empty = ext.fp_align(bank.words, bank.off, pairs[:0], 40, 15, 4096)
    assert empty.shape == (0, 3)
