"""Fingerprint alignment throughput and the duplicate audit at scale.

Part 1: a synthetic bank of --bank fingerprints of --words words and
--pairs random pairs; pairs/s of
  (a) the one-pair host function bit_match_ratio, on --host-pairs pairs,
      extrapolated (a per-pair loop: the rate does not depend on the count);
  (b) the vectorised torch statement (chromaprint._align_torch) on GPU
      tensors, on the first --fallback-pairs pairs;
  (c) the fp_align kernel on all pairs.
(b) and (c): median [min..max] of --reps timed calls after a warm-up call,
host clock around a device synchronise. (b) and (c) must agree exactly on
the pairs both score, and (a) to 1e-12.

Part 2: the whole audit (analysis/duplicates.audit_pairs: neighbour graph,
candidate pairs, gates, one match_pairs call) at --tracks synthetic tracks
with --planted planted duplicate pairs, embeddings and bank resident on
the GPU; SQL loading is not part of it.

Needs a GPU and the native extension; there is no fallback.
"""

import argparse
import statistics
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.analysis.duplicates import audit_pairs  # noqa: E402
from audiomuse_amd.engines import chromaprint as cp  # noqa: E402
from audiomuse_amd.engines.similarity import SimilarityEngine  # noqa: E402
from audiomuse_amd.index.ivf import IVFIndex  # noqa: E402
from audiomuse_amd.ops import _ext  # noqa: E402


def timed(fn, reps):
    fn()                                   # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def rate_line(name, n_pairs, times):
    med = statistics.median(times)
    print(f"{name}: {n_pairs / med:14.0f} pairs/s  "
          f"{med * 1e3:9.2f} ms [{min(times) * 1e3:.2f}.."
          f"{max(times) * 1e3:.2f}] for {n_pairs} pairs, {len(times)} reps")
    return n_pairs / med


def bench_alignment(args, dev, g):
    F, L, P = args.bank, args.words, args.pairs
    words = torch.randint(0, 1 << 24, (F * L,), generator=g, device=dev,
                          dtype=torch.int32)
    off = torch.arange(F + 1, device=dev, dtype=torch.int64) * L
    bank = cp.FingerprintBank(words, off)
    pairs = torch.randint(0, F, (P, 2), generator=g, device=dev,
                          dtype=torch.int32)
    # every 8th pair is a shifted copy, so that not every score is ~0.5
    src = pairs[::8, 0].long()
    dst = pairs[::8, 1].long()
    keep = src != dst
    src, dst = src[keep][:F // 16], dst[keep][:F // 16]
    view = words.view(F, L)
    view[dst, : L - 7] = view[src, 7:]
    mo = C.CHROMAPRINT_ALIGN_RANGE // 2
    mw = max(8, C.CHROMAPRINT_MIN_OVERLAP // 8)
    ops = P * sum(min(L - abs(o), L) for o in range(-mo, mo + 1))
    print(f"bank {F} x {L} words ({words.numel() * 4 / 2**20:.0f} MiB), "
          f"{P} pairs, max_offset {mo}, min_words {mw}: "
          f"{ops / 1e9:.1f} G xor+popcount word operations per call")

    # (a) host loop
    hp = pairs[: args.host_pairs].cpu().numpy()
    host_words = view.cpu().numpy().view(np.uint32)
    blobs = {int(f): zlib.compress(host_words[f].tobytes())
             for f in np.unique(hp)}
    t0 = time.perf_counter()
    ref = np.array([cp.bit_match_ratio(blobs[int(i)], blobs[int(j)])
                    for i, j in hp])
    t_host = time.perf_counter() - t0
    print(f"(a) bit_match_ratio loop : {len(hp) / t_host:14.0f} pairs/s  "
          f"{t_host / len(hp) * 1e3:.3f} ms per pair on {len(hp)} pairs "
          f"(host CPU; {P} pairs would take {P * t_host / len(hp):.0f} s)")

    # (b) torch fallback on GPU tensors
    sub = pairs[: args.fallback_pairs].contiguous()
    tb = timed(lambda: cp._align_torch(bank, sub, mo, mw), args.reps)
    rb = rate_line("(b) torch fallback on GPU", sub.shape[0], tb)

    # (c) kernel, through the public call (validation sync included) and raw
    tc = timed(lambda: cp.align_pairs(bank, pairs, mo, mw), args.reps)
    rc = rate_line("(c) fp_align kernel      ", P, tc)
    ext = _ext.require()
    tr = timed(lambda: ext.fp_align(words, off, pairs, mo, mw, L), args.reps)
    rate_line("    raw binding call     ", P, tr)
    med = statistics.median(tr)
    print(f"    kernel: {ops / med / 1e12:.2f} T word operations/s, "
          f"{2 * P * L * 4 / med / 1e9:.0f} GB/s of fingerprint reads")
    print(f"(c) / (b) = {rc / rb:.1f}x; spread of (b) "
          f"{(max(tb) - min(tb)) / statistics.median(tb) * 100:.1f} %, of (c) "
          f"{(max(tc) - min(tc)) / statistics.median(tc) * 100:.1f} %")

    got = cp.align_pairs(bank, pairs, mo, mw)
    same = torch.equal(got[: sub.shape[0]], cp._align_torch(bank, sub, mo, mw))
    res = got[: len(hp)].cpu().numpy()
    err = np.abs(cp.ratio_from_alignment(res[:, 0], res[:, 1]) - ref).max()
    print(f"kernel == torch fallback on {sub.shape[0]} pairs: {same}; "
          f"max |kernel - bit_match_ratio| on {len(hp)} pairs: {err:.2g}")
    if not same or err > 1e-12:
        raise SystemExit("results differ")


def bench_audit(args, dev, g):
    n, d, L, planted = args.tracks, 200, args.words, args.planted
    centres = torch.randn(64, d, generator=g, device=dev) * 3
    sub = centres[torch.randint(0, 64, (4096,), generator=g, device=dev)] \
        + torch.randn(4096, d, generator=g, device=dev) * 0.5
    x = sub[torch.randint(0, 4096, (n,), generator=g, device=dev)] \
        + torch.randn(n, d, generator=g, device=dev)
    x[1:2 * planted:2] = x[0:2 * planted:2] + 0.05 * torch.randn(
        planted, d, generator=g, device=dev)
    words = torch.randint(0, 1 << 24, (n, L), generator=g, device=dev,
                          dtype=torch.int32)
    for s in range(0, 11):                  # shifted copies, 0..10 frames
        a = torch.arange(s, planted, 11, device=dev) * 2
        words[a + 1, : L - s] = words[a, s:]
    bank = cp.FingerprintBank(
        words.view(-1), torch.arange(n + 1, device=dev, dtype=torch.int64) * L)
    has_fp = torch.ones(n, dtype=torch.bool, device=dev)
    duration = torch.full((n,), 200.0, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = IVFIndex.build(x, metric="angular", device=dev)
    torch.cuda.synchronize()
    print(f"audit: {n} tracks x {d}, bank {words.numel() * 4 / 2**30:.2f} "
          f"GiB; index build {time.perf_counter() - t0:.2f} s "
          f"(nlist {index.nlist}, storage {index.storage})")
    del x
    engine = SimilarityEngine(index, [str(i) for i in range(n)])
    k = C.DUPLICATE_AUDIT_NEIGHBOURS
    for run in range(args.audit_runs):
        marks = []

        def stage(_p, details, marks=marks):
            torch.cuda.synchronize()
            marks.append((time.perf_counter(), details))

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = audit_pairs(engine, bank, has_fp, duration, k=k,
                          max_cosine=C.DUPLICATE_AUDIT_MAX_COSINE,
                          threshold=C.CHROMAPRINT_MATCH_THRESHOLD,
                          stage=stage)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        found = {tuple(p) for p in res["pairs"].tolist()}
        hit = sum((2 * i, 2 * i + 1) in found for i in range(planted))
        t_graph = marks[1][0] - marks[0][0]
        t_gate = marks[2][0] - marks[1][0]
        t_match = t1 - marks[2][0]
        print(f"audit run {run}: {t1 - t0:.2f} s whole (k={k}: graph + "
              f"unique pairs {t_graph:.2f} s, gates {t_gate:.2f} s, "
              f"match_pairs {t_match:.2f} s); {res['n_candidates']} "
              f"candidates, {res['n_compared']} compared, "
              f"{res['n_confirmed']} confirmed, {hit}/{planted} planted "
              f"pairs found, peak device memory "
              f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--bank", type=int, default=100_000)
    ap.add_argument("--words", type=int, default=969)
    ap.add_argument("--pairs", type=int, default=1_500_000)
    ap.add_argument("--host-pairs", type=int, default=2000)
    ap.add_argument("--fallback-pairs", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tracks", type=int, default=1_000_000)
    ap.add_argument("--planted", type=int, default=1100)
    ap.add_argument("--audit-runs", type=int, default=2)
    ap.add_argument("--skip-audit", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fingerprint_bench needs a GPU")
    _ext.require()
    dev = torch.device("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device=dev).manual_seed(0)
    bench_alignment(args, dev, g)
    torch.cuda.empty_cache()
    if not args.skip_audit:
        bench_audit(args, dev, g)


if __name__ == "__main__":
    main()
