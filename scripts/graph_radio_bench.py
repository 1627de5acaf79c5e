"""The graph radio (SONIC_FINGERPRINT_ENGINE=graph) on a resident f16 index:
time per sweep of the fused rank_pull kernel for 1, 2 and 8 legs, of its
torch statement on the same GPU and of one path_relax sweep on the same
graph and legs (the yardstick: the same gather pattern), a whole
personalised PageRank at the default sweep count, and a warm graph_radio
call end to end next to the warm centroid query it replaces. Output of the
runs at 1M x 200: profiles/r9_graph_radio.txt.

    python scripts/graph_radio_bench.py [n] [--sets flat20,two15]
"""

import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.engines import graph_path as G  # noqa: E402
from audiomuse_amd.engines import graph_radio as R  # noqa: E402
from audiomuse_amd.engines.similarity import SimilarityEngine  # noqa: E402
from audiomuse_amd.index.ivf import IVFIndex  # noqa: E402


def flat20(n, d, dev):
    """20 centres x3, unit noise."""
    g = torch.Generator(device=dev).manual_seed(0)
    top = torch.randn(20, d, generator=g, device=dev) * 3
    x = top[torch.randint(0, 20, (n,), generator=g, device=dev)]
    x += torch.randn(n, d, generator=g, device=dev)
    return x


def two15(n, d, dev):
    """64 centres x3, 4096 sub-centres around them (spread 1.5), unit
    noise."""
    g = torch.Generator(device=dev).manual_seed(0)
    top = torch.randn(64, d, generator=g, device=dev) * 3
    sub = top[torch.randint(0, 64, (4096,), generator=g, device=dev)] \
        + torch.randn(4096, d, generator=g, device=dev) * 1.5
    x = sub[torch.randint(0, 4096, (n,), generator=g, device=dev)]
    x += torch.randn(n, d, generator=g, device=dev)
    return x


SETS = {"flat20": flat20, "two15": two15}


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def timed(dev, fn):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return time.perf_counter() - t0, out


def med(xs):
    return f"{np.median(xs):.3f} [{min(xs):.3f}..{max(xs):.3f}]"


def seeds_of(n, B, dev):
    gen = torch.Generator().manual_seed(3)
    r = torch.zeros(B, n)
    for b in range(B):
        r[b, torch.randint(0, n, (10,), generator=gen)] = 0.1
    return r.to(dev)


def rank_round(pull, g, inv, B, sweeps, dev):
    """One timed run of `sweeps` ping-pong launches on vertex-major
    buffers, as graph_radio._solve allocates them: ms per sweep."""
    n = g.n
    r = torch.empty(n, B, device=dev).t()
    r.copy_(seeds_of(n, B, dev))
    q = (r * inv.unsqueeze(0)).t().contiguous().t()
    q2 = torch.empty(n, B, device=dev).t()
    p = torch.empty(n, B, device=dev).t()
    sync(dev)
    t0 = time.perf_counter()
    for _ in range(sweeps):
        pull(q, p, q2, r, inv, g.idx, g.s, g.in_off, g.in_edge, None,
             C.RADIO_ALPHA)
        q, q2 = q2, q
    sync(dev)
    return (time.perf_counter() - t0) / sweeps * 1e3


def relax_round(relax, pg, B, sweeps, dev):
    """The same for path_relax, as scripts/path_graph_bench.py times it."""
    n = pg.n
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(0, n, (B,), generator=gen).to(dev)
    a = torch.full((n, B), float("inf"), device=dev).t()
    a[torch.arange(B, device=dev), src] = 0.0
    b = torch.full((n, B), -1, dtype=torch.int32, device=dev).t()
    c = torch.empty(n, B, device=dev).t()
    d = torch.empty(n, B, dtype=torch.int32, device=dev).t()
    changed = torch.zeros(B, dtype=torch.int32, device=dev)
    sync(dev)
    t0 = time.perf_counter()
    for _ in range(sweeps):
        relax(a, b, c, d, pg.idx, pg.w, pg.in_off, pg.in_edge, None, changed)
        a, b, c, d = c, d, a, b
    sync(dev)
    return (time.perf_counter() - t0) / sweeps * 1e3


def one_set(name, n, d, dev, args):
    x = SETS[name](n, d, dev)
    t_index, index = timed(dev, lambda: IVFIndex.build(
        x, metric="euclidean", storage="f16", device=dev))
    ids = [f"t{i}" for i in range(n)]
    sim = SimilarityEngine(index, ids)
    print(f"\nvariant {name}: index build {t_index:.2f} s, "
          f"nlist={index.nlist}")
    t_first, g = timed(dev, sim.rank_graph)
    t_second, pg = timed(dev, sim.path_graph)
    lens = (g.in_off[1:] - g.in_off[:-1]).float().cpu()
    print(f"first request: rank_graph() {t_first:.2f} s (neighbor_graph "
          f"k={C.PATH_GRAPH_NEIGHBOURS} + affinities + reverse lists), then "
          f"path_graph() from the same kNN build {t_second:.2f} s; filled "
          f"slots {int((g.idx >= 0).sum())}, in-degree mean "
          f"{float(lens.mean()):.1f}, max {int(lens.max())}")

    pull = R._kernels(g.device)
    relax, _ = G._kernels(g.device)
    fused = pull is not R.pull_reference
    t_deg, deg = timed(dev, lambda: R.degrees(g))
    t_deg, deg = timed(dev, lambda: R.degrees(g))
    inv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    print(f"degree pass (one plain rank_pull launch, warm): "
          f"{t_deg * 1e3:.3f} ms; isolated vertices "
          f"{int((deg == 0).sum())}")

    T = R.sweep_count(C.RADIO_ALPHA, C.RADIO_TOLERANCE, C.RADIO_MAX_SWEEPS)
    for B in (1, 2, 8):
        if fused:
            # alternate the two kernels round by round: one call, one
            # machine, the same graph and the same number of legs
            tr, tp = [], []
            for r in range(args.rounds + 1):
                a = rank_round(pull, g, inv, B, 20, dev)
                b = relax_round(relax, pg, B, 20, dev)
                if r:
                    tr.append(a)
                    tp.append(b)
            print(f"sweep B={B} rank_pull      : {med(tr)} ms "
                  f"({args.rounds} rounds of 20 sweeps, alternating)")
            print(f"sweep B={B} path_relax     : {med(tp)} ms")
        tt = [rank_round(R.pull_reference, g, inv, B, 2, dev)
              for _ in range(max(args.rounds // 2, 2) + 1)][1:]
        print(f"sweep B={B} pull_reference : {med(tt)} ms (on {dev})")

    for B in (1, 2):
        r = seeds_of(n, B, dev)
        t = []
        for rnd in range(args.rounds + 1):
            dt, p = timed(dev, lambda: R.personalized_pagerank(
                g, r, C.RADIO_ALPHA, T))
            if rnd:
                t.append(dt * 1e3)
        print(f"personalized_pagerank B={B}, T={T} sweeps + degree pass: "
              f"{med(t)} ms; mass {p.sum(dim=1).tolist()}")
    if fused:
        # results must not change: the kernel's p_T against the f64
        # statement at this size
        r = seeds_of(n, 2, dev)
        keep = R._kernels
        try:
            R._kernels = lambda _dev: R.pull_reference
            want = R.personalized_pagerank(g, r, C.RADIO_ALPHA, T)
        finally:
            R._kernels = keep
        got = R.personalized_pagerank(g, r, C.RADIO_ALPHA, T)
        nz = want > 0
        rel = ((got - want).abs()[nz] / want[nz]).max()
        print(f"kernel p_T against pull_reference p_T: largest relative "
              f"difference {float(rel):.2e} over {int(nz.sum())} nonzero "
              f"entries; zero pattern equal: "
              f"{bool(((got > 0) == nz).all())}")

    gen = torch.Generator().manual_seed(11)
    for engine in ("graph", "centroid"):
        lat, used_all = [], set()
        for rnd in range(args.rounds + 1):
            pick = torch.randint(0, n, (10,), generator=gen).tolist()
            w = (0.5 ** torch.arange(10.0)).tolist()
            dt, (items, used) = timed(dev, lambda: R.graph_radio(
                sim, [ids[i] for i in pick], w, n=20, engine=engine))
            if rnd:
                lat.append(dt * 1e3)
            used_all.add((used, len(items)))
        print(f"graph_radio(10 weighted seeds, n=20, engine={engine}) warm: "
              f"{med(lat)} ms; (engine used, tracks): {sorted(used_all)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--sets", default="flat20,two15")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times say "
                         "nothing about the GPU")
    args = ap.parse_args()
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("graph_radio_bench measures on the GPU; none found")
    where = torch.cuda.get_device_name(0) if dev != "cpu" else "cpu"
    T = R.sweep_count(C.RADIO_ALPHA, C.RADIO_TOLERANCE, C.RADIO_MAX_SWEEPS)
    print(f"== {args.n} x {args.dim}, f16 euclidean index, "
          f"k={C.PATH_GRAPH_NEIGHBOURS}, alpha={C.RADIO_ALPHA}, T={T}, {where}")
    for name in args.sets.split(","):
        one_set(name, args.n, args.dim, dev, args)


if __name__ == "__main__":
    main()
