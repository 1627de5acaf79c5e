"""The graph song path (PATH_ENGINE=graph) on a resident f16 index: graph
build on the first request, sweeps to convergence, time per sweep of the
fused kernel and of its torch statement for 1 and 8 legs, host Dijkstra
on the same graph, warm find_path latency, and the tracks-per-path
distribution for exponents 1 and 2. Output of the runs at 1M x 200 on the
three sets of profiles/r5_knn_graph.txt and on a connected 3-d manifold:
profiles/r8_graph_path.txt.

    python scripts/path_graph_bench.py [n] [--sets flat20,two05,two15,manifold3]
"""

import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.engines import graph_path as G  # noqa: E402
from audiomuse_amd.engines.path import find_path_ex  # noqa: E402
from audiomuse_amd.engines.similarity import SimilarityEngine  # noqa: E402
from audiomuse_amd.index.ivf import IVFIndex  # noqa: E402


def flat20(n, d, dev):
    """20 centres x3, unit noise."""
    g = torch.Generator(device=dev).manual_seed(0)
    top = torch.randn(20, d, generator=g, device=dev) * 3
    x = top[torch.randint(0, 20, (n,), generator=g, device=dev)]
    x += torch.randn(n, d, generator=g, device=dev)
    return x


def two_level(spread):
    def make(n, d, dev):
        """64 centres x3, 4096 sub-centres around them, unit noise."""
        g = torch.Generator(device=dev).manual_seed(0)
        top = torch.randn(64, d, generator=g, device=dev) * 3
        sub = top[torch.randint(0, 64, (4096,), generator=g, device=dev)] \
            + torch.randn(4096, d, generator=g, device=dev) * spread
        x = sub[torch.randint(0, 4096, (n,), generator=g, device=dev)]
        x += torch.randn(n, d, generator=g, device=dev)
        return x
    return make


def manifold3(n, d, dev):
    """A 3-d cube (side 10) under a random linear map into d dimensions,
    noise 0.01: one connected neighbour graph with long paths."""
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.rand(n, 3, generator=g, device=dev) * 10
    a = torch.randn(3, d, generator=g, device=dev) / d ** 0.5
    return z @ a + torch.randn(n, d, generator=g, device=dev) * 0.01


SETS = {"flat20": flat20, "two05": two_level(0.5), "two15": two_level(1.5),
        "manifold3": manifold3}


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


def sweep_ms(relax, g, B, sweeps_per_round, rounds, dev):
    """Median time of one sweep: `rounds` timed runs of `sweeps_per_round`
    ping-pong launches each, after one warm-up run."""
    n = g.n
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(0, n, (B,), generator=gen).to(dev)
    # vertex-major memory, as graph_path.solve allocates it
    d0 = torch.full((n, B), float("inf"), device=dev).t()
    d0[torch.arange(B, device=dev), src] = 0.0
    p0 = torch.full((n, B), -1, dtype=torch.int32, device=dev).t()
    d1 = torch.empty(n, B, device=dev).t()
    p1 = torch.empty(n, B, dtype=torch.int32, device=dev).t()
    changed = torch.zeros(B, dtype=torch.int32, device=dev)
    out = []
    for r in range(rounds + 1):
        a, b, c, d = d0, p0, d1, p1
        sync(dev)
        t0 = time.perf_counter()
        for _ in range(sweeps_per_round):
            relax(a, b, c, d, g.idx, g.w, g.in_off, g.in_edge, None, changed)
            a, b, c, d = c, d, a, b
        sync(dev)
        if r:
            out.append((time.perf_counter() - t0) / sweeps_per_round * 1e3)
    return out


def host_dijkstra(g, srcs, dist_gpu):
    idx = g.idx.cpu().numpy()
    w = g.w.cpu().numpy().astype(np.float64)
    n, k = idx.shape
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        print("host Dijkstra: scipy does not import; not measured")
        return
    rows = np.repeat(np.arange(n), k)[idx.reshape(-1) >= 0]
    cols = idx.reshape(-1)[idx.reshape(-1) >= 0]
    a = csr_matrix((w.reshape(-1)[idx.reshape(-1) >= 0], (rows, cols)),
                   shape=(n, n))
    times = []
    worst = 0.0
    for b, s in enumerate(srcs):
        t0 = time.perf_counter()
        d64 = dijkstra(a, directed=False, indices=int(s))
        times.append(time.perf_counter() - t0)
        d32 = dist_gpu[b].cpu().numpy().astype(np.float64)
        fin = np.isfinite(d64)
        assert np.array_equal(fin, np.isfinite(d32))
        worst = max(worst, float(np.max(
            np.abs(d32[fin] - d64[fin]) / np.maximum(d64[fin], 1e-300))))
    print(f"host Dijkstra (scipy.sparse.csgraph, f64, one source, {n} "
          f"vertices): {med(times)} s; largest relative difference of the "
          f"f32 sweep distances: {worst:.2e}")


def one_set(name, n, d, dev, args):
    x = SETS[name](n, d, dev)
    t_index, index = timed(dev, lambda: IVFIndex.build(
        x, metric="euclidean", storage="f16", device=dev))
    ids = [f"t{i}" for i in range(n)]
    sim = SimilarityEngine(index, ids)
    print(f"\nvariant {name}: index build {t_index:.2f} s, "
          f"nlist={index.nlist}")

    t_first, g = timed(dev, sim.path_graph)
    deg = (g.in_off[1:] - g.in_off[:-1]).float().cpu()
    print(f"first request: path_graph() {t_first:.2f} s "
          f"(neighbor_graph k={C.PATH_GRAPH_NEIGHBOURS} + weights + reverse "
          f"lists); filled slots {int((g.idx >= 0).sum())}, in-degree mean "
          f"{float(deg.mean()):.1f}, p99.9 "
          f"{float(torch.quantile(deg[:2_000_000], 0.999)):.0f}, "
          f"max {int(deg.max())}")
    per_vertex = (g.idx.shape[1] + float(deg.mean())) * 12
    print(f"traffic estimate per sweep and leg: (k + in-degree) x 12 B = "
          f"{per_vertex:.0f} B per vertex, {per_vertex * n / 1e6:.0f} MB")

    gen = torch.Generator().manual_seed(11)
    pairs = torch.randint(0, n, (args.pairs, 2), generator=gen).tolist()
    pos, dists = sim.neighbor_graph(C.PATH_GRAPH_NEIGHBOURS)
    near_pairs = []
    for exponent in (1.0, 2.0):
        ge = G.PathGraph.from_knn(pos, dists, exponent)
        for kind in ("random", "same component"):
            lens, sweeps, none, reach = [], [], 0, []
            for s in range(0, len(pairs), 8):
                chunk = [list(p) for p in pairs[s:s + 8]]
                if kind == "same component":
                    # targets drawn among the vertices the source reaches
                    dist, _, _ = G.solve(ge, [p[0] for p in chunk])
                    fin = torch.isfinite(dist)
                    reach += fin.float().mean(dim=1).tolist()
                    pick = torch.rand(fin.shape, generator=gen).to(dev)
                    dst = (pick * fin).argmax(dim=1).tolist()
                    chunk = [[p[0], t] for p, t in zip(chunk, dst)]
                    if exponent == 2.0:
                        near_pairs += chunk
                paths, _, sw = G.shortest_paths(ge, [p[0] for p in chunk],
                                                [p[1] for p in chunk])
                sweeps.append(sw)
                none += sum(p is None for p in paths)
                lens += [len(p) for p in paths if p is not None]
            if lens:
                q = np.percentile(lens, [0, 25, 50, 75, 100]).tolist()
            else:
                q = [float("nan")] * 5
            extra = ""
            if reach:
                extra = (f"; share of the catalogue a source reaches: median "
                         f"{np.median(reach):.4f}, max {max(reach):.4f}")
            print(f"exponent {exponent:.0f}, {len(pairs)} {kind} pairs: "
                  f"{none} without a path; tracks per path "
                  f"min/p25/median/p75/max "
                  f"{q[0]:.0f}/{q[1]:.0f}/{q[2]:.0f}/{q[3]:.0f}/{q[4]:.0f}; "
                  f"sweeps run per batch of 8 (groups of {G.SWEEP_GROUP}): "
                  f"{sorted(set(sweeps))}{extra}")
    del ge, pos, dists

    # exact sweep counts: reference loop with one flag read per sweep
    relax, _ = G._kernels(g.device)
    for B in (1, 8):
        srcs = [p[0] for p in pairs[:B]]
        dist = torch.full((n, B), float("inf"), device=dev).t()
        dist[torch.arange(B, device=dev), torch.tensor(srcs, device=dev)] = 0.0
        pred = torch.full((n, B), -1, dtype=torch.int32, device=dev).t()
        d1 = torch.empty(n, B, device=dev).t()
        p1 = torch.empty(n, B, dtype=torch.int32, device=dev).t()
        changed = torch.zeros(B, dtype=torch.int32, device=dev)
        last = [0] * B
        for sweep in range(1, n + 2):
            changed.zero_()
            relax(dist, pred, d1, p1, g.idx, g.w, g.in_off, g.in_edge, None,
                  changed)
            dist, d1, pred, p1 = d1, dist, p1, pred
            ch = changed.tolist()
            if not any(ch):
                break
            last = [sweep if c else v for c, v in zip(ch, last)]
        print(f"B={B}: last sweep that changed a leg: {last}")
        if B == 8:
            dist8 = dist.clone()
            srcs8 = srcs
    del dist, pred, d1, p1

    for B in (1, 8):
        if relax is not G.relax_reference:
            t = sweep_ms(relax, g, B, 20, args.rounds, dev)
            print(f"sweep B={B} fused kernel   : {med(t)} ms "
                  f"({args.rounds} rounds of 20 sweeps)")
        t = sweep_ms(G.relax_reference, g, B, 2, max(args.rounds // 2, 2), dev)
        print(f"sweep B={B} relax_reference: {med(t)} ms (on {dev})")

    # the whole solve for 8 sources under other group sizes
    keep = G.SWEEP_GROUP
    srcs = [p[0] for p in pairs[:8]]
    try:
        for group in (1, 2, 4, 8, 16):
            G.SWEEP_GROUP = group
            t = []
            for r in range(args.rounds + 1):
                dt, (_, _, sw) = timed(dev, lambda: G.solve(g, srcs))
                if r:
                    t.append(dt * 1e3)
            print(f"solve B=8, flags read every {group:2d} sweeps: {med(t)} ms, "
                  f"{sw} sweeps run")
    finally:
        G.SWEEP_GROUP = keep

    lat, used_all = [], set()
    for a, b in near_pairs[:args.rounds + 1]:
        t, (items, used) = timed(dev, lambda: find_path_ex(
            sim, ids[a], ids[b], length=25, engine="graph"))
        lat.append(t * 1e3)
        used_all.add((used, len(items)))
    print(f"find_path(engine=graph, length=25), same-component pairs, warm: "
          f"{med(lat[1:])} ms; "
          f"(engine used, tracks): {sorted(used_all)}")
    lat = []
    for a, b in near_pairs[:4]:
        t, _ = timed(dev, lambda: find_path_ex(
            sim, ids[a], ids[b], length=25, engine="waypoint"))
        lat.append(t * 1e3)
    print(f"find_path(engine=waypoint, length=25) warm: {med(lat[1:])} ms")
    host_dijkstra(g, srcs8[:args.host_sources], dist8)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--sets", default="flat20,two05,two15,manifold3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--host-sources", type=int, default=3)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times say "
                         "nothing about the GPU")
    args = ap.parse_args()
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("path_graph_bench measures on the GPU; none found")
    where = torch.cuda.get_device_name(0) if dev != "cpu" else "cpu"
    print(f"== {args.n} x {args.dim}, f16 euclidean index, "
          f"k={C.PATH_GRAPH_NEIGHBOURS}, {where}")
    for name in args.sets.split(","):
        one_set(name, args.n, args.dim, dev, args)


if __name__ == "__main__":
    main()
