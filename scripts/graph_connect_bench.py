"""The connected graph (PATH_GRAPH_CONNECT) on a resident f16 index, on the
sets of scripts/path_graph_bench.py: components before and after, rounds,
bridges and extra slots; seconds for the labels and for each
foreign-neighbour scan round next to the knn_graph build of the same set;
one graph_label_pull sweep against its torch statement and against
path_relax at B = 1; path_relax and rank_pull on the widened graph against
the unwidened one; and the share of uniform random pairs the graph song
path answers with the setting off and on. Output of the runs at 1M x 200:
profiles/r10_graph_connect.txt.

    python scripts/graph_connect_bench.py [n] [--sets flat20,two05,two15,manifold3]
"""

import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
sys.path.insert(0, __file__.rsplit("/", 1)[0])

from path_graph_bench import SETS, med, sweep_ms, sync, timed  # noqa: E402

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.engines import graph_connect as GC  # noqa: E402
from audiomuse_amd.engines import graph_path as G  # noqa: E402
from audiomuse_amd.engines import graph_radio as R  # noqa: E402
from audiomuse_amd.engines.path import find_path_ex  # noqa: E402
from audiomuse_amd.engines.similarity import SimilarityEngine  # noqa: E402
from audiomuse_amd.index.ivf import IVFIndex  # noqa: E402


def say(*a):
    print(*a, flush=True)


def label_sweep_ms(pull, idx, in_off, in_edge, sweeps_per_round, rounds, dev):
    """Median time of one label sweep from label[v] = v: `rounds` timed
    runs of `sweeps_per_round` ping-pong launches, after one warm-up."""
    n = idx.shape[0]
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = []
    for r in range(rounds + 1):
        a = torch.arange(n, dtype=torch.int32, device=dev)
        b = torch.empty_like(a)
        sync(dev)
        t0 = time.perf_counter()
        for _ in range(sweeps_per_round):
            pull(a, b, idx, in_off, in_edge, changed)
            a, b = b, a
        sync(dev)
        if r:
            out.append((time.perf_counter() - t0) / sweeps_per_round * 1e3)
    return out


def rank_sweep_ms(graph, sweeps, rounds, dev):
    """Median time per sweep of personalized_pagerank (B = 1, `sweeps`
    sweeps and the degree pass)."""
    restart = torch.zeros(1, graph.n, device=dev)
    restart[0, 0] = 1.0
    out = []
    for r in range(rounds + 1):
        dt, _ = timed(dev, lambda: R.personalized_pagerank(
            graph, restart, 0.85, sweeps))
        if r:
            out.append(dt / sweeps * 1e3)
    return out


def exact_sweeps(pull, idx, in_off, in_edge, dev):
    """Sweeps until the first one that changes nothing, one flag read per
    sweep."""
    n = idx.shape[0]
    a = torch.arange(n, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for sweep in range(1, n + 2):
        changed.zero_()
        pull(a, b, idx, in_off, in_edge, changed)
        a, b = b, a
        if not int(changed[0]):
            return sweep - 1
    return n


def pairs_answered(sim, ids, pairs, dev):
    """(share answered by the graph engine, tracks per shortest path,
    warm latencies in ms)."""
    used_graph, lat = 0, []
    for i, (a, b) in enumerate(pairs):
        t, (items, used) = timed(dev, lambda: find_path_ex(
            sim, ids[a], ids[b], length=25, engine="graph"))
        if i:                        # the first request pays the build
            lat.append(t * 1e3)
        used_graph += used == "graph"
    # tracks per path before thinning / backfill to the requested length
    graph = sim.path_graph()
    lens = []
    for s in range(0, len(pairs), 8):
        chunk = pairs[s:s + 8]
        paths, _, _ = G.shortest_paths(graph, [p[0] for p in chunk],
                                       [p[1] for p in chunk])
        lens += [len(p) for p in paths if p is not None]
    return used_graph / len(pairs), lens, lat


def one_set(name, n, d, dev, args):
    x = SETS[name](n, d, dev)
    t_index, index = timed(dev, lambda: IVFIndex.build(
        x, metric="euclidean", storage="f16", device=dev))
    ids = [f"t{i}" for i in range(n)]
    sim = SimilarityEngine(index, ids)
    say(f"\nvariant {name}: index build {t_index:.2f} s, nlist={index.nlist}")
    k = C.PATH_GRAPH_NEIGHBOURS
    t_knn, (pos, dists) = timed(dev, lambda: sim.neighbor_graph(k))
    say(f"neighbor_graph(k={k}): {t_knn:.2f} s")

    t_con, (pos2, dists2, rep) = timed(dev, lambda: GC.connect(
        pos, dists, index, C.PATH_GRAPH_BRIDGE_CANDIDATES,
        C.PATH_GRAPH_BRIDGE_ROUNDS))
    say(f"connect(candidates={C.PATH_GRAPH_BRIDGE_CANDIDATES}, max_rounds="
        f"{C.PATH_GRAPH_BRIDGE_ROUNDS}): {t_con:.2f} s "
        f"({t_con / t_knn:.2f} x the knn_graph build)")
    say(f"  components before {rep['components_before']} (largest "
        f"{rep['largest_before']} = "
        f"{rep['largest_before'] / n:.4f} of the catalogue), after "
        f"{rep['components_after']}; rounds {rep['rounds']}, bridges "
        f"{rep['bridges']} {rep['bridges_per_round']}, extra slots "
        f"{rep['extra_slots']}, without vector {rep['without_vector']}")
    say("  labels per labelling (s): "
        + ", ".join(f"{t:.3f}" for t in rep["label_seconds"])
        + f"; sweeps run (groups of {GC.SWEEP_GROUP}): {rep['label_sweeps']}")
    say("  foreign-neighbour scan + contraction per round (s): "
        + (", ".join(f"{t:.3f}" for t in rep["scan_seconds"]) or "none"))

    # one label sweep: kernel, torch statement, path_relax at B = 1
    idx, in_off, in_edge = GC.adjacency(pos, dists)
    pull = GC._kernel(idx.device)
    say(f"label sweeps to the fixed point (exact): "
        f"{exact_sweeps(pull, idx, in_off, in_edge, dev)}")
    if pull is not GC.label_pull_reference:
        t = label_sweep_ms(pull, idx, in_off, in_edge, 20, args.rounds, dev)
        say(f"sweep graph_label_pull      : {med(t)} ms "
            f"({args.rounds} rounds of 20 sweeps)")
    t = label_sweep_ms(GC.label_pull_reference, idx, in_off, in_edge, 2,
                       max(args.rounds // 2, 2), dev)
    say(f"sweep label_pull_reference  : {med(t)} ms (on {dev})")

    plain = G.PathGraph.from_knn(pos, dists, C.PATH_GRAPH_EXPONENT)
    wide = G.PathGraph.from_knn(pos2, dists2, C.PATH_GRAPH_EXPONENT)
    relax, _ = G._kernels(plain.device)
    for B in (1, 8):
        tp = sweep_ms(relax, plain, B, 20, args.rounds, dev)
        tw = sweep_ms(relax, wide, B, 20, args.rounds, dev)
        say(f"sweep path_relax B={B}: k={plain.idx.shape[1]} {med(tp)} ms; "
            f"widened k={wide.idx.shape[1]} {med(tw)} ms "
            f"({np.median(tw) / np.median(tp):.3f} x)")
    del plain, wide
    rp = R.RankGraph.from_knn(pos, dists, C.RADIO_BANDWIDTH)
    rw = R.RankGraph.from_knn(pos2, dists2, C.RADIO_BANDWIDTH)
    tp = rank_sweep_ms(rp, 20, args.rounds, dev)
    tw = rank_sweep_ms(rw, 20, args.rounds, dev)
    say(f"sweep rank_pull B=1 (20 sweeps + degree pass): k={rp.idx.shape[1]} "
        f"{med(tp)} ms; widened k={rw.idx.shape[1]} {med(tw)} ms "
        f"({np.median(tw) / np.median(tp):.3f} x)")
    del rp, rw, pos, dists, pos2, dists2

    gen = torch.Generator().manual_seed(11)
    pairs = torch.randint(0, n, (args.pairs, 2), generator=gen).tolist()
    keep = C.PATH_GRAPH_CONNECT
    try:
        for on in (False, True):
            C.PATH_GRAPH_CONNECT = on
            share, lens, lat = pairs_answered(sim, ids, pairs, dev)
            q = (np.percentile(lens, [0, 50, 100]).tolist() if lens
                 else [float("nan")] * 3)
            say(f"find_path(engine=graph, length=25), {len(pairs)} uniform "
                f"random pairs, PATH_GRAPH_CONNECT={'on' if on else 'off'}: "
                f"answered by the graph engine {share:.3f}; tracks per shortest "
                f"path min/median/max {q[0]:.0f}/{q[1]:.0f}/{q[2]:.0f}; "
                f"warm latency {med(lat)} ms")
    finally:
        C.PATH_GRAPH_CONNECT = keep


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--sets", default="flat20,two05,two15,manifold3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times say "
                         "nothing about the GPU")
    args = ap.parse_args()
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("graph_connect_bench measures on the GPU; none found")
    where = torch.cuda.get_device_name(0) if dev != "cpu" else "cpu"
    say(f"== {args.n} x {args.dim}, f16 euclidean index, "
        f"k={C.PATH_GRAPH_NEIGHBOURS}, {where}")
    for name in args.sets.split(","):
        one_set(name, args.n, args.dim, dev, args)


if __name__ == "__main__":
    main()
