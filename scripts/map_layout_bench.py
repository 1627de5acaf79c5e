"""The two layout engines of the 2-D maps on one graph (MAP_LAYOUT_ENGINE
torch | fused): time of umap_project and of its epoch loop, peak device
memory, in-degree figures of the graph and neighbour preservation of the
layouts, then build_song_map with either engine. Output of the runs at
4000, 100k and 1M points: profiles/r6_map_layout.txt.

    python scripts/map_layout_bench.py [n] [--rounds 3] [--no-song-map]
"""

import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.analysis import index as aindex  # noqa: E402
from audiomuse_amd.engines import projection as P  # noqa: E402

ENGINES = ("torch", "fused")


def two05(n, d, dev):
    """The set two05 of profiles/r5_knn_graph.txt: 64 centres x3, 4096
    sub-centres around them at spread 0.5, unit noise."""
    g = torch.Generator(device=dev).manual_seed(0)
    top = torch.randn(64, d, generator=g, device=dev) * 3
    sub = top[torch.randint(0, 64, (4096,), generator=g, device=dev)] \
        + torch.randn(4096, d, generator=g, device=dev) * 0.5
    x = sub[torch.randint(0, 4096, (n,), generator=g, device=dev)]
    x += torch.randn(n, d, generator=g, device=dev)
    return x


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def peak_gib(dev):
    return torch.cuda.max_memory_allocated() / 2 ** 30 if dev != "cpu" else 0.0


class Stopwatch:
    """Wraps a function of a module so that its synchronised wall time is
    added up per call."""

    def __init__(self, module, name, dev):
        self.module, self.name, self.dev = module, name, dev
        self.real = getattr(module, name)
        self.seconds, self.last_args = 0.0, None
        setattr(module, name, self)

    def __call__(self, *args, **kwargs):
        sync(self.dev)
        t0 = time.perf_counter()
        out = self.real(*args, **kwargs)
        sync(self.dev)
        self.seconds += time.perf_counter() - t0
        self.last_args = args
        return out

    def take(self):
        s, self.seconds = self.seconds, 0.0
        return s

    def restore(self):
        setattr(self.module, self.name, self.real)


def neighbour_preservation(nbrs, emb, rows, block=2000, cols=250_000):
    """Mean over the sampled rows of the share of a row's k graph
    neighbours that are among its k nearest points of the layout."""
    n, k = nbrs.shape
    kept = 0.0
    for s in range(0, rows.numel(), block):
        r = rows[s:s + block]
        best_d = torch.full((r.numel(), k), float("inf"), device=emb.device)
        best_i = torch.full((r.numel(), k), -1, dtype=torch.long,
                            device=emb.device)
        for c in range(0, n, cols):
            d = torch.cdist(emb[r], emb[c:c + cols])
            own = (r >= c) & (r < c + cols)
            d[own.nonzero().view(-1), r[own] - c] = float("inf")
            kk = min(k, d.shape[1])
            top = d.topk(kk, dim=1, largest=False)
            cat_d = torch.cat([best_d, top.values], dim=1)
            cat_i = torch.cat([best_i, top.indices + c], dim=1)
            sel = cat_d.topk(k, dim=1, largest=False)
            best_d, best_i = sel.values, cat_i.gather(1, sel.indices)
        hit = (best_i.unsqueeze(2) == nbrs[r].unsqueeze(1)).any(dim=1)
        kept += float(hit.double().sum())
    return kept / (rows.numel() * k)


def engines_on_one_graph(x, dev, rounds, sample):
    n = x.shape[0]
    sync(dev)
    t0 = time.perf_counter()
    knn = aindex._ivf_map_graph(x)
    sync(dev)
    if knn is None:
        raise SystemExit("the IVF graph left rows short of neighbours")
    print(f"neighbour graph (_ivf_map_graph, k={knn[1].shape[1]}): "
          f"{time.perf_counter() - t0:.2f} s")

    loops = {"torch": Stopwatch(P, "_torch_layout", dev),
             "fused": Stopwatch(P, "_run_fused_epochs", dev)}
    total = {e: [] for e in ENGINES}
    loop = {e: [] for e in ENGINES}
    peak = {e: 0.0 for e in ENGINES}
    emb = {}
    # one untimed fused run first: it loads the code object
    P.umap_project(x, seed=0, knn=knn, engine="fused", epochs=2)
    loops["fused"].take()
    for _ in range(rounds):
        for e in ENGINES:
            if dev != "cpu":
                torch.cuda.reset_peak_memory_stats()
            sync(dev)
            t0 = time.perf_counter()
            emb[e] = P.umap_project(x, seed=0, knn=knn, engine=e)
            sync(dev)
            total[e].append(time.perf_counter() - t0)
            loop[e].append(loops[e].take())
            peak[e] = max(peak[e], peak_gib(dev))
    in_off = loops["fused"].last_args[3]
    for w in loops.values():
        w.restore()

    for e in ENGINES:
        print(f"engine {e:5s}: umap_project {np.median(total[e]):.3f} s "
              f"(min {min(total[e]):.3f}, max {max(total[e]):.3f}), epoch "
              f"loop {np.median(loop[e]):.3f} s (min {min(loop[e]):.3f}, max "
              f"{max(loop[e]):.3f}); {rounds} interleaved rounds, 200 epochs; "
              f"peak device memory {peak[e]:.2f} GiB")
    print(f"epoch loop torch / fused (medians): "
          f"{np.median(loop['torch']) / np.median(loop['fused']):.1f}x; "
          f"fused epoch {np.median(loop['fused']) / 200 * 1e3:.3f} ms")
    deg = (in_off[1:] - in_off[:-1]).float()
    print(f"in-degree of the sampled-edge lists: mean {float(deg.mean()):.1f}, "
          f"p99.9 {float(torch.quantile(deg.cpu(), 0.999)):.0f}, "
          f"max {int(deg.max())}")
    g = torch.Generator().manual_seed(1)
    rows = torch.randperm(n, generator=g)[:min(sample, n)].to(x.device)
    nbrs = knn[1].to(x.device)
    for e in ENGINES:
        print(f"engine {e:5s}: neighbour preservation "
              f"{neighbour_preservation(nbrs, emb[e], rows):.4f} "
              f"({rows.numel()} sampled rows)")


def song_map(x, dev):
    """build_song_map with the embeddings handed to the function in place
    of the SQL load, MAP_KNN_SOURCE=ivf, one run per engine."""
    n = x.shape[0]
    ids = [f"t{i}" for i in range(n)]
    mat = x.cpu().numpy()
    stored = {}
    real_load, real_store = aindex.load_all_embeddings, aindex.store_index_blob
    aindex.load_all_embeddings = lambda conn, table: (ids, mat)
    aindex.store_index_blob = \
        lambda conn, name, blob, meta=None: stored.update(size=len(blob))
    knn_source, engine = C.MAP_KNN_SOURCE, C.MAP_LAYOUT_ENGINE
    C.MAP_KNN_SOURCE = "ivf"
    layout = Stopwatch(P, "umap_project", dev)
    try:
        for e in ENGINES:
            C.MAP_LAYOUT_ENGINE = e
            if dev != "cpu":
                torch.cuda.reset_peak_memory_stats()
            sync(dev)
            t0 = time.perf_counter()
            aindex.build_song_map(None, device=dev)
            sync(dev)
            dt = time.perf_counter() - t0
            print(f"MAP_LAYOUT_ENGINE={e}: build_song_map {dt:.1f} s for {n} "
                  f"tracks (umap_project: {layout.take():.1f} s), peak device "
                  f"memory {peak_gib(dev):.2f} GiB, blob "
                  f"{stored['size'] / 2 ** 20:.0f} MiB")
    finally:
        layout.restore()
        C.MAP_KNN_SOURCE, C.MAP_LAYOUT_ENGINE = knn_source, engine
        aindex.load_all_embeddings = real_load
        aindex.store_index_blob = real_store


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=20_000)
    ap.add_argument("--no-song-map", action="store_true")
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times say "
                         "nothing about the GPU")
    args = ap.parse_args()
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("map_layout_bench measures on the GPU; none found")
    x = two05(args.n, args.dim, dev)
    where = torch.cuda.get_device_name(0) if dev != "cpu" else "cpu"
    print(f"== {args.n} x {args.dim} (set two05), k=15, seed 0, {where}")
    engines_on_one_graph(x, dev, args.rounds, args.sample)
    if not args.no_song_map:
        song_map(x, dev)


if __name__ == "__main__":
    main()
