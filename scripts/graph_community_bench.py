"""Graph communities on a resident f16 index: time per sweep of the fused
community_move kernel, of its torch statement on the same GPU and of one
rank_pull sweep at B = 1 on the same graph (the yardstick: the same
adjacency, read once), a whole communities solve (levels, sweeps,
communities, size quartiles), and the community_playlists task end to end
on a catalogue stored in SQLite. Output of the runs at 1M x 200:
profiles/r13_graph_community.txt.

    python scripts/graph_community_bench.py [n] [--sets flat20,two15]
"""

import argparse
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
sys.path.insert(0, __file__.rsplit("/", 1)[0])

from path_graph_bench import SETS, med, sync, timed  # noqa: E402

from audiomuse_amd import config as C  # noqa: E402
from audiomuse_amd.engines import graph_community as GC  # noqa: E402
from audiomuse_amd.engines import graph_radio as R  # noqa: E402
from audiomuse_amd.engines.similarity import SimilarityEngine  # noqa: E402
from audiomuse_amd.index.ivf import IVFIndex  # noqa: E402


def say(*a):
    print(*a, flush=True)


def move_round(move, g, deg, label, tot, A, sweeps, dev):
    """One timed run of `sweeps` launches from the same labels, down and
    up alternating: ms per sweep."""
    out = torch.empty_like(label)
    sync(dev)
    t0 = time.perf_counter()
    for s in range(sweeps):
        move(label, out, tot, deg, g.idx, g.w, g.in_off, g.in_edge, A, 64,
             s % 2 == 1)
    sync(dev)
    return (time.perf_counter() - t0) / sweeps * 1e3, out


def rank_round(pull, g, sweeps, dev):
    """The same for rank_pull at B = 1, as graph_radio._solve runs it."""
    n = g.n
    deg = R.degrees(g)
    inv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    r = torch.zeros(n, 1, device=dev).t()
    r[0, :10] = 0.1
    q = (r * inv.unsqueeze(0)).t().contiguous().t()
    q2 = torch.empty(n, 1, device=dev).t()
    p = torch.empty(n, 1, device=dev).t()
    sync(dev)
    t0 = time.perf_counter()
    for _ in range(sweeps):
        pull(q, p, q2, r, inv, g.idx, g.s, g.in_off, g.in_edge, None,
             C.RADIO_ALPHA)
        q, q2 = q2, q
    sync(dev)
    return (time.perf_counter() - t0) / sweeps * 1e3


def task_end_to_end(x, dev, args):
    """community_playlists on the first task_n tracks, stored in SQLite
    with their vectors as the analysis stores them."""
    from audiomuse_amd.analysis.index import (AUDIO_INDEX, build_audio_index,
                                              load_ivf_engine)
    from audiomuse_amd.cluster.tasks import community_playlists
    from audiomuse_amd.db import connect, write_txn
    from audiomuse_amd.db.schema import init_db

    m = min(args.task_n, x.shape[0])
    vec = x[:m].float().cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        conn = connect("sqlite:///" + tmp + "/bench.db")
        init_db(conn)
        t0 = time.perf_counter()
        moods = C.MOOD_LABELS
        with write_txn(conn):
            conn.executemany(
                "INSERT INTO score (item_id, title, author, mood_vector, "
                "other_features) VALUES (?,?,?,?,?)",
                ((f"t{i}", f"Song {i}", f"Artist {i % 5000}",
                  '{"%s": 0.8}' % moods[i % len(moods)], "{}")
                 for i in range(m)))
            conn.executemany(
                "INSERT INTO embedding (item_id, embedding) VALUES (?,?)",
                ((f"t{i}", vec[i].tobytes()) for i in range(m)))
        t_store = time.perf_counter() - t0
        t_index, _ = timed(dev, lambda: build_audio_index(conn, device=dev))
        engine = load_ivf_engine(conn, AUDIO_INDEX, device=dev)
        t_task, rep = timed(dev, lambda: community_playlists(
            conn, engine, top_n=args.top_n))
        t_warm, rep = timed(dev, lambda: community_playlists(
            conn, engine, top_n=args.top_n))
        rows = conn.execute("SELECT COUNT(*) FROM playlist WHERE "
                            "kind='community'").fetchone()[0]
        conn.close()
    say(f"community_playlists on {m} stored tracks (store {t_store:.1f} s, "
        f"index {t_index:.1f} s, neither counted): first call {t_task:.2f} s "
        f"(kNN graph + solve + catalogue load + playlists), second call on "
        f"the same engine {t_warm:.2f} s (solve kept); "
        f"{rep['communities']} communities, {rep['playlists']} playlists "
        f"({rows} rows), largest {rep['largest']}")


def one_set(name, n, d, dev, args):
    x = SETS[name](n, d, dev)
    t_index, index = timed(dev, lambda: IVFIndex.build(
        x, metric="euclidean", storage="f16", device=dev))
    sim = SimilarityEngine(index, [f"t{i}" for i in range(n)])
    say(f"\nvariant {name}: index build {t_index:.2f} s, nlist={index.nlist}")
    t_first, g = timed(dev, sim.community_graph)
    t_rank, rg = timed(dev, sim.rank_graph)
    lens = (g.in_off[1:] - g.in_off[:-1]).float().cpu()
    say(f"first request: community_graph() {t_first:.2f} s (neighbor_graph "
        f"k={C.PATH_GRAPH_NEIGHBOURS}, connect="
        f"{bool(C.PATH_GRAPH_CONNECT)}, + weights + reverse lists), "
        f"rank_graph() from the same build {t_rank:.2f} s; table k="
        f"{g.idx.shape[1]}, filled slots {int((g.idx >= 0).sum())}, "
        f"in-degree mean {float(lens.mean()):.1f}, max {int(lens.max())}")

    move = GC._kernel(g)
    fused = move is not GC.move_reference
    deg = GC.degrees(g)
    two_m = int(deg.sum())
    A = GC.RESOLUTION_UNIT * two_m
    say(f"max_deg {int(deg.max())}, two_m {two_m}, 64 * max_deg * two_m = "
        f"2^{np.log2(64.0 * int(deg.max()) * two_m):.1f}")
    # two label states: singletons (sweep 0) and the end of local moving
    end, sweeps, capped = GC.local_move(g, C.COMMUNITY_RESOLUTION,
                                        C.COMMUNITY_MAX_SWEEPS)
    states = {"singletons": torch.arange(n, dtype=torch.int32, device=dev),
              f"after {sweeps} sweeps": end}
    pull = R._kernels(rg.device)
    for what, label in states.items():
        tot = torch.zeros_like(deg).index_add_(0, label.long(), deg)
        if fused:
            tk, tr = [], []
            for r in range(args.rounds + 1):
                a, got = move_round(move, g, deg, label, tot, A, 20, dev)
                b = rank_round(pull, rg, 20, dev)
                if r:
                    tk.append(a)
                    tr.append(b)
            say(f"sweep community_move ({what}): {med(tk)} ms "
                f"({args.rounds} rounds of 20 sweeps, alternating with)")
            say(f"sweep rank_pull B=1              : {med(tr)} ms "
                f"(community_move / rank_pull = "
                f"{np.median(tk) / np.median(tr):.2f})")
        tt = []
        for r in range(max(args.rounds // 2, 2) + 1):
            a, want = move_round(GC.move_reference, g, deg, label, tot, A, 2,
                                 dev)
            if r:
                tt.append(a)
        say(f"sweep move_reference ({what}): {med(tt)} ms (on {dev})"
            + (f"; kernel is {np.median(tt) / np.median(tk):.1f} x faster, "
               f"results equal: {bool(torch.equal(got, want))}"
               if fused else ""))

    for res in (C.COMMUNITY_RESOLUTION,):
        t = []
        for rnd in range(3):
            dt, (labels, rep) = timed(dev, lambda: GC.communities(
                g, res, C.COMMUNITY_MAX_SWEEPS, C.COMMUNITY_MAX_LEVELS))
            if rnd:
                t.append(dt)
        sizes = torch.bincount(labels.long()).float()
        qs = torch.quantile(sizes, torch.tensor([0.25, 0.5, 0.75],
                                                device=sizes.device)).tolist()
        say(f"communities(resolution={res}): {med(t)} s; "
            f"{rep['communities']} communities, modularity "
            f"{rep['modularity']:.4f}, sizes min/q1/median/q3/max "
            f"{int(sizes.min())}/{qs[0]:.0f}/{qs[1]:.0f}/{qs[2]:.0f}/"
            f"{int(sizes.max())}")
        for lv in rep["levels"]:
            say(f"  level: {lv}")
    if args.task_n > 0:
        task_end_to_end(x, dev, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--sets", default="flat20,two05,two15,manifold3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--task-n", type=int, default=100_000,
                    help="tracks stored in SQLite for the task (0 = skip)")
    ap.add_argument("--top-n", type=int, default=C.TOP_N_PLAYLISTS)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times say "
                         "nothing about the GPU")
    args = ap.parse_args()
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("graph_community_bench measures on the GPU; none "
                         "found")
    where = torch.cuda.get_device_name(0) if dev != "cpu" else "cpu"
    say(f"== {args.n} x {args.dim}, f16 euclidean index, "
        f"k={C.PATH_GRAPH_NEIGHBOURS}, resolution={C.COMMUNITY_RESOLUTION}, "
        f"levels={C.COMMUNITY_WEIGHT_LEVELS}, {where}")
    for name in args.sets.split(","):
        one_set(name, args.n, args.dim, dev, args)


if __name__ == "__main__":
    main()
