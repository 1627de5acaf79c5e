"""Graph song path on the torch reference (CPU): distances against an
independent float64 Dijkstra, predecessor chains, hand-built graphs, the
allowed mask, thin(), find_path with engine/scope/via, and /api/path."""

import functools
import heapq

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import graph_path as G
from audiomuse_amd.engines import projection as P
from audiomuse_amd.engines.path import find_path, find_path_ex
from audiomuse_amd.engines.similarity import build_engine_from_matrix

INF = float("inf")


# -- the oracle ----------------------------------------------------------------


def _adjacency(g, allowed=None):
    """Symmetrised adjacency {v: [(u, weight as float)]} of a PathGraph,
    restricted to allowed vertices."""
    idx, w = g.idx.tolist(), g.w.double().tolist()
    ok = [True] * g.n if allowed is None else [bool(a) for a in allowed]
    adj = [[] for _ in range(g.n)]
    for v in range(g.n):
        for s, u in enumerate(idx[v]):
            if u >= 0 and ok[v] and ok[u]:
                adj[v].append((u, w[v][s]))
                adj[u].append((v, w[v][s]))
    return adj


def dijkstra(adj, src):
    """Heap Dijkstra in float64 (Python floats)."""
    dist = [INF] * len(adj)
    dist[src] = 0.0
    heap = [(0.0, src)]
    while heap:
        d, v = heapq.heappop(heap)
        if d > dist[v]:
            continue
        for u, wt in adj[v]:
            nd = d + wt
            if nd < dist[u]:
                dist[u] = nd
                heapq.heappush(heap, (nd, u))
    return dist


def _graph(pos, dists, exponent=2.0):
    return G.PathGraph.from_knn(torch.as_tensor(pos, dtype=torch.int64),
                                torch.as_tensor(dists, dtype=torch.float32),
                                exponent)


@functools.lru_cache(maxsize=None)
def _blob_graph(k):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1000, 16, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    d, i = P.knn_graph(x, k)
    return G.PathGraph.from_knn(i, d, 2.0)


@functools.lru_cache(maxsize=None)
def _twenty_centres_graph():
    g = torch.Generator().manual_seed(1)
    centres = torch.randn(20, 32, generator=g) * 3
    x = centres[torch.arange(2000) % 20] + torch.randn(2000, 32, generator=g)
    d, i = P.knn_graph(x, 15)
    return G.PathGraph.from_knn(i, d, 2.0)


@functools.lru_cache(maxsize=None)
def _solved(name):
    g = {"blob15": lambda: _blob_graph(15), "blob5": lambda: _blob_graph(5),
         "centres": _twenty_centres_graph}[name]()
    srcs = [0, 7, 501]
    dist, pred, sweeps = G.solve(g, srcs)
    adj = _adjacency(g)
    oracle = [dijkstra(adj, s) for s in srcs]
    return g, srcs, dist, pred, sweeps, adj, oracle


def _check_against_oracle(d32, d64, sweeps):
    d32 = np.asarray(d32, dtype=np.float64)
    d64 = np.asarray(d64, dtype=np.float64)
    fin = np.isfinite(d64)
    assert np.array_equal(np.isfinite(d32), fin)
    err = np.abs(d32[fin] - d64[fin])
    bound = sweeps * 2.0 ** -23 * d64[fin]
    print("max err", float(err.max()), "max rel",
          float((err / np.maximum(d64[fin], 1e-300)).max()),
          "bound rel", sweeps * 2.0 ** -23)
    assert np.all(err <= bound)
    return float(fin.mean())


# -- distances and chains --------------------------------------------------------


@pytest.mark.parametrize("name", ["blob15", "blob5", "centres"])
def test_distances_match_float64_dijkstra(name):
    g, srcs, dist, pred, sweeps, adj, oracle = _solved(name)
    for b in range(len(srcs)):
        reach = _check_against_oracle(dist[b].tolist(), oracle[b], sweeps)
        if name == "centres":
            assert reach < 0.5          # most vertices are unreachable
        else:
            assert reach == 1.0


@pytest.mark.parametrize("name", ["blob15", "blob5", "centres"])
def test_pred_chains(name):
    g, srcs, dist, pred, sweeps, adj, oracle = _solved(name)
    edge_w = {}
    idx, w = g.idx.tolist(), g.w
    for v in range(g.n):
        for s, u in enumerate(idx[v]):
            if u >= 0:
                edge_w.setdefault((v, u), []).append(w[v, s])
                edge_w.setdefault((u, v), []).append(w[v, s])
    for b, s in enumerate(srcs):
        p = pred[b].tolist()
        for t in range(0, g.n, 13):
            if not torch.isfinite(dist[b, t]):
                assert p[t] == -1
                continue
            chain = [t]
            while chain[-1] != s:
                assert len(chain) <= sweeps
                chain.append(p[chain[-1]])
            chain.reverse()
            acc = torch.zeros((), dtype=torch.float32)
            for a, c in zip(chain[:-1], chain[1:]):
                ws = edge_w[(a, c)]          # every hop is an edge
                # the hop's weight is the one that reproduces the next dist
                nxt = [acc + x for x in ws if (acc + x) == dist[b, c]]
                assert nxt, (a, c)
                acc = nxt[0]
            assert acc.view(torch.int32) == dist[b, t].view(torch.int32)


def test_shortest_paths_lists_and_dists():
    g, srcs, dist, pred, sweeps, adj, oracle = _solved("blob15")
    dsts = [500, 900, 3]
    paths, dists, sw = G.shortest_paths(g, srcs, dsts)
    assert sw == sweeps
    for b in range(3):
        assert paths[b][0] == srcs[b] and paths[b][-1] == dsts[b]
        assert len(set(paths[b])) == len(paths[b])
        assert dists[b] == dist[b, dsts[b]]
    g2 = _twenty_centres_graph()
    # vertices 0 and 1 lie in different clusters
    paths, dists, _ = G.shortest_paths(g2, [0, 0], [1, 20])
    assert paths[0] is None and dists[0] == INF
    assert paths[1] is not None and paths[1][0] == 0 and paths[1][-1] == 20


# -- hand-built graphs -------------------------------------------------------------


def test_diamond_tie_follows_enumeration_order():
    # 0 -> 1, 0 -> 2 (both 1.0); 1 -> 3, 2 -> 3 (both 1.0); 3 has no own
    # slots, so its candidates are its in-list, ascending edge id: the
    # edge from 1 comes first
    pos = [[1, 2], [3, -1], [3, -1], [-1, -1]]
    d = [[1.0, 1.0], [1.0, 0.0], [1.0, 0.0], [0.0, 0.0]]
    g = _graph(pos, d, 1.0)
    dist, pred, _ = G.solve(g, [0, 3])
    assert dist[0].tolist() == [0.0, 1.0, 1.0, 2.0]
    assert pred[0].tolist() == [-1, 0, 0, 1]
    # from 3: vertex 0 sees its own slots first, slot 0 (vertex 1) wins
    assert dist[1].tolist() == [2.0, 1.0, 1.0, 0.0]
    assert pred[1].tolist() == [1, 3, 3, -1]
    paths, dists, _ = G.shortest_paths(g, [0], [3])
    assert paths == [[0, 1, 3]] and dists.tolist() == [2.0]
    # swapped slots: own-slot order decides, not the vertex number
    g = _graph([[2, 1], [3, -1], [3, -1], [-1, -1]], d, 1.0)
    _, pred, _ = G.solve(g, [3])
    assert pred[0].tolist() == [2, 3, 3, -1]


def test_zero_weight_duplicates_make_no_cycle():
    # 1 and 2 are exact duplicates: zero-weight edges both ways
    pos = [[1], [2], [1], [2]]
    d = [[1.0], [0.0], [0.0], [1.0]]
    g = _graph(pos, d, 2.0)
    dist, pred, sweeps = G.solve(g, [0])
    assert dist[0].tolist() == [0.0, 1.0, 1.0, 2.0]
    assert pred[0].tolist() == [-1, 0, 1, 2]
    paths, dists, _ = G.shortest_paths(g, [0, 3], [3, 0])
    assert paths == [[0, 1, 2, 3], [3, 2, 1, 0]]
    assert dists.tolist() == [2.0, 2.0]


def test_empty_slot_row_and_non_finite_slots():
    pos = [[1, 2], [-1, -1], [0, 1]]
    d = [[1.0, INF], [INF, INF], [float("nan"), 0.5]]
    g = _graph(pos, d, 1.0)
    assert g.idx.tolist() == [[1, -1], [-1, -1], [-1, 1]]
    assert g.w.tolist() == [[1.0, 0.0], [0.0, 0.0], [0.0, 0.5]]
    assert g.in_off.tolist() == [0, 0, 2, 2]
    assert g.in_edge.tolist() == [0, 5]
    dist, pred, _ = G.solve(g, [0])
    assert dist[0].tolist() == [0.0, 1.0, 1.5]
    assert pred[0].tolist() == [-1, 0, 1]
    with pytest.raises(ValueError):
        _graph([[3, 1], [0, 2], [0, 1]], [[1.0] * 2] * 3)


def test_single_vertex_and_source_equals_target():
    g = _graph([[-1]], [[INF]])
    assert g.n == 1 and g.in_edge.numel() == 0
    paths, dists, sweeps = G.shortest_paths(g, [0], [0])
    assert paths == [[0]] and dists.tolist() == [0.0] and sweeps == 0
    dist, pred, _ = G.solve(g, [0])
    assert dist.tolist() == [[0.0]] and pred.tolist() == [[-1]]
    g = _blob_graph(15)
    paths, dists, sweeps = G.shortest_paths(g, [5, 9], [5, 9])
    assert paths == [[5], [9]] and dists.tolist() == [0.0, 0.0]
    assert sweeps == 0
    # next to a real leg the trivial leg is still one track
    paths, dists, sweeps = G.shortest_paths(g, [5, 9], [5, 10])
    assert paths[0] == [5] and dists[0] == 0.0 and sweeps > 0
    with pytest.raises(ValueError):
        G.shortest_paths(g, [], [])
    with pytest.raises(ValueError):
        G.shortest_paths(g, [0] * 9, [1] * 9)
    with pytest.raises(ValueError):
        G.shortest_paths(g, [0], [1000])


def test_relax_changed_flag_is_only_ever_set():
    g = _blob_graph(5)
    n = g.n
    dist = torch.full((2, n), INF)
    dist[0, 0] = 0.0                      # leg 1 has no source: never improves
    pred = torch.full((2, n), -1, dtype=torch.int32)
    out_d, out_p = torch.empty_like(dist), torch.empty_like(pred)
    changed = torch.tensor([0, 7], dtype=torch.int32)
    G.relax_reference(dist, pred, out_d, out_p, g.idx, g.w, g.in_off,
                      g.in_edge, None, changed)
    assert changed.tolist() == [1, 7]
    assert torch.isinf(out_d[1]).all() and (out_p[1] == -1).all()


# -- allowed mask ------------------------------------------------------------------


def test_allowed_mask_matches_oracle_on_induced_subgraph():
    g = _blob_graph(15)
    gen = torch.Generator().manual_seed(5)
    allowed = (torch.rand(g.n, generator=gen) < 0.6).to(torch.uint8)
    allowed[0] = 1
    dist, pred, sweeps = G.solve(g, [0], allowed)
    off = allowed == 0
    assert torch.isinf(dist[0][off]).all() and (pred[0][off] == -1).all()
    oracle = dijkstra(_adjacency(g, allowed.tolist()), 0)
    _check_against_oracle(dist[0].tolist(), oracle, sweeps)
    targets = [t for t in range(1, g.n, 97) if allowed[t]][:4]
    paths, _, _ = G.shortest_paths(g, [0] * len(targets), targets, allowed)
    for p in paths:
        if p is not None:
            assert all(allowed[v] for v in p)
    # a masked source or target has no path
    t = int(torch.nonzero(off)[0])
    paths, dists, _ = G.shortest_paths(g, [0, t, t], [t, 0, t], allowed)
    assert paths == [None, None, None] and torch.isinf(dists).all()


# -- thin ----------------------------------------------------------------------------


def test_thin():
    tracks = list("abcdefghij")
    assert G.thin(tracks, ["a", "j"], 10) == tracks
    assert G.thin(tracks, ["a", "j"], 12) == tracks
    out = G.thin(tracks, ["a", "j"], 9)           # len = length + 1
    assert len(out) == 9 and out[0] == "a" and out[-1] == "j"
    assert out == sorted(out) and len(set(out)) == 9
    out = G.thin(tracks, ["a", "e", "j"], 4)      # m = 1: the middle interior
    assert out == ["a", "e", "f", "j"]
    assert G.thin(tracks, ["a", "e", "j"], 3) == ["a", "e", "j"]   # m = 0
    assert G.thin(tracks, ["a", "e", "j"], 2) == ["a", "e", "j"]   # m < 0
    for length in range(2, 10):
        out = G.thin(tracks, ["a", "j"], length)
        assert len(out) == length and len(set(out)) == length
        assert out == sorted(out) and out[0] == "a" and out[-1] == "j"
        inter = tracks[1:-1]
        m = length - 2
        want = [inter[int((j + 0.5) * len(inter) // m)] for j in range(m)]
        assert out[1:-1] == want


# -- find_path -----------------------------------------------------------------------


def _catalogue(n=400, d=16, seed=0, n_artists=20, metric="angular",
               matrix=None, scope_fn=None):
    rng = np.random.default_rng(seed)
    x = matrix if matrix is not None else \
        rng.standard_normal((n, d)).astype(np.float32)
    n = x.shape[0]
    ids = [f"s{i}" for i in range(n)]
    meta = {f"s{i}": {"title": f"T{i}", "author": f"artist{i % n_artists}"}
            for i in range(n)}
    eng = build_engine_from_matrix(x, ids, metric=metric, meta_fn=meta.get,
                                   scope_fn=scope_fn)
    return eng, ids, meta


@pytest.fixture(scope="module")
def manifold_engine():
    """Points along a noisy curve: graph paths between far ends are long."""
    rng = np.random.default_rng(2)
    t = np.sort(rng.uniform(0, 3.0, 300))
    x = np.stack([np.cos(t), np.sin(t), 0.3 * t], axis=1)
    x = np.concatenate([x, 0.01 * rng.standard_normal((300, 5))], axis=1)
    return _catalogue(matrix=x.astype(np.float32), n_artists=300)


def _neighbours(eng):
    g = eng.path_graph()
    nb = set()
    for v, row in enumerate(g.idx.tolist()):
        for u in row:
            if u >= 0:
                nb.add((v, u))
                nb.add((u, v))
    return nb


def test_default_engine_is_waypoint():
    eng, ids, _ = _catalogue()
    assert C.PATH_ENGINE == "waypoint"
    a = find_path(eng, "s0", "s100", length=8)
    b, used = find_path_ex(eng, "s0", "s100", length=8, engine="waypoint")
    assert a == b and used == "waypoint"
    assert a[0]["item_id"] == "s0" and a[-1]["item_id"] == "s100"
    with pytest.raises(ValueError):
        find_path(eng, "s0", "s100", engine="bogus")


def test_graph_engine_every_step_is_a_neighbour_hop(manifold_engine, monkeypatch):
    eng, ids, _ = manifold_engine
    monkeypatch.setattr(C, "PATH_FIX_SIZE", False)
    items, used = find_path_ex(eng, "s0", "s299", length=500, engine="graph")
    assert used == "graph"
    got = [p["item_id"] for p in items]
    assert got[0] == "s0" and got[-1] == "s299"
    assert 4 < len(got) < 500 and len(set(got)) == len(got)
    nb = _neighbours(eng)
    for a, b in zip(got[:-1], got[1:]):
        assert (eng.pos[a], eng.pos[b]) in nb
    # distance: to the previous returned track, from the stored vectors
    assert items[0]["distance"] == 0.0
    va, vb = eng.vector_for_id(got[0]), eng.vector_for_id(got[1])
    want = 1.0 - float(torch.dot(va, vb) / (va.norm() * vb.norm()))
    assert items[1]["distance"] == pytest.approx(want, abs=1e-6)


def test_graph_engine_length(manifold_engine, monkeypatch):
    eng, ids, _ = manifold_engine
    monkeypatch.setattr(C, "PATH_FIX_SIZE", False)
    full = [p["item_id"] for p in
            find_path(eng, "s0", "s299", length=500, engine="graph")]
    short = [p["item_id"] for p in
             find_path(eng, "s0", "s299", length=5, engine="graph")]
    assert len(short) == 5 and short[0] == "s0" and short[-1] == "s299"
    assert short == [t for t in full if t in set(short)]     # thinned, in order
    # with the backfill on, a short graph path is filled to the length
    monkeypatch.setattr(C, "PATH_FIX_SIZE", True)
    n = len(full) + 3
    filled, used = find_path_ex(eng, "s0", "s299", length=n, engine="graph")
    got = [p["item_id"] for p in filled]
    assert used == "graph" and len(got) == n and len(set(got)) == n
    assert got[0] == "s0" and got[-1] == "s299"


def test_graph_engine_artist_cap(monkeypatch):
    rng = np.random.default_rng(2)
    t = np.sort(rng.uniform(0, 3.0, 300))
    x = np.stack([np.cos(t), np.sin(t), 0.3 * t], axis=1).astype(np.float32)
    eng, ids, meta = _catalogue(matrix=x, n_artists=3)
    monkeypatch.setattr(C, "PATH_FIX_SIZE", False)
    free = find_path(eng, "s0", "s299", length=500, engine="graph")
    capped = find_path(eng, "s0", "s299", length=500, engine="graph",
                       max_per_artist=2)
    assert len(free) > 10
    counts = {}
    for p in capped[1:-1]:
        a = meta[p["item_id"]]["author"]
        counts[a] = counts.get(a, 0) + 1
    assert counts and max(counts.values()) <= 2
    free_ids = [p["item_id"] for p in free]
    assert [p["item_id"] for p in capped] == \
        [t for t in free_ids if t in {p["item_id"] for p in capped}]


def test_graph_engine_falls_back_without_a_path():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((60, 8)).astype(np.float32) * 0.05
    b = rng.standard_normal((60, 8)).astype(np.float32) * 0.05
    a[:, 0] += 1.0
    b[:, 1] += 1.0
    eng, ids, _ = _catalogue(matrix=np.concatenate([a, b]))
    items, used = find_path_ex(eng, "s0", "s100", length=6, engine="graph")
    assert used == "waypoint"
    assert items == find_path(eng, "s0", "s100", length=6, engine="waypoint")
    # inside one cluster the graph engine answers
    items, used = find_path_ex(eng, "s0", "s30", length=6, engine="graph")
    assert used == "graph"


def test_dot_metric_falls_back():
    eng, ids, _ = _catalogue(metric="dot")
    assert eng.path_graph() is None
    items, used = find_path_ex(eng, "s0", "s100", length=6, engine="graph")
    assert used == "waypoint"
    assert items[0]["item_id"] == "s0" and items[-1]["item_id"] == "s100"


@pytest.mark.parametrize("engine", ["graph", "waypoint"])
def test_via_stops(manifold_engine, engine):
    eng, ids, _ = manifold_engine
    via2 = ["s150"]
    items, used = find_path_ex(eng, "s0", "s299", length=12, engine=engine,
                               via=via2)
    got = [p["item_id"] for p in items]
    assert used == engine and len(got) == 12 and len(set(got)) == 12
    assert got[0] == "s0" and got[-1] == "s299" and "s150" in got
    via8 = [f"s{i}" for i in (40, 80, 120, 160, 200, 240, 280)]
    items = find_path(eng, "s0", "s299", length=20, engine=engine, via=via8)
    got = [p["item_id"] for p in items]
    assert len(got) == 20 and len(set(got)) == 20
    assert [t for t in got if t in set(via8)] == via8
    with pytest.raises(ValueError):
        find_path(eng, "s0", "s299", length=20, engine=engine,
                  via=via8 + ["s290"])
    assert find_path(eng, "s0", "s299", engine=engine, via=["nope"]) == []


def test_scope_masks_the_graph_path(manifold_engine):
    _, ids, _ = manifold_engine
    rng = np.random.default_rng(2)
    t = np.sort(rng.uniform(0, 3.0, 300))
    x = np.stack([np.cos(t), np.sin(t), 0.3 * t], axis=1).astype(np.float32)
    even = [f"s{i}" for i in range(0, 300, 2)]
    calls = []

    def scope_fn(name):
        calls.append(name)
        return even if name == "even" else []

    eng, ids, _ = _catalogue(matrix=x, scope_fn=scope_fn, n_artists=300)
    for engine in ("graph", "waypoint"):
        items = find_path(eng, "s0", "s298", length=10, engine=engine,
                          scope="even")
        got = [p["item_id"] for p in items]
        assert got[0] == "s0" and got[-1] == "s298" and len(got) == 10
        assert all(t in set(even) for t in got)
        assert find_path(eng, "s0", "s299", engine=engine, scope="even") == []
        assert find_path(eng, "s0", "s298", engine=engine, scope="even",
                         via=["s3"]) == []
    assert calls.count("even") <= 2      # the mask and the RowScope, cached


def test_path_graph_is_cached_until_the_index_moves(monkeypatch):
    eng, ids, _ = _catalogue()
    calls = []
    real = eng.index.knn_graph

    def counting(*a, **kw):
        calls.append(a)
        return real(*a, **kw)

    monkeypatch.setattr(eng.index, "knn_graph", counting)
    find_path(eng, "s0", "s100", length=6, engine="graph")
    g1 = eng.path_graph()
    find_path(eng, "s3", "s50", length=6, engine="graph")
    assert len(calls) == 1 and eng.path_graph() is g1
    assert calls[0][0] == C.PATH_GRAPH_NEIGHBOURS
    v = eng.index.vector_for_id(7).clone()
    eng.index.remove(torch.tensor([7]))
    eng.index.add(v.unsqueeze(0), torch.tensor([7]))
    g2 = eng.path_graph()
    assert len(calls) == 2 and g2 is not g1
    assert eng.path_graph() is g2 and len(calls) == 2


# -- web -----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def path_client(tmp_path_factory):
    from audiomuse_amd.analysis.index import build_audio_index
    from audiomuse_amd.db import connect, write_txn
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding
    from audiomuse_amd.web.app import create_app

    url = "sqlite:///" + str(tmp_path_factory.mktemp("gpath") / "web.db")
    conn = connect(url)
    init_db(conn)
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 3.0, 200))
    ids = []
    for i in range(200):
        iid = f"fp_4{'%050x' % i}"
        ids.append(iid)
        emb = 0.01 * rng.standard_normal(200)
        emb[:3] += (np.cos(t[i]), np.sin(t[i]), 0.3 * t[i])
        save_track_analysis_and_embedding(
            conn, iid, title=f"Song {i}", author=f"Artist {i}",
            album=f"Album {i % 40}", tempo=100.0, energy=0.5, key="C",
            scale="major", duration=200.0, mood_vector={}, other_features={},
            embedding=emb.astype(np.float32))
    build_audio_index(conn)
    mapped = ids[::2]
    with write_txn(conn):
        for k, iid in enumerate(mapped):
            conn.execute(
                "INSERT OR REPLACE INTO track_server_map "
                "(provider_id, server_id, item_id) VALUES (?, 'half', ?)",
                (f"hf-{k}", iid))
    app = create_app(url, device="cpu", auth_disabled=True)
    app.testing = True
    with app.test_client() as client:
        yield client, ids, mapped
    conn.close()


def test_web_path_engines(path_client):
    client, ids, mapped = path_client
    r = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&length=8"
                   "&engine=graph")
    assert r.status_code == 200 and r.headers["X-Path-Engine"] == "graph"
    body = r.json
    assert isinstance(body, list) and len(body) == 8
    assert body[0]["item_id"] == ids[0] and body[-1]["item_id"] == ids[198]
    assert all(b["title"] and "provider_id" not in b for b in body)
    plain = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&length=8")
    assert plain.status_code == 200
    assert plain.headers["X-Path-Engine"] == "waypoint"
    r = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&engine=bogus")
    assert r.status_code == 400
    via = ",".join(ids[20:180:20])                      # 8 via stops: 9 legs
    r = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&via={via}")
    assert r.status_code == 400


def test_web_path_server_and_via(path_client):
    client, ids, mapped = path_client
    pid_of = {iid: f"hf-{k}" for k, iid in enumerate(mapped)}
    for engine in ("graph", "waypoint"):
        r = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&length=8"
                       f"&engine={engine}&server=half")
        assert r.status_code == 200, engine
        assert r.headers["X-Path-Engine"] == engine
        body = r.json
        assert len(body) == 8
        for b in body:
            assert b["provider_id"] == pid_of[b["item_id"]]
    r = client.get(f"/api/path?start={ids[0]}&end={ids[199]}&server=half")
    assert r.status_code == 404                         # end not on the server
    r = client.get(f"/api/path?start={ids[0]}&end={ids[198]}&length=9"
                   f"&engine=graph&via={ids[60]},{ids[120]}")
    assert r.status_code == 200
    got = [b["item_id"] for b in r.json]
    assert len(got) == 9 and got[0] == ids[0] and got[-1] == ids[198]
    assert got.index(ids[60]) < got.index(ids[120])
