"""Graph radio (engines/graph_radio.py) on the CPU: the torch statement of
the PageRank sweep against a dense f64 statement and the closed form, mass,
independent legs, the allowed mask, the multigraph rule, the engine on a
catalogue of two tastes and the region between them, its fallbacks, the
shared kNN build, the web routes and the sonic_fingerprint task."""

import functools

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import graph_radio as R
from audiomuse_amd.engines import projection as P
from audiomuse_amd.engines.similarity import build_engine_from_matrix

ALPHA = 0.85
T = R.sweep_count(ALPHA, 1e-3, 200)


def three_clusters(seed=0):
    """(x (490, 16) unit vectors, labels (490,) in {0: A, 1: B, 2: C}): 150
    points each around e0 (A), e1 (B) and their normalised midpoint (C),
    and 20 bridge points along each of the segments A-C and C-B."""
    g = torch.Generator().manual_seed(seed)
    e0, e1 = torch.eye(16)[0], torch.eye(16)[1]
    mid = (e0 + e1) / (e0 + e1).norm()
    parts = [c + 0.35 * torch.randn(150, 16, generator=g) / 4
             for c in (e0, e1, mid)]
    t = torch.linspace(0, 1, 22)[1:-1].unsqueeze(1)
    for a, b in ((e0, mid), (mid, e1)):
        parts.append((1 - t) * a + t * b
                     + 0.25 * torch.randn(20, 16, generator=g) / 4)
    x = torch.cat(parts)
    x = x / x.norm(dim=1, keepdim=True)
    labels = (x @ torch.stack([e0, e1, mid]).t()).argmax(dim=1)
    return x, labels


@functools.lru_cache(maxsize=None)
def cluster_graph():
    x, _ = three_clusters()
    d, i = P.knn_graph(x, 15)
    return R.RankGraph.from_knn(i, d, 1.0)


def random_graph(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g)
    idx[torch.rand(n, k, generator=g) < 0.3] = -1
    idx = idx.to(torch.int32)
    s = torch.where(idx >= 0, 0.05 + torch.rand(n, k, generator=g),
                    torch.zeros(n, k))
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    return R.RankGraph(idx, s, in_off, in_edge, n)


def dense(graph, allowed=None):
    """(P (n, n) f64 row-stochastic where deg > 0, deg (n,)): W[v, u] += s
    and W[u, v] += s for every filled slot, closed vertices cut out."""
    n = graph.n
    W = np.zeros((n, n))
    idx, s = graph.idx.numpy(), graph.s.numpy().astype(np.float64)
    for v in range(n):
        for j in range(idx.shape[1]):
            u = idx[v, j]
            if u >= 0:
                W[v, u] += s[v, j]
                W[u, v] += s[v, j]
    if allowed is not None:
        a = allowed.numpy().astype(bool)
        W[~a, :] = 0
        W[:, ~a] = 0
    deg = W.sum(axis=1)
    Pm = np.divide(W, deg[:, None], out=np.zeros_like(W),
                   where=deg[:, None] > 0)
    return Pm, deg


def power(Pm, r, alpha, sweeps):
    p = r.copy()
    for _ in range(sweeps):
        p = (1 - alpha) * r + alpha * (p @ Pm)
    return p


def restarts(n, B, seed, per_leg=4):
    g = torch.Generator().manual_seed(seed)
    r = torch.zeros(B, n)
    for b in range(B):
        at = torch.randperm(n, generator=g)[:min(per_leg, n)]
        w = 0.1 + torch.rand(at.numel(), generator=g)
        r[b, at] = w / w.sum()
    return r


# one f32 rounding each for deg, 1 / deg, p and q per sweep, first order
RTOL = T * 4 * 2.0 ** -23


@pytest.mark.parametrize("make", [lambda: random_graph(97, 5, 3),
                                  cluster_graph], ids=["random", "clusters"])
def test_pagerank_matches_dense_statement_and_closed_form(make):
    graph = make()
    n = graph.n
    r = restarts(n, 2, seed=1)
    Pm, deg = dense(graph)
    a = float(np.float32(ALPHA))
    got_deg = R.degrees(graph)
    np.testing.assert_allclose(got_deg.numpy(), deg, rtol=2.0 ** -23)
    for sweeps in (0, 1, 2, T):
        got = R.personalized_pagerank(graph, r, ALPHA, sweeps)
        assert got.shape == (2, n) and got.dtype == torch.float32
        want = power(Pm, r.numpy().astype(np.float64), a, sweeps)
        np.testing.assert_allclose(got.numpy(), want, rtol=RTOL, atol=1e-37)
    star = (1 - a) * r.numpy().astype(np.float64) @ np.linalg.inv(
        np.eye(n) - a * Pm)
    gap = np.abs(got.numpy() - star).sum(axis=1)
    assert (gap <= 2 * a ** T + RTOL).all()
    assert 2 * a ** T < 2e-3


def test_mass_is_kept_without_isolated_vertices():
    graph = cluster_graph()
    assert bool((R.degrees(graph) > 0).all())
    p = R.personalized_pagerank(graph, restarts(graph.n, 3, seed=2), ALPHA, T)
    assert bool((p >= 0).all())
    np.testing.assert_allclose(p.double().sum(dim=1).numpy(), 1.0, rtol=RTOL)


def test_legs_are_independent():
    graph = cluster_graph()
    r = restarts(graph.n, 3, seed=3)
    allp = R.personalized_pagerank(graph, r, ALPHA, T)
    for b in range(3):
        one = R.personalized_pagerank(graph, r[b:b + 1], ALPHA, T)
        assert torch.equal(one[0], allp[b])


def test_allowed_mask_is_the_induced_subgraph():
    graph = random_graph(120, 6, 8)
    n = graph.n
    allowed = (torch.rand(n, generator=torch.Generator().manual_seed(4))
               < 0.7).to(torch.uint8)
    r = restarts(n, 2, seed=5)
    r[:, allowed == 0] = 0
    r = r / r.sum(dim=1, keepdim=True)
    Pm, deg = dense(graph, allowed)
    np.testing.assert_allclose(R.degrees(graph, allowed).numpy(), deg,
                               rtol=2.0 ** -23)
    assert deg[(allowed == 0).numpy()].max() == 0
    got = R.personalized_pagerank(graph, r, ALPHA, T, allowed=allowed)
    assert bool((got[:, allowed == 0] == 0).all())
    want = power(Pm, r.numpy().astype(np.float64), float(np.float32(ALPHA)), T)
    np.testing.assert_allclose(got.numpy(), want, rtol=RTOL, atol=1e-37)
    # the same numbers from a graph that holds the allowed vertices only
    keep = torch.nonzero(allowed).reshape(-1)
    new = torch.full((n,), -1, dtype=torch.int64)
    new[keep] = torch.arange(keep.numel())
    sub_idx = graph.idx[keep].long()
    sub_idx = torch.where(sub_idx >= 0, new[sub_idx.clamp(min=0)], sub_idx)
    sub_idx = sub_idx.to(torch.int32)
    sub_s = torch.where(sub_idx >= 0, graph.s[keep], torch.zeros(1))
    in_off, in_edge = P.layout_reverse_lists(sub_idx,
                                             (sub_idx >= 0).to(torch.int32))
    sub = R.RankGraph(sub_idx, sub_s, in_off, in_edge, keep.numel())
    small = R.personalized_pagerank(sub, r[:, keep], ALPHA, T)
    np.testing.assert_allclose(got[:, keep].numpy(), small.numpy(),
                               rtol=RTOL, atol=1e-37)
    # restart mass on a closed vertex is dropped, not spread
    closed = int(torch.nonzero(allowed == 0)[0])
    r1 = torch.zeros(1, n)
    r1[0, closed] = 1.0
    assert not bool(R.personalized_pagerank(graph, r1, ALPHA, 3,
                                            allowed=allowed).any())


def test_self_slots_and_repeated_slots_are_more_candidates():
    # vertex 0: itself once and vertex 1 twice; vertex 1: vertex 0 (a mutual
    # neighbour); vertex 2: nobody, but nobody's neighbour either
    idx = torch.tensor([[0, 1, 1], [0, -1, -1], [-1, -1, -1]],
                       dtype=torch.int32)
    s = torch.tensor([[0.5, 0.25, 0.125], [1.0, 0, 0], [0, 0, 0]])
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    graph = R.RankGraph(idx, s, in_off, in_edge, 3)
    deg = R.degrees(graph)
    # 0: own 0.5 + 0.25 + 0.125, in-list: its self-slot 0.5 and 1's slot 1.0
    # 1: own 1.0, in-list: 0's two slots 0.25 + 0.125
    assert deg.tolist() == [2.375, 1.375, 0.0]
    Pm, ddeg = dense(graph)
    assert ddeg.tolist() == [2.375, 1.375, 0.0]
    r = torch.tensor([[0.25, 0.25, 0.5]])
    got = R.personalized_pagerank(graph, r, 0.5, 3)
    np.testing.assert_allclose(
        got.numpy(), power(Pm, r.numpy().astype(np.float64), 0.5, 3),
        rtol=1e-6)
    # the isolated seed keeps only its restart share
    assert got[0, 2].item() == pytest.approx(0.25)


def test_rank_graph_from_knn():
    pos = torch.tensor([[1, 2], [0, -1], [0, 1]])
    d = torch.tensor([[0.2, 0.4], [0.2, float("inf")], [0.4, 0.6]])
    g = R.RankGraph.from_knn(pos, d, 2.0)
    assert g.idx.tolist() == [[1, 2], [0, -1], [0, 1]]
    sigma = 2.0 * 0.4                  # median of 0.2 0.2 0.4 0.4 0.6
    want = torch.exp(-d / sigma)
    want[1, 1] = 0.0
    assert torch.allclose(g.s, want) and g.s.dtype == torch.float32
    assert g.in_off.tolist() == [0, 2, 4, 5]
    same = R.RankGraph.from_knn(pos, torch.zeros(3, 2), 1.0)
    assert same.s.tolist() == [[1, 1], [1, 0], [1, 1]]
    with pytest.raises(ValueError):
        R.RankGraph.from_knn(pos, d, 0.0)
    with pytest.raises(ValueError):
        R.RankGraph.from_knn(pos + 2, d, 1.0)


def test_sweep_count_and_argument_checks():
    assert T == 43 and R.sweep_count(0.85, 1e-3, 20) == 20
    assert R.sweep_count(0.0, 1e-3, 200) == 0
    assert R.sweep_count(0.5, 0.25, 200) == 2
    with pytest.raises(ValueError):
        R.sweep_count(1.0, 1e-3, 200)
    graph = cluster_graph()
    r = restarts(graph.n, 1, seed=0)
    with pytest.raises(ValueError):
        R.personalized_pagerank(graph, r, 1.0, 3)
    with pytest.raises(ValueError):
        R.personalized_pagerank(graph, r[:, :-1], ALPHA, 3)
    with pytest.raises(ValueError):
        R.personalized_pagerank(graph, r.expand(9, -1), ALPHA, 3)
    with pytest.raises(ValueError):
        R.personalized_pagerank(graph, r, ALPHA, 3,
                                allowed=torch.ones(3, dtype=torch.uint8))


# -- the engine ----------------------------------------------------------------


def cluster_engine(metric="angular", scope_fn=None, n_artists=490):
    x, labels = three_clusters()
    ids = [f"s{i}" for i in range(x.shape[0])]
    meta = {f"s{i}": {"title": f"T{i}", "author": f"artist{i % n_artists}"}
            for i in range(x.shape[0])}
    eng = build_engine_from_matrix(x.numpy(), ids, metric=metric,
                                   meta_fn=meta.get, scope_fn=scope_fn)
    return eng, ids, labels.tolist(), meta


@pytest.fixture(scope="module")
def clusters():
    return cluster_engine()


SEEDS = [f"s{i}" for i in (0, 1, 2, 3, 4, 150, 151, 152, 153, 154)]


def _labels(items, labels):
    return [labels[int(it["item_id"][1:])] for it in items]


def test_two_tastes_stay_two_tastes(clusters):
    eng, ids, labels, _ = clusters
    assert [labels[int(s[1:])] for s in SEEDS] == [0] * 5 + [1] * 5
    items, used = R.graph_radio(eng, SEEDS, n=20, engine="graph")
    assert used == "graph" and len(items) == 20
    got = _labels(items, labels)
    assert all(lab in (0, 1) for lab in got), got
    assert 0 in got and 1 in got
    assert not {it["item_id"] for it in items} & set(SEEDS)
    scores = [it["score"] for it in items]
    assert scores == sorted(scores, reverse=True) and scores[-1] > 0
    assert set(items[0]) == {"item_id", "score"}
    # the mean of the two tastes lies in neither
    items, used = R.graph_radio(eng, SEEDS, n=20, engine="centroid")
    assert used == "centroid" and len(items) == 20
    assert _labels(items, labels) == [2] * 20
    assert "distance" in items[0]


def test_default_engine_is_centroid(clusters):
    eng = clusters[0]
    assert C.SONIC_FINGERPRINT_ENGINE == "centroid"
    a = R.graph_radio(eng, SEEDS, n=10)
    assert a == R.graph_radio(eng, SEEDS, n=10, engine="centroid")
    assert a[1] == "centroid"
    with pytest.raises(ValueError):
        R.graph_radio(eng, SEEDS, n=10, engine="bogus")
    with pytest.raises(ValueError):
        R.graph_radio(eng, SEEDS, [1.0], n=10, engine="graph")


def test_weights_move_the_answer(clusters):
    eng, ids, labels, _ = clusters
    w = [1.0] * 5 + [0.0] * 5
    items, used = R.graph_radio(eng, SEEDS, w, n=20, engine="graph")
    assert used == "graph" and set(_labels(items, labels)) == {0}
    # weights that sum to nothing count as equal weights
    zero, _ = R.graph_radio(eng, SEEDS, [0.0] * 10, n=20, engine="graph")
    even, _ = R.graph_radio(eng, SEEDS, n=20, engine="graph")
    assert zero == even


def test_subtract_removes_a_taste(clusters):
    eng, ids, labels, _ = clusters
    sub = [f"s{i}" for i in (155, 156, 157, 158, 159)]
    assert all(labels[int(s[1:])] == 1 for s in sub)
    items, used = R.graph_radio(eng, SEEDS, subtract_ids=sub, n=20,
                                engine="graph")
    assert used == "graph" and len(items) == 20
    assert 1 not in _labels(items, labels)
    assert not {it["item_id"] for it in items} & set(sub)


def test_scope_and_artist_cap():
    x, _ = three_clusters()
    even = [f"s{i}" for i in range(0, x.shape[0], 2)]
    eng, ids, labels, meta = cluster_engine(
        scope_fn=lambda name: even if name == "even" else [], n_artists=7)
    items, used = R.graph_radio(eng, SEEDS, n=20, scope="even",
                                engine="graph")
    assert used == "graph" and len(items) == 20
    assert all(it["item_id"] in set(even) for it in items)
    assert all(lab in (0, 1) for lab in _labels(items, labels))
    capped, used = R.graph_radio(eng, SEEDS, n=12, max_per_artist=2,
                                 engine="graph")
    assert used == "graph" and len(capped) == 12
    counts = {}
    for it in capped:
        a = meta[it["item_id"]]["author"]
        counts[a] = counts.get(a, 0) + 1
    assert max(counts.values()) <= 2
    free, _ = R.graph_radio(eng, SEEDS, n=40, engine="graph")
    order = [it["item_id"] for it in free]
    kept = [it["item_id"] for it in capped]
    assert kept == [t for t in order if t in set(kept)]
    # no seed inside the scope: the centroid engine answers
    items, used = R.graph_radio(eng, ["s1", "s151"], n=5, scope="even",
                                engine="graph")
    assert used == "centroid" and len(items) == 5
    assert all(it["item_id"] in set(even) for it in items)


def test_fallbacks(clusters, caplog):
    eng, ids, labels, _ = clusters
    R._fallback_logged = False
    with caplog.at_level("WARNING"):
        items, used = R.graph_radio(eng, ["nope"], n=5, engine="graph")
        assert (items, used) == ([], "centroid")
        # unknown seeds are ignored next to known ones
        items, used = R.graph_radio(eng, ["nope"] + SEEDS, n=5,
                                    engine="graph")
        assert used == "graph" and len(items) == 5
        # more tracks asked for than the walk can reach
        items, used = R.graph_radio(eng, SEEDS, n=485, engine="graph")
        assert used == "centroid"
        dot, *_ = cluster_engine(metric="dot")
        assert dot.rank_graph() is None
        items, used = R.graph_radio(dot, SEEDS, n=5, engine="graph")
        assert used == "centroid" and len(items) == 5
    assert sum("graph radio" in r.message for r in caplog.records) == 1


def test_one_knn_build_serves_both_graphs(monkeypatch):
    eng, *_ = cluster_engine()
    calls = []
    real = eng.index.knn_graph

    def counting(*a, **kw):
        calls.append(a)
        return real(*a, **kw)

    monkeypatch.setattr(eng.index, "knn_graph", counting)
    rg = eng.rank_graph()
    pg = eng.path_graph()
    assert len(calls) == 1 and calls[0][0] == C.PATH_GRAPH_NEIGHBOURS
    assert eng.rank_graph() is rg and eng.path_graph() is pg
    assert torch.equal(rg.idx, pg.idx) and torch.equal(rg.in_edge, pg.in_edge)
    assert bool(((rg.s > 0) == (rg.idx >= 0)).all())
    v = eng.index.vector_for_id(7).clone()
    eng.index.remove(torch.tensor([7]))
    eng.index.add(v.unsqueeze(0), torch.tensor([7]))
    assert eng.path_graph() is not pg and eng.rank_graph() is not rg
    assert len(calls) == 2


# -- web -------------------------------------------------------------------------


def _radio_db(path):
    """A catalogue database of the three clusters with its audio index;
    every second track is on the server 'half'."""
    from audiomuse_amd.analysis.index import build_audio_index
    from audiomuse_amd.db import connect, write_txn
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding

    url = "sqlite:///" + str(path / "web.db")
    conn = connect(url)
    init_db(conn)
    x, labels = three_clusters()
    ids = []
    for i in range(x.shape[0]):
        iid = f"fp_4{'%050x' % i}"
        ids.append(iid)
        emb = np.zeros(200, dtype=np.float32)
        emb[:16] = x[i].numpy()
        save_track_analysis_and_embedding(
            conn, iid, title=f"Song {i}", author=f"Artist {i}",
            album=f"Album {i % 40}", tempo=100.0, energy=0.5, key="C",
            scale="major", duration=200.0, mood_vector={}, other_features={},
            embedding=emb)
    build_audio_index(conn)
    with write_txn(conn):
        for k, iid in enumerate(ids[::2]):
            conn.execute(
                "INSERT OR REPLACE INTO track_server_map "
                "(provider_id, server_id, item_id) VALUES (?, 'half', ?)",
                (f"hf-{k}", iid))
    return url, conn, ids, labels.tolist()


@pytest.fixture(scope="module")
def radio_client(tmp_path_factory):
    from audiomuse_amd.web.app import create_app

    url, conn, ids, labels = _radio_db(tmp_path_factory.mktemp("radio"))
    app = create_app(url, device="cpu", auth_disabled=True)
    app.testing = True
    with app.test_client() as client:
        yield client, ids, labels
    conn.close()


def _seed_query(ids):
    return "&".join(f"item_id={ids[i]}"
                    for i in (0, 2, 4, 6, 8, 150, 152, 154, 156, 158))


def test_web_radio(radio_client):
    client, ids, labels = radio_client
    lab = {iid: labels[i] for i, iid in enumerate(ids)}
    q = _seed_query(ids)
    r = client.get(f"/api/radio?{q}&n=20&engine=graph")
    assert r.status_code == 200 and r.headers["X-Radio-Engine"] == "graph"
    body = r.json
    assert len(body) == 20
    assert all("title" in b and b["score"] > 0 for b in body)
    assert any(b["title"] for b in body)
    assert all(lab[b["item_id"]] in (0, 1) for b in body)
    plain = client.get(f"/api/radio?{q}&n=20")
    assert plain.status_code == 200
    assert plain.headers["X-Radio-Engine"] == "centroid"
    assert all(lab[b["item_id"]] == 2 for b in plain.json)
    sub = "&".join(f"subtract={ids[i]}" for i in (160, 162, 164, 166, 168))
    r = client.get(f"/api/radio?{q}&{sub}&n=20&engine=graph")
    assert r.status_code == 200 and r.headers["X-Radio-Engine"] == "graph"
    assert all(lab[b["item_id"]] != 1 for b in r.json)
    w = "&".join(["weight=1"] * 5 + ["weight=0"] * 5)
    r = client.get(f"/api/radio?{q}&{w}&n=20&engine=graph")
    assert r.status_code == 200
    assert all(lab[b["item_id"]] == 0 for b in r.json)
    r = client.get(f"/api/radio?{q}&n=10&engine=graph&server=half")
    assert r.status_code == 200 and len(r.json) == 10
    assert r.headers["X-Radio-Engine"] == "graph"
    assert all(b["provider_id"].startswith("hf-") for b in r.json)
    assert client.get(f"/api/radio?{q}&n=10&engine=graph&server=nobody"
                      ).json == []
    assert client.get("/api/radio?n=5").status_code == 400
    assert client.get(f"/api/radio?{q}&engine=bogus").status_code == 400
    assert client.get(f"/api/radio?{q}&weight=1").status_code == 400
    assert client.get("/api/radio?item_id=nope&engine=graph"
                      ).status_code == 404
    assert client.get("/api/radio?item_id=nope").status_code == 404


def test_web_radio_without_an_index(tmp_path):
    from audiomuse_amd.db import connect
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.web.app import create_app

    url = "sqlite:///" + str(tmp_path / "empty.db")
    conn = connect(url)
    init_db(conn)
    conn.close()
    app = create_app(url, device="cpu", auth_disabled=True)
    app.testing = True
    with app.test_client() as client:
        assert client.get("/api/radio?item_id=a").status_code == 503


def test_web_sonic_fingerprint_engines(radio_client, monkeypatch):
    client, ids, labels = radio_client
    lab = {iid: labels[i] for i, iid in enumerate(ids)}
    q = _seed_query(ids)
    plain = client.get(f"/api/sonic_fingerprint?{q}&n=20")
    assert plain.status_code == 200 and len(plain.json) == 20
    assert "X-Radio-Engine" not in plain.headers
    assert all(lab[b["item_id"]] == 2 and "distance" in b for b in plain.json)
    same = client.get(f"/api/sonic_fingerprint?{q}&n=20&engine=centroid")
    assert same.json == plain.json
    r = client.get(f"/api/sonic_fingerprint?{q}&n=20&engine=graph")
    assert r.status_code == 200 and r.headers["X-Radio-Engine"] == "graph"
    assert len(r.json) == 20
    assert all(lab[b["item_id"]] in (0, 1) for b in r.json)
    # plays of taste B half a year old: the recency weights leave taste A
    now = 1.7e9
    monkeypatch.setattr("time.time", lambda: now)
    played = "&".join(f"played_at={now - (0 if i < 5 else 180 * 86400)}"
                      for i in range(10))
    r = client.get(f"/api/sonic_fingerprint?{q}&{played}&n=20&engine=graph")
    assert r.status_code == 200
    assert all(lab[b["item_id"]] == 0 for b in r.json)
    assert client.get(f"/api/sonic_fingerprint?{q}&engine=bogus"
                      ).status_code == 400
    # the config setting is the default of the parameter
    monkeypatch.setattr(C, "SONIC_FINGERPRINT_ENGINE", "graph")
    r = client.get(f"/api/sonic_fingerprint?{q}&n=20")
    assert r.headers["X-Radio-Engine"] == "graph"
    r = client.get(f"/api/radio?{q}&n=20")
    assert r.headers["X-Radio-Engine"] == "graph"


def test_sonic_fingerprint_task_engines(tmp_path):
    import json
    from types import SimpleNamespace

    from audiomuse_amd.analysis.maintenance import sonic_fingerprint_task
    from audiomuse_amd.db import write_txn
    from audiomuse_amd.mediaserver import make_provider

    url, conn, ids, labels = _radio_db(tmp_path)
    lab = {iid: labels[i] for i, iid in enumerate(ids)}
    # the provider's 10 tracks: five plays of taste A, five of taste B
    songs = make_provider("synthetic", n_albums=2,
                          tracks_per_album=5).get_all_songs()
    assert len(songs) == 10
    with write_txn(conn):
        for j, t in enumerate(songs):
            conn.execute(
                "INSERT OR REPLACE INTO track_server_map "
                "(provider_id, server_id, item_id) VALUES (?, 'default', ?)",
                (t.provider_id, ids[j if j < 5 else 145 + j]))
    ctx = SimpleNamespace(conn=conn)
    base = {"server_config": {"n_albums": 2, "tracks_per_album": 5}, "n": 20}

    def stored(name):
        row = conn.execute("SELECT item_ids FROM playlist WHERE name=?",
                           (name,)).fetchone()
        return json.loads(row["item_ids"])

    out = sonic_fingerprint_task(ctx, {**base, "name": "plain"})
    assert out == {"tracks": 20}
    assert 2 in {lab[i] for i in stored("plain")}
    out = sonic_fingerprint_task(ctx, {**base, "name": "walk",
                                       "engine": "graph"})
    assert out == {"tracks": 20, "engine": "graph"}
    assert {lab[i] for i in stored("walk")} <= {0, 1}
    assert "error" in sonic_fingerprint_task(ctx, {**base, "engine": "bogus"})
    conn.close()
