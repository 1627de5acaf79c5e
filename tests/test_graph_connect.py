"""Connected kNN graph on the CPU: component labels against scipy, the
label exclusion of the IVF scan against scan() + mask + ordered selection,
graph_connect.connect on a clustered fixture, and the engine, settings and
web endpoint on top of it."""

import functools
import math
import threading

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from audiomuse_amd import config as C
from audiomuse_amd.engines import graph_connect as GC
from audiomuse_amd.engines import projection as P
from audiomuse_amd.engines.graph_path import PathGraph
from audiomuse_amd.engines.graph_radio import graph_radio
from audiomuse_amd.engines.path import find_path_ex
from audiomuse_amd.engines.similarity import build_engine_from_matrix
from audiomuse_amd.index.ivf import IVFIndex
from tests.test_ivf_scope import NLIST, PAIRS, N, _allowed, _index, _queries

INF = float("inf")


# -- labels ------------------------------------------------------------------

def _lists(idx):
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    return idx.contiguous(), in_off.contiguous(), in_edge.contiguous()


def scipy_labels(idx):
    """Smallest vertex id of each component of the symmetrised graph."""
    n, k = idx.shape
    tail = torch.arange(n).unsqueeze(1).expand(n, k)[idx >= 0].numpy()
    head = idx[idx >= 0].numpy()
    adj = coo_matrix((np.ones(len(tail)), (tail, head)), shape=(n, n))
    _, comp = connected_components(adj, directed=False)
    smallest = np.full(comp.max() + 1, n)
    np.minimum.at(smallest, comp, np.arange(n))
    return torch.from_numpy(smallest[comp]).to(torch.int32)


def _sparse_graph(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g)
    idx[torch.rand(n, k, generator=g) < 0.5] = -1
    return idx.to(torch.int32)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 1000])
def test_labels_equal_scipy_on_random_graphs(n, k):
    for seed in range(3):
        idx = _sparse_graph(n, k, seed * 7 + n + k)
        labels, sweeps = GC.component_labels(*_lists(idx))
        assert labels.dtype == torch.int32 and labels.shape == (n,)
        assert torch.equal(labels, scipy_labels(idx))
        assert sweeps >= 1
    if n == 1000 and k == 1:       # or this test shows nothing
        assert scipy_labels(idx).unique().numel() > 10


def test_labels_with_self_slots_and_repeated_slots():
    idx = torch.tensor([[0, 0, 0],         # self slots only
                        [2, 2, 2],         # one neighbour, repeated
                        [2, -1, 1],        # self and back
                        [-1, -1, -1],      # nothing, and nobody points here
                        [5, 5, 4],
                        [-1, 4, 4],
                        [6, 3 + 3, 6]], dtype=torch.int32)
    labels, _ = GC.component_labels(*_lists(idx))
    assert labels.tolist() == [0, 1, 1, 3, 4, 4, 6]
    assert torch.equal(labels, scipy_labels(idx))


def test_labels_of_a_long_path_converge_in_log_sweeps():
    n = 4096
    idx = torch.full((n, 1), -1, dtype=torch.int32)
    idx[:-1, 0] = torch.arange(1, n, dtype=torch.int32)
    labels, sweeps = GC.component_labels(*_lists(idx))
    assert int(labels.max()) == 0
    assert sweeps <= 2 * math.ceil(math.log2(n))
    # the same path walked from the other end: the edges are symmetric
    idx2 = torch.full((n, 1), -1, dtype=torch.int32)
    idx2[1:, 0] = torch.arange(0, n - 1, dtype=torch.int32)
    labels, sweeps = GC.component_labels(*_lists(idx2))
    assert int(labels.max()) == 0
    assert sweeps <= 2 * math.ceil(math.log2(n))
    # numbered at random the shortcut helps little (the bound is the
    # diameter); the labels are right all the same, within n sweeps
    m = 512
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(m, generator=g).to(torch.int32)
    idx3 = torch.full((m, 1), -1, dtype=torch.int32)
    idx3[perm[:-1].long(), 0] = perm[1:]
    labels, sweeps = GC.component_labels(*_lists(idx3))
    assert int(labels.max()) == 0 and sweeps <= m + GC.SWEEP_GROUP


def test_reference_sweep_statement_and_changed_flag():
    idx, in_off, in_edge = _lists(_sparse_graph(200, 3, 5))
    cur = torch.arange(200, dtype=torch.int32)
    nxt = torch.empty_like(cur)
    changed = torch.tensor([7], dtype=torch.int32)
    GC.label_pull_reference(cur, nxt, idx, in_off, in_edge, changed)
    assert changed.tolist() == [1]                  # set to 1, whatever it held
    # the statement, vertex by vertex
    nb = [set() for _ in range(200)]
    for v, row in enumerate(idx.tolist()):
        for u in row:
            if u >= 0:
                nb[v].add(u)
                nb[u].add(v)
    lab = cur.tolist()
    want = [lab[min([lab[v]] + [lab[u] for u in nb[v]])] for v in range(200)]
    assert nxt.tolist() == want
    # at the fixed point the flag is left alone
    labels, _ = GC.component_labels(idx, in_off, in_edge)
    changed = torch.tensor([0], dtype=torch.int32)
    GC.label_pull_reference(labels, nxt, idx, in_off, in_edge, changed)
    assert changed.tolist() == [0] and torch.equal(nxt, labels)
    changed = torch.tensor([5], dtype=torch.int32)
    GC.label_pull_reference(labels, nxt, idx, in_off, in_edge, changed)
    assert changed.tolist() == [5]


# -- the label exclusion of the scan -----------------------------------------

def _masked_reference(idx, q, kk, row_labels, q_labels, skip=None):
    """scan() + the label mask + _ordered_select."""
    dist, row = idx.scan(q, nprobe=NLIST)
    rl = torch.as_tensor(row_labels)
    ql = torch.as_tensor(q_labels).unsqueeze(1)
    same = (rl[row.clamp(min=0).long()] == ql) & (ql >= 0)
    dist = dist.masked_fill(same, INF)
    if skip is not None:
        dist = dist.masked_fill(row == torch.as_tensor(skip).unsqueeze(1), INF)
    return IVFIndex._ordered_select(dist, row, kk)


def _random_labels(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 5, (N,), generator=g, dtype=torch.int32)


@pytest.mark.parametrize("kk", [1, 4, 300])
@pytest.mark.parametrize("metric,storage", PAIRS)
def test_scan_topk_with_labels_equals_masked_scan(metric, storage, kk):
    idx = _index(metric, storage)
    q = _queries()
    rl = _random_labels()
    ql = torch.tensor([0, 1, 2, 3, 4, -1], dtype=torch.int32)
    exp_d, exp_r = _masked_reference(idx, q, kk, rl, ql)
    got_d, got_r = idx.scan_topk(q, kk, nprobe=NLIST, row_labels=rl,
                                 q_labels=ql)
    assert got_d.shape == (6, kk) and got_r.dtype == torch.int32
    assert torch.equal(got_r, exp_r) and torch.equal(got_d, exp_d)
    for qi in range(5):                      # nothing of the query's label
        rows = got_r[qi][got_r[qi] >= 0].long()
        assert rows.numel() and not (rl[rows] == ql[qi]).any()
    # together with skip_rows
    skip = got_r[:, 0].clone()
    exp_d, exp_r = _masked_reference(idx, q, kk, rl, ql, skip=skip)
    got_d, got_r = idx.scan_topk(q, kk, nprobe=NLIST, row_labels=rl,
                                 q_labels=ql, skip_rows=skip)
    assert torch.equal(got_r, exp_r) and torch.equal(got_d, exp_d)


def test_scan_topk_label_edge_cases():
    idx = _index("angular", "f32")
    q = _queries()
    plain_d, plain_r = idx.scan_topk(q, 7, nprobe=NLIST)
    # one label everywhere: nothing but padding
    d, r = idx.scan_topk(q, 7, nprobe=NLIST,
                         row_labels=torch.zeros(N, dtype=torch.int32),
                         q_labels=torch.zeros(6, dtype=torch.int32))
    assert (r == -1).all() and torch.isinf(d).all()
    # q_label -1 excludes nothing
    d, r = idx.scan_topk(q, 7, nprobe=NLIST, row_labels=_random_labels(),
                         q_labels=torch.full((6,), -1))
    assert torch.equal(r, plain_r) and torch.equal(d, plain_d)
    # all labels distinct, the query carrying its own row's: skip_rows = self
    rows = torch.tensor([0, 1, 17, 1500, N - 2, N - 1])
    own = idx.vectors_f32[rows]
    d, r = idx.scan_topk(own, 7, nprobe=NLIST, row_labels=torch.arange(N),
                         q_labels=rows)
    sd, sr = idx.scan_topk(own, 7, nprobe=NLIST, skip_rows=rows)
    assert torch.equal(r, sr) and torch.equal(d, sd)
    assert not (r == rows.unsqueeze(1)).any()
    # a 1-D query takes one label
    d1, r1 = idx.scan_topk(own[0], 7, nprobe=NLIST,
                           row_labels=torch.arange(N), q_labels=rows[:1])
    assert torch.equal(r1[0], sr[0])
    # what does not go together
    with pytest.raises(ValueError):
        idx.scan_topk(q, 7, row_labels=_random_labels(),
                      q_labels=torch.zeros(6), scope=idx.make_scope(_allowed(0.05)))
    with pytest.raises(ValueError):
        idx.scan_topk(q, 7, row_labels=_random_labels())
    with pytest.raises(ValueError):
        idx.scan_topk(q, 7, q_labels=torch.zeros(6))
    with pytest.raises(ValueError):
        idx.scan_topk(q, 7, row_labels=_random_labels()[:-1],
                      q_labels=torch.zeros(6))
    with pytest.raises(ValueError):
        idx.scan_topk(q, 7, row_labels=_random_labels(),
                      q_labels=torch.zeros(5))


def test_cells_of_the_querys_label_do_not_consume_nprobe():
    """Labels = cells: every cell is pure, so at nprobe 1 a query that
    carries its nearest cell's label is sent to the next cell, and an
    unlabelled one (-1) to the nearest as before."""
    idx = _index("angular", "f32")
    q = _queries()
    cells = idx._row_assignments().to(torch.int32)
    q_enc, _ = idx._prepare_queries(q)
    filled = (idx.cell_off[1:] > idx.cell_off[:-1]).tolist()
    near = torch.tensor([[c for c in order if filled[c]][:2] for order
                         in idx._rank_cells(q_enc, NLIST).tolist()],
                        dtype=torch.int32)       # the two nearest with rows
    ql = near[:, 0].clone()
    ql[5] = -1
    mask = idx._label_cell_mask(cells, ql)
    n_empty = filled.count(False)
    assert mask.shape == (6, NLIST)
    assert mask.sum(dim=1).tolist() == [1 + n_empty] * 5 + [0]
    probe = idx._rank_cells(q_enc, 1, None, mask)
    assert torch.equal(probe[:5, 0], near[:5, 1]) and probe[5, 0] == near[5, 0]
    d, r = idx.scan_topk(q, 3, nprobe=1, row_labels=cells, q_labels=ql)
    assert torch.isfinite(d).all()
    assert torch.equal(cells[r[:5, 0].long()], near[:5, 1])
    # query_topk passes the labels through and re-ranks in f32
    qd, qi = idx.query_topk(q, 3, nprobe=1, row_labels=cells, q_labels=ql)
    assert qi.dtype == torch.int64 and torch.isfinite(qd).all()
    row_of = {int(i): r_ for r_, i in enumerate(idx.ids.tolist())}
    for qq in range(5):
        assert all(int(cells[row_of[i]]) == int(near[qq, 1])
                   for i in qi[qq].tolist())


def test_foreign_neighbours_equal_brute_force():
    idx = _index("angular", "f32")
    g = torch.Generator().manual_seed(9)
    labels = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
    rows = torch.tensor([0, 5, 999, N - 1])
    fd, fi = idx.foreign_neighbours(labels, 4, rows=rows, nprobe=NLIST)
    assert fd.shape == (4, 4) and fi.dtype == torch.int64
    v = idx.vectors_f32 / idx.vectors_f32.norm(dim=1, keepdim=True)
    full = 1.0 - v[rows] @ v.T
    full[labels[rows].unsqueeze(1) == labels.unsqueeze(0)] = INF
    want = torch.topk(full, 4, dim=1, largest=False)
    assert torch.equal(fi, idx.ids[want.indices])
    torch.testing.assert_close(fd, want.values, rtol=0, atol=1e-6)
    # all rows, in chunks that do not divide N, default nprobe
    fd_all, fi_all = idx.foreign_neighbours(labels, 2, chunk=700)
    assert fd_all.shape == (N, 2) and (fi_all >= 0).all()
    row_of = torch.empty(N, dtype=torch.int64)
    row_of[idx.ids] = torch.arange(N)
    assert not (labels[row_of[fi_all]] == labels.unsqueeze(1)).any()
    # one label: padding
    fd1, fi1 = idx.foreign_neighbours(torch.zeros(N), 2, rows=rows)
    assert (fi1 == -1).all() and torch.isinf(fd1).all()
    with pytest.raises(ValueError):
        idx.foreign_neighbours(labels[:-1], 2)
    with pytest.raises(ValueError):
        idx.foreign_neighbours(labels, 2, rows=torch.tensor([N]))


# -- connect -----------------------------------------------------------------------
#
# 600 points on the unit sphere in 6 clusters of 100 around orthonormal
# centres (angular distance 1 between clusters, about 0.03 inside one).
# Point 0 of cluster i is its tip: the normalised blend of its own centre
# and the next cluster's, TIP_BLEND[i] of the way over, so it is by far the
# cluster's nearest point to another cluster and the six tip distances
# differ from each other by about 0.03. The order of the points is shuffled.

CLUSTERS, PER, DIM, K = 6, 100, 16, 5
TIP_BLEND = (0.30, 0.33, 0.36, 0.39, 0.42, 0.45)
FIXTURE_NLIST = 8


@functools.lru_cache(maxsize=None)
def clustered_points():
    """(x (600, 16) f32, cluster (600,) of each point, tips (6,) positions)."""
    rng = np.random.default_rng(0)
    centres = np.eye(DIM)[:CLUSTERS]
    x = np.empty((CLUSTERS * PER, DIM))
    for i in range(CLUSTERS):
        pts = centres[i] + 0.03 * rng.standard_normal((PER, DIM))
        t = TIP_BLEND[i]
        pts[0] = (1 - t) * centres[i] + t * centres[(i + 1) % CLUSTERS]
        x[i * PER:(i + 1) * PER] = pts
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    perm = rng.permutation(CLUSTERS * PER)
    cluster = (perm // PER)
    tips = np.array([int(np.nonzero(perm == i * PER)[0][0])
                     for i in range(CLUSTERS)])
    return x[perm].astype(np.float32), cluster, tips


def clustered_engine(device="cpu", metric="angular"):
    x, _, _ = clustered_points()
    ids = [f"s{i}" for i in range(x.shape[0])]
    meta = {i: {"title": i, "author": f"artist-{i}"} for i in ids}
    return build_engine_from_matrix(x, ids, metric=metric, storage="f32",
                                    nlist=FIXTURE_NLIST, device=device,
                                    meta_fn=meta.get)


def lightest_foreign_pairs(labels):
    """{label: ((u, v), margin)} from float64 brute force: the lightest
    pair with u in the component and v outside, and the gap to the
    lightest pair on other endpoints."""
    x, _, _ = clustered_points()
    x = x.astype(np.float64)
    d = 1.0 - x @ x.T
    out = {}
    for lab in np.unique(labels):
        inside = np.nonzero(labels == lab)[0]
        outside = np.nonzero(labels != lab)[0]
        block = d[np.ix_(inside, outside)]
        flat = np.sort(block, axis=None)
        a, b = np.unravel_index(np.argmin(block), block.shape)
        out[int(lab)] = ((int(inside[a]), int(outside[b])),
                         float(flat[1] - flat[0]))
    return out


@functools.lru_cache(maxsize=None)
def _plain_and_connected():
    eng = clustered_engine()
    assert eng.index.nlist == FIXTURE_NLIST
    pos, dists = eng.neighbor_graph(K, nprobe=FIXTURE_NLIST)
    out = GC.connect(pos, dists, eng.index, 4, 8, nprobe=FIXTURE_NLIST)
    return eng, pos, dists, out


def _ends(bridges):
    return {frozenset((u, v)) for u, v, _ in bridges}


def test_connect_bridges_the_clusters():
    eng, pos, dists, (pos2, dists2, report) = _plain_and_connected()
    labels0, _ = GC.component_labels(*GC.adjacency(pos, dists))
    before = int(labels0.unique().numel())
    assert before >= 4
    assert report["components_before"] == before
    assert report["largest_before"] == int(labels0.unique(
        return_counts=True)[1].max())
    assert report["vertices"] == 600 and report["without_vector"] == 0
    assert report["connect"] is True and report["seconds"] > 0
    # one component left, by a spanning number of bridges
    labels1, _ = GC.component_labels(*GC.adjacency(pos2, dists2))
    assert int(labels1.max()) == 0 and report["components_after"] == 1
    assert report["bridges"] == before - 1
    assert 1 <= report["rounds"] <= 8
    # the original slots are untouched, the bridges sit behind them
    x = report["extra_slots"]
    assert x >= 1 and pos2.shape == (600, K + x) and dists2.shape == pos2.shape
    assert torch.equal(pos2[:, :K], pos) and torch.equal(dists2[:, :K], dists)
    assert pos2.dtype == pos.dtype and dists2.dtype == dists.dtype
    bridges = GC.bridges_of(pos2, dists2, K)
    assert len(bridges) == before - 1
    assert ((pos2[:, K:] >= 0) == torch.isfinite(dists2[:, K:])).all()
    assert int((pos2[:, K:] >= 0).sum(dim=1).max()) == x
    # every bridge joins two components of the graph it was added to:
    # replayed in distance order per round, each one merges two sets
    parent = list(range(600))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for v, row in enumerate(pos.tolist()):
        for u in row:
            if u >= 0:
                parent[find(u)] = find(v)
    v32 = eng.index.vectors_f32
    vec = {int(i): v32[r] for r, i in enumerate(eng.index.ids.tolist())}
    for u, v, d in bridges:
        assert int(labels0[u]) != int(labels0[v])
        want = 1.0 - float(torch.dot(vec[u], vec[v])
                           / (vec[u].norm() * vec[v].norm()))
        assert d == pytest.approx(want, abs=1e-6)     # the f32 distance
    merged = 0
    for u, v, _ in sorted(bridges, key=lambda b: b[2]):
        if find(u) != find(v):
            parent[find(u)] = find(v)
            merged += 1
    assert merged == len(bridges)


def test_connect_takes_the_lightest_edge_of_every_queried_component():
    eng, pos, dists, (pos2, dists2, report) = _plain_and_connected()
    labels0, _ = GC.component_labels(*GC.adjacency(pos, dists))
    uniq, counts = labels0.unique(return_counts=True)
    big = int(uniq[counts == counts.max()].min())
    ends = _ends(GC.bridges_of(pos2, dists2, K))
    pairs = lightest_foreign_pairs(labels0.numpy())
    queried = [int(c) for c in uniq.tolist() if int(c) != big]
    assert len(queried) == len(uniq) - 1 >= 3
    for lab in queried:
        (u, v), margin = pairs[lab]
        assert margin > 1e-4            # far above f32 rounding
        assert frozenset((u, v)) in ends, (lab, u, v)


def test_connect_is_deterministic():
    eng, pos, dists, (pos2, dists2, report) = _plain_and_connected()
    pos3, dists3, report3 = GC.connect(pos, dists, eng.index, 4, 8,
                                       nprobe=FIXTURE_NLIST)
    assert torch.equal(pos3, pos2) and torch.equal(dists3, dists2)
    for key in ("components_before", "components_after", "bridges", "rounds",
                "extra_slots", "bridges_per_round", "label_sweeps"):
        assert report3[key] == report[key]


def test_connect_rounds_and_limits():
    eng, pos, dists, (pos2, _, report) = _plain_and_connected()
    # no rounds allowed: the table comes back as it went in
    p0, d0, r0 = GC.connect(pos, dists, eng.index, 4, 0, nprobe=FIXTURE_NLIST)
    assert p0 is pos and d0 is dists and r0["bridges"] == 0
    assert r0["rounds"] == 0 and r0["extra_slots"] == 0
    assert r0["components_after"] == r0["components_before"] >= 4
    # one candidate per vertex still connects, perhaps in more rounds
    p1, d1, r1 = GC.connect(pos, dists, eng.index, 1, 8, nprobe=FIXTURE_NLIST)
    assert r1["components_after"] == 1
    assert r1["bridges"] == r1["components_before"] - 1
    # a connected graph is left alone
    p2, d2, r2 = GC.connect(pos2, _, eng.index, 4, 8, nprobe=FIXTURE_NLIST)
    assert p2 is pos2 and r2["components_before"] == 1 and r2["rounds"] == 0
    with pytest.raises(ValueError):
        GC.connect(pos, dists, eng.index, 0, 8)


def test_vertices_without_a_vector_stay_isolated():
    eng = clustered_engine()
    _, _, tips = clustered_points()
    gone = [int(tips[0]), 7, 300]
    eng.index.remove(torch.tensor(gone))
    pos, dists = eng.neighbor_graph(K, nprobe=FIXTURE_NLIST)
    assert (pos[gone] == -1).all()
    pos2, dists2, report = GC.connect(pos, dists, eng.index, 4, 8,
                                      nprobe=FIXTURE_NLIST)
    assert report["without_vector"] == 3 and report["vertices"] == 600
    assert report["components_after"] == 1
    assert report["bridges"] == report["components_before"] - 1
    assert (pos2[gone] == -1).all()
    assert not torch.isin(pos2, torch.tensor(gone)).any()
    labels, _ = GC.component_labels(*GC.adjacency(pos2, dists2))
    assert labels[gone].tolist() == gone
    assert labels.unique().numel() == 1 + 3


# -- engine --------------------------------------------------------------------------

@pytest.fixture()
def exact_graph(monkeypatch):
    """The engine's graph at the fixture's width, every cell probed."""
    monkeypatch.setattr(C, "PATH_GRAPH_NEIGHBOURS", K)
    monkeypatch.setattr(C, "IVF_GRAPH_NPROBE", FIXTURE_NLIST)
    monkeypatch.setattr(C, "PATH_FIX_SIZE", False)


def _two_clusters():
    _, cluster, _ = clustered_points()
    a = int(np.nonzero(cluster == 1)[0][3])
    b = int(np.nonzero(cluster == 4)[0][3])
    return f"s{a}", f"s{b}"


def test_settings_defaults():
    assert C.PATH_GRAPH_CONNECT is False
    assert C.PATH_GRAPH_BRIDGE_CANDIDATES == 4
    assert C.PATH_GRAPH_BRIDGE_ROUNDS == 8


def test_graph_path_crosses_clusters_when_connected(exact_graph, monkeypatch):
    eng = clustered_engine()
    a, b = _two_clusters()
    items, used = find_path_ex(eng, a, b, length=500, engine="graph")
    assert used == "waypoint"                       # today: no path, fallback
    plain = eng.path_graph()
    assert plain.idx.shape == (600, K)
    assert eng.graph_report()["connect"] is False

    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    items, used = find_path_ex(eng, a, b, length=500, engine="graph")
    assert used == "graph"
    got = [p["item_id"] for p in items]
    assert got[0] == a and got[-1] == b and len(set(got)) == len(got) > 2
    wide = eng.path_graph()
    report = eng.graph_report()
    assert wide.idx.shape == (600, K + report["extra_slots"])
    assert torch.equal(wide.idx[:, :K], plain.idx)
    assert report["connect"] is True and report["components_after"] == 1
    assert report["bridges"] == report["components_before"] - 1
    # every step of the unthinned journey is a kNN edge or a bridge
    edges = set()
    for v, row in enumerate(plain.idx.tolist()):
        edges |= {frozenset((v, u)) for u in row if u >= 0}
    n_knn = len(edges)
    for v, row in enumerate(wide.idx[:, K:].tolist()):
        edges |= {frozenset((v, u)) for u in row if u >= 0}
    assert len(edges) == n_knn + report["bridges"]
    hops = [frozenset((eng.pos[s], eng.pos[t]))
            for s, t in zip(got[:-1], got[1:])]
    assert all(h in edges for h in hops)
    # path and radio share one connected build
    calls = []
    real = GC.connect
    monkeypatch.setattr(GC, "connect",
                        lambda *a_, **k_: calls.append(1) or real(*a_, **k_))
    rank = eng.rank_graph()
    assert rank.idx.shape == wide.idx.shape and not calls
    assert eng.path_graph() is wide

    # and off again: exactly the graph from before
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", False)
    again = eng.path_graph()
    for name in ("idx", "w", "in_off", "in_edge"):
        assert torch.equal(getattr(again, name), getattr(plain, name))
    pos, dists = eng.neighbor_graph(K)
    fresh = PathGraph.from_knn(pos, dists, C.PATH_GRAPH_EXPONENT)
    for name in ("idx", "w", "in_off", "in_edge"):
        assert torch.equal(getattr(again, name), getattr(fresh, name))


def test_graph_radio_with_seeds_in_two_clusters(exact_graph, monkeypatch):
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    eng = clustered_engine()
    a, b = _two_clusters()
    items, used = graph_radio(eng, [a, b], n=20, engine="graph")
    assert used == "graph" and len(items) == 20
    _, cluster, _ = clustered_points()
    seen = {int(cluster[eng.pos[i["item_id"]]]) for i in items}
    assert {1, 4} <= seen
    assert eng.rank_graph().idx.shape[1] == K + eng.graph_report()["extra_slots"]


def test_dot_metric_has_no_graph_and_no_report(exact_graph, monkeypatch):
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    eng = clustered_engine(metric="dot")
    assert eng.path_graph() is None and eng.rank_graph() is None
    assert eng.graph_report(build=True) is None


def test_graph_report_builds_only_on_request(exact_graph, monkeypatch):
    eng = clustered_engine()
    assert eng.graph_report() is None
    off = eng.graph_report(build=True)
    assert off["connect"] is False and off["bridges"] == 0
    assert off["components_after"] == off["components_before"] >= 4
    assert off["rounds"] == 0 and off["extra_slots"] == 0
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    assert eng.graph_report() is None           # the connected one is not built
    on = eng.graph_report(build=True)
    for key in ("connect", "vertices", "without_vector", "components_before",
                "largest_before", "components_after", "bridges", "rounds",
                "extra_slots", "seconds"):
        assert key in on
    assert on["components_before"] == off["components_before"]
    assert on["components_after"] == 1 and on["largest_before"] == 100
    # the index moves: the report goes with the graph
    v = eng.index.vector_for_id(7).clone()
    eng.index.remove(torch.tensor([7]))
    eng.index.add(v.unsqueeze(0), torch.tensor([7]))
    assert eng.graph_report() is None


# -- web -----------------------------------------------------------------------------

@pytest.fixture()
def components_client(tmp_path):
    from audiomuse_amd.analysis.index import build_audio_index
    from audiomuse_amd.db import connect
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding
    from audiomuse_amd.web.app import create_app

    url = "sqlite:///" + str(tmp_path / "web.db")
    conn = connect(url)
    init_db(conn)
    rng = np.random.default_rng(5)
    ids = []
    for i in range(120):
        iid = f"fp_4{'%050x' % i}"
        ids.append(iid)
        emb = 0.02 * rng.standard_normal(200)
        emb[i % 3] += 1.0                         # three far clusters
        save_track_analysis_and_embedding(
            conn, iid, title=f"Song {i}", author=f"Artist {i}",
            album=f"Album {i % 40}", tempo=100.0, energy=0.5, key="C",
            scale="major", duration=200.0, mood_vector={}, other_features={},
            embedding=emb.astype(np.float32))
    build_audio_index(conn)
    app = create_app(url, device="cpu", auth_disabled=True)
    app.testing = True
    # the boot-time warm-up loads the engine on a thread of its own and
    # stores it when done; let it finish, so that the engine the first
    # request builds the graph on is the one later requests see
    for t in threading.enumerate():
        if t.name == "audiomuse-engine-warm":
            t.join()
    with app.test_client() as client:
        yield client, ids
    conn.close()


def test_web_graph_components(components_client, monkeypatch):
    client, ids = components_client
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    monkeypatch.setattr(C, "PATH_GRAPH_NEIGHBOURS", K)
    r = client.get("/api/graph/components")
    assert r.status_code == 200 and r.json == {"built": False}
    r = client.get("/api/graph/components?build=1")
    assert r.status_code == 200
    body = r.json
    assert body["built"] is True and body["connect"] is True
    assert body["vertices"] == 120 and body["without_vector"] == 0
    assert body["components_before"] >= 3 and body["components_after"] == 1
    assert body["bridges"] == body["components_before"] - 1
    assert client.get("/api/graph/components").json == body
    # the two graph engines answer across clusters, headers as before
    r = client.get(f"/api/path?start={ids[0]}&end={ids[1]}&length=6"
                   "&engine=graph")
    assert r.status_code == 200 and r.headers["X-Path-Engine"] == "graph"
