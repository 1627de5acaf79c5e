"""The fused layout engine of the 2-D maps (MAP_LAYOUT_ENGINE=fused):
epoch semantics on the torch reference (CPU), engine selection, layout
quality against the eager engine, and the HIP epoch kernel against the
reference (GPU)."""

import functools
import io

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import projection as P

M32 = 0xFFFFFFFF
FULL = 1 << 24


# -- helpers -------------------------------------------------------------------


def _py_mix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) % (1 << 32)
    h ^= h >> 13
    h = (h * 0xC2B2AE35) % (1 << 32)
    h ^= h >> 16
    return h


def _py_draw(seed, epoch, e, d):
    base = _py_mix(seed ^ (((epoch + 1) * 0x9E3779B9) % (1 << 32)))
    return _py_mix((_py_mix((base + e) % (1 << 32)) + d) % (1 << 32))


def neighbour_preservation(nbrs: torch.Tensor, emb: torch.Tensor) -> float:
    """Mean over points of the share of a point's k graph neighbours that
    are among its k nearest points in the layout (at most 2000 points)."""
    n, k = nbrs.shape
    assert n <= 2000
    d = torch.cdist(emb.double(), emb.double())
    d.fill_diagonal_(float("inf"))
    near = d.topk(k, dim=1, largest=False).indices
    hit = (near.unsqueeze(2) == nbrs.to(near.device).unsqueeze(1)).any(dim=1)
    return float(hit.double().mean())


def _three_clusters():
    g = torch.Generator().manual_seed(0)
    centers = torch.randn(3, 16, generator=g) * 6
    assign = torch.arange(120) % 3
    x = centers[assign] + torch.randn(120, 16, generator=g) * 0.3
    return x, assign


@functools.lru_cache(maxsize=None)
def _twenty_centres():
    g = torch.Generator().manual_seed(1)
    centres = torch.randn(20, 32, generator=g) * 3
    x = centres[torch.arange(2000) % 20] + torch.randn(2000, 32, generator=g)
    _, nbrs = P.knn_graph(x, 15)
    return x, nbrs


def _intra_inter(emb, lab, n):
    intra, inter = [], []
    for i in range(0, n, 7):
        for j in range(1, n, 11):
            d = float((emb[i] - emb[j]).norm())
            (intra if lab[i] == lab[j] else inter).append(d)
    return np.mean(intra), np.mean(inter)


def _random_graph(n, k, seed, missing=0.0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g)
    thr = torch.randint(0, FULL + 1, (n, k), generator=g).to(torch.int32)
    thr[torch.rand(n, k, generator=g) < 0.2] = 0
    thr[torch.rand(n, k, generator=g) < 0.2] = FULL
    if missing:
        idx[torch.rand(n, k, generator=g) < missing] = -1
    thr = torch.where(idx < 0, torch.zeros_like(thr), thr)
    return idx, thr


# -- CPU: the reference path ---------------------------------------------------


def test_hash_vectors_match_plain_python():
    cases = [(0, 0, 0, 0), (0, 0, 1, 0), (7, 3, 12345, 1), (M32, 199, 2 ** 31 - 1, 5),
             (123456789, 50, 14999999, 64), (2 ** 31, 0, 17, 3)]
    for seed, epoch, e, d in cases:
        got = int(P.layout_draw(seed, epoch, torch.tensor([e]), d)[0])
        assert got == _py_draw(seed, epoch, e, d), (seed, epoch, e, d)
    # and vectorised: many edges at once
    e = torch.arange(0, 5000, 7)
    got = P.layout_draw(11, 4, e, 2).tolist()
    assert got == [_py_draw(11, 4, int(v), 2) for v in e]
    # a fixed value, so that a change of the formulas cannot pass unseen by
    # changing both implementations alike
    assert _py_mix(1) == 0x514E28B7


def test_inactive_epoch_is_the_identity():
    idx, thr = _random_graph(50, 4, seed=2)
    thr = torch.zeros_like(thr)
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    assert in_edge.numel() == 0 and int(in_off[-1]) == 0
    E = torch.randn(50, 2, generator=torch.Generator().manual_seed(3)) * 10
    out = P.layout_epoch_reference(E, idx, thr, in_off, in_edge, 1.0, 0, 0, 5)
    assert torch.equal(out, E)


def _py_attract(dx, dy):
    a, b = P._A, P._B
    d2 = dx * dx + dy * dy
    c = -2.0 * a * b * max(d2, 1e-12) ** (b - 1) / (1.0 + a * d2 ** b)
    return [min(max(c * dx, -4.0), 4.0), min(max(c * dy, -4.0), 4.0)]


def test_active_epoch_matches_a_plain_python_loop():
    idx = torch.tensor([[1, 2], [0, 3], [3, 0], [2, 1]])
    thr = torch.full((4, 2), FULL, dtype=torch.int32)
    E = [[0.0, 0.0], [1.5, -0.5], [-2.0, 3.0], [8.0, 7.0]]
    alpha, n, k = 0.7, 4, 2
    want = []
    for i in range(n):
        p = list(E[i])
        for j in range(n):                       # tail pulls, input positions
            for s in range(k):
                if int(idx[j, s]) == i:
                    f = _py_attract(E[j][0] - E[i][0], E[j][1] - E[i][1])
                    p = [p[0] - alpha * f[0], p[1] - alpha * f[1]]
        for s in range(k):                       # own edges, running p
            j = int(idx[i, s])
            f = _py_attract(p[0] - E[j][0], p[1] - E[j][1])
            p = [p[0] + alpha * f[0], p[1] + alpha * f[1]]
        want.append(p)
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    got = P.layout_epoch_reference(torch.tensor(E, dtype=torch.float64), idx,
                                   thr, in_off, in_edge, alpha, 5, 9, 0,
                                   dtype=torch.float64)
    assert got.dtype == torch.float64
    err = (got - torch.tensor(want, dtype=torch.float64)).abs().max()
    assert float(err) <= 1e-12, float(err)
    # every point moved: the epoch was active
    moved = (got - torch.tensor(E, dtype=torch.float64)).abs().max(dim=1)
    assert float(moved.values.min()) > 0.1


def test_reverse_lists():
    n, k = 300, 7
    idx, thr = _random_graph(n, k, seed=4, missing=0.1)
    assert (idx < 0).any() and (thr == 0).any()
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    assert in_off.dtype == torch.int32 and in_edge.dtype == torch.int32
    assert in_off.shape == (n + 1,) and int(in_off[0]) == 0
    want = [[] for _ in range(n)]
    for e in range(n * k):
        if int(thr.view(-1)[e]) > 0:
            want[int(idx.view(-1)[e])].append(e)
    for i in range(n):
        got = in_edge[int(in_off[i]):int(in_off[i + 1])].tolist()
        assert got == want[i], i
    assert int(in_off[-1]) == in_edge.numel() == int((thr > 0).sum())
    # a missing neighbour is never listed and never sampled
    gone = set(torch.nonzero(idx.view(-1) < 0).view(-1).tolist())
    assert gone and not gone & set(in_edge.tolist())
    assert P.layout_thresholds(idx, torch.ones(n, k))[idx < 0].eq(0).all()
    E = torch.randn(n, 2, generator=torch.Generator().manual_seed(5)) * 10
    lonely = torch.full((n, k), -1)
    zeros = P.layout_thresholds(lonely, torch.ones(n, k))
    off0, edge0 = P.layout_reverse_lists(lonely, zeros)
    out = P.layout_epoch_reference(E, lonely, zeros, off0, edge0, 1.0, 0, 0, 5)
    assert torch.equal(out, E)


def test_thresholds_are_rounded_weights():
    idx = torch.zeros(1, 4, dtype=torch.long)
    w = torch.tensor([[0.0, 1.0, 0.5, 2.0 ** -25]])
    assert P.layout_thresholds(idx, w).tolist() == [[0, FULL, FULL // 2, 0]]


def test_edge_count_limit_is_named():
    idx = torch.zeros(1, dtype=torch.long).expand(2 ** 29, 4)
    thr = torch.zeros(1, dtype=torch.int32).expand(2 ** 29, 4)
    with pytest.raises(ValueError, match=r"2\^31"):
        P.layout_reverse_lists(idx, thr)
    with pytest.raises(ValueError, match=r"2\^31"):
        P.layout_epoch_reference(torch.zeros(1, 2).expand(2 ** 29, 2), idx,
                                 thr, torch.zeros(2, dtype=torch.int32),
                                 torch.zeros(0, dtype=torch.int32), 1.0, 0, 0, 0)


def test_engine_selection(monkeypatch):
    x, _ = _three_clusters()
    fused = P.umap_project(x, epochs=10, seed=0, engine="fused")
    monkeypatch.setattr(C, "MAP_LAYOUT_ENGINE", "fused")
    assert torch.equal(P.umap_project(x, epochs=10, seed=0), fused)
    monkeypatch.undo()
    assert C.MAP_LAYOUT_ENGINE == "torch"
    plain = P.umap_project(x, epochs=10, seed=0)
    assert torch.equal(plain, P.umap_project(x, epochs=10, seed=0,
                                             engine="torch"))
    assert not torch.equal(plain, fused)
    with pytest.raises(ValueError):
        P.umap_project(x, epochs=10, seed=0, engine="nonsense")
    monkeypatch.setattr(C, "MAP_LAYOUT_ENGINE", "nonsense")
    with pytest.raises(ValueError):
        P.umap_project(x, epochs=10, seed=0)


def _map_db(tmp_path, x):
    from audiomuse_amd.db import connect
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding

    conn = connect(f"sqlite:///{tmp_path}/map.db")
    init_db(conn)
    for i in range(x.shape[0]):
        save_track_analysis_and_embedding(
            conn, f"fp_4{'%050x' % i}", title=f"S{i}", author=f"A{i % 6}",
            embedding=x[i].numpy().astype(np.float32))
    return conn


def test_map_builders_refuse_an_unknown_engine(tmp_path, monkeypatch):
    from audiomuse_amd.analysis import index as aindex

    x = torch.randn(12, 8, generator=torch.Generator().manual_seed(0))
    conn = _map_db(tmp_path, x)
    monkeypatch.setattr(C, "MAP_LAYOUT_ENGINE", "nonsense")
    with pytest.raises(ValueError):
        aindex.build_song_map(conn)
    with pytest.raises(ValueError):
        aindex.build_artist_map(conn)
    conn.close()


def test_fused_engine_preserves_clusters():
    x, assign = _three_clusters()
    emb = P.umap_project(x, epochs=80, seed=0, engine="fused")
    assert emb.shape == (120, 2) and torch.isfinite(emb).all()
    intra, inter = _intra_inter(emb, assign, 120)
    print(f"fused engine, 120 points: intra/inter {intra / inter:.3f}")
    assert intra < 0.5 * inter


@pytest.mark.slow
def test_fused_engine_keeps_neighbours_like_the_torch_engine():
    x, nbrs = _twenty_centres()
    score = {"fused": [], "torch": []}
    for seed in range(3):
        for engine in score:
            emb = P.umap_project(x, n_neighbors=15, epochs=200, seed=seed,
                                 engine=engine)
            assert torch.isfinite(emb).all()
            score[engine].append(neighbour_preservation(nbrs, emb))
    print("neighbour preservation:", score)
    assert np.mean(score["fused"]) >= 0.95 * np.mean(score["torch"])


def test_song_map_through_the_fused_engine(tmp_path, monkeypatch):
    from audiomuse_amd.analysis import index as aindex
    from audiomuse_amd.cluster.algorithms import pca_fit_transform
    from audiomuse_amd.db.store import load_index_blob

    g = torch.Generator().manual_seed(0)
    n = 240
    centers = torch.randn(4, 32, generator=g) * 6
    assign = torch.arange(n) % 4
    x = centers[assign] + torch.randn(n, 32, generator=g) * 0.3
    conn = _map_db(tmp_path, x)

    monkeypatch.setattr(C, "MAP_LAYOUT_ENGINE", "fused")
    calls = []
    real = P.layout_epoch_reference

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(P, "layout_epoch_reference", spy)
    assert aindex.build_song_map(conn) == n
    assert len(calls) == 200
    blob, meta = load_index_blob(conn, aindex.SONG_MAP)
    payload = torch.load(io.BytesIO(blob), weights_only=True)
    emb = payload["coords"]
    assert meta["n"] == n and emb.shape == (n, 2)
    assert torch.isfinite(emb).all()
    rows = torch.tensor([int(s[4:], 16) for s in payload["item_ids"]])
    # a layout, not the PCA fallback
    pca, _, _ = pca_fit_transform(x[rows], 2)
    assert not torch.allclose(emb, pca.float(), atol=1e-3)
    intra, inter = _intra_inter(emb, assign[rows], n)
    assert intra < 0.5 * inter
    conn.close()


# -- GPU: the epoch kernel against the reference -------------------------------
#
# Tolerance: R64 and R32 are the reference in f64 and f32 on the CPU from
# the same inputs, delta = max|R32 - R64|. The kernel passes if
# max|K - R64| <= 8*delta + 1e-6*max|R64|: its pow, its division and the
# order of its step-1 sum each differ from torch's f32 by a few ulp per
# term. A wrong sampling decision or negative index moves a point by up
# to 4*alpha, orders of magnitude beyond the bound. One epoch only: the
# f32 deviation grows about tenfold per epoch.


def _ext():
    from audiomuse_amd.ops import _ext as loader

    return loader.require()


def _kernel_epoch(E, idx, thr, in_off, in_edge, alpha, seed, epoch, neg):
    dev = "cuda"
    thr_d = thr.to(dev).contiguous()
    in_edge_d = in_edge.to(dev)
    in_thr = thr_d.view(-1)[in_edge_d.long()].contiguous()
    E_d = E.to(dev).contiguous()
    out = torch.empty_like(E_d)
    _ext().umap_epoch(E_d, out, idx.to(dev, torch.int32).contiguous(), thr_d,
                      in_off.to(dev), in_edge_d, in_thr, alpha, P._A, P._B,
                      seed, epoch, neg)
    torch.cuda.synchronize()
    return out.cpu()


def _check_epoch(tag, E, idx, thr, in_off, in_edge, alpha, seed, epoch, neg):
    r64 = P.layout_epoch_reference(E, idx, thr, in_off, in_edge, alpha, seed,
                                   epoch, neg, dtype=torch.float64)
    r32 = P.layout_epoch_reference(E, idx, thr, in_off, in_edge, alpha, seed,
                                   epoch, neg)
    got = _kernel_epoch(E, idx, thr, in_off, in_edge, alpha, seed, epoch, neg)
    assert torch.isfinite(got).all()
    delta = float((r32.double() - r64).abs().max())
    dev = float((got.double() - r64).abs().max())
    bound = 8 * delta + 1e-6 * float(r64.abs().max())
    moved = float((r64 - E.double()).abs().max())
    print(f"umap_epoch {tag}: delta {delta:.3e} kernel {dev:.3e} "
          f"bound {bound:.3e} moved {moved:.3e}")
    assert dev <= bound, (tag, dev, bound)


@functools.lru_cache(maxsize=None)
def _layout_case(n, k):
    """Graph, thresholds, reverse lists, the PCA-style init and the state
    after 50 reference epochs, from the engine's own set-up."""
    g = torch.Generator().manual_seed(n * 31 + k)
    x = torch.randn(8, 12, generator=g)[torch.arange(n) % 8] * 2 \
        + torch.randn(n, 12, generator=g)
    idx, wsym, emb, _ = P._layout_setup(x, k, 0, None)
    assert idx.shape == (n, k)
    thr = P.layout_thresholds(idx, wsym / wsym.max().clamp(min=1e-12))
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    later = emb
    for epoch in range(50):
        later = P.layout_epoch_reference(later, idx, thr, in_off, in_edge,
                                         1.0 - epoch / 200, 3, epoch, 5)
    return idx, thr, in_off, in_edge, emb, later


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["init", "after50"])
@pytest.mark.parametrize("alpha", [1.0, 0.3])
@pytest.mark.parametrize("neg", [0, 5])
@pytest.mark.parametrize("n,k", [(5, 4), (1000, 15), (777, 30), (64, 1)])
def test_gpu_epoch_matches_reference(n, k, neg, alpha, state):
    idx, thr, in_off, in_edge, init, later = _layout_case(n, k)
    E, epoch = (init, 0) if state == "init" else (later, 50)
    _check_epoch(f"n={n} k={k} neg={neg} alpha={alpha} {state}", E, idx, thr,
                 in_off, in_edge, alpha, 3, epoch, neg)


@pytest.mark.gpu
@pytest.mark.parametrize("neg", [1, 3, 4, 9])
def test_gpu_epoch_other_negative_counts(neg):
    """Counts other than 0 and 5 take the kernel's run-time loop."""
    idx, thr, in_off, in_edge, init, _ = _layout_case(777, 30)
    _check_epoch(f"n=777 k=30 neg={neg} alpha=1.0 init", init, idx, thr,
                 in_off, in_edge, 1.0, 3, 0, neg)


def _positions(n, seed):
    return torch.randn(n, 2, generator=torch.Generator().manual_seed(seed)) * 10


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["star", "orphans"])
def test_gpu_epoch_hub_and_orphan(graph):
    n, k = 3000, 3
    g = torch.Generator().manual_seed(6)
    i = torch.arange(n)
    if graph == "star":
        idx = torch.stack([torch.zeros(n, dtype=torch.long), (i + 1) % n,
                           (i + 2) % n], dim=1)
        idx[0, 0] = -1                  # vertex 0 does not list itself
    else:
        idx = torch.randint(0, n // 2, (n, k), generator=g)
    thr = torch.randint(0, FULL + 1, (n, k), generator=g).to(torch.int32)
    thr[torch.rand(n, k, generator=g) < 0.3] = FULL
    thr = torch.where(idx < 0, torch.zeros_like(thr), thr)
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    deg = in_off[1:] - in_off[:-1]
    if graph == "star":
        assert int(deg[0]) >= int((thr[1:, 0] > 0).sum()) >= 2990
    else:
        assert int(deg[n // 2:].max()) == 0
    for neg, alpha in ((0, 1.0), (5, 0.3)):
        _check_epoch(f"{graph} n={n} k={k} neg={neg} alpha={alpha}",
                     _positions(n, 7), idx, thr, in_off, in_edge, alpha, 1, 2,
                     neg)


@pytest.mark.gpu
def test_gpu_epoch_in_list_length_threshold():
    """In-edge lists up to 64 entries are walked by the owner lane, longer
    ones by its wave: 64 and 65 entries, both owners in one wave."""
    n, k = 200, 2
    i = torch.arange(n)
    idx = torch.stack([(i + 1) % n, (i + 7) % n], dim=1)
    idx[2:66, 0] = 0
    idx[66:131, 0] = 1
    idx[199, 0] = idx[0, 0] = 5          # the ring's own edges into 0 and 1
    idx[193, 1] = idx[194, 1] = 5
    thr = torch.full((n, k), FULL, dtype=torch.int32)
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    deg = (in_off[1:] - in_off[:-1]).tolist()
    assert deg[0] == 64 and deg[1] == 65, deg[:2]
    _check_epoch("list lengths 64/65", _positions(n, 8), idx, thr, in_off,
                 in_edge, 1.0, 2, 0, 5)


@pytest.mark.gpu
def test_gpu_layout_is_deterministic():
    idx, thr, in_off, in_edge, init, _ = _layout_case(1000, 15)
    dev = "cuda"
    args = [t.to(dev) for t in (idx, thr, in_off, in_edge)]
    one = P._run_fused_epochs(init.to(dev), *args, 20, 1.0, 5, 0)
    two = P._run_fused_epochs(init.to(dev), *args, 20, 1.0, 5, 0)
    assert torch.equal(one, two)
    # the same run on buffers at other offsets inside a larger allocation
    n = init.shape[0]
    pool = torch.zeros(4 * n + 64, 2, device=dev)
    cur, nxt = pool[3:3 + n], pool[2 * n + 11:3 * n + 11]
    cur.copy_(init)
    idx32 = args[0].to(torch.int32).contiguous()
    in_thr = args[1].view(-1)[args[3].long()].contiguous()
    for epoch in range(20):
        _ext().umap_epoch(cur, nxt, idx32, args[1], args[2], args[3], in_thr,
                          1.0 * (1.0 - epoch / 20), P._A, P._B, 0, epoch, 5)
        cur, nxt = nxt, cur
    assert torch.equal(cur, one)
    assert not torch.equal(one.cpu(), init)


@pytest.mark.gpu
def test_gpu_epoch_without_sampled_edges_is_a_copy():
    idx, thr, _, _, init, _ = _layout_case(1000, 15)
    thr = torch.zeros_like(thr)
    in_off, in_edge = P.layout_reverse_lists(idx, thr)
    got = _kernel_epoch(init, idx, thr, in_off, in_edge, 1.0, 0, 0, 5)
    assert torch.equal(got, init)


@pytest.mark.gpu
def test_gpu_fused_engine_end_to_end(monkeypatch):
    x, nbrs = _twenty_centres()
    counts = {"item": 0, "cpu": 0, "loops": 0}
    real_loop = P._run_fused_epochs
    real_item, real_cpu = torch.Tensor.item, torch.Tensor.cpu

    def counting_loop(*args, **kwargs):
        def item(self, *a, **kw):
            counts["item"] += 1
            return real_item(self, *a, **kw)

        def cpu(self, *a, **kw):
            counts["cpu"] += 1
            return real_cpu(self, *a, **kw)

        counts["loops"] += 1
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "item", item)
            m.setattr(torch.Tensor, "cpu", cpu)
            return real_loop(*args, **kwargs)

    monkeypatch.setattr(P, "_run_fused_epochs", counting_loop)
    fused = P.umap_project(x.cuda(), seed=0, engine="fused")
    monkeypatch.undo()
    assert counts == {"item": 0, "cpu": 0, "loops": 1}
    assert fused.is_cuda and fused.shape == (2000, 2)
    assert torch.isfinite(fused).all()
    plain = P.umap_project(x.cuda(), seed=0, engine="torch")
    kept_fused = neighbour_preservation(nbrs, fused.cpu())
    kept_torch = neighbour_preservation(nbrs, plain.cpu())
    print(f"neighbour preservation on the GPU: fused {kept_fused:.4f} "
          f"torch {kept_torch:.4f}")
    assert kept_fused >= 0.95 * kept_torch
