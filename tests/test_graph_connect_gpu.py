"""The HIP side of the connected graph: graph_label_pull
(ops/csrc/components.hip) against its torch statement sweep by sweep, the
binding's argument checks, ivf_scan_topk_excl (ops/csrc/distance.hip)
against the unfused scan on the same device, and graph_connect.connect and
the graph song path on the GPU against the CPU run."""

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import graph_connect as GC
from audiomuse_amd.engines.path import find_path_ex
from audiomuse_amd.index.ivf import IVFIndex
from tests import test_graph_connect as T
from tests.test_graph_path_gpu import LONG_LIST, _random_graph
from tests.test_ivf import _corpus
from tests.test_ivf_scope import GPU_PAIRS

pytestmark = pytest.mark.gpu

INF = float("inf")


def _ext():
    return pytest.importorskip("audiomuse_amd._C")


# -- graph_label_pull --------------------------------------------------------

@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_label_pull_matches_reference_sweep_by_sweep(n, k):
    """30 % empty slots and, where n*k has the room, hub in-lists of 64,
    65 and 300 entries, the longest on vertex n - 1 (the construction of
    tests/test_graph_path_gpu.py). Kernel and reference run side by side
    from label[v] = v, each on its own buffers; labels and the changed
    flag are compared after each of the first 4 sweeps and at
    convergence."""
    ext = _ext()
    g = _random_graph(n, k, seed=n * 31 + k)
    deg = (g.in_off[1:] - g.in_off[:-1])
    if n * k >= 900:
        assert int(deg[n - 1]) == 300
        assert {LONG_LIST, LONG_LIST + 1} <= set(deg.tolist())
    g = g.to("cuda")
    kl = torch.arange(n, dtype=torch.int32, device="cuda")
    rl = kl.clone()
    kl2, rl2 = torch.empty_like(kl), torch.empty_like(rl)
    for sweep in range(n + 1):
        kc = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = torch.zeros(1, dtype=torch.int32, device="cuda")
        ext.graph_label_pull(kl, kl2, g.idx, g.in_off, g.in_edge, kc)
        GC.label_pull_reference(rl, rl2, g.idx, g.in_off, g.in_edge, rc)
        kl, kl2, rl, rl2 = kl2, kl, rl2, rl
        done = not bool(rc.any())
        if sweep < 4 or done:
            assert torch.equal(kl, rl), f"sweep {sweep}"
            assert torch.equal(kc, rc), f"changed, sweep {sweep}"
        if done:
            break
    else:
        raise AssertionError("no convergence")
    # the fixed point is what scipy says, and what component_labels gives
    assert torch.equal(kl.cpu(), T.scipy_labels(g.idx.cpu()))
    labels, sweeps = GC.component_labels(g.idx, g.in_off, g.in_edge)
    assert labels.is_cuda and torch.equal(labels, kl) and sweeps >= sweep + 1


def test_label_pull_changed_is_only_ever_set():
    ext = _ext()
    g = _random_graph(257, 15, seed=2).to("cuda")
    cur = torch.arange(257, dtype=torch.int32, device="cuda")
    out = torch.empty_like(cur)
    changed = torch.tensor([7], dtype=torch.int32, device="cuda")
    ext.graph_label_pull(cur, out, g.idx, g.in_off, g.in_edge, changed)
    assert changed.tolist() == [1]
    labels, _ = GC.component_labels(g.idx, g.in_off, g.in_edge)
    for start in (0, 5):
        changed = torch.tensor([start], dtype=torch.int32, device="cuda")
        ext.graph_label_pull(labels, out, g.idx, g.in_off, g.in_edge, changed)
        assert changed.tolist() == [start] and torch.equal(out, labels)


def test_label_pull_binding_rejects_bad_arguments():
    ext = _ext()
    g = _random_graph(64, 15, seed=1).to("cuda")
    n = g.n

    def args(dev="cuda"):
        lab = torch.arange(n, dtype=torch.int32, device=dev)
        return [lab, torch.empty_like(lab), g.idx, g.in_off, g.in_edge,
                torch.zeros(1, dtype=torch.int32, device=dev)]

    ext.graph_label_pull(*args())                             # the good call
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*args(dev="cpu"))
    for pos, bad in ((0, torch.int64), (1, torch.float32), (2, torch.int64),
                     (3, torch.int64), (4, torch.int16), (5, torch.int64)):
        a = args()
        a[pos] = a[pos].to(bad)
        with pytest.raises(RuntimeError):
            ext.graph_label_pull(*a)
    a = args()
    a[0] = torch.arange(2 * n, dtype=torch.int32, device="cuda")[::2]
    with pytest.raises(RuntimeError):                         # strided labels
        ext.graph_label_pull(*a)
    a = args()
    a[2] = a[2].t().contiguous().t()                          # strided idx
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    a = args()
    a[1] = a[0]                                               # in place
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    a = args()
    a[1] = a[1][:-1]                                          # label sizes
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    a = args()
    a[2] = a[2][:-1].contiguous()                             # idx rows
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    a = args()
    a[3] = a[3][:-1].contiguous()                             # in_off length
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    a = args()
    a[5] = torch.zeros(2, dtype=torch.int32, device="cuda")   # changed size
    with pytest.raises(RuntimeError):
        ext.graph_label_pull(*a)
    # n*k >= 2^31 is refused by shape alone: one stored element, expanded
    big_n, big_k = 1 << 16, 1 << 15
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = args()
    a[0] = torch.arange(big_n, dtype=torch.int32, device="cuda")
    a[1] = torch.empty_like(a[0])
    a[2] = one.expand(big_n, big_k)
    a[3] = torch.zeros(big_n + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"n\*k < 2\^31"):
        ext.graph_label_pull(*a)


# -- ivf_scan_topk_excl ------------------------------------------------------

EXCL_N, EXCL_NLIST = 900, 8


def _excl_index(metric, storage, dim):
    x = _corpus(EXCL_N, dim, seed=2)
    # packed on the CPU, so the layout does not depend on the device
    idx = IVFIndex.deserialize(
        IVFIndex.build(x, metric=metric, storage=storage, nlist=EXCL_NLIST,
                       seed=0).serialize(), device="cuda")
    assert idx.nlist == EXCL_NLIST
    return x, idx


def _label_patterns(idx, Q):
    """(name, row_labels (N,), q_labels (Q,)) on the CPU."""
    n = idx.n
    off = idx.cell_off.tolist()
    counts = [off[c + 1] - off[c] for c in range(EXCL_NLIST)]
    g = torch.Generator().manual_seed(4)
    # two labels that change in the middle of the fullest cell
    c = max(range(EXCL_NLIST), key=counts.__getitem__)
    cut = off[c] + counts[c] // 2
    assert counts[c] >= 34               # both halves span whole passes
    split = (torch.arange(n) >= cut).to(torch.int32)
    return [
        ("one label", torch.zeros(n, dtype=torch.int32),
         torch.zeros(Q, dtype=torch.int32)),
        ("all distinct", torch.arange(n, dtype=torch.int32),
         torch.randint(0, n, (Q,), generator=g, dtype=torch.int32)),
        ("split mid-cell", split,
         (torch.arange(Q) % 2).to(torch.int32)),
        ("q_label -1", split, torch.full((Q,), -1, dtype=torch.int32)),
    ]


@pytest.mark.parametrize("Q", [1, 6])
@pytest.mark.parametrize("metric,storage,dim",
                         [(m, s, 200) for m, s in GPU_PAIRS]
                         + [("angular", "i8", 20)])
def test_native_scan_topk_excl_is_the_masked_unfused_scan(metric, storage,
                                                          dim, Q):
    """scan_topk with labels on the GPU (one launch of the EXCL kernel and
    the merge of its per-split lists) against the unfused kernel on the
    same device: scan() + the label mask + _ordered_select, bit for bit."""
    _ext()
    x, idx = _excl_index(metric, storage, dim)
    g = torch.Generator().manual_seed(7)
    q = (x[:Q] + 0.05 * torch.randn(Q, dim, generator=g)).cuda()
    ref_d, ref_r = idx.scan(q, nprobe=EXCL_NLIST)
    assert int((ref_r >= 0).sum(dim=1).min()) == EXCL_N
    assert idx._topk_splits(Q, EXCL_NLIST) == EXCL_NLIST
    skip = ref_r.gather(1, ref_d.argmin(dim=1, keepdim=True))[:, 0]
    for name, rl, ql in _label_patterns(idx, Q):
        rl, ql = rl.cuda(), ql.cuda()
        same = (rl[ref_r.clamp(min=0).long()] == ql.unsqueeze(1)) \
            & (ql >= 0).unsqueeze(1)
        masked = ref_d.masked_fill(same, INF)
        skipped = masked.masked_fill(ref_r == skip.unsqueeze(1), INF)
        for kk in (1, 4, 64):
            exp_d, exp_r = IVFIndex._ordered_select(masked, ref_r, kk)
            got_d, got_r = idx.scan_topk(q, kk, nprobe=EXCL_NLIST,
                                         row_labels=rl, q_labels=ql)
            tag = f"{name} kk={kk}"
            assert got_d.shape == (Q, kk) and got_r.dtype == torch.int32, tag
            assert torch.equal(got_r, exp_r), tag
            assert torch.equal(got_d.view(torch.int32),
                               exp_d.view(torch.int32)), tag
            # combined with skip_rows
            exp_d, exp_r = IVFIndex._ordered_select(skipped, ref_r, kk)
            got_d, got_r = idx.scan_topk(q, kk, nprobe=EXCL_NLIST,
                                         row_labels=rl, q_labels=ql,
                                         skip_rows=skip)
            assert torch.equal(got_r, exp_r), tag + " skip"
            assert torch.equal(got_d.view(torch.int32),
                               exp_d.view(torch.int32)), tag + " skip"
        if name == "one label":
            assert (got_r == -1).all() and torch.isinf(got_d).all()
        if name == "q_label -1":
            pd, pr = idx.scan_topk(q, 64, nprobe=EXCL_NLIST, skip_rows=skip)
            assert torch.equal(got_r, pr) and torch.equal(got_d, pd)


def test_scan_topk_excl_binding_rejects_bad_arguments():
    ext = _ext()
    from audiomuse_amd.index.ivf import _DTYPE_CODE, _METRIC_CODE
    x, idx = _excl_index("angular", "f32", 20)
    Q, kk, S = 3, 4, 2
    q_enc, q_norm = idx._prepare_queries(x[:Q].cuda())
    probe = idx._rank_cells(q_enc, EXCL_NLIST).contiguous()

    def args():
        return [_DTYPE_CODE["f32"], _METRIC_CODE["angular"],
                q_enc.contiguous(), q_norm.contiguous(), idx.data,
                idx.row_norm, probe, idx.cell_off, None,
                torch.zeros(EXCL_N, dtype=torch.int32, device="cuda"),
                torch.ones(Q, dtype=torch.int32, device="cuda"),
                torch.empty(Q, S, kk, device="cuda"),
                torch.empty(Q, S, kk, dtype=torch.int32, device="cuda"),
                idx.dim_pad]

    ext.ivf_scan_topk_excl(*args())                           # the good call
    for pos, change in ((9, lambda t: t.long()), (10, lambda t: t.long()),
                        (9, lambda t: t.cpu()), (10, lambda t: t.cpu()),
                        (9, lambda t: t[:-1]), (10, lambda t: t[:-1]),
                        (9, lambda t: t.repeat(2)[::2])):
        a = args()
        a[pos] = change(a[pos])
        with pytest.raises(RuntimeError):
            ext.ivf_scan_topk_excl(*a)
    a = args()
    a[11] = torch.empty(Q, S, 257, device="cuda")
    a[12] = torch.empty(Q, S, 257, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        ext.ivf_scan_topk_excl(*a)


# -- connect and the graph song path on the GPU ------------------------------

def test_connect_on_the_gpu_gives_the_bridges_of_the_cpu(monkeypatch):
    _ext()
    monkeypatch.setattr(C, "PATH_GRAPH_NEIGHBOURS", T.K)
    monkeypatch.setattr(C, "IVF_GRAPH_NPROBE", T.FIXTURE_NLIST)
    monkeypatch.setattr(C, "PATH_FIX_SIZE", False)
    _, cluster, tips = T.clustered_points()
    # the CPU run, and what brute force says about the fixture
    _, c_pos, c_dists, (c_pos2, c_dists2, c_rep) = T._plain_and_connected()
    c_labels, _ = GC.component_labels(*GC.adjacency(c_pos, c_dists))
    assert c_rep["components_before"] == T.CLUSTERS
    assert np.array_equal(np.unique(cluster[c_labels.numpy() == 0]),
                          [cluster[0]])
    pairs = T.lightest_foreign_pairs(c_labels.numpy())
    tip_pairs = set()
    for lab, ((u, v), margin) in pairs.items():
        assert margin > 1e-4            # far above f32 rounding
        assert u in tips or v in tips
        if lab != 0:                    # component 0 is the one not queried
            tip_pairs.add(frozenset((u, v)))
    assert len(tip_pairs) >= 3

    eng = T.clustered_engine(device="cuda")
    assert eng.index.nlist == T.FIXTURE_NLIST
    pos, dists = eng.neighbor_graph(T.K)
    assert pos.is_cuda
    pos2, dists2, rep = GC.connect(pos, dists, eng.index, 4, 8)
    assert pos2.is_cuda and torch.equal(pos2[:, :T.K], pos)
    labels, _ = GC.component_labels(*GC.adjacency(pos2, dists2))
    assert int(labels.max()) == 0 and rep["components_after"] == 1
    assert rep["components_before"] == T.CLUSTERS
    assert rep["bridges"] == rep["components_before"] - 1
    ends = T._ends(GC.bridges_of(pos2.cpu(), dists2.cpu(), T.K))
    assert tip_pairs <= ends
    assert ends == T._ends(GC.bridges_of(c_pos2, c_dists2, T.K))

    # the engine on the GPU: off falls back, on answers with the graph
    a, b = T._two_clusters()
    _, used = find_path_ex(eng, a, b, length=500, engine="graph")
    assert used == "waypoint"
    monkeypatch.setattr(C, "PATH_GRAPH_CONNECT", True)
    items, used = find_path_ex(eng, a, b, length=500, engine="graph")
    assert used == "graph"
    got = [p["item_id"] for p in items]
    assert got[0] == a and got[-1] == b
    wide = eng.path_graph()
    assert wide.idx.is_cuda
    assert wide.idx.shape[1] == T.K + eng.graph_report()["extra_slots"]
    edges = set()
    for v, row in enumerate(wide.idx.cpu().tolist()):
        edges |= {frozenset((v, u)) for u in row if u >= 0}
    assert all(frozenset((eng.pos[s], eng.pos[t])) in edges
               for s, t in zip(got[:-1], got[1:]))
