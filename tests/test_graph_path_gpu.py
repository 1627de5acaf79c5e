"""The HIP kernels of the graph song path (ops/csrc/path.hip) against
their torch statements in engines/graph_path.py: bit-identical distances
and predecessors sweep by sweep, the allowed mask, the changed flags, the
predecessor walk, the binding's argument checks, and shortest_paths on the
GPU against the CPU."""

import functools

import pytest
import torch

from audiomuse_amd.engines import graph_path as G
from audiomuse_amd.engines import projection as P

pytestmark = pytest.mark.gpu

INF = float("inf")
LONG_LIST = 64          # path.hip: longer in-lists are walked by the wave


def _ext():
    return pytest.importorskip("audiomuse_amd._C")


def _random_graph(n, k, seed, hubs=True):
    """Raw graph tensors on the CPU: 30 % empty slots, weights drawn from
    a few repeated values (exact zeros included) and some random ones, and
    hub vertices with in-lists of LONG_LIST, LONG_LIST + 1 and 300 entries
    (the longest on vertex n - 1, in the last wave) where n*k has the
    room."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g)
    flat = idx.reshape(-1)
    want = {}
    if hubs and n * k >= 900:
        want = {n - 1: 300, n // 2: LONG_LIST, n // 3: LONG_LIST + 1}
        hub_ids = torch.tensor(sorted(want))
        # nobody else points at a hub, then hand out exactly the in-lists
        clash = torch.isin(flat, hub_ids)
        flat[clash] = 0
        perm = torch.randperm(n * k, generator=g)
        at = 0
        for h, cnt in want.items():
            flat[perm[at:at + cnt]] = h
            at += cnt
        empty = torch.rand(n * k, generator=g) < 0.3
        empty[perm[:at]] = False
    else:
        empty = torch.rand(n * k, generator=g) < 0.3
    flat[empty] = -1
    idx = flat.reshape(n, k).to(torch.int32).contiguous()
    pick = torch.tensor([0.0, 0.0, 0.25, 0.5, 0.5, 1.0, 2.0])
    w = pick[torch.randint(0, pick.numel(), (n, k), generator=g)]
    rnd = torch.rand(n, k, generator=g)
    w = torch.where(torch.rand(n, k, generator=g) < 0.3, rnd, w)
    w = torch.where(idx >= 0, w, torch.zeros_like(w)).contiguous()
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    deg = (in_off[1:] - in_off[:-1]).tolist()
    for h, cnt in want.items():
        assert deg[h] == cnt
    return G.PathGraph(idx, w, in_off.contiguous(), in_edge.contiguous(), n)


def _start(g, B, seed):
    gen = torch.Generator().manual_seed(seed + 99)
    src = torch.randint(0, g.n, (B,), generator=gen)
    dist = torch.full((B, g.n), INF)
    dist[torch.arange(B), src] = 0.0
    pred = torch.full((B, g.n), -1, dtype=torch.int32)
    return dist.cuda(), pred.cuda()


def _same(kd, kp, rd, rp, what):
    assert torch.equal(kd.view(torch.int32), rd.view(torch.int32)), what
    assert torch.equal(kp, rp), what


def _vertex_major(t):
    """The same (B, n) values on transposed (n, B) memory."""
    return t.t().contiguous().t()


def _sweep_both(ext, g, dist, pred, allowed, max_sweeps):
    """Run the kernel, in both memory layouts of its (B, n) buffers, and
    the reference side by side from the same start, each on its own
    buffers; compare after every one of the first 4 sweeps and at
    convergence. Returns the number of sweeps."""
    B = dist.shape[0]
    kd, kp, rd, rp = dist.clone(), pred.clone(), dist.clone(), pred.clone()
    kd2, kp2 = torch.empty_like(kd), torch.empty_like(kp)
    rd2, rp2 = torch.empty_like(rd), torch.empty_like(rp)
    vd, vp = _vertex_major(dist), _vertex_major(pred)
    vd2, vp2 = _vertex_major(kd2), _vertex_major(kp2)
    assert B == 1 or g.n == 1 or not vd.is_contiguous()
    for sweep in range(max_sweeps):
        kc = torch.zeros(B, dtype=torch.int32, device="cuda")
        vc = torch.zeros(B, dtype=torch.int32, device="cuda")
        rc = torch.zeros(B, dtype=torch.int32, device="cuda")
        ext.path_relax(kd, kp, kd2, kp2, g.idx, g.w, g.in_off, g.in_edge,
                       allowed, kc)
        ext.path_relax(vd, vp, vd2, vp2, g.idx, g.w, g.in_off, g.in_edge,
                       allowed, vc)
        G.relax_reference(rd, rp, rd2, rp2, g.idx, g.w, g.in_off, g.in_edge,
                          allowed, rc)
        kd, kd2, kp, kp2 = kd2, kd, kp2, kp
        vd, vd2, vp, vp2 = vd2, vd, vp2, vp
        rd, rd2, rp, rp2 = rd2, rd, rp2, rp
        done = not bool(rc.any())
        if sweep < 4 or done:
            _same(kd, kp, rd, rp, f"sweep {sweep}")
            _same(vd, vp, rd, rp, f"sweep {sweep}, vertex-major")
            assert torch.equal(kc, rc), f"changed, sweep {sweep}"
            assert torch.equal(vc, rc), f"changed, sweep {sweep}"
        if done:
            return sweep + 1
    raise AssertionError("no convergence")


@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_relax_matches_reference_bit_for_bit(n, k, B):
    ext = _ext()
    g = _random_graph(n, k, seed=n * 31 + k).to("cuda")
    dist, pred = _start(g, B, seed=n + k + B)
    sweeps = _sweep_both(ext, g, dist, pred, None, max_sweeps=n + 1)
    assert sweeps >= 1


def test_relax_with_allowed_mask():
    ext = _ext()
    g = _random_graph(1000, 15, seed=5)
    src = 17
    allowed = (torch.rand(g.n, generator=torch.Generator().manual_seed(8))
               < 0.7).to(torch.uint8)
    allowed[src] = 1
    gc = g.to("cuda")
    dist = torch.full((2, g.n), INF)
    dist[:, src] = 0.0
    pred = torch.full((2, g.n), -1, dtype=torch.int32)
    _sweep_both(ext, gc, dist.cuda(), pred.cuda(), allowed.cuda(), g.n + 1)
    # the source's only neighbours (both directions) masked: nothing else
    # is ever reached
    shut = torch.ones(g.n, dtype=torch.uint8)
    own = g.idx[src][g.idx[src] >= 0].long()
    shut[own] = 0
    heads = g.in_edge[int(g.in_off[src]):int(g.in_off[src + 1])].long() // 15
    shut[heads] = 0
    shut[src] = 1
    kd, kp = dist.cuda(), pred.cuda()
    kd2, kp2 = torch.empty_like(kd), torch.empty_like(kp)
    changed = torch.zeros(2, dtype=torch.int32, device="cuda")
    for _ in range(3):
        ext.path_relax(kd, kp, kd2, kp2, gc.idx, gc.w, gc.in_off, gc.in_edge,
                       shut.cuda(), changed)
        kd, kd2, kp, kp2 = kd2, kd, kp2, kp
    want = torch.full((g.n,), INF)
    want[src] = 0.0
    assert torch.equal(kd[0].cpu(), want) and torch.equal(kd[1].cpu(), want)
    assert (kp == -1).all() and changed.tolist() == [0, 0]


def test_changed_is_set_only_for_legs_that_improved():
    ext = _ext()
    g = _random_graph(257, 15, seed=2).to("cuda")
    B = 4
    dist = torch.full((B, g.n), INF)
    dist[0, 3] = 0.0
    dist[2, 200] = 0.0                  # legs 1 and 3 have no source
    pred = torch.full((B, g.n), -1, dtype=torch.int32)
    dist, pred = dist.cuda(), pred.cuda()
    out_d, out_p = torch.empty_like(dist), torch.empty_like(pred)
    changed = torch.tensor([0, 5, 7, 0], dtype=torch.int32, device="cuda")
    ext.path_relax(dist, pred, out_d, out_p, g.idx, g.w, g.in_off, g.in_edge,
                   None, changed)
    assert changed.tolist() == [1, 5, 1, 0]
    assert torch.isinf(out_d[1]).all() and torch.isinf(out_d[3]).all()


def test_walk_matches_reference():
    ext = _ext()
    T = 6
    n = T + 3
    # leg 0: a chain of exactly T hops 0 <- 1 <- ... <- T; leg 1: an
    # unreachable target; leg 2: source = target; leg 3: a chain longer
    # than the buffer stops after T + 1 entries
    dist = torch.full((4, n), INF)
    pred = torch.full((4, n), -1, dtype=torch.int32)
    for b in (0, 3):
        for v in range(n - 1):
            dist[b, v] = float(v)
            pred[b, v] = v - 1
    dist[1, 0] = 0.0
    dist[2, 4] = 0.0
    src = torch.tensor([0, 0, 4, 0], dtype=torch.int32)
    dst = torch.tensor([T, 5, 4, T + 1], dtype=torch.int32)
    ref_out = torch.empty(4, T + 1, dtype=torch.int32)
    ref_cnt = torch.empty(4, dtype=torch.int32)
    G.walk_reference(dist, pred, src, dst, ref_out, ref_cnt)
    assert ref_cnt.tolist() == [T + 1, -1, 1, T + 1]
    assert ref_out[0].tolist() == list(range(T, -1, -1))
    assert ref_out[1].tolist() == [-1] * (T + 1)
    assert ref_out[3].tolist() == list(range(T + 1, 0, -1))
    out = torch.full((4, T + 1), 77, dtype=torch.int32, device="cuda")
    cnt = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    ext.path_walk(dist.cuda(), pred.cuda(), src.cuda(), dst.cuda(), out, cnt)
    assert torch.equal(out.cpu(), ref_out) and torch.equal(cnt.cpu(), ref_cnt)
    out.fill_(77)
    cnt.fill_(77)
    ext.path_walk(_vertex_major(dist.cuda()), _vertex_major(pred.cuda()),
                  src.cuda(), dst.cuda(), out, cnt)
    assert torch.equal(out.cpu(), ref_out) and torch.equal(cnt.cpu(), ref_cnt)


def test_binding_rejects_bad_arguments():
    ext = _ext()
    g = _random_graph(64, 15, seed=1).to("cuda")
    n = g.n

    def args(B=2, dev="cuda"):
        d = torch.full((B, n), INF, device=dev)
        p = torch.full((B, n), -1, dtype=torch.int32, device=dev)
        return [d, p, torch.empty_like(d), torch.empty_like(p), g.idx, g.w,
                g.in_off, g.in_edge, None,
                torch.zeros(B, dtype=torch.int32, device=dev)]

    ext.path_relax(*args())                                   # the good call
    with pytest.raises(RuntimeError):
        ext.path_relax(*args(dev="cpu"))
    for pos, bad in ((0, torch.float64), (1, torch.int64), (4, torch.int64),
                     (5, torch.float16), (6, torch.int64), (9, torch.int64)):
        a = args()
        a[pos] = a[pos].to(bad)
        with pytest.raises(RuntimeError):
            ext.path_relax(*a)
    a = args()
    a[8] = torch.ones(n, dtype=torch.int32, device="cuda")    # mask dtype
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    a = args()
    a[2] = a[0]                                               # in place
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    a = args()
    both = torch.empty(2 * 2 * n - n, device="cuda")
    a[0] = both[:2 * n].view(2, n)
    a[0].fill_(INF)
    a[2] = both[n:].view(2, n)                                # partial overlap
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    a = args()
    a[3] = a[1]
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    for B in (0, 9):
        with pytest.raises(RuntimeError):
            ext.path_relax(*args(B=B))
    a = args()
    a[0] = a[0].t().contiguous().t()                          # mixed layouts
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    a = args()
    a[0] = torch.full((2, 2 * n), INF, device="cuda")[:, ::2]   # strided
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    a = args()
    for i in range(4):                                        # all transposed
        a[i] = a[i].t().contiguous().t()
    ext.path_relax(*a)
    a = args()
    a[6] = a[6][:-1].contiguous()                             # in_off length
    with pytest.raises(RuntimeError):
        ext.path_relax(*a)
    d, p = args()[:2]
    s = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.empty(2, 4, dtype=torch.int32, device="cuda")
    ext.path_walk(d, p, s, s, out, s.clone())
    with pytest.raises(RuntimeError):
        ext.path_walk(d.cpu(), p, s, s, out, s.clone())
    with pytest.raises(RuntimeError):
        ext.path_walk(d, p.long(), s, s, out, s.clone())
    with pytest.raises(RuntimeError):
        ext.path_walk(d, p, s[:1], s, out, s.clone())
    with pytest.raises(RuntimeError):
        ext.path_walk(d, p, s, s, out[:1], s.clone())


@functools.lru_cache(maxsize=None)
def _knn_path_graph():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(500, 16, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    d, i = P.knn_graph(x, 15)
    return G.PathGraph.from_knn(i, d, 2.0)


def test_shortest_paths_gpu_equals_cpu():
    _ext()
    g = _knn_path_graph()
    assert g.device.type == "cpu"
    src, dst = [0, 17, 400], [250, 499, 3]
    cp, cd, cs = G.shortest_paths(g, src, dst)
    gp, gd, gs = G.shortest_paths(g.to("cuda"), src, dst)
    assert all(p is not None and len(p) >= 2 for p in cp)
    assert gp == cp and gs == cs
    assert torch.equal(gd.view(torch.int32), cd.view(torch.int32))
    allowed = torch.ones(g.n, dtype=torch.uint8)
    for p in cp:
        allowed[p[1:-1]] = 0                 # close the routes just found
    cp2, cd2, _ = G.shortest_paths(g, src, dst, allowed)
    gp2, gd2, _ = G.shortest_paths(g.to("cuda"), src, dst, allowed.cuda())
    assert gp2 == cp2 and cp2 != cp
    assert torch.equal(gd2.view(torch.int32), cd2.view(torch.int32))
