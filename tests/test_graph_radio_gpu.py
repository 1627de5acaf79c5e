"""The HIP kernel of the graph radio (ops/csrc/rank.hip) against its torch
statement, engines/graph_radio.pull_reference: the sweep and the degree
pass to a derived tolerance, bit-identical repeats, the binding's argument
checks, and graph_radio on the GPU against the CPU.

Tolerance. A vertex sums at most m_max nonnegative f32 terms (m_max = the
graph's largest candidate count), each one FMA, in some order: a relative
error of at most m_max * 2^-24 to first order; the epilogue adds at most
four more roundings ((1 - alpha) * r, the FMA, p * inv_deg and the
reference's own rounding to f32). An error in the inputs of a sweep goes
through it unamplified (all terms are nonnegative), so t sweeps compound
to rtol = t * (m_max + 4) * 2^-23, with a factor 2 to spare. Below f32's
normal range a flush to zero costs up to 2^-126 per term: atol = t *
(m_max + 4) * 2^-126."""

import functools

import pytest
import torch

from audiomuse_amd.engines import graph_radio as R
from audiomuse_amd.engines import projection as P

pytestmark = pytest.mark.gpu

LONG_LIST = 64          # rank.hip: longer in-lists are walked by the wave
ALPHA = 0.85
T = R.sweep_count(ALPHA, 1e-3, 200)


def _ext():
    return pytest.importorskip("audiomuse_amd._C")


@functools.lru_cache(maxsize=None)
def _random_graph(n, k, seed=0, hubs=True):
    """A RankGraph on the CPU: 30 % empty slots, affinities in (0, 1] drawn
    from a few repeated values and some random ones, self-slots and
    repeated slots as they fall, and hub vertices with in-lists of
    LONG_LIST, LONG_LIST + 1 and 300 entries (the longest on vertex n - 1,
    in the last wave) where n*k has the room."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + k)
    flat = torch.randint(0, n, (n * k,), generator=g)
    want = {}
    empty = torch.rand(n * k, generator=g) < 0.3
    if hubs and n * k >= 900:
        want = {n - 1: 300, n // 2: LONG_LIST, n // 3: LONG_LIST + 1}
        # nobody else points at a hub, then hand out exactly the in-lists
        flat[torch.isin(flat, torch.tensor(sorted(want)))] = 0
        perm = torch.randperm(n * k, generator=g)
        at = 0
        for h, cnt in want.items():
            flat[perm[at:at + cnt]] = h
            at += cnt
        empty[perm[:at]] = False
    flat[empty] = -1
    idx = flat.reshape(n, k).to(torch.int32).contiguous()
    pick = torch.tensor([1.0, 1.0, 0.5, 0.25, 0.75, 0.01])
    s = pick[torch.randint(0, pick.numel(), (n, k), generator=g)]
    rnd = 1.0 - torch.rand(n, k, generator=g)
    s = torch.where(torch.rand(n, k, generator=g) < 0.5, rnd, s)
    s = torch.where(idx >= 0, s, torch.zeros_like(s)).contiguous()
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    lens = (in_off[1:] - in_off[:-1]).tolist()
    for h, cnt in want.items():
        assert lens[h] == cnt
    return R.RankGraph(idx, s, in_off.contiguous(), in_edge.contiguous(), n)


def _m_max(g):
    own = (g.idx >= 0).sum(dim=1)
    return int((own + (g.in_off[1:] - g.in_off[:-1]).to(own.dtype)).max())


def _restart(n, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.zeros(B, n)
    for b in range(B):
        at = torch.randperm(n, generator=g)[:min(1 + b % 4, n)]
        w = 0.1 + torch.rand(at.numel(), generator=g)
        r[b, at] = w / w.sum()
    return r


def _vertex_major(t):
    """The same (B, n) values on transposed (n, B) memory."""
    return t.t().contiguous().t()


def _close(got, want, t, m_max, what):
    unit = t * (m_max + 4)
    torch.testing.assert_close(got, want, rtol=unit * 2.0 ** -23,
                               atol=unit * 2.0 ** -126, msg=lambda m: f"{what}: {m}")


def _degrees(g, allowed):
    """deg and 1 / deg from the reference, on the graph's device."""
    x = (torch.ones(1, g.n, device=g.device) if allowed is None
         else allowed.float().unsqueeze(0))
    deg = torch.empty(1, g.n, device=g.device)
    R.pull_reference(x, deg, None, None, None, g.idx, g.s, g.in_off,
                     g.in_edge, allowed, 0.0)
    deg = deg[0]
    return deg, torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))


def _sweep_both(ext, g, r, allowed, sweeps, m_max):
    """Run the kernel, in both memory layouts of its (B, n) buffers, and
    the reference side by side from the same start, each on its own
    buffers; compare p and q after each of the first 4 sweeps and after
    the last."""
    _, inv = _degrees(g, allowed)
    if allowed is not None:
        r = r * allowed.unsqueeze(0)
    q0 = r * inv.unsqueeze(0)
    B = r.shape[0]
    kq, kq2, kp = q0.clone(), torch.empty_like(q0), torch.empty_like(q0)
    rq, rq2, rp = q0.clone(), torch.empty_like(q0), torch.empty_like(q0)
    vr = _vertex_major(r)
    vq, vq2, vp = (_vertex_major(q0), _vertex_major(kq2), _vertex_major(kp))
    assert B == 1 or g.n == 1 or not vq.is_contiguous()
    for sweep in range(1, sweeps + 1):
        ext.rank_pull(kq, kp, kq2, r, inv, g.idx, g.s, g.in_off, g.in_edge,
                      allowed, ALPHA)
        ext.rank_pull(vq, vp, vq2, vr, inv, g.idx, g.s, g.in_off, g.in_edge,
                      allowed, ALPHA)
        R.pull_reference(rq, rp, rq2, r, inv, g.idx, g.s, g.in_off,
                         g.in_edge, allowed, ALPHA)
        kq, kq2 = kq2, kq
        vq, vq2 = vq2, vq
        rq, rq2 = rq2, rq
        if sweep <= 4 or sweep == sweeps:
            _close(kp, rp, sweep, m_max, f"p, sweep {sweep}")
            _close(kq, rq, sweep, m_max, f"q, sweep {sweep}")
            _close(vp.contiguous(), rp, sweep, m_max,
                   f"p, sweep {sweep}, vertex-major")
            _close(vq.contiguous(), rq, sweep, m_max,
                   f"q, sweep {sweep}, vertex-major")
    return kp, rp


@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_pull_matches_reference(n, k, B):
    ext = _ext()
    cpu = _random_graph(n, k)
    m_max = _m_max(cpu)
    if n * k >= 900:
        assert m_max >= 300
    g = cpu.to("cuda")
    r = _restart(n, B, seed=n + k + B).cuda()
    kp, rp = _sweep_both(ext, g, r, None, T, m_max)
    assert bool((rp >= 0).all()) and float(rp.sum()) > 0


def test_pull_with_allowed_mask():
    ext = _ext()
    cpu = _random_graph(1000, 15)
    g = cpu.to("cuda")
    allowed = (torch.rand(g.n, generator=torch.Generator().manual_seed(8))
               < 0.7).to(torch.uint8).cuda()
    r = _restart(g.n, 3, seed=4).cuda()
    kp, rp = _sweep_both(ext, g, r, allowed, T, _m_max(cpu))
    assert bool((kp[:, allowed == 0] == 0).all())
    assert float(kp.sum()) > 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,k", [(1, 1), (65, 1), (257, 15), (1000, 15)])
def test_degree_pass(n, k, masked):
    ext = _ext()
    cpu = _random_graph(n, k)
    g = cpu.to("cuda")
    allowed = None
    if masked:
        allowed = (torch.rand(n, generator=torch.Generator().manual_seed(3))
                   < 0.7).to(torch.uint8).cuda()
    want, _ = _degrees(g, allowed)
    x = (torch.ones(1, n, device="cuda") if allowed is None
         else allowed.float().unsqueeze(0))
    got = torch.full((1, n), -1.0, device="cuda")
    ext.rank_pull(x, got, None, None, None, g.idx, g.s, g.in_off, g.in_edge,
                  allowed, 0.0)
    _close(got[0], want, 1, _m_max(cpu), "degree")
    if masked:
        assert bool((got[0][allowed == 0] == 0).all())
    # the engine's degrees() is that call
    assert torch.equal(R.degrees(g, allowed), got[0])
    # several legs at once, vertex-major: leg b sums b + 1 times the ones
    x3 = _vertex_major(x * torch.tensor([[1.0], [2.0], [3.0]], device="cuda"))
    got3 = _vertex_major(torch.empty(3, n, device="cuda"))
    ext.rank_pull(x3, got3, None, None, None, g.idx, g.s, g.in_off,
                  g.in_edge, allowed, 0.0)
    _close(got3.contiguous(), torch.stack([want, 2 * want, 3 * want]),
           1, _m_max(cpu), "degree, 3 legs")


@pytest.mark.parametrize("inner", [False, True])
def test_repeats_are_bit_identical(inner):
    ext = _ext()
    g = _random_graph(1000, 15).to("cuda")
    _, inv = _degrees(g, None)
    r = _restart(g.n, 8, seed=6).cuda()
    if inner:
        r = _vertex_major(r)

    def run():
        q = r * inv.unsqueeze(0)
        q2, p = torch.empty_like(q), torch.empty_like(q)
        assert (not q.is_contiguous()) == inner
        for _ in range(10):
            ext.rank_pull(q, p, q2, r, inv, g.idx, g.s, g.in_off, g.in_edge,
                          None, ALPHA)
            q, q2 = q2, q
        return p.contiguous(), q.contiguous()

    p1, q1 = run()
    p2, q2 = run()
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert torch.equal(q1.view(torch.int32), q2.view(torch.int32))
    assert float(p1.sum()) > 0


def test_binding_rejects_bad_arguments():
    ext = _ext()
    g = _random_graph(64, 15).to("cuda")
    n = g.n

    def args(B=2, dev="cuda"):
        x = torch.zeros(B, n, device=dev)
        return [x, torch.empty_like(x), torch.empty_like(x),
                torch.zeros_like(x), torch.ones(n, device=dev), g.idx, g.s,
                g.in_off, g.in_edge, None, ALPHA]

    ext.rank_pull(*args())                                    # the good call
    with pytest.raises(RuntimeError):
        ext.rank_pull(*args(dev="cpu"))
    for pos, bad in ((0, torch.float64), (1, torch.float64),
                     (2, torch.float16), (3, torch.float64),
                     (4, torch.float64), (5, torch.int64),
                     (6, torch.float16), (7, torch.int64), (8, torch.int64)):
        a = args()
        a[pos] = a[pos].to(bad)
        with pytest.raises(RuntimeError):
            ext.rank_pull(*a)
    a = args()
    a[9] = torch.ones(n, dtype=torch.int32, device="cuda")    # mask dtype
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    a[9] = torch.ones(n + 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    a[9] = torch.ones(n, dtype=torch.uint8, device="cuda")
    ext.rank_pull(*a)
    for out, src in ((1, 0), (2, 0), (1, 3), (2, 3), (2, 1)):  # in place
        a = args()
        a[out] = a[src]
        with pytest.raises(RuntimeError):
            ext.rank_pull(*a)
    a = args()
    both = torch.zeros(2 * 2 * n - n, device="cuda")
    a[0] = both[:2 * n].view(2, n)
    a[2] = both[n:].view(2, n)                                # partial overlap
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    a = args()
    a[4] = a[1][0]                                            # inv_deg in p_out
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    for B in (0, 9):
        with pytest.raises(RuntimeError):
            ext.rank_pull(*args(B=B))
    for pos in (0, 1, 2, 3):                                  # mixed layouts
        a = args()
        a[pos] = _vertex_major(a[pos])
        with pytest.raises(RuntimeError):
            ext.rank_pull(*a)
    a = args()
    a[0] = torch.zeros(2, 2 * n, device="cuda")[:, ::2]       # strided
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    a = args()
    for i in range(4):                                        # all transposed
        a[i] = _vertex_major(a[i])
    ext.rank_pull(*a)
    a[0] = torch.zeros(2 * n + 1, device="cuda")[1:].view(n, 2).t()
    with pytest.raises(RuntimeError):                         # 4 bytes off
        ext.rank_pull(*a)
    a = args()
    a[0] = torch.zeros(2 * n + 1, device="cuda")[1:].view(2, n)
    ext.rank_pull(*a)                           # leg-major needs no alignment
    for alpha in (-0.1, 1.0, 1.0 - 1e-12, float("nan")):
        a = args()
        a[10] = alpha
        with pytest.raises(RuntimeError):
            ext.rank_pull(*a)
    a = args()
    a[10] = 0.0
    ext.rank_pull(*a)
    a = args()
    a[7] = a[7][:-1].contiguous()                             # in_off length
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    a = args()
    a[8] = torch.zeros(n * 15 + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):                         # in_edge length
        ext.rank_pull(*a)
    a = args()
    a[6] = a[6][:, :-1].contiguous()                          # s is not (n, k)
    with pytest.raises(RuntimeError):
        ext.rank_pull(*a)
    # q_out, restart and inv_deg go together
    for gone in ((2,), (3,), (4,), (2, 3), (3, 4)):
        a = args()
        for pos in gone:
            a[pos] = None
        with pytest.raises(RuntimeError):
            ext.rank_pull(*a)
    a = args()
    a[2] = a[3] = a[4] = None
    ext.rank_pull(*a)
    # n * k = 2^31, on tensors that hold no such memory
    big_n, big_k = 1 << 16, 1 << 15
    x = torch.zeros(1, big_n, device="cuda")
    with pytest.raises(RuntimeError, match="2\\^31"):
        ext.rank_pull(
            x, torch.empty_like(x), None, None, None,
            torch.zeros(1, 1, dtype=torch.int32,
                        device="cuda").expand(big_n, big_k),
            torch.zeros(1, 1, device="cuda").expand(big_n, big_k),
            torch.zeros(big_n + 1, dtype=torch.int32, device="cuda"),
            torch.zeros(0, dtype=torch.int32, device="cuda"), None, 0.0)


def test_pagerank_gpu_matches_cpu_reference():
    _ext()
    cpu = _random_graph(1000, 15)
    r = _restart(cpu.n, 2, seed=9)
    want = R.personalized_pagerank(cpu, r, ALPHA, T)
    got = R.personalized_pagerank(cpu.to("cuda"), r.cuda(), ALPHA, T)
    assert got.is_cuda and got.shape == want.shape
    _close(got.cpu().contiguous(), want.contiguous(), T + 1, _m_max(cpu),
           "personalized_pagerank")


def test_graph_radio_gpu_equals_cpu():
    _ext()
    import numpy as np

    from audiomuse_amd.engines.similarity import build_engine_from_matrix

    # the catalogue of tests/test_graph_radio.py: two tastes A and B, the
    # region C between them, bridges; generator seed 0 (the gap between
    # ranks 20 and 21 depends on it, hence the asserted precondition)
    gen = torch.Generator().manual_seed(0)
    e0, e1 = torch.eye(16)[0], torch.eye(16)[1]
    mid = (e0 + e1) / (e0 + e1).norm()
    parts = [c + 0.35 * torch.randn(150, 16, generator=gen) / 4
             for c in (e0, e1, mid)]
    t = torch.linspace(0, 1, 22)[1:-1].unsqueeze(1)
    for a, b in ((e0, mid), (mid, e1)):
        parts.append((1 - t) * a + t * b
                     + 0.25 * torch.randn(20, 16, generator=gen) / 4)
    x = torch.cat(parts)
    x = x / x.norm(dim=1, keepdim=True)
    d, i = P.knn_graph(x, 15)
    graph = R.RankGraph.from_knn(i, d, 1.0)
    ids = [f"s{j}" for j in range(x.shape[0])]
    eng = build_engine_from_matrix(x.numpy().astype(np.float32), ids,
                                   metric="angular")
    seeds = [f"s{j}" for j in (0, 1, 2, 3, 4, 150, 151, 152, 153, 154)]
    sub = [f"s{j}" for j in (155, 156, 157, 158, 159)]
    rtol = T * (_m_max(graph) + 4) * 2.0 ** -23
    for kw in ({}, {"subtract_ids": sub}):
        eng.rank_graph = lambda: graph
        c_items, c_used = R.graph_radio(eng, seeds, n=21, engine="graph", **kw)
        s = [it["score"] for it in c_items]
        assert c_used == "graph" and len(s) == 21
        if not kw:      # the top 20 are apart from the rest by far more
            assert (s[19] - s[20]) / s[19] > 2 * rtol    # than the rounding
        eng.rank_graph = lambda: graph.to("cuda")
        g_items, g_used = R.graph_radio(eng, seeds, n=20, engine="graph", **kw)
        assert g_used == c_used
        if not kw:
            assert {it["item_id"] for it in g_items} == \
                {it["item_id"] for it in c_items[:20]}
            for gi, ci in zip(g_items, c_items):
                if gi["item_id"] == ci["item_id"]:
                    assert gi["score"] == pytest.approx(ci["score"],
                                                        rel=2 * rtol)
        else:
            assert len(g_items) == 20
