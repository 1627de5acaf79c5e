"""The HIP kernel of the graph communities (ops/csrc/community.hip) against
its torch statement, engines/graph_community.move_reference, and the whole
solve on the GPU against the CPU. Every sum in the rule is an integer sum,
so every comparison here is torch.equal: there is no tolerance."""

import functools

import pytest
import torch

from audiomuse_amd.engines import graph_community as G
from audiomuse_amd.engines import projection as P

pytestmark = pytest.mark.gpu

LONG_LIST = 64          # community.hip: longer in-lists are walked by the wave


def _ext():
    return pytest.importorskip("audiomuse_amd._C")


@functools.lru_cache(maxsize=None)
def _random_graph(n, k, seed=0):
    """A CommunityGraph on the CPU, the graph of test_graph_radio_gpu with
    integer weights: 30 % empty slots, weights in 1..256, self-slots and
    repeated slots as they fall, and hub vertices with in-lists of
    LONG_LIST, LONG_LIST + 1 and 300 entries (the longest on vertex n - 1,
    in the last wave) where n*k has the room."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + k)
    flat = torch.randint(0, n, (n * k,), generator=g)
    want = {}
    empty = torch.rand(n * k, generator=g) < 0.3
    if n * k >= 900:
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
    w = torch.randint(1, 257, (n, k), generator=g).to(torch.int32)
    w = torch.where(idx >= 0, w, torch.zeros_like(w)).contiguous()
    in_off, in_edge = P.layout_reverse_lists(idx, (idx >= 0).to(torch.int32))
    lens = (in_off[1:] - in_off[:-1]).tolist()
    for h, cnt in want.items():
        assert lens[h] == cnt
    return G.CommunityGraph(idx, w, in_off.contiguous(), in_edge.contiguous(),
                            n)


def _label_states(n, seed):
    """Singletons, and labels drawn from 7 vertex ids, where a community
    collects many entries of a vertex and tot is large."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randperm(n, generator=g)[:7]
    few = vals[torch.randint(0, vals.numel(), (n,), generator=g)]
    return {"singletons": torch.arange(n, dtype=torch.int32),
            "seven": few.to(torch.int32)}


@pytest.mark.parametrize("k", [1, 15, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_move_matches_reference(n, k):
    ext = _ext()
    cpu = _random_graph(n, k)
    if n * k >= 900:
        assert int((cpu.in_off[1:] - cpu.in_off[:-1]).max()) == 300
    gr = cpu.to("cuda")
    deg = G.degrees(gr)
    assert torch.equal(deg.cpu(), G.degrees(cpu))
    A = G.RESOLUTION_UNIT * max(int(deg.sum()), 1)
    moved = 0
    for name, label in _label_states(n, seed=n + k).items():
        label = label.cuda()
        tot = torch.zeros_like(deg).index_add_(0, label.long(), deg)
        for g in (16, 64, 256):
            for up in (False, True):
                got = torch.full_like(label, -7)
                want = torch.full_like(label, -9)
                ext.community_move(label, got, tot, deg, gr.idx, gr.w,
                                   gr.in_off, gr.in_edge, A, g, up)
                G.move_reference(label, want, tot, deg, gr.idx, gr.w,
                                 gr.in_off, gr.in_edge, A, g, up)
                assert torch.equal(got, want), (name, g, up, int(
                    (got != want).sum()))
                assert bool(((want >= label) if up else (want <= label)).all())
                moved += int((want != label).sum())
    if n >= 63 and k >= 15:
        assert moved > 0        # the comparison is not of two idle sweeps


def test_reference_is_the_same_on_both_devices():
    cpu = _random_graph(1000, 15)
    gr = cpu.to("cuda")
    deg = G.degrees(cpu)
    A = G.RESOLUTION_UNIT * int(deg.sum())
    for label in _label_states(1000, seed=3).values():
        tot = torch.zeros_like(deg).index_add_(0, label.long(), deg)
        want = torch.empty_like(label)
        G.move_reference(label, want, tot, deg, cpu.idx, cpu.w, cpu.in_off,
                         cpu.in_edge, A, 64, True)
        got = torch.empty_like(label).cuda()
        G.move_reference(label.cuda(), got, tot.cuda(), deg.cuda(), gr.idx,
                         gr.w, gr.in_off, gr.in_edge, A, 64, True)
        assert torch.equal(got.cpu(), want)


def test_binding_rejects_bad_arguments():
    ext = _ext()
    gr = _random_graph(64, 15).to("cuda")
    n = gr.n
    deg = G.degrees(gr)
    A = G.RESOLUTION_UNIT * int(deg.sum())

    def args(graph=gr):
        m = graph.n
        lab = torch.arange(m, dtype=torch.int32, device="cuda")
        d = deg if graph is gr else G.degrees(graph)
        return [lab, torch.empty_like(lab), d.clone(), d, graph.idx, graph.w,
                graph.in_off, graph.in_edge, A, 64, True]

    ext.community_move(*args())                               # the good call
    a = [t.cpu() if torch.is_tensor(t) else t for t in args()]
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    for pos, bad in ((0, torch.int64), (1, torch.int64), (2, torch.int32),
                     (3, torch.int32), (4, torch.int64), (5, torch.int64),
                     (5, torch.float32), (6, torch.int64), (7, torch.int64)):
        a = args()
        a[pos] = a[pos].to(bad)
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    for pos in (0, 2, 3, 4, 5, 6, 7):                         # aliased output
        a = args()
        if a[pos].element_size() == 4 and a[pos].dim() == 1 \
                and a[pos].numel() >= n:
            a[1] = a[pos][:n]
        else:                   # int32 words inside the input's memory
            a[1] = a[pos].view(-1).view(torch.int32)[:n]
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    a = args()
    both = torch.zeros(2 * n - 1, dtype=torch.int32, device="cuda")
    a[0], a[1] = both[:n], both[n - 1:]                       # one word shared
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    for pos in (0, 1):                                        # strided labels
        a = args()
        a[pos] = torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    for pos in (2, 3):                                        # strided sums
        a = args()
        a[pos] = torch.zeros(2 * n, dtype=torch.int64, device="cuda")[::2]
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    a = args()
    a[4] = a[4].t().contiguous().t()                          # idx transposed
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    for pos, shape in ((1, n + 1), (2, n - 1), (3, n + 1)):   # lengths
        a = args()
        a[pos] = torch.zeros(shape, dtype=a[pos].dtype, device="cuda")
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    a = args()
    a[5] = a[5][:, :-1].contiguous()                          # w is not (n, k)
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    a = args()
    a[6] = a[6][:-1].contiguous()                             # in_off length
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    a = args()
    a[7] = torch.zeros(n * 15 + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):                         # in_edge length
        ext.community_move(*a)
    for A_bad in (0, -1):
        a = args()
        a[8] = A_bad
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    for g_bad in (0, -64):
        a = args()
        a[9] = g_bad
        with pytest.raises(RuntimeError):
            ext.community_move(*a)
    ext.community_move(*args(_random_graph(64, 32).to("cuda")))
    with pytest.raises(RuntimeError, match="k <= 32"):
        ext.community_move(*args(_random_graph(64, 33).to("cuda")))
    wide = torch.zeros(n, 0, dtype=torch.int32, device="cuda")
    a = args()
    a[4] = a[5] = wide                                        # k = 0
    with pytest.raises(RuntimeError):
        ext.community_move(*a)
    # n * k = 2^31: the table is a view that holds no such memory
    big_n = 1 << 26
    lab = torch.empty(big_n, dtype=torch.int32, device="cuda")
    sums = torch.empty(big_n, dtype=torch.int64, device="cuda")
    one = torch.zeros(1, 1, dtype=torch.int32, device="cuda").expand(big_n, 32)
    with pytest.raises(RuntimeError, match="2\\^31"):
        ext.community_move(
            lab, torch.empty_like(lab), sums, sums, one, one,
            torch.empty(big_n + 1, dtype=torch.int32, device="cuda"),
            torch.zeros(0, dtype=torch.int32, device="cuda"), A, 64, True)


def test_wide_tables_take_the_reference():
    _ext()
    cpu = _random_graph(257, 33)
    want = G.local_move(cpu, 1.0, 20)
    got = G.local_move(cpu.to("cuda"), 1.0, 20)
    assert torch.equal(got[0].cpu(), want[0]) and got[1:] == want[1:]


def _planted(noise, seed):
    """8 unit-norm centres in 16-d, 250 points each, angular kNN, k = 15:
    the catalogue of tests/test_graph_community.py."""
    gen = torch.Generator().manual_seed(seed)
    c = torch.randn(8, 16, generator=gen)
    c = c / c.norm(dim=1, keepdim=True)
    x = torch.cat([ci + noise * torch.randn(250, 16, generator=gen) / 4
                   for ci in c])
    x = x / x.norm(dim=1, keepdim=True)
    return x


def _strip(report):
    return {k: v for k, v in report.items() if k != "seconds"}


@pytest.mark.parametrize("noise", [0.4, 1.0])
def test_communities_gpu_equals_cpu(noise):
    _ext()
    x = _planted(noise, seed=0)
    d, i = P.knn_graph(x, 15)
    cpu = G.CommunityGraph.from_knn(i, d, 1.0, 256)
    want, wrep = G.communities(cpu, 1.0, 100, 10)
    got, grep = G.communities(cpu.to("cuda"), 1.0, 100, 10)
    assert got.is_cuda and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want)
    assert grep["levels"] == wrep["levels"]
    assert _strip(grep) == _strip(wrep)       # modularity is the same f64
    assert wrep["communities"] >= 2 and wrep["levels"][0]["sweeps"] > 2


def test_engine_communities_match_cpu():
    _ext()
    import numpy as np

    from audiomuse_amd.engines.similarity import build_engine_from_matrix

    x = _planted(0.4, seed=1)[::2].contiguous()               # 1 000 tracks
    ids = [f"s{j}" for j in range(x.shape[0])]
    eng = build_engine_from_matrix(x.numpy().astype(np.float32), ids,
                                   metric="angular", device="cuda")
    graph = eng.community_graph()
    assert graph.device.type == "cuda" and graph.n == 1000
    labels, report = eng.communities()
    assert labels.shape == (1000,) and labels.is_cuda
    # the same table on the CPU: the torch statement, no kernel
    want, wrep = G.communities(graph.to("cpu"), 1.0, 100, 10)
    assert torch.equal(labels.cpu(), want)
    assert report["levels"] == wrep["levels"]
    assert report["communities"] >= 2
    again, _ = eng.communities()
    assert again is labels                                    # kept
    finer, frep = eng.communities(resolution=4.0)         # its own entry
    assert finer is not labels and finer.shape == labels.shape
