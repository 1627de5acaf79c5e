"""Graph communities: Louvain over the kNN graph.

Playlists as sets of tracks that are each other's neighbours: the
whole-catalogue neighbour graph (SimilarityEngine.neighbor_graph) is
partitioned by modularity, with no cluster count and no sampled subset.
The graph is the symmetrised multigraph the graph radio walks, with integer
weights round(levels * exp(-d / sigma)) on the edges, so every sum in the
rule is an integer sum: the HIP kernel (ops/csrc/community.hip), its torch
statement move_reference below, the CPU and the GPU agree bit for bit.

Level 0 is a synchronous local-moving sweep over the (n, k) table, one HIP
launch per sweep; the coarse levels (communities as vertices) are small
and run the same rule in torch on a COO edge list (docs/ALGORITHM.md
"Graph communities").
"""

from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Tuple

import torch

from audiomuse_amd.engines.projection import layout_reverse_lists

MAX_KERNEL_K = 32       # community.hip holds k + 1 (label, sum) pairs a lane
RESOLUTION_UNIT = 64    # gamma = g / 64
MAX_SHIFT = 31
_I64_MIN = -(1 << 63)


@dataclass
class CommunityGraph:
    """idx (n, k) int32 neighbours (-1 = empty slot), w (n, k) int32 edge
    weights >= 1 (0 in empty slots), in_off (n+1) / in_edge (E) int32 the
    reverse lists of the filled slots (projection.layout_reverse_lists)."""
    idx: torch.Tensor
    w: torch.Tensor
    in_off: torch.Tensor
    in_edge: torch.Tensor
    n: int

    @classmethod
    def from_knn(cls, pos: torch.Tensor, dists: torch.Tensor,
                 bandwidth: float, levels: int) -> "CommunityGraph":
        """pos (n, k) positions (< 0 = no neighbour), dists (n, k)
        distances, as SimilarityEngine.neighbor_graph returns them. A
        filled slot weighs max(1, round(levels * exp(-clamp(d, min=0) /
        sigma))) with sigma = bandwidth * the median of the filled
        distances (torch.median, as RankGraph takes it); with sigma == 0
        every filled slot weighs levels."""
        if pos.dim() != 2 or dists.shape != pos.shape or pos.shape[1] < 1:
            raise ValueError("pos and dists must both be (n, k), k >= 1")
        if not bandwidth > 0:
            raise ValueError("bandwidth must be positive")
        levels = int(levels)
        if not 1 <= levels < (1 << 24):
            raise ValueError("levels must be in [1, 2^24)")
        n = pos.shape[0]
        if bool((pos >= n).any()):
            raise ValueError("neighbour positions must be below n")
        d = dists.float().clamp(min=0)
        filled = (pos >= 0) & torch.isfinite(d)
        idx = torch.where(filled, pos, torch.full_like(pos, -1)).to(torch.int32)
        sigma = 0.0
        if bool(filled.any()):
            sigma = float(bandwidth) * float(d[filled].median())
        if sigma > 0:
            w = torch.round(levels * torch.exp(-d.double() / sigma)
                            ).clamp(min=1).to(torch.int32)
        else:
            w = torch.full(d.shape, levels, dtype=torch.int32, device=d.device)
        w = torch.where(filled, w, torch.zeros_like(w))
        in_off, in_edge = layout_reverse_lists(idx, filled.to(torch.int32))
        return cls(idx.contiguous(), w.contiguous(), in_off.contiguous(),
                   in_edge.contiguous(), n)

    @property
    def device(self) -> torch.device:
        return self.idx.device

    def to(self, device) -> "CommunityGraph":
        return CommunityGraph(self.idx.to(device), self.w.to(device),
                              self.in_off.to(device), self.in_edge.to(device),
                              self.n)


def resolution_units(resolution: float) -> int:
    """g of gamma = g / 64: max(1, round(64 * resolution))."""
    if not resolution > 0:
        raise ValueError("resolution must be positive")
    return max(1, int(round(RESOLUTION_UNIT * float(resolution))))


def _own_entries(idx: torch.Tensor, w: torch.Tensor
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(valid (n, k), u (n, k) int64 clamped into [0, n), w (n, k) int64
    with 0 where not valid) of the own slots; a slot that is empty or
    holds its own vertex is no candidate."""
    n = idx.shape[0]
    ar = torch.arange(n, device=idx.device).unsqueeze(1)
    u = idx.long().clamp(max=max(n - 1, 0))
    valid = (idx >= 0) & (u != ar)
    u = u.clamp(min=0)
    w64 = w.long()
    return valid, u, torch.where(valid, w64, torch.zeros_like(w64))


def _in_entries(idx: torch.Tensor, w: torch.Tensor, in_off: torch.Tensor,
                in_edge: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(tail (E), head (E), w (E) int64 with 0 where head == tail) of the
    in-list entries: tail is the vertex that owns the list."""
    n, k = idx.shape
    E = in_edge.numel()
    e = in_edge.long().clamp(0, max(n * k - 1, 0))
    head = e // k
    tail = torch.repeat_interleave(
        torch.arange(n, device=idx.device),
        (in_off[1:] - in_off[:-1]).long(), output_size=E)
    we = w.long().reshape(-1)[e]
    return tail, head, torch.where(head != tail, we, torch.zeros_like(we))


def degrees(graph: CommunityGraph) -> torch.Tensor:
    """deg (n,) int64: the sum of w over a vertex's candidates, own slots
    and then its in-list, without the candidates that are the vertex."""
    _, _, ow = _own_entries(graph.idx, graph.w)
    deg = ow.sum(dim=1)
    if graph.in_edge.numel():
        tail, _, we = _in_entries(graph.idx, graph.w, graph.in_off,
                                  graph.in_edge)
        deg.index_add_(0, tail, we)
    return deg


def move_reference(label_in: torch.Tensor, label_out: torch.Tensor,
                   tot: torch.Tensor, deg: torch.Tensor, idx: torch.Tensor,
                   w: torch.Tensor, in_off: torch.Tensor,
                   in_edge: torch.Tensor, A: int, g: int, up: bool) -> None:
    """One local-moving sweep in torch, with the signature of
    _C.community_move and equal results: the golden reference of the
    kernel and the path where the kernel cannot run. For vertex v with
    L = label_in[v]: the candidate communities are the labels of v's own-
    slot neighbours; K[c] is the sum of w over all of v's candidates (own
    slots and in-list, u != v) whose label is c; stay = K[L] * A - g *
    deg[v] * (tot[L] - deg[v]); score[c] = K[c] * A - g * deg[v] * tot[c];
    c is eligible when c != L, score[c] > stay and c > L (up) or c < L
    (down); label_out[v] is the eligible c of highest score, ties to the
    smallest c, else L. All in int64. Any device; nothing synchronises."""
    n, k = idx.shape
    if n == 0:
        return
    A, g = int(A), int(g)
    L = label_in.long().clamp(0, n - 1)
    valid, u, ow = _own_entries(idx, w)
    c = torch.where(valid, L[u], torch.full_like(u, -1))        # (n, k)
    ct = c.t().contiguous()                                     # (k, n)
    owt = ow.t().contiguous()
    K = torch.zeros_like(owt)
    for i in range(k):      # slots that are not valid add 0
        K += torch.where(ct[i].unsqueeze(0) == ct, owt[i].unsqueeze(0),
                         torch.zeros_like(owt))
    KL = (owt * (ct == L.unsqueeze(0))).sum(dim=0)
    if in_edge.numel():
        tail, head, we = _in_entries(idx, w, in_off, in_edge)
        lh = L[head]
        KL.index_add_(0, tail, we * (lh == L[tail]))
        for j in range(k):
            K[j].index_add_(0, tail, we * (lh == ct[j][tail]))
    gd = g * deg
    stay = KL * A - gd * (tot[L] - deg)
    score = K * A - gd.unsqueeze(0) * tot[ct.clamp(min=0)]
    side = (ct > L.unsqueeze(0)) if up else (ct < L.unsqueeze(0))
    ok = (ct >= 0) & (ct != L.unsqueeze(0)) & side & (score > stay.unsqueeze(0))
    ms = torch.where(ok, score, torch.full_like(score, _I64_MIN))
    best = ms.max(dim=0).values
    pick = ok & (ms == best.unsqueeze(0))
    cm = torch.where(pick, ct, torch.full_like(ct, n)).min(dim=0).values
    label_out.copy_(torch.where(cm < n, cm, L))


def _kernel(graph: CommunityGraph):
    """The fused op when the graph is on the GPU, the extension loads and
    k fits its registers; the torch statement otherwise."""
    from audiomuse_amd.ops import _ext

    if graph.device.type != "cuda" or graph.idx.shape[1] > MAX_KERNEL_K:
        return move_reference
    ext = _ext.native_or_none()
    if ext is None:
        return move_reference
    return ext.community_move


def _level_shift(weigh: Callable[[int], Tuple[int, int]], g: int) -> int:
    """weigh(s) -> (max_deg, two_m) of the level with its weights shifted
    right by s, as Python ints. The smallest s <= 31 for which max(64, g)
    * max_deg * two_m < 2^62; ValueError when there is none."""
    for s in range(MAX_SHIFT + 1):
        max_deg, two_m = weigh(s)
        if max(RESOLUTION_UNIT, g) * max_deg * two_m < (1 << 62):
            return s
    raise ValueError("graph weights overflow int64 at every shift up to 31: "
                     "lower the resolution or the weight levels")


def _run_groups(step: Callable[[torch.Tensor, bool], torch.Tensor],
                label: torch.Tensor, max_sweeps: int
                ) -> Tuple[torch.Tensor, int, bool]:
    """Sweeps in groups of two, down then up. After each group its end
    labels are compared with the previous group's end labels (the loop's
    only host read); equal ends it: nothing moved, or the sweep has
    entered a period-two cycle. (labels, sweeps, capped)."""
    sweeps = 0
    prev = label
    while sweeps + 2 <= max_sweeps:
        label = step(step(prev, False), True)
        sweeps += 2
        if torch.equal(label, prev):
            return label, sweeps, False
        prev = label
    return label, sweeps, True


def _shifted(w: torch.Tensor, s: int) -> torch.Tensor:
    """max(1, w >> s) on the edges, 0 stays 0 (empty slots)."""
    if s == 0:
        return w
    return torch.where(w > 0, (w >> s).clamp(min=1), torch.zeros_like(w))


def _table_level(graph: CommunityGraph, g: int, max_sweeps: int
                 ) -> Tuple[torch.Tensor, int, bool, int, CommunityGraph]:
    """(labels (n,) int32 vertex ids, sweeps, capped, shift, the graph
    with the shifted weights) of the local moving on the table."""
    n = graph.n
    dev = graph.device
    label = torch.arange(n, dtype=torch.int32, device=dev)
    if n == 0:
        return label, 0, False, 0, graph
    state = {}

    def weigh(s: int) -> Tuple[int, int]:
        gs = CommunityGraph(graph.idx, _shifted(graph.w, s), graph.in_off,
                            graph.in_edge, n)
        deg = degrees(gs)
        state["graph"], state["deg"] = gs, deg
        state["two_m"] = int(deg.sum())
        return int(deg.max()), state["two_m"]

    shift = _level_shift(weigh, g)
    gs, deg, two_m = state["graph"], state["deg"], state["two_m"]
    if two_m == 0:
        return label, 0, False, shift, gs
    A = RESOLUTION_UNIT * two_m
    move = _kernel(gs)
    tot = deg.clone()
    # the previous group's end labels stay alive while two more sweeps
    # run, so three buffers rotate: a sweep writes the one after its input
    bufs = [label, torch.empty_like(label), torch.empty_like(label)]

    def step(lab: torch.Tensor, up: bool) -> torch.Tensor:
        at = next(i for i, b in enumerate(bufs) if b is lab)
        out = bufs[(at + 1) % 3]
        move(lab, out, tot, deg, gs.idx, gs.w, gs.in_off, gs.in_edge, A, g,
             up)
        tot.zero_().index_add_(0, out.long(), deg)
        return out

    label, sweeps, capped = _run_groups(step, label, max_sweeps)
    return label, sweeps, capped, shift, gs


def local_move(graph: CommunityGraph, resolution: float, max_sweeps: int
               ) -> Tuple[torch.Tensor, int, bool]:
    """Local moving on the table from singletons: (labels (n,) int32
    community ids that are vertex ids, sweeps run, capped). It stops when
    two groups of (down, up) sweeps end on equal labels, or at max_sweeps
    (capped)."""
    label, sweeps, capped, _, _ = _table_level(
        graph, resolution_units(resolution), int(max_sweeps))
    return label, sweeps, capped


# -- coarse levels: the same rule on a COO list ------------------------------


def _coo_move(label: torch.Tensor, tot: torch.Tensor, deg: torch.Tensor,
              src: torch.Tensor, dst: torch.Tensor, wt: torch.Tensor,
              A: int, g: int, up: bool) -> torch.Tensor:
    """One sweep over directed entries (src, dst, wt), src != dst, every
    edge listed from both ends: the rule of move_reference with every
    neighbour community a candidate. All int64."""
    m = label.numel()
    key = src * m + label[dst]
    pairs, inv = torch.unique(key, return_inverse=True)
    Kp = torch.zeros(pairs.numel(), dtype=torch.int64,
                     device=label.device).index_add_(0, inv, wt)
    pv = torch.div(pairs, m, rounding_mode="floor")
    pc = pairs - pv * m
    Lp = label[pv]
    here = pc == Lp
    KL = torch.zeros_like(deg).index_add_(0, pv, Kp * here)
    gd = g * deg
    stay = KL * A - gd * (tot[label] - deg)
    score = Kp * A - gd[pv] * tot[pc]
    ok = ~here & (score > stay[pv]) & ((pc > Lp) if up else (pc < Lp))
    ms = torch.where(ok, score, torch.full_like(score, _I64_MIN))
    best = torch.full_like(deg, _I64_MIN).scatter_reduce_(
        0, pv, ms, "amax", include_self=True)
    pick = ok & (ms == best[pv])
    cm = torch.full_like(deg, m).scatter_reduce_(
        0, pv, torch.where(pick, pc, torch.full_like(pc, m)), "amin",
        include_self=True)
    return torch.where(cm < m, cm, label)


def _coo_level(src: torch.Tensor, dst: torch.Tensor, wt: torch.Tensor,
               selfw: torch.Tensor, g: int, max_sweeps: int):
    """(labels (m,) int64 vertex ids, sweeps, capped, shift, wt', selfw')
    of the local moving on a coarse level; selfw counts in deg and is
    never a candidate."""
    m = selfw.numel()
    dev = selfw.device
    label = torch.arange(m, device=dev)
    state = {}

    def weigh(s: int) -> Tuple[int, int]:
        ws = wt if s == 0 else (wt >> s).clamp(min=1)
        ss = selfw >> s
        deg = ss.clone().index_add_(0, src, ws)
        state["w"], state["self"], state["deg"] = ws, ss, deg
        state["two_m"] = int(deg.sum())
        return int(deg.max()), state["two_m"]

    shift = _level_shift(weigh, g)
    ws, ss, deg = state["w"], state["self"], state["deg"]
    two_m = state["two_m"]
    if two_m == 0 or src.numel() == 0:
        return label, 0, False, shift, ws, ss
    A = RESOLUTION_UNIT * two_m
    tot = deg.clone()

    def step(lab: torch.Tensor, up: bool) -> torch.Tensor:
        out = _coo_move(lab, tot, deg, src, dst, ws, A, g, up)
        tot.zero_().index_add_(0, out, deg)
        return out

    label, sweeps, capped = _run_groups(step, label, max_sweeps)
    return label, sweeps, capped, shift, ws, ss


def _sum_pairs(a: torch.Tensor, b: torch.Tensor, wt: torch.Tensor, m: int
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                          torch.Tensor]:
    """Entries (a, b, wt) between communities: (src, dst, wt) with one
    entry per ordered pair a != b, sorted, and selfw (m,) the sum of the
    entries with a == b."""
    inner = a == b
    selfw = torch.zeros(m, dtype=torch.int64, device=a.device).index_add_(
        0, a[inner], wt[inner])
    key = (a * m + b)[~inner]
    pairs, inv = torch.unique(key, return_inverse=True)
    pw = torch.zeros(pairs.numel(), dtype=torch.int64,
                     device=a.device).index_add_(0, inv, wt[~inner])
    src = torch.div(pairs, m, rounding_mode="floor")
    return src, pairs - src * m, pw, selfw


def _compact(label: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """Community ids renumbered 0..m-1 in ascending order of id."""
    uniq, inv = torch.unique(label.long(), return_inverse=True)
    return inv, int(uniq.numel())


def _renumber(member: torch.Tensor, m: int) -> torch.Tensor:
    """Labels 0..m-1 by descending size, ties by the smallest member."""
    n = member.numel()
    size = torch.bincount(member, minlength=m)
    first = torch.full((m,), n, dtype=torch.int64,
                       device=member.device).scatter_reduce_(
        0, member, torch.arange(n, device=member.device), "amin",
        include_self=True)
    by_first = torch.argsort(first, stable=True)
    order = by_first[torch.argsort(size[by_first], descending=True,
                                   stable=True)]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(m, device=member.device)
    return rank[member].to(torch.int32)


def modularity(graph: CommunityGraph, labels: torch.Tensor,
               resolution: float) -> float:
    """Q = in / two_m - gamma * sum((tot_c / two_m) ** 2) in f64 from the
    integer sums: in is the weight of the candidates whose two ends share
    a label, tot_c the degree sum of community c, gamma = g / 64."""
    n = graph.n
    if n == 0:
        return 0.0
    lab = labels.long().to(graph.device)
    deg = degrees(graph)
    two_m = int(deg.sum())
    if two_m == 0:
        return 0.0
    valid, u, ow = _own_entries(graph.idx, graph.w)
    # an own slot (v, u) is a candidate of v and, through the in-list, of u
    inner = 2 * int((ow * (lab[u] == lab.unsqueeze(1))).sum())
    tot = torch.zeros(int(lab.max()) + 1, dtype=torch.int64,
                      device=graph.device).index_add_(0, lab, deg)
    gamma = resolution_units(resolution) / RESOLUTION_UNIT
    frac = tot.double() / two_m
    return inner / two_m - gamma * float((frac * frac).sum())


def communities(graph: CommunityGraph, resolution: float = 1.0,
                max_sweeps: int = 100, max_levels: int = 10
                ) -> Tuple[torch.Tensor, Dict]:
    """Multi-level Louvain: (labels (n,) int32 on the graph's device,
    numbered 0..C-1 by descending size with ties to the smallest member,
    report). Level 0 is local_move on the table (the kernel, on the GPU);
    then communities become vertices, the weights between them are summed
    and the weight inside one becomes its self-weight, and the coarse
    levels run the same rule with every neighbour community a candidate.
    It stops when a level merges nothing, or at max_levels. Vertices with
    no candidate stay singletons. report: levels (per level vertices,
    communities, sweeps, capped, shift), communities, modularity,
    seconds."""
    t0 = time.perf_counter()
    g = resolution_units(resolution)
    max_sweeps, max_levels = int(max_sweeps), int(max_levels)
    if max_levels < 1:
        raise ValueError("max_levels must be at least 1")
    n = graph.n
    levels: List[Dict] = []
    label, sweeps, capped, shift, gs = _table_level(graph, g, max_sweeps)
    member, m = _compact(label)
    levels.append({"vertices": n, "communities": m, "sweeps": sweeps,
                   "capped": capped, "shift": shift})
    if 0 < m < n and len(levels) < max_levels:
        valid, u, ow = _own_entries(gs.idx, gs.w)
        a = member.unsqueeze(1).expand_as(u)[valid]
        b = member[u[valid]]
        wv = ow[valid]
        # every own slot is a candidate from both of its ends
        src, dst, pw, selfw = _sum_pairs(torch.cat([a, b]), torch.cat([b, a]),
                                         torch.cat([wv, wv]), m)
        while len(levels) < max_levels:
            lab, sweeps, capped, shift, pw, selfw = _coo_level(
                src, dst, pw, selfw, g, max_sweeps)
            sub, m2 = _compact(lab)
            levels.append({"vertices": m, "communities": m2,
                           "sweeps": sweeps, "capped": capped,
                           "shift": shift})
            if m2 == m:
                break
            member = sub[member]
            src, dst, pw, inner = _sum_pairs(sub[src], sub[dst], pw, m2)
            selfw = inner.index_add_(0, sub, selfw)
            m = m2
    labels = _renumber(member, m) if n else member.to(torch.int32)
    report = {"levels": levels, "communities": m,
              "modularity": modularity(graph, labels, resolution),
              "seconds": time.perf_counter() - t0}
    return labels, report
