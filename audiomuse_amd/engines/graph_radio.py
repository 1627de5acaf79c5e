"""Graph radio: personalised PageRank over the kNN graph.

"More like what I listen to" from a set of weighted seeds, without
collapsing the listener to one point: a random walk that restarts at the
seeds spreads their mass over the whole-catalogue neighbour graph
(SimilarityEngine.neighbor_graph), so two tastes stay two tastes where
their mean vector lies in neither. The graph is the symmetrised multigraph
the graph song path walks, with affinities exp(-d / sigma) on the edges.
It is solved by a fixed number of power-iteration sweeps for up to 8 legs
(independent seed sets) at once: a pull pass in which every vertex is
computed and written by one owner, one HIP launch per sweep
(ops/csrc/rank.hip). pull_reference below is the torch statement of the
sweep (f64 accumulation) and the engine's path where the kernel cannot
run (docs/ALGORITHM.md "Graph radio").
"""

from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from audiomuse_amd.engines.projection import layout_reverse_lists

log = logging.getLogger(__name__)

MAX_LEGS = 8
RADIO_ENGINES = ("centroid", "graph")
# candidates fetched per requested track before the per-artist cap, as
# SimilarityEngine.find_similar_by_vector over-fetches
OVERFETCH = 4

_fallback_logged = False


@dataclass
class RankGraph:
    """idx (n, k) int32 neighbours (-1 = empty slot), s (n, k) f32 edge
    affinities in (0, 1] (0 in empty slots), in_off (n+1) / in_edge (E)
    int32 the reverse lists of the filled slots
    (projection.layout_reverse_lists)."""
    idx: torch.Tensor
    s: torch.Tensor
    in_off: torch.Tensor
    in_edge: torch.Tensor
    n: int

    @classmethod
    def from_knn(cls, pos: torch.Tensor, dists: torch.Tensor,
                 bandwidth: float) -> "RankGraph":
        """pos (n, k) positions (< 0 = no neighbour), dists (n, k)
        distances, as SimilarityEngine.neighbor_graph returns them. The
        affinity of an edge is exp(-clamp(d, min=0) / sigma) with sigma =
        bandwidth * the median of the filled distances (the lower of the
        two middle values, torch.median); with sigma == 0 every filled
        slot has affinity 1."""
        if pos.dim() != 2 or dists.shape != pos.shape or pos.shape[1] < 1:
            raise ValueError("pos and dists must both be (n, k), k >= 1")
        if not bandwidth > 0:
            raise ValueError("bandwidth must be positive")
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
            s = torch.exp(-d / sigma)
        else:
            s = torch.ones_like(d)
        s = torch.where(filled, s, torch.zeros_like(s))
        in_off, in_edge = layout_reverse_lists(idx, filled.to(torch.int32))
        return cls(idx.contiguous(), s.contiguous(), in_off.contiguous(),
                   in_edge.contiguous(), n)

    @property
    def device(self) -> torch.device:
        return self.idx.device

    def to(self, device) -> "RankGraph":
        return RankGraph(self.idx.to(device), self.s.to(device),
                         self.in_off.to(device), self.in_edge.to(device),
                         self.n)


def pull_reference(x_in: torch.Tensor, p_out: torch.Tensor,
                   q_out: Optional[torch.Tensor],
                   restart: Optional[torch.Tensor],
                   inv_deg: Optional[torch.Tensor], idx: torch.Tensor,
                   s: torch.Tensor, in_off: torch.Tensor,
                   in_edge: torch.Tensor, allowed: Optional[torch.Tensor],
                   alpha: float) -> None:
    """One sweep in torch, with the signature of _C.rank_pull: the golden
    reference of the kernel and the engine's path where the kernel cannot
    run. acc[b][v] is the sum of s * x_in[b][u] over v's candidates (own
    slots, then its in-list); with restart, inv_deg and q_out, p_out =
    (1 - alpha) * restart + alpha * acc and q_out = p_out * inv_deg;
    without the three, p_out = acc. Vertices that are not allowed get 0.
    Sums run in f64 and are rounded to f32 once, on output; alpha is taken
    in f32, as the kernel takes it. Any device, any strides; nothing
    synchronises."""
    sweep = restart is not None
    if (q_out is not None) != sweep or (inv_deg is not None) != sweep:
        raise ValueError("q_out, restart and inv_deg go together")
    B, n = x_in.shape
    k = idx.shape[1]
    dev = x_in.device
    x = x_in.double()
    sd = s.double()
    acc = torch.zeros(B, n, dtype=torch.float64, device=dev)
    for j in range(k):
        u = idx[:, j].long()
        term = sd[:, j].unsqueeze(0) * x[:, u.clamp(0, n - 1)]
        acc += torch.where((u >= 0).unsqueeze(0), term, torch.zeros_like(term))
    E = in_edge.numel()
    if E:
        e = in_edge.long().clamp(0, n * k - 1)
        head = e // k
        tail = torch.repeat_interleave(
            torch.arange(n, device=dev), (in_off[1:] - in_off[:-1]).long(),
            output_size=E)
        acc.index_add_(1, tail, sd.reshape(-1)[e].unsqueeze(0) * x[:, head])
    if sweep:
        a = float(torch.tensor(float(alpha), dtype=torch.float32))
        acc = (1.0 - a) * restart.double() + a * acc
    if allowed is not None:
        acc = torch.where((allowed != 0).unsqueeze(0), acc,
                          torch.zeros_like(acc))
    p_out.copy_(acc)
    if sweep:
        q_out.copy_(acc * inv_deg.double().unsqueeze(0))


def _kernels(dev: torch.device):
    """The fused op when the graph is on the GPU and the extension loads,
    the torch statement otherwise."""
    from audiomuse_amd.ops import _ext

    ext = _ext.native_or_none() if dev.type == "cuda" else None
    if ext is None:
        return pull_reference
    return ext.rank_pull


def sweep_count(alpha: float, tolerance: float, max_sweeps: int) -> int:
    """T = min(max_sweeps, ceil(log(tolerance) / log(alpha))): with p* the
    fixed point, p_T - p* = alpha^T (P^T r - p*), at most 2 alpha^T in L1,
    so T is known before the first sweep and the loop reads nothing back."""
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must be in [0, 1)")
    if not 0.0 < tolerance < 1.0:
        raise ValueError("tolerance must be in (0, 1)")
    if alpha == 0.0:
        return 0
    return max(0, min(int(max_sweeps),
                      math.ceil(math.log(tolerance) / math.log(alpha))))


def _mask(graph: RankGraph, allowed: Optional[torch.Tensor]
          ) -> Optional[torch.Tensor]:
    if allowed is None:
        return None
    if allowed.shape != (graph.n,):
        raise ValueError("allowed must be (n,)")
    return (allowed != 0).to(device=graph.device,
                             dtype=torch.uint8).contiguous()


def degrees(graph: RankGraph, allowed: Optional[torch.Tensor] = None
            ) -> torch.Tensor:
    """deg (n,) f32: the sum of s over a vertex's candidates, own slots in
    slot order and then its in-list. Under a mask only candidates whose
    other end is allowed count, and closed vertices have degree 0. It is
    the sweep's own gather over x = ones (or the mask), so one call of
    the same op."""
    dev = graph.device
    allowed = _mask(graph, allowed)
    x = (torch.ones(1, graph.n, device=dev) if allowed is None
         else allowed.float().unsqueeze(0))
    deg = torch.empty(1, graph.n, device=dev)
    _kernels(dev)(x, deg, None, None, None, graph.idx, graph.s, graph.in_off,
                  graph.in_edge, allowed, 0.0)
    return deg[0]


def _solve(graph: RankGraph, restart: torch.Tensor, alpha: float,
           sweeps: int, allowed: Optional[torch.Tensor]
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(p (B, n), deg (n,)) of personalized_pagerank."""
    n = graph.n
    if restart.dim() != 2 or restart.shape[1] != n:
        raise ValueError("restart must be (B, n)")
    B = restart.shape[0]
    if not 1 <= B <= MAX_LEGS:
        raise ValueError(f"PageRank is solved for 1 to {MAX_LEGS} legs")
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must be in [0, 1)")
    if sweeps < 0:
        raise ValueError("sweeps must be >= 0")
    dev = graph.device
    pull = _kernels(dev)
    allowed = _mask(graph, allowed)
    deg = degrees(graph, allowed)
    inv_deg = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    # (B, n) views of vertex-major memory: the B values of a vertex lie
    # side by side, so the kernel reads a candidate's legs in one piece
    r = torch.empty(n, B, device=dev).t()
    r.copy_(restart)
    if allowed is not None:     # a closed seed starts nothing
        r.masked_fill_((allowed == 0).unsqueeze(0), 0.0)
    p = torch.empty(n, B, device=dev).t()
    p.copy_(r)
    q = torch.empty(n, B, device=dev).t()
    torch.mul(r, inv_deg.unsqueeze(0), out=q)
    q_nxt = torch.empty(n, B, device=dev).t()
    for _ in range(sweeps):
        pull(q, p, q_nxt, r, inv_deg, graph.idx, graph.s, graph.in_off,
             graph.in_edge, allowed, alpha)
        q, q_nxt = q_nxt, q
    return p, deg


def personalized_pagerank(graph: RankGraph, restart: torch.Tensor,
                          alpha: float, sweeps: int,
                          allowed: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """p_T (B, n) f32 on the graph's device (a transposed view of (n, B)
    memory) for 1..8 restart distributions: p_0 = r, p_{t+1} = (1 - alpha)
    r + alpha P^T p_t, where a step of P leaves u along a candidate edge
    with probability s / deg(u). allowed: optional (n) uint8/bool mask;
    the walk stays on allowed vertices, closed vertices score 0 and
    restart mass on them is dropped. The number of sweeps is fixed
    (sweep_count), so nothing in the loop synchronises. The fused kernel
    runs when the graph is on the GPU and the extension loads, the torch
    reference otherwise."""
    return _solve(graph, restart, alpha, sweeps, allowed)[0]


# -- the engine ---------------------------------------------------------------


def _leg(sim, ids: Sequence[str], weights: Optional[Sequence[float]],
         mask: Optional[torch.Tensor]) -> Dict[int, float]:
    """{position: weight} of the ids that are known and in scope; repeated
    ids add up; weights that do not sum to a positive number count as
    equal weights."""
    if weights is not None and len(weights) != len(ids):
        raise ValueError("one weight per seed")
    w = [1.0] * len(ids) if weights is None else \
        [max(float(x), 0.0) for x in weights]
    out: Dict[int, float] = {}
    for iid, wi in zip(ids, w):
        p = sim.pos.get(iid)
        if p is None or (mask is not None and not bool(mask[p])):
            continue
        out[p] = out.get(p, 0.0) + wi
    if out and not sum(out.values()) > 0:
        out = {p: 1.0 for p in out}
    return out


def _centroid(sim, seed_ids: Sequence[str],
              weights: Optional[Sequence[float]],
              subtract_ids: Sequence[str], n: int, scope: Optional[str],
              max_per_artist: Optional[int]) -> List[Dict]:
    """The centroid engine: the weighted mean of the seed vectors,
    normalised, and one query around it (what engines/misc.
    sonic_fingerprint computes from play times)."""
    vecs, w = [], []
    for i, iid in enumerate(seed_ids):
        v = sim.vector_for_id(iid)
        if v is None:
            continue
        vecs.append(v.float().cpu().numpy())
        w.append(1.0 if weights is None else max(float(weights[i]), 0.0))
    if not vecs:
        return []
    wa = np.asarray(w, dtype=np.float32)
    if not wa.sum() > 0:
        wa = np.ones(len(vecs), dtype=np.float32)
    mean = (np.stack(vecs) * wa[:, None]).sum(axis=0) / wa.sum()
    norm = float(np.linalg.norm(mean))
    if not norm > 0:
        return []
    return sim.find_similar_by_vector(
        torch.from_numpy((mean / norm).astype(np.float32)), n,
        exclude=tuple(seed_ids) + tuple(subtract_ids), scope=scope,
        max_per_artist=max_per_artist)


def _graph_radio(sim, seed_ids, weights, subtract_ids, n, scope,
                 max_per_artist) -> Optional[List[Dict]]:
    """The graph engine; None when there is no graph (dot metric), no seed
    is known and in scope, or fewer than n tracks end with a positive
    score, and the request falls back to the centroid engine."""
    from audiomuse_amd import config as C
    graph = sim.rank_graph()
    if graph is None:
        return None
    mask = sim.scope_mask(scope) if scope is not None else None
    add = _leg(sim, seed_ids, weights, mask)
    if not add:
        return None
    sub = _leg(sim, subtract_ids, None, mask)
    legs = [add, sub] if sub else [add]
    dev = graph.device
    restart = torch.zeros(len(legs), graph.n, device=dev)
    for b, leg in enumerate(legs):
        w = torch.tensor(list(leg.values()), dtype=torch.float64)
        restart[b, torch.tensor(list(leg), device=dev)] = \
            (w / w.sum()).float().to(dev)
    alpha = float(C.RADIO_ALPHA)
    T = sweep_count(alpha, C.RADIO_TOLERANCE, C.RADIO_MAX_SWEEPS)
    p, deg = _solve(graph, restart, alpha, T, mask)
    score = p[0].clone()
    if sub:
        score -= float(C.RADIO_SUBTRACT_WEIGHT) * p[1]
    if C.RADIO_HUB_EXPONENT:
        score = torch.where(deg > 0,
                            score / deg.clamp(min=1e-30)
                            ** float(C.RADIO_HUB_EXPONENT), score)
    shut = torch.tensor(sorted(set(add) | set(sub)), device=dev)
    score[shut] = -math.inf
    if mask is not None:
        score.masked_fill_(mask.to(dev) == 0, -math.inf)
    fetch = min(max(n * OVERFETCH, n), graph.n)
    top = torch.topk(score, fetch)
    vals, at = top.values.cpu().tolist(), top.indices.cpu().tolist()
    cands = [(i, v) for i, v in zip(at, vals) if v > 0]
    if len(cands) < n:
        return None
    items: List[Dict] = []
    artist_counts: Dict[str, int] = {}
    for i, v in cands:
        iid = sim.item_ids[i]
        author = ((sim.meta_fn(iid) or {}).get("author") or ""
                  ).strip().lower()
        if max_per_artist and author:
            if artist_counts.get(author, 0) >= max_per_artist:
                continue
            artist_counts[author] = artist_counts.get(author, 0) + 1
        items.append({"item_id": iid, "score": v})
        if len(items) >= n:
            break
    return items


def graph_radio(sim, seed_ids: Sequence[str],
                weights: Optional[Sequence[float]] = None, *,
                subtract_ids: Sequence[str] = (), n: int,
                scope: Optional[str] = None,
                max_per_artist: Optional[int] = None,
                engine: Optional[str] = None) -> Tuple[List[Dict], str]:
    """The n tracks a listener of the weighted seeds would hear next, and
    the engine that produced the answer: (items, "graph" | "centroid").

    engine "graph" (None takes config.SONIC_FINGERPRINT_ENGINE): leg 0 is
    a personalised PageRank from the seeds, leg 1 (solved in the same
    batch) one from subtract_ids; score = p_add - RADIO_SUBTRACT_WEIGHT *
    p_sub, divided by degree ** RADIO_HUB_EXPONENT. Seeds, subtracted
    tracks and tracks outside the scope are never returned; max_per_artist
    caps the tracks of one artist. Items carry item_id and score, best
    first. It falls back to the centroid engine when the index metric is
    dot, no seed is known and in scope, or fewer than n tracks have a
    positive score.

    engine "centroid": the weighted mean of the seed vectors and one
    query around it (SimilarityEngine.find_similar_by_vector); items carry
    item_id and distance, and subtract_ids are only excluded."""
    global _fallback_logged
    from audiomuse_amd import config as C
    if engine is None:
        engine = C.SONIC_FINGERPRINT_ENGINE
    if engine not in RADIO_ENGINES:
        raise ValueError(f"radio engine must be centroid or graph, "
                         f"not {engine!r}")
    if n < 1:
        raise ValueError("n must be at least 1")
    seed_ids = list(seed_ids)
    subtract_ids = list(subtract_ids)
    if weights is not None and len(weights) != len(seed_ids):
        raise ValueError("one weight per seed")
    if engine == "graph":
        items = _graph_radio(sim, seed_ids, weights, subtract_ids, n, scope,
                             max_per_artist)
        if items is not None:
            return items, "graph"
        if not _fallback_logged:
            _fallback_logged = True
            log.warning("graph radio: no graph (dot metric), no known seed "
                        "in scope, or too few tracks reached; falling back "
                        "to the centroid engine")
    return _centroid(sim, seed_ids, weights, subtract_ids, n, scope,
                     max_per_artist), "centroid"
