"""Graph song path: batched shortest paths over the kNN graph.

A journey in which every step is a true nearest-neighbour hop is a
shortest path over the whole-catalogue neighbour graph
(SimilarityEngine.neighbor_graph). The graph is symmetrised (an edge can
be walked in both directions) and solved by Jacobi sweeps of
Bellman-Ford for up to 8 legs at once: a pull pass in which every vertex
is computed and written by one owner, so the f32 distances and the
predecessor forest are deterministic. The sweep is one HIP launch
(ops/csrc/path.hip); relax_reference and walk_reference below are its
torch statement, bit-identical to the kernel, and the engine's path where
the kernel cannot run (docs/ALGORITHM.md "Graph song path").
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from audiomuse_amd.engines.projection import layout_reverse_lists

MAX_LEGS = 8
# Sweeps between two reads of the changed flags. With T sweeps to the
# fixed point, a group of g costs about (1.5 g - 0.5) sweeps past T (half a
# group of overshoot and one whole group that only confirms) plus T / g
# host reads of about 20 us each. A sweep is 0.9-1.1 ms at 1M tracks and
# 0.06-0.10 ms at 100k; T is 3-5 on clustered catalogues and 55-120 on a
# connected manifold (profiles/r8_graph_path.txt). Measured over 1, 2, 4, 8
# and 16, a group of 2 is within 3 % of the best group on the long solves
# and costs at most 1.5x the per-sweep read on the short ones, where 8
# costs 2.5-3.9x.
SWEEP_GROUP = 2

_INF = float("inf")


@dataclass
class PathGraph:
    """idx (n, k) int32 neighbours (-1 = empty slot), w (n, k) f32 edge
    weights >= 0 (0 in empty slots), in_off (n+1) / in_edge (E) int32 the
    reverse lists of the filled slots (projection.layout_reverse_lists)."""
    idx: torch.Tensor
    w: torch.Tensor
    in_off: torch.Tensor
    in_edge: torch.Tensor
    n: int

    @classmethod
    def from_knn(cls, pos: torch.Tensor, dists: torch.Tensor,
                 exponent: float) -> "PathGraph":
        """pos (n, k) positions (< 0 = no neighbour), dists (n, k)
        distances, as SimilarityEngine.neighbor_graph returns them. The
        weight of an edge is clamp(d, min=0) ** exponent."""
        if pos.dim() != 2 or dists.shape != pos.shape or pos.shape[1] < 1:
            raise ValueError("pos and dists must both be (n, k), k >= 1")
        n = pos.shape[0]
        if bool((pos >= n).any()):
            raise ValueError("neighbour positions must be below n")
        d = dists.float()
        filled = (pos >= 0) & torch.isfinite(d)
        idx = torch.where(filled, pos, torch.full_like(pos, -1)).to(torch.int32)
        w = torch.where(filled, d.clamp(min=0) ** float(exponent),
                        torch.zeros_like(d))
        if not bool(torch.isfinite(w).all()):
            raise ValueError("edge weights must be finite")
        in_off, in_edge = layout_reverse_lists(idx, filled.to(torch.int32))
        return cls(idx.contiguous(), w.contiguous(), in_off.contiguous(),
                   in_edge.contiguous(), n)

    @property
    def device(self) -> torch.device:
        return self.idx.device

    def to(self, device) -> "PathGraph":
        return PathGraph(self.idx.to(device), self.w.to(device),
                         self.in_off.to(device), self.in_edge.to(device),
                         self.n)


def relax_reference(dist_in: torch.Tensor, pred_in: torch.Tensor,
                    dist_out: torch.Tensor, pred_out: torch.Tensor,
                    idx: torch.Tensor, w: torch.Tensor, in_off: torch.Tensor,
                    in_edge: torch.Tensor, allowed: Optional[torch.Tensor],
                    changed: torch.Tensor) -> None:
    """One sweep in torch, with the signature and the exact results of
    _C.path_relax: the golden reference of the kernel and the engine's
    path where the kernel cannot run. Any device, any strides (the kernel
    takes the (B, n) buffers contiguous or as transposed (n, B) memory);
    nothing synchronises."""
    B, n = dist_in.shape
    k = idx.shape[1]
    dev = dist_in.device
    best = dist_in.clone()
    bp = pred_in.clone()
    # own slots, in slot order; strict improvement keeps the earliest
    for s in range(k):
        u = idx[:, s].long()
        cand = dist_in[:, u.clamp(0, n - 1)] + w[:, s]
        better = (u >= 0).unsqueeze(0) & (cand < best)
        best = torch.where(better, cand, best)
        bp = torch.where(better, u.to(torch.int32).unsqueeze(0), bp)
    # in-lists: per tail the minimum of (candidate, list position)
    E = in_edge.numel()
    if E:
        e = in_edge.long().clamp(0, n * k - 1)
        head = e // k
        tail = torch.repeat_interleave(
            torch.arange(n, device=dev), (in_off[1:] - in_off[:-1]).long(),
            output_size=E)
        cand = dist_in[:, head] + w.reshape(-1)[e]               # (B, E)
        tails = tail.unsqueeze(0).expand(B, E)
        seg = torch.full((B, n), _INF, device=dev).scatter_reduce(
            1, tails, cand, "amin", include_self=True)
        q = torch.arange(E, device=dev).unsqueeze(0).expand(B, E)
        q = torch.where(cand == seg.gather(1, tails), q,
                        torch.full_like(q, E))
        first = torch.full((B, n), E, dtype=torch.int64,
                           device=dev).scatter_reduce(
            1, tails, q, "amin", include_self=True)
        better = seg < best
        best = torch.where(better, seg, best)
        bp = torch.where(better,
                         head[first.clamp(max=E - 1)].to(torch.int32), bp)
    improved = best < dist_in
    if allowed is not None:
        open_ = (allowed != 0).unsqueeze(0)
        best = torch.where(open_, best, torch.full_like(best, _INF))
        bp = torch.where(open_, bp, torch.full_like(bp, -1))
        improved = improved & open_
    dist_out.copy_(best)
    pred_out.copy_(bp)
    changed.masked_fill_(improved.any(dim=1), 1)


def walk_reference(dist: torch.Tensor, pred: torch.Tensor, src: torch.Tensor,
                   dst: torch.Tensor, out: torch.Tensor,
                   count: torch.Tensor) -> None:
    """The statement of _C.path_walk: out[b] holds dst[b] and then its
    predecessors until src[b] is written, a predecessor is missing or the
    row is full; the rest is -1. count[b] is the number of entries, -1
    when dst[b] was not reached."""
    B, n = dist.shape
    T1 = out.shape[1]
    d = dist.cpu()
    p = pred.cpu()
    rows = torch.full((B, T1), -1, dtype=torch.int32)
    counts = torch.full((B,), -1, dtype=torch.int32)
    for b, (s, v) in enumerate(zip(src.tolist(), dst.tolist())):
        if not (0 <= v < n and 0 <= s < n) or not float(d[b, v]) < _INF:
            continue
        c = 0
        while c < T1:
            rows[b, c] = v
            c += 1
            if v == s:
                break
            nxt = int(p[b, v])
            if nxt < 0 or nxt >= n:
                break
            v = nxt
        counts[b] = c
    out.copy_(rows)
    count.copy_(counts)


def _kernels(dev: torch.device):
    """(relax, walk): the fused ops when the graph is on the GPU and the
    extension loads, the torch statements otherwise."""
    from audiomuse_amd.ops import _ext

    ext = _ext.native_or_none() if dev.type == "cuda" else None
    if ext is None:
        return relax_reference, walk_reference
    return ext.path_relax, ext.path_walk


def solve(graph: PathGraph, src: Sequence[int],
          allowed: Optional[torch.Tensor] = None
          ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Single-source shortest paths from each of 1..8 sources: (dist
    (B, n) f32, pred (B, n) int32, sweeps), on the graph's device (the
    two are transposed views of (n, B) memory). Sweeps
    run in groups of SWEEP_GROUP launches; the changed flags are read on
    the host once per group, and a group that leaves them all 0 ends the
    loop. Nothing else in the loop synchronises."""
    B = len(src)
    if not 1 <= B <= MAX_LEGS:
        raise ValueError(f"shortest paths are solved for 1 to {MAX_LEGS} legs")
    n = graph.n
    if any(not 0 <= int(s) < n for s in src):
        raise ValueError("leg endpoints must be positions in [0, n)")
    dev = graph.device
    relax, _ = _kernels(dev)
    if allowed is not None:
        if allowed.shape != (n,):
            raise ValueError("allowed must be (n,)")
        allowed = (allowed != 0).to(device=dev, dtype=torch.uint8).contiguous()
    src_t = torch.tensor([int(s) for s in src], device=dev)
    # (B, n) views of vertex-major memory: the B values of a vertex lie
    # side by side, so the kernel reads a candidate's legs in one piece
    cur_d = torch.full((n, B), _INF, device=dev).t()
    cur_d[torch.arange(B, device=dev), src_t] = 0.0
    if allowed is not None:     # a masked source starts nothing
        cur_d.masked_fill_((allowed == 0).unsqueeze(0), _INF)
    cur_p = torch.full((n, B), -1, dtype=torch.int32, device=dev).t()
    nxt_d = torch.empty(n, B, device=dev).t()
    nxt_p = torch.empty(n, B, dtype=torch.int32, device=dev).t()
    changed = torch.zeros(B, dtype=torch.int32, device=dev)
    sweeps = 0
    while True:
        changed.zero_()
        for _ in range(SWEEP_GROUP):
            relax(cur_d, cur_p, nxt_d, nxt_p, graph.idx, graph.w,
                  graph.in_off, graph.in_edge, allowed, changed)
            cur_d, nxt_d = nxt_d, cur_d
            cur_p, nxt_p = nxt_p, cur_p
        sweeps += SWEEP_GROUP
        # the one host read per group; n - 1 sweeps always suffice
        if not bool(changed.any()) or sweeps >= n + SWEEP_GROUP:
            break
    return cur_d, cur_p, sweeps


def shortest_paths(graph: PathGraph, src: Sequence[int], dst: Sequence[int],
                   allowed: Optional[torch.Tensor] = None
                   ) -> Tuple[List[Optional[List[int]]], torch.Tensor, int]:
    """Shortest paths src[b] -> dst[b] for 1..8 legs in one batch.
    allowed: optional (n) uint8/bool mask; paths stay on allowed vertices.
    Returns (paths, dists, sweeps): paths[b] the positions from src[b] to
    dst[b] (None when unreachable), dists (B,) f32 on the CPU (+inf when
    unreachable), sweeps the number of sweeps run. The fused kernel runs
    when the graph is on the GPU and the extension loads, the torch
    reference otherwise."""
    B = len(src)
    n = graph.n
    if len(dst) != B or not 1 <= B <= MAX_LEGS:
        raise ValueError(f"shortest_paths takes 1 to {MAX_LEGS} legs")
    src = [int(s) for s in src]
    dst = [int(t) for t in dst]
    if any(not 0 <= v < n for v in src + dst):
        raise ValueError("leg endpoints must be positions in [0, n)")
    if allowed is None and src == dst:
        return [[s] for s in src], torch.zeros(B), 0
    dev = graph.device
    dist, pred, sweeps = solve(graph, src, allowed)
    _, walk = _kernels(dev)
    src_t = torch.tensor(src, dtype=torch.int32, device=dev)
    dst_t = torch.tensor(dst, dtype=torch.int32, device=dev)
    out = torch.empty(B, sweeps + 1, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    walk(dist, pred, src_t, dst_t, out, count)
    dists = dist[torch.arange(B, device=dev), dst_t.long()].cpu()
    out_h = out.cpu()
    paths: List[Optional[List[int]]] = []
    for b, c in enumerate(count.tolist()):
        chain = out_h[b, :c].tolist()[::-1] if c > 0 else None
        if chain is None or chain[0] != src[b]:
            paths.append(None)
        else:
            paths.append(chain)
    return paths, dists, sweeps


def thin(tracks: Sequence, stops: Sequence, length: int) -> List:
    """Shorten a journey to `length` tracks. All stops (start, via stops,
    end; members of tracks) are kept; with m = length - len(stops) free
    slots and I the interior tracks in order, I[floor((j + 0.5) * len(I)
    / m)] is kept for j = 0..m-1. m <= 0 returns the stops only; a list
    of at most `length` tracks is returned unchanged."""
    tracks = list(tracks)
    if len(tracks) <= length:
        return tracks
    stop_set = set(stops)
    m = length - len(stops)
    if m <= 0:
        return [t for t in tracks if t in stop_set]
    interior = [i for i, t in enumerate(tracks) if t not in stop_set]
    keep = {interior[((2 * j + 1) * len(interior)) // (2 * m)]
            for j in range(m)}
    return [t for i, t in enumerate(tracks) if t in stop_set or i in keep]
