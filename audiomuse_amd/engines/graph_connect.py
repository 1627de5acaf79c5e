"""Connected kNN graph: component labels and cross-component bridges.

The k-neighbour graph of a clustered catalogue falls into islands, and the
graph song path and the graph radio cannot leave the island they start on.
This module labels the components of the symmetrised graph, finds for the
vertices outside the largest component their nearest neighbours in other
components (IVFIndex.foreign_neighbours: the label exclusion runs inside
the index scan), and adds the lightest of those edges as bridges until one
component is left.

The label sweep is one HIP launch (ops/csrc/components.hip);
label_pull_reference below is its torch statement, bit-identical to the
kernel (integers only), and the path taken where the kernel cannot run
(docs/ALGORITHM.md "Connected graph").
"""

from __future__ import annotations

import time
from typing import Dict, List, Tuple

import torch

from audiomuse_amd.engines.projection import layout_reverse_lists

# Sweeps between two reads of the changed flag, as graph_path.SWEEP_GROUP:
# on kNN graphs the labels settle in a handful of sweeps, so a larger group
# would mostly run sweeps that change nothing.
SWEEP_GROUP = 2


def label_pull_reference(label_in: torch.Tensor, label_out: torch.Tensor,
                         idx: torch.Tensor, in_off: torch.Tensor,
                         in_edge: torch.Tensor, changed: torch.Tensor) -> None:
    """One sweep in torch, with the signature and the exact results of
    _C.graph_label_pull: m = min(label_in[v], label_in[u] over v's own
    slots and its in-list), label_out[v] = label_in[m]; changed[0] is set
    to 1 when a label dropped and never written otherwise. Any device;
    nothing synchronises."""
    n, k = idx.shape
    dev = label_in.device
    if n == 0:
        return
    m = label_in.clone()
    for s in range(k):
        u = idx[:, s].long()
        cand = label_in[u.clamp(0, n - 1)]
        m = torch.where(u >= 0, torch.minimum(m, cand), m)
    E = in_edge.numel()
    if E:
        head = in_edge.long().clamp(0, n * k - 1) // k
        tail = torch.repeat_interleave(
            torch.arange(n, device=dev), (in_off[1:] - in_off[:-1]).long(),
            output_size=E)
        m = m.scatter_reduce(0, tail, label_in[head], "amin",
                             include_self=True)
    out = label_in[m.clamp(0, n - 1).long()]
    changed.masked_fill_((out < label_in).any(), 1)
    label_out.copy_(out)


def _kernel(dev: torch.device):
    """The fused sweep when the graph is on the GPU and the extension
    loads, the torch statement otherwise."""
    from audiomuse_amd.ops import _ext

    ext = _ext.native_or_none() if dev.type == "cuda" else None
    return label_pull_reference if ext is None else ext.graph_label_pull


def adjacency(pos: torch.Tensor, dists: torch.Tensor
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(idx (n, k) int32, in_off, in_edge) of a neighbour table: the slots
    PathGraph.from_knn and RankGraph.from_knn fill (pos >= 0 with a finite
    distance) and their reverse lists."""
    if pos.dim() != 2 or dists.shape != pos.shape or pos.shape[1] < 1:
        raise ValueError("pos and dists must both be (n, k), k >= 1")
    if bool((pos >= pos.shape[0]).any()):
        raise ValueError("neighbour positions must be below n")
    filled = (pos >= 0) & torch.isfinite(dists.float())
    idx = torch.where(filled, pos, torch.full_like(pos, -1)).to(torch.int32)
    in_off, in_edge = layout_reverse_lists(idx, filled.to(torch.int32))
    return idx.contiguous(), in_off.contiguous(), in_edge.contiguous()


def component_labels(idx: torch.Tensor, in_off: torch.Tensor,
                     in_edge: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(labels (n,) int32, sweeps): the smallest vertex id of each vertex's
    component in the symmetrised graph, on idx's device. Sweeps run in
    groups of SWEEP_GROUP launches; the changed flag is read on the host
    once per group and nothing else synchronises. n sweeps always
    suffice."""
    n = idx.shape[0]
    dev = idx.device
    cur = torch.arange(n, dtype=torch.int32, device=dev)
    if n == 0:
        return cur, 0
    pull = _kernel(dev)
    nxt = torch.empty_like(cur)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    sweeps = 0
    while True:
        changed.zero_()
        for _ in range(SWEEP_GROUP):
            pull(cur, nxt, idx, in_off, in_edge, changed)
            cur, nxt = nxt, cur
        sweeps += SWEEP_GROUP
        if not bool(changed.any()) or sweeps >= n + SWEEP_GROUP:
            break
    return cur, sweeps


def _widen(pos: torch.Tensor, dists: torch.Tensor,
           bridges: List[Tuple[int, int, float]]
           ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """pos / dists with the bridges (tail, head, distance) in extra
    columns at their tails, in the order given: (n, k + x), x the largest
    number of bridges on one tail, -1 / +inf elsewhere."""
    if not bridges:
        return pos, dists, 0
    n = pos.shape[0]
    fill: Dict[int, int] = {}
    col = []
    for u, _v, _d in bridges:
        col.append(fill.get(u, 0))
        fill[u] = col[-1] + 1
    x = max(fill.values())
    dev = pos.device
    extra_p = torch.full((n, x), -1, dtype=pos.dtype, device=dev)
    extra_d = torch.full((n, x), float("inf"), dtype=dists.dtype, device=dev)
    u = torch.tensor([b[0] for b in bridges], device=dev)
    c = torch.tensor(col, device=dev)
    extra_p[u, c] = torch.tensor([b[1] for b in bridges], dtype=pos.dtype,
                                 device=dev)
    extra_d[u, c] = torch.tensor([b[2] for b in bridges], dtype=dists.dtype,
                                 device=dev)
    return (torch.cat([pos, extra_p], dim=1).contiguous(),
            torch.cat([dists, extra_d], dim=1).contiguous(), x)


def _lightest_per_pair(u: torch.Tensor, v: torch.Tensor, w: torch.Tensor,
                       cu: torch.Tensor, cv: torch.Tensor, n: int
                       ) -> torch.Tensor:
    """Indices of the candidate edges that are the lightest of their
    unordered component pair, in ascending (weight, min(u, v), max(u, v))
    order. All on the device of the inputs."""
    lo, hi = torch.minimum(u, v), torch.maximum(u, v)
    order = torch.sort(hi, stable=True).indices
    order = order[torch.sort(lo[order], stable=True).indices]
    order = order[torch.sort(w[order], stable=True).indices]
    pair = (torch.minimum(cu, cv) * n + torch.maximum(cu, cv))[order]
    by_pair = torch.sort(pair, stable=True)
    first = torch.ones_like(pair, dtype=torch.bool)
    first[1:] = by_pair.values[1:] != by_pair.values[:-1]
    # ranks in the (weight, lo, hi) order of the first edge of each pair
    keep = torch.sort(by_pair.indices[first]).values
    return order[keep]


def connect(pos: torch.Tensor, dists: torch.Tensor, index, candidates: int,
            max_rounds: int, nprobe=None
            ) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """Bridge the components of a neighbour table.

    pos (n, k) int64 / dists (n, k): SimilarityEngine.neighbor_graph, in
    item-ids order; index: the IVFIndex it was built from (index.ids are
    positions). Returns (pos', dists', report): the table with the bridges
    in extra columns (_widen) and the figures of the run.

    Each round labels the current graph, asks the index for the
    `candidates` nearest rows in other components of every vertex outside
    the largest component (ties on size: the smallest label), keeps the
    lightest candidate per unordered component pair (on the device) and
    runs Kruskal over those on the host in (weight, min(u, v), max(u, v))
    order; an edge is accepted when it merges two components. It stops
    with one component, after max_rounds rounds, or when a round adds
    nothing. Vertices the index does not hold are never queried or
    bridged; they are counted in report["without_vector"]. For every
    component queried in a round, the lightest candidate edge that leaves
    it is among the accepted ones (the cut property under unique keys)."""
    t0 = time.perf_counter()
    candidates = int(candidates)
    if candidates < 1:
        raise ValueError("candidates must be >= 1")
    n = pos.shape[0]
    dev = pos.device
    N = index.n
    ids = index.ids.to(dev)
    has_vec = torch.zeros(n, dtype=torch.bool, device=dev)
    has_vec[ids] = True
    row_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
    row_of[ids] = torch.arange(N, device=dev)
    bridges: List[Tuple[int, int, float]] = []
    report: Dict = {
        "connect": True, "vertices": n,
        "without_vector": n - int(has_vec.sum()),
        "components_before": 0, "largest_before": 0, "components_after": 0,
        "bridges": 0, "rounds": 0, "extra_slots": 0, "seconds": 0.0,
        "label_sweeps": [], "label_seconds": [], "scan_seconds": [],
        "bridges_per_round": [],
    }
    rounds = 0
    cur_pos, cur_d = pos, dists
    while True:
        t1 = time.perf_counter()
        labels, sweeps = component_labels(*adjacency(cur_pos, cur_d))
        uniq, counts = torch.unique(labels[has_vec], return_counts=True)
        report["label_sweeps"].append(sweeps)
        report["label_seconds"].append(time.perf_counter() - t1)
        ncomp = int(uniq.numel())
        if rounds == 0:
            report["components_before"] = ncomp
            report["largest_before"] = int(counts.max()) if ncomp else 0
        report["components_after"] = ncomp
        if ncomp <= 1 or rounds >= max_rounds:
            break
        rounds += 1
        big = uniq[counts == counts.max()].min()
        qpos = (has_vec & (labels != big)).nonzero(as_tuple=True)[0]
        t1 = time.perf_counter()
        fd, fi = index.foreign_neighbours(labels[ids], candidates,
                                          rows=row_of[qpos], nprobe=nprobe)
        fd, fi = fd.to(dev), fi.to(dev)
        ok = (fi >= 0) & torch.isfinite(fd)
        u = qpos.unsqueeze(1).expand_as(fi)[ok]
        v = fi[ok]
        w = fd[ok]
        cu, cv = labels[u].long(), labels[v].long()
        keep = _lightest_per_pair(u, v, w, cu, cv, n)
        eu, ev = u[keep].tolist(), v[keep].tolist()
        ew = w[keep].tolist()
        ea, eb = cu[keep].tolist(), cv[keep].tolist()
        report["scan_seconds"].append(time.perf_counter() - t1)
        # Kruskal over component labels, union by smaller label
        parent: Dict[int, int] = {}

        def find(a: int) -> int:
            root = a
            while parent.get(root, root) != root:
                root = parent[root]
            while parent.get(a, a) != root:
                parent[a], a = root, parent[a]
            return root

        added = 0
        for a, b, tail, head, d in zip(ea, eb, eu, ev, ew):
            ra, rb = find(a), find(b)
            if ra == rb:
                continue
            parent[max(ra, rb)] = min(ra, rb)
            bridges.append((tail, head, d))
            added += 1
            if added == ncomp - 1:
                break
        report["bridges_per_round"].append(added)
        if not added:
            break
        cur_pos, cur_d, _ = _widen(pos, dists, bridges)
    out_pos, out_d, x = _widen(pos, dists, bridges)
    report["bridges"] = len(bridges)
    report["rounds"] = rounds
    report["extra_slots"] = x
    report["seconds"] = time.perf_counter() - t0
    return out_pos, out_d, report


def bridges_of(pos: torch.Tensor, dists: torch.Tensor, k: int
               ) -> List[Tuple[int, int, float]]:
    """The bridges (tail, head, distance) of a table widened by connect,
    k being the width it had before."""
    extra = pos[:, k:]
    at = (extra >= 0).nonzero()
    return [(int(u), int(extra[u, c]), float(dists[u, k + c]))
            for u, c in at.tolist()]
