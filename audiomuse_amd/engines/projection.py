"""2-D map projection: first-party UMAP-style layout on torch.

Reference capability: /root/reference/alchemy_projections.py:78
(_project_with_umap; umap-learn with PCA fallback) feeding the Music Map
(app_map.py) and alchemy projections. umap-learn is not in this image;
this is our own implementation of the same construction — exact kNN
graph (chunked GEMM distances, GPU-capable), smooth-kNN fuzzy weights,
PCA init, and the standard UMAP attract/repel SGD with negative
sampling — vectorized over all edges per epoch on the device.

Two engines run the epochs (config.MAP_LAYOUT_ENGINE): "torch", the eager
loop above, and "fused", a pull formulation whose epoch is one HIP launch
(ops/csrc/layout.hip) with layout_epoch_reference as its torch statement.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from audiomuse_amd.cluster.algorithms import _pairwise_sq, pca_fit_transform

# curve parameters for min_dist=0.1 (standard UMAP fit)
_A, _B = 1.577, 0.895


def knn_graph(x: torch.Tensor, k: int, chunk: int = 4096
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dists (n,k), idx (n,k)) excluding self; euclidean."""
    n = x.shape[0]
    dists = torch.empty(n, k, device=x.device)
    idx = torch.empty(n, k, dtype=torch.long, device=x.device)
    for s in range(0, n, chunk):
        d = _pairwise_sq(x[s : s + chunk], x)
        d[torch.arange(d.shape[0]), torch.arange(s, s + d.shape[0])] = float("inf")
        top = torch.topk(d, k, dim=1, largest=False)
        dists[s : s + chunk] = top.values.clamp(min=0).sqrt()
        idx[s : s + chunk] = top.indices
    return dists, idx


def smooth_knn_weights(dists: torch.Tensor, n_iter: int = 32) -> torch.Tensor:
    """Per-point sigma via bisection so sum_j exp(-(d_j - rho)/sigma) =
    log2(k) (UMAP smooth_knn_dist)."""
    k = dists.shape[1]
    target = math.log2(k)
    rho = dists[:, 0:1]
    lo = torch.full_like(rho, 1e-6)
    hi = torch.full_like(rho, 1e3)
    for _ in range(n_iter):
        mid = (lo + hi) / 2
        val = torch.exp(-(dists - rho).clamp(min=0) / mid).sum(dim=1, keepdim=True)
        hi = torch.where(val > target, mid, hi)
        lo = torch.where(val <= target, mid, lo)
    sigma = (lo + hi) / 2
    return torch.exp(-(dists - rho).clamp(min=0) / sigma)


def _layout_setup(x: torch.Tensor, n_neighbors: int, seed: int,
                  knn: Optional[Tuple[torch.Tensor, torch.Tensor]]):
    """Everything umap_project does before its epoch loop, shared by both
    engines: the neighbour graph, the smooth-kNN weights, the symmetrise
    join and the PCA init. Returns (idx (n, k) long, wsym (n*k,), emb
    (n, 2), g): g is the seeded CPU generator after the init noise was
    drawn from it (the torch engine goes on drawing from it)."""
    n = x.shape[0]
    if knn is None:
        k = min(n_neighbors, n - 1)
        dists, idx = knn_graph(x, k)
    else:
        dists = knn[0].to(device=x.device, dtype=torch.float32)
        idx = knn[1].to(device=x.device, dtype=torch.long)
        if dists.shape != idx.shape or dists.shape[0] != n:
            raise ValueError("knn must be (dists (n, k), idx (n, k))")
        k = idx.shape[1]
    w = smooth_knn_weights(dists)

    # symmetrize: treat (i -> idx[i,j]) directed weights; w_sym = a+b-ab.
    # Reverse-edge lookup via sorted searchsorted (a Python dict over
    # n*k edges took minutes at 10^6 rows — this is the same join fully
    # on-device)
    rows = torch.arange(n, device=x.device).unsqueeze(1).expand(-1, k).reshape(-1)
    cols = idx.reshape(-1)
    vals = w.reshape(-1)
    key = rows * n + cols
    rkey = cols * n + rows
    skey, order = torch.sort(key)
    pos = torch.searchsorted(skey, rkey)
    pos = pos.clamp(max=skey.numel() - 1)
    hit = skey[pos] == rkey
    rvals = torch.where(hit, vals[order][pos], torch.zeros_like(vals))
    wsym = vals + rvals - vals * rvals

    g = torch.Generator(device="cpu").manual_seed(seed)
    init, _, _ = pca_fit_transform(x, 2)
    emb = (init / (init.std() + 1e-9)).contiguous() * 10.0
    emb += torch.randn(emb.shape, generator=g).to(x.device) * 0.01
    return idx, wsym, emb, g


def _torch_layout(emb: torch.Tensor, idx: torch.Tensor, wsym: torch.Tensor,
                  g: torch.Generator, epochs: int, lr: float,
                  neg_samples: int) -> torch.Tensor:
    """The eager engine: every epoch samples edges and negatives from the
    host generator and scatters the forces with index_add_."""
    n, k = idx.shape
    dev = emb.device
    rows = torch.arange(n, device=dev).unsqueeze(1).expand(-1, k).reshape(-1)
    cols = idx.reshape(-1)
    edge_i, edge_j, edge_w = rows, cols, wsym / wsym.max().clamp(min=1e-12)
    for epoch in range(epochs):
        alpha = lr * (1.0 - epoch / epochs)
        keep = torch.rand(edge_w.shape[0], generator=g).to(dev) <= edge_w
        ei, ej = edge_i[keep], edge_j[keep]
        if ei.numel() == 0:
            continue
        # attraction
        delta = emb[ei] - emb[ej]
        d2 = delta.square().sum(dim=1, keepdim=True)
        grad_coef = (-2.0 * _A * _B * d2.clamp(min=1e-12) ** (_B - 1)) / \
                    (1.0 + _A * d2 ** _B)
        grad = (grad_coef * delta).clamp(-4.0, 4.0)
        emb.index_add_(0, ei, grad * alpha)
        emb.index_add_(0, ej, -grad * alpha)
        # repulsion: negative samples
        for _ in range(neg_samples):
            nj = torch.randint(0, n, (ei.shape[0],), generator=g).to(dev)
            delta = emb[ei] - emb[nj]
            d2 = delta.square().sum(dim=1, keepdim=True)
            grad_coef = (2.0 * _B) / ((0.001 + d2) * (1.0 + _A * d2 ** _B))
            grad = (grad_coef * delta).clamp(-4.0, 4.0)
            emb.index_add_(0, ei, grad * alpha)
    return emb


# ---------------------------------------------------------------------------
# Fused engine: one epoch = one pull pass in which every vertex is computed
# by one owner (docs/ALGORITHM.md "Fused map layout"). The HIP kernel
# (ops/csrc/layout.hip) and layout_epoch_reference below state the same
# epoch; sampling and negative indices come from an integer hash, so the
# two take the same decisions and differ by float rounding only.
# ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF
LAYOUT_MAX_EDGES = 2 ** 31      # n*k has to stay below this


def _check_edge_count(n: int, k: int) -> None:
    if n * k >= LAYOUT_MAX_EDGES:
        raise ValueError(f"fused layout is limited to n*k < 2^31 edges "
                         f"(got {n} x {k})")


def _mul32(h: torch.Tensor, c: int) -> torch.Tensor:
    """(h * c) mod 2^32 for int64 h in [0, 2^32): split so that no
    intermediate leaves the int64 range."""
    return ((h & 0xFFFF) * c + ((((h >> 16) * c) & 0xFFFF) << 16)) & _M32


def _mix32(h: torch.Tensor) -> torch.Tensor:
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def _mix32_int(h: int) -> int:
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def layout_hash_base(seed: int, epoch: int) -> int:
    return _mix32_int((seed & _M32) ^ (((epoch + 1) * 0x9E3779B9) & _M32))


def layout_draw(seed: int, epoch: int, e: torch.Tensor, d: int
                ) -> torch.Tensor:
    """draw(e, d) of the fused epoch for int64 edge ids e: uint32 values
    held in int64."""
    h0 = _mix32((layout_hash_base(seed, epoch) + e) & _M32)
    return _mix32((h0 + d) & _M32)


def layout_thresholds(idx: torch.Tensor, w_norm: torch.Tensor) -> torch.Tensor:
    """(n, k) int32 sampling thresholds round(w_norm * 2^24) in [0, 2^24];
    0 where the slot holds no neighbour (idx < 0)."""
    thr = torch.round(w_norm.reshape(idx.shape).float().clamp(0.0, 1.0)
                      * float(1 << 24)).to(torch.int32)
    return torch.where(idx < 0, torch.zeros_like(thr), thr)


def layout_reverse_lists(idx: torch.Tensor, thr: torch.Tensor
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reverse adjacency of the edges that can ever be sampled (thr > 0):
    in_off (n+1,) and in_edge (E_in,) int32; vertex i is the tail of the
    edges e = j*k + s listed in in_edge[in_off[i]:in_off[i+1]], ascending."""
    n, k = idx.shape
    _check_edge_count(n, k)
    e_ids = torch.nonzero(thr.reshape(-1) > 0).reshape(-1)
    tails = idx.reshape(-1)[e_ids].long()
    _, order = torch.sort(tails, stable=True)
    in_edge = e_ids[order].to(torch.int32)
    counts = torch.bincount(tails, minlength=n)
    in_off = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    in_off[1:] = torch.cumsum(counts, 0)
    return in_off.to(torch.int32), in_edge


def _attract(delta: torch.Tensor) -> torch.Tensor:
    d2 = delta.square().sum(dim=1, keepdim=True)
    coef = (-2.0 * _A * _B * d2.clamp(min=1e-12) ** (_B - 1)) / \
           (1.0 + _A * d2 ** _B)
    return (coef * delta).clamp(-4.0, 4.0)


def _repel(delta: torch.Tensor) -> torch.Tensor:
    d2 = delta.square().sum(dim=1, keepdim=True)
    coef = (2.0 * _B) / ((0.001 + d2) * (1.0 + _A * d2 ** _B))
    return (coef * delta).clamp(-4.0, 4.0)


def layout_epoch_reference(E: torch.Tensor, idx: torch.Tensor,
                           thr: torch.Tensor, in_off: torch.Tensor,
                           in_edge: torch.Tensor, alpha: float, seed: int,
                           epoch: int, neg: int,
                           dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One epoch of the fused layout engine in torch: the golden reference
    of the HIP kernel and the engine's path where the kernel cannot run.
    Vectorised over vertices, sequential over the k slots; any device,
    f32 or f64. Returns the new (n, 2) positions; E is left unchanged."""
    n, k = idx.shape
    _check_edge_count(n, k)
    dev = E.device
    pos = E.to(dtype)
    idxl = idx.long()
    base = layout_hash_base(seed, epoch)
    eid = torch.arange(n * k, device=dev).view(n, k)
    h0 = _mix32((base + eid) & _M32)
    sampled = (_mix32(h0) >> 8) < thr.long()

    # step 1: tail pulls, from the input positions on both ends
    ie = in_edge.long()
    head = ie // k
    tail = torch.repeat_interleave(torch.arange(n, device=dev),
                                   (in_off[1:] - in_off[:-1]).long(),
                                   output_size=ie.numel())
    force = _attract(pos[head] - pos[tail])
    force = force * sampled.view(-1)[ie].unsqueeze(1).to(dtype)
    p = pos - alpha * torch.zeros_like(pos).index_add_(0, tail, force)

    # step 2: own edges, sequential on the running position
    for s in range(k):
        on = sampled[:, s:s + 1]
        nb = pos[idxl[:, s].clamp(min=0)]
        p = torch.where(on, p + alpha * _attract(p - nb), p)
        for t in range(neg):
            nj = (_mix32((h0[:, s] + (t + 1)) & _M32) * n) >> 32
            p = torch.where(on, p + alpha * _repel(p - pos[nj]), p)
    return p


def _run_fused_epochs(emb: torch.Tensor, idx: torch.Tensor, thr: torch.Tensor,
                      in_off: torch.Tensor, in_edge: torch.Tensor,
                      epochs: int, lr: float, neg: int, seed: int
                      ) -> torch.Tensor:
    """The fused engine's epoch loop: one launch per epoch on two
    ping-pong buffers, nothing read back to the host."""
    from audiomuse_amd.ops import _ext

    ext = _ext.native_or_none() if emb.is_cuda else None
    if ext is None:
        for epoch in range(epochs):
            alpha = lr * (1.0 - epoch / epochs)
            emb = layout_epoch_reference(emb, idx, thr, in_off, in_edge,
                                         alpha, seed, epoch, neg)
        return emb
    idx32 = idx.to(torch.int32).contiguous()
    thr = thr.contiguous()
    in_thr = thr.reshape(-1)[in_edge.long()].contiguous()
    cur = emb.float().contiguous()
    nxt = torch.empty_like(cur)
    for epoch in range(epochs):
        alpha = lr * (1.0 - epoch / epochs)
        ext.umap_epoch(cur, nxt, idx32, thr, in_off, in_edge, in_thr,
                       alpha, _A, _B, seed, epoch, neg)
        cur, nxt = nxt, cur
    return cur


def _fused_layout(emb: torch.Tensor, idx: torch.Tensor, wsym: torch.Tensor,
                  epochs: int, lr: float, neg_samples: int, seed: int
                  ) -> torch.Tensor:
    n = idx.shape[0]
    _check_edge_count(n, idx.shape[1])
    if bool((idx >= n).any()):
        raise ValueError("neighbour positions must be below n")
    thr = layout_thresholds(idx, wsym / wsym.max().clamp(min=1e-12))
    in_off, in_edge = layout_reverse_lists(idx, thr)
    return _run_fused_epochs(emb, idx, thr, in_off, in_edge, epochs, lr,
                             neg_samples, seed)


LAYOUT_ENGINES = ("torch", "fused")


def umap_project(x: torch.Tensor, n_neighbors: int = 15, epochs: int = 200,
                 lr: float = 1.0, neg_samples: int = 5,
                 seed: int = 0,
                 knn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                 engine: Optional[str] = None) -> torch.Tensor:
    """(n, d) -> (n, 2) layout. knn: optional precomputed neighbour graph
    (dists (n, k) euclidean, idx (n, k) positions into x, self excluded),
    e.g. from IVFIndex.knn_graph; without it the exact graph is built.
    engine: "torch" (eager epochs, host RNG) or "fused" (one HIP launch
    per epoch); None takes config.MAP_LAYOUT_ENGINE."""
    if engine is None:
        from audiomuse_amd import config as C

        engine = C.MAP_LAYOUT_ENGINE
    if engine not in LAYOUT_ENGINES:
        raise ValueError(f"layout engine must be torch or fused, "
                         f"not {engine!r}")
    x = x.float()
    n = x.shape[0]
    if n <= 3:
        return torch.zeros(n, 2, device=x.device)
    idx, wsym, emb, g = _layout_setup(x, n_neighbors, seed, knn)
    if engine == "fused":
        return _fused_layout(emb, idx, wsym, epochs, lr, neg_samples, seed)
    return _torch_layout(emb, idx, wsym, g, epochs, lr, neg_samples)
