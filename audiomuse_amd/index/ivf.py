"""HBM-resident IVF similarity index.

Re-design of the reference's disk-paged IVF engine
(/root/reference/tasks/paged_ivf.py: AMIV cell blobs, L1/L2 LRU caches,
mmap + idle page-drop, thread-pool NumKong scans) for a machine with
288 GB of HBM3E per GPU: every cell lives packed in GPU memory, the
probed-cell scan is one HIP kernel launch (ops/csrc/distance.hip), and
persistence is a single serialized state blob in SQL storage instead of
per-cell pages. Query semantics match the reference:

- nlist = min(8*sqrt(N), IVF_NLIST_MAX), mini-batch k-means coarse
  quantizer with random init (paged_ivf.py:1411-1460)
- storage dtypes i8 (x127, angular-only; auto-downgrade to f16 for other
  metrics), f16, f32 (ivf_quant.py:effective_code)
- distance semantics: angular = 1 - clip(cos), euclidean = sqrt(ssd),
  dot = -dot (ivf_quant.py:_cell_distances_np)
- query: rank cells by centroid distance, scan top-nprobe cells,
  over-fetch, exact-f32 re-rank upstream (paged_ivf.py:1067-1101,
  ivf_manager.py:889-933)

CPU hosts run a vectorized torch fallback of the identical math (used
by the unit tests as the kernel's golden reference).
"""

from __future__ import annotations

import io
import itertools
import math
from dataclasses import dataclass
from typing import Iterable, Optional, Tuple, Union

import torch

from audiomuse_amd import config as C
from audiomuse_amd.ops import _ext
from audiomuse_amd.ops.kmeans import assign_to_centroids, minibatch_kmeans

_METRIC_CODE = {"angular": 0, "euclidean": 1, "dot": 2}
_DTYPE_CODE = {"f32": 0, "f16": 1, "i8": 2}

# The fused scan + top-K kernel keeps at most this many candidates per
# (query, split) (TK_KMAX in ops/csrc/distance.hip); scan_topk() takes the
# unfused path beyond it.
TOPK_KMAX = 256
_TOPK_MAX_Q = 32768   # queries per launch (grid.y stays below 65536)

# Every packed layout gets a process-unique version, so a RowScope can
# never be applied to a layout (or an index) it was not built from.
_LAYOUT_VERSIONS = itertools.count(1)


@dataclass(frozen=True)
class RowScope:
    """Row selection for scoped queries (reference: the per-server
    availability mask, paged_ivf.py:_availability_mask). Holds packed-row
    indices, so it is only valid for the layout it was built from."""

    rows: torch.Tensor   # (M,) int32 allowed packed rows, ascending
    off: torch.Tensor    # (ncells+1,) int32 prefix offsets of rows per cell
    n: int               # M
    version: int         # IVFIndex.layout_version at build time


def effective_storage(storage: str, metric: str) -> str:
    """i8 is angular-only; other metrics downgrade to f16 (ivf_quant.py)."""
    if storage == "i8" and metric != "angular":
        return "f16"
    return storage


def encode_vectors(vecs: torch.Tensor, storage: str) -> torch.Tensor:
    vecs = vecs.float()
    if storage == "i8":
        return torch.clamp(torch.round(vecs * 127.0), -127, 127).to(torch.int8)
    if storage == "f16":
        return vecs.to(torch.float16)
    return vecs


def decode_vectors(enc: torch.Tensor, storage: str) -> torch.Tensor:
    """Inverse of encode_vectors (the codec contract the scan kernels
    assume; i8 rows are x*127 rounded, reference ivf_quant.py:42)."""
    if storage == "i8":
        return enc.float() / 127.0
    return enc.float()


def default_nlist(n: int) -> int:
    """min(8*sqrt(N), IVF_NLIST_MAX), >= 1 (paged_ivf.py:1412-1413)."""
    return max(1, min(int(8 * math.sqrt(max(n, 1))), C.IVF_NLIST_MAX))


class IVFIndex:
    """Packed-cell IVF index. All tensors live on `self.device`."""

    def __init__(self, dim: int, metric: Optional[str] = None,
                 storage: Optional[str] = None,
                 device: str | torch.device = "cpu"):
        metric = metric or C.IVF_METRIC
        if metric not in _METRIC_CODE:
            raise ValueError(f"unknown metric {metric}")
        self.dim = dim
        self.metric = metric
        self.storage = effective_storage(storage or C.IVF_STORAGE_DTYPE, metric)
        self.device = torch.device(device)
        # i8 rows are int32-packed for the sdot4 kernel: pad dim to /4
        self.dim_pad = ((dim + 3) // 4 * 4) if self.storage == "i8" else dim
        self.centroids: Optional[torch.Tensor] = None   # (nlist, dim) f32
        self.data: Optional[torch.Tensor] = None        # (N, dim_pad) encoded
        self.row_norm: Optional[torch.Tensor] = None    # (N,) f32 encoded-domain
        self.cell_off: Optional[torch.Tensor] = None    # (nlist+1,) int32
        self.ids: Optional[torch.Tensor] = None         # (N,) int64
        self.vectors_f32: Optional[torch.Tensor] = None  # (N, dim) exact re-rank
        self.id_to_row: dict[int, int] = {}
        self.layout_version = next(_LAYOUT_VERSIONS)

    # -- build ------------------------------------------------------------

    @classmethod
    def build(cls, vectors: torch.Tensor, ids: Optional[torch.Tensor] = None,
              metric: Optional[str] = None, storage: Optional[str] = None,
              nlist: Optional[int] = None, device: str | torch.device = "cpu",
              seed: int = 0, keep_f32: bool = True,
              group: Optional[object] = None) -> "IVFIndex":
        """vectors: (N, dim) f32. group: optional dist group for multi-GPU
        k-means training (each rank passes its shard; cells are packed from
        the local shard only — callers all-gather shards first for a
        replicated index)."""
        vectors = torch.as_tensor(vectors, dtype=torch.float32).to(device)
        n, dim = vectors.shape
        idx = cls(dim, metric=metric, storage=storage, device=device)
        metric = idx.metric  # None resolved to C.IVF_METRIC

        if metric == "angular":
            norms = vectors.norm(dim=1, keepdim=True).clamp(min=1e-12)
            unit = vectors / norms
        else:
            unit = vectors

        nlist = nlist or default_nlist(n)
        n_train = min(n, C.IVF_TRAIN_POINTS_PER_CELL * nlist)
        g = torch.Generator().manual_seed(seed)
        sample = unit[torch.randperm(n, generator=g)[:n_train].to(device)]
        centroids = minibatch_kmeans(sample, nlist, iters=C.IVF_KMEANS_ITERS,
                                     batch=C.IVF_KMEANS_BATCH,
                                     seed=seed, group=group)
        assign = assign_to_centroids(unit, centroids)

        # oversized-cell split (reference paged_ivf.py:1337-1343): any
        # cell beyond IVF_MAX_CELL_ROWS is re-clustered with a
        # sub-k-means; its members spread over the new sub-centroids so
        # a scan's per-cell work stays bounded
        max_rows = int(C.IVF_MAX_CELL_ROWS)
        if max_rows > 0 and group is None:
            counts0 = torch.bincount(assign, minlength=nlist)
            over = (counts0 > max_rows).nonzero(as_tuple=True)[0]
            if over.numel():
                import math as _math
                new_cents = [centroids]
                next_id = nlist
                for c in over.tolist():
                    idxs = (assign == c).nonzero(as_tuple=True)[0]
                    k_sub = min(int(_math.ceil(idxs.numel() / max_rows)),
                                idxs.numel())
                    if k_sub < 2:
                        continue
                    sub_c = minibatch_kmeans(unit[idxs], k_sub, iters=15,
                                             batch=C.IVF_KMEANS_BATCH,
                                             seed=seed + c + 1)
                    sub_assign = assign_to_centroids(unit[idxs], sub_c)
                    # sub-cluster 0 keeps cell id c; the rest append
                    centroids[c] = sub_c[0]
                    remap = torch.full((k_sub,), c, dtype=assign.dtype,
                                       device=device)
                    remap[1:] = torch.arange(
                        next_id, next_id + k_sub - 1, device=device)
                    assign[idxs] = remap[sub_assign]
                    new_cents.append(sub_c[1:])
                    next_id += k_sub - 1
                if next_id > nlist:
                    centroids = torch.cat(new_cents, dim=0).contiguous()
                    nlist = next_id

        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=nlist)
        cell_off = torch.zeros(nlist + 1, dtype=torch.int32, device=device)
        cell_off[1:] = torch.cumsum(counts, dim=0).to(torch.int32)

        sorted_unit = unit[order]
        enc = encode_vectors(sorted_unit, idx.storage)
        if idx.dim_pad != dim:
            pad = torch.zeros(n, idx.dim_pad - dim, dtype=enc.dtype, device=device)
            enc = torch.cat([enc, pad], dim=1)
        if ids is None:
            ids = torch.arange(n, dtype=torch.int64)
        ids = torch.as_tensor(ids, dtype=torch.int64).to(device)

        idx.centroids = centroids.contiguous()
        idx.data = enc.contiguous()
        idx.row_norm = enc.float().norm(dim=1).contiguous()
        idx.cell_off = cell_off.contiguous()
        idx.ids = ids[order].contiguous()
        if keep_f32:
            idx.vectors_f32 = vectors[order].contiguous()
        idx._rebuild_id_map()
        idx.layout_version = next(_LAYOUT_VERSIONS)
        return idx

    def _rebuild_id_map(self) -> None:
        self.id_to_row = {int(v): i for i, v in enumerate(self.ids.tolist())}

    # -- incremental update ------------------------------------------------
    # The reference rebuilds its IVF wholesale on every index task
    # (ivf_manager.py rebuild path); with the whole index HBM-resident a
    # packed-layout splice is cheap, so new/removed tracks can be folded in
    # without re-training the coarse quantizer. The quantizer is only as
    # stale as the distribution drift — callers still schedule full
    # rebuilds periodically (analysis/index.py), matching reference
    # behavior, but between rebuilds queries see fresh rows.

    def _row_assignments(self) -> torch.Tensor:
        """Recover each packed row's cell from cell_off: (N,) int64.
        Cell count comes from cell_off, which may exceed nlist when the
        build clamped k-means k to the training-sample size."""
        counts = (self.cell_off[1:] - self.cell_off[:-1]).long()
        return torch.repeat_interleave(
            torch.arange(counts.shape[0], device=self.device), counts)

    def _repack(self, assign: torch.Tensor, unit: torch.Tensor,
                raw_f32: Optional[torch.Tensor], ids: torch.Tensor) -> None:
        """Rebuild packed arrays from per-row assignments (stable order)."""
        ncells = int(self.cell_off.shape[0]) - 1
        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=ncells)
        cell_off = torch.zeros(ncells + 1, dtype=torch.int32,
                               device=self.device)
        cell_off[1:] = torch.cumsum(counts, dim=0).to(torch.int32)
        enc = encode_vectors(unit[order], self.storage)
        n = enc.shape[0]
        if self.dim_pad != self.dim:
            pad = torch.zeros(n, self.dim_pad - self.dim, dtype=enc.dtype,
                              device=self.device)
            enc = torch.cat([enc, pad], dim=1)
        self.data = enc.contiguous()
        self.row_norm = enc.float().norm(dim=1).contiguous()
        self.cell_off = cell_off.contiguous()
        self.ids = ids[order].contiguous()
        self.vectors_f32 = (None if raw_f32 is None
                            else raw_f32[order].contiguous())
        self._rebuild_id_map()
        self.layout_version = next(_LAYOUT_VERSIONS)

    def add(self, vectors: torch.Tensor, ids: torch.Tensor) -> None:
        """Fold new vectors into the packed cells without re-training the
        coarse quantizer. An id already present is replaced (upsert)."""
        if self.centroids is None:
            raise RuntimeError("add() requires a built index")
        vectors = torch.as_tensor(vectors, dtype=torch.float32).to(self.device)
        if vectors.dim() == 1:
            vectors = vectors.unsqueeze(0)
        new_ids = torch.as_tensor(ids, dtype=torch.int64).to(self.device)
        dup = [self.id_to_row[i] for i in new_ids.tolist() if i in self.id_to_row]
        if dup:
            self._drop_rows(torch.tensor(dup, dtype=torch.int64,
                                         device=self.device))
        if self.metric == "angular":
            unit_new = vectors / vectors.norm(dim=1, keepdim=True).clamp(min=1e-12)
        else:
            unit_new = vectors
        assign_new = assign_to_centroids(unit_new, self.centroids)

        old_unit = self._decode_unit()
        assign = torch.cat([self._row_assignments(), assign_new.long()])
        unit = torch.cat([old_unit, unit_new])
        raw = (torch.cat([self.vectors_f32, vectors])
               if self.vectors_f32 is not None else None)
        self._repack(assign, unit, raw, torch.cat([self.ids, new_ids]))

    def retrain(self, nlist: Optional[int] = None, seed: int = 0) -> None:
        """In-place coarse-quantizer retrain from the RESIDENT rows —
        no store round trip. Incremental add/remove splices keep the
        OLD centroids; once the distribution has drifted, this re-runs
        the k-means (+ oversized-cell split) on the decoded vectors and
        repacks, keeping ids. i8 re-encode of decoded rows is exact
        (round(round(v*127)/127*127) == round(v*127))."""
        if self.centroids is None:
            raise RuntimeError("retrain() requires a built index")
        src = (self.vectors_f32 if self.vectors_f32 is not None
               else self._decode_unit())
        fresh = IVFIndex.build(
            src, ids=self.ids, metric=self.metric, storage=self.storage,
            nlist=nlist, device=self.device, seed=seed,
            keep_f32=self.vectors_f32 is not None)
        # fresh carries its own (new, unique) layout_version
        self.__dict__.update(fresh.__dict__)

    def remove(self, ids: torch.Tensor) -> int:
        """Drop rows by id; returns how many were present and removed."""
        rows = [self.id_to_row[i] for i in
                torch.as_tensor(ids, dtype=torch.int64).tolist()
                if i in self.id_to_row]
        if rows:
            self._drop_rows(torch.tensor(sorted(rows), dtype=torch.int64,
                                         device=self.device))
        return len(rows)

    def _drop_rows(self, rows: torch.Tensor) -> None:
        keep = torch.ones(self.n, dtype=torch.bool, device=self.device)
        keep[rows] = False
        assign = self._row_assignments()[keep]
        unit = self._decode_unit()[keep]
        raw = self.vectors_f32[keep] if self.vectors_f32 is not None else None
        self._repack(assign, unit, raw, self.ids[keep])

    def _decode_unit(self) -> torch.Tensor:
        """Packed rows back to the encoded-domain f32 unit vectors."""
        if self.vectors_f32 is not None:
            v = self.vectors_f32
            if self.metric == "angular":
                return v / v.norm(dim=1, keepdim=True).clamp(min=1e-12)
            return v.float()
        v = self.data[:, : self.dim].float()
        return v / 127.0 if self.storage == "i8" else v

    def max_distance(self, q: torch.Tensor,
                     scope: Optional[RowScope] = None) -> Tuple[float, int]:
        """Distance to the FARTHEST row and its id (reference:
        PagedIvfIndex.get_max_distance via ivf_manager.py:1177 — the UI
        normalizes its similarity sliders with this). One full pass over
        the decoded rows; callers cache per item. Under a scope only the
        allowed rows are decoded and ranked; an empty scope gives
        (0.0, -1)."""
        if scope is not None:
            return self._max_distance_scoped(q, scope)
        x = self._decode_unit()
        qv = q.flatten().float().to(x.device)
        if self.metric == "angular":
            qv = qv / qv.norm().clamp(min=1e-12)
            d = 1.0 - x @ qv
        elif self.metric == "dot":
            d = -(x @ qv)
        else:
            d = (x - qv[None, :]).square().sum(dim=1)
        row = int(d.argmax())
        return float(d[row]), int(self.ids[row])

    def _max_distance_scoped(self, q: torch.Tensor,
                             scope: RowScope) -> Tuple[float, int]:
        self._check_scope(scope)
        if scope.n == 0:
            return 0.0, -1
        rows = scope.rows.long()
        if self.vectors_f32 is not None:
            x = self.vectors_f32[rows].float()
            if self.metric == "angular":
                x = x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)
        else:
            x = self.data[rows, : self.dim].float()
            if self.storage == "i8":
                x = x / 127.0
        qv = q.flatten().float().to(x.device)
        if self.metric == "angular":
            qv = qv / qv.norm().clamp(min=1e-12)
            d = 1.0 - x @ qv
        elif self.metric == "dot":
            d = -(x @ qv)
        else:  # same (squared) value the unscoped branch reports
            d = (x - qv[None, :]).square().sum(dim=1)
        j = int(d.argmax())
        return float(d[j]), int(self.ids[rows[j]])

    # -- row scopes ---------------------------------------------------------

    def make_scope(self, ids: Union[torch.Tensor, Iterable[int]]) -> RowScope:
        """Row selection for the given index ids. Unknown ids are ignored,
        duplicates collapse. The result is tied to the current packed
        layout: after add/remove/retrain it must be rebuilt."""
        if not torch.is_tensor(ids):
            ids = torch.as_tensor(list(ids), dtype=torch.int64)
        ids = ids.to(device=self.device, dtype=torch.int64).flatten()
        mask = torch.isin(self.ids, ids)                      # (N,) packed order
        rows = mask.nonzero(as_tuple=True)[0].to(torch.int32)
        prefix = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
        prefix[1:] = torch.cumsum(mask, dim=0)
        off = prefix[self.cell_off.long()].to(torch.int32)
        return RowScope(rows=rows.contiguous(), off=off.contiguous(),
                        n=int(rows.shape[0]), version=self.layout_version)

    def _check_scope(self, scope: RowScope) -> None:
        if scope.version != self.layout_version:
            raise ValueError(
                "stale RowScope: the packed layout changed since it was "
                "built (add/remove/retrain/reload); call make_scope again")

    @property
    def n(self) -> int:
        return 0 if self.ids is None else int(self.ids.shape[0])

    @property
    def nlist(self) -> int:
        return 0 if self.centroids is None else int(self.centroids.shape[0])

    def vector_for_id(self, item_id: int) -> Optional[torch.Tensor]:
        row = self.id_to_row.get(int(item_id))
        if row is None:
            return None
        if self.vectors_f32 is not None:
            return self.vectors_f32[row]
        v = self.data[row, : self.dim].float()
        return v / 127.0 if self.storage == "i8" else v

    # -- query ------------------------------------------------------------

    def _prepare_queries(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns (encoded-domain query, encoded-domain query norm)."""
        q = torch.as_tensor(q, dtype=torch.float32).to(self.device)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if self.metric == "angular":
            q = q / q.norm(dim=1, keepdim=True).clamp(min=1e-12)
        if self.storage == "i8":
            qe = torch.clamp(torch.round(q * 127.0), -127, 127)
            if self.dim_pad != self.dim:
                qe = torch.cat([qe, torch.zeros(q.shape[0], self.dim_pad - self.dim,
                                                device=self.device)], dim=1)
            return qe, qe.norm(dim=1)
        return q, q.norm(dim=1)

    def _rank_cells(self, q_enc: torch.Tensor, nprobe: int,
                    scope: Optional[RowScope] = None,
                    cell_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Top-nprobe cells by centroid score (paged_ivf.py:931-948).
        q_enc is in the encoded domain; centroids are f32 — for ranking we
        use the f32 query direction (scale-invariant for angular/dot).
        Under a scope, cells without an allowed row score +inf, so nprobe
        is spent on cells that can contribute; cell_mask (Q, ncells) bool
        does the same per query (_label_cell_mask)."""
        cen = self.centroids
        q = q_enc.float()
        if self.dim_pad != self.dim:
            q = q[:, : self.dim]
        if self.metric == "euclidean":
            scores = torch.cdist(q, cen)
        elif self.metric == "dot":
            scores = -(q @ cen.T)
        else:
            cn = cen / cen.norm(dim=1, keepdim=True).clamp(min=1e-12)
            qn = q / q.norm(dim=1, keepdim=True).clamp(min=1e-12)
            scores = 1.0 - (qn @ cn.T)
        if scope is not None:
            empty = (scope.off[1:] == scope.off[:-1])[: scores.shape[1]]
            scores = scores.masked_fill(empty.unsqueeze(0), float("inf"))
        if cell_mask is not None:
            scores = scores.masked_fill(cell_mask[:, : scores.shape[1]],
                                        float("inf"))
        nprobe = min(nprobe, self.nlist)
        return torch.topk(scores, nprobe, dim=1, largest=False).indices.to(torch.int32)

    def scan(self, q: torch.Tensor, nprobe: Optional[int] = None,
             scope: Optional[RowScope] = None,
             _cell_mask: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Scan probed cells. Returns (dist (Q, cap) f32 with +inf padding,
        row (Q, cap) int32). With a scope only its rows are scanned and
        cap follows the allowed per-cell counts."""
        nprobe = min(nprobe or C.IVF_NPROBE, self.nlist)
        q_enc, q_norm = self._prepare_queries(q)
        if scope is not None:
            self._check_scope(scope)
            if scope.n == 0:
                Q = q_enc.shape[0]
                return (torch.empty(Q, 0, device=self.device),
                        torch.empty(Q, 0, dtype=torch.int32,
                                    device=self.device))
        probe = self._rank_cells(q_enc, nprobe, scope, _cell_mask)  # (Q, P)
        Q, P = probe.shape

        off = self.cell_off if scope is None else scope.off
        counts = (off[1:] - off[:-1]).to(torch.int64)
        probed_counts = counts[probe.long()]                  # (Q, P)
        cand_off = torch.zeros(Q, P, dtype=torch.int64, device=self.device)
        cand_off[:, 1:] = torch.cumsum(probed_counts, dim=1)[:, :-1]
        totals = probed_counts.sum(dim=1)
        cap = int(totals.max().item()) if Q else 0
        if cap == 0:
            return (torch.empty(Q, 0, device=self.device),
                    torch.empty(Q, 0, dtype=torch.int32, device=self.device))

        out_dist = torch.full((Q, cap), float("inf"), device=self.device)
        out_row = torch.full((Q, cap), -1, dtype=torch.int32, device=self.device)

        if self.device.type == "cuda":
            ext = _ext.native_or_none()
            if ext is not None:
                qt = (q_enc.to(torch.int8).view(torch.int32)
                      if self.storage == "i8" else q_enc.contiguous())
                if scope is not None:
                    ext.ivf_scan_sel(
                        _DTYPE_CODE[self.storage], _METRIC_CODE[self.metric],
                        qt.contiguous(), q_norm.contiguous(),
                        self.data.view(torch.int32) if self.storage == "i8"
                        else self.data,
                        self.row_norm, probe.contiguous(),
                        scope.rows, scope.off, cand_off.contiguous(),
                        out_dist, out_row, self.dim_pad)
                    return out_dist, out_row
                ext.ivf_scan(_DTYPE_CODE[self.storage], _METRIC_CODE[self.metric],
                             qt.contiguous(), q_norm.contiguous(),
                             self.data.view(torch.int32) if self.storage == "i8"
                             else self.data,
                             self.row_norm, probe.contiguous(),
                             self.cell_off, cand_off.contiguous(),
                             out_dist, out_row, self.dim_pad)
                return out_dist, out_row
        self._scan_fallback(q_enc, q_norm, probe, cand_off, out_dist, out_row,
                            scope=scope)
        return out_dist, out_row

    def _scan_fallback(self, q_enc, q_norm, probe, cand_off, out_dist, out_row,
                       scope: Optional[RowScope] = None):
        """Vectorized torch scan with identical math (golden reference).
        Under a scope the slots of a probed cell hold its allowed rows in
        ascending order, as in the native kernel."""
        Q, P = probe.shape
        off = self.cell_off.long() if scope is None else scope.off.long()
        for qi in range(Q):
            rows = torch.cat([torch.arange(int(off[c]), int(off[c + 1]),
                                           device=self.device)
                              for c in probe[qi].tolist()])
            if rows.numel() == 0:
                continue
            if scope is not None:
                rows = scope.rows[rows].long()
            v = self.data[rows].float()
            qv = q_enc[qi].float()
            if self.metric == "angular":
                dot = v @ qv
                denom = q_norm[qi] * self.row_norm[rows] + 1e-12
                d = 1.0 - torch.clamp(dot / denom, -1.0, 1.0)
            elif self.metric == "euclidean":
                d = (v - qv).square().sum(dim=1).sqrt()
            else:
                d = -(v @ qv)
            out_dist[qi, : rows.numel()] = d
            out_row[qi, : rows.numel()] = rows.to(torch.int32)

    def query(self, q: torch.Tensor, k: int, nprobe: Optional[int] = None,
              rerank: bool = True, scope: Optional[RowScope] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns (dists (Q, k) f32, ids (Q, k) int64; missing slots id=-1).
        scope: restrict the search to a RowScope's rows (applied inside
        the scan, before any top-k).

        rerank: over-fetch IVF_RERANK_OVERFETCH*k candidates from the
        quantized scan, then exact-f32 re-score (ivf_manager.py:889-933).
        """
        single = torch.as_tensor(q).dim() == 1
        dist, row = self.scan(q, nprobe=nprobe, scope=scope)
        do_rerank = rerank and self.vectors_f32 is not None
        fetch = min(dist.shape[1], k * (C.IVF_RERANK_OVERFETCH if do_rerank else 1))
        fetch = max(fetch, min(k, dist.shape[1]))
        top = torch.topk(dist, fetch, dim=1, largest=False)
        rows = row.gather(1, top.indices.clamp(min=0)).long()   # (Q, fetch)
        dists = top.values
        return self._rerank_select(q, dists, rows, k, do_rerank, single)

    def _rerank_select(self, q: torch.Tensor, dists: torch.Tensor,
                       rows: torch.Tensor, k: int, do_rerank: bool,
                       single: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """Shared tail of query() and query_topk(): optional exact-f32
        re-score of the fetched candidates (dists (Q, fetch) scan distances
        with +inf padding, rows (Q, fetch) int64 packed rows), final top-k,
        row -> id, padding to k."""
        Q = dists.shape[0]
        valid = torch.isfinite(dists)

        if do_rerank:
            qf = torch.as_tensor(q, dtype=torch.float32).to(self.device)
            if qf.dim() == 1:
                qf = qf.unsqueeze(0)
            cand = self.vectors_f32[rows.clamp(min=0)]           # (Q, fetch, dim)
            if self.metric == "angular":
                cn = cand / cand.norm(dim=2, keepdim=True).clamp(min=1e-12)
                qn = (qf / qf.norm(dim=1, keepdim=True).clamp(min=1e-12)).unsqueeze(2)
                dists = 1.0 - torch.clamp(torch.bmm(cn, qn).squeeze(2), -1.0, 1.0)
            elif self.metric == "euclidean":
                dists = (cand - qf.unsqueeze(1)).square().sum(dim=2).sqrt()
            else:
                dists = -torch.bmm(cand, qf.unsqueeze(2)).squeeze(2)
            dists = torch.where(valid, dists, torch.full_like(dists, float("inf")))

        kk = min(k, dists.shape[1])
        final = torch.topk(dists, kk, dim=1, largest=False)
        frows = rows.gather(1, final.indices)
        fids = self.ids[frows.clamp(min=0)]
        fvalid = torch.isfinite(final.values)
        fids = torch.where(fvalid, fids, torch.full_like(fids, -1))
        out_d = final.values
        if kk < k:  # pad
            pad_d = torch.full((Q, k - kk), float("inf"), device=self.device)
            pad_i = torch.full((Q, k - kk), -1, dtype=torch.int64, device=self.device)
            out_d = torch.cat([out_d, pad_d], dim=1)
            fids = torch.cat([fids, pad_i], dim=1)
        if single:
            return out_d[0], fids[0]
        return out_d, fids

    # -- batch top-k: selection inside the scan ----------------------------

    @staticmethod
    def _ordered_select(dist: torch.Tensor, row: torch.Tensor, kk: int
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
        """First kk of each row of (dist, row) in ascending (distance, row)
        order, padded with +inf / -1: a stable sort by row, then a stable
        sort by distance."""
        Q, cap = dist.shape
        row = torch.where(torch.isfinite(dist), row, torch.full_like(row, -1))
        by_row = torch.sort(row, dim=1, stable=True)
        dist = dist.gather(1, by_row.indices)
        by_dist = torch.sort(dist, dim=1, stable=True)
        dist = by_dist.values[:, :kk]
        row = by_row.values.gather(1, by_dist.indices)[:, :kk]
        if cap < kk:
            dist = torch.cat([dist, dist.new_full((Q, kk - cap),
                                                  float("inf"))], dim=1)
            row = torch.cat([row, row.new_full((Q, kk - cap), -1)], dim=1)
        return dist.contiguous(), row.contiguous()

    def _topk_splits(self, Q: int, P: int) -> int:
        """Probe-list splits per query for the fused scan: one workgroup
        per query when the batch alone fills the device (the self-join),
        otherwise enough splits for about eight workgroups per CU (what
        fits at once; at 64 queries anything from 4 splits up ran alike,
        profiles/r5_knn_graph.txt)."""
        cus = torch.cuda.get_device_properties(
            self.device).multi_processor_count
        return max(1, min(P, -(-8 * cus // max(Q, 1))))

    def _label_cell_mask(self, row_labels: torch.Tensor,
                         q_labels: torch.Tensor) -> torch.Tensor:
        """(Q, ncells) bool: cell c holds nothing for query q because all
        its rows carry q's label (an empty cell holds nothing for any
        labelled query). One pass over the rows gives each cell its "pure
        label" (the label all its rows share, -1 when they differ); the
        mask is one comparison against it. A negative q_label masks
        nothing."""
        ncells = int(self.cell_off.shape[0]) - 1
        cells = self._row_assignments()
        big = torch.iinfo(torch.int32).max
        lo = torch.full((ncells,), big, dtype=torch.int32,
                        device=self.device).scatter_reduce(
            0, cells, row_labels, "amin", include_self=True)
        hi = torch.full((ncells,), -big - 1, dtype=torch.int32,
                        device=self.device).scatter_reduce(
            0, cells, row_labels, "amax", include_self=True)
        pure = torch.where(lo == hi, lo, torch.full_like(lo, -1))
        empty = (self.cell_off[1:] == self.cell_off[:-1]).unsqueeze(0)
        ql = q_labels.unsqueeze(1)
        return ((ql == pure.unsqueeze(0)) | empty) & (ql >= 0)

    def scan_topk(self, q: torch.Tensor, kk: int,
                  nprobe: Optional[int] = None,
                  scope: Optional[RowScope] = None,
                  skip_rows: Optional[torch.Tensor] = None,
                  row_labels: Optional[torch.Tensor] = None,
                  q_labels: Optional[torch.Tensor] = None,
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The kk best candidates of scan(), selected while scanning.
        Returns (dist (Q, kk) f32, row (Q, kk) int32), each row ascending
        by (distance, row), padded with +inf / -1. skip_rows (Q,) names one
        packed row per query that is never reported (-1: none).

        row_labels (N,) in packed order and q_labels (Q,), given together:
        query q is never given a row r with row_labels[r] == q_labels[q]
        (a negative q_label excludes nothing), and cells whose rows all
        carry q's label are ranked last, so nprobe is spent on cells that
        can contribute. Labels do not combine with a scope (ValueError).

        On the GPU this is one launch of the fused scan + top-K kernel
        (ops/csrc/distance.hip) and a merge of its per-split lists; the
        host allocates O(Q * S * kk), never the (Q, cap) candidate buffer.
        CPU hosts, and kk beyond the kernel's TOPK_KMAX, take scan() and the
        same ordered selection (the kernel's golden reference)."""
        kk = int(kk)
        if kk < 1:
            raise ValueError("kk must be >= 1")
        skip = None
        if skip_rows is not None:
            skip = torch.as_tensor(skip_rows).to(
                device=self.device, dtype=torch.int32).flatten().contiguous()
        if (row_labels is None) != (q_labels is None):
            raise ValueError("row_labels and q_labels go together")
        rl = ql = cell_mask = None
        if row_labels is not None:
            if scope is not None:
                raise ValueError("labels do not combine with a scope")
            rl = torch.as_tensor(row_labels).to(
                device=self.device, dtype=torch.int32).flatten().contiguous()
            ql = torch.as_tensor(q_labels).to(
                device=self.device, dtype=torch.int32).flatten().contiguous()
            nq = 1 if torch.as_tensor(q).dim() == 1 else len(q)
            if rl.numel() != self.n or ql.numel() != nq:
                raise ValueError("row_labels must hold one label per packed "
                                 "row, q_labels one per query")
            if nq:
                cell_mask = self._label_cell_mask(rl, ql)
        ext = (_ext.native_or_none() if self.device.type == "cuda" else None)
        if ext is None or kk > TOPK_KMAX:
            dist, row = self.scan(q, nprobe=nprobe, scope=scope,
                                  _cell_mask=cell_mask)
            if skip is not None and dist.shape[1]:
                dist = dist.masked_fill(row == skip.unsqueeze(1), float("inf"))
            if rl is not None and dist.shape[1]:
                same = rl[row.clamp(min=0).long()] == ql.unsqueeze(1)
                dist = dist.masked_fill(same & (ql >= 0).unsqueeze(1),
                                        float("inf"))
            return self._ordered_select(dist, row, kk)

        nprobe = min(nprobe or C.IVF_NPROBE, self.nlist)
        q_enc, q_norm = self._prepare_queries(q)
        Q = q_enc.shape[0]
        if skip is not None and skip.numel() != Q:
            raise ValueError("skip_rows must hold one row per query")
        if scope is not None:
            self._check_scope(scope)
        if Q == 0 or (scope is not None and scope.n == 0):
            return (torch.full((Q, kk), float("inf"), device=self.device),
                    torch.full((Q, kk), -1, dtype=torch.int32,
                               device=self.device))
        probe = self._rank_cells(q_enc, nprobe, scope, cell_mask).contiguous()
        qt = (q_enc.to(torch.int8).view(torch.int32)
              if self.storage == "i8" else q_enc).contiguous()
        data = self.data.view(torch.int32) if self.storage == "i8" else self.data
        q_norm = q_norm.contiguous()
        S = self._topk_splits(Q, probe.shape[1])
        out_d, out_r = [], []
        for a in range(0, Q, _TOPK_MAX_Q):      # grid.y limit of one launch
            b = min(a + _TOPK_MAX_Q, Q)
            dist = torch.empty(b - a, S, kk, device=self.device)
            row = torch.empty(b - a, S, kk, dtype=torch.int32,
                              device=self.device)
            if rl is not None:
                ext.ivf_scan_topk_excl(
                    _DTYPE_CODE[self.storage], _METRIC_CODE[self.metric],
                    qt[a:b], q_norm[a:b], data, self.row_norm, probe[a:b],
                    self.cell_off, None if skip is None else skip[a:b],
                    rl, ql[a:b], dist, row, self.dim_pad)
            else:
                ext.ivf_scan_topk(
                    _DTYPE_CODE[self.storage], _METRIC_CODE[self.metric],
                    qt[a:b], q_norm[a:b], data, self.row_norm, probe[a:b],
                    self.cell_off,
                    None if scope is None else scope.rows,
                    None if scope is None else scope.off,
                    None if skip is None else skip[a:b],
                    dist, row, self.dim_pad)
            if S == 1:
                d, r = dist[:, 0], row[:, 0]
            else:
                d, r = self._ordered_select(dist.view(b - a, S * kk),
                                            row.view(b - a, S * kk), kk)
            out_d.append(d)
            out_r.append(r)
        if len(out_d) == 1:
            return out_d[0], out_r[0]
        return torch.cat(out_d), torch.cat(out_r)

    def query_topk(self, q: torch.Tensor, k: int, nprobe: Optional[int] = None,
                   rerank: bool = True, scope: Optional[RowScope] = None,
                   skip_rows: Optional[torch.Tensor] = None,
                   row_labels: Optional[torch.Tensor] = None,
                   q_labels: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Batch form of query() on top of scan_topk(): same return
        contract ((Q, k) dists and int64 ids, -1 / +inf padding, 1-D query
        gives 1-D results), no (Q, cap) candidate buffer. skip_rows: one
        packed row per query that is never returned. row_labels / q_labels:
        the label exclusion of scan_topk()."""
        single = torch.as_tensor(q).dim() == 1
        do_rerank = rerank and self.vectors_f32 is not None
        fetch = k * (C.IVF_RERANK_OVERFETCH if do_rerank else 1)
        dists, rows = self.scan_topk(q, fetch, nprobe=nprobe, scope=scope,
                                     skip_rows=skip_rows,
                                     row_labels=row_labels, q_labels=q_labels)
        return self._rerank_select(q, dists, rows.long(), k, do_rerank, single)

    def knn_graph(self, k: int, nprobe: Optional[int] = None,
                  chunk: int = 8192, rerank: bool = True
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Approximate k nearest neighbours of every row, from the index
        itself. Returns (dists (N, k) f32, ids (N, k) int64) in PACKED
        order: line r describes packed row r (id self.ids[r]) and never
        holds that id; missing neighbours are -1 / +inf. Queries go
        through query_topk() chunk packed rows at a time, so consecutive
        queries share their probe lists and re-read cell data from cache."""
        nprobe = nprobe or C.IVF_GRAPH_NPROBE
        n = self.n
        dists = torch.empty(n, k, device=self.device)
        ids = torch.empty(n, k, dtype=torch.int64, device=self.device)
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            if self.vectors_f32 is not None:
                qv = self.vectors_f32[a:b]
            else:
                qv = decode_vectors(self.data[a:b, : self.dim], self.storage)
            rows = torch.arange(a, b, dtype=torch.int32, device=self.device)
            dists[a:b], ids[a:b] = self.query_topk(
                qv, k, nprobe=nprobe, rerank=rerank, skip_rows=rows)
        return dists, ids

    def foreign_neighbours(self, labels: torch.Tensor, m: int,
                           rows: Optional[torch.Tensor] = None,
                           nprobe: Optional[int] = None, chunk: int = 8192
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The m nearest rows that carry another label, for each packed
        row in `rows` (all rows when None): (dists (R, m) f32, ids (R, m)
        int64), padded with +inf / -1. labels (N,) holds one non-negative
        label per packed row. Rows go through query_topk() chunk at a time
        like knn_graph(), with the label exclusion inside the scan, so the
        distances are the re-ranked f32 ones knn_graph() reports."""
        nprobe = nprobe or C.IVF_GRAPH_NPROBE
        labels = torch.as_tensor(labels).to(
            device=self.device, dtype=torch.int32).flatten().contiguous()
        if labels.numel() != self.n:
            raise ValueError("labels must hold one label per packed row")
        if rows is None:
            rows = torch.arange(self.n, device=self.device)
        rows = torch.as_tensor(rows).to(device=self.device,
                                        dtype=torch.int64).flatten()
        R = rows.numel()
        if R and (int(rows.min()) < 0 or int(rows.max()) >= self.n):
            raise ValueError("rows must be packed rows in [0, n)")
        dists = torch.full((R, m), float("inf"), device=self.device)
        ids = torch.full((R, m), -1, dtype=torch.int64, device=self.device)
        for a in range(0, R, chunk):
            r = rows[a:a + chunk]
            if self.vectors_f32 is not None:
                qv = self.vectors_f32[r]
            else:
                qv = decode_vectors(self.data[r, : self.dim], self.storage)
            dists[a:a + chunk], ids[a:a + chunk] = self.query_topk(
                qv, m, nprobe=nprobe, skip_rows=r.to(torch.int32),
                row_labels=labels, q_labels=labels[r])
        return dists, ids

    # -- persistence ------------------------------------------------------

    def serialize(self) -> bytes:
        state = {
            "dim": self.dim, "metric": self.metric, "storage": self.storage,
            "centroids": self.centroids.cpu(), "data": self.data.cpu(),
            "row_norm": self.row_norm.cpu(), "cell_off": self.cell_off.cpu(),
            "ids": self.ids.cpu(),
            "vectors_f32": None if self.vectors_f32 is None else self.vectors_f32.cpu(),
        }
        buf = io.BytesIO()
        torch.save(state, buf)
        return buf.getvalue()

    @classmethod
    def deserialize(cls, blob: bytes, device: str | torch.device = "cpu") -> "IVFIndex":
        state = torch.load(io.BytesIO(blob), map_location="cpu", weights_only=True)
        idx = cls(state["dim"], metric=state["metric"], storage=state["storage"],
                  device=device)
        for name in ("centroids", "data", "row_norm", "cell_off", "ids"):
            setattr(idx, name, state[name].to(idx.device))
        if state["vectors_f32"] is not None:
            idx.vectors_f32 = state["vectors_f32"].to(idx.device)
        idx._rebuild_id_map()
        idx.layout_version = next(_LAYOUT_VERSIONS)
        return idx
