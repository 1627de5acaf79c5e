"""Song path: interpolated journey between two songs.

Reference: /root/reference/tasks/path_manager.py (707 LoC;
docs/ALGORITHM.md:1363-1365) — linear or slerp interpolation between the
endpoint vectors produces k waypoint centroids; each waypoint is
resolved to its nearest unused track (dedupe + artist caps); adjacent
duplicates merge. That is the "waypoint" engine.

The "graph" engine (config.PATH_ENGINE, or engine= per request) is an
MI355X-native extra: the journey is a shortest path over the resident
kNN graph (SimilarityEngine.path_graph, engines/graph_path.py), so every
step is a true nearest-neighbour hop; all legs of a request (start, via
stops, end) are solved in one batch.
"""

from __future__ import annotations

import logging
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from audiomuse_amd.engines.graph_path import MAX_LEGS, shortest_paths, thin
from audiomuse_amd.engines.similarity import SimilarityEngine

log = logging.getLogger(__name__)

PATH_ENGINES = ("waypoint", "graph")
_fallback_logged = False


def interpolate(a: np.ndarray, b: np.ndarray, k: int,
                mode: str = "slerp") -> np.ndarray:
    """k interior waypoints between unit vectors a and b (k, d)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    an = a / (np.linalg.norm(a) + 1e-12)
    bn = b / (np.linalg.norm(b) + 1e-12)
    ts = np.linspace(0.0, 1.0, k + 2)[1:-1]
    if mode == "linear":
        pts = np.stack([(1 - t) * an + t * bn for t in ts])
    else:
        cos = float(np.clip(np.dot(an, bn), -1.0, 1.0))
        omega = math.acos(cos)
        if omega < 1e-6:
            pts = np.stack([an for _ in ts])
        else:
            so = math.sin(omega)
            pts = np.stack([
                (math.sin((1 - t) * omega) / so) * an
                + (math.sin(t * omega) / so) * bn for t in ts])
    pts /= np.linalg.norm(pts, axis=1, keepdims=True) + 1e-12
    return pts.astype(np.float32)


def _backfill(sim: SimilarityEngine, path: List[Dict], used: set,
              length: int, mode: str, scope: Optional[str] = None) -> None:
    """PATH_FIX_SIZE: the path came out short (starved waypoints, or a
    graph path with fewer hops than asked) — backfill in place by
    re-querying the midpoints of the gaps until `length` is met
    (reference: merge-on-starve keeps the playlist size fixed)."""
    guard = 0
    while len(path) < length and guard < length * 2:
        guard += 1
        grew = False
        for i in range(len(path) - 1):
            a = sim.vector_for_id(path[i]["item_id"])
            b = sim.vector_for_id(path[i + 1]["item_id"])
            if a is None or b is None:
                continue
            mid = interpolate(a.cpu().numpy(), b.cpu().numpy(), 1,
                              mode=mode)[0]
            cands = sim.find_similar_by_vector(
                torch.from_numpy(mid), 5, exclude=tuple(used), scope=scope)
            if cands:
                used.add(cands[0]["item_id"])
                path.insert(i + 1, cands[0])
                grew = True
                if len(path) >= length:
                    break
        if not grew:
            break


def _waypoint_leg(sim: SimilarityEngine, start_id: str, end_id: str,
                  length: int, mode: str, max_per_artist: Optional[int],
                  scope: Optional[str], used: set,
                  artist_counts: Dict[str, int]) -> List[Dict]:
    """The waypoint routine for one leg: `length` - 2 interpolated
    waypoints, each snapped to its nearest unused track; backfilled to
    `length` under PATH_FIX_SIZE. `used` and `artist_counts` carry over
    from leg to leg."""
    from audiomuse_amd import config as C
    va = sim.vector_for_id(start_id)
    vb = sim.vector_for_id(end_id)
    k = max(0, length - 2)
    waypoints = interpolate(va.cpu().numpy(), vb.cpu().numpy(), k, mode=mode)
    path = [{"item_id": start_id, "distance": 0.0}]
    for wp in waypoints:
        cands = sim.find_similar_by_vector(
            torch.from_numpy(wp), 10, exclude=tuple(used), scope=scope)
        picked = None
        for c in cands:
            meta = sim.meta_fn(c["item_id"]) or {}
            author = (meta.get("author") or "").strip().lower()
            if max_per_artist and author and \
                    artist_counts.get(author, 0) >= max_per_artist:
                continue
            picked = c
            if author:
                artist_counts[author] = artist_counts.get(author, 0) + 1
            break
        if picked is None:
            continue  # waypoint merges into its neighbor
        used.add(picked["item_id"])
        path.append(picked)
    path.append({"item_id": end_id, "distance": 0.0})
    if C.PATH_FIX_SIZE:
        _backfill(sim, path, used, length, mode, scope)
    return path


def _step_distances(sim: SimilarityEngine, ids: Sequence[str]) -> List[Dict]:
    """{"item_id", "distance"} per track; distance is the index metric's
    distance to the previous track from the stored f32 vectors (0.0 for
    the first)."""
    out: List[Dict] = []
    prev = None
    metric = sim.index.metric
    for iid in ids:
        v = sim.vector_for_id(iid).float()
        if prev is None:
            d = 0.0
        elif metric == "angular":
            cos = torch.dot(prev, v) / (prev.norm() * v.norm()).clamp(min=1e-12)
            d = 1.0 - float(cos.clamp(-1.0, 1.0))
        elif metric == "euclidean":
            d = float((prev - v).norm())
        else:
            d = -float(torch.dot(prev, v))
        out.append({"item_id": iid, "distance": d})
        prev = v
    return out


def _waypoint_path(sim: SimilarityEngine, stops: List[str], length: int,
                   mode: str, max_per_artist: Optional[int],
                   scope: Optional[str]) -> List[Dict]:
    used = set(stops)
    artist_counts: Dict[str, int] = {}
    legs = len(stops) - 1
    if legs == 1:
        return _waypoint_leg(sim, stops[0], stops[1], length, mode,
                             max_per_artist, scope, used, artist_counts)
    per_leg = -(-(length + legs - 1) // legs)
    ids = [stops[0]]
    for a, b in zip(stops[:-1], stops[1:]):
        leg = _waypoint_leg(sim, a, b, per_leg, mode, max_per_artist, scope,
                            used, artist_counts)
        ids.extend(p["item_id"] for p in leg[1:] if p["item_id"] not in ids)
    return _step_distances(sim, thin(ids, stops, length))


def _graph_path(sim: SimilarityEngine, stops: List[str], length: int,
                mode: str, max_per_artist: Optional[int],
                scope: Optional[str]) -> Optional[List[Dict]]:
    """The graph engine; None when there is no graph (dot metric) or a
    leg has no path, and the request falls back to the waypoint engine."""
    from audiomuse_amd import config as C
    graph = sim.path_graph()
    if graph is None:
        return None
    allowed = sim.scope_mask(scope) if scope is not None else None
    pos = [sim.pos[s] for s in stops]
    paths, _dists, _sweeps = shortest_paths(graph, pos[:-1], pos[1:],
                                            allowed=allowed)
    if any(p is None for p in paths):
        return None
    ids = [stops[0]]
    used = set(stops)
    artist_counts: Dict[str, int] = {}
    for leg, junction in zip(paths, stops[1:]):
        for p in leg[1:-1]:
            iid = sim.item_ids[p]
            if iid in used:
                continue
            author = ((sim.meta_fn(iid) or {}).get("author") or ""
                      ).strip().lower()
            if max_per_artist and author:
                if artist_counts.get(author, 0) >= max_per_artist:
                    continue
                artist_counts[author] = artist_counts.get(author, 0) + 1
            used.add(iid)
            ids.append(iid)
        if junction not in ids:
            ids.append(junction)
    if len(ids) > length:
        ids = thin(ids, stops, length)
    elif len(ids) < length and C.PATH_FIX_SIZE:
        path = [{"item_id": i} for i in ids]
        _backfill(sim, path, used, length, mode, scope)
        ids = [p["item_id"] for p in path]
    return _step_distances(sim, ids)


def find_path_ex(sim: SimilarityEngine, start_id: str, end_id: str,
                 length: Optional[int] = None, mode: Optional[str] = None,
                 max_per_artist: Optional[int] = None, *,
                 engine: Optional[str] = None, scope: Optional[str] = None,
                 via: Sequence[str] = ()) -> Tuple[List[Dict], str]:
    """find_path, and the engine that produced the answer: (items,
    "waypoint" | "graph"). A graph request falls back to the waypoint
    engine when a leg has no path over the kNN graph or the index metric
    is dot."""
    global _fallback_logged
    from audiomuse_amd import config as C
    if engine is None:
        engine = C.PATH_ENGINE
    if engine not in PATH_ENGINES:
        raise ValueError(f"path engine must be waypoint or graph, "
                         f"not {engine!r}")
    stops = [start_id, *via, end_id]
    if len(stops) - 1 > MAX_LEGS:
        raise ValueError(f"a path takes at most {MAX_LEGS - 1} via stops")
    if length is None:
        length = C.PATH_DEFAULT_LENGTH
    if mode is None:
        mode = "slerp" if C.PATH_DISTANCE_METRIC == "angular" else "linear"
    if any(sim.vector_for_id(s) is None for s in stops):
        return [], engine
    if scope is not None:
        mask = sim.scope_mask(scope)
        if not all(bool(mask[sim.pos[s]]) for s in stops):
            return [], engine
    if engine == "graph":
        items = _graph_path(sim, stops, length, mode, max_per_artist, scope)
        if items is not None:
            return items, "graph"
        if not _fallback_logged:
            _fallback_logged = True
            log.warning("graph song path: no path over the kNN graph (or dot "
                        "metric); falling back to the waypoint engine")
    return _waypoint_path(sim, stops, length, mode, max_per_artist,
                          scope), "waypoint"


def find_path(sim: SimilarityEngine, start_id: str, end_id: str,
              length: Optional[int] = None, mode: Optional[str] = None,
              max_per_artist: Optional[int] = None, *,
              engine: Optional[str] = None, scope: Optional[str] = None,
              via: Sequence[str] = ()) -> List[Dict]:
    """Path of ~`length` tracks from start to end (path_manager entry).
    Defaults from config: PATH_DEFAULT_LENGTH; interpolation follows
    PATH_DISTANCE_METRIC (angular -> slerp on the unit sphere,
    euclidean/dot -> linear); PATH_FIX_SIZE backfills starved waypoints
    so the playlist comes out at exactly `length` (the reference's
    merge-on-starve behavior).

    engine: "waypoint" or "graph" (None takes config.PATH_ENGINE). scope:
    a scope name of the similarity engine; the path stays on that scope's
    tracks, and endpoints outside it give []. via: stops to pass through,
    in order (at most 8 legs). Under the graph engine, and with via
    stops, "distance" is the distance to the previous returned track."""
    return find_path_ex(sim, start_id, end_id, length, mode, max_per_artist,
                        engine=engine, scope=scope, via=via)[0]
