"""Audio-index query engine.

Reference: /root/reference/tasks/ivf_manager.py — query-side feature
logic over the IVF index: over-fetch + exact-f32 re-rank (inside
IVFIndex.query here), near-duplicate filtering with a lookback window,
mood filtering, per-artist caps, radius-walk mode, multi-query union,
and a small result cache. This engine is shared by similar-song, song
path, alchemy, SemGrove and sonic-fingerprint features.
"""

from __future__ import annotations

import threading
import time
from collections import OrderedDict
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines.radius_walk import execute_radius_walk
from audiomuse_amd.index.ivf import IVFIndex, RowScope


class ResultCache:
    """TTL LRU cache (reference: ivf_manager._ResultCache :73)."""

    def __init__(self, max_items: Optional[int] = None,
                 ttl: Optional[float] = None):
        if max_items is None:
            max_items = C.IVF_RESULT_CACHE_MAX
        if ttl is None:
            ttl = C.IVF_RESULT_CACHE_SECONDS
        self.max_items = max_items
        self.ttl = ttl
        self._data: OrderedDict = OrderedDict()
        self._lock = threading.Lock()

    def get(self, key):
        with self._lock:
            hit = self._data.get(key)
            if hit is None:
                return None
            ts, value = hit
            if time.monotonic() - ts > self.ttl:
                del self._data[key]
                return None
            self._data.move_to_end(key)
            return value

    def put(self, key, value):
        with self._lock:
            self._data[key] = (time.monotonic(), value)
            self._data.move_to_end(key)
            while len(self._data) > self.max_items:
                self._data.popitem(last=False)

    def clear(self):
        with self._lock:
            self._data.clear()


MetaFn = Callable[[str], Optional[Dict]]   # item_id -> {title, author, mood_vector}
ScopeFn = Callable[[str], Iterable[str]]   # scope name -> allowed item_ids


class SimilarityEngine:
    def __init__(self, index: IVFIndex, ids: Sequence[str],
                 meta_fn: Optional[MetaFn] = None,
                 scope_fn: Optional[ScopeFn] = None):
        """index: built IVFIndex whose int64 ids are positions into `ids`
        (the canonical string item_ids). scope_fn maps a scope name (a
        media-server id) to the item_ids that scope may return."""
        self.index = index
        self.item_ids = list(ids)
        self.pos = {s: i for i, s in enumerate(self.item_ids)}
        self.meta_fn = meta_fn or (lambda _id: None)
        self.scope_fn = scope_fn
        self.cache = ResultCache()
        # {name: (built_at, RowScope)} — reference: the availability-mask
        # cache of paged_ivf.py (_AVAILABILITY_CACHE_TTL)
        self._scopes: Dict[str, Tuple[float, RowScope]] = {}
        self._scope_lock = threading.Lock()
        self._time = time.monotonic
        # {name: (built_at, layout_version, (n,) uint8 mask)}: the named
        # scopes again, as masks over positions for the graph song path
        self._scope_masks: Dict[str, Tuple[float, int, torch.Tensor]] = {}
        # (layout_version, PathGraph) of the graph song path
        self._path_graph = None
        self._path_graph_lock = threading.Lock()
        # (layout_version, RankGraph) of the graph radio, and the one kNN
        # build (layout_version, pos, dists) both graphs are made from;
        # all three under _path_graph_lock
        self._rank_graph = None
        self._graph_knn = None
        # (key, CommunityGraph) of the graph communities and {(key, g):
        # (labels, report)} of the solves over it, under the same lock
        self._community_graph = None
        self._communities: Dict = {}
        # ((layout_version, True), pos', dists', report): the kNN build
        # with the bridges of PATH_GRAPH_CONNECT, and ((layout_version,
        # False), report) of the plain build once graph_report() was asked
        self._graph_connected = None
        self._graph_plain_report = None

    # -- named scopes (reference: paged_ivf._availability_mask) ------------

    def _resolve_scope(self, name: Optional[str]
                       ) -> Tuple[Optional[float], Optional[RowScope]]:
        """(build stamp, RowScope) for a scope name; (None, None) for no
        scope. Entries expire after IVF_SCOPE_CACHE_SECONDS and are
        dropped when the index layout has moved under them. The stamp
        goes into the result-cache keys, so answers computed under a
        superseded scope are never served."""
        if name is None:
            return None, None
        if self.scope_fn is None:
            raise ValueError(f"scope {name!r} requested but the engine has "
                             "no scope_fn")
        now = self._time()
        with self._scope_lock:
            hit = self._scopes.get(name)
            if hit is not None:
                ts, sc = hit
                if (now - ts < C.IVF_SCOPE_CACHE_SECONDS
                        and sc.version == self.index.layout_version):
                    return ts, sc
                del self._scopes[name]
        pos = [self.pos[i] for i in self.scope_fn(name) if i in self.pos]
        sc = self.index.make_scope(torch.tensor(pos, dtype=torch.int64))
        with self._scope_lock:
            self._scopes[name] = (now, sc)
        return now, sc

    def invalidate_scopes(self) -> None:
        with self._scope_lock:
            self._scopes.clear()
            self._scope_masks.clear()

    def scope_mask(self, name: str) -> torch.Tensor:
        """(N,) uint8 mask over positions into item_ids for a scope name,
        on the CPU: what the graph song path takes where the index scan
        takes a RowScope. Cached next to the RowScopes, same expiry."""
        if self.scope_fn is None:
            raise ValueError(f"scope {name!r} requested but the engine has "
                             "no scope_fn")
        now = self._time()
        version = self.index.layout_version
        with self._scope_lock:
            hit = self._scope_masks.get(name)
            if hit is not None:
                ts, ver, mask = hit
                if now - ts < C.IVF_SCOPE_CACHE_SECONDS and ver == version:
                    return mask
                del self._scope_masks[name]
        mask = torch.zeros(len(self.item_ids), dtype=torch.uint8)
        pos = [self.pos[i] for i in self.scope_fn(name) if i in self.pos]
        if pos:
            mask[torch.tensor(pos, dtype=torch.int64)] = 1
        with self._scope_lock:
            self._scope_masks[name] = (now, version, mask)
        return mask

    # -- vector resolution (ivf_manager._resolve_neighbor_query_vector) ---

    def vector_for_id(self, item_id: str) -> Optional[torch.Tensor]:
        p = self.pos.get(item_id)
        if p is None:
            return None
        return self.index.vector_for_id(p)

    def max_distance_for_id(self, item_id: str,
                            scope: Optional[str] = None) -> Optional[Dict]:
        """Distance to the farthest catalogue track (reference:
        get_max_distance_for_id ivf_manager.py:1177 — UI slider
        normalization). Cached per item. Under a scope, the farthest
        track among the scope's tracks (farthest_item_id None when the
        scope is empty)."""
        stamp, sc = self._resolve_scope(scope)
        key = ("maxd", item_id, scope, stamp)
        hit = self.cache.get(key)
        if hit is not None:
            return dict(hit)
        vec = self.vector_for_id(item_id)
        if vec is None:
            return None
        if sc is None:
            d, fid = self.index.max_distance(vec)
        else:
            d, fid = self.index.max_distance(vec, scope=sc)
        out = {"max_distance": d,
               "farthest_item_id": self.item_ids[fid] if fid >= 0 else None}
        self.cache.put(key, dict(out))
        return out

    # -- whole-catalogue neighbour graph -----------------------------------

    def neighbor_graph(self, k: int, nprobe: Optional[int] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """k nearest neighbours of every track, in item_ids order:
        (positions (N, k) int64 into self.item_ids, dists (N, k)). Line i
        describes item_ids[i] and never holds i; missing neighbours (and
        the lines of ids the index no longer holds) are -1 / +inf.
        IVFIndex.knn_graph reports in packed order; this fixes the order
        for callers who think in item ids."""
        gd, gi = self.index.knn_graph(k, nprobe=nprobe)
        n = len(self.item_ids)
        pos = torch.full((n, k), -1, dtype=torch.int64, device=gi.device)
        dists = torch.full((n, k), float("inf"), device=gd.device)
        pos[self.index.ids] = gi
        dists[self.index.ids] = gd
        return pos, dists

    def path_graph(self):
        """The PathGraph of the graph song path (engines/graph_path.py):
        neighbor_graph(PATH_GRAPH_NEIGHBOURS) with weights distance **
        PATH_GRAPH_EXPONENT, built on first use and kept until the index
        layout moves (add / remove / retrain). None for the dot metric,
        whose distances can be negative."""
        if self.index.metric == "dot":
            return None
        from audiomuse_amd.engines.graph_path import PathGraph

        with self._path_graph_lock:
            key = (self.index.layout_version, bool(C.PATH_GRAPH_CONNECT))
            if self._path_graph is None or self._path_graph[0] != key:
                pos, dists = self._graph_neighbours(key[0])
                self._path_graph = (key, PathGraph.from_knn(
                    pos, dists, C.PATH_GRAPH_EXPONENT))
            return self._path_graph[1]

    def _graph_neighbours(self, version: int
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
        """neighbor_graph(PATH_GRAPH_NEIGHBOURS) of this layout version,
        built once for path_graph and rank_graph; with PATH_GRAPH_CONNECT
        on, that table with the bridges of graph_connect.connect in extra
        columns, again built once per layout version. Called under
        _path_graph_lock."""
        if self._graph_knn is None or self._graph_knn[0] != version:
            k = max(1, min(C.PATH_GRAPH_NEIGHBOURS,
                           max(self.index.n - 1, 1)))
            self._graph_knn = (version, *self.neighbor_graph(k))
        if not C.PATH_GRAPH_CONNECT:
            return self._graph_knn[1], self._graph_knn[2]
        key = (version, True)
        if self._graph_connected is None or self._graph_connected[0] != key:
            from audiomuse_amd.engines.graph_connect import connect

            self._graph_connected = (key, *connect(
                self._graph_knn[1], self._graph_knn[2], self.index,
                C.PATH_GRAPH_BRIDGE_CANDIDATES, C.PATH_GRAPH_BRIDGE_ROUNDS))
        return self._graph_connected[1], self._graph_connected[2]

    def graph_report(self, build: bool = False) -> Optional[Dict]:
        """The figures of the graph that path_graph() and rank_graph() are
        made from, under the current PATH_GRAPH_CONNECT: connect,
        vertices, without_vector, components_before, largest_before,
        components_after, bridges, rounds, extra_slots, seconds (and the
        per-round label and scan timings of graph_connect.connect). None
        when that graph has not been built and build is False, and for
        the dot metric, which has no graph. With the setting off nothing
        is bridged: the components are counted once, on request."""
        if self.index.metric == "dot":
            return None
        with self._path_graph_lock:
            version = self.index.layout_version
            on = bool(C.PATH_GRAPH_CONNECT)
            if on:
                hit = self._graph_connected
                if hit is None or hit[0] != (version, True):
                    if not build:
                        return None
                    self._graph_neighbours(version)
                return dict(self._graph_connected[3])
            if self._graph_knn is None or self._graph_knn[0] != version:
                if not build:
                    return None
                self._graph_neighbours(version)
            hit = self._graph_plain_report
            if hit is None or hit[0] != (version, False):
                from audiomuse_amd.engines.graph_connect import connect

                _, _, rep = connect(self._graph_knn[1], self._graph_knn[2],
                                    self.index, 1, 0)
                rep["connect"] = False
                self._graph_plain_report = ((version, False), rep)
            return dict(self._graph_plain_report[1])

    def rank_graph(self):
        """The RankGraph of the graph radio (engines/graph_radio.py): the
        neighbours of path_graph with affinities exp(-d / sigma), sigma =
        RADIO_BANDWIDTH * the median edge distance; built on first use
        and kept until the index layout moves. None for the dot metric."""
        if self.index.metric == "dot":
            return None
        from audiomuse_amd.engines.graph_radio import RankGraph

        with self._path_graph_lock:
            key = (self.index.layout_version, bool(C.PATH_GRAPH_CONNECT))
            if self._rank_graph is None or self._rank_graph[0] != key:
                pos, dists = self._graph_neighbours(key[0])
                self._rank_graph = (key, RankGraph.from_knn(
                    pos, dists, C.RADIO_BANDWIDTH))
            return self._rank_graph[1]

    def community_graph(self):
        """The CommunityGraph of the graph communities (engines/
        graph_community.py): the neighbours of path_graph with integer
        weights round(COMMUNITY_WEIGHT_LEVELS * exp(-d / sigma)), sigma =
        COMMUNITY_BANDWIDTH * the median edge distance; built on first use
        and kept until the index layout moves. None for the dot metric."""
        if self.index.metric == "dot":
            return None
        from audiomuse_amd.engines.graph_community import CommunityGraph

        with self._path_graph_lock:
            key = (self.index.layout_version, bool(C.PATH_GRAPH_CONNECT))
            if self._community_graph is None or \
                    self._community_graph[0] != key:
                pos, dists = self._graph_neighbours(key[0])
                self._community_graph = (key, CommunityGraph.from_knn(
                    pos, dists, C.COMMUNITY_BANDWIDTH,
                    C.COMMUNITY_WEIGHT_LEVELS))
                self._communities = {}
            return self._community_graph[1]

    def communities(self, resolution: Optional[float] = None):
        """(labels (N,) int32 in item_ids order, 0..C-1 by descending
        size; report) of graph_community.communities over
        community_graph(), kept per graph and resolution (in 64ths). None
        for the dot metric."""
        from audiomuse_amd.engines import graph_community as GC

        if resolution is None:
            resolution = C.COMMUNITY_RESOLUTION
        g = GC.resolution_units(resolution)
        graph = self.community_graph()
        if graph is None:
            return None
        key = self._community_graph[0]
        with self._path_graph_lock:
            hit = self._communities.get((key, g))
        if hit is None:
            labels, report = GC.communities(
                graph, g / GC.RESOLUTION_UNIT, C.COMMUNITY_MAX_SWEEPS,
                C.COMMUNITY_MAX_LEVELS)
            hit = (labels, report)
            with self._path_graph_lock:
                if self._community_graph[0] == key:
                    self._communities[(key, g)] = hit
        return hit[0], dict(hit[1])

    # -- core query ------------------------------------------------------

    def _query_candidates(self, vec: torch.Tensor, fetch: int,
                          nprobe: Optional[int] = None,
                          scope: Optional[RowScope] = None
                          ) -> List[Tuple[str, float]]:
        if scope is None:
            dist, ids = self.index.query(vec, k=fetch, nprobe=nprobe)
        else:
            dist, ids = self.index.query(vec, k=fetch, nprobe=nprobe,
                                         scope=scope)
        out = []
        for d, i in zip(dist.tolist(), ids.tolist()):
            if i < 0 or not np.isfinite(d):
                continue
            out.append((self.item_ids[int(i)], float(d)))
        return out

    def _apply_filters(self, cands: List[Tuple[str, float]], n: int, *,
                       exclude: Sequence[str] = (),
                       eliminate_duplicates: Optional[bool] = None,
                       max_per_artist: Optional[int] = None,
                       mood_filter: Optional[str] = None
                       ) -> List[Tuple[str, float]]:
        """Near-dup lookback filter + artist cap + mood filter
        (ivf_manager.py:419-502, 652, 935)."""
        if eliminate_duplicates is None:
            eliminate_duplicates = C.SIMILARITY_ELIMINATE_DUPLICATES_DEFAULT
        lookback = C.DUPLICATE_DISTANCE_CHECK_LOOKBACK
        # threshold follows the index metric (reference keeps separate
        # cosine/euclidean knobs, ivf_manager.py:419)
        thresh = (C.DUPLICATE_DISTANCE_THRESHOLD_EUCLIDEAN
                  if self.index.metric == "euclidean"
                  else C.DUPLICATE_DISTANCE_THRESHOLD_COSINE)
        exclude_set = set(exclude)
        accepted: List[Tuple[str, float]] = []
        accepted_vecs: List[torch.Tensor] = []
        artist_counts: Dict[str, int] = {}
        # seed-mood similarity gate (reference MOOD_SIMILARITY_ENABLE:
        # neighbors must share the seed's mood profile, not just its
        # embedding neighborhood)
        seed_moods = None
        if C.MOOD_SIMILARITY_ENABLE and getattr(self, "_seed_moods", None):
            seed_moods = self._seed_moods
            seed_top = max(seed_moods, key=seed_moods.get)
            top_keys = sorted(seed_moods, key=seed_moods.get)[-5:]
        for item_id, dist in cands:
            if item_id in exclude_set:
                continue
            meta = self.meta_fn(item_id) or {}
            if mood_filter:
                moods = meta.get("mood_vector") or {}
                if moods and moods.get(mood_filter, 0.0) <= 0.0:
                    continue
            if seed_moods:
                moods = meta.get("mood_vector") or {}
                if moods:
                    if moods.get(seed_top, 0.0) < C.MOOD_SCORE_MATCH_THRESHOLD:
                        continue
                    drift = sum(abs(moods.get(m, 0.0) - seed_moods[m])
                                for m in top_keys) / max(len(top_keys), 1)
                    if drift > C.MOOD_SIMILARITY_THRESHOLD:
                        continue
            author = (meta.get("author") or "").strip().lower()
            cap = max_per_artist if max_per_artist is not None else C.MAX_SONGS_PER_ARTIST
            if cap and author and artist_counts.get(author, 0) >= cap:
                continue
            if eliminate_duplicates:
                vec = self.vector_for_id(item_id)
                dup = False
                if vec is not None:
                    for prev in accepted_vecs[-lookback:]:
                        cos = torch.dot(vec, prev) / (
                            vec.norm() * prev.norm() + 1e-12)
                        if 1.0 - float(cos) < thresh:
                            dup = True
                            break
                if dup:
                    continue
                if vec is not None:
                    accepted_vecs.append(vec)
            if author:
                artist_counts[author] = artist_counts.get(author, 0) + 1
            accepted.append((item_id, dist))
            if len(accepted) >= n:
                break
        return accepted

    def find_similar_by_vector(self, vec: torch.Tensor, n: int, *,
                               exclude: Sequence[str] = (),
                               eliminate_duplicates: Optional[bool] = None,
                               max_per_artist: Optional[int] = None,
                               mood_filter: Optional[str] = None,
                               radius: bool = False,
                               nprobe: Optional[int] = None,
                               scope: Optional[str] = None
                               ) -> List[Dict]:
        """scope: name resolved through scope_fn; only that scope's
        tracks are searched (the mask is applied inside the index scan,
        so a small scope still fills n)."""
        _stamp, sc = self._resolve_scope(scope)
        fetch = max(n * 4 + len(exclude), 32)
        cands = self._query_candidates(vec, fetch, nprobe=nprobe, scope=sc)
        if radius:
            nprobe = nprobe or C.IVF_MAX_DISTANCE_NPROBE  # wider probe
            cands = self._query_candidates(vec, fetch, nprobe=nprobe,
                                           scope=sc)
            cdata = []
            for item_id, dist in cands:
                if item_id in set(exclude):
                    continue
                v = self.vector_for_id(item_id)
                if v is None:
                    continue
                meta = self.meta_fn(item_id) or {}
                cdata.append({"item_id": item_id, "vector": v.cpu().numpy(),
                              "dist_anchor": dist,
                              "author": meta.get("author")})
            walked = execute_radius_walk(
                cdata, n, eliminate_duplicates=eliminate_duplicates,
                max_songs_per_artist=max_per_artist or C.MAX_SONGS_PER_ARTIST
                or None)
            return walked
        picked = self._apply_filters(
            cands, n, exclude=exclude,
            eliminate_duplicates=eliminate_duplicates,
            max_per_artist=max_per_artist, mood_filter=mood_filter)
        return [{"item_id": i, "distance": d} for i, d in picked]

    def find_similar_by_id(self, item_id: str, n: int, *,
                           scope: Optional[str] = None, **kw) -> List[Dict]:
        """reference: find_nearest_neighbors_by_id (ivf_manager.py:994)."""
        stamp, _sc = self._resolve_scope(scope)
        key = (item_id, n, scope, stamp, tuple(sorted(kw.items())))
        hit = self.cache.get(key)
        if hit is not None:
            return hit
        vec = self.vector_for_id(item_id)
        if vec is None:
            return []
        kw.setdefault("exclude", (item_id,))
        # stash the seed's mood profile for the MOOD_SIMILARITY_ENABLE
        # gate (id-anchored queries only — raw vectors carry no moods)
        self._seed_moods = (self.meta_fn(item_id) or {}).get("mood_vector") \
            if C.MOOD_SIMILARITY_ENABLE else None
        try:
            out = self.find_similar_by_vector(vec, n, scope=scope, **kw)
        finally:
            self._seed_moods = None
        self.cache.put(key, out)
        return out

    def multi_query(self, vectors: Sequence[torch.Tensor], n: int, *,
                    exclude: Sequence[str] = (),
                    scope: Optional[str] = None, **kw) -> List[Dict]:
        """Union of per-vector queries, best distance per id, re-sorted
        (reference: multi_query_ids, ivf_manager.py:389)."""
        _stamp, sc = self._resolve_scope(scope)
        best: Dict[str, float] = {}
        for vec in vectors:
            for item_id, dist in self._query_candidates(vec, n * 4, scope=sc):
                if dist < best.get(item_id, float("inf")):
                    best[item_id] = dist
        merged = sorted(best.items(), key=lambda kv: kv[1])
        picked = self._apply_filters(merged, n, exclude=exclude, **kw)
        return [{"item_id": i, "distance": d} for i, d in picked]


def build_engine_from_matrix(matrix: np.ndarray, ids: Sequence[str],
                             metric: str = "angular",
                             storage: Optional[str] = None,
                             device: str = "cpu",
                             meta_fn: Optional[MetaFn] = None,
                             nlist: Optional[int] = None,
                             scope_fn: Optional[ScopeFn] = None
                             ) -> SimilarityEngine:
    x = torch.as_tensor(np.asarray(matrix, dtype=np.float32))
    index = IVFIndex.build(x, metric=metric, storage=storage, device=device,
                           nlist=nlist)
    return SimilarityEngine(index, ids, meta_fn=meta_fn, scope_fn=scope_fn)
