"""Catalogue duplicate audit: the same recording under two canonical ids.

Identity is decided once, at analysis time (tasks._persist_album: simhash
band lookup, cosine, duration, fingerprint gate). A remaster, another
encode or the same song on an album and on a compilation can land just
outside SIMHASH_CONFIRM_COSINE and stay split. The audit looks at the
finished catalogue instead: the embedding index proposes the k nearest
neighbours of every track (SimilarityEngine.neighbor_graph) and the
acoustic fingerprint decides (engines/chromaprint.match_pairs, one batched
call for all candidate pairs).

The audit reports and never merges.
"""

from __future__ import annotations

import sqlite3
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines.chromaprint import FingerprintBank, match_pairs
from audiomuse_amd.taskqueue.worker import TaskContext, task_handler

StageFn = Callable[[float, str], None]


def candidate_pairs(engine, k: int, max_cosine: float = 0.0
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Unordered, unique neighbour pairs of the whole catalogue:
    (pairs (M, 2) int64 positions into engine.item_ids with i < j, dist
    (M,) the pair's distance), on the index's device. -1 padding is
    dropped; with max_cosine > 0 so are pairs farther apart than that."""
    pos, dist = engine.neighbor_graph(k)
    n = pos.shape[0]
    src = torch.arange(n, device=pos.device)[:, None].expand_as(pos)
    keep = (pos >= 0) & (pos != src)
    if max_cosine > 0:
        keep &= dist <= max_cosine
    a, b, d = src[keep], pos[keep], dist[keep]
    key = torch.minimum(a, b) * n + torch.maximum(a, b)
    uniq, inv = torch.unique(key, return_inverse=True)
    # i -> j and j -> i carry the same distance up to the scan's rounding;
    # keep the smaller
    dmin = torch.full((uniq.numel(),), float("inf"), device=d.device,
                      dtype=d.dtype).scatter_reduce(0, inv, d, "amin")
    pairs = torch.stack([uniq // max(n, 1), uniq % max(n, 1)], dim=1)
    return pairs, dmin


def audit_pairs(engine, bank: FingerprintBank, has_fp: torch.Tensor,
                duration: torch.Tensor, *, k: int, max_cosine: float,
                threshold: float, stage: Optional[StageFn] = None) -> Dict:
    """The audit on arrays. bank, has_fp (bool) and duration (float, <= 0
    or NaN for unknown) are indexed like engine.item_ids and live on the
    bank's device. Returns the confirmed pairs (numpy) and the counters."""
    stage = stage or (lambda _p, _d: None)
    dev = bank.device
    stage(10.0, "neighbour graph")
    pairs, dist = candidate_pairs(engine, k, max_cosine)
    pairs, dist = pairs.to(dev), dist.to(dev)
    n_candidates = int(pairs.shape[0])
    stage(40.0, f"{n_candidates} candidate pairs")
    i, j = pairs[:, 0], pairs[:, 1]
    keep = has_fp[i] & has_fp[j]
    di, dj = duration[i], duration[j]
    known = (di > 0) & (dj > 0)     # NaN compares false: unknown
    keep &= ~(known & ((di - dj).abs() > C.SIMHASH_CONFIRM_DURATION_SECONDS))
    pairs, dist = pairs[keep], dist[keep]
    n_compared = int(pairs.shape[0])
    stage(50.0, f"comparing {n_compared} fingerprint pairs")
    ratio, offset = match_pairs(bank, pairs)
    hit = np.nonzero(ratio >= threshold)[0]
    return {"pairs": pairs.cpu().numpy()[hit], "ratio": ratio[hit],
            "offset": offset[hit], "distance": dist.cpu().numpy()[hit],
            "n_candidates": n_candidates, "n_compared": n_compared,
            "n_confirmed": int(hit.size)}


def _groups(pairs: np.ndarray) -> List[List[int]]:
    """Union-find over the confirmed pairs: member positions per group."""
    parent: Dict[int, int] = {}

    def find(x: int) -> int:
        root = x
        while parent.setdefault(root, root) != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    out: Dict[int, List[int]] = {}
    for x in sorted(parent):
        out.setdefault(find(x), []).append(x)
    return list(out.values())


def _member_rows(conn: sqlite3.Connection, item_ids: List[str]) -> Dict:
    meta: Dict[str, Dict] = {}
    for lo in range(0, len(item_ids), 500):
        part = tuple(item_ids[lo:lo + 500])
        marks = ",".join("?" for _ in part)
        for r in conn.execute(
                "SELECT item_id, title, author, album, duration FROM score "
                f"WHERE item_id IN ({marks})", part).fetchall():
            meta[r["item_id"]] = {"item_id": r["item_id"], "title": r["title"],
                                  "author": r["author"], "album": r["album"],
                                  "duration": r["duration"], "servers": []}
        for r in conn.execute(
                "SELECT item_id, server_id FROM track_server_map "
                f"WHERE item_id IN ({marks}) ORDER BY server_id",
                part).fetchall():
            m = meta.get(r["item_id"])
            if m is not None and r["server_id"] not in m["servers"]:
                m["servers"].append(r["server_id"])
    return meta


def find_duplicate_recordings(conn: sqlite3.Connection, engine, *,
                              k: Optional[int] = None,
                              max_cosine: Optional[float] = None,
                              threshold: Optional[float] = None,
                              stage: Optional[StageFn] = None) -> Dict:
    """Groups of catalogue tracks whose fingerprints agree although they
    carry different canonical ids. Candidates are the k nearest neighbours
    of every track in `engine`; pairs without a fingerprint row on either
    side, or with known durations more than
    SIMHASH_CONFIRM_DURATION_SECONDS apart (the resolver's gate), are
    dropped; the rest are compared in one match_pairs call and kept at
    ratio >= threshold. Returns the report dict; nothing is written."""
    k = int(C.DUPLICATE_AUDIT_NEIGHBOURS if k is None else k)
    max_cosine = float(C.DUPLICATE_AUDIT_MAX_COSINE if max_cosine is None
                       else max_cosine)
    threshold = float(C.CHROMAPRINT_MATCH_THRESHOLD if threshold is None
                      else threshold)
    stage = stage or (lambda _p, _d: None)
    ids = engine.item_ids
    n = len(ids)
    dev = engine.index.device
    report = {"groups": [], "n_tracks": n, "n_candidates": 0,
              "n_compared": 0, "n_confirmed": 0, "n_groups": 0,
              "truncated": False}
    if n < 2:
        return report

    stage(2.0, "loading fingerprints")
    blobs: List[Optional[bytes]] = [None] * n
    has_fp = np.zeros(n, dtype=bool)
    duration = np.zeros(n, dtype=np.float64)
    for r in conn.execute("SELECT item_id, duration FROM score").fetchall():
        p = engine.pos.get(r["item_id"])
        if p is not None and r["duration"]:
            duration[p] = r["duration"]
    for r in conn.execute(
            "SELECT item_id, fingerprint, duration FROM chromaprint"
    ).fetchall():
        p = engine.pos.get(r["item_id"])
        if p is None:
            continue
        has_fp[p] = True
        blobs[p] = r["fingerprint"]
        if duration[p] <= 0 and r["duration"]:
            duration[p] = r["duration"]
    bank = FingerprintBank.from_blobs(blobs, dev)
    del blobs

    res = audit_pairs(engine, bank, torch.from_numpy(has_fp).to(dev),
                      torch.from_numpy(duration).to(dev), k=k,
                      max_cosine=max_cosine, threshold=threshold, stage=stage)
    for key in ("n_candidates", "n_compared", "n_confirmed"):
        report[key] = res[key]
    stage(90.0, f"{res['n_confirmed']} confirmed pairs")

    by_group = []
    root_of = {}
    for g, members in enumerate(_groups(res["pairs"])):
        for m in members:
            root_of[m] = g
        by_group.append({"members": members, "pairs": []})
    for (a, b), ratio, off, dist in zip(res["pairs"].tolist(),
                                        res["ratio"].tolist(),
                                        res["offset"].tolist(),
                                        res["distance"].tolist()):
        by_group[root_of[a]]["pairs"].append(
            {"a": ids[a], "b": ids[b], "ratio": ratio, "offset": off,
             "distance": dist})
    for g in by_group:
        g["size"] = len(g["members"])
        g["best_ratio"] = max(p["ratio"] for p in g["pairs"])
    by_group.sort(key=lambda g: (-g["size"], -g["best_ratio"],
                                 ids[g["members"][0]]))
    report["n_groups"] = len(by_group)
    cap = int(C.DUPLICATE_AUDIT_MAX_GROUPS)
    if cap > 0 and len(by_group) > cap:
        by_group = by_group[:cap]
        report["truncated"] = True
    meta = _member_rows(conn, [ids[m] for g in by_group
                               for m in g["members"]])
    for g in by_group:
        g["members"] = [meta.get(ids[m]) or
                        {"item_id": ids[m], "title": None, "author": None,
                         "album": None, "duration": None, "servers": []}
                        for m in g["members"]]
    report["groups"] = by_group
    return report


@task_handler("duplicate_audit")
def duplicate_audit_task(ctx: TaskContext, payload: Dict) -> Dict:
    """Run the audit over the stored audio index; the report is the task
    result (GET /api/duplicates serves the newest one)."""
    from audiomuse_amd.analysis.index import AUDIO_INDEX, load_ivf_engine

    device = "cuda" if torch.cuda.is_available() else "cpu"
    ctx.report(1.0, "loading audio index")
    engine = load_ivf_engine(ctx.conn, AUDIO_INDEX, device=device)
    if engine is None:
        # a failed task, not a "successful" report without groups
        raise RuntimeError("audio index not built")
    ctx.check_cancelled()

    def stage(progress: float, details: str) -> None:
        ctx.check_cancelled()
        ctx.report(progress, details)

    report = find_duplicate_recordings(
        ctx.conn, engine, k=payload.get("k"),
        max_cosine=payload.get("max_cosine"),
        threshold=payload.get("threshold"), stage=stage)
    ctx.report(100.0, f"{report['n_groups']} duplicate groups")
    return report
