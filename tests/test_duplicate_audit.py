"""Catalogue duplicate audit (analysis/duplicates.py), its task handler and
the /api/duplicates routes, over a catalogue with planted duplicates."""

import zlib

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.analysis import duplicates as dup
from audiomuse_amd.db import connect, write_txn
from audiomuse_amd.db.schema import init_db
from audiomuse_amd.db.store import save_track_analysis_and_embedding
from audiomuse_amd.engines.similarity import build_engine_from_matrix

DIM = 200
K = 2            # small on purpose: see the triple below
NEAR = 0.05      # cosine distance of planted neighbours


def _iid(i: int) -> str:
    return f"fp_4{'%050x' % i}"


def _unit(v):
    return v / np.linalg.norm(v)


def _rotate(a, u, delta):
    """Unit vector at cosine distance delta from a, in the plane (a, u);
    u is orthonormal to a."""
    c = 1.0 - delta
    return c * a + np.sqrt(1.0 - c * c) * u


def _orth(a, rng):
    u = rng.standard_normal(a.size)
    return _unit(u - (u @ a) * a)


def _fp(base, shift, rng, flips=3) -> bytes:
    words = base[40 + shift: 300 + shift].copy()
    for w in rng.choice(words.size, size=flips, replace=False):
        words[w] ^= np.uint32(1 << int(rng.integers(0, 24)))
    return zlib.compress(words.tobytes())


def _catalogue(n: int):
    """n tracks. Planted, by name -> position:
    - dup1a/dup1b and dup2a/dup2b: one fingerprint shifted by 5 and by -12
      frames; embeddings NEAR apart, beyond SIMHASH_CONFIRM_COSINE;
    - triA - triB - triC on one great circle with B in the middle, and one
      closer satellite beyond A and beyond C, so that with K = 2 the graph
      holds A-B and B-C but not A-C;
    - decoy a/b: NEAR embeddings, unrelated fingerprints;
    - dur a/b: agreeing fingerprints, durations 40 s apart;
    - nofp a/b: NEAR embeddings, b has no fingerprint row.
    Everything else is random."""
    rng = np.random.default_rng(2024)
    assert NEAR > C.SIMHASH_CONFIRM_COSINE
    emb = np.stack([_unit(rng.standard_normal(DIM)) for _ in range(n)])
    fps = [zlib.compress(rng.integers(0, 1 << 24, size=260,
                                      dtype=np.uint32).tobytes())
           for _ in range(n)]
    dur = np.full(n, 200.0)
    names = ["dup1a", "dup1b", "dup2a", "dup2b", "triA", "triB", "triC",
             "satA", "satC", "decoya", "decoyb", "dura", "durb", "nofpa",
             "nofpb"]
    # spread the planted tracks over the catalogue
    where = dict(zip(names, rng.choice(n, size=len(names), replace=False)
                     .tolist()))

    def near_pair(a, b):
        emb[where[b]] = _rotate(emb[where[a]], _orth(emb[where[a]], rng),
                                NEAR)

    def base():
        return rng.integers(0, 1 << 24, size=400, dtype=np.uint32)

    for a, b, shift in (("dup1a", "dup1b", 5), ("dup2a", "dup2b", -12)):
        near_pair(a, b)
        src = base()
        fps[where[a]], fps[where[b]] = _fp(src, 0, rng), _fp(src, shift, rng)

    mid = emb[where["triB"]]
    u = _orth(mid, rng)
    theta, sat = np.arccos(1.0 - NEAR), np.arccos(1.0 - 0.03)
    for name, angle in (("triA", theta), ("satA", theta + sat),
                        ("triC", -theta), ("satC", -theta - sat)):
        emb[where[name]] = np.cos(angle) * mid + np.sin(angle) * u
    src = base()
    for name, shift in (("triA", 0), ("triB", 3), ("triC", -4)):
        fps[where[name]] = _fp(src, shift, rng)

    near_pair("decoya", "decoyb")
    near_pair("dura", "durb")
    src = base()
    fps[where["dura"]], fps[where["durb"]] = _fp(src, 0, rng), _fp(src, 2, rng)
    dur[where["durb"]] = 240.0
    near_pair("nofpa", "nofpb")
    fps[where["nofpb"]] = None
    return {"emb": emb.astype(np.float32), "fps": fps, "dur": dur,
            "where": where, "ids": [_iid(i) for i in range(n)]}


def _store(conn, cat) -> None:
    with write_txn(conn):
        for i, iid in enumerate(cat["ids"]):
            save_track_analysis_and_embedding(
                conn, iid, title=f"Song {i}", author=f"Artist {i % 7}",
                album=f"Album {i % 11}", duration=float(cat["dur"][i]),
                embedding=cat["emb"][i])
            if cat["fps"][i] is not None:
                conn.execute(
                    "INSERT INTO chromaprint (item_id, fingerprint, duration) "
                    "VALUES (?,?,?)", (iid, cat["fps"][i],
                                       float(cat["dur"][i])))
            for server in ("main", "second")[: 1 + i % 2]:
                conn.execute(
                    "INSERT INTO track_server_map (provider_id, server_id, "
                    "item_id) VALUES (?,?,?)", (f"p{i}", server, iid))


def _expected_groups(cat):
    w, ids = cat["where"], cat["ids"]
    return {frozenset(ids[w[m]] for m in members)
            for members in (("dup1a", "dup1b"), ("dup2a", "dup2b"),
                            ("triA", "triB", "triC"))}


def _group_sets(report):
    return {frozenset(m["item_id"] for m in g["members"])
            for g in report["groups"]}


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    cat = _catalogue(60)
    url = "sqlite:///" + str(tmp_path_factory.mktemp("dup") / "dup.db")
    conn = connect(url)
    init_db(conn)
    _store(conn, cat)
    engine = build_engine_from_matrix(cat["emb"], cat["ids"])
    yield {"cat": cat, "conn": conn, "engine": engine, "url": url}
    conn.close()


def test_groups_and_counters(small):
    cat, conn, engine = small["cat"], small["conn"], small["engine"]
    w = cat["where"]
    pairs, dist = dup.candidate_pairs(engine, K)
    cand = {tuple(p) for p in pairs.tolist()}
    assert all(a < b for a, b in cand) and len(cand) == pairs.shape[0]

    def pair(a, b):
        return (min(w[a], w[b]), max(w[a], w[b]))

    # the construction holds: the graph proposes every planted pair and
    # does not propose A-C
    for a, b in (("dup1a", "dup1b"), ("dup2a", "dup2b"), ("triA", "triB"),
                 ("triB", "triC"), ("decoya", "decoyb"), ("dura", "durb"),
                 ("nofpa", "nofpb")):
        assert pair(a, b) in cand, (a, b)
    assert pair("triA", "triC") not in cand
    by_pair = dict(zip(map(tuple, pairs.tolist()), dist.tolist()))
    assert abs(by_pair[pair("dup1a", "dup1b")] - NEAR) < 5e-3

    report = dup.find_duplicate_recordings(conn, engine, k=K)
    assert _group_sets(report) == _expected_groups(cat)
    assert report["n_tracks"] == 60
    assert report["n_candidates"] == len(cand)
    # every pair with the track that has no fingerprint row goes, and so
    # does every pair with the one track whose duration is 40 s off
    gone = {w["nofpb"], w["durb"]}
    assert report["n_compared"] == sum(1 for a, b in cand
                                       if a not in gone and b not in gone)
    assert report["n_confirmed"] == 4 and report["n_groups"] == 3
    assert report["truncated"] is False

    sizes = [g["size"] for g in report["groups"]]
    assert sizes == [3, 2, 2]
    triple = report["groups"][0]
    assert len(triple["pairs"]) == 2
    ids = cat["ids"]
    offsets = {frozenset((p["a"], p["b"])): p for p in triple["pairs"]}
    ab = offsets[frozenset((ids[w["triA"]], ids[w["triB"]]))]
    assert abs(ab["offset"]) == 3 and ab["ratio"] > 0.99
    assert abs(ab["distance"] - NEAR) < 5e-3
    for g in report["groups"]:
        assert g["best_ratio"] >= C.CHROMAPRINT_MATCH_THRESHOLD
        for m in g["members"]:
            i = ids.index(m["item_id"])
            assert m["title"] == f"Song {i}" and m["author"] == f"Artist {i % 7}"
            assert m["album"] == f"Album {i % 11}" and m["duration"] == 200.0
            assert m["servers"] == ["main", "second"][: 1 + i % 2]
    for g in report["groups"][1:]:
        (p,) = g["pairs"]
        assert abs(p["offset"]) in (5, 12)


def test_truncated(small, monkeypatch):
    monkeypatch.setattr(C, "DUPLICATE_AUDIT_MAX_GROUPS", 1)
    report = dup.find_duplicate_recordings(small["conn"], small["engine"],
                                           k=K)
    assert report["truncated"] is True and report["n_groups"] == 3
    assert len(report["groups"]) == 1 and report["groups"][0]["size"] == 3


def test_max_cosine_removes_everything(small, monkeypatch):
    monkeypatch.setattr(C, "DUPLICATE_AUDIT_MAX_COSINE", NEAR / 2)
    report = dup.find_duplicate_recordings(small["conn"], small["engine"],
                                           k=K)
    assert report["groups"] == [] and report["n_confirmed"] == 0
    # nothing planted is within the cap (the closest, the satellites, are
    # 0.03 apart) and random tracks are far
    assert report["n_candidates"] == 0 and report["n_compared"] == 0
    # a cap between the satellites and the planted pairs keeps only those
    monkeypatch.setattr(C, "DUPLICATE_AUDIT_MAX_COSINE", 0.04)
    report = dup.find_duplicate_recordings(small["conn"], small["engine"],
                                           k=K)
    assert report["n_candidates"] == 2 and report["n_confirmed"] == 0


# -- task handler and API ----------------------------------------------------

def _run_pending(url):
    from audiomuse_amd.taskqueue.worker import Worker, import_builtin_handlers

    import_builtin_handlers()
    conn = connect(url)
    try:
        assert Worker(db_url=url).run_one(conn)
    finally:
        conn.close()


def test_api_start_conflict_and_report(tmp_path):
    from audiomuse_amd.analysis.index import build_audio_index
    from audiomuse_amd.web.app import create_app

    cat = _catalogue(60)
    url = "sqlite:///" + str(tmp_path / "api.db")
    conn = connect(url)
    init_db(conn)
    _store(conn, cat)
    assert build_audio_index(conn) == 60
    app = create_app(url, auth_disabled=True)
    app.testing = True
    with app.test_client() as client:
        assert client.get("/api/duplicates").status_code == 404
        r = client.post("/api/duplicates/start", json={"k": K})
        assert r.status_code == 202
        tid = r.json["task_id"]
        again = client.post("/api/duplicates/start", json={})
        assert again.status_code == 409 and again.json["task_id"] == tid
        assert client.get("/api/duplicates").status_code == 404  # not run yet
        _run_pending(url)
        task = client.get(f"/api/task/{tid}").json
        assert task["status"] == "SUCCESS" and task["progress"] == 100.0
        r = client.get("/api/duplicates")
        assert r.status_code == 200 and r.json["task_id"] == tid
        assert _group_sets(r.json) == _expected_groups(cat)
        assert r.json["n_confirmed"] == 4 and r.json["n_tracks"] == 60
        # a finished audit admits the next one
        assert client.post("/api/duplicates/start").status_code == 202
    conn.close()


def test_api_needs_auth(tmp_path):
    from audiomuse_amd.web.app import create_app

    url = "sqlite:///" + str(tmp_path / "auth.db")
    conn = connect(url)
    init_db(conn)
    app = create_app(url, auth_disabled=False)
    app.testing = True
    with app.test_client() as client:
        r = client.post("/api/setup/admin", json={"username": "admin",
                                                  "password": "longenough1"})
        assert r.status_code == 200
    with app.test_client() as anon:
        assert anon.post("/api/duplicates/start").status_code == 401
        assert anon.get("/api/duplicates").status_code == 401
    assert conn.execute("SELECT COUNT(*) FROM task_status").fetchone()[0] == 0
    conn.close()


def test_task_without_index_fails(tmp_path):
    from audiomuse_amd.taskqueue import enqueue, task_row

    url = "sqlite:///" + str(tmp_path / "noindex.db")
    conn = connect(url)
    init_db(conn)
    tid = enqueue(conn, "duplicate_audit", {}, queue="high")
    _run_pending(url)
    assert task_row(conn, tid)["status"] == "FAILURE"
    conn.close()


# -- GPU ---------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_audit_matches_cpu(tmp_path):
    cat = _catalogue(2000)
    conn = connect("sqlite:///" + str(tmp_path / "gpu.db"))
    init_db(conn)
    _store(conn, cat)
    cpu = dup.find_duplicate_recordings(
        conn, build_engine_from_matrix(cat["emb"], cat["ids"]), k=K)
    engine = build_engine_from_matrix(cat["emb"], cat["ids"], device="cuda")
    assert engine.index.device.type == "cuda"
    gpu = dup.find_duplicate_recordings(conn, engine, k=K)
    conn.close()
    assert _group_sets(cpu) == _expected_groups(cat)
    assert _group_sets(gpu) == _group_sets(cpu)
    assert gpu["n_confirmed"] == cpu["n_confirmed"] == 4
    assert gpu["n_tracks"] == 2000
    for gg, gc in zip(gpu["groups"], cpu["groups"]):
        key = lambda p: (p["a"], p["b"])                       # noqa: E731
        for pg, pc in zip(sorted(gg["pairs"], key=key),
                          sorted(gc["pairs"], key=key)):
            assert (pg["a"], pg["b"], pg["offset"]) == \
                (pc["a"], pc["b"], pc["offset"])
            assert pg["ratio"] == pc["ratio"]      # integers in, same float
