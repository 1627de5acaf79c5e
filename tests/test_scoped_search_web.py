"""Web API under ?server=: a server that holds a small share of the
catalogue still gets full answers, because the availability mask is
applied inside the index scan and not after top-k."""

import numpy as np
import pytest

from audiomuse_amd.analysis.index import build_audio_index
from audiomuse_amd.db import connect, write_txn
from audiomuse_amd.db.schema import init_db
from audiomuse_amd.db.store import save_track_analysis_and_embedding
from audiomuse_amd.web.app import create_app

N_TRACKS = 400


@pytest.fixture(scope="module")
def scoped_client(tmp_path_factory):
    url = "sqlite:///" + str(tmp_path_factory.mktemp("scoped") / "web.db")
    conn = connect(url)
    init_db(conn)
    rng = np.random.default_rng(3)
    ids = []
    for i in range(N_TRACKS):
        iid = f"fp_4{'%050x' % i}"
        ids.append(iid)
        save_track_analysis_and_embedding(
            conn, iid, title=f"Song {i}", author=f"Artist {i}",
            album=f"Album {i % 40}", tempo=100.0, energy=0.5, key="C",
            scale="major", duration=200.0, mood_vector={}, other_features={},
            embedding=rng.standard_normal(200).astype(np.float32))
    build_audio_index(conn)
    mapped = ids[5::33][:12]
    assert len(mapped) == 12 and ids[0] not in mapped
    with write_txn(conn):
        for k, iid in enumerate(mapped):
            conn.execute(
                "INSERT OR REPLACE INTO track_server_map "
                "(provider_id, server_id, item_id) VALUES (?, 'tiny', ?)",
                (f"tn-{k}", iid))
        # a second server maps the same tracks under other provider ids
        for k, iid in enumerate(ids[:50]):
            conn.execute(
                "INSERT OR REPLACE INTO track_server_map "
                "(provider_id, server_id, item_id) VALUES (?, 'other', ?)",
                (f"ot-{k}", iid))
    app = create_app(url, device="cpu", auth_disabled=True)
    app.testing = True
    with app.test_client() as client:
        yield client, ids, mapped
    conn.close()


def test_similar_tracks_small_server_gets_full_answer(scoped_client):
    client, ids, mapped = scoped_client
    r = client.get(f"/api/similar_tracks?item_id={ids[0]}&n=8&server=tiny")
    assert r.status_code == 200
    body = r.json
    assert len(body) == 8
    pid_of = {iid: f"tn-{k}" for k, iid in enumerate(mapped)}
    for b in body:
        assert b["item_id"] in pid_of
        assert b["provider_id"] == pid_of[b["item_id"]]
        assert b["title"] and b["author"]
    assert len({b["item_id"] for b in body}) == 8
    dists = [b["distance"] for b in body]
    assert dists == sorted(dists)
    # the unscoped answer is another one and carries no provider id
    plain = client.get(f"/api/similar_tracks?item_id={ids[0]}&n=8").json
    assert len(plain) == 8
    assert [b["item_id"] for b in plain] != [b["item_id"] for b in body]
    assert all("provider_id" not in b for b in plain)
    # asked again (now from the result cache), each stays itself
    again = client.get(
        f"/api/similar_tracks?item_id={ids[0]}&n=8&server=tiny").json
    assert again == body


def test_similar_tracks_unknown_server_is_empty(scoped_client):
    client, ids, _ = scoped_client
    r = client.get(f"/api/similar_tracks?item_id={ids[0]}&n=8&server=nobody")
    assert r.status_code == 200 and r.json == []


def test_max_distance_scoped_to_server(scoped_client):
    client, ids, mapped = scoped_client
    r = client.get(f"/api/max_distance?item_id={ids[0]}&server=tiny")
    assert r.status_code == 200
    assert r.json["farthest_item_id"] in mapped
    plain = client.get(f"/api/max_distance?item_id={ids[0]}").json
    assert r.json["max_distance"] <= plain["max_distance"]
    r = client.get(f"/api/max_distance?item_id={ids[0]}&server=nobody")
    assert r.status_code == 200 and r.json["farthest_item_id"] is None


def test_invalidate_clears_scopes(scoped_client):
    client, ids, mapped = scoped_client
    state = client.application.extensions["audiomuse"]
    client.get(f"/api/similar_tracks?item_id={ids[0]}&n=3&server=tiny")
    from audiomuse_amd.analysis import index as idx

    eng = state.engine(idx.AUDIO_INDEX)
    assert "tiny" in eng._scopes
    state.invalidate()
    assert eng._scopes == {}
