"""Selection inside the IVF scan: scan_topk / query_topk / knn_graph, the
fused scan + top-K kernel behind them, and the consumers of the
whole-catalogue neighbour graph (song map, SimilarityEngine)."""

import io

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines import projection
from audiomuse_amd.engines.similarity import build_engine_from_matrix
from audiomuse_amd.index.ivf import (_DTYPE_CODE, _METRIC_CODE, TOPK_KMAX,
                                     IVFIndex)
from tests.test_ivf import _corpus
from tests.test_ivf_scope import (GPU_PAIRS, NLIST, PAIRS, D, N, _allowed,
                                  _index, _queries, _x)

INF = float("inf")


def _select(dist, row, kk, skip=None):
    """scan() output -> the kk best in (distance, row) order, written
    independently of IVFIndex._ordered_select: a python sort per query."""
    out_d = torch.full((dist.shape[0], kk), INF)
    out_r = torch.full((dist.shape[0], kk), -1, dtype=torch.int32)
    for qi in range(dist.shape[0]):
        cands = [(d, r) for d, r in zip(dist[qi].tolist(), row[qi].tolist())
                 if r >= 0 and d != INF
                 and (skip is None or r != int(skip[qi]))]
        cands.sort()
        for j, (d, r) in enumerate(cands[:kk]):
            out_d[qi, j], out_r[qi, j] = d, r
    return out_d, out_r


# -- CPU: semantics ----------------------------------------------------------

@pytest.mark.parametrize("kk", [1, 10, 300])
@pytest.mark.parametrize("metric,storage", PAIRS)
def test_scan_topk_equals_scan_and_ordered_selection(metric, storage, kk):
    assert TOPK_KMAX == 256 and 300 > TOPK_KMAX
    idx = _index(metric, storage)
    q = _queries()
    dist, row = idx.scan(q, nprobe=4)
    exp_d, exp_r = _select(dist, row, kk)
    got_d, got_r = idx.scan_topk(q, kk, nprobe=4)
    assert got_d.shape == (6, kk) and got_r.shape == (6, kk)
    assert got_r.dtype == torch.int32 and got_d.dtype == torch.float32
    assert torch.equal(got_r, exp_r) and torch.equal(got_d, exp_d)


def test_scan_topk_pads_when_kk_exceeds_candidates():
    idx = _index("angular", "i8")
    q = _queries()
    dist, row = idx.scan(q, nprobe=1)
    counts = (row >= 0).sum(dim=1)
    kk = int(counts.max()) + 7
    got_d, got_r = idx.scan_topk(q, kk, nprobe=1)
    assert got_d.shape == (6, kk)
    for qi in range(6):
        c = int(counts[qi])
        assert (got_r[qi, :c] >= 0).all() and torch.isfinite(got_d[qi, :c]).all()
        assert (got_r[qi, c:] == -1).all() and torch.isinf(got_d[qi, c:]).all()
        assert sorted(got_r[qi, :c].tolist()) == sorted(
            row[qi][row[qi] >= 0].tolist())


def test_scan_topk_skip_rows_and_1d_query():
    idx = _index("angular", "f32")
    q = _queries()
    base_d, base_r = idx.scan_topk(q, 10, nprobe=4)
    # skip each query's best hit: exactly that row goes, the rest moves up
    skip = base_r[:, 0].clone()
    d1, r1 = idx.scan_topk(q, 10, nprobe=4, skip_rows=skip)
    full_d, full_r = idx.scan_topk(q, 11, nprobe=4)
    assert torch.equal(r1, full_r[:, 1:]) and torch.equal(d1, full_d[:, 1:])
    # -1 skips nothing
    d2, r2 = idx.scan_topk(q, 10, nprobe=4,
                           skip_rows=torch.full((6,), -1))
    assert torch.equal(r2, base_r) and torch.equal(d2, base_d)
    # packed rows 0 and N-1, all cells probed so both are candidates
    for edge in (0, N - 1):
        all_d, all_r = idx.scan_topk(q, N, nprobe=NLIST)
        got_d, got_r = idx.scan_topk(q, N, nprobe=NLIST,
                                     skip_rows=torch.full((6,), edge))
        for qi in range(6):
            assert edge in all_r[qi].tolist()
            keep = all_r[qi] != edge
            assert torch.equal(got_r[qi, : N - 1], all_r[qi][keep])
            assert torch.equal(got_d[qi, : N - 1], all_d[qi][keep])
            assert int(got_r[qi, -1]) == -1 and got_d[qi, -1] == INF
    # a row outside the probed cells: nothing changes
    q_enc, _ = idx._prepare_queries(q[:1])
    probed = set(idx._rank_cells(q_enc, 4)[0].tolist())
    off = idx.cell_off.tolist()
    outside = next(off[c] for c in range(NLIST)
                   if c not in probed and off[c + 1] > off[c])
    d3, r3 = idx.scan_topk(q[:1], 10, nprobe=4, skip_rows=[outside])
    assert torch.equal(r3, base_r[:1]) and torch.equal(d3, base_d[:1])
    # 1-D query: one line of results
    d4, r4 = idx.scan_topk(q[0], 10, nprobe=4)
    assert d4.shape == (1, 10)
    assert torch.equal(r4[0], base_r[0]) and torch.equal(d4[0], base_d[0])


@pytest.mark.parametrize("metric,storage", PAIRS)
def test_scan_topk_scoped_matches_scan(metric, storage):
    idx = _index(metric, storage)
    q = _queries()
    scope = idx.make_scope(_allowed(0.05))
    dist, row = idx.scan(q, nprobe=8, scope=scope)
    for kk in (1, 10, 300):
        exp_d, exp_r = _select(dist, row, kk)
        got_d, got_r = idx.scan_topk(q, kk, nprobe=8, scope=scope)
        assert torch.equal(got_r, exp_r) and torch.equal(got_d, exp_d)


def test_scan_topk_empty_and_stale_scope():
    x = _corpus(300, 16)
    idx = IVFIndex.build(x, metric="angular", storage="i8", nlist=8, seed=0)
    q = x[:3]
    d, r = idx.scan_topk(q, 5, scope=idx.make_scope([]))
    assert d.shape == (3, 5) and torch.isinf(d).all() and (r == -1).all()
    qd, qi = idx.query_topk(q, 4, scope=idx.make_scope([]))
    assert qd.shape == (3, 4) and torch.isinf(qd).all() and (qi == -1).all()
    sc = idx.make_scope(range(50))
    idx.scan_topk(q, 5, scope=sc)
    idx.remove(torch.tensor([7]))
    with pytest.raises(ValueError):
        idx.scan_topk(q, 5, scope=sc)
    with pytest.raises(ValueError):
        idx.query_topk(q, 5, scope=sc)
    with pytest.raises(ValueError):
        idx.scan_topk(q, 0)


@pytest.mark.parametrize("nprobe", [4, 32])
@pytest.mark.parametrize("metric", ["angular", "dot"])
def test_query_topk_equals_query_on_f32(metric, nprobe):
    """f32 storage: Gaussian data has no tied scan distances there, so the
    unspecified tie order of torch.topk inside query() cannot matter."""
    idx = _index(metric, "f32")
    q = _queries()
    for rerank in (True, False):
        d0, i0 = idx.query(q, k=10, nprobe=nprobe, rerank=rerank)
        d1, i1 = idx.query_topk(q, k=10, nprobe=nprobe, rerank=rerank)
        assert i1.dtype == torch.int64 and i1.shape == (6, 10)
        assert torch.equal(i0, i1)
        torch.testing.assert_close(d1, d0)
    d0, i0 = idx.query(q[0], k=10, nprobe=nprobe)
    d1, i1 = idx.query_topk(q[0], k=10, nprobe=nprobe)
    assert d1.shape == (10,) and torch.equal(i0, i1)
    sc = idx.make_scope(_allowed(0.05))
    d0, i0 = idx.query(q, k=10, nprobe=nprobe, scope=sc)
    d1, i1 = idx.query_topk(q, k=10, nprobe=nprobe, scope=sc)
    assert torch.equal(i0, i1)
    torch.testing.assert_close(d1, d0)
    # k beyond the candidates: -1 / +inf padding, as in query()
    tiny = idx.make_scope([3, 4, 5])
    d1, i1 = idx.query_topk(q, k=6, nprobe=NLIST, scope=tiny)
    assert sorted(i1[0, :3].tolist()) == [3, 4, 5]
    assert (i1[:, 3:] == -1).all() and torch.isinf(d1[:, 3:]).all()


def _brute_dist(x, metric):
    """All-pairs distances, self at +inf."""
    if metric == "angular":
        xn = x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)
        d = 1 - xn @ xn.T
    else:
        d = torch.cdist(x, x)
    d.fill_diagonal_(INF)
    return d


def _assert_is_knn(ids_row, dist_row, k, where):
    """ids_row holds the k nearest by dist_row (brute force, self at +inf).
    Two f32 evaluations of one distance differ by a few ulp of the operands'
    scale (1 for 1 - cos, the distance itself for euclidean), so a neighbour
    within 16 ulp of the k-th distance may fall on either side; anything
    clearly nearer must be present, anything clearly farther absent."""
    got = ids_row.tolist()
    assert len(set(got)) == k and all(j >= 0 for j in got), where
    kth = float(torch.kthvalue(dist_row, k).values)
    tol = 16 * 1.2e-7 * max(1.0, kth)
    assert all(float(dist_row[j]) <= kth + tol for j in got), where
    must = (dist_row < kth - tol).nonzero(as_tuple=True)[0].tolist()
    assert set(must) <= set(got), where


@pytest.mark.parametrize("metric,storage", [("angular", "f32"),
                                            ("euclidean", "f16")])
def test_knn_graph_equals_brute_force(metric, storage):
    x = _x()
    idx = _index(metric, storage)
    dists, ids = idx.knn_graph(10, nprobe=NLIST, chunk=700)   # 700 !| 3000
    assert dists.shape == (N, 10) and ids.shape == (N, 10)
    assert ids.dtype == torch.int64 and torch.isfinite(dists).all()
    assert (dists[:, 1:] >= dists[:, :-1]).all()
    own = idx.ids
    assert not (ids == own.unsqueeze(1)).any()
    bf = _brute_dist(x, metric)
    for r in range(N):
        _assert_is_knn(ids[r], bf[int(own[r])], 10, r)
    d_one, i_one = idx.knn_graph(10, nprobe=NLIST, chunk=N)
    assert torch.equal(i_one, ids)
    torch.testing.assert_close(d_one, dists)


def test_knn_graph_rows_are_query_topk_with_self_skipped():
    idx = _index("angular", "f32")
    dists, ids = idx.knn_graph(10, nprobe=4, chunk=700)
    for r in (0, 1, 699, 700, 1777, N - 1):
        d, i = idx.query_topk(idx.vectors_f32[r], 10, nprobe=4, skip_rows=[r])
        assert torch.equal(i, ids[r])
        torch.testing.assert_close(d, dists[r])
    # no f32 copy kept: queries are decoded from the packed rows per chunk
    lean = IVFIndex.build(_x()[:500], metric="angular", storage="i8", nlist=8,
                          seed=0, keep_f32=False)
    d, i = lean.knn_graph(5, nprobe=8, chunk=128)
    assert i.shape == (500, 5) and (i >= 0).all()
    assert not (i == lean.ids.unsqueeze(1)).any()


def test_knn_graph_default_nprobe_is_the_setting(monkeypatch):
    idx = _index("angular", "f32")
    monkeypatch.setattr(C, "IVF_GRAPH_NPROBE", 2)
    d_def, i_def = idx.knn_graph(5, chunk=N)
    d_two, i_two = idx.knn_graph(5, nprobe=2, chunk=N)
    assert torch.equal(i_def, i_two) and torch.equal(d_def, d_two)


def test_umap_project_with_precomputed_graph_is_identical():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(150, 16, generator=g)
    plain = projection.umap_project(x, seed=0)
    given = projection.umap_project(x, seed=0,
                                    knn=projection.knn_graph(x, 15))
    assert torch.equal(plain, given)
    with pytest.raises(ValueError):
        projection.umap_project(x, seed=0, knn=(torch.zeros(3, 2),
                                                torch.zeros(3, 2)))


def test_engine_neighbor_graph_is_in_item_ids_order():
    x = _corpus(600, 32, seed=3)
    ids = [f"t{i:04d}" for i in range(600)]
    eng = build_engine_from_matrix(x.numpy(), ids, storage="i8", nlist=16)
    # the packed order is not the item order, or this test shows nothing
    assert not torch.equal(eng.index.ids, torch.arange(600))
    pos, dists = eng.neighbor_graph(10, nprobe=16)
    assert pos.shape == (600, 10) and pos.dtype == torch.int64
    assert dists.shape == (600, 10) and torch.isfinite(dists).all()
    bf = _brute_dist(x, "angular")
    for i in range(600):
        _assert_is_knn(pos[i], bf[i], 10, i)
        assert i not in pos[i].tolist()


def _map_db(tmp_path, x):
    from audiomuse_amd.db import connect
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding

    conn = connect(f"sqlite:///{tmp_path}/map.db")
    init_db(conn)
    for i in range(x.shape[0]):
        save_track_analysis_and_embedding(
            conn, f"fp_4{'%050x' % i}", title=f"S{i}", author="A",
            embedding=x[i].numpy().astype(np.float32))
    return conn


def test_build_song_map_from_ivf_graph(tmp_path, monkeypatch):
    from audiomuse_amd.analysis import index as aindex
    from audiomuse_amd.db.store import load_index_blob

    g = torch.Generator().manual_seed(0)
    n = 240
    centers = torch.randn(4, 32, generator=g) * 6
    assign = torch.arange(n) % 4
    x = centers[assign] + torch.randn(n, 32, generator=g) * 0.3
    conn = _map_db(tmp_path, x)

    monkeypatch.setattr(C, "MAP_KNN_SOURCE", "ivf")
    calls = []
    real = aindex._ivf_map_graph

    def spy(xd, k=15):
        out = real(xd, k)
        calls.append(out)
        return out

    monkeypatch.setattr(aindex, "_ivf_map_graph", spy)
    assert aindex.build_song_map(conn) == n
    # the IVF graph was built and used (no fallback to the exact one)
    assert len(calls) == 1 and calls[0] is not None
    gd, gi = calls[0]
    assert gi.shape == (n, 15) and not (gi == torch.arange(n)[:, None]).any()
    # scattered back to input order: neighbours sit in the row's own cluster
    assert (assign[gi] == assign[:, None]).all()
    blob, meta = load_index_blob(conn, aindex.SONG_MAP)
    payload = torch.load(io.BytesIO(blob), weights_only=True)
    emb = payload["coords"]
    assert meta["n"] == n and emb.shape == (n, 2)
    assert torch.isfinite(emb).all()
    # the stored order is load order; map ids back to the synthetic rows
    rows = torch.tensor([int(s[4:], 16) for s in payload["item_ids"]])
    lab = assign[rows]
    intra, inter = [], []
    for i in range(0, n, 7):
        for j in range(1, n, 11):
            d = float((emb[i] - emb[j]).norm())
            (intra if lab[i] == lab[j] else inter).append(d)
    assert np.mean(intra) < 0.5 * np.mean(inter)

    monkeypatch.setattr(C, "MAP_KNN_SOURCE", "nonsense")
    with pytest.raises(ValueError):
        aindex.build_song_map(conn)
    conn.close()


# -- GPU: the fused scan + top-K kernel ---------------------------------------
#
# Tolerance-aware verification against the UNFUSED kernel on the same
# probes: ties and 1-ulp differences cannot fail it and cannot hide a miss.

RTOL, ATOL = 1e-4, 1e-5          # the project's scan tolerance


def _verify(top_d, top_r, ref_d, ref_r, kk, skip=None, tag=""):
    top_d, top_r = top_d.cpu(), top_r.cpu()
    ref_d, ref_r = ref_d.cpu(), ref_r.cpu()
    assert top_d.shape == top_r.shape == (ref_d.shape[0], kk)
    bit_equal = True
    for qi in range(top_d.shape[0]):
        cand = {r: d for d, r in zip(ref_d[qi].tolist(), ref_r[qi].tolist())
                if r >= 0 and (skip is None or r != int(skip[qi]))}
        rows, dists = top_r[qi].tolist(), top_d[qi].tolist()
        nfin = sum(r >= 0 for r in rows)
        # (a) distinct candidates, then nothing but (-1, +inf) padding
        got = rows[:nfin]
        assert all(r >= 0 for r in got) and len(set(got)) == nfin
        assert all(r in cand for r in got), (tag, qi)
        assert rows[nfin:] == [-1] * (kk - nfin)
        assert all(d == INF for d in dists[nfin:])
        # (b) each distance is the unfused kernel's for that row
        want = torch.tensor([cand[r] for r in got])
        have = top_d[qi, :nfin]
        torch.testing.assert_close(have, want, rtol=RTOL, atol=ATOL)
        bit_equal &= bool(torch.equal(have, want))
        # (c) non-decreasing in (distance, row), up to the tolerance
        for j in range(1, nfin):
            tol = ATOL + RTOL * abs(dists[j])
            assert dists[j] >= dists[j - 1] - tol, (tag, qi, j)
            if dists[j] == dists[j - 1]:
                assert rows[j] > rows[j - 1], (tag, qi, j)
        # (d) complete: nothing better was left behind
        assert nfin == min(kk, len(cand)), (tag, qi, nfin, len(cand))
        if nfin and nfin < len(cand):
            last = dists[nfin - 1]
            tol = ATOL + RTOL * abs(last)
            taken = set(got)
            rest = min(d for r, d in cand.items() if r not in taken)
            assert rest >= last - tol, (tag, qi, rest, last)
    return bit_equal


@pytest.mark.gpu
@pytest.mark.parametrize("kk", [1, 10, 64, 256])
@pytest.mark.parametrize("metric,storage", GPU_PAIRS)
def test_native_scan_topk_matches_unfused_scan(metric, storage, kk):
    idx = _index(metric, storage, "cuda")
    q = _queries().cuda()
    ref_d, ref_r = idx.scan(q, nprobe=8)
    top_d, top_r = idx.scan_topk(q, kk, nprobe=8)
    assert idx._topk_splits(6, 8) == 8       # small batch: split per probe
    bit = _verify(top_d, top_r, ref_d, ref_r, kk, tag=f"{metric}/{storage}")
    print(f"scan_topk {metric}/{storage} kk={kk}: distances bit-equal to "
          f"ivf_scan: {bit}")
    skip = top_r[:, 0].clone()
    sk_d, sk_r = idx.scan_topk(q, kk, nprobe=8, skip_rows=skip)
    _verify(sk_d, sk_r, ref_d, ref_r, kk, skip=skip.cpu(), tag="skip")
    scope = idx.make_scope(_allowed(0.05))
    sref_d, sref_r = idx.scan(q, nprobe=8, scope=scope)
    sc_d, sc_r = idx.scan_topk(q, kk, nprobe=8, scope=scope)
    _verify(sc_d, sc_r, sref_d, sref_r, kk, tag="scoped")


def _raw_args(idx, q):
    q_enc, q_norm = idx._prepare_queries(q)
    qt = (q_enc.to(torch.int8).view(torch.int32) if idx.storage == "i8"
          else q_enc).contiguous()
    data = idx.data.view(torch.int32) if idx.storage == "i8" else idx.data
    return qt, q_norm.contiguous(), data


def _raw_ref(idx, q, probe, scope=None):
    """The unfused kernels through the raw binding, on a given probe list
    (which may hold -1 entries)."""
    from audiomuse_amd.ops import _ext
    off = idx.cell_off if scope is None else scope.off
    counts = (off[1:] - off[:-1]).long()
    pc = torch.where(probe >= 0, counts[probe.clamp(min=0).long()],
                     torch.zeros_like(probe, dtype=torch.long))
    cand_off = torch.zeros_like(pc)
    cand_off[:, 1:] = torch.cumsum(pc, dim=1)[:, :-1]
    cap = max(int(pc.sum(dim=1).max()), 1)
    Q = probe.shape[0]
    dist = torch.full((Q, cap), INF, device="cuda")
    row = torch.full((Q, cap), -1, dtype=torch.int32, device="cuda")
    qt, q_norm, data = _raw_args(idx, q)
    code = (_DTYPE_CODE[idx.storage], _METRIC_CODE[idx.metric])
    if scope is None:
        _ext.require().ivf_scan(*code, qt, q_norm, data, idx.row_norm, probe,
                                idx.cell_off, cand_off, dist, row, idx.dim_pad)
    else:
        _ext.require().ivf_scan_sel(*code, qt, q_norm, data, idx.row_norm,
                                    probe, scope.rows, scope.off, cand_off,
                                    dist, row, idx.dim_pad)
    return dist, row


def _raw_topk(idx, q, probe, S, kk, scope=None, skip=None):
    """The fused kernel through the raw binding, its S lists merged."""
    from audiomuse_amd.ops import _ext
    Q = probe.shape[0]
    dist = torch.zeros(Q, S, kk, device="cuda")
    row = torch.zeros(Q, S, kk, dtype=torch.int32, device="cuda")
    qt, q_norm, data = _raw_args(idx, q)
    _ext.require().ivf_scan_topk(
        _DTYPE_CODE[idx.storage], _METRIC_CODE[idx.metric], qt, q_norm, data,
        idx.row_norm, probe, idx.cell_off,
        None if scope is None else scope.rows,
        None if scope is None else scope.off,
        None if skip is None else skip, dist, row, idx.dim_pad)
    # every (q, s) list is sorted and padded on its own
    d, r = dist.cpu(), row.cpu()
    fin = r >= 0
    assert ((d == INF) == ~fin).all()
    assert (d[..., 1:] >= d[..., :-1]).all()
    assert (fin[..., :-1] | ~fin[..., 1:]).all()      # padding only at the end
    return IVFIndex._ordered_select(dist.view(Q, S * kk), row.view(Q, S * kk),
                                    kk)


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 6])
@pytest.mark.parametrize("metric,storage,dim", [("angular", "i8", 20),
                                                ("angular", "f32", 33)])
def test_native_scan_topk_smallest_shapes(metric, storage, dim, Q):
    """Raw binding, n = 900 in 8 cells: every split count, a probe list
    given farthest cell first (the threshold tightens as late as possible,
    so the staging area overflows again and again), kk = 1 and kk = 256
    over all 900 candidates, a -1 probe entry, a scope with cells of 0, 1
    and 17 allowed rows, kk = the candidate count and one more."""
    n = 900
    x = _corpus(n, dim, seed=2)
    # packed on the CPU, so the layout does not depend on the device
    idx = IVFIndex.deserialize(
        IVFIndex.build(x, metric=metric, storage=storage, nlist=8,
                       seed=0).serialize(), device="cuda")
    nprobe = idx.nlist
    assert nprobe == 8
    g = torch.Generator().manual_seed(7)
    q = (x[:Q] + 0.05 * torch.randn(Q, dim, generator=g)).cuda()
    q_enc, _ = idx._prepare_queries(q)
    near = idx._rank_cells(q_enc, nprobe).contiguous()
    far = near.flip(1).contiguous()
    bits = []
    for name, probe in (("near", near), ("far", far)):
        ref_d, ref_r = _raw_ref(idx, q, probe)
        assert int((ref_r >= 0).sum(dim=1).min()) == n
        for S in (1, 3, nprobe):
            for kk in (1, 256):
                top_d, top_r = _raw_topk(idx, q, probe, S, kk)
                bits.append(_verify(top_d, top_r, ref_d, ref_r, kk,
                                    tag=f"{name} S={S} kk={kk}"))
    # skipped rows: packed rows 0 and n-1
    for edge in (0, n - 1):
        skip = torch.full((Q,), edge, dtype=torch.int32, device="cuda")
        top_d, top_r = _raw_topk(idx, q, far, 3, 256, skip=skip)
        _verify(top_d, top_r, ref_d, ref_r, 256, skip=skip.cpu(), tag="edge")
    # a -1 probe entry is skipped; more splits than live probes
    holed = far.clone()
    holed[:, 2] = -1
    ref_d, ref_r = _raw_ref(idx, q, holed)
    for S in (1, 3, nprobe):
        top_d, top_r = _raw_topk(idx, q, holed, S, 64)
        _verify(top_d, top_r, ref_d, ref_r, 64, tag=f"holed S={S}")

    # scope: cells with 17, 0, 1 and 17 allowed rows (17 = one more than a
    # pass of 16 rows), rows 0 and n-1 among them
    off = idx.cell_off.tolist()
    counts = [off[c + 1] - off[c] for c in range(nprobe)]
    first = min(c for c in range(nprobe) if counts[c])
    last = max(c for c in range(nprobe) if counts[c])
    assert counts[first] >= 17 and counts[last] >= 17
    mid = [c for c in range(first + 1, last) if counts[c] >= 4]
    c_zero, c_one = mid[0], mid[1]
    rows = torch.cat([torch.arange(0, 17),
                      torch.arange(off[c_one] + 3, off[c_one] + 4),
                      torch.arange(n - 17, n)])
    scope = idx.make_scope(idx.ids[rows.cuda()])
    sc_counts = (scope.off[1:] - scope.off[:-1]).tolist()
    assert sc_counts[first] == 17 and sc_counts[last] == 17
    assert sc_counts[c_zero] == 0 and sc_counts[c_one] == 1
    assert scope.n == 35
    ref_d, ref_r = _raw_ref(idx, q, far, scope)
    for S in (1, 3, nprobe):
        for kk in (1, 34, 35, 36, 256):       # 35 = the candidate count
            top_d, top_r = _raw_topk(idx, q, far, S, kk, scope=scope)
            _verify(top_d, top_r, ref_d, ref_r, kk,
                    tag=f"scoped S={S} kk={kk}")
    print(f"raw scan_topk {metric}/{storage} dim={dim} Q={Q}: distances "
          f"bit-equal to ivf_scan in {sum(bits)}/{len(bits)} runs")
    # the binding refuses what the kernel cannot hold
    with pytest.raises(RuntimeError):
        _raw_topk(idx, q, far, 1, 257)


@pytest.mark.gpu
def test_native_scan_topk_memory_stays_below_candidate_buffer():
    """What the feature exists for: the fused path never allocates the
    (Q, cap) f32 + i32 candidate buffer of the unfused scan."""
    idx = _index("angular", "i8", "cuda")
    g = torch.Generator().manual_seed(3)
    Q, kk = 512, 16
    q = (_x()[:Q] + 0.05 * torch.randn(Q, D, generator=g)).cuda()
    cap = N                                     # all cells probed
    unfused = Q * cap * 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    top_d, top_r = idx.scan_topk(q, kk, nprobe=NLIST)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"scan_topk peak rise {rise} B; unfused buffer {unfused} B")
    assert rise < unfused // 2
    ref_d, ref_r = idx.scan(q[:8], nprobe=NLIST)
    assert ref_d.shape == (8, cap)
    _verify(top_d[:8], top_r[:8], ref_d, ref_r, kk, tag="memory")


@pytest.mark.gpu
def test_gpu_knn_graph_matches_cpu():
    cpu = _index("angular", "f32")
    gpu = IVFIndex.deserialize(cpu.serialize(), device="cuda")
    d_c, i_c = cpu.knn_graph(10, nprobe=NLIST)
    d_g, i_g = gpu.knn_graph(10, nprobe=NLIST, chunk=700)
    assert i_g.shape == (N, 10) and torch.isfinite(d_g).all()
    assert torch.equal(i_g.sort(dim=1).values.cpu(), i_c.sort(dim=1).values)
    assert not (i_g == gpu.ids.unsqueeze(1)).any()
