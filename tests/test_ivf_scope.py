"""Scoped similarity search: the row selection (reference: the per-server
availability mask of paged_ivf.py) is applied inside the IVF scan, before
any top-k, so a scope that holds a small share of the catalogue still
fills k with its true nearest neighbours."""

import functools

import numpy as np
import pytest
import torch

from audiomuse_amd import config as C
from audiomuse_amd.engines.similarity import build_engine_from_matrix
from audiomuse_amd.index.ivf import IVFIndex, RowScope
from tests.test_ivf import _brute_force_ids, _corpus

PAIRS = [("angular", "i8"), ("angular", "f16"), ("angular", "f32"),
         ("euclidean", "f16"), ("dot", "f32")]
N, D, NLIST = 3000, 64, 32


@functools.lru_cache(maxsize=None)
def _x():
    return _corpus(N, D)


@functools.lru_cache(maxsize=None)
def _index(metric, storage, device="cpu"):
    """Shared read-only index; tests that mutate build their own."""
    return IVFIndex.build(_x(), metric=metric, storage=storage, nlist=NLIST,
                          device=device, seed=0)


def _queries(n=6, seed=11):
    g = torch.Generator().manual_seed(seed)
    return _x()[:n] + 0.05 * torch.randn(n, D, generator=g)


def _allowed(frac, seed=5):
    g = torch.Generator().manual_seed(seed + int(frac * 1000))
    return torch.randperm(N, generator=g)[: int(N * frac)]


# -- CPU: semantics ----------------------------------------------------------

@pytest.mark.parametrize("frac", [0.02, 0.05, 0.5])
@pytest.mark.parametrize("metric,storage", PAIRS)
def test_scoped_query_equals_brute_force_over_scope(metric, storage, frac):
    x = _x()
    idx = _index(metric, storage)
    allowed = _allowed(frac)
    scope = idx.make_scope(allowed)
    assert scope.n == allowed.numel()
    q = _queries()
    dist, ids = idx.query(q, k=10, nprobe=32, scope=scope)
    assert dist.shape == (6, 10) and ids.shape == (6, 10)
    assert torch.isfinite(dist).all()
    allowed_set = set(allowed.tolist())
    assert all(i in allowed_set for i in ids.flatten().tolist())
    local = _brute_force_ids(x[allowed], q, 10, metric)
    expect = allowed[local]
    for got, exp in zip(ids, expect):
        assert set(got.tolist()) == set(exp.tolist())


def test_empty_cells_do_not_consume_nprobe():
    idx = _index("angular", "i8")
    q = _queries()
    counts = (idx.cell_off[1:] - idx.cell_off[:-1]).long()
    # the two cells FARTHEST from query 0 among those holding >= 5 rows:
    # an unscoped nprobe=2 ranking would never reach them
    q_enc, _ = idx._prepare_queries(q[:1])
    order = idx._rank_cells(q_enc, idx.nlist)[0].long()
    far = [c for c in reversed(order.tolist()) if counts[c] >= 5][:2]
    off = idx.cell_off.tolist()
    members = torch.cat([idx.ids[off[c]:off[c + 1]] for c in far])
    scope = idx.make_scope(members)
    dist, ids = idx.query(q, k=5, nprobe=2, scope=scope)
    assert torch.isfinite(dist).all()
    member_set = set(members.tolist())
    assert all(i in member_set for i in ids.flatten().tolist())
    # the scoped ranking itself: only the two populated cells are probed
    probe = idx._rank_cells(idx._prepare_queries(q)[0], 2, scope)
    assert all(set(r.tolist()) == set(far) for r in probe)


def test_scope_edges():
    idx = _index("angular", "i8")
    q = _queries()
    # empty scope: all padding, for a batch and for a single vector
    empty = idx.make_scope([])
    assert empty.n == 0
    dist, ids = idx.query(q, k=4, scope=empty)
    assert (ids == -1).all() and torch.isinf(dist).all()
    assert dist.shape == (6, 4)
    d1, i1 = idx.query(q[0], k=4, scope=empty)
    assert i1.tolist() == [-1] * 4 and torch.isinf(d1).all()
    # single id: that id, then padding
    one = idx.make_scope([1234])
    dist, ids = idx.query(q, k=3, nprobe=32, scope=one)
    assert (ids[:, 0] == 1234).all() and (ids[:, 1:] == -1).all()
    assert torch.isfinite(dist[:, 0]).all() and torch.isinf(dist[:, 1:]).all()
    # unknown and duplicate ids are ignored
    sc = idx.make_scope([5, 5, 7, 999_999, -3, 7])
    assert sc.n == 2
    assert torch.equal(sc.rows, idx.make_scope(torch.tensor([7, 5])).rows)
    assert sc.rows.dtype == torch.int32 and sc.off.dtype == torch.int32
    assert int(sc.off[-1]) == 2 and sc.off.shape == idx.cell_off.shape
    # rows are ascending packed rows
    big = idx.make_scope(_allowed(0.5))
    assert (big.rows[1:] > big.rows[:-1]).all()


@pytest.mark.parametrize("metric,storage", PAIRS)
def test_all_ids_scope_equals_unscoped(metric, storage):
    idx = _index(metric, storage)
    q = _queries()
    full = idx.make_scope(torch.arange(N))
    assert torch.equal(full.off, idx.cell_off)
    # every cell probed: cells the build left empty rank last under a
    # scope, but hold no slots either way, so the layouts coincide. (At a
    # partial nprobe the scoped ranking skips those cells by design.)
    d0, r0 = idx.scan(q, nprobe=NLIST)
    d1, r1 = idx.scan(q, nprobe=NLIST, scope=full)
    assert torch.equal(r0, r1) and torch.equal(d0, d1)
    qd0, qi0 = idx.query(q, k=10, nprobe=NLIST)
    qd1, qi1 = idx.query(q, k=10, nprobe=NLIST, scope=full)
    assert torch.equal(qi0, qi1) and torch.equal(qd0, qd1)


def test_stale_scope_raises():
    x = _corpus(300, 16)
    idx = IVFIndex.build(x, metric="angular", storage="i8", nlist=8, seed=0)
    q = x[:2]

    def stale(scope):
        with pytest.raises(ValueError):
            idx.query(q, k=3, scope=scope)
        with pytest.raises(ValueError):
            idx.scan(q, scope=scope)
        with pytest.raises(ValueError):
            idx.max_distance(q[0], scope=scope)

    sc = idx.make_scope(range(50))
    idx.query(q, k=3, scope=sc)
    idx.add(_corpus(5, 16, seed=4), torch.arange(1000, 1005))
    stale(sc)
    sc = idx.make_scope(range(50))
    idx.query(q, k=3, scope=sc)
    idx.remove(torch.tensor([1000, 1001]))
    stale(sc)
    sc = idx.make_scope(range(50))
    idx.retrain(nlist=8, seed=1)
    stale(sc)
    # a reloaded index is another layout; so is any other index
    sc = idx.make_scope(range(50))
    back = IVFIndex.deserialize(idx.serialize())
    with pytest.raises(ValueError):
        back.query(q, k=3, scope=sc)
    # a fresh scope works again, and an even emptier one is still checked
    idx.query(q, k=3, scope=idx.make_scope(range(50)))
    with pytest.raises(ValueError):
        back.query(q, k=3, scope=RowScope(sc.rows[:0], sc.off * 0, 0,
                                          sc.version))


@pytest.mark.parametrize("metric,storage", PAIRS)
def test_scoped_max_distance(metric, storage):
    x = _x()
    idx = _index(metric, storage)
    qv = _queries()[0]
    d_all, far_all = idx.max_distance(qv)
    allowed = _allowed(0.05)
    allowed = allowed[allowed != far_all]          # exclude the global farthest
    scope = idx.make_scope(allowed)
    d_sc, far_sc = idx.max_distance(qv, scope=scope)
    xa = x[allowed]
    if metric == "angular":
        bd = 1.0 - (xa / xa.norm(dim=1, keepdim=True)) @ (qv / qv.norm())
    elif metric == "dot":
        bd = -(xa @ qv)
    else:   # the unscoped branch reports the squared distance; so does this
        bd = (xa - qv).square().sum(dim=1)
    j = int(bd.argmax())
    assert far_sc == int(allowed[j])
    assert d_sc == pytest.approx(float(bd[j]), rel=1e-5, abs=1e-6)
    assert far_sc != far_all and d_sc < d_all
    assert idx.max_distance(qv, scope=idx.make_scope([])) == (0.0, -1)


# -- CPU: engine ---------------------------------------------------------------

def _engine(calls):
    x = _corpus(600, 32, seed=3)
    ids = [f"t{i:04d}" for i in range(600)]
    tiny = ids[7::33][:18]                      # 3 % of the ids
    assert len(tiny) == 18

    def scope_fn(name):
        calls.append(name)
        return {"tiny": tiny, "ghosts": ["nope-1", "nope-2"]}.get(name, [])

    eng = build_engine_from_matrix(x.numpy(), ids, storage="i8", nlist=16,
                                   scope_fn=scope_fn)
    return eng, ids, set(tiny)


def test_engine_scoped_search_fills_n_and_caches_apart():
    calls = []
    eng, ids, tiny = _engine(calls)
    seed = ids[0]
    assert seed not in tiny
    scoped = eng.find_similar_by_id(seed, n=8, scope="tiny")
    assert len(scoped) == 8
    assert all(r["item_id"] in tiny for r in scoped)
    plain = eng.find_similar_by_id(seed, n=8)
    assert len(plain) == 8
    assert [r["item_id"] for r in plain] != [r["item_id"] for r in scoped]
    assert any(r["item_id"] not in tiny for r in plain)
    # both are now cached: neither may be served for the other
    assert eng.find_similar_by_id(seed, n=8, scope="tiny") == scoped
    assert eng.find_similar_by_id(seed, n=8) == plain
    # the other entry points take the scope too
    vec = eng.vector_for_id(seed)
    by_vec = eng.find_similar_by_vector(vec, 8, scope="tiny", exclude=(seed,))
    assert [r["item_id"] for r in by_vec] == [r["item_id"] for r in scoped]
    walked = eng.find_similar_by_vector(vec, 5, scope="tiny", radius=True)
    assert walked and all(r["item_id"] in tiny for r in walked)
    multi = eng.multi_query([vec, eng.vector_for_id(ids[1])], 6, scope="tiny")
    assert len(multi) == 6 and all(r["item_id"] in tiny for r in multi)
    # farthest track: scoped and unscoped answers differ and cache apart
    m_all = eng.max_distance_for_id(seed)
    m_sc = eng.max_distance_for_id(seed, scope="tiny")
    assert m_sc["farthest_item_id"] in tiny
    assert m_all["farthest_item_id"] not in tiny
    assert eng.max_distance_for_id(seed) == m_all
    assert eng.max_distance_for_id(seed, scope="tiny") == m_sc
    # unknown scope / scope of unknown ids: nothing to return
    assert eng.find_similar_by_id(seed, n=8, scope="nobody") == []
    assert eng.find_similar_by_id(seed, n=8, scope="ghosts") == []
    assert eng.max_distance_for_id(seed, scope="nobody")[
        "farthest_item_id"] is None


def test_engine_scope_cache_ttl_and_invalidation(monkeypatch):
    calls = []
    eng, ids, tiny = _engine(calls)
    assert C.IVF_SCOPE_CACHE_SECONDS == 30.0   # reference TTL
    now = [1000.0]
    monkeypatch.setattr(eng, "_time", lambda: now[0])
    eng.find_similar_by_id(ids[0], n=8, scope="tiny")
    assert calls == ["tiny"]
    eng.find_similar_by_id(ids[1], n=8, scope="tiny")     # result-cache miss
    assert calls == ["tiny"]
    now[0] += 29.0
    eng.find_similar_by_id(ids[2], n=8, scope="tiny")
    assert calls == ["tiny"]
    now[0] += 2.0                                           # past the TTL
    eng.find_similar_by_id(ids[2], n=8, scope="tiny")
    assert calls == ["tiny"] * 2
    eng.invalidate_scopes()
    eng.find_similar_by_id(ids[3], n=8, scope="tiny")
    assert calls == ["tiny"] * 3
    # the layout moves: the cached scope is dropped, not used stale
    eng.index.remove(torch.tensor([599]))
    out = eng.find_similar_by_id(ids[4], n=8, scope="tiny")
    assert calls == ["tiny"] * 4
    assert len(out) == 8 and all(r["item_id"] in tiny for r in out)


def test_engine_scope_without_scope_fn_is_an_error():
    x = _corpus(100, 16)
    eng = build_engine_from_matrix(x.numpy(), [str(i) for i in range(100)],
                                   nlist=4)
    with pytest.raises(ValueError):
        eng.find_similar_by_id("0", n=3, scope="tiny")


# -- GPU: the row-selection scan kernel ---------------------------------------

def _fallback_scan(idx, q, nprobe, scope, probe=None):
    """Golden: the torch fallback on the same packed data and slots."""
    q_enc, q_norm = idx._prepare_queries(q)
    if probe is None:
        probe = idx._rank_cells(q_enc, nprobe, scope)
    counts = (scope.off[1:] - scope.off[:-1]).long()
    pc = counts[probe.long()]
    cand_off = torch.zeros_like(pc)
    cand_off[:, 1:] = torch.cumsum(pc, dim=1)[:, :-1]
    cap = int(pc.sum(dim=1).max())
    dist = torch.full((q_enc.shape[0], cap), float("inf"), device=idx.device)
    row = torch.full((q_enc.shape[0], cap), -1, dtype=torch.int32,
                     device=idx.device)
    idx._scan_fallback(q_enc, q_norm, probe, cand_off, dist, row, scope=scope)
    return dist, row


GPU_PAIRS = [("angular", "i8"), ("angular", "f16"), ("euclidean", "f16"),
             ("dot", "f32"), ("angular", "f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.05, 0.5])
@pytest.mark.parametrize("metric,storage", GPU_PAIRS)
def test_native_scoped_scan_matches_fallback(metric, storage, frac):
    idx = _index(metric, storage, "cuda")
    q = _queries().cuda()
    scope = idx.make_scope(_allowed(frac))
    dist_n, row_n = idx.scan(q, nprobe=8, scope=scope)
    dist_f, row_f = _fallback_scan(idx, q, 8, scope)
    assert dist_n.shape == dist_f.shape and dist_n.shape[1] > 0
    assert torch.equal(row_n, row_f)
    torch.testing.assert_close(dist_n, dist_f, rtol=1e-4, atol=1e-5)
    allowed_rows = set(scope.rows.tolist()) | {-1}
    assert set(row_n.flatten().tolist()) <= allowed_rows


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 6])
@pytest.mark.parametrize("metric,storage,dim", [("angular", "i8", 20),
                                                ("angular", "f32", 33)])
def test_native_scoped_scan_smallest_shapes(metric, storage, dim, Q):
    """Hand-built scope: probed cells with 0, 1 and 17 allowed rows (17 =
    one more than a workgroup's 16 rows per pass), a fully allowed cell,
    and packed rows 0 and N-1."""
    n = 900
    x = _corpus(n, dim, seed=2)
    # packed on the CPU, so the cell layout the scope is cut from does not
    # depend on the device's k-means arithmetic
    idx = IVFIndex.deserialize(
        IVFIndex.build(x, metric=metric, storage=storage, nlist=8,
                       seed=0).serialize(), device="cuda")
    off = idx.cell_off.tolist()
    counts = [off[c + 1] - off[c] for c in range(len(off) - 1)]
    first = min(c for c in range(len(counts)) if counts[c])
    last = max(c for c in range(len(counts)) if counts[c])
    assert counts[first] >= 17 and counts[last] >= 17
    mid = [c for c in range(first + 1, last) if counts[c] >= 18]
    c_zero, c_one, c_full = mid[0], mid[1], mid[2]
    rows = [torch.arange(0, 17),                              # 17, has row 0
            torch.arange(off[c_one] + 3, off[c_one] + 4),     # 1
            torch.arange(off[c_full], off[c_full + 1]),       # full cell
            torch.arange(n - 17, n)]                          # 17, has row N-1
    rows = torch.cat(rows)
    scope = idx.make_scope(idx.ids[rows.cuda()])
    sc_counts = (scope.off[1:] - scope.off[:-1]).tolist()
    assert sc_counts[first] == 17 and sc_counts[last] == 17
    assert sc_counts[c_zero] == 0 and sc_counts[c_one] == 1
    assert sc_counts[c_full] == counts[c_full]
    assert int(scope.rows[0]) == 0 and int(scope.rows[-1]) == n - 1

    g = torch.Generator().manual_seed(7)
    q = (x[:Q] + 0.05 * torch.randn(Q, dim, generator=g)).cuda()
    # every cell is probed, the empty ones included
    dist_n, row_n = idx.scan(q, nprobe=idx.nlist, scope=scope)
    dist_f, row_f = _fallback_scan(idx, q, idx.nlist, scope)
    assert dist_n.shape == (Q, scope.n)
    assert torch.equal(row_n, row_f)
    torch.testing.assert_close(dist_n, dist_f, rtol=1e-4, atol=1e-5)
    assert sorted(row_n[0].tolist()) == scope.rows.tolist()
    # and with the empty cell probed explicitly in front of the others
    probe = torch.tensor([[c_zero, first, c_one, last, c_full]] * Q,
                         dtype=torch.int32, device="cuda")
    q_enc, q_norm = idx._prepare_queries(q)
    dist_f2, row_f2 = _fallback_scan(idx, q, 5, scope, probe=probe)
    pc = torch.tensor(sc_counts, device="cuda")[probe.long()]
    cand_off = torch.zeros_like(pc)
    cand_off[:, 1:] = torch.cumsum(pc, dim=1)[:, :-1]
    dist_n2 = torch.full_like(dist_f2, float("inf"))
    row_n2 = torch.full_like(row_f2, -1)
    from audiomuse_amd.index.ivf import _DTYPE_CODE, _METRIC_CODE
    from audiomuse_amd.ops import _ext
    qt = (q_enc.to(torch.int8).view(torch.int32) if storage == "i8"
          else q_enc.contiguous())
    _ext.require().ivf_scan_sel(
        _DTYPE_CODE[idx.storage], _METRIC_CODE[metric], qt.contiguous(),
        q_norm.contiguous(),
        idx.data.view(torch.int32) if storage == "i8" else idx.data,
        idx.row_norm, probe, scope.rows, scope.off, cand_off, dist_n2, row_n2,
        idx.dim_pad)
    assert torch.equal(row_n2, row_f2)
    torch.testing.assert_close(dist_n2, dist_f2, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,storage", GPU_PAIRS)
def test_native_all_ids_scope_equals_unscoped_scan(metric, storage):
    """Same rows, same lane striding, same reduce order: the scoped kernel
    is expected to reproduce the unscoped one bit for bit."""
    idx = _index(metric, storage, "cuda")
    q = _queries().cuda()
    full = idx.make_scope(torch.arange(N))
    # all cells probed, so both rankings lay the candidates out alike
    d0, r0 = idx.scan(q, nprobe=NLIST)
    d1, r1 = idx.scan(q, nprobe=NLIST, scope=full)
    assert torch.equal(r0, r1)
    print("all-ids scope: max |d_scoped - d_unscoped| =",
          float((d0 - d1).nan_to_num(posinf=0.0).abs().max()),
          "bit-equal:", bool(torch.equal(d0, d1)))
    torch.testing.assert_close(d1, d0, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_gpu_scoped_query_matches_cpu():
    q = _queries()
    allowed = _allowed(0.05)
    cpu = _index("angular", "i8")
    gpu = _index("angular", "i8", "cuda")
    _, ids_c = cpu.query(q, k=10, nprobe=32, scope=cpu.make_scope(allowed))
    d_g, ids_g = gpu.query(q.cuda(), k=10, nprobe=32,
                           scope=gpu.make_scope(allowed))
    assert torch.isfinite(d_g).all()
    assert torch.equal(ids_g.cpu(), ids_c)
