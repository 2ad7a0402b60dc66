"""Rectangular CCH matrices on the GPU (csrc/cch_query.hip rect_jobs_kernel, meet_rect_kernel;
``CchGpu.matrix_rect``, ``RoadRouter.matrix_rect`` / ``matrices_rect``, ``POST /api/matrix``) against
the CPU reference ``_rt.CCH.query`` over the S x D pairs with the output rule applied (equal nodes
0, no route +inf, cells past a row's counts 0), on the adversarial graphs of tests/_cch_graphs.py.
Every float comparison is on the int32 view, bit for bit.
"""
import os

import numpy as np
import pytest
import torch

import _cch_graphs as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRICS = ["islands", "clique_narrow", "clique_wide", "ties_ones", "ties_ints"]
KEY = {name: (1 << 40) + i for i, name in enumerate(METRICS)}
GRAPHS = {"islands": ["islands"], "clique": ["clique_narrow", "clique_wide"], "ties": ["ties_ones", "ties_ints"]}
FIX = os.path.join(os.path.dirname(__file__), "fixtures")
RAGGED = [(1, 1), (2, 64), (64, 2), (7, 65), (0, 5), (5, 0)]
INF = np.float32(np.inf)


def _graph_of(name):
    return name.split("_")[0]


@pytest.fixture(scope="module")
def model():
    from routest_amd.serve.eta_service import default_model
    return default_model(hidden=64, steps=50)


@pytest.fixture(scope="module")
def routers(model):
    from routest_amd.routing.cch import RoadRouter
    out = {}
    for graph, names in GRAPHS.items():
        r = RoadRouter(G.fixture_metrics()[names[0]][0], model, device=DEV)
        for name in names:
            r.metric_from_costs(KEY[name], G.fixture_metrics()[name][1])
        out[graph] = r
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got, want, what=""):
    for field, a, b in zip(("sec", "metres"), got, want):
        assert a.shape == b.shape and a.dtype == np.float32, (what, field, a.shape, b.shape, a.dtype)
        assert np.array_equal(_bits(a), _bits(b)), (what, field, np.argwhere(_bits(a) != _bits(b))[:8])


def _ref(name, S, D):
    """(sec, met) [S, D] of the reference with the output rule."""
    c, mc = G.cpu_metric(name)
    S, D = np.asarray(S, np.int32).reshape(-1), np.asarray(D, np.int32).reshape(-1)
    if not len(S) or not len(D):
        return np.zeros((len(S), len(D)), np.float32), np.zeros((len(S), len(D)), np.float32)
    ss, tt = np.repeat(S, len(D)), np.tile(D, len(S))
    sec, met, st, _ = c.query(mc, ss, tt, False)
    sec, met, st = np.asarray(sec), np.asarray(met), np.asarray(st)
    same = ss == tt
    shape = (len(S), len(D))
    return (np.where(same, np.float32(0), np.where(st == 0, sec, INF)).astype(np.float32).reshape(shape),
            np.where(same, np.float32(0), np.where(st == 0, met, INF)).astype(np.float32).reshape(shape))


def _gpu_rect(router, name, rows, meet=0):
    """CchGpu.matrix_rect of ragged rows [(S, D)] in ONE padded call -> (sec, met) [R, SM, DM]; the
    padding slots hold valid node ids that must not matter."""
    SM = max(1, max(len(s) for s, _ in rows))
    DM = max(1, max(len(d) for _, d in rows))
    src = np.full((len(rows), SM), 5, np.int32)
    dst = np.full((len(rows), DM), 7, np.int32)
    for r, (s, d) in enumerate(rows):
        src[r, :len(s)], dst[r, :len(d)] = s, d
    nsrc = np.array([len(s) for s, _ in rows], np.int32)
    ndst = np.array([len(d) for _, d in rows], np.int32)
    sec, met = router.gpu.matrix_rect(KEY[name], _dev(src), _dev(nsrc), _dev(dst), _dev(ndst), meet)
    return sec.cpu().numpy(), met.cpu().numpy()


def _lists(name, S, D, seed):
    """S sources and D destinations of a fixture graph: uniform draws; on islands sources 0 / 1 sit
    in the west / east half; on the clique the lowest rank (chain depth 320) is a source and a
    destination."""
    g = G.fixture_metrics()[name][0]
    src, dst = G.uniform_pairs(g, max(S, D), seed)
    src, dst = src[:S].copy(), dst[:D].copy()
    if name == "islands":
        mid = (g.lon.min() + g.lon.max()) / 2
        src[0] = np.flatnonzero(g.lon < mid)[seed]
        if S > 1:
            src[1] = np.flatnonzero(g.lon >= mid)[seed]
    if _graph_of(name) == "clique":
        low = G.cpu_cch("clique").arrays()["node"][0]
        src[0] = low
        dst[D - 1] = low
    return src, dst


# ---- 1. tile edges on every metric ----

@pytest.mark.parametrize("name", METRICS)
def test_tile_edges_equal_reference(routers, name):
    """meet_rect_kernel's tiles of 64 destinations: a single cell, a partial tile after a full one,
    one destination per source (65 workgroups of one lane), exactly one tile, and two full tiles plus
    one cell; MEET_PAIRS (meet_kernel over the same cells) gives the same bits.  islands: rows that
    are +inf throughout and rows that mix +inf with routes; clique: a chain of depth 320 (the LDS
    staging loop past 256 threads) on both sides and, on clique_narrow, nodes with more than 256 kept
    arcs; ties: the deepest meeting depth decides the metres."""
    router = routers[_graph_of(name)]
    full_inf = mixed = False
    for k, (S, D) in enumerate([(1, 1), (3, 70), (65, 1), (64, 64), (2, 129)]):
        src, dst = _lists(name, S, D, seed=20 + k)
        want = _ref(name, src, dst)
        got = _gpu_rect(router, name, [(src, dst)])
        _same([a[0] for a in got], want, (name, S, D))
        _same(_gpu_rect(router, name, [(src, dst)], meet=2), got, (name, S, D, "meet_kernel"))
        _same(router.matrix_rect(src, dst, KEY[name]), want, (name, S, D, "router"))
        rows_inf = np.isinf(want[0]).all(1)
        full_inf |= bool(rows_inf.any())
        mixed |= bool((np.isinf(want[0]).any(1) & ~rows_inf).any())
        assert np.array_equal(np.isinf(want[0]), np.isinf(want[1]))
    if name == "islands":
        assert full_inf and mixed
    else:
        assert not full_inf
    if _graph_of(name) == "clique":
        A = G.cpu_cch("clique").arrays()
        assert A["depth"][0] == G.CLIQUE_N - 1 == 320
    if name == "clique_narrow":
        d = router.gpu.metric_dump(KEY[name])
        assert np.diff(d["f_ptr"].cpu().numpy()).max() > 256 and np.diff(d["b_ptr"].cpu().numpy()).max() > 256
    if name.startswith("ties"):
        g, cost = G.fixture_metrics()[name]
        src, dst = _lists(name, 3, 70, seed=21)
        sec = router.matrix_rect(src, dst, KEY[name])[0]
        ref = G.dijkstra_pairs(g, cost, np.repeat(src, 70), np.tile(dst, 3)).reshape(3, 70)
        assert np.array_equal(sec.astype(np.float64), ref)


# ---- 2. shared and repeated nodes ----

@pytest.mark.parametrize("name", ["islands", "ties_ints"])
def test_shared_and_repeated_nodes(routers, name):
    router = routers[_graph_of(name)]
    src, dst = _lists(name, 4, 9, seed=31)
    v = int(src[2])
    dst[1] = dst[6] = v
    got = router.matrix_rect(src, dst, KEY[name])
    _same(got, _ref(name, src, dst), name)
    for a in got:
        assert _bits(a[2, 1]) == 0 and _bits(a[2, 6]) == 0            # +0.0
        assert np.array_equal(_bits(a[:, 1]), _bits(a[:, 6]))


# ---- 3. a ragged batch in one call ----

def _ragged_rows(name):
    return [_lists(name, max(S, 1), max(D, 1), seed=40 + k) for k, (S, D) in enumerate(RAGGED)]


def _cut(rows):
    return [(s[:S], d[:D]) for (s, d), (S, D) in zip(rows, RAGGED)]


@pytest.mark.parametrize("name", ["islands", "clique_wide"])
def test_ragged_batch_in_one_call(routers, name):
    router = routers[_graph_of(name)]
    rows = _cut(_ragged_rows(name))
    sec, met = _gpu_rect(router, name, rows)
    assert sec.shape == met.shape == (6, 64, 65)
    for r, (s, d) in enumerate(rows):
        single = _gpu_rect(router, name, [(s, d)])
        for whole, one in ((sec, single[0]), (met, single[1])):
            assert np.array_equal(_bits(whole[r, :len(s), :len(d)]), _bits(one[0, :len(s), :len(d)])), (name, r)
            pad = np.ones((64, 65), bool)
            pad[:len(s), :len(d)] = False
            assert (_bits(whole[r][pad]) == 0).all(), (name, r)           # exactly +0.0
        _same((sec[r, :len(s), :len(d)], met[r, :len(s), :len(d)]), _ref(name, s, d), (name, r))


# ---- 4. against the existing kernels ----

@pytest.mark.parametrize("name", ["islands", "ties_ones"])
def test_equals_square_matrix_and_route(routers, name):
    router = routers[_graph_of(name)]
    g = G.fixture_metrics()[name][0]
    L = np.random.default_rng(50).choice(g.num_nodes, 40, replace=False).astype(np.int32)
    rect = router.matrix_rect(L, L, KEY[name])
    _same(rect, router.matrix(L, KEY[name]), name + " square")
    ss, tt = np.repeat(L, 40), np.tile(L, 40)
    sec, met, st, _, _ = [t.cpu().numpy() for t in router.gpu.route(KEY[name], _dev(ss), _dev(tt), 4096, False)]
    assert set(st.tolist()) <= {0, 1}
    for a, leg in ((rect[0], sec), (rect[1], met)):
        a = a.reshape(-1)
        assert np.array_equal(_bits(a[st == 0]), _bits(leg[st == 0]))
        assert np.isinf(a[st == 1]).all()
    if name == "islands":
        assert (st == 1).sum() > 100


# ---- 5. chunking ----

@pytest.mark.parametrize("name", ["islands"])
def test_chunking_equals_unchunked(routers, name):
    """``matrices_rect`` with max_jobs = 16 (rows go to separate calls; the 64- and 65-wide rows are
    split along their destinations, the 64-source row along its sources too) and max_jobs = 1 (one
    source and one destination per call) equals the one-call answer."""
    router = routers[_graph_of(name)]
    rows = _cut(_ragged_rows(name))
    whole = router.matrices_rect(rows, KEY[name])
    assert [a.shape for a, _ in whole] == RAGGED
    calls = []
    orig = router._rect_call_gpu
    router._rect_call_gpu = lambda *a: (calls.append(tuple(a[0].shape) + tuple(a[2].shape)), orig(*a))[1]
    try:
        for mj in (16, 1):
            calls.clear()
            got = router.matrices_rect(rows, KEY[name], max_jobs=mj)
            for r, (a, b) in enumerate(zip(got, whole)):
                _same(a, b, (name, mj, r))
            assert all(c[0] * (c[1] + c[3]) <= max(mj, 2) for c in calls), (mj, calls)
            if mj == 16:
                assert any(c[1] == 2 and c[3] == 14 for c in calls)        # (2, 64): destinations split
                assert any(c[1] == 8 for c in calls)                       # (64, 2): sources split too
        # five small rows: three share a call, two the next
        small = [_lists(name, 2, 3, seed=60 + k) for k in range(5)]
        calls.clear()
        got = router.matrices_rect(small, KEY[name], max_jobs=16)
        assert [c[0] for c in calls] == [3, 2]
        for r, (s, d) in enumerate(small):
            _same(got[r], _ref(name, s, d), (name, "small", r))
    finally:
        del router._rect_call_gpu
    for r, (s, d) in enumerate(rows):
        _same(whole[r], _ref(name, s, d), (name, r))


# ---- 6. kept chains are invalidated ----

def test_matrix_rect_invalidates_kept_chains(routers):
    """PyCchGpu keeps ONE CchScratch for route / matrix / matrix_rect / legs_from_matrix, so a
    matrix_rect overwrites a matrix_keep's chains: the old tag must be refused."""
    router = routers["islands"]
    key = KEY["islands"]
    pts = _dev(np.arange(100, 106, dtype=np.int32)[None, :])
    npts = _dev([6])
    _, _, tag = router.gpu.matrix_keep(key, pts, npts)
    leg = (_dev([0]), _dev([1]), _dev([2]))
    router.gpu.legs_from_matrix(key, tag, pts, *leg, 128, True)                 # the tag is live
    router.matrix_rect([1, 2], [3, 4, 5], key)
    with pytest.raises(RuntimeError):
        router.gpu.legs_from_matrix(key, tag, pts, *leg, 128, True)


def test_out_of_range_nodes_raise(routers):
    router = routers["islands"]
    n = router.g.num_nodes
    for s, d in (([0, n], [1]), ([0], [-1])):
        with pytest.raises(IndexError):
            router.matrix_rect(s, d, KEY["islands"])


# ---- 7. the endpoint ----

def test_matrix_endpoint_on_the_gpu(model):
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.cch import RouteContext
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    prov = GraphProvider.from_path(os.path.join(FIX, "manila_small.edges.csv"), eta_model=model,
                                   device=torch.device("cuda", 0))
    g = prov.g
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    nodes = [100, 900, 17, 450, 1200, 33]
    body = {"locations": [[float(g.lon[n]) + 1e-5, float(g.lat[n])] for n in nodes], "sources": [0, 1],
            "destinations": [2, 3, 4, 5], "metrics": ["duration", "distance"],
            "context": {"weather": "Windy", "traffic": "Medium", "pickup_time": "2025-08-27T08:00:00"}}
    with TestClient(create_app(sv)) as c:
        resp = c.post("/api/matrix", json=body)
        assert resp.status_code == 200, resp.text
        out = resp.json()
    snapped = [p["node"] for p in out["sources"] + out["destinations"]]
    assert snapped == g.nearest_nodes([p[1] for p in body["locations"]], [p[0] for p in body["locations"]]).tolist()
    router = prov.router(sv.route_device)
    assert router.gpu is not None
    sec, met = router.matrix_rect(snapped[:2], snapped[2:], RouteContext.from_request(body))
    assert out["durations"] == [[float(x) for x in row] for row in sec]
    assert out["distances"] == [[float(x) for x in row] for row in met]
    assert (np.isfinite(sec) & (sec > 0)).any()
    assert out["metadata"]["engine"] == "cch"
    sv.close()
