"""One-to-all road travel times on the GPU CCH (csrc/cch_all.hip) against the CPU reference
(``_rt.CCH.one_to_all``, bit for bit), scipy Dijkstra, and through ``POST /api/isochrones``.

* the one-way / two-islands graph: S = 1, 63, 64, 65, 130 sources (block padding, two and three
  blocks), forward and reverse, every schedule (a launch per depth level, fused narrow levels) —
  seconds and metres equal the reference's bits, unreachable = inf, a second call repeats them;
* the 20k graph (supernodal customization): 70 sources bit-equal, Dijkstra within the legs'
  tolerance, a routing context customized on the GPU;
* a one_to_all call leaves a matrix_keep tag usable;
* the endpoint on the GPU reaches the node sets the CPU provider reaches on the same costs.
"""
import dataclasses

import numpy as np
import pytest
import torch

from routest_amd.data.graph import synth_road_graph
from routest_amd.routing.graph import edge_costs
from routest_amd.serve.eta_service import default_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dijkstra(g, cost, sources, reverse=False):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    A = csr_matrix((cost.astype(np.float64), g.indices, g.indptr), shape=(g.num_nodes,) * 2)
    return dijkstra(A.T.tocsr() if reverse else A, directed=True, indices=np.asarray(sources))


def _check_vs_dijkstra(sec, ref):
    assert (np.isfinite(ref) == np.isfinite(sec)).all()
    ok = np.isfinite(ref)
    np.testing.assert_allclose(sec[ok], ref[ok], rtol=1e-5, atol=1e-4)


def _gpu(router, key, src, reverse=False, fuse=-1):
    sec, met = router.gpu.one_to_all(key, torch.from_numpy(np.ascontiguousarray(src, np.int32)).to(DEV), reverse, fuse)
    return sec.cpu().numpy(), met.cpu().numpy()


@pytest.fixture(scope="module")
def model():
    return default_model(hidden=64, steps=50)


@pytest.fixture(scope="module")
def islands(model):
    """The one-way / two-islands graph of test_cch_cpu.py::test_one_way_streets_and_components, its
    GPU router and the CPU reference's answers for 130 sources, forward and reverse."""
    from routest_amd import _rt
    from routest_amd.routing.cch import RoadRouter
    g = synth_road_graph(3000, seed=7)
    rng = np.random.default_rng(1)
    src_of = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    keep = np.ones(g.num_edges, bool)
    drop = rng.random(g.num_edges) < 0.3
    keep &= ~(drop & (src_of < g.indices))
    mid = (g.lon.min() + g.lon.max()) / 2
    keep &= ~((g.lon[src_of] < mid) != (g.lon[g.indices] < mid))
    indptr = np.zeros(g.num_nodes + 1, np.int32)
    np.cumsum(np.bincount(src_of[keep], minlength=g.num_nodes), out=indptr[1:])
    length = g.length_m[keep].astype(np.float32)
    g = dataclasses.replace(g, indptr=indptr, indices=g.indices[keep].astype(np.int32), length_m=length,
                            road_class=g.road_class[keep],
                            edge_name=None if g.edge_name is None else g.edge_name[keep])
    cost = (length / 12.0).astype(np.float32)
    router = RoadRouter(g, model, device=DEV)
    key = router.metric_from_costs(1 << 40, cost)
    cpu = _rt.CCH(g.indptr, g.indices, g.lat, g.lon, 0)
    mc = cpu.customize(cost, g.length_m)
    top = int(router.gpu.topology_arrays()["node"][-1])
    west, east = int(np.argmin(g.lon)), int(np.argmax(g.lon))          # one node of each island
    src = np.concatenate([[top, west, east, west], np.random.default_rng(3).integers(0, g.num_nodes, 126)]).astype(np.int32)
    ref = {rev: cpu.one_to_all(mc, src, rev) for rev in (False, True)}
    return g, router, key, src, ref


@pytest.mark.parametrize("reverse", [False, True])
def test_islands_bit_equal_to_cpu_reference(islands, reverse):
    g, router, key, src, ref = islands
    rsec, rmet = ref[reverse]
    assert not np.isfinite(rsec[1, src[2]]) and not np.isfinite(rsec[2, src[1]])     # two islands
    assert np.isinf(rsec).sum() > g.num_nodes and np.isfinite(rsec).sum() > g.num_nodes
    for S in (1, 63, 64, 65, 130):
        sec, met = _gpu(router, key, src[:S], reverse)
        assert sec.shape == (S, g.num_nodes)
        assert np.array_equal(sec, rsec[:S]), (S, reverse)
        assert np.array_equal(met, rmet[:S]), (S, reverse)
        sec2, met2 = _gpu(router, key, src[:S], reverse)
        assert np.array_equal(sec, sec2) and np.array_equal(met, met2)
    # every schedule: a launch per level, fused runs of levels up to 3 / 64 nodes wide
    for fuse in (0, 3, 64):
        sec, met = _gpu(router, key, src[:65], reverse, fuse)
        assert np.array_equal(sec, rsec[:65]) and np.array_equal(met, rmet[:65]), fuse
    # the router's numpy interface, duplicates included
    sec, met = router.one_to_all(src[:4], key, reverse=reverse)
    assert np.array_equal(sec, rsec[:4]) and np.array_equal(sec[1], sec[3]) and np.array_equal(met[1], met[3])
    with pytest.raises(Exception, match="out of range"):
        _gpu(router, key, np.array([0, g.num_nodes], np.int32), reverse)


@pytest.fixture(scope="module")
def city(model):
    from routest_amd import _rt
    from routest_amd.routing.cch import RoadRouter
    g = synth_road_graph(20_000, seed=5)
    router = RoadRouter(g, model, device=DEV)
    assert router.stats()["supernodal"]
    cost = edge_costs(g, model, device=DEV)
    key = router.metric_from_costs(1 << 40, cost)
    cpu = _rt.CCH(g.indptr, g.indices, g.lat, g.lon, 0)
    return g, router, key, cost, cpu, cpu.customize(cost, g.length_m)


def test_city_bit_equal_and_exact(city):
    g, router, key, cost, cpu, mc = city
    src = np.random.default_rng(11).integers(0, g.num_nodes, 70).astype(np.int32)
    for reverse in (False, True):
        sec, met = _gpu(router, key, src, reverse)
        rsec, rmet = cpu.one_to_all(mc, src, reverse)
        assert np.array_equal(sec, rsec) and np.array_equal(met, rmet), reverse
        _check_vs_dijkstra(sec[:3], _dijkstra(g, cost, src[:3], reverse))
        assert (sec[np.arange(70), src] == 0).all() and (met[np.arange(70), src] == 0).all()


def test_city_routing_context(city):
    from routest_amd.routing.cch import RouteContext
    g, router, key, cost, cpu, mc = city
    ctx = RouteContext.from_request({"context": {"weather": "Stormy", "traffic": "Jam",
                                                 "pickup_time": "2025-08-29T18:00:00"}})
    src = np.array([17, 9000, 19_999], np.int32)
    sec, met = router.one_to_all(src, ctx)
    ccost = router.costs(ctx)
    assert not np.array_equal(ccost, cost)
    _check_vs_dijkstra(sec, _dijkstra(g, ccost, src))
    rsec, _ = router.one_to_all(src, ctx, reverse=True)
    _check_vs_dijkstra(rsec, _dijkstra(g, ccost, src, True))


def test_matrix_tag_survives_one_to_all(city):
    g, router, key, cost, cpu, mc = city
    rng = np.random.default_rng(2)
    R, NM, Q = 20, 6, 100
    pts = torch.from_numpy(rng.integers(0, g.num_nodes, (R, NM)).astype(np.int32)).to(DEV)
    npts = torch.full((R,), NM, dtype=torch.int32, device=DEV)
    _, _, tag = router.gpu.matrix_keep(key, pts, npts)
    r = torch.from_numpy(rng.integers(0, R, Q).astype(np.int32)).to(DEV)
    i = torch.from_numpy(rng.integers(0, NM, Q).astype(np.int32)).to(DEV)
    j = torch.from_numpy(rng.integers(0, NM, Q).astype(np.int32)).to(DEV)
    before = [t.cpu() for t in router.gpu.legs_from_matrix(key, tag, pts, r, i, j, 4096, True)]
    _gpu(router, key, np.arange(70, dtype=np.int32))
    after = [t.cpu() for t in router.gpu.legs_from_matrix(key, tag, pts, r, i, j, 4096, True)]
    assert (after[2] == 0).any()
    for a, b in zip(before[:4], after[:4]):
        assert torch.equal(a, b)


def test_isochrones_endpoint_on_the_gpu(city, model):
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.cch import RouteContext
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    g, router, key, cost, cpu, mc = city
    prov = GraphProvider(g, None, device=torch.device("cuda", 0), eta_model=model)
    prov._routers[str(torch.device("cuda", 0))] = router            # the module's router (same graph and model)
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    nodes = [123, 15_000]
    body = {"locations": [[float(g.lon[n]), float(g.lat[n])] for n in nodes], "range": [600, 1800],
            "context": {"weather": "Windy", "traffic": "Medium", "pickup_time": "2025-08-27T08:00:00"}}
    with TestClient(create_app(sv)) as c:
        resp = c.post("/api/isochrones", json=body)
        assert resp.status_code == 200, resp.text
        feats = resp.json()["features"]
        assert len(feats) == 4
        ctx = RouteContext.from_request(body)
        pts = [{"lon": p[0], "lat": p[1]} for p in body["locations"]]
        on_gpu = prov.reachable(pts, body["range"], ctx=ctx)
        cpu_prov = GraphProvider(g, router.costs(ctx), device=None, engine="cch")
        on_cpu = cpu_prov.reachable(pts, body["range"])
        sec_cpu, _ = cpu_prov.router().one_to_all(nodes, cpu_prov.FIXED_KEY)
        assert len(on_gpu) == len(on_cpu) == 4
        for k, (f, a, b) in enumerate(zip(feats, on_gpu, on_cpu)):
            thr = np.float32(b["value"])
            # nodes within rounding of the threshold may fall on either side
            edge = set(np.flatnonzero(np.abs(sec_cpu[k // 2] - thr) <= 1e-5 * thr).tolist())
            assert f["properties"]["reached_nodes"] == a["reached_nodes"] > 1
            assert set(a["nodes"].tolist()) - edge == set(b["nodes"].tolist()) - edge, k
            assert abs(a["reached_nodes"] - b["reached_nodes"]) <= len(edge)
            assert f["geometry"]["type"] == "MultiPolygon" and f["geometry"]["coordinates"]
    sv.close()
