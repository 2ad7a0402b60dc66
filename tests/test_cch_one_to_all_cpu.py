"""One-to-all road travel times on the CCH, CPU reference (``_rt.CCH.one_to_all``), the provider's
``reachable`` and ``POST /api/isochrones``.

* exact: the reached set equals scipy Dijkstra's, forward and reverse (reverse = Dijkstra on the
  transposed graph), finite seconds within the legs' tolerance (rtol 1e-5, atol 1e-4), metres equal
  to the pair queries' on a random-cost graph (no ties);
* provider: ranges nest, ``distance`` thresholds the metres of the time-shortest path, one-way
  streets make reverse differ from forward;
* endpoint (the committed Manila-shaped fixture): one Feature per (location, range), every reached
  node inside its MultiPolygon, cell masks nest, ``reached_nodes`` is the direct count, bad bodies
  and a haversine provider answer 400.
"""
import dataclasses
import os

import numpy as np
import pytest

from routest_amd.data.graph import synth_road_graph

rt = pytest.importorskip("routest_amd._rt")

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")


def _dijkstra(indptr, indices, cost, n, sources, reverse=False):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    A = csr_matrix((cost.astype(np.float64), indices, indptr), shape=(n, n))
    return dijkstra(A.T.tocsr() if reverse else A, directed=True, indices=np.asarray(sources))


def _check_vs_dijkstra(sec, ref, sources):
    assert (np.isfinite(ref) == np.isfinite(sec)).all()
    ok = np.isfinite(ref)
    np.testing.assert_allclose(sec[ok], ref[ok], rtol=1e-5, atol=1e-4)
    for i, s in enumerate(sources):
        assert sec[i, s] == 0


def islands_graph():
    """The one-way / two-islands graph of test_cch_cpu.py::test_one_way_streets_and_components."""
    g = synth_road_graph(3000, seed=7)
    rng = np.random.default_rng(1)
    src_of = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    keep = np.ones(g.num_edges, bool)
    drop = rng.random(g.num_edges) < 0.3
    keep &= ~(drop & (src_of < g.indices))
    mid = (g.lon.min() + g.lon.max()) / 2
    cross = (g.lon[src_of] < mid) != (g.lon[g.indices] < mid)
    keep &= ~cross
    indices = g.indices[keep].astype(np.int32)
    counts = np.bincount(src_of[keep], minlength=g.num_nodes)
    indptr = np.zeros(g.num_nodes + 1, np.int32)
    np.cumsum(counts, out=indptr[1:])
    length = g.length_m[keep].astype(np.float32)
    cost = (length / 12.0).astype(np.float32)
    gi = dataclasses.replace(g, indptr=indptr, indices=indices, length_m=length, road_class=g.road_class[keep],
                             edge_name=None if g.edge_name is None else g.edge_name[keep])
    return gi, cost


@pytest.fixture(scope="module")
def islands():
    g, cost = islands_graph()
    c = rt.CCH(g.indptr, g.indices, g.lat, g.lon, 4)
    return g, cost, c, c.customize(cost, g.length_m)


@pytest.fixture(scope="module")
def small():
    g = synth_road_graph(6000, seed=3)
    rng = np.random.default_rng(0)
    cost = (g.length_m / np.array([8.3, 12.5, 16.7, 22.2], np.float32)[g.road_class]
            * rng.uniform(0.7, 1.6, g.num_edges)).astype(np.float32)
    c = rt.CCH(g.indptr, g.indices, g.lat, g.lon, 4)
    return g, cost, c, c.customize(cost, g.length_m)


@pytest.mark.parametrize("reverse", [False, True])
def test_islands_match_dijkstra(islands, reverse):
    g, cost, c, m = islands
    sources = np.array([0, 1500, 2999], np.int32)
    sec, met = c.one_to_all(m, sources, reverse)
    assert sec.shape == met.shape == (3, g.num_nodes) and sec.dtype == met.dtype == np.float32
    _check_vs_dijkstra(sec, _dijkstra(g.indptr, g.indices, cost, g.num_nodes, sources, reverse), sources)
    assert (np.isfinite(sec) == np.isfinite(met)).all()
    reached = np.isfinite(sec).sum(axis=1)
    assert (reached > 1000).all() and (reached < 2000).all()           # one island each


def test_random_costs_match_dijkstra_and_pair_metres(small):
    g, cost, c, m = small
    sources = np.array([5, 4000], np.int32)
    sec, met = c.one_to_all(m, sources)
    _check_vs_dijkstra(sec, _dijkstra(g.indptr, g.indices, cost, g.num_nodes, sources), sources)
    assert np.isfinite(sec).all()
    rsec, rmet = c.one_to_all(m, sources, True)
    _check_vs_dijkstra(rsec, _dijkstra(g.indptr, g.indices, cost, g.num_nodes, sources, True), sources)
    allv = np.arange(g.num_nodes, dtype=np.int32)
    for i, s in enumerate(sources):
        src = np.full(g.num_nodes, s, np.int32)
        _, qmet, st, _ = c.query(m, src, allv, False)
        assert (st == 0).all()
        np.testing.assert_allclose(met[i], qmet, rtol=1e-5)
        _, qmet, st, _ = c.query(m, allv, src, False)
        np.testing.assert_allclose(rmet[i], qmet, rtol=1e-5)


def test_source_handling(islands):
    g, cost, c, m = islands
    sec, met = c.one_to_all(m, np.array([7, 2000, 7], np.int32))
    assert np.array_equal(sec[0], sec[2]) and np.array_equal(met[0], met[2])
    assert not np.array_equal(sec[0], sec[1])
    for bad in (-1, g.num_nodes):
        with pytest.raises((IndexError, ValueError)):
            c.one_to_all(m, np.array([0, bad], np.int32))
    sec, met = c.one_to_all(m, np.zeros(0, np.int32))
    assert sec.shape == (0, g.num_nodes)


def test_router_and_provider_reachable(islands, monkeypatch):
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.providers import ProviderError
    g, cost, c, m = islands
    prov = GraphProvider(g, cost, device=None, engine="cch")
    router = prov.router()
    assert isinstance(router, RoadRouter)
    nodes = [0, 2999]
    sec, met = router.one_to_all(nodes, prov.FIXED_KEY)
    rsec, rmet = c.one_to_all(m, np.array(nodes, np.int32))
    assert np.array_equal(sec, rsec) and np.array_equal(met, rmet)
    with pytest.raises(IndexError):
        router.one_to_all([g.num_nodes], prov.FIXED_KEY)
    pts = [{"lat": float(g.lat[n]), "lon": float(g.lon[n])} for n in nodes]
    ranges = [60.0, 240.0]
    out = prov.reachable(pts, ranges)
    assert [(r["point"], r["range"]) for r in out] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for i in range(2):
        lo, hi = out[2 * i], out[2 * i + 1]
        assert lo["node"] == nodes[i] and lo["value"] == 60.0
        assert 1 < lo["reached_nodes"] < hi["reached_nodes"]
        assert set(lo["nodes"].tolist()) <= set(hi["nodes"].tolist())
        assert 0 < lo["reach_m"] < hi["reach_m"]
        for r in (lo, hi):
            assert np.array_equal(r["nodes"], np.flatnonzero(sec[i] <= np.float32(r["value"])))
            assert np.array_equal(r["values"], sec[i][r["nodes"]])
    # distance: the metres of the time-shortest path, thresholded
    dist = prov.reachable(pts[:1], [800.0], range_type="distance")[0]
    assert np.array_equal(dist["nodes"], np.flatnonzero(met[0] <= np.float32(800.0)))
    assert np.array_equal(dist["values"], met[0][dist["nodes"]]) and dist["reached_nodes"] > 1
    # one-way streets: what reaches a point is not what it reaches
    fwd = prov.reachable(pts[:1], [240.0])[0]
    rev = prov.reachable(pts[:1], [240.0], reverse=True)[0]
    assert set(fwd["nodes"].tolist()) != set(rev["nodes"].tolist())
    rs, _ = router.one_to_all(nodes[:1], prov.FIXED_KEY, reverse=True)
    assert np.array_equal(rev["nodes"], np.flatnonzero(rs[0] <= np.float32(240.0)))
    with pytest.raises(ValueError):
        prov.reachable(pts, ranges, range_type="hops")
    with pytest.raises(ProviderError, match="ROUTEST_ROUTER"):
        GraphProvider(g, cost, device=None, engine="astar").reachable(pts, ranges)


# ---------------------------------------------------------------------------------------- endpoint
def _inside(ring, x, y):
    """Ray cast: is (x, y) inside the closed ring [[x, y], ...]?"""
    inside = False
    for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]):
        if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
            inside = not inside
    return inside


def _in_multipolygon(geom, x, y):
    return any(_inside(poly[0], x, y) for poly in geom["coordinates"])


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.serve.eta_service import EtaService, default_model
    env = {"ROUTEST_PROVIDER": "graph", "ROUTEST_GRAPH_PATH": os.path.join(FIX, "manila_small.edges.csv")}
    s = load_settings(env=env, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(default_model(hidden=64, steps=20), device="cpu"), store=None)
    with TestClient(create_app(sv)) as c:
        yield c, sv
    sv.close()


def test_isochrones_endpoint(client):
    from routest_amd.routing.cch import RouteContext
    from routest_amd.routing.isochrone import Grid
    c, sv = client
    g = sv.provider.g
    nodes = [100, 900]
    ranges = [600, 1200]
    body = {"locations": [[float(g.lon[n]), float(g.lat[n])] for n in nodes], "range": ranges,
            "context": {"weather": "Stormy", "traffic": "High", "pickup_time": "2025-08-29T18:00:00"}}
    r = c.post("/api/isochrones", json=body)
    assert r.status_code == 200, r.text
    fc = r.json()
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == 4
    ctx = RouteContext.from_request(body)
    sec, _ = sv.provider.router().one_to_all(nodes, ctx)
    grid = Grid(g, fc["metadata"]["cell_m"])
    masks = {}
    for k, f in enumerate(fc["features"]):
        i, j = divmod(k, 2)
        p = f["properties"]
        assert f["type"] == "Feature" and f["geometry"]["type"] == "MultiPolygon"
        assert p["group_index"] == i and p["value"] == ranges[j]
        assert p["center"] == [round(float(g.lon[nodes[i]]), 6), round(float(g.lat[nodes[i]]), 6)]
        ids = np.flatnonzero(sec[i] <= np.float32(ranges[j]))
        assert p["reached_nodes"] == len(ids) > 1 and p["reach_m"] > 0
        for n in ids:
            assert _in_multipolygon(f["geometry"], float(g.lon[n]), float(g.lat[n])), (k, int(n))
        for poly in f["geometry"]["coordinates"]:
            assert len(poly) == 1 and poly[0][0] == poly[0][-1] and len(poly[0]) >= 5     # outer ring only
        masks[(i, j)] = grid.mask(ids)
        # the polygons cover the mask's cells and nothing else: cell centres in <=> cell marked
        rows, cols = np.nonzero(masks[(i, j)])
        for rr, cc in list(zip(rows.tolist(), cols.tolist()))[::7]:
            x, y = grid.lon0 + (cc - 1.5) / grid.kx, grid.lat0 + (rr - 1.5) / grid.ky
            assert _in_multipolygon(f["geometry"], x, y)
    for i in range(2):
        assert masks[(i, 0)].sum() < masks[(i, 1)].sum()
        assert not (masks[(i, 0)] & ~masks[(i, 1)]).any()
        a, b = fc["features"][2 * i]["properties"], fc["features"][2 * i + 1]["properties"]
        assert a["reached_nodes"] < b["reached_nodes"] and a["reach_m"] < b["reach_m"]
    # destination + distance: thresholds the metres of the all-to-one paths
    body2 = dict(body, range=[3000], range_type="distance", location_type="destination")
    r = c.post("/api/isochrones", json=body2)
    assert r.status_code == 200, r.text
    _, rmet = sv.provider.router().one_to_all(nodes, ctx, reverse=True)
    got = [f["properties"]["reached_nodes"] for f in r.json()["features"]]
    assert got == [int((rmet[i] <= np.float32(3000)).sum()) for i in range(2)]


@pytest.mark.parametrize("body", [
    [],
    {},
    {"locations": [], "range": [60]},
    {"locations": [[121.0]], "range": [60]},
    {"locations": [[121.0, "x"]], "range": [60]},
    {"locations": [[121.0, 14.6]]},
    {"locations": [[121.0, 14.6]], "range": []},
    {"locations": [[121.0, 14.6]], "range": [-5]},
    {"locations": [[121.0, 14.6]], "range": ["60"]},
    {"locations": [[121.0, 14.6]], "range": list(range(1, 12))},
    {"locations": [[121.0, 14.6]] * 65, "range": [60]},
    {"locations": [[121.0, 14.6]], "range": [60], "range_type": "hops"},
    {"locations": [[121.0, 14.6]], "range": [60], "location_type": "via"},
    {"locations": [[121.0, 14.6]], "range": [60], "cell_m": 0},
    {"locations": [[121.0, 14.6]], "range": [60], "cell_m": 0.001},
])
def test_isochrones_bad_bodies(client, body):
    c, _ = client
    r = c.post("/api/isochrones", json=body)
    assert r.status_code == 400 and r.json()["error"]


def test_isochrones_need_the_graph_provider():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.serve.eta_service import EtaService
    s = load_settings(env={"ROUTEST_PROVIDER": "haversine"}, dotenv_path=None, device="cpu", route_batch="0",
                      warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/isochrones", json={"locations": [[121.0, 14.6]], "range": [60]})
        assert r.status_code == 400 and "ROUTEST_PROVIDER=graph" in r.json()["error"]
    sv.close()
