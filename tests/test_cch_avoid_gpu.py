"""Avoid areas on the GPU CCH router (csrc/cch_avoid.hip, K9e) against the numpy reference
(routing/avoid.py) and the CPU hierarchy (csrc/runtime/cch.h): the mask byte for byte, the context's
costs, the metric of +inf costs on both customization paths, every query kind bit for bit, the cache
rules, the background builder and the endpoints.  Float comparisons are on int32 views.
"""
import dataclasses
import json
import os
import time

import numpy as np
import pytest
import torch

import _avoid_cases as A
import _cch_graphs as G
from routest_amd.routing.avoid import AvoidSet, avoid_mask

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIX = os.path.join(os.path.dirname(__file__), "fixtures")
INF_BITS = np.float32(np.inf).view(np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def model():
    from routest_amd.serve.eta_service import default_model
    return default_model(hidden=64, steps=50)


@pytest.fixture(scope="module")
def graphs():
    from routest_amd.data.roads import load_graph
    return {"ties": G.ties_graph()[0], "islands": G.islands_graph()[0],
            "manila": load_graph(os.path.join(FIX, "manila_small.edges.csv"))}


@pytest.fixture(scope="module")
def routers(model, graphs):
    from routest_amd.routing.cch import RoadRouter
    return {k: RoadRouter(g, model, device=DEV) for k, g in graphs.items()}


def gpu_mask(router, avoid):
    return router.gpu.avoid_mask(torch.from_numpy(avoid.array.astype(np.int32))).cpu().numpy()


# ---- 1. the mask ----

@pytest.mark.parametrize("graph", ["ties", "islands", "manila"])
def test_mask_equals_reference(routers, graphs, graph):
    g = graphs[graph]
    if graph == "ties":
        assert g.num_edges == 27140 and g.num_edges % 64 != 0
    closed = {}
    for name, a in A.avoid_sets(g).items():
        want = avoid_mask(g, a)
        got = gpu_mask(routers[graph], a)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (graph, name, np.flatnonzero(got != want)[:8])
        closed[name] = int(want.sum())
    assert closed["everything"] == g.num_edges and closed["nothing"] == 0
    # (the islands graph has no edge across its middle band, where the sliver lies)
    assert all(closed[k] > 0 for k in A.SET_NAMES if k != "nothing" and (k, graph) != ("sliver", "islands")), closed


@pytest.mark.parametrize("E", [1, 63, 64, 65])
def test_mask_on_the_lattice(model, E):
    """Edge counts around one wave, a zero-length edge, edges collinear with ring edges."""
    from routest_amd.routing.cch import RoadRouter
    g = A.lattice_graph(E)
    a = A.lattice_set()
    want = avoid_mask(g, a)
    got = gpu_mask(RoadRouter(g, model, device=DEV), a)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert want[0] == 1                      # the zero-length edge lies on the ring's lower edge
    if E >= 63:
        assert 0 < want.sum() < E


# ---- 2. costs and metric arrays ----

def test_costs_are_the_base_costs_with_inf_where_closed(routers, graphs):
    from routest_amd.routing.cch import RouteContext
    g, router = graphs["ties"], routers["ties"]
    a = A.avoid_sets(g)["hole"]
    base = RouteContext(weather=1, congestion=2, weekhour=30)
    ctx = dataclasses.replace(base, avoid=a)
    assert ctx.key != base.key and ctx.key & 0xFFFFFFFF == base.key
    router.metric(base)
    router.metric(ctx)
    assert router.last_metric["fresh"] is True
    mask = avoid_mask(g, a).astype(bool)
    want = np.where(mask, np.float32(np.inf), router.costs(base))
    assert np.array_equal(bits(router.costs(ctx)), bits(want))
    router.metric(ctx)
    assert router.last_metric["fresh"] is False


def _assert_metric_equals_cpu(d, c, mc):
    """tests/test_cch_edges_gpu.py's comparison of a device metric with the reference's arrays."""
    T, MA = c.arrays(), c.metric_arrays(mc)
    for k in ("sub_up", "sub_dn"):
        assert np.array_equal(d[k], MA[k]), k
    for k in ("len_up", "len_dn"):
        assert np.array_equal(d[k].view(np.int32), MA[k].view(np.int32)), k
    cu, cd = G.edge_counts(MA["sub_up"], MA["sub_dn"])
    assert np.array_equal(d["cnt_up"], cu) and np.array_equal(d["cnt_dn"], cd)
    hd = T["depth"][T["up_head"]]
    for ptr, rec, w, p in (("f_ptr", "f_rec", "w_up", "p_up"), ("b_ptr", "b_rec", "w_dn", "p_dn")):
        kept = np.isfinite(MA[p]) & (MA[p] == MA[w])
        want_ptr = np.concatenate([[0], np.cumsum(np.bincount(T["arc_lo"][kept], minlength=len(T["rank"])))])
        assert np.array_equal(d[ptr], want_ptr), ptr
        arcs = np.flatnonzero(kept)
        want = np.stack([MA[p][arcs].view(np.int32), hd[arcs], arcs.astype(np.int32), np.zeros(len(arcs), np.int32)], 1)
        assert np.array_equal(d[rec].reshape(-1, 4), want), rec


@pytest.mark.parametrize("graph", ["ties", "islands"])
def test_metric_from_inf_costs_equals_cpu_on_both_paths(routers, graphs, model, monkeypatch, graph):
    """+inf costs are absent edges: the default customization (triangle table, supernodal fronts)
    and the per-level fallback (ROUTEST_CCH_TRI_GB=0) give the reference's metric arrays."""
    from routest_amd.routing.cch import RoadRouter
    g = graphs[graph]
    cost = (G.ties_graph()[2] if graph == "ties" else G.islands_graph()[1]).copy()
    cost[avoid_mask(g, A.avoid_sets(g)["hole"]).astype(bool)] = np.inf
    assert np.isinf(cost).sum() > 100
    c = G.cpu_cch(graph)
    mc = c.customize(cost, g.length_m, allow_inf=True)
    key = (1 << 40) + 77
    routers[graph].metric_from_costs(key, cost)
    assert routers[graph].stats()["triangle_table"]
    _assert_metric_equals_cpu({k: v.cpu().numpy() for k, v in routers[graph].gpu.metric_dump(key).items()}, c, mc)
    with monkeypatch.context() as mp:
        mp.setenv("ROUTEST_CCH_TRI_GB", "0")
        r2 = RoadRouter(g, model, device=DEV)
    assert not r2.stats()["triangle_table"]
    r2.metric_from_costs(key, cost)
    _assert_metric_equals_cpu({k: v.cpu().numpy() for k, v in r2.gpu.metric_dump(key).items()}, c, mc)
    for bad in (np.nan, -1.0, -np.inf):
        c2 = cost.copy()
        c2[5] = bad
        with pytest.raises(RuntimeError):
            r2.metric_from_costs(key + 1, c2)


# ---- 3. queries ----

def test_queries_under_an_avoid_context_equal_the_cpu_reference(routers, graphs):
    from routest_amd.routing.cch import RouteContext
    g, router = graphs["ties"], routers["ties"]
    a = A.avoid_sets(g)["hole"]
    base = RouteContext(weather=2, congestion=1, weekhour=50)
    ctx = dataclasses.replace(base, avoid=a)
    mask = avoid_mask(g, a).astype(bool)
    key = router.metric(ctx)
    cost = router.costs(key)
    assert np.array_equal(np.isinf(cost), mask)
    c = G.cpu_cch("ties")
    mc = c.customize(cost, g.length_m, allow_inf=True)
    src, dst = G.uniform_pairs(g, 1500, seed=4)
    src[:8] = dst[:8]
    sec, met, st, paths = router.route(src, dst, ctx)
    s2, m2, st2, p2 = c.query(mc, src, dst, True, router.max_path)
    assert np.array_equal(bits(sec), bits(s2)) and np.array_equal(bits(met), bits(m2)) and np.array_equal(st, st2)
    assert all(np.array_equal(x, y) for x, y in zip(paths, p2))
    assert (st == 1).any() and (st == 0).any()           # the hole is cut off from the outside
    for p in paths[::7]:
        if len(p) > 1:
            assert not mask[A.path_edges(g, p)].any()
    bsec, _, bst, bpaths = router.route(src, dst, base)
    assert (bst == 0).all()
    differs = [i for i in range(len(src)) if st[i] == 0 and not np.array_equal(paths[i], bpaths[i])]
    assert differs and (sec[differs] >= bsec[differs]).all()
    # matrix, matrix_rect, one_to_all
    nodes = np.unique(np.concatenate([src[:6], dst[:6]]))[:10]
    n = len(nodes)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rs, rm, rst, _ = c.query(mc, nodes[ii.ravel()].astype(np.int32), nodes[jj.ravel()].astype(np.int32), False)
    want_s = np.where(rst == 0, rs, np.inf).reshape(n, n).astype(np.float32)
    want_m = np.where(rst == 0, rm, np.inf).reshape(n, n).astype(np.float32)
    np.fill_diagonal(want_s, 0)
    np.fill_diagonal(want_m, 0)
    ms, mm = router.matrix(nodes, ctx)
    assert np.array_equal(bits(ms), bits(want_s)) and np.array_equal(bits(mm), bits(want_m))
    xs, xm = router.matrix_rect(nodes[:4], nodes[3:], ctx)
    assert np.array_equal(bits(xs), bits(want_s[:4, 3:])) and np.array_equal(bits(xm), bits(want_m[:4, 3:]))
    assert np.isinf(ms).any()
    for rev in (False, True):
        os_, om = router.one_to_all(src[:5], ctx, reverse=rev)
        ws, wm = c.one_to_all(mc, src[:5], rev)
        assert np.array_equal(bits(os_), bits(ws)) and np.array_equal(bits(om), bits(wm))
        assert np.isinf(os_).any()


# ---- 4. cache and builders ----

def test_cache_rules(graphs, model):
    from routest_amd.routing.cch import RoadRouter, RouteContext
    g = graphs["islands"]
    router = RoadRouter(g, model, device=DEV, capacity=8)
    sets = A.avoid_sets(g)
    a, b = sets["triangle"], sets["overlap"]
    ca = RouteContext(avoid=a)
    router.metric(ca)
    assert router.last_metric["fresh"] is True
    router.metric(ca)
    assert router.last_metric["fresh"] is False
    # another set under the same digest never gets the first one's metric
    with pytest.raises(ValueError):
        router.metric(RouteContext(avoid=dataclasses.replace(b, digest=a.digest)))
    # the cap: base contexts survive ten distinct sets, at most two avoid metrics stay
    bases = [RouteContext(weekhour=h) for h in range(4)]
    for c in bases:
        router.metric(c)
    fx, fy = A.frac(g)
    ctxs = [RouteContext(avoid=AvoidSet.from_geojson({"type": "Polygon", "coordinates": [
        A.box(fx(.1 + .05 * i), fx(.2 + .05 * i), fy(.1), fy(.3))]})) for i in range(10)]
    for c in ctxs:
        router.metric(c)
    assert all(router.is_cached(c) for c in bases)
    assert sum(router.is_cached(c) for c in ctxs + [ca]) == 2
    assert router.is_cached(ctxs[-1]) and router.is_cached(ctxs[-2])


def test_background_prefetch_of_an_avoid_context(graphs, model):
    from routest_amd.routing.cch import RoadRouter, RouteContext
    g = graphs["islands"]
    router = RoadRouter(g, model, device=DEV)
    a = A.avoid_sets(g)["hole"]
    ctx = RouteContext(weather=3, congestion=1, weekhour=100, avoid=a)
    assert router.prefetch(ctx)
    deadline = time.monotonic() + 30.0
    while not router.is_cached(ctx) and time.monotonic() < deadline:
        time.sleep(0.005)
    assert router.is_cached(ctx), router.stats()
    assert np.array_equal(np.isinf(router.costs(ctx)), avoid_mask(g, a).astype(bool))
    router.metric(ctx)
    assert router.last_metric["fresh"] is False


# ---- 5. endpoints ----

def _crosses(g, a, coords):
    """Does a [lon, lat] polyline over graph nodes use a closed edge?"""
    nodes = g.nearest_nodes([p[1] for p in coords], [p[0] for p in coords])
    mask = avoid_mask(g, a).astype(bool)
    hops = [(u, v) for u, v in zip(nodes[:-1], nodes[1:]) if u != v]
    return any(mask[A.path_edges(g, [u, v])].any() for u, v in hops)


def test_endpoints_with_the_gpu_router(model):
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    prov = GraphProvider.from_path(os.path.join(FIX, "manila_small.edges.csv"), eta_model=model,
                                   device=torch.device("cuda", 0))
    g = prov.g
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    fx, fy = A.frac(g)
    ring = A.hole_geojson(g)
    a = AvoidSet.from_geojson(ring)
    corner = lambda x, y: {"lat": fy(y), "lon": fx(x)}          # noqa: E731
    body = {"source_point": corner(.1, .1), "destination_points": [dict(corner(.9, .9), payload=1)],
            "options": {"avoid_polygons": ring}}
    centre = int(g.nearest_nodes([fy(.5)], [fx(.5)])[0])
    iso = {"locations": [[float(g.lon[centre]), float(g.lat[centre])]], "range": [100000], "range_type": "distance"}
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/optimize_route", json=body)
        assert r.status_code == 200, r.text
        f = r.json()
        assert f["properties"]["avoid"] == {"polygons": 1, "vertices": 8}
        assert not _crosses(g, a, f["geometry"]["coordinates"])
        r0 = c.post("/api/optimize_route", json={k: v for k, v in body.items() if k != "options"})
        assert r0.status_code == 200 and "avoid" not in r0.json()["properties"]
        assert r0.json()["properties"]["summary"]["duration"] <= f["properties"]["summary"]["duration"]
        i0 = c.post("/api/isochrones", json=iso).json()
        i1 = c.post("/api/isochrones", json=dict(iso, options={"avoid_polygons": ring})).json()
        assert i1["metadata"]["avoid"] == {"polygons": 1, "vertices": 8} and "avoid" not in i0["metadata"]
        n0, n1 = (x["features"][0]["properties"]["reached_nodes"] for x in (i0, i1))
        assert 0 < n1 < n0
        bad = c.post("/api/optimize_route", json=dict(body, options={"avoid_polygons": {"type": "Point"}}))
        assert bad.status_code == 400 and "avoid_polygons" in bad.json()["error"]
    sv.close()


def test_main_port_relays_requests_with_avoid_polygons(model):
    """The native front end does not answer avoid requests: relayed, the app's bytes, no native flush."""
    import http.client
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    from routest_amd.serve.frontend import ServingStack
    g = G.ties_graph()[0]
    prov = GraphProvider(g, None, device=torch.device("cuda", 0), eta_model=model)
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="1", route_gpu_min_stops=1, warm_scorer=False)
    sv = build_services(s, eta=EtaService(model, devices=[0]), provider=prov, store=None)
    st = ServingStack(sv, create_app(sv), model, [0], threads=2, timeout_us=300)

    def post(port, body):
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/api/optimize_route", body=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, r.read()
    try:
        fx, fy = A.frac(g)
        body = {"source_point": {"lat": fy(.1), "lon": fx(.1)},
                "destination_points": [{"lat": fy(.9), "lon": fx(.9), "payload": 1}, {"lat": fy(.2), "lon": fx(.8), "payload": 1}],
                "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7},
                "context": {"weather": "Sunny", "traffic": "Low", "pickup_time": "2025-08-26T03:00:00"},
                "options": {"avoid_polygons": A.hole_geojson(g)}}
        f0 = st.front.stats()
        a = post(st.port, body)
        b = post(st.app_server.port, body)
        f1 = st.front.stats()
        assert a[0] == 200 and a == b, (a[1][:300], b[1][:300])
        assert json.loads(a[1])["properties"]["avoid"] == {"polygons": 1, "vertices": 8}
        assert f1["relayed"] - f0["relayed"] == 1 and f1["route_flushes"] == f0["route_flushes"], (f0, f1)
    finally:
        st.close()
