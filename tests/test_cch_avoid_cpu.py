"""Avoid areas (options.avoid_polygons, K9e) without a GPU: the mask's three implementations against
an independent oracle, request validation, context keys, the CPU router under avoid contexts against
Dijkstra on the graph without the closed edges, +inf costs in the customization, the native front
end's hand-over, the cache cap and the endpoints.  Float comparisons are on int32 views.
"""
import dataclasses
import json
import math
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import _avoid_cases as A
import _cch_graphs as G
from routest_amd import _rt
from routest_amd.routing.avoid import AvoidSet, avoid_mask, quantize
from routest_amd.routing.cch import RoadRouter, RouteContext

FIX = os.path.join(os.path.dirname(__file__), "fixtures")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def rt_mask(g, a):
    return np.asarray(_rt.avoid_mask(np.ascontiguousarray(g.indptr, dtype=np.int32),
                                     np.ascontiguousarray(g.indices, dtype=np.int32),
                                     quantize(g.lon), quantize(g.lat), a.array.astype(np.int32)))


# ---- 1. the oracle: exact rational segment intersection + winding number by summed angles ----

def _seg_meet(a, b, p, q, kinds):
    """Do the closed segments a-b and p-q share a point?  Parametric, in Fractions."""
    (ax, ay), (bx, by), (px, py), (qx, qy) = a, b, p, q
    if a == b or p == q:                                   # a point against a segment (or a point)
        pt, (s0, s1) = (a, (p, q)) if a == b else (p, (a, b))
        dx, dy = s1[0] - s0[0], s1[1] - s0[1]
        if dx == 0 and dy == 0:
            return pt == s0
        if dx * (pt[1] - s0[1]) != dy * (pt[0] - s0[0]):
            return False
        t = Fraction(pt[0] - s0[0], dx) if dx else Fraction(pt[1] - s0[1], dy)
        return 0 <= t <= 1
    rx, ry, sx, sy = bx - ax, by - ay, qx - px, qy - py
    den = rx * sy - ry * sx
    if den == 0:
        if rx * (py - ay) - ry * (px - ax) != 0:
            return False                                   # parallel, apart
        # collinear: project on a-b
        rr = rx * rx + ry * ry
        t0 = Fraction((px - ax) * rx + (py - ay) * ry, rr)
        t1 = Fraction((qx - ax) * rx + (qy - ay) * ry, rr)
        lo, hi = max(min(t0, t1), 0), min(max(t0, t1), 1)
        if lo > hi:
            return False
        kinds["collinear_overlap" if lo < hi else "touching"] += 1
        return True
    t = Fraction((px - ax) * sy - (py - ay) * sx, den)
    s = Fraction((px - ax) * ry - (py - ay) * rx, den)
    if not (0 <= t <= 1 and 0 <= s <= 1):
        return False
    if s in (0, 1) and 0 < t < 1:
        kinds["vertex_through_edge"] += 1
    elif t in (0, 1) or s in (0, 1):
        kinds["touching"] += 1
    return True


def _winding(pt, ring):
    tot = 0.0
    for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]):
        a0 = math.atan2(y0 - pt[1], x0 - pt[0])
        a1 = math.atan2(y1 - pt[1], x1 - pt[0])
        d = a1 - a0
        while d > math.pi:
            d -= 2 * math.pi
        while d <= -math.pi:
            d += 2 * math.pi
        tot += d
    return int(round(tot / (2 * math.pi)))


def oracle_closed(a, b, polygons, kinds):
    if a == b:
        kinds["zero_length"] += 1
    for poly in polygons:
        if any(v in (a, b) for ring in poly for v in ring):
            kinds["shared_vertex"] += 1
        meets = [_seg_meet(a, b, p, q, kinds) for ring in poly for p, q in zip(ring, ring[1:] + ring[:1])]
        if any(meets):
            return True
        if sum(_winding(a, ring) for ring in poly) % 2:
            return True
    return False


def test_mask_reference_runtime_and_oracle_agree_on_the_lattice():
    rng = np.random.default_rng(12)
    kinds = dict.fromkeys(["touching", "collinear_overlap", "vertex_through_edge", "zero_length", "shared_vertex"], 0)
    cases = closed_total = 0
    bx, by = 121000000, 14500000
    for _ in range(400):
        n = 6
        ox, oy = rng.integers(-6, 7, n), rng.integers(-6, 7, n)
        if rng.random() < 0.3:
            ox[1], oy[1] = ox[0], oy[0]
        src = np.arange(n - 1)
        dst = np.arange(1, n)
        g = types.SimpleNamespace(lon=(bx + ox) * 1e-6, lat=(by + oy) * 1e-6, num_nodes=n,
                                  indptr=np.concatenate([np.arange(n), [n - 1]]).astype(np.int32),
                                  indices=dst.astype(np.int32))
        assert np.array_equal(quantize(g.lon), bx + ox) and np.array_equal(quantize(g.lat), by + oy)
        polys = []
        for _p in range(int(rng.integers(1, 3))):
            rings = []
            for _r in range(int(rng.integers(1, 3))):
                while True:
                    k = int(rng.integers(3, 6))
                    ring = [(int(x), int(y)) for x, y in zip(rng.integers(-6, 7, k), rng.integers(-6, 7, k))]
                    if ring[0] != ring[-1]:
                        break
                rings.append(ring)
            polys.append(rings)
        a = AvoidSet.from_rings([[np.array([(bx + x, by + y) for x, y in r]) for r in p] for p in polys])
        ref = avoid_mask(g, a)
        assert np.array_equal(ref, rt_mask(g, a))
        pts = [(int(x), int(y)) for x, y in zip(ox, oy)]
        want = np.array([oracle_closed(pts[u], pts[v], polys, kinds) for u, v in zip(src, dst)], dtype=np.uint8)
        assert np.array_equal(ref, want), (pts, polys, ref, want)
        cases += len(src)
        closed_total += int(want.sum())
    assert cases == 2000 and 0.2 * cases < closed_total < 0.95 * cases
    assert all(v > 0 for v in kinds.values()), kinds


# ---- 2. named cases ----

@pytest.fixture(scope="module")
def ties():
    return G.ties_graph()[0]


def test_named_cases(ties):
    g = ties
    fx, fy = A.frac(g)
    masks = {}
    for name, a in A.avoid_sets(g).items():
        masks[name] = avoid_mask(g, a)
        assert np.array_equal(masks[name], rt_mask(g, a)), name
    assert masks["everything"].all() and not masks["nothing"].any()
    # direction symmetry: u -> v closed iff v -> u closed
    src = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    rev = {(int(u), int(v)): e for e, (u, v) in enumerate(zip(src, g.indices))}
    back = np.array([rev[(int(v), int(u))] for u, v in zip(src, g.indices)])
    for name, m in masks.items():
        assert np.array_equal(m, m[back]), name
    # clockwise == counter-clockwise, closed == unclosed ring
    ccw = A.box(fx(.3), fx(.6), fy(.3), fy(.6))
    sets = [AvoidSet.from_geojson({"type": "Polygon", "coordinates": [r]}) for r in (ccw, ccw[::-1], ccw[:-1])]
    assert sets[0].blob == sets[2].blob and sets[0].blob != sets[1].blob
    assert np.array_equal(avoid_mask(g, sets[0]), avoid_mask(g, sets[1]))
    # a hole opens the edges wholly inside it; the ring closes what the prototype measured
    qx, qy = quantize(g.lon).astype(np.int64), quantize(g.lat).astype(np.int64)
    hx0, hx1, hy0, hy1 = (int(quantize(v)) for v in (fx(.4), fx(.6), fy(.4), fy(.6)))
    inside = (qx > hx0) & (qx < hx1) & (qy > hy0) & (qy < hy1)
    in_hole = inside[src] & inside[g.indices]
    assert in_hole.sum() > 100 and not masks["hole"][in_hole].any()
    solid = avoid_mask(g, AvoidSet.from_geojson({"type": "Polygon", "coordinates": [A.box(fx(.3), fx(.7), fy(.3), fy(.7))]}))
    assert solid[in_hole].all() and np.array_equal(solid & ~in_hole, masks["hole"] & ~in_hole | (solid & masks["hole"]))
    # overlapping polygons: the union, not the XOR
    b1 = avoid_mask(g, AvoidSet.from_geojson({"type": "Polygon", "coordinates": [A.box(fx(.2), fx(.5), fy(.2), fy(.5))]}))
    b2 = avoid_mask(g, AvoidSet.from_geojson({"type": "Polygon", "coordinates": [A.box(fx(.4), fx(.7), fy(.4), fy(.7))]}))
    assert np.array_equal(masks["overlap"], b1 | b2) and (b1 & b2).any()
    # a sliver between two node columns holds no node and still closes the edges across it
    a = A.avoid_sets(g)["sliver"]
    (ring,), = a.rings()
    sx0, sx1 = ring[:, 0].min(), ring[:, 0].max()
    assert sx1 - sx0 == 2 and not ((qx >= sx0) & (qx <= sx1)).any()
    assert masks["sliver"].sum() >= 10


# ---- 3. validation ----

def _poly(n_rings=1, n_vert=4, x=121.0, y=14.5):
    rings = []
    for r in range(n_rings):
        t = np.linspace(0, 2 * np.pi, n_vert, endpoint=False)
        rings.append([[x + (1 + r) * 1e-3 * math.cos(v), y + (1 + r) * 1e-3 * math.sin(v)] for v in t])
    return rings


@pytest.mark.parametrize("obj", [
    5, "x", [], {"type": "Point", "coordinates": [1, 2]}, {"type": "Polygon"}, {"type": "Polygon", "coordinates": []},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [121, 14]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], ["a", 14.1]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [True, 14.1]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [181, 14.1]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [121, 90.5]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [121, float("nan")]]]},
    {"type": "Polygon", "coordinates": [[[121, 14], [121.1, 14], [float("inf"), 14]]]},
    {"type": "MultiPolygon", "coordinates": [_poly() for _ in range(65)]},
    {"type": "MultiPolygon", "coordinates": [_poly(n_rings=257, n_vert=3)]},
    {"type": "Polygon", "coordinates": _poly(n_vert=2049)},
])
def test_malformed_sets_are_refused(obj):
    with pytest.raises(ValueError) as e:
        AvoidSet.from_geojson(obj)
    assert "avoid_polygons" in str(e.value)
    with pytest.raises(ValueError):
        RouteContext.from_request({"options": {"avoid_polygons": obj}})


def test_limits_are_accepted_exactly():
    assert RouteContext.from_request({}).avoid is None
    assert RouteContext.from_request({"options": {}}).avoid is None
    assert RouteContext.from_request({"options": {"avoid_polygons": None}}).avoid is None
    a = AvoidSet.from_geojson({"type": "MultiPolygon", "coordinates": [_poly() for _ in range(64)]})
    assert a.polygons == 64
    a = AvoidSet.from_geojson({"type": "MultiPolygon", "coordinates": [_poly(n_rings=4, n_vert=3) for _ in range(64)]})
    assert int(a.array[1]) == 256
    a = AvoidSet.from_geojson({"type": "Polygon", "coordinates": _poly(n_vert=2048)})
    assert a.vertices == 2048 and a.summary() == {"polygons": 1, "vertices": 2048}
    assert hash(a) == hash(AvoidSet(a.blob, a.digest)) and 1 <= a.digest < 1 << 31
    # FNV-1a-64 over the blob's bytes, folded
    h = 0xCBF29CE484222325
    for b in a.blob:
        h = ((h ^ b) * 0x100000001B3) % (1 << 64)
    assert a.digest == ((h ^ (h >> 31) ^ (h >> 62)) & 0x7FFFFFFF or 1)


# ---- 4. keys ----

def test_context_keys(ties):
    for w, c, h in ((2, 0, 9), (255, 3, 167), (1, 2, 0)):
        assert RouteContext(w, c, h).key == (w & 0xFF) | ((c & 0xFF) << 8) | ((h & 0xFFFF) << 16)
    sets = A.avoid_sets(ties)
    a, b = sets["triangle"], sets["hole"]
    ka, kb = RouteContext(avoid=a).key, RouteContext(avoid=b).key
    assert ka != kb and ka >> 32 == a.digest and ka & 0xFFFFFFFF == RouteContext().key and ka < 1 << 63


# ---- 5. the CPU router ----

@pytest.fixture(scope="module")
def ties_router(ties):
    return RoadRouter(ties, capacity=8)


def test_forced_digest_collision_raises(ties, ties_router):
    sets = A.avoid_sets(ties)
    a, b = sets["triangle"], sets["overlap"]
    ties_router.metric(RouteContext(weekhour=1, avoid=a))
    with pytest.raises(ValueError):
        ties_router.metric(RouteContext(weekhour=1, avoid=dataclasses.replace(b, digest=a.digest)))


@pytest.mark.parametrize("graph", ["ties", "islands"])
def test_cpu_router_against_dijkstra_without_the_closed_edges(graph, ties_router):
    g = {"ties": G.ties_graph, "islands": G.islands_graph}[graph]()[0]
    router = ties_router if graph == "ties" else RoadRouter(g, capacity=8)
    a = A.avoid_sets(g)["hole"]
    ctx, base = RouteContext(avoid=a), RouteContext()
    mask = avoid_mask(g, a).astype(bool)
    src, dst = G.uniform_pairs(g, 400, seed=8)
    fx, fy = A.frac(g)
    inner = g.nearest_nodes([fy(.45), fy(.55), fy(.5)], [fx(.45), fx(.55), fx(.52)]).astype(np.int32)
    outer = g.nearest_nodes([fy(.05), fy(.95)], [fx(.05), fx(.95)]).astype(np.int32)
    src = np.concatenate([src, inner[:2], inner[:2], outer]).astype(np.int32)
    dst = np.concatenate([dst, inner[1:], outer, inner[:2]]).astype(np.int32)
    sec, met, st, paths = router.route(src, dst, ctx)
    cost = router.costs(ctx)
    router.metric(base)
    assert np.array_equal(np.isinf(cost), mask)
    assert np.array_equal(bits(cost[~mask]), bits(router.costs(base)[~mask]))
    g2, kept = A.without_edges(g, mask)
    ref = G.dijkstra_pairs(g2, cost[kept], src, dst)
    assert np.array_equal(st == 0, np.isfinite(ref))
    ok = st == 0
    np.testing.assert_allclose(sec[ok], ref[ok], rtol=1e-5, atol=1e-4)
    for p in paths:
        if len(p) > 1:
            assert not mask[A.path_edges(g, p)].any()
    if graph == "ties":
        # inside the hole: reachable from each other, cut off from the outside in both directions
        assert (st[-6:-4] == 0).all() and (st[-4:] == 1).all()
        bsec, _, bst, bpaths = router.route(src, dst, base)
        assert (bst == 0).all()
        changed = [i for i in np.flatnonzero(ok) if mask[A.path_edges(g, bpaths[i])].any()]
        assert changed and (sec[changed] >= bsec[changed]).all()
    # matrix_rect cells are the legs; one_to_all leaves out what the ring encloses
    xs, xm = router.matrix_rect(src[-8:], dst[-8:], ctx)
    for i in range(8):
        s2, m2, st2, _ = router.route(np.full(8, src[-8 + i], np.int32), dst[-8:], ctx, want_path=False)
        same = src[-8 + i] == dst[-8:]
        assert np.array_equal(bits(xs[i]), bits(np.where(same, 0, np.where(st2 == 0, s2, np.inf))))
        assert np.array_equal(bits(xm[i]), bits(np.where(same, 0, np.where(st2 == 0, m2, np.inf))))
    if graph == "ties":
        osec, _ = router.one_to_all(outer[:1], ctx)
        qx, qy = quantize(g.lon), quantize(g.lat)
        enclosed = ((qx > quantize(fx(.3))) & (qx < quantize(fx(.7))) & (qy > quantize(fy(.3))) & (qy < quantize(fy(.7))))
        assert enclosed.sum() > 500 and np.isinf(osec[0][enclosed]).all() and np.isfinite(osec[0][~enclosed]).all()


# ---- 6. customization ----

def test_inf_costs_are_absent_edges():
    """One direction of every fifth street closed: the hierarchy of the graph without those edges is
    the same (it depends on the undirected structure), so every metric array must agree, edge ids
    renumbered."""
    g, cost = G.islands_graph()
    src = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    pairs = set(zip(src.tolist(), g.indices.tolist()))
    two_way = np.array([(v, u) in pairs for u, v in zip(src.tolist(), g.indices.tolist())])
    drop = two_way & (src < g.indices) & (np.random.default_rng(2).random(g.num_edges) < 0.2)
    assert drop.sum() > 300
    c = G.cpu_cch("islands")
    cinf = cost.copy()
    cinf[drop] = np.inf
    ma = c.metric_arrays(c.customize(cinf, g.length_m, allow_inf=True))
    g2, kept = A.without_edges(g, drop)
    c2 = _rt.CCH(g2.indptr, g2.indices, g2.lat, g2.lon, 0)
    assert all(np.array_equal(c.arrays()[k], c2.arrays()[k]) for k in ("rank", "up_ptr", "up_head"))
    mb = c2.metric_arrays(c2.customize(cost[kept], g2.length_m))
    for k in ("w_up", "w_dn", "p_up", "p_dn", "len_up", "len_dn"):
        assert np.array_equal(ma[k].view(np.int32), mb[k].view(np.int32)), k
    for k in ("sub_up", "sub_dn"):
        x, y = ma[k].reshape(-1, 2), mb[k].reshape(-1, 2).copy()
        leaf = (y[:, 0] < 0) & (y[:, 1] >= 0)
        y[leaf, 1] = kept[y[leaf, 1]]
        assert np.array_equal(x, y), k
    for k in ("pay_up", "pay_dn"):
        x, y = ma[k], mb[k].copy()
        leaf = (y & 0x80000000 != 0) & (y != 0xFFFFFFFF)
        y[leaf] = (kept[y[leaf] & 0x7FFFFFFF] | 0x80000000).astype(np.uint32)
        assert np.array_equal(x, y), k
    assert (ma["pay_up"][np.isinf(ma["w_up"])] == 0xFFFFFFFF).all()      # an absent arc: PACK_INF
    assert ma["kept_f"] == mb["kept_f"] and ma["kept_b"] == mb["kept_b"]
    # finite costs: nothing changes; NaN, negative and -inf are still refused
    for bad in (np.nan, -1.0, -np.inf):
        c3 = cost.copy()
        c3[7] = bad
        with pytest.raises(ValueError):
            c.customize(c3, g.length_m, allow_inf=True)
    with pytest.raises(ValueError):                        # +inf only where the caller asks for it
        c.customize(cinf, g.length_m)


# ---- 7. native front end, cache ----

def test_native_front_end_hands_avoid_requests_to_the_app():
    body = {"source_point": {"lat": 14.5, "lon": 121.0},
            "destination_points": [{"lat": 14.6, "lon": 121.05, "payload": 1}, {"lat": 14.55, "lon": 121.02, "payload": 1}],
            "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7}}
    plain = _rt.route_optimize_cpu(json.dumps(body).encode())
    assert plain is not None and plain[0] == 200 and b'"Feature"' in plain[1]
    ring = {"type": "Polygon", "coordinates": [A.box(121.01, 121.02, 14.51, 14.52)]}
    for opt in ({"avoid_polygons": ring}, {"avoid_polygons": None}, {"avoid_polygons": 5}):
        assert _rt.route_optimize_cpu(json.dumps(dict(body, options=opt)).encode()) is None
    assert _rt.route_optimize_cpu(json.dumps(dict(body, options={})).encode()) == plain
    assert _rt.route_optimize_cpu(json.dumps(dict(body, options={"other": 1})).encode()) == plain


def test_avoid_metrics_share_a_quarter_of_the_cache(ties):
    g = ties
    router = RoadRouter(g, capacity=8)
    bases = [RouteContext(weekhour=h) for h in range(4)]
    for c in bases:
        router.metric(c)
    fx, fy = A.frac(g)
    ctxs = [RouteContext(avoid=AvoidSet.from_geojson({"type": "Polygon", "coordinates": [
        A.box(fx(.1 + .05 * i), fx(.2 + .05 * i), fy(.1), fy(.3))]})) for i in range(10)]
    for c in ctxs:
        router.metric(c)
        assert sum(router.is_cached(x) for x in ctxs) <= 2
    assert all(router.is_cached(c) for c in bases)
    assert router.is_cached(ctxs[-1]) and router.is_cached(ctxs[-2])


# ---- 8. endpoints on the CPU router ----

@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    prov = GraphProvider.from_path(os.path.join(FIX, "manila_small.edges.csv"))
    s = load_settings(env={}, dotenv_path=None, devices=[], route_batch="1", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    with TestClient(create_app(sv)) as c:
        yield c, prov.g
    sv.close()


def test_endpoints_with_a_polygon(client):
    c, g = client
    fx, fy = A.frac(g)
    ring = A.hole_geojson(g)
    opt = {"avoid_polygons": ring}
    want = {"polygons": 1, "vertices": 8}
    a = AvoidSet.from_geojson(ring)
    mask = avoid_mask(g, a).astype(bool)
    pt = lambda x, y: {"lat": fy(y), "lon": fx(x)}   # noqa: E731
    body = {"source_point": pt(.1, .1), "destination_points": [dict(pt(.9, .9), payload=1), dict(pt(.1, .9), payload=1)],
            "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7}}
    r0 = c.post("/api/optimize_route", json=body)
    r1 = c.post("/api/optimize_route", json=dict(body, options=opt))
    assert r0.status_code == 200 and r1.status_code == 200, (r0.text[:300], r1.text[:300])
    f0, f1 = r0.json(), r1.json()
    assert "avoid" not in f0["properties"] and f1["properties"]["avoid"] == want
    assert f1["type"] == "Feature" and f1["properties"]["summary"]["duration"] >= f0["properties"]["summary"]["duration"]
    coords = f1["geometry"]["coordinates"]
    nodes = g.nearest_nodes([p[1] for p in coords], [p[0] for p in coords])
    assert not any(mask[A.path_edges(g, [u, v])].any() for u, v in zip(nodes[:-1], nodes[1:]) if u != v)
    # a stop inside the hole cannot be reached
    r = c.post("/api/optimize_route", json=dict(body, options=opt, destination_points=[dict(pt(.5, .5), payload=1)]))
    assert r.status_code == 400
    # matrix: null cells to the enclosed node, the avoid object in metadata.context
    locs = [[fx(.1), fy(.1)], [fx(.9), fy(.9)], [fx(.5), fy(.5)]]
    m = c.post("/api/matrix", json={"locations": locs, "metrics": ["duration"], "options": opt})
    assert m.status_code == 200, m.text
    m = m.json()
    assert m["metadata"]["context"]["avoid"] == want
    assert m["durations"][0][2] is None and m["durations"][2][0] is None and m["durations"][0][1] > 0
    m0 = c.post("/api/matrix", json={"locations": locs, "metrics": ["duration"]}).json()
    assert "avoid" not in m0["metadata"]["context"] and m0["durations"][0][2] > 0
    # isochrones: fewer nodes reached from inside the hole
    iso = {"locations": [locs[2]], "range": [100000], "range_type": "distance"}
    i0 = c.post("/api/isochrones", json=iso).json()
    i1 = c.post("/api/isochrones", json=dict(iso, options=opt)).json()
    assert i1["metadata"]["avoid"] == want and "avoid" not in i0["metadata"]
    assert 0 < i1["features"][0]["properties"]["reached_nodes"] < i0["features"][0]["properties"]["reached_nodes"]
    # match: a trace across the ring breaks
    xs = np.linspace(.1, .9, 30)
    trace = {"traces": [{"coordinates": [[fx(v), fy(v)] for v in xs]}]}
    t0 = c.post("/api/match", json=trace)
    t1 = c.post("/api/match", json=dict(trace, options=opt))
    assert t0.status_code == 200 and t1.status_code == 200, (t0.text[:300], t1.text[:300])
    assert t1.json()["avoid"] == want and "avoid" not in t0.json()
    assert len(t1.json()["traces"][0]["matchings"]) > len(t0.json()["traces"][0]["matchings"])
    # the 400s
    for path, b in (("/api/optimize_route", body), ("/api/matrix", {"locations": locs}), ("/api/isochrones", iso),
                    ("/api/match", trace)):
        r = c.post(path, json=dict(b, options={"avoid_polygons": {"type": "Polygon", "coordinates": [[[1, 2], [3, 4]]]}}))
        assert r.status_code == 400 and "avoid_polygons" in r.json()["error"], (path, r.text)
        r = c.post(path, json=dict(b, options={"avoid_polygons": None}))
        assert r.status_code == 200, (path, r.text)


def test_batch_with_one_malformed_polygon(client):
    c, g = client
    fx, fy = A.frac(g)
    def req(i):
        return {"source_point": {"lat": fy(.1), "lon": fx(.1 + .01 * i)},
                "destination_points": [{"lat": fy(.9), "lon": fx(.9), "payload": 1}, {"lat": fy(.8), "lon": fx(.2), "payload": 1}],
                "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7}}
    reqs = [req(0), dict(req(1), options={"avoid_polygons": A.hole_geojson(g)}),
            dict(req(2), options={"avoid_polygons": {"type": "Polygon", "coordinates": [[[121, 14]]]}}), req(3)]
    r = c.post("/api/optimize_routes_batch", json={"requests": reqs})
    assert r.status_code == 200, r.text
    res = r.json()["results"]
    assert [("error" in x) for x in res] == [False, False, True, False]
    assert "avoid_polygons" in res[2]["error"] and res[1]["properties"]["avoid"] == {"polygons": 1, "vertices": 8}


def test_providers_without_contexts_answer_400():
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.providers import HaversineProvider
    body = {"source_point": {"lat": 14.5, "lon": 121.0}, "destination_points": [{"lat": 14.6, "lon": 121.05}],
            "options": {"avoid_polygons": {"type": "Polygon", "coordinates": [A.box(121.01, 121.02, 14.51, 14.52)]}}}
    out = optimize_route(body, HaversineProvider())
    assert "error" in out and "avoid_polygons" in out["error"] and "ROUTEST_PROVIDER=graph" in out["error"]
    assert "error" not in optimize_route({k: v for k, v in body.items() if k != "options"}, HaversineProvider())
