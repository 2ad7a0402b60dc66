"""Edge-based map matching (routing/mapmatch_edge.py) on the CPU: the Python reference against the
host C++ (``_rt.MmEdgeGrid`` / ``_rt.mm_edge_route_cm``, csrc/runtime/map_match.h), both against
brute force, and end to end on the CPU router.  Every comparison is ``==``.

* candidates: reference == ``_rt`` == a plain-integer scan on the 3000-node graph, the islands graph
  and the hand-built tie set (two edges equidistant from a fix, both directions of one street, a
  zero-length edge, projections before the tail / beyond the head / inside, ``d2 == radius²`` kept
  and ``radius² + 1`` dropped, an edge at the 2^22 span and one 1 cm over, k above / at / below the
  edges in range); the answer does not depend on the grid's cell;
* the grid: every matchable edge is listed in each cell its box touches, ``len(items) <= 4E + cells``;
* ``edge_route_cm_ref`` == ``_rt`` == Dijkstra over the graph with the two points inserted as nodes;
* non-vacuity: 300 fixes on random edges of the 3000-node graph, radius 250 m: the node matcher
  leaves at least 20 % without a candidate (measured 29.7 %), edge mode matches all within 25 cm²;
* end to end: noise-free traces along router paths with the fixes mid-edge (query seeds 5 and 11
  with a fix on every edge, seeds 11 and 7 with one on every second edge; the streets are 15 %
  longer than their chords, so at some trace ends the model prefers a candidate at a node, seed 5
  with every second edge among them), a break across the islands cut, an unmatched fix,
  ``trips_from_traces(snap="edge")``, and ``POST /api/match`` with ``"snap"``.
"""
import os

import numpy as np
import pytest

import _mapmatch_cases as cases
import _mapmatch_edge_cases as ec
from routest_amd.routing import mapmatch as mm
from routest_amd.routing import mapmatch_edge as me
from routest_amd.routing.mapmatch import MatchParams

rt = pytest.importorskip("routest_amd._rt")

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")


def _native(nqy, nqx, edges, cell=None):
    cell = cell or me.build_edge_grid(nqy, nqx, edges)["cell"]
    return rt.MmEdgeGrid(nqy, nqx, edges["tail"], edges["head"], np.where(edges["ok"], edges["lc"], -1), cell)


def _equal(ref, got):
    for a, b in zip(ref, got):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------- candidates
@pytest.fixture(scope="module", params=["plain", "islands"])
def city(request):
    g, cost = cases.plain_graph() if request.param == "plain" else cases.islands_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    edges = me.graph_edges(g)
    rng = np.random.default_rng(0)
    on = ec.fixes_on_edges(g, rng.integers(0, g.num_edges, 60), rng.random(60))
    lat = np.concatenate([on[:, 0], rng.uniform(g.lat.min() - 0.01, g.lat.max() + 0.01, 40)])
    lon = np.concatenate([on[:, 1], rng.uniform(g.lon.min() - 0.01, g.lon.max() + 0.01, 40)])
    lat[60], lon[60] = g.lat.max() + 0.5, g.lon.mean()                    # far outside
    lat[61], lon[61] = g.lat[7], g.lon[7]                                 # exactly on a node
    py, px = mm.quantize(lat, lon)
    return g, nqy, nqx, edges, py, px


@pytest.mark.parametrize("k,radius_cm", [(1, 25_000), (8, 25_000), (16, 100_000), (3, 1), (2, 60_000)])
def test_candidates_reference_native_and_scan(city, k, radius_cm):
    g, nqy, nqx, edges, py, px = city
    ref = me.edge_candidates_ref(edges, py, px, radius_cm, k)
    _equal(ref, _native(nqy, nqx, edges).candidates(py, px, radius_cm, k))
    _equal(ref, _native(nqy, nqx, edges, cell=31_337).candidates(py, px, radius_cm, k))     # any cell, same answer
    _equal(ref, _native(nqy, nqx, edges, cell=10 ** 8).candidates(py, px, radius_cm, k))    # a single cell
    ce, cd2, cfq, nc = ref
    assert ce.dtype == np.int32 and cd2.dtype == np.int64 and cfq.dtype == np.int32 and nc.dtype == np.int32
    assert nc[60] == 0 and (ce[60] == -1).all() and (cd2[60] == -1).all() and (cfq[60] == -1).all()
    for p in range(0, 100, 7):
        want = ec.scan_one(edges, int(py[p]), int(px[p]), radius_cm, k)
        assert nc[p] == len(want)
        assert list(zip(cd2[p, :nc[p]].tolist(), ce[p, :nc[p]].tolist(), cfq[p, :nc[p]].tolist())) == want
        assert (ce[p, nc[p]:] == -1).all() and (cd2[p, nc[p]:] == -1).all() and (cfq[p, nc[p]:] == -1).all()
    if radius_cm >= 25_000:
        assert (nc[:60] >= 1).all() and (cd2[:60, 0] <= 25).all()          # the fixes placed on edges
        assert cd2[61, 0] == 0 and cfq[61, 0] in (0, me.ONE)
    if k <= 2:
        assert (nc == k).any()
    if k == 16:
        assert ((nc > 0) & (nc < k)).any()


def test_tie_set():
    nqy, nqx, edges, eid = ec.tie_edges()
    assert edges["ok"].tolist() == [e != eid[(7, 8)] for e in range(6)]
    R = 25_000
    py, px = ec.tie_fixes(R)
    nat = _native(nqy, nqx, edges)
    for k in (2, 3, 8):                       # below, at and above the three edges in range of fix 0
        ref = me.edge_candidates_ref(edges, py, px, R, k)
        _equal(ref, nat.candidates(py, px, R, k))
        ec.check_tie_answers(eid, ref, k, R)
    for p in range(len(py)):
        want = ec.scan_one(edges, int(py[p]), int(px[p]), R, 8)
        assert [w[1] for w in want] == ref[0][p, :ref[3][p]].tolist()


def test_native_argument_checks():
    nqy, nqx, edges, _ = ec.tie_edges()
    nat = _native(nqy, nqx, edges)
    for bad in ((nqy[:2], nqx[:2], 100, 17), (nqy[:2], nqx[:2], 0, 4), (nqy[:2], nqx[:3], 100, 4),
                (nqy[:2], nqx[:2], 100_001, 4)):
        with pytest.raises(ValueError):
            nat.candidates(*bad)
    with pytest.raises(ValueError):
        rt.MmEdgeGrid(nqy, nqx, edges["tail"], edges["head"][:-1], edges["lc"], 1000)
    with pytest.raises(ValueError):
        rt.MmEdgeGrid(nqy, nqx, edges["tail"], edges["head"] + 100, edges["lc"], 1000)
    with pytest.raises(ValueError):
        rt.MmEdgeGrid(nqy, nqx, edges["tail"], edges["head"], edges["lc"], 0)
    z = np.zeros((1, 2), np.int64)
    with pytest.raises(ValueError):
        rt.mm_edge_route_cm(np.zeros((1, 2, 2), np.float32), z.astype(np.int32), z, z, z[:, :1].astype(np.int32), z)


# ---------------------------------------------------------------------------------------- the grid
def _grids():
    from routest_amd.data.roads import load_edge_csv
    yield "plain", cases.plain_graph()[0]
    yield "islands", cases.islands_graph()[0]
    yield "manila_small", load_edge_csv(os.path.join(FIX, "manila_small.edges.csv"))


@pytest.mark.parametrize("name,g", list(_grids()), ids=lambda v: v if isinstance(v, str) else "")
def test_grid_lists_every_edge_in_every_cell_its_box_touches(name, g):
    nqy, nqx = mm.quantize(g.lat, g.lon)
    edges = me.graph_edges(g)
    grid = me.build_edge_grid(nqy, nqx, edges)
    E, cells = g.num_edges, grid["ny"] * grid["nx"]
    assert grid["ny"] <= 2048 and grid["nx"] <= 2048 and len(grid["start"]) == cells + 1
    assert grid["start"][-1] == len(grid["items"]) <= 4 * E + cells
    listed = set(zip(np.repeat(np.arange(cells), np.diff(grid["start"])).tolist(), grid["items"].tolist()))
    assert len(listed) == len(grid["items"])                            # no edge twice in one cell
    want = set()
    c = grid["cell"]
    for e in np.flatnonzero(edges["ok"]).tolist():
        ys = sorted((int(edges["ay"][e]), int(edges["ay"][e] + edges["wy"][e])))
        xs = sorted((int(edges["ax"][e]), int(edges["ax"][e] + edges["wx"][e])))
        for cy in range((ys[0] - grid["y0"]) // c, (ys[1] - grid["y0"]) // c + 1):
            for cx in range((xs[0] - grid["x0"]) // c, (xs[1] - grid["x0"]) // c + 1):
                want.add((cy * grid["nx"] + cx, e))
    assert listed == want
    nat = _native(nqy, nqx, edges).layout()                             # the host grid is the same listing
    assert all(nat[n] == grid[n] for n in ("y0", "x0", "cell", "ny", "nx"))
    assert np.array_equal(nat["start"], grid["start"]) and np.array_equal(nat["items"], grid["items"])


# ------------------------------------------------------------------------------ route centimetres
@pytest.mark.parametrize("costs,seed", [((1,), 0), ((1, 2, 3), 1)])
def test_route_cm_reference_native_and_dijkstra(costs, seed):
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.data.graph import build_graph
    indptr, indices, cost, length = ec.small_cost_graph(seed, costs=costs)
    n, E = len(indptr) - 1, len(indices)
    rng = np.random.default_rng(seed)
    g = build_graph(14.6 + rng.random(n) * 0.01, 121.0 + rng.random(n) * 0.01, np.repeat(np.arange(n), np.diff(indptr)),
                    indices, np.zeros(E, np.uint8), length_m=length)
    assert np.array_equal(g.indptr, indptr) and np.array_equal(g.indices, indices) and np.array_equal(g.length_m, length)
    router = RoadRouter(g, None, device=None)
    key = router.metric_from_costs(1 << 40, cost)
    lc = np.rint(length.astype(np.float64) * 100).astype(np.int64)
    tail = np.repeat(np.arange(n), np.diff(indptr)).astype(np.int32)
    rng = np.random.default_rng(seed)
    K, rows = 8, 40
    e1 = rng.integers(0, E, (rows, K)).astype(np.int32)
    e2 = rng.integers(0, E, (rows, K)).astype(np.int32)
    twin = {(int(tail[e]), int(indices[e])): e for e in range(E)}
    for r in range(rows):
        e2[r, 0] = e1[r, 0]                                               # same edge, forward or backward
        e2[r, 1] = e1[r, 1]
        back = twin.get((int(indices[e1[r, 2]]), int(tail[e1[r, 2]])))
        if back is not None:
            e2[r, 2] = back                                               # the U-turn pair
    e1[:, 7], e2[:, 6] = -1, -1                                           # padding
    e1[:5, 3] = twin[(n - 1, 0)]                                          # from the edge out of the dead-end node: fine
    e2[:5, 4] = twin[(n - 1, 0)]                                          # onto it: nothing reaches its tail
    fq1, fq2 = rng.integers(0, me.ONE + 1, (rows, K)), rng.integers(0, me.ONE + 1, (rows, K))
    fq2[:, 1] = fq1[:, 1]                                                 # same edge, same point: 0
    l1, l2 = lc[np.maximum(e1, 0)], lc[np.maximum(e2, 0)]
    o1, o2 = me.edge_offsets(l1, fq1), me.edge_offsets(l2, fq2)
    import torch
    hd, tl = indices[np.maximum(e1, 0)], tail[np.maximum(e2, 0)]
    cnt = torch.full((rows,), K, dtype=torch.int32)
    _, met = router.rect_rows(torch.from_numpy(hd.astype(np.int32)), cnt, torch.from_numpy(tl), cnt, key)
    met = met.numpy()
    ref = me.edge_route_cm_ref(met, e1, o1, l1, e2, o2)
    nat = rt.mm_edge_route_cm(met, e1, o1, l1, e2, o2)
    assert ref.dtype == nat.dtype == np.int64 and ref.shape == (rows, K, K) and np.array_equal(ref, nat)
    seen = {"fwd": 0, "back": 0, "uturn": 0, "none": 0, "pad": 0}
    for r in range(rows):
        for i in range(K):
            for j in range(K):
                a, b = int(e1[r, i]), int(e2[r, j])
                if a < 0 or b < 0:
                    assert ref[r, i, j] == -1
                    seen["pad"] += 1
                    continue
                want = ec.brute_route_cm(indptr, indices, lc, a, int(o1[r, i]), b, int(o2[r, j]))
                assert ref[r, i, j] == want, (r, i, j, a, b)
                seen["fwd"] += a == b and o2[r, j] >= o1[r, i]
                seen["back"] += a == b and o2[r, j] < o1[r, i]
                seen["uturn"] += a != b and indices[a] == tail[b] and indices[b] == tail[a]
                seen["none"] += want == -1
    assert all(v > 0 for v in seen.values()), seen
    assert (ref[np.arange(rows), 1, 1] == 0).all()


# ------------------------------------------------------------------------------------ non-vacuity
def test_edge_mode_matches_what_the_node_matcher_loses():
    g, _ = cases.plain_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    rng = np.random.default_rng(0)
    f = ec.fixes_on_edges(g, rng.integers(0, g.num_edges, 300), rng.random(300))
    py, px = mm.quantize(f[:, 0], f[:, 1])
    p = MatchParams()
    assert p.radius_cm == 25_000
    node_nc = mm.candidates_ref(nqy, nqx, py, px, p.radius_cm, p.k)[2]
    share = float((node_nc == 0).mean())
    print("node matcher: share of fixes without a candidate", share)
    assert share >= 0.20
    _, cd2, _, nc = me.edge_candidates_ref(me.graph_edges(g), py, px, p.radius_cm, p.k)
    print("edge mode: unmatched", int((nc == 0).sum()), "largest cm2 to the own edge", int(cd2[:, 0].max()))
    assert (nc >= 1).all() and (cd2[:, 0] <= 25).all()


# ------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def world():
    from routest_amd.routing.graph import GraphProvider
    g, cost = cases.plain_graph()
    prov = GraphProvider(g, cost, device=None, engine="cch")
    return g, cost, prov, prov.router()


def _is_edge(g, a, b):
    lo, hi = g.indptr[a], g.indptr[a + 1]
    j = lo + int(np.searchsorted(g.indices[lo:hi], b))
    return j < hi and g.indices[j] == b


@pytest.mark.parametrize("seed,every", [(5, 1), (11, 1), (11, 2), (7, 2)])
def test_end_to_end_distance_is_the_true_path(world, seed, every):
    from routest_amd.data.graph import synth_route_queries
    g, cost, prov, router = world
    edges = me.graph_edges(g)
    lc = edges["lc"]
    s, t = synth_route_queries(g, 6, seed=seed, min_km=3.0, max_km=8.0)
    _, _, st, paths = router.route(s, t, prov.FIXED_KEY)
    assert (st == 0).all()
    tr = [ec.fixes_along(g, p, 0.5, every) for p in paths]
    res = me.match_traces_edge(router, g, [x[0] for x in tr], prov.FIXED_KEY, MatchParams())
    c64 = np.asarray(router.costs(prov.FIXED_KEY), dtype=np.float64)
    for r, (fx, on, all_e), p in zip(res, tr, paths):
        assert (r["edge"] == on).all() and (r["cand_d2"] <= 25).all() and (r["cand_d2"] >= 0).all()
        assert r["n_segments"] == 1 and len(r["matchings"]) == 1 and (r["matching"] == 0).all()
        assert (np.abs(r["fq"] - me.ONE // 2) <= 2).all()
        m = r["matchings"][0]
        off = me.edge_offsets(lc[r["edge"]], r["fq"])
        last = len(all_e) - 1 - (len(all_e) - 1) % every
        true_cm = int(lc[on[0]] - off[0] + lc[all_e[1:last]].sum() + off[-1])
        steps = len(on) - 1
        print("distance cm", m["distance"] * 100.0, "true", true_cm, "steps", steps)
        assert abs(m["distance"] * 100.0 - true_cm) <= steps
        # the nodes passed are the path's inner nodes: from the head of the first edge to the tail of the last
        assert m["nodes"].tolist() == [int(v) for v in p[1:last + 1]]
        assert all(_is_edge(g, int(a), int(b)) for a, b in zip(m["nodes"][:-1], m["nodes"][1:]))
        true_s = c64[on[0]] * (me.ONE - r["fq"][0]) / me.ONE + c64[all_e[1:last]].sum() + c64[on[-1]] * r["fq"][-1] / me.ONE
        assert abs(m["duration"] - true_s) <= 1e-4 * true_s
        assert np.array_equal(m["start"], r["proj"][0]) and np.array_equal(m["end"], r["proj"][-1])
        assert me.node_path(g, r, 0).tolist() == [int(v) for v in p[:last + 2]]


def test_one_edge_and_backwards_on_it(world):
    """A trace that stays on one edge passes no node; one that goes back on it drives round."""
    g, cost, prov, router = world
    e = 1000
    fwd = ec.fixes_on_edges(g, np.array([e, e, e]), np.array([0.2, 0.5, 0.9]))
    r = me.match_traces_edge(router, g, [fwd], prov.FIXED_KEY)[0]
    # both directions of the street are equally near; whichever is chosen, the trace stays on it
    assert r["n_segments"] == 1 and len(set(r["edge"].tolist())) == 1 and len(r["matchings"][0]["nodes"]) == 0
    lc = int(me.graph_edges(g)["lc"][r["edge"][0]])
    off = me.edge_offsets(lc, r["fq"])
    assert r["matchings"][0]["distance"] * 100.0 == float(off[-1] - off[0]) and abs(off[-1] - off[0] - 0.7 * lc) <= 2
    c = float(router.costs(prov.FIXED_KEY)[r["edge"][0]])
    assert abs(r["matchings"][0]["duration"] - 0.7 * c) <= 1e-3 * c


def test_break_across_the_cut_and_an_unmatched_fix():
    from routest_amd.routing.cch import RoadRouter
    g, cost = cases.islands_graph()
    router = RoadRouter(g, None, device=None)
    key = router.metric_from_costs(1 << 40, cost)
    f, nodes, n_west = cases.cross_cut_trace(g, router, key)
    f = np.concatenate([f, f[-1:]])
    f[-1] = (g.lat.max() + 0.05, f[-1, 1])                               # 5 km north of everything
    r = me.match_traces_edge(router, g, [f], key)[0]
    assert (r["edge"][:-1] >= 0).all() and r["edge"][-1] == -1 and r["fq"][-1] == -1 and r["cand_d2"][-1] == -1
    assert r["segment"][-1] == -1 and r["matching"][-1] == -1
    assert r["n_segments"] >= 2 and len(r["matchings"]) == r["n_segments"]
    assert r["segment"][n_west - 1] + 1 == r["segment"][n_west]
    mid = (g.lon.min() + g.lon.max()) / 2
    tail = me.graph_edges(g)["tail"]
    for q, mt in enumerate(r["matchings"]):
        side = g.lon[mt["nodes"]] < mid
        assert side.all() or not side.any()
        assert all(_is_edge(g, int(a), int(b)) for a, b in zip(mt["nodes"][:-1], mt["nodes"][1:]))
        fixes = np.flatnonzero(r["matching"] == q)
        assert (r["segment"][fixes] == mt["segment"]).all()
        assert ((g.lon[tail[r["edge"][fixes]]] < mid) == (fixes < n_west)).all()


def test_python_fallback_equals_native(world, monkeypatch):
    g, cost, prov, router = world
    from routest_amd.data.graph import synth_route_queries
    s, t = synth_route_queries(g, 3, seed=5, min_km=3.0, max_km=8.0)
    _, _, _, paths = router.route(s, t, prov.FIXED_KEY)
    fixes = [ec.fixes_along(g, p, 0.3)[0] for p in paths]
    want = me.match_traces_edge(router, g, fixes, prov.FIXED_KEY)
    from routest_amd.ops import _ext
    real = _ext.runtime
    monkeypatch.setattr(_ext, "runtime", lambda required=True: None if not required else real(required))
    monkeypatch.setattr(g, "_mm_edge_host", None, raising=False)
    got = me.match_traces_edge(router, g, fixes, prov.FIXED_KEY)
    monkeypatch.setattr(g, "_mm_edge_host", None, raising=False)
    for a, b in zip(want, got):
        for n in ("edge", "fq", "proj", "cand_d2", "segment", "matching"):
            assert np.array_equal(a[n], b[n])
        assert [(m["nodes"].tolist(), m["distance"], m["duration"]) for m in a["matchings"]] == \
               [(m["nodes"].tolist(), m["distance"], m["duration"]) for m in b["matchings"]]


def test_trips_from_traces_edge_mode(world):
    from routest_amd.data.graph import synth_route_queries
    from routest_amd.models.gcn_observed import TripWorld, trips_from_traces
    g, cost, prov, router = world
    s, t = synth_route_queries(g, 6, seed=5, min_km=3.0, max_km=8.0)
    _, _, _, paths = router.route(s, t, prov.FIXED_KEY)
    fixes = [ec.fixes_along(g, p, 0.5)[0] for p in paths]
    fixes[1] = cases.with_unmatched_fix(g, fixes[1], 0)
    seconds = [100.0 + i for i in range(6)]
    trips, dropped = trips_from_traces(prov, fixes, seconds, snap="edge")
    assert dropped == [1] and [sec for _, sec in trips] == [seconds[i] for i in (0, 2, 3, 4, 5)]
    assert [p for p, _ in trips] == [[int(v) for v in paths[i]] for i in (0, 2, 3, 4, 5)]
    assert (TripWorld(g, cost, seed=0).edge_seconds([p for p, _ in trips]) > 0).all()      # raises on a non-edge step
    # mid-edge fixes are mostly beyond the node matcher's radius: it keeps fewer of these traces
    assert len(trips_from_traces(prov, fixes, seconds)[0]) < len(trips)
    with pytest.raises(ValueError):
        trips_from_traces(prov, fixes, seconds, snap="way")
    with pytest.raises(ValueError):
        prov.match(fixes, snap="way")


# ---------------------------------------------------------------------------------------- endpoint
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


CTX_BODY = {"context": {"weather": "Stormy", "traffic": "High", "pickup_time": "2025-08-29T18:00:00"}}


def _bodies(sv):
    from routest_amd.routing.cch import RouteContext
    g = sv.provider.g
    ctx = RouteContext.from_request(CTX_BODY)
    _, _, st, paths = sv.provider.router().route([100, 900], [400, 300], ctx)
    assert (st == 0).all()
    mid = [ec.fixes_along(g, p, 0.5)[0] for p in paths]
    mid[1][1] = (float(g.lat.max()) + 0.05, mid[1][1, 1])                            # an unmatched fix
    coords = [[[float(lo), float(la)] for la, lo in f] for f in mid]
    return ctx, mid, dict(CTX_BODY, traces=[{"coordinates": co} for co in coords], radius=200, k=6)


def test_snap_absent_answers_the_node_matcher_bytes(client):
    c, sv = client
    g = sv.provider.g
    ctx, mid, body = _bodies(sv)
    r = c.post("/api/match", json=body)
    assert r.status_code == 200, r.text
    assert c.post("/api/match", json=dict(body, snap="node")).content == r.content
    # the answer rebuilt from the node matcher's own result, field by field in the documented order
    want = mm.match_traces(sv.provider.router(), g, mid, ctx, MatchParams(k=6, radius_m=200))
    ll = lambda n: [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)]    # noqa: E731
    traces = []
    for w in want:
        dist = mm.isqrt64(np.maximum(w["cand_d2"], 0))
        traces.append({"matchings": [{"nodes": [int(x) for x in m["nodes"]],
                                      "geometry": {"type": "LineString", "coordinates": [ll(int(x)) for x in m["nodes"]]},
                                      "distance": float(m["distance"]), "duration": float(m["duration"])}
                                     for m in w["matchings"]],
                       "tracepoints": [None if w["matched"][i] < 0 else
                                       {"location": ll(int(w["matched"][i])), "node": int(w["matched"][i]),
                                        "matchings_index": int(w["matching"][i]), "distance": int(dist[i]) / 100.0}
                                       for i in range(len(w["matched"]))]})
    import json
    assert json.loads(r.content) == {"code": "Ok", "traces": traces}
    assert list(json.loads(r.content)) == ["code", "traces"]
    assert [list(t) for t in json.loads(r.content)["traces"]] == [["matchings", "tracepoints"]] * 2


def test_edge_mode_response(client):
    c, sv = client
    g = sv.provider.g
    ctx, mid, body = _bodies(sv)
    r = c.post("/api/match", json=dict(body, snap="edge"))
    assert r.status_code == 200, r.text
    out = r.json()
    assert out["code"] == "Ok" and len(out["traces"]) == 2
    want = sv.provider.match(mid, ctx=ctx, params=MatchParams(k=6, radius_m=200), snap="edge")
    edges = me.graph_edges(g)
    for tr, w in zip(out["traces"], want):
        assert set(tr) == {"matchings", "tracepoints"} and len(tr["tracepoints"]) == len(w["edge"])
        assert len(tr["matchings"]) == len(w["matchings"]) >= 1
        for mt, wm in zip(tr["matchings"], w["matchings"]):
            assert set(mt) == {"nodes", "geometry", "distance", "duration"}
            assert mt["nodes"] == wm["nodes"].tolist() and mt["distance"] == wm["distance"] and mt["duration"] == wm["duration"]
            line = mt["geometry"]["coordinates"]
            assert mt["geometry"]["type"] == "LineString" and all(a != b for a, b in zip(line[:-1], line[1:]))
            la, lo = me.dequantize(wm["start"][0], wm["start"][1])
            assert line[0] == [round(float(lo), 6), round(float(la), 6)]
            la, lo = me.dequantize(wm["end"][0], wm["end"][1])
            assert line[-1] == [round(float(lo), 6), round(float(la), 6)]
            inner = [[round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)] for n in mt["nodes"]]
            assert [p for p in line if p in inner] == inner
        for i, tp in enumerate(tr["tracepoints"]):
            if w["edge"][i] < 0:
                assert tp is None
                continue
            e = int(w["edge"][i])
            assert set(tp) == {"location", "edge", "matchings_index", "distance"}
            assert set(tp["edge"]) == {"from", "to", "offset", "length"}
            assert (tp["edge"]["from"], tp["edge"]["to"]) == (int(edges["tail"][e]), int(edges["head"][e]))
            assert tp["edge"]["length"] == int(edges["lc"][e]) / 100.0
            assert tp["edge"]["offset"] == int(me.edge_offsets(edges["lc"][e], w["fq"][i])) / 100.0
            assert 0.0 <= tp["edge"]["offset"] <= tp["edge"]["length"]
            assert tp["matchings_index"] == int(w["matching"][i])
            assert tp["distance"] == int(mm.isqrt64(w["cand_d2"][i])) / 100.0 <= 200.0
            la, lo = me.dequantize(w["proj"][i, 0], w["proj"][i, 1])
            assert tp["location"] == [round(float(lo), 6), round(float(la), 6)]
            # the location lies on the edge: between its two ends on both axes
            for ax, co in ((0, g.lon), (1, g.lat)):
                lo_, hi_ = sorted((float(co[tp["edge"]["from"]]), float(co[tp["edge"]["to"]])))
                assert lo_ - 2e-6 <= tp["location"][ax] <= hi_ + 2e-6
    near = [tp["distance"] for t in out["traces"] for tp in t["tracepoints"] if tp is not None]
    assert sum(d <= 0.05 for d in near) >= 0.8 * len(near)                # mid-edge fixes: most snap onto their edge
    assert out["traces"][1]["tracepoints"][1] is None and None not in out["traces"][0]["tracepoints"]
    # the node matcher loses most of these fixes
    node = c.post("/api/match", json=body).json()
    assert sum(tp is None for t in node["traces"] for tp in t["tracepoints"]) > 1
    # the single-trace form
    r1 = c.post("/api/match", json=dict(CTX_BODY, coordinates=body["traces"][0]["coordinates"], radius=200, k=6,
                                        snap="edge"))
    assert r1.status_code == 200 and r1.json()["traces"] == out["traces"][:1]


@pytest.mark.parametrize("snap", [None, 5, True, "", "Edge", "nodes", ["edge"], {"edge": 1}])
def test_bad_snap_is_a_400_that_names_the_field(client, snap):
    c, _ = client
    r = c.post("/api/match", json={"coordinates": [[121.0, 14.6]], "snap": snap})
    assert r.status_code == 400 and "snap" in r.json()["error"]


@pytest.mark.parametrize("body", [
    [],
    {"snap": "edge"},
    {"traces": [], "snap": "edge"},
    {"traces": [{"coordinates": [[121.0, 95.0]]}], "snap": "edge"},
    {"coordinates": [[121.0, 14.6]], "k": 17, "snap": "edge"},
    {"coordinates": [[121.0, 14.6]], "radius": 1001, "snap": "edge"},
])
def test_edge_mode_keeps_the_other_400s(client, body):
    c, _ = client
    r = c.post("/api/match", json=body)
    assert r.status_code == 400 and r.json()["error"]
