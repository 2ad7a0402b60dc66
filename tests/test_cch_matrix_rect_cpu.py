"""Rectangular matrices without a GPU: the CPU router's ``matrix_rect`` / ``matrices_rect`` (the
reference of tests/test_cch_matrix_rect_gpu.py) against Dijkstra, ``POST /api/matrix`` (every 400,
the response's shape, ``null`` cells, snapping) and the matcher's ``transitions="matrix"`` on the
CPU router."""
import os

import numpy as np
import pytest

import _cch_graphs as G
import _mapmatch_cases as cases

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
KEY = 1 << 40
RAGGED = [(1, 1), (2, 64), (64, 2), (7, 65), (0, 5), (5, 0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def model():
    from routest_amd.serve.eta_service import default_model
    return default_model(hidden=64, steps=20)


@pytest.fixture(scope="module")
def islands(model):
    from routest_amd.routing.cch import RoadRouter
    g, cost = G.islands_graph()
    r = RoadRouter(g, model, device=None)
    r.metric_from_costs(KEY, cost)
    return g, cost, r


def _lists(g, S, D, seed):
    src, dst = G.uniform_pairs(g, max(S, D, 2), seed)
    src, dst = src.copy(), dst.copy()
    mid = (g.lon.min() + g.lon.max()) / 2
    src[0], src[1] = np.flatnonzero(g.lon < mid)[seed], np.flatnonzero(g.lon >= mid)[seed]
    return src[:S], dst[:D]


# ---------------------------------------------------------------------------------- the CPU router
def test_cpu_matrix_rect_against_dijkstra(islands):
    """The bound is the one tests/test_cch_edges_cpu.py uses for CCH seconds against float64
    Dijkstra (rtol 1e-5, atol 1e-4)."""
    g, cost, r = islands
    src, dst = _lists(g, 9, 70, seed=3)
    dst[4] = src[2]
    sec, met = r.matrix_rect(src, dst, KEY)
    assert sec.shape == met.shape == (9, 70) and sec.dtype == met.dtype == np.float32
    ref = G.dijkstra_pairs(g, cost, np.repeat(src, 70), np.tile(dst, 9)).reshape(9, 70)
    assert np.array_equal(np.isinf(ref), np.isinf(sec)) and np.array_equal(np.isinf(sec), np.isinf(met))
    assert np.isinf(sec).any() and np.isfinite(sec).any()
    ok = np.isfinite(ref)
    np.testing.assert_allclose(sec[ok], ref[ok], rtol=1e-5, atol=1e-4)
    assert _bits(sec[2, 4]) == 0 and _bits(met[2, 4]) == 0


def test_cpu_matrix_rect_equals_square_matrix(islands):
    g, _, r = islands
    L = np.random.default_rng(50).choice(g.num_nodes, 40, replace=False).astype(np.int32)
    rect, sq = r.matrix_rect(L, L, KEY), r.matrix(L, KEY)
    for a, b in zip(rect, sq):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_cpu_chunking_equals_unchunked(islands):
    g, _, r = islands
    rows = [_lists(g, S, D, seed=40 + k) for k, (S, D) in enumerate(RAGGED)]
    whole = r.matrices_rect(rows, KEY)
    assert [a.shape for a, _ in whole] == RAGGED
    for mj in (16, 1):
        for (a, b), (c, d) in zip(r.matrices_rect(rows, KEY, max_jobs=mj), whole):
            assert a.shape == c.shape and np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(b), _bits(d))
    for (s, d), (a, b) in zip(rows, whole):
        one = r.matrix_rect(s, d, KEY)
        assert np.array_equal(_bits(one[0]), _bits(a)) and np.array_equal(_bits(one[1]), _bits(b))
    with pytest.raises(IndexError):
        r.matrix_rect([0, g.num_nodes], [1], KEY)
    with pytest.raises(ValueError):
        r.matrices_rect(rows, KEY, max_jobs=0)


# ------------------------------------------------------------------------------------ the endpoint
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


P = [121.0, 14.6]
BAD = [
    [],
    {},
    {"locations": "x"},
    {"locations": []},
    {"locations": [P] * 4097},
    {"locations": [[121.0]]},
    {"locations": [[121.0, "x"]]},
    {"locations": [[121.0, float("nan")]]},
    {"locations": [[121.0, float("inf")]]},
    {"locations": [[121.0, True]]},
    {"locations": [[181.0, 14.6]]},
    {"locations": [P, P], "sources": "some"},
    {"locations": [P, P], "sources": []},
    {"locations": [P, P], "sources": 0},
    {"locations": [P, P], "sources": [2]},
    {"locations": [P, P], "sources": [-1]},
    {"locations": [P, P], "sources": [0.5]},
    {"locations": [P, P], "sources": [1.0]},
    {"locations": [P, P], "sources": ["0"]},
    {"locations": [P, P], "sources": [True]},
    {"locations": [P, P], "sources": [0, 0]},
    {"locations": [P, P], "destinations": []},
    {"locations": [P, P], "destinations": [2]},
    {"locations": [P, P], "destinations": [False]},
    {"locations": [P, P], "destinations": [1, 1]},
    {"locations": [P, P], "destinations": {"0": 1}},
    {"locations": [P] * 513, "sources": list(range(513)), "destinations": list(range(513))},      # 263,169 cells
    {"locations": [P] * 513},                                                                      # the same, by "all"
    {"locations": [P, P], "metrics": []},
    {"locations": [P, P], "metrics": "duration"},
    {"locations": [P, P], "metrics": ["duration", "hops"]},
    {"locations": [P, P], "metrics": [1]},
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_matrix_bad_bodies(client, k):
    import json
    c, _ = client
    # (json.dumps writes NaN / Infinity literals, which the service's parser accepts as floats)
    r = c.post("/api/matrix", content=json.dumps(BAD[k]), headers={"content-type": "application/json"})
    assert r.status_code == 400 and r.json()["error"], (BAD[k], r.text)


def test_matrix_cell_cap_is_exact():
    from routest_amd.routing.matrix import MAX_CELLS, MAX_LOCATIONS, parse_request
    assert MAX_CELLS == 262_144 and MAX_LOCATIONS == 4096
    ok = parse_request({"locations": [P] * 512})                         # 512 x 512 = the cap
    assert len(ok["sources"]) == len(ok["destinations"]) == 512
    parse_request({"locations": [P] * 4096, "sources": list(range(64))})  # 64 x 4096 = the cap
    with pytest.raises(ValueError):
        parse_request({"locations": [P] * 4096, "sources": list(range(65))})
    with pytest.raises(ValueError):
        parse_request({"locations": [P] * 513})


def test_matrix_endpoint(client):
    from routest_amd.routing.cch import RouteContext
    from routest_amd.routing.providers import haversine_scalar
    c, sv = client
    g = sv.provider.g
    nodes = [100, 900, 17, 450, 1200, 33]
    locs = [[float(g.lon[n]) + 2e-5, float(g.lat[n]) - 1e-5] for n in nodes]
    ctx_body = {"context": {"weather": "Stormy", "traffic": "High", "pickup_time": "2025-08-29T18:00:00"}}
    body = dict(ctx_body, locations=locs, sources=[0, 1], destinations=[2, 3, 4, 5], metrics=["distance", "duration"])
    r = c.post("/api/matrix", json=body)
    assert r.status_code == 200, r.text
    out = r.json()
    assert set(out) == {"durations", "distances", "sources", "destinations", "metadata"}
    snapped = g.nearest_nodes([p[1] for p in locs], [p[0] for p in locs])
    ctx = RouteContext.from_request(body)
    sec, met = sv.provider.router().matrix_rect(snapped[:2], snapped[2:], ctx)
    assert out["durations"] == [[float(x) for x in row] for row in sec]
    assert out["distances"] == [[float(x) for x in row] for row in met]
    pts = out["sources"] + out["destinations"]
    assert len(out["sources"]) == 2 and len(out["destinations"]) == 4
    for k, p in enumerate(pts):
        n = int(snapped[k])
        assert p["node"] == n and p["location"] == [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)]
        assert p["snapped_distance"] == haversine_scalar(locs[k][1], locs[k][0], float(g.lat[n]), float(g.lon[n]))
        assert 0 < p["snapped_distance"] < 50
    assert out["metadata"] == {"engine": "cch", "context": {"weather": ctx.weather, "congestion": ctx.congestion,
                                                            "weekhour": ctx.weekhour}}
    # metrics decide the keys; the default is durations only
    only = c.post("/api/matrix", json=dict(body, metrics=["distance"])).json()
    assert "distances" in only and "durations" not in only and only["distances"] == out["distances"]
    dflt = c.post("/api/matrix", json={k: v for k, v in body.items() if k != "metrics"}).json()
    assert "durations" in dflt and "distances" not in dflt and dflt["durations"] == out["durations"]
    # "all" and absent are the same request
    small = dict(ctx_body, locations=locs[:3], metrics=["duration", "distance"])
    a = c.post("/api/matrix", json=small).json()
    b = c.post("/api/matrix", json=dict(small, sources="all", destinations="all")).json()
    e = c.post("/api/matrix", json=dict(small, sources=[0, 1, 2], destinations=[0, 1, 2])).json()
    assert a == b == e and len(a["durations"]) == 3 and len(a["durations"][0]) == 3
    assert [a["durations"][i][i] for i in range(3)] == [0.0] * 3
    # the rows follow the order of the index lists
    rev = c.post("/api/matrix", json=dict(small, sources=[2, 0], destinations=[1])).json()
    assert rev["durations"] == [[a["durations"][2][1]], [a["durations"][0][1]]]


def test_matrix_unreachable_cells_are_null():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    g, cost = G.islands_graph()
    prov = GraphProvider(g, cost, device=None, engine="cch")
    s = load_settings(env={}, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    mid = (g.lon.min() + g.lon.max()) / 2
    west, east = np.flatnonzero(g.lon < mid - 0.01)[:2], np.flatnonzero(g.lon > mid + 0.01)[:2]
    nodes = [int(west[0]), int(east[0]), int(west[1]), int(east[1])]
    body = {"locations": [[float(g.lon[n]), float(g.lat[n])] for n in nodes], "sources": [0, 1],
            "destinations": [2, 3], "metrics": ["duration", "distance"]}
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/matrix", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
    sec, met = prov.router().matrix_rect(nodes[:2], nodes[2:], prov.FIXED_KEY)
    assert np.isinf(sec[0, 1]) and np.isinf(sec[1, 0])
    for got, want in ((out["durations"], sec), (out["distances"], met)):
        assert got == [[float(x) if np.isfinite(x) else None for x in row] for row in want]
        assert got[0][1] is None and got[1][0] is None
    assert [p["node"] for p in out["sources"] + out["destinations"]] == nodes
    assert all(p["snapped_distance"] == 0.0 for p in out["sources"] + out["destinations"])
    sv.close()


def test_matrix_needs_the_graph_provider_and_the_cch_router():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    body = {"locations": [[121.0, 14.6], [121.01, 14.61]]}
    s = load_settings(env={"ROUTEST_PROVIDER": "haversine"}, dotenv_path=None, device="cpu", route_batch="0",
                      warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/matrix", json=body)
        assert r.status_code == 400 and "ROUTEST_PROVIDER=graph" in r.json()["error"]
    sv.close()
    g, cost = G.islands_graph()
    prov = GraphProvider(g, cost, device=None, engine="astar")
    s = load_settings(env={}, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=prov, store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/matrix", json={"locations": [[float(g.lon[0]), float(g.lat[0])]] * 2})
        assert r.status_code == 400 and "ROUTEST_ROUTER=astar" in r.json()["error"]
    sv.close()


# ------------------------------------------------------------------------------------- the matcher
def _same_matches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("matched", "segment", "matching", "cand_d2"):
            assert np.array_equal(x[f], y[f]), f
        assert x["n_segments"] == y["n_segments"] and len(x["matchings"]) == len(y["matchings"])
        for m, n in zip(x["matchings"], y["matchings"]):
            assert np.array_equal(m["nodes"], n["nodes"]) and m["segment"] == n["segment"]
            assert m["duration"] == n["duration"] and m["distance"] == n["distance"]


def test_matcher_matrix_transitions_equal_pairs_on_the_cpu(islands, monkeypatch):
    from routest_amd.routing import mapmatch as mm
    g, cost, r = islands
    sim = cases.simulated_traces(g, r, KEY, 6, seed=3, noise_m=15.0)
    fixes = [f for f, _ in sim]
    cut, _, n_west = cases.cross_cut_trace(g, r, KEY)
    fixes.append(cut)
    fixes.append(cases.with_unmatched_fix(g, fixes[0], 1))
    for p in (mm.MatchParams(), mm.MatchParams(k=1), mm.MatchParams(k=16, radius_m=600, sigma_m=20, beta_m=5)):
        sp, sm = {}, {}
        pairs = mm.match_traces(r, g, fixes, KEY, p, transitions="pairs", stats=sp)
        _same_matches(pairs, mm.match_traces(r, g, fixes, KEY, p, transitions="matrix", stats=sm))
        _same_matches(pairs, mm.match_traces(r, g, fixes, KEY, p))
        assert set(sp) == set(sm) and sm["pairs_queried"] >= sp["pairs_queried"] > 0
    assert pairs[-2]["n_segments"] >= 2 and pairs[-1]["matched"][1] == -1
    monkeypatch.setattr(mm, "RECT_MAX_JOBS", 40)
    _same_matches(pairs, mm.match_traces(r, g, fixes, KEY, p, transitions="matrix"))
    with pytest.raises(ValueError):
        mm.match_traces(r, g, fixes, KEY, p, transitions="rows")
