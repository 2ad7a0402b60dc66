"""GPS-trace map matching (routing/mapmatch.py) on the CPU: the Python reference against the host
C++ (``_rt.MmGrid`` / ``_rt.mm_viterbi``, csrc/runtime/map_match.h), both against brute force, and
end to end on the CPU router.

* candidates: reference == ``_rt`` == an independent scan of all nodes sorted by (d2, node id), on
  the 3000-node graph and the hand-built tie graph (equidistant nodes, identical coordinates);
* Viterbi: reference == ``_rt`` on generated cost tensors (ties, dead states, breaks, no feasible
  transition at all, costs at the parameter maxima, ragged batches); the total cost equals full
  enumeration for T <= 5, K <= 3 (the minimum only: the tie rule is not lexicographic);
* end to end on ``synth_road_graph(3000, seed=7)``: matched nodes within the radius, connected
  segment paths (every step an edge), the detour bound between consecutive matched nodes, a break
  where no road joins, an unmatched fix, ``trips_from_traces`` feeding ``paths_csr`` /
  ``TripWorld.edge_seconds``, and ``POST /api/match`` with its 400s.
"""
import os

import numpy as np
import pytest

import _mapmatch_cases as cases
from routest_amd.routing import mapmatch as mm
from routest_amd.routing.mapmatch import MatchParams

rt = pytest.importorskip("routest_amd._rt")

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")


def _scan(nqy, nqx, y, x, r, k):
    """One fix, plain Python integers."""
    found = sorted((int(dy) ** 2 + int(dx) ** 2, v) for v, (dy, dx) in enumerate(zip(nqy - y, nqx - x))
                   if int(dy) ** 2 + int(dx) ** 2 <= r * r)[:k]
    return [v for _, v in found], [d for d, _ in found]


# ------------------------------------------------------------------------------------- parameters
def test_params_ranges_and_units():
    p = MatchParams()
    assert (p.k, p.radius_cm, p.sigma_cm, p.beta_cm, p.max_detour_cm) == (8, 25000, 5000, 3000, 200000)
    assert MatchParams(k=16, radius_m=1000, sigma_m=200, beta_m=100, max_detour_m=5000).radius_cm == 100000
    for bad in ({"k": 0}, {"k": 17}, {"k": 2.5}, {"k": True}, {"radius_m": 0}, {"radius_m": 1000.5}, {"sigma_m": -1},
                {"sigma_m": 201}, {"beta_m": 0}, {"beta_m": 101}, {"max_detour_m": 5001}, {"max_detour_m": float("nan")},
                {"radius_m": "250"}):
        with pytest.raises(ValueError):
            MatchParams(**bad)
    # the documented bound of a path score stays below the dead-state sentinel
    assert mm.MAX_POINTS * (10_000 * 100_000 ** 2 + 2 * 20_000 ** 2 * 500_000) < mm.DEAD < 2 ** 63


def test_quantize_and_isqrt():
    qy, qx = mm.quantize([14.6, -33.0], [121.0, -70.25])
    assert qy.dtype == qx.dtype == np.int64
    assert qy.tolist() == [int(np.rint(14.6 * 11_119_500)), int(np.rint(-33.0 * 11_119_500))]
    c = float(np.cos(np.radians(14.6)))
    assert qx.tolist() == [int(np.rint((121.0 * c) * 11_119_500)), int(np.rint((-70.25 * c) * 11_119_500))]
    with pytest.raises(ValueError):
        mm.quantize([float("nan")], [0.0])
    xs = np.array([0, 1, 2, 3, 4, 8, 9, 15, 16, 10 ** 10, 10 ** 10 - 1, (3 * 10 ** 9) ** 2 - 1, (3 * 10 ** 9) ** 2,
                   8 * 10 ** 18], dtype=np.int64)
    import math
    assert mm.isqrt64(xs).tolist() == [math.isqrt(int(x)) for x in xs]


# ------------------------------------------------------------------------------------- candidates
@pytest.fixture(scope="module")
def plain():
    g, cost = cases.plain_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    return g, cost, nqy, nqx, rt.MmGrid(nqy, nqx)


@pytest.mark.parametrize("k,radius_cm", [(1, 25_000), (2, 100_000), (8, 60_000), (16, 100_000), (3, 1)])
def test_candidates_reference_native_and_scan(plain, k, radius_cm):
    g, _, nqy, nqx, grid = plain
    rng = np.random.default_rng(k)
    lat = rng.uniform(g.lat.min() - 0.01, g.lat.max() + 0.01, 60)
    lon = rng.uniform(g.lon.min() - 0.01, g.lon.max() + 0.01, 60)
    lat[:5], lon[:5] = g.lat[[0, 17, 1500, 2998, 2999]], g.lon[[0, 17, 1500, 2998, 2999]]     # exactly on a node
    lat[5], lon[5] = g.lat.max() + 0.5, g.lon.mean()                                          # far outside
    lat[6], lon[6] = g.lat.min() - radius_cm / 100 / cases.M_PER_DEG * 0.9, g.lon[3]           # just outside the box
    py, px = mm.quantize(lat, lon)
    ref = mm.candidates_ref(nqy, nqx, py, px, radius_cm, k)
    nat = grid.candidates(py, px, radius_cm, k)
    one = rt.mm_candidates(nqy, nqx, py, px, radius_cm, k)
    for a, b, c in zip(ref, nat, one):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and np.array_equal(a, c)
    cand, cd2, nc = ref
    assert nc[5] == 0 and (cand[5] == -1).all() and (cd2[5] == -1).all()
    assert (cd2[:5, 0] == 0).all() and cand[:5, 0].tolist() == [0, 17, 1500, 2998, 2999]
    for p in range(0, 60, 3):
        ids, d2s = _scan(nqy, nqx, py[p], px[p], radius_cm, k)
        assert nc[p] == len(ids) and cand[p, :nc[p]].tolist() == ids and cd2[p, :nc[p]].tolist() == d2s
        assert (cand[p, nc[p]:] == -1).all() and (cd2[p, nc[p]:] == -1).all()
    if k <= 2:
        assert (nc == k).any()                                  # more nodes in range than asked for
    if k >= 8:
        assert ((nc > 0) & (nc < k)).any()                      # fewer than asked for


def test_candidate_ties_go_to_the_lower_node_id():
    g, (fy, fx) = cases.tie_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    py, px = np.array([fy, nqy[2]], np.int64), np.array([fx, nqx[2]], np.int64)
    assert (nqy[0] - py[0]) ** 2 + (nqx[0] - px[0]) ** 2 == (nqy[1] - py[0]) ** 2 + (nqx[1] - px[0]) ** 2
    assert nqy[2] == nqy[3] and nqx[2] == nqx[3]
    grid = rt.MmGrid(nqy, nqx)
    for k in (1, 2, 4, 8):
        ref = mm.candidates_ref(nqy, nqx, py, px, 50_000, k)
        nat = grid.candidates(py, px, 50_000, k)
        for a, b in zip(ref, nat):
            assert np.array_equal(a, b)
        assert ref[0][0, :min(k, 4)].tolist() == [0, 1, 2, 3][:k]
        assert ref[0][1, :min(k, 2)].tolist() == [2, 3][:k]
        assert ref[2].tolist() == [min(k, 4), min(k, 4)]


def test_native_argument_checks(plain):
    _, _, nqy, nqx, grid = plain
    with pytest.raises(ValueError):
        grid.candidates(nqy[:2], nqx[:2], 100, 17)
    with pytest.raises(ValueError):
        grid.candidates(nqy[:2], nqx[:2], 0, 4)
    with pytest.raises(ValueError):
        grid.candidates(nqy[:2], nqx[:3], 100, 4)
    cd, nc, route, g, npts = cases.viterbi_case(0, 1, 3, 2)
    with pytest.raises(ValueError):
        rt.mm_viterbi(cd, nc, route[:, :1], g, npts, 3000, 5000, 200000)
    with pytest.raises(ValueError):
        rt.mm_viterbi(cd, nc, route, g, npts, 0, 5000, 200000)


# ---------------------------------------------------------------------------------------- Viterbi
VITERBI_CASES = [(B, T, K, kind) for kind in ("random", "ties", "dead", "none", "max", "breaks")
                 for B, T, K in ((1, 1, 1), (3, 2, 3), (2, 9, 8), (2, 40, 16), (4, 5, 3))]


@pytest.mark.parametrize("B,T,K,kind", VITERBI_CASES)
def test_viterbi_reference_equals_native(B, T, K, kind):
    p = MatchParams(k=K, radius_m=1000, sigma_m=200, beta_m=100, max_detour_m=5000) if kind == "max" else MatchParams(k=K)
    cd, nc, route, g, npts = cases.viterbi_case(hash((B, T, K)) % 1000, B, T, K, kind, p, ragged=B > 2)
    ref = mm.viterbi_batch_ref(cd, nc, route, g, npts, p)
    nat = rt.mm_viterbi(cd, nc, route, g, npts, p.beta_cm, p.sigma_cm, p.max_detour_cm)
    for a, b in zip(ref, nat):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    choice, seg, nseg, cost = ref
    for b in range(B):
        n = int(npts[b])
        assert (choice[b, n:] == -1).all() and (seg[b, n:] == -1).all()
        assert nseg[b] == (seg[b, n - 1] + 1 if n else 0)
        assert (choice[b, :n] >= 0).all() and (choice[b, :n] < nc[b, :n]).all()
        if kind == "none":
            assert nseg[b] == n and (choice[b, :n] == 0).all()       # every fix its own segment, its nearest node
        if kind == "breaks" and n == T and T >= 2:
            assert seg[b, 1] == 1 and seg[b, T - 1] == seg[b, T - 2] + 1
            if T >= 6:
                assert seg[b, T // 2 + 1] == seg[b, T // 2 - 1] + 2
    if kind == "max" and T > 1:
        assert cost.max() > 2 ** 40                                   # far beyond any 32-bit intermediate


@pytest.mark.parametrize("kind", ["random", "ties", "dead", "breaks"])
def test_viterbi_cost_is_the_enumerated_minimum(kind):
    for seed in range(12):
        T, K = 1 + seed % 5, 1 + seed % 3
        p = MatchParams(k=K)
        cd, nc, route, g, npts = cases.viterbi_case(100 + seed, 2, T, K, kind, p)
        _, _, nseg, cost = mm.viterbi_batch_ref(cd, nc, route, g, npts, p)
        for b in range(2):
            assert (int(cost[b]), int(nseg[b])) == cases.enumerate_cost(cd[b], nc[b], route[b], g[b], T, p)


def test_viterbi_ties_take_the_lowest_predecessor_and_final_state():
    p = MatchParams(k=3)
    cd = np.zeros((1, 3, 3), np.int64)
    nc = np.full((1, 3), 3, np.int32)
    g = np.full((1, 2), 1000, np.int64)
    route = np.full((1, 2, 3, 3), 1000, np.int64)                     # every transition costs 0: all tie
    choice, seg, nseg, cost = mm.viterbi_batch_ref(cd, nc, route, g, np.array([3], np.int32), p)
    assert choice.tolist() == [[0, 0, 0]] and seg.tolist() == [[0, 0, 0]] and nseg[0] == 1 and cost[0] == 0
    route[0, 1, 0, :] = -1                                            # state 0 at step 1 reaches nothing
    choice, _, _, _ = mm.viterbi_batch_ref(cd, nc, route, g, np.array([3], np.int32), p)
    assert choice.tolist() == [[0, 1, 0]]
    assert np.array_equal(rt.mm_viterbi(cd, nc, route, g, np.array([3], np.int32), 3000, 5000, 200000)[0], choice)


# ------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def world(plain):
    from routest_amd.routing.graph import GraphProvider
    g, cost, _, _, _ = plain
    prov = GraphProvider(g, cost, device=None, engine="cch")
    router = prov.router()
    traces = cases.simulated_traces(g, router, prov.FIXED_KEY, 24, seed=5, noise_m=10.0)
    assert len(traces) >= 20
    return g, cost, prov, router, traces


def _is_edge(g, a, b):
    lo, hi = g.indptr[a], g.indptr[a + 1]
    j = lo + int(np.searchsorted(g.indices[lo:hi], b))
    return j < hi and g.indices[j] == b


def test_end_to_end_on_the_cpu_router(world):
    g, cost, prov, router, traces = world
    p = MatchParams()
    fixes = [f for f, _ in traces]
    fixes[3] = cases.with_unmatched_fix(g, fixes[3], 2)
    res = mm.match_traces(router, g, fixes, prov.FIXED_KEY, p)
    assert len(res) == len(fixes)
    nqy, nqx = mm.quantize(g.lat, g.lon)
    whole = hits = total = 0
    for i, (r, f) in enumerate(zip(res, fixes)):
        m, s = r["matched"], r["segment"]
        assert len(m) == len(s) == len(f)
        py, px = mm.quantize(f[:, 0], f[:, 1])
        on = m >= 0
        assert ((m < 0) == (s < 0)).all() and ((r["cand_d2"] < 0) == (m < 0)).all()
        d2 = (nqy[m[on]] - py[on]) ** 2 + (nqx[m[on]] - px[on]) ** 2
        assert (d2 <= p.radius_cm ** 2).all() and np.array_equal(d2, r["cand_d2"][on])
        assert r["n_segments"] == (s.max() + 1 if on.any() else 0) and len(r["matchings"]) == r["n_segments"]
        assert (np.diff(s[on]) >= 0).all()
        for q, mt in enumerate(r["matchings"]):
            nodes = mt["nodes"]
            assert mt["segment"] == q and len(nodes) >= 1
            for a, b in zip(nodes[:-1], nodes[1:]):
                assert _is_edge(g, int(a), int(b)), (i, q, int(a), int(b))
            ms = m[s == q]
            assert nodes[0] == ms[0] and nodes[-1] == ms[-1]
            # the matched nodes appear along the path in order
            it = iter(nodes.tolist())
            assert all(any(v == w for w in it) for v in ms.tolist())
            # detour bound between consecutive matched nodes of the segment
            col = ms[np.concatenate([[True], ms[1:] != ms[:-1]])]
            kept = np.flatnonzero(s == q)
            if len(col) > 1:
                sec, met, st, _ = router.route(col[:-1], col[1:], prov.FIXED_KEY, want_path=False)
                assert (st == 0).all()
                assert mt["duration"] == float(np.sum(sec.astype(np.float64))) or abs(mt["duration"] - sec.astype(np.float64).sum()) < 1e-9
                assert abs(mt["distance"] - met.astype(np.float64).sum()) < 1e-6
            for a, b in zip(kept[:-1], kept[1:]):
                if m[a] == m[b]:
                    continue
                _, met, st, _ = router.route([m[a]], [m[b]], prov.FIXED_KEY, want_path=False)
                rr = int(np.rint(float(met[0]) * 100.0))
                gg = int(mm.isqrt64((py[b] - py[a]) ** 2 + (px[b] - px[a]) ** 2))
                assert st[0] in (0, 4) and abs(rr - gg) <= p.max_detour_cm
        if i == 3:
            assert m[2] == -1 and s[2] == -1 and (np.delete(m, 2) >= 0).all()
        else:
            assert on.all()
            whole += r["n_segments"] == 1
            hits += int((m == traces[i][1]).sum())
            total += len(m)
    assert whole >= len(fixes) - 3                 # clean 10 m traces match in one piece
    assert hits >= 0.9 * total                     # and mostly to the node they were sampled at


def test_break_where_no_road_joins():
    from routest_amd.routing.cch import RoadRouter
    g, cost = cases.islands_graph()
    router = RoadRouter(g, None, device=None)
    key = router.metric_from_costs(1 << 40, cost)
    f, nodes, n_west = cases.cross_cut_trace(g, router, key)
    r = mm.match_traces(router, g, [f], key)[0]
    assert (r["matched"] >= 0).all() and r["n_segments"] >= 2 and len(r["matchings"]) == r["n_segments"]
    assert r["segment"][n_west - 1] + 1 == r["segment"][n_west]
    mid = (g.lon.min() + g.lon.max()) / 2
    for mt in r["matchings"]:
        side = g.lon[mt["nodes"]] < mid
        assert side.all() or not side.any()
        assert all(_is_edge(g, int(a), int(b)) for a, b in zip(mt["nodes"][:-1], mt["nodes"][1:]))


def test_python_fallback_equals_native(world, monkeypatch):
    """Without ``_rt`` the matcher runs on the Python reference: same answer."""
    g, cost, prov, router, traces = world
    fixes = [f for f, _ in traces[:3]]
    want = mm.match_traces(router, g, fixes, prov.FIXED_KEY)
    from routest_amd.ops import _ext
    real = _ext.runtime
    monkeypatch.setattr(_ext, "runtime", lambda required=True: None if not required else real(required))
    monkeypatch.setattr(g, "_mm_host", None, raising=False)
    got = mm.match_traces(router, g, fixes, prov.FIXED_KEY)
    for a, b in zip(want, got):
        assert np.array_equal(a["matched"], b["matched"]) and np.array_equal(a["segment"], b["segment"])
        assert [m["nodes"].tolist() for m in a["matchings"]] == [m["nodes"].tolist() for m in b["matchings"]]


def test_trips_from_traces_feed_the_observed_trainer(world):
    from routest_amd.models.gcn_observed import TripWorld, paths_csr, trips_from_traces
    g, cost, prov, router, traces = world
    fixes = [f for f, _ in traces[:8]]
    fixes[1] = cases.with_unmatched_fix(g, fixes[1], 0)
    seconds = [100.0 + i for i in range(8)]
    trips, dropped = trips_from_traces(prov, fixes, seconds)
    assert 1 in dropped and len(trips) + len(dropped) == 8 and len(trips) >= 5
    assert sorted(dropped) == dropped and all(0 <= i < 8 for i in dropped)
    kept = [i for i in range(8) if i not in dropped]
    assert [s for _, s in trips] == [seconds[i] for i in kept]
    paths = [p for p, _ in trips]
    rptr, nodes = paths_csr(paths)
    assert rptr[-1] == len(nodes) == sum(len(p) for p in paths)
    known = TripWorld(g, cost, seed=0).edge_seconds(paths)           # raises on a step that is no edge
    assert (known > 0).all()
    res = prov.match([fixes[i] for i in kept])
    for r, k in zip(res, known):
        assert abs(r["matchings"][0]["duration"] - k) < 1e-3 * max(1.0, k)
    with pytest.raises(ValueError):
        trips_from_traces(prov, fixes, seconds[:-1])


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


def test_match_endpoint(client):
    from routest_amd.routing.cch import RouteContext
    c, sv = client
    g = sv.provider.g
    ctx_body = {"context": {"weather": "Stormy", "traffic": "High", "pickup_time": "2025-08-29T18:00:00"}}
    ctx = RouteContext.from_request(ctx_body)
    _, _, st, paths = sv.provider.router().route([100, 900], [400, 300], ctx)
    assert (st == 0).all()
    coords = [[[float(g.lon[n]), float(g.lat[n])] for n in p] for p in paths]
    coords[1][1] = [coords[1][1][0], float(g.lat.max()) + 0.05]                      # an unmatched fix
    body = dict(ctx_body, traces=[{"coordinates": co} for co in coords], radius=200, k=6)
    r = c.post("/api/match", json=body)
    assert r.status_code == 200, r.text
    out = r.json()
    assert out["code"] == "Ok" and len(out["traces"]) == 2
    want = sv.provider.match([np.array([[la, lo] for lo, la in co]) for co in coords], ctx=ctx,
                             params=MatchParams(k=6, radius_m=200))
    for t, (tr, w, co) in enumerate(zip(out["traces"], want, coords)):
        assert set(tr) == {"matchings", "tracepoints"} and len(tr["tracepoints"]) == len(co)
        assert len(tr["matchings"]) == len(w["matchings"]) >= 1
        for mt, wm in zip(tr["matchings"], w["matchings"]):
            assert set(mt) == {"nodes", "geometry", "distance", "duration"}
            assert mt["nodes"] == wm["nodes"].tolist() and mt["distance"] == wm["distance"] and mt["duration"] == wm["duration"]
            assert mt["geometry"]["type"] == "LineString"
            assert mt["geometry"]["coordinates"] == [[round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)] for n in mt["nodes"]]
        for i, tp in enumerate(tr["tracepoints"]):
            if w["matched"][i] < 0:
                assert tp is None
                continue
            n = int(w["matched"][i])
            assert set(tp) == {"location", "node", "matchings_index", "distance"}
            assert tp["node"] == n and tp["location"] == [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)]
            assert tp["matchings_index"] == int(w["matching"][i]) and n in tr["matchings"][tp["matchings_index"]]["nodes"]
            assert tp["distance"] == int(mm.isqrt64(w["cand_d2"][i])) / 100.0
    assert out["traces"][0]["tracepoints"][0]["distance"] == 0.0 and None not in out["traces"][0]["tracepoints"]
    assert out["traces"][1]["tracepoints"][1] is None
    # the single-trace form
    r1 = c.post("/api/match", json=dict(ctx_body, coordinates=coords[0], radius=200, k=6))
    assert r1.status_code == 200 and r1.json()["traces"] == out["traces"][:1]


@pytest.mark.parametrize("body", [
    [],
    {},
    {"traces": []},
    {"traces": "x"},
    {"traces": [{"coordinates": []}]},
    {"traces": [{"nodes": [1, 2]}]},
    {"traces": [{"coordinates": [[121.0]]}]},
    {"traces": [{"coordinates": [[121.0, "x"]]}]},
    {"traces": [{"coordinates": [[121.0, 95.0]]}]},
    {"traces": [{"coordinates": [[121.0, 14.6]]}] * 65},
    {"traces": [{"coordinates": [[121.0, 14.6]] * 2049}]},
    {"coordinates": [[121.0, 14.6]], "k": 0},
    {"coordinates": [[121.0, 14.6]], "k": 17},
    {"coordinates": [[121.0, 14.6]], "k": 2.5},
    {"coordinates": [[121.0, 14.6]], "radius": 0},
    {"coordinates": [[121.0, 14.6]], "radius": 1001},
    {"coordinates": [[121.0, 14.6]], "sigma": 201},
    {"coordinates": [[121.0, 14.6]], "beta": "30"},
    {"coordinates": [[121.0, 14.6]], "max_detour": 5001},
])
def test_match_bad_bodies(client, body):
    c, _ = client
    r = c.post("/api/match", json=body)
    assert r.status_code == 400 and r.json()["error"]


def test_match_needs_the_graph_provider_and_the_cch_router():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.providers import ProviderError
    from routest_amd.serve.eta_service import EtaService
    s = load_settings(env={"ROUTEST_PROVIDER": "haversine"}, dotenv_path=None, device="cpu", route_batch="0",
                      warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/match", json={"coordinates": [[121.0, 14.6]]})
        assert r.status_code == 400 and "ROUTEST_PROVIDER=graph" in r.json()["error"]
    sv.close()
    g, cost = cases.plain_graph()
    with pytest.raises(ProviderError, match="ROUTEST_ROUTER"):
        GraphProvider(g, cost, device=None, engine="astar").match([[(14.6, 121.0)]])
