"""Intra-trip 2-opt / Or-opt improvement of the greedy's trips (routing/improve.py): the Python
reference against the host C++ (``_rt.improve_trips``) with ``==``, the reference's own
properties, the revert rule, the size limits, and the ``improve`` field on the HTTP API.
Instances: tests/_improve_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.greedy import greedy_trips
from routest_amd.routing.improve import (BIG, MAX_STOPS, apply_move, improve_trips, quantize,
                                         quantize_matrix, search_trip, trip_length_q, walk_feasible)

from _improve_cases import expected, named_instances, random_instance, revert_instance

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = list(named_instances())


# --------------------------------------------------------------------------- reference vs host C++
def test_host_cpp_equals_reference_on_every_instance():
    rt = pytest.importorskip("routest_amd._rt")
    changed = 0
    for name in NAMES:
        d, _, _, md = named_instances()[name]
        g, new, st = expected(name)
        got_trips, got_st = rt.improve_trips(np.asarray(d, dtype=np.float64), g, md)
        assert got_trips == new, name
        assert got_st == st, name
        changed += st["trips_changed"]
    assert changed > 20


def test_instances_cover_the_issue():
    ks = {len(t) - 2 for n in NAMES for t in expected(n)[0]}
    assert {1, 2, 3, 4, 7, 32, 33, 128, 129} <= ks
    assert [len(t) - 2 for t in expected("trips_k65_cap33")[0]] == [33, 32]
    assert len(expected("trips_k20_cap6")[0]) == 4
    assert sum(n.startswith("association_") for n in NAMES) > 60
    # grid instances: some applied move had an exact tie for the best gain
    assert _tied_best_moves("grid_k12") > 0


# --------------------------------------------------------------------------- brute force helpers
def _all_moves(k):
    for i in range(1, k + 1):
        for j in range(i + 1, k + 1):
            yield 0, i, j
    for ln in (1, 2, 3):
        for i in range(1, k - ln + 2):
            e = i + ln - 1
            for j in range(0, k + 1):
                if j < i - 1 or j > e:
                    yield ln, i, j


def _gain(q, t, typ, i, j):
    """The issue's gain formulas, written out with plain loops."""
    Q = lambda a, b: int(q[t[a], t[b]])  # noqa: E731
    if typ == 0:
        fwd = sum(Q(p, p + 1) for p in range(i, j))
        bwd = sum(Q(p + 1, p) for p in range(i, j))
        return (Q(i - 1, i) + Q(j, j + 1) + fwd) - (Q(i - 1, j) + Q(i, j + 1) + bwd)
    e = i + typ - 1
    return Q(i - 1, i) + Q(e, e + 1) + Q(j, j + 1) - Q(i - 1, e + 1) - Q(j, i) - Q(e, j + 1)


def _best_by_brute_force(q, t):
    """(gain, type, i, j) of the best move by the selection rule; by applying every move and
    measuring the trip when the trip is short, by the gain formulas otherwise."""
    k = len(t) - 2
    L = trip_length_q(q, t)
    best = (0, -1, -1, -1)
    for typ, i, j in _all_moves(k):
        g = L - trip_length_q(q, apply_move(list(t), typ, i, j)) if k <= 12 else _gain(q, t, typ, i, j)
        if g > best[0]:            # moves come in (type, i, j) order: the first maximum wins
            best = (g, typ, i, j)
    return best


def _tied_best_moves(name):
    """How many applied moves of the instance's search had another move with the same gain."""
    d, _, _, _ = named_instances()[name]
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    ties = 0
    for trip in expected(name)[0]:
        t = list(trip)
        k = len(t) - 2
        while k >= 2:
            gains = [L0 - trip_length_q(q, apply_move(list(t), *m))
                     for L0 in [trip_length_q(q, t)] for m in _all_moves(k)]
            top = max(gains)
            if top <= 0:
                break
            ties += gains.count(top) > 1
            t = apply_move(t, *list(_all_moves(k))[gains.index(top)])
    return ties


# --------------------------------------------------------------------------- the reference itself
def test_quantization():
    assert quantize(0.0) == 0 and quantize(1.0005) == 1000 and quantize(1.0015) == 1002
    assert quantize(0.0005) == 0 and quantize(0.0015) == 2 and quantize(0.0025) == 2   # half-even
    for bad in (float("nan"), float("inf"), float("-inf"), -1e-9, 2.0 ** 40, 1e300):
        assert quantize(bad) == BIG
    assert quantize(np.nextafter(2.0 ** 40, 0)) == int(np.rint(np.nextafter(2.0 ** 40, 0) * 1000.0))
    x = np.array([[0.0, np.nan, -1.0], [np.inf, 0.0, 2.5], [2.0 ** 40, 1e-4, 0.0]])
    assert quantize_matrix(x).tolist() == [[quantize(v) for v in row] for row in x.tolist()]
    assert 4097 * BIG < 2 ** 63


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("association_")] +
                         ["association_0", "association_30", "association_60"])
def test_reference_properties(name):
    d, _, _, md = named_instances()[name]
    g, new, st = expected(name)
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    assert len(new) == len(g)                                   # trip count and order unchanged
    moves = changed = before = after = 0
    for tg, tn in zip(g, new):
        k = len(tg) - 2
        assert tn[0] == 0 and tn[-1] == 0 and sorted(tn) == sorted(tg)   # stop set and ends kept
        lg, ln = trip_length_q(q, tg), trip_length_q(q, tn)
        assert ln <= lg
        before += lg
        after += ln
        if k < 2 or k > MAX_STOPS:
            assert tn == tg
            continue
        if tn != tg:
            changed += 1
            assert ln < lg
            assert walk_feasible(d, tn, md)                     # the f64 walk holds max_dist
            if k > 40:                                          # long trips: the end state only
                moves += search_trip(q, tg)[1]
                assert _best_by_brute_force(q, tn)[0] == 0
                continue
            # replay: every applied move is the brute-force best, and none is left at the end
            t, m = list(tg), 0
            while t != tn:
                gain, typ, i, j = _best_by_brute_force(q, t)
                assert gain > 0
                t = apply_move(t, typ, i, j)
                m += 1
                assert m < 4 * k                                # the cap did not bind
            moves += m
            assert _best_by_brute_force(q, t)[0] == 0
    assert (st["moves"], st["trips_changed"], st["len_before_q"], st["len_after_q"]) == \
        (moves, changed, before, after)
    assert after <= before


def test_cap_never_binds_and_unchanged_trips_are_local_optima():
    """``moves < 4k`` on every trip of this file, so no test passes on a truncated search; a trip
    that came back unchanged (and was not reverted) has no move of positive gain."""
    for name in NAMES:
        d, _, _, md = named_instances()[name]
        g, new, st = expected(name)
        q = quantize_matrix(np.asarray(d, dtype=np.float64))
        for tg, tn in zip(g, new):
            k = len(tg) - 2
            if k < 2 or k > MAX_STOPS:
                continue
            _, m = search_trip(q, tg)
            assert m < 4 * k, name
            if tn == tg and m == 0 and k <= 12:
                assert _best_by_brute_force(q, tg)[0] == 0, name


def test_bad_entries_are_big_and_avoided():
    """An inf / NaN / negative entry between two stops quantizes to BIG: a search that starts on
    such an edge leaves it whenever a finite order exists."""
    for i in range(4):
        d, _, _, _ = named_instances()[f"special_{i}"]
        g, new, st = expected(f"special_{i}")
        q = quantize_matrix(np.asarray(d, dtype=np.float64))
        assert (q == BIG).sum() >= 1
        assert st["len_after_q"] < BIG


# --------------------------------------------------------------------------- revert and size limits
def test_revert_when_the_f64_walk_exceeds_max_dist():
    d, dem, cap, g, new, wg, wn = revert_instance()
    assert 3 <= len(g) - 2 <= 4 and wn > wg
    q = quantize_matrix(np.asarray(d))
    assert trip_length_q(q, new) < trip_length_q(q, g)          # shorter in q, longer in f64
    assert greedy_trips(d, dem, cap, wg) == [g]
    rt = pytest.importorskip("routest_amd._rt")
    for fn in (improve_trips, rt.improve_trips):
        trips, st = fn(np.asarray(d), [g], wg)                  # max_dist = the greedy trip's own total
        assert trips == [g] and st["moves"] == 0 and st["trips_changed"] == 0
        assert st["len_after_q"] == st["len_before_q"] == trip_length_q(q, g)
        trips, st = fn(np.asarray(d), [g], wn)                  # just enough for the new order
        assert trips == [new] and st["moves"] >= 1 and st["trips_changed"] == 1
        assert st["len_after_q"] == trip_length_q(q, new)


def test_size_limits():
    rt = pytest.importorskip("routest_amd._rt")
    for k in (129, 1):
        d, dem, cap, md = random_instance(k, 40 + k)
        g = greedy_trips(d, dem, cap, md)
        assert [len(t) - 2 for t in g] == [k]
        for fn in (improve_trips, rt.improve_trips):
            trips, st = fn(np.asarray(d), g, md)
            assert trips == g and st["moves"] == 0 and st["trips_changed"] == 0
            assert st["len_before_q"] == st["len_after_q"] > 0
    d, dem, cap, md = random_instance(128, 41)
    g = greedy_trips(d, dem, cap, md)
    assert improve_trips(np.asarray(d), g, md)[1]["moves"] > 0


# --------------------------------------------------------------------------- API contract
def _zigzag(lat0, lon0, n=9, **extra):
    """Stops on alternating sides of the depot at growing distance."""
    dests = [{"lat": lat0 + (0.002 + 0.002 * i) * (1 if i % 2 else -1), "lon": lon0 + 0.0004 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": 99,
                            "maximum_distance": 1e6}}
    p.update(extra)
    return p


@pytest.fixture(scope="module", params=["haversine", "graph"])
def client(request):
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.serve.eta_service import EtaService, default_model
    env = {"ROUTEST_PROVIDER": "haversine"}
    if request.param == "graph":
        env = {"ROUTEST_PROVIDER": "graph", "ROUTEST_GRAPH_PATH": os.path.join(FIX, "manila_small.edges.csv")}
    s = load_settings(env=env, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False,
                      scorer_train_steps=40)
    sv = build_services(s, eta=EtaService(default_model(hidden=64, steps=20), device="cpu"), store=None)
    assert sv.provider.name == request.param
    if request.param == "graph":
        g = sv.provider.g
        lat0, lon0 = float(np.median(g.lat)), float(np.median(g.lon))
    else:
        lat0, lon0 = 14.58, 121.04
    with TestClient(create_app(sv)) as c:
        yield c, sv, lat0, lon0
    sv.close()


def _post(c, path, body):
    r = c.post(path, json=body)
    assert r.status_code == 200, r.text
    return r.json()


@pytest.mark.parametrize("path", ["/api/optimize_route", "/route", "/api/request_route"])
def test_api_improve_field(client, path):
    c, sv, lat0, lon0 = client
    plain = _post(c, path, _zigzag(lat0, lon0))
    assert "improvement" not in plain["properties"]
    out = _post(c, path, _zigzag(lat0, lon0, improve=True))
    imp = out["properties"]["improvement"]
    assert list(imp) == ["method", "moves", "trips_changed", "matrix_distance_before",
                         "matrix_distance_after"]
    assert imp["method"] == "2opt+oropt" and imp["moves"] >= 1 and imp["trips_changed"] >= 1
    assert imp["matrix_distance_after"] < imp["matrix_distance_before"]
    assert out["properties"]["summary"]["distance"] < plain["properties"]["summary"]["distance"]
    assert out["properties"]["summary"]["trips"] == plain["properties"]["summary"]["trips"]
    assert sorted(out["properties"]["optimized_order"]) == sorted(plain["properties"]["optimized_order"])
    assert out["properties"]["optimized_order"] != plain["properties"]["optimized_order"]
    # nothing else changes shape
    assert set(out["properties"]) - {"improvement"} == set(plain["properties"])
    # anything but JSON true is off
    for v in ("yes", 1, False, None, "true", [True]):
        assert _post(c, path, _zigzag(lat0, lon0, improve=v)) == plain, v


def test_api_single_destination_ignores_improve(client):
    c, sv, lat0, lon0 = client
    one = _zigzag(lat0, lon0, n=1)
    assert _post(c, "/api/optimize_route", dict(one, improve=True)) == _post(c, "/api/optimize_route", one)


def test_api_alternatives_ignore_improve(client):
    c, sv, lat0, lon0 = client
    if sv.provider.name != "graph":
        return          # alternatives need the road graph; elsewhere the answer is an error either way
    body = _zigzag(lat0, lon0, n=4, alternatives=3)
    a = c.post("/api/optimize_route", json=body)
    b = c.post("/api/optimize_route", json=dict(body, improve=True))
    assert a.status_code == b.status_code and a.json() == b.json()
    if sv.provider.name == "graph":
        assert a.status_code == 200 and "alternatives" in a.json()["properties"]
        assert "improvement" not in b.json()["properties"]


def test_api_batch_takes_the_field_per_request(client):
    c, sv, lat0, lon0 = client
    reqs = [_zigzag(lat0, lon0), _zigzag(lat0, lon0, improve=True), _zigzag(lat0, lon0, n=1, improve=True),
            _zigzag(lat0, lon0, n=6, improve="yes")]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs})["results"]
    assert ["improvement" in r["properties"] for r in res] == [False, True, False, False]
    assert res[1] == _post(c, "/api/request_route", reqs[1])
    assert res[0] == _post(c, "/api/request_route", reqs[0])


def test_native_cpu_planner_answers_like_the_app():
    """``_rt.route_optimize_cpu`` (csrc/runtime/route_bind.cpp) writes ``improvement`` byte for byte
    like the app's JSON response."""
    rt = pytest.importorskip("routest_amd._rt")
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.providers import HaversineProvider
    prov = HaversineProvider()
    for extra in ({"improve": True}, {"improve": True, "driver_details": {"vehicle_capacity": 4,
                                                                         "maximum_distance": 1e6}},
                  {"improve": "yes"}, {}):
        p = _zigzag(14.58, 121.04, **extra)
        ref = optimize_route(p, prov, "backend:mi355x")
        assert ("improvement" in ref["properties"]) == (extra.get("improve") is True)
        want = json.dumps(ref, ensure_ascii=False, separators=(",", ":"), allow_nan=False).encode()
        st, body = rt.route_optimize_cpu(json.dumps(p).encode())
        assert st == 200 and bytes(body) == want
