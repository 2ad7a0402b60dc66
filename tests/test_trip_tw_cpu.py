"""Delivery time windows (routing/timewindows.py): the Python reference against the host C++
(``_rt.tw_trips``) with ``==``, the O(1) admissibility test against full re-simulation, the
invariants of the produced trips, the unchanged answers of requests without the fields, and the
``time_window`` / ``service`` fields on the HTTP API.  Instances: tests/_tw_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.exchange import UNBOUNDED, load_feasible
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.improve import walk_feasible
from routest_amd.routing.timewindows import (parse_time_windows, time_admissible, tw_trips, usable_matrix,
                                             wants_time_windows)

from _tw_cases import expected, named_instances, random_instance, resimulate

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = list(named_instances())


def _rt_answer(rt, c):
    got = rt.tw_trips(np.asarray(c["d"], dtype=np.float64), np.asarray(c["t"], dtype=np.float64), c["demand"],
                      c["cap"], c["max_dist"], c["open_q"], c["close_q"], c["sv_q"])
    if got[0] is None:
        return ("infeasible", list(got[1]))
    return got[0], [[tuple(r) for r in trip] for trip in got[1]], got[2]


# --------------------------------------------------------------------------- reference vs host C++
def test_host_cpp_equals_reference_on_every_instance():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    inserted = 0
    for name in NAMES:
        want = expected(name)
        assert _rt_answer(rt, named_instances()[name]) == want, name
        if want[0] != "infeasible":
            inserted += want[2]["insertions"]
    assert inserted > 500


def test_host_cpp_equals_reference_on_random_instances():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    rng = np.random.default_rng(5)
    trips = 0
    for seed in range(300):
        ns = int(rng.integers(1, 15))
        c = random_instance(ns, 20_000 + seed, road=bool(seed % 2), cap_frac=(None, 0.4)[seed % 3 == 0])
        try:
            want = tw_trips(**c)
            trips += len(want[0])
        except InfeasibleStops as e:
            want = ("infeasible", e.stops)
        assert _rt_answer(rt, c) == want, seed
    assert trips > 300


def test_instances_cover_the_issue():
    inst = named_instances()
    sizes = {len(c["d"]) - 1 for c in inst.values()}
    assert {1, 2, 31, 32, 33, 64, 127, 128} <= sizes
    assert all(c == UNBOUNDED for c in inst["service_only"]["close_q"]) and any(inst["service_only"]["sv_q"])
    z = inst["zero_width"]
    assert all(a == b for a, b in zip(z["open_q"][1:], z["close_q"][1:]))
    assert expected("waiting")[2]["waiting_q"] == 2_470_000
    assert expected("infeasible_alone") == ("infeasible", [1, 4])
    assert expected("unreachable") == ("infeasible", [2, 3])
    assert expected("reject_float_walk")[2]["rejected"] >= 1 and expected("reject_float_walk")[2]["insertions"] >= 1
    assert expected("cap_float_reject")[2]["rejected"] >= 1
    assert len(expected("grid_cap_equal")[0]) == 4 and len(expected("grid_maxd_equal")[0]) == 2
    assert len(set(inst["seed_ties"]["close_q"][1:])) == 1
    trace = []
    tw_trips(trace=trace, **inst["seed_ties"])
    seeds = [trip[1] for trip, _, _, _ in trace if len(trip) == 3]
    assert len(seeds) == 4 and seeds == sorted(seeds) and seeds[0] == 1
    sp = inst["special_entries"]
    assert not np.isfinite(np.asarray(sp["d"])).all() and not np.isfinite(np.asarray(sp["t"])).all()
    q = usable_matrix(sp["d"])
    assert q[7, 8] == 1 << 50 and q[8, 7] == (1 << 31) - 2


def test_grid_ties_are_decided_by_the_rule():
    """On the grid many candidates tie on ``ins``; taking the largest (u, j) instead of the smallest
    among them gives other trips, so the rule is exercised."""
    c = named_instances()["grid_ties"]
    trace = []
    tw_trips(trace=trace, **c)
    q = usable_matrix(c["d"])
    tied = 0
    for trip, dep, z, unrouted in trace:
        cands = []
        for u in unrouted:
            for j in range(len(trip) - 1):
                a, b = trip[j], trip[j + 1]
                if time_admissible(usable_matrix(c["t"]), trip, dep, z, u, j, c["open_q"], c["close_q"], c["sv_q"]):
                    cands.append((int(q[a, u] + q[u, b] - q[a, b]), u, j))
        if cands:
            best = min(cands)[0]
            tied += sum(1 for x in cands if x[0] == best) > 1
    assert tied >= 5


# --------------------------------------------------------------------------- O(1) test vs re-simulation
def _check_every_candidate(c):
    """Every (u, j) of every scan: the O(1) time test == re-simulating the lengthened trip."""
    trace = []
    try:
        tw_trips(trace=trace, **c)
    except InfeasibleStops:
        return 0, 0
    qt = usable_matrix(c["t"])
    n = yes = 0
    for trip, dep, z, unrouted in trace:
        assert resimulate(c, trip)[0]
        for u in unrouted:
            for j in range(len(trip) - 1):
                fast = time_admissible(qt, trip, dep, z, u, j, c["open_q"], c["close_q"], c["sv_q"])
                new = trip[:j + 1] + [u] + trip[j + 1:]
                # the distance entries play no part in the time test: mask them out of the oracle
                slow = resimulate(dict(c, d=np.zeros_like(np.asarray(c["t"])).tolist()), new)[0]
                assert fast == slow, (trip, u, j)
                n += 1
                yes += fast
    return n, yes


def test_admissibility_equals_resimulation_on_every_candidate():
    n = yes = 0
    for seed in range(300):
        ns = 1 + seed % 14
        a, b = _check_every_candidate(random_instance(ns, 40_000 + seed, road=True))
        n, yes = n + a, yes + b
    for name in NAMES:
        if len(named_instances()[name]["d"]) <= 41:
            a, b = _check_every_candidate(named_instances()[name])
            n, yes = n + a, yes + b
    assert n > 20_000 and 0.05 < yes / n < 0.95, (n, yes)


# --------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    c = named_instances()[name]
    want = expected(name)
    ns = len(c["d"]) - 1
    if want[0] == "infeasible":
        assert want[1] == sorted(want[1]) and want[1]
        return
    trips, schedule, st = want
    assert sorted(s for t in trips for s in t[1:-1]) == list(range(1, ns + 1))
    assert st["trips"] == len(trips) and st["insertions"] == ns - len(trips)
    d = np.asarray(c["d"], dtype=np.float64)
    q = usable_matrix(d)
    assert st["len_q"] == sum(int(q[t[p], t[p + 1]]) for t in trips for p in range(len(t) - 1))
    wait = 0
    for t, rows in zip(trips, schedule):
        assert t[0] == 0 and t[-1] == 0 and len(t) >= 3
        ok, sim = resimulate(c, t)
        assert ok and sim == rows
        for s, arr, start, dep in rows:
            assert c["open_q"][s] <= start <= c["close_q"][s] and arr <= start and dep == start + c["sv_q"][s]
            wait += start - arr
        assert [r[1] for r in rows] == sorted(r[1] for r in rows)
        # the limits by the greedy's own float64 accumulation
        assert walk_feasible(d, t, c["max_dist"]) and load_feasible(c["demand"], t, c["cap"])
    assert wait == st["waiting_q"]


# --------------------------------------------------------------------------- requests without the fields
def _cluster(lat0, lon0, n=10, cap=4, **extra):
    dests = [{"lat": lat0 + (0.004 + 0.0015 * (i // 2)) * (1 if i % 2 else -1), "lon": lon0 + 0.0005 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": cap,
                            "maximum_distance": 1e6}}
    p.update(extra)
    return p


def _with_windows(p, windows=None, service=None):
    p = json.loads(json.dumps(p))
    for i, w in (windows or {}).items():
        p["destination_points"][i]["time_window"] = list(w)
    for i, s in (service or {}).items():
        p["destination_points"][i]["service"] = s
    return p


def test_requests_without_the_fields_are_answered_as_before():
    from routest_amd.routing.batched import batched_trips
    from routest_amd.routing.optimizer import multi_stop, optimize_many, optimize_route
    from routest_amd.routing.providers import HaversineProvider
    prov = HaversineProvider()
    reqs = [_cluster(14.58, 121.04), _cluster(14.6, 121.0, n=7, cap=3, improve=True),
            _cluster(14.5, 121.1, n=12, exchange=True), _cluster(14.58, 121.04, n=1)]
    assert not any(wants_time_windows(r) for r in reqs)
    # the same objects as the calls that never pass the new arguments
    plain = [optimize_route(r, prov, "e") for r in reqs]
    for r, want in zip(reqs, plain):
        assert "schedule" not in want["properties"] and "time_windows" not in want["properties"]
        drv = r["driver_details"]
        if len(r["destination_points"]) > 1:
            f = multi_stop(prov, r["source_point"], r["destination_points"], "driving-car", drv,
                           improve=r.get("improve") is True, exchange=r.get("exchange") is True)
            assert f["properties"]["summary"] == want["properties"]["summary"]
            assert f["properties"].get("improvement") == want["properties"].get("improvement")
    assert optimize_many(reqs, prov, "e") == plain
    multi = reqs[:3]
    flags = dict(improve=[False, True, False], exchange=[False, False, True])
    base = batched_trips(multi, **flags)
    assert batched_trips(multi, time_windows=[None] * 3, **flags)[:2] == base
    assert batched_trips(multi, time_windows=[None] * 3, **flags)[2] == [None] * 3
    assert batched_trips(multi, time_windows=[None] * 3)[0] == batched_trips(multi)
    # unflagged rows beside a flagged one take today's path
    twr = _with_windows(_cluster(14.58, 121.04, n=5), {0: (0, 5000)}, {1: 60})
    mixed = batched_trips(multi + [twr], time_windows=[None] * 3 + [parse_time_windows(twr)],
                          improve=flags["improve"] + [True], exchange=flags["exchange"] + [True])
    assert mixed[0][:3] == base[0] and mixed[1][:3] == base[1] and mixed[1][3] is None
    assert mixed[2][:3] == [None] * 3 and mixed[2][3] is not None


# --------------------------------------------------------------------------- API contract
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


def _tw_body(lat0, lon0, **extra):
    """Six stops: two must be served late (the vehicle waits), one early, and unloading takes time."""
    return _with_windows(_cluster(lat0, lon0, n=6, cap=99, **extra),
                         {0: (3600, 4000), 3: (0, 1800), 5: (7200, 7200.5)}, {0: 300, 2: 120.5, 5: 0})


@pytest.mark.parametrize("path", ["/api/optimize_route", "/route", "/api/request_route"])
def test_api_response_shape_and_schedule(client, path):
    c, sv, lat0, lon0 = client
    body = _tw_body(lat0, lon0)
    plain = _post(c, path, _cluster(lat0, lon0, n=6, cap=99))
    out = _post(c, path, body)
    props = out["properties"]
    assert set(props) - {"schedule", "time_windows"} == set(plain["properties"])
    tw = props["time_windows"]
    assert list(tw) == ["method", "stops_with_windows", "trips", "waiting"]
    assert tw["method"] == "cheapest_insertion" and tw["stops_with_windows"] == 3
    assert tw["trips"] == len(props["schedule"]) == props["summary"]["trips"]
    assert [e["destination"] for trip in props["schedule"] for e in trip] == props["optimized_order"]
    assert sorted(props["optimized_order"]) == list(range(6))
    waiting = 0.0
    for trip in props["schedule"]:
        clock = 0.0
        for e in trip:
            assert list(e) == ["destination", "arrival", "start", "departure", "waiting"]
            p = body["destination_points"][e["destination"]]
            lo, hi = p.get("time_window", [0, float("inf")])
            assert clock <= e["arrival"] <= e["start"] <= e["departure"] and lo <= e["start"] <= hi
            assert e["start"] == max(e["arrival"], lo)
            assert abs(e["departure"] - e["start"] - p.get("service", 0)) < 1e-9
            assert abs(e["waiting"] - (e["start"] - e["arrival"])) < 1e-9
            waiting += e["waiting"]
            clock = e["departure"]
    assert abs(waiting - tw["waiting"]) < 1e-6 and tw["waiting"] > 0
    # improve / exchange are ignored on a time-window request
    for extra in ({"improve": True}, {"exchange": True}, {"improve": True, "exchange": True}):
        assert _post(c, path, _tw_body(lat0, lon0, **extra)) == out
    if sv.provider.name != "haversine":
        return          # the road matrices depend on the week-hour the request is routed in
    # the reference on the provider's own matrices gives these trips
    pts =[body["source_point"]] + body["destination_points"]
    sec, met = sv.provider.time_matrix(pts, "driving-car")
    trips, _, st = tw_trips(met, sec, [0.0] + [1.0] * 6, 99.0, 1e6, *parse_time_windows(body))
    assert [s - 1 for t in trips for s in t[1:-1]] == props["optimized_order"]
    assert tw["waiting"] == st["waiting_q"] / 1000.0


def test_api_single_destination_and_alternatives_ignore_the_fields(client):
    c, sv, lat0, lon0 = client
    def echo_free(f):
        # the response echoes the destinations as they were sent: compare without the new keys
        for p in f["properties"]["destinations"]:
            p.pop("time_window", None)
            p.pop("service", None)
        return f
    one = _cluster(lat0, lon0, n=1)
    want = _post(c, "/api/optimize_route", one)
    assert echo_free(_post(c, "/api/optimize_route", _with_windows(one, {0: (0, 1)}, {0: 5}))) == want
    assert echo_free(_post(c, "/api/optimize_route", _with_windows(one, {0: "never"}))) == want
    if sv.provider.name != "graph":
        return          # alternatives need the road graph
    body = _cluster(lat0, lon0, n=4, alternatives=3)
    a = c.post("/api/optimize_route", json=body)
    b = c.post("/api/optimize_route", json=_with_windows(body, {0: (0, 1)}))
    assert a.status_code == b.status_code == 200 and echo_free(b.json()) == a.json()
    assert "schedule" not in b.json()["properties"]


BAD_FIELDS = [("time_window", [5]), ("time_window", [1, 2, 3]), ("time_window", "9-11"), ("time_window", None),
              ("time_window", [10, 5]), ("time_window", [-1, 5]), ("time_window", [0, 2_000_001]),
              ("time_window", ["0", 5]), ("time_window", [True, 5]), ("time_window", {"open": 0}),
              ("service", -1), ("service", "5"), ("service", None), ("service", 2_000_001), ("service", [5]),
              ("service", True)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_api_malformed_fields_are_a_400_naming_the_field(client, field, value):
    c, sv, lat0, lon0 = client
    body = _cluster(lat0, lon0, n=4)
    body["destination_points"][2][field] = value
    for path in ("/api/optimize_route", "/route"):
        r = c.post(path, json=body)
        assert r.status_code == 400, r.text
        err = r.json()["error"]
        assert field in err and "destination_points[2]" in err and "Traceback" not in err
    res = _post(c, "/api/optimize_routes_batch", {"requests": [body, _cluster(lat0, lon0, n=4)]})["results"]
    assert field in res[0]["error"] and "error" not in res[1]


def test_api_non_finite_numbers_are_refused():
    for v in (float("nan"), float("inf")):
        for body in ({"time_window": [0, v]}, {"service": v}):
            p = {"destination_points": [dict(lat=0, lon=0, **body), dict(lat=0, lon=1)]}
            with pytest.raises(ValueError):
                parse_time_windows(p)
    ok = {"destination_points": [dict(lat=0, lon=0, time_window=[0, 2_000_000], service=2_000_000), dict(lat=0, lon=1)]}
    assert parse_time_windows(ok) == ([0, 0, 0], [UNBOUNDED, 2_000_000_000, UNBOUNDED], [0, 2_000_000_000, 0])


def test_api_more_than_128_destinations_is_a_400(client):
    c, sv, lat0, lon0 = client
    if sv.provider.name != "haversine":
        return          # the limit is checked before any provider is asked
    body = _with_windows(_cluster(lat0, lon0, n=129, cap=999), service={0: 5})
    r = c.post("/api/optimize_route", json=body)
    assert r.status_code == 400 and "destination_points" in r.json()["error"] and "128" in r.json()["error"]
    body = _with_windows(_cluster(lat0, lon0, n=128, cap=999), service={0: 5})
    assert _post(c, "/api/optimize_route", body)["properties"]["time_windows"]["trips"] == 1


def test_api_infeasible_alone_message(client):
    c, sv, lat0, lon0 = client
    body = _with_windows(_cluster(lat0, lon0, n=5, cap=99), {3: (0, 0.001), 1: (0, 0)})
    for path in ("/api/optimize_route", "/route", "/api/request_route"):
        r = c.post(path, json=body)
        # (/api/request_route reports optimizer errors with the status its compatibility setting picks)
        compat = path == "/api/request_route" and sv.settings.compat_request_route_200
        assert r.status_code == (200 if compat else 400)
        err = r.json()["error"]
        assert "or its time window cannot be met" in err and err.endswith("destination indices [1, 3]")
    # payload over capacity is reported on the same path, and requests without the fields keep their text
    heavy = _with_windows(_cluster(lat0, lon0, n=5, cap=99), service={0: 1})
    heavy["destination_points"][4]["payload"] = 500
    assert c.post("/api/optimize_route", json=heavy).json()["error"].endswith("destination indices [4]")
    heavy["destination_points"][0].pop("service")
    err = c.post("/api/optimize_route", json=heavy).json()["error"]
    assert "time window" not in err and err.endswith("destination indices [4]")
    res = _post(c, "/api/optimize_routes_batch", {"requests": [body]})["results"]
    assert "or its time window cannot be met" in res[0]["error"]


def test_api_batch_takes_the_fields_per_request(client):
    c, sv, lat0, lon0 = client
    reqs = [_cluster(lat0, lon0), _tw_body(lat0, lon0), _cluster(lat0, lon0, improve=True),
            _with_windows(_cluster(lat0, lon0, n=1), {0: (0, 1)})]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs})["results"]
    assert ["schedule" in r["properties"] for r in res] == [False, True, False, False]
    for k in range(4):
        assert res[k] == _post(c, "/api/request_route", reqs[k])


def test_unsupported_provider_and_engine_are_a_400():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.providers import ORSProvider
    from routest_amd.serve.eta_service import EtaService, default_model
    body = _tw_body(14.58, 121.04)

    class NoNetwork:
        def post(self, *a, **k):
            raise AssertionError("a time-window request must not reach the remote provider")
    out = optimize_route(body, ORSProvider("key", session=NoNetwork()), "e")
    assert "time_window" in out["error"] and "service" in out["error"]
    g = synth_road_graph(400, seed=3)
    prov = GraphProvider(g, (g.length_m / 9.0).astype(np.float32), device=None, engine="astar")
    lat0, lon0 = float(np.median(g.lat)), float(np.median(g.lon))
    s = load_settings(env={}, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(default_model(hidden=64, steps=20), device="cpu"), provider=prov, store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/optimize_route", json=_tw_body(lat0, lon0))
        assert r.status_code == 400 and "time_window" in r.json()["error"], r.text
        assert c.post("/api/optimize_route", json=_cluster(lat0, lon0, n=4)).status_code == 200
    sv.close()


def test_batcher_plans_time_window_requests_like_the_app(client):
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.route_batcher import RouteBatcher
    c, sv, lat0, lon0 = client
    reqs = [_cluster(lat0, lon0), _tw_body(lat0, lon0), _tw_body(lat0, lon0, improve=True),
            _with_windows(_cluster(lat0, lon0, n=5, cap=99), {3: (0, 0.001)}), _cluster(lat0, lon0, exchange=True)]
    b = RouteBatcher(sv.provider, "e", devices=[None])
    try:
        plans = b.plan_batch(reqs)
        assert [len(p) for p in plans] == [4, 5, 5, 4, 4]
        got = [b.assemble(r, p) for r, p in zip(reqs, plans)]
    finally:
        b.close()
    if sv.provider.name == "haversine":
        assert got == [optimize_route(r, sv.provider, "e") for r in reqs]
    assert "schedule" in got[1]["properties"] and got[1] == got[2]
    assert "or its time window cannot be met" in got[3]["error"]
    assert "schedule" not in got[0]["properties"] and "improvement" in got[4]["properties"]


# --------------------------------------------------------------------------- native front end
def test_native_front_end_hands_time_window_requests_to_the_app():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    body = _cluster(14.58, 121.04, n=3)
    plain = rt.route_optimize_cpu(json.dumps(body).encode())
    assert plain is not None and plain[0] == 200
    for w, s in (({0: (0, 100)}, None), (None, {2: 5}), ({1: "bad"}, None), (None, {0: None})):
        assert rt.route_optimize_cpu(json.dumps(_with_windows(body, w, s)).encode()) is None
    # single-destination requests ignore the fields: answered natively, with the plain bytes
    one = _cluster(14.58, 121.04, n=1)
    assert rt.route_optimize_cpu(json.dumps(_with_windows(one, {0: (0, 1)})).encode()) is not None
    other = json.loads(json.dumps(body))
    other["destination_points"][0]["note"] = "ring twice"
    assert rt.route_optimize_cpu(json.dumps(other).encode()) is not None
