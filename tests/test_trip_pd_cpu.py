"""Pickup-and-delivery pairs (routing/shipments.py): the reference against the host C++
(``_rt.pd_trips``), against ``tw_trips`` where there are no pairs and against re-simulating every
candidate of every scan; the invariants of its trips; the request field through the API, the batched
paths, the batcher and the native parser.  Instances: tests/_pd_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.improve import quantize, walk_feasible
from routest_amd.routing.shipments import (DELIVERY, PICKUP, PLAIN, apply_insertion, kinds_of, parse_shipments,
                                           pd_load_feasible, pd_trips, wants_shipments)
from routest_amd.routing.timewindows import limit_q, parse_time_windows, tw_trips, usable_matrix

from _pd_cases import answer, expected, named_instances, only_failed, paired, scans
from _tw_cases import named_instances as tw_named_instances, random_instance, resimulate

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = sorted(named_instances())


def _rt_answer(rt, c):
    got = rt.pd_trips(np.asarray(c["d"], dtype=np.float64), np.asarray(c["t"], dtype=np.float64), c["demand"],
                      c["cap"], c["max_dist"], c["open_q"], c["close_q"], c["sv_q"], c["pickup_from"])
    if got[0] is None:
        return ("infeasible", list(got[1]))
    return ([list(t) for t in got[0]], [[tuple(e) for e in trip] for trip in got[1]], dict(got[2]))


@pytest.fixture(scope="module")
def rt():
    from routest_amd.ops import _ext
    return _ext.runtime(required=True)


def test_host_cpp_equals_reference_on_every_instance(rt):
    for name in NAMES:
        assert _rt_answer(rt, named_instances()[name]) == expected(name), name


def test_host_cpp_equals_reference_on_random_instances(rt):
    separated = 0
    for k in range(120):
        ns = 2 + k % 39
        c = paired(random_instance(ns, 40_000 + k, windowed=(0.7, 0.3)[k % 2], road=bool(k % 3 == 0),
                                   cap_frac=(None, 0.3)[k % 4 == 0]), k, frac=(0.5, 1.0)[k % 5 == 0])
        want = answer(c)
        assert _rt_answer(rt, c) == want, (k, ns)
        if want[0] != "infeasible":
            pos = {s: (t, x) for t, trip in enumerate(want[0]) for x, s in enumerate(trip) if s}
            separated += sum(1 for v, p in enumerate(c["pickup_from"]) if p > 0 and pos[v][1] > pos[p][1] + 1)
    assert separated > 20


def test_malformed_pickup_from_is_refused(rt):
    c = named_instances()["pair_plus_plain"]
    for pf in ([-1, 2, 3, -1], [-1, -1, 3, 3], [-1, 1, -1, -1], [-1, 4, -1, -1], [-1, 0, -1, -1],
               [-1, 3, -1, 2], [-1, -1, 1, 1]):
        with pytest.raises(ValueError):
            pd_trips(**dict(c, pickup_from=pf))
        with pytest.raises(ValueError):
            _rt_answer(rt, dict(c, pickup_from=pf))


def test_without_pairs_it_is_the_time_window_construction(rt):
    for name, c in tw_named_instances().items():
        try:
            want = tw_trips(**c)
        except InfeasibleStops as e:
            want = ("infeasible", e.stops)
        assert answer(dict(c, pickup_from=[-1] * len(c["d"]))) == want, name


# --------------------------------------------------------------------------- every candidate, re-simulated
def _resimulated(c, kind, mate, q, qd, cap_q, max_q, new):
    """Feasibility of a whole trip from scratch: the schedule (``_tw_cases.resimulate``), the load on
    leaving every position and the length."""
    ok, _ = resimulate(c, new)
    length = sum(int(q[a, b]) for a, b in zip(new[:-1], new[1:]))
    load = sum(qd[s] for s in new[1:-1] if kind[s] == PLAIN)
    top = load
    for s in new[1:-1]:
        load += qd[mate[s]] if kind[s] == PICKUP else -qd[s]
        top = max(top, load)
    return ok and top <= cap_q and length <= max_q, length


def _check_every_candidate(c):
    n1 = len(c["d"])
    q = usable_matrix(np.asarray(c["d"], dtype=np.float64))
    qd = [0] + [quantize(c["demand"][s]) for s in range(1, n1)]
    cap_q, max_q = limit_q(c["cap"]), limit_q(c["max_dist"])
    seen = admissible = 0
    for scan in scans(c):
        kind, mate, trip = scan["kind"], scan["mate"], scan["trip"]
        # the incremental tests assume a trip that is itself within the limits
        assert max(scan["load"]) <= cap_q and scan["Lq"] <= max_q
        assert scan["Lq"] == sum(int(q[a, b]) for a, b in zip(trip[:-1], trip[1:]))
        for (u, i, j), (ins, tests) in scan["candidates"].items():
            new = apply_insertion(trip, mate, kind, u, i, j)
            want, length = _resimulated(c, kind, mate, q, qd, cap_q, max_q, new)
            assert all(tests.values()) == want, (trip, u, i, j, tests)
            if tests["usable"]:
                assert scan["Lq"] + ins == length, (trip, u, i, j)
            seen += 1
            admissible += want
        # a best candidate that the next state does not show applied was rejected by a float walk
        if scan["best"] is not None and not scan["applied"]:
            new = apply_insertion(trip, mate, kind, *scan["best"][1:])
            assert not (walk_feasible(np.asarray(c["d"]), new, c["max_dist"])
                        and pd_load_feasible(c["demand"], kind, mate, new, c["cap"])), (trip, scan["best"])
    return seen, admissible


def test_admissibility_equals_resimulation_on_every_candidate():
    seen = admissible = 0
    for name in NAMES:
        if max(len(named_instances()[name]["d"]) - 1, 0) > 40 or name in ("amount_negative",):
            continue        # (a negative amount passes the float test alone and overloads its seed)
        a, b = _check_every_candidate(named_instances()[name])
        seen, admissible = seen + a, admissible + b
    for k in range(40):
        a, b = _check_every_candidate(paired(random_instance(2 + k % 12, 50_000 + k, road=bool(k % 2)), k))
        seen, admissible = seen + a, admissible + b
    assert seen > 5000 and admissible > 1000


def test_the_chosen_candidate_is_the_smallest_admissible_one():
    """The next state of every scan is the scalar enumeration's best candidate applied, or the trip
    was closed: by a float rejection or because nothing was admissible."""
    for name in NAMES:
        c = named_instances()[name]
        if len(c["d"]) - 1 > 40 or expected(name)[0] == "infeasible":
            continue
        sc = scans(c)
        trips = expected(name)[0]
        applied = sum(s["applied"] for s in sc)
        assert applied == expected(name)[2]["insertions"], name
        closed = [s["trip"] for s in sc if s["best"] is None]
        rejected = [s for s in sc if s["best"] is not None and not s["applied"]]
        assert len(rejected) == expected(name)[2]["rejected"], name
        assert all(t in trips for t in closed), name


def test_instances_cover_the_issue():
    far = adjacent = load_only = z_only = v_only = rejected = 0
    for name in NAMES:
        c = named_instances()[name]
        if len(c["d"]) - 1 > 40:
            continue
        if expected(name)[0] != "infeasible":
            rejected += expected(name)[2]["rejected"]
        for s in scans(c):
            if s["applied"] and s["kind"][s["best"][1]] == PICKUP:
                far += s["best"][3] > s["best"][2] + 1
                adjacent += s["best"][3] == s["best"][2]
            for (u, i, j), (_, tests) in s["candidates"].items():
                load_only += only_failed(tests, "load")
                if s["kind"][u] == PICKUP and j > i:
                    z_only += only_failed(tests, "z_u")
                    v_only += only_failed(tests, "time_v")
    assert far > 0 and adjacent > 0 and load_only > 0 and z_only > 0 and v_only > 0 and rejected > 0
    # the named situations are what their docstrings say
    sep = scans(named_instances()["separated_only"])[0]
    assert [k for k, (_, t) in sep["candidates"].items() if all(t.values())] == [(2, 0, 1)]
    adj = scans(named_instances()["adjacent_only"])[0]
    assert [k for k, (_, t) in adj["candidates"].items() if all(t.values())] == [(2, 1, 1)]
    zf = [s for s in scans(named_instances()["z_fail"]) if len(s["trip"]) == 4 and 3 in s["unrouted"]][0]
    assert all(not t["z_u"] for (u, i, j), (_, t) in zf["candidates"].items() if u == 3 and j > i)
    assert expected("z_fail")[0] == [[0, 1, 2, 3, 4, 0]]
    assert expected("infeasible_pair") == ("infeasible", [1, 4])
    assert expected("unreachable_mate") == ("infeasible", [0, 1, 3, 4])
    zw = expected("zero_width_delivery")
    assert [e for trip in zw[1] for e in trip if e[0] == 2][0][2] == 400_000 and zw[2]["waiting_q"] > 0
    assert expected("float_reject")[2]["rejected"] == 1
    assert expected("one_pair")[0] == [[0, 1, 2, 0]]


def test_grid_ties_are_decided_by_the_rule():
    ties = 0
    for name in ("grid_ties", "grid_ties_cap", "grid_ties_ns40"):
        for s in scans(named_instances()[name]):
            if s["best"] is None:
                continue
            same = [(ins, u, i, j) for (u, i, j), (ins, t) in s["candidates"].items()
                    if all(t.values()) and ins == s["best"][0]]
            ties += len(same) > 1
            assert min(same) == s["best"]
    assert ties > 10


@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    c = named_instances()[name]
    n1 = len(c["d"])
    kind, mate = kinds_of(c["pickup_from"], n1)
    got = expected(name)
    if got[0] == "infeasible":
        assert got[1] == sorted(set(got[1])) and all(0 <= s < n1 - 1 for s in got[1])
        for s in got[1]:
            if kind[s + 1] != PLAIN:
                assert mate[s + 1] - 1 in got[1]
        return
    trips, schedule, st = got
    assert sorted(s for t in trips for s in t[1:-1]) == list(range(1, n1))
    where = {s: (t, x) for t, trip in enumerate(trips) for x, s in enumerate(trip) if s}
    for s in range(1, n1):
        if kind[s] == PICKUP:
            assert where[s][0] == where[mate[s]][0] and where[s][1] < where[mate[s]][1]
    units = sum(1 for s in range(1, n1) if kind[s] != DELIVERY)
    assert st["insertions"] + st["trips"] == units and st["trips"] == len(trips)
    q = usable_matrix(np.asarray(c["d"], dtype=np.float64))
    waiting = length = 0
    for trip, rows in zip(trips, schedule):
        ok, sim = resimulate(c, trip)
        assert ok and [tuple(r) for r in rows] == sim
        assert walk_feasible(np.asarray(c["d"]), trip, c["max_dist"])
        assert pd_load_feasible(c["demand"], kind, mate, trip, c["cap"])
        waiting += sum(b - a for _, a, b, _ in rows)
        length += sum(int(q[a, b]) for a, b in zip(trip[:-1], trip[1:]))
    assert (st["len_q"], st["waiting_q"]) == (length, waiting)


def test_float_load_walk_without_pairs_is_the_plain_one():
    from routest_amd.routing.exchange import load_feasible
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 9))
        dem = [0.0] + [float(v) for v in rng.choice([0.1, 0.2, 0.3, 0.7, 1.1], n)]
        trip = [0] + [int(s) for s in rng.permutation(np.arange(1, n + 1))] + [0]
        cap = float(rng.choice([0.3, 0.6, 0.9, 1.2]))
        assert pd_load_feasible(dem, [PLAIN] * (n + 1), [0] * (n + 1), trip, cap) == load_feasible(dem, trip, cap)


# --------------------------------------------------------------------------- the request field
def _cluster(lat0, lon0, n=10, cap=4, **extra):
    dests = [{"lat": lat0 + (0.004 + 0.0015 * (i // 2)) * (1 if i % 2 else -1), "lon": lon0 + 0.0005 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": cap,
                            "maximum_distance": 1e6}}
    p.update(extra)
    return p


def _with_pairs(p, pairs, windows=None, service=None):
    """``pairs``: {delivery: pickup}, 0-based destination indices; the pickup's payload is dropped."""
    p = json.loads(json.dumps(p))
    for v, pk in pairs.items():
        p["destination_points"][v]["pickup_from"] = pk
        p["destination_points"][pk].pop("payload", None)
    for i, w in (windows or {}).items():
        p["destination_points"][i]["time_window"] = list(w)
    for i, s in (service or {}).items():
        p["destination_points"][i]["service"] = s
    return p


def _pd_body(lat0, lon0, **extra):
    """Seven stops: 4 -> 1 and 0 -> 5 are pairs, stop 3 is served late and unloading takes time."""
    return _with_pairs(_cluster(lat0, lon0, n=7, cap=3, **extra), {1: 4, 5: 0}, {3: (3600, 4000)}, {4: 120, 2: 60.5})


def test_requests_without_the_field_are_answered_as_before():
    from routest_amd.routing.batched import batched_trips
    from routest_amd.routing.optimizer import _tw_or_none, optimize_many, optimize_route
    from routest_amd.routing.providers import HaversineProvider
    prov = HaversineProvider()
    tw = _cluster(14.58, 121.04, n=5)
    tw["destination_points"][0]["time_window"] = [0, 5000]
    reqs = [_cluster(14.58, 121.04), _cluster(14.6, 121.0, n=7, cap=3, improve=True),
            _cluster(14.5, 121.1, n=12, exchange=True), _cluster(14.58, 121.04, n=1), tw]
    assert not any(wants_shipments(r) for r in reqs)
    assert [len(_tw_or_none(r) or ()) for r in reqs] == [0, 0, 0, 0, 3]
    plain = [optimize_route(r, prov, "e") for r in reqs]
    assert all("shipments" not in f["properties"] for f in plain)
    assert "type" not in plain[4]["properties"]["schedule"][0][0]
    assert optimize_many(reqs, prov, "e") == plain
    # unflagged rows beside a shipment row take today's path, whatever they ask for
    multi = reqs[:3] + [tw]
    flags = dict(improve=[False, True, False, True], exchange=[False, False, True, False])
    tws = [None, None, None, parse_time_windows(tw)]
    base = batched_trips(multi, time_windows=tws, **flags)
    ship = _pd_body(14.58, 121.04, improve=True, exchange=True, tw_improve=True)
    mixed = batched_trips(multi + [ship], time_windows=tws + [_tw_or_none(ship)], improve=flags["improve"] + [True],
                          exchange=flags["exchange"] + [True], tw_improve=[False] * 4 + [True])
    for x in range(3):
        assert mixed[x][:4] == base[x]
    assert mixed[1][4] is None and "search" not in mixed[2][4][1]


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
def test_api_response_shape(client, path):
    c, sv, lat0, lon0 = client
    body = _pd_body(lat0, lon0)
    plain = _post(c, path, _cluster(lat0, lon0, n=7, cap=3))
    out = _post(c, path, body)
    props = out["properties"]
    assert set(props) - {"schedule", "time_windows", "shipments"} == set(plain["properties"])
    assert list(props["time_windows"]) == ["method", "stops_with_windows", "trips", "waiting"]
    assert props["time_windows"]["method"] == "cheapest_insertion" and props["time_windows"]["stops_with_windows"] == 1
    assert list(props["shipments"]) == ["pairs", "max_load"] and props["shipments"]["pairs"] == 2
    assert [e["destination"] for trip in props["schedule"] for e in trip] == props["optimized_order"]
    assert sorted(props["optimized_order"]) == list(range(7))
    kinds = {4: "pickup", 1: "delivery", 0: "pickup", 5: "delivery"}
    top = 0.0
    for trip in props["schedule"]:
        order = [e["destination"] for e in trip]
        load = float(sum(1 for s in order if s not in kinds))
        top = max(top, load)
        for e in trip:
            assert list(e) == ["destination", "arrival", "start", "departure", "waiting", "type", "load"]
            s = e["destination"]
            assert e["type"] == kinds.get(s, "stop")
            load += 1.0 if e["type"] == "pickup" else -1.0
            top = max(top, load)
            assert e["load"] == load
            if e["type"] == "delivery":
                assert body["destination_points"][s]["pickup_from"] in order[:order.index(s)]
        assert load == 0.0
    assert props["shipments"]["max_load"] == top <= 3.0
    # improve / exchange / tw_improve are ignored on a shipment request
    for extra in ({"improve": True}, {"exchange": True}, {"tw_improve": True},
                  {"improve": True, "exchange": True, "tw_improve": True}):
        assert _post(c, path, _pd_body(lat0, lon0, **extra)) == out
    if sv.provider.name != "haversine":
        return          # the road matrices depend on the week-hour the request is routed in
    pts = [body["source_point"]] + body["destination_points"]
    sec, met = sv.provider.time_matrix(pts, "driving-car")
    dem = [0.0] + [float(p.get("payload", 0)) for p in body["destination_points"]]
    trips, _, st = pd_trips(met, sec, dem, 3.0, 1e6, *parse_time_windows(body), parse_shipments(body))
    assert [s - 1 for t in trips for s in t[1:-1]] == props["optimized_order"]
    assert props["time_windows"]["waiting"] == st["waiting_q"] / 1000.0


def test_api_single_destination_and_alternatives_ignore_the_field(client):
    c, sv, lat0, lon0 = client

    def echo_free(f):
        for p in f["properties"]["destinations"]:
            p.pop("pickup_from", None)
        return f
    one = _cluster(lat0, lon0, n=1)
    want = _post(c, "/api/optimize_route", one)
    bad = json.loads(json.dumps(one))
    bad["destination_points"][0]["pickup_from"] = "elsewhere"
    assert echo_free(_post(c, "/api/optimize_route", bad)) == want
    if sv.provider.name != "graph":
        return          # alternatives need the road graph
    body = _cluster(lat0, lon0, n=4, alternatives=3)
    other = json.loads(json.dumps(body))
    other["destination_points"][0]["pickup_from"] = 2
    a = c.post("/api/optimize_route", json=body)
    b = c.post("/api/optimize_route", json=other)
    assert a.status_code == b.status_code == 200 and echo_free(b.json()) == a.json()
    assert "shipments" not in b.json()["properties"]


def _bad_bodies(lat0, lon0):
    out = []
    for v in ("1", 1.0, True, None, [1], -1, 4, 2):                 # not an int, out of range, itself
        b = _cluster(lat0, lon0, n=4)
        b["destination_points"][1].pop("payload")
        b["destination_points"][2]["pickup_from"] = v
        out.append((2, b))
    b = _with_pairs(_cluster(lat0, lon0, n=4), {2: 1})
    b["destination_points"][1]["pickup_from"] = 0                    # the pickup itself carries the field
    b["destination_points"][0].pop("payload")
    out.append((2, b))
    b = _with_pairs(_cluster(lat0, lon0, n=4), {2: 1})
    b["destination_points"][3]["pickup_from"] = 1                    # the pickup of two deliveries
    out.append((3, b))
    b = _with_pairs(_cluster(lat0, lon0, n=4), {2: 1})
    b["destination_points"][1]["payload"] = 2                        # a pickup with a payload of its own
    out.append((2, b))
    return out


def test_api_malformed_fields_are_a_400_naming_the_field(client):
    c, sv, lat0, lon0 = client
    for i, body in _bad_bodies(lat0, lon0):
        for path in ("/api/optimize_route", "/route"):
            r = c.post(path, json=body)
            assert r.status_code == 400, (r.text, body["destination_points"])
            err = r.json()["error"]
            assert f"destination_points[{i}].pickup_from" in err and "Traceback" not in err
        res = _post(c, "/api/optimize_routes_batch", {"requests": [body, _cluster(lat0, lon0, n=4)]})["results"]
        assert "pickup_from" in res[0]["error"] and "error" not in res[1]
    # a pickup may say "payload": 0
    ok = _with_pairs(_cluster(lat0, lon0, n=4), {2: 1})
    ok["destination_points"][1]["payload"] = 0
    assert _post(c, "/api/optimize_route", ok)["properties"]["shipments"]["pairs"] == 1


def test_api_more_than_128_destinations_is_a_400(client):
    c, sv, lat0, lon0 = client
    if sv.provider.name != "haversine":
        return          # the limit is checked before any provider is asked
    r = c.post("/api/optimize_route", json=_with_pairs(_cluster(lat0, lon0, n=129, cap=999), {5: 6}))
    assert r.status_code == 400 and "destination_points" in r.json()["error"] and "128" in r.json()["error"]
    body = _with_pairs(_cluster(lat0, lon0, n=129, cap=999), {5: 6}, service={0: 5})
    assert c.post("/api/optimize_route", json=body).json() == r.json()


def test_api_infeasible_pair_message(client):
    c, sv, lat0, lon0 = client
    # the delivery 3 closes before the vehicle can come by way of its pickup 1 (which opens late)
    body = _with_pairs(_cluster(lat0, lon0, n=5, cap=99), {3: 1}, {1: (3000, 4000), 3: (0, 2000)})
    for path in ("/api/optimize_route", "/route", "/api/request_route"):
        r = c.post(path, json=body)
        compat = path == "/api/request_route" and sv.settings.compat_request_route_200
        assert r.status_code == (200 if compat else 400)
        err = r.json()["error"]
        assert "or its time window cannot be met" in err and err.endswith("destination indices [1, 3]")
    res = _post(c, "/api/optimize_routes_batch", {"requests": [body]})["results"]
    assert res[0]["error"].endswith("destination indices [1, 3]")
    # an amount over the capacity fails the pair, not only the delivery
    heavy = _with_pairs(_cluster(lat0, lon0, n=5, cap=99), {3: 1})
    heavy["destination_points"][3]["payload"] = 500
    assert c.post("/api/optimize_route", json=heavy).json()["error"].endswith("destination indices [1, 3]")


def test_api_batch_takes_the_field_per_request(client):
    c, sv, lat0, lon0 = client
    one = _cluster(lat0, lon0, n=1)
    one["destination_points"][0]["pickup_from"] = 0
    tw = _cluster(lat0, lon0, n=5)
    tw["destination_points"][2]["service"] = 30
    reqs = [_cluster(lat0, lon0), _pd_body(lat0, lon0), _cluster(lat0, lon0, improve=True), one, tw,
            _pd_body(lat0, lon0, tw_improve=True)]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs})["results"]
    assert ["shipments" in r["properties"] for r in res] == [False, True, False, False, False, True]
    assert ["schedule" in r["properties"] for r in res] == [False, True, False, False, True, True]
    for k in range(len(reqs)):
        assert res[k] == _post(c, "/api/request_route", reqs[k])


def test_unsupported_provider_and_engine_are_a_400():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.providers import ORSProvider
    from routest_amd.routing.shipments import NEEDS_MATRIX_TIMES
    from routest_amd.serve.eta_service import EtaService, default_model

    class NoNetwork:
        def post(self, *a, **k):
            raise AssertionError("a shipment request must not reach the remote provider")
    out = optimize_route(_pd_body(14.58, 121.04), ORSProvider("key", session=NoNetwork()), "e")
    assert out == {"error": NEEDS_MATRIX_TIMES} and "pickup_from" in out["error"]
    g = synth_road_graph(400, seed=3)
    prov = GraphProvider(g, (g.length_m / 9.0).astype(np.float32), device=None, engine="astar")
    lat0, lon0 = float(np.median(g.lat)), float(np.median(g.lon))
    s = load_settings(env={}, dotenv_path=None, device="cpu", route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(default_model(hidden=64, steps=20), device="cpu"), provider=prov, store=None)
    with TestClient(create_app(sv)) as c:
        r = c.post("/api/optimize_route", json=_pd_body(lat0, lon0))
        assert r.status_code == 400 and r.json()["error"] == NEEDS_MATRIX_TIMES, r.text
        assert c.post("/api/optimize_route", json=_cluster(lat0, lon0, n=4)).status_code == 200
    sv.close()


def test_batcher_plans_shipment_requests_like_the_app(client):
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.route_batcher import RouteBatcher
    c, sv, lat0, lon0 = client
    bad = _with_pairs(_cluster(lat0, lon0, n=5, cap=99), {3: 1}, {1: (3000, 4000), 3: (0, 2000)})
    malformed = _cluster(lat0, lon0, n=4)
    malformed["destination_points"][2]["pickup_from"] = 2
    reqs = [_cluster(lat0, lon0), _pd_body(lat0, lon0), _pd_body(lat0, lon0, improve=True, tw_improve=True), bad,
            _cluster(lat0, lon0, exchange=True), malformed]
    b = RouteBatcher(sv.provider, "e", devices=[None])
    try:
        plans = b.plan_batch(reqs)
        assert [len(p) for p in plans] == [4, 5, 5, 4, 4, 4]
        got = [b.assemble(r, p) for r, p in zip(reqs, plans)]
    finally:
        b.close()
    if sv.provider.name == "haversine":
        assert got == [optimize_route(r, sv.provider, "e") for r in reqs]
    assert got[1]["properties"]["shipments"]["pairs"] == 2 and got[1] == got[2]
    assert got[3]["error"].endswith("destination indices [1, 3]")
    assert "schedule" not in got[0]["properties"] and "improvement" in got[4]["properties"]
    assert "destination_points[2].pickup_from" in got[5]["error"]


def test_native_front_end_hands_shipment_requests_to_the_app(rt):
    body = _cluster(14.58, 121.04, n=3)
    plain = rt.route_optimize_cpu(json.dumps(body).encode())
    assert plain is not None and plain[0] == 200
    for v in (0, "bad", None, 7):
        other = json.loads(json.dumps(body))
        other["destination_points"][1]["pickup_from"] = v
        assert rt.route_optimize_cpu(json.dumps(other).encode()) is None
    # single-destination requests ignore the field: answered natively
    one = _cluster(14.58, 121.04, n=1)
    one["destination_points"][0]["pickup_from"] = 0
    assert rt.route_optimize_cpu(json.dumps(one).encode()) is not None
