"""The unit-relocate search on shipment trips (routing/shipment_improve.py) against the host C++
(``_rt.pd_improve``), its fast tests against the re-simulation definition candidate by candidate, the
invariants of its output, and the request field ``shipment_improve`` through the API.  Instances:
tests/_pd_improve_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.shipment_improve import METHOD, STAT_KEYS, moved_trips, wants_shipment_improve
from routest_amd.routing.shipments import PICKUP, PLAIN, kinds_of, load_profile, parse_shipments, pd_trips
from routest_amd.routing.improve import quantize
from routest_amd.routing.timewindows import limit_q, parse_time_windows

from _pd_cases import paired
from _pd_improve_cases import built, expected, improve, named_instances, skip_cases, traced
from _tw_cases import random_instance, resimulate

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = sorted(named_instances())
TRACED = [n for n in NAMES if len(named_instances()[n]["d"]) - 1 <= 16]


@pytest.fixture(scope="module")
def rt():
    from routest_amd.ops import _ext
    return _ext.runtime(required=True)


def _rt_answer(rt, c, trips):
    got = rt.pd_improve(np.asarray(c["d"], dtype=np.float64), np.asarray(c["t"], dtype=np.float64), trips, c["demand"],
                        c["cap"], c["max_dist"], c["open_q"], c["close_q"], c["sv_q"], c["pickup_from"])
    return ([list(t) for t in got[0]], [[tuple(e) for e in trip] for trip in got[1]], dict(got[2]))


def test_host_cpp_equals_reference_on_every_instance(rt):
    for name in NAMES:
        c = named_instances()[name]
        got = _rt_answer(rt, c, built(c))
        assert got == expected(name)[:3], name
        assert list(got[2]) == list(STAT_KEYS)


def test_host_cpp_equals_reference_on_random_instances(rt):
    moved = pairs = 0
    for k in range(140):
        ns = 1 + k % 48
        c = paired(random_instance(ns, 60_000 + k, windowed=(0.7, 0.3)[k % 2], road=bool(k % 3 == 0),
                                   cap_frac=(None, 0.3)[k % 4 == 0]), k, frac=(0.5, 1.0)[k % 5 == 0])
        trips = built(c)
        if trips is None:
            continue
        want = improve(c, trips)
        assert _rt_answer(rt, c, trips) == want, (k, ns)
        moved += want[2]["moves"] > 0
        pairs += want[2]["pair_moves"] > 0
    assert moved > 60 and pairs > 30


def test_skip_conditions(rt):
    """More than 128 stops, a negative fixed-point limit, an unusable demand on a plain stop or a
    delivery: the trips come back as given, with 0 moves."""
    for name, (c, trips) in skip_cases().items():
        out, sched, st = improve(c, trips)
        assert out == trips and st["moves"] == st["rejected"] == 0 and st["trips_after"] == len(trips), name
        assert st["len_before_q"] == st["len_after_q"], name
        assert _rt_answer(rt, c, trips) == (out, sched, st), name
    # the same trips on the sound sibling are improved
    from _pd_cases import named_instances as pd_named
    base = pd_named()["cap_bound_ns20"]
    assert improve(base, skip_cases()["cap_nan"][1])[2]["moves"] > 0
    # a pickup's own demand is never read: an unusable one does not skip the stage
    pk = next(s for s in range(1, 21) if s in base["pickup_from"])
    odd = dict(base, demand=[float("nan") if s == pk else x for s, x in enumerate(base["demand"])])
    assert improve(odd, built(base))[:2] == improve(base)[:2]


@pytest.mark.parametrize("name", TRACED)
def test_fast_tests_equal_resimulation_on_every_candidate(name):
    """The slow path prices every candidate of the definition's ranges twice: by the fast tests the
    host C++ and the kernel evaluate, and by re-simulating the touched trips.  Verdicts agree on
    every candidate, gains on every admissible one; the chosen move is the admissible one of
    largest gain and smallest code; and the slow path returns what the bulk path returns."""
    c = named_instances()[name]
    trace, applied = traced(c)
    assert tuple(applied) == expected(name)[3]
    assert len(trace) in (len(applied), len(applied) + 1)
    for x, (trips, seen) in enumerate(trace):
        moves = [m for m, *_ in seen]
        assert moves == sorted(set(moves))
        for m, g, tests, ok, dg, dok in seen:
            assert ok == dok, (name, m, tests)
            if dok:
                assert g == dg, (name, m)
        good = [(-g, m) for m, g, _, ok, _, _ in seen if ok and g > 0]
        if x < len(applied):
            assert good and min(good)[1] == applied[x]
        else:
            assert not good or expected(name)[2]["rejected"] == 1 or len(applied) == 4 * (len(c["d"]) - 1)


def test_candidate_ranges():
    """The slow path's candidates are exactly the definition's ranges."""
    c = named_instances()["cap_bound_ns20"]
    kind, mate = kinds_of(c["pickup_from"], len(c["d"]))
    trips, seen = traced(c)[0][0]
    want = set()
    for A, a in enumerate(trips):
        for x in range(1, len(a) - 1):
            u = a[x]
            if kind[u] not in (PLAIN, PICKUP):
                continue
            size = 2 if kind[u] == PICKUP else 1
            for B, b in enumerate(trips):
                k = len(b) - 2 - (size if B == A else 0)
                if k < 1:
                    continue
                for i in range(k + 1):
                    for j in range(i, k + 1) if size == 2 else (i,):
                        want.add((int(B == A), A, x, B, i, j))
    assert {m for m, *_ in seen} == want


def _check_invariants(c, trips, schedule, st, given):
    n1 = len(c["d"])
    kind, mate = kinds_of(c["pickup_from"], n1)
    assert sorted(s for t in trips for s in t[1:-1]) == list(range(1, n1))
    qd = [0] + [quantize(c["demand"][s]) for s in range(1, n1)]
    cap_q = limit_q(c["cap"])
    pos = {s: (t, x) for t, trip in enumerate(trips) for x, s in enumerate(trip) if s}
    for s in range(1, n1):
        if kind[s] == PICKUP:
            assert pos[s][0] == pos[mate[s]][0] and pos[s][1] < pos[mate[s]][1]
    waiting = 0
    for trip, rows in zip(trips, schedule):
        assert trip[0] == trip[-1] == 0 and len(trip) > 2
        ok, want = resimulate(c, trip)
        assert ok and [tuple(r) for r in rows] == [tuple(r) for r in want]
        waiting += sum(b - a for _, a, b, _ in rows)
        if trip not in given:          # a trip the search touched passed the integer tests
            assert max(load_profile(qd, kind, mate, trip)) <= cap_q
    assert st["waiting_q"] == waiting and st["trips_after"] == len(trips) and st["trips_before"] == len(given)
    assert st["len_after_q"] <= st["len_before_q"] and st["moves"] <= 4 * (n1 - 1)
    assert (st["len_after_q"] < st["len_before_q"]) == (st["moves"] > 0)


@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    c = named_instances()[name]
    trips, schedule, st, applied = expected(name)
    _check_invariants(c, trips, schedule, st, built(c))
    # the applied sequence, replayed by the definition, ends in the trips that came out
    kind, mate = kinds_of(c["pickup_from"], len(c["d"]))
    cur = built(c)
    for mv in applied:
        for t, o in moved_trips(cur, kind, mate, mv).items():
            cur[t] = o
    assert [t for t in cur if len(t) > 2] == trips and len(applied) == st["moves"]
    assert sum(1 for t in cur if len(t) == 2) == st["trips_before"] - st["trips_after"]


def test_without_pairs_it_never_lengthens_and_keeps_every_window():
    for k in range(30):
        c = dict(random_instance(4 + k, 61_000 + k, windowed=0.6, cap_frac=(None, 0.3)[k % 2]),
                 pickup_from=[-1] * (5 + k))
        trips = built(c)
        if trips is None:
            continue
        out, sched, st = improve(c, trips)
        _check_invariants(c, out, sched, st, trips)
        for rows in sched:
            for s, _, start, _ in rows:
                assert c["open_q"][s] <= start <= c["close_q"][s]
        assert st["pair_moves"] == 0


def test_instances_cover_the_issue():
    """The named instances jointly apply both move types on both unit kinds, one empties a trip, one
    is rejected; the constructed ones show what they were built for."""
    seen = set()
    for name in NAMES:
        c = named_instances()[name]
        kind, mate = kinds_of(c["pickup_from"], len(c["d"]))
        cur = built(c)
        for mv in expected(name)[3]:
            seen.add((mv[0], kind[cur[mv[1]][mv[2]]]))
            for t, o in moved_trips(cur, kind, mate, mv).items():
                cur[t] = o
    assert seen == {(0, PLAIN), (0, PICKUP), (1, PLAIN), (1, PICKUP)}
    st = expected("empties_trip")[2]
    assert st["trips_after"] < st["trips_before"] and st["moves"] > 0
    st = expected("float_reject_move")[2]
    assert st["rejected"] == 1
    assert any(mv[0] == 0 and mv[5] > mv[4] for mv in expected("separated_only_move")[3])
    assert expected("load_max")[2]["moves"] > 0 and expected("grid_tie_move")[2]["moves"] > 0
    # the removal that would make the next stop late: inadmissible by the removal test alone
    c = named_instances()["late_after_removal"]
    assert any(g > 0 and not t["removal"] and t["target"] and t["insertion"] and t["length"]
               for _, seen_ in traced(c)[0] for m, g, t, *_ in seen_ if m[0] == 0)


# --------------------------------------------------------------------------- the request field
def test_wants_shipment_improve_is_json_true_exactly():
    assert wants_shipment_improve({"shipment_improve": True})
    for v in (1, "true", 1.0, None, False, [True], {"a": 1}):
        assert not wants_shipment_improve({"shipment_improve": v})
    assert not wants_shipment_improve({}) and not wants_shipment_improve(None) and not wants_shipment_improve([1])


def _cluster(lat0, lon0, n=10, cap=4, **extra):
    dests = [{"lat": lat0 + (0.004 + 0.0015 * (i // 2)) * (1 if i % 2 else -1), "lon": lon0 + 0.0005 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": cap,
                            "maximum_distance": 1e6}}
    p.update(extra)
    return p


PAIRS = {1: 4, 5: 0, 9: 6}      # delivery: pickup, 0-based destination indices


def _pd_body(lat0, lon0, **extra):
    """Twelve stops on both sides of the depot, three pairs across them, a late stop and two service
    times: the insertion's trips leave the search something to do."""
    p = _cluster(lat0, lon0, n=12, cap=3, **extra)
    for v, pk in PAIRS.items():
        p["destination_points"][v]["pickup_from"] = pk
        p["destination_points"][pk].pop("payload", None)
    p["destination_points"][3]["time_window"] = [3600, 4000]
    p["destination_points"][4]["service"] = 120
    p["destination_points"][2]["service"] = 60.5
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
def test_api_contract(client, path):
    c, sv, lat0, lon0 = client
    plain = _post(c, path, _pd_body(lat0, lon0))
    out = _post(c, path, _pd_body(lat0, lon0, shipment_improve=True))
    props, tw = out["properties"], out["properties"]["time_windows"]
    assert set(props) == set(plain["properties"])
    assert list(tw) == ["method", "stops_with_windows", "trips", "waiting", "moves", "pair_moves", "trips_before",
                        "matrix_distance_before", "matrix_distance_after"]
    assert tw["method"] == METHOD == "cheapest_insertion+unit_relocate" and tw["stops_with_windows"] == 1
    assert tw["trips_before"] == plain["properties"]["time_windows"]["trips"] >= tw["trips"] == len(props["schedule"])
    assert tw["matrix_distance_after"] <= tw["matrix_distance_before"] and 0 <= tw["pair_moves"] <= tw["moves"]
    assert (tw["moves"] > 0) == (tw["matrix_distance_after"] < tw["matrix_distance_before"])
    assert [e["destination"] for trip in props["schedule"] for e in trip] == props["optimized_order"]
    assert sorted(props["optimized_order"]) == list(range(12))
    kinds = {pk: "pickup" for pk in PAIRS.values()}
    kinds.update({v: "delivery" for v in PAIRS})
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
                assert PAIRS[s] in order[:order.index(s)]
        assert load == 0.0
    assert props["shipments"] == {"pairs": 3, "max_load": top} and top <= 3.0
    if sv.provider.name != "haversine":
        return          # the road matrices depend on the week-hour the request is routed in
    assert tw["moves"] > 0
    body = _pd_body(lat0, lon0)
    pts = [body["source_point"]] + body["destination_points"]
    sec, met = sv.provider.time_matrix(pts, "driving-car")
    dem = [0.0] + [float(p.get("payload", 0)) for p in body["destination_points"]]
    args = (dem, 3.0, 1e6, *parse_time_windows(body), parse_shipments(body))
    from routest_amd.routing.shipment_improve import pd_improve_trips
    trips, _, st = pd_improve_trips(met, sec, pd_trips(met, sec, *args)[0], *args)
    assert [s - 1 for t in trips for s in t[1:-1]] == props["optimized_order"]
    assert tw["waiting"] == st["waiting_q"] / 1000.0 and tw["moves"] == st["moves"]
    assert tw["matrix_distance_after"] == st["len_after_q"] / 1000.0


def test_api_without_the_field_nothing_changes(client):
    """A shipment request without ``shipment_improve: true`` is answered as the insertion alone
    answers it, byte for byte; so is one with any value but JSON true, and with ``tw_improve`` alone.
    Requests that are no shipment requests ignore the field."""
    c, sv, lat0, lon0 = client
    base = c.post("/api/optimize_route", json=_pd_body(lat0, lon0))
    assert base.status_code == 200
    assert list(base.json()["properties"]["time_windows"]) == ["method", "stops_with_windows", "trips", "waiting"]
    assert base.json()["properties"]["time_windows"]["method"] == "cheapest_insertion"
    for extra in ({"shipment_improve": False}, {"shipment_improve": 1}, {"shipment_improve": "true"},
                  {"shipment_improve": None}, {"tw_improve": True}, {"improve": True, "exchange": True, "tw_improve": True}):
        assert c.post("/api/optimize_route", json=_pd_body(lat0, lon0, **extra)).content == base.content, extra
    # improve / exchange / tw_improve stay ignored beside the field
    want = c.post("/api/optimize_route", json=_pd_body(lat0, lon0, shipment_improve=True)).content
    assert want != base.content
    both = _pd_body(lat0, lon0, shipment_improve=True, improve=True, exchange=True, tw_improve=True)
    assert c.post("/api/optimize_route", json=both).content == want
    # no shipment request: a plain one, a time-window one, a single destination
    tw = _cluster(lat0, lon0, n=6)
    tw["destination_points"][2]["time_window"] = [0, 9000]
    for body in (_cluster(lat0, lon0), tw, _cluster(lat0, lon0, n=1), dict(tw, tw_improve=True)):
        a = c.post("/api/optimize_route", json=body)
        b = c.post("/api/optimize_route", json=dict(body, shipment_improve=True))
        assert a.status_code == 200 and a.content == b.content


def test_api_batch_takes_the_field_per_request(client):
    c, sv, lat0, lon0 = client
    tw = _cluster(lat0, lon0, n=5)
    tw["destination_points"][2]["service"] = 30
    reqs = [_cluster(lat0, lon0, shipment_improve=True), _pd_body(lat0, lon0), _pd_body(lat0, lon0, shipment_improve=True),
            dict(tw, shipment_improve=True), _pd_body(lat0, lon0, tw_improve=True),
            _pd_body(lat0, lon0, shipment_improve=True, tw_improve=True)]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs})["results"]
    methods = [r["properties"].get("time_windows", {}).get("method") for r in res]
    assert methods == [None, "cheapest_insertion", METHOD, "cheapest_insertion", "cheapest_insertion", METHOD]
    for k in range(len(reqs)):
        assert res[k] == _post(c, "/api/request_route", reqs[k])


def test_batcher_and_optimize_many_plan_the_field_like_the_app():
    """The batched planners (``optimize_many`` and the batcher's flush) on the CPU give what
    ``optimize_route`` gives, request by request."""
    from routest_amd.routing.optimizer import optimize_many, optimize_route
    from routest_amd.routing.providers import HaversineProvider
    from routest_amd.routing.route_batcher import RouteBatcher
    prov = HaversineProvider()
    reqs = [_pd_body(14.58, 121.04, shipment_improve=True), _pd_body(14.6, 121.0), _cluster(14.5, 121.1, improve=True),
            _pd_body(14.55, 121.02, shipment_improve=True, tw_improve=True)]
    want = [optimize_route(json.loads(json.dumps(r)), prov, "e") for r in reqs]
    assert [w["properties"].get("time_windows", {}).get("method") for w in want] == [METHOD, "cheapest_insertion", None, METHOD]
    assert optimize_many(reqs, prov, "e") == want
    b = RouteBatcher(prov, "e", devices=[None])
    try:
        plans = b.plan_batch(reqs)
        assert [len(p) for p in plans] == [5, 5, 4, 5]
        assert [b.assemble(r, p) for r, p in zip(reqs, plans)] == want
    finally:
        b.close()
