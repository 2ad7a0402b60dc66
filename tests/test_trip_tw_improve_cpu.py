"""The window-aware local search on time-window trips (routing/tw_improve.py): the Python reference
against the host C++ (``_rt.tw_improve``), every O(1) time verdict against re-simulating the touched
trips, the invariants of the answer, the non-vacuity of the instance sets, and the ``tw_improve``
request field through the optimizer, the batched path, the batcher and the API.  Instances:
tests/_tw_improve_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.exchange import load_feasible
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.improve import walk_feasible
from routest_amd.routing.timewindows import parse_time_windows, tw_trips
from routest_amd.routing.tw_improve import STAT_KEYS, moved_trips, tw_improve_trips, wants_tw_improve

from _tw_cases import random_instance, resimulate
from _tw_improve_cases import LARGE, SMALL, built, expected, named_instances, opened, search_args, stops_of

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = [n for n in named_instances() if expected(n) is not None]


def _rt_answer(rt, case, trips):
    got = rt.tw_improve(np.asarray(case["d"], dtype=np.float64), np.asarray(case["t"], dtype=np.float64), trips,
                        case["demand"], case["cap"], case["max_dist"], case["open_q"], case["close_q"], case["sv_q"])
    return got[0], [[tuple(r) for r in trip] for trip in got[1]], dict(got[2])


# --------------------------------------------------------------------------- reference vs host C++
def test_host_cpp_equals_reference_on_every_instance():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    moves = 0
    for name in NAMES:
        want = expected(name)
        assert _rt_answer(rt, named_instances()[name], built(name)[0]) == want[:3], name
        assert list(want[2]) == list(STAT_KEYS)
        moves += want[2]["moves"]
    assert moves > 300


def test_host_cpp_equals_reference_on_random_instances():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    searched = 0
    for k in range(60):
        c = random_instance(2 + (k * 7) % 45, 81_000 + k, road=bool(k % 2), cap_frac=(None, 0.3)[k % 3 == 0])
        try:
            trips = tw_trips(**c)[0]
        except InfeasibleStops:
            continue
        want = tw_improve_trips(*search_args(c, trips))
        assert _rt_answer(rt, c, trips) == want, k
        searched += want[2]["moves"] > 0
    assert searched > 30


# --------------------------------------------------------------------------- the O(1) time tests
def test_time_verdicts_equal_resimulation_on_every_candidate():
    """Every candidate of every selection on the small instances: the O(1) verdict (type 2: the
    bounded walk) is whether the touched trips re-simulate as feasible on the seconds matrix."""
    from routest_amd.routing.timewindows import schedule_of, usable_matrix
    seen = {0: [0, 0], 1: [0, 0], 2: [0, 0]}
    for name in NAMES:
        if stops_of(name) > 14:
            continue
        c = named_instances()[name]
        qt = usable_matrix(c["t"])
        cl = list(c["close_q"])
        cl[0] = 1 << 62
        trace = []
        assert tw_improve_trips(*search_args(c, built(name)[0]), trace=trace) == expected(name)[:3], name
        for trips, verdicts in trace:
            for mv, tok in verdicts:
                want = all(len(o) == 2 or schedule_of(qt, o, c["open_q"], cl, c["sv_q"])[3]
                           for o in moved_trips(trips, mv).values())
                assert tok == want, (name, mv, trips)
                seen[mv[0]][tok] += 1
    # both verdicts occur for every move type
    assert all(min(v) > 20 for v in seen.values()), seen


# --------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    c = named_instances()[name]
    before = built(name)
    trips, schedule, st, applied = expected(name)
    assert sorted(s for t in trips for s in t[1:-1]) == list(range(1, stops_of(name) + 1))
    waiting = 0
    for t, rows in zip(trips, schedule):
        assert len(t) >= 3 and t[0] == 0 and t[-1] == 0
        ok, want = resimulate(c, t)
        assert ok and want == [tuple(r) for r in rows], t
        assert walk_feasible(c["d"], t, c["max_dist"]) and load_feasible(c["demand"], t, c["cap"])
        waiting += sum(b - a for _, a, b, _ in rows)
    assert st["len_after_q"] <= st["len_before_q"] == before[2]["len_q"]
    assert st["trips_before"] == len(before[0]) and st["trips_after"] == len(trips) <= len(before[0])
    assert st["waiting_q"] == waiting and st["moves"] == len(applied) <= 4 * stops_of(name)
    assert (st["moves"] > 0) == (st["len_after_q"] < st["len_before_q"]) and st["rejected"] in (0, 1)
    if st["moves"] == 0:
        assert trips == before[0] and schedule == before[1] and st["waiting_q"] == before[2]["waiting_q"]
    # idempotent: a second run finds nothing (a rejected move would be found and rejected again)
    again = tw_improve_trips(*search_args(c, trips))
    assert again[0] == trips and again[1] == schedule and again[2]["moves"] == 0
    assert again[2]["rejected"] == st["rejected"] or st["moves"] == 4 * stops_of(name)


def test_skip_conditions_return_the_trips_as_given():
    for name in ("demand_negative",):
        c, b = named_instances()[name], built(name)
        trips, schedule, st, _ = expected(name)
        assert trips == b[0] and schedule == b[1] and st["moves"] == 0 and st["rejected"] == 0
        assert st["len_before_q"] == st["len_after_q"] == b[2]["len_q"] and st["waiting_q"] == b[2]["waiting_q"]
    # a limit that cannot be quantized: the trips of another run, handed over with a NaN capacity
    c, b = named_instances()["random_ns31"], built("random_ns31")
    for extra in ({"cap": float("nan")}, {"max_dist": -1.0}):
        got = tw_improve_trips(*search_args(dict(c, **extra), b[0]))
        assert got[0] == b[0] and got[1] == b[1] and got[2]["moves"] == 0


# --------------------------------------------------------------------------- non-vacuity
@pytest.mark.parametrize("tier", ["small", "large"])
def test_instances_exercise_every_part_of_the_search(tier):
    names = [n for n in (SMALL if tier == "small" else LARGE) if expected(n) is not None]
    if tier == "small":
        assert {1, 2, 31, 32} <= {stops_of(n) for n in names}
    else:
        assert {33, 64, 127, 128} <= {stops_of(n) for n in names}
    types = {mv[0] for n in names for mv in expected(n)[3]}
    assert types == {0, 1, 2}
    assert any(expected(n)[2]["trips_after"] < expected(n)[2]["trips_before"] for n in names)
    assert any(expected(n)[2]["rejected"] == 1 for n in names)
    # the windows matter: with every window opened the same search returns other trips
    differ = [n for n in names
              if tw_improve_trips(*search_args(opened(named_instances()[n]), built(n)[0]))[0] != expected(n)[0]]
    assert len(differ) >= 3, differ


def test_the_issue_s_instances():
    km = lambda n, key: round(expected(n)[2][key] / 1e6, 1)  # noqa: E731
    assert (km("random_ns31", "len_before_q"), km("random_ns31", "len_after_q")) == (106.2, 70.9)
    assert (km("road_ns33", "len_before_q"), km("road_ns33", "len_after_q")) == (128.8, 88.3)
    assert (km("zero_width_ns36", "len_before_q"), km("zero_width_ns36", "len_after_q")) == (119.1, 94.6)
    assert (km("service_only_ns40", "len_before_q"), km("service_only_ns40", "len_after_q")) == (47.9, 46.8)
    for n in ("drop_road_ns8", "drop_ns12", "drop_cap_ns20", "drop_ns36"):
        assert expected(n)[2]["trips_after"] == expected(n)[2]["trips_before"] - 1, n
    assert expected("cap_float_reject")[2]["rejected"] == 1


# --------------------------------------------------------------------------- the request field
def _cluster(lat0, lon0, n=10, cap=4, **extra):
    dests = [{"lat": lat0 + (0.004 + 0.0015 * (i // 2)) * (1 if i % 2 else -1), "lon": lon0 + 0.0005 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": cap,
                            "maximum_distance": 1e6}}
    p.update(extra)
    return p


def _tw_body(lat0, lon0, **extra):
    """Ten stops on two sides of the depot, capacity 4; the early windows pull far stops to the front
    of the insertion's trips, which leaves the local search something to move."""
    p = _cluster(lat0, lon0, n=10, cap=4, **extra)
    for i, w in {0: (0, 600), 7: (0, 900), 4: (1800, 5400), 9: (3600, 7200)}.items():
        p["destination_points"][i]["time_window"] = list(w)
    for i, s in {1: 120, 6: 300.5}.items():
        p["destination_points"][i]["service"] = s
    return p


def test_wants_tw_improve_is_json_true_exactly():
    assert wants_tw_improve({"tw_improve": True})
    for v in (1, "true", False, None, [True], 1.0):
        assert not wants_tw_improve({"tw_improve": v})
    assert not wants_tw_improve({}) and not wants_tw_improve(None)


def test_optimizer_batched_and_batcher_agree():
    from routest_amd.routing.batched import batched_trips
    from routest_amd.routing.optimizer import optimize_many, optimize_route
    from routest_amd.routing.providers import HaversineProvider
    from routest_amd.routing.route_batcher import RouteBatcher
    prov = HaversineProvider()
    reqs = [_tw_body(14.58, 121.04, tw_improve=True), _tw_body(14.58, 121.04), _cluster(14.6, 121.0, tw_improve=True),
            _cluster(14.6, 121.0), _tw_body(14.5, 121.1, tw_improve=True, improve=True, exchange=True),
            _cluster(14.58, 121.04, n=1, tw_improve=True), _tw_body(14.5, 121.1, tw_improve="yes")]
    one = [optimize_route(r, prov, "e") for r in reqs]
    assert optimize_many(reqs, prov, "e") == one
    b = RouteBatcher(prov, "e", devices=[None])
    try:
        assert [b.assemble(r, p) for r, p in zip(reqs, b.plan_batch(reqs))] == one
    finally:
        b.close()
    tw0, tw1 = one[0]["properties"]["time_windows"], one[1]["properties"]["time_windows"]
    assert list(tw0) == ["method", "stops_with_windows", "trips", "waiting", "moves", "trips_before",
                         "matrix_distance_before", "matrix_distance_after"]
    assert tw0["method"] == "cheapest_insertion+relocate+swap" and tw0["moves"] >= 1
    assert tw0["matrix_distance_after"] < tw0["matrix_distance_before"] and tw0["trips_before"] == tw1["trips"]
    assert list(tw1) == ["method", "stops_with_windows", "trips", "waiting"] and tw1["method"] == "cheapest_insertion"
    # on a plain request, a single destination and with a value that is not JSON true: ignored
    assert one[2] == one[3] and "time_windows" not in one[2]["properties"]
    assert "time_windows" not in one[5]["properties"]
    assert one[6] == optimize_route(_tw_body(14.5, 121.1), prov, "e")
    # improve / exchange stay ignored beside it
    assert one[4] == optimize_route(_tw_body(14.5, 121.1, tw_improve=True), prov, "e")
    # the reference on the provider's own matrices gives these trips
    body = reqs[0]
    sec, met = prov.time_matrix([body["source_point"]] + body["destination_points"], "driving-car")
    tw = parse_time_windows(body)
    trips = tw_trips(met, sec, [0.0] + [1.0] * 10, 4.0, 1e6, *tw)[0]
    want = tw_improve_trips(met, sec, trips, [0.0] + [1.0] * 10, 4.0, 1e6, *tw)
    assert [s - 1 for t in want[0] for s in t[1:-1]] == one[0]["properties"]["optimized_order"]
    assert tw0["waiting"] == want[2]["waiting_q"] / 1000.0 and tw0["moves"] == want[2]["moves"]
    # batched_trips: the flag only changes the rows that carry it, and only time-window rows
    multi = [r for r in reqs if len(r["destination_points"]) > 1]
    tws = [parse_time_windows(r) if "time_window" in r["destination_points"][0] else None for r in multi]
    base = batched_trips(multi, time_windows=tws)
    flagged = batched_trips(multi, time_windows=tws, tw_improve=[True, False, True, False, False, False])
    assert flagged[0][1:] == base[0][1:] and flagged[2][1:] == base[2][1:] and flagged[1] == base[1]
    assert flagged[2][0][1]["search"] == want[2] and flagged[2][0][0] == want[1] and flagged[0][0] == want[0]
    assert "search" not in base[2][0][1]
    assert batched_trips(multi, time_windows=tws, tw_improve=[False] * 6) == base


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
    return r


@pytest.mark.parametrize("path", ["/api/optimize_route", "/route", "/api/request_route"])
def test_api_field_and_schedule(client, path):
    c, sv, lat0, lon0 = client
    body = _tw_body(lat0, lon0, tw_improve=True)
    without = _post(c, path, _tw_body(lat0, lon0))
    out = _post(c, path, body).json()
    props = out["properties"]
    assert set(props) == set(without.json()["properties"])
    tw = props["time_windows"]
    assert list(tw) == ["method", "stops_with_windows", "trips", "waiting", "moves", "trips_before",
                        "matrix_distance_before", "matrix_distance_after"]
    assert tw["method"] == "cheapest_insertion+relocate+swap" and tw["stops_with_windows"] == 4
    assert tw["trips"] == len(props["schedule"]) == props["summary"]["trips"] <= tw["trips_before"]
    assert tw["trips_before"] == without.json()["properties"]["time_windows"]["trips"]
    assert tw["matrix_distance_after"] <= tw["matrix_distance_before"]
    assert (tw["moves"] > 0) == (tw["matrix_distance_after"] < tw["matrix_distance_before"])
    if sv.provider.name == "haversine":
        assert tw["moves"] >= 1
    assert [e["destination"] for trip in props["schedule"] for e in trip] == props["optimized_order"]
    assert sorted(props["optimized_order"]) == list(range(10))
    waiting = 0.0
    for trip in props["schedule"]:
        clock = 0.0
        assert len(trip) <= 4                     # vehicle_capacity
        for e in trip:
            p = body["destination_points"][e["destination"]]
            lo, hi = p.get("time_window", [0, float("inf")])
            assert clock <= e["arrival"] <= e["start"] <= e["departure"] and lo <= e["start"] <= hi
            assert e["start"] == max(e["arrival"], lo)
            assert abs(e["departure"] - e["start"] - p.get("service", 0)) < 1e-9
            waiting += e["waiting"]
            clock = e["departure"]
    assert abs(waiting - tw["waiting"]) < 1e-6
    # without the field, or with a value that is not JSON true: the bytes of the request without it
    for v in (False, "true", 1, None):
        echo = _post(c, path, _tw_body(lat0, lon0, tw_improve=v))
        if path == "/api/optimize_route":
            assert echo.content == without.content
        assert echo.json()["properties"]["time_windows"] == without.json()["properties"]["time_windows"]
        assert echo.json()["properties"]["schedule"] == without.json()["properties"]["schedule"]
    assert list(without.json()["properties"]["time_windows"]) == ["method", "stops_with_windows", "trips", "waiting"]
    # on a plain request the field is ignored
    plain = _post(c, path, _cluster(lat0, lon0))
    flagged = _post(c, path, _cluster(lat0, lon0, tw_improve=True))
    if path == "/api/optimize_route":
        assert flagged.content == plain.content
    assert flagged.json()["properties"] == plain.json()["properties"]
    # improve / exchange stay ignored beside it
    both = _post(c, path, _tw_body(lat0, lon0, tw_improve=True, improve=True, exchange=True)).json()
    assert both["properties"] == props


def test_api_batch_takes_the_field_per_request(client):
    c, sv, lat0, lon0 = client
    reqs = [_cluster(lat0, lon0, tw_improve=True), _tw_body(lat0, lon0, tw_improve=True), _tw_body(lat0, lon0),
            _cluster(lat0, lon0, n=1, tw_improve=True)]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs}).json()["results"]
    assert ["moves" in r["properties"].get("time_windows", {}) for r in res] == [False, True, False, False]
    for k in range(4):
        assert res[k] == _post(c, "/api/request_route", reqs[k]).json()


def test_native_front_end_hands_the_request_to_the_app():
    from routest_amd.ops import _ext
    rt = _ext.runtime(required=True)
    assert rt.route_optimize_cpu(json.dumps(_tw_body(14.58, 121.04, tw_improve=True)).encode()) is None
    plain = rt.route_optimize_cpu(json.dumps(_cluster(14.58, 121.04, n=3)).encode())
    assert plain is not None and plain[0] == 200
