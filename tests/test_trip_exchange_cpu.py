"""Inter-trip relocate / swap improvement of the greedy's trips (routing/exchange.py): the Python
reference against the host C++ (``_rt.exchange_trips``) with ``==``, a brute-force oracle of the move
sequence, the reference's invariants, and the ``exchange`` field on the HTTP API.
Instances: tests/_exchange_cases.py."""
import json
import os

import numpy as np
import pytest

from routest_amd.routing.exchange import (UNBOUNDED, exchange_trips, improve_exchange_trips, load_feasible,
                                          quantize_limit, wants_exchange)
from routest_amd.routing.improve import BIG, improve_trips, quantize, quantize_matrix, trip_length_q, walk_feasible

from _exchange_cases import expected, named_instances

FIX = os.path.join(os.path.dirname(__file__), "fixtures")
NAMES = list(named_instances())


# --------------------------------------------------------------------------- reference vs host C++
def test_host_cpp_equals_reference_on_every_instance():
    rt = pytest.importorskip("routest_amd._rt")
    assert hasattr(rt, "exchange_trips")
    moved = 0
    for name in NAMES:
        d, dem, cap, md, trips, mc = named_instances()[name]
        want_trips, want_st = expected(name)
        got_trips, got_st = rt.exchange_trips(np.asarray(d, dtype=np.float64), trips, dem, cap, md, mc)
        assert got_trips == want_trips, name
        assert got_st == want_st, name
        moved += want_st["moves"]
    assert moved > 100


def test_instances_cover_the_issue():
    st = {n: expected(n)[1] for n in NAMES}
    for ns in (2, 3, 10, 31, 32, 33, 64, 127, 128):
        inst = named_instances()[f"random_ns{ns}"]
        assert len(inst[0]) == ns + 1 and len(inst[4]) >= min(3, ns)
    assert all(st[f"random_ns{ns}"]["moves"] > 0 for ns in (10, 31, 32, 33, 64, 127, 128))
    # skipped stages: trips as given, nothing moved
    for n in ("skipped_ns129", "demand_negative", "demand_nan"):
        assert st[n]["moves"] == 0 and expected(n)[0] == [list(t) for t in named_instances()[n][4]]
        assert st[n]["trips_after"] == st[n]["trips_before"] and st[n]["len_after_q"] == st[n]["len_before_q"]
    # full trips: only swaps are admissible (between one-stop trips a swap changes nothing)
    assert st["singletons_swaps_only"]["moves"] == 0 and st["singletons_swaps_only"]["trips_after"] == 12
    assert st["pairs_swaps_only"]["moves"] > 0 and st["pairs_swaps_only"]["trips_after"] == 6
    assert {m[0] for m in _reference_sequence("pairs_swaps_only")} == {1}
    # no limits: relocates merge the one-stop trips; every trip that stays non-empty is a local optimum
    assert st["singletons_merge"]["trips_before"] == 9 > st["singletons_merge"]["trips_after"]
    assert {m[0] for m in _reference_sequence("singletons_merge")} == {0}
    assert st["singletons_merge_k40"]["trips_after"] < 40
    assert st["move_cap_1"]["moves"] == 1 and st["move_cap_2"]["moves"] == 2
    assert st["move_cap_2_k40"]["moves"] == 2
    assert st["reject_float_walk"]["rejected"] == 1 and st["reject_float_walk"]["moves"] >= 1
    assert st["cap_float_reject"] == dict(st["cap_float_reject"], moves=0, rejected=1)
    assert st["cap_boundary"]["moves"] > 0 and max(len(t) for t in expected("cap_boundary")[0]) == 5
    assert st["special_big_edges"]["len_before_q"] >= BIG and st["special_big_edges"]["moves"] > 0
    # the non-metric instance: a relocate that gains 4 m is one the source-trip test forbids
    d, dem, cap, md, trips, _ = named_instances()["nonmetric_source_grows"]
    cands = _candidates(quantize_matrix(np.asarray(d)), np.array([quantize(v) for v in dem]),
                        [list(t) for t in trips], UNBOUNDED, UNBOUNDED)
    assert (-4000000, 0, 0, 2, 1, 1) in cands
    assert (0, 0, 2, 1, 1) not in [c[1:] for c in _candidates(
        quantize_matrix(np.asarray(d)), np.array([quantize(v) for v in dem]), [list(t) for t in trips],
        quantize_limit(cap), quantize_limit(md))]
    assert _tied_best_moves("grid_ties") > 0
    # the admissibility tests one by one: the source trip forbids / meets the limit with equality,
    # a swap leaves the first / the second trip at the limit exactly, an emptied trip is no target
    assert st["source_check_forbids"]["moves"] == 0 and st["source_check_forbids"]["rejected"] == 0
    assert _reference_sequence("source_check_equal") == [(0, 0, 2, 1, 1)]
    assert trip_length_q(quantize_matrix(np.asarray(named_instances()["source_check_equal"][0])),
                         expected("source_check_equal")[0][0]) == 3_500_000
    q = quantize_matrix(np.asarray(named_instances()["swap_first_trip_equal"][0]))
    assert _reference_sequence("swap_first_trip_equal") == _reference_sequence("swap_second_trip_equal") == [(1, 0, 1, 1, 1)]
    assert [trip_length_q(q, t) for t in expected("swap_first_trip_equal")[0]] == [1_000_000, 600_000]
    assert [trip_length_q(q, t) for t in expected("swap_second_trip_equal")[0]] == [600_000, 1_000_000]
    assert st["emptied_trip_no_target"]["moves"] == 1 and st["emptied_trip_no_target"]["trips_after"] == 2


def test_limits_are_quantized_as_defined():
    assert quantize_limit(4.5) == 4500 and quantize_limit(0.0) == 0 and quantize_limit(0.0019) == 1
    assert quantize_limit(9e12) == UNBOUNDED and quantize_limit(float(2 ** 40)) == UNBOUNDED
    assert quantize_limit(float("inf")) == UNBOUNDED
    assert quantize_limit(float("nan")) is None and quantize_limit(-1e-9) is None
    d, dem, cap, md, trips, _ = named_instances()["random_ns10"]
    for bad_cap, bad_md in ((float("nan"), md), (-1.0, md), (cap, float("nan")), (cap, -5.0)):
        out, st = exchange_trips(np.asarray(d), trips, dem, bad_cap, bad_md)
        assert out == trips and st["moves"] == 0 and st["rejected"] == 0


# --------------------------------------------------------------------------- brute force oracle
def _moved(trips, typ, A, i, B, j):
    a, b = list(trips[A]), list(trips[B])
    if typ == 0:
        s = a.pop(i)
        b.insert(j + 1, s)
    else:
        a[i], b[j] = b[j], a[i]
    return a, b


def _candidates(q, qd, trips, cap_q, max_q):
    """Every admissible move as (-gain, type, A, i, B, j), sorted: both trips rebuilt per candidate,
    the gain the difference of their full lengths."""
    out = []
    m = len(trips)
    for typ in (0, 1):
        for A in range(m):
            for B in range(m):
                if A == B or (typ == 1 and not A < B) or len(trips[B]) <= 2:
                    continue
                for i in range(1, len(trips[A]) - 1):
                    for j in range(1 if typ else 0, len(trips[B]) - 1):
                        a, b = _moved(trips, typ, A, i, B, j)
                        la, lb = trip_length_q(q, a), trip_length_q(q, b)
                        wa, wb = sum(int(qd[s]) for s in a[1:-1]), sum(int(qd[s]) for s in b[1:-1])
                        if wb > cap_q or lb > max_q or la > max_q or (typ == 1 and wa > cap_q):
                            continue
                        gain = trip_length_q(q, trips[A]) + trip_length_q(q, trips[B]) - la - lb
                        out.append((-gain, typ, A, i, B, j))
    return sorted(out)


def _oracle(d, trips, dem, cap, md, move_cap):
    """The search of the issue with the brute-force candidate list: (trips, move sequence, rejected)."""
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    qd = np.array([0] + [quantize(v) for v in dem[1:]])
    cur = [list(t) for t in trips]
    seq = []
    limit = 4 * (len(d) - 1) if move_cap is None else move_cap
    while len(seq) < limit:
        cands = _candidates(q, qd, cur, quantize_limit(cap), quantize_limit(md))
        if not cands or cands[0][0] >= 0:
            break
        _, typ, A, i, B, j = cands[0]
        a, b = _moved(cur, typ, A, i, B, j)
        if not all(walk_feasible(d, t, md) and load_feasible(dem, t, cap) for t in (a, b)):
            return [t for t in cur if len(t) > 2], seq, 1
        cur[A], cur[B] = a, b
        seq.append((typ, A, i, B, j))
    return [t for t in cur if len(t) > 2], seq, 0


def _reference_sequence(name):
    """The reference's own move sequence, replayed through best_move."""
    from routest_amd.routing.exchange import apply_move, best_move
    d, dem, cap, md, trips, mc = named_instances()[name]
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    qd = np.array([0] + [quantize(v) for v in dem[1:]], dtype=np.int64)
    cur = [list(t) for t in trips]
    seq = []
    for _ in range(expected(name)[1]["moves"]):
        Lq = [trip_length_q(q, t) for t in cur]
        Wq = [int(sum(int(qd[s]) for s in t[1:-1])) for t in cur]
        gain, typ, A, i, B, j = best_move(q, qd, cur, Lq, Wq, quantize_limit(cap), quantize_limit(md))
        assert gain > 0
        apply_move(cur, typ, A, i, B, j)
        seq.append((typ, A, i, B, j))
    assert [t for t in cur if len(t) > 2] == expected(name)[0]
    return seq


def _tied_best_moves(name):
    d, dem, cap, md, trips, mc = named_instances()[name]
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    qd = np.array([0] + [quantize(v) for v in dem[1:]])
    cur = [list(t) for t in trips]
    ties = 0
    for typ, A, i, B, j in _reference_sequence(name):
        c = _candidates(q, qd, cur, quantize_limit(cap), quantize_limit(md))
        ties += len(c) > 1 and c[0][0] == c[1][0]
        cur[A], cur[B] = _moved(cur, typ, A, i, B, j)
    return ties


SMALL = [n for n in NAMES if len(named_instances()[n][0]) - 1 <= 10 and not n.startswith("demand_")]


@pytest.mark.parametrize("name", SMALL)
def test_brute_force_oracle_gives_the_reference_move_sequence(name):
    d, dem, cap, md, trips, mc = named_instances()[name]
    want_trips, want_st = expected(name)
    got_trips, seq, rejected = _oracle(d, trips, dem, cap, md, mc)
    assert got_trips == want_trips
    assert len(seq) == want_st["moves"] and rejected == want_st["rejected"]
    assert seq == _reference_sequence(name)


def test_oracle_covers_both_move_types_and_the_small_instances():
    assert len(SMALL) >= 10
    types = {m[0] for n in SMALL for m in _reference_sequence(n)}
    assert types == {0, 1}


# --------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    d, dem, cap, md, trips, mc = named_instances()[name]
    out, st = expected(name)
    q = quantize_matrix(np.asarray(d, dtype=np.float64))
    assert sorted(s for t in out for s in t[1:-1]) == sorted(s for t in trips for s in t[1:-1])
    assert all(t[0] == 0 and t[-1] == 0 and len(t) > 2 for t in out)
    assert st["trips_before"] == len(trips) and st["trips_after"] == len(out) <= len(trips)
    assert st["len_before_q"] == sum(trip_length_q(q, t) for t in trips)
    assert st["len_after_q"] == sum(trip_length_q(q, t) for t in out)
    assert st["len_after_q"] <= st["len_before_q"] and (st["moves"] > 0) == (st["len_after_q"] < st["len_before_q"])
    assert st["moves"] <= (4 * (len(d) - 1) if mc is None else mc)
    given = [list(t) for t in trips]
    for t in out:
        if t not in given:
            assert walk_feasible(d, t, md) and load_feasible(dem, t, cap), name
    if st["moves"] and not st["rejected"] and mc is None:
        # a local optimum of the unbounded search, too, unless a limit was what stopped it
        again, st2 = exchange_trips(np.asarray(d), out, dem, cap, md)
        assert again == out and st2["moves"] == 0


def test_pipeline_composes_the_three_stages():
    d, dem, cap, md, _, _ = named_instances()["random_ns31"]
    from routest_amd.routing.greedy import greedy_trips
    g = greedy_trips(d, dem, cap, md)
    t1, s1 = improve_trips(np.asarray(d), g, md)
    t2, s2 = exchange_trips(np.asarray(d), t1, dem, cap, md)
    t3, s3 = improve_trips(np.asarray(d), t2, md)
    out, st = improve_exchange_trips(np.asarray(d), g, dem, cap, md)
    assert out == t3 and s2["moves"] > 0
    assert st == {"moves": s1["moves"] + s3["moves"], "exchange_moves": s2["moves"],
                  "trips_before": len(g), "trips_after": len(t3), "len_before_q": s1["len_before_q"],
                  "len_after_q": s3["len_after_q"]}
    assert st["len_after_q"] < s1["len_after_q"]


# --------------------------------------------------------------------------- API contract
def _cluster(lat0, lon0, n=10, cap=4, **extra):
    """Stops in pairs at growing distance, the two of a pair on opposite sides of the depot: the
    greedy's rings put the two sides into the same trips."""
    dests = [{"lat": lat0 + (0.004 + 0.0015 * (i // 2)) * (1 if i % 2 else -1), "lon": lon0 + 0.0005 * i,
              "payload": 1} for i in range(n)]
    p = {"source_point": {"lat": lat0, "lon": lon0}, "destination_points": dests,
         "driver_details": {"driver_name": "Ana", "vehicle_type": "car", "vehicle_capacity": cap,
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
def test_api_exchange_field(client, path):
    from routest_amd.routing.optimizer import optimize_route
    c, sv, lat0, lon0 = client
    plain = _post(c, path, _cluster(lat0, lon0))
    assert "improvement" not in plain["properties"]
    only = _post(c, path, _cluster(lat0, lon0, improve=True))
    assert list(only["properties"]["improvement"]) == ["method", "moves", "trips_changed",
                                                       "matrix_distance_before", "matrix_distance_after"]
    assert only["properties"]["improvement"]["method"] == "2opt+oropt"
    out = _post(c, path, _cluster(lat0, lon0, exchange=True))
    imp = out["properties"]["improvement"]
    assert list(imp) == ["method", "moves", "exchange_moves", "trips_before", "trips_after",
                         "matrix_distance_before", "matrix_distance_after"]
    assert imp["method"] == "2opt+oropt+exchange" and imp["exchange_moves"] >= 1
    assert imp["trips_after"] <= imp["trips_before"] == plain["properties"]["summary"]["trips"]
    assert out["properties"]["summary"]["trips"] == imp["trips_after"]
    assert imp["matrix_distance_after"] < only["properties"]["improvement"]["matrix_distance_after"]
    assert imp["matrix_distance_before"] == only["properties"]["improvement"]["matrix_distance_before"]
    assert sorted(out["properties"]["optimized_order"]) == sorted(plain["properties"]["optimized_order"])
    assert set(out["properties"]) - {"improvement"} == set(plain["properties"])
    # exchange implies improve: the value of improve is ignored
    for v in (True, False, "no"):
        assert _post(c, path, _cluster(lat0, lon0, exchange=True, improve=v)) == out
    # anything but JSON true is off, and then the answers are the ones of the payload without the field
    for v in (1, "true", "yes", False, None, [True]):
        assert _post(c, path, _cluster(lat0, lon0, exchange=v)) == plain, v
        assert _post(c, path, _cluster(lat0, lon0, exchange=v, improve=True)) == only, v
    if path == "/api/optimize_route" and sv.provider.name == "haversine":
        for extra, want in (({}, plain), ({"improve": True}, only), ({"exchange": True}, out)):
            assert optimize_route(_cluster(lat0, lon0, **extra), sv.provider, plain["properties"]["engine"]) == want


def test_api_exchange_can_answer_with_fewer_trips(client):
    c, sv, lat0, lon0 = client
    if sv.provider.name != "haversine":
        return          # the distance limit below is sized for the haversine matrix
    # the distance limit, measured on the greedy's zig-zag order, forces three trips; once the
    # stops are sorted by side the exchange merges them
    p = _cluster(lat0, lon0, n=10, cap=99)
    p["driver_details"]["maximum_distance"] = 8000
    plain = _post(c, "/api/optimize_route", p)
    out = _post(c, "/api/optimize_route", dict(p, exchange=True))
    imp = out["properties"]["improvement"]
    assert plain["properties"]["summary"]["trips"] == imp["trips_before"] == 3
    assert out["properties"]["summary"]["trips"] == imp["trips_after"] == 1
    assert out["properties"]["summary"]["distance"] < plain["properties"]["summary"]["distance"]
    assert sorted(out["properties"]["optimized_order"]) == list(range(10))


def test_api_single_destination_and_alternatives_ignore_exchange(client):
    c, sv, lat0, lon0 = client
    one = _cluster(lat0, lon0, n=1)
    assert _post(c, "/api/optimize_route", dict(one, exchange=True)) == _post(c, "/api/optimize_route", one)
    if sv.provider.name != "graph":
        return          # alternatives need the road graph; elsewhere the answer is an error either way
    body = _cluster(lat0, lon0, n=4, alternatives=3)
    a = c.post("/api/optimize_route", json=body)
    b = c.post("/api/optimize_route", json=dict(body, exchange=True))
    assert a.status_code == b.status_code == 200 and a.json() == b.json()
    assert "alternatives" in a.json()["properties"] and "improvement" not in b.json()["properties"]


def test_api_batch_takes_the_field_per_request(client):
    c, sv, lat0, lon0 = client
    reqs = [_cluster(lat0, lon0), _cluster(lat0, lon0, exchange=True), _cluster(lat0, lon0, improve=True),
            _cluster(lat0, lon0, n=1, exchange=True), _cluster(lat0, lon0, n=6, exchange="yes")]
    res = _post(c, "/api/optimize_routes_batch", {"requests": reqs})["results"]
    methods = [r["properties"].get("improvement", {}).get("method") for r in res]
    assert methods == [None, "2opt+oropt+exchange", "2opt+oropt", None, None]
    for k in (0, 1, 2):
        assert res[k] == _post(c, "/api/request_route", reqs[k])


def test_wants_exchange_is_json_true_only():
    assert wants_exchange({"exchange": True})
    for v in (1, "true", False, None, [True], 1.0):
        assert not wants_exchange({"exchange": v})
    assert not wants_exchange(None) and not wants_exchange([])


def test_native_cpu_planner_answers_like_the_app():
    """``_rt.route_optimize_cpu`` (csrc/runtime/route_bind.cpp) runs the three stages and writes
    ``improvement`` byte for byte like the app's JSON response."""
    rt = pytest.importorskip("routest_amd._rt")
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.routing.providers import HaversineProvider
    prov = HaversineProvider()
    seen = set()
    for extra in ({"exchange": True}, {"exchange": True, "improve": False}, {"exchange": True, "cap": 3},
                  {"exchange": True, "n": 24, "cap": 5}, {"exchange": 1}, {"exchange": "true", "improve": True},
                  {"improve": True}, {}):
        p = _cluster(14.58, 121.04, **extra)
        ref = optimize_route(p, prov, "backend:mi355x")
        seen.add(ref["properties"].get("improvement", {}).get("method"))
        want = json.dumps(ref, ensure_ascii=False, separators=(",", ":"), allow_nan=False).encode()
        st, body = rt.route_optimize_cpu(json.dumps(p).encode())
        assert st == 200 and bytes(body) == want, extra
    assert seen == {None, "2opt+oropt", "2opt+oropt+exchange"}


def test_graph_assembly_carries_the_statistics():
    """``_rt.route_assemble_graph`` with given trips and their statistics (the six of an exchange
    request, the four of an improve request) writes the app's bytes on the road-graph provider."""
    rt = pytest.importorskip("routest_amd._rt")
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.greedy import greedy_trips
    from routest_amd.routing.optimizer import optimize_route
    g = synth_road_graph(3000, seed=1)
    prov = GraphProvider(g, (g.length_m / 9.0).astype(np.float32), device=None)
    lat0, lon0 = float(np.median(g.lat)), float(np.median(g.lon))
    for extra in ({"exchange": True}, {"improve": True}):
        p = _cluster(lat0, lon0, n=9, cap=4, **extra)
        body = json.dumps(p).encode()
        ref = optimize_route(json.loads(body), prov, "backend:mi355x")
        want = json.dumps(ref, ensure_ascii=False, separators=(",", ":"), allow_nan=False).encode()
        pts = [p["source_point"]] + p["destination_points"]
        d = np.asarray(prov.matrix(pts, "driving-car"), dtype=np.float64)
        dem = [0.0] + [float(q["payload"]) for q in pts[1:]]
        g0 = greedy_trips(d.tolist(), dem, 4.0, 1e6)
        if "exchange" in extra:
            trips, st = improve_exchange_trips(d, g0, dem, 4.0, 1e6)
            assert st["exchange_moves"] > 0
            tup = (st["moves"], st["exchange_moves"], st["trips_before"], st["trips_after"],
                   st["len_before_q"], st["len_after_q"])
        else:
            trips, st = improve_trips(d, g0, 1e6)
            tup = (st["moves"], st["trips_changed"], st["len_before_q"], st["len_after_q"])
        calls = [[pts[i] for i in t] for t in trips]
        nodes = np.concatenate([g.nearest_nodes([q["lat"] for q in c], [q["lon"] for q in c]) for c in calls])
        pairs, o = set(), 0
        for c in calls:
            pairs.update((int(nodes[o + i]), int(nodes[o + i + 1])) for i in range(len(c) - 1))
            o += len(c)
        legs = dict(zip(sorted(pairs), prov.legs(sorted(pairs))[0]))
        got = rt.route_assemble_graph(body, "backend:mi355x", g.lat, g.lon, nodes.astype(np.int32), trips,
                                      {k: tuple(v) for k, v in legs.items()}, prov._steps, prov.cost,
                                      improvement=tup)
        assert got[0] == 200 and bytes(got[1]) == want, extra
