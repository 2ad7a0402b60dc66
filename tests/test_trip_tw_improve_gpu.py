"""K6e (``_C.route_tw_improve``, csrc/route_tw_improve.hip) on K6d's outputs against the Python
reference (routing/tw_improve.py): ``visit`` / ``trip_of`` / ``ntrips`` / ``status``, the arrival and
start milliseconds and the search's statistics are compared with ``torch.equal``; then random rows
against the host C++, the device path of ``batched_trips`` against the CPU path, the app on the GPU
road router against the CPU router, and the main port relaying a ``tw_improve`` request.
Instances: tests/_tw_improve_cases.py."""
import json

import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import batched_trips, pack_requests
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.timewindows import parse_time_windows, tw_trips

from _tw_cases import expected_rows as k6d_rows, pack_rows, random_instance
from _tw_improve_cases import LARGE, SMALL, expected_rows, named_instances, rows_of, stops_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

DEV = "cuda:0"
OUT = ("visit", "trip_of", "ntrips", "status", "arrival_q", "start_q", "search stats")


def _args(cases, nm):
    D, T, npts, dem, cap, maxd, op, cl, sv = pack_rows(cases, nm)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(DEV)  # noqa: E731
    return [t(D), t(T), t(npts, torch.int32), t(dem), t(cap), t(maxd), t(op, torch.int64), t(cl, torch.int64),
            t(sv, torch.int64)]


def _launch(cases, nm, flags=None):
    """K6d over every row, then K6e over the flagged ones: the six outputs and the search's stats."""
    C = _ext.native(required=True)
    args = _args(cases, nm)
    ones = torch.ones(len(cases), dtype=torch.uint8, device=DEV)
    f = ones if flags is None else torch.as_tensor(np.asarray(flags, np.uint8)).to(DEV)
    out = C.route_tw_trips(*args, ones)
    stats = C.route_tw_improve(*args, *out[:6], f)
    torch.cuda.synchronize()
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (len(cases), 7)
    return [c.cpu() for c in out[:6]] + [stats.cpu()]


def _stack(rows):
    return [torch.from_numpy(np.stack([np.asarray(r[i]) for r in rows])) for i in range(len(OUT))]


def _compare(got, want, names):
    for key, g, w in zip(OUT, got, want):
        if g.dtype != w.dtype:
            w = w.to(g.dtype)
        if not torch.equal(g, w):
            bad = [names[k] for k in range(len(names)) if not torch.equal(g[k], w[k])]
            raise AssertionError(f"{key} differs on {bad}")


def _check(names, nm):
    cases = [named_instances()[n] for n in names]
    _compare(_launch(cases, nm), _stack([expected_rows(n, nm) for n in names]), names)


def test_small_tier_equals_reference_on_every_instance():
    """Rows of at most 32 stops in a batch whose width keeps the launch to the wave tier."""
    assert {1, 2, 31, 32} <= {stops_of(n) for n in SMALL}
    assert {"cap_float_reject", "drop_road_ns8", "drop_ns12", "drop_cap_ns20", "special_entries", "grid_ties",
            "demand_negative", "infeasible_alone"} <= set(SMALL)
    _check(SMALL, 33)


def test_large_tier_equals_reference_on_every_instance():
    assert {33, 64, 127, 128} <= {stops_of(n) for n in LARGE}
    assert {"drop_ns36", "cap_float_reject_ns40", "road_ns33", "road_ns50", "zero_width_ns36"} <= set(LARGE)
    _check(LARGE, 129)


def test_both_tiers_in_one_launch():
    """Every instance in one batch of width 129: each row is taken by the tier its stop count picks."""
    _check(SMALL + LARGE, 129)


def test_rows_that_do_not_ask_are_left_alone():
    """Unflagged rows, a status-1 row and npts 0 / 1 rows beside flagged ones: K6e writes nothing for
    them (K6d's outputs bit for bit, zero statistics), and the flagged rows get their answers."""
    names = ["random_ns31", "drop_ns12", "random_ns33", "infeasible_alone", "road_ns12", "random_ns64", "zero_width"]
    flags = [1, 0, 1, 1, 0, 0, 1]
    cases = [named_instances()[n] for n in names]
    C = _ext.native(required=True)
    pad = lambda a: torch.cat([a, torch.zeros((2,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)])  # noqa: E731
    args = [pad(a) for a in _args(cases, 65)]
    args[2][7], args[2][8] = 0, 1                                       # npts
    ones = torch.ones(9, dtype=torch.uint8, device=DEV)
    k6d = C.route_tw_trips(*args, ones)
    before = [c.clone() for c in k6d]
    stats = C.route_tw_improve(*args, *k6d[:6], torch.as_tensor(np.array(flags + [1, 1], np.uint8)).to(DEV))
    torch.cuda.synchronize()
    assert int(before[3][3]) == 1 and int(before[3][7]) == 0 and int(before[3][8]) == 0
    want = _stack([expected_rows(n, 65) for n in names])
    changed = 0
    for key, g, b, w in zip(OUT, list(k6d[:6]) + [stats], before[:6] + [None], want):
        g = g.cpu()
        for k, f in enumerate(flags + [1, 1]):
            if f and k < 7 and names[k] != "infeasible_alone":
                assert torch.equal(g[k], w[k].to(g.dtype)), (key, names[k])
                changed += b is not None and not torch.equal(g[k], b[k].cpu())
            elif b is not None:
                assert torch.equal(g[k], b[k].cpu()), (key, k)
            else:
                assert bool((g[k] == 0).all()), (key, k)
    assert changed >= 6                     # the flagged rows were rewritten
    assert torch.equal(k6d[6], before[6])   # K6d's own statistics stay


@pytest.mark.parametrize("ns_lo,ns_hi,nm", [(1, 32, 33), (33, 128, 129)])
def test_random_rows_equal_host_cpp(ns_lo, ns_hi, nm):
    """32 random rows per tier against ``_rt.tw_improve``: windows on 70 % of the stops, road-like
    seconds on every other row, a binding capacity on every third."""
    rt = _ext.runtime(required=True)
    rng = np.random.default_rng(ns_hi + 5)
    sizes = [int(v) for v in rng.integers(ns_lo, min(ns_hi, 48 if ns_lo > 32 else ns_hi) + 1, 30)] + [ns_lo, ns_hi]
    cases = [random_instance(ns, 90_000 + ns_hi * 100 + k, road=bool(k % 2), cap_frac=(None, 0.3)[k % 3 == 0])
             for k, ns in enumerate(sizes)]
    rows, moved = [], 0
    for c in cases:
        try:
            trips = tw_trips(**c)[0]
        except InfeasibleStops as e:
            rows.append(k6d_rows(c, ("infeasible", e.stops), nm)[:6] + (np.zeros(7, dtype=np.int64),))
            continue
        got = rt.tw_improve(np.asarray(c["d"]), np.asarray(c["t"]), trips, c["demand"], c["cap"], c["max_dist"],
                            c["open_q"], c["close_q"], c["sv_q"])
        rows.append(rows_of(got, nm))
        moved += got[2]["moves"] > 0
    assert moved > 16
    _compare(_launch(cases, nm), _stack(rows), [f"row{k}_ns{ns}" for k, ns in enumerate(sizes)])


def _request(n, seed, cap=99, **extra):
    rng = np.random.default_rng(seed)
    lat, lon = 14.55 + rng.normal(0, 0.03, n + 1), 121.02 + rng.normal(0, 0.03, n + 1)
    r = {"source_point": {"lat": float(lat[0]), "lon": float(lon[0])},
         "destination_points": [{"lat": float(lat[i]), "lon": float(lon[i]), "payload": int(rng.integers(1, 4))}
                                for i in range(1, n + 1)],
         "driver_details": {"vehicle_capacity": cap, "maximum_distance": 1e7, "vehicle_type": ["car", "bike"][seed % 2]}}
    for i, p in enumerate(r["destination_points"]):
        if rng.random() < 0.7:
            lo = float(rng.uniform(0, 6 * 3600))
            p["time_window"] = [round(lo, 1), round(lo + float(rng.uniform(1800, 4 * 3600)), 1)]
        if rng.random() < 0.5:
            p["service"] = int(rng.integers(0, 600))
    r.update(extra)
    return r


def _same(gpu, cpu):
    assert len(gpu) == len(cpu) == 3
    for g, c in zip(gpu[0], cpu[0]):
        if isinstance(c, InfeasibleStops):
            assert isinstance(g, InfeasibleStops) and g.stops == c.stops and str(g) == str(c)
        else:
            assert g == c
    assert gpu[1] == cpu[1] and gpu[2] == cpu[2]


def test_batched_trips_device_equals_cpu():
    """``batched_trips(device="cuda")`` == ``batched_trips`` on the CPU with flagged time-window rows
    beside unflagged, plain, improve and exchange rows: on K5's haversine matrix and on a given road
    D / T."""
    reqs = [_request(n, s, cap=c) for n, s, c in
            ((2, 1, 9), (5, 2, 6), (12, 3, 9), (33, 4, 30), (40, 5, 40), (9, 6, 7), (128, 7, 400), (20, 8, 15))]
    reqs[5]["destination_points"][2]["time_window"] = [0, 0]            # infeasible alone
    for k in (1, 4):                                                    # rows without the fields
        for p in reqs[k]["destination_points"]:
            p.pop("time_window", None)
            p.pop("service", None)
    tw = [None if k in (1, 4) else parse_time_windows(r) for k, r in enumerate(reqs)]
    imp = [True, True, False, False, False, False, True, False]
    exc = [False, False, False, True, True, False, False, False]
    twi = [True, True, True, True, True, True, True, False]
    kw = dict(time_windows=tw, improve=imp, exchange=exc, tw_improve=twi)
    gpu = batched_trips(reqs, device=DEV, **kw)
    _same(gpu, batched_trips(reqs, device=None, **kw))
    base = batched_trips(reqs, device=DEV, time_windows=tw, improve=imp, exchange=exc)
    # the flag is honoured on time-window rows only, and only where it is set
    assert [v is not None and "search" in v[1] for v in gpu[2]] == [True, False, True, True, False, False, True, False]
    for k in (1, 4, 7):
        assert gpu[0][k] == base[0][k] and gpu[1][k] == base[1][k] and gpu[2][k] == base[2][k]
    assert sum(gpu[2][k][1]["search"]["moves"] for k in (2, 3, 6)) > 10
    assert sum(len(t) - 2 for t in gpu[0][6]) == 128
    # a given road-like D / T (seconds unrelated to the metres)
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    nm = lat.shape[1]
    rng = np.random.default_rng(11)
    D = rng.uniform(200.0, 9000.0, (len(reqs), nm, nm))
    T = rng.uniform(20.0, 900.0, (len(reqs), nm, nm))
    for M in (D, T):
        M[:, np.arange(nm), np.arange(nm)] = 0.0
    _same(batched_trips(reqs, device=DEV, D=D, T=T, **kw), batched_trips(reqs, device=None, D=D, T=T, **kw))
    # a batch nobody flags is the call without the argument
    assert batched_trips(reqs, device=DEV, time_windows=tw, tw_improve=[False] * 8)[2] == \
        batched_trips(reqs, device=DEV, time_windows=tw)[2]


def test_app_on_the_gpu_router_equals_the_cpu_router():
    """One ``tw_improve`` request through the app on the GPU graph provider (per-request path and
    the batcher's flush) equals ``optimize_route`` on the CPU CCH router.  Both routers customize the
    same given edge costs."""
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.routing.optimizer import optimize_route
    from routest_amd.serve.eta_service import EtaService
    g = synth_road_graph(3000, seed=1)
    cost = (g.length_m / 9.0).astype(np.float32)
    rng = np.random.default_rng(3)
    idx = rng.choice(g.num_nodes, 13, replace=False)
    body = {"source_point": {"lat": float(g.lat[idx[0]]), "lon": float(g.lon[idx[0]])},
            "destination_points": [{"lat": float(g.lat[j]), "lon": float(g.lon[j]), "payload": 1} for j in idx[1:]],
            "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7}, "tw_improve": True}
    body["destination_points"][0]["time_window"] = [14400, 18000]
    body["destination_points"][3]["time_window"] = [0, 36000]
    body["destination_points"][7]["time_window"] = [1800, 5400]
    body["destination_points"][5]["service"] = 240
    cpu = GraphProvider(g, cost, device=None)
    for batch in ("0", "1"):
        gpu = GraphProvider(g, cost, device=torch.device("cuda", 0))
        s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch=batch, route_gpu_min_stops=1,
                          warm_scorer=False)
        sv = build_services(s, eta=EtaService(None, device="cpu"), provider=gpu, store=None)
        try:
            with TestClient(create_app(sv)) as c:
                r = c.post("/api/optimize_route", json=body)
                assert r.status_code == 200, r.text
                got = r.json()
        finally:
            sv.close()
        want = optimize_route(json.loads(json.dumps(body)), cpu, got["properties"]["engine"])
        tw = got["properties"]["time_windows"]
        assert tw["method"] == "cheapest_insertion+relocate+swap" and tw["stops_with_windows"] == 3
        assert tw["moves"] >= 1 and tw["matrix_distance_after"] < tw["matrix_distance_before"]
        assert got == json.loads(json.dumps(want)), batch


def test_main_port_relays_requests_with_the_field():
    """The native front end does not answer time-window requests: relayed, the app's bytes, no
    native flush."""
    import http.client
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.providers import HaversineProvider
    from routest_amd.serve.eta_service import EtaService, default_model
    from routest_amd.serve.frontend import ServingStack
    model = default_model(steps=30)
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="1", route_gpu_min_stops=1, warm_scorer=False)
    sv = build_services(s, eta=EtaService(model, devices=[0]), provider=HaversineProvider(), store=None)
    st = ServingStack(sv, create_app(sv), model, [0], threads=2, timeout_us=300)

    def post(port, body):
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/api/optimize_route", body=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, r.read()
    try:
        assert st.front.routes, "native routes not enabled"
        body = _request(12, 21, cap=9, tw_improve=True)
        body["destination_points"][0]["time_window"] = [0, 7200]
        f0 = st.front.stats()
        a = post(st.port, body)
        b = post(st.app_server.port, body)
        f1 = st.front.stats()
        assert a[0] == 200 and a == b, (a[1][:300], b[1][:300])
        assert json.loads(a[1])["properties"]["time_windows"]["method"] == "cheapest_insertion+relocate+swap"
        assert f1["relayed"] - f0["relayed"] == 1 and f1["route_flushes"] == f0["route_flushes"], (f0, f1)
    finally:
        st.close()
