"""K6d (``_C.route_tw_trips``, csrc/route_tw.hip) against the Python reference
(routing/timewindows.py): ``visit`` / ``trip_of`` / ``ntrips`` / ``status``, the arrival and start
milliseconds and the statistics are compared with ``torch.equal``; then the device path of
``batched_trips`` against the CPU path, the app on the GPU road router against the CPU router, and
the main port relaying a time-window request.  Instances: tests/_tw_cases.py."""
import json

import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import batched_trips, pack_requests
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.timewindows import parse_time_windows, tw_trips

from _tw_cases import expected, expected_rows, named_instances, pack_rows, random_instance

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

DEV = "cuda:0"
OUT = ("visit", "trip_of", "ntrips", "status", "arrival_q", "start_q", "stats")


def _launch(cases, nm, flags=None):
    C = _ext.native(required=True)
    D, T, npts, dem, cap, maxd, op, cl, sv = pack_rows(cases, nm)
    f = np.ones(len(cases), np.uint8) if flags is None else np.asarray(flags, np.uint8)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(DEV)  # noqa: E731
    out = C.route_tw_trips(t(D), t(T), t(npts, torch.int32), t(dem), t(cap), t(maxd), t(op, torch.int64),
                           t(cl, torch.int64), t(sv, torch.int64), t(f, torch.uint8))
    torch.cuda.synchronize()
    assert len(out) == len(OUT)
    return [c.cpu() for c in out]


def _want(cases, answers, nm):
    rows = [expected_rows(c, a, nm) for c, a in zip(cases, answers)]
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
    _compare(_launch(cases, nm), _want(cases, [expected(n) for n in names], nm), names)


SMALL = [n for n, c in named_instances().items() if len(c["d"]) - 1 <= 32]
LARGE = [n for n, c in named_instances().items() if len(c["d"]) - 1 > 32]


def test_small_tier_equals_reference_on_every_instance():
    """Rows of at most 32 stops in a batch whose width keeps the launch to the wave tier."""
    assert {"random_ns1", "random_ns2", "random_ns31", "random_ns32", "infeasible_alone", "grid_ties",
            "special_entries", "reject_float_walk", "seed_ties", "zero_width", "waiting"} <= set(SMALL)
    _check(SMALL, 33)


def test_large_tier_equals_reference_on_every_instance():
    assert {"random_ns33", "random_ns64", "random_ns127", "random_ns128", "road_ns33", "grid_ties_ns40",
            "zero_width_ns36", "grid_maxd_equal_ns40"} <= set(LARGE)
    _check(LARGE, 129)


def test_both_tiers_in_one_launch_and_every_padding_width():
    """Every instance in one batch of width 129 (each row taken by the tier its stop count picks),
    and the small ones again at a width that is no multiple of anything."""
    _check(SMALL + LARGE, 129)
    _check([n for n in SMALL if len(named_instances()[n]["d"]) <= 15], 15)


def test_mixed_batch_leaves_unflagged_rows_alone():
    """Flagged and unflagged rows side by side, with npts 0 and 1 padding rows: K6d writes nothing
    for an unflagged row, and the flagged rows get the answers they get alone."""
    names = ["random_ns31", "grid_ties", "random_ns33", "zero_width", "road_ns12", "random_ns64", "waiting"]
    flags = [1, 0, 1, 1, 0, 0, 1]
    cases = [named_instances()[n] for n in names]
    D, T, npts, dem, cap, maxd, op, cl, sv = pack_rows(cases, 65)
    C = _ext.native(required=True)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(DEV)  # noqa: E731
    pad = lambda a, v=0: np.concatenate([a, np.full((2,) + a.shape[1:], v, dtype=a.dtype)])  # noqa: E731
    npts2 = np.concatenate([npts, np.array([0, 1], dtype=np.int32)])
    flags2 = np.array(flags + [1, 1], dtype=np.uint8)
    args = [t(pad(D)), t(pad(T)), t(npts2, torch.int32), t(pad(dem)), t(pad(cap)), t(pad(maxd)),
            t(pad(op), torch.int64), t(pad(cl), torch.int64), t(pad(sv), torch.int64)]
    got = [c.cpu() for c in C.route_tw_trips(*args, t(flags2, torch.uint8))]
    greedy = [c.cpu() for c in C.route_greedy_cvrp(args[0], args[2], args[3], args[4], args[5])]
    torch.cuda.synchronize()
    want = _want(cases, [expected(n) for n in names], 65)
    for key, g, w in zip(OUT, got, want):
        for k, f in enumerate(flags):
            if f:
                assert torch.equal(g[k], w[k].to(g.dtype)), (key, names[k])
            else:       # the fill of the binding: nothing was written
                assert bool((g[k] == (-1 if key in ("visit", "trip_of", "arrival_q", "start_q") else 0)).all()), (key, names[k])
        # npts 0 and 1: no stops, no trips, status 0
        for k in (7, 8):
            assert bool((g[k] == (-1 if key in ("visit", "trip_of", "arrival_q", "start_q") else 0)).all()), key
    # merged as batched_trips does it, the unflagged rows are route_greedy_cvrp's alone
    reqs = []
    for c in cases:
        n = len(c["d"])
        reqs.append({"source_point": {"lat": 0.0, "lon": 0.0},
                     "destination_points": [{"lat": 0.0, "lon": 0.0, "payload": c["demand"][s]} for s in range(1, n)],
                     "driver_details": {"vehicle_capacity": c["cap"], "maximum_distance": c["max_dist"]}})
    tw = [(c["open_q"], c["close_q"], c["sv_q"]) if f else None for c, f in zip(cases, flags)]
    res, _, sched = batched_trips(reqs, device=DEV, D=D, T=T, time_windows=tw)
    plain = batched_trips(reqs, device=DEV, D=D)
    for k, f in enumerate(flags):
        if f:
            assert res[k] == expected(names[k])[0] and sched[k] == (expected(names[k])[1], expected(names[k])[2])
        else:
            assert res[k] == plain[k] and sched[k] is None
            v, to = greedy[0][k].numpy(), greedy[1][k].numpy()
            trips = [[0] + [int(s) for s, x in zip(v, to) if x == j and s > 0] + [0] for j in range(int(greedy[2][k]))]
            assert res[k] == trips


@pytest.mark.parametrize("ns_lo,ns_hi,nm", [(1, 32, 33), (33, 128, 129)])
def test_random_rows_equal_reference(ns_lo, ns_hi, nm):
    """64 random rows per tier: windows on 70 % of the stops, road-like seconds on every other row,
    a binding capacity on every third."""
    rng = np.random.default_rng(ns_hi)
    sizes = [int(v) for v in rng.integers(ns_lo, min(ns_hi, 48 if ns_lo > 32 else ns_hi) + 1, 62)] + [ns_lo, ns_hi]
    cases = [random_instance(ns, 70_000 + ns_hi * 100 + k, road=bool(k % 2), cap_frac=(None, 0.3)[k % 3 == 0])
             for k, ns in enumerate(sizes)]
    answers = []
    for c in cases:
        try:
            answers.append(tw_trips(**c))
        except InfeasibleStops as e:
            answers.append(("infeasible", e.stops))
    assert sum(a[0] != "infeasible" and len(a[0]) > 1 for a in answers) > 20
    _compare(_launch(cases, nm), _want(cases, answers, nm), [f"row{k}_ns{ns}" for k, ns in enumerate(sizes)])


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
    """``batched_trips(device="cuda")`` == ``batched_trips`` on the CPU with time-window rows beside
    plain, improve and exchange rows: on K5's haversine matrix and on a given road D / T."""
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
    gpu = batched_trips(reqs, device=DEV, time_windows=tw, improve=imp, exchange=exc)
    cpu = batched_trips(reqs, device=None, time_windows=tw, improve=imp, exchange=exc)
    _same(gpu, cpu)
    assert isinstance(gpu[0][5], InfeasibleStops) and "time window" in str(gpu[0][5])
    assert gpu[1][1] is not None and gpu[1][4] is not None and gpu[1][0] is None and gpu[1][3] is None
    assert gpu[2][1] is None and gpu[2][6] is not None and sum(len(t) - 2 for t in gpu[0][6]) == 128
    base = batched_trips(reqs, device=DEV, improve=imp, exchange=exc)
    assert gpu[0][1] == base[0][1] and gpu[0][4] == base[0][4] and gpu[1][1] == base[1][1]
    # a given road-like D / T (seconds unrelated to the metres)
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    nm = lat.shape[1]
    rng = np.random.default_rng(11)
    D = rng.uniform(200.0, 9000.0, (len(reqs), nm, nm))
    T = rng.uniform(20.0, 900.0, (len(reqs), nm, nm))
    for M in (D, T):
        M[:, np.arange(nm), np.arange(nm)] = 0.0
    _same(batched_trips(reqs, device=DEV, D=D, T=T, time_windows=tw, improve=imp, exchange=exc),
          batched_trips(reqs, device=None, D=D, T=T, time_windows=tw, improve=imp, exchange=exc))
    # a batch nobody flags is the call without the argument
    assert batched_trips(reqs, device=DEV, time_windows=[None] * 8)[0] == batched_trips(reqs, device=DEV)


def test_app_on_the_gpu_router_equals_the_cpu_router():
    """One time-window request through the app on the GPU graph provider (per-request path and the
    batcher's flush) equals ``optimize_route`` on the CPU CCH router.  Both routers customize the
    same given edge costs: learned costs are evaluated by the ETA model on each provider's own
    device and differ in the last digits there, for any request."""
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
    idx = rng.choice(g.num_nodes, 9, replace=False)
    body = {"source_point": {"lat": float(g.lat[idx[0]]), "lon": float(g.lon[idx[0]])},
            "destination_points": [{"lat": float(g.lat[j]), "lon": float(g.lon[j]), "payload": 1} for j in idx[1:]],
            "driver_details": {"vehicle_capacity": 5, "maximum_distance": 1e7}}
    body["destination_points"][0]["time_window"] = [14400, 18000]
    body["destination_points"][3]["time_window"] = [0, 36000]
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
        assert got["properties"]["time_windows"]["stops_with_windows"] == 2
        assert got["properties"]["time_windows"]["waiting"] > 0
        assert got == json.loads(json.dumps(want)), batch


def test_main_port_relays_requests_with_time_windows():
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
        body = _request(6, 21)
        body["destination_points"][0]["time_window"] = [0, 7200]
        f0 = st.front.stats()
        a = post(st.port, body)
        b = post(st.app_server.port, body)
        f1 = st.front.stats()
        assert a[0] == 200 and a == b, (a[1][:300], b[1][:300])
        assert json.loads(a[1])["properties"]["time_windows"]["method"] == "cheapest_insertion"
        assert f1["relayed"] - f0["relayed"] == 1 and f1["route_flushes"] == f0["route_flushes"], (f0, f1)
    finally:
        st.close()
