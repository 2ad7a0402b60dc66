"""K6f followed by K6g (``_C.route_pd_improve``, csrc/route_pd_improve.hip) against the reference
(routing/shipment_improve.py; for rows above 48 stops the host C++ ``_rt.pd_improve``, which the CPU
test holds equal to it): ``visit`` / ``trip_of`` / ``ntrips`` / ``status``, the arrival and start
milliseconds and the 8 statistics are compared with ``torch.equal``; then the device path of
``batched_trips`` against the CPU path, the app on the GPU road router against the CPU router, and the
main port relaying such a request.  Instances: tests/_pd_improve_cases.py."""
import functools
import json

import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import batched_trips, pack_requests
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.optimizer import _tw_or_none
from routest_amd.routing.shipment_improve import METHOD, STAT_KEYS

import _pd_cases
from _pd_cases import pack_rows, paired
from _pd_improve_cases import built, expected, improve, named_instances, skip_cases
from _tw_cases import random_instance

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

DEV = "cuda:0"
OUT = ("visit", "trip_of", "ntrips", "status", "arrival_q", "start_q")


def _t(a, dt=torch.float64):
    return torch.as_tensor(a, dtype=dt).to(DEV)


def _args(cases, nm):
    D, T, npts, dem, cap, maxd, op, cl, sv, pf = pack_rows(cases, nm)
    return [_t(D), _t(T), _t(npts, torch.int32), _t(dem), _t(cap), _t(maxd), _t(op, torch.int64), _t(cl, torch.int64),
            _t(sv, torch.int64), _t(pf, torch.int32)]


def _launch(cases, nm, flags=None, args=None):
    """K6f over every row, then K6g over the flagged ones: the six outputs and K6g's statistics."""
    C = _ext.native(required=True)
    args = _args(cases, nm) if args is None else args
    R = int(args[0].shape[0])
    f = np.ones(R, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    out = C.route_pd_trips(*args, _t(np.ones(R, np.uint8), torch.uint8))
    stats = C.route_pd_improve(*args, *out[:6], _t(f, torch.uint8))
    torch.cuda.synchronize()
    assert tuple(stats.shape) == (R, 8) and stats.dtype == torch.int64
    return [c.cpu() for c in out[:6]] + [stats.cpu()]


def _rt_answer(c, trips):
    rt = _ext.runtime(required=True)
    got = rt.pd_improve(np.asarray(c["d"], dtype=np.float64), np.asarray(c["t"], dtype=np.float64), trips, c["demand"],
                        c["cap"], c["max_dist"], c["open_q"], c["close_q"], c["sv_q"], c["pickup_from"])
    return ([list(t) for t in got[0]], [[tuple(e) for e in trip] for trip in got[1]], dict(got[2]))


def _answer(c):
    """The expectation for an instance: the reference, or the host C++ above 48 stops."""
    trips = built(c)
    return _rt_answer(c, trips) if len(c["d"]) - 1 > 48 else improve(c, trips)


@functools.lru_cache(maxsize=None)
def _named_answer(name):
    c = named_instances()[name]
    return _rt_answer(c, built(c)) if len(c["d"]) - 1 > 48 else expected(name)[:3]


def _rows(answer, nm):
    trips, schedule, st = answer
    visit = np.full(nm, -1, dtype=np.int32)
    trip_of = np.full(nm, -1, dtype=np.int32)
    arr = np.full(nm, -1, dtype=np.int64)
    start = np.full(nm, -1, dtype=np.int64)
    p = 0
    for t, rows in enumerate(schedule):
        for s, a, b, _ in rows:
            visit[p], trip_of[p], arr[p], start[p] = s, t, a, b
            p += 1
    return visit, trip_of, len(trips), 0, arr, start, np.array([st[k] for k in STAT_KEYS], dtype=np.int64)


def _want(answers, nm):
    rows = [_rows(a, nm) for a in answers]
    return [torch.from_numpy(np.stack([np.asarray(r[i]) for r in rows])) for i in range(7)]


def _compare(got, want, names):
    for key, g, w in zip(OUT + ("stats",), got, want):
        w = w.to(g.dtype)
        if not torch.equal(g, w):
            bad = [names[k] for k in range(len(names)) if not torch.equal(g[k], w[k])]
            raise AssertionError(f"{key} differs on {bad}")


def _check(names, nm):
    cases = [named_instances()[n] for n in names]
    _compare(_launch(cases, nm), _want([_named_answer(n) for n in names], nm), names)


SMALL = [n for n, c in named_instances().items() if len(c["d"]) - 1 <= 32]
LARGE = [n for n, c in named_instances().items() if len(c["d"]) - 1 > 32]
ISSUE = ["separated_only_move", "load_max", "late_after_removal", "empties_trip", "float_reject_move", "grid_tie_move",
         "random_ns31", "random_ns32", "cap_bound_ns20", "road_ns12", "capacity_bind", "grid_ties", "one_pair",
         "all_pairs_ns16", "no_pairs"]


def test_small_tier_equals_reference_on_every_instance():
    """Rows of at most 32 stops in a batch whose width keeps the launch to the wave tier."""
    assert set(ISSUE) <= set(SMALL)
    assert sum(_named_answer(n)[2]["moves"] > 0 for n in SMALL) >= 12
    _check(SMALL, 33)


def test_named_instances_again_in_the_large_tier():
    """The named instances posed again with more than 32 stops so that the large tier takes them:
    the instance's own points keep their indices and plain stops of demand 0 without windows, 50 km
    and 5000 s from everything, are appended up to 34 stops.  The reference is asked again for the
    padded instance."""
    names, cases = [], []
    for n in ISSUE:
        c = named_instances()[n]
        n1 = len(c["d"])
        extra = 34 - (n1 - 1)
        m = n1 + extra
        d = np.full((m, m), 50_000.0)
        t = np.full((m, m), 5_000.0)
        np.fill_diagonal(d, 0.0)
        np.fill_diagonal(t, 0.0)
        d[:n1, :n1], t[:n1, :n1] = c["d"], c["t"]
        cases.append(dict(c, d=d.tolist(), t=t.tolist(), demand=list(c["demand"]) + [0.0] * extra,
                          open_q=list(c["open_q"]) + [0] * extra, close_q=list(c["close_q"]) + [1 << 62] * extra,
                          sv_q=list(c["sv_q"]) + [0] * extra, pickup_from=list(c["pickup_from"]) + [-1] * extra))
        names.append(n + "_padded")
    assert all(len(c["d"]) - 1 == 34 for c in cases)
    answers = [_answer(c) for c in cases]
    assert sum(a[2]["moves"] > 0 for a in answers) >= 10 and any(a[2]["rejected"] for a in answers)
    _compare(_launch(cases, 129), _want(answers, 129), names)


def test_large_tier_equals_reference_on_every_instance():
    assert {"random_ns33", "random_ns64", "random_ns127", "random_ns128", "grid_ties_ns40", "road_cap_ns40"} <= set(LARGE)
    assert all(_named_answer(n)[2]["pair_moves"] > 0 for n in ("random_ns33", "random_ns64", "random_ns127", "random_ns128"))
    _check(LARGE, 129)


def test_both_tiers_in_one_launch_and_an_odd_width():
    """Every instance in one batch of width 129 (each row taken by the tier its stop count picks),
    and the rows of at most 40 stops at the odd width 47."""
    _check(SMALL + LARGE, 129)
    _check([n for n in SMALL + LARGE if len(named_instances()[n]["d"]) <= 41], 47)


@pytest.mark.parametrize("ns", [2, 3, 32, 33, 128])
def test_sizes_at_the_tier_and_capacity_bounds(ns):
    _check([f"random_ns{ns}"], ns + 1)


def test_rows_that_are_not_asked_or_not_planned_are_left_alone():
    """Unflagged rows, rows K6f gave a status other than 0 (an infeasible pair, a malformed
    ``pickup_from``) and ``npts`` 0 / 1 rows come out of K6g bit-identical to K6f's outputs, with
    statistics of 0; the flagged rows beside them get the answers they get alone."""
    names = ["random_ns31", "grid_ties", "random_ns33", "cap_bound_ns20", "road_ns12", "random_ns64", "empties_trip"]
    flags = [1, 0, 1, 1, 0, 0, 1]
    cases = [named_instances()[n] for n in names]
    bad = _pd_cases.named_instances()["infeasible_pair"]
    mal = dict(_pd_cases.named_instances()["pair_plus_plain"], pickup_from=[-1, 2, 3, -1])
    cases += [bad, mal]
    flags += [1, 1]
    args = _args(cases, 65)
    pad = lambda a, v=0: torch.cat([a, torch.full((2,) + tuple(a.shape[1:]), v, dtype=a.dtype, device=a.device)])  # noqa: E731
    args = [pad(a, -1) if k == 9 else pad(a) for k, a in enumerate(args)]
    args[2][9], args[2][10] = 0, 1
    flags += [1, 1]
    C = _ext.native(required=True)
    ones = _t(np.ones(len(flags), np.uint8), torch.uint8)
    k6f = [c.cpu() for c in C.route_pd_trips(*args, ones)[:6]]
    got = _launch(None, 65, flags, args)
    assert k6f[3].tolist() == [0] * 7 + [1, 3, 0, 0]
    want = _want([_named_answer(n) for n in names], 65)
    for x, (key, g) in enumerate(zip(OUT + ("stats",), got)):
        for k, f in enumerate(flags):
            if f and k < 7:
                assert torch.equal(g[k], want[x][k].to(g.dtype)), (key, names[k])
            elif key == "stats":
                assert bool((g[k] == 0).all()), (key, k)
            else:
                assert torch.equal(g[k], k6f[x][k]), (key, k)
    assert any(not torch.equal(got[0][k], k6f[0][k]) for k in (0, 2, 3, 6))


def test_skipped_rows_report_the_trips_as_given():
    """The skip conditions the kernel can meet (K6f plans no such row, so its outputs are taken from
    the sound sibling): the six outputs stay and the statistics say 0 moves."""
    skips = {n: v for n, v in skip_cases().items() if n != "ns129"}
    base = _pd_cases.named_instances()["cap_bound_ns20"]
    C = _ext.native(required=True)
    sound = _args([base] * len(skips), 21)
    out = C.route_pd_trips(*sound, _t(np.ones(len(skips), np.uint8), torch.uint8))
    before = [c.cpu().clone() for c in out[:6]]
    args = _args([c for c, _ in skips.values()], 21)
    stats = C.route_pd_improve(*args, *out[:6], _t(np.ones(len(skips), np.uint8), torch.uint8)).cpu()
    torch.cuda.synchronize()
    for g, w in zip(out[:6], before):
        assert torch.equal(g.cpu(), w)
    want = torch.from_numpy(np.stack([np.array([improve(c, tr)[2][k] for k in STAT_KEYS]) for c, tr in skips.values()]))
    assert torch.equal(stats, want) and bool((stats[:, 0] == 0).all())


@functools.lru_cache(maxsize=None)
def _random_rows(ns_lo, ns_hi):
    """48 random rows of ``ns_lo..ns_hi`` stops that ``pd_trips`` can plan, with the host C++'s
    answers; the seeds are walked until 48 rows are found."""
    rng = np.random.default_rng(ns_hi)
    cases, answers, k = [], [], 0
    while len(cases) < 48:
        ns = (ns_lo, ns_hi)[len(cases)] if len(cases) < 2 else int(rng.integers(ns_lo, ns_hi + 1))
        c = paired(random_instance(ns, 90_000 + ns_hi * 100 + k, windowed=0.4, road=bool(k % 2),
                                   cap_frac=(None, 0.3)[k % 3 == 0]), k, frac=(0.5, 1.0)[k % 5 == 0])
        k += 1
        trips = built(c)
        if trips is not None:
            cases.append(c)
            answers.append(_rt_answer(c, trips))
    return cases, answers


@pytest.mark.parametrize("ns_lo,ns_hi,nm", [(1, 32, 33), (33, 128, 129)])
def test_random_rows_equal_the_host_cpp(ns_lo, ns_hi, nm):
    cases, answers = _random_rows(ns_lo, ns_hi)
    assert sum(a[2]["moves"] > 0 for a in answers) >= 16      # at least a third of the rows apply a move
    assert sum(a[2]["pair_moves"] > 0 for a in answers) >= 5
    _compare(_launch(cases, nm), _want(answers, nm), [f"row{k}_ns{len(c['d']) - 1}" for k, c in enumerate(cases)])


def _request(n, seed, cap=99, pairs=True, **extra):
    rng = np.random.default_rng(seed)
    lat, lon = 14.55 + rng.normal(0, 0.03, n + 1), 121.02 + rng.normal(0, 0.03, n + 1)
    r = {"source_point": {"lat": float(lat[0]), "lon": float(lon[0])},
         "destination_points": [{"lat": float(lat[i]), "lon": float(lon[i]), "payload": int(rng.integers(1, 4))}
                                for i in range(1, n + 1)],
         "driver_details": {"vehicle_capacity": cap, "maximum_distance": 1e7, "vehicle_type": ["car", "bike"][seed % 2]}}
    for p in r["destination_points"]:
        if rng.random() < 0.3:
            lo = float(rng.uniform(0, 6 * 3600))
            p["time_window"] = [round(lo, 1), round(lo + float(rng.uniform(3 * 3600, 8 * 3600)), 1)]
        if rng.random() < 0.5:
            p["service"] = int(rng.integers(0, 600))
    if pairs:
        order = [int(v) for v in rng.permutation(n)]
        for x in range(n // 4):
            pk, dl = order[2 * x], order[2 * x + 1]
            r["destination_points"][dl]["pickup_from"] = pk
            r["destination_points"][pk].pop("payload")
            r["destination_points"][dl].pop("time_window", None)
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
    """``batched_trips(device="cuda")`` == ``batched_trips`` on the CPU with shipment-improve rows
    beside ``tw_improve``, plain and exchange rows: on K5's haversine matrix and on a given road D / T."""
    reqs = [_request(n, s, cap=c, pairs=p) for n, s, c, p in
            ((2, 1, 9, True), (5, 2, 6, False), (12, 3, 9, True), (33, 4, 30, True), (40, 5, 40, False), (9, 6, 7, True),
             (64, 7, 200, True), (20, 8, 15, False), (24, 9, 12, True))]
    reqs[0]["destination_points"][1]["pickup_from"] = 0
    reqs[0]["destination_points"][0].pop("payload", None)
    v = next(i for i, p in enumerate(reqs[5]["destination_points"]) if "pickup_from" in p)
    reqs[5]["destination_points"][v]["time_window"] = [0, 0]            # an infeasible pair
    for p in reqs[1]["destination_points"]:                             # a row without any of the fields
        p.pop("time_window", None)
        p.pop("service", None)
    tw = [_tw_or_none(r) for r in reqs]
    assert [len(v or ()) for v in tw] == [4, 0, 4, 4, 3, 4, 4, 3, 4]
    imp = [True, True, False, False, False, False, True, False, False]
    exc = [False, False, False, True, True, False, False, False, False]
    twi = [True, False, True, False, True, False, False, True, False]
    pdi = [True, True, True, True, True, True, True, True, False]
    kw = dict(time_windows=tw, improve=imp, exchange=exc, tw_improve=twi, shipment_improve=pdi)
    gpu = batched_trips(reqs, device=DEV, **kw)
    _same(gpu, batched_trips(reqs, device=None, **kw))
    # the flag is honoured on shipment rows only, and only where it is set
    assert [v is not None and len(v[1].get("search", ())) == 8 for v in gpu[2]] == \
        [True, False, True, True, False, False, True, False, False]
    assert isinstance(gpu[0][5], InfeasibleStops)
    assert sum(gpu[2][k][1]["search"]["moves"] for k in (2, 3, 6)) > 10
    base = batched_trips(reqs, device=DEV, time_windows=tw, improve=imp, exchange=exc, tw_improve=twi)
    for k in (1, 4, 5, 7, 8):
        assert gpu[0][k] == base[0][k] or isinstance(gpu[0][k], InfeasibleStops)
        assert gpu[1][k] == base[1][k] and gpu[2][k] == base[2][k]
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
    assert batched_trips(reqs, device=DEV, time_windows=tw, shipment_improve=[False] * 9)[2] == \
        batched_trips(reqs, device=DEV, time_windows=tw)[2]


def test_app_on_the_gpu_router_equals_the_cpu_router():
    """One ``shipment_improve`` request through the app on the GPU graph provider (per-request path
    and the batcher's flush) equals ``optimize_route`` on the CPU CCH router.  Both routers customize
    the same given edge costs."""
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
            "driver_details": {"vehicle_capacity": 3, "maximum_distance": 1e7}, "shipment_improve": True}
    for dl, pk in ((0, 6), (4, 2), (9, 11)):
        body["destination_points"][dl]["pickup_from"] = pk
        body["destination_points"][pk].pop("payload")
    body["destination_points"][3]["time_window"] = [0, 36000]
    body["destination_points"][6]["time_window"] = [3600, 18000]
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
        assert tw["method"] == METHOD and tw["stops_with_windows"] == 2 and got["properties"]["shipments"]["pairs"] == 3
        assert tw["matrix_distance_after"] <= tw["matrix_distance_before"]
        assert got == json.loads(json.dumps(want)), batch


def test_main_port_relays_requests_with_the_field():
    """The native front end does not answer shipment requests: relayed, the app's bytes, no native
    flush."""
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
        body = _request(12, 21, cap=9, shipment_improve=True)
        f0 = st.front.stats()
        a = post(st.port, body)
        b = post(st.app_server.port, body)
        f1 = st.front.stats()
        assert a[0] == 200 and a == b, (a[1][:300], b[1][:300])
        assert json.loads(a[1])["properties"]["time_windows"]["method"] == METHOD
        assert f1["relayed"] - f0["relayed"] == 1 and f1["route_flushes"] == f0["route_flushes"], (f0, f1)
    finally:
        st.close()
