"""K6f (``_C.route_pd_trips``, csrc/route_pd.hip) against the Python reference
(routing/shipments.py): ``visit`` / ``trip_of`` / ``ntrips`` / ``status``, the arrival and start
milliseconds and the statistics are compared with ``torch.equal``; then the device path of
``batched_trips`` against the CPU path, the app on the GPU road router against the CPU router, and
the main port relaying a shipment request.  Instances: tests/_pd_cases.py."""
import json

import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import batched_trips, pack_requests
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.optimizer import _tw_or_none

from _pd_cases import answer, expected, named_instances, pack_rows, paired
from _tw_cases import expected_rows, random_instance

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

DEV = "cuda:0"
OUT = ("visit", "trip_of", "ntrips", "status", "arrival_q", "start_q", "stats")
FILL = {"visit": -1, "trip_of": -1, "arrival_q": -1, "start_q": -1}


def _t(a, dt=torch.float64):
    return torch.as_tensor(a, dtype=dt).to(DEV)


def _args(cases, nm):
    D, T, npts, dem, cap, maxd, op, cl, sv, pf = pack_rows(cases, nm)
    return [_t(D), _t(T), _t(npts, torch.int32), _t(dem), _t(cap), _t(maxd), _t(op, torch.int64), _t(cl, torch.int64),
            _t(sv, torch.int64), _t(pf, torch.int32)]


def _launch(cases, nm, flags=None):
    C = _ext.native(required=True)
    f = np.ones(len(cases), np.uint8) if flags is None else np.asarray(flags, np.uint8)
    out = C.route_pd_trips(*_args(cases, nm), _t(f, torch.uint8))
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
ISSUE = ["one_pair", "pair_plus_plain", "separated_only", "adjacent_only", "capacity_bind", "z_fail",
         "zero_width_delivery", "grid_ties", "float_reject", "infeasible_pair", "unreachable_mate", "no_pairs"]


def test_small_tier_equals_reference_on_every_instance():
    """Rows of at most 32 stops in a batch whose width keeps the launch to the wave tier."""
    assert set(ISSUE) | {"random_ns2", "random_ns3", "random_ns31", "random_ns32", "special_entries"} <= set(SMALL)
    _check(SMALL, 33)


def test_named_instances_again_in_the_large_tier():
    """The instances the issue names, posed again with more than 32 stops so that the large tier
    takes them: the instance's own points keep their indices and plain stops of demand 0 without
    windows, 50 km and 5000 s from everything, are appended up to 34 stops.  The reference is asked
    again for the padded instance."""
    names, cases = [], []
    for n in ISSUE:
        c = named_instances()[n]
        n1 = len(c["d"])
        extra = 34 - (n1 - 1) if n1 - 1 < 34 else 0
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
    assert all(len(c["d"]) - 1 > 32 for c in cases)
    _compare(_launch(cases, 129), _want(cases, [answer(c) for c in cases], 129), names)


def test_large_tier_equals_reference_on_every_instance():
    assert {"random_ns33", "random_ns64", "random_ns127", "random_ns128", "grid_ties_ns40", "road_cap_ns40"} <= set(LARGE)
    _check(LARGE, 129)


def test_both_tiers_in_one_launch_and_every_padding_width():
    """Every instance in one batch of width 129 (each row taken by the tier its stop count picks),
    the rows of at most 40 stops at a width in between, and the small ones at a width that is no
    multiple of anything."""
    _check(SMALL + LARGE, 129)
    _check([n for n in SMALL + LARGE if len(named_instances()[n]["d"]) <= 41], 47)
    _check([n for n in SMALL if len(named_instances()[n]["d"]) <= 15], 15)


@pytest.mark.parametrize("ns", [2, 3, 32, 33, 128])
def test_sizes_at_the_tier_and_capacity_bounds(ns):
    name = f"random_ns{ns}"
    assert sum(1 for p in named_instances()[name]["pickup_from"] if p > 0) >= 1 and expected(name)[0] != "infeasible"
    _check([name], ns + 1)


def test_malformed_pairs_are_status_3():
    c = named_instances()["pair_plus_plain"]
    rows = [dict(c, pickup_from=pf) for pf in ([-1, 2, 3, -1], [-1, -1, 3, 3], [-1, 1, -1, -1], [-1, 4, -1, -1],
                                               [-1, 0, -1, -1], [-1, 3, -1, 2], [-1, -1, 1, 1])] + [c]
    got = _launch(rows, 5)
    assert got[3].tolist() == [3] * 7 + [0] and got[2].tolist() == [0] * 7 + [1]
    assert bool((got[0][:7] == -1).all()) and bool((got[6][:7] == 0).all())
    _compare([g[7:] for g in got], _want([c], [expected("pair_plus_plain")], 5), ["pair_plus_plain"])


def test_mixed_batch_leaves_unflagged_rows_alone():
    """Flagged and unflagged rows side by side, with npts 0 and 1 padding rows: K6f writes nothing
    for an unflagged row, and the flagged rows get the answers they get alone."""
    names = ["random_ns31", "grid_ties", "random_ns33", "zero_width_delivery", "road_ns12", "random_ns64", "z_fail"]
    flags = [1, 0, 1, 1, 0, 0, 1]
    cases = [named_instances()[n] for n in names]
    args = _args(cases, 65)
    pad = lambda a, v=0: torch.cat([a, torch.full((2,) + tuple(a.shape[1:]), v, dtype=a.dtype, device=a.device)])  # noqa: E731
    args = [pad(a, -1) if k == 9 else pad(a) for k, a in enumerate(args)]
    args[2][7], args[2][8] = 0, 1
    C = _ext.native(required=True)
    got = [c.cpu() for c in C.route_pd_trips(*args, _t(np.array(flags + [1, 1], np.uint8), torch.uint8))]
    torch.cuda.synchronize()
    want = _want(cases, [expected(n) for n in names], 65)
    for key, g, w in zip(OUT, got, want):
        for k, f in enumerate(flags):
            if f:
                assert torch.equal(g[k], w[k].to(g.dtype)), (key, names[k])
            else:       # the fill of the binding: nothing was written
                assert bool((g[k] == FILL.get(key, 0)).all()), (key, names[k])
        for k in (7, 8):    # npts 0 and 1: no stops, no trips, status 0
            assert bool((g[k] == FILL.get(key, 0)).all()), key


@pytest.mark.parametrize("ns_lo,ns_hi,nm", [(1, 32, 33), (33, 128, 129)])
def test_random_rows_equal_reference(ns_lo, ns_hi, nm):
    """48 random rows per tier, about half of the stops paired (all of them on every fifth row):
    windows on 40 % of the stops, road-like seconds on every other row, a binding capacity on every
    third."""
    rng = np.random.default_rng(ns_hi)
    sizes = [int(v) for v in rng.integers(ns_lo, min(ns_hi, 48 if ns_lo > 32 else ns_hi) + 1, 46)] + [ns_lo, ns_hi]
    cases = [paired(random_instance(ns, 80_000 + ns_hi * 100 + k, windowed=0.4, road=bool(k % 2),
                                    cap_frac=(None, 0.3)[k % 3 == 0]), k, frac=(0.5, 1.0)[k % 5 == 0])
             for k, ns in enumerate(sizes)]
    answers = [answer(c) for c in cases]
    assert sum(a[0] != "infeasible" and a[2]["insertions"] > 2 for a in answers) > 20
    _compare(_launch(cases, nm), _want(cases, answers, nm), [f"row{k}_ns{ns}" for k, ns in enumerate(sizes)])


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
    """``batched_trips(device="cuda")`` == ``batched_trips`` on the CPU with shipment rows beside
    time-window, plain, improve and exchange rows: on K5's haversine matrix and on a given road D / T."""
    reqs = [_request(n, s, cap=c, pairs=p) for n, s, c, p in
            ((2, 1, 9, True), (5, 2, 6, False), (12, 3, 9, True), (33, 4, 30, True), (40, 5, 40, False), (9, 6, 7, True),
             (128, 7, 400, True), (20, 8, 15, False))]
    reqs[0]["destination_points"][1]["pickup_from"] = 0
    reqs[0]["destination_points"][0].pop("payload", None)
    v = next(i for i, p in enumerate(reqs[5]["destination_points"]) if "pickup_from" in p)
    reqs[5]["destination_points"][v]["time_window"] = [0, 0]            # an infeasible pair
    for p in reqs[1]["destination_points"]:                             # a row without any of the fields
        p.pop("time_window", None)
        p.pop("service", None)
    tw = [_tw_or_none(r) for r in reqs]
    assert [len(v or ()) for v in tw] == [4, 0, 4, 4, 3, 4, 4, 3]
    imp = [True, True, False, False, False, False, True, False]
    exc = [False, False, False, True, True, False, False, False]
    twi = [True, False, True, False, True, False, False, False]
    gpu = batched_trips(reqs, device=DEV, time_windows=tw, improve=imp, exchange=exc, tw_improve=twi)
    cpu = batched_trips(reqs, device=None, time_windows=tw, improve=imp, exchange=exc, tw_improve=twi)
    _same(gpu, cpu)
    assert isinstance(gpu[0][5], InfeasibleStops) and len(gpu[0][5].stops) >= 2
    assert gpu[1][1] is not None and gpu[1][0] is None and gpu[1][3] is None and gpu[1][6] is None
    assert "search" in gpu[2][4][1] and "search" not in gpu[2][0][1] and "search" not in gpu[2][2][1]
    assert sum(len(t) - 2 for t in gpu[0][6]) == 128
    # the rows that are no shipment rows are what the call gives without them
    keep = [1, 4, 7]
    base = batched_trips([reqs[k] for k in keep], device=DEV, time_windows=[tw[k] for k in keep],
                         improve=[imp[k] for k in keep], exchange=[exc[k] for k in keep],
                         tw_improve=[twi[k] for k in keep])
    for x in range(3):
        assert [gpu[x][k] for k in keep] == base[x]
    # a given road-like D / T (seconds unrelated to the metres)
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    nm = lat.shape[1]
    rng = np.random.default_rng(11)
    D = rng.uniform(200.0, 9000.0, (len(reqs), nm, nm))
    T = rng.uniform(20.0, 900.0, (len(reqs), nm, nm))
    for M in (D, T):
        M[:, np.arange(nm), np.arange(nm)] = 0.0
    _same(batched_trips(reqs, device=DEV, D=D, T=T, time_windows=tw, improve=imp, exchange=exc, tw_improve=twi),
          batched_trips(reqs, device=None, D=D, T=T, time_windows=tw, improve=imp, exchange=exc, tw_improve=twi))
    # a batch of shipment rows only launches K6f alone
    only = [0, 2, 3]
    _same(batched_trips([reqs[k] for k in only], device=DEV, time_windows=[tw[k] for k in only]),
          batched_trips([reqs[k] for k in only], device=None, time_windows=[tw[k] for k in only]))


def test_app_on_the_gpu_router_equals_the_cpu_router():
    """One shipment request through the app on the GPU graph provider (per-request path and the
    batcher's flush) equals ``optimize_route`` on the CPU CCH router.  Both routers customize the
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
    idx = rng.choice(g.num_nodes, 9, replace=False)
    body = {"source_point": {"lat": float(g.lat[idx[0]]), "lon": float(g.lon[idx[0]])},
            "destination_points": [{"lat": float(g.lat[j]), "lon": float(g.lon[j]), "payload": 1} for j in idx[1:]],
            "driver_details": {"vehicle_capacity": 3, "maximum_distance": 1e7}}
    for dl, pk in ((0, 6), (4, 2)):
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
        assert got["properties"]["shipments"] == {"pairs": 2, "max_load": 3.0}
        assert got["properties"]["time_windows"]["stops_with_windows"] == 2 and got["properties"]["summary"]["trips"] == 2
        assert got == json.loads(json.dumps(want)), batch


def test_main_port_relays_shipment_requests():
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
        body = _request(6, 21, pairs=False)
        body["destination_points"][4]["pickup_from"] = 1
        body["destination_points"][1].pop("payload")
        f0 = st.front.stats()
        a = post(st.port, body)
        b = post(st.app_server.port, body)
        f1 = st.front.stats()
        assert a[0] == 200 and a == b, (a[1][:300], b[1][:300])
        assert json.loads(a[1])["properties"]["shipments"]["pairs"] == 1
        assert f1["relayed"] - f0["relayed"] == 1 and f1["route_flushes"] == f0["route_flushes"], (f0, f1)
    finally:
        st.close()
