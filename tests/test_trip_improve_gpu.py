"""K6b (``_C.route_improve_trips``, csrc/route_improve.hip) against the Python reference
(routing/improve.py) on K6's real outputs: ``visit``, ``trip_of`` and the four statistics arrays
are compared with ``torch.equal``.  Instances: tests/_improve_cases.py."""
import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import batched_trips
from routest_amd.routing.greedy import InfeasibleStops

from _greedy_cases import pack_matrix_instances
from _improve_cases import expected, named_instances, random_instance

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

DEV = "cuda:0"


def _run(names, flags=None, extra=()):
    """K6 then K6b on the named instances (+ ``extra`` raw instances appended, flag as given).
    Returns K6's own (visit, trip_of, status), K6b's visit and statistics, all on the host."""
    C = _ext.native(required=True)
    insts = [named_instances()[n] for n in names] + [e[0] for e in extra]
    D, dem, npts, cap, maxd = pack_matrix_instances(insts)
    for k, e in enumerate(extra):
        if e[1] is not None:            # a row that claims fewer points than it was packed with
            npts[len(names) + k] = e[1]
    R = len(insts)
    f = np.ones(R, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(DEV)  # noqa: E731
    Dt, nt, mt = t(D), t(npts, torch.int32), t(maxd)
    visit, trip_of, ntrips, status = C.route_greedy_cvrp(Dt, nt, t(dem), t(cap), mt)
    v0, t0 = visit.clone(), trip_of.clone()
    moves, changed, before, after = C.route_improve_trips(Dt, nt, mt, visit, trip_of, status,
                                                          t(f, torch.uint8))
    torch.cuda.synchronize()
    assert torch.equal(trip_of, t0), "stops never change trips"
    return dict(v0=v0.cpu(), visit=visit.cpu(), trip_of=trip_of.cpu(), status=status.cpu(),
                moves=moves.cpu(), changed=changed.cpu(), before=before.cpu(), after=after.cpu(),
                nm=D.shape[1], flags=f)


def _expected_rows(names, nm, flags):
    """The reference's visit rows and statistics for the named instances."""
    R = len(names)
    visit = torch.full((R, nm), -1, dtype=torch.int32)
    trip_of = torch.full((R, nm), -1, dtype=torch.int32)
    st = torch.zeros((4, R), dtype=torch.int64)
    for r, name in enumerate(names):
        g, new, s = expected(name)
        trips = new if flags[r] else g
        flat = [v for tr in trips for v in tr[1:-1]]
        visit[r, :len(flat)] = torch.tensor(flat, dtype=torch.int32)
        trip_of[r, :len(flat)] = torch.tensor([i for i, tr in enumerate(trips) for _ in tr[1:-1]],
                                              dtype=torch.int32)
        if flags[r]:
            st[:, r] = torch.tensor([s["moves"], s["trips_changed"], s["len_before_q"], s["len_after_q"]])
    return visit, trip_of, st


def _check(names, flags=None):
    out = _run(names, flags)
    R = len(names)
    flags = out["flags"]
    visit, trip_of, st = _expected_rows(names, out["nm"], flags)
    assert torch.equal(out["status"], torch.zeros(R, dtype=torch.int32))
    assert torch.equal(out["trip_of"], trip_of)
    assert torch.equal(out["visit"], visit)
    assert torch.equal(out["moves"], st[0].to(torch.int32))
    assert torch.equal(out["changed"], st[1].to(torch.int32))
    assert torch.equal(out["before"], st[2])
    assert torch.equal(out["after"], st[3])
    return out


def _small_names():
    return [n for n, inst in named_instances().items() if len(inst[0]) <= 33]


def test_small_tier_every_instance():
    """NM = 33: every instance of at most 32 stops (association, grid ties, inf / NaN / negative
    entries, the revert pair, k = 1..32), a wavefront each."""
    names = _small_names()
    assert "random_k32" in names and "revert_at_greedy_total" in names and "special_3" in names
    out = _check(names)
    assert out["nm"] == 33
    r = names.index("revert_at_greedy_total")
    assert int(out["moves"][r]) == 0 and torch.equal(out["visit"][r], out["v0"][r])
    assert int(out["moves"][names.index("revert_one_higher")]) == 1


@pytest.mark.parametrize("names,nm", [
    (["random_k63", "random_k7", "random_k33", "grid_k30", "trips_k20_cap6"], 64),          # R = 5
    (["trips_k64_cap33", "random_k64", "random_k32", "random_k33", "grid_k40_cap25",
      "trips_k40_maxd", "random_k2", "special_3", "random_k1"], 65),                        # R = 9
    (["random_k33"], 34),                                                                   # R = 1
    (["random_k32"], 33),
    (["random_k129", "random_k128", "trips_k65_cap33", "random_k4", "grid_k12"], 130),
])
def test_large_tier_and_mixed_rows(names, nm):
    """Rows of both tiers in one batch; trips of 32 and 33 stops in one request; k = 128 (the
    largest LDS carve) and k = 129 (left as the greedy built it)."""
    out = _check(names)
    assert out["nm"] == nm
    if "random_k129" in names:
        r = names.index("random_k129")
        assert int(out["moves"][r]) == 0 and int(out["before"][r]) == int(out["after"][r]) > 0
        assert torch.equal(out["visit"][r], out["v0"][r])
        assert int(out["moves"][names.index("random_k128")]) > 0


def test_flags_status_and_empty_rows():
    """One batch mixes flag 0 and flag 1 rows, a status != 0 row, an npts == 1 row and an
    npts == 0 row: untouched rows are bit-equal to K6's output and their statistics are 0."""
    names = ["random_k7", "random_k33", "grid_k12", "random_k63", "trips_k20_cap6"]
    flags = [1, 0, 0, 1, 1, 1, 1, 1]
    d, dem, cap, md = random_instance(9, 900)
    dem = list(dem)
    dem[4] = 5.0                                             # over capacity: K6 reports status 1
    extra = [((d, dem, 3.0, md), None), (random_instance(5, 901), 1), (random_instance(5, 902), 0)]
    out = _run(names, flags, extra)
    assert out["status"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    visit, trip_of, st = _expected_rows(names, out["nm"], flags)
    n = len(names)
    assert torch.equal(out["visit"][:n], visit) and torch.equal(out["trip_of"][:n], trip_of)
    for r in (1, 2, 5, 6, 7):
        assert torch.equal(out["visit"][r], out["v0"][r])
    for key, ref in (("moves", st[0]), ("changed", st[1]), ("before", st[2]), ("after", st[3])):
        assert out[key][:n].to(torch.int64).tolist() == ref.tolist()
        assert out[key][n:].tolist() == [0, 0, 0]
    assert int(out["moves"][0]) > 0 and int(out["moves"][3]) > 0


def _zigzag_request(n, seed, improve=None, cap=None):
    rng = np.random.default_rng(seed)
    dests = [{"lat": 14.58 + (0.002 + 0.003 * i) * (1 if i % 2 else -1) + float(rng.uniform(0, 1e-3)),
              "lon": 121.04 + float(rng.uniform(-0.02, 0.02)), "payload": 1} for i in range(n)]
    r = {"source_point": {"lat": 14.58, "lon": 121.04}, "destination_points": dests,
         "driver_details": {"vehicle_capacity": cap or 10_000, "maximum_distance": 5e6}}
    if improve is not None:
        r["improve"] = improve
    return r


def test_batched_trips_device_equals_cpu():
    """``batched_trips(..., device="cuda")`` equals ``batched_trips(..., device=None)`` with
    per-request flags, haversine matrices and given matrices."""
    reqs = [_zigzag_request(n, n, cap=c) for n, c in
            ((2, None), (5, None), (12, 5), (33, None), (40, 32), (70, None), (9, None))]
    reqs[2]["destination_points"][3]["payload"] = 6          # infeasible: over capacity
    flags = [True, True, True, False, True, True, False]
    # K5's matrices, so both sides search the same float64 entries
    from routest_amd.routing.batched import pack_requests
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    C = _ext.native(required=True)
    D = C.route_haversine_matrix(torch.tensor(lat).to(DEV), torch.tensor(lon).to(DEV),
                                 torch.tensor(npts).to(DEV), 1.3).cpu().numpy()
    gpu, gst = batched_trips(reqs, device=DEV, D=D, improve=flags)
    cpu, cst = batched_trips(reqs, device=None, D=D, improve=flags)
    assert isinstance(cpu[2], InfeasibleStops) and isinstance(gpu[2], InfeasibleStops)
    assert sorted(gpu[2].stops) == sorted(cpu[2].stops)
    assert [g for i, g in enumerate(gpu) if i != 2] == [c for i, c in enumerate(cpu) if i != 2]
    assert gst == cst
    assert gst[3] is None and gst[6] is None and gst[2] is None and gst[5]["moves"] > 0
    plain = batched_trips(reqs, device=DEV, D=D)
    assert plain[3] == gpu[3] and plain[6] == gpu[6] and plain[5] != gpu[5]
    # without a given D the device path computes the same K5 matrices itself
    g2, s2 = batched_trips(reqs, device=DEV, improve=flags)
    assert g2[5] == gpu[5] and s2 == gst


# ---------------------------------------------------------------------------------------------
# Native front end vs the Python app: "improve": true answered byte-identically, the way
# tests/test_frontend_gpu.py compares plain requests.
# ---------------------------------------------------------------------------------------------
def _http(port, path, body, conn=None):
    import http.client
    import json
    c = conn or http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, r.read()


def _stack(provider, timeout_us=300):
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.serve.eta_service import EtaService, default_model
    from routest_amd.serve.frontend import ServingStack
    model = default_model(steps=30)
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="1", route_gpu_min_stops=1,
                      warm_scorer=False)
    sv = build_services(s, eta=EtaService(model, devices=[0]), provider=provider, store=None)
    return ServingStack(sv, create_app(sv), model, [0], threads=4, timeout_us=timeout_us), sv


def _improve_payloads(n, lat, lon, seed):
    """Requests of 1..40 stops drawn from the given points; two in three ask for improve (JSON
    true), some with values that must not count, some over capacity, some with several trips."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.choice([1, 2, 3, 5, 8, 12, 20, 34, 40]))
        idx = rng.choice(len(lat), k + 1, replace=False)
        p = {"source_point": {"lat": float(lat[idx[0]]), "lon": float(lon[idx[0]])},
             "destination_points": [{"lat": float(lat[j]), "lon": float(lon[j]), "payload": 1} for j in idx[1:]],
             "driver_details": {"driver_name": f"drv{i}", "vehicle_type": ["car", "truck", "bike"][i % 3],
                                "vehicle_capacity": [99, 7, 36][i % 3], "maximum_distance": 1e7}}
        if i % 3 != 2:
            p["improve"] = True
        elif i % 2:
            p["improve"] = ["yes", 1, False][i % 3]
        if i % 11 == 5:
            p["driver_details"]["vehicle_capacity"] = 0                 # infeasible stops
        out.append(p)
    return out


def test_native_haversine_improve_byte_identical():
    from routest_amd.routing.providers import HaversineProvider
    st, sv = _stack(HaversineProvider())
    try:
        assert st.front.routes, "native routes not enabled"
        rng = np.random.default_rng(7)
        lat, lon = 14.55 + rng.normal(0, 0.04, 500), 121.02 + rng.normal(0, 0.04, 500)
        pays = _improve_payloads(45, lat, lon, seed=1)
        improved = 0
        for k, p in enumerate(pays):
            path = ("/api/optimize_route", "/route", "/api/request_route")[k % 3]
            a = _http(st.port, path, p)
            b = _http(st.app_server.port, path, p)
            assert a[0] == b[0] and a[1] == b[1], (path, p, a[1][:300], b[1][:300])
            improved += b'"improvement":{"method":"2opt+oropt"' in a[1]
        assert improved >= 15
        assert st.front.stats()["route_service_fallbacks"] == 0
    finally:
        st.close()


def test_native_graph_cch_improve_mixed_flush_two_contexts():
    """Road-graph provider over the CCH: asking and non-asking requests under two routing contexts
    arrive together and share flushes; every answer equals the app's."""
    import threading
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import default_model
    g = synth_road_graph(6000, seed=2)
    prov = GraphProvider(g, None, device=torch.device("cuda", 0), eta_model=default_model(hidden=64, steps=50))
    st, sv = _stack(prov, timeout_us=20_000)
    try:
        assert st.front.routes and st.front.routes[0]["provider"] == "graph"
        ctxs = ({"weather": "Sunny", "traffic": "Low", "pickup_time": "2025-08-26T03:00:00"},
                {"weather": "Stormy", "traffic": "Jam", "pickup_time": "2025-08-29T18:00:00"})
        pays = [dict(p, context=ctxs[i % 2]) for i, p in enumerate(_improve_payloads(48, g.lat, g.lon, seed=3))]
        want = [_http(st.app_server.port, "/api/optimize_route", p) for p in pays]
        for c in ctxs:                                   # both contexts customized before the burst
            _http(st.port, "/api/optimize_route", dict(pays[0], context=c))
        f0 = st.front.stats()["route_flushes"]
        got = [None] * len(pays)

        def worker(k):
            import http.client
            c = http.client.HTTPConnection("127.0.0.1", st.port, timeout=60)
            for i in range(k, len(pays), 16):
                got[i] = _http(st.port, "/api/optimize_route", pays[i], conn=c)
        th = [threading.Thread(target=worker, args=(k,)) for k in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for p, a, b in zip(pays, got, want):
            assert a[0] == b[0] and a[1] == b[1], (p, a[1][:300], b[1][:300])
        stats = st.front.stats()
        assert stats["route_flushes"] - f0 < len(pays)               # requests shared flushes
        assert stats["route_service_fallbacks"] == 0, stats
        assert sum(b'"improvement":' in a[1] for a in got) >= 20
        assert sum(b'"improvement":' not in a[1] and a[0] == 200 for a in got) >= 8
    finally:
        st.close()
