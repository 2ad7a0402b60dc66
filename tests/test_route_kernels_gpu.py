"""K5 (batched haversine matrices) and K6 (batched greedy CVRP, wavefront per request) vs the CPU
reference of R21 on the SAME matrices: optimized_order / trips must be identical."""
import numpy as np
import pytest
import torch

from routest_amd.ops import _ext
from routest_amd.routing.batched import (batched_trips, batched_trips_cpu, batched_trips_device,
                                         pack_requests)
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.providers import haversine_matrix

pytestmark = pytest.mark.gpu


def _requests(n_req, max_stops, seed, infeasible_frac=0.05):
    rng = np.random.default_rng(seed)
    reqs = []
    for k in range(n_req):
        n = int(rng.integers(1, max_stops + 1)) + 1
        dests = [{"lat": float(rng.uniform(14.4, 14.7)), "lon": float(rng.uniform(120.95, 121.1)),
                  "payload": int(rng.integers(1, 5))} for _ in range(n)]
        cap = int(rng.integers(4, 16))
        if rng.random() < infeasible_frac:
            dests[int(rng.integers(0, n))]["payload"] = cap + 1
        reqs.append({"source_point": {"lat": 14.5836, "lon": 121.0409}, "destination_points": dests,
                     "driver_details": {"vehicle_capacity": cap,
                                        "maximum_distance": float(rng.uniform(30_000, 150_000))}})
    return reqs


def test_haversine_matrix_kernel():
    C = _ext.native()
    reqs = _requests(200, 12, 0)
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    D = C.route_haversine_matrix(torch.tensor(lat).cuda(), torch.tensor(lon).cuda(),
                                 torch.tensor(npts).cuda(), 1.3).cpu().numpy()
    for k in range(len(reqs)):
        n = npts[k]
        ref = haversine_matrix(lat[k, :n], lon[k, :n], 1.3)
        np.testing.assert_allclose(D[k, :n, :n], ref, rtol=1e-12, atol=1e-6)
        assert (D[k, n:, :] == 0).all()


@pytest.mark.parametrize("max_stops,n_req", [(10, 10_000), (63, 500), (200, 64), (1500, 4)])
def test_greedy_kernel_identical_to_cpu(max_stops, n_req):
    C = _ext.native()
    reqs = _requests(n_req, max_stops, max_stops)
    lat, lon, dem, npts, cap, maxd = pack_requests(reqs)
    dev = torch.device("cuda:0")
    D = C.route_haversine_matrix(torch.tensor(lat, device=dev), torch.tensor(lon, device=dev),
                                 torch.tensor(npts, device=dev), 1.3)
    gpu = batched_trips_device(lat, lon, dem, npts, cap, maxd, 1.3, dev)
    cpu = batched_trips_cpu(lat, lon, dem, npts, cap, maxd, 1.3, D=D.cpu().numpy())
    n_inf = 0
    for g, c in zip(gpu, cpu):
        if isinstance(c, InfeasibleStops):
            assert isinstance(g, InfeasibleStops)
            assert sorted(g.stops) == sorted(c.stops)
            n_inf += 1
        else:
            assert g == c
    assert n_inf < len(reqs)


# ---------------------------------------------------------------------------------------------
# Crafted instances.  Every comparison below is equality with the CPU reference on the SAME
# matrix (and, where the expected trips are written out, with those): no tolerance anywhere.
# An instance is (d, demand, cap, max_dist) as in tests/_greedy_cases.py.
# ---------------------------------------------------------------------------------------------
from _greedy_cases import association_instances, pack_matrix_instances  # noqa: E402
from routest_amd.routing.greedy import greedy_trips_reference_literal  # noqa: E402

BIG = 1e18


def _run_both(D, dem, npts, cap, maxd):
    """K6 and the CPU reference on the given matrices; asserts they agree exactly, infeasible stops
    in the same ORDER, and returns the CPU results."""
    assert (np.asarray(npts) <= D.shape[1]).all() and (np.asarray(npts) >= 0).all()
    z = np.zeros(D.shape[:2])
    gpu = batched_trips_device(z, z, dem, npts, cap, maxd, 1.3, "cuda:0", D=D)
    cpu = batched_trips_cpu(z, z, dem, npts, cap, maxd, 1.3, D=D)
    assert len(gpu) == len(cpu) == len(npts)
    for k, (g, c) in enumerate(zip(gpu, cpu)):
        if isinstance(c, InfeasibleStops):
            assert isinstance(g, InfeasibleStops) and g.stops == c.stops, k
        else:
            assert g == c, k
    return cpu


def _line(pos, dem, cap, maxd=BIG):
    """Points on a line at integer positions (pos[0] = depot): an integer matrix, exact sums."""
    p = np.asarray(pos, dtype=np.float64)
    return np.abs(p[:, None] - p[None]).tolist(), [0.0] + [float(q) for q in dem], float(cap), float(maxd)


def _random_instance(n_pts, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform([14.4, 120.95], [14.7, 121.1], size=(n_pts, 2))
    pts[0] = [14.55, 121.025]                                        # central depot: every stop is within reach
    d = haversine_matrix(pts[:, 0], pts[:, 1], 1.3)
    dem = [0.0] + rng.integers(1, 5, n_pts - 1).astype(float).tolist()
    return d.tolist(), dem, float(rng.integers(8, 16)), float(rng.uniform(60_000, 150_000))


def test_greedy_kernel_association_boundaries():
    """`di = d[cur][i] + d[i][0]; (tdist + di) <= MD` (route_kernels.hip): on max_dist values that
    separate it from `(tdist + d[cur][i]) + d[i][0]` K6 returns the reference loop's trips."""
    insts = association_instances()
    cpu = _run_both(*pack_matrix_instances(insts))
    for inst, c in zip(insts, cpu):
        assert c == greedy_trips_reference_literal(*inst)


@pytest.mark.parametrize("copies,others", [(2, 5), (3, 4), (70, 70)])
def test_repeated_coordinates(copies, others):
    """Several parcels for one address.  K5: `i != j` is the only zero the kernel writes by decree;
    identical points must still come out as exactly 0.0.  K6: the stable rank `(kj < key) || (kj ==
    key && j < i)` with equal keys — a rank shared by two stops would leave a slot of s_order
    unwritten.  The copies are interleaved by index with other stops and carry different demands,
    so their order shows in the trips."""
    C = _ext.native()
    rng = np.random.default_rng(copies)
    n = 1 + copies + others
    lat = rng.uniform(14.4, 14.7, n)
    lon = rng.uniform(120.95, 121.1, n)
    idx = np.arange(1, 2 * copies, 2)                                # copies at 1, 3, 5, ...: others in between
    assert idx[-1] <= n - 1
    lat[idx], lon[idx] = lat[idx[0]], lon[idx[0]]
    dem = np.zeros((1, n))
    dem[0, 1:] = rng.integers(1, 5, n - 1)
    npts = np.array([n], np.int32)
    dev = torch.device("cuda:0")
    D = C.route_haversine_matrix(torch.tensor(lat[None], device=dev), torch.tensor(lon[None], device=dev),
                                 torch.tensor(npts, device=dev), 1.3).cpu().numpy()
    sub = D[0][np.ix_(idx, idx)]
    assert (sub == 0.0).all() and not np.signbit(sub).any()
    assert (D[0][0, idx] == D[0][0, idx[0]]).all() and (D[0][idx, 0] == D[0][idx[0], 0]).all()
    cpu = _run_both(D, dem, npts, np.array([7.0]), np.array([200_000.0]))
    assert not isinstance(cpu[0], InfeasibleStops)
    assert sorted(i for t in cpu[0] for i in t[1:-1]) == list(range(1, n))


@pytest.mark.parametrize("nm", [64, 65, 1024, 1025])
def test_packed_width_at_the_tier_edges(nm):
    """launch_greedy_cvrp picks greedy_cvrp_kernel<64> for NM <= 64, <1024> for NM <= 1024, <4096>
    above: one request that fills the padded width exactly, on either side of both thresholds (the
    last stop's index is NMAX - 1 of the LDS arrays at 64 and 1024)."""
    inst = _random_instance(nm, nm)
    D, dem, npts, cap, maxd = pack_matrix_instances([inst])
    assert D.shape == (1, nm, nm) and npts[0] == nm
    cpu = _run_both(D, dem, npts, cap, maxd)
    assert not isinstance(cpu[0], InfeasibleStops) and len(cpu[0]) > 1


@pytest.mark.parametrize("nm", [9, 70])
@pytest.mark.parametrize("R", [1, 5, 7])
def test_mixed_request_sizes(nm, R):
    """npts = 1 (a depot only: `placed < ns` never holds, zero trips), 2 and NM in one batch, with R
    no multiple of 4: the last block has idle waves (`if (r >= R) return`)."""
    sizes = [1, 2, nm]
    batches = [[s] for s in sizes] if R == 1 else [[sizes[k % 3] for k in range(R)]]
    for b in batches:
        insts = [_random_instance(s, 100 * nm + 10 * R + k) for k, s in enumerate(b)]
        D, dem, npts, cap, maxd = pack_matrix_instances(insts)
        if D.shape[1] < nm:                                          # a batch of small requests keeps the width
            pad = nm - D.shape[1]
            D = np.pad(D, ((0, 0), (0, pad), (0, pad)))
            dem = np.pad(dem, ((0, 0), (0, pad)))
        assert D.shape == (len(b), nm, nm)
        cpu = _run_both(D, dem, npts, cap, maxd)
        for s, c in zip(b, cpu):
            if s == 1:
                assert c == []


def test_late_feasible_candidate():
    """The scan `for (base = pos; base < ns && found < 0; base += 64)`: a first 64-lane group in
    which nothing is feasible and a later group that holds the next stop; an acceptance by lane 63
    of a group (scan position 63) and by lane 0 of the second group (position 64)."""
    # stop 1 (demand 6) fills the van so far that the 69 stops behind it (5 each) do not fit; stop 71 (4) does
    late = _line(range(131), [6] + [5] * 69 + [4] + [5] * 59, cap=10)
    # trip 1 takes stops 1..63 (demand 1, cap 63); trip 2 starts with positions 0..62 visited, 63 open
    at63 = _line(range(71), [1] * 63 + [2] + [1] * 6, cap=63)
    at64 = _line(range(71), [1] * 64 + [2] + [1] * 5, cap=64)
    cpu = _run_both(*pack_matrix_instances([late, at63, at64]))
    assert cpu[0][0] == [0, 1, 71, 0]
    assert cpu[1][0] == [0] + list(range(1, 64)) + [0] and cpu[1][1][:2] == [0, 64]
    assert cpu[2][0] == [0] + list(range(1, 65)) + [0] and cpu[2][1][:2] == [0, 65]


def test_bounds_that_hold_with_equality():
    """`(load + dem[i]) <= C && (tdist + di) <= MD` are both `<=`: equality accepts, the next
    representable bound below rejects.  Integer matrix (3-4-5 triangle), so every sum is exact."""
    d = [[0.0, 3.0, 5.0], [3.0, 0.0, 4.0], [5.0, 4.0, 0.0]]
    dem = [0.0, 4.0, 6.0]
    below = lambda v: float(np.nextafter(v, 0.0))  # noqa: E731
    insts = [(d, dem, 10.0, 12.0),                 # 4 + 6 == cap and 3 + (4 + 5) == max_dist
             (d, dem, 10.0, below(12.0)),
             (d, dem, below(10.0), 12.0),
             (d, dem, 10.0, 10.0),                 # the lone second trip 0 + (5 + 5) == max_dist
             (d, dem, 10.0, below(10.0))]          # ... and just below: stop 2 is infeasible on its own
    cpu = _run_both(*pack_matrix_instances(insts))
    assert cpu[0] == [[0, 1, 2, 0]]
    assert cpu[1] == cpu[2] == cpu[3] == [[0, 1, 0], [0, 2, 0]]
    assert isinstance(cpu[4], InfeasibleStops) and cpu[4].stops == [1]


def test_partly_infeasible_request_reports_stops_in_cpu_order():
    """`if (accepted == 0) { st = 1; break; }` after feasible trips: the stops left over are
    reported in depot-distance order with ties by index, as the CPU does (the unpacking sorts the
    unplaced stops by D[0][i])."""
    # stops 1..3 feasible; 4 (far), 5 and 6 (one address, nearer than 4) exceed the capacity
    a = _line([0, 1, 2, 3, 9, 7, 7], [1, 1, 1, 99, 99, 99], cap=2)
    # infeasible by distance, not load: the round trip to stops 3 and 4 alone exceeds max_dist
    b = _line([0, 1, 2, 40, 30], [1, 1, 1, 1], cap=10, maxd=50)
    cpu = _run_both(*pack_matrix_instances([a, b]))
    assert isinstance(cpu[0], InfeasibleStops) and cpu[0].stops == [4, 5, 3]
    assert isinstance(cpu[1], InfeasibleStops) and cpu[1].stops == [3, 2]


def test_batched_trips_api_device():
    reqs = _requests(300, 8, 5)
    g = batched_trips(reqs, device="cuda:0")
    c = batched_trips(reqs)
    agree = sum(1 for a, b in zip(g, c) if (isinstance(a, InfeasibleStops) and isinstance(b, InfeasibleStops)) or a == b)
    # numpy vs device libm may differ in the last ulp; decisions agree on (essentially) all requests
    assert agree >= len(reqs) - 1
