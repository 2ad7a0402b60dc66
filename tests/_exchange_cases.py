"""Instances for the trip-exchange tests (routing/exchange.py, ``_rt.exchange_trips``, K6c).

An instance is ``(d, demand, cap, max_dist, trips, move_cap)``: the matrix over [depot] + stops, the
demand per point, the two limits, the trips the search starts from (the greedy's after the
intra-trip improvement, or hand-made) and the move cap (``None``: the default).  Shared by the CPU
test of the reference against the host C++ and the GPU test of the kernel against the reference;
the reference's answer for an instance is computed once (:func:`expected`) and never changed.
"""
import functools

import numpy as np

from routest_amd.routing.exchange import exchange_trips
from routest_amd.routing.greedy import greedy_trips
from routest_amd.routing.improve import improve_trips

BIGD = 9e12


def _planar(ns, seed, asym=0.05):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 8_000.0, (ns + 1, 2))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    d *= 1.0 + asym * rng.uniform(-1.0, 1.0, d.shape)
    np.fill_diagonal(d, 0.0)
    return rng, d


def _start(d, dem, cap, md):
    """What the exchange sees in the pipeline: the greedy's trips after the intra-trip pass."""
    g = greedy_trips(np.asarray(d).tolist(), dem, cap, md)
    return improve_trips(np.asarray(d, dtype=np.float64), g, md)[0]


def random_instance(ns, seed, move_cap=None):
    """Random planar points (+-5 % asymmetric), demands 1..3, a capacity of 40 % of the total demand
    (3 trips, the last with room to spare); up to 3 stops: every stop alone."""
    rng, d = _planar(ns, seed)
    if ns <= 3:
        dem, cap = [0.0] + [2.0] * ns, 3.0
    else:
        dem = [0.0] + [float(v) for v in rng.integers(1, 4, ns)]
        cap = float(max(3, int(np.ceil(sum(dem) / 2.5))))
    trips = _start(d, dem, cap, BIGD)
    assert len(trips) >= min(3, ns)
    return d.tolist(), dem, cap, BIGD, trips, move_cap


def singletons_instance(ns, seed, cap):
    """Hand-made trips of one stop each.  cap = one demand: only swaps are admissible; cap
    unbounded: relocates merge the trips until one is left (an emptied trip is never a target)."""
    _, d = _planar(ns, seed)
    return d.tolist(), [0.0] + [1.0] * ns, float(cap), BIGD, [[0, s, 0] for s in range(1, ns + 1)], None


def grid_instance(ns, seed, cap, max_dist=BIGD):
    """Lattice coordinates with Manhattan distances in whole metres: many moves tie exactly, so the
    (type, A, i, B, j) rule decides, and the limits are met with equality."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 5, (ns + 1, 2)).astype(np.float64) * 100.0
    d = np.abs(xy[:, None] - xy[None]).sum(-1)
    dem = [0.0] + [1.0] * ns
    return d.tolist(), dem, float(cap), float(max_dist), _start(d, dem, float(cap), float(max_dist)), None


def asymmetric_instance(ns, seed):
    """No geometry at all: independent uniform entries, d[a][b] unrelated to d[b][a]."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(100.0, 5_000.0, (ns + 1, ns + 1))
    np.fill_diagonal(d, 0.0)
    dem = [0.0] + [1.0] * ns
    return d.tolist(), dem, 4.0, BIGD, _start(d, dem, 4.0, BIGD), None


def special_instance(seed):
    """inf, NaN and a negative entry between stops (quantized to BIG), hand-made trips crossing them."""
    _, d = _planar(9, seed)
    d[2, 5] = np.inf
    d[3, 4] = np.nan
    d[6, 1] = -3.0
    d[7, 8] = np.inf
    trips = [[0, 2, 5, 1, 0], [0, 3, 4, 6, 0], [0, 7, 8, 9, 0]]
    return d.tolist(), [0.0] + [1.0] * 9, 4.0, BIGD, trips, None


def nonmetric_instance():
    """Taking stop 2 out of [0,1,2,3,0] lengthens that trip (d[1][3] is huge) past the limit, while
    putting it between 4 and 5 shortens the other by more: the gain is positive and only the
    source-trip test keeps the move out."""
    d = np.full((6, 6), 1000.0)
    np.fill_diagonal(d, 0.0)
    d[1, 2] = d[2, 3] = 100.0
    d[1, 3] = 5000.0
    d[4, 5] = 9000.0
    d[4, 2] = d[2, 5] = 100.0
    return d.tolist(), [0.0] + [1.0] * 5, 9.0, 6500.0, [[0, 1, 2, 3, 0], [0, 4, 5, 0]], None


def source_only_instance(max_dist):
    """The same shape with every other move shut out (50 km between {1, 3} and {4, 5}): the one
    candidate with a positive gain (7.5 m) takes stop 2 out of [0,1,2,3,0], which then measures
    3500 m.  max_dist 3000: only the source-trip test forbids it, so nothing moves; max_dist 3500:
    the source trip meets the limit with equality and the move is taken."""
    d = np.full((6, 6), 1000.0)
    np.fill_diagonal(d, 0.0)
    d[1, 2] = d[2, 3] = 100.0
    d[1, 3] = 1500.0
    d[4, 5] = 9000.0
    d[4, 2] = d[2, 5] = 100.0
    for x in (1, 3):
        for y in (4, 5):
            d[x, y] = d[y, x] = 50_000.0
    return d.tolist(), [0.0] + [1.0] * 5, 9.0, float(max_dist), [[0, 1, 2, 3, 0], [0, 4, 5, 0]], None


def swap_equal_instance(mirrored):
    """Stops on a line, Manhattan metres, both trips full (cap 2): only swaps.  The best swap (by
    the tie rule) leaves one trip at 600 m and the other at 1000 m = max_dist exactly: the second
    trip, or with the trips in the other order the first."""
    x = np.array([0.0, 100.0, -300.0, -100.0, 500.0])
    d = np.abs(x[:, None] - x[None])
    trips = [[0, 3, 4, 0], [0, 1, 2, 0]] if mirrored else [[0, 1, 2, 0], [0, 3, 4, 0]]
    return d.tolist(), [0.0] + [1.0] * 4, 2.0, 1000.0, trips, None


def emptied_trip_instance():
    """Stop 1 leaves its own trip for [0,2,3,0] (2 -> 1 -> 3 is 2 m against 1000 m).  Stops 4 and 5
    sit in one trip across an inf edge and are 50 km from the other stops, so the only place either
    could go is the trip stop 1 left empty, which must never be a target: one move, then nothing."""
    d = np.full((6, 6), 1000.0)
    np.fill_diagonal(d, 0.0)
    d[0, 1:] = d[1:, 0] = 10.0
    d[2, 1] = d[1, 3] = 1.0
    d[4, 5] = np.inf
    for x in (1, 2, 3):
        for y in (4, 5):
            d[x, y] = d[y, x] = 50_000.0
    return d.tolist(), [0.0] + [1.0] * 5, BIGD, 20_000.0, [[0, 1, 0], [0, 2, 3, 0], [0, 4, 5, 0]], None


def cap_boundary_instance(seed):
    """Demands of 1.5 and cap 4.5: a third stop brings a trip's load to cap_q exactly."""
    _, d = _planar(8, seed)
    trips = [[0, 1, 2, 0], [0, 3, 4, 0], [0, 5, 6, 0], [0, 7, 8, 0]]
    return d.tolist(), [0.0] + [1.5] * 8, 4.5, BIGD, trips, None


def cap_float_instance(seed):
    """Demands of 0.1 and cap 0.3: three stops are 300 <= 300 in fixed point, but the greedy's own
    float sum 0.1 + 0.1 + 0.1 exceeds 0.3, so the first relocate is undone."""
    _, d = _planar(6, seed)
    trips = [[0, 1, 2, 0], [0, 3, 4, 0], [0, 5, 6, 0]]
    return d.tolist(), [0.0] + [0.1] * 6, 0.3, BIGD, trips, None


def bad_demand_instance(seed, value):
    d, dem, cap, md, trips, mc = random_instance(10, seed)
    dem = list(dem)
    dem[4] = value
    return d, dem, cap, md, trips, mc


@functools.lru_cache(maxsize=None)
def reject_instance():
    """Found by search: every entry is whole millimetres + 0.0004 m, so q rounds the fraction away
    and ``Lq + ins <= max_q`` holds where the float64 walk exceeds ``max_dist``.  The limit sits on a
    trip that a later move builds, so earlier moves are kept and that one is undone."""
    for seed in range(2000):
        rng = np.random.default_rng(50_000 + seed)
        ns = 7
        xy = rng.uniform(0.0, 3_000.0, (ns + 1, 2))
        d = np.rint(np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1)) * 1000.0) / 1000.0 + 0.0004
        np.fill_diagonal(d, 0.0)
        dem = [0.0] + [1.0] * ns
        trips = [[0, 1, 2, 0], [0, 3, 4, 0], [0, 5, 6, 7, 0]]
        free, _ = exchange_trips(d, trips, dem, 5.0, BIGD)
        for t in free:
            md = round(sum(np.rint(d[t[p], t[p + 1]] * 1000.0) for p in range(len(t) - 1))) / 1000.0
            _, st = exchange_trips(d, trips, dem, 5.0, md)
            if st["rejected"] == 1 and st["moves"] >= 1:
                return d.tolist(), dem, 5.0, md, trips, None
    raise AssertionError("no reject instance found")


@functools.lru_cache(maxsize=None)
def named_instances():
    out = {}
    for ns in (2, 3, 10, 31, 32, 33, 64, 127, 128):
        out[f"random_ns{ns}"] = random_instance(ns, 900 + ns)
    out["skipped_ns129"] = random_instance(129, 1029)
    out["singletons_swaps_only"] = singletons_instance(12, 301, cap=1.0)
    d, dem, cap, md, _, _ = singletons_instance(12, 304, cap=2.0)
    out["pairs_swaps_only"] = (d, dem, cap, md, [[0, s, s + 1, 0] for s in range(1, 12, 2)], None)
    out["singletons_merge"] = singletons_instance(9, 302, cap=BIGD)
    out["singletons_merge_k40"] = singletons_instance(40, 303, cap=BIGD)
    out["grid_ties"] = grid_instance(14, 401, cap=4)
    out["grid_ties_k40"] = grid_instance(40, 402, cap=9)
    out["grid_maxd_equal"] = grid_instance(14, 403, cap=BIGD, max_dist=1600.0)
    out["asymmetric"] = asymmetric_instance(12, 501)
    out["asymmetric_k36"] = asymmetric_instance(36, 502)
    out["special_big_edges"] = special_instance(601)
    out["nonmetric_source_grows"] = nonmetric_instance()
    out["source_check_forbids"] = source_only_instance(3000.0)
    out["source_check_equal"] = source_only_instance(3500.0)
    out["swap_second_trip_equal"] = swap_equal_instance(False)
    out["swap_first_trip_equal"] = swap_equal_instance(True)
    out["emptied_trip_no_target"] = emptied_trip_instance()
    out["cap_boundary"] = cap_boundary_instance(701)
    out["cap_float_reject"] = cap_float_instance(702)
    out["demand_negative"] = bad_demand_instance(801, -1.0)
    out["demand_nan"] = bad_demand_instance(802, float("nan"))
    d, dem, cap, md, trips, _ = singletons_instance(9, 302, cap=BIGD)
    out["move_cap_1"] = (d, dem, cap, md, trips, 1)
    out["move_cap_2"] = (d, dem, cap, md, trips, 2)
    d, dem, cap, md, trips, _ = random_instance(40, 940)
    out["move_cap_2_k40"] = (d, dem, cap, md, trips, 2)
    out["reject_float_walk"] = reject_instance()
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's answer: (trips, stats)."""
    d, dem, cap, md, trips, mc = named_instances()[name]
    return exchange_trips(np.asarray(d, dtype=np.float64), trips, dem, cap, md, mc)


def pack_k6(trips, nm):
    """Trips as K6 writes them: visit / trip_of rows of width ``nm`` (-1 padded) and the count."""
    visit = np.full(nm, -1, dtype=np.int32)
    trip_of = np.full(nm, -1, dtype=np.int32)
    p = 0
    for t, trip in enumerate(trips):
        for s in trip[1:-1]:
            visit[p] = s
            trip_of[p] = t
            p += 1
    return visit, trip_of, len(trips)


def unpack_k6(visit, trip_of, ntrips):
    trips = [[0] for _ in range(int(ntrips))]
    for v, t in zip(visit, trip_of):
        if v < 0:
            break
        trips[int(t)].append(int(v))
    return [t + [0] for t in trips]
