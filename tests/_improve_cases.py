"""Instances for the trip-improvement tests (routing/improve.py, ``_rt.improve_trips``, K6b).

An instance is ``(d, demand, cap, max_dist)`` as in ``tests/_greedy_cases.py``.  Shared by the CPU
test of the reference against the host C++ and the GPU test of the kernel against the reference;
the reference's answer for an instance is computed once (:func:`expected`) and never changed.
"""
import functools

import numpy as np

from routest_amd.routing.greedy import InfeasibleStops, greedy_trips
from routest_amd.routing.improve import improve_trips, walk_feasible

from _greedy_cases import association_instances

BIGD = 9e12


def random_instance(k, seed, cap=BIGD, max_dist=BIGD):
    """Random planar points, distances made +-5 % asymmetric, unit demands."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 20_000.0, (k + 1, 2))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    d *= 1.0 + 0.05 * rng.uniform(-1.0, 1.0, d.shape)
    np.fill_diagonal(d, 0.0)
    return d.tolist(), [0.0] + [1.0] * k, float(cap), float(max_dist)


def grid_instance(k, seed, cap=BIGD):
    """Lattice coordinates with Manhattan distances in whole metres: many moves tie exactly, so
    the (type, i, j) rule decides."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 6, (k + 1, 2)).astype(np.float64) * 100.0
    d = np.abs(xy[:, None] - xy[None]).sum(-1)
    return d.tolist(), [0.0] + [1.0] * k, float(cap), BIGD


def special_instances():
    """inf, NaN and a negative entry between two stops (quantized to BIG), one each and together."""
    out = []
    for which in (("inf",), ("nan",), ("neg",), ("inf", "nan", "neg")):
        d, dem, cap, md = random_instance(8, 700 + len(out))
        d = np.asarray(d)
        if "inf" in which:
            d[2, 5] = np.inf
        if "nan" in which:
            d[3, 4] = np.nan
        if "neg" in which:
            d[6, 1] = -3.0
        out.append((d.tolist(), dem, cap, md))
    return out


def _walk(d, t):
    s = 0.0
    for p in range(len(t) - 2):
        s += d[t[p]][t[p + 1]]
    return s + d[t[-2]][0]


@functools.lru_cache(maxsize=None)
def revert_instance():
    """Found by search: entries carry sub-millimetre fractions, so the improved order is shorter in
    q but LONGER in f64.  Returns (d, demand, cap, greedy trip, improved trip, f64 total of the
    greedy trip, f64 total of the improved trip)."""
    rng = np.random.default_rng(12345)
    for _ in range(200_000):
        k = int(rng.integers(3, 5))
        mm = 1000.0 + rng.integers(0, 3, (k + 1, k + 1)) + rng.uniform(-0.49, 0.49, (k + 1, k + 1))
        d = mm / 1000.0
        np.fill_diagonal(d, 0.0)
        dl = d.tolist()
        dem = [0.0] + [1.0] * k
        g = greedy_trips(dl, dem, BIGD, BIGD)
        if len(g) != 1:
            continue
        wg = _walk(dl, g[0])
        try:
            if greedy_trips(dl, dem, BIGD, wg) != g:
                continue
        except InfeasibleStops:
            continue
        new, st = improve_trips(d, g, BIGD)
        if st["moves"] and _walk(dl, new[0]) > wg:
            return dl, dem, BIGD, g[0], new[0], wg, _walk(dl, new[0])
    raise AssertionError("no revert instance found")


@functools.lru_cache(maxsize=None)
def named_instances():
    out = {}
    for k in (1, 2, 3, 4, 7, 32, 33, 63, 64, 128, 129):
        out[f"random_k{k}"] = random_instance(k, k)
    out["trips_k20_cap6"] = random_instance(20, 101, cap=6)
    out["trips_k64_cap33"] = random_instance(64, 102, cap=33)      # trips of 33 and 31 stops
    out["trips_k65_cap33"] = random_instance(65, 103, cap=33)      # trips of 33 and 32 stops
    out["trips_k40_maxd"] = random_instance(40, 104, max_dist=60_000.0)
    for i, inst in enumerate(association_instances()):
        out[f"association_{i}"] = inst
    out["grid_k12"] = grid_instance(12, 201)
    out["grid_k30"] = grid_instance(30, 202)
    out["grid_k40_cap25"] = grid_instance(40, 203, cap=25)
    for i, inst in enumerate(special_instances()):
        out[f"special_{i}"] = inst
    d, dem, cap, g, new, wg, wn = revert_instance()
    out["revert_at_greedy_total"] = (d, dem, cap, wg)
    out["revert_one_higher"] = (d, dem, cap, wn)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's answer: (greedy trips, improved trips, stats)."""
    d, dem, cap, md = named_instances()[name]
    g = greedy_trips(d, dem, cap, md)
    new, st = improve_trips(np.asarray(d, dtype=np.float64), g, md)
    return g, new, st


def feasible_after(name):
    d, _, _, md = named_instances()[name]
    return all(walk_feasible(d, t, md) for t in expected(name)[1] if len(t) > 2)
