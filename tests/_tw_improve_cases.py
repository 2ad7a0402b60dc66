"""Instances for the tests of the window-aware local search (routing/tw_improve.py,
``_rt.tw_improve``, K6e): the named instances of tests/_tw_cases.py plus seeded additions (instances
on which the search drops a trip, and a large one whose float load walk rejects a move).  The
search runs on what the cheapest insertion built (:func:`_tw_cases.expected` /
:func:`built`); the reference's answer is computed once (:func:`expected`) and never changed.
"""
import functools

import numpy as np

from routest_amd.routing.exchange import UNBOUNDED
from routest_amd.routing.greedy import InfeasibleStops
from routest_amd.routing.timewindows import tw_trips
from routest_amd.routing.tw_improve import STAT_KEYS, tw_improve_trips

import _tw_cases
from _tw_cases import SPEED, _planar, make, random_instance


def cap_float_large_instance(ns, seed):
    """``_tw_cases.cap_float_instance`` with more stops: demands of 0.1 and cap 0.3, so a third stop
    fits a trip in fixed point (300 <= 300) but not in the greedy's own float sum."""
    _, d = _planar(ns, seed)
    return make(d, d / SPEED, demand=[0.0] + [0.1] * ns, cap=0.3, service={1: 5})


@functools.lru_cache(maxsize=None)
def named_instances():
    out = dict(_tw_cases.named_instances())
    out["drop_road_ns8"] = random_instance(8, 5002, road=True)
    out["drop_ns12"] = random_instance(12, 5001)
    out["drop_cap_ns20"] = random_instance(20, 5014, cap_frac=0.3)
    out["drop_ns36"] = random_instance(36, 5010)
    out["road_ns50"] = random_instance(50, 5021, road=True)
    out["cap_float_reject_ns40"] = cap_float_large_instance(40, 703)
    return out


def stops_of(name):
    return len(named_instances()[name]["d"]) - 1


SMALL = [n for n in named_instances() if stops_of(n) <= 32]
LARGE = [n for n in named_instances() if stops_of(n) > 32]


@functools.lru_cache(maxsize=None)
def built(name):
    """What the cheapest insertion answers: ``(trips, schedule, stats)`` or ``("infeasible", stops)``."""
    if name in _tw_cases.named_instances():
        return _tw_cases.expected(name)
    try:
        return tw_trips(**named_instances()[name])
    except InfeasibleStops as e:
        return ("infeasible", e.stops)


def search_args(case, trips):
    return (case["d"], case["t"], trips, case["demand"], case["cap"], case["max_dist"], case["open_q"],
            case["close_q"], case["sv_q"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's answer ``(trips, schedule, stats, applied moves)``; None for an instance the
    insertion reports infeasible."""
    b = built(name)
    if b[0] == "infeasible":
        return None
    applied = []
    trips, schedule, stats = tw_improve_trips(*search_args(named_instances()[name], b[0]), applied=applied)
    return trips, schedule, stats, tuple(applied)


def opened(case):
    """The case with every window opened (service times kept)."""
    n1 = len(case["d"])
    return dict(case, open_q=[0] * n1, close_q=[UNBOUNDED] * n1)


def expected_rows(name, nm):
    """What K6d then K6e must leave for the instance: visit, trip_of, ntrips, status, arrival, start
    and the search's stats [7] (a row the search does not touch keeps K6d's outputs and zeros)."""
    case = named_instances()[name]
    ans = expected(name)
    if ans is None:
        return _tw_cases.expected_rows(case, built(name), nm)[:6] + (np.zeros(7, dtype=np.int64),)
    return rows_of(ans, nm)


def rows_of(ans, nm):
    trips, schedule, st = ans[:3]
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
