"""Delivery time windows and service times: cheapest-insertion trip construction — CPU reference.

A multi-stop request whose destinations carry ``"time_window": [open, close]`` (seconds after the
trip leaves the depot; the stop's service must *start* inside it, early arrivals wait) or
``"service": s`` (seconds spent at the stop) is planned by :func:`tw_trips` instead of the greedy
(:mod:`routing.greedy`): a sequential cheapest-insertion construction in the spirit of Solomon's I1
with an O(1) exact time test per candidate.  Every trip's clock starts at 0 at the depot and the
depot never closes.  The definition is schedule-independent, so this reference, the host C++
(``rtr::tw_trips``, ``csrc/runtime/route_core.h``) and the GPU kernel (K6d, ``csrc/route_tw.hip``)
return the same trips, schedule and statistics, compared with ``==``.

Fixed point as in :mod:`routing.improve` / :mod:`routing.exchange`: ``q = quantize_matrix(D)``
(millimetres), ``qt = quantize_matrix(T)`` (milliseconds of the seconds matrix), ``qd``, ``cap_q``,
``max_q`` as in ``exchange.py`` (a NaN / negative ``cap`` or ``max_dist`` gives ``-1``: no insertion
is admissible).  An entry of ``q`` or ``qt`` that is ``>= 2**31 - 1`` is *unusable* and treated as
``BIG`` (a leg is never 2,147 km or 24.8 days long; both matrices of a 128-stop request then fit
the GPU's LDS as int32).  ``open_q[s]``, ``close_q[s]``, ``sv_q[s]``: ``quantize`` of the request's
fields, ``0 <= open_q <= close_q <= 2 * 10**9`` and ``0 <= sv_q <= 2 * 10**9``; a stop without a window has
``open_q = 0`` and ``close_q = UNBOUNDED = 2**62``, one without ``service`` has ``sv_q = 0``.  Sums
are int64.  At most 128 stops.

Schedule of a trip ``0, s1..sk, 0`` (``dep_0 = 0``)::

    arr_i = dep_{i-1} + qt(s_{i-1}, s_i);  start_i = max(arr_i, open_i);  dep_i = start_i + sv_i

The trip is time-feasible iff every ``start_i <= close_i`` and no used entry (the leg back to the
depot included) is unusable.  Latest starts: ``z_k = close_k``,
``z_i = min(close_i, z_{i+1} - qt(s_i, s_{i+1}) - sv_i)``.

Alone-feasibility of every stop ``s``, checked first, in ascending ``s``: in float64 with the
greedy's own expressions ``float(demand[s]) <= cap`` and ``(0.0 + (d[0][s] + d[s][0])) <= max_dist``;
in integers ``q`` and ``qt`` usable both ways and ``max(qt(0,s), open_s) <= close_s``.  Any failure
raises :class:`InfeasibleStops` with all failing stops (ascending; status 1 on the GPU).

Construction, while stops are unrouted:

1. seed a trip with the unrouted stop of smallest ``(close_q, index)``; ``Lq = q(0,s) + q(s,0)``,
   ``Wq = qd[s]``;
2. for every unrouted ``u`` and position ``j in 0..k`` between ``a = t[j]`` and ``b = t[j+1]``:
   ``ins = q(a,u) + q(u,b) - q(a,b)``, ``st = max(dep_j + qt(a,u), open_u)``;
3. the candidate is admissible iff ``q(a,u)``, ``q(u,b)``, ``qt(a,u)``, ``qt(u,b)`` are usable,
   ``st <= close_u``, ``j == k`` or ``st + sv_u + qt(u,b) <= z_{j+1}``, ``Wq + qd[u] <= cap_q`` and
   ``Lq + ins <= max_q``;
4. the admissible candidate of smallest ``(ins, u, j)`` is taken; none: the trip is closed;
5. the lengthened trip is walked in float64 as the greedy measures it (:func:`improve.walk_feasible`
   against ``max_dist``, :func:`exchange.load_feasible` against ``cap``); if either fails the
   insertion is not applied and the trip is closed (``rejected`` counts these);
6. otherwise the insertion is applied: ``Lq += ins``, ``Wq += qd[u]``, ``dep`` and ``z`` are
   recomputed, and the scan repeats from 2.

Every trip holds at least its seed, so the construction ends; trips come out in the order they were
built.  Pushing the stops behind ``j`` later by the insertion keeps the trip feasible exactly when
the new start of ``t[j+1]`` is ``<= z_{j+1}`` (waiting only absorbs delay), which is what test 3
checks in O(1); the tests compare it with re-simulating the whole trip on every candidate.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .exchange import UNBOUNDED, load_feasible, quantize_limit
from .greedy import InfeasibleStops
from .improve import BIG, quantize, quantize_matrix, walk_feasible

MAX_STOPS = 128
METHOD = "cheapest_insertion"
USABLE_LIMIT = (1 << 31) - 1          # entries of q / qt from here on are unusable
FIELD_LIMIT = 2_000_000.0             # seconds: the largest open / close / service
NEEDS_MATRIX_TIMES = ("time windows need the haversine provider or the CCH road router "
                      "(time_window / service are not supported by this provider or engine)")

Schedule = List[List[Tuple[int, int, int, int]]]       # per trip: (stop, arrival, start, departure)


def usable_matrix(m) -> np.ndarray:
    """``quantize_matrix`` with every entry ``>= 2**31 - 1`` set to ``BIG``."""
    q = quantize_matrix(np.asarray(m, dtype=np.float64))
    q[q >= USABLE_LIMIT] = BIG
    return q


def limit_q(x: float) -> int:
    v = quantize_limit(x)
    return -1 if v is None else v


def schedule_of(qt: np.ndarray, trip: Sequence[int], open_q, close_q, sv_q):
    """(arr, start, dep, feasible) over the positions ``0..k`` of ``trip`` by the recurrence;
    ``feasible`` also asks for a usable leg back to the depot."""
    k = len(trip) - 2
    arr, start, dep = [0] * (k + 1), [0] * (k + 1), [0] * (k + 1)
    ok = True
    for i in range(1, k + 1):
        leg = int(qt[trip[i - 1], trip[i]])
        ok = ok and leg < BIG
        arr[i] = dep[i - 1] + leg
        start[i] = max(arr[i], int(open_q[trip[i]]))
        ok = ok and start[i] <= int(close_q[trip[i]])
        dep[i] = start[i] + int(sv_q[trip[i]])
    ok = ok and int(qt[trip[k], 0]) < BIG
    return arr, start, dep, ok


def latest_starts(qt: np.ndarray, trip: Sequence[int], close_q, sv_q) -> List[int]:
    """``z[1..k]`` (``z[0]`` unused)."""
    k = len(trip) - 2
    z = [0] * (k + 1)
    z[k] = int(close_q[trip[k]])
    for i in range(k - 1, 0, -1):
        z[i] = min(int(close_q[trip[i]]), z[i + 1] - int(qt[trip[i], trip[i + 1]]) - int(sv_q[trip[i]]))
    return z


def time_admissible(qt, trip, dep, z, u: int, j: int, open_q, close_q, sv_q) -> bool:
    """The time part of test 3 for inserting ``u`` behind position ``j``."""
    k = len(trip) - 2
    a, b = trip[j], trip[j + 1]
    if int(qt[a, u]) >= BIG or int(qt[u, b]) >= BIG:
        return False
    st = max(dep[j] + int(qt[a, u]), int(open_q[u]))
    if st > int(close_q[u]):
        return False
    return j == k or st + int(sv_q[u]) + int(qt[u, b]) <= z[j + 1]


def alone_infeasible(dn, q, qt, demand, cap: float, max_dist: float, open_q, close_q) -> List[int]:
    """0-based destination indices of the stops that no trip of their own can serve, ascending."""
    bad = []
    for s in range(1, dn.shape[0]):
        ok = float(demand[s]) <= cap and (0.0 + (float(dn[0][s]) + float(dn[s][0]))) <= max_dist
        ok = ok and max(int(q[0, s]), int(q[s, 0]), int(qt[0, s]), int(qt[s, 0])) < BIG
        ok = ok and max(int(qt[0, s]), int(open_q[s])) <= int(close_q[s])
        if not ok:
            bad.append(s - 1)
    return bad


def best_insertion(q, qt, qd, trip, dep, z, unrouted: np.ndarray, Lq: int, Wq: int, cap_q: int,
                   max_q: int, open_q, close_q, sv_q) -> Optional[Tuple[int, int, int]]:
    """(ins, u, j) of the admissible candidate of smallest (ins, u, j), or None."""
    k = len(trip) - 2
    U = np.flatnonzero(unrouted)
    if U.size == 0:
        return None
    a = np.array(trip[:-1], dtype=np.int64)[None, :]
    b = np.array(trip[1:], dtype=np.int64)[None, :]
    u = U[:, None]
    qau, qub, tau, tub = q[a, u], q[u, b], qt[a, u], qt[u, b]
    usable = (qau < BIG) & (qub < BIG) & (tau < BIG) & (tub < BIG)
    ins = qau + qub - q[a, b]
    st = np.maximum(np.array(dep, dtype=np.int64)[None, :] + tau, open_q[u])
    zn = np.array(list(z[1:]) + [0], dtype=np.int64)[None, :]      # z[j + 1]; unused at j == k
    last = (np.arange(k + 1) == k)[None, :]
    with np.errstate(over="ignore"):
        ok = (usable & (st <= close_q[u]) & (last | (st + sv_q[u] + tub <= zn))
              & (Wq + qd[u] <= cap_q) & (Lq + ins <= max_q))
    if not ok.any():
        return None
    c = int(np.argmin(np.where(ok, ins, np.int64(1) << 62)))      # first minimum in (u, j) order
    r, j = divmod(c, k + 1)
    return int(ins[r, j]), int(U[r]), int(j)


def tw_trips(d, t, demand: Sequence[float], cap: float, max_dist: float, open_q: Sequence[int],
             close_q: Sequence[int], sv_q: Sequence[int], trace: Optional[list] = None
             ) -> Tuple[List[List[int]], Schedule, Dict[str, int]]:
    """``d`` / ``t``: (ns+1)x(ns+1) float64 metres / seconds over [depot] + stops; ``demand[s]``,
    ``open_q[s]``, ``close_q[s]``, ``sv_q[s]`` per point (index 0 ignored).  Returns the trips
    ``[0, ..., 0]``, per trip the ``(stop, arrival, start, departure)`` milliseconds of its stops, and
    ``{"insertions", "rejected", "trips", "len_q", "waiting_q"}``.  Raises :class:`InfeasibleStops`.
    ``trace``: a list that receives ``(trip, dep, z, unrouted stops)`` before every scan (tests)."""
    dn = np.asarray(d, dtype=np.float64)
    tn = np.asarray(t, dtype=np.float64)
    n1 = dn.shape[0]
    ns = n1 - 1
    if tn.shape != dn.shape or dn.shape != (n1, n1):
        raise ValueError("the distance and the time matrix must be square and of one shape")
    if ns > MAX_STOPS:
        raise ValueError(f"at most {MAX_STOPS} stops with time windows, got {ns}")
    cap, max_dist = float(cap), float(max_dist)
    q, qt = usable_matrix(dn), usable_matrix(tn)
    qd = np.array([0] + [quantize(demand[s]) for s in range(1, n1)], dtype=np.int64)
    op = np.array([0] + [int(open_q[s]) for s in range(1, n1)], dtype=np.int64)
    cl = np.array([UNBOUNDED] + [int(close_q[s]) for s in range(1, n1)], dtype=np.int64)
    sv = np.array([0] + [int(sv_q[s]) for s in range(1, n1)], dtype=np.int64)
    cap_q, max_q = limit_q(cap), limit_q(max_dist)
    bad = alone_infeasible(dn, q, qt, demand, cap, max_dist, op, cl)
    if bad:
        raise InfeasibleStops(bad, time_windows=True)
    unrouted = np.zeros(n1, dtype=bool)
    unrouted[1:] = True
    trips: List[List[int]] = []
    schedule: Schedule = []
    stats = {"insertions": 0, "rejected": 0, "trips": 0, "len_q": 0, "waiting_q": 0}
    while unrouted.any():
        U = np.flatnonzero(unrouted)
        seed = int(U[np.lexsort((U, cl[U]))[0]])
        trip = [0, seed, 0]
        unrouted[seed] = False
        Lq, Wq = int(q[0, seed]) + int(q[seed, 0]), int(qd[seed])
        while True:
            _, _, dep, _ = schedule_of(qt, trip, op, cl, sv)
            z = latest_starts(qt, trip, cl, sv)
            if trace is not None:
                trace.append((list(trip), list(dep), list(z), [int(v) for v in np.flatnonzero(unrouted)]))
            best = best_insertion(q, qt, qd, trip, dep, z, unrouted, Lq, Wq, cap_q, max_q, op, cl, sv)
            if best is None:
                break
            ins, u, j = best
            new = trip[:j + 1] + [u] + trip[j + 1:]
            if not (walk_feasible(dn, new, max_dist) and load_feasible(demand, new, cap)):
                stats["rejected"] += 1
                break
            trip = new
            unrouted[u] = False
            Lq += ins
            Wq += int(qd[u])
            stats["insertions"] += 1
        arr, start, dep, _ = schedule_of(qt, trip, op, cl, sv)
        k = len(trip) - 2
        trips.append(trip)
        schedule.append([(trip[i], arr[i], start[i], dep[i]) for i in range(1, k + 1)])
        stats["len_q"] += Lq
        stats["waiting_q"] += sum(start[i] - arr[i] for i in range(1, k + 1))
    stats["trips"] = len(trips)
    return trips, schedule, stats


# ------------------------------------------------------------------ the request fields
def _is_tw_request(payload) -> bool:
    return (isinstance(payload, dict) and isinstance(payload.get("destination_points"), list)
            and len(payload["destination_points"]) > 1)


def wants_time_windows(payload) -> bool:
    """A multi-stop request is a time-window request iff a destination carries ``time_window`` or
    ``service``; single-destination and ``alternatives`` requests ignore the fields."""
    if not _is_tw_request(payload):
        return False
    alt = payload.get("alternatives")
    if isinstance(alt, (int, float)) and not isinstance(alt, bool) and alt >= 2:
        return False
    return any(isinstance(p, dict) and ("time_window" in p or "service" in p)
               for p in payload["destination_points"])


def _seconds(v: Any) -> Optional[float]:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return None
    v = float(v)
    return v if math.isfinite(v) else None


def parse_time_windows(payload) -> Tuple[List[int], List[int], List[int]]:
    """``(open_q, close_q, sv_q)`` per point of ``[source] + destination_points`` (index 0 the
    depot).  Raises ``ValueError`` naming the field on a malformed one or on more than 128 stops."""
    dests = payload["destination_points"]
    if len(dests) > MAX_STOPS:
        raise ValueError(f"destination_points: at most {MAX_STOPS} destinations with time_window / "
                         f"service, got {len(dests)}")
    open_q, close_q, sv_q = [0], [UNBOUNDED], [0]
    for i, p in enumerate(dests):
        o, c, s = 0, UNBOUNDED, 0
        if isinstance(p, dict) and "time_window" in p:
            w = p["time_window"]
            lo = _seconds(w[0]) if isinstance(w, (list, tuple)) and len(w) == 2 else None
            hi = _seconds(w[1]) if lo is not None else None
            if lo is None or hi is None or not (0.0 <= lo <= hi <= FIELD_LIMIT):
                raise ValueError(f"destination_points[{i}].time_window must be [open, close] in seconds "
                                 f"with 0 <= open <= close <= {int(FIELD_LIMIT)}")
            o, c = quantize(lo), quantize(hi)
        if isinstance(p, dict) and "service" in p:
            v = _seconds(p["service"])
            if v is None or not (0.0 <= v <= FIELD_LIMIT):
                raise ValueError(f"destination_points[{i}].service must be a number of seconds in "
                                 f"[0, {int(FIELD_LIMIT)}]")
            s = quantize(v)
        open_q.append(o)
        close_q.append(c)
        sv_q.append(s)
    return open_q, close_q, sv_q


def schedule_properties(schedule: Schedule, stats: Dict[str, int], close_q: Sequence[int]
                        ) -> Tuple[List[List[Dict[str, Any]]], Dict[str, Any]]:
    """``(properties.schedule, properties.time_windows)`` of a response; seconds.  With
    ``stats["search"]`` (the statistics of :mod:`routing.tw_improve`) the second also reports the
    local search."""
    out = [[{"destination": s - 1, "arrival": a / 1000.0, "start": b / 1000.0,
             "departure": c / 1000.0, "waiting": (b - a) / 1000.0} for s, a, b, c in trip]
           for trip in schedule]
    search = stats.get("search")
    if search is not None:
        info = {"method": METHOD + "+relocate+swap",
                "stops_with_windows": sum(1 for c in close_q[1:] if int(c) < UNBOUNDED),
                "trips": int(search["trips_after"]), "waiting": int(search["waiting_q"]) / 1000.0,
                "moves": int(search["moves"]), "trips_before": int(search["trips_before"]),
                "matrix_distance_before": int(search["len_before_q"]) / 1000.0,
                "matrix_distance_after": int(search["len_after_q"]) / 1000.0}
        return out, info
    info = {"method": METHOD,
            "stops_with_windows": sum(1 for c in close_q[1:] if int(c) < UNBOUNDED),
            "trips": int(stats["trips"]), "waiting": int(stats["waiting_q"]) / 1000.0}
    return out, info


def schedule_from_trips(t, trips: Sequence[Sequence[int]], open_q, close_q, sv_q
                        ) -> Tuple[Schedule, Dict[str, int]]:
    """The schedule and the reported statistics of given trips (the batched paths hand the trips
    over and the schedule is a function of them)."""
    qt = usable_matrix(t)
    schedule: Schedule = []
    waiting = 0
    for trip in trips:
        arr, start, dep, _ = schedule_of(qt, trip, open_q, close_q, sv_q)
        k = len(trip) - 2
        schedule.append([(int(trip[i]), arr[i], start[i], dep[i]) for i in range(1, k + 1)])
        waiting += sum(start[i] - arr[i] for i in range(1, k + 1))
    return schedule, {"trips": len(trips), "waiting_q": waiting}
