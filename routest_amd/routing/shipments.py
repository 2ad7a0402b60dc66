"""Pickup-and-delivery pairs in multi-stop routing: cheapest insertion of units — CPU reference.

A delivery entry of ``destination_points`` may carry ``"pickup_from": p``, the 0-based index of
another entry: the delivery ``v`` and its pickup ``p`` form a *pair*.  The pair's amount is the
delivery's ``payload``; both stops are visited by one trip, ``p`` before ``v``, and the amount is
on board from leaving ``p`` until arriving at ``v``.  Entries in no pair stay *plain* stops: loaded
at the depot, dropped at the stop.  A multi-stop request in which a destination carries the field
is a *shipment request* and is planned by :func:`pd_trips`; ``time_window`` / ``service`` are
honoured on every stop, ``improve`` / ``exchange`` / ``tw_improve`` are ignored (their moves take
single stops and would split pairs; ``shipment_improve`` asks for the search that moves whole units,
:mod:`routing.shipment_improve`).  Single-destination and ``alternatives`` requests ignore the
field.  The definition is schedule-independent, so this reference, the host C++ (``rtr::pd_trips``,
``csrc/runtime/route_core.h``) and the GPU kernel (K6f, ``csrc/route_pd.hip``) return the same
trips, schedule and statistics, compared with ``==``.

Carried over from :mod:`routing.timewindows`, unchanged: ``q``, ``qt`` (``usable_matrix``), ``qd``,
``open_q`` / ``close_q`` / ``sv_q``, ``cap_q`` / ``max_q`` (``limit_q``), ``dep`` / ``z``
(``schedule_of``, ``latest_starts``), the unusable-entry rule, int64 sums, at most 128 stops.

Kinds.  ``pickup_from[s]`` per point of ``[depot] + stops`` (index 0 ignored) is the *point* index
(``1..ns``) of the pickup of delivery ``s``, or negative: none.  It must name another stop that is
itself no delivery and is named by no other delivery (``ValueError``; status 3 on the GPU).
``kind[s]`` is ``PLAIN``, ``PICKUP`` or ``DELIVERY``, ``mate[s]`` the other stop of the pair (0 for
a plain stop) and ``amt(p) = qd[mate[p]]``; the demand of a pickup entry itself is never read.

Integer load profile of a trip ``t[0..k+1]``: ``load[x]`` is the load on leaving position ``x``,
``load[0]`` the sum of ``qd`` over the trip's plain stops, then ``load[x] = load[x-1] - qd[s]``
behind a plain stop or a delivery and ``load[x-1] + amt`` behind a pickup; ``pm[x] = max(load[0..x])``.
The float64 walk :func:`pd_load_feasible` uses adds and subtracts only, in trip order; without pairs
it is ``exchange.load_feasible``.

Alone-feasibility, checked first, in ascending stop order: a plain stop exactly as
``timewindows.alone_infeasible``; a pair once, at its pickup, as the trip ``[0, p, v, 0]``
(``walk_feasible``, :func:`pd_load_feasible`, all three legs usable in ``q`` and ``qt``,
``schedule_of`` feasible); a failing pair reports both indices.  The ascending list is raised as
:class:`InfeasibleStops` (status 1 on the GPU).

Construction.  A *unit* is a plain stop or a pair, identified by its plain stop or its pickup ``u``.
While units are unrouted:

1. seed a trip with the unrouted unit of smallest ``(key, u)``, ``key = close_q[u]`` for a plain
   stop and ``min(close_q[p], close_q[v])`` for a pair; the trip is ``[0,u,0]`` or ``[0,p,v,0]``
   (no integer test is made on a seed: alone-feasibility admitted it);
2. a plain ``u`` behind position ``i`` (``a = t[i]``, ``b = t[i+1]``) is K6d's candidate with the
   load test ``pm[i] + qd[u] <= cap_q``;
3. a pair ``(p, v)``, ``p`` behind ``i`` and ``v`` behind ``j``, ``i <= j <= k``; all used entries
   usable; ``stp = max(dep[i] + qt(a,p), open_p) <= close_p``;

   * ``j == i`` (``a -> p -> v -> b``): ``ins = q(a,p) + q(p,v) + q(v,b) - q(a,b)``;
     ``stv = max(stp + sv_p + qt(p,v), open_v) <= close_v``; ``i == k`` or
     ``stv + sv_v + qt(v,b) <= z[i+1]``; ``load[i] + amt <= cap_q``;
   * ``j > i``: ``stp + sv_p + qt(p,b) <= z[i+1]`` (every stop up to ``j`` stays feasible); shifted
     departures ``nd[i+1] = max(stp + sv_p + qt(p,b), open_b) + sv_b``,
     ``nd[x] = max(nd[x-1] + qt(t[x-1],t[x]), open_t[x]) + sv_t[x]``; with ``c = t[j]``, ``e = t[j+1]``:
     ``ins = [q(a,p) + q(p,b) - q(a,b)] + [q(c,v) + q(v,e) - q(c,e)]``;
     ``stv = max(nd[j] + qt(c,v), open_v) <= close_v``; ``j == k`` or
     ``stv + sv_v + qt(v,e) <= z[j+1]``; ``max(load[i..j]) + amt <= cap_q``;

   both: ``Lq + ins <= max_q``;
4. the admissible candidate of smallest ``(ins, u, i, j)`` is taken (a plain one has ``j = i``);
   none: the trip is closed;
5. the lengthened trip is walked in float64 (``walk_feasible`` against ``max_dist``,
   :func:`pd_load_feasible` against ``cap``); on failure the insertion is not applied, ``rejected``
   counts it and the trip is closed;
6. otherwise it is applied, ``Lq += ins``, and ``dep``, ``z``, ``load``, ``pm`` are recomputed.

``insertions`` counts units, so ``insertions + trips`` is the number of units.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .exchange import UNBOUNDED
from .greedy import InfeasibleStops
from .improve import BIG, quantize, walk_feasible
from .timewindows import (MAX_STOPS, Schedule, latest_starts, limit_q, schedule_of,
                          schedule_properties, usable_matrix)

PLAIN, PICKUP, DELIVERY = 0, 1, 2
KIND_NAMES = ("stop", "pickup", "delivery")
NEEDS_MATRIX_TIMES = ("shipments need the haversine provider or the CCH road router "
                      "(pickup_from is not supported by this provider or engine)")
_INF = np.int64(1) << 62


def kinds_of(pickup_from: Sequence[int], n1: int) -> Tuple[List[int], List[int]]:
    """``(kind, mate)`` per point; ``ValueError`` on a malformed ``pickup_from``."""
    if len(pickup_from) != n1:
        raise ValueError("pickup_from must hold one entry per point")
    kind, mate = [PLAIN] * n1, [0] * n1
    for v in range(1, n1):
        p = int(pickup_from[v])
        if p < 0:
            continue
        if p < 1 or p >= n1 or p == v:
            raise ValueError(f"pickup_from[{v}] must name another stop")
        kind[v], mate[v] = DELIVERY, p
    for v in range(1, n1):
        if kind[v] != DELIVERY:
            continue
        p = mate[v]
        if kind[p] == DELIVERY:
            raise ValueError(f"pickup_from[{v}] names a stop that is itself a delivery")
        if kind[p] == PICKUP:
            raise ValueError(f"pickup_from[{v}] names the pickup of another delivery")
        kind[p], mate[p] = PICKUP, v
    return kind, mate


def load_profile(qd, kind, mate, trip: Sequence[int]) -> List[int]:
    """``load[0..k]``: the integer load on leaving every position."""
    k = len(trip) - 2
    load = [0] * (k + 1)
    load[0] = sum(int(qd[s]) for s in trip[1:-1] if kind[s] == PLAIN)
    for x in range(1, k + 1):
        s = trip[x]
        load[x] = load[x - 1] + int(qd[mate[s]]) if kind[s] == PICKUP else load[x - 1] - int(qd[s])
    return load


def pd_load_feasible(demand, kind, mate, t: Sequence[int], cap: float) -> bool:
    """The float64 load walk over the order ``t``: adds and subtracts only, in this order."""
    base = 0.0
    for s in t[1:-1]:
        if kind[s] == PLAIN:
            base += float(demand[s])
    ok = bool(base <= cap)
    load = base
    for s in t[1:-1]:
        if kind[s] == PICKUP:
            load += float(demand[mate[s]])
            ok = ok and bool(load <= cap)
        else:
            load -= float(demand[s])
    return ok


def alone_infeasible(dn, q, qt, demand, cap: float, max_dist: float, open_q, close_q, sv_q, kind, mate
                     ) -> List[int]:
    """0-based destination indices of the stops no trip of their own unit can serve, ascending."""
    bad = []
    for s in range(1, dn.shape[0]):
        if kind[s] == PLAIN:
            ok = float(demand[s]) <= cap and (0.0 + (float(dn[0][s]) + float(dn[s][0]))) <= max_dist
            ok = ok and max(int(q[0, s]), int(q[s, 0]), int(qt[0, s]), int(qt[s, 0])) < BIG
            ok = ok and max(int(qt[0, s]), int(open_q[s])) <= int(close_q[s])
            if not ok:
                bad.append(s - 1)
        elif kind[s] == PICKUP:
            v = mate[s]
            trip = [0, s, v, 0]
            ok = walk_feasible(dn, trip, max_dist) and pd_load_feasible(demand, kind, mate, trip, cap)
            ok = ok and max(int(q[0, s]), int(q[s, v]), int(q[v, 0]), int(qt[0, s]), int(qt[s, v]), int(qt[v, 0])) < BIG
            ok = ok and schedule_of(qt, trip, open_q, close_q, sv_q)[3]
            if not ok:
                bad += [s - 1, v - 1]
    return sorted(bad)


def candidate_tests(q, qt, qd, kind, mate, trip, dep, z, load, Lq: int, cap_q: int, max_q: int,
                    open_q, close_q, sv_q, u: int, i: int, j: int) -> Tuple[int, Dict[str, bool]]:
    """One candidate of step 2 / 3, test by test (the scalar form of the definition; the tests
    compare it with re-simulation): ``(ins, {"usable", "time_u", "z_u", "time_v", "z_v", "load",
    "length"})``.  A test that an earlier failure leaves undefined is reported as False; ``ins`` is 0
    when an entry is unusable."""
    k = len(trip) - 2
    a, b = trip[i], trip[i + 1]
    res = dict.fromkeys(("usable", "time_u", "z_u", "time_v", "z_v", "load", "length"), False)
    Q = lambda x, y: int(q[x, y])       # noqa: E731
    T = lambda x, y: int(qt[x, y])      # noqa: E731
    if kind[u] == PLAIN:
        if max(Q(a, u), Q(u, b), T(a, u), T(u, b)) >= BIG:
            return 0, res
        res["usable"] = True
        ins = Q(a, u) + Q(u, b) - Q(a, b)
        st = max(dep[i] + T(a, u), int(open_q[u]))
        res["time_u"] = st <= int(close_q[u])
        res["z_u"] = i == k or st + int(sv_q[u]) + T(u, b) <= z[i + 1]
        res["time_v"] = res["z_v"] = True
        res["load"] = max(load[:i + 1]) + int(qd[u]) <= cap_q
        res["length"] = Lq + ins <= max_q
        return ins, res
    p, v = u, mate[u]
    amt = int(qd[v])
    if j == i:
        if max(Q(a, p), Q(p, v), Q(v, b), T(a, p), T(p, v), T(v, b)) >= BIG:
            return 0, res
        res["usable"] = True
        ins = Q(a, p) + Q(p, v) + Q(v, b) - Q(a, b)
        stp = max(dep[i] + T(a, p), int(open_q[p]))
        res["time_u"] = stp <= int(close_q[p])
        res["z_u"] = True
        stv = max(stp + int(sv_q[p]) + T(p, v), int(open_q[v]))
        res["time_v"] = stv <= int(close_q[v])
        res["z_v"] = i == k or stv + int(sv_q[v]) + T(v, b) <= z[i + 1]
        res["load"] = load[i] + amt <= cap_q
        res["length"] = Lq + ins <= max_q
        return ins, res
    c, e = trip[j], trip[j + 1]
    if max(Q(a, p), Q(p, b), Q(c, v), Q(v, e), T(a, p), T(p, b), T(c, v), T(v, e)) >= BIG:
        return 0, res
    res["usable"] = True
    ins = (Q(a, p) + Q(p, b) - Q(a, b)) + (Q(c, v) + Q(v, e) - Q(c, e))
    stp = max(dep[i] + T(a, p), int(open_q[p]))
    res["time_u"] = stp <= int(close_q[p])
    first = stp + int(sv_q[p]) + T(p, b)
    res["z_u"] = first <= z[i + 1]
    nd = max(first, int(open_q[b])) + int(sv_q[b])
    for x in range(i + 2, j + 1):
        nd = max(nd + T(trip[x - 1], trip[x]), int(open_q[trip[x]])) + int(sv_q[trip[x]])
    stv = max(nd + T(c, v), int(open_q[v]))
    res["time_v"] = stv <= int(close_q[v])
    res["z_v"] = j == k or stv + int(sv_q[v]) + T(v, e) <= z[j + 1]
    res["load"] = max(load[i:j + 1]) + amt <= cap_q
    res["length"] = Lq + ins <= max_q
    return ins, res


def best_insertion(q, qt, qd, kind, mate, trip, dep, z, load, unrouted: np.ndarray, Lq: int, cap_q: int,
                   max_q: int, open_q, close_q, sv_q) -> Optional[Tuple[int, int, int, int]]:
    """``(ins, u, i, j)`` of the admissible candidate of smallest ``(ins, u, i, j)``, or None."""
    k = len(trip) - 2
    kd = np.asarray(kind)
    units = np.flatnonzero(unrouted & (kd != DELIVERY))
    if units.size == 0:
        return None
    found = []                  # per scan below its first minimum; the smallest tuple of them wins
    a = np.array(trip[:-1], dtype=np.int64)[None, :]            # t[i], i = 0..k
    b = np.array(trip[1:], dtype=np.int64)[None, :]             # t[i+1]
    depv = np.array(dep, dtype=np.int64)[None, :]
    zn = np.array(list(z[1:]) + [0], dtype=np.int64)[None, :]   # z[i+1]; unused at i == k
    last = (np.arange(k + 1) == k)[None, :]
    ld = np.array(load, dtype=np.int64)
    pm = np.maximum.accumulate(ld)[None, :]
    qab = q[a, b]

    def first_min(ok, ins, U, jof):
        # the first minimum in (u, i) order of the masked costs; j = jof(i)
        if ok.any():
            c = int(np.argmin(np.where(ok, ins, _INF)))
            r, i = divmod(c, k + 1)
            found.append((int(ins[r, i]), int(U[r]), int(i), int(jof(i))))

    with np.errstate(over="ignore"):
        U = units[kd[units] == PLAIN]
        if U.size:
            u = U[:, None]
            qau, qub, tau, tub = q[a, u], q[u, b], qt[a, u], qt[u, b]
            ins = qau + qub - qab
            st = np.maximum(depv + tau, open_q[u])
            ok = ((qau < BIG) & (qub < BIG) & (tau < BIG) & (tub < BIG) & (st <= close_q[u])
                  & (last | (st + sv_q[u] + tub <= zn)) & (pm + qd[u] <= cap_q) & (Lq + ins <= max_q))
            first_min(ok, ins, U, lambda i: i)
        P = units[kd[units] == PICKUP]
        if P.size:
            p = P[:, None]
            v = np.asarray(mate, dtype=np.int64)[P][:, None]
            amt = qd[v]
            qap, tap = q[a, p], qt[a, p]
            stp = np.maximum(depv + tap, open_q[p])
            okp = (qap < BIG) & (tap < BIG) & (stp <= close_q[p])
            # j == i
            qpv, tpv, qvb, tvb = q[p, v], qt[p, v], q[v, b], qt[v, b]
            ins = qap + qpv + qvb - qab
            stv = np.maximum(stp + sv_q[p] + tpv, open_q[v])
            ok = (okp & (qpv < BIG) & (tpv < BIG) & (qvb < BIG) & (tvb < BIG) & (stv <= close_q[v])
                  & (last | (stv + sv_q[v] + tvb <= zn)) & (ld[None, :] + amt <= cap_q) & (Lq + ins <= max_q))
            first_min(ok, ins, P, lambda i: i)
            # j > i: every (pair, i) carries nd, the running maximum of the load and its first bracket
            qpb, tpb = q[p, b], qt[p, b]
            first = stp + sv_q[p] + tpb
            live = okp & (qpb < BIG) & (tpb < BIG) & ~last & (first <= zn)
            ins1 = qap + qpb - qab
            nd = np.zeros_like(first)
            mx = np.broadcast_to(ld[None, :], first.shape).copy()
            cols = np.arange(k + 1)[None, :]
            for j in range(1, k + 1):
                s = trip[j]
                started = cols == j - 1
                step = np.maximum(nd + int(qt[trip[j - 1], s]), int(open_q[s])) + int(sv_q[s])
                nd = np.where(started, np.maximum(first, int(open_q[s])) + int(sv_q[s]), step)
                mx = np.where(cols < j, np.maximum(mx, ld[j]), mx)      # max(load[i..j]) of the columns i < j
                e = trip[j + 1]
                qcv, tcv, qve, tve = q[s, v], qt[s, v], q[v, e], qt[v, e]
                ins = ins1 + (qcv + qve - int(q[s, e]))
                stv = np.maximum(nd + tcv, open_q[v])
                ok = (live & (cols < j) & (qcv < BIG) & (tcv < BIG) & (qve < BIG) & (tve < BIG)
                      & (stv <= close_q[v]) & (mx + amt <= cap_q) & (Lq + ins <= max_q))
                if j < k:
                    ok &= stv + sv_q[v] + tve <= z[j + 1]
                first_min(ok, ins, P, lambda i: j)
    return min(found) if found else None


def apply_insertion(trip: Sequence[int], mate, kind, u: int, i: int, j: int) -> List[int]:
    """The trip with unit ``u`` inserted: ``u`` behind position ``i`` and, for a pair, its delivery
    behind position ``j`` of the trip as it was."""
    if kind[u] == PLAIN:
        return list(trip[:i + 1]) + [u] + list(trip[i + 1:])
    return list(trip[:i + 1]) + [u] + list(trip[i + 1:j + 1]) + [mate[u]] + list(trip[j + 1:])


def pd_trips(d, t, demand: Sequence[float], cap: float, max_dist: float, open_q: Sequence[int],
             close_q: Sequence[int], sv_q: Sequence[int], pickup_from: Sequence[int],
             trace: Optional[list] = None) -> Tuple[List[List[int]], Schedule, Dict[str, int]]:
    """Arguments as :func:`timewindows.tw_trips` takes them, with ``pickup_from[s]`` per point (see
    the module).  Returns the trips ``[0, ..., 0]``, per trip the ``(stop, arrival, start,
    departure)`` milliseconds of its stops, and ``{"insertions", "rejected", "trips", "len_q",
    "waiting_q"}``.  Raises :class:`InfeasibleStops`.  ``trace``: a list that receives
    ``(trip, dep, z, unrouted stops, load, Lq)`` before every scan (tests)."""
    dn = np.asarray(d, dtype=np.float64)
    tn = np.asarray(t, dtype=np.float64)
    n1 = dn.shape[0]
    ns = n1 - 1
    if tn.shape != dn.shape or dn.shape != (n1, n1):
        raise ValueError("the distance and the time matrix must be square and of one shape")
    if ns > MAX_STOPS:
        raise ValueError(f"at most {MAX_STOPS} stops with shipments, got {ns}")
    kind, mate = kinds_of(pickup_from, n1)
    cap, max_dist = float(cap), float(max_dist)
    q, qt = usable_matrix(dn), usable_matrix(tn)
    qd = np.array([0] + [quantize(demand[s]) for s in range(1, n1)], dtype=np.int64)
    op = np.array([0] + [int(open_q[s]) for s in range(1, n1)], dtype=np.int64)
    cl = np.array([UNBOUNDED] + [int(close_q[s]) for s in range(1, n1)], dtype=np.int64)
    sv = np.array([0] + [int(sv_q[s]) for s in range(1, n1)], dtype=np.int64)
    cap_q, max_q = limit_q(cap), limit_q(max_dist)
    bad = alone_infeasible(dn, q, qt, demand, cap, max_dist, op, cl, sv, kind, mate)
    if bad:
        raise InfeasibleStops(bad, time_windows=True)
    unrouted = np.zeros(n1, dtype=bool)
    unrouted[1:] = True
    trips: List[List[int]] = []
    schedule: Schedule = []
    stats = {"insertions": 0, "rejected": 0, "trips": 0, "len_q": 0, "waiting_q": 0}
    while unrouted.any():
        seed, key = -1, 0
        for u in np.flatnonzero(unrouted).tolist():
            if kind[u] == DELIVERY:
                continue
            ku = int(cl[u]) if kind[u] == PLAIN else min(int(cl[u]), int(cl[mate[u]]))
            if seed < 0 or ku < key:
                seed, key = u, ku
        trip = [0, seed, 0] if kind[seed] == PLAIN else [0, seed, mate[seed], 0]
        for s in trip[1:-1]:
            unrouted[s] = False
        Lq = sum(int(q[trip[x], trip[x + 1]]) for x in range(len(trip) - 1))
        while True:
            _, _, dep, _ = schedule_of(qt, trip, op, cl, sv)
            z = latest_starts(qt, trip, cl, sv)
            load = load_profile(qd, kind, mate, trip)
            if trace is not None:
                trace.append((list(trip), list(dep), list(z), [int(v) for v in np.flatnonzero(unrouted)],
                              list(load), Lq))
            best = best_insertion(q, qt, qd, kind, mate, trip, dep, z, load, unrouted, Lq, cap_q, max_q, op, cl, sv)
            if best is None:
                break
            ins, u, i, j = best
            new = apply_insertion(trip, mate, kind, u, i, j)
            if not (walk_feasible(dn, new, max_dist) and pd_load_feasible(demand, kind, mate, new, cap)):
                stats["rejected"] += 1
                break
            trip = new
            unrouted[u] = False
            if kind[u] == PICKUP:
                unrouted[mate[u]] = False
            Lq += ins
            stats["insertions"] += 1
        arr, start, dep, _ = schedule_of(qt, trip, op, cl, sv)
        k = len(trip) - 2
        trips.append(trip)
        schedule.append([(trip[i], arr[i], start[i], dep[i]) for i in range(1, k + 1)])
        stats["len_q"] += Lq
        stats["waiting_q"] += sum(start[i] - arr[i] for i in range(1, k + 1))
    stats["trips"] = len(trips)
    return trips, schedule, stats


# ------------------------------------------------------------------ the request field
def _float(v: Any, default: float) -> float:
    try:
        return float(v)
    except (TypeError, ValueError):
        return default


def wants_shipments(payload) -> bool:
    """A multi-stop request is a shipment request iff a destination carries ``pickup_from``;
    single-destination and ``alternatives`` requests ignore the field."""
    if not (isinstance(payload, dict) and isinstance(payload.get("destination_points"), list)
            and len(payload["destination_points"]) > 1):
        return False
    alt = payload.get("alternatives")
    if isinstance(alt, (int, float)) and not isinstance(alt, bool) and alt >= 2:
        return False
    return any(isinstance(p, dict) and "pickup_from" in p for p in payload["destination_points"])


def parse_shipments(payload) -> List[int]:
    """``pickup_from`` per point of ``[source] + destination_points`` as :func:`pd_trips` takes it:
    the point index of a delivery's pickup, ``-1`` elsewhere.  Raises ``ValueError`` naming the
    field on a malformed one or on more than 128 destinations."""
    dests = payload["destination_points"]
    if len(dests) > MAX_STOPS:
        raise ValueError(f"destination_points: at most {MAX_STOPS} destinations with time_window / "
                         f"service, got {len(dests)}")
    out = [-1] * (len(dests) + 1)
    used = set()
    for i, d in enumerate(dests):
        if not (isinstance(d, dict) and "pickup_from" in d):
            continue
        name = f"destination_points[{i}].pickup_from"
        p = d["pickup_from"]
        if isinstance(p, bool) or not isinstance(p, int) or not (0 <= p < len(dests)) or p == i:
            raise ValueError(f"{name} must be the index of another entry of destination_points")
        other = dests[p]
        if isinstance(other, dict) and "pickup_from" in other:
            raise ValueError(f"{name} names an entry that itself carries pickup_from")
        if p in used:
            raise ValueError(f"{name} names an entry that is already the pickup of another delivery")
        if isinstance(other, dict) and "payload" in other and not _float(other["payload"], 0.0) == 0.0:
            raise ValueError(f"{name} names an entry with a payload of its own (a pickup's payload must be 0 or absent)")
        used.add(p)
        out[i + 1] = p + 1
    return out


def shipment_properties(schedule: Schedule, stats: Dict[str, int], close_q: Sequence[int], demand: Sequence[float],
                        pickup_from: Sequence[int]) -> Tuple[List[List[Dict[str, Any]]], Dict[str, Any], Dict[str, Any]]:
    """``(properties.schedule, properties.time_windows, properties.shipments)`` of a response: the
    time-window properties, every schedule entry with its ``type`` and the ``load`` on leaving it.
    With ``stats["search"]`` (the statistics of :mod:`routing.shipment_improve`) the second also
    reports the local search."""
    n1 = len(pickup_from)
    kind, mate = kinds_of(pickup_from, n1)
    qd = [0] + [quantize(demand[s]) for s in range(1, n1)]
    out, info = schedule_properties(schedule, {k: v for k, v in stats.items() if k != "search"}, close_q)
    search = stats.get("search")
    if search is not None:
        # the statistics of routing/shipment_improve.py: the schedule given here is the improved one
        info = {"method": info["method"] + "+unit_relocate", "stops_with_windows": info["stops_with_windows"],
                "trips": int(search["trips_after"]), "waiting": int(search["waiting_q"]) / 1000.0,
                "moves": int(search["moves"]), "pair_moves": int(search["pair_moves"]),
                "trips_before": int(search["trips_before"]),
                "matrix_distance_before": int(search["len_before_q"]) / 1000.0,
                "matrix_distance_after": int(search["len_after_q"]) / 1000.0}
    top = 0
    for rows, trip in zip(out, schedule):
        load = load_profile(qd, kind, mate, [0] + [s for s, _, _, _ in trip] + [0])
        top = max([top] + load)
        for x, (row, (s, _, _, _)) in enumerate(zip(rows, trip)):
            row["type"] = KIND_NAMES[kind[s]]
            row["load"] = load[x + 1] / 1000.0
    return out, info, {"pairs": sum(1 for k in kind if k == PICKUP), "max_load": top / 1000.0}


__all__ = ["PLAIN", "PICKUP", "DELIVERY", "NEEDS_MATRIX_TIMES", "kinds_of", "load_profile",
           "pd_load_feasible", "alone_infeasible", "candidate_tests", "best_insertion", "apply_insertion",
           "pd_trips", "wants_shipments", "parse_shipments", "shipment_properties"]
