"""Intra-trip 2-opt / Or-opt improvement of the greedy's trips — CPU reference.

The greedy (:mod:`routing.greedy`) visits each trip's stops in order of distance from the depot.
:func:`improve_trips` re-sequences every trip by best-improvement local search; stops never change
trips, so capacity is untouched.  The definition is schedule-independent, so this reference, the
host C++ (``rtr::improve_trips``, ``csrc/runtime/route_core.h``) and the GPU kernel (K6b,
``csrc/route_improve.hip``) return the same trips and statistics, compared with ``==``.

Distances are fixed point.  For a float64 matrix entry ``x``, ``q(x)`` is ``BIG = 2**50`` if
``not (x >= 0) or x >= 2**40`` (NaN, +-inf, negatives), else ``int(rint(x * 1000.0))``: millimetres,
round-half-even.  All search arithmetic is int64 on ``q``.

A trip is ``t[0..k+1]`` with ``t[0] = t[k+1] = 0`` and stops at positions ``1..k``;
``L = sum q(t[p], t[p+1])``.  Moves (every positive gain equals the decrease of ``L``):

* type 0, reversal (asymmetric 2-opt), ``1 <= i < j <= k``: reverse ``t[i..j]``;
  gain = ``[q(t[i-1],t[i]) + q(t[j],t[j+1]) + fwd(i,j)] - [q(t[i-1],t[j]) + q(t[i],t[j+1]) + bwd(i,j)]``
  with ``fwd(i,j) = sum_{p=i}^{j-1} q(t[p],t[p+1])`` and ``bwd(i,j) = sum_{p=i}^{j-1} q(t[p+1],t[p])``;
* types 1, 2, 3, Or-opt of a segment ``t[i..e]`` of that length (``e = i + len - 1 <= k``),
  orientation kept, moved between ``t[j]`` and ``t[j+1]`` for ``j`` in ``0..k`` outside ``i-1..e``;
  gain = ``q(t[i-1],t[i]) + q(t[e],t[e+1]) + q(t[j],t[j+1]) - q(t[i-1],t[e+1]) - q(t[j],t[i]) - q(t[e],t[j+1])``.

The move of largest gain is applied if that gain is > 0; among equal gains the smallest
``(type, i, j)`` wins.  Repeat until no move has positive gain or ``4k`` moves were applied (``L``
strictly decreases, so the loop ends without the cap; the cap bounds the kernel's worst case and
keeps what was reached).  Trips with ``k > 128`` or ``k < 2`` are left as the greedy built them.

Feasibility as the greedy measures it: the new order is walked in float64 exactly like the greedy
accumulates (``s = 0; s += d[t[p]][t[p+1]]`` for ``p = 0..k-1``) and kept iff
``s + d[t[k]][0] <= max_dist``; otherwise the greedy's order is restored for that trip (rounding to
mm can make a trip that is shorter in ``q`` a few mm longer in float64).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

BIG = 1 << 50
Q_LIMIT = float(1 << 40)
MAX_STOPS = 128
METHOD = "2opt+oropt"


def quantize(x: float) -> int:
    """q(x): millimetres, round-half-even; BIG for NaN, +-inf, negatives and x >= 2**40."""
    x = float(x)
    if not (x >= 0.0) or x >= Q_LIMIT:
        return BIG
    return int(np.rint(x * 1000.0))


def quantize_matrix(d: np.ndarray) -> np.ndarray:
    d = np.asarray(d, dtype=np.float64)
    bad = ~(d >= 0.0) | (d >= Q_LIMIT)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(np.where(bad, 0.0, d) * 1000.0).astype(np.int64)
    q[bad] = BIG
    return q


def trip_length_q(q: np.ndarray, trip: Sequence[int]) -> int:
    return int(sum(int(q[trip[p], trip[p + 1]]) for p in range(len(trip) - 1)))


def best_move(q: np.ndarray, t: Sequence[int]) -> Tuple[int, int, int, int]:
    """(gain, type, i, j) of the best-improvement move on trip ``t``, or (0, -1, -1, -1)."""
    k = len(t) - 2
    P = q[np.ix_(t, t)]                       # P[a][b] = q(t[a], t[b]), positions 0..k+1
    f = P[np.arange(k + 1), np.arange(1, k + 2)]      # f[p] = q(t[p], t[p+1])
    b = P[np.arange(1, k + 2), np.arange(k + 1)]      # b[p] = q(t[p+1], t[p])
    pf = np.concatenate([[0], np.cumsum(f)])          # fwd(i, j) = pf[j] - pf[i]
    pb = np.concatenate([[0], np.cumsum(b)])
    best = (0, -1, -1, -1)
    # type 0: reversal of t[i..j]
    i = np.arange(1, k + 1)[:, None]
    j = np.arange(1, k + 1)[None, :]
    g = (f[i - 1] + f[j] + (pf[j] - pf[i])) - (P[i - 1, j] + P[i, j + 1] + (pb[j] - pb[i]))
    g = np.where(i < j, g, -1)
    c = int(np.argmax(g))                     # first maximum in (i, j) order
    if int(g.flat[c]) > best[0]:
        best = (int(g.flat[c]), 0, 1 + c // k, 1 + c % k)
    # types 1..3: Or-opt of t[i..e] to between t[j] and t[j+1]
    for ln in (1, 2, 3):
        if k - ln + 1 < 1:
            break
        i = np.arange(1, k - ln + 2)[:, None]
        e = i + ln - 1
        j = np.arange(0, k + 1)[None, :]
        g = f[i - 1] + f[e] + f[j] - P[i - 1, e + 1] - P[j, i] - P[e, j + 1]
        g = np.where((j < i - 1) | (j > e), g, -1)
        c = int(np.argmax(g))
        if int(g.flat[c]) > best[0]:
            best = (int(g.flat[c]), ln, 1 + c // (k + 1), c % (k + 1))
    return best


def apply_move(t: List[int], typ: int, i: int, j: int) -> List[int]:
    if typ == 0:
        return t[:i] + t[i:j + 1][::-1] + t[j + 1:]
    e = i + typ - 1
    seg = t[i:e + 1]
    if j < i - 1:
        return t[:j + 1] + seg + t[j + 1:i] + t[e + 1:]
    return t[:i] + t[e + 1:j + 1] + seg + t[j + 1:]


def search_trip(q: np.ndarray, trip: Sequence[int]) -> Tuple[List[int], int]:
    """Best-improvement search on one trip: (new trip, moves applied)."""
    t = list(trip)
    k = len(t) - 2
    moves = 0
    while moves < 4 * k:
        gain, typ, i, j = best_move(q, t)
        if gain <= 0:
            break
        t = apply_move(t, typ, i, j)
        moves += 1
    return t, moves


def walk_feasible(d, t: Sequence[int], max_dist: float) -> bool:
    """The greedy's own float64 accumulation over the order ``t``."""
    k = len(t) - 2
    s = 0.0
    for p in range(k):
        s += float(d[t[p]][t[p + 1]])
    return bool(s + float(d[t[k]][0]) <= max_dist)


def improve_trips(d, trips: Sequence[Sequence[int]], max_dist: float
                  ) -> Tuple[List[List[int]], Dict[str, int]]:
    """``d``: (N+1)x(N+1) float64 matrix over [depot] + stops; ``trips``: the greedy's trips.
    Returns the re-sequenced trips and ``{"moves", "trips_changed", "len_before_q", "len_after_q"}``."""
    dn = np.asarray(d, dtype=np.float64)
    q = quantize_matrix(dn)
    out: List[List[int]] = []
    stats = {"moves": 0, "trips_changed": 0, "len_before_q": 0, "len_after_q": 0}
    for trip in trips:
        trip = [int(v) for v in trip]
        k = len(trip) - 2
        before = trip_length_q(q, trip)
        stats["len_before_q"] += before
        new, moves = (trip, 0) if (k < 2 or k > MAX_STOPS) else search_trip(q, trip)
        if moves and walk_feasible(dn, new, float(max_dist)):
            stats["moves"] += moves
            stats["trips_changed"] += 1
            stats["len_after_q"] += trip_length_q(q, new)
            out.append(new)
        else:
            stats["len_after_q"] += before
            out.append(trip)
    return out, stats


def improvement_properties(stats: Dict[str, int]) -> Dict[str, object]:
    """``properties.improvement`` of a response, from the statistics of :func:`improve_trips`, or
    from the composed statistics of an ``exchange`` request (:mod:`routing.exchange`)."""
    if "exchange_moves" in stats:
        return {"method": METHOD + "+exchange", "moves": int(stats["moves"]),
                "exchange_moves": int(stats["exchange_moves"]),
                "trips_before": int(stats["trips_before"]), "trips_after": int(stats["trips_after"]),
                "matrix_distance_before": int(stats["len_before_q"]) / 1000.0,
                "matrix_distance_after": int(stats["len_after_q"]) / 1000.0}
    return {"method": METHOD, "moves": int(stats["moves"]),
            "trips_changed": int(stats["trips_changed"]),
            "matrix_distance_before": int(stats["len_before_q"]) / 1000.0,
            "matrix_distance_after": int(stats["len_after_q"]) / 1000.0}


def wants_improve(payload) -> bool:
    """The request field: JSON ``true`` exactly; anything else is off."""
    return isinstance(payload, dict) and payload.get("improve") is True
