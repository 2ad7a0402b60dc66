"""Inter-trip relocate / swap improvement of the greedy's trips — CPU reference.

The greedy (:mod:`routing.greedy`) fills one trip after the other in order of distance from the
depot, so neighbouring stops end up in different trips, and :mod:`routing.improve` only re-sequences
stops inside a trip.  :func:`exchange_trips` moves single stops between trips by best-improvement
local search under the capacity and the distance limit.  The definition is schedule-independent,
so this reference, the host C++ (``rtr::exchange_trips``, ``csrc/runtime/route_core.h``) and the GPU
kernel (K6c, ``csrc/route_exchange.hip``) return the same trips and statistics, compared with ``==``.

Fixed point as in :mod:`routing.improve` (``q``: millimetres, ``BIG`` for unusable entries).
``qd[s] = quantize(demand[s])``; ``cap_q = floor(cap * 1000)`` for ``0 <= cap < 2**40`` and
``UNBOUNDED = 2**62`` for ``cap >= 2**40``; ``max_q`` likewise from ``max_dist``.

The stage is skipped (trips returned as given, 0 moves) when there are more than 128 stops, fewer
than 2 non-empty trips, a stop with ``qd[s] == BIG``, or a NaN / negative ``cap`` / ``max_dist``.

State by the trips' original positions ``0..m-1`` (an emptied trip keeps its index and is never an
insertion target): ``Lq[t]`` the trip's length in ``q``, ``Wq[t]`` the sum of ``qd`` over its stops.
With ``a = trips[A]``, ``b = trips[B]``, ``kA`` / ``kB`` stop counts, positions as in ``improve.py``:

* type 0, relocate, ``A != B``, ``kB >= 1``, ``1 <= i <= kA``, ``0 <= j <= kB``: ``s = a[i]`` leaves
  ``A`` and goes between ``b[j]`` and ``b[j+1]``;
  ``rem = q(a[i-1],s) + q(s,a[i+1]) - q(a[i-1],a[i+1])``,
  ``ins = q(b[j],s) + q(s,b[j+1]) - q(b[j],b[j+1])``, gain = ``rem - ins``; admissible iff
  ``Wq[B] + qd[s] <= cap_q``, ``Lq[B] + ins <= max_q`` and ``Lq[A] - rem <= max_q`` (a road matrix
  need not obey the triangle inequality, so the source trip may grow);
* type 1, swap, ``A < B``, ``1 <= i <= kA``, ``1 <= j <= kB``: ``s = a[i]`` and ``u = b[j]`` change
  places; ``dA = q(a[i-1],u) + q(u,a[i+1]) - q(a[i-1],s) - q(s,a[i+1])``, ``dB`` the same in ``b``
  with ``s`` and ``u`` exchanged, gain = ``-(dA + dB)``; admissible iff both loads stay
  ``<= cap_q``, ``Lq[A] + dA <= max_q`` and ``Lq[B] + dB <= max_q``.

The admissible move of largest gain is applied if that gain is > 0; among equal gains the smallest
``(type, A, i, B, j)`` wins.  After each move the two touched trips are walked in float64 as the
greedy measures them (:func:`improve.walk_feasible`, and ``load += demand[stop]`` in visiting order
against ``cap``); if either fails, the move is undone and the search ends with ``rejected = 1``,
keeping what was reached.  The search also ends when no admissible move has positive gain or after
``move_cap`` moves (default ``4 * ns``).  Empty trips are dropped from the output, the others keep
their relative order; trips are never created.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .improve import BIG, Q_LIMIT, improve_trips, quantize, quantize_matrix, trip_length_q, walk_feasible

UNBOUNDED = 1 << 62
MAX_STOPS = 128
METHOD = "2opt+oropt+exchange"


def quantize_limit(x: float) -> Optional[int]:
    """``cap_q`` / ``max_q``: None for NaN and negatives (the stage is skipped)."""
    x = float(x)
    if not (x >= 0.0):
        return None
    if x >= Q_LIMIT:
        return UNBOUNDED
    return int(math.floor(x * 1000.0))


def load_feasible(demand, t: Sequence[int], cap: float) -> bool:
    """The greedy's own float64 accumulation of the load over the order ``t``."""
    load = 0.0
    for s in t[1:-1]:
        load += float(demand[s])
    return bool(load <= cap)


def best_move(q: np.ndarray, qd: np.ndarray, trips: Sequence[Sequence[int]], Lq: Sequence[int],
              Wq: Sequence[int], cap_q: int, max_q: int) -> Tuple[int, int, int, int, int, int]:
    """(gain, type, A, i, B, j) of the best admissible move, or (0, -1, -1, -1, -1, -1)."""
    # stops in (A, i) order with their neighbours; insertion edges in (B, j) order
    sA, sI, sS, sP, sN = [], [], [], [], []
    eB, eJ, eU, eV = [], [], [], []
    for t, trip in enumerate(trips):
        k = len(trip) - 2
        if k < 1:
            continue
        for i in range(1, k + 1):
            sA.append(t); sI.append(i); sS.append(trip[i]); sP.append(trip[i - 1]); sN.append(trip[i + 1])
        for j in range(0, k + 1):
            eB.append(t); eJ.append(j); eU.append(trip[j]); eV.append(trip[j + 1])
    sA, sI, sS, sP, sN = (np.array(v, dtype=np.int64) for v in (sA, sI, sS, sP, sN))
    eB, eJ, eU, eV = (np.array(v, dtype=np.int64) for v in (eB, eJ, eU, eV))
    L = np.array([int(v) for v in Lq], dtype=np.int64)
    W = np.array([int(v) for v in Wq], dtype=np.int64)
    best = (0, -1, -1, -1, -1, -1)
    # type 0: relocate the stop of row p to the edge of column e
    rem = q[sP, sS] + q[sS, sN] - q[sP, sN]
    ins = q[eU[None, :], sS[:, None]] + q[sS[:, None], eV[None, :]] - q[eU, eV][None, :]
    g = rem[:, None] - ins
    ok = ((sA[:, None] != eB[None, :]) & (W[eB][None, :] + qd[sS][:, None] <= cap_q)
          & (L[eB][None, :] + ins <= max_q) & ((L[sA] - rem)[:, None] <= max_q))
    g = np.where(ok, g, -1)
    if g.size:
        c = int(np.argmax(g))                 # first maximum in (A, i, B, j) order
        if int(g.flat[c]) > best[0]:
            p, e = divmod(c, g.shape[1])
            best = (int(g.flat[c]), 0, int(sA[p]), int(sI[p]), int(eB[e]), int(eJ[e]))
    # type 1: swap the stop of row p with the stop of column c
    s, u = sS[:, None], sS[None, :]
    dA = q[sP[:, None], u] + q[u, sN[:, None]] - (q[sP, sS] + q[sS, sN])[:, None]
    dB = q[sP[None, :], s] + q[s, sN[None, :]] - (q[sP, sS] + q[sS, sN])[None, :]
    g = -(dA + dB)
    wd = qd[sS][None, :] - qd[sS][:, None]    # what trip A's load gains
    ok = ((sA[:, None] < sA[None, :]) & (W[sA][:, None] + wd <= cap_q) & (W[sA][None, :] - wd <= cap_q)
          & (L[sA][:, None] + dA <= max_q) & (L[sA][None, :] + dB <= max_q))
    g = np.where(ok, g, -1)
    if g.size:
        c = int(np.argmax(g))
        if int(g.flat[c]) > best[0]:
            p, e = divmod(c, g.shape[1])
            best = (int(g.flat[c]), 1, int(sA[p]), int(sI[p]), int(sA[e]), int(sI[e]))
    return best


def apply_move(trips: List[List[int]], typ: int, A: int, i: int, B: int, j: int) -> None:
    a, b = trips[A], trips[B]
    if typ == 0:
        s = a.pop(i)
        b.insert(j + 1, s)
    else:
        a[i], b[j] = b[j], a[i]


def exchange_trips(d, trips: Sequence[Sequence[int]], demand: Sequence[float], cap: float,
                   max_dist: float, move_cap: Optional[int] = None
                   ) -> Tuple[List[List[int]], Dict[str, int]]:
    """``d``: (ns+1)x(ns+1) float64 matrix over [depot] + stops; ``trips``: trips ``[0, ..., 0]`` over
    the stops; ``demand[s]`` per point (``demand[0]`` ignored).  Returns the new trips and
    ``{"moves", "rejected", "trips_before", "trips_after", "len_before_q", "len_after_q"}``."""
    dn = np.asarray(d, dtype=np.float64)
    q = quantize_matrix(dn)
    ns = dn.shape[0] - 1
    cur = [[int(v) for v in t] for t in trips]
    before = sum(trip_length_q(q, t) for t in cur)
    stats = {"moves": 0, "rejected": 0, "trips_before": len(cur), "trips_after": len(cur),
             "len_before_q": before, "len_after_q": before}
    qd = np.array([0] + [quantize(demand[s]) for s in range(1, ns + 1)], dtype=np.int64)
    cap_q, max_q = quantize_limit(cap), quantize_limit(max_dist)
    if (ns > MAX_STOPS or sum(1 for t in cur if len(t) > 2) < 2 or bool((qd[1:] == BIG).any())
            or cap_q is None or max_q is None):
        return cur, stats
    Lq = [trip_length_q(q, t) for t in cur]
    Wq = [int(sum(int(qd[s]) for s in t[1:-1])) for t in cur]
    limit = 4 * ns if move_cap is None else int(move_cap)
    while stats["moves"] < limit:
        gain, typ, A, i, B, j = best_move(q, qd, cur, Lq, Wq, cap_q, max_q)
        if gain <= 0:
            break
        saved = (list(cur[A]), list(cur[B]))
        apply_move(cur, typ, A, i, B, j)
        if not all(walk_feasible(dn, cur[t], float(max_dist)) and load_feasible(demand, cur[t], float(cap))
                   for t in (A, B)):
            cur[A], cur[B] = saved
            stats["rejected"] = 1
            break
        for t in (A, B):
            Lq[t] = trip_length_q(q, cur[t])
            Wq[t] = int(sum(int(qd[s]) for s in cur[t][1:-1]))
        stats["moves"] += 1
    out = [t for t in cur if len(t) > 2]
    stats["trips_after"] = len(out)
    stats["len_after_q"] = sum(trip_length_q(q, t) for t in out)
    return out, stats


def improve_exchange_trips(d, trips: Sequence[Sequence[int]], demand: Sequence[float], cap: float,
                           max_dist: float) -> Tuple[List[List[int]], Dict[str, int]]:
    """The pipeline of an ``"exchange": true`` request on the greedy's trips: intra-trip improvement,
    the exchange, intra-trip improvement again.  Returns the trips and ``{"moves" (both intra
    stages), "exchange_moves", "trips_before", "trips_after", "len_before_q", "len_after_q"}``."""
    t1, s1 = improve_trips(d, trips, max_dist)
    t2, s2 = exchange_trips(d, t1, demand, cap, max_dist)
    t3, s3 = improve_trips(d, t2, max_dist)
    return t3, compose_stats(s1, s2, s3)


def compose_stats(s1: Dict[str, int], s2: Dict[str, int], s3: Dict[str, int]) -> Dict[str, int]:
    return {"moves": int(s1["moves"]) + int(s3["moves"]), "exchange_moves": int(s2["moves"]),
            "trips_before": int(s2["trips_before"]), "trips_after": int(s2["trips_after"]),
            "len_before_q": int(s1["len_before_q"]), "len_after_q": int(s3["len_after_q"])}


def wants_exchange(payload) -> bool:
    """The request field: JSON ``true`` exactly; anything else is off."""
    return isinstance(payload, dict) and payload.get("exchange") is True
