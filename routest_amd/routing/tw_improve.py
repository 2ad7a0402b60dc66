"""Window-aware local search on the trips of a time-window request (relocate, swap) — CPU reference.

The cheapest insertion of :mod:`routing.timewindows` builds the trips of a time-window request one
after the other and never looks back.  :func:`tw_improve_trips` improves them by best-improvement
local search under the windows, the service times, the capacity and the distance limit.  It is
opt-in (``"tw_improve": true``).  The definition is schedule-independent, so this reference, the
host C++ (``rtr::tw_improve_trips``, ``csrc/runtime/route_core.h``) and the GPU kernel (K6e,
``csrc/route_tw_improve.hip``) return the same trips, schedule and statistics, compared with ``==``.

Fixed point as in :mod:`routing.timewindows`: ``q`` millimetres and ``qt`` milliseconds, both with
the unusable-entry rule (``>= 2**31 - 1`` is ``BIG``); ``qd``, ``cap_q``, ``max_q``, ``open_q``,
``close_q``, ``sv_q`` as there; all sums int64.  "usable(x, y)" means ``q(x,y) < BIG`` and
``qt(x,y) < BIG``.

Input: the trips of ``tw_trips``, all time-feasible.  State per trip by its original position (an
emptied trip keeps its index and is never a target): ``Lq[t]``, ``Wq[t]``, ``dep_t[0..k]`` and
``z_t[1..k]`` (the schedule and latest-start recurrences of ``timewindows.py``).

The stage is skipped (trips returned as given, 0 moves) with more than 128 stops, a stop with
``qd == BIG``, or ``cap_q < 0`` / ``max_q < 0``.

With ``a = trips[A]``, ``b = trips[B]``, ``kA`` / ``kB`` stops, ``p = a[i-1]``, ``s = a[i]``,
``n = a[i+1]``; a move is admissible only if every leg the new orders have and the old lack is
usable:

* type 0, relocate between trips, ``A != B``, ``kB >= 1``, ``1 <= i <= kA``, ``0 <= j <= kB``: ``s``
  goes between ``u = b[j]`` and ``v = b[j+1]``.  ``rem = q(p,s) + q(s,n) - q(p,n)`` (with
  ``kA == 1``: ``rem = q(0,s) + q(s,0)`` and ``A`` is emptied), ``ins = q(u,s) + q(s,v) - q(u,v)``,
  gain = ``rem - ins``.  Limits: ``Wq[B] + qd[s] <= cap_q``, ``Lq[B] + ins <= max_q``,
  ``Lq[A] - rem <= max_q``.  Time in ``B``: ``st = max(dep_B[j] + qt(u,s), open_s) <= close_s`` and
  (``j == kB`` or ``st + sv_s + qt(s,v) <= z_B[j+1]``).  Time in ``A``: ``kA == 1`` or ``i == kA`` or
  ``max(dep_A[i-1] + qt(p,n), open_n) <= z_A[i+1]`` (a seconds matrix need not obey the triangle
  inequality, so removing a stop can make the next one late);
* type 1, swap between trips, ``A < B``, ``1 <= i <= kA``, ``1 <= j <= kB``: ``s`` and ``u = b[j]``
  change places; ``dA``, ``dB``, gain and the load / length limits exactly as in
  :mod:`routing.exchange`.  Time in ``A``: ``su = max(dep_A[i-1] + qt(p,u), open_u) <= close_u`` and
  (``i == kA`` or ``su + sv_u + qt(u,n) <= z_A[i+1]``); time in ``B``: the same with ``s`` and ``u``
  exchanged;
* type 2, relocate inside a trip, ``B = A``, ``kA >= 2``, ``1 <= i <= kA``, ``0 <= j <= kA``, ``j``
  not in ``{i-1, i}``: ``s`` goes between ``a[j]`` and ``a[j+1]`` of the trip as it stands
  (``improve.py``'s Or-opt of length 1, the same gain).  Limit: ``Lq[A] - gain <= max_q``.  Time on
  the new order ``a'`` with ``m = min(i, j+1)`` and ``M = max(i, j)``: walk the positions ``m..M``
  from ``clock = dep_A[m-1]`` by the schedule recurrence, every ``start <= close``; then ``M == kA``
  or ``max(clock + qt(a'[M], a'[M+1]), open) <= z_A[M+1]`` (the suffix behind ``M`` is unchanged, so
  the old ``z`` holds).

The admissible move of largest gain is applied if that gain is > 0; among equal gains the smallest
``(type, A, i, B, j)`` wins.  After a move the touched non-empty trips are walked in float64 as the
greedy measures them (:func:`improve.walk_feasible`, :func:`exchange.load_feasible`); a failing
walk undoes the move and ends the search with ``rejected = 1``.  The search also ends at gain
``<= 0`` or after ``4 * ns`` moves.  ``Lq``, ``Wq``, ``dep`` and ``z`` of the touched trips are then
recomputed.  Empty trips are dropped from the output, the others keep their relative order.

Reversals (2-opt) and segments of 2-3 stops are out of scope: a reversal changes every arrival of
the reversed part, so it has no O(1) time test.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .exchange import UNBOUNDED, load_feasible
from .improve import BIG, quantize, walk_feasible
from .timewindows import MAX_STOPS, Schedule, latest_starts, limit_q, schedule_of, usable_matrix

METHOD = "cheapest_insertion+relocate+swap"
STAT_KEYS = ("moves", "rejected", "trips_before", "trips_after", "len_before_q", "len_after_q", "waiting_q")

Move = Tuple[int, int, int, int, int]            # (type, A, i, B, j)


def wants_tw_improve(payload) -> bool:
    """The request field: JSON ``true`` exactly; anything else is off."""
    return isinstance(payload, dict) and payload.get("tw_improve") is True


def moved_trips(trips: Sequence[Sequence[int]], move: Move) -> Dict[int, List[int]]:
    """The new orders of the trips that ``move`` touches, by trip index."""
    typ, A, i, B, j = move
    a = list(trips[A])
    if typ == 0:
        b = list(trips[B])
        s = a.pop(i)
        b.insert(j + 1, s)
        return {A: a, B: b}
    if typ == 1:
        b = list(trips[B])
        a[i], b[j] = b[j], a[i]
        return {A: a, B: b}
    s = a[i]
    if j < i - 1:
        return {A: a[:j + 1] + [s] + a[j + 1:i] + a[i + 1:]}
    return {A: a[:i] + a[i + 1:j + 1] + [s] + a[j + 1:]}


class _Search:
    """The state of one search: the quantized inputs and, per trip, Lq / Wq / dep / z."""

    def __init__(self, q, qt, qd, op, cl, sv, cap_q, max_q, trips):
        self.q, self.qt, self.qd, self.op, self.cl, self.sv = q, qt, qd, op, cl, sv
        self.cap_q, self.max_q = cap_q, max_q
        self.trips = trips
        m = len(trips)
        self.Lq, self.Wq, self.dep, self.z = [0] * m, [0] * m, [None] * m, [None] * m
        for t in range(m):
            self.refresh(t)

    def refresh(self, t: int) -> None:
        trip = self.trips[t]
        self.Lq[t] = int(sum(int(self.q[trip[p], trip[p + 1]]) for p in range(len(trip) - 1))) if len(trip) > 2 else 0
        self.Wq[t] = int(sum(int(self.qd[s]) for s in trip[1:-1]))
        if len(trip) > 2:
            self.dep[t] = schedule_of(self.qt, trip, self.op, self.cl, self.sv)[2]
            self.z[t] = latest_starts(self.qt, trip, self.cl, self.sv)
        else:
            self.dep[t], self.z[t] = [0], [0]

    def usable(self, x: int, y: int) -> bool:
        return int(self.q[x, y]) < BIG and int(self.qt[x, y]) < BIG

    # ---- one candidate: (gain, admissible apart from time, time verdict)
    def price(self, move: Move) -> Tuple[int, bool, bool]:
        typ, A, i, B, j = move
        q, qt, qd, op, cl, sv = self.q, self.qt, self.qd, self.op, self.cl, self.sv
        Q = lambda x, y: int(q[x, y])       # noqa: E731
        T = lambda x, y: int(qt[x, y])      # noqa: E731
        a = self.trips[A]
        kA = len(a) - 2
        p, s, n = a[i - 1], a[i], a[i + 1]
        depA, zA = self.dep[A], self.z[A]
        if typ == 0:
            b = self.trips[B]
            kB = len(b) - 2
            u, v = b[j], b[j + 1]
            rem = Q(0, s) + Q(s, 0) if kA == 1 else Q(p, s) + Q(s, n) - Q(p, n)
            ins = Q(u, s) + Q(s, v) - Q(u, v)
            ok = (kA == 1 or self.usable(p, n)) and self.usable(u, s) and self.usable(s, v)
            ok = ok and (self.Wq[B] + int(qd[s]) <= self.cap_q and self.Lq[B] + ins <= self.max_q
                         and self.Lq[A] - rem <= self.max_q)
            tok = T(u, s) < BIG and T(s, v) < BIG and (kA == 1 or T(p, n) < BIG)
            if tok:
                st = max(self.dep[B][j] + T(u, s), int(op[s]))
                tok = st <= int(cl[s]) and (j == kB or st + int(sv[s]) + T(s, v) <= self.z[B][j + 1])
                tok = tok and (kA == 1 or i == kA or max(depA[i - 1] + T(p, n), int(op[n])) <= zA[i + 1])
            return rem - ins, ok, tok
        if typ == 1:
            b = self.trips[B]
            kB = len(b) - 2
            u, pb, nb = b[j], b[j - 1], b[j + 1]
            dA = Q(p, u) + Q(u, n) - Q(p, s) - Q(s, n)
            dB = Q(pb, s) + Q(s, nb) - Q(pb, u) - Q(u, nb)
            wd = int(qd[u]) - int(qd[s])
            ok = self.usable(p, u) and self.usable(u, n) and self.usable(pb, s) and self.usable(s, nb)
            ok = ok and (self.Wq[A] + wd <= self.cap_q and self.Wq[B] - wd <= self.cap_q
                         and self.Lq[A] + dA <= self.max_q and self.Lq[B] + dB <= self.max_q)
            tok = max(T(p, u), T(u, n), T(pb, s), T(s, nb)) < BIG
            if tok:
                su = max(depA[i - 1] + T(p, u), int(op[u]))
                tok = su <= int(cl[u]) and (i == kA or su + int(sv[u]) + T(u, n) <= zA[i + 1])
                ss = max(self.dep[B][j - 1] + T(pb, s), int(op[s]))
                tok = tok and ss <= int(cl[s]) and (j == kB or ss + int(sv[s]) + T(s, nb) <= self.z[B][j + 1])
            return -(dA + dB), ok, tok
        u, v = a[j], a[j + 1]
        gain = Q(p, s) + Q(s, n) + Q(u, v) - Q(p, n) - Q(u, s) - Q(s, v)
        ok = self.usable(p, n) and self.usable(u, s) and self.usable(s, v) and self.Lq[A] - gain <= self.max_q
        tok = max(T(p, n), T(u, s), T(s, v)) < BIG
        if tok:
            new = moved_trips(self.trips, move)[A]
            lo, hi = min(i, j + 1), max(i, j)
            clock = depA[lo - 1]
            for x in range(lo, hi + 1):
                start = max(clock + T(new[x - 1], new[x]), int(op[new[x]]))
                if start > int(cl[new[x]]):
                    tok = False
                    break
                clock = start + int(sv[new[x]])
            if tok and hi < kA:
                tok = max(clock + T(new[hi], new[hi + 1]), int(op[new[hi + 1]])) <= zA[hi + 1]
        return gain, ok, tok

    def candidates(self):
        """Every move of the definition's ranges, in ``(type, A, i, B, j)`` order."""
        trips = self.trips
        m = len(trips)
        k = [len(t) - 2 for t in trips]
        for A in range(m):
            for i in range(1, k[A] + 1):
                for B in range(m):
                    if B != A and k[B] >= 1:
                        for j in range(k[B] + 1):
                            yield (0, A, i, B, j)
        for A in range(m):
            for i in range(1, k[A] + 1):
                for B in range(A + 1, m):
                    for j in range(1, k[B] + 1):
                        yield (1, A, i, B, j)
        for A in range(m):
            if k[A] >= 2:
                for i in range(1, k[A] + 1):
                    for j in range(k[A] + 1):
                        if j not in (i - 1, i):
                            yield (2, A, i, A, j)

    def gains(self):
        """The candidates with their gains, vectorized: ``(moves int64 [C, 5], gain int64 [C])`` in
        ``(type, A, i, B, j)`` order (the time and limit tests are left to :meth:`price`)."""
        q = self.q
        sA, sI, sS, sP, sN, sK = [], [], [], [], [], []
        eB, eJ, eU, eV = [], [], [], []
        for t, trip in enumerate(self.trips):
            k = len(trip) - 2
            for i in range(1, k + 1):
                sA.append(t); sI.append(i); sS.append(trip[i]); sP.append(trip[i - 1]); sN.append(trip[i + 1]); sK.append(k)
            if k >= 1:
                for j in range(k + 1):
                    eB.append(t); eJ.append(j); eU.append(trip[j]); eV.append(trip[j + 1])
        sA, sI, sS, sP, sN, sK = (np.array(v, dtype=np.int64) for v in (sA, sI, sS, sP, sN, sK))
        eB, eJ, eU, eV = (np.array(v, dtype=np.int64) for v in (eB, eJ, eU, eV))
        nb = q[sP, sS] + q[sS, sN]
        rem = nb - np.where(sK == 1, 0, q[sP, sN])
        ins = q[eU[None, :], sS[:, None]] + q[sS[:, None], eV[None, :]] - q[eU, eV][None, :]
        g = rem[:, None] - ins
        rows, cols = np.nonzero(sA[:, None] != eB[None, :])
        out = [(np.stack([np.zeros_like(rows), sA[rows], sI[rows], eB[cols], eJ[cols]], axis=1), g[rows, cols])]
        s, u = sS[:, None], sS[None, :]
        dA = q[sP[:, None], u] + q[u, sN[:, None]] - nb[:, None]
        dB = q[sP[None, :], s] + q[s, sN[None, :]] - nb[None, :]
        rows, cols = np.nonzero(sA[:, None] < sA[None, :])
        out.append((np.stack([np.ones_like(rows), sA[rows], sI[rows], sA[cols], sI[cols]], axis=1),
                    (-(dA + dB))[rows, cols]))
        same = ((sA[:, None] == eB[None, :]) & (eJ[None, :] != sI[:, None] - 1) & (eJ[None, :] != sI[:, None])
                & (sK[:, None] >= 2))
        rows, cols = np.nonzero(same)
        out.append((np.stack([np.full_like(rows, 2), sA[rows], sI[rows], eB[cols], eJ[cols]], axis=1), g[rows, cols]))
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    def best_move(self, trace: Optional[list]) -> Tuple[int, Optional[Move]]:
        if trace is not None:
            # the slow way, every candidate priced: the tests compare each time verdict
            best: Tuple[int, Optional[Move]] = (0, None)
            verdicts = []
            for mv in self.candidates():
                gain, ok, tok = self.price(mv)
                verdicts.append((mv, tok))
                if ok and tok and gain > best[0]:
                    best = (gain, mv)
            trace.append(([list(t) for t in self.trips], verdicts))
            return best
        moves, gain = self.gains()
        pos = np.flatnonzero(gain > 0)
        # descending gain, ties in (type, A, i, B, j) order (the candidates come in that order)
        for c in pos[np.argsort(-gain[pos], kind="stable")]:
            mv = tuple(int(v) for v in moves[c])
            g, ok, tok = self.price(mv)
            if ok and tok:
                return g, mv
        return 0, None


def tw_improve_trips(d, t, trips: Sequence[Sequence[int]], demand: Sequence[float], cap: float,
                     max_dist: float, open_q: Sequence[int], close_q: Sequence[int], sv_q: Sequence[int],
                     trace: Optional[list] = None, applied: Optional[list] = None
                     ) -> Tuple[List[List[int]], Schedule, Dict[str, int]]:
    """``d`` / ``t``, ``demand``, ``open_q``, ``close_q``, ``sv_q`` as :func:`timewindows.tw_trips`
    takes them; ``trips``: its trips.  Returns the new trips, their schedule (as ``tw_trips`` returns
    it) and ``{"moves", "rejected", "trips_before", "trips_after", "len_before_q", "len_after_q",
    "waiting_q"}``.  ``trace``: a list that receives ``(trips, [(move, time verdict)])`` with every
    candidate of the definition's ranges before each selection; ``applied``: a list that receives
    the ``(type, A, i, B, j)`` of every move that is kept (tests)."""
    dn = np.asarray(d, dtype=np.float64)
    tn = np.asarray(t, dtype=np.float64)
    n1 = dn.shape[0]
    ns = n1 - 1
    cap, max_dist = float(cap), float(max_dist)
    q, qt = usable_matrix(dn), usable_matrix(tn)
    qd = np.array([0] + [quantize(demand[s]) for s in range(1, n1)], dtype=np.int64)
    op = np.array([0] + [int(open_q[s]) for s in range(1, n1)], dtype=np.int64)
    cl = np.array([UNBOUNDED] + [int(close_q[s]) for s in range(1, n1)], dtype=np.int64)
    sv = np.array([0] + [int(sv_q[s]) for s in range(1, n1)], dtype=np.int64)
    cap_q, max_q = limit_q(cap), limit_q(max_dist)
    cur = [[int(v) for v in trip] for trip in trips]
    st = _Search(q, qt, qd, op, cl, sv, cap_q, max_q, cur)
    before = sum(st.Lq)
    stats = {"moves": 0, "rejected": 0, "trips_before": len(cur), "trips_after": len(cur),
             "len_before_q": before, "len_after_q": before, "waiting_q": 0}
    skip = ns > MAX_STOPS or bool((qd[1:] == BIG).any()) or cap_q < 0 or max_q < 0
    while not skip and stats["moves"] < 4 * ns:
        gain, mv = st.best_move(trace)
        if mv is None or gain <= 0:
            break
        new = moved_trips(cur, mv)
        if not all(len(o) == 2 or (walk_feasible(dn, o, max_dist) and load_feasible(demand, o, cap))
                   for o in new.values()):
            stats["rejected"] = 1
            break
        for x, o in new.items():
            cur[x] = o
            st.refresh(x)
        stats["moves"] += 1
        if applied is not None:
            applied.append(mv)
    out = [trip for trip in cur if len(trip) > 2]
    schedule: Schedule = []
    for trip in out:
        arr, start, dep, _ = schedule_of(qt, trip, op, cl, sv)
        k = len(trip) - 2
        schedule.append([(trip[i], arr[i], start[i], dep[i]) for i in range(1, k + 1)])
        stats["waiting_q"] += sum(start[i] - arr[i] for i in range(1, k + 1))
    stats["trips_after"] = len(out)
    stats["len_after_q"] = sum(st.Lq[x] for x, trip in enumerate(cur) if len(trip) > 2)
    return out, schedule, stats
