"""Unit-relocate local search on the trips of a shipment request — CPU reference.

The cheapest insertion of :mod:`routing.shipments` builds the trips of a shipment request one after
the other and never looks back.  :func:`pd_improve_trips` improves them by best-improvement local
search whose only move takes a whole *unit* (a plain stop, or a pickup -> delivery pair) out of its
trip and puts it back at its cheapest admissible place, in another trip or in its own.  It is opt-in
(``"shipment_improve": true``).  The definition is schedule-independent, so this reference, the host
C++ (``rtr::pd_improve_trips``, ``csrc/runtime/route_core.h``) and the GPU kernel (K6g,
``csrc/route_pd_improve.hip``) return the same trips, schedule and statistics, compared with ``==``.

Carried over from :mod:`routing.shipments`, unchanged: ``q``, ``qt``, ``qd``, ``kind``, ``mate``,
``amt``; ``open_q`` / ``close_q`` / ``sv_q``, ``cap_q`` / ``max_q``, the unusable-entry rule, int64
sums.  Input: the trips of ``pd_trips`` (every stop once, a pair in one trip with its pickup first,
every trip time-feasible over usable legs; the construction guarantees the last).

A unit of trip ``A`` is named by the position ``x`` of its plain stop or its pickup.  The
millimetre length of a trip is the sum of ``q`` over its legs, 0 for the empty trip ``[0, 0]``.  A
trip is *integer-feasible* if it is empty or

* every consecutive leg is usable in both ``q`` and ``qt``;
* ``schedule_of`` is feasible;
* ``max(load_profile) <= cap_q``;
* its millimetre length is ``<= max_q``.

A move ``(type, A, x, B, i, j)`` removes the unit at ``x`` from ``A``, giving ``A'``, and reinserts
it with ``apply_insertion(target, mate, kind, u, i, j)``, K6f's position convention:
``0 <= i <= j <= k_target``, a plain unit has ``j == i``.

* type 0: the unit goes to another trip; ``B != A``, ``B`` is non-empty, the target is ``B``;
* type 1: the unit is moved inside its trip; ``B == A``, the target is ``A'``, which must be
  non-empty.

A move is admissible iff the resulting trips (type 0: ``A'`` and the new ``B``; type 1: the new
``A``) are integer-feasible.  Its gain is the millimetre length of the touched trips before minus
after.  The admissible move of largest gain is applied if that gain is > 0; among equal gains the
smallest ``(type, A, x, B, i, j)`` wins.  The touched non-empty trips are then walked in float64
(``walk_feasible`` against ``max_dist``, ``pd_load_feasible`` against ``cap``); a failing walk undoes
the move and ends the search with ``rejected = 1``.  The search also ends after ``4 * ns`` moves.
An emptied trip keeps its index during the search and is never a target; it is dropped from the
output, the others keep their order.

The stage is skipped (trips returned as given, 0 moves) with more than 128 stops, ``cap_q < 0`` or
``max_q < 0``, or a plain stop or a delivery with ``qd == BIG``.

Fast tests (:func:`candidate_tests`; what the host C++ and K6g evaluate; the tests compare them with
the re-simulation above candidate by candidate).  Per trip the search keeps ``Lq``, ``dep``, ``z``,
``load`` and ``sound``: its legs usable, its schedule feasible and ``max(load) <= cap_q``.

* The gain is O(1): ``rem - ins``.  ``rem = Lq[A] - length(A')`` is a per-unit term; ``ins`` is K6f's
  bracket sum on the target's legs (on ``A'`` for type 1, where the brackets of the removed unit
  and of the inserted one may share a cancelled leg: int64 sums cancel exactly).
* Removal (type 0): ``A'`` is walked once per unit (seconds need not obey the triangle inequality,
  so removing a stop can make a later one late; loads only fall, lengths are tested as
  ``Lq[A] - rem <= max_q``).
* Target of type 0: ``sound[B]`` and K6f's candidate tests on ``B`` (``shipments.candidate_tests``:
  O(1) time tests against ``dep`` / ``z``, the departures behind the pickup and the running load
  maximum carried forward over ``j``).  Insertion never lowers a load and the old ``z`` presumes the
  stops behind it were in time, hence ``sound[B]``; ``Lq[B] + ins <= max_q`` is exact by itself.
* Target of type 1: ``A'`` has per-unit state, so the gain is priced first and the new order is
  walked only for a candidate that would replace the best one found so far, with
  ``Lq[A] - gain <= max_q``.  K6g's walk (:func:`inside_walk`) is bounded: in a sound trip it
  starts behind the last position in front of every change from the old ``dep`` / ``load``, ends at
  the first failure, and at the first stop behind every change the old ``z`` decides; an unsound
  trip is walked in full.  The host C++ walks the whole new order, which is the definition itself.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .exchange import UNBOUNDED
from .improve import BIG, quantize, walk_feasible
from .shipments import (PICKUP, PLAIN, DELIVERY, apply_insertion, candidate_tests as insertion_tests,
                        kinds_of, load_profile, pd_load_feasible)
from .timewindows import MAX_STOPS, Schedule, latest_starts, limit_q, schedule_of, usable_matrix

METHOD = "cheapest_insertion+unit_relocate"
STAT_KEYS = ("moves", "pair_moves", "rejected", "trips_before", "trips_after", "len_before_q", "len_after_q",
             "waiting_q")

Move = Tuple[int, int, int, int, int, int]       # (type, A, x, B, i, j)


def wants_shipment_improve(payload) -> bool:
    """The request field: JSON ``true`` exactly; anything else is off."""
    return isinstance(payload, dict) and payload.get("shipment_improve") is True


def move_code(move: Move) -> int:
    """The move as one integer that orders like the tuple (six 8-bit fields below the type)."""
    typ, A, x, B, i, j = move
    return (typ << 40) | (A << 32) | (x << 24) | (B << 16) | (i << 8) | j


def remove_unit(trip: Sequence[int], kind, mate, x: int) -> List[int]:
    """``A'``: the trip without the unit whose plain stop or pickup is at position ``x``."""
    u = trip[x]
    if kind[u] == PLAIN:
        return list(trip[:x]) + list(trip[x + 1:])
    v = mate[u]
    return [s for p, s in enumerate(trip) if not (0 < p < len(trip) - 1 and s in (u, v))]


def moved_trips(trips: Sequence[Sequence[int]], kind, mate, move: Move) -> Dict[int, List[int]]:
    """The new orders of the trips that ``move`` touches, by trip index."""
    typ, A, x, B, i, j = move
    u = trips[A][x]
    rest = remove_unit(trips[A], kind, mate, x)
    if typ == 0:
        return {A: rest, B: apply_insertion(trips[B], mate, kind, u, i, j)}
    return {A: apply_insertion(rest, mate, kind, u, i, j)}


class _Search:
    """The state of one search: the quantized inputs and, per trip, Lq / dep / z / load / sound."""

    def __init__(self, q, qt, qd, kind, mate, op, cl, sv, cap_q, max_q, trips):
        self.q, self.qt, self.qd, self.kind, self.mate = q, qt, qd, kind, mate
        self.op, self.cl, self.sv, self.cap_q, self.max_q = op, cl, sv, cap_q, max_q
        self.trips = trips
        m = len(trips)
        self.Lq, self.dep, self.z, self.load, self.sound = [0] * m, [None] * m, [None] * m, [None] * m, [True] * m
        self._rem: Dict[Tuple[int, int], Tuple[List[int], int, bool]] = {}
        for t in range(m):
            self.refresh(t)

    # ---- the definition's terms
    def length(self, trip: Sequence[int]) -> int:
        if len(trip) <= 2:
            return 0
        return int(sum(int(self.q[trip[p], trip[p + 1]]) for p in range(len(trip) - 1)))

    def trip_sound(self, trip: Sequence[int]) -> bool:
        """Legs usable, schedule feasible, load within ``cap_q`` (all but the length test)."""
        if len(trip) <= 2:
            return True
        if any(int(self.q[trip[p], trip[p + 1]]) >= BIG or int(self.qt[trip[p], trip[p + 1]]) >= BIG
               for p in range(len(trip) - 1)):
            return False
        if not schedule_of(self.qt, trip, self.op, self.cl, self.sv)[3]:
            return False
        return max(load_profile(self.qd, self.kind, self.mate, trip)) <= self.cap_q

    def feasible(self, trip: Sequence[int]) -> bool:
        return len(trip) <= 2 or (self.trip_sound(trip) and self.length(trip) <= self.max_q)

    def refresh(self, t: int) -> None:
        trip = self.trips[t]
        self._rem.clear()
        self.Lq[t] = self.length(trip)
        if len(trip) > 2:
            self.dep[t] = schedule_of(self.qt, trip, self.op, self.cl, self.sv)[2]
            self.z[t] = latest_starts(self.qt, trip, self.cl, self.sv)
            self.load[t] = load_profile(self.qd, self.kind, self.mate, trip)
            self.sound[t] = self.trip_sound(trip)
        else:
            self.dep[t], self.z[t], self.load[t], self.sound[t] = [0], [0], [0], True

    def removal(self, A: int, x: int) -> Tuple[List[int], int, bool]:
        """``(A', rem, A' is integer-feasible)`` of the unit at ``x`` of trip ``A`` (one walk of ``A'``)."""
        got = self._rem.get((A, x))
        if got is None:
            rest = remove_unit(self.trips[A], self.kind, self.mate, x)
            rem = self.Lq[A] - self.length(rest)
            got = (rest, rem, self.trip_sound(rest) and self.Lq[A] - rem <= self.max_q)
            self._rem[(A, x)] = got
        return got

    # ---- one candidate, twice
    def define(self, move: Move) -> Tuple[int, bool]:
        """``(gain, admissible)`` by re-simulation of the touched trips: the definition."""
        new = moved_trips(self.trips, self.kind, self.mate, move)
        before = sum(self.length(self.trips[t]) for t in new)
        after = sum(self.length(o) for o in new.values())
        return before - after, all(self.feasible(o) for o in new.values())

    def fast(self, move: Move) -> Tuple[int, bool]:
        """``(gain, admissible)`` by the fast tests (see the module)."""
        gain, tests = candidate_tests(self, move)
        return gain, all(tests.values())

    def units(self):
        """``(A, x, u)`` of every unit, in ``(A, x)`` order."""
        for A, trip in enumerate(self.trips):
            for x in range(1, len(trip) - 1):
                if self.kind[trip[x]] != DELIVERY:
                    yield A, x, trip[x]

    def candidates(self):
        """Every move of the definition's ranges, in ``(type, A, x, B, i, j)`` order."""
        trips, kind = self.trips, self.kind
        for typ in (0, 1):
            for A, x, u in self.units():
                size = 1 if kind[u] == PLAIN else 2
                targets = ([B for B in range(len(trips)) if B != A and len(trips[B]) > 2] if typ == 0
                           else ([A] if len(trips[A]) - 2 - size >= 1 else []))
                for B in targets:
                    k = len(trips[B]) - 2 - (size if typ == 1 else 0)
                    for i in range(k + 1):
                        for j in (range(i, k + 1) if size == 2 else (i,)):
                            yield (typ, A, x, B, i, j)

    def ins_table(self, trip: Sequence[int], u: int):
        """``(i, j, ins)`` int64 vectors over the positions of unit ``u`` in the target ``trip``."""
        q = self.q
        a = np.asarray(trip[:-1], dtype=np.int64)
        b = np.asarray(trip[1:], dtype=np.int64)
        qab = q[a, b]
        pos = np.arange(a.size, dtype=np.int64)
        if self.kind[u] == PLAIN:
            return pos, pos, q[a, u] + q[u, b] - qab
        v = self.mate[u]
        same = q[a, u] + int(q[u, v]) + q[v, b] - qab
        ins1 = q[a, u] + q[u, b] - qab
        ins2 = q[a, v] + q[v, b] - qab
        I, J = np.triu_indices(a.size, 1)
        return np.concatenate([pos, I]), np.concatenate([pos, J]), np.concatenate([same, ins1[I] + ins2[J]])

    def gains(self):
        """``(code, gain)`` int64 vectors of every candidate, priced in bulk (no admissibility)."""
        codes, gains = [], []
        for A, x, u in self.units():
            rest, rem, _ = self.removal(A, x)
            targets = [(0, B, self.trips[B]) for B in range(len(self.trips)) if B != A and len(self.trips[B]) > 2]
            if len(rest) > 2:
                targets.append((1, A, rest))
            for typ, B, trip in targets:
                i, j, ins = self.ins_table(trip, u)
                codes.append((typ << 40) | (A << 32) | (x << 24) | (B << 16) | (i << 8) | j)
                gains.append(rem - ins)
        if not codes:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return np.concatenate(codes), np.concatenate(gains)

    def best_move(self, trace: Optional[list]) -> Tuple[int, Optional[Move]]:
        if trace is not None:
            # the slow way, every candidate priced and tested both ways: the tests compare them
            best: Tuple[int, Optional[Move]] = (0, None)
            seen = []
            for mv in self.candidates():
                gain, tests = candidate_tests(self, mv)
                seen.append((mv, gain, tests) + self.define(mv))
                if all(tests.values()) and gain > best[0]:
                    best = (gain, mv)
            trace.append(([list(t) for t in self.trips], seen))
            return best
        code, gain = self.gains()
        pos = np.flatnonzero(gain > 0)
        # descending gain, ties in code order
        for c in pos[np.lexsort((code[pos], -gain[pos]))]:
            w = int(code[c])
            mv = (w >> 40, (w >> 32) & 255, (w >> 24) & 255, (w >> 16) & 255, (w >> 8) & 255, w & 255)
            g, ok = self.fast(mv)
            if ok:
                return g, mv
        return 0, None


def candidate_tests(st: _Search, move: Move) -> Tuple[int, Dict[str, bool]]:
    """One candidate, test by test, as the host C++ and K6g evaluate it: ``(gain, {"removal",
    "target", "insertion", "length"})``.  Type 0: ``removal`` is the walk of ``A'`` with
    ``Lq[A] - rem <= max_q``, ``target`` is ``sound[B]``, ``insertion`` K6f's candidate tests on ``B``
    but for its length test, which is ``length``.  Type 1: ``removal`` and ``target`` hold by
    themselves, ``insertion`` is K6g's bounded walk (:func:`inside_walk`) and ``length`` is
    ``Lq[A] - gain <= max_q``."""
    typ, A, x, B, i, j = move
    u = st.trips[A][x]
    rest, rem, rest_ok = st.removal(A, x)
    if typ == 0:
        trip = st.trips[B]
        ins, t = insertion_tests(st.q, st.qt, st.qd, st.kind, st.mate, trip, st.dep[B], st.z[B], st.load[B],
                                 st.Lq[B], st.cap_q, st.max_q, st.op, st.cl, st.sv, u, i, j)
        return rem - ins, {"removal": rest_ok, "target": st.sound[B],
                           "insertion": all(v for k, v in t.items() if k != "length"), "length": t["length"]}
    _, _, ins = st.ins_table(rest, u)
    k = len(rest) - 2
    # the row of (i, j) in ins_table's order: the diagonal first, then the upper triangle by rows
    at = i if j == i else (k + 1) + i * (k + 1) - i * (i + 1) // 2 + (j - i - 1)
    gain = rem - int(ins[at])
    return gain, {"removal": True, "target": True, "insertion": inside_walk(st, A, x, i, j),
                  "length": st.Lq[A] - gain <= st.max_q}


def inside_walk(st: _Search, A: int, x: int, i: int, j: int) -> bool:
    """The walk of a type-1 candidate as K6g runs it.  In a sound trip nothing changes in front of
    the unit and of the insertion position: the walk starts behind the last unchanged position
    ``y0`` from the old ``dep`` / ``load``, ends at the first failure, and at the first stop behind
    every change the old ``z`` decides for the rest (its legs and loads are the old ones).  An
    unsound trip (a seed the float tests alone admitted) is walked in full."""
    a = st.trips[A]
    kA = len(a) - 2
    u = a[x]
    pair = st.kind[u] == PICKUP
    v = st.mate[u] if pair else 0
    yv = a.index(v) if pair else 0
    if not st.sound[A]:
        return st.trip_sound(apply_insertion(remove_unit(a, st.kind, st.mate, x), st.mate, st.kind, u, i, j))
    y = i + 1                       # stop number i + 1 of A' as a position of A (kA + 1: the end)
    y += 1 if y >= x else 0
    y += 1 if pair and y >= yv else 0
    y0 = min(x, y) - 1
    clock, ld, prev, at = st.dep[A][y0], st.load[A][y0], a[y0], y0
    last = j if pair else i
    ok = True

    def step(s):
        nonlocal clock, ld, prev, ok
        leg = int(st.qt[prev, s])
        start = max(clock + leg, int(st.op[s]))
        ok = ok and int(st.q[prev, s]) < BIG and leg < BIG and start <= int(st.cl[s])
        clock = start + int(st.sv[s])
        ld += int(st.qd[st.mate[s]]) if st.kind[s] == PICKUP else -int(st.qd[s])
        ok = ok and ld <= st.cap_q
        prev = s

    if i == y0:
        step(u)
        if pair and j == y0:
            step(v)
    for p in range(y0 + 1, kA + 1):
        if p == x or p == yv:
            continue
        at += 1
        s = a[p]
        if p > x and p > yv and at > last:
            leg = int(st.qt[prev, s])
            return (ok and int(st.q[prev, s]) < BIG and leg < BIG
                    and max(clock + leg, int(st.op[s])) <= st.z[A][p])
        step(s)
        if at == i:
            step(u)
        if pair and at == j:
            step(v)
        if not ok:
            return False
    return ok and int(st.q[prev, 0]) < BIG and int(st.qt[prev, 0]) < BIG


def pd_improve_trips(d, t, trips: Sequence[Sequence[int]], demand: Sequence[float], cap: float,
                     max_dist: float, open_q: Sequence[int], close_q: Sequence[int], sv_q: Sequence[int],
                     pickup_from: Sequence[int], trace: Optional[list] = None, applied: Optional[list] = None
                     ) -> Tuple[List[List[int]], Schedule, Dict[str, int]]:
    """Arguments as :func:`shipments.pd_trips` takes them; ``trips``: its trips.  Returns the new
    trips, their schedule (as ``pd_trips`` returns it) and ``{"moves", "pair_moves", "rejected",
    "trips_before", "trips_after", "len_before_q", "len_after_q", "waiting_q"}``.  ``trace``: a list
    that receives ``(trips, [(move, fast gain, fast tests, defined gain, defined verdict)])`` with
    every candidate of the definition's ranges before each selection (the slow path); ``applied``: a
    list that receives the ``(type, A, x, B, i, j)`` of every move that is kept (tests)."""
    dn = np.asarray(d, dtype=np.float64)
    tn = np.asarray(t, dtype=np.float64)
    n1 = dn.shape[0]
    ns = n1 - 1
    kind, mate = kinds_of(pickup_from, n1)
    cap, max_dist = float(cap), float(max_dist)
    q, qt = usable_matrix(dn), usable_matrix(tn)
    qd = np.array([0] + [quantize(demand[s]) for s in range(1, n1)], dtype=np.int64)
    op = np.array([0] + [int(open_q[s]) for s in range(1, n1)], dtype=np.int64)
    cl = np.array([UNBOUNDED] + [int(close_q[s]) for s in range(1, n1)], dtype=np.int64)
    sv = np.array([0] + [int(sv_q[s]) for s in range(1, n1)], dtype=np.int64)
    cap_q, max_q = limit_q(cap), limit_q(max_dist)
    cur = [[int(v) for v in trip] for trip in trips]
    st = _Search(q, qt, qd, kind, mate, op, cl, sv, cap_q, max_q, cur)
    before = sum(st.Lq)
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats.update(trips_before=len(cur), trips_after=len(cur), len_before_q=before, len_after_q=before)
    skip = (ns > MAX_STOPS or cap_q < 0 or max_q < 0
            or any(int(qd[s]) == BIG and kind[s] != PICKUP for s in range(1, n1)))
    while not skip and stats["moves"] < 4 * ns:
        gain, mv = st.best_move(trace)
        if mv is None or gain <= 0:
            break
        new = moved_trips(cur, kind, mate, mv)
        if not all(len(o) == 2 or (walk_feasible(dn, o, max_dist) and pd_load_feasible(demand, kind, mate, o, cap))
                   for o in new.values()):
            stats["rejected"] = 1
            break
        pair = kind[cur[mv[1]][mv[2]]] == PICKUP
        for x, o in new.items():
            cur[x] = o
        for x in new:
            st.refresh(x)
        stats["moves"] += 1
        stats["pair_moves"] += 1 if pair else 0
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


__all__ = ["METHOD", "STAT_KEYS", "wants_shipment_improve", "move_code", "remove_unit", "moved_trips",
           "candidate_tests", "inside_walk", "pd_improve_trips"]
