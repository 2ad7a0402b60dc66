"""Batched multi-stop trip construction for many concurrent requests (K5 + K6).

``batched_trips(requests)`` packs R requests (each ``[source] + destinations``) into padded fp64
tensors, then on a GPU runs ONE K5 launch (all haversine matrices) and ONE K6 launch (all greedy
trip constructions, a wavefront per request); on CPU it runs the numpy/Python reference.  The
result per request is the trips list (index lists into ``[source]+destinations``) or an
:class:`InfeasibleStops` instance.  With per-request ``improve`` flags the flagged requests' trips
are re-sequenced by the intra-trip 2-opt / Or-opt of :mod:`routing.improve` (on a GPU one more
launch, K6b, on K6's own tensors) and the call returns ``(results, stats)``, ``stats[k]`` being the
request's improvement statistics or ``None``.  Per-request ``exchange`` flags add the inter-trip
relocate / swap search of :mod:`routing.exchange` between two such passes (on a GPU K6b, K6c, K6b).
Requests given ``time_windows`` are planned by the cheapest insertion of :mod:`routing.timewindows`
instead (on a GPU one launch, K6d, over the flagged rows only); per-request ``tw_improve`` flags add
the window-aware local search of :mod:`routing.tw_improve` on those rows (on a GPU one more launch, K6e).
A ``time_windows`` entry of four, ``pickup_from`` per point behind the windows, makes its row a
shipment row: pickup -> delivery pairs planned by :mod:`routing.shipments` (on a GPU one launch, K6f,
over those rows only); such a row is none of K6b's, K6c's, K6d's or K6e's.  Per-request
``shipment_improve`` flags add the unit-relocate search of :mod:`routing.shipment_improve` on those
rows (on a GPU one more launch, K6g).
Sharding over several GPUs is done by
:class:`routing.route_batcher.RouteBatcher` (one worker thread per device, no collective).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from ..ops import _ext
from .greedy import InfeasibleStops, greedy_trips
from .exchange import UNBOUNDED, improve_exchange_trips
from .improve import improve_trips
from .providers import haversine_matrix
from .shipment_improve import STAT_KEYS as PDI_STAT_KEYS, pd_improve_trips
from .shipments import pd_trips
from .timewindows import MAX_STOPS as TW_MAX_STOPS, tw_trips
from .tw_improve import STAT_KEYS as TWI_STAT_KEYS, tw_improve_trips

TripsOrError = Union[List[List[int]], InfeasibleStops]


def _f(v: Any, default: float) -> float:
    try:
        return float(v)
    except (TypeError, ValueError):
        return default


def pack_requests(requests: Sequence[Dict[str, Any]]):
    R = len(requests)
    nm = max(1 + len(r["destination_points"]) for r in requests) if R else 1
    lat = np.zeros((R, nm))
    lon = np.zeros((R, nm))
    dem = np.zeros((R, nm))
    npts = np.zeros(R, dtype=np.int32)
    cap = np.zeros(R)
    maxd = np.zeros(R)
    for k, r in enumerate(requests):
        pts = [r["source_point"]] + list(r["destination_points"])
        npts[k] = len(pts)
        lat[k, :len(pts)] = [p["lat"] for p in pts]
        lon[k, :len(pts)] = [p["lon"] for p in pts]
        dem[k, 1:len(pts)] = [_f(p.get("payload", 0), 0.0) for p in pts[1:]]
        drv = r.get("driver_details") or {}
        cap[k] = _f(drv.get("vehicle_capacity", 9e12), 9e12)
        maxd[k] = _f(drv.get("maximum_distance", 9e12), 9e12)
    return lat, lon, dem, npts, cap, maxd


def _unpack(visit: np.ndarray, trip_of: np.ndarray, ntrips: np.ndarray, status: np.ndarray,
            npts: np.ndarray, D: Optional[np.ndarray]) -> List[TripsOrError]:
    out: List[TripsOrError] = []
    for k in range(len(npts)):
        if status[k] != 0:
            placed = set(int(v) for v in visit[k] if v >= 0)
            rest = [i for i in range(1, int(npts[k])) if i not in placed]
            if D is not None:
                rest.sort(key=lambda i: D[k, 0, i])
            out.append(InfeasibleStops([i - 1 for i in rest]))
            continue
        trips: List[List[int]] = [[0] for _ in range(int(ntrips[k]))]
        for v, t in zip(visit[k], trip_of[k]):
            if v < 0:
                break
            trips[t].append(int(v))
        for t in trips:
            t.append(0)
        out.append(trips)
    return out


def _flags(improve: Optional[Sequence[Any]], R: int) -> Optional[np.ndarray]:
    if improve is None:
        return None
    f = np.array([1 if v else 0 for v in improve], dtype=np.uint8)
    if f.shape != (R,):
        raise ValueError(f"improve must hold one flag per request ({R}), got {f.shape[0]}")
    return f


def _both_flags(improve, exchange, R: int):
    """(improve flags, exchange flags), or (None, None) when neither list was given."""
    flags, xflags = _flags(improve, R), _flags(exchange, R)
    if flags is None and xflags is None:
        return None, None
    zeros = np.zeros(R, dtype=np.uint8)
    return (zeros if flags is None else flags), (zeros if xflags is None else xflags)


def pack_time_windows(requests: Sequence[Dict[str, Any]], time_windows: Sequence[Any], nm: int):
    """``time_windows[k]``: None, or the ``(open_q, close_q, sv_q)`` of
    :func:`timewindows.parse_time_windows` for request ``k``.  Returns ``(open, close, service``
    int64 [R, nm] milliseconds, ``flags`` uint8 [R], ``speed`` float64 [R]: the request profile's
    metres per second, which turns a haversine matrix into seconds)."""
    from .providers import PROFILE_SPEED_MPS, profile_for
    R = len(requests)
    if len(time_windows) != R:
        raise ValueError(f"time_windows must hold one entry per request ({R}), got {len(time_windows)}")
    op = np.zeros((R, nm), dtype=np.int64)
    cl = np.full((R, nm), UNBOUNDED, dtype=np.int64)
    sv = np.zeros((R, nm), dtype=np.int64)
    flags = np.zeros(R, dtype=np.uint8)
    speed = np.ones(R)
    for k, (r, tw) in enumerate(zip(requests, time_windows)):
        if tw is None:
            continue
        n = 1 + len(r["destination_points"])
        if n - 1 > TW_MAX_STOPS or len(tw) not in (3, 4) or any(len(v) != n for v in tw):
            raise ValueError(f"time_windows[{k}] must hold one entry per point, at most {TW_MAX_STOPS} stops")
        flags[k] = 1
        op[k, :n], cl[k, :n], sv[k, :n] = tw[:3]
        drv = r.get("driver_details") or {}
        profile = profile_for(drv.get("vehicle_type") if isinstance(drv, dict) else None)
        speed[k] = PROFILE_SPEED_MPS.get(profile, PROFILE_SPEED_MPS["driving-car"])
    return op, cl, sv, flags, speed


def pack_shipments(time_windows: Sequence[Any], nm: int):
    """The shipment rows of ``time_windows`` (entries of four: ``pickup_from`` per point behind the
    windows, :func:`shipments.parse_shipments`): ``(pickup_from`` int32 [R, nm], -1 where there is
    none, ``flags`` uint8 [R])."""
    R = len(time_windows)
    pf = np.full((R, nm), -1, dtype=np.int32)
    flags = np.zeros(R, dtype=np.uint8)
    for k, tw in enumerate(time_windows):
        if tw is not None and len(tw) == 4:
            flags[k] = 1
            pf[k, :len(tw[3])] = tw[3]
    return pf, flags


def _pd_device(C, t, D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, pd, pdi=None):
    """K6f over the shipment rows: K6d's seven outputs, on the host, and the statistics [R, 8] of
    K6g over the rows of them that ``pdi`` flags (None: nobody asks)."""
    pf, pdf = pd
    pf_t = t(pf, torch.int32)
    out = C.route_pd_trips(D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, pf_t, t(pdf, torch.uint8))
    search = None
    if pdi is not None and (pdi & pdf).any():
        # K6g rewrites K6f's outputs in place for the asking rows; K6f's own statistics stay
        search = C.route_pd_improve(D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, pf_t, *out[:6],
                                    t(pdi & pdf, torch.uint8)).cpu().numpy()
    out = [c.cpu().numpy() for c in out]
    if (out[3][pdf != 0] == 3).any():
        raise ValueError("pickup_from must name another stop that is no delivery and no other delivery's pickup")
    return out, search


def _tw_device(C, t, D, T, npts, npts_t, dem_t, cap_t, maxd_t, tw, twi=None, pd=None, pdi=None):
    """K6d over the flagged rows: ``{row: trips or InfeasibleStops}``, ``{row: (schedule, stats)}``.
    ``twi``: uint8 flags of the rows whose trips K6e then improves (``stats["search"]``).  ``pd``:
    ``(pickup_from, flags)`` of :func:`pack_shipments`; those rows are K6f's, not K6d's or K6e's.
    ``pdi``: uint8 flags of the shipment rows whose trips K6g then improves (``stats["search"]``)."""
    op, cl, sv, twf, speed = tw
    if T is None:
        # one IEEE division per entry, as HaversineProvider.time_matrix does it on the host
        T = D / t(speed).reshape(-1, 1, 1)
    else:
        T = t(np.ascontiguousarray(T, dtype=np.float64))
    T = T.contiguous()
    op_t, cl_t, sv_t = t(op, torch.int64), t(cl, torch.int64), t(sv, torch.int64)
    pdf = pd[1] if pd is not None else np.zeros_like(twf)
    k6d = twf & ~pdf & 1
    out = search = None
    if k6d.any():
        out = C.route_tw_trips(D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, t(k6d, torch.uint8))
        if twi is not None and (twi & k6d).any():
            # K6e rewrites K6d's outputs in place for the asking rows; K6d's own statistics stay
            search = C.route_tw_improve(D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, *out[:6],
                                        t(twi & k6d, torch.uint8)).cpu().numpy()
            twi = twi & k6d
        out = [c.cpu().numpy() for c in out]
    psearch = None
    if pdf.any():
        # K6f's rows beside K6d's (a batch without shipment rows launches nothing more)
        ship, psearch = _pd_device(C, t, D, T, npts_t, dem_t, cap_t, maxd_t, op_t, cl_t, sv_t, pd, pdi)
        pdi = pdi & pdf if psearch is not None else None
        if out is None:
            out = ship
        else:
            for a, b in zip(out, ship):
                a[pdf != 0] = b[pdf != 0]
    visit, trip_of, ntrips, status, arr, start, stats = out
    rows = np.flatnonzero(twf)
    if (status[rows] > 1).any():
        raise ValueError(f"time-window rows take at most {TW_MAX_STOPS} stops")
    trips = _unpack(visit[rows], trip_of[rows], ntrips[rows], status[rows], np.asarray(npts)[rows], None)
    res, sched = {}, {}
    for x, k in enumerate(rows.tolist()):
        if isinstance(trips[x], InfeasibleStops):
            res[k] = InfeasibleStops(trips[x].stops, time_windows=True)
            continue
        res[k] = trips[x]
        one, p = [], 0
        for trip in trips[x]:
            one.append([(s, int(arr[k, p + i]), int(start[k, p + i]), int(start[k, p + i]) + int(sv[k, s]))
                        for i, s in enumerate(trip[1:-1])])
            p += len(trip) - 2
        sched[k] = (one, {"insertions": int(stats[k, 0]), "rejected": int(stats[k, 1]), "trips": len(trips[x]),
                          "len_q": int(stats[k, 2]), "waiting_q": int(stats[k, 3])})
        if search is not None and twi[k]:
            sched[k][1]["search"] = {key: int(v) for key, v in zip(TWI_STAT_KEYS, search[k])}
        if psearch is not None and pdi[k]:
            sched[k][1]["search"] = {key: int(v) for key, v in zip(PDI_STAT_KEYS, psearch[k])}
    return res, sched


def batched_trips_device(lat, lon, dem, npts, cap, maxd, circuity: float, device,
                         D: Optional[np.ndarray] = None, improve: Optional[Sequence[Any]] = None,
                         exchange: Optional[Sequence[Any]] = None, tw=None, T: Optional[np.ndarray] = None,
                         tw_improve: Optional[Sequence[Any]] = None, pd=None,
                         shipment_improve: Optional[Sequence[Any]] = None):
    # K6 indexes its LDS order / visited arrays by stop number: a request longer than the padded
    # width would write past them, so it is refused here, before anything reaches the device
    nm = int(D.shape[1]) if D is not None else int(np.shape(lat)[1])
    n = np.asarray(npts)
    if n.size and (int(n.min()) < 0 or int(n.max()) > nm):
        raise ValueError(f"npts must lie in 0..{nm} (the padded width of the batch), got "
                         f"{int(n.min())}..{int(n.max())}")
    C = _ext.native(required=True)
    dev = torch.device(device)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(dev)  # noqa: E731
    if D is None:
        D = C.route_haversine_matrix(t(lat), t(lon), t(npts, torch.int32), float(circuity))
    else:
        D = t(np.ascontiguousarray(D, dtype=np.float64))
    flags, xflags = _both_flags(improve, exchange, len(n))
    if tw is not None and flags is not None:
        # improve / exchange know nothing of windows: a time-window row ignores them
        flags, xflags = flags & ~tw[3] & 1, xflags & ~tw[3] & 1
    npts_t, maxd_t, dem_t, cap_t = t(npts, torch.int32), t(maxd), t(dem), t(cap)
    visit, trip_of, ntrips, status = C.route_greedy_cvrp(D, npts_t, dem_t, cap_t, maxd_t)
    stats = xstats = stats3 = None
    if flags is not None and (flags | xflags).any():
        # K6b rewrites visit in place for the flagged rows; a batch nobody flags launches nothing
        stats = C.route_improve_trips(D, npts_t, maxd_t, visit, trip_of, status,
                                      t(flags | xflags, torch.uint8))
    if flags is not None and xflags.any():
        # K6c moves stops between the trips of the rows that ask for the exchange, then K6b runs
        # again over those rows only: it overwrites a row's statistics, so an improve-only row
        # (whose second pass would find nothing) must keep the first launch's
        xf = t(xflags, torch.uint8)
        xstats = C.route_exchange_trips(D, npts_t, dem_t, cap_t, maxd_t, visit, trip_of, ntrips,
                                        status, xf)
        stats3 = C.route_improve_trips(D, npts_t, maxd_t, visit, trip_of, status, xf)
    status_h = status.cpu().numpy()
    out = _unpack(visit.cpu().numpy(), trip_of.cpu().numpy(), ntrips.cpu().numpy(), status_h,
                  npts, D.cpu().numpy())
    if tw is not None:
        # K6d plans the flagged rows (a batch nobody flags launches nothing); the others keep K6's
        twres: List[Any] = [None] * len(n)
        if tw[3].any():
            planned, sched = _tw_device(C, t, D, T, npts, npts_t, dem_t, cap_t, maxd_t, tw,
                                        _flags(tw_improve, len(n)), pd,
                                        _flags(shipment_improve, len(n)) if pd is not None else None)
            for k, v in planned.items():
                out[k] = v
                twres[k] = sched.get(k)
            status_h = np.where(tw[3] != 0, 1, status_h)      # no improvement statistics for these rows
        if flags is None:
            return out, [None] * len(n), twres
    elif flags is None:
        return out
    cols = [c.cpu().numpy() for c in stats] if stats is not None else None
    xcols = [c.cpu().numpy() for c in xstats] if xstats is not None else None
    cols3 = [c.cpu().numpy() for c in stats3] if stats3 is not None else None
    res: List[Optional[Dict[str, int]]] = [None] * len(n)
    # only the asking rows are visited: a batch nobody asks in pays nothing per request
    for k in np.flatnonzero((flags | xflags) & (status_h == 0)).tolist():
        if xflags[k]:
            res[k] = {"moves": int(cols[0][k]) + int(cols3[0][k]), "exchange_moves": int(xcols[0][k]),
                      "trips_before": int(xcols[2][k]), "trips_after": int(xcols[3][k]),
                      "len_before_q": int(cols[2][k]), "len_after_q": int(cols3[3][k])}
        else:
            res[k] = {"moves": int(cols[0][k]), "trips_changed": int(cols[1][k]),
                      "len_before_q": int(cols[2][k]), "len_after_q": int(cols[3][k])}
    return (out, res) if tw is None else (out, res, twres)


def batched_trips_cpu(lat, lon, dem, npts, cap, maxd, circuity: float,
                      D: Optional[np.ndarray] = None, improve: Optional[Sequence[Any]] = None,
                      exchange: Optional[Sequence[Any]] = None, tw=None, T: Optional[np.ndarray] = None,
                      tw_improve: Optional[Sequence[Any]] = None, pd=None,
                      shipment_improve: Optional[Sequence[Any]] = None):
    out: List[TripsOrError] = []
    flags, xflags = _both_flags(improve, exchange, len(npts))
    twi = _flags(tw_improve, len(npts))
    pdi = _flags(shipment_improve, len(npts))
    stats: List[Optional[Dict[str, int]]] = []
    twres: List[Any] = []
    for k in range(len(npts)):
        n = int(npts[k])
        d = D[k, :n, :n] if D is not None else haversine_matrix(lat[k, :n], lon[k, :n], circuity)
        st = None
        if tw is not None and tw[3][k]:
            # the reference of K6d (routing/timewindows.py); improve / exchange are ignored
            sec = T[k, :n, :n] if T is not None else np.asarray(d, dtype=np.float64) / tw[4][k]
            try:
                if pd is not None and pd[1][k]:
                    # the reference of K6f (routing/shipments.py); tw_improve is ignored as well
                    trips, sched, tst = pd_trips(d, sec, dem[k, :n].tolist(), float(cap[k]), float(maxd[k]),
                                                 tw[0][k, :n], tw[1][k, :n], tw[2][k, :n], pd[0][k, :n].tolist())
                else:
                    trips, sched, tst = tw_trips(d, sec, dem[k, :n].tolist(), float(cap[k]), float(maxd[k]),
                                                 tw[0][k, :n], tw[1][k, :n], tw[2][k, :n])
                if twi is not None and twi[k] and not (pd is not None and pd[1][k]):
                    # the reference of K6e (routing/tw_improve.py) on the insertion's trips
                    trips, sched, search = tw_improve_trips(d, sec, trips, dem[k, :n].tolist(), float(cap[k]),
                                                            float(maxd[k]), tw[0][k, :n], tw[1][k, :n], tw[2][k, :n])
                    tst = dict(tst, trips=len(trips), search=search)
                if pdi is not None and pdi[k] and pd is not None and pd[1][k]:
                    # the reference of K6g (routing/shipment_improve.py) on the insertion's trips
                    trips, sched, search = pd_improve_trips(d, sec, trips, dem[k, :n].tolist(), float(cap[k]),
                                                            float(maxd[k]), tw[0][k, :n], tw[1][k, :n], tw[2][k, :n],
                                                            pd[0][k, :n].tolist())
                    tst = dict(tst, trips=len(trips), search=search)
                out.append(trips)
                twres.append((sched, tst))
            except InfeasibleStops as e:
                out.append(e)
                twres.append(None)
            stats.append(None)
            continue
        twres.append(None)
        try:
            trips = greedy_trips(d.tolist(), dem[k, :n].tolist(), float(cap[k]), float(maxd[k]))
            if flags is not None and xflags[k]:
                trips, st = improve_exchange_trips(d, trips, dem[k, :n].tolist(), float(cap[k]),
                                                   float(maxd[k]))
            elif flags is not None and flags[k]:
                trips, st = improve_trips(d, trips, float(maxd[k]))
            out.append(trips)
        except InfeasibleStops as e:
            out.append(e)
        stats.append(st)
    if tw is not None:
        return out, stats, twres
    return out if flags is None else (out, stats)


def batched_trips(requests: Sequence[Dict[str, Any]], circuity: float = 1.3,
                  device: Optional[Any] = None, D: Optional[np.ndarray] = None,
                  improve: Optional[Sequence[Any]] = None,
                  exchange: Optional[Sequence[Any]] = None,
                  time_windows: Optional[Sequence[Any]] = None, T: Optional[np.ndarray] = None,
                  tw_improve: Optional[Sequence[Any]] = None,
                  shipment_improve: Optional[Sequence[Any]] = None):
    """``D``: given distance matrices [R, nm, nm] (road metres from the CCH router) instead of the
    haversine K5.  ``improve`` / ``exchange``: one flag per request; when either is given, returns
    ``(results, stats)``.  ``exchange`` implies ``improve`` (:mod:`routing.exchange`).

    ``time_windows``: per request None or the ``(open_q, close_q, sv_q)`` of
    :func:`timewindows.parse_time_windows`; those requests are planned by the cheapest insertion of
    :mod:`routing.timewindows` (on a GPU one launch, K6d) and ignore ``improve`` / ``exchange``, the
    others are planned as without the argument.  ``T``: the seconds matrices that go with ``D``
    (without ``D``: haversine metres over the request profile's speed).  When given, the call
    returns ``(results, stats, tw)`` with ``tw[k]`` None or ``(schedule, statistics)``.

    ``tw_improve``: one flag per request, honoured only on time-window rows: their trips are improved
    by the window-aware local search of :mod:`routing.tw_improve` (on a GPU one more launch, K6e) and
    ``statistics["search"]`` holds what it did; an unflagged row's entry is as without the argument.

    A ``time_windows`` entry ``(open_q, close_q, sv_q, pickup_from)`` (``pickup_from`` as
    :func:`shipments.parse_shipments` returns it) is a shipment request: planned by
    :mod:`routing.shipments` (on a GPU one launch, K6f); ``improve`` / ``exchange`` / ``tw_improve``
    are ignored on it and its ``tw[k]`` is shaped like a time-window row's.

    ``shipment_improve``: one flag per request, honoured only on shipment rows: their trips are
    improved by the unit-relocate search of :mod:`routing.shipment_improve` (on a GPU one more launch,
    K6g, over the asking shipment rows only) and ``statistics["search"]`` holds what it did."""
    if time_windows is not None and (D is None) != (T is None):
        raise ValueError("time windows on given matrices need both D (metres) and T (seconds)")
    if not requests:
        if time_windows is not None:
            return [], [], []
        return [] if improve is None and exchange is None else ([], [])
    packed = pack_requests(requests)
    tw = pd = None
    if time_windows is not None:
        nm = int(D.shape[1]) if D is not None else int(packed[0].shape[1])
        tw = pack_time_windows(requests, time_windows, nm)
        pd = pack_shipments(time_windows, nm)
        pd = pd if pd[1].any() else None
    if device is not None and torch.device(device).type == "cuda":
        return batched_trips_device(*packed, circuity=circuity, device=device, D=D, improve=improve,
                                    exchange=exchange, tw=tw, T=T, tw_improve=tw_improve, pd=pd,
                                    shipment_improve=shipment_improve)
    return batched_trips_cpu(*packed, circuity=circuity, D=D, improve=improve, exchange=exchange, tw=tw, T=T,
                             tw_improve=tw_improve, pd=pd, shipment_improve=shipment_improve)
