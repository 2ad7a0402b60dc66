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
Sharding over several GPUs is done by
:class:`routing.route_batcher.RouteBatcher` (one worker thread per device, no collective).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from ..ops import _ext
from .greedy import InfeasibleStops, greedy_trips
from .exchange import improve_exchange_trips
from .improve import improve_trips
from .providers import haversine_matrix

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


def batched_trips_device(lat, lon, dem, npts, cap, maxd, circuity: float, device,
                         D: Optional[np.ndarray] = None, improve: Optional[Sequence[Any]] = None,
                         exchange: Optional[Sequence[Any]] = None):
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
    if flags is None:
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
    return out, res


def batched_trips_cpu(lat, lon, dem, npts, cap, maxd, circuity: float,
                      D: Optional[np.ndarray] = None, improve: Optional[Sequence[Any]] = None,
                      exchange: Optional[Sequence[Any]] = None):
    out: List[TripsOrError] = []
    flags, xflags = _both_flags(improve, exchange, len(npts))
    stats: List[Optional[Dict[str, int]]] = []
    for k in range(len(npts)):
        n = int(npts[k])
        d = D[k, :n, :n] if D is not None else haversine_matrix(lat[k, :n], lon[k, :n], circuity)
        st = None
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
    return out if flags is None else (out, stats)


def batched_trips(requests: Sequence[Dict[str, Any]], circuity: float = 1.3,
                  device: Optional[Any] = None, D: Optional[np.ndarray] = None,
                  improve: Optional[Sequence[Any]] = None,
                  exchange: Optional[Sequence[Any]] = None):
    """``D``: given distance matrices [R, nm, nm] (road metres from the CCH router) instead of the
    haversine K5.  ``improve`` / ``exchange``: one flag per request; when either is given, returns
    ``(results, stats)``.  ``exchange`` implies ``improve`` (:mod:`routing.exchange`)."""
    if not requests:
        return [] if improve is None and exchange is None else ([], [])
    packed = pack_requests(requests)
    if device is not None and torch.device(device).type == "cuda":
        return batched_trips_device(*packed, circuity=circuity, device=device, D=D, improve=improve,
                                    exchange=exchange)
    return batched_trips_cpu(*packed, circuity=circuity, D=D, improve=improve, exchange=exchange)
