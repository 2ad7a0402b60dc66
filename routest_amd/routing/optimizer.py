"""Route optimizer: dispatcher + point-to-point + multi-stop + trip assembly (R19-R23).

Reference: ``optimize_route`` (``RO/Flaskr/utils.py:10-48``), ``_point_to_point`` (``:53-82``),
``_multi_stop`` (``:85-193``), ``_annotate_common_props`` (``:196-201``).  Behaviour kept:

* ``{"error": "no destination points specified."}`` on empty input;
* vehicle_type -> profile mapping (lower-cased, stripped; default ``driving-car``);
* one destination: route first, *then* the payload/max-distance feasibility check with the
  reference's ``" | "``-joined messages; ``optimized_order=[0]``, ``source``, ``destinations``;
* many destinations: distance matrix over ``[source]+destinations``, greedy multi-trip
  construction (:mod:`routing.greedy`), per-trip directions concatenated, bbox, summary with
  ``trips``; ``optimized_order`` as 0-based destination indices;
* metadata ``vehicle_type``, ``driver_name``, ``engine``.

Fixed: infeasible stops return an error instead of hanging (Appendix B #3).

Opt-in (``"improve": true`` on a multi-stop request, JSON ``true`` exactly): every trip of the
greedy is re-sequenced by the intra-trip 2-opt / Or-opt of :mod:`routing.improve` before the legs
are routed, and ``properties.improvement`` reports what it did.  Single-destination requests and
``alternatives`` requests ignore the field; without it every response is unchanged.
``"exchange": true`` (same rule; it implies ``improve``) adds the inter-trip relocate / swap search
of :mod:`routing.exchange` between two such passes; the answer may then hold fewer trips.
``"tw_improve": true`` (same rule) on a time-window request improves the cheapest insertion's trips
by the window-aware local search of :mod:`routing.tw_improve`; any other request ignores it.
A destination carrying ``"pickup_from": p`` makes a multi-stop request a shipment request
(:mod:`routing.shipments`): pickup -> delivery pairs and plain stops planned by cheapest insertion
of units under the windows; ``improve`` / ``exchange`` / ``tw_improve`` are ignored there.
``"shipment_improve": true`` (same rule) on a shipment request improves those trips by the
unit-relocate search of :mod:`routing.shipment_improve`; any other request ignores it.
The batched GPU path for many concurrent requests (K5 + K6) is :func:`optimize_many`.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .greedy import InfeasibleStops, greedy_trips, optimized_order
from .exchange import improve_exchange_trips, wants_exchange
from .improve import improve_trips, improvement_properties, wants_improve
from .providers import ProviderError, _bbox, profile_for
from .timewindows import (NEEDS_MATRIX_TIMES, parse_time_windows, schedule_properties, tw_trips,
                          wants_time_windows)
from .shipments import (NEEDS_MATRIX_TIMES as PD_NEEDS_MATRIX_TIMES, parse_shipments, pd_trips,
                        shipment_properties, wants_shipments)
from .shipment_improve import pd_improve_trips, wants_shipment_improve
from .tw_improve import tw_improve_trips, wants_tw_improve


def _annotate(feature: Dict[str, Any], driver: Dict[str, Any], vehicle_type: str, engine: str) -> None:
    p = feature.setdefault("properties", {})
    p["vehicle_type"] = vehicle_type
    p["driver_name"] = driver.get("driver_name")
    p["engine"] = engine


def _vehicle_type(driver: Dict[str, Any]) -> str:
    vt = driver.get("vehicle_type") or "car"
    return vt.lower().strip() if isinstance(vt, str) else "car"


def _float(v: Any, default: float) -> float:
    try:
        return float(v)
    except (TypeError, ValueError):
        return default


def _ctx_kw(ctx) -> Dict[str, Any]:
    """Routing context for context-aware providers (routing/cch.py); others take no such argument."""
    return {"ctx": ctx} if ctx is not None else {}


def point_to_point(provider, source, dest, profile: str, driver: Dict[str, Any], ctx=None) -> Dict[str, Any]:
    coords = [[source["lon"], source["lat"]], [dest["lon"], dest["lat"]]]
    try:
        feature = provider.directions(coords, profile, **_ctx_kw(ctx))
    except ProviderError as e:
        return {"error": str(e)}
    payload = dest.get("payload", 0)
    cap = driver.get("vehicle_capacity", 999999)
    max_dist = _float(driver.get("maximum_distance", 9e12), 9e12)
    dist_m = float(feature["properties"]["summary"]["distance"])
    errors = []
    try:
        if payload > cap:
            errors.append("payload exceeds vehicle capacity")
    except TypeError:
        pass
    if dist_m > max_dist:
        errors.append("route distance exceeds maximum_distance")
    if errors:
        return {"error": " | ".join(errors)}
    return feature


def assemble_trips(provider, all_points: List[Dict[str, Any]], trips: List[List[int]],
                   profile: str, source, destinations, ctx=None) -> Dict[str, Any]:
    geometry: List[List[float]] = []
    segments: List[Any] = []
    tot_d = 0.0
    tot_t = 0.0
    for trip in trips:
        coords = [[all_points[i]["lon"], all_points[i]["lat"]] for i in trip]
        try:
            f = provider.directions(coords, profile, **_ctx_kw(ctx))
        except ProviderError as e:
            return {"error": str(e)}
        geometry += f["geometry"]["coordinates"]
        segments += f["properties"].get("segments", [])
        tot_d += float(f["properties"]["summary"]["distance"])
        tot_t += float(f["properties"]["summary"]["duration"])
    return {
        "bbox": _bbox(geometry),
        "type": "Feature",
        "geometry": {"type": "LineString", "coordinates": geometry},
        "properties": {
            "source": source,
            "destinations": destinations,
            "optimized_order": optimized_order(trips),
            "segments": segments,
            "summary": {"distance": tot_d, "duration": tot_t, "trips": len(trips)},
        },
    }


def multi_stop(provider, source, destinations, profile: str, driver: Dict[str, Any],
               trips: Optional[List[List[int]]] = None, ctx=None, improve: bool = False,
               improvement: Optional[Dict[str, int]] = None, exchange: bool = False,
               tw=None, tw_result=None, tw_improve: bool = False, pd=None,
               shipment_improve: bool = False) -> Dict[str, Any]:
    """``improve``: re-sequence the trips built here (routing/improve.py); ``exchange``: also move
    stops between them (routing/exchange.py; it implies ``improve``).  Trips given by the caller
    are taken as they are; ``improvement`` holds their statistics if they were improved.
    ``tw``: the request's ``(open_q, close_q, sv_q)`` (routing/timewindows.py): the trips are built
    by cheapest insertion under the windows, ``improve`` / ``exchange`` are ignored and the response
    carries ``schedule`` / ``time_windows``; ``tw_result``: the ``(schedule, statistics)`` of given trips.
    ``tw_improve``: the trips built here under the windows are improved (routing/tw_improve.py).
    ``pd``: the request's ``pickup_from`` per point (routing/shipments.py; it comes with ``tw``): the
    trips hold pickup -> delivery pairs, ``tw_improve`` is ignored as well and the response also
    carries ``shipments``.  ``shipment_improve``: the trips built here for a shipment request are
    improved by the unit-relocate search (routing/shipment_improve.py)."""
    all_points = [source] + list(destinations)
    demand = [0.0] + [_float(p.get("payload", 0), 0.0) for p in destinations]
    if tw is not None and tw_result is None:
        # (trips that come without their schedule were not planned under the windows)
        needs = NEEDS_MATRIX_TIMES if pd is None else PD_NEEDS_MATRIX_TIMES
        if not hasattr(provider, "time_matrix"):
            return {"error": needs}
        try:
            sec, d = provider.time_matrix(all_points, profile, **_ctx_kw(ctx))
        except ProviderError as e:
            return {"error": needs if str(e) == NEEDS_MATRIX_TIMES else str(e)}
        try:
            plan = tw_trips if pd is None else pd_trips
            trips, schedule, tstats = plan(d, sec, demand, _float(driver.get("vehicle_capacity", 9e12), 9e12),
                                           _float(driver.get("maximum_distance", 9e12), 9e12), *tw,
                                           *(() if pd is None else (pd,)))
        except InfeasibleStops as e:
            return {"error": str(e)}
        if tw_improve and pd is None:
            trips, schedule, search = tw_improve_trips(
                d, sec, trips, demand, _float(driver.get("vehicle_capacity", 9e12), 9e12),
                _float(driver.get("maximum_distance", 9e12), 9e12), *tw)
            tstats = dict(tstats, trips=len(trips), search=search)
        if shipment_improve and pd is not None:
            trips, schedule, search = pd_improve_trips(
                d, sec, trips, demand, _float(driver.get("vehicle_capacity", 9e12), 9e12),
                _float(driver.get("maximum_distance", 9e12), 9e12), *tw, pd)
            tstats = dict(tstats, trips=len(trips), search=search)
        tw_result = (schedule, tstats)
    if tw is not None:
        feature = assemble_trips(provider, all_points, trips, profile, source, destinations, ctx)
        if "error" not in feature and tw_result is not None:
            p = feature["properties"]
            if pd is None:
                p["schedule"], p["time_windows"] = schedule_properties(tw_result[0], tw_result[1], tw[1])
            else:
                p["schedule"], p["time_windows"], p["shipments"] = shipment_properties(
                    tw_result[0], tw_result[1], tw[1], demand, pd)
        return feature
    if trips is None:
        try:
            d = provider.matrix(all_points, profile, **_ctx_kw(ctx))
        except ProviderError as e:
            return {"error": str(e)}
        cap = _float(driver.get("vehicle_capacity", 9e12), 9e12)
        max_dist = _float(driver.get("maximum_distance", 9e12), 9e12)
        try:
            dm = np.asarray(d, dtype=np.float64)
            trips = greedy_trips(dm.tolist(), demand, cap, max_dist)
        except InfeasibleStops as e:
            return {"error": str(e)}
        if exchange:
            trips, improvement = improve_exchange_trips(dm, trips, demand, cap, max_dist)
        elif improve:
            trips, improvement = improve_trips(dm, trips, max_dist)
    feature = assemble_trips(provider, all_points, trips, profile, source, destinations, ctx)
    if improvement is not None and "error" not in feature:
        feature["properties"]["improvement"] = improvement_properties(improvement)
    return feature


def optimize_route(input_data: Any, provider, engine: str = "backend:mi355x",
                   trips: Optional[List[List[int]]] = None, ctx=None,
                   improvement: Optional[Dict[str, int]] = None, tw_result=None) -> Dict[str, Any]:
    """Pure function: GeoJSON Feature on success, ``{"error": ...}`` on failure (R19).  ``ctx``:
    the request's routing context as resolved when its legs were planned (the batcher), so a
    request without ``pickup_time`` is assembled under the same week-hour it was routed in.
    ``improvement``: the statistics of given ``trips`` that were already improved (the batcher);
    ``tw_result``: the ``(schedule, statistics)`` of given ``trips`` of a time-window request."""
    if not input_data or not isinstance(input_data, dict) or not input_data.get("destination_points"):
        return {"error": "no destination points specified."}
    driver = input_data.get("driver_details") or {}
    vehicle_type = _vehicle_type(driver)
    profile = profile_for(vehicle_type)
    source = input_data.get("source_point")
    if not isinstance(source, dict) or "lat" not in source or "lon" not in source:
        return {"error": "source_point with lat/lon is required."}
    destinations = input_data["destination_points"]
    # road providers route under the request's context (weather, traffic, pickup week-hour, and
    # the areas options.avoid_polygons closes)
    from .avoid import NEEDS_CCH, parse_options
    try:
        avoid = parse_options(input_data)
    except ValueError as e:
        return {"error": str(e)}
    if not getattr(provider, "uses_context", False):
        if avoid is not None:
            return {"error": NEEDS_CCH}
        ctx = None
    elif ctx is None:
        from .cch import RouteContext
        ctx = RouteContext.from_request(input_data)
    if avoid is None:
        return _optimize(input_data, provider, engine, trips, ctx, improvement, driver, vehicle_type, profile,
                         source, destinations, tw_result)
    try:
        feature = _optimize(input_data, provider, engine, trips, ctx, improvement, driver, vehicle_type, profile,
                            source, destinations, tw_result)
    except ValueError as e:                     # the set's digest is cached for another set (routing/cch.py)
        return {"error": str(e)}
    if "error" not in feature:
        feature.setdefault("properties", {})["avoid"] = avoid.summary()
    return feature


def _optimize(input_data, provider, engine, trips, ctx, improvement, driver, vehicle_type, profile, source,
              destinations, tw_result=None) -> Dict[str, Any]:
    if len(destinations) == 1:
        feature = point_to_point(provider, source, destinations[0], profile, driver, ctx)
        if "error" in feature:
            return feature
        p = feature.setdefault("properties", {})
        p["optimized_order"] = [0]
        p["source"] = source
        p["destinations"] = [destinations[0]]
        _annotate(feature, driver, vehicle_type, engine)
        return feature
    tw = pd = None
    ship = wants_shipments(input_data)
    if ship or wants_time_windows(input_data):
        try:
            tw = parse_time_windows(input_data)
            pd = parse_shipments(input_data) if ship else None
        except ValueError as e:
            return {"error": str(e)}
    feature = multi_stop(provider, source, destinations, profile, driver, trips, ctx,
                         improve=wants_improve(input_data), improvement=improvement,
                         exchange=wants_exchange(input_data), tw=tw, tw_result=tw_result,
                         tw_improve=wants_tw_improve(input_data), pd=pd,
                         shipment_improve=wants_shipment_improve(input_data))
    if "error" in feature:
        return feature
    _annotate(feature, driver, vehicle_type, engine)
    return feature


def optimize_many(requests: Sequence[Dict[str, Any]], provider, engine: str = "backend:mi355x",
                  device=None) -> List[Dict[str, Any]]:
    """Batched optimizer for many concurrent requests: the distance matrices and greedy trips of
    every multi-stop request are computed in ONE pair of GPU launches (K5 + K6) when a GPU device
    is given (haversine provider only); assembly stays on the host."""
    from .batched import batched_trips
    multi = [i for i, r in enumerate(requests)
             if isinstance(r, dict) and isinstance(r.get("destination_points"), list)
             and len(r["destination_points"]) > 1 and isinstance(r.get("source_point"), dict)]
    trip_map: Dict[int, Any] = {}
    stat_map: Dict[int, Any] = {}
    tw_map: Dict[int, Any] = {}
    if multi and getattr(provider, "name", "") == "haversine":
        # time-window requests (routing/timewindows.py) ride in the same batch; a malformed one is
        # left out here and answered with its error by optimize_route below
        tws = [_tw_or_none(requests[i]) for i in multi]
        kw = ({"time_windows": tws, "tw_improve": [wants_tw_improve(requests[i]) for i in multi],
               "shipment_improve": [wants_shipment_improve(requests[i]) for i in multi]}
              if any(v is not None for v in tws) else {})
        got = batched_trips([requests[i] for i in multi], circuity=provider.circuity,
                            device=device, improve=[wants_improve(requests[i]) for i in multi],
                            exchange=[wants_exchange(requests[i]) for i in multi], **kw)
        res, stats = got[0], got[1]
        # a malformed time-window request keeps no trips: optimize_route answers with its error
        trip_map = {i: t for i, t in zip(multi, res) if not _tw_malformed(requests[i])}
        stat_map = dict(zip(multi, stats))
        if kw:
            tw_map = dict(zip(multi, got[2]))
    out = []
    for i, r in enumerate(requests):
        t = trip_map.get(i)
        if isinstance(t, InfeasibleStops):
            out.append({"error": str(t)})
            continue
        out.append(optimize_route(r, provider, engine, trips=t, improvement=stat_map.get(i),
                                  tw_result=tw_map.get(i)))
    return out


def _tw_or_none(request):
    """``(open_q, close_q, sv_q)`` of a time-window request, ``(open_q, close_q, sv_q, pickup_from)``
    of a shipment request (routing/shipments.py), None for any other and for a malformed one."""
    ship = wants_shipments(request)
    if not (ship or wants_time_windows(request)):
        return None
    try:
        tw = parse_time_windows(request)
        return tw + (parse_shipments(request),) if ship else tw
    except ValueError:
        return None


def _tw_malformed(request) -> bool:
    return (wants_time_windows(request) or wants_shipments(request)) and _tw_or_none(request) is None
