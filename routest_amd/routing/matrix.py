"""``POST /api/matrix``: ORS's matrix shape (``locations`` with ``sources`` / ``destinations``
index lists, ``metrics``) answered by the CCH router's rectangular matrices under the request's
routing context (``RoadRouter.matrix_rect``, csrc/cch_query.hip meet_rect_kernel).  The reference
service bought these from ORS ``/v2/matrix`` (``RO/Flaskr/utils.py:97-105``).

A cell is ``float()`` of the router's f32 value, unrounded (a client can compare it with a leg of
the same pair), ``null`` where there is no route.  ``distances`` are the metres of the
time-shortest paths, like every other distance this service reports.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List

import numpy as np

MAX_LOCATIONS = 4096
MAX_CELLS = 262_144            # |sources| x |destinations| of one request
METRICS = ("duration", "distance")


def _number(x: Any) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)


def _indices(data: Dict[str, Any], name: str, n: int) -> List[int]:
    v = data.get(name, "all")
    if v is None or v == "all":
        return list(range(n))
    if not isinstance(v, list) or not v:
        raise ValueError(f"{name}: 'all' or a non-empty list of indices into locations")
    for i in v:
        if isinstance(i, bool) or not isinstance(i, int):
            raise ValueError(f"{name}: integer indices")
        if not 0 <= i < n:
            raise ValueError(f"{name}: index {i} out of range (0..{n - 1})")
    if len(set(v)) != len(v):
        raise ValueError(f"{name}: distinct indices")
    return list(v)


def parse_request(data: Any) -> Dict[str, Any]:
    """The validated request; :class:`ValueError` (the 400's message) on anything malformed."""
    if not isinstance(data, dict):
        raise ValueError("expected a JSON object")
    locs = data.get("locations")
    if not isinstance(locs, list) or not locs:
        raise ValueError("locations: a non-empty list of [lon, lat]")
    if len(locs) > MAX_LOCATIONS:
        raise ValueError(f"locations: at most {MAX_LOCATIONS}")
    for p in locs:
        if not (isinstance(p, (list, tuple)) and len(p) == 2 and _number(p[0]) and _number(p[1])
                and -180.0 <= p[0] <= 180.0 and -90.0 <= p[1] <= 90.0):
            raise ValueError("locations: every entry is [lon, lat] in degrees")
    src = _indices(data, "sources", len(locs))
    dst = _indices(data, "destinations", len(locs))
    if len(src) * len(dst) > MAX_CELLS:
        raise ValueError(f"sources x destinations: at most {MAX_CELLS} cells")
    metrics = data.get("metrics", ["duration"])
    if not isinstance(metrics, list) or not metrics or not all(isinstance(m, str) and m in METRICS for m in metrics):
        raise ValueError("metrics: a non-empty subset of ['duration', 'distance']")
    return {"locations": [[float(p[0]), float(p[1])] for p in locs], "sources": src, "destinations": dst,
            "metrics": [m for m in METRICS if m in metrics]}


def _cells(a: np.ndarray) -> List[List[Any]]:
    return [[float(x) if math.isfinite(x) else None for x in row] for row in a.tolist()]


def matrix_response(provider, data: Any, ctx=None, device=None) -> Dict[str, Any]:
    """The endpoint's answer for a road-graph provider (``routing.graph.GraphProvider``)."""
    from .avoid import check_provider
    from .cch import RouteContext
    req = parse_request(data)
    g = provider.g
    ctx = ctx or RouteContext()
    check_provider(provider, ctx)
    sec, met, nodes, snap = provider.matrix_rect([{"lon": p[0], "lat": p[1]} for p in req["locations"]],
                                                 req["sources"], req["destinations"], ctx=ctx, device=device)

    def point(i: int) -> Dict[str, Any]:
        n = int(nodes[i])
        return {"location": [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)], "node": n,
                "snapped_distance": float(snap[i])}

    out: Dict[str, Any] = {}
    if "duration" in req["metrics"]:
        out["durations"] = _cells(sec)
    if "distance" in req["metrics"]:
        out["distances"] = _cells(met)
    out["sources"] = [point(i) for i in req["sources"]]
    out["destinations"] = [point(i) for i in req["destinations"]]
    out["metadata"] = {"engine": "cch", "context": {"weather": int(ctx.weather), "congestion": int(ctx.congestion),
                                                    "weekhour": int(ctx.weekhour)}}
    if ctx.avoid is not None:
        out["metadata"]["context"]["avoid"] = ctx.avoid.summary()
    return out
