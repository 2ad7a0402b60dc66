"""Isochrones: the request / response shape of ``POST /api/isochrones`` and the polygons around the
reached nodes (host side; the reached sets come from ``GraphProvider.reachable``, one one-to-all
call of the CCH router, csrc/cch_all.hip).

Request (OpenRouteService's isochrones shape)::

    {"locations": [[lon, lat], ...], "range": [seconds or metres, ...],
     "range_type": "time" | "distance", "location_type": "start" | "destination",
     "context": {"weather": ..., "traffic": ..., "pickup_time": ...}}

Response: a GeoJSON FeatureCollection, one Feature per (location, range), locations outermost.
``properties``: ``group_index`` (the location), ``value`` (the range), ``center`` ([lon, lat] of
the snapped node), ``reached_nodes`` and ``reach_m`` (metres of streets with both ends reached).

Geometry: a ``MultiPolygon`` from a grid over the graph's bounding box with ``cell_m``-metre cells
(default 2 x the median edge length, so neighbouring reached nodes land in touching cells): the
cells that hold a reached node are marked, the mask is dilated by one cell (8-neighbourhood) and
the outer rings of the result are traced.  HOLES ARE DROPPED: an unreached pocket inside a reached
area is covered by its polygon.  A larger range's mask contains a smaller range's, cell for cell.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

MAX_LOCATIONS = 64
MAX_RANGES = 10
MAX_CELLS = 1 << 22          # grid cells of one request (a cell_m far below the street spacing)

_M_PER_DEG = 111_320.0


class Grid:
    """``cell_m`` cells over the graph's bounding box (equirectangular around its mid latitude),
    one cell of margin on every side so a dilated mask never touches the border."""

    def __init__(self, g, cell_m: float):
        self.cell_m = float(cell_m)
        self.lon0, self.lat0 = float(np.min(g.lon)), float(np.min(g.lat))
        mid = 0.5 * (self.lat0 + float(np.max(g.lat)))
        self.kx = _M_PER_DEG * math.cos(math.radians(mid)) / self.cell_m     # cells per degree of longitude
        self.ky = _M_PER_DEG / self.cell_m
        self.col = np.floor((np.asarray(g.lon, np.float64) - self.lon0) * self.kx).astype(np.int64) + 2
        self.row = np.floor((np.asarray(g.lat, np.float64) - self.lat0) * self.ky).astype(np.int64) + 2
        self.w = int(self.col.max()) + 3
        self.h = int(self.row.max()) + 3

    def mask(self, node_ids: np.ndarray) -> np.ndarray:
        """bool [h, w]: the cells that hold one of the nodes, dilated by one cell (8-neighbourhood)."""
        m = np.zeros((self.h, self.w), dtype=bool)
        m[self.row[node_ids], self.col[node_ids]] = True
        out = np.zeros_like(m)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                out[1 + dr:self.h - 1 + dr, 1 + dc:self.w - 1 + dc] |= m[1:-1, 1:-1]
        return out

    def lonlat(self, x: float, y: float) -> List[float]:
        """Grid corner (x, y) -> [lon, lat] (6 decimals, like the route geometries)."""
        return [round(self.lon0 + (x - 2) / self.kx, 6), round(self.lat0 + (y - 2) / self.ky, 6)]


def outer_rings(mask: np.ndarray) -> List[List[Tuple[int, int]]]:
    """Outer boundary rings of the mask's cells as grid-corner (x, y) lists, counter-clockwise, closed
    (first == last), corners only.  Boundary edges run with the mask on their left; where two cells
    touch only at a corner the walk turns left (stays on its cell), so rings never cross.  Rings
    with negative area are the holes and are dropped."""
    h, w = mask.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = mask
    c = p[1:-1, 1:-1]
    nxt: Dict[Tuple[int, int], List[Tuple[int, int]]] = {}

    def add(rr, cc, x0, y0, dx, dy):
        for r, q in zip(rr.tolist(), cc.tolist()):
            nxt.setdefault((q + x0, r + y0), []).append((dx, dy))

    add(*np.nonzero(c & ~p[:-2, 1:-1]), 0, 0, 1, 0)       # bottom edge, heading +x
    add(*np.nonzero(c & ~p[1:-1, 2:]), 1, 0, 0, 1)        # right edge, heading +y
    add(*np.nonzero(c & ~p[2:, 1:-1]), 1, 1, -1, 0)       # top edge, heading -x
    add(*np.nonzero(c & ~p[1:-1, :-2]), 0, 1, 0, -1)      # left edge, heading -y
    rings = []
    for start in list(nxt):
        while nxt.get(start):
            d = nxt[start].pop()
            ring = [start]
            v = (start[0] + d[0], start[1] + d[1])
            area2 = start[0] * v[1] - v[0] * start[1]
            while v != start:
                outs = nxt[v]
                for cand in ((-d[1], d[0]), d, (d[1], -d[0])):     # left, straight, right
                    if cand in outs:
                        break
                outs.remove(cand)
                if cand != d:
                    ring.append(v)
                d = cand
                u = (v[0] + d[0], v[1] + d[1])
                area2 += v[0] * u[1] - u[0] * v[1]
                v = u
            ring.append(start)
            if area2 > 0:
                rings.append(ring)
    return rings


def multipolygon(grid: Grid, node_ids: np.ndarray) -> Dict[str, Any]:
    if len(node_ids) == 0:
        return {"type": "MultiPolygon", "coordinates": []}
    return {"type": "MultiPolygon",
            "coordinates": [[[grid.lonlat(x, y) for x, y in ring]] for ring in outer_rings(grid.mask(node_ids))]}


def _number(x: Any) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)


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
    rng = data.get("range")
    if not isinstance(rng, list) or not rng:
        raise ValueError("range: a non-empty list of seconds or metres")
    if len(rng) > MAX_RANGES:
        raise ValueError(f"range: at most {MAX_RANGES} values")
    if not all(_number(r) and r > 0 for r in rng):
        raise ValueError("range: positive numbers")
    rtype = data.get("range_type", "time")
    if rtype not in ("time", "distance"):
        raise ValueError("range_type: 'time' or 'distance'")
    ltype = data.get("location_type", "start")
    if ltype not in ("start", "destination"):
        raise ValueError("location_type: 'start' or 'destination'")
    cell = data.get("cell_m")
    if cell is not None and not (_number(cell) and cell > 0):
        raise ValueError("cell_m: a positive number of metres")
    return {"locations": [[float(p[0]), float(p[1])] for p in locs], "range": [float(r) for r in rng],
            "range_type": rtype, "reverse": ltype == "destination", "cell_m": None if cell is None else float(cell)}


def isochrones(provider, data: Any, ctx=None, device=None) -> Dict[str, Any]:
    """The endpoint's answer for a road-graph provider (``routing.graph.GraphProvider``)."""
    from .graph import median_edge_m
    from .avoid import check_provider
    req = parse_request(data)
    check_provider(provider, ctx)
    g = provider.g
    cell_m = req["cell_m"]
    if cell_m is None:
        cell_m = getattr(provider, "_iso_cell_m", None)
        if cell_m is None:
            cell_m = provider._iso_cell_m = max(1.0, 2.0 * median_edge_m(g))
    span_m = _M_PER_DEG * max(float(np.ptp(g.lat)), float(np.ptp(g.lon)))
    if (span_m / cell_m + 5) ** 2 > MAX_CELLS:
        raise ValueError("cell_m: too small for this graph")
    grid = Grid(g, cell_m)
    reached = provider.reachable([{"lon": p[0], "lat": p[1]} for p in req["locations"]], req["range"],
                                 range_type=req["range_type"], reverse=req["reverse"], ctx=ctx, device=device)
    feats = []
    for r in reached:
        n = r["node"]
        feats.append({"type": "Feature", "geometry": multipolygon(grid, r["nodes"]),
                      "properties": {"group_index": r["point"], "value": r["value"],
                                     "center": [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)],
                                     "reached_nodes": r["reached_nodes"], "reach_m": round(r["reach_m"], 1)}})
    meta = {"range_type": req["range_type"], "location_type": "destination" if req["reverse"] else "start",
            "cell_m": cell_m}
    if getattr(ctx, "avoid", None) is not None:
        meta["avoid"] = ctx.avoid.summary()
    return {"type": "FeatureCollection", "features": feats, "metadata": meta}
