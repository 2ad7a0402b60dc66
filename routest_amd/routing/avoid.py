"""Avoid areas of a routing context (OpenRouteService ``options.avoid_polygons``).

One definition, implemented three times (here in numpy on int64 — the reference; on the host in
``csrc/runtime/avoid.h``; on the GPU in ``csrc/cch_avoid.hip``):

* coordinates are quantized once to integer microdegrees, ``q(x) = rint(x * 1e6)`` in float64
  (round-half-even), graph nodes and polygon vertices alike; x = longitude, y = latitude;
* an avoid set is a list of polygons, a polygon a list of rings (outer ring, then holes); a point
  is inside a polygon by the even-odd rule over its rings; polygons are OR-ed;
* a directed edge u -> v is closed iff the closed segment q(u)-q(v) has a point in the closed region
  of some polygon: it meets a ring edge (touching and collinear overlap count), or q(u) is strictly
  inside by crossing number.  Differences stay below 2^29, cross products below 2^58, so every
  orientation test is exact in int64.

A closed edge costs ``+inf``: the customization treats it as absent (csrc/runtime/cch.h).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, List, Tuple

import numpy as np

MAX_POLYGONS = 64
MAX_RINGS = 256
MAX_VERTICES = 2048


def quantize(x) -> np.ndarray:
    """Microdegrees as int32: rint(x * 1e6) in float64."""
    return np.rint(np.asarray(x, dtype=np.float64) * 1e6).astype(np.int32)


def _fnv1a31(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    d = (h ^ (h >> 31) ^ (h >> 62)) & 0x7FFFFFFF
    return d or 1


@dataclass(frozen=True)
class AvoidSet:
    """Canonical form of an avoid set.  ``blob``: the bytes of a little-endian int32 array
    ``[P, R, V, rings of polygon 0..P-1, vertices of ring 0..R-1, x0, y0, x1, y1, ...]`` in request
    order, closing vertices dropped; ``digest``: FNV-1a-64 of those bytes folded to 31 bits
    (0 -> 1), the part of a context key that stands for the set."""
    blob: bytes
    digest: int

    @classmethod
    def from_rings(cls, polygons: List[List[np.ndarray]]) -> "AvoidSet":
        """``polygons[p][r]``: int [n, 2] quantized (x, y) vertices, already validated."""
        head = [len(polygons), sum(len(p) for p in polygons), sum(len(r) for p in polygons for r in p)]
        head += [len(p) for p in polygons]
        head += [len(r) for p in polygons for r in p]
        parts = [np.asarray(head, dtype="<i4")]
        parts += [np.asarray(r, dtype="<i4").reshape(-1) for p in polygons for r in p]
        blob = np.concatenate(parts).astype("<i4").tobytes()
        return cls(blob=blob, digest=_fnv1a31(blob))

    @classmethod
    def from_geojson(cls, obj: Any) -> "AvoidSet":
        """A GeoJSON ``Polygon`` or ``MultiPolygon`` object -> its avoid set; ``ValueError`` naming
        the offending part for anything else."""
        if not isinstance(obj, dict):
            raise ValueError("avoid_polygons: a GeoJSON Polygon or MultiPolygon object")
        kind, coords = obj.get("type"), obj.get("coordinates")
        if kind == "Polygon":
            coords = [coords]
        elif kind != "MultiPolygon":
            raise ValueError("avoid_polygons.type: 'Polygon' or 'MultiPolygon'")
        if not isinstance(coords, list) or not coords:
            raise ValueError("avoid_polygons.coordinates: a non-empty list")
        if len(coords) > MAX_POLYGONS:
            raise ValueError(f"avoid_polygons: at most {MAX_POLYGONS} polygons")
        polys: List[List[np.ndarray]] = []
        rings = verts = 0
        for pi, poly in enumerate(coords):
            if not isinstance(poly, list) or not poly:
                raise ValueError(f"avoid_polygons: polygon {pi}: a non-empty list of rings")
            out = []
            for ri, ring in enumerate(poly):
                where = f"avoid_polygons: polygon {pi} ring {ri}"
                if not isinstance(ring, list):
                    raise ValueError(f"{where}: a list of [lon, lat] positions")
                pts = []
                for vi, pos in enumerate(ring):
                    if (not isinstance(pos, (list, tuple)) or len(pos) < 2
                            or any(isinstance(c, bool) or not isinstance(c, (int, float)) for c in pos[:2])):
                        raise ValueError(f"{where} vertex {vi}: [lon, lat] numbers")
                    lon, lat = float(pos[0]), float(pos[1])
                    if not (math.isfinite(lon) and math.isfinite(lat)):
                        raise ValueError(f"{where} vertex {vi}: not finite")
                    if not (-180.0 <= lon <= 180.0 and -90.0 <= lat <= 90.0):
                        raise ValueError(f"{where} vertex {vi}: longitude in [-180, 180], latitude in [-90, 90]")
                    pts.append((lon, lat))
                q = quantize(np.asarray(pts, dtype=np.float64).reshape(-1, 2))
                if len(q) > 1 and (q[0] == q[-1]).all():
                    q = q[:-1]
                if len(q) < 3:
                    raise ValueError(f"{where}: at least 3 vertices")
                out.append(q)
                rings += 1
                verts += len(q)
                if rings > MAX_RINGS:
                    raise ValueError(f"avoid_polygons: at most {MAX_RINGS} rings")
                if verts > MAX_VERTICES:
                    raise ValueError(f"avoid_polygons: at most {MAX_VERTICES} vertices")
            polys.append(out)
        return cls.from_rings(polys)

    # ---- views ----
    @property
    def array(self) -> np.ndarray:
        return np.frombuffer(self.blob, dtype="<i4")

    @property
    def polygons(self) -> int:
        return int(self.array[0])

    @property
    def vertices(self) -> int:
        return int(self.array[2])

    def rings(self) -> List[List[np.ndarray]]:
        a = self.array
        P, R = int(a[0]), int(a[1])
        nring = a[3:3 + P]
        nvert = a[3 + P:3 + P + R]
        xy = a[3 + P + R:].reshape(-1, 2).astype(np.int64)
        out, r, v = [], 0, 0
        for p in range(P):
            rs = []
            for _ in range(int(nring[p])):
                rs.append(xy[v:v + int(nvert[r])])
                v += int(nvert[r])
                r += 1
            out.append(rs)
        return out

    def summary(self) -> dict:
        """The small object responses carry."""
        return {"polygons": self.polygons, "vertices": self.vertices}


def parse_options(data: Any):
    """``options.avoid_polygons`` of a request body -> :class:`AvoidSet` or None (absent / null);
    ``ValueError`` for a malformed one."""
    opt = data.get("options") if isinstance(data, dict) else None
    if not isinstance(opt, dict):
        return None
    ap = opt.get("avoid_polygons")
    return None if ap is None else AvoidSet.from_geojson(ap)


NEEDS_CCH = ("options.avoid_polygons needs the context-aware road router: start the service with "
             "ROUTEST_PROVIDER=graph and the CCH router (not ROUTEST_ROUTER=astar or fixed edge costs)")


def check_provider(provider, ctx) -> None:
    """``ValueError`` (a 400) when a context carries an avoid set the provider cannot honour."""
    if ctx is not None and getattr(ctx, "avoid", None) is not None and not getattr(provider, "uses_context", False):
        raise ValueError(NEEDS_CCH)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _on(ax, ay, bx, by, cx, cy):
    """c within the bounding box of a-b (with orient == 0: on the segment)."""
    return ((np.minimum(ax, bx) <= cx) & (cx <= np.maximum(ax, bx))
            & (np.minimum(ay, by) <= cy) & (cy <= np.maximum(ay, by)))


def edge_endpoints(g) -> Tuple[np.ndarray, np.ndarray]:
    src = np.repeat(np.arange(g.num_nodes, dtype=np.int64), np.diff(np.asarray(g.indptr, dtype=np.int64)))
    return src, np.asarray(g.indices, dtype=np.int64)


def avoid_mask(g, avoid: AvoidSet) -> np.ndarray:
    """uint8 [E]: 1 where the directed edge is closed by the avoid set (the reference)."""
    qx = quantize(g.lon).astype(np.int64)
    qy = quantize(g.lat).astype(np.int64)
    u, v = edge_endpoints(g)
    ax, ay, bx, by = qx[u], qy[u], qx[v], qy[v]
    closed = np.zeros(len(u), dtype=bool)
    for poly in avoid.rings():
        allv = np.concatenate(poly)
        x0, y0, x1, y1 = allv[:, 0].min(), allv[:, 1].min(), allv[:, 0].max(), allv[:, 1].max()
        cand = ((np.maximum(ax, bx) >= x0) & (np.minimum(ax, bx) <= x1)
                & (np.maximum(ay, by) >= y0) & (np.minimum(ay, by) <= y1) & ~closed)
        idx = np.nonzero(cand)[0]
        if not len(idx):
            continue
        Ax, Ay, Bx, By = ax[idx], ay[idx], bx[idx], by[idx]
        hit = np.zeros(len(idx), dtype=bool)
        par = np.zeros(len(idx), dtype=bool)
        for ring in poly:
            nxt = np.roll(ring, -1, axis=0)
            for (px, py), (sx, sy) in zip(ring, nxt):
                d1 = _orient(px, py, sx, sy, Ax, Ay)
                d2 = _orient(px, py, sx, sy, Bx, By)
                d3 = _orient(Ax, Ay, Bx, By, px, py)
                d4 = _orient(Ax, Ay, Bx, By, sx, sy)
                hit |= ((((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0)))
                        & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0))))
                hit |= (d1 == 0) & _on(px, py, sx, sy, Ax, Ay)
                hit |= (d2 == 0) & _on(px, py, sx, sy, Bx, By)
                hit |= (d3 == 0) & _on(Ax, Ay, Bx, By, px, py)
                hit |= (d4 == 0) & _on(Ax, Ay, Bx, By, sx, sy)
                # crossing number of the ray from A towards +x (half-open in y)
                par ^= ((py > Ay) != (sy > Ay)) & ((d1 > 0) == (sy > py)) & (d1 != 0)
        closed[idx] |= hit | par
    return closed.astype(np.uint8)
