"""Avoid sets and small graphs shared by tests/test_cch_avoid_cpu.py and tests/test_cch_avoid_gpu.py.

The sets are placed by fractions of a graph's bounding box, so the same names work on every fixture
graph: a triangle; one ring of 2,048 vertices (the limit); 64 small polygons; 256 rings; a ring with
a hole; two overlapping boxes; a sliver thinner than the node spacing; everything; nothing.
"""
import functools

import numpy as np

from routest_amd.data.graph import build_graph
from routest_amd.routing.avoid import AvoidSet

SET_NAMES = ["triangle", "ring2048", "poly64", "rings256", "hole", "overlap", "sliver", "everything", "nothing"]


def box(x0, x1, y0, y1, close=True):
    r = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    return r + [r[0]] if close else r


def frac(g):
    x0, x1, y0, y1 = float(g.lon.min()), float(g.lon.max()), float(g.lat.min()), float(g.lat.max())
    return (lambda f: x0 + (x1 - x0) * f), (lambda f: y0 + (y1 - y0) * f)


def hole_geojson(g):
    """A square ring (0.3 .. 0.7 of the box) with a square hole (0.4 .. 0.6)."""
    fx, fy = frac(g)
    return {"type": "Polygon", "coordinates": [box(fx(.3), fx(.7), fy(.3), fy(.7)), box(fx(.4), fx(.6), fy(.4), fy(.6))]}


def geojson_sets(g):
    fx, fy = frac(g)
    out = {}
    out["triangle"] = {"type": "Polygon", "coordinates": [[[fx(.2), fy(.2)], [fx(.6), fy(.25)], [fx(.3), fy(.7)]]]}
    t = np.linspace(0.0, 2 * np.pi, 2048, endpoint=False)
    rad = 0.25 + 0.05 * np.cos(7 * t)
    out["ring2048"] = {"type": "Polygon", "coordinates": [[[fx(.5 + r * np.cos(a)), fy(.5 + r * np.sin(a))]
                                                            for a, r in zip(t, rad)]]}
    out["poly64"] = {"type": "MultiPolygon", "coordinates": [
        [box(fx(.05 + .11 * i), fx(.09 + .11 * i), fy(.05 + .11 * j), fy(.09 + .11 * j))]
        for i in range(8) for j in range(8)]}
    out["rings256"] = {"type": "MultiPolygon", "coordinates": [
        [box(fx(.05 + .11 * i), fx(.15 + .11 * i), fy(.05 + .11 * j), fy(.15 + .11 * j))] +
        [box(fx(.06 + .11 * i + .03 * k), fx(.08 + .11 * i + .03 * k), fy(.07 + .11 * j), fy(.13 + .11 * j), close=False)
         for k in range(3)]
        for i in range(8) for j in range(8)]}
    out["hole"] = hole_geojson(g)
    out["overlap"] = {"type": "MultiPolygon", "coordinates": [[box(fx(.2), fx(.5), fy(.2), fy(.5))],
                                                              [box(fx(.4), fx(.7), fy(.4), fy(.7))]]}
    xm = float(np.median(g.lon)) + 3e-6
    out["sliver"] = {"type": "Polygon", "coordinates": [box(xm, xm + 2e-6, fy(.1), fy(.9))]}
    out["everything"] = {"type": "Polygon", "coordinates": [box(fx(0) - .01, fx(1) + .01, fy(0) - .01, fy(1) + .01)]}
    out["nothing"] = {"type": "Polygon", "coordinates": [box(fx(1) + 1.0, fx(1) + 1.1, fy(1) + 1.0, fy(1) + 1.1)]}
    return out


def avoid_sets(g):
    return {k: AvoidSet.from_geojson(v) for k, v in geojson_sets(g).items()}


BASE_X, BASE_Y = 121.0, 14.5


@functools.lru_cache(maxsize=None)
def lattice_graph(E):
    """E directed edges on integer microdegree offsets around (121, 14.5): the first is zero-length in
    its quantized form (two nodes a nanodegree apart), the next ones run along y = 2 (collinear with
    the lattice set's lower ring edge) and along x = -3 (its left edge); the rest cross the box."""
    n = E + 1
    ox = np.zeros(n)
    oy = np.zeros(n)
    for i in range(n):
        if i < 2:
            ox[i], oy[i] = 0, 2                      # nodes 0, 1 coincide after quantization
        elif i % 3 == 0:
            ox[i], oy[i] = -6 + (i * 5) % 13, 2      # on the line y = 2
        elif i % 3 == 1:
            ox[i], oy[i] = -3, -6 + (i * 7) % 13     # on the line x = -3
        else:
            ox[i], oy[i] = -6 + (i * 3) % 13, -6 + (i * 11) % 13
    lon = BASE_X + ox * 1e-6
    lat = BASE_Y + oy * 1e-6
    lat[1] += 1e-9
    s = np.arange(E)
    d = np.arange(1, E + 1)
    g = build_graph(lat, lon, s, d, np.zeros(E, np.uint8), length_m=np.full(E, 10.0, np.float32), seed=3)
    assert g.num_edges == E
    return g


def lattice_set():
    """The box [-3, 3] x [2, 5] in microdegree offsets with a hole [-1, 1] x [3, 4]."""
    def b(x0, x1, y0, y1):
        return box(BASE_X + x0 * 1e-6, BASE_X + x1 * 1e-6, BASE_Y + y0 * 1e-6, BASE_Y + y1 * 1e-6)
    return AvoidSet.from_geojson({"type": "Polygon", "coordinates": [b(-3, 3, 2, 5), b(-1, 1, 3, 4)]})


def path_edges(g, path):
    """Edge ids along a node path (the cheapest is not needed: the fixture graphs have no parallel edges)."""
    out = []
    for u, v in zip(path[:-1], path[1:]):
        nb = g.indices[g.indptr[u]:g.indptr[u + 1]]
        k = np.flatnonzero(nb == v)
        assert len(k) >= 1, (u, v)
        out.append(int(g.indptr[u] + k[0]))
    return np.asarray(out, dtype=np.int64)


def without_edges(g, drop):
    """(graph without the edges where ``drop``, old edge id of each kept edge)."""
    import dataclasses
    keep = ~np.asarray(drop, dtype=bool)
    src = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    indptr = np.zeros(g.num_nodes + 1, np.int32)
    np.cumsum(np.bincount(src[keep], minlength=g.num_nodes), out=indptr[1:])
    g2 = dataclasses.replace(g, indptr=indptr, indices=g.indices[keep].astype(np.int32),
                             length_m=g.length_m[keep].astype(np.float32), road_class=g.road_class[keep],
                             edge_name=None if g.edge_name is None else g.edge_name[keep])
    return g2, np.flatnonzero(keep)
