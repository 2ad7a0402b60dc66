"""Shared inputs of the edge-mode map-matching tests (test_map_match_edge_cpu.py,
test_map_match_edge_gpu.py): raw edge sets in quantized centimetres (the hand-built tie set, a dense
patch), fixes along edges, the survivor count the GPU kernel's LDS buffer sees, and a brute force
for the route centimetres between two points on edges."""
import heapq

import numpy as np

import _mapmatch_cases as cases  # noqa: F401  (re-exported for the tests)
from routest_amd.routing import mapmatch_edge as me

Y0, X0 = 162_000_000, 1_300_000_000
SPAN = 1 << 22


def raw_edges(qy, qx, uvl):
    """(nqy, nqx, edge records, {(u, v): edge id}) of a hand-built edge list [(u, v, metres)]."""
    nqy, nqx = np.asarray(qy, np.int64), np.asarray(qx, np.int64)
    uvl = sorted(uvl, key=lambda t: (t[0], t[1]))
    u = np.array([t[0] for t in uvl])
    indptr = np.zeros(len(nqy) + 1, np.int32)
    np.cumsum(np.bincount(u, minlength=len(nqy)), out=indptr[1:])
    indices = np.array([t[1] for t in uvl], np.int32)
    length = np.array([t[2] for t in uvl], np.float32)
    return nqy, nqx, me.edge_records(nqy, nqx, indptr, indices, length), {(t[0], t[1]): i for i, t in enumerate(uvl)}


def tie_edges():
    """Street 0-1 in both directions and the one-way 2->3 parallel to it 20 m north (a fix half way
    between is equidistant from all three); a zero-length edge 4->4 far from everything; 5->6 exactly
    2^22 cm long and 7->8 one centimetre longer (unmatchable)."""
    qy = Y0 + np.array([0, 0, 2000, 2000, 500_000, 1_000_000, 1_000_000, 1_500_000, 1_500_000])
    qx = X0 + np.array([0, 10_000, 0, 10_000, 500_000, 0, SPAN, 0, SPAN + 1])
    return raw_edges(qy, qx, [(0, 1, 100.0), (1, 0, 100.0), (2, 3, 100.0), (4, 4, 0.0), (5, 6, 41943.04),
                             (7, 8, 41943.05)])


def tie_fixes(R=25_000):
    """(py, px) of the fixes that go with :func:`tie_edges` at radius ``R``."""
    Y, X = Y0, X0
    fixes = [(Y + 1000, X + 5000),             # 0: half way between the two streets: three edges at 1000 cm
             (Y, X - 500),                     # 1: before the tail of 0->1 (beyond the head of 1->0)
             (Y, X + 10_500),                  # 2: beyond the head of 0->1
             (Y + 300, X + 2500),              # 3: strictly inside
             (Y + 500_000 + R, X + 500_000),   # 4: exactly the radius from the zero-length edge
             (Y + 500_000 + R, X + 500_001),   # 5: radius² + 1
             (Y + 1_000_000 + 7, X + SPAN // 2),   # 6: on the edge of exactly 2^22 cm
             (Y + 1_500_000 + 7, X + SPAN // 2)]   # 7: on the edge 1 cm over: never a candidate
    return np.array([f[0] for f in fixes], np.int64), np.array([f[1] for f in fixes], np.int64)


def check_tie_answers(eid, out, k, R=25_000):
    """The answers :func:`tie_fixes` must get (``out`` = cand_edge, cand_d2, cand_fq, n_cand)."""
    ONE = me.ONE
    a, b, c = eid[(0, 1)], eid[(1, 0)], eid[(2, 3)]
    ce, cd2, cfq, nc = out[:4]
    assert nc[0] == min(k, 3) and ce[0, :nc[0]].tolist() == [a, b, c][:k] and (cd2[0, :nc[0]] == 1000 ** 2).all()
    assert cfq[0, :nc[0]].tolist() == [ONE // 2] * nc[0]
    assert (ce[1, 0], cd2[1, 0], cfq[1, 0]) == (a, 500 ** 2, 0) and (ce[1, 1], cfq[1, 1]) == (b, ONE)
    assert (ce[2, 0], cd2[2, 0], cfq[2, 0]) == (a, 500 ** 2, ONE) and (ce[2, 1], cfq[2, 1]) == (b, 0)
    assert (ce[3, 0], cd2[3, 0], cfq[3, 0]) == (a, 300 ** 2, ONE // 4) and cfq[3, 1] == 3 * ONE // 4
    assert nc[4] == 1 and (ce[4, 0], cd2[4, 0], cfq[4, 0]) == (eid[(4, 4)], R * R, 0)
    assert nc[5] == 0
    assert nc[6] == 1 and (ce[6, 0], cd2[6, 0], cfq[6, 0]) == (eid[(5, 6)], 49, ONE // 2)
    assert nc[7] == 0


def dense_patch(seed=4, n=4000, side=200_000, reach=3000):
    """About ``n`` short edges (each axis of w within +-``reach`` cm) in a ``side`` cm square."""
    rng = np.random.default_rng(seed)
    ty, tx = rng.integers(0, side, n), rng.integers(0, side, n)
    hy = np.clip(ty + rng.integers(-reach, reach + 1, n), 0, side)
    hx = np.clip(tx + rng.integers(-reach, reach + 1, n), 0, side)
    qy = Y0 + np.concatenate([ty, hy])
    qx = X0 + np.concatenate([tx, hx])
    return raw_edges(qy, qx, [(i, n + i, 10.0 + i % 7) for i in range(n)])


def survivors(grid, edges, py, px, radius_cm):
    """Per fix the number of entries of ``items`` in the cells the radius covers whose edge projects
    within the radius: what the candidate kernel compacts (an edge counts once per covered cell that
    lists it)."""
    out = np.zeros(len(py), np.int64)
    r = int(radius_cm)
    for p, (y, x) in enumerate(zip(np.asarray(py).tolist(), np.asarray(px).tolist())):
        ylo, yhi, xlo, xhi = y - r - grid["y0"], y + r - grid["y0"], x - r - grid["x0"], x + r - grid["x0"]
        if yhi < 0 or xhi < 0:
            continue
        cy0, cx0 = max(ylo, 0) // grid["cell"], max(xlo, 0) // grid["cell"]
        if cy0 >= grid["ny"] or cx0 >= grid["nx"]:
            continue
        cy1, cx1 = min(yhi // grid["cell"], grid["ny"] - 1), min(xhi // grid["cell"], grid["nx"] - 1)
        it = np.concatenate([grid["items"][grid["start"][cy * grid["nx"] + cx0]:grid["start"][cy * grid["nx"] + cx1 + 1]]
                             for cy in range(cy0, cy1 + 1)])
        ay, ax, wy, wx = (edges[n][it] for n in ("ay", "ax", "wy", "wx"))
        near = ((y >= ay + np.minimum(wy, 0) - r) & (y <= ay + np.maximum(wy, 0) + r)
                & (x >= ax + np.minimum(wx, 0) - r) & (x <= ax + np.maximum(wx, 0) + r))
        d2, _, _, _ = me.project(ay, ax, wy, wx, np.where(near, y, ay), np.where(near, x, ax))
        out[p] = int((near & (d2 <= r * r)).sum())
    return out


def radius_for_survivors(grid, edges, y, x, want, hi=100_000):
    """The smallest radius at which the fix has at least ``want`` survivors (the count only grows
    with the radius), and the count there."""
    lo = 1
    while lo < hi:
        mid = (lo + hi) // 2
        if survivors(grid, edges, [y], [x], mid)[0] >= want:
            hi = mid
        else:
            lo = mid + 1
    return lo, int(survivors(grid, edges, [y], [x], lo)[0])


def scan_one(edges, y, x, radius_cm, k):
    """One fix against every edge in plain Python integers: [(d2, edge, fq)] ascending, at most k."""
    found = []
    for e in np.flatnonzero(edges["ok"]).tolist():
        ay, ax, wy, wx = (int(edges[n][e]) for n in ("ay", "ax", "wy", "wx"))
        L2 = wy * wy + wx * wx
        f = min(max((y - ay) * wy + (x - ax) * wx, 0), L2)
        fq = (f << 16) // L2 if L2 else 0
        qy, qx = ay + ((wy * fq + 32768) >> 16), ax + ((wx * fq + 32768) >> 16)
        d2 = (y - qy) ** 2 + (x - qx) ** 2
        if d2 <= radius_cm * radius_cm:
            found.append((d2, e, fq))
    return sorted(found)[:k]


def fixes_on_edges(g, eids, frac):
    """(lat, lon) fixes exactly on the given CSR edges at the given fractions of the way."""
    tail = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))[eids]
    head = g.indices[eids]
    lat = g.lat[tail] + (g.lat[head] - g.lat[tail]) * frac
    lon = g.lon[tail] + (g.lon[head] - g.lon[tail]) * frac
    return np.stack([lat, lon], axis=1)


def edge_id(g, u, v):
    lo, hi = g.indptr[u], g.indptr[u + 1]
    j = lo + int(np.searchsorted(g.indices[lo:hi], v))
    assert j < hi and g.indices[j] == v
    return int(j)


def fixes_along(g, path, frac=0.5, every=1):
    """Noise-free fixes along a node path: one at fraction ``frac`` of every ``every``-th edge of
    the path.  Returns (fixes [m, 2] as (lat, lon), the edges they lie on, all edges of the path)."""
    all_e = np.array([edge_id(g, int(a), int(b)) for a, b in zip(path[:-1], path[1:])])
    on = all_e[::every]
    return fixes_on_edges(g, on, frac), on, all_e


# ------------------------------------------------------------------------------ route centimetres
def small_cost_graph(seed, n=9, m=22, costs=(1,)):
    """A small directed graph with edge costs drawn from ``costs`` and lengths proportional to them
    (50 m per unit), so that every time-shortest path is also a shortest one and equal-time ties
    carry equal metres; nodes 0..n-2 are joined at random, node n-1 only has an edge out (nothing
    reaches it).  Returns (indptr, indices, cost f32, length f32)."""
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < m:
        u, v = rng.integers(0, n - 1, 2)
        if u != v:
            pairs.add((int(u), int(v)))
    for u, v in list(pairs)[:4]:
        pairs.add((v, u))                          # a few two-way streets: U-turn pairs
    pairs.add((n - 1, 0))
    pairs = sorted(pairs)
    c = rng.choice(np.asarray(costs, np.float32), len(pairs)).astype(np.float32)
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount([u for u, _ in pairs], minlength=n), out=indptr[1:])
    return indptr, np.array([v for _, v in pairs], np.int32), c, (c * 50.0).astype(np.float32)


def brute_route_cm(indptr, indices, lc, e1, off1, e2, off2):
    """Centimetres of the shortest way from the point ``off1`` along edge ``e1`` to the point
    ``off2`` along ``e2`` by Dijkstra over the graph with the two points inserted as nodes X and Y
    (X leaves only forward along e1, Y is entered only along e2); -1 without a way."""
    n = len(indptr) - 1
    tail = np.repeat(np.arange(n), np.diff(indptr))
    X, Y = n, n + 1
    adj = {v: [] for v in range(n + 2)}
    for e in range(len(indices)):
        adj[int(tail[e])].append((int(indices[e]), int(lc[e])))
    adj[X].append((int(indices[e1]), int(lc[e1]) - off1))
    adj[int(tail[e2])].append((Y, off2))
    if e1 == e2 and off2 >= off1:
        adj[X].append((Y, off2 - off1))
    dist = {X: 0}
    heap = [(0, X)]
    while heap:
        d, v = heapq.heappop(heap)
        if d > dist.get(v, 1 << 62):
            continue
        if v == Y:
            return d
        for w, c in adj[v]:
            if d + c < dist.get(w, 1 << 62):
                dist[w] = d + c
                heapq.heappush(heap, (d + c, w))
    return -1
