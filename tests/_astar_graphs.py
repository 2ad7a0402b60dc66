"""Small adversarial graphs for the batched A* (tests/test_astar_edges_cpu.py checks their
preconditions and the heuristic the kernel is given, tests/test_astar_edges_gpu.py runs the GPU tiers
on them).  The CCH fixtures (tests/_cch_graphs.py: islands, clique, ties) are reused; new here:

* oneway_patches: a 1,600-node grid with a 36-node source patch A (no edge enters it) and a 36-node
  sink patch B (no edge leaves it): landmarks that cannot reach a node, or be reached from it;
* straight: a 2,500-node grid whose edge lengths are the plain great-circle lengths (ratio 1.0, not
  the 1.15 the synthetic family has), with road-class speeds and a second, faster metric;
* chain: a 64-node path graph (unique shortest paths of known node counts);
* zero_cost: the ties grid with ~5 % of the streets free (cost 0.0 both ways), the rest in {1, 2, 3}.

Everything is numpy / scipy; references are cached per process so both test files share them.
"""
import dataclasses
import functools

import numpy as np

import _cch_graphs as C
from routest_amd.data.graph import build_graph, synth_road_graph
from routest_amd.routing.providers import haversine_m

U = 2.0 ** -24                                  # f32 unit roundoff
STRAIGHT_SPEED = np.array([8.0, 14.0, 25.0, 25.0])
EXACT = ("ties_ones", "ties_ints", "zero_cost")    # integer costs: f32 sums are exact
SINKS = (28, 84)                                # islands: the 2-node sink component


def src_of(g):
    return np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))


def _sub(g, keep, length=None):
    """g restricted to the edges in ``keep`` (bool per edge)."""
    s = src_of(g)
    indptr = np.zeros(g.num_nodes + 1, np.int32)
    np.cumsum(np.bincount(s[keep], minlength=g.num_nodes), out=indptr[1:])
    return dataclasses.replace(g, indptr=indptr, indices=g.indices[keep].astype(np.int32),
                               length_m=(g.length_m if length is None else length)[keep].astype(np.float32),
                               road_class=g.road_class[keep],
                               edge_name=None if g.edge_name is None else g.edge_name[keep])


def _box(g, lat0, lat1, lon0, lon1):
    la = (g.lat - g.lat.min()) / (g.lat.max() - g.lat.min())
    lo = (g.lon - g.lon.min()) / (g.lon.max() - g.lon.min())
    return (la >= lat0) & (la < lat1) & (lo >= lon0) & (lo < lon1)


@functools.lru_cache(maxsize=None)
def oneway_graph():
    """(graph, cost, in_a, in_b): synth_road_graph(1600, seed=4) without the edges entering patch A
    and without those leaving patch B; cost = length / 12."""
    g = synth_road_graph(1600, seed=4)
    in_a = _box(g, 0.2, 0.35, 0.2, 0.35)
    in_b = _box(g, 0.6, 0.75, 0.55, 0.7)
    s, t = src_of(g), g.indices
    keep = ~(~in_a[s] & in_a[t]) & ~(in_b[s] & ~in_b[t])
    g = _sub(g, keep)
    return g, (g.length_m / np.float32(12.0)).astype(np.float32), in_a, in_b


@functools.lru_cache(maxsize=None)
def straight_graph():
    """(graph, cost, faster): synth_road_graph(2500, seed=9) with length = great circle (f32) and
    cost = length / speed, speed (8, 14, 25, 25) m/s by road class; ``faster``: every speed x 1.5."""
    g = synth_road_graph(2500, seed=9)
    s = src_of(g)
    gc = haversine_m(g.lat[s], g.lon[s], g.lat[g.indices], g.lon[g.indices]).astype(np.float32)
    g = dataclasses.replace(g, length_m=gc)
    sp = STRAIGHT_SPEED[g.road_class]
    return g, (gc / sp).astype(np.float32), (gc / (1.5 * sp)).astype(np.float32)


CHAIN_N = 64


@functools.lru_cache(maxsize=None)
def chain_graph():
    """(graph, cost): nodes 0..63 along a meridian, edges i <-> i + 1; cost = length / 10."""
    i = np.arange(CHAIN_N - 1)
    g = build_graph(14.4 + 0.001 * np.arange(CHAIN_N), np.full(CHAIN_N, 121.0), i, i + 1,
                    np.zeros(CHAIN_N - 1, np.uint8), both_ways=True, seed=3)
    return g, (g.length_m / np.float32(10.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def zero_cost_graph():
    """(graph, cost): the ties grid, costs in {1, 2, 3}, ~5 % of the streets at 0.0 in both
    directions (so equal-cost cycles exist)."""
    g, _, ints = C.ties_graph()
    s, t = src_of(g).astype(np.int64), g.indices.astype(np.int64)
    street = np.minimum(s, t) * g.num_nodes + np.maximum(s, t)
    uniq = np.unique(street)
    free = uniq[np.random.default_rng(23).random(len(uniq)) < 0.05]
    cost = ints.copy()
    cost[np.isin(street, free)] = 0.0
    return g, cost


def fixture_metrics():
    """name -> (graph, cost) of every A* fixture metric."""
    go, co, _, _ = oneway_graph()
    gs, cs, cf = straight_graph()
    out = dict(C.fixture_metrics())
    out.update({"oneway_patches": (go, co), "straight": (gs, cs), "straight_fast": (gs, cf),
                "chain": chain_graph(), "zero_cost": zero_cost_graph()})
    return out


# ------------------------------------------------------------------------------------- references
def _csr(g, cost):
    from scipy.sparse import csr_matrix
    return csr_matrix((np.asarray(cost, np.float64), g.indices, g.indptr), shape=(g.num_nodes,) * 2)


@functools.lru_cache(maxsize=None)
def all_pairs(name):
    """float64 Dijkstra matrix [N, N] of a fixture metric (inf where there is no route)."""
    from scipy.sparse.csgraph import dijkstra
    g, cost = fixture_metrics()[name]
    return dijkstra(_csr(g, cost), directed=True)


def scc_sizes(g):
    from scipy.sparse.csgraph import connected_components
    _, lab = connected_components(_csr(g, np.ones(g.num_edges)), directed=True, connection="strong")
    return sorted(np.bincount(lab).tolist())


def reference(g, cost, src, dst):
    """(D, hops): float64 Dijkstra seconds per pair (inf: no route) and the edge count of scipy's
    predecessor path (-1: no route)."""
    from scipy.sparse.csgraph import dijkstra
    src, dst = np.asarray(src), np.asarray(dst)
    uniq, inv = np.unique(src, return_inverse=True)
    D = np.empty(len(src))
    hops = np.full(len(src), -1, np.int64)
    m = _csr(g, cost)
    for lo in range(0, len(uniq), 256):                    # bounded memory: 256 sources at a time
        dist, pred = dijkstra(m, directed=True, indices=uniq[lo:lo + 256], return_predecessors=True)
        for q in np.flatnonzero((inv >= lo) & (inv < lo + 256)):
            r = inv[q] - lo
            D[q] = dist[r, dst[q]]
            if np.isfinite(D[q]):
                n, v = 0, dst[q]
                while v != src[q]:
                    v = pred[r, v]
                    n += 1
                hops[q] = n
    return D, hops


def _mix(rng, parts):
    src = np.concatenate([p[0] for p in parts]).astype(np.int32)
    dst = np.concatenate([p[1] for p in parts]).astype(np.int32)
    o = rng.permutation(len(src))
    return src[o], dst[o]


def _uniform_pool(g, n, seed, same=16, dup=32):
    """n pairs: uniform random, ``same`` with s == t, ``dup`` repeated pairs, shuffled."""
    rng = np.random.default_rng(seed)
    k = n - same - dup
    s, t = rng.integers(0, g.num_nodes, k), rng.integers(0, g.num_nodes, k)
    e = rng.integers(0, g.num_nodes, same)
    return _mix(rng, [(s, t), (e, e), (s[:dup], t[:dup])])


@functools.lru_cache(maxsize=None)
def pool(name):
    """(src, dst, D, hops) of a fixture's query pool (shared by every metric of its graph except
    D / hops, which are per metric)."""
    g, cost = fixture_metrics()[name]
    if name == "oneway_patches":
        _, _, in_a, in_b = oneway_graph()
        rng = np.random.default_rng(31)
        A, B, R = np.flatnonzero(in_a), np.flatnonzero(in_b), np.flatnonzero(~in_a & ~in_b)
        pick = lambda X, n: X[rng.integers(0, len(X), n)]   # noqa: E731
        parts = [(pick(A, 300), pick(R, 300)), (pick(R, 300), pick(B, 300)), (pick(A, 200), pick(B, 200)),
                 (pick(R, 100), pick(A, 100)), (pick(B, 100), pick(R, 100)), (pick(B, 50), pick(A, 50))]
        e = pick(np.arange(g.num_nodes), 16)
        parts += [(e, e), (parts[0][0][:17], parts[0][1][:17]), (parts[3][0][:17], parts[3][1][:17])]
        src, dst = _mix(rng, parts)
    elif name == "islands":
        d = all_pairs("islands")
        parts = []
        for t in SINKS:                                    # every source with a route into the sink
            s = np.flatnonzero(np.isfinite(d[:, t]))
            parts.append((s, np.full(len(s), t)))
        ps, pd, _ = C.islands_pool()
        src, dst = _mix(np.random.default_rng(37), parts + [(ps[:1000], pd[:1000])])
    elif name in ("straight", "straight_fast"):
        src, dst = _uniform_pool(g, 1000, 41)
    elif name.startswith("clique"):
        src, dst = _uniform_pool(g, 1000, 43)
    elif name == "chain":
        src, dst = _uniform_pool(g, 500, 47)
    else:                                                  # the ties grid: ties_ones, ties_ints, zero_cost
        src, dst = _uniform_pool(g, 1000, 53)
    D, hops = reference(g, cost, src, dst)
    return src, dst, D, hops


@functools.lru_cache(maxsize=None)
def far_pairs(min_hops=130, n=32):
    """(src, dst, BFS edge count) of pairs of the ties grid at least ``min_hops`` edges apart: a
    corner and nodes around the opposite corner."""
    from scipy.sparse.csgraph import dijkstra
    g, _, _ = C.ties_graph()
    corners = np.array([0, g.cols - 1, g.num_nodes - g.cols, g.num_nodes - 1])
    bfs = dijkstra(_csr(g, np.ones(g.num_edges)), directed=True, indices=corners, unweighted=True)
    src, dst, hops = [], [], []
    for i, c in enumerate(corners):
        far = np.flatnonzero(bfs[i] >= min_hops)[: n // 4]
        src += [c] * len(far)
        dst += far.tolist()
        hops += bfs[i, far].tolist()
    return np.array(src, np.int32), np.array(dst, np.int32), np.array(hops, np.int64)


# ------------------------------------------------------------------------------------- the heuristic
def split_tables(lm):
    """[N, 2K] interleaved f32 tables -> (fwd [K, N], bwd [K, N]) float64: d(L_k -> v), d(v -> L_k)."""
    x = np.asarray(lm, np.float64).reshape(lm.shape[0], -1, 4)
    K = x.shape[1] * 2
    fwd = np.empty((K, lm.shape[0]))
    bwd = np.empty((K, lm.shape[0]))
    fwd[0::2], fwd[1::2] = x[:, :, 0].T, x[:, :, 1].T
    bwd[0::2], bwd[1::2] = x[:, :, 2].T, x[:, :, 3].T
    return fwd, bwd


def heuristic(g, factor, lm, targets):
    """h[v, j] the kernel's heuristic of node v towards targets[j], evaluated in float64 from what
    the kernel is given (csrc/astar.hip hdist / halt): max(0.999 * gc(v, t) * factor,
    0.9999 * max(0, max_k fwd_k(t) - fwd_k(v), max_k bwd_k(v) - bwd_k(t)))."""
    targets = np.asarray(targets)
    h = 0.999 * haversine_m(g.lat[:, None], g.lon[:, None], g.lat[targets][None, :],
                            g.lon[targets][None, :]) * float(factor)
    if lm is not None:
        fwd, bwd = split_tables(lm)
        alt = np.zeros_like(h)
        for k in range(fwd.shape[0]):
            np.maximum(alt, fwd[k][targets][None, :] - fwd[k][:, None], out=alt)
            np.maximum(alt, bwd[k][:, None] - bwd[k][targets][None, :], out=alt)
        np.maximum(h, 0.9999 * alt, out=h)
    return h


def heuristic_violations(g, cost, factor, lm, targets, dist):
    """(inadmissible pairs, worst excess, inconsistent (edge, target) pairs, h(t, t) != 0 count) of the
    heuristic against ``dist`` [N, len(targets)] (float64 Dijkstra), with the derived slack: the
    tables are f32 roundings of float64 distances, so 2 * 2^-24 * (largest table entry)."""
    h = heuristic(g, factor, lm, targets)
    slack = 2 * U * float(np.max(lm)) if lm is not None else 0.0
    fin = np.isfinite(dist)
    over = np.where(fin, h - np.where(fin, dist, 0.0), -np.inf)
    bad = over > slack
    s, t = src_of(g), g.indices
    c = np.asarray(cost, np.float64)
    incons = 0
    for lo in range(0, len(s), 4096):
        e = slice(lo, lo + 4096)
        incons += int((h[s[e]] > c[e, None] + h[t[e]] + slack).sum())
    return int(bad.sum()), float(over.max()) if bad.any() else 0.0, incons, int((h[targets, np.arange(len(targets))] != 0).sum())


# ------------------------------------------------------------------------------------- grading
def edge_keys(g):
    k = src_of(g).astype(np.int64) * g.num_nodes + g.indices
    assert (np.diff(k) > 0).all()                          # CSR sorted by (source, target), no parallel edges
    return k


def grade(g, cost, src, dst, D, hops, out, exact=False):
    """Compare (cost, len, status, path) arrays of a run with the reference.  Returns a dict of
    counts of queries violating: status (0 iff Dijkstra finite, else 1, with cost -1 and len 0),
    path (from s to t along edges; [s] with cost 0.0 where s == t), sum (cost == the f32
    left-to-right sum of the path's edge costs) and optimal (-(n-1) u D <= cost - D <=
    (n_d-1) u D 1.01, or cost == D when ``exact``); plus ``worst`` = max relative excess."""
    c, n, st, p = (np.asarray(x) for x in out)
    src, dst = np.asarray(src), np.asarray(dst)
    fin = np.isfinite(D)
    bad_status = (st != np.where(fin, 0, 1)) | ((st != 0) & ((c != -1) | (n != 0)))
    ok = np.flatnonzero((st == 0) & fin)
    keys = edge_keys(g)
    cost = np.asarray(cost, np.float32)
    bad_path = np.zeros(len(src), bool)
    bad_sum = np.zeros(len(src), bool)
    L = int(n[ok].max()) if len(ok) else 1
    steps = np.zeros((len(src), max(L - 1, 1)), np.float32)
    for q in ok:
        path = p[q, :n[q]].astype(np.int64)
        if n[q] < 1 or path[0] != src[q] or path[-1] != dst[q] or (path < 0).any() or (path >= g.num_nodes).any():
            bad_path[q] = True
            continue
        k = path[:-1] * g.num_nodes + path[1:]
        e = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        if (keys[e] != k).any():
            bad_path[q] = True
            continue
        steps[q, :len(e)] = cost[e]
    acc = np.zeros(len(src), np.float32)
    for j in range(steps.shape[1]):
        acc = (acc + steps[:, j]).astype(np.float32)       # adding the 0.0 padding is exact
    good = np.zeros(len(src), bool)
    good[ok] = True
    good &= ~bad_path
    bad_sum[good] = c[good] != acc[good]
    same = good & (src == dst)
    bad_path |= same & ((n != 1) | (c != 0.0))
    diff = c.astype(np.float64) - np.where(fin, D, 0.0)
    nh = np.maximum(n.astype(np.int64) - 2, 0)             # additions along the returned path
    nd = np.maximum(hops - 1, 0)
    Dz = np.where(fin, D, 0.0)
    if exact:
        bad_opt = good & (diff != 0)
    else:
        bad_opt = good & ((diff < -nh * U * Dz) | (diff > nd * U * Dz * 1.01))
    rel = np.where(good & (Dz > 0), diff / np.where(Dz > 0, Dz, 1.0), 0.0)
    return {"status": int(bad_status.sum()), "path": int(bad_path.sum()), "sum": int(bad_sum.sum()),
            "optimal": int(bad_opt.sum()), "worst": float(rel.max()) if len(rel) else 0.0}
