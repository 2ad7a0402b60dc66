"""Small adversarial graphs for the CCH pair queries (tests/test_cch_edges_cpu.py checks their
preconditions on the CPU reference, tests/test_cch_edges_gpu.py runs the GPU kernels on them).

* islands: one-way streets and two disconnected halves (infinite arc weights, unreachable pairs in
  one elimination tree and across two, every path edge count 0..48);
* clique: the complete directed graph on 321 nodes (one chain of 321 consecutive ranks, nodes with
  more than 256 kept arcs), a metric that keeps every arc and one that prunes two thirds;
* ties: a 6,400-node grid with unit costs and with costs in {1, 2, 3} (exact f32 sums, most queries
  have several shortest paths).

Everything is numpy; the CPU reference objects are cached per process so both test files share them.
"""
import dataclasses
import functools

import numpy as np

from routest_amd.data.graph import build_graph, synth_road_graph

CLIQUE_N = 321
POOL = 4000
EDGE_COUNTS = 49            # path edge counts 0..48 must all occur among the islands pool


@functools.lru_cache(maxsize=None)
def islands_graph():
    """(graph, cost): synth_road_graph(3000, seed=7) with ~30 % of the streets one-way and every edge
    across the middle column band removed; cost = length / 12."""
    g = synth_road_graph(3000, seed=7)
    rng = np.random.default_rng(1)
    src_of = np.repeat(np.arange(g.num_nodes), np.diff(g.indptr))
    keep = np.ones(g.num_edges, bool)
    # drop one direction of ~30% of the edges, only where the reverse exists (stay strongly connected
    # mostly; unreachable pairs are checked against Dijkstra's inf anyway)
    drop = rng.random(g.num_edges) < 0.3
    keep &= ~(drop & (src_of < g.indices))
    # cut the graph into two islands: remove every edge crossing the middle column band
    mid = (g.lon.min() + g.lon.max()) / 2
    cross = (g.lon[src_of] < mid) != (g.lon[g.indices] < mid)
    keep &= ~cross
    indptr = np.zeros(g.num_nodes + 1, np.int32)
    np.cumsum(np.bincount(src_of[keep], minlength=g.num_nodes), out=indptr[1:])
    length = g.length_m[keep].astype(np.float32)
    g = dataclasses.replace(g, indptr=indptr, indices=g.indices[keep].astype(np.int32), length_m=length,
                            road_class=g.road_class[keep],
                            edge_name=None if g.edge_name is None else g.edge_name[keep])
    return g, (length / 12.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clique_graph():
    """(graph, narrow, wide): the complete directed graph on 321 nodes.  narrow ~ U[1, 1.9): every
    direct edge beats every detour (1 + 1 > 1.9), so no arc is pruned; length = 10 * narrow.  wide ~
    U[1, 20) on the same topology (and the same lengths): about two thirds of the arcs are pruned."""
    n = CLIQUE_N
    rng = np.random.default_rng(11)
    lat = 14.5 + rng.uniform(0.0, 0.1, n)
    lon = 121.0 + rng.uniform(0.0, 0.1, n)
    s, d = np.divmod(np.arange(n * n), n)
    off = s != d
    s, d = s[off], d[off]                                  # sorted by (source, target): the CSR order
    narrow = rng.uniform(1.0, 1.9, len(s)).astype(np.float32)
    narrow = np.minimum(narrow, np.nextafter(np.float32(1.9), np.float32(0)))
    wide = rng.uniform(1.0, 20.0, len(s)).astype(np.float32)
    g = build_graph(lat, lon, s, d, np.zeros(len(s), np.uint8), length_m=np.float32(10.0) * narrow, seed=11)
    assert np.array_equal(g.indices, d) and g.num_edges == n * (n - 1)
    return g, narrow, wide


@functools.lru_cache(maxsize=None)
def ties_graph():
    """(graph, ones, ints): synth_road_graph(6400, seed=2) with every cost 1.0, and with integer
    costs drawn from {1, 2, 3}."""
    g = synth_road_graph(6400, seed=2)
    ones = np.ones(g.num_edges, np.float32)
    ints = np.random.default_rng(5).integers(1, 4, g.num_edges).astype(np.float32)
    return g, ones, ints


def perturbed(cost, seed=0):
    """cost * (1 + U[0, 1e-4)): breaks every tie without changing which paths are near-shortest."""
    u = np.random.default_rng(seed).uniform(0.0, 1e-4, len(cost))
    return (cost.astype(np.float64) * (1.0 + u)).astype(np.float32)


def fixture_metrics():
    """name -> (graph, cost) of every fixture metric."""
    gi, ci = islands_graph()
    gc, cn, cw = clique_graph()
    gt, c1, c3 = ties_graph()
    return {"islands": (gi, ci), "clique_narrow": (gc, cn), "clique_wide": (gc, cw), "ties_ones": (gt, c1),
            "ties_ints": (gt, c3)}


@functools.lru_cache(maxsize=None)
def cpu_cch(graph_name):
    """The CPU reference hierarchy of a fixture graph ("islands", "clique", "ties")."""
    from routest_amd import _rt
    g = {"islands": islands_graph, "clique": clique_graph, "ties": ties_graph}[graph_name]()[0]
    return _rt.CCH(g.indptr, g.indices, g.lat, g.lon, 0)


@functools.lru_cache(maxsize=None)
def cpu_metric(name):
    """(cpu hierarchy, customized metric) of a fixture metric."""
    g, cost = fixture_metrics()[name]
    c = cpu_cch(name.split("_")[0])
    return c, c.customize(cost, g.length_m)


def etree_roots(parent):
    """Root of every rank's elimination tree (parent[r] > r, -1 at a root)."""
    root = np.arange(len(parent), dtype=np.int32)
    for r in range(len(parent) - 1, -1, -1):
        if parent[r] >= 0:
            root[r] = root[parent[r]]
    return root


def longest_consecutive_run(parent):
    """Nodes of the longest chain x, x + 1, ... with parent[x + i] == x + i + 1."""
    best = cur = 1
    for x in range(len(parent) - 1):
        cur = cur + 1 if parent[x] == x + 1 else 1
        best = max(best, cur)
    return best


def edge_counts(sub_up, sub_dn):
    """Road edges every arc stands for, from the sub-arc arrays ([2M] each): an arc without a route
    (-1, -1) is 0, a road edge (-1, e) is 1, a shortcut is cnt_dn[first] + cnt_up[second] — both
    sub-arcs start at a lower rank, so they have smaller arc ids."""
    su = np.asarray(sub_up).reshape(-1, 2)
    sd = np.asarray(sub_dn).reshape(-1, 2)
    M = len(su)
    cu = np.zeros(M, np.int64)
    cd = np.zeros(M, np.int64)
    for a in range(M):
        for sub, cnt in ((su, cu), (sd, cd)):
            s0, s1 = sub[a]
            if s0 < 0:
                cnt[a] = 0 if s1 < 0 else 1
            else:
                assert s0 < a and s1 < a
                cnt[a] = cd[s0] + cu[s1]
    return cu.astype(np.int32), cd.astype(np.int32)


def dijkstra_pairs(g, cost, src, dst):
    """float64 Dijkstra seconds per pair (inf where unreachable)."""
    from routest_amd.routing.graph import dijkstra_ref
    return dijkstra_ref(g, cost, src, dst)


@functools.lru_cache(maxsize=None)
def islands_pool():
    """The islands query pool: 4,000 pairs — uniform random ones, 16 with s == t, 32 adjacent nodes,
    and (should the draw hold none) unreachable pairs inside one elimination tree — ordered so that
    statuses 0 and 1 alternate irregularly: the four pairs a wave of the cooperative unpack takes
    differ in status.  Returns (src, dst, (sec, met, status, paths) of the CPU reference)."""
    g, _ = islands_graph()
    c, mc = cpu_metric("islands")
    rng = np.random.default_rng(17)
    src = rng.integers(0, g.num_nodes, POOL).astype(np.int32)
    dst = rng.integers(0, g.num_nodes, POOL).astype(np.int32)
    dst[:16] = src[:16]
    has_out = np.flatnonzero(np.diff(g.indptr) > 0)
    src[16:48] = has_out[rng.integers(0, len(has_out), 32)]
    dst[16:48] = g.indices[g.indptr[src[16:48]]]
    A = c.arrays()
    root = etree_roots(A["parent"])[A["rank"]]
    st = np.asarray(c.query(mc, src, dst, False)[2])
    for _ in range(20):                                    # same-tree unreachable pairs, if none yet
        if ((st == 1) & (root[src] == root[dst])).any():
            break
        s2 = rng.integers(0, g.num_nodes, POOL).astype(np.int32)
        t2 = rng.integers(0, g.num_nodes, POOL).astype(np.int32)
        st2 = np.asarray(c.query(mc, s2, t2, False)[2])
        hit = np.flatnonzero((st2 == 1) & (root[s2] == root[t2]))[:8]
        src[POOL - len(hit):] = s2[hit]
        dst[POOL - len(hit):] = t2[hit]
        st = np.asarray(c.query(mc, src, dst, False)[2])
    i0, i1 = list(np.flatnonzero(st == 0)), list(np.flatnonzero(st != 0))
    order = []
    pattern = (0, 1, 0, 0, 1, 1, 0)                        # period 7: a wave's four pairs vary
    k = 0
    while i0 and i1:
        order.append((i1 if pattern[k % 7] else i0).pop(0))
        k += 1
    order += i0 + i1
    src, dst = src[order].copy(), dst[order].copy()
    sec, met, st, paths = c.query(mc, src, dst, True)
    return src, dst, (np.asarray(sec), np.asarray(met), np.asarray(st), [np.asarray(p) for p in paths])


@functools.lru_cache(maxsize=None)
def clique_all_pairs():
    s, t = np.divmod(np.arange(CLIQUE_N * CLIQUE_N, dtype=np.int32), np.int32(CLIQUE_N))
    return s.astype(np.int32), t.astype(np.int32)


def uniform_pairs(g, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, g.num_nodes, n).astype(np.int32), rng.integers(0, g.num_nodes, n).astype(np.int32))


def reference_query(A, MA, s_node, t_node):
    """One pair query in plain Python from the hierarchy (``arrays()``) and a customized metric
    (``metric_arrays()``), with the documented rules spelled out: an arc direction is kept iff its
    perfect weight is finite and equals its basic weight; a chain sweep visits a node's kept arcs in
    arc order and replaces a label only by a strictly smaller f32 sum; the pair meets at the deepest
    common depth of minimum sum; a shortcut unpacks first sub-arc (down) then second (up).
    Returns (seconds, node path), or (None, None) when there is no route."""
    rank, node, parent, depth = A["rank"], A["node"], A["parent"], A["depth"]
    up_ptr, up_head, arc_lo = A["up_ptr"], A["up_head"], A["arc_lo"]
    inf = np.float32(np.inf)

    def sweep(r, w, p):
        D = int(depth[r])
        dist, pred, chain = [inf] * (D + 1), [-1] * (D + 1), [-1] * (D + 1)
        dist[D] = np.float32(0)
        x = int(r)
        while x >= 0:
            chain[depth[x]] = x
            dx = dist[depth[x]]
            if dx < inf:
                for a in range(int(up_ptr[x]), int(up_ptr[x + 1])):
                    if p[a] < inf and p[a] == w[a]:
                        nd = np.float32(dx + p[a])
                        slot = depth[up_head[a]]
                        if nd < dist[slot]:
                            dist[slot], pred[slot] = nd, a
            x = int(parent[x])
        return dist, pred, chain

    s, t = int(rank[s_node]), int(rank[t_node])
    df, pf, cf = sweep(s, MA["w_up"], MA["p_up"])
    db, pb, cb = sweep(t, MA["w_dn"], MA["p_dn"])
    best, bestd = inf, -1
    common = 0                                             # the chains share their top `common` nodes
    while common < min(len(cf), len(cb)) and cf[common] == cb[common]:
        common += 1
    for d in range(common - 1, -1, -1):
        v = np.float32(df[d] + db[d])
        if v < best:
            best, bestd = v, d
    if bestd < 0:
        return None, None
    fw, bw = [], []
    x = cf[bestd]
    while x != s:
        fw.append(pf[depth[x]])
        x = int(arc_lo[fw[-1]])
    x = cf[bestd]
    while x != t:
        bw.append(pb[depth[x]])
        x = int(arc_lo[bw[-1]])
    sub = (MA["sub_up"].reshape(-1, 2), MA["sub_dn"].reshape(-1, 2))
    path = [int(s_node)]

    def unpack(a, down):
        s0, s1 = sub[down][a]
        if s0 < 0:
            path.append(int(node[arc_lo[a] if down else up_head[a]]))
            return
        unpack(int(s0), 1)
        unpack(int(s1), 0)

    for a in reversed(fw):
        unpack(int(a), 0)
    for a in bw:
        unpack(int(a), 1)
    return best, path


def front_plan(parent, min_chain):
    """(fronts, nodes in fronts) the supernodal customization plans for ROUTEST_CCH_DENSE=min_chain
    (csrc/cch_customize.hip build_supernodes): a supernode is a maximal run of ranks in which every
    node is the only child of the next; those of at least min_chain nodes and all their ancestor
    supernodes are dense fronts."""
    N = len(parent)
    if min_chain <= 0 or N < 2:
        return 0, 0
    nch = np.bincount(parent[parent >= 0], minlength=N)
    sid, first, size = np.zeros(N, np.int64), [], []
    for i in range(N):
        if not (i > 0 and parent[i - 1] == i and nch[i] == 1):
            first.append(i)
            size.append(0)
        sid[i] = len(first) - 1
        size[-1] += 1
    spar = [sid[parent[c + m - 1]] if parent[c + m - 1] >= 0 else -1 for c, m in zip(first, size)]
    dense = [False] * len(first)
    for s in range(len(first)):
        if size[s] >= min_chain:
            q = s
            while q >= 0 and not dense[q]:
                dense[q] = True
                q = spar[q]
    return sum(dense), sum(m for m, d in zip(size, dense) if d)
