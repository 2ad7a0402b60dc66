"""Preconditions of the adversarial CCH fixtures (tests/_cch_graphs.py), on the CPU reference alone.

tests/test_cch_edges_gpu.py compares the GPU kernels with ``_rt.CCH`` on these graphs; that only
bites while the graphs keep the properties the kernels' branches need — infinite arc weights,
unreachable pairs of both kinds, every small path length, a 321-rank chain, nodes with more than 256
kept arcs, abundant exact ties.  Each is asserted here so a fixture that silently loses one fails in
the CPU suite.  The reference itself is pinned too: a plain-Python query with the documented tie
rules must reproduce its paths on the tie metrics, and the status-4 contract (seconds and metres are
the route's whenever status != 1) is checked at the exact ``max_path`` boundary.
"""
import numpy as np
import pytest

import _cch_graphs as G

rt = pytest.importorskip("routest_amd._rt")


def test_islands_have_infinite_weights_and_both_kinds_of_unreachable_pairs():
    g, cost = G.islands_graph()
    c, mc = G.cpu_metric("islands")
    ma = c.metric_arrays(mc)
    assert np.isinf(ma["w_up"]).sum() >= 1000 and np.isinf(ma["w_dn"]).sum() >= 1000
    assert np.isinf(ma["len_up"]).sum() >= 1000 and (ma["sub_up"].reshape(-1, 2)[np.isinf(ma["w_up"])] == -1).all()
    src, dst, (sec, met, st, paths) = G.islands_pool()
    assert len(src) == G.POOL and set(np.unique(st)) == {0, 1}
    assert (st == 0).sum() > G.POOL // 4 and (st == 1).sum() > G.POOL // 4, np.bincount(st)
    A = c.arrays()
    root = G.etree_roots(A["parent"])[A["rank"]]
    same = root[src] == root[dst]
    assert ((st == 1) & same).any() and ((st == 1) & ~same).any()
    assert (st[~same] == 1).all()
    # unreachable exactly where Dijkstra says so, and -1 / empty path there
    ref = G.dijkstra_pairs(g, cost, src, dst)
    assert np.array_equal(np.isfinite(ref), st == 0)
    assert (sec[st == 1] == -1).all() and (met[st == 1] == -1).all()
    assert all(len(paths[i]) == 0 for i in np.flatnonzero(st == 1))
    np.testing.assert_allclose(sec[st == 0], ref[st == 0], rtol=1e-5, atol=1e-4)
    # every path edge count 0..48, s == t and adjacent pairs among them
    edges = np.array([len(paths[i]) - 1 for i in np.flatnonzero(st == 0)])
    assert set(range(G.EDGE_COUNTS)) <= set(edges.tolist()), sorted(set(range(G.EDGE_COUNTS)) - set(edges.tolist()))
    assert ((src == dst) & (st == 0)).sum() >= 16
    # the order mixes the statuses inside the first waves of four pairs
    mixed = [len(set(st[w:w + 4].tolist())) == 2 for w in range(0, 64, 4)]
    assert sum(mixed) >= 12, mixed


def test_clique_is_one_chain_with_wide_nodes():
    g, narrow, wide = G.clique_graph()
    c = G.cpu_cch("clique")
    s, A = c.stats(), c.arrays()
    M = s["arcs"]
    assert s["nodes"] == G.CLIQUE_N and M == G.CLIQUE_N * (G.CLIQUE_N - 1) // 2
    assert s["max_depth"] == G.CLIQUE_N - 1 and (s["max_depth"] + 1) % 64 != 0
    assert G.longest_consecutive_run(A["parent"]) >= 129
    assert np.diff(A["up_ptr"]).max() > 256
    _, mn = G.cpu_metric("clique_narrow")
    ma = c.metric_arrays(mn)
    assert ma["kept_f"] == M and ma["kept_b"] == M            # so rank 0 keeps 320 arcs each way
    assert (ma["sub_up"].reshape(-1, 2)[:, 0] == -1).all()     # every arc is its road edge
    _, mw = G.cpu_metric("clique_wide")
    mb = c.metric_arrays(mw)
    assert M // 5 < mb["kept_f"] < M // 2 and M // 5 < mb["kept_b"] < M // 2, (mb["kept_f"], mb["kept_b"])
    src, dst = G.uniform_pairs(g, 2000, seed=4)
    sec, met, st, paths = c.query(mw, src, dst, True)
    assert (st == 0).all()
    edges = np.array([len(p) - 1 for p in paths])
    assert edges.max() >= 3 and (edges[src != dst] >= 1).all()
    np.testing.assert_allclose(sec, G.dijkstra_pairs(g, wide, src, dst), rtol=1e-5, atol=1e-4)
    s2, t2 = G.clique_all_pairs()
    sec, met, st, paths = c.query(mn, s2, t2, True)
    off = s2 != t2
    assert (st == 0).all() and all(len(p) == 2 for p, o in zip(paths, off) if o)
    assert np.array_equal(sec[off], narrow) and np.array_equal(met[off], g.length_m)


@pytest.mark.parametrize("name", ["ties_ones", "ties_ints"])
def test_tie_metrics_are_exact_and_full_of_ties(name):
    g, cost = G.fixture_metrics()[name]
    c, mc = G.cpu_metric(name)
    s = c.stats()
    assert s["max_depth"] >= 129 and G.longest_consecutive_run(c.arrays()["parent"]) >= 129
    src, dst = G.uniform_pairs(g, 1000, seed=6)
    sec, met, st, paths = c.query(mc, src, dst, True)
    assert (st == 0).all()
    # integer costs: every f32 sum is exact, so the seconds ARE Dijkstra's
    assert np.array_equal(np.asarray(sec).astype(np.float64), G.dijkstra_pairs(g, cost, src, dst))
    # ties are abundant: breaking them moves at least half of the paths
    m2 = c.customize(G.perturbed(cost), g.length_m)
    p2 = c.query(m2, src, dst, True)[3]
    changed = sum(not np.array_equal(a, b) for a, b in zip(paths, p2))
    assert changed >= 500, changed


@pytest.mark.parametrize("name", ["ties_ones", "ties_ints", "islands"])
def test_reference_follows_the_documented_tie_rules(name):
    """csrc/runtime/cch.h sweep (strict <, kept arcs in arc order), query (deepest meeting depth) and
    unpack_arc (first sub-arc down, then second up) against tests/_cch_graphs.py reference_query: a
    `<=` in either loop keeps every second but moves the paths on the tie metrics."""
    g, cost = G.fixture_metrics()[name]
    c, mc = G.cpu_metric(name)
    if name == "islands":
        src, dst = G.islands_pool()[:2]
        src, dst = src[:48], dst[:48]
    else:
        src, dst = G.uniform_pairs(g, 48, seed=6)
    sec, met, st, paths = c.query(mc, src, dst, True)
    A, MA = c.arrays(), c.metric_arrays(mc)
    for i in range(len(src)):
        rs, rp = G.reference_query(A, MA, int(src[i]), int(dst[i]))
        if rs is None:
            assert st[i] == 1
            continue
        assert st[i] == 0 and sec[i] == rs and np.array_equal(paths[i], rp), i


def test_status_4_keeps_seconds_and_metres_at_the_exact_boundary():
    """_rt.CCH.query (csrc/runtime/cch_bind.cpp): a path of exactly max_path nodes is status 0, one
    more node is status 4 with an empty path — and a status-4 row still carries the route's seconds
    and metres (they do not depend on want_path); only status 1 reports -1."""
    c, mc = G.cpu_metric("islands")
    src, dst, (sec, met, st, paths) = G.islands_pool()
    nodes = np.array([len(p) for p in paths])
    med = int(np.median(nodes[st == 0]))
    pick = int(np.flatnonzero((st == 0) & (nodes > med))[0])
    for mp in (med, nodes[pick] - 1, nodes[pick], nodes[pick] + 1, 1):
        s2, m2, st2, p2 = c.query(mc, src, dst, True, int(mp))
        want = np.where(st == 1, 1, np.where(nodes <= mp, 0, 4))
        assert np.array_equal(st2, want), mp
        assert np.array_equal(s2, sec) and np.array_equal(m2, met), mp
        assert all(np.array_equal(p2[i], paths[i]) if want[i] == 0 else len(p2[i]) == 0 for i in range(len(src)))
        assert (want == 4).any()
        s3, m3, st3, _ = c.query(mc, src, dst, False, int(mp))
        assert np.array_equal(s3, sec) and np.array_equal(m3, met) and np.array_equal(st3, st)
    assert st2[pick] == 4 and (st2[src == dst] == 0).all() and ((st2 == 0) == (src == dst)).all()   # max_path 1
