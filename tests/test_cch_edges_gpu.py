"""GPU CCH customization and pair queries (csrc/cch_customize.hip, csrc/cch_query.hip) against the CPU
reference (``_rt.CCH``) on the small adversarial graphs of tests/_cch_graphs.py — whose properties
tests/test_cch_edges_cpu.py asserts without a GPU.  Every comparison is equality, bit for bit.

* islands: infinite arc weights through every customization path; status 1 from two elimination
  trees and from one tree without a finite meeting depth; status 4 at the exact ``max_path``
  boundary; every path edge count 0..48 through the cooperative unpack's 16-lane split and through
  the serial unpack; waves of four pairs that differ in status; Q that is no multiple of 4.
* clique (321 nodes, one chain of consecutive ranks, 320 kept arcs at the lowest rank): the sweep's
  64-node runs that continue into the next header, the clipped last run, the top rank's header past
  N, and the record loop past the 256 prefetched records.
* ties (unit and {1, 2, 3} costs): the tie rules of the customization (packed middle node), the
  sweep (strict <) and the meet (deepest depth), with seconds that equal float64 Dijkstra exactly.
* matrix / matrix_keep / legs_from_matrix with request rows of 0, 1, NM - 1 and NM points whose
  padding slots hold valid node ids.

Not covered, on purpose — limits the reference does not have and small graphs cannot reach: the
meet kernel's MAX_ARCS = 1024 shortcut arcs and its ``fw[4096]`` list, the serial unpack's DFS stack
(UNPACK_STACK = 128), the cooperative unpack's stack (UNPACK_SD = 64) with its ``out_len = -1``
hand-off to the serial kernel, and the multi-context ``route_multi`` / ``matrix_multi`` views (only
the C++ route service reaches them).  Nothing here tries to overflow anything on the device.
"""
import numpy as np
import pytest
import torch

import _cch_graphs as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRICS = ["islands", "clique_narrow", "clique_wide", "ties_ones", "ties_ints"]
KEY = {name: (1 << 40) + i for i, name in enumerate(METRICS)}
GRAPHS = {"islands": ["islands"], "clique": ["clique_narrow", "clique_wide"], "ties": ["ties_ones", "ties_ints"]}


def _graph_of(name):
    return name.split("_")[0]


@pytest.fixture(scope="module")
def model():
    from routest_amd.serve.eta_service import default_model
    return default_model(hidden=64, steps=50)


@pytest.fixture(scope="module")
def routers(model):
    """One default-settings router per fixture graph, every fixture metric customized on it."""
    from routest_amd.routing.cch import RoadRouter
    out = {}
    for graph, names in GRAPHS.items():
        r = RoadRouter(G.fixture_metrics()[names[0]][0], model, device=DEV)
        for name in names:
            r.metric_from_costs(KEY[name], G.fixture_metrics()[name][1])
        out[graph] = r
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _pad_paths(paths, width):
    """list of node arrays -> [Q, width] padded with -1."""
    out = np.full((len(paths), width), -1, np.int32)
    ln = np.array([len(p) for p in paths], np.int64)
    if len(paths) and ln.sum():
        out[np.arange(width)[None, :] < ln[:, None]] = np.concatenate([np.asarray(p, np.int32) for p in paths])
    return out, ln.astype(np.int32)


def _gpu_route(router, name, src, dst, max_path=4096, serial=False, want_path=True):
    """(sec, met, status, len, paths padded with -1 past len) of CchGpu.route, as numpy."""
    gpu = router.gpu
    gpu.set_unpack_serial(serial)
    try:
        out = gpu.route(KEY[name], _dev(src), _dev(dst), int(max_path), want_path)
    finally:
        gpu.set_unpack_serial(False)
    return _as_numpy(out, want_path)


def _as_numpy(out, want_path=True):
    sec, met, st, ln, path = [t.cpu().numpy() for t in out]
    if want_path:
        path = np.where(np.arange(path.shape[1])[None, :] < ln[:, None], path, -1)
    return sec, met, st, ln, path


def _cpu_route(name, src, dst, max_path=None):
    """The reference's (sec, met, status, len, padded paths); max_path None: the longest path of the
    batch, so that some rows are exactly full and none is status 4."""
    c, mc = G.cpu_metric(name)
    src, dst = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32)
    sec, met, st, paths = c.query(mc, src, dst, True, 1 << 20 if max_path is None else int(max_path))
    width = max([len(p) for p in paths] + [1]) if max_path is None else int(max_path)
    path, ln = _pad_paths(paths, width)
    return np.asarray(sec), np.asarray(met), np.asarray(st), ln, path


def _assert_same(got, want, what=""):
    assert len(got) == len(want)
    for field, a, b in zip(("sec", "metres", "status", "len", "path"), got, want):
        if a.dtype.kind == "f":                    # bit for bit (-1 and +inf included)
            a, b = a.view(np.int32), b.view(np.int32)
        assert a.shape == b.shape, (what, field, a.shape, b.shape)
        assert np.array_equal(a, b), (what, field, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:8])


# ---- 1. customization: every path, every fixture metric ----

@pytest.mark.parametrize("graph", list(GRAPHS))
def test_customization_paths_agree_on_every_metric(routers, model, monkeypatch, graph):
    """csrc/cch_customize.hip: the accelerated path (basic_task_kernel, perfect_pull_*_kernel), the
    fallback (ROUTEST_CCH_TRI_GB=0: basic_level_kernel / perfect_level_kernel) and the supernodal
    fronts (ROUTEST_CCH_DENSE=0 / 1 / 32: sup_*_kernel) give the same metric arrays bit for bit —
    with infinite weights (islands: the 64-bit atomicMin on weight | middle, its skip-if-not-better
    pre-check, the pull records and the pruning) and with ties decided by the packed middle node.
    Each variant must really have taken the path it names (stats())."""
    from routest_amd.routing.cch import RoadRouter
    base = routers[graph]
    g = base.g
    parent = G.cpu_cch(graph).arrays()["parent"]
    N = g.num_nodes

    def check_stats(st, tri, dense):
        fronts, nodes = G.front_plan(parent, dense) if tri else (0, 0)
        assert bool(st["triangle_table"]) == tri, st
        assert (st["triangles"] > 0) == tri and (st["basic_tasks"] > 0) == (tri and nodes < N), st
        assert bool(st["supernodal"]) == (fronts > 0), st
        assert (st["sup_fronts"], st["sup_nodes"]) == (fronts, nodes), st
        if fronts:
            assert st["sup_levels"] >= 1 and st["sup_blocks"] >= 1, st

    check_stats(base.stats(), True, 8)
    ref = {name: {k: v.cpu() for k, v in base.gpu.metric_dump(KEY[name]).items()} for name in GRAPHS[graph]}
    for env, val, tri, dense in (("ROUTEST_CCH_TRI_GB", "0", False, 8), ("ROUTEST_CCH_DENSE", "0", True, 0),
                                 ("ROUTEST_CCH_DENSE", "1", True, 1), ("ROUTEST_CCH_DENSE", "32", True, 32)):
        with monkeypatch.context() as mp:
            mp.setenv(env, val)
            r2 = RoadRouter(g, model, device=DEV)
        check_stats(r2.stats(), tri, dense)
        for name in GRAPHS[graph]:
            for rep in range(2):                   # a second customization reuses the temporaries
                r2.metric_from_costs(KEY[name] + 64 * rep, G.fixture_metrics()[name][1])
                d = r2.gpu.metric_dump(KEY[name] + 64 * rep)
                assert d.keys() == ref[name].keys()
                for k, v in ref[name].items():
                    assert torch.equal(d[k].cpu(), v), (env, val, name, k, rep)
        del r2


# ---- 2. GPU metric == CPU metric ----

@pytest.mark.parametrize("name", METRICS)
def test_gpu_metric_equals_cpu_metric(routers, name):
    """csrc/cch_customize.hip basic_finalize_arc / sup_panel_body (sub-arcs, metres, edge counts) and
    prune_scatter_wave_kernel (kept-arc records) against csrc/runtime/cch.h customize: sub_up, sub_dn,
    len_up, len_dn equal the reference's bits on EVERY arc (no restriction to kept arcs was needed:
    both sides break weight ties by the smallest middle node, a road edge last); cnt_up / cnt_dn equal
    the edge counts recomputed from the sub-arcs; f_ptr / b_ptr / f_rec / b_rec equal the kept arcs
    (perfect weight finite and equal to the basic one) in arc order."""
    c, mc = G.cpu_metric(name)
    A, MA = c.arrays(), c.metric_arrays(mc)
    d = {k: v.cpu().numpy() for k, v in routers[_graph_of(name)].gpu.metric_dump(KEY[name]).items()}
    for k in ("sub_up", "sub_dn"):
        assert np.array_equal(d[k], MA[k]), k
    for k in ("len_up", "len_dn"):
        assert np.array_equal(d[k].view(np.int32), MA[k].view(np.int32)), k
    cu, cd = G.edge_counts(MA["sub_up"], MA["sub_dn"])
    assert np.array_equal(d["cnt_up"], cu) and np.array_equal(d["cnt_dn"], cd)
    hd = A["depth"][A["up_head"]]
    for ptr, rec, w, p in (("f_ptr", "f_rec", "w_up", "p_up"), ("b_ptr", "b_rec", "w_dn", "p_dn")):
        kept = np.isfinite(MA[p]) & (MA[p] == MA[w])
        want_ptr = np.concatenate([[0], np.cumsum(np.bincount(A["arc_lo"][kept], minlength=len(A["rank"])))])
        assert np.array_equal(d[ptr], want_ptr), ptr
        arcs = np.flatnonzero(kept)
        want = np.stack([MA[p][arcs].view(np.int32), hd[arcs], arcs.astype(np.int32), np.zeros(len(arcs), np.int32)], 1)
        assert np.array_equal(d[rec].reshape(-1, 4), want), rec
    if name == "islands":
        assert np.isinf(d["len_up"]).sum() >= 1000 and np.isinf(d["len_dn"]).sum() >= 1000
    if name == "clique_narrow":                    # the sweep's loop past 256 prefetched records runs
        assert np.diff(d["f_ptr"]).max() > 256 and np.diff(d["b_ptr"]).max() > 256


# ---- 3. route ----

def _queries(name):
    g = G.fixture_metrics()[name][0]
    if name == "islands":
        return G.islands_pool()[:2]
    if name == "clique_narrow":
        return G.clique_all_pairs()
    if name == "clique_wide":
        return G.uniform_pairs(g, 2000, seed=4)
    return G.uniform_pairs(g, 1000, seed=6)


@pytest.mark.parametrize("name", METRICS)
def test_route_equals_cpu_reference(routers, name):
    """csrc/cch_query.hip sweep_kernel (runs of 64 consecutive ranks continuing into the next
    header, `L > d + 1` clipping, `cand < N` at the top rank, sweep_fetch's `ii = i < 63 ? i : 63`,
    the `k = b + 64 * SWEEP_RECS + lane` loop of nodes with more than 256 kept arcs, the strict `<`
    of sweep_relax), meet_kernel (different roots; one tree without a finite meeting depth; the
    deepest-depth tie in the lane loop and the shuffle reduction) and the unpack kernels: seconds,
    metres, status, length and node path equal ``_rt.CCH.query``; on the tie metrics the seconds
    also equal float64 Dijkstra exactly.  max_path is the longest reference path: exactly full rows."""
    router = routers[_graph_of(name)]
    g, cost = G.fixture_metrics()[name]
    src, dst = _queries(name)
    c, mc = G.cpu_metric(name)
    want = _cpu_route(name, src, dst)
    longest = want[4].shape[1]
    assert (want[3] == longest).any() and (want[2] != 4).all()
    got = _gpu_route(router, name, src, dst, longest)
    _assert_same(got, want, name)
    _assert_same(_gpu_route(router, name, src, dst, longest), want, name + " again")
    nopath = _gpu_route(router, name, src, dst, longest, want_path=False)
    _assert_same(nopath[:3], want[:3], name + " without paths")
    if name.startswith("ties"):
        assert (got[2] == 0).all()
        assert np.array_equal(got[0].astype(np.float64), G.dijkstra_pairs(g, cost, src, dst))
    if name == "clique_narrow":
        assert (got[3][src != dst] == 2).all()
    if name == "islands":
        same_root = G.etree_roots(c.arrays()["parent"])[c.arrays()["rank"]]
        same_root = same_root[src] == same_root[dst]
        assert ((got[2] == 1) & same_root).any() and ((got[2] == 1) & ~same_root).any()
        assert (got[0][got[2] == 1] == -1).all() and (got[1][got[2] == 1] == -1).all()


@pytest.mark.parametrize("serial", [False, True])
def test_route_batch_sizes_and_scratch_growth(routers, serial):
    """CchScratch::ensure and the unpack kernels' tails: Q = 0, 1, 3, 4, 5, 63, 64, 65 pairs of the
    islands pool (waves of four pairs that mix statuses 0 and 1; a last wave of 1, 3 or 4 pairs), in
    the order small, large, small on a fresh router so the scratch grows in between and is reused
    after."""
    from routest_amd.routing.cch import RoadRouter
    src, dst, _ = G.islands_pool()
    g, cost = G.fixture_metrics()["islands"]
    router = RoadRouter(g, routers["islands"].eta_model, device=DEV)
    router.metric_from_costs(KEY["islands"], cost)
    want = _cpu_route("islands", src, dst, 128)
    st = want[2]
    assert all(len(set(st[w:w + 4].tolist())) == 2 for w in (0, 4, 60))
    for Q in (0, 1, 3, 4, 5, 63, 64, 65, len(src), 65, 5, 1, 0):
        got = _gpu_route(router, "islands", src[:Q], dst[:Q], 128, serial)
        _assert_same(got, [w[:Q] for w in want], Q)
        assert got[4].shape == (Q, 128)


# ---- 4. cooperative unpack == serial unpack == CPU ----

@pytest.mark.parametrize("name", ["islands", "ties_ones", "ties_ints"])
def test_serial_unpack_equals_cooperative_unpack(routers, name):
    """csrc/cch_query.hip unpack_coop_kernel (E road edges split as per = ceil(E / 16) over 16 lanes:
    E = 0, 1, 15, 16, 17, 31, 32, 33, ... 48 all occur; the binary search over the arcs' offsets, the
    descent by edge counts) against unpack_kernel (one lane's DFS), switched per call with
    CchGpu.set_unpack_serial: identical lengths and paths, both equal to the CPU reference."""
    router = routers[_graph_of(name)]
    src, dst = _queries(name)
    want = _cpu_route(name, src, dst, 256)
    assert (want[2] != 4).all()
    if name == "islands":
        edges = want[3][want[2] == 0] - 1
        assert set(range(G.EDGE_COUNTS)) <= set(edges.tolist())
    assert not router.gpu.unpack_serial()
    coop = _gpu_route(router, name, src, dst, 256, serial=False)
    ser = _gpu_route(router, name, src, dst, 256, serial=True)
    assert not router.gpu.unpack_serial()
    _assert_same(coop, want, name + " cooperative")
    _assert_same(ser, want, name + " serial")
    _assert_same(_gpu_route(router, name, src, dst, 256, serial=True), ser, name + " serial again")


# ---- 5 and 6. the max_path boundary; status-4 rows ----

@pytest.mark.parametrize("serial", [False, True])
def test_max_path_boundary_and_status_4_rows(routers, serial):
    """csrc/cch_query.hip unpack_coop_kernel `E + 1 > max_path` and unpack_kernel `n >= max_path`: a
    path of exactly max_path nodes is status 0 with its full path, one more node is status 4 with
    len 0 — for max_path = the batch's median node count, a chosen query's count and that +- 1, and
    max_path = 1 (only s == t survives).  A status-4 row keeps the route's seconds and metres (the
    meet kernel wrote them; the route exists, only its listing was refused), exactly like
    ``_rt.CCH.query``: all three arrays are compared on every row, status-4 rows included, and they
    do not depend on want_path."""
    router = routers["islands"]
    src, dst, (sec, met, st, paths) = G.islands_pool()
    nodes = np.array([len(p) for p in paths])
    med = int(np.median(nodes[st == 0]))
    pick = int(np.flatnonzero((st == 0) & (nodes > med))[0])
    n = int(nodes[pick])
    for mp in (med, n - 1, n, n + 1, 1, med):
        want = _cpu_route("islands", src, dst, mp)
        assert np.array_equal(want[2], np.where(st == 1, 1, np.where(nodes <= mp, 0, 4)))
        assert (want[2] == 4).sum() > 100 and ((want[2] == 0) & (want[3] == mp)).any()
        assert np.array_equal(want[0], sec) and np.array_equal(want[1], met)
        got = _gpu_route(router, "islands", src, dst, mp, serial)
        _assert_same(got, want, mp)
        assert got[2][pick] == (4 if mp < n else 0) and got[3][pick] == (0 if mp < n else n)
        assert (got[3][got[2] != 0] == 0).all() and (got[0][got[2] == 4] > 0).all()
        nopath = _gpu_route(router, "islands", src, dst, mp, serial, want_path=False)
        assert np.array_equal(nopath[0], got[0]) and np.array_equal(nopath[1], got[1])
        assert np.array_equal(nopath[2], st)
        if mp == 1:
            assert np.array_equal(got[2] == 0, src == dst)


# ---- 7. matrix, matrix_keep, legs_from_matrix ----

def _matrix_case(router, name, R, NM, rng, variant):
    g = G.fixture_metrics()[name][0]
    c, mc = G.cpu_metric(name)
    pts = rng.integers(0, g.num_nodes, (R, NM)).astype(np.int32)      # padding slots hold valid ids too
    choices = [0, 1, NM - 1, NM]
    npts = np.array([choices[(r + variant) % 4] for r in range(R)], np.int32)
    ii, jj = np.meshgrid(np.arange(NM), np.arange(NM), indexing="ij")
    s_all = pts[:, ii.ravel()].ravel()
    t_all = pts[:, jj.ravel()].ravel()
    sec, met, st, _ = c.query(mc, s_all, t_all, False)
    inside = (ii[None] < npts[:, None, None]) & (jj[None] < npts[:, None, None]) & (ii != jj)[None]
    shape = (R, NM, NM)
    inf = np.float32(np.inf)
    want_sec = np.where(inside, np.where(st.reshape(shape) == 0, sec.reshape(shape), inf), np.float32(0))
    want_met = np.where(inside, np.where(st.reshape(shape) == 0, met.reshape(shape), inf), np.float32(0))
    dp, dn = _dev(pts), _dev(npts)
    for call in range(2):
        gs, gm = [t.cpu().numpy() for t in router.gpu.matrix(KEY[name], dp, dn)]
        assert np.array_equal(gs.view(np.int32), want_sec.astype(np.float32).view(np.int32)), (name, R, NM, call)
        assert np.array_equal(gm.view(np.int32), want_met.astype(np.float32).view(np.int32)), (name, R, NM, call)
    unreachable = inside & (st.reshape(shape) != 0)
    assert np.isinf(gs[unreachable]).all() and np.isinf(gm[unreachable]).all() and (gs[~inside] == 0).all()
    # legs between points inside npts, from the kept chains, then the same pairs swept afresh
    ks, km, tag = router.gpu.matrix_keep(KEY[name], dp, dn)
    assert torch.equal(ks.cpu(), torch.from_numpy(gs)) and torch.equal(km.cpu(), torch.from_numpy(gm))
    rows = np.flatnonzero(npts > 0)
    Q = 0 if len(rows) == 0 else 37
    r = rows[rng.integers(0, max(1, len(rows)), Q)].astype(np.int32) if Q else np.zeros(0, np.int32)
    i = (rng.integers(0, 1 << 20, Q) % np.maximum(npts[r], 1)).astype(np.int32)
    j = (rng.integers(0, 1 << 20, Q) % np.maximum(npts[r], 1)).astype(np.int32)
    legs = [_as_numpy(router.gpu.legs_from_matrix(KEY[name], tag, dp, _dev(r), _dev(i), _dev(j), 128, True))
            for _ in range(2)]
    _assert_same(legs[1], legs[0], (name, R, NM, "legs again"))
    fresh = _gpu_route(router, name, pts[r, i], pts[r, j], 128)
    _assert_same(legs[0], fresh, (name, R, NM, "legs vs route"))
    _assert_same(legs[0], _cpu_route(name, pts[r, i], pts[r, j], 128), (name, R, NM, "legs vs cpu"))
    if Q:
        with pytest.raises(RuntimeError):          # route() above replaced the chains
            router.gpu.legs_from_matrix(KEY[name], tag, dp, _dev(r), _dev(i), _dev(j), 128, True)
    return unreachable.sum(), (legs[0][2] == 1).sum()


@pytest.mark.parametrize("name", ["islands", "clique_wide"])
def test_matrix_padding_and_legs_from_kept_chains(routers, name):
    """csrc/cch_query.hip matrix_jobs_kernel (`i >= npts[r]` gives jobs -1), sweep_kernel and
    meet_kernel's padding branches, matrix_out_kernel's `out` / `diag` handling and the legs that
    reuse the matrix chains (leg_pairs_kernel, meet + unpack only): R = 1, 2, 5 requests of NM = 1,
    2, 7, 12 slots with rows of 0, 1, NM - 1 and NM points in one call.  Inside npts an entry equals
    the reference's bits, unreachable ones (other island, one-way) are +inf in both arrays, the
    diagonal and everything outside npts is 0; legs from the kept chains equal fresh route() calls
    and the reference, unreachable legs (status 1) included; a stale tag is refused."""
    router = routers[_graph_of(name)]
    rng = np.random.default_rng(8)
    unreachable = status1 = 0
    cases = [(R, NM) for NM in (1, 2, 7, 12) for R in (1, 2, 5)]
    for variant, (R, NM) in enumerate(cases + [(1, 1), (5, 12), (2, 2)]):     # small, large, small
        u, s1 = _matrix_case(router, name, R, NM, rng, variant)
        unreachable += u
        status1 += s1
    if name == "islands":
        assert unreachable > 50 and status1 > 10
