"""GPU customizable contraction hierarchy (csrc/cch.hip) vs the CPU reference (csrc/runtime/cch.h)
and scipy Dijkstra, on the 100k-node synthetic graph with MLP edge costs.

* customization + queries are BIT-identical to the CPU reference (same tie rules, f32 adds);
* every leg equals Dijkstra; paths are real edge sequences;
* matrices equal the legs; contexts customize on the GPU and change the answers.
"""
import numpy as np
import pytest
import torch

from routest_amd.data.graph import synth_road_graph, synth_route_queries
from routest_amd.routing.graph import dijkstra_ref, edge_costs
from routest_amd.serve.eta_service import default_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from routest_amd.routing.cch import RoadRouter
    g = synth_road_graph(100_000, seed=5)
    m = default_model(hidden=64, steps=50)
    router = RoadRouter(g, m, device="cuda:0")
    cost = edge_costs(g, m, device="cuda:0")
    key = router.metric_from_costs(1 << 40, cost)
    from routest_amd import _rt
    cpu = _rt.CCH(g.indptr, g.indices, g.lat, g.lon, 0)
    mc = cpu.customize(cost, g.length_m)
    return g, m, router, cost, key, cpu, mc


def test_legs_exact_and_bit_identical_to_cpu(setup):
    g, m, router, cost, key, cpu, mc = setup
    src, dst = synth_route_queries(g, 3000, seed=1)
    src[:4] = dst[:4]
    sec, met, st, paths = router.route(src, dst, key)
    assert (st == 0).all(), np.unique(st, return_counts=True)
    ref = dijkstra_ref(g, cost, src, dst)
    np.testing.assert_allclose(sec, ref, rtol=1e-5, atol=1e-4)
    s2, m2, st2, p2 = cpu.query(mc, src, dst, True)
    assert np.array_equal(sec, s2) and np.array_equal(met, m2) and np.array_equal(st, st2)
    assert all(np.array_equal(a, b) for a, b in zip(paths, p2))
    for i in range(0, 3000, 61):
        p = paths[i]
        assert p[0] == src[i] and p[-1] == dst[i]
        tot = 0.0
        for u, v in zip(p[:-1], p[1:]):
            nb = g.indices[g.indptr[u]:g.indptr[u + 1]]
            k = np.where(nb == v)[0]
            assert len(k) == 1
            tot += cost[g.indptr[u] + k[0]]
        assert abs(tot - sec[i]) <= 1e-4 * max(1.0, sec[i])
    # repeatable
    sec_b = router.route(src, dst, key, want_path=False)[0]
    assert np.array_equal(sec, sec_b)


def test_matrices_equal_legs(setup):
    g, m, router, cost, key, cpu, mc = setup
    rng = np.random.default_rng(3)
    lists = [rng.integers(0, g.num_nodes, rng.integers(2, 12)).tolist() for _ in range(40)]
    mats = router.matrices(lists, key)
    for nodes, (sec, met) in zip(lists[:10], mats[:10]):
        n = len(nodes)
        ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        nd = np.asarray(nodes, np.int32)
        s2, m2, st2, _ = cpu.query(mc, nd[ii.ravel()], nd[jj.ravel()], False)
        s2 = s2.reshape(n, n)
        m2 = m2.reshape(n, n)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(sec[off], s2[off]) and np.array_equal(met[off], m2[off])
        assert (np.diag(sec) == 0).all()


def test_context_customization_on_gpu(setup):
    from routest_amd.routing.cch import RouteContext
    g, m, router, cost, key, cpu, mc = setup
    sunny = RouteContext(weather=2, congestion=0, weekhour=3)
    storm = RouteContext(weather=1, congestion=3, weekhour=4 * 24 + 18)
    src, dst = synth_route_queries(g, 500, seed=9)
    res = {}
    for ctx in (sunny, storm):
        sec, met, st, _ = router.route(src, dst, ctx, want_path=False)
        info = router.last_metric
        c = router.costs(ctx)
        assert (c > 0).all()
        np.testing.assert_allclose(sec, dijkstra_ref(g, c, src, dst), rtol=1e-5, atol=1e-4)
        res[ctx.key] = (sec, c)
    assert not np.allclose(res[sunny.key][0], res[storm.key][0])
    # cached: a second use does not customize again
    router.route(src[:10], dst[:10], sunny, want_path=False)
    assert router.last_metric["fresh"] is False
    # the GPU context costs match the CPU edge-cost model within bf16 tolerance
    from routest_amd.routing.cch import context_costs_cpu
    np.testing.assert_allclose(res[storm.key][1], context_costs_cpu(g, m, storm), rtol=2e-2, atol=0.05)


def test_legs_from_matrix_chains_equal_fresh_legs(setup):
    """BulkRouteStep's legs reuse the matrix stage's chains (meet + unpack only): identical seconds,
    metres, status and paths to sweeping them again; a stale tag is refused."""
    g, m, router, cost, key, cpu, mc = setup
    rng = np.random.default_rng(3)
    R, NM = 300, 7
    pts = torch.from_numpy(rng.integers(0, g.num_nodes, (R, NM)).astype(np.int32)).cuda()
    npts = torch.full((R,), NM, dtype=torch.int32, device="cuda")
    _, _, tag = router.gpu.matrix_keep(key, pts, npts)
    Q = 2000
    r = torch.from_numpy(rng.integers(0, R, Q).astype(np.int32)).cuda()
    i = torch.from_numpy(rng.integers(0, NM, Q).astype(np.int32)).cuda()
    j = torch.from_numpy(rng.integers(0, NM, Q).astype(np.int32)).cuda()
    a = router.gpu.legs_from_matrix(key, tag, pts, r, i, j, 4096, True)
    src = pts[r.long(), i.long()].contiguous()
    dst = pts[r.long(), j.long()].contiguous()
    b = router.gpu.route(key, src, dst, 4096, True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    ln = a[3].cpu().numpy()
    pa, pb = a[4].cpu().numpy(), b[4].cpu().numpy()
    assert all(np.array_equal(pa[q, :ln[q]], pb[q, :ln[q]]) for q in range(Q))
    with pytest.raises(RuntimeError):          # route() above replaced the chains
        router.gpu.legs_from_matrix(key, tag, pts, r, i, j, 4096, True)


def test_bulk_route_step_reuse_matches_fresh_sweeps(setup, monkeypatch):
    from routest_amd.routing.bulk import BulkRouteStep
    g, m, router, cost, key, cpu, mc = setup
    step = BulkRouteStep(g, cost, torch.device("cuda:0"), 500, router=router, key=key)
    n1, c1, st1, k1 = step.step()
    monkeypatch.setattr(BulkRouteStep, "reuse_chains", False)
    n2, c2, st2, k2 = step.step()
    assert n1 == n2 and torch.equal(c1, c2) and torch.equal(st1, st2) and torch.equal(k1, k2)
    assert int((st1 == 0).sum()) == n1


def test_paced_background_build_bit_identical_to_cpu(setup):
    """A context built by the background builders with pacing (wide levels launched in pieces of
    16 workgroups, csrc/cch_customize.hip customize) gives the CPU reference's answers bit for bit."""
    import time
    from routest_amd.routing.cch import RouteContext
    g, m, router, cost, key, cpu, mc = setup
    before = router.stats().get("async_paced", 0)
    router.gpu.set_builder_pacing(16, always=True)
    try:
        ctx = RouteContext(weather=3, congestion=2, weekhour=2 * 24 + 9)
        assert not router.is_cached(ctx)
        router.prefetch(ctx, urgent=True)
        t_end = time.time() + 60
        while not router.is_cached(ctx) and time.time() < t_end:
            time.sleep(0.01)
        assert router.is_cached(ctx)
        assert router.stats()["async_paced"] == before + 1
    finally:
        router.gpu.set_builder_pacing(0)
    src, dst = synth_route_queries(g, 2000, seed=11)
    sec, met, st, paths = router.route(src, dst, ctx)
    assert router.last_metric["fresh"] is False          # the background build was used
    c = router.costs(ctx)
    mcc = cpu.customize(c, g.length_m)
    s2, m2, st2, p2 = cpu.query(mcc, src, dst, True)
    assert np.array_equal(sec, s2) and np.array_equal(met, m2) and np.array_equal(st, st2)
    assert all(np.array_equal(a, b) for a, b in zip(paths, p2))


def test_no_triangle_table_fallback_bit_identical(monkeypatch):
    """ROUTEST_CCH_TRI_GB=0: without the triangle table the customization is the fallback path
    (basic_level_kernel / perfect_level_kernel, binary searches).  Its metric arrays equal the
    accelerated path's bit for bit, and its answers the CPU reference's."""
    from routest_amd import _rt
    from routest_amd.routing.cch import RoadRouter
    g = synth_road_graph(20_000, seed=5)
    m = default_model(hidden=64, steps=50)
    cost = edge_costs(g, m, device="cuda:0")
    ra = RoadRouter(g, m, device="cuda:0")
    st = ra.stats()
    assert st["triangle_table"] and st["supernodal"], st
    monkeypatch.setenv("ROUTEST_CCH_TRI_GB", "0")
    rb = RoadRouter(g, m, device="cuda:0")
    st = rb.stats()
    assert not st["triangle_table"] and not st["supernodal"], st
    ka = ra.metric_from_costs(1 << 40, cost)
    kb = rb.metric_from_costs(1 << 40, cost)
    da = {k: v.cpu() for k, v in ra.gpu.metric_dump(ka).items()}
    db = {k: v.cpu() for k, v in rb.gpu.metric_dump(kb).items()}
    assert da.keys() == db.keys()
    for name, ref in da.items():
        assert torch.equal(db[name], ref), name
    cpu = _rt.CCH(g.indptr, g.indices, g.lat, g.lon, 0)
    mc = cpu.customize(cost, g.length_m)
    src, dst = synth_route_queries(g, 1000, seed=3)
    a = rb.route(src, dst, kb, want_path=False)
    b = cpu.query(mc, src, dst, False)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_supernodal_fronts_bit_identical_to_per_level(setup, monkeypatch):
    """ROUTEST_CCH_DENSE: the dense-front customization of the elimination tree's top
    (csrc/cch_customize.hip sup_*_kernel: blocked (min, +) elimination / back substitution per chain) gives the per-level
    kernels' metric arrays bit for bit — with no fronts (0), every chain a front (1), only long chains
    (32) and the default — and so the CPU reference's answers (the other tests here run the default)."""
    from routest_amd.routing.cch import RoadRouter
    g, m, router, cost, key, cpu, mc = setup
    st = router.stats()
    assert st["supernodal"] and st["sup_fronts"] > 0 and st["sparse_depths"] < st["max_depth"], st
    base = {k: v.cpu() for k, v in router.gpu.metric_dump(key).items()}
    for thr in ("0", "1", "32"):
        monkeypatch.setenv("ROUTEST_CCH_DENSE", thr)
        r2 = RoadRouter(g, m, device="cuda:0")
        assert bool(r2.stats()["supernodal"]) == (thr != "0"), r2.stats()
        k2 = r2.metric_from_costs(1 << 42, cost)
        d = {k: v.cpu() for k, v in r2.gpu.metric_dump(k2).items()}
        for name, ref in base.items():
            assert torch.equal(d[name], ref), (thr, name)
        del r2
