"""Edge-based map matching on the GPU (csrc/map_match_edge.hip) against the reference
(routing/mapmatch_edge.py): every comparison is exact equality.

* ``_C.mm_edge_candidates`` on the 3000-node graph and the hand-built tie set: k = 1, 8, 16; radius
  25,000 and 100,000 cm; 1, 63, 64, 65 and 1000 fixes; fixes on edges, outside the bounding box and
  beyond the radius from everything;
* a dense patch of 4000 short edges in 4 km² with survivor counts below, exactly at and far above
  the kernel's LDS buffer: the kernel's own survivor counts are asserted, so the rescanning
  fallback is known to have run;
* ``_C.mm_edge_route_cm`` for K = 1, 3, 8, 16 with unreachable cells, padding, equal head and tail
  and same-edge pairs;
* ``RoadRouter.rect_rows`` with a node repeated within a row: the repeated columns are bit-equal to
  each other and to the CPU router;
* end to end: ``match_traces_edge`` on cuda:0 equals the CPU router's answer in every field on
  simulated traces, the break across the two-islands cut, an unmatched fix and a context customized
  on the GPU; ``POST /api/match`` with ``"snap": "edge"`` on the GPU equals the CPU answer.
"""
import numpy as np
import pytest
import torch

import _mapmatch_cases as cases
import _mapmatch_edge_cases as ec
from routest_amd.routing import mapmatch as mm
from routest_amd.routing import mapmatch_edge as me
from routest_amd.routing.mapmatch import MatchParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def C():
    from routest_amd.ops import _ext
    return _ext.native(required=True)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_grid(nqy, nqx, edges, cell=None):
    grid = me.build_edge_grid(nqy, nqx, edges, cell)
    dev = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in grid.items()}
    dev["rec"] = _t(me.pack_records(edges))
    return grid, dev


def _gpu_candidates(C, dev, py, px, radius_cm, k):
    out = C.mm_edge_candidates(dev["start"], dev["items"], dev["rec"], dev["y0"], dev["x0"], dev["cell"], dev["ny"],
                               dev["nx"], _t(py), _t(px), radius_cm, k)
    return [o.cpu().numpy() for o in out]


def _prefix(ref, k):
    """The reference's answer for a smaller k: the first k candidates."""
    ce, cd2, cfq, nc = ref
    return ce[:, :k], cd2[:, :k], cfq[:, :k], np.minimum(nc, k).astype(np.int32)


def _equal(ref, got):
    for a, b in zip(ref, got):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------- candidates
@pytest.fixture(scope="module")
def plain():
    """The 3000-node graph, its edge grid on the device, 1000 fixes and the reference's answers with
    k = 16 per radius (computed once; a smaller k is their prefix)."""
    g, _ = cases.plain_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    edges = me.graph_edges(g)
    grid, dev = _dev_grid(nqy, nqx, edges)
    rng = np.random.default_rng(0)
    lat = rng.uniform(g.lat.min() - 0.02, g.lat.max() + 0.02, 1000)
    lon = rng.uniform(g.lon.min() - 0.02, g.lon.max() + 0.02, 1000)
    on = ec.fixes_on_edges(g, rng.integers(0, g.num_edges, 300), rng.random(300))
    lat[:300], lon[:300] = on[:, 0], on[:, 1]                              # on random edges
    lat[300], lon[300] = g.lat.max() + 0.5, g.lon.mean()                   # far outside the bounding box
    lat[301], lon[301] = g.lat.min() - 0.3, g.lon.min() - 0.3
    low = int(np.argmin(g.lat))
    lat[302], lon[302] = g.lat[low] - 0.001, g.lon[low]                    # outside the box, an edge in range
    py, px = mm.quantize(lat, lon)
    ref = {r: me.edge_candidates_ref(edges, py, px, r, 16) for r in (25_000, 100_000)}
    return g, edges, grid, dev, py, px, ref


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("radius_cm", [25_000, 100_000])
def test_candidates_equal_reference(C, plain, k, radius_cm):
    g, edges, grid, dev, py, px, ref = plain
    want = _prefix(ref[radius_cm], k)
    got = _gpu_candidates(C, dev, py, px, radius_cm, k)
    _equal(want, got[:4])
    assert np.array_equal(got[4][:40], ec.survivors(grid, edges, py[:40], px[:40], radius_cm))
    nc = want[3]
    assert (nc[:300] >= 1).all() and (want[1][:300, 0] <= 25).all() and nc[300] == 0 and nc[301] == 0 and nc[302] >= 1
    assert (nc == 0).sum() > 2                                             # beyond the radius from everything
    if k == 1:
        assert (nc == 1).any()
    if k == 16:
        assert ((nc > 0) & (nc < k)).any()                                 # fewer edges in range than asked for


@pytest.mark.parametrize("P", [1, 63, 64, 65])
def test_candidates_point_counts(C, plain, P):
    g, edges, grid, dev, py, px, ref = plain
    s = slice(270, 270 + P)                                                # on edges, then random ones
    want = me.edge_candidates_ref(edges, py[s], px[s], 60_000, 8)
    _equal(want, _gpu_candidates(C, dev, py[s], px[s], 60_000, 8)[:4])


def test_candidates_do_not_depend_on_the_cell(C, plain):
    g, edges, grid, dev, py, px, ref = plain
    nqy, nqx = mm.quantize(g.lat, g.lon)
    for cell in (31_337, 10 ** 8):                                         # small cells; a single cell
        _, other = _dev_grid(nqy, nqx, edges, cell)
        _equal(_prefix(ref[25_000], 8), _gpu_candidates(C, other, py, px, 25_000, 8)[:4])


def test_tie_set(C):
    nqy, nqx, edges, eid = ec.tie_edges()
    _, dev = _dev_grid(nqy, nqx, edges)
    py, px = ec.tie_fixes(25_000)
    for k in (2, 3, 8):
        ref = me.edge_candidates_ref(edges, py, px, 25_000, k)
        ec.check_tie_answers(eid, ref, k)
        _equal(ref, _gpu_candidates(C, dev, py, px, 25_000, k)[:4])


def test_dense_patch_forces_the_rescanning_fallback(C):
    """Survivor counts below, at and above the LDS buffer's capacity."""
    cap = int(C.mm_edge_lds_capacity())
    nqy, nqx, edges, _ = ec.dense_patch()
    grid, dev = _dev_grid(nqy, nqx, edges)
    assert len(edges["ok"]) == 4000 and edges["ok"].all()
    rng = np.random.default_rng(9)
    py = (ec.Y0 + rng.integers(-20_000, 220_000, 64)).astype(np.int64)
    px = (ec.X0 + rng.integers(-20_000, 220_000, 64)).astype(np.int64)
    py[:8], px[:8] = ec.Y0 + 100_000 + np.arange(8) * 3000, ec.X0 + 100_000 - np.arange(8) * 2000     # well inside
    # a radius at which one of the first fixes has exactly `cap` survivors
    exact = None
    for p in range(8):
        r, n = ec.radius_for_survivors(grid, edges, int(py[p]), int(px[p]), cap)
        if n == cap:
            exact = (p, r)
            break
    assert exact is not None
    seen = []
    for radius_cm in (15_000, exact[1], exact[1] + 1500, 100_000):
        surv = ec.survivors(grid, edges, py, px, radius_cm)
        seen.append(surv)
        for k in (8, 16):
            ref = me.edge_candidates_ref(edges, py, px, radius_cm, k)
            got = _gpu_candidates(C, dev, py, px, radius_cm, k)
            _equal(ref, got[:4])
            assert np.array_equal(got[4], surv)                            # the kernel saw the same counts
    assert seen[0].max() < cap and (seen[0] > 64).any()                    # more than one item per lane, all in LDS
    assert seen[1][exact[0]] == cap                                        # the buffer exactly full
    assert seen[2][exact[0]] > cap                                         # just over: the fallback
    assert (seen[3] > 8 * cap).any() and (seen[3][:8] > cap).all()         # far over
    # duplicates: an edge listed in several cells is one candidate
    assert len(grid["items"]) > 4000
    ref = me.edge_candidates_ref(edges, py, px, 100_000, 16)
    assert all(len(set(row[:n].tolist())) == n for row, n in zip(ref[0], ref[3]))


# ------------------------------------------------------------------------------ route centimetres
@pytest.mark.parametrize("K", [1, 3, 8, 16])
def test_route_cm_equals_reference(C, K):
    rng = np.random.default_rng(K)
    rows = 257
    e1 = rng.integers(0, 40, (rows, K)).astype(np.int32)
    e2 = rng.integers(0, 40, (rows, K)).astype(np.int32)
    e2[::3, 0] = e1[::3, 0]                                               # same-edge pairs, forward and backward
    lc1 = rng.integers(0, 200_000, (rows, K)).astype(np.int64)
    off1 = (lc1 * rng.random((rows, K))).astype(np.int64)
    off2 = rng.integers(0, 200_000, (rows, K)).astype(np.int64)
    off2[::6, 0] = off1[::6, 0]                                           # the same point
    n1, n2 = rng.integers(1, K + 1, rows), rng.integers(1, K + 1, rows)
    e1[np.arange(K)[None, :] >= n1[:, None]] = -1                         # padding
    e2[np.arange(K)[None, :] >= n2[:, None]] = -1
    met = (rng.random((rows, K, K)) * 30_000).astype(np.float32)
    met[rng.random((rows, K, K)) < 0.15] = np.inf                         # no route
    met[rng.random((rows, K, K)) < 0.15] = 0.0                            # equal head and tail
    met[0, 0, 0] = 16_777_217.0                                           # metres beyond f32's integers
    ref = me.edge_route_cm_ref(met, e1, off1, lc1, e2, off2)
    got = C.mm_edge_route_cm(_t(met), _t(e1), _t(off1), _t(lc1), _t(e2), _t(off2)).cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(ref, got)
    real = (e1 >= 0)[:, :, None] & (e2 >= 0)[:, None, :]
    assert (ref[~real] == -1).all() and (ref[real] == -1).any() and (ref[real] >= 0).any()
    same = real & (e1[:, :, None] == e2[:, None, :])
    assert (same & (off2[:, None, :] >= off1[:, :, None])).any() and (same & (off2[:, None, :] < off1[:, :, None])).any()
    try:
        from routest_amd import _rt
    except ImportError:
        return
    assert np.array_equal(_rt.mm_edge_route_cm(met, e1, off1, lc1, e2, off2), ref)


# ------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def routers():
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.serve.eta_service import default_model
    g, cost = cases.islands_graph()
    model = default_model(hidden=64, steps=50)
    gpu = RoadRouter(g, model, device=DEV)
    cpu = RoadRouter(g, model, device=None)
    key = 1 << 40
    gpu.metric_from_costs(key, cost)
    cpu.metric_from_costs(key, cost)
    return g, cost, gpu, cpu, key


def test_rect_rows_with_a_node_repeated_within_a_row(routers):
    g, cost, gpu, cpu, key = routers
    src = np.array([[100, 100, 250, 100], [7, 900, 7, 7]], np.int32)       # heads of candidates repeat
    dst = np.array([[400, 250, 400, 100], [900, 900, 7, 30]], np.int32)
    cnt = np.array([4, 4], np.int32)
    sec_g, met_g = (x.cpu().numpy() for x in gpu.rect_rows(_t(src), _t(cnt), _t(dst), _t(cnt), key))
    sec_c, met_c = (x.numpy() for x in cpu.rect_rows(*(torch.from_numpy(a) for a in (src, cnt, dst, cnt)), key))
    for a, b in ((sec_g, sec_c), (met_g, met_c)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for m in (sec_g, met_g):
        assert np.array_equal(m[0, 0].view(np.uint32), m[0, 1].view(np.uint32))          # repeated sources
        assert np.array_equal(m[0, 0].view(np.uint32), m[0, 3].view(np.uint32))
        assert np.array_equal(m[0, :, 0].view(np.uint32), m[0, :, 2].view(np.uint32))    # repeated destinations
        assert np.array_equal(m[1, :, 0].view(np.uint32), m[1, :, 1].view(np.uint32))
        assert m[0, 0, 3] == 0 and m[0, 2, 1] == 0 and m[1, 0, 2] == 0                   # equal head and tail
    assert np.isfinite(met_g).any() and (met_g > 0).any()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("edge", "fq", "proj", "cand_d2", "segment", "matching"):
            assert x[f].dtype == y[f].dtype and np.array_equal(x[f], y[f]), f
        assert x["n_segments"] == y["n_segments"] and len(x["matchings"]) == len(y["matchings"])
        for m, n in zip(x["matchings"], y["matchings"]):
            assert np.array_equal(m["nodes"], n["nodes"]) and m["segment"] == n["segment"]
            assert m["duration"] == n["duration"] and m["distance"] == n["distance"]
            assert np.array_equal(m["start"], n["start"]) and np.array_equal(m["end"], n["end"])


def test_match_traces_edge_gpu_equals_cpu(routers):
    from routest_amd.routing.cch import RouteContext
    g, cost, gpu, cpu, key = routers
    sim = cases.simulated_traces(g, cpu, key, 16, seed=3, noise_m=15.0)
    fixes = [f for f, _ in sim][:3]
    assert len(fixes) == 3
    cut, _, n_west = cases.cross_cut_trace(g, cpu, key)
    fixes.append(cut)
    fixes.append(cases.with_unmatched_fix(g, fixes[0], 1))
    p = MatchParams()
    ref = me.match_traces_edge(cpu, g, fixes, key, p)
    # the inputs hold all three situations (checked on the reference's answer)
    assert any(r["n_segments"] == 1 and (r["edge"] >= 0).all() and len(r["matchings"][0]["nodes"]) > 3 for r in ref)
    assert ref[-2]["n_segments"] >= 2 and ref[-2]["segment"][n_west - 1] + 1 == ref[-2]["segment"][n_west]
    assert ref[-1]["edge"][1] == -1 and (np.delete(ref[-1]["edge"], 1) >= 0).all()
    stats = {}
    _same(ref, me.match_traces_edge(gpu, g, fixes, key, p, stats=stats))
    assert stats["fixes"] == sum(len(f) for f in fixes) and stats["pairs_queried"] > 0 and stats["candidates_s"] > 0
    wide = MatchParams(k=16, radius_m=1000, sigma_m=20, beta_m=5)         # many candidates per fix
    _same(me.match_traces_edge(cpu, g, fixes, key, wide), me.match_traces_edge(gpu, g, fixes, key, wide))
    # a routing context customized on the GPU; the CPU router gets that context's edge costs
    ctx = RouteContext.from_request({"context": {"weather": "Stormy", "traffic": "Jam",
                                                 "pickup_time": "2025-08-29T18:00:00"}})
    on_gpu = me.match_traces_edge(gpu, g, fixes, ctx, p)
    ccost = gpu.costs(ctx)
    assert not np.array_equal(ccost, cost)
    cpu.metric_from_costs(77, ccost)
    _same(me.match_traces_edge(cpu, g, fixes, 77, p), on_gpu)


def test_match_endpoint_edge_mode_on_the_gpu():
    from fastapi.testclient import TestClient
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.serve.eta_service import EtaService
    g, cost = cases.plain_graph()
    on_gpu = GraphProvider(g, cost, device=torch.device("cuda", 0), engine="cch")
    on_cpu = GraphProvider(g, cost, device=None, engine="cch")
    _, _, st, paths = on_cpu.router().route([100, 900], [400, 300], on_cpu.FIXED_KEY)
    assert (st == 0).all()
    mid = [ec.fixes_along(g, p, 0.4)[0] for p in paths]
    mid[1][1] = (float(g.lat.max()) + 0.05, mid[1][1, 1])                            # an unmatched fix
    body = {"traces": [{"coordinates": [[float(lo), float(la)] for la, lo in f]} for f in mid], "snap": "edge", "k": 6}
    s = load_settings(env={}, dotenv_path=None, devices=[0], route_batch="0", warm_scorer=False)
    sv = build_services(s, eta=EtaService(None, device="cpu"), provider=on_gpu, store=None)
    with TestClient(create_app(sv)) as c:
        resp = c.post("/api/match", json=body)
        assert resp.status_code == 200, resp.text
        out = resp.json()
    assert on_gpu.router(sv.route_device).gpu is not None
    want = mm.match_response(on_cpu, body)
    assert out == want
    tps = out["traces"][0]["tracepoints"]
    assert None not in tps and out["traces"][1]["tracepoints"][1] is None
    assert all(set(tp) == {"location", "edge", "matchings_index", "distance"} for tp in tps)
    sv.close()
