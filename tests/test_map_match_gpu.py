"""GPS-trace map matching on the GPU (csrc/map_match.hip) against the reference
(routing/mapmatch.py; where present also ``_rt``): every comparison is exact equality.

* ``_C.mm_candidates`` on the 3000-node graph and the hand-built tie graph (two nodes equidistant
  from a fix, two at identical coordinates: the node id decides): fixes on a node, outside the
  bounding box, beyond the radius from everything; k = 1, 8, 16; radii with fewer than k, exactly
  k, more than 64 and several hundred nodes in range; 1, 63, 64, 65 and 1000 fixes;
* ``_C.mm_viterbi`` on generated cost tensors: B = 1, 3, 130; T = 1, 2, 63, 64, 65 and one trace of
  2048; K = 1, 3, 8, 16 with n_cand varying per step; equal costs, dead states, breaks at step 1, at
  the last step and twice in a row, no feasible transition at all, costs at the parameter maxima,
  ragged npts;
* end to end: ``match_traces`` on cuda:0 equals ``match_traces`` on the CPU router (matched,
  segment, segment node paths, durations, distances) on simulated traces holding a whole match, a
  break across the two-islands cut and an unmatched fix, fixed costs and a context customized on
  the GPU.
"""
import numpy as np
import pytest
import torch

import _mapmatch_cases as cases
from routest_amd.routing import mapmatch as mm
from routest_amd.routing.mapmatch import MatchParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def C():
    from routest_amd.ops import _ext
    return _ext.native(required=True)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------- candidates
@pytest.fixture(scope="module")
def plain():
    """The 3000-node graph, its grid on the device, 1000 fixes and the reference's answers."""
    g, cost = cases.plain_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    grid = mm.build_grid(nqy, nqx)
    dev = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in grid.items()}
    dev["nqy"], dev["nqx"] = _t(nqy), _t(nqx)
    rng = np.random.default_rng(0)
    lat = rng.uniform(g.lat.min() - 0.02, g.lat.max() + 0.02, 1000)
    lon = rng.uniform(g.lon.min() - 0.02, g.lon.max() + 0.02, 1000)
    on = rng.integers(0, g.num_nodes, 20)
    lat[:20], lon[:20] = g.lat[on], g.lon[on]                              # exactly on a node
    lat[20], lon[20] = g.lat.max() + 0.5, g.lon.mean()                     # far outside the bounding box
    lat[21], lon[21] = g.lat.min() - 0.3, g.lon.min() - 0.3
    low = int(np.argmin(g.lat))
    lat[22], lon[22] = g.lat[low] - 0.001, g.lon[low]                      # outside the box, a node in range
    py, px = mm.quantize(lat, lon)
    return g, nqy, nqx, dev, py, px


def _gpu_candidates(C, dev, py, px, radius_cm, k):
    out = C.mm_candidates(dev["start"], dev["items"], dev["nqy"], dev["nqx"], dev["y0"], dev["x0"], dev["cell"],
                          dev["ny"], dev["nx"], _t(py), _t(px), radius_cm, k)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("radius_cm", [25_000, 100_000])
def test_candidates_equal_reference(C, plain, k, radius_cm):
    g, nqy, nqx, dev, py, px = plain
    ref = mm.candidates_ref(nqy, nqx, py, px, radius_cm, k)
    got = _gpu_candidates(C, dev, py, px, radius_cm, k)
    for a, b in zip(ref, got):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    nc = ref[2]
    assert (ref[1][:20, 0] == 0).all() and nc[20] == 0 and nc[21] == 0 and nc[22] >= 1
    assert (nc == 0).sum() > 2                                             # beyond the radius from everything
    if k == 1:
        assert (nc == 1).any()
    if k == 16:
        assert ((nc > 0) & (nc < k)).any()                                 # fewer nodes in range than asked for


@pytest.mark.parametrize("P", [1, 63, 64, 65])
def test_candidates_point_counts(C, plain, P):
    g, nqy, nqx, dev, py, px = plain
    ref = mm.candidates_ref(nqy, nqx, py[:P], px[:P], 60_000, 8)
    for a, b in zip(ref, _gpu_candidates(C, dev, py[:P], px[:P], 60_000, 8)):
        assert np.array_equal(a, b)


def test_candidates_many_nodes_in_range(C):
    """A dense patch: about 40 / 150 / 600 nodes within the radius (up to ten items per lane),
    exactly k in range, and duplicates of whole nodes."""
    rng = np.random.default_rng(4)
    n = 4000
    qy = 162_000_000 + rng.integers(0, 400_000, n)
    qx = 1_300_000_000 + rng.integers(0, 400_000, n)
    qy[1000:1010], qx[1000:1010] = qy[0], qx[0]                            # eleven nodes on one spot
    qy, qx = qy.astype(np.int64), qx.astype(np.int64)
    grid = mm.build_grid(qy, qx)
    dev = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in grid.items()}
    dev["nqy"], dev["nqx"] = _t(qy), _t(qx)
    py = np.concatenate([[qy[0]], 162_000_000 + rng.integers(-50_000, 450_000, 64)]).astype(np.int64)
    px = np.concatenate([[qx[0]], 1_300_000_000 + rng.integers(-50_000, 450_000, 64)]).astype(np.int64)
    seen = []
    for radius_cm in (25_000, 50_000, 100_000):
        for k in (8, 16):
            ref = mm.candidates_ref(qy, qx, py, px, radius_cm, k)
            for a, b in zip(ref, _gpu_candidates(C, dev, py, px, radius_cm, k)):
                assert np.array_equal(a, b)
            assert ref[0][0, :min(k, 11)].tolist() == ([0] + list(range(1000, 1010)))[:k]     # node id decides
        dy, dx = qy[None, :] - py[:, None], qx[None, :] - px[:, None]
        seen.append(int((dy * dy + dx * dx <= radius_cm * radius_cm).sum(1).max()))
    assert seen[0] > 64 and seen[2] > 300
    # exactly k nodes in range: the fix's 11 co-located nodes with a 1 cm radius
    ref = mm.candidates_ref(qy, qx, py[:1], px[:1], 1, 11)
    assert ref[2][0] == 11
    for a, b in zip(ref, _gpu_candidates(C, dev, py[:1], px[:1], 1, 11)):
        assert np.array_equal(a, b)


def test_candidate_ties_go_to_the_lower_node_id(C):
    g, (fy, fx) = cases.tie_graph()
    nqy, nqx = mm.quantize(g.lat, g.lon)
    grid = mm.build_grid(nqy, nqx)
    dev = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in grid.items()}
    dev["nqy"], dev["nqx"] = _t(nqy), _t(nqx)
    py, px = np.array([fy, nqy[2]], np.int64), np.array([fx, nqx[2]], np.int64)
    for k in (1, 2, 4, 8):
        ref = mm.candidates_ref(nqy, nqx, py, px, 50_000, k)
        assert ref[0][0, :min(k, 4)].tolist() == [0, 1, 2, 3][:k] and ref[0][1, :min(k, 2)].tolist() == [2, 3][:k]
        assert ref[1][0, 0] == ref[1][0, min(k, 2) - 1]                     # equidistant
        for a, b in zip(ref, _gpu_candidates(C, dev, py, px, 50_000, k)):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------- Viterbi
def _gpu_viterbi(C, case, p):
    cd, nc, route, g, npts = case
    out = C.mm_viterbi(_t(cd), _t(nc), _t(route), _t(g), _t(npts), p.beta_cm, p.sigma_cm, p.max_detour_cm)
    return [o.cpu().numpy() for o in out]


def _reference(case, p):
    ref = mm.viterbi_batch_ref(*case, p)
    try:
        from routest_amd import _rt
    except ImportError:
        return ref
    cd, nc, route, g, npts = case
    nat = _rt.mm_viterbi(cd, nc, route, g, npts, p.beta_cm, p.sigma_cm, p.max_detour_cm)
    for a, b in zip(ref, nat):
        assert np.array_equal(a, b)
    return ref


MAXP = dict(radius_m=1000, sigma_m=200, beta_m=100, max_detour_m=5000)


@pytest.mark.parametrize("kind", ["random", "ties", "dead", "none", "max", "breaks"])
@pytest.mark.parametrize("B,T,K", [(1, 1, 1), (3, 2, 3), (3, 63, 8), (1, 64, 16), (3, 65, 3), (130, 9, 8), (130, 5, 16),
                                   (3, 64, 1)])
def test_viterbi_equals_reference(C, B, T, K, kind):
    p = MatchParams(k=K, **MAXP) if kind == "max" else MatchParams(k=K)
    case = cases.viterbi_case(7 * B + 3 * T + K, B, T, K, kind, p, ragged=B >= 3)
    ref = _reference(case, p)
    got = _gpu_viterbi(C, case, p)
    for name, a, b in zip(("choice", "segment", "n_segments", "cost"), ref, got):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b), (name, B, T, K, kind)
    choice, seg, nseg, cost = ref
    full = np.flatnonzero(case[4] == T)
    assert len(full)
    if kind == "none":
        assert (nseg[full] == T).all()
    if kind == "breaks" and T >= 2:
        assert (seg[full, 1] == 1).all() and (seg[full, T - 1] == seg[full, T - 2] + 1).all()
        if T >= 6:
            assert (seg[full, T // 2 + 1] == seg[full, T // 2 - 1] + 2).all()
    if kind == "max" and T >= 2:
        assert cost[full].min() > 2 ** 40            # a 32-bit intermediate anywhere would show


def test_viterbi_longest_trace(C):
    """One trace of 2048 fixes with 16 candidates, ordinary costs and costs at the maxima."""
    for kind, p in (("random", MatchParams(k=16)), ("max", MatchParams(k=16, **MAXP)), ("breaks", MatchParams(k=16))):
        case = cases.viterbi_case(11, 1, 2048, 16, kind, p)
        ref = _reference(case, p)
        for a, b in zip(ref, _gpu_viterbi(C, case, p)):
            assert np.array_equal(a, b), kind
        if kind == "max":
            assert 2 ** 59 < ref[3][0] < 2 ** 62     # the documented bound, nearly reached


def test_viterbi_lowest_predecessor_and_final_state(C):
    p = MatchParams(k=3)
    cd = np.zeros((1, 3, 3), np.int64)
    nc = np.full((1, 3), 3, np.int32)
    g = np.full((1, 2), 1000, np.int64)
    route = np.full((1, 2, 3, 3), 1000, np.int64)
    npts = np.array([3], np.int32)
    assert _gpu_viterbi(C, (cd, nc, route, g, npts), p)[0].tolist() == [[0, 0, 0]]
    route[0, 1, 0, :] = -1
    assert _gpu_viterbi(C, (cd, nc, route, g, npts), p)[0].tolist() == [[0, 1, 0]]


# ------------------------------------------------------------------------------------- end to end
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("matched", "segment", "matching", "cand_d2"):
            assert np.array_equal(x[f], y[f]), f
        assert x["n_segments"] == y["n_segments"] and len(x["matchings"]) == len(y["matchings"])
        for m, n in zip(x["matchings"], y["matchings"]):
            assert np.array_equal(m["nodes"], n["nodes"]) and m["segment"] == n["segment"]
            assert m["duration"] == n["duration"] and m["distance"] == n["distance"]


def test_match_traces_gpu_equals_cpu():
    from routest_amd.routing.cch import RoadRouter, RouteContext
    from routest_amd.serve.eta_service import default_model
    g, cost = cases.islands_graph()
    model = default_model(hidden=64, steps=50)
    gpu = RoadRouter(g, model, device=DEV)
    cpu = RoadRouter(g, model, device=None)
    key = 1 << 40
    gpu.metric_from_costs(key, cost)
    cpu.metric_from_costs(key, cost)
    sim = cases.simulated_traces(g, cpu, key, 16, seed=3, noise_m=15.0)
    fixes = [f for f, _ in sim]
    cut, _, n_west = cases.cross_cut_trace(g, cpu, key)
    fixes.append(cut)
    fixes.append(cases.with_unmatched_fix(g, fixes[0], 1))
    p = MatchParams()
    ref = mm.match_traces(cpu, g, fixes, key, p)
    # the inputs hold all three situations (checked on the reference's answer)
    assert any(r["n_segments"] == 1 and (r["matched"] >= 0).all() and len(r["matchings"][0]["nodes"]) > 3 for r in ref)
    assert ref[-2]["n_segments"] >= 2 and ref[-2]["segment"][n_west - 1] + 1 == ref[-2]["segment"][n_west]
    assert ref[-1]["matched"][1] == -1 and (np.delete(ref[-1]["matched"], 1) >= 0).all()
    _same(ref, mm.match_traces(gpu, g, fixes, key, p))
    wide = MatchParams(k=8, radius_m=1000, sigma_m=20, beta_m=5)          # several candidates per fix
    _same(mm.match_traces(cpu, g, fixes, key, wide), mm.match_traces(gpu, g, fixes, key, wide))
    # a routing context customized on the GPU; the CPU router gets that context's edge costs
    ctx = RouteContext.from_request({"context": {"weather": "Stormy", "traffic": "Jam",
                                                 "pickup_time": "2025-08-29T18:00:00"}})
    on_gpu = mm.match_traces(gpu, g, fixes, ctx, p)
    ccost = gpu.costs(ctx)
    assert not np.array_equal(ccost, cost)
    cpu.metric_from_costs(77, ccost)
    _same(mm.match_traces(cpu, g, fixes, 77, p), on_gpu)
