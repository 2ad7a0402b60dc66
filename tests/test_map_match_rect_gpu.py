"""Map matching with the steps' transitions asked as rectangular matrix rows
(``match_traces(..., transitions="matrix")``: ``RoadRouter.rect_rows``, csrc/cch_query.hip
meet_rect_kernel) against the pair-query path and the CPU router: every comparison is ``==``."""
import numpy as np
import pytest

import _mapmatch_cases as cases
from routest_amd.routing import mapmatch as mm
from routest_amd.routing.mapmatch import MatchParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY = 1 << 40


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("matched", "segment", "matching", "cand_d2"):
            assert np.array_equal(x[f], y[f]), f
        assert x["n_segments"] == y["n_segments"] and len(x["matchings"]) == len(y["matchings"])
        for m, n in zip(x["matchings"], y["matchings"]):
            assert np.array_equal(m["nodes"], n["nodes"]) and m["segment"] == n["segment"]
            assert m["duration"] == n["duration"] and m["distance"] == n["distance"]


@pytest.fixture(scope="module")
def world():
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.serve.eta_service import default_model
    g, cost = cases.islands_graph()
    model = default_model(hidden=64, steps=50)
    gpu = RoadRouter(g, model, device=DEV)
    cpu = RoadRouter(g, model, device=None)
    gpu.metric_from_costs(KEY, cost)
    cpu.metric_from_costs(KEY, cost)
    fixes = [f for f, _ in cases.simulated_traces(g, cpu, KEY, 12, seed=3, noise_m=15.0)]
    cut, _, n_west = cases.cross_cut_trace(g, cpu, KEY)
    fixes.append(cut)                                                   # breaks into two segments
    fixes.append(cases.with_unmatched_fix(g, fixes[0], 1))              # an unmatched fix
    return g, gpu, cpu, fixes, n_west


PARAMS = [MatchParams(), MatchParams(k=1), MatchParams(k=16, radius_m=600, sigma_m=20, beta_m=5)]


@pytest.mark.parametrize("p", PARAMS, ids=["k8", "k1", "k16"])
def test_matrix_transitions_equal_pairs_and_cpu(world, p):
    g, gpu, cpu, fixes, n_west = world
    ref = mm.match_traces(cpu, g, fixes, KEY, p, transitions="pairs")
    assert ref[-2]["n_segments"] >= 2 and ref[-2]["segment"][n_west - 1] + 1 == ref[-2]["segment"][n_west]
    assert ref[-1]["matched"][1] == -1 and (np.delete(ref[-1]["matched"], 1) >= 0).all()
    sp, sm = {}, {}
    pairs = mm.match_traces(gpu, g, fixes, KEY, p, transitions="pairs", stats=sp)
    matrix = mm.match_traces(gpu, g, fixes, KEY, p, transitions="matrix", stats=sm)
    _same(ref, pairs)
    _same(ref, matrix)
    _same(ref, mm.match_traces(gpu, g, fixes, KEY, p))                   # the default ("auto")
    assert set(sp) == set(sm) and sm["pairs_queried"] >= sp["pairs_queried"] > 0
    kept = sum(int((r["matched"] >= 0).sum()) for r in ref)              # more than the steps there are
    if p.k == 16:
        assert sm["pairs_queried"] > kept                                # blocks of several cells
    if p.k == 1:
        assert sm["pairs_queried"] < kept                                # one cell per step


def test_matrix_transitions_in_several_chunks(world, monkeypatch):
    """RECT_MAX_JOBS below one step's 2K chains (rows one per call, columns split) and at a few
    rows per call."""
    g, gpu, cpu, fixes, _ = world
    p = PARAMS[2]
    want = mm.match_traces(gpu, g, fixes, KEY, p, transitions="pairs")
    calls = []
    orig = gpu._rect_call_gpu
    monkeypatch.setattr(gpu, "_rect_call_gpu", lambda *a: (calls.append(tuple(a[0].shape) + tuple(a[2].shape)), orig(*a))[1],
                        raising=False)
    for mj, rows in ((24, 1), (100, 3)):
        calls.clear()
        monkeypatch.setattr(mm, "RECT_MAX_JOBS", mj)
        _same(want, mm.match_traces(gpu, g, fixes, KEY, p, transitions="matrix"))
        assert len(calls) > 3 and max(c[0] for c in calls) == rows and all(c[0] * (c[1] + c[3]) <= mj for c in calls)
