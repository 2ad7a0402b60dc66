"""K4 tree-ensemble compatibility path: sklearn parity, XGBoost-JSON round trip, GPU kernel."""
import json

import numpy as np
import pytest
import torch

from _forest_synth import FMAP_PERM, I32_MAX, I32_MIN, LDS_NODES, TreeGen, edge_records, scalar_reference
from routest_amd.data.synth import synth_records, synth_trips
from routest_amd.models.features import records_to_features
from routest_amd.models.forest import ForestModel


@pytest.fixture(scope="module")
def hgb():
    from sklearn.ensemble import HistGradientBoostingRegressor
    x, y = synth_trips(20000, 0)
    x[::97, 10] = np.nan  # exercise missing-value routing
    return HistGradientBoostingRegressor(max_iter=120, max_leaf_nodes=31, random_state=0).fit(x, y)


def test_sklearn_conversion_matches_sklearn(hgb):
    m = ForestModel.from_sklearn_hgb(hgb)
    x, _ = synth_trips(5000, 1)
    x[::50, 10] = np.nan
    np.testing.assert_allclose(m.predict_features(x), hgb.predict(x), rtol=1e-5, atol=1e-4)


def test_xgboost_json_roundtrip(hgb, tmp_path):
    m = ForestModel.from_sklearn_hgb(hgb)
    p = tmp_path / "eta_xgb.json"
    p.write_text(json.dumps(m.to_xgboost_json()))
    m2 = ForestModel.from_xgboost_json(str(p))
    assert not m2.le
    x, _ = synth_trips(3000, 2)
    np.testing.assert_allclose(m2.predict_features(x), m.predict_features(x), rtol=1e-6, atol=1e-5)
    # load_any dispatches .json to the forest loader
    from routest_amd.models.checkpoint import load_any
    assert isinstance(load_any(str(p)), ForestModel)


def test_xgboost_feature_name_reorder(hgb):
    m = ForestModel.from_sklearn_hgb(hgb)
    d = m.to_xgboost_json()
    names = d["learner"]["feature_names"]
    perm = list(reversed(range(12)))
    # re-express the same model with features declared in reversed order
    d["learner"]["feature_names"] = [names[i] for i in perm]
    inv = {old: new for new, old in enumerate(perm)}
    for t in d["learner"]["gradient_booster"]["model"]["trees"]:
        t["split_indices"] = [inv[f] for f in t["split_indices"]]
    m3 = ForestModel.from_xgboost_json(d)
    x, _ = synth_trips(2000, 3)
    np.testing.assert_allclose(m3.predict_features(x), m.predict_features(x), rtol=1e-6, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("fmt", ["xgb", "sklearn"])
def test_forest_kernel_vs_cpu(hgb, lds, fmt):
    from routest_amd.ops.eta_mlp import records_to_tensor
    from routest_amd.serve.eta_service import ForestKernel
    m = ForestModel.from_sklearn_hgb(hgb)
    if fmt == "xgb":
        m = ForestModel.from_xgboost_json(m.to_xgboost_json())
    rec, _ = synth_records(100_003, 4)
    k = ForestKernel(m, "cuda:0", lds=lds)
    assert (k.chunks is not None) == lds
    got = k(records_to_tensor(rec).cuda()).cpu().numpy()
    ref = m.predict_features(records_to_features(rec))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-4)


def test_chunk_table():
    rng = np.random.default_rng(0)
    sizes = rng.integers(1, 300, size=200) * 2 - 1          # odd node counts (full binary trees)
    roots = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    M = int(sizes.sum())
    m = ForestModel(np.zeros(M, np.float32), np.full(M, 1 << 31, np.uint32), roots, 0.0, True)
    tab = m.chunk_table(cap=1000)
    assert tab[0].tolist() == [0, 0] and tab[-1].tolist() == [200, M]
    for (t0, n0), (t1, n1) in zip(tab[:-1], tab[1:]):
        assert n1 - n0 <= 1000 and roots[t0] == n0 and t1 > t0
    assert m.chunk_table(cap=10) is None


def test_service_serves_forest_on_cpu(hgb):
    from routest_amd.serve.eta_service import EtaService
    m = ForestModel.from_sklearn_hgb(hgb)
    svc = EtaService(model=m, device="cpu")
    try:
        minutes, iso = svc.predict_eta_minutes(weather="Sunny", traffic="High", distance_m=8000,
                                               pickup_time="2025-08-25T08:30:00", driver_age=30)
        assert minutes is not None and minutes > 0 and iso.startswith("2025-08-25T")
    finally:
        svc.close()


def test_corrupt_forest_rejected_before_launch(hgb):
    m = ForestModel.from_sklearn_hgb(hgb)
    bad = ForestModel(m.values, m.info.copy(), m.roots, m.base_score, m.le)
    bad.info[0] = (bad.info[0] & ~np.uint32(0xFFFFFF)) | np.uint32(len(bad.values) + 5)
    with pytest.raises(ValueError):
        bad.validate()
    # a child inside the forest but past its own tree's end: in the LDS kernel it can lie past the chunk
    m.validate()
    size0 = int(m.roots[1] - m.roots[0])
    assert size0 + 1 < len(m.values) and not (m.info[0] >> 31)
    nxt = ForestModel(m.values, m.info.copy(), m.roots, m.base_score, m.le)
    nxt.info[0] = (nxt.info[0] & ~np.uint32(0xFFFFFF)) | np.uint32(size0)      # first node of tree 1
    with pytest.raises(ValueError, match="out of range"):
        nxt.validate()
    nxt.info[0] = (nxt.info[0] & ~np.uint32(0xFFFFFF)) | np.uint32(size0 - 1)  # right child = that node
    with pytest.raises(ValueError, match="out of range"):
        nxt.validate()


# =============================================================================================
# Exactness on synthetic forests (tests/_forest_synth.py): integer leaves and base make every f32
# sum exact in any order, so each comparison below is np.array_equal and nothing has a tolerance.
# =============================================================================================
ROW_COUNTS = [1, 255, 256, 257, 1023, 1024, 1025]


def changed(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.mean(a != b))


class Case:
    """A synthetic forest on fixed records, with the reference computed once per ``le``."""

    def __init__(self, trees, base, rec, feature_map=None):
        self.trees, self.base, self.rec = trees, base, rec
        self.fmap = list(feature_map) if feature_map is not None else list(range(12))
        self.x = records_to_features(rec)
        self.model = {le: ForestModel._pack(trees, base, le, self.fmap) for le in (False, True)}
        self.ref = {}
        for le, m in self.model.items():
            m.validate()
            self.ref[le] = m.predict_features(self.x)
            self.ref[le].setflags(write=False)

    def assert_exact_sums(self):
        """The design rule that makes bit equality the right assertion: integer leaves and base, and
        no ordering of the sum can leave the integers f32 holds exactly."""
        m = self.model[True]
        leaf = (m.info >> 31) == 1
        assert np.array_equal(m.values[leaf], np.round(m.values[leaf])) and float(self.base).is_integer()
        assert abs(self.base) + float(np.abs(m.values[leaf]).max()) * m.num_trees < 2 ** 24

    def run_gpu(self, le, lds, n=None, expect_lds=None):
        from routest_amd.ops.eta_mlp import records_to_tensor
        from routest_amd.serve.eta_service import ForestKernel
        m = self.model[le]
        k = ForestKernel(m, "cuda:0", lds=lds)
        if expect_lds is not None:
            assert (k.chunks is not None) == expect_lds
        rec = self.rec if n is None else self.rec[:n]
        return k(records_to_tensor(rec).cuda()).cpu().numpy()


@pytest.fixture(scope="module")
def recs():
    rec = edge_records(1025, 11)
    x = records_to_features(rec)
    # the edges the issue lists are present in what the kernels read
    assert np.isnan(x[:, 10]).mean() > 0.1 and np.isnan(x[:, 11]).mean() > 0.1
    assert np.isinf(x[:, 10]).any() and np.isinf(x[:, 11]).any()
    assert (x[:, :4].sum(1) == 0).any() and (x[:, 4:8].sum(1) == 0).any()
    assert {I32_MIN, I32_MAX, -1, 86399, 86400, 86401}.issubset(set(rec["wallclock_s"].tolist()))
    tiny = np.finfo(np.float32).tiny
    for col in (x[:, 10], x[:, 11]):
        fin = col[np.isfinite(col) & (col != 0)]
        assert (np.abs(fin) >= tiny).all()                           # no subnormals
    return rec


@pytest.fixture(scope="module")
def multichunk(recs):
    """Four LDS chunks.  0: exactly LDS_NODES nodes, even tree count, opening with a single-leaf
    tree paired with a 64-deep chain and the reverse pair.  1: odd count, the unpaired tail a
    64-deep chain.  2: odd count, the tail a single leaf.  3: even count."""
    g = TreeGen(records_to_features(recs), 5)
    c0 = g.fill(LDS_NODES, head=[("leaf",), ("chain", 64), ("chain", 64), ("leaf",), ("chain", 1), ("grow", 40, 30, 40)])
    assert len(c0) % 2 == 0
    c1 = [g.tree(s) for s in [("chain", 64), ("leaf",), ("grow", 900, 3, 14), ("leaf",), ("grow", 7, 7, 7),
                              ("full", 5), ("chain", 64)]]
    # chunk 2 opens with a tree that no longer fits chunk 1
    room1 = LDS_NODES - sum(len(t["left"]) for t in c1)
    c2 = [g.tree(("grow", room1 // 2 + 1, 3, 16))] + [g.tree(s) for s in [("chain", 33), ("grow", 60, 2, 9), ("leaf",),
                                                                           ("leaf",)]]
    room2 = LDS_NODES - sum(len(t["left"]) for t in c2)
    c3 = [g.tree(("grow", room2 // 2 + 1, 3, 16))] + [g.tree(s) for s in [("leaf",), ("chain", 64), ("grow", 25, 5, 6)]]
    case = Case(c0 + c1 + c2 + c3, -3.0, recs)
    case.counts = [len(c0), len(c1), len(c2), len(c3)]
    return case


@pytest.fixture(scope="module")
def remapped(recs):
    """Two chunks on a feature map that permutes every column."""
    g = TreeGen(records_to_features(recs), 6, feature_map=FMAP_PERM)
    trees = g.fill(LDS_NODES - 2, head=[("leaf",), ("chain", 64)]) + g.fill(1501, head=[("grow", 50, 4, 8)])
    return Case(trees, 7.0, recs, feature_map=FMAP_PERM)


def _chunk_shape(m):
    tab = m.chunk_table()
    return np.diff(tab[:, 0]).tolist(), np.diff(tab[:, 1]).tolist()


def test_multichunk_forest_is_multichunk(multichunk):
    """Adequacy of the GPU cases' input (forest.hip forest_lds_kernel, `for (c ...)`): the chunk loop
    takes four trips, one chunk fills LDS to the last node, the two-walk loop (`t + 1 < t1`) and the
    single-walk tail (`if (t < t1)`) both run, and trees of depth 0 and 64 share a pair."""
    multichunk.assert_exact_sums()
    m = multichunk.model[True]
    ntree, nnode = _chunk_shape(m)
    assert ntree == multichunk.counts and len(ntree) == 4
    assert nnode[0] == LDS_NODES and max(nnode) <= LDS_NODES
    assert [c % 2 for c in ntree] == [0, 1, 1, 0]
    sizes = np.diff(np.append(m.roots, len(m.values)))
    assert sizes[:4].tolist() == [1, 129, 129, 1]
    t1, t2 = ntree[0] + ntree[1] - 1, ntree[0] + ntree[1] + ntree[2] - 1   # the unpaired tails
    assert sizes[t1] == 129 and sizes[t2] == 1


def test_synthetic_reference_matches_scalar_walk(multichunk, remapped):
    """predict_features (the reference of every GPU case below) against a row-by-row walk of the
    unpacked trees, on rows that hold every special value."""
    rows = slice(0, 48)
    for case in (multichunk, remapped):
        for le in (False, True):
            want = scalar_reference(case.trees, case.base, le, case.fmap, case.x[rows])
            assert np.array_equal(case.ref[le][rows], want)


def test_inputs_tell_wrong_kernels_apart(multichunk, remapped):
    """Each of these mistakes in a kernel changes the result of at least 10 % of the rows, so none
    of them can pass the exact comparison: ignoring the default direction of a NaN (`(inf >> 30) &
    1`), `<` for `<=` or the reverse (`a.le ? v <= thr : v < thr`), losing every chunk after the
    first (`(c == 0 ? a.base : a.out[row]) + acc`), and reading features through the identity
    instead of `a.fmap`."""
    for le in (False, True):
        m = multichunk.model[le]
        ref = multichunk.ref[le]
        flipped = ForestModel(m.values, m.info ^ np.uint32(1 << 30), m.roots, m.base_score, le, m.feature_map)
        assert changed(flipped.predict_features(multichunk.x), ref) >= 0.10
        assert changed(multichunk.ref[not le], ref) >= 0.10
        t1, n1 = m.chunk_table()[1]
        first = ForestModel(m.values[:n1], m.info[:n1], m.roots[:t1], m.base_score, le, m.feature_map)
        assert changed(first.predict_features(multichunk.x), ref) >= 0.10
        r = remapped.model[le]
        ident = ForestModel(r.values, r.info, r.roots, r.base_score, le, list(range(12)))
        assert changed(ident.predict_features(remapped.x), remapped.ref[le]) >= 0.10
        assert changed(remapped.ref[not le], remapped.ref[le]) >= 0.10


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("le", [False, True])
def test_multichunk_forest_exact(multichunk, le, lds, n):
    """forest_lds_kernel: LDS re-staging per chunk, `roots[t] - n0` rebasing, the accumulation into
    out[row] across chunks, pairs of unequal depth, the unpaired tail, a partial last tile and
    (n = 1025) a second tile; forest_kernel: the same forest through `(B + 255) / 256` blocks."""
    got = multichunk.run_gpu(le, lds, n, expect_lds=lds)
    assert got.dtype == np.float32 and np.array_equal(got, multichunk.ref[le][:n])


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("le", [False, True])
def test_remapped_features_exact(remapped, le, lds):
    """The select chain `v = (a.fmap[j] == c) ? raw[c] : v` of both kernels with a map that moves
    every column."""
    assert len(_chunk_shape(remapped.model[le])[0]) == 2
    assert np.array_equal(remapped.run_gpu(le, lds, expect_lds=lds), remapped.ref[le])


@pytest.fixture(scope="module")
def gridcase(recs):
    n = torch.cuda.get_device_properties(0).multi_processor_count * 1024 + 1029
    g = TreeGen(records_to_features(recs), 8)
    return Case([g.tree(("full", 11)) for _ in range(7)], 2.0, np.resize(recs, n))


@pytest.mark.gpu
@pytest.mark.parametrize("le", [False, True])
def test_grid_stride_rows_exact(gridcase, le):
    """forest_lds_kernel's `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)`: with more
    tiles than compute units some workgroups take a second tile for every chunk, the others do not,
    and the last tile is partial.  Seven complete depth-11 trees (three chunks): shallow and wide,
    so the reference stays cheap at this row count."""
    case = gridcase
    assert len(case.rec) % 1024 == 5 and len(case.rec) // 1024 > torch.cuda.get_device_properties(0).multi_processor_count
    assert _chunk_shape(case.model[le])[0] == [3, 3, 1]
    assert changed(case.ref[not le], case.ref[le]) >= 0.10
    for lds in (True, False):
        assert np.array_equal(case.run_gpu(le, lds, expect_lds=lds), case.ref[le])


@pytest.mark.gpu
@pytest.mark.parametrize("le", [False, True])
def test_tree_larger_than_lds_takes_global_kernel_exact(recs, le):
    """A tree of more than LDS_NODES nodes has no chunk table: ForestKernel(lds=True) must run
    forest_kernel, whose child offsets here exceed anything the LDS path ever sees."""
    g = TreeGen(records_to_features(recs), 9)
    trees = [g.tree(("leaf",)), g.tree(("grow", LDS_NODES // 2 + 1, 5, 15)), g.tree(("chain", 64)), g.tree(("full", 4))]
    case = Case(trees, 0.0, recs)
    assert len(trees[1]["left"]) == LDS_NODES + 3 and case.model[le].chunk_table() is None
    assert np.array_equal(case.run_gpu(le, True, expect_lds=False), case.ref[le])


# ---------------------------------------------------------------------------------------------
# Depth limit: both kernels stop a walk after 64 steps (`guard++ < 64`).  64 inner nodes on a path
# are walked in full; a 65th would leave the walk on an inner node, whose threshold would be added
# as if it were a leaf.  The validators refuse such a tree before any launch.
# ---------------------------------------------------------------------------------------------
def _chain_case(recs, depth):
    g = TreeGen(records_to_features(recs), 100 + depth)
    return [g.tree(("chain", depth)), g.tree(("leaf",)), g.tree(("chain", depth))]


def scalar_nodes_visited(t, le, x):
    out = []
    for row in np.asarray(x, np.float32):
        n, seen = 0, set()
        while t["left"][n] != -1:
            seen.add(n)
            v, thr = row[t["feat"][n]], t["thr"][n]
            go_left = bool(t["default_left"][n]) if np.isnan(v) else bool(v <= thr if le else v < thr)
            n = t["left"][n] if go_left else t["right"][n]
        out.append(seen)
    return out


def _steered_chain(recs, depth):
    """A chain whose path every row follows to the bottom: each on-path node splits on a one-hot
    column with a threshold that sends every value (0 or 1, never NaN) to the on-path child."""
    g = TreeGen(records_to_features(recs), 200 + depth)
    t = g.tree(("chain", depth))
    for n in np.nonzero(t["left"] != -1)[0]:
        on_left = t["left"][t["right"][n]] == -1                  # the inner child; left at the bottom
        t["feat"][n] = int(g.rng.integers(0, 8))
        t["thr"][n] = 2.0 if on_left else -1.0
    return t


def test_depth_64_is_accepted_and_scored(recs):
    x = records_to_features(recs)
    for le in (False, True):
        t = _steered_chain(recs, 64)
        trees = [t] + _chain_case(recs, 64)
        m = ForestModel._pack(trees, 1.0, le, list(range(12)))
        m.validate()                                                 # 64 inner nodes on a path: the limit, inclusive
        assert all(len(v) == 64 for v in scalar_nodes_visited(t, le, x[:64]))
        assert np.array_equal(m.predict_features(x[:64]), scalar_reference(trees, 1.0, le, list(range(12)), x[:64]))


@pytest.mark.gpu
@pytest.mark.parametrize("le", [False, True])
def test_depth_64_exact_on_gpu(recs, le):
    """`guard++ < 64` is inclusive: every row takes all 64 steps of the first tree (and of the
    paired walk's partner in the LDS kernel) and must end on the leaf, in both kernels."""
    trees = [_steered_chain(recs, 64)] + _chain_case(recs, 64)
    case = Case(trees, 1.0, recs)
    assert all(len(v) == 64 for v in scalar_nodes_visited(trees[0], le, case.x[:32]))
    for lds in (True, False):
        assert np.array_equal(case.run_gpu(le, lds, expect_lds=lds), case.ref[le])


def test_depth_65_refused_by_python_validator(recs):
    for shape in (("chain", 65), ("grow", 70, 65, 65)):
        g = TreeGen(records_to_features(recs), 3)
        m = ForestModel._pack([g.tree(("leaf",)), g.tree(shape), g.tree(("chain", 64))], 0.0, True, list(range(12)))
        with pytest.raises(ValueError, match="depth limit of 64"):
            m.validate()
        with pytest.raises(ValueError, match="depth limit of 64"):
            m.device_arrays("cpu")                                   # the gate in front of every launch


def _native_spec(m):
    return {"kind": "forest", "values": torch.from_numpy(m.values.copy()),
            "info": torch.from_numpy(m.info.view(np.int32).copy()), "roots": torch.from_numpy(m.roots.copy()),
            "base": float(m.base_score), "le": bool(m.le), "fmap": [int(j) for j in m.feature_map]}


def _native_refuses(spec, match):
    """The native front end builds its model from the spec (make_forest_model) before it opens a
    socket or touches a GPU; a refused spec is a RuntimeError."""
    from routest_amd.ops import _ext
    from routest_amd.serve.native_server import free_port
    C = _ext.native()
    h = None
    try:
        with pytest.raises(RuntimeError, match=match):
            h = C.native_server_start(free_port(), 1, [0], [spec], 1024, [], False, False, 0, [], "")
    finally:
        if h is not None:
            C.native_server_stop(h)


def test_depth_65_refused_by_native_model(recs):
    g = TreeGen(records_to_features(recs), 3)
    m = ForestModel._pack([g.tree(("leaf",)), g.tree(("chain", 65)), g.tree(("chain", 64))], 0.0, True, list(range(12)))
    _native_refuses(_native_spec(m), "depth limit of 64")
    # and the two validators agree on a child that points into the next tree
    ok = ForestModel._pack([g.tree(("chain", 2)), g.tree(("chain", 3))], 0.0, True, list(range(12)))
    ok.validate()
    ok.info[0] = (ok.info[0] & ~np.uint32(0xFFFFFF)) | np.uint32(5)  # tree 0 has 5 nodes
    with pytest.raises(ValueError, match="out of range"):
        ok.validate()
    _native_refuses(_native_spec(ok), "out of range")
