"""GPS-trace map matching on the road graph: a node-based hidden-Markov matcher (Newson-Krumm)
defined entirely in integers, so this reference, the host C++ (``rtr::mm_candidates`` /
``rtr::mm_viterbi``, csrc/runtime/map_match.h, ``_rt``) and the HIP kernels (csrc/map_match.hip,
``_C.mm_candidates`` / ``_C.mm_viterbi``) agree with ``==``.

**Units.**  ``S = 11_119_500`` centimetres per degree, ``c = RoadGraph.SNAP_C``.  A coordinate
becomes ``qy = rint(lat * S)``, ``qx = rint((lon * c) * S)`` (int64), computed once on the host in
numpy float64 for graph nodes and fixes alike (:func:`quantize`); the C++ and HIP code only ever see
these integers.  ``d2(a, b) = dy*dy + dx*dx`` (cm², int64); ``isqrt`` is the exact floor root.

**Candidates** of a fix: the nodes with ``d2 <= radius_cm²``, the ``k`` smallest by the key
``(d2, node id)`` in ascending key order (``cand`` int32, -1 padded; ``cand_d2`` int64, -1 padded;
``n_cand``).  A fix without a candidate is *unmatched* and leaves the chain, which goes on from the
previous kept fix to the next kept one.

**Costs** over the kept fixes ``t``: ``emit(t, j) = beta_cm * cand_d2[t][j]``;
``g(t) = isqrt(d2(fix[t-1], fix[t]))``; ``r(t, i, j)`` is 0 for equal nodes, else the centimetres
(``llrint(float64(metres_f32) * 100)``) of the time-shortest road path between the two candidates
under the request's routing context (``RoadRouter.route``; feasible on status 0 and 4; asked as
deduplicated pair queries or, ``transitions="matrix"``, as one rectangular matrix row per step —
the same bits either way);
``trans(t, i, j) = 2 * sigma_cm² * |r - g(t)|``, infeasible without a route or with
``|r - g(t)| > max_detour_cm``.

**Viterbi.**  ``score[0][j] = emit(0, j)``; ``score[t][j] = emit(t, j) + min_i(score[t-1][i] +
trans(t, i, j))`` over live ``i`` with a feasible transition, ties to the lowest ``i``; a ``j``
without such an ``i`` is dead.  Every ``j`` dead at ``t`` is a *break*: the segment ends at ``t-1``
and a new one starts at ``t`` with ``score[t][j] = emit(t, j)`` and no back pointer.  Each segment
ends in its lowest score (ties to the lowest ``j``) and is read back along the back pointers.

**Stitching.**  Inside a segment consecutive equal nodes collapse, the remaining consecutive pairs
are routed with their paths and joined without repeating the joints: one connected node path per
segment, ``duration`` / ``distance`` the float64 sums of the legs' seconds / metres in leg order.
A leg whose listing was refused (status 4) splits the segment there.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..data.graph import RoadGraph

S_CM_PER_DEG = 11_119_500
MAX_POINTS = 2048          # fixes of one trace
MAX_K = 16
MAX_TRACES = 64            # traces of one POST /api/match
PAIR_CHUNK = 1 << 22       # pair queries of one router call
RECT_MAX_JOBS = 2 * PAIR_CHUNK   # chains of one rectangular-matrix call (what PAIR_CHUNK pairs sweep)
#: what transitions="auto" asks a GPU router for: the matrix rows measured faster than the pair
#: queries on the 1,000 x 100 workload (profiles/cch_matrix_rect.md, part c)
AUTO_TRANSITIONS_GPU = "matrix"
LEG_CHUNK = 1 << 15        # legs with node listings of one router call
MAX_SPAN_CM = 2_000_000_000   # a trace's extent per axis: keeps d2 between its fixes below 2^63
DEAD = 1 << 62             # score of a dead state (above any path score, see MatchParams)


@dataclass(frozen=True)
class MatchParams:
    """The matcher's parameters (metres; the matcher itself runs on ``rint(x * 100)`` centimetres).

    The ranges bound a path score: at most 2048 fixes, each adding ``emit <= beta_cm * radius_cm²
    <= 1e4 * 1e10`` and ``trans <= 2 * sigma_cm² * max_detour_cm <= 2 * 4e8 * 5e5``, so a score
    stays below ``2048 * (1e14 + 4e14) ~ 1.0e18 < 2^62 < 2^63``: int64 holds every sum, and
    :data:`DEAD` lies above all of them."""
    k: int = 8
    radius_m: float = 250.0
    sigma_m: float = 50.0
    beta_m: float = 30.0
    max_detour_m: float = 2000.0

    def __post_init__(self):
        if isinstance(self.k, bool) or not isinstance(self.k, (int, np.integer)) or not 1 <= self.k <= MAX_K:
            raise ValueError(f"k: an integer in 1..{MAX_K}")
        for name, hi in (("radius_m", 1000.0), ("sigma_m", 200.0), ("beta_m", 100.0), ("max_detour_m", 5000.0)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 < v <= hi:
                raise ValueError(f"{name}: a number in (0, {hi:g}]")
            if int(np.rint(float(v) * 100.0)) < 1:
                raise ValueError(f"{name}: at least one centimetre")

    @property
    def radius_cm(self) -> int:
        return int(np.rint(float(self.radius_m) * 100.0))

    @property
    def sigma_cm(self) -> int:
        return int(np.rint(float(self.sigma_m) * 100.0))

    @property
    def beta_cm(self) -> int:
        return int(np.rint(float(self.beta_m) * 100.0))

    @property
    def max_detour_cm(self) -> int:
        return int(np.rint(float(self.max_detour_m) * 100.0))


def quantize(lat, lon) -> Tuple[np.ndarray, np.ndarray]:
    """(qy, qx) int64 centimetres of coordinates in degrees (numpy float64, the one place a float
    coordinate is touched)."""
    la = np.asarray(lat, dtype=np.float64)
    lo = np.asarray(lon, dtype=np.float64)
    if not (np.isfinite(la).all() and np.isfinite(lo).all()):
        raise ValueError("coordinates must be finite")
    if la.size and (np.abs(la).max() > 90.0 or np.abs(lo).max() > 360.0):
        raise ValueError("coordinates must be degrees (|lat| <= 90, |lon| <= 360)")
    return np.rint(la * S_CM_PER_DEG).astype(np.int64), np.rint((lo * RoadGraph.SNAP_C) * S_CM_PER_DEG).astype(np.int64)


def isqrt64(x: np.ndarray) -> np.ndarray:
    """Exact floor square root of non-negative int64 values (float estimate, integer correction)."""
    x = np.asarray(x, dtype=np.int64)
    s = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    for _ in range(2):
        s = s - (s * s > x)
        s = s + ((s + 1) * (s + 1) <= x)
    return s


# ------------------------------------------------------------------------------------- references
def candidates_ref(nqy: np.ndarray, nqx: np.ndarray, py: np.ndarray, px: np.ndarray, radius_cm: int,
                   k: int, chunk: int = 256) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(cand i32 [P, k], cand_d2 i64 [P, k], n_cand i32 [P]) by a scan of all nodes per fix."""
    nqy = np.asarray(nqy, dtype=np.int64)
    nqx = np.asarray(nqx, dtype=np.int64)
    py = np.asarray(py, dtype=np.int64).reshape(-1)
    px = np.asarray(px, dtype=np.int64).reshape(-1)
    P = len(py)
    r = int(radius_cm)
    cand = np.full((P, k), -1, dtype=np.int32)
    cd2 = np.full((P, k), -1, dtype=np.int64)
    ncand = np.zeros(P, dtype=np.int32)
    for lo in range(0, P, chunk):
        dy = nqy[None, :] - py[lo:lo + chunk, None]
        dx = nqx[None, :] - px[lo:lo + chunk, None]
        near = (np.abs(dy) <= r) & (np.abs(dx) <= r)          # squares only of what cannot overflow
        dy = np.where(near, dy, 0)
        dx = np.where(near, dx, 0)
        d2 = dy * dy + dx * dx
        ok = near & (d2 <= r * r)
        for p in range(d2.shape[0]):
            ids = np.flatnonzero(ok[p])
            if not len(ids):
                continue
            order = np.lexsort((ids, d2[p, ids]))[:k]
            n = len(order)
            cand[lo + p, :n] = ids[order]
            cd2[lo + p, :n] = d2[p, ids[order]]
            ncand[lo + p] = n
    return cand, cd2, ncand


def viterbi_ref(cand_d2: np.ndarray, n_cand: np.ndarray, route_cm: np.ndarray, g: np.ndarray,
                params: MatchParams, npts: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """One trace: (choice i32 [T], segment i32 [T], n_segments, cost) from ``cand_d2`` [T, K],
    ``n_cand`` [T] (clamped to 1..K), ``route_cm`` [T-1, K, K] (-1 infeasible) and ``g`` [T-1].
    Rows from ``npts`` on are left at -1.  ``cost`` is the sum of the segments' final scores."""
    cand_d2 = np.asarray(cand_d2, dtype=np.int64)
    T, K = cand_d2.shape
    n = T if npts is None else max(0, min(int(npts), T))
    beta, two_s2, maxdet = params.beta_cm, 2 * params.sigma_cm * params.sigma_cm, params.max_detour_cm
    choice = np.full(T, -1, dtype=np.int32)
    seg = np.full(T, -1, dtype=np.int32)
    if n == 0:
        return choice, seg, 0, 0
    nc = [min(max(int(x), 1), K) for x in np.asarray(n_cand).reshape(-1)[:n]]
    back = [[-1] * K for _ in range(n)]
    ends: List[Tuple[int, int]] = []           # (last fix of the segment, its best final state)
    cost = 0

    def close(t_last: int, sc: List[int]) -> int:
        j = min(range(K), key=lambda q: (sc[q], q))
        ends.append((t_last, j))
        return sc[j]

    score = [beta * int(cand_d2[0, j]) if j < nc[0] else DEAD for j in range(K)]
    nseg = 0
    seg[0] = 0
    for t in range(1, n):
        gt = int(g[t - 1])
        rows = np.asarray(route_cm[t - 1]).tolist()
        new = [DEAD] * K
        for j in range(nc[t]):
            best, arg = DEAD, -1
            for i in range(nc[t - 1]):
                r = rows[i][j]
                if score[i] >= DEAD or r < 0:
                    continue
                dev = abs(r - gt)
                if dev > maxdet:
                    continue
                v = score[i] + two_s2 * dev
                if v < best:
                    best, arg = v, i
            if arg >= 0:
                new[j] = best + beta * int(cand_d2[t, j])
                back[t][j] = arg
        if all(v >= DEAD for v in new):        # a break
            cost += close(t - 1, score)
            nseg += 1
            new = [beta * int(cand_d2[t, j]) if j < nc[t] else DEAD for j in range(K)]
            back[t] = [-1] * K
        seg[t] = nseg
        score = new
    cost += close(n - 1, score)
    nseg += 1
    e = len(ends) - 1
    cur = ends[e][1]
    for t in range(n - 1, -1, -1):
        choice[t] = cur
        b = back[t][cur]
        if b < 0 and t > 0:
            e -= 1
            cur = ends[e][1]
        else:
            cur = b
    return choice, seg, nseg, cost


# ---------------------------------------------------------------------------------------- the grid
def grid_cell_cm(qy: np.ndarray, qx: np.ndarray) -> int:
    """Cell edge of the bucket grid: about two nodes per cell, at most 2048 cells per axis."""
    sy = int(qy.max() - qy.min()) + 1
    sx = int(qx.max() - qx.min()) + 1
    cell = int(np.sqrt(float(sy) * float(sx) / max(1.0, len(qy) / 2.0)))
    return max(100, cell, max(sy, sx) // 2048 + 1)


def build_grid(qy: np.ndarray, qx: np.ndarray) -> Dict[str, Any]:
    """Integer bucket grid over the quantized node coordinates (row-major cells, CSR ``start`` /
    ``items``), the layout csrc/map_match.hip reads."""
    qy = np.asarray(qy, dtype=np.int64)
    qx = np.asarray(qx, dtype=np.int64)
    if not len(qy):
        raise ValueError("a graph without nodes")
    cell = grid_cell_cm(qy, qx)
    y0, x0 = int(qy.min()), int(qx.min())
    cy = (qy - y0) // cell
    cx = (qx - x0) // cell
    ny, nx = int(cy.max()) + 1, int(cx.max()) + 1
    code = cy * nx + cx
    items = np.argsort(code, kind="stable").astype(np.int32)
    start = np.zeros(ny * nx + 1, dtype=np.int32)
    np.cumsum(np.bincount(code, minlength=ny * nx), out=start[1:])
    return {"y0": y0, "x0": x0, "cell": cell, "ny": ny, "nx": nx, "start": start, "items": items}


def _graph_q(g: RoadGraph) -> Tuple[np.ndarray, np.ndarray]:
    q = getattr(g, "_mm_q", None)
    if q is None:
        q = g._mm_q = quantize(g.lat, g.lon)
    return q


def _host_grid(g: RoadGraph):
    """``_rt.MmGrid`` of the graph (None without the C++ runtime)."""
    h = getattr(g, "_mm_host", None)
    if h is None:
        from ..ops import _ext
        rt = _ext.runtime(required=False)
        if rt is None or not hasattr(rt, "MmGrid"):
            return None
        nqy, nqx = _graph_q(g)
        h = g._mm_host = rt.MmGrid(nqy, nqx)
    return h


def _device_grid(g: RoadGraph, dev: torch.device) -> Dict[str, Any]:
    """The grid and the quantized node coordinates on a device, uploaded once per (graph, device)."""
    cache = getattr(g, "_mm_dev", None)
    if cache is None:
        cache = g._mm_dev = {}
    d = cache.get(str(dev))
    if d is None:
        if g.num_nodes >= 1 << 30:
            raise ValueError("map matching needs node ids below 2^30")
        nqy, nqx = _graph_q(g)
        d = build_grid(nqy, nqx)
        for name, a in (("start", d["start"]), ("items", d["items"]), ("nqy", nqy), ("nqx", nqx)):
            d[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        cache[str(dev)] = d
    return d


def find_candidates(g: RoadGraph, py: np.ndarray, px: np.ndarray, params: MatchParams, dev: torch.device):
    """(cand, cand_d2, n_cand) tensors on ``dev``: the HIP kernel on a GPU, else ``_rt``, else the
    Python reference."""
    if dev.type == "cuda":
        from ..ops import _ext
        C = _ext.native(required=True)
        d = _device_grid(g, dev)
        return tuple(C.mm_candidates(d["start"], d["items"], d["nqy"], d["nqx"], d["y0"], d["x0"], d["cell"],
                                     d["ny"], d["nx"], torch.from_numpy(py).to(dev), torch.from_numpy(px).to(dev),
                                     params.radius_cm, params.k))
    h = _host_grid(g)
    if h is not None:
        out = h.candidates(py, px, params.radius_cm, params.k)
    else:
        nqy, nqx = _graph_q(g)
        out = candidates_ref(nqy, nqx, py, px, params.radius_cm, params.k)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)


def run_viterbi(cand_d2: torch.Tensor, n_cand: torch.Tensor, route_cm: torch.Tensor, g: torch.Tensor,
                npts: torch.Tensor, params: MatchParams):
    """(choice i32 [B, T], segment i32 [B, T], n_segments i32 [B], cost i64 [B]) on the inputs'
    device: the HIP kernel on a GPU, else ``_rt``, else the Python reference."""
    if cand_d2.device.type == "cuda":
        from ..ops import _ext
        C = _ext.native(required=True)
        return tuple(C.mm_viterbi(cand_d2, n_cand, route_cm, g, npts, params.beta_cm, params.sigma_cm,
                                  params.max_detour_cm))
    from ..ops import _ext
    rt = _ext.runtime(required=False)
    if rt is not None and hasattr(rt, "mm_viterbi"):
        out = rt.mm_viterbi(cand_d2.numpy(), n_cand.numpy(), route_cm.numpy(), g.numpy(), npts.numpy(),
                            params.beta_cm, params.sigma_cm, params.max_detour_cm)
        return tuple(torch.from_numpy(np.asarray(a)) for a in out)
    return tuple(torch.from_numpy(a) for a in viterbi_batch_ref(cand_d2.numpy(), n_cand.numpy(), route_cm.numpy(),
                                                                g.numpy(), npts.numpy(), params))


def viterbi_batch_ref(cand_d2, n_cand, route_cm, g, npts, params: MatchParams):
    """:func:`viterbi_ref` over a batch [B, T, K]."""
    B, T, K = cand_d2.shape
    choice = np.full((B, T), -1, dtype=np.int32)
    seg = np.full((B, T), -1, dtype=np.int32)
    nseg = np.zeros(B, dtype=np.int32)
    cost = np.zeros(B, dtype=np.int64)
    for b in range(B):
        choice[b], seg[b], nseg[b], cost[b] = viterbi_ref(cand_d2[b], n_cand[b], route_cm[b], g[b], params,
                                                          int(npts[b]))
    return choice, seg, nseg, cost


# ------------------------------------------------------------------------------------------ driver
def _isqrt_t(x: torch.Tensor) -> torch.Tensor:
    s = torch.floor(torch.sqrt(x.double())).long()
    for _ in range(2):
        s = s - (s * s > x).long()
        s = s + ((s + 1) * (s + 1) <= x).long()
    return s


def _route_cm(router, key: int, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """Centimetres of the time-shortest road path per (src, dst) pair, -1 without a route (int64,
    on the pairs' device), asked in chunks of at most PAIR_CHUNK pairs."""
    out = []
    for lo in range(0, int(src.numel()), PAIR_CHUNK):
        s, t = src[lo:lo + PAIR_CHUNK].to(torch.int32), dst[lo:lo + PAIR_CHUNK].to(torch.int32)
        if router.gpu is not None:
            _, met, st, _, _ = router.gpu.route(key, s.contiguous(), t.contiguous(), router.max_path, False)
        else:
            _, met, st, _ = router._route(s.numpy(), t.numpy(), key, False)
            met, st = torch.from_numpy(np.ascontiguousarray(met)), torch.from_numpy(np.ascontiguousarray(st))
        cm = torch.round(met.double() * 100.0).long()
        out.append(torch.where((st == 0) | (st == 4), cm, torch.full_like(cm, -1)))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64, device=src.device)


def _as_latlon(trace) -> np.ndarray:
    a = np.asarray(trace, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError("a trace is a non-empty list of (lat, lon) fixes")
    if a.shape[0] > MAX_POINTS:
        raise ValueError(f"a trace has at most {MAX_POINTS} fixes")
    return a


def match_traces(router, g: RoadGraph, traces: Sequence[Any], ctx_or_key, params: Optional[MatchParams] = None,
                 device=None, stats: Optional[Dict[str, Any]] = None,
                 transitions: str = "auto") -> List[Dict[str, Any]]:
    """Match GPS traces (each a list of ``(lat, lon)`` fixes) to the road graph.

    ``router``: a :class:`routing.cch.RoadRouter` (its device decides where the matcher runs: HIP
    kernels next to a GPU router, ``_rt`` or the Python reference next to the CPU router; ``device``
    may only name that same device).  One dict per trace: ``matched`` (node per fix, -1 unmatched),
    ``segment`` (Viterbi segment per fix, -1 unmatched), ``matching`` (index into ``matchings`` per
    fix, -1 unmatched), ``cand_d2`` (cm² from the fix to its node, -1 unmatched), ``n_segments`` and
    ``matchings``: per stitched path ``{"segment", "nodes" (int32), "duration", "distance"}``.
    ``stats``: a dict that receives the seconds of each stage (the device is synchronized around
    them, so only pass it to measure) and the number of pair queries.

    ``transitions``: how the steps' candidate-to-candidate road metres are asked.  ``"pairs"``: the
    unique (src, dst) pairs of all steps as pair queries, two chain sweeps each.  ``"matrix"``: one
    rectangular matrix row per step (``RoadRouter.rect_rows``: previous fix's candidates x this
    fix's), 2K sweeps per step instead of up to 2K², no pair table (``pairs_queried`` then counts
    the cells asked).  ``"auto"``: :data:`AUTO_TRANSITIONS_GPU` on a GPU router, ``"pairs"`` on
    the CPU router.  All three return ``==`` results."""
    import time
    params = params or MatchParams()
    dev = router.dev
    if transitions not in ("auto", "pairs", "matrix"):
        raise ValueError("transitions: 'auto', 'pairs' or 'matrix'")
    if transitions == "auto":
        transitions = AUTO_TRANSITIONS_GPU if router.gpu is not None else "pairs"

    def lap(name: str) -> None:
        if stats is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            now = time.perf_counter()
            stats[name] = stats.get(name, 0.0) + now - lap.t0
            lap.t0 = now

    lap.t0 = time.perf_counter()
    if device is not None and torch.device(device).type != dev.type:
        raise ValueError("match_traces runs on its router's device")
    tr = [_as_latlon(t) for t in traces]
    if not tr:
        return []
    if g.num_nodes >= 1 << 30:
        raise ValueError("map matching needs node ids below 2^30")
    K = int(params.k)
    B = len(tr)
    lens = np.array([len(t) for t in tr], dtype=np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    allp = np.concatenate(tr)
    py, px = quantize(allp[:, 0], allp[:, 1])
    for b in range(B):
        if (np.ptp(py[off[b]:off[b + 1]]) > MAX_SPAN_CM) or (np.ptp(px[off[b]:off[b + 1]]) > MAX_SPAN_CM):
            raise ValueError("a trace spans more than 20,000 km")
    P = int(off[-1])
    with router.pinned(ctx_or_key) as key:
        lap("prepare_s")
        cand, cd2, ncand = find_candidates(g, py, px, params, dev)
        lap("candidates_s")
        # compact the kept fixes of every trace into [B, T] rows
        tid = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int64), lens)).to(dev)
        kept = ncand > 0
        csum = torch.cumsum(kept.long(), 0)
        before = torch.cat([csum.new_zeros(1), csum])[torch.from_numpy(off[:-1]).to(dev)]   # kept before each trace
        pos = csum - 1 - before[tid]
        npts = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, tid, kept.long())
        T = max(1, int(npts.max().item()))
        kp = kept.nonzero().flatten()
        kb, kt = tid[kp], pos[kp]
        Cn = torch.full((B, T, K), -1, dtype=torch.int32, device=dev)
        Cd = torch.zeros((B, T, K), dtype=torch.int64, device=dev)
        Nc = torch.ones((B, T), dtype=torch.int32, device=dev)
        Qy = torch.zeros((B, T), dtype=torch.int64, device=dev)
        Qx = torch.zeros((B, T), dtype=torch.int64, device=dev)
        Cn[kb, kt] = cand[kp]
        Cd[kb, kt] = cd2[kp]
        Nc[kb, kt] = ncand[kp]
        Qy[kb, kt] = torch.from_numpy(py).to(dev)[kp]
        Qx[kb, kt] = torch.from_numpy(px).to(dev)[kp]
        step = torch.arange(1, T, device=dev)[None, :] < npts[:, None]             # [B, T-1] steps that exist
        dy, dx = Qy[:, 1:] - Qy[:, :-1], Qx[:, 1:] - Qx[:, :-1]
        gg = torch.where(step, _isqrt_t(dy * dy + dx * dx), torch.zeros_like(dy))
        n_pairs = 0
        if transitions == "matrix":
            # one rectangular row per step that exists: candidates of t-1 x candidates of t
            R = torch.full((B, T - 1, K, K), -1, dtype=torch.int64, device=dev)
            rows = step.flatten().nonzero().flatten()
            if rows.numel():
                cs = Cn[:, :-1].reshape(-1, K)[rows].contiguous()
                cd = Cn[:, 1:].reshape(-1, K)[rows].contiguous()
                ns, nd = (cs >= 0).sum(1).to(torch.int32), (cd >= 0).sum(1).to(torch.int32)    # -1 pads the tail
                n_pairs = int((ns.long() * nd.long()).sum().item())
                lap("pairs_build_s")
                _, met = router.rect_rows(cs.clamp(min=0), ns, cd.clamp(min=0), nd, key, RECT_MAX_JOBS)
                lap("pair_queries_s")
                cm = torch.round(met.double() * 100.0).long()
                real = (cs >= 0)[:, :, None] & (cd >= 0)[:, None, :] & torch.isfinite(met)
                R.view(-1, K, K)[rows] = torch.where(real, cm, torch.full_like(cm, -1))
        else:
            # the unique (src, dst) pairs of all steps of all traces, self pairs dropped
            src = Cn[:, :-1, :, None].long().expand(B, T - 1, K, K)
            dst = Cn[:, 1:, None, :].long().expand(B, T - 1, K, K)
            valid = step[:, :, None, None] & (src >= 0) & (dst >= 0)
            R = torch.where(valid & (src == dst), 0, -1).to(torch.int64)
            ask = (valid & (src != dst)).nonzero(as_tuple=True)
            if ask[0].numel():
                N = int(g.num_nodes)
                uniq, inv = torch.unique(src[ask] * N + dst[ask], return_inverse=True)
                n_pairs = int(uniq.numel())
                lap("pairs_build_s")
                cm = _route_cm(router, key, uniq // N, uniq % N)
                lap("pair_queries_s")
                R[ask] = cm[inv]
        R, gg, npts32 = R.contiguous(), gg.contiguous(), npts.to(torch.int32)
        lap("pairs_build_s")
        choice, seg, nseg, _ = run_viterbi(Cd, Nc, R, gg, npts32, params)
        lap("viterbi_s")
        # back to the original fixes
        sel = choice[kb, kt].long()
        matched = torch.full((P,), -1, dtype=torch.int32, device=dev)
        segment = torch.full((P,), -1, dtype=torch.int32, device=dev)
        md2 = torch.full((P,), -1, dtype=torch.int64, device=dev)
        matched[kp] = Cn[kb, kt, sel]
        segment[kp] = seg[kb, kt]
        md2[kp] = Cd[kb, kt, sel]
        matched, segment, md2, nseg = (x.cpu().numpy() for x in (matched, segment, md2, nseg))
        out = _stitch(router, key, off, matched, segment, md2, nseg)
        lap("stitching_s")
    if stats is not None:
        stats["pairs_queried"] = stats.get("pairs_queried", 0) + n_pairs
        stats["fixes"] = stats.get("fixes", 0) + P
    return out


def _route_legs(router, key: int, ls: List[int], ld: List[int]):
    """(seconds, metres, status, node paths) of the legs, asked in chunks of LEG_CHUNK (the router
    lists into a [legs, max_path] table).  On the GPU only the table's used columns leave the device."""
    sec, met, st = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    paths: List[np.ndarray] = []
    for lo in range(0, len(ls), LEG_CHUNK):
        s, t = ls[lo:lo + LEG_CHUNK], ld[lo:lo + LEG_CHUNK]
        if router.gpu is None:
            a, m, c, p = router._route(s, t, key, True)
            p = list(p)
        else:
            dev = router.dev
            a, m, c, ln, tab = router.gpu.route(key, torch.tensor(s, dtype=torch.int32, device=dev),
                                                torch.tensor(t, dtype=torch.int32, device=dev), router.max_path, True)
            ln = torch.where(c == 0, ln, torch.zeros_like(ln))
            tab = tab[:, :max(1, int(ln.max().item()))].cpu().numpy()
            a, m, c, ln = a.cpu().numpy(), m.cpu().numpy(), c.cpu().numpy(), ln.cpu().numpy()
            p = [tab[i, :ln[i]] for i in range(len(s))]
        sec, met, st = np.concatenate([sec, a]), np.concatenate([met, m]), np.concatenate([st, c])
        paths += p
    return sec, met, st, paths


def _stitch(router, key: int, off, matched, segment, md2, nseg) -> List[Dict[str, Any]]:
    """Connected node paths of the segments (see the module docstring) from the per-fix results."""
    B = len(off) - 1
    chains: List[Tuple[int, int, np.ndarray, np.ndarray]] = []   # (trace, segment, collapsed nodes, run id per fix)
    ls: List[int] = []
    ld: List[int] = []
    for b in range(B):
        m, s = matched[off[b]:off[b + 1]], segment[off[b]:off[b + 1]]
        for q in range(int(nseg[b])):
            idx = np.flatnonzero(s == q)
            nodes = m[idx]
            first = np.ones(len(nodes), dtype=bool)
            first[1:] = nodes[1:] != nodes[:-1]
            col = nodes[first]
            chains.append((b, q, col, idx))
            ls += col[:-1].tolist()
            ld += col[1:].tolist()
    sec, met, st, paths = _route_legs(router, key, ls, ld)
    out = []
    for b in range(B):
        n = int(off[b + 1] - off[b])
        out.append({"matched": matched[off[b]:off[b + 1]].copy(), "segment": segment[off[b]:off[b + 1]].copy(),
                    "matching": np.full(n, -1, dtype=np.int32), "cand_d2": md2[off[b]:off[b + 1]].copy(),
                    "n_segments": int(nseg[b]), "matchings": []})
    leg = 0
    for b, q, col, idx in chains:
        o = out[b]
        m = o["matched"][idx]
        nodes: List[np.ndarray] = [col[:1]]
        dur = dist = 0.0
        # run[f]: which collapsed node fix f of the segment sits on; a fix belongs to the stitched
        # path that holds its node
        run = np.cumsum(np.concatenate([[0], (m[1:] != m[:-1]).astype(np.int64)]))
        start_run = 0
        for c in range(len(col) - 1):
            if st[leg] == 0:
                nodes.append(paths[leg][1:])
                dur += float(sec[leg])
                dist += float(met[leg])
            else:                                     # listing refused: the segment splits here
                o["matching"][idx[(run >= start_run) & (run <= c)]] = len(o["matchings"])
                o["matchings"].append({"segment": q, "nodes": np.concatenate(nodes).astype(np.int32),
                                       "duration": dur, "distance": dist})
                nodes, dur, dist, start_run = [col[c + 1:c + 2]], 0.0, 0.0, c + 1
            leg += 1
        o["matching"][idx[run >= start_run]] = len(o["matchings"])
        o["matchings"].append({"segment": q, "nodes": np.concatenate(nodes).astype(np.int32),
                               "duration": dur, "distance": dist})
    return out


# ---------------------------------------------------------------------------------------- endpoint
MATCH_FIELDS = (("k", "k"), ("radius", "radius_m"), ("sigma", "sigma_m"), ("beta", "beta_m"),
                ("max_detour", "max_detour_m"))


def parse_match_request(data: Any) -> Tuple[List[np.ndarray], MatchParams]:
    """(traces as (lat, lon) arrays, parameters) of a ``POST /api/match`` body; :class:`ValueError`
    (the 400's message) on anything malformed."""
    import math
    if not isinstance(data, dict):
        raise ValueError("expected a JSON object")
    if "traces" in data:
        raw = data["traces"]
        if not isinstance(raw, list) or not raw:
            raise ValueError("traces: a non-empty list of {'coordinates': [[lon, lat], ...]}")
    elif "coordinates" in data:
        raw = [data]
    else:
        raise ValueError("expected 'traces' or 'coordinates'")
    if len(raw) > MAX_TRACES:
        raise ValueError(f"traces: at most {MAX_TRACES}")
    traces = []
    for t in raw:
        co = t.get("coordinates") if isinstance(t, dict) else None
        if not isinstance(co, list) or not co:
            raise ValueError("coordinates: a non-empty list of [lon, lat]")
        if len(co) > MAX_POINTS:
            raise ValueError(f"coordinates: at most {MAX_POINTS} fixes per trace")
        for p in co:
            if not (isinstance(p, (list, tuple)) and len(p) == 2
                    and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in p)
                    and -180.0 <= p[0] <= 180.0 and -90.0 <= p[1] <= 90.0):
                raise ValueError("coordinates: every entry is [lon, lat] in degrees")
        traces.append(np.array([[float(p[1]), float(p[0])] for p in co], dtype=np.float64))
    kw = {}
    for field, name in MATCH_FIELDS:
        if field in data and data[field] is not None:
            v = data[field]
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{field}: a number")
            if field == "k":
                if int(v) != v:
                    raise ValueError("k: an integer")
                v = int(v)
            kw[name] = v
    return traces, MatchParams(**kw)


def match_response(provider, data: Any, ctx=None, device=None) -> Dict[str, Any]:
    """The endpoint's answer for a road-graph provider: OSRM-shaped ``matchings`` / ``tracepoints``
    per trace.  ``"snap": "edge"`` answers the edge-based matcher's shape
    (:func:`mapmatch_edge.edge_match_response`); absent or ``"node"`` it is this module's."""
    from .avoid import check_provider
    traces, params = parse_match_request(data)
    snap = data.get("snap", "node")
    if snap not in ("node", "edge") or not isinstance(snap, str):
        raise ValueError("snap: 'node' or 'edge'")
    g = provider.g
    check_provider(provider, ctx)
    if snap == "edge":
        from .mapmatch_edge import edge_match_response
        ans = {"code": "Ok", "traces": edge_match_response(provider, traces, params, ctx=ctx, device=device)}
        if getattr(ctx, "avoid", None) is not None:
            ans["avoid"] = ctx.avoid.summary()
        return ans
    res = provider.match(traces, ctx=ctx, params=params, device=device)

    def lonlat(n: int) -> List[float]:
        return [round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)]

    out = []
    for r in res:
        matchings = [{"nodes": [int(x) for x in m["nodes"]],
                      "geometry": {"type": "LineString", "coordinates": [lonlat(int(x)) for x in m["nodes"]]},
                      "distance": float(m["distance"]), "duration": float(m["duration"])} for m in r["matchings"]]
        dist = isqrt64(np.maximum(r["cand_d2"], 0))
        points = [None if r["matched"][i] < 0 else
                  {"location": lonlat(int(r["matched"][i])), "node": int(r["matched"][i]),
                   "matchings_index": int(r["matching"][i]), "distance": int(dist[i]) / 100.0}
                  for i in range(len(r["matched"]))]
        out.append({"matchings": matchings, "tracepoints": points})
    ans: Dict[str, Any] = {"code": "Ok", "traces": out}
    if getattr(ctx, "avoid", None) is not None:
        ans["avoid"] = ctx.avoid.summary()
    return ans
