"""Edge-based map matching (``snap="edge"``): a fix snaps to a point along a directed road edge, not
to a graph node.  The hidden-Markov model, its parameters and the segmenting Viterbi are those of
:mod:`routing.mapmatch` (``MatchParams``, ``viterbi_ref`` / ``run_viterbi``, ``quantize``,
``isqrt64``, reused unchanged); this module defines the edge candidates, the transition centimetres
between two points on edges, and the stitching.  Every value is an integer, so this reference, the
host C++ (``rtr::mm_edge_candidates`` / ``rtr::mm_edge_route_cm``, csrc/runtime/map_match.h, ``_rt``)
and the HIP kernels (csrc/map_match_edge.hip, ``_C.mm_edge_candidates`` / ``_C.mm_edge_route_cm``)
agree with ``==``.

**Units.**  ``mapmatch.py``'s centimetres; ``FR = 16``, ``ONE = 1 << FR``; all variables int64.

**Edge.**  A directed CSR edge ``e = (u -> v)`` has ``A = (qy[u], qx[u])``, ``w = (qy[v], qx[v]) - A``,
``L2 = wy² + wx²`` and ``lc[e] = llrint(float64(length_m[e]) * 100)``.  It is *matchable* iff
``|wy| <= 2^22``, ``|wx| <= 2^22`` (41.9 km per axis) and ``0 <= lc <= 2^40``; an unmatchable edge
is never a candidate.

**Projection** of a fix ``P`` on ``e``: ``h = (P - A) . w``, ``f = clamp(h, 0, L2)``,
``fq = (f << FR) // L2`` (0 when ``L2 == 0``), ``Q = A + ((w * fq + ONE/2) >> FR)`` per axis
(arithmetic shift), ``d2 = |P - Q|²``, ``off = (lc * fq + ONE/2) >> FR``.  ``Q`` lies inside the
edge's closed bounding box: ``0 <= fq <= ONE`` and ``(w * ONE + ONE/2) >> FR == w``, so the shifted
term lies between 0 and ``w`` for either sign of ``w``.  A fix farther than the radius from that box
on one axis therefore has ``d2 > radius²``, and all three implementations reject on the box first.

**Bounds** (why int64 holds every product).  After the box test ``|P - A| <= 2^22 + radius <
2^22 + 2^17`` per axis, so ``|h| <= 2 * (2^22 + 2^17) * 2^22 < 2^46``; ``f <= L2 <= 2^45`` and
``f << FR <= 2^61 < 2^62``; ``fq <= 2^16``, ``|w * fq| <= 2^38``, ``lc * fq <= 2^56``;
``|P - Q| < 2^23`` per axis, ``d2 < 2^47`` before and ``<= radius² <= 1e10 < 2^34`` after the radius
test.  With edge ids below 2^30 the selection key ``d2 << 30 | e`` fits an unsigned 64-bit word.

**Candidates** of a fix: the matchable edges with ``d2 <= radius_cm²``, the ``k`` smallest by the
key ``(d2, edge id)``, ascending (``cand_edge`` i32, ``cand_d2`` i64, ``cand_fq`` i32, all -1
padded; ``n_cand``).  The two directions of a two-way street are separate candidates.

**Costs.**  ``emit`` and ``g(t)`` as in ``mapmatch.py``.  Between candidate ``a = (e1: u1 -> v1,
off1)`` of fix ``t-1`` and ``b = (e2: u2 -> v2, off2)`` of fix ``t`` the route centimetres are
``off2 - off1`` if ``e1 == e2`` and ``off2 >= off1``, else ``(lc[e1] - off1) + R(v1, u2) + off2``
with ``R(x, x) = 0`` and otherwise ``llrint(float64(metres_f32) * 100)`` of the time-shortest path
under the context, -1 (infeasible) without a route.  ``R`` comes from one rectangular matrix row per
step (``RoadRouter.rect_rows``: heads of ``t-1`` x tails of ``t``).  ``trans`` is still capped by
``max_detour``, so ``MatchParams``' score bound holds unchanged.

**Stitching.**  Inside a segment a same-edge forward step adds no node; every other step adds
``head(e_{t-1})`` and the leg ``head(e_{t-1}) -> tail(e_t)`` with its nodes (a leg between equal
nodes is that node), consecutive equal nodes collapse.  ``distance`` is the sum of the chosen
steps' ``r`` / 100, ``duration`` the float64 sum in step order of ``c[e] * (fq_t - fq_{t-1}) / ONE``
(same-edge forward) or ``c[e_{t-1}] * (ONE - fq_{t-1}) / ONE + leg seconds + c[e_t] * fq_t / ONE``
with ``c = float64(router.costs(key))``.  A leg whose listing was refused (status 4) splits the
matching between its two fixes.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..data.graph import RoadGraph
from .mapmatch import (MAX_SPAN_CM, RECT_MAX_JOBS, S_CM_PER_DEG, MatchParams, _as_latlon, _graph_q, _isqrt_t,
                       _route_legs, grid_cell_cm, isqrt64, quantize, run_viterbi)

FR = 16
ONE = 1 << FR
HALF = ONE >> 1
MAX_EDGE_SPAN_CM = 1 << 22      # |w| per axis of a matchable edge
MAX_EDGE_LC = 1 << 40           # centimetres of a matchable edge
MAX_GRID_AXIS = 2048


# ------------------------------------------------------------------------------------ edge records
def edge_records(nqy: np.ndarray, nqx: np.ndarray, indptr: np.ndarray, indices: np.ndarray,
                 length_m: np.ndarray) -> Dict[str, np.ndarray]:
    """Per directed CSR edge: ``tail`` / ``head`` (i32), ``ay`` / ``ax`` / ``wy`` / ``wx`` / ``lc``
    (i64) and ``ok`` (matchable).  ``w`` and ``lc`` of an unmatchable edge are stored as 0."""
    nqy = np.asarray(nqy, dtype=np.int64)
    nqx = np.asarray(nqx, dtype=np.int64)
    tail = np.repeat(np.arange(len(indptr) - 1, dtype=np.int32), np.diff(indptr))
    head = np.asarray(indices, dtype=np.int32)
    ay, ax = nqy[tail], nqx[tail]
    wy, wx = nqy[head] - ay, nqx[head] - ax
    ln = np.asarray(length_m, dtype=np.float32).astype(np.float64) * 100.0
    fin = np.isfinite(ln) & (np.abs(ln) <= float(MAX_EDGE_LC))
    lc = np.where(fin, np.rint(np.where(fin, ln, 0.0)), -1.0).astype(np.int64)
    ok = (np.abs(wy) <= MAX_EDGE_SPAN_CM) & (np.abs(wx) <= MAX_EDGE_SPAN_CM) & (lc >= 0) & (lc <= MAX_EDGE_LC)
    return {"tail": tail, "head": head, "ay": ay, "ax": ax, "wy": np.where(ok, wy, 0), "wx": np.where(ok, wx, 0),
            "lc": np.where(ok, lc, 0), "ok": ok}


def project(ay, ax, wy, wx, py, px):
    """(d2, fq, qy, qx) of fixes on edges (broadcasting int64 arrays); the caller keeps the fixes
    within the radius of the edges' boxes (the module docstring's bounds)."""
    dy, dx = py - ay, px - ax
    L2 = wy * wy + wx * wx
    f = np.clip(dy * wy + dx * wx, 0, L2)
    fq = np.where(L2 > 0, (f << FR) // np.maximum(L2, 1), 0)
    sy, sx = (wy * fq + HALF) >> FR, (wx * fq + HALF) >> FR
    return (dy - sy) ** 2 + (dx - sx) ** 2, fq, ay + sy, ax + sx


def edge_offsets(lc, fq):
    """``off``: centimetres from the tail to the projection."""
    return (np.asarray(lc, dtype=np.int64) * np.asarray(fq, dtype=np.int64) + HALF) >> FR


# -------------------------------------------------------------------------------------- references
def edge_candidates_ref(edges: Dict[str, np.ndarray], py: np.ndarray, px: np.ndarray, radius_cm: int, k: int,
                        chunk: Optional[int] = None):
    """(cand_edge i32 [P, k], cand_d2 i64 [P, k], cand_fq i32 [P, k], n_cand i32 [P]) by a scan of
    all edges per fix, in chunks of fixes."""
    py = np.asarray(py, dtype=np.int64).reshape(-1)
    px = np.asarray(px, dtype=np.int64).reshape(-1)
    P, E, r = len(py), len(edges["ok"]), int(radius_cm)
    ce = np.full((P, k), -1, dtype=np.int32)
    cd2 = np.full((P, k), -1, dtype=np.int64)
    cfq = np.full((P, k), -1, dtype=np.int32)
    ncand = np.zeros(P, dtype=np.int32)
    ay, ax, wy, wx, ok = (edges[n][None, :] for n in ("ay", "ax", "wy", "wx", "ok"))
    y0, y1 = ay + np.minimum(wy, 0), ay + np.maximum(wy, 0)
    x0, x1 = ax + np.minimum(wx, 0), ax + np.maximum(wx, 0)
    chunk = chunk or max(1, 2_000_000 // max(E, 1))
    for lo in range(0, P, chunk):
        qy, qx = py[lo:lo + chunk, None], px[lo:lo + chunk, None]
        near = ok & (qy >= y0 - r) & (qy <= y1 + r) & (qx >= x0 - r) & (qx <= x1 + r)
        # products only of what cannot overflow: a fix beyond the box sits on the tail instead
        d2, fq, _, _ = project(ay, ax, wy, wx, np.where(near, qy, ay), np.where(near, qx, ax))
        hit = near & (d2 <= r * r)
        for p in range(hit.shape[0]):
            ids = np.flatnonzero(hit[p])
            if not len(ids):
                continue
            order = ids[np.lexsort((ids, d2[p, ids]))[:k]]
            n = len(order)
            ce[lo + p, :n], cd2[lo + p, :n], cfq[lo + p, :n], ncand[lo + p] = order, d2[p, order], fq[p, order], n
    return ce, cd2, cfq, ncand


def edge_route_cm_ref(met: np.ndarray, e1: np.ndarray, off1: np.ndarray, lc1: np.ndarray, e2: np.ndarray,
                      off2: np.ndarray) -> np.ndarray:
    """``route_cm`` i64 [rows, K, K] from the matrix rows' metres (f32 [rows, K, K]: heads of the
    previous fix's candidates x tails of this fix's; inf = no route) and the candidates' ``edge``
    (i32 [rows, K], -1 padded), ``off`` and ``lc`` (i64 [rows, K])."""
    met = np.asarray(met, dtype=np.float32)
    a, b = np.asarray(e1)[:, :, None], np.asarray(e2)[:, None, :]
    o1, l1 = np.asarray(off1, dtype=np.int64)[:, :, None], np.asarray(lc1, dtype=np.int64)[:, :, None]
    o2 = np.asarray(off2, dtype=np.int64)[:, None, :]
    fin = np.isfinite(met) & (met >= 0)
    R = np.rint(np.where(fin, met, np.float32(0)).astype(np.float64) * 100.0).astype(np.int64)
    out = np.where(fin, (l1 - o1) + R + o2, -1)
    out = np.where((a == b) & (o2 >= o1), o2 - o1, out)
    return np.where((a >= 0) & (b >= 0), out, -1).astype(np.int64)


# ---------------------------------------------------------------------------------------- the grid
def edge_grid_cell(nqy: np.ndarray, nqx: np.ndarray, edges: Dict[str, np.ndarray]) -> int:
    """Cell edge of the edge grid: the larger of the node grid's cell and the 95th percentile of the
    matchable edges' spans (so that most edges touch at most 2 x 2 cells), at most 2048 cells per
    axis."""
    cell = grid_cell_cm(nqy, nqx)
    span = np.maximum(np.abs(edges["wy"]), np.abs(edges["wx"]))[edges["ok"]]
    if len(span):
        cell = max(cell, int(np.percentile(span, 95)))
    ext = max(int(nqy.max() - nqy.min()), int(nqx.max() - nqx.min())) + 1
    return max(cell, ext // MAX_GRID_AXIS + 1)


def build_edge_grid(nqy: np.ndarray, nqx: np.ndarray, edges: Dict[str, np.ndarray],
                    cell: Optional[int] = None) -> Dict[str, Any]:
    """Integer bucket grid over the matchable edges (row-major cells, CSR ``start`` / ``items``): an
    edge is listed in every cell its closed bounding box touches.  The cell doubles until
    ``len(items) <= 4 E + cells``."""
    nqy = np.asarray(nqy, dtype=np.int64)
    nqx = np.asarray(nqx, dtype=np.int64)
    if not len(nqy):
        raise ValueError("a graph without nodes")
    E = len(edges["ok"])
    ids = np.flatnonzero(edges["ok"])
    ay, ax, wy, wx = (edges[n][ids] for n in ("ay", "ax", "wy", "wx"))
    y0, x0 = int(nqy.min()), int(nqx.min())
    sy, sx = int(nqy.max()) - y0, int(nqx.max()) - x0
    fixed = cell is not None
    cell = max(int(cell) if fixed else edge_grid_cell(nqy, nqx, edges), max(sy, sx) // MAX_GRID_AXIS + 1, 1)
    while True:
        ny, nx = sy // cell + 1, sx // cell + 1
        cy0, cy1 = (ay + np.minimum(wy, 0) - y0) // cell, (ay + np.maximum(wy, 0) - y0) // cell
        cx0, cx1 = (ax + np.minimum(wx, 0) - x0) // cell, (ax + np.maximum(wx, 0) - x0) // cell
        h, w = cy1 - cy0 + 1, cx1 - cx0 + 1
        total = int((h * w).sum())
        if fixed or total <= 4 * E + ny * nx:
            break
        cell *= 2
    rep = np.repeat(np.arange(len(ids)), h * w)
    local = np.arange(total) - np.repeat(np.cumsum(h * w) - h * w, h * w)
    code = (cy0[rep] + local // w[rep]) * nx + cx0[rep] + local % w[rep]
    order = np.argsort(code, kind="stable")
    start = np.zeros(ny * nx + 1, dtype=np.int32)
    np.cumsum(np.bincount(code, minlength=ny * nx), out=start[1:])
    return {"y0": y0, "x0": x0, "cell": int(cell), "ny": int(ny), "nx": int(nx), "start": start,
            "items": ids[rep[order]].astype(np.int32)}


def pack_records(edges: Dict[str, np.ndarray]) -> np.ndarray:
    """The per-edge record the kernel reads, i64 [E, 4]: ``ay``, ``ax``, ``wy`` (low 32 bits) with
    ``wx`` (high 32 bits), ``lc``."""
    rec = np.empty((len(edges["ok"]), 4), dtype=np.int64)
    rec[:, 0], rec[:, 1], rec[:, 3] = edges["ay"], edges["ax"], edges["lc"]
    rec[:, 2] = (edges["wy"] & 0xFFFFFFFF) | (edges["wx"] << 32)
    return rec


def graph_edges(g: RoadGraph) -> Dict[str, np.ndarray]:
    e = getattr(g, "_mm_edges", None)
    if e is None:
        if g.num_edges >= 1 << 30 or g.num_nodes >= 1 << 30:
            raise ValueError("map matching needs node and edge ids below 2^30")
        nqy, nqx = _graph_q(g)
        e = g._mm_edges = edge_records(nqy, nqx, g.indptr, g.indices, g.length_m)
    return e


def _host_edge_grid(g: RoadGraph):
    """``_rt.MmEdgeGrid`` of the graph (None without the C++ runtime)."""
    h = getattr(g, "_mm_edge_host", None)
    if h is None:
        from ..ops import _ext
        rt = _ext.runtime(required=False)
        if rt is None or not hasattr(rt, "MmEdgeGrid"):
            return None
        nqy, nqx = _graph_q(g)
        e = graph_edges(g)
        h = g._mm_edge_host = rt.MmEdgeGrid(nqy, nqx, e["tail"], e["head"], np.where(e["ok"], e["lc"], -1),
                                            build_edge_grid(nqy, nqx, e)["cell"])
    return h


def _device_edge_grid(g: RoadGraph, dev: torch.device) -> Dict[str, Any]:
    """The edge grid, the edge records and the edges' tail / head / lc on a device, uploaded once per
    (graph, device)."""
    cache = getattr(g, "_mm_edge_dev", None)
    if cache is None:
        cache = g._mm_edge_dev = {}
    d = cache.get(str(dev))
    if d is None:
        nqy, nqx = _graph_q(g)
        e = graph_edges(g)
        d = build_edge_grid(nqy, nqx, e) if dev.type == "cuda" else {}
        up = [("tail", e["tail"]), ("head", e["head"]), ("lc", e["lc"])]
        if dev.type == "cuda":
            up += [("start", d["start"]), ("items", d["items"]), ("rec", pack_records(e))]
        for name, a in up:
            d[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        cache[str(dev)] = d
    return d


def find_edge_candidates(g: RoadGraph, py: np.ndarray, px: np.ndarray, params: MatchParams, dev: torch.device):
    """(cand_edge, cand_d2, cand_fq, n_cand) tensors on ``dev``: the HIP kernel on a GPU, else
    ``_rt``, else the Python reference."""
    if dev.type == "cuda":
        from ..ops import _ext
        C = _ext.native(required=True)
        d = _device_edge_grid(g, dev)
        return tuple(C.mm_edge_candidates(d["start"], d["items"], d["rec"], d["y0"], d["x0"], d["cell"], d["ny"],
                                          d["nx"], torch.from_numpy(py).to(dev), torch.from_numpy(px).to(dev),
                                          params.radius_cm, params.k))[:4]
    h = _host_edge_grid(g)
    out = (h.candidates(py, px, params.radius_cm, params.k) if h is not None
           else edge_candidates_ref(graph_edges(g), py, px, params.radius_cm, params.k))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)


def run_edge_route_cm(met: torch.Tensor, e1, off1, lc1, e2, off2) -> torch.Tensor:
    """``route_cm`` [rows, K, K] on the inputs' device: the HIP kernel on a GPU, else ``_rt``, else
    the Python reference."""
    args = [x.contiguous() for x in (met, e1, off1, lc1, e2, off2)]
    from ..ops import _ext
    if met.device.type == "cuda":
        return _ext.native(required=True).mm_edge_route_cm(*args)
    rt = _ext.runtime(required=False)
    fn = rt.mm_edge_route_cm if rt is not None and hasattr(rt, "mm_edge_route_cm") else edge_route_cm_ref
    return torch.from_numpy(np.ascontiguousarray(fn(*(a.numpy() for a in args))))


# ------------------------------------------------------------------------------------------ driver
def match_traces_edge(router, g: RoadGraph, traces: Sequence[Any], ctx_or_key, params: Optional[MatchParams] = None,
                      stats: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
    """Match GPS traces (each a list of ``(lat, lon)`` fixes) to points along road edges.

    Runs on the router's device, as :func:`mapmatch.match_traces` does.  One dict per trace:
    ``edge`` (i32 per fix, -1 unmatched), ``fq`` (i32, the projection's fraction of the edge in
    1/65536, -1 unmatched), ``proj`` (i64 [n, 2], the projection ``Q`` as quantized (qy, qx); zeros
    for an unmatched fix), ``cand_d2`` (cm² from the fix to ``Q``, -1 unmatched), ``segment``,
    ``matching`` (index into ``matchings``, -1 unmatched), ``n_segments`` and ``matchings``: per
    stitched path ``{"segment", "nodes" (i32, the graph nodes passed), "duration", "distance",
    "start", "end"}`` with ``start`` / ``end`` the projections (qy, qx) it runs between.
    ``stats`` receives the stages' seconds as in ``match_traces``."""
    import time
    params = params or MatchParams()
    dev = router.dev

    def lap(name: str) -> None:
        if stats is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            now = time.perf_counter()
            stats[name] = stats.get(name, 0.0) + now - lap.t0
            lap.t0 = now

    lap.t0 = time.perf_counter()
    tr = [_as_latlon(t) for t in traces]
    if not tr:
        return []
    edges = graph_edges(g)
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
    n_pairs = 0
    with router.pinned(ctx_or_key) as key:
        lap("prepare_s")
        cand, cd2, cfq, ncand = find_edge_candidates(g, py, px, params, dev)
        lap("candidates_s")
        ed = _device_edge_grid(g, dev)
        # compact the kept fixes of every trace into [B, T] rows
        tid = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int64), lens)).to(dev)
        kept = ncand > 0
        csum = torch.cumsum(kept.long(), 0)
        before = torch.cat([csum.new_zeros(1), csum])[torch.from_numpy(off[:-1]).to(dev)]
        pos = csum - 1 - before[tid]
        npts = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, tid, kept.long())
        T = max(1, int(npts.max().item()))
        kp = kept.nonzero().flatten()
        kb, kt = tid[kp], pos[kp]
        Ce = torch.full((B, T, K), -1, dtype=torch.int32, device=dev)
        Cd = torch.zeros((B, T, K), dtype=torch.int64, device=dev)
        Cf = torch.zeros((B, T, K), dtype=torch.int64, device=dev)
        Nc = torch.ones((B, T), dtype=torch.int32, device=dev)
        Qy = torch.zeros((B, T), dtype=torch.int64, device=dev)
        Qx = torch.zeros((B, T), dtype=torch.int64, device=dev)
        Ce[kb, kt] = cand[kp]
        Cd[kb, kt] = cd2[kp]
        Cf[kb, kt] = cfq[kp].long()
        Nc[kb, kt] = ncand[kp]
        Qy[kb, kt] = torch.from_numpy(py).to(dev)[kp]
        Qx[kb, kt] = torch.from_numpy(px).to(dev)[kp]
        real = Ce >= 0
        el = Ce.clamp(min=0).long()
        Cl = torch.where(real, ed["lc"][el], torch.zeros_like(Cf))
        Co = torch.where(real, (Cl * Cf + HALF) >> FR, torch.zeros_like(Cf))
        Hd, Tl = ed["head"][el], ed["tail"][el]                     # valid node ids in the padding too
        step = torch.arange(1, T, device=dev)[None, :] < npts[:, None]             # [B, T-1] steps that exist
        dy, dx = Qy[:, 1:] - Qy[:, :-1], Qx[:, 1:] - Qx[:, :-1]
        gg = torch.where(step, _isqrt_t(dy * dy + dx * dx), torch.zeros_like(dy))
        # one rectangular row per step that exists: heads of t-1's candidates x tails of t's
        R = torch.full((B, T - 1, K, K), -1, dtype=torch.int64, device=dev)
        rows = step.flatten().nonzero().flatten()
        if rows.numel():
            def prev(x):
                return x[:, :-1].reshape(-1, K)[rows].contiguous()

            def cur(x):
                return x[:, 1:].reshape(-1, K)[rows].contiguous()
            e1, e2 = prev(Ce), cur(Ce)
            ns, nd = (e1 >= 0).sum(1).to(torch.int32), (e2 >= 0).sum(1).to(torch.int32)      # -1 pads the tail
            n_pairs = int((ns.long() * nd.long()).sum().item())
            lap("pairs_build_s")
            _, met = router.rect_rows(prev(Hd), ns, cur(Tl), nd, key, RECT_MAX_JOBS)
            lap("pair_queries_s")
            R.view(-1, K, K)[rows] = run_edge_route_cm(met, e1, prev(Co), prev(Cl), e2, cur(Co))
        R, gg, npts32 = R.contiguous(), gg.contiguous(), npts.to(torch.int32)
        lap("pairs_build_s")
        choice, seg, nseg, _ = run_viterbi(Cd, Nc, R, gg, npts32, params)
        lap("viterbi_s")
        # back to the original fixes
        sel = choice[kb, kt].long()
        fields = {n: torch.full((P,), -1, dtype=torch.int64, device=dev) for n in ("edge", "fq", "d2", "off", "seg", "r")}
        fields["edge"][kp] = Ce[kb, kt, sel].long()
        fields["fq"][kp] = Cf[kb, kt, sel]
        fields["d2"][kp] = Cd[kb, kt, sel]
        fields["off"][kp] = Co[kb, kt, sel]
        fields["seg"][kp] = seg[kb, kt].long()
        if T > 1:
            # the Viterbi's own centimetres of the step into each fix that continues its segment
            tp = (kt - 1).clamp(min=0)
            cont = (kt > 0) & (seg[kb, tp] == seg[kb, kt])
            fields["r"][kp] = torch.where(cont, R[kb, tp, choice[kb, tp].long(), sel], torch.full_like(sel, -1))
        host = {n: v.cpu().numpy() for n, v in fields.items()}
        out = _stitch_edges(router, key, edges, off, py, px, host, nseg.cpu().numpy())
        lap("stitching_s")
    if stats is not None:
        stats["pairs_queried"] = stats.get("pairs_queried", 0) + n_pairs
        stats["fixes"] = stats.get("fixes", 0) + P
    return out


def _stitch_edges(router, key: int, edges, off, py, px, host, nseg) -> List[Dict[str, Any]]:
    """Node paths, durations and distances of the segments (see the module docstring)."""
    B = len(off) - 1
    edge, fq, offc, seg, rstep = host["edge"], host["fq"], host["off"], host["seg"], host["r"]
    tail, head = edges["tail"], edges["head"]
    on = edge >= 0
    ei = np.where(on, edge, 0)
    _, _, qy, qx = project(edges["ay"][ei], edges["ax"][ei], edges["wy"][ei], edges["wx"][ei],
                           np.where(on, py, edges["ay"][ei]), np.where(on, px, edges["ax"][ei]))
    proj = np.where(on[:, None], np.stack([qy, qx], axis=1), 0).astype(np.int64)
    cost = np.asarray(router.costs(key), dtype=np.float64)
    # the steps of every segment; a step that leaves its edge (or goes back on it) asks for a leg
    steps: List[Tuple[int, int, int, int]] = []          # (trace, segment, fix before, fix) as global fix ids
    ls: List[int] = []
    ld: List[int] = []
    for b in range(B):
        idx = off[b] + np.flatnonzero(on[off[b]:off[b + 1]])
        for a, c in zip(idx[:-1], idx[1:]):
            if seg[a] != seg[c]:
                continue
            steps.append((b, int(seg[c]), int(a), int(c)))
            if not (edge[a] == edge[c] and offc[c] >= offc[a]) and head[edge[a]] != tail[edge[c]]:
                ls.append(int(head[edge[a]]))
                ld.append(int(tail[edge[c]]))
    sec, _, st, paths = _route_legs(router, key, ls, ld)
    out = []
    for b in range(B):
        s = slice(off[b], off[b + 1])
        out.append({"edge": edge[s].astype(np.int32), "fq": fq[s].astype(np.int32), "proj": proj[s].copy(),
                    "cand_d2": host["d2"][s].copy(), "segment": seg[s].astype(np.int32),
                    "matching": np.full(int(off[b + 1] - off[b]), -1, dtype=np.int32), "n_segments": int(nseg[b]),
                    "matchings": []})
    state: Dict[str, Any] = {}

    def open_at(b: int, q: int, f: int) -> None:
        state.update(b=b, q=q, first=f, last=f, nodes=[], dur=0.0, cm=0)
        out[b]["matching"][f - off[b]] = len(out[b]["matchings"])

    def close() -> None:
        if not state:
            return
        n = np.asarray(state["nodes"], dtype=np.int32)
        if len(n) > 1:
            n = n[np.concatenate([[True], n[1:] != n[:-1]])]
        out[state["b"]]["matchings"].append({"segment": state["q"], "nodes": n, "duration": state["dur"],
                                             "distance": state["cm"] / 100.0, "start": proj[state["first"]].copy(),
                                             "end": proj[state["last"]].copy()})
        state.clear()

    leg = 0
    at = 0
    for b in range(B):
        idx = off[b] + np.flatnonzero(on[off[b]:off[b + 1]])
        for f in idx:
            f = int(f)
            if not state or state["b"] != b or state["q"] != seg[f]:
                close()
                open_at(b, int(seg[f]), f)         # the first fix of a segment
                continue
            _, _, a, c = steps[at]
            at += 1
            assert c == f and a == state["last"]
            e1, e2 = int(edge[a]), int(edge[c])
            if e1 == e2 and offc[c] >= offc[a]:
                state["dur"] += cost[e1] * float(fq[c] - fq[a]) / ONE
            else:
                u, v = int(head[e1]), int(tail[e2])
                if u == v:
                    leg_sec, path = 0.0, [u]
                else:
                    ok, leg_sec, path = st[leg] == 0, float(sec[leg]), paths[leg]
                    leg += 1
                    if not ok:                       # listing refused: the matching splits between the two fixes
                        close()
                        open_at(b, int(seg[f]), f)
                        continue
                state["nodes"].append(u)
                state["nodes"].extend(int(x) for x in path)
                state["dur"] += cost[e1] * float(ONE - fq[a]) / ONE + leg_sec + cost[e2] * float(fq[c]) / ONE
            state["cm"] += int(rstep[c])
            state["last"] = f
            out[b]["matching"][f - off[b]] = len(out[b]["matchings"])
    close()
    return out


def node_path(g: RoadGraph, r: Dict[str, Any], index: int = 0) -> np.ndarray:
    """The graph-node path that covers matching ``index`` of one trace's result: the tail of its
    first edge, the nodes passed and the head of its last edge, consecutive duplicates collapsed."""
    e = graph_edges(g)
    fixes = np.flatnonzero(r["matching"] == index)
    n = np.concatenate([[e["tail"][r["edge"][fixes[0]]]], r["matchings"][index]["nodes"],
                        [e["head"][r["edge"][fixes[-1]]]]])
    return n[np.concatenate([[True], n[1:] != n[:-1]])].astype(np.int32)


# ---------------------------------------------------------------------------------------- endpoint
def dequantize(qy, qx) -> Tuple[np.ndarray, np.ndarray]:
    """(lat, lon) degrees of quantized centimetres."""
    return (np.asarray(qy, dtype=np.float64) / S_CM_PER_DEG,
            np.asarray(qx, dtype=np.float64) / S_CM_PER_DEG / RoadGraph.SNAP_C)


def edge_match_response(provider, traces, params: MatchParams, ctx=None, device=None) -> List[Dict[str, Any]]:
    """The ``traces`` of ``POST /api/match`` with ``"snap": "edge"``: per tracepoint the projected
    ``location``, its ``edge`` (``from`` / ``to`` nodes, ``offset`` and ``length`` in metres), the
    ``matchings_index`` and the ``distance`` to the fix; per matching the nodes passed and a
    ``geometry`` from the first projection over the nodes to the last one."""
    g = provider.g
    e = graph_edges(g)
    res = provider.match(traces, ctx=ctx, params=params, device=device, snap="edge")

    def lonlat_q(q) -> List[float]:
        la, lo = dequantize(q[0], q[1])
        return [round(float(lo), 6), round(float(la), 6)]

    out = []
    for r in res:
        matchings = []
        for m in r["matchings"]:
            line = [lonlat_q(m["start"])] + [[round(float(g.lon[n]), 6), round(float(g.lat[n]), 6)] for n in m["nodes"]] \
                + [lonlat_q(m["end"])]
            line = [p for i, p in enumerate(line) if i == 0 or p != line[i - 1]]
            matchings.append({"nodes": [int(x) for x in m["nodes"]],
                              "geometry": {"type": "LineString", "coordinates": line},
                              "distance": float(m["distance"]), "duration": float(m["duration"])})
        dist = isqrt64(np.maximum(r["cand_d2"], 0))
        offs = edge_offsets(e["lc"][np.maximum(r["edge"], 0)], np.maximum(r["fq"], 0))
        points = [None if r["edge"][i] < 0 else
                  {"location": lonlat_q(r["proj"][i]),
                   "edge": {"from": int(e["tail"][r["edge"][i]]), "to": int(e["head"][r["edge"][i]]),
                            "offset": int(offs[i]) / 100.0, "length": int(e["lc"][r["edge"][i]]) / 100.0},
                   "matchings_index": int(r["matching"][i]), "distance": int(dist[i]) / 100.0}
                  for i in range(len(r["edge"]))]
        out.append({"matchings": matchings, "tracepoints": points})
    return out
