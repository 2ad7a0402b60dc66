#!/usr/bin/env python3
"""Rectangular CCH matrices (csrc/cch_query.hip matrix_rect / meet_rect_kernel) on the 100k-node
synthetic graph.  Every figure is the median and the range (min .. max) of ``--reps`` interleaved
repetitions after a warm-up; device times are hipEvent times around the binding call.

(a) ``matrix_rect`` against the square ``matrix`` of the union of the two lists, for 10 x 5,000,
    100 x 100 and 2,048 x 2,048 (disjoint random nodes).
(b) the meet alone: ``meet_rect_kernel`` (MEET_RECT) against ``meet_kernel`` fed with pair job
    indices (MEET_PAIRS) on the same swept chains, each as the call's time minus the time of the
    same call without a meet (MEET_NONE: jobs + sweeps), at 10 x 5,000 and at 1,000 rows of 8 x 8.
(c) map matching (bench/map_match_bench.py's workload, 1,000 traces x 100 fixes) with
    ``transitions="pairs"`` and ``"matrix"`` in one process, interleaved.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEET_RECT, MEET_PAIRS, MEET_NONE = 1, 2, 3


def stat(xs):
    return {"median_ms": round(float(np.median(xs)), 3), "min_ms": round(float(np.min(xs)), 3),
            "max_ms": round(float(np.max(xs)), 3)}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def interleaved(fns, reps, warmup=1):
    """{name: [ms per rep]} with the variants taking turns inside every repetition."""
    ms = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, fn in fns.items():
            t, _ = timed(fn)
            if it >= warmup:
                ms[k].append(t)
    return ms


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--traces", type=int, default=1000)
    ap.add_argument("--fixes", type=int, default=100)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--skip", default="", help="comma-separated parts to skip (a, b, c)")
    a = ap.parse_args()
    skip = set(a.skip.split(","))

    import torch
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.cch import RoadRouter
    g = synth_road_graph(a.nodes)
    cost = (g.length_m / np.array([8.3, 12.5, 16.7, 22.2], np.float32)[g.road_class]).astype(np.float32)
    key = 1 << 40
    dev = torch.device(a.device)
    gpu = RoadRouter(g, None, device=dev)
    gpu.metric_from_costs(key, cost)
    base = {"nodes": g.num_nodes, "reps": a.reps, "max_depth": gpu.stats()["max_depth"],
            "device": torch.cuda.get_device_name(dev)}
    rng = np.random.default_rng(0)

    def t32(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)

    def rect_args(S, D, R=1):
        nodes = np.stack([rng.choice(g.num_nodes, S + D, replace=False) for _ in range(R)])
        return nodes, (t32(nodes[:, :S]), t32(np.full(R, S)), t32(nodes[:, S:]), t32(np.full(R, D)))

    if "a" not in skip:
        for S, D in ((10, 5000), (100, 100), (2048, 2048)):
            nodes, args = rect_args(S, D)
            pts, npts = t32(nodes), t32([S + D])
            sq = gpu.gpu.matrix(key, pts, npts)
            re = gpu.gpu.matrix_rect(key, *args)
            equal = all(torch.equal(x[0, :S, S:], y[0]) for x, y in zip(sq, re))
            del sq, re
            ms = interleaved({"square": lambda: gpu.gpu.matrix(key, pts, npts),
                              "rect": lambda: gpu.gpu.matrix_rect(key, *args)}, a.reps)
            print(json.dumps({"bench": "cch_matrix_rect", "part": "a", "S": S, "D": D, **base, "equal": equal,
                              "square": stat(ms["square"]), "rect": stat(ms["rect"]),
                              "speedup": round(float(np.median(ms["square"]) / np.median(ms["rect"])), 2)}), flush=True)

    if "b" not in skip:
        for S, D, R in ((10, 5000, 1), (8, 8, 1000)):
            _, args = rect_args(S, D, R)
            one = gpu.gpu.matrix_rect(key, *args, MEET_RECT)
            two = gpu.gpu.matrix_rect(key, *args, MEET_PAIRS)
            equal = all(torch.equal(x, y) for x, y in zip(one, two))
            del one, two
            ms = interleaved({m: (lambda m=m: gpu.gpu.matrix_rect(key, *args, m))
                              for m in (MEET_NONE, MEET_RECT, MEET_PAIRS)}, a.reps)
            none = np.array(ms[MEET_NONE])
            rect, pairs = np.array(ms[MEET_RECT]) - none, np.array(ms[MEET_PAIRS]) - none
            print(json.dumps({"bench": "cch_matrix_rect", "part": "b", "S": S, "D": D, "rows": R, **base, "equal": equal,
                              "sweeps_only": stat(none), "call_meet_rect": stat(ms[MEET_RECT]),
                              "call_meet_pairs": stat(ms[MEET_PAIRS]), "meet_rect": stat(rect), "meet_pairs": stat(pairs),
                              "meet_speedup": round(float(np.median(pairs) / np.median(rect)), 2)}), flush=True)

    if "c" not in skip:
        from map_match_bench import make_traces, same
        from routest_amd.routing.mapmatch import MatchParams, match_traces
        cpu = RoadRouter(g, None, device=None)
        cpu.metric_from_costs(key, cost)
        fixes = [f for f, _ in make_traces(g, cpu, key, a.traces, a.fixes, 10.0, seed=1)]
        params = MatchParams(k=8, radius_m=250.0)
        laps = {"pairs": [], "matrix": []}
        res = {}
        for it in range(1 + a.reps):
            for tr in ("pairs", "matrix"):
                st = {}
                t0 = time.perf_counter()
                res[tr] = match_traces(gpu, g, fixes, key, params, stats=st, transitions=tr)
                st["total_s"] = time.perf_counter() - t0
                if it >= 1:
                    laps[tr].append(st)
        out = {"bench": "cch_matrix_rect", "part": "c", "traces": a.traces, "fixes": a.fixes, "k": 8, **base,
               "equal": same(res["pairs"], res["matrix"])}
        for tr, ls in laps.items():
            out[tr] = {k[:-2]: stat([1e3 * l[k] for l in ls]) for k in ls[0] if k.endswith("_s")}
            out[tr]["pairs_queried"] = ls[0]["pairs_queried"]
        tp = [1e3 * l["total_s"] for l in laps["pairs"]]
        tm = [1e3 * l["total_s"] for l in laps["matrix"]]
        out["pairs_range_ms"] = round(max(tp) - min(tp), 3)
        out["matrix_faster_by_more_than_pairs_range"] = bool(np.median(tp) - np.median(tm) > max(tp) - min(tp))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
