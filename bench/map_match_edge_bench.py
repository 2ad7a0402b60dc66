#!/usr/bin/env python3
"""Edge-based map matching (K10 edge mode, csrc/map_match_edge.hip + routing/mapmatch_edge.py): the
stage times of ``match_traces_edge`` beside the node matcher's on the same fixes, and the share of
fixes each mode leaves unmatched.

Workload (default): bench/map_match_bench.py's, 1,000 traces x 100 fixes on the 100k-node synthetic
graph, fixes equidistant along routed paths with Gaussian noise (``--noise`` metres per axis).

Stages (``stats=``, the device synchronized around each): candidates, building the matrix rows and
the route_cm tensor, the router's rectangular rows, Viterbi, stitching.  The node matcher runs with
``transitions="matrix"``, the same router calls.  ``--host`` also runs both on the CPU router with
``_rt`` (minutes at the default size) and reports whether the GPU's edge-mode answer equals it.
``--no-gpu`` runs the host part alone.  Prints one JSON line per part."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(fn, steps: int, warmup: int):
    res, laps = None, []
    for it in range(warmup + steps):
        st = {}
        t0 = time.perf_counter()
        res = fn(st)
        st["total_s"] = time.perf_counter() - t0
        if it >= warmup:
            laps.append(st)
    med = {k[:-2] + "_ms": round(1e3 * float(np.median([l[k] for l in laps])), 3) for k in laps[0] if k.endswith("_s")}
    med["pairs_queried"] = laps[0]["pairs_queried"]
    return res, med


def same_edge(a, b) -> bool:
    return all(all(np.array_equal(x[f], y[f]) for f in ("edge", "fq", "proj", "cand_d2", "segment", "matching"))
               and len(x["matchings"]) == len(y["matchings"])
               and all(np.array_equal(m["nodes"], n["nodes"]) and m["duration"] == n["duration"]
                       and m["distance"] == n["distance"] for m, n in zip(x["matchings"], y["matchings"]))
               for x, y in zip(a, b))


def both(router, g, fixes, key, params, steps, warmup):
    from routest_amd.routing.mapmatch import match_traces
    from routest_amd.routing.mapmatch_edge import match_traces_edge
    edge, edge_ms = run(lambda st: match_traces_edge(router, g, fixes, key, params, stats=st), steps, warmup)
    node, node_ms = run(lambda st: match_traces(router, g, fixes, key, params, stats=st, transitions="matrix"),
                        steps, warmup)
    tot = sum(len(f) for f in fixes)
    shares = {"unmatched_edge": round(sum(int((r["edge"] < 0).sum()) for r in edge) / tot, 4),
              "unmatched_node": round(sum(int((r["matched"] < 0).sum()) for r in node) / tot, 4),
              "one_segment_edge": round(float(np.mean([r["n_segments"] == 1 for r in edge])), 4),
              "one_segment_node": round(float(np.mean([r["n_segments"] == 1 for r in node])), 4)}
    return edge, {"edge": edge_ms, "node": node_ms, **shares}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--traces", type=int, default=1000)
    ap.add_argument("--fixes", type=int, default=100)
    ap.add_argument("--noise", type=float, default=10.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=float, nargs="+", default=[250.0], help="one run per radius (metres)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--host", action="store_true", help="also the host reference (one run, no warm-up)")
    ap.add_argument("--no-gpu", action="store_true", help="the host reference only")
    a = ap.parse_args()

    from map_match_bench import make_traces
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.routing.mapmatch import MatchParams
    g = synth_road_graph(a.nodes)
    cost = (g.length_m / np.array([8.3, 12.5, 16.7, 22.2], np.float32)[g.road_class]).astype(np.float32)
    key = 1 << 40
    cpu = RoadRouter(g, None, device=None)
    cpu.metric_from_costs(key, cost)
    fixes = [f for f, _ in make_traces(g, cpu, key, a.traces, a.fixes, a.noise, seed=1)]
    gpu = None
    if not a.no_gpu:
        import torch
        gpu = RoadRouter(g, None, device=a.device)
        gpu.metric_from_costs(key, cost)
    for radius in a.radius:
        params = MatchParams(k=a.k, radius_m=radius)
        base = {"nodes": g.num_nodes, "edges": g.num_edges, "traces": a.traces, "fixes": a.fixes, "noise_m": a.noise,
                "k": a.k, "radius_m": radius}
        ref = None
        if a.host or a.no_gpu:
            ref, host = both(cpu, g, fixes, key, params, 1, 0)
            print(json.dumps({"bench": "map_match_edge", "where": "host (_rt + CPU CCH)", **base, "steps": 1, **host}),
                  flush=True)
        if gpu is not None:
            got, dev = both(gpu, g, fixes, key, params, a.steps, a.warmup)
            extra = {} if ref is None else {"equal": same_edge(ref, got)}
            print(json.dumps({"bench": "map_match_edge", "where": torch.cuda.get_device_name(0), **base,
                              "steps": a.steps, **dev, **extra}), flush=True)


if __name__ == "__main__":
    main()
