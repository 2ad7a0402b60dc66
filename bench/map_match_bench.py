#!/usr/bin/env python3
"""GPS-trace map matching (K10, csrc/map_match.hip + routing/mapmatch.py): stage times on one GPU
beside the same stages of the host reference (``_rt``, CPU CCH router) on the same box, and the
matcher's accuracy on simulated traces.

Workload (default): 1,000 traces x 100 fixes on the 100k-node synthetic graph.  A trace follows the
time-shortest path between two random nodes 6-12 km apart; its fixes are equidistant along the
path's polyline, each displaced by Gaussian noise (``--noise`` metres per axis).

Stages (``match_traces(stats=...)``, the device synchronized around each): candidates, building the
unique pair list, the router's pair queries, Viterbi, stitching (path queries + host assembly).
``pair_share`` is the pair queries' share of the total.  The same traces then run on the CPU router
with ``_rt``; ``equal`` says whether both produced the same matched nodes and paths.

Accuracy (``--accuracy``; the reference alone, so it needs no GPU): the share of fixes matched to
the node of the true path nearest to the fix's true position, at noise 0 / 10 / 30 m.
Prints one JSON line per part."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_PER_DEG = 111_195.0


def make_traces(g, router, key, n_traces: int, n_fixes: int, noise_m: float, seed: int):
    """[(fixes [n_fixes, 2] as (lat, lon), true node per fix)]."""
    from routest_amd.data.graph import synth_route_queries
    rng = np.random.default_rng(seed)
    out = []
    want = n_traces
    while len(out) < n_traces:
        s, t = synth_route_queries(g, want + 16, seed=seed + len(out), min_km=6.0, max_km=12.0)
        _, _, st, paths = router.route(s, t, key)
        for i in range(len(s)):
            if st[i] != 0 or len(paths[i]) < 4 or len(out) >= n_traces:
                continue
            p = paths[i]
            la, lo = g.lat[p], g.lon[p]
            seg = np.hypot((la[1:] - la[:-1]) * M_PER_DEG, (lo[1:] - lo[:-1]) * M_PER_DEG * np.cos(np.radians(la[:-1])))
            cum = np.concatenate([[0.0], np.cumsum(seg)])
            at = np.linspace(0.0, cum[-1], n_fixes)
            k = np.clip(np.searchsorted(cum, at, side="right") - 1, 0, len(p) - 2)
            w = (at - cum[k]) / np.maximum(seg[k], 1e-9)
            tla, tlo = la[k] + w * (la[k + 1] - la[k]), lo[k] + w * (lo[k + 1] - lo[k])
            true = np.where(w <= 0.5, p[k], p[k + 1])          # the path node nearest to the true position
            fla = tla + rng.normal(0.0, 1.0, n_fixes) * noise_m / M_PER_DEG
            flo = tlo + rng.normal(0.0, 1.0, n_fixes) * noise_m / (M_PER_DEG * np.cos(np.radians(tla)))
            out.append((np.stack([fla, flo], axis=1), true))
    return out


def run(router, g, fixes, key, params, steps: int, warmup: int):
    from routest_amd.routing.mapmatch import match_traces
    res = None
    laps = []
    for it in range(warmup + steps):
        st = {}
        t0 = time.perf_counter()
        res = match_traces(router, g, fixes, key, params, stats=st)
        st["total_s"] = time.perf_counter() - t0
        if it >= warmup:
            laps.append(st)
    keys = [k for k in laps[0] if k.endswith("_s")]
    med = {k[:-2] + "_ms": round(1e3 * float(np.median([l[k] for l in laps])), 3) for k in keys}
    med["pairs_queried"] = laps[0]["pairs_queried"]
    med["pair_share"] = round(med["pair_queries_ms"] / med["total_ms"], 3)
    return res, med


def same(a, b) -> bool:
    return all(np.array_equal(x["matched"], y["matched"]) and np.array_equal(x["segment"], y["segment"])
               and len(x["matchings"]) == len(y["matchings"])
               and all(np.array_equal(m["nodes"], n["nodes"]) and m["duration"] == n["duration"]
                       and m["distance"] == n["distance"] for m, n in zip(x["matchings"], y["matchings"]))
               for x, y in zip(a, b))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--traces", type=int, default=1000)
    ap.add_argument("--fixes", type=int, default=100)
    ap.add_argument("--noise", type=float, default=10.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=float, default=250.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-steps", type=int, default=1, help="runs of the host reference (no warm-up: one takes a minute)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--no-gpu", action="store_true", help="the host reference only")
    ap.add_argument("--accuracy", action="store_true", help="also the accuracy at noise 0 / 10 / 30 m (reference)")
    ap.add_argument("--accuracy-traces", type=int, default=200)
    a = ap.parse_args()

    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.cch import RoadRouter
    from routest_amd.routing.mapmatch import MatchParams
    g = synth_road_graph(a.nodes)
    cost = (g.length_m / np.array([8.3, 12.5, 16.7, 22.2], np.float32)[g.road_class]).astype(np.float32)
    key = 1 << 40
    params = MatchParams(k=a.k, radius_m=a.radius)
    cpu = RoadRouter(g, None, device=None)
    cpu.metric_from_costs(key, cost)
    sim = make_traces(g, cpu, key, a.traces, a.fixes, a.noise, seed=1)
    fixes = [f for f, _ in sim]
    base = {"nodes": g.num_nodes, "traces": a.traces, "fixes": a.fixes, "noise_m": a.noise, "k": a.k,
            "radius_m": a.radius, "steps": a.steps}
    ref, host = run(cpu, g, fixes, key, params, a.host_steps, 0)
    print(json.dumps({"bench": "map_match", "where": "host (_rt + CPU CCH)", **base, **host}), flush=True)
    if not a.no_gpu:
        import torch
        gpu = RoadRouter(g, None, device=a.device)
        gpu.metric_from_costs(key, cost)
        got, dev = run(gpu, g, fixes, key, params, a.steps, a.warmup)
        print(json.dumps({"bench": "map_match", "where": torch.cuda.get_device_name(0), **base, **dev,
                          "equal": same(ref, got),
                          "speedup": {k: round(host[k] / dev[k], 2) for k in dev if k.endswith("_ms") and dev[k] > 0}}),
              flush=True)
    if a.accuracy:
        from routest_amd.routing.mapmatch import match_traces
        for noise in (0.0, 10.0, 30.0):
            sim = make_traces(g, cpu, key, a.accuracy_traces, a.fixes, noise, seed=2)
            res = match_traces(cpu, g, [f for f, _ in sim], key, params)
            hit = sum(int((r["matched"] == t).sum()) for r, (_, t) in zip(res, sim))
            unmatched = sum(int((r["matched"] < 0).sum()) for r in res)
            tot = sum(len(t) for _, t in sim)
            print(json.dumps({"bench": "map_match_accuracy", "noise_m": noise, "traces": len(sim), "fixes": tot,
                              "matched_to_true_node": round(hit / tot, 4), "unmatched": unmatched,
                              "one_segment": round(float(np.mean([r["n_segments"] == 1 for r in res])), 4)}), flush=True)


if __name__ == "__main__":
    main()
