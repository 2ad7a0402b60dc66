"""Avoid areas on the CCH router (K9e, csrc/cch_avoid.hip) on the 100k-node synthetic graph: what a
closure costs next to the customization it rides on.  One JSON line per measurement:

* ``mask``    — the mask kernel alone (``CchGpu.avoid_mask``: upload of the set, kernel, stream
  sync) for a small box (4 vertices), a city-quarter ring with a hole (256 vertices) and one ring
  at the limit (2,048 vertices); ``host_ms`` is ``_rt.avoid_mask`` (one thread) on the same set.
* ``context`` — a fresh routing context with and without an avoid set, in the same run (costs +
  customization, wall clock around ``RoadRouter.metric``), and the mask's share of it.

    python bench/cch_avoid_bench.py [--nodes 100000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(d):
    print(json.dumps(d), flush=True)


def ring(cx, cy, rx, ry, n, phase=0.0):
    t = np.linspace(0.0, 2 * np.pi, n, endpoint=False) + phase
    return [[cx + rx * np.cos(a), cy + ry * np.sin(a)] for a in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from routest_amd import _rt
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.avoid import AvoidSet, quantize
    from routest_amd.routing.cch import RoadRouter, RouteContext
    from routest_amd.serve.eta_service import default_model
    g = synth_road_graph(a.nodes, seed=0)
    router = RoadRouter(g, default_model(hidden=64, steps=50), device="cuda:0", capacity=64)
    x0, x1, y0, y1 = g.lon.min(), g.lon.max(), g.lat.min(), g.lat.max()
    cx, cy, w, h = (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0
    sets = {
        "box4": {"type": "Polygon", "coordinates": [ring(cx, cy, .02 * w, .02 * h, 4)]},
        "quarter256": {"type": "Polygon", "coordinates": [ring(cx, cy, .25 * w, .25 * h, 128),
                                                          ring(cx, cy, .15 * w, .15 * h, 128)]},
        "limit2048": {"type": "Polygon", "coordinates": [ring(cx, cy, .3 * w, .3 * h, 2048)]},
    }
    ip, ix = np.ascontiguousarray(g.indptr, np.int32), np.ascontiguousarray(g.indices, np.int32)
    qx, qy = quantize(g.lon), quantize(g.lat)
    emit({"stage": "setup", "nodes": g.num_nodes, "edges": g.num_edges, **{k: router.stats()[k] for k in ("arcs", "supernodal")}})
    mask_ms = {}
    for name, gj in sets.items():
        s = AvoidSet.from_geojson(gj)
        blob = torch.from_numpy(s.array.astype(np.int32))
        m = router.gpu.avoid_mask(blob)          # warm: the geometry's upload, the staging buffers
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m = router.gpu.avoid_mask(blob)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        hm = _rt.avoid_mask(ip, ix, qx, qy, s.array.astype(np.int32))
        host_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(m.cpu().numpy(), np.asarray(hm))
        mask_ms[name] = float(np.median(ts))
        emit({"stage": "mask", "set": name, "vertices": s.vertices, "closed_edges": int(np.asarray(hm).sum()),
              "gpu_ms_median": round(mask_ms[name], 4), "gpu_ms_min": round(min(ts), 4), "host_ms": round(host_ms, 3)})
    # fresh contexts, alternating without / with each set (distinct week-hours: nothing is cached)
    hour = 0
    for name, gj in sets.items():
        s = AvoidSet.from_geojson(gj)
        plain, avoid = [], []
        for _ in range(max(3, a.reps // 4)):
            for lst, av in ((plain, None), (avoid, s)):
                ctx = RouteContext(weather=2, congestion=1, weekhour=hour, avoid=av)
                hour += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                router.metric(ctx)
                torch.cuda.synchronize()
                lst.append((time.perf_counter() - t0) * 1e3)
                assert router.last_metric["fresh"]
        p, v = float(np.median(plain)), float(np.median(avoid))
        emit({"stage": "context", "set": name, "fresh_ms_plain": round(p, 3), "fresh_ms_avoid": round(v, 3),
              "mask_ms": round(mask_ms[name], 4), "mask_share_of_plain": round(mask_ms[name] / p, 4)})


if __name__ == "__main__":
    main()
