"""One-to-all (isochrone) benchmark of the CCH router: csrc/cch_all.hip against the existing way to
get the same numbers (S x N pair queries through ``CchGpu.route``) and, with ``--cpu``, the
multi-threaded CPU reference.  One JSON line.

Every figure is wall time around device-synchronised calls on device tensors, after one warm-up
call, over as many repeats as fill ``--min-s`` seconds.  ``--fuse`` lists the schedules to compare:
0 = one launch per depth level, n = runs of levels of at most n nodes fused into one launch.

Bytes model (from shapes, not counters), per 64-source block: label traffic 8 B x 64 x (N + kept
arcs of the pull direction) + 16 B per kept record, plus the [S][N] seconds and metres written.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from routest_amd.data.graph import synth_road_graph  # noqa: E402
from routest_amd.serve.eta_service import default_model  # noqa: E402


def timed(fn, min_s):
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        el = time.perf_counter() - t0
        if el >= min_s:
            return el / n * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--sources", default="64,256,1024")
    ap.add_argument("--fuse", default="0,16,64", help="schedules to time (the first listed after -1, the default)")
    ap.add_argument("--pairs-sources", type=int, default=4, help="sources answered by S x N pair queries")
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--cpu", action="store_true", help="also time the multi-threaded CPU reference")
    ap.add_argument("--threads", type=int, default=0)
    a = ap.parse_args()
    from routest_amd.routing.cch import RoadRouter, RouteContext
    dev = torch.device("cuda:0")
    g = synth_road_graph(a.nodes, seed=5)
    N = g.num_nodes
    router = RoadRouter(g, default_model(hidden=64, steps=50), device=dev)
    ctx = RouteContext(weather=2, congestion=1, weekhour=9)
    key = router.metric(ctx, pin=True)
    kept = int(router.last_metric["kept_b"])
    st = router.stats()
    rng = np.random.default_rng(3)
    out = {"bench": "cch_one_to_all", "nodes": N, "edges": int(g.num_edges), "arcs": int(st["arcs"]),
           "depth_levels": int(st["max_depth"]) + 1, "kept_pull_arcs": kept, "runs": []}
    for S in [int(x) for x in a.sources.split(",")]:
        src = torch.from_numpy(rng.integers(0, N, S).astype(np.int32)).to(dev)
        blocks = (S + 63) // 64
        model_bytes = blocks * (8 * 64 * (N + kept) + 16 * kept) + 8 * S * N
        for fuse in [-1] + [int(x) for x in a.fuse.split(",")]:
            ms, reps = timed(lambda: router.gpu.one_to_all(key, src, False, fuse), a.min_s)
            out["runs"].append({"sources": S, "fuse": fuse, "ms": round(ms, 3), "us_per_source": round(ms * 1e3 / S, 2),
                                "ns_per_result": round(ms * 1e6 / (S * N), 3), "reps": reps,
                                "model_bytes": model_bytes, "model_gb_s": round(model_bytes / ms / 1e6, 1)})
    # the existing path: the same answers as S x N pair queries (chain sweeps + one meet wave per pair)
    Sp = a.pairs_sources
    srcs = rng.integers(0, N, Sp).astype(np.int32)
    s_t = torch.from_numpy(np.repeat(srcs, N)).to(dev)
    d_t = torch.from_numpy(np.tile(np.arange(N, dtype=np.int32), Sp)).to(dev)
    ms, reps = timed(lambda: router.gpu.route(key, s_t, d_t, 4096, False), a.min_s)
    out["pairs"] = {"sources": Sp, "ms": round(ms, 3), "us_per_source": round(ms * 1e3 / Sp, 2),
                    "ns_per_result": round(ms * 1e6 / (Sp * N), 3), "reps": reps}
    sec_p = router.gpu.route(key, s_t, d_t, 4096, False)[0].cpu().numpy().reshape(Sp, N)
    sec_a = router.gpu.one_to_all(key, torch.from_numpy(srcs).to(dev), False, -1)[0].cpu().numpy()
    ok = np.isfinite(sec_a) & (sec_p >= 0)
    out["pairs"]["max_rel_diff_vs_one_to_all"] = float(np.max(np.abs(sec_a[ok] - sec_p[ok]) / np.maximum(sec_p[ok], 1e-6)))
    best = min((r for r in out["runs"] if r["fuse"] == -1), key=lambda r: r["ns_per_result"])
    out["speedup_per_result_vs_pairs"] = round(out["pairs"]["ns_per_result"] / best["ns_per_result"], 1)
    if a.cpu:
        from routest_amd import _rt
        threads = a.threads or int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
        c = _rt.CCH(g.indptr, g.indices, g.lat, g.lon, threads)
        mc = c.customize(router.costs(ctx), g.length_m)
        S = 64
        src = rng.integers(0, N, S).astype(np.int32)
        c.one_to_all(mc, src)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.min_s:
            c.one_to_all(mc, src)
            n += 1
        ms = (time.perf_counter() - t0) / n * 1e3
        out["cpu"] = {"threads": threads, "sources": S, "ms": round(ms, 3), "us_per_source": round(ms * 1e3 / S, 2),
                      "ns_per_result": round(ms * 1e6 / (S * N), 3), "reps": n}
    router.unpin(key)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
