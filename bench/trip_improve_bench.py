#!/usr/bin/env python3
"""Trip improvement (K6b, csrc/route_improve.hip) beside the matrix + greedy launches of the same
batch, on one GPU.

Per case (default: 10k requests of 10 stops, 1k requests of 100 stops; random stops around one
depot, capacity unbounded so a request is one trip) and per step:
  K5 haversine matrices -> K6 greedy CVRP -> K6b on K6's outputs, every row asking,
each timed by its own pair of events on the same stream in the same run.  K6b is then launched a
second time on its own output: no move is left, so that launch is the gather plus ONE candidate
scan per trip, and the difference to the first launch is the applied moves' scans.
Quality: the saved share of the trip length in the matrix (``1 - len_after_q / len_before_q``),
mean and worst over the requests; the baseline is the greedy's own trips.
Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _case(C, torch, dev, R: int, stops: int, steps: int, warmup: int, seed: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nm = stops + 1
    lat = 14.55 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lon = 121.02 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lat, lon = lat.to(dev), lon.to(dev)
    npts = torch.full((R,), nm, dtype=torch.int32, device=dev)
    dem = torch.ones(R, nm, dtype=torch.float64, device=dev)
    cap = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    maxd = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    flag = torch.ones(R, dtype=torch.uint8, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t = {"matrix": 0.0, "greedy": 0.0, "improve": 0.0, "improve_again": 0.0}
    stats = None
    for it in range(warmup + steps):
        e = [ev() for _ in range(5)]
        e[0].record()
        D = C.route_haversine_matrix(lat, lon, npts, 1.3)
        e[1].record()
        visit, trip_of, ntrips, status = C.route_greedy_cvrp(D, npts, dem, cap, maxd)
        e[2].record()
        stats = C.route_improve_trips(D, npts, maxd, visit, trip_of, status, flag)
        e[3].record()
        again = C.route_improve_trips(D, npts, maxd, visit, trip_of, status, flag)
        e[4].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(t):
                t[name] += e[k].elapsed_time(e[k + 1])
    assert int(status.abs().sum()) == 0 and int(again[0].sum()) == 0
    moves, changed, before, after = (s.cpu().double() for s in stats)
    saved = 1.0 - after / before
    ms = {k: v / steps for k, v in t.items()}
    base = ms["matrix"] + ms["greedy"]
    return {"metric": "trip improvement (2-opt + Or-opt, K6b) beside matrix + greedy",
            "requests": R, "stops": stops, "steps": steps,
            "matrix_ms": ms["matrix"], "greedy_ms": ms["greedy"], "improve_ms": ms["improve"],
            "improve_again_ms": ms["improve_again"],
            "improve_over_matrix_plus_greedy": ms["improve"] / base,
            "improve_over_greedy": ms["improve"] / ms["greedy"],
            "moves_per_request": float(moves.mean()), "moves_per_stop": float(moves.mean()) / stops,
            "max_moves_per_stop": float(moves.max()) / stops,
            "saved_share_mean": float(saved.mean()), "saved_share_worst": float(saved.min()),
            "requests_changed_frac": float((changed > 0).double().mean())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10,1000x100", help="requests x stops, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from routest_amd.ops import _ext
    C = _ext.native(required=True)
    dev = torch.device("cuda", 0)
    for k, case in enumerate(a.cases.split(",")):
        R, stops = (int(v) for v in case.lower().split("x"))
        print(json.dumps(_case(C, torch, dev, R, stops, a.steps, a.warmup, seed=k)), flush=True)


if __name__ == "__main__":
    main()
