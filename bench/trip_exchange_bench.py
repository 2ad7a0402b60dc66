#!/usr/bin/env python3
"""Trip exchange (K6c, csrc/route_exchange.hip) beside the matrix, greedy and intra-trip launches
of the same batch, on one GPU.

Per case (default: 10k requests of 10 stops with a capacity giving about 3 trips, 1k requests of
100 stops with about 7 trips; random stops around one depot, demands 1..3) and per step:
  K5 haversine matrices -> K6 greedy CVRP -> K6b -> K6c -> K6c again -> K6b,
every row asking, each launch timed by its own pair of events on the same stream in the same run.
K5 + K6 + the first K6b are the kernels a request without ``exchange`` runs and are the baseline.
The second K6c launch runs on the first one's output: no move is left, so it is the gather plus ONE
candidate scan, and the difference to the first launch is the applied moves.
Quality: the total matrix distance and the trip count after the whole pipeline against the output
of the first K6b alone; exchange moves per stop (mean and worst request) and the rejected count.
Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _case(C, torch, dev, R: int, stops: int, trips: int, steps: int, warmup: int, seed: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nm = stops + 1
    lat = 14.55 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lon = 121.02 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    dem = torch.randint(1, 4, (R, nm), generator=g).double()
    dem[:, 0] = 0.0
    lat, lon, dem = lat.to(dev), lon.to(dev), dem.to(dev)
    npts = torch.full((R,), nm, dtype=torch.int32, device=dev)
    cap = torch.full((R,), float(-(-2 * stops // trips)), dtype=torch.float64, device=dev)
    maxd = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    flag = torch.ones(R, dtype=torch.uint8, device=dev)
    names = ("matrix", "greedy", "improve", "exchange", "exchange_again", "improve_second")
    t = dict.fromkeys(names, 0.0)
    for it in range(warmup + steps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names]
        ev[0][0].record()
        D = C.route_haversine_matrix(lat, lon, npts, 1.3)
        ev[0][1].record()
        ev[1][0].record()
        visit, trip_of, ntrips, status = C.route_greedy_cvrp(D, npts, dem, cap, maxd)
        ev[1][1].record()
        ev[2][0].record()
        s1 = C.route_improve_trips(D, npts, maxd, visit, trip_of, status, flag)
        ev[2][1].record()
        trips_k6b = ntrips.clone()
        ev[3][0].record()
        s2 = C.route_exchange_trips(D, npts, dem, cap, maxd, visit, trip_of, ntrips, status, flag)
        ev[3][1].record()
        ev[4][0].record()
        again = C.route_exchange_trips(D, npts, dem, cap, maxd, visit, trip_of, ntrips, status, flag)
        ev[4][1].record()
        ev[5][0].record()
        s3 = C.route_improve_trips(D, npts, maxd, visit, trip_of, status, flag)
        ev[5][1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                t[name] += ev[k][0].elapsed_time(ev[k][1])
    assert int(status.abs().sum()) == 0 and int(again[0].sum()) == 0
    xmoves, rejected = s2[0].cpu().double(), s2[1].cpu().double()
    len_k6b, len_final = s1[3].cpu().double(), s3[3].cpu().double()
    ms = {k: v / steps for k, v in t.items()}
    base = ms["matrix"] + ms["greedy"] + ms["improve"]
    return {"metric": "trip exchange (relocate + swap, K6c) beside matrix + greedy + intra-trip improvement",
            "requests": R, "stops": stops, "steps": steps, "capacity": float(cap[0]),
            "matrix_ms": ms["matrix"], "greedy_ms": ms["greedy"], "improve_ms": ms["improve"],
            "exchange_ms": ms["exchange"], "exchange_again_ms": ms["exchange_again"],
            "improve_second_ms": ms["improve_second"],
            "exchange_over_baseline": ms["exchange"] / base,
            "exchange_over_improve": ms["exchange"] / ms["improve"],
            "exchange_moves_per_stop": float(xmoves.mean()) / stops,
            "max_exchange_moves_per_stop": float(xmoves.max()) / stops,
            "rejected_requests": int(rejected.sum()),
            "second_improve_moves_per_request": float(s3[0].cpu().double().mean()),
            "distance_vs_improve_only": float(len_final.sum() / len_k6b.sum()),
            "distance_vs_improve_only_worst": float((len_final / len_k6b).max()),
            "trips_improve_only": int(trips_k6b.sum()), "trips_final": int(ntrips.sum())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10x3,1000x100x7",
                    help="requests x stops x trips (the capacity is sized for that many), comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from routest_amd.ops import _ext
    C = _ext.native(required=True)
    dev = torch.device("cuda", 0)
    for k, case in enumerate(a.cases.split(",")):
        R, stops, trips = (int(v) for v in case.lower().split("x"))
        print(json.dumps(_case(C, torch, dev, R, stops, trips, a.steps, a.warmup, seed=k)), flush=True)


if __name__ == "__main__":
    main()
