#!/usr/bin/env python3
"""Time-window trip construction (K6d, csrc/route_tw.hip) beside the matrix and the plain greedy of
the same batch on one GPU, and against the host C++ (``_rt.tw_trips``) on the same instances.

Per case (default: 10k requests of 10 stops, 1k requests of 100 stops; random stops around one depot,
demands 1..3, unbounded capacity; 70 % of the stops with a window that its stop can meet alone, half
with a service time; seconds = haversine metres / 30 km/h) and per step:
  K5 haversine matrices -> K6 greedy CVRP (windows dropped) -> K6d,
each launch timed by its own pair of events on the same stream in the same run.  The host C++ runs
the same rows one after the other on one thread (the time includes the binding's copies).
Quality: trips and total matrix distance of K6d against the plain greedy on the same instances with
the windows dropped: the cost of the constraint, not a target.  Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEED = 30 / 3.6
UNBOUNDED = 1 << 62


def _metres(torch, D, visit, trip_of):
    """Total matrix distance of K6-shaped trips, per row."""
    R, NM = visit.shape
    v = visit.long().clamp(min=0)
    live = visit >= 0
    first = torch.ones_like(live)
    first[:, 1:] = trip_of[:, 1:] != trip_of[:, :-1]
    last = torch.ones_like(live)
    last[:, :-1] = (trip_of[:, :-1] != trip_of[:, 1:]) | ~live[:, 1:]
    prev = torch.zeros_like(v)
    prev[:, 1:] = v[:, :-1]
    prev = torch.where(first, torch.zeros_like(v), prev)
    rows = torch.arange(R, device=D.device)[:, None].expand(R, NM)
    leg = D[rows, prev, v] + torch.where(last, D[rows, v, torch.zeros_like(v)], torch.zeros_like(D[rows, prev, v]))
    return (leg * live).sum(1)


def _case(C, rt, torch, dev, R: int, stops: int, steps: int, warmup: int, seed: int, host_rows: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nm = stops + 1
    lat = 14.55 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lon = 121.02 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    dem = torch.randint(1, 4, (R, nm), generator=g).double()
    dem[:, 0] = 0.0
    lat, lon, dem = lat.to(dev), lon.to(dev), dem.to(dev)
    npts = torch.full((R,), nm, dtype=torch.int32, device=dev)
    cap = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    maxd = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    flag = torch.ones(R, dtype=torch.uint8, device=dev)
    D = C.route_haversine_matrix(lat, lon, npts, 1.3)
    T = (D / SPEED).contiguous()
    # windows: 70 % of the stops, opening somewhere in a horizon that grows with the stop count,
    # closing no earlier than the drive from the depot ends; half of the stops with a service time
    reach = torch.ceil(T[:, 0, :] * 1000.0).long().cpu() + 1
    horizon = int(float(T.max()) * 1000.0 * max(2.0, stops / 4.0))
    has = torch.rand(R, nm, generator=g) < 0.7
    lo = (torch.rand(R, nm, generator=g, dtype=torch.float64) * horizon).long()
    width = (torch.rand(R, nm, generator=g, dtype=torch.float64) * horizon / 3.0).long()
    op = torch.where(has, lo, torch.zeros_like(lo))
    cl = torch.where(has, torch.maximum(lo + width, reach), torch.full_like(lo, UNBOUNDED))
    sv = torch.where(torch.rand(R, nm, generator=g) < 0.5, torch.randint(0, 600_000, (R, nm), generator=g),
                     torch.zeros(R, nm, dtype=torch.long))
    for a in (op, sv):
        a[:, 0] = 0
    cl[:, 0] = UNBOUNDED
    op_d, cl_d, sv_d = op.to(dev), cl.to(dev), sv.to(dev)
    names = ("matrix", "greedy", "time_windows")
    t = dict.fromkeys(names, 0.0)
    for it in range(warmup + steps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names]
        ev[0][0].record()
        D = C.route_haversine_matrix(lat, lon, npts, 1.3)
        ev[0][1].record()
        ev[1][0].record()
        gv, gt, gn, gs = C.route_greedy_cvrp(D, npts, dem, cap, maxd)
        ev[1][1].record()
        ev[2][0].record()
        visit, trip_of, ntrips, status, arr, start, stats = C.route_tw_trips(D, T, npts, dem, cap, maxd, op_d, cl_d,
                                                                              sv_d, flag)
        ev[2][1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                t[name] += ev[k][0].elapsed_time(ev[k][1])
    assert int(status.abs().sum()) == 0 and int(gs.abs().sum()) == 0
    ms = {k: v / steps for k, v in t.items()}
    # the host C++ on the same rows, one thread
    hr = min(R, host_rows)
    Dh, Th, demh = D[:hr].cpu().numpy(), T[:hr].cpu().numpy(), dem[:hr].cpu().numpy()
    oph, clh, svh = op[:hr].tolist(), cl[:hr].tolist(), sv[:hr].tolist()
    vh, nh = visit[:hr].cpu().numpy(), ntrips[:hr].cpu().numpy()
    t0 = time.perf_counter()
    host = [rt.tw_trips(Dh[k], Th[k], demh[k].tolist(), 9e12, 9e12, oph[k], clh[k], svh[k]) for k in range(hr)]
    host_ms = (time.perf_counter() - t0) * 1000.0
    for k in range(hr):       # the same answers
        assert [s for trip in host[k][0] for s in trip[1:-1]] == vh[k][:stops].tolist() and len(host[k][0]) == nh[k]
    tw_m, greedy_m = _metres(torch, D, visit, trip_of), _metres(torch, D, gv, gt)
    assert abs(float(tw_m.sum()) * 1000.0 - float(stats[:, 2].sum())) < 1e-3 * float(stats[:, 2].sum())
    return {"metric": "time-window trips (cheapest insertion, K6d) beside matrix + plain greedy, and the host C++",
            "requests": R, "stops": stops, "steps": steps, "windowed_share": 0.7,
            "matrix_ms": ms["matrix"], "greedy_ms": ms["greedy"], "time_windows_ms": ms["time_windows"],
            "host_cpp_rows": hr, "host_cpp_ms": host_ms, "host_cpp_ms_all_rows": host_ms * R / hr,
            "host_cpp_over_kernel": host_ms * R / hr / ms["time_windows"],
            "insertions_per_request": float(stats[:, 0].double().mean()), "rejected": int(stats[:, 1].sum()),
            "trips_time_windows": int(ntrips.sum()), "trips_greedy_no_windows": int(gn.sum()),
            "distance_vs_greedy_no_windows": float(tw_m.sum() / greedy_m.sum()),
            "waiting_s_per_request": float(stats[:, 3].double().mean()) / 1000.0}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10,1000x100", help="requests x stops, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=10000, help="rows the host C++ is timed on (scaled to all)")
    a = ap.parse_args()
    import torch
    from routest_amd.ops import _ext
    C = _ext.native(required=True)
    rt = _ext.runtime(required=True)
    dev = torch.device("cuda", 0)
    for k, case in enumerate(a.cases.split(",")):
        R, stops = (int(v) for v in case.lower().split("x"))
        print(json.dumps(_case(C, rt, torch, dev, R, stops, a.steps, a.warmup, k, a.host_rows)), flush=True)


if __name__ == "__main__":
    main()
