#!/usr/bin/env python3
"""Shipment trip construction (K6f, csrc/route_pd.hip) beside K6d (csrc/route_tw.hip) on the same
rows with the pairs dropped, on one GPU, and against the host C++ (``_rt.pd_trips``).

Per case (default: 10k requests of 10 stops, 1k requests of 100 stops; the instances of
bench/trip_tw_bench.py: random stops around one depot, demands 1..3, 70 % of the stops with a window
that its stop can meet alone, half with a service time; seconds = haversine metres / 30 km/h).  Half
of the stops are paired at random, pickup -> delivery; a delivery keeps its service time and loses
its window, so that every pair can be served alone.  The capacity is 12 by default (``--capacity``),
so the load profile binds and a request takes several trips.
Per step: K6d on the rows as plain stops -> K6f on the rows with their pairs, each launch timed by
its own pair of events on the same stream in the same run.  The host C++ runs ``--host-rows`` of the
rows one after the other on one thread and must give the kernel's answers.  Prints one JSON line per
case."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEED = 30 / 3.6
UNBOUNDED = 1 << 62


def _case(C, rt, torch, dev, R: int, stops: int, steps: int, warmup: int, seed: int, host_rows: int, CAP: float):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nm = stops + 1
    lat = 14.55 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lon = 121.02 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    dem = torch.randint(1, 4, (R, nm), generator=g).double()
    dem[:, 0] = 0.0
    lat, lon = lat.to(dev), lon.to(dev)
    npts = torch.full((R,), nm, dtype=torch.int32, device=dev)
    cap = torch.full((R,), CAP, dtype=torch.float64, device=dev)
    maxd = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    flag = torch.ones(R, dtype=torch.uint8, device=dev)
    D = C.route_haversine_matrix(lat, lon, npts, 1.3)
    T = (D / SPEED).contiguous()
    reach = torch.ceil(T[:, 0, :] * 1000.0).long().cpu() + 1
    horizon = int(float(T.max()) * 1000.0 * max(2.0, stops / 4.0))
    has = torch.rand(R, nm, generator=g) < 0.7
    lo = (torch.rand(R, nm, generator=g, dtype=torch.float64) * horizon).long()
    width = (torch.rand(R, nm, generator=g, dtype=torch.float64) * horizon / 3.0).long()
    op = torch.where(has, lo, torch.zeros_like(lo))
    cl = torch.where(has, torch.maximum(lo + width, reach), torch.full_like(lo, UNBOUNDED))
    sv = torch.where(torch.rand(R, nm, generator=g) < 0.5, torch.randint(0, 600_000, (R, nm), generator=g),
                     torch.zeros(R, nm, dtype=torch.long))
    # half of the stops in pairs: consecutive entries of a random order of the stops, per row
    order = torch.rand(R, stops, generator=g).argsort(1) + 1
    npairs = stops // 4
    pick, deliv = order[:, 0:2 * npairs:2], order[:, 1:2 * npairs:2]
    pf = torch.full((R, nm), -1, dtype=torch.int32)
    pf.scatter_(1, deliv, pick.int())
    op.scatter_(1, deliv, torch.zeros_like(deliv))
    cl.scatter_(1, deliv, torch.full_like(deliv, UNBOUNDED))
    dem.scatter_(1, pick, torch.zeros(R, npairs, dtype=torch.float64))
    for a in (op, sv):
        a[:, 0] = 0
    cl[:, 0] = UNBOUNDED
    op_d, cl_d, sv_d, pf_d, dem_d = op.to(dev), cl.to(dev), sv.to(dev), pf.to(dev), dem.to(dev)
    names = ("time_windows", "shipments")
    t = dict.fromkeys(names, 0.0)
    for it in range(warmup + steps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names]
        ev[0][0].record()
        tw = C.route_tw_trips(D, T, npts, dem_d, cap, maxd, op_d, cl_d, sv_d, flag)
        ev[0][1].record()
        ev[1][0].record()
        visit, trip_of, ntrips, status, arr, start, stats = C.route_pd_trips(D, T, npts, dem_d, cap, maxd, op_d, cl_d,
                                                                              sv_d, pf_d, flag)
        ev[1][1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                t[name] += ev[k][0].elapsed_time(ev[k][1])
    assert int(status.abs().sum()) == 0 and int(tw[3].abs().sum()) == 0
    ms = {k: v / steps for k, v in t.items()}
    # pairs share a trip, pickup first; how many ended up with stops between them
    pos = torch.full((R, nm), -1, dtype=torch.long)
    vis = visit.cpu().long()
    pos.scatter_(1, vis[:, :stops], torch.arange(stops).expand(R, stops))
    trip = torch.zeros((R, nm), dtype=torch.long)
    trip.scatter_(1, vis[:, :stops], trip_of.cpu().long()[:, :stops])
    pp, pd = pos.gather(1, pick), pos.gather(1, deliv)
    assert bool((pp < pd).all()) and bool((trip.gather(1, pick) == trip.gather(1, deliv)).all())
    # the host C++ on the first rows, one thread
    hr = min(R, host_rows)
    Dh, Th, demh = D[:hr].cpu().numpy(), T[:hr].cpu().numpy(), dem[:hr].numpy()
    oph, clh, svh, pfh = op[:hr].tolist(), cl[:hr].tolist(), sv[:hr].tolist(), pf[:hr].tolist()
    vh, nh = visit[:hr].cpu().numpy(), ntrips[:hr].cpu().numpy()
    t0 = time.perf_counter()
    host = [rt.pd_trips(Dh[k], Th[k], demh[k].tolist(), CAP, 9e12, oph[k], clh[k], svh[k], pfh[k]) for k in range(hr)]
    host_ms = (time.perf_counter() - t0) * 1000.0
    for k in range(hr):       # the same answers
        assert [s for tr in host[k][0] for s in tr[1:-1]] == vh[k][:stops].tolist() and len(host[k][0]) == nh[k]
    return {"metric": "shipment trips (cheapest insertion of pairs, K6f) beside K6d on the same rows without pairs",
            "requests": R, "stops": stops, "pairs_per_request": npairs, "steps": steps, "capacity": CAP,
            "time_windows_ms": ms["time_windows"], "shipments_ms": ms["shipments"],
            "shipments_over_time_windows": ms["shipments"] / ms["time_windows"],
            "host_cpp_rows": hr, "host_cpp_ms": host_ms, "host_cpp_ms_all_rows": host_ms * R / hr,
            "host_cpp_over_kernel": host_ms * R / hr / ms["shipments"],
            "insertions_per_request": float(stats[:, 0].double().mean()), "rejected": int(stats[:, 1].sum()),
            "trips_shipments": int(ntrips.sum()), "trips_time_windows": int(tw[2].sum()),
            "length_vs_time_windows": float(stats[:, 2].sum()) / float(tw[6][:, 2].sum()),
            "pairs_separated_share": float((pd > pp + 1).double().mean())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10,1000x100", help="requests x stops, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity", type=float, default=12.0,
                    help="vehicle_capacity of every request (demands are 1..3; 9e12: one long trip per request)")
    ap.add_argument("--host-rows", type=int, default=1000, help="rows the host C++ is timed on (scaled to all)")
    a = ap.parse_args()
    import torch
    from routest_amd.ops import _ext
    C = _ext.native(required=True)
    rt = _ext.runtime(required=True)
    dev = torch.device("cuda", 0)
    for k, case in enumerate(a.cases.split(",")):
        R, stops = (int(v) for v in case.lower().split("x"))
        print(json.dumps(_case(C, rt, torch, dev, R, stops, a.steps, a.warmup, k, a.host_rows, a.capacity)),
              flush=True)


if __name__ == "__main__":
    main()
