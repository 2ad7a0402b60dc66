#!/usr/bin/env python3
"""Unit-relocate search on shipment trips (K6g, csrc/route_pd_improve.hip) beside the construction
it improves (K6f, csrc/route_pd.hip) on the same rows, on one GPU, and against the host C++
(``_rt.pd_improve``).

Per case (default: 10k requests of 10 stops, 1k requests of 100 stops; the instances of
bench/trip_pd_bench.py: random stops around one depot, demands 1..3, 70 % of the stops with a window
that its stop can meet alone, half with a service time; seconds = haversine metres / 30 km/h; half of
the stops paired at random, pickup -> delivery; capacity 12 by default).
Per step: K6f on the rows -> K6g on K6f's outputs, each launch timed by its own pair of events on the
same stream in the same run.  The share of the time spent in the type-1 walks cannot be told apart
from outside the kernel and is not reported.  The host C++ runs ``--host-rows`` of the rows one after the
other on one thread and must give the kernel's answers.  Prints one JSON line per case."""
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
    names = ("shipments", "improve")
    t = dict.fromkeys(names, 0.0)
    for it in range(warmup + steps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names]
        ev[0][0].record()
        out = C.route_pd_trips(D, T, npts, dem_d, cap, maxd, op_d, cl_d, sv_d, pf_d, flag)
        ev[0][1].record()
        if it == warmup + steps - 1:
            given = [c.cpu() for c in out]      # the construction's own answer, before K6g rewrites it
        ev[1][0].record()
        search = C.route_pd_improve(D, T, npts, dem_d, cap, maxd, op_d, cl_d, sv_d, pf_d, *out[:6], flag)
        ev[1][1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                t[name] += ev[k][0].elapsed_time(ev[k][1])
    visit, trip_of, ntrips, status = (c.cpu() for c in out[:4])
    assert int(status.abs().sum()) == 0
    ms = {k: v / steps for k, v in t.items()}
    st = search.cpu()
    assert bool((st[:, 5] == given[6][:, 2]).all()) and bool((st[:, 6] <= st[:, 5]).all())
    # the host C++ on the first rows, one thread, on the construction's trips
    hr = min(R, host_rows)
    Dh, Th, demh = D[:hr].cpu().numpy(), T[:hr].cpu().numpy(), dem[:hr].numpy()
    oph, clh, svh, pfh = op[:hr].tolist(), cl[:hr].tolist(), sv[:hr].tolist(), pf[:hr].tolist()
    gv, gt, gn = given[0].numpy(), given[1].numpy(), given[2].numpy()
    trips = []
    for k in range(hr):
        one = [[0] for _ in range(int(gn[k]))]
        for s, x in zip(gv[k][:stops], gt[k][:stops]):
            one[x].append(int(s))
        trips.append([tr + [0] for tr in one])
    t0 = time.perf_counter()
    host = [rt.pd_improve(Dh[k], Th[k], trips[k], demh[k].tolist(), CAP, 9e12, oph[k], clh[k], svh[k], pfh[k])
            for k in range(hr)]
    host_ms = (time.perf_counter() - t0) * 1000.0
    vh, nh = visit.numpy(), ntrips.numpy()
    for k in range(hr):       # the same answers
        assert [s for tr in host[k][0] for s in tr[1:-1]] == vh[k][:stops].tolist() and len(host[k][0]) == nh[k]
        assert [host[k][2][key] for key in ("moves", "pair_moves", "rejected")] == st[k, :3].tolist()
    return {"metric": "unit relocate on shipment trips (K6g) beside the construction (K6f) on the same rows",
            "requests": R, "stops": stops, "pairs_per_request": npairs, "steps": steps, "capacity": CAP,
            "shipments_ms": ms["shipments"], "improve_ms": ms["improve"],
            "improve_over_shipments": ms["improve"] / ms["shipments"],
            "host_cpp_rows": hr, "host_cpp_ms": host_ms, "host_cpp_ms_all_rows": host_ms * R / hr,
            "host_cpp_over_kernel": host_ms * R / hr / ms["improve"],
            "moves_per_request": float(st[:, 0].double().mean()), "pair_moves_per_request": float(st[:, 1].double().mean()),
            "rejected": int(st[:, 2].sum()), "trips_before": int(st[:, 3].sum()), "trips_after": int(st[:, 4].sum()),
            "matrix_distance_saved": 1.0 - float(st[:, 6].sum()) / float(st[:, 5].sum()),
            "improve_ms_per_move": ms["improve"] / max(1.0, float(st[:, 0].double().mean()))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10,1000x100", help="requests x stops, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity", type=float, default=12.0,
                    help="vehicle_capacity of every request (demands are 1..3; 9e12: one long trip per request)")
    ap.add_argument("--host-rows", type=int, default=200, help="rows the host C++ is timed on (scaled to all)")
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
