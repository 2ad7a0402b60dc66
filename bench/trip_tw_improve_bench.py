#!/usr/bin/env python3
"""Window-aware local search on time-window trips (K6e, csrc/route_tw_improve.hip) beside the
cheapest insertion (K6d) of the same batch on one GPU, and against the host C++
(``_rt.tw_improve``) on the same rows.

Per case (default: 10k requests of 10 stops, 1k requests of 100 stops; the instances of
bench/trip_tw_bench.py: random stops around one depot, demands 1..3, unbounded capacity, 70 % of the
stops with a window that its stop can meet alone, half with a service time, seconds = haversine
metres / 30 km/h) and per step: K6d -> K6e on K6d's outputs, each launch timed by its own pair of
events on the same stream in the same run.  The host C++ runs the search on the first rows one after
the other on one thread (the time includes the binding's copies) and must give the kernel's answer.
Quality: matrix distance and trips before and after the search.  Prints one JSON line per case."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEED = 30 / 3.6
UNBOUNDED = 1 << 62


def _instances(C, torch, dev, R: int, stops: int, seed: int):
    """The batch of bench/trip_tw_bench.py for this seed."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    nm = stops + 1
    lat = 14.55 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    lon = 121.02 + 0.08 * (torch.rand(R, nm, generator=g, dtype=torch.float64) - 0.5)
    dem = torch.randint(1, 4, (R, nm), generator=g).double()
    dem[:, 0] = 0.0
    lat, lon, dem = lat.to(dev), lon.to(dev), dem.to(dev)
    npts = torch.full((R,), nm, dtype=torch.int32, device=dev)
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
    for a in (op, sv):
        a[:, 0] = 0
    cl[:, 0] = UNBOUNDED
    return D, T, npts, dem, op, cl, sv


def _trips(visit, trip_of, ntrips):
    trips = [[0] for _ in range(int(ntrips))]
    for v, t in zip(visit, trip_of):
        if v < 0:
            break
        trips[t].append(int(v))
    return [t + [0] for t in trips]


def _case(C, rt, torch, dev, R: int, stops: int, steps: int, warmup: int, seed: int, host_rows: int):
    D, T, npts, dem, op, cl, sv = _instances(C, torch, dev, R, stops, seed)
    cap = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    maxd = torch.full((R,), 9e12, dtype=torch.float64, device=dev)
    flag = torch.ones(R, dtype=torch.uint8, device=dev)
    op_d, cl_d, sv_d = op.to(dev), cl.to(dev), sv.to(dev)
    args = (D, T, npts, dem, cap, maxd, op_d, cl_d, sv_d)
    names = ("time_windows", "tw_improve")
    t = dict.fromkeys(names, 0.0)
    for it in range(warmup + steps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names]
        ev[0][0].record()
        out = C.route_tw_trips(*args, flag)
        ev[0][1].record()
        built = [c.clone() for c in out[:3]]          # (outside both event pairs)
        ev[1][0].record()
        search = C.route_tw_improve(*args, *out[:6], flag)
        ev[1][1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                t[name] += ev[k][0].elapsed_time(ev[k][1])
    visit, trip_of, ntrips, status = out[:4]
    assert int(status.abs().sum()) == 0
    ms = {k: v / steps for k, v in t.items()}
    # the host C++ on the first rows, one thread, from K6d's trips
    hr = min(R, host_rows)
    Dh, Th, demh = D[:hr].cpu().numpy(), T[:hr].cpu().numpy(), dem[:hr].cpu().numpy()
    oph, clh, svh = op[:hr].tolist(), cl[:hr].tolist(), sv[:hr].tolist()
    bv, bt, bn = (c[:hr].cpu().numpy() for c in built)
    before = [_trips(bv[k], bt[k], bn[k]) for k in range(hr)]
    t0 = time.perf_counter()
    host = [rt.tw_improve(Dh[k], Th[k], before[k], demh[k].tolist(), 9e12, 9e12, oph[k], clh[k], svh[k])
            for k in range(hr)]
    host_ms = (time.perf_counter() - t0) * 1000.0
    vh, th, nh, sh = visit[:hr].cpu().numpy(), trip_of[:hr].cpu().numpy(), ntrips[:hr].cpu().numpy(), search[:hr].cpu().numpy()
    keys = ("moves", "rejected", "trips_before", "trips_after", "len_before_q", "len_after_q", "waiting_q")
    for k in range(hr):       # the same answers
        assert host[k][0] == _trips(vh[k], th[k], nh[k]) and [host[k][2][key] for key in keys] == sh[k].tolist(), k
    s = search.double()
    return {"metric": "window-aware local search (relocate / swap, K6e) beside the cheapest insertion (K6d), and the host C++",
            "requests": R, "stops": stops, "steps": steps, "windowed_share": 0.7,
            "time_windows_ms": ms["time_windows"], "tw_improve_ms": ms["tw_improve"],
            "tw_improve_over_time_windows": ms["tw_improve"] / ms["time_windows"],
            "host_cpp_rows": hr, "host_cpp_ms": host_ms, "host_cpp_ms_all_rows": host_ms * R / hr,
            "host_cpp_over_kernel": host_ms * R / hr / ms["tw_improve"],
            "moves_per_request": float(s[:, 0].mean()), "rejected": int(search[:, 1].sum()),
            "trips_before": int(search[:, 2].sum()), "trips_after": int(search[:, 3].sum()),
            "distance_after_over_before": float(s[:, 5].sum() / s[:, 4].sum()),
            "km_saved_per_request": float((s[:, 4] - s[:, 5]).mean()) / 1e6,
            "waiting_s_per_request": float(s[:, 6].mean()) / 1000.0}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x10,1000x100", help="requests x stops, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=500, help="rows the host C++ is timed on (scaled to all)")
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
