// What the four windowed trip kernels K6d-K6g (route_tw / route_tw_improve / route_pd /
// route_pd_improve .hip) share on top of route_team.h, each piece defined once: the launch
// arguments (WindowedRows, declared in ops.h), the LDS prefix and its typed view, the row's global
// pointers and limits, the gather, the walks over one trip (departures, latest starts, schedule), the
// row as the constructor left it, kinds and mates of a shipment row and the f64 acceptance walks.
// Only those four files include this header.  The host twin is WindowedProblem with its walks in
// runtime/route_trips.h.
//
// Barrier discipline: route_team.h's.  Every helper says whether it is team-uniform (it holds a
// barrier or a reduction: call it from control flow the whole team takes alike), one lane, or
// per-lane with no barrier and no cross-lane operation.  No helper adds LDS or atomics.
#pragma once
#include "ops.h"
#include "route_team.h"

namespace rt {
namespace team {

constexpr int kPlain = 0, kPickup = 1, kDelivery = 2;  // the kind of a stop of a shipment row

// ---- the LDS prefix of K6d-K6g (offsets in bytes): a kernel's layout struct takes it first, then
// its own arrays
struct WindowLds {
  size_t Q = 0, T = 0, open = 0, close = 0, sv = 0, qd = 0, dep = 0, z = 0;
  WindowLds() = default;
  __host__ __device__ constexpr WindowLds(LdsCarve& c, int kc) {
    Q = c.take(4, (size_t)(kc + 1) * matrix_stride(kc));
    T = c.take(4, (size_t)(kc + 1) * matrix_stride(kc));
    open = c.take(8, kc + 4);
    close = c.take(8, kc + 4);
    sv = c.take(8, kc + 4);
    qd = c.take(8, kc + 4);
    dep = c.take(8, kc + 4);  // K6d / K6f: [0..k] of the trip under construction; K6e / K6g: per flat position
    z = c.take(8, kc + 4);    // likewise, [1..k]
  }
};

// the prefix as typed pointers into one team's LDS: both quantized matrices as int32 with row stride
// S (an unusable entry is INT_MAX), open / close / service / demand per stop (int64; the depot is
// open from 0, never closes and takes no service), dep[] and z[]
struct WindowView {
  int *sQ, *sT;
  long long *open, *close, *sv, *qd, *dep, *z;
  int S;
};
__device__ __forceinline__ WindowView window_view(unsigned char* base, const WindowLds& L, int kc) {
  return {(int*)(base + L.Q),         (int*)(base + L.T),        (long long*)(base + L.open),
          (long long*)(base + L.close), (long long*)(base + L.sv), (long long*)(base + L.qd),
          (long long*)(base + L.dep),   (long long*)(base + L.z),  matrix_stride(kc)};
}

// ---- one request row in global memory: its matrices, demands, windows and pickup_from (null
// without), its four per-position outputs, the per-row outputs of the launch (whole arrays), and the
// limits as f64 and fixed point (-1: NaN or negative)
struct WindowRow {
  const double *d, *t, *dem;
  const long long *op, *cl, *sv;
  const int* pf;
  int *vrow, *trow;
  long long *arow, *strow;
  int *ntrips, *status;
  long long* stats;
  double MD, CAP;
  long long cap_q, max_q;
};

// per-lane, no barrier: row r of the launch arguments (K6e / K6g; K6d / K6f through
// window_row_restrict)
__device__ __forceinline__ WindowRow window_row(const WindowedRows& a, int r) {
  const size_t at = (size_t)r * a.NM;
  WindowRow w = {a.D + at * a.NM, a.T + at * a.NM, a.demand + at, a.open + at, a.close + at, a.service + at,
                 a.pickup_from ? a.pickup_from + at : nullptr, a.visit + at, a.trip_of + at, a.arrival + at,
                 a.start + at, a.ntrips, a.status, a.stats, a.maxd[r], a.cap[r], 0, 0};
  w.cap_q = quantize_limit(w.CAP);
  w.max_q = quantize_limit(w.MD);
  return w;
}

// WindowedRows reaches a kernel as a struct by value, which cannot say that its arrays do not
// overlap; they are distinct tensors.  The two constructions K6d / K6f run faster when the compiler
// may assume so, the two searches K6e / K6g when it may not (measured:
// profiles/route_windows_refactor.md).  So K6d / K6f pass the row's pointers through __restrict__
// parameters once, here, and run as body(row) inside; a `return` in the body ends the stage for the
// thread.  per-lane, no barrier.
template <class Body>
__device__ __forceinline__ void with_restrict(const double* __restrict__ d, const double* __restrict__ t,
                                              const double* __restrict__ dem, const long long* __restrict__ op,
                                              const long long* __restrict__ cl, const long long* __restrict__ sv,
                                              const int* __restrict__ pf, int* __restrict__ vrow,
                                              int* __restrict__ trow, long long* __restrict__ arow,
                                              long long* __restrict__ strow, int* __restrict__ ntrips,
                                              int* __restrict__ status, long long* __restrict__ stats,
                                              const WindowRow& w, Body&& body) {
  body(WindowRow{d, t, dem, op, cl, sv, pf, vrow, trow, arow, strow, ntrips, status, stats, w.MD, w.CAP, w.cap_q,
                 w.max_q});
}
template <class Body>
__device__ __forceinline__ void window_row_restrict(const WindowedRows& a, int r, Body&& body) {
  const WindowRow w = window_row(a, r);
  with_restrict(w.d, w.t, w.dem, w.op, w.cl, w.sv, w.pf, w.vrow, w.trow, w.arow, w.strow, w.ntrips, w.status,
                w.stats, w, body);
}

// No barrier inside, but meant for the whole team: the row's n points are gathered into the view,
// both matrices quantized, the per-stop vectors with the depot's values at 0; per_stop(s) runs
// behind the writes of stop s in the same thread (K6e counts unusable demands there, K6f / K6g
// decode pickup_from).  The caller's next barrier covers the writes: K6d / K6f sync right behind
// it, K6e / K6g rely on the first barrier of flat_build.
template <int TEAM, class PerStop>
__device__ __forceinline__ void window_gather(const WindowRow& w, const WindowView& v, int NM, int n, int tid,
                                              PerStop&& per_stop) {
  const int S = v.S;
  for (int c = tid; c < n * n; c += TEAM) {
    const int x = c / n, y = c - x * n;
    v.sQ[x * S + y] = quantize_entry(w.d[(size_t)x * NM + y]);
    v.sT[x * S + y] = quantize_entry(w.t[(size_t)x * NM + y]);
  }
  for (int s = tid; s < n; s += TEAM) {
    v.open[s] = s == 0 ? 0 : w.op[s];
    v.close[s] = s == 0 ? kUnbounded : w.cl[s];
    v.sv[s] = s == 0 ? 0 : w.sv[s];
    v.qd[s] = s == 0 ? 0 : quantize_mm(w.dem[s]);
    per_stop(s);
  }
}

// per-lane, no barrier: kind / mate of point s as pickup_from names them (K6f's first pass, K6g's
// only one): a delivery names its pickup, a stop of the row other than itself; every other point is
// plain so far.  False on an entry that names something else.
__device__ __forceinline__ bool kind_mate_named(const int* pf, int s, int ns, int* kind, int* mate) {
  const int p = s == 0 ? -1 : pf[s];
  const bool named = p >= 1 && p <= ns && p != s;
  kind[s] = named ? kDelivery : kPlain;
  mate[s] = named ? p : 0;
  return p < 0 || named;
}

// ---- one trip of k stops as the walks see it: stop y = 0..k-1 is st[y], its departure dep[y] and
// its latest start z[y].  K6d / K6f keep the trip under construction as 0, s1..sk, 0 in ord[] with
// dep[0..k] and z[1..k], so they pass ord + 1, dep + 1, z + 1.  K6e / K6g pass the flat order, dep
// and z at the trip's start.
struct TripView {
  const int* st;
  int k;
  long long *dep, *z;
};

// one lane: the departures of the trip's stops, forwards (K6d / K6f: lane 0; K6e: a lane per trip)
__device__ __forceinline__ void trip_dep(const WindowView& v, const TripView& tr) {
  long long dp = 0;
  int a = 0;
  for (int y = 0; y < tr.k; ++y) {
    const int b = tr.st[y];
    dp = max64(dp + v.sT[a * v.S + b], v.open[b]) + v.sv[b];
    tr.dep[y] = dp;
    a = b;
  }
}
// one lane: the latest starts of the trip's k >= 1 stops, backwards (K6d / K6f: lane 1; K6e / K6g: a
// lane per trip, behind the forward walk)
__device__ __forceinline__ void trip_z(const WindowView& v, const TripView& tr) {
  int a = tr.st[tr.k - 1];
  long long zz = v.close[a];
  tr.z[tr.k - 1] = zz;
  for (int y = tr.k - 2; y >= 0; --y) {
    const int b = tr.st[y];
    const long long lim = zz - v.sT[b * v.S + a] - v.sv[b];
    zz = v.close[b] < lim ? v.close[b] : lim;
    tr.z[y] = zz;
    a = b;
  }
}

// one lane: the trip's schedule, arrivals into z[] and starts into dep[] (both no longer needed).
// K6d / K6f: lane 0 when a trip closes; K6e: a lane per trip at the end (K6g's own walk also adds
// the trip's length).
__device__ __forceinline__ void trip_schedule(const WindowView& v, const TripView& tr) {
  long long dp = 0;
  int a = 0;
  for (int y = 0; y < tr.k; ++y) {
    const int b = tr.st[y];
    const long long ar = dp + v.sT[a * v.S + b];
    const long long stt = max64(ar, v.open[b]);
    tr.z[y] = ar;
    tr.dep[y] = stt;
    dp = stt + v.sv[b];
    a = b;
  }
}

// per-lane, no barrier: cnt positions of the schedule trip_schedule left in z[] / dep[] go out behind
// position `first` of the row, a position per thread; trip_at(p) is the trip index written for
// position p.  Returns this lane's part of the waiting time (the caller sums over the team).
// K6d / K6f: a closed trip; K6e / K6g: the whole row.
template <int TEAM, class TripAt>
__device__ __forceinline__ long long schedule_out(const WindowRow& w, int first, const int* stops,
                                                  const long long* arr, const long long* sta, int cnt, int tid,
                                                  TripAt&& trip_at) {
  long long wait_part = 0;
  for (int p = tid; p < cnt; p += TEAM) {
    w.vrow[first + p] = stops[p];
    w.trow[first + p] = trip_at(p);
    w.arow[first + p] = arr[p];
    w.strow[first + p] = sta[p];
    wait_part += sta[p] - arr[p];
  }
  return wait_part;
}

// team-uniform (three team sums): the row as K6d / K6f left it in global memory: m, its trips, and
// wait0, its waiting time; false when visit is not a constructor's output, and the row is then left
// alone.  Used by K6e / K6g.
template <int TEAM>
__device__ __forceinline__ bool left_by_constructor(const WindowRow& w, int n, int ns, long long* red, int tid,
                                                    int& m, long long& wait0) {
  long long groups = 0, wait = 0, badv = 0;
  for (int p = tid; p < ns; p += TEAM) {
    const int s = w.vrow[p];
    badv += (s < 1 || s >= n) ? 1 : 0;
    groups += (p == 0 || w.trow[p] != w.trow[p - 1]) ? 1 : 0;
    wait += w.strow[p] - w.arow[p];
  }
  m = (int)Team<TEAM>::sum(groups, red, tid);
  wait0 = Team<TEAM>::sum(wait, red, tid);
  return Team<TEAM>::sum(badv, red, tid) == 0;
}

// ---- the f64 acceptance walks over staged legs / demands: the only places where float association
// matters.  One lane each.
// dv[0..c]: the legs of a trip of c stops, the way back last (K6d, K6f, K6g)
__device__ __forceinline__ bool length_walk(const double* dv, int c, double MD) {
  double s = 0.0;
  for (int p = 0; p < c; ++p) s += dv[p];
  return s + dv[c] <= MD;
}
// dm[0..c-1]: what the stops of a shipment trip add to or take from the load, kind_at(p) the kind of
// stop p: the plain stops' demands from the depot on, a pickup adds, every other stop takes off
// (K6f step 3, K6g step 4)
template <class KindAt>
__device__ __forceinline__ bool pd_load_walk(const double* dm, int c, double CAP, KindAt&& kind_at) {
  // dm[p] is loaded beside the kind lookup, not behind it: this is one lane's serial path
  double bs = 0.0;
  for (int p = 0; p < c; ++p) {
    const double w = dm[p];
    if (kind_at(p) == kPlain) bs += w;
  }
  bool fits = bs <= CAP;
  double load = bs;
  for (int p = 0; p < c; ++p) {
    const double w = dm[p];
    if (kind_at(p) == kPickup) {
      load += w;
      fits = fits && load <= CAP;
    } else {
      load -= w;
    }
  }
  return fits;
}

}  // namespace team
}  // namespace rt
