// K6d: cheapest-insertion construction of trips under time windows and service times (gfx950),
// opt-in per request row.
//
// The definition (fixed-point millimetres and milliseconds, the unusable-entry rule, the schedule
// and latest-start recurrences, alone-feasibility, the seed rule, the O(1) admissibility test, the
// (ins, u, j) tie rule and the f64 acceptance walks) is in routest_amd/routing/timewindows.py; the
// host C++ is rtr::tw_trips (runtime/route_trips.h).  All three are compared with ==: every quantity
// the search orders by is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row (teams, tiers and the barrier discipline: route_team.h).  What
// K6d shares with K6e-K6g (the launch arguments, the LDS prefix, the gather, the walks over one trip
// and the f64 length walk) is in route_windows.h.
//
// The row's two quantized matrices are gathered ONCE into LDS as int32 (an unusable entry is
// INT_MAX, so the narrowing is exact), with open / close / service / demand (int64), the trip
// order, dep[] and z[] of the trip under construction and the unrouted flags.  Per insertion step:
//   1. a lane owns an insertion position j (a power of two of lanes per row of candidates, so no
//      division) and strides over the unrouted stops u; the candidate is priced from four matrix
//      reads and tested against dep[j], z[j+1], the load and the length; the lane keeps
//      (min ins, then min code) with code = u << 8 | j.  No barrier, no cross-lane operation;
//   2. the team reduces (shuffles in a wave, LDS across waves);
//   3. the lengthened trip's f64 legs and demands are staged into LDS in parallel and two lanes,
//      one per walk, add them in order (the only place where float association matters);
//   4. accepted: the order shifts by one position per thread, one lane recomputes dep, one z.
// A closed trip's stops, arrivals and starts go out one position per thread.
#include "route_windows.h"

namespace rt {

namespace {

using namespace team;

// LDS of one team (offsets in bytes), for a stop capacity of kc
struct TwLds {
  WindowLds w;
  size_t dv = 0, dm = 0, ord = 0, unr = 0, reda = 0, redb = 0, misc = 0, bytes = 0;
  __host__ __device__ constexpr explicit TwLds(int kc) {
    LdsCarve c;
    w = WindowLds(c, kc);
    dv = c.take(8, kc + 4);   // the lengthened trip's legs, [0..k+1]
    dm = c.take(8, kc + 4);   // ... and its stops' demands, [0..k]
    ord = c.take(4, kc + 4);  // the trip 0, s1..sk, 0: [0..k+1]
    unr = c.take(4, kc + 4);  // per stop: still unrouted (alone pass: failed)
    reda = c.take(8, 16);
    redb = c.take(8, 16);
    misc = c.take(4, 8);      // [0], [1]: the two walks' verdicts
    bytes = c.bytes;
  }
};
static_assert(TwLds(32).bytes == 11616 && TwLds(128).bytes == 142944, "the layout is fixed");

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).  It must stay the
// first parameter: launch_two_tiers passes it there, in front of the launch's own arguments.
template <int TEAM>
__global__ __launch_bounds__(Team<TEAM>::BLOCK) void tw_trips_kernel(int KC, const WindowedRows rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Tm = Team<TEAM>;
  const Row rw = Tm::row(rows.npts, rows.R, rows.NM);
  if (!rw.mine) return;
  const int tid = rw.tid, r = rw.r, n = rw.n, ns = rw.ns, NM = rows.NM;
  if (rows.flag[r] == 0) return;  // not a time-window row: nothing of it is touched
  window_row_restrict(rows, r, [&](const WindowRow& row) {
    int *ntrips = row.ntrips, *status = row.status;
    long long* srow = row.stats + (size_t)r * 4;  // insertions, rejected, len_q, waiting_q
    if (ns == 0 || ns > kMaxStops || ns > KC) {
      if (tid == 0) {
        ntrips[r] = 0;
        status[r] = ns == 0 ? 0 : 2;  // 2: more stops than the stage takes
        srow[0] = srow[1] = srow[2] = srow[3] = 0;
      }
      return;
    }

    const TwLds L(KC);
    unsigned char* base = smem + (size_t)rw.team * L.bytes;
    const WindowView vw = window_view(base, L.w, KC);
    const int S = vw.S;
    int *sQ = vw.sQ, *sT = vw.sT;
    long long *s_open = vw.open, *s_close = vw.close, *s_sv = vw.sv, *s_qd = vw.qd, *s_dep = vw.dep, *s_z = vw.z;
    double* s_dv = (double*)(base + L.dv);
    double* s_dm = (double*)(base + L.dm);
    int* s_ord = (int*)(base + L.ord);
    int* s_unr = (int*)(base + L.unr);
    long long* s_reda = (long long*)(base + L.reda);
    long long* s_redb = (long long*)(base + L.redb);
    int* s_misc = (int*)(base + L.misc);

    const double *d = row.d, *dem = row.dem;
    int* vrow = row.vrow;
    const double MD = row.MD, CAP = row.CAP;
    const long long cap_q = row.cap_q, max_q = row.max_q;

    // ---- gather: both quantized matrices and the per-stop vectors
    window_gather<TEAM>(row, vw, NM, n, tid, [](int) {});
    Tm::sync();

    // ---- alone-feasibility of every stop
    long long nbad = 0;
    for (int s = 1 + tid; s <= ns; s += TEAM) {
      bool ok = dem[s] <= CAP && (0.0 + (d[s] + d[(size_t)s * NM])) <= MD;
      const int t0s = sT[s], ts0 = sT[s * S];
      ok = ok && sQ[s] != kUnusable && sQ[s * S] != kUnusable && t0s != kUnusable && ts0 != kUnusable;
      const long long st0 = (long long)t0s > s_open[s] ? (long long)t0s : s_open[s];
      ok = ok && st0 <= s_close[s];
      s_unr[s] = ok ? 0 : 1;
      nbad += ok ? 0 : 1;
    }
    nbad = Tm::sum(nbad, s_reda, tid);
    Tm::sync();
    if (nbad != 0) {  // status 1: visit lists the stops that passed, so the others are the failing ones
      if (tid == 0) {
        int k = 0;
        for (int s = 1; s <= ns; ++s)
          if (!s_unr[s]) vrow[k++] = s;
        ntrips[r] = 0;
        status[r] = 1;
        srow[0] = srow[1] = srow[2] = srow[3] = 0;
      }
      return;
    }
    for (int s = tid; s <= ns; s += TEAM) s_unr[s] = s == 0 ? 0 : 1;

    // ---- the construction
    int left = ns, placed = 0, trips = 0;
    long long insertions = 0, rejected = 0, len_q = 0, wait_part = 0;
    while (left > 0) {
      Tm::sync();
      // the seed: the unrouted stop of smallest (close, index)
      long long ka = LLONG_MAX, kb = LLONG_MAX;
      for (int s = 1 + tid; s <= ns; s += TEAM)
        if (s_unr[s]) {
          const long long c = s_close[s];
          if (c < ka || (c == ka && s < kb)) {
            ka = c;
            kb = s;
          }
        }
      Tm::min2(ka, kb, s_reda, s_redb, tid);
      if (kb == LLONG_MAX) break;  // cannot happen: left > 0 stops are unrouted (uniform over the team)
      const int seed = (int)kb;    // 1..ns
      int k = 1;
      long long Lq = (long long)sQ[seed] + sQ[seed * S], Wq = s_qd[seed];
      if (tid == 0) {
        s_ord[0] = 0;
        s_ord[1] = seed;
        s_ord[2] = 0;
        s_unr[seed] = 0;
      }
      --left;
      while (left > 0) {
        Tm::sync();
        // dep[0..k] and z[1..k] of the trip as it stands, one lane each
        const TripView trip = {s_ord + 1, k, s_dep + 1, s_z + 1};
        if (tid == 0) {
          s_dep[0] = 0;
          trip_dep(vw, trip);
        } else if (tid == 1) {
          trip_z(vw, trip);
        }
        Tm::sync();

        // 1. the candidate scan: this lane's position j, the unrouted stops u it strides over
        const Lanes ln = Tm::split(k + 1, tid);
        const int CW = ln.CW, col0 = ln.col0, row0 = ln.row0, rstep = ln.rstep;
        long long bi = LLONG_MAX, bc = LLONG_MAX;
        for (int j = col0; j <= k; j += CW) {
          const int a = s_ord[j], b = s_ord[j + 1];
          const long long depj = s_dep[j], qab = sQ[a * S + b];
          const long long zn = j < k ? s_z[j + 1] : 0;
          const int* qa = sQ + a * S;
          const int* ta = sT + a * S;
          for (int u = 1 + row0; u <= ns; u += rstep) {
            if (!s_unr[u]) continue;
            const int qau = qa[u], qub = sQ[u * S + b], tau = ta[u], tub = sT[u * S + b];
            if (qau == kUnusable || qub == kUnusable || tau == kUnusable || tub == kUnusable) continue;
            const long long ins = (long long)qau + qub - qab;
            const long long ar = depj + tau;
            const long long st = ar > s_open[u] ? ar : s_open[u];
            if (st > s_close[u]) continue;
            if (j < k && st + s_sv[u] + tub > zn) continue;
            if (!(Wq + s_qd[u] <= cap_q) || !(Lq + ins <= max_q)) continue;
            const long long code = ((long long)u << 8) | j;
            if (ins < bi || (ins == bi && code < bc)) {
              bi = ins;
              bc = code;
            }
          }
        }
        // 2. (min ins, then min code) over the team
        Tm::min2(bi, bc, s_reda, s_redb, tid);
        if (bc == LLONG_MAX) break;  // no admissible candidate: the trip is closed
        const int bu = (int)(bc >> 8), bj = (int)(bc & 255);

        // 3. acceptance as the greedy measures it: the lengthened trip, f64, in visiting order
        const int kk = k + 1;  // its stops; position p of it is ord[p], u at bj + 1, ord[p - 1] behind
        for (int e = tid; e <= kk; e += TEAM) {
          const int a = e <= bj ? s_ord[e] : (e == bj + 1 ? bu : s_ord[e - 1]);
          const int b = e + 1 <= bj ? s_ord[e + 1] : (e == bj ? bu : s_ord[e]);
          s_dv[e] = d[(size_t)a * NM + b];
          if (e < kk) s_dm[e] = dem[b];
        }
        Tm::sync();
        if (tid == 0) {
          s_misc[0] = length_walk(s_dv, kk, MD) ? 1 : 0;
        } else if (tid == 1) {
          double load = 0.0;
          for (int p = 0; p < kk; ++p) load += s_dm[p];
          s_misc[1] = load <= CAP ? 1 : 0;
        }
        Tm::sync();
        if (!(s_misc[0] != 0 && s_misc[1] != 0)) {  // not applied: the trip is closed
          ++rejected;
          break;
        }

        // 4. the insertion: the positions behind bj move back by one, one position per thread
        const int p = tid;  // k + 3 <= TEAM positions in both tiers
        const int moved = (p >= bj + 2 && p <= kk + 1) ? s_ord[p - 1] : 0;
        Tm::sync();
        if (p >= bj + 2 && p <= kk + 1) s_ord[p] = moved;
        if (p == bj + 1) {
          s_ord[p] = bu;
          s_unr[bu] = 0;
        }
        k = kk;
        Lq += bi;
        Wq += s_qd[bu];
        ++insertions;
        --left;
      }
      Tm::sync();
      // the closed trip: one lane walks its schedule (arrivals into z[], starts into dep[], both no
      // longer needed), then its stops, arrivals and starts go out one position per thread
      if (tid == 0) trip_schedule(vw, TripView{s_ord + 1, k, s_dep + 1, s_z + 1});
      Tm::sync();
      wait_part += schedule_out<TEAM>(row, placed, s_ord + 1, s_z + 1, s_dep + 1, k, tid, [&](int) { return trips; });
      placed += k;
      len_q += Lq;
      ++trips;
    }
    const long long waiting = Tm::sum(wait_part, s_reda, tid);
    if (tid == 0) {
      ntrips[r] = trips;
      status[r] = 0;
      srow[0] = insertions;
      srow[1] = rejected;
      srow[2] = len_q;
      srow[3] = waiting;
    }
  });
}

}  // namespace

hipError_t launch_tw_trips(const WindowedRows& rows, hipStream_t stream) {
  // both int32 matrices of 128 stops (2 x 66.6 KB) and the per-stop arrays
  return team::launch_two_tiers<TwLds>(tw_trips_kernel<64>, tw_trips_kernel<team::kLargeTeam>, rows.R, rows.NM,
                                       stream, rows);
}

}  // namespace rt
