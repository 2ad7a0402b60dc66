// K6f: cheapest-insertion construction of trips that hold plain stops and pickup -> delivery pairs,
// under time windows and service times (gfx950), opt-in per request row.
//
// The definition (K6d's fixed point and time tests; kinds and mates; the integer load profile and
// its maximum; alone-feasibility of a pair as the trip 0, p, v, 0; the seed rule over units; the
// candidates of a pair at two positions (i, j) with the departures behind p carried forward; the
// (ins, u, i, j) tie rule and the two f64 acceptance walks) is in routest_amd/routing/shipments.py;
// the host C++ is rtr::pd_trips (runtime/route_trips.h).  All three are compared with ==: every
// quantity the search orders by is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row (teams, tiers and the barrier discipline: route_team.h).  What
// K6f shares with K6d, K6e and K6g (the launch arguments, the LDS prefix, the gather, kinds and
// mates, the walks over one trip and the f64 acceptance walks) is in route_windows.h.  The pricing of
// one unit at one position (step 1) is kept in two copies, here and in K6g's type-0 scan: shared, it
// put K6g's small tier over the speed bound in the one visit that measured it
// (profiles/route_windows_refactor.md).
//
// The LDS is K6d's image (both quantized matrices as int32, open / close / service / demand, the
// trip order, dep[], z[], the unrouted flags) plus load[] / pm[] of the trip under construction
// (int64) and kind / mate per stop (int32).  Per insertion step:
//   1. a lane owns a position i (a power of two of lanes per row of candidates) and strides over
//      the unrouted units u.  A plain unit is K6d's candidate with pm[i] in the load test.  For a
//      pair the lane prices j == i, then, unless the z[i+1] test fails, walks j = i+1..k carrying
//      the shifted departure nd, the running max(load[i..j]) and the first bracket of ins in
//      registers, reading only LDS.  The walk's only exit is j > k; everything else inside it is a
//      select.  No barrier, no cross-lane operation.  The lane keeps (min ins, then min code),
//      code = u << 16 | i << 8 | j;
//   2. the team reduces (shuffles in a wave, LDS across waves);
//   3. the lengthened trip's f64 legs and demands are staged into LDS in parallel and two lanes,
//      one per walk, add them in order (the only place where float association matters);
//   4. accepted: the order shifts by up to two positions, one position per thread; one lane each
//      recomputes dep, z and load / pm.
// A closed trip's stops, arrivals and starts go out one position per thread.
#include "route_windows.h"

namespace rt {

namespace {

using namespace team;

// LDS of one team (offsets in bytes), for a stop capacity of kc
struct PdLds {
  WindowLds w;
  size_t dv = 0, dm = 0, ord = 0, unr = 0, reda = 0, redb = 0, misc = 0, load = 0, pm = 0, kind = 0, mate = 0,
         bytes = 0;
  __host__ __device__ constexpr explicit PdLds(int kc) {
    LdsCarve c;
    w = WindowLds(c, kc);
    dv = c.take(8, kc + 4);    // the lengthened trip's legs, [0..k+2]
    dm = c.take(8, kc + 4);    // ... and what its stops add to or take from the load, [0..k+1]
    ord = c.take(4, kc + 4);   // the trip 0, s1..sk, 0: [0..k+1]
    unr = c.take(4, kc + 4);   // per stop: still unrouted (alone pass: failed)
    reda = c.take(8, 16);
    redb = c.take(8, 16);
    misc = c.take(4, 8);       // [0], [1]: the two walks' verdicts
    load = c.take(8, kc + 4);  // the load on leaving position x, [0..k]
    pm = c.take(8, kc + 4);    // max(load[0..x])
    kind = c.take(4, kc + 4);
    mate = c.take(4, kc + 4);
    bytes = c.bytes;
  }
};
static_assert(PdLds(32).bytes == 12480 && PdLds(128).bytes == 146112, "the layout is fixed");

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).  It must stay the
// first parameter: launch_two_tiers passes it there, in front of the launch's own arguments.
template <int TEAM>
__global__ __launch_bounds__(Team<TEAM>::BLOCK) void pd_trips_kernel(int KC, const WindowedRows rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Tm = Team<TEAM>;
  const Row rw = Tm::row(rows.npts, rows.R, rows.NM);
  if (!rw.mine) return;
  const int tid = rw.tid, r = rw.r, n = rw.n, ns = rw.ns, NM = rows.NM;
  if (rows.flag[r] == 0) return;  // not a shipment row: nothing of it is touched
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

    const PdLds L(KC);
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
    long long* s_load = (long long*)(base + L.load);
    long long* s_pm = (long long*)(base + L.pm);
    int* s_kind = (int*)(base + L.kind);
    int* s_mate = (int*)(base + L.mate);

    const double *d = row.d, *dem = row.dem;
    int* vrow = row.vrow;
    const double MD = row.MD, CAP = row.CAP;
    const long long cap_q = row.cap_q, max_q = row.max_q;

    // ---- gather: both quantized matrices and the per-stop vectors; kinds, first pass: a delivery
    // names its pickup, a stop of the row other than itself
    long long nbad = 0;
    window_gather<TEAM>(row, vw, NM, n, tid,
                        [&](int s) { nbad += kind_mate_named(row.pf, s, ns, s_kind, s_mate) ? 0 : 1; });
    Tm::sync();
    // second pass: the pickup learns its delivery (of two deliveries that name it, one is kept and
    // the third pass finds the other).  Only mate[] of stops that are no delivery is written here and
    // only mate[] of deliveries is read.
    for (int v = 1 + tid; v <= ns; v += TEAM)
      if (s_kind[v] == kDelivery) {
        const int p = s_mate[v];
        if (s_kind[p] == kDelivery) nbad += 1;  // the named stop is itself a delivery
        else s_mate[p] = v;
      }
    Tm::sync();
    // third pass, a stop per thread (ns <= TEAM in both tiers): a delivery checks that its pickup
    // kept it, a stop that learnt a delivery becomes a pickup.  kind[] is read here and written
    // behind the barrier.
    const int own = 1 + tid;
    int own_kind = kPlain;
    if (own <= ns) {
      own_kind = s_kind[own];
      if (own_kind == kDelivery) {
        const int p = s_mate[own];
        if (s_kind[p] != kDelivery && s_mate[p] != own) nbad += 1;  // its pickup serves another delivery
      } else if (s_mate[own] != 0) {
        own_kind = kPickup;
      }
    }
    Tm::sync();
    if (own <= ns) s_kind[own] = own_kind;
    nbad = Tm::sum(nbad, s_reda, tid);
    if (nbad != 0) {  // status 3: pickup_from is malformed
      if (tid == 0) {
        ntrips[r] = 0;
        status[r] = 3;
        srow[0] = srow[1] = srow[2] = srow[3] = 0;
      }
      return;
    }
    Tm::sync();

    // ---- alone-feasibility: a plain stop as in K6d; a pair once, at its pickup, as 0, p, v, 0
    for (int s = 1 + tid; s <= ns; s += TEAM) {
      const int kd = s_kind[s];
      if (kd == kDelivery) continue;  // its pickup's lane writes both flags
      bool ok;
      if (kd == kPlain) {
        ok = dem[s] <= CAP && (0.0 + (d[s] + d[(size_t)s * NM])) <= MD;
        const int t0s = sT[s], ts0 = sT[s * S];
        ok = ok && sQ[s] != kUnusable && sQ[s * S] != kUnusable && t0s != kUnusable && ts0 != kUnusable;
        ok = ok && max64(t0s, s_open[s]) <= s_close[s];
      } else {
        const int v = s_mate[s];
        double w = 0.0;
        w += d[s];
        w += d[(size_t)s * NM + v];
        ok = w + d[(size_t)v * NM] <= MD;
        double ld = 0.0;
        ok = ok && ld <= CAP;
        ld += dem[v];
        ok = ok && ld <= CAP;
        const int t0p = sT[s], tpv = sT[s * S + v], tv0 = sT[v * S];
        ok = ok && sQ[s] != kUnusable && sQ[s * S + v] != kUnusable && sQ[v * S] != kUnusable &&
             t0p != kUnusable && tpv != kUnusable && tv0 != kUnusable;
        const long long sp = max64(t0p, s_open[s]);
        const long long s2 = max64(sp + s_sv[s] + tpv, s_open[v]);
        ok = ok && sp <= s_close[s] && s2 <= s_close[v];
        s_unr[v] = ok ? 0 : 1;
        nbad += ok ? 0 : 1;
      }
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
      // the seed: the unrouted unit of smallest (key, index)
      long long ka = LLONG_MAX, kb = LLONG_MAX;
      for (int s = 1 + tid; s <= ns; s += TEAM) {
        const int kd = s_kind[s];
        if (s_unr[s] && kd != kDelivery) {
          long long c = s_close[s];
          if (kd == kPickup) {
            const long long c2 = s_close[s_mate[s]];
            c = c2 < c ? c2 : c;
          }
          if (c < ka || (c == ka && s < kb)) {
            ka = c;
            kb = s;
          }
        }
      }
      Tm::min2(ka, kb, s_reda, s_redb, tid);
      if (kb == LLONG_MAX) break;  // cannot happen: left > 0 stops are unrouted (uniform over the team)
      const int seed = (int)kb;    // 1..ns
      const int seed_mate = s_kind[seed] == kPickup ? s_mate[seed] : 0;
      int k = seed_mate ? 2 : 1;
      long long Lq = seed_mate ? (long long)sQ[seed] + sQ[seed * S + seed_mate] + sQ[seed_mate * S]
                               : (long long)sQ[seed] + sQ[seed * S];
      Tm::sync();  // every lane has read the seed's kind and unrouted flags
      if (tid == 0) {
        s_ord[0] = 0;
        s_ord[1] = seed;
        s_ord[2] = seed_mate;  // 0: the way back of a plain seed
        s_ord[3] = 0;
        s_unr[seed] = 0;
        if (seed_mate) s_unr[seed_mate] = 0;
      }
      left -= k;
      while (left > 0) {
        Tm::sync();
        // dep[0..k], z[1..k] and load / pm [0..k] of the trip as it stands, one lane each
        const TripView trip = {s_ord + 1, k, s_dep + 1, s_z + 1};
        if (tid == 0) {
          s_dep[0] = 0;
          trip_dep(vw, trip);
        } else if (tid == 1) {
          trip_z(vw, trip);
        } else if (tid == 2) {
          long long ld = 0;
          for (int i = 1; i <= k; ++i) {
            const int b = s_ord[i];
            ld += s_kind[b] == kPlain ? s_qd[b] : 0;
          }
          long long top = ld;
          s_load[0] = ld;
          s_pm[0] = ld;
          for (int i = 1; i <= k; ++i) {
            const int b = s_ord[i];
            ld += s_kind[b] == kPickup ? s_qd[s_mate[b]] : -s_qd[b];
            top = ld > top ? ld : top;
            s_load[i] = ld;
            s_pm[i] = top;
          }
        }
        Tm::sync();

        // 1. the candidate scan: this lane's position i, the unrouted units u it strides over
        const Lanes ln = Tm::split(k + 1, tid);
        const int CW = ln.CW, col0 = ln.col0, row0 = ln.row0, rstep = ln.rstep;
        long long bi = LLONG_MAX, bc = LLONG_MAX;
        for (int i = col0; i <= k; i += CW) {
          const int a = s_ord[i], b = s_ord[i + 1];
          const long long depi = s_dep[i], qab = sQ[a * S + b];
          const long long zn = i < k ? s_z[i + 1] : 0;
          const long long ldi = s_load[i], pmi = s_pm[i];
          const long long open_b = s_open[b], sv_b = s_sv[b];
          const int* qa = sQ + a * S;
          const int* ta = sT + a * S;
          for (int u = 1 + row0; u <= ns; u += rstep) {
            const int kd = s_kind[u];
            if (!s_unr[u] || kd == kDelivery) continue;
            const int qau = qa[u], tau = ta[u];
            if (qau == kUnusable || tau == kUnusable) continue;
            const long long st = max64(depi + tau, s_open[u]);
            if (st > s_close[u]) continue;
            const int qub = sQ[u * S + b], tub = sT[u * S + b];
            const bool ub = qub != kUnusable && tub != kUnusable;
            const long long code0 = ((long long)u << 16) | ((long long)i << 8);
            if (kd == kPlain) {
              const long long ins = (long long)qau + qub - qab;
              bool ok = ub && (i == k || st + s_sv[u] + tub <= zn);
              ok = ok && pmi + s_qd[u] <= cap_q && Lq + ins <= max_q;
              const long long code = code0 | i;
              if (ok && (ins < bi || (ins == bi && code < bc))) {
                bi = ins;
                bc = code;
              }
              continue;
            }
            const int v = s_mate[u];
            const long long amt = s_qd[v], open_v = s_open[v], close_v = s_close[v], sv_v = s_sv[v];
            const long long dpu = st + s_sv[u];  // the departure from the pickup
            {  // j == i: a -> p -> v -> b
              const int quv = sQ[u * S + v], tuv = sT[u * S + v], qvb = sQ[v * S + b], tvb = sT[v * S + b];
              const long long ins = (long long)qau + quv + qvb - qab;
              const long long s2 = max64(dpu + tuv, open_v);
              bool ok = quv != kUnusable && tuv != kUnusable && qvb != kUnusable && tvb != kUnusable;
              ok = ok && s2 <= close_v && (i == k || s2 + sv_v + tvb <= zn);
              ok = ok && ldi + amt <= cap_q && Lq + ins <= max_q;
              const long long code = code0 | i;
              if (ok && (ins < bi || (ins == bi && code < bc))) {
                bi = ins;
                bc = code;
              }
            }
            // j > i: needs the leg p -> b and the stops behind p still in time
            const long long first = dpu + tub;
            if (i == k || !ub || first > zn) continue;
            const long long ins1 = (long long)qau + qub - qab;
            long long nd = max64(first, open_b) + sv_b, mx = ldi;
            int c = b;                   // t[j]
            const int* tv = sT + v * S;  // rows of the delivery
            const int* qv = sQ + v * S;
            for (int j = i + 1; j <= k; ++j) {
              const int e = s_ord[j + 1];
              const long long lj = s_load[j];
              mx = lj > mx ? lj : mx;
              const int qcv = sQ[c * S + v], tcv = sT[c * S + v], qve = qv[e], tve = tv[e];
              const long long ins = ins1 + ((long long)qcv + qve - sQ[c * S + e]);
              const long long s2 = max64(nd + tcv, open_v);
              const long long zj = j < k ? s_z[j + 1] : LLONG_MAX;
              bool ok = qcv != kUnusable && tcv != kUnusable && qve != kUnusable && tve != kUnusable;
              ok = ok && s2 <= close_v && (j == k || s2 + sv_v + tve <= zj);
              ok = ok && mx + amt <= cap_q && Lq + ins <= max_q;
              const long long code = code0 | j;
              const bool take = ok && (ins < bi || (ins == bi && code < bc));
              bi = take ? ins : bi;
              bc = take ? code : bc;
              // the departure from t[j+1] behind the shift (unused behind j == k)
              nd = max64(nd + sT[c * S + e], s_open[e]) + s_sv[e];
              c = e;
            }
          }
        }
        // 2. (min ins, then min code) over the team
        Tm::min2(bi, bc, s_reda, s_redb, tid);
        if (bc == LLONG_MAX) break;  // no admissible candidate: the trip is closed
        const int bu = (int)(bc >> 16), pi = (int)((bc >> 8) & 255), pj = (int)(bc & 255);
        const int bv = s_kind[bu] == kPickup ? s_mate[bu] : 0;
        const int cnt = bv ? 2 : 1;

        // 3. acceptance as the greedy measures it: the lengthened trip, f64, in visiting order
        const int kk = k + cnt;  // its stops
        // position x of the lengthened trip: u at pi + 1 and, for a pair, v at pj + 2
        auto newat = [&](int x) -> int {
          if (x <= pi) return s_ord[x];
          if (x == pi + 1) return bu;
          if (cnt == 1 || x <= pj + 1) return s_ord[x - 1];
          if (x == pj + 2) return bv;
          return s_ord[x - 2];
        };
        for (int e = tid; e <= kk; e += TEAM) {
          const int a = newat(e), b = newat(e + 1);
          s_dv[e] = d[(size_t)a * NM + b];
          if (e < kk) s_dm[e] = dem[s_kind[b] == kPickup ? s_mate[b] : b];
        }
        Tm::sync();
        if (tid == 0) {
          s_misc[0] = length_walk(s_dv, kk, MD) ? 1 : 0;
        } else if (tid == 1) {
          s_misc[1] = pd_load_walk(s_dm, kk, CAP, [&](int p) { return s_kind[newat(p + 1)]; }) ? 1 : 0;
        }
        Tm::sync();
        if (!(s_misc[0] != 0 && s_misc[1] != 0)) {  // not applied: the trip is closed
          ++rejected;
          break;
        }

        // 4. the insertion: the positions behind pi move back by one or two, one position per thread
        const int x = tid;  // k + 4 <= TEAM positions in both tiers
        const bool mine = x >= pi + 1 && x <= kk + 1;
        const int moved = mine ? newat(x) : 0;
        Tm::sync();
        if (mine) s_ord[x] = moved;
        if (x == 0) {
          s_unr[bu] = 0;
          if (bv) s_unr[bv] = 0;
        }
        k = kk;
        Lq += bi;
        ++insertions;
        left -= cnt;
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

hipError_t launch_pd_trips(const WindowedRows& rows, hipStream_t stream) {
  // K6d's image (both int32 matrices of 128 stops: 2 x 66.6 KB) and the load profile, kinds and mates
  return team::launch_two_tiers<PdLds>(pd_trips_kernel<64>, pd_trips_kernel<team::kLargeTeam>, rows.R, rows.NM,
                                       stream, rows);
}

}  // namespace rt
