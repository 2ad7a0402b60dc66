// K6e: window-aware local search (relocate between trips, swap, relocate inside a trip) on the trips
// K6d built for a time-window row (gfx950), opt-in per request row.
//
// The definition (fixed-point millimetres and milliseconds, the unusable-entry rule, the three move
// types with their limits and O(1) / bounded-walk time tests, best-improvement selection with the
// (type, A, i, B, j) tie rule, the f64 acceptance walks, the move cap and the skip conditions) is in
// routest_amd/routing/tw_improve.py; the host C++ is rtr::tw_improve_trips (runtime/route_trips.h).
// All three are compared with ==: every quantity the search orders by is an int64 sum, so the
// schedule below cannot change it.
//
// One TEAM of threads per request row (teams, tiers and the barrier discipline: route_team.h).  What
// K6e shares with K6d, K6f and K6g (the launch arguments, the LDS prefix, the gather, the row as the
// constructor left it and the walks over one trip) is in route_windows.h.
//
// The row's two quantized matrices are gathered ONCE into LDS as int32 (an unusable entry is
// INT_MAX, so the narrowing is exact), as K6d does, with open / close / service / demand (int64).
// The order is route_team.h's flat order (a flat position orders like (A, i)); dep[] and z[] are
// kept per flat position.  Per move:
//   0. one lane per trip walks dep forwards and z backwards over its positions;
//   1. per position p (stop s, trip A, index i, neighbours prev / next): nb = q(prev,s) + q(s,next),
//      rem, whether A may lose s to another trip (bridge leg usable, Lq[A] - rem <= max_q, the next
//      stop still in time) and whether s may move inside A;
//   2. the candidate scan: a lane owns one column, an insertion edge (one in front of every position,
//      one closing every trip) or a swap partner, and strides over the positions p (a power of two
//      of lanes per row of candidates, so no division).  An edge of another trip prices a type-0
//      move, an edge of p's own trip a type-2 move; both and the swap are O(1) but for type 2's time
//      test, a walk of M - m + 1 positions that is run only for a candidate that would replace the
//      lane's best, with no barrier and no cross-lane operation inside it.  The lane keeps
//      (max gain, then min move code), the code packing (type, A, i, B, j);
//   3. the team reduces; everyone writes the moved order into the second copy, a position a thread;
//   4. acceptance as the greedy measures it: the touched trips' f64 legs and demands are staged into
//      LDS in parallel and one lane per trip adds them in order (the only place where float
//      association matters); accepted: the copies change roles, Lq / Wq take the move's deltas;
//      rejected: the first copy stays and the search ends.
// At the end the non-empty trips are compacted: one lane per trip walks its schedule, the positions
// go out one per thread and the waiting time by a team sum.
#include "route_windows.h"

namespace rt {

namespace {

using namespace team;

// LDS of one team (offsets in bytes), for a stop capacity of kc; [2]: two arrays of stride v8 / v4
struct TwImproveLds {
  WindowLds w;  // dep, z: per flat position, the departure and the latest start of its stop
  size_t Lq = 0, Wq = 0, rem = 0, nb = 0, dv = 0, dm = 0, ord = 0, tof = 0, tst = 0, cnt = 0, pw = 0, pn = 0,
         rank = 0, bnd = 0, redg = 0, redc = 0, misc = 0, bytes = 0;
  int v8 = 0, v4 = 0;
  __host__ __device__ constexpr explicit TwImproveLds(int kc) {
    LdsCarve c;
    w = WindowLds(c, kc);
    Lq = c.take(8, kc + 4);     // per trip
    Wq = c.take(8, kc + 4);
    rem = c.take(8, kc + 4);    // per flat position
    nb = c.take(8, kc + 4);
    dv = c.take(8, kc + 4, 2);  // a touched trip's legs
    dm = c.take(8, kc + 4, 2);  // ... and its stops' demands
    ord = c.take(4, kc + 4, 2); // the order and its moved copy
    tof = c.take(4, kc + 4, 2);
    tst = c.take(4, kc + 4, 2);
    cnt = c.take(4, kc + 4, 2);
    pw = c.take(4, kc + 4);     // s | A << 8 | i << 16 | may-leave << 25 | may-shift << 26
    pn = c.take(4, kc + 4);     // prev | next << 8
    rank = c.take(4, kc + 4);
    bnd = c.take(4, kc + 4);
    redg = c.take(8, 16);
    redc = c.take(8, 16);
    misc = c.take(4, 8);        // [0], [1]: the two walks' verdicts
    bytes = c.bytes;
    v8 = (int)(align16((size_t)(kc + 4) * 8) / 8);
    v4 = (int)(align16((size_t)(kc + 4) * 4) / 4);
  }
};
static_assert(TwImproveLds(32).bytes == 14784 && TwImproveLds(128).bytes == 154560, "the layout is fixed");

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).  It must stay the
// first parameter: launch_two_tiers passes it there, in front of the launch's own arguments.
template <int TEAM>
__global__ __launch_bounds__(Team<TEAM>::BLOCK) void tw_improve_kernel(int KC, const WindowedRows rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Tm = Team<TEAM>;
  const Row rw = Tm::row(rows.npts, rows.R, rows.NM);
  if (!rw.mine) return;
  const int tid = rw.tid, r = rw.r, n = rw.n, ns = rw.ns, NM = rows.NM;
  if (rows.flag[r] == 0 || rows.status[r] != 0) return;  // not asked for, or not planned: nothing is touched
  if (ns == 0 || ns > kMaxStops || ns > KC) return;

  const TwImproveLds L(KC);
  unsigned char* base = smem + (size_t)rw.team * L.bytes;
  const WindowView vw = window_view(base, L.w, KC);
  const int S = vw.S, V4 = L.v4, V8 = L.v8;
  int *sQ = vw.sQ, *sT = vw.sT;
  long long *s_open = vw.open, *s_close = vw.close, *s_sv = vw.sv, *s_qd = vw.qd, *s_dep = vw.dep, *s_z = vw.z;
  long long* s_Lq = (long long*)(base + L.Lq);
  long long* s_Wq = (long long*)(base + L.Wq);
  long long* s_rem = (long long*)(base + L.rem);
  long long* s_nb = (long long*)(base + L.nb);
  double* s_dv = (double*)(base + L.dv);
  double* s_dm = (double*)(base + L.dm);
  const FlatOrder flat = {(int*)(base + L.ord), (int*)(base + L.tof), (int*)(base + L.tst),
                          (int*)(base + L.cnt)};
  unsigned* s_pw = (unsigned*)(base + L.pw);
  unsigned* s_pn = (unsigned*)(base + L.pn);
  int* s_rank = (int*)(base + L.rank);
  int* s_bnd = (int*)(base + L.bnd);
  long long* s_redg = (long long*)(base + L.redg);
  long long* s_redc = (long long*)(base + L.redc);
  int* s_misc = (int*)(base + L.misc);

  const WindowRow row = window_row(rows, r);
  const double *d = row.d, *dem = row.dem;
  int *vrow = row.vrow, *trow = row.trow;
  long long* srow = rows.stats + (size_t)r * 7;
  const double MD = row.MD, CAP = row.CAP;
  const long long cap_q = row.cap_q, max_q = row.max_q;

  // ---- the row as K6d left it, from global memory: its trips, its waiting time, its validity
  int m;
  long long wait0;
  if (!left_by_constructor<TEAM>(row, n, ns, s_redg, tid, m, wait0)) return;  // not K6d's output

  // ---- gather: both quantized matrices, the per-stop vectors, the order, the trips
  long long bigdem = 0;
  window_gather<TEAM>(row, vw, NM, n, tid, [&](int s) { bigdem += s_qd[s] == kBig ? 1 : 0; });
  flat_build<TEAM>(flat, s_bnd, vrow, trow, ns, tid);
  const long long part = flat_trip_sums<TEAM>(flat, m, sQ, S, s_qd, s_Lq, s_Wq, tid);
  const long long before = Tm::sum(part, s_redg, tid);
  bigdem = Tm::sum(bigdem, s_redg, tid);
  if (bigdem != 0 || cap_q < 0 || max_q < 0) {  // the stage is skipped
    if (tid == 0) {
      srow[0] = srow[1] = 0;
      srow[2] = srow[3] = m;
      srow[4] = srow[5] = before;
      srow[6] = wait0;
    }
    return;
  }

  // ---- best-improvement search
  const int ncols = ns + m + ns;  // insertion edges (one per position, one per trip), swap partners
  const Lanes ln = Tm::split(ncols, tid);  // ncols >= 3
  const int CW = ln.CW, col0 = ln.col0, row0 = ln.row0, rstep = ln.rstep;
  const int limit = 4 * ns;
  int cur = 0, moves = 0, rejected = 0;
  while (moves < limit) {
    Tm::sync();
    const FlatOrder co = flat.copy(cur, V4);
    const int *ord = co.ord, *tof = co.tof, *tst = co.tst, *cnt = co.cnt;
    // 0. dep forwards and z backwards, one lane per trip
    for (int x = tid; x < m; x += TEAM) {
      const int st = tst[x];
      const TripView trip = {ord + st, cnt[x], s_dep + st, s_z + st};
      if (trip.k > 0) {
        trip_dep(vw, trip);
        trip_z(vw, trip);
      }
    }
    Tm::sync();
    // 1. per-position terms
    for (int p = tid; p < ns; p += TEAM) {
      const int s = ord[p], x = tof[p], i = p - tst[x] + 1, c = cnt[x];
      const int pv = i == 1 ? 0 : ord[p - 1], nx = i == c ? 0 : ord[p + 1];
      const long long nb = (long long)sQ[pv * S + s] + sQ[s * S + nx];
      const int qpn = sQ[pv * S + nx], tpn = sT[pv * S + nx];
      const bool single = c == 1;
      const long long rem = single ? nb : nb - qpn;
      const bool bridge = single || (qpn != kUnusable && tpn != kUnusable);
      bool may = bridge && s_Lq[x] - rem <= max_q;
      if (may && !single && i != c) {  // the next stop must still start in time
        const long long dprev = i == 1 ? 0 : s_dep[p - 1];
        may = max64(dprev + tpn, s_open[nx]) <= s_z[p + 1];
      }
      const bool shift = c >= 2 && bridge;
      s_nb[p] = nb;
      s_rem[p] = rem;
      s_pw[p] = (unsigned)s | ((unsigned)x << 8) | ((unsigned)i << 16) | (may ? 1u << 25 : 0u) |
                (shift ? 1u << 26 : 0u);
      s_pn[p] = (unsigned)pv | ((unsigned)nx << 8);
    }
    Tm::sync();

    // 2. the candidate scan
    long long bg = 0, bc = LLONG_MAX;
    for (int c = col0; c < ncols; c += CW) {
      if (c < ns + m) {  // the stop of position p goes to this edge (u, v) behind position j of trip B
        int u, v, B, j;
        long long depj, zn;
        if (c < ns) {
          const unsigned w = s_pw[c];
          u = s_pn[c] & 255;
          v = w & 255;
          B = (w >> 8) & 255;
          j = (int)((w >> 16) & 255) - 1;
          depj = j == 0 ? 0 : s_dep[c - 1];
          zn = s_z[c];
        } else {
          B = c - ns;
          j = cnt[B];
          if (j == 0) continue;  // an emptied trip is never a target
          const int lastp = tst[B] + j - 1;
          u = ord[lastp];
          v = 0;
          depj = s_dep[lastp];
          zn = LLONG_MAX;  // nothing behind: no latest start to meet
        }
        const long long eb = sQ[u * S + v], LB = s_Lq[B], WB = s_Wq[B];
        const int kB = cnt[B], fb = tst[B];
        const int* qu = sQ + u * S;
        const int* tu = sT + u * S;
        for (int p = row0; p < ns; p += rstep) {
          const unsigned pw = s_pw[p];
          const int s = pw & 255, A = (pw >> 8) & 255, i = (pw >> 16) & 255;
          const int qus = qu[s], qsv = sQ[s * S + v], tus = tu[s], tsv = sT[s * S + v];
          if (qus == kUnusable || qsv == kUnusable || tus == kUnusable || tsv == kUnusable) continue;
          const long long ins = (long long)qus + qsv - eb;
          const long long g = s_rem[p] - ins;
          if (g <= 0) continue;
          if (A != B) {  // type 0
            if (!((pw >> 25) & 1)) continue;
            if (!(WB + s_qd[s] <= cap_q) || !(LB + ins <= max_q)) continue;
            const long long st = max64(depj + tus, s_open[s]);
            if (st > s_close[s] || st + s_sv[s] + tsv > zn) continue;
            const long long code = move_code(0, A, i, B, j);
            if (g > bg || (g == bg && code < bc)) {
              bg = g;
              bc = code;
            }
          } else {       // type 2: inside the trip, positions lo..hi change
            if (!((pw >> 26) & 1) || j == i - 1 || j == i) continue;
            if (!(LB - g <= max_q)) continue;
            const long long code = move_code(2, A, i, A, j);
            if (!(g > bg || (g == bg && code < bc))) continue;  // the walk only where it can matter
            const int lo = j < i ? j + 1 : i, hi = j < i ? i : j;
            long long clock = lo == 1 ? 0 : s_dep[fb + lo - 2];
            int a = lo == 1 ? 0 : ord[fb + lo - 2];
            bool ok = true;
            for (int x = lo; x <= hi; ++x) {  // per-lane bounds: no barrier, no cross-lane operation
              const int b = j < i ? (x == lo ? s : ord[fb + x - 2]) : (x == hi ? s : ord[fb + x]);
              const long long st = max64(clock + sT[a * S + b], s_open[b]);
              if (st > s_close[b]) {
                ok = false;
                break;
              }
              clock = st + s_sv[b];
              a = b;
            }
            if (ok && hi < kB) {  // the suffix is unchanged: its first stop against the old z
              const int b = ord[fb + hi];
              ok = max64(clock + sT[a * S + b], s_open[b]) <= s_z[fb + hi];
            }
            if (ok) {
              bg = g;
              bc = code;
            }
          }
        }
      } else {           // type 1: the stop of position p and this partner change places, A < B
        const int p2 = c - (ns + m);
        const unsigned pw2 = s_pw[p2], pn2 = s_pn[p2];
        const int u = pw2 & 255, B = (pw2 >> 8) & 255, j = (pw2 >> 16) & 255;
        const int pb = pn2 & 255, nxb = (pn2 >> 8) & 255;
        const long long nb2 = s_nb[p2], LB = s_Lq[B], WB = s_Wq[B], qdu = s_qd[u];
        const long long dprevB = pb == 0 ? 0 : s_dep[p2 - 1];
        const long long znB = nxb == 0 ? LLONG_MAX : s_z[p2 + 1];
        const long long open_u = s_open[u], close_u = s_close[u], sv_u = s_sv[u];
        for (int p = row0; p < ns; p += rstep) {
          const unsigned pw = s_pw[p];
          const int s = pw & 255, A = (pw >> 8) & 255;
          if (A >= B) continue;
          const unsigned pn = s_pn[p];
          const int pa = pn & 255, na = (pn >> 8) & 255;
          const int qpu = sQ[pa * S + u], qun = sQ[u * S + na], qps = sQ[pb * S + s], qsn = sQ[s * S + nxb];
          const int tpu = sT[pa * S + u], tun = sT[u * S + na], tps = sT[pb * S + s], tsn = sT[s * S + nxb];
          if (qpu == kUnusable || qun == kUnusable || qps == kUnusable || qsn == kUnusable ||
              tpu == kUnusable || tun == kUnusable || tps == kUnusable || tsn == kUnusable)
            continue;
          const long long dA = (long long)qpu + qun - s_nb[p];
          const long long dB = (long long)qps + qsn - nb2;
          const long long g = -(dA + dB);
          if (g <= 0) continue;
          const long long wd = qdu - s_qd[s];  // what trip A's load gains
          if (!(s_Wq[A] + wd <= cap_q) || !(WB - wd <= cap_q) || !(s_Lq[A] + dA <= max_q) ||
              !(LB + dB <= max_q))
            continue;
          const long long dprevA = pa == 0 ? 0 : s_dep[p - 1];
          const long long su = max64(dprevA + tpu, open_u);
          if (su > close_u || (na != 0 && su + sv_u + tun > s_z[p + 1])) continue;
          const long long ss = max64(dprevB + tps, s_open[s]);
          if (ss > s_close[s] || ss + s_sv[s] + tsn > znB) continue;
          const long long code = move_code(1, A, (pw >> 16) & 255, B, j);
          if (g > bg || (g == bg && code < bc)) {
            bg = g;
            bc = code;
          }
        }
      }
    }
    // 3. (max gain, then min move code) over the team
    Tm::best(bg, bc, s_redg, s_redc, tid);
    if (bg <= 0) break;

    // the moved order in the other copy, then 4. the acceptance walks of the touched trips; an
    // emptied trip is not walked.  Undone: the first copy stays, the search ends.
    const Move mv = decode_move(bc);
    const FlatOrder nx = flat.copy(cur ^ 1, V4);
    const MoveDelta dl = flat_write_move<TEAM>(co, nx, mv, bg, ns, m, sQ, S, s_qd, s_rem, s_nb, s_pn, tid);
    Tm::sync();
    if (!flat_accept<TEAM, true>(nx, mv, d, dem, NM, MD, CAP, s_dv, s_dm, V8, s_misc, tid)) {
      rejected = 1;
      break;
    }
    if (tid == 0) flat_commit(s_Lq, s_Wq, mv, dl);
    cur ^= 1;
    ++moves;
  }
  Tm::sync();

  // ---- the non-empty trips, compacted in their order, with their schedule
  const FlatOrder fin = flat.copy(cur, V4);
  const int *ord = fin.ord, *tof = fin.tof, *tst = fin.tst, *cnt = fin.cnt;
  if (tid == 0) {
    long long after;
    const int k = flat_rank(cnt, s_Lq, m, s_rank, after);
    rows.ntrips[r] = k;
    srow[0] = moves;
    srow[1] = rejected;
    srow[2] = m;
    srow[3] = k;
    srow[4] = before;
    srow[5] = after;
  }
  // one lane per trip walks its schedule: arrivals into z[], starts into dep[] (no longer needed)
  for (int x = tid; x < m; x += TEAM)
    trip_schedule(vw, TripView{ord + tst[x], cnt[x], s_dep + tst[x], s_z + tst[x]});
  Tm::sync();
  const long long wait_part =
      schedule_out<TEAM>(row, 0, ord, s_z, s_dep, ns, tid, [&](int p) { return s_rank[tof[p]]; });
  const long long waiting = Tm::sum(wait_part, s_redg, tid);
  if (tid == 0) srow[6] = waiting;
}

}  // namespace

hipError_t launch_tw_improve(const WindowedRows& rows, hipStream_t stream) {
  // both int32 matrices of 128 stops (2 x 66.6 KB) and the per-stop / per-trip arrays
  return team::launch_two_tiers<TwImproveLds>(tw_improve_kernel<64>, tw_improve_kernel<team::kLargeTeam>, rows.R,
                                              rows.NM, stream, rows);
}

}  // namespace rt
