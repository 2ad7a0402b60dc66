// K6b: intra-trip 2-opt / Or-opt improvement of K6's greedy trips (gfx950), opt-in per request.
//
// The definition (fixed-point millimetres, move types, best-improvement selection with the
// (type, i, j) tie rule, the 4k move cap, the 128-stop limit and the f64 feasibility walk) is in
// routest_amd/routing/improve.py; the host C++ is rtr::improve_trips (runtime/route_core.h).  All
// three are compared with ==: every gain is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row (teams, tiers and the barrier discipline: route_team.h), the
// row's trips one after the other; each tier also zeroes the statistics of its rows that do not ask.
//
// Per trip of k stops (2 <= k <= 128): the (k+1)^2 sub-matrix is gathered ONCE into LDS, quantized,
// indexed by trip-local stop number (0 = depot, a = a-th stop of the greedy); the order lives in
// LDS as local numbers.  Per move:
//   1. f[p] = q(t[p], t[p+1]) and b[p] = q(t[p+1], t[p]) for every position;
//   2. their prefix sums pf / pb and, per row i, what the gains of the row share: the reversal's
//      c0[i] = pb[i] - pf[i-1], the Or-opt's rem[len][i] = f[i-1] + f[e] - q(t[i-1], t[e+1]), and
//      the window t[i-1..i+2] packed into one word;
//   3. the candidate scan: a lane owns one insertion point / reversal end j and strides over the
//      rows i (JW = the power of two >= k + 1 lanes per row, so no division); per row it prices
//      the four moves (type 0..3) from the row's shared terms and five matrix entries:
//        reversal: (pf[j+1] - pb[j]) + c0[i] - q(t[i-1], t[j]) - q(t[i], t[j+1])
//        Or-opt:   rem[len][i] + f[j] - q(t[j], t[i]) - q(t[e], t[j+1])
//      and keeps (max gain, then min (type, i, j));
//   4. the team reduces (max gain, then min (type, i, j)); everyone applies the move to the LDS
//      order, one element per thread.
#include "ops.h"
#include "route_team.h"

namespace rt {

namespace {

using namespace team;

constexpr long long kNever = -(1LL << 62);  // a row term that keeps a gain below 0 whatever is added

// LDS of one team (offsets in bytes), for a stop capacity of kc
struct ImproveLds {
  size_t Q = 0, f = 0, b = 0, pf = 0, pb = 0, row = 0, dv = 0, node = 0, ord = 0, win = 0, redg = 0, redc = 0,
         misc = 0, bytes = 0;
  __host__ __device__ constexpr explicit ImproveLds(int kc) {
    LdsCarve c;
    Q = c.take(8, (size_t)(kc + 1) * matrix_stride(kc));
    f = c.take(8, kc + 2);
    b = c.take(8, kc + 2);
    pf = c.take(8, kc + 2);
    pb = c.take(8, kc + 2);
    row = c.take(8, kc + 2, 4);  // [kc + 2][4]: c0, rem[1], rem[2], rem[3]
    dv = c.take(8, kc + 2);
    node = c.take(4, kc + 2);
    ord = c.take(4, kc + 2);
    win = c.take(4, kc + 2);     // t[i-1] | t[i] << 8 | t[i+1] << 16 | t[i+2] << 24
    redg = c.take(8, 16);
    redc = c.take(4, 16);
    misc = c.take(4, 4);         // [0] end of the trip, [1] bad stop number, [2] keep
    bytes = c.bytes;
  }
};
static_assert(ImproveLds(32).bytes == 11808 && ImproveLds(128).bytes == 144288, "the layout is fixed");

// a move as one int that orders like (type, i, j): i, j <= 128
__device__ __forceinline__ int move_code(int type, int i, int j) { return (type << 16) | (i << 8) | j; }

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).  It must stay the
// first parameter: launch_two_tiers passes it there, in front of the launch's own arguments.
template <int TEAM>
__global__ __launch_bounds__(Team<TEAM>::BLOCK) void improve_trips_kernel(
    int KC, const double* __restrict__ D, const int* __restrict__ npts, const double* __restrict__ maxd,
    const unsigned char* __restrict__ flag, const int* __restrict__ status, int R, int NM,
    int* __restrict__ visit, const int* __restrict__ trip_of, int* __restrict__ moves_out,
    int* __restrict__ changed_out, long long* __restrict__ before_out,
    long long* __restrict__ after_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Tm = Team<TEAM>;
  const Row rw = Tm::row(npts, R, NM);
  if (!rw.mine) return;
  const int tid = rw.tid, r = rw.r, n = rw.n, ns = rw.ns;
  const bool asks = flag[r] != 0 && status[r] == 0;
  if (!asks || ns == 0) {
    if (tid == 0) {
      moves_out[r] = 0;
      changed_out[r] = 0;
      before_out[r] = 0;
      after_out[r] = 0;
    }
    return;
  }

  const ImproveLds L(KC);
  unsigned char* base = smem + (size_t)rw.team * L.bytes;
  const int S = matrix_stride(KC);
  long long* sQ = (long long*)(base + L.Q);
  long long* s_f = (long long*)(base + L.f);
  long long* s_b = (long long*)(base + L.b);
  long long* s_pf = (long long*)(base + L.pf);
  long long* s_pb = (long long*)(base + L.pb);
  long long* s_row = (long long*)(base + L.row);
  double* s_dv = (double*)(base + L.dv);
  int* s_node = (int*)(base + L.node);
  int* s_ord = (int*)(base + L.ord);
  unsigned* s_win = (unsigned*)(base + L.win);
  long long* s_redg = (long long*)(base + L.redg);
  int* s_redc = (int*)(base + L.redc);
  int* s_misc = (int*)(base + L.misc);

  const double* d = D + (size_t)r * NM * NM;
  int* vrow = visit + (size_t)r * NM;
  const int* trow = trip_of + (size_t)r * NM;
  const double MD = maxd[r];

  int tot_moves = 0, tot_changed = 0;
  long long tot_before = 0, tot_after = 0;

  if (tid == 0) s_misc[1] = 0;  // only a bad trip sets it, and that ends the row: cleared once
  int pos = 0;
  while (pos < ns) {
    // ---- the trip's extent: the first position whose successor belongs to another trip
    const int tr = trow[pos];
    if (tid == 0) s_misc[0] = ns;
    Tm::sync();
    for (int p = pos + tid; p < ns; p += TEAM)
      if (trow[p] == tr && (p + 1 == ns || trow[p + 1] != tr)) atomicMin(&s_misc[0], p + 1);
    Tm::sync();
    const int end = s_misc[0];
    const int k = end - pos;  // >= 1
    Tm::sync();

    // ---- the greedy's length of the trip, from global memory (any k)
    long long part = 0;
    bool bad = false;
    for (int p = tid; p <= k; p += TEAM) {
      const int a = p == 0 ? 0 : vrow[pos + p - 1];
      const int b = p == k ? 0 : vrow[pos + p];
      if (a < 0 || a >= n || b < 0 || b >= n) {
        bad = true;
      } else {
        part += quantize_mm(d[(size_t)a * NM + b]);
      }
    }
    // the large tier's flag rides on the sum's barriers: set before its first, read behind its last.
    // Nothing clears it again, and the next trip can set it only behind that trip's three barriers.
    if constexpr (TEAM == 64) {
      bad = __ballot(bad) != 0ULL;
    } else if (bad) {
      s_misc[1] = 1;
    }
    const long long before = Tm::sum(part, s_redg, tid);
    if constexpr (TEAM != 64) bad = s_misc[1] != 0;
    if (bad) break;  // a stop number outside the row: not K6's output, leave the rest alone
    tot_before += before;
    if (k < 2 || k > kMaxStops || k > KC) {
      tot_after += before;
      pos = end;
      continue;
    }

    // ---- gather: local stop numbers, the order, the quantized sub-matrix
    for (int a = tid; a <= k; a += TEAM) {
      s_node[a] = a == 0 ? 0 : vrow[pos + a - 1];
      s_ord[a] = a;
    }
    if (tid == 0) s_ord[k + 1] = 0;
    Tm::sync();
    const int k1 = k + 1;
    for (int c = tid; c < k1 * k1; c += TEAM) {
      const int a = c / k1, b = c - a * k1;
      sQ[a * S + b] = quantize_mm(d[(size_t)s_node[a] * NM + s_node[b]]);
    }
    Tm::sync();

    // ---- best-improvement search
    // a lane's insertion point / reversal end j and its first row; 2^sh >= k + 1 lanes per row
    const Lanes ln = Tm::split(k + 1, tid);
    const int j = ln.col0, i0 = 1 + ln.row0, istep = ln.rstep;
    int moves = 0;
    long long after = before;
    for (;;) {
      for (int p = tid; p <= k; p += TEAM) {
        const int a = s_ord[p], b = s_ord[p + 1];
        s_f[p] = sQ[a * S + b];
        s_b[p] = sQ[b * S + a];
      }
      Tm::sync();
      // prefix sums over positions: pf[p] = sum_{x < p} f[x]; the segment part of the Or-opt gains
      for (int p = tid; p <= k + 1; p += TEAM) {
        long long f = 0, b = 0;
#pragma unroll 8
        for (int x = 0; x < p; ++x) {
          f += s_f[x];
          b += s_b[x];
        }
        s_pf[p] = f;
        s_pb[p] = b;
        if (p >= 1) s_row[p * 4] = b - (f - s_f[p - 1]);  // c0[p] = pb[p] - pf[p-1]
      }
      for (int i = 1 + (TEAM >= 512 ? tid - 512 : tid); i >= 1 && i <= k; i += TEAM) {
        const int tp = s_ord[i - 1], ti = s_ord[i], t1 = s_ord[i + 1];
        const int t2 = i + 2 <= k + 1 ? s_ord[i + 2] : 0, t3 = i + 3 <= k + 1 ? s_ord[i + 3] : 0;
        s_win[i] = (unsigned)tp | ((unsigned)ti << 8) | ((unsigned)t1 << 16) | ((unsigned)t2 << 24);
        const long long fp = s_f[i - 1];
        const long long* qp = sQ + tp * S;
        // a segment that would run past the last stop can never win
        s_row[i * 4 + 1] = fp + s_f[i] - qp[t1];
        s_row[i * 4 + 2] = i + 1 <= k ? fp + s_f[i + 1] - qp[t2] : kNever;
        s_row[i * 4 + 3] = i + 2 <= k ? fp + s_f[i + 2] - qp[t3] : kNever;
      }
      Tm::sync();
      after = s_pf[k + 1];
      if (moves >= 4 * k) break;

      long long bg = 0;
      int bc = INT_MAX;
      if (j <= k) {
        const int tj = s_ord[j], tj1 = s_ord[j + 1];
        const long long aj = s_pf[j + 1] - s_pb[j];
        const long long fj = s_f[j];
        const long long* qj = sQ + tj * S;
        auto take = [&](long long g, int code) {
          if (g > bg || (g == bg && code < bc)) {
            bg = g;
            bc = code;
          }
        };
        for (int i = i0; i <= k; i += istep) {
          const unsigned w = s_win[i];
          const int tp = w & 255, ti = (w >> 8) & 255, t1 = (w >> 16) & 255, t2 = w >> 24;
          const long long* row = s_row + i * 4;
          const long long q_i_j1 = sQ[ti * S + tj1];
          // reversal of t[i..j]
          if (i < j) take(aj + row[0] - sQ[tp * S + tj] - q_i_j1, move_code(0, i, j));
          // Or-opt of t[i..e] to between t[j] and t[j+1], j outside i-1..e
          const long long ins = fj - qj[ti];
          const bool front = j < i - 1;
          if (front || j > i) take(row[1] + ins - q_i_j1, move_code(1, i, j));
          if (front || j > i + 1) take(row[2] + ins - sQ[t1 * S + tj1], move_code(2, i, j));
          if (front || j > i + 2) take(row[3] + ins - sQ[t2 * S + tj1], move_code(3, i, j));
        }
      }
      // (max gain, then min move code) over the team
      Tm::best(bg, bc, s_redg, s_redc, tid);
      if (bg <= 0) break;

      // ---- apply: every thread moves at most one element of the order
      const int mt = bc >> 16, mi = (bc >> 8) & 255, mj = bc & 255;
      int lo, hi, src;
      if (mt == 0) {
        lo = mi;
        hi = mj;
        src = mj - tid;  // position p = lo + tid takes t[i + j - p]
      } else {
        const int e = mi + mt - 1;
        if (mj < mi - 1) {  // towards the front: segment lands at j+1.., the stops between shift back
          lo = mj + 1;
          hi = e;
          const int p = lo + tid;
          src = p <= mj + mt ? mi + (p - mj - 1) : p - mt;
        } else {            // towards the back: the stops between shift forward, segment ends at j
          lo = mi;
          hi = mj;
          const int p = lo + tid;
          src = p <= mj - mt ? p + mt : mi + (p - (mj - mt + 1));
        }
      }
      const int p = lo + tid;
      int val = 0;
      if (p <= hi) val = s_ord[src];
      Tm::sync();
      if (p <= hi) s_ord[p] = val;
      Tm::sync();
      ++moves;
    }

    // ---- feasibility as the greedy measures it: f64 walk in order, one lane adds
    bool keep = false;
    if (moves > 0) {
      for (int p = tid; p <= k; p += TEAM)
        s_dv[p] = d[(size_t)s_node[s_ord[p]] * NM + s_node[s_ord[p + 1]]];
      Tm::sync();
      if (tid == 0) {
        double s = 0.0;
        for (int p = 0; p < k; ++p) s += s_dv[p];
        s_misc[2] = (s + s_dv[k]) <= MD ? 1 : 0;
      }
      Tm::sync();
      keep = s_misc[2] != 0;
    }
    if (keep) {
      for (int p = 1 + tid; p <= k; p += TEAM) vrow[pos + p - 1] = s_node[s_ord[p]];
      tot_moves += moves;
      ++tot_changed;
      tot_after += after;
    } else {
      tot_after += before;
    }
    Tm::sync();
    pos = end;
  }
  if (tid == 0) {
    moves_out[r] = tot_moves;
    changed_out[r] = tot_changed;
    before_out[r] = tot_before;
    after_out[r] = tot_after;
  }
}

}  // namespace

hipError_t launch_improve_trips(const double* D, const int* npts, const double* maxd,
                                const unsigned char* flag, const int* status, int R, int NM,
                                int* visit, const int* trip_of, int* moves, int* trips_changed,
                                long long* len_before_q, long long* len_after_q,
                                hipStream_t stream) {
  // up to 141 KB of LDS per large row (k = 128)
  return team::launch_two_tiers<ImproveLds>(improve_trips_kernel<64>, improve_trips_kernel<team::kLargeTeam>,
                                            R, NM, stream, D, npts, maxd, flag, status, R, NM, visit,
                                            trip_of, moves, trips_changed, len_before_q, len_after_q);
}

}  // namespace rt
