// K6e: window-aware local search (relocate between trips, swap, relocate inside a trip) on the trips
// K6d built for a time-window row (gfx950), opt-in per request row.
//
// The definition (fixed-point millimetres and milliseconds, the unusable-entry rule, the three move
// types with their limits and O(1) / bounded-walk time tests, best-improvement selection with the
// (type, A, i, B, j) tie rule, the f64 acceptance walks, the move cap and the skip conditions) is in
// routest_amd/routing/tw_improve.py; the host C++ is rtr::tw_improve_trips (runtime/route_core.h).
// All three are compared with ==: every quantity the search orders by is an int64 sum, so the
// schedule below cannot change it.
//
// One TEAM of threads per request row, with K6c / K6d's two tiers and their barrier discipline:
//   * small tier: rows with at most 32 stops, TEAM = one wavefront, four rows per 256-thread block;
//     only wave barriers, so a wave may leave early;
//   * large tier: rows with 33..128 stops, TEAM = one 1024-thread block; every branch around a
//     __syncthreads depends only on values all threads read from LDS (reduction results) or from the
//     same global address.
// Both tiers are launched over all rows and each row is handled by the tier its stop count picks.
//
// The row's two quantized matrices are gathered ONCE into LDS as int32 (an unusable entry is
// INT_MAX, so the narrowing is exact), as K6d does, with open / close / service / demand (int64).
// The order is K6c's flat array of stops grouped by trip in the trips' original order (a flat
// position orders like (A, i)) with the trip of every position and every trip's start / count, in
// two copies; an emptied trip keeps its index.  dep[] and z[] are kept per flat position.  Per move:
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
// go out one per thread and the waiting time by a team sum.  No global atomics, nothing waits on
// another team; every loop that holds a barrier is bounded by values the whole team holds alike.
#include <climits>

#include "common.h"
#include "ops.h"

namespace rt {

namespace {

constexpr long long kBig = 1LL << 50;
constexpr long long kUnbounded = 1LL << 62;
constexpr int kUnusable = INT_MAX;
constexpr int kMaxStops = 128;
constexpr int kSmallStops = 32;
constexpr int kLargeTeam = 1024;

__device__ __forceinline__ long long quantize_mm(double x) {
  if (!(x >= 0.0) || x >= 1099511627776.0) return kBig;  // NaN, +-inf, negatives, >= 2^40
  return __double2ll_rn(x * 1000.0);
}

// a matrix entry as the int32 the LDS holds: INT_MAX for every value >= 2^31 - 1
__device__ __forceinline__ int quantize_entry(double x) {
  const long long v = quantize_mm(x);
  return v >= (long long)kUnusable ? kUnusable : (int)v;
}

// cap_q / max_q: floor(x * 1000) below 2^40, unbounded from there; -1 for NaN and negatives
__device__ __forceinline__ long long quantize_limit(double x) {
  if (!(x >= 0.0)) return -1;
  if (x >= 1099511627776.0) return kUnbounded;
  return (long long)floor(x * 1000.0);
}

// LDS of one team, carved from the dynamic region (every offset a multiple of 16).
__host__ __device__ constexpr int twi_stride(int kc) { return (kc + 1) | 1; }
__host__ __device__ constexpr size_t ialign16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t twi_team_bytes(int kc) {
  return 2 * ialign16((size_t)(kc + 1) * twi_stride(kc) * 4)  // Q, T
         + 14 * ialign16((size_t)(kc + 4) * 8)  // open, close, sv, qd, dep, z, Lq, Wq, rem, nb, dv[2], dm[2]
         + 12 * ialign16((size_t)(kc + 4) * 4)  // ord[2], tof[2], tst[2], cnt[2], pw, pn, rank, bnd
         + 128 + 128 + 32;                      // red_g[16] | red_c[16] | misc[8]
}

template <int TEAM>
__device__ __forceinline__ void team_sync() {
  if constexpr (TEAM == 64) {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS traffic is done
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

__device__ __forceinline__ long long wave_first(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL));
  const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned int)lo;
}

// the sum of v over the team, held by every thread (red: 16 words of the team's LDS)
template <int TEAM>
__device__ __forceinline__ long long team_sum(long long v, long long* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if constexpr (TEAM != 64) {
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    v = 0;
#pragma unroll
    for (int w = 0; w < TEAM / 64; ++w) v += red[w];
    __syncthreads();
  }
  return wave_first(v);
}

// (max g, then min c) over the team, held by every thread
template <int TEAM>
__device__ __forceinline__ void team_best(long long& g, long long& c, long long* red_g, long long* red_c,
                                          int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long og = __shfl_xor(g, o);
    const long long oc = __shfl_xor(c, o);
    if (og > g || (og == g && oc < c)) {
      g = og;
      c = oc;
    }
  }
  if constexpr (TEAM != 64) {
    if ((tid & 63) == 0) {
      red_g[tid >> 6] = g;
      red_c[tid >> 6] = c;
    }
    __syncthreads();
    g = red_g[0];
    c = red_c[0];
#pragma unroll
    for (int w = 1; w < TEAM / 64; ++w) {
      const long long og = red_g[w];
      const long long oc = red_c[w];
      if (og > g || (og == g && oc < c)) {
        g = og;
        c = oc;
      }
    }
    __syncthreads();
  }
  g = wave_first(g);
  c = wave_first(c);
}

// a move as one word that orders like (type, A, i, B, j): A, B <= 127, i, j <= 128
__device__ __forceinline__ long long move_code(int type, int A, int i, int B, int j) {
  return ((long long)type << 32) | ((long long)A << 24) | ((long long)i << 16) | ((long long)B << 8) | j;
}

__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).
template <int TEAM>
__global__ __launch_bounds__(TEAM == 64 ? 256 : TEAM) void tw_improve_kernel(
    const double* __restrict__ D, const double* __restrict__ T, const int* __restrict__ npts,
    const double* __restrict__ demand, const double* __restrict__ cap, const double* __restrict__ maxd,
    const long long* __restrict__ open, const long long* __restrict__ close,
    const long long* __restrict__ service, const unsigned char* __restrict__ flag, int R, int NM, int KC,
    int* __restrict__ visit, int* __restrict__ trip_of, int* __restrict__ ntrips,
    const int* __restrict__ status, long long* __restrict__ arrival, long long* __restrict__ start,
    long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TEAMS = TEAM == 64 ? 4 : 1;
  constexpr int TEAM_SHIFT = TEAM == 64 ? 6 : 10;
  const int team = TEAM == 64 ? (int)(threadIdx.x >> 6) : 0;
  const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int r = blockIdx.x * TEAMS + team;
  if (r >= R) return;  // small tier: wave-uniform, no block barrier below; large tier: never taken
  if (flag[r] == 0 || status[r] != 0) return;  // not asked for, or not planned: nothing is touched
  int n = npts[r];
  n = n < 0 ? 0 : (n > NM ? NM : n);
  const int ns = n > 0 ? n - 1 : 0;
  const bool small_row = ns <= kSmallStops;
  if (small_row != (TEAM == 64)) return;  // the other tier's row (uniform over the team)
  if (ns == 0 || ns > kMaxStops || ns > KC) return;

  unsigned char* base = smem + (size_t)team * twi_team_bytes(KC);
  const int S = twi_stride(KC);
  const size_t mat = ialign16((size_t)(KC + 1) * S * 4);
  const size_t vec8 = ialign16((size_t)(KC + 4) * 8), vec4 = ialign16((size_t)(KC + 4) * 4);
  int* sQ = (int*)base;
  int* sT = (int*)(base + mat);
  base += 2 * mat;
  long long* s_open = (long long*)base;
  long long* s_close = (long long*)(base + vec8);
  long long* s_sv = (long long*)(base + 2 * vec8);
  long long* s_qd = (long long*)(base + 3 * vec8);
  long long* s_dep = (long long*)(base + 4 * vec8);  // per flat position: the departure of its stop
  long long* s_z = (long long*)(base + 5 * vec8);    // per flat position: the latest start of its stop
  long long* s_Lq = (long long*)(base + 6 * vec8);   // per trip
  long long* s_Wq = (long long*)(base + 7 * vec8);
  long long* s_rem = (long long*)(base + 8 * vec8);  // per flat position
  long long* s_nb = (long long*)(base + 9 * vec8);
  double* s_dv = (double*)(base + 10 * vec8);        // [2][KC + 4]: a touched trip's legs
  double* s_dm = (double*)(base + 12 * vec8);        // [2][KC + 4]: ... and its stops' demands
  base += 14 * vec8;
  int* s_ord = (int*)base;                           // [2][KC + 4]: the order and its moved copy
  int* s_tof = (int*)(base + 2 * vec4);              // [2][KC + 4]
  int* s_tst = (int*)(base + 4 * vec4);              // [2][KC + 4]
  int* s_cnt = (int*)(base + 6 * vec4);              // [2][KC + 4]
  unsigned* s_pw = (unsigned*)(base + 8 * vec4);     // s | A << 8 | i << 16 | may-leave << 25 | may-shift << 26
  unsigned* s_pn = (unsigned*)(base + 9 * vec4);     // prev | next << 8
  int* s_rank = (int*)(base + 10 * vec4);
  int* s_bnd = (int*)(base + 11 * vec4);
  base += 12 * vec4;
  long long* s_redg = (long long*)base;
  long long* s_redc = (long long*)(base + 128);
  int* s_misc = (int*)(base + 256);  // [0], [1]: the two walks' verdicts
  const int V4 = (int)(vec4 / 4), V8 = (int)(vec8 / 8);

  const double* d = D + (size_t)r * NM * NM;
  const double* t = T + (size_t)r * NM * NM;
  const double* dem = demand + (size_t)r * NM;
  const long long* op = open + (size_t)r * NM;
  const long long* cl = close + (size_t)r * NM;
  const long long* sv = service + (size_t)r * NM;
  int* vrow = visit + (size_t)r * NM;
  int* trow = trip_of + (size_t)r * NM;
  long long* arow = arrival + (size_t)r * NM;
  long long* strow = start + (size_t)r * NM;
  long long* srow = stats + (size_t)r * 7;
  const double MD = maxd[r], CAP = cap[r];
  const long long cap_q = quantize_limit(CAP), max_q = quantize_limit(MD);

  // ---- the row as K6d left it, from global memory: its trips, its waiting time, its validity
  long long groups = 0, wait0 = 0, badv = 0;
  for (int p = tid; p < ns; p += TEAM) {
    const int v = vrow[p];
    badv += (v < 1 || v >= n) ? 1 : 0;
    groups += (p == 0 || trow[p] != trow[p - 1]) ? 1 : 0;
    wait0 += strow[p] - arow[p];
  }
  const int m = (int)team_sum<TEAM>(groups, s_redg, tid);
  wait0 = team_sum<TEAM>(wait0, s_redg, tid);
  if (team_sum<TEAM>(badv, s_redg, tid) != 0) return;  // not K6d's output: leave the row alone

  // ---- gather: both quantized matrices, the per-stop vectors, the order, the trips
  for (int c = tid; c < n * n; c += TEAM) {
    const int a = c / n, b = c - a * n;
    sQ[a * S + b] = quantize_entry(d[(size_t)a * NM + b]);
    sT[a * S + b] = quantize_entry(t[(size_t)a * NM + b]);
  }
  long long bigdem = 0;
  for (int s = tid; s < n; s += TEAM) {
    s_open[s] = s == 0 ? 0 : op[s];
    s_close[s] = s == 0 ? kUnbounded : cl[s];
    s_sv[s] = s == 0 ? 0 : sv[s];
    const long long qd = s == 0 ? 0 : quantize_mm(dem[s]);
    s_qd[s] = qd;
    bigdem += qd == kBig ? 1 : 0;
  }
  for (int p = tid; p < ns; p += TEAM) {
    s_ord[p] = vrow[p];
    s_bnd[p] = p > 0 && trow[p] != trow[p - 1];
  }
  team_sync<TEAM>();
  for (int p = tid; p < ns; p += TEAM) {
    int x = 0;
    for (int y = 1; y <= p; ++y) x += s_bnd[y];
    s_tof[p] = x;
    if (p == 0 || s_bnd[p]) s_tst[x] = p;
  }
  team_sync<TEAM>();
  for (int p = tid; p < ns; p += TEAM)
    if (p + 1 == ns || s_bnd[p + 1]) s_cnt[s_tof[p]] = p + 1 - s_tst[s_tof[p]];
  team_sync<TEAM>();
  long long part = 0;
  for (int x = tid; x < m; x += TEAM) {
    const int st = s_tst[x], c = s_cnt[x];
    long long L = 0, W = 0;
    int a = 0;
    for (int y = 0; y < c; ++y) {
      const int b = s_ord[st + y];
      L += sQ[a * S + b];
      W += s_qd[b];
      a = b;
    }
    L += sQ[a * S];
    s_Lq[x] = L;
    s_Wq[x] = W;
    part += L;
  }
  const long long before = team_sum<TEAM>(part, s_redg, tid);
  bigdem = team_sum<TEAM>(bigdem, s_redg, tid);
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
  int sh = 32 - __builtin_clz(ncols - 1);  // 2^sh >= ncols (ncols >= 3)
  sh = sh > TEAM_SHIFT ? TEAM_SHIFT : sh;
  const int CW = 1 << sh;
  const int col0 = tid & (CW - 1), row0 = tid >> sh, rstep = TEAM >> sh;
  const int limit = 4 * ns;
  int cur = 0, moves = 0, rejected = 0;
  while (moves < limit) {
    team_sync<TEAM>();
    int* ord = s_ord + cur * V4;
    int* tof = s_tof + cur * V4;
    int* tst = s_tst + cur * V4;
    int* cnt = s_cnt + cur * V4;
    // 0. dep forwards and z backwards, one lane per trip
    for (int x = tid; x < m; x += TEAM) {
      const int st = tst[x], c = cnt[x];
      if (c > 0) {
        long long dp = 0;
        int a = 0;
        for (int y = 0; y < c; ++y) {
          const int b = ord[st + y];
          dp = max64(dp + sT[a * S + b], s_open[b]) + s_sv[b];
          s_dep[st + y] = dp;
          a = b;
        }
        long long zz = s_close[a];
        s_z[st + c - 1] = zz;
        for (int y = c - 2; y >= 0; --y) {
          const int b = ord[st + y];
          const long long v = zz - sT[b * S + a] - s_sv[b];
          zz = s_close[b] < v ? s_close[b] : v;
          s_z[st + y] = zz;
          a = b;
        }
      }
    }
    team_sync<TEAM>();
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
    team_sync<TEAM>();

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
    team_best<TEAM>(bg, bc, s_redg, s_redc, tid);
    if (bg <= 0) break;

    // the move, its effect on the touched trips' Lq / Wq, and the moved order in the other copy
    const int mt = (int)(bc >> 32), mA = (int)(bc >> 24) & 255, mi = (int)(bc >> 16) & 255;
    const int mB = (int)(bc >> 8) & 255, mj = (int)bc & 255;
    const int nxt = cur ^ 1;
    int* nord = s_ord + nxt * V4;
    int* ntof = s_tof + nxt * V4;
    int* ntst = s_tst + nxt * V4;
    int* ncnt = s_cnt + nxt * V4;
    const int pA = tst[mA] + mi - 1;
    const int sA = ord[pA];
    long long dLA, dLB, dWA, dWB;
    if (mt != 1) {
      const int u = mj == 0 ? 0 : ord[tst[mB] + mj - 1];
      const int v = mj == cnt[mB] ? 0 : ord[tst[mB] + mj];
      if (mt == 0) {
        dLA = -s_rem[pA];
        dLB = (long long)sQ[u * S + sA] + sQ[sA * S + v] - sQ[u * S + v];
        dWA = -s_qd[sA];
        dWB = s_qd[sA];
      } else {  // one trip: its length drops by the gain
        dLA = -bg;
        dLB = dWA = dWB = 0;
      }
      // the target behind the source: the stops between move one place to the front; else one back
      const bool fwd = mB > mA || (mB == mA && mj > mi);
      const int dst = fwd ? tst[mB] + mj - 1 : tst[mB] + mj;
      for (int p = tid; p < ns; p += TEAM) {
        int src = p;
        if (fwd) {
          if (p >= pA && p < dst) src = p + 1;
        } else {
          if (p > dst && p <= pA) src = p - 1;
        }
        nord[p] = p == dst ? sA : ord[src];
        ntof[p] = p == dst ? mB : tof[src];
      }
      for (int x = tid; x < m; x += TEAM) {
        int st = tst[x];
        if (mB > mA) {
          if (x > mA && x <= mB) --st;
        } else {
          if (x > mB && x <= mA) ++st;
        }
        ntst[x] = st;
        ncnt[x] = cnt[x] + (x == mB) - (x == mA);
      }
    } else {
      const int pB = tst[mB] + mj - 1;
      const int sB = ord[pB];
      const unsigned pna = s_pn[pA], pnb = s_pn[pB];
      dLA = (long long)sQ[(pna & 255) * S + sB] + sQ[sB * S + ((pna >> 8) & 255)] - s_nb[pA];
      dLB = (long long)sQ[(pnb & 255) * S + sA] + sQ[sA * S + ((pnb >> 8) & 255)] - s_nb[pB];
      dWA = s_qd[sB] - s_qd[sA];
      dWB = -dWA;
      for (int p = tid; p < ns; p += TEAM) {
        nord[p] = p == pA ? sB : (p == pB ? sA : ord[p]);
        ntof[p] = tof[p];
      }
      for (int x = tid; x < m; x += TEAM) {
        ntst[x] = tst[x];
        ncnt[x] = cnt[x];
      }
    }
    team_sync<TEAM>();

    // 4. acceptance as the greedy measures it: the touched non-empty trips, f64, in visiting order
    const int walks = mt == 2 ? 1 : 2;
    for (int x = 0; x < walks; ++x) {
      const int tr = x == 0 ? mA : mB;
      const int st = ntst[tr], c = ncnt[tr];
      if (c == 0) continue;
      for (int e = tid; e <= c; e += TEAM) {
        const int a = e == 0 ? 0 : nord[st + e - 1];
        const int b = e == c ? 0 : nord[st + e];
        s_dv[x * V8 + e] = d[(size_t)a * NM + b];
        if (e < c) s_dm[x * V8 + e] = dem[b];
      }
    }
    team_sync<TEAM>();
    if (tid < 2) {
      const int c = tid < walks ? ncnt[tid == 0 ? mA : mB] : 0;
      int ok = 1;
      if (c > 0) {
        const double* dv = s_dv + tid * V8;
        const double* dm = s_dm + tid * V8;
        double s = 0.0, load = 0.0;
        for (int p = 0; p < c; ++p) {
          s += dv[p];
          load += dm[p];
        }
        ok = (s + dv[c] <= MD && load <= CAP) ? 1 : 0;
      }
      s_misc[tid] = ok;
    }
    team_sync<TEAM>();
    if (!(s_misc[0] != 0 && s_misc[1] != 0)) {  // undone: the first copy stays, the search ends
      rejected = 1;
      break;
    }
    if (tid == 0) {
      s_Lq[mA] += dLA;
      s_Wq[mA] += dWA;
      if (mt != 2) {
        s_Lq[mB] += dLB;
        s_Wq[mB] += dWB;
      }
    }
    cur = nxt;
    ++moves;
  }
  team_sync<TEAM>();

  // ---- the non-empty trips, compacted in their order, with their schedule
  const int* ord = s_ord + cur * V4;
  const int* tof = s_tof + cur * V4;
  const int* tst = s_tst + cur * V4;
  const int* cnt = s_cnt + cur * V4;
  if (tid == 0) {
    int k = 0;
    long long after = 0;
    for (int x = 0; x < m; ++x) {
      s_rank[x] = k;
      if (cnt[x] > 0) {
        ++k;
        after += s_Lq[x];
      }
    }
    ntrips[r] = k;
    srow[0] = moves;
    srow[1] = rejected;
    srow[2] = m;
    srow[3] = k;
    srow[4] = before;
    srow[5] = after;
  }
  // one lane per trip walks its schedule: arrivals into z[], starts into dep[] (no longer needed)
  for (int x = tid; x < m; x += TEAM) {
    const int st = tst[x], c = cnt[x];
    long long dp = 0;
    int a = 0;
    for (int y = 0; y < c; ++y) {
      const int b = ord[st + y];
      const long long ar = dp + sT[a * S + b];
      const long long stt = max64(ar, s_open[b]);
      s_z[st + y] = ar;
      s_dep[st + y] = stt;
      dp = stt + s_sv[b];
      a = b;
    }
  }
  team_sync<TEAM>();
  long long wait_part = 0;
  for (int p = tid; p < ns; p += TEAM) {
    vrow[p] = ord[p];
    trow[p] = s_rank[tof[p]];
    arow[p] = s_z[p];
    strow[p] = s_dep[p];
    wait_part += s_dep[p] - s_z[p];
  }
  const long long waiting = team_sum<TEAM>(wait_part, s_redg, tid);
  if (tid == 0) srow[6] = waiting;
}

}  // namespace

hipError_t launch_tw_improve(const double* D, const double* T, const int* npts, const double* demand,
                             const double* cap, const double* maxd, const long long* open,
                             const long long* close, const long long* service, const unsigned char* flag,
                             int R, int NM, int* visit, int* trip_of, int* ntrips, const int* status,
                             long long* arrival, long long* start, long long* stats, hipStream_t stream) {
  if (R == 0) return hipSuccess;
  if (NM < 1 || NM > 4096) return hipErrorInvalidValue;
  static_assert(twi_team_bytes(kMaxStops) <= 160 * 1024, "a row's LDS must fit a CU");
  static_assert(4 * twi_team_bytes(kSmallStops) <= 64 * 1024, "the small tier stays in the default LDS size");
  // small tier: rows of at most 32 stops, a wavefront each
  {
    const int kc = NM - 1 < kSmallStops ? (NM - 1 < 1 ? 1 : NM - 1) : kSmallStops;
    const size_t lds = 4 * twi_team_bytes(kc);
    hipLaunchKernelGGL(tw_improve_kernel<64>, dim3((R + 3) / 4), dim3(256), lds, stream, D, T, npts, demand,
                       cap, maxd, open, close, service, flag, R, NM, kc, visit, trip_of, ntrips, status,
                       arrival, start, stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (NM - 1 <= kSmallStops) return hipSuccess;
  // large tier: a 1024-thread workgroup each; both int32 matrices of 128 stops (2 x 66.6 KB) and the
  // per-stop / per-trip arrays need the opt-in LDS size
  const int kc = NM - 1 < kMaxStops ? NM - 1 : kMaxStops;
  const size_t lds = twi_team_bytes(kc);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)tw_improve_kernel<kLargeTeam>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tw_improve_kernel<kLargeTeam>, dim3(R), dim3(kLargeTeam), lds, stream, D, T, npts,
                     demand, cap, maxd, open, close, service, flag, R, NM, kc, visit, trip_of, ntrips,
                     status, arrival, start, stats);
  return hipGetLastError();
}

}  // namespace rt
