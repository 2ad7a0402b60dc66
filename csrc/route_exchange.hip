// K6c: inter-trip relocate / swap improvement of K6's greedy trips (gfx950), opt-in per request.
//
// The definition (fixed-point millimetres, the two move types and their admissibility tests,
// best-improvement selection with the (type, A, i, B, j) tie rule, the f64 acceptance walks, the
// move cap, the 128-stop limit and the skip conditions) is in routest_amd/routing/exchange.py; the
// host C++ is rtr::exchange_trips (runtime/route_core.h).  All three are compared with ==: every
// gain is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row, with K6b's two tiers and its barrier discipline:
//   * small tier: rows with at most 32 stops, TEAM = one wavefront, four rows per 256-thread block;
//     only wave barriers, so a wave may leave early;
//   * large tier: rows with more stops, TEAM = one 1024-thread block; every branch around a
//     __syncthreads depends only on values all threads read from LDS or from the same address.
// Both tiers are launched over all rows and each row is handled by the tier its stop count picks
// (rows above 128 stops by the large tier, which only measures them).
//
// The row's whole quantized matrix is gathered ONCE into LDS.  The order is a flat array of stops
// grouped by trip in the trips' original order (so a flat position orders like (A, i)), with the
// trip of every position and every trip's start / count; an emptied trip keeps its index.  Per move:
//   1. per position p (stop s, trip A, index i, neighbours prev / next):
//      nb[p] = q(prev,s) + q(s,next), rem[p] = nb[p] - q(prev,next), whether A may lose s
//      (Lq[A] - rem <= max_q), and the insertion edge in front of s; per trip its closing edge;
//   2. the candidate scan: a lane owns one column, an insertion edge (relocate) or a partner
//      position (swap), and strides over the positions p (a power of two of lanes per row of
//      candidates, so no division); a relocate is priced from rem[p], the edge's base and two
//      matrix reads, a swap from four reads and the two nb terms; the lane keeps (max gain, then
//      min move code), the code packing (type, A, i, B, j);
//   3. the team reduces (max gain, then min code); everyone writes the moved order into the second
//      copy of the order arrays, one position per thread;
//   4. acceptance as the greedy measures it: the two touched trips' f64 entries and demands are
//      staged into LDS in parallel and one lane per trip adds them in order (the only place where
//      float association matters); accepted: the copies change roles, Lq / Wq take the move's
//      deltas; rejected: the first copy stays and the search ends.
// At the end the non-empty trips are compacted into visit / trip_of / ntrips.
// The per-lane loops of step 2 hold no barrier and no cross-lane operation; every loop that does is
// bounded by values the whole team holds.  No global atomics, nothing waits on another team.
#include <climits>

#include "common.h"
#include "ops.h"

namespace rt {

namespace {

constexpr long long kBig = 1LL << 50;
constexpr long long kUnbounded = 1LL << 62;
constexpr int kMaxStops = 128;
constexpr int kSmallStops = 32;
constexpr int kLargeTeam = 1024;
constexpr unsigned kNoEdge = 255;  // an insertion edge of an emptied trip: never a target

__device__ __forceinline__ long long quantize_mm(double x) {
  if (!(x >= 0.0) || x >= 1099511627776.0) return kBig;  // NaN, +-inf, negatives, >= 2^40
  return __double2ll_rn(x * 1000.0);
}

// cap_q / max_q: floor(x * 1000) below 2^40, unbounded from there; -1 for NaN and negatives
__device__ __forceinline__ long long quantize_limit(double x) {
  if (!(x >= 0.0)) return -1;
  if (x >= 1099511627776.0) return kUnbounded;
  return (long long)floor(x * 1000.0);
}

// LDS of one team, carved from the dynamic region (every offset a multiple of 16).
__host__ __device__ constexpr int exchange_stride(int kc) { return (kc + 1) | 1; }
__host__ __device__ constexpr size_t xalign16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t exchange_team_bytes(int kc) {
  return xalign16((size_t)(kc + 1) * exchange_stride(kc) * 8)  // Q
         + 11 * xalign16((size_t)(kc + 2) * 8)  // nb, rem, qd, Lq, Wq, ebase[2], dv[2], dm[2]
         + 14 * xalign16((size_t)(kc + 2) * 4)  // ord[2], tof[2], tst[2], cnt[2], pw, pn, edge[2], rank, bnd
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

// a move as one word that orders like (type, A, i, B, j): A, B <= 127, i, j <= 128
__device__ __forceinline__ long long move_code(int type, int A, int i, int B, int j) {
  return ((long long)type << 32) | ((long long)A << 24) | ((long long)i << 16) | ((long long)B << 8) | j;
}

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).
template <int TEAM>
__global__ __launch_bounds__(TEAM == 64 ? 256 : TEAM) void exchange_trips_kernel(
    const double* __restrict__ D, const int* __restrict__ npts, const double* __restrict__ demand,
    const double* __restrict__ cap, const double* __restrict__ maxd,
    const unsigned char* __restrict__ flag, const int* __restrict__ status, int R, int NM, int KC,
    int move_cap, int* __restrict__ visit, int* __restrict__ trip_of, int* __restrict__ ntrips,
    int* __restrict__ moves_out, int* __restrict__ rejected_out, int* __restrict__ tbefore_out,
    int* __restrict__ tafter_out, long long* __restrict__ before_out,
    long long* __restrict__ after_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TEAMS = TEAM == 64 ? 4 : 1;
  constexpr int WAVES = TEAM / 64;
  constexpr int TEAM_SHIFT = TEAM == 64 ? 6 : 10;
  const int team = TEAM == 64 ? (int)(threadIdx.x >> 6) : 0;
  const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int r = blockIdx.x * TEAMS + team;
  if (r >= R) return;  // small tier: wave-uniform, no block barrier below; large tier: never taken
  int n = npts[r];
  n = n < 0 ? 0 : (n > NM ? NM : n);
  const int ns = n > 0 ? n - 1 : 0;
  const bool small_row = ns <= kSmallStops;
  if (small_row != (TEAM == 64)) return;  // the other tier's row (uniform over the team)

  auto put_stats = [&](int mv, int rej, int tb, int ta, long long lb, long long la) {
    if (tid == 0) {
      moves_out[r] = mv;
      rejected_out[r] = rej;
      tbefore_out[r] = tb;
      tafter_out[r] = ta;
      before_out[r] = lb;
      after_out[r] = la;
    }
  };
  const bool asks = flag[r] != 0 && status[r] == 0;
  if (!asks || ns == 0) {
    put_stats(0, 0, 0, 0, 0, 0);
    return;
  }

  unsigned char* base = smem + (size_t)team * exchange_team_bytes(KC);
  const int S = exchange_stride(KC);
  const size_t vec8 = xalign16((size_t)(KC + 2) * 8), vec4 = xalign16((size_t)(KC + 2) * 4);
  long long* sQ = (long long*)base;
  base += xalign16((size_t)(KC + 1) * S * 8);
  long long* s_nb = (long long*)base;
  long long* s_rem = (long long*)(base + vec8);
  long long* s_qd = (long long*)(base + 2 * vec8);
  long long* s_Lq = (long long*)(base + 3 * vec8);
  long long* s_Wq = (long long*)(base + 4 * vec8);
  long long* s_ebase = (long long*)(base + 5 * vec8);  // [2 * (KC + 2)]: at most ns + m <= 2 KC edges
  double* s_dv = (double*)(base + 7 * vec8);           // [2][KC + 2]
  double* s_dm = (double*)(base + 9 * vec8);           // [2][KC + 2]
  base += 11 * vec8;
  int* s_ord = (int*)base;                             // [2][KC + 2]: the order and its moved copy
  int* s_tof = (int*)(base + 2 * vec4);                // [2][KC + 2]
  int* s_tst = (int*)(base + 4 * vec4);                // [2][KC + 2]
  int* s_cnt = (int*)(base + 6 * vec4);                // [2][KC + 2]
  unsigned* s_pw = (unsigned*)(base + 8 * vec4);       // s | A << 8 | i << 16 | may-leave << 25
  unsigned* s_pn = (unsigned*)(base + 9 * vec4);       // prev | next << 8
  unsigned* s_edge = (unsigned*)(base + 10 * vec4);    // [2 * (KC + 2)]: u | v << 8 | B << 16 | j << 24
  int* s_rank = (int*)(base + 12 * vec4);
  int* s_bnd = (int*)(base + 13 * vec4);
  base += 14 * vec4;
  long long* s_redg = (long long*)base;
  long long* s_redc = (long long*)(base + 128);
  int* s_misc = (int*)(base + 256);  // [0], [1]: the two walks' verdicts
  const int V4 = (int)(vec4 / 4), V8 = (int)(vec8 / 8);

  const double* d = D + (size_t)r * NM * NM;
  const double* dem = demand + (size_t)r * NM;
  int* vrow = visit + (size_t)r * NM;
  int* trow = trip_of + (size_t)r * NM;
  const double MD = maxd[r], CAP = cap[r];

  // ---- measure the row as K6 left it, from global memory (any ns): trips, length, validity
  long long part = 0, flags = 0;  // flags: bit 0 a stop number outside the row, bit 1 an unusable demand
  long long groups = 0;
  for (int p = tid; p < ns; p += TEAM) {
    const int v = vrow[p];
    const bool first = p == 0 || trow[p] != trow[p - 1];
    const bool last = p + 1 == ns || trow[p + 1] != trow[p];
    const int a = first ? 0 : vrow[p - 1];
    if (v < 1 || v >= n || a < 0 || a >= n) {
      flags |= 1;
    } else {
      part += quantize_mm(d[(size_t)a * NM + v]);
      if (last) part += quantize_mm(d[(size_t)v * NM]);
      if (quantize_mm(dem[v]) == kBig) flags |= 2;
    }
    groups += first;
  }
  const long long before = team_sum<TEAM>(part, s_redg, tid);
  const int m = (int)team_sum<TEAM>(groups, s_redg, tid);
  const bool bad = team_sum<TEAM>(flags & 1, s_redg, tid) != 0;
  const bool bigdem = team_sum<TEAM>(flags >> 1, s_redg, tid) != 0;
  if (bad) {  // not K6's output: leave the row alone
    put_stats(0, 0, 0, 0, 0, 0);
    return;
  }
  const long long cap_q = quantize_limit(CAP), max_q = quantize_limit(MD);
  if (ns > kMaxStops || ns > KC || m < 2 || bigdem || cap_q < 0 || max_q < 0) {
    put_stats(0, 0, m, m, before, before);  // the stage is skipped
    return;
  }

  // ---- gather: the quantized matrix, the demands, the order, the trips
  for (int c = tid; c < n * n; c += TEAM) {
    const int a = c / n, b = c - a * n;
    sQ[a * S + b] = quantize_mm(d[(size_t)a * NM + b]);
  }
  for (int s = tid; s < n; s += TEAM) s_qd[s] = s == 0 ? 0 : quantize_mm(dem[s]);
  for (int p = tid; p < ns; p += TEAM) {
    s_ord[p] = vrow[p];
    s_bnd[p] = p > 0 && trow[p] != trow[p - 1];
  }
  team_sync<TEAM>();
  for (int p = tid; p < ns; p += TEAM) {
    int t = 0;
    for (int x = 1; x <= p; ++x) t += s_bnd[x];
    s_tof[p] = t;
    if (p == 0 || s_bnd[p]) s_tst[t] = p;
  }
  team_sync<TEAM>();
  for (int p = tid; p < ns; p += TEAM)
    if (p + 1 == ns || s_bnd[p + 1]) s_cnt[s_tof[p]] = p + 1 - s_tst[s_tof[p]];
  team_sync<TEAM>();
  for (int t = tid; t < m; t += TEAM) {
    const int st = s_tst[t], c = s_cnt[t];
    long long L = 0, W = 0;
    int a = 0;
    for (int x = 0; x < c; ++x) {
      const int b = s_ord[st + x];
      L += sQ[a * S + b];
      W += s_qd[b];
      a = b;
    }
    s_Lq[t] = L + sQ[a * S];
    s_Wq[t] = W;
  }

  // ---- best-improvement search
  const int ncols = ns + m + ns;  // insertion edges (one per position, one per trip), swap partners
  int sh = 32 - __builtin_clz(ncols - 1);  // 2^sh >= ncols (ncols >= 4)
  sh = sh > TEAM_SHIFT ? TEAM_SHIFT : sh;
  const int CW = 1 << sh;
  const int col0 = tid & (CW - 1), row0 = tid >> sh, rstep = TEAM >> sh;
  const int limit = move_cap < 0 ? 4 * ns : move_cap;
  int cur = 0, moves = 0, rejected = 0;
  while (moves < limit) {
    team_sync<TEAM>();
    int* ord = s_ord + cur * V4;
    int* tof = s_tof + cur * V4;
    int* tst = s_tst + cur * V4;
    int* cnt = s_cnt + cur * V4;
    // 1. per-position and per-edge terms
    for (int p = tid; p < ns; p += TEAM) {
      const int s = ord[p], t = tof[p], i = p - tst[t] + 1;
      const int pv = i == 1 ? 0 : ord[p - 1], nx = i == cnt[t] ? 0 : ord[p + 1];
      const long long in = sQ[pv * S + s];
      const long long nb = in + sQ[s * S + nx];
      const long long rem = nb - sQ[pv * S + nx];
      s_nb[p] = nb;
      s_rem[p] = rem;
      const unsigned may = s_Lq[t] - rem <= max_q ? 1u : 0u;
      s_pw[p] = (unsigned)s | ((unsigned)t << 8) | ((unsigned)i << 16) | (may << 25);
      s_pn[p] = (unsigned)pv | ((unsigned)nx << 8);
      s_edge[p] = (unsigned)pv | ((unsigned)s << 8) | ((unsigned)t << 16) | ((unsigned)(i - 1) << 24);
      s_ebase[p] = in;
    }
    for (int t = tid; t < m; t += TEAM) {
      const int c = cnt[t];
      if (c > 0) {
        const int lastv = ord[tst[t] + c - 1];
        s_edge[ns + t] = (unsigned)lastv | ((unsigned)t << 16) | ((unsigned)c << 24);
        s_ebase[ns + t] = sQ[lastv * S];
      } else {
        s_edge[ns + t] = kNoEdge;
      }
    }
    team_sync<TEAM>();

    // 2. the candidate scan
    long long bg = 0, bc = LLONG_MAX;
    auto take = [&](long long g, long long code) {
      if (g > bg || (g == bg && code < bc)) {
        bg = g;
        bc = code;
      }
    };
    for (int c = col0; c < ncols; c += CW) {
      if (c < ns + m) {  // relocate the stop of position p to this edge
        const unsigned w = s_edge[c];
        const int u = w & 255;
        if ((unsigned)u == kNoEdge) continue;
        const int v = (w >> 8) & 255, B = (w >> 16) & 255, j = w >> 24;
        const long long eb = s_ebase[c], LB = s_Lq[B], WB = s_Wq[B];
        const long long* qu = sQ + u * S;
        for (int p = row0; p < ns; p += rstep) {
          const unsigned pw = s_pw[p];
          const int s = pw & 255, A = (pw >> 8) & 255;
          if (A == B || !((pw >> 25) & 1)) continue;
          const long long ins = qu[s] + sQ[s * S + v] - eb;
          const long long g = s_rem[p] - ins;
          if (g > 0 && WB + s_qd[s] <= cap_q && LB + ins <= max_q)
            take(g, move_code(0, A, (pw >> 16) & 255, B, j));
        }
      } else {           // swap the stop of position p with this partner, A < B
        const int p2 = c - (ns + m);
        const unsigned pw2 = s_pw[p2], pn2 = s_pn[p2];
        const int u = pw2 & 255, B = (pw2 >> 8) & 255, j = (pw2 >> 16) & 255;
        const int pb = pn2 & 255, nxb = (pn2 >> 8) & 255;
        const long long nb2 = s_nb[p2], LB = s_Lq[B], WB = s_Wq[B], qu = s_qd[u];
        const long long* qpb = sQ + pb * S;
        const long long* qrow_u = sQ + u * S;
        for (int p = row0; p < ns; p += rstep) {
          const unsigned pw = s_pw[p];
          const int s = pw & 255, A = (pw >> 8) & 255;
          if (A >= B) continue;
          const unsigned pn = s_pn[p];
          const int pa = pn & 255, na = (pn >> 8) & 255;
          const long long dA = sQ[pa * S + u] + qrow_u[na] - s_nb[p];
          const long long dB = qpb[s] + sQ[s * S + nxb] - nb2;
          const long long g = -(dA + dB);
          if (g <= 0) continue;
          const long long wd = qu - s_qd[s];  // what trip A's load gains
          if (s_Wq[A] + wd <= cap_q && WB - wd <= cap_q && s_Lq[A] + dA <= max_q && LB + dB <= max_q)
            take(g, move_code(1, A, (pw >> 16) & 255, B, j));
        }
      }
    }
    // 3. (max gain, then min move code) over the wave, then over the team
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long og = __shfl_xor(bg, o);
      const long long oc = __shfl_xor(bc, o);
      if (og > bg || (og == bg && oc < bc)) {
        bg = og;
        bc = oc;
      }
    }
    if constexpr (TEAM != 64) {
      if ((tid & 63) == 0) {
        s_redg[tid >> 6] = bg;
        s_redc[tid >> 6] = bc;
      }
      __syncthreads();
      bg = s_redg[0];
      bc = s_redc[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) {
        const long long og = s_redg[w];
        const long long oc = s_redc[w];
        if (og > bg || (og == bg && oc < bc)) {
          bg = og;
          bc = oc;
        }
      }
    }
    bg = wave_first(bg);
    bc = wave_first(bc);
    if (bg <= 0) break;

    // the move, its effect on the two trips' Lq / Wq, and the moved order in the other copy
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
    if (mt == 0) {
      const int u = mj == 0 ? 0 : ord[tst[mB] + mj - 1];
      const int v = mj == cnt[mB] ? 0 : ord[tst[mB] + mj];
      dLA = -s_rem[pA];
      dLB = sQ[u * S + sA] + sQ[sA * S + v] - sQ[u * S + v];
      dWA = -s_qd[sA];
      dWB = s_qd[sA];
      // B behind A: the stops between move one place to the front; B before A: one place back
      const int dst = mB > mA ? tst[mB] + mj - 1 : tst[mB] + mj;
      for (int p = tid; p < ns; p += TEAM) {
        int src = p;
        if (mB > mA) {
          if (p >= pA && p < dst) src = p + 1;
        } else {
          if (p > dst && p <= pA) src = p - 1;
        }
        nord[p] = p == dst ? sA : ord[src];
        ntof[p] = p == dst ? mB : tof[src];
      }
      for (int t = tid; t < m; t += TEAM) {
        int st = tst[t];
        if (mB > mA) {
          if (t > mA && t <= mB) --st;
        } else {
          if (t > mB && t <= mA) ++st;
        }
        ntst[t] = st;
        ncnt[t] = cnt[t] + (t == mB) - (t == mA);
      }
    } else {
      const int pB = tst[mB] + mj - 1;
      const int sB = ord[pB];
      const unsigned pna = s_pn[pA], pnb = s_pn[pB];
      dLA = sQ[(pna & 255) * S + sB] + sQ[sB * S + ((pna >> 8) & 255)] - s_nb[pA];
      dLB = sQ[(pnb & 255) * S + sA] + sQ[sA * S + ((pnb >> 8) & 255)] - s_nb[pB];
      dWA = s_qd[sB] - s_qd[sA];
      dWB = -dWA;
      for (int p = tid; p < ns; p += TEAM) {
        nord[p] = p == pA ? sB : (p == pB ? sA : ord[p]);
        ntof[p] = tof[p];
      }
      for (int t = tid; t < m; t += TEAM) {
        ntst[t] = tst[t];
        ncnt[t] = cnt[t];
      }
    }
    team_sync<TEAM>();

    // 4. acceptance as the greedy measures it: the two touched trips, f64, in visiting order
    for (int x = 0; x < 2; ++x) {
      const int t = x == 0 ? mA : mB;
      const int st = ntst[t], c = ncnt[t];
      for (int e = tid; e <= c; e += TEAM) {
        const int a = e == 0 ? 0 : nord[st + e - 1];
        const int b = e == c ? 0 : nord[st + e];
        s_dv[x * V8 + e] = d[(size_t)a * NM + b];
        if (e < c) s_dm[x * V8 + e] = dem[b];
      }
    }
    team_sync<TEAM>();
    if (tid < 2) {
      const int c = ncnt[tid == 0 ? mA : mB];
      const double* dv = s_dv + tid * V8;
      const double* dm = s_dm + tid * V8;
      double s = 0.0, load = 0.0;
      for (int p = 0; p < c; ++p) {
        s += dv[p];
        load += dm[p];
      }
      s_misc[tid] = (s + dv[c] <= MD && load <= CAP) ? 1 : 0;
    }
    team_sync<TEAM>();
    if (!(s_misc[0] != 0 && s_misc[1] != 0)) {  // undone: the first copy stays, the search ends
      rejected = 1;
      break;
    }
    if (tid == 0) {
      s_Lq[mA] += dLA;
      s_Lq[mB] += dLB;
      s_Wq[mA] += dWA;
      s_Wq[mB] += dWB;
    }
    cur = nxt;
    ++moves;
  }
  team_sync<TEAM>();

  // ---- the non-empty trips, compacted in their order
  const int* ord = s_ord + cur * V4;
  const int* tof = s_tof + cur * V4;
  const int* cnt = s_cnt + cur * V4;
  if (tid == 0) {
    int k = 0;
    long long after = 0;
    for (int t = 0; t < m; ++t) {
      s_rank[t] = k;
      if (cnt[t] > 0) {
        ++k;
        after += s_Lq[t];
      }
    }
    moves_out[r] = moves;
    rejected_out[r] = rejected;
    tbefore_out[r] = m;
    tafter_out[r] = k;
    before_out[r] = before;
    after_out[r] = after;
    if (moves > 0) ntrips[r] = k;
  }
  team_sync<TEAM>();
  if (moves > 0)
    for (int p = tid; p < ns; p += TEAM) {
      vrow[p] = ord[p];
      trow[p] = s_rank[tof[p]];
    }
}

}  // namespace

hipError_t launch_exchange_trips(const double* D, const int* npts, const double* demand,
                                 const double* cap, const double* maxd, const unsigned char* flag,
                                 const int* status, int R, int NM, int move_cap, int* visit,
                                 int* trip_of, int* ntrips, int* moves, int* rejected,
                                 int* trips_before, int* trips_after, long long* len_before_q,
                                 long long* len_after_q, hipStream_t stream) {
  if (R == 0) return hipSuccess;
  if (NM < 1 || NM > 4096) return hipErrorInvalidValue;
  // small tier: rows of at most 32 stops, a wavefront each
  {
    const int kc = NM - 1 < kSmallStops ? (NM - 1 < 1 ? 1 : NM - 1) : kSmallStops;
    const size_t lds = 4 * exchange_team_bytes(kc);
    hipLaunchKernelGGL(exchange_trips_kernel<64>, dim3((R + 3) / 4), dim3(256), lds, stream, D, npts,
                       demand, cap, maxd, flag, status, R, NM, kc, move_cap, visit, trip_of, ntrips,
                       moves, rejected, trips_before, trips_after, len_before_q, len_after_q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (NM - 1 <= kSmallStops) return hipSuccess;
  // large tier: a 1024-thread workgroup each; the whole matrix of 128 stops (133 KB) and the
  // per-stop / per-trip arrays need the opt-in LDS size
  const int kc = NM - 1 < kMaxStops ? NM - 1 : kMaxStops;
  const size_t lds = exchange_team_bytes(kc);
  static_assert(exchange_team_bytes(kMaxStops) <= 160 * 1024, "a row's LDS must fit a CU");
  static_assert(4 * exchange_team_bytes(kSmallStops) <= 64 * 1024, "the small tier stays in the default LDS size");
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)exchange_trips_kernel<kLargeTeam>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(exchange_trips_kernel<kLargeTeam>, dim3(R), dim3(kLargeTeam), lds, stream, D,
                     npts, demand, cap, maxd, flag, status, R, NM, kc, move_cap, visit, trip_of,
                     ntrips, moves, rejected, trips_before, trips_after, len_before_q, len_after_q);
  return hipGetLastError();
}

}  // namespace rt
