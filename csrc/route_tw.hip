// K6d: cheapest-insertion construction of trips under time windows and service times (gfx950),
// opt-in per request row.
//
// The definition (fixed-point millimetres and milliseconds, the unusable-entry rule, the schedule
// and latest-start recurrences, alone-feasibility, the seed rule, the O(1) admissibility test, the
// (ins, u, j) tie rule and the f64 acceptance walks) is in routest_amd/routing/timewindows.py; the
// host C++ is rtr::tw_trips (runtime/route_core.h).  All three are compared with ==: every quantity
// the search orders by is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row, with K6b / K6c's two tiers and their barrier discipline:
//   * small tier: rows with at most 32 stops, TEAM = one wavefront, four rows per 256-thread block;
//     only wave barriers, so a wave may leave early;
//   * large tier: rows with 33..128 stops, TEAM = one 1024-thread block; every branch around a
//     __syncthreads depends only on values all threads read from LDS (reduction results) or from the
//     same global address.
// Both tiers are launched over all rows and each row is handled by the tier its stop count picks.
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
// A closed trip's stops, arrivals and starts go out one position per thread.  No global atomics,
// nothing waits on another team; every loop that holds a barrier is bounded by values the whole
// team holds alike.
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
__host__ __device__ constexpr int tw_stride(int kc) { return (kc + 1) | 1; }
__host__ __device__ constexpr size_t talign16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t tw_team_bytes(int kc) {
  return 2 * talign16((size_t)(kc + 1) * tw_stride(kc) * 4)  // Q, T
         + 8 * talign16((size_t)(kc + 4) * 8)                // open, close, sv, qd, dep, z, dv, dm
         + 2 * talign16((size_t)(kc + 4) * 4)                // ord, unr
         + 128 + 128 + 32;                                   // red_a[16] | red_b[16] | misc[8]
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

// the lexicographic minimum of (a, b) over the team, held by every thread
template <int TEAM>
__device__ __forceinline__ void team_min2(long long& a, long long& b, long long* red_a, long long* red_b,
                                          int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long oa = __shfl_xor(a, o);
    const long long ob = __shfl_xor(b, o);
    if (oa < a || (oa == a && ob < b)) {
      a = oa;
      b = ob;
    }
  }
  if constexpr (TEAM != 64) {
    if ((tid & 63) == 0) {
      red_a[tid >> 6] = a;
      red_b[tid >> 6] = b;
    }
    __syncthreads();
    a = red_a[0];
    b = red_b[0];
#pragma unroll
    for (int w = 1; w < TEAM / 64; ++w) {
      const long long oa = red_a[w];
      const long long ob = red_b[w];
      if (oa < a || (oa == a && ob < b)) {
        a = oa;
        b = ob;
      }
    }
    __syncthreads();
  }
  a = wave_first(a);
  b = wave_first(b);
}

// the sum of v over the team, held by every thread
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

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).
template <int TEAM>
__global__ __launch_bounds__(TEAM == 64 ? 256 : TEAM) void tw_trips_kernel(
    const double* __restrict__ D, const double* __restrict__ T, const int* __restrict__ npts,
    const double* __restrict__ demand, const double* __restrict__ cap, const double* __restrict__ maxd,
    const long long* __restrict__ open, const long long* __restrict__ close,
    const long long* __restrict__ service, const unsigned char* __restrict__ flag, int R, int NM, int KC,
    int* __restrict__ visit, int* __restrict__ trip_of, int* __restrict__ ntrips, int* __restrict__ status,
    long long* __restrict__ arrival, long long* __restrict__ start, long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TEAMS = TEAM == 64 ? 4 : 1;
  constexpr int TEAM_SHIFT = TEAM == 64 ? 6 : 10;
  const int team = TEAM == 64 ? (int)(threadIdx.x >> 6) : 0;
  const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int r = blockIdx.x * TEAMS + team;
  if (r >= R) return;  // small tier: wave-uniform, no block barrier below; large tier: never taken
  if (flag[r] == 0) return;  // not a time-window row: nothing of it is touched
  int n = npts[r];
  n = n < 0 ? 0 : (n > NM ? NM : n);
  const int ns = n > 0 ? n - 1 : 0;
  const bool small_row = ns <= kSmallStops;
  if (small_row != (TEAM == 64)) return;  // the other tier's row (uniform over the team)
  long long* srow = stats + (size_t)r * 4;  // insertions, rejected, len_q, waiting_q
  if (ns == 0 || ns > kMaxStops || ns > KC) {
    if (tid == 0) {
      ntrips[r] = 0;
      status[r] = ns == 0 ? 0 : 2;  // 2: more stops than the stage takes
      srow[0] = srow[1] = srow[2] = srow[3] = 0;
    }
    return;
  }

  unsigned char* base = smem + (size_t)team * tw_team_bytes(KC);
  const int S = tw_stride(KC);
  const size_t mat = talign16((size_t)(KC + 1) * S * 4);
  const size_t vec8 = talign16((size_t)(KC + 4) * 8), vec4 = talign16((size_t)(KC + 4) * 4);
  int* sQ = (int*)base;
  int* sT = (int*)(base + mat);
  base += 2 * mat;
  long long* s_open = (long long*)base;
  long long* s_close = (long long*)(base + vec8);
  long long* s_sv = (long long*)(base + 2 * vec8);
  long long* s_qd = (long long*)(base + 3 * vec8);
  long long* s_dep = (long long*)(base + 4 * vec8);  // [0..k]
  long long* s_z = (long long*)(base + 5 * vec8);    // [1..k]
  double* s_dv = (double*)(base + 6 * vec8);         // the lengthened trip's legs, [0..k+1]
  double* s_dm = (double*)(base + 7 * vec8);         // ... and its stops' demands, [0..k]
  base += 8 * vec8;
  int* s_ord = (int*)base;                           // the trip 0, s1..sk, 0: [0..k+1]
  int* s_unr = (int*)(base + vec4);                  // per stop: still unrouted (alone pass: failed)
  base += 2 * vec4;
  long long* s_reda = (long long*)base;
  long long* s_redb = (long long*)(base + 128);
  int* s_misc = (int*)(base + 256);  // [0], [1]: the two walks' verdicts

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
  const double MD = maxd[r], CAP = cap[r];
  const long long cap_q = quantize_limit(CAP), max_q = quantize_limit(MD);

  // ---- gather: both quantized matrices and the per-stop vectors
  for (int c = tid; c < n * n; c += TEAM) {
    const int a = c / n, b = c - a * n;
    sQ[a * S + b] = quantize_entry(d[(size_t)a * NM + b]);
    sT[a * S + b] = quantize_entry(t[(size_t)a * NM + b]);
  }
  for (int s = tid; s < n; s += TEAM) {
    s_open[s] = s == 0 ? 0 : op[s];
    s_close[s] = s == 0 ? kUnbounded : cl[s];
    s_sv[s] = s == 0 ? 0 : sv[s];
    s_qd[s] = s == 0 ? 0 : quantize_mm(dem[s]);
  }
  team_sync<TEAM>();

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
  nbad = team_sum<TEAM>(nbad, s_reda, tid);
  team_sync<TEAM>();
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
    team_sync<TEAM>();
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
    team_min2<TEAM>(ka, kb, s_reda, s_redb, tid);
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
      team_sync<TEAM>();
      // dep[0..k] and z[1..k] of the trip as it stands, one lane each
      if (tid == 0) {
        long long dp = 0;
        s_dep[0] = 0;
        for (int i = 1; i <= k; ++i) {
          const int a = s_ord[i - 1], b = s_ord[i];
          const long long ar = dp + sT[a * S + b];
          dp = (ar > s_open[b] ? ar : s_open[b]) + s_sv[b];
          s_dep[i] = dp;
        }
      } else if (tid == 1) {
        long long zz = s_close[s_ord[k]];
        s_z[k] = zz;
        for (int i = k - 1; i >= 1; --i) {
          const int a = s_ord[i], b = s_ord[i + 1];
          const long long v = zz - sT[a * S + b] - s_sv[a];
          zz = s_close[a] < v ? s_close[a] : v;
          s_z[i] = zz;
        }
      }
      team_sync<TEAM>();

      // 1. the candidate scan: this lane's position j, the unrouted stops u it strides over
      int sh = 32 - __builtin_clz(k);  // 2^sh >= k + 1 positions
      sh = sh > TEAM_SHIFT ? TEAM_SHIFT : sh;
      const int CW = 1 << sh;
      const int col0 = tid & (CW - 1), row0 = tid >> sh, rstep = TEAM >> sh;
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
      team_min2<TEAM>(bi, bc, s_reda, s_redb, tid);
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
      team_sync<TEAM>();
      if (tid == 0) {
        double s = 0.0;
        for (int p = 0; p < kk; ++p) s += s_dv[p];
        s_misc[0] = s + s_dv[kk] <= MD ? 1 : 0;
      } else if (tid == 1) {
        double load = 0.0;
        for (int p = 0; p < kk; ++p) load += s_dm[p];
        s_misc[1] = load <= CAP ? 1 : 0;
      }
      team_sync<TEAM>();
      if (!(s_misc[0] != 0 && s_misc[1] != 0)) {  // not applied: the trip is closed
        ++rejected;
        break;
      }

      // 4. the insertion: the positions behind bj move back by one, one position per thread
      const int p = tid;  // k + 3 <= TEAM positions in both tiers
      const int moved = (p >= bj + 2 && p <= kk + 1) ? s_ord[p - 1] : 0;
      team_sync<TEAM>();
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
    team_sync<TEAM>();
    // the closed trip: one lane walks its schedule (arrivals into z[], starts into dep[], both no
    // longer needed), then its stops, arrivals and starts go out one position per thread
    if (tid == 0) {
      long long dp = 0;
      for (int i = 1; i <= k; ++i) {
        const int a = s_ord[i - 1], b = s_ord[i];
        const long long ar = dp + sT[a * S + b];
        const long long stt = ar > s_open[b] ? ar : s_open[b];
        s_z[i] = ar;
        s_dep[i] = stt;
        dp = stt + s_sv[b];
      }
    }
    team_sync<TEAM>();
    for (int i = 1 + tid; i <= k; i += TEAM) {
      vrow[placed + i - 1] = s_ord[i];
      trow[placed + i - 1] = trips;
      arow[placed + i - 1] = s_z[i];
      strow[placed + i - 1] = s_dep[i];
      wait_part += s_dep[i] - s_z[i];
    }
    placed += k;
    len_q += Lq;
    ++trips;
  }
  const long long waiting = team_sum<TEAM>(wait_part, s_reda, tid);
  if (tid == 0) {
    ntrips[r] = trips;
    status[r] = 0;
    srow[0] = insertions;
    srow[1] = rejected;
    srow[2] = len_q;
    srow[3] = waiting;
  }
}

}  // namespace

hipError_t launch_tw_trips(const double* D, const double* T, const int* npts, const double* demand,
                           const double* cap, const double* maxd, const long long* open,
                           const long long* close, const long long* service, const unsigned char* flag,
                           int R, int NM, int* visit, int* trip_of, int* ntrips, int* status,
                           long long* arrival, long long* start, long long* stats, hipStream_t stream) {
  if (R == 0) return hipSuccess;
  if (NM < 1 || NM > 4096) return hipErrorInvalidValue;
  static_assert(tw_team_bytes(kMaxStops) <= 160 * 1024, "a row's LDS must fit a CU");
  static_assert(4 * tw_team_bytes(kSmallStops) <= 64 * 1024, "the small tier stays in the default LDS size");
  // small tier: rows of at most 32 stops, a wavefront each
  {
    const int kc = NM - 1 < kSmallStops ? (NM - 1 < 1 ? 1 : NM - 1) : kSmallStops;
    const size_t lds = 4 * tw_team_bytes(kc);
    hipLaunchKernelGGL(tw_trips_kernel<64>, dim3((R + 3) / 4), dim3(256), lds, stream, D, T, npts, demand,
                       cap, maxd, open, close, service, flag, R, NM, kc, visit, trip_of, ntrips, status,
                       arrival, start, stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (NM - 1 <= kSmallStops) return hipSuccess;
  // large tier: a 1024-thread workgroup each; both int32 matrices of 128 stops (2 x 66.6 KB) and the
  // per-stop arrays need the opt-in LDS size
  const int kc = NM - 1 < kMaxStops ? NM - 1 : kMaxStops;
  const size_t lds = tw_team_bytes(kc);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)tw_trips_kernel<kLargeTeam>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tw_trips_kernel<kLargeTeam>, dim3(R), dim3(kLargeTeam), lds, stream, D, T, npts,
                     demand, cap, maxd, open, close, service, flag, R, NM, kc, visit, trip_of, ntrips,
                     status, arrival, start, stats);
  return hipGetLastError();
}

}  // namespace rt
