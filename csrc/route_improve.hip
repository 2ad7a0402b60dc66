// K6b: intra-trip 2-opt / Or-opt improvement of K6's greedy trips (gfx950), opt-in per request.
//
// The definition (fixed-point millimetres, move types, best-improvement selection with the
// (type, i, j) tie rule, the 4k move cap, the 128-stop limit and the f64 feasibility walk) is in
// routest_amd/routing/improve.py; the host C++ is rtr::improve_trips (runtime/route_core.h).  All
// three are compared with ==: every gain is an int64 sum, so the schedule below cannot change it.
//
// One TEAM of threads per request row, the row's trips one after the other:
//   * small tier: rows with at most 32 stops, TEAM = one wavefront, four rows per 256-thread block
//     (like K6); only wave barriers, so a wave may leave early;
//   * large tier: rows with more stops, TEAM = one 1024-thread block (the sub-matrix of a long
//     trip fills most of a CU's LDS, so the block's 16 waves are what hides the LDS latency);
//     every branch around a __syncthreads depends only on values all threads read from LDS or from
//     the same address.
// Both tiers are launched over all rows and each row is handled by the tier its stop count picks;
// the small tier also zeroes the statistics of rows that do not ask.
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
// The per-lane loops of step 3 hold no barrier and no cross-lane operation; every loop that does
// is bounded by values the whole team holds.  No global atomics, nothing waits on another team.
#include <climits>

#include "common.h"
#include "ops.h"

namespace rt {

namespace {

constexpr long long kBig = 1LL << 50;
constexpr long long kNever = -(1LL << 62);  // a row term that keeps a gain below 0 whatever is added
constexpr int kMaxStops = 128;
constexpr int kSmallStops = 32;
constexpr int kLargeTeam = 1024;

__device__ __forceinline__ long long quantize_mm(double x) {
  if (!(x >= 0.0) || x >= 1099511627776.0) return kBig;  // NaN, +-inf, negatives, >= 2^40
  return __double2ll_rn(x * 1000.0);
}

// LDS of one team, carved from the dynamic region (every offset a multiple of 16).
__host__ __device__ constexpr int improve_stride(int kc) { return (kc + 1) | 1; }
__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t improve_team_bytes(int kc) {
  return align16((size_t)(kc + 1) * improve_stride(kc) * 8)  // Q
         + 9 * align16((size_t)(kc + 2) * 8)                 // f, b, pf, pb, row[4], dv
         + 3 * align16((size_t)(kc + 2) * 4)                 // node, ord, win
         + 128 + 64 + 16;                                    // red_g[16] | red_c[16] | misc[4]
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

// a move as one int that orders like (type, i, j): i, j <= 128
__device__ __forceinline__ int move_code(int type, int i, int j) { return (type << 16) | (i << 8) | j; }

// KC: stop capacity of the LDS carve (the launch sizes the dynamic region for it).
template <int TEAM>
__global__ __launch_bounds__(TEAM == 64 ? 256 : TEAM) void improve_trips_kernel(
    const double* __restrict__ D, const int* __restrict__ npts, const double* __restrict__ maxd,
    const unsigned char* __restrict__ flag, const int* __restrict__ status, int R, int NM, int KC,
    int* __restrict__ visit, const int* __restrict__ trip_of, int* __restrict__ moves_out,
    int* __restrict__ changed_out, long long* __restrict__ before_out,
    long long* __restrict__ after_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TEAMS = TEAM == 64 ? 4 : 1;
  constexpr int WAVES = TEAM / 64;
  const int team = TEAM == 64 ? (int)(threadIdx.x >> 6) : 0;
  const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int r = blockIdx.x * TEAMS + team;
  if (r >= R) return;  // small tier: wave-uniform, no block barrier below; large tier: never taken
  int n = npts[r];
  n = n < 0 ? 0 : (n > NM ? NM : n);
  const int ns = n > 0 ? n - 1 : 0;
  const bool small_row = ns <= kSmallStops;
  if (small_row != (TEAM == 64)) return;  // the other tier's row (uniform over the team)
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

  unsigned char* base = smem + (size_t)team * improve_team_bytes(KC);
  const int S = improve_stride(KC);
  const size_t vec8 = align16((size_t)(KC + 2) * 8), vec4 = align16((size_t)(KC + 2) * 4);
  long long* sQ = (long long*)base;
  base += align16((size_t)(KC + 1) * S * 8);
  long long* s_f = (long long*)base;
  long long* s_b = (long long*)(base + vec8);
  long long* s_pf = (long long*)(base + 2 * vec8);
  long long* s_pb = (long long*)(base + 3 * vec8);
  long long* s_row = (long long*)(base + 4 * vec8);  // [KC + 2][4]: c0, rem[1], rem[2], rem[3]
  double* s_dv = (double*)(base + 8 * vec8);
  base += 9 * vec8;
  int* s_node = (int*)base;
  int* s_ord = (int*)(base + vec4);
  unsigned* s_win = (unsigned*)(base + 2 * vec4);    // t[i-1] | t[i] << 8 | t[i+1] << 16 | t[i+2] << 24
  base += 3 * vec4;
  long long* s_redg = (long long*)base;
  int* s_redc = (int*)(base + 128);
  int* s_misc = (int*)(base + 192);  // [0] end of the trip, [1] bad stop number, [2] keep

  const double* d = D + (size_t)r * NM * NM;
  int* vrow = visit + (size_t)r * NM;
  const int* trow = trip_of + (size_t)r * NM;
  const double MD = maxd[r];

  int tot_moves = 0, tot_changed = 0;
  long long tot_before = 0, tot_after = 0;

  int pos = 0;
  while (pos < ns) {
    // ---- the trip's extent: the first position whose successor belongs to another trip
    const int tr = trow[pos];
    if (tid == 0) {
      s_misc[0] = ns;
      s_misc[1] = 0;
    }
    team_sync<TEAM>();
    for (int p = pos + tid; p < ns; p += TEAM)
      if (trow[p] == tr && (p + 1 == ns || trow[p + 1] != tr)) atomicMin(&s_misc[0], p + 1);
    team_sync<TEAM>();
    const int end = s_misc[0];
    const int k = end - pos;  // >= 1
    team_sync<TEAM>();

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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    long long before = part;
    if constexpr (TEAM != 64) {
      if ((tid & 63) == 0) s_redg[tid >> 6] = part;
      if (bad) s_misc[1] = 1;
      __syncthreads();
      before = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) before += s_redg[w];
      bad = s_misc[1] != 0;
      __syncthreads();
    } else {
      bad = __ballot(bad) != 0ULL;
    }
    before = wave_first(before);
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
    team_sync<TEAM>();
    const int k1 = k + 1;
    for (int c = tid; c < k1 * k1; c += TEAM) {
      const int a = c / k1, b = c - a * k1;
      sQ[a * S + b] = quantize_mm(d[(size_t)s_node[a] * NM + s_node[b]]);
    }
    team_sync<TEAM>();

    // ---- best-improvement search
    // a lane's insertion point / reversal end j and its first row; JW lanes per row
    const int jsh = 32 - __builtin_clz(k);  // JW = 2^jsh >= k + 1 (k >= 2); <= TEAM in both tiers
    const int j = tid & ((1 << jsh) - 1);
    const int i0 = 1 + (tid >> jsh);
    const int istep = TEAM >> jsh;
    int moves = 0;
    long long after = before;
    for (;;) {
      for (int p = tid; p <= k; p += TEAM) {
        const int a = s_ord[p], b = s_ord[p + 1];
        s_f[p] = sQ[a * S + b];
        s_b[p] = sQ[b * S + a];
      }
      team_sync<TEAM>();
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
      team_sync<TEAM>();
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
      // (max gain, then min move code) over the wave, then over the team
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const long long og = __shfl_xor(bg, o);
        const int oc = __shfl_xor(bc, o);
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
          const int oc = s_redc[w];
          if (og > bg || (og == bg && oc < bc)) {
            bg = og;
            bc = oc;
          }
        }
      }
      bg = wave_first(bg);
      bc = __builtin_amdgcn_readfirstlane(bc);
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
      team_sync<TEAM>();
      if (p <= hi) s_ord[p] = val;
      team_sync<TEAM>();
      ++moves;
    }

    // ---- feasibility as the greedy measures it: f64 walk in order, one lane adds
    bool keep = false;
    if (moves > 0) {
      for (int p = tid; p <= k; p += TEAM)
        s_dv[p] = d[(size_t)s_node[s_ord[p]] * NM + s_node[s_ord[p + 1]]];
      team_sync<TEAM>();
      if (tid == 0) {
        double s = 0.0;
        for (int p = 0; p < k; ++p) s += s_dv[p];
        s_misc[2] = (s + s_dv[k]) <= MD ? 1 : 0;
      }
      team_sync<TEAM>();
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
    team_sync<TEAM>();
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
  if (R == 0) return hipSuccess;
  if (NM < 1 || NM > 4096) return hipErrorInvalidValue;
  // small tier: rows of at most 32 stops, a wavefront each
  {
    const int kc = NM - 1 < kSmallStops ? (NM - 1 < 1 ? 1 : NM - 1) : kSmallStops;
    const size_t lds = 4 * improve_team_bytes(kc);
    hipLaunchKernelGGL(improve_trips_kernel<64>, dim3((R + 3) / 4), dim3(256), lds, stream, D, npts,
                       maxd, flag, status, R, NM, kc, visit, trip_of, moves, trips_changed,
                       len_before_q, len_after_q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (NM - 1 <= kSmallStops) return hipSuccess;
  // large tier: a 1024-thread workgroup each; up to 143 KB of LDS (k = 128) needs the opt-in size
  const int kc = NM - 1 < kMaxStops ? NM - 1 : kMaxStops;
  const size_t lds = improve_team_bytes(kc);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)improve_trips_kernel<kLargeTeam>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(improve_trips_kernel<kLargeTeam>, dim3(R), dim3(kLargeTeam), lds, stream, D,
                     npts, maxd, flag, status, R, NM, kc, visit, trip_of, moves, trips_changed,
                     len_before_q, len_after_q);
  return hipGetLastError();
}

}  // namespace rt
