// K10: GPS-trace map matching on the road graph (gfx950): candidate search and the segmenting
// Viterbi of the node-based hidden-Markov matcher.
//
// The definition (integer centimetres, the (d2, node id) candidate order, emission / transition
// costs, lowest-i / lowest-j ties, breaks) is in routest_amd/routing/mapmatch.py; the host C++ is
// rtr::mm_candidates / rtr::mm_viterbi (runtime/map_match.h).  All three are compared with ==: every
// value below is an integer, every selection a minimum over totally ordered keys, so neither the
// lane mapping nor the schedule can change a result.  No floats, no atomics.
//
// mm_candidates_kernel: one wave per fix, four fixes per 256-thread block.  The cells the radius
// covers are row-major, so each covered grid row is ONE contiguous span of `items`; the lanes stride
// over it.  Then k rounds of "the smallest 64-bit key (d2 << 30 | node) greater than the previous
// round's", reduced across the wave by xor shuffles: round m yields the m-th candidate.  d2 <=
// (1e5 cm)^2 < 2^34 and node < 2^30, so a key fits an unsigned 64-bit word and is never ~0.
//
// mm_viterbi_kernel: one wave per trace (a 64-thread block).  With KP = the power of two >= K the
// lane l is target state j = l % KP of predecessor group ig = l / KP (G = 64 / KP groups); a lane
// walks the predecessors i = ig, ig + G, ... (at most 4 of them) in ascending order with a strict
// <, and the groups fold (score, i) by xor shuffles over KP, 2 KP, ..., 32, so that every lane of a
// column ends up with the column's minimum and the lowest i among equals.  Scores are int64 in
// registers (lane j of group 0 is read by __shfl), back pointers are bytes in LDS (T * K, plus T
// bytes for the segments' final states, reused for the choices on the way back); the next step's
// K x K block of route centimetres is loaded before the current one is reduced.  The same wave
// walks the back pointers (lane 0) and the 64 lanes copy the choices out.  Every shuffle and every
// barrier sits in wave-uniform control flow: the loop bounds and the break test are the same in
// all lanes.
#include <climits>

#include "common.h"
#include "ops.h"

namespace rt {

namespace {

constexpr int kMmMaxK = 16;
constexpr int kMmMaxPoints = 2048;
// Score bounds (MatchParams in mapmatch.py): radius <= 1e5 cm, beta <= 1e4 cm, sigma <= 2e4 cm,
// max_detour <= 5e5 cm, at most 2048 fixes: a step adds at most 1e4 * 1e10 + 2 * 4e8 * 5e5 = 5e14,
// a path score stays below 2048 * 5e14 ~ 1.0e18 < kDead = 2^62.
constexpr long long kDead = 1LL << 62;
constexpr unsigned long long kNone = ~0ULL;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void mm_candidates_kernel(
    const int* __restrict__ start, const int* __restrict__ items, const long long* __restrict__ nqy,
    const long long* __restrict__ nqx, int N, long long y0, long long x0, long long cell, int ny, int nx,
    const long long* __restrict__ py, const long long* __restrict__ px, int P, long long radius, int k,
    int* __restrict__ cand, long long* __restrict__ cand_d2, int* __restrict__ n_cand) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
  if (p >= P) return;
  const long long qy = py[p], qx = px[p];
  // the cells the radius covers, clamped to the grid; empty when the fix lies beyond it
  const long long yhi = qy + radius - y0, xhi = qx + radius - x0;
  long long ylo = qy - radius - y0, xlo = qx - radius - x0;
  ylo = ylo < 0 ? 0 : ylo;
  xlo = xlo < 0 ? 0 : xlo;
  int cy0 = 0, cy1 = -1, cx0 = 0, cx1 = -1;
  if (yhi >= 0 && xhi >= 0 && ylo / cell < ny && xlo / cell < nx) {
    cy0 = (int)(ylo / cell);
    cx0 = (int)(xlo / cell);
    const long long a = yhi / cell, b = xhi / cell;
    cy1 = a < ny - 1 ? (int)a : ny - 1;
    cx1 = b < nx - 1 ? (int)b : nx - 1;
  }
  const long long r2 = radius * radius;
  unsigned long long prev = 0;
  int found = 0;
  for (int m = 0; m < k; ++m) {
    unsigned long long best = kNone;
    for (int cy = cy0; cy <= cy1; ++cy) {
      int lo = start[(size_t)cy * nx + cx0], hi = start[(size_t)cy * nx + cx1 + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > N ? N : hi;
      for (int e = lo + lane; e < hi; e += 64) {
        const int v = items[e];
        if ((unsigned)v >= (unsigned)N) continue;
        const long long dy = nqy[v] - qy, dx = nqx[v] - qx;
        if (dy > radius || dy < -radius || dx > radius || dx < -radius) continue;
        const long long d2 = dy * dy + dx * dx;
        if (d2 > r2) continue;
        const unsigned long long key = ((unsigned long long)d2 << 30) | (unsigned)v;
        if ((m == 0 || key > prev) && key < best) best = key;
      }
    }
    best = wave_min_u64(best);
    if (best == kNone) break;   // wave-uniform: every lane holds the reduced value
    if (lane == 0) {
      cand[(size_t)p * k + m] = (int)(best & ((1ULL << 30) - 1));
      cand_d2[(size_t)p * k + m] = (long long)(best >> 30);
    }
    prev = best;
    ++found;
  }
  if (lane == 0) n_cand[p] = found;
  for (int m = found + lane; m < k; m += 64) {
    cand[(size_t)p * k + m] = -1;
    cand_d2[(size_t)p * k + m] = -1;
  }
}

// the lowest (score, j) over the K states; every lane returns the same j (ties: the lowest j)
__device__ __forceinline__ int best_state(long long score, int j, int KP, long long* out_score) {
  long long s = score;
  int a = j;
  for (int off = 1; off < KP; off <<= 1) {
    const long long os = __shfl_xor(s, off, 64);
    const int oa = __shfl_xor(a, off, 64);
    if (os < s || (os == s && oa < a)) {
      s = os;
      a = oa;
    }
  }
  *out_score = s;
  return a;
}

__global__ __launch_bounds__(64) void mm_viterbi_kernel(
    const long long* __restrict__ cand_d2, const int* __restrict__ n_cand, const long long* __restrict__ route_cm,
    const long long* __restrict__ g, const int* __restrict__ npts, int B, int T, int K, int KP, long long beta,
    long long two_s2, long long max_detour, int* __restrict__ choice, int* __restrict__ seg,
    int* __restrict__ nseg_out, long long* __restrict__ cost_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mm_lds[];
  unsigned char* bp = mm_lds;                      // [T][K] back pointers, 0xFF = none
  unsigned char* fin = mm_lds + (size_t)T * K;     // [T] a segment's final state at its last fix; then the choices
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int j = lane & (KP - 1);
  const int G = 64 / KP;
  const int ig = lane / KP;
  int n = npts[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  const long long* cd = cand_d2 + (size_t)b * T * K;
  const int* nc = n_cand + (size_t)b * T;
  const long long* rc = route_cm + (size_t)b * (T - 1) * K * K;
  const long long* gg = g + (size_t)b * (T - 1);
  int* ch = choice + (size_t)b * T;
  int* sg = seg + (size_t)b * T;
  for (int t = n + lane; t < T; t += 64) {
    ch[t] = -1;
    sg[t] = -1;
  }
  if (n == 0) {   // wave-uniform
    if (lane == 0) {
      nseg_out[b] = 0;
      cost_out[b] = 0;
    }
    return;
  }
  auto clampn = [K](int x) { return x < 1 ? 1 : (x > K ? K : x); };
  auto emit = [&](int t, int ncur) { return j < ncur ? beta * cd[(size_t)t * K + j] : kDead; };
  // the lane's (at most 4) entries of step t's K x K block: rows i = ig + m G, column j
  auto load_block = [&](int t, long long* r) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = ig + m * G;
      r[m] = (i < K && j < K) ? rc[((size_t)(t - 1) * K + i) * K + j] : -1;
    }
  };

  int n_prev = clampn(nc[0]);
  long long score = emit(0, n_prev);
  long long cost = 0;
  int nseg = 0;
  if (ig == 0 && j < K) bp[j] = 0xFF;
  if (lane == 0) sg[0] = 0;
  long long cur[4] = {-1, -1, -1, -1}, nxt[4] = {-1, -1, -1, -1};
  if (n > 1) load_block(1, cur);
  for (int t = 1; t < n; ++t) {
    if (t + 1 < n) load_block(t + 1, nxt);   // in flight while this step is reduced
    const int n_cur = clampn(nc[t]);
    const long long gt = gg[t - 1];
    long long best = kDead;
    int arg = 255;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = ig + m * G;
      const long long sp = __shfl(score, i & (KP - 1), 64);   // unconditional: all 64 lanes take part
      const long long r = cur[m];
      const long long dev = r > gt ? r - gt : gt - r;
      if (i < n_prev && j < n_cur && sp < kDead && r >= 0 && dev <= max_detour) {
        const long long v = sp + two_s2 * dev;
        if (v < best) {
          best = v;
          arg = i;
        }
      }
    }
    for (int off = KP; off < 64; off <<= 1) {
      const long long ob = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(arg, off, 64);
      if (ob < best || (ob == best && oa < arg)) {
        best = ob;
        arg = oa;
      }
    }
    long long ns = best < kDead ? best + emit(t, n_cur) : kDead;
    if (__ballot(ns < kDead) == 0ULL) {   // a break: the segment ends at t - 1, a new one starts here
      long long s;
      const int a = best_state(score, j, KP, &s);
      if (lane == 0) fin[t - 1] = (unsigned char)a;
      cost += s;
      ++nseg;
      ns = emit(t, n_cur);
      arg = 255;
    }
    if (ig == 0 && j < K) bp[(size_t)t * K + j] = (unsigned char)arg;
    if (lane == 0) sg[t] = nseg;
    score = ns;
    n_prev = n_cur;
#pragma unroll
    for (int m = 0; m < 4; ++m) cur[m] = nxt[m];
  }
  {
    long long s;
    const int a = best_state(score, j, KP, &s);
    if (lane == 0) fin[n - 1] = (unsigned char)a;
    cost += s;
    ++nseg;
  }
  __syncthreads();   // one wave: orders the LDS writes above before lane 0's reads
  if (lane == 0) {
    int c = fin[n - 1];
    for (int t = n - 1; t >= 0; --t) {
      const unsigned char back = bp[(size_t)t * K + c];
      const int here = c;
      if (back == 0xFF) {
        if (t > 0) c = fin[t - 1];
      } else {
        c = back;
      }
      fin[t] = (unsigned char)here;   // fin[t - 1] was read before this slot is reused
    }
    nseg_out[b] = nseg;
    cost_out[b] = cost;
  }
  __syncthreads();
  for (int t = lane; t < n; t += 64) ch[t] = fin[t];
}

}  // namespace

hipError_t launch_mm_candidates(const int* start, const int* items, const long long* nqy, const long long* nqx,
                                int N, long long y0, long long x0, long long cell, int ny, int nx,
                                const long long* py, const long long* px, int P, long long radius_cm, int k,
                                int* cand, long long* cand_d2, int* n_cand, hipStream_t stream) {
  if (P <= 0) return hipSuccess;
  if (N < 1 || N >= (1 << 30) || cell < 1 || ny < 1 || nx < 1 || k < 1 || k > kMmMaxK || radius_cm < 1 ||
      radius_cm > 100000)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(mm_candidates_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, stream, start, items, nqy,
                     nqx, N, y0, x0, cell, ny, nx, py, px, P, radius_cm, k, cand, cand_d2, n_cand);
  return hipGetLastError();
}

hipError_t launch_mm_viterbi(const long long* cand_d2, const int* n_cand, const long long* route_cm,
                             const long long* g, const int* npts, int B, int T, int K, long long beta_cm,
                             long long sigma_cm, long long max_detour_cm, int* choice, int* seg, int* nseg,
                             long long* cost, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (T < 1 || T > kMmMaxPoints || K < 1 || K > kMmMaxK || beta_cm < 1 || beta_cm > 10000 || sigma_cm < 1 ||
      sigma_cm > 20000 || max_detour_cm < 1 || max_detour_cm > 500000)
    return hipErrorInvalidValue;
  int KP = 1;
  while (KP < K) KP <<= 1;
  const size_t lds = ((size_t)T * K + (size_t)T + 15) & ~(size_t)15;   // <= 2048 * 17 B, below the 64 KiB default
  hipLaunchKernelGGL(mm_viterbi_kernel, dim3((unsigned)B), dim3(64), lds, stream, cand_d2, n_cand, route_cm, g, npts,
                     B, T, K, KP, beta_cm, 2 * sigma_cm * sigma_cm, max_detour_cm, choice, seg, nseg, cost);
  return hipGetLastError();
}

}  // namespace rt
