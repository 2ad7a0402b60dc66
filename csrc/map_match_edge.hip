// K10 edge mode: map matching to points along road edges (gfx950): the edge candidate search and the
// route centimetres between two points on edges.
//
// The definition (projection in 1/65536 of the edge, the (d2, edge id) candidate order, matchable
// edges, the transition arithmetic and the derivation of the integer bounds) is in
// routest_amd/routing/mapmatch_edge.py; the host C++ is rtr::mm_edge_candidates /
// rtr::mm_edge_route_cm (runtime/map_match.h).  All three are compared with ==.  The Viterbi over the
// route_cm tensor is map_match.hip's mm_viterbi_kernel, unchanged.
//
// mm_edge_candidates_kernel: one wave per fix, four fixes per 256-thread block, map_match.hip's
// row-span walk: the cells the radius covers are row-major, so each covered grid row is ONE
// contiguous span of `items`.  Per item first a bounding-box reject against fix +- radius (from A
// and w, no division), then the projection with its one 64-bit division.  A pass over the spans
// compacts the wave's survivors (ballot + popcount) into a per-wave LDS buffer of keys
// (d2 << 30 | edge) with their fq, so that the k selection rounds ("the smallest key above the
// previous round's", reduced by xor shuffles) run over LDS and the division is done once per item,
// not k times.  An edge listed in several cells sits in the buffer several times; the strict
// key > prev rule skips the copies.  A fix with more survivors than the buffer holds selects by
// rescanning global memory instead (the node kernel's scheme): same keys, same result.  d2 <=
// (1e5 cm)^2 < 2^34 and edge < 2^30, so a key fits an unsigned 64-bit word and is never ~0.
// No atomics, no scratch, no floats; every ballot, shuffle and barrier sits in wave-uniform control
// flow (the span loops run over a wave-uniform base, the survivor count comes from ballots).
//
// mm_edge_route_cm_kernel: elementwise over [rows, K, K].
#include <climits>

#include "common.h"
#include "ops.h"

namespace rt {

namespace {

constexpr int kMmMaxK = 16;
constexpr int kFr = 16;
constexpr long long kHalf = 1LL << (kFr - 1);
constexpr long long kMaxSpan = 1LL << 22;   // |w| per axis of a matchable edge
constexpr int kEdgeCap = 256;               // survivors of one fix kept in LDS (12 B each)
constexpr unsigned long long kNone = ~0ULL;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// One item of a span against the fix: false when the edge id is out of range, its box lies beyond
// the radius or its projection does; else the selection key and fq.  rec: i64 [E, 4] = ay, ax,
// wy | wx << 32, lc.  After the box test |P - A| < 2^22 + 2^17 per axis: every product < 2^62.
__device__ __forceinline__ bool edge_hit(const long long* __restrict__ rec, int E, int e, long long qy, long long qx,
                                         long long radius, long long r2, unsigned long long* key, int* fq) {
  if ((unsigned)e >= (unsigned)E) return false;
  const longlong2 a = reinterpret_cast<const longlong2*>(rec)[2 * (size_t)e];
  const long long packed = rec[4 * (size_t)e + 2];
  const long long wy = (int)(unsigned)(packed & 0xFFFFFFFFLL), wx = (int)(packed >> 32);
  if (wy > kMaxSpan || wy < -kMaxSpan || wx > kMaxSpan || wx < -kMaxSpan) return false;
  const long long dy = qy - a.x, dx = qx - a.y;
  if (dy < (wy < 0 ? wy : 0) - radius || dy > (wy > 0 ? wy : 0) + radius || dx < (wx < 0 ? wx : 0) - radius ||
      dx > (wx > 0 ? wx : 0) + radius)
    return false;
  const long long L2 = wy * wy + wx * wx;
  long long f = dy * wy + dx * wx;
  f = f < 0 ? 0 : (f > L2 ? L2 : f);
  const long long q = L2 > 0 ? (long long)(((unsigned long long)f << kFr) / (unsigned long long)L2) : 0;
  const long long ry = dy - ((wy * q + kHalf) >> kFr), rx = dx - ((wx * q + kHalf) >> kFr);
  const long long d2 = ry * ry + rx * rx;
  if (d2 > r2) return false;
  *key = ((unsigned long long)d2 << 30) | (unsigned)e;
  *fq = (int)q;
  return true;
}

__global__ __launch_bounds__(256) void mm_edge_candidates_kernel(
    const int* __restrict__ start, const int* __restrict__ items, int n_items, const long long* __restrict__ rec, int E,
    long long y0, long long x0, long long cell, int ny, int nx, const long long* __restrict__ py,
    const long long* __restrict__ px, int P, long long radius, int k, int* __restrict__ cand_edge,
    long long* __restrict__ cand_d2, int* __restrict__ cand_fq, int* __restrict__ n_cand, int* __restrict__ n_surv) {
  __shared__ unsigned long long s_key[4][kEdgeCap];
  __shared__ int s_fq[4][kEdgeCap];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int p = blockIdx.x * 4 + w;   // wave-uniform
  const bool live = p < P;            // a wave past the last fix walks no cell and writes nothing
  const long long qy = live ? py[p] : 0, qx = live ? px[p] : 0;
  // the cells the radius covers, clamped to the grid; empty when the fix lies beyond it
  const long long yhi = qy + radius - y0, xhi = qx + radius - x0;
  long long ylo = qy - radius - y0, xlo = qx - radius - x0;
  ylo = ylo < 0 ? 0 : ylo;
  xlo = xlo < 0 ? 0 : xlo;
  int cy0 = 0, cy1 = -1, cx0 = 0, cx1 = -1;
  if (live && yhi >= 0 && xhi >= 0 && ylo / cell < ny && xlo / cell < nx) {
    cy0 = (int)(ylo / cell);
    cx0 = (int)(xlo / cell);
    const long long a = yhi / cell, b = xhi / cell;
    cy1 = a < ny - 1 ? (int)a : ny - 1;
    cx1 = b < nx - 1 ? (int)b : nx - 1;
  }
  const long long r2 = radius * radius;
  // one pass: count the survivors, keep the first kEdgeCap of them in LDS
  int total = 0;
  for (int cy = cy0; cy <= cy1; ++cy) {
    int lo = start[(size_t)cy * nx + cx0], hi = start[(size_t)cy * nx + cx1 + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_items ? n_items : hi;
    for (int base = lo; base < hi; base += 64) {   // wave-uniform bounds
      const int i = base + lane;
      unsigned long long key = 0;
      int fq = 0;
      const bool hit = i < hi && edge_hit(rec, E, items[i], qy, qx, radius, r2, &key, &fq);
      const unsigned long long mask = __ballot(hit);
      if (hit) {
        const int slot = total + __popcll(mask & ((1ULL << lane) - 1ULL));
        if (slot < kEdgeCap) {
          s_key[w][slot] = key;
          s_fq[w][slot] = fq;
        }
      }
      total += __popcll(mask);
    }
  }
  __syncthreads();   // every thread of the block arrives exactly once: the buffer is read below
  const bool in_lds = total <= kEdgeCap;   // wave-uniform
  unsigned long long prev = 0;
  int found = 0;
  for (int m = 0; m < k; ++m) {
    unsigned long long mine = kNone;
    int mine_fq = 0;
    if (in_lds) {
      for (int s = lane; s < total; s += 64) {
        const unsigned long long key = s_key[w][s];
        if ((m == 0 || key > prev) && key < mine) {
          mine = key;
          mine_fq = s_fq[w][s];
        }
      }
    } else {
      for (int cy = cy0; cy <= cy1; ++cy) {
        int lo = start[(size_t)cy * nx + cx0], hi = start[(size_t)cy * nx + cx1 + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_items ? n_items : hi;
        for (int i = lo + lane; i < hi; i += 64) {
          unsigned long long key;
          int fq;
          if (edge_hit(rec, E, items[i], qy, qx, radius, r2, &key, &fq) && (m == 0 || key > prev) && key < mine) {
            mine = key;
            mine_fq = fq;
          }
        }
      }
    }
    const unsigned long long best = wave_min_u64(mine);
    if (best == kNone) break;   // wave-uniform: every lane holds the reduced value
    const unsigned long long who = __ballot(mine == best);   // copies of one edge carry the same fq
    const int fq = __shfl(mine_fq, __ffsll(who) - 1, 64);
    if (lane == 0) {
      cand_edge[(size_t)p * k + m] = (int)(best & ((1ULL << 30) - 1));
      cand_d2[(size_t)p * k + m] = (long long)(best >> 30);
      cand_fq[(size_t)p * k + m] = fq;
    }
    prev = best;
    ++found;
  }
  if (!live) return;
  if (lane == 0) {
    n_cand[p] = found;
    n_surv[p] = total;
  }
  for (int m = found + lane; m < k; m += 64) {
    cand_edge[(size_t)p * k + m] = -1;
    cand_d2[(size_t)p * k + m] = -1;
    cand_fq[(size_t)p * k + m] = -1;
  }
}

__global__ __launch_bounds__(256) void mm_edge_route_cm_kernel(
    const float* __restrict__ met, const int* __restrict__ e1, const long long* __restrict__ off1,
    const long long* __restrict__ lc1, const int* __restrict__ e2, const long long* __restrict__ off2, long long n,
    int K, long long* __restrict__ out) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const long long row = c / ((long long)K * K);
  const int i = (int)((c / K) % K), j = (int)(c % K);
  const long long a = row * K + i, b = row * K + j;
  const int ea = e1[a], eb = e2[b];
  const long long oa = off1[a], ob = off2[b];
  const float m = met[c];
  long long v = -1;
  if (ea >= 0 && eb >= 0) {
    if (ea == eb && ob >= oa)
      v = ob - oa;
    else if (m >= 0.0f && m < INFINITY)   // a NaN fails both
      v = (lc1[a] - oa) + __double2ll_rn((double)m * 100.0) + ob;
  }
  out[c] = v;
}

}  // namespace

int mm_edge_lds_capacity() { return kEdgeCap; }

hipError_t launch_mm_edge_candidates(const int* start, const int* items, int n_items, const long long* rec, int E,
                                     long long y0, long long x0, long long cell, int ny, int nx, const long long* py,
                                     const long long* px, int P, long long radius_cm, int k, int* cand_edge,
                                     long long* cand_d2, int* cand_fq, int* n_cand, int* n_surv, hipStream_t stream) {
  if (P <= 0) return hipSuccess;
  if (E < 1 || E >= (1 << 30) || n_items < 0 || cell < 1 || ny < 1 || nx < 1 || (long long)ny * nx >= INT_MAX ||
      k < 1 || k > kMmMaxK || radius_cm < 1 || radius_cm > 100000)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(mm_edge_candidates_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, stream, start, items,
                     n_items, rec, E, y0, x0, cell, ny, nx, py, px, P, radius_cm, k, cand_edge, cand_d2, cand_fq, n_cand,
                     n_surv);
  return hipGetLastError();
}

hipError_t launch_mm_edge_route_cm(const float* met, const int* e1, const long long* off1, const long long* lc1,
                                   const int* e2, const long long* off2, long long rows, int K, long long* out,
                                   hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (K < 1 || K > kMmMaxK || rows > (1LL << 30)) return hipErrorInvalidValue;   // at most 2^30 blocks
  const long long n = rows * K * K;
  hipLaunchKernelGGL(mm_edge_route_cm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, met, e1, off1,
                     lc1, e2, off2, n, K, out);
  return hipGetLastError();
}

}  // namespace rt
