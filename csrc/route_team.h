// What the trip kernels K6b-K6g (route_improve / route_exchange / route_tw / route_tw_improve /
// route_pd / route_pd_improve .hip) share, each piece defined once: the fixed-point constants and
// quantizers, the team of threads with its reductions, the row prologue, the LDS carve, the two-tier
// launcher and the flat trip order of K6c / K6e / K6g.  Only those six files include this header.
//
// Teams and tiers.  One TEAM of threads works on one request row:
//   * small tier: rows with at most 32 stops, TEAM = one wavefront, four rows per 256-thread block
//     (like K6); only wave barriers, so a wave may leave early;
//   * large tier: rows with more stops, TEAM = one 1024-thread block (a long row fills most of a
//     CU's LDS, so the block's 16 waves are what hides the LDS latency).
// Both tiers are launched over all rows and each row is handled by the tier its stop count picks.
//
// Barrier discipline.  In the large tier Team::sync and every reduction are a __syncthreads, so
// every helper below that says "team-uniform" may only be called from control flow the whole team
// takes alike: every branch and loop bound around such a call depends only on values all threads
// read from LDS (reduction results) or from the same global address.  The per-lane candidate loops
// of the kernels hold no barrier and no cross-lane operation.  Every cross-wave reduction ends
// with a barrier behind its last read of the reduction words, so two reductions may follow each
// other directly.  No global atomics, nothing waits on another team.
#pragma once
#include <climits>

#include "common.h"

namespace rt {
namespace team {

constexpr long long kBig = 1LL << 50;        // an unusable length, time or demand
constexpr long long kUnbounded = 1LL << 62;  // a limit that never binds
constexpr int kUnusable = INT_MAX;           // an unusable matrix entry held as int32
constexpr int kMaxStops = 128;
constexpr int kSmallStops = 32;
constexpr int kLargeTeam = 1024;

// The quantizers are bit-identical to routest_amd/routing/*.py and runtime/route_trips.h.
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

__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_first(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long wave_first(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL));
  const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned int)lo;
}

// a request row as its team sees it; mine: the row exists and this tier owns it
struct Row {
  int team, tid, r, n, ns;
  bool mine;
};

// a lane's place in the candidate scan: CW = a power of two of lanes per row of candidates (so no
// division), the lane's column and first row, and the rows it strides by
struct Lanes {
  int CW, col0, row0, rstep;
};

template <int TEAM>
struct Team {
  static_assert(TEAM == 64 || TEAM == kLargeTeam, "a team is a wavefront or a 1024-thread block");
  static constexpr int TEAMS = TEAM == 64 ? 4 : 1;  // per block
  static constexpr int SHIFT = TEAM == 64 ? 6 : 10;
  static constexpr int WAVES = TEAM / 64;
  static constexpr int BLOCK = TEAM * TEAMS;

  // team-uniform
  static __device__ __forceinline__ void sync() {
    if constexpr (TEAM == 64) {
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS traffic is done
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  }

  // team, tid, r, n (clamped to 0..NM) and ns of this thread's row.  r >= R is wave-uniform in the
  // small tier and never true in the large one; the tier test is uniform over the team.
  static __device__ __forceinline__ Row row(const int* __restrict__ npts, int R, int NM) {
    Row w;
    w.team = TEAM == 64 ? (int)(threadIdx.x >> 6) : 0;
    w.tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    w.r = blockIdx.x * TEAMS + w.team;
    w.n = w.ns = 0;
    w.mine = false;
    if (w.r < R) {
      const int n = npts[w.r];
      w.n = n < 0 ? 0 : (n > NM ? NM : n);
      w.ns = w.n > 0 ? w.n - 1 : 0;
      w.mine = (w.ns <= kSmallStops) == (TEAM == 64);
    }
    return w;
  }

  // ncols >= 2 columns: 2^sh >= ncols, at most the team
  static __device__ __forceinline__ Lanes split(int ncols, int tid) {
    int sh = 32 - __builtin_clz(ncols - 1);
    sh = sh > SHIFT ? SHIFT : sh;
    return {1 << sh, tid & ((1 << sh) - 1), tid >> sh, TEAM >> sh};
  }

  // team-uniform: the sum of v over the team, held by every thread (red: 16 words of the team's LDS)
  static __device__ __forceinline__ long long sum(long long v, long long* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if constexpr (TEAM != 64) {
      if ((tid & 63) == 0) red[tid >> 6] = v;
      __syncthreads();
      v = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) v += red[w];
      __syncthreads();
    }
    return wave_first(v);
  }

  // team-uniform: (max g, then min c) over the team, held by every thread: shuffles in a wave, 16
  // words of LDS each across waves.  The two phases are written differently on purpose, here and in
  // min2: selects in the wave's butterfly, where most steps change the pair, and a branch per word
  // across waves, where few do (measured: profiles/route_team_refactor.md).
  template <class B>
  static __device__ __forceinline__ void best(long long& g, B& c, long long* red_g, B* red_c, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long og = __shfl_xor(g, o);
      const B oc = __shfl_xor(c, o);
      const bool take = og > g || (og == g && oc < c);
      g = take ? og : g;
      c = take ? oc : c;
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
      for (int w = 1; w < WAVES; ++w) {
        const long long og = red_g[w];
        const B oc = red_c[w];
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

  // team-uniform: the lexicographic minimum of (a, b) over the team, held by every thread
  static __device__ __forceinline__ void min2(long long& a, long long& b, long long* red_a, long long* red_b,
                                              int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long oa = __shfl_xor(a, o);
      const long long ob = __shfl_xor(b, o);
      const bool take = oa < a || (oa == a && ob < b);
      a = take ? oa : a;
      b = take ? ob : b;
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
      for (int w = 1; w < WAVES; ++w) {
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
};

// ---- the LDS of one team, carved from the dynamic region.  A kernel describes its arrays once, in
// a constexpr struct whose constructor takes them from an LdsCarve in order: the launch reads the
// struct's byte size, the kernel its offsets, so the two cannot disagree.
__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
// the row stride of a (kc + 1)^2 matrix: odd, so a column walk spreads over the banks
__host__ __device__ constexpr int matrix_stride(int kc) { return (kc + 1) | 1; }

struct LdsCarve {
  size_t bytes = 0;
  // `copies` arrays of `count` elements of `elem` bytes, each padded to a multiple of 16 bytes;
  // the offset of the first
  __host__ __device__ constexpr size_t take(size_t elem, size_t count, int copies = 1) {
    const size_t at = bytes;
    bytes += copies * align16(elem * count);
    return at;
  }
};

// Launches both tiers of a trip kernel over R rows of NM points.  Layout(kc).bytes is one team's LDS
// for a stop capacity of kc; the kernels take kc as their first argument, args... behind it.
template <class Layout, class Kernel, class... Args>
hipError_t launch_two_tiers(Kernel small_kernel, Kernel large_kernel, int R, int NM, hipStream_t stream,
                            Args... args) {
  static_assert(Layout(kMaxStops).bytes <= 160 * 1024, "a row's LDS must fit a CU");
  static_assert(4 * Layout(kSmallStops).bytes <= 64 * 1024, "the small tier stays in the default LDS size");
  if (R == 0) return hipSuccess;
  if (NM < 1 || NM > 4096) return hipErrorInvalidValue;
  // small tier: rows of at most 32 stops, a wavefront each
  {
    const int kc = NM - 1 < kSmallStops ? (NM - 1 < 1 ? 1 : NM - 1) : kSmallStops;
    hipLaunchKernelGGL(small_kernel, dim3((R + 3) / 4), dim3(256), 4 * Layout(kc).bytes, stream, kc, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (NM - 1 <= kSmallStops) return hipSuccess;
  // large tier: a 1024-thread workgroup each; above 64 KB the LDS needs the opt-in size
  const int kc = NM - 1 < kMaxStops ? NM - 1 : kMaxStops;
  const size_t lds = Layout(kc).bytes;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)large_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(large_kernel, dim3(R), dim3(kLargeTeam), lds, stream, kc, args...);
  return hipGetLastError();
}

// ---- the flat trip order of K6c / K6e: the row's stops grouped by trip in the trips' original
// order (so a flat position orders like (trip, index)), the trip of every position and every trip's
// start / count; an emptied trip keeps its index.  Kept in two copies: a move is written into the
// other copy and the copies change roles when it is accepted.  Q is the matrix element type.
struct FlatOrder {
  int *ord, *tof, *tst, *cnt;
  __device__ __forceinline__ FlatOrder copy(int which, int v4) const {
    const int o = which * v4;
    return {ord + o, tof + o, tst + o, cnt + o};
  }
};

// team-uniform: the order from K6's visit / trip_of (bnd: ns words of scratch).  Its first barrier
// also covers whatever the caller wrote to LDS before.
template <int TEAM>
__device__ __forceinline__ void flat_build(const FlatOrder& o, int* bnd, const int* vrow, const int* trow,
                                           int ns, int tid) {
  for (int p = tid; p < ns; p += TEAM) {
    o.ord[p] = vrow[p];
    bnd[p] = p > 0 && trow[p] != trow[p - 1];
  }
  Team<TEAM>::sync();
  for (int p = tid; p < ns; p += TEAM) {
    int t = 0;
    for (int x = 1; x <= p; ++x) t += bnd[x];
    o.tof[p] = t;
    if (p == 0 || bnd[p]) o.tst[t] = p;
  }
  Team<TEAM>::sync();
  for (int p = tid; p < ns; p += TEAM)
    if (p + 1 == ns || bnd[p + 1]) o.cnt[o.tof[p]] = p + 1 - o.tst[o.tof[p]];
  Team<TEAM>::sync();
}

// Lq / Wq of the m trips, one lane per trip; returns the lengths this lane added
template <int TEAM, class Q>
__device__ __forceinline__ long long flat_trip_sums(const FlatOrder& o, int m, const Q* sQ, int S,
                                                    const long long* qd, long long* Lq, long long* Wq,
                                                    int tid) {
  long long part = 0;
  for (int t = tid; t < m; t += TEAM) {
    const int st = o.tst[t], c = o.cnt[t];
    long long L = 0, W = 0;
    int a = 0;
    for (int x = 0; x < c; ++x) {
      const int b = o.ord[st + x];
      L += sQ[a * S + b];
      W += qd[b];
      a = b;
    }
    L += sQ[a * S];
    Lq[t] = L;
    Wq[t] = W;
    part += L;
  }
  return part;
}

// a move as one word that orders like (type, A, i, B, j): A, B <= 127, i, j <= 128.  Type 0 moves
// stop i of trip A behind position j of trip B, type 1 swaps it with stop j of trip B (A < B),
// type 2 is type 0 inside one trip (A == B).
__device__ __forceinline__ long long move_code(int type, int A, int i, int B, int j) {
  return ((long long)type << 32) | ((long long)A << 24) | ((long long)i << 16) | ((long long)B << 8) | j;
}
struct Move {
  int type, A, i, B, j;
};
__device__ __forceinline__ Move decode_move(long long c) {
  return {(int)(c >> 32), (int)(c >> 24) & 255, (int)(c >> 16) & 255, (int)(c >> 8) & 255, (int)c & 255};
}
// what an accepted move adds to Lq / Wq of its trips A and B
struct MoveDelta {
  long long LA, LB, WA, WB;
};

// Writes the order after move mv (of gain g) into the copy nx, one position per thread, and returns
// the move's deltas.  rem / nb / pn are the kernel's per-position terms of the copy o (pn: prev |
// next << 8).  No barrier inside: the caller syncs before nx is read.
template <int TEAM, class Q>
__device__ __forceinline__ MoveDelta flat_write_move(const FlatOrder& o, const FlatOrder& nx, const Move& mv,
                                                     long long g, int ns, int m, const Q* sQ, int S,
                                                     const long long* qd, const long long* rem,
                                                     const long long* nb, const unsigned* pn, int tid) {
  const int mA = mv.A, mB = mv.B, mi = mv.i, mj = mv.j;
  const int pA = o.tst[mA] + mi - 1;
  const int sA = o.ord[pA];
  MoveDelta dl;
  if (mv.type != 1) {
    const int u = mj == 0 ? 0 : o.ord[o.tst[mB] + mj - 1];
    const int v = mj == o.cnt[mB] ? 0 : o.ord[o.tst[mB] + mj];
    if (mv.type == 0) {
      dl.LA = -rem[pA];
      dl.LB = (long long)sQ[u * S + sA] + sQ[sA * S + v] - sQ[u * S + v];
      dl.WA = -qd[sA];
      dl.WB = qd[sA];
    } else {  // one trip: its length drops by the gain
      dl.LA = -g;
      dl.LB = dl.WA = dl.WB = 0;
    }
    // the target behind the source: the stops between move one place to the front; else one back
    const bool fwd = mB > mA || (mB == mA && mj > mi);
    const int dst = fwd ? o.tst[mB] + mj - 1 : o.tst[mB] + mj;
    for (int p = tid; p < ns; p += TEAM) {
      int src = p;
      if (fwd) {
        if (p >= pA && p < dst) src = p + 1;
      } else {
        if (p > dst && p <= pA) src = p - 1;
      }
      nx.ord[p] = p == dst ? sA : o.ord[src];
      nx.tof[p] = p == dst ? mB : o.tof[src];
    }
    for (int t = tid; t < m; t += TEAM) {
      int st = o.tst[t];
      if (mB > mA) {
        if (t > mA && t <= mB) --st;
      } else {
        if (t > mB && t <= mA) ++st;
      }
      nx.tst[t] = st;
      nx.cnt[t] = o.cnt[t] + (t == mB) - (t == mA);
    }
  } else {
    const int pB = o.tst[mB] + mj - 1;
    const int sB = o.ord[pB];
    const unsigned pna = pn[pA], pnb = pn[pB];
    dl.LA = (long long)sQ[(pna & 255) * S + sB] + sQ[sB * S + ((pna >> 8) & 255)] - nb[pA];
    dl.LB = (long long)sQ[(pnb & 255) * S + sA] + sQ[sA * S + ((pnb >> 8) & 255)] - nb[pB];
    dl.WA = qd[sB] - qd[sA];
    dl.WB = -dl.WA;
    for (int p = tid; p < ns; p += TEAM) {
      nx.ord[p] = p == pA ? sB : (p == pB ? sA : o.ord[p]);
      nx.tof[p] = o.tof[p];
    }
    for (int t = tid; t < m; t += TEAM) {
      nx.tst[t] = o.tst[t];
      nx.cnt[t] = o.cnt[t];
    }
  }
  return dl;
}

// team-uniform: acceptance as the greedy measures it.  The f64 legs and demands of the trips the
// move touched (one for type 2) are staged from the written copy nx into dv / dm ([2] arrays of
// stride v8) in parallel and one lane per trip adds them in visiting order, the only place where
// float association matters; true when every walk stays within maxd / cap.  An emptied trip is not
// walked under SKIP_EMPTIED; otherwise its depot -> depot entry is tested like any other trip.
template <int TEAM, bool SKIP_EMPTIED>
__device__ __forceinline__ bool flat_accept(const FlatOrder& nx, const Move& mv, const double* d,
                                            const double* dem, int NM, double MD, double CAP, double* dv,
                                            double* dm, int v8, int* verdict, int tid) {
  const int walks = mv.type == 2 ? 1 : 2;
  for (int x = 0; x < walks; ++x) {
    const int t = x == 0 ? mv.A : mv.B;
    const int st = nx.tst[t], c = nx.cnt[t];
    if (SKIP_EMPTIED && c == 0) continue;
    for (int e = tid; e <= c; e += TEAM) {
      const int a = e == 0 ? 0 : nx.ord[st + e - 1];
      const int b = e == c ? 0 : nx.ord[st + e];
      dv[x * v8 + e] = d[(size_t)a * NM + b];
      if (e < c) dm[x * v8 + e] = dem[b];
    }
  }
  Team<TEAM>::sync();
  if (tid < 2) {
    int ok = 1;
    if (tid < walks) {
      const int c = nx.cnt[tid == 0 ? mv.A : mv.B];
      if (!SKIP_EMPTIED || c > 0) {
        const double* wv = dv + tid * v8;
        const double* wm = dm + tid * v8;
        double s = 0.0, load = 0.0;
        for (int p = 0; p < c; ++p) {
          s += wv[p];
          load += wm[p];
        }
        ok = (s + wv[c] <= MD && load <= CAP) ? 1 : 0;
      }
    }
    verdict[tid] = ok;
  }
  Team<TEAM>::sync();
  return verdict[0] != 0 && verdict[1] != 0;
}

// one lane: Lq / Wq take an accepted move's deltas
__device__ __forceinline__ void flat_commit(long long* Lq, long long* Wq, const Move& mv, const MoveDelta& dl) {
  Lq[mv.A] += dl.LA;
  Wq[mv.A] += dl.WA;
  if (mv.type != 2) {
    Lq[mv.B] += dl.LB;
    Wq[mv.B] += dl.WB;
  }
}

// one lane: rank[t] = the number of non-empty trips before t; returns their count, `after` their length
__device__ __forceinline__ int flat_rank(const int* cnt, const long long* Lq, int m, int* rank,
                                         long long& after) {
  int k = 0;
  after = 0;
  for (int t = 0; t < m; ++t) {
    rank[t] = k;
    if (cnt[t] > 0) {
      ++k;
      after += Lq[t];
    }
  }
  return k;
}

}  // namespace team
}  // namespace rt
