// GPU customizable contraction hierarchy, customization: per routing context, the edge costs and
// from them the metric the queries read (csrc/cch_query.hip).  Preprocessing (node order, chordal
// supergraph, elimination tree, levels) is host C++ (csrc/runtime/cch.h) and metric-independent;
// everything here is per metric, all on the device, bit-identical to that file's CPU reference:
//
//  * context costs: 2E ETA records (edge traffic level shifted by the context's congestion, the
//    context's weather and week-hour) -> the fused featurize+MLP kernel -> seconds per edge;
//  * basic customization, bottom-up by etree HEIGHT: every node z relaxes all pairs (u, v) of its
//    upward clique (lower triangle z of arc {u, v}) with a 64-bit atomicMin on a (weight bits, middle
//    node) word — ties resolve deterministically, exactly like the CPU reference — and each arc is
//    finalized (its best triangle's two sub-arcs and the metres and road edges it stands for);
//  * perfect customization, top-down: every arc (x, y) takes the min over x's other arcs c of the
//    candidate through z = head(c) (the intermediate / upper triangles);
//  * pruning: an arc direction is kept for queries iff its perfect weight equals its basic one;
//    kept arcs are compacted into 16-byte records {weight, head depth, arc id} per node (hipCUB scan).
//
// The two middle phases run one of two paths, chosen once per graph (build_tables):
//
//  * accelerated (the default): a triangle table holds the arc of every pair of a node's upward
//    arcs.  Basic: one launch per height of basic_task_kernel over a precomputed task table (a wave
//    per row of triangles).  Perfect: a PULL over precomputed per-arc records, one launch per depth,
//    plain stores.  On top of that (ROUTEST_CCH_DENSE, default on) the chains at the top of the etree
//    are dense supernodal fronts, customized by blocked (min, +) elimination (sup_*_kernel); the task
//    table and the pull then cover only the nodes outside the fronts;
//  * fallback (the tables do not fit ROUTEST_CCH_TRI_GB of HBM, or could not be built): one launch
//    per height of basic_level_kernel and per depth of perfect_level_kernel, work items flattened
//    over the level, every pair's arc found by binary search, atomics in both phases.
//
// customize() runs the phases in order on the caller's stream with an event between them; background
// builds may be paced (launch_pieces).
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "cch_dev.h"
#include "cch_gpu.h"
#include "ops.h"
#include "runtime/rt_core.h"

namespace rt {

using namespace cchd;

namespace {

using EtaRecordDev = rtc::EtaRecord;

// largest i in [lo, hi) with ofs[i] <= g  (per item, from global memory: staging the block's slice of
// ofs in LDS and searching that instead measured the same level-kernel times, r4x — the levels are
// bound by their gathers and atomics, not by this search)
__device__ __forceinline__ int item_owner(const int64_t* __restrict__ ofs, int lo, int hi, long long g) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ofs[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void fill_u64_kernel(unsigned long long* __restrict__ p, long long n, unsigned long long v) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = v;
}

__global__ void edge_scatter_kernel(const float* __restrict__ cost, const int32_t* __restrict__ edge_arc,
                                    const uint8_t* __restrict__ edge_dir, int E, unsigned long long* __restrict__ up,
                                    unsigned long long* __restrict__ dn) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int a = edge_arc[e];
  const float c = cost[e];
  if (a < 0 || c == INFINITY) return;           // a self loop; an edge this metric closes (absent)
  atomicMin(edge_dir[e] ? dn + a : up + a, packw(c, EDGE_FLAG_D | (uint32_t)e));
}

struct LevelArgs {
  const int32_t* up_ptr;
  const int32_t* up_head;
  const int32_t* nodes;    // level-ordered node list
  const int64_t* ofs;      // item prefix over that list
  int lo, hi;              // node index range of this level
  long long base, items;
};

// one-time triangle table: item g -> (rank z, pair q) -> arc of the pair's heads
__global__ void tri_build_kernel(const int32_t* __restrict__ up_ptr, const int32_t* __restrict__ up_head,
                                 const int64_t* __restrict__ tofs, int N, long long T, int32_t* __restrict__ tri) {
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < T; g += (long long)gridDim.x * blockDim.x) {
    const int z = item_owner(tofs, 0, N, g);
    const long long q = g - tofs[z];
    const int a0 = up_ptr[z];
    const int k = up_ptr[z + 1] - a0;
    const double kk = (double)(2 * k - 1);
    int i = (int)((kk - sqrt(kk * kk - 8.0 * (double)q)) * 0.5);
    if (i < 0) i = 0;
    auto row0 = [&](int r) { return (long long)r * (2 * k - r - 1) / 2; };
    while (i > 0 && row0(i) > q) --i;
    while (i + 1 < k && row0(i + 1) <= q) ++i;
    const int j = (int)(q - row0(i)) + i + 1;
    tri[g] = find_arc_d(up_ptr, up_head, up_head[a0 + i], up_head[a0 + j]);
  }
}

// The two steps of the basic customization, shared by its fallback kernel (basic_level_kernel) and
// its task kernel (basic_task_kernel).
//
// Finalize arc a = (z, v) once every lower triangle has been relaxed into it: the best triangle's two
// sub-arcs (or the road edge), the metres and the road edges the arc stands for (all lower arcs are
// final; the sub-arcs by binary search: one pair per arc, not one per triangle).
__device__ __forceinline__ void basic_finalize_arc(int a, int z, int v, const int32_t* __restrict__ up_ptr,
                                                   const int32_t* __restrict__ up_head,
                                                   const unsigned long long* __restrict__ up,
                                                   const unsigned long long* __restrict__ dn,
                                                   int32_t* __restrict__ sub_up, int32_t* __restrict__ sub_dn,
                                                   float* __restrict__ len_up, float* __restrict__ len_dn,
                                                   int32_t* __restrict__ cnt_up, int32_t* __restrict__ cnt_dn,
                                                   const float* __restrict__ length) {
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const unsigned long long w = dir ? dn[a] : up[a];
    int32_t* sub = (dir ? sub_dn : sub_up) + 2 * (long long)a;
    float* len = dir ? len_dn : len_up;
    int32_t* cnt = dir ? cnt_dn : cnt_up;
    if (!(wof(w) < F_INF)) {
      sub[0] = -1;
      sub[1] = -1;
      len[a] = F_INF;
      cnt[a] = 0;
      continue;
    }
    const uint32_t pl = (uint32_t)w;
    if (pl & EDGE_FLAG_D) {
      const int e = (int)(pl & ~EDGE_FLAG_D);
      sub[0] = -1;
      sub[1] = e;
      len[a] = length[e];
      cnt[a] = 1;
      continue;
    }
    const int zz = (int)pl;
    const int azu = find_arc_d(up_ptr, up_head, zz, z), azv = find_arc_d(up_ptr, up_head, zz, v);
    const int s0 = dir ? azv : azu, s1 = dir ? azu : azv;
    sub[0] = s0;
    sub[1] = s1;
    len[a] = len_dn[s0] + len_up[s1];
    cnt[a] = cnt_dn[s0] + cnt_up[s1];     // road edges the arc stands for (cooperative unpack)
  }
}

// Relax the lower triangle z of the pair (ai, aj) of z's upward arcs (heads u < v) into t, the arc
// {u, v}: u -> z -> v takes (z,u) down and (z,v) up, v -> z -> u takes (z,v) down and (z,u) up.
// A candidate is sent to the atomic only if it beats the target's current value (a plain load; a
// stale value is only ever larger, so nothing that could win is skipped) — most of a target's
// candidates lose, and the 64-bit atomics were the level kernels' L2 traffic (round 5).
__device__ __forceinline__ void basic_relax_pair(int z, int ai, int aj, int t, unsigned long long* __restrict__ up,
                                                 unsigned long long* __restrict__ dn) {
  const float wu = wof(dn[ai]) + wof(up[aj]);
  const float wd = wof(dn[aj]) + wof(up[ai]);
  if (wu < F_INF) {
    const unsigned long long pu = packw(wu, (uint32_t)z);
    if (pu < up[t]) atomicMin(up + t, pu);
  }
  if (wd < F_INF) {
    const unsigned long long pd = packw(wd, (uint32_t)z);
    if (pd < dn[t]) atomicMin(dn + t, pd);
  }
}

// Fallback basic customization of one height level (no triangle table): items [0, k) of node z
// finalize arc k-th of z; items [k, k + k(k-1)/2) relax the lower triangle z of one pair of z's
// upward neighbours, whose arc a binary search finds.  Work items are FLATTENED over the level (a
// binary search maps an item to its node), so the top of the hierarchy — one node per level with a
// clique of hundreds — still spreads over the whole chip.
__global__ __launch_bounds__(256) void basic_level_kernel(LevelArgs L, unsigned long long* __restrict__ up,
                                                          unsigned long long* __restrict__ dn,
                                                          int32_t* __restrict__ sub_up, int32_t* __restrict__ sub_dn,
                                                          float* __restrict__ len_up, float* __restrict__ len_dn,
                                                          int32_t* __restrict__ cnt_up, int32_t* __restrict__ cnt_dn,
                                                          const float* __restrict__ length) {
  const long long gi = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (gi >= L.items) return;
  const long long g = L.base + gi;
  const int ni = item_owner(L.ofs, L.lo, L.hi, g);
  const int z = L.nodes[ni];
  const long long p = g - L.ofs[ni];
  const int a0 = L.up_ptr[z];
  const int k = L.up_ptr[z + 1] - a0;
  if (p < k) {
    const int a = a0 + (int)p;
    basic_finalize_arc(a, z, L.up_head[a], L.up_ptr, L.up_head, up, dn, sub_up, sub_dn, len_up, len_dn, cnt_up, cnt_dn,
                       length);
    return;
  }
  // pair (i, j), i < j, row-major over i
  const long long q = p - k;
  const double kk = (double)(2 * k - 1);
  int i = (int)((kk - sqrt(kk * kk - 8.0 * (double)q)) * 0.5);
  if (i < 0) i = 0;
  auto row0 = [&](int r) { return (long long)r * (2 * k - r - 1) / 2; };
  while (i > 0 && row0(i) > q) --i;
  while (i + 1 < k && row0(i + 1) <= q) ++i;
  const int j = (int)(q - row0(i)) + i + 1;
  const int ai = a0 + i, aj = a0 + j;
  const int t = find_arc_d(L.up_ptr, L.up_head, L.up_head[ai], L.up_head[aj]);
  if (t < 0) return;   // cannot happen in a chordal completion
  basic_relax_pair(z, ai, aj, t, up, dn);
}

// Accelerated basic customization (round 5): a wave's work is one precomputed, metric-independent
// TASK (built once per graph in height order, build_tasks) with its node's arc range and its
// triangle row's base folded in (24 bytes), and its 64 lanes take 64 consecutive columns.  That
// replaces the per-item chain of the flattened kernel (binary search for the item's node, node id,
// arc range, the pair decode by sqrt, the pair's arc by binary search) — a ~6-deep chain of dependent
// global loads per wave — by one scalar load of the task, and the lanes' loads are coalesced along a
// row of the triangle table.
struct BasicTask {
  int64_t rowbase;   // pair rows: tofs[z] + i (2k - i - 1) / 2 - i - 1 (column j's triangle at rowbase + j)
  int32_t node;
  int32_t a0;        // z's first upward arc
  uint16_t k;        // z's upward arcs
  uint16_t row;      // pair row i, or ROW_FINAL
  uint16_t col0;     // first column of the wave's 64
  uint16_t pad;
};
static_assert(sizeof(BasicTask) == 24, "basic task layout");
constexpr uint16_t ROW_FINAL = 0xFFFF;

// One task per wave: a pair row (i, j0 .. j0+63) of node z relaxes its lower triangles z of the
// arcs {head i, head j}; a ROW_FINAL task finalizes 64 of z's own arcs.  Same math as
// basic_level_kernel (bit-identical).
__global__ __launch_bounds__(256) void basic_task_kernel(const BasicTask* __restrict__ tasks, long long ntask,
                                                         const int32_t* __restrict__ up_ptr,
                                                         const int32_t* __restrict__ up_head,
                                                         const int32_t* __restrict__ tri,
                                                         unsigned long long* __restrict__ up,
                                                         unsigned long long* __restrict__ dn, int32_t* __restrict__ sub_up,
                                                         int32_t* __restrict__ sub_dn, float* __restrict__ len_up,
                                                         float* __restrict__ len_dn, int32_t* __restrict__ cnt_up,
                                                         int32_t* __restrict__ cnt_dn, const float* __restrict__ length) {
  const long long ti = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ti >= ntask) return;
  const BasicTask& T = tasks[ti];
  const int lane = threadIdx.x & 63;
  const int z = T.node;
  const int a0 = T.a0;
  const int k = T.k;
  if (T.row == ROW_FINAL) {
    const int p = T.col0 + lane;
    if (p >= k) return;
    const int a = a0 + p;
    basic_finalize_arc(a, z, up_head[a], up_ptr, up_head, up, dn, sub_up, sub_dn, len_up, len_dn, cnt_up, cnt_dn,
                       length);
    return;
  }
  const int i = T.row;
  const int j = T.col0 + lane;
  if (j >= k) return;
  const int t = tri[T.rowbase + j];
  if (t < 0) return;
  basic_relax_pair(z, a0 + i, a0 + j, t, up, dn);
}

__global__ void perfect_init_kernel(const unsigned long long* __restrict__ up, const unsigned long long* __restrict__ dn,
                                    uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn, long long M) {
  for (long long a = blockIdx.x * (long long)blockDim.x + threadIdx.x; a < M; a += (long long)gridDim.x * blockDim.x) {
    pup[a] = (uint32_t)(up[a] >> 32);
    pdn[a] = (uint32_t)(dn[a] >> 32);
  }
}

// Fallback perfect customization of one depth level (no triangle table): ordered pairs (c, a),
// a != c, of node x's arcs; the candidate for arc a = (x, y) goes through z = head(c): x -> z on c
// (basic), z -> y on {z, y} (perfect: an arc between two ancestors, finished by an earlier level;
// found by binary search).  Consecutive items share c and spread over a (different atomic targets);
// 32-bit atomicMin on the float bits, sent only if it beats the current value (basic_relax_pair).
__global__ __launch_bounds__(256) void perfect_level_kernel(LevelArgs L, const unsigned long long* __restrict__ up,
                                                            const unsigned long long* __restrict__ dn,
                                                            uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn) {
  const long long gi = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (gi >= L.items) return;
  const long long g = L.base + gi;
  const int ni = item_owner(L.ofs, L.lo, L.hi, g);
  const int x = L.nodes[ni];
  const long long p = g - L.ofs[ni];
  const int a0 = L.up_ptr[x];
  const int k = L.up_ptr[x + 1] - a0;
  const int c = (int)(p / (k - 1));
  const int r = (int)(p % (k - 1));
  const int a = r < c ? r : r + 1;
  const int ac = a0 + c, aa = a0 + a;
  const int y = L.up_head[aa], z = L.up_head[ac];
  const int azy = find_arc_d(L.up_ptr, L.up_head, z < y ? z : y, z < y ? y : z);
  if (azy < 0) return;
  const float xz = wof(up[ac]), zx = wof(dn[ac]);
  const float zy = __uint_as_float(z < y ? pup[azy] : pdn[azy]);
  const float yz = __uint_as_float(z < y ? pdn[azy] : pup[azy]);
  const float cu = xz + zy, cd = yz + zx;
  if (cu < F_INF && __float_as_uint(cu) < pup[aa]) atomicMin(pup + aa, __float_as_uint(cu));
  if (cd < F_INF && __float_as_uint(cd) < pdn[aa]) atomicMin(pdn + aa, __float_as_uint(cd));
}

// Perfect customization as a PULL over one depth level (round 5): every arc a = (x, y) of the
// level's nodes takes the min over x's other arcs c of the candidate through z = head(c), and is
// written once with a plain store — the level owns its arcs, so no atomics and no per-item decode.
// Same candidate set and fp32 sums as the fallback's push kernel / the CPU reference (bit-identical).
//
// Per level-ordered arc, one record holds everything the pull needs before its candidate loads, in
// one load — instead of a binary search over the level's nodes (a level of thousands of nodes
// searched ~12 dependent steps per wave) and the dependent loads of the node's arc range, triangle
// offset and the arc's head.
struct PArc {
  int64_t tb;        // the node's triangle table offset
  int32_t a0;        // x's first upward arc
  int32_t y;         // the arc's head
  uint16_t k;        // x's upward arcs
  uint16_t ia;       // the arc's index among them
  int32_t pad;
};
static_assert(sizeof(PArc) == 24, "pull arc record");

struct PullArgs {
  const int32_t* up_head;
  const int32_t* tri;      // triangle table
  const PArc* parc;        // the records, in level order (d_parc by depth, d_parc2 by depth below a front)
  long long base, arcs;    // the level's (piece of) records
};

__device__ __forceinline__ void pull_cand(const PullArgs& P, long long tb, int k, int a0, int ia, int ic, float xz_c,
                                          float zx_c, const uint32_t* __restrict__ pup, const uint32_t* __restrict__ pdn,
                                          int y, int z, float& bu, float& bd) {
  const int i = ic < ia ? ic : ia, j = ic < ia ? ia : ic;
  const int azy = P.tri[tb + (long long)i * (2 * k - i - 1) / 2 + (j - i - 1)];
  const float zy = __uint_as_float(z < y ? pup[azy] : pdn[azy]);
  const float yz = __uint_as_float(z < y ? pdn[azy] : pup[azy]);
  const float cu = xz_c + zy, cd = yz + zx_c;
  bu = cu < bu ? cu : bu;
  bd = cd < bd ? cd : bd;
}

// The wave's minimum over candidate chunks c_begin, c_begin + c_step, ... of arc (x -> y) = x's arc
// ia (x: arcs a0 .. a0 + k, triangle rows at tb): four 64-wide chunks of candidates per step, every
// stage's loads issued together (the serial tri -> weight chain of a high-degree node's ~22 chunks
// was the kernel's latency); bu / bd are reduced over the wave.
__device__ __forceinline__ void pull_arc_min(const PullArgs& P, long long tb, int a0, int k, int ia, int y, int c_begin,
                                             int c_step, int lane, const unsigned long long* __restrict__ up,
                                             const unsigned long long* __restrict__ dn, const uint32_t* __restrict__ pup,
                                             const uint32_t* __restrict__ pdn, float& bu, float& bd) {
  for (int c0 = c_begin; c0 < k; c0 += c_step) {
    int azy[4], z[4];
    unsigned long long wu[4], wd[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ic = c0 + 64 * u + lane;
      ok[u] = ic < k && ic != ia;
      const int i = ic < ia ? ic : ia, j = ic < ia ? ia : ic;
      azy[u] = ok[u] ? P.tri[tb + (long long)i * (2 * k - i - 1) / 2 + (j - i - 1)] : 0;
      z[u] = ok[u] ? P.up_head[a0 + ic] : 0;
      wu[u] = ok[u] ? up[a0 + ic] : 0ull;
      wd[u] = ok[u] ? dn[a0 + ic] : 0ull;
    }
    uint32_t gu[4], gd[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gu[u] = ok[u] ? pup[azy[u]] : 0u;
      gd[u] = ok[u] ? pdn[azy[u]] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      const float zy = __uint_as_float(z[u] < y ? gu[u] : gd[u]);
      const float yz = __uint_as_float(z[u] < y ? gd[u] : gu[u]);
      const float cu = wof(wu[u]) + zy, cd = yz + wof(wd[u]);
      bu = cu < bu ? cu : bu;
      bd = cd < bd ? cd : bd;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ou = __shfl_xor(bu, o), od = __shfl_xor(bd, o);
    bu = ou < bu ? ou : bu;
    bd = od < bd ? od : bd;
  }
}

// S waves per arc (4 / S arcs per workgroup), lanes over the node's other arcs, wave `part` of an
// arc taking candidate chunks part, part + S, ... (levels of high-degree nodes: the top separators,
// k up to ~1400 on the 1M-node city — one wave walked ~6 chunks of 256 candidates one after the
// other; split, each wave walks k / (256 S)).  The parts' minima meet in LDS (min is exact and
// order-free: bit-identical to one wave).
template <int S>
__global__ __launch_bounds__(256) void perfect_pull_wave_kernel(PullArgs P, const unsigned long long* __restrict__ up,
                                                                const unsigned long long* __restrict__ dn,
                                                                uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn) {
  static_assert(S == 1 || S == 2 || S == 4, "waves per arc");
  constexpr int APB = 4 / S;
  __shared__ float red[2][4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * APB + w / S;
  const int part = w % S;
  const bool active = g < P.arcs;
  float bu = F_INF, bd = F_INF;
  int aa = 0;
  if (active) {
    const PArc pa = P.parc[P.base + g];
    aa = pa.a0 + pa.ia;
    pull_arc_min(P, pa.tb, pa.a0, pa.k, pa.ia, pa.y, 256 * part, 256 * S, lane, up, dn, pup, pdn, bu, bd);
  }
  if constexpr (S > 1) {
    if (lane == 0) {
      red[0][w] = bu;
      red[1][w] = bd;
    }
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int q = 1; q < S; ++q) {
      const float ou = red[0][w + q], od = red[1][w + q];
      bu = ou < bu ? ou : bu;
      bd = od < bd ? od : bd;
    }
  }
  if (active && lane == 0) {
    const float cu = __uint_as_float(pup[aa]), cd = __uint_as_float(pdn[aa]);
    if (bu < cu) pup[aa] = __float_as_uint(bu);
    if (bd < cd) pdn[aa] = __float_as_uint(bd);
  }
}

// one lane per arc, looping over the node's other arcs (levels of low-degree nodes)
__global__ __launch_bounds__(256) void perfect_pull_lane_kernel(PullArgs P, const unsigned long long* __restrict__ up,
                                                                const unsigned long long* __restrict__ dn,
                                                                uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.arcs) return;
  const PArc pa = P.parc[P.base + g];
  const long long tb = pa.tb;
  const int a0 = pa.a0, k = pa.k, ia = pa.ia, y = pa.y;
  const int aa = a0 + ia;
  float bu = __uint_as_float(pup[aa]), bd = __uint_as_float(pdn[aa]);
  for (int ic = 0; ic < k; ++ic) {
    if (ic == ia) continue;
    const int ac = a0 + ic;
    pull_cand(P, tb, k, a0, ia, ic, wof(up[ac]), wof(dn[ac]), pup, pdn, y, P.up_head[ac], bu, bd);
  }
  pup[aa] = __float_as_uint(bu);
  pdn[aa] = __float_as_uint(bd);
}

__device__ __forceinline__ bool kept(uint32_t p, unsigned long long b) {
  return __uint_as_float(p) < F_INF && p == (uint32_t)(b >> 32);
}

// Pruning, one wave per node: lanes over its arcs (coalesced), ballot counts and in-order
// positions (round 5; a thread per node walking its arcs serially took 1.5 ms per customization
// on the 100k graph)
__global__ __launch_bounds__(256) void prune_count_wave_kernel(const int32_t* __restrict__ up_ptr,
                                                               const uint32_t* __restrict__ pup,
                                                               const uint32_t* __restrict__ pdn,
                                                               const unsigned long long* __restrict__ up,
                                                               const unsigned long long* __restrict__ dn, int N,
                                                               int32_t* __restrict__ fcnt, int32_t* __restrict__ bcnt) {
  const int x = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (x >= N) return;
  int kf = 0, kb = 0;
  for (int a = up_ptr[x] + lane; a < up_ptr[x + 1]; a += 64) {
    kf += kept(pup[a], up[a]);
    kb += kept(pdn[a], dn[a]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    kf += __shfl_xor(kf, o);
    kb += __shfl_xor(kb, o);
  }
  if (lane == 0) {
    fcnt[x] = kf;
    bcnt[x] = kb;
  }
}

__global__ __launch_bounds__(256) void prune_scatter_wave_kernel(
    const int32_t* __restrict__ up_ptr, const int32_t* __restrict__ up_head, const int32_t* __restrict__ depth,
    const uint32_t* __restrict__ pup, const uint32_t* __restrict__ pdn, const unsigned long long* __restrict__ up,
    const unsigned long long* __restrict__ dn, int N, const int32_t* __restrict__ f_ptr, const int32_t* __restrict__ b_ptr,
    int4* __restrict__ f_rec, int4* __restrict__ b_rec) {
  const int x = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (x >= N) return;
  int kf = f_ptr[x], kb = b_ptr[x];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int a0 = up_ptr[x]; a0 < up_ptr[x + 1]; a0 += 64) {
    const int a = a0 + lane;
    const bool in = a < up_ptr[x + 1];
    const bool f = in && kept(pup[a], up[a]);
    const bool b = in && kept(pdn[a], dn[a]);
    const unsigned long long mf = __ballot(f), mb = __ballot(b);
    if (f || b) {
      const int hd = depth[up_head[a]];        // records in arc order, like the serial kernel
      if (f) f_rec[kf + __popcll(mf & below)] = make_int4((int)pup[a], hd, a, 0);
      if (b) b_rec[kb + __popcll(mb & below)] = make_int4((int)pdn[a], hd, a, 0);
    }
    kf += __popcll(mf);
    kb += __popcll(mb);
  }
}

// ---- supernodal customization of the top of the elimination tree (round 6) ----
// The top ~80 % of the etree levels are the nested-dissection separators: CHAINS of nodes (each the
// only child of the next), one etree level per node, so the per-level kernels above walk them one
// ~12 us level at a time (963 levels per phase on the 100k graph, profiles/cch_customize_r6.md).
// A chain with its upper set is a dense FRONT (chordality: every chain node's upward arcs lead into
// the chain above it or into the top node's upward set), and its customization is dense (min, +)
// elimination: basic = tropical Gaussian elimination of the chain's pivots (a triangle z of pair
// {u, v} is "pivot z updates D[u][v]"), perfect = tropical back substitution from the top.  Blocked
// 32 pivots at a time, a level of the supernode tree takes 2 (basic) / 3 (perfect) launches per
// block instead of one launch per node — and every candidate is the same single f32 add of the
// same two operands as in the per-level kernels (min is exact and order-free), so the results are
// bit-identical to them and to the CPU reference (csrc/runtime/cch.h).
// A front's D is row-major n x n over its nodes in rank order (chain c0 .. c0 + m - 1 first, then
// the top's upward set): D[i][j] = weight f_i -> f_j — basic: the packed (weight, middle) word,
// perfect: two f32 matrices (basic Db, perfect P) in the same bytes.  farc[i][j]: the arc of
// {f_i, f_j} (-1: none).  Entries between two upper-set nodes (U x U) are only ever TARGETS here
// (their arcs belong to an ancestor front): basic sends them with one atomicMin each at the end.
struct SupNode {
  int64_t dofs;      // first entry of the front in the level's dense buffer
  int64_t foff;      // first entry of its farc table
  int32_t c0, m, n;  // first chain rank, chain length, front size
  int32_t fnode;     // offset of its node list
};
struct SupWork {
  int32_t s, b, t0, t1;   // supernode, block (or row), tile indices
  SupNode sn;             // the front itself (one load per workgroup instead of two dependent ones)
};
constexpr int SUP_B = 32;      // pivots per block
constexpr int SUP_PJ = 32;     // basic panel: front columns per workgroup
constexpr int SUP_TT = 64;     // basic trailing update: 64 x 64 targets per workgroup
constexpr int SUP_G1Y = 32;    // perfect GEMM: 32 output columns per workgroup
constexpr int SUP_G1Z = 128;   // ... over at most 128 intermediate nodes (more: split, atomicMin)
constexpr int SUP_SJ = 64;     // perfect solve: front columns per workgroup

__device__ __forceinline__ unsigned long long sup_cand(unsigned long long a, unsigned long long b, uint32_t z) {
  const float w = wof(a) + wof(b);
  return w < F_INF ? packw(w, z) : PACK_INF_D;
}
__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

// farc of every front row (once per graph): a wave per row
__global__ __launch_bounds__(256) void sup_farc_kernel(const SupNode* __restrict__ sn, const SupWork* __restrict__ w,
                                                       long long nw, const int32_t* __restrict__ fnode,
                                                       const int32_t* __restrict__ up_ptr,
                                                       const int32_t* __restrict__ up_head, int32_t* __restrict__ farc) {
  const long long wi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= nw) return;
  const SupWork W = w[wi];
  const SupNode S = W.sn;
  const int i = W.b, n = S.n;
  const int fi = fnode[S.fnode + i];
  for (int j = threadIdx.x & 63; j < n; j += 64) {
    const int fj = fnode[S.fnode + j];
    farc[S.foff + (long long)i * n + j] = i == j ? -1 : find_arc_d(up_ptr, up_head, fi < fj ? fi : fj, fi < fj ? fj : fi);
  }
}

// basic: a front's rows from the arc weights (all lower levels are done; U x U starts at +inf), a
// workgroup per row.  An entry whose best triangle so far has a middle node (necessarily below the
// front: no pivot of it has run) also gets that triangle's finalization now — sub-arcs by binary
// search, metres, road edges — in SS / SL: the elimination only adds middles from the chain, so if
// the entry still has this middle at the end, the panel takes it from here (off its serial path).
__global__ __launch_bounds__(256) void sup_gather_basic_kernel(
    const SupNode* __restrict__ sn, const SupWork* __restrict__ w, const int32_t* __restrict__ fnode,
    const int32_t* __restrict__ farc, const unsigned long long* __restrict__ up, const unsigned long long* __restrict__ dn,
    const int32_t* __restrict__ up_ptr, const int32_t* __restrict__ up_head, const float* __restrict__ len_up,
    const float* __restrict__ len_dn, const int32_t* __restrict__ cnt_up, const int32_t* __restrict__ cnt_dn,
    unsigned long long* __restrict__ D, int2* __restrict__ SS, int2* __restrict__ SL) {
  const SupWork W = w[blockIdx.x];
  const SupNode S = W.sn;
  const int i = W.b, n = S.n;
  const long long r0 = S.dofs + (long long)i * n;
  const int32_t* fr = farc + S.foff + (long long)i * n;
  const int fi = fnode[S.fnode + i];
  for (int j = threadIdx.x; j < n; j += 256) {
    unsigned long long v = PACK_INF_D;
    if (i != j && (i < S.m || j < S.m)) {
      const int a = fr[j];
      if (a >= 0) {
        v = i < j ? up[a] : dn[a];
        const uint32_t pl = (uint32_t)v;
        if (wof(v) < F_INF && !(pl & EDGE_FLAG_D)) {
          const int zz = (int)pl, fj = fnode[S.fnode + j];
          const int lo = i < j ? fi : fj, hi = i < j ? fj : fi;
          const int azx = find_arc_d(up_ptr, up_head, zz, lo), azv = find_arc_d(up_ptr, up_head, zz, hi);
          const int s0 = i < j ? azx : azv, s1 = i < j ? azv : azx;
          SS[r0 + j] = make_int2(s0, s1);
          SL[r0 + j] = make_int2(__float_as_int(len_dn[s0] + len_up[s1]), cnt_dn[s0] + cnt_up[s1]);
        }
      }
    }
    D[r0 + j] = v;
  }
}

// basic, block b of a front: the 32 pivots K = [k0, k1) eliminated in the diagonal block and in the
// row / column panels of this workgroup's 32 front columns J (every workgroup of the front redoes
// the 32 x 32 diagonal block: no inter-workgroup dependency), then the rows of K are final: their
// arcs' weights go out, and they are FINALIZED (best triangle's sub-arcs, metres, road edges —
// basic_finalize_arc): a middle below the front from the gather's SS / SL, one in an earlier
// block from its (final) arcs, and one inside K row by row from LDS (it needs the lengths of an arc
// of K finalized just before).  1024 threads: one entry of each matrix per thread and pivot.
__device__ __forceinline__ void sup_panel_body(
    const SupWork& W, const int32_t* __restrict__ farc, unsigned long long* __restrict__ D, const int2* __restrict__ SS,
    const int2* __restrict__ SL, unsigned long long* __restrict__ up, unsigned long long* __restrict__ dn,
    int32_t* __restrict__ sub_up, int32_t* __restrict__ sub_dn, float* __restrict__ len_up, float* __restrict__ len_dn,
    int32_t* __restrict__ cnt_up, int32_t* __restrict__ cnt_dn, const float* __restrict__ length) {
  constexpr int B = SUP_B, J = SUP_PJ, W2 = SUP_B + SUP_PJ;
  static_assert(B == 32 && J == 32, "one entry of each matrix per thread");
  __shared__ unsigned long long Dk[B][B + 1];   // D[K][K]
  __shared__ unsigned long long R[B][J + 1];    // D[K][J]
  __shared__ unsigned long long C[J][B + 1];    // D[J][K]
  __shared__ int32_t FK[B][W2];                 // arcs of the rows of K: columns K | J
  __shared__ float lu[B][W2], ld[B][W2];        // their finalized metres
  __shared__ int32_t cu[B][W2], cd[B][W2];      // ... and road edges
  const SupNode S = W.sn;
  const int n = S.n, tid = threadIdx.x;
  const int k0 = W.b * B, k1 = min(k0 + B, S.m), kb = k1 - k0;
  const int j0 = k1 + W.t0 * J, nj = max(0, min(J, n - j0));
  const bool diag_writer = W.t0 == 0;
  unsigned long long* Df = D + S.dofs;
  const int32_t* F = farc + S.foff;
  const int ty = tid >> 5, tx = tid & 31;      // (row, column) of this thread's entry of each matrix
  Dk[ty][tx] = (ty < kb && tx < kb) ? Df[(long long)(k0 + ty) * n + k0 + tx] : PACK_INF_D;
  R[ty][tx] = (ty < kb && tx < nj) ? Df[(long long)(k0 + ty) * n + j0 + tx] : PACK_INF_D;
  C[ty][tx] = (tx < kb && ty < nj) ? Df[(long long)(j0 + ty) * n + k0 + tx] : PACK_INF_D;
  FK[ty][tx] = (ty < kb && tx < kb && tx > ty) ? F[(long long)(k0 + ty) * n + k0 + tx] : -1;
  FK[ty][B + tx] = (ty < kb && tx < nj) ? F[(long long)(k0 + ty) * n + j0 + tx] : -1;
  __syncthreads();
  // the block below K (K- = [k0 - 32, k0), its panels finished in the previous launch): its pivots'
  // candidates for this workgroup's entries.  That block's trailing update runs in the same launch
  // as this and leaves the rows and columns of K to here (left-looking for one block).
  if (W.b > 0) {
    const int km = k0 - B;                      // (every block but a front's last is full)
    __shared__ unsigned long long Ay[B][B + 1];   // D[K][K-]
    __shared__ unsigned long long Aj[J][B + 1];   // D[J][K-]
    __shared__ unsigned long long Bx[B][B + 1];   // D[K-][K]
    __shared__ unsigned long long Bj[B][J + 1];   // D[K-][J]
    Ay[ty][tx] = ty < kb ? Df[(long long)(k0 + ty) * n + km + tx] : PACK_INF_D;
    Aj[ty][tx] = ty < nj ? Df[(long long)(j0 + ty) * n + km + tx] : PACK_INF_D;
    Bx[ty][tx] = tx < kb ? Df[(long long)(km + ty) * n + k0 + tx] : PACK_INF_D;
    Bj[ty][tx] = tx < nj ? Df[(long long)(km + ty) * n + j0 + tx] : PACK_INF_D;
    __syncthreads();
    unsigned long long dk = Dk[ty][tx], rr = R[ty][tx], cc = C[ty][tx];
    const bool odk = ty < kb && tx < kb && ty != tx, orr = ty < kb && tx < nj, occ = ty < nj && tx < kb;
    for (int p = 0; p < B; ++p) {
      const uint32_t z = (uint32_t)(S.c0 + km + p);
      if (odk) dk = umin64(dk, sup_cand(Ay[ty][p], Bx[p][tx], z));
      if (orr) rr = umin64(rr, sup_cand(Ay[ty][p], Bj[p][tx], z));
      if (occ) cc = umin64(cc, sup_cand(Aj[ty][p], Bx[p][tx], z));
    }
    Dk[ty][tx] = dk;
    R[ty][tx] = rr;
    C[ty][tx] = cc;
    __syncthreads();
  }
  // pivot p: entries of rows / columns above p (row p and column p are final and only read)
  for (int p = 0; p < kb; ++p) {
    const uint32_t z = (uint32_t)(S.c0 + k0 + p);
    if (ty > p && tx > p && ty < kb && tx < kb && ty != tx) Dk[ty][tx] = umin64(Dk[ty][tx], sup_cand(Dk[ty][p], Dk[p][tx], z));
    if (ty > p && ty < kb && tx < nj) R[ty][tx] = umin64(R[ty][tx], sup_cand(Dk[ty][p], R[p][tx], z));
    if (tx > p && tx < kb && ty < nj) C[ty][tx] = umin64(C[ty][tx], sup_cand(C[ty][p], Dk[p][tx], z));
    __syncthreads();
  }
  if (ty < kb && tx < nj) {
    Df[(long long)(k0 + ty) * n + j0 + tx] = R[ty][tx];
    Df[(long long)(j0 + tx) * n + k0 + ty] = C[tx][ty];
    const int a = FK[ty][B + tx];
    if (a >= 0) {
      up[a] = R[ty][tx];
      dn[a] = C[tx][ty];
    }
  }
  if (diag_writer && ty < kb && tx < kb) {
    Df[(long long)(k0 + ty) * n + k0 + tx] = Dk[ty][tx];
    const int a = FK[ty][tx];
    if (a >= 0) {
      up[a] = Dk[ty][tx];
      dn[a] = Dk[tx][ty];
    }
  }
  // finalize the arcs (x, v), x in K, v in K above x (column v - k0) or in J (column B + j)
  const int zK = S.c0 + k0;     // rank of K's first pivot
  auto vfront = [&](int col) { return col < B ? k0 + col : j0 + col - B; };
  auto weight = [&](int x, int col, int dir) -> unsigned long long {
    if (col < B) return dir ? Dk[col][x] : Dk[x][col];
    return dir ? C[col - B][x] : R[x][col - B];
  };
  auto put = [&](int x, int col, int a, int dir, int s0, int s1, float L, int32_t Cn) {
    (dir ? ld : lu)[x][col] = L;
    (dir ? cd : cu)[x][col] = Cn;
    if (col >= B || diag_writer) {
      int32_t* sub = (dir ? sub_dn : sub_up) + 2 * (long long)a;
      sub[0] = s0;
      sub[1] = s1;
      (dir ? len_dn : len_up)[a] = L;
      (dir ? cnt_dn : cnt_up)[a] = Cn;
    }
  };
  // every entry whose middle is not in K, in two rounds of independent loads: (1) the gather's
  // finalization (middle below the front), a road edge's metres, or the sub-arcs through an earlier
  // block's node; (2) those sub-arcs' metres and road edges
  {
    constexpr int Q = B * W2 / 1024;
    int kind[Q][2], s0[Q][2], s1[Q][2];
    float L[Q][2];
    int32_t Cn[Q][2];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = tid + 1024 * q, x = e / W2, col = e % W2;
      const int a = FK[x][col];
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        kind[q][dir] = 0;
        if (a < 0) continue;
        const unsigned long long wt = weight(x, col, dir);
        const uint32_t pl = (uint32_t)wt;
        const int vf = vfront(col);
        if (!(wof(wt) < F_INF)) {
          kind[q][dir] = 1;
          s0[q][dir] = -1;
          s1[q][dir] = -1;
          L[q][dir] = F_INF;
          Cn[q][dir] = 0;
        } else if (pl & EDGE_FLAG_D) {
          const int ed = (int)(pl & ~EDGE_FLAG_D);
          kind[q][dir] = 1;
          s0[q][dir] = -1;
          s1[q][dir] = ed;
          L[q][dir] = length[ed];
          Cn[q][dir] = 1;
        } else if ((int)pl < S.c0) {           // below the front: the gather's
          const long long idx = dir ? (long long)vf * n + k0 + x : (long long)(k0 + x) * n + vf;
          const int2 ss = SS[S.dofs + idx], sl = SL[S.dofs + idx];
          kind[q][dir] = 1;
          s0[q][dir] = ss.x;
          s1[q][dir] = ss.y;
          L[q][dir] = __int_as_float(sl.x);
          Cn[q][dir] = sl.y;
        } else if ((int)pl < zK) {             // an earlier block of the chain
          const long long fz = (int)pl - S.c0;
          const int azx = F[fz * n + k0 + x], azv = F[fz * n + vf];
          kind[q][dir] = 2;
          s0[q][dir] = dir ? azv : azx;
          s1[q][dir] = dir ? azx : azv;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int dir = 0; dir < 2; ++dir)
        if (kind[q][dir] == 2) {
          L[q][dir] = len_dn[s0[q][dir]] + len_up[s1[q][dir]];
          Cn[q][dir] = cnt_dn[s0[q][dir]] + cnt_up[s1[q][dir]];
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = tid + 1024 * q, x = e / W2, col = e % W2;
#pragma unroll
      for (int dir = 0; dir < 2; ++dir)
        if (kind[q][dir]) put(x, col, FK[x][col], dir, s0[q][dir], s1[q][dir], L[q][dir], Cn[q][dir]);
    }
  }
  __syncthreads();
  for (int x = 1; x < kb; ++x) {
    if (tid < 2 * W2) {
      const int dir = tid / W2, col = tid % W2;
      const int a = FK[x][col];
      const unsigned long long wt = a >= 0 ? weight(x, col, dir) : PACK_INF_D;
      const uint32_t pl = (uint32_t)wt;
      const int zl = (int)pl - zK;
      if (wof(wt) < F_INF && !(pl & EDGE_FLAG_D) && zl >= 0) {
        // zl < x: row zl is final (the round above or an earlier row here); arc (z, x) is its column x
        const int azx = FK[zl][x], azv = FK[zl][col];
        if (dir == 0)
          put(x, col, a, 0, azx, azv, ld[zl][x] + lu[zl][col], cd[zl][x] + cu[zl][col]);
        else
          put(x, col, a, 1, azv, azx, ld[zl][col] + lu[zl][x], cd[zl][col] + cu[zl][x]);
      }
    }
    __syncthreads();
  }
}

// basic, block b: the trailing update of the front's targets above the next block up — for every
// (y, z), both past k1' (the end of the block above K; k1 for a front's last block), the best pivot p
// in K of D[y][p] + D[p][z] (ties: the lowest pivot = the smallest middle rank, as the packed
// atomicMin); the rows and columns of the block above K get theirs in its panel (same launch as this).
// U x U targets go to their arcs with one atomicMin after the last block.  1024 threads, 64 x 64
// targets, four per thread.
__device__ __forceinline__ void sup_trailing_body(const SupWork& W, const int32_t* __restrict__ farc,
                                                  unsigned long long* __restrict__ D, unsigned long long* __restrict__ up,
                                                  unsigned long long* __restrict__ dn) {
  constexpr int B = SUP_B, T = SUP_TT;
  __shared__ float A[T][B + 1];     // weights D[y][K]
  __shared__ float Bm[B][T + 1];    // weights D[K][z]
  const SupNode S = W.sn;
  const int n = S.n, m = S.m, tid = threadIdx.x;
  const int nb = (m + B - 1) / B;
  const int k0 = W.b * B, k1 = min(k0 + B, m), kb = k1 - k0;
  const int zr0 = W.b + 1 < nb ? min(k1 + B, m) : k1;
  const int y0 = zr0 + W.t0 * T, z0 = zr0 + W.t1 * T;
  unsigned long long* Df = D + S.dofs;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = tid + 1024 * h;
    {
      const int r = e / B, p = e % B;
      A[r][p] = (y0 + r < n && p < kb) ? wof(Df[(long long)(y0 + r) * n + k0 + p]) : F_INF;
    }
    {
      const int p = e / T, c = e % T;
      Bm[p][c] = (p < kb && z0 + c < n) ? wof(Df[(long long)(k0 + p) * n + z0 + c]) : F_INF;
    }
  }
  // the targets' current words, loaded now (their latency hides behind the loop below)
  const int ty = tid >> 4, tz = tid & 15;
  const int y = y0 + ty;
  unsigned long long old[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int z = z0 + tz + 16 * j;
    old[j] = (y < n && z < n && y != z) ? Df[(long long)y * n + z] : PACK_INF_D;
  }
  __syncthreads();
  float bw[4];
  int bp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bw[j] = F_INF;
    bp[j] = 0;
  }
  for (int p = 0; p < kb; ++p) {
    const float a = A[ty][p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sum = a + Bm[p][tz + 16 * j];
      if (sum < bw[j]) {        // strict: the first (lowest) pivot keeps a tie
        bw[j] = sum;
        bp[j] = p;
      }
    }
  }
  const bool last = k1 == m;
  const int32_t* F = farc + S.foff;
  unsigned long long nv[4];
  int arc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int z = z0 + tz + 16 * j;
    const unsigned long long c = bw[j] < F_INF ? packw(bw[j], (uint32_t)(S.c0 + k0 + bp[j])) : PACK_INF_D;
    nv[j] = umin64(old[j], c);
    arc[j] = -1;
    if (y >= n || z >= n || y == z) continue;
    if (y >= m && z >= m && last) {
      if (nv[j] != PACK_INF_D) arc[j] = F[(long long)y * n + z];
    } else if (c < old[j]) {
      Df[(long long)y * n + z] = c;
    }
  }
  if (!last) return;
  unsigned long long cur[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int z = z0 + tz + 16 * j;
    cur[j] = arc[j] >= 0 ? (y < z ? up : dn)[arc[j]] : 0ull;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int z = z0 + tz + 16 * j;
    if (arc[j] >= 0 && nv[j] < cur[j]) atomicMin((y < z ? up : dn) + arc[j], nv[j]);
  }
}

// one launch per block step of the basic phase: the panels of block r of every front (work items
// with t1 < 0) beside the trailing updates of block r - 1 (1024 threads)
__global__ __launch_bounds__(1024) void sup_step_basic_kernel(
    const SupWork* __restrict__ w, const int32_t* __restrict__ farc, unsigned long long* __restrict__ D,
    const int2* __restrict__ SS, const int2* __restrict__ SL, unsigned long long* __restrict__ up,
    unsigned long long* __restrict__ dn, int32_t* __restrict__ sub_up, int32_t* __restrict__ sub_dn,
    float* __restrict__ len_up, float* __restrict__ len_dn, int32_t* __restrict__ cnt_up, int32_t* __restrict__ cnt_dn,
    const float* __restrict__ length) {
  const SupWork W = w[blockIdx.x];
  if (W.t1 < 0)
    sup_panel_body(W, farc, D, SS, SL, up, dn, sub_up, sub_dn, len_up, len_dn, cnt_up, cnt_dn, length);
  else
    sup_trailing_body(W, farc, D, up, dn);
}

// perfect: a front's basic weights (f32) of every pair with a chain node, and the perfect weights
// of U x U (final: an ancestor front's or an earlier level's); the diagonal is +inf (no candidate
// through the target's own head)
__global__ __launch_bounds__(256) void sup_gather_perfect_kernel(const SupNode* __restrict__ sn,
                                                                 const SupWork* __restrict__ w, long long nw,
                                                                 const int32_t* __restrict__ farc,
                                                                 const unsigned long long* __restrict__ up,
                                                                 const unsigned long long* __restrict__ dn,
                                                                 const uint32_t* __restrict__ pup,
                                                                 const uint32_t* __restrict__ pdn, float* __restrict__ D) {
  const long long wi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= nw) return;
  const SupWork W = w[wi];
  const SupNode S = W.sn;
  const int i = W.b, n = S.n;
  float* Db = D + 2 * S.dofs;
  float* P = Db + (long long)n * n;
  const int32_t* fr = farc + S.foff + (long long)i * n;
  for (int j = threadIdx.x & 63; j < n; j += 64) {
    float db = F_INF, p = F_INF;
    const int a = fr[j];
    if (i != j && a >= 0) {
      if (i < S.m || j < S.m) {
        db = wof(i < j ? up[a] : dn[a]);
        p = db;
      } else {
        p = __uint_as_float(i < j ? pup[a] : pdn[a]);
      }
    }
    Db[(long long)i * n + j] = db;
    P[(long long)i * n + j] = p;
  }
}

// perfect, block b (blocks from the top): the candidates through the final part above the next
// block up, F' = [k1', n) (k1' = the end of the block above K; the whole F = [k1, n) for a front's top
// block) — up: P[x][y] = min_z Db[x][z] + P[z][y], dn: P[y][x] = min_z P[y][z] + Db[z][x]  (x in K,
// y in F, z in F') — a (min, +) product, 32 x 32 outputs per workgroup over <= SUP_G1Z z (t1 = split
// << 1 | dir).  The block above K (z in [k1, k1')) is added by sup_solve_perfect_kernel: it is only
// final after that block's K x K kernel, which runs in the same launch as this (no data shared).
__device__ __forceinline__ void sup_gemm_body(const SupWork& W, float* __restrict__ D) {
  constexpr int B = SUP_B, ZC = 64;
  __shared__ float As[32][ZC + 1];
  __shared__ float Bs[ZC][33];
  const SupNode S = W.sn;
  const int n = S.n, tid = threadIdx.x;
  const int nb = (S.m + B - 1) / B;
  const int k0 = W.b * B, k1 = min(k0 + B, S.m), kb = k1 - k0;
  const int zlo = W.b + 1 < nb ? min(k1 + B, S.m) : k1;
  const int y0 = k1 + W.t0 * SUP_G1Y, ny = min(SUP_G1Y, n - y0);
  const int dir = W.t1 & 1, zs = W.t1 >> 1;
  const int zbeg = zlo + zs * SUP_G1Z, zend = min(zbeg + SUP_G1Z, n);
  const bool split = n - zlo > SUP_G1Z;
  float* Db = D + 2 * S.dofs;
  float* P = Db + (long long)n * n;
  const int r = tid >> 5, c = tid & 31;
  float best = F_INF;
  for (int zc = zbeg; zc < zend; zc += ZC) {
    const int nz = min(ZC, zend - zc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = tid + 1024 * h;
      {
        const int rr = e / ZC, q = e % ZC;
        float v = F_INF;
        if (q < nz) {
          if (dir == 0 && rr < kb) v = Db[(long long)(k0 + rr) * n + zc + q];
          if (dir == 1 && rr < ny) v = P[(long long)(y0 + rr) * n + zc + q];
        }
        As[rr][q] = v;
      }
      {
        const int q = e / 32, cc = e % 32;
        float v = F_INF;
        if (q < nz) {
          if (dir == 0 && cc < ny) v = P[(long long)(zc + q) * n + y0 + cc];
          if (dir == 1 && cc < kb) v = Db[(long long)(zc + q) * n + k0 + cc];
        }
        Bs[q][cc] = v;
      }
    }
    __syncthreads();
    for (int q = 0; q < nz; ++q) {
      const float sum = As[r][q] + Bs[q][c];
      best = sum < best ? sum : best;
    }
    __syncthreads();
  }
  if (!(best < F_INF)) return;
  long long idx;
  if (dir == 0) {
    if (r >= kb || c >= ny) return;
    idx = (long long)(k0 + r) * n + y0 + c;
  } else {
    if (r >= ny || c >= kb) return;
    idx = (long long)(y0 + r) * n + k0 + c;
  }
  if (split) atomicMin((uint32_t*)(P + idx), __float_as_uint(best));
  else if (best < P[idx]) P[idx] = best;
}

// perfect, block b: the rows of K against this workgroup's 64 columns y of F, top-down through K
// (candidates through z in K above x), then written out; and the F-part of the K x K targets through
// these 64 z (atomicMin into P[K][K], finished by sup_kk_body in the next launch).  1024 threads: two entries
// of each direction per thread and step.
__global__ __launch_bounds__(1024) void sup_solve_perfect_kernel(const SupNode* __restrict__ sn,
                                                                 const SupWork* __restrict__ w,
                                                                 const int32_t* __restrict__ farc, float* __restrict__ D,
                                                                 uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn) {
  constexpr int B = SUP_B, Y = SUP_SJ;
  static_assert(B * Y == 2048, "two entries per thread");
  __shared__ float Dk[B][B + 1];     // Db[K][K]
  __shared__ float PU[B][Y + 1];     // P[K][y]
  __shared__ float PD[Y][B + 1];     // P[y][K]
  __shared__ float DKT[B][Y + 1];    // Db[K][y]
  __shared__ float DTK[Y][B + 1];    // Db[y][K]
  const SupWork W = w[blockIdx.x];
  const SupNode S = W.sn;
  const int n = S.n, tid = threadIdx.x;
  const int k0 = W.b * B, k1 = min(k0 + B, S.m), kb = k1 - k0;
  const int y0 = k1 + W.t0 * Y, ny = min(Y, n - y0);
  float* Db = D + 2 * S.dofs;
  float* P = Db + (long long)n * n;
  {
    const int y = tid >> 5, x = tid & 31;
    Dk[y][x] = (y < kb && x < kb) ? Db[(long long)(k0 + y) * n + k0 + x] : F_INF;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 1024 * q;
    {
      const int x = e / Y, y = e % Y;
      const bool ok = x < kb && y < ny;
      PU[x][y] = ok ? P[(long long)(k0 + x) * n + y0 + y] : F_INF;
      DKT[x][y] = ok ? Db[(long long)(k0 + x) * n + y0 + y] : F_INF;
    }
    {
      const int y = e / B, x = e % B;
      const bool ok = x < kb && y < ny;
      PD[y][x] = ok ? P[(long long)(y0 + y) * n + k0 + x] : F_INF;
      DTK[y][x] = ok ? Db[(long long)(y0 + y) * n + k0 + x] : F_INF;
    }
  }
  __syncthreads();
  // the block above K, K' = [k1, k2) (finished in the previous launches: its rows by its solve, its
  // K' x K' by its K x K kernel): its candidates for this workgroup's entries (the product left it out)
  const int nbk = (S.m + B - 1) / B;
  if (W.b + 1 < nbk) {
    const int k2 = min(k1 + B, S.m), kb2 = k2 - k1;
    __shared__ float A2[B][B + 1];    // Db[K][K']
    __shared__ float E2[B][B + 1];    // Db[K'][K]
    __shared__ float B2[B][Y + 1];    // P[K'][y]
    __shared__ float C2[Y][B + 1];    // P[y][K']
    {
      const int y = tid >> 5, x = tid & 31;
      A2[y][x] = (y < kb && x < kb2) ? Db[(long long)(k0 + y) * n + k1 + x] : F_INF;
      E2[y][x] = (y < kb2 && x < kb) ? Db[(long long)(k1 + y) * n + k0 + x] : F_INF;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 1024 * q;
      {
        const int z = e / Y, y = e % Y;
        B2[z][y] = (z < kb2 && y < ny) ? P[(long long)(k1 + z) * n + y0 + y] : F_INF;
      }
      {
        const int y = e / B, z = e % B;
        C2[y][z] = (z < kb2 && y < ny) ? P[(long long)(y0 + y) * n + k1 + z] : F_INF;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 1024 * q;
      {
        const int x = e / Y, y = e % Y;
        if (x < kb && y < ny) {
          float v = PU[x][y];
          for (int z = 0; z < kb2; ++z) {
            const float c = A2[x][z] + B2[z][y];
            v = c < v ? c : v;
          }
          PU[x][y] = v;
        }
      }
      {
        const int y = e / B, x = e % B;
        if (x < kb && y < ny) {
          float v = PD[y][x];
          for (int z = 0; z < kb2; ++z) {
            const float c = C2[y][z] + E2[z][x];
            v = c < v ? c : v;
          }
          PD[y][x] = v;
        }
      }
    }
    __syncthreads();
  }
  // top-down through K, four pivots z0 > z1 > z2 > z3 per barrier: every thread first finishes the
  // group's own entries of its column (u_i = P[z_i][y] through z_j, j < i) from LDS, then applies
  // all four to its entry (a group row stores its u).  A group row may be read while its owner
  // stores it: the value read is either the old one or the finished one, and u_i comes out the same
  // (its candidates are recomputed either way) — every candidate is the same single add as one pivot
  // per step, so the minima are bit-identical.
  for (int zt = kb - 1; zt >= 1; zt -= 4) {
    const int G = min(4, zt);                 // members zt, zt - 1, ..., zt - G + 1 (>= 1)
    const int zb = zt - G + 1;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 1024 * q;
      {
        const int x = e / Y, y = e % Y;
        if (x < zt && y < ny) {
          float u[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (i >= G) break;
            float v = PU[zt - i][y];
#pragma unroll
            for (int j = 0; j < i; ++j) {
              const float c = Dk[zt - i][zt - j] + u[j];
              v = c < v ? c : v;
            }
            u[i] = v;
          }
          if (x < zb) {
            float v = PU[x][y];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (i >= G) break;
              const float c = Dk[x][zt - i] + u[i];
              v = c < v ? c : v;
            }
            PU[x][y] = v;
          } else {
            PU[x][y] = u[zt - x];
          }
        }
      }
      {
        const int y = e / B, x = e % B;
        if (x < zt && y < ny) {
          float u[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (i >= G) break;
            float v = PD[y][zt - i];
#pragma unroll
            for (int j = 0; j < i; ++j) {
              const float c = u[j] + Dk[zt - j][zt - i];
              v = c < v ? c : v;
            }
            u[i] = v;
          }
          if (x < zb) {
            float v = PD[y][x];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (i >= G) break;
              const float c = u[i] + Dk[zt - i][x];
              v = c < v ? c : v;
            }
            PD[y][x] = v;
          } else {
            PD[y][x] = u[zt - x];
          }
        }
      }
    }
    __syncthreads();
  }
  const int32_t* F = farc + S.foff;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 1024 * q, x = e / Y, y = e % Y;
    if (x < kb && y < ny) {
      const long long iu = (long long)(k0 + x) * n + y0 + y;
      P[iu] = PU[x][y];
      P[(long long)(y0 + y) * n + k0 + x] = PD[y][x];
      const int a = F[iu];
      if (a >= 0) {
        pup[a] = __float_as_uint(PU[x][y]);
        pdn[a] = __float_as_uint(PD[y][x]);
      }
    }
  }
  {
    const int x = tid >> 5, y = tid & 31;
    if (x < y && y < kb) {
      float bu = F_INF, bd = F_INF;
      for (int q = 0; q < ny; ++q) {
        const float su = DKT[x][q] + PD[q][y];
        const float sd = PU[y][q] + DTK[q][x];
        bu = su < bu ? su : bu;
        bd = sd < bd ? sd : bd;
      }
      if (bu < F_INF) atomicMin((uint32_t*)(P + (long long)(k0 + x) * n + k0 + y), __float_as_uint(bu));
      if (bd < F_INF) atomicMin((uint32_t*)(P + (long long)(k0 + y) * n + k0 + x), __float_as_uint(bd));
    }
  }
}

// perfect, block b: the K x K targets top-down (x from the top of K: all of its candidates through
// z in K above x are final), one workgroup per front; 16 lanes per target split the z loop
__device__ __forceinline__ void sup_kk_body(const SupWork& W, const int32_t* __restrict__ farc, float* __restrict__ D,
                                            uint32_t* __restrict__ pup, uint32_t* __restrict__ pdn) {
  constexpr int B = SUP_B;
  __shared__ float Dk[B][B + 1];
  __shared__ float Pk[B][B + 1];
  const SupNode S = W.sn;
  const int n = S.n, tid = threadIdx.x;
  const int k0 = W.b * B, k1 = min(k0 + B, S.m), kb = k1 - k0;
  float* Db = D + 2 * S.dofs;
  float* P = Db + (long long)n * n;
  {
    const int y = tid >> 5, x = tid & 31;
    const bool ok = y < kb && x < kb;
    Dk[y][x] = ok ? Db[(long long)(k0 + y) * n + k0 + x] : F_INF;
    Pk[y][x] = ok ? P[(long long)(k0 + y) * n + k0 + x] : F_INF;
  }
  __syncthreads();
  const int g = tid >> 4, q = tid & 15;
  const int dir = g >> 5, y = g & 31;
  for (int x = kb - 2; x >= 0; --x) {
    float best = F_INF;
    if (y > x && y < kb)
      for (int z = x + 1 + q; z < kb; z += 16) {
        if (z == y) continue;
        const float s = dir == 0 ? Dk[x][z] + Pk[z][y] : Pk[y][z] + Dk[z][x];
        best = s < best ? s : best;
      }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float v = __shfl_xor(best, o);
      best = v < best ? v : best;
    }
    if (q == 0 && y > x && y < kb) {
      if (dir == 0) {
        if (best < Pk[x][y]) Pk[x][y] = best;
      } else {
        if (best < Pk[y][x]) Pk[y][x] = best;
      }
    }
    __syncthreads();
  }
  const int32_t* F = farc + S.foff;
  {
    const int x = tid >> 5, yy = tid & 31;
    if (x < kb && yy < kb) {
      const long long idx = (long long)(k0 + x) * n + k0 + yy;
      P[idx] = Pk[x][yy];
      if (x < yy) {
        const int a = F[idx];
        if (a >= 0) {
          pup[a] = __float_as_uint(Pk[x][yy]);
          pdn[a] = __float_as_uint(Pk[yy][x]);
        }
      }
    }
  }
}

// one launch per block step of the perfect phase: the K x K kernels of the blocks solved in the
// previous launch (work items with t0 < 0) beside the products of the next blocks down (1024 threads)
__global__ __launch_bounds__(1024) void sup_kk_gemm_perfect_kernel(const SupWork* __restrict__ w,
                                                                   const int32_t* __restrict__ farc,
                                                                   float* __restrict__ D, uint32_t* __restrict__ pup,
                                                                   uint32_t* __restrict__ pdn) {
  const SupWork W = w[blockIdx.x];
  if (W.t0 < 0) sup_kk_body(W, farc, D, pup, pdn);
  else sup_gemm_body(W, D);
}

// ---- context costs (routing/graph.py edge_records / edge_costs) ----
constexpr float L_REF_M = 10000.f;
constexpr int32_t MONDAY_2025_08_25 = 2063 * 86400;   // seconds since 2020-01-01 (a Monday)

__global__ void ctx_records_kernel(const uint8_t* __restrict__ base_traffic, int E, int weather, int congestion,
                                   int weekhour, float age, EtaRecordDev* __restrict__ rec) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int lvl = (int)base_traffic[e] + congestion - 1;
  lvl = lvl < 0 ? 0 : (lvl > 3 ? 3 : lvl);
  // TRAFFIC_LEVELS (Low, Medium, High, Jam) -> features.py traffic codes (High 0, Jam 1, Low 2, Medium 3)
  const uint8_t code = (uint8_t)((0x01000302u >> (8 * lvl)) & 0xFF);
  EtaRecordDev r;
  r.distance_m = L_REF_M;
  r.driver_age = age;
  r.wallclock_s = MONDAY_2025_08_25 + weekhour * 3600;
  r.weather = (uint8_t)weather;
  r.traffic = code;
  r.pad = 0;
  rec[2 * (long long)e] = r;
  r.distance_m = 0.f;
  rec[2 * (long long)e + 1] = r;
}

__global__ void ctx_cost_kernel(const float* __restrict__ minutes, const float* __restrict__ length,
                                const uint8_t* __restrict__ road_class, int E, float* __restrict__ cost) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float k60 = (float)(60.0 / 10000.0);
  const float rate = (minutes[2 * (long long)e] - minutes[2 * (long long)e + 1]) * k60;
  const float cf[4] = {1.15f, 1.0f, 0.85f, 0.65f};
  const float sec = rate * length[e] * cf[road_class[e] & 3];
  const float floor_s = length[e] / (float)(130.0 / 3.6);
  cost[e] = sec > floor_s ? sec : floor_s;
}

}  // namespace

// The customization's path, chosen once per graph.  Accelerated: the triangle table within
// ROUTEST_CCH_TRI_GB of HBM (default 48 — a 1M-node city needs ~38 GB of the 288; 0 disables), the
// basic task table, the pull records and (optionally: ROUTEST_CCH_DENSE) the supernodal fronts.  If any
// of the three required tables cannot be built — no room, an allocation failure, a node with more
// than 0xFFFE upward arcs — all are freed and every customization takes the fallback path.
void CchGpu::build_tables() {
  const int N = T_.N;
  std::vector<int64_t> tofs(N + 1, 0);
  for (int z = 0; z < N; ++z) {
    const int64_t k = T_.up_ptr[z + 1] - T_.up_ptr[z];
    tofs[z + 1] = tofs[z] + k * (k - 1) / 2;
  }
  const char* env = std::getenv("ROUTEST_CCH_TRI_GB");
  const double budget = env ? std::atof(env) : 48.0;
  const int64_t T = tofs[N];
  if (!(T > 0 && (double)T * 4.0 <= budget * 1073741824.0 && T < ((int64_t)1 << 40))) return;
  accel_ = build_triangles(tofs);
  if (accel_) build_supernodes(tofs);       // (before the tasks: they leave the fronts' nodes out)
  accel_ = accel_ && build_tasks(tofs) && build_pull_records(tofs);
  if (!accel_) {
    (void)hipGetLastError();
    free_tables();
  }
}

void CchGpu::free_tables() {
  dfree(d_tri);
  dfree(d_btask);
  dfree(d_parc);
  dfree(d_sup_sn);
  dfree(d_sup_work);
  dfree(d_sup_fnode);
  dfree(d_sup_farc);
  dfree(d_parc2);
  dfree(cs0_.sup_buf);
  n_tri = n_btask_ = 0;
  sup_on_ = false;
  sup_lev_.clear();
  rlev_nodes_.clear();
  sup_fronts_ = sup_nodes_ = sup_blocks_ = sparse_heights_ = 0;
}

bool CchGpu::build_triangles(const std::vector<int64_t>& tofs) {
  const int N = T_.N;
  const int64_t T = tofs[N];
  int64_t* dofs = nullptr;
  bool ok = up_copy(dofs, tofs.data(), N + 1) == hipSuccess && dmalloc(d_tri, (size_t)T) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(tri_build_kernel, dim3((unsigned)std::min<int64_t>(65536, (T + 255) / 256)), dim3(256), 0, 0,
                       d_up_ptr, d_up_head, dofs, N, (long long)T, d_tri);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  dfree(dofs);                            // (the tasks and pull records carry their nodes' offsets)
  if (ok) n_tri = T;
  return ok;
}

// The supernodal plan (metric-independent, once per graph).  A supernode is a maximal chain of ranks
// c0, c0 + 1, ... in which every node is the only child of the next; the chains of at least
// ROUTEST_CCH_DENSE nodes (default 8; 0: off) and all their ancestor chains are dense fronts, levelled
// by height in the tree of fronts.  Per level: the gather rows, and per block the panel / trailing
// (basic) and GEMM / solve / K x K (perfect) workgroup lists.  The nodes outside the fronts keep the
// per-level kernels: basic by etree height (their heights end far below the top), perfect by depth
// below their nearest front (all of their ancestors inside fronts are final by then).
void CchGpu::build_supernodes(const std::vector<int64_t>& tofs) {
  const char* v = std::getenv("ROUTEST_CCH_DENSE");
  const int S0 = v ? std::atoi(v) : 8;
  const int N = T_.N;
  if (S0 <= 0 || N < 2) return;
  std::vector<int> nch(N, 0);
  for (int i = 0; i < N; ++i)
    if (T_.parent[i] >= 0) ++nch[T_.parent[i]];
  std::vector<int> sid(N), sc0, ssz;
  for (int i = 0; i < N; ++i) {
    if (!(i > 0 && T_.parent[i - 1] == i && nch[i] == 1)) {
      sc0.push_back(i);
      ssz.push_back(0);
    }
    sid[i] = (int)sc0.size() - 1;
    ++ssz.back();
  }
  const int NS = (int)sc0.size();
  std::vector<int> spar(NS, -1);
  for (int s = 0; s < NS; ++s) {
    const int p = T_.parent[sc0[s] + ssz[s] - 1];
    spar[s] = p >= 0 ? sid[p] : -1;
  }
  std::vector<uint8_t> dense(NS, 0);
  for (int s = 0; s < NS; ++s)
    if (ssz[s] >= S0)
      for (int q = s; q >= 0 && !dense[q]; q = spar[q]) dense[q] = 1;
  std::vector<int> lev(NS, 0);       // children precede parents (ranks grow upward)
  int L = 0;
  for (int s = 0; s < NS; ++s) {
    if (!dense[s]) continue;
    L = std::max(L, lev[s] + 1);
    if (spar[s] >= 0) lev[spar[s]] = std::max(lev[spar[s]], lev[s] + 1);
  }
  if (L == 0) return;
  // fronts: chain, then the top node's upward set; every chain arc must lead into the front
  std::vector<SupNode> sn;
  std::vector<int32_t> fnode;
  std::vector<std::vector<int>> by_lev(L);
  int64_t foff = 0;
  for (int s = 0; s < NS; ++s) {
    if (!dense[s]) continue;
    const int c0 = sc0[s], m = ssz[s], top = c0 + m - 1;
    const int64_t a0 = T_.up_ptr[top], a1 = T_.up_ptr[top + 1];
    const int64_t n = m + (a1 - a0);
    if (n > 32767) return;
    const int32_t* U0 = T_.up_head.data() + a0;
    const int32_t* U1 = T_.up_head.data() + a1;
    for (int i = 0; i < m; ++i)
      for (int64_t a = T_.up_ptr[c0 + i]; a < T_.up_ptr[c0 + i + 1]; ++a) {
        const int h = T_.up_head[a];
        if (!((h > c0 + i && h <= top) || std::binary_search(U0, U1, h))) {
          std::fprintf(stderr, "[cch] rank %d: arc to %d outside its front; supernodal customization off\n", c0 + i, h);
          return;
        }
      }
    by_lev[lev[s]].push_back((int)sn.size());
    sn.push_back(SupNode{0, foff, c0, m, (int32_t)n, (int32_t)fnode.size()});
    for (int i = 0; i < m; ++i) fnode.push_back(c0 + i);
    fnode.insert(fnode.end(), U0, U1);
    foff += n * n;
  }
  const auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  std::vector<SupWork> work;
  auto range_of = [&](int64_t from) { return SupRange{from, (int64_t)work.size() - from}; };
  // every front row (farc build)
  for (int f = 0; f < (int)sn.size(); ++f)
    for (int i = 0; i < sn[f].n; ++i) work.push_back(SupWork{f, i, 0, 0});
  const SupRange all_rows = range_of(0);
  // the trailing update of front f's block b: targets past the end of the block above it
  auto push_trail = [&](int f, int b) {
    const SupNode& S = sn[f];
    const int nb = (int)cdiv(S.m, SUP_B);
    const int k1 = std::min(SUP_B * (b + 1), S.m);
    const int zr0 = b + 1 < nb ? std::min(k1 + SUP_B, S.m) : k1;
    const int T = (int)cdiv(S.n - zr0, SUP_TT);
    for (int ty = 0; ty < T; ++ty)
      for (int tz = 0; tz < T; ++tz) work.push_back(SupWork{f, b, ty, tz});
  };
  std::vector<SupLevel> levs(L);
  int64_t buf = 0;
  int blocks = 0;
  for (int l = 0; l < L; ++l) {
    SupLevel& SL = levs[l];
    int64_t dofs = 0;
    int nbmax = 0;
    for (int f : by_lev[l]) {
      sn[f].dofs = dofs;
      dofs += (int64_t)sn[f].n * sn[f].n;
      nbmax = std::max(nbmax, (int)cdiv(sn[f].m, SUP_B));
    }
    buf = std::max(buf, dofs);
    blocks += nbmax;
    int64_t w0 = (int64_t)work.size();
    for (int f : by_lev[l])
      for (int i = 0; i < sn[f].n; ++i) work.push_back(SupWork{f, i, 0, 0});
    SL.gather = range_of(w0);
    for (int r = 0; r < nbmax; ++r) {
      // basic, step r: the panels of every front's block r (t1 = -1) beside the trailing updates of
      // its block r - 1 (sup_step_basic_kernel)
      w0 = (int64_t)work.size();
      for (int f : by_lev[l]) {
        const SupNode& S = sn[f];
        const int nb = (int)cdiv(S.m, SUP_B);
        if (nb > r) {
          const int k1 = std::min(SUP_B * (r + 1), S.m);
          const int nt = std::max<int64_t>(1, cdiv(S.n - k1, SUP_PJ));
          for (int t = 0; t < nt; ++t) work.push_back(SupWork{f, r, t, -1});
        }
        if (r >= 1 && nb > r - 1) push_trail(f, r - 1);
      }
      SL.panel.push_back(range_of(w0));
      // perfect, launch pair r: [the K x K kernels of the blocks solved at r - 1 | the products of
      // the r-th blocks from the top], then the r-th blocks' solves
      w0 = (int64_t)work.size();
      for (int f : by_lev[l]) {
        const SupNode& S = sn[f];
        const int nb = (int)cdiv(S.m, SUP_B);
        if (r >= 1 && nb > r - 1) work.push_back(SupWork{f, nb - r, -1, 0});
        if (nb <= r) continue;
        const int b = nb - 1 - r, k1 = std::min(SUP_B * (b + 1), S.m), nF = S.n - k1;
        const int zlo = b + 1 < nb ? std::min(k1 + SUP_B, S.m) : k1;
        if (nF <= 0 || S.n - zlo <= 0) continue;
        const int TY = (int)cdiv(nF, SUP_G1Y), Z = (int)cdiv(S.n - zlo, SUP_G1Z);
        for (int dir = 0; dir < 2; ++dir)
          for (int zs = 0; zs < Z; ++zs)
            for (int ty = 0; ty < TY; ++ty) work.push_back(SupWork{f, b, ty, (zs << 1) | dir});
      }
      SL.px.push_back(range_of(w0));
      w0 = (int64_t)work.size();
      for (int f : by_lev[l]) {
        const SupNode& S = sn[f];
        const int nb = (int)cdiv(S.m, SUP_B);
        if (nb <= r) continue;
        const int b = nb - 1 - r, k1 = std::min(SUP_B * (b + 1), S.m), nF = S.n - k1;
        for (int t = 0; t < (int)cdiv(nF, SUP_SJ); ++t) work.push_back(SupWork{f, b, t, 0});
      }
      SL.py.push_back(range_of(w0));
    }
    {
      const int64_t w1 = (int64_t)work.size();
      for (int f : by_lev[l]) {
        const int nb = (int)cdiv(sn[f].m, SUP_B);
        if (nb == nbmax) work.push_back(SupWork{f, 0, -1, 0});   // the last blocks' K x K
      }
      SL.px.push_back(range_of(w1));
      const int64_t w2 = (int64_t)work.size();
      for (int f : by_lev[l])
        if ((int)cdiv(sn[f].m, SUP_B) == nbmax) push_trail(f, nbmax - 1);   // the last blocks' trailing
      SL.panel.push_back(range_of(w2));
    }
  }
  for (SupWork& wk : work) wk.sn = sn[wk.s];
  // the other nodes: perfect by depth below their nearest front
  std::vector<uint8_t> node_in(N, 0);
  int nodes_in = 0;
  for (int i = 0; i < N; ++i)
    if (dense[sid[i]]) {
      node_in[i] = 1;
      ++nodes_in;
    }
  std::vector<int> rd(N, -1);
  int R = 0, hmax = -1;
  for (int x = N - 1; x >= 0; --x) {
    if (node_in[x]) continue;
    const int p = T_.parent[x];
    rd[x] = (p < 0 || node_in[p]) ? 0 : rd[p] + 1;
    R = std::max(R, rd[x] + 1);
    hmax = std::max(hmax, T_.height[x]);
  }
  std::vector<int64_t> rptr(R + 1, 0);
  for (int x = 0; x < N; ++x)
    if (rd[x] >= 0) ++rptr[rd[x] + 1];
  for (int d = 0; d < R; ++d) rptr[d + 1] += rptr[d];
  std::vector<int> order(rptr[R]);
  {
    std::vector<int64_t> pos(rptr.begin(), rptr.end() - 1);
    for (int x = 0; x < N; ++x)
      if (rd[x] >= 0) order[pos[rd[x]]++] = x;
  }
  std::vector<PArc> parc;
  std::vector<int64_t> raofs(R + 1, 0);
  std::vector<int> rnodes(R, 0), rkmax(R, 0);
  std::vector<uint8_t> rmulti(R, 0);
  for (int d = 0; d < R; ++d) {
    raofs[d] = (int64_t)parc.size();
    for (int64_t q = rptr[d]; q < rptr[d + 1]; ++q) {
      const int x = order[q];
      const int a0 = (int)T_.up_ptr[x], k = (int)(T_.up_ptr[x + 1] - T_.up_ptr[x]);
      if (k > 0xFFFF) return;
      ++rnodes[d];
      rkmax[d] = std::max(rkmax[d], k);
      if (k >= 2) rmulti[d] = 1;
      for (int ia = 0; ia < k; ++ia)
        parc.push_back(PArc{tofs[x], a0, (int32_t)T_.up_head[a0 + ia], (uint16_t)k, (uint16_t)ia, 0});
    }
  }
  raofs[R] = (int64_t)parc.size();
  // device copies; any failure leaves the plan off (nothing filtered yet)
  SupNode* dsn = nullptr;
  SupWork* dwk = nullptr;
  int32_t *dfn = nullptr, *dfa = nullptr;
  PArc* dpa = nullptr;
  bool ok = up_copy(dsn, sn.data(), sn.size()) == hipSuccess && up_copy(dwk, work.data(), work.size()) == hipSuccess &&
            up_copy(dfn, fnode.data(), fnode.size()) == hipSuccess && dmalloc(dfa, (size_t)foff) == hipSuccess &&
            up_copy(dpa, parc.data(), parc.size()) == hipSuccess && dmalloc(cs0_.sup_buf, 3 * (size_t)buf) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(sup_farc_kernel, dim3((unsigned)cdiv(all_rows.cnt, 4)), dim3(256), 0, 0, dsn, dwk + all_rows.off,
                       (long long)all_rows.cnt, dfn, d_up_ptr, d_up_head, dfa);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    dfree(dsn);
    dfree(dwk);
    dfree(dfn);
    dfree(dfa);
    dfree(dpa);
    dfree(cs0_.sup_buf);
    std::fprintf(stderr, "[cch] supernodal plan: device allocation failed; per-level customization\n");
    return;
  }
  d_sup_sn = dsn;
  d_sup_work = dwk;
  d_sup_fnode = dfn;
  d_sup_farc = dfa;
  d_parc2 = dpa;
  sup_buf_entries_ = buf;
  sup_lev_ = std::move(levs);
  sup_node_ = std::move(node_in);
  rlev_aofs_ = std::move(raofs);
  rlev_nodes_ = std::move(rnodes);
  rlev_kmax_ = std::move(rkmax);
  rlev_multi_ = std::move(rmulti);
  sup_fronts_ = (int)sn.size();
  sup_nodes_ = nodes_in;
  sup_blocks_ = blocks;
  sparse_heights_ = hmax + 1;
  sup_on_ = true;
}

// the perfect pull's per-arc records in depth order (without fronts: with them the pull runs over
// d_parc2, the records of the nodes outside the fronts)
bool CchGpu::build_pull_records(const std::vector<int64_t>& tofs) {
  if (sup_on_) return true;
  const int N = T_.N;
  std::vector<PArc> parc((size_t)aofs_[N]);
  for (int i = 0; i < N; ++i) {
    const int x = T_.dlev_nodes[i];
    const int a0 = (int)T_.up_ptr[x], k = (int)(T_.up_ptr[x + 1] - T_.up_ptr[x]);
    if (k > 0xFFFF) return false;             // (never on road graphs)
    for (int ia = 0; ia < k; ++ia)
      parc[(size_t)aofs_[i] + ia] = PArc{tofs[x], a0, (int32_t)T_.up_head[a0 + ia], (uint16_t)k, (uint16_t)ia, 0};
  }
  PArc* dp = nullptr;
  const bool ok = up_copy(dp, parc.data(), parc.size()) == hipSuccess;
  d_parc = dp;
  return ok;
}

// the basic phase's task table (metric-independent; height order, the fronts' nodes left out)
bool CchGpu::build_tasks(const std::vector<int64_t>& tofs) {
  std::vector<BasicTask> bt;
  btask_ptr_.assign(T_.max_height + 2, 0);
  for (int h = 0; h <= T_.max_height; ++h) {
    for (int64_t q = T_.hlev_ptr[h]; q < T_.hlev_ptr[h + 1]; ++q) {
      const int z = T_.hlev_nodes[q];
      if (sup_on_ && sup_node_[z]) continue;                // a dense front's (sup_panel_body)
      const int k = (int)(T_.up_ptr[z + 1] - T_.up_ptr[z]);
      if (k > 0xFFFE) return false;                         // (never on road graphs: k <= ~2k)
      const int a0 = (int)T_.up_ptr[z];
      for (int j0 = 0; j0 < k; j0 += 64)
        bt.push_back(BasicTask{0, z, a0, (uint16_t)k, ROW_FINAL, (uint16_t)j0, 0});
      for (int i = 0; i + 1 < k; ++i) {
        const int64_t rb = tofs[z] + (int64_t)i * (2 * k - i - 1) / 2 - i - 1;
        for (int j0 = i + 1; j0 < k; j0 += 64)
          bt.push_back(BasicTask{rb, z, a0, (uint16_t)k, (uint16_t)i, (uint16_t)j0, 0});
      }
    }
    btask_ptr_[h + 1] = (int64_t)bt.size();
  }
  BasicTask* db = nullptr;
  const bool ok = up_copy(db, bt.data(), bt.size()) == hipSuccess;
  d_btask = db;
  if (ok) n_btask_ = (int64_t)bt.size();
  return ok;
}

hipError_t CchGpu::alloc_scratch(CustScratch& x) {
  const int N = T_.N;
  const int64_t M = T_.M;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t r) {
    if (r != hipSuccess && e == hipSuccess) e = r;
  };
  ck(dmalloc(x.up64, M));
  ck(dmalloc(x.dn64, M));
  ck(dmalloc(x.pup, M));
  ck(dmalloc(x.pdn, M));
  ck(dmalloc(x.fcnt, N));
  ck(dmalloc(x.bcnt, N));
  size_t tb = 0;
  ck(hipcub::DeviceScan::InclusiveSum(nullptr, tb, x.fcnt, x.fcnt, N));
  x.cub_bytes = tb;
  ck(hipMalloc(&x.cub, x.cub_bytes ? x.cub_bytes : 1));
  ck(hipHostMalloc((void**)&x.h_stage, (size_t)std::max<int64_t>(1, T_.E) * sizeof(float), hipHostMallocDefault));
  if (sup_on_) ck(dmalloc(x.sup_buf, 3 * (size_t)sup_buf_entries_));   // D | SS | SL
  return e;
}

void CchGpu::free_scratch(CustScratch& x) {
  dfree(x.up64);
  dfree(x.dn64);
  dfree(x.pup);
  dfree(x.pdn);
  dfree(x.fcnt);
  dfree(x.bcnt);
  if (x.cub) (void)hipFree(x.cub);
  x.cub = nullptr;
  if (x.rec_buf) (void)hipFree(x.rec_buf);
  x.rec_buf = nullptr;
  dfree(x.min_buf);
  if (x.h_stage) (void)hipHostFree(x.h_stage);
  x.h_stage = nullptr;
  dfree(x.sup_buf);
  dfree(x.avoid_dev);
  if (x.avoid_host) (void)hipHostFree(x.avoid_host);
  x.avoid_host = nullptr;
}

hipError_t CchGpu::context_costs(const CchContext& c, float* d_cost, hipStream_t s, CustScratch* cs) {
  if (eta_blob_ == nullptr || d_class == nullptr || d_base_traffic == nullptr) return hipErrorInvalidValue;
  const int E = (int)T_.E;
  hipError_t e = hipSuccess;
  std::unique_lock<std::mutex> lk(mu_cust_, std::defer_lock);
  if (cs == nullptr) lk.lock();
  CustScratch& X = cs ? *cs : cs0_;
  void*& rec_buf = X.rec_buf;
  float*& min_buf = X.min_buf;
  if (rec_buf == nullptr) {
    if ((e = hipMalloc(&rec_buf, (size_t)2 * E * sizeof(EtaRecordDev))) != hipSuccess) return e;
    if ((e = dmalloc(min_buf, (size_t)2 * E)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ctx_records_kernel, dim3(blocks_for(E, 256)), dim3(256), 0, s, d_base_traffic, E, c.weather,
                     c.congestion, c.weekhour, c.driver_age, (EtaRecordDev*)rec_buf);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  e = launch_eta_mlp3_fwd(rec_buf, min_buf, 2 * E, eta_blob_, eta_H_, eta_np_, eta_variant_, eta_cus_, s, 16);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ctx_cost_kernel, dim3(blocks_for(E, 256)), dim3(256), 0, s, min_buf, d_length, d_class, E, d_cost);
  e = hipGetLastError();
  // the context's avoid areas: +inf into the closed edges' costs (csrc/cch_avoid.hip)
  if (e == hipSuccess && c.avoid) e = apply_avoid(*c.avoid, d_cost, nullptr, s, X);
  // the shared temporaries are free again only once this stream has consumed them
  if (e == hipSuccess && cs == nullptr) e = hipStreamSynchronize(s);
  return e;
}

namespace {

// Pacing (builder_max_wg_ > 0, the background builders): a wide level is launched in pieces of at
// most max_wg workgroups, one after the other on the stream, so a build never has more than that
// many workgroups of memory traffic in flight next to the flushes' query kernels.  wave_cap: the
// waves (4 per workgroup) of one piece; launch_pieces: launch(first, count) per piece of `total`.
inline long long wave_cap(int max_wg) { return max_wg > 0 ? 4LL * max_wg : (1LL << 40); }

template <class F>
hipError_t launch_pieces(long long total, long long cap, F&& launch) {
  for (long long i0 = 0; i0 < total; i0 += cap) {
    launch(i0, std::min(cap, total - i0));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// A level with a node of at least this many arcs below the fronts takes the wave kernel whatever its
// mean degree: a lane looping over a ~200-arc node's candidates was the level's time, 30-50 us
// (r6ah; swept once, r6am: 64 kept).
constexpr int PULL_WAVE_K = 64;

// one level of the pull (nodes: its node count; km: its widest node's arcs), P.base / P.arcs its records
hipError_t pull_level(hipStream_t s, const CustScratch& X, PullArgs P, long long nodes, int km, int wave_km, int max_wg) {
  // mean degree of the level's nodes: wide nodes get a wave per arc, narrow ones a lane per arc —
  // or a level with a node of >= wave_km arcs
  const bool wave = P.arcs >= 24 * nodes || km >= wave_km;
  // waves per arc by the level's widest node
  // (only where the level's arcs alone do not fill the GPU: 1M-city levels of thousands of wide
  // nodes are bound by their random gathers, and splitting them measured 1 % slower, r5z)
  const int S = P.arcs >= 8192 ? 1 : (km > 768 ? 4 : (km > 256 ? 2 : 1));
  const long long cap = wave ? std::max(1LL, wave_cap(max_wg) / S) : 64 * wave_cap(max_wg);   // arcs per piece
  const long long base = P.base;
  return launch_pieces(P.arcs, cap, [&](long long a0, long long n) {
    P.base = base + a0;
    P.arcs = n;
    if (wave && S == 4)
      hipLaunchKernelGGL(perfect_pull_wave_kernel<4>, dim3((unsigned)P.arcs), dim3(256), 0, s, P, X.up64, X.dn64,
                         X.pup, X.pdn);
    else if (wave && S == 2)
      hipLaunchKernelGGL(perfect_pull_wave_kernel<2>, dim3((unsigned)((P.arcs + 1) / 2)), dim3(256), 0, s, P,
                         X.up64, X.dn64, X.pup, X.pdn);
    else if (wave)
      hipLaunchKernelGGL(perfect_pull_wave_kernel<1>, dim3((unsigned)((P.arcs + 3) / 4)), dim3(256), 0, s, P,
                         X.up64, X.dn64, X.pup, X.pdn);
    else
      hipLaunchKernelGGL(perfect_pull_lane_kernel, dim3(blocks_for(P.arcs, 256)), dim3(256), 0, s, P, X.up64,
                         X.dn64, X.pup, X.pdn);
  });
}

}  // namespace

// the arc weights back to +inf, then every road edge into its arc
hipError_t CchGpu::reset_weights(hipStream_t s, CustScratch& X, CchMetricDev& m) {
  const int64_t M = T_.M, E = T_.E;
  const int fill_blocks = (int)std::min<int64_t>(4096, (M + 255) / 256 + 1);
  hipLaunchKernelGGL(fill_u64_kernel, dim3(fill_blocks), dim3(256), 0, s, X.up64, (long long)M, PACK_INF_D);
  hipLaunchKernelGGL(fill_u64_kernel, dim3(fill_blocks), dim3(256), 0, s, X.dn64, (long long)M, PACK_INF_D);
  hipLaunchKernelGGL(edge_scatter_kernel, dim3(blocks_for(E, 256)), dim3(256), 0, s, m.cost, d_edge_arc, d_edge_dir,
                     (int)E, X.up64, X.dn64);
  return hipGetLastError();
}

// basic, bottom-up by height
hipError_t CchGpu::basic_phase(hipStream_t s, CustScratch& X, CchMetricDev& m, int max_wg) {
  hipError_t e = hipSuccess;
  if (!accel_) {
    for (int h = 0; h <= T_.max_height && e == hipSuccess; ++h) {
      LevelArgs L{d_up_ptr, d_up_head, d_hnodes, d_bofs, (int)T_.hlev_ptr[h], (int)T_.hlev_ptr[h + 1], 0, 0};
      if (L.lo >= L.hi) continue;
      L.base = bofs_[L.lo];
      L.items = bofs_[L.hi] - bofs_[L.lo];
      if (L.items <= 0) continue;
      hipLaunchKernelGGL(basic_level_kernel, dim3(blocks_for(L.items, 256)), dim3(256), 0, s, L, X.up64, X.dn64,
                         m.sub_up, m.sub_dn, m.len_up, m.len_dn, m.cnt_up, m.cnt_dn, d_length);
      e = hipGetLastError();
    }
    return e;
  }
  for (int h = 0; h <= T_.max_height && e == hipSuccess; ++h) {
    const BasicTask* level = (const BasicTask*)d_btask + btask_ptr_[h];
    e = launch_pieces(btask_ptr_[h + 1] - btask_ptr_[h], wave_cap(max_wg), [&](long long t0, long long nt) {
      hipLaunchKernelGGL(basic_task_kernel, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, s, level + t0, nt, d_up_ptr,
                         d_up_head, d_tri, X.up64, X.dn64, m.sub_up, m.sub_dn, m.len_up, m.len_dn, m.cnt_up, m.cnt_dn,
                         d_length);
    });
  }
  if (!sup_on_ || e != hipSuccess) return e;
  // the dense fronts (build_supernodes), bottom-up by front level: gather, then per block of 32
  // pivots the panel and the trailing update (the task table above left their nodes out)
  if (X.sup_buf == nullptr) return hipErrorOutOfMemory;
  const SupNode* sup_sn = (const SupNode*)d_sup_sn;
  const SupWork* sup_wk = (const SupWork*)d_sup_work;
  int2* sup_ss = (int2*)(X.sup_buf + sup_buf_entries_);       // gather's sub-arcs
  int2* sup_sl = (int2*)(X.sup_buf + 2 * sup_buf_entries_);   // ... metres, edges
  for (size_t l = 0; l < sup_lev_.size() && e == hipSuccess; ++l) {
    const SupLevel& SL = sup_lev_[l];
    hipLaunchKernelGGL(sup_gather_basic_kernel, dim3((unsigned)SL.gather.cnt), dim3(256), 0, s, sup_sn,
                       sup_wk + SL.gather.off, d_sup_fnode, d_sup_farc, X.up64, X.dn64, d_up_ptr, d_up_head, m.len_up,
                       m.len_dn, m.cnt_up, m.cnt_dn, X.sup_buf, sup_ss, sup_sl);
    for (size_t r = 0; r < SL.panel.size(); ++r)
      if (SL.panel[r].cnt > 0)
        hipLaunchKernelGGL(sup_step_basic_kernel, dim3((unsigned)SL.panel[r].cnt), dim3(1024), 0, s,
                           sup_wk + SL.panel[r].off, d_sup_farc, X.sup_buf, sup_ss, sup_sl, X.up64, X.dn64, m.sub_up,
                           m.sub_dn, m.len_up, m.len_dn, m.cnt_up, m.cnt_dn, d_length);
    e = hipGetLastError();
  }
  return e;
}

// perfect, top-down
hipError_t CchGpu::perfect_phase(hipStream_t s, CustScratch& X, CchMetricDev& m, int max_wg) {
  (void)m;
  const int64_t M = T_.M;
  const int fill_blocks = (int)std::min<int64_t>(4096, (M + 255) / 256 + 1);
  hipLaunchKernelGGL(perfect_init_kernel, dim3(fill_blocks), dim3(256), 0, s, X.up64, X.dn64, X.pup, X.pdn, (long long)M);
  hipError_t e = hipGetLastError();
  if (!accel_) {
    for (int d = 0; d <= T_.max_depth && e == hipSuccess; ++d) {
      LevelArgs L{d_up_ptr, d_up_head, d_dnodes, d_pofs, (int)T_.dlev_ptr[d], (int)T_.dlev_ptr[d + 1], 0, 0};
      if (L.lo >= L.hi) continue;
      L.base = pofs_[L.lo];
      L.items = pofs_[L.hi] - pofs_[L.lo];
      if (L.items <= 0) continue;
      hipLaunchKernelGGL(perfect_level_kernel, dim3(blocks_for(L.items, 256)), dim3(256), 0, s, L, X.up64, X.dn64, X.pup,
                         X.pdn);
      e = hipGetLastError();
    }
    return e;
  }
  if (!sup_on_) {
    // the pull by depth over d_parc (measured faster than a perfect task kernel: 12.0 vs 15.3 ms on
    // the 100k graph, 227 vs 351 ms on the 1M city, round 5)
    for (int d = 0; d <= T_.max_depth && e == hipSuccess; ++d) {
      const int lo = (int)T_.dlev_ptr[d], hi = (int)T_.dlev_ptr[d + 1];
      if (lo >= hi) continue;
      const PullArgs P{d_up_head, d_tri, (const PArc*)d_parc, aofs_[lo], aofs_[hi] - aofs_[lo]};
      if (P.arcs <= 0 || pofs_[hi] == pofs_[lo]) continue;       // no node of the level has two arcs
      e = pull_level(s, X, P, hi - lo, plev_kmax_[d], 1 << 30, max_wg);
    }
    return e;
  }
  // the dense fronts top-down by front level (per block from the top: the (min, +) product through
  // the final part, the solve through K, the K x K targets), then the other nodes by depth below
  // their nearest front, pulled over d_parc2
  const SupNode* sup_sn = (const SupNode*)d_sup_sn;
  const SupWork* sup_wk = (const SupWork*)d_sup_work;
  for (int l = (int)sup_lev_.size() - 1; l >= 0 && e == hipSuccess; --l) {
    const SupLevel& SL = sup_lev_[l];
    float* Dp = (float*)X.sup_buf;
    hipLaunchKernelGGL(sup_gather_perfect_kernel, dim3(blocks_for(SL.gather.cnt, 4)), dim3(256), 0, s, sup_sn,
                       sup_wk + SL.gather.off, (long long)SL.gather.cnt, d_sup_farc, X.up64, X.dn64, X.pup, X.pdn, Dp);
    for (size_t r = 0; r < SL.px.size(); ++r) {
      if (SL.px[r].cnt > 0)
        hipLaunchKernelGGL(sup_kk_gemm_perfect_kernel, dim3((unsigned)SL.px[r].cnt), dim3(1024), 0, s,
                           sup_wk + SL.px[r].off, d_sup_farc, Dp, X.pup, X.pdn);
      if (r < SL.py.size() && SL.py[r].cnt > 0)
        hipLaunchKernelGGL(sup_solve_perfect_kernel, dim3((unsigned)SL.py[r].cnt), dim3(1024), 0, s, sup_sn,
                           sup_wk + SL.py[r].off, d_sup_farc, Dp, X.pup, X.pdn);
    }
    e = hipGetLastError();
  }
  for (size_t d = 0; d < rlev_nodes_.size() && e == hipSuccess; ++d) {
    if (!rlev_multi_[d]) continue;
    const PullArgs P{d_up_head, d_tri, (const PArc*)d_parc2, rlev_aofs_[d], rlev_aofs_[d + 1] - rlev_aofs_[d]};
    e = pull_level(s, X, P, rlev_nodes_[d], rlev_kmax_[d], PULL_WAVE_K, max_wg);
  }
  return e;
}

// pruning: kept arcs per node, their prefix sums (the metric's f_ptr / b_ptr), then the kept arcs'
// records — the counts' totals come to the host in between to size the record arrays
hipError_t CchGpu::prune_phase(hipStream_t s, CustScratch& X, CchMetricDev& m) {
  const int N = T_.N;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t x) {
    if (x != hipSuccess && e == hipSuccess) e = x;
  };
  hipLaunchKernelGGL(prune_count_wave_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, d_up_ptr, X.pup, X.pdn,
                     X.up64, X.dn64, N, X.fcnt, X.bcnt);
  ck(hipGetLastError());
  ck(hipMemsetAsync(m.f_ptr, 0, sizeof(int32_t), s));
  ck(hipMemsetAsync(m.b_ptr, 0, sizeof(int32_t), s));
  size_t tb = X.cub_bytes;
  ck(hipcub::DeviceScan::InclusiveSum(X.cub, tb, X.fcnt, m.f_ptr + 1, N, s));
  tb = X.cub_bytes;
  ck(hipcub::DeviceScan::InclusiveSum(X.cub, tb, X.bcnt, m.b_ptr + 1, N, s));
  int32_t tot[2] = {0, 0};
  ck(hipMemcpyAsync(&tot[0], m.f_ptr + N, 4, hipMemcpyDeviceToHost, s));
  ck(hipMemcpyAsync(&tot[1], m.b_ptr + N, 4, hipMemcpyDeviceToHost, s));
  ck(hipStreamSynchronize(s));
  if (e != hipSuccess) return e;
  if (tot[0] > m.kept_f || m.f_rec == nullptr) {
    dfree(m.f_rec);
    ck(dmalloc(m.f_rec, tot[0]));
  }
  if (tot[1] > m.kept_b || m.b_rec == nullptr) {
    dfree(m.b_rec);
    ck(dmalloc(m.b_rec, tot[1]));
  }
  m.kept_f = tot[0];
  m.kept_b = tot[1];
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(prune_scatter_wave_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, d_up_ptr, d_up_head,
                     d_depth, X.pup, X.pdn, X.up64, X.dn64, N, m.f_ptr, m.b_ptr, m.f_rec, m.b_rec);
  return hipGetLastError();
}

hipError_t CchGpu::customize(const float* d_cost, CchMetricDev& m, hipStream_t s, CustScratch* cs) {
  std::unique_lock<std::mutex> lk(mu_cust_, std::defer_lock);
  if (cs == nullptr) lk.lock();
  CustScratch& X = cs ? *cs : cs0_;
  // a background build while queries are served (or always, set_builder_pacing): paced launches
  const bool paced = cs != nullptr && builder_max_wg_.load() > 0 && (pace_always_.load() || serving_now());
  if (paced) n_paced_.fetch_add(1, std::memory_order_relaxed);
  const int max_wg = paced ? std::max(0, builder_max_wg_.load(std::memory_order_relaxed)) : 0;
  auto t0 = std::chrono::steady_clock::now();
  const int N = T_.N;
  const int64_t M = T_.M, E = T_.E;
  m.device = dev_;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t x) {
    if (x != hipSuccess && e == hipSuccess) e = x;
  };
  const auto ta = std::chrono::steady_clock::now();
  if (m.cost == nullptr) ck(dmalloc(m.cost, E));
  if (m.sub_up == nullptr) {
    ck(dmalloc(m.sub_up, 2 * M));
    ck(dmalloc(m.sub_dn, 2 * M));
    ck(dmalloc(m.len_up, M));
    ck(dmalloc(m.len_dn, M));
    ck(dmalloc(m.cnt_up, M));
    ck(dmalloc(m.cnt_dn, M));
    ck(dmalloc(m.f_ptr, N + 1));
    ck(dmalloc(m.b_ptr, N + 1));
  }
  m.alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
  if (e != hipSuccess) return e;
  if (d_cost != m.cost) ck(hipMemcpyAsync(m.cost, d_cost, E * sizeof(float), hipMemcpyDeviceToDevice, s));
  // phase boundaries (basic / perfect / prune device times, reported with the metric)
  struct Events {
    hipEvent_t e[4] = {};
    Events() {
      for (auto& x : e)
        if (hipEventCreate(&x) != hipSuccess) x = nullptr;
    }
    ~Events() {
      for (auto& x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } evs;
  hipEvent_t* ev = evs.e;
  ck(reset_weights(s, X, m));
  if (ev[0]) (void)hipEventRecord(ev[0], s);
  if (e == hipSuccess) ck(basic_phase(s, X, m, max_wg));
  if (ev[1]) (void)hipEventRecord(ev[1], s);
  if (e == hipSuccess) ck(perfect_phase(s, X, m, max_wg));
  if (ev[2]) (void)hipEventRecord(ev[2], s);
  if (e == hipSuccess) ck(prune_phase(s, X, m));
  if (ev[3]) (void)hipEventRecord(ev[3], s);
  ck(hipStreamSynchronize(s));
  if (e != hipSuccess) return e;
  m.customize_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  float ms = 0.f;
  if (ev[0] && ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) m.basic_ms = ms;
  if (ev[1] && ev[2] && hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) m.perfect_ms = ms;
  if (ev[2] && ev[3] && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) m.prune_ms = ms;
  // the host copy of the costs (maneuver durations, the exact host fallback) is made here, on the
  // builder's stream, before the metric is published: a flush that first meets this context finds
  // it ready instead of copying E floats on its own critical path
  // (through the scratch's pinned stage: a pageable copy is staged by the runtime in pieces on the
  // copy engines the flushes' transfers use)
  const auto th = std::chrono::steady_clock::now();
  m.host_cost.resize((size_t)E);
  if (X.h_stage != nullptr) {
    ck(hipMemcpyAsync(X.h_stage, m.cost, (size_t)E * sizeof(float), hipMemcpyDeviceToHost, s));
    ck(hipStreamSynchronize(s));
    if (e == hipSuccess) std::memcpy(m.host_cost.data(), X.h_stage, (size_t)E * sizeof(float));
  } else {
    ck(hipMemcpyAsync(m.host_cost.data(), m.cost, (size_t)E * sizeof(float), hipMemcpyDeviceToHost, s));
    ck(hipStreamSynchronize(s));
  }
  if (e != hipSuccess) m.host_cost.clear();
  m.hostcopy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th).count();
  return e;
}

}  // namespace rt
