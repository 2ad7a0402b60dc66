// GPU customizable contraction hierarchy, queries: batched elimination-tree searches over a
// customized metric (csrc/cch_customize.hip; the CPU reference is csrc/runtime/cch.h "elimination-tree
// search"; replaces per-request directions / matrix calls).
//
// The forward search space of s is its etree ancestor chain, swept bottom-up once with labels in LDS
// indexed by depth (one wave per chain job; runs of consecutive ranks — the separators — are fetched
// 64 at a time, so pointer chasing is per run, not per node).  A meet kernel takes each pair's two
// chains (one wave per pair: LCA by binary search on the chains' node arrays, min over common depths,
// deepest tie) and lists the shortcut arcs of the chosen up-down path; the unpack kernels expand them
// to road nodes (cooperatively, 16 lanes per pair; a serial DFS per lane for the longest arc lists).
// Many-to-many matrices reuse each point's two chains, and legs can reuse a matrix call's chains.
// Rectangular matrices sweep one forward chain per source and one backward chain per destination
// and meet per (source, tile of 64 destinations) with the source's chain in LDS (meet_rect_kernel).
#include "cch_dev.h"
#include "cch_gpu.h"

namespace rt {

using namespace cchd;

namespace {

// One wave per chain job (rank << 1 | dir): sweep the etree ancestor chain bottom-up with labels in
// LDS by depth, then dump them (dist, pred arc) and the chain's node ranks to the job's scratch row.
//
// The chain is walked in runs of consecutive ranks (parent(x + i) == x + i + 1: the separators), up to
// 64 per run, whose headers (parent, record range) one coalesced load fetches; the next run's header
// is loaded while the current run is swept.  Inside a run, node i's first 256 kept-arc records (4 per lane) are
// loaded SWEEP_AHEAD nodes ahead, so the sequential label sweep waits on LDS, not on one global
// load per chain node (r4c profile: the sweep was 49.6 % of the CCH GPU time at ~25 us per chain).
constexpr int SWEEP_AHEAD = 3;
constexpr int SWEEP_RECS = 4;          // records per lane fetched ahead per chain node (256 per node)

typedef int sweep_v4i __attribute__((ext_vector_type(4)));

struct SweepRecs {
  sweep_v4i r[SWEEP_RECS];
};

// The record prefetch is issued as inline-asm loads the compiler does not track, and each use
// waits for its own loads with an explicit vmcnt (sweep_wait): compiler-tracked loads that stay in
// flight across the loop's back edge made it wait for all of them at the top of every iteration.
// Branch-free: lanes past the node's records load record 0 (always allocated) and are masked where
// the records are used, so every fetch issues exactly SWEEP_RECS loads.
__device__ __forceinline__ SweepRecs sweep_fetch(const int4* __restrict__ rec, int pb, int pe, int i, int L, int lane) {
  SweepRecs v;
  const int ii = i < 63 ? i : 63;
  const int b = __shfl(pb, ii);
  const int e = i < L ? __shfl(pe, ii) : b;
#pragma unroll
  for (int k = 0; k < SWEEP_RECS; ++k) {
    const int idx = b + lane + 64 * k;
    const int4* p = rec + (idx < e ? idx : 0);
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v.r[k]) : "v"(p));
  }
  return v;
}

// wait until the loads of the fetch issued `newer` fetches before the current one have landed
template <int NEWER>
__device__ __forceinline__ void sweep_wait(SweepRecs& q) {
  static_assert(NEWER * SWEEP_RECS <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(q.r[0]), "+v"(q.r[1]), "+v"(q.r[2]), "+v"(q.r[3]) : "n"(NEWER * SWEEP_RECS));
}

__device__ __forceinline__ void sweep_relax(float* sd, int32_t* sp, float dx, int w, int hd, int arc) {
  const float nd = dx + __int_as_float(w);
  if (nd < sd[hd]) {
    sd[hd] = nd;
    sp[hd] = arc;
  }
}

__global__ __launch_bounds__(64) void sweep_kernel(const int32_t* __restrict__ jobs, int J,
                                                   const int32_t* __restrict__ parent,
                                                   const int32_t* __restrict__ depth, int N,
                                                   const int32_t* __restrict__ f_ptr, const int4* __restrict__ f_rec,
                                                   const int32_t* __restrict__ b_ptr, const int4* __restrict__ b_rec,
                                                   int stride, float* __restrict__ out_dist,
                                                   int32_t* __restrict__ out_pred, int32_t* __restrict__ out_node,
                                                   const CchMView* __restrict__ mv, const int32_t* __restrict__ grp,
                                                   int gdiv) {
  extern __shared__ unsigned char smem[];
  float* sd = reinterpret_cast<float*>(smem);
  int32_t* sp = reinterpret_cast<int32_t*>(smem + (size_t)stride * 4);
  const int j = blockIdx.x;
  if (j >= J) return;
  const int lane = threadIdx.x;
  const int code = jobs[j];
  if (code < 0) return;                     // matrix padding
  const int r = code >> 1;
  const bool fwd = (code & 1) == 0;
  if (mv != nullptr) {                      // this job's metric (one job per workgroup: uniform)
    const CchMView& v = mv[grp[j / gdiv]];
    f_ptr = v.f_ptr;
    f_rec = v.f_rec;
    b_ptr = v.b_ptr;
    b_rec = v.b_rec;
  }
  const int32_t* __restrict__ ptr = fwd ? f_ptr : b_ptr;
  const int4* __restrict__ rec = fwd ? f_rec : b_rec;
  const int D = depth[r];
  for (int d = lane; d <= D; d += 64) {
    sd[d] = F_INF;
    sp[d] = -1;
  }
  __syncthreads();
  if (lane == 0) sd[D] = 0.f;
  __syncthreads();
  const size_t base = (size_t)j * stride;
  int x = r, d = D;
  // header of the run starting at x: parent and record range of x + lane
  int cand = x + lane;
  int par = cand < N ? parent[cand] : -2;
  int pb = cand < N ? ptr[cand] : 0;
  int pe = cand < N ? ptr[cand + 1] : 0;
  while (x >= 0 && d >= 0) {
    const unsigned long long cont = __ballot(cand < N && par == cand + 1);
    int L = (~cont == 0ull) ? 64 : (__builtin_ctzll(~cont) + 1);
    if (L > d + 1) L = d + 1;
    const int next = __shfl(par, L - 1);
    if (lane < L) out_node[base + (d - lane)] = x + lane;
    // the next run's header, in flight while this run is swept
    const int ncand = next + lane;
    const bool nin = next >= 0 && ncand < N;
    const int npar = nin ? parent[ncand] : -2;
    const int npb = nin ? ptr[ncand] : 0;
    const int npe = nin ? ptr[ncand + 1] : 0;
    // each node's records were requested three nodes earlier; named buffers, unrolled by four
    auto node = [&](int i, const SweepRecs& q) {
      if (i >= L) return;
      const float dx = sd[d - i];
      if (dx < F_INF) {
        // a node's kept arcs have distinct heads: the lanes' updates never collide
        const int b = __shfl(pb, i), e = __shfl(pe, i);
#pragma unroll
        for (int k = 0; k < SWEEP_RECS; ++k)
          if (b + lane + 64 * k < e) sweep_relax(sd, sp, dx, q.r[k].x, q.r[k].y, q.r[k].z);
        for (int k = b + 64 * SWEEP_RECS + lane; k < e; k += 64) {     // nodes with > 256 kept arcs
          const int4 rc = rec[k];
          sweep_relax(sd, sp, dx, rc.x, rc.y, rc.z);
        }
        __syncthreads();
      }
    };
    SweepRecs qa = sweep_fetch(rec, pb, pe, 0, L, lane);
    SweepRecs qb = sweep_fetch(rec, pb, pe, 1, L, lane);
    SweepRecs qc = sweep_fetch(rec, pb, pe, 2, L, lane);
    for (int i = 0; i < L; i += 4) {
      SweepRecs qd = sweep_fetch(rec, pb, pe, i + 3, L, lane);
      sweep_wait<3>(qa);
      node(i, qa);
      qa = sweep_fetch(rec, pb, pe, i + 4, L, lane);
      sweep_wait<3>(qb);
      node(i + 1, qb);
      qb = sweep_fetch(rec, pb, pe, i + 5, L, lane);
      sweep_wait<3>(qc);
      node(i + 2, qc);
      qc = sweep_fetch(rec, pb, pe, i + 6, L, lane);
      sweep_wait<3>(qd);
      node(i + 3, qd);
    }
    sweep_wait<0>(qa);          // drain the prefetch past the run's end before the buffers are reused
    sweep_wait<0>(qb);
    sweep_wait<0>(qc);
    x = next;
    d -= L;
    cand = ncand;
    par = npar;
    pb = npb;
    pe = npe;
  }
  __syncthreads();
  for (int dd = lane; dd <= D; dd += 64) {
    out_dist[base + dd] = sd[dd];
    out_pred[base + dd] = sp[dd];
  }
}

// One wave per pair: LCA depth, best common depth (min sum, deepest tie), metres along the chosen
// shortcut arcs (forward arcs from the meeting node down to s, then backward ones down to t), and —
// with `arcs` — the arc list in path order (arc << 1 | traversed-down).
__global__ __launch_bounds__(64) void meet_kernel(int P, const int32_t* __restrict__ pjf, const int32_t* __restrict__ pjb,
                                                  int jf0, int jb0, const int32_t* __restrict__ jobs, int stride,
                                                  const float* __restrict__ sdist, const int32_t* __restrict__ spred,
                                                  const int32_t* __restrict__ snode, const int32_t* __restrict__ depth,
                                                  const int32_t* __restrict__ arc_lo, const float* __restrict__ len_up,
                                                  const float* __restrict__ len_dn, float* __restrict__ out_sec,
                                                  float* __restrict__ out_met, int* __restrict__ out_status,
                                                  int32_t* __restrict__ arcs, int32_t* __restrict__ narcs, int max_arcs,
                                                  const CchMView* __restrict__ mv, const int32_t* __restrict__ grp,
                                                  int gdiv) {
  __shared__ int32_t fw[4096];
  const int q = blockIdx.x;
  if (q >= P) return;
  const int lane = threadIdx.x;
  if (mv != nullptr) {
    const CchMView& v = mv[grp[q / gdiv]];
    len_up = v.len_up;
    len_dn = v.len_dn;
  }
  const int jf = pjf ? pjf[q] : jf0 + 2 * q;
  const int jb = pjb ? pjb[q] : jb0 + 2 * q;
  if (jobs[jf] < 0 || jobs[jb] < 0) {       // a matrix padding point: nothing to meet
    if (threadIdx.x == 0) {
      if (out_sec) out_sec[q] = -1.f;
      if (out_met) out_met[q] = -1.f;
      if (out_status) out_status[q] = 1;
      if (narcs) narcs[q] = 0;
    }
    return;
  }
  const int s = jobs[jf] >> 1, t = jobs[jb] >> 1;
  const int ds = depth[s], dt = depth[t];
  const size_t bf = (size_t)jf * stride, bb = (size_t)jb * stride;
  int status = 1;
  float best = F_INF;
  int bestd = -1;
  if (snode[bf] == snode[bb]) {
    // chains agree on depths [0, L]
    int lo = 0, hi = ds < dt ? ds : dt;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (snode[bf + mid] == snode[bb + mid]) lo = mid;
      else hi = mid - 1;
    }
    const int L = lo;
    for (int d = lane; d <= L; d += 64) {
      const float v = sdist[bf + d] + sdist[bb + d];
      if (v < best || (v == best && d > bestd)) {
        best = v;
        bestd = d;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int od = __shfl_xor(bestd, o);
      if (ov < best || (ov == best && od > bestd)) {
        best = ov;
        bestd = od;
      }
    }
    if (best < F_INF) status = 0;
  }
  if (lane != 0) return;
  float met = 0.f;
  int n = 0;
  if (status == 0) {
    int nf = 0;
    for (int slot = bestd; slot != ds;) {
      const int a = spred[bf + slot];
      met += len_up[a];
      if (nf < 4096) fw[nf] = a;
      ++nf;
      slot = depth[arc_lo[a]];
    }
    if (arcs != nullptr) {
      int32_t* out = arcs + (size_t)q * max_arcs;
      if (nf > 4096 || nf > max_arcs) status = 4;
      for (int i = nf - 1; i >= 0 && status == 0; --i) out[n++] = fw[i] << 1;
      for (int slot = bestd; slot != dt && status == 0;) {
        const int a = spred[bb + slot];
        met += len_dn[a];
        if (n >= max_arcs) { status = 4; break; }
        out[n++] = (a << 1) | 1;
        slot = depth[arc_lo[a]];
      }
    } else {
      for (int slot = bestd; slot != dt;) {
        const int a = spred[bb + slot];
        met += len_dn[a];
        slot = depth[arc_lo[a]];
      }
    }
  }
  if (out_sec) out_sec[q] = status == 0 ? best : -1.f;
  if (out_met) out_met[q] = status == 0 ? met : -1.f;
  if (out_status) out_status[q] = status;
  if (narcs) narcs[q] = n;
}

// One lane per pair: expand the shortcut arcs to road node ids (DFS, first sub-arc first).
constexpr int UNPACK_STACK = 128;
__global__ __launch_bounds__(64) void unpack_kernel(int P, const int* __restrict__ src_node, const int32_t* __restrict__ arcs,
                                                    const int32_t* __restrict__ narcs, int max_arcs,
                                                    const int32_t* __restrict__ sub_up,
                                                    const int32_t* __restrict__ sub_dn,
                                                    const int32_t* __restrict__ arc_lo,
                                                    const int32_t* __restrict__ up_head,
                                                    const int32_t* __restrict__ node_of, int* __restrict__ status,
                                                    int* __restrict__ out_len, int* __restrict__ out_path, int max_path,
                                                    int min_arcs, int* __restrict__ out_edge,
                                                    const CchMView* __restrict__ mv, const int32_t* __restrict__ grp) {
  __shared__ int32_t stk[64 * UNPACK_STACK];
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  if (mv != nullptr) {
    const CchMView& v = mv[grp[q]];
    sub_up = v.sub_up;
    sub_dn = v.sub_dn;
  }
  int32_t* st = stk + threadIdx.x * UNPACK_STACK;
  if (status[q] != 0) {
    if (min_arcs < 0) out_len[q] = 0;
    return;
  }
  if (narcs[q] <= min_arcs && out_len[q] != -1) return;   // unpacked by unpack_coop_kernel
  int* out = out_path + (size_t)q * max_path;
  int n = 0;
  out[n++] = src_node[q];
  const int na = narcs[q];
  const int32_t* al = arcs + (size_t)q * max_arcs;
  bool ok = true;
  for (int k = 0; k < na && ok; ++k) {
    int sp = 0;
    st[sp++] = al[k];
    while (sp > 0) {
      const int code = st[--sp];
      const int a = code >> 1, dn = code & 1;
      const int32_t* sub = (dn ? sub_dn : sub_up) + 2 * (long long)a;
      const int s0 = sub[0];
      if (s0 < 0) {
        if (n >= max_path) { ok = false; break; }
        if (out_edge) out_edge[(size_t)q * max_path + n - 1] = sub[1];
        out[n++] = node_of[dn ? arc_lo[a] : up_head[a]];
        continue;
      }
      if (sp + 2 > UNPACK_STACK) { ok = false; break; }
      st[sp++] = sub[1] << 1;        // second: traversed up
      st[sp++] = (s0 << 1) | 1;      // first: traversed down (popped first)
    }
  }
  if (!ok) {
    status[q] = 4;
    out_len[q] = 0;
    return;
  }
  out_len[q] = n;
}

// Cooperative unpack: UNPACK_LANES lanes per pair share its path.  The arcs' road-edge counts
// (cnt_*, from the customization) give each shortcut arc its offset in the path, every lane takes a
// contiguous range of road edges, descends the shortcut tree once to its first edge (counts pick the
// branch), then walks the DFS for the rest of its range — ~depth + edges/UNPACK_LANES dependent
// loads per lane instead of one lane walking the whole path (the serial unpack's time was the
// longest path's DFS).  Pairs with more than UNPACK_MAX_ARCS shortcut arcs take the serial kernel.
constexpr int UNPACK_LANES = 16;
constexpr int UNPACK_MAX_ARCS = 256;
constexpr int UNPACK_SD = 64;                 // per-lane DFS stack (pending second sub-arcs)
__global__ __launch_bounds__(64) void unpack_coop_kernel(int P, const int* __restrict__ src_node,
                                                         const int32_t* __restrict__ arcs,
                                                         const int32_t* __restrict__ narcs, int max_arcs,
                                                         const int32_t* __restrict__ sub_up,
                                                         const int32_t* __restrict__ sub_dn,
                                                         const int32_t* __restrict__ cnt_up,
                                                         const int32_t* __restrict__ cnt_dn,
                                                         const int32_t* __restrict__ arc_lo,
                                                         const int32_t* __restrict__ up_head,
                                                         const int32_t* __restrict__ node_of, int* __restrict__ status,
                                                         int* __restrict__ out_len, int* __restrict__ out_path,
                                                         int max_path, int* __restrict__ out_edge,
                                                         const CchMView* __restrict__ mv,
                                                         const int32_t* __restrict__ grp) {
  constexpr int G = 64 / UNPACK_LANES;
  __shared__ int32_t offs[G][UNPACK_MAX_ARCS + 1];
  __shared__ int32_t stk[64 * UNPACK_SD];
  const int lane = threadIdx.x, g = lane / UNPACK_LANES, sl = lane % UNPACK_LANES;
  const int q = blockIdx.x * G + g;
  const bool active = q < P;
  if (mv != nullptr && active) {            // (per pair: the four pairs of a wave may differ)
    const CchMView& v = mv[grp[q]];
    sub_up = v.sub_up;
    sub_dn = v.sub_dn;
    cnt_up = v.cnt_up;
    cnt_dn = v.cnt_dn;
  }
  int st = active ? status[q] : 1;
  const int na = active && st == 0 ? narcs[q] : 0;
  const bool coop = active && st == 0 && na <= UNPACK_MAX_ARCS;   // longer arc lists: the serial kernel
  if (active && st != 0 && sl == 0) out_len[q] = 0;
  // exclusive prefix of the arcs' edge counts, UNPACK_LANES at a time
  const int32_t* al = arcs + (size_t)(active ? q : 0) * max_arcs;
  int carry = 0;
  for (int b = 0; b < (coop ? na : 0); b += UNPACK_LANES) {
    const int k = b + sl;
    int c = 0;
    if (k < na) {
      const int code = al[k];
      c = (code & 1) ? cnt_dn[code >> 1] : cnt_up[code >> 1];
    }
    int incl = c;
#pragma unroll
    for (int o = 1; o < UNPACK_LANES; o <<= 1) {
      const int y = __shfl_up(incl, o, UNPACK_LANES);
      if (sl >= o) incl += y;
    }
    if (k < na) offs[g][k] = carry + incl - c;
    carry += __shfl(incl, UNPACK_LANES - 1, UNPACK_LANES);
  }
  const int E = carry;                       // road edges of the path (uniform in the group)
  if (coop) {
    if (sl == 0) offs[g][na] = E;
    if (E + 1 > max_path) {
      if (sl == 0) {
        status[q] = 4;
        out_len[q] = 0;
      }
      st = 4;
    } else if (sl == 0) {
      out_len[q] = E + 1;
    }
  }
  __syncthreads();
  if (!coop || st != 0) return;
  int* out = out_path + (size_t)q * max_path;
  int* oe = out_edge ? out_edge + (size_t)q * max_path : nullptr;
  if (sl == 0) out[0] = src_node[q];
  const int per = (E + UNPACK_LANES - 1) / UNPACK_LANES;
  int e = sl * per;
  const int e1 = min(E, e + per);
  if (e >= e1) return;
  int32_t* sk = stk + lane * UNPACK_SD;
  // the arc holding edge e
  int lo = 0, hi = na - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[g][mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  int k = lo;
  int r = e - offs[g][k];                  // edge index inside arc k
  int sp = 0;
  bool ok = true;
  int code = al[k];
  // descend to the r-th edge of `code`, keeping the pending second halves
  auto descend = [&](int c, int rr) -> int {
    while (true) {
      const int a = c >> 1, dn = c & 1;
      const int32_t* sub = (dn ? sub_dn : sub_up) + 2 * (long long)a;
      const int s0 = sub[0];
      if (s0 < 0) return c;                  // an original edge
      const int s1 = sub[1];
      const int first = (s0 << 1) | 1, second = s1 << 1;     // first traversed down, second up
      const int c0 = cnt_dn[s0];
      if (rr < c0) {
        if (sp >= UNPACK_SD) { ok = false; return c; }
        sk[sp++] = second;
        c = first;
      } else {
        rr -= c0;
        c = second;
      }
    }
  };
  int leaf = descend(code, r);
  while (ok) {
    const int a = leaf >> 1, dn = leaf & 1;
    out[e + 1] = node_of[dn ? arc_lo[a] : up_head[a]];
    if (oe) oe[e] = (dn ? sub_dn : sub_up)[2 * (long long)a + 1];    // a leaf arc's original edge
    if (++e >= e1) break;
    if (sp > 0) {
      leaf = descend(sk[--sp], 0);
    } else {
      ++k;                                   // next shortcut arc of the path
      leaf = descend(al[k], 0);
    }
  }
  if (!ok) out_len[q] = -1;                  // stack overflow: the serial kernel redoes the pair
}

// (node ids are range-checked by the callers; out-of-range ids are clamped, never dereferenced)
__global__ void route_jobs_kernel(const int* __restrict__ src, const int* __restrict__ dst, int Q,
                                  const int32_t* __restrict__ rank, int N, int32_t* __restrict__ jobs) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  int s = src[q], t = dst[q];
  s = (s < 0 || s >= N) ? 0 : s;
  t = (t < 0 || t >= N) ? 0 : t;
  jobs[2 * q] = rank[s] << 1;
  jobs[2 * q + 1] = (rank[t] << 1) | 1;
}

// legs from a matrix call's chains: job indices of (r, i) forward and (r, j) backward
__global__ void leg_pairs_kernel(int NM, const int* __restrict__ r, const int* __restrict__ i,
                                 const int* __restrict__ j, int Q, int R, int32_t* __restrict__ pjf,
                                 int32_t* __restrict__ pjb) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  int rr = r[q], ii = i[q], jj = j[q];
  rr = rr < 0 ? 0 : (rr >= R ? R - 1 : rr);       // clamped: the host checks the ranges
  ii = ii < 0 ? 0 : (ii >= NM ? NM - 1 : ii);
  jj = jj < 0 ? 0 : (jj >= NM ? NM - 1 : jj);
  pjf[q] = 2 * (rr * NM + ii);
  pjb[q] = 2 * (rr * NM + jj) + 1;
}

// matrix: jobs [R][NM][2] (forward, backward per point); pairs (r, i, j) for i != j
__global__ void matrix_jobs_kernel(const int* __restrict__ pts, const int* __restrict__ npts, int R, int NM,
                                   const int32_t* __restrict__ rank, int N, int32_t* __restrict__ jobs) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= (long long)R * NM) return;
  const int r = (int)(g / NM), i = (int)(g % NM);
  if (i >= npts[r]) {                       // padding of a shorter request: no chain is swept
    jobs[2 * g] = -1;
    jobs[2 * g + 1] = -1;
    return;
  }
  int v = pts[g];
  if (v < 0 || v >= N) v = 0;
  jobs[2 * g] = rank[v] << 1;
  jobs[2 * g + 1] = (rank[v] << 1) | 1;
}

__global__ void matrix_pairs_kernel(const int* __restrict__ npts, int R, int NM, int32_t* __restrict__ pjf,
                                    int32_t* __restrict__ pjb) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= (long long)R * NM * NM) return;
  const int r = (int)(g / ((long long)NM * NM));
  const int rem = (int)(g % ((long long)NM * NM));
  const int i = rem / NM, j = rem % NM;
  pjf[g] = 2 * (r * NM + i);
  pjb[g] = 2 * (r * NM + j) + 1;
}

__global__ void matrix_out_kernel(const int* __restrict__ npts, int R, int NM, float* __restrict__ sec,
                                  float* __restrict__ met, double* __restrict__ D64) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= (long long)R * NM * NM) return;
  const int r = (int)(g / ((long long)NM * NM));
  const int rem = (int)(g % ((long long)NM * NM));
  const int i = rem / NM, j = rem % NM;
  const int n = npts[r];
  const bool diag = i == j;
  const bool out = i >= n || j >= n;
  float s = sec ? sec[g] : 0.f, m = met ? met[g] : 0.f;
  if (diag || out) s = m = 0.f;
  else {
    if (s < 0.f) s = F_INF;
    if (m < 0.f) m = F_INF;
  }
  if (sec) sec[g] = s;
  if (met) met[g] = m;
  if (D64) D64[g] = (double)m;
}

// rectangular matrix: jobs [R][SM + DM] — row r's forward chains of its sources, then the backward
// chains of its destinations; a padding slot is -1 (no chain is swept)
__global__ void rect_jobs_kernel(const int* __restrict__ src, const int* __restrict__ nsrc, const int* __restrict__ dst,
                                 const int* __restrict__ ndst, int R, int SM, int DM, const int32_t* __restrict__ rank,
                                 int N, int32_t* __restrict__ jobs) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int W = SM + DM;
  if (g >= (long long)R * W) return;
  const int r = (int)(g / W), k = (int)(g % W);
  const bool fwd = k < SM;
  const int i = fwd ? k : k - SM;
  if (i >= (fwd ? nsrc[r] : ndst[r])) {
    jobs[g] = -1;
    return;
  }
  int v = fwd ? src[(size_t)r * SM + i] : dst[(size_t)r * DM + i];
  if (v < 0 || v >= N) v = 0;
  jobs[g] = (rank[v] << 1) | (fwd ? 0 : 1);
}

// One workgroup per (row, source, tile of MEET_TILE destinations) of a rectangular matrix.  The
// source's forward chain (node ranks, labels, predecessor arcs of depths 0..ds) is staged in LDS
// once; the waves then take the tile's destinations in turn and do meet_kernel's search (other
// root: unreachable; LCA depth by binary search; min of F[d] + B[d] over the common depths, deepest
// tie) with the source side read from LDS; after a barrier lane p sums pair p's metres in
// meet_kernel's order (forward arcs from the meeting depth down to s, then backward ones down to t,
// f32 from 0.f), the tile's walks side by side instead of one lane per wave.  The output rule is
// fused: equal nodes and cells past nsrc / ndst are 0, unreachable ones +inf.
constexpr int MEET_TILE = 64;
constexpr int MEET_THREADS = 256;
__global__ __launch_bounds__(MEET_THREADS) void meet_rect_kernel(
    int SM, int DM, const int* __restrict__ nsrc, const int* __restrict__ ndst, const int32_t* __restrict__ jobs,
    int stride, const float* __restrict__ sdist, const int32_t* __restrict__ spred, const int32_t* __restrict__ snode,
    const int32_t* __restrict__ depth, const int32_t* __restrict__ arc_lo, const float* __restrict__ len_up,
    const float* __restrict__ len_dn, float* __restrict__ out_sec, float* __restrict__ out_met) {
  extern __shared__ unsigned char smem[];
  int32_t* fn = reinterpret_cast<int32_t*>(smem);
  float* fd = reinterpret_cast<float*>(smem + (size_t)stride * 4);
  int32_t* fp = reinterpret_cast<int32_t*>(smem + (size_t)stride * 8);
  __shared__ float s_best[MEET_TILE];
  __shared__ int s_bestd[MEET_TILE];
  const int tid = threadIdx.x;
  const int ntile = (DM + MEET_TILE - 1) / MEET_TILE;
  const int tile = blockIdx.x % ntile;
  const int i = (blockIdx.x / ntile) % SM;
  const int r = blockIdx.x / (ntile * SM);
  const int j0 = tile * MEET_TILE;
  const int nj = min(MEET_TILE, DM - j0);                     // cells of the tile
  const int nv = min(nj, ndst[r] - j0);                       // of which real destinations (may be <= 0)
  const size_t cell = ((size_t)r * SM + i) * DM + j0;
  if (i >= nsrc[r] || nv <= 0) {                              // padding only (uniform in the workgroup)
    if (tid < nj) {
      out_sec[cell + tid] = 0.f;
      out_met[cell + tid] = 0.f;
    }
    return;
  }
  const size_t jrow = (size_t)r * (SM + DM);
  const int s = jobs[jrow + i] >> 1;
  const int ds = depth[s];
  const size_t bf = (jrow + i) * stride;
  for (int d = tid; d <= ds; d += MEET_THREADS) {
    fn[d] = snode[bf + d];
    fd[d] = sdist[bf + d];
    fp[d] = spred[bf + d];
  }
  __syncthreads();
  const int lane = tid & 63;
  for (int p = tid >> 6; p < nv; p += MEET_THREADS / 64) {
    const size_t jb = jrow + SM + j0 + p;
    const int t = jobs[jb] >> 1;
    const int dt = depth[t];
    const size_t bb = jb * stride;
    float best = F_INF;
    int bestd = -1;
    if (fn[0] == snode[bb]) {
      // chains agree on depths [0, L]
      int lo = 0, hi = ds < dt ? ds : dt;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (fn[mid] == snode[bb + mid]) lo = mid;
        else hi = mid - 1;
      }
      const int L = lo;
      for (int d = lane; d <= L; d += 64) {
        const float v = fd[d] + sdist[bb + d];
        if (v < best || (v == best && d > bestd)) {
          best = v;
          bestd = d;
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int od = __shfl_xor(bestd, o);
        if (ov < best || (ov == best && od > bestd)) {
          best = ov;
          bestd = od;
        }
      }
    }
    if (lane == 0) {
      s_best[p] = best;
      s_bestd[p] = bestd;
    }
  }
  __syncthreads();
  if (tid >= nj) return;
  float sec = 0.f, met = 0.f;
  if (tid < nv) {
    const size_t jb = jrow + SM + j0 + tid;
    const int t = jobs[jb] >> 1;
    if (t != s) {
      sec = s_best[tid];
      if (sec < F_INF) {
        const int dt = depth[t];
        const size_t bb = jb * stride;
        const int bestd = s_bestd[tid];
        for (int slot = bestd; slot != ds;) {
          const int a = fp[slot];
          met += len_up[a];
          slot = depth[arc_lo[a]];
        }
        for (int slot = bestd; slot != dt;) {
          const int a = spred[bb + slot];
          met += len_dn[a];
          slot = depth[arc_lo[a]];
        }
      } else {
        sec = met = F_INF;
      }
    }
  }
  out_sec[cell + tid] = sec;
  out_met[cell + tid] = met;
}

// The same cells through meet_kernel (one wave per pair): pair job indices and the output rule
__global__ void rect_pairs_kernel(int R, int SM, int DM, int32_t* __restrict__ pjf, int32_t* __restrict__ pjb) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= (long long)R * SM * DM) return;
  const int r = (int)(g / ((long long)SM * DM));
  const int rem = (int)(g % ((long long)SM * DM));
  pjf[g] = r * (SM + DM) + rem / DM;
  pjb[g] = r * (SM + DM) + SM + rem % DM;
}

__global__ void rect_out_kernel(const int* __restrict__ nsrc, const int* __restrict__ ndst, int R, int SM, int DM,
                                const int32_t* __restrict__ jobs, float* __restrict__ sec, float* __restrict__ met) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= (long long)R * SM * DM) return;
  const int r = (int)(g / ((long long)SM * DM));
  const int rem = (int)(g % ((long long)SM * DM));
  const int i = rem / DM, j = rem % DM;
  float s = sec[g], m = met[g];
  const size_t jrow = (size_t)r * (SM + DM);
  if (i >= nsrc[r] || j >= ndst[r] || (jobs[jrow + i] >> 1) == (jobs[jrow + SM + j] >> 1)) s = m = 0.f;
  else {
    if (s < 0.f) s = F_INF;
    if (m < 0.f) m = F_INF;
  }
  sec[g] = s;
  met[g] = m;
}

}  // namespace

CchScratch::~CchScratch() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(device);
  dfree(dist);
  dfree(pred);
  dfree(node);
  dfree(jobs);
  dfree(arcs);
  dfree(narcs);
  dfree(pj);
  for (void* p : old) (void)hipFree(p);
  (void)hipSetDevice(cur);
}

// (outgrown buffers are kept until the scratch dies: a hipFree would wait for the whole device)
hipError_t CchScratch::ensure(size_t J, size_t P, int stride, int max_arcs) {
  hipError_t e = hipSuccess;
  auto retire = [&](auto*& p) {
    if (p) old.push_back((void*)p);
    p = nullptr;
  };
  if (J > jobs_cap) {
    retire(dist);
    retire(pred);
    retire(node);
    retire(jobs);
    const size_t cap = std::max(J, jobs_cap * 3 / 2);
    if ((e = dmalloc(dist, cap * stride)) != hipSuccess) return e;
    if ((e = dmalloc(pred, cap * stride)) != hipSuccess) return e;
    if ((e = dmalloc(node, cap * stride)) != hipSuccess) return e;
    if ((e = dmalloc(jobs, cap)) != hipSuccess) return e;
    jobs_cap = cap;
  }
  if (P > pairs_cap) {
    retire(arcs);
    retire(narcs);
    const size_t cap = std::max(P, pairs_cap * 3 / 2);
    if ((e = dmalloc(arcs, cap * (size_t)max_arcs)) != hipSuccess) return e;
    if ((e = dmalloc(narcs, cap)) != hipSuccess) return e;
    pairs_cap = cap;
  }
  return e;
}

hipError_t CchGpu::launch_unpack(const CchMetricDev* m, const CchMView* mv, const int* grp, int Q, const int* d_src,
                                 CchScratch& sc, const CchRouteOut& o, hipStream_t s) {
  const bool serial_only = unpack_serial();
  const int32_t* sub_up = m ? m->sub_up : nullptr;
  const int32_t* sub_dn = m ? m->sub_dn : nullptr;
  if (!serial_only) {
    constexpr int G = 64 / UNPACK_LANES;
    hipLaunchKernelGGL(unpack_coop_kernel, dim3((Q + G - 1) / G), dim3(64), 0, s, Q, d_src, sc.arcs, sc.narcs, MAX_ARCS,
                       sub_up, sub_dn, m ? m->cnt_up : nullptr, m ? m->cnt_dn : nullptr, d_arc_lo, d_up_head, d_node,
                       o.status, o.len, o.path, o.max_path, o.edges, mv, grp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(unpack_kernel, dim3(blocks_for(Q, 64)), dim3(64), 0, s, Q, d_src, sc.arcs, sc.narcs, MAX_ARCS,
                     sub_up, sub_dn, d_arc_lo, d_up_head, d_node, o.status, o.len, o.path, o.max_path,
                     serial_only ? -1 : UNPACK_MAX_ARCS, o.edges, mv, grp);
  return hipGetLastError();
}

hipError_t CchGpu::route_impl(const CchMetricDev* m, const CchMView* mv, const int* grp, const int* d_src,
                              const int* d_dst, int Q, const CchRouteOut& o, CchScratch& sc, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  const int S = stride();
  sc.device = dev_;
  sc.chain_tag = 0;
  hipError_t e = sc.ensure((size_t)2 * Q, (size_t)Q, S, MAX_ARCS);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(route_jobs_kernel, dim3(blocks_for(Q, 256)), dim3(256), 0, s, d_src, d_dst, Q, d_rank, T_.N,
                     sc.jobs);
  hipLaunchKernelGGL(sweep_kernel, dim3(2 * Q), dim3(64), (size_t)S * 8, s, sc.jobs, 2 * Q, d_parent, d_depth, T_.N,
                     m ? m->f_ptr : nullptr, m ? m->f_rec : nullptr, m ? m->b_ptr : nullptr, m ? m->b_rec : nullptr, S,
                     sc.dist, sc.pred, sc.node, mv, grp, 2);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(meet_kernel, dim3(Q), dim3(64), 0, s, Q, nullptr, nullptr, 0, 1, sc.jobs, S, sc.dist, sc.pred,
                     sc.node, d_depth, d_arc_lo, m ? m->len_up : nullptr, m ? m->len_dn : nullptr, o.sec, o.metres,
                     o.status, o.path ? sc.arcs : nullptr, o.path ? sc.narcs : nullptr, MAX_ARCS, mv, grp, 1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (o.path != nullptr) e = launch_unpack(m, mv, grp, Q, d_src, sc, o, s);
  return e;
}

hipError_t CchGpu::route(const CchMetricDev& m, const int* d_src, const int* d_dst, int Q, const CchRouteOut& o,
                         CchScratch& sc, hipStream_t s) {
  return route_impl(&m, nullptr, nullptr, d_src, d_dst, Q, o, sc, s);
}

hipError_t CchGpu::route_multi(const CchMView* d_mv, const int* d_grp, const int* d_src, const int* d_dst, int Q,
                               const CchRouteOut& o, CchScratch& sc, hipStream_t s) {
  if (d_mv == nullptr || d_grp == nullptr) return hipErrorInvalidValue;
  return route_impl(nullptr, d_mv, d_grp, d_src, d_dst, Q, o, sc, s);
}

hipError_t CchGpu::matrix_impl(const CchMetricDev* m, const CchMView* mv, const int* grp, const int* d_pts,
                               const int* d_npts, int R, int NM, float* d_sec, float* d_met, double* d_D64,
                               CchScratch& sc, hipStream_t s) {
  if (R <= 0 || NM <= 0) return hipSuccess;
  if (d_sec == nullptr || d_met == nullptr) return hipErrorInvalidValue;   // the meet writes both
  const int S = stride();
  sc.device = dev_;
  const size_t J = (size_t)R * NM * 2, P = (size_t)R * NM * NM;
  // pair job indices live in the arcs buffer (2 ints per pair)
  hipError_t e = sc.ensure(J, (P * 2 + MAX_ARCS - 1) / MAX_ARCS + 1, S, MAX_ARCS);
  if (e != hipSuccess) return e;
  int32_t* pjf = sc.arcs;
  int32_t* pjb = sc.arcs + P;
  float* sec = d_sec;
  float* met = d_met;
  hipLaunchKernelGGL(matrix_jobs_kernel, dim3(blocks_for((long long)R * NM, 256)), dim3(256), 0, s, d_pts, d_npts, R, NM,
                     d_rank, T_.N, sc.jobs);
  hipLaunchKernelGGL(matrix_pairs_kernel, dim3(blocks_for((long long)P, 256)), dim3(256), 0, s, d_npts, R, NM, pjf, pjb);
  // (job 2(r NM + i) + dir and pair r NM^2 + i NM + j belong to request row r)
  hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)J), dim3(64), (size_t)S * 8, s, sc.jobs, (int)J, d_parent, d_depth,
                     T_.N, m ? m->f_ptr : nullptr, m ? m->f_rec : nullptr, m ? m->b_ptr : nullptr,
                     m ? m->b_rec : nullptr, S, sc.dist, sc.pred, sc.node, mv, grp, 2 * NM);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(meet_kernel, dim3((unsigned)P), dim3(64), 0, s, (int)P, pjf, pjb, 0, 0, sc.jobs, S, sc.dist,
                     sc.pred, sc.node, d_depth, d_arc_lo, m ? m->len_up : nullptr, m ? m->len_dn : nullptr, sec, met,
                     nullptr, nullptr, nullptr, MAX_ARCS, mv, grp, NM * NM);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(matrix_out_kernel, dim3(blocks_for((long long)P, 256)), dim3(256), 0, s, d_npts, R, NM, sec, met,
                     d_D64);
  e = hipGetLastError();
  sc.chain_tag = e == hipSuccess ? ++tag_ctr_ : 0;
  sc.chain_nm = NM;
  sc.chain_r = R;
  return e;
}

hipError_t CchGpu::matrix(const CchMetricDev& m, const int* d_pts, const int* d_npts, int R, int NM, float* d_sec,
                          float* d_met, double* d_D64, CchScratch& sc, hipStream_t s) {
  return matrix_impl(&m, nullptr, nullptr, d_pts, d_npts, R, NM, d_sec, d_met, d_D64, sc, s);
}

hipError_t CchGpu::matrix_multi(const CchMView* d_mv, const int* d_row_grp, const int* d_pts, const int* d_npts, int R,
                                int NM, float* d_sec, float* d_met, double* d_D64, CchScratch& sc, hipStream_t s) {
  if (d_mv == nullptr || d_row_grp == nullptr) return hipErrorInvalidValue;
  return matrix_impl(nullptr, d_mv, d_row_grp, d_pts, d_npts, R, NM, d_sec, d_met, d_D64, sc, s);
}

hipError_t CchGpu::matrix_rect(const CchMetricDev& m, const int* d_src, const int* d_nsrc, const int* d_dst,
                               const int* d_ndst, int R, int SM, int DM, float* d_sec, float* d_met, CchScratch& sc,
                               hipStream_t s, int meet) {
  if (R <= 0 || SM <= 0 || DM <= 0) return hipSuccess;
  if (d_sec == nullptr || d_met == nullptr || meet < MEET_AUTO || meet > MEET_NONE) return hipErrorInvalidValue;
  const int S = stride();
  const size_t J = (size_t)R * ((size_t)SM + DM), P = (size_t)R * SM * DM;
  if (J > (size_t)INT32_MAX || P > (size_t)INT32_MAX) return hipErrorInvalidValue;
  const size_t lds = (size_t)S * 12;
  const bool fits = lds + MEET_TILE * 8 <= 64 * 1024;          // else the chains do not fit one workgroup's LDS
  if (meet == MEET_RECT && !fits) return hipErrorInvalidValue;
  if (meet == MEET_AUTO) meet = fits ? MEET_RECT : MEET_PAIRS;
  sc.device = dev_;
  sc.chain_tag = 0;                                            // a kept matrix's chains are overwritten
  // (MEET_PAIRS: the pair job indices live in the arcs buffer, 2 ints per pair)
  hipError_t e = sc.ensure(J, meet == MEET_PAIRS ? (P * 2 + MAX_ARCS - 1) / MAX_ARCS + 1 : 0, S, MAX_ARCS);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rect_jobs_kernel, dim3(blocks_for((long long)J, 256)), dim3(256), 0, s, d_src, d_nsrc, d_dst,
                     d_ndst, R, SM, DM, d_rank, T_.N, sc.jobs);
  hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)J), dim3(64), (size_t)S * 8, s, sc.jobs, (int)J, d_parent, d_depth,
                     T_.N, m.f_ptr, m.f_rec, m.b_ptr, m.b_rec, S, sc.dist, sc.pred, sc.node, nullptr, nullptr, 1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (meet == MEET_RECT) {
    const size_t blocks = (size_t)R * SM * ((DM + MEET_TILE - 1) / MEET_TILE);
    hipLaunchKernelGGL(meet_rect_kernel, dim3((unsigned)blocks), dim3(MEET_THREADS), lds, s, SM, DM, d_nsrc, d_ndst,
                       sc.jobs, S, sc.dist, sc.pred, sc.node, d_depth, d_arc_lo, m.len_up, m.len_dn, d_sec, d_met);
  } else if (meet == MEET_PAIRS) {
    int32_t* pjf = sc.arcs;
    int32_t* pjb = sc.arcs + P;
    hipLaunchKernelGGL(rect_pairs_kernel, dim3(blocks_for((long long)P, 256)), dim3(256), 0, s, R, SM, DM, pjf, pjb);
    hipLaunchKernelGGL(meet_kernel, dim3((unsigned)P), dim3(64), 0, s, (int)P, pjf, pjb, 0, 0, sc.jobs, S, sc.dist,
                       sc.pred, sc.node, d_depth, d_arc_lo, m.len_up, m.len_dn, d_sec, d_met, nullptr, nullptr, nullptr,
                       MAX_ARCS, nullptr, nullptr, 1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rect_out_kernel, dim3(blocks_for((long long)P, 256)), dim3(256), 0, s, d_nsrc, d_ndst, R, SM, DM,
                       sc.jobs, d_sec, d_met);
  }
  return hipGetLastError();
}

hipError_t CchGpu::legs_impl(const CchMetricDev* m, const CchMView* mv, const int* grp, const int* d_src,
                             const int* d_r, const int* d_i, const int* d_j, int Q, uint64_t tag, const CchRouteOut& o,
                             CchScratch& sc, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  if (tag == 0 || tag != sc.chain_tag) return hipErrorInvalidValue;   // chains overwritten since
  const int S = stride();
  hipError_t e = sc.ensure(0, (size_t)Q, S, MAX_ARCS);
  if (e != hipSuccess) return e;
  if ((size_t)Q > sc.pj_cap) {
    if (sc.pj) sc.old.push_back((void*)sc.pj);
    sc.pj = nullptr;
    const size_t cap = std::max((size_t)Q, sc.pj_cap * 3 / 2);
    if ((e = dmalloc(sc.pj, 2 * cap)) != hipSuccess) return e;
    sc.pj_cap = cap;
  }
  int32_t* pjf = sc.pj;
  int32_t* pjb = sc.pj + sc.pj_cap;
  hipLaunchKernelGGL(leg_pairs_kernel, dim3(blocks_for(Q, 256)), dim3(256), 0, s, sc.chain_nm, d_r, d_i, d_j, Q,
                     sc.chain_r, pjf, pjb);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(meet_kernel, dim3(Q), dim3(64), 0, s, Q, pjf, pjb, 0, 0, sc.jobs, S, sc.dist, sc.pred, sc.node,
                     d_depth, d_arc_lo, m ? m->len_up : nullptr, m ? m->len_dn : nullptr, o.sec, o.metres, o.status,
                     o.path ? sc.arcs : nullptr, o.path ? sc.narcs : nullptr, MAX_ARCS, mv, grp, 1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (o.path != nullptr) e = launch_unpack(m, mv, grp, Q, d_src, sc, o, s);
  return e;
}

hipError_t CchGpu::legs_from_matrix(const CchMetricDev& m, const int* d_src, const int* d_r, const int* d_i,
                                    const int* d_j, int Q, uint64_t tag, const CchRouteOut& o, CchScratch& sc,
                                    hipStream_t s) {
  return legs_impl(&m, nullptr, nullptr, d_src, d_r, d_i, d_j, Q, tag, o, sc, s);
}

hipError_t CchGpu::legs_from_matrix_multi(const CchMView* d_mv, const int* d_grp, const int* d_src, const int* d_r,
                                          const int* d_i, const int* d_j, int Q, uint64_t tag, const CchRouteOut& o,
                                          CchScratch& sc, hipStream_t s) {
  if (d_mv == nullptr || d_grp == nullptr) return hipErrorInvalidValue;
  return legs_impl(nullptr, d_mv, d_grp, d_src, d_r, d_i, d_j, Q, tag, o, sc, s);
}

}  // namespace rt
