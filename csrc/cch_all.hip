// GPU customizable contraction hierarchy, one-to-all: every node's time-shortest seconds (and the
// metres of that path) from each of S sources — the isochrone primitive.  CPU reference, bit for
// bit: rcch::one_to_all (csrc/runtime/cch.h).
//
// The source's etree chain is swept upward once over its kept forward arcs, then every node, in
// etree depth order, pulls from the heads of its kept backward arcs.  A head is an ancestor, so it
// sits on a smaller depth level and is final: every label is written by exactly one thread after
// everything it reads — no atomics.  Labels are the lexicographic minimum of (seconds, metres) over
// the candidates, which does not depend on the order they arrive in; sums are single f32 adds (this
// file is built with -ffp-contract=off).
//
// Work labels: seconds and metres as [blocks][N][64] in rank space, 64 sources per block on the lane
// axis.  A wave that handles node v reads v's records wave-uniformly and reads / writes 256-byte
// label rows.  Lanes past the last source stay +inf.
//
//   cch_all_fill_kernel        labels = +inf
//   cch_all_up_kernel          one wave per source: the chain sweep with labels in LDS by depth,
//                              scattered into the source's lane of the work arrays
//   cch_all_pull_kernel        one depth level, one workgroup per (node, source block): its 1, 2, 4
//                              or 8 waves split the node's records
//   cch_all_pull_fused_kernel  a run of consecutive narrow levels in one launch: one workgroup per
//                              source block, its 16 waves split each level's nodes and records, a
//                              barrier between levels (most levels of a road hierarchy are a few
//                              separator nodes wide: a launch each costs more than their work)
//   cch_all_out_kernel         [S][N] by node id, through a 64 x 64 LDS transpose so both the reads
//                              and the writes are whole 256-byte rows
#include <algorithm>
#include <cstdlib>

#include "cch_dev.h"
#include "cch_gpu.h"

namespace rt {

using namespace cchd;

namespace {

constexpr int ALL_FUSED_THREADS = 1024;   // 16 waves per source block in the fused kernel
constexpr int ALL_FUSE_MAX = ALL_FUSED_THREADS / 64;
constexpr int ALL_ROWS = 16;              // label rows a wave keeps in flight
constexpr int ALL_PRE = 64 / ALL_ROWS;    // chunks of ALL_ROWS records whose (w, head, metres) a wave fetches at once

__device__ __forceinline__ bool label_less(float s1, float m1, float s0, float m0) {
  return s1 < s0 || (s1 == s0 && m1 < m0);
}

__global__ __launch_bounds__(256) void cch_all_fill_kernel(float4* __restrict__ sec, float4* __restrict__ met,
                                                           long long n4) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g >= n4) return;
  const float4 v = make_float4(F_INF, F_INF, F_INF, F_INF);
  sec[g] = v;
  met[g] = v;
}

// One wave per source j of the chunk (block j / 64, lane j % 64).  ptr / rec / len: the kept arcs the
// sweep climbs (forward: f_*, len_up).  A record's .y is its head's depth — the head's LDS slot.
__global__ __launch_bounds__(64) void cch_all_up_kernel(const int* __restrict__ src, int cnt,
                                                        const int32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ parent,
                                                        const int32_t* __restrict__ depth,
                                                        const int32_t* __restrict__ ptr, const int4* __restrict__ rec,
                                                        const float* __restrict__ len, int N, int stride,
                                                        float* __restrict__ wsec, float* __restrict__ wmet) {
  extern __shared__ unsigned char smem[];
  float* sd = reinterpret_cast<float*>(smem);
  float* sm = sd + stride;
  int32_t* sn = reinterpret_cast<int32_t*>(sm + stride);
  const int j = blockIdx.x;
  if (j >= cnt) return;
  const int lane = threadIdx.x;
  const int node = src[j];
  if (node < 0 || node >= N) return;        // (the callers range-check; never index with a bad id)
  const int r = rank[node];
  const int D = depth[r];
  if (D >= stride) return;
  for (int d = lane; d <= D; d += 64) {
    sd[d] = F_INF;
    sm[d] = F_INF;
    sn[d] = -1;
  }
  __syncthreads();
  if (lane == 0) {
    sd[D] = 0.f;
    sm[D] = 0.f;
  }
  __syncthreads();
  int x = r;
  for (int d = D; d >= 0 && x >= 0; --d) {
    const int par = parent[x];
    const int kb = ptr[x], ke = ptr[x + 1];
    if (lane == 0) sn[d] = x;
    const float dx = sd[d], mx = sm[d];
    if (dx < F_INF) {
      // a node's kept arcs have distinct heads: the lanes' updates never collide
      for (int k = kb + lane; k < ke; k += 64) {
        const int4 rc = rec[k];
        const int hd = rc.y;
        const float cs = dx + __int_as_float(rc.x);
        const float cm = mx + len[rc.z];
        if (hd >= 0 && hd < d && label_less(cs, cm, sd[hd], sm[hd])) {
          sd[hd] = cs;
          sm[hd] = cm;
        }
      }
    }
    __syncthreads();
    x = par;
  }
  const size_t base = (size_t)(j >> 6) * (size_t)N * 64 + (size_t)(j & 63);
  for (int d = lane; d <= D; d += 64) {
    const int y = sn[d];
    if (y < 0) continue;
    wsec[base + (size_t)y * 64] = sd[d];
    wmet[base + (size_t)y * 64] = sm[d];
  }
}

// The label rows of n (1..ALL_ROWS) heads, all in flight at once, folded into (bs, bm): lane l0 + q,
// q < n, of (w_l, u_l, m_l) holds record q's weight bits, head rank and metres bits.  Indices past
// the last record repeat it: a minimum takes the same candidate twice unharmed.
__device__ __forceinline__ void pull_rows(int n, int l0, int w_l, int u_l, int m_l, size_t base, const float* wsec,
                                          const float* wmet, float& bs, float& bm) {
  float ls[ALL_ROWS], lm[ALL_ROWS];
#pragma unroll
  for (int q = 0; q < ALL_ROWS; ++q) {
    const int u = __builtin_amdgcn_readlane(u_l, l0 + (q < n ? q : n - 1));
    ls[q] = wsec[base + (size_t)u * 64];
    lm[q] = wmet[base + (size_t)u * 64];
  }
#pragma unroll
  for (int q = 0; q < ALL_ROWS; ++q) {
    const int ii = l0 + (q < n ? q : n - 1);
    const float cs = ls[q] + __int_as_float(__builtin_amdgcn_readlane(w_l, ii));
    const float cm = lm[q] + __int_as_float(__builtin_amdgcn_readlane(m_l, ii));
    if (ls[q] < F_INF && label_less(cs, cm, bs, bm)) {
      bs = cs;
      bm = cm;
    }
  }
}

// A node's kept arcs of the pull direction are dealt to the `parts` waves that share the node in
// chunks of ALL_ROWS records: chunk t of part `part` starts at record kb + ALL_ROWS * (part + parts * t).
// A wave fetches ALL_PRE of its chunks at once — lane ALL_ROWS * t' + q holds record q of chunk
// t0 + t': (weight bits, head rank, metres bits) — and then reads the chunks' rows, ALL_ROWS
// together (the pass is a chain of dependent loads: rows in flight are all the parallelism it has).
__device__ __forceinline__ int chunk_record(int kb, int part, int parts, int t0, int lane) {
  return kb + ALL_ROWS * (part + parts * (t0 + lane / ALL_ROWS)) + lane % ALL_ROWS;
}

// the rows of chunks t0 .. t0 + ALL_PRE - 1, whose records the lanes hold, folded into (bs, bm)
__device__ __forceinline__ void pull_chunks(int kb, int ke, int part, int parts, int t0, int w_l, int u_l, int m_l,
                                            size_t base, const float* wsec, const float* wmet, float& bs, float& bm) {
#pragma unroll
  for (int t = 0; t < ALL_PRE; ++t) {
    const int left = ke - (kb + ALL_ROWS * (part + parts * (t0 + t)));      // records from the chunk's first
    if (left > 0) pull_rows(left < ALL_ROWS ? left : ALL_ROWS, ALL_ROWS * t, w_l, u_l, m_l, base, wsec, wmet, bs, bm);
  }
}

// part `part` of a node's pull from its chunk t0 on: (bs, bm) = the lexicographic minimum of itself
// and, per record, the head's label row + (w, metres)
__device__ __forceinline__ void pull_part(int kb, int ke, int part, int parts, int t0, size_t base, int lane,
                                          const int4* __restrict__ rec, const int32_t* __restrict__ up_head,
                                          const float* __restrict__ len, const float* wsec, const float* wmet,
                                          float& bs, float& bm) {
  for (; kb + ALL_ROWS * (part + parts * t0) < ke; t0 += ALL_PRE) {
    const int k = chunk_record(kb, part, parts, t0, lane);
    int w_l = 0, u_l = 0, m_l = 0;
    if (k < ke) {
      const int4 rc = rec[k];
      w_l = rc.x;
      u_l = up_head[rc.z];
      m_l = __float_as_int(len[rc.z]);
    }
    pull_chunks(kb, ke, part, parts, t0, w_l, u_l, m_l, base, wsec, wmet, bs, bm);
  }
}

// One depth level: nodes dnodes[lb .. lb + cnt), one workgroup of WAVES waves per (node, source
// block); the waves split the node's records and wave 0 merges their minima with the node's own
// label (the up-sweep's, or +inf) and writes the row.  The host picks WAVES per level from the
// level's widest node, so that a wave gets one chunk where eight waves reach that far.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void cch_all_pull_kernel(
    const int32_t* __restrict__ dnodes, int lb, int cnt, int nblk, int N, const int32_t* __restrict__ ptr,
    const int4* __restrict__ rec, const int32_t* __restrict__ up_head, const float* __restrict__ len, float* wsec,
    float* wmet) {
  __shared__ float red_s[WAVES][64], red_m[WAVES][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ni = blockIdx.x / nblk, b = blockIdx.x % nblk;
  if (ni >= cnt) return;
  const int v = dnodes[lb + ni];
  const int kb = ptr[v], ke = ptr[v + 1];
  if (ke <= kb) return;
  const size_t base = (size_t)b * (size_t)N * 64 + (size_t)lane;
  const size_t row = base + (size_t)v * 64;
  float bs = F_INF, bm = F_INF;
  if (wave == 0) {
    bs = wsec[row];
    bm = wmet[row];
  }
  pull_part(kb, ke, wave, WAVES, 0, base, lane, rec, up_head, len, wsec, wmet, bs, bm);
  if (WAVES > 1) {
    red_s[wave][lane] = bs;
    red_m[wave][lane] = bm;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int p = 1; p < WAVES; ++p)
      if (label_less(red_s[p][lane], red_m[p][lane], bs, bm)) {
        bs = red_s[p][lane];
        bm = red_m[p][lane];
      }
  }
  wsec[row] = bs;
  wmet[row] = bm;
}

// Depth levels [d0, d1), each of at most 16 nodes: workgroup b takes source block b through all of
// them, a barrier between levels.  A level of `width` nodes gives each node 16 / width waves, which
// split its records in chunks of ALL_ROWS; the node's first wave merges their minima (through LDS)
// with the node's own label and writes the row.  A level reads only rows of smaller depths, written
// by this workgroup before the barrier that ends their level (__syncthreads orders the workgroup's
// global writes and reads).
//
// What a wave needs before it can read rows — the level's bounds, its node, the node's record
// range, its first 64 records, their heads and metres — is a chain of five dependent loads that does
// not depend on any label.  It is software-pipelined across levels: iteration d issues stage 1 of
// level d + 5 .. stage 5 of level d + 1, each from what the stage before it fetched one iteration
// earlier, and only then reads the rows of level d.  So a level costs one round trip to memory, not
// six.  (The barrier drains every load of the iteration; they were issued before the rows.)
__global__ __launch_bounds__(ALL_FUSED_THREADS) void cch_all_pull_fused_kernel(
    const int32_t* __restrict__ dlev_ptr, const int32_t* __restrict__ dnodes, int d0, int d1, int N,
    const int32_t* __restrict__ ptr, const int4* __restrict__ rec, const int32_t* __restrict__ up_head,
    const float* __restrict__ len, float* wsec, float* wmet) {
  constexpr int NW = ALL_FUSED_THREADS / 64;
  __shared__ float red_s[NW][64], red_m[NW][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t base = (size_t)blockIdx.x * (size_t)N * 64 + (size_t)lane;
  // pipeline registers, named by the stage that filled them (all 0: an idle wave or no level)
  int lb1 = 0, width1 = 0;                                    // stage 1: the level's node range
  int act2 = 0, part2 = 0, parts2 = 1, v2 = 0;                // stage 2: this wave's node and share
  int act3 = 0, part3 = 0, parts3 = 1, v3 = 0, kb3 = 0, ke3 = 0;   // stage 3: the node's records
  int act4 = 0, part4 = 0, parts4 = 1, v4 = 0, kb4 = 0, ke4 = 0, n4 = 0;   // stage 4: its first 64 records (n: this lane has one)
  int4 rc4 = make_int4(0, 0, 0, 0);
  int act5 = 0, part5 = 0, parts5 = 1, v5 = 0, kb5 = 0, ke5 = 0;   // stage 5: their heads and metres
  int w5 = 0, u5 = 0, m5 = 0;
  for (int d = d0 - 5; d < d1; ++d) {
    // level d: what stage 5 fetched last iteration
    const int act = act5, part = part5, parts = parts5, v = v5, kb = kb5, ke = ke5;
    const int w_l = w5, u_l = u5, m_l = m5;
    // stage 5 of level d + 1
    act5 = act4, part5 = part4, parts5 = parts4, v5 = v4, kb5 = kb4, ke5 = ke4;
    w5 = rc4.x;
    u5 = m5 = 0;
    if (n4) {
      u5 = up_head[rc4.z];
      m5 = __float_as_int(len[rc4.z]);
    }
    // stage 4 of level d + 2
    act4 = act3, part4 = part3, parts4 = parts3, v4 = v3, kb4 = kb3, ke4 = ke3;
    {
      const int k = chunk_record(kb3, part3, parts3, 0, lane);         // (n4: the lane has a record)
      n4 = act3 && k < ke3;
      rc4 = make_int4(0, 0, 0, 0);
      if (n4) rc4 = rec[k];
    }
    // stage 3 of level d + 3
    act3 = act2, part3 = part2, parts3 = parts2, v3 = v2;
    kb3 = ke3 = 0;
    if (act2) {
      kb3 = ptr[v2];
      ke3 = ptr[v2 + 1];
    }
    // stage 2 of level d + 4
    act2 = 0, part2 = 0, parts2 = 1, v2 = 0;
    if (width1 > 0 && width1 <= NW) {
      parts2 = NW / width1;
      part2 = wave % parts2;
      const int ni = wave / parts2;
      if (ni < width1) {
        act2 = 1;
        v2 = dnodes[lb1 + ni];
      }
    }
    // stage 1 of level d + 5
    lb1 = width1 = 0;
    if (d + 5 >= d0 && d + 5 < d1) {
      lb1 = dlev_ptr[d + 5];
      width1 = dlev_ptr[d + 6] - lb1;
    }
    if (d < d0) continue;                   // filling the pipeline
    size_t row = 0;
    float bs = F_INF, bm = F_INF;
    if (act) {
      row = base + (size_t)v * 64;
      if (part == 0) {
        bs = wsec[row];
        bm = wmet[row];
      }
      pull_chunks(kb, ke, part, parts, 0, w_l, u_l, m_l, base, wsec, wmet, bs, bm);
      pull_part(kb, ke, part, parts, ALL_PRE, base, lane, rec, up_head, len, wsec, wmet, bs, bm);
      red_s[wave][lane] = bs;
      red_m[wave][lane] = bm;
    }
    __syncthreads();
    if (act && part == 0) {
      for (int p = 1; p < parts; ++p)
        if (label_less(red_s[wave + p][lane], red_m[wave + p][lane], bs, bm)) {
          bs = red_s[wave + p][lane];
          bm = red_m[wave + p][lane];
        }
      wsec[row] = bs;
      wmet[row] = bm;
    }
    __syncthreads();
  }
}

// out[s0 + l][n] = work[b][rank[n]][l] for a tile of 64 node ids x the 64 sources of block b
// (blockIdx.z: seconds | metres).  Rows are read lane = source and written lane = node id.
__global__ __launch_bounds__(256) void cch_all_out_kernel(const int32_t* __restrict__ rank, int N, int cnt,
                                                          const float* __restrict__ wsec,
                                                          const float* __restrict__ wmet, float* __restrict__ osec,
                                                          float* __restrict__ omet) {
  __shared__ float tile[64][65];
  const float* __restrict__ w = blockIdx.z == 0 ? wsec : wmet;
  float* __restrict__ o = blockIdx.z == 0 ? osec : omet;
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)b * (size_t)N * 64;
  for (int i = wave; i < 64; i += 4) {
    const int n = n0 + i;
    if (n < N) tile[i][lane] = w[base + (size_t)rank[n] * 64 + lane];
  }
  __syncthreads();
  const int nl = cnt - b * 64 < 64 ? cnt - b * 64 : 64;    // sources of this block
  if (n0 + lane < N)
    for (int l = wave; l < nl; l += 4) o[(size_t)(b * 64 + l) * (size_t)N + n0 + lane] = tile[lane][l];
}

}  // namespace

CchAllScratch::~CchAllScratch() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(device);
  dfree(sec);
  dfree(met);
  for (void* p : old) (void)hipFree(p);
  (void)hipSetDevice(cur);
}

// (outgrown buffers are kept until the scratch dies: a hipFree would wait for the whole device)
hipError_t CchAllScratch::ensure(size_t blocks, size_t N) {
  if (blocks <= blocks_cap) return hipSuccess;
  if (sec) old.push_back((void*)sec);
  if (met) old.push_back((void*)met);
  sec = met = nullptr;
  blocks_cap = 0;
  hipError_t e;
  if ((e = dmalloc(sec, blocks * N * 64)) != hipSuccess) return e;
  if ((e = dmalloc(met, blocks * N * 64)) != hipSuccess) return e;
  blocks_cap = blocks;
  return hipSuccess;
}

hipError_t CchGpu::one_to_all(const CchMetricDev& m, const int* d_src, int S, bool reverse, float* d_sec, float* d_met,
                              CchAllScratch& sc, hipStream_t s, int fuse) {
  if (S <= 0) return hipSuccess;
  if (d_src == nullptr || d_sec == nullptr || d_met == nullptr) return hipErrorInvalidValue;
  static const int fuse_default = [] {
    const char* v = std::getenv("ROUTEST_CCH_ALL_FUSE");
    return v ? std::max(0, std::atoi(v)) : ALL_FUSE_WIDTH;
  }();
  if (fuse < 0) fuse = fuse_default;
  fuse = std::min(fuse, ALL_FUSE_MAX);      // the fused kernel gives every node of a level at least one wave
  const int N = T_.N, ST = stride();
  const size_t up_lds = (size_t)ST * 12;
  if (up_lds > 64 * 1024) return hipErrorInvalidValue;      // the chain's labels must fit LDS
  // up-sweep climbs the kept forward arcs, the pull descends the kept backward ones; reverse swaps them
  const int32_t* u_ptr = reverse ? m.b_ptr : m.f_ptr;
  const int4* u_rec = reverse ? m.b_rec : m.f_rec;
  const float* u_len = reverse ? m.len_dn : m.len_up;
  const int32_t* p_ptr = reverse ? m.f_ptr : m.b_ptr;
  const int4* p_rec = reverse ? m.f_rec : m.b_rec;
  const float* p_len = reverse ? m.len_up : m.len_dn;
  // source blocks per chunk: both work arrays within ALL_SCRATCH_BYTES (at least one block)
  const size_t block_bytes = (size_t)N * 64 * 4 * 2;
  const int total_blocks = (S + 63) / 64;
  const int chunk_blocks = (int)std::min<size_t>((size_t)total_blocks, std::max<size_t>(1, ALL_SCRATCH_BYTES / block_bytes));
  sc.device = dev_;
  hipError_t e = sc.ensure((size_t)chunk_blocks, (size_t)N);
  if (e != hipSuccess) return e;
  for (int c0 = 0; c0 < total_blocks; c0 += chunk_blocks) {
    const int nb = std::min(chunk_blocks, total_blocks - c0);
    const int s0 = c0 * 64;
    const int cnt = std::min(S - s0, nb * 64);
    const long long n4 = (long long)nb * N * 16;
    hipLaunchKernelGGL(cch_all_fill_kernel, dim3(blocks_for(n4, 256)), dim3(256), 0, s,
                       reinterpret_cast<float4*>(sc.sec), reinterpret_cast<float4*>(sc.met), n4);
    hipLaunchKernelGGL(cch_all_up_kernel, dim3(cnt), dim3(64), up_lds, s, d_src + s0, cnt, d_rank, d_parent, d_depth,
                       u_ptr, u_rec, u_len, N, ST, sc.sec, sc.met);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // depth 0 holds the roots (no upward arcs: nothing to pull)
    for (int d = 1; d <= T_.max_depth;) {
      int d1 = d;
      while (fuse > 0 && d1 <= T_.max_depth && T_.dlev_ptr[d1 + 1] - T_.dlev_ptr[d1] <= fuse) ++d1;
      if (d1 - d >= 2) {
        hipLaunchKernelGGL(cch_all_pull_fused_kernel, dim3(nb), dim3(ALL_FUSED_THREADS), 0, s, d_dlev_ptr, d_dnodes, d,
                           d1, N, p_ptr, p_rec, d_up_head, p_len, sc.sec, sc.met);
        d = d1;
      } else {
        const int lb = (int)T_.dlev_ptr[d], lc = (int)(T_.dlev_ptr[d + 1] - T_.dlev_ptr[d]);
        // waves per node: one per ALL_ROWS-record chunk of the level's widest node (its upward arcs
        // bound its kept ones), eight at the most
        const int kmax = plev_kmax_[d];
        const dim3 grid((unsigned)((long long)lc * nb));
        auto launch = [&](auto kernel, int waves) {
          hipLaunchKernelGGL(kernel, grid, dim3(64 * waves), 0, s, d_dnodes, lb, lc, nb, N, p_ptr, p_rec, d_up_head, p_len,
                             sc.sec, sc.met);
        };
        if (kmax <= ALL_ROWS) launch(cch_all_pull_kernel<1>, 1);
        else if (kmax <= 2 * ALL_ROWS) launch(cch_all_pull_kernel<2>, 2);
        else if (kmax <= 4 * ALL_ROWS) launch(cch_all_pull_kernel<4>, 4);
        else launch(cch_all_pull_kernel<8>, 8);
        ++d;
      }
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(cch_all_out_kernel, dim3(blocks_for(N, 64), nb, 2), dim3(256), 0, s, d_rank, N, cnt, sc.sec,
                       sc.met, d_sec + (size_t)s0 * N, d_met + (size_t)s0 * N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rt
