// GPS-trace map matching, host reference (the definition is in routest_amd/routing/mapmatch.py;
// the HIP kernels are csrc/map_match.hip).  Everything here is integer arithmetic on coordinates the
// caller quantized to centimetres, so the three implementations agree with ==.
//
//   MmGrid         integer bucket grid over the quantized node coordinates (in the spirit of
//                  route_core.h NodeGrid, but on (qy, qx) and for radius queries)
//   mm_candidates  per fix the k nodes within radius_cm with the smallest (d2, node id)
//   mm_viterbi     the segmenting Viterbi over given costs: lowest-i / lowest-j ties, a step at which
//                  every state is dead starts a new segment
//   MmEdgeGrid / mm_edge_candidates / mm_edge_route_cm
//                  edge-based matching (routing/mapmatch_edge.py): per fix the k edges within
//                  radius_cm with the smallest (d2 to the projection, edge id), and the route
//                  centimetres between two points on edges from a matrix row's metres
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

namespace rtr {

constexpr int kMmMaxK = 16;
constexpr int kMmMaxPoints = 2048;
// Score bounds (MatchParams in mapmatch.py): k <= 16, radius <= 1e5 cm, beta <= 1e4 cm, sigma <=
// 2e4 cm, max_detour <= 5e5 cm, at most 2048 fixes.  A step adds at most emit = 1e4 * 1e10 and
// trans = 2 * 4e8 * 5e5, so a path score stays below 2048 * (1e14 + 4e14) ~ 1.0e18 < kMmDead.
constexpr int64_t kMmDead = (int64_t)1 << 62;

// exact floor square root: a double estimate corrected by integer comparison
inline int64_t mm_isqrt(int64_t x) {
  if (x <= 0) return 0;
  int64_t s = (int64_t)std::sqrt((double)x);
  while (s > 0 && (uint64_t)s * (uint64_t)s > (uint64_t)x) --s;
  while ((uint64_t)(s + 1) * (uint64_t)(s + 1) <= (uint64_t)x) ++s;
  return s;
}

struct MmGrid {
  int64_t y0 = 0, x0 = 0, cell = 1;
  int ny = 0, nx = 0;
  std::vector<int32_t> start, items;   // CSR over row-major cells
  std::vector<int64_t> qy, qx;         // the nodes' quantized coordinates

  void build(const int64_t* y, const int64_t* x, size_t n) {
    if (n == 0 || n >= ((size_t)1 << 30)) throw std::invalid_argument("MmGrid: 1 .. 2^30 - 1 nodes");
    qy.assign(y, y + n);
    qx.assign(x, x + n);
    int64_t y1 = y[0], x1 = x[0];
    y0 = y[0];
    x0 = x[0];
    for (size_t i = 1; i < n; ++i) {
      y0 = std::min(y0, y[i]);
      y1 = std::max(y1, y[i]);
      x0 = std::min(x0, x[i]);
      x1 = std::max(x1, x[i]);
    }
    if (y1 - y0 > ((int64_t)1 << 40) || x1 - x0 > ((int64_t)1 << 40) || y0 < -((int64_t)1 << 40) ||
        x0 < -((int64_t)1 << 40))
      throw std::invalid_argument("MmGrid: coordinates out of range");
    const int64_t sy = y1 - y0 + 1, sx = x1 - x0 + 1;
    // about two nodes per cell, at most 2048 cells per axis
    cell = (int64_t)std::sqrt((double)sy * (double)sx / std::max(1.0, (double)n / 2.0));
    cell = std::max<int64_t>({100, cell, std::max(sy, sx) / 2048 + 1});
    ny = (int)((y1 - y0) / cell) + 1;
    nx = (int)((x1 - x0) / cell) + 1;
    start.assign((size_t)ny * nx + 1, 0);
    for (size_t i = 0; i < n; ++i) ++start[cell_of(i) + 1];
    for (size_t c = 0; c < (size_t)ny * nx; ++c) start[c + 1] += start[c];
    items.resize(n);
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) items[at[cell_of(i)]++] = (int32_t)i;
  }
  size_t cell_of(size_t i) const { return (size_t)((qy[i] - y0) / cell) * nx + (size_t)((qx[i] - x0) / cell); }
};

// cand [P, k] (-1 padded), cand_d2 [P, k] (-1 padded), n_cand [P]
inline void mm_candidates(const MmGrid& g, const int64_t* py, const int64_t* px, size_t P, int64_t radius_cm,
                          int k, int32_t* cand, int64_t* cand_d2, int32_t* n_cand) {
  if (k < 1 || k > kMmMaxK) throw std::invalid_argument("mm_candidates: k in 1..16");
  if (radius_cm < 1 || radius_cm > 100000) throw std::invalid_argument("mm_candidates: radius in 1..100000 cm");
  const int64_t r2 = radius_cm * radius_cm;
  std::vector<std::pair<int64_t, int32_t>> found;
  for (size_t p = 0; p < P; ++p) {
    for (int j = 0; j < k; ++j) {
      cand[p * k + j] = -1;
      cand_d2[p * k + j] = -1;
    }
    n_cand[p] = 0;
    constexpr int64_t lim = (int64_t)1 << 40;   // far beyond any quantized coordinate (|q| < 2^33)
    if (py[p] > lim || py[p] < -lim || px[p] > lim || px[p] < -lim)
      throw std::invalid_argument("mm_candidates: fix coordinate out of range");
    // the cells the radius covers, clamped to the grid (empty when the fix lies beyond it)
    const int64_t ylo = py[p] - radius_cm - g.y0, yhi = py[p] + radius_cm - g.y0;
    const int64_t xlo = px[p] - radius_cm - g.x0, xhi = px[p] + radius_cm - g.x0;
    if (yhi < 0 || xhi < 0) continue;
    const int64_t cy0 = std::max<int64_t>(ylo, 0) / g.cell, cx0 = std::max<int64_t>(xlo, 0) / g.cell;
    if (cy0 >= g.ny || cx0 >= g.nx) continue;
    const int64_t cy1 = std::min<int64_t>(yhi / g.cell, g.ny - 1), cx1 = std::min<int64_t>(xhi / g.cell, g.nx - 1);
    found.clear();
    for (int64_t cy = cy0; cy <= cy1; ++cy)
      for (int32_t e = g.start[cy * g.nx + cx0]; e < g.start[cy * g.nx + cx1 + 1]; ++e) {
        const int32_t v = g.items[e];
        const int64_t dy = g.qy[v] - py[p], dx = g.qx[v] - px[p];
        if (dy > radius_cm || dy < -radius_cm || dx > radius_cm || dx < -radius_cm) continue;
        const int64_t d2 = dy * dy + dx * dx;
        if (d2 <= r2) found.emplace_back(d2, v);
      }
    const size_t n = std::min(found.size(), (size_t)k);
    std::partial_sort(found.begin(), found.begin() + n, found.end());
    for (size_t j = 0; j < n; ++j) {
      cand[p * k + j] = found[j].second;
      cand_d2[p * k + j] = found[j].first;
    }
    n_cand[p] = (int32_t)n;
  }
}

// ---- edge-based matching (routing/mapmatch_edge.py holds the definition and the bound derivation) ----
constexpr int kMmFr = 16;
constexpr int64_t kMmOne = (int64_t)1 << kMmFr;
constexpr int64_t kMmMaxEdgeSpan = (int64_t)1 << 22;   // |w| per axis of a matchable edge
constexpr int64_t kMmMaxEdgeLc = (int64_t)1 << 40;     // centimetres of a matchable edge

struct MmEdge {
  int64_t ay, ax;    // the tail's quantized coordinates
  int32_t wy, wx;    // head - tail
  int64_t lc;        // centimetres
};

// d2 and fq of a fix on an edge; the caller keeps the fix within the radius of the edge's box, so
// |P - A| < 2^22 + 2^17 per axis and every product below stays under 2^62
inline void mm_edge_project(const MmEdge& e, int64_t py, int64_t px, int64_t* d2, int32_t* fq) {
  const int64_t dy = py - e.ay, dx = px - e.ax, wy = e.wy, wx = e.wx;
  const int64_t L2 = wy * wy + wx * wx;
  const int64_t f = std::min(std::max<int64_t>(dy * wy + dx * wx, 0), L2);
  const int64_t q = L2 > 0 ? (f << kMmFr) / L2 : 0;
  const int64_t ry = dy - ((wy * q + kMmOne / 2) >> kMmFr), rx = dx - ((wx * q + kMmOne / 2) >> kMmFr);
  *d2 = ry * ry + rx * rx;
  *fq = (int32_t)q;
}

// Bucket grid over the matchable edges: an edge is listed in every cell its closed bounding box
// touches.  The candidate set does not depend on the cell size, which the caller chooses (it is
// raised to keep at most 2048 cells per axis).
struct MmEdgeGrid {
  int64_t y0 = 0, x0 = 0, cell = 1;
  int ny = 0, nx = 0;
  std::vector<int32_t> start, items;   // CSR over row-major cells
  std::vector<MmEdge> edges;           // every edge; an unmatchable one is in no cell
  std::vector<uint8_t> ok;

  void build(const int64_t* qy, const int64_t* qx, size_t n, const int32_t* tail, const int32_t* head,
             const int64_t* lc, size_t E, int64_t cell_cm) {
    if (n == 0 || n >= ((size_t)1 << 30) || E >= ((size_t)1 << 30))
      throw std::invalid_argument("MmEdgeGrid: 1 .. 2^30 - 1 nodes, fewer than 2^30 edges");
    int64_t y1 = qy[0], x1 = qx[0];
    y0 = qy[0];
    x0 = qx[0];
    for (size_t i = 1; i < n; ++i) {
      y0 = std::min(y0, qy[i]);
      y1 = std::max(y1, qy[i]);
      x0 = std::min(x0, qx[i]);
      x1 = std::max(x1, qx[i]);
    }
    constexpr int64_t lim = (int64_t)1 << 40;
    if (y1 - y0 > lim || x1 - x0 > lim || y0 < -lim || x0 < -lim || y1 > lim || x1 > lim)
      throw std::invalid_argument("MmEdgeGrid: coordinates out of range");
    cell = std::max<int64_t>({cell_cm, 1, std::max(y1 - y0, x1 - x0) / 2048 + 1});
    ny = (int)((y1 - y0) / cell) + 1;
    nx = (int)((x1 - x0) / cell) + 1;
    edges.resize(E);
    ok.assign(E, 0);
    for (size_t e = 0; e < E; ++e) {
      if (tail[e] < 0 || (size_t)tail[e] >= n || head[e] < 0 || (size_t)head[e] >= n)
        throw std::invalid_argument("MmEdgeGrid: edge end out of range");
      const int64_t wy = qy[head[e]] - qy[tail[e]], wx = qx[head[e]] - qx[tail[e]];
      ok[e] = wy <= kMmMaxEdgeSpan && wy >= -kMmMaxEdgeSpan && wx <= kMmMaxEdgeSpan && wx >= -kMmMaxEdgeSpan &&
              lc[e] >= 0 && lc[e] <= kMmMaxEdgeLc;
      edges[e] = ok[e] ? MmEdge{qy[tail[e]], qx[tail[e]], (int32_t)wy, (int32_t)wx, lc[e]}
                       : MmEdge{qy[tail[e]], qx[tail[e]], 0, 0, 0};
    }
    start.assign((size_t)ny * nx + 1, 0);
    size_t total = 0;
    for_cells([&](size_t c, size_t) {
      ++start[c + 1];
      ++total;
    });
    if (total >= ((size_t)1 << 31)) throw std::invalid_argument("MmEdgeGrid: too many cell entries (cell too small)");
    for (size_t c = 0; c < (size_t)ny * nx; ++c) start[c + 1] += start[c];
    items.resize(total);
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for_cells([&](size_t c, size_t e) { items[at[c]++] = (int32_t)e; });
  }

  // fn(cell, edge) for every cell each matchable edge's box touches, edges ascending
  template <class F>
  void for_cells(F fn) const {
    for (size_t e = 0; e < edges.size(); ++e) {
      if (!ok[e]) continue;
      const MmEdge& g = edges[e];
      const int64_t cy0 = (g.ay + std::min<int64_t>(g.wy, 0) - y0) / cell, cy1 = (g.ay + std::max<int64_t>(g.wy, 0) - y0) / cell;
      const int64_t cx0 = (g.ax + std::min<int64_t>(g.wx, 0) - x0) / cell, cx1 = (g.ax + std::max<int64_t>(g.wx, 0) - x0) / cell;
      for (int64_t cy = cy0; cy <= cy1; ++cy)
        for (int64_t cx = cx0; cx <= cx1; ++cx) fn((size_t)(cy * nx + cx), e);
    }
  }
};

// cand_edge / cand_d2 / cand_fq [P, k] (-1 padded), n_cand [P]: per fix the k matchable edges within
// radius_cm with the smallest (d2, edge id)
inline void mm_edge_candidates(const MmEdgeGrid& g, const int64_t* py, const int64_t* px, size_t P, int64_t radius_cm,
                               int k, int32_t* cand_edge, int64_t* cand_d2, int32_t* cand_fq, int32_t* n_cand) {
  if (k < 1 || k > kMmMaxK) throw std::invalid_argument("mm_edge_candidates: k in 1..16");
  if (radius_cm < 1 || radius_cm > 100000)
    throw std::invalid_argument("mm_edge_candidates: radius in 1..100000 cm");
  const int64_t r2 = radius_cm * radius_cm;
  struct Hit {
    int64_t d2;
    int32_t e, fq;
    bool operator<(const Hit& o) const { return d2 != o.d2 ? d2 < o.d2 : e < o.e; }
    bool operator==(const Hit& o) const { return d2 == o.d2 && e == o.e; }
  };
  std::vector<Hit> found;
  for (size_t p = 0; p < P; ++p) {
    for (int j = 0; j < k; ++j) {
      cand_edge[p * k + j] = -1;
      cand_d2[p * k + j] = -1;
      cand_fq[p * k + j] = -1;
    }
    n_cand[p] = 0;
    constexpr int64_t lim = (int64_t)1 << 41;   // far beyond any quantized coordinate (|q| < 2^33)
    if (py[p] > lim || py[p] < -lim || px[p] > lim || px[p] < -lim)
      throw std::invalid_argument("mm_edge_candidates: fix coordinate out of range");
    const int64_t ylo = py[p] - radius_cm - g.y0, yhi = py[p] + radius_cm - g.y0;
    const int64_t xlo = px[p] - radius_cm - g.x0, xhi = px[p] + radius_cm - g.x0;
    if (yhi < 0 || xhi < 0) continue;
    const int64_t cy0 = std::max<int64_t>(ylo, 0) / g.cell, cx0 = std::max<int64_t>(xlo, 0) / g.cell;
    if (cy0 >= g.ny || cx0 >= g.nx) continue;
    const int64_t cy1 = std::min<int64_t>(yhi / g.cell, g.ny - 1), cx1 = std::min<int64_t>(xhi / g.cell, g.nx - 1);
    found.clear();
    for (int64_t cy = cy0; cy <= cy1; ++cy)
      for (int32_t i = g.start[cy * g.nx + cx0]; i < g.start[cy * g.nx + cx1 + 1]; ++i) {
        const int32_t e = g.items[i];
        const MmEdge& ed = g.edges[e];
        // the box test first: it bounds P - A for the products of the projection
        const int64_t by0 = ed.ay + std::min<int64_t>(ed.wy, 0), by1 = ed.ay + std::max<int64_t>(ed.wy, 0);
        const int64_t bx0 = ed.ax + std::min<int64_t>(ed.wx, 0), bx1 = ed.ax + std::max<int64_t>(ed.wx, 0);
        if (py[p] < by0 - radius_cm || py[p] > by1 + radius_cm || px[p] < bx0 - radius_cm || px[p] > bx1 + radius_cm)
          continue;
        int64_t d2;
        int32_t fq;
        mm_edge_project(ed, py[p], px[p], &d2, &fq);
        if (d2 <= r2) found.push_back(Hit{d2, e, fq});
      }
    std::sort(found.begin(), found.end());   // an edge listed in several cells was found several times
    found.erase(std::unique(found.begin(), found.end()), found.end());
    const size_t n = std::min(found.size(), (size_t)k);
    for (size_t j = 0; j < n; ++j) {
      cand_edge[p * k + j] = found[j].e;
      cand_d2[p * k + j] = found[j].d2;
      cand_fq[p * k + j] = found[j].fq;
    }
    n_cand[p] = (int32_t)n;
  }
}

// route_cm [rows, K, K] of the steps: met [rows, K, K] are the matrix rows' metres (heads of the
// previous fix's candidates x tails of this fix's; inf = no route), e1 / off1 / lc1 [rows, K] the
// previous fix's candidates (edge -1 = padding), e2 / off2 this fix's
inline void mm_edge_route_cm(const float* met, const int32_t* e1, const int64_t* off1, const int64_t* lc1,
                             const int32_t* e2, const int64_t* off2, size_t rows, int K, int64_t* out) {
  if (K < 1 || K > kMmMaxK) throw std::invalid_argument("mm_edge_route_cm: K in 1..16");
  for (size_t r = 0; r < rows; ++r)
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) {
        const size_t a = r * K + i, b = r * K + j, c = (r * K + i) * K + j;
        const float m = met[c];
        int64_t v = -1;
        if (e1[a] >= 0 && e2[b] >= 0) {
          if (e1[a] == e2[b] && off2[b] >= off1[a])
            v = off2[b] - off1[a];
          else if (std::isfinite(m) && m >= 0.0f)
            v = (lc1[a] - off1[a]) + (int64_t)std::llrint((double)m * 100.0) + off2[b];
        }
        out[c] = v;
      }
}

struct MmCosts {
  int64_t beta_cm, sigma_cm, max_detour_cm;
};

inline void mm_check_costs(const MmCosts& c) {
  if (c.beta_cm < 1 || c.beta_cm > 10000 || c.sigma_cm < 1 || c.sigma_cm > 20000 || c.max_detour_cm < 1 ||
      c.max_detour_cm > 500000)
    throw std::invalid_argument("map matching: beta 1..1e4, sigma 1..2e4, max_detour 1..5e5 cm");
}

// One trace: cand_d2 [T, K], n_cand [T] (clamped to 1..K), route_cm [T-1, K, K] (-1 infeasible),
// g [T-1]; the first n fixes are matched.  choice / seg [T] (-1 from n on); returns the sum of the
// segments' final scores.
inline int64_t mm_viterbi(const int64_t* cand_d2, const int32_t* n_cand, const int64_t* route_cm, const int64_t* g,
                          int T, int K, int n, const MmCosts& c, int32_t* choice, int32_t* seg, int32_t* nseg_out) {
  if (K < 1 || K > kMmMaxK || T < 1 || T > kMmMaxPoints) throw std::invalid_argument("mm_viterbi: K in 1..16, T in 1..2048");
  n = std::max(0, std::min(n, T));
  for (int t = 0; t < T; ++t) choice[t] = seg[t] = -1;
  *nseg_out = 0;
  if (n == 0) return 0;
  const int64_t two_s2 = 2 * c.sigma_cm * c.sigma_cm;
  std::vector<uint8_t> back((size_t)n * K, 0xFF), fin(n, 0xFF);
  int64_t score[kMmMaxK], next[kMmMaxK];
  auto nc = [&](int t) { return std::min(std::max((int)n_cand[t], 1), K); };
  auto start = [&](int t, int64_t* s) {
    for (int j = 0; j < K; ++j) s[j] = j < nc(t) ? c.beta_cm * cand_d2[(size_t)t * K + j] : kMmDead;
  };
  int64_t cost = 0;
  int nseg = 0;
  auto close = [&](int t_last, const int64_t* s) {
    int bj = 0;
    for (int j = 1; j < K; ++j)
      if (s[j] < s[bj]) bj = j;
    fin[t_last] = (uint8_t)bj;
    cost += s[bj];
    ++nseg;
  };
  start(0, score);
  seg[0] = 0;
  for (int t = 1; t < n; ++t) {
    const int np = nc(t - 1), ncur = nc(t);
    const int64_t gt = g[t - 1];
    bool any = false;
    for (int j = 0; j < K; ++j) {
      next[j] = kMmDead;
      if (j >= ncur) continue;
      int64_t best = kMmDead;
      int arg = -1;
      for (int i = 0; i < np; ++i) {
        const int64_t r = route_cm[((size_t)(t - 1) * K + i) * K + j];
        if (score[i] >= kMmDead || r < 0) continue;
        const int64_t dev = r > gt ? r - gt : gt - r;
        if (dev > c.max_detour_cm) continue;
        const int64_t v = score[i] + two_s2 * dev;
        if (v < best) {
          best = v;
          arg = i;
        }
      }
      if (arg >= 0) {
        next[j] = best + c.beta_cm * cand_d2[(size_t)t * K + j];
        back[(size_t)t * K + j] = (uint8_t)arg;
        any = true;
      }
    }
    if (!any) {   // a break: the segment ends at t - 1, a new one starts here
      close(t - 1, score);
      start(t, next);
    }
    seg[t] = nseg;
    std::copy(next, next + K, score);
  }
  close(n - 1, score);
  int cur = fin[n - 1];
  for (int t = n - 1; t >= 0; --t) {
    choice[t] = cur;
    const uint8_t b = back[(size_t)t * K + cur];
    if (b == 0xFF) {
      if (t > 0) cur = fin[t - 1];
    } else {
      cur = b;
    }
  }
  *nseg_out = nseg;
  return cost;
}

}  // namespace rtr
