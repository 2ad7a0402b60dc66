// Native route service, legs: every waypoint snapped, the flush's unique legs searched on the CCH
// (under each request's routing context) or by the batched A*, the found paths compacted on the GPU
// into one flat array before the copy-out, and the "alternatives" candidates chosen among them
// (see route_service.hip for the service, route_service_impl.h for its state).
#include <algorithm>
#include <cmath>
#include <queue>

#include "route_service_impl.h"
#include "runtime/alternatives.h"

namespace rt {

namespace {

// one block per found path: copy its nodes from the (Q, max_path) rows into the flat array
__global__ void compact_paths_kernel(const int* __restrict__ rows, int max_path, const int* __restrict__ len,
                                     const int* __restrict__ status, const long long* __restrict__ off, int Q,
                                     int* __restrict__ flat) {
  const int q = blockIdx.x;
  if (q >= Q || status[q] != 0) return;
  const int n = min(len[q], max_path);
  const long long o = off[q];
  for (int i = threadIdx.x; i < n; i += blockDim.x) flat[o + i] = rows[(size_t)q * max_path + i];
}

// Exact host search for the rare leg both GPU stages gave up on (graph.py _exact_fallback):
// Dijkstra from s stopping when t is settled.
bool host_dijkstra(const int* indptr, const int* indices, const float* cost, int N, int s, int t, int max_path,
                   float& out_cost, std::vector<int32_t>& path) {
  std::vector<double> dist((size_t)N, INFINITY);
  std::vector<int32_t> par((size_t)N, -1);
  using QE = std::pair<double, int>;
  std::priority_queue<QE, std::vector<QE>, std::greater<QE>> pq;
  dist[s] = 0.0;
  pq.push({0.0, s});
  while (!pq.empty()) {
    auto [d, v] = pq.top();
    pq.pop();
    if (d > dist[v]) continue;
    if (v == t) break;
    for (int e = indptr[v]; e < indptr[v + 1]; ++e) {
      const int w = indices[e];
      const double nd = d + (double)cost[e];
      if (nd < dist[w]) {
        dist[w] = nd;
        par[w] = v;
        pq.push({nd, w});
      }
    }
  }
  if (!std::isfinite(dist[t])) return false;
  path.clear();
  for (int v = t; v != -1; v = par[v]) {
    path.push_back(v);
    if ((int)path.size() > max_path) return false;
    if (v == s) break;
  }
  std::reverse(path.begin(), path.end());
  out_cost = (float)dist[t];
  return true;
}

}  // namespace

// every waypoint of the flush's routed jobs snapped to its road node (j->nodes, call by call)
std::vector<RouteJob*> RouteService::Impl::snap_jobs(Batch& b) {
  const double t0 = now_us();
  std::vector<RouteJob*> g;
  for (RouteJob* j : b.jobs)
    if (!j->fallback && !j->calls.empty()) g.push_back(j);
  rtc::parallel_chunks(g.size(), 64, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      RouteJob* j = g[i];
      j->nodes.clear();
      for (const auto& c : j->calls)
        for (const auto& pt : c) j->nodes.push_back(grid.nearest(pt.second, pt.first, cfg.snap_c));
    }
  });
  add_t(2, t0);
  return g;
}

// The found paths of the Q searched legs (lb.h_st / lb.h_len are on the host) compacted on the GPU
// into one flat array and copied out into b.flat; with `edges` their hops' road edges the same way
// into b.flat_e (maneuvers look them up instead of scanning adjacency).  lb.h_off[i] is where leg
// i's path starts.  The next flush reuses the pinned buffers.
bool RouteService::Impl::compact_out(Batch& b, int Q, bool edges, const char* what) {
  const int MP = cfg.max_path;
  long long total = 0;
  for (int i = 0; i < Q; ++i) {
    lb.h_off.h[i] = total;
    if (lb.h_st.h[i] == 0) total += std::min(lb.h_len.h[i], MP);
  }
  if (total == 0) return true;
  if (!lb.reserve_flat((size_t)total)) return false;
  hipError_t e = qcopy(lb.d_off.d, lb.h_off.h, (size_t)Q * 8, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(compact_paths_kernel, dim3(Q), dim3(256), 0, stream, lb.d_path.d, MP, lb.d_len.d, lb.d_st.d,
                       lb.d_off.d, Q, lb.d_flat.d);
    e = hipGetLastError();
  }
  if (edges) {
    if (e == hipSuccess && !lb.reserve_flat_e((size_t)total)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) {
      hipLaunchKernelGGL(compact_paths_kernel, dim3(Q), dim3(256), 0, stream, lb.d_edge.d, MP, lb.d_len.d, lb.d_st.d,
                         lb.d_off.d, Q, lb.d_flat_e.d);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = qcopy(lb.h_flat.h, lb.d_flat.d, (size_t)total * 4, stream);
  if (edges && e == hipSuccess) e = qcopy(lb.h_flat_e.h, lb.d_flat_e.d, (size_t)total * 4, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, what);
  if (e != hipSuccess) return false;
  b.flat.assign(lb.h_flat.h, lb.h_flat.h + total);
  if (edges) b.flat_e.assign(lb.h_flat_e.h, lb.h_flat_e.h + total);
  return true;
}

// CCH legs: every unique (context, s, t) leg of the flush, one route call per context group
// (sweep + meet + unpack launches), then the same path compaction / copy-out as the A* path
bool RouteService::Impl::search_legs_cch(Batch& b) {
  std::vector<rtr::Leg>& legs = b.legs;
  std::unordered_map<uint64_t, int>& leg_index = b.leg_index;
  const std::vector<RouteJob*> g = snap_jobs(b);
  double t0 = now_us();
  const int G = (int)b.metrics.size();
  std::vector<std::vector<std::pair<int, int>>> pairs(G);
  std::vector<int> order;                    // leg index -> (group, index in group) flattened
  // legs of a multi-stop job run between points of its group's matrix: their chains are reused
  // (meet + unpack only); every other leg (point-to-point jobs, alternatives' via legs) is routed
  std::vector<std::vector<std::array<int, 3>>> tri(G);      // (row, i, j) of each matrix-derived pair
  std::vector<std::vector<std::pair<int, int>>> rest(G);
  auto want = [&](int grp, int s, int t, int row, int i, int jj) {
    if (!leg_index.emplace(leg_key(grp, s, t), -1 - grp).second) return;
    if (row >= 0) {
      pairs[grp].emplace_back(s, t);
      tri[grp].push_back({row, i, jj});
    } else {
      rest[grp].emplace_back(s, t);
    }
  };
  for (RouteJob* j : g) {
    int row = -1;
    if (mtag != 0 && !j->plan.trips.empty()) {
      auto it = jrow.find(j);
      if (it != jrow.end()) row = it->second;
    }
    size_t off = 0;
    for (size_t ci = 0; ci < j->calls.size(); ++ci) {
      const auto& c = j->calls[ci];
      // call ci of a multi-stop job is trip ci: its points are the trip's point indices
      const bool from_trip = row >= 0 && ci < j->plan.trips.size() && j->plan.trips[ci].size() == c.size();
      for (size_t i = 0; i + 1 < c.size(); ++i)
        want(j->group, j->nodes[off + i], j->nodes[off + i + 1], from_trip ? row : -1,
             from_trip ? j->plan.trips[ci][i] : 0, from_trip ? j->plan.trips[ci][i + 1] : 0);
      off += c.size();
    }
  }
  // "alternatives": every unique leg (in order) gets its via nodes; s->w and w->t join the batch
  std::vector<RouteJob*> alt_jobs;
  for (RouteJob* j : g)
    if (j->req.alt_k > 0) alt_jobs.push_back(j);
  rtc::parallel_chunks(alt_jobs.size(), 1, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      RouteJob* j = alt_jobs[i];
      j->alt_pairs.clear();
      std::unordered_map<uint64_t, int> seen;
      size_t off = 0;
      for (const auto& c : j->calls) {
        for (size_t k = 0; k + 1 < c.size(); ++k) {
          const int s = j->nodes[off + k], t = j->nodes[off + k + 1];
          if (seen.emplace(((uint64_t)(uint32_t)s << 32) | (uint32_t)t, 0).second) j->alt_pairs.emplace_back(s, t);
        }
        off += c.size();
      }
      j->alt_vias.assign(j->alt_pairs.size(), {});
      for (size_t k = 0; k < j->alt_pairs.size(); ++k)
        j->alt_vias[k] = ralt::via_nodes(cfg.glat, cfg.glon, cfg.N, j->alt_pairs[k].first, j->alt_pairs[k].second,
                                         j->req.alt_k - 1);
    }
  });
  for (RouteJob* j : alt_jobs)
    for (size_t k = 0; k < j->alt_pairs.size(); ++k)
      for (int w : j->alt_vias[k]) {
        want(j->group, j->alt_pairs[k].first, w, -1, 0, 0);
        want(j->group, w, j->alt_pairs[k].second, -1, 0, 0);
      }
  // leg order: every group's matrix-derived legs (group order), then every other leg (group order)
  int QA = 0, QR = 0;
  for (int gi = 0; gi < G; ++gi) {
    QA += (int)pairs[gi].size();
    QR += (int)rest[gi].size();
  }
  const int Q = QA + QR;
  {
    int a = 0, r = QA;
    for (int gi = 0; gi < G; ++gi) {
      for (const auto& pr : pairs[gi]) leg_index[leg_key(gi, pr.first, pr.second)] = a++;
      for (const auto& pr : rest[gi]) leg_index[leg_key(gi, pr.first, pr.second)] = r++;
    }
  }
  legs.assign(Q, rtr::Leg());
  if (Q == 0) return true;
  n_legs.fetch_add(Q, std::memory_order_relaxed);
  const int MP = cfg.max_path;
  if (!lb.reserve((size_t)Q, (size_t)QA, (size_t)MP, true)) return false;
  {
    int a = 0, r = QA;
    for (int gi = 0; gi < G; ++gi) {
      for (size_t k = 0; k < pairs[gi].size(); ++k, ++a) {
        lb.h_src.h[a] = pairs[gi][k].first;
        lb.h_dst.h[a] = pairs[gi][k].second;
        lb.h_lgrp.h[a] = gi;
        lb.h_lr.h[a] = tri[gi][k][0];
        lb.h_li.h[a] = tri[gi][k][1];
        lb.h_lj.h[a] = tri[gi][k][2];
      }
      for (const auto& pr : rest[gi]) {
        lb.h_src.h[r] = pr.first;
        lb.h_dst.h[r] = pr.second;
        lb.h_lgrp.h[r] = gi;
        ++r;
      }
    }
  }
  hipError_t e = qcopy(lb.d_src.d, lb.h_src.h, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.d_dst.d, lb.h_dst.h, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.d_lgrp.d, lb.h_lgrp.h, (size_t)Q * 4, stream);
  if (QA > 0) {
    if (e == hipSuccess) e = qcopy(lb.d_lr.d, lb.h_lr.h, (size_t)QA * 4, stream);
    if (e == hipSuccess) e = qcopy(lb.d_li.d, lb.h_li.h, (size_t)QA * 4, stream);
    if (e == hipSuccess) e = qcopy(lb.d_lj.d, lb.h_lj.h, (size_t)QA * 4, stream);
  }
  auto out_at = [&](int q) {
    CchRouteOut o;
    o.sec = lb.d_cost.d + q;
    o.metres = lb.d_met.d + q;
    o.status = lb.d_st.d + q;
    o.len = lb.d_len.d + q;
    o.path = lb.d_path.d + (size_t)q * MP;
    o.edges = lb.d_edge.d + (size_t)q * MP;
    o.max_path = MP;
    return o;
  };
  if (e == hipSuccess && QA > 0)
    e = cfg.cch->legs_from_matrix_multi(cb.d_mv.d, lb.d_lgrp.d, lb.d_src.d, lb.d_lr.d, lb.d_li.d, lb.d_lj.d, QA, mtag, out_at(0), msc,
                                        stream);
  if (e == hipSuccess && QR > 0)
    e = cfg.cch->route_multi(cb.d_mv.d, lb.d_lgrp.d + QA, lb.d_src.d + QA, lb.d_dst.d + QA, QR, out_at(QA), csc, stream);
  n_legs_reused.fetch_add(QA, std::memory_order_relaxed);
  if (e == hipSuccess) e = qcopy(lb.h_st.h, lb.d_st.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.h_len.h, lb.d_len.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.h_cost.h, lb.d_cost.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.h_met.h, lb.d_met.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, "cch-legs");
  add_t(3, t0);
  t0 = now_us();
  if (e != hipSuccess) return false;
  if (!compact_out(b, Q, true, "cch-paths")) return false;
  add_t(4, t0);
  // legs the GPU could not return (status 4: longer than max_path / unpack stack): exact on the host
  int nbad = 0;
  for (int i = 0; i < Q; ++i) nbad += lb.h_st.h[i] == 4;
  b.host_paths.resize(Q);
  for (int i = 0; i < Q; ++i) {
      const int gi = lb.h_lgrp.h[i];
      rtr::Leg& L = legs[i];
      if (lb.h_st.h[i] == 0) {
        L.sec = lb.h_cost.h[i];
        L.metres = lb.h_met.h[i];
        L.len = std::min(lb.h_len.h[i], MP);
        L.path = b.flat.data() + lb.h_off.h[i];
        L.edges = b.flat_e.data() + lb.h_off.h[i];
      } else if (lb.h_st.h[i] == 4 && nbad <= 1024 && cfg.h_indptr != nullptr) {
        const std::vector<float>& hc = *b.host_cost[gi];
        float c;
        if (host_dijkstra(cfg.h_indptr, cfg.h_indices, hc.data(), cfg.N, lb.h_src.h[i], lb.h_dst.h[i], 1 << 22, c,
                          b.host_paths[i])) {
          L.sec = c;
          float met = 0.f;
          const auto& p = b.host_paths[i];
          for (size_t k = 0; k + 1 < p.size(); ++k) {
            int32_t best = -1;
            for (int32_t ee = cfg.h_indptr[p[k]]; ee < cfg.h_indptr[p[k] + 1]; ++ee)
              if (cfg.h_indices[ee] == p[k + 1] && (best < 0 || hc[ee] < hc[best])) best = ee;
            if (best >= 0) met += cfg.h_length[best];
          }
          L.metres = met;
          L.len = (int)p.size();
          L.path = p.data();
          n_host_legs.fetch_add(1, std::memory_order_relaxed);
        }
      }
    }
  return true;
}

// graph provider: snap, search every unique leg of the flush once, fill the batch's legs
bool RouteService::Impl::search_legs(Batch& b) {
  std::vector<rtr::Leg>& legs = b.legs;
  std::vector<std::vector<int32_t>>& host_paths = b.host_paths;
  std::unordered_map<uint64_t, int>& leg_index = b.leg_index;
  const std::vector<RouteJob*> g = snap_jobs(b);
  double t0 = now_us();
  std::vector<std::pair<int, int>> pairs;
  for (RouteJob* j : g) {
    size_t off = 0;
    for (const auto& c : j->calls) {
      for (size_t i = 0; i + 1 < c.size(); ++i) {
        const uint64_t key = ((uint64_t)(uint32_t)j->nodes[off + i] << 32) | (uint32_t)j->nodes[off + i + 1];
        if (leg_index.emplace(key, (int)pairs.size()).second) pairs.emplace_back(j->nodes[off + i], j->nodes[off + i + 1]);
      }
      off += c.size();
    }
  }
  const int Q = (int)pairs.size();
  legs.assign(Q, rtr::Leg());
  if (Q == 0) return true;
  n_legs.fetch_add(Q, std::memory_order_relaxed);
  const int MP = cfg.max_path;
  if (!lb.reserve((size_t)Q, 0, (size_t)MP, false)) return false;
  for (int i = 0; i < Q; ++i) {
    lb.h_src.h[i] = pairs[i].first;
    lb.h_dst.h[i] = pairs[i].second;
  }
  hipError_t e = qcopy(lb.d_src.d, lb.h_src.h, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.d_dst.d, lb.h_dst.h, (size_t)Q * 4, stream);
  // the tiered search (csrc/astar.hip): interactive flushes (few thousand legs) skip the lane tier
  // (routing/graph.py BatchedAstar.run calls the same function)
  AstarGraphDev gd;
  gd.indptr = cfg.indptr;
  gd.indices = cfg.indices;
  gd.cost = cfg.cost;
  gd.lat = cfg.lat32;
  gd.lon = cfg.lon32;
  gd.N = cfg.N;
  gd.inv_vmax = cfg.inv_vmax;
  gd.lm = cfg.lm;
  gd.K = cfg.K;
  AstarOut ao;
  ao.cost = lb.d_cost.d;
  ao.len = lb.d_len.d;
  ao.status = lb.d_st.d;
  ao.path = lb.d_path.d;
  ao.max_path = MP;
  ao.iters = lb.d_iters.d;
  AstarPlan pl;
  pl.max_iters = cfg.max_iters;
  pl.lane_pops = cfg.lane_pops;
  pl.wave_only_below = cfg.wave_only_below;
  pl.delta = cfg.wave_delta;
  pl.lane_max_m = cfg.lane_max_m;
  AstarRunStats rs;
  if (e == hipSuccess)
    e = astar_search(gd, lb.d_src.d, lb.d_dst.d, Q, cfg.lane_ws.slots > 0 ? &cfg.lane_ws : nullptr,
                     cfg.wave_ws.slots > 0 ? &cfg.wave_ws : nullptr, cfg.big_ws.slots > 0 ? &cfg.big_ws : nullptr,
                     ao, pl, lb.d_qidx.d, stream, &rs, cfg.arena.base ? &cfg.arena : nullptr);
  n_escalated.fetch_add(rs.escalated, std::memory_order_relaxed);
  if (e == hipSuccess) e = qcopy(lb.h_st.h, lb.d_st.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, "astar");
  add_t(3, t0);
  t0 = now_us();
  if (e == hipSuccess) e = qcopy(lb.h_len.h, lb.d_len.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = qcopy(lb.h_cost.h, lb.d_cost.d, (size_t)Q * 4, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, "astar-escalate");
  if (e != hipSuccess) return false;
  if (!compact_out(b, Q, false, "astar-paths")) return false;
  add_t(4, t0);
  // searches both GPU stages gave up on (status 2 / 3): exact on the host, like graph.py
  int nbad = 0;
  for (int i = 0; i < Q; ++i) nbad += (lb.h_st.h[i] == 2 || lb.h_st.h[i] == 3);
  host_paths.resize(Q);
  for (int i = 0; i < Q; ++i) {
    rtr::Leg& L = legs[i];
    if (lb.h_st.h[i] == 0) {
      L.sec = lb.h_cost.h[i];
      L.len = std::min(lb.h_len.h[i], MP);
      L.path = b.flat.data() + lb.h_off.h[i];
    } else if ((lb.h_st.h[i] == 2 || lb.h_st.h[i] == 3) && nbad <= 1024 && cfg.h_indptr != nullptr) {
      float c;
      if (host_dijkstra(cfg.h_indptr, cfg.h_indices, cfg.h_cost, cfg.N, pairs[i].first, pairs[i].second, MP, c,
                        host_paths[i])) {
        L.sec = c;
        L.len = (int)host_paths[i].size();
        L.path = host_paths[i].data();
        n_host_legs.fetch_add(1, std::memory_order_relaxed);
      }
    }
  }
  return true;
}

// "alternatives": per unique leg, the candidates (time-shortest path, then s->w->t per via node
// when both parts were found), the scorer's values, the pick, and the response block — exactly
// routing/alternatives.py AlternativeLegs.choose + optimize_with_alternatives
void RouteService::Impl::choose_alternatives(Batch& b, RouteJob* j) {
  const std::vector<rtr::Leg>& legs = b.legs;
  const double* delay = b.alt_delay->data();
  const size_t P = j->alt_pairs.size();
  struct Cand {
    double sec, met;
    const int32_t* p1;
    int n1;
    const int32_t* p2;   // second part (from its node 1 on), or nullptr
    int n2;
    const int32_t* e1;   // hop edges of the parts (nullptr: unknown, looked up on the host)
    const int32_t* e2;
  };
  auto leg = [&](int s, int t) -> const rtr::Leg* {
    auto it = b.leg_index.find(leg_key(j->group, s, t));
    return it == b.leg_index.end() || it->second < 0 ? nullptr : &legs[it->second];
  };
  std::vector<std::vector<Cand>> cands(P);
  size_t total = 0;
  for (size_t k = 0; k < P; ++k) {
    const int s = j->alt_pairs[k].first, t = j->alt_pairs[k].second;
    const rtr::Leg* d = leg(s, t);
    if (d && d->len > 0) cands[k].push_back({d->sec, d->metres, d->path, d->len, nullptr, 0, d->edges, nullptr});
    for (int w : j->alt_vias[k]) {
      const rtr::Leg* a = leg(s, w);
      const rtr::Leg* c = leg(w, t);
      if (a && c && a->len > 0 && c->len > 0)
        cands[k].push_back({a->sec + c->sec, a->metres + c->metres, a->path, a->len, c->path + 1, c->len - 1,
                            a->edges, c->edges});
    }
    total += cands[k].size();
  }
  (void)total;
  j->alt_legs.assign(P, rtr::Leg());
  j->alt_paths.assign(P, {});
  j->alt_edges.assign(P, {});
  std::string o = ",\"alternatives\":{\"k\":";
  rtr::put_int(o, j->req.alt_k);
  o += ",\"scorer\":";
  rtr::put_str(o, b.alt_engine);
  o += ",\"legs\":[";
  std::vector<int32_t> tmp;
  for (size_t k = 0; k < P; ++k) {
    if (k) o += ',';
    o += "{\"from_node\":";
    rtr::put_int(o, j->alt_pairs[k].first);
    o += ",\"to_node\":";
    rtr::put_int(o, j->alt_pairs[k].second);
    o += ",\"candidates\":";
    rtr::put_int(o, (long long)cands[k].size());
    if (cands[k].empty()) {
      o += '}';
      continue;       // Leg stays "not found": the assembly reports it like a plain request
    }
    std::vector<double> sc(cands[k].size());
    for (size_t c = 0; c < cands[k].size(); ++c) {
      const Cand& x = cands[k][c];
      tmp.assign(x.p1, x.p1 + x.n1);
      if (x.p2) tmp.insert(tmp.end(), x.p2, x.p2 + x.n2);
      sc[c] = ralt::candidate_score(cfg.glat, cfg.glon, delay, tmp.data(), tmp.size(), x.sec, b.alt_kind);
    }
    const int best = ralt::argmin_score(sc);
    const Cand& x = cands[k][best];
    std::vector<int32_t>& own = j->alt_paths[k];
    own.assign(x.p1, x.p1 + x.n1);
    if (x.p2) own.insert(own.end(), x.p2, x.p2 + x.n2);
    rtr::Leg& L = j->alt_legs[k];
    L.sec = x.sec;
    L.metres = x.met;
    L.path = own.data();
    L.len = (int)own.size();
    if (x.e1 && (x.p2 == nullptr || x.e2)) {
      std::vector<int32_t>& oe = j->alt_edges[k];
      oe.assign(x.e1, x.e1 + (x.n1 - 1));
      if (x.p2) oe.insert(oe.end(), x.e2, x.e2 + x.n2);     // the second part's hops: n2 of them
      L.edges = oe.data();
    }
    o += ",\"chosen\":";
    rtr::put_int(o, best);
    o += ",\"scores\":[";
    for (size_t c = 0; c < sc.size(); ++c) {
      if (c) o += ',';
      rtr::put_float(o, sc[c]);
    }
    o += "],\"seconds\":[";
    for (size_t c = 0; c < cands[k].size(); ++c) {
      if (c) o += ',';
      rtr::put_float(o, cands[k][c].sec);
    }
    o += "]}";
  }
  o += "]}";
  j->alt_json = std::move(o);
}

}  // namespace rt
