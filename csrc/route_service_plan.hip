// Native route service, trip planning: the flush's routing contexts (CCH) and its multi-stop
// requests' trips — ONE K5 + ONE K6 launch over coordinates, or the CCH's road matrices + K6
// (see route_service.hip for the service, route_service_impl.h for its state).  When a request of
// the flush asks for "improve", K6b (route_improve.hip) re-sequences the asking rows' trips right
// after K6, on the same buffers; for "exchange" K6c (route_exchange.hip) and a second K6b follow
// over the asking rows.  A flush nobody asks in launches nothing more.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "route_service_impl.h"

namespace rt {

// edge costs of a metric on the host (maneuver durations, exact host fallback): the copy the
// customization left with the metric (shares its lifetime), else copied once here
std::shared_ptr<const std::vector<float>> RouteService::Impl::host_costs(const std::shared_ptr<CchMetricDev>& m) {
  if (m->host_cost.size() == (size_t)cfg.cch->topo().E) return {m, &m->host_cost};
  {
    std::lock_guard<std::mutex> lk(hc_mu);
    auto it = hc_index.find(m->key);
    if (it != hc_index.end()) {
      hc_lru.splice(hc_lru.begin(), hc_lru, it->second);     // most recently used
      return it->second->second;
    }
  }
  auto v = std::make_shared<std::vector<float>>((size_t)cfg.cch->topo().E);
  // (through the pinned staging buffer: the copy kernel writes device-visible host memory only)
  if (cb.h_hcost.need(v->size()) != hipSuccess || qcopy(cb.h_hcost.h, m->cost, v->size() * 4, stream) != hipSuccess ||
      sync(stream, ev_gpu, "host-costs") != hipSuccess)
    return nullptr;
  std::memcpy(v->data(), cb.h_hcost.h, v->size() * 4);
  std::lock_guard<std::mutex> lk(hc_mu);
  if (hc_index.count(m->key)) return v;
  hc_lru.emplace_front(m->key, v);
  hc_index[m->key] = hc_lru.begin();
  while (hc_lru.size() > HC_MAX) {                            // evict the least recently used
    hc_index.erase(hc_lru.back().first);
    hc_lru.pop_back();
  }
  return v;
}

// CCH: group the flush's jobs by routing context and get each metric.  A context that is not
// customized yet does not stall the flush: its jobs leave the batch and wait for the router's
// background build (on_built requeues them), the other groups proceed now.  Contexts of requests
// routed at "now" are prefetched for the next week-hour shortly before the hour turns.
bool RouteService::Impl::cch_groups(Batch& b) {
  if (cfg.cch != nullptr) cfg.cch->note_queries();     // background builds now run paced
  const rtc::Stamp now = local_now(clock_skew_s);
  const int64_t days = (int64_t)std::floor((double)now.secs / 86400.0);
  const int64_t sec_of_day = now.secs - days * 86400;
  const int now_wh = (int)(((days + 3) % 7 + 7) % 7) * 24 + (int)(sec_of_day / 3600);
  const double t_now = now_us();
  std::unordered_map<uint64_t, int> gidx;
  std::vector<CchContext> ctxs;
  std::vector<char> sync;
  for (RouteJob* j : b.jobs) {
    if (j->fallback || !j->req.error.empty()) continue;
    CchContext c;
    uint64_t key = cfg.cch_fixed_key;
    if (cfg.cch_contexts) {
      c.weather = j->req.route_weather;
      c.congestion = j->req.route_congestion;
      c.weekhour = j->req.route_weekhour >= 0 ? j->req.route_weekhour : now_wh;
      key = c.key();
      if (j->req.route_weekhour < 0) seen_now[(c.weather & 0xFF) | (c.congestion << 8)] = t_now;
    }
    auto it = gidx.find(key);
    if (it == gidx.end()) {
      it = gidx.emplace(key, (int)ctxs.size()).first;
      ctxs.push_back(c);
      sync.push_back(0);
    }
    j->group = it->second;
    if (j->sync_ctx) sync[j->group] = 1;
  }
  // which groups are ready now
  std::vector<std::shared_ptr<CchMetricDev>> met(ctxs.size());
  std::vector<char> ready(ctxs.size(), 1);
  for (size_t g = 0; g < ctxs.size(); ++g) {
    if (!cfg.cch_contexts) {
      if (!cfg.cch->cached_metric(cfg.cch_fixed_key, met[g])) return false;
    } else if (async_ctx && !sync[g]) {
      ready[g] = cfg.cch->cached_metric(ctxs[g].key(), met[g]) ? 1 : 0;
    } else {
      const double t0 = now_us();
      bool fresh = false;
      if (cfg.cch->metric_for(ctxs[g], stream, met[g], &fresh) != hipSuccess) return false;
      if (fresh) {
        n_ctx_built.fetch_add(1, std::memory_order_relaxed);
        t_ctx_us.fetch_add((long long)(now_us() - t0), std::memory_order_relaxed);
      }
    }
  }
  // defer the jobs of groups still building; compact the ready groups
  std::vector<int> remap(ctxs.size(), -1);
  for (size_t g = 0; g < ctxs.size(); ++g)
    if (ready[g]) {
      remap[g] = (int)b.metrics.size();
      b.metrics.push_back(met[g]);
    }
  std::vector<CchContext> to_build;
  if (b.metrics.size() < ctxs.size()) {
    std::vector<RouteJob*> keep;
    keep.reserve(b.jobs.size());
    {
      std::lock_guard<std::mutex> lk(wmu);
      for (RouteJob* j : b.jobs) {
        if (j->fallback || !j->req.error.empty() || ready[j->group]) {
          keep.push_back(j);
          continue;
        }
        if (j->defer_t0 == 0.0) {
          j->defer_t0 = t_now;
          n_deferred.fetch_add(1, std::memory_order_relaxed);
        }
        waiting[ctxs[j->group].key()].push_back(j);
      }
    }
    b.jobs.swap(keep);
    for (size_t g = 0; g < ctxs.size(); ++g)
      if (!ready[g]) to_build.push_back(ctxs[g]);
  }
  for (RouteJob* j : b.jobs) {
    if (j->fallback || !j->req.error.empty()) continue;
    j->group = remap[j->group];
    if (j->defer_t0 > 0.0) {
      t_wait_us.fetch_add((long long)(t_now - j->defer_t0), std::memory_order_relaxed);
      j->defer_t0 = -1.0;                      // counted once
    }
  }
  // (no lock held: a context finished meanwhile notifies on this thread)
  for (const CchContext& c : to_build) cfg.cch->request_build(c, true);
  // the next week-hour of the contexts seen at "now" during the last hour, before it begins
  const int min_in_hour = (int)((sec_of_day % 3600) / 60);
  const int next_wh = (now_wh + 1) % 168;
  if (cfg.cch_contexts && async_ctx && prefetch_min > 0 && min_in_hour >= 60 - prefetch_min) {
    if (prefetched_wh != next_wh) {
      prefetched_wh = next_wh;
      prefetched.clear();
    }
    for (auto it = seen_now.begin(); it != seen_now.end();) {
      if (t_now - it->second > 3600e6) { it = seen_now.erase(it); continue; }
      if (!prefetched.insert(it->first).second) { ++it; continue; }     // queued for next_wh already
      CchContext c;
      c.weather = it->first & 0xFF;
      c.congestion = it->first >> 8;
      c.weekhour = next_wh;
      cfg.cch->request_build(c, false);
      n_prefetch.fetch_add(1, std::memory_order_relaxed);
      ++it;
    }
  }
  b.host_cost.assign(b.metrics.size(), nullptr);
  for (size_t g = 0; g < b.metrics.size(); ++g) {
    b.host_cost[g] = host_costs(b.metrics[g]);
    if (!b.host_cost[g]) return false;
  }
  // the flush's metrics as device views for the multi-context launches (b.metrics keeps them alive
  // until the flush is done)
  const size_t G = b.metrics.size();
  if (G > 0) {
    if (!cb.reserve(G)) return false;
    for (size_t g = 0; g < G; ++g) cb.h_mv.h[g] = CchGpu::view(*b.metrics[g]);
    if (qcopy(cb.d_mv.d, cb.h_mv.h, G * sizeof(CchMView), stream) != hipSuccess) return false;
  }
  return true;
}

bool RouteService::Impl::plan_multi(std::vector<RouteJob*>& jobs) {
  std::vector<RouteJob*> m;
  for (RouteJob* j : jobs)
    if (!j->fallback && j->req.error.empty() && j->req.dst.size() > 1) m.push_back(j);
  if (m.empty()) return true;
  const int R = (int)m.size();
  int NM = 1;
  for (RouteJob* j : m) NM = std::max(NM, (int)j->req.dst.size() + 1);
  if (NM > 4096) {   // beyond the greedy kernel's LDS scan: CPU greedy for those (never in the UI)
    for (RouteJob* j : m) j->fallback = true;
    return true;
  }
  const size_t RN = (size_t)R * NM;
  if (!tb.reserve((size_t)R, (size_t)NM, false)) return false;
  for (int k = 0; k < R; ++k) {
    const rtr::RouteReq& r = m[k]->req;
    const int n = (int)r.dst.size() + 1;
    double* la = tb.h_lat.h + (size_t)k * NM;
    double* lo = tb.h_lon.h + (size_t)k * NM;
    double* de = tb.h_dem.h + (size_t)k * NM;
    std::fill(la, la + NM, 0.0);
    std::fill(lo, lo + NM, 0.0);
    std::fill(de, de + NM, 0.0);
    la[0] = r.src.lat;
    lo[0] = r.src.lon;
    for (int i = 1; i < n; ++i) {
      la[i] = r.dst[i - 1].lat;
      lo[i] = r.dst[i - 1].lon;
      de[i] = r.dst[i - 1].demand;
    }
    tb.h_npts.h[k] = n;
    tb.h_cap.h[k] = r.cap;
    tb.h_maxd.h[k] = r.maxd;
    tb.imp.h_flag.h[k] = r.improve || r.exchange ? 1 : 0;
    tb.imp.h_xflag.h[k] = r.exchange ? 1 : 0;
  }
  const bool any_imp = std::any_of(m.begin(), m.end(), [](const RouteJob* j) { return j->req.improve || j->req.exchange; });
  hipError_t e = hipSuccess;
  cp(e, tb.d_lat.d, tb.h_lat.h, RN * 8);
  cp(e, tb.d_lon.d, tb.h_lon.h, RN * 8);
  cp(e, tb.d_dem.d, tb.h_dem.h, RN * 8);
  cp(e, tb.d_npts.d, tb.h_npts.h, (size_t)R * 4);
  cp(e, tb.d_cap.d, tb.h_cap.h, (size_t)R * 8);
  cp(e, tb.d_maxd.d, tb.h_maxd.h, (size_t)R * 8);
  if (e == hipSuccess) e = launch_haversine_matrix(tb.d_lat.d, tb.d_lon.d, tb.d_npts.d, R, NM, cfg.circuity, tb.d_D.d, stream);
  if (e == hipSuccess)
    e = launch_greedy_cvrp(tb.d_D.d, tb.d_npts.d, tb.d_dem.d, tb.d_cap.d, tb.d_maxd.d, R, NM, tb.d_visit.d, tb.d_trip.d, tb.d_ntrips.d,
                           tb.d_status.d, stream);
  if (e == hipSuccess) e = improve_rows(any_imp, tb.d_npts.d, R, NM);
  cp(e, tb.h_visit.h, tb.d_visit.d, RN * 4);
  cp(e, tb.h_trip.h, tb.d_trip.d, RN * 4);
  cp(e, tb.h_ntrips.h, tb.d_ntrips.d, (size_t)R * 4);
  cp(e, tb.h_status.h, tb.d_status.d, (size_t)R * 4);
  // the depot row of every D (the infeasible-stop order key) — the matrices stay on the GPU
  if (e == hipSuccess)
    e = qcopy2d(tb.h_row0.h, (size_t)NM * 8, tb.d_D.d, (size_t)NM * NM * 8, (size_t)NM * 8, (size_t)R, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, "k5k6-matrix");
  if (e != hipSuccess) return false;
  for (int k = 0; k < R; ++k) unpack_plan(m[k], tb.h_npts.h[k], NM, k, any_imp);
  return true;
}

// CCH: road-metre matrices of every multi-stop job, then the greedy (K6) over them — the same
// kernel as the haversine path, on road distances.  The jobs of all context groups are ONE set of
// rows (grouped, a common row width) with each row's group: one upload, one matrix launch sequence
// over every row (the sweep / meet kernels read the row's metric from the flush's views), one
// greedy launch, one read-back and one wait — a flush spread over 64 routing contexts costs what
// a single-context flush of the same size costs.
bool RouteService::Impl::plan_multi_road(Batch& b) {
  jrow.clear();
  mtag = 0;
  const int G = (int)b.metrics.size();
  std::vector<std::vector<RouteJob*>> byg(G);
  int NM = 1;
  for (RouteJob* j : b.jobs)
    if (!j->fallback && j->req.error.empty() && j->req.dst.size() > 1 && j->group >= 0 && j->group < G) {
      if ((int)j->req.dst.size() + 1 > 4096) {
        j->fallback = true;
        continue;
      }
      byg[j->group].push_back(j);
      NM = std::max(NM, (int)j->req.dst.size() + 1);
    }
  std::vector<RouteJob*> m;                  // all rows, grouped
  std::vector<int> r0(G + 1, 0);
  for (int g = 0; g < G; ++g) {
    r0[g] = (int)m.size();
    m.insert(m.end(), byg[g].begin(), byg[g].end());
  }
  r0[G] = (int)m.size();
  if (m.empty()) return true;
  const int R = (int)m.size();
  const size_t RN = (size_t)R * NM;
  if (!tb.reserve((size_t)R, (size_t)NM, true)) return false;
  for (int g = 0; g < G; ++g)
    for (int k = r0[g]; k < r0[g + 1]; ++k) tb.h_rowg.h[k] = g;
  rtc::parallel_chunks((size_t)R, 64, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const rtr::RouteReq& r = m[k]->req;
      const int n = (int)r.dst.size() + 1;
      int* pt = tb.h_pts.h + k * NM;
      double* de = tb.h_dem.h + k * NM;
      std::fill(pt, pt + NM, 0);
      std::fill(de, de + NM, 0.0);
      pt[0] = grid.nearest(r.src.lat, r.src.lon, cfg.snap_c);
      for (int i = 1; i < n; ++i) {
        pt[i] = grid.nearest(r.dst[i - 1].lat, r.dst[i - 1].lon, cfg.snap_c);
        de[i] = r.dst[i - 1].demand;
      }
      tb.h_npts2.h[k] = n;
      tb.h_cap.h[k] = r.cap;
      tb.h_maxd.h[k] = r.maxd;
      tb.imp.h_flag.h[k] = r.improve || r.exchange ? 1 : 0;
    tb.imp.h_xflag.h[k] = r.exchange ? 1 : 0;
    }
  });
  const bool any_imp = std::any_of(m.begin(), m.end(), [](const RouteJob* j) { return j->req.improve || j->req.exchange; });
  hipError_t e = hipSuccess;
  cp(e, tb.d_pts.d, tb.h_pts.h, RN * 4);
  cp(e, tb.d_npts2.d, tb.h_npts2.h, (size_t)R * 4);
  cp(e, tb.d_dem.d, tb.h_dem.h, RN * 8);
  cp(e, tb.d_cap.d, tb.h_cap.h, (size_t)R * 8);
  cp(e, tb.d_maxd.d, tb.h_maxd.h, (size_t)R * 8);
  cp(e, tb.d_rowg.d, tb.h_rowg.h, (size_t)R * 4);
  if (e == hipSuccess)
    e = cfg.cch->matrix_multi(cb.d_mv.d, tb.d_rowg.d, tb.d_pts.d, tb.d_npts2.d, R, NM, tb.d_msec.d, tb.d_mmet.d, tb.d_D.d, msc, stream);
  mtag = e == hipSuccess ? msc.chain_tag : 0;
  for (int k = 0; k < R; ++k) jrow[m[k]] = k;
  if (e == hipSuccess)
    e = launch_greedy_cvrp(tb.d_D.d, tb.d_npts2.d, tb.d_dem.d, tb.d_cap.d, tb.d_maxd.d, R, NM, tb.d_visit.d, tb.d_trip.d, tb.d_ntrips.d,
                           tb.d_status.d, stream);
  if (e == hipSuccess) e = improve_rows(any_imp, tb.d_npts2.d, R, NM);
  cp(e, tb.h_visit.h, tb.d_visit.d, RN * 4);
  cp(e, tb.h_trip.h, tb.d_trip.d, RN * 4);
  cp(e, tb.h_ntrips.h, tb.d_ntrips.d, (size_t)R * 4);
  cp(e, tb.h_status.h, tb.d_status.d, (size_t)R * 4);
  if (e == hipSuccess)
    e = qcopy2d(tb.h_row0.h, (size_t)NM * 8, tb.d_D.d, (size_t)NM * NM * 8, (size_t)NM * 8, (size_t)R, stream);
  if (e == hipSuccess) e = sync(stream, ev_gpu, "cch-matrix+greedy");
  if (e != hipSuccess) return false;
  for (int k = 0; k < R; ++k) unpack_plan(m[k], tb.h_npts2.h[k], NM, k, any_imp);
  return true;
}

// K6b over the rows K6 just wrote (same stream, before the read-back): the flags go up, visit is
// rewritten in place for the asking rows, the statistics come back with the trips.
hipError_t RouteService::Impl::improve_rows(bool any, const int* d_npts, int R, int NM) {
  if (!any) return hipSuccess;
  hipError_t e = hipSuccess;
  cp(e, tb.imp.d_flag.d, tb.imp.h_flag.h, (size_t)R);
  if (e == hipSuccess)
    e = launch_improve_trips(tb.d_D.d, d_npts, tb.d_maxd.d, tb.imp.d_flag.d, tb.d_status.d, R, NM, tb.d_visit.d, tb.d_trip.d,
                             tb.imp.d_moves.d, tb.imp.d_changed.d, tb.imp.d_before.d, tb.imp.d_after.d, stream);
  cp(e, tb.imp.h_moves.h, tb.imp.d_moves.d, (size_t)R * 4);
  cp(e, tb.imp.h_changed.h, tb.imp.d_changed.d, (size_t)R * 4);
  cp(e, tb.imp.h_before.h, tb.imp.d_before.d, (size_t)R * 8);
  cp(e, tb.imp.h_after.h, tb.imp.d_after.d, (size_t)R * 8);
  if (!std::any_of(tb.imp.h_xflag.h, tb.imp.h_xflag.h + R, [](unsigned char f) { return f != 0; })) return e;
  // "exchange" rows: K6c (route_exchange.hip) moves stops between their trips, then K6b once more
  // over those rows only, into second statistics buffers (K6b writes every row's statistics, and
  // the improve-only rows' are in the first)
  cp(e, tb.imp.d_xflag.d, tb.imp.h_xflag.h, (size_t)R);
  if (e == hipSuccess)
    e = launch_exchange_trips(tb.d_D.d, d_npts, tb.d_dem.d, tb.d_cap.d, tb.d_maxd.d, tb.imp.d_xflag.d, tb.d_status.d, R, NM, -1,
                              tb.d_visit.d, tb.d_trip.d, tb.d_ntrips.d, tb.imp.d_xmoves.d, tb.imp.d_xrej.d, tb.imp.d_xtb.d,
                              tb.imp.d_xta.d, tb.imp.d_xbefore.d, tb.imp.d_xafter.d, stream);
  if (e == hipSuccess)
    e = launch_improve_trips(tb.d_D.d, d_npts, tb.d_maxd.d, tb.imp.d_xflag.d, tb.d_status.d, R, NM, tb.d_visit.d, tb.d_trip.d,
                             tb.imp.d_moves2.d, tb.imp.d_changed2.d, tb.imp.d_before2.d, tb.imp.d_after2.d, stream);
  cp(e, tb.imp.h_xmoves.h, tb.imp.d_xmoves.d, (size_t)R * 4);
  cp(e, tb.imp.h_xtb.h, tb.imp.d_xtb.d, (size_t)R * 4);
  cp(e, tb.imp.h_xta.h, tb.imp.d_xta.d, (size_t)R * 4);
  cp(e, tb.imp.h_moves2.h, tb.imp.d_moves2.d, (size_t)R * 4);
  cp(e, tb.imp.h_after2.h, tb.imp.d_after2.d, (size_t)R * 8);
  return e;
}

// K6 output of request k -> its Plan (trips, or the infeasible stops by depot distance); `improved`:
// K6b ran over the flush's rows, so an asking request carries its statistics
void RouteService::Impl::unpack_plan(RouteJob* j, int n, int NM, int k, bool improved) {
  rtr::Plan& p = j->plan;
  const int* vis = tb.h_visit.h + (size_t)k * NM;
  const int* tof = tb.h_trip.h + (size_t)k * NM;
  if (tb.h_status.h[k] != 0) {           // batched.py _unpack: unplaced stops by depot distance
    std::vector<char> placed(n, 0);
    for (int i = 0; i < NM && vis[i] >= 0; ++i) placed[vis[i]] = 1;
    std::vector<int> rest;
    for (int i = 1; i < n; ++i)
      if (!placed[i]) rest.push_back(i);
    const double* d0 = tb.h_row0.h + (size_t)k * NM;
    std::stable_sort(rest.begin(), rest.end(), [&](int a, int c) { return d0[a] < d0[c]; });
    p.infeasible = true;
    for (int i : rest) p.infeasible_stops.push_back(i - 1);
    return;
  }
  p.trips.assign(tb.h_ntrips.h[k], std::vector<int>{0});
  for (int i = 0; i < NM && vis[i] >= 0; ++i) p.trips[tof[i]].push_back(vis[i]);
  for (auto& t : p.trips) t.push_back(0);
  if (improved && j->req.exchange) {  // exchange.py compose_stats
    p.improved = true;
    p.imp.exchange = true;
    p.imp.moves = (long long)tb.imp.h_moves.h[k] + tb.imp.h_moves2.h[k];
    p.imp.exchange_moves = tb.imp.h_xmoves.h[k];
    p.imp.trips_before = tb.imp.h_xtb.h[k];
    p.imp.trips_after = tb.imp.h_xta.h[k];
    p.imp.len_before_q = tb.imp.h_before.h[k];
    p.imp.len_after_q = tb.imp.h_after2.h[k];
  } else if (improved && j->req.improve) {
    p.improved = true;
    p.imp.moves = tb.imp.h_moves.h[k];
    p.imp.trips_changed = tb.imp.h_changed.h[k];
    p.imp.len_before_q = tb.imp.h_before.h[k];
    p.imp.len_after_q = tb.imp.h_after.h[k];
  }
}

}  // namespace rt
