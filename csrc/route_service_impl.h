// Native route service, private: the flush in flight, the stages' buffers and RouteService::Impl.
//   route_service.hip        queue, threads, watchdog, hand-off, assembly + ETA, lifecycle, public API
//   route_service_plan.hip   routing contexts (CCH) and the trips (K5 / road matrices + K6)
//   route_service_legs.hip   snapping, the leg searches (CCH / A*), path compaction, alternatives
#pragma once
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <deque>
#include <functional>
#include <list>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "common.h"
#include "ops.h"
#include "route_service.h"
#include "route_service_bufs.h"

namespace rt {

// One flush in flight between the two stages: its jobs and the legs its responses are built from.
struct Batch {
  std::vector<RouteJob*> jobs;
  std::vector<std::shared_ptr<CchMetricDev>> metrics;   // per routing-context group (CCH)
  std::vector<std::shared_ptr<const std::vector<float>>> host_cost;   // their edge costs on the host
  std::vector<rtr::Leg> legs;
  std::vector<std::vector<int32_t>> host_paths;
  std::vector<int32_t> flat;                 // found paths, compacted (Leg::path points in here)
  std::vector<int32_t> flat_e;               // their hop edges (CCH; Leg::edges points in here)
  std::unordered_map<uint64_t, int> leg_index;
  bool failed = false;
  // "alternatives" jobs of the flush: the scorer snapshot they use
  std::shared_ptr<const std::vector<double>> alt_delay;
  int alt_kind = 0;
  std::string alt_engine;
  std::vector<RouteJob*> save;               // jobs whose rows the persistence thread writes
};

inline double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline rtc::Stamp local_now(int64_t skew_s = 0) {
  struct timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  struct tm lt;
  time_t t = ts.tv_sec + (time_t)skew_s;
  localtime_r(&t, &lt);
  rtc::Stamp s;
  s.secs = rtc::days_from_civil(lt.tm_year + 1900, (unsigned)lt.tm_mon + 1, (unsigned)lt.tm_mday) * 86400 +
           lt.tm_hour * 3600 + lt.tm_min * 60 + lt.tm_sec;
  s.us = (int32_t)(ts.tv_nsec / 1000);
  return s;
}

// The stages' buffers.  Each stage and prewarm() size them through the same reserve (true: all
// there), so a buffer added to a stage is prewarmed with it.
//
// Trips: R requests of up to NM points — K5 + K6 over coordinates, or (road) the CCH matrices +
// K6 over snapped nodes, each row with its routing-context group.
struct TripBufs {
  HostBuf<double> h_lat, h_lon, h_dem, h_cap, h_maxd, h_row0;
  HostBuf<int> h_npts, h_visit, h_trip, h_ntrips, h_status;
  DevBuf<double> d_lat, d_lon, d_dem, d_cap, d_maxd, d_D;
  DevBuf<int> d_npts, d_visit, d_trip, d_ntrips, d_status;
  HostBuf<int> h_pts, h_npts2, h_rowg;
  DevBuf<int> d_pts, d_npts2, d_rowg;
  DevBuf<float> d_msec, d_mmet;
  ImproveBufs imp;
  bool reserve(size_t R, size_t NM, bool road) {
    const size_t RN = R * NM;
    if (!imp.reserve(R)) return false;
    if (road)
      return !(h_pts.need(RN) || h_npts2.need(R) || h_dem.need(RN) || h_cap.need(R) || h_maxd.need(R) ||
               h_visit.need(RN) || h_trip.need(RN) || h_ntrips.need(R) || h_status.need(R) || h_row0.need(RN) ||
               d_pts.need(RN) || d_npts2.need(R) || d_dem.need(RN) || d_cap.need(R) || d_maxd.need(R) ||
               d_D.need(RN * NM) || d_msec.need(RN * NM) || d_mmet.need(RN * NM) || d_visit.need(RN) ||
               d_trip.need(RN) || d_ntrips.need(R) || d_status.need(R) || h_rowg.need(R) || d_rowg.need(R));
    return !(h_lat.need(RN) || h_lon.need(RN) || h_dem.need(RN) || h_npts.need(R) || h_cap.need(R) || h_maxd.need(R) ||
             h_visit.need(RN) || h_trip.need(RN) || h_ntrips.need(R) || h_status.need(R) || h_row0.need(RN) ||
             d_lat.need(RN) || d_lon.need(RN) || d_dem.need(RN) || d_npts.need(R) || d_cap.need(R) || d_maxd.need(R) ||
             d_D.need(RN * NM) || d_visit.need(RN) || d_trip.need(RN) || d_ntrips.need(R) || d_status.need(R));
  }
};

// Legs: Q unique legs with paths of up to MP nodes — the batched A*, or (cch) the CCH's route
// calls with hop edges, metres, each leg's group and, for the first QA legs, their matrix cell.
// The found paths leave compacted into the flat arrays, sized once the lengths are known.
struct LegBufs {
  HostBuf<int> h_src, h_dst, h_len, h_st, h_qidx, h_flat, h_flat_e;
  HostBuf<float> h_cost, h_met;
  HostBuf<long long> h_off;
  DevBuf<int> d_src, d_dst, d_len, d_st, d_path, d_qidx, d_flat, d_iters, d_edge, d_flat_e;
  DevBuf<float> d_cost, d_met;
  DevBuf<long long> d_off;
  HostBuf<int> h_lgrp, h_lr, h_li, h_lj;
  DevBuf<int> d_lgrp, d_lr, d_li, d_lj;
  bool reserve(size_t Q, size_t QA, size_t MP, bool cch) {
    if (!cch)
      return !(h_src.need(Q) || h_dst.need(Q) || h_len.need(Q) || h_st.need(Q) || h_cost.need(Q) || h_off.need(Q) ||
               h_qidx.need(Q) || d_src.need(Q) || d_dst.need(Q) || d_len.need(Q) || d_st.need(Q) || d_cost.need(Q) ||
               d_off.need(Q) || d_qidx.need(Q + 1) || d_iters.need(Q) || d_path.need(Q * MP));
    if (h_src.need(Q) || h_dst.need(Q) || h_len.need(Q) || h_st.need(Q) || h_cost.need(Q) || h_met.need(Q) ||
        h_off.need(Q) || d_src.need(Q) || d_dst.need(Q) || d_len.need(Q) || d_st.need(Q) || d_cost.need(Q) ||
        d_met.need(Q) || d_off.need(Q) || d_path.need(Q * MP) || d_edge.need(Q * MP) || h_lgrp.need(Q) ||
        d_lgrp.need(Q))
      return false;
    return QA == 0 ||
           !(h_lr.need(QA) || h_li.need(QA) || h_lj.need(QA) || d_lr.need(QA) || d_li.need(QA) || d_lj.need(QA));
  }
  bool reserve_flat(size_t total) { return !(h_flat.need(total) || d_flat.need(total)); }
  bool reserve_flat_e(size_t total) { return !(h_flat_e.need(total) || d_flat_e.need(total)); }
};

// CCH: the flush's metrics as device views (one per context group), and the pinned staging of a
// metric's edge costs on their way to the host
struct CchBufs {
  HostBuf<CchMView> h_mv;
  DevBuf<CchMView> d_mv;
  HostBuf<float> h_hcost;
  bool reserve(size_t G) { return !(h_mv.need(G) || d_mv.need(G)); }
};

struct EtaBufs {
  HostBuf<rtc::EtaRecord> h_rec;
  HostBuf<float> h_eta;
  DevBuf<rtc::EtaRecord> d_rec;
  DevBuf<float> d_eta;
  bool reserve(size_t n) { return !(h_rec.need(n) || h_eta.need(n) || d_rec.need(n) || d_eta.need(n)); }
};

struct RouteService::Impl {
  RouteServiceCfg cfg;
  std::function<void(RouteJob*)> done;
  // chunks per parallel_chunks call: cfg.chunk_threads, a 1/k share of the process's CPU pool when
  // k route services run per GPU (profiles/route_pipelines_r6ax.md: two services' full fan-outs
  // oversubscribed the box's CPU share and raised the no-store p99 from 15 to 34 ms)
  unsigned chunk_threads() const { return (unsigned)(cfg.chunk_threads < 1 ? 1 : cfg.chunk_threads); }
  std::function<void(std::vector<RouteJob*>&)> done_many;
  void done_all(std::vector<RouteJob*>& js) {
    if (js.empty()) return;
    if (done_many) {
      done_many(js);
    } else {
      for (RouteJob* j : js) done(j);
    }
  }
  std::mutex mu;
  std::condition_variable cv;
  std::deque<RouteJob*> q;
  bool stop = false;
  std::thread th, th_asm;
  hipStream_t stream{}, stream_asm{};
  rtr::NodeGrid grid;
  // GPU stage -> assembly stage hand-off (at most 2 flushes waiting: the GPU runs ahead by one)
  std::mutex amu;
  std::condition_variable acv;
  std::deque<Batch*> aq;
  bool gpu_done = false;
  // statistics
  std::atomic<long long> n_legs_reused{0};
  std::atomic<long long> n_jobs{0}, n_flushes{0}, n_fallback{0}, n_legs{0}, n_host_legs{0}, n_escalated{0};
  // stage times (us): parse, trips (K5+K6), snap, A*, copy-out, assembly, ETA, persistence
  std::atomic<long long> t_stage[8] = {};
  // GPU thread waits (us): collecting a flush after its first job, handing it to a full assembly queue
  std::atomic<long long> t_collect_us{0}, t_handoff_us{0};
  void add_t(int k, double t0) {
    const long long dt = (long long)(now_us() - t0);
    t_stage[k].fetch_add(dt, std::memory_order_relaxed);
    if (trace_ms >= 0 && dt > trace_ms * 1e3) {   // a stage that alone outlasts the trace threshold
      static const char* const names[8] = {"parse", "trips", "snap", "astar", "copyout", "assemble", "eta", "persist"};
      trace("stage %s took %.1f ms", names[k], dt * 1e-3);
    }
  }
  TripBufs tb;
  LegBufs lb;
  CchBufs cb;
  EtaBufs eb;
  ModelWs eta_ws;
  // a stage's chained queue-local copies on the GPU stage's stream: the first error sticks
  void cp(hipError_t& e, void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess) e = qcopy(dst, src, bytes, stream);
  }
  // CCH
  CchScratch csc;
  // the matrix stage's chains (kept for the multi-stop legs), the tag of its matrix call and each
  // multi-stop job's row in it; the flush's metrics as device views (one per context group) and the
  // group of every request row / leg, so ONE launch sequence serves all the flush's contexts
  CchScratch msc;
  uint64_t mtag = 0;
  std::unordered_map<const RouteJob*, int> jrow;
  // host copies of metrics' edge costs (maneuver durations, exact host fallback): LRU by key
  std::mutex hc_mu;
  std::list<std::pair<uint64_t, std::shared_ptr<const std::vector<float>>>> hc_lru;
  std::unordered_map<uint64_t, decltype(hc_lru)::iterator> hc_index;
  static constexpr size_t HC_MAX = 64;
  std::atomic<long long> n_ctx_built{0};
  std::atomic<long long> t_ctx_us{0};
  // Routing contexts off the flush's critical path (CCH): a job whose context is not customized
  // yet waits here while the router's background builder customizes it; the rest of its flush
  // proceeds.  The build's listener puts the jobs back at the head of the queue.
  bool async_ctx = true;
  int listener = 0;
  std::mutex wmu;
  std::unordered_map<uint64_t, std::vector<RouteJob*>> waiting;
  std::atomic<long long> n_deferred{0}, t_wait_us{0}, n_prefetch{0};
  // latency watchdog: every wait on the flush's GPU work is bounded (ROUTEST_ROUTE_DEADLINE_MS)
  double deadline_ms = 2000.0;
  // the deadline of the current flush's waits: deadline_ms scaled with its work (a healthy
  // flush of oversized requests — NM up to 4096 stops, or a context built synchronously — must not
  // read as a hung GPU and quarantine the slot)
  std::atomic<double> flush_deadline_ms{2000.0};
  std::atomic<bool> broken{false};
  hipEvent_t ev_gpu{}, ev_asm{};
  hipStream_t hang_stream{};              // the gpu_hang fault hook's stream (own hardware queue)
  std::atomic<long long> n_failed_over{0};
  std::atomic<long long> n_records{0}, n_record_bytes{0};
  bool fail_fault = false;                 // ROUTEST_FAULT=route_fail (test hook)

  // ROUTEST_ROUTE_TRACE_MS=<ms>: every wait on the GPU longer than that, every deadline, hand-off and
  // recovery is logged to stderr with the slot and a steady-clock time stamp (the watchdog rehearsal's
  // timeline: which wait of which slot stalled, and on what)
  double trace_ms = -1.0;
  void trace(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    if (trace_ms < 0) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "[route slot %d t=%.3f] %s\n", cfg.slot,
                 std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(), buf);
  }
  hipError_t sync(hipStream_t s, hipEvent_t ev, const char* what = "");
  // the work that missed the deadline has drained: the service's buffers are its own again
  bool drained() {
    return (!ev_gpu || hipEventQuery(ev_gpu) != hipErrorNotReady) && (!ev_asm || hipEventQuery(ev_asm) != hipErrorNotReady);
  }
  void hand_off(std::vector<RouteJob*>& jobs);
  // prefetch of the next week-hour: (weather, congestion) of requests routed at "now" -> last seen
  std::unordered_map<int, double> seen_now;
  int prefetched_wh = -1;
  int64_t clock_skew_s = 0;
  std::unordered_set<int> prefetched;      // pairs already queued for prefetched_wh
  int prefetch_min = 10;
  // store: the writer (csrc/runtime/route_store.h), and the assembly -> persistence hand-off
  // (every flush waiting is one group commit)
  rts::RouteStore store;
  std::thread th_persist;
  std::mutex pmu;
  std::condition_variable pcv;
  std::deque<std::vector<RouteJob*>> pq;
  bool asm_done = false;

  rtr::CoordCache coord_cache;             // graph nodes' "[lon,lat]" strings (graph provider)
  std::vector<double> edge_heading;        // per road edge: rtr::hop_heading (graph provider)
  // compact route records (runtime/route_record.h): the graph view persisted rows are encoded
  // against — the server's shared one, or this service's own over the tables above
  std::shared_ptr<const rrec::RecordGraph> rg;
  const rtr::CoordCache* ccache() const {
    if (rg) return rg->cc;
    return coord_cache.ofs.empty() ? nullptr : &coord_cache;
  }
  const double* headings() const {
    if (rg) return rg->heading;
    return edge_heading.empty() ? nullptr : edge_heading.data();
  }
  static uint64_t leg_key(int group, int s, int t) {
    return ((uint64_t)(uint32_t)group << 48) ^ ((uint64_t)(uint32_t)s << 24) ^ (uint64_t)(uint32_t)t;
  }

  // route_service.hip
  void run();
  void asm_loop();
  void persist_loop();
  void prewarm();
  void on_built(uint64_t key, bool ok);
  static void parse_job(RouteJob* j);
  void gpu_stage(Batch& b);
  void asm_stage(Batch& b);
  void assemble_all(Batch& b);
  bool run_eta(std::vector<RouteJob*>& jobs);
  void finish(RouteJob* j);
  // route_service_plan.hip
  std::shared_ptr<const std::vector<float>> host_costs(const std::shared_ptr<CchMetricDev>& m);
  bool cch_groups(Batch& b);
  bool plan_multi(std::vector<RouteJob*>& jobs);
  bool plan_multi_road(Batch& b);
  hipError_t improve_rows(bool any, const int* d_npts, int R, int NM);
  void unpack_plan(RouteJob* j, int n, int NM, int k, bool improved);
  // route_service_legs.hip
  std::vector<RouteJob*> snap_jobs(Batch& b);
  bool compact_out(Batch& b, int Q, bool edges, const char* what);
  bool search_legs_cch(Batch& b);
  bool search_legs(Batch& b);
  void choose_alternatives(Batch& b, RouteJob* j);
};

}  // namespace rt
