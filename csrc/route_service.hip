// Native route service: /api/optimize_route, /route and /api/request_route answered without Python
// (reference RO/Flaskr/routes.py:29-50,89-127 -> RO/Flaskr/utils.py:10-201; Python equivalent
// routest_amd/routing/route_batcher.py + optimizer.py + api/app.py _optimize).
//
// One worker thread per GPU pulls the requests the native front end's reactors parsed off their
// sockets, and flushes them together (batch_max requests or timeout_us after the first):
//   1. parse + validate every request (csrc/runtime/route_core.h RouteReq; unusual inputs are
//      handed back for the Python app);
//   2. ONE K5 + ONE K6 launch for every multi-stop request of the flush (csrc/route_kernels.hip);
//      only the trips and, for infeasible requests, the depot row of D come back to the host;
//   3. road-graph provider: every waypoint snapped (NodeGrid), the flush's unique legs searched on
//      the CCH (csrc/cch.hip, under each request's routing context) or by the batched A*
//      (csrc/astar.hip), and the found paths COMPACTED on the GPU into one flat array before the
//      copy-out (a leg row is max_path ints; a path is ~200);
//   4. responses assembled on the assembly thread (route_core.h: byte-identical to the FastAPI
//      handler) while the GPU stage runs the next flush;
//   5. use_ml_eta: one fused featurize+MLP launch (K1+K2) for the flush's ETA records;
//   6. persistence of /api/optimize_route results on a thread of its own: every flush waiting is
//      group-committed in one SQLite transaction into the database file the Python store reads
//      (reference routes.py:119-125, best effort; the writer and its WAL checkpoint thread are
//      csrc/runtime/route_store.h);
//   7. completed jobs go back to their reactors (eventfd wake-up), which write the bytes -- a
//      persisted job only after its commit.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "route_service_impl.h"

namespace rt {

namespace {

// the watchdog's fault hook (ROUTEST_FAULT=gpu_hang@<slot>): one wave waiting on a host flag, at
// most max_ticks of the 100 MHz wall clock; reads only, every wave reaches the exit condition
__global__ __launch_bounds__(64) void route_hang_kernel(const int* release, long long max_ticks) {
  const long long t0 = wall_clock64();
  // (also bounded by iterations: ~3.4 us per sleep at 2.4 GHz, 2M of them ~7 s, whatever the
  // wall clock's rate)
  for (int it = 0; it < 2000000 && __hip_atomic_load(release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 &&
                   wall_clock64() - t0 < max_ticks;
       ++it)
    __builtin_amdgcn_s_sleep(127);
}

}  // namespace

hipError_t RouteService::Impl::sync(hipStream_t s, hipEvent_t ev, const char* what) {
  hipError_t e = hipEventRecord(ev, s);
  if (e != hipSuccess) return e;
  const auto t0 = std::chrono::steady_clock::now();
  auto waited = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  for (int i = 0;; ++i) {
    e = hipEventQuery(ev);
    if (e != hipErrorNotReady) {
      if (trace_ms >= 0 && waited() > trace_ms) trace("wait %s %.1f ms", what, waited());
      return e;
    }
    const double dl = flush_deadline_ms.load(std::memory_order_relaxed);
    if (dl > 0 && (i & 15) == 15 && waited() > dl) {
      trace("DEADLINE in %s after %.1f ms", what, waited());
      if (!broken.exchange(true) && cfg.on_timeout) cfg.on_timeout();
      return hipErrorLaunchTimeOut;
    }
    if (i > 4096) std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// jobs of a failed / abandoned flush: to another GPU's route service, else relayed to the app
void RouteService::Impl::hand_off(std::vector<RouteJob*>& jobs) {
  for (RouteJob* j : jobs) {
    if (!j->fallback && !j->status && cfg.failover) {
      j->plan = rtr::Plan();
      j->calls.clear();
      j->nodes.clear();
      j->group = 0;
      j->alt_pairs.clear();
      j->alt_vias.clear();
      j->alt_legs.clear();
      j->alt_paths.clear();
      j->alt_edges.clear();
      j->alt_json.clear();
      j->row.asmb = rtr::Assembled();
      if (cfg.failover(j)) {
        n_failed_over.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      trace("no other route service takes the job (hops %d): relayed to the app", j->hops);
    }
    if (!j->status) j->fallback = true;
    finish(j);
    done(j);
  }
  jobs.clear();
}

void RouteService::Impl::run() {
  if (hipSetDevice(cfg.device) != hipSuccess) return;
  // the query stream at the highest priority: the router's background context builds (lowest
  // priority, csrc/cch.hip builder_loop) never delay a flush's launches
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
      hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, greatest) != hipSuccess) {
    (void)hipGetLastError();
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return;
  }
  if (const char* v = std::getenv("ROUTEST_CCH_ASYNC")) async_ctx = std::string(v) != "0";
  if (const char* v = std::getenv("ROUTEST_ROUTE_DEADLINE_MS")) deadline_ms = std::atof(v);
  flush_deadline_ms.store(deadline_ms);
  if (const char* v = std::getenv("ROUTEST_ROUTE_TRACE_MS")) trace_ms = std::atof(v);
  // ROUTEST_FAULT=route_fail: every flush of every service fails (not a timeout) — the hop limit
  // of the failover must end each job at the app
  if (const char* v = std::getenv("ROUTEST_FAULT")) fail_fault = std::string(v).find("route_fail") != std::string::npos;
  if (hipEventCreateWithFlags(&ev_gpu, hipEventDisableTiming) != hipSuccess) ev_gpu = nullptr;
  if (const char* v = std::getenv("ROUTEST_CCH_PREFETCH_MIN")) prefetch_min = std::atoi(v);
  // rehearsal knob (bench/route_context_bench.py): shifts the clock "now" routing contexts are
  // resolved with, so an hour boundary can be crossed on demand
  if (const char* v = std::getenv("ROUTEST_ROUTE_CLOCK_SKEW_S")) clock_skew_s = std::atoll(v);
  if (cfg.cch != nullptr && cfg.cch_contexts && async_ctx) {
    listener = cfg.cch->add_build_listener([this](uint64_t key, bool ok) { on_built(key, ok); });
    cfg.cch->start_builders();         // their allocations at startup, not mid-serving
  }
  if (std::getenv("ROUTEST_ROUTE_PREWARM") == nullptr || std::string(std::getenv("ROUTEST_ROUTE_PREWARM")) != "0")
    prewarm();
  if (const char* v = std::getenv("ROUTEST_HANG_ARM"))      // the watchdog rehearsal: see native_server.hip
    if (std::string(v) == "1" && isolated_stream(cfg.device, &hang_stream) != hipSuccess) hang_stream = nullptr;
  th_asm = std::thread([this] { asm_loop(); });
  while (true) {
    auto* b = new Batch();
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || !q.empty(); });
      if (stop && q.empty()) { delete b; break; }
      // collect: up to batch_max, or timeout_us after the OLDEST queued job's arrival — jobs that
      // queued during the previous flush's GPU stage have waited long enough already (timing the
      // window from this wake-up added up to timeout_us to every flush of a busy service)
      const double t_wake = now_us();
      static const bool from_wake = [] {   // ROUTEST_ROUTE_COLLECT=wake: the round-5 window (A/B)
        const char* v = std::getenv("ROUTEST_ROUTE_COLLECT");
        return v && std::string(v) == "wake";
      }();
      const double t_open = from_wake ? t_wake : q.front()->t_enq_us;
      const auto deadline = std::chrono::steady_clock::time_point(std::chrono::duration_cast<std::chrono::steady_clock::duration>(
          std::chrono::duration<double, std::micro>(t_open + cfg.timeout_us)));
      while ((int)q.size() < cfg.batch_max && !stop && std::chrono::steady_clock::now() < deadline) {
        if (cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
      t_collect_us.fetch_add((long long)(now_us() - t_wake), std::memory_order_relaxed);
      const size_t take = std::min<size_t>(q.size(), (size_t)cfg.batch_max);
      b->jobs.assign(q.begin(), q.begin() + take);
      q.erase(q.begin(), q.begin() + take);
    }
    if (broken.load()) {
      if (drained()) {
        trace("drained: serving again");
        broken.store(false);      // the late work finished: buffers and streams usable again
      } else {
        trace("broken: handing %zu jobs off", b->jobs.size());
        hand_off(b->jobs);
        delete b;
        continue;
      }
    }
    // gpu_hang fault hook: this flush's GPU work goes to a stream on a hardware queue of its own,
    // behind a kernel that waits on the host flag (abandoned, not destroyed, if it hangs)
    hipStream_t main_stream = stream;
    if (cfg.hang_fault && cfg.hang_release_d && cfg.hang_fault()) {
      if (!hang_stream && isolated_stream(cfg.device, &hang_stream) != hipSuccess) hang_stream = nullptr;
      if (hang_stream) {
        stream = hang_stream;
        hipLaunchKernelGGL(route_hang_kernel, dim3(1), dim3(64), 0, stream, cfg.hang_release_d, 500000000ll);
      }
    }
    gpu_stage(*b);
    stream = main_stream;         // (the hang stream is reused once drained: see drained())
    if (fail_fault && !b->jobs.empty()) b->failed = true;
    if (b->failed) {              // a GPU error or the deadline: another GPU's service answers
      trace("flush of %zu jobs failed: handing off", b->jobs.size());
      hand_off(b->jobs);
      delete b;
      continue;
    }
    if (b->jobs.empty()) {        // every job of the flush is waiting for its routing context
      delete b;
      continue;
    }
    const double t_h = now_us();
    std::unique_lock<std::mutex> lk(amu);
    acv.wait(lk, [&] { return aq.size() < 2; });
    t_handoff_us.fetch_add((long long)(now_us() - t_h), std::memory_order_relaxed);
    aq.push_back(b);
    acv.notify_all();
  }
  // stopping: no more requeues; jobs still waiting for a context go to the app
  if (listener) cfg.cch->remove_build_listener(listener);
  std::vector<RouteJob*> left;
  {
    std::lock_guard<std::mutex> lk(wmu);
    for (auto& kv : waiting) left.insert(left.end(), kv.second.begin(), kv.second.end());
    waiting.clear();
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    left.insert(left.end(), q.begin(), q.end());
    q.clear();
  }
  for (RouteJob* j : left) {
    j->fallback = true;
    finish(j);
    done(j);
  }
  {
    std::lock_guard<std::mutex> lk(amu);
    gpu_done = true;
  }
  acv.notify_all();
  th_asm.join();
  (void)hipStreamDestroy(stream);
  if (ev_gpu) (void)hipEventDestroy(ev_gpu);
}

void RouteService::Impl::asm_loop() {
  if (hipSetDevice(cfg.device) != hipSuccess) return;
  if (hipStreamCreateWithFlags(&stream_asm, hipStreamNonBlocking) != hipSuccess) return;
  if (hipEventCreateWithFlags(&ev_asm, hipEventDisableTiming) != hipSuccess) ev_asm = nullptr;
  store.open(cfg.sqlite_path);
  th_persist = std::thread([this] { persist_loop(); });
  while (true) {
    Batch* b = nullptr;
    {
      std::unique_lock<std::mutex> lk(amu);
      acv.wait(lk, [&] { return gpu_done || !aq.empty(); });
      if (aq.empty()) break;
      b = aq.front();
      aq.pop_front();
      acv.notify_all();
    }
    asm_stage(*b);
    n_flushes.fetch_add(1, std::memory_order_relaxed);
    // jobs that persist nothing answer now; the others after their group commit
    std::vector<RouteJob*> save = std::move(b->save);
    std::vector<RouteJob*> now_done;
    {
      const std::unordered_set<RouteJob*> saving(save.begin(), save.end());
      for (RouteJob* j : b->jobs)
        if (!saving.count(j)) {
          finish(j);
          now_done.push_back(j);
        }
    }
    done_all(now_done);
    delete b;
    if (!save.empty()) {
      std::unique_lock<std::mutex> lk(pmu);
      pcv.wait(lk, [&] { return pq.size() < 8; });     // back-pressure on a stalled disk
      pq.push_back(std::move(save));
      pcv.notify_all();
    }
  }
  {
    std::lock_guard<std::mutex> lk(pmu);
    asm_done = true;
  }
  pcv.notify_all();
  th_persist.join();
  (void)hipStreamDestroy(stream_asm);
  if (ev_asm) (void)hipEventDestroy(ev_asm);
}

// Buffers sized up front for a full flush of dashboard-sized requests (batch_max requests of up to
// 10 stops, MAX_STOPS of the UI): growing one mid-serving allocates while other GPU work is in
// flight (a flush handed over from another GPU doubles this service's flush size at once).
void RouteService::Impl::prewarm() {
  const size_t R = (size_t)std::max(1, cfg.batch_max), NM = 11, RN = R * NM, Q = RN;
  const size_t MP = (size_t)std::max(1, cfg.max_path);
  bool ok = tb.reserve(R, NM, false) && lb.reserve(Q, Q, MP, cfg.cch != nullptr) && lb.reserve_flat(Q * 256) &&
            eb.reserve(R);
  if (cfg.cch != nullptr) {
    ok = ok && tb.reserve(R, NM, true) && lb.reserve_flat_e(Q * 256) && cb.reserve(R) &&
         cb.h_hcost.need((size_t)cfg.cch->topo().E) == hipSuccess;
    const int S = cfg.cch->stride();
    msc.device = cfg.device;
    ok = ok && msc.ensure(RN * 2, std::max(Q, (RN * NM * 2 + CchGpu::MAX_ARCS - 1) / CchGpu::MAX_ARCS + 1), S,
                              CchGpu::MAX_ARCS) == hipSuccess;
  }
  if (!ok) (void)hipGetLastError();       // best effort: the flushes grow what is missing
}

// a context's background build finished: its waiting jobs go back to the head of the queue
// (a failed build: they build it synchronously in their next flush, which reports the error)
void RouteService::Impl::on_built(uint64_t key, bool ok) {
  std::vector<RouteJob*> js;
  {
    std::lock_guard<std::mutex> lk(wmu);
    auto it = waiting.find(key);
    if (it == waiting.end()) return;
    js.swap(it->second);
    waiting.erase(it);
  }
  if (!ok)
    for (RouteJob* j : js) j->sync_ctx = true;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (auto it = js.rbegin(); it != js.rend(); ++it) q.push_front(*it);
  }
  cv.notify_one();
}

void RouteService::Impl::assemble_all(Batch& b) {
  std::vector<RouteJob*>& jobs = b.jobs;
  const std::vector<rtr::Leg>& legs = b.legs;
  const std::unordered_map<uint64_t, int>& leg_index = b.leg_index;
  rtc::parallel_chunks(jobs.size(), 8, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      RouteJob* j = jobs[i];
      if (j->fallback || j->status) continue;
      if (j->req.alt_k > 0) choose_alternatives(b, j);
      std::vector<rtr::Dir> dirs(j->calls.size());
      std::string perr;
      size_t off = 0;
      // the compact record of a route that will be persisted (graph provider, no alternatives)
      bool want_rec = rg != nullptr && store.opened() && !j->request_route && j->req.alt_k == 0 &&
                      cfg.provider == 1 && !j->calls.empty();
      rrec::Writer rw;
      std::vector<uint64_t> durs;
      std::vector<uint32_t> per_leg;
      j->row.rec.clear();
      for (size_t k = 0; k < j->calls.size() && perr.empty(); ++k) {
        if (cfg.provider == 0) {
          rtr::haversine_directions(j->calls[k], j->req.profile, cfg.circuity, cfg.step_m, dirs[k]);
        } else {
          std::vector<const rtr::Leg*> lp;
          for (size_t t = 0; t + 1 < j->calls[k].size(); ++t) {
            const int s0 = j->nodes[off + t], s1 = j->nodes[off + t + 1];
            if (j->req.alt_k > 0) {        // the pair's chosen candidate
              size_t a = 0;
              while (j->alt_pairs[a].first != s0 || j->alt_pairs[a].second != s1) ++a;
              lp.push_back(&j->alt_legs[a]);
              continue;
            }
            const uint64_t key = cfg.cch ? leg_key(j->group, s0, s1)
                                         : (((uint64_t)(uint32_t)s0 << 32) | (uint32_t)s1);
            lp.push_back(&legs[leg_index.at(key)]);
          }
          rtr::GraphHost gh;
          const rtr::GraphHost* ghp = nullptr;
          if (cfg.cch && cfg.h_length != nullptr) {
            gh.indptr = cfg.h_indptr;
            gh.indices = cfg.h_indices;
            gh.length = cfg.h_length;
            gh.cost = b.host_cost[j->group]->data();
            gh.edge_name = cfg.h_edge_name;
            gh.names = &cfg.names;
            gh.edge_heading = headings();
            ghp = &gh;
          }
          if (k == 0 && want_rec) rrec::begin(rw, *rg, ghp != nullptr, j->req.profile, j->calls.size());
          durs.clear();
          per_leg.clear();
          rtr::StepDurs sd;
          sd.out = &durs;
          sd.per_leg = &per_leg;
          perr = rtr::graph_directions(j->calls[k], j->nodes.data() + off, lp, j->req.profile, cfg.glat, cfg.glon,
                                       dirs[k], ghp, want_rec && ghp ? &sd : nullptr);
          off += j->calls[k].size();
          if (want_rec && perr.empty())
            want_rec = !sd.bad && rrec::add_call(rw, *rg, ghp, j->calls[k], lp, durs, per_leg);
        }
      }
      if (!perr.empty()) j->req.error = perr;
      if (want_rec && perr.empty()) {
        j->row.rec = std::move(rw.b);
        n_records.fetch_add(1, std::memory_order_relaxed);
        n_record_bytes.fetch_add((long long)j->row.rec.size(), std::memory_order_relaxed);
      }
      if (!rtr::assemble(j->req, j->plan, dirs, cfg.engine, j->row.asmb, ccache()))
        j->fallback = true;
      else if (j->req.alt_k > 0 && j->row.asmb.ok) j->row.asmb.body += j->alt_json;
    }
  });
}

bool RouteService::Impl::run_eta(std::vector<RouteJob*>& jobs) {
  std::vector<RouteJob*> m;
  for (RouteJob* j : jobs)
    if (!j->fallback && !j->status && j->row.asmb.ok && j->req.use_ml_eta && j->req.eta_ok) m.push_back(j);
  if (m.empty()) return true;
  std::shared_ptr<const NativeModel> model = cfg.eta_model ? cfg.eta_model() : nullptr;
  if (model == nullptr) {          // the served model is one the native path does not run: the app answers
    for (RouteJob* j : m) j->fallback = true;
    return true;
  }
  const int n = (int)m.size();
  if (!eb.reserve((size_t)n)) return false;
  const rtc::Stamp now = local_now();
  for (int k = 0; k < n; ++k) {
    RouteJob* j = m[k];
    j->now = now;
    rtc::EtaRecord& r = eb.h_rec.h[k];
    r.distance_m = (float)j->row.asmb.dist;
    r.driver_age = (float)j->req.eta_age;
    r.wallclock_s = (int32_t)(now.secs - rtc::EPOCH2020_DAYS * 86400);
    r.weather = j->req.eta_weather;
    r.traffic = j->req.eta_traffic;
    r.pad = 0;
  }
  hipError_t e = qcopy(eb.d_rec.d, eb.h_rec.h, (size_t)n * 16, stream_asm);
  if (e == hipSuccess) e = model->predict(eb.d_rec.d, 16, eb.d_eta.d, n, stream_asm, eta_ws);
  if (e == hipSuccess) e = qcopy(eb.h_eta.h, eb.d_eta.d, (size_t)n * 4, stream_asm);
  if (e == hipSuccess) e = sync(stream_asm, ev_asm, "eta");
  // a failed GPU round: the model's fp32 CPU forward (same fallback as the reactors), into a
  // buffer of its own (a round past the deadline may still write h_eta later)
  std::vector<float> cpu_eta;
  const float* eta = eb.h_eta.h;
  if (e != hipSuccess) {
    cpu_eta.resize((size_t)n);
    std::vector<rtc::EtaRecord> rec(eb.h_rec.h, eb.h_rec.h + n);
    if (!model->cpu_predict(rec.data(), cpu_eta.data(), n)) return false;
    eta = cpu_eta.data();
  }
  for (int k = 0; k < n; ++k) {
    RouteJob* j = m[k];
    const double mins = (double)eta[k];
    // EtaService.finish: pickup + timedelta(minutes) — raises (-> no ETA fields) when out of range
    if (!std::isfinite(mins) || std::fabs(mins) > 1.4e9) continue;
    std::string tmp;
    rtc::format_one(tmp, mins, now.secs, now.us, false, 0, "");
    // {"eta_minutes_ml":X,"eta_completion_time_ml":"..."}: keep the iso text
    const size_t a = tmp.find("\"eta_completion_time_ml\":\"");
    if (a == std::string::npos) continue;
    const size_t b0 = a + 26;
    j->row.eta_iso = tmp.substr(b0, tmp.size() - 2 - b0);
    j->row.eta_min = eta[k];
  }
  return true;
}

// the request body -> j->root / j->req, once (a job back from waiting for its routing context,
// or handed over from another GPU's service, is parsed already)
void RouteService::Impl::parse_job(RouteJob* j) {
  if (j->parsed) return;
  j->parsed = true;
  bool parsed = false;
  if (j->json_ok && !j->body.empty()) {
    try {
      j->root = rtj::Parser(j->body.data(), j->body.size()).parse();
      parsed = true;
    } catch (const std::exception&) {
    }
  }
  if (j->request_route && (!j->json_ok || (!parsed && !j->body.empty()))) {
    j->fallback = true;
    return;
  }
  static const rtj::Value empty = [] { rtj::Value v; v.kind = rtj::Value::Obj; return v; }();
  const rtj::Value* rootp = parsed ? &j->root : (j->request_route ? nullptr : &empty);
  if (!j->request_route && parsed && j->root.kind != rtj::Value::Obj) rootp = &empty;
  j->req = rtr::parse_route_request(rootp);
  if (j->req.fallback) j->fallback = true;
}

// GPU stage: parse, trips (K5 + K6), snapping + the batched A* (graph provider)
void RouteService::Impl::gpu_stage(Batch& b) {
  std::vector<RouteJob*>& jobs = b.jobs;
  long long fresh_jobs = 0;
  for (RouteJob* j : jobs) fresh_jobs += !j->parsed;
  n_jobs.fetch_add(fresh_jobs, std::memory_order_relaxed);   // (submitted unparsed: none normally)
  double t0 = now_us();
  // (jobs are parsed on the submitting reactor thread, RouteService::submit; this catches any
  // that were not)
  rtc::parallel_chunks(jobs.size(), 32, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) parse_job(jobs[i]);
  });
  // "alternatives" need the road graph through the CCH and a published scorer; else the app
  bool any_alt = false;
  for (RouteJob* j : jobs) any_alt |= !j->fallback && j->req.alt_k > 0;
  if (any_alt) {
    if (cfg.alt && cfg.provider == 1 && cfg.cch != nullptr) b.alt_delay = cfg.alt->get(b.alt_kind, b.alt_engine);
    const bool ok = b.alt_delay != nullptr && (int)b.alt_delay->size() == cfg.N;
    for (RouteJob* j : jobs)
      if (!j->fallback && j->req.alt_k > 0 && (!ok || !j->req.error.empty())) j->fallback = !ok || j->fallback;
  }
  add_t(0, t0);
  {
    double pairs = 0.0;
    bool sync_build = false;
    for (RouteJob* j : jobs) {
      if (j->fallback) continue;
      const double n = (double)j->req.dst.size() + 1.0;
      pairs += n * n;
      sync_build |= j->sync_ctx;
    }
    // ~2 M matrix pairs ride on the base deadline; a synchronous context build gets 30 s more
    flush_deadline_ms.store(deadline_ms <= 0 ? deadline_ms
                                             : deadline_ms * (1.0 + pairs / 2.0e6) + (sync_build ? 30000.0 : 0.0));
  }
  if (cfg.park_scorer) cfg.park_scorer();
  t0 = now_us();
  if (cfg.provider == 1 && cfg.cch != nullptr) {
    // road graph through the CCH: contexts -> road matrices + greedy -> legs
    if (!cch_groups(b) || !plan_multi_road(b)) {
      b.failed = true;
      return;
    }
    add_t(1, t0);
    for (RouteJob* j : jobs)
      if (!j->fallback) rtr::directions_calls(j->req, j->plan, j->calls);
    if (!search_legs_cch(b)) b.failed = true;
    return;
  }
  if (!plan_multi(jobs)) { b.failed = true; return; }
  add_t(1, t0);
  for (RouteJob* j : jobs)
    if (!j->fallback) rtr::directions_calls(j->req, j->plan, j->calls);
  if (cfg.provider == 1 && !search_legs(b)) b.failed = true;
}

// assembly stage: GeoJSON, ETA, persistence, response bytes
void RouteService::Impl::asm_stage(Batch& b) {
  std::vector<RouteJob*>& jobs = b.jobs;
  if (b.failed) return;
  double t0 = now_us();
  assemble_all(b);
  add_t(5, t0);
  t0 = now_us();
  if (!run_eta(jobs)) {
    for (RouteJob* j : jobs) j->row.eta_iso.clear();
  }
  add_t(6, t0);
  // persistence (optimize_route / route only; request_route never persists) is the persistence
  // thread's: it group-commits these with whatever else is waiting
  for (RouteJob* j : jobs)
    if (store.opened() && !j->fallback && !j->status && j->row.asmb.ok && !j->request_route) b.save.push_back(j);
  t0 = now_us();
  rtc::parallel_chunks(b.save.size(), 16, chunk_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      b.save[i]->row.root = b.save[i]->req.root;
      rts::RouteStore::prepare(b.save[i]->row);
    }
  });
  add_t(7, t0);
}

// the response bytes of a job whose assembly (and persistence, if any) is done
void RouteService::Impl::finish(RouteJob* j) {
  if (j->fallback) { n_fallback.fetch_add(1, std::memory_order_relaxed); return; }
  if (j->status) return;
  if (!j->row.asmb.ok) {
    j->status = (j->request_route && cfg.compat200) ? 200 : 400;
    j->out = rtr::error_body(j->row.asmb.error.empty() ? j->req.error : j->row.asmb.error);
    return;
  }
  j->status = 200;
  j->out = std::move(j->row.asmb.body);
  if (!j->row.eta_iso.empty()) {
    j->out += ",\"eta_minutes_ml\":";
    rtr::put_float(j->out, (double)j->row.eta_min);
    j->out += ",\"eta_completion_time_ml\":";
    rtr::put_str(j->out, j->row.eta_iso);
  }
  if (!j->row.request_id.empty()) {
    j->out += ",\"request_id\":";
    rtr::put_str(j->out, j->row.request_id);
    j->out += ",\"saved\":true";
  }
  j->out += "}}";
}

// Group commit: every flush waiting when the thread wakes goes into ONE transaction
// (rts::RouteStore::commit_group).  A response leaves only after its commit, so a client that
// reads its request_id back (/api/history/<id>) finds it.
void RouteService::Impl::persist_loop() {
  while (true) {
    std::vector<std::vector<RouteJob*>> groups;
    {
      std::unique_lock<std::mutex> lk(pmu);
      pcv.wait(lk, [&] { return asm_done || !pq.empty(); });
      if (pq.empty()) break;
      groups.assign(std::make_move_iterator(pq.begin()), std::make_move_iterator(pq.end()));
      pq.clear();
      pcv.notify_all();
    }
    std::vector<RouteJob*> fin;
    std::vector<rts::StoreRow*> rows;
    for (auto& g : groups)
      for (RouteJob* j : g) {
        fin.push_back(j);
        rows.push_back(&j->row);
      }
    const double t0 = now_us();
    store.commit_group(rows);
    add_t(7, t0);
    for (RouteJob* j : fin) finish(j);
    done_all(fin);
  }
}

RouteService::RouteService(const RouteServiceCfg& cfg, std::function<void(RouteJob*)> done) : p_(new Impl) {
  p_->cfg = cfg;
  p_->done = std::move(done);
  if (cfg.provider == 1 && cfg.glat != nullptr) {
    p_->grid.build(cfg.glat, cfg.glon, (size_t)cfg.N, cfg.snap_c);
    const auto& shared = cfg.record_graph;
    if (shared && shared->ok() && shared->N == cfg.N && shared->glat == cfg.glat && shared->indptr == cfg.h_indptr &&
        shared->length == cfg.h_length) {
      p_->rg = shared;                 // the server's view of this same graph (its tables too)
    } else {
      p_->coord_cache.build(cfg.glat, cfg.glon, (size_t)cfg.N);
      if (cfg.h_indptr != nullptr && cfg.h_indices != nullptr) {
        const int64_t E = cfg.h_indptr[cfg.N];
        p_->edge_heading.resize((size_t)E);
        for (int u = 0; u < cfg.N; ++u)
          for (int32_t e = cfg.h_indptr[u]; e < cfg.h_indptr[u + 1]; ++e)
            p_->edge_heading[(size_t)e] = rtr::hop_heading(cfg.glat, cfg.glon, u, cfg.h_indices[e]);
      }
      if (cfg.h_length != nullptr && cfg.h_indptr != nullptr && cfg.h_indices != nullptr) {
        auto g = std::make_shared<rrec::RecordGraph>();
        const Impl* ip = p_;
        g->build(cfg.N, cfg.glat, cfg.glon, cfg.h_indptr, cfg.h_indices, cfg.h_length, cfg.h_edge_name,
                 &ip->cfg.names, &ip->coord_cache, ip->edge_heading.empty() ? nullptr : ip->edge_heading.data());
        if (g->ok()) p_->rg = g;
      }
    }
  }
  p_->th = std::thread([this] { p_->run(); });
}

RouteService::~RouteService() {
  {
    std::lock_guard<std::mutex> lk(p_->mu);
    p_->stop = true;
  }
  p_->cv.notify_all();
  if (p_->th.joinable()) p_->th.join();
  delete p_;
}

void RouteService::set_done_batch(std::function<void(std::vector<RouteJob*>&)> done_many) {
  p_->done_many = std::move(done_many);
}

bool RouteService::submit(RouteJob* j) {
  if (!j->parsed) {             // on the submitting reactor's thread: off the flush's critical path
    p_->n_jobs.fetch_add(1, std::memory_order_relaxed);
    Impl::parse_job(j);
  }
  // avoid areas, time windows: the app answers, no flush waits for this job
  if (j->req.avoid || j->req.time_windows) return false;
  {
    std::lock_guard<std::mutex> lk(p_->mu);
    if (p_->stop) return false;   // the run loop may have drained its queue already
    j->t_enq_us = now_us();
    p_->q.push_back(j);
  }
  p_->cv.notify_one();
  return true;
}

std::vector<long long> RouteService::stats() const {
  std::vector<long long> v = {p_->n_jobs.load(), p_->n_flushes.load(), p_->n_fallback.load(), p_->n_legs.load(),
                              p_->n_host_legs.load(), p_->store.rows_persisted()};
  for (int k = 0; k < 8; ++k) v.push_back(p_->t_stage[k].load());
  v.push_back(p_->n_escalated.load());     // A* searches rerun in the big tier
  v.push_back(p_->n_ctx_built.load());     // routing contexts customized by this service (CCH)
  v.push_back(p_->t_ctx_us.load());        // ... and their cost + customization time (us)
  v.push_back(p_->n_legs_reused.load());   // legs that reused their matrix chains (meet + unpack only)
  v.push_back(p_->n_deferred.load());      // jobs that waited for their context's background build
  v.push_back(p_->t_wait_us.load());       // ... their total wait (us)
  v.push_back(p_->n_prefetch.load());      // next-week-hour contexts queued ahead of time
  v.push_back(p_->n_failed_over.load());   // jobs handed to another GPU's route service
  v.push_back(p_->n_records.load());       // rows persisted as compact route records
  v.push_back(p_->n_record_bytes.load());  // ... and their record bytes
  v.push_back(p_->t_collect_us.load());    // GPU thread: collecting flushes (us)
  v.push_back(p_->t_handoff_us.load());    // GPU thread: waiting for the assembly queue (us)
  return v;
}

bool RouteService::broken() const { return p_->broken.load();
}

}  // namespace rt
