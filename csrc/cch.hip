// GPU customizable contraction hierarchy (SURVEY K9 "edge costs precomputed per (graph, context) and
// cached"): the router object.  The constructor uploads the host-built topology (csrc/runtime/cch.h)
// and picks the customization path (csrc/cch_customize.hip build_tables); customized metrics live in
// an LRU cache keyed by routing context, filled on demand (metric_for) or by background builder
// threads on their own low-priority, CU-masked streams (request_build).  Queries: csrc/cch_query.hip.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "cch_dev.h"
#include "cch_gpu.h"

namespace rt {

using namespace cchd;

CchMetricDev::~CchMetricDev() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(device);
  dfree(cost);
  dfree(sub_up);
  dfree(sub_dn);
  dfree(len_up);
  dfree(len_dn);
  dfree(cnt_up);
  dfree(cnt_dn);
  dfree(f_ptr);
  dfree(b_ptr);
  dfree(f_rec);
  dfree(b_rec);
  (void)hipSetDevice(cur);
}

CchGpu::CchGpu(rcch::Topology T, const float* length, const uint8_t* road_class, const uint8_t* base_traffic,
               int device)
    : T_(std::move(T)), dev_(device) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (hipSetDevice(dev_) != hipSuccess) throw std::runtime_error("CchGpu: bad device");
  const int N = T_.N;
  const int64_t M = T_.M, E = T_.E;
  if (M >= (int64_t)1 << 31 || E >= (int64_t)1 << 31) throw std::runtime_error("CchGpu: graph too large");
  std::vector<int32_t> up_ptr32(N + 1);
  for (int r = 0; r <= N; ++r) up_ptr32[r] = (int32_t)T_.up_ptr[r];
  // level work prefixes: basic items per node = k(k+1)/2 (k finalize + k(k-1)/2 pairs), height
  // order; perfect items = k(k-1), depth order
  bofs_.assign(N + 1, 0);
  pofs_.assign(N + 1, 0);
  aofs_.assign(N + 1, 0);
  for (int i = 0; i < N; ++i) {
    const int64_t kb = T_.up_ptr[T_.hlev_nodes[i] + 1] - T_.up_ptr[T_.hlev_nodes[i]];
    bofs_[i + 1] = bofs_[i] + kb * (kb + 1) / 2;
    const int64_t kp = T_.up_ptr[T_.dlev_nodes[i] + 1] - T_.up_ptr[T_.dlev_nodes[i]];
    pofs_[i + 1] = pofs_[i] + kp * (kp - 1);
    aofs_[i + 1] = aofs_[i] + kp;
  }
  plev_kmax_.assign((size_t)T_.max_depth + 1, 0);
  for (int d = 0; d <= T_.max_depth; ++d)
    for (int64_t i = T_.dlev_ptr[d]; i < T_.dlev_ptr[d + 1]; ++i) {
      const int x = T_.dlev_nodes[i];
      plev_kmax_[d] = std::max(plev_kmax_[d], (int)(T_.up_ptr[x + 1] - T_.up_ptr[x]));
    }
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t x) {
    if (x != hipSuccess && e == hipSuccess) e = x;
  };
  ck(up_copy(d_up_ptr, up_ptr32.data(), N + 1));
  ck(up_copy(d_up_head, T_.up_head.data(), M));
  ck(up_copy(d_arc_lo, T_.arc_lo.data(), M));
  ck(up_copy(d_parent, T_.parent.data(), N));
  ck(up_copy(d_depth, T_.depth.data(), N));
  ck(up_copy(d_rank, T_.rank.data(), N));
  ck(up_copy(d_node, T_.node.data(), N));
  ck(up_copy(d_edge_arc, T_.edge_arc.data(), E));
  ck(up_copy(d_edge_dir, T_.edge_dir.data(), E));
  ck(up_copy(d_length, length, E));
  if (road_class) ck(up_copy(d_class, road_class, E));
  if (base_traffic) ck(up_copy(d_base_traffic, base_traffic, E));
  ck(up_copy(d_hnodes, T_.hlev_nodes.data(), N));
  ck(up_copy(d_dnodes, T_.dlev_nodes.data(), N));
  {
    std::vector<int32_t> dlev32(T_.dlev_ptr.begin(), T_.dlev_ptr.end());
    ck(up_copy(d_dlev_ptr, dlev32.data(), dlev32.size()));
  }
  ck(up_copy(d_bofs, bofs_.data(), N + 1));
  ck(up_copy(d_pofs, pofs_.data(), N + 1));

  ck(alloc_scratch(cs0_));
  if (builder_max_wg_.load() < 0) builder_max_wg_.store(M >= 20000000LL ? 512 : 0);
  if (e == hipSuccess) build_tables();      // the accelerated customization, or the fallback
  (void)hipSetDevice(cur);
  if (e != hipSuccess) throw std::runtime_error(std::string("CchGpu: ") + hipGetErrorString(e));
  if (const char* gb = std::getenv("ROUTEST_CCH_CACHE_GB")) cache_gb_ = std::atof(gb);
}

CchGpu::~CchGpu() {
  {
    std::lock_guard<std::mutex> lk(bmu_);
    bstop_ = true;
    bq_.clear();
  }
  bcv_.notify_all();
  for (auto& t : bths_)
    if (t.joinable()) t.join();
  for (auto& x : bscr_) free_scratch(*x);
  {
    std::lock_guard<std::mutex> lk(mu_);
    cache_.clear();
  }
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(dev_);
  dfree(d_up_ptr);
  dfree(d_up_head);
  dfree(d_arc_lo);
  dfree(d_parent);
  dfree(d_depth);
  dfree(d_rank);
  dfree(d_node);
  dfree(d_edge_arc);
  dfree(d_edge_dir);
  dfree(d_length);
  dfree(d_class);
  dfree(d_base_traffic);
  dfree(d_hnodes);
  dfree(d_dnodes);
  dfree(d_dlev_ptr);
  dfree(d_bofs);
  dfree(d_pofs);
  free_tables();
  free_geometry();
  free_scratch(cs0_);
  (void)hipSetDevice(cur);
}

void CchGpu::set_eta(const void* blob, int H, const NormParams& np, int variant, int num_cus) {
  std::lock_guard<std::mutex> lk(mu_cust_);
  eta_blob_ = blob;
  eta_H_ = H;
  eta_np_ = np;
  eta_variant_ = variant;
  eta_cus_ = num_cus;
}

hipError_t CchGpu::metric_from_costs(uint64_t key, const float* d_cost, hipStream_t s,
                                     std::shared_ptr<CchMetricDev>& out) {
  auto m = std::make_shared<CchMetricDev>();
  m->key = key;
  hipError_t e = customize(d_cost, *m, s);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto it = cache_.begin(); it != cache_.end(); ++it)
      if ((*it)->key == key) {
        cache_.erase(it);
        break;
      }
  }
  insert_cached(m);
  out = m;
  return hipSuccess;
}

// device bytes of one customized metric (what the LRU budget is divided by)
static int64_t metric_device_bytes(const CchMetricDev& m, int64_t N, int64_t M, int64_t E) {
  return E * 4 + M * (8 + 8 + 4 + 4 + 4 + 4) + (N + 1) * 8 + (m.kept_f + m.kept_b) * 16;
}

void CchGpu::insert_cached(const std::shared_ptr<CchMetricDev>& m) {
  const int64_t b = metric_device_bytes(*m, T_.N, T_.M, T_.E);
  metric_bytes_.store(b);
  std::lock_guard<std::mutex> lk(mu_);
  if (cache_gb_ > 0.0 && b > 0) capacity_ = (int)std::max<int64_t>(4, (int64_t)(cache_gb_ * 1073741824.0 / (double)b));
  cache_.push_front(m);
  // metrics with avoid areas share a quarter of the slots: a client that sends a new polygon with
  // every request evicts its own metrics, not the week-hour contexts everyone uses
  if (m->avoid) {
    const int cap = std::max(1, capacity_ / 4);
    int n = 0;
    for (const auto& x : cache_) n += x->avoid != nullptr;
    for (auto it = cache_.end(); n > cap && it != cache_.begin();) {
      --it;
      if ((*it)->avoid) {
        it = cache_.erase(it);
        --n;
      }
    }
  }
  while ((int)cache_.size() > capacity_) cache_.pop_back();
}

static bool same_avoid(const std::shared_ptr<const std::vector<int32_t>>& a,
                       const std::shared_ptr<const std::vector<int32_t>>& b) {
  return a == b || (a && b && *a == *b);
}

bool CchGpu::avoid_clash(const CchContext& c) {
  const uint64_t key = c.key();
  std::lock_guard<std::mutex> lk(mu_);
  for (const auto& m : cache_)
    if (m->key == key) return !same_avoid(m->avoid, c.avoid);
  return false;
}

void CchGpu::set_cache_gb(double gb) {
  std::lock_guard<std::mutex> lk(mu_);
  cache_gb_ = gb > 0.0 ? gb : 0.0;
  const int64_t b = metric_bytes_.load();
  if (cache_gb_ > 0.0 && b > 0) capacity_ = (int)std::max<int64_t>(4, (int64_t)(cache_gb_ * 1073741824.0 / (double)b));
  while ((int)cache_.size() > capacity_) cache_.pop_back();
}

void CchGpu::request_build(const CchContext& c, bool urgent) {
  const uint64_t key = c.key();
  std::shared_ptr<CchMetricDev> m;
  if (cached_metric(key, m)) {
    notify_built(key, same_avoid(m->avoid, c.avoid));
    return;
  }
  {
    std::lock_guard<std::mutex> lk(bmu_);
    if (bstop_ || !bpending_.insert(key).second) return;   // stopping, or already queued / building
    if (urgent) bq_.push_front(c);
    else bq_.push_back(c);
    start_builders_locked();
  }
  n_bqueued_.fetch_add(1, std::memory_order_relaxed);
  bcv_.notify_one();
}

// ROUTEST_CCH_BUILDERS concurrent builders (default 3), each with its own temporaries: a
// customization is a chain of dependent level launches that keeps a fraction of the GPU busy, so a
// burst of fresh contexts builds several at a time.  (caller holds bmu_)
void CchGpu::start_builders_locked() {
  if (!bths_.empty() || bstop_) return;
  static const int nb = [] {
    const char* v = std::getenv("ROUTEST_CCH_BUILDERS");
    const int k = v ? std::atoi(v) : 3;
    return k < 1 ? 1 : (k > 8 ? 8 : k);
  }();
  for (int i = 0; i < nb; ++i) bths_.emplace_back([this, i] { builder_loop(i); });
}

// the builders and their temporaries (device + pinned host allocations) now — a route service
// calls this at startup, so no allocation happens on the GPU while flushes are in flight
void CchGpu::start_builders() {
  std::lock_guard<std::mutex> lk(bmu_);
  start_builders_locked();
}

int CchGpu::add_build_listener(std::function<void(uint64_t, bool)> cb) {
  std::lock_guard<std::mutex> lk(lmu_);
  listeners_.emplace_back(next_listener_, std::move(cb));
  return next_listener_++;
}

void CchGpu::remove_build_listener(int id) {
  std::lock_guard<std::mutex> lk(lmu_);
  for (auto it = listeners_.begin(); it != listeners_.end(); ++it)
    if (it->first == id) {
      listeners_.erase(it);
      break;
    }
}

void CchGpu::notify_built(uint64_t key, bool ok) {
  std::lock_guard<std::mutex> lk(lmu_);
  for (auto& l : listeners_) l.second(key, ok);
}

CchGpu::AsyncStats CchGpu::async_stats() {
  AsyncStats a;
  a.queued = n_bqueued_.load();
  a.built = n_bbuilt_.load();
  a.failed = n_bfailed_.load();
  a.build_ms = us_build_.load() / 1e3;
  a.alloc_ms = us_alloc_.load() / 1e3;
  a.hostcopy_ms = us_hostcopy_.load() / 1e3;
  a.paced = n_paced_.load();
  std::lock_guard<std::mutex> lk(bmu_);
  a.pending = (int)bpending_.size();
  return a;
}

void CchGpu::builder_loop(int idx) {
  (void)idx;
  if (hipSetDevice(dev_) != hipSuccess) return;
  CustScratch* xs = nullptr;                // this builder's temporaries (freed by the destructor)
  {
    auto x = std::make_unique<CustScratch>();
    if (alloc_scratch(*x) == hipSuccess) {
      xs = x.get();
      std::lock_guard<std::mutex> lk(bmu_);
      bscr_.push_back(std::move(x));
    } else {
      free_scratch(*x);
      (void)hipGetLastError();              // builds below share cs0_ (under mu_cust_)
    }
  }
  hipStream_t s = nullptr;
  // The builder's kernels run on one CU in every ROUTEST_CCH_BUILDER_CU_SHARE (default 4: 64 of
  // the 256, spread over every XCD): a stream priority only orders dispatch, and the wide leaf
  // levels of a 1M-node customization otherwise fill every CU while the flushes' query kernels
  // wait for slots.  The customization is latency-bound (one dependent level after another), so
  // a quarter of the CUs costs it little.  1: all CUs, lowest priority.
  static const int share = [] {
    const char* v = std::getenv("ROUTEST_CCH_BUILDER_CU_SHARE");
    const int k = v ? std::atoi(v) : 4;
    return k < 1 ? 1 : k;
  }();
  if (share > 1) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_) != hipSuccess || cus <= 0) cus = 256;
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int c = share - 1; c < cus; c += share) mask[(size_t)c / 32] |= 1u << (c % 32);
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
      (void)hipGetLastError();
      s = nullptr;
    }
  }
  if (s == nullptr) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
        hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) != hipSuccess) {
      (void)hipGetLastError();
      if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    }
  }
  while (true) {
    CchContext c;
    {
      std::unique_lock<std::mutex> lk(bmu_);
      bcv_.wait(lk, [&] { return bstop_ || !bq_.empty(); });
      if (bstop_) break;
      c = bq_.front();
      bq_.pop_front();
    }
    std::shared_ptr<CchMetricDev> m;
    bool fresh = false;
    const auto tb = std::chrono::steady_clock::now();
    const bool ok = s != nullptr && metric_for(c, s, m, &fresh, xs) == hipSuccess;
    if (ok && fresh && m) {
      us_build_.fetch_add((long long)(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tb).count()));
      us_alloc_.fetch_add((long long)(m->alloc_ms * 1e3));
      us_hostcopy_.fetch_add((long long)(m->hostcopy_ms * 1e3));
    }
    if (!ok) (void)hipGetLastError();
    (ok ? n_bbuilt_ : n_bfailed_).fetch_add(1, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> lk(bmu_);
      bpending_.erase(c.key());
    }
    notify_built(c.key(), ok);
  }
  if (s) (void)hipStreamDestroy(s);
}

bool CchGpu::cached_metric(uint64_t key, std::shared_ptr<CchMetricDev>& out) {
  std::lock_guard<std::mutex> lk(mu_);
  for (auto it = cache_.begin(); it != cache_.end(); ++it)
    if ((*it)->key == key) {
      out = *it;
      cache_.splice(cache_.begin(), cache_, it);
      return true;
    }
  return false;
}

hipError_t CchGpu::metric_for(const CchContext& c, hipStream_t s, std::shared_ptr<CchMetricDev>& out, bool* fresh,
                              CustScratch* cs) {
  const uint64_t key = c.key();
  if (fresh) *fresh = false;
  auto lookup = [&]() -> bool { return cached_metric(key, out); };
  // the key under another avoid set (equal digests): never that set's metric
  auto checked = [&]() -> hipError_t {
    if (same_avoid(out->avoid, c.avoid)) return hipSuccess;
    out.reset();
    return hipErrorInvalidValue;
  };
  if (lookup()) return checked();
  {
    // a context another caller is building: wait for it, then hit; different contexts build
    // concurrently (each caller on its own stream and temporaries)
    std::unique_lock<std::mutex> lk(mu_inflight_);
    cv_inflight_.wait(lk, [&] { return inflight_.count(key) == 0; });
    if (lookup()) return checked();
    inflight_.insert(key);
  }
  struct Done {
    CchGpu* g;
    uint64_t k;
    ~Done() {
      {
        std::lock_guard<std::mutex> lk(g->mu_inflight_);
        g->inflight_.erase(k);
      }
      g->cv_inflight_.notify_all();
    }
  } done{this, key};
  auto m = std::make_shared<CchMetricDev>();
  m->key = key;
  m->device = dev_;
  m->avoid = c.avoid;
  const auto ta = std::chrono::steady_clock::now();
  hipError_t e = dmalloc(m->cost, T_.E);
  m->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
  if (e != hipSuccess) return e;
  auto t0 = std::chrono::steady_clock::now();
  e = context_costs(c, m->cost, s, cs);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  m->cost_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  e = customize(m->cost, *m, s, cs);
  if (e != hipSuccess) return e;
  insert_cached(m);
  out = m;
  if (fresh) *fresh = true;
  return hipSuccess;
}

}  // namespace rt
