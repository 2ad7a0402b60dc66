// ETA model objects of the native front end (csrc/native_model.h): the GPU launch per family, the
// owned weight copies that make a hot swap safe, and the fp32 CPU fallback forward.
#include <cmath>
#include <cstring>

#include "native_model.h"
#include "ops.h"

namespace rt {

ModelWs::~ModelWs() {
  if (p) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipFree(p);
    (void)hipSetDevice(cur);
  }
}

hipError_t ModelWs::need(int dev, size_t b) {
  if (p && device == dev && bytes >= b) return hipSuccess;
  if (p) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipFree(p);
    (void)hipSetDevice(cur);
    p = nullptr;
  }
  bytes = 0;
  device = dev;
  const size_t m = b < 4096 ? 4096 : b;
  hipError_t e = hipMalloc(&p, m);
  if (e == hipSuccess) bytes = m;
  return e;
}

namespace {

// device allocation owned by a model, freed on its device
struct DevOwned {
  void* p = nullptr;
  int device = 0;
  DevOwned() = default;
  DevOwned(const DevOwned&) = delete;
  ~DevOwned() {
    if (p) {
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(device);
      (void)hipFree(p);
      (void)hipSetDevice(cur);
    }
  }
  hipError_t copy_from(int dev, const void* src, size_t bytes, hipMemcpyKind kind) {
    device = dev;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(dev);
    hipError_t e = hipMalloc(&p, bytes ? bytes : 4);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, kind);
    (void)hipSetDevice(cur);
    return e;
  }
};

// K1 featurization of a 16-byte record (routest_amd/ops/eta_mlp.py featurize_torch)
inline void featurize(const rtc::EtaRecord& r, float x[12]) {
  for (int i = 0; i < 8; ++i) x[i] = 0.f;
  if (r.weather < 4) x[r.weather] = 1.f;
  if (r.traffic < 4) x[4 + r.traffic] = 1.f;
  const int64_t secs = r.wallclock_s;
  const int64_t days = secs >= 0 ? secs / 86400 : -((-secs + 86399) / 86400);
  const int64_t sod = secs - days * 86400;
  x[8] = (float)(((days + 2) % 7 + 7) % 7);
  x[9] = (float)(sod / 3600);
  x[10] = r.distance_m / 1000.0f;
  x[11] = r.driver_age;
}

bool mlp_cpu_batch(const MlpHost& m, const rtc::EtaRecord* rec, float* out, int B) {
  if (m.H <= 0) return false;
  for (int i = 0; i < B; ++i) out[i] = mlp_cpu_forward(m, rec[i]);
  return true;
}

struct Mlp3Model : NativeModel {
  DevOwned blob;
  NormParams np{};
  int variant = -1, cus = 256;
  MlpHost host;
  hipError_t predict(const void* rec, int rec_bytes, float* out, int B, hipStream_t s, ModelWs&) const override {
    return launch_eta_mlp3_fwd(rec, out, B, blob.p, H, np, variant, cus, s, rec_bytes);
  }
  const void* mlp3_blob() const override { return blob.p; }
  const NormParams* mlp3_norm() const override { return &np; }
  bool cpu_predict(const rtc::EtaRecord* rec, float* out, int B) const override { return mlp_cpu_batch(host, rec, out, B); }
  std::string describe() const override { return "mlp3 H=" + std::to_string(H); }
};

struct WideModel : NativeModel {
  DevOwned w1q, w2f, b2, w3;
  float b3 = 0.f;
  NormParams np{};
  MlpHost host;
  hipError_t predict(const void* rec, int rec_bytes, float* out, int B, hipStream_t s, ModelWs& ws) const override {
    const int parts = H / 64;
    hipError_t e = ws.need(device, (size_t)B * parts * sizeof(float));
    if (e != hipSuccess) return e;
    float* yp = (float*)ws.p;
    e = launch_big_fused(rec, rec_bytes, B, w1q.p, w2f.p, H, np, (const float*)b2.p, (const float*)w3.p, yp, s);
    if (e != hipSuccess) return e;
    return launch_big_yreduce(yp, parts, B, b3, nullptr, out, nullptr, 0.f, nullptr, nullptr, nullptr, s);
  }
  bool cpu_predict(const rtc::EtaRecord* rec, float* out, int B) const override { return mlp_cpu_batch(host, rec, out, B); }
  std::string describe() const override { return "mlp3-wide H=" + std::to_string(H); }
};

struct ForestModelN : NativeModel {
  DevOwned values, info, roots;
  ForestHost host;
  int fm[12];
  hipError_t predict(const void* rec, int rec_bytes, float* out, int B, hipStream_t s, ModelWs&) const override {
    if (rec_bytes != 16) return hipErrorInvalidValue;
    return launch_forest(rec, (const float*)values.p, (const unsigned*)info.p, (const int*)roots.p, out, B,
                         (int)host.roots.size(), (int)host.values.size(), host.base, host.le ? 1 : 0, fm, s);
  }
  bool takes_wire8() const override { return false; }
  bool cpu_predict(const rtc::EtaRecord* rec, float* out, int B) const override {
    const int T = (int)host.roots.size();
    for (int i = 0; i < B; ++i) {
      float x[12], xm[12];
      featurize(rec[i], x);
      for (int j = 0; j < 12; ++j) xm[j] = x[host.fmap[j]];
      double acc = host.base;
      for (int t = 0; t < T; ++t) {
        const int root = host.roots[t];
        int n = root;
        while (!(host.info[n] >> 31)) {
          const uint32_t inf = host.info[n];
          const float v = xm[(inf >> 24) & 63];
          const float thr = host.values[n];
          const bool left = std::isnan(v) ? ((inf >> 30) & 1) != 0 : (host.le ? v <= thr : v < thr);
          n = root + (int)(inf & 0xFFFFFF) + (left ? 0 : 1);
        }
        acc += host.values[n];
      }
      out[i] = (float)acc;
    }
    return true;
  }
  std::string describe() const override { return "forest trees=" + std::to_string(host.roots.size()); }
};

}  // namespace

float mlp_cpu_forward(const MlpHost& m, const rtc::EtaRecord& r) {
  float x[12];
  featurize(r, x);
  for (int j = 0; j < 12; ++j) x[j] = (x[j] - m.x_mean[j]) / m.x_std[j];
  const int H = m.H;
  std::vector<float> h1(H), h2(H);
  for (int u = 0; u < H; ++u) {
    float a = m.b1[u];
    const float* w = m.w1.data() + (size_t)u * 12;
    for (int j = 0; j < 12; ++j) a += w[j] * x[j];
    h1[u] = a > 0.f ? a : 0.f;
  }
  for (int u = 0; u < H; ++u) {
    float a = m.b2[u];
    const float* w = m.w2.data() + (size_t)u * H;
    for (int j = 0; j < H; ++j) a += w[j] * h1[j];
    h2[u] = a > 0.f ? a : 0.f;
  }
  float y = m.b3;
  for (int j = 0; j < H; ++j) y += m.w3[j] * h2[j];
  return y * m.y_std + m.y_mean;
}

std::shared_ptr<NativeModel> make_mlp3_model(int device, const void* blob, size_t blob_bytes, int H,
                                             const NormParams& np, int variant, int num_cus, MlpHost host,
                                             std::string& err) {
  auto m = std::make_shared<Mlp3Model>();
  m->kind = NativeModel::MLP3;
  m->device = device;
  m->H = H;
  m->np = np;
  m->variant = variant;
  m->cus = num_cus;
  m->host = std::move(host);
  if (m->blob.copy_from(device, blob, blob_bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
    err = "mlp3 blob copy failed";
    return nullptr;
  }
  return m;
}

std::shared_ptr<NativeModel> make_wide_model(int device, int H, const void* w1q, size_t w1q_bytes, const void* w2f,
                                             size_t w2f_bytes, const float* b2, const float* w3, float b3,
                                             const NormParams& np, MlpHost host, std::string& err) {
  if (H != 512 && H != 1024) {
    err = "wide model: H must be 512 or 1024";
    return nullptr;
  }
  auto m = std::make_shared<WideModel>();
  m->kind = NativeModel::WIDE;
  m->device = device;
  m->H = H;
  m->np = np;
  m->b3 = b3;
  m->host = std::move(host);
  if (m->w1q.copy_from(device, w1q, w1q_bytes, hipMemcpyDeviceToDevice) != hipSuccess ||
      m->w2f.copy_from(device, w2f, w2f_bytes, hipMemcpyDeviceToDevice) != hipSuccess ||
      m->b2.copy_from(device, b2, (size_t)H * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
      m->w3.copy_from(device, w3, (size_t)H * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
    err = "wide model weight copy failed";
    return nullptr;
  }
  return m;
}

constexpr int FOREST_MAX_DEPTH = 64;   // forest.hip: a walk takes at most 64 steps (`guard++ < 64`)

std::shared_ptr<NativeModel> make_forest_model(int device, ForestHost host, std::string& err) {
  const size_t M = host.values.size();
  if (M == 0 || host.info.size() != M || host.roots.empty() || host.roots[0] != 0) {
    err = "forest: malformed arrays";
    return nullptr;
  }
  for (size_t i = 1; i < host.roots.size(); ++i)
    if (host.roots[i] <= host.roots[i - 1] || (size_t)host.roots[i] >= M) {
      err = "forest: roots not increasing";
      return nullptr;
    }
  // every inner node's children inside the forest, features < 12 (forest.py validate)
  for (size_t t = 0; t < host.roots.size(); ++t) {
    const size_t b = (size_t)host.roots[t], e = t + 1 < host.roots.size() ? (size_t)host.roots[t + 1] : M;
    for (size_t n = b; n < e; ++n) {
      const uint32_t inf = host.info[n];
      if (inf >> 31) continue;
      if (((inf >> 24) & 63) >= 12 || b + (inf & 0xFFFFFF) + 1 >= e) {
        err = "forest: node reference out of range";
        return nullptr;
      }
    }
  }
  // at most FOREST_MAX_DEPTH inner nodes on a root-to-leaf path: the kernels stop a walk after that
  // many steps (forest.py validate).  Level k = the nodes a walk can stand on after k steps; a
  // cycle never empties the frontier and is refused as well.
  {
    std::vector<int> seen(M, -1);
    std::vector<uint32_t> cur, nxt;
    for (size_t t = 0; t < host.roots.size(); ++t) {
      const uint32_t b = (uint32_t)host.roots[t];
      cur.assign(1, b);
      for (int level = 0; !cur.empty(); ++level) {
        nxt.clear();
        for (uint32_t n : cur) {
          const uint32_t inf = host.info[n];
          if (inf >> 31) continue;
          if (level == FOREST_MAX_DEPTH) {
            err = "forest: tree " + std::to_string(t) + " is deeper than the kernels' depth limit of " +
                  std::to_string(FOREST_MAX_DEPTH) + " inner nodes on a root-to-leaf path";
            return nullptr;
          }
          for (uint32_t c = b + (inf & 0xFFFFFF), e = c + 2; c < e; ++c)
            if (seen[c] != level) {
              seen[c] = level;
              nxt.push_back(c);
            }
        }
        cur.swap(nxt);
      }
    }
  }
  for (int j = 0; j < 12; ++j)
    if (host.fmap[j] < 0 || host.fmap[j] >= 12) {
      err = "forest: feature map out of range";
      return nullptr;
    }
  auto m = std::make_shared<ForestModelN>();
  m->kind = NativeModel::FOREST;
  m->device = device;
  m->H = 0;
  for (int j = 0; j < 12; ++j) m->fm[j] = host.fmap[j];
  if (m->values.copy_from(device, host.values.data(), M * 4, hipMemcpyHostToDevice) != hipSuccess ||
      m->info.copy_from(device, host.info.data(), M * 4, hipMemcpyHostToDevice) != hipSuccess ||
      m->roots.copy_from(device, host.roots.data(), host.roots.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    err = "forest copy failed";
    return nullptr;
  }
  m->host = std::move(host);
  return m;
}

}  // namespace rt
