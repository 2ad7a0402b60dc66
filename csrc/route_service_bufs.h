// Native route service (csrc/route_service*.hip): the flushes' queue-local copies and growable
// buffers.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "common.h"

namespace rt {

// Queue-local copies: the flush's host <-> device transfers run as a small kernel on the flush's own
// stream (mapped pinned host memory, read / written by the GPU over PCIe) instead of on the copy
// engines.  The SDMA queues are shared by every stream of the process: a copy queued behind a
// kernel that never finishes (a hung GPU slot; the watchdog rehearsal's gpu_hang hook) blocked the
// OTHER slot's copies behind it for the hang's whole duration (r6 trace: the healthy slot's matrix
// stage missed its 300 ms deadline waiting on its own tiny H2D copies).  On the compute queue a
// flush's copies wait only for its own stream.  16-byte vector body, byte tail; 2-D for the depot rows.
static __global__ __launch_bounds__(256) void route_copy_kernel(unsigned char* __restrict__ dst,
                                                                const unsigned char* __restrict__ src, size_t bytes) {
  const size_t nv = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0 ? bytes / 16 : 0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride)
    reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(src)[i];
  for (size_t i = nv * 16 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < bytes; i += stride) dst[i] = src[i];
}
static __global__ __launch_bounds__(256) void route_copy2d_kernel(unsigned char* __restrict__ dst, size_t dpitch,
                                                                  const unsigned char* __restrict__ src, size_t spitch,
                                                                  size_t width, size_t height) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < width * height; i += stride) {
    const size_t r = i / width, c = i - r * width;
    dst[r * dpitch + c] = src[r * spitch + c];
  }
}
inline std::atomic<bool>& qcopy_same_va() {
  static std::atomic<bool> ok{true};
  return ok;
}
inline hipError_t qcopy(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if (!qcopy_same_va().load(std::memory_order_relaxed)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s);
  const size_t blocks = std::min<size_t>(1024, (bytes / 16 + 255) / 256 + 1);
  hipLaunchKernelGGL(route_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (unsigned char*)dst,
                     (const unsigned char*)src, bytes);
  return hipGetLastError();
}
inline hipError_t qcopy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                          hipStream_t s) {
  if (width == 0 || height == 0) return hipSuccess;
  if (!qcopy_same_va().load(std::memory_order_relaxed))
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDefault, s);
  const size_t blocks = std::min<size_t>(1024, (width * height + 255) / 256);
  hipLaunchKernelGGL(route_copy2d_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (unsigned char*)dst, dpitch,
                     (const unsigned char*)src, spitch, width, height);
  return hipGetLastError();
}

// Growable buffers of the service's flushes.  A buffer outgrown while serving is not freed at
// once: hipFree / hipHostFree wait for the whole device, i.e. for every other service's and
// reactor's kernels on this GPU (a hung one included) — it is kept until the service ends (the
// geometric growth bounds the extra memory by the final size).
template <class T>
struct DevBuf {
  T* d = nullptr;
  size_t n = 0;
  std::vector<T*> old;
  hipError_t need(size_t k) {
    if (k <= n) return hipSuccess;
    const size_t m = std::max(k, n * 3 / 2);
    if (d) old.push_back(d);
    d = nullptr;
    n = 0;
    hipError_t e = hipMalloc((void**)&d, m * sizeof(T));
    if (e == hipSuccess) n = m;
    return e;
  }
  ~DevBuf() {
    if (d) (void)hipFree(d);
    for (T* p : old) (void)hipFree(p);
  }
};
template <class T>
struct HostBuf {
  T* h = nullptr;
  size_t n = 0;
  std::vector<T*> old;
  hipError_t need(size_t k) {
    if (k <= n) return hipSuccess;
    const size_t m = std::max(k, n * 3 / 2);
    if (h) old.push_back(h);
    h = nullptr;
    n = 0;
    hipError_t e = hipHostMalloc((void**)&h, m * sizeof(T), hipHostMallocMapped | hipHostMallocPortable);
    if (e == hipSuccess) {
      n = m;
      void* dp = nullptr;      // the GPU sees it at the same address (qcopy); else copies take the DMA path
      if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess || dp != (void*)h) qcopy_same_va().store(false);
    }
    return e;
  }
  ~HostBuf() {
    if (h) (void)hipHostFree(h);
    for (T* p : old) (void)hipHostFree(p);
  }
};

// Trip improvement (K6b, route_improve.hip) over the trip buffers' rows: the per-row flag going up,
// the four per-row statistics coming back with the trips.
struct ImproveBufs {
  HostBuf<unsigned char> h_flag;
  DevBuf<unsigned char> d_flag;
  HostBuf<int> h_moves, h_changed;
  DevBuf<int> d_moves, d_changed;
  HostBuf<long long> h_before, h_after;
  DevBuf<long long> d_before, d_after;
  // Trip exchange (K6c, route_exchange.hip) between two K6b launches: its own flag, its statistics,
  // and the second K6b launch's (which runs over the exchange rows only and so must not write the
  // first launch's buffers, where the improve-only rows' statistics live).
  HostBuf<unsigned char> h_xflag;
  DevBuf<unsigned char> d_xflag;
  HostBuf<int> h_xmoves, h_xtb, h_xta, h_moves2;
  DevBuf<int> d_xmoves, d_xrej, d_xtb, d_xta, d_moves2, d_changed2;
  HostBuf<long long> h_after2;
  DevBuf<long long> d_xbefore, d_xafter, d_before2, d_after2;
  bool reserve(size_t R) {
    return !(h_flag.need(R) || d_flag.need(R) || h_moves.need(R) || h_changed.need(R) || d_moves.need(R) ||
             d_changed.need(R) || h_before.need(R) || h_after.need(R) || d_before.need(R) || d_after.need(R) ||
             h_xflag.need(R) || d_xflag.need(R) || h_xmoves.need(R) || h_xtb.need(R) || h_xta.need(R) ||
             h_moves2.need(R) || d_xmoves.need(R) || d_xrej.need(R) || d_xtb.need(R) || d_xta.need(R) ||
             d_moves2.need(R) || d_changed2.need(R) || h_after2.need(R) || d_xbefore.need(R) || d_xafter.need(R) ||
             d_before2.need(R) || d_after2.need(R));
  }
};

}  // namespace rt
