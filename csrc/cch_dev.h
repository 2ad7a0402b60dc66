// Helpers shared by the CCH translation units (csrc/cch.hip, cch_customize.hip, cch_query.hip):
// the packed (weight, middle) arc word, the arc lookup, and the device allocation wrappers.
// Internal: include only from those files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rt {
namespace cchd {

constexpr unsigned long long PACK_INF_D = 0x7F800000FFFFFFFFull;
constexpr uint32_t EDGE_FLAG_D = 0x80000000u;
constexpr float F_INF = __builtin_inff();

__device__ __forceinline__ unsigned long long packw(float w, uint32_t p) {
  return ((unsigned long long)__float_as_uint(w) << 32) | p;
}
__device__ __forceinline__ float wof(unsigned long long p) { return __uint_as_float((uint32_t)(p >> 32)); }

// position of b in the sorted upward list of a (a < b), -1 if absent
__device__ __forceinline__ int find_arc_d(const int32_t* __restrict__ up_ptr, const int32_t* __restrict__ up_head,
                                          int a, int b) {
  int lo = up_ptr[a], hi = up_ptr[a + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (up_head[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  return (lo < up_ptr[a + 1] && up_head[lo] == b) ? lo : -1;
}

inline int blocks_for(long long n, int b) { return (int)((n + b - 1) / b); }

template <class T>
hipError_t dmalloc(T*& p, size_t n) {
  p = nullptr;
  if (n == 0) n = 1;
  return hipMalloc((void**)&p, n * sizeof(T));
}
template <class T>
hipError_t up_copy(T*& p, const T* h, size_t n) {
  hipError_t e = dmalloc(p, n);
  if (e == hipSuccess && n) e = hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice);
  return e;
}
template <class T>
void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

}  // namespace cchd
}  // namespace rt
