// The fp32 per-polygon Newell geometry of tnp_polygon_report
// (include/tropical_hip.h), shared by polygons.hip and topology.hip so that
// both give a polygon's area the same bits.  Included by those two files only
// (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// sum += x with the rounding error carried in comp (no fast-math: the
// compiler keeps the order)
__device__ __forceinline__ void kahan_add(float& sum, float& comp, float x) {
  const float y = x - comp;
  const float t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}

// fp32 Newell about the members' mean c of polygon idx[a, b):
// N = 1/2 sum (p_i - c) x (p_i+1 - c); returns the area |N|.  One thread
// walks the members in order (degrees are 3..20 on the extracted surfaces;
// any degree works).
__device__ __forceinline__ float newell_area(const float* __restrict__ xyz, const int64_t* __restrict__ idx, int64_t a,
                                             int64_t b, float c[3], float N[3]) {
  // both sums are compensated (Kahan): a plain fp32 running sum over a
  // 200-gon's members drifts by several ulp of the result, more than the
  // formula's own rounding
  float cc[3] = {0.f, 0.f, 0.f}, Nc[3] = {0.f, 0.f, 0.f};
  c[0] = c[1] = c[2] = 0.f;
  for (int64_t i = a; i < b; ++i) {
    const float* q = xyz + 3 * idx[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) kahan_add(c[k], cc[k], q[k]);
  }
  const float m = (float)(b - a);
  c[0] /= m, c[1] /= m, c[2] /= m;
  N[0] = N[1] = N[2] = 0.f;
  const float* q0 = xyz + 3 * idx[b - 1];
  float u[3] = {q0[0] - c[0], q0[1] - c[1], q0[2] - c[2]};  // the edge (last, first) comes first
  for (int64_t i = a; i < b; ++i) {
    const float* q = xyz + 3 * idx[i];
    const float v[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
    kahan_add(N[0], Nc[0], u[1] * v[2] - u[2] * v[1]);
    kahan_add(N[1], Nc[1], u[2] * v[0] - u[0] * v[2]);
    kahan_add(N[2], Nc[2], u[0] * v[1] - u[1] * v[0]);
    u[0] = v[0], u[1] = v[1], u[2] = v[2];
  }
  N[0] *= 0.5f, N[1] *= 0.5f, N[2] *= 0.5f;
  return sqrtf(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
}

}  // namespace
