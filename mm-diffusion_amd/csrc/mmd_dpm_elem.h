// The element helpers the DPM-Solver kernels of mmd_diffusion.hip and mmd_adapt.hip share, so that a fused launch writes the bits of
// the launches it replaces: the terms of mmd_lincomb, the element of mmd_clamp_scale, a thread's quad of consecutive floats, and the
// overlap / alignment tests of their argument checks.
#pragma once
#include "mmd_common.h"

// The terms of out = ca a + cb b + cc c (mmd_lincomb), shared with the graph step's kernels (dpmpp_x0_kernel, dpmpp_update_kernel, ...)
// so that all write the same bits: lincomb_kernel has always compiled to a rounded ca a and one fused multiply-add per further term, and
// that form is spelled out here (its device code is unchanged by it).  A term that is absent is not added: -0 + 0 * c is +0.
__device__ __forceinline__ float lincomb_first(float ca, float a) { return ca * a; }
__device__ __forceinline__ float lincomb_add(float v, float c, float t) { return fmaf(c, t, v); }

// x = clamp(x, -s_n, s_n) / (s_n / max_val),  s_n = max(s, 1): one element of mmd_clamp_scale
__device__ __forceinline__ float clamp_scale_elem(float v, float s, float max_val) {
  const float sn = fmaxf(s, 1.f);
  return fminf(fmaxf(v, -sn), sn) / (sn / max_val);
}

// A thread's quad: 16 bytes at once (vec: the quad is whole and its address a multiple of 16), else its cnt elements one by one
__device__ __forceinline__ void quad_load(const float* p, int cnt, bool vec, float* v) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) v[j] = p[j];
  }
}
__device__ __forceinline__ void quad_store(float* p, int cnt, bool vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[j] = v[j];
  }
}
__device__ __forceinline__ bool quad_on16(const float* p, int cnt) { return cnt == 4 && ((uintptr_t)p & 15) == 0; }

// [a, a + n) and [b, b + n) floats share no byte
static inline bool dpm_disjoint(const float* a, const float* b, int64_t n) {
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return ua + len <= ub || ub + len <= ua;
}
static inline bool on16(const void* p) { return ((uintptr_t)p & 15) == 0; }
