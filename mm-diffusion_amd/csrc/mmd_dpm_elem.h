// The step core of the DPM-Solver kernels (mmd_dpm.hip; the slerp of mmd_diffusion.hip uses its quad_load / quad_store only), written once so that
// a fused launch writes the bits of the launches it replaces: mmd_lincomb's terms, mmd_clamp_scale's element, the geometry and address of
// the model output, the table row, the model value of an element and of a quad, the quad walk, the error term, the shared host checks.
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

// e of the adaptive pair's error norm sum e^2 (dpm:1088-1149): mmd_dpm_err's and mmd_dpm_adapt_close's element
__device__ __forceinline__ float dpm_err_term(float hi, float lo, float prev, float atol, float rtol) {
  const float delta = fmaxf(atol, rtol * fmaxf(fabsf(lo), fabsf(prev)));
  return (hi - lo) / delta;
}

// ----------------------------------------------------------------------------- geometry and table
// The state (x, M1, XB, ...) is fp32 [N, F, C, HW], the source of the model value fp32 [N, F, Cm, HW]: its first C channels are read.
// PRECONDITION of every kernel that takes a DpmGeom: Cm == C or 2C, which the entry point has checked with dpm_geom_ok.
struct DpmGeom {
  int N, F, C, Cm, HW;
  __device__ __forceinline__ int64_t per() const { return (int64_t)F * C * HW; }
};
// element r = (f, c, hw) of sample n in the source; Cm spelled as C or 2C saves registers (profiles/dpm_step_core.txt has the table)
__device__ __forceinline__ int64_t dpm_src_addr(const DpmGeom& g, int64_t n, int64_t r) {
  const int hw = (int)(r % g.HW), c = (int)((r / g.HW) % g.C);
  const int64_t f = r / ((int64_t)g.HW * g.C);
  const int Cm = g.C + (g.Cm > g.C ? g.C : 0);
  return ((n * g.F + f) * Cm + c) * (int64_t)g.HW + hw;
}

// tab: fp32 [slots][rows], k: the row of every sample.  Slots 0, 1: (cx, ce) of the data prediction cx x + ce eps; slots 2 ...: the update's
// coefficients in the order its entry point documents (include/mmd.h); the multistep and single-step tables keep the row's kind in slot 5.
struct DpmX0 { float cx, ce; };
struct DpmTab {
  const float* tab; const int64_t* k; int rows;
  // the row of sample n, or -1: the sample is not written (k outside [0, rows): a finished or masked-out sample)
  __device__ __forceinline__ int64_t row(int64_t n) const {
    const int64_t ki = k[n];
    return ki < 0 || ki >= rows ? -1 : ki;
  }
  __device__ __forceinline__ DpmX0 x0(int64_t ki) const { return {tab[ki], tab[rows + ki]}; }
  __device__ __forceinline__ float coef(int j, int64_t ki) const { return tab[(2 + j) * rows + ki]; }
  __device__ __forceinline__ int kind(int64_t ki) const { return (int)tab[5 * rows + ki]; }
};

// ----------------------------------------------------------------------------- the quad walk
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

// The cnt <= 4 consecutive elements r0 ... of sample n; i0 = n per + r0 is their offset in a [N, per] buffer.
struct DpmQuad {
  int64_t n, r0, i0; int cnt;
  // 16 bytes at once in a buffer that starts on 16 bytes (its alignment bit, dpm_vec_bits)
  __device__ __forceinline__ bool vec(bool on16) const { return cnt == 4 && on16 && !(i0 & 3); }
};
// the quad at r0 of sample n, cut at `end` (per, or the end of a workgroup's chunk)
__device__ __forceinline__ DpmQuad dpm_quad_at(int64_t n, int64_t r0, int64_t end, int64_t per) {
  return {n, r0, n * per + r0, end - r0 < 4 ? (int)(end - r0) : 4};
}
// unit u of a grid-stride kernel over ups = ceil(per / 4) quads a sample
__device__ __forceinline__ DpmQuad dpm_quad(int64_t u, int64_t ups, int64_t per) { return dpm_quad_at(u / ups, (u % ups) * 4, per, per); }

// ----------------------------------------------------------------------------- the model value
// Of one element, from raw = its value in the source (src[dpm_src_addr]).  X0FORM: m = cx x + ce eps (mmd_dpmpp_x0's value; xv = x
// there, k = the row's pair), else raw itself, clamp-scaled by sv = s[n] when thresholding is on (thr: s != NULL).
template <bool X0FORM>
__device__ __forceinline__ float dpm_model_value(float raw, float xv, const DpmX0& k, bool thr, float sv, float max_val) {
  if (X0FORM) return lincomb_add(lincomb_first(k.cx, xv), k.ce, raw);
  return thr ? clamp_scale_elem(raw, sv, max_val) : raw;
}
// Of a quad: the source moves as 16 bytes where the quad is whole, the source starts on 16 bytes (vsrc), the address is a multiple of 16
// and the quad stays inside one (frame, channel) row, else element by element.
template <bool X0FORM>
__device__ __forceinline__ void dpm_model_quad(const DpmGeom& g, const float* src, bool vsrc, const DpmQuad& q, const float* xv, const DpmX0& k,
                                               const float* __restrict__ s, float max_val, float* m) {
  const int64_t a0 = dpm_src_addr(g, q.n, q.r0);
  if (q.cnt == 4 && vsrc && !(a0 & 3) && (int)(q.r0 % g.HW) + 4 <= g.HW) {
    quad_load(src + a0, 4, true, m);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < q.cnt) m[j] = src[dpm_src_addr(g, q.n, q.r0 + j)];
  }
  if (!X0FORM && !s) return;
  const float sv = X0FORM ? 0.f : s[q.n];      // one load and one s_n / max_val for the quad
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = dpm_model_value<X0FORM>(m[j], xv[j], k, true, sv, max_val);
}

// ----------------------------------------------------------------------------- host checks
// the element counts and ranks of a sample are 32-bit in the tables
#define DPM_MAX_PER ((int64_t)1 << 31)

// [a, a + n) and [b, b + n) floats share no byte
static inline bool dpm_disjoint(const float* a, const float* b, int64_t n) {
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return ua + len <= ub || ub + len <= ua;
}
// no two of the n buffers of `total` floats share a byte
static inline bool dpm_all_disjoint(const float* const* b, int n, int64_t total) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (!dpm_disjoint(b[i], b[j], total)) return false;
  return true;
}
static inline bool on16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the kernels' `vec`: bit 0: all n state buffers start on 16 bytes, bit 1: the source of the model value does
static inline int dpm_vec_bits(const float* const* state, int n, const float* src) {
  int all = 1;
  for (int i = 0; i < n; ++i) all &= on16(state[i]) ? 1 : 0;
  return all | (on16(src) ? 2 : 0);
}
static inline int dpm_geom_ok(const char* what, int rows, int N, int F, int C, int Cm, int HW) {
  MMD_REQUIRE(rows > 0 && N > 0 && N <= 65535 && F > 0 && C > 0 && HW > 0, "%s: rows, N (<= 65535), F, C, HW must be positive", what);
  MMD_REQUIRE(Cm == C || Cm == 2 * C, "%s: the model output has C = %d or 2C channels; got %d", what, C, Cm);
  MMD_REQUIRE((int64_t)F * C * HW <= DPM_MAX_PER, "%s: sample too large", what);
  return MMD_OK;
}
static inline int dpm_form_ok(const char* what, int form, const float* s, float max_val) {
  MMD_REQUIRE(form == 0 || form == 1, "%s: form is 0 (the model value = the source) or 1 (= cx x + ce eps); got %d", what, form);
  MMD_REQUIRE(!s || form == 0, "%s: thresholding (s != NULL) goes with form 0 only: the quantile is taken of the stored x0raw", what);
  MMD_REQUIRE(!s || max_val > 0.f, "%s: max_val must be positive with thresholding (s != NULL)", what);
  return MMD_OK;
}
