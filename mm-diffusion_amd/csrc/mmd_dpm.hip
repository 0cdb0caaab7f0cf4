// The DPM-Solver kernels on API-layout fp32 tensors: dynamic thresholding (quantile selection, clamp-scale), the adaptive pair's error
// norm, and the step kernels of the graph-replayed loops: multistep (mmd_dpmpp_*), single-step (mmd_dpm_single_update), stochastic
// (mmd_dpmpp_sde_update*), adaptive (mmd_dpm_adapt_open / _close / _commit; controller: mmd_adapt.hip).  Each reads its coefficients by
// the row k[n] of a device table and is built on the step core of mmd_dpm_elem.h, so it writes the bits of the launches it replaces.
#include "mmd_dpm_elem.h"
#include "mmd_ctr.h"

// ----------------------------------------------------------------------------- DPM-Solver helpers
// Dynamic thresholding of the x0 prediction (multimodal_dpm_solver_plus.py:419-440): per sample, s = the p-quantile of
// |x0| (torch.quantile 'linear' interpolation), s = max(s, 1), x0 = clamp(x0, -s, s) / (s / max_val).
// Exact selection: |x| as IEEE bits is order-preserving for non-negative floats -> 4 passes of an 8-bit radix select per
// wanted rank; one 1024-thread block per sample.
__device__ __forceinline__ uint32_t absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__device__ uint32_t radix_select_block(const float* __restrict__ x, int64_t n, int64_t rank, uint32_t* hist, int tid, int nth) {
  uint32_t prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += nth) hist[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += nth) {
      const uint32_t b = absbits(x[i]);
      if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
    }
    __syncthreads();
    // every thread walks the 256 bins (uniform result, no extra broadcast)
    int64_t r = rank;
    uint32_t digit = 0;
    for (int d = 0; d < 256; ++d) {
      const uint32_t c = hist[d];
      if (r < (int64_t)c) { digit = (uint32_t)d; break; }
      r -= c;
    }
    rank = r;
    prefix |= digit << shift;
    mask |= 255u << shift;
    __syncthreads();
  }
  return prefix;
}

// The two neighbouring ranks of torch.quantile(..., 'linear') among `per` values and the weight between them, and the interpolation:
// shared with the multi-workgroup selection (dpmpp_select_final_kernel), which therefore returns the same bits.
struct QuantileRanks { int64_t lo, hi; float frac; };
__device__ __forceinline__ QuantileRanks quantile_ranks(int64_t per, float q) {
  const double pos = (double)q * (double)(per - 1);
  const int64_t lo = (int64_t)floor(pos);
  const int64_t hi = lo + 1 < per ? lo + 1 : lo;
  return {lo, hi, (float)(pos - (double)lo)};
}
// vlo + (vhi - vlo) frac; torch.lerp(lo, hi, frac) for frac < 0.5 and its mirror agree to 1 ulp
__device__ __forceinline__ float quantile_lerp(float vlo, float vhi, float frac) { return fmaf(vhi - vlo, frac, vlo); }

__global__ __launch_bounds__(1024) void abs_quantile_kernel(const float* __restrict__ x, int64_t per, float q, float* __restrict__ out) {
  __shared__ uint32_t hist[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* xs = x + (int64_t)n * per;
  const QuantileRanks r = quantile_ranks(per, q);
  const float vlo = __uint_as_float(radix_select_block(xs, per, r.lo, hist, tid, blockDim.x));
  const float vhi = r.hi == r.lo ? vlo : __uint_as_float(radix_select_block(xs, per, r.hi, hist, tid, blockDim.x));
  if (tid == 0) out[n] = quantile_lerp(vlo, vhi, r.frac);
}
extern "C" int mmd_abs_quantile(const float* x, int N, int64_t per_sample, float q, float* out, void* stream) {
  MMD_REQUIRE(x && out && N > 0 && per_sample > 0 && q >= 0.f && q <= 1.f, "abs_quantile: bad argument");
  return mmd_launch<abs_quantile_kernel>("abs_quantile", dim3(N), dim3(1024), 0, (hipStream_t)stream, x, per_sample, q, out);
}

// x[n, :] = clamp(x, -s_n, s_n) / (s_n / max_val),  s_n = max(s[n], 1)        (in place)
// one element of it: clamp_scale_elem (mmd_dpm_elem.h), shared with the update kernels
__global__ __launch_bounds__(256) void clamp_scale_kernel(float* __restrict__ x, const float* __restrict__ s, float max_val, int64_t per,
                                                          int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float sv = s[i / per];
    x[i] = clamp_scale_elem(x[i], sv, max_val);
  }
}
extern "C" int mmd_clamp_scale(float* x, const float* s, float max_val, int N, int64_t per_sample, void* stream) {
  MMD_REQUIRE(x && s && N > 0 && per_sample > 0 && max_val > 0.f, "clamp_scale: bad argument");
  const int64_t total = per_sample * N;
  return mmd_launch<clamp_scale_kernel>("clamp_scale", dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x, s, max_val, per_sample, total);
}

// Adaptive step-size error term (dpm:1088-1149): out[n] += sum_i ((hi - lo) / max(atol, rtol * max(|lo|, |prev|)))^2
// (caller zeroes out and takes sqrt(out / per)).  One block per sample: thread t sums the elements t, t + 256, ... in ascending order in
// double, then the fixed tree over the 256 threads, and thread 0 alone adds the total to out[n] - no atomic, so the sum does not depend
// on the order in which blocks retire and is bitwise repeatable for every sample size.  The kernel runs once per adaptive step next to
// a network evaluation; a sample of 2 * 10^5 elements is 768 trips of the loop.
__global__ __launch_bounds__(256) void dpm_err_kernel(const float* __restrict__ hi, const float* __restrict__ lo, const float* __restrict__ prev,
                                                      float atol, float rtol, int64_t per, double* __restrict__ out) {
  __shared__ double red[256];
  const int n = blockIdx.x;
  const int64_t base = (int64_t)n * per;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < per; i += 256) {
    const float e = dpm_err_term(hi[base + i], lo[base + i], prev[base + i], atol, rtol);
    acc += (double)e * (double)e;
  }
  red[threadIdx.x] = acc;
  block_tree_sum256(threadIdx.x, red);
  if (threadIdx.x == 0) out[n] += red[0];
}
extern "C" int mmd_dpm_err(const float* hi, const float* lo, const float* prev, float atol, float rtol, int N, int64_t per_sample,
                           double* out, void* stream) {
  MMD_REQUIRE(hi && lo && prev && out && N > 0 && per_sample > 0, "dpm_err: bad argument");
  return mmd_launch<dpm_err_kernel>("dpm_err", dim3(N), dim3(256), 0, (hipStream_t)stream, hi, lo, prev, atol, rtol, per_sample, out);
}

// ----------------------------------------------------------------------------- DPM-Solver / DPM-Solver++ multistep step, graph form
// One evaluation of the fixed-grid multistep loop (DPM_Solver.sample(method="multistep"), dpm:1252-1283, with data_prediction_fn
// dpm:419-440, dpm_solver_first_update dpm:532-590 and multistep_dpm_solver_second_update dpm:889-947) without a host scalar: every
// coefficient comes from a device table indexed by the step number k[n] (int64 [N], like t of the other steppers), so a captured step
// bakes none in.  tab: fp32 [6][rows], rows = cx, ce (x0raw = cx x + ce eps), c0, c1, c2 (x = c0 x + c1 m0 + c2 m1) and the row's kind:
//   0 first order (m1 is not read)   1 second order   2 denoise (x = m0)
// One table per stream (the noise-prediction first-order step moves the audio stream with other coefficients, dpm:576-584).  A sample
// whose k is outside [0, rows) is not written.  Tensors are API layout as in the update kernels above: x / x0raw / M1 fp32 [N, F, C, HW],
// the model output fp32 [N, F, Cm, HW] with Cm = C or 2C (the first C channels are eps: learned-sigma outputs need no slicing copy).
#define DPMPP_CHUNK 4096            // elements of one sample per workgroup in the histogram passes
#define DPMPP_L0_BINS 2048          // level 0: the top 11 of the 31 magnitude bits
#define DPMPP_L_BINS 1024           // levels 1 and 2: 10 bits each, one table per wanted rank
#define DPMPP_WS_WORDS (DPMPP_L0_BINS + 4 * DPMPP_L_BINS)      // per sample: level 0, level 1 [2], level 2 [2]

// Level 0 of the selection, per workgroup: h = one 2048-bin table PER WAVE in LDS (activations sit in a handful of exponents, so one
// table for 256 threads would serialize on a few addresses), then the non-empty bins go to the sample's global table with integer
// atomicAdd - order-independent, so the table is deterministic.
__device__ __forceinline__ void l0_hist_zero(uint32_t* h, int tid) {
  for (int b = tid; b < 4 * DPMPP_L0_BINS; b += 256) h[b] = 0;
  __syncthreads();
}
__device__ __forceinline__ void l0_hist_add(uint32_t* h, int tid, float v) { atomicAdd(&h[(tid >> 6) * DPMPP_L0_BINS + (absbits(v) >> 20)], 1u); }
__device__ __forceinline__ void l0_hist_flush(const uint32_t* h, int tid, uint32_t* g) {
  __syncthreads();
  for (int b = tid; b < DPMPP_L0_BINS; b += 256) {
    const uint32_t c = h[b] + h[DPMPP_L0_BINS + b] + h[2 * DPMPP_L0_BINS + b] + h[3 * DPMPP_L0_BINS + b];
    if (c) atomicAdd(g + b, c);
  }
}

// x0raw = cx[k] x + ce[k] eps (data_prediction_fn before its thresholding); HIST: the same pass builds level 0 of |x0raw|
template <bool HIST>
__global__ __launch_bounds__(256) void dpmpp_x0_kernel(const DpmGeom g, const DpmTab t, const float* x, const float* mo, float* __restrict__ x0raw,
                                                       uint32_t* ws) {
  __shared__ uint32_t h[HIST ? 4 * DPMPP_L0_BINS : 1];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int64_t per = g.per();
  const int64_t ki = t.row(n);
  if (ki < 0) return;          // uniform over the workgroup
  const DpmX0 k0 = t.x0(ki);
  if (HIST) l0_hist_zero(h, tid);
  const int64_t lo = (int64_t)blockIdx.x * DPMPP_CHUNK, hi = lo + DPMPP_CHUNK < per ? lo + DPMPP_CHUNK : per;
  for (int64_t r = lo + tid; r < hi; r += 256) {
    const int64_t i = n * per + r;
    const float v = dpm_model_value<true>(mo[dpm_src_addr(g, n, r)], x[i], k0, false, 0.f, 0.f);
    x0raw[i] = v;
    if (HIST) l0_hist_add(h, tid, v);
  }
  if (HIST) l0_hist_flush(h, tid, ws + (int64_t)n * DPMPP_WS_WORDS);
}

// The bin of hist[NB] that holds rank `rank` (0-based, in ascending bin order) and the rank inside that bin; every thread of the 256
// returns the same pair.  sm: 8 words of LDS.  A rank past the table's total (a workspace that was not zero) leaves (0, 0).
template <int NB>
__device__ __forceinline__ void find_bin(const uint32_t* hist, uint32_t rank, uint32_t* sm, int tid, uint32_t& bin, uint32_t& rem) {
  constexpr int PT = NB / 256;
  uint32_t c[PT], sum = 0;
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    c[j] = hist[tid * PT + j];
    sum += c[j];
  }
  uint32_t inc = sum;                       // inclusive scan over the wave, then over the four waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, 64);
    if ((tid & 63) >= o) inc += v;
  }
  __syncthreads();                          // the previous call's readers are done with sm
  if ((tid & 63) == 63) sm[tid >> 6] = inc;
  if (tid == 0) sm[4] = sm[5] = 0;
  __syncthreads();
  uint32_t exc = inc - sum;
  for (int w = 0; w < (tid >> 6); ++w) exc += sm[w];
  __syncthreads();
  if (rank >= exc && rank - exc < sum) {    // exactly one thread
    uint32_t r = rank - exc, b = 0;
    bool done = false;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      if (!done) {
        if (r < c[j]) { b = j; done = true; }
        else r -= c[j];
      }
    }
    sm[4] = tid * PT + b;
    sm[5] = r;
  }
  __syncthreads();
  bin = sm[4];
  rem = sm[5];
}
// The magnitude-bit prefix of rank `rank` of sample table w after LEVELS levels (1: 11 bits, 2: 21, 3: all 31) and the rank left
// inside it; e = 0 / 1: the lower / upper of the two wanted ranks (levels 1 and 2 keep one table each).
template <int LEVELS>
__device__ __forceinline__ uint32_t select_prefix(const uint32_t* w, int e, uint32_t rank, uint32_t* sm, int tid) {
  uint32_t b, r;
  find_bin<DPMPP_L0_BINS>(w, rank, sm, tid, b, r);
  uint32_t pre = b;
  if (LEVELS >= 2) {
    find_bin<DPMPP_L_BINS>(w + DPMPP_L0_BINS + e * DPMPP_L_BINS, r, sm, tid, b, r);
    pre = (pre << 10) | b;
  }
  if (LEVELS >= 3) {
    find_bin<DPMPP_L_BINS>(w + DPMPP_L0_BINS + (2 + e) * DPMPP_L_BINS, r, sm, tid, b, r);
    pre = (pre << 10) | b;
  }
  return pre;
}

// One grid-wide histogram pass over x [N, per].  LEVEL 0: the top 11 magnitude bits of every element (what dpmpp_x0_kernel<true> fuses).
// LEVEL 1 / 2: every workgroup re-derives the 11- / 21-bit prefixes of the two wanted ranks from the tables of the levels before - no
// data-dependent buffer, no host read - and counts the next 10 bits of the elements under each prefix.
template <int LEVEL>
__global__ __launch_bounds__(256) void dpmpp_hist_kernel(const float* __restrict__ x, int64_t per, float q, uint32_t* ws) {
  __shared__ uint32_t h[LEVEL == 0 ? 4 * DPMPP_L0_BINS : 2 * DPMPP_L_BINS];
  __shared__ uint32_t sm[8];
  const int n = blockIdx.y, tid = threadIdx.x;
  uint32_t* w = ws + (int64_t)n * DPMPP_WS_WORDS;
  const float* xs = x + (int64_t)n * per;
  const int64_t lo = (int64_t)blockIdx.x * DPMPP_CHUNK, hi = lo + DPMPP_CHUNK < per ? lo + DPMPP_CHUNK : per;
  if (LEVEL == 0) {
    l0_hist_zero(h, tid);
    for (int64_t r = lo + tid; r < hi; r += 256) l0_hist_add(h, tid, xs[r]);
    l0_hist_flush(h, tid, w);
  } else {
    const QuantileRanks qr = quantile_ranks(per, q);
    const uint32_t pre0 = select_prefix<LEVEL>(w, 0, (uint32_t)qr.lo, sm, tid), pre1 = select_prefix<LEVEL>(w, 1, (uint32_t)qr.hi, sm, tid);
    constexpr int SHIFT = LEVEL == 1 ? 20 : 10;
    for (int b = tid; b < 2 * DPMPP_L_BINS; b += 256) h[b] = 0;
    __syncthreads();
    for (int64_t r = lo + tid; r < hi; r += 256) {
      const uint32_t b = absbits(xs[r]);
      const uint32_t d = (b >> (SHIFT - 10)) & (DPMPP_L_BINS - 1);
      if ((b >> SHIFT) == pre0) atomicAdd(&h[d], 1u);
      if ((b >> SHIFT) == pre1) atomicAdd(&h[DPMPP_L_BINS + d], 1u);
    }
    __syncthreads();
    uint32_t* g = w + DPMPP_L0_BINS + (LEVEL - 1) * 2 * DPMPP_L_BINS;
    for (int b = tid; b < 2 * DPMPP_L_BINS; b += 256)
      if (h[b]) atomicAdd(g + b, h[b]);
  }
}
// The last consumer: one workgroup per sample walks the three levels for both ranks, interpolates as abs_quantile_kernel does, and
// leaves the sample's tables zero for the next step.
__global__ __launch_bounds__(256) void dpmpp_select_final_kernel(int64_t per, float q, uint32_t* ws, float* __restrict__ out) {
  __shared__ uint32_t sm[8];
  const int n = blockIdx.x, tid = threadIdx.x;
  uint32_t* w = ws + (int64_t)n * DPMPP_WS_WORDS;
  const QuantileRanks qr = quantile_ranks(per, q);
  const float vlo = __uint_as_float(select_prefix<3>(w, 0, (uint32_t)qr.lo, sm, tid));
  const float vhi = __uint_as_float(select_prefix<3>(w, 1, (uint32_t)qr.hi, sm, tid));
  if (tid == 0) out[n] = quantile_lerp(vlo, vhi, qr.frac);
  __syncthreads();
  for (int b = tid; b < DPMPP_WS_WORDS; b += 256) w[b] = 0;
}

// x = c0[k] x + c1[k] m0 + c2[k] m1 in place, m0 = clamp_scale(m0src, s[n], max_val) (s == NULL: m0src itself), M1 = m0
__global__ __launch_bounds__(256) void dpmpp_update_kernel(const DpmGeom g, const DpmTab t, const float* src, float* x, float* M1,
                                                           const float* __restrict__ s, float max_val) {
  const int64_t per = g.per(), total = per * g.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const int64_t ki = t.row(n);
    if (ki < 0) continue;
    const float c0 = t.coef(0, ki), c1 = t.coef(1, ki), c2 = t.coef(2, ki);
    const int kind = t.kind(ki);
    const float m0 = dpm_model_value<false>(src[dpm_src_addr(g, n, i % per)], 0.f, DpmX0{}, s != nullptr, s ? s[n] : 0.f, max_val);
    float v;
    if (kind == 2) {
      v = m0;
    } else {
      v = lincomb_add(lincomb_first(c0, x[i]), c1, m0);
      if (kind == 1) v = lincomb_add(v, c2, M1[i]);
    }
    x[i] = v;
    M1[i] = m0;
  }
}

extern "C" int64_t mmd_dpmpp_workspace_bytes(int N) { return N > 0 ? (int64_t)N * DPMPP_WS_WORDS * sizeof(uint32_t) : 0; }

extern "C" int mmd_dpmpp_x0(const float* x, const float* model_out, float* x0raw, const float* tab, const int64_t* k, int rows, void* hist, int N,
                            int F, int C, int Cm, int HW, void* stream) {
  MMD_REQUIRE(x && model_out && x0raw && tab && k, "dpmpp_x0: needs x, the model output, x0raw, the table and the step numbers");
  if (int rc = dpm_geom_ok("dpmpp_x0", rows, N, F, C, Cm, HW)) return rc;
  const DpmGeom g{N, F, C, Cm, HW};
  const DpmTab t{tab, k, rows};
  const dim3 grid(cdiv((int64_t)F * C * HW, DPMPP_CHUNK), N);
  if (hist) return mmd_launch<dpmpp_x0_kernel<true>>("dpmpp_x0", grid, dim3(256), 0, (hipStream_t)stream, g, t, x, model_out, x0raw, (uint32_t*)hist);
  return mmd_launch<dpmpp_x0_kernel<false>>("dpmpp_x0", grid, dim3(256), 0, (hipStream_t)stream, g, t, x, model_out, x0raw, (uint32_t*)nullptr);
}

extern "C" int mmd_dpmpp_select(const float* x, void* workspace, int level0_done, int N, int64_t per_sample, float q, float* out, void* stream) {
  MMD_REQUIRE(x && workspace && out, "dpmpp_select: needs x, the workspace and out");
  MMD_REQUIRE(N > 0 && N <= 65535 && per_sample > 0 && per_sample <= DPM_MAX_PER, "dpmpp_select: N in [1, 65535], per_sample in [1, 2^31]");
  MMD_REQUIRE(q >= 0.f && q <= 1.f, "dpmpp_select: q must be in [0, 1]; got %g", (double)q);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* ws = (uint32_t*)workspace;
  const dim3 grid(cdiv(per_sample, DPMPP_CHUNK), N);
  int rc = MMD_OK;
  if (!level0_done) rc = mmd_launch<dpmpp_hist_kernel<0>>("dpmpp_select level 0", grid, dim3(256), 0, st, x, per_sample, q, ws);
  if (!rc) rc = mmd_launch<dpmpp_hist_kernel<1>>("dpmpp_select level 1", grid, dim3(256), 0, st, x, per_sample, q, ws);
  if (!rc) rc = mmd_launch<dpmpp_hist_kernel<2>>("dpmpp_select level 2", grid, dim3(256), 0, st, x, per_sample, q, ws);
  if (!rc) rc = mmd_launch<dpmpp_select_final_kernel>("dpmpp_select final", dim3(N), dim3(256), 0, st, per_sample, q, ws, out);
  return rc;
}

extern "C" int mmd_dpmpp_update(float* x, const float* m0, float* M1, const float* s, float max_val, const float* tab, const int64_t* k, int rows,
                                int N, int F, int C, int Cm, int HW, void* stream) {
  MMD_REQUIRE(x && m0 && M1 && tab && k, "dpmpp_update: needs x, m0, M1, the table and the step numbers");
  if (int rc = dpm_form_ok("dpmpp_update", 0, s, max_val)) return rc;
  if (int rc = dpm_geom_ok("dpmpp_update", rows, N, F, C, Cm, HW)) return rc;
  return mmd_launch<dpmpp_update_kernel>("dpmpp_update", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream,
                                         DpmGeom{N, F, C, Cm, HW}, DpmTab{tab, k, rows}, m0, x, M1, s, max_val);
}

// ----------------------------------------------------------------------------- DPM-Solver / DPM-Solver++ single-step step, graph form
// One evaluation of the single-step loop (DPM_Solver.sample(method="singlestep"), dpm:1277-1300, with dpm_solver_first_update
// dpm:532-590, singlestep_dpm_solver_second_update dpm:590-704 and singlestep_dpm_solver_third_update dpm:706-887) from the same tables:
// a step of order p is p evaluations, and every later stage combines the state and the model value at the START of the step with the
// newest model value, so the step keeps two histories, XB (the state there) and MS (the model value there).  The row's kind:
//   0 open (first evaluation of a step)  XB = x, MS = m0, x = c0 x + c1 m0     1 stage  x = c0 XB + c1 MS + c2 m0 (XB, MS kept)
//   2 denoise  x = m0 (XB, MS kept)
// X0FORM: m0 = cx x + ce eps in the kernel (the data prediction without thresholding: mmd_dpmpp_x0's value without its launch), else
// m0 = the source's first C channels, clamp-scaled by s[n] when s is given.
template <bool X0FORM>
__global__ __launch_bounds__(256) void dpm_single_update_kernel(const DpmGeom g, const DpmTab t, const float* src, float* x, float* XB, float* MS,
                                                                const float* __restrict__ s, float max_val) {
  const int64_t per = g.per(), total = per * g.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const int64_t ki = t.row(n);
    if (ki < 0) continue;
    const float c0 = t.coef(0, ki), c1 = t.coef(1, ki), c2 = t.coef(2, ki);
    const int kind = t.kind(ki);
    const int64_t a = dpm_src_addr(g, n, i % per);
    const float xv = x[i];
    const float m0 = dpm_model_value<X0FORM>(src[a], xv, t.x0(ki), s != nullptr, s ? s[n] : 0.f, max_val);
    if (kind == 0) {
      XB[i] = xv;
      MS[i] = m0;
      x[i] = lincomb_add(lincomb_first(c0, xv), c1, m0);
    } else if (kind == 1) {
      x[i] = lincomb_add(lincomb_add(lincomb_first(c0, XB[i]), c1, MS[i]), c2, m0);
    } else {
      x[i] = m0;
    }
  }
}

extern "C" int mmd_dpm_single_update(float* x, const float* src, int form, float* XB, float* MS, const float* s, float max_val, const float* tab,
                                     const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream) {
  MMD_REQUIRE(x && src && XB && MS && tab && k, "dpm_single_update: needs x, the source of m0, XB, MS, the table and the step numbers");
  MMD_REQUIRE(form == 0 || form == 1, "dpm_single_update: form is 0 (m0 = the source) or 1 (m0 = cx x + ce eps); got %d", form);      // its own wording
  if (int rc = dpm_form_ok("dpm_single_update", form, s, max_val)) return rc;
  if (int rc = dpm_geom_ok("dpm_single_update", rows, N, F, C, Cm, HW)) return rc;
  const int64_t total = (int64_t)N * F * C * HW;
  const float* bufs[3] = {x, XB, MS};
  MMD_REQUIRE(dpm_all_disjoint(bufs, 3, total),
              "dpm_single_update: XB and MS must overlap neither x nor each other (x is updated in place, the stages read both)");
  const DpmGeom g{N, F, C, Cm, HW};
  const DpmTab t{tab, k, rows};
  const dim3 grid(ew_grid(total));
  if (form == 1) return mmd_launch<dpm_single_update_kernel<true>>("dpm_single_update", grid, dim3(256), 0, (hipStream_t)stream, g, t, src, x, XB, MS, s, max_val);
  return mmd_launch<dpm_single_update_kernel<false>>("dpm_single_update", grid, dim3(256), 0, (hipStream_t)stream, g, t, src, x, XB, MS, s, max_val);
}

// ----------------------------------------------------------------------------- SDE-DPM-Solver++ multistep step, graph form
// One evaluation of the stochastic data-prediction multistep solver (Lu et al., DPM-Solver++ 2022, the "SDE-DPM-Solver++(2M)" update;
// DPM_Solver.sample_graph_sde) from mmd_dpmpp_update's table plus cz fp32 [rows], the noise coefficient of the row:
//   kind 0  x = c0 x + c1 m0 + cz z        1  x = c0 x + c1 m0 + c2 M1 + cz z        2  x = m0 (no noise is read or drawn)
// and M1 = m0.  mmd_lincomb's terms in that order, so the result is bitwise mmd_clamp_scale + mmd_lincomb(x, c0, m0, c1, M1, c2) +
// mmd_lincomb(v, 1, z, cz).  z = noise[i], or the counter normal of (element, draw = the low 32 bits of k[n], ids[n], tag): the value
// mmd_ctr_fill(draw = k) gives the element.  A thread owns one quad of consecutive elements of a sample in both forms; the quad moves as
// 16 bytes where it is whole and its address is a multiple of 16 (x, M1 and the noise share one offset; in the model output a quad is
// contiguous while it stays inside one (frame, channel) row), else element by element - a sample of 6147 elements has a ragged last
// quad and, from the second sample on, no aligned one.
struct DpmppSdeParams {
  float* x; const float* m0; float* M1; const float* s; const float* cz;
  float max_val;
  int vec;      // dpm_vec_bits of x, M1 (and the noise) and of the model output
};
struct SdeNoiseFromMemory {
  const float* noise;
  __device__ __forceinline__ void draw(const DpmQuad& q, uint32_t, bool vec, float* z) const { quad_load(noise + q.i0, q.cnt, vec, z); }
};
struct SdeNoiseFromCounter {
  CtrKey k;
  __device__ __forceinline__ void draw(const DpmQuad& q, uint32_t d, bool, float* z) const { ctr_normals(k, q.n, q.r0, d, z); }
};
template <class Src>
__global__ __launch_bounds__(256) void dpmpp_sde_update_kernel(const DpmGeom g, const DpmTab t, const DpmppSdeParams p, const Src src) {
  const int64_t per = g.per();
  const int64_t ups = (per + 3) / 4, total = ups * g.N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const DpmQuad q = dpm_quad(u, ups, per);
    const int64_t ki = t.row(q.n);
    if (ki < 0) continue;
    const float c0 = t.coef(0, ki), c1 = t.coef(1, ki), c2 = t.coef(2, ki), cz = p.cz[ki];
    const int kind = t.kind(ki);
    const bool vx = q.vec(p.vec & 1);
    float m0[4] = {}, v[4] = {}, m1[4] = {}, z[4] = {};
    dpm_model_quad<false>(g, p.m0, (p.vec & 2) != 0, q, v, DpmX0{}, p.s, p.max_val, m0);
    if (kind == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = m0[j];
    } else {
      quad_load(p.x + q.i0, q.cnt, vx, v);
      if (kind == 1) quad_load(p.M1 + q.i0, q.cnt, vx, m1);
      src.draw(q, (uint32_t)ki, vx, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float w = lincomb_add(lincomb_first(c0, v[j]), c1, m0[j]);
        if (kind == 1) w = lincomb_add(w, c2, m1[j]);
        v[j] = lincomb_add(w, cz, z[j]);
      }
    }
    quad_store(p.x + q.i0, q.cnt, vx, v);
    quad_store(p.M1 + q.i0, q.cnt, vx, m0);
  }
}

static int dpmpp_sde_args(const char* what, const float* x, const float* m0, const float* M1, const float* s, float max_val, const float* tab,
                          const float* cz, const int64_t* k, int rows, int N, int F, int C, int Cm, int HW) {
  MMD_REQUIRE(x && m0 && M1 && tab && k, "%s: needs x, m0, M1, the table and the step numbers", what);
  MMD_REQUIRE(cz, "%s: needs cz, the noise coefficient of every row", what);
  if (int rc = dpm_form_ok(what, 0, s, max_val)) return rc;
  return dpm_geom_ok(what, rows, N, F, C, Cm, HW);
}
extern "C" int mmd_dpmpp_sde_update(float* x, const float* m0, float* M1, const float* noise, const float* s, float max_val, const float* tab,
                                    const float* cz, const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream) {
  if (int rc = dpmpp_sde_args("dpmpp_sde_update", x, m0, M1, s, max_val, tab, cz, k, rows, N, F, C, Cm, HW)) return rc;
  MMD_REQUIRE(noise, "dpmpp_sde_update: needs the noise (the counter form draws it: mmd_dpmpp_sde_update_ctr)");
  const int64_t per = (int64_t)F * C * HW;
  const float* state[3] = {x, M1, noise};
  MMD_REQUIRE(dpm_all_disjoint(state, 3, per * N), "dpmpp_sde_update: x, M1 and noise must not overlap (x and M1 are written in place)");
  const DpmppSdeParams p{x, m0, M1, s, cz, max_val, dpm_vec_bits(state, 3, m0)};
  return mmd_launch<dpmpp_sde_update_kernel<SdeNoiseFromMemory>>("dpmpp_sde_update", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream,
                                                                 DpmGeom{N, F, C, Cm, HW}, DpmTab{tab, k, rows}, p, SdeNoiseFromMemory{noise});
}
extern "C" int mmd_dpmpp_sde_update_ctr(float* x, const float* m0, float* M1, const uint32_t* key, const int64_t* ids, int tag, const float* s,
                                        float max_val, const float* tab, const float* cz, const int64_t* k, int rows, int N, int F, int C, int Cm,
                                        int HW, void* stream) {
  if (int rc = dpmpp_sde_args("dpmpp_sde_update_ctr", x, m0, M1, s, max_val, tab, cz, k, rows, N, F, C, Cm, HW)) return rc;
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "dpmpp_sde_update_ctr: needs the key, the sample ids and a stream tag in [0, 3]");
  const int64_t per = (int64_t)F * C * HW;
  const float* state[2] = {x, M1};
  MMD_REQUIRE(dpm_all_disjoint(state, 2, per * N), "dpmpp_sde_update_ctr: x and M1 must not overlap (both are written in place)");
  const DpmppSdeParams p{x, m0, M1, s, cz, max_val, dpm_vec_bits(state, 2, m0)};
  return mmd_launch<dpmpp_sde_update_kernel<SdeNoiseFromCounter>>("dpmpp_sde_update_ctr", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream,
                                                                  DpmGeom{N, F, C, Cm, HW}, DpmTab{tab, k, rows}, p, SdeNoiseFromCounter{{key, ids, tag}});
}

// ----------------------------------------------------------------------------- the embedded pair of the adaptive loop
// The elementwise kernels of a trial step (mmd_adapt.hip's header has the loop and what each does).  Table slots: open (cx, ce, a0, a1,
// b0, b1), close (cx, ce, c0, c1, c2).
struct AdaptOpen {
  float* x; const float* src; float* XB; float* MS; float* LO; const float* s;
  float max_val;
  int vec;      // dpm_vec_bits of x, XB, MS, LO and of the source
};
template <bool X0FORM>
__global__ __launch_bounds__(256) void dpm_adapt_open_kernel(const DpmGeom g, const DpmTab t, const AdaptOpen p) {
  const int64_t per = g.per();
  const int64_t ups = (per + 3) / 4, total = ups * g.N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const DpmQuad q = dpm_quad(u, ups, per);
    const int64_t ki = t.row(q.n);
    if (ki < 0) continue;
    const DpmX0 k0 = t.x0(ki);
    const float a0 = t.coef(0, ki), a1 = t.coef(1, ki), b0 = t.coef(2, ki), b1 = t.coef(3, ki);
    const bool vx = q.vec(p.vec & 1);
    float xv[4] = {}, m0[4] = {}, lo[4], nx[4];
    quad_load(p.x + q.i0, q.cnt, vx, xv);
    dpm_model_quad<X0FORM>(g, p.src, (p.vec & 2) != 0, q, xv, k0, p.s, p.max_val, m0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo[j] = lincomb_add(lincomb_first(a0, xv[j]), a1, m0[j]);
      nx[j] = lincomb_add(lincomb_first(b0, xv[j]), b1, m0[j]);
    }
    quad_store(p.XB + q.i0, q.cnt, vx, xv);
    quad_store(p.MS + q.i0, q.cnt, vx, m0);
    quad_store(p.LO + q.i0, q.cnt, vx, lo);
    quad_store(p.x + q.i0, q.cnt, vx, nx);
  }
}

extern "C" int mmd_dpm_adapt_open(float* x, const float* src, int form, float* XB, float* MS, float* LO, const float* s, float max_val,
                                  const float* tab, const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream) {
  MMD_REQUIRE(x && src && XB && MS && LO && tab && k, "dpm_adapt_open: needs x, the source of m0, XB, MS, LO, the table and the row indices");
  if (int rc = dpm_form_ok("dpm_adapt_open", form, s, max_val)) return rc;
  if (int rc = dpm_geom_ok("dpm_adapt_open", rows, N, F, C, Cm, HW)) return rc;
  const int64_t per = (int64_t)F * C * HW, total = per * N;
  const float* bufs[4] = {x, XB, MS, LO};
  MMD_REQUIRE(dpm_all_disjoint(bufs, 4, total), "dpm_adapt_open: x, XB, MS and LO must not overlap (all four are written)");
  const DpmGeom g{N, F, C, Cm, HW};
  const DpmTab t{tab, k, rows};
  const AdaptOpen p{x, src, XB, MS, LO, s, max_val, dpm_vec_bits(bufs, 4, src)};
  const dim3 grid(ew_grid((per + 3) / 4 * N));
  if (form == 1) return mmd_launch<dpm_adapt_open_kernel<true>>("dpm_adapt_open", grid, dim3(256), 0, (hipStream_t)stream, g, t, p);
  return mmd_launch<dpm_adapt_open_kernel<false>>("dpm_adapt_open", grid, dim3(256), 0, (hipStream_t)stream, g, t, p);
}

// params: the controller's fp64 parameter block (MMD_ADAPT_P_*); the close kernel reads atol and rtol from it, rounded to fp32 - the
// values mmd_dpm_err takes as arguments - and sums mmd_dpm_err's term (dpm_err_term).
struct AdaptClose {
  float* x; const float* src; const float* XB; const float* MS; const float* LO; const float* PREV; const float* s;
  float max_val;
  int vec;      // dpm_vec_bits of x, XB, MS, LO, PREV and of the source
  const double* params; double* partial;
};
template <bool X0FORM>
__global__ __launch_bounds__(256) void dpm_adapt_close_kernel(const DpmGeom g, const DpmTab t, const AdaptClose p) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.y;
  const int64_t ki = t.row(n);
  if (ki < 0) return;          // uniform over the workgroup: a finished sample writes neither x nor its partial sums
  const int64_t per = g.per();
  const DpmX0 k0 = t.x0(ki);
  const float c0 = t.coef(0, ki), c1 = t.coef(1, ki), c2 = t.coef(2, ki);
  const float atol = (float)p.params[MMD_ADAPT_P_ATOL], rtol = (float)p.params[MMD_ADAPT_P_RTOL];
  const int64_t lo_r = (int64_t)blockIdx.x * MMD_DPM_ADAPT_CHUNK, hi_r = lo_r + MMD_DPM_ADAPT_CHUNK < per ? lo_r + MMD_DPM_ADAPT_CHUNK : per;
  double acc = 0.0;
  for (int64_t r0 = lo_r + (int64_t)tid * 4; r0 < hi_r; r0 += 256 * 4) {
    const DpmQuad q = dpm_quad_at(n, r0, hi_r, per);
    const bool vx = q.vec(p.vec & 1);
    float xv[4] = {}, xb[4] = {}, ms[4] = {}, lo[4] = {}, pv[4] = {}, m1[4] = {}, v[4];
    if (X0FORM) quad_load(p.x + q.i0, q.cnt, vx, xv);
    quad_load(p.XB + q.i0, q.cnt, vx, xb);
    quad_load(p.MS + q.i0, q.cnt, vx, ms);
    quad_load(p.LO + q.i0, q.cnt, vx, lo);
    quad_load(p.PREV + q.i0, q.cnt, vx, pv);
    dpm_model_quad<X0FORM>(g, p.src, (p.vec & 2) != 0, q, xv, k0, p.s, p.max_val, m1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = lincomb_add(lincomb_add(lincomb_first(c0, xb[j]), c1, ms[j]), c2, m1[j]);
      if (j < q.cnt) {      // ascending element order inside the thread
        const float e = dpm_err_term(v[j], lo[j], pv[j], atol, rtol);
        acc += (double)e * (double)e;
      }
    }
    quad_store(p.x + q.i0, q.cnt, vx, v);
  }
  red[tid] = acc;
  block_tree_sum256(tid, red);
  if (tid == 0) p.partial[n * gridDim.x + blockIdx.x] = red[0];
}

extern "C" int64_t mmd_dpm_adapt_chunks(int64_t per_sample) { return per_sample > 0 ? (per_sample + MMD_DPM_ADAPT_CHUNK - 1) / MMD_DPM_ADAPT_CHUNK : 0; }

extern "C" int mmd_dpm_adapt_close(float* x, const float* src, int form, const float* XB, const float* MS, const float* LO, const float* PREV,
                                   const float* s, float max_val, const float* tab, const int64_t* k, int rows, const double* params,
                                   double* partial, int N, int F, int C, int Cm, int HW, void* stream) {
  MMD_REQUIRE(x && src && XB && MS && LO && PREV && tab && k, "dpm_adapt_close: needs x, the source of m1, XB, MS, LO, PREV, the table and the row indices");
  MMD_REQUIRE(params && partial, "dpm_adapt_close: needs the parameter block and the partial sums [N, chunks]");
  if (int rc = dpm_form_ok("dpm_adapt_close", form, s, max_val)) return rc;
  if (int rc = dpm_geom_ok("dpm_adapt_close", rows, N, F, C, Cm, HW)) return rc;
  const int64_t per = (int64_t)F * C * HW, total = per * N;
  const float* bufs[5] = {x, XB, MS, LO, PREV};
  MMD_REQUIRE(dpm_all_disjoint(bufs, 5, total), "dpm_adapt_close: x, XB, MS, LO and PREV must not overlap (x is written while the others are read)");
  const DpmGeom g{N, F, C, Cm, HW};
  const DpmTab t{tab, k, rows};
  const AdaptClose p{x, src, XB, MS, LO, PREV, s, max_val, dpm_vec_bits(bufs, 5, src), params, partial};
  const dim3 grid((unsigned)mmd_dpm_adapt_chunks(per), N);
  if (form == 1) return mmd_launch<dpm_adapt_close_kernel<true>>("dpm_adapt_close", grid, dim3(256), 0, (hipStream_t)stream, g, t, p);
  return mmd_launch<dpm_adapt_close_kernel<false>>("dpm_adapt_close", grid, dim3(256), 0, (hipStream_t)stream, g, t, p);
}

__global__ __launch_bounds__(256) void dpm_adapt_commit_kernel(float* x, const float* __restrict__ XB, float* PREV, const float* __restrict__ LO,
                                                               const int32_t* __restrict__ cnt, int N, int64_t per, int vec) {
  const int64_t ups = (per + 3) / 4, total = ups * N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const DpmQuad q = dpm_quad(u, ups, per);
    const int flag = cnt[4 * q.n + MMD_ADAPT_C_FLAG];
    if (flag != MMD_ADAPT_FLAG_ACCEPT && flag != MMD_ADAPT_FLAG_REJECT) continue;
    const bool vx = q.vec(vec);
    float v[4] = {};
    if (flag == MMD_ADAPT_FLAG_ACCEPT) {
      quad_load(LO + q.i0, q.cnt, vx, v);
      quad_store(PREV + q.i0, q.cnt, vx, v);
    } else {
      quad_load(XB + q.i0, q.cnt, vx, v);
      quad_store(x + q.i0, q.cnt, vx, v);
    }
  }
}

extern "C" int mmd_dpm_adapt_commit(float* x, const float* XB, float* PREV, const float* LO, const int32_t* cnt, int N, int64_t per_sample,
                                    void* stream) {
  MMD_REQUIRE(x && XB && PREV && LO && cnt, "dpm_adapt_commit: needs x, XB, PREV, LO and the counters");
  MMD_REQUIRE(N > 0 && N <= 65535 && per_sample > 0 && per_sample <= DPM_MAX_PER, "dpm_adapt_commit: N in [1, 65535], per_sample in [1, 2^31]");
  const float* bufs[4] = {x, XB, PREV, LO};
  MMD_REQUIRE(dpm_all_disjoint(bufs, 4, per_sample * N), "dpm_adapt_commit: x, XB, PREV and LO must not overlap");
  const int vec = dpm_vec_bits(bufs, 4, nullptr) & 1;
  return mmd_launch<dpm_adapt_commit_kernel>("dpm_adapt_commit", dim3(ew_grid((per_sample + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream, x, XB,
                                             PREV, LO, cnt, N, per_sample, vec);
}
