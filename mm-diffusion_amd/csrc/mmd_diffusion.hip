// The diffusion process on API-layout fp32 tensors: the fused DDPM ancestral update (multimodal_gaussian_diffusion.py:231-343
// get_variance + 453-470 p_sample) and its backward, the DDIM step, q_sample, the coefficient combinations, the training-loss and
// variational-bound reductions with their gradients, and the slerp of two encoded latents.  (The DPM-Solver kernels: mmd_dpm.hip.)
#include "mmd_common.h"
#include "mmd_ctr.h"
#include "mmd_dpm_elem.h"      // lincomb's terms, a thread's quad (slerp), dpm_disjoint

// ----------------------------------------------------------------------------- the element core
// What every kernel of the process shares, written once.  tables: fp32 [7][T], rows = sqrt_recip_ac, sqrt_recipm1_ac, post_c1, post_c2,
// logvar_fixed, min_log (= the true posterior's clipped log-variance), max_log.  x (= x_t) and its like: fp32 [N, F, C, HW]; the model
// output: fp32 [N, F, Cm, HW] with Cm = C (fixed variance) or 2C (learned range: C mean channels, then C variance channels).
// flags bit0: clip x0 to [-1,1], bit1: model predicts x0, bit2: learned-range variance.
// The helpers take the arithmetic type R: float everywhere but in vlb_terms_kernel, which evaluates the fp32 data in double.  Each
// kernel reads the table rows where it needs them (a row nobody uses costs a load per element), in ascending row order.
struct DiffusionParams {
  const float* x; const float* mo; const float* tables; const int64_t* t;
  int T, N, F, C, HW, flags;
};
template <typename R>
__device__ __forceinline__ R table_row(const DiffusionParams& p, int row, int ti) { return p.tables[row * p.T + ti]; }
template <typename R> struct X0Coef { R cr, crm1; };                  // rows 0, 1: x0 from an eps prediction
template <typename R>
__device__ __forceinline__ X0Coef<R> x0_coef(const DiffusionParams& p, int ti) { return {table_row<R>(p, 0, ti), table_row<R>(p, 1, ti)}; }
template <typename R> struct PostCoef { R c1, c2; };                   // rows 2, 3: posterior mean
template <typename R>
__device__ __forceinline__ PostCoef<R> post_coef(const DiffusionParams& p, int ti) { return {table_row<R>(p, 2, ti), table_row<R>(p, 3, ti)}; }
template <typename R> struct RangeLogs { R min_log, max_log; };       // rows 5, 6: the ends of the learned range
template <typename R>
__device__ __forceinline__ RangeLogs<R> range_logs(const DiffusionParams& p, int ti) { return {table_row<R>(p, 5, ti), table_row<R>(p, 6, ti)}; }

// Element r = (f, c, hw) of sample n: the offsets of its mean channel and of its variance channel (flag 4) in the model output
struct ElemAddr { int64_t mean, var; };
__device__ __forceinline__ ElemAddr elem_addr(const DiffusionParams& p, int64_t n, int64_t r) {
  const int Cm = (p.flags & 4) ? 2 * p.C : p.C;
  const int hw = (int)(r % p.HW), c = (int)((r / p.HW) % p.C);
  const int64_t f = r / ((int64_t)p.HW * p.C);
  const int64_t mbase = ((n * p.F + f) * Cm) * (int64_t)p.HW + hw;
  return {mbase + (int64_t)c * p.HW, mbase + (int64_t)(c + p.C) * p.HW};
}

// learned-range log-variance (flag 4): the variance channel in [-1, 1] interpolates between min_log and max_log
template <typename R>
__device__ __forceinline__ R range_logvar(const DiffusionParams& p, const ElemAddr& a, const RangeLogs<R>& l) {
  const R vv = p.mo[a.var];
  const R frac = (vv + R(1)) / R(2);
  return frac * l.max_log + (R(1) - frac) * l.min_log;
}
// x0 prediction from the mean channel o: as the losses and gradients see it, and clamped (flag 1) as the samplers and the bound do
template <typename R>
__device__ __forceinline__ R pred_x0(const DiffusionParams& p, const X0Coef<R>& k, R o, R xv) { return (p.flags & 2) ? o : k.cr * xv - k.crm1 * o; }
template <typename R>
__device__ __forceinline__ R pred_x0_clamped(const DiffusionParams& p, const X0Coef<R>& k, R o, R xv) {
  R x0 = pred_x0(p, k, o, xv);
  if (p.flags & 1) x0 = fmin(fmax(x0, R(-1)), R(1));
  return x0;
}
// mean of q(x_{t-1} | x_t, x0): the model's with its x0 prediction, the true posterior's with the datum
template <typename R>
__device__ __forceinline__ R post_mean(const PostCoef<R>& q, R x0, R xv) { return q.c1 * x0 + q.c2 * xv; }

// ----------------------------------------------------------------------------- counter-based noise (the generator: mmd_ctr.h)
// Where an update kernel's noise comes from.  A thread owns W consecutive elements of one sample: one element with the noise in memory,
// one Philox quad with the counter source.  draw() fills z[0 .. W) for the elements r0 ... of sample n (i0 = n per + r0).
struct NoiseFromMemory {
  static constexpr int W = 1;
  const float* noise;
  __device__ __forceinline__ bool present() const { return noise != nullptr; }
  __device__ __forceinline__ void draw(int64_t, int64_t, int64_t i0, int, float* z) const { z[0] = noise[i0]; }
};
struct NoiseFromCounter {
  static constexpr int W = 4;
  CtrKey k;
  __device__ __forceinline__ bool present() const { return true; }
  __device__ __forceinline__ void draw(int64_t n, int64_t r0, int64_t, int ti, float* z) const { ctr_normals(k, n, r0, (uint32_t)ti, z); }
};
// The counter source with the draw handed in per sample (c1 = the low 32 bits of at[n]) instead of taken from the timestep: a loop that
// visits a timestep more than once (resampling jumps) gives every visit its own draw.
struct NoiseFromCounterAt {
  static constexpr int W = 4;
  CtrKey k;
  const int64_t* at;
  __device__ __forceinline__ bool present() const { return true; }
  __device__ __forceinline__ void draw(int64_t n, int64_t r0, int64_t, int, float* z) const { ctr_normals(k, n, r0, (uint32_t)at[n], z); }
};

// kind 0: fp32 normals, kind 1: the raw words; out [N, per]
template <int KIND>
__global__ __launch_bounds__(256) void ctr_fill_kernel(const CtrKey k, uint32_t draw, int64_t per, int N, void* out) {
  const int64_t ups = (per + 3) / 4, total = ups * N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t n = u / ups, r0 = (u % ups) * 4;
    const int64_t left = per - r0;
    uint32_t w[4];
    if (KIND == 0) {
      float z[4];
      ctr_normals(k, n, r0, draw, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = __float_as_uint(z[j]);
    } else {
      ctr_words(k, n, r0, draw, w);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < left) ((uint32_t*)out)[n * per + r0 + j] = w[j];
  }
}
// a sample's quads are counted in 32 bits
#define MMD_CTR_MAX_PER ((int64_t)1 << 34)

extern "C" int mmd_ctr_fill(void* out, int kind, const uint32_t* key, const int64_t* ids, int N, int64_t per_sample, uint32_t draw, int tag,
                            void* stream) {
  MMD_REQUIRE(out && ctr_args_ok(key, ids, tag) && N > 0 && per_sample > 0 && per_sample <= MMD_CTR_MAX_PER, "ctr_fill: bad argument");
  MMD_REQUIRE(kind == 0 || kind == 1, "ctr_fill: kind is 0 (fp32 normals) or 1 (uint32 words); got %d", kind);
  const CtrKey k{key, ids, tag};
  const dim3 grid(ew_grid((per_sample + 3) / 4 * N));
  if (kind == 0) return mmd_launch<ctr_fill_kernel<0>>("ctr_fill", grid, dim3(256), 0, (hipStream_t)stream, k, draw, per_sample, N, out);
  return mmd_launch<ctr_fill_kernel<1>>("ctr_fill", grid, dim3(256), 0, (hipStream_t)stream, k, draw, per_sample, N, out);
}

// ----------------------------------------------------------------------------- fused DDPM ancestral update
// out = mean + [t != 0] exp(logvar / 2) noise; x0_out / mean_out / logvar_out optional (p_mean_variance's results)
template <class Src>
__global__ __launch_bounds__(256) void ddpm_update_kernel(const DiffusionParams p, const Src src, float* out, float* x0_out, float* mean_out,
                                                          float* logvar_out) {
  constexpr int W = Src::W;
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int64_t ups = (per + W - 1) / W, total = ups * p.N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t n = u / ups, r0 = (u % ups) * W;
    const int ti = (int)p.t[n];
    const X0Coef<float> k = x0_coef<float>(p, ti);
    const PostCoef<float> q = post_coef<float>(p, ti);
    const float nz = ti != 0 ? 1.f : 0.f;
    float z[W] = {};
    if (out) src.draw(n, r0, n * per + r0, ti, z);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int64_t r = r0 + j, i = n * per + r;
      if (r >= per) break;
      const ElemAddr a = elem_addr(p, n, r);
      const float o = p.mo[a.mean];
      const float logvar = (p.flags & 4) ? range_logvar(p, a, range_logs<float>(p, ti)) : table_row<float>(p, 4, ti);
      const float xv = p.x[i];
      const float x0 = pred_x0_clamped(p, k, o, xv);
      const float mean = post_mean(q, x0, xv);
      if (out) out[i] = mean + nz * expf(0.5f * logvar) * z[j];
      if (x0_out) x0_out[i] = x0;
      if (mean_out) mean_out[i] = mean;
      if (logvar_out) logvar_out[i] = logvar;
    }
  }
}

extern "C" int mmd_ddpm_update(const float* x, const float* model_out, const float* noise, float* out, float* x0_out,
                               float* mean_out, float* logvar_out, const float* tables, const int64_t* t, int T, int N, int F,
                               int C, int HW, int flags, void* stream) {
  MMD_REQUIRE(x && model_out && tables && t && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "ddpm_update: bad argument");
  MMD_REQUIRE(!out || noise, "ddpm_update: sampling (out != NULL) needs noise");
  const DiffusionParams p{x, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<ddpm_update_kernel<NoiseFromMemory>>("ddpm_update", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream, p,
                                                         NoiseFromMemory{noise}, out, x0_out, mean_out, logvar_out);
}
extern "C" int mmd_ddpm_update_ctr(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out,
                                   float* x0_out, float* mean_out, float* logvar_out, const float* tables, const int64_t* t, int T, int N,
                                   int F, int C, int HW, int flags, void* stream) {
  MMD_REQUIRE(x && model_out && tables && t && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "ddpm_update_ctr: bad argument");
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "ddpm_update_ctr: needs the key, the sample ids and a stream tag in [0, 3]");
  const int64_t per = (int64_t)F * C * HW;
  MMD_REQUIRE(per <= MMD_CTR_MAX_PER, "ddpm_update_ctr: sample too large");
  const DiffusionParams p{x, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<ddpm_update_kernel<NoiseFromCounter>>("ddpm_update_ctr", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream, p,
                                                          NoiseFromCounter{{key, ids, tag}}, out, x0_out, mean_out, logvar_out);
}
extern "C" int mmd_ddpm_update_ctr_at(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out,
                                      float* x0_out, float* mean_out, float* logvar_out, const float* tables, const int64_t* t,
                                      const int64_t* draw, int T, int N, int F, int C, int HW, int flags, void* stream) {
  MMD_REQUIRE(x && model_out && tables && t && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "ddpm_update_ctr_at: bad argument");
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "ddpm_update_ctr_at: needs the key, the sample ids and a stream tag in [0, 3]");
  MMD_REQUIRE(draw, "ddpm_update_ctr_at: needs one draw per sample");
  const int64_t per = (int64_t)F * C * HW;
  MMD_REQUIRE(per <= MMD_CTR_MAX_PER, "ddpm_update_ctr_at: sample too large");
  const DiffusionParams p{x, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<ddpm_update_kernel<NoiseFromCounterAt>>("ddpm_update_ctr_at", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream,
                                                            p, NoiseFromCounterAt{{key, ids, tag}, draw}, out, x0_out, mean_out, logvar_out);
}

// Backward of the sampling update through the posterior mean (gradient-guided conditional sampling, gd:722-817):
//   sample = c1 clamp(x0) + c2 x + noise term,  x0 = cr x - crm1 eps  (or x0 = model output with flag 2)
//   dx = dsample (c1 cr [|x0| <= 1] + c2),  dmo = dsample (-c1 crm1 [|x0| <= 1])   (fixed variance only)
// Fixed variance means Cm = C: the model output is indexed like x, and the launcher passes the sample as one row (F = C = 1).
__global__ __launch_bounds__(256) void ddpm_update_bwd_kernel(const DiffusionParams p, const float* __restrict__ ds, float* __restrict__ dx,
                                                              float* __restrict__ dmo) {
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int64_t total = per * p.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ti = (int)p.t[i / per];
    const X0Coef<float> k = x0_coef<float>(p, ti);
    const PostCoef<float> q = post_coef<float>(p, ti);
    const float o = p.mo[i], xv = p.x[i], g = ds[i];
    const float x0 = pred_x0(p, k, o, xv);
    const float pass = (!(p.flags & 1) || (x0 >= -1.f && x0 <= 1.f)) ? 1.f : 0.f;
    if (dx) dx[i] = g * (((p.flags & 2) ? 0.f : q.c1 * k.cr * pass) + q.c2);
    if (dmo) dmo[i] = g * ((p.flags & 2) ? q.c1 * pass : -q.c1 * k.crm1 * pass);
  }
}
extern "C" int mmd_ddpm_update_bwd(const float* x, const float* model_out, const float* dsample, float* dx, float* dmodel_out,
                                   const float* tables, const int64_t* t, int T, int N, int64_t per_sample, int flags, void* stream) {
  MMD_REQUIRE(x && model_out && dsample && tables && t && T > 0 && N > 0 && per_sample > 0, "ddpm_update_bwd: bad argument");
  MMD_REQUIRE(!(flags & 4), "ddpm_update_bwd: learned variance is not differentiable here");
  const DiffusionParams p{x, model_out, tables, t, T, N, 1, 1, (int)per_sample, flags};
  return mmd_launch<ddpm_update_bwd_kernel>("ddpm_update_bwd", dim3(ew_grid((int64_t)N * per_sample)), dim3(256), 0, (hipStream_t)stream, p, dsample, dx,
                                            dmodel_out);
}

// ----------------------------------------------------------------------------- DDIM step / helper combinations
// ddim_sample (gd:821-901) and ddim_reverse_sample (gd:903-953) for one stream, API layout [N, F, Cm, HW]:
//   x0 = eps-or-x0 prediction (clamped with flag 1), eps = (sqrt_recip_ac x - x0) / sqrt_recipm1_ac,
//   sigma = eta sqrt((1-ac_prev)/(1-ac)) sqrt(1 - ac/ac_prev),
//   out = x0 sqrt(ac_prev) + sqrt(1 - ac_prev - sigma^2) eps + [t != 0] sigma noise          (flag 8: reverse ODE with ac_next, no noise)
// tab3 = [3][T] fp32: alphas_cumprod, alphas_cumprod_prev, alphas_cumprod_next.
// The noise of the forward step is read (or drawn) wherever a source is present; sigma == 0 (eta == 0) multiplies it away.
template <class Src>
__global__ __launch_bounds__(256) void ddim_update_kernel(const DiffusionParams p, const Src src, float* out, float* x0_out, const float* tab3,
                                                          float eta) {
  constexpr int W = Src::W;
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int64_t ups = (per + W - 1) / W, total = ups * p.N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t n = u / ups, r0 = (u % ups) * W;
    const int ti = (int)p.t[n];
    const X0Coef<float> k = x0_coef<float>(p, ti);
    float z[W] = {};
    if (!(p.flags & 8) && src.present()) src.draw(n, r0, n * per + r0, ti, z);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int64_t r = r0 + j, i = n * per + r;
      if (r >= per) break;
      const ElemAddr a = elem_addr(p, n, r);
      const float o = p.mo[a.mean];
      const float xv = p.x[i];
      const float x0 = pred_x0_clamped(p, k, o, xv);
      const float eps = (k.cr * xv - x0) / k.crm1;
      float res;
      if (p.flags & 8) {
        const float an = tab3[2 * p.T + ti];
        res = x0 * sqrtf(an) + sqrtf(1.f - an) * eps;
      } else {
        const float ab = tab3[ti], ap = tab3[p.T + ti];
        const float sigma = eta * sqrtf((1.f - ap) / (1.f - ab)) * sqrtf(1.f - ab / ap);
        const float mean = x0 * sqrtf(ap) + sqrtf(1.f - ap - sigma * sigma) * eps;
        const float nz = ti != 0 ? 1.f : 0.f;
        res = mean + nz * sigma * z[j];
      }
      if (out) out[i] = res;
      if (x0_out) x0_out[i] = x0;
    }
  }
}
extern "C" int mmd_ddim_update(const float* x, const float* model_out, const float* noise, float* out, float* x0_out,
                               const float* tables, const float* tab3, const int64_t* t, int T, int N, int F, int C, int HW,
                               int flags, float eta, void* stream) {
  MMD_REQUIRE(x && model_out && tables && tab3 && t && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "ddim_update: bad argument");
  MMD_REQUIRE((flags & 8) || eta == 0.f || noise, "ddim_update: eta > 0 needs noise");
  const DiffusionParams p{x, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<ddim_update_kernel<NoiseFromMemory>>("ddim_update", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream, p,
                                                         NoiseFromMemory{noise}, out, x0_out, tab3, eta);
}
extern "C" int mmd_ddim_update_ctr(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out,
                                   float* x0_out, const float* tables, const float* tab3, const int64_t* t, int T, int N, int F, int C,
                                   int HW, int flags, float eta, void* stream) {
  MMD_REQUIRE(x && model_out && tables && tab3 && t && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "ddim_update_ctr: bad argument");
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "ddim_update_ctr: needs the key, the sample ids and a stream tag in [0, 3]");
  const int64_t per = (int64_t)F * C * HW;
  MMD_REQUIRE(per <= MMD_CTR_MAX_PER, "ddim_update_ctr: sample too large");
  const DiffusionParams p{x, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<ddim_update_kernel<NoiseFromCounter>>("ddim_update_ctr", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream, p,
                                                          NoiseFromCounter{{key, ids, tag}}, out, x0_out, tab3, eta);
}

// x_t = sqrt_ac[t] x0 + sqrt_1mac[t] eps   (q_sample, multimodal_gaussian_diffusion.py:187-205); tab2 = [2][T]
// One element of it, shared with cond_replace_kernel so that both write the same bits.  Under -ffp-contract=fast the compiler fuses ONE
// of the two products of a x0 + b eps into the sum, and which one depends on the code around the expression; q_sample_kernel has
// always compiled to a rounded b eps and a fused a x0, and that form is spelled out here (its device code is unchanged by it).
__device__ __forceinline__ float q_sample_elem(float a, float x0, float b, float eps) { return fmaf(a, x0, b * eps); }
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ eps, float* __restrict__ out,
                                                       const float* __restrict__ tab2, const int64_t* __restrict__ t, int T, int64_t per,
                                                       int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ti = (int)t[i / per];
    out[i] = q_sample_elem(tab2[ti], x0[i], tab2[T + ti], eps[i]);
  }
}

extern "C" int mmd_q_sample(const float* x0, const float* eps, float* out, const float* tab2, const int64_t* t, int T, int N,
                            int64_t per_sample, void* stream) {
  MMD_REQUIRE(x0 && eps && out && tab2 && t && T > 0 && N > 0 && per_sample > 0, "q_sample: bad argument");
  const int64_t total = per_sample * N;
  return mmd_launch<q_sample_kernel>("q_sample", dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x0, eps, out, tab2, t, T, per_sample, total);
}

// Replacement-method conditioning with partial masks (the reference overwrites a whole stream before every step, gd:642-720): where a
// cell of the mask is set, x = A known + B eps in place, q_sample's element; elsewhere x is not written.  x / known (/ noise): fp32
// [N, F, C, HW]; mask: uint8, one cell per (frame, position) shared by the channels - element (n, f, c, p) reads
// mask[n * mask_stride + f * HW + p], mask_stride = 0 (one mask for the batch) or F * HW; mask == NULL = the whole stream.
// A, B = tab2[t[n]], tab2[T + t[n]], or the host scalars ca, cb with t == NULL (a timestep outside [0, T) replaces nothing).
// eps = noise[i], or the counter's x_T draw of the element: the value mmd_ctr_fill(draw = 0xFFFFFFFF) gives it.  Without a noise tensor
// (t == NULL, cb == 0) x = ca known, which is `known` bit for bit with ca == 1: the final paste.
// A thread owns W consecutive elements of a sample like the update kernels; a quad may straddle a mask row, a channel, a frame and the
// end of the sample, so the cell is tested per element, and a quad with no known element draws nothing.
#define MMD_CTR_DRAW_X_T (-1)      // NoiseFromCounter::draw casts its int to the 32-bit draw: 0xFFFFFFFF
struct CondReplaceParams {
  float* x; const float* known; const uint8_t* mask; int64_t mask_stride; const float* tab2; const int64_t* t;
  float ca, cb;
  int T, N, F, C, HW;
};
template <class Src>
__global__ __launch_bounds__(256) void cond_replace_kernel(const CondReplaceParams p, const Src src) {
  constexpr int W = Src::W;
  const int64_t chw = (int64_t)p.C * p.HW, per = chw * p.F;
  const int64_t ups = (per + W - 1) / W, total = ups * p.N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t n = u / ups, r0 = (u % ups) * W;
    float a = p.ca, b = p.cb;
    if (p.t) {
      const int64_t ti = p.t[n];
      if (ti < 0 || ti >= p.T) continue;
      a = p.tab2[ti];
      b = p.tab2[p.T + ti];
    }
    bool on[W];
    bool any = false;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int64_t r = r0 + j;
      on[j] = r < per && (!p.mask || p.mask[n * p.mask_stride + (r / chw) * p.HW + r % p.HW] != 0);
      any = any || on[j];
    }
    if (!any) continue;
    float z[W] = {};
    if (src.present()) src.draw(n, r0, n * per + r0, MMD_CTR_DRAW_X_T, z);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (!on[j]) continue;
      const int64_t i = n * per + r0 + j;
      p.x[i] = src.present() ? q_sample_elem(a, p.known[i], b, z[j]) : a * p.known[i];
    }
  }
}
static int cond_replace_args(const char* what, const float* x, const float* known, int64_t mask_stride, const float* tab2, const int64_t* t,
                             int T, int N, int F, int C, int HW) {
  MMD_REQUIRE(x && known && (!t || tab2), "%s: needs x and known, and tab2 when t is given", what);
  MMD_REQUIRE(T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "%s: T, N, F, C, HW must be positive", what);
  MMD_REQUIRE(mask_stride == 0 || mask_stride == (int64_t)F * HW, "%s: mask_stride is 0 (one mask for the batch) or F * HW = %ld; got %ld", what,
              (long)((int64_t)F * HW), (long)mask_stride);
  return MMD_OK;
}
extern "C" int mmd_cond_replace(float* x, const float* known, const float* noise, const uint8_t* mask, int64_t mask_stride, const float* tab2,
                                const int64_t* t, float ca, float cb, int T, int N, int F, int C, int HW, void* stream) {
  if (int rc = cond_replace_args("cond_replace", x, known, mask_stride, tab2, t, T, N, F, C, HW)) return rc;
  MMD_REQUIRE(noise || (!t && cb == 0.f), "cond_replace: noise may be NULL only with t == NULL and cb == 0 (the paste)");
  const CondReplaceParams p{x, known, mask, mask_stride, tab2, t, ca, cb, T, N, F, C, HW};
  return mmd_launch<cond_replace_kernel<NoiseFromMemory>>("cond_replace", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream, p,
                                                          NoiseFromMemory{noise});
}
extern "C" int mmd_cond_replace_ctr(float* x, const float* known, const uint32_t* key, const int64_t* ids, int tag, const uint8_t* mask,
                                    int64_t mask_stride, const float* tab2, const int64_t* t, float ca, float cb, int T, int N, int F, int C,
                                    int HW, void* stream) {
  if (int rc = cond_replace_args("cond_replace_ctr", x, known, mask_stride, tab2, t, T, N, F, C, HW)) return rc;
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "cond_replace_ctr: needs the key, the sample ids and a stream tag in [0, 3]");
  const int64_t per = (int64_t)F * C * HW;
  MMD_REQUIRE(per <= MMD_CTR_MAX_PER, "cond_replace_ctr: sample too large");
  const CondReplaceParams p{x, known, mask, mask_stride, tab2, t, ca, cb, T, N, F, C, HW};
  return mmd_launch<cond_replace_kernel<NoiseFromCounter>>("cond_replace_ctr", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream, p,
                                                           NoiseFromCounter{{key, ids, tag}});
}

// The forward jump of resampled masked sampling (RePaint, Lugmayr et al., CVPR 2022): the state at level m goes back up to level m + J,
//   x = a[m] x + b[m] z in place,   a[m] = sqrt(ac[m + J] / ac[m]),  b[m] = sqrt(1 - ac[m + J] / ac[m])      jtab = [2][T] fp32: a, b
// with q_sample's element, so the result is bitwise mmd_ctr_fill(draw) followed by mmd_q_sample(x, eps, x, jtab, m).  z = the counter
// normal of (element, draw[n], ids[n], tag).  One quad per thread; an m[n] outside [0, T) writes nothing.
__global__ __launch_bounds__(256) void renoise_ctr_kernel(float* x, const CtrKey k, const float* __restrict__ jtab, const int64_t* __restrict__ m,
                                                          const int64_t* __restrict__ draw, int T, int64_t per, int N) {
  const int64_t ups = (per + 3) / 4, total = ups * N;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t n = u / ups, r0 = (u % ups) * 4;
    const int64_t mi = m[n];
    if (mi < 0 || mi >= T) continue;
    const float a = jtab[mi], b = jtab[T + mi];
    float z[4];
    ctr_normals(k, n, r0, (uint32_t)draw[n], z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = r0 + j, i = n * per + r;
      if (r >= per) break;
      x[i] = q_sample_elem(a, x[i], b, z[j]);
    }
  }
}
extern "C" int mmd_renoise_ctr(float* x, const uint32_t* key, const int64_t* ids, int tag, const float* jtab, const int64_t* m,
                               const int64_t* draw, int T, int N, int F, int C, int HW, void* stream) {
  MMD_REQUIRE(x && jtab && m && draw, "renoise_ctr: needs x, the jump table, the levels and the draws");
  MMD_REQUIRE(T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "renoise_ctr: T, N, F, C, HW must be positive");
  MMD_REQUIRE(ctr_args_ok(key, ids, tag), "renoise_ctr: needs the key, the sample ids and a stream tag in [0, 3]");
  const int64_t per = (int64_t)F * C * HW;
  MMD_REQUIRE(per <= MMD_CTR_MAX_PER, "renoise_ctr: sample too large");
  return mmd_launch<renoise_ctr_kernel>("renoise_ctr", dim3(ew_grid((per + 3) / 4 * N)), dim3(256), 0, (hipStream_t)stream, x, CtrKey{key, ids, tag}, jtab,
                                        m, draw, T, per, N);
}

// out[n, i] = (ca[t_n] a + cb[t_n] b) * cs[t_n]    per-sample coefficients looked up from fp32 tables of length T
// (ca / cb / cs may be NULL = 1; b may be NULL).  Covers _predict_xstart_from_eps, _predict_eps_from_xstart,
// _predict_xstart_from_xprev, q_posterior mean, q_mean (gd:170-229,345-366).
__global__ __launch_bounds__(256) void lincomb_t_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                        const float* __restrict__ ca, const float* __restrict__ cb, const float* __restrict__ cs,
                                                        const int64_t* __restrict__ t, int64_t per, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ti = (int)t[i / per];
    float v = (ca ? ca[ti] : 1.f) * a[i];
    if (b) v += (cb ? cb[ti] : 1.f) * b[i];
    out[i] = cs ? v * cs[ti] : v;
  }
}
extern "C" int mmd_lincomb_t(const float* a, const float* b, float* out, const float* ca, const float* cb, const float* cs,
                             const int64_t* t, int N, int64_t per_sample, void* stream) {
  MMD_REQUIRE(a && out && t && N > 0 && per_sample > 0, "lincomb_t: bad argument");
  const int64_t total = per_sample * N;
  return mmd_launch<lincomb_t_kernel>("lincomb_t", dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, a, b, out, ca, cb, cs, t, per_sample, total);
}

// out = ca a + cb b + cc c with host scalars (b, c nullable): the DPM-Solver update combinations (dpm:520-1100).
// Its terms are lincomb_first / lincomb_add (mmd_dpm_elem.h), shared with the graph step's kernels so that all write the same bits.
__global__ __launch_bounds__(256) void lincomb_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                      float* __restrict__ out, float ca, float cb, float cc, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float v = lincomb_first(ca, a[i]);
    if (b) v = lincomb_add(v, cb, b[i]);
    if (c) v = lincomb_add(v, cc, c[i]);
    out[i] = v;
  }
}
extern "C" int mmd_lincomb(const float* a, float ca, const float* b, float cb, const float* c, float cc, float* out, int64_t n,
                           void* stream) {
  MMD_REQUIRE(a && out && n > 0, "lincomb: bad argument");
  return mmd_launch<lincomb_kernel>("lincomb", dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, c, out, ca, cb, cc, n);
}

// ----------------------------------------------------------------------------- training-loss reductions (forward values)
// Per-sample terms of multimodal_training_losses (gd:1114-1203) for one stream, API layout [N, F, Cm, HW]:
//   mse[n]  = mean((target - eps_hat)^2)                      (target = noise, or x0 when the model predicts x0)
//   vb[n]   = mean(KL(q(x_{t-1}|x_t,x_0) || p) ) / ln2  for t > 0, decoder NLL / ln2 at t == 0   (learned-range variance;
//             _vb_terms_bpd gd:1048-1092 with the frozen mean, normal_kl / discretized_gaussian_log_likelihood losses.py:12-77)
// One block per (sample, chunk); fixed-order tree reduction -> deterministic.  partial [N, nchunk, 2] doubles.
__device__ __forceinline__ float approx_std_normal_cdf(float x) {
  return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}
// One element of the variational bound in nats, shared by loss_terms_kernel (R = float: the training loss, fp32 like the reference) and
// vlb_terms_kernel (R = double: the evaluation form, evaluated in double from the fp32 inputs and tables): the discretized-Gaussian
// decoder NLL at t == 0, else KL(q(x_{t-1}|x_t,x_0) || p) with the true posterior (tmean, post_log).  The |x0| > 0.999 edge tests
// compare the fp32 datum, as the reference does.
__device__ __forceinline__ float vlb_exp(float x) { return expf(x); }
__device__ __forceinline__ double vlb_exp(double x) { return exp(x); }
__device__ __forceinline__ float vlb_log(float x) { return logf(x); }
__device__ __forceinline__ double vlb_log(double x) { return log(x); }
__device__ __forceinline__ float vlb_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double vlb_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float vlb_cdf(float x) { return approx_std_normal_cdf(x); }
__device__ __forceinline__ double vlb_cdf(double x) { return 0.5 * (1.0 + tanh(0.7978845608028654 * (x + 0.044715 * x * x * x))); }
template <typename R>
__device__ __forceinline__ R vlb_term(int ti, float x0f, R mean, R tmean, R logvar, R post_log) {
  const R x0 = x0f;
  R term;
  if (ti == 0) {        // decoder NLL
    const R cx = x0 - mean, inv = vlb_exp(R(-0.5) * logvar);
    const R cdf_p = vlb_cdf(inv * (cx + R(1) / R(255)));
    const R cdf_m = vlb_cdf(inv * (cx - R(1) / R(255)));
    const R lp = vlb_log(vlb_max(cdf_p, R(1e-12))), lm = vlb_log(vlb_max(R(1) - cdf_m, R(1e-12)));
    const R ld = vlb_log(vlb_max(cdf_p - cdf_m, R(1e-12)));
    term = -(x0f < -0.999f ? lp : (x0f > 0.999f ? lm : ld));
  } else {              // KL(q || p), true posterior log-variance = posterior_log_variance_clipped
    const R dm = tmean - mean;
    term = R(0.5) * (R(-1) + logvar - post_log + vlb_exp(post_log - logvar) + dm * dm * vlb_exp(-logvar));
  }
  return term;
}
// p.x = x_t; x0 and p.x are read with flag 4 only
__global__ __launch_bounds__(256) void loss_terms_kernel(const DiffusionParams p, const float* x0, const float* target, double* partial, int nchunk) {
  __shared__ double s_a[256], s_b[256];
  const int n = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int ti = (int)p.t[n];
  const X0Coef<float> k = x0_coef<float>(p, ti);
  const PostCoef<float> q = post_coef<float>(p, ti);
  const RangeLogs<float> l = range_logs<float>(p, ti);
  double mse = 0.0, vb = 0.0;
  const int64_t lo = per * chunk / nchunk, hi = per * (chunk + 1) / nchunk;
  for (int64_t r = lo + tid; r < hi; r += 256) {
    const ElemAddr a = elem_addr(p, n, r);
    const int64_t i = n * per + r;
    const float o = p.mo[a.mean];
    const float d = target[i] - o;
    mse += (double)(d * d);
    if (p.flags & 4) {
      const float logvar = range_logvar(p, a, l);
      const float xv = p.x[i], x0v = x0[i];
      const float mean = post_mean(q, pred_x0(p, k, o, xv), xv);          // clip_denoised=False in the vb term
      const float term = vlb_term<float>(ti, x0v, mean, post_mean(q, x0v, xv), logvar, l.min_log);
      vb += (double)term;
    }
  }
  s_a[tid] = mse;
  s_b[tid] = vb;
  block_tree_sum256(tid, s_a, s_b);
  if (tid == 0) {
    partial[((int64_t)n * nchunk + chunk) * 2] = s_a[0];
    partial[((int64_t)n * nchunk + chunk) * 2 + 1] = s_b[0];
  }
}
__global__ void loss_finalize_kernel(const double* __restrict__ partial, int nchunk, double inv_count, float vb_scale,
                                     float* __restrict__ mse_out, float* __restrict__ vb_out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= (int)gridDim.x * (int)blockDim.x) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nchunk; ++k) { a += partial[((int64_t)n * nchunk + k) * 2]; b += partial[((int64_t)n * nchunk + k) * 2 + 1]; }
  mse_out[n] = (float)(a * inv_count);
  if (vb_out) vb_out[n] = (float)(b * inv_count / 0.6931471805599453) * vb_scale;
}

#define MMD_LOSS_CHUNKS 64
extern "C" int64_t mmd_loss_workspace_bytes(int N) { return (int64_t)N * MMD_LOSS_CHUNKS * 2 * sizeof(double); }

// Per-sample loss terms of one stream (see loss_terms_kernel).  x0/xt may be NULL without flag 4.  vb_scale = T/1000 for
// RESCALED_MSE else 1.  mse_out/vb_out fp32 [N].
extern "C" int mmd_loss_terms(const float* x0, const float* xt, const float* model_out, const float* target, const float* tables,
                              const int64_t* t, int T, int N, int F, int C, int HW, int flags, float vb_scale, float* mse_out,
                              float* vb_out, void* workspace, void* stream) {
  MMD_REQUIRE(model_out && target && tables && t && mse_out && workspace && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "loss_terms: bad argument");
  MMD_REQUIRE(!(flags & 4) || (x0 && xt && vb_out), "loss_terms: the vb term needs x0, x_t and vb_out");
  const DiffusionParams p{xt, model_out, tables, t, T, N, F, C, HW, flags};
  hipStream_t st = (hipStream_t)stream;
  int rc = mmd_launch<loss_terms_kernel>("loss_terms", dim3(MMD_LOSS_CHUNKS, N), dim3(256), 0, st, p, x0, target, (double*)workspace, MMD_LOSS_CHUNKS);
  if (rc) return rc;
  return mmd_launch<loss_finalize_kernel>("loss_finalize", dim3(1), dim3(N), 0, st, (const double*)workspace, MMD_LOSS_CHUNKS, 1.0 / ((double)F * C * HW),
                                          vb_scale, mse_out, (flags & 4) ? vb_out : nullptr);
}

// ----------------------------------------------------------------------------- training-loss gradient (learned-range variance)
// Gradient of  sum_n ( dmse[n] * mse[n] + dvb[n] * vb[n] )  w.r.t. the model output [N, F, Cm, HW] (Cm = 2C with flag 4):
//   mean channels c < C     : dmse[n] * 2 (o - target) / per                      (the vb term sees the mean DETACHED, gd:1147-1151)
//   variance channels c >= C: dvb[n] * vb_scale / (per ln 2) * d term / d logvar * (max_log - min_log) / 2
// with term = KL(q || p) for t > 0 and the discretized-Gaussian decoder NLL at t == 0 (losses.py:12-77), in the forward
// arithmetic of loss_terms_kernel: both evaluate the element core's log-variance, x0 prediction and posterior means.
// d vlb_term / d logvar (returned) and d vlb_term / d mean (*dmean), in the forward's own arithmetic; the clamped logs of the decoder
// NLL have zero slope below the clamp.
__device__ __forceinline__ float vlb_term_grad(int ti, float x0, float mean, float tmean, float logvar, float post_log, float* dmean) {
  float dterm;
  if (ti == 0) {
    const float cx = x0 - mean, inv = expf(-0.5f * logvar);
    const float up = inv * (cx + 1.f / 255.f), um = inv * (cx - 1.f / 255.f);
    const float cdf_p = approx_std_normal_cdf(up), cdf_m = approx_std_normal_cdf(um);
    // d cdf(u) / d logvar = pdf~(u) * (-u / 2),  pdf~ = derivative of the tanh approximation
    auto dcdf = [](float u) {
      const float k = 0.7978845608028654f, a = 0.044715f;
      const float th_ = tanhf(k * (u + a * u * u * u));
      return 0.5f * (1.f - th_ * th_) * k * (1.f + 3.f * a * u * u) * (-0.5f * u);
    };
    // d cdf(u) / d mean = pdf~(u) * (-inv)
    auto dcdf_mean = [inv](float u) {
      const float k = 0.7978845608028654f, a = 0.044715f;
      const float th_ = tanhf(k * (u + a * u * u * u));
      return 0.5f * (1.f - th_ * th_) * k * (1.f + 3.f * a * u * u) * (-inv);
    };
    const float dp = dcdf(up), dm_ = dcdf(um);
    const float ep = dcdf_mean(up), em = dcdf_mean(um);
    float dlog, elog;
    if (x0 < -0.999f) { dlog = cdf_p > 1e-12f ? dp / cdf_p : 0.f; elog = cdf_p > 1e-12f ? ep / cdf_p : 0.f; }
    else if (x0 > 0.999f) { dlog = (1.f - cdf_m) > 1e-12f ? -dm_ / (1.f - cdf_m) : 0.f; elog = (1.f - cdf_m) > 1e-12f ? -em / (1.f - cdf_m) : 0.f; }
    else { dlog = (cdf_p - cdf_m) > 1e-12f ? (dp - dm_) / (cdf_p - cdf_m) : 0.f; elog = (cdf_p - cdf_m) > 1e-12f ? (ep - em) / (cdf_p - cdf_m) : 0.f; }
    dterm = -dlog;
    *dmean = -elog;
  } else {
    const float dm = tmean - mean;
    dterm = 0.5f * (1.f - expf(post_log - logvar) - dm * dm * expf(-logvar));
    *dmean = -dm * expf(-logvar);
  }
  return dterm;
}
__global__ __launch_bounds__(256) void loss_terms_bwd_kernel(const DiffusionParams p, const float* x0, const float* target,
                                                             const float* __restrict__ dmse, const float* __restrict__ dvb, float vb_scale,
                                                             float* __restrict__ g) {
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int64_t total = per * p.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const ElemAddr a = elem_addr(p, n, i % per);
    const int ti = (int)p.t[n];
    const float o = p.mo[a.mean];
    g[a.mean] = dmse[n] * 2.f * (o - target[i]) / (float)per;
    if (p.flags & 4) {
      const X0Coef<float> k = x0_coef<float>(p, ti);
      const PostCoef<float> q = post_coef<float>(p, ti);
      const RangeLogs<float> l = range_logs<float>(p, ti);
      const float logvar = range_logvar(p, a, l);
      const float xv = p.x[i], x0v = x0[i];
      const float mean = post_mean(q, pred_x0(p, k, o, xv), xv);
      float dmean_unused;
      const float dterm = vlb_term_grad(ti, x0v, mean, post_mean(q, x0v, xv), logvar, l.min_log, &dmean_unused);      // d term / d logvar
      g[a.var] = dvb[n] * vb_scale / ((float)per * 0.6931471805599453f) * dterm * 0.5f * (l.max_log - l.min_log);
    }
  }
}
extern "C" int mmd_loss_terms_bwd(const float* x0, const float* xt, const float* model_out, const float* target, const float* tables,
                                  const int64_t* t, int T, int N, int F, int C, int HW, int flags, float vb_scale, const float* dmse,
                                  const float* dvb, float* g_model_out, void* stream) {
  MMD_REQUIRE(model_out && target && tables && t && dmse && g_model_out && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "loss_terms_bwd: bad argument");
  MMD_REQUIRE(!(flags & 4) || (x0 && xt && dvb), "loss_terms_bwd: the vb term needs x0, x_t and dvb");
  const DiffusionParams p{xt, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<loss_terms_bwd_kernel>("loss_terms_bwd", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream, p, x0, target, dmse, dvb,
                                           vb_scale, g_model_out);
}

// ----------------------------------------------------------------------------- variational bound, evaluation form (bits / dim)
// One term of calc_bpd_loop (gd:1048-1092, 1231-1286; SR gaussian_diffusion.py:796-829, 953-1008) for one stream, API layout as
// ddpm_update / loss_terms, in ONE pass over the tensors.  Per sample n (t = t[n]):
//   vb[n]         = mean KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) / ln 2  (t > 0), decoder NLL / ln 2 (t == 0)
//   xstart_mse[n] = mean((pred_x0 - x0)^2)
//   eps_mse[n]    = mean((eps - noise)^2),  eps = (sqrt_recip_ac x_t - pred_x0) / sqrt_recipm1_ac  (so it sees the clamp); noise nullable
// flags 1 / 2 / 4 as ddpm_update; without flag 4 the model's log-variance is table row 4; the true posterior's is always row 5.
// Inputs and table coefficients are fp32; the per-element arithmetic and the sums are evaluated in double (vlb_term<double>).
// Same (sample, chunk) grid and fixed-order double reduction as loss_terms_kernel; partial [N, nchunk, 3] doubles.  The finalize
// kernel writes sample n's results at column t[n] of row n of the result tables (ld floats per row; ld == 0: plain [N] vectors), so a
// whole loop needs no per-step host value and sits in a captured graph.
__global__ __launch_bounds__(256) void vlb_terms_kernel(const DiffusionParams p, const float* x0, const float* noise, float* px0_out, double* partial,
                                                        int nchunk) {
  __shared__ double s_a[256], s_b[256], s_c[256];
  const int n = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int ti = (int)p.t[n];
  // fp32 table and tensor values, every operation on them in double (what that costs beside an fp32 form: DESIGN, the bound's row)
  const X0Coef<double> k = x0_coef<double>(p, ti);
  const PostCoef<double> q = post_coef<double>(p, ti);
  const double fixed_log = table_row<double>(p, 4, ti);
  const RangeLogs<double> l = range_logs<double>(p, ti);
  double vb = 0.0, xs = 0.0, em = 0.0;
  const int64_t lo = per * chunk / nchunk, hi = per * (chunk + 1) / nchunk;
  for (int64_t r = lo + tid; r < hi; r += 256) {
    const ElemAddr a = elem_addr(p, n, r);
    const int64_t i = n * per + r;
    const double o = p.mo[a.mean];
    const double logvar = (p.flags & 4) ? range_logvar(p, a, l) : fixed_log;
    const float x0f = x0[i];
    const double xv = p.x[i], x0v = x0f;
    const double px0 = pred_x0_clamped(p, k, o, xv);
    vb += vlb_term<double>(ti, x0f, post_mean(q, px0, xv), post_mean(q, x0v, xv), logvar, l.min_log);
    const double dx = px0 - x0v;
    xs += dx * dx;
    if (noise) {
      const double de = (k.cr * xv - px0) / k.crm1 - (double)noise[i];
      em += de * de;
    }
    if (px0_out) px0_out[i] = (float)px0;
  }
  s_a[tid] = vb;
  s_b[tid] = xs;
  s_c[tid] = em;
  block_tree_sum256(tid, s_a, s_b, s_c);
  if (tid == 0) {
    double* q = partial + ((int64_t)n * nchunk + chunk) * 3;
    q[0] = s_a[0]; q[1] = s_b[0]; q[2] = s_c[0];
  }
}
__global__ void vlb_finalize_kernel(const double* __restrict__ partial, int nchunk, int N, double inv_count, const int64_t* __restrict__ t,
                                    int64_t ld, float* __restrict__ vb_out, float* __restrict__ xs_out, float* __restrict__ eps_out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int k = 0; k < nchunk; ++k) {
    const double* q = partial + ((int64_t)n * nchunk + k) * 3;
    a += q[0]; b += q[1]; c += q[2];
  }
  if (ld && (t[n] < 0 || t[n] >= ld)) return;      // a timestep outside the row is never written
  const int64_t at = ld ? (int64_t)n * ld + t[n] : n;
  vb_out[at] = (float)(a * inv_count / 0.6931471805599453);
  if (xs_out) xs_out[at] = (float)(b * inv_count);
  if (eps_out) eps_out[at] = (float)(c * inv_count);
}

extern "C" int64_t mmd_vlb_workspace_bytes(int N) { return (int64_t)N * MMD_LOSS_CHUNKS * 3 * sizeof(double); }

// vb_out / xstart_mse_out / eps_mse_out: fp32 result tables [N, out_ld], sample n written at column t[n]; out_ld == 0: fp32 [N].
// noise == NULL skips eps_mse (eps_mse_out must then be NULL); xstart_mse_out and pred_xstart_out (fp32 like x0) are optional.
extern "C" int mmd_vlb_terms(const float* x0, const float* xt, const float* noise, const float* model_out, const float* tables,
                             const int64_t* t, int T, int N, int F, int C, int HW, int flags, float* vb_out, float* xstart_mse_out,
                             float* eps_mse_out, int64_t out_ld, float* pred_xstart_out, void* workspace, void* stream) {
  MMD_REQUIRE(x0 && xt && model_out && tables && t && vb_out && workspace && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "vlb_terms: bad argument");
  MMD_REQUIRE(!(flags & ~7), "vlb_terms: flags are 1 (clip x0), 2 (model predicts x0), 4 (learned-range variance); got %d", flags);
  MMD_REQUIRE(!eps_mse_out || noise, "vlb_terms: eps_mse needs the noise tensor");
  MMD_REQUIRE(out_ld == 0 || out_ld >= T, "vlb_terms: result rows of %ld floats cannot hold %d timesteps", (long)out_ld, T);
  const DiffusionParams p{xt, model_out, tables, t, T, N, F, C, HW, flags};
  hipStream_t st = (hipStream_t)stream;
  int rc = mmd_launch<vlb_terms_kernel>("vlb_terms", dim3(MMD_LOSS_CHUNKS, N), dim3(256), 0, st, p, x0, eps_mse_out ? noise : nullptr, pred_xstart_out,
                                        (double*)workspace, MMD_LOSS_CHUNKS);
  if (rc) return rc;
  return mmd_launch<vlb_finalize_kernel>("vlb_finalize", dim3(cdiv(N, 64)), dim3(64), 0, st, (const double*)workspace, MMD_LOSS_CHUNKS, N,
                                         1.0 / ((double)F * C * HW), t, out_ld, vb_out, xstart_mse_out, eps_mse_out);
}

// ----------------------------------------------------------------------------- variational-bound gradient (KL / RESCALED_KL training)
// Gradient of  sum_n dvb[n] * vb[n]  of mmd_vlb_terms w.r.t. the model output, the mean NOT detached (gaussian_diffusion.py:872-882 calls
// _vb_terms_bpd on the live model output with clip_denoised=False):
//   mean channels     : dvb[n] / (per ln 2) * d term / d mean * c1 * (1 with flag 2, else -sqrt_recipm1_ac)     (pred_x0 -> posterior mean)
//   variance channels : as loss_terms_bwd_kernel (flag 4 only)
__global__ __launch_bounds__(256) void vlb_terms_bwd_kernel(const DiffusionParams p, const float* x0, const float* __restrict__ dvb,
                                                            float* __restrict__ g) {
  const int64_t per = (int64_t)p.F * p.C * p.HW;
  const int64_t total = per * p.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per;
    const ElemAddr a = elem_addr(p, n, i % per);
    const int ti = (int)p.t[n];
    const X0Coef<float> k = x0_coef<float>(p, ti);
    const PostCoef<float> q = post_coef<float>(p, ti);
    const RangeLogs<float> l = range_logs<float>(p, ti);
    const float o = p.mo[a.mean];
    const float logvar = (p.flags & 4) ? range_logvar(p, a, l) : table_row<float>(p, 4, ti);
    const float xv = p.x[i], x0v = x0[i];
    const float mean = post_mean(q, pred_x0(p, k, o, xv), xv);
    float dmean;
    const float dterm = vlb_term_grad(ti, x0v, mean, post_mean(q, x0v, xv), logvar, l.min_log, &dmean);
    const float w = dvb[n] / ((float)per * 0.6931471805599453f);
    g[a.mean] = w * dmean * q.c1 * ((p.flags & 2) ? 1.f : -k.crm1);
    if (p.flags & 4) g[a.var] = w * dterm * 0.5f * (l.max_log - l.min_log);
  }
}
// g_model_out like model_out ([N, F, Cm, HW]); every element is written.  Clip (flag 1) is not differentiable here.
extern "C" int mmd_vlb_terms_bwd(const float* x0, const float* xt, const float* model_out, const float* tables, const int64_t* t, int T,
                                 int N, int F, int C, int HW, int flags, const float* dvb, float* g_model_out, void* stream) {
  MMD_REQUIRE(x0 && xt && model_out && tables && t && dvb && g_model_out && T > 0 && N > 0 && F > 0 && C > 0 && HW > 0, "vlb_terms_bwd: bad argument");
  MMD_REQUIRE(!(flags & ~7), "vlb_terms_bwd: flags are 2 (model predicts x0) and 4 (learned-range variance); got %d", flags);
  MMD_REQUIRE(!(flags & 1), "vlb_terms_bwd: the clipped x0 prediction (flag 1) is not differentiable here (training uses clip_denoised=False)");
  const DiffusionParams p{xt, model_out, tables, t, T, N, F, C, HW, flags};
  return mmd_launch<vlb_terms_bwd_kernel>("vlb_terms_bwd", dim3(ew_grid((int64_t)N * F * C * HW)), dim3(256), 0, (hipStream_t)stream, p, x0, dvb, g_model_out);
}

// ----------------------------------------------------------------------------- spherical interpolation of two latents
// out[n] = w_a a[n] + w_b b[n] for fp32 [N, per] rows, lam fp32 [N] (ddim_interpolate: the slerp of two encoded clips).  With
//   dot = sum a b, na = sum a^2, nb = sum b^2 (fp64 sums of fp32 data: every product is exact in fp64),
//   c = clamp(dot / sqrt(na nb), -1, 1), theta = acos c, s = sin theta,
// the weights are w_a = sin((1 - lam) theta) / s, w_b = sin(lam theta) / s, or the chord's 1 - lam, lam when na nb == 0 or |c| > 0.9995
// (sin theta < 0.032 there: the two forms differ by less than theta^2 / 8 and the quotient loses its digits).  They are formed in fp64
// and rounded to fp32 once, so the error of out is that of the combine fma(w_a, a, fl(w_b b)).  theta is evaluated once: lam = 0 gives
// s / s = 1 and sin(0) / s = 0, lam = 1 the mirror image, so out is bitwise a or b (finite data without negative zeros).
// Two launches, SLERP_BLOCK threads per workgroup, grid (chunks, N): slerp_sums_kernel writes the three partial sums of its chunk to
// ws [N, chunks, 3]; slerp_combine_kernel re-reduces the chunks of its sample - every workgroup in the same tree order - and one
// thread forms the weights.  No atomics, no host read; the chunking depends on `per` alone (slerp_chunk), so a row's bits do not
// depend on N.  A thread owns quads of consecutive elements of a sample: 16-byte accesses where the quad is whole and its address a
// multiple of 16 (a, b and out each by their own address), element by element otherwise, and the order of every sum follows the element
// index alone - a row's bits do not depend on where its buffers start either.
#define SLERP_BLOCK 256
#define SLERP_UNIT (SLERP_BLOCK * 4 * 2)      // two quads per thread: the smallest chunk
#define SLERP_MAX_CHUNKS 256                  // the combine kernel reduces them with one block tree sum
static int64_t slerp_chunk(int64_t per) {
  const int64_t units = (per + (int64_t)SLERP_UNIT * SLERP_MAX_CHUNKS - 1) / ((int64_t)SLERP_UNIT * SLERP_MAX_CHUNKS);
  return units * SLERP_UNIT;
}
static int slerp_chunks(int64_t per) { return (int)((per + slerp_chunk(per) - 1) / slerp_chunk(per)); }

__global__ __launch_bounds__(SLERP_BLOCK) void slerp_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ ws,
                                                                 int64_t per, int64_t chunk) {
  __shared__ double s_d[SLERP_BLOCK], s_a[SLERP_BLOCK], s_b[SLERP_BLOCK];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.y, lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < per ? lo + chunk : per;
  const float* an = a + n * per;
  const float* bn = b + n * per;
  double dot = 0.0, na = 0.0, nb = 0.0;
  for (int64_t r0 = lo + (int64_t)tid * 4; r0 < hi; r0 += SLERP_BLOCK * 4) {
    const int cnt = hi - r0 < 4 ? (int)(hi - r0) : 4;
    float av[4] = {}, bv[4] = {};
    quad_load(an + r0, cnt, quad_on16(an + r0, cnt), av);
    quad_load(bn + r0, cnt, quad_on16(bn + r0, cnt), bv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // elements past the end are zeros: they add nothing
      const double x = av[j], y = bv[j];
      dot += x * y;
      na += x * x;
      nb += y * y;
    }
  }
  s_d[tid] = dot;
  s_a[tid] = na;
  s_b[tid] = nb;
  block_tree_sum256(tid, s_d, s_a, s_b);
  if (tid == 0) {
    double* w = ws + (n * gridDim.x + blockIdx.x) * 3;
    w[0] = s_d[0];
    w[1] = s_a[0];
    w[2] = s_b[0];
  }
}

__global__ __launch_bounds__(SLERP_BLOCK) void slerp_combine_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    const float* __restrict__ lam, float* __restrict__ out,
                                                                    const double* __restrict__ ws, int64_t per, int64_t chunk) {
  __shared__ double s_d[SLERP_BLOCK], s_a[SLERP_BLOCK], s_b[SLERP_BLOCK];
  __shared__ float s_w[2];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.y, lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < per ? lo + chunk : per;
  const bool have = tid < (int)gridDim.x;      // gridDim.x = the chunks of a sample <= SLERP_MAX_CHUNKS
  const double* w = ws + (n * gridDim.x + (have ? tid : 0)) * 3;
  s_d[tid] = have ? w[0] : 0.0;
  s_a[tid] = have ? w[1] : 0.0;
  s_b[tid] = have ? w[2] : 0.0;
  block_tree_sum256(tid, s_d, s_a, s_b);
  if (tid == 0) {
    const double l = lam[n], den = s_a[0] * s_b[0];
    double wa = 1.0 - l, wb = l;
    if (den != 0.0) {
      const double c = fmin(fmax(s_d[0] / sqrt(den), -1.0), 1.0);
      if (!(fabs(c) > 0.9995)) {      // a NaN goes through the quotient and shows in out
        const double theta = acos(c), s = sin(theta);
        wa = sin((1.0 - l) * theta) / s;
        wb = sin(l * theta) / s;
      }
    }
    s_w[0] = (float)wa;
    s_w[1] = (float)wb;
  }
  __syncthreads();
  const float wa = s_w[0], wb = s_w[1];
  const float* an = a + n * per;
  const float* bn = b + n * per;
  float* on = out + n * per;
  for (int64_t r0 = lo + (int64_t)tid * 4; r0 < hi; r0 += SLERP_BLOCK * 4) {
    const int cnt = hi - r0 < 4 ? (int)(hi - r0) : 4;
    float av[4] = {}, bv[4] = {}, v[4];
    quad_load(an + r0, cnt, quad_on16(an + r0, cnt), av);
    quad_load(bn + r0, cnt, quad_on16(bn + r0, cnt), bv);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __fmaf_rn(wa, av[j], __fmul_rn(wb, bv[j]));      // spelled out: one rounded product, one fma
    quad_store(on + r0, cnt, quad_on16(on + r0, cnt), v);
  }
}

extern "C" int64_t mmd_slerp_ws_bytes(int N, int64_t per) {
  return N > 0 && per > 0 ? (int64_t)N * slerp_chunks(per) * 3 * (int64_t)sizeof(double) : 0;
}

extern "C" int mmd_slerp(const float* a, const float* b, const float* lam, float* out, double* ws, int N, int64_t per, void* stream) {
  MMD_REQUIRE(a && b && lam && out && ws, "slerp: needs a, b, lam, out and the workspace ws (mmd_slerp_ws_bytes)");
  MMD_REQUIRE(N > 0 && N <= 65535 && per > 0, "slerp: N must be in [1, 65535] and per positive, got N %d per %lld", N, (long long)per);
  MMD_REQUIRE(per <= ((int64_t)1 << 40) / N, "slerp: N per = %d x %lld elements is too large", N, (long long)per);
  MMD_REQUIRE(dpm_disjoint(out, a, per * N) && dpm_disjoint(out, b, per * N), "slerp: out must not overlap a or b (a and b may overlap)");
  const int64_t chunk = slerp_chunk(per);
  const dim3 grid(slerp_chunks(per), N);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mmd_launch<slerp_sums_kernel>("slerp_sums", grid, dim3(SLERP_BLOCK), 0, st, a, b, ws, per, chunk)) return rc;
  return mmd_launch<slerp_combine_kernel>("slerp_combine", grid, dim3(SLERP_BLOCK), 0, st, a, b, lam, out, (const double*)ws, per, chunk);
}
