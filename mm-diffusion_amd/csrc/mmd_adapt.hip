// The adaptive (embedded-pair) DPM-Solver++ of order 2 with its step-size controller on the device (DPM_Solver.sample_graph_adaptive;
// eager: dpm_solver_adaptive, the reference's dpm:1088-1149).  A trial step s -> t evaluates the network at (x, s) and at
// (x_s1, s1 = lambda^-1(lambda_s + h / 2)); the first-order result LO and the second-order result at t give the error norm E, the step is
// accepted when E <= 1 and the next h follows from E.  Four kernels keep every scalar of that loop in device memory, so a trial step is
// a fixed launch sequence (include/mmd.h has the contract of each):
//   mmd_dpm_adapt_open     XB = x, MS = m0, LO = a0 x + a1 m0, x = b0 x + b1 m0
//   mmd_dpm_adapt_close    x = c0 XB + c1 MS + c2 m1, and the fp64 chunk sums of the squared error terms
//   mmd_dpm_adapt_control  E, the decision, the next s / h / t / s1, and every coefficient row the next trial reads
//   mmd_dpm_adapt_commit   accept: PREV = LO; reject: x = XB
// open, close and commit are step kernels and live with the other solvers' in mmd_dpm.hip; here: controller, schedule, mmd_dpm_adapt_time.
#include "mmd_common.h"
#include <math.h>

// ----------------------------------------------------------------------------- the controller
// The discrete VP schedule in fp64 (NoiseScheduleVP's 'discrete' family): log alpha is known at t_i = (i + 1) / T and linear in between,
// the end segments extended outside.
struct AdaptSchedule { const double* la; int T; };
__device__ __forceinline__ double sched_knot(const AdaptSchedule& S, int i) { return (double)(i + 1) / (double)S.T; }
__device__ double sched_log_alpha(const AdaptSchedule& S, double t) {
  int hi = (int)ceil(t * (double)S.T) - 1;                       // about the first knot >= t; made exact below
  hi = hi < 1 ? 1 : (hi > S.T - 1 ? S.T - 1 : hi);
  while (hi > 1 && sched_knot(S, hi - 1) >= t) --hi;
  while (hi < S.T - 1 && sched_knot(S, hi) < t) ++hi;
  const int lo = hi - 1;
  const double xl = sched_knot(S, lo), xh = sched_knot(S, hi);
  return S.la[lo] + (t - xl) * (S.la[hi] - S.la[lo]) / (xh - xl);
}
__device__ __forceinline__ double sched_sigma(double la) { return sqrt(-expm1(2.0 * la)); }
__device__ __forceinline__ double sched_lambda_of_la(double la) { return la - 0.5 * log(-expm1(2.0 * la)); }
// t(lambda): log alpha = -1/2 log(1 + e^(-2 lambda)), then the table read backwards (log alpha descends in t)
__device__ double sched_inverse_lambda(const AdaptSchedule& S, double lam) {
  const double m = -2.0 * lam;
  const double q = -0.5 * (m > 0.0 ? m + log1p(exp(-m)) : log1p(exp(m)));
  // ascending abscissa xp[j] = la[T - 1 - j]; the first j with xp[j] >= q, kept in [1, T - 1]
  int a = 0, b = S.T;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (S.la[S.T - 1 - mid] < q) a = mid + 1; else b = mid;
  }
  const int hi = a < 1 ? 1 : (a > S.T - 1 ? S.T - 1 : a), lo = hi - 1;
  const double xl = S.la[S.T - 1 - lo], xh = S.la[S.T - 1 - hi];
  const double yl = sched_knot(S, S.T - 1 - lo), yh = sched_knot(S, S.T - 1 - hi);
  return yl + (q - xl) * (yh - yl) / (xh - xl);
}
// model_wrapper.get_model_input_time on the time rounded to fp32: ((t - 1 / T) * T).to(int), each operation rounded to fp32
__device__ __forceinline__ int64_t sched_model_time(const AdaptSchedule& S, double t) {
  const float d = __fsub_rn((float)t, (float)(1.0 / (double)S.T));
  return (int64_t)(int)__fmul_rn(d, (float)S.T);
}

struct AdaptCtl {
  int mode, batch, N;
  const double* params; AdaptSchedule S;
  const double* part_v; int chunks_v; double per_v;
  const double* part_a; int chunks_a; double per_a;
  double* state; int64_t* itab; int32_t* cnt; float* ftab; int32_t* status;
};

// Everything the next trial of sample n reads, from its s, h and lambda_s: t, s1, the model timesteps, the coefficient rows (fp64,
// rounded to fp32 once) and the conditioning levels.  The expressions are _first_coefs' and _single_second_coefs' (r1 = 1 / 2,
// 'dpm_solver') in their data-prediction form.
__device__ void adapt_write_rows(const AdaptCtl& c, int n) {
  double* st = c.state + (int64_t)MMD_ADAPT_STATE_WORDS * n;
  const double s = st[MMD_ADAPT_S_S], h = st[MMD_ADAPT_S_H], lam_s = st[MMD_ADAPT_S_LAM];
  const double t = sched_inverse_lambda(c.S, lam_s + h), s1 = sched_inverse_lambda(c.S, lam_s + 0.5 * h);
  st[MMD_ADAPT_S_T] = t;
  st[MMD_ADAPT_S_S1] = s1;
  const double la_s = sched_log_alpha(c.S, s), la_1 = sched_log_alpha(c.S, s1), la_t = sched_log_alpha(c.S, t);
  const double al_s = exp(la_s), al_1 = exp(la_1), al_t = exp(la_t);
  const double sg_s = sched_sigma(la_s), sg_1 = sched_sigma(la_1), sg_t = sched_sigma(la_t);
  const double h_t = sched_lambda_of_la(la_t) - lam_s, h_1 = sched_lambda_of_la(la_1) - lam_s;
  const double first = -(al_t * expm1(-h_t));          // the model coefficient of the first-order update s -> t
  // r1 = 1 / 2: c2 = (0.5 / r1) first = first and c1 = first - c2 = 0, as the host's fp32 values come out.  Written as constants: a
  // contracted first - c2 would keep the product's rounding residual, a c1 of 1e-17 where the eager update has an exact zero.
  const double c2 = first, c1 = 0.0;
  const int64_t N = c.N;
  float* f = c.ftab + n;
  f[0 * N] = (float)(1.0 / al_s);   f[1 * N] = (float)(-sg_s / al_s);
  f[2 * N] = (float)(sg_t / sg_s);  f[3 * N] = (float)first;
  f[4 * N] = (float)(sg_1 / sg_s);  f[5 * N] = (float)(-(al_1 * expm1(-h_1)));
  f[6 * N] = (float)(1.0 / al_1);   f[7 * N] = (float)(-sg_1 / al_1);
  f[8 * N] = (float)(sg_t / sg_s);  f[9 * N] = (float)c1;  f[10 * N] = (float)c2;  f[11 * N] = 0.f;
  f[12 * N] = (float)al_s;  f[13 * N] = (float)sg_s;
  f[14 * N] = (float)al_1;  f[15 * N] = (float)sg_1;
  c.itab[1 * N + n] = sched_model_time(c.S, s);
  c.itab[2 * N + n] = sched_model_time(c.S, s1);
}

__global__ __launch_bounds__(256) void dpm_adapt_control_kernel(const AdaptCtl c) {
  __shared__ float s_e[256];
  __shared__ int s_bad[256], s_act[256];
  const int tid = threadIdx.x;
  const double theta = c.params[MMD_ADAPT_P_THETA], t_err = c.params[MMD_ADAPT_P_TERR], t_0 = c.params[MMD_ADAPT_P_T0];
  // pass 1 (a trial's end): every open sample's E from the chunk sums of both streams, in ascending chunk order
  float emax = 0.f;
  int bad_any = 0;
  if (c.mode == 0) {
    for (int n = tid; n < c.N; n += 256) {
      if (c.cnt[4 * n + MMD_ADAPT_C_DONE]) continue;
      double sv = 0.0, sa = 0.0;
      for (int j = 0; j < c.chunks_v; ++j) sv += c.part_v[(int64_t)n * c.chunks_v + j];
      for (int j = 0; j < c.chunks_a; ++j) sa += c.part_a[(int64_t)n * c.chunks_a + j];
      float e = (float)sqrt(sv / c.per_v);
      if (c.part_a) e = fmaxf(e, (float)sqrt(sa / c.per_a));
      const bool bad = !(isfinite(sv) && isfinite(sa) && isfinite(e));
      c.state[(int64_t)MMD_ADAPT_STATE_WORDS * n + MMD_ADAPT_S_E] = bad ? (double)NAN : (double)e;
      bad_any |= bad ? 1 : 0;
      if (!bad) emax = fmaxf(emax, e);
    }
    if (c.batch) {      // the reference's rule: one E, the maximum over the batch (a maximum does not depend on its order)
      s_e[tid] = emax;
      s_bad[tid] = bad_any;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
          s_e[tid] = fmaxf(s_e[tid], s_e[tid + o]);
          s_bad[tid] |= s_bad[tid + o];
        }
        __syncthreads();
      }
      emax = s_e[0];
      bad_any = s_bad[0];
      __syncthreads();
    }
  }
  // pass 2: the decision and the next trial of every sample
  int active = 0, fault = 0;
  for (int n = tid; n < c.N; n += 256) {
    double* st = c.state + (int64_t)MMD_ADAPT_STATE_WORDS * n;
    int32_t* cn = c.cnt + 4 * n;
    if (c.mode == 1) {
      const double s = c.params[MMD_ADAPT_P_TT];
      st[MMD_ADAPT_S_S] = s;
      st[MMD_ADAPT_S_H] = c.params[MMD_ADAPT_P_HINIT];
      st[MMD_ADAPT_S_LAM] = sched_lambda_of_la(sched_log_alpha(c.S, s));
      st[MMD_ADAPT_S_E] = 0.0;
      st[MMD_ADAPT_S_LAM0] = sched_lambda_of_la(sched_log_alpha(c.S, t_0));
      st[MMD_ADAPT_S_SPARE] = 0.0;
      cn[MMD_ADAPT_C_ATTEMPTS] = 0;
      cn[MMD_ADAPT_C_ACCEPTED] = 0;
      cn[MMD_ADAPT_C_FLAG] = MMD_ADAPT_FLAG_IDLE;
      cn[MMD_ADAPT_C_DONE] = 0;
    } else {
      if (cn[MMD_ADAPT_C_DONE]) {
        cn[MMD_ADAPT_C_FLAG] = MMD_ADAPT_FLAG_IDLE;
        continue;
      }
      const bool bad = c.batch ? bad_any != 0 : isnan(st[MMD_ADAPT_S_E]);
      if (bad) {      // the state stays as it was: x goes back to XB, nothing else moves, and the host sees the fault bit
        cn[MMD_ADAPT_C_FLAG] = MMD_ADAPT_FLAG_REJECT;
        fault = 1;
        ++active;
        continue;
      }
      const float E = c.batch ? emax : (float)st[MMD_ADAPT_S_E];
      if (c.batch) st[MMD_ADAPT_S_E] = (double)E;
      cn[MMD_ADAPT_C_ATTEMPTS] += 1;
      if (E <= 1.f) {
        st[MMD_ADAPT_S_S] = st[MMD_ADAPT_S_T];
        st[MMD_ADAPT_S_LAM] = sched_lambda_of_la(sched_log_alpha(c.S, st[MMD_ADAPT_S_T]));
        cn[MMD_ADAPT_C_ACCEPTED] += 1;
        cn[MMD_ADAPT_C_FLAG] = MMD_ADAPT_FLAG_ACCEPT;
      } else {
        cn[MMD_ADAPT_C_FLAG] = MMD_ADAPT_FLAG_REJECT;
      }
      st[MMD_ADAPT_S_H] = fmin(theta * st[MMD_ADAPT_S_H] * (1.0 / sqrt((double)E)), st[MMD_ADAPT_S_LAM0] - st[MMD_ADAPT_S_LAM]);
    }
    if (fabs(st[MMD_ADAPT_S_S] - t_0) <= t_err) {      // finished: its row index leaves the tables and no kernel writes it again
      cn[MMD_ADAPT_C_DONE] = 1;
      c.itab[n] = -1;
      if (c.mode == 1) adapt_write_rows(c, n);        // rows and timesteps are defined even for a loop that starts at its end
      continue;
    }
    c.itab[n] = n;
    adapt_write_rows(c, n);
    ++active;
  }
  s_act[tid] = active;
  s_bad[tid] = fault;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      s_act[tid] += s_act[tid + o];
      s_bad[tid] |= s_bad[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    c.status[0] = s_act[0];
    c.status[1] = (c.mode == 1 ? 0 : c.status[1]) | s_bad[0];
  }
}

extern "C" int mmd_dpm_adapt_control(int mode, int batch, const double* params, const double* log_alpha, int T, const double* partial_v,
                                     int chunks_v, int64_t per_v, const double* partial_a, int chunks_a, int64_t per_a, double* state,
                                     int64_t* itab, int32_t* cnt, float* ftab, int32_t* status, int N, void* stream) {
  MMD_REQUIRE(mode == 0 || mode == 1, "dpm_adapt_control: mode is 0 (a trial's end) or 1 (init); got %d", mode);
  MMD_REQUIRE(params && log_alpha && state && itab && cnt && ftab && status,
              "dpm_adapt_control: needs the parameter block, the log alpha table, state, itab, cnt, ftab and status");
  MMD_REQUIRE(N > 0 && N <= 65535 && T >= 2, "dpm_adapt_control: N must be in [1, 65535] and the table hold at least 2 knots; got N %d T %d", N, T);
  if (mode == 0) {
    MMD_REQUIRE(partial_v && chunks_v > 0 && per_v > 0, "dpm_adapt_control: needs the first stream's partial sums, chunks > 0 and per > 0");
    MMD_REQUIRE(partial_a ? (chunks_a > 0 && per_a > 0) : chunks_a == 0, "dpm_adapt_control: the second stream needs chunks > 0 and per > 0 (or no partial sums and chunks 0)");
  }
  const AdaptCtl c{mode, batch ? 1 : 0, N, params, AdaptSchedule{log_alpha, T}, partial_v, mode == 0 ? chunks_v : 0, (double)per_v,
                   partial_a, mode == 0 && partial_a ? chunks_a : 0, (double)per_a, state, itab, cnt, ftab, status};
  return mmd_launch<dpm_adapt_control_kernel>("dpm_adapt_control", dim3(1), dim3(256), 0, (hipStream_t)stream, c);
}

// dst[n] = src[n]: the model timesteps of the coming evaluation (itab row 1 or 2) into the U-Net's timestep buffer, which both
// evaluations of a trial share.  (mmd_copy2d moves 16-byte rows; N int64 words are 8 N bytes.)
__global__ __launch_bounds__(256) void dpm_adapt_time_kernel(const int64_t* __restrict__ src, int64_t* __restrict__ dst, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) dst[i] = src[i];
}
extern "C" int mmd_dpm_adapt_time(const int64_t* src, int64_t* dst, int N, void* stream) {
  MMD_REQUIRE(src && dst && N > 0 && N <= 65535, "dpm_adapt_time: needs src, dst and N in [1, 65535]");
  MMD_REQUIRE((uintptr_t)src + (uintptr_t)N * 8 <= (uintptr_t)dst || (uintptr_t)dst + (uintptr_t)N * 8 <= (uintptr_t)src, "dpm_adapt_time: src and dst overlap");
  return mmd_launch<dpm_adapt_time_kernel>("dpm_adapt_time", dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, N);
}
