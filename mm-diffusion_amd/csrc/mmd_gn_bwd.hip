// GroupNorm backward of the training step: backward of y = act((x - mu) rstd gamma (1 + scale) ... ) in the fused-affine form of mmd_norm.hip.
// Forward (mmd_norm.hip): v = x*a[s,c] + b[s,c], y = act(v) with a = rstd*gamma*(1+sc), b = (beta - mu*rstd*gamma)(1+sc) + sh.
// With z = (x - mu) rstd:   P[s,c] = sum_rows dv,  Q[s,c] = sum_rows dv*z   (dv = dy * act'(v))
//   dshift = P, dscale = gamma*Q + beta*P, dbeta += (1+sc) P, dgamma += (1+sc) Q
//   dx = rstd * ( (1+sc) gamma dv - mean_g[(1+sc) gamma P]/... )   -> per (slice, group) m1 = sum_c g_c P_c / cnt, m2 = sum_c g_c Q_c / cnt
//   dx = rstd * (g_c dv - m1 - z m2),  g_c = (1+sc_c) gamma_c
// P / Q and dgamma / dbeta are accumulated with fp32 L2 atomics (run-to-run bit differences of the last ulp are possible); dx and dfilm
// are deterministic given P and Q.
#include "mmd_common.h"

struct GnBwdGeom {
  int S, Tn, inner;
  int64_t outer_stride, inner_stride, tstride;
};
__device__ __forceinline__ int64_t gnb_base(const GnBwdGeom& g, int s) {
  return (int64_t)(s / g.inner) * g.outer_stride + (int64_t)(s % g.inner) * g.inner_stride;
}

// ----------------------------------------------------------------------------- the row walk of the reduce and apply stages
// block = (row chunk, slice, column chunk), thread = (channel vector `col` of the row, row lane `rl` of RPP).  gridDim.z column chunks of
// CW channels each (1 chunk unless a row is more than 256 16-byte vectors: fp32 above 1024 channels).
template <typename T>
struct GnbThread {
  static constexpr int EPV = Elt<T>::EPV, ES = 16 / EPV;
  int CW, RPP, col, rl;
  __device__ __forceinline__ GnbThread(int C) {
    CW = C / (int)gridDim.z;
    const int CV = CW / EPV;
    RPP = 256 / CV;
    col = (int)blockIdx.z * CV + (int)threadIdx.x % CV;
    rl = (int)threadIdx.x / CV;
  }
  // body(x vector, dy vector, row) for this thread's rows j0 + rl, + RPP, ... below j1 of the slice at `base`: two rows in flight, both
  // operands of both rows loaded before either body runs, then the single-row tail.
  template <class F>
  __device__ __forceinline__ void walk(const char* __restrict__ x, int64_t ldx, const char* __restrict__ dy, int64_t lddy, const GnBwdGeom& g,
                                       int64_t base, int j0, int j1, F&& body) const {
    int j = j0 + rl;
    for (; j + RPP < j1; j += 2 * RPP) {
      const int64_t r0 = base + (int64_t)j * g.tstride, r1 = base + (int64_t)(j + RPP) * g.tstride;
      const u32x4 x0 = *(const u32x4*)(x + (r0 * ldx + col * EPV) * ES);
      const u32x4 d0 = *(const u32x4*)(dy + (r0 * lddy + col * EPV) * ES);
      const u32x4 x1 = *(const u32x4*)(x + (r1 * ldx + col * EPV) * ES);
      const u32x4 d1 = *(const u32x4*)(dy + (r1 * lddy + col * EPV) * ES);
      body(x0, d0, r0);
      body(x1, d1, r1);
    }
    if (j < j1) {
      const int64_t r0 = base + (int64_t)j * g.tstride;
      body(*(const u32x4*)(x + (r0 * ldx + col * EPV) * ES), *(const u32x4*)(dy + (r0 * lddy + col * EPV) * ES), r0);
    }
  }
};

// stage 1: per (slice, row chunk) partial P, Q per channel -> atomics into PQ[S][C][2] (fp32)
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const char* __restrict__ x, int64_t ldx, const char* __restrict__ dy, int64_t lddy,
                                                            int C, GnBwdGeom g, const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ mr, int act, int R, float* __restrict__ PQ) {
  constexpr int EPV = Elt<T>::EPV;
  __shared__ float s_p[256 * EPV], s_q[256 * EPV];
  const int s = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const GnbThread<T> th(C);
  const int CW = th.CW, RPP = th.RPP, col = th.col, rl = th.rl, c0 = (int)blockIdx.z * CW;
  const int cpg = C / 32;
  const int64_t base = gnb_base(g, s);
  float P[EPV], Q[EPV], av[EPV], bv[EPV], mu[EPV], rs[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const int c = col * EPV + e;
    P[e] = Q[e] = 0.f;
    av[e] = a[(int64_t)s * C + c];
    bv[e] = b[(int64_t)s * C + c];
    mu[e] = mr[((int64_t)s * 32 + c / cpg) * 2];
    rs[e] = mr[((int64_t)s * 32 + c / cpg) * 2 + 1];
  }
  if (rl < RPP) {
    th.walk(x, ldx, dy, lddy, g, base, chunk * R, min(chunk * R + R, g.Tn), [&](const u32x4& vx, const u32x4& vd, int64_t) {
      float fx[EPV], fd[EPV];
      Elt<T>::unpack(vx, fx);
      Elt<T>::unpack(vd, fd);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        float dv = fd[e];
        if (act) dv *= dsilu_f(fx[e] * av[e] + bv[e]);
        P[e] += dv;
        Q[e] += dv * (fx[e] - mu[e]) * rs[e];
      }
    });
#pragma unroll
    for (int e = 0; e < EPV; ++e) { s_p[rl * CW + col * EPV - c0 + e] = P[e]; s_q[rl * CW + col * EPV - c0 + e] = Q[e]; }
  }
  __syncthreads();
  for (int c = tid; c < CW; c += 256) {
    float pa = 0.f, qa = 0.f;
    for (int r = 0; r < RPP; ++r) { pa += s_p[r * CW + c]; qa += s_q[r * CW + c]; }
    atomicAdd(PQ + ((int64_t)s * C + c0 + c) * 2, pa);
    atomicAdd(PQ + ((int64_t)s * C + c0 + c) * 2 + 1, qa);
  }
}

// stage 2: parameter / FiLM gradients and the per-(slice, group) means m1, m2   (one block per slice)
__global__ __launch_bounds__(256) void gn_bwd_params_kernel(float* __restrict__ PQ, int C, int Tn, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ film, int64_t film_ld,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dfilm,
                                                            int64_t dfilm_ld, float* __restrict__ m12, int rezero) {
  // round 6: grid (4, S) - a block owns 8 groups = 8 cpg <= 256 channels, one per thread (it was one block per slice looping over C);
  // above 1024 channels grid (8, S): 4 groups = 4 cpg <= 256 channels per block
  __shared__ float s_g1[256], s_g2[256];
  const int GPB = 32 / (int)gridDim.x;
  const int s = blockIdx.y, g0 = blockIdx.x * GPB, tid = threadIdx.x;
  const int cpg = C / 32, nch = GPB * cpg;
  if (tid < nch) {
    const int c = g0 * cpg + tid;
    const float P = PQ[((int64_t)s * C + c) * 2], Q = PQ[((int64_t)s * C + c) * 2 + 1];
    if (rezero) {                        // mmd_gn_bwd_ws0: the accumulators go back to zero for the next call on this workspace
      PQ[((int64_t)s * C + c) * 2] = 0.f;
      PQ[((int64_t)s * C + c) * 2 + 1] = 0.f;
    }
    const float sc1 = film ? 1.f + film[(int64_t)s * film_ld + c] : 1.f;
    const float gc = sc1 * gamma[c];
    s_g1[tid] = gc * P;
    s_g2[tid] = gc * Q;
    atomicAdd(dgamma + c, sc1 * Q);
    atomicAdd(dbeta + c, sc1 * P);
    if (dfilm) {
      dfilm[(int64_t)s * dfilm_ld + c] = gamma[c] * Q + beta[c] * P;        // d scale
      dfilm[(int64_t)s * dfilm_ld + C + c] = P;                             // d shift
    }
  }
  __syncthreads();
  if (tid < GPB) {
    float a1 = 0.f, a2 = 0.f;
    for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a1 += s_g1[c]; a2 += s_g2[c]; }
    const float cnt = (float)Tn * (float)cpg;
    m12[((int64_t)s * 32 + g0 + tid) * 2] = a1 / cnt;
    m12[((int64_t)s * 32 + g0 + tid) * 2 + 1] = a2 / cnt;
  }
}

// stage 3: dx = rstd * (g_c dv - m1 - z m2) = k1 dv + k2 x + k3 with per-(slice, channel) coefficients held in registers
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const char* __restrict__ x, int64_t ldx, const char* __restrict__ dy, int64_t lddy,
                                                           char* __restrict__ dx, int64_t lddx, int C, GnBwdGeom g,
                                                           const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mr,
                                                           const float* __restrict__ m12, const float* __restrict__ gamma,
                                                           const float* __restrict__ film, int64_t film_ld, int act, int R) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  const int s = blockIdx.y, chunk = blockIdx.x;
  const GnbThread<T> th(C);
  const int col = th.col, cpg = C / 32;
  if (th.rl >= th.RPP) return;
  const int64_t base = gnb_base(g, s);
  float av[EPV], bv[EPV], k1[EPV], k2[EPV], k3[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const int c = col * EPV + e, gi = c / cpg;
    av[e] = a[(int64_t)s * C + c];
    bv[e] = b[(int64_t)s * C + c];
    const float mu = mr[((int64_t)s * 32 + gi) * 2], rs = mr[((int64_t)s * 32 + gi) * 2 + 1];
    const float m1 = m12[((int64_t)s * 32 + gi) * 2], m2 = m12[((int64_t)s * 32 + gi) * 2 + 1];
    const float gc = (film ? 1.f + film[(int64_t)s * film_ld + c] : 1.f) * gamma[c];
    k1[e] = rs * gc;
    k2[e] = -rs * rs * m2;
    k3[e] = rs * (mu * rs * m2 - m1);
  }
  th.walk(x, ldx, dy, lddy, g, base, chunk * R, min(chunk * R + R, g.Tn), [&](const u32x4& vx, const u32x4& vd, int64_t row) {
    float fx[EPV], fd[EPV], out[EPV];
    Elt<T>::unpack(vx, fx);
    Elt<T>::unpack(vd, fd);
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      float dv = fd[e];
      if (act) dv *= dsilu_f(fx[e] * av[e] + bv[e]);
      out[e] = k1[e] * dv + k2[e] * fx[e] + k3[e];
    }
    *(u32x4*)(dx + (row * lddx + col * EPV) * ES) = Elt<T>::pack(out);
  });
}

__global__ __launch_bounds__(256) void zero_f32_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.f;
}

// ============================================================================= C-ABI
// GroupNorm(+FiLM)(+SiLU) backward.  a, b [S,C] and mr [S,32,2] (mean, rstd) come from the forward mmd_gn_stats.
// dgamma / dbeta fp32 [C] are ACCUMULATED (caller zeroes); dfilm (nullable) [S, >= 2C] receives (dscale | dshift);
// workspace: (S*C*2 + S*64) floats, zeroed by this call.
static int gn_bwd_impl(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int64_t rows, int C,
                       int S, int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a,
                       const float* b, const float* mr, const float* gamma, const float* beta, const float* film, int64_t film_ld,
                       int act, float* dgamma, float* dbeta, float* dfilm, int64_t dfilm_ld, float* workspace, void* stream, bool ws0) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "gn_bwd: bad dtype");
  MMD_REQUIRE(x && dy && dx && a && b && mr && gamma && beta && dgamma && dbeta && workspace, "gn_bwd: null pointer");
  MMD_REQUIRE(C > 0 && C % 32 == 0 && C % epv == 0 && C <= 2048, "gn_bwd: unsupported channel count %d (a multiple of 32 and of the 16-byte vector, at most 2048)", C);
  MMD_REQUIRE(S > 0 && S <= 65535, "gn_bwd: %d slices (the slice index is a grid y coordinate: at most 65535)", S);
  // column chunks: a block covers at most 256 16-byte vectors of a row, so fp32 rows above 1024 channels go in two halves (C % 32 == 0
  // keeps a half a whole number of vectors); one chunk - today's launch shapes - for every C <= 1024 and every bf16 C <= 2048
  const int NZ = C / epv <= 256 ? 1 : 2;
  const int CW = C / NZ;
  GnBwdGeom g{S, Tn, inner, outer_stride, inner_stride, tstride};
  hipStream_t st = (hipStream_t)stream;
  float* PQ = workspace;
  float* m12 = workspace + (int64_t)S * C * 2;
  // zeroed by a kernel, not hipMemsetAsync: memset nodes of a captured graph were observed to lose their ordering against the
  // neighbouring kernel nodes on replay (train_graph.py), a fill kernel is an ordinary node of the chain
  if (!ws0) {
    if (int zrc = mmd_launch<zero_f32_kernel>("gn_bwd_zero", dim3(ew_grid((int64_t)S * C * 2)), dim3(256), 0, st, PQ, (int64_t)S * C * 2)) return zrc;
  }
  const int rpp = max(1, 256 / (CW / epv));
  int R = 4 * rpp;
  while ((int64_t)S * cdiv(Tn, R) > 1280 && R < 1024) R *= 2;
  dim3 grid(cdiv(Tn, R), S, NZ);
  int rc = mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<gn_bwd_reduce_kernel<typename decltype(t)::type>>("gn_bwd_reduce", grid, dim3(256), 0, st, (const char*)x, ldx, (const char*)dy, lddy, C,
                                                                        g, a, b, mr, act, R, PQ);
  });
  if (rc) return rc;
  rc = mmd_launch<gn_bwd_params_kernel>("gn_bwd_params", dim3(C <= 1024 ? 4 : 8, S), dim3(256), 0, st, PQ, C, Tn, gamma, beta, film, film_ld, dgamma, dbeta,
                                        dfilm, dfilm_ld, m12, ws0 ? 1 : 0);
  if (rc) return rc;
  int R3 = 4 * rpp;
  while ((int64_t)S * cdiv(Tn, R3) > 4096 && R3 < 1024) R3 *= 2;
  dim3 grid3(cdiv(Tn, R3), S, NZ);
  (void)rows;
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<gn_bwd_apply_kernel<typename decltype(t)::type>>("gn_bwd_apply", grid3, dim3(256), 0, st, (const char*)x, ldx, (const char*)dy, lddy,
                                                                       (char*)dx, lddx, C, g, a, b, mr, (const float*)m12, gamma, film, film_ld, act, R3);
  });
}

extern "C" int mmd_gn_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int64_t rows, int C,
                          int S, int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a,
                          const float* b, const float* mr, const float* gamma, const float* beta, const float* film, int64_t film_ld,
                          int act, float* dgamma, float* dbeta, float* dfilm, int64_t dfilm_ld, float* workspace, void* stream) {
  return gn_bwd_impl(dtype, x, ldx, dy, lddy, dx, lddx, rows, C, S, Tn, inner, outer_stride, inner_stride, tstride, a, b, mr, gamma, beta, film,
                     film_ld, act, dgamma, dbeta, dfilm, dfilm_ld, workspace, stream, false);
}
// The same with a workspace the CALLER keeps: its first S * C * 2 floats are zero on entry and zero again on exit (the parameter stage
// clears what it has read), so a training step's 243 norms do not pay a fill launch each.  One workspace per stream AND per S * C:
// the group means live behind the accumulators, at workspace + S * C * 2, and are NOT cleared, so a buffer of the same total length
// handed to a norm with another S * C (S = 6, C = 32 and S = 2, C = 160 are both 768 floats) is not zero where that norm accumulates.
extern "C" int mmd_gn_bwd_ws0(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int64_t rows, int C,
                              int S, int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a,
                              const float* b, const float* mr, const float* gamma, const float* beta, const float* film, int64_t film_ld,
                              int act, float* dgamma, float* dbeta, float* dfilm, int64_t dfilm_ld, float* workspace, void* stream) {
  return gn_bwd_impl(dtype, x, ldx, dy, lddy, dx, lddx, rows, C, S, Tn, inner, outer_stride, inner_stride, tstride, a, b, mr, gamma, beta, film,
                     film_ld, act, dgamma, dbeta, dfilm, dfilm_ld, workspace, stream, true);
}
