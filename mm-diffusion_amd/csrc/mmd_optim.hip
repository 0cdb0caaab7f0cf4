// Optimizer side of the training step: AdamW (+EMA) on the flat parameter buffer, the training step guard (gradient / parameter norms,
// non-finite skip, clipping) and the per-step conv weight pack / gradient unpack.  Everything here is deterministic: the norms are
// per-block partials in double folded in a fixed order, no atomics on floating-point data.
#include "mmd_common.h"

// ----------------------------------------------------------------------------- AdamW
// One element of the AdamW step (torch.optim.AdamW semantics: decoupled weight decay) on the gradient g[i] * clip; returns the new weight.
// p[i] is read before g[i]: with -ffp-contract=fast the order of the loads decides which product of each moment update is fused.
__device__ __forceinline__ float adamw_elem(float* __restrict__ p, const float* __restrict__ g, float clip, float* __restrict__ m,
                                            float* __restrict__ v, int64_t i, float lr, float beta1, float beta2, float eps, float wd,
                                            float bc1, float bc2) {
  float w = p[i] * (1.f - lr * wd);
  const float gi = g[i] * clip;
  const float mi = beta1 * m[i] + (1.f - beta1) * gi;
  const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  w -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
  p[i] = w;
  return w;
}

// AdamW step + optional EMA update (nn.py:128-138)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ ema, int64_t n, float lr, float beta1, float beta2, float eps, float wd,
                                                    float bc1, float bc2, float ema_rate) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float w = adamw_elem(p, g, 1.f, m, v, i, lr, beta1, beta2, eps, wd, bc1, bc2);
    if (ema) ema[i] = ema[i] * ema_rate + w * (1.f - ema_rate);
  }
}

// ----------------------------------------------------------------------------- training step guard (include/mmd.h: mmd_step_ctrl)
// Three launches in stream order, the reduction pattern of loss_terms_kernel / loss_finalize_kernel (mmd_diffusion.hip): per-block partials
// in double, folded in ascending order by a second launch.  No block waits for or signals another one.
// One block per chunk: every thread sums its elements in ascending order, then a fixed tree over the 256 threads.  The chunk start is
// only element aligned (chunks are cut at parameter boundaries): up to 3 head elements, 16-byte vectors, up to 3 tail elements.
__global__ __launch_bounds__(256) void sumsq_chunks_kernel(const float* __restrict__ g, const float* __restrict__ p, int64_t n,
                                                           const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_len,
                                                           double* __restrict__ partial) {
  __shared__ double s_g[256], s_p[256];
  const int tid = threadIdx.x;
  int64_t lo = chunk_lo[blockIdx.x];
  int64_t hi = lo + chunk_len[blockIdx.x];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  const int len = hi > lo ? (int)(hi - lo) : 0;
  const int head = min(len, (int)((4 - (lo & 3)) & 3));          // g and p are 16-byte aligned (checked by the caller side)
  const int nvec = (len - head) >> 2;
  const int tail = len - head - 4 * nvec;
  double sg = 0.0, sp = 0.0;
  if (tid < head) {
    const double a = (double)g[lo + tid];
    sg += a * a;
    if (p) { const double b = (double)p[lo + tid]; sp += b * b; }
  }
  const float4* gv = (const float4*)(g + lo + head);
  const float4* pv = p ? (const float4*)(p + lo + head) : nullptr;
  for (int i = tid; i < nvec; i += 256) {
    const float4 a = gv[i];
    sg += (double)a.x * (double)a.x;
    sg += (double)a.y * (double)a.y;
    sg += (double)a.z * (double)a.z;
    sg += (double)a.w * (double)a.w;
    if (pv) {
      const float4 b = pv[i];
      sp += (double)b.x * (double)b.x;
      sp += (double)b.y * (double)b.y;
      sp += (double)b.z * (double)b.z;
      sp += (double)b.w * (double)b.w;
    }
  }
  if (tid < tail) {
    const int64_t i = lo + head + 4 * (int64_t)nvec + tid;
    const double a = (double)g[i];
    sg += a * a;
    if (p) { const double b = (double)p[i]; sp += b * b; }
  }
  s_g[tid] = sg;
  s_p[tid] = sp;
  block_tree_sum256(tid, s_g, s_p);
  if (tid == 0) {
    partial[(int64_t)blockIdx.x * 2] = s_g[0];
    partial[(int64_t)blockIdx.x * 2 + 1] = s_p[0];
  }
}

__device__ __forceinline__ bool sg_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for inf and nan

// One block.  Thread i folds the chunks of parameters i, i + 256, ... in ascending order; the totals are each thread's parameters in
// ascending order, then the same fixed tree.  Thread 0 advances the control block.
__global__ __launch_bounds__(256) void step_control_kernel(const double* __restrict__ partial, const int32_t* __restrict__ first_chunk, int P,
                                                           double* __restrict__ param_sumsq, float max_grad_norm, float beta1, float beta2,
                                                           mmd_step_ctrl* __restrict__ ctrl) {
  __shared__ double s_g[256], s_p[256];
  __shared__ int s_bad[256];
  const int tid = threadIdx.x;
  double tg = 0.0, tp = 0.0;
  int bad = 0x7fffffff;
  for (int i = tid; i < P; i += 256) {
    double a = 0.0, b = 0.0;
    const int c1 = first_chunk[i + 1];
    for (int c = first_chunk[i]; c < c1; ++c) { a += partial[(int64_t)c * 2]; b += partial[(int64_t)c * 2 + 1]; }
    param_sumsq[(int64_t)i * 2] = a;
    param_sumsq[(int64_t)i * 2 + 1] = b;
    tg += a;
    tp += b;
    if (!sg_finite(a) && i < bad) bad = i;
  }
  s_g[tid] = tg;
  s_p[tid] = tp;
  s_bad[tid] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {      // block_tree_sum256's order, written out: the first bad parameter folds with min in the same levels
    if (tid < o) {
      s_g[tid] += s_g[tid + o];
      s_p[tid] += s_p[tid + o];
      s_bad[tid] = min(s_bad[tid], s_bad[tid + o]);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double gsum = s_g[0], psum = s_p[0];
  const bool ok = sg_finite(gsum);
  const float gn = (float)sqrt(gsum), pn = (float)sqrt(psum);
  ctrl->grad_norm = gn;
  ctrl->param_norm = pn;
  ctrl->took_step = ok ? 1 : 0;
  ctrl->first_bad_param = ok ? -1 : s_bad[0];
  if (ok) {
    const int steps = ctrl->steps_taken + 1;
    ctrl->steps_taken = steps;
    ctrl->bc1 = (float)(1.0 - pow((double)beta1, (double)steps));
    ctrl->bc2 = (float)(1.0 - pow((double)beta2, (double)steps));
    ctrl->clip_coef = (max_grad_norm > 0.f && gn > max_grad_norm) ? max_grad_norm / (gn + 1e-6f) : 1.f;
    ctrl->cum_grad_norm += sqrt(gsum);
    ctrl->cum_param_norm += sqrt(psum);
    ctrl->cum_count += 1;
  } else {
    ctrl->clip_coef = 1.f;
    ctrl->skipped_total += 1;
    ctrl->last_bad_param = s_bad[0];
  }
}

struct EmaSet { float* e[MMD_STEP_MAX_EMA]; float rate[MMD_STEP_MAX_EMA]; };
// adamw_kernel's arithmetic on g * clip_coef with the bias corrections of the control block; every EMA copy in the same launch.
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const EmaSet ema, int64_t n, float lr, float beta1, float beta2,
                                                            float eps, float wd, const mmd_step_ctrl* __restrict__ ctrl) {
  if (!ctrl->took_step) return;
  const float clip = ctrl->clip_coef, bc1 = ctrl->bc1, bc2 = ctrl->bc2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float w = adamw_elem(p, g, clip, m, v, i, lr, beta1, beta2, eps, wd, bc1, bc2);
#pragma unroll
    for (int k = 0; k < MMD_STEP_MAX_EMA; ++k)
      if (ema.e[k]) ema.e[k][i] = ema.e[k][i] * ema.rate[k] + w * (1.f - ema.rate[k]);
  }
}

// ============================================================================= C-ABI
extern "C" int mmd_adamw_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, float ema_rate, void* stream) {
  MMD_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw_step: bad argument");
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  return mmd_launch<adamw_kernel>("adamw_step", dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay,
                                  bc1, bc2, ema_rate);
}

extern "C" int mmd_step_ctrl_bytes(void) { return (int)sizeof(mmd_step_ctrl); }

extern "C" int mmd_sumsq_chunks(const float* g, const float* p, int64_t n, const int64_t* chunk_lo, const int32_t* chunk_len, int nchunks,
                                double* partial, void* stream) {
  MMD_REQUIRE(g && chunk_lo && chunk_len && partial && n > 0 && nchunks > 0, "sumsq_chunks: bad argument");
  MMD_REQUIRE(((uintptr_t)g | (uintptr_t)p) % 16 == 0 && (uintptr_t)partial % 8 == 0, "sumsq_chunks: unaligned pointer");
  return mmd_launch<sumsq_chunks_kernel>("sumsq_chunks", dim3(nchunks), dim3(256), 0, (hipStream_t)stream, g, p, n, chunk_lo, chunk_len, partial);
}

extern "C" int mmd_step_control(const double* partial, const int32_t* param_first_chunk, int P, double* param_sumsq, float max_grad_norm,
                                float beta1, float beta2, struct mmd_step_ctrl* ctrl, void* stream) {
  MMD_REQUIRE(partial && param_first_chunk && param_sumsq && ctrl && P > 0, "step_control: bad argument");
  MMD_REQUIRE(((uintptr_t)partial | (uintptr_t)param_sumsq | (uintptr_t)ctrl) % 8 == 0, "step_control: unaligned pointer");
  MMD_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "step_control: betas must be in [0, 1)");
  return mmd_launch<step_control_kernel>("step_control", dim3(1), dim3(256), 0, (hipStream_t)stream, partial, param_first_chunk, P, param_sumsq,
                                         max_grad_norm, beta1, beta2, ctrl);
}

extern "C" int mmd_adamw_step_guarded(float* p, const float* g, float* m, float* v, float* ema0, float* ema1, float* ema2, float* ema3,
                                      float rate0, float rate1, float rate2, float rate3, int64_t n, float lr, float beta1, float beta2,
                                      float eps, float weight_decay, const struct mmd_step_ctrl* ctrl, void* stream) {
  MMD_REQUIRE(p && g && m && v && ctrl && n > 0, "adamw_step_guarded: bad argument");
  MMD_REQUIRE((uintptr_t)ctrl % 8 == 0, "adamw_step_guarded: unaligned control block");
  EmaSet ema;
  ema.e[0] = ema0; ema.e[1] = ema1; ema.e[2] = ema2; ema.e[3] = ema3;
  ema.rate[0] = rate0; ema.rate[1] = rate1; ema.rate[2] = rate2; ema.rate[3] = rate3;
  return mmd_launch<adamw_guarded_kernel>("adamw_step_guarded", dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, lr, beta1,
                                          beta2, eps, weight_decay, ctrl);
}

// ----------------------------------------------------------------------------- weight packing for the training step
// One launch re-packs EVERY conv weight after an optimizer step: src fp32 [Cout][Cin][nt] (torch conv layout, a view of the
// flat parameter buffer) -> fwd [Cout][nt*Cin] (GEMM operand of the forward conv) and bwd [Cin][nt*Cout] (operand of the
// data-gradient conv) in the activation dtype.  The per-weight torch version was ~6 tiny kernels per conv per step.
struct PackDesc {
  const float* src; void* fwd; void* bwd;
  int Cout, Cin, nt;
  int block_start;                 // first block of this weight; a block covers a tile of 32 output x 16 input channels x all taps
};
// Round 6: tiles through LDS.  The first version walked 2048 consecutive source elements per block and stored each one twice with 2-byte
// stores Cin / Cout elements apart, behind a nine-deep dependent binary search of the descriptor table per block (2.07 ms per step for
// the 133 M parameters = 0.39 TB/s of traffic that should take 0.2 ms).  A tile of 32 co x (216 / nt) ci x nt taps is read as 32 contiguous
// runs, then written as runs of consecutive ci per (co, tap) into the forward operand and runs of 32 consecutive co per (ci, tap) into
// the data-gradient operand; no integer division in the loops; the descriptor of a block is found by ONE parallel pass over the table.
#define PK_CO 32
#define PK_ROW 216
#define PK_NT_MAX 27
__host__ __device__ __forceinline__ int pack_ci_tile(int nt) { const int c = PK_ROW / nt; return c >= 16 ? (c & ~15) : c; }
__device__ __forceinline__ PackDesc pack_find(const PackDesc* __restrict__ descs, int n, int* s_cnt) {
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  int local = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) local += descs[i].block_start <= (int)blockIdx.x ? 1 : 0;   // block_start ascends
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(s_cnt, local);
  __syncthreads();
  return descs[*s_cnt - 1];
}
struct PackTile { int co0, ci0, nco, nci, nt, run; };
__device__ __forceinline__ PackTile pack_tile(const PackDesc& d) {
  const int ct = pack_ci_tile(d.nt);
  const int tiles_ci = (d.Cin + ct - 1) / ct;
  const int tb = (int)blockIdx.x - d.block_start;
  PackTile t;
  t.co0 = (tb / tiles_ci) * PK_CO;
  t.ci0 = (tb % tiles_ci) * ct;
  t.nco = min(PK_CO, d.Cout - t.co0);
  t.nci = min(ct, d.Cin - t.ci0);
  t.nt = d.nt;
  t.run = t.nci * d.nt;
  return t;
}
template <typename T>
__global__ __launch_bounds__(256) void pack_weights_kernel(const PackDesc* __restrict__ descs, int n) {
  __shared__ float sT[PK_CO][PK_ROW + 1];
  __shared__ int s_cnt;
  const PackDesc d = pack_find(descs, n, &s_cnt);
  const PackTile t = pack_tile(d);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = wave; c < t.nco; c += 4) {
    const float* sp = d.src + ((int64_t)(t.co0 + c) * d.Cin + t.ci0) * t.nt;
    for (int r = lane; r < t.run; r += 64) sT[c][r] = sp[r];
  }
  __syncthreads();
  // forward operand [Cout][nt * Cin]: lanes along ci; a tile narrower than a wave (16 ci at nine taps) puts 64 / nci taps side by side
  const int tstep = t.nci >= 64 ? 1 : 64 / t.nci, lt = lane / t.nci, lci = lane - lt * t.nci, cstep = tstep > 1 ? t.nci : 64;
  if (lt < tstep)
    for (int c = wave; c < t.nco; c += 4)
      for (int tap = lt; tap < t.nt; tap += tstep) {
        const int64_t base = (int64_t)(t.co0 + c) * t.nt * d.Cin + (int64_t)tap * d.Cin + t.ci0;
        for (int ci = lci; ci < t.nci; ci += cstep) Elt<T>::st(d.fwd, base + ci, sT[c][ci * t.nt + tap]);
      }
  const int c = lane & 31, h = lane >> 5;                      // data-gradient operand [Cin][nt * Cout]: lanes along co, two taps per wave pass
  if (c < t.nco)
    for (int ci = wave; ci < t.nci; ci += 4)
      for (int tap = h; tap < t.nt; tap += 2)
        Elt<T>::st(d.bwd, (int64_t)(t.ci0 + ci) * t.nt * d.Cout + (int64_t)tap * d.Cout + t.co0 + c, sT[c][ci * t.nt + tap]);
}
// Reverse direction for the gradients: wgrad accumulates with COALESCED atomics in the packed layout [Cout][nt*Cin] (fp32, `fwd` of
// the record); once per step this adds every packed gradient into the parameter's .grad ([Cout][Cin][nt], `src` of the record,
// written here) and clears the packed buffer for the next step.  (Atomics straight into the torch layout are strided by nt
// floats: 18 64-byte segments per wave instruction instead of 2.)  Same tiles as the weight pack: packed runs of consecutive ci per
// (co, tap) in, .grad runs of nci x nt floats per co out.
__global__ __launch_bounds__(256) void unpack_grads_kernel(const PackDesc* __restrict__ descs, int n) {
  __shared__ float sT[PK_CO][PK_ROW + 1];
  __shared__ int s_cnt;
  const PackDesc d = pack_find(descs, n, &s_cnt);
  const PackTile t = pack_tile(d);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* grad = const_cast<float*>(d.src);
  float* packed = (float*)d.fwd;
  const int tstep = t.nci >= 64 ? 1 : 64 / t.nci, lt = lane / t.nci, lci = lane - lt * t.nci, cstep = tstep > 1 ? t.nci : 64;
  if (lt < tstep)
    for (int c = wave; c < t.nco; c += 4)
      for (int tap = lt; tap < t.nt; tap += tstep) {
        float* pp = packed + (int64_t)(t.co0 + c) * t.nt * d.Cin + (int64_t)tap * d.Cin + t.ci0;
        for (int ci = lci; ci < t.nci; ci += cstep) {
          sT[c][ci * t.nt + tap] = pp[ci];
          pp[ci] = 0.f;
        }
      }
  __syncthreads();
  for (int c = wave; c < t.nco; c += 4) {
    float* gp = grad + ((int64_t)(t.co0 + c) * d.Cin + t.ci0) * t.nt;
    for (int r = lane; r < t.run; r += 64) gp[r] += sT[c][r];
  }
}

extern "C" int mmd_pack_blocks(int Cout, int Cin, int nt) {
  if (Cout <= 0 || Cin <= 0 || nt <= 0 || nt > PK_NT_MAX) return -1;
  const int ct = pack_ci_tile(nt);
  return ((Cout + PK_CO - 1) / PK_CO) * ((Cin + ct - 1) / ct);
}

extern "C" int mmd_unpack_conv_grads(const void* descs_dev, int n, int total_blocks, void* stream) {
  MMD_REQUIRE(descs_dev && n > 0 && total_blocks > 0, "unpack_conv_grads: bad argument");      // (descriptors: at most 27 taps, mmd_pack_blocks blocks each)
  return mmd_launch<unpack_grads_kernel>("unpack_conv_grads", dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const PackDesc*)descs_dev, n);
}

extern "C" int mmd_pack_conv_weights(int dtype, const void* descs_dev, int n, int total_blocks, void* stream) {
  MMD_REQUIRE((dtype == MMD_BF16 || dtype == MMD_F32) && descs_dev && n > 0 && total_blocks > 0, "pack_conv_weights: bad argument");
  hipStream_t st = (hipStream_t)stream;
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<pack_weights_kernel<typename decltype(t)::type>>("pack_conv_weights", dim3(total_blocks), dim3(256), 0, st, (const PackDesc*)descs_dev, n);
  });
}
