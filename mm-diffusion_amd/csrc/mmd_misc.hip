// Small kernels around the U-Net that belong to neither a convolution nor the diffusion process:
//   timestep embedding + MLP (nn.py:192-210, multimodal_unet.py:791-795,1075), batched emb_layers Linear (unet:366-372),
//   avg-pool / nearest resampling (unet:133-208) with and without GroupNorm statistics, skip-concat copies (unet:1093-1094) and the
//   gradient payload cast; SiLU, dropout and the MSE gradient of the training step.  The layout-edge convolutions are in mmd_edge.hip, the diffusion process in mmd_diffusion.hip,
//   the DPM-Solver kernels in mmd_dpm.hip.
#include "mmd_common.h"

// ----------------------------------------------------------------------------- timestep embedding + MLP
// one block per sample; out_silu = SiLU(W2 SiLU(W0 e + b0) + b2), out_raw (optional) = without the last SiLU
__global__ __launch_bounds__(256) void temb_kernel(const void* __restrict__ t, int t_kind, int dim, const float* __restrict__ W0,
                                                   const float* __restrict__ b0, const float* __restrict__ W2,
                                                   const float* __restrict__ b2, float* __restrict__ out_silu,
                                                   float* __restrict__ out_raw) {
  extern __shared__ float sm[];
  float* e = sm;          // [dim]
  float* h = sm + dim;    // [dim]
  const int n = blockIdx.x, tid = threadIdx.x;
  float tv;
  if (t_kind == 0) tv = (float)((const int64_t*)t)[n];
  else if (t_kind == 1) tv = (float)((const int32_t*)t)[n];
  else tv = ((const float*)t)[n];
  const int half = dim / 2;
  for (int i = tid; i < dim; i += 256) {
    float v = 0.f;
    if (i < 2 * half) {
      const int k = i < half ? i : i - half;
      const float f = expf(-logf(10000.f) * (float)k / (float)half);
      const float a = tv * f;
      v = i < half ? cosf(a) : sinf(a);
    }
    e[i] = v;
  }
  __syncthreads();
  for (int j = tid; j < dim; j += 256) {
    float a = b0[j];
    for (int k = 0; k < dim; ++k) a += W0[j * dim + k] * e[k];
    h[j] = silu_f(a);
  }
  __syncthreads();
  for (int j = tid; j < dim; j += 256) {
    float a = b2[j];
    for (int k = 0; k < dim; ++k) a += W2[j * dim + k] * h[k];
    if (out_raw) out_raw[n * dim + j] = a;
    out_silu[n * dim + j] = silu_f(a);
  }
}

// y[n, j] = b[j] + sum_k x[n,k] W[j,k] ; one wave per output column j, all n (N <= 16)
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                     const float* __restrict__ b, float* __restrict__ y, int N, int K, int J) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= J) return;
  for (int n0 = 0; n0 < N; n0 += 8) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float w = W[(int64_t)j * K + k];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (n0 + i < N) acc[i] += w * x[(int64_t)(n0 + i) * K + k];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float s = wave_sum(acc[i]);
      if (lane == 0 && n0 + i < N) y[(int64_t)(n0 + i) * J + j] = s + (b ? b[j] : 0.f);
    }
  }
}

// ----------------------------------------------------------------------------- resampling (channels-last rows)
// mode 0: average pool, mode 1: nearest upsample.  Rows are (n, f, h, w) with factors (1, fh, fw) - audio uses
// F=1, H=1, W=L, fw=4.  Geometry given for the INPUT; output dims = in / factor (pool) or in * factor (up).
template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(const char* __restrict__ x, int64_t ldx, char* __restrict__ y, int64_t ldy,
                                                       int C, int NF, int H, int W, int fh, int fw, int mode, float scale) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  const int CV = C / EPV;
  const int Ho = mode == 0 ? H / fh : H * fh, Wo = mode == 0 ? W / fw : W * fw;
  const int64_t total = (int64_t)NF * Ho * Wo * CV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const int64_t orow = i / CV;
    const int wo = (int)(orow % Wo), ho = (int)((orow / Wo) % Ho);
    const int64_t nf = orow / ((int64_t)Wo * Ho);
    float acc[EPV];
    if (mode == 0) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
      for (int a = 0; a < fh; ++a)
        for (int b = 0; b < fw; ++b) {
          const int64_t irow = (nf * H + ho * fh + a) * W + wo * fw + b;
          float f[EPV];
          Elt<T>::unpack(*(const u32x4*)(x + (irow * ldx + (int64_t)cv * EPV) * ES), f);
#pragma unroll
          for (int e = 0; e < EPV; ++e) acc[e] += f[e];
        }
      const float inv = scale / (float)(fh * fw);
#pragma unroll
      for (int e = 0; e < EPV; ++e) acc[e] *= inv;
      *(u32x4*)(y + (orow * ldy + (int64_t)cv * EPV) * ES) = Elt<T>::pack(acc);
    } else {
      const int64_t irow = (nf * H + ho / fh) * W + wo / fw;
      u32x4 v = *(const u32x4*)(x + (irow * ldx + (int64_t)cv * EPV) * ES);
      if (scale != 1.f) {
        Elt<T>::unpack(v, acc);
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] *= scale;
        v = Elt<T>::pack(acc);
      }
      *(u32x4*)(y + (orow * ldy + (int64_t)cv * EPV) * ES) = v;
    }
  }
}

// The same resampling (bf16) with the GroupNorm statistics of the OUTPUT in the epilogue (round 5): one block owns one 64-row RECORD of the
// output, writes its rows and leaves (sum, sum of squares) of the values AS STORED per quad of channels - the record format of the GEMM
// epilogues (mmd_conv_gemm_stats) - so a norm that follows a resample (the out_layers norm of the down ResBlocks, every norm that reads
// an up ResBlock's output, unet:441-448) finalizes from records instead of paying a statistics pass over the tensor.
// Thread (rg, cv) owns channel vector cv (8 channels = two quads) of the rows rg, rg + RGN, ...: per-thread sums in row order, then the
// row groups are folded in ascending order by the rg == 0 threads - a fixed order, bitwise repeatable and independent of the grid.
__global__ __launch_bounds__(256) void resample_stats_kernel(const char* __restrict__ x, int64_t ldx, char* __restrict__ y, int64_t ldy, int C,
                                                             int NF, int H, int W, int fh, int fw, int mode, float* __restrict__ stats,
                                                             int64_t stats_ld, int nrec, int lcvp) {
  __shared__ float sPart[256 * 4];
  const int tid = threadIdx.x, CV = C >> 3;
  const int cv = tid & ((1 << lcvp) - 1), rg = tid >> lcvp, rgn = 256 >> lcvp;
  const int Ho = mode == 0 ? H / fh : H * fh, Wo = mode == 0 ? W / fw : W * fw;
  const float inv = 1.f / (float)(fh * fw);
  for (int rec = blockIdx.x; rec < nrec; rec += gridDim.x) {
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
    if (cv < CV) {
#pragma unroll 4
      for (int r = rg; r < 64; r += rgn) {
        const int orow = rec * 64 + r;                     // < 2^31 (checked by the launcher)
        const int wo = orow % Wo, t = orow / Wo, ho = t % Ho, nf = t / Ho;
        u32x4 v;
        if (mode == 0) {
          float acc[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = 0.f;
          for (int a = 0; a < fh; ++a)
            for (int b = 0; b < fw; ++b) {
              const int64_t irow = ((int64_t)nf * H + ho * fh + a) * W + wo * fw + b;
              float f[8];
              Elt<__bf16>::unpack(*(const u32x4*)(x + (irow * ldx + (int64_t)cv * 8) * 2), f);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[e] += f[e];
            }
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] *= inv;
          v = Elt<__bf16>::pack(acc);
        } else {
          const int64_t irow = ((int64_t)nf * H + ho / fh) * W + wo / fw;
          v = *(const u32x4*)(x + (irow * ldx + (int64_t)cv * 8) * 2);
        }
        *(u32x4*)(y + ((int64_t)orow * ldy + (int64_t)cv * 8) * 2) = v;
        float f[8];
        Elt<__bf16>::unpack(v, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s0 += f[j];
          s1 += f[4 + j];
          q0 += f[j] * f[j];
          q1 += f[4 + j] * f[4 + j];
        }
      }
    }
    *(f32x4*)(sPart + tid * 4) = f32x4{s0, s1, q0, q1};
    __syncthreads();
    if (rg == 0 && cv < CV) {
      for (int g = 1; g < rgn; ++g) {
        const f32x4 o = *(const f32x4*)(sPart + ((g << lcvp) + cv) * 4);
        s0 += o[0];
        s1 += o[1];
        q0 += o[2];
        q1 += o[3];
      }
      *(f32x4*)(stats + ((int64_t)rec * stats_ld + 2 * cv) * 2) = f32x4{s0, q0, s1, q1};     // quads 2 cv, 2 cv + 1: (sum, sum of squares)
    }
    __syncthreads();
  }
}

// strided 2-D copy of 16-byte vecs (skip-connection concat: write a tensor into a column slice)
__global__ __launch_bounds__(256) void copy2d_kernel(const char* __restrict__ x, int64_t ldx_b, char* __restrict__ y, int64_t ldy_b,
                                                     int64_t rows, int vecs) {
  const int64_t total = rows * vecs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / vecs;
    const int v = (int)(i % vecs);
    *(u32x4*)(y + r * ldy_b + (int64_t)v * 16) = *(const u32x4*)(x + r * ldx_b + (int64_t)v * 16);
  }
}

// ============================================================================= C-ABI
extern "C" int mmd_temb_fwd(const void* t, int t_kind, int N, int dim, const float* W0, const float* b0, const float* W2,
                            const float* b2, float* out_silu, float* out_raw, void* stream) {
  MMD_REQUIRE(t && W0 && b0 && W2 && b2 && out_silu && N > 0 && dim > 0 && dim <= 4096, "temb_fwd: bad argument");
  MMD_REQUIRE(t_kind >= 0 && t_kind <= 2, "temb_fwd: t_kind must be 0 (int64), 1 (int32) or 2 (float32)");
  return mmd_launch<temb_kernel>("temb", dim3(N), dim3(256), 2 * dim * sizeof(float), (hipStream_t)stream, t, t_kind, dim, W0, b0, W2, b2, out_silu, out_raw);
}

extern "C" int mmd_linear_fwd(const float* x, const float* W, const float* b, float* y, int N, int K, int J, void* stream) {
  MMD_REQUIRE(x && W && y && N > 0 && K > 0 && J > 0, "linear_fwd: bad argument");
  return mmd_launch<linear_kernel>("linear", dim3(cdiv(J, 4)), dim3(256), 0, (hipStream_t)stream, x, W, b, y, N, K, J);
}

extern "C" int mmd_resample(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int C, int NF, int H, int W, int fh,
                            int fw, int mode, float scale, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "resample: bad dtype");
  MMD_REQUIRE(x && y && C % epv == 0 && NF > 0 && H > 0 && W > 0 && fh > 0 && fw > 0, "resample: bad argument");
  MMD_REQUIRE(mode == 1 || (H % fh == 0 && W % fw == 0), "resample: pooled dims must divide (%d/%d, %d/%d)", H, fh, W, fw);
  const int64_t orows = mode == 0 ? (int64_t)NF * (H / fh) * (W / fw) : (int64_t)NF * H * fh * W * fw;
  const int grid = ew_grid(orows * (C / epv));
  hipStream_t st = (hipStream_t)stream;
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<resample_kernel<typename decltype(t)::type>>("resample", dim3(grid), dim3(256), 0, st, (const char*)x, ldx, (char*)y, ldy, C, NF, H, W,
                                                                   fh, fw, mode, scale);
  });
}

extern "C" int mmd_resample_stats(const void* x, int64_t ldx, void* y, int64_t ldy, int C, int NF, int H, int W, int fh, int fw, int mode,
                                  float* stats, int64_t stats_ld, void* stream) {
  MMD_REQUIRE(x && y && stats && C > 0 && C % 8 == 0 && C <= 2048 && NF > 0 && H > 0 && W > 0 && fh > 0 && fw > 0 && (mode == 0 || mode == 1),
              "resample_stats: bad argument (bf16 rows of 8 .. 2048 channels in whole 16-byte vectors)");
  MMD_REQUIRE(mode == 1 || (H % fh == 0 && W % fw == 0), "resample_stats: pooled dims must divide (%d/%d, %d/%d)", H, fh, W, fw);
  const int64_t orows = mode == 0 ? (int64_t)NF * (H / fh) * (W / fw) : (int64_t)NF * H * fh * W * fw;
  MMD_REQUIRE(orows % 64 == 0 && orows < ((int64_t)1 << 31), "resample_stats: %ld output rows (records are 64 rows; < 2^31)", (long)orows);
  MMD_REQUIRE((uintptr_t)stats % 16 == 0 && stats_ld % 2 == 0 && stats_ld >= C / 4, "resample_stats: the record view must start on an even quad "
              "of a 16-byte aligned buffer (ld %ld quads)", (long)stats_ld);
  MMD_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "resample_stats: unaligned rows");
  int lcvp = 0;
  while ((1 << lcvp) < C / 8) ++lcvp;
  const int nrec = (int)(orows / 64);
  return mmd_launch<resample_stats_kernel>("resample_stats", dim3(min(nrec, 8192)), dim3(256), 0, (hipStream_t)stream, (const char*)x, ldx, (char*)y, ldy, C,
                                           NF, H, W, fh, fw, mode, stats, stats_ld, nrec, lcvp);
}

extern "C" int mmd_copy2d(const void* x, int64_t ldx_bytes, void* y, int64_t ldy_bytes, int64_t rows, int64_t row_bytes, void* stream) {
  MMD_REQUIRE(x && y && rows > 0 && row_bytes > 0 && row_bytes % 16 == 0 && ldx_bytes % 16 == 0 && ldy_bytes % 16 == 0,
              "copy2d: rows must be 16-byte multiples");
  MMD_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "copy2d: unaligned pointer");
  const int vecs = (int)(row_bytes / 16);
  return mmd_launch<copy2d_kernel>("copy2d", dim3(ew_grid(rows * vecs)), dim3(256), 0, (hipStream_t)stream, (const char*)x, ldx_bytes, (char*)y, ldy_bytes,
                                   rows, vecs);
}

// sinusoidal timestep embedding alone (nn.py:192-210): out[N, dim] fp32 (training path keeps the MLP as separate linears)
__global__ void timestep_embedding_kernel(const void* __restrict__ t, int t_kind, int dim, float* __restrict__ out) {
  const int n = blockIdx.x;
  float tv;
  if (t_kind == 0) tv = (float)((const int64_t*)t)[n];
  else if (t_kind == 1) tv = (float)((const int32_t*)t)[n];
  else tv = ((const float*)t)[n];
  const int half = dim / 2;
  for (int i = threadIdx.x; i < dim; i += blockDim.x) {
    float v = 0.f;
    if (i < 2 * half) {
      const int k = i < half ? i : i - half;
      const float a = tv * expf(-logf(10000.f) * (float)k / (float)half);
      v = i < half ? cosf(a) : sinf(a);
    }
    out[(int64_t)n * dim + i] = v;
  }
}
extern "C" int mmd_timestep_embedding(const void* t, int t_kind, int N, int dim, float* out, void* stream) {
  MMD_REQUIRE(t && out && N > 0 && dim > 0 && t_kind >= 0 && t_kind <= 2, "timestep_embedding: bad argument");
  return mmd_launch<timestep_embedding_kernel>("timestep_embedding", dim3(N), dim3(128), 0, (hipStream_t)stream, t, t_kind, dim, out);
}

// Gradient payload conversion of the data-parallel all-reduce (optim.FlatAdamW, grad_payload = "bf16"): y = (T_out)(x * scale).
__global__ __launch_bounds__(256) void cast_kernel(const void* __restrict__ x, void* __restrict__ y, int src_bf16, int dst_bf16, float scale,
                                                   int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = (src_bf16 ? Elt<__bf16>::ld(x, i) : ((const float*)x)[i]) * scale;
    if (dst_bf16) Elt<__bf16>::st(y, i, v);
    else ((float*)y)[i] = v;
  }
}
extern "C" int mmd_cast(const void* x, int src_dtype, void* y, int dst_dtype, float scale, int64_t n, void* stream) {
  MMD_REQUIRE(x && y && n > 0, "cast: bad argument");
  MMD_REQUIRE((src_dtype == MMD_F32 || src_dtype == MMD_BF16) && (dst_dtype == MMD_F32 || dst_dtype == MMD_BF16), "cast: bad dtype");
  return mmd_launch<cast_kernel>("cast", dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, src_dtype == MMD_BF16, dst_dtype == MMD_BF16, scale, n);
}

// ----------------------------------------------------------------------------- element-wise pieces of the training step
// out = silu(x) or dy * silu'(x).  The product is (dy sg) (1 + x (1 - sg)): dsilu_f(x) would round sg (1 + ...) first.
template <typename T>
__global__ __launch_bounds__(256) void silu_kernel(const char* __restrict__ x, const char* __restrict__ dy, char* __restrict__ out, int64_t nvec) {
  constexpr int EPV = Elt<T>::EPV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float f[EPV], d[EPV];
    Elt<T>::unpack(((const u32x4*)x)[i], f);
    if (dy) Elt<T>::unpack(((const u32x4*)dy)[i], d);
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-f[e]));
      f[e] = dy ? d[e] * sg * (1.f + f[e] * (1.f - sg)) : f[e] * sg;
    }
    ((u32x4*)out)[i] = Elt<T>::pack(f);
  }
}

// inverted dropout: out = x * mask * scale (mask bytes 0/1, drawn by the caller); the backward is the same kernel on dy
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const char* __restrict__ x, const uint8_t* __restrict__ mask, float scale,
                                                      char* __restrict__ out, int64_t nvec) {
  constexpr int EPV = Elt<T>::EPV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float f[EPV];
    Elt<T>::unpack(((const u32x4*)x)[i], f);
#pragma unroll
    for (int e = 0; e < EPV; ++e) f[e] = mask[i * EPV + e] ? f[e] * scale : 0.f;
    ((u32x4*)out)[i] = Elt<T>::pack(f);
  }
}

// d loss / d out for loss = sum_n w[n] * mean_n((target - out)^2):  g = 2 (out - target) * w[n] / per
__global__ __launch_bounds__(256) void mse_grad_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                       const float* __restrict__ w, float* __restrict__ g, int64_t per, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    g[i] = 2.f * (out[i] - target[i]) * w[i / per] / (float)per;
}

// out = silu(x) (dy == NULL) or dy * silu'(x); contiguous buffers of n elements (n % (16/elsize) == 0)
extern "C" int mmd_silu(int dtype, const void* x, const void* dy, void* out, int64_t n, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE((dtype == MMD_BF16 || dtype == MMD_F32) && x && out && n > 0 && n % epv == 0, "silu: bad argument");
  hipStream_t st = (hipStream_t)stream;
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<silu_kernel<typename decltype(t)::type>>("silu", dim3(ew_grid(n / epv)), dim3(256), 0, st, (const char*)x, (const char*)dy, (char*)out,
                                                               n / epv);
  });
}

extern "C" int mmd_dropout(int dtype, const void* x, const uint8_t* mask, float scale, void* out, int64_t n, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE((dtype == MMD_BF16 || dtype == MMD_F32) && x && mask && out && n > 0 && n % epv == 0, "dropout: bad argument");
  hipStream_t st = (hipStream_t)stream;
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<dropout_kernel<typename decltype(t)::type>>("dropout", dim3(ew_grid(n / epv)), dim3(256), 0, st, (const char*)x, mask, scale,
                                                                  (char*)out, n / epv);
  });
}

extern "C" int mmd_mse_grad(const float* out, const float* target, const float* w, float* g, int N, int64_t per_sample, void* stream) {
  MMD_REQUIRE(out && target && w && g && N > 0 && per_sample > 0, "mse_grad: bad argument");
  const int64_t total = per_sample * N;
  return mmd_launch<mse_grad_kernel>("mse_grad", dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, out, target, w, g, per_sample, total);
}
