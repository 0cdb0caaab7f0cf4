// Convolutions at the API layout edge: the stem (InitialBlock, unet:680-694; fp32 [N, F, C, H, W] -> channels-last rows) and the head
// (unet:1003-1012; rows -> fp32 [N, F, C, H, W]) in their direct, cooperative, strip, MFMA and GEMM + gather forms, and the
// super-resolution model's bilinear-upsample + concat input (image_unet.py:704-715).
#include "mmd_rowwave.h"

// ----------------------------------------------------------------------------- stem conv (API layout -> channels-last)
// in : fp32 [N, F, Cin, H, W] (audio: F=1, H=1, W=L)   W packed fp32 [ntaps][Cin][Cout]   out: T [N*F*H*W, Cout]
struct EdgeConvParams {
  const float* x; const float* w; const float* bias;
  char* y; int64_t ldy;
  int N, F, Cin, H, W, Cout, ntaps;
  int taps[27 * 3];
};
template <typename T>
__global__ __launch_bounds__(256) void stem_conv_kernel(const EdgeConvParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  extern __shared__ float sw[];    // [ntaps*Cin][Cout]
  const int KW = p.ntaps * p.Cin;
  for (int i = threadIdx.x; i < KW * p.Cout; i += 256) sw[i] = p.w[i];
  __syncthreads();
  const int CV = p.Cout / EPV;
  const int HW = p.H * p.W;
  const int64_t rows = (int64_t)p.N * p.F * HW;
  const int64_t total = rows * CV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const int64_t m = i / CV;
    const int w0 = (int)(m % p.W), h0 = (int)((m / p.W) % p.H), f0 = (int)((m / HW) % p.F);
    const int64_t n = m / ((int64_t)HW * p.F);
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = p.bias ? p.bias[cv * EPV + e] : 0.f;
    for (int t = 0; t < p.ntaps; ++t) {
      const int f = f0 + p.taps[t * 3], h = h0 + p.taps[t * 3 + 1], w = w0 + p.taps[t * 3 + 2];
      if ((unsigned)f >= (unsigned)p.F || (unsigned)h >= (unsigned)p.H || (unsigned)w >= (unsigned)p.W) continue;
      for (int ci = 0; ci < p.Cin; ++ci) {
        const float xv = p.x[(((n * p.F + f) * p.Cin + ci) * p.H + h) * p.W + w];
        const float* wr = sw + (t * p.Cin + ci) * p.Cout + cv * EPV;
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] += xv * wr[e];
      }
    }
    *(u32x4*)(p.y + (m * p.ldy + (int64_t)cv * EPV) * ES) = Elt<T>::pack(acc);
  }
}

// Strip variant (W % 4 == 0, Cin in {1, 3}): thread = (one 16-byte chunk of output channels, FOUR consecutive pixels along w).
// The per-pixel kernel above walks its taps one dependent scalar load at a time (27 L2 round trips per thread: 210 us for the
// 16x64x64 stem, 8.6 TFLOP/s) and re-reads every weight from LDS per pixel; here three taps x Cin x 4 pixels of loads are in
// flight before the first FMA, borders are handled branch-free (clamped address, zeroed value), and each weight read from LDS
// feeds four pixels.
template <typename T, int CIN>
__global__ __launch_bounds__(256) void stem_conv_strip_kernel(const EdgeConvParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  constexpr int PX = 4;
  extern __shared__ float sw[];    // [ntaps*CIN][Cout]
  for (int i = threadIdx.x; i < p.ntaps * CIN * p.Cout; i += 256) sw[i] = p.w[i];
  __syncthreads();
  const int CV = p.Cout / EPV;
  const int WS = p.W / PX;
  const int64_t total = (int64_t)p.N * p.F * p.H * WS * CV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    int64_t sidx = i / CV;
    const int w0 = (int)(sidx % WS) * PX;
    sidx /= WS;
    const int h0 = (int)(sidx % p.H);
    sidx /= p.H;
    const int f0 = (int)(sidx % p.F);
    const int64_t n = sidx / p.F;
    float acc[PX][EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      const float b = p.bias ? p.bias[cv * EPV + e] : 0.f;
#pragma unroll
      for (int px = 0; px < PX; ++px) acc[px][e] = b;
    }
    for (int tg = 0; tg < p.ntaps; tg += 3) {
      float xv[3][CIN][PX];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int t = min(tg + u, p.ntaps - 1);
        const int f = f0 + p.taps[t * 3], h = h0 + p.taps[t * 3 + 1], wb = w0 + p.taps[t * 3 + 2];
        const bool okfh = (tg + u < p.ntaps) && (unsigned)f < (unsigned)p.F && (unsigned)h < (unsigned)p.H;
        const int fc = okfh ? f : f0, hc = okfh ? h : h0;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const float* xr = p.x + (((n * p.F + fc) * CIN + ci) * p.H + hc) * (int64_t)p.W;
#pragma unroll
          for (int px = 0; px < PX; ++px) {
            const int w = wb + px;
            const float v = xr[min(max(w, 0), p.W - 1)];
            xv[u][ci][px] = (okfh && (unsigned)w < (unsigned)p.W) ? v : 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        if (tg + u < p.ntaps) {
#pragma unroll
          for (int ci = 0; ci < CIN; ++ci) {
            const float* wr = sw + ((tg + u) * CIN + ci) * p.Cout + cv * EPV;
            float wv[EPV];
#pragma unroll
            for (int e = 0; e < EPV; e += 4) {
              const f32x4 w4 = *(const f32x4*)(wr + e);
#pragma unroll
              for (int k = 0; k < 4; ++k) wv[e + k] = w4[k];
            }
#pragma unroll
            for (int px = 0; px < PX; ++px)
#pragma unroll
              for (int e = 0; e < EPV; ++e) acc[px][e] += xv[u][ci][px] * wv[e];
          }
        }
      }
    }
    const int64_t m0 = ((n * p.F + f0) * p.H + h0) * (int64_t)p.W + w0;
#pragma unroll
    for (int px = 0; px < PX; ++px) *(u32x4*)(p.y + ((m0 + px) * p.ldy + (int64_t)cv * EPV) * ES) = Elt<T>::pack(acc[px]);
  }
}

// ----------------------------------------------------------------------------- head conv (channels-last -> API layout)
// in: T rows [N*F*H*W, Cin] (already GN+SiLU'd)   W packed fp32 [ntaps][Cin][Co] (Co <= 8)   out fp32 [N,F,Co,H,W]
struct HeadConvParams {
  const char* x; int64_t ldx; const float* w; const float* bias;
  float* y;
  int N, F, Cin, H, W, Co, ntaps;
  int taps[27 * 3];
};
template <typename T, int CO>
__global__ __launch_bounds__(256) void head_conv_kernel(const HeadConvParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  extern __shared__ float sw[];    // [ntaps*Cin][CO]
  const int KW = p.ntaps * p.Cin;
  for (int i = threadIdx.x; i < KW * CO; i += 256) {
    const int co = i % CO;
    sw[i] = co < p.Co ? p.w[(i / CO) * p.Co + co] : 0.f;
  }
  __syncthreads();
  const int HW = p.H * p.W;
  const int64_t rows = (int64_t)p.N * p.F * HW;
  const int CinV = p.Cin / EPV;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < rows; m += (int64_t)gridDim.x * 256) {
    const int w0 = (int)(m % p.W), h0 = (int)((m / p.W) % p.H), f0 = (int)((m / HW) % p.F);
    const int64_t n = m / ((int64_t)HW * p.F);
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = (p.bias && c < p.Co) ? p.bias[c] : 0.f;
    for (int t = 0; t < p.ntaps; ++t) {
      const int df = p.taps[t * 3], dh = p.taps[t * 3 + 1], dw = p.taps[t * 3 + 2];
      if ((unsigned)(f0 + df) >= (unsigned)p.F || (unsigned)(h0 + dh) >= (unsigned)p.H || (unsigned)(w0 + dw) >= (unsigned)p.W) continue;
      const int64_t src = m + (int64_t)df * HW + dh * p.W + dw;
      const char* xr = p.x + src * p.ldx * ES;
      const float* wt = sw + (int64_t)t * p.Cin * CO;
      for (int v = 0; v < CinV; ++v) {
        float f[EPV];
        Elt<T>::unpack(*(const u32x4*)(xr + v * 16), f);
#pragma unroll
        for (int e = 0; e < EPV; ++e)
#pragma unroll
          for (int c = 0; c < CO; ++c) acc[c] += f[e] * wt[(v * EPV + e) * CO + c];
      }
    }
    const int hw = h0 * p.W + w0;
    for (int c = 0; c < p.Co; ++c) p.y[((n * p.F + f0) * p.Co + c) * HW + hw] = acc[c];
  }
}

// MFMA stem conv (bf16 rows out; ntaps * Cin <= 28, Cout = 32 NB <= 128, W % 32 == 0): the 27-term dot products of the video stem on
// the fp32 matrix pipe (v_mfma_f32_32x32x2f32: exact fp32 products, fp32 accumulation) instead of 0.9 G scalar FMAs - the strip kernel
// above runs at 17 TFLOP/s of VALU (107 us for the 16 x 64 x 64 stem against an 8 us output write).  D[cout][pixel] = W[cout][k] X[k][pixel]:
// a wave owns 32 consecutive pixels of one image row; lane (n = lane % 32, kk = lane / 32) gathers x for k = 2 s + kk straight from the
// API-layout input (coalesced along w; padding reads as zero), the weights of the lane's output channel sit in registers for the whole
// kernel, and the epilogue is the row-strip GEMM's: half-wave swap -> 8 consecutive channels per lane -> bias -> one 16-byte store.
template <int NB>
__global__ __launch_bounds__(256, 2) void stem_conv_mfma_kernel(const EdgeConvParams p) {
  constexpr int MAXS = 14;
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int K = p.ntaps * p.Cin, KS = (K + 1) >> 1;
  float wreg[MAXS][NB];
  int kd[MAXS];                                          // per step: this lane's (df, dh, dw, ci), or -1 past K
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int k = 2 * s + half;
    const bool kv = s < KS && k < K;
    const int kc = kv ? k : 0, t = kc / p.Cin, ci = kc - t * p.Cin;
    kd[s] = kv ? ((p.taps[t * 3] + 1) | ((p.taps[t * 3 + 1] + 1) << 2) | ((p.taps[t * 3 + 2] + 1) << 4) | (ci << 6)) : -1;
#pragma unroll
    for (int b = 0; b < NB; ++b) wreg[s][b] = kv ? p.w[(int64_t)kc * p.Cout + b * 32 + l31] : 0.f;
  }
  const int HW = p.H * p.W, WG = p.W >> 5;
  const int64_t groups = (int64_t)p.N * p.F * p.H * WG;
  const int64_t nwave = (int64_t)gridDim.x * 4, wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  auto gather = [&](int64_t g, float (&xv)[MAXS]) {
    const int w = (int)(g % WG) * 32 + l31;
    int64_t r = g / WG;
    const int h = (int)(r % p.H);
    r /= p.H;
    const int f = (int)(r % p.F);
    const int64_t n = r / p.F;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < KS) {                                        // uniform: the audio stem (3 taps x 1 channel) has two steps, not fourteen
        const int d = kd[s];
        const int df = (d & 3) - 1, dh = ((d >> 2) & 3) - 1, dw = ((d >> 4) & 3) - 1, ci = (d >> 6) & 3;
        const bool ok = d >= 0 && (unsigned)(f + df) < (unsigned)p.F && (unsigned)(h + dh) < (unsigned)p.H && (unsigned)(w + dw) < (unsigned)p.W;
        const int64_t src = (((n * p.F + (f + df)) * p.Cin + ci) * p.H + (h + dh)) * (int64_t)p.W + (w + dw);
        xv[s] = ok ? p.x[src] : 0.f;
      }
    }
  };
  float xcur[MAXS] = {}, xnext[MAXS] = {};
  if (wave_id < groups) gather(wave_id, xcur);
  for (int64_t g = wave_id; g < groups; g += nwave) {
    if (g + nwave < groups) gather(g + nwave, xnext);    // the next group's gather flies under this group's MFMAs
    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < KS) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[s][b], xcur[s], acc[b], 0, 0, 0);
      }
    }
    // the row-wave epilogue (mmd_rowwave.h): the lane's octets are the channels 32 b + 16 j2 + 8 half .. + 8 of pixel l31
    const int64_t m = g * 32 + l31;                      // groups walk the rows in order: 32 consecutive pixels of one image row
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j2 = 0; j2 < 2; ++j2) {
        float v[8];
        acc_octet(acc[b], j2, v);
        const int col = b * 32 + 16 * j2 + 8 * half;
        if (p.bias) octet_add(v, load_octet(p.bias + col));
        *(u32x4*)(p.y + (m * p.ldy + col) * 2) = Elt<__bf16>::pack(v);
      }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) xcur[s] = s < KS ? xnext[s] : 0.f;
  }
}

static bool stem_mfma_ok(int dtype, const EdgeConvParams& p) {
  static const bool on = mmd_env_char("MMD_STEM_MFMA") != '0';
  for (int i = 0; i < p.ntaps * 3; ++i)
    if (p.taps[i] < -1 || p.taps[i] > 1) return false;          // the kernel packs a tap offset + 1 into two bits
  return on && dtype == MMD_BF16 && p.W % 32 == 0 && p.ntaps * p.Cin <= 28 && p.Cin <= 3 && p.Cout % 32 == 0 && p.Cout <= 128 && p.ldy % 8 == 0 &&
         ((uintptr_t)p.y) % 16 == 0 && (!p.bias || ((uintptr_t)p.bias) % 16 == 0);
}

static int launch_stem_mfma(const EdgeConvParams& p, hipStream_t st) {
  const int64_t groups = (int64_t)p.N * p.F * p.H * (p.W / 32);
  const int grid = (int)min((int64_t)2048, (groups + 3) / 4);
  switch (p.Cout / 32) {
    case 1: return mmd_launch<stem_conv_mfma_kernel<1>>("stem_conv_mfma", dim3(grid), dim3(256), 0, st, p);
    case 2: return mmd_launch<stem_conv_mfma_kernel<2>>("stem_conv_mfma", dim3(grid), dim3(256), 0, st, p);
    case 3: return mmd_launch<stem_conv_mfma_kernel<3>>("stem_conv_mfma", dim3(grid), dim3(256), 0, st, p);
    default: return mmd_launch<stem_conv_mfma_kernel<4>>("stem_conv_mfma", dim3(grid), dim3(256), 0, st, p);
  }
}

extern "C" int mmd_stem_conv(int dtype, const float* x, const float* w, const float* bias, void* y, int64_t ldy, int N, int F,
                             int Cin, int H, int W, int Cout, int ntaps, const int* taps, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "stem_conv: bad dtype");
  MMD_REQUIRE(x && w && y && taps && ntaps >= 1 && ntaps <= 27 && Cout % epv == 0, "stem_conv: bad argument");
  const size_t lds = (size_t)ntaps * Cin * Cout * sizeof(float);
  MMD_REQUIRE(lds <= 64 * 1024, "stem_conv: weights (%zu B) exceed the 64 KiB LDS stage", lds);
  EdgeConvParams p;
  p.x = x; p.w = w; p.bias = bias; p.y = (char*)y; p.ldy = ldy;
  p.N = N; p.F = F; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.ntaps = ntaps;
  for (int i = 0; i < ntaps * 3; ++i) p.taps[i] = taps[i];
  const int64_t total = (int64_t)N * F * H * W * (Cout / epv);
  hipStream_t st = (hipStream_t)stream;
  if (stem_mfma_ok(dtype, p)) return launch_stem_mfma(p, st);
  if (W % 4 == 0 && (Cin == 1 || Cin == 3) && Cout % 4 == 0) {
    const dim3 grid(ew_grid(total / 4));
    return mmd_by_dtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      if (Cin == 3) return mmd_launch<stem_conv_strip_kernel<T, 3>>("stem_conv_strip", grid, dim3(256), lds, st, p);
      return mmd_launch<stem_conv_strip_kernel<T, 1>>("stem_conv_strip", grid, dim3(256), lds, st, p);
    });
  }
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<stem_conv_kernel<typename decltype(t)::type>>("stem_conv", dim3(ew_grid(total)), dim3(256), lds, st, p);
  });
}

// Cooperative head conv: LPR = Cin/EPV lanes share one output row (each lane owns one 16-byte channel chunk, so every
// tap is ONE coalesced row read), partial dot products are reduced across the row's lanes with xor-shuffles.
// Weights sit in LDS as [tap][quad j][lane chunk][4 floats] so the 16 lanes of a row read 256 contiguous bytes
// (conflict-free) and the row groups of a wave broadcast.
__device__ __attribute__((aligned(16))) uint32_t g_zero_page_misc[8] = {0, 0, 0, 0, 0, 0, 0, 0};

template <typename T, int CO, int LPR>
__global__ __launch_bounds__(256) void head_conv_coop_kernel(const HeadConvParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  constexpr int NQ = EPV * CO / 4;       // float4 quads of weights per (tap, lane)
  constexpr int RPW = 64 / LPR;          // rows per wave pass
  extern __shared__ __attribute__((aligned(16))) float sw[];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < p.ntaps * NQ * LPR * 4; i += 256) {
    const int k = i & 3, cvi = (i >> 2) % LPR, j = ((i >> 2) / LPR) % NQ, t = (i >> 2) / (LPR * NQ);
    const int ec = j * 4 + k, e = ec / CO, c = ec % CO;
    sw[i] = c < p.Co ? p.w[((int64_t)t * p.Cin + cvi * EPV + e) * p.Co + c] : 0.f;
  }
  __syncthreads();
  const int HW = p.H * p.W;
  const int64_t rows = (int64_t)p.N * p.F * HW;
  const int cvi = lane % LPR, rsel = lane / LPR;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (tid >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t mb = wave_id * RPW; mb < rows; mb += nwaves * RPW) {
    const int64_t m = mb + rsel;
    const bool rok = m < rows;
    const int64_t mm = rok ? m : 0;
    const int w0 = (int)(mm % p.W), h0 = (int)((mm / p.W) % p.H), f0 = (int)((mm / HW) % p.F);
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    // taps in groups of 9: all 9 row reads are issued branch-free (padding -> zero page) before any is consumed
    for (int tg = 0; tg < p.ntaps; tg += 9) {
      u32x4 v[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int t = min(tg + u, p.ntaps - 1);
        const int df = p.taps[t * 3], dh = p.taps[t * 3 + 1], dw = p.taps[t * 3 + 2];
        const bool ok = rok && (tg + u < p.ntaps) && (unsigned)(f0 + df) < (unsigned)p.F && (unsigned)(h0 + dh) < (unsigned)p.H &&
                        (unsigned)(w0 + dw) < (unsigned)p.W;
        const int64_t src = mm + (int64_t)df * HW + dh * p.W + dw;
        const char* sp = ok ? p.x + (src * p.ldx + (int64_t)cvi * EPV) * ES : (const char*)g_zero_page_misc;
        v[u] = *(const u32x4*)sp;
      }
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        if (tg + u < p.ntaps) {
          float f[EPV];
          Elt<T>::unpack(v[u], f);
          const float* wq = sw + ((int64_t)(tg + u) * NQ * LPR + cvi) * 4;
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const f32x4 w4 = *(const f32x4*)(wq + j * LPR * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int ec = j * 4 + k;
              acc[ec % CO] += f[ec / CO] * w4[k];
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    }
    if (rok && cvi == 0) {
      const int64_t n = m / ((int64_t)HW * p.F);
      const int hw = h0 * p.W + w0;
      for (int c = 0; c < p.Co; ++c) p.y[((n * p.F + f0) * p.Co + c) * HW + hw] = acc[c] + (p.bias ? p.bias[c] : 0.f);
    }
  }
}

// Strip variant of the cooperative kernel (W % 4 == 0): the LPR lanes of a group own FOUR consecutive output pixels, so
// every weight quad read from LDS feeds four pixels (the per-row version re-reads all ntaps*Cin*CO weights per output row:
// 14 GB of LDS returns for the 16x64x64 head, 355 us), CO is the exact output width (3, not 4), and twelve row reads are in
// flight per tap group.
template <typename T, int CO, int LPR>
__global__ __launch_bounds__(256) void head_conv_strip_kernel(const HeadConvParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  constexpr int PX = 4;
  constexpr int NQ = EPV * CO / 4;       // float4 quads of weights per (tap, lane)
  constexpr int SPW = 64 / LPR;          // strips per wave pass
  extern __shared__ __attribute__((aligned(16))) float sw[];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < p.ntaps * NQ * LPR * 4; i += 256) {
    const int k = i & 3, cvi = (i >> 2) % LPR, j = ((i >> 2) / LPR) % NQ, t = (i >> 2) / (LPR * NQ);
    const int ec = j * 4 + k, e = ec / CO, c = ec % CO;
    sw[i] = p.w[((int64_t)t * p.Cin + cvi * EPV + e) * CO + c];
  }
  __syncthreads();
  const int HW = p.H * p.W, WS = p.W / PX;
  const int64_t strips = (int64_t)p.N * p.F * p.H * WS;
  const int cvi = lane % LPR, rsel = lane / LPR;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (tid >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t sb = wave_id * SPW; sb < strips; sb += nwaves * SPW) {
    const bool rok = sb + rsel < strips;
    int64_t sidx = rok ? sb + rsel : 0;
    const int w0 = (int)(sidx % WS) * PX;
    sidx /= WS;
    const int h0 = (int)(sidx % p.H);
    sidx /= p.H;
    const int f0 = (int)(sidx % p.F);
    const int64_t n = sidx / p.F;
    const int64_t m0 = ((n * p.F + f0) * p.H + h0) * (int64_t)p.W + w0;
    float acc[PX][CO];
#pragma unroll
    for (int px = 0; px < PX; ++px)
#pragma unroll
      for (int c = 0; c < CO; ++c) acc[px][c] = 0.f;
    for (int tg = 0; tg < p.ntaps; tg += 3) {
      u32x4 v[3][PX];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int t = min(tg + u, p.ntaps - 1);
        const int df = p.taps[t * 3], dh = p.taps[t * 3 + 1], dw = p.taps[t * 3 + 2];
        const bool okfh = rok && (tg + u < p.ntaps) && (unsigned)(f0 + df) < (unsigned)p.F && (unsigned)(h0 + dh) < (unsigned)p.H;
        const int64_t src = m0 + (int64_t)df * HW + dh * p.W + dw;
#pragma unroll
        for (int px = 0; px < PX; ++px) {
          const bool ok = okfh && (unsigned)(w0 + px + dw) < (unsigned)p.W;
          const char* sp = ok ? p.x + ((src + px) * p.ldx + (int64_t)cvi * EPV) * ES : (const char*)g_zero_page_misc;
          v[u][px] = *(const u32x4*)sp;
        }
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        if (tg + u < p.ntaps) {
          const float* wq = sw + ((int64_t)(tg + u) * NQ * LPR + cvi) * 4;
          float wv[NQ * 4];
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const f32x4 w4 = *(const f32x4*)(wq + j * LPR * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) wv[j * 4 + k] = w4[k];
          }
#pragma unroll
          for (int px = 0; px < PX; ++px) {
            float f[EPV];
            Elt<T>::unpack(v[u][px], f);
#pragma unroll
            for (int e = 0; e < EPV; ++e)
#pragma unroll
              for (int c = 0; c < CO; ++c) acc[px][c] += f[e] * wv[e * CO + c];
          }
        }
      }
    }
#pragma unroll
    for (int px = 0; px < PX; ++px)
#pragma unroll
      for (int c = 0; c < CO; ++c) {
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) acc[px][c] += __shfl_xor(acc[px][c], o, 64);
      }
    if (rok && cvi == 0) {
      const int hw = h0 * p.W + w0;
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        const float b = p.bias ? p.bias[c] : 0.f;
        const f32x4 o4 = {acc[0][c] + b, acc[1][c] + b, acc[2][c] + b, acc[3][c] + b};
        *(f32x4*)(p.y + ((n * p.F + f0) * CO + c) * HW + hw) = o4;
      }
    }
  }
}

template <typename T, int CO>
static int launch_head_strip(const HeadConvParams& p, int lpr, hipStream_t st) {
  constexpr int EPV = Elt<T>::EPV;
  const size_t lds = (size_t)p.ntaps * (EPV * CO / 4) * lpr * 4 * sizeof(float);
  const int64_t strips = (int64_t)p.N * p.F * p.H * (p.W / 4);
  const int spb = 4 * (64 / lpr);                       // strips per block pass
  const int grid = (int)min((int64_t)2048, (strips + spb - 1) / spb);
  switch (lpr) {
    case 4: return mmd_launch<head_conv_strip_kernel<T, CO, 4>>("head_conv_strip", dim3(grid), dim3(256), lds, st, p);
    case 8: return mmd_launch<head_conv_strip_kernel<T, CO, 8>>("head_conv_strip", dim3(grid), dim3(256), lds, st, p);
    case 16: return mmd_launch<head_conv_strip_kernel<T, CO, 16>>("head_conv_strip", dim3(grid), dim3(256), lds, st, p);
    default: return mmd_launch<head_conv_strip_kernel<T, CO, 32>>("head_conv_strip", dim3(grid), dim3(256), lds, st, p);
  }
}

template <typename T, int CO>
static int launch_head_coop(const HeadConvParams& p, int lpr, hipStream_t st) {
  constexpr int EPV = Elt<T>::EPV;
  const size_t lds = (size_t)p.ntaps * (EPV * CO / 4) * lpr * 4 * sizeof(float);
  const int64_t rows = (int64_t)p.N * p.F * p.H * p.W;
  const int grid = (int)min((int64_t)2048, (rows + 63) / 64);
  switch (lpr) {
    case 4: return mmd_launch<head_conv_coop_kernel<T, CO, 4>>("head_conv_coop", dim3(grid), dim3(256), lds, st, p);
    case 8: return mmd_launch<head_conv_coop_kernel<T, CO, 8>>("head_conv_coop", dim3(grid), dim3(256), lds, st, p);
    case 16: return mmd_launch<head_conv_coop_kernel<T, CO, 16>>("head_conv_coop", dim3(grid), dim3(256), lds, st, p);
    case 32: return mmd_launch<head_conv_coop_kernel<T, CO, 32>>("head_conv_coop", dim3(grid), dim3(256), lds, st, p);
    case 64: return mmd_launch<head_conv_coop_kernel<T, CO, 64>>("head_conv_coop", dim3(grid), dim3(256), lds, st, p);
    default: return mmd_set_error(MMD_ERR_UNSUPPORTED, "head_conv: lanes per row %d", lpr);
  }
}


// (Round 3 tried the head as a GEMM on 32x32x16 MFMAs with the X fragments read straight from global memory - the output channels as
// the mostly empty M side, fp32 weights split into two bf16 parts.  Correct, and slower: 270 us against the strip kernel's 160 us.  All
// 27 taps re-read the tensor through the texture path, 1.8 GB per launch at the ~8 TB/s that 16-byte-per-lane row reads sustain; a
// version that pays would stage a three-frame halo in LDS like the 3x3 conv tiles do.  Not built: the head is 1.3 % of the step.)

template <typename T>
static int launch_head(const HeadConvParams& p, hipStream_t st) {
  const int64_t rows = (int64_t)p.N * p.F * p.H * p.W;
  const int grid = (int)min((int64_t)8192, (rows + 255) / 256);
  {   // strip kernel: four pixels per lane group, exact output width
    const int lpr = p.Cin / Elt<T>::EPV;
    const bool lpr_ok = p.Cin % Elt<T>::EPV == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32);
    const size_t lds_s = (size_t)p.ntaps * Elt<T>::EPV * p.Co * lpr * sizeof(float);
    if (p.W % 4 == 0 && ((uintptr_t)p.y) % 16 == 0 && lpr_ok && lds_s <= 150 * 1024) {
      switch (p.Co) {
        case 1: return launch_head_strip<T, 1>(p, lpr, st);
        case 2: return launch_head_strip<T, 2>(p, lpr, st);
        case 3: return launch_head_strip<T, 3>(p, lpr, st);
        case 6: return launch_head_strip<T, 6>(p, lpr, st);
        default: break;
      }
    }
  }
  const int CO = p.Co <= 2 ? 2 : (p.Co <= 4 ? 4 : 8);
  {   // cooperative kernel whenever the channel chunks of a row map onto a power-of-two lane group
    const int lpr = p.Cin / Elt<T>::EPV;
    const size_t lds_c = (size_t)p.ntaps * (Elt<T>::EPV * CO / 4) * lpr * 4 * sizeof(float);
    if (p.Cin % Elt<T>::EPV == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32 || lpr == 64) && lds_c <= 150 * 1024) {
      if (CO == 2) return launch_head_coop<T, 2>(p, lpr, st);
      if (CO == 4) return launch_head_coop<T, 4>(p, lpr, st);
      return launch_head_coop<T, 8>(p, lpr, st);
    }
  }
  const size_t lds = (size_t)p.ntaps * p.Cin * CO * sizeof(float);
  if (lds > 150 * 1024) return mmd_set_error(MMD_ERR_UNSUPPORTED, "head_conv: weights (%zu B) exceed LDS", lds);
  if (CO == 2) return mmd_launch<head_conv_kernel<T, 2>>("head_conv", dim3(grid), dim3(256), lds, st, p);
  if (CO == 4) return mmd_launch<head_conv_kernel<T, 4>>("head_conv", dim3(grid), dim3(256), lds, st, p);
  return mmd_launch<head_conv_kernel<T, 8>>("head_conv", dim3(grid), dim3(256), lds, st, p);
}

// ----------------------------------------------------------------------------- head conv as GEMM + gather (round 5, bf16)
// The head (GroupNorm32 + SiLU + Conv3d 3x3x3, 128 -> 3 channels, unet:1003-1012) was the video stream's LAST launch pair and its
// slowest HBM-side kernel: gn_apply wrote the normalised tensor (134 MB of traffic) and head_conv_strip read it 27 times through L1 / L2
// (0.45 TB/s).  A convolution with few output channels factors the other way round: FIRST the per-row products
//     P[o, m] = sum_ci W[tap, ci, co] act(norm(x))[m, ci],   o = tap Co + co   (a GEMM with N = ntaps Co = 81 columns, K = Cin),
// with the norm applied in registers on the way into the MFMA operand (x is read ONCE, nothing normalised is written), THEN
//     y[n, f, co, h, w] = bias[co] + sum_tap P[tap Co + co, m + offset(tap)]    (zero outside the frame),
// a pure gather over fp32 planes P[o][m] that are contiguous in m (coalesced along w) and read exactly once.
// Weights enter the matrix pipe as a bf16 (hi, lo) pair, so the products keep the fp32 weights to 2^-17 (the direct kernel uses fp32
// weights); the activations are rounded to bf16 exactly where gn_apply used to store them.
struct HeadGemmParams {
  const char* x; int64_t ldx; int64_t M;
  const float* gn_a; const float* gn_b; int64_t gn_rows; int gn_S; int act;
  const char* wimg;          // [2 hi/lo][3 blocks of 32 outputs][KS k-steps][64 lanes][16 B]: lane (l31, half) = W[32 ob + l31][16 cg + 8 half .. + 8]
  float* P;                  // [NO][M] fp32 planes
  int NO;                    // ntaps * Co <= 96
  int per_block;             // consecutive 128-row groups per block
};
template <int KS>
__global__ __launch_bounds__(256, 2) void head_gemm_kernel(const HeadGemmParams p) {
  constexpr int C = 16 * KS, WIMG_B = 2 * 3 * KS * 1024;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sW = smem;
  float* sGN = (float*)(smem + WIMG_B);                  // [a | b][C] of the current slice
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  for (int i = tid; i < WIMG_B / 16; i += 256) *(u32x4*)(sW + i * 16) = *(const u32x4*)(p.wimg + i * 16);
  const int64_t ngroups = (p.M + 127) / 128;
  const int64_t g0 = (int64_t)blockIdx.x * p.per_block, g1 = min(g0 + p.per_block, ngroups);
  int cur_slice = -1;
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t m = g * 128 + wave * 32 + l31;
    const bool ok = m < p.M;
    const int64_t mc = ok ? m : p.M - 1;
    u32x4 xa[KS];
    const char* ap = p.x + (mc * p.ldx + half * 8) * 2;
#pragma unroll
    for (int cg = 0; cg < KS; ++cg) xa[cg] = *(const u32x4*)(ap + cg * 32);
    const int slice = (int)((g * 128) / p.gn_rows);       // gn_rows % 128 == 0: a 128-row group lies inside one slice (block-uniform)
    if (slice != cur_slice) {
      __syncthreads();                                     // every wave is past its reads of the previous table (and of nothing, first time)
      for (int i = tid; i < 2 * C; i += 256) sGN[i] = (i < C ? p.gn_a : p.gn_b)[(int64_t)slice * C + (i < C ? i : i - C)];
      cur_slice = slice;
      __syncthreads();                                     // (also covers the weight image on the first pass)
    }
#pragma unroll
    for (int cg = 0; cg < KS; ++cg) {
      float v[8];
      Elt<__bf16>::unpack(xa[cg], v);
      const float* a4 = sGN + cg * 16 + half * 8;
#pragma unroll
      for (int e = 0; e < 8; e += 4) {
        const f32x4 av = *(const f32x4*)(a4 + e), bv = *(const f32x4*)(a4 + C + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float y = v[e + k] * av[k] + bv[k];
          v[e + k] = p.act ? silu_f(y) : y;
        }
      }
      u32x4 y = Elt<__bf16>::pack(v);
      asm volatile("" : "+v"(y.x), "+v"(y.y), "+v"(y.z), "+v"(y.w));      // keep the normalisation here (see the strip GEMM)
      xa[cg] = y;
    }
#pragma unroll
    for (int ob = 0; ob < 3; ++ob) {
      if (ob * 32 >= p.NO) break;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int hl = 0; hl < 2; ++hl)
#pragma unroll
        for (int cg = 0; cg < KS; ++cg) {
          const u32x4 fw = *(const u32x4*)(sW + (((hl * 3 + ob) * KS + cg) * 64 + lane) * 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fw), __builtin_bit_cast(bf16x8, xa[cg]), acc, 0, 0, 0);
        }
      // acc[4 q + j] = output 32 ob + 8 q + 4 half + j of row m: lanes 0 - 31 of a register are 32 consecutive m of one plane (128 bytes)
      if (ok) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int o = ob * 32 + 8 * q + 4 * half + j;
            if (o < p.NO) p.P[(int64_t)o * p.M + m] = acc[4 * q + j];
          }
      }
    }
  }
}

struct HeadGatherParams {
  const float* P; int64_t M; const float* bias; float* y;
  int N, F, H, W, Co, ntaps;
  int taps[27 * 3];
};
template <int CO>
__global__ __launch_bounds__(256) void head_gather_kernel(const HeadGatherParams p) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= p.M) return;
  const int w = (int)(m % p.W), h = (int)((m / p.W) % p.H);
  const int64_t nf = m / ((int64_t)p.W * p.H);
  const int f = (int)(nf % p.F);
  const int64_t HW = (int64_t)p.H * p.W;
  float acc[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) acc[c] = p.bias ? p.bias[c] : 0.f;
  // nine taps per trip: their 9 CO loads are independent and issue together (branch-free: a tap outside the frame reads the centre
  // element and is multiplied by zero); the sum runs in tap order
  for (int t0 = 0; t0 < p.ntaps; t0 += 9) {
    float v[9][CO], k[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int t = min(t0 + u, p.ntaps - 1);
      const int df = p.taps[3 * t], dh = p.taps[3 * t + 1], dw = p.taps[3 * t + 2];
      const bool ok = t0 + u < p.ntaps && (unsigned)(f + df) < (unsigned)p.F && (unsigned)(h + dh) < (unsigned)p.H && (unsigned)(w + dw) < (unsigned)p.W;
      const int64_t src = ok ? m + df * HW + dh * p.W + dw : m;
      k[u] = ok ? 1.f : 0.f;
#pragma unroll
      for (int c = 0; c < CO; ++c) v[u][c] = p.P[(int64_t)(t * CO + c) * p.M + src];
    }
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int c = 0; c < CO; ++c) acc[c] += k[u] * v[u][c];
  }
  const int64_t n = nf / p.F;
#pragma unroll
  for (int c = 0; c < CO; ++c) p.y[(((n * p.F + f) * CO + c) * p.H + h) * (int64_t)p.W + w] = acc[c];
}

extern "C" int64_t mmd_head_gemm_weight_bytes(int Cin) { return (Cin == 128) ? 2 * 3 * (Cin / 16) * 1024 : 0; }
extern "C" int64_t mmd_head_gemm_workspace_bytes(int64_t M, int ntaps, int Co) { return (int64_t)ntaps * Co * M * 4; }

// P = W act(x a + b): x bf16 rows [M, Cin] (Cin = 128), a / b fp32 [S, Cin] = the fused GroupNorm affine over S slices of gn_rows rows
// (gn_rows % 128 == 0; a == NULL is not supported: the head always follows its norm), wimg = the packed (hi, lo) weight image
// (mmd_head_gemm_weight_bytes; packed by the host mirror), P fp32 [ntaps * Co][M].
extern "C" int mmd_head_gemm(const void* x, int64_t ldx, int64_t M, int Cin, const float* gn_a, const float* gn_b, int S, int64_t gn_rows,
                             int act, const void* wimg, float* P, int NO, void* stream) {
  MMD_REQUIRE(x && gn_a && gn_b && wimg && P && M > 0, "head_gemm: null pointer / empty");
  MMD_REQUIRE(Cin == 128, "head_gemm: built for 128 input channels (got %d)", Cin);
  MMD_REQUIRE(NO >= 1 && NO <= 96, "head_gemm: 1 .. 96 outputs (taps x channels), got %d", NO);
  MMD_REQUIRE(S > 0 && gn_rows > 0 && gn_rows % 128 == 0 && (int64_t)S * gn_rows == M, "head_gemm: S x gn_rows must tile the rows in multiples of 128");
  MMD_REQUIRE(((uintptr_t)x | (uintptr_t)wimg) % 16 == 0 && ldx % 8 == 0 && (uintptr_t)P % 4 == 0, "head_gemm: unaligned operand");
  HeadGemmParams p;
  p.x = (const char*)x; p.ldx = ldx; p.M = M; p.gn_a = gn_a; p.gn_b = gn_b; p.gn_rows = gn_rows; p.gn_S = S; p.act = act;
  p.wimg = (const char*)wimg; p.P = P; p.NO = NO;
  const int64_t ngroups = (M + 127) / 128;
  p.per_block = (int)max((int64_t)1, (ngroups + 1023) / 1024);          // <= 1024 blocks: two per CU, each a run of consecutive row groups
  const int grid = (int)((ngroups + p.per_block - 1) / p.per_block);
  const size_t lds = 2 * 3 * 8 * 1024 + 2 * 128 * sizeof(float);
  return mmd_launch<head_gemm_kernel<8>>("head_gemm", dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
}

// y[n, f, co, h, w] = bias[co] + sum_tap P[tap Co + co][m + offset(tap)] (zero outside (F, H, W)); y fp32 API layout [N, F, Co, H, W].
extern "C" int mmd_head_gather(const float* P, const float* bias, float* y, int N, int F, int H, int W, int Co, int ntaps, const int* taps,
                               void* stream) {
  MMD_REQUIRE(P && y && taps && N > 0 && F > 0 && H > 0 && W > 0 && ntaps >= 1 && ntaps <= 27, "head_gather: bad argument");
  MMD_REQUIRE(Co == 1 || Co == 2 || Co == 3 || Co == 4 || Co == 6, "head_gather: Co in {1, 2, 3, 4, 6} (got %d)", Co);
  HeadGatherParams p;
  p.P = P; p.M = (int64_t)N * F * H * W; p.bias = bias; p.y = y; p.N = N; p.F = F; p.H = H; p.W = W; p.Co = Co; p.ntaps = ntaps;
  for (int i = 0; i < ntaps * 3; ++i) p.taps[i] = taps[i];
  const int grid = (int)((p.M + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  switch (Co) {
    case 1: return mmd_launch<head_gather_kernel<1>>("head_gather", dim3(grid), dim3(256), 0, st, p);
    case 2: return mmd_launch<head_gather_kernel<2>>("head_gather", dim3(grid), dim3(256), 0, st, p);
    case 3: return mmd_launch<head_gather_kernel<3>>("head_gather", dim3(grid), dim3(256), 0, st, p);
    case 4: return mmd_launch<head_gather_kernel<4>>("head_gather", dim3(grid), dim3(256), 0, st, p);
    default: return mmd_launch<head_gather_kernel<6>>("head_gather", dim3(grid), dim3(256), 0, st, p);
  }
}

extern "C" int mmd_head_conv(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, float* y, int N, int F,
                             int Cin, int H, int W, int Co, int ntaps, const int* taps, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "head_conv: bad dtype");
  MMD_REQUIRE(x && w && y && taps && ntaps >= 1 && ntaps <= 27 && Cin % epv == 0 && Co >= 1 && Co <= 8, "head_conv: bad argument");
  HeadConvParams p;
  p.x = (const char*)x; p.ldx = ldx; p.w = w; p.bias = bias; p.y = y;
  p.N = N; p.F = F; p.Cin = Cin; p.H = H; p.W = W; p.Co = Co; p.ntaps = ntaps;
  for (int i = 0; i < ntaps * 3; ++i) p.taps[i] = taps[i];
  hipStream_t st = (hipStream_t)stream;
  return dtype == MMD_BF16 ? launch_head<__bf16>(p, st) : launch_head<float>(p, st);
}

// ----------------------------------------------------------------------------- super-resolution model input
// ImageSuperResModel.forward (image_unet.py:704-715): out[n, 0:C] = x[n], out[n, C:2C] = F.interpolate(low_res[n], (H, W),
// mode="bilinear") (align_corners=False: src = (dst + 0.5) * in/out - 0.5 clamped at 0, neighbours clamped at the edge).
__global__ __launch_bounds__(256) void bilinear_concat_kernel(const float* __restrict__ x, const float* __restrict__ low, float* __restrict__ out,
                                                              int N, int C, int H, int W, int h, int w) {
  const int64_t total = (int64_t)N * 2 * C * H * W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int xo = (int)(i % W), yo = (int)((i / W) % H);
    const int c = (int)((i / ((int64_t)W * H)) % (2 * C));
    const int64_t n = i / ((int64_t)W * H * 2 * C);
    if (c < C) {
      out[i] = x[((n * C + c) * H + yo) * (int64_t)W + xo];
    } else {
      const float fy = fmaxf(((float)yo + 0.5f) * sh - 0.5f, 0.f), fx = fmaxf(((float)xo + 0.5f) * sw - 0.5f, 0.f);
      const int y0 = (int)fy, x0 = (int)fx;
      const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
      const float ly = fy - (float)y0, lx = fx - (float)x0;
      const float* p = low + (n * C + (c - C)) * (int64_t)h * w;
      out[i] = (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) + ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
    }
  }
}
extern "C" int mmd_bilinear_concat(const float* x, const float* low, float* out, int N, int C, int H, int W, int h, int w, void* stream) {
  MMD_REQUIRE(x && low && out && N > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0, "bilinear_concat: bad argument");
  return mmd_launch<bilinear_concat_kernel>("bilinear_concat", dim3(ew_grid((int64_t)N * 2 * C * H * W)), dim3(256), 0, (hipStream_t)stream, x, low, out, N, C,
                                            H, W, h, w);
}

// The same input as channels-last ROWS for the implicit-GEMM stem: rows[(n, y, x), 0:C] = x, [C:2C] = bilinear(low), [2C:Cpad] = 0.
// The direct stem kernel spent 3.3 ms per evaluation on the 16 x 256 x 256 frames of a clip (6 -> 192 channels); as a K = 9 * 8
// GEMM on rows the stem is one pass of output-write bandwidth.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_concat_rows_kernel(const float* __restrict__ x, const float* __restrict__ low, char* __restrict__ out,
                                                                   int N, int C, int H, int W, int h, int w, int Cpad) {
  const int64_t rows = (int64_t)N * H * W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < rows; m += (int64_t)gridDim.x * 256) {
    const int xo = (int)(m % W), yo = (int)((m / W) % H);
    const int64_t n = m / ((int64_t)W * H);
    const float fy = fmaxf(((float)yo + 0.5f) * sh - 0.5f, 0.f), fx = fmaxf(((float)xo + 0.5f) * sw - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    for (int c = 0; c < Cpad; ++c) {
      float v = 0.f;
      if (c < C) {
        v = x[((n * C + c) * H + yo) * (int64_t)W + xo];
      } else if (c < 2 * C) {
        const float* p = low + (n * C + (c - C)) * (int64_t)h * w;
        v = (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) + ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
      }
      Elt<T>::st(out, m * Cpad + c, v);
    }
  }
}
extern "C" int mmd_bilinear_concat_rows(int dtype, const float* x, const float* low, void* out, int N, int C, int H, int W, int h, int w,
                                        int Cpad, void* stream) {
  MMD_REQUIRE(x && low && out && N > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && Cpad >= 2 * C, "bilinear_concat_rows: bad argument");
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "bilinear_concat_rows: bad dtype");
  const dim3 grid(ew_grid((int64_t)N * H * W));
  return mmd_by_dtype(dtype, [&](auto t) {
    return mmd_launch<bilinear_concat_rows_kernel<typename decltype(t)::type>>("bilinear_concat_rows", grid, dim3(256), 0, (hipStream_t)stream, x, low,
                                                                               (char*)out, N, C, H, W, h, w, Cpad);
  });
}
