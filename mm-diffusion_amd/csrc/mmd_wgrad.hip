// Convolution weight gradient of the training step (multimodal_training_losses backward, reference gd:1114-1203 through the U-Net).
//
//   conv wgrad   dW[co, tap*Cin + ci] += sum_m dY[m, co] * X[src(m, tap), ci]        (implicit GEMM, reduction over rows)
//   conv dgrad   = mmd_conv_gemm on dY with the transposed weight and mirrored taps   (no new kernel)
//   colsum       db[c] += sum_m dY[m, c]
// Accumulation into dW / db uses fp32 L2 atomics over row splits (like the vendor conv backward, run-to-run bit
// differences of the last ulp are possible).  The GroupNorm backward is in mmd_gn_bwd.hip, the optimizer in mmd_optim.hip.
#include "mmd_common.h"

// ============================================================================= conv wgrad (implicit GEMM-TN on MFMA)
struct WgradParams {
  const char* dY; int64_t lddy;      // [M, Cout]
  const char* X; int64_t ldx;        // [rows, Cin]
  float* dW;                         // fp32, accumulated with atomics: [Cout][ntaps*Cin] (packed) or [Cout][Cin][ntaps] (torch conv layout)
  float* db;                         // 128-tile kernels: bias gradient (column sums of dY) accumulated by the (tap 0, ci tile 0) blocks
  int torch_layout;
  int M, Cout, Cin, ntaps;
  int D0, D1, D2;
  int rows_per_split, splits, xcd_order;
  int taps[27 * 3];
};

// ----------------------------------------------------------------------------- the tile core of wgrad_kernel<T> and wgrad_tr_bf16_kernel
// A block owns a TW (co) x TW (ci of ONE tap) tile of dW over the rows [m_begin, m_end) of one split.  kt = (tap, ci tile) index.
struct WgTile {
  int tap, ci0, co0;
  int o0, o1, o2, D12;               // the tap's offsets in the (D0, D1, D2) frame
  int64_t roff;                      // ... and as a row offset into X
  int m_begin, m_end;
};
template <int TW>
__device__ __forceinline__ WgTile wg_tile(const WgradParams& p, int kt, int co_blk, int split) {
  const int ci_tiles = (p.Cin + TW - 1) / TW;
  WgTile t;
  t.tap = kt / ci_tiles;
  t.ci0 = (kt % ci_tiles) * TW;
  t.co0 = co_blk * TW;
  t.o0 = p.taps[t.tap * 3], t.o1 = p.taps[t.tap * 3 + 1], t.o2 = p.taps[t.tap * 3 + 2];
  t.D12 = p.D1 * p.D2;
  t.roff = (int64_t)t.o0 * t.D12 + t.o1 * p.D2 + t.o2;
  t.m_begin = split * p.rows_per_split;
  t.m_end = min(t.m_begin + p.rows_per_split, p.M);
  return t;
}
// Row m shifted by the tile's tap is inside the frame (else the tap reads padding: zero).  The VGPR-staged kernels; the DMA kernel has
// its own float-reciprocal form.
__device__ __forceinline__ bool wg_row_in_frame(const WgradParams& p, const WgTile& t, int m) {
  const int p2 = m % p.D2, p1 = (m / p.D2) % p.D1, p0 = (m / t.D12) % p.D0;
  return (unsigned)(p0 + t.o0) < (unsigned)p.D0 && (unsigned)(p1 + t.o1) < (unsigned)p.D1 && (unsigned)(p2 + t.o2) < (unsigned)p.D2;
}
// The wave's NT x NT 32x32 MFMA accumulators (wave tile wi, wj of the block tile) into dW.  D[row = co][col = ci]: the lane holds
// ci = l31 and co = (r&3) + 8*(r>>2) + 4*half of each 32x32 tile.  Every field of p is read before the first atomic.
template <int NT>
__device__ __forceinline__ void wg_scatter(const WgradParams& p, const WgTile& t, int wi, int wj, int l31, int half, const f32x16 (&acc)[NT][NT]) {
  float* const dW = p.dW;
  const int Cout = p.Cout, Cin = p.Cin, ntaps = p.ntaps, torch_layout = p.torch_layout;
  const int64_t K = (int64_t)Cin * ntaps;
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const int ci = t.ci0 + (wj * NT + b) * 32 + l31;
      float* col = dW + (torch_layout ? (int64_t)ci * ntaps + t.tap : (int64_t)t.tap * Cin + ci);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = t.co0 + (wi * NT + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co < Cout && ci < Cin) atomicAdd(col + (int64_t)co * K, acc[a][b][r]);
      }
    }
}

// Block = 64 (co) x 64 (ci of ONE tap) output tile x one row split; 4 waves, each a 32x32 MFMA tile.
// The reduction index is the row m, so both operands are needed "column-wise" (8 consecutive rows of one channel):
// tiles are staged row-major in LDS (coalesced 16-B loads) and the fragments are gathered with 2-byte LDS reads
// (bf16) / 4-byte reads (fp32), which are conflict free because adjacent lanes read adjacent channels.
template <typename T>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  constexpr int MT = 64;                       // rows per staged chunk
  constexpr int LDT = 64 * ES + 16;            // bytes per staged row (64 channels + pad)
  __shared__ __attribute__((aligned(16))) char sdy[MT * LDT];
  __shared__ __attribute__((aligned(16))) char sx[MT * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave & 1, wj = wave >> 1;     // wave tile: co 32*wi, ci 32*wj
  const int half = lane >> 5, l31 = lane & 31;
  const WgTile t = wg_tile<64>(p, blockIdx.y, blockIdx.x, blockIdx.z);
  const int ci0 = t.ci0, co0 = t.co0, m_end = t.m_end;

  f32x16 acc[1][1];                            // 1 x 1: the array shape wg_scatter<NT> takes
  zero_acc(acc[0]);

  constexpr int VPR = 64 / EPV;                // 16-byte vecs per staged row
  for (int mc = t.m_begin; mc < m_end; mc += MT) {
    __syncthreads();
    for (int i = tid; i < MT * VPR; i += 256) {
      const int r = i / VPR, v = i % VPR;
      const int m = mc + r;
      u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
      if (m < m_end) {
        if (co0 + v * EPV < p.Cout) a = *(const u32x4*)(p.dY + ((int64_t)m * p.lddy + co0 + v * EPV) * ES);
        if (ci0 + v * EPV < p.Cin && wg_row_in_frame(p, t, m))
          b = *(const u32x4*)(p.X + (((int64_t)m + t.roff) * p.ldx + ci0 + v * EPV) * ES);
      }
      *(u32x4*)(sdy + r * LDT + v * 16) = a;
      *(u32x4*)(sx + r * LDT + v * 16) = b;
    }
    __syncthreads();
    if constexpr (EPV == 8) {
#pragma unroll
      for (int ks = 0; ks < MT / 16; ++ks) {        // 16 rows per MFMA: lane (channel l31, half) takes rows ks*16 + 8*half + j
        bf16x8 fa, fb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = ks * 16 + 8 * half + j;
          fa[j] = *(const __bf16*)(sdy + r * LDT + (wi * 32 + l31) * 2);
          fb[j] = *(const __bf16*)(sx + r * LDT + (wj * 32 + l31) * 2);
        }
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[0][0], 0, 0, 0);
      }
    } else {
#pragma unroll 8
      for (int ks = 0; ks < MT / 2; ++ks) {         // 2 rows per MFMA: lane half takes row 2*ks + half
        const int r = ks * 2 + half;
        const float fa = *(const float*)(sdy + r * LDT + (wi * 32 + l31) * 4);
        const float fb = *(const float*)(sx + r * LDT + (wj * 32 + l31) * 4);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[0][0], 0, 0, 0);
      }
    }
  }
  wg_scatter(p, t, wi, wj, l31, half, acc);
}

// bf16 weight gradient, 128 (co) x 128 (ci of ONE tap) tile per block, 4 waves each 64 x 64 (2 x 2 MFMA tiles).
// The reduction index is the row m, so both MFMA operands need 8 CONSECUTIVE ROWS of one channel per lane.  The 64-tile kernel
// above stages row-major and gathers every fragment with eight 2-byte LDS reads (16 reads per MFMA); here the 64-row chunk is
// transposed while it is stored to LDS ([channel][64 rows], 136-byte pitch: the 32-rows x 2-vectors lane pattern of the
// attention V^T staging, conflict free) and a fragment is two ds_read_b64 - 4 LDS reads per 4 MFMAs.  The next chunk's global
// loads are in flight under the MFMAs (register prefetch).
// This kernel keeps its OWN tile decode, row test and scatter: with the shared wg_tile / wg_row_in_frame / wg_scatter it measured 2 - 4 % slower
// at equal registers and instruction mix (profiles/bwd_split_core.txt), and it is the live fallback for M >= 2^24 or operands of 2 GiB.
#define WG_PITCH 136
__global__ __launch_bounds__(256, 2) void wgrad128_bf16_kernel(const WgradParams p) {
  __shared__ __attribute__((aligned(16))) char sA[128 * WG_PITCH];      // dY^T chunk: [co][m]
  __shared__ __attribute__((aligned(16))) char sB[128 * WG_PITCH];      // X^T  chunk: [ci][m]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave & 1, wj = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const int ci_tiles = (p.Cin + 127) / 128;
  const int kt = blockIdx.y;
  const int tap = kt / ci_tiles, ci0 = (kt % ci_tiles) * 128;
  const int co0 = blockIdx.x * 128;
  const int o0 = p.taps[tap * 3], o1 = p.taps[tap * 3 + 1], o2 = p.taps[tap * 3 + 2];
  const int D12 = p.D1 * p.D2;
  const int64_t roff = (int64_t)o0 * D12 + o1 * p.D2 + o2;
  const int m_begin = blockIdx.z * p.rows_per_split;
  const int m_end = min(m_begin + p.rows_per_split, p.M);

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // staging slots of this thread: 4 x (row j, 8-channel vector v) per operand
  int sj[4], sv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + 256 * i;
    sj[i] = (id & 31) + 32 * ((id >> 6) & 1);
    sv[i] = 2 * (id >> 7) + ((id >> 5) & 1);
  }
  u32x4 ra[4], rb[4];
  auto load_chunk = [&](int mc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mc + sj[i];
      u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
      if (m < m_end) {
        if (co0 + sv[i] * 8 < p.Cout) a = *(const u32x4*)(p.dY + ((int64_t)m * p.lddy + co0 + sv[i] * 8) * 2);
        const int p2 = m % p.D2, p1 = (m / p.D2) % p.D1, p0 = (m / D12) % p.D0;
        if (ci0 + sv[i] * 8 < p.Cin && (unsigned)(p0 + o0) < (unsigned)p.D0 && (unsigned)(p1 + o1) < (unsigned)p.D1 &&
            (unsigned)(p2 + o2) < (unsigned)p.D2)
          b = *(const u32x4*)(p.X + (((int64_t)m + roff) * p.ldx + ci0 + sv[i] * 8) * 2);
      }
      ra[i] = a;
      rb[i] = b;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t* da = (uint16_t*)(sA + (8 * sv[i]) * WG_PITCH + 2 * sj[i]);
      uint16_t* db = (uint16_t*)(sB + (8 * sv[i]) * WG_PITCH + 2 * sj[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        da[e * (WG_PITCH / 2)] = (uint16_t)((ra[i][e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        db[e * (WG_PITCH / 2)] = (uint16_t)((rb[i][e >> 1] >> ((e & 1) * 16)) & 0xffffu);
      }
    }
  };

  const bool do_db = p.db != nullptr && kt == 0;
  float dbacc = 0.f;
  load_chunk(m_begin);
  for (int mc = m_begin; mc < m_end; mc += 64) {
    __syncthreads();                 // previous chunk fully consumed
    store_chunk();
    __syncthreads();
    if (mc + 64 < m_end) load_chunk(mc + 64);
    if (do_db) {                     // bias gradient from the staged dY^T tile: thread = (channel, 32-row half); rows past m_end are zero
      const char* q = sA + (tid >> 1) * WG_PITCH + (tid & 1) * 64;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const u32x2 v = *(const u32x2*)(q + 8 * u);
        dbacc += __uint_as_float(v[0] << 16) + __uint_as_float(v[0] & 0xffff0000u) + __uint_as_float(v[1] << 16) + __uint_as_float(v[1] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const char* q = sA + (wi * 64 + a * 32 + l31) * WG_PITCH + (16 * ks + 8 * half) * 2;
        const u32x2 v0 = *(const u32x2*)q, v1 = *(const u32x2*)(q + 8);
        fa[a] = u32x4{v0[0], v0[1], v1[0], v1[1]};
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const char* q = sB + (wj * 64 + b * 32 + l31) * WG_PITCH + (16 * ks + 8 * half) * 2;
        const u32x2 v0 = *(const u32x2*)q, v1 = *(const u32x2*)(q + 8);
        fb[b] = u32x4{v0[0], v0[1], v1[0], v1[1]};
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[a]), __builtin_bit_cast(bf16x8, fb[b]), acc[a][b], 0, 0, 0);
    }
  }
  if (do_db) {
    dbacc += __shfl_xor(dbacc, 1, 64);
    const int co = co0 + (tid >> 1);
    if ((tid & 1) == 0 && co < p.Cout) atomicAdd(p.db + co, dbacc);
  }
  // D[row = co][col = ci]: lane holds ci = l31, co = (r&3) + 8*(r>>2) + 4*half of its 32x32 tile
  const int64_t K = (int64_t)p.Cin * p.ntaps;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ci = ci0 + wj * 64 + b * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wi * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co < p.Cout && ci < p.Cin)
          atomicAdd(p.dW + (int64_t)co * K + (p.torch_layout ? (int64_t)ci * p.ntaps + tap : (int64_t)tap * p.Cin + ci), acc[a][b][r]);
      }
    }
}

// bf16 weight gradient, round 3: the same 128 (co) x 128 (ci of ONE tap) tile per block, 4 waves each 64 x 64, but nothing is transposed
// by the kernel.  The reduction index is the row m, so both MFMA operands want 8 consecutive ROWS of one channel per lane - exactly what
// ds_read_b64_tr_b16 returns from a ROW-MAJOR tile.  A 64-row chunk of dY and of X therefore goes global -> LDS by buffer-descriptor DMA
// (no VGPR staging, no ds_write; a padding row or a row past the split is an out-of-range offset and lands as zeros), in the tile format
// of the attention kernel's V ([plane of 64 channels][64 rows][128 B], 16-byte chunk ^ (((row >> 1) & 1) << 2)), double buffered with one
// barrier per chunk; a fragment is two transposing reads.  wgrad128_bf16_kernel above spent 64 ds_write_b16 + 12 integer divisions per
// thread and chunk on what the DMA and two float reciprocals do here.  The column sums (bias gradient) ride in the (tap 0, ci tile 0) blocks (round 6).
__device__ __forceinline__ int wg_fdiv(int n, int d, float rd) {       // n / d for 0 <= n < 2^24 (the launcher checks M)
  int q = (int)((float)n * rd);
  const int r = n - q * d;
  q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
  return q;
}

__global__ __launch_bounds__(256, 2) void wgrad_tr_bf16_kernel(const WgradParams p) {
  constexpr int PLANE_B = 64 * 128, OP_B = 2 * PLANE_B, STAGE_B = 2 * OP_B;
  extern __shared__ __attribute__((aligned(16))) char smem_w[];        // [2 stages][dY | X][2 planes][64 rows][128 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave & 1, wj = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  // round 6: XCD-aware block order.  The (co tile, ci tile, tap) blocks of one row split read the SAME rows of dY (per co tile) and of X
  // (per ci tile, shifted by the tap): 9 - 27 blocks per split for the 3 x 3 convs.  Dispatched in grid order they land on all eight XCDs
  // (workgroup id % 8) and every L2 fetches its own copy.  The grid is one-dimensional and padded to 8 x (blocks per split) x ceil(splits / 8):
  // XCD k works through the splits k, k + 8, ..., the blocks of a split back to back on one L2 (1 - 3 MB of rows per split).
  int kt_blk, co_blk, split;
  {
    const int nx = (p.Cout + 127) / 128, per = nx * ((p.Cin + 127) / 128) * p.ntaps;
    const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
    split = p.xcd_order ? xcd + 8 * (j / per) : bid / per;
    const int inner = p.xcd_order ? j % per : bid % per;
    co_blk = inner % nx;
    kt_blk = inner / nx;
    if (split >= p.splits) return;                         // padding blocks (before any barrier)
  }
  const WgTile t = wg_tile<128>(p, kt_blk, co_blk, split);
  const int ci0 = t.ci0, co0 = t.co0, o0 = t.o0, o1 = t.o1, o2 = t.o2, m_begin = t.m_begin, m_end = t.m_end;
  const int roff = (int)t.roff;                             // the launcher keeps every byte offset of this kernel below 2 GiB
  const bool shifted = (o0 | o1 | o2) != 0;
  const float rD2 = 1.f / (float)p.D2, rD1 = 1.f / (float)p.D1, rD0 = 1.f / (float)p.D0;

  typedef __attribute__((address_space(3))) void* lptr_t;
  const auto rsrcY = __builtin_amdgcn_make_buffer_rsrc((void*)p.dY, 0, (int)((int64_t)p.M * p.lddy * 2), 0x00020000);
  const auto rsrcX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (int)((int64_t)p.M * p.ldx * 2), 0x00020000);
  // DMA: wave w stages row groups {w, w + 4} of every plane; lane L of a group covers row 8 g + L / 8, physical chunk L % 8
  const int lrow = lane >> 3, pc = lane & 7;
  int drow[2];
  uint32_t ycol[2][2], xcol[2][2];            // [row group][plane]: byte column of the lane's (logical) chunk, or ~0 past the channel count
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 8 * (wave + 4 * i) + lrow;
    drow[i] = row;
    const int lc = pc ^ (((row >> 1) & 1) << 2);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const int co = co0 + 64 * pl + 8 * lc, ci = ci0 + 64 * pl + 8 * lc;
      ycol[i][pl] = co < p.Cout ? (uint32_t)(co * 2) : 0xffffffffu;
      xcol[i][pl] = ci < p.Cin ? (uint32_t)(ci * 2) : 0xffffffffu;
    }
  }
  const uint32_t ldyb = (uint32_t)(p.lddy * 2), ldxb = (uint32_t)(p.ldx * 2);
  auto issue = [&](int stage, int mc) {
    char* sb = smem_w + stage * STAGE_B;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mc + drow[i];
      const bool okm = m < m_end;
      bool okx = okm;
      if (shifted) {
        const int q1 = wg_fdiv(m, p.D2, rD2), p2 = m - q1 * p.D2;
        const int q2 = wg_fdiv(q1, p.D1, rD1), p1 = q1 - q2 * p.D1;
        const int q3 = wg_fdiv(q2, p.D0, rD0), p0 = q2 - q3 * p.D0;
        okx = okm && (unsigned)(p0 + o0) < (unsigned)p.D0 && (unsigned)(p1 + o1) < (unsigned)p.D1 && (unsigned)(p2 + o2) < (unsigned)p.D2;
      }
      const uint32_t yrow = (uint32_t)m * ldyb, xrow = (uint32_t)(m + roff) * ldxb;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const uint32_t yo = okm && ycol[i][pl] != 0xffffffffu ? yrow + ycol[i][pl] : 0xfffffff0u;
        const uint32_t xo = okx && xcol[i][pl] != 0xffffffffu ? xrow + xcol[i][pl] : 0xfffffff0u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcY, (lptr_t)(sb + pl * PLANE_B + (wave + 4 * i) * 1024), 16, yo, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcX, (lptr_t)(sb + OP_B + pl * PLANE_B + (wave + 4 * i) * 1024), 16, xo, 0, 0, 0);
      }
    }
  };

  f32x16 acc[2][2];
  zero_acc(acc[0]);
  zero_acc(acc[1]);
  // transposing reads: this lane supplies row base + 4 half + (lane & 15) / 4, byte column 32 ((lane >> 4) & 1) + 8 (lane & 3) of a 64-byte
  // channel tile, and receives the four rows base + 4 half + [0, 4) of channel l31 of that tile
  const int vrow0 = 4 * half + ((lane & 15) >> 2);
  const int vcolb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  typedef __attribute__((address_space(3))) s16x4* lp4;
  auto frag = [&](const char* plane, int rbase, int ct) -> bf16x8 {
    s16x4 lo, hi;
    {
      const int row = rbase + vrow0;
      const int ch = ((vcolb >> 4) + 4 * ct) ^ (((row >> 1) & 1) << 2);
      lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(plane + row * 128 + ch * 16 + (vcolb & 15)));
    }
    {
      const int row = rbase + 8 + vrow0;
      const int ch = ((vcolb >> 4) + 4 * ct) ^ (((row >> 1) & 1) << 2);
      hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(plane + row * 128 + ch * 16 + (vcolb & 15)));
    }
    const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
  };

  // bias gradient (round 6: db != NULL): the (tap 0, ci tile 0) blocks sum the columns of the dY stage they have in LDS anyway - thread =
  // (channel tid & 127, row half tid >> 7): a wave reads 128 contiguous bytes of a row per step (the chunk swizzle permutes 16-byte pieces
  // inside them), rows past the split are zero-filled by the DMA.  No colsum launch: the 1x1 / k = 3 convs can use this kernel too.
  const bool do_db = p.db != nullptr && kt_blk == 0;
  float dbacc = 0.f;
  const int dbc = tid & 127, dbh = tid >> 7;
  int stage = 0;
  if (m_begin < m_end) issue(0, m_begin);
  for (int mc = m_begin; mc < m_end; mc += 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this chunk's DMA (the only one in flight) has landed
    __builtin_amdgcn_s_barrier();                           // ... for every wave; everyone is past its reads of the other stage
    asm volatile("" ::: "memory");
    if (mc + 64 < m_end) issue(stage ^ 1, mc + 64);         // in flight under this chunk's MFMAs
    const char* pa = smem_w + stage * STAGE_B + wi * PLANE_B;
    const char* pb = smem_w + stage * STAGE_B + OP_B + wj * PLANE_B;
    if (do_db) {                                            // block-uniform
      const char* q = smem_w + stage * STAGE_B + (dbc >> 6) * PLANE_B + (dbc & 7) * 2;
      const int lc = (dbc & 63) >> 3;
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        const int row = 32 * dbh + r;
        const uint16_t v = *(const uint16_t*)(q + row * 128 + ((lc ^ (((row >> 1) & 1) << 2)) * 16));
        dbacc += __uint_as_float((uint32_t)v << 16);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {                        // 16 rows per k-step
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) fa[a] = frag(pa, 16 * ks, a);
#pragma unroll
      for (int b = 0; b < 2; ++b) fb[b] = frag(pb, 16 * ks, b);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    stage ^= 1;
  }
  if (do_db && co0 + dbc < p.Cout) atomicAdd(p.db + co0 + dbc, dbacc);
  wg_scatter(p, t, wi, wj, l31, half, acc);
}

// db[c] += sum over rows of dY[m, c]
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const char* __restrict__ dy, int64_t ld, int M, int C, float* __restrict__ out,
                                                     int rows_per_block) {
  constexpr int EPV = Elt<T>::EPV;
  constexpr int ES = 16 / EPV;
  __shared__ float s_sum[256 * EPV];
  const int tid = threadIdx.x;
  const int CV = C / EPV, RPP = 256 / CV;
  const int col = tid % CV, rl = tid / CV;
  float sum[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) sum[e] = 0.f;
  const int m0 = blockIdx.x * rows_per_block, m1 = min(m0 + rows_per_block, M);
  if (rl < RPP) {
    int m = m0 + rl;
    for (; m + 3 * RPP < m1; m += 4 * RPP) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const u32x4*)(dy + ((int64_t)(m + u * RPP) * ld + col * EPV) * ES);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[EPV];
        Elt<T>::unpack(v[u], f);
#pragma unroll
        for (int e = 0; e < EPV; ++e) sum[e] += f[e];
      }
    }
    for (; m < m1; m += RPP) {
      float f[EPV];
      Elt<T>::unpack(*(const u32x4*)(dy + ((int64_t)m * ld + col * EPV) * ES), f);
#pragma unroll
      for (int e = 0; e < EPV; ++e) sum[e] += f[e];
    }
#pragma unroll
    for (int e = 0; e < EPV; ++e) s_sum[rl * C + col * EPV + e] = sum[e];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int r = 0; r < RPP; ++r) a += s_sum[r * C + c];
    atomicAdd(out + c, a);
  }
}

// ============================================================================= C-ABI
// Row splits of a launch with `tiles` blocks per split aiming at `target` blocks: whole 64-row chunks, at least 256 rows per split.
struct WgSplit { int splits, rows; };
static WgSplit wg_split(int M, int tiles, int target) {
  const int sp = max(1, min(cdiv(M, 256), target / max(tiles, 1)));
  const int rows = cdiv(cdiv(M, sp), 64) * 64;
  return {cdiv(M, rows), rows};
}
// out[c] += column sums of the M rows at dy.  A block covers <= 256 16-byte column vectors: wide fp32 outputs (qkv 1536) go in slabs.
static int colsum_launch(const char* what, int dtype, const char* dy, int64_t ld, int M, int C, float* out, hipStream_t st) {
  const int epv = dtype == MMD_BF16 ? 8 : 4, es = 16 / epv;
  const int rpb = M >= 65536 ? 256 : 128;
  for (int c0 = 0; c0 < C; c0 += 256 * epv) {
    const int cw = C - c0 < 256 * epv ? C - c0 : 256 * epv;
    const int rc = mmd_by_dtype(dtype, [&](auto t) {
      return mmd_launch<colsum_kernel<typename decltype(t)::type>>(what, dim3(cdiv(M, rpb)), dim3(256), 0, st, dy + (int64_t)c0 * es, ld, M, cw, out + c0, rpb);
    });
    if (rc) return rc;
  }
  return MMD_OK;
}

// dW (fp32 [Cout][ntaps*Cin], caller zeroes it) += dY^T * gather(X); db (nullable, fp32 [Cout], zeroed) += colsum(dY).
extern "C" int mmd_conv_wgrad(int dtype, const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, float* db, int M, int Cout,
                              int Cin, int ntaps, const int* taps, int D0, int D1, int D2, int torch_layout, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "conv_wgrad: bad dtype");
  MMD_REQUIRE(dY && X && dW && taps && M > 0 && ntaps >= 1 && ntaps <= 27, "conv_wgrad: bad argument");
  MMD_REQUIRE(Cin % epv == 0 && Cout % epv == 0 && lddy % epv == 0 && ldx % epv == 0, "conv_wgrad: channel counts / strides must be 16-byte multiples");
  MMD_REQUIRE(((uintptr_t)dY | (uintptr_t)X) % 16 == 0, "conv_wgrad: unaligned pointer");
  WgradParams p;
  p.dY = (const char*)dY; p.lddy = lddy; p.X = (const char*)X; p.ldx = ldx; p.dW = dW; p.db = nullptr; p.torch_layout = torch_layout;
  p.M = M; p.Cout = Cout; p.Cin = Cin; p.ntaps = ntaps; p.D0 = D0; p.D1 = D1; p.D2 = D2;
  for (int i = 0; i < ntaps * 3; ++i) p.taps[i] = taps[i];
  hipStream_t st = (hipStream_t)stream;
  static const bool use128 = !mmd_env_set("MMD_WGRAD_TILE64");           // A/B switch for tools/wgrad_bench.py
  if (use128 && dtype == MMD_BF16 && Cout >= 64 && Cin >= 64) {          // the 128x128 kernels
    const int tiles = cdiv(Cout, 128) * cdiv(Cin, 128) * ntaps;
    // Row splits per launch.  Every split adds Cout * Cin * ntaps atomics on the same addresses; the blocks of a split share its rows of dY / X.
    // Round 6 (XCD-aware block order in wgrad_tr_bf16_kernel: a split count that is a multiple of 8 gives every XCD whole splits, the blocks of
    // a split back to back on ONE L2; other counts run in plain grid order): the candidates are what the block targets 256 ... 2048 give, and
    // the choice is a three-term cost fitted to a sweep of the training shapes (profiles/r06_wgrad_xcd_order.txt: it picks the measured best
    // or within 3 % of it on all 13): rounds of blocks on the 64 (per XCD) / 512 (chip) block slots x (rows per split + 300) + 40 x splits.
    // MMD_WGRAD_BLOCKS: one fixed target (the sweep).
    auto derive = [&](int target, int& sp, int& rps, int& xo) {
      const WgSplit w = wg_split(M, tiles, target);
      sp = w.splits, rps = w.rows, xo = 0;
      for (int s8 = sp / 8 * 8; s8 >= 8; s8 -= 8) {
        const int r = cdiv(cdiv(M, s8), 64) * 64;
        if (cdiv(M, r) % 8 == 0) { rps = r; sp = cdiv(M, r); xo = 1; break; }
      }
    };
    int splits = 1, xo = 0;
    p.rows_per_split = M;
    {
      static const int env_target = mmd_env_int("MMD_WGRAD_BLOCKS", 0);
      static const int targets[] = {256, 384, 512, 768, 1024, 1536, 2048};
      int64_t best = -1;
      for (int t : targets) {
        int sp, rps, x;
        derive(env_target > 0 ? env_target : t, sp, rps, x);
        const int64_t rounds = x ? cdiv((int64_t)tiles * (sp / 8), 64) : cdiv((int64_t)tiles * sp, 512);
        const int64_t cost = rounds * (rps + 300) + 40 * (int64_t)sp;
        if (best < 0 || cost < best) { best = cost; splits = sp; p.rows_per_split = rps; xo = x; }
      }
    }
    p.xcd_order = xo;
    p.splits = splits;
    p.db = db;                                                   // column sums ride in the (tap 0, ci tile 0) blocks: no colsum launch
    // DMA-staged kernel (round 3; MMD_WGRAD_TR=0: the transposed-staging kernel): 32-bit byte offsets, float-reciprocal row positions
    static const char tr_env = mmd_env_char("MMD_WGRAD_TR");
    const bool use_tr = tr_env != '0';
    // measured (tools/wgrad_bench.py, batch 8): 3x3 ds1 128->128 436 -> 372 us, ds2 256->256 405 -> 251, ds4 384->384 240 -> 180, ds8 130 -> 110;
    // the 1x1 / k=3 convs lose what the separate colsum launch costs (1x1 ds1: 82 -> 127 us), so they stay on the older kernel
    // round 6: the bias gradient rides in the kernel (no colsum launch), so every tap count uses it; MMD_WGRAD_TR=9: the 9-tap convs only
    const int tr_min_taps = tr_env == '9' ? 9 : 1;
    if (use_tr && ntaps >= tr_min_taps && M < (1 << 24) && (int64_t)M * lddy * 2 < 0x7fffffffLL && (int64_t)M * ldx * 2 < 0x7fffffffLL) {
      const size_t lds = 2 * 4 * 64 * 128;
      return mmd_launch<wgrad_tr_bf16_kernel>("conv_wgrad", dim3(p.xcd_order ? 8 * tiles * cdiv(splits, 8) : tiles * splits), dim3(256), lds, st, p);
    }
    return mmd_launch<wgrad128_bf16_kernel>("conv_wgrad", dim3(cdiv(Cout, 128), cdiv(Cin, 128) * ntaps, splits), dim3(256), 0, st, p);
  }
  const WgSplit w = wg_split(M, cdiv(Cout, 64) * cdiv(Cin, 64) * ntaps, 2048);
  p.rows_per_split = w.rows;
  dim3 grid(cdiv(Cout, 64), cdiv(Cin, 64) * ntaps, w.splits);
  const int rc = mmd_by_dtype(dtype, [&](auto t) { return mmd_launch<wgrad_kernel<typename decltype(t)::type>>("conv_wgrad", grid, dim3(256), 0, st, p); });
  if (rc || !db) return rc;
  return colsum_launch("colsum", dtype, (const char*)dY, lddy, M, Cout, db, st);
}

// out[s, c] += sum over the Tn rows of slice s of dY[row, c] (S contiguous slices): the gradient of a per-sample row bias - the
// non-FiLM ResBlock's h + emb_out (unet:473-477).  `out` [S, ldo] fp32 is ACCUMULATED (caller zeroes).
extern "C" int mmd_colsum_slices(int dtype, const void* dY, int64_t lddy, int S, int64_t Tn, int C, float* out, int64_t ldo, void* stream) {
  const int epv = dtype == MMD_BF16 ? 8 : 4, es = dtype == MMD_BF16 ? 2 : 4;
  MMD_REQUIRE(dtype == MMD_BF16 || dtype == MMD_F32, "colsum_slices: bad dtype");
  MMD_REQUIRE(dY && out && S > 0 && Tn > 0 && C > 0 && C % epv == 0 && lddy % epv == 0 && ((uintptr_t)dY) % 16 == 0, "colsum_slices: bad argument");
  for (int s = 0; s < S; ++s)
    if (const int rc = colsum_launch("colsum_slices", dtype, (const char*)dY + (int64_t)s * Tn * lddy * es, lddy, (int)Tn, C, out + (int64_t)s * ldo,
                                     (hipStream_t)stream))
      return rc;
  return MMD_OK;
}
