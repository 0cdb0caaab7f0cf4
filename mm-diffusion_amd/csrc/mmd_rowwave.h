// The row-wave epilogue: what a kernel whose wave owns 32 rows x 32-column MFMA sub-tiles does with its accumulators, and the ONE
// place where the fold order of the quad statistics records is written down.  Users: mmd_aconv, mmd_res_tail, mmd_vconv2d1d (both
// epilogues), the MFMA stem conv, and the block remap of the conv-GEMM kernels.  Three kernels keep private copies of the epilogue that
// must follow the order below: the hand-scheduled row-strip GEMM (mmd_gemm.hip: conv1x1_strip_body, the original these helpers were
// lifted from), mmd_tconv and mmd_tattn_block - converted, the last two measured 0.1 - 0.4 us per launch behind their private copies
// (profiles/rowwave_epilogue_device_code.txt).
//
// Layout.  After v_mfma_f32_32x32x16_bf16 with the weights as A and the rows as B, lane (l31 = lane & 31, half = lane >> 5) holds
// acc[4 q + j] = channel 8 q + 4 half + j of row l31 of the sub-tile.  v_permlane32_swap pairs q = 2 j2 (vdst) with q = 2 j2 + 1 (src)
// across the half-waves: afterwards the lane holds the 8 CONSECUTIVE channels 16 j2 + 8 half .. + 8 of its row (acc_octet) - one 16-byte
// store, and two channel quads of a statistics record.
//
// Fold order of a record (sum, sum of squares of one channel quad over 64 rows; the GroupNorm that consumes them needs them bitwise
// equal to what the unfused launches write, and the tests pin that):
//   1. the values are the ones STORED: packed to bf16, unpacked again (quad_sums);
//   2. per lane, four running sums u = {sum quad 0, sum quad 1, squares quad 0, squares quad 1}, each over its quad's four channels in
//      ascending order, squares as u += x * x; a lane that holds two rows of the record (row r, then row r + 32: the strip kernel's two
//      fragments, vconv's two frames, res_tail's two-fragment fold) CONTINUES the same four sums with the second row;
//   3. halfwave_total of each of the four over the 32 lanes of a half-wave; lanes 16 / 17 of each half then take quad 0 / 1 (quad_fold,
//      is_record_lane);
//   4. a wave that holds only half a record (32 rows, one row per lane): the odd wave of a pair parks its (sum, squares) in LDS, and
//      behind a barrier the even wave writes own + partner, in that order (quad_put, half_record_finish).
// The helpers hold no loop of the kernels' own: sub-tile, octet and chunk loops stay in the kernel (a helper with the loop inside is
// simplified before it is inlined and can cost registers: profiles/attn_core_device_code.txt).
#pragma once
#include "mmd_common.h"

// Workgroup id for a grid whose neighbours in id should share an L2: hardware block bid runs on XCD bid & 7, so XCD x gets the
// contiguous id range [start(x), start(x) + blocks on x) of the nwg ids.  (mmd_wgrad.hip's weight-gradient order is another formula.)
__device__ __forceinline__ int xcd_block_id(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// eight consecutive floats of a bias row (LDS or global memory, 16-byte aligned), read ahead of the pairing where the kernel wants them
struct Octet { f32x4 lo, hi; };
__device__ __forceinline__ Octet load_octet(const float* t8) { return Octet{*(const f32x4*)t8, *(const f32x4*)(t8 + 4)}; }
// v[0 .. 8) = channels 16 j2 + 8 half .. + 8 of row l31 from the sub-tile's accumulator (no bias: the callers differ in what they add)
__device__ __forceinline__ void acc_octet(f32x16 acc, int j2, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[8 * j2 + j]), __float_as_uint(acc[8 * j2 + 4 + j]), false, false);
    v[j] = __uint_as_float(sw[0]);
    v[4 + j] = __uint_as_float(sw[1]);
  }
}
// the same with the bias added inside the pairing (one expression per swap: the form of res_tail's skip product).
// Why the swap loop is written twice: the statement order the compiler sees decides its schedule and register allocation.  With one
// form only (pairing, then octet_add) three rtail_kernel instances took 2 more VGPRs than their private copies had; with each kernel
// in the order it was written in, every instance keeps its counts (profiles/rowwave_epilogue_device_code.txt).  For the same reason the
// bias is read by the caller (load_octet) where its kernel read it, not inside octet_add.
__device__ __forceinline__ void acc_octet(f32x16 acc, int j2, const Octet& b, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[8 * j2 + j]), __float_as_uint(acc[8 * j2 + 4 + j]), false, false);
    v[j] = __uint_as_float(sw[0]) + b.lo[j];
    v[4 + j] = __uint_as_float(sw[1]) + b.hi[j];
  }
}
__device__ __forceinline__ void octet_add(float (&v)[8], const Octet& b) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] += b.lo[j]; v[4 + j] += b.hi[j]; }
}
// step 2 of the fold: the stored octet pk continues the lane's four running sums (u is NOT reset here)
__device__ __forceinline__ void quad_sums(const u32x4& pk, float (&u)[4]) {
  float rf[8];
  Elt<__bf16>::unpack(pk, rf);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u[0] += rf[j];
    u[1] += rf[4 + j];
    u[2] += rf[j] * rf[j];
    u[3] += rf[4 + j] * rf[4 + j];
  }
}
// step 3: lanes 16 / 17 of each half end up with the (sum, sum of squares) of quad 0 / 1 of the lane group's 8 channels
__device__ __forceinline__ bool is_record_lane(int l31) { return (l31 >> 1) == 8; }
__device__ __forceinline__ void quad_fold(const float (&u)[4], int l31, float& msum, float& msq) {
  const float t0 = halfwave_total(u[0]), t1 = halfwave_total(u[1]), t2 = halfwave_total(u[2]), t3 = halfwave_total(u[3]);
  msum = (l31 & 1) ? t1 : t0;
  msq = (l31 & 1) ? t3 : t2;
}
// where a record lane writes: record rec, the quad of column col (the lane group's first of 8 channels) + the lane's quad
__device__ __forceinline__ float* quad_record(float* stats, int64_t rec, int64_t stats_ld, int col, int l31) {
  return stats + (rec * stats_ld + (col >> 2) + (l31 & 1)) * 2;
}
// a record lane's (sum, squares): to the record, or (step 4) to its LDS slot - the kernels index their own slot tables
__device__ __forceinline__ void quad_put(float* slot, float msum, float msq) {
  slot[0] = msum;
  slot[1] = msq;
}
__device__ __forceinline__ void half_record_finish(float* d, const float* own, const float* partner) {
  d[0] = own[0] + partner[0];
  d[1] = own[1] + partner[1];
}

// Byte offset of logical 16-byte chunk 2 c + half inside a lane's 128-byte row of a swizzled weight plane (xsw = (row >> 1) & 7)
__device__ __forceinline__ int swz_frag_off(int c, int half, int xsw) { return ((2 * c + half) ^ xsw) * 16; }

// ----------------------------------------------------------------------------- K-streamed row-wave kernels (mmd_aconv, mmd_res_tail)
// Weight slab of one K step: [CS rows][64 channels] of W [Cout][K] bf16 as the swizzled LDS image, by global_load_lds.  Piece
// ih * 4 + wave = 8 rows (1 KB): lane (lrow = lane >> 3, pc = lane & 7) fetches the 16 bytes that land at chunk pc of its row, i.e.
// logical chunk pc ^ ((row >> 1) & 7).  slab_row_ptr: that lane's source at K offset 0; slab_issue: one piece into a plane.
__device__ __forceinline__ const char* slab_row_ptr(const char* W, int cbase, int K, int ih, int wave, int lane) {
  const int row = 8 * (ih * 4 + wave) + (lane >> 3);
  const int logical = (lane & 7) ^ ((row >> 1) & 7);
  return W + ((int64_t)(cbase + row) * K + logical * 8) * 2;
}
__device__ __forceinline__ void slab_issue(const char* src, char* plane, int ih, int wave) {
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(plane + (ih * 4 + wave) * 1024), 16, 0, 0);
}
// sAB [2 samples][a | b][K] <- the fused-affine rows of samples s0 and min(s0 + 1, nS - 1): a workgroup's 128 rows touch at most two
__device__ __forceinline__ void load_affine_rows(float* sAB, const float* ga, const float* gb, int s0, int nS, int K, int tid) {
  for (int i = tid; i < 4 * K; i += 256) {
    const int sl = i / (2 * K), ab = (i / K) & 1, c = i % K;
    const int sidx = min(s0 + sl, nS - 1);
    sAB[i] = (ab ? gb : ga)[(int64_t)sidx * K + c];
  }
}
// act(x * a + b) of a B-operand octet, rounded to bf16 where gn_apply stores the normalised tensor
__device__ __forceinline__ u32x4 affine_act_octet(u32x4 xin, const float* ap, const float* bp, int act) {
  float x[8];
  Elt<__bf16>::unpack(xin, x);
#pragma unroll
  for (int e = 0; e < 8; e += 4) {
    const f32x4 av = *(const f32x4*)(ap + e), bv = *(const f32x4*)(bp + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float y = x[e + k] * av[k] + bv[k];
      x[e + k] = act ? silu_f(y) : y;
    }
  }
  return Elt<__bf16>::pack(x);
}
