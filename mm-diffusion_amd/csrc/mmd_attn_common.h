// What the bf16 MFMA attention kernels share (mmd_attn.hip: attn_mfma / attn_dma / attn_pipe / attn_stage_kernel; mmd_attn_bwd_mfma.hip).
//
// All of them use one register layout: S^T = K Q^T on v_mfma_f32_32x32x16_bf16 with keys = D rows and queries = D cols, so a lane owns
// ONE query (lane & 31; the partner lane ^ 32 holds the other half of the keys), a 64-key tile of S^T sits in two f32x16 registers
// (register r of sub-tile kt <-> key 32 kt + (r & 3) + 8 (r >> 2) + 4 half), and P goes from those registers straight into the B
// operand of O^T += V^T P^T (k-slot j of step st <-> register 8 st + j).  Everything that layout dictates is written once, here; a
// kernel keeps its staging, its barriers / waits and the order of its statements.
#pragma once
#include "mmd_common.h"

#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0)
#define TSTRIDE 136     // bytes per row of a transposed [D][64 keys] tile (64 * 2 B + 8): (stride/8) odd -> conflict-free ds_read_b64

// ============================================================================= window geometry and block order
struct GroupInfo {
  int64_t q_row0, k_row0;
  int q_count, k_count, k_start;
  int k_mod;
};

// P: AttnParams / AttnBwdMParams (G, q_rows_per_batch, q_per_group, k_rows_per_batch, k_per_group, win, shift_ptr)
template <typename P>
__device__ __forceinline__ GroupInfo group_info(const P& p, int n, int g) {
  GroupInfo gi;
  gi.q_row0 = (int64_t)n * p.q_rows_per_batch + (int64_t)g * p.q_per_group;
  gi.q_count = (g == p.G - 1) ? (int)(p.q_rows_per_batch - (int64_t)g * p.q_per_group) : p.q_per_group;
  gi.k_row0 = (int64_t)n * p.k_rows_per_batch;
  gi.k_mod = (int)p.k_rows_per_batch;
  gi.k_count = p.win * p.k_per_group;
  const int shift = p.shift_ptr ? *p.shift_ptr : 0;
  gi.k_start = (int)(((int64_t)(g + shift) * p.k_per_group) % gi.k_mod);
  return gi;
}
template <typename P>
__device__ __forceinline__ GroupInfo group_info(const P& p, int bg) {
  return group_info(p, bg / p.G, bg % p.G);
}
// XCD-aware block remap.  Workgroups are dealt round-robin to the 8 XCDs by flat id, and blockIdx.x (the query / key tile) is
// the fastest index: by default the tiles of one (head, group) land on 8 DIFFERENT XCDs and each private L2 fetches the same
// K / V window (forward, dQ) or Q / dO rows (dK, dV) from HBM again.  Remap so all tiles of a (head, group) share flat-id mod 8
// (same XCD, and adjacent in dispatch order).  Returns (tile, head, batch-group = the blockIdx.z equivalent).
__device__ __forceinline__ void attn_block_coords(int& qt, int& h, int& bg) {
  const int nx = gridDim.x, ny = gridDim.y, nz = gridDim.z;
  const int hz_count = ny * nz;
  int hz;
  if ((hz_count & 7) == 0 && nx > 1) {
    const int f = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
    const int k = f >> 3, r = f & 7;
    qt = k % nx;
    hz = r + 8 * (k / nx);
  } else {
    qt = blockIdx.x;
    hz = blockIdx.y + ny * blockIdx.z;
  }
  h = hz % ny;
  bg = hz / ny;
}

__device__ __forceinline__ int64_t key_row(const GroupInfo& gi, int kk) {
  int r = gi.k_start + kk;
  if (r >= gi.k_mod) r -= gi.k_mod;
  return gi.k_row0 + r;
}

// max / sum over the two lanes (l, l ^ 32) that share a query: v_permlane32_swap (VALU) instead of ds_bpermute (an LDS round trip
// queued behind the fragment reads).  swap(x, x) leaves {lower-half values, upper-half values} in the two results for every lane.
__device__ __forceinline__ float half_pair_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_pair_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ============================================================================= fragments and accumulators
// Q fragments (B operand of S^T = K Q^T): lane (q = lane & 31, half) holds d = 16 s + 8 half + [0, 8); zero beyond the group
// (one fragment per call and the loop over s in the kernel: unrolled inside a helper, the loads of a wide head end up under ONE
// branch and attn_mfma_kernel<96> / <192> are allocated 6 / 10 more registers)
__device__ __forceinline__ u32x4 q_frag(const char* qp, int s, int half, bool qok) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (qok) v = *(const u32x4*)(qp + (s * 16 + half * 8) * 2);
  return v;
}

// A fragment (8 k-slots) of a transposed, key-permuted [D][64] tile for MFMA step (kt, st): slots j<4 -> cols 32kt+16st+4half+j, j>=4 -> +8
__device__ __forceinline__ u32x4 tr_frag(const char* tr, int row, int kt, int st, int half) {
  const char* vb = tr + row * TSTRIDE + (32 * kt + 16 * st + 4 * half) * 2;
  const u32x2 v0 = *(const u32x2*)(vb);
  const u32x2 v1 = *(const u32x2*)(vb + 16);
  return u32x4{v0[0], v0[1], v1[0], v1[1]};
}

// ============================================================================= online softmax on the 32x32 C layout
// ragged last tile: keys at or beyond k_count never win.  kbase = first key of the tile + 4 half
__device__ __forceinline__ void mask_ragged(f32x16 (&s)[2], int kbase, int k_count) {
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = kbase + 32 * kt + (r & 3) + 8 * (r >> 2);
      s[kt][r] = kk < k_count ? s[kt][r] : -3e38f;
    }
}

// One online-softmax step of a 64-key tile (lane-local row; partner lane ^ 32 holds the other 32 keys): s becomes the UNROUNDED
// exponentials, from which the row sum is taken.  VALU diet: the softmax scale rides in the exp2 fma (sc = scale * log2 e > 0:
// max commutes with the scale), and the O rescale is skipped when no lane's running max moved (alpha == 1 for the whole wave).
//   NCH: independent max / sum chains (1: one sequential chain; 4: chain r & 3 - a single 32-deep chain is latency-bound)
//   SWAP: the pair exchange by v_permlane32_swap (a ds_bpermute drains lgkmcnt - the V fragment reads in flight - first); else __shfl_xor
//   ALWAYS_RESCALE: no branch around the rescale (alpha == 1.0 exactly where the running max did not move)
template <int NCH, bool SWAP, bool ALWAYS_RESCALE, int DT>
__device__ __forceinline__ void softmax_step(f32x16 (&s)[2], f32x16 (&o)[DT], float& m_run, float& l_run, float sc) {
  static_assert(NCH == 1 || NCH == 4, "one chain or four");
  float mxp[NCH], psp[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) { mxp[c] = -3e38f; psp[c] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) mxp[r & (NCH - 1)] = fmaxf(mxp[r & (NCH - 1)], s[kt][r]);
  float mx = mxp[0];
  if constexpr (NCH == 4) mx = fmaxf(fmaxf(mxp[0], mxp[1]), fmaxf(mxp[2], mxp[3]));
  mx = SWAP ? half_pair_max(mx) : fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx * sc);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][r], sc, -m_new));
      s[kt][r] = e;
      psp[r & (NCH - 1)] += e;
    }
  float ps = psp[0];
  if constexpr (NCH == 4) ps = (psp[0] + psp[1]) + (psp[2] + psp[3]);
  ps = SWAP ? half_pair_sum(ps) : ps + __shfl_xor(ps, 32, 64);
  l_run = l_run * alpha + ps;
  if (ALWAYS_RESCALE || __any(m_new != m_run)) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
  }
  m_run = m_new;
}

// P fragment of k-slot group (kt, st), straight from the S^T registers (k-slot j <-> reg 8 st + j): the ONE place where P is
// rounded to bf16
__device__ __forceinline__ bf16x8 p_frag(const f32x16 (&s)[2], int kt, int st) {
  bf16x8 pf;
#pragma unroll
  for (int j = 0; j < 8; ++j) pf[j] = (__bf16)s[kt][8 * st + j];
  return pf;
}

// ============================================================================= DMA-staged K / V tiles (head width 64: one 128-byte LDS row per key)
// K row-major with the GEMMs' swizzle (16-byte chunk ^ (row >> 1) & 7), V row-major with chunk ^ (bit 1 of the row) << 2; both
// [stage][64 keys][128 B].  Wave w stages row groups {w, w + 4} of a tile; lane L of a group covers row 8 g + L / 8, physical chunk L % 8.
typedef __attribute__((address_space(3))) void* lptr_t;
#define ATTN_DMA_OOB 0xfffffff0u     // offset of a key beyond the window: out of the descriptor's range, which lands zeros

struct KvDmaLanes {
  int row_in_tile[2];
  uint32_t kswz[2], vswz[2];         // swizzled byte column of this lane's chunk inside a K / V row
};
__device__ __forceinline__ KvDmaLanes kv_dma_lanes(int wave, int lane) {
  KvDmaLanes dl;
  const int lrow = lane >> 3, pc = lane & 7;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 8 * (wave + 4 * i) + lrow;
    dl.row_in_tile[i] = row;
    dl.kswz[i] = (uint32_t)((pc ^ ((row >> 1) & 7)) * 16);
    dl.vswz[i] = (uint32_t)((pc ^ (((row >> 1) & 1) << 2)) * 16);
  }
  return dl;
}
template <typename P>
__device__ __forceinline__ auto kv_dma_rsrc(const P& p) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p.KV, 0, (int)((int64_t)p.nb * p.k_rows_per_batch * p.ldkv * 2), 0x00020000);
}
// per-lane buffer offset of key kk of the (circular) window at byte column col; ldb = bytes per KV row
__device__ __forceinline__ uint32_t kv_dma_offset(const GroupInfo& gi, int kk, uint32_t ldb, uint32_t col) {
  int r = gi.k_start + kk;
  r = r >= gi.k_mod ? r - gi.k_mod : r;
  const uint32_t rowoff = (uint32_t)(gi.k_row0 + r) * ldb;
  return kk < gi.k_count ? rowoff + col : ATTN_DMA_OOB;
}

// S^T = K Q^T of one swizzled K tile: two 32-key sub-tiles, fragments by ds_read_b128, the first k-step on a zero accumulator
// operand (no 32 v_mov).  kb = tile + (lane & 31) * 128; K row 32 kt + l31, logical chunk 2 st + half; kx = (l31 >> 1) & 7
template <int KST>
__device__ __forceinline__ void s_tile_zero_acc(const char* kb, int half, int kx, const u32x4 (&qf)[KST], f32x16 (&s)[2]) {
  u32x4 kf[KST][2];
#pragma unroll
  for (int st = 0; st < KST; ++st)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) kf[st][kt] = *(const u32x4*)(kb + kt * 32 * 128 + (((2 * st + half) ^ kx) * 16));
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    s[kt] = MFMA_BF16(kf[0][kt], qf[0], z);
  }
#pragma unroll
  for (int st = 1; st < KST; ++st)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) s[kt] = MFMA_BF16(kf[st][kt], qf[st], s[kt]);
}

// V^T fragments of one swizzled row-major V tile by ds_read_b64_tr_b16: lane i of a 16-lane group supplies the 8 bytes
// V[key0 + i / 4][d0 + 4 (i % 4) ..] and receives V[key0 .. key0 + 3][d0 + i].  Group (kt, st, u) of 4 keys, key0 = 32 kt + 16 st + 8 u
// + 4 half; this lane supplies row key0 + (lane & 15) / 4 (vrow0 = 4 half + (lane & 15) / 4), columns dt * 32 + 16 ((lane >> 4) & 1)
// + 4 (lane & 3) (vcolb = their byte column inside a 64-byte d tile: chunk = vcolb / 16 + 4 dt)
template <int DT>
__device__ __forceinline__ void read_vt_frags_tr(const char* vb, int vrow0, int vcolb, bf16x8 (&vf)[2][2][DT]) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  typedef __attribute__((address_space(3))) s16x4* lp4;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        s16x4 lo, hi;
        {
          const int row = 32 * kt + 16 * st + vrow0;
          const int ch = ((vcolb >> 4) + 4 * dt) ^ (((row >> 1) & 1) << 2);
          lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(vb + row * 128 + ch * 16 + (vcolb & 15)));
        }
        {
          const int row = 32 * kt + 16 * st + 8 + vrow0;
          const int ch = ((vcolb >> 4) + 4 * dt) ^ (((row >> 1) & 1) << 2);
          hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(vb + row * 128 + ch * 16 + (vcolb & 15)));
        }
        const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        vf[kt][st][dt] = __builtin_bit_cast(bf16x8, both);
      }
}

// ============================================================================= epilogue: whole head rows through LDS
// Normalise, transpose this wave's 32 query rows through LDS (rows of D * 2 + 16 bytes at smem + wave * 32 rows; written and read
// by this wave only) and store whole D * 2-byte head rows: a lane owns a query ROW, so direct stores would be 8-byte pieces at a
// row stride (64 lines per wave instruction); staged, D / 8 lanes cover one row.  Also the lse2 store (v_log_f32 = log2).  The
// caller has made sure that every wave is past its last read of that LDS.  tq = first query of this wave.
template <int D, typename P>
__device__ __forceinline__ void store_o_rows_via_lds(const P& p, const GroupInfo& gi, char* smem, int wave, int lane, int tq, int h,
                                                     const f32x16 (&o)[D / 32], float m_run, float l_run) {
  constexpr int SO = D * 2 + 16, DV = D / 8;
  const int half = lane >> 5, l31 = lane & 31, qi = tq + l31;
  const float inv = 1.f / l_run;
  if (p.lse2 && half == 0 && qi < gi.q_count) p.lse2[(gi.q_row0 + qi) * p.heads + h] = m_run + __builtin_amdgcn_logf(l_run);
  char* so = smem + (wave * 32) * SO;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int d = dt * 32 + 8 * q4 + 4 * half;
      bf16x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (__bf16)(o[dt][4 * q4 + e] * inv);
      *(bf16x4*)(so + l31 * SO + d * 2) = w;
    }
#pragma unroll
  for (int ps = 0; ps < 32 * DV / 64; ++ps) {
    const int idx = ps * 64 + lane;
    const int row = idx / DV, v = idx % DV;
    if (tq + row < gi.q_count) {
      const u32x4 x = *(const u32x4*)(so + row * SO + v * 16);
      *(u32x4*)(p.O + ((gi.q_row0 + tq + row) * p.ldo + h * D + v * 8) * 2) = x;
    }
  }
}
