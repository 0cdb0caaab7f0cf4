// Counter-based noise: one definition for mmd_diffusion.hip (DDPM / DDIM updates, cond_replace, renoise, ctr_fill) and mmd_dpm.hip (SDE step).
// N(0,1) values that are a pure function of (seed, sample id, draw, stream tag, element): Philox4x32-10 (Salmon et al., SC'11) keyed
// with the 64-bit seed (low word first) on the counter
//   c0 = r >> 2   r = the element's index inside its sample in API layout     c1 = draw (the loop index t[n]; 0xFFFFFFFF = x_T)
//                 resampled loops (mmd_ddpm_update_ctr_at, mmd_renoise_ctr) hand the draw in: visit r of step i of T draws i + r T (< 2^31),
//                 the k-th forward jump 0x80000000 + k; the stochastic solver step (mmd_dpmpp_sde_update_ctr) draws at its evaluation number k[n]
//   c2 = sample id (low 32 bits of ids[n]; the host refuses ids outside [0, 2^32))   c3 = tag (0 video, 1 audio, 2 SR image, 3 shifts)
// The four output words belong to elements 4 c0 ... 4 c0 + 3; words past the end of a sample are dropped.  Nothing in the counter
// depends on the batch position, the batch size, the lane or the rank.  Word w -> u = ((w >> 9) + 0.5) 2^-23, exact in fp32 and inside
// (0, 1); words (0, 1) and (2, 3) each feed one Box-Muller pair z = sqrt(-2 ln u_a) (cos, sin)(2 pi u_b) through the precise logf /
// sqrtf and sincospif(2 u_b), whose argument reduction is exact.  u >= 2^-24, so |z| <= sqrt(2 * 24 ln 2) = 5.77.
// One evaluation costs 20 32-bit multiply pairs (low + high half) for four outputs, next to 16 bytes per element of memory traffic.
#pragma once
#include "mmd_common.h"

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* w) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
struct CtrKey { const uint32_t* key; const int64_t* ids; int tag; };
// the words of the quad that starts at element r0 (a multiple of 4) of sample n
__device__ __forceinline__ void ctr_words(const CtrKey& k, int64_t n, int64_t r0, uint32_t draw, uint32_t* w) {
  philox4x32_10((uint32_t)(r0 >> 2), draw, (uint32_t)k.ids[n], (uint32_t)k.tag, k.key[0], k.key[1], w);
}
__device__ __forceinline__ float ctr_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }
__device__ __forceinline__ void ctr_box_muller(uint32_t wa, uint32_t wb, float* z) {
  const float rho = sqrtf(-2.f * logf(ctr_uniform(wa)));
  float s, c;
  sincospif(2.f * ctr_uniform(wb), &s, &c);
  z[0] = rho * c;
  z[1] = rho * s;
}
__device__ __forceinline__ void ctr_normals(const CtrKey& k, int64_t n, int64_t r0, uint32_t draw, float* z) {
  uint32_t w[4];
  ctr_words(k, n, r0, draw, w);
  ctr_box_muller(w[0], w[1], z);
  ctr_box_muller(w[2], w[3], z + 2);
}

static inline bool ctr_args_ok(const uint32_t* key, const int64_t* ids, int tag) { return key && ids && tag >= 0 && tag <= 3; }
