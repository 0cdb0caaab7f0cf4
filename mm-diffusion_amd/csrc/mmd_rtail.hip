// The tail of a channel-changing ResBlock in ONE launch: the out conv of the normalised h and the 1x1 skip conv of x, K streamed.
//
//   reference: out_layers = normalization, SiLU, Dropout, zero_module(conv 1x1); skip_connection = conv 1x1 (unet:347-375);
//              return skip_connection(x) + out_layers(h) (unet:494-495)
//   y[m, :] = bf16( (W . act(h[m, :] * a[s] + b[s]) + bias) + float(bf16(W2 . x[m, :] + bias2)) )
//
// The row-strip kernel does this for K1 + K2 <= 512 (mmd_gn_conv1x1_skip: both operands register-stationary, 128 operand registers).
// The deeper levels (256 - 512 channels into the out conv, up to 1024 into the skip conv) ran two launches: conv_gemm(x, W2) -> sk, then
// the out conv with R = sk - the skip tensor written to HBM and read straight back.  Here the mapping is mmd_aconv's instead:
//   * a workgroup of four waves covers 128 rows x CS = 64 / 128 columns; a wave owns 32 rows and TWO accumulator sets of its column
//     range (one per product) for the whole K loop;
//   * K is streamed in 64-channel steps (128-channel steps in the launches of few workgroups, whose time is the latency of a step's
//     loads): first the steps of (x, W2) into the second set, then the steps of (h, W) into the first.  The wave loads its rows of the
//     step straight from global memory into MFMA B-operand fragments one step ahead; h gets the fused affine + SiLU in registers
//     (affine rows of the at most two samples of a workgroup in LDS) and is rounded to bf16 where gn_apply rounds; the step's weight
//     slab [CS][64] goes through a two-stage LDS ring (global_load_lds, the strip kernel's swizzled image);
//   * the row-wave epilogue (mmd_rowwave.h) in the form of the strip kernel's two-operand instance: the skip product gets its bias and
//     its bf16 rounding, then it is added where the residual is added.
// Within each accumulator K runs in ascending 16-channel MFMA steps, so Y is bitwise the two launches'.  The statistics records are
// folded in the order of the out conv the layer runs today (mmd_gemm.hip: dispatch_conv1x1_strip), which has two (steps 2 and 4 of the
// fold order in mmd_rowwave.h):
//   one fragment  (K1 >= 384, and K1 = 128 with the norm fused and samples of >= 16384 rows): a wave folds its 32 rows, then even wave
//                 + odd wave through LDS;
//   two fragments (K1 = 256, K1 = 128 otherwise): rows r and r + 32 of a record are one lane's running sums in that kernel.  Here
//                 they belong to the same lane of the even and the odd wave of a pair: the odd wave hands its stored values over
//                 through LDS (the weight ring is free by then) and the even wave continues its running sums with them.
// A null affine (ga == gb == nullptr) means h is already normalised: the launch then runs behind gn_apply.
#include "mmd_rowwave.h"
#include <type_traits>

struct RTailParams {
  const char* H; int64_t ldh;          // [M, K1]
  const char* X; int64_t ldx;          // [M, K2]
  const char* W;                       // [Cout][K1] bf16 (pack_conv_weight layout)
  const char* W2;                      // [Cout][K2]
  const float* bias; const float* bias2;
  const float* ga; const float* gb;    // [S][K1] fused GroupNorm(+FiLM) affine per sample (GN instances)
  char* Y; int64_t ldy;
  float* stats; int64_t stats_ld;      // optional quad records of Y
  int M, L, K1, K2, Cout, act;
  int pair;                            // record fold: 0 one fragment, 1 two fragments (head of this file)
};

// CSUB: 32-column sub-tiles per workgroup (2 / 4); GN: normalise h in registers; KB: 64-channel planes per K step
template <int CSUB, bool GN, int KB>
__global__ __launch_bounds__(256, 2) void rtail_kernel(const RTailParams p, const int nsplit) {
  constexpr int CS = 32 * CSUB;
  constexpr int PLANE_B = CS * 128;    // one plane of a weight slab: CS rows x 64 channels
  constexpr int STAGE_B = KB * PLANE_B;
  constexpr int NCG = 4 * KB;          // 16-channel MFMA steps per K step
  constexpr int GP = CS / 32;          // weight DMA instructions per wave and plane (8 rows each)
  static_assert(2 * STAGE_B >= 2 * CSUB * 2 * 64 * 16, "the two-fragment fold parks two waves' stored values in the weight ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sW = smem;                                         // [2 stages][KB planes][CS rows][128 B], 16-byte chunks XOR-swizzled by (row >> 1) & 7
  float* sBias = (float*)(smem + 2 * STAGE_B);             // [CS] bias of the out conv
  float* sBias2 = sBias + CS;                              // [CS] bias of the skip conv (its own row: the two products are rounded apart)
  float* sRec = sBias2 + CS;                               // [4 waves][CSUB * 2][2 halves][2 quads][2] half-record statistics
  float* sAB = sRec + 4 * CSUB * 2 * 2 * 2 * 2;            // [2 samples][a | b][K1]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  // the nsplit workgroups of one row block get consecutive ids inside one XCD's contiguous range: they share the block's rows in that L2
  const int wgid = xcd_block_id(blockIdx.x, gridDim.x);
  const int sp = wgid % nsplit, mt = wgid / nsplit;
  const int cbase = sp * CS, m0 = mt * 128;
  const int n2 = p.K2 / (64 * KB), nsteps = n2 + p.K1 / (64 * KB);

  const char *w_ptr[GP], *w2_ptr[GP];
#pragma unroll
  for (int ih = 0; ih < GP; ++ih) {
    w_ptr[ih] = slab_row_ptr(p.W, cbase, p.K1, ih, wave, lane);
    w2_ptr[ih] = slab_row_ptr(p.W2, cbase, p.K2, ih, wave, lane);
  }
  auto issue_w = [&](int stage, int s) {                   // step s: channels [64 KB s, + 64 KB) of x (s < n2), then of h (from s = n2)
#pragma unroll
    for (int pl = 0; pl < KB; ++pl)
#pragma unroll
      for (int ih = 0; ih < GP; ++ih) {
        const char* src = s < n2 ? w2_ptr[ih] + (int64_t)(s * KB + pl) * 128 : w_ptr[ih] + (int64_t)((s - n2) * KB + pl) * 128;
        slab_issue(src, sW + stage * STAGE_B + pl * PLANE_B, ih, wave);
      }
  };
  // this lane's row and its sample; the workgroup's rows touch at most two samples (L >= 128); rows past M read row M - 1 once more and
  // store nothing
  const int row = m0 + wave * 32 + l31;
  const bool rok = row < p.M;
  const int rowc = rok ? row : p.M - 1;
  const int s0 = m0 / p.L;
  const int gsel = min(rowc / p.L - s0, 1) * 2 * p.K1;
  auto load_act = [&](int s, u32x4 (&x)[NCG]) {
    const bool second = s < n2;
    const char* base = second ? p.X : p.H;
    const int64_t ld = second ? p.ldx : p.ldh;
    const int ck = second ? s : s - n2;
    const char* ap = base + ((int64_t)rowc * ld + ck * (64 * KB) + half * 8) * 2;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) x[cg] = *(const u32x4*)(ap + cg * 32);
  };

  issue_w(0, 0);
  u32x4 xc[NCG], xn[NCG];
  load_act(0, xc);
  // biases of the column range and the affine rows of the two samples -> LDS
  if (tid < CS) {
    sBias[tid] = p.bias ? p.bias[cbase + tid] : 0.f;
    sBias2[tid] = p.bias2 ? p.bias2[cbase + tid] : 0.f;
  }
  if constexpr (GN) load_affine_rows(sAB, p.ga, p.gb, s0, p.M / p.L, p.K1, tid);
  f32x16 acc[CSUB], acc2[CSUB];                            // out conv | skip conv
#pragma unroll
  for (int a = 0; a < CSUB; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = acc2[a][r] = 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                         // slab 0 landed; bias / affine tables visible

  const int xsw = (l31 >> 1) & 7;
  // one K step into one accumulator set; norm: the step's rows are h and get the fused affine (+ SiLU)
  auto step = [&](int s, auto norm, f32x16 (&ac)[CSUB]) __attribute__((always_inline)) {
    const int st = s & 1;
    if (s + 1 < nsteps) {                                  // next slab and next activations in flight under this step
      issue_w(st ^ 1, s + 1);
      load_act(s + 1, xn);
    }
    if constexpr (decltype(norm)::value) {                 // rounded to bf16 where gn_apply stores the tensor
      const int ck = s - n2;
#pragma unroll
      for (int cg = 0; cg < NCG; ++cg) {
        const float* ap = sAB + gsel + ck * (64 * KB) + cg * 16 + half * 8;
        xc[cg] = affine_act_octet(xc[cg], ap, ap + p.K1, p.act);
      }
    }
    const char* bW = sW + st * STAGE_B + l31 * 128;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg)
#pragma unroll
      for (int a = 0; a < CSUB; ++a) {
        const u32x4 fw = *(const u32x4*)(bW + (cg >> 2) * PLANE_B + a * 32 * 128 + swz_frag_off(cg & 3, half, xsw));
        ac[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fw), __builtin_bit_cast(bf16x8, xc[cg]), ac[a], 0, 0, 0);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                       // next slab landed; every wave is past its reads of this stage
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) xc[cg] = xn[cg];
  };
  int s = 0;
  for (; s < n2; ++s) step(s, std::false_type{}, acc2);
  for (; s < nsteps; ++s) step(s, std::integral_constant<bool, GN>{}, acc);

  // ---- epilogue (mmd_rowwave.h): this lane's octets are the channels 32 a + 16 j2 + 8 half .. + 8 of its row
  const bool wave_ok = (int64_t)m0 + wave * 32 < p.M;      // wave-uniform (M % 64 == 0 when statistics are on: wave pairs are whole records)
  const int64_t rec = ((int64_t)m0 + wave * 32) / 64;
  u32x4* sPk = (u32x4*)sW;                                 // two-fragment fold: [2 odd waves][CSUB * 2][64 lanes] stored values (the ring is free)
  float srec[CSUB][2][4];                                  // one fragment: [0 .. 1] the wave's folded half record; two: the lane's four running sums
#pragma unroll
  for (int a = 0; a < CSUB; ++a)
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2) {
      const int cb = a * 32 + 16 * j2 + 8 * half;
      float v[8], sk[8], rf[8];
      const Octet b = load_octet(sBias + cb), c = load_octet(sBias2 + cb);
      acc_octet(acc[a], j2, v);
      octet_add(v, b);
      // + float(bf16(W2 . x + bias2)): the tensor the separate launch stores, then the residual add
      acc_octet(acc2[a], j2, c, sk);
      Elt<__bf16>::unpack(Elt<__bf16>::pack(sk), rf);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += rf[j];
      const u32x4 pk = Elt<__bf16>::pack(v);
      if (rok) *(u32x4*)(p.Y + ((int64_t)rowc * p.ldy + cbase + cb) * 2) = pk;
      if (p.stats) {
        if (p.pair && (wave & 1)) {                        // (wave-uniform) the even wave sums these values behind its own
          sPk[((wave >> 1) * (CSUB * 2) + a * 2 + j2) * 64 + lane] = pk;
          continue;
        }
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        quad_sums(pk, u);
        if (p.pair) {
#pragma unroll
          for (int k = 0; k < 4; ++k) srec[a][j2][k] = u[k];
          continue;
        }
        quad_fold(u, l31, srec[a][j2][0], srec[a][j2][1]);
        if ((wave & 1) && is_record_lane(l31))             // a wave holds HALF a record (32 rows): the odd wave parks its half
          quad_put(sRec + (((wave * CSUB + a) * 2 + j2) * 2 + half) * 4 + (l31 & 1) * 2, srec[a][j2][0], srec[a][j2][1]);
      }
    }
  if (p.stats) {
    __syncthreads();
    if (wave_ok && (wave & 1) == 0) {                      // the even wave of a pair finishes the record in the layer's fixed order
#pragma unroll
      for (int a = 0; a < CSUB; ++a)
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2) {
          float* d = quad_record(p.stats, rec, p.stats_ld, cbase + a * 32 + 16 * j2 + 8 * half, l31);
          if (p.pair) {                                    // own row's running sums, continued with row + 32, then the fold over the rows
            float u[4], m[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) u[k] = srec[a][j2][k];
            quad_sums(sPk[((wave >> 1) * (CSUB * 2) + a * 2 + j2) * 64 + lane], u);
            quad_fold(u, l31, m[0], m[1]);
            if (is_record_lane(l31)) quad_put(d, m[0], m[1]);
          } else if (is_record_lane(l31)) {                // own half + partner's half
            half_record_finish(d, srec[a][j2], sRec + ((((wave + 1) * CSUB + a) * 2 + j2) * 2 + half) * 4 + (l31 & 1) * 2);
          }
        }
    }
  }
}

template <int CSUB, bool GN, int KB>
static int launch_rtail(const RTailParams& p, hipStream_t st) {
  constexpr int CS = 32 * CSUB;
  const int rowblocks = cdiv(p.M, 128), nsplit = p.Cout / CS;
  constexpr size_t FIXED = 2 * (size_t)KB * CS * 128 + 2 * (size_t)CS * 4 + 4 * CSUB * 2 * 2 * 2 * 2 * 4;      // ring | two bias rows | records
  const size_t lds = FIXED + (GN ? 4 * (size_t)p.K1 * 4 : 0);
  const size_t lds_max = FIXED + 4 * (size_t)512 * 4;
  return mmd_launch_cap<rtail_kernel<CSUB, GN, KB>>("res_tail", dim3(rowblocks * nsplit), dim3(256), lds, lds_max, st, p, nsplit);
}

template <bool GN>
static int dispatch_rtail(RTailParams& p, hipStream_t st) {
  // the record fold of the out conv this layer runs today (mmd_gemm.hip: dispatch_conv1x1_strip): two row fragments per wave at
  // K1 <= 256, except K1 = 128 with the norm fused and samples of >= 16384 rows.  By the layer's rows per SAMPLE: never by the batch size
  p.pair = p.K1 == 256 || (p.K1 == 128 && (!GN || p.L < 16384));
  // 128 columns per workgroup (each weight fragment feeds more MFMAs, the rows are re-read and the normalisation redone for half as
  // many column ranges) from 192 workgroups on: measured ahead at 192 - 1024 workgroups, 3 - 8 us behind the 64-column instance below
  // at 128 and fewer (profiles/restail_ab.txt).  Results do not depend on it
  if (p.Cout % 128 == 0 && (int64_t)cdiv(p.M, 128) * (p.Cout / 128) >= 192) return launch_rtail<4, GN, 1>(p, st);
  // the launches of few workgroups are bound by the latency of a step's loads (one step ahead, then vmcnt(0) + barrier): 128 channels
  // per step halve the number of exposed round trips (same 32 KB ring: 64 columns x 2 planes).  The MFMA order inside an accumulator
  // is still ascending k: results do not depend on it either
  if (p.K1 % 128 == 0 && p.K2 % 128 == 0) return launch_rtail<2, GN, 2>(p, st);
  return launch_rtail<2, GN, 1>(p, st);
}

// ResBlock out conv + 1x1 skip conv on channels-last bf16 rows of S = M / L whole samples, K streamed (see the head of this file).
// h [M, ldh] (K1 columns), x [M, ldx] (K2 columns), W [Cout][K1], W2 [Cout][K2] (mmd_conv_gemm's weight layout), ga / gb [S, K1] = the
// fused affine of mmd_gn_finalize_stats / mmd_gn_stats or both null (h already normalised), Y [M, ldy]; stats (optional): quad records
// of Y as the layer's out conv writes them today (M % 64 == 0).  No fallback: shapes outside K1 in {128, 256, 384, 512}, K2 % 64 == 0
// (<= 1024), Cout % 64 == 0, L >= 128 are refused.
extern "C" int mmd_res_tail(const void* h, int64_t ldh, const float* ga, const float* gb, int act, const void* W, const float* bias,
                            const void* x, int64_t ldx, const void* W2, const float* bias2, void* Y, int64_t ldy, int M, int L, int K1,
                            int K2, int Cout, float* stats, int64_t stats_ld, void* stream) {
  MMD_REQUIRE(h && x && W && W2 && Y, "res_tail: null pointer");
  MMD_REQUIRE((ga == nullptr) == (gb == nullptr), "res_tail: the fused affine needs both ga and gb (or neither: h is already normalised)");
  MMD_REQUIRE(M > 0 && L >= 128 && M % L == 0, "res_tail: M = %d rows must be whole samples of L = %d >= 128 rows", M, L);
  MMD_REQUIRE(K1 == 128 || K1 == 256 || K1 == 384 || K1 == 512, "res_tail: K1 = %d must be 128, 256, 384 or 512", K1);
  MMD_REQUIRE(K2 >= 64 && K2 % 64 == 0 && K2 <= 1024, "res_tail: K2 = %d must be a multiple of 64 up to 1024", K2);
  MMD_REQUIRE(Cout > 0 && Cout % 64 == 0, "res_tail: Cout = %d must be a multiple of 64", Cout);
  MMD_REQUIRE(ldh >= K1 && ldx >= K2 && ldy >= Cout && ldh % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 &&
                  ((uintptr_t)h | (uintptr_t)x | (uintptr_t)W | (uintptr_t)W2 | (uintptr_t)Y) % 16 == 0,
              "res_tail: rows must be 16-byte aligned");
  MMD_REQUIRE(!stats || (M % 64 == 0 && stats_ld >= Cout / 4 && (uintptr_t)stats % 8 == 0),
              "res_tail: statistics need M %% 64 == 0 and a record row of >= Cout / 4 quads");
  const char *y0 = (const char*)Y, *y1 = y0 + ((int64_t)(M - 1) * ldy + Cout) * 2;
  const char *h0 = (const char*)h, *h1 = h0 + ((int64_t)(M - 1) * ldh + K1) * 2, *x0 = (const char*)x, *x1 = x0 + ((int64_t)(M - 1) * ldx + K2) * 2;
  MMD_REQUIRE((h1 <= y0 || y1 <= h0) && (x1 <= y0 || y1 <= x0), "res_tail: h / x and Y overlap (the column ranges of a row block read rows the others write)");
  RTailParams p;
  p.H = h0; p.ldh = ldh; p.X = x0; p.ldx = ldx; p.W = (const char*)W; p.W2 = (const char*)W2; p.bias = bias; p.bias2 = bias2;
  p.ga = ga; p.gb = gb; p.Y = (char*)Y; p.ldy = ldy; p.stats = stats; p.stats_ld = stats_ld;
  p.M = M; p.L = L; p.K1 = K1; p.K2 = K2; p.Cout = Cout; p.act = act; p.pair = 0;
  return ga ? dispatch_rtail<true>(p, (hipStream_t)stream) : dispatch_rtail<false>(p, (hipStream_t)stream);
}
