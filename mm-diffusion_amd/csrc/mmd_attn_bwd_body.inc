// The two kernels of mmd_attn_bwd (mmd_attn_bwd.hip), included once per tile size: AB_DQ / AB_DKV name the kernels, AB_TM is the
// rows and columns of the score tile per thread (R = 16 * AB_TM rows per LDS tile), AB_NC the head-width columns per thread (x 16).
template <typename T>
__global__ __launch_bounds__(256) void AB_DQ(const AttnBwdParams p) {
  constexpr int TM = AB_TM, NC = AB_NC;
  constexpr int R = 16 * TM, R1 = R + 1, RSH = TM == 4 ? 6 : 5, PSH = 8 - RSH, PARTS = 256 / R, KP = R / PARTS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ch = p.ch, LQ = ch + 1;
  float* sQ = (float*)smem;            // [R][LQ] scaled q
  float* sdO = sQ + R * LQ;           // [R][LQ]
  float* sK = sdO + R * LQ;           // [R][LQ]
  float* sV = sK + R * LQ;            // [R][LQ]
  float* sS = sV + R * LQ;            // [R][R+1]
  float* sM = sS + R * R1;            // [R]
  float* sL = sM + R;                 // [R]
  float* sD = sL + R;                 // [R]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int h = blockIdx.y;
  const int b = blockIdx.z / p.G, g = blockIdx.z % p.G;
  const int qcount = ab_qcount(p, g);
  const int q0 = blockIdx.x * R;
  if (q0 >= qcount) return;
  const int64_t qb = ab_qbase(p, b), kb = ab_kbase(p, b);
  const int kstart = ab_kstart(p, g), kcount = p.win * p.k_per_group;
  auto qrow = [&](int i) { return qb + (int64_t)(g * p.q_per_group + q0 + i) * p.q_tstride; };
  auto krow = [&](int j) { int r = kstart + j; if (r >= p.k_mod) r -= p.k_mod; return kb + (int64_t)r * p.k_tstride; };

  for (int i = tid; i < R * ch; i += 256) {
    const int r = i / ch, d = i % ch;
    float q = 0.f, go = 0.f;
    if (q0 + r < qcount) {
      q = Elt<T>::ld(p.Q, qrow(r) * p.ldq + p.q_off + h * ch + d) * p.scale;
      go = Elt<T>::ld(p.dO, qrow(r) * p.lddo + h * ch + d);
    }
    sQ[r * LQ + d] = q;
    sdO[r * LQ + d] = go;
  }
  if (tid < R) { sM[tid] = -1e30f; sL[tid] = 0.f; }
  __syncthreads();
  {   // D_i = dO_i . O_i   (PARTS threads per row)
    const int r = tid >> PSH, part = tid & (PARTS - 1);
    float acc = 0.f;
    if (q0 + r < qcount)
      for (int d = part; d < ch; d += PARTS) acc += sdO[r * LQ + d] * Elt<T>::ld(p.O, qrow(r) * p.ldo + h * ch + d);
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (PARTS == 8) acc += __shfl_xor(acc, 4, 64);
    if (part == 0) sD[r] = acc;
  }
  const int ntiles = (kcount + R - 1) >> RSH;
  // ---- pass 1: running max / sum per query row
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    for (int i = tid; i < R * ch; i += 256) {
      const int r = i / ch, d = i % ch;
      sK[r * LQ + d] = (t * R + r < kcount) ? Elt<T>::ld(p.KV, krow(t * R + r) * p.ldkv + p.k_off + h * ch + d) : 0.f;
    }
    __syncthreads();
    float s[TM][TM];
    tile_dot<TM>(sQ, sK, LQ, ch, ty, tx, s);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int c = 0; c < TM; ++c) sS[(ty * TM + a) * R1 + tx * TM + c] = (t * R + tx * TM + c < kcount) ? s[a][c] : -1e30f;
    __syncthreads();
    const int r = tid >> PSH, part = tid & (PARTS - 1);
    float mx = -1e30f;
    for (int k = part * KP; k < part * KP + KP; ++k) mx = fmaxf(mx, sS[r * R1 + k]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    if (PARTS == 8) mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
    const float m_old = sM[r], m_new = fmaxf(m_old, mx);
    float sum = 0.f;
    for (int k = part * KP; k < part * KP + KP; ++k) sum += __expf(sS[r * R1 + k] - m_new);
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    if (PARTS == 8) sum += __shfl_xor(sum, 4, 64);
    __syncthreads();
    if (part == 0) { sL[r] = sL[r] * __expf(m_old - m_new) + sum; sM[r] = m_new; }
  }
  __syncthreads();
  if (tid < R) {
    const float l = sM[tid] + logf(sL[tid]);
    sM[tid] = l;                                        // sM now holds the log-sum-exp
    if (q0 + tid < qcount) {
      const int64_t qr = qrow(tid);
      p.lse[qr * p.heads + h] = l;
      p.dsum[qr * p.heads + h] = sD[tid];
    }
  }
  // ---- pass 2: dQ
  float dq[TM][NC];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int c = 0; c < NC; ++c) dq[a][c] = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    for (int i = tid; i < R * ch; i += 256) {
      const int r = i / ch, d = i % ch;
      float kv = 0.f, vv = 0.f;
      if (t * R + r < kcount) {
        const int64_t row = krow(t * R + r);
        kv = Elt<T>::ld(p.KV, row * p.ldkv + p.k_off + h * ch + d);
        vv = Elt<T>::ld(p.KV, row * p.ldkv + p.v_off + h * ch + d);
      }
      sK[r * LQ + d] = kv;
      sV[r * LQ + d] = vv;
    }
    __syncthreads();
    float s[TM][TM], dp[TM][TM];
    tile_dot<TM>(sQ, sK, LQ, ch, ty, tx, s);
    tile_dot<TM>(sdO, sV, LQ, ch, ty, tx, dp);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int c = 0; c < TM; ++c) {
        const int r = ty * TM + a;
        const bool ok = t * R + tx * TM + c < kcount;
        const float pr = ok ? __expf(s[a][c] - sM[r]) : 0.f;
        sS[r * R1 + tx * TM + c] = pr * (dp[a][c] - sD[r]);
      }
    __syncthreads();
    for (int k = 0; k < R; ++k) {
      float ds[TM];
#pragma unroll
      for (int a = 0; a < TM; ++a) ds[a] = sS[(ty * TM + a) * R1 + k];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d = tx + 16 * c;
        if (d < ch) {
          const float kv = sK[k * LQ + d];
#pragma unroll
          for (int a = 0; a < TM; ++a) dq[a][c] += ds[a] * kv;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int r = ty * TM + a;
    if (q0 + r < qcount) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d = tx + 16 * c;
        if (d < ch) Elt<T>::st(p.dQ, qrow(r) * p.lddq + p.dq_off + h * ch + d, dq[a][c] * p.scale);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void AB_DKV(const AttnBwdParams p) {
  constexpr int TM = AB_TM, NC = AB_NC;
  constexpr int R = 16 * TM, R1 = R + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ch = p.ch, LQ = ch + 1;
  float* sQ = (float*)smem;            // [R][LQ] scaled q
  float* sdO = sQ + R * LQ;
  float* sK = sdO + R * LQ;
  float* sV = sK + R * LQ;
  float* sS = sV + R * LQ;            // [R q][R+1]
  float* sLse = sS + R * R1;          // [R]
  float* sD = sLse + R;               // [R]
  int* sFlag = (int*)(sD + R);
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int h = blockIdx.y, b = blockIdx.z;
  const int k0 = blockIdx.x * R;      // key index (within [0, k_mod)) of this tile
  if (k0 >= p.k_mod) return;
  const int64_t qb = ab_qbase(p, b), kb = ab_kbase(p, b);
  const int kcount = p.win * p.k_per_group;

  for (int i = tid; i < R * ch; i += 256) {
    const int r = i / ch, d = i % ch;
    float kv = 0.f, vv = 0.f;
    if (k0 + r < p.k_mod) {
      const int64_t row = kb + (int64_t)(k0 + r) * p.k_tstride;
      kv = Elt<T>::ld(p.KV, row * p.ldkv + p.k_off + h * ch + d);
      vv = Elt<T>::ld(p.KV, row * p.ldkv + p.v_off + h * ch + d);
    }
    sK[r * LQ + d] = kv;
    sV[r * LQ + d] = vv;
  }
  float dk[TM][NC], dv[TM][NC];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int c = 0; c < NC; ++c) dk[a][c] = dv[a][c] = 0.f;

  for (int g = 0; g < p.G; ++g) {
    const int kstart = ab_kstart(p, g);
    // does any key of this tile fall into the window [kstart, kstart + kcount) on the circle?
    __syncthreads();
    if (tid == 0) *sFlag = 0;
    __syncthreads();
    if (tid < R && k0 + tid < p.k_mod) {
      int rel = k0 + tid - kstart;
      if (rel < 0) rel += p.k_mod;
      if (rel < kcount) *sFlag = 1;
    }
    __syncthreads();
    if (*sFlag == 0) continue;
    const int qcount = ab_qcount(p, g);
    for (int q0 = 0; q0 < qcount; q0 += R) {
      __syncthreads();
      for (int i = tid; i < R * ch; i += 256) {
        const int r = i / ch, d = i % ch;
        float q = 0.f, go = 0.f;
        if (q0 + r < qcount) {
          const int64_t row = qb + (int64_t)(g * p.q_per_group + q0 + r) * p.q_tstride;
          q = Elt<T>::ld(p.Q, row * p.ldq + p.q_off + h * ch + d) * p.scale;
          go = Elt<T>::ld(p.dO, row * p.lddo + h * ch + d);
        }
        sQ[r * LQ + d] = q;
        sdO[r * LQ + d] = go;
      }
      if (tid < R) {
        float l = 0.f, dd = 0.f;
        if (q0 + tid < qcount) {
          const int64_t row = qb + (int64_t)(g * p.q_per_group + q0 + tid) * p.q_tstride;
          l = p.lse[row * p.heads + h];
          dd = p.dsum[row * p.heads + h];
        }
        sLse[tid] = l;
        sD[tid] = dd;
      }
      __syncthreads();
      float s[TM][TM], dp[TM][TM];
      tile_dot<TM>(sQ, sK, LQ, ch, ty, tx, s);        // rows = queries, cols = keys of this tile
      tile_dot<TM>(sdO, sV, LQ, ch, ty, tx, dp);
      float pr[TM][TM];
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int c = 0; c < TM; ++c) {
          const int r = ty * TM + a, kk = k0 + tx * TM + c;
          int rel = kk - kstart;
          if (rel < 0) rel += p.k_mod;
          const bool ok = (q0 + r < qcount) && kk < p.k_mod && rel < kcount;
          pr[a][c] = ok ? __expf(s[a][c] - sLse[r]) : 0.f;
          sS[r * R1 + tx * TM + c] = pr[a][c];
        }
      __syncthreads();
      // dV[k][d] += sum_q P[q][k] dO[q][d]   (thread: keys ty*TM+a, d = tx + 16c)
      for (int q = 0; q < R; ++q) {
        float pv[TM];
#pragma unroll
        for (int a = 0; a < TM; ++a) pv[a] = sS[q * R1 + ty * TM + a];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d = tx + 16 * c;
          if (d < ch) {
            const float go = sdO[q * LQ + d];
#pragma unroll
            for (int a = 0; a < TM; ++a) dv[a][c] += pv[a] * go;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int c = 0; c < TM; ++c) {
          const int r = ty * TM + a;
          sS[r * R1 + tx * TM + c] = pr[a][c] * (dp[a][c] - sD[r]);
        }
      __syncthreads();
      // dK[k][d] += sum_q dS[q][k] (scale q)[q][d]
      for (int q = 0; q < R; ++q) {
        float ds[TM];
#pragma unroll
        for (int a = 0; a < TM; ++a) ds[a] = sS[q * R1 + ty * TM + a];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d = tx + 16 * c;
          if (d < ch) {
            const float qv = sQ[q * LQ + d];
#pragma unroll
            for (int a = 0; a < TM; ++a) dk[a][c] += ds[a] * qv;
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int r = ty * TM + a;
    if (k0 + r < p.k_mod) {
      const int64_t row = kb + (int64_t)(k0 + r) * p.k_tstride;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d = tx + 16 * c;
        if (d < ch) {
          Elt<T>::st(p.dKV, row * p.lddkv + p.dk_off + h * ch + d, dk[a][c]);
          Elt<T>::st(p.dKV, row * p.lddkv + p.dv_off + h * ch + d, dv[a][c]);
        }
      }
    }
  }
}
