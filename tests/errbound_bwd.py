"""Element-wise error bounds for the BACKWARD kernels against float64 references (test infrastructure; plain torch, no import of the
package under test).  The forward half and the notation are in tests/errbound.py: u = 2**-24 (fp32), v = 2**-8 (bf16), every bound
first order in u, `check` admits zero violating elements.  The rule used throughout: a sum of n fp32 terms accumulated in ANY order -
per-thread partials, LDS folds, atomics across row splits, the add onto a zeroed buffer - carries at most (n - 1) u sum|terms|.

conv weight gradient (`wgrad_ref`, `wgrad_bound`; mmd_wgrad.hip: wgrad_kernel<T>, wgrad128_bf16_kernel, wgrad_tr_bf16_kernel)
    dW[co, tap * Cin + ci] = sum_m dY[m, co] X[src(m, tap), ci], the gather of errbound.conv_gather (zero where the tap leaves
    the frame); S = |dY|^T |gather(X)|.  The M products of one element are accumulated on the MFMA in fp32 (mmd_wgrad.hip:119 / :127 /
    :240 / :410), one partial per row split, and the partials meet in fp32 atomics on the buffer the caller zeroed (wg_scatter, :67; wgrad128, :259):
    M + 1 terms with the zero, M roundings.  bf16 x bf16 products are exact in fp32; an fp32 product is rounded once more.
        bf16 inputs: (M + 1) u S        fp32 inputs: (M + 2) u S.
    The output is fp32 in both modes: no store rounding.
    db[c] = sum_m dY[m, c] (colsum_kernel :420-461; in the 128-tiles the (tap 0, ci tile 0) blocks, :213-220 / :390-399): M terms and
    the zero, no products: (M + 1) u Sb, Sb = sum_m |dY|.  `colsum_slices` is the same kernel per sample: (Tn + 1) u Sb.

conv input gradient: no kernel of its own - mmd_conv_gemm on dY with the weight transposed to [Cin, ntaps * Cout] and the taps
    negated (train_ops.ConvFn.backward).  Reference: errbound.conv_rows_ref on exactly those operands BUILT BY THE TEST from the
    torch-layout weight, bound errbound.gemm_bound unchanged; what the test proves is the transposition and the mirroring.

exact-sum inputs (`grid_randn`)
    Values k * 2**-3 with integer |k| <= 7 (3 significand bits, exact in bf16 and fp32).  A product is an integer <= 49 in units
    of 2**-6; a sum of n of them is an integer <= 49 n.  While 49 n < 2**24 every partial sum of every accumulation order is an
    integer below 2**24 units, i.e. exactly representable in fp32: NO rounding happens anywhere and every legal kernel returns the
    same bits, float64 reference cast to fp32.  `exact_sum_ok(n)` asserts 49 n < 2**24 (the deepest n used is 2376: 116 424).

GroupNorm backward (`gn_fwd_ref` with its bounds e_a / e_b / e_mean / e_rstd, `gn_bwd_ref`; mmd_gn_bwd.hip: gn_bwd_reduce / params / apply, :55-180)
    Forward (mmd_norm.hip:39-159, :161-235): per (slice, group) the sums of d = x - pivot and of d^2 (pivot = the group's first
    element of the slice's first row), per-thread in fp32 (:94), then in double; mean = pivot + sum d / cnt, var = sum d^2 / cnt -
    dm^2 and rstd = 1 / sqrt(var + eps) in double, each rounded once to fp32 (:134-135).  With Sd = sum |d|, Sq = sum d^2 over the
    cnt = Tn * cpg elements (d is itself rounded: one more u per term, two more on its square):
        e_mean = (Tn + 2) u Sd / cnt + u |mean|
        e_var  = (Tn + 4) u Sq / cnt + 2 |dm| (Tn + 2) u Sd / cnt
        e_rstd = rstd^3 e_var / 2 + u rstd                                   (d rstd / d var = - rstd^3 / 2)
    a = rstd gamma (1 + scale), b = (beta - mean rstd gamma)(1 + scale) + shift (:147-154, :229-232):
        e_a = |gamma (1 + scale)| e_rstd + 3 u |a|
        e_b = |1 + scale| (|rstd gamma| e_mean + |mean gamma| e_rstd) + 4 u (|beta (1 + scale)| + |mean rstd gamma (1 + scale)| + |shift|)
    The backward TAKES the stored a, b, mean, rstd as inputs, so `gn_bwd_ref` computes in float64 from the STORED x, dy, a, b, mean,
    rstd: its bounds cover the backward's arithmetic alone, and the forward's error is tested separately against the bounds of `gn_fwd_ref`.
        v = x a + b, sg = 1 / (1 + exp(-v)), dv = dy sg (1 + v (1 - sg))  (SiLU; dv = dy without it),  z = (x - mean) rstd
        P[s, c] = sum_rows dv,  Q[s, c] = sum_rows dv z,  g_c = (1 + scale) gamma
        m1 = sum_{c in group} g_c P_c / cnt,  m2 = sum g_c Q_c / cnt
        dx = rstd (g_c dv - m1 - z m2),  dgamma = sum_s (1 + scale) Q,  dbeta = sum_s (1 + scale) P,
        dscale = gamma Q + beta P,  dshift = P.
    Error of dv as the kernels compute it (:84-85 = :174-175, dsilu_f of mmd_common.h), every operation rounded once, v_exp_f32 and v_rcp_f32 accurate to
    1 ulp = 2 u relative, __expf's multiply by log2(e) one more rounding of the argument:
        e_v  = 2 u (|x a| + |b|)
        e_sg = sg ((1 - sg) (e_v + u |v| + 2 u) + 3 u)                       (exp, the add of 1, the reciprocal)
        e_w  = e_sg + u (1 - sg)                                             w = 1 - sg
        e_q  = |v| e_w + w e_v + u |v w| + u |1 + v w|                       q = 1 + v w
        e_r  = sg e_q + |q| e_sg + u |sg q|                                  r = sg q
        e_dv = |dy| e_r + u |dv|
    Sums (:86-87, :94-98 atomics onto the zeroed workspace): Tn terms and the zero; a term of Q carries three more roundings:
        e_P = (Tn + 1) u sum |dv| + sum e_dv,   e_Q = (Tn + 4) u sum |dv z| + sum e_dv |z|
    Parameter stage (:113-137): g_c two roundings, g_c P one, the group sum of cpg terms, the division:
        e_m1 = (sum_c |g_c| e_P + (cpg + 4) u sum_c |g_c P_c|) / cnt,  e_m2 likewise with Q
        e_dgamma = sum_s (|1 + scale| e_Q + 2 u |(1 + scale) Q|) + (S + 1) u sum_s |(1 + scale) Q|      (atomics over the slices, :124)
        e_dscale = |gamma| e_Q + |beta| e_P + 3 u (|gamma Q| + |beta P|),  e_dshift = e_P
    dx in the kernel's own form k1 dv + k2 x + k3 (:164-166, :176), k1 = rstd g_c, k2 = - rstd^2 m2, k3 = rstd (mean rstd m2 - m1):
        e_k1 = 3 u |k1|,  e_k2 = rstd^2 e_m2 + 2 u |k2|,
        e_k3 = rstd (|mean rstd| e_m2 + e_m1) + 4 u rstd (|mean rstd m2| + |m1|)
        e_dx = |k1| e_dv + e_k1 |dv| + e_k2 |x| + e_k3 + 3 u (|k1 dv| + |k2 x| + |k3|)
    k2 x and k3 CANCEL when |mean| is large against 1 / rstd (k2 x + k3 = - rstd m2 z - rstd m1 with |z| ~ 1, the two terms of size
    |mean| rstd^2 |m2| each): the bound grants the rounding of both large terms as the kernel computes them, 3 u (|k2 x| + |k3|), and
    is therefore about |mean| rstd wider than a bound on the cancellation-free form would be.  That is the kernel's choice (two FMAs
    per element instead of a subtraction and two multiplies), granted as computed.
    bf16 output: v (|ref| + e) + e, one round-to-nearest store (Elt<__bf16>::pack).

attention backward (`attn_bwd_ref`, `attn_out_bound`, `attn_bwd_bound_kv`, `attn_bwd_assemble`)
    Per (query set, key set) and head, float64: a = scale q k^T, p = softmax(a), dP = dO V^T, D_i = dO_i . O_i with O the STORED
    forward output (mmd_attn_bwd_mfma.hip: `Dq` of attn_bwd_dq_mfma_kernel, mmd_attn_bwd_body.inc:40-49) or, mode 'small', D_i = sum_j p_ij dP_ij
    (mmd_attn_bwd.hip:247); dS = p (dP - D); dV = p^T dO, dQ = scale dS K, dK = scale dS^T Q.  dK / dV of a key sum over every
    query of every group whose window holds the key: the reference returns per-pair contributions and per-pair error terms that add.
    With A_ij = scale sum_d |q_id k_jd|, AP_ij = sum_d |dO_id v_jd|, R_i = max_j a_ij - min_j a_ij, n keys, T = ceil(n / 32):
      P:   the three kernels recompute p_ij = exp(a_ij - LSE_i).  The MFMA path takes LSE (log2 domain, lse2) from the forward
           (`exp2(fma(s, scale * log2e, -lse2))`, `pr` in both kernels), the VALU kernel from its own first pass (body.inc:52-84), the short
           kernel divides by its own row sum (mmd_attn_bwd.hip:241-247).  LSE carries the forward's row-sum error, the terms of
           errbound.attn_ref:  e_L_i = sum_j p_ij eps_ij + (n + T (2 R_i + 3) + 4) u + 3 u |ln2 lse2_i|  (natural-log units; the
           last term: log2 / logf at 1 ulp, the add, the fp32 store), eps_ij = ((ch + 3) A_ij + 2 R_i + 2) u.  It enters EVERY p_ij
           of the row.  The score (ch products in fp32, the scale constant rounded once), the fma's single rounding of
           |log2 p_ij| and v_exp_f32 at 1 ulp:   eps_P_ij = ((ch + 3) A_ij + |ln p_ij| + 2) u + e_L_i.
           `attn_bwd_ref` also returns the exact lse2 and e_L / ln2, so the test holds the STORED lse2 to that bound first.
      dP:  ch products in fp32: (ch + 1) u AP_ij.   D: ch products: e_D_i = (ch + 1) u sum_d |dO_id O_id|; mode 'small':
           e_D_i = sum_j p_ij ((eps_P_ij + (n + 2) u) |dP_ij| + (ch + 1) u AP_ij).
      dS:  e_dS_ij = p_ij ((eps_P_ij + 2 u) |dP_ij - D_i| + (ch + 1) u AP_ij + e_D_i)
      MFMA path only: P and dS each rounded ONCE to bf16 in front of the second MFMA (mmd_attn_common.h: p_frag):  E_dS = e_dS + v (|dS| + e_dS),
           E_P = p eps_P + v p (1 + eps_P).  The VALU kernels keep both in fp32: E_dS = e_dS, E_P = p eps_P.
      dQ:  n products accumulated in fp32 over the keys, one multiply by scale (itself rounded):
           e_dQ = scale (E_dS |K| + (n + 1) u |dS| |K|) + 3 u scale |dS| |K|
      dK, dV: accumulated over all Nq queries of all groups that see the key:
           e_dK = scale (E_dS^T |Q| + (Nq + 1) u |dS|^T |Q|) + 3 u scale |dS|^T |Q|,   e_dV = E_P^T |dO| + (Nq + 1) u p^T |dO|  (VALU kernels: Nq + 2, the fp32 product p dO is rounded)
      store: fp32 as is, bf16 v (|ref| + e) + e.
    A key in nobody's window has no term at all: its dK and dV are exactly zero in every kernel (the accumulators start at zero).
"""
import math

import torch

import errbound as E
from errbound import U16, U32, _f64

LN2 = math.log(2.0)


# --------------------------------------------------------------------------- conv weight gradient
def wgrad_ref(dy, x, taps, dims):
    """float64 dW [Cout, ntaps * Cin] (K index = tap * Cin + ci, the packed layout), S = |dY|^T |gather(X)|, db [Cout], Sb."""
    dy, x = _f64(dy), _f64(x)
    g = E.conv_gather(x, taps, dims)
    dW = torch.cat([dy.t() @ gx for gx, _ in g], dim=1)
    S = torch.cat([dy.abs().t() @ gx.abs() for gx, _ in g], dim=1)
    return dW, S, dy.sum(0), dy.abs().sum(0)


def wgrad_bound(S, M, in_dtype):
    return (M + (1 if in_dtype == torch.bfloat16 else 2)) * U32 * S


def colsum_bound(Sb, M):
    return (M + 1) * U32 * Sb


def to_torch_layout(dW, Cin, ntaps):
    """[Cout, ntaps * Cin] (tap major) -> [Cout, Cin * ntaps] (the flattened [Cout, Cin, *k] of the parameter)."""
    return dW.reshape(dW.shape[0], ntaps, Cin).permute(0, 2, 1).reshape(dW.shape[0], Cin * ntaps)


def dgrad_operands(w_torch, taps):
    """The operands ConvFn.backward hands to conv_gemm, built from the torch-layout weight [Cout, Cin, ntaps]: wT [Cin, ntaps * Cout]
    with wT[ci, t * Cout + co] = w[co, ci, t], and the negated taps."""
    Cout, Cin, nt = w_torch.shape
    return w_torch.permute(1, 2, 0).reshape(Cin, nt * Cout).contiguous(), [(-a, -b, -c) for a, b, c in taps]


def grid_randn(shape, gen, device="cpu"):
    """Exact-sum inputs: k / 8 with integer k in [-7, 7] (module docstring)."""
    return torch.randint(-7, 8, shape, generator=gen, device=device).float() / 8.0


def exact_sum_ok(nterms):
    assert 49 * nterms < 2 ** 24, nterms
    return True


def _cdiv(a, b):
    return -(-a // b)


def wgrad_plan(M, Cin, Cout, ntaps, bf16):
    """The launcher's arithmetic (mmd_wgrad.hip: mmd_conv_wgrad with wg_split, no MMD_WGRAD_* switch set): (kernel, splits, rows per split, xcd order).
    kernel 'tr' = the 128-tile (wgrad_tr_bf16_kernel, or wgrad128_bf16_kernel with MMD_WGRAD_TR=0: same splits), '64' = wgrad_kernel<T>."""
    if bf16 and Cout >= 64 and Cin >= 64:
        tiles = _cdiv(Cout, 128) * _cdiv(Cin, 128) * ntaps

        def derive(target):
            sp = max(1, min(_cdiv(M, 256), target // max(tiles, 1)))
            rps = _cdiv(_cdiv(M, sp), 64) * 64
            sp, xo = _cdiv(M, rps), 0
            s8 = sp // 8 * 8
            while s8 >= 8:
                r = _cdiv(_cdiv(M, s8), 64) * 64
                if _cdiv(M, r) % 8 == 0:
                    rps, sp, xo = r, _cdiv(M, r), 1
                    break
                s8 -= 8
            return sp, rps, xo
        best = None
        for t in (256, 384, 512, 768, 1024, 1536, 2048):
            sp, rps, xo = derive(t)
            rounds = _cdiv(tiles * (sp // 8), 64) if xo else _cdiv(tiles * sp, 512)
            cost = rounds * (rps + 300) + 40 * sp
            if best is None or cost < best[0]:
                best = (cost, sp, rps, xo)
        return ("tr",) + best[1:]
    tiles = _cdiv(Cout, 64) * _cdiv(Cin, 64) * ntaps
    sp = max(1, min(_cdiv(M, 256), 2048 // max(tiles, 1)))
    rps = _cdiv(_cdiv(M, sp), 64) * 64
    return "64", _cdiv(M, rps), rps, 0


def check_groups(y, ref, bound, group, label, what="", pixels=None):
    """errbound.check, with a histogram of the violations by column // group (tap of a packed dW, head of an attention gradient)."""
    try:
        return E.check(y, ref, bound, pixels, what)
    except AssertionError as e:
        _, _, bad = E.violations(y, ref, bound)
        cols = torch.nonzero(bad)[:, 1].cpu() // group
        raise AssertionError(f"{e}\n  by {label}: {E._hist(cols, int(cols.max()) + 1)}") from None


def wgrad_cases():
    """The launch geometries of the weight-gradient tests: dicts with name, taps, dims, M, chans [(Cin, Cout)], and the split plan the
    bf16 128-tile launcher must take (splits, rows per split, xcd order) - derived here, asserted against `wgrad_plan`:
    sp = min(ceil(M / 256), target / tiles); with tiles <= 54 the larger targets (up to 2048) reach the cap ceil(M / 256), and at these
    sizes the cost (rounds x (rows per split + 300) + 40 x splits, one round of blocks) falls with every further split, so the cap is
    taken: splits = ceil(M / 256), rows per split = ceil(M / splits) rounded up to 64, XCD order when the count is a multiple of 8."""
    T3, TT = E.TAPS_SPATIAL, E.TAPS_TEMPORAL
    C4 = [(64, 96), (192, 264), (128, 128), (256, 72)]
    cases = []

    def add(name, taps, dims, M, chans, plan):
        cases.append(dict(name=name, taps=taps, dims=tuple(dims), M=M, chans=chans, plan=plan))

    # the two smallest frames: 70 rows -> one split of 128; 384 rows -> ceil(384 / 256) = 2 splits of 192, plain order
    add("3x3-2x5x7", T3, (2, 5, 7), 70, C4[:2], (1, 128, 0))
    add("3x3-3x8x16", T3, (3, 8, 16), 384, C4[2:], (2, 192, 0))
    # M = 1050: ceil(1050 / 256) = 5 splits of ceil(210 / 64) * 64 = 256 rows, no multiple of 8: plain order; the last split has 26 rows
    add("3x3-2x21x25", T3, (2, 21, 25), 1050, C4, (5, 256, 0))
    # M = 2048 / 2046: 8 splits of 256 rows: XCD order; 2046: the last split has 254 rows, frame sides 33 x 31 are no powers of two
    add("3x3-2x32x32", T3, (2, 32, 32), 2048, C4[:2], (8, 256, 1))
    add("3x3-2x33x31", T3, (2, 33, 31), 2046, C4[1:], (8, 256, 1))
    # temporal (F, HW, 1) repeating over the samples; F = 1: both side taps always outside.  525 rows: 3 splits of 192
    add("temporal-2x1x35", TT, (1, 35, 1), 70, C4[:1], (1, 128, 0))
    add("temporal-5x3x35", TT, (3, 35, 1), 525, C4[1:2], (3, 192, 0))
    # audio, L = 100: two samples = 200 rows, one split; d = 128 > L: the side taps never land.  Six samples: 3 splits of 256 / 256 / 88
    for d in (1, 4, 128):
        add(f"audio-2x100-d{d}", E.taps_audio(d), (100, 1, 1), 200, C4[:1] if d != 4 else C4[3:], (1, 256, 0))
    add("audio-6x100-d4", E.taps_audio(4), (100, 1, 1), 600, C4[2:3], (3, 256, 0))
    # 1x1
    add("1x1-77", E.TAPS_1, (1, 1, 1), 77, C4[:1], (1, 128, 0))
    add("1x1-1050", E.TAPS_1, (1, 1, 1), 1050, C4[2:3], (5, 256, 0))
    add("1x1-2046", E.TAPS_1, (1, 1, 1), 2046, C4[1:2], (8, 256, 1))
    return cases


# wgrad_kernel<__bf16>: Cin < 64 or Cout < 64 (the input / output convs); Cout = 2056: colsum in two slabs (2048 + 8)
WGRAD64_BF16_CHANS = [(8, 64), (64, 8), (32, 40), (8, 2056)]
WGRAD64_BF16_GEOMS = ["3x3-2x21x25", "audio-2x100-d4", "1x1-1050", "temporal-5x3x35"]
# the two child processes (MMD_WGRAD_TR=0: wgrad128_bf16_kernel; MMD_WGRAD_TILE64=1: wgrad_kernel<__bf16> at every width)
WGRAD_CHILD_GEOMS = ["3x3-2x5x7", "3x3-2x21x25", "3x3-2x33x31", "temporal-5x3x35", "audio-6x100-d4", "1x1-77"]
# (geometry of wgrad_cases, Cin, Cout) of the ConvFn.backward tests: one per tap family, and 128 -> 72 on five splits of rows
DGRAD = [("1x1-77", 64, 96), ("3x3-2x5x7", 64, 96), ("3x3-2x21x25", 128, 72), ("temporal-5x3x35", 64, 96), ("audio-2x100-d4", 64, 96)]
GN_AUTOGRAD = [("bf16", 96, "per_sample_film", 30), ("f32", 96, "temporal", 7), ("bf16", 320, "spatial", 257)]     # GroupNormFn: dtype, C, kind, Tn
COLSUM_SLICES = [(2, 100, 96, "bf16"), (3, 257, 2056, "bf16"), (2, 130, 264, "f32"), (2, 1, 1056, "f32")]          # S, Tn, C, dtype


def wgrad_case(name):
    return next(c for c in wgrad_cases() if c["name"] == name)


def wgrad64_bf16_cases():
    """(case, (Cin, Cout)) of the wgrad_kernel<__bf16> tests."""
    return [(wgrad_case(g), ch) for g in WGRAD64_BF16_GEOMS for ch in WGRAD64_BF16_CHANS]


# --------------------------------------------------------------------------- GroupNorm
GN_EPS = 1e-5


def gn_slices(kind, N, Tn, HW=3):
    """Row indices [S, Tn] of every slice and the Geom constructor arguments (S, Tn, inner, outer_stride, inner_stride, tstride)."""
    if kind.startswith("per_sample") or kind == "spatial":
        return torch.arange(N * Tn).reshape(N, Tn), (N, Tn, 1, Tn, 1, 1)
    assert kind == "temporal"                                   # rows (n, f, pixel): slice (n, pixel) takes every HW-th row
    idx = torch.arange(N * Tn * HW).reshape(N, Tn, HW).permute(0, 2, 1).reshape(N * HW, Tn)
    return idx, (N * HW, Tn, HW, Tn * HW, 1, HW)


def gn_fwd_ref(x, gamma, beta, film, slices):
    """float64 forward of one GroupNorm32(+FiLM): a, b [S, C], mean, rstd [S, 32] and their fp32 bounds (module docstring)."""
    x, gamma, beta, film = _f64(x), _f64(gamma), _f64(beta), _f64(film)
    S, Tn = slices.shape
    C = x.shape[1]
    cpg = C // 32
    xs = x[slices.to(x.device)].reshape(S, Tn, 32, cpg)
    piv = xs[:, :1, :, :1]
    d = xs - piv
    cnt = Tn * cpg
    Sd, Sq = d.abs().sum((1, 3)), (d * d).sum((1, 3))
    dm = d.sum((1, 3)) / cnt
    mean = piv[:, 0, :, 0] + dm
    var = (Sq / cnt - dm * dm).clamp_min(0)
    rstd = (var + GN_EPS).rsqrt()
    e_dm = (Tn + 2) * U32 * Sd / cnt
    e_mean = e_dm + U32 * mean.abs()
    e_var = (Tn + 4) * U32 * Sq / cnt + 2 * dm.abs() * e_dm
    e_rstd = rstd ** 3 * e_var / 2 + U32 * rstd
    a, b, e_a, e_b = gn_affine(mean, rstd, e_mean, e_rstd, gamma, beta, film)
    return dict(a=a, b=b, mean=mean, rstd=rstd, e_a=e_a, e_b=e_b, e_mean=e_mean, e_rstd=e_rstd)


def gn_affine(mean, rstd, e_mean, e_rstd, gamma, beta, film):
    """The fused affine a, b [S, C] in float64 from mean, rstd [S, 32] and its bounds e_a, e_b from theirs (module docstring): the
    arithmetic every GroupNorm kernel shares (a = rstd gamma, b = beta - mean a, then a *= 1 + scale, b = b (1 + scale) + shift)."""
    S = mean.shape[0]
    C = gamma.shape[0]
    cpg = C // 32
    rep = lambda t: t.repeat_interleave(cpg, dim=1)                              # [S, 32] -> [S, C]
    sc = 1 + film[:, :C] if film is not None else torch.ones(S, C, dtype=torch.float64, device=mean.device)
    sh = film[:, C:2 * C] if film is not None else torch.zeros(S, C, dtype=torch.float64, device=mean.device)
    a0 = rep(rstd) * gamma
    a = a0 * sc
    b = (beta - rep(mean) * a0) * sc + sh
    e_a = (gamma * sc).abs() * rep(e_rstd) + 3 * U32 * a.abs()
    e_b = sc.abs() * (a0.abs() * rep(e_mean) + (rep(mean) * gamma).abs() * rep(e_rstd)) \
        + 4 * U32 * ((beta * sc).abs() + (rep(mean) * a0 * sc).abs() + sh.abs())
    return a, b, e_a, e_b


def gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=None, out_dtype=torch.float32):
    """float64 GroupNorm32(+FiLM)(+SiLU) backward from the stored x and dy.  stored = (a, b, mean, rstd) as the forward kernel wrote
    them (the backward's inputs); None: the float64 forward values (then the result is the exact gradient, what autograd gives).
    Returns a dict: dx [rows, C] (rows outside every slice NaN), dgamma, dbeta [C], dfilm [S, 2C] (None without film), each with its
    bound e_*, and fwd = gn_fwd_ref's dict."""
    fwd = gn_fwd_ref(x, gamma, beta, film, slices)
    x, dy, gamma, beta, film = _f64(x), _f64(dy), _f64(gamma), _f64(beta), _f64(film)
    a, b, mean, rstd = (fwd["a"], fwd["b"], fwd["mean"], fwd["rstd"]) if stored is None else (_f64(t) for t in stored)
    S, Tn = slices.shape
    C = x.shape[1]
    cpg = C // 32
    cnt = Tn * cpg
    sl = slices.to(x.device)
    rep = lambda t: t.repeat_interleave(cpg, dim=-1)
    xs, ds = x[sl], dy[sl]                                                        # [S, Tn, C]
    A, B, mu, rs = a[:, None], b[:, None], rep(mean)[:, None], rep(rstd)[:, None]
    if act:
        v = xs * A + B
        sg = torch.sigmoid(v)
        w = 1 - sg
        q = 1 + v * w
        r = sg * q
        dv = ds * r
        e_v = 2 * U32 * ((xs * A).abs() + B.abs())
        e_sg = sg * (w * (e_v + U32 * v.abs() + 2 * U32) + 3 * U32)
        e_w = e_sg + U32 * w
        e_q = v.abs() * e_w + w * e_v + U32 * (v * w).abs() + U32 * q.abs()
        e_r = sg * e_q + q.abs() * e_sg + U32 * r.abs()
        e_dv = ds.abs() * e_r + U32 * dv.abs()
    else:
        dv, e_dv = ds, torch.zeros_like(ds)
    z = (xs - mu) * rs
    P, Q = dv.sum(1), (dv * z).sum(1)                                             # [S, C]
    e_P = (Tn + 1) * U32 * dv.abs().sum(1) + e_dv.sum(1)
    e_Q = (Tn + 4) * U32 * (dv * z).abs().sum(1) + (e_dv * z.abs()).sum(1)
    sc = 1 + film[:, :C] if film is not None else torch.ones_like(P)
    g = sc * gamma
    grp = lambda t: t.reshape(S, 32, cpg).sum(-1)
    m1, m2 = grp(g * P) / cnt, grp(g * Q) / cnt
    e_m1 = (grp(g.abs() * e_P) + (cpg + 4) * U32 * grp((g * P).abs())) / cnt
    e_m2 = (grp(g.abs() * e_Q) + (cpg + 4) * U32 * grp((g * Q).abs())) / cnt
    M1, M2, eM1, eM2 = (rep(t)[:, None] for t in (m1, m2, e_m1, e_m2))
    k1, k2, k3 = rs * g[:, None], -rs * rs * M2, rs * (mu * rs * M2 - M1)
    dxs = rs * (g[:, None] * dv - M1 - z * M2)
    e_k1 = 3 * U32 * k1.abs()
    e_k2 = rs * rs * eM2 + 2 * U32 * k2.abs()
    e_k3 = rs * ((mu * rs).abs() * eM2 + eM1) + 4 * U32 * rs * ((mu * rs * M2).abs() + M1.abs())
    e_dxs = k1.abs() * e_dv + e_k1 * dv.abs() + e_k2 * xs.abs() + e_k3 + 3 * U32 * ((k1 * dv).abs() + (k2 * xs).abs() + k3.abs())
    if out_dtype == torch.bfloat16:
        e_dxs = U16 * (dxs.abs() + e_dxs) + e_dxs
    dx = torch.full_like(x, float("nan"))
    e_dx = torch.full_like(x, float("nan"))
    dx[sl], e_dx[sl] = dxs, e_dxs
    out = dict(dx=dx, e_dx=e_dx, fwd=fwd, P=P, Q=Q)
    out["dgamma"], out["dbeta"] = (sc * Q).sum(0), (sc * P).sum(0)
    out["e_dgamma"] = (sc.abs() * e_Q + 2 * U32 * (sc * Q).abs()).sum(0) + (S + 1) * U32 * (sc * Q).abs().sum(0)
    out["e_dbeta"] = (sc.abs() * e_P + 2 * U32 * (sc * P).abs()).sum(0) + (S + 1) * U32 * (sc * P).abs().sum(0)
    if film is not None:
        out["dfilm"] = torch.cat([gamma * Q + beta * P, P], dim=1)
        out["e_dfilm"] = torch.cat([gamma.abs() * e_Q + beta.abs() * e_P + 3 * U32 * ((gamma * Q).abs() + (beta * P).abs()), e_P], dim=1)
    else:
        out["dfilm"] = out["e_dfilm"] = None
    return out


def gn_cases():
    """(dtype, C, kind, Tn, big_mean).  kind: per_sample_film (FiLM + SiLU), per_sample (SiLU), spatial, temporal (neither).
    Every width meets every Tn on the fullest path; the other geometries at Tn = 7 and 30; the inputs with mean = 20 std at 30 and 257.
    Thread shapes (256 / (C / EPV) row lanes, EPV = 8 bf16 / 4 fp32): bf16 32 -> 64 lanes, 96 -> 21 (4 idle threads), 160 -> 12 (16
    idle), 320 -> 6 (16 idle), 2048 -> 1; fp32 96 -> 10 (16 idle), 1024 -> 1, 1056 -> two column chunks of 132 vectors, 1 lane (124 idle).
    Tn = 7 and 30 are multiples of none of the lane counts above 1, 257 = 4 * 64 + 1, Tn = 1 leaves all lanes but one without a row."""
    cases = []
    for dt, widths in (("bf16", (32, 96, 160, 320, 2048)), ("f32", (96, 1024, 1056))):
        for C in widths:
            for Tn in (1, 7, 30, 257):
                cases.append((dt, C, "per_sample_film", Tn, False))
            for kind in ("per_sample", "spatial", "temporal"):
                for Tn in (7, 30):
                    cases.append((dt, C, kind, Tn, False))
            for Tn in (30, 257):
                cases.append((dt, C, "per_sample_film", Tn, True))
    return cases


# --------------------------------------------------------------------------- attention backward
def attn_bwd_ref(q, k, v, o_stored, do, heads, mode):
    """One (query set, key set) pair: q, do [Tq, C], k, v [Tk, C] (C = heads * ch), o_stored [Tq, C] or None (D from the float64
    forward output: the exact gradient; always so in mode 'small').  mode: 'mfma' (P, dS rounded to bf16), 'valu', 'small'.
    Returns a dict of float64 tensors: dq, e_dq [Tq, C]; dk, dv [Tk, C] and the additive error parts of this pair Ek, Sk, Ev, Sv
    (e_dK = Ek + (Nq + 4) u Sk, e_dV = Ev + (Nq + 1 or 2) u Sv once the pairs are summed: `attn_bwd_bound_kv`); lse2, e_lse2 [Tq, heads]."""
    q, k, v, do = _f64(q), _f64(k), _f64(v), _f64(do)
    Tq, C = q.shape
    n = k.shape[0]
    ch = C // heads
    sc = 1.0 / math.sqrt(ch)
    hd = lambda t: t.reshape(-1, heads, ch).permute(1, 0, 2)                     # [heads, T, ch]
    qh, kh, vh, gh = hd(q), hd(k), hd(v), hd(do)
    a = sc * qh @ kh.transpose(1, 2)
    A = sc * qh.abs() @ kh.abs().transpose(1, 2)
    lse = torch.logsumexp(a, dim=-1, keepdim=True)
    p = torch.exp(a - lse)
    dP = gh @ vh.transpose(1, 2)
    AP = gh.abs() @ vh.abs().transpose(1, 2)
    R = (a.amax(-1) - a.amin(-1))[..., None]
    T = -(-n // 32)
    eps = ((ch + 3) * A + 2 * R + 2) * U32
    e_L = (p * eps).sum(-1, keepdim=True) + (n + T * (2 * R + 3) + 4) * U32 + 3 * U32 * lse.abs()
    eps_P = ((ch + 3) * A + (a - lse).abs() + 2) * U32 + e_L
    if o_stored is None or mode == "small":
        D = (p * dP).sum(-1, keepdim=True)
    else:
        D = (gh * hd(_f64(o_stored))).sum(-1, keepdim=True)
    if mode == "small":
        e_D = (p * ((eps_P + (n + 2) * U32) * dP.abs() + (ch + 1) * U32 * AP)).sum(-1, keepdim=True)
    else:
        oh = hd(_f64(o_stored)) if o_stored is not None else p @ vh
        e_D = (ch + 1) * U32 * (gh * oh).abs().sum(-1, keepdim=True)
    dS = p * (dP - D)
    e_dS = p * ((eps_P + 2 * U32) * (dP - D).abs() + (ch + 1) * U32 * AP + e_D)
    E_P = p * eps_P
    if mode == "mfma":
        e_dS = e_dS + U16 * (dS.abs() + e_dS)
        E_P = E_P + U16 * p * (1 + eps_P)
    back = lambda t: t.permute(1, 0, 2).reshape(-1, C)
    SQ = sc * dS.abs() @ kh.abs()
    out = dict(dq=back(sc * dS @ kh), e_dq=back(sc * e_dS @ kh.abs() + (n + 4) * U32 * SQ))
    out["dk"], out["dv"] = back(sc * dS.transpose(1, 2) @ qh), back(p.transpose(1, 2) @ gh)
    out["Ek"], out["Sk"] = back(sc * e_dS.transpose(1, 2) @ qh.abs()), back(sc * dS.abs().transpose(1, 2) @ qh.abs())
    out["Ev"], out["Sv"] = back(E_P.transpose(1, 2) @ gh.abs()), back(p.transpose(1, 2) @ gh.abs())
    out["lse2"] = (lse[..., 0] / LN2).t()                                        # [Tq, heads]
    out["e_lse2"] = (e_L[..., 0] / LN2).t()
    return out


def attn_out_bound(ref, e, out_dtype):
    return e if out_dtype == torch.float32 else U16 * (ref.abs() + e) + e


def attn_bwd_bound_kv(Esum, Ssum, nq, ref, out_dtype, extra):
    """Bound of a dK / dV element from the summed per-pair parts; nq [Tk, 1] = number of queries that see the key; extra = the
    roundings besides the Nq of the sum: dK 4 (the zero start, the scale constant, the multiply by it, the product in the VALU
    kernels), dV 1 on the MFMA (bf16 x bf16 products are exact) and 2 in the VALU kernels (p dO is an fp32 product, rounded once:
    mmd_attn_bwd_body.inc:255, mmd_attn_bwd.hip:274)."""
    return attn_out_bound(ref, Esum + (nq + extra) * U32 * Ssum, out_dtype)


SELF_ATTN_BWD = [(4, 4, 16, 2), (70, 1, 96, 2), (130, 2, 48, 2), (257, 2, 64, 2), (130, 1, 192, 2), (200, 1, 128, 2),
                 (130, 2, 32, 4)]                                                # T, heads, ch, batches; the last: heads * nb = 8
# (F, HW, L, win, shift, heads, ch): errbound.CROSS_ATTN, the longer last audio group (43 = 4 * 10 + 3), and the same without
# shift and with one-group windows, where the audio positions 40 ... 42 lie in no video query's window
CROSS_ATTN_BWD = E.CROSS_ATTN + [(4, 8, 43, 3, 2, 2, 32), (4, 8, 43, 1, 0, 2, 32)]
VALU_ATTN_BWD = [(70, 2, 32), (16, 2, 24)]                                       # T, heads, ch
TEMPORAL_ATTN_BWD = E.TEMPORAL_ATTN
# the pass through SelfAttnFn / CrossAttnFn: spatial (T, heads, ch, N * F), temporal (F, HW, heads, ch), cross as above
ATTN_AUTOGRAD = dict(spatial=(70, 2, 32, 6), temporal=TEMPORAL_ATTN_BWD[1], cross=CROSS_ATTN_BWD[-2])


def cross_pairs(N, F, HW, L, win, shift, device="cpu"):
    """(video query rows, audio key rows) and (audio query rows, video key rows) of every (sample, group), as the forward defines
    them (tests/test_elementwise_gpu.py): windows wrap modulo the key count, the last audio group owns the remainder L - F * apf."""
    apf = L // F
    ar = lambda *a: torch.arange(*a, device=device)
    vp, ap = [], []
    for n in range(N):
        for i in range(F):
            vp.append((n * F * HW + ar(i * HW, (i + 1) * HW), n * L + (ar(win * apf) + (i + shift) * apf) % L))
            ap.append((n * L + ar(i * apf, L if i == F - 1 else (i + 1) * apf), n * F * HW + (ar(win * HW) + (i + shift) * HW) % (F * HW)))
    return vp, ap


def attn_bwd_assemble(qbuf, kvbuf, o_stored, do, pairs, heads, mode, out_dtype):
    """Every (query rows, key rows) pair of one attention call: qbuf [Nq, 3C] (q in columns [0, C)), kvbuf [Nk, 3C] (k in [C, 2C),
    v in [2C, 3C)), o_stored / do [Nq, C].  Every query row is covered exactly once; key rows any number of times (0: dK = dV = 0
    with a zero bound).  Returns dq, dk, dv with bounds e_dq, e_dk, e_dv, lse2 / e_lse2 [Nq, heads] and nq [Nk] (queries per key)."""
    C = do.shape[1]
    dev = qbuf.device
    z = lambda r, c=C: torch.zeros(r, c, dtype=torch.float64, device=dev)
    Nq, Nk = qbuf.shape[0], kvbuf.shape[0]
    out = dict(dq=z(Nq), e_dq=z(Nq), dk=z(Nk), dv=z(Nk), lse2=z(Nq, heads), e_lse2=z(Nq, heads))
    Ek, Sk, Ev, Sv, nq = z(Nk), z(Nk), z(Nk), z(Nk), z(Nk, 1)
    seen = torch.zeros(Nq, dtype=torch.int32, device=dev)
    for qi, ki in pairs:
        r = attn_bwd_ref(qbuf[qi, :C], kvbuf[ki, C:2 * C], kvbuf[ki, 2 * C:], None if o_stored is None else o_stored[qi], do[qi], heads, mode)
        out["dq"][qi], out["lse2"][qi], out["e_lse2"][qi] = r["dq"], r["lse2"], r["e_lse2"]
        out["e_dq"][qi] = attn_out_bound(r["dq"], r["e_dq"], out_dtype)
        seen[qi] += 1
        for acc, key in ((out["dk"], "dk"), (out["dv"], "dv"), (Ek, "Ek"), (Sk, "Sk"), (Ev, "Ev"), (Sv, "Sv")):
            acc.index_add_(0, ki, r[key])                     # (the key rows of one pair are distinct)
        nq.index_add_(0, ki, torch.full((len(ki), 1), float(len(qi)), dtype=torch.float64, device=dev))
    assert bool((seen == 1).all())
    out["e_dk"] = attn_bwd_bound_kv(Ek, Sk, nq, out["dk"], out_dtype, 4)
    out["e_dv"] = attn_bwd_bound_kv(Ev, Sv, nq, out["dv"], out_dtype, 1 if mode == "mfma" else 2)
    out["nq"] = nq[:, 0]
    return out


def check_gn(got, r, what):
    """The forward's a, b, mean, rstd against float64, then the backward's outputs; returns the worst ratios."""
    f = r["fwd"]
    worst = {}
    for k in ("a", "b", "mean", "rstd"):
        worst[k] = E.check(got[k], f[k], f["e_" + k], what=f"{what}: forward {k}")
    ok = ~torch.isnan(r["dx"][:, 0])
    worst["dx"] = E.check(got["dx"][ok], r["dx"][ok], r["e_dx"][ok], what=f"{what}: dx")
    assert bool(torch.isnan(got["dx"][~ok].float()).all()), f"{what}: rows outside every slice written"
    for k in ("dgamma", "dbeta"):
        worst[k] = E.check(got[k][None], r[k][None], r["e_" + k][None], what=f"{what}: {k}")
    if r["dfilm"] is not None:
        worst["dfilm"] = E.check(got["dfilm"], r["dfilm"], r["e_dfilm"], what=f"{what}: dfilm")
    return worst


def check_attn_bwd(got, r, C, what, heads):
    dq, dk, dv = got
    ch = C // heads
    w = [check_groups(dq, r["dq"], r["e_dq"], ch, "head", what + ": dQ"), check_groups(dk, r["dk"], r["e_dk"], ch, "head", what + ": dK"),
         check_groups(dv, r["dv"], r["e_dv"], ch, "head", what + ": dV")]
    dead = r["nq"] == 0
    assert bool((dk[dead] == 0).all()) and bool((dv[dead] == 0).all()), what + ": keys in nobody's window must have zero gradients"
    return max(w)
