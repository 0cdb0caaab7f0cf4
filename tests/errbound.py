"""Element-wise error bounds against float64 references (test infrastructure; plain torch, no import of the package under test).

A whole-tensor rel-L2 cannot see an error confined to a few rows, one border or one tap, nor a small systematic one (an extra
rounding per K step).  The helpers here give every output ELEMENT its own budget, derived from how the kernels are allowed to
compute, and `check` admits no violating element at all.

Notation: u = 2**-24 (unit roundoff of fp32), v = 2**-8 (unit roundoff of bf16: round-to-nearest to 8 significand bits moves a
value by at most half a unit in the last place = 2**-8 relative).  All bounds are first order in u (terms of order K u^2 are
below 3e-4 of the bound at the deepest K used, 4608).

conv-as-GEMM (`conv_rows_ref`, `gemm_bound`)
    The kernels compute  y[m, c] = fl( sum_k x[src(m, k)] w[c, k] + bias[c] + residual[m, c] )  with fp32 accumulation on the MFMA,
    in some order (tiles 64 / 128 / 129 / 131 / 132: k order in 128-byte steps; tiles 130 / 133: channel-chunk major; the MFMA adds
    16 (bf16) or 2 (fp32) products per instruction in an order of its own), then `acc + bias`, `+ residual` in fp32
    (mmd_gemm.hip: gemm_epilogue) and ONE round-to-nearest-even conversion on store (mmd_common.h: Elt<__bf16>::pack).
    A sum of n fp32 terms accumulated in ANY order carries at most (n - 1) u sum|terms| (every partial sum is rounded once and is
    bounded by the sum of absolute values); K products, the bias and the residual are K + 2 terms, and a product of two fp32
    operands is itself rounded once (bf16 x bf16 products are exact in fp32), so with
        S[m, c] = sum_k |x[src(m, k)]| |w[c, k]| + |bias[c]| + |residual[m, c]|
        e32 = (K + 2) u S
    |acc - ref| <= e32 holds for every legal order.  Random rounding errors add like sqrt(K), so the typical error sits about
    sqrt(K) below e32 - that gap is the headroom for the matrix core's internal adder (which is not specified to round every
    partial sum to nearest).  fp32 output: bound = e32.  bf16 output: the stored value is rn(acc) with |acc| <= |ref| + e32, so
        bound = v (|ref| + e32) + e32.
    Truncation on store costs up to 2 v, a second rounding (accumulator held in bf16 anywhere) another v per occurrence: both
    exceed the bound.

attention (`attn_ref`, `attn_bound`)
    out[i, d] = sum_j p_ij v_jd, p = softmax_j(a_ij), a_ij = ch**-0.5 q_i . k_j.  With Sv[i, d] = sum_j p_ij |v_jd|:
    * weights perturbed by relative errors eps_ij move the ratio sum_j e_ij v_jd / sum_j e_ij by at most
      sum_j p_ij eps_ij |v_jd| + |out| sum_j p_ij eps_ij  (numerator and denominator).
    * P in bf16 in front of the PV MFMA (mmd_attn_common.h: p_frag, `pf[j] = (__bf16)s[..]`, the one packing of all four flash
      kernels; mmd_attn_pipe_body.inc: the v_cvt_pk_bf16_f32 of the P registers): eps <= v on the NUMERATOR only, because every
      flash kernel sums the row from the UNROUNDED fp32 exponentials (mmd_attn_common.h: softmax_step, `psp[..] += e` and
      `l_run = l_run * alpha + ps`; the pipelined body is bitwise the DMA-staged kernel).  So the P term is c v Sv with c = 1.
      (A row sum taken from the rounded P would add v |out| <= v Sv: c = 2.  Not what the kernels do, so not granted.)
    * attn_small_mfma_kernel (mmd_attn.hip: `lo4` / `pf`) feeds P as a bf16 hi + lo pair: lo = e - bf16(e), |lo| <= v e, and
      rounding lo to bf16 costs v |lo| <= v^2 e: P term v^2 Sv (p_round = 2**-16).
    * the VALU kernels (attn_generic_kernel, attn_small_kernel: `__expf(..)` to the `oacc` / `o` sums) and fp32 mode keep P in
      fp32: no P term.
    * fp32-level terms, returned by attn_ref as `e32` (absolute, per element), D = ch, n = keys, T = ceil(n / 32) key tiles (32 =
      the smallest key tile of any kernel: attn_generic_kernel<T, 32, 12>), A_ij = ch**-0.5 sum_d |q_id k_jd|,
      R_i = max_j a_ij - min_j a_ij:
        score:     D products summed in fp32, the scale applied to q (the VALU kernels' Q loads) or inside the exp2 fma with the
                   constant scale * log2(e) rounded once (`sc`; softmax_step): |da_ij| <= (D + 3) u A_ij
        argument:  a_ij - m is rounded once (softmax_step's fma / the VALU kernels' subtraction), |a_ij - m| <= R_i, and __expf multiplies by
                   log2(e) once more: 2 u R_i
        exp:       v_exp_f32 is accurate to 1 ulp = 2 u relative
        so         eps_ij = ((D + 3) A_ij + 2 R_i + 2) u, entering as in the first bullet;
        rescale:   per key tile alpha = exp2(m_old - m_new) carries 2 u R_i + 2 u and o *= alpha one rounding (softmax_step); it
                   reweights the earlier keys against the later ones: T (2 R_i + 3) u Sv
        PV, sums:  n products accumulated in fp32: (n + 1) u Sv; the row sum of n terms: n u |out| <= n u Sv
        1 / l, o * inv (the epilogues; store_o_rows_via_lds): 3 u |out| <= 3 u Sv
    bound, fp32 output: e32.  bf16 output, with eP = p_round * Sv:  v (|ref| + eP + e32) + eP + e32.

GroupNorm fused into the GEMM loader (tests/test_elementwise_gpu.py: the tile-128 loader)
    conv_gemm_kernel<.., GN = true>::store_tile (mmd_gemm.hip:322-337) computes  pack(silu_f(x * a + b))  with the expressions of
    gn_apply_kernel (mmd_norm.hip:279-282): the operand that reaches the MFMA is bit for bit what gn_apply stores, so the
    reference is conv_rows_ref on gn_apply's stored output and the bound gains no term.
"""
import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8

# tap tables, (d0, d1, d2) offsets; the same lists as mm_diffusion.ops (tests/test_errbound_cpu.py asserts that)
TAPS_1 = [(0, 0, 0)]
TAPS_SPATIAL = [(0, dh, dw) for dh in (-1, 0, 1) for dw in (-1, 0, 1)]
TAPS_TEMPORAL = [(df, 0, 0) for df in (-1, 0, 1)]
TAPS_TEMPORAL_D1 = [(0, df, 0) for df in (-1, 0, 1)]


def taps_audio(d):
    return [(-d, 0, 0), (0, 0, 0), (d, 0, 0)]


def _f64(t):
    return None if t is None else t.detach().double()


def conv_gather(x, taps, dims):
    """The rows of x [M, Cin] every tap reads: a list of ([M, Cin] tensor, [M] bool mask), zero where the tap leaves [0, Di).
    Row m has coordinates (m // (D1 D2) % D0, m // D2 % D1, m % D2): the block of D0 D1 D2 rows repeats over M."""
    M = x.shape[0]
    D0, D1, D2 = (int(d) for d in dims)
    m = torch.arange(M, device=x.device)
    p2, p1, p0 = m % D2, (m // D2) % D1, (m // (D1 * D2)) % D0
    out = []
    for d0, d1, d2 in taps:
        ok = (p0 + d0 >= 0) & (p0 + d0 < D0) & (p1 + d1 >= 0) & (p1 + d1 < D1) & (p2 + d2 >= 0) & (p2 + d2 < D2)
        src = (m + d0 * D1 * D2 + d1 * D2 + d2).clamp(0, M - 1)
        out.append((x[src] * ok[:, None].to(x.dtype), ok))
    return out


def conv_rows_ref(x, w, bias, residual, taps, dims):
    """float64 conv-as-GEMM over rows and the matching sum of absolute values.  x [M, Cin], w [Cout, ntaps * Cin] (K index =
    tap * Cin + ci, the order of ops.pack_conv_weight), bias [Cout] or None, residual [M, Cout] or None: the STORED operands
    (bf16 or fp32).  Returns (ref, S), both float64 [M, Cout] on x's device."""
    x, w, bias, residual = _f64(x), _f64(w), _f64(bias), _f64(residual)
    M, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape[1] == len(taps) * Cin
    ref = torch.zeros(M, Cout, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(ref)
    for t, (g, _) in enumerate(conv_gather(x, taps, dims)):
        wt = w[:, t * Cin:(t + 1) * Cin]
        ref += g @ wt.t()
        S += g.abs() @ wt.abs().t()
    if bias is not None:
        ref += bias
        S += bias.abs()
    if residual is not None:
        ref += residual
        S += residual.abs()
    return ref, S


def gemm_bound(ref, S, K, out_dtype):
    """Per-element bound for an fp32-accumulating GEMM of depth K with bias and residual (module docstring)."""
    e32 = (K + 2) * U32 * S
    if out_dtype == torch.float32:
        return e32
    assert out_dtype == torch.bfloat16
    return U16 * (ref.abs() + e32) + e32


def attn_ref(q, k, v, heads):
    """One (query set, key set) pair in float64: q [Tq, C], k / v [Tk, C] (rows, C = heads * ch), the stored operands.
    Returns (ref, Sv, e32), float64 [Tq, C]: the attention output, Sv = sum_j p_j |v_j| and the fp32-level error term of the
    module docstring."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    Tq, C = q.shape
    n = k.shape[0]
    ch = C // heads
    sc = 1.0 / math.sqrt(ch)
    qh, kh, vh = (t.reshape(-1, heads, ch).permute(1, 0, 2) for t in (q, k, v))        # [heads, T, ch]
    a = sc * qh @ kh.transpose(1, 2)                                                  # [heads, Tq, n]
    A = sc * qh.abs() @ kh.abs().transpose(1, 2)
    p = torch.softmax(a, dim=-1)
    ref = p @ vh
    Sv = p @ vh.abs()
    R = (a.amax(-1) - a.amin(-1))[..., None]                                          # [heads, Tq, 1]
    eps = ((ch + 3) * A + 2 * R + 2) * U32
    T = -(-n // 32)
    e32 = (p * eps) @ vh.abs() + ref.abs() * (p * eps).sum(-1, keepdim=True) + (T * (2 * R + 3) + 2 * n + 4) * U32 * Sv
    back = lambda t: t.permute(1, 0, 2).reshape(Tq, C)
    return back(ref), back(Sv), back(e32)


def attn_bound(ref, Sv, out_dtype, e32, p_round=None):
    """Per-element bound of an attention output.  p_round: relative rounding of P in front of the PV product - 2**-8 (the flash
    MFMA kernels, the default for bf16), 2**-16 (attn_small_mfma_kernel's hi + lo pair) or 0 (VALU kernels; always in fp32 mode)."""
    if out_dtype == torch.float32:
        assert not p_round
        return e32
    assert out_dtype == torch.bfloat16
    eP = (U16 if p_round is None else p_round) * Sv          # c = 1: the row sum is taken from the unrounded exponentials
    return U16 * (ref.abs() + eP + e32) + eP + e32


def _hist(idx, mod, top=8):
    c = torch.bincount(idx % mod, minlength=1)
    nz = torch.nonzero(c).flatten()
    order = nz[torch.argsort(c[nz], descending=True)][:top]
    return ", ".join(f"{int(i)}:{int(c[i])}" for i in order) + (" ..." if nz.numel() > top else "")


def violations(y, ref, bound):
    """(number of elements that are not finite or lie outside the bound, worst error / bound ratio, their mask)."""
    yd = y.detach().double()
    err = (yd - ref).abs()
    bad = ~torch.isfinite(yd) | ~(err <= bound)                       # (a NaN fails `<=`)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(nan=float("inf"), posinf=float("inf"))
    return int(bad.sum()), float(ratio.max()), bad


def check(y, ref, bound, pixels=None, what=""):
    """Every element of y [M, C] finite and within bound of ref: the allowed number of violations is ZERO.  Returns the worst
    error / bound ratio; on failure reports the count, the worst ratio, the first violations and their histograms by row % 128,
    column % 128 and (pixels = D1 * D2 of a 3x3 conv) by pixel."""
    assert y.shape == ref.shape == bound.shape, (y.shape, ref.shape, bound.shape)
    nbad, worst, bad = violations(y, ref, bound)
    if nbad:
        rc = torch.nonzero(bad).cpu()
        rows, cols = rc[:, 0], rc[:, 1]
        first = ", ".join(f"({int(r)},{int(c)}): got {float(y[int(r), int(c)]):.6g} ref {float(ref[int(r), int(c)]):.6g} "
                          f"bound {float(bound[int(r), int(c)]):.3g}" for r, c in rc[:6])
        msg = (f"{what}: {nbad} of {y.numel()} elements outside the bound (non-finite: {int((~torch.isfinite(y.double())).sum())}), "
               f"worst error/bound {worst:.3g}\n  first: {first}\n  by row % 128: {_hist(rows, 128)}\n  by column % 128: {_hist(cols, 128)}")
        if pixels:
            msg += f"\n  by pixel (row % {pixels}): {_hist(rows, pixels)}"
        raise AssertionError(msg)
    return worst


# --------------------------------------------------------------------------- the shapes of tests/test_elementwise_gpu.py
# (kept here so that tests/test_errbound_cpu.py proves the metric on exactly these shapes)
def conv_cases():
    """Every conv_gemm launch geometry of the GPU file: dicts with name, M, Cin, Cout, taps, dims, tiles (the forced main loops),
    dtypes ('f32' / 'bf16') and pixels (for the histogram of 3x3 convs)."""
    cases = []

    def add(name, M, Cin, Cout, taps, dims, tiles, dtypes=("f32", "bf16"), pixels=None):
        cases.append(dict(name=name, M=M, Cin=Cin, Cout=Cout, taps=taps, dims=tuple(dims), tiles=tuple(tiles), dtypes=dtypes, pixels=pixels))

    # 1x1: ragged against both row tiles (293 = 2 * 128 + 37) with a ragged last column tile; Cin not a multiple of a K step; deep K
    for M, Cin, Cout in ((293, 256, 264), (77, 96, 72), (300, 1024, 128)):
        add(f"1x1-{M}x{Cin}x{Cout}", M, Cin, Cout, TAPS_1, (1, 1, 1), (64, 128, 129) + ((132,) if Cin % 64 == 0 else ()))
    # 3x3: frame sides that divide nothing; K = 4608, the deepest of the model family
    for D, Cin, Cout in (((3, 8, 16), 64, 136), ((2, 5, 7), 32, 96), ((2, 8, 16), 512, 128)):
        add(f"3x3-{D[0]}x{D[1]}x{D[2]}-{Cin}-{Cout}", D[0] * D[1] * D[2], Cin, Cout, TAPS_SPATIAL, D, (64, 128, 129), pixels=D[1] * D[2])
    # 3x3 on the halo tile: one patch row; interior patches as well as all four borders
    for D in ((3, 8, 16), (2, 24, 48)):
        for Cin in (64, 192):
            for Cout in (96, 264):
                add(f"halo-{D[0]}x{D[1]}x{D[2]}-{Cin}-{Cout}", D[0] * D[1] * D[2], Cin, Cout, TAPS_SPATIAL, D, (130,), pixels=D[1] * D[2])
    for D in ((2, 16, 32), (1, 32, 32)):
        add(f"halo16-{D[0]}x{D[1]}x{D[2]}", D[0] * D[1] * D[2], 256, 128, TAPS_SPATIAL, D, (133,), dtypes=("bf16",), pixels=D[1] * D[2])
    # temporal k=3 as (F, HW, 1) repeating over the N samples; F = 1: both side taps always outside the clip
    for N, F, HW in ((2, 1, 5), (2, 3, 5), (2, 16, 6)):
        add(f"temporal-{N}x{F}x{HW}", N * F * HW, 64, 72, TAPS_TEMPORAL, (F, HW, 1), (64, 128, 129))
    add("temporal_d1-2x8x16", 2 * 8 * 16, 64, 96, TAPS_TEMPORAL_D1, (2, 8, 16), (130,))
    # audio, two samples; d = 128 > L: the side taps never land
    for L, d in ((100, 1), (100, 4), (257, 16), (100, 128)):
        add(f"audio-L{L}-d{d}", 2 * L, 64, 96, taps_audio(d), (L, 1, 1), (64, 128, 129))
    return cases


def strip_cases():
    """Tile 131 (bf16): (name, M, Cin, Cout, taps, dims)."""
    cases = []
    for K in (128, 256, 384, 512):
        for M in (100, 288, 608):                   # 288 = 256 + 32, 608 = 512 + 96
            for Cout in ((64, 192) if K <= 256 else (96, 1536)):
                cases.append((f"strip-1x1-{M}x{K}x{Cout}", M, K, Cout, TAPS_1, (1, 1, 1)))
    cases.append(("strip-temporal-2x5x24", 2 * 5 * 24, 128, 96, TAPS_TEMPORAL, (5, 24, 1)))
    cases.append(("strip-audio4-2x150", 2 * 150, 128, 96, taps_audio(4), (150, 1, 1)))
    return cases


GN_LOADER_CASE = (3, 400, 256, 256)                  # S, Tn, Cin, Cout: blocks of 128 rows straddle the samples

SELF_ATTN = [(4, 4, 16), (70, 1, 96), (130, 2, 48), (257, 2, 64), (1024, 1, 64)]                     # T, heads, ch
TEMPORAL_ATTN = [(1, 6, 2, 64), (13, 4, 2, 32), (16, 3, 4, 96)]                                     # F, HW, heads, ch
CROSS_ATTN = [(8, 4, 8, 8, 0, 4, 16), (8, 4, 32, 8, 0, 2, 32),                                     # the two smallest
              (8, 16, 64, 1, 5, 2, 32), (8, 16, 64, 4, 3, 4, 32), (16, 4, 100, 4, 12, 2, 32)]      # the wrapping windows
