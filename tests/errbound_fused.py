"""Element-wise error bounds for the two FUSED chains of the sampling hot path - the VideoConv '2d+1d' (mmd_vconv.hip) and the temporal
attention block (mmd_tattn.hip) - against staged float64 references (test infrastructure; plain torch, no import of the package under
test).  Notation and house rules are those of tests/errbound.py and tests/errbound_fwd.py: u = 2**-24, v = 2**-8, every reference
float64 on the STORED operands, `errbound.check` admits zero violating elements.

Both kernels are chains of stages.  A stage computes in fp32 and rounds ONCE to bf16 where the unfused path would store a tensor; the
intermediates never reach memory, so they cannot be compared.  The reference is the same chain in float64 with one round-to-nearest-
even to bf16 restated at each of the kernel's rounding points (`rn_bf16`: straight from float64 - `t.double().to(torch.bfloat16)` goes
through float32 and rounds twice), and a per-element DEVIATION bound is carried from stage to stage.

deviation of a stored intermediate (`dev`)
    z = the reference's value in front of the rounding, s = rn_bf16(z), and the kernel's value in front of ITS rounding lies within D
    of z.  Rounding is monotone, so the kernel's stored value lies in [rn_bf16(z - D), rn_bf16(z + D)]:
        d = max(|rn_bf16(z + D) - s|, |rn_bf16(z - D) - s|)
    which is ZERO wherever no rounding midpoint lies in [z - D, z + D] and one bf16 step (rarely two) elsewhere.  A blanket v |z| + D
    would charge every element half a step at every stage: through the four stages of the attention block that moves the scores by
    about 0.5 and makes the bound vacuous; with the midpoint mask the bound stays first order.  (z +- D is itself computed in float64:
    D is widened by 2**-40 relative, a million times the rounding of that addition and 1e-12 of any bound here.)

per-stage D = the stage's own arithmetic term on the reference's stored inputs + the propagated deviation of those inputs
    own terms (existing helpers only):
        GroupNorm apply         errbound_fwd.apply_ref / two_pass_ref with an fp32 output (e_y: no store term - the store is `dev`)
        GEMM                    errbound.conv_rows_ref and errbound.gemm_bound's e32 = (K + 2) u S, S taken on |s| + d (`_gemm_stage`)
        softmax . V             errbound.attn_ref; eP + e32 of errbound.attn_bound with p_round = 2**-16 (the bf16 hi + lo pair of P)
    propagation through a GEMM: the operand moves by at most d, the weights are the stored ones:  sum_k |w| d
        = conv_rows_ref(d, |w|, None, None, taps, dims)  (padding taps gather d = 0: a padding slot is exactly zero in the kernel)
    propagation through attention (`_attn_prop`), per head, ch = 64, d* = deviations of the stored q, k, v:
        scores      |da_ij| <= ch**-0.5 sum_c (dq_ic |k_jc| + |q_ic| dk_jc + dq_ic dk_jc),      eta_ij = expm1(|da_ij|)
                    every weight e_ij moves by a relative factor in [exp(-|da|), exp(|da|)], i.e. by at most eta_ij; the bullet
                    "weights perturbed by relative errors" of errbound.py in its exact form (numerator sum_j p eta |v|, denominator
                    |out| sum_j p eta, over a denominator that shrank to no less than 1 - sum_j p eta) plus v's own deviation under
                    weights that grew to no more than p (1 + eta) / (1 - sum p eta) - the last factor is dropped on the dv term
                    (second order: dv and eta are both deviations):
        output      (sum_j p_ij eta_ij |v_jd| + |out_id| sum_j p_ij eta_ij) / (1 - sum_j p_ij eta_ij) + sum_j p_ij (1 + eta_ij) dv_jd
        VALIDITY    sum_j p_ij eta_ij < 1/2 on every row of every case (`tattn_ref` asserts it and returns the maximum; the CPU test
                    holds it on every case).  A condition of the formula, not a tolerance.
    final store: errbound_fwd._store, v (|ref| + D) + D.

fused VideoConv (`vconv_ref`; mmd_vconv.hip, rows (n, f, h, w), Cout = 128)
    rounding points (the header of the file names them):
      1. the normalised activation in bf16 in the halo: tr_piece :199-200 `w = x * a + b`, `silu_f(w)` (the apply step of
         errbound_fwd with the STORED fp32 a, b: e_a = e_b = 0) and vc_pack2 :48-52, `(__bf16)` = round-to-nearest-even.  Padding
         slots are zeroed per patch (:129-136) and left alone by the norm (:204, `gvalid`), so the zero padding pads the NORMALISED
         activation: the reference gathers zeros there, with deviation zero.  Without a norm (GNM = 0) the operand is the stored x.
      2. T = bf16(acc + bias_s) :414-415 (Elt<__bf16>::pack), K = 9 Cin in the order (32-channel chunk, tap, k): any order is inside
         (K + 2) u S.  Frames -1 and 16 of the T image are zero rows (:389-393): the temporal taps gather zeros with deviation zero,
         per SAMPLE (dims (16, H W, 1) repeating over the samples).
      3. the output bf16(acc + bias_t) :511-514, K = 3 * 128.
    stages: [apply -> dev] -> spatial GEMM -> dev -> temporal GEMM -> store.

temporal attention block (`tattn_ref`; mmd_tattn.hip, rows (n, f, pixel), C = 256, 4 heads, a sequence = the 16 frames of a pixel)
    rounding points: n1 :296-299, q / k + bias :329-331 and v + bias :339-340, P as hi + lo :374-376, O = oT * inv :391-392, the
    output (acc + bias) + residual :232-234 with the stored x as the residual.
    in-register GroupNorm (:276-302): the lane adds its 8 channels as a tree, ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) :280
    (depth 3), then four DPP row steps over the 16 frames (ta_row16_total :72-77, depth 4): D = 7 for the mean; the squares are a chain
    of 8 (:285) and the same four steps: D = 12.  mean = s * (1 / 128) :282 is exact, rstd = rsqrtf(q * (1 / 128) + eps) :287 and the
    affine `av = rstd * g, bv = b - mean * av, x * av + bv` :294-296 are gn_small's expressions (mmd_norm.hip:363, :367-368, :379-383).
    gn_small's depth is 4 Tn + qpg = 66 at Tn = 16, C = 256 - not smaller - so errbound_fwd.two_pass_ref(kernel="small") is reused as is.
    softmax (:346-376): 64 products per score on the MFMA, the maximum and the sum over the pixel's own 16 keys (:360-363, :371), exp2
    with scale * log2(e) folded into one fma (:368; `msc = mx * sc` is common to the row and cancels in the ratio), the row sum from the
    UNROUNDED exponentials (:369), P as the bf16 pair hi = bf16(e), lo = bf16(e - hi) (:374-375) with zeros for the keys of the wave's
    other pixel (:376), one key tile (no rescale; attn_ref's T (2 R + 3) u Sv is granted and covers the 32-term hi + lo sum), `1.f / sum`
    and `oT * inv` (:372, :391): the numerics of attn_small_mfma_kernel, errbound.attn_ref + p_round = 2**-16.
    stages: GroupNorm -> dev -> qkv GEMM (K = 256) -> dev -> attention -> dev -> proj_out GEMM (K = 256) + bias + residual -> store.
    The front stage (pre = ...) is chained bitwise to the strip GEMM and to this block by
    tests/test_tattn_gpu.py::test_tattn_front_stage_is_the_spatial_proj_out and has no case here.

What the metric sees and what it does not (tests/test_errbound_fused_cpu.py proves both on fp32 emulations of the two chains)
    HOW SHARP.  The share of the plain store term v |ref| in the bound (median over a case's elements, CPU test, `-s`): VideoConv 0.5
    (Cin = 32) falling to 0.05 (Cin = 160) - K = 9 Cin enters the spatial e32, a larger e32 puts more T elements next to a midpoint, and
    each of those enters a 384-term temporal sum with a whole step; attention block 0.02 (0.28 on the offset case, where the residual
    dominates).  In the attention block the mask stops being sparse at O: about a quarter of the stored q / k elements carry a step
    (they are small where the step is small), 64 channels of them move a score by |da| ~ 8e-3, and eta (Sv + |out|) is then about one
    bf16 step of O itself, so nearly every O element is granted a step and proj_out adds 256 of them.  The bound is first order and
    finite - a blanket propagation is not - but it is a STRUCTURAL check there: every mask / border / statistics / operand-order defect
    below exceeds it 19 to 600 times, rounding-level defects of an intermediate do not reach it.
    FLAGGED on at least one case (VCONV_DEFECTS, TATTN_DEFECTS): padding normalised, a halo corner slot from the wrong pixel (the cases with
    an interior patch corner), temporal taps across the sample boundary, a non-zero zero frame, the previous chunk's affine, a
    truncating store (VideoConv: nine of eighteen launches; attention block: the offset case); the other pixel's keys unmasked, heads
    swapped in the projection, the neighbour's residual, the neighbour pixel's GroupNorm statistics.
    BLIND SPOTS, evaluated on every case and inside the bound:
      * attention block, row sum taken from the rounded P (TATTN_BLIND): it scales a head's O row by 1 + delta, |delta| <= v (the key at
        the maximum has e = 1 exactly and does not contribute) - at most half a step of O, behind a stage that is granted a whole one.  No
        test of the fused block sees it today; the same arithmetic is held element-wise in attn_small_mfma_kernel only
        (tests/test_elementwise_gpu.py::test_temporal_attention_elementwise), whose numerics this kernel restates (:369-375).
      * a DOUBLE rounding of an intermediate (`defect="double_round_T"`: T = bf16(bf16(acc) + bias_s); `"double_round_O"`:
        O = bf16(bf16(oT) * inv)).  VideoConv: flagged on the single-chunk case only (537 elements, ratio 3.3), inside the bound from
        Cin = 64 on - but about half of the output elements change their bits, so tests/test_vconv_gpu.py::test_vconv_vs_two_launch_path
        (> 97 % of the elements bitwise equal to the unfused path, which rounds once; its rel-L2 < 4e-3 alone would pass at 3e-3) sees it.
        Attention block: inside the bound on every case, 38 % of the output bits change, rel-L2 2.3e-3 from the clean chain: below
        the 4e-3 of tests/test_tattn_gpu.py::test_tattn_block_vs_torch_and_the_four_launch_path, which has no bitwise clause - not seen
        by any test today.
    No element is excluded from any check: neither kernel takes a hard decision on a rounded value.
"""
import math

import torch

import errbound as E
import errbound_bwd as B
import errbound_fwd as EF
from errbound import _f64

BF = torch.bfloat16
GN_EPS = B.GN_EPS
F = 16                                   # frames: both kernels are built for 16
C_T, HEADS = 256, 4                      # the attention block's width and heads
COUT = 128                               # the VideoConv's output width


# --------------------------------------------------------------------------- exact rounding, deviation
def _pow2(k):
    """2**k as float64 from an integer tensor, built from the exponent bits (exact; -1022 <= k <= 1023)."""
    return ((k.long() + 1023) << 52).view(torch.float64)


def rn_bf16(z):
    """Round-to-nearest-even to bf16 (8 significand bits, fp32's exponent range) straight from float64; the result is float64.
    |z| = m 2**e with 0.5 <= m < 1: the spacing of bf16 there is 2**(e - 8); below 2**-126 (e < -125) it stays 2**-133."""
    z = z.double()
    _, e = torch.frexp(z)
    e = e.clamp_min(-125)
    q = torch.round(z * _pow2(8 - e))                   # scaling by a power of two is exact; torch.round rounds halves to even
    out = q * _pow2(e - 8)
    assert bool((out.abs() < 3.4e38).all()), "rn_bf16: overflow"
    return out


def dev(z, D):
    """(s, d): s = rn_bf16(z) and the largest distance of rn_bf16(z') from s over |z' - z| <= D (module docstring)."""
    s = rn_bf16(z)
    Dw = D * (1 + 2.0 ** -40)
    d = torch.maximum((rn_bf16(z + Dw) - s).abs(), (rn_bf16(z - Dw) - s).abs())
    return s, d


def _gemm_stage(s, d, w, bias, residual, taps, dims):
    """One GEMM stage on the reference's stored operand s with deviation d (None: exact operand): (ref, D) in front of the store."""
    ref, S = E.conv_rows_ref(s, w, bias, residual, taps, dims)
    K = len(taps) * s.shape[1]
    if d is None:
        return ref, E.gemm_bound(ref, S, K, torch.float32)
    P, _ = E.conv_rows_ref(d, _f64(w).abs(), None, None, taps, dims)
    return ref, E.gemm_bound(ref, S + P, K, torch.float32) + P


# --------------------------------------------------------------------------- fused VideoConv
def vconv_ref(x, ws, wt, bs, bt, a, b, act, N, Hh, Ww, rounded=True):
    """x [N 16 H W, Cin] bf16, ws [128, 9 Cin] / wt [128, 384] bf16 GEMM matrices (K index = tap * Cin + ci), bs / bt [128] fp32,
    a / b [S, Cin] fp32 or None (S slices of whole samples), act: SiLU behind the affine.  Returns (ref, bound) float64 [M, 128].
    rounded=False: the chain without the restated roundings (the CPU test compares it with torch's own convolutions)."""
    M, Cin = x.shape
    rnd = dev if rounded else (lambda z, D: (z, torch.zeros_like(z)))
    if a is not None:
        S = a.shape[0]
        z0, D0 = EF.apply_ref(x.reshape(S, M // S, Cin), a, b, act, torch.float32)
        assert float(z0.abs().max()) < 40                # the validity range of the silu_f bound (errbound_fwd)
        s0, d0 = rnd(z0.reshape(M, Cin), D0.reshape(M, Cin))
    else:
        s0, d0 = _f64(x), None
    z1, D1 = _gemm_stage(s0, d0, ws, bs, None, E.TAPS_SPATIAL, (N * F, Hh, Ww))
    s1, d1 = rnd(z1, D1)
    z2, D2 = _gemm_stage(s1, d1, wt, bt, None, E.TAPS_TEMPORAL, (F, Hh * Ww, 1))
    return z2, EF._store(z2, D2, BF)


def _gather_fill(x, taps, dims, fill=None, remap=None):
    """errbound.conv_gather with the out-of-range slots holding fill [M, Cin] instead of zero, and remap(tap index, src, ok) ->
    (src, ok) to bend single slots (the seeded halo defects)."""
    M = x.shape[0]
    D0, D1, D2 = dims
    m = torch.arange(M)
    p2, p1, p0 = m % D2, (m // D2) % D1, (m // (D1 * D2)) % D0
    out = []
    for t, (d0, d1, d2) in enumerate(taps):
        ok = (p0 + d0 >= 0) & (p0 + d0 < D0) & (p1 + d1 >= 0) & (p1 + d1 < D1) & (p2 + d2 >= 0) & (p2 + d2 < D2)
        src = m + d0 * D1 * D2 + d1 * D2 + d2
        if remap is not None:
            src, ok = remap(t, src, ok)
        g = x[src.clamp(0, M - 1)] * ok[:, None].to(x.dtype)
        if fill is not None:
            g = g + fill * (~ok)[:, None].to(x.dtype)
        out.append(g)
    return out


VCONV_DEFECTS = ["pad_normalised", "corner_slot", "cross_sample", "zero_frame", "affine_next_chunk", "trunc"]


def emu_vconv(x, ws, wt, bs, bt, a, b, act, N, Hh, Ww, defect=None):
    """The kernel's chain in fp32 torch arithmetic with its three rounding points; K order (32-channel chunk, tap).  defect:
    'pad_normalised'    the in-place norm also transforms the padding slots: they hold act(b) instead of zero
    'corner_slot'       halo slot (hh, ww) = (0, 0) of a patch holds pixel (h0 - 1, w0) instead of (h0 - 1, w0 - 1)
    'cross_sample'      the temporal taps run over the sample boundary: frame -1 of sample n + 1 = frame 15 of sample n
    'zero_frame'        frames -1 / 16 of the T image went through the transition like every other row: they hold bf16(bias_s)
    'affine_next_chunk' the affine ring slot of chunk c is still in place when chunk c + 1 is normalised
    'trunc'             truncating output store
    'double_round_T'    T = bf16(bf16(acc) + bias_s) (the stated blind spot)."""
    M, Cin = x.shape
    HW = Hh * Ww
    xs = x.float()
    fill = None
    if a is not None:
        S = a.shape[0]
        af, bf = a.float(), b.float()
        if defect == "affine_next_chunk":
            assert Cin >= 64
            af, bf = torch.cat([af[:, :32], af[:, :-32]], 1), torch.cat([bf[:, :32], bf[:, :-32]], 1)
        ar, br = af.repeat_interleave(M // S, 0), bf.repeat_interleave(M // S, 0)
        w = xs * ar + br
        fn = EF._silu32 if act else (lambda t: t)
        xs = fn(w).to(BF).float()
        if defect == "pad_normalised":
            fill = fn(br).to(BF).float()
    remap = None
    if defect == "corner_slot":
        m = torch.arange(M)
        hit = ((m // Ww) % Hh % 4 == 0) & (m % Ww % 4 == 0) & ((m // Ww) % Hh > 0)

        def remap(t, src, ok):                            # tap 0 = (dh, dw) = (-1, -1) of a patch's first pixel: one column to the right
            return (torch.where(hit, src + 1, src), ok | hit) if t == 0 else (src, ok)
    g = _gather_fill(xs, E.TAPS_SPATIAL, (N * F, Hh, Ww), fill, remap)
    wsf = ws.float()
    acc = torch.zeros(M, COUT)
    for c in range(Cin // 32):
        for t in range(9):
            acc = acc + g[t][:, 32 * c:32 * c + 32] @ wsf[:, t * Cin + 32 * c:t * Cin + 32 * c + 32].t()
    if defect == "double_round_T":
        acc = acc.to(BF).float()
    T = (acc + bs.float()).to(BF).float()
    tfill = bs.float().to(BF).float().expand(M, COUT) if defect == "zero_frame" else None
    tdims = (N * F, HW, 1) if defect == "cross_sample" else (F, HW, 1)
    gt = _gather_fill(T, E.TAPS_TEMPORAL, tdims, tfill)
    wtf = wt.float()
    acc = torch.zeros(M, COUT)
    for t in range(3):
        acc = acc + gt[t] @ wtf[:, t * COUT:(t + 1) * COUT].t()
    y = acc + bt.float()
    return EF._trunc_bf16(y) if defect == "trunc" else y.to(BF)


def vconv_inputs(N, Hh, Ww, Cin, S, seed):
    """The operands of tests/test_vconv_gpu.py::make on a CPU generator, as GEMM matrices, with the affine offset b around 2: act(b) is
    then three orders above the bound, so a normalised padding slot is a violation at every border element."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(N * F * Hh * Ww, Cin).to(BF)
    ws = (rn(COUT, 9 * Cin) * (9 * Cin) ** -0.5).to(BF)
    wt = (rn(COUT, 3 * COUT) * (3 * COUT) ** -0.5).to(BF)
    bs, bt = rn(COUT), rn(COUT)
    a = torch.rand(S, Cin, generator=g) + 0.5
    b = 2.0 + 0.25 * rn(S, Cin)
    return x, ws, wt, bs, bt, a, b


# (name, N, H, W, Cin, S = GroupNorm slices, strided): a block is a 4 x 4 patch x 16 frames, Cin comes in 32-channel chunks
VCONV_CASES = [("1x4x4-c32", 1, 4, 4, 32, 1, False),          # one block: every border at once; a single chunk
               ("2x4x8-c96", 2, 4, 8, 96, 2, False),          # three chunks: the halo ring wraps, the split fetch crosses a chunk boundary; sample boundary
               ("1x12x12-c64", 1, 12, 12, 64, 1, False),      # 3 x 3 patches: an interior patch, all four edge and corner kinds
               ("2x8x12-c160", 2, 8, 12, 160, 2, False),      # non-square, odd chunk count
               ("2x4x8-c96-oneslice", 2, 4, 8, 96, 1, False),   # a single GroupNorm slice spanning both samples
               ("2x4x8-c96-strided", 2, 4, 8, 96, 2, True)]   # ldx > Cin, the output a column slice of a wider buffer
VCONV_GN = ["none", "affine", "silu"]


def vconv_case(name, gn):
    """(operands of emu_vconv / vconv_ref on the CPU: x, ws, wt, bs, bt, a, b, act, N, H, W).  The strided and the plain 2x4x8-c96 case
    share their operands (the seed depends on the geometry alone)."""
    _, N, Hh, Ww, Cin, S, _ = next(c for c in VCONV_CASES if c[0] == name)
    x, ws, wt, bs, bt, a, b = vconv_inputs(N, Hh, Ww, Cin, S, seed=Hh * Ww + Cin + S)
    if gn == "none":
        a = b = None
    return x, ws, wt, bs, bt, a, b, gn == "silu", N, Hh, Ww


# --------------------------------------------------------------------------- temporal attention block
def _heads(t, S):
    """[M, C] rows (n, f, pixel) -> [S = N HW sequences, heads, 16, ch] through the temporal slices."""
    return t.reshape(S, F, HEADS, -1).permute(0, 2, 1, 3)


def _attn_prop(q, k, v, dq, dk, dv, out):
    """Propagated deviation of the attention output (module docstring), all [S, heads, 16, ch]; returns (term, max_row sum p eta)."""
    sc = q.shape[-1] ** -0.5
    kt, dkt = k.abs().transpose(-1, -2), dk.transpose(-1, -2)
    da = sc * (dq @ kt + q.abs() @ dkt + dq @ dkt)
    eta = torch.expm1(da)
    p = torch.softmax(sc * q @ k.transpose(-1, -2), dim=-1)
    pe = p * eta
    spe = pe.sum(-1, keepdim=True)
    term = (pe @ v.abs() + out.abs() * spe) / (1 - spe) + (p * (1 + eta)) @ dv
    return term, float(spe.max())


def tattn_ref(x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW, rounded=True):
    """x [N 16 HW, 256] bf16 rows (n, f, pixel), wqkv [768, 256], wproj [256, 256] bf16, the rest fp32.  Returns (ref, bound, validity):
    float64 [M, 256] and the largest sum_j p eta of the case (asserted < 1/2).  rounded=False: the chain without the restated
    roundings (the CPU test compares it with torch's own operators)."""
    M, C = x.shape
    rnd = dev if rounded else (lambda z, D: (z, torch.zeros_like(z)))
    slices, _ = B.gn_slices("temporal", N, F, HW)
    S = slices.shape[0]
    sl = slices.to(x.device)
    g = EF.two_pass_ref(x, gamma, beta, None, slices, False, torch.float32, "small")
    n1, dn = rnd(g["y"], g["e_y"])
    zq, Dq = _gemm_stage(n1, dn, wqkv, bqkv, None, E.TAPS_1, (1, 1, 1))
    qkv, dqkv = rnd(zq, Dq)
    zo, Do = torch.empty(M, C, dtype=torch.float64, device=x.device), torch.empty(M, C, dtype=torch.float64, device=x.device)
    for i in range(S):                                     # own arithmetic term: errbound.attn_ref per sequence, eP + e32 of attn_bound
        r = qkv[sl[i]]
        ref, Sv, e32 = E.attn_ref(r[:, :C], r[:, C:2 * C], r[:, 2 * C:], HEADS)
        zo[sl[i]], Do[sl[i]] = ref, 2.0 ** -16 * Sv + e32
    parts = lambda t: [_heads(t[sl][..., j * C:(j + 1) * C], S) for j in range(3)]     # q | k | v thirds, each [S, heads, 16, ch]
    (q, k, v), (dq, dk, dv) = parts(qkv), parts(dqkv)
    term, validity = _attn_prop(q, k, v, dq, dk, dv, _heads(zo[sl], S))
    assert validity < 0.5, f"sum_j p eta = {validity}: the propagation formula needs < 1/2"
    prop = torch.empty_like(zo)
    prop[sl] = term.permute(0, 2, 1, 3).reshape(S, F, C)
    o, do = rnd(zo, Do + prop)
    zy, Dy = _gemm_stage(o, do, wproj, bproj, x, E.TAPS_1, (1, 1, 1))
    return zy, EF._store(zy, Dy, BF), validity


TATTN_DEFECTS = ["unmasked", "heads_swapped", "residual_neighbour", "gn_neighbour", "rowsum_rounded", "trunc"]
TATTN_BLIND = ["rowsum_rounded"]                   # evaluated and inside the bound on every case (module docstring)


def _row16(t):
    """ta_row16_total over the frame axis (dim 1 of [S, 16, ...]): v += ror 8, 4, 2, 1; every lane ends with the same tree."""
    for o in (8, 4, 2, 1):
        t = t + torch.roll(t, o, 1)
    return t


def emu_tattn(x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW, defect=None):
    """The kernel's chain in fp32 torch arithmetic with its rounding points and its summation orders in the GroupNorm.  defect:
    'unmasked'            the keys of the wave's other pixel take part in the softmax and in P V
    'heads_swapped'       heads 1 and 2 of O swapped in the projection's K order
    'residual_neighbour'  the residual is read from the next row
    'gn_neighbour'        the odd pixel of a wave is normalised with the even pixel's statistics
    'rowsum_rounded'      the row sum is taken from the rounded P (hi only)
    'trunc'               truncating output store
    'double_round_O'      O = bf16(bf16(oT) * inv) (the stated blind spot)."""
    M, C = x.shape
    ch = C // HEADS
    slices, _ = B.gn_slices("temporal", N, F, HW)
    S = slices.shape[0]
    xs = x.float()[slices].reshape(S, F, 32, 8)
    s = ((xs[..., 0] + xs[..., 1]) + (xs[..., 2] + xs[..., 3])) + ((xs[..., 4] + xs[..., 5]) + (xs[..., 6] + xs[..., 7]))
    mean = _row16(s) * (1.0 / 128.0)                                                  # [S, 16, 32], equal along the frames
    if defect == "gn_neighbour":
        mean = mean.clone()
        mean[1::2] = mean[0::2]
    d = xs - mean[..., None]
    rstd = torch.rsqrt(_row16(EF._chain_sum(d * d)) * (1.0 / 128.0) + GN_EPS)
    if defect == "gn_neighbour":
        rstd = rstd.clone()
        rstd[1::2] = rstd[0::2]
    av = rstd[..., None] * gamma.float().reshape(32, 8)
    bv = beta.float().reshape(32, 8) - mean[..., None] * av
    n1 = (xs * av + bv).reshape(S, F, C).to(BF).float()
    qkv = (n1 @ wqkv.float().t() + bqkv.float()).to(BF).float()                       # [S, 16, 3 C]
    hd = lambda t: t.reshape(S, F, HEADS, ch).permute(0, 2, 1, 3)                     # [S, heads, 16, ch]
    q, k, v = hd(qkv[..., :C]), hd(qkv[..., C:2 * C]), hd(qkv[..., 2 * C:])
    if defect == "unmasked":                                                          # a wave = pixels (2 w, 2 w + 1): 32 keys
        pair = lambda t: t.reshape(S // 2, 2, HEADS, F, ch).permute(0, 2, 1, 3, 4).reshape(S // 2, 1, HEADS, 2 * F, ch).expand(-1, 2, -1, -1, -1).reshape(S, HEADS, 2 * F, ch)
        k, v = pair(k), pair(v)
    sT = q @ k.transpose(-1, -2)
    sc = torch.tensor(1.44269504088896 / math.sqrt(ch), dtype=torch.float32)
    mx = sT.amax(-1, keepdim=True)
    arg = (sT.double() * sc.double() - (mx * sc).double()).float()                    # one fma
    e = torch.exp2(arg)
    hi = e.to(BF).float()
    lo = (e - hi).to(BF).float()
    inv = 1.0 / (hi if defect == "rowsum_rounded" else e).sum(-1, keepdim=True)
    oT = hi @ v + lo @ v
    if defect == "double_round_O":
        oT = oT.to(BF).float()
    o = (oT * inv).to(BF).float().permute(0, 2, 1, 3).reshape(S, F, C)
    if defect == "heads_swapped":
        o = torch.cat([o[..., :ch], o[..., 2 * ch:3 * ch], o[..., ch:2 * ch], o[..., 3 * ch:]], -1)
    O = torch.empty(M, C)
    O[slices] = o
    res = x.float()
    if defect == "residual_neighbour":
        res = res[(torch.arange(M) + 1).clamp_max(M - 1)]
    y = (O @ wproj.float().t() + bproj.float()) + res
    return EF._trunc_bf16(y) if defect == "trunc" else y.to(BF)


def tattn_inputs(N, HW, seed, qk_scale=1.0, offset=0.0):
    """The operands of tests/test_tattn_gpu.py::_case on a CPU generator: per-pixel scales and offsets, so the two pixels of a wave
    differ.  qk_scale multiplies the q and k rows of the qkv weight and bias: the scores grow with its square (the spike case).
    offset is added to the 0.5 std of the per-(pixel, channel) offsets: at 32 the residual is two orders above the attention branch
    and the store term v |y| is the largest term of the bound - the case on which a truncating store shows."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    C = C_T
    x = rn(N, F, HW, C)
    x = x * (0.5 + torch.rand(N, 1, HW, 1, generator=g)) + (0.5 + offset) * rn(N, 1, HW, C)
    x = x.reshape(N * F * HW, C).to(BF)
    wqkv = rn(3 * C, C) * C ** -0.5
    wproj = (rn(C, C) * C ** -0.5).to(BF)
    bqkv = 0.3 * rn(3 * C)
    wqkv[:2 * C] *= qk_scale
    bqkv[:2 * C] *= qk_scale
    bproj = 0.3 * rn(C)
    gamma = 1 + 0.2 * rn(C)
    beta = 0.2 * rn(C)
    return x, wqkv.to(BF), wproj, bqkv, bproj, gamma, beta


# (name, N, HW, qk_scale, offset, strided): a workgroup is 128 rows = 8 pixels, a wave 2 pixels
TATTN_CASES = [("1x8", 1, 8, 1.0, 0.0, False),               # one workgroup
               ("3x8", 3, 8, 1.0, 0.0, False),               # a sample boundary at every workgroup
               ("1x40", 1, 40, 1.0, 0.0, False),             # five workgroups, the last one full
               ("2x24", 2, 24, 1.0, 0.0, False),             # mixed
               ("2x8-spike", 2, 8, 3.0, 0.0, False),         # q, k three times larger: scores nine times, one key dominates a row
               ("2x8-offset", 2, 8, 1.0, 32.0, False),       # the residual dominates: the store term is the largest of the bound
               ("2x24-strided", 2, 24, 1.0, 0.0, True)]      # input and output column slices of wider buffers


def tattn_case(name):
    """(operands of emu_tattn / tattn_ref on the CPU: x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW)."""
    _, N, HW, qk, off, _ = next(c for c in TATTN_CASES if c[0] == name)
    return tattn_inputs(N, HW, 100 * N + HW, qk, off) + (N, HW)
