"""Element-wise error bounds for the rest of the FORWARD path against float64 references: the GroupNorm kernels of mmd_norm.hip, the
layout-edge convolutions and bilinear_concat of mmd_edge.hip, resample and the statistics records (test infrastructure; plain torch,
no import of the package under test).  Notation and house rules are those of tests/errbound.py and tests/errbound_bwd.py:
u = 2**-24, v = 2**-8, every bound first order in u and v, every reference float64 on the STORED operands, `errbound.check` admits zero
violating elements.  Sums: this file uses the DEPTH form, depth * u * sum|terms|, depth = the longest chain of fp32 additions a term
passes through in the kernel as written (each addition rounds a partial sum that is bounded by sum|terms|, and a term is touched by
at most `depth` of them); the any-order form (n - 1) u sum|terms| is vacuous for a block reduction over 16k elements.

apply step (`apply_ref`; gn_apply_kernel :278-282, gn_small_kernel :379-383, gn_group_kernel :630-639, all `w = f * a + b`, `silu_f(w)`)
    w = x a + b is one rounding (fma under -ffp-contract=fast) or two; two are granted, the e_v of errbound_bwd:
        e_w  = |x| e_a + e_b + 2 u (|x a| + |b|)           (e_a = e_b = 0 when a, b are the stored fp32 tensors: gn_apply)
    silu_f (mmd_common.h: `x * rcp(1 + __expf(-x))`): __expf multiplies the argument by log2(e) (one rounding, u |w| absolute in the
    exponent), v_exp_f32 is accurate to 1 ulp = 2 u, the add of 1 rounds once, v_rcp_f32 is accurate to 1 ulp = 2 u, the product once.
    That is errbound_bwd's e_sg with e_v = e_w, and then
        e_y  = |w| e_sg + sg e_w + u |y|                   (y = w sg;  without SiLU e_y = e_w)
    store: fp32 as is; bf16 ONE round-to-nearest (Elt<__bf16>::pack, the `(__bf16)o[e]` of gn_group_kernel): v (|ref| + e_y) + e_y.
    Truncation costs up to 2 v, SiLU of the bf16-rounded affine a second v |w| |d silu / dw|: both exceed the bound where the element
    lies near a rounding midpoint (proven on the CPU for every family, tests/test_errbound_fwd_cpu.py).
    Validity: |w| < 87 (beyond it __expf(-w) overflows and the kernel returns -0 where float64 gives -1e-36); the cases stay below 40.

two-pass statistics in fp32 (`two_pass_ref`; gn_small_kernel :315-363, gn_group_kernel :586-599)
    mean = fl(fl(sum x) inv_cnt), inv_cnt = 1.f / (cpg Tn) (one rounding, the product another), with Sx = sum |x| over the cnt elements:
        e_mean = D u Sx / cnt + 2 u |mean|
    var: d = x - mean_c is rounded once, d * d once (or fused into the add), the sum has depth D, the scaling two roundings; the sum of
    (x - mean_c)^2 over the group equals cnt (var + (mean - mean_c)^2) EXACTLY (the cross term vanishes), so the mean's error enters
    in second order only - kept, because at mean = 20 std it is of the size of u var:
        e_var  = e_mean^2 + (D + 5) u (var + e_mean^2)
    rstd: gn_small `rsqrtf(a * inv_cnt + eps)` :363 - the add of eps one rounding, rsqrtf 1 ulp = 2 u; gn_group
    `(float)(1.0 / sqrt((double)var + (double)eps))` :599 - one rounding in all:
        e_rstd = rstd^3 (e_var + n_add u (var + eps)) / 2 + n_r u rstd        (small: n_add = 1, n_r = 2;  group: n_add = 0, n_r = 1)
    depth D
        gn_small: the thread adds its quad's 4 Tn elements one after the other (:318-324), then qpg quads one after the other
                  (:337, :362):  D = 4 Tn + qpg                                                      (at most 64 + 16)
        gn_group: (f0 + f1) + (f2 + f3) = 2, the thread's 16 items in a chain (:588, :593-597) = 16, wave_sum's six butterfly steps,
                  the LDS fold (s0 + s1) + (s2 + s3) = 2:  D = 26, whatever the size of the group (items <= 4096).
    a, b and FiLM: errbound_bwd.gn_affine (the shared arithmetic, gn_group :602-608; gn_small :367-368 has no FiLM), then the apply step
    with those e_a, e_b.  x a + b cancels when |mean| is large against std; the bound grants the roundings of both large terms and
    |x| e_a + e_b in the worst case, as the kernels compute it.
    mr_out (gn_group :615-618, read by the backward): mean, rstd against e_mean, e_rstd.

gn_finalize_stats, stage-wise (`finalize_ref`; gn_finalize_rec_kernel :470-529)
    The records are given fp32 tensors; the kernel sums them in double (:499-509) and takes var = E[x^2] - mean^2 in double (:512): the
    reference does the same sums in float64, so the bound on mean and rstd holds the double arithmetic (n + 4 roundings of 2**-53 on
    E[x^2] + mean^2, n = nrec * qpg terms; 1e-9 of the rest) and ONE fp32 conversion each (:514):
        e_mean = u |mean|,   e_var = (n + 4) 2**-53 (E[x^2] + mean^2),   e_rstd = rstd^3 e_var / 2 + u rstd
    then errbound_bwd.gn_affine (:519-525).  What this bound cannot see: how far the records themselves are from the tensor they
    summarise (the producers' fp32 sums and the (1 + mean^2 / var) cancellation) - that is the chain producer -> records -> finalize,
    `chain_ref` below.  A variance taken in fp32 from E[x^2] - mean^2 at mean = 8 std is wrong by 65 u relative and is flagged.

add_rowbias (`rowbias_ref`; add_rowbias_kernel :401-405): one fp32 add, one store: fp32 u |ref|; bf16 v (|ref| + u |ref|) + u |ref|.

Host-side selection rules, restated with their lines (the library does not report which path a launch took):
    `gn_rows_per_block` / `nchunks` (mmd_norm.hip:418-429, :446-448), `gn_apply_R` (:672-674), `gn_small_spb` (:704-706),
    `thread_shape` (gn_apply_kernel :246-248 = gn_partial_kernel :51-54: column passes, row lanes, idle threads).
tests/test_errbound_fwd_cpu.py asserts that the case lists below reach every variant named in VARIANTS.

layout-edge convolutions (`edge_ref`; mmd_edge.hip: stem_conv_kernel, stem_conv_strip_kernel, stem_conv_mfma_kernel, head_conv_kernel,
head_conv_coop_kernel, head_conv_strip_kernel)
    Both are errbound.conv_rows_ref on rows with the 3-D tap list and dims (F, H, W): the stem on the fp32 API-layout input
    [N, F, Cin, H, W] viewed as rows (`api_to_rows`), the head on the stored rows with its fp32 API-layout output viewed as rows.  Bound:
    errbound.gemm_bound with K = ntaps * Cin, the any-order form: the kernels add K fp32 products (each rounded once, or fused) and
    the bias in orders of their own - the per-pixel and strip kernels in tap order from the bias (:33-41, :75-115), the MFMA stem two
    products per instruction and the bias after the half-wave swap (:230, :247-251), the cooperative head kernels EPV * ntaps terms per
    lane, log2(LPR) xor-shuffle steps, then the bias (:362, :371, :376; :452, :462, :468) - and K + 2 covers every one of them.  The
    stem stores T with one rounding (Elt<T>::pack), the head stores fp32.
    Which kernel a launch takes: `stem_variant` (mmd_stem_conv :291-301 with stem_mfma_ok :259-265: the MFMA kernel packs a tap offset
    + 1 into two bits, so it takes offsets in [-1, 1] only - the 5-tap list (0, 0, -2 .. 2) goes to the strip kernel; the head kernels
    take arbitrary offsets) and `head_variant` (launch_head :514-546: strip, then coop, then plain, each with its LDS limit).
    Not reached: the plain head kernel's second grid-stride pass (more than 8192 * 256 = 2 M rows).

resample (`resample_ref`; mmd_misc.hip: resample_kernel :88-112): the pool adds its fh fw rows one after the other ((n - 1) u sum |x|),
    inv = scale / (fh fw) is rounded once and the product once: e = (n - 1) u |inv| sum |x| + 2 u |ref|, then the store.  The nearest
    upsample at scale 1 copies 16-byte vectors (torch.equal); at another scale one product, u |ref|, and the store.
records (`records_ref`, `check_records`): see `records_ref`; every (64-row record, channel quad) pair has its own bound.
bilinear_concat(_rows) (`bilinear_ref`): see `bilinear_ref`; the x half is a copy (rows in bf16: x rounded once), columns [2C, Cpad) zero.

chain producer -> records -> gn_finalize_stats (`chain_ref`): see `chain_ref`, which also states where its bound on `a` passes 2**-9.

head_gemm + head_gather (`head_gemm_ref`, `head_gather_ref`; mmd_edge.hip: head_gemm_kernel :566-635, head_gather_kernel :642-675), Cin = 128 bf16,
three levels:
    P against float64 from the stored x, a, b and the fp32 weights.  The kernel takes s = silu_f(x a + b) in fp32 (:602-603, the apply
    step above: e_y) and rounds it ONCE to bf16 where gn_apply would store it (:606): e_s = v (|s| + e_y) + e_y, which is `apply_ref`
    with a bf16 store.  The weights enter as the (hi, lo) bf16 pair of ops.head_gemm_pack; the residual r = W - hi - lo is read off the
    packed image (|r| <= 2**-18 |W|: two roundings of 2**-9 relative).  bf16 x bf16 products are exact in fp32; the MFMA chain adds
    2 * 128 of them (:617-622) in an order of its own: the any-order form with 256 terms.  With Sw = sum_ci (|hi| + |lo|) (|s| + e_s):
        e_P = sum_ci |W| e_s + sum_ci |r| (|s| + e_s) + 255 u Sw
    BLIND SPOT: e_P is dominated by sum |W| v |s|, the granted activation rounding (2**-9 relative per term), and a DROPPED lo half
    changes P by sum |lo| |s| <= 2**-9 sum |W| |s| - the same order.  This bound cannot see it (tests/test_errbound_fwd_cpu.py
    evaluates it: the defect stays inside e_P).  The check that sees it is test_round5_gpu.py::test_head_gemm_gather,
    rel_l2(y, gn_apply + head_conv) < 2e-5: both paths round the SAME activations, so the rounding cancels and 2**-9 of the weights shows.
    y against float64 from the STORED P: bias + ntaps terms, each multiplied by an exact 0 or 1 (:663, :670), ntaps fp32 additions in
    tap order from the bias: the any-order form  e_y = ntaps u (|bias| + sum_taps |P|).
    End to end: the float64 tap sum of the float64 P, with the tap sum of e_P added to the gather's own bound (taken on |P| + e_P).
    NO = ntaps * Co in {27, 33, 54, 81, 96, 36}: every `ob` break (:612) and the `o < NO` guard (:630); slices of 128 and 384 rows; and
    one launch of 1025 row groups, where per_block = 2 (:694) and every second block changes its slice (:585-591).

chain producers: conv_gemm tiles 64 / 128 / 129 / 131, gn_conv1x1 (tiled loader) and resample with stats= (`CHAIN_CASES`).
"""
import itertools

import torch

import errbound as E
import errbound_bwd as B
from errbound import U16, U32, _f64

GN_EPS = B.GN_EPS
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U64 = 2.0 ** -53


def _cdiv(a, b):
    return -(-a // b)


def epv(dt):
    return 8 if dt == "bf16" else 4


# --------------------------------------------------------------------------- host-side selection rules
def thread_shape(dt, C):
    """(column passes, row lanes RPP, idle threads of the 256) of gn_apply_kernel / gn_partial_kernel (mmd_norm.hip:246-248)."""
    cv = C // epv(dt)
    cvb = min(cv, 256)
    rpp = 256 // cvb
    return _cdiv(cv, 256), rpp, 256 - rpp * cvb


def gn_rows_per_block(dt, C, Tn, cap=1280):
    """mmd_norm.hip:418-429 (MMD_GN_BLOCKS unset)."""
    cv = C // epv(dt)
    R = 4 * max(1, 256 // cv)
    while _cdiv(Tn, R) > cap // 4 and R < 1024:
        R *= 2
    return R


def nchunks(dt, C, Tn):
    """mmd_gn_stats :446-448: 1 = gn_partial_kernel<T, true> alone, more = partial + gn_finalize_kernel."""
    return _cdiv(Tn, gn_rows_per_block(dt, C, Tn))


def gn_apply_R(dt, C, S, Tn):
    """mmd_gn_apply :672-674: (R, number of doublings)."""
    R0 = R = 4 * max(1, 256 // (C // epv(dt)))
    while S * _cdiv(Tn, R) > 4096 and R < 4096:
        R *= 2
    return R, (R // R0).bit_length() - 1


def gn_small_spb(dt, C):
    """mmd_gn_small :704-706: (slices per block, threads of the 256 that are never `live`)."""
    cv = C // epv(dt)
    spb = 256 // cv
    return spb, 256 - spb * cv


def gn_small_ok(dt, C, Tn):
    """mmd_gn_small :700-702."""
    return Tn <= 16 and C % 128 == 0 and C // epv(dt) <= 256


def gn_group_ok(C, Tn, ld):
    """mmd_gn_group :652-655."""
    return C % 128 == 0 and C <= 2048 and Tn * (C // 128) <= 4096 and ld % 4 == 0


# --------------------------------------------------------------------------- references and bounds
def _store(ref, e, out_dtype):
    return e if out_dtype == torch.float32 else U16 * (ref.abs() + e) + e


def apply_ref(xs, a, b, act, out_dtype, e_a=None, e_b=None):
    """y = act(x a + b) in float64 and its bound.  xs [S, Tn, C] (the stored x by slice), a, b [S, C]; e_a / e_b: bounds of the
    COMPUTED a, b against the float64 a, b given here (None: a, b are the stored tensors the kernel reads)."""
    xs, a, b = _f64(xs), _f64(a)[:, None], _f64(b)[:, None]
    w = xs * a + b
    e_w = 2 * U32 * ((xs * a).abs() + b.abs())
    if e_a is not None:
        e_w = e_w + xs.abs() * e_a[:, None] + e_b[:, None]
    if not act:
        return w, _store(w, e_w, out_dtype)
    sg = torch.sigmoid(w)
    e_sg = sg * ((1 - sg) * (e_w + U32 * w.abs() + 2 * U32) + 3 * U32)               # errbound_bwd: e_sg with e_v = e_w
    y = w * sg
    e_y = w.abs() * e_sg + sg * e_w + U32 * y.abs()
    return y, _store(y, e_y, out_dtype)


def scatter(vals, slices, rows):
    """[S, Tn, C] by slice -> [rows, C] (every row belongs to exactly one slice)."""
    out = torch.full((rows, vals.shape[-1]), float("nan"), dtype=vals.dtype, device=vals.device)
    out[slices.to(vals.device)] = vals
    return out


def two_pass_ref(x, gamma, beta, film, slices, act, out_dtype, kernel):
    """gn_small / gn_group end to end from the stored x, gamma, beta, film: dict of float64 y [rows, C], a, b [S, C], mean, rstd [S, 32]
    and their bounds e_* (module docstring).  kernel: 'small' | 'group'."""
    x, gamma, beta, film = _f64(x), _f64(gamma), _f64(beta), _f64(film)
    S, Tn = slices.shape
    C = x.shape[1]
    cpg = C // 32
    cnt = Tn * cpg
    xs = x[slices.to(x.device)]
    xg = xs.reshape(S, Tn, 32, cpg)
    mean = xg.mean((1, 3))
    dev = xg - mean[:, None, :, None]
    var = (dev * dev).mean((1, 3))
    rstd = (var + GN_EPS).rsqrt()
    D = 4 * Tn + cpg // 4 if kernel == "small" else 26
    n_add, n_r = (1, 2) if kernel == "small" else (0, 1)
    e_mean = D * U32 * xg.abs().sum((1, 3)) / cnt + 2 * U32 * mean.abs()
    e_var = e_mean ** 2 + (D + 5) * U32 * (var + e_mean ** 2)
    e_rstd = rstd ** 3 * (e_var + n_add * U32 * (var + GN_EPS)) / 2 + n_r * U32 * rstd
    a, b, e_a, e_b = B.gn_affine(mean, rstd, e_mean, e_rstd, gamma, beta, film)
    y, e_y = apply_ref(xs, a, b, act, out_dtype, e_a, e_b)
    rows = slices.numel()
    return dict(y=scatter(y, slices, rows), e_y=scatter(e_y, slices, rows), a=a, b=b, e_a=e_a, e_b=e_b, mean=mean, rstd=rstd,
                e_mean=e_mean, e_rstd=e_rstd)


def finalize_ref(rec, C, S, Tn, gamma, beta, film):
    """gn_finalize_stats from the given fp32 records rec [S * Tn / 64, C / 4, 2] (sum, sum of squares per 64 rows and channel quad)."""
    rec, gamma, beta, film = _f64(rec), _f64(gamma), _f64(beta), _f64(film)
    nrec, cpg = Tn // 64, C // 32
    qpg = cpg // 4
    r = rec.reshape(S, nrec, 32, qpg, 2)
    cnt = Tn * cpg
    mean = r[..., 0].sum((1, 3)) / cnt
    ex2 = r[..., 1].sum((1, 3)) / cnt
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = (var + GN_EPS).rsqrt()
    e_mean = U32 * mean.abs()
    e_var = (nrec * qpg + 4) * U64 * (ex2.abs() + mean * mean)
    e_rstd = rstd ** 3 * e_var / 2 + U32 * rstd
    a, b, e_a, e_b = B.gn_affine(mean, rstd, e_mean, e_rstd, gamma, beta, film)
    return dict(a=a, b=b, e_a=e_a, e_b=e_b, mean=mean, rstd=rstd, e_mean=e_mean, e_rstd=e_rstd)


def rowbias_ref(x, e, rows_per_sample, out_dtype):
    x, e = _f64(x), _f64(e)
    ref = x + e.repeat_interleave(rows_per_sample, dim=0)
    return ref, _store(ref, U32 * ref.abs(), out_dtype)


# --------------------------------------------------------------------------- emulations (fp32 torch arithmetic, the kernel's order)
def _trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _silu32(w):
    return w * (1.0 / (1.0 + torch.exp(-w)))


def emu_apply(xs, a, b, act, out_dtype, defect=None):
    """gn_apply on xs [S, Tn, C] with fp32 a, b [S, C].  defect: None | 'trunc' | 'double_round' | 'next_affine' | 'first_pass_ab'."""
    xs, a, b = xs.float(), a.float()[:, None].expand(-1, xs.shape[1], -1), b.float()[:, None].expand(-1, xs.shape[1], -1)
    if defect == "next_affine":                     # the last row of each slice normalised with the next slice's affine
        a, b = a.clone(), b.clone()
        a[:-1, -1], b[:-1, -1] = a[1:, 0], b[1:, 0]
    if defect == "first_pass_ab":                   # channels >= 1024 of an fp32 row take a / b from the first column pass
        a, b = a.clone(), b.clone()
        n = a.shape[-1] - 1024
        assert n > 0
        a[..., 1024:], b[..., 1024:] = a[..., :n], b[..., :n]
    w = xs * a + b
    if defect == "double_round":
        w = w.to(out_dtype).float()
    y = _silu32(w) if act else w
    return _trunc_bf16(y) if defect == "trunc" and out_dtype == torch.bfloat16 else y.to(out_dtype)


def _chain_sum(t):
    """Sum over the last dimension, one fp32 addition after the other."""
    acc = torch.zeros_like(t[..., 0])
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def _block_sum_group(t):
    """gn_group_kernel's block reduction of per-element terms t [S, 32, items, 4] (zero past `items`): item i sits in thread i % 256,
    slot i // 256; the thread's chain over (t0 + t1) + (t2 + t3), a 64-lane butterfly, the fold of the four waves."""
    S, G, items, _ = t.shape
    pad = torch.zeros(S, G, 4096 - items, 4, dtype=t.dtype)
    t = torch.cat([t, pad], 2).reshape(S, G, 16, 256, 4)
    q = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    v = _chain_sum(q.transpose(2, 3)).reshape(S, G, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def emu_two_pass(x, gamma, beta, film, slices, act, out_dtype, kernel, defect=None):
    """gn_small / gn_group in fp32, sums in the kernel's order.  defect: None | 'unbiased' | 'count16' | 'no_eps' | 'trunc' |
    'double_round'.  Returns dict(y [rows, C] in out_dtype, a, b [S, C], mean, rstd [S, 32] fp32)."""
    S, Tn = slices.shape
    C = x.shape[1]
    cpg = C // 32
    qpg = cpg // 4
    xs = x[slices].float()
    one = torch.ones((), dtype=torch.float32)
    n_rows = 16 if defect == "count16" else Tn
    inv_cnt = one / (torch.tensor(float(cpg)) * torch.tensor(float(n_rows)))
    inv_var = one / torch.tensor(float(cpg * n_rows - 1)) if defect == "unbiased" else inv_cnt
    eps = 0.0 if defect == "no_eps" else GN_EPS
    if kernel == "small":
        quads = lambda t: t.reshape(S, Tn, 32 * qpg, 4).permute(0, 2, 1, 3).reshape(S, 32, qpg, Tn * 4)
        red = lambda t: _chain_sum(_chain_sum(quads(t)))
        mean = red(xs) * inv_cnt
        d = xs - mean.repeat_interleave(cpg, 1)[:, None]
        var = red(d * d) * inv_var
        rstd = torch.rsqrt(var + eps)
    else:
        items = lambda t: t.reshape(S, Tn, 32, qpg, 4).permute(0, 2, 1, 3, 4).reshape(S, 32, Tn * qpg, 4)
        mean = _block_sum_group(items(xs)) * inv_cnt
        d = xs - mean.repeat_interleave(cpg, 1)[:, None]
        var = _block_sum_group(items(d * d)) * inv_var
        rstd = (1.0 / torch.sqrt(var.double() + eps)).float()
    rep = lambda t: t.repeat_interleave(cpg, 1)
    a = rep(rstd) * gamma.float()
    b = beta.float() - rep(mean) * a
    if film is not None:
        sc = 1.0 + film[:, :C].float()
        a = a * sc
        b = b * sc + film[:, C:].float()
    y = emu_apply(xs, a, b, act, out_dtype, defect if defect in ("trunc", "double_round") else None)
    return dict(y=scatter(y, slices, slices.numel()), a=a, b=b, mean=mean, rstd=rstd)


def emu_finalize(rec, C, S, Tn, gamma, beta, film, defect=None):
    """gn_finalize_rec_kernel: double sums, fp32 mean / rstd, fp32 affine.  defect: None | 'drop_last_record' | 'fp32_var'."""
    nrec, cpg = Tn // 64, C // 32
    r = rec.double().reshape(S, nrec, 32, cpg // 4, 2)
    if defect == "drop_last_record":
        r = r[:, :nrec - 1] if nrec > 1 else r * 0
    cnt = float(Tn * cpg)
    mean = r[..., 0].sum((1, 3)) / cnt
    ex2 = r[..., 1].sum((1, 3)) / cnt
    if defect == "fp32_var":
        var = (ex2.float() - mean.float() * mean.float()).clamp_min(0).double()
    else:
        var = (ex2 - mean * mean).clamp_min(0)
    mean_f, rstd_f = mean.float(), (1.0 / torch.sqrt(var + GN_EPS)).float()
    rep = lambda t: t.repeat_interleave(cpg, 1)
    a = rep(rstd_f) * gamma.float()
    b = beta.float() - rep(mean_f) * a
    if film is not None:
        sc = 1.0 + film[:, :C].float()
        a = a * sc
        b = b * sc + film[:, C:].float()
    return dict(a=a, b=b, mean=mean_f, rstd=rstd_f)


def emu_rowbias(x, e, rows_per_sample):
    return (x.float() + e.float().repeat_interleave(rows_per_sample, dim=0)).to(x.dtype)


# --------------------------------------------------------------------------- inputs (CPU generator: the CPU proof and the GPU file share them)
def gn_inputs(dt, C, kind, N, Tn, HW, big, seed, film=None, std=1.5):
    """x [rows, C] in the stored dtype (mean `big` std, or 0.3 / 1.5), gamma, beta fp32, film [S, 2C] or None, slices, geometry."""
    g = torch.Generator().manual_seed(seed + 7 * C + Tn)
    slices, geom = B.gn_slices(kind, N, Tn, HW)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(slices.numel(), C) * (1.0 if big else std) + (float(big) if big else 0.3)).to(DT[dt])
    gamma, beta = 1 + 0.1 * rn(C), rn(C)
    use_film = kind == "per_sample_film" if film is None else film
    fl = rn(geom[0], 2 * C) * 0.3 if use_film else None
    return x, gamma, beta, fl, slices, geom


def apply_inputs(dt, C, kind, N, Tn, HW, big, seed=21):
    """gn_apply's operands: x and the float64 GroupNorm affine of x rounded to fp32 - the STORED a, b the kernel reads."""
    x, gamma, beta, film, slices, geom = gn_inputs(dt, C, kind, N, Tn, HW, 20.0 if big else 0.0, seed)
    f = B.gn_fwd_ref(x, gamma, beta, film, slices)
    return x, f["a"].float(), f["b"].float(), slices, geom


def apply_cases():
    """(name, dt, C, kind, N, Tn, HW, big, strided): every entry of errbound_bwd.gn_cases() (N = 2, HW = 3), column slices with
    ldx != ldy, and the R-doubling geometry (S = 4100 temporal slices of 5 rows)."""
    cases = [(f"{dt}-{C}-{kind}-{Tn}-{int(big)}", dt, C, kind, 2, Tn, 3, big, False) for dt, C, kind, Tn, big in B.gn_cases()]
    for dt, C in (("bf16", 96), ("f32", 1056), ("bf16", 2048), ("f32", 96)):
        cases.append((f"{dt}-{C}-strided", dt, C, "temporal", 2, 7, 3, False, True))
    for dt in ("bf16", "f32"):
        cases.append((f"{dt}-256-Rdouble", dt, 256, "temporal", 2, 5, 2050, False, False))
    return cases


def small_cases():
    """(name, dt, C, kind, N, Tn, HW, big): temporal geometry with S = 3 * 7 = 21 slices (a multiple of no spb above 1), one contiguous
    geometry per dtype, one group mean of 20 std per dtype."""
    cases = []
    for dt, widths in (("bf16", (128, 384, 1024, 2048)), ("f32", (128, 384, 1024))):
        for C in widths:
            for Tn in (1, 5, 16):
                cases.append((f"{dt}-{C}-temporal-{Tn}", dt, C, "temporal", 3, Tn, 7, 0.0))
        cases.append((f"{dt}-384-spatial-16", dt, 384, "spatial", 7, 16, 1, 0.0))
        cases.append((f"{dt}-384-temporal-5-big", dt, 384, "temporal", 3, 5, 7, 20.0))
    return cases


def group_cases():
    """(name, dt, C, kind, N, Tn, HW, big, film, act, mode, strided).  mode: 'affine' (a, b only), 'tensor' (y only), 'both'; every
    case also takes mr_out.  strided: x and y column slices of buffers C + 44 wide (ld % 4 == 0, ld % 8 != 0)."""
    cases = []
    for dt in ("bf16", "f32"):
        for Tn, C, mode, film, act in ((1, 128, "both", True, True), (37, 128, "tensor", False, True), (400, 1024, "both", True, True),
                                       (256, 2048, "tensor", True, False), (4096, 128, "both", False, False), (37, 384, "affine", True, False)):
            cases.append((f"{dt}-{C}-{Tn}-{mode}", dt, C, "per_sample", 2, Tn, 1, 0.0, film, act, mode, False))
        cases.append((f"{dt}-128-37-strided", dt, 128, "per_sample", 2, 37, 1, 0.0, True, True, "both", True))
        cases.append((f"{dt}-256-30-temporal", dt, 256, "temporal", 2, 30, 3, 0.0, False, True, "both", False))
        cases.append((f"{dt}-256-100-big", dt, 256, "per_sample", 2, 100, 1, 20.0, True, True, "both", False))
    return cases


def finalize_cases():
    """(name, C, S, nrec, ratio = group mean / std, film, strided).  total = nrec * qpg terms per (group, slice): 1 (one thread with data),
    80 and 1200 (no multiples of 256; 1200: the second trip of the `i += 1024` loop), 512 (every lane of the first trip full)."""
    return [("one-record", 128, 2, 1, 0.6, False, False), ("c2048", 2048, 2, 5, 0.6, True, False),
            ("second-trip", 512, 2, 300, 0.6, True, False), ("full-trip", 1024, 3, 64, 0.6, False, False),
            ("strided", 256, 3, 7, 0.6, True, True), ("mean-8-std", 384, 2, 9, 8.0, True, False)]


def finalize_inputs(C, S, nrec, ratio, film, seed=31):
    """Synthetic fp32 records [S * nrec, C / 4, 2] of 256 values each with group mean = ratio * std, and gamma, beta, film."""
    g = torch.Generator().manual_seed(seed + C + nrec)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    NQ = C // 4
    std = (0.5 + torch.rand(S, 1, 32, 1, generator=g, dtype=torch.float64)).expand(S, nrec, 32, NQ // 32)
    m = std * ratio + std * rn(S, nrec, 32, NQ // 32) / 16
    s2 = std * std * (1 + 0.1 * rn(S, nrec, 32, NQ // 32)).abs() + m * m
    rec = torch.stack([256 * m, 256 * s2], -1).reshape(S * nrec, NQ, 2).float()
    gamma, beta = 1 + 0.1 * rn(C).float(), rn(C).float()
    return rec, gamma, beta, (rn(S, 2 * C).float() * 0.3 if film else None)


ROWBIAS_CASES = [("bf16", 3, 37, 136, False), ("f32", 3, 37, 136, True), ("bf16", 2, 1, 2048, True), ("f32", 5, 300, 8, False)]   # dt, N, rows per sample, C, strided


def rowbias_inputs(dt, N, rps, C, seed=41):
    g = torch.Generator().manual_seed(seed + C)
    return torch.randn(N * rps, C, generator=g).to(DT[dt]), torch.randn(N, C, generator=g)


# the variants the case lists must reach (asserted by tests/test_errbound_fwd_cpu.py)
VARIANTS = ["apply:two-column-passes", "apply:idle-lanes", "apply:one-row-lane", "apply:R-doubled", "apply:strided",
            "small:dead-threads", "small:S%spb", "small:spb1", "small:Tn16", "small:Tn1",
            "group:items1", "group:items37", "group:items3200", "group:items4096-wide", "group:items4096-tall", "group:ld%8", "group:tstride",
            "group:affine-only", "group:tensor-only", "group:both",
            "finalize:one-term", "finalize:second-trip", "finalize:ragged", "finalize:strided", "finalize:film"]


def variants_reached():
    got = set()
    for _, dt, C, kind, N, Tn, HW, big, strided in apply_cases():
        passes, rpp, idle = thread_shape(dt, C)
        S = B.gn_slices(kind, N, Tn, HW)[1][0]
        got |= {"apply:two-column-passes"} if passes == 2 else set()
        got |= {"apply:idle-lanes"} if idle and passes == 1 else set()
        got |= {"apply:one-row-lane"} if rpp == 1 else set()
        got |= {"apply:R-doubled"} if gn_apply_R(dt, C, S, Tn)[1] else set()
        got |= {"apply:strided"} if strided else set()
    for _, dt, C, kind, N, Tn, HW, big in small_cases():
        assert gn_small_ok(dt, C, Tn)
        spb, dead = gn_small_spb(dt, C)
        S = B.gn_slices(kind, N, Tn, HW)[1][0]
        got |= {"small:dead-threads"} if dead else set()
        got |= {"small:S%spb"} if S % spb else set()
        got |= {"small:spb1"} if spb == 1 else set()
        got |= {f"small:Tn{Tn}"} if Tn in (1, 16) else set()
    for _, dt, C, kind, N, Tn, HW, big, film, act, mode, strided in group_cases():
        assert gn_group_ok(C, Tn, C + 44 if strided else C)
        items = Tn * (C // 128)
        got.add(f"group:items{items}" + (("-wide" if C == 2048 else "-tall") if items == 4096 else ""))
        got |= {"group:ld%8"} if strided and (C + 44) % 8 else set()
        got |= {"group:tstride"} if kind == "temporal" else set()
        got.add({"affine": "group:affine-only", "tensor": "group:tensor-only", "both": "group:both"}[mode])
    for _, C, S, nrec, ratio, film, strided in finalize_cases():
        total = nrec * (C // 128)
        got |= {"finalize:one-term"} if total == 1 else set()
        got |= {"finalize:second-trip"} if total > 1024 else set()
        got |= {"finalize:ragged"} if total % 256 else set()
        got |= {"finalize:strided"} if strided else set()
        got |= {"finalize:film"} if film else set()
    return got


# =========================================================================== layout-edge convolutions (mmd_edge.hip)
T27 = [t for t in itertools.product((-1, 0, 1), repeat=3)]
T9 = E.TAPS_SPATIAL
TT3 = E.TAPS_TEMPORAL
TA3 = [(0, 0, -1), (0, 0, 0), (0, 0, 1)]                  # the audio taps on (F, H, W) = (1, 1, L)
T5 = [(0, 0, d) for d in (-2, -1, 0, 1, 2)]
T10 = T27[1::2][:10]
TAPS = {"27": T27, "9": T9, "t3": TT3, "a3": TA3, "5": T5, "10": T10}


def stem_variant(dt, Cin, W, Cout, taps, ldy):
    """mmd_stem_conv :291-301, stem_mfma_ok :259-265 (MMD_STEM_MFMA unset; y and bias 16-byte aligned): 'mfma' | 'strip' | 'pixel'."""
    unit = all(-1 <= o <= 1 for t in taps for o in t)
    if unit and dt == "bf16" and W % 32 == 0 and len(taps) * Cin <= 28 and Cin <= 3 and Cout % 32 == 0 and Cout <= 128 and ldy % 8 == 0:
        return "mfma"
    if W % 4 == 0 and Cin in (1, 3) and Cout % 4 == 0:
        return "strip"
    return "pixel"


def head_variant(dt, Cin, Co, ntaps, W, y_aligned=True):
    """launch_head :514-546: (kernel, lanes per row, padded output width CO) or None where the launch is refused."""
    e = epv(dt)
    lpr = Cin // e
    if W % 4 == 0 and y_aligned and Cin % e == 0 and lpr in (4, 8, 16, 32) and ntaps * e * Co * lpr * 4 <= 150 * 1024 and Co in (1, 2, 3, 6):
        return "strip", lpr, Co
    CO = 2 if Co <= 2 else (4 if Co <= 4 else 8)
    if Cin % e == 0 and lpr in (4, 8, 16, 32, 64) and ntaps * (e * CO // 4) * lpr * 16 <= 150 * 1024:
        return "coop", lpr, CO
    if ntaps * Cin * CO * 4 > 150 * 1024:
        return None
    return "plain", lpr, CO


def api_to_rows(x5):
    """[N, F, C, H, W] -> rows [N F H W, C]."""
    return x5.permute(0, 1, 3, 4, 2).reshape(-1, x5.shape[2])


def rows_to_api(r, N, F, Hh, Ww):
    return r.reshape(N, F, Hh, Ww, r.shape[1]).permute(0, 1, 4, 2, 3)


def edge_weight_rows(w):
    """packed [ntaps, Cin, Cout] -> [Cout, ntaps * Cin] (K index = tap * Cin + ci, the layout of errbound.conv_rows_ref)."""
    return w.permute(2, 0, 1).reshape(w.shape[2], -1)


def edge_ref(rows, w, bias, taps, dims, out_dtype):
    """float64 conv on rows [M, Cin] (stored operands) with the packed weight w [ntaps, Cin, Cout]: (ref [M, Cout], bound)."""
    ref, S = E.conv_rows_ref(rows, edge_weight_rows(w), bias, None, taps, dims)
    return ref, E.gemm_bound(ref, S, len(taps) * rows.shape[1], out_dtype)


def _gather_defect(x, taps, dims, defect):
    """errbound.conv_gather with a border mask left open: 'next_row' - a tap with dw > 0 at the last pixel of an image row reads the
    next row's first pixel; 'next_sample' - a tap with df > 0 in a sample's last frame reads the next sample's first frame."""
    M = x.shape[0]
    D0, D1, D2 = dims
    m = torch.arange(M)
    p2, p1, p0 = m % D2, (m // D2) % D1, (m // (D1 * D2)) % D0
    out = []
    for d0, d1, d2 in taps:
        ok0, ok1, ok2 = (p0 + d0 >= 0) & (p0 + d0 < D0), (p1 + d1 >= 0) & (p1 + d1 < D1), (p2 + d2 >= 0) & (p2 + d2 < D2)
        src = m + d0 * D1 * D2 + d1 * D2 + d2
        if defect == "next_row" and d2 > 0:
            ok2 = ok2 | ((p2 == D2 - 1) & (src < M))
        if defect == "next_sample" and d0 > 0:
            ok0 = ok0 | ((p0 == D0 - 1) & (src < M))
        ok = ok0 & ok1 & ok2
        out.append(x[src.clamp(0, M - 1)] * ok[:, None].to(x.dtype))
    return out


def emu_edge(rows, w, bias, taps, dims, out_dtype, defect=None, lpr=1):
    """fp32 accumulation tap by tap, the bias, one round-to-nearest store.  defect: None | 'next_row' | 'next_sample' | 'bias_per_lane'
    (every one of the lpr lanes of a cooperative row adds the bias) | 'tap_group' (the clamped taps of a partly filled group of 3 count again)."""
    x = rows.float()
    Cin = x.shape[1]
    W2 = edge_weight_rows(w).float()
    g = _gather_defect(x, taps, dims, defect) if defect in ("next_row", "next_sample") else [t for t, _ in E.conv_gather(x, taps, dims)]
    acc = torch.zeros(x.shape[0], W2.shape[0])
    for t, gx in enumerate(g):
        acc = acc + gx @ W2[:, t * Cin:(t + 1) * Cin].t()
    if defect == "tap_group":
        assert len(taps) % 3
        acc = acc + (3 - len(taps) % 3) * (g[-1] @ W2[:, -Cin:].t())
    if bias is not None:
        acc = acc + bias.float() * (lpr if defect == "bias_per_lane" else 1)
    return acc.to(out_dtype)


def stem_cases():
    """dicts: name, dt, N, F, Cin, H, W, Cout, taps (key of TAPS), bias, y_strided, variant (the kernel the launch must take)."""
    cases = []

    def add(name, dt, N, F, Cin, Hh, Ww, Cout, taps, variant, bias=True, y_strided=False):
        cases.append(dict(name=f"{variant}-{name}-{dt}", dt=dt, N=N, F=F, Cin=Cin, H=Hh, W=Ww, Cout=Cout, taps=taps, bias=bias, y_strided=y_strided, variant=variant))

    for dt in ("f32", "bf16"):
        add("3x5x7-c3", dt, 2, 3, 3, 5, 7, 64, "27", "pixel")             # W % 4 != 0
        add("2x4x8-c2", dt, 2, 2, 2, 4, 8, 32, "9", "pixel")              # Cin = 2 at W % 4 == 0
        add("1x3x6-c1", dt, 2, 1, 1, 3, 6, 8, "27", "pixel", bias=False)  # F = 1: every df != 0 tap outside
    add("3x5x8", "f32", 2, 3, 3, 5, 8, 64, "27", "strip")
    add("3x5x32", "f32", 2, 3, 3, 5, 32, 64, "9", "strip")               # fp32 never takes the MFMA kernel
    add("2x3x12", "bf16", 2, 2, 3, 3, 12, 64, "9", "strip")
    add("1x4x4", "bf16", 2, 1, 3, 4, 4, 72, "27", "strip", y_strided=True)    # F = 1, W = 4: one strip per image row
    add("2x1x4", "f32", 2, 2, 1, 1, 4, 32, "27", "strip")                # H = 1
    add("w5tap", "bf16", 2, 1, 1, 1, 32, 32, "5", "strip")               # offsets of +-2: refused by the MFMA kernel
    for dt in ("f32", "bf16"):
        add("audio-L52", dt, 2, 1, 1, 1, 52, 96, "a3", "strip")
    for Cout in (32, 64, 96, 128):
        add(f"3x5x32-o{Cout}", "bf16", 2, 3, 3, 5, 32, Cout, "9", "mfma")     # K = 27: 14 k-steps, the last half-filled
    add("audio-L64", "bf16", 2, 1, 1, 1, 64, 96, "a3", "mfma")           # K = 3: two k-steps, the second half-filled
    add("audio-3xL96", "bf16", 3, 1, 1, 1, 96, 64, "a3", "mfma")         # 9 groups: a ragged last block
    add("3x4x32-c1", "bf16", 2, 3, 1, 4, 32, 64, "27", "mfma")
    add("1x1x32-c1", "bf16", 2, 1, 1, 1, 32, 32, "27", "mfma")           # F = H = 1: nine of the 27 taps can land
    add("4x2x32-t3", "bf16", 2, 4, 3, 2, 32, 64, "t3", "mfma")           # K = 9
    add("3x5x32-nobias", "bf16", 2, 3, 3, 5, 32, 64, "9", "mfma", bias=False)
    add("3x5x32-slice", "bf16", 2, 3, 3, 5, 32, 96, "9", "mfma", y_strided=True)
    add("pipelined", "bf16", 1, 3, 3, 96, 1024, 32, "9", "mfma")         # 9216 groups > 8192 waves: 1024 waves take a second group through xnext
    return cases


def head_cases():
    """dicts: name, dt, N, F, H, W, Cin, Co, taps, bias, x_strided, y_off (output view 4 bytes off a 16-byte boundary), variant, lpr."""
    cases = []

    def add(name, dt, N, F, Hh, Ww, Cin, Co, taps, variant, bias=True, x_strided=False, y_off=False):
        v = head_variant(dt, Cin, Co, len(TAPS[taps]), Ww, not y_off)
        assert v is not None and v[0] == variant, (name, dt, v)
        cases.append(dict(name=f"{variant}-{name}-{dt}", dt=dt, N=N, F=F, H=Hh, W=Ww, Cin=Cin, Co=Co, taps=taps, bias=bias, x_strided=x_strided,
                          y_off=y_off, variant=variant, lpr=v[1]))

    rot = [("27", 3, (3, 5, 8)), ("a3", 1, (1, 1, 52)), ("5", 2, (2, 3, 8)), ("10", 6, (3, 4, 4))]
    for dt, e in (("bf16", 8), ("f32", 4)):
        for i, lanes in enumerate((4, 8, 16, 32)):                       # strip: every lane count, Co 1 / 2 / 3 / 6, the four tap lists
            for k in range(2):
                taps, Co, (F, Hh, Ww) = rot[(i + k) % 4]
                if lanes == 32 and taps in ("27", "10") and Co * len(TAPS[taps]) * e * 32 * 4 > 150 * 1024:
                    taps = "9"                                             # the strip kernel's LDS limit
                add(f"l{lanes}-{F}x{Hh}x{Ww}-o{Co}-{taps}", dt, 2, F, Hh, Ww, lanes * e, Co, taps, "strip", x_strided=k == 1, bias=(i + k) % 3 != 0)
        add("1x4x4-27", dt, 2, 1, 4, 4, 8 * e, 3, "27", "strip")        # F = 1, W = 4
        add("2x1x4-27", dt, 2, 2, 1, 4, 4 * e, 1, "27", "strip")        # H = 1
        for i, (Co, taps) in enumerate(((4, "27"), (5, "10"), (7, "5"), (8, "a3"))):     # coop by output width
            F, Hh, Ww = (1, 1, 52) if taps == "a3" else (3, 5, 8)
            add(f"o{Co}-{taps}", dt, 2, F, Hh, Ww, (8, 16, 4, 32)[i] * e, Co, taps, "coop", x_strided=i == 1)
        add("w6-27", dt, 2, 3, 5, 6, 16 * e, 3, "27", "coop")           # W % 4 != 0
        add("w6-1x1x6", dt, 2, 1, 1, 6, 4 * e, 2, "27", "coop", bias=False)
        add("l64-9", dt, 2, 2, 4, 8, 64 * e, 3, "9", "coop")            # 64 lanes per row
        add("yoff", dt, 2, 3, 5, 8, 8 * e, 3, "27", "coop", y_off=True)  # strip refused: the output view is 4 bytes off
    for Cin, taps, Co, x_strided in ((96, "27", 3, False), (24, "10", 5, True), (8, "5", 1, False), (24, "a3", 8, False)):
        F, Hh, Ww = (1, 1, 52) if taps == "a3" else (3, 5, 8)
        add(f"c{Cin}-o{Co}-{taps}", "bf16", 2, F, Hh, Ww, Cin, Co, taps, "plain", x_strided=x_strided)
    add("c48-o3-27", "f32", 2, 3, 5, 7, 48, 3, "27", "plain")
    add("c48-o2-5", "f32", 2, 1, 1, 9, 48, 2, "5", "plain", x_strided=True)
    # grid-stride second passes, audio form: 16400 strips against 2048 blocks x 8; 131075 rows against 2048 blocks x 64
    add("stride2-L65600", "f32", 1, 1, 1, 65600, 128, 3, "a3", "strip")
    add("stride2-L131075", "bf16", 1, 1, 1, 131075, 32, 2, "a3", "coop")
    return cases


def edge_inputs(c, seed=61):
    """The operands of a stem / head case on the CPU: (x, w packed fp32 [ntaps, Cin, Cout], bias or None).  x: the stem's fp32 API-layout
    input [N, F, Cin, H, W]; the head's rows [N F H W, Cin] in the stored dtype."""
    g = torch.Generator().manual_seed(seed + c["Cin"] + 3 * c["W"])
    nt = len(TAPS[c["taps"]])
    if "Cout" in c:
        x = torch.randn(c["N"], c["F"], c["Cin"], c["H"], c["W"], generator=g)
        Cout = c["Cout"]
    else:
        x = torch.randn(c["N"] * c["F"] * c["H"] * c["W"], c["Cin"], generator=g).to(DT[c["dt"]])
        Cout = c["Co"]
    w = torch.randn(nt, c["Cin"], Cout, generator=g) / (nt * c["Cin"]) ** 0.5
    return x, w, (torch.randn(Cout, generator=g) if c["bias"] else None)


EDGE_VARIANTS = ["stem:pixel", "stem:strip", "stem:mfma", "stem:mfma-NB1", "stem:mfma-NB2", "stem:mfma-NB3", "stem:mfma-NB4", "stem:mfma-K3",
                 "stem:mfma-pipelined", "stem:mfma-ragged-block", "stem:strip-tap-clamp", "head:strip", "head:coop", "head:plain",
                 "head:coop-l64", "head:coop-yoff", "head:strip-stride2", "head:coop-stride2", "head:tap-clamp-3", "head:tap-clamp-9"] + \
                [f"head:strip-l{n}-{dt}" for n in (4, 8, 16, 32) for dt in ("bf16", "f32")] + [f"head:strip-o{n}" for n in (1, 2, 3, 6)] + \
                [f"head:coop-o{n}" for n in (4, 5, 7, 8)]


def edge_variants_reached():
    got = set()
    for c in stem_cases():
        nt = len(TAPS[c["taps"]])
        v = stem_variant(c["dt"], c["Cin"], c["W"], c["Cout"], TAPS[c["taps"]], c["Cout"] + (40 if c["y_strided"] else 0))
        assert v == c["variant"], c["name"]
        got.add("stem:" + v)
        groups = c["N"] * c["F"] * c["H"] * (c["W"] // 32)
        if v == "mfma":
            got.add(f"stem:mfma-NB{c['Cout'] // 32}")
            got |= {"stem:mfma-K3"} if nt * c["Cin"] == 3 else set()
            # launch_stem_mfma :268-269: grid = min(2048, ceil(groups / 4)) blocks of 4 waves; stem_conv_mfma_kernel :198, :219-220: a wave
            # walks g = wave_id, wave_id + 4 grid, ... and gathers the next group into xnext while g + nwave < groups
            got |= {"stem:mfma-pipelined"} if groups > 4 * min(2048, _cdiv(groups, 4)) else set()
            got |= {"stem:mfma-ragged-block"} if groups % 4 else set()
        if v == "strip" and nt % 3:
            got.add("stem:strip-tap-clamp")
    for c in head_cases():
        nt = len(TAPS[c["taps"]])
        v, lpr = c["variant"], c["lpr"]
        rows = c["N"] * c["F"] * c["H"] * c["W"]
        got.add("head:" + v)
        if v == "strip":
            got |= {f"head:strip-l{lpr}-{c['dt']}", f"head:strip-o{c['Co']}"}
            # launch_head_strip :480-482: strips = rows / 4, spb = 4 * (64 / lpr) strips per block pass, grid = min(2048, ceil(strips / spb));
            # head_conv_strip_kernel :403-404: sb += nwaves * SPW - a second pass where strips > 2048 * spb
            got |= {"head:strip-stride2"} if rows // 4 > 2048 * 4 * (64 // lpr) else set()
            got |= {"head:tap-clamp-3"} if nt % 3 else set()
        if v == "coop":
            got.add(f"head:coop-o{c['Co']}")
            got |= {"head:coop-l64"} if lpr == 64 else set()
            got |= {"head:coop-yoff"} if c["y_off"] else set()
            # launch_head_coop :495-496: grid = min(2048, ceil(rows / 64)); head_conv_coop_kernel :316, :328-329: a block pass covers
            # 4 waves * RPW = 4 * (64 / lpr) rows, mb += nwaves * RPW - a second pass where rows > 2048 * 4 * (64 / lpr)
            got |= {"head:coop-stride2"} if rows > 2048 * 4 * (64 // lpr) else set()
            got |= {"head:tap-clamp-9"} if nt % 9 else set()
    return got


# =========================================================================== resample, statistics records, bilinear_concat
def resample_ref(x, NF, Hh, Ww, fh, fw, mode, scale, out_dtype):
    """float64 (1, fh, fw) average pool (mode 0) or nearest upsample (mode 1) of rows (nf, h, w) times scale, and the bound."""
    x = _f64(x)
    C = x.shape[1]
    if mode == 0:
        v = x.reshape(NF, Hh // fh, fh, Ww // fw, fw, C)
        inv = scale / (fh * fw)
        ref = (v.sum((2, 4)) * inv).reshape(-1, C)
        e = (fh * fw - 1) * U32 * (v.abs().sum((2, 4)) * abs(inv)).reshape(-1, C) + 2 * U32 * ref.abs()
    else:
        ref = (x.reshape(NF, Hh, 1, Ww, 1, C).expand(NF, Hh, fh, Ww, fw, C) * scale).reshape(-1, C)
        e = (0.0 if scale == 1.0 else U32) * ref.abs()
    return ref, _store(ref, e, out_dtype)


def emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale, defect=None, prestore=False):
    """resample_kernel in fp32.  defect: None | 'bf16_sum' (the pool divides after a bf16 rounding of the sum) | 'fh_both' (the
    upsample uses fh for both axes).  prestore: return the fp32 values in front of the store."""
    C = x.shape[1]
    xf = x.float()
    if mode == 0:
        v = xf.reshape(NF, Hh // fh, fh, Ww // fw, fw, C)
        acc = torch.zeros(NF, Hh // fh, Ww // fw, C)
        for a in range(fh):
            for b in range(fw):
                acc = acc + v[:, :, a, :, b]
        if defect == "bf16_sum":
            acc = acc.to(torch.bfloat16).float()
        y = (acc * (torch.tensor(scale, dtype=torch.float32) / torch.tensor(float(fh * fw)))).reshape(-1, C)
    else:
        ho, wo = torch.arange(Hh * fh) // fh, torch.arange(Ww * fw) // (fh if defect == "fh_both" else fw)
        y = xf.reshape(NF, Hh, Ww, C)[:, ho][:, :, wo.clamp(max=Ww - 1)].reshape(-1, C)
        y = y * scale if scale != 1.0 else y
    return y if prestore else y.to(x.dtype)


def resample_cases():
    """(name, dt, NF, H, W, C, fh, fw, mode, scale, strided, stats).  stats (bf16, scale 1, output rows % 64 == 0): mmd_resample_stats
    too - its output bitwise the plain kernel's, its records per (record, quad)."""
    cases = []
    for dt in ("bf16", "f32"):
        st = dt == "bf16"
        cases += [(f"pool2x2-{dt}", dt, 4, 8, 16, 64, 2, 2, 0, 1.0, False, st), (f"pool2x2-s.25-{dt}", dt, 3, 6, 10, 24, 2, 2, 0, 0.25, True, False),
                  (f"pool1x4-{dt}", dt, 2, 1, 512, 24, 1, 4, 0, 1.0, True, st), (f"pool1x3-{dt}", dt, 2, 1, 384, 256, 1, 3, 0, 1.0, False, st),
                  (f"pool1x3-s.25-{dt}", dt, 3, 2, 9, 40, 1, 3, 0, 0.25, False, False),
                  (f"up2x2-{dt}", dt, 2, 4, 4, 72, 2, 2, 1, 1.0, True, st), (f"up1x4-s.25-{dt}", dt, 3, 1, 7, 32, 1, 4, 1, 0.25, False, False),
                  (f"up1x3-{dt}", dt, 2, 3, 5, 2048, 1, 3, 1, 1.0, False, False)]
    return cases


def resample_inputs(NF, Hh, Ww, C, dt, seed=71):
    g = torch.Generator().manual_seed(seed + C + Ww)
    return (torch.randn(NF * Hh * Ww, C, generator=g) * 1.5 + 0.6).to(DT[dt])


def record_values(y):
    """The 256 stored values of every (64-row record, channel quad) of y [M, C]: [M / 64, C / 4, 256]."""
    M, C = y.shape
    return y.reshape(M // 64, 64, C // 4, 4).permute(0, 2, 1, 3).reshape(M // 64, C // 4, 256)


def records_ref(vals):
    """float64 (sum, sum of squares) of vals [nrec, Q, n] and their bounds: n terms in ANY order ((n - 1) u sum |y|; the squares are
    rounded once more or fused: n u sum y^2) - the producers fold their partial sums in orders of their own (resample_stats_kernel
    :162-180: the thread's rows in order, then the row groups; the GEMM epilogues: per lane, across lanes, across waves)."""
    v = _f64(vals)
    n = v.shape[-1]
    ref = torch.stack([v.sum(-1), (v * v).sum(-1)], -1)
    bound = torch.stack([(n - 1) * U32 * v.abs().sum(-1), n * U32 * (v * v).sum(-1)], -1)
    return ref, bound


def check_records(rec, vals, what):
    """Every (record, quad) pair (sum, sum of squares) of rec [nrec, Q, 2] against float64 sums of its own 256 stored values with its
    own bound; returns the worst ratio."""
    ref, bound = records_ref(vals)
    return E.check(rec.reshape(rec.shape[0], -1), ref.reshape(rec.shape[0], -1), bound.reshape(rec.shape[0], -1), what=what)


def emu_records(vals, defect=None, prestore=None):
    """fp32 records of vals [nrec, Q, 256] (row-major chain per quad).  defect: None | 'miss_row' (the 64th row missing) | 'prestore'
    (summed from the fp32 values `prestore` in front of the store rounding)."""
    v = (prestore if defect == "prestore" else vals).float()
    if defect == "miss_row":
        v = v[..., :252]
    return torch.stack([_chain_sum(v), _chain_sum(v * v)], -1)


GEMM_RECORD_CASES = [(256, 64, 96), (192, 256, 264), (128, 128, 128), (256, 256, 192)]   # M, Cin, Cout (1 x 1)


def strip_ok(dt, Cin, Cout):
    """ops.strip_tile_ok for a 1 x 1 conv with statistics (M % 64 == 0): tile 131 is bf16, K in {128, 256, 384, 512}, Cout a multiple of
    64 (K <= 256) or 32."""
    return dt == "bf16" and Cin in (128, 256, 384, 512) and Cout % (64 if Cin <= 256 else 32) == 0


def bilinear_ref(low, Hh, Ww):
    """float64 bilinear upsample of low [N, C, h, w] to (H, W) with the align_corners=False coordinates, and the fp32 bound of
    bilinear_concat_kernel (mmd_edge.hip:746-751): the source coordinate fy = max((yo + 0.5) sh - 0.5, 0) carries the rounding of
    sh = h / H, of the product and of the subtraction, e_fy = 2 u (yo + 0.5) sh + u fy (fy - y0 is exact); the interpolant is continuous
    and piecewise linear, so a coordinate error moves the value by at most e_fy times the steepest slope among the cell and its two
    neighbours along that axis - a floor that lands one cell off at an exactly integral coordinate is inside the bound by construction;
    each of the four terms passes 6 roundings (1 - l, two products, two adds, the second 1 - l): 6 u sum weight |p|."""
    p = _f64(low)
    N, C, h, w = p.shape

    def coord(n_out, n_in):
        o = torch.arange(n_out, dtype=torch.float64, device=p.device)
        s = n_in / n_out
        f = ((o + 0.5) * s - 0.5).clamp_min(0)
        i0 = f.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return f, i0, i1, f - i0, 2 * U32 * (o + 0.5) * s + U32 * f

    fy, y0, y1, ly, e_fy = coord(Hh, h)
    fx, x0, x1, lx, e_fx = coord(Ww, w)
    ly_, lx_ = ly[:, None], lx[None, :]
    g = lambda yi, xi: p[:, :, yi][:, :, :, xi]                                       # [N, C, H, W]
    p00, p01, p10, p11 = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
    ref = (1 - ly_) * ((1 - lx_) * p00 + lx_ * p01) + ly_ * ((1 - lx_) * p10 + lx_ * p11)
    Sw = (1 - ly_) * ((1 - lx_) * p00.abs() + lx_ * p01.abs()) + ly_ * ((1 - lx_) * p10.abs() + lx_ * p11.abs())
    ym, yp = (y0 - 1).clamp(min=0), (y1 + 1).clamp(max=h - 1)
    xm, xp = (x0 - 1).clamp(min=0), (x1 + 1).clamp(max=w - 1)
    # slopes along y between consecutive source rows (at both x neighbours), along x likewise: the steepest of three cells
    sy = torch.stack([(g(b, xi) - g(a, xi)).abs() for a, b in ((ym, y0), (y0, y1), (y1, yp)) for xi in (x0, x1)]).amax(0)
    sx = torch.stack([(g(yi, b) - g(yi, a)).abs() for a, b in ((xm, x0), (x0, x1), (x1, xp)) for yi in (y0, y1)]).amax(0)
    bound = 6 * U32 * Sw + e_fy[:, None] * sy + e_fx[None, :] * sx
    return ref, bound


def emu_bilinear(low, Hh, Ww, defect=None):
    """bilinear_concat_kernel's arithmetic in fp32.  defect: None | 'align_corners' | 'no_clamp' (the neighbour index of the last row is
    not clamped: it reads the first row of the next plane)."""
    p = low.float()
    N, C, h, w = p.shape
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)

    def coord(n_out, n_in):
        o = torch.arange(n_out, dtype=torch.float32)
        if defect == "align_corners":
            f = o * (f32(max(n_in - 1, 0)) / f32(max(n_out - 1, 1)))
        else:
            f = ((o + 0.5) * (f32(n_in) / f32(n_out)) - 0.5).clamp_min(0)
        i0 = f.long()
        return i0, i0 + (i0 < n_in - 1).long(), f - i0.float()

    y0, y1, ly = coord(Hh, h)
    x0, x1, lx = coord(Ww, w)
    if defect == "no_clamp":
        y1 = y0 + 1
        p = torch.cat([p, p.flatten(0, 1).roll(-1, 0).reshape(N, C, h, w)[:, :, :1]], 2)      # row h of a plane = row 0 of the next one
    ly, lx = ly[:, None], lx[None, :]
    g = lambda yi, xi: p[:, :, yi][:, :, :, xi]
    return (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))


# (N, C, H, W, h, w): ratios 8 -> 32, 7 -> 20, 5 -> 12, 9 -> 6 (down), and a single source row / column
BILINEAR_CASES = [(2, 3, 32, 32, 8, 8), (2, 3, 20, 20, 7, 7), (1, 2, 12, 20, 5, 7), (2, 3, 6, 6, 9, 9), (1, 3, 8, 12, 1, 5), (1, 3, 12, 8, 5, 1)]


def bilinear_inputs(N, C, Hh, Ww, h, w, seed=81):
    g = torch.Generator().manual_seed(seed + Hh + w)
    return torch.randn(N, C, Hh, Ww, generator=g), torch.randn(N, C, h, w, generator=g)


# =========================================================================== chain: producer -> records -> gn_finalize_stats
def chain_ref(y, gamma, beta, film, S):
    """GroupNorm affine of the STORED producer output y [S * Tn, C] (Tn % 64 == 0) in float64, with the bound of the path records ->
    gn_finalize_stats.  Per record the producer's fp32 sums carry (records_ref) 255 u sum |y| and 256 u sum y^2; the finalize adds
    them in double and converts once.  With A = sum |y| / cnt and E2 = sum y^2 / cnt over the group:
        e_mean = 255 u A + u |mean|,   e_var = 256 u E2 + 2 |mean| 255 u A,   e_rstd = rstd^3 e_var / 2 + u rstd
    and errbound_bwd.gn_affine.  The cancellation of var = E[y^2] - mean^2: with r = mean^2 / var, E2 = var (1 + r) and
    A <= sqrt(E2), so e_var / var <= 256 u (1 + r) + 510 u sqrt(r (1 + r)) -> 766 u r, and the relative bound on a, e_var / (2 var),
    passes 2**-9 (half a bf16 ulp) where 383 u r = 2**-9: r = 2**15 / 383 = 86, a group mean of 9.2 std.  The inputs here have means of
    0.6 and 5 std (r = 0.36 and 25: bounds of 2e-5 and 6e-4 relative)."""
    y, gamma, beta, film = _f64(y), _f64(gamma), _f64(beta), _f64(film)
    M, C = y.shape
    Tn, cpg = M // S, C // 32
    g = y.reshape(S, Tn, 32, cpg)
    cnt = Tn * cpg
    mean = g.mean((1, 3))
    dev = g - mean[:, None, :, None]
    var = (dev * dev).mean((1, 3))
    rstd = (var + GN_EPS).rsqrt()
    A, E2 = g.abs().sum((1, 3)) / cnt, (g * g).sum((1, 3)) / cnt
    e_mean = 255 * U32 * A + U32 * mean.abs()
    e_var = 256 * U32 * E2 + 2 * mean.abs() * 255 * U32 * A
    e_rstd = rstd ** 3 * e_var / 2 + U32 * rstd
    a, b, e_a, e_b = B.gn_affine(mean, rstd, e_mean, e_rstd, gamma, beta, film)
    return dict(a=a, b=b, e_a=e_a, e_b=e_b, mean=mean, rstd=rstd, e_mean=e_mean, e_rstd=e_rstd)


CHAIN_RATIO_AT_HALF_ULP = 2.0 ** 15 / 383                 # mean^2 / var at which the chain's bound on a passes 2**-9 (chain_ref)
# (producer, M, Cin, C, S, mean / std of the producer's output): conv_gemm tiles (1 x 1, the mean through the residual), resample with stats=
CHAIN_CASES = [(f"tile{t}", 256, 128, 128, 2, m) for t in (64, 128, 129, 131) for m in (0.6, 5.0)] + \
              [("gn_conv1x1", 256, 128, 128, 2, m) for m in (0.6, 5.0)] + [("resample", 512, 0, 256, 2, m) for m in (0.6, 5.0)]


def chain_inputs(M, Cin, C, S, m, seed=91):
    """bf16 operands of a chain case whose stored output has a group mean of about m std: x [M, Cin or C], the packed 1 x 1 weight
    [C, Cin], bias, a residual that carries the mean (conv output and residual both of unit variance: std sqrt 2), the next norm's
    gamma, beta, film."""
    g = torch.Generator().manual_seed(seed + int(10 * m))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(M, Cin or C).to(torch.bfloat16)
    w = (rn(C, Cin) * Cin ** -0.5).to(torch.bfloat16) if Cin else None
    return x, w, rn(C) * 0.1, (rn(M, C) + m * 2 ** 0.5).to(torch.bfloat16), 1 + 0.1 * rn(C), rn(C), 0.3 * rn(S, 2 * C)


# =========================================================================== head as GEMM + gather (mmd_head_gemm, mmd_head_gather)
def head_gemm_unpack(img):
    """The (hi, lo) bf16 matrices [2, 96, 128] out of the weight image of ops.head_gemm_pack ([2][3][8][2 halves][32][8], lane (l31, half)
    of (block ob, k-step cg) = W[32 ob + l31][16 cg + 8 half .. + 8])."""
    return img.view(2, 3, 8, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(2, 96, 128)


def head_weight_rows(w):
    """packed [ntaps, 128, Co] -> W [ntaps * Co, 128], row o = tap * Co + co."""
    return w.permute(0, 2, 1).reshape(-1, w.shape[1])


def head_gemm_ref(xs, a, b, act, w, hilo):
    """P [NO, M] in float64 from the stored xs [S, Tn, 128] (bf16), a, b [S, 128] (fp32), the fp32 packed weight w [ntaps, 128, Co] and
    the unpacked image hilo [2, 96, 128]; returns (P, e_P)  (module docstring)."""
    s, e_s = apply_ref(xs, a, b, act, torch.bfloat16)
    s, e_s = s.flatten(0, 1), e_s.flatten(0, 1)                                        # [M, 128]
    Wm = _f64(head_weight_rows(w))
    NO = Wm.shape[0]
    hi, lo = _f64(hilo[0, :NO]), _f64(hilo[1, :NO])
    r = (Wm - hi - lo).abs()
    sa = s.abs() + e_s
    P = Wm @ s.t()
    e_P = Wm.abs() @ e_s.t() + r @ sa.t() + 255 * U32 * ((hi.abs() + lo.abs()) @ sa.t())
    return P, e_P


def head_gather_ref(P, bias, Co, taps, dims, e_P=None):
    """y rows [M, Co] in float64 = bias + the tap sum of the planes P [ntaps * Co, M] (zero outside dims), and the bound: ntaps fp32
    additions on |bias| + sum |P| (e_P given: P is the float64 reference of a computed P with that bound - its tap sum is added)."""
    P, bias = _f64(P), _f64(bias)
    nt = len(taps)
    Pr = P.reshape(nt, Co, -1).permute(2, 0, 1)                                        # [M, ntaps, Co]
    Er = None if e_P is None else e_P.reshape(nt, Co, -1).permute(2, 0, 1)
    y = torch.zeros(Pr.shape[0], Co, dtype=torch.float64, device=P.device)
    Sa, Se = torch.zeros_like(y), torch.zeros_like(y)
    for t in range(nt):
        (g, ok), = E.conv_gather(Pr[:, t], [taps[t]], dims)
        y += g
        Sa += g.abs()
        if Er is not None:
            Se += E.conv_gather(Er[:, t], [taps[t]], dims)[0][0]
    if bias is not None:
        y += bias
        Sa += bias.abs()
    return y, nt * U32 * (Sa + Se) + Se


def emu_head_gemm(xs, a, b, act, hilo, NO, drop_lo=False):
    """head_gemm_kernel: fp32 affine + silu, one bf16 rounding, bf16 x bf16 products summed in fp32 (hi first, then lo)."""
    s = emu_apply(xs, a, b, act, torch.bfloat16).flatten(0, 1).float()
    P = hilo[0, :NO].float() @ s.t()
    return P if drop_lo else P + hilo[1, :NO].float() @ s.t()


def emu_head_gather(P, bias, Co, taps, dims):
    nt = len(taps)
    Pr = P.float().reshape(nt, Co, -1).permute(2, 0, 1)
    acc = torch.zeros(Pr.shape[0], Co) + (0.0 if bias is None else bias.float())
    for t in range(nt):
        acc = acc + E.conv_gather(Pr[:, t], [taps[t]], dims)[0][0]
    return acc


def host_head_gemm_pack(w):
    """ops.head_gemm_pack's arithmetic on the host (the CPU proof has no library): [2, 96, 128] bf16."""
    full = torch.zeros(96, 128)
    full[: w.shape[0] * w.shape[2]] = head_weight_rows(w)
    hi = full.to(torch.bfloat16)
    return torch.stack([hi, (full - hi.float()).to(torch.bfloat16)])


# (name, Co, taps, N, F, H, W, S): rows = N F H W = S slices of 128 or 384 rows; NO = ntaps * Co
T11, T24 = T27[:11], T27[:24]
TAPS.update({"11": T11, "24": T24})
HEAD_GEMM_CASES = [("o1-27", 1, "27", 3, 2, 8, 8, 3), ("o2-27", 2, "27", 2, 6, 8, 8, 2), ("o3-27", 3, "27", 3, 2, 8, 8, 3),
                   ("o4-9", 4, "9", 2, 6, 8, 8, 2), ("o6-9", 6, "9", 3, 2, 8, 8, 3), ("o3-11", 3, "11", 2, 6, 8, 8, 2),
                   ("o4-24", 4, "24", 3, 2, 8, 8, 3), ("o1-27-1025-groups", 1, "27", 1025, 2, 8, 8, 1025)]


def head_gemm_inputs(Co, taps, N, F, Hh, Ww, S, seed=101):
    g = torch.Generator().manual_seed(seed + Co + S)
    M, nt = N * F * Hh * Ww, len(TAPS[taps])
    x = (torch.randn(M, 128, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    a, b = torch.rand(S, 128, generator=g) + 0.5, torch.randn(S, 128, generator=g) * 0.3
    w = torch.randn(nt, 128, Co, generator=g) * (nt * 128) ** -0.5
    return x, a, b, w, torch.randn(Co, generator=g)
