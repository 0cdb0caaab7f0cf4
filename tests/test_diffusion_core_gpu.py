"""Every kernel built on the element core of mmd_diffusion.hip (ddpm_update, ddim_update, ddpm_update_bwd, loss_terms, loss_terms_bwd,
vlb_terms, vlb_terms_bwd) over the whole flag space, against float64 references built from oracle/diffusion_ref.py on the same fp32
inputs and fp32 tables.

Cases.  Main: N, F, C, HW = 3, 2, 3, 5 with t = [0, 4, 9] on a 10-step schedule - the t = 0 branch, odd extents (a slip in the
(n, f, c, hw) decomposition lands on another element), and 30 elements per sample against the 64 chunks of the reducing kernels, so
most chunks are empty.  Second reduce shape: 1000 elements per sample, which 64 does not divide.  Large: 3 x 4 x 3 x 32768 elements,
one flag set per element-wise kernel - more than the 4096 x 256 threads of the grid, so the grid-stride loop takes a second trip.
Flags 0 - 7 (1 clip x0, 2 model predicts x0, 4 learned-range variance), 8 more with the reverse-ODE bit for ddim_update; the two
combinations an entry point rejects must raise MMDError.  Optional outputs are checked present and absent.

Per-sample reductions keep the tolerances the suite already states: mse rtol 1e-5 and vb rtol 2e-4 / atol 1e-6 (test_ops_gpu.py:
test_loss_terms); vlb_terms at most twice the error of the same formulas evaluated with torch in fp32 on the CPU, t = 0 and t > 0
apart (test_vlb_gpu.py).  The model outputs are predictions of realistic quality (as in test_vlb_gpu.py: at t = 0 the decoder's
standard deviation is ~0.01, and a random prediction would leave every likelihood on its 1e-12 clamp).

Element-wise outputs: ZERO elements outside a per-element bound (tests/errbound.py: violations / check).  The bound comes from
evaluating the kernel's expression once more in float64 with the class `V` below, which carries beside the value v
    m >= |v|: the summed magnitudes of the terms of the expression (a difference keeps both sides, a quotient and a root keep the
              amplification of their operand), and
    n       : the number of fp32 roundings so far,
so that an fp32 evaluation in any association, with or without fused multiply-adds, is within n U m of v (U = 2^-24, first order).
The values v are not the reference: every test first requires them to agree with the float64 result of oracle/diffusion_ref.py (the
forward outputs) or with float64 autograd through it (the gradients) to 1e-9, then holds the kernel to the bound around the oracle.
Where a kernel takes a hard decision on a rounded value (ddpm_update_bwd: |x0| <= 1) the elements whose float64 x0 lies within its
own bound of the threshold are left out; the tests require them to be few.

Library functions.  expf and tanhf enter a bound as K_EXP and K_TANH roundings of their result (expf: relative to the result; tanhf:
relative to |tanh|).  Their error on gfx950 was measured with this file, on an MI355X and on the library as it was before the element
core existed, as the smallest count at which no element of an output that passes through them (ddpm_update `out`, the variance
channels of loss_terms_bwd, vlb_terms_bwd; every case of this file) leaves its bound:
    measured count = 0    (none leaves it even with the two functions counted as exact: beneath the allowance of the arithmetic
                           around them the library's own error cannot be resolved through these kernels)
Twice that is still nothing, and no margin for a compiler update that moves a last bit.  The allowance is therefore what the
library promises rather than what was seen: the device library implements the single-precision accuracy of the OpenCL C
specification (exp <= 3 ulp, tanh <= 5 ulp), and an ulp is 2 U, hence K_EXP = 6 and K_TANH = 10.  An update that stays within the
specification stays within these bounds.

Worst error / bound per output over all cases of this file on an MI355X (`-s` prints them per case); `exact` = the same with
expf / tanhf counted as exact, the measurement above.  The library before the element core and the one with it give the same
figures: every output is bit for bit the same (profiles/diffusion_core_device_code.txt).

    output                                              main case      large case
                                         libm       ratio   exact   ratio   exact
    ddpm_update x0_out                              0.347   0.347   0.588   0.588
    ddpm_update mean_out                            0.378   0.378   0.432   0.432
    ddpm_update logvar_out                          0.311   0.311   0.466   0.466
    ddpm_update out                      yes        0.120   0.221   0.132   0.188
    ddim_update x0_out                              0.347   0.347   0.588   0.588
    ddim_update out                                 0.264   0.264   0.038   0.038
    ddpm_update_bwd dx                              0.862   0.862   0.456   0.456
    ddpm_update_bwd dmo                             0.770   0.770   0.660   0.660
    loss_terms_bwd mean channels                    0.615   0.615   0.750   0.750
    vlb_terms_bwd                        yes        0.003   0.005   0.005   0.007
    loss_terms_bwd variance channels     yes        0.001   0.001   0.003   0.005
(main case: flags 0 - 7, ddim_update 0 - 15; large case: one flag set per kernel.)
"""
import math

import numpy as np
import pytest
import torch

import errbound as eb
from errbound_expr import C32, K_EXP, K_TANH, V, cat, where          # (the class `V` of the docstring lives in tests/errbound_expr.py)
from helpers import rel_l2

pytestmark = pytest.mark.gpu

U = eb.U32
LN2 = math.log(2.0)


# ------------------------------------------------------------------ schedule, tables, inputs
T = 10
MAIN, REDUCE2, LARGE = (3, 2, 3, 5), (3, 2, 5, 100), (3, 4, 3, 32768)
T_MAIN = [0, 4, 9]
_cache = {}


def schedule(flags):
    from oracle import diffusion_ref as dref
    key = ("S", flags & 6)
    if key not in _cache:
        _cache[key] = dref.Schedule(respacing=str(T), learn_sigma=bool(flags & 4), predict_xstart=bool(flags & 2))
    return _cache[key]


def tables():
    """fp32 [7, T] coefficient rows and [3, T] DDIM rows, host copies (what the references read) and device copies"""
    if "tab" not in _cache:
        S = schedule(0)
        tab = np.stack([S.sqrt_recip_ac, S.sqrt_recipm1_ac, S.post_c1, S.post_c2, np.log(np.append(S.post_var[1], S.betas[1:])),
                        S.post_logvar_clipped, np.log(S.betas)])
        tab3 = np.stack([S.alphas_cumprod, S.alphas_cumprod_prev, np.append(S.alphas_cumprod[1:], 0.0)])
        tab, tab3 = torch.from_numpy(tab).float(), torch.from_numpy(tab3).float()
        _cache["tab"] = (tab, tab3, tab.cuda(), tab3.cuda())
    return _cache["tab"]


def inputs(shape, flags):
    """x0 in [-1, 1] with exact -1 / +1 entries, noise, x_t = q_sample, a model output of realistic quality, upstream gradients; shared
    by the tests of one (shape, flags) and never written to"""
    key = ("in", shape, flags & 6)
    if key not in _cache:
        from oracle import diffusion_ref as dref
        N, F, C, HW = shape
        S = schedule(flags)
        g = torch.Generator().manual_seed(1000 * (flags & 6) + HW)
        t = torch.tensor(T_MAIN)
        x0 = torch.rand(N, F, C, HW, generator=g) * 2 - 1
        x0.view(-1)[::53] = -1.0
        x0.view(-1)[29::53] = 1.0
        noise = torch.randn(N, F, C, HW, generator=g)
        xt = dref.q_sample(S, x0, t, noise)
        sb = torch.from_numpy(S.sqrt_1mac)[t].float().view(-1, 1, 1, 1)
        r = torch.randn(N, F, C, HW, generator=g)
        mo = (x0 + 0.3 * sb * r) if flags & 2 else (noise + 0.2 * r)
        if flags & 4:
            mo = torch.cat([mo, 0.6 * torch.randn(N, F, C, HW, generator=g)], dim=2)
        d = dict(t=t, x0=x0, noise=noise, xt=xt, mo=mo.contiguous(), z=torch.randn(N, F, C, HW, generator=g),
                 dmse=torch.linspace(0.5, 1.5, N), dvb=torch.linspace(1.25, 0.75, N))
        d["cuda"] = {k: v.cuda() for k, v in d.items()}
        _cache[key] = d
    return _cache[key]


def rows(t):
    tab = tables()[0].double()
    return [V(tab[r][t].view(-1, 1, 1, 1)) for r in range(7)]


def core(flags, mo, x, t, clamp):
    """the element core in V arithmetic -> (rows, o, logvar, px0, mean)"""
    C = x.shape[2]
    k = rows(t)
    cr, crm1, c1, c2, fixed, lo, hi = k
    o, xv = V(mo[:, :, :C]), V(x)
    if flags & 4:
        frac = (V(mo[:, :, C:]) + 1.0).exact(0.5)
        logvar = frac * hi + (1.0 - frac) * lo
    else:
        logvar = fixed.expand_as(xv.v)
    px0 = o if flags & 2 else cr * xv - crm1 * o
    if clamp and flags & 1:
        px0 = px0.clamp(-1.0, 1.0)
    return k, o, logvar, px0, c1 * px0 + c2 * xv


def oracle_pmv(flags, mo, x, t, clip):
    from oracle import diffusion_ref as dref
    return tuple(r.double() for r in dref.p_mean_variance(schedule(flags), mo.double(), x.double(), t, 2, clip=clip))      # (a fixed log-variance is a table value)


def agree(v, ref, what):
    """the V restatement IS the oracle's expression: equal in float64 up to its own rounding"""
    scale = float(ref.abs().max().clamp_min(1e-300))
    assert float((v.v - ref).abs().max()) <= 1e-9 * scale, (what, float((v.v - ref).abs().max()), scale)


def check(y, ref, v, what, skip=None):
    """zero elements of the kernel output y outside v's bound around the oracle's ref; returns the worst error / bound"""
    y, ref, b = (a.reshape(-1, a.shape[-1]) for a in (y.detach().cpu(), ref, v.bound()))
    if skip is not None:
        skip = skip.reshape(y.shape)
        assert int(skip.sum()) <= max(2, y.numel() // 1000), (what, int(skip.sum()))
        y, ref = torch.where(skip, ref.float(), y), ref
    worst = eb.check(y, ref, b, what=what)
    print(f"{what}: worst error / bound {worst:.3f}")
    return worst


def nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda")


def vb_oracle(flags, mo, x0, xt, t, clip, dt, detach_mean=False):
    """per-sample variational bound in bits (dref: _vb_terms_bpd restated in training_losses) in dtype dt -> vb [N], pred_x0"""
    from oracle import diffusion_ref as dref
    S = schedule(flags)
    C = x0.shape[2]
    mo, x0, xt = mo.to(dt), x0.to(dt), xt.to(dt)
    if detach_mean and flags & 4:
        mo = torch.cat([mo[:, :, :C].detach(), mo[:, :, C:]], dim=2)
    elif detach_mean:
        mo = mo.detach()
    mean, logvar, px0 = dref.p_mean_variance(S, mo, xt, t, 2, clip=clip)
    tmean, _, tlv = dref.q_posterior(S, x0, xt, t)
    logvar, tlv = logvar.to(dt), tlv.to(dt)               # (table values come back as fp32)
    kl = dref._mean_flat(dref._normal_kl(tmean, tlv, mean, logvar)) / LN2
    nll = dref._mean_flat(-dref._disc_gauss_ll(x0, mean, 0.5 * logvar)) / LN2
    return torch.where(t == 0, nll, kl), px0


# ------------------------------------------------------------------ runners: one call of an entry point on the shared inputs
def run_ddpm_update(shape, flags, optional=True, sample=True):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    tab = tables()[2]
    out = nan_like(shape) if sample else None
    opt = {k: nan_like(shape) for k in ("x0_out", "mean_out", "logvar_out")} if optional else {}
    ops.ddpm_update(d["xt"], d["mo"], d["z"] if sample else None, out, tab, d["t"], F, C, HW, flags, **opt)
    return dict(out=out, **opt)


def run_ddim_update(shape, flags, optional=True):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    out, x0o = nan_like(shape), (nan_like(shape) if optional else None)
    ops.ddim_update(d["xt"], d["mo"], d["z"], out, tables()[2], tables()[3], d["t"], F, C, HW, flags, 0.5, x0_out=x0o)
    return dict(out=out, x0_out=x0o)


def run_ddpm_update_bwd(shape, flags):
    from mm_diffusion import ops
    d = inputs(shape, flags)["cuda"]
    dx, dmo = nan_like(shape), nan_like(shape)
    ops.ddpm_update_bwd(d["xt"], d["mo"], d["z"], dx, dmo, tables()[2], d["t"], flags)
    return dict(dx=dx, dmo=dmo)


def run_loss_terms(shape, flags, vb_scale=1.0):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    target = d["x0"] if flags & 2 else d["noise"]
    mse, vb = ops.loss_terms(d["mo"], target, tables()[2], d["t"], F, C, HW, flags, x0=d["x0"] if flags & 4 else None,
                             xt=d["xt"] if flags & 4 else None, vb_scale=vb_scale)
    return dict(mse=mse, vb=vb)


def run_loss_terms_bwd(shape, flags, vb_scale=0.25):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    target = d["x0"] if flags & 2 else d["noise"]
    g = torch.full_like(d["mo"], float("nan"))
    ops.loss_terms_bwd(d["mo"], target, tables()[2], d["t"], F, C, HW, flags, d["dmse"], d["dvb"] if flags & 4 else None, g,
                       x0=d["x0"] if flags & 4 else None, xt=d["xt"] if flags & 4 else None, vb_scale=vb_scale)
    return dict(g=g)


def run_vlb_terms(shape, flags, optional=True):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    vb = torch.full((N,), float("nan"), device="cuda")
    xs, em = (torch.full((N,), float("nan"), device="cuda") if optional else None for _ in range(2))
    px0 = nan_like(shape) if optional else None
    ops.vlb_terms(d["x0"], d["xt"], d["mo"], tables()[2], d["t"], F, C, HW, flags, vb, xstart_mse=xs, eps_mse=em,
                  noise=d["noise"] if optional else None, pred_xstart=px0)
    return dict(vb=vb, xstart_mse=xs, eps_mse=em, pred_xstart=px0)


def run_vlb_terms_bwd(shape, flags):
    from mm_diffusion import ops
    N, F, C, HW = shape
    d = inputs(shape, flags)["cuda"]
    g = torch.full_like(d["mo"], float("nan"))
    ops.vlb_terms_bwd(d["x0"], d["xt"], d["mo"], tables()[2], d["t"], F, C, HW, flags, d["dvb"], g)
    return dict(g=g)


# ------------------------------------------------------------------ ddpm_update / ddim_update
def ddpm_update_check(shape, flags):
    d = inputs(shape, flags)
    t = d["t"]
    got = run_ddpm_update(shape, flags)
    mean_r, logvar_r, x0_r = oracle_pmv(flags, d["mo"], d["xt"], t, bool(flags & 1))
    nz = (t != 0).view(-1, 1, 1, 1)
    out_r = mean_r + nz.double() * torch.exp(0.5 * logvar_r) * d["z"].double()
    _, _, logvar, px0, mean = core(flags, d["mo"], d["xt"], t, clamp=True)
    out = mean + where(nz, logvar.exact(0.5).exp() * V(d["z"]), 0.0)
    worst = {}
    for name, v, ref in (("x0_out", px0, x0_r), ("mean_out", mean, mean_r), ("logvar_out", logvar, logvar_r.expand_as(mean_r)), ("out", out, out_r)):
        agree(v, ref, name)
        worst[name] = check(got[name], ref, v, f"ddpm_update flags {flags} {name}")
    return got, worst


@pytest.mark.parametrize("flags", range(8))
def test_ddpm_update(flags):
    got, _ = ddpm_update_check(MAIN, flags)
    # the optional outputs absent, then the sample absent: what remains is bit for bit what it was
    assert torch.equal(run_ddpm_update(MAIN, flags, optional=False)["out"], got["out"])
    rest = run_ddpm_update(MAIN, flags, sample=False)
    assert all(torch.equal(rest[k], got[k]) for k in ("x0_out", "mean_out", "logvar_out"))


def test_ddpm_update_large():
    ddpm_update_check(LARGE, 5)


def ddim_update_check(shape, flags):
    d = inputs(shape, flags)
    t = d["t"]
    got = run_ddim_update(shape, flags)
    _, _, x0_r = oracle_pmv(flags, d["mo"], d["xt"], t, bool(flags & 1))
    (cr, crm1, *_), _, _, px0, _ = core(flags, d["mo"], d["xt"], t, clamp=True)
    tab3 = tables()[1].double()
    ab, ap, an = (V(tab3[r][t].view(-1, 1, 1, 1)) for r in range(3))
    xv = V(d["xt"])
    eps = (cr * xv - px0) / crm1
    x0d, xd, epsd = x0_r, d["xt"].double(), None
    epsd = (cr.v * xd - x0d) / crm1.v
    if flags & 8:         # ddim_reverse_sample (gd:903-953)
        out = px0 * an.sqrt() + (1.0 - an).sqrt() * eps
        out_r = x0d * an.v.sqrt() + (1 - an.v).sqrt() * epsd
    else:                 # oracle/diffusion_ref.py: ddim_sample's expressions, in float64
        sigma = V(0.5) * ((1.0 - ap) / (1.0 - ab)).sqrt() * (1.0 - ab / ap).sqrt()
        out = px0 * ap.sqrt() + (1.0 - ap - sigma * sigma).sqrt() * eps + where((t != 0).view(-1, 1, 1, 1), sigma * V(d["z"]), 0.0)
        sg = 0.5 * torch.sqrt((1 - ap.v) / (1 - ab.v)) * torch.sqrt(1 - ab.v / ap.v)
        out_r = x0d * torch.sqrt(ap.v) + torch.sqrt(1 - ap.v - sg ** 2) * epsd + (t != 0).double().view(-1, 1, 1, 1) * sg * d["z"].double()
    agree(px0, x0_r, "x0")
    agree(out, out_r, "out")
    check(got["x0_out"], x0_r, px0, f"ddim_update flags {flags} x0_out")
    check(got["out"], out_r, out, f"ddim_update flags {flags} out")
    return got


@pytest.mark.parametrize("flags", range(16))
def test_ddim_update(flags):
    got = ddim_update_check(MAIN, flags)
    assert torch.equal(run_ddim_update(MAIN, flags, optional=False)["out"], got["out"])


def test_ddim_update_large():
    ddim_update_check(LARGE, 5)


# ------------------------------------------------------------------ ddpm_update_bwd
def ddpm_update_bwd_check(shape, flags):
    d = inputs(shape, flags)
    t = d["t"]
    got = run_ddpm_update_bwd(shape, flags)
    (cr, crm1, c1, c2, *_), _, _, px0, _ = core(flags, d["mo"], d["xt"], t, clamp=False)
    inside = (px0.v >= -1) & (px0.v <= 1) if flags & 1 else torch.ones_like(px0.v, dtype=torch.bool)
    undecided = ((px0.v.abs() - 1).abs() <= px0.bound()) if flags & 1 else None
    g = V(d["z"])
    dx = g * (c2.expand_as(g.v) if flags & 2 else where(inside, c1 * cr, 0.0) + c2)
    dmo = g * where(inside, c1 if flags & 2 else -(c1 * crm1), 0.0)
    # float64 autograd through the oracle's posterior mean
    x, mo = d["xt"].double().requires_grad_(), d["mo"].double().requires_grad_()
    mean, _, _ = oracle_pmv(flags, mo, x, t, bool(flags & 1))
    (mean * d["z"].double()).sum().backward()
    agree(dx, x.grad, "dx")
    agree(dmo, mo.grad, "dmo")
    check(got["dx"], x.grad, dx, f"ddpm_update_bwd flags {flags} dx", skip=undecided)
    check(got["dmo"], mo.grad, dmo, f"ddpm_update_bwd flags {flags} dmo", skip=undecided)


@pytest.mark.parametrize("flags", range(8))
def test_ddpm_update_bwd(flags):
    from mm_diffusion import _hip as H
    if flags & 4:
        from mm_diffusion import ops
        d = inputs(MAIN, flags & 3)["cuda"]
        with pytest.raises(H.MMDError, match="learned variance"):
            ops.ddpm_update_bwd(d["xt"], d["mo"], d["z"], nan_like(MAIN), nan_like(MAIN), tables()[2], d["t"], flags)
        return
    ddpm_update_bwd_check(MAIN, flags)


def test_ddpm_update_bwd_large():
    ddpm_update_bwd_check(LARGE, 1)


# ------------------------------------------------------------------ loss_terms and its gradient
@pytest.mark.parametrize("shape", [MAIN, REDUCE2], ids=["main", "per1000"])
@pytest.mark.parametrize("flags", range(8))
def test_loss_terms(shape, flags):
    d = inputs(shape, flags)
    C = shape[2]
    for vb_scale in (1.0, 0.25):
        got = run_loss_terms(shape, flags, vb_scale)
        target = d["x0"] if flags & 2 else d["noise"]
        mse_r = ((target.double() - d["mo"].double()[:, :, :C]) ** 2).flatten(1).mean(1)
        np.testing.assert_allclose(got["mse"].cpu().numpy(), mse_r.numpy(), rtol=1e-5)
        if flags & 4:
            vb_r, _ = vb_oracle(flags, d["mo"], d["x0"], d["xt"], d["t"], False, torch.float64)          # clip_denoised=False in the vb term
            np.testing.assert_allclose(got["vb"].cpu().numpy(), (vb_r * vb_scale).numpy(), rtol=2e-4, atol=1e-6)
        else:
            assert got["vb"] is None


def cdf(u):
    return (1.0 + (C32(math.sqrt(2.0 / math.pi)) * (u + C32(0.044715) * u * u * u)).tanh()).exact(0.5)


def term_grad(t, x0f, mean, tmean, logvar, post_log):
    """vlb_term_grad in V arithmetic -> (d term / d logvar, d term / d mean)"""
    # KL(q || p)
    dm = tmean - mean
    e2 = (-logvar).exp()
    kl_lv, kl_mean = (1.0 - (post_log - logvar).exp() - dm * dm * e2).exact(0.5), -(dm * e2)
    # decoder NLL
    x0 = V(x0f)
    cx, inv = x0 - mean, logvar.exact(-0.5).exp()
    c255 = C32(1.0 / 255.0)
    up, um = inv * (cx + c255), inv * (cx - c255)
    cp, cm = cdf(up), cdf(um)
    k, a = C32(math.sqrt(2.0 / math.pi)), C32(0.044715)

    def pdf(u):
        th = (k * (u + a * u * u * u)).tanh()
        return (1.0 - th * th).exact(0.5) * k * (1.0 + 3.0 * a * u * u)

    pp, pm = pdf(up), pdf(um)
    dp, dn = pp * up.exact(-0.5), pm * um.exact(-0.5)
    ep, en = pp * -inv, pm * -inv
    lo_edge, hi_edge = x0f < -0.999, x0f > 0.999
    den = where(lo_edge, cp, where(hi_edge, 1.0 - cm, cp - cm))
    num_lv = where(lo_edge, dp, where(hi_edge, -dn, dp - dn))
    num_mean = where(lo_edge, ep, where(hi_edge, -en, ep - en))
    live = den.v > 1e-12
    nll_lv, nll_mean = where(live, -(num_lv / den), 0.0), where(live, -(num_mean / den), 0.0)
    t0 = (t == 0).view(-1, 1, 1, 1)
    return where(t0, nll_lv, kl_lv), where(t0, nll_mean, kl_mean)


def loss_terms_bwd_check(shape, flags, vb_scale=0.25):
    d = inputs(shape, flags)
    N, F, C, HW = shape
    t, per = d["t"], F * C * HW
    got = run_loss_terms_bwd(shape, flags, vb_scale)["g"]
    target = d["x0"] if flags & 2 else d["noise"]
    (cr, crm1, c1, c2, _, lo, hi), o, logvar, px0, mean = core(flags, d["mo"], d["xt"], t, clamp=False)
    dmse, dvb = (V(d[k].double().view(-1, 1, 1, 1)) for k in ("dmse", "dvb"))
    g = dmse.exact(2.0) * (o - V(target)) / float(per)
    if flags & 4:
        dterm, _ = term_grad(t, d["x0"], mean, c1 * V(d["x0"]) + c2 * V(d["xt"]), logvar, lo)
        g_var = dvb * vb_scale / (V(float(per)) * C32(LN2)) * dterm * (hi - lo).exact(0.5)
    # float64 autograd through the oracle: sum dmse mse + dvb vb_scale vb, the vb term on the detached mean
    mo = d["mo"].double().requires_grad_()
    loss = (d["dmse"].double() * ((target.double() - mo[:, :, :C]) ** 2).flatten(1).mean(1)).sum()
    if flags & 4:
        loss = loss + (d["dvb"].double() * vb_scale * vb_oracle(flags, mo, d["x0"], d["xt"], t, False, torch.float64, detach_mean=True)[0]).sum()
    loss.backward()
    agree(g, mo.grad[:, :, :C], "g mean channels")
    check(got[:, :, :C], mo.grad[:, :, :C], g, f"loss_terms_bwd flags {flags} mean channels")
    if flags & 4:
        agree(g_var, mo.grad[:, :, C:], "g variance channels")
        check(got[:, :, C:], mo.grad[:, :, C:], g_var, f"loss_terms_bwd flags {flags} variance channels")


@pytest.mark.parametrize("flags", range(8))
def test_loss_terms_bwd(flags):
    loss_terms_bwd_check(MAIN, flags)


def test_loss_terms_bwd_large():
    loss_terms_bwd_check(LARGE, 4)


# ------------------------------------------------------------------ vlb_terms and its gradient
def vlb_yardstick(shape, flags, dt):
    """vb, xstart_mse, eps_mse, pred_xstart of vlb_terms from the oracle's functions in dtype dt"""
    d = inputs(shape, flags)
    S = schedule(flags)
    from oracle import diffusion_ref as dref
    vb, px0 = vb_oracle(flags, d["mo"], d["x0"], d["xt"], d["t"], bool(flags & 1), dt)
    eps = dref.predict_eps_from_xstart(S, d["xt"].to(dt), d["t"], px0)
    return vb, dref._mean_flat((px0 - d["x0"].to(dt)) ** 2), dref._mean_flat((eps - d["noise"].to(dt)) ** 2), px0


def worst_of(a, ref):
    """test_vlb_gpu.py's metric: largest error over the samples relative to the largest float64 value among them; rel-L2 for a tensor"""
    if a.dim() > 1:
        return rel_l2(a, ref)
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("shape", [MAIN, REDUCE2], ids=["main", "per1000"])
@pytest.mark.parametrize("flags", range(8))
def test_vlb_terms(shape, flags):
    t = inputs(shape, flags)["t"]
    got = run_vlb_terms(shape, flags)
    r64, r32 = vlb_yardstick(shape, flags, torch.float64), vlb_yardstick(shape, flags, torch.float32)
    fails = []
    for name, r32_, r64_ in zip(("vb", "xstart_mse", "eps_mse", "pred_xstart"), r32, r64):
        g_ = got[name].cpu()
        for gname, sel in ([("all", slice(None))] if g_.dim() > 1 else [("t=0", t == 0), ("t>0", t != 0)]):
            e_k, e_y = worst_of(g_[sel], r64_[sel]), worst_of(r32_[sel], r64_[sel])
            print(f"vlb_terms flags {flags} {name} {gname}: kernel {e_k:.3e}  fp32-on-CPU yardstick {e_y:.3e}")
            if not (torch.isfinite(g_).all() and e_k <= 2 * e_y):
                fails.append((name, gname, e_k, e_y))
    assert not fails, fails
    # the optional results absent: the bound itself is bit for bit what it was
    assert torch.equal(run_vlb_terms(shape, flags, optional=False)["vb"], got["vb"])


def vlb_terms_bwd_check(shape, flags):
    d = inputs(shape, flags)
    N, F, C, HW = shape
    t, per = d["t"], F * C * HW
    got = run_vlb_terms_bwd(shape, flags)["g"]
    (cr, crm1, c1, c2, _, lo, hi), o, logvar, px0, mean = core(flags, d["mo"], d["xt"], t, clamp=False)
    dterm, dmean = term_grad(t, d["x0"], mean, c1 * V(d["x0"]) + c2 * V(d["xt"]), logvar, lo)
    w = V(d["dvb"].double().view(-1, 1, 1, 1)) / (V(float(per)) * C32(LN2))
    g = w * dmean * c1 if flags & 2 else w * dmean * c1 * -crm1
    if flags & 4:
        g = cat(g, w * dterm * (hi - lo).exact(0.5), 2)
    mo = d["mo"].double().requires_grad_()
    (d["dvb"].double() * vb_oracle(flags, mo, d["x0"], d["xt"], t, False, torch.float64)[0]).sum().backward()
    agree(g, mo.grad, "g")
    return check(got, mo.grad, g, f"vlb_terms_bwd flags {flags}")


@pytest.mark.parametrize("flags", range(8))
def test_vlb_terms_bwd(flags):
    from mm_diffusion import _hip as H
    if flags & 1:
        with pytest.raises(H.MMDError, match="clip"):
            run_vlb_terms_bwd(MAIN, flags)
        return
    vlb_terms_bwd_check(MAIN, flags)


def test_vlb_terms_bwd_large():
    vlb_terms_bwd_check(LARGE, 6)
