"""CPU proof of tests/errbound_small.py, following tests/test_errbound_fwd_cpu.py (no GPU, no libmmd kernel):

1. The float64 references equal torch's own float64 operators (F.linear, F.silu and its autograd, torch.optim.AdamW in float64,
   permute) to 1e-12 on every case of the lists the GPU file iterates over, and the values `V` carries equal the references.
2. An fp32 emulation of each kernel - torch fp32 arithmetic, the sums in the kernel's own order where the bound depends on it (temb: one
   sequential chain per output; linear: 64 strided chains and the xor butterfly), one round-to-nearest store - has ZERO violating
   elements on every GPU case, the second-trip sizes included.  That is the evidence that the bounds are not too tight; it held before
   anything ran on a GPU.  The bit-exact kernels (dropout, cast, pack, unpack) are emulated by the expression the GPU file compares with.
   No element of any case is excused: clamp_scale and dropout decide on exact inputs, and dpm_err's maximum is bounded without a branch.
3. Seeded defects, each flagged by `check` or by the equality - except the one that must not be.  DEFECT_LOG records for each whether the
   assertion that holds its kernel today would have passed the same emulated output: test_ops_gpu.py::test_temb_and_linear (rel-L2 <
   2e-5, dim 128, N = 5), test_bwd_gpu.py::test_small_ops_backward (rel-L2 < 5e-5 fp32; the suite's 1e-2 in bf16),
   test_bwd_gpu.py::test_adamw_step (rel-L2 of p and the EMA < 1e-6 after three steps at n = 1000),
   test_round6_gpu.py::test_weight_pack_and_grad_unpack_tiles (equality on its nine shapes); `none` = no assertion reaches the kernel.
   Output of test_defects_todays_assertions_pass (`pytest -s`):

       defect                                                                  error     today's assertion
       emb: sine and cosine halves swapped                                     4.5e-01   fails (2e-5)
       emb: frequency exponent k / (half - 1)                                  2.6e-01   fails (2e-5)
       emb: float t truncated to an integer                                    2.2e-02   fails (2e-5)
       linear: drops the sample at index 8                                     8.0e-08   PASSES (2e-5: N = 5 has no index 8)
       linear: adds the bias once per lane                                     5.6e+00   fails (2e-5)
       silu': no x (1 - sg) term on one vector lane                            1.3e-01   fails (5e-5)
       silu bf16: truncating store                                             5.9e-04   PASSES (1e-2)
       cast: NaN with the sign bit becomes 0                                   -         PASSES (none)
       adamw: eps inside the square root                                       9.8e-06   fails (1e-6; flagged here where eps decides, g ~ 1e-9)
       adamw: bias correction of v omitted at step 100000                      -         (not a defect there: must not be flagged, and is not)
       adamw: bias correction of v omitted at step 2                           2.2e-01   fails (1e-6)
       adamw: EMA reads the parameter from before the step                     3.0e-04   fails (1e-6)
       adamw: v not stored                                                     3.7e-03   fails (1e-6)
       pack: tail Cin tile written at the full tile width                      -         fails (equality)
       pack: taps of the 6-wide tile interleaved with tstep = 64 / 8           -         PASSES (equality: its shapes have no 6-wide tile)
       pack: second trip of the descriptor search skipped                      -         PASSES (equality: nine descriptors)
       unpack: packed buffer not cleared                                       -         fails (equality)
       lincomb: third term dropped when b is null                              -         PASSES (none)
       clamp_scale: no floor at 1                                              -         PASSES (none)
       dpm_err: |hi| in place of |prev|                                        -         PASSES (none)
"""
import pytest
import torch
import torch.nn.functional as F_

import errbound as E
import errbound_small as S
from errbound_expr import V
from helpers import CONFIGS, rel_l2

F32, BF16 = torch.float32, torch.bfloat16
DEFECT_LOG = {}


def _close12(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _ok(y, ref, bound, what):
    return E.check(y.reshape(-1, 1) if y.dim() < 2 else y.flatten(1), ref.reshape(-1, 1) if ref.dim() < 2 else ref.flatten(1),
                   bound.reshape(-1, 1) if bound.dim() < 2 else bound.flatten(1), what=what)


def _flagged(y, ref, bound):
    return E.violations(y, ref, bound)[0] > 0


def _log(name, err, passes, note):
    DEFECT_LOG[name] = (err, passes)
    e = "-      " if err is None else f"{err:.1e}"
    print(f"\nDEFECT {name:<70s}  {e}   {'PASSES' if passes else 'fails'} ({note})")


# ----------------------------------------------------------------------------- 1 + 2: references and emulations
def test_embedding_dims_cover_the_shipped_configurations():
    from mm_diffusion import multimodal_script_util as msu, script_util as su
    shipped = {msu.model_and_diffusion_defaults()["num_channels"], su.image_sr_model_and_diffusion_defaults()["sr_num_channels"]}
    shipped |= {c["num_channels"] for c in CONFIGS.values()}
    assert shipped <= set(S.EMB_DIMS), shipped


@pytest.mark.parametrize("dim", S.EMB_DIMS)
def test_embedding_and_temb(dim):
    from oracle import unet_ref as uref
    W = S.temb_weights(dim)
    for d, N, kind in S.emb_cases():
        if d != dim:
            continue
        t = S.emb_t(kind, N)
        ref, e = S.emb_ref(t, dim), S.emb_V(t, dim)
        _close12(e.v, ref)
        _ok(S.emu_emb(t, dim), ref, e.bound(), f"emb {dim} {N} {kind}")
        _ok(uref.timestep_embedding(t, dim).float(), ref, e.bound(), f"oracle emb {dim} {N} {kind}")          # the reference model's own fp32 statement
        z = t == 0
        if z.any():
            half = dim // 2
            exact = torch.cat([torch.ones(half), torch.zeros(dim - half)])
            assert torch.equal(S.emu_emb(t, dim)[z], exact.expand(int(z.sum()), -1))
        raw, Eraw, out, Eout = S.temb_ref(t, dim, *W)
        W64 = [w.double() for w in W]
        lib = F_.linear(F_.silu(F_.linear(ref, W64[0], W64[1])), W64[2], W64[3])
        _close12(raw, lib)
        _close12(out, F_.silu(lib))
        eraw, eout = S.emu_temb(t, dim, *W)
        _ok(eraw, raw, Eraw, f"temb raw {dim} {N} {kind}")
        _ok(eout, out, Eout, f"temb silu {dim} {N} {kind}")


@pytest.mark.parametrize("case", S.linear_cases(), ids=lambda c: c[0])
def test_linear(case):
    name, N, K, J, bias, bwd = case
    x, W, b = S.linear_inputs(N, K, J, bias, bwd)
    ref, bound = S.linear_ref(x, W, b)
    _close12(ref, F_.linear(x.double(), W.double(), None if b is None else b.double()))
    _ok(S.emu_linear(x, W, b), ref, bound, name)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_silu(dtype):
    for n in S.ew_sizes(dtype):
        x, dy = S.silu_inputs(n, dtype)
        ref, bound = S.silu_ref(x, None, dtype)
        rb, bb = S.silu_ref(x, dy, dtype)
        if n <= 8 * 37:
            xd = x.double().requires_grad_()
            y = F_.silu(xd)
            _close12(ref, y.detach())
            y.backward(dy.double())
            _close12(rb, xd.grad)
        yf, yb = S.emu_silu(x, None, dtype), S.emu_silu(x, dy, dtype)
        assert torch.isfinite(yf.float()).all() and torch.isfinite(yb.float()).all()          # __expf overflows at +-88.7: the finite limit, not NaN
        _ok(yf, ref, bound, f"silu fwd {n}")
        _ok(yb, rb, bb, f"silu bwd {n}")


def test_mse_grad():
    for per in (30, 1000):
        out, target, w = S.mse_inputs(per)
        ref, bound, v = S.mse_grad_ref(out, target, w)
        _close12(v, ref)
        od = out.double().requires_grad_()
        (w.double() * ((target.double() - od) ** 2).mean(1)).sum().backward()
        _close12(ref, od.grad)
        _ok(S.emu_mse_grad(out, target, w), ref, bound, f"mse_grad {per}")
        assert torch.equal(S.emu_mse_grad(out, target, w)[1], torch.zeros(per))          # weight 0: exactly 0


def test_adamw_reference_is_torch_adamw():
    """adamw_plain64 chained over three steps = torch.optim.AdamW in float64, and V's values are adamw_plain64's"""
    H = S.HYPER
    st = S.adamw_state(1000, 1.0)
    ref = torch.nn.Parameter(st["p"].double().clone())
    opt = torch.optim.AdamW([ref], lr=H["lr"], betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=S.f32(0.05))
    p, m, v = st["p"].double(), st["m"].double(), st["v"].double()
    for step in (1, 2, 3):
        g = st["g"].double() * step
        ref.grad = g.clone()
        opt.step()
        bc1, bc2 = S.bias_corrections(H["beta1"], H["beta2"], step)
        vv = S.adamw_V(p, g, m, v, [p], [0.99], wd=S.f32(0.05), bc1=bc1, bc2=bc2, **H)
        p2, m2, v2, (e2,) = S.adamw_plain64(p, g, m, v, [p], [0.99], wd=S.f32(0.05), step=step, **H)
        for k, r in (("p", p2), ("m", m2), ("v", v2), ("ema0", e2)):
            _close12(vv[k].v, r)
        p, m, v = p2, m2, v2
        _close12(p, ref.detach())
        _close12(m, opt.state[ref]["exp_avg"])
        _close12(v, opt.state[ref]["exp_avg_sq"])


def adamw_walk(n, gs, wd, n_ema, defect=None, at_step=None, clip=None):
    """the GPU test's loop with the emulation in the kernel's place: every step checked against V from the state stored before it.
    Returns the number of violating elements per (step, tensor)."""
    H = S.HYPER
    st = S.adamw_state(n, gs)
    rates = [S.f32(0.99), S.f32(0.9999), S.f32(0.5), S.f32(0.9)][:n_ema]
    emas = [st["p"].clone() for _ in rates]
    bad = {}
    for step in S.ADAM_STEPS:
        bc1, bc2 = S.bias_corrections(H["beta1"], H["beta2"], step)
        want = S.adamw_V(st["p"], st["g"], st["m"], st["v"], emas, rates, wd=wd, bc1=bc1, bc2=bc2, clip=clip, **H)
        got = S.emu_adamw(st["p"], st["g"], st["m"], st["v"], emas, rates, wd=wd, step=step, clip=clip,
                          defect=defect if at_step in (None, step) else None, **H)
        for k, w in want.items():
            bad[(step, k)] = E.violations(got[k], w.v, w.bound())[0]
        st.update(p=got["p"], m=got["m"], v=got["v"])
        emas = [got[f"ema{k}"] for k in range(n_ema)]
    return bad


@pytest.mark.parametrize("case", S.adamw_cases(), ids=lambda c: c[0])
def test_adamw(case):
    name, n, gs, wd, n_ema = case
    bad = adamw_walk(n, gs, wd, n_ema)
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
    if n == 1000:                        # the guarded kernel: a clip coefficient, four and two EMA copies
        for ne in (4, 2):
            bad = adamw_walk(n, gs, wd, ne, clip=S.f32(0.37))
            assert not any(bad.values()), {k: v for k, v in bad.items() if v}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pack_and_unpack_emulation_is_the_permutation(dtype):
    for shapes in (S.PACK_SHAPES, S.PACK_MANY):
        ws = S.pack_weights(shapes)
        want, got = S.pack_expected(ws, shapes, dtype), S.emu_pack(ws, shapes, dtype)
        assert S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1])
        if dtype == F32:
            grad, packed = S.unpack_inputs(shapes)
            wg, wp = S.unpack_expected(grad, packed, shapes)
            gg, gp = S.emu_unpack(grad, packed, shapes)
            assert S.same_bits(gg, wg) and S.same_bits(gp, wp)
            sel = [1, 3, 5]
            wg, wp = S.unpack_expected(grad, packed, shapes, sel)
            gg, gp = S.emu_unpack(grad, packed, shapes, sel)
            assert S.same_bits(gg, wg) and S.same_bits(gp, wp)
    assert S.pack_blocks(8, 8, 28) < 0 and S.pack_blocks(8, 8, 27) == 1
    assert [S.pack_ci_tile(nt) for nt in (1, 3, 5, 9, 27)] == [208, 64, 32, 16, 8]


def test_dropout_and_cast_expressions():
    """the expressions the GPU file compares with: a zero mask gives +0 whatever x is, NaNs stay NaN, ties go to even, fp32 max to inf"""
    for dtype in (F32, BF16):
        x, mask = S.dropout_inputs(8 * 37, dtype, "random")
        y = S.dropout_expr(x, mask, 1 / 0.7)
        assert y.dtype == dtype and not y[mask == 0].any() and not torch.signbit(y[mask == 0]).any()
    x = S.cast_inputs(F32, 64)
    y = S.cast_expr(x, BF16, 1.0)
    assert y.view(torch.int16)[:8].tolist() == [0x3F80, 0x3F82, 0xBF80 - 65536, 0xBF82 - 65536, 0x7F80, 0xFF80 - 65536, 0x7F80, 0xFF80 - 65536]
    assert torch.isnan(y[8:12]).all() and not torch.isnan(y[12:]).any()
    assert S.same_bits(y, y) and not S.same_bits(S.cast_expr(x, BF16, 1.0, "trunc_store"), y)


def test_solver_helpers():
    a, b, c = S.lincomb_inputs()
    for name, ca, cb, cc in S.lincomb_cases():
        args = (a, ca, b if cb is not None else None, cb, c if cc is not None else None, cc)
        ref, bound, v = S.lincomb_ref(*args)
        _close12(v, ref)
        _ok(S.emu_lincomb(*args), ref, bound, f"lincomb {name}")
    assert torch.signbit(S.emu_lincomb(torch.full((4,), -0.0), 1.0, None, 0.0, None, 0.0)).all()
    for name, per, tk, has in S.lincomb_t_cases():
        a, b, tabs, t = S.lincomb_t_inputs(per, tk)
        ref, bound, v = S.lincomb_t_ref(a, b, tabs, t, has)
        _close12(v, ref)
        _ok(S.emu_lincomb_t(a, b, tabs, t, has), ref, bound, f"lincomb_t {name}")
    for name, per, mv in S.clamp_cases():
        x, s = S.clamp_inputs(per)
        ref, bound, v = S.clamp_ref(x, s, mv)
        _close12(v, ref)
        _close12(ref, x.double().clamp(-s.double().clamp_min(1)[:, None], s.double().clamp_min(1)[:, None]) / (s.double().clamp_min(1)[:, None] / mv))
        _ok(S.emu_clamp(x, s, mv), ref, bound, f"clamp_scale {name}")
    for per in S.DPM_PERS:
        hi, lo, prev = S.dpm_err_inputs(per)
        ref, bound = S.dpm_err_ref(hi, lo, prev)
        delta = S.DPM_RTOL * torch.maximum(lo.abs(), prev.abs())
        frac = float((delta > S.DPM_ATOL).double().mean())
        assert 0.1 < frac < 0.9, frac                                          # atol- and rtol-dominated elements both occur
        _ok(S.emu_dpm_err(hi, lo, prev), ref, bound, f"dpm_err {per}")


def test_dpm_order_input_tells_the_orders_apart():
    """in float64, 2^53 + 1 + 1 is 2^53 one by one and 2^53 + 2 when the small ones meet first"""
    big = torch.tensor(2.0 ** 53, dtype=torch.float64)
    one = torch.ones((), dtype=torch.float64)
    assert float((big + one) + one) == 2.0 ** 53 and float(big + (one + one)) == 2.0 ** 53 + 2
    hi, lo, prev = S.dpm_order_inputs((128, 64))
    assert float(S.emu_dpm_err(hi, lo, prev, atol=1.0, rtol=0.0)[0]) in (2.0 ** 53, 2.0 ** 53 + 2)


# ----------------------------------------------------------------------------- 3: seeded defects
def _today_temb(emb_defect, t):
    dim = 128
    W = S.temb_weights(dim)
    raw, _, _, _ = S.temb_ref(t, dim, *W)
    return rel_l2(S.emu_temb(t, dim, *W, emb_defect=emb_defect)[0], raw)


def test_embedding_defects_are_flagged():
    ti, tf = torch.tensor([0, 1, 17, 999, 500]), torch.tensor([0.0, 0.25, 131.5, 999.0, 3.0])          # test_temb_and_linear's timesteps
    for defect, label, t in (("swap", "emb: sine and cosine halves swapped", ti), ("half_minus_1", "emb: frequency exponent k / (half - 1)", ti),
                             ("trunc_t", "emb: float t truncated to an integer", tf)):
        for dim in (128, 130):
            tt = S.emb_t("f32" if defect == "trunc_t" else "i64", 5)
            e = S.emb_V(tt, dim)
            assert _flagged(S.emu_emb(tt, dim, defect), e.v, e.bound()), label
        r = _today_temb(defect, t)
        _log(label, r, r < 2e-5, "2e-5")


def test_linear_defects_are_flagged():
    x, W, b = S.linear_inputs(9, 128, 1234, True, False)
    ref, bound = S.linear_ref(x, W, b)
    x5, W5, b5 = S.linear_inputs(5, 128, 1234, True, False)                     # today: N = 5
    ref5, _ = S.linear_ref(x5, W5, b5)
    for defect, label in (("drop_sample_8", "linear: drops the sample at index 8"), ("bias_per_lane", "linear: adds the bias once per lane")):
        assert _flagged(S.emu_linear(x, W, b, defect), ref, bound), label
        r = rel_l2(S.emu_linear(x5, W5, b5, defect), ref5)
        _log(label, r, r < 2e-5, "2e-5")


def test_silu_and_cast_defects_are_flagged():
    x, dy = S.silu_inputs(8 * 37, F32)
    ref, bound = S.silu_ref(x, dy, F32)
    y = S.emu_silu(x, dy, F32, "no_x_term_lane3")
    assert _flagged(y, ref, bound)
    r = rel_l2(y, ref)
    _log("silu': no x (1 - sg) term on one vector lane", r, r < 5e-5, "5e-5")
    x, _ = S.silu_inputs(8 * 37, BF16)
    ref, bound = S.silu_ref(x, None, BF16)
    y = S.emu_silu(x, None, BF16, "trunc_store")
    assert _flagged(y, ref, bound)
    r = rel_l2(y.float(), ref)
    _log("silu bf16: truncating store", r, r < 1e-2, "1e-2")
    x = S.cast_inputs(F32, 64)
    assert not S.same_bits(S.cast_expr(x, BF16, 1.0, "signed_nan_to_zero"), S.cast_expr(x, BF16, 1.0))
    assert not S.same_bits(S.cast_expr(x, BF16, 1.0, "trunc_store"), S.cast_expr(x, BF16, 1.0))
    _log("cast: NaN with the sign bit becomes 0", None, True, "none")


def _today_adamw(defect, at_step=None):
    """test_bwd_gpu.py::test_adamw_step with the emulation: three steps, g * step, rel-L2 of p and the EMA against float64"""
    H = S.HYPER
    st = S.adamw_state(1000, 1.0)
    wd, rate = S.f32(0.05), S.f32(0.99)
    p, m, v, ema = st["p"], st["m"], st["v"], st["p"].clone()
    pr, mr, vr, er = (a.double() for a in (p, m, v, ema))
    for step in (1, 2, 3):
        got = S.emu_adamw(p, st["g"] * step, m, v, [ema], [rate], wd=wd, step=step, defect=defect if at_step in (None, step) else None, **H)
        p, m, v, ema = got["p"], got["m"], got["v"], got["ema0"]
        pr, mr, vr, (er,) = S.adamw_plain64(pr, st["g"].double() * step, mr, vr, [er], [rate], wd=wd, step=step, **H)
    return max(rel_l2(p, pr), rel_l2(ema, er))


def test_adamw_defects_are_flagged():
    wd = S.f32(0.05)
    bad = adamw_walk(1000, 1e-9, wd, 1, "eps_in_sqrt")
    assert bad[(1, "p")] > 0
    r = _today_adamw("eps_in_sqrt")
    _log("adamw: eps inside the square root", r, r < 1e-6, "1e-6")
    bad = adamw_walk(1000, 1.0, wd, 1, "no_bc2", at_step=100000)
    assert not any(bad.values()), "beta2^100000 is below the bound: omitting the correction there is not an error"
    DEFECT_LOG["adamw: bias correction of v omitted at step 100000"] = (None, None)
    bad = adamw_walk(1000, 1.0, wd, 1, "no_bc2", at_step=2)
    assert bad[(2, "p")] > 0 and bad[(1, "p")] == 0
    r = _today_adamw("no_bc2", at_step=2)
    _log("adamw: bias correction of v omitted at step 2", r, r < 1e-6, "1e-6")
    bad = adamw_walk(1000, 1.0, wd, 1, "ema_old_p")
    assert bad[(1, "ema0")] > 0 and bad[(1, "p")] == 0
    r = _today_adamw("ema_old_p")
    _log("adamw: EMA reads the parameter from before the step", r, r < 1e-6, "1e-6")
    bad = adamw_walk(1000, 1.0, wd, 1, "v_not_stored")
    assert bad[(1, "v")] > 0 and bad[(1, "p")] == 0
    r = _today_adamw("v_not_stored")
    _log("adamw: v not stored", r, r < 1e-6, "1e-6")


def _pack_equal(shapes, defect, dtype=F32):
    ws = S.pack_weights(shapes)
    want, got = S.pack_expected(ws, shapes, dtype), S.emu_pack(ws, shapes, dtype, defect)
    return S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1])


def test_pack_defects_are_flagged():
    for defect, label, shapes in (("tail_full", "pack: tail Cin tile written at the full tile width", S.PACK_SHAPES),
                                  ("tstep8", "pack: taps of the 6-wide tile interleaved with tstep = 64 / 8", S.PACK_SHAPES),
                                  ("one_trip", "pack: second trip of the descriptor search skipped", S.PACK_MANY)):
        assert not _pack_equal(shapes, defect), label
        _log(label, None, _pack_equal(S.PACK_TODAY, defect), "equality")
    grad, packed = S.unpack_inputs(S.PACK_SHAPES)
    wg, wp = S.unpack_expected(grad, packed, S.PACK_SHAPES)
    gg, gp = S.emu_unpack(grad, packed, S.PACK_SHAPES, defect="no_clear")
    assert S.same_bits(gg, wg) and not S.same_bits(gp, wp)
    _log("unpack: packed buffer not cleared", None, False, "equality: test_weight_pack_and_grad_unpack_tiles looks at the buffer")


def test_solver_helper_defects_are_flagged():
    a, b, c = S.lincomb_inputs()
    name, ca, cb, cc = next(k for k in S.lincomb_cases() if k[0] == "row0-ac")
    ref, bound, _ = S.lincomb_ref(a, ca, None, None, c, cc)
    assert _flagged(S.emu_lincomb(a, ca, None, None, c, cc, "drop_c_without_b"), ref, bound)
    _log("lincomb: third term dropped when b is null", None, True, "none")
    x, s = S.clamp_inputs(30)
    ref, bound, _ = S.clamp_ref(x, s, 1.0)
    y = S.emu_clamp(x, s, 1.0, "no_floor")
    bad = E.violations(y, ref, bound)[2]
    assert bad[0].any() and not bad[1:].any()                                  # only the sample with s < 1
    _log("clamp_scale: no floor at 1", None, True, "none")
    hi, lo, prev = S.dpm_err_inputs(4096)
    ref, bound = S.dpm_err_ref(hi, lo, prev)
    assert _flagged(S.emu_dpm_err(hi, lo, prev, defect="hi_for_prev"), ref, bound)
    _log("dpm_err: |hi| in place of |prev|", None, True, "none")


PASSES_TODAY = {"linear: drops the sample at index 8", "silu bf16: truncating store", "cast: NaN with the sign bit becomes 0",
                "pack: taps of the 6-wide tile interleaved with tstep = 64 / 8",
                "pack: second trip of the descriptor search skipped", "lincomb: third term dropped when b is null",
                "clamp_scale: no floor at 1", "dpm_err: |hi| in place of |prev|"}


def test_defects_todays_assertions_pass():
    """Exactly the eight defects of PASSES_TODAY pass what holds their kernel today (the table of the module docstring); the log is
    computed here, whatever ran before."""
    DEFECT_LOG.clear()
    for t in (test_embedding_defects_are_flagged, test_linear_defects_are_flagged, test_silu_and_cast_defects_are_flagged,
              test_adamw_defects_are_flagged, test_pack_defects_are_flagged, test_solver_helper_defects_are_flagged):
        t()
    assert len(DEFECT_LOG) == 20, sorted(DEFECT_LOG)
    assert {k for k, (_, ok) in DEFECT_LOG.items() if ok} == PASSES_TODAY, DEFECT_LOG
