"""The small kernels that were held only by whole-tensor rel-L2, element by element against float64 or bit for bit
(tests/errbound_small.py: the references, the bounds and their derivation, the fp32 emulations, the case lists;
tests/test_errbound_small_cpu.py: the bounds proven on the CPU and on seeded defects):

    mmd_misc.hip        mmd_timestep_embedding, mmd_temb_fwd, mmd_linear_fwd (forward and the backward use with W^T), mmd_cast,
                        mmd_silu (forward and `dy` form), mmd_dropout, mmd_mse_grad
    mmd_optim.hip       mmd_adamw_step, mmd_adamw_step_guarded (behind mmd_sumsq_chunks + mmd_step_control), mmd_pack_conv_weights,
                        mmd_unpack_conv_grads, mmd_pack_blocks
    mmd_diffusion.hip   mmd_lincomb, mmd_lincomb_t
    mmd_dpm.hip         mmd_clamp_scale, mmd_dpm_err

Every case calls the kernel through mm_diffusion.ops (H.call for the pack pair, as optim.WeightPacker does) with NaN-prefilled outputs,
builds the reference with torch double ops - never with a libmmd kernel - and admits ZERO elements outside the per-element bound.
dropout, cast, pack and unpack hold as equalities of bits; a NaN stays a NaN.  AdamW is checked ONE step at a time from the state the
kernel stored before it.  mmd_dpm_err's sum is held to a fixed order (test_dpm_err_order).

Worst error / bound ratio over the cases of each kernel, as printed at the end of the module (`-s`) on an MI355X (a record of
headroom, not a tolerance); `exact` = the same with sinf / cosf counted as exact (K_SIN = K_COS = 0), the measurement of the minimal
count reported in tests/errbound_expr.py:

    kernel                                    dtype      cases   worst ratio   exact
    timestep_embedding                        f32           45         0.116   0.177
    temb_fwd out_raw / out_silu               f32           45   0.038 / 0.040   0.047
    linear_fwd                                f32           48         0.011
    linear_fwd, backward use (W^T, K = 1234)  f32            1         0.000 (< 0.0005)
    silu forward                              f32 / bf16   3 / 3   0.781 / 0.996
    silu `dy` form                            f32 / bf16   3 / 3   0.265 / 0.996
    mse_grad                                  f32            2         0.854
    adamw_step p / m / v / ema                f32           52   0.139 / 0.362 / 0.394 / 0.077
    adamw_step_guarded p / m / v / ema        f32           32   0.103 / 0.324 / 0.473 / 0.086
    lincomb                                   f32           16         1.000 (one rounding: half an ulp of a value just above 2^k)
    lincomb_t                                 f32           18         0.995
    clamp_scale                               f32            4         0.489
    dpm_err                                   f64 sum        3         0.153
    dropout, cast, pack, unpack               both                     equal bit for bit

Every case: zero violating elements.  The minimal count of roundings to grant sinf / cosf is 0: with both counted as exact the worst
ratio is 0.177 (the rounding of the argument t f_k hides the library's error).  linear sits at 0.01 like every any-order sum bound
(each of K additions is granted a full U).  Run time on an MI355X: 4.1 s for the 101 cases.
"""
import pytest
import torch

import errbound as E
import errbound_small as S
from errbound_expr import U, V, C32

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    yield o
    print("\n    kernel                                    cases   worst ratio")
    for k, (n, w) in RATIOS.items():
        print(f"    {k:<42s}{n:5d}   {w:11.3f}")


def nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _2d(a):
    return a.reshape(-1, 1) if a.dim() < 2 else a.flatten(1)


def ratio(y, ref, bound):
    return E.violations(_2d(y.detach().cpu()), _2d(ref), _2d(bound))[1]


def check(group, y, ref, bound, what):
    """zero elements of y outside `bound` around `ref`; records the worst error / bound of the group"""
    worst = E.check(_2d(y.detach().cpu()), _2d(ref), _2d(bound), what=what)
    n, w = RATIOS.get(group, (0, 0.0))
    RATIOS[group] = (n + 1, max(w, worst))
    return worst


def note(group, worst):
    n, w = RATIOS.get(group, (0, 0.0))
    RATIOS[group] = (n + 1, max(w, worst))


# ----------------------------------------------------------------------------- conditioning path
@pytest.mark.parametrize("dim", S.EMB_DIMS)
def test_timestep_embedding(ops, dim):
    for d, N, kind in S.emb_cases():
        if d != dim:
            continue
        t = S.emb_t(kind, N)
        out = nan(N, dim)
        ops.timestep_embedding(t.cuda(), dim, out)
        ref, e = S.emb_ref(t, dim), S.emb_V(t, dim)
        check("timestep_embedding", out, ref, e.bound(), f"timestep_embedding {dim} {N} {kind}")
        note("timestep_embedding, sinf / cosf exact", ratio(out, ref, S.emb_V(t, dim, ksin=0).bound()))
        z = t == 0
        if z.any():                      # t = 0: exactly (1.., 0..)
            half = dim // 2
            assert torch.equal(out.cpu()[z], torch.cat([torch.ones(half), torch.zeros(dim - half)]).expand(int(z.sum()), -1))
        if dim % 2:
            assert not out[:, -1].any()


@pytest.mark.parametrize("dim", S.EMB_DIMS)
def test_temb(ops, dim):
    W = S.temb_weights(dim)
    Wc = [w.cuda() for w in W]
    for d, N, kind in S.emb_cases():
        if d != dim:
            continue
        t = S.emb_t(kind, N)
        o_s, o_r = nan(N, dim), nan(N, dim)
        ops.temb(t.cuda(), dim, *Wc, o_s, o_r)
        raw, Eraw, out, Eout = S.temb_ref(t, dim, *W)
        check("temb_fwd out_raw", o_r, raw, Eraw, f"temb raw {dim} {N} {kind}")
        check("temb_fwd out_silu", o_s, out, Eout, f"temb silu {dim} {N} {kind}")
        x = S.temb_ref(t, dim, *W, ksin=0)
        note("temb_fwd, sinf / cosf exact", max(ratio(o_r, raw, x[1]), ratio(o_s, out, x[3])))
        o2 = nan(N, dim)
        ops.temb(t.cuda(), dim, *Wc, o2)                      # out_raw absent: out_silu bit for bit what it was
        assert torch.equal(o2, o_s)


@pytest.mark.parametrize("case", S.linear_cases(), ids=lambda c: c[0])
def test_linear(ops, case):
    name, N, K, J, bias, bwd = case
    x, W, b = S.linear_inputs(N, K, J, bias, bwd)
    pad = J + 3
    buf = nan(pad + N * J + pad)                              # padded in front of and behind the output
    y = buf[pad:pad + N * J].view(N, J)
    ops.linear(x.cuda(), W.cuda(), None if b is None else b.cuda(), y)
    ref, bound = S.linear_ref(x, W, b)
    check("linear_fwd" + (" (backward use, W^T)" if bwd else ""), y, ref, bound, name)
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + N * J:]).all()


# ----------------------------------------------------------------------------- element-wise training kernels
@pytest.mark.parametrize("form", ["fwd", "dy"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_silu(ops, dtype, form):
    for n in S.ew_sizes(dtype):
        x, dy = S.silu_inputs(n, dtype)
        dy = dy if form == "dy" else None
        out = nan(n, dtype=dtype)
        ops.silu(x.cuda(), None if dy is None else dy.cuda(), out)
        ref, bound = S.silu_ref(x, dy, dtype)
        check(f"silu {form} {'f32' if dtype == F32 else 'bf16'}", out.float(), ref, bound, f"silu {form} {dtype} {n}")


@pytest.mark.parametrize("mask_kind", ["zeros", "ones", "random"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dropout_bits(ops, dtype, mask_kind):
    for n in S.ew_sizes(dtype):
        x, mask = S.dropout_inputs(n, dtype, mask_kind)
        for scale in (1.0, 1 / 0.7) if n <= 8 * 37 else (1 / 0.7,):
            out = nan(n, dtype=dtype)
            ops.dropout(x.cuda(), mask.cuda(), scale, out)
            assert S.same_bits(out, S.dropout_expr(x, mask, scale)), (n, scale)


@pytest.mark.parametrize("dst", [F32, BF16], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src", [F32, BF16], ids=["f32", "bf16"])
def test_cast_bits(ops, src, dst):
    for n in (8 * 37, S.SECOND_TRIP_VECS):
        x = S.cast_inputs(src, n)
        for scale in (1.0, 1.0 / 3.0):
            out = nan(n, dtype=dst)
            ops.cast(x.cuda(), out, scale)
            want = S.cast_expr(x, dst, scale)
            assert S.same_bits(out, want), (n, scale)
            assert not (torch.isnan(want) & ~torch.isnan(out.cpu())).any()          # a NaN never becomes inf or 0


def test_mse_grad(ops):
    for per in (30, 1000):
        out, target, w = S.mse_inputs(per)
        g = nan(3, per)
        ops.mse_grad(out.cuda(), target.cuda(), w.cuda(), g)
        ref, bound, _ = S.mse_grad_ref(out, target, w)
        check("mse_grad", g, ref, bound, f"mse_grad {per}")
        assert not g[1].any()                                # weight 0


# ----------------------------------------------------------------------------- AdamW
def _adam_check(group, dev, want, what):
    for k, w in want.items():
        check(f"{group} {k[:3]}", dev[k], w.v, w.bound(), f"{what} {k}")


@pytest.mark.parametrize("case", S.adamw_cases(), ids=lambda c: c[0])
def test_adamw_step(ops, case):
    name, n, gs, wd, n_ema = case
    H = S.HYPER
    st = S.adamw_state(n, gs)
    rate = S.f32(0.99)
    dev = {k: v.cuda() for k, v in st.items()}
    if n_ema:
        dev["ema0"] = st["p"].cuda()
    for step in S.ADAM_STEPS:
        host = {k: v.cpu() for k, v in dev.items()}          # the state the kernel stored after the step before
        emas = [host["ema0"]] if n_ema else []
        bc1, bc2 = S.bias_corrections(H["beta1"], H["beta2"], step)
        want = S.adamw_V(host["p"], host["g"], host["m"], host["v"], emas, [rate] * n_ema, wd=wd, bc1=bc1, bc2=bc2, **H)
        ops.adamw_step(dev["p"], dev["g"], dev["m"], dev["v"], dev.get("ema0"), H["lr"], H["beta1"], H["beta2"], H["eps"], wd, step, ema_rate=rate)
        _adam_check("adamw_step", dev, want, f"adamw {name} step {step}")
        assert torch.equal(dev["g"].cpu(), host["g"])


@pytest.mark.parametrize("n_ema", [4, 2])
def test_adamw_step_guarded(ops, n_ema):
    from mm_diffusion import optim
    H = S.HYPER
    rates = [S.f32(r) for r in (0.99, 0.9999, 0.5, 0.9)][:n_ema]
    steps_at = optim.StepCtrl.steps_taken.offset // 4
    for gs, wd in ((1.0, S.f32(0.05)), (1e-9, 0.0), (1.0, 0.0), (1e-9, S.f32(0.05))):
        n = 1000
        st = S.adamw_state(n, gs, seed=n_ema)
        dev = {k: v.cuda() for k, v in st.items()}
        for k in range(n_ema):
            dev[f"ema{k}"] = st["p"].cuda()
        lo, ln, first = (torch.from_numpy(a).cuda() for a in optim.chunk_table([600, 400]))
        partial = torch.zeros(len(lo), 2, dtype=torch.float64, device="cuda")
        sumsq = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
        ctrl = optim.new_step_ctrl("cuda")
        gn64 = st["g"].double().norm()
        max_norm = S.f32(0.37 * float(gn64))                   # a clip coefficient below 1
        for step in S.ADAM_STEPS:
            if step == 100000:
                ctrl[steps_at] = step - 1
            host = {k: v.cpu() for k, v in dev.items()}
            ops.sumsq_chunks(dev["g"], dev["p"], lo, ln, partial)
            ops.step_control(partial, first, sumsq, max_norm, H["beta1"], H["beta2"], ctrl)
            c = optim.read_step_ctrl(ctrl)
            assert c["took_step"] == 1 and c["steps_taken"] == step
            # the control block against float64: bc one rounding of a double result; the clip coefficient through V
            for name, beta in (("bc1", H["beta1"]), ("bc2", H["beta2"])):
                bc = 1.0 - float(torch.tensor(beta, dtype=torch.float64) ** step)
                assert abs(c[name] - bc) <= 2 * U * abs(bc), (name, step, c[name], bc)
            clip = V(torch.tensor(max_norm, dtype=torch.float64)) / (V(gn64, n=1) + C32(1e-6))
            assert abs(c["clip_coef"] - float(clip.v)) <= float(clip.bound()) and c["clip_coef"] < 1.0, (c["clip_coef"], float(clip.v))
            emas = [host[f"ema{k}"] for k in range(n_ema)]
            want = S.adamw_V(host["p"], host["g"], host["m"], host["v"], emas, rates, wd=wd, bc1=c["bc1"], bc2=c["bc2"], clip=c["clip_coef"], **H)
            ops.adamw_step_guarded(dev["p"], dev["g"], dev["m"], dev["v"], [dev[f"ema{k}"] for k in range(n_ema)], rates, H["lr"], H["beta1"],
                                   H["beta2"], H["eps"], wd, ctrl)
            _adam_check("adamw_step_guarded", dev, want, f"guarded g{gs:g} wd{wd:g} ema{n_ema} step {step}")


# ----------------------------------------------------------------------------- weight pack / gradient unpack
def _descs(shapes, src, fwd, bwd, select=None):
    """the descriptor table as optim.WeightPacker builds it -> (device bytes, n, blocks)"""
    from mm_diffusion import optim
    offs, _ = S.pack_layout(shapes)
    idx = list(range(len(shapes))) if select is None else list(select)
    descs = (optim._PackDesc * len(idx))()
    blocks = 0
    for j, i in enumerate(idx):
        Cout, Cin, nt = shapes[i]
        descs[j] = optim._PackDesc(src.data_ptr() + offs[i] * 4, fwd.data_ptr() + offs[i] * fwd.element_size(),
                                   None if bwd is None else bwd.data_ptr() + offs[i] * bwd.element_size(), Cout, Cin, nt, blocks)
        nb = optim._pack_blocks(Cout, Cin, nt)
        assert nb == S.pack_blocks(Cout, Cin, nt)
        blocks += nb
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda(), len(idx), blocks


@pytest.mark.parametrize("shapes", [S.PACK_SHAPES, S.PACK_MANY], ids=["tiles", "300-weights"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pack_conv_weights(ops, dtype, shapes):
    from mm_diffusion import _hip as H
    offs, total = S.pack_layout(shapes)
    ws = S.pack_weights(shapes)
    src = torch.full((total,), NAN)
    for w, off in zip(ws, offs):
        src[off:off + w.numel()] = w.reshape(-1)
    src = src.cuda()
    fwd, bwd = nan(total, dtype=dtype), nan(total, dtype=dtype)
    d, n, blocks = _descs(shapes, src, fwd, bwd)
    H.call("mmd_pack_conv_weights", H.BF16 if dtype == BF16 else H.F32, d.data_ptr(), n, blocks, H.stream_handle())
    wf, wb = S.pack_expected(ws, shapes, dtype)
    assert S.same_bits(fwd, wf), "forward operand (the NaN gaps included)"
    assert S.same_bits(bwd, wb), "data-gradient operand (the NaN gaps included)"
    for w, (Cout, Cin, nt), off in zip(ws[:7], shapes, offs):
        assert torch.equal(fwd[off:off + w.numel()].view(Cout, nt * Cin).cpu(), ops.pack_conv_weight(w, dtype))


@pytest.mark.parametrize("shapes", [S.PACK_SHAPES, S.PACK_MANY], ids=["tiles", "300-weights"])
def test_unpack_conv_grads(ops, shapes):
    from mm_diffusion import _hip as H
    grad0, packed0 = S.unpack_inputs(shapes)
    grad, packed = grad0.cuda(), packed0.cuda()
    d, n, blocks = _descs(shapes, grad, packed, None)
    H.call("mmd_unpack_conv_grads", d.data_ptr(), n, blocks, H.stream_handle())
    wg, wp = S.unpack_expected(grad0, packed0, shapes)
    assert S.same_bits(grad, wg), ".grad == grad_old + permuted(packed), gaps untouched"
    assert S.same_bits(packed, wp), "packed buffer cleared, gaps untouched"
    offs, _ = S.pack_layout(shapes)
    assert all(not packed[o:o + c * i * t].any() for o, (c, i, t) in zip(offs, shapes))
    # a per-bucket table (block starts relative to the bucket): the same for its weights, the others left alone
    sel = [1, 3, 5]
    grad, packed = grad0.cuda(), packed0.cuda()
    d, n, blocks = _descs(shapes, grad, packed, None, sel)
    H.call("mmd_unpack_conv_grads", d.data_ptr(), n, blocks, H.stream_handle())
    wg, wp = S.unpack_expected(grad0, packed0, shapes, sel)
    assert S.same_bits(grad, wg) and S.same_bits(packed, wp)


def test_pack_blocks_refuses_more_than_27_taps(ops):
    from mm_diffusion import _hip as H, optim
    assert H.lib().mmd_pack_blocks(8, 8, 28) <= 0 and H.lib().mmd_pack_blocks(8, 8, 27) == 1
    with pytest.raises(H.MMDError, match="taps"):
        optim._pack_blocks(8, 8, 28)


# ----------------------------------------------------------------------------- solver helpers
def test_lincomb(ops):
    a, b, c = S.lincomb_inputs()
    ac, bc, cc_ = a.cuda(), b.cuda(), c.cuda()
    for name, ca, cb, cc in S.lincomb_cases():
        out = nan(a.numel())
        ops.lincomb(ac, ca, bc if cb is not None else None, cb or 0.0, cc_ if cc is not None else None, cc or 0.0, out=out)
        ref, bound, _ = S.lincomb_ref(a, ca, b if cb is not None else None, cb, c if cc is not None else None, cc)
        check("lincomb", out, ref, bound, f"lincomb {name}")
    # an absent term is not added: -0 stays -0 (-0 + 0 * c would be +0)
    out = nan(8)
    ops.lincomb(torch.full((8,), -0.0, device="cuda"), 1.0, out=out)
    assert torch.signbit(out).all() and not out.any()


def test_lincomb_t(ops):
    for name, per, tk, has in S.lincomb_t_cases():
        a, b, tabs, t = S.lincomb_t_inputs(per, tk)
        tc = [tab.cuda() if h else None for tab, h in zip(tabs, has[:3])]
        out = nan(*a.shape)
        ops.lincomb_t(a.cuda(), b.cuda() if has[3] else None, out, tc[0], tc[1], tc[2], t.cuda())
        ref, bound, _ = S.lincomb_t_ref(a, b, tabs, t, has)
        check("lincomb_t", out, ref, bound, f"lincomb_t {name}")


def test_clamp_scale(ops):
    for name, per, mv in S.clamp_cases():
        x, s = S.clamp_inputs(per)
        xc = x.cuda()
        ops.clamp_scale_(xc, s.cuda(), mv)
        ref, bound, _ = S.clamp_ref(x, s, mv)
        check("clamp_scale", xc, ref, bound, f"clamp_scale {name}")


def test_dpm_err(ops):
    for per in S.DPM_PERS:
        hi, lo, prev = S.dpm_err_inputs(per)
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        ops.dpm_err(hi.cuda(), lo.cuda(), prev.cuda(), S.DPM_ATOL, S.DPM_RTOL, out)
        ref, bound = S.dpm_err_ref(hi, lo, prev)
        check("dpm_err", out, ref, bound, f"dpm_err {per}")
        one = out.clone()
        ops.dpm_err(hi.cuda(), lo.cuda(), prev.cuda(), S.DPM_ATOL, S.DPM_RTOL, out)          # the call accumulates
        assert torch.equal(out, one + one)


def test_dpm_err_order(ops):
    """The order of mmd_dpm_err's sum, documented on an input on which the orders differ in float64 (errbound_small.dpm_order_inputs):
    one block per sample, thread t sums its elements t, t + 256, .. in ascending order, then s[t] += s[t + o] for o = 128 .. 1.
    Small terms that meet the 2^53 of thread 0 one by one are rounded away (2^53); small terms that meet each other first survive
    (2^53 + 2).  This pins the order after the per-block float64 atomics were replaced by one block per sample; it is NOT claimed to
    fail on the library before that change in every run (there the order of the block partials was the hardware's)."""
    for small_at, want in (((128, 64), 2.0 ** 53), ((64, 192), 2.0 ** 53 + 2)):
        hi, lo, prev = S.dpm_order_inputs(small_at)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        ops.dpm_err(hi.cuda(), lo.cuda(), prev.cuda(), 1.0, 0.0, out)
        assert float(out[0]) == want, (small_at, float(out[0]) - 2.0 ** 53)
