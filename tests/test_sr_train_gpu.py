"""Backward kernels at the shapes of the image super-resolution U-Net (head width 192, GroupNorm over up to 1536 channels, 6 channels per
group) against torch CPU autograd in fp64 on the same (bf16-rounded) inputs.

Bounds: those of test_bwd_gpu.py for the same quantities - rel-L2 <= 5e-5 for the fp32 kernels (fp32 accumulation / atomics order),
<= 2e-2 for bf16 (bf16 activations and gradient tensors, fp32 accumulation) - for each of dq / dk / dv and dx / dgamma / dbeta / dfilm.
Every case here fails on the parent commit: head widths above 128 and GroupNorms above 1024 channels were argument errors there, and
head width 192 in bf16 fell to the fp32-in-LDS pair that stopped at 128.
"""
import pytest
import torch
import torch.nn.functional as F_

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def tol(dt):
    return 5e-5 if dt == torch.float32 else 2e-2


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    from mm_diffusion import ops, train_ops
    return ops, train_ops


def rnd(*shape, dt=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).float()


def leaf(x, dt):
    return x.to(dt).cuda().requires_grad_(True)


def attend64(q, k, v, heads):
    """[Tq, C], [Tk, C], [Tk, C] fp64 -> [Tq, C]: softmax(q k^T / sqrt(ch)) v per head."""
    Tq, C = q.shape
    ch = C // heads
    qh, kh, vh = (t.reshape(t.shape[0], heads, ch).permute(1, 0, 2) for t in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(1, 2) / ch ** 0.5, dim=-1)
    return (w @ vh).permute(1, 0, 2).reshape(Tq, C)


def check_parts(tag, got, ref, C, bound):
    """rel-L2 of the dq / dk / dv column ranges of a [rows, 3C] gradient, each against the bound; the figures are printed first."""
    errs = {name: rel_l2(got[:, i * C:(i + 1) * C], ref[:, i * C:(i + 1) * C].float()) for i, name in enumerate(("dq", "dk", "dv"))}
    print(tag, {k: "%.3g" % v for k, v in errs.items()}, "bound %g" % bound)
    for name, e in errs.items():
        assert e < bound, (tag, name, e)


# (T, heads, ch, paths): 192 = the SR model's 768 channels / 4 heads at its 8 x 8 and 16 x 16 token counts plus a ragged count; bf16 runs the
# MFMA pair, fp32 the VALU pair.  144 (96-channel base width x 3, 2 heads ... ) and 160 are off the MFMA list: VALU pair in both dtypes.
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T_,heads,ch", [(64, 4, 192), (256, 4, 192), (293, 2, 192), (100, 2, 144), (77, 2, 160)])
def test_self_attention_backward_wide_heads(T, dt, T_, heads, ch):
    ops, tr = T
    C, N = heads * ch, 2
    rows = N * T_
    qkv = rnd(rows, 3 * C, dt=dt, seed=21)
    gy = rnd(rows, C, dt=dt, seed=22)
    qc = qkv.double().requires_grad_(True)
    loss = 0
    for n in range(N):
        idx = torch.arange(n * T_, (n + 1) * T_)
        loss = loss + (attend64(qc[idx, :C], qc[idx, C:2 * C], qc[idx, 2 * C:], heads) * gy[idx].double()).sum()
    loss.backward()
    qd = leaf(qkv, dt)
    assert ops.attn_mfma_ok(qd, ch) == (dt == torch.bfloat16 and ch == 192)      # the path this case is meant to take
    od = tr.SelfAttnFn.apply(qd, heads, "spatial", N, 1, T_)
    od.backward(gy.to(dt).cuda())
    torch.cuda.synchronize()
    check_parts("self T=%d heads=%d ch=%d %s" % (T_, heads, ch, dt), qd.grad.float().cpu(), qc.grad, C, tol(dt))


# several query groups and a window that wraps round the key rows, at head width 192: the G > 1 walk of the split dK / dV kernel (bf16)
# and of the 32-row VALU kernels (fp32); L = 403 is not a multiple of F, so the last group is the long one
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("F,HW,L,win,shift,heads,ch", [(4, 64, 403, 3, 2, 1, 192), (4, 40, 160, 2, 3, 2, 192)])
def test_cross_attention_backward_head_width_192(T, dt, F, HW, L, win, shift, heads, ch):
    ops, tr = T
    N, C = 2, heads * ch
    apf = L // F
    vq, aq = rnd(N * F * HW, 3 * C, dt=dt, seed=23), rnd(N * L, 3 * C, dt=dt, seed=24)
    gv, ga = rnd(N * F * HW, C, dt=dt, seed=25), rnd(N * L, C, dt=dt, seed=26)
    vc, ac = vq.double().requires_grad_(True), aq.double().requires_grad_(True)
    loss = 0
    for n in range(N):
        for i in range(F):
            a_idx = n * L + (torch.arange(win * apf) + (i + shift) * apf) % L
            qi = n * F * HW + torch.arange(i * HW, (i + 1) * HW)
            loss = loss + (attend64(vc[qi, :C], ac[a_idx, C:2 * C], ac[a_idx, 2 * C:], heads) * gv[qi].double()).sum()
            v_idx = n * F * HW + (torch.arange(win * HW) + (i + shift) * HW) % (F * HW)
            hi = L if i == F - 1 else (i + 1) * apf
            qa = n * L + torch.arange(i * apf, hi)
            loss = loss + (attend64(ac[qa, :C], vc[v_idx, C:2 * C], vc[v_idx, 2 * C:], heads) * ga[qa].double()).sum()
    loss.backward()
    vd, ad = leaf(vq, dt), leaf(aq, dt)
    vo, ao = tr.CrossAttnFn.apply(vd, ad, heads, N, F, HW, L, win, shift)
    torch.autograd.backward([vo, ao], [gv.to(dt).cuda(), ga.to(dt).cuda()])
    torch.cuda.synchronize()
    check_parts("cross video %s" % dt, vd.grad.float().cpu(), vc.grad, C, tol(dt))
    check_parts("cross audio %s" % dt, ad.grad.float().cpu(), ac.grad, C, tol(dt))


# the SR decoder's concatenated inputs (1536 = 768 + 768, 1152 = 768 + 384) and its 192-channel level (6 channels per group against
# 8-element bf16 vectors).  fp32 rows of 1152 / 1536 channels are 288 / 384 16-byte vectors: the column-chunked launches.
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("C,HW", [(1152, 64), (1536, 64), (192, 100), (2048, 16)])
def test_groupnorm_backward_wide(T, dt, film, C, HW):
    ops, tr = T
    N = 2
    x = (rnd(N, C, HW, dt=dt, seed=31) * 1.5 + 0.3).to(dt).float()
    g, b = 1 + 0.1 * rnd(C, seed=32), rnd(C, seed=33)
    gy = rnd(N * HW, C, dt=dt, seed=34)
    fl = rnd(N, 2 * C, seed=35, scale=0.3) if film else None
    xc, gc, bc = (t.double().requires_grad_(True) for t in (x, g, b))
    fc = None if fl is None else fl.double().requires_grad_(True)
    y = F_.group_norm(xc, 32, gc, bc, 1e-5)
    if fc is not None:
        y = y * (1 + fc[:, :C, None]) + fc[:, C:, None]
    y = F_.silu(y)
    to_rows = lambda t: t.permute(0, 2, 1).reshape(N * HW, C)
    to_rows(y).backward(gy.double())
    xd, gd, bd = leaf(to_rows(x), dt), leaf(g, torch.float32), leaf(b, torch.float32)
    fd = None if fl is None else leaf(fl, torch.float32)
    yd = tr.group_norm(xd, gd, bd, ops.Geom.per_sample(N, HW), True, film=fd)
    e_fwd = rel_l2(yd.detach().float().cpu(), to_rows(y.detach()).float())
    yd.backward(gy.to(dt).cuda())
    torch.cuda.synchronize()
    errs = {"dx": rel_l2(xd.grad.float().cpu(), to_rows(xc.grad).float()), "dgamma": rel_l2(gd.grad.cpu(), gc.grad.float()),
            "dbeta": rel_l2(bd.grad.cpu(), bc.grad.float())}
    if film:
        errs["dfilm"] = rel_l2(fd.grad.cpu(), fc.grad.float())
    print("gn C=%d film=%s %s fwd %.3g" % (C, film, dt, e_fwd), {k: "%.3g" % v for k, v in errs.items()}, "bound %g" % tol(dt))
    assert e_fwd < (2e-5 if dt == torch.float32 else 1e-2)
    for name, e in errs.items():
        assert e < tol(dt), (C, film, dt, name, e)


# ============================================================================= model level: the SR U-Net's training step against the reference
# tests/golden/sr_*_train_grads.npz (tools/gen_golden.py: gen_sr_train): the reference's diffusion.training_losses(...).backward() on the CPU
# with synth weights - loss terms, the L2 norm of every parameter's gradient and every stride-th gradient element.  The two measures and
# the bounds of test_configs_gpu.py::test_config3_full_size_gradients_match_the_reference_fixture (GRAD_FP32 / GRAD_BF16 there; the base
# model measured 4.2e-6 / 8.0e-3).  Measured here on MI355X (subsample rel-L2, worst per-tensor norm error):
#   sr_tiny         fp32 2.5e-6, 2.6e-6     bf16 1.01e-2, 1.23e-2 (input_blocks.3.1.norm.bias)
#   sr_tiny_nofilm  fp32 1.4e-6, 1.5e-6     bf16 9.5e-3, 8.2e-3
#   sr_w192         fp32 1.9e-6, 5.8e-7     bf16 7.5e-3, 3.7e-3
#   sr_full         fp32 2.3e-6, 9.7e-7     bf16 1.07e-2, 9.0e-3 (input_blocks.10.0.out_layers.0.weight, norm 6.0e-3 of a largest 3.55)
GRAD_FP32 = 1e-4
GRAD_BF16 = 3e-2
NORM_FLOOR = 1e-4      # of the largest per-tensor norm OF THE FIXTURE; at least 90 % of the tensors must clear it (the reference alone: 97.8 % tiny,
#                        94.9 % tiny non-FiLM, 100 % w192 and full; the base model's 1e-3 would leave only 71 % of the full SR model's tensors)

SR_TINY = dict(large_size=64, small_size=16, sr_num_channels=32, sr_num_res_blocks=1, sr_attention_resolutions="2,4", sr_num_heads=2,
               sr_resblock_updown=True)
SR_CONFIGS = {       # the flag sets of tools/gen_golden.py: SR_TRAIN
    "sr_tiny": dict(),
    "sr_w192": dict(sr_num_channels=192, sr_attention_resolutions="8", sr_num_heads=4),
    "sr_full": dict(large_size=256, small_size=64, sr_num_channels=192, sr_num_res_blocks=2, sr_attention_resolutions="8,16,32", sr_num_heads=4,
                    sr_use_scale_shift_norm=True),
    "sr_tiny_nofilm": dict(sr_use_scale_shift_norm=False, sr_learn_sigma=False),
}


def sr_build(name, dt, **over):
    from mm_diffusion import logger, script_util as su
    from mm_diffusion.synth import synth_tensor
    logger.set_quiet(True)
    d = su.image_sr_model_and_diffusion_defaults()
    d.update(SR_TINY)
    d.update(SR_CONFIGS[name])
    d.update(use_fp16=(dt == torch.bfloat16), **over)
    model, diff = su.image_sr_create_model_and_diffusion(**d)
    model.load_state_dict({k: synth_tensor(k, v.shape) for k, v in model.state_dict().items()})
    model.cuda().train()
    return d, model, diff


def sr_inputs(g, d):
    """The fixture's draws: x0, low (uniform [-1, 1]), noise (normal), in that order from one seeded generator."""
    gen = torch.Generator().manual_seed(int(g["seed"]))
    B, L, S = int(g["B"]), d["large_size"], d["small_size"]
    x0 = torch.rand(B, 3, L, L, generator=gen) * 2 - 1
    low = torch.rand(B, 3, S, S, generator=gen) * 2 - 1
    noise = torch.randn(B, 3, L, L, generator=gen)
    return x0.cuda(), low.cuda(), noise.cuda(), torch.from_numpy(g["t"]).cuda()


def sr_step(name, dt):
    import numpy as np
    from helpers import gold
    g = gold(f"{name}_train_grads")
    d, model, diff = sr_build(name, dt)
    x0, low, noise, t = sr_inputs(g, d)
    terms = diff.training_losses(model, x0, t, model_kwargs={"low_res": low}, noise=noise)
    assert terms["loss"].grad_fn is not None
    got_terms = {k: v.detach().float().cpu().numpy() for k, v in terms.items()}
    terms["loss"].mean().backward()
    torch.cuda.synchronize()
    return g, model, got_terms, np


@pytest.mark.parametrize("name", ["sr_tiny", "sr_tiny_nofilm", "sr_w192", "sr_full"])
def test_sr_training_gradients_match_the_reference_fixture(name):
    """fp32 mode, then bf16, on the same fixture: loss terms (rtol 5e-4 / 3e-2) and the gradient of EVERY parameter - subsample rel-L2 over
    all tensors and the worst per-tensor norm ratio over the tensors above NORM_FLOOR of the fixture's largest norm."""
    for dt in (torch.float32, torch.bfloat16):
        g, model, terms, np = sr_step(name, dt)
        tol_loss, tol = (5e-4, GRAD_FP32) if dt == torch.float32 else (3e-2, GRAD_BF16)
        keys = [k for k in ("loss", "mse", "vb") if k in g.files]
        assert sorted(terms) == sorted(keys)
        for k in keys:
            print(f"{name} {dt} {k}: {terms[k]} reference {g[k]}")
        stride, names = int(g["stride"]), [str(n) for n in g["names"]]
        params = dict(model.named_parameters())
        assert names == list(params)
        assert all(params[k].grad is not None for k in names), [k for k in names if params[k].grad is None][:5]
        sub = torch.cat([params[k].grad.detach().float().flatten()[::stride] for k in names]).cpu()
        norms = np.asarray([float(params[k].grad.detach().double().norm()) for k in names])
        e_sub = rel_l2(sub, g["sub"])
        big = g["norms"] > NORM_FLOOR * g["norms"].max()
        ratio = np.abs(norms / np.maximum(g["norms"], 1e-30) - 1)
        e_norm = float(ratio[big].max())
        wi = int(np.argmax(np.where(big, ratio, 0)))
        print(f"{name} gradients vs the reference ({dt}): subsample rel-L2 {e_sub:.3e} over {sub.numel()} elements, worst per-tensor norm error "
              f"{e_norm:.3e} ({names[wi]}, norm {g['norms'][wi]:.3e} of max {g['norms'].max():.3e}; {int(big.sum())} of {len(names)} tensors "
              f"above {NORM_FLOOR:g} of the largest norm)")
        assert big.mean() >= 0.9, f"only {100 * big.mean():.1f} % of the tensors clear the norm floor"
        for k in keys:
            np.testing.assert_allclose(terms[k], g[k], rtol=tol_loss)
        assert torch.isfinite(sub).all() and e_sub < tol and e_norm < tol
        del model
        torch.cuda.empty_cache()


def test_sr_qkv_gradients_stay_in_the_reference_channel_order():
    """The legacy qkv order [head][q|k|v][ch] is re-ordered for the kernels inside the differentiable walk; .grad of *.qkv.weight / .bias must
    come back in the REFERENCE's order, un-permuted.  A wrong permutation is the likeliest silent error, hence its own assertion."""
    g, model, _, np = sr_step("sr_tiny", torch.float32)
    stride, names = int(g["stride"]), [str(n) for n in g["names"]]
    off = g["sub_off"]
    params = dict(model.named_parameters())
    seen = 0
    for i, k in enumerate(names):
        if k.startswith("input_blocks.") and (k.endswith(".1.qkv.weight") or k.endswith(".1.qkv.bias")):
            got = params[k].grad.detach().float().flatten()[::stride].cpu()
            ref = torch.from_numpy(g["sub"][off[i]:off[i + 1]])
            e = rel_l2(got, ref)
            print(f"{k}: rel-L2 {e:.3e} over {ref.numel()} elements")
            assert e < 1e-3, f"{k}: gradient does not match the reference in the reference's qkv channel order (rel-L2 {e:.3g})"
            seen += 1
    assert seen >= 2


def _inference_walk(model, x, t, low):
    from mm_diffusion import ops
    N, C, Hh, Ww = x.shape
    rows = ops.alloc(N * Hh * Ww, (2 * C + 7) // 8 * 8, dtype=model.dtype, device=x.device)
    ops.bilinear_concat_rows(x.float().contiguous(), low.float().contiguous(), rows)
    with torch.no_grad():
        return model._run(None, t, rows=rows, shape=(N, 2 * C, Hh, Ww))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_sr_forward_routing(dt):
    from helpers import gold
    g = gold("sr_tiny_forward")
    _, model, _ = sr_build("sr_tiny", dt)
    x, t, low = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["low"]).cuda()
    assert model.training and all(p.requires_grad for p in model.parameters())
    ref = _inference_walk(model, x, t, low)
    with torch.no_grad():                               # no_grad: the inference walk, bitwise, no autograd node
        y = model(x, t, low_res=low)
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, ref)
    y = model(x, t, low_res=low)                        # grad enabled, trainable parameters: the differentiable walk
    e = rel_l2(y.detach().cpu(), ref.cpu())
    print(f"differentiable walk vs inference walk ({dt}): rel-L2 {e:.3e}")
    assert y.grad_fn is not None and e < (1e-4 if dt == torch.float32 else 3e-2)
    e_ref = rel_l2(y.detach().cpu(), g["y"])
    assert e_ref < (1e-4 if dt == torch.float32 else 3e-2)
    with pytest.raises(NotImplementedError):            # gradients with respect to the images are not built
        model(x.clone().requires_grad_(True), t, low_res=low)
    for p in model.parameters():
        p.requires_grad_(False)
    y = model(x, t, low_res=low)                        # grad enabled, nothing requires grad: the inference walk
    assert y.grad_fn is None and torch.equal(y, ref)
    y = model(x.clone().requires_grad_(True), t, low_res=low)      # frozen parameters, an input that requires grad: still the inference walk
    assert y.grad_fn is None and torch.equal(y, ref)


def test_plain_image_unet_differentiable_walk_matches_the_sr_model():
    """ImageUnet.forward (no low_res: the input rows are built by image_train_forward.input_rows) on cat(x, bilinear(low_res)) is the SR
    model by construction (reference image_unet.py:704-715), so with the same weights its output and EVERY parameter gradient must agree
    with ImageSuperResModel's differentiable walk.  fp32 mode; bound 1e-4 as the forward tests (the two differ only in where the bilinear
    upsample is computed: torch vs mmd_bilinear_concat_rows, fp32 rounding)."""
    import torch.nn.functional as F_
    from helpers import gold
    from mm_diffusion.image_unet import ImageUnet
    g = gold("sr_tiny_forward")
    _, sr_model, _ = sr_build("sr_tiny", torch.float32)
    x, t, low = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["low"]).cuda()
    plain = ImageUnet(image_size=64, in_channels=6, model_channels=32, out_channels=6, num_res_blocks=1, attention_resolutions=(2, 4),
                      channel_mult=(1, 2, 3, 4), num_heads=2, use_scale_shift_norm=True, resblock_updown=True)
    plain.load_state_dict(sr_model.state_dict())
    plain.cuda().train()
    gy = torch.randn(2, 6, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    ys = sr_model(x, t, low_res=low)
    ys.backward(gy)
    yp = plain(torch.cat([x, F_.interpolate(low, (64, 64), mode="bilinear")], dim=1), t)
    assert yp.grad_fn is not None
    yp.backward(gy)
    torch.cuda.synchronize()
    e = rel_l2(yp.detach().cpu(), ys.detach().cpu())
    ps, pp = dict(sr_model.named_parameters()), dict(plain.named_parameters())
    assert list(ps) == list(pp) and all(v.grad is not None for v in pp.values())
    eg = rel_l2(torch.cat([v.grad.flatten() for v in pp.values()]).cpu(), torch.cat([v.grad.flatten() for v in ps.values()]).cpu())
    print(f"plain ImageUnet vs SR model: output rel-L2 {e:.3e}, all gradients rel-L2 {eg:.3e}")
    assert e < 1e-4 and eg < 1e-4


# ============================================================================= TrainLoop
def _seed():
    import random

    import numpy as np
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)


def _mk_loop(tmp, dt=torch.float32, respacing="", **kw):
    from mm_diffusion import logger
    from mm_diffusion.real_image_datasets import load_data
    from mm_diffusion.train_util import TrainLoop
    d, model, diff = sr_build("sr_tiny", dt, sr_timestep_respacing=respacing)
    logger.configure(dir=str(tmp))

    def data():
        for lr_, hr, sr, cond in load_data(data_dir="synthetic", batch_size=4, image_size=d["large_size"]):
            cond["low_res"] = lr_
            yield lr_, hr, sr, cond
    args = dict(model=model, diffusion=diff, data=data(), batch_size=4, microbatch=2, ema_rate="0.9,0.99", log_interval=1, save_interval=3,
                resume_checkpoint="", lr=1e-4, weight_decay=0.01, lr_anneal_steps=0, use_fp16=(dt == torch.bfloat16), sample_fn="ddim")
    args.update(kw)
    return d, model, diff, TrainLoop(**args)


def test_sr_trainloop_checkpoints_resume_and_sample(tmp_path):
    import os
    _seed()
    d, model, diff, loop = _mk_loop(tmp_path / "a", respacing="ddim4", lr_anneal_steps=4)      # steps 1, 2, 3 -> save (and sample dump) at 3
    w0 = loop.opt.flat.clone()
    loop.run_loop()
    assert loop.step == 4 and not torch.equal(w0, loop.opt.flat)
    names = set(os.listdir(tmp_path / "a"))
    assert {"model000003.pt", "ema_0.9_000003.pt", "ema_0.99_000003.pt", "opt000003.pt"} <= names, names
    try:
        import PIL  # noqa: F401
        assert "ddim_samples_steps3.png" in names             # the sample dump at the save (skipped with a log line without PIL)
    except ImportError:
        pass
    sd = torch.load(tmp_path / "a" / "model000003.pt")
    assert list(sd.keys()) == list(model.state_dict().keys())
    ema = torch.load(tmp_path / "a" / "ema_0.9_000003.pt")
    assert list(ema.keys()) == list(sd.keys()) and any(not torch.equal(sd[k].cpu(), ema[k].cpu()) for k in sd)
    osd = torch.load(tmp_path / "a" / "opt000003.pt")
    assert set(osd.keys()) == {"state", "param_groups"} and len(osd["state"]) == len(list(model.parameters()))
    torch.optim.AdamW([torch.nn.Parameter(torch.zeros_like(p)) for p in model.parameters()]).load_state_dict(osd)

    _seed()
    _, model2, _, loop2 = _mk_loop(tmp_path / "a", respacing="ddim4", lr_anneal_steps=6)         # resumes at 3: bit-for-bit
    assert loop2.resume_step == 3 and loop2.opt.steps == 3
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    off = 0
    for i, p in enumerate(loop2.opt.params):
        assert torch.equal(loop2.opt.m[off:off + p.numel()].view_as(p).cpu(), osd["state"][i]["exp_avg"].cpu())
        assert torch.equal(loop2.opt.v[off:off + p.numel()].view_as(p).cpu(), osd["state"][i]["exp_avg_sq"].cpu())
        off += p.numel()
    loop2.run_loop()
    assert "model000006.pt" in os.listdir(tmp_path / "a")

    # train -> sample round trip: the checkpoint loads into a fresh model and samples
    _, fresh, sdiff = sr_build("sr_tiny", torch.float32, sr_timestep_respacing="ddim4")
    fresh.load_state_dict(torch.load(tmp_path / "a" / "model000006.pt"))
    fresh.eval()
    low = torch.rand(2, 3, 16, 16).cuda() * 2 - 1
    out = sdiff.ddim_sample_loop(fresh, (2, 3, 64, 64), clip_denoised=True, model_kwargs={"low_res": low}, device=torch.device("cuda"))
    assert out.shape == (2, 3, 64, 64) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0


def test_sr_trainloop_loss_goes_down_bf16(tmp_path):
    """Ten AdamW steps on one repeated batch with the same timesteps lower the training loss (bf16 activations, fp32 masters)."""
    import random

    import numpy as np
    _seed()
    _, model, _, loop = _mk_loop(tmp_path / "b", dt=torch.bfloat16, lr=2e-4, ema_rate="0.999")
    low, hr, _, cond = next(loop.data)
    losses = []
    for _ in range(10):
        np.random.seed(1)
        random.seed(1)
        torch.manual_seed(1)
        out = loop.run_step(hr, cond)
        losses.append(float(out["loss"].detach().mean()))
        loop.step += 1
    print("sr losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0]


def test_sr_no_grad_forward_follows_the_training_weights(tmp_path):
    """The inference walk packs its GEMM operands once; training rewrites the parameters in place (FlatAdamW's kernel on the flat buffer,
    the EMA swap of the sample dump).  A no_grad evaluation between training steps must see the CURRENT weights: after an optimizer step
    it equals a fresh model loaded from the checkpoint of that step, and after a sample dump (EMA in, masters back) it still does."""
    from helpers import gold
    g = gold("sr_tiny_forward")
    x, t, low = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["low"]).cuda()
    _seed()
    d, model, diff, loop = _mk_loop(tmp_path / "w", lr=1e-3, ema_rate="0.5", sample_fn="dpm_solver")
    with torch.no_grad():
        y0 = model(x, t, low_res=low)                   # packs the initial weights
    lr_, hr, sr, cond = next(loop.data)
    loop._last = (lr_, hr, sr)
    loop.run_step(hr, cond)
    loop.save()
    with torch.no_grad():
        y1 = model(x, t, low_res=low)
    _, fresh, _ = sr_build("sr_tiny", torch.float32)
    fresh.load_state_dict(torch.load(tmp_path / "w" / "model000001.pt"))
    with torch.no_grad():
        yf = fresh(x, t, low_res=low)
    e_new, e_old = rel_l2(y1.cpu(), yf.cpu()), rel_l2(y0.cpu(), yf.cpu())
    print(f"no_grad forward after one AdamW step vs a fresh model with the saved weights: rel-L2 {e_new:.3e}; the stale output is {e_old:.3e} away")
    assert e_new < 1e-6 and e_old > 1e-4
    masters = loop.opt.flat.clone()
    assert not torch.equal(masters, loop.opt.ema_params[0])
    loop.save_sr()                                      # 50-evaluation DPM-Solver dump from the EMA copy; the masters come back
    assert torch.equal(loop.opt.flat, masters)
    with torch.no_grad():
        y2 = model(x, t, low_res=low)
    e_after = rel_l2(y2.cpu(), yf.cpu())
    print(f"no_grad forward after the sample dump: rel-L2 {e_after:.3e}")
    assert e_after < 1e-6


def test_sr_trainloop_resumed_trajectory_matches_an_uninterrupted_one(tmp_path):
    """Five steps in one process against three steps, a checkpoint, and two more steps in a fresh loop that resumes from it, with the same
    batches and the same timestep draws per step.  The two are not bitwise (the weight gradients accumulate with fp32 atomics, whose order
    moves the last bits), so the measure is the distance of the final parameters relative to what steps 4 and 5 moved them: rounding noise
    in the gradients changes an AdamW update by parts in 1e6, a resume that lost the moments or the step count changes it by order one.
    Bound 1e-2."""
    import random

    import numpy as np

    def steps(loop, batches, ks):
        for k in ks:
            np.random.seed(100 + k)
            random.seed(100 + k)
            torch.manual_seed(100 + k)
            lr_, hr, sr, cond = batches[k]
            loop.run_step(hr, cond)
            loop.step += 1
    _seed()
    _, _, _, loop_u = _mk_loop(tmp_path / "u", lr=1e-3)
    batches = [next(loop_u.data) for _ in range(5)]
    steps(loop_u, batches, range(3))
    p3 = loop_u.opt.flat.clone()
    steps(loop_u, batches, range(3, 5))
    _seed()
    _, _, _, loop_a = _mk_loop(tmp_path / "r", lr=1e-3)
    steps(loop_a, batches, range(3))
    loop_a.step -= 1                                    # save() names the checkpoint after the step just taken
    loop_a.save()
    _seed()
    _, _, _, loop_b = _mk_loop(tmp_path / "r", lr=1e-3)
    assert loop_b.resume_step == 3 and loop_b.opt.steps == 3
    steps(loop_b, batches, range(3, 5))
    moved = float((loop_u.opt.flat - p3).norm())
    e = float((loop_b.opt.flat - loop_u.opt.flat).norm()) / moved
    e_ema = float((loop_b.opt.ema_params[0] - loop_u.opt.ema_params[0]).norm()) / float(loop_u.opt.ema_params[0].norm())
    print(f"resumed vs uninterrupted after 5 steps: parameter distance {e:.3e} of the movement of steps 4-5, EMA rel-L2 {e_ema:.3e}")
    assert moved > 0 and e < 1e-2 and e_ema < 1e-4
