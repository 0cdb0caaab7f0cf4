"""The training step guard on the GPU: mmd_sumsq_chunks + mmd_step_control + mmd_adamw_step_guarded through ops / optim.FlatAdamW,
and what both TrainLoop classes do with them (norm logging, non-finite skip, clipping, step count).

Bounds (derived, not measured):
  * per-parameter sums of squares against torch fp64: relative 1e-10.  Every fp32 square is exact in double and at most 2^17 of
    them are added sequentially in double: n * 2^-52 ~ 3e-11.
  * ctrl.grad_norm / param_norm against the fp64 norm: relative 2.4e-7 = 2 fp32 ulp (a sum exact to double, one sqrt, one rounding).
  * the guarded AdamW against torch.optim.AdamW in fp64: rel-L2 <= 2 * e_old + 1e-7, e_old = the same measure of the UNCHANGED
    mmd_adamw_step (+ torch's in-place update for the EMA copies after the first) on the same inputs; the only licensed difference
    is the rounding of the bias corrections, computed on the device.
Every test prints its figures before it asserts (run with -s).
"""
import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

ULP2 = 2.4e-7


def _sizes():
    from mm_diffusion.optim import STEP_CHUNK as L
    return [1, 3, 255, 256, 257, 4093, L, L + 1, 70001]


class Raw:
    """Flat buffers + chunk table + workspaces of the three launches, without FlatAdamW."""

    def __init__(self, sizes, seed=0, n_ema=0, max_grad_norm=0.0, gscale=1.0):
        from mm_diffusion import optim
        self.sizes, self.n = sizes, sum(sizes)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        gen = torch.Generator().manual_seed(seed)
        self.g = (torch.randn(self.n, generator=gen) * gscale).cuda()
        self.p = torch.randn(self.n, generator=gen).cuda()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.rates = [0.9, 0.99, 0.999][:n_ema]
        self.emas = [self.p.clone() for _ in self.rates]
        lo, ln, first = optim.chunk_table(sizes)
        self.lo, self.ln, self.first = (torch.from_numpy(a).cuda() for a in (lo, ln, first))
        self.partial = torch.zeros(len(lo), 2, dtype=torch.float64, device="cuda")
        self.sumsq = torch.zeros(len(sizes), 2, dtype=torch.float64, device="cuda")
        self.ctrl = optim.new_step_ctrl("cuda")
        self.max_grad_norm = max_grad_norm
        self.hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05)

    def norms(self):
        from mm_diffusion import ops, optim
        ops.sumsq_chunks(self.g, self.p, self.lo, self.ln, self.partial)
        ops.step_control(self.partial, self.first, self.sumsq, self.max_grad_norm, self.hyper["beta1"], self.hyper["beta2"], self.ctrl)
        return optim.read_step_ctrl(self.ctrl)

    def step(self):
        from mm_diffusion import ops
        c = self.norms()
        ops.adamw_step_guarded(self.p, self.g, self.m, self.v, self.emas, self.rates, ctrl=self.ctrl, **self.hyper)
        return c

    def state(self):
        return [t.clone() for t in (self.p, self.m, self.v, *self.emas)]

    def ref_sumsq(self):
        g, p = self.g.double().cpu(), self.p.double().cpu()
        return torch.stack([torch.stack([(t[a:b] ** 2).sum() for t in (g, p)]) for a, b in zip(self.off[:-1], self.off[1:])])


# ----------------------------------------------------------------------------- 1, 2: norms
@pytest.mark.parametrize("sizes", ["P9", [1]])
def test_norms_match_fp64(sizes):
    r = Raw(_sizes() if sizes == "P9" else sizes, seed=1)
    assert r.n % 4 != 0 or len(r.sizes) == 1
    c = r.norms()
    ref = r.ref_sumsq()
    got = r.sumsq.cpu()
    err = float(((got - ref).abs() / ref).max())
    gn, pn = float(ref[:, 0].sum().sqrt()), float(ref[:, 1].sum().sqrt())
    eg, ep = abs(c["grad_norm"] / gn - 1), abs(c["param_norm"] / pn - 1)
    print(f"sizes {r.sizes}: worst per-parameter sum-of-squares error {err:.3e} (bound 1e-10); grad_norm {eg:.3e}, param_norm {ep:.3e} (bound {ULP2})")
    assert err <= 1e-10
    assert eg <= ULP2 and ep <= ULP2
    assert c["took_step"] == 1 and c["steps_taken"] == 1 and c["skipped_total"] == 0 and c["first_bad_param"] == -1 and c["clip_coef"] == 1.0
    assert c["cum_count"] == 1
    assert abs(c["cum_grad_norm"] / gn - 1) <= 1e-10 and abs(c["cum_param_norm"] / pn - 1) <= 1e-10


def test_squares_beyond_fp32_range_are_not_a_false_positive():
    """g = 3e19 everywhere: every square (9e38) exceeds the fp32 maximum, the norm (~1e22) does not."""
    r = Raw(_sizes(), seed=2)
    r.g.fill_(3e19)
    c = r.norms()
    want = float(torch.tensor(3e19, dtype=torch.float32).double()) * r.n ** 0.5
    e = abs(c["grad_norm"] / want - 1)
    print(f"constant 3e19 over {r.n} elements: grad_norm {c['grad_norm']:.6e} vs {want:.6e}, error {e:.3e}")
    assert c["took_step"] == 1 and c["first_bad_param"] == -1 and np.isfinite(c["grad_norm"]) and e <= ULP2


# ----------------------------------------------------------------------------- 3: detection
def _poison_cases():
    from mm_diffusion.optim import STEP_CHUNK as L
    off = np.concatenate([[0], np.cumsum(_sizes())])
    return {"nan_first": ([(int(off[0]), float("nan"))], 0),
            "inf_last": ([(int(off[9]) - 1, float("inf"))], 8),
            "neginf_past_chunk": ([(int(off[7]) + L, float("-inf"))], 7),
            "two_params": ([(int(off[5]) + 17, float("nan")), (int(off[2]) + 254, float("inf"))], 2)}


@pytest.mark.parametrize("case", ["nan_first", "inf_last", "neginf_past_chunk", "two_params"])
def test_nonfinite_gradient_is_detected(case):
    poison, bad = _poison_cases()[case]
    r = Raw(_sizes(), seed=3)
    c0 = r.norms()                                      # one clean step first: steps_taken = 1
    assert c0["took_step"] == 1 and c0["steps_taken"] == 1
    for idx, val in poison:
        r.g[idx] = val
    c = r.norms()
    assert c["took_step"] == 0 and c["skipped_total"] == c0["skipped_total"] + 1 and c["steps_taken"] == c0["steps_taken"]
    assert c["first_bad_param"] == bad and c["last_bad_param"] == bad
    assert c["cum_count"] == c0["cum_count"] and c["cum_grad_norm"] == c0["cum_grad_norm"]
    assert (c["bc1"], c["bc2"]) == (c0["bc1"], c0["bc2"])


# ----------------------------------------------------------------------------- 4: the skip changes nothing
def test_skipped_step_is_bitwise_a_no_op_and_the_next_one_trains():
    r = Raw(_sizes(), seed=4, n_ema=3)
    r.step()                                            # moments and EMA copies away from their initial values
    before = r.state()
    clean = r.g.clone()
    r.g[int(r.off[4]) + 5] = float("nan")
    c = r.step()
    assert c["took_step"] == 0 and c["steps_taken"] == 1
    for a, b in zip(r.state(), before):
        assert torch.equal(a, b)
    r.g.copy_(clean)
    c2 = r.step()
    assert c2["took_step"] == 1 and c2["steps_taken"] == 2 and c2["skipped_total"] == 1 and c2["first_bad_param"] == -1
    assert c2["last_bad_param"] == 4
    for a, b in zip(r.state(), before):
        assert not torch.equal(a, b)
        assert torch.isfinite(a).all()


# ----------------------------------------------------------------------------- 5, 6: arithmetic, clipping
def _adamw_case(max_grad_norm, clip_ref, gscale=1.0):
    """Three steps on the inputs of test_bwd_gpu.py::test_adamw_matches_torch (n = 1000, lr 1e-2, weight decay 0.05, gradient g * step)
    plus three EMA rates.  Returns rel-L2 against fp64 of (guarded, old) per quantity, and the guarded Raw."""
    from mm_diffusion import ops

    def rnd(n, seed):
        return torch.randn(n, generator=torch.Generator().manual_seed(seed))
    p0, g = rnd(1000, 25), rnd(1000, 26) * gscale
    rates = [0.9, 0.99, 0.999]
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-2, weight_decay=0.05)
    ema_ref = [p0.double().clone() for _ in rates]
    r = Raw([1000], n_ema=3, max_grad_norm=max_grad_norm)
    r.p.copy_(p0)
    for e in r.emas:
        e.copy_(p0)
    po, mo, vo = p0.clone().cuda(), torch.zeros(1000).cuda(), torch.zeros(1000).cuda()
    eo = [p0.clone().cuda() for _ in rates]
    pre = []
    for step in (1, 2, 3):
        ref.grad = (g * step).double()
        if clip_ref:
            torch.nn.utils.clip_grad_norm_([ref], clip_ref)
        opt.step()
        for e, rate in zip(ema_ref, rates):
            e.mul_(rate).add_(ref.detach(), alpha=1 - rate)
        r.g.copy_(g * step)
        pre.append((r.step(), float((g * step).double().norm())))
        # the old path: FlatAdamW(guard=False).step() - the unchanged kernel with the first EMA copy, torch for the others (and, for
        # the clipped case, torch's fp32 clip_grad_norm_ in front of it)
        go = torch.nn.Parameter(torch.zeros(1000, device="cuda"))
        go.grad = (g * step).cuda()
        if clip_ref:
            torch.nn.utils.clip_grad_norm_([go], clip_ref)
        ops.adamw_step(po, go.grad, mo, vo, eo[0], 1e-2, 0.9, 0.999, 1e-8, 0.05, step, ema_rate=rates[0])
        for rate, e in zip(rates[1:], eo[1:]):
            e.mul_(rate).add_(po, alpha=1 - rate)
    errs = {"p": (rel_l2(r.p.cpu(), ref.detach()), rel_l2(po.cpu(), ref.detach()))}
    for rate, a, b, c in zip(rates, r.emas, eo, ema_ref):
        errs[f"ema_{rate}"] = (rel_l2(a.cpu(), c), rel_l2(b.cpu(), c))
    return errs, r, pre


def _check_against_old(tag, errs):
    for k, (e_new, e_old) in errs.items():
        print(f"{tag} {k}: guarded {e_new:.3e}  unchanged mmd_adamw_step {e_old:.3e}  bound {2 * e_old + 1e-7:.3e}")
    for k, (e_new, e_old) in errs.items():
        assert e_new <= 2 * e_old + 1e-7, (tag, k, e_new, e_old)


def test_guarded_arithmetic_matches_fp64_adamw():
    errs, r, pre = _adamw_case(0.0, None)
    _check_against_old("adamw", errs)
    from mm_diffusion import optim
    c = optim.read_step_ctrl(r.ctrl)
    assert c["steps_taken"] == 3 and c["clip_coef"] == 1.0
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))          # the betas as the kernel receives them
    assert abs(c["bc1"] / (1 - b1 ** 3) - 1) <= ULP2 and abs(c["bc2"] / (1 - b2 ** 3) - 1) <= ULP2


def test_clipping_matches_fp64_clip_grad_norm():
    errs, r, pre = _adamw_case(0.5, 0.5)                 # |g| ~ 31.6, 63, 95 against max_grad_norm 0.5
    _check_against_old("clip 0.5", errs)
    for c, want in pre:                                  # the logged norm is the norm BEFORE clipping
        assert want > 25 and abs(c["grad_norm"] / want - 1) <= ULP2
        assert abs(c["clip_coef"] / (0.5 / (want + 1e-6)) - 1) <= 2 * ULP2
    _, r_hi, pre_hi = _adamw_case(1e4, None)             # a bound above the norm: coefficient exactly 1, bitwise the unclipped step
    _, r_0, _ = _adamw_case(0.0, None)
    assert all(c["clip_coef"] == 1.0 for c, _ in pre_hi)
    for a, b in zip(r_hi.state(), r_0.state()):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 7: repeatability
def test_the_three_launches_are_bitwise_repeatable():
    outs = []
    for _ in range(2):
        r = Raw(_sizes(), seed=7, n_ema=2, max_grad_norm=1.0)
        r.step()
        r.step()
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().tobytes() for t in (r.partial, r.sumsq, r.ctrl, r.p, *r.emas)])
    assert outs[0] == outs[1]


# ----------------------------------------------------------------------------- 8 - 10: the loops
KEYS = ("grad_norm", "param_norm", "current_grad_norm", "current_param_norm", "skipped_steps")
STREAM_KEYS = ("grad_norm_v", "grad_norm_a")


def _seed():
    import random
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)


def _logged():
    from mm_diffusion import logger
    return dict(logger.get_current().name2val)


def _poison(loop, param_index):
    """all_reduce_grads first writes a nan into the first element of one parameter's gradient; returns the undo."""
    opt = loop.opt
    off = sum(p.numel() for p in opt.params[:param_index])
    orig = opt.all_reduce_grads

    def poisoned():
        opt.grad[off] = float("nan")
        orig()
    opt.all_reduce_grads = poisoned

    def undo():
        del opt.all_reduce_grads
    return undo


def _skip_and_recover(loop, step_fn, monkeypatch, stream_keys):
    """One clean step (keys and values), one poisoned step (bitwise skip, logged with the tensor's name), one clean step again."""
    from mm_diffusion import logger
    lines = []
    monkeypatch.setattr(logger, "log", lambda *a: lines.append(" ".join(str(x) for x in a)))
    step_fn()
    kv = _logged()
    for k in KEYS + (STREAM_KEYS if stream_keys else ()):
        assert k in kv, (k, sorted(kv))
    if not stream_keys:
        assert not any(k in kv for k in STREAM_KEYS)
    want = float(loop.opt.grad.double().norm())
    assert abs(kv["current_grad_norm"] / want - 1) <= ULP2 and kv["grad_norm"] == pytest.approx(kv["current_grad_norm"], rel=1e-6)
    assert kv["skipped_steps"] == 0 and loop.opt.steps == 1
    if stream_keys:
        assert 0 < kv["grad_norm_v"] and 0 < kv["grad_norm_a"]
        assert kv["grad_norm_v"] ** 2 + kv["grad_norm_a"] ** 2 <= kv["grad_norm"] ** 2 * (1 + 1e-6)
    loop.step += 1
    bad = 5
    undo = _poison(loop, bad)
    before = [t.clone() for t in (loop.opt.flat, loop.opt.m, loop.opt.v, *loop.opt.ema_params)]
    assert len(loop.opt.ema_params) == 2
    step_fn()
    for a, b in zip((loop.opt.flat, loop.opt.m, loop.opt.v, *loop.opt.ema_params), before):
        assert torch.equal(a, b)
    kv = _logged()
    assert loop.opt.steps == 1 and kv["skipped_steps"] == 1
    assert any(loop._names[bad] in ln and "skipped 1" in ln for ln in lines), lines
    loop.step += 1
    undo()
    step_fn()
    assert loop.opt.steps == 2 and _logged()["skipped_steps"] == 1 and np.isfinite(_logged()["current_grad_norm"])
    assert not torch.equal(loop.opt.flat, before[0]) and all(not torch.equal(a, b) for a, b in zip(loop.opt.ema_params, before[3:]))
    assert torch.isfinite(loop.opt.flat).all()


def test_trainloop_logs_norms_skips_and_recovers(tmp_path, monkeypatch):
    from test_trainloop_gpu import _mk
    _seed()
    model, loop = _mk(tmp_path / "a")
    assert loop.opt.guard
    _skip_and_recover(loop, lambda: loop.run_step(next(loop.data)), monkeypatch, stream_keys=True)
    # the optimizer state dict carries the steps TAKEN (2 of 3), and a resumed loop restores that count
    assert loop.step == 3
    osd = loop.opt_state_dict()
    assert all(float(st["step"]) == 2.0 for st in osd["state"].values())
    loop.save()
    _seed()
    _, loop2 = _mk(tmp_path / "a")
    assert loop2.resume_step == 3 and loop2.opt.steps == 2 and isinstance(loop2.opt.steps, int)
    assert torch.equal(loop2.opt.m, loop.opt.m) and torch.equal(loop2.opt.flat, loop.opt.flat)


def test_control_block_is_read_only_on_logging_steps(tmp_path):
    from test_trainloop_gpu import _mk
    _seed()
    model, loop = _mk(tmp_path / "b", log_interval=5)
    calls = []
    orig = loop.opt.read_control
    loop.opt.read_control = lambda: (calls.append(loop.step), orig())[1]
    batch = next(loop.data)
    for _ in range(5):
        loop.run_step(batch)
        if loop.step < 5:
            assert not calls, calls
        loop.step += 1
    assert calls == [5]
    kv = _logged()
    assert kv["skipped_steps"] == 0 and kv["grad_norm"] > 0 and kv["grad_norm"] != kv["current_grad_norm"]      # a mean over 5 steps


def test_graph_replayed_loop_is_guarded_too(tmp_path, monkeypatch):
    from test_trainloop_gpu import _mk
    _seed()
    model, loop = _mk(tmp_path / "c", microbatch=4, use_graph=True)
    batch = next(loop.data)
    _skip_and_recover(loop, lambda: loop.run_step(batch), monkeypatch, stream_keys=True)
    assert loop._gstep is not None


def test_sr_loop_is_guarded_too(tmp_path, monkeypatch):
    from test_sr_train_gpu import _mk_loop
    _seed()
    _, model, _, loop = _mk_loop(tmp_path / "d")
    low, hr, _, cond = next(loop.data)
    _skip_and_recover(loop, lambda: loop.run_step(hr, cond), monkeypatch, stream_keys=False)


def test_unguarded_loop_issues_the_old_single_launch(tmp_path, monkeypatch):
    from mm_diffusion import ops
    from test_trainloop_gpu import _mk
    _seed()
    model, loop = _mk(tmp_path / "e", guard_nonfinite=False)
    assert not loop.opt.guard
    calls = []
    old, new = ops.adamw_step, ops.adamw_step_guarded
    monkeypatch.setattr(ops, "adamw_step", lambda *a, **k: (calls.append("adamw_step"), old(*a, **k))[1])
    monkeypatch.setattr(ops, "adamw_step_guarded", lambda *a, **k: (calls.append("guarded"), new(*a, **k))[1])
    monkeypatch.setattr(ops, "sumsq_chunks", lambda *a, **k: calls.append("sumsq"))
    w0 = loop.opt.flat.clone()
    loop.run_step(next(loop.data))
    assert calls == ["adamw_step"] and loop.opt.steps == 1 and not torch.equal(w0, loop.opt.flat)
    kv = _logged()
    assert not any(k in kv for k in KEYS + STREAM_KEYS)


def test_poisoned_parameters_raise(tmp_path):
    from mm_diffusion._hip import MMDError
    from test_trainloop_gpu import _mk
    _seed()
    model, loop = _mk(tmp_path / "f")
    orig = loop.opt.all_reduce_grads

    def poisoned():                                     # as after a resume from a poisoned checkpoint, without an inf in the forward
        orig()
        loop.opt.flat[3] = float("inf")
    loop.opt.all_reduce_grads = poisoned
    with pytest.raises(MMDError, match="parameter norm"):
        loop.run_step(next(loop.data))
