"""Multimodal DPM-Solver / DPM-Solver++ driver on the MI355X HIP path.

Same public surface as the reference's `multimodal_dpm_solver_plus.py` (/root/reference/mm_diffusion/
multimodal_dpm_solver_plus.py): `NoiseScheduleVP`, `model_wrapper`, `DPM_Solver(model, betas=None,
alphas_cumprod=None, predict_x0=False, thresholding=False, ...)` with `.sample(x, steps, order, skip_type, method,
...)`, the single-step / multi-step update methods and the adaptive solver (Lu et al., DPM-Solver 2022 and
DPM-Solver++ 2022; the reference adapts the authors' public implementation to {"video", "audio"} dicts).

MI355X-first structure: all samples of a batch share the solver time, so every per-step coefficient (lambda, alpha,
sigma, phi_k, ...) is a HOST fp32 scalar computed with the same formulas as the reference (which evaluates them as
[B]-shaped device tensors, one tiny kernel per arithmetic op) and every state update
`x_t = c0 x + c1 model_s + c2 model_s1` is ONE fused kernel per stream (mmd_lincomb); dynamic thresholding is an
exact radix-select quantile + clamp (mmd_abs_quantile / mmd_clamp_scale); the adaptive error norm is mmd_dpm_err.

`DPM_Solver.sample_graph` runs the fixed-grid multistep method (orders 1 and 2) without any of those host scalars in the launch path:
the coefficients go into device tables indexed by the step number (`graph_tables`, built from the helpers the eager updates call) and
one evaluation is one graph replay per lane (sampler.DpmppStepper: mmd_dpmpp_x0 / mmd_dpmpp_select / mmd_dpmpp_update), bitwise the
eager loop, with batch lanes, seeded.CounterNoise and the partial masks of masked_sample_loop.  `DPM_Solver.sample_graph_singlestep`
does the same for the single-step method of orders 1-3 (the reference sampling script's call): `singlestep_tables` has one row per network
evaluation - a step of order p is p rows, at s, s1 and s2 - and the recorded update is mmd_dpm_single_update (sampler.DpmSingleStepper).
`DPM_Solver.sample_graph_sde` is the stochastic multistep solver in its data-prediction form (SDE-DPM-Solver++, orders 1 and 2; eager:
sample(method="multistep_sde")): `sde_tables` adds a noise coefficient per row, the recorded update mmd_dpmpp_sde_update draws or reads a
fresh z ~ N(0, I) inside the step graph (sampler.DpmppSdeStepper).  Generation quality is not assessed: there are no trained weights.
`DPM_Solver.sample_graph_adaptive` is the adaptive solver of order 2 (data prediction) with its step-size controller on the device: the
error norm, the accept test, the next step size and every coefficient derived from it stay in device memory (mmd_dpm_adapt_*,
sampler.DpmAdaptiveStepper), a trial step is two graph replays per lane and the host reads a status word every `poll` trial steps.
All share one driver (`_graph_loop`) and the stepper kept from the last call.

Reference behaviours reproduced knowingly:
  * the noise-prediction first-order update moves the AUDIO stream with the x0-form coefficients
    (sigma_t/sigma_s, alpha_t * expm1(h)) while video uses (alpha_t/alpha_s, sigma_t * expm1(h))   (dpm:576-584)
  * batch size 1 raises inside model_fn (`x.shape` on a dict, dpm:344-345)
Reference code paths that cannot execute there are not built and raise NotImplementedError with the reason:
third-order 'taylor' updates (dict arithmetic / undefined name, dpm:761-764,873), the multistep third-order update
and the noise-prediction multistep 'taylor' update (audio coefficients expanded to the VIDEO rank, dpm:1006-1013,
961: shape blow-up for B > 1), classifier / classifier-free guidance (tensor ops on the stream dict).
"""
import math

import torch

from . import _hip as H
from . import ops


class _Knots:
    """y(x), piecewise linear through ascending knots, the end segments extended outside (what the reference's interpolate_fn
    computes, dpm:1306-1347, for one curve): fp32, same expression order - the solver's integer model timesteps are floor((t - 1/N) N),
    so t must come out to the last bit."""

    def __init__(self, x, y):
        self.x, self.y = x.reshape(-1).cpu().contiguous(), y.reshape(-1).cpu().contiguous()     # dtypes kept: a float64 beta table gives float64 curves

    def __call__(self, q):
        q = q.reshape(-1).contiguous()
        x, y = self.x.to(q.device), self.y.to(q.device)
        ct = torch.promote_types(x.dtype, q.dtype)
        hi = torch.searchsorted(x.to(ct), q.to(ct), right=False).clamp(1, x.numel() - 1)         # first knot >= q, kept inside the table
        lo = hi - 1
        return y[lo] + (q - x[lo]) * (y[hi] - y[lo]) / (x[hi] - x[lo])

    def swapped(self):
        """x(y) of a DEcreasing curve: the knots reversed so that the abscissa ascends again."""
        return _Knots(self.y.flip(0), self.x.flip(0))


def interpolate_fn(x, xp, yp):
    """The reference's module-level helper (dpm:1306-1347), kept for its import surface: x [N, C], keypoints xp / yp [C, K] ->
    [N, C], one knot table per channel."""
    return torch.stack([_Knots(xp[c], yp[c])(x[:, c]) for c in range(xp.shape[0])], dim=1)


def _log_alpha_of_lambda(lamb):
    """log alpha = -1/2 log(1 + exp(-2 lambda)) for a VP process (alpha^2 + sigma^2 = 1, lambda = log alpha - log sigma)."""
    return -0.5 * torch.logaddexp(torch.zeros((1,)).to(lamb), -2. * lamb)


class _TableSchedule:
    """'discrete': log alpha known at t_i = (i + 1) / N from the trained betas / alphas_cumprod, linear in between."""

    def __init__(self, log_alphas):
        self.total_N, self.T = len(log_alphas), 1.
        self.curve = _Knots(torch.linspace(0., 1., self.total_N + 1)[1:], log_alphas)
        self.inverse = self.curve.swapped()

    def log_alpha(self, t):
        return self.curve(t)

    def t_of_lambda(self, lamb):
        return self.inverse(_log_alpha_of_lambda(lamb))


class _LinearSchedule:
    """'linear' VP-SDE: beta(t) = beta_0 + t (beta_1 - beta_0), log alpha(t) = -t^2 (beta_1 - beta_0) / 4 - t beta_0 / 2."""

    def __init__(self, beta_0, beta_1):
        self.total_N, self.T, self.b0, self.db = 1000, 1., beta_0, beta_1 - beta_0

    def log_alpha(self, t):
        return -0.25 * t ** 2 * self.db - 0.5 * t * self.b0

    def t_of_lambda(self, lamb):          # the positive root of the quadratic in t, in the cancellation-free form
        w = 2. * self.db * torch.logaddexp(-2. * lamb, torch.zeros((1,)).to(lamb))
        return w / (torch.sqrt(self.b0 ** 2 + w) + self.b0) / self.db


class _CosineSchedule:
    """'cosine': alpha(t) = cos(pi/2 (t + s) / (1 + s)) / cos(pi/2 s / (1 + s)), s = 0.008, T = 0.9946."""

    def __init__(self):
        self.total_N, self.T, self.s = 1000, 0.9946, 0.008
        self.log_alpha_0 = math.log(math.cos(self.s / (1. + self.s) * math.pi / 2.))

    def log_alpha(self, t):
        return torch.log(torch.cos((t + self.s) / (1. + self.s) * math.pi / 2.)) - self.log_alpha_0

    def t_of_lambda(self, lamb):
        la = -0.5 * torch.logaddexp(-2. * lamb, torch.zeros((1,)).to(lamb))
        return torch.arccos(torch.exp(la + self.log_alpha_0)) * 2. * (1. + self.s) / math.pi - self.s


class NoiseScheduleVP:
    """The VP noise schedule the solver integrates over (the reference's class of the same name, dpm:11-181): alpha(t), sigma(t),
    lambda(t) = log alpha - log sigma and its inverse for the 'discrete' (trained betas), 'linear' and 'cosine' families.  Times are
    fp32 torch tensors (any device; the solver's scalars live on the CPU)."""

    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None, continuous_beta_0=0.1, continuous_beta_1=20.):
        if schedule == "discrete":
            if betas is not None:
                log_alphas = 0.5 * torch.log(1 - torch.as_tensor(betas)).cumsum(dim=0)
            elif alphas_cumprod is not None:
                log_alphas = 0.5 * torch.log(torch.as_tensor(alphas_cumprod))
            else:
                raise ValueError("the 'discrete' noise schedule needs betas or alphas_cumprod")
            self._family = _TableSchedule(log_alphas)
        elif schedule == "linear":
            self._family = _LinearSchedule(continuous_beta_0, continuous_beta_1)
        elif schedule == "cosine":
            self._family = _CosineSchedule()
        else:
            raise ValueError(f"Unsupported noise schedule {schedule}. The schedule needs to be 'discrete' or 'linear' or 'cosine'")
        self.schedule, self.total_N, self.T = schedule, self._family.total_N, self._family.T

    # read-only counterparts of the attributes the reference's class exposes (dpm:113-118): nothing here uses them
    @property
    def t_array(self):
        if self.schedule != "discrete":
            raise AttributeError("t_array exists for the 'discrete' schedule only")
        return self._family.curve.x.reshape((1, -1))

    @property
    def log_alpha_array(self):
        if self.schedule != "discrete":
            raise AttributeError("log_alpha_array exists for the 'discrete' schedule only")
        return self._family.curve.y.reshape((1, -1))

    @property
    def beta_0(self):
        if self.schedule != "linear":
            raise AttributeError("beta_0 exists for the 'linear' schedule only")
        return self._family.b0

    @property
    def beta_1(self):
        if self.schedule != "linear":
            raise AttributeError("beta_1 exists for the 'linear' schedule only")
        return self._family.b0 + self._family.db

    def marginal_log_mean_coeff(self, t):
        shape = t.shape
        return self._family.log_alpha(t).reshape(shape) if self.schedule != "discrete" else self._family.log_alpha(t).reshape((-1))

    def marginal_alpha(self, t):
        return torch.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t):
        la = self.marginal_log_mean_coeff(t)
        return la - 0.5 * torch.log(1. - torch.exp(2. * la))

    def inverse_lambda(self, lamb):
        t = self._family.t_of_lambda(lamb)
        return t.reshape((-1,)) if self.schedule == "discrete" else t


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs={}, rescale=False):
    """Continuous-time noise prediction function over the {"video", "audio"} dict (dpm:183-370).  Only the
    configuration the reference's own callers use can run there: model_type 'noise', guidance_type 'uncond'."""
    assert model_type in ["noise", "x_start", "v"]
    assert guidance_type in ["uncond", "classifier", "classifier-free"]
    if model_type != "noise" or guidance_type != "uncond":
        raise NotImplementedError("the reference applies tensor arithmetic to the stream dict for model_type != 'noise' and for "
                                  "guided sampling (dpm:316-332,350-368) and raises; only ('noise', 'uncond') is built")

    def get_model_input_time(t_continuous):
        if noise_schedule.schedule == "discrete":
            max_step = 1000. if rescale else noise_schedule.total_N
            return ((t_continuous - 1. / noise_schedule.total_N) * max_step).to(torch.int)
        return t_continuous

    def model_fn(x, t_continuous):
        if t_continuous.reshape((-1,)).shape[0] == 1:
            t_continuous = t_continuous.expand((x.shape[0]))           # dict has no .shape: the reference's B = 1 failure
        t_input = get_model_input_time(t_continuous)
        video_output, audio_output = model(x["video"], x["audio"], t_input, **model_kwargs)
        if model.video_out_channels == 6:
            video_output = video_output[:, :, :3, ...]
        if model.audio_out_channels == 2:
            audio_output = audio_output[:, :1, ...]
        return {"video": video_output, "audio": audio_output}

    model_fn.get_model_input_time = get_model_input_time      # DPM_Solver.sample_graph tabulates the model timesteps with it
    return model_fn


def _f(v):
    """host fp32 scalar of a 1-element tensor."""
    return float(v.reshape(-1)[0])


def _comb(terms):
    """sum_i c_i * t_i for up to three (coefficient, fp32 tensor) terms as ONE kernel."""
    (ca, a), rest = terms[0], terms[1:]
    cb, b = rest[0] if len(rest) > 0 else (0.0, None)
    cc, c = rest[1] if len(rest) > 1 else (0.0, None)
    return ops.lincomb(a, ca, b, cb, c, cc)


class DPM_Solver:
    KEYS = ("video", "audio")        # state streams; the tensor-valued solver of the SR stage (dpm_solver_plus.py) uses ("x",)

    def _streams(self, fn):
        return {k: fn(k) for k in self.KEYS}

    def _batch(self, x):
        return x[self.KEYS[0]].shape[0]

    def __init__(self, model, betas=None, alphas_cumprod=None, predict_x0=False, thresholding=False, guidance_type="uncond",
                 max_val=1., model_kwargs={}, rescale=False):
        noise_schedule = NoiseScheduleVP(schedule="discrete", betas=betas, alphas_cumprod=alphas_cumprod)
        self.model = model_wrapper(model, noise_schedule, model_type="noise", model_kwargs=model_kwargs, guidance_type=guidance_type)
        self.raw_model, self.model_kwargs = model, model_kwargs
        self.noise_schedule = noise_schedule
        self.predict_x0 = predict_x0
        self.thresholding = thresholding
        self.max_val = max_val
        self.rescale = rescale
        self.nfe = 0

    # ------------------------------------------------------------------ model evaluations
    def _prep(self, x):
        for k in self.KEYS:
            H.require_cuda(x[k])
        return {k: x[k].float().contiguous() for k in self.KEYS}

    def noise_prediction_fn(self, x, t):
        self.nfe += 1
        t_dev = t.contiguous().to(x[self.KEYS[0]].device) if torch.is_tensor(t) else t
        out = self.model(x, t_dev)
        return {k: out[k].float().contiguous() for k in self.KEYS}

    def data_prediction_fn(self, x, t):
        """x0 = (x - sigma_t eps) / alpha_t, optionally with Imagen-style dynamic thresholding (dpm:419-440)."""
        noise = self.noise_prediction_fn(x, t)
        cx, ce = self._x0_coefs(t)
        x0 = {}
        for k in self.KEYS:
            v = ops.lincomb(x[k].float().contiguous(), cx, noise[k], ce)
            if self.thresholding:
                s = ops.abs_quantile(v, 0.995)          # p of the Imagen paper
                ops.clamp_scale_(v, s, self.max_val)
            x0[k] = v
        return x0

    def model_fn(self, x, t):
        return self.data_prediction_fn(x, t) if self.predict_x0 else self.noise_prediction_fn(x, t)

    # ------------------------------------------------------------------ time grids
    def get_time_steps(self, skip_type, t_T, t_0, N, device):
        if skip_type == "logSNR":
            lambda_T = self.noise_schedule.marginal_lambda(torch.tensor(t_T))
            lambda_0 = self.noise_schedule.marginal_lambda(torch.tensor(t_0))
            logSNR_steps = torch.linspace(lambda_T.item(), lambda_0.item(), N + 1)
            return self.noise_schedule.inverse_lambda(logSNR_steps).to(device)
        if skip_type == "time_uniform":
            return torch.linspace(t_T, t_0, N + 1).to(device)
        if skip_type == "time_quadratic":
            t_order = 2
            return torch.linspace(t_T ** (1. / t_order), t_0 ** (1. / t_order), N + 1).pow(t_order).to(device)
        raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")

    def get_orders_for_singlestep_solver(self, steps, order):
        if order == 3:
            K = steps // 3 + 1
            if steps % 3 == 0:
                return [3, ] * (K - 2) + [2, 1]
            if steps % 3 == 1:
                return [3, ] * (K - 1) + [1]
            return [3, ] * (K - 1) + [2]
        if order == 2:
            K = steps // 2
            return [2, ] * K if steps % 2 == 0 else [2, ] * K + [1]
        if order == 1:
            return [1, ] * steps
        raise ValueError("'order' must be '1' or '2' or '3'.")

    def _single_grid(self, steps, order, skip_type, method, t_T, t_0):
        """(orders, host time grid) of the single-step loop (dpm:1277-1284): 'singlestep' spends `steps` evaluations on steps of the
        orders get_orders_for_singlestep_solver lists, 'singlestep_fixed' on steps // order steps of the full order."""
        if method == "singlestep":
            orders = self.get_orders_for_singlestep_solver(steps=steps, order=order)
            timesteps = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=steps, device="cpu")
        else:
            K = steps // order
            orders = [order, ] * K
            timesteps = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=(K * order), device="cpu")
        return orders, timesteps

    def _single_ratios(self, timesteps, i, order):
        """(r1, r2) of the step of `order` that starts at grid point i: where its inner grid points lie in lambda (dpm:1290-1292)."""
        ns = self.noise_schedule
        tc = timesteps.detach().float().cpu()
        h = ns.marginal_lambda(tc[i + order]) - ns.marginal_lambda(tc[i])
        r1 = None if order <= 1 else (ns.marginal_lambda(tc[i + 1]) - ns.marginal_lambda(tc[i])) / h
        r2 = None if order <= 2 else (ns.marginal_lambda(tc[i + 2]) - ns.marginal_lambda(tc[i])) / h
        return r1, r2

    def denoise_fn(self, x, s):
        return self.data_prediction_fn(x, s)

    # ------------------------------------------------------------------ schedule scalars of one step
    def _sc(self, *times):
        """(lambda, log_alpha, sigma) host tensors [1] for each solver time (fp32, same formulas as the reference)."""
        ns = self.noise_schedule
        out = []
        for t in times:
            tc = t.detach().float().cpu().reshape(-1)[:1]
            out.append((ns.marginal_lambda(tc), ns.marginal_log_mean_coeff(tc), ns.marginal_std(tc)))
        return out

    # ------------------------------------------------------------------ coefficients: host scalars, shared by the eager updates and
    # the device tables of sample_graph (the kernels round them to fp32 on the way in, the tables when they are built)
    def _alpha_sigma(self, t):
        """(alpha_t, sigma_t) as host fp32 values."""
        tc = t.detach().float().cpu().reshape(-1)[:1]
        return _f(self.noise_schedule.marginal_alpha(tc)), _f(self.noise_schedule.marginal_std(tc))

    def _x0_coefs(self, t):
        """x0 = cx x + ce eps at time t (dpm:419-428)."""
        alpha_t, sigma_t = self._alpha_sigma(t)
        return 1.0 / alpha_t, -sigma_t / alpha_t

    def _first_coefs(self, s, t):
        """{stream: (c_x, c_model)} of the first-order update s -> t (dpm:532-590)."""
        (lam_s, la_s, sig_s), (lam_t, la_t, sig_t) = self._sc(s, t)
        h = lam_t - lam_s
        alpha_t = torch.exp(la_t)
        if self.predict_x0:
            phi_1 = torch.expm1(-h)
            c = {k: (_f(sig_t / sig_s), -_f(alpha_t * phi_1)) for k in self.KEYS}
        else:
            phi_1 = torch.expm1(h)
            # the audio stream takes the x0-form coefficients here, exactly like dpm:576-584
            c = {k: (_f(torch.exp(la_t - la_s)), -_f(sig_t * phi_1)) for k in self.KEYS}
            if "audio" in c:
                c["audio"] = (_f(sig_t / sig_s), -_f(alpha_t * phi_1))
        return c

    def _second_coefs(self, t_prev_1, t_prev_0, t, solver_type):
        """(c_x, c_model_prev_0, c_model_prev_1) of the multistep second-order update (dpm:889-947), D1_0 = (m0 - m1) / r0 expanded."""
        if solver_type not in ["dpm_solver", "taylor"]:
            raise ValueError(f"'solver_type' must be either 'dpm_solver' or 'taylor', got {solver_type}")
        if solver_type == "taylor" and not self.predict_x0:
            raise NotImplementedError("noise-prediction multistep 'taylor': the reference expands the audio coefficient to the video "
                                      "rank (dpm:961) - wrong shapes for B > 1")
        (lam_p1, _, _), (lam_p0, la_p0, sig_p0), (lam_t, la_t, sig_t) = self._sc(t_prev_1, t_prev_0, t)
        alpha_t = torch.exp(la_t)
        h_0, h = lam_p0 - lam_p1, lam_t - lam_p0
        r0 = h_0 / h
        inv_r0 = _f(1. / r0)
        if self.predict_x0:
            c0, c1 = _f(sig_t / sig_p0), -_f(alpha_t * (torch.exp(-h) - 1.))
            cd = (-0.5 * _f(alpha_t * (torch.exp(-h) - 1.))) if solver_type == "dpm_solver" else _f(alpha_t * ((torch.exp(-h) - 1.) / h + 1.))
        else:
            c0, c1 = _f(torch.exp(la_t - la_p0)), -_f(sig_t * (torch.exp(h) - 1.))
            cd = -0.5 * _f(sig_t * (torch.exp(h) - 1.))
        return c0, c1 + cd * inv_r0, -cd * inv_r0

    def _sde_coefs(self, t_prev_1, s, t):
        """(c0, c1, c2, cz) of the stochastic data-prediction update s -> t (SDE-DPM-Solver++, Lu et al. 2022): x_t = c0 x_s + c1 m0 + c2 m1
        + cz z with h = lambda_t - lambda_s, E = -expm1(-2 h): c0 = (sigma_t / sigma_s) e^-h, cm = alpha_t E, cz = sigma_t sqrt(E); first
        order (t_prev_1 None) c1 = cm, c2 = 0; second order, r0 = (lambda_s - lambda_prev) / h: c1 = cm (1 + 1 / (2 r0)), c2 = -cm / (2 r0).
        So c0 alpha_s + c1 + c2 = alpha_t and c0^2 sigma_s^2 + cz^2 = sigma_t^2: a perfect data prediction keeps the marginal.  Formed in
        float64 from _sc()'s fp32 values, each coefficient rounded to fp32 once."""
        import numpy as np
        (lam_s, _, sig_s), (lam_t, la_t, sig_t) = (tuple(float(v.reshape(-1)[0]) for v in sc) for sc in self._sc(s, t))
        h = lam_t - lam_s
        E = -math.expm1(-2. * h)
        c0, cm, cz = sig_t / sig_s * math.exp(-h), math.exp(la_t) * E, sig_t * math.sqrt(E)
        c1, c2 = cm, 0.
        if t_prev_1 is not None:
            r0 = (lam_s - float(self._sc(t_prev_1)[0][0].reshape(-1)[0])) / h
            c1, c2 = cm * (1. + 0.5 / r0), -cm * 0.5 / r0
        return tuple(float(np.float32(v)) for v in (c0, c1, c2, cz))

    @staticmethod
    def _ratio(r):
        """a step ratio r1 / r2 (host tensor of sample(), or a number) as a host fp32 tensor [1]."""
        return r.detach().float().cpu().reshape(-1)[:1] if torch.is_tensor(r) else torch.tensor([float(r)])

    def _single_second_coefs(self, s, t, r1, solver_type):
        """The single-step second-order update s -> t (dpm:590-704): (s1, (a1, b1), (c0, c1, c2)) with x_s1 = a1 x + b1 m_s and
        x_t = c0 x + c1 m_s + c2 m_s1 (c1 has the -c2 of c2 (m_s1 - m_s) in it, formed in double and rounded once by the kernel's argument)."""
        if solver_type not in ["dpm_solver", "taylor"]:
            raise ValueError(f"'solver_type' must be either 'dpm_solver' or 'taylor', got {solver_type}")
        r1t = self._ratio(0.5 if r1 is None else r1)
        (lam_s, la_s, sig_s), (lam_t, la_t, sig_t) = self._sc(s, t)
        h = lam_t - lam_s
        s1 = self.noise_schedule.inverse_lambda(lam_s + r1t * h)
        (_, la_s1, sig_s1), = self._sc(s1)
        alpha_s1, alpha_t = torch.exp(la_s1), torch.exp(la_t)
        r1f = _f(r1t)
        if self.predict_x0:
            phi_11, phi_1 = torch.expm1(-r1t * h), torch.expm1(-h)
            a1, b1 = _f(sig_s1 / sig_s), -_f(alpha_s1 * phi_11)
            c0, c1 = _f(sig_t / sig_s), -_f(alpha_t * phi_1)
            c2 = (-(0.5 / r1f) * _f(alpha_t * phi_1)) if solver_type == "dpm_solver" else \
                ((1. / r1f) * _f(alpha_t * ((torch.exp(-h) - 1.) / h + 1.)))
        else:
            phi_11, phi_1 = torch.expm1(r1t * h), torch.expm1(h)
            a1, b1 = _f(torch.exp(la_s1 - la_s)), -_f(sig_s1 * phi_11)
            c0, c1 = _f(torch.exp(la_t - la_s)), -_f(sig_t * phi_1)
            c2 = (-(0.5 / r1f) * _f(sig_t * phi_1)) if solver_type == "dpm_solver" else \
                (-(1. / r1f) * _f(sig_t * ((torch.exp(h) - 1.) / h - 1.)))
        return s1, (a1, b1), (c0, c1 - c2, c2)

    def _single_third_coefs(self, s, t, r1, r2, solver_type):
        """The single-step third-order update s -> t (dpm:706-887): (s1, s2, (a1, b1), (a2, b2, d2), (c0, c1, c2)) with
        x_s1 = a1 x + b1 m_s, x_s2 = a2 x + b2 m_s + d2 m_s1 and x_t = c0 x + c1 m_s + c2 m_s2 (b2 and c1 hold the -d2 and -c2 of the
        differences, formed in double)."""
        if solver_type not in ["dpm_solver", "taylor"]:
            raise ValueError(f"'solver_type' must be either 'dpm_solver' or 'taylor', got {solver_type}")
        if solver_type == "taylor":
            raise NotImplementedError("third-order 'taylor' update: the reference subtracts stream dicts (dpm:761-764) / reads an "
                                      "undefined name (dpm:873) and raises")
        r1t, r2t = self._ratio(1. / 3. if r1 is None else r1), self._ratio(2. / 3. if r2 is None else r2)
        ns = self.noise_schedule
        (lam_s, la_s, sig_s), (lam_t, la_t, sig_t) = self._sc(s, t)
        h = lam_t - lam_s
        s1, s2 = ns.inverse_lambda(lam_s + r1t * h), ns.inverse_lambda(lam_s + r2t * h)
        (_, la_s1, sig_s1), (_, la_s2, sig_s2) = self._sc(s1, s2)
        alpha_s1, alpha_s2, alpha_t = torch.exp(la_s1), torch.exp(la_s2), torch.exp(la_t)
        r1f, r2f = _f(r1t), _f(r2t)
        if self.predict_x0:
            phi_11, phi_12, phi_1 = torch.expm1(-r1t * h), torch.expm1(-r2t * h), torch.expm1(-h)
            phi_22 = torch.expm1(-r2t * h) / (r2t * h) + 1.
            phi_2 = phi_1 / h + 1.
            a1, b1 = _f(sig_s1 / sig_s), -_f(alpha_s1 * phi_11)
            a2, b2, d2 = _f(sig_s2 / sig_s), -_f(alpha_s2 * phi_12), (r2f / r1f) * _f(alpha_s2 * phi_22)
            c0, c1, c2 = _f(sig_t / sig_s), -_f(alpha_t * phi_1), (1. / r2f) * _f(alpha_t * phi_2)
        else:
            phi_11, phi_12, phi_1 = torch.expm1(r1t * h), torch.expm1(r2t * h), torch.expm1(h)
            phi_22 = torch.expm1(r2t * h) / (r2t * h) - 1.
            phi_2 = phi_1 / h - 1.
            a1, b1 = _f(torch.exp(la_s1 - la_s)), -_f(sig_s1 * phi_11)
            a2, b2, d2 = _f(torch.exp(la_s2 - la_s)), -_f(sig_s2 * phi_12), -(r2f / r1f) * _f(sig_s2 * phi_22)
            c0, c1, c2 = _f(torch.exp(la_t - la_s)), -_f(sig_t * phi_1), -(1. / r2f) * _f(sig_t * phi_2)
        return s1, s2, (a1, b1), (a2, b2 - d2, d2), (c0, c1 - c2, c2)

    # ------------------------------------------------------------------ first order (DDIM)
    def dpm_solver_first_update(self, x, s, t, model_s=None, return_intermediate=False):
        c = self._first_coefs(s, t)
        x = self._prep(x)
        if model_s is None:
            model_s = self.model_fn(x, s)
        x_t = self._streams(lambda k: _comb([(c[k][0], x[k]), (c[k][1], model_s[k])]))
        return (x_t, {"model_s": model_s}) if return_intermediate else x_t

    # ------------------------------------------------------------------ single-step second order
    def singlestep_dpm_solver_second_update(self, x, s, t, r1=0.5, model_s=None, return_intermediate=False, solver_type="dpm_solver"):
        s1, (a1, b1), (c0, c1, c2) = self._single_second_coefs(s, t, r1, solver_type)
        x = self._prep(x)
        B = self._batch(x)
        if model_s is None:
            model_s = self.model_fn(x, s)
        x_s1 = self._streams(lambda k: _comb([(a1, x[k]), (b1, model_s[k])]))
        model_s1 = self.model_fn(x_s1, s1.expand(B))
        # c0 x + c1 m_s + c2 (m_s1 - m_s)
        x_t = self._streams(lambda k: _comb([(c0, x[k]), (c1, model_s[k]), (c2, model_s1[k])]))
        return (x_t, {"model_s": model_s, "model_s1": model_s1}) if return_intermediate else x_t

    # ------------------------------------------------------------------ single-step third order
    def singlestep_dpm_solver_third_update(self, x, s, t, r1=1. / 3., r2=2. / 3., model_s=None, model_s1=None, return_intermediate=False,
                                           solver_type="dpm_solver"):
        s1, s2, (a1, b1), (a2, b2, d2), (c0, c1, c2) = self._single_third_coefs(s, t, r1, r2, solver_type)
        x = self._prep(x)
        B = self._batch(x)
        if model_s is None:
            model_s = self.model_fn(x, s)
        if model_s1 is None:
            x_s1 = self._streams(lambda k: _comb([(a1, x[k]), (b1, model_s[k])]))
            model_s1 = self.model_fn(x_s1, s1.expand(B))
        x_s2 = self._streams(lambda k: _comb([(a2, x[k]), (b2, model_s[k]), (d2, model_s1[k])]))
        model_s2 = self.model_fn(x_s2, s2.expand(B))
        x_t = self._streams(lambda k: _comb([(c0, x[k]), (c1, model_s[k]), (c2, model_s2[k])]))
        if return_intermediate:
            return x_t, {"model_s": model_s, "model_s1": model_s1, "model_s2": model_s2}
        return x_t

    # ------------------------------------------------------------------ multistep
    def multistep_dpm_solver_second_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpm_solver"):
        model_prev_1, model_prev_0 = model_prev_list
        t_prev_1, t_prev_0 = t_prev_list
        c0, cm0, cm1 = self._second_coefs(t_prev_1, t_prev_0, t, solver_type)
        x = self._prep(x)
        return self._streams(lambda k: _comb([(c0, x[k]), (cm0, model_prev_0[k]), (cm1, model_prev_1[k])]))

    def multistep_dpm_solver_third_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpm_solver"):
        raise NotImplementedError("multistep third-order update: the reference expands every audio coefficient to the video rank "
                                  "(dpm:1006-1013) - the audio state becomes [B,1,B,C,L] for B > 1 and B = 1 fails earlier")

    def singlestep_dpm_solver_update(self, x, s, t, order, return_intermediate=False, solver_type="dpm_solver", r1=None, r2=None):
        if order == 1:
            return self.dpm_solver_first_update(x, s, t, return_intermediate=return_intermediate)
        if order == 2:
            return self.singlestep_dpm_solver_second_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type, r1=r1)
        if order == 3:
            return self.singlestep_dpm_solver_third_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type, r1=r1, r2=r2)
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")

    def multistep_dpm_solver_update(self, x, model_prev_list, t_prev_list, t, order, solver_type="dpm_solver"):
        if order == 1:
            return self.dpm_solver_first_update(x, t_prev_list[-1], t, model_s=model_prev_list[-1])
        if order == 2:
            return self.multistep_dpm_solver_second_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        if order == 3:
            return self.multistep_dpm_solver_third_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")

    # ------------------------------------------------------------------ adaptive step size
    def dpm_solver_adaptive(self, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, solver_type="dpm_solver",
                            verbose=False):
        """Embedded-pair step-size control (dpm:1088-1149).  The accept test and the next step size need the error on
        the host: one scalar read-back per trial step."""
        ns = self.noise_schedule
        x = self._prep(x)
        dev, B = x[self.KEYS[0]].device, self._batch(x)
        s = t_T * torch.ones((1,))
        lambda_s = ns.marginal_lambda(s)
        lambda_0 = ns.marginal_lambda(t_0 * torch.ones_like(s))
        h = h_init * torch.ones_like(s)
        x_prev = x
        nfe = 0
        if order == 2:
            r1 = 0.5
            lower_update = lambda x, s, t: self.dpm_solver_first_update(x, s, t, return_intermediate=True)                       # noqa: E731
            higher_update = lambda x, s, t, **kw: self.singlestep_dpm_solver_second_update(x, s, t, r1=r1, solver_type=solver_type, **kw)   # noqa: E731
        elif order == 3:
            r1, r2 = 1. / 3., 2. / 3.
            lower_update = lambda x, s, t: self.singlestep_dpm_solver_second_update(x, s, t, r1=r1, return_intermediate=True, solver_type=solver_type)   # noqa: E731
            higher_update = lambda x, s, t, **kw: self.singlestep_dpm_solver_third_update(x, s, t, r1=r1, r2=r2, solver_type=solver_type, **kw)         # noqa: E731
        else:
            raise ValueError(f"For adaptive step size solver, order must be 2 or 3, got {order}")
        nk = len(self.KEYS)
        acc = torch.zeros(nk * B, dtype=torch.float64, device=dev)
        while torch.abs((s - t_0)).mean() > t_err:
            if verbose:
                print(f"{torch.abs((s - t_0)).mean()} > {t_err}")
            t = ns.inverse_lambda(lambda_s + h)
            vs, vt = s.expand(B), t.expand(B)
            x_lower, lower_noise_kwargs = lower_update(x, vs, vt)
            x_higher = higher_update(x, vs, vt, **lower_noise_kwargs)
            acc.zero_()
            for i, k in enumerate(self.KEYS):
                ops.dpm_err(x_higher[k], x_lower[k], x_prev[k], atol, rtol, acc[i * B:(i + 1) * B])
            per = torch.tensor([v for k in self.KEYS for v in [x[k][0].numel()] * B], dtype=torch.float64, device=dev)
            E = torch.sqrt(acc / per).max().float().cpu()
            if torch.all(E <= 1.):
                x = x_higher
                s = t
                x_prev = x_lower
                lambda_s = ns.marginal_lambda(s)
            h = torch.min(theta * h * torch.float_power(E, -1. / order).float(), lambda_0 - lambda_s)
            nfe += order
        if verbose:
            print("adaptive solver nfe", nfe)
        return x

    # ------------------------------------------------------------------ driver
    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type="time_uniform", method="singlestep", denoise=False,
               solver_type="dpm_solver", atol=0.0078, rtol=0.05, noise_source=None):
        """method "multistep_sde": the stochastic data-prediction multistep solver of orders 1 and 2 (_sample_sde); noise_source (that
        method only): None = torch.randn, or a seeded.CounterNoise."""
        t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
        t_T = self.noise_schedule.T if t_start is None else t_start
        if method == "multistep_sde":
            return self._sample_sde(x, steps, order, skip_type, denoise, solver_type, t_T, t_0, noise_source)
        if noise_source is not None:
            raise H.MMDError(f"sample: method {method!r} is deterministic and draws nothing: noise_source goes with 'multistep_sde' only")
        x = self._prep(x)
        device, B = x[self.KEYS[0]].device, self._batch(x)
        with torch.no_grad():
            if method == "adaptive":
                x = self.dpm_solver_adaptive(x, order=order, t_T=t_T, t_0=t_0, atol=atol, rtol=rtol, solver_type=solver_type)
            elif method == "multistep":
                assert steps >= order
                # the time grid stays on the HOST: every coefficient is a host scalar, so no step waits on the device; the model's
                # integer timestep is uploaded asynchronously inside noise_prediction_fn
                timesteps = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=steps, device="cpu")
                assert timesteps.shape[0] - 1 == steps
                vec_t = timesteps[0].expand(B)
                model_prev_list = [self.model_fn(x, vec_t)]
                t_prev_list = [vec_t]
                for init_order in range(1, order):        # lower-order warm-up
                    vec_t = timesteps[init_order].expand(B)
                    x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, vec_t, init_order, solver_type=solver_type)
                    model_prev_list.append(self.model_fn(x, vec_t))
                    t_prev_list.append(vec_t)
                for step in range(order, steps + 1):
                    vec_t = timesteps[step].expand(B)
                    x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, vec_t, order, solver_type=solver_type)
                    for i in range(order - 1):
                        t_prev_list[i] = t_prev_list[i + 1]
                        model_prev_list[i] = model_prev_list[i + 1]
                    t_prev_list[-1] = vec_t
                    if step < steps:                      # the final model value is never used
                        model_prev_list[-1] = self.model_fn(x, vec_t)
            elif method in ["singlestep", "singlestep_fixed"]:
                orders, timesteps = self._single_grid(steps, order, skip_type, method, t_T, t_0)
                i = 0
                for order in orders:
                    vec_s, vec_t = timesteps[i].expand(B), timesteps[i + order].expand(B)
                    r1, r2 = self._single_ratios(timesteps, i, order)
                    x = self.singlestep_dpm_solver_update(x, vec_s, vec_t, order, solver_type=solver_type, r1=r1, r2=r2)
                    i += order
        if denoise:
            x = self.denoise_fn(x, torch.ones((B,)) * t_0)
        return x

    # ------------------------------------------------------------------ stochastic multistep solver (SDE-DPM-Solver++)
    def _sde_check(self, who, steps, order, solver_type="dpm_solver"):
        if not self.predict_x0:
            raise H.MMDError(f"{who}: the stochastic solver is built in its data-prediction form only (predict_x0=True): the reference's "
                             "noise-prediction first update moves the audio stream with x0-form coefficients (dpm:576-584), and that form does "
                             "not keep the marginal")
        if order not in (1, 2):
            raise H.MMDError(f"{who}: order must be 1 or 2 (no third-order stochastic update is built); got {order}")
        if solver_type != "dpm_solver":
            raise H.MMDError(f"{who}: solver_type must be 'dpm_solver' (the stochastic update has one form), got {solver_type!r}")
        steps = int(steps)
        if steps < order:
            raise H.MMDError(f"{who}: steps ({steps}) must be at least the order ({order})")
        return steps

    def multistep_sde_update(self, x, m0, m1, coefs, z):
        """x_t = c0 x + c1 m0 (+ c2 m1) + cz z per stream from the kernels of the deterministic updates: one mmd_lincomb for the
        deterministic terms (m1 None: first order), then mmd_lincomb(v, 1, z, cz).  coefs = _sde_coefs' tuple, z = {stream: N(0, 1)}."""
        c0, c1, c2, cz = coefs
        x = self._prep(x)
        out = {}
        for k in self.KEYS:
            v = _comb([(c0, x[k]), (c1, m0[k])] + ([(c2, m1[k])] if m1 is not None else []))
            out[k] = ops.lincomb(v, 1.0, z[k].float().contiguous(), cz)
        return out

    def _sample_sde(self, x, steps, order, skip_type, denoise, solver_type, t_T, t_0, noise_source):
        """sample(method="multistep_sde"): the multistep loop's structure with a fresh z ~ N(0, I) at every update - torch.randn, video
        first, then audio, or noise_source.randn(shape, tag, draw=i) of a seeded.CounterNoise at evaluation i, whose window shifts then
        come from the counter too (x is expected to be its X_T draw) - and none at the closing denoise evaluation."""
        from .seeded import CounterNoise, TAG_AUDIO, TAG_VIDEO
        steps = self._sde_check("sample(method='multistep_sde')", steps, order, solver_type)
        if self.KEYS != ("video", "audio"):
            raise H.MMDError("sample(method='multistep_sde'): the stochastic solver is built for the multimodal base model's "
                             "{'video', 'audio'} state only")
        ctr = noise_source
        if ctr is not None and not isinstance(ctr, CounterNoise):
            raise H.MMDError("sample(method='multistep_sde'): noise_source must be a seeded.CounterNoise or None")
        tags = {"video": TAG_VIDEO, "audio": TAG_AUDIO}
        x = self._prep(x)
        device, B = x[self.KEYS[0]].device, self._batch(x)
        def evaluate(fn, x, i, t):      # evaluation i: with a counter its window shifts are the counter's at draw i
            if ctr is None:
                return fn(x, t)
            ctr.set_draw(i)
            with ctr.shifting(self.raw_model):
                return fn(x, t)
        with torch.no_grad():
            timesteps = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=steps, device="cpu")
            m1 = None
            for i in range(steps):
                m0 = evaluate(self.model_fn, x, i, timesteps[i].expand(B))
                second = order == 2 and i > 0
                coefs = self._sde_coefs(timesteps[i - 1:i] if second else None, timesteps[i:i + 1], timesteps[i + 1:i + 2])
                if ctr is not None:
                    z = {k: ctr.randn(tuple(x[k].shape), tags[k], i, device) for k in self.KEYS}
                else:
                    z = {k: torch.randn(tuple(x[k].shape), device=device) for k in self.KEYS}
                x = self.multistep_sde_update(x, m0, m1 if second else None, coefs, z)
                m1 = m0
            if denoise:
                x = evaluate(self.denoise_fn, x, steps, torch.ones((B,)) * t_0)
        return x

    def sde_tables(self, steps, order=2, skip_type="logSNR", denoise=False, device="cpu"):
        """graph_tables' dictionary for sample_graph_sde, plus "cz": {stream: float32 [rows]}, the noise coefficient of each row (0 at the
        denoise row).  Rows and kinds as in graph_tables - row 0 first order, the denoise row last - with c0, c1, c2, cz from _sde_coefs,
        the helper the eager method calls."""
        import numpy as np
        steps = self._sde_check("sde_tables", steps, order)
        key = (steps, order, skip_type, bool(denoise), str(device))
        cache = self.__dict__.setdefault("_sde_tables", {})
        if key not in cache:
            cache[key] = self._build_sde_tables(np, steps, order, skip_type, denoise, device)
        return cache[key]

    def _build_sde_tables(self, np, steps, order, skip_type, denoise, device):
        t_0, t_T = 1. / self.noise_schedule.total_N, self.noise_schedule.T
        grid = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=steps, device="cpu")
        times = [grid[i:i + 1] for i in range(steps + 1)]
        evals, cz = [], np.zeros(steps + (1 if denoise else 0), dtype=np.float32)
        for i in range(steps):
            second = order == 2 and i > 0
            c0, c1, c2, cz[i] = self._sde_coefs(times[i - 1] if second else None, times[i], times[i + 1])
            evals.append((times[i], self._same((c0, c1, c2, ops.DPMPP_KIND_SECOND if second else ops.DPMPP_KIND_FIRST))))
        return self._eval_tables(np, evals, denoise, device, cz=cz)

    def sample_graph_sde(self, x_T=None, *, shape=None, steps, order=2, skip_type="logSNR", denoise=False, known=None, mask=None,
                         noise_source=None, paste_known=True, use_graph=True, lanes=None):
        """sample(method="multistep_sde") as one graph replay per lane and evaluation (sampler.DpmppSdeStepper, the tables of sde_tables):
        the same x_T, window-shift stream and torch device seed give the same bits.  The update draws its noise inside the step graph:
        with a seeded.CounterNoise in the kernel, at draw = the evaluation number (sample k of a seed is then the same at any batch and
        lane count, on the graph and the eager path), else from full-batch buffers refilled before every update row in the eager order.
        x_T / shape, known / mask / paste_known, use_graph and lanes as in sample_graph: the known cells are set to alpha(t) known +
        sigma(t) eps (eps = that stream's x_T) before every evaluation, so the unknown part is re-randomised at every step around them.
        Data prediction (predict_x0=True), orders 1 and 2; batch 1 is accepted."""
        from .sampler import DpmppSdeStepper
        return self._graph_loop("sample_graph_sde", DpmppSdeStepper, lambda: self._sde_check("sample_graph_sde", steps, order),
                                lambda device: self.sde_tables(steps, order, skip_type, denoise, device=device),
                                x_T, shape, known, mask, noise_source, paste_known, use_graph, lanes)

    # ------------------------------------------------------------------ graph-replayed multistep loop
    def graph_tables(self, steps, order=2, skip_type="logSNR", solver_type="dpm_solver", denoise=False, device="cpu"):
        """The per-evaluation tables of sample_graph, from the very helpers the eager updates call on the same host fp32 time grid.
        Row i < steps: evaluation at timesteps[i] and the update to timesteps[i + 1] (first order at i == 0 or order == 1, else second
        order); row `steps` (denoise): the final data prediction at t_0.  Returns {"rows", "timesteps" (fp32 [rows], host),
        "tab": {stream: float32 [6, rows] = cx, ce, c0, c1, c2, kind}, "tab2": float32 [2, rows] = alpha, sigma (mmd_cond_replace's table),
        "tm": the model's integer timesteps, get_model_input_time evaluated on `device` as the eager path evaluates it}."""
        import numpy as np
        steps = self._graph_check(steps, order, solver_type)
        # kept per argument set: a sampling call otherwise spends the host time of every evaluation's scalars before its first launch
        key = (steps, order, skip_type, solver_type, bool(denoise), str(device), bool(self.predict_x0))
        cache = self.__dict__.setdefault("_graph_tables", {})
        if key not in cache:
            cache[key] = self._build_graph_tables(np, steps, order, skip_type, solver_type, denoise, device)
        return cache[key]

    def _build_graph_tables(self, np, steps, order, skip_type, solver_type, denoise, device):
        t_0, t_T = 1. / self.noise_schedule.total_N, self.noise_schedule.T
        grid = self.get_time_steps(skip_type=skip_type, t_T=t_T, t_0=t_0, N=steps, device="cpu")
        times = [grid[i:i + 1] for i in range(steps + 1)]
        evals = []
        for i in range(steps):
            if i == 0 or order == 1:      # per stream: the noise-prediction form moves the audio stream with other coefficients (_first_coefs)
                c = {k: v + (0.0, ops.DPMPP_KIND_FIRST) for k, v in self._first_coefs(times[i], times[i + 1]).items()}
            else:
                c = self._same(self._second_coefs(times[i - 1], times[i], times[i + 1], solver_type) + (ops.DPMPP_KIND_SECOND,))
            evals.append((times[i], c))
        return self._eval_tables(np, evals, denoise, device)

    def _same(self, c):
        return {k: c for k in self.KEYS}

    def _eval_tables(self, np, evals, denoise, device, cz=None):
        """The tables dictionary of graph_tables from evals = [(time [1], {stream: (c0, c1, c2, kind)})], one entry per network evaluation
        in the loop's order; denoise: one more row at t_0, the final data prediction.  Slots 0, 1 of a row are the data prediction's
        (cx, ce) where the row's model value is one (predict_x0, and the denoise row of either form), else zeros.  cz: float32 [rows], the
        rows' noise coefficients (sde_tables), the same for every stream."""
        if denoise:
            evals = evals + [(torch.ones((1,)) * (1. / self.noise_schedule.total_N), self._same((0.0, 0.0, 0.0, ops.DPMPP_KIND_DENOISE)))]
        rows = len(evals)
        tab = {k: np.zeros((ops.DPMPP_TAB_ROWS, rows), dtype=np.float32) for k in self.KEYS}
        tab2 = np.zeros((2, rows), dtype=np.float32)
        for j, (tau, c) in enumerate(evals):
            tab2[:, j] = self._alpha_sigma(tau)
            cx, ce = self._x0_coefs(tau) if (self.predict_x0 or c[self.KEYS[0]][3] == ops.DPMPP_KIND_DENOISE) else (0.0, 0.0)
            for k in self.KEYS:
                tab[k][:, j] = (cx, ce) + tuple(c[k])
        times = torch.cat([tau.reshape(-1)[:1] for tau, _ in evals])
        tm = self.model.get_model_input_time(times.to(device))
        out = {"rows": rows, "timesteps": times, "tab": tab, "tab2": tab2, "tm": [int(v) for v in tm.cpu()]}
        if cz is not None:
            out["cz"] = {k: cz.copy() for k in self.KEYS}
        return out

    def _graph_check(self, steps, order, solver_type):
        if order not in (1, 2):
            raise H.MMDError(f"sample_graph: order must be 1 or 2 (the reference's third-order multistep update cannot run, dpm:1006-1013); got {order}")
        if solver_type not in ("dpm_solver", "taylor"):
            raise H.MMDError(f"sample_graph: solver_type must be 'dpm_solver' or 'taylor', got {solver_type!r}")
        if solver_type == "taylor" and not self.predict_x0 and order == 2:
            raise H.MMDError("sample_graph: solver_type 'taylor' needs predict_x0 (the reference's noise-prediction 'taylor' update has wrong shapes, dpm:961)")
        steps = int(steps)
        if steps < order:
            raise H.MMDError(f"sample_graph: steps ({steps}) must be at least the order ({order})")
        return steps

    def sample_graph(self, x_T=None, *, shape=None, steps, order=2, skip_type="logSNR", solver_type="dpm_solver", denoise=False, known=None,
                     mask=None, noise_source=None, paste_known=True, use_graph=True, lanes=None, method="multistep"):
        """sample(method="multistep") as one graph replay per lane and evaluation (sampler.DpmppStepper): the same x_T and window-shift
        stream give the same bits.  x_T: {"video", "audio"} device tensors, or `shape` = {"video": (B,F,C,H,W), "audio": (B,C,L)} to draw
        it.  noise_source: a seeded.CounterNoise - x_T is then its start draw (passing x_T as well raises), the window shifts and the
        conditioning noise come from the counter, and sample k of a seed is the same at any batch and lane count.  known / mask: the
        replacement method of masked_sample_loop (masking.normalize has the shapes): before every evaluation the known cells are set to
        alpha(t) known + sigma(t) eps with eps = that stream's x_T; with paste_known the result carries `known` itself there.  Orders 1
        and 2 of the fixed-grid multistep method only (the single-step method: sample_graph_singlestep); batch 1 is accepted."""
        from .sampler import DpmppStepper
        if method != "multistep":
            raise H.MMDError(f"sample_graph: only method 'multistep' is recorded here, got {method!r}: the single-step solver has "
                             "sample_graph_singlestep, the adaptive solver sample_graph_adaptive")
        return self._graph_loop("sample_graph", DpmppStepper, lambda: self._graph_check(steps, order, solver_type),
                                lambda device: self.graph_tables(steps, order, skip_type, solver_type, denoise, device=device),
                                x_T, shape, known, mask, noise_source, paste_known, use_graph, lanes)

    def _graph_loop(self, who, stepper_cls, check, tables, x_T, shape, known, mask, noise_source, paste_known, use_graph, lanes, drive=None,
                    stepper_kw=None):
        """What the graph-replayed loops share: the argument checks (check() has the method's own), the drawing of x_T, the conditioning,
        the kept stepper of class stepper_cls with the tables of tables(device), and one stepper.step per table row - or drive(stepper),
        the loop of a method whose evaluations no table lists (its return value is handed back next to the samples).  stepper_kw: further
        constructor arguments of the stepper; they are part of the kept stepper's key."""
        stepper_kw = dict(stepper_kw or {})
        from . import masking, sampler
        from .sampler import unwrap_unet
        from .seeded import CounterNoise, TAG_AUDIO, TAG_VIDEO, X_T
        if self.model_kwargs:
            raise H.MMDError(f"{who}: model_kwargs cannot be recorded into the step graph - use sample()")
        check()
        ctr = noise_source
        if ctr is not None and not isinstance(ctr, CounterNoise):
            raise H.MMDError(f"{who}: noise_source must be a seeded.CounterNoise or None")
        if ctr is not None and x_T is not None:
            raise H.MMDError(f"{who}: a CounterNoise source draws x_T itself: x_T must be None")
        if x_T is None and shape is None:
            raise H.MMDError(f"{who}: give x_T or shape")
        if x_T is not None:
            for k in self.KEYS:
                H.require_cuda(x_T[k])
            device = x_T[self.KEYS[0]].device
            shape = {k: tuple(x_T[k].shape) for k in self.KEYS}
        unet = unwrap_unet(self.raw_model)
        if unet is None:
            raise H.MMDError(f"{who}: the model is no MultimodalUNet (or a wrapper of one)")
        if x_T is None:
            device = next(unet.parameters()).device
            if device.type != "cuda":
                raise H.MMDError(f"{who} runs on the MI355X HIP path only (the model must be on a GPU); no CPU fallback")
            shape = {k: tuple(int(v) for v in shape[k]) for k in self.KEYS}
        tabs = tables(device)
        if mask is not None and known is None:
            raise H.MMDError(f"{who}: mask without known")
        cond = masking.to_device(masking.normalize(known, mask, shape), device) if known is not None else {}
        if x_T is None:
            if ctr is not None:
                x_T = {"video": ctr.randn(shape["video"], TAG_VIDEO, X_T, device), "audio": ctr.randn(shape["audio"], TAG_AUDIO, X_T, device)}
            else:
                x_T = {k: torch.randn(*shape[k]).to(device) for k in self.KEYS}
        x_T = {k: x_T[k].float().contiguous() for k in self.KEYS}
        # the stepper of the last call is kept: another call of the same kind, shape and structure reloads its tables and replays its graphs
        B = shape["video"][0]
        key = (stepper_cls.__name__, B, sampler.default_lanes(B) if lanes is None else int(lanes), bool(use_graph), ctr is not None,
               sampler.DPMPP_SELECT, tuple((k, c.mask is not None) for k, c in sorted(cond.items())), bool(self.predict_x0),
               bool(self.thresholding), float(self.max_val), str(device), id(unet), tuple(sorted(stepper_kw.items())))
        kept = getattr(self, "_stepper", None)
        self._stepper = None
        with torch.no_grad():
            if kept is not None and kept[0] == key and kept[1].usable():
                stepper = kept[1]
                stepper.retable(tabs, ctr)
            else:
                if kept is not None:
                    kept[1].close()
                stepper = stepper_cls(self, unet, B, device, tabs, use_graph=use_graph, lanes=lanes, cond=cond, ctr=ctr, **stepper_kw)
            try:
                stepper.load(x_T["video"], x_T["audio"])
                if cond:
                    stepper.load_cond(cond, x_T)
                extra = None
                if drive is not None:
                    extra = drive(stepper)
                else:
                    for i in range(tabs["rows"]):
                        stepper.step(i)
                        self.nfe += 1
                if cond and paste_known:
                    stepper.paste_known()
                out = stepper.current()
            except BaseException:
                stepper.close()
                raise
            self._stepper = (key, stepper)
            return out if drive is None else (out, extra)

    # ------------------------------------------------------------------ graph-replayed single-step loop
    def _single_check(self, steps, order, method, solver_type):
        who = "sample_graph_singlestep"
        if method not in ("singlestep", "singlestep_fixed"):
            raise H.MMDError(f"{who}: method must be 'singlestep' or 'singlestep_fixed', got {method!r}: the multistep method has sample_graph, "
                             "the adaptive solver sample_graph_adaptive")
        if order not in (1, 2, 3):
            raise H.MMDError(f"{who}: order must be 1, 2 or 3; got {order}")
        if solver_type not in ("dpm_solver", "taylor"):
            raise H.MMDError(f"{who}: solver_type must be 'dpm_solver' or 'taylor', got {solver_type!r}")
        if solver_type == "taylor" and order == 3:
            raise H.MMDError(f"{who}: third-order 'taylor' update: the reference subtracts stream dicts (dpm:761-764) / reads an undefined "
                             "name (dpm:873) and raises")
        steps = int(steps)
        if steps < 1:
            raise H.MMDError(f"{who}: steps ({steps}) must be at least 1")
        if method == "singlestep_fixed" and steps < order:
            raise H.MMDError(f"{who}: 'singlestep_fixed' takes steps // order steps: steps ({steps}) must be at least the order ({order})")
        return steps

    def singlestep_tables(self, steps, order=3, skip_type="logSNR", method="singlestep", solver_type="dpm_solver", denoise=False, device="cpu"):
        """The per-evaluation tables of sample_graph_singlestep, graph_tables' dictionary: one row per network evaluation in the eager
        loop's order, from the helpers the eager updates call on the same host grid.  A step of order p from timesteps[i] to
        timesteps[i + p] gives p rows - an open row at s, then stage rows at s1 = inverse_lambda(lam_s + r1 h) and (order 3) s2 - whose
        c0, c1, c2 are what the eager update hands to mmd_lincomb for the state it evaluates the model on next; with denoise one more
        row at t_0.  Kinds: ops.DPM1_KIND_*; "timesteps" are the evaluation times."""
        import numpy as np
        steps = self._single_check(steps, order, method, solver_type)
        key = (steps, order, skip_type, method, solver_type, bool(denoise), str(device), bool(self.predict_x0))
        cache = self.__dict__.setdefault("_single_tables", {})
        if key not in cache:
            cache[key] = self._build_single_tables(np, steps, order, skip_type, method, solver_type, denoise, device)
        return cache[key]

    def _build_single_tables(self, np, steps, order, skip_type, method, solver_type, denoise, device):
        t_0, t_T = 1. / self.noise_schedule.total_N, self.noise_schedule.T
        orders, grid = self._single_grid(steps, order, skip_type, method, t_T, t_0)
        OPEN, STAGE, same = ops.DPM1_KIND_OPEN, ops.DPM1_KIND_STAGE, self._same
        evals = []          # (time [1], {stream: (c0, c1, c2, kind)})
        i = 0
        for p in orders:
            s, t = grid[i:i + 1], grid[i + p:i + p + 1]
            r1, r2 = self._single_ratios(grid, i, p)
            if p == 1:      # per stream: the noise-prediction form moves the audio stream with other coefficients (_first_coefs)
                evals.append((s, {k: v + (0.0, OPEN) for k, v in self._first_coefs(s, t).items()}))
            elif p == 2:
                s1, first, last = self._single_second_coefs(s, t, r1, solver_type)
                evals += [(s, same(first + (0.0, OPEN))), (s1, same(last + (STAGE,)))]
            else:
                s1, s2, first, mid, last = self._single_third_coefs(s, t, r1, r2, solver_type)
                evals += [(s, same(first + (0.0, OPEN))), (s1, same(mid + (STAGE,))), (s2, same(last + (STAGE,)))]
            i += p
        return self._eval_tables(np, evals, denoise, device)

    def sample_graph_singlestep(self, x_T=None, *, shape=None, steps, order=3, skip_type="logSNR", method="singlestep", solver_type="dpm_solver",
                                denoise=False, known=None, mask=None, noise_source=None, paste_known=True, use_graph=True, lanes=None):
        """sample(method="singlestep" / "singlestep_fixed") of orders 1-3 as one graph replay per lane and network evaluation
        (sampler.DpmSingleStepper, the tables of singlestep_tables): the same x_T and window-shift stream - one draw per evaluation, in
        the eager order - give the same bits.  x_T / shape, noise_source, known / mask / paste_known, use_graph and lanes as in
        sample_graph; the known cells are set before EVERY evaluation, the stage evaluations at s1 and s2 included, to
        alpha(tau) known + sigma(tau) eps at that evaluation's time tau.  Batch 1 is accepted."""
        from .sampler import DpmSingleStepper
        return self._graph_loop("sample_graph_singlestep", DpmSingleStepper, lambda: self._single_check(steps, order, method, solver_type),
                                lambda device: self.singlestep_tables(steps, order, skip_type, method, solver_type, denoise, device=device),
                                x_T, shape, known, mask, noise_source, paste_known, use_graph, lanes)

    # ------------------------------------------------------------------ graph-replayed adaptive loop: the controller on the device
    def _adaptive_check(self, order, solver_type, control, lanes, poll, max_attempts):
        who = "sample_graph_adaptive"
        if self.KEYS != ("video", "audio"):
            raise H.MMDError(f"{who}: built for the multimodal base model's {{'video', 'audio'}} state only, not for the SR stage's tensor solver")
        if not self.predict_x0:
            raise H.MMDError(f"{who}: predict_x0=False is not built: the reference's noise-prediction first update moves the audio stream with "
                             "x0-form coefficients (dpm:576-584) - use sample(method='adaptive')")
        if order != 2:
            raise H.MMDError(f"{who}: order must be 2 (the embedded pair of orders 1 and 2), got order {order}")
        if solver_type != "dpm_solver":
            raise H.MMDError(f"{who}: solver_type must be 'dpm_solver', got solver_type {solver_type!r}")
        if control not in ("sample", "batch"):
            raise H.MMDError(f"{who}: control must be 'sample' or 'batch', got control {control!r}")
        if control == "batch" and lanes is not None and int(lanes) != 1:
            raise H.MMDError(f"{who}: control='batch' takes the maximum over the whole batch, which must sit in one lane: lanes must be 1, got lanes {lanes}")
        if int(poll) < 1:
            raise H.MMDError(f"{who}: poll must be at least 1 trial step between two status reads, got poll {poll}")
        if int(max_attempts) < 1:
            raise H.MMDError(f"{who}: max_attempts must be at least 1, got max_attempts {max_attempts}")

    def adaptive_tables(self, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, t_start=None, t_end=None):
        """What the device controller of sample_graph_adaptive reads: {"params": the parameter block's values, "log_alpha": the discrete
        schedule's knots as float64 (log alpha at t_i = (i + 1) / N - the table the eager solver interpolates in its own dtype)}."""
        ns = self.noise_schedule
        t_0 = 1. / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
        return {"params": dict(atol=atol, rtol=rtol, theta=theta, t_err=t_err, h_init=h_init, t_T=t_T, t_0=t_0),
                "log_alpha": ns.log_alpha_array.reshape(-1).double().cpu().numpy()}

    def sample_graph_adaptive(self, x_T=None, *, shape=None, order=2, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5,
                              control="sample", poll=4, max_attempts=1000, known=None, mask=None, noise_source=None, paste_known=True,
                              use_graph=True, lanes=None, return_stats=False, solver_type="dpm_solver"):
        """sample(method="adaptive") of order 2 in its data-prediction form with the step-size controller on the device
        (sampler.DpmAdaptiveStepper; include/mmd.h: mmd_dpm_adapt_*): a trial step is two graph replays per lane, and the error norm, the
        accept test, the next step size, the next times and every coefficient derived from them stay in device memory.  The host replays
        `poll` trial steps, then reads one status word per lane (samples not done, fault bit); a trial step replayed after a sample is
        done is an exact no-op for it, so samples and statistics are bitwise the same for every poll.  A model with a host shift_source
        draws the shifts of up to poll - 1 trial steps (2 (poll - 1) evaluations) more than the loop needed.
        control="sample": every sample has its own s, h, error and decision - sample k of a seed is the same at any batch and lane count;
        control="batch": the reference's rule, E = the maximum over all samples and streams and one s, h for the batch (one lane), the form
        to hold against sample(method="adaptive"), whose coefficients are fp32 where the controller's are fp64 rounded once.
        More than max_attempts trial steps, or a non-finite error sum (the fault bit; that sample's state is left as it was), raise MMDError
        at the poll that sees them.  x_T / shape, known / mask / paste_known, noise_source, use_graph and lanes as in sample_graph; the
        known cells are set before both evaluations at the levels of s and s1.  return_stats: also {"attempts", "accepted", "nfe"} per
        sample and "trials", "host_reads" of the call.  self.nfe grows by 2 x the trial steps replayed.  The tolerances live in a device
        parameter block: another call with other values replays the kept stepper's graph execs."""
        from .sampler import DpmAdaptiveStepper
        who = "sample_graph_adaptive"
        self._adaptive_check(order, solver_type, control, lanes, poll, max_attempts)      # first: the SR stage's solver gets no further
        if control == "batch" and lanes is None:
            lanes = 1

        def drive(stepper):
            stepper.start()
            while True:
                for _ in range(min(int(poll), int(max_attempts) - stepper.trials)):
                    stepper.trial()
                    self.nfe += 2
                active, fault = stepper.poll()
                if fault:
                    raise H.MMDError(f"{who}: a non-finite error sum after {stepper.trials} trial steps (the sample's state was left as it was)")
                if not active:
                    break
                if stepper.trials >= int(max_attempts):
                    raise H.MMDError(f"{who}: {active} sample(s) not done after max_attempts = {stepper.trials} trial steps")
            return dict(stepper.stats(), trials=stepper.trials, host_reads=stepper.host_reads)
        out, stats = self._graph_loop(who, DpmAdaptiveStepper, lambda: None, lambda device: self.adaptive_tables(h_init, atol, rtol, theta, t_err), x_T, shape, known, mask, noise_source,
                                      paste_known, use_graph, lanes, drive=drive, stepper_kw=dict(control=control))
        return (out, stats) if return_stats else out


def expand_dims(v, dims):
    """[N] -> [N, 1, ..., 1] with `dims` dimensions (dpm:1349-1358)."""
    return v[(...,) + (None,) * (dims - 1)]
