"""Graph-replayed denoising step: [U-Net launch plan + fused DDPM update of both streams] captured once into a
hipGraph (mmd_graph_*), replayed per step.  Between replays only three small device buffers change: the
timestep (loop index + model timestep), the window shifts and the noise.  update="vlb" replays one step of the
variational bound instead (calc_bpd_loop): [q_sample of both streams from static x_0 buffers + U-Net plan + mmd_vlb_terms of
both streams], whose per-sample results land in device tables at the step's column.  update="ddim_reverse" replays one step of DDIM
inversion (ddim_encode_loop): [U-Net plan + mmd_ddim_update with flag 8 of both streams], which draws nothing.

Replaces the per-step host work of the reference loop (gd:561-582 + resp:134-139): th.tensor([i]*B) H2D,
the timestep_map tensor rebuild, ~16 table uploads and ~55k ATen dispatches.

Structure: LaneStepper owns what every replayed step shares - the batch lanes and their engines, the conditioning buffers and the
pre-plan that replaces the known cells, the per-step uploads, the lane events, and capture / launch / close over NAMED PLAN SETS
(name -> per-lane plans behind the U-Net plan, and their per-lane graph execs once captured).  GraphStepper (DDPM / DDIM / variational
bound) and SolverStepper (DPM-Solver / DPM-Solver++: DpmppStepper multistep, DpmSingleStepper single-step, DpmppSdeStepper stochastic multistep) record their update plans into
sets and say, in set_step, which set the next launch replays.  A set may be `bare`: launched without the pre-plan and the U-Net plan (the
forward jump of masked sampling with resampling, GraphStepper.jump).  DpmAdaptiveStepper (the adaptive DPM-Solver++ with its step-size
controller on the device) has two sets per trial step, each with a pre-plan of its own, and no table rows: the controller writes them."""
import ctypes
import os

import torch as th

from . import _hip as H
from . import ops


def unwrap_unet(model):
    """Return the MultimodalUNet behind `model` (possibly wrapped by _WrappedModel / DDP), else None."""
    from .multimodal_unet import MultimodalUNet
    seen = 0
    while model is not None and seen < 4:
        if isinstance(model, MultimodalUNet):
            return model
        model = getattr(model, "model", None) or getattr(model, "module", None)
        seen += 1
    return None


def default_lanes(batch):
    """Batch lanes of a sampling step (see GraphStepper).  MMD_LANES overrides.  Round 6: TWO lanes for batches of 4 and more (each
    lane at least two samples).  Measured on MI355X at batch 4 (BASELINE configs[1]), same-call A/B on three boxes: 11.28 -> 11.09,
    10.85 -> 10.77, 10.87 -> 10.79 ms per step with two lanes (profiles/r06_suite_and_lanes_call9.txt, r06_wgrad_strip_lanes_call10.txt,
    r06_lanes_width_aconv_call11.txt); four lanes 15.0 ms (batch-1 launches fill a fraction of the chip and the 2 600 launches of a step
    queue).  Round 2 had measured 15.53 / 15.37 / 20.5 ms for 1 / 2 / 4 lanes and kept one: the per-level kernels have become short
    enough since that a second half-batch chain finds idle CUs beside the first one's latency-bound small levels.  The lanes are
    independent engines: the trajectory does not depend on the lane count (bitwise, tests/test_lifetime_gpu.py)."""
    v = os.environ.get("MMD_LANES")
    lanes = int(v) if v else (2 if batch >= 4 and batch % 2 == 0 else 1)
    return lanes if lanes >= 1 and batch % lanes == 0 else 1


STREAMS = (("video", 0), ("audio", 1))      # stream key, and its plan stream id = its counter tag


class _PlanSet:
    """One named plan set: the per-lane plans that follow the U-Net plan, and their per-lane graph execs (None before capture).  A
    `bare` set is launched on its own, without the pre-plan and the U-Net plan in front of it."""

    def __init__(self, plans, bare=False):
        self.plans, self.graphs, self.bare = plans, None, bare


def _replay(ps, r, stream):
    H.call("mmd_graph_launch", ps.graphs[r], stream)


class LaneStepper:
    """What a replayed step of `batch` trajectories is made of, whatever its update: lanes, conditioning, uploads, capture and launch.

    lanes > 1 splits the batch into independent sub-batches, each with its own engine (activation buffers, video + audio launch
    streams; packed weights are shared) and its own captured graph; the lane graphs are launched on the lanes' private streams,
    forked from and joined to the caller's stream with events.  Every sample's trajectory is independent (GroupNorm / attention
    never mix batch elements, tests: batch sharding is bitwise exact), so the result is identical.  Timestep, sample-id and noise
    buffers stay full-batch (lanes read slices), so the RNG stream does not depend on `lanes`.  Default: see default_lanes.

    A lane's launch is [pre-plan] + U-Net plan + the plans of the current set (self._set); subclasses record plans with _add_set."""

    def __init__(self, unet, batch, device, lanes, use_graph, use_f32=False, ctr=None, own_ids=False):
        self.unet, self.N, self.device = unet, int(batch), th.device(device)
        self.lanes = default_lanes(self.N) if lanes is None else int(lanes)
        if self.lanes < 1 or self.N % self.lanes:
            raise H.MMDError(f"batch {self.N} does not split into {self.lanes} lanes")
        self.n = self.N // self.lanes
        self.engs = [unet.engine(self.n, self.device, replica=r) for r in range(self.lanes)]
        self.eng = self.engs[0]
        self.t_idx = th.zeros(self.N, dtype=th.int64, device=self.device)      # loop index / step number (table row)
        self.ctr = ctr
        if ctr is not None:      # own_ids: copies that a later source can be loaded into (DpmppStepper.retable)
            self.key, self.ids = ctr.key(self.device), ctr.ids(self.N, self.device)
            if own_ids:
                self.key, self.ids = self.key.clone(), self.ids.clone()
        self.use_graph, self.use_f32 = use_graph, use_f32
        self.cond, self.pre_plans = {}, []
        self._sets, self._set = {}, "step"
        # per-step scalars go up through pinned rings (H.Staged): the host runs ahead of the GPU, one reused pinned buffer would race
        self._up_t = H.Staged(self.t_idx)
        self._up_tm = [H.Staged(e.t_f32 if use_f32 else e.t_i64) for e in self.engs]
        # lane fork / join events (lane 0 rides the origin stream, lane r > 0 its engine's private `side` stream)
        self._lane_ev = []
        for _ in range(self.lanes + 1 if self.lanes > 1 else 0):
            ev = ctypes.c_void_p()
            H.call("mmd_event_create", ctypes.byref(ev))
            self._lane_ev.append(ev)

    def _lane(self, r):
        return slice(r * self.n, (r + 1) * self.n)

    def _add_set(self, name, plans, bare=False):
        self._sets[name] = _PlanSet(plans, bare)
        return plans

    @property
    def graphs(self):
        """The step set's per-lane graph execs, None before capture."""
        return self._sets["step"].graphs

    # ------------------------------------------------------------------ masked conditioning
    def _record_cond(self, cond, qtab):
        """cond (masking.normalize's result): per conditioned stream the static known values, one uint8 mask row per sample (none: the
        whole stream) and, without a counter source, the fixed conditioning noise (= that stream's x_T); load_cond fills them.  Every
        lane's pre-plan then starts the step with one mmd_cond_replace per conditioned stream, which sets the known cells of the state
        to q_sample(known, t, noise) by the [2, T] table qtab and leaves the others alone.  cond=None records nothing."""
        self._alloc_cond(cond)
        for r in range(self.lanes if self.cond else 0):
            pre = []
            with ops.recording(pre):       # on the origin stream: the known cells at this step's noise level
                for k, tag in STREAMS:
                    if k in self.cond:
                        self._cond_replace(r, k, tag, qtab, self.t_idx[self._lane(r)], None)
            self.pre_plans.append(pre)

    def _alloc_cond(self, cond):
        """The conditioning buffers of _record_cond, without a recorded pre-plan (a stepper whose levels are not indexed by t_idx records
        its own mmd_cond_replace launches with _cond_replace)."""
        e = self.eng
        for k, c in (cond or {}).items():
            xk = e.x_video if k == "video" else e.x_audio
            like = dict(size=(self.N,) + tuple(xk.shape[1:]), dtype=th.float32, device=self.device)
            cells = e.F * e.H0 * e.W0 if k == "video" else e.L0
            self.cond[k] = {"known": th.zeros(**like),
                            "mask": None if c.mask is None else th.zeros(self.N, cells, dtype=th.uint8, device=self.device),
                            "noise": None if self.ctr is not None else th.zeros(**like)}

    def _cond_replace(self, r, k, tag, tab2, t, coef):
        """ops.cond_replace of stream k on lane r's state and its slices of the conditioning buffers; coef = (ca, cb) draws no noise."""
        e, sl = self.engs[r], self._lane(r)
        b = self.cond[k]
        src = {}
        if coef is None:
            src = dict(ctr=(self.key, self.ids[sl], tag)) if self.ctr is not None else dict(noise=b["noise"][sl])
        ops.cond_replace(e.x_video if k == "video" else e.x_audio, b["known"][sl], tab2, t, mask=None if b["mask"] is None else b["mask"][sl],
                         coef=coef, **src)

    def load_cond(self, cond, noise=None):
        """Fill the conditioning buffers from masking.normalize's result (the streams and the presence of masks as at construction);
        noise: {stream: x_T}, the fixed conditioning noise - needed unless the kernels draw it from the counter."""
        if set(cond) != set(self.cond) or any((cond[k].mask is None) != (self.cond[k]["mask"] is None) for k in cond):
            raise H.MMDError("load_cond: the conditioned streams and their masks' presence are fixed when the stepper is built")
        for k, c in cond.items():
            b = self.cond[k]
            b["known"].copy_(c.known)
            if c.mask is not None:      # one row per sample: a lane reads its slice whether the caller's mask was shared or not
                b["mask"].copy_(c.mask.reshape(-1, b["mask"].shape[1]).expand_as(b["mask"]))
            if b["noise"] is not None:
                if noise is None or k not in noise:
                    raise H.MMDError(f"load_cond: the fixed conditioning noise of {k!r} is missing")
                b["noise"].copy_(noise[k])

    def paste_known(self):
        """The current state's known cells = the known values, bit for bit (after the last step)."""
        for r in range(self.lanes):
            for k, tag in STREAMS:
                if k in self.cond:
                    self._cond_replace(r, k, tag, None, None, (1.0, 0.0))

    # ------------------------------------------------------------------ state
    def load(self, video, audio):
        for r, e in enumerate(self.engs):
            e.x_video.copy_(video[self._lane(r)])
            e.x_audio.copy_(audio[self._lane(r)])

    def set_x(self, key, value):
        """Overwrite one stream of the current state (replacement-method conditional sampling)."""
        for r, e in enumerate(self.engs):
            (e.x_video if key == "video" else e.x_audio).copy_(value[self._lane(r)])

    def current(self):
        if self.lanes == 1:
            return {"video": self.eng.x_video.clone(), "audio": self.eng.x_audio.clone()}
        return {"video": th.cat([e.x_video for e in self.engs]), "audio": th.cat([e.x_audio for e in self.engs])}

    # ------------------------------------------------------------------ per-step uploads
    def _push_step(self, i, tm, shifts):
        """Loop index i and model timestep tm into their device buffers, and the window shifts: one draw per block for the whole batch
        (unet:619-620), from the counter with a CounterNoise (a model with a shift_source of its own keeps it)."""
        self._up_t.host().fill_(i)
        self._up_t.push()
        for up in self._up_tm:
            up.host().fill_(tm)
            up.push()
        if shifts is None:
            own = self.ctr is not None and self.unet.shift_source is None
            shifts = self.ctr.shifts(i, self.unet) if own else self.unet.draw_shifts()
        for e in self.engs:
            e.set_shifts(shifts)

    # ------------------------------------------------------------------ capture and launch
    def _lane_launch(self, ps, r, stream):
        """Enqueue lane r's pre-plan, U-Net plan and its plan of set `ps` with `stream` as its video-chain stream (its engine's aux =
        audio chain)."""
        e = self.engs[r]
        aux = e.aux.cuda_stream
        if not ps.bare:
            if self.pre_plans:
                ops.run_plan(self.pre_plans[r], stream, aux)
            ops.run_plan(e.plan_f32 if self.use_f32 else e.plan, stream, aux)
        ops.run_plan(ps.plans[r], stream, aux)

    def _capture(self, ps):
        """One graph PER LANE, each captured with the lane's own private stream as the capture origin and its engine's aux stream
        as the only forked stream.  (All lanes in one capture would need two non-origin streams - a lane's video and audio chains
        - that wait on each other at every cross-attention; the HIP runtime re-parents the waiting stream on each such wait, the
        two become each other's parent and hipStreamEndCapture recurses until the stack overflows: the SIGSEGV of
        tools/lanes_probe.py.  Streams keep ONE role for life here: an engine's `side` is only ever an origin, its `aux` only ever
        the origin's child.)"""
        cur = th.cuda.current_stream(self.device)
        for r, e in enumerate(self.engs):
            e.side.wait_stream(cur)
            self._lane_launch(ps, r, e.side.cuda_stream)        # warm-up: one-time function attributes, lazy module load
        th.cuda.synchronize(self.device)
        graphs = []
        for r, e in enumerate(self.engs):
            with H.capture(e.side.cuda_stream) as cap:
                self._lane_launch(ps, r, e.side.cuda_stream)
            graphs.append(cap.exec)
        ps.graphs = graphs

    def _fan(self, body, ps):
        """Run body(ps, r, stream) for every lane: lane streams fork from the current stream and join it again (plain events)."""
        cur = H.stream_handle()
        if self.lanes == 1:
            body(ps, 0, cur)
            return
        lib = H.lib()
        lib.mmd_event_record(self._lane_ev[0], cur)
        for r, e in enumerate(self.engs):
            ls = e.side.cuda_stream
            lib.mmd_stream_wait_event(ls, self._lane_ev[0])
            body(ps, r, ls)
            lib.mmd_event_record(self._lane_ev[r + 1], ls)
        for r in range(self.lanes):
            if lib.mmd_stream_wait_event(cur, self._lane_ev[r + 1]):
                raise H.MMDError(f"lane join failed: {lib.mmd_last_error().decode()}")

    def launch(self):
        """Replay the current set (set_step chose it); a set is warmed up and captured the first time it is launched."""
        ps = self._sets[self._set]
        if self.use_graph:
            if ps.graphs is None:
                # capture replays the step once as warm-up: keep x intact around it
                keep = [(e.x_video.clone(), e.x_audio.clone()) for e in self.engs]
                self._capture(ps)
                for e, (xv, xa) in zip(self.engs, keep):
                    e.x_video.copy_(xv)
                    e.x_audio.copy_(xa)
            self._fan(_replay, ps)
        else:
            if self.lanes == 1:
                self.eng.aux.wait_stream(th.cuda.current_stream(self.device))
            self._fan(self._lane_launch, ps)

    def step(self, i, shifts=None, noise=None):
        self.set_step(i, shifts, noise)
        self.launch()

    def close(self):
        """Retire every set's graph execs and its plans' join events, and the lane events (destroyed by H.reap() at the next safe
        point, never here: this also runs as a finaliser from the cyclic GC, possibly on a half-built stepper)."""
        try:
            for ps in getattr(self, "_sets", {}).values():
                for g in ps.graphs or []:
                    H.retire("graph", g)
                for ev in H.plan_events(*ps.plans):
                    H.retire("event", ev)
                ps.graphs = None
                del ps.plans[:]
            for ev in getattr(self, "_lane_ev", []):
                H.retire("event", ev)
            self.update_plan, self._lane_ev = [], []
        except Exception:
            pass

    __del__ = close


class GraphStepper(LaneStepper):
    """One denoising step of `batch` trajectories as one graph replay per lane (LaneStepper): update "ddpm" / "ddim", one step of the
    variational bound ("vlb"), or one step of the DDIM reverse ODE ("ddim_reverse": level i -> level i + 1, mmd_ddim_update with flag 8).

    The reverse step draws nothing, so it owns no noise buffers and has no counter form; with a seeded.CounterNoise on the diffusion its
    set_step(i) still takes the window shifts from ctr.shifts(i, unet) - the draw decode step i uses, and both evaluate the model at the
    level-i state.  It takes neither cond nor jump_length.

    With a seeded.CounterNoise as the diffusion's noise_source (update "ddpm" / "ddim") the step owns no noise buffers: the graph records
    mmd_ddpm_update_ctr / mmd_ddim_update_ctr, which draw the noise of (seed, sample id, loop index, stream, element) in the kernel - a
    lane reads its slice of the sample ids as it reads its slice of the timesteps - and set_step takes the window shifts from the counter.

    cond (masking.normalize's result; update "ddpm" / "ddim") conditions the step on known cells: every lane's graph starts with one
    mmd_cond_replace per conditioned stream, with noise = that stream's x_T (masked_sample_loop).  cond=None records nothing.

    jump_length (update "ddpm") equips the stepper for masked sampling with resampling jumps (masking.repaint_schedule), where a step
    runs more than once: a full-batch device `draw` buffer sits next to t_idx and is pushed with it; with a counter source the step set
    records mmd_ddpm_update_ctr_at, which draws at draw[n] instead of t[n], and the window shifts come from ctr.shifts(draw); and a
    second, bare plan set "jump" - no pre-plan, no U-Net plan - holds the forward jump of t_idx[n] = m over jump_length levels: per
    stream on its own stream one mmd_renoise_ctr at draw[n], or without a counter source one mmd_q_sample on the stream's noise buffer
    (jump() refills it: video first, then audio), then the join.  jump_length=None records none of this."""

    def __init__(self, diffusion, unet, batch, device, clip_denoised=True, use_graph=True, update="ddpm", eta=0.0, lanes=None, cond=None,
                 jump_length=None):
        if update not in ("ddpm", "ddim", "ddim_reverse", "vlb"):
            raise H.MMDError(f"unknown update {update!r} (ddpm, ddim, ddim_reverse or vlb)")
        if update == "ddim_reverse" and jump_length is not None:
            raise H.MMDError("jump_length: resampling jumps ride the ddpm update; the ddim_reverse update (DDIM inversion) takes none")
        if update == "ddim_reverse" and cond:
            raise H.MMDError("cond: masked conditioning rides the sampling steps (ddpm, ddim), not the ddim_reverse update (DDIM inversion)")
        if jump_length is not None and update != "ddpm":
            raise H.MMDError(f"resampling jumps ride the ddpm update, not {update!r}")
        if cond and update == "vlb":
            raise H.MMDError("masked conditioning rides the sampling steps (ddpm, ddim), not the variational bound")
        from .seeded import counter_source
        ctr = counter_source(diffusion) if update != "vlb" else None
        self.rescale = bool(diffusion.rescale_timesteps)
        super().__init__(unet, batch, device, lanes, use_graph, use_f32=self.rescale, ctr=ctr)
        self.diff, self.update, self.eta = diffusion, update, eta
        self.tab, qtab = diffusion.device_tables(self.device)
        self.flags = diffusion._flags(clip_denoised)
        e, n = self.eng, self.n
        self.noise_v = self.noise_a = None
        if ctr is None and update != "ddim_reverse":      # the reverse ODE step draws nothing
            self.noise_v = th.zeros((self.N,) + tuple(e.x_video.shape[1:]), dtype=th.float32, device=self.device)
            self.noise_a = th.zeros((self.N,) + tuple(e.x_audio.shape[1:]), dtype=th.float32, device=self.device)
        self._noise = {"video": self.noise_v, "audio": self.noise_a}
        # model timestep: SpacedDiffusion maps the loop index to the original step (resp:134-139)
        tmap = getattr(diffusion, "timestep_map", None)
        self.tmap = list(tmap) if tmap is not None else list(range(diffusion.num_timesteps))
        self.orig_T = getattr(diffusion, "original_num_steps", diffusion.num_timesteps)
        self._record_cond(cond, qtab)
        self.draw = self._up_d = self.jtab = None
        if jump_length is not None:
            self.draw = th.zeros(self.N, dtype=th.int64, device=self.device)      # the counter's draw word of the step or the jump
            self._up_d = H.Staged(self.draw)
            self.jtab = diffusion.jump_tables(jump_length, self.device)
            self.jump_levels = self.jtab.shape[1] - int(jump_length)               # levels m with m + jump_length <= T - 1
        if update == "vlb":
            # static x_0, and per stream the (vb, xstart_mse, eps_mse) result tables [N, T] the reductions write at column t
            T = self.tab.shape[1]
            self.x0_v, self.x0_a = th.zeros_like(self.noise_v), th.zeros_like(self.noise_a)
            self._x0 = {"video": self.x0_v, "audio": self.x0_a}
            self.res = {k: tuple(th.zeros(self.N, T, dtype=th.float32, device=self.device) for _ in range(3)) for k in ("video", "audio")}
            self._ws = [(ops.vlb_workspace(n, self.device), ops.vlb_workspace(n, self.device)) for _ in self.engs]
        elif update in ("ddim", "ddim_reverse"):       # ddim_sample (gd:821-901) / ddim_reverse_sample (gd:903-953): same graph, different fused update
            self._tab3 = diffusion.ddim_tables(self.device)
        plans = self.update_plans = self._add_set("step", [])
        self.jump_plans = self._add_set("jump", [], bare=True) if self.jtab is not None else []
        for r, e in enumerate(self.engs):
            sl = self._lane(r)
            # per stream: (stream id, key, state, model output, (F, C, HW), counter tag)
            rows = ((0, "video", e.x_video, e.out_video, (e.F, e.Cv_in, e.H0 * e.W0), 0),
                    (1, "audio", e.x_audio, e.out_audio, (1, e.Ca_in, e.L0), 1))
            if update == "vlb":
                pre = []
                with ops.recording(pre):       # both on the origin stream: the U-Net plan forks its audio stream behind them
                    for _, k, xk, *_ in rows:
                        ops.q_sample(self._x0[k][sl], self._noise[k][sl], xk, qtab, self.t_idx[sl])
                self.pre_plans.append(pre)
            plan = []
            with ops.recording(plan):
                # in place: x_{t-1} overwrites x_t (purely elementwise); each update rides its own stream, then join
                for row in rows:
                    with ops.on_stream(row[0]):
                        self._record_update(r, *row[1:])
                ops.record_sync(1, 0)
            plans.append(plan)
            if self.jtab is not None:
                jump = []
                with ops.recording(jump):      # the audio stream forks from the origin here: no U-Net plan in front has done it
                    ops.record_sync(0, 1)
                    for sid, k, xk, _, _, tag in rows:
                        with ops.on_stream(sid):
                            if ctr is not None:
                                ops.renoise_ctr(xk, self.key, self.ids[sl], tag, self.jtab, self.t_idx[sl], self.draw[sl])
                            else:
                                ops.q_sample(xk, self._noise[k][sl], xk, self.jtab, self.t_idx[sl])
                    ops.record_sync(1, 0)
                self.jump_plans.append(jump)
        self.update_plan = plans[0]

    def _record_update(self, r, k, x, out, geom, tag):
        """Record lane r's update of one stream.  The noise source of the lane: (key, its sample ids, the stream's tag) for the kernels
        that draw by counter, else (its slice of the stream's noise buffer,)."""
        sl = self._lane(r)
        t_idx, (F, C, HW) = self.t_idx[sl], geom
        if self.update == "ddim_reverse":      # flag 8: x_t -> x_{t+1} by alphas_cumprod_next; no noise source in either form
            ops.ddim_update(x, out, None, x, self.tab, self._tab3, t_idx, F, C, HW, self.flags | 8, 0.0)
            return
        src = (self.key, self.ids[sl], tag) if self.ctr is not None else (self._noise[k][sl],)
        if self.update == "vlb":
            vb, xs, em = (a[sl] for a in self.res[k])
            ops.vlb_terms(self._x0[k][sl], x, out, self.tab, t_idx, F, C, HW, self.flags, vb, xstart_mse=xs, eps_mse=em, noise=src[0],
                          ws=self._ws[r][tag])
        elif self.update == "ddim":
            fn = ops.ddim_update_ctr if self.ctr is not None else ops.ddim_update
            fn(x, out, *src, x, self.tab, self._tab3, t_idx, F, C, HW, self.flags, self.eta)
        else:
            if self.ctr is not None and self.draw is not None:
                ops.ddpm_update_ctr_at(x, out, *src, x, self.tab, t_idx, self.draw[sl], F, C, HW, self.flags)
                return
            fn = ops.ddpm_update_ctr if self.ctr is not None else ops.ddpm_update
            fn(x, out, *src, x, self.tab, t_idx, F, C, HW, self.flags)

    def load_x0(self, video, audio):
        """update="vlb": the clean clips every step noises afresh."""
        self.x0_v.copy_(video)
        self.x0_a.copy_(audio)

    def results(self):
        """update="vlb": {"video" / "audio": (vb, xstart_mse, eps_mse)} [N, T] tables, column = loop index t."""
        return self.res

    def _push_draw(self, draw):
        self._up_d.host().fill_(int(draw))
        self._up_d.push()

    def _fresh_noise(self):
        """Both noise buffers from the diffusion's source: video first, then audio."""
        if self.diff.noise_source is not None:
            self.noise_v.copy_(self.diff.noise_source(self.noise_v))
            self.noise_a.copy_(self.diff.noise_source(self.noise_a))
        else:
            self.noise_v.normal_()
            self.noise_a.normal_()

    def jump(self, m, draw, noise=None):
        """The forward jump from level m (jump_length levels up) at `draw`: refresh t_idx, the draw and - without a counter source - the
        noise (`noise` = {"video", "audio"}, else drawn video first, then audio), and replay the jump set."""
        if self.jtab is None:
            raise H.MMDError("this stepper was built without jump_length: it has no jump set")
        m = int(m)
        if not 0 <= m < self.jump_levels:
            raise H.MMDError(f"jump: level {m} is outside [0, {self.jump_levels}): the jump would end above the last level")
        self._set = "jump"
        self._up_t.host().fill_(m)
        self._up_t.push()
        self._push_draw(draw)
        if self.ctr is not None:
            if noise is not None:
                raise H.MMDError("this jump draws its noise in the kernel (CounterNoise): it takes no noise tensors")
        elif noise is not None:
            self.noise_v.copy_(noise["video"])
            self.noise_a.copy_(noise["audio"])
        else:
            self._fresh_noise()
        self.launch()

    def step(self, i, shifts=None, noise=None, draw=None):
        self.set_step(i, shifts, noise, draw)
        self.launch()

    def set_step(self, i, shifts=None, noise=None, draw=None):
        """Refresh the per-step device state: timestep, shifts, noise (video first, then audio - gd:453-454).  draw (a stepper with
        jump_length only; default i): the counter's draw word of this visit of step i, for the noise and the window shifts."""
        tm = self.tmap[int(i)]
        self._set = "step"
        if self.draw is not None:
            draw = int(i) if draw is None else int(draw)
            self._push_draw(draw)
            if shifts is None and self.ctr is not None and self.unet.shift_source is None:
                shifts = self.ctr.shifts(draw, self.unet)
        elif draw is not None and int(draw) != int(i):
            raise H.MMDError("a draw other than the step's index needs a stepper built with jump_length")
        self._push_step(int(i), float(tm) * (1000.0 / self.orig_T) if self.use_f32 else int(tm), shifts)
        if self.update == "ddim_reverse":
            if noise is not None:
                raise H.MMDError("the ddim_reverse step draws nothing: it takes no noise tensors")
            return
        if self.ctr is not None:
            if noise is not None:
                raise H.MMDError("this step draws its noise in the update kernels (CounterNoise): it takes no noise tensors")
        elif noise is not None:
            self.noise_v.copy_(noise["video"])
            self.noise_a.copy_(noise["audio"])
        else:
            if hasattr(self.diff.noise_source, "set_draw"):      # update="vlb" keeps its noise in memory: the callable form at this index
                self.diff.noise_source.set_draw(int(i))
            self._fresh_noise()


# Which kernel a recorded DPM-Solver++ step takes its thresholding quantile from: "multi" = the three-level multi-workgroup selection
# whose first level rides mmd_dpmpp_x0, "block" = mmd_abs_quantile (one workgroup per sample).  The two return the same bits; the choice
# is a timing one (tools/dpm_graph_bench.py).
DPMPP_SELECT = "multi"


class SolverLanes(LaneStepper):
    """What the replayed DPM-Solver steppers share besides the lanes: geometry, the model-value recorder, the counter source's refresh."""

    def __init__(self, unet, batch, device, lanes, use_graph, ctr, select):
        self.select = DPMPP_SELECT if select is None else select
        if self.select not in ("multi", "block"):
            raise H.MMDError(f"unknown selection {select!r} (multi or block)")
        super().__init__(unet, batch, device, lanes, use_graph, ctr=ctr, own_ids=True)      # own ids: retable() refills them
        self.diff = None

    def _geom(self):
        e, unet = self.eng, self.unet          # {stream: (F, C, Cm, HW)}: the state is [n, F, C, HW], the model output [n, F, Cm, HW]
        return {"video": (e.F, e.Cv_in, unet.video_out_channels, e.H0 * e.W0), "audio": (1, e.Ca_in, unet.audio_out_channels, e.L0)}

    def _record_model_value(self, xk, ok, b, tab, rows, geom, data_form, thresholding, fused):
        """Record what runs before one stream's update and return (src, form, s, Cm), the update's source of the model value: the model
        output ok - form 1 where a fused update forms the data prediction itself (include/mmd.h: mmd_dpm_single_update) - or, where
        the prediction is stored (thresholding; an update that is not fused), b["x0"] of mmd_dpmpp_x0 with the selected scale b["s"]."""
        F, C, Cm, HW = geom
        if not data_form or (fused and not thresholding):
            return ok, 1 if data_form else 0, None, Cm
        multi = thresholding and self.select == "multi"
        ops.dpmpp_x0(xk, ok, b["x0"], tab, rows, F, C, Cm, HW, hist=b["ws"] if multi else None)
        if multi:
            ops.dpmpp_select(b["x0"], 0.995, b["s"], b["ws"], level0_done=True)      # p of the Imagen paper
        elif thresholding:
            ops.abs_quantile(b["x0"], 0.995, out=b["s"])
        return b["x0"], 0, b["s"] if thresholding else None, C

    def _load_ctr(self, ctr):
        if (ctr is None) != (self.ctr is None):
            raise H.MMDError("the noise source's kind is fixed when the stepper is built")
        self.ctr = ctr
        if ctr is not None:
            self.key.copy_(ctr.key(self.device))
            self.ids.copy_(ctr.ids(self.N, self.device))

    def usable(self):
        """False once the model has rebuilt its engines (new weights, another dtype): the recorded plans then point at retired buffers."""
        try:
            return all(self.unet.engine(self.n, self.device, replica=r) is e for r, e in enumerate(self.engs))
        except Exception:
            return False


class SolverStepper(SolverLanes):
    """One evaluation of a fixed-grid DPM-Solver / DPM-Solver++ loop as one graph replay per lane: [mmd_cond_replace of each conditioned
    stream] + U-Net plan + per stream on its own stream [the model value m0 + the solver's update] + join.  Every coefficient sits in
    device tables (fp32 [6, rows] per stream, include/mmd.h), indexed by the evaluation number in t_idx, so the graph of one evaluation
    serves them all.  The noise-prediction solver updates from the model output directly; its closing denoise evaluation is a data
    prediction and has a second plan set ("final"), which set_step selects at the denoise row.  Lanes, conditioning buffers, capture and
    launch are LaneStepper's.  A subclass names the solver's update: its history buffers (_history) and the launch that consumes m0
    (_update); with FUSED_X0 that launch forms an unthresholded data prediction itself and mmd_dpmpp_x0 is recorded only where the
    quantile selection has to read x0raw.

    The tables have a fixed capacity (ROWS_CAP rows, the stride the recorded launches carry), so a stepper outlives one sampling call:
    retable() loads another time grid, order or seed into the same buffers and the captured graphs are replayed as they are
    (DPM_Solver keeps its last stepper; a capture costs about as much as five evaluations of a 50-evaluation call)."""
    ROWS_CAP = 1024
    FUSED_X0 = False
    WHO = "sample_graph"

    def __init__(self, solver, unet, batch, device, tabs, use_graph=True, lanes=None, cond=None, ctr=None, select=None):
        super().__init__(unet, batch, device, lanes, use_graph, ctr, select)
        self.tab = {k: th.zeros(ops.DPMPP_TAB_ROWS, self.ROWS_CAP, dtype=th.float32, device=self.device) for k in ("video", "audio")}
        self._qtab = th.zeros(2, self.ROWS_CAP, dtype=th.float32, device=self.device)
        self.retable(tabs, ctr)
        self._record_cond(cond, self._qtab)
        n, geom = self.n, self._geom()
        self._prepare()
        self.predict_x0 = predict_x0 = bool(solver.predict_x0)
        thresholding, max_val = bool(solver.thresholding), float(solver.max_val)
        self.has_final = not predict_x0      # the noise-prediction solver's denoise row needs the data-prediction plan
        self.update_plans, self.final_plans, self._bufs = self._add_set("step", []), [], []
        if self.has_final:
            self._add_set("final", self.final_plans)
        for r, e in enumerate(self.engs):
            t_idx = self.t_idx[self._lane(r)]
            streams = []
            for sid, k, xk, ok in ((0, "video", e.x_video, e.out_video), (1, "audio", e.x_audio, e.out_audio)):
                buf = dict(self._history(xk), x0=th.empty_like(xk), s=th.zeros(n, dtype=th.float32, device=self.device),
                           ws=ops.dpmpp_workspace(n, self.device), lane=r, stream=k)
                self._bufs.append(buf)
                streams.append((sid, k, xk, ok, buf))

            def record(data_form):
                plan = []
                with ops.recording(plan):
                    for sid, k, xk, ok, b in streams:
                        Fk, C, _, HWk = geom[k]
                        with ops.on_stream(sid):
                            src, form, s, Cm = self._record_model_value(xk, ok, b, self.tab[k], t_idx, geom[k], data_form, thresholding, self.FUSED_X0)
                            self._update(xk, src, form == 1, b, self.tab[k], t_idx, Fk, C, Cm, HWk, s, max_val)
                    ops.record_sync(1, 0)
                return plan
            self.update_plans.append(record(predict_x0))
            if self.has_final:
                self.final_plans.append(record(True))
        self.update_plan = self.update_plans[0]

    def _prepare(self):
        """Allocate what the recorded updates read besides the tables and the histories (before anything is recorded)."""

    def _history(self, xk):
        """{name: buffer}: what the update keeps of one stream between evaluations."""
        raise NotImplementedError

    def _update(self, x, src, x0_form, b, tab, t_idx, F, C, Cm, HW, s, max_val):
        """Record the update of one stream from m0 = the first C of src's Cm channels, clamp-scaled by s if given; x0_form (FUSED_X0
        only): src is the model output and m0 its data prediction.  b: the stream's buffers, with its lane (b["lane"]) and key (b["stream"])."""
        raise NotImplementedError

    def retable(self, tabs, ctr=None):
        """Load the tables of DPM_Solver.graph_tables / singlestep_tables (and the key and sample ids of `ctr`) into the buffers the
        recorded plans read."""
        if tabs["rows"] > self.ROWS_CAP:
            raise H.MMDError(f"{self.WHO}: {tabs['rows']} evaluations exceed the table capacity of {self.ROWS_CAP} rows")
        self._load_ctr(ctr)
        self.rows, self.tm = tabs["rows"], tabs["tm"]
        for k in ("video", "audio"):
            self.tab[k][:, :self.rows].copy_(th.from_numpy(tabs["tab"][k]))
        self._qtab[:, :self.rows].copy_(th.from_numpy(tabs["tab2"]))
        self.kinds = [int(v) for v in tabs["tab"]["video"][5]]

    def set_step(self, i, shifts=None, noise=None):
        """Refresh the per-evaluation device state: the step number, the model timestep and the window shifts (one draw per
        evaluation, in the eager loop's order; from the counter with a CounterNoise), and choose the plan set of this row."""
        i = int(i)
        if not 0 <= i < self.rows:
            raise H.MMDError(f"step {i} is outside the {self.rows} rows of the tables")
        self._set = "final" if self.has_final and self.kinds[i] == ops.DPMPP_KIND_DENOISE else "step"      # = DPM1_KIND_DENOISE
        self._push_step(i, int(self.tm[i]), shifts)


class DpmppStepper(SolverStepper):
    """The fixed-grid multistep loop (multimodal_dpm_solver_plus.DPM_Solver.sample_graph): per stream [mmd_dpmpp_x0 (+ the quantile
    selection) + mmd_dpmpp_update], with the previous evaluation's model value m1 as the history."""

    def _history(self, xk):
        return {"m1": th.zeros_like(xk)}

    def _update(self, x, src, x0_form, b, tab, t_idx, F, C, Cm, HW, s, max_val):
        ops.dpmpp_update(x, src, b["m1"], tab, t_idx, F, C, Cm, HW, s=s, max_val=max_val)


class DpmSingleStepper(SolverStepper):
    """The single-step loop of orders 1-3 (DPM_Solver.sample_graph_singlestep): one row per network evaluation, open / stage / denoise
    (ops.DPM1_KIND_*), per stream ONE launch of mmd_dpm_single_update - the data prediction is formed inside it - or, with thresholding,
    mmd_dpmpp_x0 + the quantile selection + that launch.  History: XB, the state at the step's start, and MS, the model value there.

    The first launch of a plan set is its capture's warm-up run, which writes XB and MS (LaneStepper.launch keeps only x around it).
    That is harmless: row 0 is always an open row, which the replay that follows rewrites from the restored x with the same values
    before any stage row reads them, and the denoise row of the "final" set writes neither."""
    FUSED_X0 = True
    WHO = "sample_graph_singlestep"

    def _history(self, xk):
        return {"xb": th.zeros_like(xk), "ms": th.zeros_like(xk)}

    def _update(self, x, src, x0_form, b, tab, t_idx, F, C, Cm, HW, s, max_val):
        ops.dpm_single_update(x, src, b["xb"], b["ms"], tab, t_idx, F, C, Cm, HW, form=1 if x0_form else 0, s=s, max_val=max_val)



class DpmppSdeStepper(SolverStepper):
    """The stochastic multistep loop of the data-prediction solver (DPM_Solver.sample_graph_sde, SDE-DPM-Solver++ of orders 1 and 2): per
    stream [mmd_dpmpp_x0 (+ the quantile selection) + mmd_dpmpp_sde_update], with the previous evaluation's data prediction m1 as the
    history.  Next to the coefficient tables sit the cz tables (fp32 [ROWS_CAP] per stream, the noise coefficient of each row), reloaded
    by retable.  With a seeded.CounterNoise the recorded update is mmd_dpmpp_sde_update_ctr, which draws at the evaluation number it reads
    from t_idx, and the stepper owns no noise buffers; otherwise full-batch noise buffers (lanes read slices) are refilled by set_step at
    every update row - video first, then audio, as the eager loop draws - and left alone at the denoise row."""
    WHO = "sample_graph_sde"

    def _prepare(self):
        e = self.eng
        self.noise = None
        if self.ctr is None:
            self.noise = {k: th.zeros((self.N,) + tuple(xk.shape[1:]), dtype=th.float32, device=self.device)
                          for k, xk in (("video", e.x_video), ("audio", e.x_audio))}

    def _history(self, xk):
        return {"m1": th.zeros_like(xk)}

    def _update(self, x, src, x0_form, b, tab, t_idx, F, C, Cm, HW, s, max_val):
        k, sl = b["stream"], self._lane(b["lane"])
        noise = dict(ctr=(self.key, self.ids[sl], dict(STREAMS)[k])) if self.ctr is not None else dict(noise=self.noise[k][sl])
        ops.dpmpp_sde_update(x, src, b["m1"], tab, self.cz[k], t_idx, F, C, Cm, HW, s=s, max_val=max_val, **noise)

    def retable(self, tabs, ctr=None):
        super().retable(tabs, ctr)
        if not hasattr(self, "cz"):
            self.cz = {k: th.zeros(self.ROWS_CAP, dtype=th.float32, device=self.device) for k in ("video", "audio")}
        for k in ("video", "audio"):
            self.cz[k][:self.rows].copy_(th.from_numpy(tabs["cz"][k]))

    def set_step(self, i, shifts=None, noise=None):
        """SolverStepper.set_step, and the noise of an update row: `noise` = {"video", "audio"}, else drawn (video first, then audio)."""
        super().set_step(i, shifts, noise)
        if self.ctr is not None:
            if noise is not None:
                raise H.MMDError("this step draws its noise in the update kernels (CounterNoise): it takes no noise tensors")
        elif self.kinds[int(i)] != ops.DPMPP_KIND_DENOISE:
            for k in ("video", "audio"):
                if noise is not None:
                    self.noise[k].copy_(noise[k])
                else:
                    self.noise[k].normal_()


class DpmAdaptiveStepper(SolverLanes):
    """The adaptive DPM-Solver++ of order 2 (DPM_Solver.sample_graph_adaptive) with the step-size controller on the device.  A trial
    step s -> t is two graph replays per lane, and no host scalar enters either:
      "open"   [model timesteps of s -> the network's timestep buffer + mmd_cond_replace at alpha(s), sigma(s)] + U-Net plan + per stream
               [the data prediction (+ the quantile selection) + mmd_dpm_adapt_open]
      "stage"  the same at s1, with mmd_dpm_adapt_close per stream, then the join, mmd_dpm_adapt_control and one mmd_dpm_adapt_commit
               per stream.
    The controller (one ops.AdaptBlock per lane) writes the times, the model timesteps, the coefficient rows and the conditioning
    levels of the next trial into device memory that the recorded launches read: rows = the lane's samples, row index n for sample n,
    -1 once it is done - the kernels then write nothing for it, so further trial steps are exact no-ops for a finished sample.
    control="sample": every sample has its own s, h, E and decision; control="batch": the reference's rule, one E (the maximum) and one
    s, h for the batch, which needs the whole batch in one lane.  atol, rtol, theta, t_err, h_init, t_T and t_0 sit in a device
    parameter block (retable refills it), so a kept stepper serves other tolerances with the graph execs it has.

    The first launch of a set is its capture's warm-up run; launch() keeps the state, PREV and the controller's block intact around it
    (the warm-up of "stage" would otherwise count as a trial)."""
    WHO = "sample_graph_adaptive"

    def __init__(self, solver, unet, batch, device, tabs, use_graph=True, lanes=None, cond=None, ctr=None, select=None, control="sample"):
        if control not in ("sample", "batch"):
            raise H.MMDError(f"{self.WHO}: control must be 'sample' or 'batch', got {control!r}")
        if control == "batch":
            lanes = 1 if lanes is None else lanes
            if int(lanes) != 1:
                raise H.MMDError(f"{self.WHO}: control='batch' takes the maximum over the whole batch, which must sit in one lane: lanes must be 1, got {lanes}")
        if not solver.predict_x0:
            raise H.MMDError(f"{self.WHO}: the adaptive stepper is built in its data-prediction form only (predict_x0=True)")
        super().__init__(unet, batch, device, lanes, use_graph, ctr, select)
        self.control = control
        self.params = th.zeros(ops.ADAPT_PARAMS, dtype=th.float64, device=self.device)
        self.log_alpha = th.zeros(len(tabs["log_alpha"]), dtype=th.float64, device=self.device)
        self.blk = [ops.AdaptBlock(self.n, self.device) for _ in self.engs]
        self._status = th.zeros(self.lanes, 2, dtype=th.int32).pin_memory()
        self.retable(tabs, ctr)
        self._alloc_cond(cond)
        n, geom = self.n, self._geom()
        thresholding, max_val = bool(solver.thresholding), float(solver.max_val)
        self._bufs = []
        sets = {"open": ([], []), "stage": ([], [])}
        for r, e in enumerate(self.engs):
            blk, streams = self.blk[r], []
            for sid, k, xk, ok in ((0, "video", e.x_video, e.out_video), (1, "audio", e.x_audio, e.out_audio)):
                per = xk[0].numel()
                buf = dict(xb=th.zeros_like(xk), ms=th.zeros_like(xk), lo=th.zeros_like(xk), prev=th.zeros_like(xk), x0=th.zeros_like(xk),
                           s=th.zeros(n, dtype=th.float32, device=self.device), ws=ops.dpmpp_workspace(n, self.device),
                           partial=th.zeros(n, ops.dpm_adapt_chunks(per), dtype=th.float64, device=self.device), per=per, lane=r, stream=k, x=xk)
                self._bufs.append(buf)
                streams.append((sid, k, xk, ok, buf))
            for name, (pres, plans) in sets.items():
                opening = name == "open"
                tab, qtab, tm = (blk.tab_open, blk.q_s, blk.tm_s) if opening else (blk.tab_close, blk.q_s1, blk.tm_s1)
                pre, plan = [], []
                with ops.recording(pre):       # on the origin stream: this evaluation's model timesteps, and the known cells at its level
                    ops.dpm_adapt_time(tm, e.t_i64)
                    for k, tag in STREAMS:
                        if k in self.cond:
                            self._cond_replace(r, k, tag, qtab, blk.k, None)
                with ops.recording(plan):
                    for sid, k, xk, ok, b in streams:
                        Fk, C, _, HWk = geom[k]
                        with ops.on_stream(sid):
                            src, form, s, Cm = self._record_model_value(xk, ok, b, tab, blk.k, geom[k], True, thresholding, True)
                            if opening:
                                ops.dpm_adapt_open(xk, src, b["xb"], b["ms"], b["lo"], tab, blk.k, Fk, C, Cm, HWk, form=form, s=s, max_val=max_val)
                            else:
                                ops.dpm_adapt_close(xk, src, b["xb"], b["ms"], b["lo"], b["prev"], tab, blk.k, self.params, b["partial"], Fk, C, Cm,
                                                    HWk, form=form, s=s, max_val=max_val)
                    ops.record_sync(1, 0)
                    if not opening:      # behind the join, on the origin stream: the decision, then what it means for x and PREV
                        ops.dpm_adapt_control(blk, self.params, self.log_alpha, [(b["partial"], b["per"]) for *_, b in streams],
                                              batch=control == "batch")
                        for _, _, xk, _, b in streams:
                            ops.dpm_adapt_commit(xk, b["xb"], b["prev"], b["lo"], blk.cnt)
                pres.append(pre)
                plans.append(plan)
        for name, (pres, plans) in sets.items():
            self._add_set(name, plans)
            self._sets[name].pre = pres
        self.update_plans = self._sets["open"].plans
        self.trials = self.evals = self.host_reads = 0

    @property
    def graphs(self):
        return self._sets["open"].graphs

    def retable(self, tabs, ctr=None):
        """Load the parameter block, the schedule and (with a counter source) the key and sample ids: what another call may change."""
        if len(tabs["log_alpha"]) != self.log_alpha.numel():
            raise H.MMDError(f"{self.WHO}: the schedule's length is fixed when the stepper is built")
        self._load_ctr(ctr)
        ops.dpm_adapt_params(self.device, out=self.params, **tabs["params"])
        self.log_alpha.copy_(th.as_tensor(tabs["log_alpha"], dtype=th.float64))

    # ------------------------------------------------------------------ launch: the sets carry their own pre-plans
    def _lane_launch(self, ps, r, stream):
        e = self.engs[r]
        aux = e.aux.cuda_stream
        ops.run_plan(ps.pre[r], stream, aux)
        ops.run_plan(e.plan, stream, aux)
        ops.run_plan(ps.plans[r], stream, aux)

    def _mutable(self):
        """Every buffer a set's warm-up run may change and its first replay does not rewrite from scratch."""
        out = [b[name] for b in self._bufs for name in ("x", "prev")]
        for blk in self.blk:
            out += [blk.state, blk.itab, blk.cnt, blk.ftab, blk.status]
        return out + [e.t_i64 for e in self.engs]

    def launch(self):
        ps = self._sets[self._set]
        if self.use_graph and ps.graphs is None:
            keep = [(t, t.clone()) for t in self._mutable()]
            self._capture(ps)
            for t, v in keep:
                t.copy_(v)
        if self.use_graph:
            self._fan(_replay, ps)
        else:
            if self.lanes == 1:
                self.eng.aux.wait_stream(th.cuda.current_stream(self.device))
            self._fan(self._lane_launch, ps)

    # ------------------------------------------------------------------ the loop's pieces
    def start(self):
        """After load() (and load_cond()): PREV = x_T, and the controller's init - s = t_T, h = h_init, the first trial's rows."""
        for b in self._bufs:
            b["prev"].copy_(b["x"])
        for blk in self.blk:
            ops.dpm_adapt_control(blk, self.params, self.log_alpha, batch=self.control == "batch", init=True)
        self.trials = self.evals = self.host_reads = 0

    def _push_shifts(self, i, shifts=None):
        """The window shifts of evaluation i: one draw per block for the whole batch, from the counter with a CounterNoise."""
        if shifts is None:
            own = self.ctr is not None and self.unet.shift_source is None
            shifts = self.ctr.shifts(i, self.unet) if own else self.unet.draw_shifts()
        for e in self.engs:
            e.set_shifts(shifts)

    def trial(self):
        """One trial step of every lane: the open and the stage replay, two network evaluations."""
        for name in ("open", "stage"):
            self._set = name
            self._push_shifts(self.evals)
            self.launch()
            self.evals += 1
        self.trials += 1

    def poll(self):
        """(samples not done, fault) from the lanes' status words: one small read through a pinned buffer, and the only host wait."""
        for r, blk in enumerate(self.blk):
            self._status[r].copy_(blk.status, non_blocking=True)
        th.cuda.current_stream(self.device).synchronize()
        self.host_reads += 1
        return int(self._status[:, 0].sum()), bool(self._status[:, 1].any())

    def stats(self):
        """Per-sample {"attempts", "accepted", "nfe"} (int64 host tensors [N]) of the loop so far."""
        cnt = th.cat([blk.cnt for blk in self.blk]).cpu().to(th.int64)
        a = cnt[:, ops.ADAPT_C["attempts"]]
        return {"attempts": a, "accepted": cnt[:, ops.ADAPT_C["accepted"]], "nfe": 2 * a}

    def trace(self):
        """The controller's block of every sample as host tensors (a device read: for tests and tools, one call per trial step with
        poll=1): "state" fp64 [N, 8], "cnt" int32 [N, 4], "ftab" fp32 [16, N], "itab" int64 [3, N]."""
        return {"state": th.cat([b.state for b in self.blk]).cpu(), "cnt": th.cat([b.cnt for b in self.blk]).cpu(),
                "ftab": th.cat([b.ftab for b in self.blk], dim=1).cpu(), "itab": th.cat([b.itab for b in self.blk], dim=1).cpu()}
