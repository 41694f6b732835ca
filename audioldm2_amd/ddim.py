"""DDIM sampler on MI355X: drop-in for `audioldm2.latent_diffusion.models.ddim.DDIMSampler`
(models/ddim.py:15-355).  Same constructor / `sample()` / `ddim_sampling()` / `p_sample_ddim()`
signatures and return values; constructed by name in `LatentDiffusion.sample_log` (ddpm.py:1437), so a
reference user rebinds `ddpm.DDIMSampler = audioldm2_amd.ddim.DDIMSampler`.

Differences that matter on MI355X:
  * classifier-free guidance runs as ONE UNet pass over [uncond ; cond] (2B samples) when the model
    exposes `apply_model_cfg` (the reference runs two sequential passes, ddim.py:293-296);
  * CFG combine + x0 prediction + x_{t-1} update is one fused kernel (ops.ddim_step);
  * the per-step launch sequence (~1000 kernels) is captured once into a HIP graph and replayed;
    timestep, DDIM coefficients and noise are device-side inputs of the graph;
  * RNG contract: x_T and the per-step noise are drawn from the HOST CPU
    generator in the reference's order and shapes (ddim.py:191,351 via util.py:289-294), uploaded
    once — results match the CPU reference on the same seed.

What this class shares with PLMSSampler and DPMSolverSampler (the schedule, the run plan, the UNet pass of a step, the graph
stepper, the noise feed) is in sampling.py; here are DDIM's coefficient rows, its step closure, the graph cache on the UNet and the
threaded noise feed of its loop, the eager single-step methods, and sdedit_plan.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
# the samplers' shared core; every name below lived in this module before sampling.py existed and is still exported from here
from .sampling import (GraphStepper, SamplerBase, _NoiseFeed, check_guidance_rescale, check_resample, check_t_start,  # noqa: F401
                       ddim_step_rows, drop_graph_entries, guidance_table, host_drawer, log_step, make_ddim_sampling_parameters,
                       make_ddim_timesteps, renoise_coef, resample_visits)



def sdedit_plan(strength, ddim_steps, alphas_cumprod, num_timesteps):
    """Pure host function: where an audio-to-audio job (SDEdit: noise the source, then denoise it under the prompt) enters a
    sampler's schedule -> (t_enc, timestep, sqrt_abar, sqrt_1m_abar).

    t_enc = int(strength * ddim_steps) is the number of steps to run (AudioLDM's `transfer_strength` rule); strength must lie in
    (0, 1] and t_enc must be >= 1.  The run executes schedule indices t_enc-1 ... 0, and its first step takes its input to be at
    the noise level of index t_enc-1: `timestep` = make_ddim_timesteps("uniform", ddim_steps, num_timesteps)[t_enc - 1], and the
    source is noised to exactly that level, x_t = sqrt_abar * z + sqrt_1m_abar * noise with abar = alphas_cumprod[timestep].  The
    well-known img2img scripts noise to index t_enc instead — one level above what their first step assumes, and at strength 1
    an index past the end of the table; this function does not follow them.  The two coefficients are evaluated in fp64 from
    `alphas_cumprod` as given and returned as Python floats (the caller rounds them to fp32 once)."""
    try:
        s = float(strength)
    except (TypeError, ValueError):
        raise ValueError(f"strength must be a number in (0, 1], got {strength!r} (ddim_steps={ddim_steps!r})")
    if isinstance(ddim_steps, bool) or not isinstance(ddim_steps, (int, np.integer)) or ddim_steps < 1:
        raise ValueError(f"ddim_steps must be a positive integer, got {ddim_steps!r} (strength={strength!r})")
    if not (np.isfinite(s) and 0.0 < s <= 1.0):
        raise ValueError(f"strength must lie in (0, 1], got strength={strength!r} (ddim_steps={ddim_steps})")
    t_enc = int(s * int(ddim_steps))
    if t_enc < 1:
        raise ValueError(f"strength={strength!r} of ddim_steps={ddim_steps} leaves int(strength * ddim_steps) = 0 steps to run: "
                         "raise one of them")
    ts = make_ddim_timesteps("uniform", int(ddim_steps), int(num_timesteps), verbose=False)
    t_enc = min(t_enc, len(ts))
    timestep = int(ts[t_enc - 1])
    ac = alphas_cumprod.detach().cpu().numpy() if torch.is_tensor(alphas_cumprod) else np.asarray(alphas_cumprod)
    abar = float(np.asarray(ac, dtype=np.float64)[timestep])
    return t_enc, timestep, float(np.sqrt(abar)), float(np.sqrt(1.0 - abar))


class DDIMSampler(SamplerBase):
    def __init__(self, model, schedule="linear", device=torch.device("cuda"), **kwargs):
        super().__init__(model, schedule)
        self.device = device

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """ddim.py:33-91 (host side, float tables only)."""
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1.0 - self.ddim_alphas.numpy())
        self.ddim_coef = ddim_step_rows(self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev,
                                        self.ddim_sqrt_one_minus_alphas)  # [S, 5] fp32 (host)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0,
               noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               dynamic_threshold=None, ucg_schedule=None, guidance_rescale=0.0, t_start=None, windows=None, resample=None,
               graded=False, **kwargs):
        """ddim.py:94-163, plus `guidance_rescale` (phi of Lin et al. 2023; 0: off — the reference's step), `t_start` (None: the
        whole schedule; k: its first k entries, indices k-1 ... 0, from x_T — see check_t_start), `windows` (None, or a
        windows.window_plan over the long latent `shape`: windowed diffusion, see SamplerBase.plan_run) and `resample` (None, or
        RePaint's pair (n, jump): resampled inpainting, see ddim_sampling) and `graded` (True: `mask` is a map of keep levels in
        [0, 1], graded keep, see ddim_sampling)"""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._refuse_resample(resample, temperature, mask, x0, windows)
        if quantize_x0 or score_corrector is not None or dynamic_threshold is not None \
                or noise_dropout != 0.0 or ucg_schedule is not None:
            raise NotImplementedError("DDIMSampler(HIP): option not used by the AudioLDM2 pipeline")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        check_t_start(t_start, kwargs.get("timesteps"), len(self.ddim_timesteps))
        C, H, W = shape
        size = (batch_size, C, H, W)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  mask=mask, x0=x0, temperature=temperature, x_T=x_T,
                                  log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, guidance_rescale=guidance_rescale,
                                  t_start=t_start, windows=windows, resample=resample, graded=graded)

    @staticmethod
    def _refuse_resample(resample, temperature, mask, x0, windows):
        """What `resample=` cannot go with, refused before the schedule is cut (plan_run refuses the values against the cut
        schedule, before the run's first draw)."""
        if check_resample(resample) is None:
            return
        if temperature != 1.0:
            raise ValueError(f"resample= needs temperature == 1.0, got {temperature!r}: the noise feed scales the step-noise row, "
                             "and the forward jump's noise must be unit")
        if mask is None and x0 is None and getattr(windows, "x0", None) is None:
            raise ValueError("resample= needs something to harmonise with: a mask / x0, or a source on the window plan "
                             "(windows.with_source)")

    # ------------------------------------------------------------------------------------------
    def _draw_noise(self, shape, steps, x_T, with_mask):
        """Replays the reference's host RNG order: x_T, then per step [q_sample noise (inpainting
        only, ddim.py:228 / ddpm.py:430-436)], step noise (ddim.py:351).  (Eager form, used by tests;
        ddim_sampling streams the same sequence through _NoiseFeed.)"""
        draw = host_drawer(shape, self.noise_shard)
        img = draw() if x_T is None else x_T
        step_noise, q_noise = [], []
        for _ in range(steps):
            if with_mask:
                q_noise.append(draw())
            step_noise.append(draw())
        return img, torch.stack(step_noise), (torch.stack(q_noise) if with_mask else None)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None,
                      timesteps=None, quantize_denoised=False, mask=None, x0=None, img_callback=None,
                      log_every_t=100, temperature=1.0, noise_dropout=0.0, score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, guidance_rescale=0.0,
                      t_start=None, windows=None, resample=None, graded=False):
        """ddim.py:166-262; `t_start=k`: run exactly the schedule's first k entries (check_t_start); `windows`: a window plan
        over the long latent `shape` (SamplerBase.plan_run) — gather and merge become two nodes of the step graph; a plan
        with a source (windows.with_source) blends the source in inside the step: the gather node becomes ops.window_blend_gather,
        which reads the feed's q-noise table with the graph's step counter — the host issues nothing new per step.

        `resample=(n, jump)` (RePaint's jump_n_sample and jump_length, in sampler steps): resampled inpainting.  The
        run is a sequence of V visits (sampling.resample_visits), every table has V rows in visit order and the device counter
        counts visits.  A step visit is the step it is without the keyword — the same replayed graph, captured once; a renoise
        visit k -> k - jump is two host-issued launches between two replays: ops.renoise_indexed on the whole latent (the known
        region is blended back in by the next step visit) with the visit's step-noise row as its unit noise, then
        ops.step_advance.  EVERY visit makes the feed's draws in the feed's order (q-noise row, step-noise row); a renoise
        visit's q-noise row is drawn and not read.  Callbacks and `intermediates` see step visits only, with the step's loop
        position i (the schedule index total_steps - 1 - i), so a position that is sampled n times is reported n times.  Needs
        a mask / x0 or a source on the plan, and temperature == 1.0; (1, jump) is the run without the keyword.

        `graded=True`: `mask` is a map of keep LEVELS in [0, 1] (differential diffusion; windows.keep_levels).  In
        front of every blend one launch, ops.keep_threshold_indexed, rewrites the binary mask the blend reads from the levels and
        the visit's threshold (sampling.keep_thresholds): a frame of level m is replaced by q_sample(x0, t) for its first
        sampling.hold_steps(m, S) steps and is free afterwards.  A windowed run issues it inside the captured step (model_output),
        the plain masked loop between the replays.  The draws and their order do not change.  Refused before any draw: no mask
        or source, levels outside [0, 1] or not finite.  A source on the plan carries its own flag (windows.with_source)."""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._refuse_resample(resample, temperature, mask, x0, windows)
        if ddim_use_original_steps:
            # the reference's own p_sample_ddim reads `self.model.ddim_sigmas_for_original_num_steps` here (ddim.py:324-327), a
            # buffer it registered on the SAMPLER (ddim.py:84-91): with LatentDiffusion as the model this path raises
            # AttributeError in the reference itself, so there is no behaviour to reproduce
            raise NotImplementedError("DDIMSampler(HIP): ddim_use_original_steps=True is not runnable in the reference either "
                                      "(ddim.py:324-327 reads a buffer the model does not have)")
        dev = torch.device("cuda")
        shape = tuple(shape)
        b = shape[0]
        # RNG contract R: x_T first, then the per-step draws, all from the host generator in the reference's order; the per-step
        # draws are streamed (see _NoiseFeed).  The table: the schedule's rows total_steps-1 ... 0
        plan = self.plan_run(cond, shape, x_T, t_start, timesteps,
                             lambda n, cfg: guidance_table(self.ddim_coef[:n].flip(0), unconditional_guidance_scale, cfg,
                                                           guidance_rescale),
                             unconditional_guidance_scale, unconditional_conditioning, guidance_rescale, mask, x0, windows,
                             resample, graded)
        total_steps, use_cfg, rescale, img, prepared = plan.total_steps, plan.use_cfg, plan.rescale, plan.img, plan.prepared
        cond, unconditional_conditioning = plan.cond, plan.uncond   # tiled W times in a windowed run, else the arguments
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        if total_steps == 0:
            return img, intermediates
        # resampled inpainting: the tables' rows — and the counter — are per VISIT (plan_run); without it a visit is a step
        visits = plan.visits
        n_rows = total_steps if visits is None else len(visits)

        # The captured step graph, its static input buffers and the batched conditioning live on the UNet
        # module and are reused by the next sampling run of the same geometry (text_to_audio in a loop):
        # that run skips the eager first step and the re-capture (~0.1 s per job).  New conditioning is
        # copied INTO the captured tensors and the cross-attention K/V projections are recomputed in
        # place; invalidate_packed() (weights changed) drops the cache.
        # The graph's per-step inputs are selected ON THE DEVICE: a step counter indexes the coefficient table and the noise
        # buffer (aldm_ddim_step_indexed, in place on x) and the graph's last node advances the counter and writes the next
        # step's timestep row (aldm_step_advance) — between two replays the host issues nothing but a stream wait on the
        # noise upload event, once per 8 steps (round 2 issued three copies per step from the host).
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        # a window plan with a source: the blend is a node of the step graph (model_output), its q-noise the feed's table.  Like
        # a masked run it stays out of the cross-run graph cache
        blend = plan.win is not None and plan.win.blend
        can_cache = (prepared is not None and mask is None and not blend and self.use_graph
                     and hasattr(unet, "refresh_context_kv")
                     and os.environ.get("ALDM_NO_GRAPH_CACHE", "0") != "1")
        key = None
        if can_cache:
            # `rescale`: the launch sequence differs; the VALUES of the scale and phi live in coef_all, copied in below
            key = (shape, total_steps, tuple(tuple(c.shape) for c in prepared["ctxs"]),
                   None if prepared["y"] is None else tuple(prepared["y"].shape), rescale)
            if windows is not None:
                # the starts are kernel arguments of the captured gather and merge nodes
                from .windows import plan_key
                key = key + (plan_key(windows),)
            if plan.compose is not None:
                # composable guidance: K and the table's row count are kernel arguments of the captured compose node; the weight
                # VALUES live in the entry's table, refilled per job.  A K = 1 job has a plain guided job's context shapes, not its
                # launch sequence: the marker keeps the two apart
                key = key + (("compose",) + tuple(plan.compose.shape),)
        ent = unet._graph_cache.get(key) if can_cache else None
        if ent is not None and ent.get("kv") is None:
            # the entry never got as far as recording the K/V buffers its graph reads (e.g. an interrupted first run)
            drop_graph_entries(unet._graph_cache)
            ent = None
        if ent is not None:
            for dst, src in zip(ent["prepared"]["ctxs"] + ent["prepared"]["masks"],
                                prepared["ctxs"] + prepared["masks"]):
                dst.copy_(src)
            if prepared["y"] is not None:
                ent["prepared"]["y"].copy_(prepared["y"])
            unet.refresh_context_kv(ent["kv"])  # in place: the captured graph keeps reading these buffers
            ent["x_cur"].copy_(img)
            ent["coef_all"].copy_(plan.coef)
            ent["t_tab"].copy_(plan.t_tab)
            if plan.win is not None and plan.win.wr is not None:
                # a row plan: the captured merge node reads the entry's weight buffer; this job's timeline goes INTO it (the key
                # holds the row geometry only), outside any capture
                ent["win"].wr.copy_(plan.win.wr)
            if plan.win is not None and plan.win.phase is not None:
                # a phased ring plan: the captured gather and merge nodes read the entry's phase table; this job's phases go INTO
                # it (the key holds "phased" and the step count, not the values), outside any capture
                ent["win"].phase.copy_(plan.win.phase)
            if plan.compose is not None:
                # composable guidance: the captured compose node reads the entry's table; this job's weights go INTO it
                ent["compose"].copy_(plan.compose)
        else:
            # static buffers = the graph's inputs
            ent = {"x_cur": img.clone(), "pred_x0": torch.empty_like(img), "t_cur": plan.t_tab[0].clone(),
                   "step_idx": torch.zeros(1, device=dev, dtype=torch.int32), "coef_all": plan.coef.clone(),
                   "t_tab": plan.t_tab.clone(),
                   "noise_all": torch.empty((n_rows,) + shape, device=dev, dtype=torch.float32), "prepared": prepared}
            if rescale:
                ent["eps_g"] = torch.empty_like(img)   # the rescaled combined model output
            if plan.win is not None:
                ent["win"] = plan.win   # the window plan and the static buffers of the gather and the merge
            if blend:
                # the fused blend-and-gather node reads row step_idx of the q-noise table the feed fills
                ent["qnoise_all"] = torch.empty_like(ent["noise_all"])
                plan.win.qnoise, plan.win.step_idx = ent["qnoise_all"], ent["step_idx"]
            if plan.win is not None and plan.win.phase is not None:
                # moving window phases: the gather and merge nodes select the visit's phase with the graph's step counter
                plan.win.step_idx = ent["step_idx"]
            if plan.compose is not None:
                # composable guidance: the compose node behind the UNet pass selects the visit's weights with the graph's counter
                ent["compose"], cond.step_idx = plan.compose, ent["step_idx"]

            def step(e=ent):
                x_c = e["x_cur"]
                eps = self.model_output(x_c, e["t_cur"], b, cond, unconditional_conditioning, use_cfg, e["prepared"],
                                        win=e.get("win"))
                if rescale:
                    eps = ops.cfg_rescale_indexed(eps, e["eps_g"], e["coef_all"], e["step_idx"])
                ops.ddim_step_indexed(x_c, eps, e["noise_all"], e["coef_all"], e["step_idx"], e["pred_x0"])
                ops.step_advance(e["step_idx"], e["t_tab"], e["t_cur"])
            ent["run_step"] = GraphStepper(step, self.use_graph)
            if can_cache:
                drop_graph_entries(unet._graph_cache)  # one geometry at a time: the graph pins its activation pool
                unet._graph_cache[key] = ent
        ent["step_idx"].zero_()
        ent["t_cur"].copy_(ent["t_tab"][0])
        x_cur, pred_x0 = ent["x_cur"], ent["pred_x0"]
        # the per-step draws are streamed by a drawer thread straight into the graph's static noise buffer (see _NoiseFeed)
        # While a run is in flight ONLY the drawer thread may consume torch's default CPU generator (it runs up to three 8-step
        # chunks ahead).  In the reference ANY callback may draw from that generator between two steps, so a run WITH a callback
        # keeps the draws on the launching thread, one step at a time, sequenced with the callback exactly as in the reference —
        # unless the callback declares that it never draws (`callback.uses_rng = False`), which restores the threaded feed
        # (ADVICE r3 + r4: opt-OUT, not opt-in — a silent interleaving gives a different noise stream with no diagnostic;
        # INTEGRATION.md §5; ALDM_NOISE_THREAD=0 forces the unthreaded feed for every run).
        cb_rng = any(getattr(f, "uses_rng", True) for f in (callback, img_callback) if f is not None)
        feed = _NoiseFeed(plan.draw, n_rows, shape, mask is not None or blend, temperature, dev, noise_buf=ent["noise_all"],
                          qnoise_buf=ent.get("qnoise_all"), **({"threaded": False, "chunk": 1} if cb_rng else {}))
        feed.produce_next()
        qn = feed.qnoise
        run_step = ent["run_step"]
        try:
            for v in range(n_rows):
                opens_chunk = feed.wait(v)  # current stream waits for the upload of visit v's noise chunk
                if visits is not None and visits[v][0] == "renoise":
                    # the forward jump k -> k - jump on the whole latent, between two replays: the counter selects the visit's
                    # (c0, c1) and its step-noise row, as it does for a step; the step graph is neither touched nor re-captured
                    ops.renoise_indexed(x_cur, ent["noise_all"], ent["coef_all"], ent["step_idx"])
                    ops.step_advance(ent["step_idx"], ent["t_tab"], ent["t_cur"])
                    if opens_chunk and not cb_rng:
                        feed.produce_next()
                    continue
                i = v if visits is None else visits[v][1]   # the loop position of this step
                if mask is not None:
                    # img = q_sample(x0, ts)*mask + (1-mask)*img   (ddim.py:226-231, ddpm.py:430-436)
                    if plan.level_d is not None:   # graded keep levels: this visit's binary mask first
                        ops.keep_threshold_indexed(plan.level_d, plan.keep_thr[v:v + 1], plan.mask_d)
                    ops.inpaint_blend(x_cur, plan.x0_d, qn[v], plan.mask_d, plan.blend_coef[v])
                run_step()  # eager the first time, then one HIP-graph replay per step
                if can_cache and ent.get("kv") is None:
                    # after the eager first step: the K/V projections of this run's contexts exist; the cache entry owns
                    # them from here on (the graph captured at the next step reads these very buffers)
                    ent["kv"] = unet.collect_context_kv(ent["prepared"]["ctxs"])
                if opens_chunk and not cb_rng:
                    feed.produce_next()  # (unthreaded mode only) draw + upload the NEXT chunk while the GPU works on this one
                log_step(i, total_steps, log_every_t, x_cur, pred_x0, intermediates, callback, img_callback)
        finally:
            feed.close()   # the generator is past the run's last draw before anyone else draws from it
        return x_cur.clone(), intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False,
                      quantize_denoised=False, temperature=1.0, noise_dropout=0.0, score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, dynamic_threshold=None, guidance_rescale=0.0):
        """ddim.py:265-355 — single step with the reference's signature (noise from the host CPU
        generator, like `noise_like` does on a CPU reference run), plus `guidance_rescale`."""
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        b = x.shape[0]
        use_cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
        eps = self.model_output(x, t.float().repeat(2 if use_cfg else 1), b, c, unconditional_conditioning, use_cfg, None)
        coef = guidance_table(self.ddim_coef[index].reshape(1, 5), unconditional_guidance_scale, use_cfg, guidance_rescale)
        if use_cfg and guidance_rescale > 0.0:
            eps = ops.cfg_rescale_indexed(eps, torch.empty_like(eps[0]), coef.to(x.device))
        coef = coef[0]
        if repeat_noise:
            noise = torch.randn((1, *x.shape[1:])).repeat(b, 1, 1, 1)
        else:
            noise = torch.randn(x.shape)
        noise = (noise * temperature).to(x.device)
        x_prev, pred_x0 = ops.ddim_step(x.float().contiguous(), eps, noise.contiguous(), coef.to(x.device))
        return x_prev, pred_x0

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:434-449: x0 noised to DDIM index t (fast, no exact reconstruction): sqrt(a_t) x0 + sqrt(1 - a_t) noise,
        the noise from the host generator when not given (a CPU reference run's `randn_like`)."""
        if use_original_steps:
            sa, so = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        else:
            sa, so = torch.sqrt(self.ddim_alphas), torch.from_numpy(np.asarray(self.ddim_sqrt_one_minus_alphas))
        if noise is None:
            noise = torch.randn(x0.shape)
        tt = t.detach().cpu().long()
        shape = (x0.shape[0],) + (1,) * (x0.dim() - 1)
        a = sa.float()[tt].reshape(shape).to(x0.device)
        b = so.float()[tt].reshape(shape).to(x0.device)
        return a * x0 + b * noise.to(x0.device)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, guidance_rescale=0.0):
        """ddim.py:452-491: run the last `t_start` DDIM steps from x_latent (one p_sample_ddim per step: the eager path over
        the same kernels as ddim_sampling; the step noise comes from the host generator in the reference's order)."""
        if use_original_steps:
            raise NotImplementedError("DDIMSampler(HIP): use_original_steps=True is not runnable in the reference either "
                                      "(ddim.py:324-327 reads a buffer the model does not have)")
        timesteps = self.ddim_timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        x_dec = x_latent
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
            x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index, use_original_steps=use_original_steps,
                                          unconditional_guidance_scale=unconditional_guidance_scale,
                                          unconditional_conditioning=unconditional_conditioning,
                                          guidance_rescale=guidance_rescale)
            if callback:
                callback(i)
        return x_dec
