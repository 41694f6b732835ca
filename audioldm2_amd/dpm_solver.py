"""DPM-Solver++(2M) sampler on MI355X (Lu et al. 2022, "DPM-Solver++", Algorithm 2): the deterministic second-order multistep
solver in its data-prediction form, over the model's eps output.  It has no counterpart in the reference; the class carries
PLMSSampler's parameter lists and `(samples, intermediates)` return, and is selected by name: `sampler="dpmpp_2m"` in
`LatentDiffusion.sample_log` / `generate_batch` / `generate_batch_masked` / `text_to_audio` / `super_resolution_and_inpainting`.

One step from abar_t to abar_prev — DDIM's `ddim_alphas[index]` and `ddim_alphas_prev[index]`, so the last step lands on
`alphas_cumprod[0]` — with alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), h = lambda_prev - lambda_t > 0:
    e  = e_u + s (e_c - e_u)                                  guidance combine
    x0 = (x - sigma_t e) / alpha_t
    D  = x0                                                   first-order step
       = x0 + w (x0 - x0_last),  w = 1 / (2 r), r = h_last / h   otherwise
    x  = (sigma_prev / sigma_t) x - alpha_prev expm1(-h) D ;  x0_last = x0
Step 0 is first order (no history yet); the last step is first order when the run has fewer than 15 steps ("lower order final":
the last interval has by far the largest h on the uniform grid and the linear extrapolation overshoots there on short runs).  A
first-order step is algebraically the DDIM eta = 0 step.

On MI355X:
  * guidance combine + x0 + extrapolation + update + history are one kernel per step (ops.dpmpp_step_indexed); the history is ONE
    slab, which is also the pred_x0 output;
  * the order of a step is a column of its coefficient row (w = 0: first order, the slab is not read), so EVERY step, step 0
    included, is the same launch sequence on one stream: UNet pass -> dpmpp_step_indexed -> step_advance, run eagerly once,
    captured into a HIP graph at the second step and replayed after (sampling.GraphStepper).  The graph lives for one sampling run;
    nothing is read from or written to the UNet's DDIM graph cache;
  * the coefficient table is built in fp64 from the fp32 `alphas_cumprod` buffer and rounded once to fp32
    (dpmpp_2m_coefficients);
  * RNG: the solver is deterministic and there is no reference implementation whose discarded draws would have to be mirrored.
    The host generator is consumed by x_T (when not given) and, when inpainting, by one `q_sample` draw per step — and by
    nothing else.

SDE.  DPMSolverSDESampler (`sampler="dpmpp_2m_sde"`) is the second-order multistep SDE solver of the same paper in its
midpoint form, generalised by eta in (0, 1] from the ODE solver above (eta = 0) to the full SDE (eta = 1): e, x0 and D as above, then
    x  = c2 x + c3 D + c4 z ;  x0_last = x0
    c2 = (sigma_prev / sigma_t) exp(-eta h),  c3 = -alpha_prev expm1(-(1 + eta) h),  c4 = sigma_prev sqrt(-expm1(-2 eta h))
with z the step's unit noise times `temperature`, and the same rule for the order of a step.  For any eta a first-order step is a
member of the DDIM family (c2 alpha_t + c3 = alpha_prev, (c2 sigma_t)^2 + c4^2 = sigma_prev^2); at eta = 1 it is DDIM's eta = 1
step.  One kernel per step again (ops.dpmpp_sde_step_indexed: the row's first eight columns are dpmpp_step_indexed's, column 8 is
c4), the same launch sequence, the same loop — `dpm_sampling` serves both classes.  RNG: DDIM's contract and machinery — x_T first;
then per step the q-noise draw where there is a mask or a source on the plan, then the step noise; streamed by sampling._NoiseFeed
into static [total_steps, *shape] device tables the kernel indexes with the step counter, so the host issues nothing per step; a
callback that may draw (`uses_rng` not False) forces the unthreaded one-step-at-a-time feed, as in ddim_sampling.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .sampling import GraphStepper, SamplerBase, _NoiseFeed, check_guidance_rescale, check_t_start, guidance_table, log_step

LOWER_ORDER_FINAL_BELOW = 15   # runs shorter than this take their last step at first order


def dpmpp_2m_coefficients(alphas, alphas_prev):
    """Pure host function: the [S, 5] fp64 rows {sigma_t, alpha_t, sigma_prev / sigma_t, -alpha_prev expm1(-h), w} of a run whose
    step i goes from abar = alphas[i] to alphas_prev[i] (step order: the noisiest step first).  w = 1 / (2 r) with r = h_last / h
    and h_last the previous step's h; w = 0 marks a first-order step: row 0, and the last row when S < 15."""
    a_t = np.asarray(alphas, dtype=np.float64).reshape(-1)
    a_p = np.asarray(alphas_prev, dtype=np.float64).reshape(-1)
    assert a_t.shape == a_p.shape
    S = a_t.shape[0]
    alpha_t, sigma_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    alpha_p, sigma_p = np.sqrt(a_p), np.sqrt(1.0 - a_p)
    h = np.log(alpha_p / sigma_p) - np.log(alpha_t / sigma_t)
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        raise ValueError("dpmpp_2m_coefficients: every step must go to a less noisy state (0 < abar_t < abar_prev < 1)")
    w = np.zeros(S)
    w[1:] = h[1:] / (2.0 * h[:-1])
    if S < LOWER_ORDER_FINAL_BELOW:
        w[S - 1:] = 0.0
    return np.stack([sigma_t, alpha_t, sigma_p / sigma_t, -alpha_p * np.expm1(-h), w], 1)


def dpmpp_2m_sde_coefficients(alphas, alphas_prev, eta):
    """Pure host function: the [S, 6] fp64 rows {sigma_t, alpha_t, c2, c3, w, c4} of the SDE solver (module docstring, "SDE") over
    the same steps as dpmpp_2m_coefficients, with its argument checks and its w rule:
        c2 = (sigma_prev / sigma_t) exp(-eta h),  c3 = -alpha_prev expm1(-(1 + eta) h),  c4 = sigma_prev sqrt(-expm1(-2 eta h)).
    eta must be finite and in [0, 1] (ValueError otherwise).  At eta = 0 columns 0-4 are dpmpp_2m_coefficients' rows exactly and
    c4 = 0; at eta = 1 a first-order row is DDIM's eta = 1 step."""
    try:
        eta = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"dpmpp_2m_sde_coefficients: eta must be a number in [0, 1], got {eta!r}")
    if not (np.isfinite(eta) and 0.0 <= eta <= 1.0):
        raise ValueError(f"dpmpp_2m_sde_coefficients: eta must be finite and in [0, 1], got {eta!r}")
    a_t = np.asarray(alphas, dtype=np.float64).reshape(-1)
    a_p = np.asarray(alphas_prev, dtype=np.float64).reshape(-1)
    assert a_t.shape == a_p.shape
    S = a_t.shape[0]
    alpha_t, sigma_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    alpha_p, sigma_p = np.sqrt(a_p), np.sqrt(1.0 - a_p)
    h = np.log(alpha_p / sigma_p) - np.log(alpha_t / sigma_t)
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        raise ValueError("dpmpp_2m_sde_coefficients: every step must go to a less noisy state (0 < abar_t < abar_prev < 1)")
    w = np.zeros(S)
    w[1:] = h[1:] / (2.0 * h[:-1])
    if S < LOWER_ORDER_FINAL_BELOW:
        w[S - 1:] = 0.0
    return np.stack([sigma_t, alpha_t, sigma_p / sigma_t * np.exp(-eta * h), -alpha_p * np.expm1(-(1.0 + eta) * h), w,
                     sigma_p * np.sqrt(-np.expm1(-2.0 * eta * h))], 1)


class DPMSolverSampler(SamplerBase):
    ORIGINAL_STEPS = "is not supported (the other samplers refuse it too)"
    STOCHASTIC = False   # DPMSolverSDESampler: the step adds the run's per-step noise, streamed as in ddim_sampling

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__(model, schedule)
        # phi of Lin et al. 2023 (section 3.4), 0: off.  Sampler state, as in PLMSSampler, whose parameter lists this class
        # carries: `sample` sets it on every call from its `guidance_rescale=` keyword (absent: 0), `dpm_sampling` reads it.
        self.guidance_rescale = 0.0
        self.t_start = None   # the same way: `sample` sets it from its `t_start=` keyword (absent: None), `dpm_sampling` reads it
        self.windows = None   # the same way: a windows.window_plan over the long latent (`windows=`), or None
        self.graded = False   # the same way: `mask` is a map of keep levels in [0, 1] (`graded=`)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """DDIM's timestep grid and abar tables at eta = 0 (host side), and the solver's coefficient table for the whole grid."""
        if ddim_eta != 0:
            raise ValueError("ddim_eta must equal 0 for DPM-Solver++(2M): the solver is deterministic")
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.dpm_coef = self._table(len(self.ddim_timesteps))

    def _table(self, total_steps):
        """[total_steps, 5] fp32 rows in loop order for a run over the first `total_steps` grid entries (i = 0 is the noisiest
        step, index = total_steps - 1): fp64 from the fp32 abar values, rounded once."""
        a = np.asarray(self.ddim_alphas, dtype=np.float64)[:total_steps][::-1]
        a_prev = np.asarray(self.ddim_alphas_prev, dtype=np.float64)[:total_steps][::-1]
        return torch.from_numpy(dpmpp_2m_coefficients(a, a_prev)).float()

    def _coef_table(self, n, scale, use_cfg, phi):
        """The run's [n, 8] host table (plan_run's `table`): a sub-range has its own rows (its own first and last step)."""
        return guidance_table(self.dpm_coef if n == self.dpm_coef.shape[0] else self._table(n), scale, use_cfg, phi)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0,
               noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None, **kwargs):
        """PLMSSampler.sample's parameter list; S is the grid parameter of make_ddim_timesteps.  `guidance_rescale` is read from
        **kwargs, as there, and becomes `self.guidance_rescale` for this run."""
        self.guidance_rescale = check_guidance_rescale(kwargs.pop("guidance_rescale", 0.0))
        if kwargs.get("resample") is not None:
            raise ValueError(f"{type(self).__name__}: resample= (resampled inpainting) is DDIM's: the multistep history does not survive a "
                             "jump back to a higher noise level")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        # `t_start` (None or absent: the whole schedule; k: its first k entries, indices k-1 ... 0, from x_T) is read from **kwargs
        # like `guidance_rescale`, and becomes `self.t_start` for this run
        self.t_start = check_t_start(kwargs.pop("t_start", None), kwargs.get("timesteps"), len(self.ddim_timesteps))
        self.windows = kwargs.pop("windows", None)   # the same way: windowed diffusion over the long `shape` (SamplerBase.plan_run)
        self.graded = bool(kwargs.pop("graded", False))   # the same way: `mask` holds keep levels (SamplerBase.plan_run)
        C, H, W = shape
        size = (batch_size, C, H, W)
        return self.dpm_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                 quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                 noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                 corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                     quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.0,
                     noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.0,
                     unconditional_conditioning=None):
        """PLMSSampler.plms_sampling's parameter list and loop structure; guidance rescale: `self.guidance_rescale`; a window plan over
        the long `shape`: `self.windows`."""
        guidance_rescale = check_guidance_rescale(self.guidance_rescale)
        self._refuse(ddim_use_original_steps, quantize_denoised, score_corrector, noise_dropout)
        dev = torch.device("cuda")
        shape = tuple(shape)
        b = shape[0]
        # the host generator: x_T first, then (inpainting only) one q_sample draw per step — nothing else.  The table: a
        # sub-range has its own (its own first and last step)
        plan = self.plan_run(cond, shape, x_T, self.t_start, timesteps,
                             lambda n, cfg: self._coef_table(n, unconditional_guidance_scale, cfg, guidance_rescale),
                             unconditional_guidance_scale, unconditional_conditioning, guidance_rescale, mask, x0, self.windows,
                             graded=self.graded)
        total_steps, use_cfg, rescale, draw, img = plan.total_steps, plan.use_cfg, plan.rescale, plan.draw, plan.img
        cond, unconditional_conditioning = plan.cond, plan.uncond   # tiled W times in a windowed run, else the arguments
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        if total_steps == 0:
            return img, intermediates
        coef, t_tab, prepared = plan.coef, plan.t_tab, plan.prepared

        # static buffers = the inputs of the step graph.  pred_x0 is the solver's history slab: step 0 (w = 0) does not read it
        x_cur, pred_x0 = img.clone(), torch.empty_like(img)
        step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
        t_cur = t_tab[0].clone()
        eps_g = torch.empty_like(img) if rescale else None   # the rescaled combined model output

        blend = plan.win is not None and plan.win.blend
        # the SDE solver: the per-step draws — the q-noise draw first where there is a region to keep, then the step
        # noise, times `temperature` — are streamed into static [total_steps, *shape] device tables the counter indexes, with
        # ddim_sampling's machinery and its rule for callbacks: one that may draw (`uses_rng` not False) keeps the draws on the
        # launching thread, one step at a time
        feed, cb_rng = None, False
        if self.STOCHASTIC:
            cb_rng = any(getattr(f, "uses_rng", True) for f in (callback, img_callback) if f is not None)
            feed = _NoiseFeed(draw, total_steps, shape, mask is not None or blend, temperature, dev,
                              **({"threaded": False, "chunk": 1} if cb_rng else {}))
        qbuf = None
        if blend:
            # a plan with a source: the fused blend-and-gather node reads row step_idx of blend_coef and its q-noise — without a
            # feed the step's draw, staged into this one-row static buffer before the launch (q_rows = 1), else the feed's table
            qbuf = torch.empty_like(img) if feed is None else None
            plan.win.qnoise, plan.win.step_idx = (qbuf if feed is None else feed.qnoise), step_idx
        if plan.win is not None and plan.win.phase is not None:
            # moving window phases: the gather and merge nodes select the step's phase with the counter
            plan.win.step_idx = step_idx
        if plan.compose is not None:
            # composable guidance: the compose node behind the UNet pass selects the step's weights with the counter
            cond.step_idx = step_idx

        def step():
            eps = self.model_output(x_cur, t_cur, b, cond, unconditional_conditioning, use_cfg, prepared, win=plan.win)
            if rescale:
                eps = ops.cfg_rescale_indexed(eps, eps_g, coef, step_idx)
            if feed is None:
                ops.dpmpp_step_indexed(x_cur, eps, pred_x0, coef, step_idx)
            else:
                ops.dpmpp_sde_step_indexed(x_cur, eps, pred_x0, feed.noise, coef, step_idx)
            ops.step_advance(step_idx, t_tab, t_cur)
        run_step = GraphStepper(step, self.use_graph)   # every step: eager once, captured at the next, replayed after
        try:
            if feed is not None:
                feed.produce_next()
            for i in range(total_steps):
                # with a feed the current stream waits for the upload of step i's chunk; nothing else is issued for the noise
                opens_chunk = feed is not None and feed.wait(i)
                if mask is not None:
                    # img = q_sample(x0, ts)*mask + (1-mask)*img, between the replays; its draw comes first
                    if plan.level_d is not None:   # graded keep levels: this step's binary mask from the level map
                        ops.keep_threshold_indexed(plan.level_d, plan.keep_thr[i:i + 1], plan.mask_d)
                    ops.inpaint_blend(x_cur, plan.x0_d, draw().to(dev) if feed is None else feed.qnoise[i], plan.mask_d,
                                      plan.blend_coef[i])
                if qbuf is not None:
                    qbuf.copy_(draw())   # the same draw; the blend itself is a node of the step
                run_step()
                if opens_chunk and not cb_rng:
                    feed.produce_next()   # (unthreaded mode only) draw + upload the NEXT chunk while the GPU works on this one
                log_step(i, total_steps, log_every_t, x_cur, pred_x0, intermediates, callback, img_callback)
        finally:
            if feed is not None:
                feed.close()   # the generator is past the run's last draw before anyone else draws from it
        out = x_cur.clone()
        torch.cuda.synchronize()   # no replay in flight
        run_step.release()
        return out, intermediates


class DPMSolverSDESampler(DPMSolverSampler):
    """DPM-Solver++(2M) SDE (module docstring, "SDE"; `sampler="dpmpp_2m_sde"`): DPMSolverSampler's parameter lists, keywords, run
    plan and loop — one body, `dpm_sampling` — with 0 < eta <= 1, a sixth coefficient c4 in column 8 of the run's table and the
    per-step noise of DDIM's contract.  eta = 0 is DPMSolverSampler."""
    STOCHASTIC = True

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """DDIM's timestep grid and abar tables (host side), and the solver's [S, 6] coefficient rows at eta = ddim_eta."""
        try:
            eta = float(ddim_eta)
        except (TypeError, ValueError):
            eta = float("nan")
        if not 0.0 < eta <= 1.0:
            raise ValueError(f"ddim_eta = {ddim_eta!r}: DPM-Solver++(2M) SDE needs 0 < ddim_eta <= 1; eta = 0 is sampler='dpmpp_2m'")
        SamplerBase.make_schedule(self, ddim_num_steps, ddim_discretize, eta, verbose)
        self.eta = eta
        self.dpm_coef = self._table(len(self.ddim_timesteps))

    def _table(self, total_steps):
        """[total_steps, 6] fp32 rows {sigma_t, alpha_t, c2, c3, w, c4} in loop order for a run over the first `total_steps` grid
        entries: fp64 from the fp32 abar values, rounded once."""
        a = np.asarray(self.ddim_alphas, dtype=np.float64)[:total_steps][::-1]
        a_prev = np.asarray(self.ddim_alphas_prev, dtype=np.float64)[:total_steps][::-1]
        return torch.from_numpy(dpmpp_2m_sde_coefficients(a, a_prev, self.eta)).float()

    def _coef_table(self, n, scale, use_cfg, phi):
        """The run's [n, 9] host table: guidance_table over the first five columns of the rows, c4 appended as column 8."""
        rows = self.dpm_coef if n == self.dpm_coef.shape[0] else self._table(n)
        return torch.cat([guidance_table(rows[:, :5], scale, use_cfg, phi), rows[:, 5:6]], 1).contiguous()
