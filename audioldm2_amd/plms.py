"""PLMS sampler on MI355X: counterpart of `audioldm2.latent_diffusion.models.plms.PLMSSampler` (models/plms.py:14-360).  Same
constructor / `sample()` / `plms_sampling()` / `p_sample_plms()` signatures and return values; constructed by name in
`LatentDiffusion.sample_log(use_plms=True)` (ddpm.py:1449-1461).

PLMS is a pseudo linear multistep method over DDIM's eta = 0 update: step 0 is a pseudo improved Euler step (two UNet passes), every
later step combines its model output with up to three earlier ones (Adams-Bashforth weights, plms.py:346-356) and costs ONE pass.

On MI355X:
  * guidance combine + multistep combine + x0 prediction + x_{t-1} update + the history update are one kernel per step
    (ops.plms_step_indexed; step 0: ops.plms_first_step, twice);
  * the history is a ring of three slabs whose slots follow the device-side step counter, so steps >= 1 are ONE launch sequence:
    UNet pass -> plms_step_indexed -> step_advance, captured once into a HIP graph on one stream and replayed (sampling.GraphStepper);
    step 0 runs eagerly.  The graph lives for one sampling run: nothing is read from or written to the UNet's DDIM graph cache;
  * RNG contract: the reference's `get_x_prev_and_pred_x0` draws `noise_like(x.shape)` every time it runs although
    sigma = 0 multiplies the result away (plms.py:334) — two draws in step 0, one in every later step, after the q_sample draw of an
    inpainting step and after x_T.  They are made on the host generator, in that order, on the launching thread, and discarded: the
    next consumer of the generator sees the state the reference leaves.

The schedule, the run plan and the UNet pass come from sampling.SamplerBase, shared with DDIMSampler and DPMSolverSampler; this module
keeps what is PLMS's own: the eager step 0, the ring, the discarded draws.

Stated deviations: with guidance the reference concatenates the two conditionings with `torch.cat` (plms.py:290),
which raises for AudioLDM2's dict conditioning; here guidance runs as in DDIMSampler — one pass over [uncond ; cond], e_u + s (e_c -
e_u).  `make_schedule` raises ValueError for eta != 0 where the reference as shipped sets eta to 0 silently (plms.py:30-32).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .sampling import GraphStepper, SamplerBase, check_guidance_rescale, check_t_start, ddim_step_rows, guidance_table, log_step


class PLMSSampler(SamplerBase):
    # p_sample_plms reads `self.model.ddim_sigmas_for_original_num_steps` there (plms.py:313-317), a buffer make_schedule registered on
    # the SAMPLER (plms.py:87-89): with LatentDiffusion as the model this path raises AttributeError in the reference itself, so
    # there is no behaviour to reproduce
    ORIGINAL_STEPS = "is not runnable in the reference either (plms.py:313-317 reads a buffer the model does not have)"

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__(model, schedule)
        self.t_start = None   # sampler state like guidance_rescale: `sample` sets it on every call, `plms_sampling` reads it
        self.windows = None   # the same way: a windows.window_plan over the long latent (`windows=`), or None
        self.graded = False   # the same way: `mask` is a map of keep levels in [0, 1] (`graded=`)
        # phi of Lin et al. 2023 (section 3.4), 0: off.  Sampler state like the schedule, not a parameter: `plms_sampling` and
        # `p_sample_plms` keep the reference class's signatures, which have no **kwargs to take it.  `sample` sets it on every
        # call from its `guidance_rescale=` keyword (absent: 0); a caller of the two other methods sets the attribute.
        self.guidance_rescale = 0.0

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """plms.py:27-89 (host side, float tables only): DDIM's schedule at eta = 0."""
        if ddim_eta != 0:
            raise ValueError("ddim_eta must equal 0 for PLMS")
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)
        self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1.0 - self.ddim_alphas.numpy()))
        self.plms_coef = ddim_step_rows(self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev,
                                        self.ddim_sqrt_one_minus_alphas)  # [S, 5] fp32 (host)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0,
               noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None, **kwargs):
        """plms.py:91-154; `guidance_rescale` (phi of Lin et al. 2023; 0 or absent: off — the reference's step) is read from
        **kwargs, so the signature stays the reference's, and becomes `self.guidance_rescale` for this run"""
        self.guidance_rescale = check_guidance_rescale(kwargs.pop("guidance_rescale", 0.0))
        if kwargs.get("resample") is not None:
            raise ValueError("PLMSSampler: resample= (resampled inpainting) is DDIM's: the multistep history does not survive a jump "
                             "back to a higher noise level")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        # `t_start` (None or absent: the whole schedule; k: its first k entries, indices k-1 ... 0, from x_T) is read from **kwargs
        # like `guidance_rescale`, and becomes `self.t_start` for this run
        self.t_start = check_t_start(kwargs.pop("t_start", None), kwargs.get("timesteps"), len(self.ddim_timesteps))
        self.windows = kwargs.pop("windows", None)   # the same way: windowed diffusion over the long `shape` (SamplerBase.plan_run)
        self.graded = bool(kwargs.pop("graded", False))   # the same way: `mask` holds keep levels (SamplerBase.plan_run)
        C, H, W = shape
        size = (batch_size, C, H, W)
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.0,
                      noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None):
        """plms.py:156-258; guidance rescale: `self.guidance_rescale`; a window plan over the long `shape`: `self.windows`"""
        guidance_rescale = check_guidance_rescale(self.guidance_rescale)
        self._refuse(ddim_use_original_steps, quantize_denoised, score_corrector, noise_dropout)
        dev = torch.device("cuda")
        shape = tuple(shape)
        b = shape[0]
        # RNG contract R: x_T first, then the per-step draws, all from the host generator on this thread in the reference's order.
        # The table: the schedule's rows total_steps-1 ... 0; with guidance rescale the history ring holds the rescaled e_t
        plan = self.plan_run(cond, shape, x_T, self.t_start, timesteps,
                             lambda n, cfg: guidance_table(self.plms_coef[:n].flip(0), unconditional_guidance_scale, cfg,
                                                           guidance_rescale),
                             unconditional_guidance_scale, unconditional_conditioning, guidance_rescale, mask, x0, self.windows,
                             graded=self.graded)
        total_steps, use_cfg, rescale, draw, img = plan.total_steps, plan.use_cfg, plan.rescale, plan.draw, plan.img
        cond, unconditional_conditioning, win = plan.cond, plan.uncond, plan.win   # tiled W times in a windowed run
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        if total_steps == 0:
            return img, intermediates
        coef, t_tab, prepared = plan.coef, plan.t_tab, plan.prepared

        # static buffers = the inputs of the step graph
        x_cur, pred_x0 = img.clone(), torch.empty_like(img)
        hist = torch.zeros((3,) + shape, device=dev, dtype=torch.float32)   # model outputs of the last three steps, slot = step % 3
        step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
        t_cur = t_tab[0].clone()
        eps_g = torch.empty_like(img) if rescale else None   # the rescaled combined model output of the replayed step

        qbuf = None
        if win is not None and win.blend:
            # a plan with a source: the step's q-noise draw is staged into this one-row static buffer before the launch; the
            # fused blend-and-gather of the step's first pass reads it (q_rows = 1) and row step_idx of blend_coef
            qbuf = torch.empty_like(img)
            win.qnoise, win.step_idx = qbuf, step_idx
        if win is not None and win.phase is not None:
            # moving window phases: every pass's gather and merge select the step's phase with the counter (both passes of the
            # eager step 0 run under row 0: the counter advances after them)
            win.step_idx = step_idx
        if plan.compose is not None:
            # composable guidance: the compose launch behind every pass selects the step's weights with the counter (both passes of
            # the eager step 0 read row 0: the counter advances after them, as for cfg_rescale_indexed)
            cond.step_idx = step_idx

        def guided_eps(x, t_row, out=None, idx=None, first_pass=True):
            """eps [2, b, ...] for the step kernel to combine, or with rescale the combined and rescaled [b, ...] (row: the
            counter's, or row 0 — the step's row in the eager calls of step 0).  The eager calls (idx is None) keep their
            results side by side: a windowed run merges them into fresh tensors, not the step graph's static one"""
            eps = self.model_output(x, t_row, b, cond, unconditional_conditioning, use_cfg, prepared, win=win,
                                    static=idx is not None, first_pass=first_pass)
            if not rescale:
                return eps
            return ops.cfg_rescale_indexed(eps, torch.empty_like(img) if out is None else out, coef, idx)

        def step():
            eps = guided_eps(x_cur, t_cur, eps_g, step_idx)
            ops.plms_step_indexed(x_cur, eps, hist, coef, step_idx, pred_x0)
            ops.step_advance(step_idx, t_tab, t_cur)
        run_step = GraphStepper(step, self.use_graph)   # steps >= 1: eager once, captured at the next, replayed after
        for i in range(total_steps):
            if mask is not None:
                # img = q_sample(x0, ts)*mask + (1-mask)*img   (plms.py:222-227, ddpm.py:430-436); its draw comes first
                if plan.level_d is not None:   # graded keep levels: this step's binary mask from the level map
                    ops.keep_threshold_indexed(plan.level_d, plan.keep_thr[i:i + 1], plan.mask_d)
                ops.inpaint_blend(x_cur, plan.x0_d, draw().to(dev), plan.mask_d, plan.blend_coef[i])
            if qbuf is not None:
                qbuf.copy_(draw())   # the same draw, first in the step; the blend itself runs inside the step's first pass
            if i == 0:
                # pseudo improved Euler (plms.py:341-345): provisional x_prev from e_t, a second pass at (x_prev, t_next)
                e_t = guided_eps(x_cur, t_cur)
                x_tmp, _ = ops.plms_first_step(x_cur, e_t, None, coef[0])
                draw()                                                   # the noise_like of the provisional update
                t_next = t_tab[min(1, total_steps - 1)]
                e_next = guided_eps(x_tmp, t_next, first_pass=False)   # on the provisional x_prev: a plain gather, no blend
                ops.plms_first_step(x_cur, e_t, e_next, coef[0], x_out=x_cur, pred_x0=pred_x0, hist=hist)
                ops.step_advance(step_idx, t_tab, t_cur)
                del e_t, e_next, x_tmp
            else:
                run_step()
            draw()   # the step's noise_like (plms.py:334): consumed after the launch, while the GPU works
            log_step(i, total_steps, log_every_t, x_cur, pred_x0, intermediates, callback, img_callback)
        out = x_cur.clone()
        torch.cuda.synchronize()   # no replay in flight
        run_step.release()
        return out, intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, old_eps=None, t_next=None):
        """plms.py:260-360 — one eager step with the reference's signature: returns (x_prev, pred_x0, e_t); the caller keeps the
        Python list `old_eps` (oldest first, at most the last three are read).  The same kernels as plms_sampling; the noise
        draws come from the host generator like `noise_like` on a CPU reference run, and are discarded (sigma = 0)."""
        self._refuse(use_original_steps, quantize_denoised, score_corrector, noise_dropout)
        guidance_rescale = check_guidance_rescale(self.guidance_rescale)
        b = x.shape[0]
        use_cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
        rescale = use_cfg and guidance_rescale > 0.0
        x = x.float().contiguous()
        coef = guidance_table(self.plms_coef[index].reshape(1, 5).repeat(4, 1), unconditional_guidance_scale, use_cfg,
                              guidance_rescale).to(x.device)
        nrep = 2 if use_cfg else 1

        def noise_like():
            torch.randn((1, *x.shape[1:])) if repeat_noise else torch.randn(x.shape)

        def guided_eps(xx, tt):
            eps = self.model_output(xx, tt.float().repeat(nrep), b, c, unconditional_conditioning, use_cfg, None)
            return ops.cfg_rescale_indexed(eps, torch.empty_like(x), coef) if rescale else eps
        e_t = guided_eps(x, t)
        hist = torch.zeros((3,) + tuple(x.shape), device=x.device, dtype=torch.float32)
        old_eps = list(old_eps or [])[-3:]
        k = len(old_eps)
        if k == 0:
            x_tmp, _ = ops.plms_first_step(x, e_t, None, coef[0])
            noise_like()
            e_next = guided_eps(x_tmp, t_next)
            x_prev, pred_x0 = ops.plms_first_step(x, e_t, e_next, coef[0], hist=hist)
        else:
            # the ring as the sampling loop would hold it at step k: the j-th newest entry in slot (k - j) % 3
            for j in range(1, k + 1):
                hist[(k - j) % 3].copy_(old_eps[-j])
            x_prev, pred_x0 = x.clone(), torch.empty_like(x)
            ops.plms_step_indexed(x_prev, e_t, hist, coef, torch.full((1,), k, device=x.device, dtype=torch.int32), pred_x0)
        noise_like()
        return x_prev, pred_x0, hist[k % 3].clone()   # e_t after the guidance combine, as the kernel stored it
