"""Shared by tests/test_timeline_cpu.py and tests/test_timeline_gpu.py (prompt timelines): the grid of row plans with
the row counts worked out by hand from the definitions, an independent fp64 restatement of the prompt and row weights, the kernel
cases, and the composition loops of windowed sampling under a timeline — a model wrapper that slices the rows of the long latent,
runs the SAME model on them under per-row conditioning and merges in fp64, stepped by each sampler's existing eager single-step form
(tests/windowed.py, tests/long_source.py).

The merge kernel's bar is tests/windowed.py's with the ROW cover: an output element is a sum over at most `cover` rows of non-zero
weight, one rounding per term, each at most 2^-24 of the sum of the magnitudes: cover * 2^-24.
"""
from types import SimpleNamespace

import numpy as np
import torch

import audio2audio as A
import long_source as Ls
import windowed as Wd

# ((T, Tw, hop), boundaries, transition) -> (R, cover or None where the issue leaves it open)
ROW_GRID = [((40, 16, 10), [12, 28], 4, 8, 4), ((40, 16, 10), [12, 28], 0, 8, 3), ((40, 16, 10), [13.5], 6, 6, None),
            ((24, 16, 1), [12], 8, 18, 18), ((48, 16, 16), [16, 32], 0, 3, 1), ((48, 16, 16), [16, 32], 4, 7, None),
            ((768, 256, 192), [256, 512], 64, 8, None), ((3072, 256, 192), [256 * i for i in range(1, 12)], 64, 35, None)]

# kernel cases (B, (T, Tw, hop), boundaries, transition, C, F): F = 5 and 7 take the scalar path and rows of 7 floats straddle the
# waves; (768, 256, 192) is the 30 s shape on the 16-byte path; the last has 35 rows, past the 32 of aldm_window_starts
KERNEL_CASES = [(2, (40, 16, 10), [12, 28], 4, 3, 5), (1, (24, 16, 1), [12], 8, 2, 7), (1, (768, 256, 192), [256, 512], 64, 8, 16),
                (1, (3072, 256, 192), [256 * i for i in range(1, 12)], 64, 1, 4)]


def case_id(c):
    B, key, bounds, tau, C, F = c
    return f"B{B}-T{key[0]}w{key[1]}h{key[2]}-K{len(bounds) + 1}tau{tau}-C{C}-F{F}"


def plans_of(key, bounds, tau):
    """(base plan, row plan)."""
    from audioldm2_amd.windows import prompt_weights, row_plan, window_plan
    base = window_plan(*key)
    return base, row_plan(base, prompt_weights(key[0], bounds, tau))


def weights_fp64(key, bounds, tau):
    """The definitions restated with Python floats, frame by frame: (m [K][T], rows [(j, k)], wr64 [R][Tw], starts)."""
    T, Tw, hop = key
    starts, s = [], 0
    while s + Tw < T:
        starts.append(s)
        s += hop
    starts.append(T - Tw)
    K = len(bounds) + 1

    def u(k, t):
        if k == 0:
            return 1.0
        if k == K:
            return 0.0
        if tau > 0:
            return min(1.0, max(0.0, (t + 0.5 - bounds[k - 1]) / tau + 0.5))
        return 1.0 if t + 0.5 >= bounds[k - 1] else 0.0
    m = [[u(k, t) - u(k + 1, t) for t in range(T)] for k in range(K)]
    ramp = Tw - hop
    taper = [min(1.0, (p + 1.0) / (ramp + 1.0), (Tw - p) / (ramp + 1.0)) for p in range(Tw)]
    rows = [(j, k) for j, s in enumerate(starts) for k in range(K) if any(m[k][s + p] != 0.0 for p in range(Tw))]
    norm = [0.0] * T
    for j, k in rows:
        for p in range(Tw):
            norm[starts[j] + p] += taper[p] * m[k][starts[j] + p]
    wr = [[taper[p] * m[k][starts[j] + p] / norm[starts[j] + p] for p in range(Tw)] for j, k in rows]
    return m, rows, wr, starts


def as_window_plan(rp):
    """A row plan seen as a plain plan of R windows (starts = row starts, wn = wr): what tests/windowed.py's torch restatements
    (gather_ref, merge_fp64) take."""
    return SimpleNamespace(T=rp.T, Tw=rp.Tw, W=rp.R, starts=rp.row_starts, wn=rp.wr, cover=rp.cover)


def row_inputs(B, rp, C, F, H=None, seed=0):
    """fp32 host tensors of one case: x [B, C, T, F] and win [(H,) R*B, C, Tw, F], N(0, 1)."""
    return Wd.window_inputs(B, as_window_plan(rp), C, F, H=H, seed=seed)


def bar(rp):
    return rp.cover * 2.0 ** -24


def rows_cond_ref(conds, rp):
    """Per-row conditioning by hand (tensors inside lists, tuples and dicts): row r*b + i = prompt k_r's sample i."""
    def cat(cs):
        if torch.is_tensor(cs[0]):
            return torch.cat(cs)
        if isinstance(cs[0], dict):
            return {key: cat([c[key] for c in cs]) for key in cs[0]}
        return type(cs[0])(cat([c[n] for c in cs]) for n in range(len(cs[0])))
    return cat([conds[k] for k in rp.row_prompt])


class TimelineModel:
    """windowed.WindowedModel under a timeline: slice the R rows of the long latent, run the same model under per-row conditioning
    (`cond` is the list of the K prompts' conditionings; the unconditional one is tiled R times), merge in fp64 with the row
    weights, round to fp32."""

    def __init__(self, inner, rp):
        self.inner, self.rp, self.wp = inner, rp, as_window_plan(rp)
        self.num_timesteps, self.alphas_cumprod = inner.num_timesteps, inner.alphas_cumprod

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        assert prepared is None
        R, b = self.rp.R, x.shape[0]
        xw = Wd.gather_ref(x.float(), self.wp)
        eps = self.inner.apply_model_cfg(xw, t2[:1].float().repeat(2 * R * b), rows_cond_ref(cond, self.rp), Wd.tile(uncond, R))
        return Wd.merge_fp64(eps, self.wp)[0].float().contiguous()


def _coef(sampler, step):
    return float(sampler.sqrt_alphas_cumprod[int(step)]), float(sampler.sqrt_one_minus_alphas_cumprod[int(step)])


def ddim_loop(inner, rp, x_T, conds, uncond, S, gs, guidance_rescale=0.0, k=None, source=None, eta=0.0):
    """DDIMSampler.p_sample_ddim per step over the timeline model (it draws the step noise); `source` = (x0, mask): the q-noise
    draw (host generator) and the torch blend on the long latent in front of every step, as long_source.ddim_source_loop."""
    from audioldm2_amd.ddim import DDIMSampler
    s = DDIMSampler(TimelineModel(inner, rp))
    s.make_schedule(S, ddim_eta=eta, verbose=False)
    k = len(s.ddim_timesteps) if k is None else k
    x = x_T.cuda()
    for i, step in enumerate(np.flip(s.ddim_timesteps[:k])):
        if source is not None:
            sa, so = _coef(s, step)
            x = Ls.torch_blend(x, source[0].cuda(), torch.randn(x.shape).cuda(), source[1].cuda(), sa, so)
        ts = torch.full((x.shape[0],), int(step), device="cuda", dtype=torch.long)
        x, _ = s.p_sample_ddim(x, conds, ts, index=k - i - 1, unconditional_guidance_scale=gs, unconditional_conditioning=uncond,
                               guidance_rescale=guidance_rescale)
    return x


def plms_loop(inner, rp, x_T, conds, uncond, steps):
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(TimelineModel(inner, rp))
    s.make_schedule(steps, verbose=False)
    return A.plms_eager_loop(s, x_T.cuda(), conds, uncond, steps)


def dpmpp_loop(inner, rp, x_T, conds, uncond, steps):
    from audioldm2_amd.sampling import make_ddim_timesteps
    tm = TimelineModel(inner, rp)
    b = x_T.shape[0]
    model_cfg = lambda xx, t: tm.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), conds, uncond)
    ts = make_ddim_timesteps("uniform", steps, inner.num_timesteps, verbose=False)
    return A.dpmpp_fp64_loop(model_cfg, inner.alphas_cumprod, ts[:steps], x_T)
