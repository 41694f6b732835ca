"""Shared helpers of tests/test_dpmpp_sde_cpu.py and tests/test_dpmpp_sde_gpu.py (the DPM-Solver++(2M) SDE sampler):
the coefficient rows restated in plain Python floats, the step formula in the kernel's operation order, the tiny-UNet fixture, the
host draws in the contract's order and the fp64 sampling loop the sampler is compared with.  No test lives here."""
import math

import numpy as np
import torch

GS = 3.5
TINY_SHAPE = (2, 8, 16, 8)
NUM_TIMESTEPS = 1000


def alphas_cumprod():
    """The fp32 `alphas_cumprod` buffer of the audioldm2-full schedule (sqrt-linear betas, 0.0015 ... 0.0195)."""
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, NUM_TIMESTEPS, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, 0).float()


class ScheduleOnly:
    """What make_schedule reads on its model."""
    num_timesteps = NUM_TIMESTEPS
    alphas_cumprod = alphas_cumprod()


def project_grid(S, ac=None):
    """abar_t / abar_prev of the project's `uniform` grid in step order (noisiest first), as the samplers use them -> fp64 arrays."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    ac = (alphas_cumprod() if ac is None else ac).double().numpy()
    ts = make_ddim_timesteps("uniform", S, NUM_TIMESTEPS, verbose=False)
    a, a_prev = ac[ts], np.concatenate([ac[:1], ac[ts[:-1]]])
    return a[::-1].copy(), a_prev[::-1].copy()


def uneven_grid():
    """A hand-made descending-noise abar sequence with uneven steps (so w varies) -> (abar_t, abar_prev), 16 steps."""
    a = [0.004, 0.01, 0.013, 0.05, 0.07, 0.2, 0.21, 0.3, 0.5, 0.52, 0.6, 0.8, 0.83, 0.9, 0.97, 0.99, 0.9991]
    return np.asarray(a[:-1]), np.asarray(a[1:])


def rows_py(a_t, a_p, eta):
    """The issue's formulas, one step at a time in plain Python floats (no vector code shared with the builder) ->
    [S][6] = {sigma_t, alpha_t, c2, c3, w, c4}."""
    S, rows, h_last = len(a_t), [], None
    for i in range(S):
        at, ap = float(a_t[i]), float(a_p[i])
        al_t, sg_t, al_p, sg_p = math.sqrt(at), math.sqrt(1.0 - at), math.sqrt(ap), math.sqrt(1.0 - ap)
        h = math.log(al_p / sg_p) - math.log(al_t / sg_t)
        first = i == 0 or (i == S - 1 and S < 15)
        w = 0.0 if first else 1.0 / (2.0 * (h_last / h))
        rows.append([sg_t, al_t, (sg_p / sg_t) * math.exp(-eta * h), -al_p * math.expm1(-(1.0 + eta) * h), w,
                     sg_p * math.sqrt(-math.expm1(-2.0 * eta * h))])
        h_last = h
    return rows


def step_rows(ac, ts, eta):
    """fp64 rows over the ascending timestep subset `ts` of the fp32 schedule `ac`, in loop order (a run of its own: its first
    step, and its last when it has fewer than 15, are first order)."""
    n = len(ts)
    a_t = [float(ac[ts[n - 1 - i]]) for i in range(n)]
    a_p = [float(ac[ts[n - 2 - i]]) if n - 1 - i > 0 else float(ac[0]) for i in range(n)]
    return torch.tensor(rows_py(a_t, a_p, eta), dtype=torch.float64)


# ---- the step, in the kernel's operation order ------------------------------------------------------------------------------------
def sde_formula(x, e, old, z, c, dt):
    """One step on tensors of dtype dt; c = {sigma_t, alpha_t, c2, c3, w, c4} as 0-dim tensors; e is the combined model output.
    Returns (x_new, x0)."""
    x, e = x.to(dt), e.to(dt)
    c = [v.to(dt) for v in c]
    p0 = (x - c[0] * e) / c[1]
    d = p0 if float(c[4]) == 0.0 else p0 + c[4] * (p0 - old.to(dt))
    xn = c[2] * x + c[3] * d
    if float(c[5]) != 0.0:
        xn = xn + c[5] * z.to(dt)
    return xn, p0


def combine(eps, cfg, dt, gs=GS, phi=0.0):
    """The guidance combine of eps [2, b, ...] (cfg) in dtype dt, with guidance rescale phi (per sample, Lin et al. 2023, 3.4)."""
    eps = eps.to(dt)
    if not cfg:
        return eps
    e = eps[0] + gs * (eps[1] - eps[0])
    if phi > 0.0:
        dims = tuple(range(1, e.dim()))
        f = phi * eps[1].std(dims, keepdim=True) / e.std(dims, keepdim=True) + (1.0 - phi)
        e = f * e
    return e


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


def rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))


def rel_rms(a, ref):
    a, ref = a.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    return rms(a - ref) / rms(ref)


def kernel_table(S, cfg, eta, seed=0, gs=GS):
    """[S, 9] fp32 rows of aldm_dpmpp_sde_step_indexed from a decreasing-noise abar sequence with uneven steps -> (fp32 table,
    the [S, 6] rows it was rounded from)."""
    from audioldm2_amd.dpm_solver import dpmpp_2m_sde_coefficients
    a = torch.linspace(0.05, 0.95, S + 1, dtype=torch.float64) + \
        0.01 * torch.rand(S + 1, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    rows = torch.from_numpy(dpmpp_2m_sde_coefficients(a[:-1].numpy(), a[1:].numpy(), eta)).float()
    tab = torch.zeros(S, 9)
    tab[:, :5] = rows[:, :5]
    tab[:, 5], tab[:, 6], tab[:, 8] = gs, 1.0 if cfg else 0.0, rows[:, 5]
    return tab, rows


# ---- the tiny UNet ----------------------------------------------------------------------------------------------------------------
class TinyModel:
    """What a sampler touches on its model (num_timesteps, alphas_cumprod, apply_model, prepare_cfg, apply_model_cfg) over the tiny
    UNet (cases.UNET_TINY); conditioning = (contexts, masks)."""
    num_timesteps = NUM_TIMESTEPS

    def __init__(self):
        from audioldm2_amd.unet import UNetModel
        from oracle import cases, weights
        self.unet = UNetModel(**cases.UNET_TINY)
        self.unet.load_state_dict(weights.make_state_dict(weights.shapes_of(self.unet), seed=0))
        self.unet.cuda()
        self.alphas_cumprod = alphas_cumprod()

    def apply_model(self, x, t, cond):
        return self.unet(x.contiguous(), t, context_list=cond[0], context_attn_mask_list=cond[1])

    def prepare_cfg(self, cond, uncond):
        return {"ctxs": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[0], cond[0])],
                "masks": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[1], cond[1])]}

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        p = prepared or self.prepare_cfg(cond, uncond)
        eps = self.unet(x.repeat(2, 1, 1, 1).contiguous(), t2, context_list=p["ctxs"], context_attn_mask_list=p["masks"])
        return eps.view(2, x.shape[0], *eps.shape[1:])


def tiny_conditioning():
    from oracle import cases
    B = TINY_SHAPE[0]
    _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=1)
    _, _, uctx, umask, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=2)
    return ([c.cuda() for c in ctxs], [k.cuda() for k in masks]), ([c.cuda() for c in uctx], [k.cuda() for k in umask])


def tiny_model_cfg(m, cond, uncond):
    b = TINY_SHAPE[0]
    return lambda xx, t: m.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), cond, uncond)


def x_T(seed=3, shape=TINY_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- the draws and the loop -------------------------------------------------------------------------------------------------------
def host_draws(seed, shape, steps, with_q, draw_x_T=False):
    """What a run consumes from the host generator seeded with `seed`, in the contract's order: x_T first (when the run draws
    it), then per step the q-noise draw (a mask or a source) and the step noise -> (x_T or None, [q or None] * steps, [z] * steps)."""
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    xT = torch.randn(shape) if draw_x_T else None
    q, z = [], []
    for _ in range(steps):
        q.append(torch.randn(shape) if with_q else None)
        z.append(torch.randn(shape))
    torch.set_rng_state(state)
    return xT, q, z


def fp64_loop(model_cfg, ac, ts, xT, eta, z, gs=GS, phi=0.0, mask=None, x0=None, q=None, temperature=1.0, level=None):
    """DPM-Solver++(2M) SDE over the ascending timestep subset `ts` of the fp32 schedule `ac`: eps from model_cfg(x fp32, t) ->
    [2, b, ...] on the fp32 image of the fp64 state, every other operation in fp64 with unrounded coefficients; z[i] (and, with a
    mask, q[i] for the blend in front of the step) are the run's host draws.  `level`: a map of keep levels in the mask's place —
    step i blends under level > sampling.keep_thresholds(steps)[i].  Returns x, the last x0 and the worst per-step error of the
    same step evaluated by torch in fp32 with the coefficients rounded to fp32 (the yardstick of the bars)."""
    rows = step_rows(ac, ts, eta)
    time_range = np.flip(ts)
    x = xT.double().cuda()
    old, p0, e32 = None, None, 0.0
    for i, t in enumerate(time_range):
        x_32 = x.float()
        if level is not None:
            from audioldm2_amd.sampling import keep_thresholds
            mask = (level.float().cpu() > keep_thresholds(len(ts))[i]).float()
        if mask is not None:
            a = float(ac[int(t)])
            m64, s64 = mask.double().cuda(), x0.double().cuda()
            x = (math.sqrt(a) * s64 + math.sqrt(1.0 - a) * q[i].double().cuda()) * m64 + (1.0 - m64) * x
            sa, so = torch.tensor(a).sqrt(), (1.0 - torch.tensor(a)).sqrt()
            m32 = mask.float().cuda()
            x_32 = (sa * x0.float().cuda() + so * q[i].cuda()) * m32 + (1.0 - m32) * x_32
        eps = model_cfg(x.float(), float(t))
        zi = (z[i] * temperature).cuda()
        x_new, p0 = sde_formula(x, combine(eps, True, torch.float64, gs, phi), old, zi, [rows[i, j] for j in range(6)], torch.float64)
        x_f32, _ = sde_formula(x_32, combine(eps, True, torch.float32, gs, phi), old, zi, [rows[i, j].float() for j in range(6)],
                               torch.float32)
        e32 = max(e32, relmax(x_f32, x_new))
        old, x = p0, x_new
    return x, p0, e32
