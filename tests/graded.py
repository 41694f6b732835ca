"""Shared by tests/test_graded_cpu.py and tests/test_graded_gpu.py (graded keep levels, differential diffusion): the
tables of the issue, the kernel's cases, the level maps of the sampler tests, and the composition loops of a graded run — the
loops of tests/long_source.py and tests/resample.py with ONE change: per step the torch blend is fed the binary mask
(level > keep_thresholds(S)[i]).float() instead of a fixed one.  The draws are made by hand in contract order (q-noise first).

The kernel has no rounding: its output is a comparison, so the bar against torch's `(level > thr).float()` is bitwise equality.
"""
import numpy as np
import torch

import audio2audio as A
import long_source as Ls
import resample as Rs

# ---- the tables of the issue -----------------------------------------------------------------------------------------------------
LEVEL_TABLE = [
    ((12, [(2, 5)], 3, False), [.5, .75, 1, 1, 1, .75, .5, .25, 0, 0, 0, 0]),
    ((12, [(2, 5)], 3, True), [.5, .75, 1, 1, 1, .75, .5, .25, 0, 0, 0, .25]),
    ((12, [(0, 4), (8, 12, .5)], 1, False), [1, 1, 1, 1, .5, 0, 0, .25, .5, .5, .5, .5]),
    ((8, [(0, 2), (5, 8, .5)], 3, False), [1, 1, .75, .5, .375, .5, .5, .5]),
]
SIXTH = np.float32(1.0 / 6.0)
HOLD_TABLE = [(0.0, 6, 0), (.25, 6, 2), (.5, 6, 3), (.75, 6, 5), (1.0, 6, 6), (SIXTH, 6, 1),
              (np.nextafter(SIXTH, np.float32(1.0)), 6, 2), (0.3, 200, 60)]
HOLD_GRID = [(S, k / 8.0) for S in (2, 3, 6, 7, 50, 200) for k in range(9)]
THRESHOLD_NUMERATORS_6_2_2 = [0, 1, 2, 3, 2, 2, 3, 4, 5, 4, 4, 5]


def hold_steps_literal(level, S):
    """The documented meaning of a level, as a loop: the steps i < S whose threshold float32(i / S) lies strictly below float32(level)."""
    return sum(1 for i in range(S) if np.float32(level) > np.float32(np.float64(i) / np.float64(S)))


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
KERNEL_N = Rs.KERNEL_N          # 3 and 1021: the scalar path; 8*8*40*5 and 1*8*768*16: the 16-byte one
KERNEL_THR = [0.0, 0.25, float(np.float32(5.0 / 6.0))]   # three distinct rows: the first, an exact one, a rounded one
COUNTERS = [(0, 0), (1, 1), (2, 2), (None, 0), (len(KERNEL_THR) + 5, 2), (-3, 0)]   # (counter, the row it must select)


def kernel_inputs(n, seed=0):
    """fp32 host tensors: levels [n], uniform in [0, 1) with planted values at seeded places — 0, 1, each row's threshold itself,
    the floats just above and just below it, -0.0, 2.0, -1.0, NaN (with n = 3: as many as fit, the thresholds first) — and the
    threshold table [3]."""
    g = torch.Generator().manual_seed(seed)
    level = torch.rand(n, generator=g)
    thr = torch.tensor(KERNEL_THR, dtype=torch.float32)
    t32 = thr.numpy()
    planted = list(t32) + [np.nextafter(t, np.float32(2.0)) for t in t32] + [np.nextafter(t, np.float32(-2.0)) for t in t32] \
        + [0.0, 1.0, -0.0, 2.0, -1.0, float("nan")]
    where = torch.randperm(n, generator=g)[:len(planted)].tolist()
    for i, v in zip(where, planted):
        level[i] = float(v)
    return level, thr


# ---- level maps of the sampler tests ------------------------------------------------------------------------------------------------
FEATHER = 3
TINY_KEEP = [(0, 3), (11, 14, .5)]


def tiny_levels():
    from audioldm2_amd.windows import keep_levels
    lv = keep_levels(A.TINY_SHAPE[2], TINY_KEEP, FEATHER)
    assert {0.0, .25, .5, .75, 1.0} <= set(lv.tolist())
    return lv


def long_levels(plan, ring=False):
    """Levels over the long latent of tests/long_source.py: a kept head whose feathered edge (.75, .5, .25) falls inside a window
    overlap of the linear `plan` (Ls.overlap_interval; the ring and the row plan of the same key overlap there too), and a
    half-kept interval further on.  ring=True: the fades go round the circle."""
    from audioldm2_amd.windows import keep_levels
    a, b = Ls.overlap_interval(plan)
    lv = keep_levels(plan.T, [(0, a), (b - 8, b - 2, .5)], FEATHER, ring=ring)
    assert {0.0, .25, .5, .75, 1.0} <= set(lv.tolist())
    count = np.zeros(plan.T, dtype=int)
    for s in plan.starts:
        count[s:s + plan.Tw] += 1
    assert lv[a - 1] == 1.0 and lv[a:a + FEATHER].tolist() == [.75, .5, .25] and all(count[a - 1:a + FEATHER] >= 2)
    return lv


def level4(lv, shape):
    return lv.view(1, 1, -1, 1).expand(shape).contiguous()


def step_mask(level, S, i):
    """The binary mask of loop step i of a run of S steps: the thresholds are the package's own table, pinned by the CPU tests."""
    from audioldm2_amd.sampling import keep_thresholds
    return (level > keep_thresholds(S)[i].to(level.device)).float()


# ---- the composition loops ----------------------------------------------------------------------------------------------------------
def ddim_graded_loop(model, x_T, x0, level, cond, uncond, ddim_steps, S, gs, eta=0.0, guidance_rescale=0.0, resample=(1, 1)):
    """Rs.resample_loop with the per-step mask: visits from Rs.published_visits ((1, 1): the plain run); per visit the q-noise row,
    then the step-noise row, on the host generator; a step visit at loop position i blends under step_mask(level, S, i).
    -> (x, the number of visits)."""
    from audioldm2_amd.ddim import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(ddim_steps, ddim_eta=eta, verbose=False)
    time_range = np.flip(s.ddim_timesteps[:S])
    visits = Rs.published_visits(S, *resample)
    x, x0, level = x_T.cuda(), x0.cuda(), level.cuda()
    for v in visits:
        qn = torch.randn(x.shape)
        if v[0] == "step":
            i = v[1]
            step = int(time_range[i])
            sa, so = float(s.sqrt_alphas_cumprod[step]), float(s.sqrt_one_minus_alphas_cumprod[step])
            x = Ls.torch_blend(x, x0, qn.cuda(), step_mask(level, S, i), sa, so)
            ts = torch.full((x.shape[0],), step, device="cuda", dtype=torch.long)
            x, _ = s.p_sample_ddim(x, cond, ts, index=S - 1 - i, unconditional_guidance_scale=gs, unconditional_conditioning=uncond,
                                   guidance_rescale=guidance_rescale)
        else:
            c0, c1 = Rs.loop_coef(s, S, v[1], v[2])
            x = c0 * x + c1 * torch.randn(x.shape).cuda()
    return x, len(visits)


def plms_graded_loop(model, x_T, x0, level, cond, uncond, steps):
    """Ls.plms_source_loop over `model` with the per-step mask."""
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(model)
    s.make_schedule(steps, verbose=False)
    time_range = np.flip(s.ddim_timesteps[:steps])
    img, x0, level, old_eps = x_T.cuda(), x0.cuda(), level.cuda(), []
    b = img.shape[0]
    for i, step in enumerate(time_range):
        sa, so = float(s.sqrt_alphas_cumprod[int(step)]), float(s.sqrt_one_minus_alphas_cumprod[int(step)])
        img = Ls.torch_blend(img, x0, torch.randn(img.shape).cuda(), step_mask(level, steps, i), sa, so)
        ts = torch.full((b,), int(step), device="cuda", dtype=torch.long)
        ts_next = torch.full((b,), int(time_range[min(i + 1, steps - 1)]), device="cuda", dtype=torch.long)
        img, _, e_t = s.p_sample_plms(img, cond, ts, index=steps - i - 1, unconditional_guidance_scale=A.GS,
                                      unconditional_conditioning=uncond, old_eps=old_eps, t_next=ts_next)
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    return img


def dpmpp_graded_loop(model, x_T, x0, level, cond, uncond, steps, gs=A.GS):
    """Ls.dpmpp_source_loop over `model` with the per-step mask: the solver and the blend in fp64 around the model's fp32 output."""
    from audioldm2_amd.sampling import make_ddim_timesteps
    ac = model.alphas_cumprod
    ts = make_ddim_timesteps("uniform", steps, model.num_timesteps, verbose=False)[:steps]
    n, b = len(ts), x_T.shape[0]
    sqrt_ac, sqrt_1m = torch.sqrt(ac.float()), torch.sqrt(1.0 - ac.float())
    x, x0, level = x_T.double().cuda(), x0.double().cuda(), level.cuda()
    old, h_last = None, None
    for i, t in enumerate(np.flip(ts)):
        x = Ls.torch_blend(x, x0, torch.randn(x.shape).double().cuda(), step_mask(level, n, i).double(), float(sqrt_ac[int(t)]),
                           float(sqrt_1m[int(t)]))
        index = n - i - 1
        a_t = float(ac[ts[index]])
        a_p = float(ac[ts[index - 1]]) if index > 0 else float(ac[0])
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        wgt = 0.0 if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
        eps = model.apply_model_cfg(x.float(), torch.full((2 * b,), float(t), device="cuda"), cond, uncond).double()
        e = eps[0] + gs * (eps[1] - eps[0])
        p0 = (x - sg_t * e) / al_t
        d = p0 if wgt == 0.0 else p0 + wgt * (p0 - old)
        x = (sg_p / sg_t) * x + (-al_p * np.expm1(-h)) * d
        old, h_last = p0, h
    return x


def draws_after(seed, shape, n):
    """The torch.rand(1) that follows n draws at `shape` on the freshly seeded host generator."""
    torch.manual_seed(seed)
    for _ in range(n):
        torch.randn(tuple(shape))
    return float(torch.rand(1))
