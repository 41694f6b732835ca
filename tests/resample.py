"""Shared by tests/test_resample_cpu.py and tests/test_resample_gpu.py (resampled inpainting, RePaint's jumps): the
visit table of the issue, an independent restatement of the published jump schedule, a literal fp64 restatement of the forward
jump's coefficients, the kernel's cases and derived bar, and the composition loop of a resampled run — per visit the draws by hand
in contract order (q-noise row, step-noise row), on a step visit the torch blend and DDIMSampler.p_sample_ddim over the model (or
over the slicing model wrappers of tests/windowed.py, tests/looped.py, tests/timeline.py), on a renoise visit a torch fp32 axpby.

The kernel's bar, u = 2^-24.  x = c0*x + c1*eps rounds two products and one sum: fl(c0 x) = c0 x (1 + d1), fl(c1 eps) = c1 eps (1 + d2),
and the sum once more (1 + d3), |d| <= u.  |err| <= (|c0 x| + |c1 eps|) ((1 + u)^2 - 1) = (2u + u^2)(|c0 x| + |c1 eps|), written
2u(1 + u)(|c0 x| + |c1 eps|) with room for the u^2 term — derived from the three roundings, not measured.
"""
import numpy as np
import torch

import audio2audio as A
import long_source as Ls

# (S, n, jump) -> the visits, as the issue prints them
VISIT_TABLE = {
    (6, 2, 2): "s0 s1 s2 s3 R(4→2) s2 s3 s4 s5 R(6→4) s4 s5",
    (5, 2, 2): "s0 s1 s2 R(3→1) s1 s2 s3 s4 R(5→3) s3 s4",
    (3, 2, 1): "s0 s1 R(2→1) s1 s2 R(3→2) s2",
    (4, 2, 2): "s0 s1 s2 s3 R(4→2) s2 s3",
    (6, 1, 2): "s0 s1 s2 s3 s4 s5",
}
VISIT_COUNTS = {(6, 2, 2): 12, (5, 2, 2): 11, (3, 2, 1): 7, (4, 2, 2): 7, (6, 1, 2): 6}
# (S, n, jump) -> (step visits, renoise visits)
LARGE_COUNTS = {(200, 10, 10): (1910, 171), (50, 10, 10): (410, 36)}
GRID = [(S, n, jump) for S in (2, 3, 5, 6, 7, 12, 50) for n in (1, 2, 3, 10) for jump in (1, 2, 3, 5, 10) if jump <= S - 1]


def show(visits):
    return " ".join(f"s{v[1]}" if v[0] == "step" else f"R({v[1]}→{v[2]})" for v in visits)


def jump_points(S, jump):
    return [k for k in range(S + 1) if (S - k) % jump == 0 and k > jump]


def published_visits(S, n, jump):
    """RePaint's get_schedule_jump restated over the count t of steps REMAINING: a dictionary of the remaining-step counts 0, jump,
    2*jump, ... below S - jump, each good for n - 1 jumps; walk t down, and where an entry is left, go back up by `jump`."""
    jumps = {t: n - 1 for t in range(0, S - jump, jump)}
    t, visits = S, []
    while t >= 1:
        visits.append(("step", S - t))
        t -= 1
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            visits.append(("renoise", S - t, S - t - jump))
            t += jump
    return tuple(visits)


# ---- the forward jump's coefficients ------------------------------------------------------------------------------------------------
class ScheduleModel:
    """What DDIMSampler.make_schedule reads: the shipped schedule as the model holds it, fp32."""
    num_timesteps = A.NUM_TIMESTEPS

    def __init__(self):
        self.alphas_cumprod = torch.from_numpy(A.alphas_cumprod_fp64()).float()


def coef_fp64(ddim_steps, S, k, k_to):
    """(c0, c1) straight from the definitions, in fp64 from the model's fp32 schedule: the uniform grid is range(0, 1000, 1000 //
    ddim_steps) + 1, a run of S steps uses its entries S-1 ... 0, position p < S is at abar[grid[S-1-p]] and position S at abar[0]."""
    ac = ScheduleModel().alphas_cumprod.double().numpy()
    grid = np.arange(0, A.NUM_TIMESTEPS, A.NUM_TIMESTEPS // ddim_steps) + 1
    abar = lambda p: ac[grid[S - 1 - p]] if p < S else ac[0]
    rho = abar(k_to) / abar(k)
    return float(np.sqrt(rho)), float(np.sqrt(1.0 - rho))


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
KERNEL_BAR = 2 * U * (1 + U)
# n: 3 and 1021 take the scalar path, 8*8*40*5 and 1*8*768*16 the 16-byte one (the tiny long latent and the 30 s one)
KERNEL_N = [3, 1021, 8 * 8 * 40 * 5, 1 * 8 * 768 * 16]
KERNEL_ROWS = 3


def kernel_inputs(n, seed=0):
    """fp32 host tensors: x [n], a noise table [3, n] of distinct rows, a coefficient table [3, 8] of distinct rows whose first two
    columns are forward-jump coefficients of the shipped schedule (the other six hold sentinels the kernel must not read into x)."""
    g = torch.Generator().manual_seed(seed)
    x, noise = torch.randn(n, generator=g) * 1.5, torch.randn(KERNEL_ROWS, n, generator=g)
    coef = torch.full((KERNEL_ROWS, 8), 1e30)
    for r, (S, k, k_to) in enumerate(((200, 200, 190), (50, 20, 10), (6, 4, 2))):
        coef[r, 0], coef[r, 1] = coef_fp64(S, S, k, k_to)
    return x, noise, coef


# ---- the composition loop ---------------------------------------------------------------------------------------------------------
def loop_coef(sampler, S, k, k_to):
    """The forward jump's fp32 coefficients from the sampler's own schedule tables, literally."""
    a = np.asarray(sampler.ddim_alphas, dtype=np.float64)
    abar = lambda p: float(a[S - 1 - p]) if p < S else float(np.asarray(sampler.ddim_alphas_prev, dtype=np.float64)[0])
    rho = abar(k_to) / abar(k)
    return float(np.float32(np.sqrt(rho))), float(np.float32(np.sqrt(1.0 - rho)))


def resample_loop(model, x_T, x0, mask, cond, uncond, ddim_steps, S, n, jump, gs, eta=0.0, guidance_rescale=0.0):
    """A resampled DDIM run by composition over `model` (the tiny model, a LatentDiffusion, or one of the slicing wrappers around
    them): the first S entries of the `ddim_steps` schedule, visits from published_visits.  Per visit, on the host generator in
    contract order: the q-noise row, then the step-noise row.  Step visit at loop position i: the torch blend of q_sample(x0, t_i)
    where mask == 1, then DDIMSampler.p_sample_ddim at index S-1-i (it draws the step noise).  Renoise visit k -> k': the q-noise
    row is drawn and dropped, the step-noise row is eps, x = c0*x + c1*eps in torch fp32 on the device.  -> (x, the number of visits)."""
    from audioldm2_amd.ddim import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(ddim_steps, ddim_eta=eta, verbose=False)
    time_range = np.flip(s.ddim_timesteps[:S])
    visits = published_visits(S, n, jump)
    x, x0, mask = x_T.cuda(), x0.cuda(), mask.cuda()
    for v in visits:
        qn = torch.randn(x.shape)
        if v[0] == "step":
            i = v[1]
            step = int(time_range[i])
            sa, so = float(s.sqrt_alphas_cumprod[step]), float(s.sqrt_one_minus_alphas_cumprod[step])
            x = Ls.torch_blend(x, x0, qn.cuda(), mask, sa, so)
            ts = torch.full((x.shape[0],), step, device="cuda", dtype=torch.long)
            x, _ = s.p_sample_ddim(x, cond, ts, index=S - 1 - i, unconditional_guidance_scale=gs, unconditional_conditioning=uncond,
                                   guidance_rescale=guidance_rescale)
        else:
            c0, c1 = loop_coef(s, S, v[1], v[2])
            eps = torch.randn(x.shape).cuda()
            x = c0 * x + c1 * eps
    return x, len(visits)


def draws_after(seed, shape, visits, x_T_drawn=True, before=()):
    """The torch.rand(1) that follows a resampled run on the host default generator: the draws `before` (shapes), x_T when the
    run draws it, then two draws at the latent's shape per visit."""
    torch.manual_seed(seed)
    for sh in before:
        torch.randn(tuple(sh))
    if x_T_drawn:
        torch.randn(tuple(shape))
    for _ in range(2 * visits):
        torch.randn(tuple(shape))
    return float(torch.rand(1))
