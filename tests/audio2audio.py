"""Shared by tests/test_audio2audio_cpu.py and tests/test_audio2audio_gpu.py: the fp64 restatements (sdedit_plan, the
aldm_posterior_qsample arithmetic, the PLMS and DPM-Solver++(2M) loops over a schedule prefix), the kernel's cases and bar, and the
host-generator contract of LatentDiffusion.generate_batch_from_audio.

The kernel's bar.  Per element the kernel makes, in fp32: 0.5*lv (exact), expf (<= 1 ulp), std*n_post, mean + ., scale*., a*z,
b*n_enc and the last sum — four or five roundings of 2^-24 = 6e-8 each behind a <= 1.2e-7 exponential, measured against the SUM
OF THE MAGNITUDES of the terms (so cancellation does not enter): about 3e-7 worst case.  The project's rule puts the bar at 5x the
maximum measured on an MI355X against fp64 of the same fp32 inputs, and the bar may not exceed 1e-6 (a dropped or doubled term is an
error of order 1e-1).  Measured (profiles/r14_audio2audio_errors.txt): see KERNEL_MEASURED_MAX below.
"""
import numpy as np
import torch

# ---- sdedit_plan ----------------------------------------------------------------------------------------------------------------
PLAN_CASES = [(0.5, 200), (1.0, 200), (0.25, 4), (1.0, 1), (0.999, 7)]
PLAN_REFUSED = [(0.0, 200), (-0.1, 200), (1.01, 200), (float("nan"), 200), (0.1, 4)]
NUM_TIMESTEPS = 1000


def alphas_cumprod_fp64():
    """The schedule of every shipped config (linear_start 0.0015, linear_end 0.0195, 1000 steps), in fp64."""
    betas = np.linspace(np.sqrt(0.0015), np.sqrt(0.0195), NUM_TIMESTEPS, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def plan_fp64(strength, steps):
    """(t_enc, timestep, sqrt(abar), sqrt(1 - abar)) straight from the definitions, in fp64: the uniform DDIM grid is
    range(0, 1000, 1000 // steps) + 1; the run executes its entries t_enc-1 ... 0 and enters at the level of entry t_enc-1."""
    t_enc = int(strength * steps)
    grid = np.arange(0, NUM_TIMESTEPS, NUM_TIMESTEPS // steps) + 1
    t = int(grid[t_enc - 1])
    abar = alphas_cumprod_fp64()[t]
    return t_enc, t, float(np.sqrt(abar)), float(np.sqrt(1.0 - abar))


def ulps_fp32(got, ref64):
    """|fp32(got) - ref64| in units of the fp32 spacing at ref64."""
    return abs(float(np.float32(got)) - ref64) / float(np.spacing(np.float32(ref64)))


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
# (B0, n_gen, C, h, w): one pixel block; a ragged tail with r % B0 varying; hw = 63 / 64 / 65 around one wave; the 16 kHz shape;
# the 48 kHz shape
KERNEL_SHAPES = [(1, 1, 8, 2, 2), (3, 2, 8, 5, 3), (2, 3, 16, 7, 9), (1, 1, 8, 8, 8), (1, 2, 8, 13, 5), (2, 1, 8, 256, 16),
                 (1, 2, 16, 128, 32)]
KERNEL_SCALE = 0.75
PLANTED_LOGVAR = [-40.0, -30.0, 20.0, 25.0, float("inf"), float("-inf")]
GUARD = 64
# max over every shape and both coefficient pairs of the error figures below, measured on an MI355X against fp64
# (profiles/r14_audio2audio_errors.txt: x_t of the 48 kHz shape at index 0; z at most 1.68e-7, the tiling figure 1.35e-7); the bar
# is 5x that (1.09e-6) and may not exceed 1e-6, so it is 1e-6 — 4.6x the measured maximum
KERNEL_MEASURED_MAX = 2.173e-7
KERNEL_BAR = min(5 * KERNEL_MEASURED_MAX, 1e-6)
assert KERNEL_BAR <= 1e-6


def kernel_coef_pairs():
    """(sqrt(abar), sqrt(1 - abar)) at index 0 and at the last index of a 200-step grid, as fp32-representable floats."""
    ac = alphas_cumprod_fp64()
    grid = np.arange(0, NUM_TIMESTEPS, NUM_TIMESTEPS // 200) + 1
    return [(float(np.float32(np.sqrt(ac[t]))), float(np.float32(np.sqrt(1.0 - ac[t])))) for t in (grid[0], grid[-1])]


def kernel_inputs(shape, seed=0, nan_at=()):
    """fp32 host inputs of one case: moments_cl [B0, h, w, 2C] (mean N(0, 1); logvar U(-12, 4) with PLANTED_LOGVAR at seeded
    positions and NaN at the flat (b, c, p) positions `nan_at`), n_post [B0, C, h, w], n_enc [B0*n_gen, C, h, w]."""
    B0, n_gen, C, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B0, h * w, C, generator=g)
    logvar = torch.rand(B0, h * w, C, generator=g) * 16.0 - 12.0
    flat = logvar.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:len(PLANTED_LOGVAR)]
    for i, v in zip(pos.tolist(), PLANTED_LOGVAR):
        flat[i] = v
    for (b, c, p) in nan_at:
        logvar[b, p, c] = float("nan")
    moments = torch.cat([mean, logvar], dim=2).view(B0, h, w, 2 * C).contiguous()
    n_post = torch.randn(B0, C, h, w, generator=g)
    n_enc = torch.randn(B0 * n_gen, C, h, w, generator=g)
    return moments, n_post, n_enc


def kernel_fp64(moments, n_post, n_enc, scale, a, b):
    """The entry point's arithmetic in fp64 on the fp32 inputs -> (z, x_t, dz, dx): the outputs and the error denominators
    |s mean| + |s std n_post| and a*dz + |b n_enc| (sums of the magnitudes of the terms)."""
    B0, h, w, C2 = moments.shape
    C = C2 // 2
    m = moments.double().view(B0, h * w, C2).permute(0, 2, 1).reshape(B0, C2, h, w)
    mean, logvar = m[:, :C], m[:, C:]
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    n_gen = n_enc.shape[0] // B0
    t1, t2 = scale * mean, scale * std * n_post.double()
    z = t1 + t2
    dz = t1.abs() + t2.abs()
    zz, dzz = torch.cat([z] * n_gen), torch.cat([dz] * n_gen)
    t3 = b * n_enc.double()
    return z, a * zz + t3, dz, abs(a) * dzz + t3.abs()


def guarded(shape, fill=-777.0):
    """A CUDA tensor of `shape` inside a buffer with GUARD sentinel floats on each side -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda")
    return buf[GUARD:GUARD + n].view(shape), buf


def guards_intact(buf, fill=-777.0):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


# ---- the samplers over a schedule prefix ----------------------------------------------------------------------------------------
GS = 3.5


def rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))


def rel_rms(a, ref):
    a, ref = a.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    return rms(a - ref) / rms(ref)


TINY_SHAPE = (2, 8, 16, 8)


class TinyModel:
    """What a sampler touches on its model (num_timesteps, alphas_cumprod, apply_model, prepare_cfg, apply_model_cfg) over the tiny
    UNet (cases.UNET_TINY), as in tests/test_dpmpp_gpu.py; conditioning = (contexts, masks)."""
    num_timesteps = 1000

    def __init__(self):
        from audioldm2_amd.unet import UNetModel
        from oracle import cases, weights
        self.unet = UNetModel(**cases.UNET_TINY)
        self.unet.load_state_dict(weights.make_state_dict(weights.shapes_of(self.unet), seed=0))
        self.unet.cuda()
        self.alphas_cumprod = torch.from_numpy(alphas_cumprod_fp64()).float()

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


def tstart_bar(k):
    """Bar of a k-step latent against the sampler's own step-by-step loop (relative rms): the project's bar of a short-run latent,
    tolerances.latent_tol(k), scaled by the UNet bar of the mode over the fp32-grade one (1 in the fp32-grade modes).  Both sides run
    the same kernels on the same inputs (the fp64 DPM-Solver++ loop differs by fp32 step arithmetic, ~4e-7 in tests/test_dpmpp_gpu.py)."""
    from tolerances import latent_tol, unet_tol
    return latent_tol(k) * unet_tol() / unet_tol("bf16x6")


def plms_eager_loop(sampler, x, cond, uncond, k):
    """PLMS over schedule indices k-1 ... 0 with the eager single-step form and a Python `old_eps` list (plms.py:229-248), as
    tests/test_plms_gpu.py::test_p_sample_plms_steps_equal_the_sampling_loop walks the whole schedule."""
    time_range = np.flip(sampler.ddim_timesteps[:k])
    b = x.shape[0]
    img, old_eps = x, []
    for i, step in enumerate(time_range):
        ts = torch.full((b,), int(step), device="cuda", dtype=torch.long)
        ts_next = torch.full((b,), int(time_range[min(i + 1, k - 1)]), device="cuda", dtype=torch.long)
        img, _, e_t = sampler.p_sample_plms(img, cond, ts, index=k - i - 1, unconditional_guidance_scale=GS,
                                            unconditional_conditioning=uncond, old_eps=old_eps, t_next=ts_next)
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    return img


def dpmpp_fp64_loop(model_cfg, ac, ts, xT, gs=GS):
    """DPM-Solver++(2M) over the ascending timestep subset `ts` of the fp32 schedule `ac`, as tests/test_dpmpp_gpu.py::fp64_loop:
    eps from model_cfg(x fp32, t) -> [2, b, ...] on the fp32 image of the fp64 state, everything else in fp64 with unrounded
    coefficients; first order at the first step and (runs under 15 steps) at the last."""
    n = len(ts)
    time_range = np.flip(ts)
    x = xT.double().cuda()
    old, h_last = None, None
    for i, t in enumerate(time_range):
        index = n - i - 1
        a_t = float(ac[ts[index]])
        a_p = float(ac[ts[index - 1]]) if index > 0 else float(ac[0])
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        wgt = 0.0 if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
        eps = model_cfg(x.float(), float(t)).double()
        e = eps[0] + gs * (eps[1] - eps[0])
        p0 = (x - sg_t * e) / al_t
        d = p0 if wgt == 0.0 else p0 + wgt * (p0 - old)
        x = (sg_p / sg_t) * x + (-al_p * np.expm1(-h)) * d
        old, h_last = p0, h
    return x


# ---- the host-generator contract ----------------------------------------------------------------------------------------------
def expected_rand_after(seed, B0, n_gen, latent_shape, t_enc, second_call=False, sampler=None, cond_draws=None, n_neg=0):
    """The torch.rand(1) that follows one generate_batch_from_audio job on the host default generator, by performing the job's
    draws by hand (RNG contract): (1) randn(B0, C, h, w), the posterior noise; (2) rand(1) on every call of an
    object but its first; (3) the conditioners' draws (`cond_draws()`, once more per negative-prompt pass; the synthetic
    conditioners of the test fixtures have a generator of their own and draw nothing); (4) randn(B0*n_gen, C, h, w), the
    forward-diffusion noise; (5) the sampler's per-step draws for t_enc steps: DDIM one randn of the batch per step at every eta,
    PLMS (`sampler="plms"`) one per step and one more for the provisional update of its first step, DPM-Solver++(2M)
    (`sampler="dpmpp_2m"`) none."""
    C, h, w = latent_shape
    torch.manual_seed(seed)
    torch.randn((B0, C, h, w))
    if second_call:
        torch.rand(1)
    for _ in range(1 + n_neg):
        if cond_draws is not None:
            cond_draws()
    torch.randn((B0 * n_gen, C, h, w))
    per_run = {None: t_enc, "plms": t_enc + 1, "dpmpp_2m": 0}[sampler]
    for _ in range(per_run):
        torch.randn((B0 * n_gen, C, h, w))
    return float(torch.rand(1))
