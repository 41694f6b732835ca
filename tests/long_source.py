"""Shared by tests/test_long_source_cpu.py and tests/test_long_source_gpu.py (continuation and inpainting of long clips, DESIGN.md
9f): the mask patterns of the fused blend-and-gather kernel, its fp64 restatement and derived bar, and the composition loops of
windowed sampling WITH a source — per step a torch blend on the long latent with the q-noise drawn by hand in contract order, then
the sampler's existing eager single-step form over windowed.WindowedModel (slice, same model, fp64 merge).

The kernel's bar, u = 2^-24, D = |sa*x0| + |so*qn| + |x_in|.  x = (sa*x0 + so*qn)*m + (1 - m)*x rounds, in fp32: sa*x0, so*qn and
their sum (3u of |sa*x0| + |so*qn| together), the product with m (one more u, scaled like the three before it by m), (1 - m)*x (u of
(1 - m)|x|; 1 - m itself is exact for the masks used) and the last sum (u of the result): at most 4u m (|sa*x0| + |so*qn|) +
2u (1 - m)|x| to first order.  A binary mask makes the products with m and 1 - m and the last sum exact: 3u (|sa*x0| + |so*qn|) at
m = 1, nothing at m = 0.  At m = 0.25 it is u (|sa*x0| + |so*qn|) + 1.5u |x|.  All are within the issue's bar of three roundings
of the whole sum, 3u D element-wise — derived, not measured.
"""
import numpy as np
import torch

import audio2audio as A
import windowed as Wd

# the sampler tests: the tiny model's long shape and plan of tests/test_windowed_gpu.py, six steps, two kept intervals that both cut
# through window overlaps of the plan (40, 16, 10): starts 0, 10, 20, 24 -> overlaps [10, 16), [20, 26), [24, 36)
LONG_KEY, STEPS = (40, 16, 10), 6
LONG_SHAPE = (A.TINY_SHAPE[0], A.TINY_SHAPE[1], LONG_KEY[0], A.TINY_SHAPE[3])
KEEP = [(0, 13), (29, 33)]


def overlap_interval(plan):
    """A half-open interval [a, b) whose two ends fall strictly inside a window overlap and on no window start: a and b are frames
    under two or more windows whose predecessor is too, and neither is a start."""
    count = np.zeros(plan.T + 1, dtype=int)
    for s in plan.starts:
        count[s:s + plan.Tw] += 1
    ok = [t for t in range(1, plan.T) if count[t] >= 2 and count[t - 1] >= 2 and t not in plan.starts]
    assert len(ok) >= 2 and ok[0] < ok[-1], "the plan has no overlap to cut through"
    return ok[0], ok[-1]


def mask_patterns(plan, shape):
    """name -> mask [B, C, T, F] fp32 (host): all 0, all 1, a kept interval cutting through overlaps, and a non-binary 0.25."""
    a, b = overlap_interval(plan)
    cut = torch.zeros(shape)
    cut[:, :, a:b] = 1.0
    return {"zeros": torch.zeros(shape), "ones": torch.ones(shape), f"keep[{a},{b})": cut, "quarter": torch.full(shape, 0.25)}


def blend_inputs(B, plan, C, F, S=1, seed=0):
    """fp32 host tensors of one case: x, x0 [B, C, T, F], qnoise [S, B, C, T, F] N(0, 1), blend_coef [S, 2] = {sa, so} from the
    shipped schedule at S spread timesteps."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, plan.T, F)
    x, x0, qn = torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn((S,) + shape, generator=g)
    ac = A.alphas_cumprod_fp64()
    ts = np.linspace(900, 1, S).astype(int)
    coef = torch.tensor([[np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])] for t in ts], dtype=torch.float32)
    return x, x0, qn, coef


def blend_fp64(x, x0, qn, m, sa, so):
    """The blend in fp64 on the fp32 inputs -> (x_new, the error denominator |sa*x0| + |so*qn| + |x_in|)."""
    x, x0, qn, m = x.double(), x0.double(), qn.double(), m.double()
    sa, so = float(sa), float(so)
    return (sa * x0 + so * qn) * m + (1.0 - m) * x, (sa * x0).abs() + (so * qn).abs() + x.abs()


def blend_gather_fp64(x, x0, qn, m, sa, so, plan):
    """Blend, then gather: the windows of the blended long latent, fp64."""
    return Wd.gather_ref(blend_fp64(x, x0, qn, m, sa, so)[0], plan)


BLEND_BAR = 3 * 2.0 ** -24


# ---- the composition loops with a source -----------------------------------------------------------------------------------------
def torch_blend(x, x0, qn, m, sa, so):
    return (sa * x0 + so * qn) * m + (1.0 - m) * x


def _coef(sampler, step):
    return float(sampler.sqrt_alphas_cumprod[int(step)]), float(sampler.sqrt_one_minus_alphas_cumprod[int(step)])


def ddim_source_loop(inner, plan, x_T, x0, mask, cond, uncond, S, gs, eta=0.0, guidance_rescale=0.0, k=None):
    """Per step: the q-noise draw (host generator), the torch blend on the long latent, then DDIMSampler.p_sample_ddim over the
    windowed model — which draws the step noise: q-noise first, as the contract says."""
    from audioldm2_amd.ddim import DDIMSampler
    s = DDIMSampler(Wd.WindowedModel(inner, plan))
    s.make_schedule(S, ddim_eta=eta, verbose=False)
    k = len(s.ddim_timesteps) if k is None else k
    time_range = np.flip(s.ddim_timesteps[:k])
    x, x0, mask = x_T.cuda(), x0.cuda(), mask.cuda()
    for i, step in enumerate(time_range):
        sa, so = _coef(s, step)
        x = torch_blend(x, x0, torch.randn(x.shape).cuda(), mask, sa, so)
        ts = torch.full((x.shape[0],), int(step), device="cuda", dtype=torch.long)
        x, _ = s.p_sample_ddim(x, cond, ts, index=k - i - 1, unconditional_guidance_scale=gs,
                               unconditional_conditioning=uncond, guidance_rescale=guidance_rescale)
    return x


def plms_source_loop(inner, plan, x_T, x0, mask, cond, uncond, steps):
    """audio2audio.plms_eager_loop with the q-noise draw and the torch blend in front of every p_sample_plms (whose discarded
    noise_like draws follow)."""
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(Wd.WindowedModel(inner, plan))
    s.make_schedule(steps, verbose=False)
    time_range = np.flip(s.ddim_timesteps[:steps])
    img, x0, mask, old_eps = x_T.cuda(), x0.cuda(), mask.cuda(), []
    b = img.shape[0]
    for i, step in enumerate(time_range):
        sa, so = _coef(s, step)
        img = torch_blend(img, x0, torch.randn(img.shape).cuda(), mask, sa, so)
        ts = torch.full((b,), int(step), device="cuda", dtype=torch.long)
        ts_next = torch.full((b,), int(time_range[min(i + 1, steps - 1)]), device="cuda", dtype=torch.long)
        img, _, e_t = s.p_sample_plms(img, cond, ts, index=steps - i - 1, unconditional_guidance_scale=A.GS,
                                      unconditional_conditioning=uncond, old_eps=old_eps, t_next=ts_next)
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    return img


def dpmpp_source_loop(inner, plan, x_T, x0, mask, cond, uncond, steps, gs=A.GS):
    """audio2audio.dpmpp_fp64_loop with the q-noise draw and the blend (in fp64, fp32 coefficients) in front of every step: the
    solver in fp64 around the windowed model's fp32 output; the q-noise is the run's only draw."""
    from audioldm2_amd.sampling import make_ddim_timesteps
    wm = Wd.WindowedModel(inner, plan)
    ac = inner.alphas_cumprod
    ts = make_ddim_timesteps("uniform", steps, inner.num_timesteps, verbose=False)[:steps]
    n, b = len(ts), x_T.shape[0]
    sqrt_ac, sqrt_1m = torch.sqrt(ac.float()), torch.sqrt(1.0 - ac.float())
    x, x0, mask = x_T.double().cuda(), x0.double().cuda(), mask.double().cuda()
    old, h_last = None, None
    for i, t in enumerate(np.flip(ts)):
        x = torch_blend(x, x0, torch.randn(x.shape).double().cuda(), mask, float(sqrt_ac[int(t)]), float(sqrt_1m[int(t)]))
        index = n - i - 1
        a_t = float(ac[ts[index]])
        a_p = float(ac[ts[index - 1]]) if index > 0 else float(ac[0])
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        wgt = 0.0 if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
        eps = wm.apply_model_cfg(x.float(), torch.full((2 * b,), float(t), device="cuda"), cond, uncond).double()
        e = eps[0] + gs * (eps[1] - eps[0])
        p0 = (x - sg_t * e) / al_t
        d = p0 if wgt == 0.0 else p0 + wgt * (p0 - old)
        x = (sg_p / sg_t) * x + (-al_p * np.expm1(-h)) * d
        old, h_last = p0, h
    return x


def expected_rand_after_source(seed, B0, long_shape, steps, second_call=False, sampler=None):
    """The torch.rand(1) that follows one generate_batch_long_from_audio job on the host default generator, by performing the job's
    draws by hand (its docstring): randn(B0, *long_shape), the posterior noise at the LONG shape; rand(1) on every call of an object
    but its first; (the synthetic conditioners draw nothing); randn(B0, *long_shape), x_T; per step at the long shape DDIM two draws
    (q-noise, step noise), PLMS the q-noise and its own (one per step and one more in its first), DPM-Solver++ the q-noise."""
    torch.manual_seed(seed)
    torch.randn((B0,) + tuple(long_shape))
    if second_call:
        torch.rand(1)
    torch.randn((B0,) + tuple(long_shape))
    for _ in range({None: 2 * steps, "plms": 2 * steps + 1, "dpmpp_2m": steps}[sampler]):
        torch.randn((B0,) + tuple(long_shape))
    return float(torch.rand(1))
