"""Shared by tests/test_windowed_cpu.py and tests/test_windowed_gpu.py: the plan grid, the fp64 restatements of the window gather
and merge (torch slicing, an overlap-add in double precision), and the composition loop of windowed sampling — a model wrapper
that slices the long latent, runs the SAME model on the windows and merges in fp64, stepped by each sampler's existing eager
single-step form.

The merge kernel's bar.  An output element is sum_j wn_j e_j over at most `cover` windows: one rounding for the first product and
one per fused multiply-add, each at most 2^-24 of the magnitude it rounds, which never exceeds sum_j |wn_j e_j|.  Measured against
that sum of magnitudes (so cancellation does not enter) the error is at most cover * 2^-24, up to terms of order 2^-48.
"""
import numpy as np
import torch

# (T, Tw, hop) -> (W, cover, last start)
PLAN_GRID = {(40, 16, 10): (4, 3, 24), (48, 16, 16): (3, 1, 32), (16, 16, 8): (1, 1, 0), (24, 16, 1): (9, 9, 8),
             (768, 256, 192): (4, 2, 512), (320, 128, 96): (3, 2, 192), (160, 64, 48): (3, 2, 96), (384, 256, 128): (2, 2, 128),
             (32, 16, 16): (2, 1, 16), (40, 16, 16): (3, 2, 24)}
PLAN_REFUSED = [(36, 16, 8), (40, 12, 8), (0, 16, 8), (40, 0, 8), (8, 16, 8), (40, 16, 0), (40, 16, 17), (40, 16, 2.5), (40, 16, None),
                (8 * 40, 8, 1)]   # the last: 33 windows

# gather / merge cases (B, (T, Tw, hop), C, F): F = 5 and 7 take the scalar path, 16 / 32 / 64 the 16-byte one; rows of 5 and 7 floats
# straddle the waves; the two last plans are the 10.24 s windows of audioldm2-full at 30 s and of audioldm_48k at 25 s
KERNEL_CASES = [(2, (40, 16, 10), 3, 5), (1, (24, 16, 1), 2, 7), (1, (768, 256, 192), 8, 16), (1, (320, 128, 96), 16, 32)]
MEL_CASE = (2, (160, 64, 48), 1, 64)


def bar(plan):
    return plan.cover * 2.0 ** -24


def window_inputs(B, plan, C, F, H=None, seed=0):
    """fp32 host tensors of one case: x [B, C, T, F] and win [(H,) W*B, C, Tw, F], N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, plan.T, F, generator=g)
    win = torch.randn(*(() if H is None else (H,)), plan.W * B, C, plan.Tw, F, generator=g)
    return x, win


def gather_ref(x, plan):
    """torch slicing: window-major rows j*B + b."""
    return torch.cat([x[:, :, s:s + plan.Tw] for s in plan.starts]).contiguous()


def merge_fp64(win, plan):
    """The overlap-add in fp64 on the fp32 inputs: win [..., W*B, C, Tw, F] -> (out [..., B, C, T, F], the sum of the magnitudes
    of the terms, the number of windows over every frame [T])."""
    win = win.double()
    W, Tw = plan.W, plan.Tw
    B = win.shape[-4] // W
    shape = tuple(win.shape[:-4]) + (B,) + tuple(win.shape[-3:-2]) + (plan.T, win.shape[-1])
    out = torch.zeros(shape, dtype=torch.float64, device=win.device)
    den = torch.zeros_like(out)
    count = torch.zeros(plan.T, dtype=torch.int64)
    wn = plan.wn.double().to(win.device)
    for j, s in enumerate(plan.starts):
        term = wn[j].view(Tw, 1) * win[..., j * B:(j + 1) * B, :, :, :]
        out[..., s:s + Tw, :] += term
        den[..., s:s + Tw, :] += term.abs()
        count[s:s + Tw] += 1
    return out, den, count


def tile(c, W):
    """A conditioning repeated for W windows, window-major (tensors inside lists, tuples and dicts)."""
    if c is None:
        return None
    if torch.is_tensor(c):
        return torch.cat([c] * W, dim=0)
    if isinstance(c, dict):
        return {k: tile(v, W) for k, v in c.items()}
    return type(c)(tile(v, W) for v in c)


class WindowedModel:
    """What a sampler touches on its model, over `inner` (audio2audio.TinyModel, or a LatentDiffusion) applied window by window:
    slice the long latent, run the same model on the W*b windows under the tiled conditioning, merge in fp64, round to fp32."""

    def __init__(self, inner, plan):
        self.inner, self.plan = inner, plan
        self.num_timesteps, self.alphas_cumprod = inner.num_timesteps, inner.alphas_cumprod

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        assert prepared is None
        W, b = self.plan.W, x.shape[0]
        xw = gather_ref(x.float(), self.plan)
        eps = self.inner.apply_model_cfg(xw, t2[:1].float().repeat(2 * W * b), tile(cond, W), tile(uncond, W))
        return merge_fp64(eps, self.plan)[0].float().contiguous()


# ---- the composition loops: each sampler's existing eager single-step form over the windowed model -------------------------------
def ddim_loop(inner, plan, x_T, cond, uncond, S, gs, eta=0.0, guidance_rescale=0.0, k=None):
    """DDIMSampler.decode over the first k entries of the S-step schedule (None: all of them; one p_sample_ddim per step; with
    guidance_rescale, ops.cfg_rescale_indexed on the merged pair)."""
    from audioldm2_amd.ddim import DDIMSampler
    s = DDIMSampler(WindowedModel(inner, plan))
    s.make_schedule(S, ddim_eta=eta, verbose=False)
    return s.decode(x_T.cuda(), cond, len(s.ddim_timesteps) if k is None else k, unconditional_guidance_scale=gs,
                    unconditional_conditioning=uncond, guidance_rescale=guidance_rescale)


def plms_loop(inner, plan, x_T, cond, uncond, steps):
    """audio2audio.plms_eager_loop over the first `steps` entries of the `steps`-step schedule (one p_sample_plms per step, a
    Python history list), guidance audio2audio.GS."""
    import audio2audio as A
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(WindowedModel(inner, plan))
    s.make_schedule(steps, verbose=False)
    return A.plms_eager_loop(s, x_T.cuda(), cond, uncond, steps)


def dpmpp_loop(inner, plan, x_T, cond, uncond, steps):
    """audio2audio.dpmpp_fp64_loop over the first `steps` entries of the `steps`-step schedule (the solver in fp64 around the
    model's fp32 output), guidance audio2audio.GS."""
    import audio2audio as A
    from audioldm2_amd.sampling import make_ddim_timesteps
    wm = WindowedModel(inner, plan)
    b = x_T.shape[0]
    model_cfg = lambda xx, t: wm.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), cond, uncond)
    ts = make_ddim_timesteps("uniform", steps, inner.num_timesteps, verbose=False)
    return A.dpmpp_fp64_loop(model_cfg, inner.alphas_cumprod, ts[:steps], x_T)


def expected_rand_after_long(seed, B0, r1_shape, long_shape, steps, second_call=False, sampler=None):
    """The torch.rand(1) that follows one generate_batch_long job on the host default generator, by performing the job's draws by
    hand (generate_batch_long's docstring): randn(B0, *r1_shape) drawn and discarded; rand(1) on every call of an object but its
    first; (the synthetic conditioners draw nothing); randn(B0, *long_shape), x_T; the sampler's per-step draws at the long shape."""
    torch.manual_seed(seed)
    torch.randn((B0,) + tuple(r1_shape))
    if second_call:
        torch.rand(1)
    torch.randn((B0,) + tuple(long_shape))
    for _ in range({None: steps, "plms": steps + 1, "dpmpp_2m": 0}[sampler]):
        torch.randn((B0,) + tuple(long_shape))
    return float(torch.rand(1))
