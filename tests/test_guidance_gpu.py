"""Negative prompts and guidance rescale on the GPU (ops.cfg_rescale_indexed, the three samplers, pipeline.generate_batch):

 1. the kernel against an fp64 restatement at five shapes (16-byte and scalar form, fewer elements than a wave, more than one
    sweep iteration, the largest latent), phi 0.7 and 1.0, the counter at row 0 and row 2 of a three-row table, samples of very
    different scale, with and without an offset of 50 that a one-pass variance does not survive; inputs untouched, two calls bitwise equal;
 2. special values: phi = 0, s = 1, an all-zero sample, n_s = 1, a NaN confined to its sample;
 3. the wrapper's checks;
 4. DDIM (eta 0), PLMS and DPM-Solver++(2M) on the tiny UNet with guidance 3.5 and phi 0.7 against a loop written here (eps from
    apply_model_cfg, everything else in fp64); graph replay == eager bitwise; phi = 0 == the sampler without the argument bitwise;
 5. on a LatentDiffusion at a 64 x 16 latent: two rescaled DDIM jobs with different (scale, phi) through one cached graph, a
    plain job after a rescaled one, a one-rank shard, text_to_audio;
 6. negative prompts through the HIP conditioner stack.

Bars.  f = phi std(e_c) / std(e_g) + 1 - phi, out = f e_g evaluated by torch in fp32 on the same inputs is measured against its
fp64 evaluation in the test itself; the bar is 4x that figure, for a sampler run times the number of steps.  Comparisons of one
launch sequence with itself (graph against eager, a cached graph against a fresh model, a shard of one rank) are bitwise.

Measured on an MI355X (max|err| / max|ref|; kernel / torch fp32; every case: profiles/r11_guidance_errors.txt):
 (1) worst kernel-to-torch ratios: n_s = 3 offset 0 phi 0.7: 8.70e-8 / 2.95e-8 (2.9x); n_s = 98 304 offset 50 phi 1.0: 2.30e-7 /
     8.91e-8 (2.6x); n_s = 4100 offset 50 phi 1.0: 1.49e-7 / 9.12e-8; every other case below 1.6x, e.g. n_s = 1024 offset 0
     8.59e-8 / 8.59e-8, n_s = 1003 offset 50 6.63e-8 / 1.30e-7.  n_s = 3 at offset 50 is 8.25e-6 / 8.25e-6: the fp32 inputs
     themselves carry the std of three values near 50 to five digits.
 (2) phi = 0 against the plain combine 6.29e-8 (bar 2.52e-7); s = 1 against e_c 2.13e-8 (bar 8.51e-8).
 (4) sampler vs fp64 loop (x) / torch fp32 per step / bar: DDIM 2.35e-7 / 1.42e-7 / 3.97e-6; PLMS 4.07e-7 / 1.53e-7 / 4.30e-6;
     2M 4.27e-7 / 3.30e-7 / 9.23e-6.  phi 0.7 moves the 7-step latent by 6.1e-2 (DDIM), 2.7e-2 (PLMS), 5.5e-2 (2M) of its maximum.
 (6) the job against sample_log by hand: 0 (bar 4.77e-7).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, weights
from tolerances import log_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GS, PHI = 3.5, 0.7


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


def rescale_formula(eps, s, phi, dt):
    """eps [2, B, ...] -> f e_g on tensors of dtype dt, per sample; f = 1 where std(e_g) == 0 or the sample has one element."""
    eps = eps.to(dt)
    eu, ec = eps[0], eps[1]
    eg = eu + s * (ec - eu)
    B = eg.shape[0]
    if eg[0].numel() == 1:
        return eg
    sc, sg = ec.reshape(B, -1).std(1), eg.reshape(B, -1).std(1)
    f = torch.where(sg == 0, torch.ones_like(sg), phi * sc / sg + (1 - phi))
    return f.reshape((B,) + (1,) * (eg.dim() - 1)) * eg


# ---- 1. kernel vs fp64 ------------------------------------------------------------------------------------------------------------
SCALES = (0.1, 1.0, 30.0)


def kernel_inputs(shape, offset, seed=17):
    """eps [2, B, C, H, W]: seeded normals, e_u = e_c + 0.3 N(0, 1), sample b's two slabs scaled by SCALES[b] (a batch-wide
    statistic fails on them), then `offset` added to both."""
    g = torch.Generator().manual_seed(seed)
    ec = torch.randn(shape, generator=g)
    eu = ec + 0.3 * torch.randn(shape, generator=g)
    sc = torch.tensor(SCALES[:shape[0]]).reshape(-1, 1, 1, 1)
    return (torch.stack([eu * sc, ec * sc]) + offset).contiguous()


def table(phi):
    """three rows of eight floats: row 0 = (3.5, phi), row 2 another scale and phi; the step columns hold junk the kernel ignores"""
    tab = torch.full((3, 8), 0.123)
    tab[0, 5], tab[0, 7] = GS, phi
    tab[1, 5], tab[1, 7] = 1.5, 0.5
    tab[2, 5], tab[2, 7] = 2.25, 0.45
    return tab


KERNEL_SHAPES = [(3, 8, 8, 16), (3, 1, 17, 59), (2, 1, 1, 3), (1, 1, 41, 100), (1, 16, 192, 32)]


@pytest.mark.parametrize("offset", [0.0, 50.0], ids=["offset0", "offset50"])
@pytest.mark.parametrize("phi", [0.7, 1.0])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["1024", "1003", "3", "4100", "98304"])
def test_kernel_matches_fp64(shape, phi, offset):
    from audioldm2_amd import ops
    eps_h, tab_h = kernel_inputs(shape, offset), table(phi)
    eps, tab = eps_h.cuda(), tab_h.cuda()
    if shape == (3, 1, 17, 59):
        assert (eps[0, 1].data_ptr() % 16) != 0   # unaligned sample bases
    for row in (0, 2):
        s, p = float(tab_h[row, 5]), float(tab_h[row, 7])   # the fp32 values the kernel reads
        idx = torch.full((1,), row, device="cuda", dtype=torch.int32)
        out = torch.full(shape, float("nan"), device="cuda")
        assert ops.cfg_rescale_indexed(eps, out, tab, idx) is out
        ref64, ref32 = rescale_formula(eps_h, s, p, torch.float64), rescale_formula(eps_h, s, p, torch.float32)
        ek, et = relmax(out, ref64), relmax(ref32, ref64)
        print(f"cfg_rescale kernel {shape} phi={p:.2f} s={s} offset={offset}: kernel {ek:.2e} / torch fp32 {et:.2e}")
        assert log_err(ek, 4 * et, f"cfg_rescale kernel n_s={out[0].numel()} row={row} offset={offset}") <= 4 * et
        assert torch.equal(eps.cpu(), eps_h) and torch.equal(tab.cpu(), tab_h)
        again = torch.empty_like(out)
        ops.cfg_rescale_indexed(eps, again, tab, idx)
        assert torch.equal(out, again)
        if row == 0:   # no counter: row 0
            ops.cfg_rescale_indexed(eps, again.zero_(), tab)
            assert torch.equal(out, again)


# ---- 2. special values ------------------------------------------------------------------------------------------------------------
def one_row(s, phi):
    tab = torch.zeros(1, 8)
    tab[0, 5], tab[0, 7] = s, phi
    return tab.cuda()


@pytest.mark.parametrize("shape", [(3, 8, 8, 16), (3, 1, 17, 59)], ids=["1024", "1003"])
def test_phi_zero_is_the_plain_combine_and_scale_one_is_e_c(shape):
    from audioldm2_amd import ops
    eps_h = kernel_inputs(shape, 0.0)
    eps = eps_h.cuda()
    for s, phi, want in ((GS, 0.0, lambda e: e[0] + GS * (e[1] - e[0])), (1.0, PHI, lambda e: e[1])):
        out = ops.cfg_rescale_indexed(eps, torch.empty(shape, device="cuda"), one_row(s, phi))
        ref64 = rescale_formula(eps_h, s, phi, torch.float64)
        bar = 4 * relmax(rescale_formula(eps_h, s, phi, torch.float32), ref64)
        ek, ew = relmax(out, ref64), relmax(out, want(eps_h.double()))
        print(f"cfg_rescale s={s} phi={phi} {shape}: vs fp64 {ek:.2e}, vs the closed form {ew:.2e}, bar {bar:.2e}")
        assert log_err(ek, bar, f"cfg_rescale s={s} phi={phi}") <= bar and ew <= bar


def test_zero_sample_and_single_element_give_factor_one():
    from audioldm2_amd import ops
    eps_h = kernel_inputs((3, 8, 8, 16), 0.0)
    eps_h[:, 1] = 0.0                                   # sample 1: e_u and e_c all zero, std(e_g) == 0
    out = ops.cfg_rescale_indexed(eps_h.cuda(), torch.empty(3, 8, 8, 16, device="cuda"), one_row(GS, PHI))
    assert bool(torch.isfinite(out).all()) and bool((out[1] == 0).all())
    ref = rescale_formula(eps_h, GS, PHI, torch.float64)
    assert relmax(out, ref) <= 4 * relmax(rescale_formula(eps_h, GS, PHI, torch.float32), ref)
    # a constant non-zero sample has std(e_g) == 0 too: f = 1, the plain combine
    const = torch.stack([torch.full((1, 1, 4, 8), 2.0), torch.full((1, 1, 4, 8), 3.0)]).cuda()
    out = ops.cfg_rescale_indexed(const, torch.empty(1, 1, 4, 8, device="cuda"), one_row(GS, PHI))
    assert torch.equal(out, torch.full_like(out, 2.0 + GS * (3.0 - 2.0)))
    # n_s == 1
    one = torch.tensor([[-1.5, 0.25], [2.0, 4.0]]).reshape(2, 2, 1, 1, 1).cuda()
    out = ops.cfg_rescale_indexed(one, torch.empty(2, 1, 1, 1, device="cuda"), one_row(GS, PHI))
    want = one[0] + GS * (one[1] - one[0])
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want)


@pytest.mark.parametrize("shape", [(3, 8, 8, 16), (3, 1, 17, 59)], ids=["1024", "1003"])
def test_nan_stays_in_its_sample(shape):
    from audioldm2_amd import ops
    eps = kernel_inputs(shape, 0.0).cuda()
    clean = ops.cfg_rescale_indexed(eps, torch.empty(shape, device="cuda"), one_row(GS, PHI))
    bad = eps.clone()
    bad[1, 1].view(-1)[5] = float("nan")               # e_c of sample 1
    out = ops.cfg_rescale_indexed(bad, torch.empty(shape, device="cuda"), one_row(GS, PHI))
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    assert bool(torch.isnan(out[1]).all())            # non-finite inputs propagate: through the statistics to the whole sample


# ---- 3. wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_checks_its_tensors():
    from audioldm2_amd import ops
    shape = (2, 1, 5, 24)
    eps, out, tab = torch.randn((2,) + shape).cuda(), torch.empty(shape).cuda(), one_row(GS, PHI)
    idx = torch.zeros(1, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.cfg_rescale_indexed(eps.cpu(), out, tab, idx)
    with pytest.raises(RuntimeError, match=r"out \[B, \.\.\.\]"):
        ops.cfg_rescale_indexed(eps, out[:, :, :4].contiguous(), tab, idx)
    with pytest.raises(RuntimeError, match="int32"):
        ops.cfg_rescale_indexed(eps, out, tab, idx.long())
    with pytest.raises(RuntimeError, match="coef_ld=7"):
        ops.cfg_rescale_indexed(eps, out, tab[:, :7].contiguous(), idx)
    big = torch.randn(3 * out.numel()).cuda()
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.cfg_rescale_indexed(big[:2 * out.numel()].view((2,) + shape), big[out.numel():2 * out.numel()].view(shape), tab, idx)
    ops.cfg_rescale_indexed(big[:2 * out.numel()].view((2,) + shape), big[2 * out.numel():].view(shape), tab, idx)   # adjacent: fine


# ---- 4. the samplers on the tiny UNet -------------------------------------------------------------------------------------------
class TinyModel:
    """What a sampler touches on its model (num_timesteps, alphas_cumprod, apply_model, prepare_cfg, apply_model_cfg) over the tiny
    UNet of test_model_gpu's `unet_tiny`; conditioning = (contexts, masks)."""
    num_timesteps = 1000

    def __init__(self):
        from audioldm2_amd.unet import UNetModel
        self.unet = UNetModel(**cases.UNET_TINY)
        self.unet.load_state_dict(weights.make_state_dict(weights.shapes_of(self.unet), seed=0))
        self.unet.cuda()
        betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()

    def apply_model(self, x, t, cond):
        return self.unet(x.contiguous(), t, context_list=cond[0], context_attn_mask_list=cond[1])

    def prepare_cfg(self, cond, uncond):
        return {"ctxs": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[0], cond[0])],
                "masks": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[1], cond[1])]}

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        p = prepared or self.prepare_cfg(cond, uncond)
        eps = self.unet(x.repeat(2, 1, 1, 1).contiguous(), t2, context_list=p["ctxs"], context_attn_mask_list=p["masks"])
        return eps.view(2, x.shape[0], *eps.shape[1:])


TINY_SHAPE = (2, 8, 16, 8)


@pytest.fixture(scope="module")
def tiny():
    m = TinyModel()
    B = TINY_SHAPE[0]
    _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=1)
    _, _, uctx, umask, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=2)
    cond = ([c.cuda() for c in ctxs], [k.cuda() for k in masks])
    uncond = ([c.cuda() for c in uctx], [k.cuda() for k in umask])
    return m, cond, uncond


def x_T(seed=3, shape=TINY_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def ddim_update(x, e, c, dt):
    """x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t); x = sqrt(a_prev) x0 + sqrt(1 - a_prev) e (eta = 0); c = those four square roots"""
    x, e = x.to(dt), e.to(dt)
    c = [v.to(dt) for v in c]
    p0 = (x - c[0] * e) / c[1]
    return c[3] * p0 + c[2] * e, p0


def plms_combine(e, olds):
    if len(olds) == 0:
        return e
    if len(olds) == 1:
        return (3 * e - olds[0]) / 2
    if len(olds) == 2:
        return (23 * e - 16 * olds[0] + 5 * olds[1]) / 12
    return (55 * e - 59 * olds[0] + 37 * olds[1] - 9 * olds[2]) / 24


def dpm_update(x, e, old, c, dt):
    """c = {sigma_t, alpha_t, sigma_prev / sigma_t, -alpha_prev expm1(-h), w}"""
    x, e = x.to(dt), e.to(dt)
    c = [v.to(dt) for v in c]
    p0 = (x - c[0] * e) / c[1]
    d = p0 if float(c[4]) == 0.0 else p0 + c[4] * (p0 - old.to(dt))
    return c[2] * x + c[3] * d, p0


def fp64_loop(kind, model_cfg, ac, ts, xT, gs=GS, phi=PHI):
    """`kind` in ddim | plms | dpmpp over the ascending timestep subset `ts` with guidance rescale: eps from model_cfg(x fp32, t) ->
    [2, b, ...] on the fp32 image of the fp64 state, the rescaled combine and every other operation in fp64 (the scale and phi as
    the fp32 numbers the table holds).  Returns x and the worst per-step error of the same step evaluated by torch in fp32 with
    fp32 coefficients (the yardstick of the bars)."""
    n = len(ts)
    time_range = np.flip(ts)
    gs, phi = float(torch.tensor(gs, dtype=torch.float32)), float(torch.tensor(phi, dtype=torch.float32))
    x = xT.double().cuda()
    olds, old_p0, h_last, e32 = [], None, None, 0.0
    for i, t in enumerate(time_range):
        index = n - i - 1
        a_t = ac[ts[index]].double()
        a_p = (ac[ts[index - 1]] if index > 0 else ac[0]).double()
        eps = model_cfg(x.float(), float(t))
        e, e_32 = rescale_formula(eps, gs, phi, torch.float64), rescale_formula(eps, gs, phi, torch.float32)
        if kind == "dpmpp":
            al_t, sg_t, al_p, sg_p = a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()
            h = torch.log(al_p / sg_p) - torch.log(al_t / sg_t)
            w = torch.zeros((), dtype=torch.float64) if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
            c64 = [sg_t, al_t, sg_p / sg_t, -al_p * torch.expm1(-h), w]
            x_new, p0 = dpm_update(x, e, old_p0, c64, torch.float64)
            x_32, _ = dpm_update(x, e_32, old_p0, [v.float() for v in c64], torch.float32)
            old_p0, h_last = p0, h
        else:
            c64 = [(1 - a_t).sqrt(), a_t.sqrt(), (1 - a_p).sqrt(), a_p.sqrt()]
            c32 = [v.float() for v in c64]
            if kind == "plms" and i == 0:
                x_tmp, _ = ddim_update(x, e, c64, torch.float64)
                e_next = rescale_formula(model_cfg(x_tmp.float(), float(time_range[min(1, n - 1)])), gs, phi, torch.float64)
                ep, ep_32 = (e + e_next) / 2, (e_32 + e_next.float()) / 2
            elif kind == "plms":
                ep, ep_32 = plms_combine(e, olds[:3]), plms_combine(e_32, [o.float() for o in olds[:3]])
            else:
                ep, ep_32 = e, e_32
            x_new, _ = ddim_update(x, ep, c64, torch.float64)
            x_32, _ = ddim_update(x, ep_32, c32, torch.float32)
            olds.insert(0, e)
        e32 = max(e32, relmax(x_32, x_new))
        x = x_new
    return x, e32


def make_sampler(kind, m):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp": DPMSolverSampler}[kind](m)


def run_sampler(kind, m, cond, uncond, S, xT, sampler=None, **kw):
    s = sampler or make_sampler(kind, m)
    return s.sample(S, TINY_SHAPE[0], TINY_SHAPE[1:], cond, verbose=False, x_T=xT, eta=0.0, unconditional_guidance_scale=GS,
                    unconditional_conditioning=uncond, **kw)[0]


@pytest.mark.parametrize("kind", ["ddim", "plms", "dpmpp"])
def test_sampler_matches_fp64_loop_graph_equals_eager_and_phi_zero_is_today(tiny, kind, monkeypatch):
    """S = 6 makes seven steps: the first runs eagerly, the graph is captured at the next replayable step and replayed after."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    m, cond, uncond = tiny
    b = TINY_SHAPE[0]
    ts = make_ddim_timesteps("uniform", 6, 1000)
    steps = len(ts)
    assert steps == 7
    model_cfg = lambda xx, t: m.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), cond, uncond)
    ref, e32 = fp64_loop(kind, model_cfg, m.alphas_cumprod, ts, x_T())
    out = run_sampler(kind, m, cond, uncond, 6, x_T(), guidance_rescale=PHI)
    plain = run_sampler(kind, m, cond, uncond, 6, x_T())
    zero = run_sampler(kind, m, cond, uncond, 6, x_T(), guidance_rescale=0.0)
    ex, bar = relmax(out, ref), 4 * e32 * steps
    print(f"guidance rescale {kind} sampler, 7 steps: x {ex:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}  "
          f"(phi 0.7 vs phi 0: {relmax(out, plain):.2e})")
    assert log_err(ex, bar, f"guidance rescale {kind} sampler x") <= bar
    assert torch.equal(zero, plain), "phi = 0 must be the sampler without the argument"
    assert relmax(out, plain) > 1e-3
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    eager = make_sampler(kind, m)
    assert not eager.use_graph
    out_e = run_sampler(kind, m, cond, uncond, 6, x_T(), sampler=eager, guidance_rescale=PHI)
    assert torch.equal(out, out_e), "graph replay and eager launches must agree bitwise"


def test_ddim_eager_step_and_decode_take_the_argument(tiny):
    """p_sample_ddim / decode with guidance_rescale: the eager forms over the same two kernels equal the sampling loop's last
    steps (eta = 0: the step noise is multiplied by sigma = 0)."""
    m, cond, uncond = tiny
    s = make_sampler("ddim", m)
    s.make_schedule(6, ddim_eta=0.0, verbose=False)
    x = x_T(4).cuda()
    kw = dict(unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    torch.manual_seed(0)
    dec = s.decode(x, cond, 3, guidance_rescale=PHI, **kw)
    dec0 = s.decode(x, cond, 3, **kw)
    loop, _ = s.ddim_sampling(cond, TINY_SHAPE, x_T=x.cpu(), timesteps=4, guidance_rescale=PHI, **kw)
    assert torch.equal(dec, loop) and not torch.equal(dec, dec0)


# ---- 5. LatentDiffusion at a small latent ---------------------------------------------------------------------------------------
LATENT_T = 64


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    ld = build_model(model_name="audioldm2-full")
    with open(os.path.join(GOLD, "e2e_statedict_keys.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = weights.make_state_dict(shapes, seed=0)
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    ld.load_state_dict(sd, strict=False)
    return ld.cuda()


def generate(ld, batch=None, steps=4, **kw):
    """One job from seed 42 as a fresh object's first call; records the latent handed to the decoder and the next draw of the
    host generator."""
    from audioldm2_amd.pipeline import seed_everything
    rec = {}
    orig = ld.decode_first_stage_cl

    def hook(z):
        rec["latent"] = z.clone()
        return orig(z)
    ld.decode_first_stage_cl = hook
    try:
        seed_everything(cases.E2E_SEED)
        ld.latent_t_size = LATENT_T
        ld.conditional_dry_run_finished = False
        args = dict(ddim_eta=0.0, unconditional_guidance_scale=GS, n_gen=1, duration=2.5, ddim_steps=steps)
        args.update(kw)
        rec["wave"] = ld.generate_batch(cases.e2e_batch(2) if batch is None else batch, **args)
        rec["rand_after"] = float(torch.rand(1))
    finally:
        ld.decode_first_stage_cl = orig
    return rec


def test_two_rescaled_ddim_jobs_share_one_graph_and_plain_jobs_are_untouched(ld):
    """The cache key carries "rescale on / off", the values of the scale and phi live in the coefficient table that is copied into
    a reused entry: a second job with another (scale, phi) on the cached graph equals that job on a model with nothing cached,
    and a plain job after a rescaled one equals a plain job on a model with nothing cached — all bitwise."""
    unet = ld.model.diffusion_model
    job_a = lambda: generate(ld, ddim_eta=1.0, guidance_rescale=0.7)["latent"]
    job_b = lambda: generate(ld, ddim_eta=1.0, guidance_rescale=0.3, unconditional_guidance_scale=2.5)["latent"]
    plain = lambda: generate(ld, ddim_eta=1.0)["latent"]
    unet.drop_step_caches()
    a_fresh = job_a()
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    b_hit = job_b()
    assert next(iter(unet._graph_cache.values())) is ent
    a_hit = job_a()
    assert next(iter(unet._graph_cache.values())) is ent
    plain_after = plain()                     # another launch sequence: its own entry
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is not ent
    unet.drop_step_caches()
    b_fresh = job_b()
    unet.drop_step_caches()
    plain_fresh = plain()
    unet.drop_step_caches()
    assert torch.equal(a_hit, a_fresh) and torch.equal(b_hit, b_fresh) and torch.equal(plain_after, plain_fresh)
    assert not torch.equal(a_fresh, b_fresh) and not torch.equal(a_fresh, plain_fresh)
    assert bool(torch.isfinite(a_fresh).all())


@pytest.mark.parametrize("how", [dict(), dict(use_plms=True), dict(sampler="dpmpp_2m")], ids=["ddim", "plms", "dpmpp"])
def test_one_rank_shard_equals_the_unsharded_job(ld, how):
    a = generate(ld, guidance_rescale=PHI, **how)
    b = generate(ld, guidance_rescale=PHI, shard=(0, 1), **how)
    c = generate(ld, **how)
    assert torch.equal(a["latent"], b["latent"]) and np.array_equal(a["wave"], b["wave"]) and a["rand_after"] == b["rand_after"]
    assert not torch.equal(a["latent"], c["latent"]) and a["rand_after"] == c["rand_after"]   # the rescale draws nothing


def test_text_to_audio_takes_guidance_rescale(ld):
    from audioldm2_amd.pipeline import text_to_audio
    kw = dict(seed=7, ddim_steps=4, duration=2.5, batchsize=1, n_candidate_gen_per_text=1, sampler="dpmpp_2m")

    def job(**more):
        ld.conditional_dry_run_finished = False   # every call as an object's first (pipeline._cfg_dropout_draw)
        return text_to_audio(ld, "a dog barking", **kw, **more)
    a, b, c = job(guidance_rescale=PHI), job(guidance_rescale=PHI), job()
    assert a.ndim == 3 and a.shape[:2] == (1, 1) and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(c, job(guidance_rescale=0.0))
    with pytest.raises(ValueError, match="guidance_rescale"):
        job(guidance_rescale=1.5)


# ---- 6. negative prompts through the HIP conditioner stack ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ld_cond():
    from audioldm2_amd.pipeline import LatentDiffusion, default_audioldm_config
    with open(os.path.join(GOLD, "e2econd_statedict_keys.json")) as f:
        k = json.load(f)
    hot, cond = {a: tuple(b) for a, b in k["hot"].items()}, {a: tuple(b) for a, b in k["cond"].items()}
    cfg = default_audioldm_config("audioldm2-full", conditioners="hip", t5_config=cases.t5_test_config(),
                                  clap_config=cases.clap_text_test_config())
    cfg["model"]["params"]["build_clap"] = False    # one candidate per prompt: no re-ranker needed
    torch.manual_seed(0)
    ld = LatentDiffusion(**cfg["model"]["params"]).eval()
    sd = weights.make_state_dict(hot, seed=0)
    sd.update(cases.cond_state_dict(cond, seed=0))
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    res = ld.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys[:5]
    ld = ld.cuda()
    seq = ld.cond_stage_models[0]
    seq.cond_stage_models[0].tokenize = cases.StubRobertaTokenizer()
    seq.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    ld.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    return ld


def flat(v):
    if isinstance(v, dict):
        return [t for k in sorted(v) for t in flat(v[k])]
    if isinstance(v, (list, tuple)):
        return [t for e in v for t in flat(e)]
    return [v]


def cond_job(ld, monkeypatch, **kw):
    """generate() on the two-prompt batch with sample_log wrapped: records what it was handed and the generator at its entry."""
    rec = {}
    orig = ld.sample_log

    def wrapped(cond, batch_size, **k):
        rec["rng"] = torch.get_rng_state()
        rec["cond"], rec["uncond"], rec["kwargs"], rec["batch_size"] = cond, k.get("unconditional_conditioning"), k, batch_size
        return orig(cond=cond, batch_size=batch_size, **k)
    monkeypatch.setattr(ld, "sample_log", wrapped, raising=False)
    try:
        rec.update(generate(ld, batch=cases.e2e_cond_batch(), steps=2, **kw))
    finally:
        monkeypatch.undo()
    return rec


NEG = "Low quality."


def test_negative_prompt_is_the_unconditional_half(ld_cond, monkeypatch):
    from audioldm2_amd.pipeline import negative_batch
    ld = ld_cond
    rec = cond_job(ld, monkeypatch, negative_prompt=NEG)
    want = ld.get_learned_conditioning_dict(negative_batch(cases.e2e_cond_batch(), NEG))
    assert sorted(rec["uncond"]) == sorted(want) == sorted(rec["cond"])
    for a, b in zip(flat(rec["uncond"]), flat(want)):
        assert a.shape == b.shape and torch.equal(a, b)
    t5 = rec["uncond"]["crossattn_flan_t5"][0]
    t5_pos = rec["cond"]["crossattn_flan_t5"][0]
    assert 1 < t5.shape[1] < t5_pos.shape[1], (t5.shape, t5_pos.shape)     # prepare_cfg pads the shorter half
    # the job's latent is sample_log on that cond / uncond from the generator state at its entry
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    torch.set_rng_state(rec["rng"])
    by_hand, _ = ld.sample_log(rec["cond"], rec["batch_size"], **rec["kwargs"])
    unet.drop_step_caches()
    steps = 2
    bar = 4 * steps * 2.0 ** -24    # the same launches on the same inputs: expected 0; the bar is 4 fp32 roundings per step
    e = relmax(rec["latent"], by_hand)
    print(f"negative prompt job vs sample_log by hand: {e:.2e} (bar {bar:.2e})")
    assert log_err(e, bar, "negative prompt job vs sample_log by hand") <= bar
    other = cond_job(ld, monkeypatch, negative_prompt="Music.")
    listed = cond_job(ld, monkeypatch, negative_prompt=[NEG, "Music."])
    assert not torch.equal(other["latent"], rec["latent"])
    assert not torch.equal(listed["latent"][1], rec["latent"][1])
    assert all(bool(torch.isfinite(r["latent"]).all()) for r in (rec, other, listed))


def test_no_negative_prompt_is_todays_job(ld_cond, monkeypatch):
    ld = ld_cond
    today = cond_job(ld, monkeypatch)
    none = cond_job(ld, monkeypatch, negative_prompt=None)
    neg = cond_job(ld, monkeypatch, negative_prompt=NEG)
    assert torch.equal(today["latent"], none["latent"]) and today["rand_after"] == none["rand_after"]
    assert torch.equal(torch.as_tensor(today["rng"]), torch.as_tensor(none["rng"]))
    want = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(2) for k, m in ld.cond_stage_model_metadata.items()}
    for a, b in zip(flat(none["uncond"]), flat(want)):
        assert torch.equal(a, b)
    assert not torch.equal(neg["latent"], today["latent"])
    with pytest.raises(ValueError, match="negative_prompt"):
        ld.generate_batch(cases.e2e_cond_batch(), ddim_steps=2, unconditional_guidance_scale=1.0, negative_prompt=NEG, duration=2.5)
