"""The DPM-Solver++(2M) sampler on the GPU (audioldm2_amd/dpm_solver.py, ops.dpmpp_step_indexed):

 1. the step kernel against an fp64 restatement, call by call, the device counter running 0..6 (first order, five second-order
    steps, first-order final), with and without guidance; n = 3072 and 1000 take the 16-byte form, n = 1003 the scalar one;
 2. w = 0 ignores the history slab: a NaN-filled slab gives, bitwise, what a zero-filled one gives;
 3. DPMSolverSampler.sample on the tiny UNet under guidance against a loop written here (eps from apply_model_cfg, arithmetic in
    fp64), graph replay == eager bitwise, two jobs on one object, a `timesteps` sub-range, zero steps;
 4. first order is DDIM: at S = 2 both steps are first order and the output is DDIMSampler's at eta = 0 — the tie to the sampler
    that is pinned on the real reference's fixtures;
 5. end to end: generate_batch / generate_batch_masked / sample_log with sampler="dpmpp_2m".

Bars.  (1), (3), (4) and the masked job: the same formula evaluated by torch in fp32 on the same inputs is measured against fp64 in
the test itself; the bar is 4x that figure ((3), (4): times the number of steps).  The kernel is built without contraction and
keeps the operation order of the formula, so it sits at torch's error.  (5): tolerances.latent_tol(5, mode), the project's bar of a
5-step DDIM latent, and its 1e-3 waveform bars.

Measured on an MI355X (max|err| / max|ref|, worst of the seven calls; kernel / torch fp32):
    3072 elements  plain: x 8.12e-8 / 9.33e-8, x0_buf 7.08e-8 / 9.98e-8;  cfg: x 1.53e-7 / 1.38e-7, x0_buf 1.23e-7 / 1.22e-7
    1000 elements  plain: x 7.75e-8 / 8.86e-8, x0_buf 7.49e-8 / 1.06e-7;  cfg: x 1.33e-7 / 1.44e-7, x0_buf 1.21e-7 / 1.61e-7
    1003 elements  plain: x 7.05e-8 / 8.77e-8, x0_buf 7.71e-8 / 9.46e-8;  cfg: x 1.37e-7 / 1.96e-7, x0_buf 1.38e-7 / 1.56e-7
(3), guidance 3.5, sampler vs fp64 loop (x) / torch fp32 per step / bar: 7 steps 4.02e-7 / 1.85e-7 / 5.18e-6; 1 step 6.82e-8 / 5.64e-8 /
2.26e-7; 3 of 8 steps 1.16e-6 / 2.34e-7 / 2.81e-6.  (4): 2M vs DDIM at S = 2 1.60e-7, bar 8.60e-7.
(5): 2 steps vs DDIM eta 0: latent 1.08e-7 relative rms (bar 1e-5), wave rms error 2.08e-7, between-sample 7.0e-2.  7 steps vs the fp64
loop, latent relative rms: bf16x6 2.67e-7, f16x3 2.60e-7 (bar 1e-5), bf16x3 6.64e-7 (bar 1e-4).  Masked job, kept region: 1.17e-7,
torch fp32 1.17e-7.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, weights
from tolerances import latent_tol, log_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GS = 3.5


def rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


# ---- 1. / 2. kernel -------------------------------------------------------------------------------------------------------------
def dpm_formula(x, e, old, c, dt):
    """One step on tensors of dtype dt in the kernel's operation order; c = {sigma_t, alpha_t, sigma_prev / sigma_t,
    -alpha_prev expm1(-h), w} as 0-dim tensors.  Returns (x_new, x0)."""
    x, e = x.to(dt), e.to(dt)
    c = [v.to(dt) for v in c]
    p0 = (x - c[0] * e) / c[1]
    d = p0 if float(c[4]) == 0.0 else p0 + c[4] * (p0 - old.to(dt))
    return c[2] * x + c[3] * d, p0


def combine(eps, cfg, dt):
    eps = eps.to(dt)
    return eps[0] + GS * (eps[1] - eps[0]) if cfg else eps


def coef_table(S, cfg, seed=0):
    """[S, 8] fp32 rows of aldm_dpmpp_step_indexed from a decreasing-noise abar sequence with uneven steps (so w varies)."""
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    a = torch.linspace(0.05, 0.95, S + 1, dtype=torch.float64) + \
        0.01 * torch.rand(S + 1, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    tab = torch.zeros(S, 8)
    tab[:, :5] = torch.from_numpy(dpmpp_2m_coefficients(a[:-1].numpy(), a[1:].numpy())).float()
    tab[:, 5], tab[:, 6] = GS, 1.0 if cfg else 0.0
    return tab


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("shape", [(3, 8, 8, 16), (1, 8, 5, 25), (1, 1, 17, 59)], ids=["3072", "1000", "1003"])
def test_step_kernel_matches_fp64_call_by_call(shape, cfg):
    from audioldm2_amd import ops
    S = 7
    g = torch.Generator().manual_seed(5)
    dev = "cuda"
    tab_h = coef_table(S, cfg)
    assert [float(w) == 0.0 for w in tab_h[:, 4]] == [True] + [False] * 5 + [True]
    tab = tab_h.to(dev)
    x = torch.randn(shape, generator=g).to(dev)
    eshape = ((2,) if cfg else ()) + shape
    slab = torch.full(shape, 7.0, device=dev)     # step 0 must not read it
    step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
    t_tab = torch.arange(S, dtype=torch.float32, device=dev)[:, None].contiguous()
    t_cur = t_tab[0].clone()
    worst = {"x": [0.0, 0.0], "x0_buf": [0.0, 0.0]}   # [kernel, torch fp32] vs fp64

    def check(what, got, ref64, ref32):
        ek, et = relmax(got, ref64), relmax(ref32, ref64)
        worst[what][0], worst[what][1] = max(worst[what][0], ek), max(worst[what][1], et)
        assert ek <= 4 * et, (what, s, ek, et)

    for s in range(S):
        c = [tab_h[s, j] for j in range(5)]
        eps = torch.randn(eshape, generator=g).to(dev)
        eps_in, x_in, old = eps.clone(), x.clone(), slab.clone()
        assert int(step_idx.item()) == s
        assert ops.dpmpp_step_indexed(x, eps, slab, tab, step_idx) is x
        refs = {dt: dpm_formula(x_in, combine(eps, cfg, dt), old, c, dt) for dt in (torch.float64, torch.float32)}
        check("x", x, refs[torch.float64][0], refs[torch.float32][0])
        check("x0_buf", slab, refs[torch.float64][1], refs[torch.float32][1])
        assert torch.equal(eps, eps_in) and torch.equal(tab, tab_h.to(dev))
        ops.step_advance(step_idx, t_tab, t_cur)
    print(f"dpmpp kernel {shape} cfg={cfg}: " + "  ".join(f"{k} kernel {v[0]:.2e} / torch fp32 {v[1]:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        log_err(v[0], 4 * v[1], f"dpmpp kernel {k} cfg={cfg} n={x.numel()}")


@pytest.mark.parametrize("shape", [(1, 8, 5, 25), (1, 1, 17, 59)], ids=["1000", "1003"])
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_first_order_step_ignores_the_slab(shape, cfg):
    """With w == 0 the old x0_buf element does not enter the arithmetic: a NaN slab gives, bitwise, the result of a zero slab."""
    from audioldm2_amd import ops
    g = torch.Generator().manual_seed(9)
    tab = coef_table(3, cfg).cuda()
    x = torch.randn(shape, generator=g).cuda()
    eps = torch.randn(((2,) if cfg else ()) + shape, generator=g).cuda()
    out = {}
    for name, fill in (("nan", float("nan")), ("zero", 0.0)):
        xx, slab = x.clone(), torch.full(shape, fill, device="cuda")
        ops.dpmpp_step_indexed(xx, eps, slab, tab, torch.zeros(1, device="cuda", dtype=torch.int32))
        out[name] = (xx, slab)
    assert bool(torch.isfinite(out["nan"][0]).all()) and bool(torch.isfinite(out["nan"][1]).all())
    assert torch.equal(out["nan"][0], out["zero"][0]) and torch.equal(out["nan"][1], out["zero"][1])
    assert not torch.equal(out["nan"][0], x)
    # ... and a second-order row does read it
    xx, slab = x.clone(), torch.full(shape, float("nan"), device="cuda")
    ops.dpmpp_step_indexed(xx, eps, slab, tab, torch.ones(1, device="cuda", dtype=torch.int32))
    assert bool(torch.isnan(xx).all()) and bool(torch.isfinite(slab).all())


def test_wrapper_checks_its_tensors():
    from audioldm2_amd import ops
    shape = (1, 8, 5, 25)
    x, eps, slab = torch.randn(shape).cuda(), torch.randn(shape).cuda(), torch.zeros(shape).cuda()
    tab, idx = coef_table(2, False).cuda(), torch.zeros(1, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.dpmpp_step_indexed(x.cpu(), eps, slab, tab, idx)
    with pytest.raises(AssertionError):
        ops.dpmpp_step_indexed(x, eps, slab[:, :4].contiguous(), tab, idx)
    with pytest.raises(AssertionError):
        ops.dpmpp_step_indexed(x, eps, slab, tab, idx.long())
    with pytest.raises(RuntimeError, match="coef_ld=6"):
        ops.dpmpp_step_indexed(x, eps, slab, tab[:, :6].contiguous(), idx)


# ---- 3. / 4. sampler on the tiny UNet -------------------------------------------------------------------------------------------
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


def step_rows(ac, ts):
    """fp64 rows {sigma_t, alpha_t, sigma_prev / sigma_t, -alpha_prev expm1(-h), w} over the ascending timestep subset `ts` of
    the fp32 schedule `ac`, in loop order, straight from the formulas (first order: step 0, and the last step of a run under 15)."""
    n = len(ts)
    rows, h_last = [], None
    for i in range(n):
        index = n - i - 1
        a_t = float(ac[ts[index]])
        a_p = float(ac[ts[index - 1]]) if index > 0 else float(ac[0])
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        w = 0.0 if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
        rows.append([sg_t, al_t, sg_p / sg_t, -al_p * np.expm1(-h), w])
        h_last = h
    return torch.tensor(rows, dtype=torch.float64)


def fp64_loop(model_cfg, ac, ts, xT, gs=GS):
    """DPM-Solver++(2M) over `ts`: eps from model_cfg(x fp32, t) -> [2, b, ...] on the fp32 image of the fp64 state, every other
    operation in fp64 with unrounded coefficients.  Returns x, the last x0 and the worst per-step error of the same step evaluated
    by torch in fp32 with the coefficients rounded to fp32 (the yardstick of the bars)."""
    rows = step_rows(ac, ts)
    time_range = np.flip(ts)
    x = xT.double().cuda()
    old, p0, e32 = None, None, 0.0
    for i, t in enumerate(time_range):
        eps = model_cfg(x.float(), float(t))
        e = eps[0].double() + gs * (eps[1].double() - eps[0].double())
        e_32 = eps[0] + gs * (eps[1] - eps[0])
        c64 = [rows[i, j] for j in range(5)]
        c32 = [rows[i, j].float() for j in range(5)]
        x_new, p0 = dpm_formula(x, e, old, c64, torch.float64)
        x_32, _ = dpm_formula(x, e_32, old, c32, torch.float32)
        e32 = max(e32, relmax(x_32, x_new))
        old, x = p0, x_new
    return x, p0, e32


def tiny_model_cfg(m, cond, uncond):
    b = TINY_SHAPE[0]
    return lambda xx, t: m.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), cond, uncond)


def run_sampler(m, cond, uncond, S, xT, sampler=None, **kw):
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    s = sampler or DPMSolverSampler(m)
    return s.sample(S, TINY_SHAPE[0], TINY_SHAPE[1:], cond, verbose=False, x_T=xT, unconditional_guidance_scale=GS,
                    unconditional_conditioning=uncond, **kw)


@pytest.mark.parametrize("S,steps", [(6, 7), (1, 1)])
def test_sampler_matches_fp64_loop_and_graph_equals_eager(tiny, S, steps, monkeypatch):
    """S = 6 makes seven steps (make_ddim_timesteps: range(0, 1000, 1000 // 6)): first order, five second-order steps, first-order
    final; step 0 runs eagerly, the graph is captured at step 1 and replayed five times.  S = 1: one eager step."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    m, cond, uncond = tiny
    ts = make_ddim_timesteps("uniform", S, 1000)
    assert len(ts) == steps
    ref, ref_p0, e32 = fp64_loop(tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, ts, x_T())
    out, inter = run_sampler(m, cond, uncond, S, x_T(), log_every_t=1)
    ex, ep = relmax(out, ref), relmax(inter["pred_x0"][-1], ref_p0)
    bar = 4 * e32 * steps
    print(f"dpmpp sampler S={S} ({steps} steps): x {ex:.2e} pred_x0 {ep:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert len(inter["x_inter"]) == steps + 1 and torch.equal(inter["x_inter"][-1], out)
    assert log_err(ex, bar, f"dpmpp sampler x S={S}") <= bar and ep <= bar
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    eager = DPMSolverSampler(m)
    assert not eager.use_graph
    out_e, _ = run_sampler(m, cond, uncond, S, x_T(), sampler=eager)
    assert torch.equal(out, out_e), "graph replay and eager launches must agree bitwise"


def test_sampler_timesteps_subrange_three_steps_and_zero_steps(tiny):
    """`timesteps` keeps the first int(min(timesteps / S, 1) * S) - 1 entries of the schedule, as in DDIM and PLMS; the sub-range
    is a run of its own: its first and its last step are first order."""
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    m, cond, uncond = tiny
    s = DPMSolverSampler(m)
    s.make_schedule(8, verbose=False)
    kw = dict(unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    out, inter = s.dpm_sampling(cond, TINY_SHAPE, x_T=x_T(), timesteps=4, **kw)
    ref, _, e32 = fp64_loop(tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, s.ddim_timesteps[:3], x_T())
    ex = relmax(out, ref)
    print(f"dpmpp sampler sub-range (3 of 8 steps): x {ex:.2e}  torch fp32 per step {e32:.2e}")
    assert ex <= 4 * e32 * 3
    out0, inter0 = s.dpm_sampling(cond, TINY_SHAPE, x_T=x_T(), timesteps=1, **kw)
    assert torch.equal(out0.cpu(), x_T()) and len(inter0["x_inter"]) == 1


def test_second_job_on_one_sampler_equals_a_fresh_one(tiny):
    """No stale slab, counter or graph: job B after job A on one object == job B on a new object, bitwise; callbacks see every step."""
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    m, cond, uncond = tiny
    s = DPMSolverSampler(m)
    run_sampler(m, cond, uncond, 6, x_T(11), sampler=s)
    seen = []
    b_used, _ = run_sampler(m, cond, uncond, 4, x_T(12), sampler=s, callback=seen.append,
                            img_callback=lambda p, i: seen.append(tuple(p.shape)))
    b_fresh, _ = run_sampler(m, cond, uncond, 4, x_T(12))
    assert torch.equal(b_used, b_fresh)
    assert seen == [v for i in range(4) for v in (i, TINY_SHAPE)]


def test_first_order_is_ddim_at_eta_zero(tiny):
    """S = 2: step 0 is first order and so is the final step of a run under 15 steps; a first-order step is algebraically DDIM's
    eta = 0 step, so the two samplers agree from the same x_T within the bar of the fp64 comparison."""
    from audioldm2_amd.ddim import DDIMSampler, make_ddim_timesteps
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    m, cond, uncond = tiny
    s = DPMSolverSampler(m)
    out, _ = run_sampler(m, cond, uncond, 2, x_T(), sampler=s)
    assert s.dpm_coef.shape == (2, 5) and float(s.dpm_coef[:, 4].abs().max()) == 0.0
    ddim, _ = DDIMSampler(m).sample(2, TINY_SHAPE[0], TINY_SHAPE[1:], cond, verbose=False, x_T=x_T(), eta=0.0,
                                    unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    _, _, e32 = fp64_loop(tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, make_ddim_timesteps("uniform", 2, 1000), x_T())
    ed, bar = relmax(out, ddim), 4 * e32 * 2
    print(f"dpmpp S=2 vs DDIM eta 0: {ed:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert log_err(ed, bar, "dpmpp first order vs ddim") <= bar


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
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


def generate(ld, masked=False, steps=2, **kw):
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
        ld.latent_t_size = 256
        ld.conditional_dry_run_finished = False
        args = dict(ddim_eta=0.0, unconditional_guidance_scale=GS, n_gen=1, duration=10, ddim_steps=steps)
        args.update(kw)
        if masked:
            rec["wave"] = ld.generate_batch_masked(cases.e2e_masked_batch(1), **args)
        else:
            rec["wave"] = ld.generate_batch(cases.e2e_batch(2), **args)
        rec["rand_after"] = float(torch.rand(1))
    finally:
        ld.decode_first_stage_cl = orig
    return rec


def test_e2e_two_steps_equal_ddim_at_eta_zero(ld):
    """generate_batch(sampler="dpmpp_2m", ddim_steps=2, ddim_eta=0.0) against generate_batch(ddim_steps=2, ddim_eta=0.0) under the
    same seed (both steps first order = DDIM): conditioners, x_T draw, sampler, VAE decode, vocoder."""
    ref = generate(ld)
    rec = generate(ld, sampler="dpmpp_2m")
    assert rec["wave"].shape == ref["wave"].shape == (2, 1, 163872) and rec["wave"].dtype == np.float32
    el = rms((rec["latent"] - ref["latent"]).double().cpu().numpy()) / rms(ref["latent"].double().cpu().numpy())
    ew = rms(rec["wave"].astype(np.float64) - ref["wave"])
    between = rms(ref["wave"][0].astype(np.float64) - ref["wave"][1])
    print(f"dpmpp e2e 2 steps B=2 vs DDIM eta 0: latent rel rms {el:.2e} (bar {latent_tol(5):.1e})  wave rms_err {ew:.3e} / "
          f"between-sample {between:.3e}")
    assert log_err(el, latent_tol(5), "dpmpp latent 2 steps vs ddim") < latent_tol(5)
    assert between > 1e-2 and ew < 1e-3 and ew < 1e-3 * between, (ew, between)


def e2e_conditioning(ld, B):
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
              for k, m in ld.cond_stage_model_metadata.items()}
    return cond, uncond


E2E_SHAPE = (2, 8, 256, 16)


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3", "bf16x3"])
def test_e2e_seven_steps_match_the_fp64_loop(ld, mode):
    """A 7-step job (ddim_steps=6) through sample_log in each matrix-core mode against the fp64 loop over the model's own
    apply_model_cfg in that mode."""
    from audioldm2_amd import ops
    from audioldm2_amd.ddim import make_ddim_timesteps
    unet = ld.model.diffusion_model
    ld.latent_t_size = 256
    cond, uncond = e2e_conditioning(ld, 2)
    xT = x_T(21, E2E_SHAPE)
    prev = ops.set_mma(mode)
    unet.drop_step_caches()
    try:
        out, _ = ld.sample_log(cond=cond, batch_size=2, ddim=True, ddim_steps=6, eta=0.0, unconditional_guidance_scale=GS,
                               unconditional_conditioning=uncond, sampler="dpmpp_2m", x_T=xT)
        prepared = ld.prepare_cfg(cond, uncond)
        ts = make_ddim_timesteps("uniform", 6, 1000)
        ref, _, e32 = fp64_loop(lambda xx, t: ld.apply_model_cfg(xx, torch.full((4,), t, device="cuda"), prepared=prepared),
                                ld.alphas_cumprod.detach().float().cpu(), ts, xT)
    finally:
        ops.set_mma(prev)
        unet.drop_step_caches()
    assert len(ts) == 7
    el = rms((out.double() - ref).cpu().numpy()) / rms(ref.cpu().numpy())
    print(f"dpmpp e2e 7 steps B=2 [{mode}] vs fp64 loop: latent rel rms {el:.2e} (bar {latent_tol(5, mode):.1e})  torch fp32 per step {e32:.2e}")
    assert log_err(el, latent_tol(5, mode), "dpmpp latent 7 steps vs fp64 loop") < latent_tol(5, mode)


def test_e2e_masked_region_follows_x0(ld, monkeypatch):
    """generate_batch_masked(sampler="dpmpp_2m"), 4 steps, B = 1.  Where mask == 1 the last step starts from q_sample(x0, t_last)
    — the blend runs between the steps, its draw first — and is first order (a run under 15 steps), so the final latent there is a
    known function of x0, the last q_sample draw and the last model output.  The blend's operands and the model output are
    recorded (eagerly: ALDM_NO_GRAPH=1, which the sampler tests show to be bitwise the replayed path); the bar is 4x what torch
    makes of the same two formulas in fp32."""
    from audioldm2_amd import ops
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    blends, passes = [], []
    blend, model_cfg = ops.inpaint_blend, ld.apply_model_cfg

    def blend_hook(x, x0, qnoise, mask, coef):
        blends.append((x0.clone(), qnoise.clone(), mask.clone(), coef.clone()))
        return blend(x, x0, qnoise, mask, coef)

    def model_hook(*a, **k):
        eps = model_cfg(*a, **k)
        passes.append(eps.clone())
        return eps
    monkeypatch.setattr(ops, "inpaint_blend", blend_hook)
    monkeypatch.setattr(ld, "apply_model_cfg", model_hook, raising=False)
    rec = generate(ld, masked=True, steps=4, sampler="dpmpp_2m", unconditional_guidance_scale=2.5)
    assert rec["wave"].shape == (1, 1, 163872) and np.isfinite(rec["wave"]).all()
    assert len(blends) == 4 and len(passes) == 4
    x0, n, mask, bc = blends[-1]
    keep = mask == 1
    assert 0 < int(keep.sum()) < mask.numel()
    ac = ld.alphas_cumprod.detach().float().cpu()
    row = step_rows(ac, np.asarray([1]))[0]      # the last step: abar[1] -> abar[0], first order
    assert float(row[4]) == 0.0
    res = {}
    for dt in (torch.float64, torch.float32):
        xb = bc[0].to(dt) * x0.to(dt) + bc[1].to(dt) * n.to(dt)
        e = passes[-1][0].to(dt) + 2.5 * (passes[-1][1].to(dt) - passes[-1][0].to(dt))
        res[dt] = dpm_formula(xb, e, None, [row[j].to(dt).cuda() for j in range(5)], dt)[0][keep]
    assert relmax(bc.cpu(), torch.stack([ac[1].sqrt(), (1 - ac[1]).sqrt()])) == 0.0
    ek, et = relmax(rec["latent"][keep], res[torch.float64]), relmax(res[torch.float32], res[torch.float64])
    print(f"dpmpp masked 4 steps B=1: kept region vs fp64 {ek:.2e}  torch fp32 {et:.2e}")
    assert log_err(ek, 4 * et, "dpmpp masked kept region") <= 4 * et
    # ... and only there: the regenerated region is not q_sample(x0)
    full = dpm_formula(bc[0].double() * x0.double() + bc[1].double() * n.double(),
                       passes[-1][0].double() + 2.5 * (passes[-1][1].double() - passes[-1][0].double()), None,
                       [row[j].cuda() for j in range(5)], torch.float64)[0]
    assert relmax(rec["latent"][~keep], full[~keep]) > 1e-2


def test_ddim_job_after_a_dpmpp_job_equals_ddim_on_a_fresh_model(ld):
    """A 2M run neither reads nor writes the UNet's DDIM graph cache: a DDIM job after it equals, bitwise, the same job without it
    — through the graph an earlier DDIM job cached, and on a model with nothing cached."""
    from audioldm2_amd.pipeline import seed_everything
    unet = ld.model.diffusion_model

    def ddim():
        seed_everything(cases.E2E_SEED)
        ld.latent_t_size = 256
        ld.conditional_dry_run_finished = False
        return ld.generate_batch(cases.e2e_batch(2), unconditional_guidance_scale=3.5, ddim_steps=4, n_gen=1, duration=10)
    unet.drop_step_caches()
    fresh = ddim()                       # nothing cached: as on a fresh model
    hit = ddim()                         # through the graph the first job cached
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    generate(ld, steps=4, sampler="dpmpp_2m")
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    hit_after = ddim()
    assert next(iter(unet._graph_cache.values())) is ent and np.array_equal(hit, hit_after)
    unet.drop_step_caches()
    generate(ld, steps=4, sampler="dpmpp_2m")
    assert len(unet._graph_cache) == 0
    fresh_after = ddim()
    unet.drop_step_caches()
    assert np.array_equal(fresh, fresh_after)


def test_one_rank_shard_equals_the_unsharded_job(ld):
    """shard=(0, 1): the sharded code path draws the global batch and keeps its rows — the same latent, bitwise."""
    a = generate(ld, steps=4, sampler="dpmpp_2m")
    b = generate(ld, steps=4, sampler="dpmpp_2m", shard=(0, 1))
    assert torch.equal(a["latent"], b["latent"]) and np.array_equal(a["wave"], b["wave"])
    assert a["rand_after"] == b["rand_after"]


def test_host_generator_is_where_one_x_T_draw_leaves_it(ld, monkeypatch):
    """The sampler consumes the host generator for x_T and nothing else (no inpainting here): around DPMSolverSampler.sample the
    generator advances by exactly one torch.randn of the latent shape, whatever the number of steps."""
    from audioldm2_amd import dpm_solver
    states = []
    orig = dpm_solver.DPMSolverSampler.sample

    def wrapped(self, S, batch_size, shape, *a, **k):
        before = torch.get_rng_state()
        out = orig(self, S, batch_size, shape, *a, **k)
        after = torch.get_rng_state()
        torch.set_rng_state(before)
        torch.randn((batch_size,) + tuple(shape))
        states.append(torch.equal(torch.get_rng_state(), after))
        torch.set_rng_state(after)
        return out
    monkeypatch.setattr(dpm_solver.DPMSolverSampler, "sample", wrapped)
    r2 = generate(ld, steps=2, sampler="dpmpp_2m")
    r6 = generate(ld, steps=6, sampler="dpmpp_2m")
    assert states == [True, True]
    assert r2["rand_after"] == r6["rand_after"]
    assert not torch.equal(r2["latent"], r6["latent"])


def test_surface(ld):
    ld.latent_t_size = 256
    with pytest.raises(ValueError, match="ddim_eta must equal 0"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=4, sampler="dpmpp_2m", duration=10)          # default ddim_eta = 1.0
    with pytest.raises(ValueError, match="needs ddim_steps"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=None, ddim_eta=0.0, sampler="dpmpp_2m", duration=10)
    with pytest.raises(ValueError, match="unknown sampler"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=4, ddim_eta=0.0, sampler="dpm", duration=10)


def test_text_to_audio_takes_the_sampler_by_name(ld):
    """The entry point has no eta parameter: eta 0 travels with the name.  Deterministic under its seed; not the DDIM clip."""
    from audioldm2_amd.pipeline import text_to_audio
    kw = dict(seed=7, ddim_steps=4, duration=10, batchsize=1, n_candidate_gen_per_text=1)

    def job(**more):
        ld.conditional_dry_run_finished = False   # every call as an object's first (pipeline._cfg_dropout_draw)
        return text_to_audio(ld, "a dog barking", **kw, **more)
    a, b, c = job(sampler="dpmpp_2m"), job(sampler="dpmpp_2m"), job()
    assert a.shape == (1, 1, 163872) and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
