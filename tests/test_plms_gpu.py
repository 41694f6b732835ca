"""The PLMS sampler on the GPU (audioldm2_amd/plms.py, ops.plms_first_step / ops.plms_step_indexed):

 1. the two step kernels against an fp64 restatement, call by call, the device counter running 0..6 so the ring wraps twice;
 2. PLMSSampler.sample on the tiny UNet under guidance against a loop written here (eps from apply_model_cfg, arithmetic in fp64),
    graph replay == eager bitwise, short runs, a `timesteps` sub-range, two jobs on one object;
 3. generate_batch / generate_batch_masked (use_plms=True) against the REAL reference's fixtures (tools/make_golden_plms.py);
 4. RNG contract R: the host generator is where the reference leaves it;
 5. the public surface: eta, ddim_steps=None, and DDIM's graph cache untouched by a PLMS job.

Bars.  (1) and (2): the same formula evaluated by torch in fp32 on the same inputs is measured against fp64 in the test itself; the
bar is 4x that figure ((2): times the number of steps).  The kernels are built without contraction and keep the reference's operation
order, so they sit at torch's error.  Measured on an MI355X (max|err| / max|ref|, worst of the calls; kernel / torch fp32):
    3072 elements  plain: x 1.47e-7 / 1.47e-7, pred_x0 1.24e-7 / 1.24e-7, e_t 0 / 0 (a copy)
                   cfg:   x 2.31e-7 / 3.19e-7, pred_x0 1.83e-7 / 2.28e-7, e_t 1.38e-7 / 1.38e-7
    1000 elements  plain: x 1.92e-7 / 1.57e-7, pred_x0 1.36e-7 / 1.08e-7;  cfg: x 2.60e-7 / 2.60e-7, pred_x0 1.80e-7 / 1.97e-7, e_t 9.85e-8 / 9.85e-8
(2), guidance 3.5, sampler vs fp64 loop (x) / torch fp32 per step / bar: 7 steps 4.82e-7 / 1.63e-7 / 4.58e-6; 1 step 7.91e-8 / 1.21e-7 /
4.85e-7; 2 steps 4.88e-7 / 1.91e-7 / 1.53e-6; 3 of 8 steps 7.11e-7 / 1.85e-7 / 2.22e-6.
(3): relative rms of the latent and rms error of the waveform against the fixture, measured on an MI355X
(profiles/r09_plms_errors.txt); every bar is <= 5x the measured value:
    mode     latent (7 steps, B = 2)   wave rms err        |  masked (4 steps, B = 1): latent      wave rms err
    bf16x6   2.99e-7 (bar 1.4e-6)      2.45e-7 (1.2e-6)    |  2.54e-7 (bar 1.2e-6)                 2.54e-7 (1.2e-6)
    f16x3    2.88e-7 (bar 1.4e-6)      2.45e-7 (1.2e-6)    |
    bf16x3   1.67e-6 (bar 8e-6)        1.47e-6 (7e-6)      |
Ceiling: the measured latent error also has to stay under 160/24 (the absolute sum of the 4th-order weights: the most the multistep
combine can amplify a per-pass eps error) times the 5-step DDIM latent bar of the mode (tolerances.latent_tol): 6.7e-5 / 6.7e-4.  It
is 200x / 400x below it.  The waveform also meets the project's 1e-3 rms and 1e-3 of the distance between two unrelated samples.
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


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


# ---- 1. kernels -----------------------------------------------------------------------------------------------------------------
def plms_formula(x, e, olds, c, dt):
    """plms.py:319-358 on tensors of dtype dt, the reference's operation order: olds = model outputs newest first (at most three
    are read; none: e is already e'), c = {sqrt(1-a_t), sqrt(a_t), sqrt(1-a_prev), sqrt(a_prev)} as 0-dim tensors."""
    x, e = x.to(dt), e.to(dt)
    olds = [o.to(dt) for o in olds]
    c = [v.to(dt) for v in c]
    if len(olds) == 0:
        ep = e
    elif len(olds) == 1:
        ep = (3 * e - olds[0]) / 2
    elif len(olds) == 2:
        ep = (23 * e - 16 * olds[0] + 5 * olds[1]) / 12
    else:
        ep = (55 * e - 59 * olds[0] + 37 * olds[1] - 9 * olds[2]) / 24
    p0 = (x - c[0] * ep) / c[1]
    return c[3] * p0 + c[2] * ep, p0


def combine(eps, cfg, dt):
    eps = eps.to(dt)
    return eps[0] + GS * (eps[1] - eps[0]) if cfg else eps


def coef_table(S, cfg, seed=0):
    """[S, 8] rows in ops.ddim_step's layout from a decreasing-noise alpha sequence."""
    a = torch.linspace(0.05, 0.95, S + 1) + 0.01 * torch.rand(S + 1, generator=torch.Generator().manual_seed(seed))
    tab = torch.zeros(S, 8)
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = (1 - a[:-1]).sqrt(), a[:-1].sqrt(), (1 - a[1:]).sqrt(), a[1:].sqrt()
    tab[:, 5], tab[:, 6] = GS, 1.0 if cfg else 0.0
    return tab


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("shape", [(3, 8, 8, 16), (1, 8, 5, 25)], ids=["3072", "1000"])
def test_step_kernels_match_fp64_call_by_call(shape, cfg):
    from audioldm2_amd import ops
    S = 7
    g = torch.Generator().manual_seed(5)
    dev = "cuda"
    tab_h = coef_table(S, cfg)
    tab = tab_h.to(dev)
    x = torch.randn(shape, generator=g).to(dev)
    eshape = ((2,) if cfg else ()) + shape
    hist = torch.full((3,) + shape, 7.0, device=dev)     # a value no model output has: an untouched slab stays recognisable
    pred = torch.empty_like(x)
    step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
    t_tab = torch.arange(S, dtype=torch.float32, device=dev)[:, None].contiguous()
    t_cur = t_tab[0].clone()
    worst = {"x": [0.0, 0.0], "pred_x0": [0.0, 0.0], "e_t": [0.0, 0.0]}   # [kernel, torch fp32] vs fp64

    def check(what, got, ref64, ref32):
        ek, et = relmax(got, ref64), relmax(ref32, ref64)
        worst[what][0], worst[what][1] = max(worst[what][0], ek), max(worst[what][1], et)
        assert ek <= 4 * et, (what, s, ek, et)

    for s in range(S):
        c = [tab_h[s, j] for j in range(4)]
        eps = torch.randn(eshape, generator=g).to(dev)
        x_in, hist_in = x.clone(), hist.clone()
        if s == 0:
            # provisional update from e_t alone, out of place: x and the ring stay as they are
            x_tmp, p_tmp = ops.plms_first_step(x, eps, None, tab[0])
            assert torch.equal(x, x_in) and torch.equal(hist, hist_in)
            r64 = plms_formula(x_in, combine(eps, cfg, torch.float64), [], c, torch.float64)
            r32 = plms_formula(x_in, combine(eps, cfg, torch.float32), [], c, torch.float32)
            check("x", x_tmp, r64[0], r32[0])
            check("pred_x0", p_tmp, r64[1], r32[1])
            eps_next = torch.randn(eshape, generator=g).to(dev)
            ops.plms_first_step(x, eps, eps_next, tab[0], x_out=x, pred_x0=pred, hist=hist)
            refs = {}
            for dt in (torch.float64, torch.float32):
                e = combine(eps, cfg, dt)
                refs[dt] = plms_formula(x_in, (e + combine(eps_next, cfg, dt)) / 2, [], c, dt) + (e,)
        else:
            assert int(step_idx.item()) == s
            ops.plms_step_indexed(x, eps, hist, tab, step_idx, pred)
            olds = [hist_in[(s - j) % 3] for j in range(1, min(s, 3) + 1)]   # newest first
            refs = {dt: plms_formula(x_in, combine(eps, cfg, dt), olds, c, dt) + (combine(eps, cfg, dt),)
                    for dt in (torch.float64, torch.float32)}
        slot = s % 3
        check("x", x, refs[torch.float64][0], refs[torch.float32][0])
        check("pred_x0", pred, refs[torch.float64][1], refs[torch.float32][1])
        check("e_t", hist[slot], refs[torch.float64][2], refs[torch.float32][2])
        for other in range(3):   # the two other slabs: bitwise untouched; the written one: changed
            assert torch.equal(hist[other], hist_in[other]) == (other != slot), (s, other)
        ops.step_advance(step_idx, t_tab, t_cur)
    print(f"plms kernels {shape} cfg={cfg}: " + "  ".join(f"{k} kernel {v[0]:.2e} / torch fp32 {v[1]:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        log_err(v[0], 4 * v[1], f"plms kernel {k} cfg={cfg} n={x.numel()}")


def test_step_indexed_at_counter_zero_writes_nothing():
    """Step 0 has no history: it belongs to plms_first_step, and a launch that finds the counter at 0 leaves every operand alone."""
    from audioldm2_amd import ops
    shape = (1, 8, 5, 25)
    x, eps, hist = torch.randn(shape).cuda(), torch.randn(shape).cuda(), torch.randn((3,) + shape).cuda()
    pred = torch.full(shape, 7.0).cuda()
    x0, h0 = x.clone(), hist.clone()
    ops.plms_step_indexed(x, eps, hist, coef_table(2, False).cuda(), torch.zeros(1, device="cuda", dtype=torch.int32), pred)
    assert torch.equal(x, x0) and torch.equal(hist, h0) and bool((pred == 7.0).all())


# ---- 2. sampler on the tiny UNet ----------------------------------------------------------------------------------------------
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


def x_T(seed=3):
    return torch.randn(TINY_SHAPE, generator=torch.Generator().manual_seed(seed))


def fp64_loop(m, cond, uncond, ts, xT):
    """PLMS over the ascending timestep subset `ts` (plms.py:200-258 and 261-360), eps from apply_model_cfg on the fp32 image of
    the fp64 state, every other operation in fp64.  Returns x, the last pred_x0 and the worst per-step error of the same step
    evaluated by torch in fp32 (the yardstick of the bars)."""
    ac = m.alphas_cumprod
    n = len(ts)
    time_range = np.flip(ts)
    x = xT.double().cuda()
    b = x.shape[0]
    olds, p0, e32 = [], None, 0.0

    def model(xx, t):
        eps = m.apply_model_cfg(xx.float(), torch.full((2 * b,), float(t), device="cuda"), cond, uncond)
        return eps

    for i, t in enumerate(time_range):
        index = n - i - 1
        a_t, a_prev = ac[ts[index]], (ac[ts[index - 1]] if index > 0 else ac[0])
        c = [(1 - a_t).sqrt(), a_t.sqrt(), (1 - a_prev).sqrt(), a_prev.sqrt()]      # fp32, as the reference rounds them
        c64 = [(1 - a_t.double()).sqrt(), a_t.double().sqrt(), (1 - a_prev.double()).sqrt(), a_prev.double().sqrt()]
        eps = model(x, t)
        e = combine(eps, True, torch.float64)
        if i == 0:
            x_tmp, _ = plms_formula(x, e, [], c64, torch.float64)
            e_next = combine(model(x_tmp, time_range[min(1, n - 1)]), True, torch.float64)
            args = ((e + e_next) / 2, [])
            args32 = ((combine(eps, True, torch.float32) + e_next.float()) / 2, [])
        else:
            args = (e, olds[:3])
            args32 = (combine(eps, True, torch.float32), olds[:3])
        x_new, p0 = plms_formula(x, *args, c64, torch.float64)
        x_32, _ = plms_formula(x, *args32, c, torch.float32)
        e32 = max(e32, relmax(x_32, x_new))
        olds.insert(0, e)
        x = x_new
    return x, p0, e32


def run_sampler(m, cond, uncond, S, xT, sampler=None, **kw):
    from audioldm2_amd.plms import PLMSSampler
    s = sampler or PLMSSampler(m)
    out, inter = s.sample(S, TINY_SHAPE[0], TINY_SHAPE[1:], cond, verbose=False, x_T=xT, unconditional_guidance_scale=GS,
                          unconditional_conditioning=uncond, **kw)
    return out, inter


@pytest.mark.parametrize("S,steps", [(6, 7), (1, 1), (2, 2)])
def test_sampler_matches_fp64_loop_and_graph_equals_eager(tiny, S, steps, monkeypatch):
    """S = 6 makes seven steps (make_ddim_timesteps: range(0, 1000, 1000 // 6)): Euler, 2nd, 3rd, four 4th-order steps; the step
    graph is captured at step 2 and replayed five times.  S = 1, 2: the ring is never full, nothing is captured."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    ts = make_ddim_timesteps("uniform", S, 1000)
    assert len(ts) == steps
    ref, ref_p0, e32 = fp64_loop(m, cond, uncond, ts, x_T())
    out, inter = run_sampler(m, cond, uncond, S, x_T(), log_every_t=1)
    ex, ep = relmax(out, ref), relmax(inter["pred_x0"][-1], ref_p0)
    bar = 4 * e32 * steps
    print(f"plms sampler S={S} ({steps} steps): x {ex:.2e} pred_x0 {ep:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert len(inter["x_inter"]) == steps + 1 and torch.equal(inter["x_inter"][-1], out)
    assert log_err(ex, bar, f"plms sampler x S={S}") <= bar and ep <= bar
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    eager = PLMSSampler(m)
    assert not eager.use_graph
    out_e, _ = run_sampler(m, cond, uncond, S, x_T(), sampler=eager)
    assert torch.equal(out, out_e), "graph replay and eager launches must agree bitwise"


def test_sampler_timesteps_subrange_three_steps_and_zero_steps(tiny):
    """plms.py:190-198: `timesteps` keeps the first int(min(timesteps / S, 1) * S) - 1 entries of the schedule."""
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    s = PLMSSampler(m)
    s.make_schedule(8, verbose=False)
    kw = dict(unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    out, inter = s.plms_sampling(cond, TINY_SHAPE, x_T=x_T(), timesteps=4, **kw)
    ref, _, e32 = fp64_loop(m, cond, uncond, s.ddim_timesteps[:3], x_T())
    ex = relmax(out, ref)
    print(f"plms sampler sub-range (3 of 8 steps): x {ex:.2e}  torch fp32 per step {e32:.2e}")
    assert ex <= 4 * e32 * 3
    out0, inter0 = s.plms_sampling(cond, TINY_SHAPE, x_T=x_T(), timesteps=1, **kw)
    assert torch.equal(out0.cpu(), x_T()) and len(inter0["x_inter"]) == 1


def test_second_job_on_one_sampler_equals_a_fresh_one(tiny):
    """No stale ring, counter or graph: job B after job A on one object == job B on a new object, bitwise; callbacks see every step."""
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    s = PLMSSampler(m)
    run_sampler(m, cond, uncond, 6, x_T(11), sampler=s)
    seen = []
    b_used, _ = run_sampler(m, cond, uncond, 4, x_T(12), sampler=s, callback=seen.append,
                            img_callback=lambda p, i: seen.append(tuple(p.shape)))
    b_fresh, _ = run_sampler(m, cond, uncond, 4, x_T(12))
    assert torch.equal(b_used, b_fresh)
    assert seen == [v for i in range(4) for v in (i, TINY_SHAPE)]


def test_p_sample_plms_steps_equal_the_sampling_loop(tiny):
    """The eager single-step form with a Python `old_eps` list (plms.py:229-248) walks the same trajectory as plms_sampling."""
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    s = PLMSSampler(m)
    out, _ = run_sampler(m, cond, uncond, 4, x_T(), sampler=s)
    time_range = np.flip(s.ddim_timesteps)
    img, old_eps = x_T().cuda(), []
    for i, step in enumerate(time_range):
        ts = torch.full((TINY_SHAPE[0],), int(step), device="cuda", dtype=torch.long)
        ts_next = torch.full((TINY_SHAPE[0],), int(time_range[min(i + 1, 3)]), device="cuda", dtype=torch.long)
        img, pred_x0, e_t = s.p_sample_plms(img, cond, ts, index=4 - i - 1, unconditional_guidance_scale=GS,
                                            unconditional_conditioning=uncond, old_eps=old_eps, t_next=ts_next)
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    assert torch.equal(img, out)


# ---- 3.-5. end to end against the real reference ------------------------------------------------------------------------------
AMPLIFICATION = 160.0 / 24.0   # |55| + |59| + |37| + |9| over 24


# (latent rel rms, wave rms err) bars, <= 5x the errors measured on an MI355X (module docstring, profiles/r09_plms_errors.txt)
E2E_BARS = {"bf16x6": (1.4e-6, 1.2e-6), "f16x3": (1.4e-6, 1.2e-6), "bf16x3": (8e-6, 7e-6)}
MASKED_BARS = (1.2e-6, 1.2e-6)


def ceiling(steps, mode=None):
    return AMPLIFICATION * latent_tol(steps, mode)


def assert_wave(ew, g):
    between = float(g["wave_between_rms"])
    assert between > 1e-2 and ew < 1e-3 and ew < 1e-3 * between, (ew, between)


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


def generate(ld, masked=False, **kw):
    """One job as the fixtures ran it (a fresh reference object's first call, seed 42), then the next draw of the host generator."""
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
        args = dict(use_plms=True, ddim_eta=0.0, unconditional_guidance_scale=1.0, n_gen=1, duration=10)
        args.update(kw)
        if masked:
            rec["wave"] = ld.generate_batch_masked(cases.e2e_masked_batch(1), ddim_steps=4, **args)
        else:
            rec["wave"] = ld.generate_batch(cases.e2e_batch(2), ddim_steps=6, **args)
        rec["rand_after"] = float(torch.rand(1))
    finally:
        ld.decode_first_stage_cl = orig
    return rec


def e2e_errors(rec, g):
    el = rms(rec["latent"].double().cpu().numpy() - g["latent"]) / rms(g["latent"])
    if "wave" in g.files:
        ew = rms(rec["wave"].astype(np.float64) - g["wave"])
    else:
        ew = max(rms(rec["wave"][..., :32768].astype(np.float64) - g["wave_head"]),
                 rms(rec["wave"][..., ::16].astype(np.float64) - g["wave_dec"]))
    return el, ew


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3", "bf16x3"])
def test_e2e_plms_matches_reference_generate_batch(ld, mode):
    """generate_batch(use_plms=True, ddim_eta=0.0, ddim_steps=6, guidance 1.0), B = 2, against the real reference's run; and the
    generator state it leaves (RNG contract R: x_T, two draws in step 0, one per later step)."""
    from audioldm2_amd import ops
    g = gold("e2e_plms_6step_b2")
    unet = ld.model.diffusion_model
    prev = ops.set_mma(mode)
    unet.drop_step_caches()
    try:
        rec = generate(ld)
    finally:
        ops.set_mma(prev)
        unet.drop_step_caches()
    assert rec["wave"].shape == (2, 1, int(g["wave_len"]))
    el, ew = e2e_errors(rec, g)
    bl, bw = E2E_BARS[mode]
    print(f"plms e2e 6 steps B=2 [{mode}]: latent rel rms {el:.2e} (bar {bl:.1e}, ceiling {ceiling(5, mode):.1e})  wave rms_err {ew:.3e} "
          f"(bar {bw:.1e}) / between-sample {float(g['wave_between_rms']):.3e}")
    assert el < ceiling(5, mode), "above what the 4th-order combine can make of the DDIM per-pass error"
    assert log_err(el, bl, "plms latent 6 steps B=2") < bl
    assert log_err(ew, bw, "plms wave 6 steps B=2") < bw
    assert_wave(ew, g)
    assert rec["rand_after"] == float(g["rand_after"])


def test_e2e_plms_masked_matches_reference_generate_batch_masked(ld):
    """The inpainting path: q_sample's draw first in every step, the blend between the replays."""
    g = gold("e2e_plms_masked_4step_b1")
    rec = generate(ld, masked=True)
    el, ew = e2e_errors(rec, g)
    print(f"plms masked 4 steps B=1: latent rel rms {el:.2e} (bar {MASKED_BARS[0]:.1e})  wave rms_err {ew:.3e} (bar {MASKED_BARS[1]:.1e}) / "
          f"between-sample {float(g['wave_between_rms']):.3e}")
    assert el < ceiling(4)
    assert log_err(el, MASKED_BARS[0], "plms masked latent") < MASKED_BARS[0]
    assert log_err(ew, MASKED_BARS[1], "plms masked wave") < MASKED_BARS[1]
    assert_wave(ew, g)
    assert rec["rand_after"] == float(g["rand_after"])


def test_rng_contract_holds_on_a_one_rank_shard(ld):
    """shard=(0, 1): the sharded code path draws the global batch and keeps its rows — same latent, same generator state."""
    g = gold("e2e_plms_6step_b2")
    rec = generate(ld, shard=(0, 1))
    el, _ = e2e_errors(rec, g)
    assert el < E2E_BARS["bf16x6"][0]
    assert rec["rand_after"] == float(g["rand_after"])


def test_surface_eta_and_steps(ld):
    ld.latent_t_size = 256
    with pytest.raises(ValueError, match="ddim_eta must equal 0 for PLMS"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=4, use_plms=True, duration=10)          # default ddim_eta = 1.0
    with pytest.raises(AssertionError):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=None, ddim_eta=0.0, use_plms=True, duration=10)
    with pytest.raises(AssertionError):
        ld.generate_batch_masked(cases.e2e_masked_batch(1), ddim_steps=None, ddim_eta=0.0, use_plms=True, duration=10)


def test_ddim_job_after_a_plms_job_equals_ddim_on_a_fresh_model(ld):
    """A PLMS run (here under guidance) neither reads nor writes the UNet's DDIM graph cache: a DDIM job after it equals, bitwise,
    the same job without it — through the graph an earlier DDIM job cached, and on a model with nothing cached."""
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
    generate(ld, unconditional_guidance_scale=3.5)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    hit_after = ddim()
    assert next(iter(unet._graph_cache.values())) is ent and np.array_equal(hit, hit_after)
    unet.drop_step_caches()
    generate(ld, unconditional_guidance_scale=3.5)
    assert len(unet._graph_cache) == 0
    fresh_after = ddim()
    unet.drop_step_caches()
    assert np.array_equal(fresh, fresh_after)
