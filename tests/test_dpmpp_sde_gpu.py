"""The DPM-Solver++(2M) SDE sampler on the GPU (audioldm2_amd/dpm_solver.py: DPMSolverSDESampler, ops.dpmpp_sde_step_indexed;
DESIGN.md 9l):

 1. the step kernel against an fp64 restatement, call by call, the device counter running 0..6 (first order, five second-order
    steps, first-order final) over a 7-row noise table, with and without the combine flag, eta 0.3 and 1; n = 3072 and 1000 take the
    16-byte form, n = 1003 the scalar one; inputs and tables unchanged, two calls bitwise equal, guard bands intact;
 2. rows with c4 == 0 and a NaN noise table are bitwise ops.dpmpp_step_indexed; w == 0 ignores a NaN history slab;
 3. the noise row clamp; 4. the wrapper's refusals;
 5. DPMSolverSDESampler.sample on the tiny UNet under guidance 3.5 against the fp64 loop of tests/dpmpp_sde.py on the same seeded
    host draws (7 steps, 1 step, t_start = 3 of 8, guidance_rescale = 0.7, a mask / x0; eta 0.5 and 1), graph replay == eager
    bitwise, two jobs on one object, seeds, zero steps, temperature, callbacks;
 6. the tie to the pinned sampler: at S = 2 both steps are first order and, at eta = 1, the output is DDIMSampler's at eta = 1 from
    the same x_T and seed, with and without a mask;
 7. windows: a linear plan, a ring plan with a source and graded levels, a phased ring, a row plan, against the composition loops
    of tests/windowed.py / looped.py / phased.py / timeline.py around the same fp64 step;
 8. end to end on the real model: generate_batch / generate_batch_masked / text_to_audio / text_to_audio_long(loop=True), a 7-step
    latent against the fp64 loop, a one-rank shard.

Bars.  (1), (5), (6): the same formula evaluated by torch in fp32 on the same inputs is measured against fp64 in the test itself;
the bar is 4x that figure ((5), (6): times the number of steps) — tests/test_dpmpp_gpu.py's rule.  The kernel is built without
contraction and keeps the formula's operation order.  (7): 1e-5 relative rms, the bar of those suites for the other samplers
(audio2audio.tstart_bar).  (8): tolerances.latent_tol(5, mode).

Measured on an MI355X (max|err| / max|ref|, worst of the seven calls; kernel / torch fp32; the full log: profiles/r24_dpmpp_sde_errors.txt):
    3072 elements  eta .3 plain: x 1.12e-7 / 1.16e-7, x0_buf 8.37e-8 / 1.23e-7;  cfg: x 1.57e-7 / 1.57e-7, x0_buf 9.98e-8 / 1.32e-7
                   eta 1  plain: x 1.18e-7 / 1.56e-7, x0_buf 8.37e-8 / 1.09e-7;  cfg: x 1.44e-7 / 1.58e-7, x0_buf 9.98e-8 / 1.32e-7
    1000 elements  eta .3 plain: x 1.01e-7 / 1.01e-7, x0_buf 7.42e-8 / 8.00e-8;  cfg: x 1.37e-7 / 1.37e-7, x0_buf 1.20e-7 / 1.29e-7
                   eta 1  plain: x 9.11e-8 / 1.09e-7, x0_buf 5.50e-8 / 1.04e-7;  cfg: x 1.16e-7 / 1.23e-7, x0_buf 1.20e-7 / 1.29e-7
    1003 elements  eta .3 plain: x 1.02e-7 / 9.88e-8, x0_buf 8.65e-8 / 9.11e-8;  cfg: x 1.18e-7 / 1.30e-7, x0_buf 9.96e-8 / 1.58e-7
                   eta 1  plain: x 1.28e-7 / 1.28e-7, x0_buf 9.38e-8 / 1.11e-7;  cfg: x 1.39e-7 / 1.58e-7, x0_buf 1.13e-7 / 1.58e-7
(5), guidance 3.5, sampler vs fp64 loop (x) / torch fp32 per step / bar: 7 steps eta 1 5.85e-7 / 2.50e-7 / 7.00e-6; 7 steps eta .5
5.43e-7 / 2.26e-7 / 6.32e-6; 1 step 5.85e-8 / 9.70e-8 / 3.88e-7; 3 of 8 steps 1.51e-6 / 3.45e-7 / 4.14e-6; guidance_rescale .7
8.52e-7 / 2.01e-7 / 5.64e-6; mask 1.28e-6 / 2.34e-7 / 6.55e-6; mask, 4 steps, eta .5 9.96e-7 / 1.88e-7 / 3.01e-6.  Another seed moves
the latent by 4.7e-1 (100 x bar: 7.7e-4).  (6): SDE at eta 1 vs DDIM at eta 1, S = 2: 1.60e-7, bar 1.00e-6; with a mask 1.56e-7, bar
9.22e-7.  (7), 6 steps, relative rms vs the composition loop (bar 1e-5): linear 4.35e-7, ring + source + graded levels 9.42e-7, ring +
source 9.95e-7, phased ring 4.38e-7, row plan 4.32e-7.  (8): 7 steps vs the fp64 loop, latent relative rms: bf16x6 3.96e-7, f16x3
3.89e-7 (bar 1e-5), bf16x3 8.99e-7 (bar 1e-4).
"""
import json
import os

import numpy as np
import pytest
import torch

import audio2audio as A
import dpmpp_sde as D
from oracle import cases, weights
from tolerances import latent_tol, log_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GS = D.GS


# ---- 1. kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.3, 1.0])
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("shape", [(3, 8, 8, 16), (1, 8, 5, 25), (1, 1, 17, 59)], ids=["3072", "1000", "1003"])
def test_step_kernel_matches_fp64_call_by_call(shape, cfg, eta):
    from audioldm2_amd import ops
    S = 7
    g = torch.Generator().manual_seed(5)
    dev = "cuda"
    tab_h, rows = D.kernel_table(S, cfg, eta)
    assert [float(w) == 0.0 for w in tab_h[:, 4]] == [True] + [False] * 5 + [True] and bool((tab_h[:, 8] > 0).all())
    tab = tab_h.to(dev)
    n = int(np.prod(shape))
    x, xbuf = A.guarded(shape)
    slab, sbuf = A.guarded(shape)
    x.copy_(torch.randn(shape, generator=g))
    slab.fill_(7.0)                                  # step 0 must not read it
    if n % 4:                                        # 1003: x and every noise row but the first sit off 16 bytes
        assert x.data_ptr() % 16 == 0 and (4 * n) % 16 != 0
    noise_h = torch.randn((S,) + shape, generator=g)
    noise = noise_h.to(dev)
    eshape = ((2,) if cfg else ()) + shape
    step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
    t_tab = torch.arange(S, dtype=torch.float32, device=dev)[:, None].contiguous()
    t_cur = t_tab[0].clone()
    worst = {"x": [0.0, 0.0], "x0_buf": [0.0, 0.0]}   # [kernel, torch fp32] vs fp64

    def check(what, got, ref64, ref32):
        ek, et = D.relmax(got, ref64), D.relmax(ref32, ref64)
        worst[what][0], worst[what][1] = max(worst[what][0], ek), max(worst[what][1], et)
        assert ek <= 4 * et, (what, s, ek, et)

    for s in range(S):
        c = [rows[s, j] for j in range(6)]
        eps = torch.randn(eshape, generator=g).to(dev)
        eps_in, x_in, old = eps.clone(), x.clone(), slab.clone()
        assert int(step_idx.item()) == s
        assert ops.dpmpp_sde_step_indexed(x, eps, slab, noise, tab, step_idx) is x
        # the same call again on the same inputs: bitwise the first
        x2, slab2 = x_in.clone(), old.clone()
        ops.dpmpp_sde_step_indexed(x2, eps, slab2, noise, tab, step_idx)
        assert torch.equal(x2, x) and torch.equal(slab2, slab)
        refs = {dt: D.sde_formula(x_in, D.combine(eps, cfg, dt), old, noise[s], c, dt) for dt in (torch.float64, torch.float32)}
        check("x", x, refs[torch.float64][0], refs[torch.float32][0])
        check("x0_buf", slab, refs[torch.float64][1], refs[torch.float32][1])
        assert torch.equal(eps, eps_in) and torch.equal(tab, tab_h.to(dev)) and torch.equal(noise.cpu(), noise_h)
        assert A.guards_intact(xbuf) and A.guards_intact(sbuf)
        ops.step_advance(step_idx, t_tab, t_cur)
    print(f"dpmpp sde kernel {shape} cfg={cfg} eta={eta}: " +
          "  ".join(f"{k} kernel {v[0]:.2e} / torch fp32 {v[1]:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        log_err(v[0], 4 * v[1], f"dpmpp sde kernel {k} cfg={cfg} eta={eta} n={n}")


# ---- 2. special rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8, 5, 25), (1, 1, 17, 59)], ids=["1000", "1003"])
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_rows_without_noise_are_bitwise_the_ode_kernel_and_first_order_ignores_the_slab(shape, cfg):
    from audioldm2_amd import ops
    g = torch.Generator().manual_seed(9)
    tab, _ = D.kernel_table(3, cfg, 0.0)
    assert float(tab[:, 8].abs().max()) == 0.0           # eta = 0: c4 == 0 in every row
    tab = tab.cuda()
    x = torch.randn(shape, generator=g).cuda()
    eps = torch.randn(((2,) if cfg else ()) + shape, generator=g).cuda()
    old = torch.randn(shape, generator=g).cuda()
    nan_noise = torch.full((3,) + shape, float("nan"), device="cuda")
    for s in (0, 1, 2):
        idx = torch.full((1,), s, device="cuda", dtype=torch.int32)
        xa, sa, xb, sb = x.clone(), old.clone(), x.clone(), old.clone()
        ops.dpmpp_sde_step_indexed(xa, eps, sa, nan_noise, tab, idx)
        ops.dpmpp_step_indexed(xb, eps, sb, tab[:, :8].contiguous(), idx)
        assert bool(torch.isfinite(xa).all()) and torch.equal(xa, xb) and torch.equal(sa, sb) and not torch.equal(xa, x)
    # w == 0 with a NaN history slab is bitwise the zero-filled one — under a row that does add noise
    tab1, _ = D.kernel_table(3, cfg, 1.0)
    tab1 = tab1.cuda()
    noise = torch.randn((3,) + shape, generator=g).cuda()
    out = {}
    for name, fill in (("nan", float("nan")), ("zero", 0.0)):
        xx, slab = x.clone(), torch.full(shape, fill, device="cuda")
        ops.dpmpp_sde_step_indexed(xx, eps, slab, noise, tab1, torch.zeros(1, device="cuda", dtype=torch.int32))
        out[name] = (xx, slab)
    assert bool(torch.isfinite(out["nan"][0]).all()) and bool(torch.isfinite(out["nan"][1]).all())
    assert torch.equal(out["nan"][0], out["zero"][0]) and torch.equal(out["nan"][1], out["zero"][1])
    # ... a second-order row does read the slab, and a row with c4 != 0 its noise
    xx, slab = x.clone(), torch.full(shape, float("nan"), device="cuda")
    ops.dpmpp_sde_step_indexed(xx, eps, slab, noise, tab1, torch.ones(1, device="cuda", dtype=torch.int32))
    assert bool(torch.isnan(xx).all()) and bool(torch.isfinite(slab).all())
    xx, slab = x.clone(), old.clone()
    ops.dpmpp_sde_step_indexed(xx, eps, slab, nan_noise, tab1, torch.zeros(1, device="cuda", dtype=torch.int32))
    assert bool(torch.isnan(xx).all()) and bool(torch.isfinite(slab).all())


# ---- 3. the clamp -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8, 5, 25), (1, 1, 17, 59)], ids=["1000", "1003"])
def test_noise_row_is_clamped_into_the_table(shape):
    """noise_rows = 3 under a coefficient table of 7 rows: counter 5 reads noise row 2 (and coefficient row 5); a negative counter
    is not exercised, its coefficient row would lie in front of the table."""
    from audioldm2_amd import ops
    g = torch.Generator().manual_seed(4)
    tab, _ = D.kernel_table(7, True, 1.0)
    tab = tab.cuda()
    x, eps, old = torch.randn(shape, generator=g).cuda(), torch.randn((2,) + shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    noise = torch.randn((3,) + shape, generator=g).cuda()
    idx = torch.full((1,), 5, device="cuda", dtype=torch.int32)
    xa, sa, xb, sb = x.clone(), old.clone(), x.clone(), old.clone()
    ops.dpmpp_sde_step_indexed(xa, eps, sa, noise, tab, idx)
    ops.dpmpp_sde_step_indexed(xb, eps, sb, noise[2].clone(), tab, idx)          # one row [*x.shape]: noise_rows = 1
    assert torch.equal(xa, xb) and torch.equal(sa, sb)
    xc = x.clone()
    ops.dpmpp_sde_step_indexed(xc, eps, old.clone(), noise[1].clone(), tab, idx)
    assert not torch.equal(xa, xc)


# ---- 4. the wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_checks_its_tensors():
    from audioldm2_amd import ops
    shape = (1, 8, 5, 25)
    x, eps, slab = torch.randn(shape).cuda(), torch.randn(shape).cuda(), torch.zeros(shape).cuda()
    noise = torch.randn((2,) + shape).cuda()
    tab, idx = D.kernel_table(2, False, 1.0)[0].cuda(), torch.zeros(1, device="cuda", dtype=torch.int32)
    f = ops.dpmpp_sde_step_indexed
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        f(x.cpu(), eps, slab, noise, tab, idx)                                   # device
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        f(x, eps, slab, noise.double(), tab, idx)                                # dtype
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        f(x, eps, slab, noise.transpose(-1, -2), tab, idx)                       # non-contiguous
    with pytest.raises(AssertionError):
        f(x, eps, slab[:, :4].contiguous(), noise, tab, idx)                     # shape
    with pytest.raises(RuntimeError, match="dpmpp_sde_indexed.noise: expected"):
        f(x, eps, slab, noise[..., :5].contiguous(), tab, idx)
    with pytest.raises(AssertionError):
        f(x, eps, slab, noise, tab, idx.long())
    with pytest.raises(RuntimeError, match="coef_ld=8"):
        f(x, eps, slab, noise, tab[:, :8].contiguous(), idx)
    with pytest.raises(RuntimeError, match="x overlaps noise"):
        f(noise[1], eps, slab, noise, tab, idx)                                  # overlap
    with pytest.raises(RuntimeError, match="x0_buf overlaps noise"):
        f(x, eps, noise[0], noise, tab, idx)


# ---- 5. / 6. sampler on the tiny UNet ---------------------------------------------------------------------------------------------
SEED = 17


@pytest.fixture(scope="module")
def tiny():
    m = D.TinyModel()
    cond, uncond = D.tiny_conditioning()
    return m, cond, uncond


def run_sampler(m, cond, uncond, S, xT, eta=1.0, sampler=None, seed=SEED, shape=D.TINY_SHAPE, **kw):
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    s = sampler or DPMSolverSDESampler(m)
    torch.manual_seed(seed)
    return s.sample(S, shape[0], shape[1:], cond, verbose=False, x_T=xT, eta=eta, unconditional_guidance_scale=GS,
                    unconditional_conditioning=uncond, **kw)


def tiny_source():
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(D.TINY_SHAPE, generator=g)
    mask = torch.zeros(1, 1, D.TINY_SHAPE[2], 1)
    mask[:, :, :5] = 1.0
    mask[:, :, 11:13] = 1.0
    return x0, mask


RUNS = {"7 steps eta 1": dict(S=6, steps=7, eta=1.0), "7 steps eta .5": dict(S=6, steps=7, eta=0.5), "1 step": dict(S=1, steps=1, eta=1.0),
        "3 of 8": dict(S=8, steps=3, eta=1.0, t_start=3), "rescale .7": dict(S=6, steps=7, eta=0.5, guidance_rescale=0.7),
        "mask": dict(S=6, steps=7, eta=1.0, masked=True), "mask eta .5": dict(S=4, steps=4, eta=0.5, masked=True)}


@pytest.mark.parametrize("name", list(RUNS))
def test_sampler_matches_fp64_loop_and_graph_equals_eager(tiny, name, monkeypatch):
    """S = 6 makes seven steps (make_ddim_timesteps: range(0, 1000, 1000 // 6)): first order, five second-order steps, first-order
    final; step 0 runs eagerly, the graph is captured at step 1 and replayed five times."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    m, cond, uncond = tiny
    r = dict(RUNS[name])
    S, steps, eta, masked = r.pop("S"), r.pop("steps"), r.pop("eta"), r.pop("masked", False)
    ts = make_ddim_timesteps("uniform", S, 1000)[:steps]
    assert len(ts) == steps
    x0, mask = tiny_source() if masked else (None, None)
    _, q, z = D.host_draws(SEED, D.TINY_SHAPE, steps, masked)
    ref, ref_p0, e32 = D.fp64_loop(D.tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, ts, D.x_T(), eta, z,
                                   phi=r.get("guidance_rescale", 0.0), mask=mask, x0=x0, q=q)
    kw = dict(r, **(dict(mask=mask, x0=x0) if masked else {}))
    out, inter = run_sampler(m, cond, uncond, S, D.x_T(), eta=eta, log_every_t=1, **kw)
    rand_after = float(torch.rand(1))
    ex, ep = D.relmax(out, ref), D.relmax(inter["pred_x0"][-1], ref_p0)
    bar = 4 * e32 * steps
    print(f"dpmpp sde sampler [{name}] ({steps} steps): x {ex:.2e} pred_x0 {ep:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert len(inter["x_inter"]) == steps + 1 and torch.equal(inter["x_inter"][-1], out)
    assert log_err(ex, bar, f"dpmpp sde sampler x [{name}]") <= bar and ep <= bar
    # the host generator is where the contract's draws leave it
    torch.manual_seed(SEED)
    for _ in range(steps * (2 if masked else 1)):
        torch.randn(D.TINY_SHAPE)
    assert float(torch.rand(1)) == rand_after
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    eager = DPMSolverSDESampler(m)
    assert not eager.use_graph
    out_e, _ = run_sampler(m, cond, uncond, S, D.x_T(), eta=eta, sampler=eager, **kw)
    assert torch.equal(out, out_e), "graph replay and eager launches must agree bitwise"


def test_seeds_jobs_on_one_object_callbacks_temperature_and_zero_steps(tiny):
    from audioldm2_amd.ddim import make_ddim_timesteps
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    m, cond, uncond = tiny
    s = DPMSolverSDESampler(m)
    a, _ = run_sampler(m, cond, uncond, 6, D.x_T(11), sampler=s)
    # no stale slab, counter, table or graph: job B after job A on one object == job B on a new object, bitwise
    seen = []
    b_used, _ = run_sampler(m, cond, uncond, 4, D.x_T(12), sampler=s, callback=seen.append,
                            img_callback=lambda p, i: seen.append(tuple(p.shape)))
    b_fresh, _ = run_sampler(m, cond, uncond, 4, D.x_T(12))
    assert torch.equal(b_used, b_fresh)            # ... and the unthreaded one-step feed a callback forces draws the same stream
    assert seen == [v for i in range(4) for v in (i, D.TINY_SHAPE)]
    cb = lambda i: None
    cb.uses_rng = False
    b_decl, _ = run_sampler(m, cond, uncond, 4, D.x_T(12), callback=cb)
    assert torch.equal(b_decl, b_fresh)
    # the same seed twice is bitwise equal; another seed differs by far more than the bar
    a2, _ = run_sampler(m, cond, uncond, 6, D.x_T(11))
    other, _ = run_sampler(m, cond, uncond, 6, D.x_T(11), seed=SEED + 1)
    ts = make_ddim_timesteps("uniform", 6, 1000)
    _, _, z = D.host_draws(SEED, D.TINY_SHAPE, 7, False)
    _, _, e32 = D.fp64_loop(D.tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, ts, D.x_T(11), 1.0, z)
    d = D.relmax(other, a)
    print(f"dpmpp sde: another seed moves the latent by {d:.2e}; 100 x bar = {100 * 4 * e32 * 7:.2e}")
    assert torch.equal(a, a2) and d > 100 * 4 * e32 * 7
    # temperature scales the step noise, as DDIM's feed scales it
    _, _, zt = D.host_draws(SEED, D.TINY_SHAPE, 4, False)
    ts4 = make_ddim_timesteps("uniform", 4, 1000)
    ref, _, e32 = D.fp64_loop(D.tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, ts4, D.x_T(12), 1.0, zt, temperature=0.5)
    cold, _ = run_sampler(m, cond, uncond, 4, D.x_T(12), temperature=0.5)
    assert D.relmax(cold, ref) <= 4 * e32 * 4 and not torch.equal(cold, b_fresh)
    # zero steps: x_T comes back, nothing is drawn
    s.make_schedule(8, ddim_eta=1.0, verbose=False)
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    out0, inter0 = s.dpm_sampling(cond, D.TINY_SHAPE, x_T=D.x_T(), timesteps=1, unconditional_guidance_scale=GS,
                                  unconditional_conditioning=uncond)
    assert torch.equal(out0.cpu(), D.x_T()) and len(inter0["x_inter"]) == 1 and torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
def test_first_order_at_eta_one_is_ddim_at_eta_one(tiny, masked):
    """S = 2: step 0 is first order and so is the final step of a run under 15 steps; at eta = 1 a first-order step is algebraically
    DDIM's eta = 1 step, and both samplers consume the host generator in the same order: from the same x_T and seed they agree
    within the bar of the fp64 comparison."""
    from audioldm2_amd.ddim import DDIMSampler, make_ddim_timesteps
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    m, cond, uncond = tiny
    x0, mask = tiny_source() if masked else (None, None)
    kw = dict(mask=mask, x0=x0) if masked else {}
    s = DPMSolverSDESampler(m)
    out, _ = run_sampler(m, cond, uncond, 2, D.x_T(), sampler=s, **kw)
    assert s.dpm_coef.shape == (2, 6) and float(s.dpm_coef[:, 4].abs().max()) == 0.0
    torch.manual_seed(SEED)
    ddim, _ = DDIMSampler(m).sample(2, D.TINY_SHAPE[0], D.TINY_SHAPE[1:], cond, verbose=False, x_T=D.x_T(), eta=1.0,
                                    unconditional_guidance_scale=GS, unconditional_conditioning=uncond, **kw)
    _, q, z = D.host_draws(SEED, D.TINY_SHAPE, 2, masked)
    _, _, e32 = D.fp64_loop(D.tiny_model_cfg(m, cond, uncond), m.alphas_cumprod, make_ddim_timesteps("uniform", 2, 1000), D.x_T(), 1.0, z,
                            mask=mask, x0=x0, q=q)
    ed, bar = D.relmax(out, ddim), 4 * e32 * 2
    print(f"dpmpp sde S=2 eta=1 vs DDIM eta 1 (masked={masked}): {ed:.2e}  torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert log_err(ed, bar, f"dpmpp sde first order vs ddim eta 1 masked={masked}") <= bar


# ---- 7. windows -------------------------------------------------------------------------------------------------------------------
def _window_cases(tiny):
    """name -> (the plan the sampler gets, the model the fp64 loop steps, the conditioning of either side, source or None, levels)."""
    import graded as G
    import long_source as Ls
    import looped as Lp
    import phased as Ph
    import timeline as Tl
    import windowed as Wd
    from audioldm2_amd.windows import PerPrompt, keep_mask, phase_table, window_plan, with_phase, with_source
    from oracle import cases as oc
    m, cond, uncond = tiny
    shape = Ls.LONG_SHAPE
    linear, ring = window_plan(*Ls.LONG_KEY), Lp.ring_plan(Ls.LONG_KEY)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    levels = G.long_levels(linear, ring=True)
    tab = phase_table(ring, Ls.STEPS, "golden")
    assert tab.tolist() == Ph.GOLDEN_6
    _, _, ctxs, masks, _ = oc.unet_inputs(oc.UNET_TINY, shape[0], 16, 8, 12, seed=3)
    prompts = [cond, ([c.cuda() for c in ctxs], [k.cuda() for k in masks])]
    rp = Tl.plans_of(Ls.LONG_KEY, [20], 4)[1]
    assert rp.R > rp.W
    return {"linear": (linear, Wd.WindowedModel(m, linear), cond, cond, None, None),
            "ring+source+graded": (with_source(ring, x0, levels, graded=True), Lp.RingModel(m, ring), cond, cond, x0, levels),
            "ring+source": (with_source(ring, x0, keep_mask(shape[2], Ls.KEEP)), Lp.RingModel(m, ring), cond, cond, x0,
                            keep_mask(shape[2], Ls.KEEP)),
            "phased ring": (with_phase(ring, tab), Ph.PhasedRingModel(m, ring, Ph.GOLDEN_6), cond, cond, None, None),
            "rows": (rp, Tl.TimelineModel(m, rp), PerPrompt(prompts), prompts, None, None)}, shape, Ls.STEPS


@pytest.mark.parametrize("name", ["linear", "ring+source+graded", "ring+source", "phased ring", "rows"])
def test_windowed_sampler_equals_the_composition_loop(tiny, name):
    from audioldm2_amd.sampling import make_ddim_timesteps
    m, _, uncond = tiny
    table, shape, steps = _window_cases(tiny)
    plan, model, cond, loop_cond, x0, levels = table[name]
    xT = D.x_T(3, shape)
    out, _ = run_sampler(m, cond, uncond, steps, xT, shape=shape, windows=plan, t_start=steps)
    rand_after = float(torch.rand(1))
    _, q, z = D.host_draws(SEED, shape, steps, x0 is not None)
    b = shape[0]
    model_cfg = lambda xx, t: model.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), loop_cond, uncond)
    ts = make_ddim_timesteps("uniform", steps, 1000, verbose=False)[:steps]
    graded = name.endswith("graded")
    lv4 = None if levels is None else levels.view(1, 1, -1, 1)
    ref, _, _ = D.fp64_loop(model_cfg, m.alphas_cumprod, ts, xT, 1.0, z, x0=x0, q=q, mask=None if graded else lv4,
                            level=lv4 if graded else None)
    e, bar = D.rel_rms(out, ref), A.tstart_bar(steps)
    print(f"dpmpp sde windows [{name}] {steps} steps vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert tuple(out.shape) == shape and bool(torch.isfinite(out).all())
    assert log_err(e, bar, f"dpmpp sde windowed [{name}]") <= bar
    torch.manual_seed(SEED)
    for _ in range(steps * (2 if x0 is not None else 1)):
        torch.randn(shape)
    assert float(torch.rand(1)) == rand_after
    # a second job of the same geometry under the same seed: bitwise the first
    out2, _ = run_sampler(m, cond, uncond, steps, xT, shape=shape, windows=_window_cases(tiny)[0][name][0], t_start=steps)
    assert torch.equal(out2, out)


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
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


def generate(ld, masked=False, steps=4, **kw):
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
        args = dict(unconditional_guidance_scale=GS, n_gen=1, duration=10, ddim_steps=steps, sampler="dpmpp_2m_sde")
        args.update(kw)
        if masked:
            rec["wave"] = ld.generate_batch_masked(cases.e2e_masked_batch(1), **args)
        else:
            rec["wave"] = ld.generate_batch(cases.e2e_batch(2), **args)
        rec["rand_after"] = float(torch.rand(1))
    finally:
        ld.decode_first_stage_cl = orig
    return rec


E2E_SHAPE = (2, 8, 256, 16)


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3", "bf16x3"])
def test_e2e_seven_steps_match_the_fp64_loop(ld, mode):
    """A 7-step job (ddim_steps=6) through sample_log in each matrix-core mode against the fp64 loop over the model's own
    apply_model_cfg in that mode, on the same seeded host draws."""
    from audioldm2_amd import ops
    from audioldm2_amd.ddim import make_ddim_timesteps
    unet = ld.model.diffusion_model
    ld.latent_t_size = 256
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(2))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(2) for k, m in ld.cond_stage_model_metadata.items()}
    xT = D.x_T(21, E2E_SHAPE)
    prev = ops.set_mma(mode)
    unet.drop_step_caches()
    try:
        torch.manual_seed(SEED)
        out, _ = ld.sample_log(cond=cond, batch_size=2, ddim=True, ddim_steps=6, eta=1.0, unconditional_guidance_scale=GS,
                               unconditional_conditioning=uncond, sampler="dpmpp_2m_sde", x_T=xT)
        prepared = ld.prepare_cfg(cond, uncond)
        ts = make_ddim_timesteps("uniform", 6, 1000)
        _, _, z = D.host_draws(SEED, E2E_SHAPE, len(ts), False)
        ref, _, e32 = D.fp64_loop(lambda xx, t: ld.apply_model_cfg(xx, torch.full((4,), t, device="cuda"), prepared=prepared),
                                  ld.alphas_cumprod.detach().float().cpu(), ts, xT, 1.0, z)
    finally:
        ops.set_mma(prev)
        unet.drop_step_caches()
    assert len(ts) == 7
    el = D.rel_rms(out, ref)
    print(f"dpmpp sde e2e 7 steps B=2 [{mode}] vs fp64 loop: latent rel rms {el:.2e} (bar {latent_tol(5, mode):.1e})  "
          f"torch fp32 per step {e32:.2e}")
    assert log_err(el, latent_tol(5, mode), "dpmpp sde latent 7 steps vs fp64 loop") < latent_tol(5, mode)


def test_e2e_jobs_take_the_sampler_by_name(ld):
    """generate_batch (default ddim_eta = 1.0: the full SDE) and generate_batch_masked: finite waves of the right length, the same
    seed twice bitwise equal, eta = 0.5 another clip, a one-rank shard bitwise the unsharded job, and nothing in the DDIM graph cache."""
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    a, b = generate(ld), generate(ld)
    assert a["wave"].shape == (2, 1, 163872) and a["wave"].dtype == np.float32 and np.isfinite(a["wave"]).all()
    assert torch.equal(a["latent"], b["latent"]) and np.array_equal(a["wave"], b["wave"]) and a["rand_after"] == b["rand_after"]
    half = generate(ld, ddim_eta=0.5)
    assert not torch.equal(half["latent"], a["latent"]) and half["rand_after"] == a["rand_after"]
    sh = generate(ld, shard=(0, 1))
    assert torch.equal(a["latent"], sh["latent"]) and np.array_equal(a["wave"], sh["wave"]) and a["rand_after"] == sh["rand_after"]
    mk = generate(ld, masked=True, unconditional_guidance_scale=2.5)
    assert mk["wave"].shape == (1, 1, 163872) and np.isfinite(mk["wave"]).all() and bool(torch.isfinite(mk["latent"]).all())
    assert len(unet._graph_cache) == 0
    with pytest.raises(ValueError, match="needs 0 < ddim_eta <= 1"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=4, ddim_eta=0.0, sampler="dpmpp_2m_sde", duration=10)
    with pytest.raises(ValueError, match="needs ddim_steps"):
        ld.generate_batch(cases.e2e_batch(1), ddim_steps=None, sampler="dpmpp_2m_sde", duration=10)


def test_entry_points_take_the_sampler_by_name(ld):
    """text_to_audio and text_to_audio_long(loop=True) have no eta parameter: eta 1 travels with the name.  Deterministic under the
    seed; neither the DDIM clip nor the deterministic solver's."""
    from audioldm2_amd.pipeline import text_to_audio, text_to_audio_long
    kw = dict(seed=7, ddim_steps=4, duration=10, batchsize=1, n_candidate_gen_per_text=1)

    def job(**more):
        ld.conditional_dry_run_finished = False   # every call as an object's first (pipeline._cfg_dropout_draw)
        return text_to_audio(ld, "a dog barking", **kw, **more)
    a, b, c, d = job(sampler="dpmpp_2m_sde"), job(sampler="dpmpp_2m_sde"), job(), job(sampler="dpmpp_2m")
    assert a.shape == (1, 1, 163872) and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)

    def long_job():
        ld.conditional_dry_run_finished = False
        return text_to_audio_long(ld, "rain on a tin roof", duration=15, overlap=5.0, seed=7, ddim_steps=4, guidance_scale=GS,
                                  loop=True, sampler="dpmpp_2m_sde")
    w = long_job()
    h = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert w.shape == (1, 1, 384 * 4 * h) and w.dtype == np.float32 and np.isfinite(w).all()
    assert np.array_equal(w, long_job()) and ld.latent_t_size == 256
    ld.model.diffusion_model.drop_step_caches()
