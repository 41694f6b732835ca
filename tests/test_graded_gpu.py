"""GPU tests of graded keep levels (differential diffusion): aldm_keep_threshold_indexed against torch's
`(level > thr[r]).float()` (bitwise: the kernel is a comparison), its device-side row selection and clamping, both access paths,
bounds and refusals; the three samplers with `graded=True` on the tiny UNet — the masked path, and a source on a linear, a ring and a
row plan, with guidance rescale and with resample= — against the composition loops of tests/graded.py (per step the torch blend under
the mask (level > keep_thresholds(S)[i]), the draws by hand in contract order); binary levels against the run without the keyword
(bitwise); the step graph captured once, with the new launch inside it; off by default; extend_audio end to end.

The bar of a sampler against its composition loop is 1e-5 relative rms, the project's bar for sampler compositions,
in the default fp32-grade matrix modes."""
import numpy as np
import pytest
import torch

import audio2audio as A
import graded as G
import long_source as Ls
import looped as Lp
import resample as Rs
import timeline as Tl
import windowed as Wd
from tolerances import latent_tol, log_err

pytestmark = pytest.mark.gpu

LOOP_BAR = 1e-5
NAN = float("nan")
ZERO_BITS, ONE_BITS = 0, 0x3F800000


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
def counter(idx):
    return None if idx is None else torch.full((1,), idx, device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("n", G.KERNEL_N)
def test_threshold_is_bitwise_the_torch_comparison_for_every_counter(n):
    from audioldm2_amd import ops
    level, thr = G.kernel_inputs(n, seed=n)
    ld_, thrd = level.cuda(), thr.cuda()
    if n > 64:
        assert bool(torch.isnan(level).any()) and all(bool((level == t).any()) for t in thr.tolist())   # the planted values are there
    results = {}
    for idx, row in G.COUNTERS:
        mask, buf = A.guarded((n,))
        step_idx = counter(idx)
        got = ops.keep_threshold_indexed(ld_, thrd, mask, step_idx)
        assert got is mask and A.guards_intact(buf)
        if step_idx is not None:
            assert int(step_idx) == idx                                  # the counter is read, not written
        want = (ld_ > thrd[row]).float()
        assert torch.equal(bits(mask), bits(want)), f"n={n} counter {idx}: not (level > thr[{row}]).float()"
        b = bits(mask)
        assert bool(((b == ZERO_BITS) | (b == ONE_BITS)).all())          # two bit patterns, no -0.0, no NaN
        assert torch.equal(bits(ld_), bits(level.cuda()))                 # the levels are read, not written
        mask2 = torch.full((n,), NAN, device="cuda")                      # a second call: bitwise the first
        assert torch.equal(bits(ops.keep_threshold_indexed(ld_, thrd, mask2, step_idx)), b)
        results[idx] = mask.clone()
    if n > 64:
        # equality releases the frame, NaN gives 0, and the rows differ, so the selection was seen
        for r, t in enumerate(thr.tolist()):
            at = level == t
            assert bool((results[r].cpu()[at] == 0).all())
        assert bool((results[0].cpu()[torch.isnan(level)] == 0).all())
        assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
    # a one-row table: every counter selects it
    one = thrd[1:2]
    assert torch.equal(bits(ops.keep_threshold_indexed(ld_, one, torch.empty_like(ld_), counter(7))), bits((ld_ > one[0]).float()))


@pytest.mark.parametrize("n", G.KERNEL_N[2:])
def test_a_pointer_off_by_one_float_takes_the_scalar_path_and_gives_the_same_bits(n):
    from audioldm2_amd import ops
    level, thr = G.kernel_inputs(n, seed=1)
    ld_, thrd, idx = level.cuda(), thr.cuda(), counter(2)
    ref = ops.keep_threshold_indexed(ld_, thrd, torch.empty_like(ld_), idx)
    assert ld_.data_ptr() % 16 == 0 and ref.data_ptr() % 16 == 0 and n % 4 == 0
    assert torch.equal(bits(ref), bits((ld_ > thrd[2]).float()))

    def off(t, fill=-777.0):
        buf = torch.full((t.numel() + 1 + 2 * A.GUARD,), fill, device="cuda")
        u = buf[A.GUARD + 1:A.GUARD + 1 + t.numel()].view(t.shape).copy_(t)
        assert u.data_ptr() % 16 == 4
        return u, buf
    mu, mbuf = off(torch.zeros_like(ld_))
    assert torch.equal(bits(ops.keep_threshold_indexed(ld_, thrd, mu, idx)), bits(ref))
    assert bool((mbuf[:A.GUARD + 1] == -777.0).all()) and bool((mbuf[-A.GUARD:] == -777.0).all())
    lu, _ = off(ld_)
    mask, buf = A.guarded((n,))
    assert torch.equal(bits(ops.keep_threshold_indexed(lu, thrd, mask, idx)), bits(ref)) and A.guards_intact(buf)


def test_wrapper_refuses_what_it_cannot_run_and_launches_nothing():
    from audioldm2_amd import ops
    n = 64
    level, thr = G.kernel_inputs(n)
    buf = torch.full((2 * n,), .5, device="cuda")
    ld_, thrd, mask = buf[:n], thr.cuda(), torch.full((n,), -5.0, device="cuda")
    with pytest.raises(RuntimeError, match="keep_threshold.mask overlaps level"):
        ops.keep_threshold_indexed(ld_, thrd, ld_)
    with pytest.raises(RuntimeError, match="keep_threshold.mask overlaps level"):
        ops.keep_threshold_indexed(ld_, thrd, buf[n - 1:2 * n - 1])
    assert bool((buf == .5).all())                                       # nothing ran
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.keep_threshold_indexed(level, thrd, mask)                    # a host tensor
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.keep_threshold_indexed(ld_, thrd.double(), mask)
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.keep_threshold_indexed(ld_, thrd, torch.empty(n, 2, device="cuda")[:, 0])
    with pytest.raises(RuntimeError, match="keep_threshold.mask: expected"):
        ops.keep_threshold_indexed(ld_, thrd, mask[:32])
    with pytest.raises(RuntimeError, match="keep_threshold.mask: expected"):
        ops.keep_threshold_indexed(ld_.view(8, 8), thrd, mask)
    with pytest.raises(RuntimeError, match="keep_threshold.thr_tab: expected"):
        ops.keep_threshold_indexed(ld_, thrd.view(1, 3), mask)
    with pytest.raises(RuntimeError, match="keep_threshold.thr_tab: expected"):
        ops.keep_threshold_indexed(ld_, thrd[:0], mask)
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.keep_threshold_indexed(ld_, thrd, mask, torch.zeros(1, device="cuda"))
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.keep_threshold_indexed(ld_, thrd, mask, torch.zeros(1, dtype=torch.int32))
    assert bool((mask == -5.0).all()) and bool((buf == .5).all())


# ---- 2. the samplers on the tiny UNet --------------------------------------------------------------------------------------------------
STEPS, RESAMPLE, VISITS, SEED = Ls.STEPS, (2, 2), 12, 13


@pytest.fixture(scope="module")
def tiny():
    """The tiny model, two distinct seeded conditionings (the prompts of the row plan) and the unconditional one."""
    from oracle import cases
    m = A.TinyModel()
    B = A.TINY_SHAPE[0]

    def conditioning(seed):
        _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=seed)
        return ([c.cuda() for c in ctxs], [k.cuda() for k in masks])
    return m, [conditioning(1), conditioning(3)], conditioning(2)


def x_start(shape, seed=3):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sampler_class(name):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp_2m": DPMSolverSampler}[name]


def case(kind, tiny, levels=None):
    """One way of keeping a source -> the latent shape, the source, its level map [T], `kw(mask, graded)`: the sampler's keywords for
    a run under that mask (fresh per run), the model the composition loop steps, the conditioning of either side."""
    from audioldm2_amd.windows import PerPrompt, window_plan, with_source
    m, prompts, _ = tiny
    linear = window_plan(*Ls.LONG_KEY)
    shape = A.TINY_SHAPE if kind == "masked" else Ls.LONG_SHAPE
    if levels is None:
        levels = G.tiny_levels() if kind == "masked" else G.long_levels(linear, ring=kind == "ring")
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    c = dict(shape=shape, x0=x0, levels=levels, level4=G.level4(levels, shape), cond=prompts[0], loop_cond=prompts[0])
    if kind == "masked":
        c.update(model=m, kw=lambda mask, graded: dict(mask=mask.view(1, 1, -1, 1), x0=x0, **({"graded": True} if graded else {})))
        return c
    if kind == "linear":
        plan = linear
        c["model"] = Wd.WindowedModel(m, plan)
    elif kind == "ring":
        plan = Lp.ring_plan(Ls.LONG_KEY)
        c["model"] = Lp.RingModel(m, plan)
    else:
        plan = Tl.plans_of(Ls.LONG_KEY, [20], 4)[1]
        assert kind == "rows" and plan.R > plan.W
        c.update(model=Tl.TimelineModel(m, plan), cond=PerPrompt(prompts), loop_cond=prompts)
    c["kw"] = lambda mask, graded: dict(windows=with_source(plan, x0, mask, graded=True) if graded else with_source(plan, x0, mask))
    return c


def run(name, tiny, c, mask=None, graded=True, eta=0.0, use_graph=None, **kw):
    """One run over the STEPS-step schedule from a fixed x_T under the seed -> (latent, the rand(1) that follows it).  `mask`: the
    [T] vector the run is given (default: the case's level map)."""
    m, _, uncond = tiny
    shape = c["shape"]
    s = sampler_class(name)(m)
    if use_graph is not None:
        s.use_graph = use_graph
    torch.manual_seed(SEED)
    out, _ = s.sample(STEPS, shape[0], shape[1:], c["cond"], eta=eta, verbose=False, unconditional_guidance_scale=A.GS,
                      unconditional_conditioning=uncond, x_T=x_start(shape), t_start=STEPS,
                      **dict(c["kw"](c["levels"] if mask is None else mask, graded), **kw))
    return out, float(torch.rand(1))


def loop(name, tiny, c, eta=0.0, guidance_rescale=0.0, resample=None):
    """The composition loop of the same job -> (latent, the rand(1) after its draws by hand, the number of visits)."""
    _, _, uncond = tiny
    args = (c["model"], x_start(c["shape"]), c["x0"], c["level4"], c["loop_cond"], uncond)
    torch.manual_seed(SEED)
    visits = STEPS
    if name == "ddim":
        ref, visits = G.ddim_graded_loop(*args, STEPS, STEPS, A.GS, eta=eta, guidance_rescale=guidance_rescale, resample=resample or (1, 1))
    elif name == "plms":
        ref = G.plms_graded_loop(*args, STEPS)
    else:
        ref = G.dpmpp_graded_loop(*args, STEPS)
    return ref, float(torch.rand(1)), visits


# name -> (sampler, way of keeping the source, keywords)
CONFIGS = {"ddim-masked": ("ddim", "masked", {}), "ddim-masked-eta1": ("ddim", "masked", dict(eta=1.0)), "ddim-linear": ("ddim", "linear", {}),
           "ddim-linear-rescale": ("ddim", "linear", dict(guidance_rescale=0.7)), "ddim-ring": ("ddim", "ring", {}),
           "ddim-rows": ("ddim", "rows", {}), "ddim-linear-resample": ("ddim", "linear", dict(resample=RESAMPLE)),
           "plms-masked": ("plms", "masked", {}), "plms-linear": ("plms", "linear", {}),
           "dpmpp-masked": ("dpmpp_2m", "masked", {}), "dpmpp-linear": ("dpmpp_2m", "linear", {})}
# the host generator's draws per visit at the latent's shape (x_T is given): DDIM q-noise and step noise; PLMS q-noise and its own
# (one more in step 0); DPM-Solver++ the q-noise
DRAWS = {"ddim": lambda v: 2 * v, "plms": lambda v: 2 * v + 1, "dpmpp_2m": lambda v: v}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_graded_sampler_equals_the_composition_loop(tiny, cfg):
    """On the parent commit the samplers swallow the unknown keyword (and with_source refuses it) and mix linearly: this test fails
    there."""
    name, kind, kw = CONFIGS[cfg]
    c = case(kind, tiny)
    out, rand_after = run(name, tiny, c, **kw)
    assert tuple(out.shape) == c["shape"] and bool(torch.isfinite(out).all())
    ref, rand_ref, visits = loop(name, tiny, c, **kw)
    assert visits == (VISITS if "resample" in kw else STEPS)
    e = A.rel_rms(out, ref)
    print(f"graded {cfg}, {STEPS} steps, {visits} visits vs the composition loop: {e:.2e}  bar {LOOP_BAR:.1e}")
    assert log_err(e, LOOP_BAR, f"graded {cfg}") < LOOP_BAR
    # the host generator: the plain job's draws, where the loop's draws by hand end
    assert rand_after == rand_ref == G.draws_after(SEED, c["shape"], DRAWS[name](visits))
    if name == "ddim":
        assert rand_after == Rs.draws_after(SEED, c["shape"], visits, x_T_drawn=False)
    # the levels matter: the graded run is neither of the two binary readings of its map
    for what, mask in (("level > 0", (c["levels"] > 0).float()), ("level == 1", (c["levels"] == 1).float())):
        binary, rand_binary = run(name, tiny, c, mask=mask, graded=False, **kw)
        d = A.rel_rms(out, binary)
        print(f"graded {cfg}: vs the binary run mask = ({what}): rel rms {d:.2e}")
        log_err(d, 1e-3, f"graded {cfg}, distance from mask = ({what}) (a lower bound)")
        assert d > 1e-3 and rand_binary == rand_after


@pytest.mark.parametrize("kind", ["masked", "linear"])
def test_binary_levels_are_bitwise_the_run_without_the_keyword(tiny, kind, monkeypatch):
    from audioldm2_amd import ops
    from audioldm2_amd.windows import keep_mask
    calls, real = [], ops.keep_threshold_indexed

    def threshold(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "keep_threshold_indexed", threshold)
    keep = [(0, 5), (9, 12)] if kind == "masked" else Ls.KEEP
    c = case(kind, tiny, levels=keep_mask(A.TINY_SHAPE[2] if kind == "masked" else Ls.LONG_SHAPE[2], keep))
    for name in ("ddim", "plms", "dpmpp_2m"):
        eta = 1.0 if name == "ddim" else 0.0
        graded, rand_graded = run(name, tiny, c, eta=eta)
        assert len(calls) > 0, f"{name}: the graded run did not threshold"     # the keyword was not swallowed
        del calls[:]
        plain, rand_plain = run(name, tiny, c, graded=False, eta=eta)
        assert len(calls) == 0
        assert torch.equal(bits(graded), bits(plain)) and rand_graded == rand_plain, name


@pytest.mark.parametrize("kind", ["masked", "linear"])
def test_the_step_graph_is_captured_once_and_the_eager_run_is_bitwise_the_same(tiny, kind, monkeypatch):
    """A windowed run issues the threshold launch inside the step: twice from Python (the eager first step and the capture), then
    it is a node of the replayed graph.  The plain masked loop issues it from the host in front of every blend."""
    from audioldm2_amd import ddim, ops
    steppers, calls = [], []

    class Recording(ddim.GraphStepper):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            steppers.append(self)
    real = ops.keep_threshold_indexed

    def threshold(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ddim, "GraphStepper", Recording)
    monkeypatch.setattr(ops, "keep_threshold_indexed", threshold)
    c = case(kind, tiny)
    out, rand_after = run("ddim", tiny, c, eta=1.0, use_graph=True)
    assert len(steppers) == 1 and steppers[0].use_graph and steppers[0].calls == STEPS and steppers[0].graph is not None
    assert len(calls) == (STEPS if kind == "masked" else 2)
    del calls[:]
    eager, rand_eager = run("ddim", tiny, c, eta=1.0, use_graph=False)
    assert len(steppers) == 2 and steppers[1].graph is None and len(calls) == STEPS
    assert torch.equal(bits(eager), bits(out)) and rand_eager == rand_after
    again, rand_again = run("ddim", tiny, c, eta=1.0, use_graph=True)
    assert torch.equal(bits(again), bits(out)) and rand_again == rand_after


@pytest.mark.parametrize("kind", ["masked", "linear"])
def test_without_the_keyword_the_launch_is_never_issued_and_a_level_map_mixes_linearly(tiny, kind, monkeypatch):
    from audioldm2_amd import ops

    def never(*a, **k):
        raise AssertionError("ops.keep_threshold_indexed was called without graded=True")
    monkeypatch.setattr(ops, "keep_threshold_indexed", never)
    m, prompts, uncond = tiny
    c = case(kind, tiny)
    for name in ("ddim", "plms", "dpmpp_2m"):
        out, _ = run(name, tiny, c, graded=False)
        assert bool(torch.isfinite(out).all())
    if kind == "linear":
        # today's behaviour of a non-binary mask: the linear mix of tests/long_source.py's loop, not a threshold
        out, rand_after = run("ddim", tiny, c, graded=False)
        torch.manual_seed(SEED)
        ref = Ls.ddim_source_loop(m, c["model"].plan, x_start(c["shape"]), c["x0"], c["level4"], prompts[0], uncond, STEPS, A.GS, k=STEPS)
        assert float(torch.rand(1)) == rand_after
        e = A.rel_rms(out, ref)
        print(f"a level map without graded=True vs the linear-mix loop: {e:.2e}  bar {LOOP_BAR:.1e}")
        assert log_err(e, LOOP_BAR, "level map, linear mix") < LOOP_BAR


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED, E2E_TEXT = 384, 128, 4, 42, "rain on a tin roof"
E2E_KEEP, E2E_FEATHER = [(0.0, 4.0), (4.0, 6.0, 0.5)], 1.0


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def source_audio():
    """A seeded synthetic 6 s recording at 16 kHz: two tones under a slow envelope, and a little noise."""
    rng = np.random.RandomState(0)
    t = np.arange(6 * 16000) / 16000.0
    return ((np.sin(2 * np.pi * 220.0 * t) + 0.5 * np.sin(2 * np.pi * 1330.0 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
            + 0.05 * rng.randn(t.shape[0])).astype(np.float32)


def extend_job(ld, **kw):
    from audioldm2_amd import extend_audio
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = extend_audio(ld, E2E_TEXT, source_audio(), duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS,
                        guidance_scale=A.GS, **kw)
    return wave, ld.last_long_latent.clone(), ld.last_long_source.clone(), float(torch.rand(1))


def test_extend_audio_with_levels_and_a_feather_end_to_end(ld, monkeypatch):
    from audioldm2_amd import ops
    from audioldm2_amd.pipeline import keep_frames, make_batch_for_text_to_audio, seed_everything
    from audioldm2_amd.sampling import hold_steps, make_ddim_timesteps
    from audioldm2_amd.windows import keep_levels
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, _ = ld.long_form_plans(E2E_T, E2E_HOP)
    S = len(make_ddim_timesteps("uniform", E2E_STEPS, ld.num_timesteps, verbose=False))
    frames, feather = keep_frames(E2E_KEEP, ld.latent_t_per_second, E2E_T), int(round(E2E_FEATHER * ld.latent_t_per_second))
    assert S == 4 and frames == [(0, 102), (103, 153, 0.5)] and feather == 26
    levels = keep_levels(E2E_T, frames, feather)
    assert [hold_steps(m, S) for m in (1.0, .5, 0.0)] == [4, 2, 0]
    wave, latent, z, rand_after = extend_job(ld, keep=E2E_KEEP, feather=E2E_FEATHER)
    C, F_ = ld.channels, ld.latent_f_size
    assert tuple(latent.shape) == tuple(z.shape) == (1, C, E2E_T, F_) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert ld.latent_t_size == 256 and len(unet._graph_cache) == 0     # a graded run stays out of the cross-run graph cache too
    # the host generator after the job: the plain job's
    assert rand_after == Ls.expected_rand_after_source(E2E_SEED, 1, (C, E2E_T, F_), S)

    # the latent: the graded composition loop — the job's draws by hand, the job's own source latent
    seed_everything(E2E_SEED)
    torch.randn((1, C, E2E_T, F_))
    cond = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(E2E_TEXT))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    ref, _ = G.ddim_graded_loop(Wd.WindowedModel(ld, plan), torch.randn((1, C, E2E_T, F_)), z, G.level4(levels, (1, C, E2E_T, F_)),
                                cond, uncond, E2E_STEPS, S, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"graded extend_audio latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "graded long source latent") <= latent_tol(E2E_STEPS)

    # the distance from the source follows the levels (comparative only)
    full, half, free = (levels == 1).nonzero().view(-1), (levels == .5).nonzero().view(-1), (levels == 0).nonzero().view(-1)
    assert len(full) == 102 and len(half) == 50 and len(free) > 100
    d = [A.rel_rms(latent[:, :, idx.cuda()], z[:, :, idx.cuda()]) for idx in (full, half, free)]
    print(f"graded extend_audio final latent vs the source latent: level 1 {d[0]:.3e}, level 0.5 {d[1]:.3e}, generated {d[2]:.3e} (rel rms)")
    assert d[0] < d[1] < d[2]

    # a second identical job is bitwise the first
    wave2, latent2, z2, rand2 = extend_job(ld, keep=E2E_KEEP, feather=E2E_FEATHER)
    assert torch.equal(latent2, latent) and torch.equal(z2, z) and np.array_equal(wave2, wave) and rand2 == rand_after

    # without levels and feather the job is today's: the launch is never issued, the default keep is [0, 6 s)
    def never(*a, **k):
        raise AssertionError("ops.keep_threshold_indexed was called by a job without levels")
    monkeypatch.setattr(ops, "keep_threshold_indexed", never)
    default = extend_job(ld)
    for kw in (dict(keep=[(0.0, 6.0)]), dict(keep=[(0.0, 6.0)], feather=0.0), dict(keep=[(0.0, 6.0, 1.0)])):
        wave3, latent3, z3, rand3 = extend_job(ld, **kw)
        assert torch.equal(latent3, default[1]) and torch.equal(z3, z) and np.array_equal(wave3, default[0]) and rand3 == default[3], kw
    d = A.rel_rms(latent, default[1])
    print(f"graded extend_audio vs the plain keep of [0, 6 s): rel rms {d:.2e}")
    assert d > 1e-3
    unet.drop_step_caches()
