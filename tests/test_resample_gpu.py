"""GPU tests of resampled inpainting (RePaint's jumps): aldm_renoise_indexed against torch's fp32 expression (bitwise)
and against fp64 of the same fp32 inputs (bar: two rounded products and one rounded sum, tests/resample.py), its device-side row
selection, both access paths, bounds and refusals; DDIMSampler with `resample=` on the tiny UNet — the masked path, and a source on
a linear, a ring and a row plan — against the composition loop of tests/resample.py (the draws by hand in contract order, torch
blend + p_sample_ddim on step visits, a torch axpby on renoise visits); n = 1 against the run without the keyword (bitwise); the
host generator after a job; the step graph captured once; generate_batch_long_from_audio end to end.

The bar of a sampler against its composition loop is 1e-5 relative rms, the project's bar for sampler compositions,
in the default fp32-grade matrix modes."""
import numpy as np
import pytest
import torch

import audio2audio as A
import long_source as Ls
import looped as Lp
import resample as Rs
import timeline as Tl
import windowed as Wd
from tolerances import log_err, mel_tol

pytestmark = pytest.mark.gpu

LOOP_BAR = 1e-5


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
def torch_renoise(x, noise, coef, s):
    """coef[s, 0] * x + coef[s, 1] * noise[s], by torch in fp32 on the device: two products and a sum, each its own launch."""
    return coef[s, 0] * x + coef[s, 1] * noise[s]


@pytest.mark.parametrize("n", Rs.KERNEL_N)
def test_renoise_is_bitwise_the_torch_expression_and_within_three_roundings_of_fp64(n):
    from audioldm2_amd import ops
    x, noise, coef = Rs.kernel_inputs(n, seed=n)
    xd, noised, coefd = x.cuda(), noise.cuda(), coef.cuda()
    assert not torch.equal(noise[0], noise[1]) and not torch.equal(noise[1], noise[2]) and not torch.equal(coef[0], coef[2])
    results = []
    for idx in (0, 1, 2, None):
        s = 0 if idx is None else idx
        xg, buf = A.guarded((n,))
        xg.copy_(xd)
        step_idx = None if idx is None else torch.full((1,), idx, device="cuda", dtype=torch.int32)
        got = ops.renoise_indexed(xg, noised, coefd, step_idx)
        assert got is xg and A.guards_intact(buf)
        if step_idx is not None:
            assert int(step_idx) == idx                                  # the counter is read, not written
        assert torch.equal(bits(xg), bits(torch_renoise(xd, noised, coefd, s))), f"n={n} row {idx}: not the torch fp32 expression"
        t0, t1 = coef[s, 0].double() * x.double(), coef[s, 1].double() * noise[s].double()
        den = t0.abs() + t1.abs()
        err = (xg.double().cpu() - (t0 + t1)).abs()
        assert bool((err <= Rs.KERNEL_BAR * den).all()), f"n={n} row {idx}"
        worst = float((err / den).max())
        print(f"renoise_indexed n={n} row {idx}: max |err| / (|c0 x| + |c1 eps|) = {worst:.3e}  bar {Rs.KERNEL_BAR:.3e}")
        log_err(worst, Rs.KERNEL_BAR, f"renoise_indexed n={n} row {idx}")
        x2 = xd.clone()                                                  # a second call: bitwise the first
        assert torch.equal(bits(ops.renoise_indexed(x2, noised, coefd, step_idx)), bits(xg))
        results.append(xg.clone())
    assert torch.equal(results[0], results[3])                          # no counter: row 0
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])   # the selection was seen
    # the table may be one row of the latent's own shape
    x3 = xd.clone()
    assert torch.equal(bits(ops.renoise_indexed(x3, noised[0].contiguous(), coefd)), bits(results[0]))


@pytest.mark.parametrize("n", Rs.KERNEL_N[2:])
def test_a_pointer_off_by_one_float_takes_the_scalar_path_and_gives_the_same_bits(n):
    from audioldm2_amd import ops
    x, noise, coef = Rs.kernel_inputs(n, seed=1)
    xd, noised, coefd = x.cuda(), noise.cuda(), coef.cuda()
    idx = torch.full((1,), 2, device="cuda", dtype=torch.int32)
    ref = ops.renoise_indexed(xd.clone(), noised, coefd, idx)
    assert xd.data_ptr() % 16 == 0 and noised.data_ptr() % 16 == 0 and n % 4 == 0

    def off(t):
        buf = torch.full((t.numel() + 1 + 2 * A.GUARD,), -777.0, device="cuda")
        u = buf[A.GUARD + 1:A.GUARD + 1 + t.numel()].view(t.shape).copy_(t)
        assert u.data_ptr() % 16 == 4
        return u, buf
    xu, xbuf = off(xd)
    assert torch.equal(bits(ops.renoise_indexed(xu, noised, coefd, idx)), bits(ref))
    assert bool((xbuf[:A.GUARD + 1] == -777.0).all()) and bool((xbuf[-A.GUARD:] == -777.0).all())
    nu, _ = off(noised)
    assert torch.equal(bits(ops.renoise_indexed(xd.clone(), nu, coefd, idx)), bits(ref))


def test_wrapper_refuses_what_it_cannot_run_and_launches_nothing():
    from audioldm2_amd import ops
    n = 64
    x, noise, coef = Rs.kernel_inputs(n)
    xd, noised, coefd = x.cuda(), noise.cuda(), coef.cuda()
    tab = noise.cuda()
    with pytest.raises(RuntimeError, match="renoise.x overlaps noise_tab"):
        ops.renoise_indexed(tab[2], tab, coefd)                          # the LAST row of the table: the wrapper knows the rows
    with pytest.raises(RuntimeError, match="renoise.x overlaps noise_tab"):
        ops.renoise_indexed(tab[0], tab, coefd)
    assert torch.equal(tab, noised)                                      # nothing ran
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.renoise_indexed(x, noised, coefd)                            # a host tensor
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.renoise_indexed(xd, noised.double(), coefd)
    with pytest.raises(RuntimeError, match="renoise.noise_tab: expected"):
        ops.renoise_indexed(xd, noised[:, :32].contiguous(), coefd)
    with pytest.raises(RuntimeError, match="renoise.coef_tab: expected"):
        ops.renoise_indexed(xd, noised, coefd[:, :1].contiguous())
    with pytest.raises(RuntimeError, match="renoise.coef_tab: expected"):
        ops.renoise_indexed(xd, noised, coefd[0].contiguous())
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.renoise_indexed(xd, noised, coefd, torch.zeros(1, device="cuda"))
    assert torch.equal(xd, x.cuda())


# ---- 2. the sampler on the tiny UNet --------------------------------------------------------------------------------------------------
STEPS, RESAMPLE, VISITS, SEED = Ls.STEPS, (2, 2), 12, 11
KEEP_TINY = [(0, 5), (9, 12)]


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


def case(kind, tiny):
    """One way of keeping a source -> the latent shape, the source and its frame mask, the sampler's keywords (fresh per run),
    the model the composition loop steps, the conditioning of either side."""
    from audioldm2_amd.windows import PerPrompt, keep_mask, window_plan, with_source
    m, prompts, _ = tiny
    shape, keep = (A.TINY_SHAPE, KEEP_TINY) if kind == "masked" else (Ls.LONG_SHAPE, Ls.KEEP)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    mask = keep_mask(shape[2], keep)
    c = dict(shape=shape, x0=x0, mask4=mask.view(1, 1, -1, 1).expand(shape).contiguous(), cond=prompts[0], loop_cond=prompts[0])
    if kind == "masked":
        c.update(model=m, kw=lambda: dict(mask=mask.view(1, 1, -1, 1), x0=x0))
        return c
    if kind == "linear":
        plan = window_plan(*Ls.LONG_KEY)
        c["model"] = Wd.WindowedModel(m, plan)
    elif kind == "ring":
        plan = Lp.ring_plan(Ls.LONG_KEY)
        c["model"] = Lp.RingModel(m, plan)
    else:
        plan = Tl.plans_of(Ls.LONG_KEY, [20], 4)[1]
        assert kind == "rows" and plan.R > plan.W
        c.update(model=Tl.TimelineModel(m, plan), cond=PerPrompt(prompts), loop_cond=prompts)
    c["kw"] = lambda: dict(windows=with_source(plan, x0, mask))
    return c


def run(tiny, c, resample=None, eta=0.0, steps=STEPS, use_graph=None, x_T="given", **kw):
    """One DDIM run over the first `steps` entries of the `steps`-step schedule -> (latent, the rand(1) that follows it)."""
    from audioldm2_amd.ddim import DDIMSampler
    m, _, uncond = tiny
    shape = c["shape"]
    s = DDIMSampler(m)
    if use_graph is not None:
        s.use_graph = use_graph
    args = dict(c["kw"](), **kw)
    if resample is not None:
        args["resample"] = resample
    if x_T == "given":
        args.update(x_T=x_start(shape), t_start=steps)
    torch.manual_seed(SEED)
    out, _ = s.sample(steps, shape[0], shape[1:], c["cond"], eta=eta, verbose=False, unconditional_guidance_scale=A.GS,
                      unconditional_conditioning=uncond, **args)
    return out, float(torch.rand(1))


def loop(tiny, c, eta=0.0, guidance_rescale=0.0):
    m, _, uncond = tiny
    torch.manual_seed(SEED)
    ref, visits = Rs.resample_loop(c["model"], x_start(c["shape"]), c["x0"], c["mask4"], c["loop_cond"], uncond, STEPS, STEPS,
                                   RESAMPLE[0], RESAMPLE[1], A.GS, eta=eta, guidance_rescale=guidance_rescale)
    assert visits == VISITS
    return ref, float(torch.rand(1))


CONFIGS = {"masked": ("masked", {}), "masked-eta1": ("masked", dict(eta=1.0)), "linear": ("linear", {}),
           "linear-rescale": ("linear", dict(guidance_rescale=0.7)), "ring": ("ring", {}), "rows": ("rows", {})}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_resampled_sampler_equals_the_composition_loop(tiny, cfg):
    """On the parent commit DDIMSampler.sample swallows the unknown keyword and runs the plain schedule: this test fails there."""
    kind, kw = CONFIGS[cfg]
    c = case(kind, tiny)
    out, rand_after = run(tiny, c, RESAMPLE, **kw)
    assert tuple(out.shape) == c["shape"] and bool(torch.isfinite(out).all())
    ref, rand_ref = loop(tiny, c, **kw)
    e = A.rel_rms(out, ref)
    print(f"resample={RESAMPLE} {cfg}, {STEPS} steps, {VISITS} visits vs the composition loop: {e:.2e}  bar {LOOP_BAR:.1e}")
    assert log_err(e, LOOP_BAR, f"resample {cfg}") < LOOP_BAR
    # the host generator: two draws per visit at the latent's shape (x_T was given), and where the loop's draws by hand end
    assert rand_after == rand_ref == Rs.draws_after(SEED, c["shape"], VISITS, x_T_drawn=False)
    # the keyword matters: the same run without it is somewhere else
    plain, rand_plain = run(tiny, c, None, **kw)
    d = A.rel_rms(out, plain)
    print(f"resample={RESAMPLE} {cfg}: vs the run without the keyword: rel rms {d:.2e}")
    log_err(d, 1e-3, f"resample {cfg}, distance from the plain run (a lower bound)")
    assert d > 1e-3
    assert rand_plain == Rs.draws_after(SEED, c["shape"], STEPS, x_T_drawn=False) != rand_after
    # a second run is bitwise the first
    out2, rand2 = run(tiny, c, RESAMPLE, **kw)
    assert torch.equal(out2, out) and rand2 == rand_after


@pytest.mark.parametrize("kind", ["masked", "linear"])
def test_n_equal_one_is_bitwise_the_run_without_the_keyword(tiny, kind):
    c = case(kind, tiny)
    one, rand_one = run(tiny, c, (1, 2), eta=1.0)
    plain, rand_plain = run(tiny, c, None, eta=1.0)
    assert torch.equal(bits(one), bits(plain)) and rand_one == rand_plain


def test_a_job_that_draws_x_T_leaves_the_generator_after_x_T_and_two_draws_per_visit(tiny):
    """Five steps (the uniform grid of 5 has 5 entries), no x_T: (5, 2, 2) is 11 visits, an odd run whose first jump point is 3."""
    from audioldm2_amd.sampling import resample_visits
    c = case("masked", tiny)
    S, m, uncond = 5, tiny[0], tiny[2]
    V = len(resample_visits(S, *RESAMPLE))
    assert V == 11
    out, rand_after = run(tiny, c, RESAMPLE, eta=1.0, steps=S, x_T=None)
    assert rand_after == Rs.draws_after(SEED, c["shape"], V, x_T_drawn=True)
    torch.manual_seed(SEED)
    x_T = torch.randn(c["shape"])
    ref, visits = Rs.resample_loop(m, x_T, c["x0"], c["mask4"], c["loop_cond"], uncond, S, S, *RESAMPLE, A.GS, eta=1.0)
    assert visits == V and float(torch.rand(1)) == rand_after
    e = A.rel_rms(out, ref)
    print(f"resample={RESAMPLE} masked, 5 steps from a drawn x_T, eta 1 vs the composition loop: {e:.2e}  bar {LOOP_BAR:.1e}")
    assert log_err(e, LOOP_BAR, "resample masked S=5 drawn x_T") < LOOP_BAR


@pytest.mark.parametrize("kind", ["masked", "linear"])
def test_the_step_graph_is_captured_once_and_the_eager_run_is_bitwise_the_same(tiny, kind, monkeypatch):
    from audioldm2_amd import ddim, ops
    steppers, seen = [], []

    class Recording(ddim.GraphStepper):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            steppers.append(self)
    real = ops.renoise_indexed

    def renoise(*a, **k):
        before = (steppers[-1].graph, steppers[-1].calls)
        out = real(*a, **k)
        seen.append(before + (steppers[-1].graph,))
        return out
    monkeypatch.setattr(ddim, "GraphStepper", Recording)
    monkeypatch.setattr(ops, "renoise_indexed", renoise)
    c = case(kind, tiny)
    out, _ = run(tiny, c, RESAMPLE, use_graph=True)
    assert len(steppers) == 1 and steppers[0].use_graph
    st = steppers[0]
    assert st.calls == VISITS - 2 and [s[1] for s in seen] == [4, 8]   # ten step visits; the jumps follow steps 3 and 5
    g = st.graph
    assert g is not None and all(s[0] is g and s[2] is g for s in seen)  # one graph object, before and after every renoise visit
    eager, _ = run(tiny, c, RESAMPLE, use_graph=False)
    assert len(steppers) == 2 and steppers[1].graph is None and len(seen) == 4
    assert torch.equal(bits(eager), bits(out))


def test_callbacks_see_step_visits_only_with_the_loop_position(tiny):
    c = case("masked", tiny)
    got = []
    cb = lambda i: got.append(i)
    cb.uses_rng = False
    out, rand_after = run(tiny, c, RESAMPLE, callback=cb)
    from audioldm2_amd.sampling import resample_visits
    assert got == [v[1] for v in resample_visits(STEPS, *RESAMPLE) if v[0] == "step"]
    plain, rand_plain = run(tiny, c, RESAMPLE)
    assert torch.equal(out, plain) and rand_after == rand_plain
    # a callback that may draw keeps the feed on the launching thread, one visit at a time: the same draws, the same latent
    got.clear()
    out2, rand2 = run(tiny, c, RESAMPLE, callback=lambda i: got.append(i))
    assert torch.equal(out2, plain) and rand2 == rand_plain and len(got) == VISITS - 2


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED, E2E_TEXT, E2E_RESAMPLE = 384, 128, 4, 42, "rain on a tin roof", (2, 1)


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


def test_generate_batch_long_from_audio_resampled_end_to_end(ld):
    """The smallest end-to-end configuration of tests/test_long_source_gpu.py (the 16 kHz model, 15 s = 384 latent frames, windows
    of 256 at hop 128, the first 6 s kept), resample=(2, 1), ddim_steps=4.  No `ddim_steps` gives a run of three steps through this
    entry point: the uniform grid of ddim_steps=3 is 1, 334, 667, 1000 — four entries, the last past the end of the 1000-entry
    schedule, refused by make_schedule as in the reference — and that of 2 has two.  So the run is the next one up, (4, 2, 1): 7 step
    visits and 3 renoise visits, 10 in all, every position from 2 on a jump point."""
    from audioldm2_amd.pipeline import keep_frames, make_batch_for_text_to_audio, seed_everything, wav_to_fbank
    from audioldm2_amd.sampling import make_ddim_timesteps, resample_visits
    from audioldm2_amd.stft import TacotronSTFT
    from audioldm2_amd.windows import keep_mask
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, E2E_HOP)
    S = len(make_ddim_timesteps("uniform", E2E_STEPS, ld.num_timesteps, verbose=False))
    visits = resample_visits(S, *E2E_RESAMPLE)
    assert S == 4 and len(visits) == 10 and sum(v[0] == "renoise" for v in visits) == 3
    frames = keep_frames([(0.0, 6.0)], ld.latent_t_per_second, E2E_T)
    assert frames == [(0, 153)]
    mel, _, _ = wav_to_fbank(source_audio(), target_length=E2E_T * 4, fn_STFT=TacotronSTFT(1024, 160, 1024, 64, 16000, 0, 8000))
    C, F_ = ld.channels, ld.latent_f_size

    def job():
        batch = make_batch_for_text_to_audio(E2E_TEXT)
        batch["log_mel_spec"] = batch["fbank"] = mel[None, ...].float().cpu()
        ld.conditional_dry_run_finished = False      # the job as an object's first (pipeline._cfg_dropout_draw)
        seed_everything(E2E_SEED)
        wave = ld.generate_batch_long_from_audio(batch, E2E_T, frames, hop=E2E_HOP, unconditional_guidance_scale=A.GS,
                                                 ddim_steps=E2E_STEPS, resample=E2E_RESAMPLE)
        return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), ld.last_long_source.clone(), float(torch.rand(1)), batch
    wave, latent, mel_out, z, rand_after, batch = job()
    assert tuple(latent.shape) == tuple(z.shape) == (1, C, E2E_T, F_) and tuple(mel_out.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.dtype == np.float32 and np.isfinite(wave).all() and ld.latent_t_size == 256
    assert len(unet._graph_cache) == 0            # a run with a source stays out of the cross-run graph cache, resampled or not
    # the host generator: the posterior noise and x_T at the long shape, then two draws per VISIT
    assert rand_after == Rs.draws_after(E2E_SEED, (1, C, E2E_T, F_), len(visits), x_T_drawn=True, before=[(1, C, E2E_T, F_)])

    # the latent handed to the tail: the composition loop — the job's draws by hand, the job's own source latent
    mask4 = keep_mask(E2E_T, frames).view(1, 1, -1, 1).expand(1, C, E2E_T, F_).contiguous()
    seed_everything(E2E_SEED)
    torch.randn((1, C, E2E_T, F_))
    cond = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(E2E_TEXT))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    ref, n_visits = Rs.resample_loop(Wd.WindowedModel(ld, plan), torch.randn((1, C, E2E_T, F_)), z, mask4, cond, uncond, E2E_STEPS, S,
                                     *E2E_RESAMPLE, A.GS, eta=1.0)
    assert n_visits == len(visits) and float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"generate_batch_long_from_audio resample={E2E_RESAMPLE}, {len(visits)} visits: latent vs the composition loop: "
          f"rel rms {e:.2e}  bar {LOOP_BAR:.1e}")
    assert log_err(e, LOOP_BAR, "resample long source latent") < LOOP_BAR

    # the mel is the plan's tail of that latent: the tail run again on it, bitwise, and an fp64 merge of the windows' decodes
    ld._long_tail(latent.clone(), plan, mel_plan, batch)
    assert torch.equal(ld.last_long_mel, mel_out)
    mel_ref = Wd.merge_fp64(ld.decode_first_stage(Wd.gather_ref(latent, plan)), mel_plan)[0]
    e = A.rel_rms(mel_out, mel_ref)
    print(f"resampled long source mel vs the fp64 merge of the windows' decodes: rel rms {e:.2e}  bar {mel_tol(E2E_STEPS):.1e}")
    assert log_err(e, mel_tol(E2E_STEPS), "resample long source mel") <= mel_tol(E2E_STEPS)

    # without the keyword the job is another one
    batch2 = make_batch_for_text_to_audio(E2E_TEXT)
    batch2["log_mel_spec"] = batch2["fbank"] = mel[None, ...].float().cpu()
    ld.conditional_dry_run_finished = False
    seed_everything(E2E_SEED)
    ld.generate_batch_long_from_audio(batch2, E2E_T, frames, hop=E2E_HOP, unconditional_guidance_scale=A.GS, ddim_steps=E2E_STEPS)
    d = A.rel_rms(latent, ld.last_long_latent)
    print(f"resampled long source latent vs the job without the keyword: rel rms {d:.2e}")
    assert d > 1e-3 and torch.equal(ld.last_long_source, z)
    unet.drop_step_caches()
