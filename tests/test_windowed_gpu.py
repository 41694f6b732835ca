"""GPU tests of long-form generation (windowed diffusion): aldm_window_gather against torch slicing (bitwise),
aldm_window_merge against an fp64 overlap-add of the same fp32 inputs (bar: cover * 2^-24 of the sum of the terms' magnitudes,
tests/windowed.py), its bit-exact cases, NaN propagation and bounds; the three samplers with `windows=` on the tiny UNet against the
composition loop (slice, run the same model, merge in fp64, the sampler's eager single-step form); the degenerate one-window plan
against the run without a plan (bitwise); LatentDiffusion.generate_batch_long / text_to_audio_long end to end."""
import numpy as np
import pytest
import torch

import audio2audio as A
import windowed as Wd
from tolerances import latent_tol, log_err, mel_tol

pytestmark = pytest.mark.gpu


def plan_of(key, scale=1):
    from audioldm2_amd.windows import window_plan
    return window_plan(*key, scale=scale)


def case_id(c):
    B, key, C, F = c
    return f"B{B}-T{key[0]}w{key[1]}h{key[2]}-C{C}-F{F}"


# ---- 1. the gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Wd.KERNEL_CASES + [Wd.MEL_CASE], ids=case_id)
def test_gather_is_bitwise_torch_slicing(case):
    from audioldm2_amd import ops
    B, key, C, F = case
    plan = plan_of(key)
    x, _ = Wd.window_inputs(B, plan, C, F)
    x = x.cuda()
    out, buf = A.guarded((plan.W * B, C, plan.Tw, F))
    got = ops.window_gather(x, plan, out=out)
    assert got is out and torch.equal(out, Wd.gather_ref(x, plan))
    assert A.guards_intact(buf)
    assert torch.equal(ops.window_gather(x, plan), out)            # the allocating form


def test_gather_and_merge_from_unaligned_pointers_take_the_scalar_path():
    """F % 4 == 0 but the tensors start 4 bytes off a 16-byte boundary: the same results as the aligned launches."""
    from audioldm2_amd import ops
    B, key, C, F = 1, (40, 16, 10), 3, 16
    plan = plan_of(key)
    x, win = Wd.window_inputs(B, plan, C, F, H=2)
    xb = torch.empty(x.numel() + 1, device="cuda")
    xu = xb[1:].view(x.shape).copy_(x)
    assert xu.data_ptr() % 16 == 4
    assert torch.equal(ops.window_gather(xu, plan), Wd.gather_ref(x.cuda(), plan))
    wb = torch.empty(win.numel() + 1, device="cuda")
    wu = wb[1:].view(win.shape).copy_(win)
    ob = torch.empty(2 * x.numel() + 1, device="cuda")
    ou = ob[1:].view((2,) + tuple(x.shape))
    assert torch.equal(ops.window_merge(wu, plan, out=ou), ops.window_merge(win.cuda(), plan))


# ---- 2. the merge against fp64 ----------------------------------------------------------------------------------------------------
MERGE_CASES = [(2,) + c for c in Wd.KERNEL_CASES] + [(1,) + Wd.MEL_CASE]


@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: f"H{c[0]}-" + case_id(c[1:]))
def test_merge_matches_fp64(case):
    from audioldm2_amd import ops
    H, B, key, C, F = case
    plan = plan_of(key)
    _, win = Wd.window_inputs(B, plan, C, F, H=H if H == 2 else None, seed=1)
    win = win.cuda()
    out, buf = A.guarded(((2,) if H == 2 else ()) + (B, C, plan.T, F))
    got = ops.window_merge(win, plan, out=out)
    assert got is out and A.guards_intact(buf)
    ref, den, count = Wd.merge_fp64(win, plan)
    assert int(count.max()) == plan.cover and float(den.min()) > 0.0
    err = float(((out.double() - ref).abs() / den).max())
    bar = Wd.bar(plan)
    print(f"window_merge {case_id(case[1:])} H={H} cover={plan.cover}: max |err| / sum |wn e| = {err:.3e}  bar {bar:.3e}")
    assert log_err(err, bar, f"window_merge {case_id(case[1:])}") <= bar
    # frames under ONE window (wn == 1) reproduce their input bit for bit
    one = (count == 1).nonzero().view(-1).tolist()
    for t in one[:4] + one[-4:]:
        j = max(i for i, s in enumerate(plan.starts) if s <= t < s + plan.Tw)
        assert torch.equal(out[..., t, :], win[..., j * B:(j + 1) * B, :, t - plan.starts[j], :])
    # two runs are bitwise equal, and so is the allocating form
    assert torch.equal(ops.window_merge(win, plan), out.clone())


# ---- 3. the bit-exact plans ---------------------------------------------------------------------------------------------------------
def test_merge_of_one_window_returns_its_input():
    from audioldm2_amd import ops
    plan = plan_of((16, 16, 8))
    for F in (5, 8):
        _, win = Wd.window_inputs(2, plan, 3, F, H=2, seed=2)
        win = win.cuda()
        win[0, 0, 0, 0, 0], win[1, 1, 2, 3, 1] = -0.0, float("inf")
        assert torch.equal(ops.window_merge(win, plan).view(torch.int32), win.view(torch.int32))
        assert torch.equal(ops.window_gather(win[0], plan), win[0])


def test_merge_without_overlap_is_a_concatenation():
    from audioldm2_amd import ops
    plan = plan_of((48, 16, 16))
    assert plan.cover == 1
    for F in (7, 16):
        _, win = Wd.window_inputs(2, plan, 3, F, H=2, seed=3)
        win = win.cuda()
        want = torch.cat([win[:, j * 2:(j + 1) * 2] for j in range(plan.W)], dim=3)
        assert torch.equal(ops.window_merge(win, plan), want)
        x = want[1].contiguous()
        assert torch.equal(ops.window_merge(ops.window_gather(x, plan), plan), x)     # gather then merge: the identity here


# ---- 4. NaN propagation and safety --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 16])
def test_merge_carries_a_nan_to_the_frames_its_window_covers_and_no_further(F):
    from audioldm2_amd import ops
    B, C = 2, 3
    plan = plan_of((40, 16, 10))
    _, win = Wd.window_inputs(B, plan, C, F, H=2, seed=4)
    win = win.cuda()
    h, j, b, c = 1, 2, 1, 2
    win[h, j * B + b, c] = float("nan")
    out, buf = A.guarded((2, B, C, plan.T, F))
    ops.window_merge(win, plan, out=out)
    want = torch.zeros_like(out, dtype=torch.bool)
    want[h, b, c, plan.starts[j]:plan.starts[j] + plan.Tw] = True
    assert torch.equal(torch.isnan(out), want)
    assert A.guards_intact(buf)


def test_wrappers_refuse_what_they_cannot_run():
    from audioldm2_amd import ops
    B, C, F = 2, 3, 8
    plan = plan_of((40, 16, 10))
    x, win = Wd.window_inputs(B, plan, C, F, H=2)
    n_win, n_out = win.numel(), 2 * x.numel()
    buf = torch.zeros(n_win + n_out, device="cuda")
    w = buf[:n_win].view(win.shape).copy_(win)
    with pytest.raises(RuntimeError, match="overlaps win"):
        ops.window_merge(w, plan, out=buf[n_win - 8:n_win - 8 + n_out].view((2,) + tuple(x.shape)))
    with pytest.raises(RuntimeError, match="overlaps x"):
        xs = buf[:x.numel()].view(x.shape)
        ops.window_gather(xs, plan, out=buf[x.numel() - 4:x.numel() - 4 + n_win // 2].view(plan.W * B, C, plan.Tw, F))
    assert bool((buf[n_win:] == 0).all())                      # nothing ran
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.window_merge(win, plan)                            # a host tensor
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.window_gather(x.cuda().double(), plan)
    with pytest.raises(RuntimeError, match="window_gather: x must be"):
        ops.window_gather(x.cuda()[:, :, :32].contiguous(), plan)
    with pytest.raises(RuntimeError, match="window_merge: win must be"):
        ops.window_merge(w[:, :7].contiguous(), plan)
    with pytest.raises(RuntimeError, match="window_merge.out: expected"):
        ops.window_merge(w, plan, out=torch.empty(2, B, C, 48, F, device="cuda"))


# ---- 5. the samplers on the tiny UNet -------------------------------------------------------------------------------------------------
# 6 steps: the first 6 entries of the 6-step grid, which has 7 (1000 // 6 = 166), cut with t_start as tests/test_audio2audio_gpu.py does
LONG_KEY, STEPS = (40, 16, 10), 6
LONG_SHAPE = (A.TINY_SHAPE[0], A.TINY_SHAPE[1], LONG_KEY[0], A.TINY_SHAPE[3])


@pytest.fixture(scope="module")
def tiny():
    m = A.TinyModel()
    cond, uncond = A.tiny_conditioning()
    return m, cond, uncond


def x_long(seed=3, shape=LONG_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sample_kw(uncond, **kw):
    return dict(verbose=False, unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond, **kw)


def run(cls, tiny, plan, shape=LONG_SHAPE, steps=STEPS, **kw):
    m, cond, uncond = tiny
    out, _ = cls(m).sample(steps, shape[0], shape[1:], cond, x_T=x_long(shape=shape), eta=0.0, windows=plan, t_start=steps,
                           **sample_kw(uncond, **kw))
    return out


@pytest.fixture(scope="module")
def references(tiny):
    """The composition loops, computed once."""
    m, cond, uncond = tiny
    plan = plan_of(LONG_KEY)
    return {"ddim": Wd.ddim_loop(m, plan, x_long(), cond, uncond, STEPS, A.GS, k=STEPS),
            "ddim-rescale": Wd.ddim_loop(m, plan, x_long(), cond, uncond, STEPS, A.GS, guidance_rescale=0.7, k=STEPS),
            "plms": Wd.plms_loop(m, plan, x_long(), cond, uncond, STEPS),
            "dpmpp_2m": Wd.dpmpp_loop(m, plan, x_long(), cond, uncond, STEPS)}


def sampler_class(name):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp_2m": DPMSolverSampler}[name]


@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_windowed_sampler_equals_the_composition_loop(tiny, references, name):
    plan = plan_of(LONG_KEY)
    out = run(sampler_class(name), tiny, plan)
    assert tuple(out.shape) == LONG_SHAPE and bool(torch.isfinite(out).all())
    e, bar = A.rel_rms(out, references[name]), A.tstart_bar(STEPS)
    print(f"{name} windows={LONG_KEY} {STEPS} steps vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"windowed {name}") <= bar
    assert A.rel_rms(out, x_long().cuda()) > 1e-3
    # a second job of the same geometry under the same seed: bitwise the first
    assert torch.equal(run(sampler_class(name), tiny, plan), out)


def test_windowed_ddim_with_guidance_rescale_equals_the_loop_with_the_rescale_on_the_merged_pair(tiny, references):
    plan = plan_of(LONG_KEY)
    out = run(sampler_class("ddim"), tiny, plan, guidance_rescale=0.7)
    e, bar = A.rel_rms(out, references["ddim-rescale"]), A.tstart_bar(STEPS)
    print(f"ddim windows={LONG_KEY} guidance_rescale=0.7 vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "windowed ddim rescale") <= bar
    assert A.rel_rms(out, references["ddim"]) > 1e-3          # ... and the rescale matters


def test_windowed_ddim_draws_the_step_noise_at_the_long_shape(tiny):
    """eta 1 without x_T: x_T and one draw per step at the long shape, in DDIMSampler.decode's order (the whole 4-step grid)."""
    from audioldm2_amd.ddim import DDIMSampler
    m, cond, uncond = tiny
    plan = plan_of(LONG_KEY)
    torch.manual_seed(11)
    out, _ = DDIMSampler(m).sample(4, LONG_SHAPE[0], LONG_SHAPE[1:], cond, eta=1.0, windows=plan, **sample_kw(uncond))
    after = float(torch.rand(1))
    torch.manual_seed(11)
    ref = Wd.ddim_loop(m, plan, torch.randn(LONG_SHAPE), cond, uncond, 4, A.GS, eta=1.0)
    assert float(torch.rand(1)) == after
    e, bar = A.rel_rms(out, ref), A.tstart_bar(4)
    print(f"ddim windows eta=1 vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "windowed ddim eta=1") <= bar


# ---- 6. the degenerate plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_one_window_plan_is_bitwise_the_run_without_a_plan(tiny, name):
    cls = sampler_class(name)
    with_plan = run(cls, tiny, plan_of((16, 16, 8)), shape=A.TINY_SHAPE, steps=4)
    without = run(cls, tiny, None, shape=A.TINY_SHAPE, steps=4)
    assert torch.equal(with_plan, without)
    if name == "ddim":
        assert torch.equal(run(cls, tiny, plan_of((16, 16, 8)), shape=A.TINY_SHAPE, steps=4, guidance_rescale=0.7),
                           run(cls, tiny, None, shape=A.TINY_SHAPE, steps=4, guidance_rescale=0.7))


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED = 384, 128, 2, 42


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def long_job(ld, **kw):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    seed_everything(E2E_SEED)
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = ld.generate_batch_long(make_batch_for_text_to_audio("rain on a tin roof"), E2E_T, hop=E2E_HOP, ddim_steps=E2E_STEPS,
                                  unconditional_guidance_scale=A.GS, **kw)
    return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), float(torch.rand(1))


def test_generate_batch_long_end_to_end(ld):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything, text_to_audio_long
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, E2E_HOP)
    assert (plan.W, plan.starts, mel_plan.starts, mel_plan.Tw) == (2, (0, 128), (0, 512), 1024)
    wave, latent, mel, rand_after = long_job(ld)
    C, F_ = ld.channels, ld.latent_f_size
    hop_length = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert tuple(latent.shape) == (1, C, E2E_T, F_) and tuple(mel.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.shape == (1, 1, E2E_T * 4 * hop_length) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert ld.latent_t_size == 256
    # the host generator after the job (generate_batch_long's docstring)
    assert rand_after == Wd.expected_rand_after_long(E2E_SEED, 1, (C, 256, F_), (C, E2E_T, F_), E2E_STEPS)

    # the latent: the composition loop — the job's draws by hand, DDIMSampler.decode over the windowed model
    batch = make_batch_for_text_to_audio("rain on a tin roof")
    seed_everything(E2E_SEED)
    torch.randn((1, C, 256, F_))
    cond = ld.get_learned_conditioning_dict(batch)
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    ref = Wd.ddim_loop(ld, plan, torch.randn((1, C, E2E_T, F_)), cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"generate_batch_long latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "long-form latent") <= latent_tol(E2E_STEPS)

    # the mel: an fp64 merge of decode_first_stage on the sliced windows of the job's own latent
    mel_ref = Wd.merge_fp64(ld.decode_first_stage(Wd.gather_ref(latent, plan)), mel_plan)[0]
    e = A.rel_rms(mel, mel_ref)
    print(f"generate_batch_long mel vs the fp64 merge of the windows' decodes: rel rms {e:.2e}  bar {mel_tol(E2E_STEPS):.1e}")
    assert log_err(e, mel_tol(E2E_STEPS), "long-form mel") <= mel_tol(E2E_STEPS)

    # a second job of the same geometry replays the cached step graph and gives the first job's result under the same seed
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and ent["win"].plan.starts == plan.starts
    wave2, latent2, _, rand2 = long_job(ld)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    assert torch.equal(latent2, latent) and np.array_equal(wave2, wave) and rand2 == rand_after

    # the entry point: 15 s with 5 s of overlap is this very job
    ld.conditional_dry_run_finished = False
    wave3 = text_to_audio_long(ld, "rain on a tin roof", duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS,
                               guidance_scale=A.GS)
    assert np.array_equal(wave3, wave) and ld.latent_t_size == 256
    unet.drop_step_caches()


def test_generate_batch_long_with_the_other_samplers(ld):
    """PLMS and DPM-Solver++(2M) run the long job too, consume the generator as documented, and differ from DDIM at eta 1."""
    ddim = long_job(ld)
    C, F_ = ld.channels, ld.latent_f_size
    for name, kw in (("plms", dict(use_plms=True, ddim_eta=0.0)), ("dpmpp_2m", dict(sampler="dpmpp_2m", ddim_eta=0.0))):
        wave, latent, _, rand_after = long_job(ld, **kw)
        assert np.isfinite(wave).all() and bool(torch.isfinite(latent).all())
        assert rand_after == Wd.expected_rand_after_long(E2E_SEED, 1, (C, 256, F_), (C, E2E_T, F_), E2E_STEPS, sampler=name)
        assert A.rel_rms(latent, ddim[1]) > 1e-3
    ld.model.diffusion_model.drop_step_caches()
