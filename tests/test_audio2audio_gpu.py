"""Audio-to-audio generation on the GPU (ops.posterior_qsample, `t_start` of the three samplers,
LatentDiffusion.generate_batch_from_audio, pipeline.audio_to_audio):

 1. aldm_posterior_qsample against fp64 of the same fp32 inputs over audio2audio.KERNEL_SHAPES (ragged tails, hw around one wave,
    the 16 kHz and the 48 kHz latent shapes), two (sqrt(abar), sqrt(1 - abar)) pairs; NaN propagation; guard floats; tiling;
 2. `t_start=k` of DDIM / PLMS / DPM-Solver++(2M) on the tiny UNet against the sampler's own step-by-step loop over indices k-1 ... 0;
 3. end to end: the latent handed to the decoder against the composition of the existing pieces (encode_first_stage().sample() *
    scale, one randn, DDIMSampler.stochastic_encode, DDIMSampler.decode) under the same seed, the host generator's position after
    the job, the cached step graph, the two other samplers;
 4. the audio_to_audio entry point.

Bars.  (1): audio2audio.KERNEL_BAR, 5x the maximum measured on an MI355X, at most 1e-6 (that module's docstring).  The error of an
element is |got - ref| over the sum of the magnitudes of its terms.  (2): audio2audio.tstart_bar(k).  (3): tolerances.latent_tol(4).

Measured on an MI355X: profiles/r14_audio2audio_errors.txt.
"""
import json
import os

import numpy as np
import pytest
import torch

import audio2audio as A
from oracle import cases, weights
from tolerances import latent_tol, log_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- 1. kernel ------------------------------------------------------------------------------------------------------------------
def run_kernel(moments, n_post, n_enc, a, b, z=None, x_t=None):
    from audioldm2_amd import ops
    coef = torch.tensor([A.KERNEL_SCALE, a, b], dtype=torch.float32).cuda()
    return ops.posterior_qsample(moments.cuda(), n_post.cuda(), n_enc.cuda(), coef, z=z, x_t=x_t)


def kernel_errors(z, x_t, ref):
    rz, rx, dz, dx = ref
    ez = float(((z.double().cpu() - rz).abs() / dz).max())
    ex = float(((x_t.double().cpu() - rx).abs() / dx).max())
    return ez, ex


@pytest.mark.parametrize("shape", A.KERNEL_SHAPES, ids=["x".join(map(str, s)) for s in A.KERNEL_SHAPES])
def test_kernel_matches_fp64(shape):
    moments, n_post, n_enc = A.kernel_inputs(shape, seed=sum(shape))
    lv = moments[..., shape[2]:]
    assert bool(torch.isinf(lv).any()) and float(lv[torch.isfinite(lv)].max()) == 25.0 and float(lv[torch.isfinite(lv)].min()) == -40.0
    for which, (a, b) in zip(("index 0", "last index"), A.kernel_coef_pairs()):
        z, x_t = run_kernel(moments, n_post, n_enc, a, b)
        assert z.shape == n_post.shape and x_t.shape == n_enc.shape
        ez, ex = kernel_errors(z, x_t, A.kernel_fp64(moments, n_post, n_enc, A.KERNEL_SCALE, a, b))
        print(f"posterior_qsample {shape} {which} (a={a:.6f}, b={b:.6f}): z {ez:.3e}  x_t {ex:.3e}  bar {A.KERNEL_BAR:.1e}")
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(x_t).all())
        assert log_err(ez, A.KERNEL_BAR, f"posterior_qsample z {shape} {which}") <= A.KERNEL_BAR
        assert log_err(ex, A.KERNEL_BAR, f"posterior_qsample x_t {shape} {which}") <= A.KERNEL_BAR


def test_kernel_propagates_nan_like_torch_clamp():
    """A NaN logvar gives NaN in z at exactly its position and in x_t there in every candidate row; everything else is finite."""
    shape = (3, 2, 8, 5, 3)
    B0, n_gen, C, h, w = shape
    planted = [(0, 0, 0), (1, 5, 14), (2, 7, 8)]          # (b, c, pixel)
    moments, n_post, n_enc = A.kernel_inputs(shape, seed=3, nan_at=planted)
    a, b = A.kernel_coef_pairs()[1]
    z, x_t = run_kernel(moments, n_post, n_enc, a, b)
    want = torch.zeros(B0, C, h * w, dtype=torch.bool)
    for (bb, c, p) in planted:
        want[bb, c, p] = True
    want = want.view(B0, C, h, w)
    assert torch.equal(torch.isnan(z).cpu(), want) and torch.equal(torch.isnan(x_t).cpu(), torch.cat([want] * n_gen))
    assert bool(torch.isfinite(z.cpu()[~want]).all()) and bool(torch.isfinite(x_t.cpu()[~torch.cat([want] * n_gen)]).all())
    # torch.clamp agrees on what a NaN, +inf and -inf logvar become
    lv = torch.tensor([float("nan"), float("inf"), float("-inf")])
    assert torch.isnan(torch.clamp(lv, -30.0, 20.0)[0]) and torch.clamp(lv, -30.0, 20.0)[1:].tolist() == [20.0, -30.0]


@pytest.mark.parametrize("shape", [(3, 2, 8, 5, 3), (1, 2, 8, 13, 5)], ids=["3x2x8x5x3", "1x2x8x13x5"])
def test_kernel_stays_inside_its_outputs(shape):
    B0, n_gen, C, h, w = shape
    moments, n_post, n_enc = A.kernel_inputs(shape, seed=4)
    a, b = A.kernel_coef_pairs()[0]
    (z, zbuf), (x_t, xbuf) = A.guarded((B0, C, h, w)), A.guarded((B0 * n_gen, C, h, w))
    z2, x2 = run_kernel(moments, n_post, n_enc, a, b, z=z, x_t=x_t)
    assert z2 is z and x2 is x_t
    assert A.guards_intact(zbuf) and A.guards_intact(xbuf)
    assert not bool((z == -777.0).any()) and not bool((x_t == -777.0).any())
    ez, ex = kernel_errors(z, x_t, A.kernel_fp64(moments, n_post, n_enc, A.KERNEL_SCALE, a, b))
    assert ez <= A.KERNEL_BAR and ex <= A.KERNEL_BAR


def test_wrapper_refuses_outputs_that_alias_an_operand():
    from audioldm2_amd import ops
    moments, n_post, n_enc = (t.cuda() for t in A.kernel_inputs((2, 1, 8, 5, 3), seed=6))
    coef = torch.tensor([A.KERNEL_SCALE, 0.6, 0.8]).cuda()
    keep = (n_post.clone(), n_enc.clone())
    with pytest.raises(RuntimeError, match="z overlaps n_post"):
        ops.posterior_qsample(moments, n_post, n_enc, coef, z=n_post)
    with pytest.raises(RuntimeError, match="x_t overlaps n_enc"):
        ops.posterior_qsample(moments, n_post, n_enc, coef, x_t=n_enc)
    buf = torch.empty(2 * n_post.numel() - 8, device="cuda")
    with pytest.raises(RuntimeError, match="x_t overlaps z"):
        ops.posterior_qsample(moments, n_post, n_enc, coef, z=buf[:n_post.numel()].view(n_post.shape),
                              x_t=buf[-n_enc.numel():].view(n_enc.shape))
    assert torch.equal(n_post, keep[0]) and torch.equal(n_enc, keep[1])      # refused before the launch


def test_kernel_tiles_candidate_major():
    """n_gen = 3: x_t[r] - b*n_enc[r] is a*z[r % B0] — the same for the three rows that share a source."""
    shape = (2, 3, 16, 7, 9)
    B0, n_gen = shape[0], shape[1]
    moments, n_post, n_enc = A.kernel_inputs(shape, seed=5)
    a, b = A.kernel_coef_pairs()[1]
    z, x_t = run_kernel(moments, n_post, n_enc, a, b)
    _, _, _, dx = A.kernel_fp64(moments, n_post, n_enc, A.KERNEL_SCALE, a, b)
    rest = (x_t.double().cpu() - b * n_enc.double()).view(n_gen, B0, *shape[2:])
    dx = dx.view(n_gen, B0, *shape[2:])
    worst = 0.0
    for g in range(1, n_gen):
        worst = max(worst, float(((rest[g] - rest[0]).abs() / torch.maximum(dx[g], dx[0])).max()))
    az = float(((rest[0] - a * z.double().cpu()).abs() / dx[0]).max())
    print(f"posterior_qsample tiling {shape}: rows of one source differ by {worst:.3e}, from a*z by {az:.3e}  bar {A.KERNEL_BAR:.1e}")
    assert log_err(worst, A.KERNEL_BAR, "posterior_qsample tiling") <= A.KERNEL_BAR and az <= A.KERNEL_BAR
    assert float((z[0] - z[1]).abs().max()) > 1e-2       # ... and the sources differ


# ---- 2. t_start on the tiny UNet ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    m = A.TinyModel()
    cond, uncond = A.tiny_conditioning()
    return m, cond, uncond


def x_start(seed=3):
    return torch.randn(A.TINY_SHAPE, generator=torch.Generator().manual_seed(seed))


S_TINY = 6


def sample_kw(uncond, **kw):
    return dict(verbose=False, unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond, **kw)


@pytest.mark.parametrize("k", [1, 3, 6])
def test_ddim_t_start_equals_decode(tiny, k):
    from audioldm2_amd.ddim import DDIMSampler
    m, cond, uncond = tiny
    s = DDIMSampler(m)
    out, _ = s.sample(S_TINY, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), t_start=k, eta=0.0, **sample_kw(uncond))
    ref = s.decode(x_start().cuda(), cond, k, unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond)
    e, bar = A.rel_rms(out, ref), A.tstart_bar(k)
    print(f"ddim t_start={k} of {len(s.ddim_timesteps)} vs decode: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"ddim t_start={k}") <= bar
    assert A.rel_rms(out, x_start().cuda()) > 1e-3


def test_ddim_t_start_at_eta_one_draws_in_decodes_order(tiny):
    from audioldm2_amd.ddim import DDIMSampler
    m, cond, uncond = tiny
    s = DDIMSampler(m)
    torch.manual_seed(17)
    out, _ = s.sample(S_TINY, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), t_start=3, eta=1.0, **sample_kw(uncond))
    after = float(torch.rand(1))
    torch.manual_seed(17)
    ref = s.decode(x_start().cuda(), cond, 3, unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond)
    assert float(torch.rand(1)) == after
    e, bar = A.rel_rms(out, ref), A.tstart_bar(3)
    print(f"ddim t_start=3 eta=1 vs decode: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "ddim t_start=3 eta=1") <= bar
    torch.manual_seed(18)
    other, _ = s.sample(S_TINY, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), t_start=3, eta=1.0, **sample_kw(uncond))
    assert A.rel_rms(other, ref) > 1e-2                  # the noise matters at eta 1


@pytest.mark.parametrize("k", [1, 3, 6])
def test_plms_t_start_equals_the_eager_loop(tiny, k):
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    s = PLMSSampler(m)
    out, _ = s.sample(S_TINY, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), t_start=k, **sample_kw(uncond))
    ref = A.plms_eager_loop(s, x_start().cuda(), cond, uncond, k)
    e, bar = A.rel_rms(out, ref), A.tstart_bar(k)
    print(f"plms t_start={k} vs the eager loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"plms t_start={k}") <= bar
    assert A.rel_rms(out, x_start().cuda()) > 1e-3


@pytest.mark.parametrize("k", [1, 3, 6])
def test_dpmpp_t_start_equals_the_fp64_loop(tiny, k):
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    m, cond, uncond = tiny
    s = DPMSolverSampler(m)
    out, _ = s.sample(S_TINY, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), t_start=k, **sample_kw(uncond))
    b = A.TINY_SHAPE[0]
    model_cfg = lambda xx, t: m.apply_model_cfg(xx, torch.full((2 * b,), t, device="cuda"), cond, uncond)
    ref = A.dpmpp_fp64_loop(model_cfg, m.alphas_cumprod, s.ddim_timesteps[:k], x_start())
    e, bar = A.rel_rms(out, ref), A.tstart_bar(k)
    print(f"dpmpp t_start={k} vs the fp64 loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"dpmpp t_start={k}") <= bar
    assert A.rel_rms(out, x_start().cuda()) > 1e-3


def test_t_start_none_is_the_call_without_the_keyword(tiny):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    m, cond, uncond = tiny
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        outs = []
        for kw in (dict(), dict(t_start=None)):
            torch.manual_seed(5)
            o, _ = cls(m).sample(4, A.TINY_SHAPE[0], A.TINY_SHAPE[1:], cond, x_T=x_start(), eta=0.0, **sample_kw(uncond, **kw))
            outs.append((o, float(torch.rand(1))))
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], cls.__name__


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
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


STEPS, STRENGTH, T_ENC, LATENT = 4, 0.5, 2, (8, 256, 16)


def job(ld, second_call=False, strength=STRENGTH, **kw):
    """One generate_batch_from_audio job from seed 42; records the latent handed to the decoder and the next host draw."""
    from audioldm2_amd.pipeline import seed_everything
    rec = {}
    orig = ld.decode_first_stage_cl

    def hook(z):
        rec["latent"] = z.clone()
        return orig(z)
    ld.decode_first_stage_cl = hook
    try:
        seed_everything(cases.E2E_SEED)
        ld.conditional_dry_run_finished = second_call
        args = dict(ddim_steps=STEPS, ddim_eta=0.0, n_gen=1, unconditional_guidance_scale=A.GS)
        args.update(kw)
        rec["wave"] = ld.generate_batch_from_audio(cases.e2e_masked_batch(2), strength, **args)
        rec["rand_after"] = float(torch.rand(1))
    finally:
        ld.decode_first_stage_cl = orig
    return rec


def composition(ld, eta, second_call=False):
    """The same job from the existing pieces: encode_first_stage(x).sample() * scale, (the R1b draw), the conditioners, one randn,
    DDIMSampler.stochastic_encode to index t_enc-1, DDIMSampler.decode over t_enc steps."""
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.pipeline import seed_everything
    batch = cases.e2e_masked_batch(2)
    seed_everything(cases.E2E_SEED)
    x = batch["log_mel_spec"].unsqueeze(1).float().contiguous().cuda()
    z = ld.get_first_stage_encoding(ld.encode_first_stage(x))
    if second_call:
        torch.rand(1)
    cond = ld.get_learned_conditioning_dict(batch)
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(2) for k, m in ld.cond_stage_model_metadata.items()}
    noise = torch.randn(z.shape)
    s = DDIMSampler(ld)
    s.make_schedule(STEPS, ddim_eta=eta, verbose=False)
    x_t = s.stochastic_encode(z, torch.full((2,), T_ENC - 1, dtype=torch.long), noise=noise)
    out = s.decode(x_t, cond, T_ENC, unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond)
    return out, float(torch.rand(1))


@pytest.mark.parametrize("eta,second_call", [(0.0, False), (1.0, False), (1.0, True)], ids=["eta0", "eta1", "eta1-second-call"])
def test_e2e_latent_equals_the_composition_of_existing_pieces(ld, eta, second_call):
    from audioldm2_amd.ddim import sdedit_plan
    assert sdedit_plan(STRENGTH, STEPS, ld.alphas_cumprod, ld.num_timesteps)[0] == T_ENC
    ref, ref_rand = composition(ld, eta, second_call)
    rec = job(ld, second_call, ddim_eta=eta)
    assert rec["wave"].shape == (2, 1, 163872) and rec["wave"].dtype == np.float32 and np.isfinite(rec["wave"]).all()
    assert tuple(rec["latent"].shape) == (2,) + LATENT
    e = A.rel_rms(rec["latent"], ref)
    want = A.expected_rand_after(cases.E2E_SEED, 2, 1, LATENT, T_ENC, second_call=second_call)
    print(f"audio2audio e2e eta={eta} second_call={second_call}: latent rel rms {e:.2e} (bar {latent_tol(4):.1e})  "
          f"rand after {rec['rand_after']!r} / composition {ref_rand!r} / contract {want!r}")
    assert log_err(e, latent_tol(4), f"audio2audio latent eta={eta}") < latent_tol(4)
    assert rec["rand_after"] == want == ref_rand
    assert ld.conditional_dry_run_finished


def test_e2e_second_job_reuses_the_cached_step_graph(ld):
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    a = job(ld)
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    b = job(ld)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    # job a ran its first step eagerly and captured at the second; job b replays both
    assert A.rel_rms(b["latent"], a["latent"]) < latent_tol(4) and a["rand_after"] == b["rand_after"]
    unet.drop_step_caches()


def test_e2e_the_other_samplers_run_from_the_same_start(ld):
    """strength 0.5 (t_enc = 2): PLMS differs from DDIM at eta 0; both steps of a 2-step 2M run are first order, i.e. DDIM's eta-0
    steps, so 2M agrees with DDIM there up to rounding.  strength 0.75 (t_enc = 3) puts a second-order step in the middle: there
    2M gives another latent than DDIM."""
    ddim = job(ld)
    dpm = job(ld, sampler="dpmpp_2m")
    plms = job(ld, use_plms=True)
    for name, rec in (("dpmpp_2m", dpm), ("plms", plms)):
        assert bool(torch.isfinite(rec["latent"]).all()) and np.isfinite(rec["wave"]).all()
        assert rec["rand_after"] == A.expected_rand_after(cases.E2E_SEED, 2, 1, LATENT, T_ENC, sampler=name)
    d_plms, d_dpm = A.rel_rms(plms["latent"], ddim["latent"]), A.rel_rms(dpm["latent"], ddim["latent"])
    ddim3, dpm3 = job(ld, strength=0.75), job(ld, strength=0.75, sampler="dpmpp_2m")
    assert bool(torch.isfinite(dpm3["latent"]).all()) and np.isfinite(dpm3["wave"]).all()
    assert dpm3["rand_after"] == A.expected_rand_after(cases.E2E_SEED, 2, 1, LATENT, 3, sampler="dpmpp_2m")
    assert ddim3["rand_after"] == A.expected_rand_after(cases.E2E_SEED, 2, 1, LATENT, 3)
    d_dpm3 = A.rel_rms(dpm3["latent"], ddim3["latent"])
    print(f"audio2audio e2e vs ddim eta 0, latent rel rms: plms (2 steps) {d_plms:.2e}  dpmpp_2m (2 steps, both first order) {d_dpm:.2e}  "
          f"dpmpp_2m (3 steps) {d_dpm3:.2e}")
    assert d_plms > 1e-4 and d_dpm3 > 1e-4          # three orders above the rounding-level agreement of the first-order run
    assert d_dpm < latent_tol(4)
    assert A.rel_rms(ddim3["latent"], ddim["latent"]) > 1e-2      # ... and the strength matters
    with pytest.raises(ValueError, match="shard"):
        job(ld, shard=(0, 1))
    with pytest.raises(ValueError, match="needs ddim_steps"):
        job(ld, ddim_steps=None)


# ---- 4. the entry point ---------------------------------------------------------------------------------------------------------
def source_clip():
    t = np.arange(3 * 16000) / 16000.0
    g = np.random.default_rng(0)
    return (np.sin(2 * np.pi * 440.0 * t) + 0.1 * g.standard_normal(t.shape)).astype(np.float32)


def test_audio_to_audio_entry_point(ld):
    from audioldm2_amd.pipeline import audio_to_audio
    kw = dict(seed=7, ddim_steps=4, duration=10, batchsize=1, n_candidate_gen_per_text=1)

    def run(**more):
        ld.conditional_dry_run_finished = False   # every call as an object's first (pipeline._cfg_dropout_draw)
        return audio_to_audio(ld, "a dog barking", source_clip(), **kw, **more)
    a, b, c = run(strength=0.5), run(strength=0.5), run(strength=1.0)
    assert a.shape == (1, 1, 163872) and a.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(c).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    state = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="strength=0.1 of ddim_steps=4"):
        run(strength=0.1)
    assert torch.cuda.memory_allocated() == state


def test_audio_to_audio_refuses_a_48k_model():
    """What the refusal reads of a model — sampling rate, latent_f_size, the encoder's depth — taken from the audioldm_48k config;
    the check runs before the front end, so no weights are built for it."""
    from audioldm2_amd.pipeline import audio_to_audio, default_audioldm_config
    import types
    p = default_audioldm_config("audioldm_48k")["model"]["params"]
    ddc = p["first_stage_config"]["params"]["ddconfig"]
    ld48 = types.SimpleNamespace(alphas_cumprod=torch.from_numpy(A.alphas_cumprod_fp64()).float(), num_timesteps=p["timesteps"],
                                 sampling_rate=p["sampling_rate"], latent_f_size=p["latent_f_size"],
                                 first_stage_model=types.SimpleNamespace(
                                     encoder=types.SimpleNamespace(num_resolutions=len(ddc["ch_mult"]))))
    with pytest.raises(ValueError, match="16 kHz / 64-bin"):
        audio_to_audio(ld48, "a dog barking", source_clip(), ddim_steps=4, n_candidate_gen_per_text=1)
