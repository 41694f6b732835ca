"""Host side of audio-to-audio generation (no GPU): ddim.sdedit_plan against an fp64 restatement, what it refuses, the new entry
point's export and its argument validation (which happens before any launch), `t_start` next to `timesteps` in the three samplers,
the surface of generate_batch_from_audio / audio_to_audio, and the host-generator contract helper the GPU test compares against."""
import inspect
import types

import numpy as np
import pytest
import torch

import audio2audio as A


# ---- sdedit_plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength,steps", A.PLAN_CASES)
def test_sdedit_plan_matches_the_fp64_restatement(strength, steps):
    from audioldm2_amd.ddim import make_ddim_timesteps, sdedit_plan
    t_enc, t, sa, so = sdedit_plan(strength, steps, A.alphas_cumprod_fp64(), A.NUM_TIMESTEPS)
    r_enc, r_t, r_sa, r_so = A.plan_fp64(strength, steps)
    assert t_enc == r_enc == int(strength * steps) and 1 <= t_enc <= steps
    assert t == r_t == int(make_ddim_timesteps("uniform", steps, A.NUM_TIMESTEPS, verbose=False)[t_enc - 1])
    u = (A.ulps_fp32(sa, r_sa), A.ulps_fp32(so, r_so))
    print(f"sdedit_plan({strength}, {steps}): t_enc {t_enc} timestep {t} sqrt_abar {sa!r} sqrt_1m_abar {so!r}  fp32 ulps {u}")
    assert max(u) <= 1.0
    assert abs(sa * sa + so * so - 1.0) < 1e-12
    # a torch fp32 table (what the model keeps) is taken as it is: the look-up happens at the same timestep
    got = sdedit_plan(strength, steps, torch.from_numpy(A.alphas_cumprod_fp64()).float(), A.NUM_TIMESTEPS)
    assert got[:2] == (t_enc, t) and abs(got[2] - sa) < 1e-7


def test_sdedit_plan_enters_at_the_level_the_first_step_expects():
    """The run executes indices t_enc-1 ... 0; DDIM's step at index i takes its input at abar = ddim_alphas[i]."""
    from audioldm2_amd.ddim import DDIMSampler, sdedit_plan
    ac = torch.from_numpy(A.alphas_cumprod_fp64()).float()
    s = DDIMSampler(types.SimpleNamespace(num_timesteps=A.NUM_TIMESTEPS, alphas_cumprod=ac))
    for strength, steps in A.PLAN_CASES:
        s.make_schedule(steps, ddim_eta=0.0, verbose=False)
        t_enc, t, sa, _ = sdedit_plan(strength, steps, ac, A.NUM_TIMESTEPS)
        assert int(s.ddim_timesteps[t_enc - 1]) == t
        assert abs(float(s.ddim_alphas[t_enc - 1]) - sa * sa) < 1e-6
    assert sdedit_plan(1.0, 200, ac, A.NUM_TIMESTEPS)[0] == 200          # strength 1 stays on the table: index 199


@pytest.mark.parametrize("strength,steps", A.PLAN_REFUSED)
def test_sdedit_plan_refuses_and_names_both_numbers(strength, steps):
    from audioldm2_amd.ddim import sdedit_plan
    with pytest.raises(ValueError) as e:
        sdedit_plan(strength, steps, A.alphas_cumprod_fp64(), A.NUM_TIMESTEPS)
    assert repr(strength) in str(e.value) and str(steps) in str(e.value)


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_abi_is_bumped():
    from audioldm2_amd import lib
    assert "aldm_posterior_qsample" in lib.EXPORTED_SYMBOLS
    assert lib.ABI_VERSION >= 16
    l = lib.load()
    assert hasattr(l, "aldm_posterior_qsample") and l.aldm_version() == lib.ABI_VERSION


def test_bad_arguments_are_refused_before_any_launch():
    """Null pointers, B0 <= 0, n_gen <= 0, hw <= 0 and a refused C: a negative value and a message; no GPU is touched."""
    from audioldm2_amd import lib
    l = lib.load()
    P = 4096   # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused first
    good = dict(moments=P, n_post=P, n_enc=P, coef=P, z=P, x_t=P, B0=2, n_gen=1, C=8, hw=64)

    def call(**over):
        a = dict(good, **over)
        return l.aldm_posterior_qsample(a["moments"], a["n_post"], a["n_enc"], a["coef"], a["z"], a["x_t"], a["B0"], a["n_gen"],
                                        a["C"], a["hw"], None)
    cases = [(dict([(k, None)]), "null pointer") for k in ("moments", "n_post", "n_enc", "coef", "z", "x_t")]
    cases += [(dict(B0=0), "B0=0"), (dict(B0=-1), "B0=-1"), (dict(n_gen=0), "n_gen=0"), (dict(n_gen=-3), "n_gen=-3"),
              (dict(hw=0), "hw=0"), (dict(hw=-5), "hw=-5"), (dict(C=0), "C=0"), (dict(C=6), "C=6"), (dict(C=-8), "C=-8"),
              (dict(moments=P + 4), "16-byte aligned")]
    for over, msg in cases:
        rc = call(**over)
        err = l.aldm_last_error().decode()
        assert rc < 0 and "aldm_posterior_qsample" in err and msg in err, (over, rc, err)


def test_wrapper_refuses_wrong_shapes_and_host_tensors():
    """The shape checks come first (no tensor is touched), then the device / dtype / layout check."""
    from audioldm2_amd import ops
    m, npost, nenc, coef = torch.zeros(2, 4, 4, 16), torch.zeros(2, 8, 4, 4), torch.zeros(4, 8, 4, 4), torch.zeros(3)
    for bad_m in (torch.zeros(2, 4, 4, 8), torch.zeros(3, 4, 4, 16), torch.zeros(2, 4, 5, 16), torch.zeros(2, 16, 16)):
        with pytest.raises(RuntimeError, match=r"moments_cl must be \[B0, h, w, 2C\]"):
            ops.posterior_qsample(bad_m, npost, nenc, coef)
    for bad_e in (torch.zeros(3, 8, 4, 4), torch.zeros(0, 8, 4, 4), torch.zeros(4, 8, 4, 5), torch.zeros(4, 16, 4, 4)):
        with pytest.raises(RuntimeError, match=r"n_enc must be \[B0\*n_gen, C, h, w\]"):
            ops.posterior_qsample(m, npost, bad_e, coef)
    with pytest.raises(RuntimeError, match="expected 3 floats, got 2"):
        ops.posterior_qsample(m, npost, nenc, torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"posterior_qsample.z: expected \(2, 8, 4, 4\)"):
        ops.posterior_qsample(m, npost, nenc, coef, z=torch.zeros(2, 8, 4, 5))
    with pytest.raises(RuntimeError, match=r"posterior_qsample.x_t: expected \(4, 8, 4, 4\)"):
        ops.posterior_qsample(m, npost, nenc, coef, x_t=torch.zeros(2, 8, 4, 4))
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.posterior_qsample(m, npost, nenc, coef)


# ---- t_start ----------------------------------------------------------------------------------------------------------------------
def samplers():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return ((DDIMSampler, "ddim_sampling"), (PLMSSampler, "plms_sampling"), (DPMSolverSampler, "dpm_sampling"))


def test_t_start_together_with_timesteps_raises_in_all_three_samplers():
    """... in `sample` and in the loop, before anything is drawn or launched.  DDIMSampler names `t_start` as a parameter of both;
    PLMSSampler keeps the reference class's signatures (and DPMSolverSampler carries them), so their `sample` reads the keyword from
    **kwargs into `self.t_start`, which the loop reads — the way they take `guidance_rescale`."""
    model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
    for cls, loop in samplers():
        s = cls(model)
        state = torch.get_rng_state()
        with pytest.raises(ValueError, match="t_start=2 and timesteps=3"):
            s.sample(4, 1, (8, 8, 8), None, verbose=False, t_start=2, timesteps=3)
        s.make_schedule(4, ddim_eta=0.0, verbose=False)
        with pytest.raises(ValueError, match="t_start=2 and timesteps=3"):
            if loop == "ddim_sampling":
                s.ddim_sampling(None, (1, 8, 8, 8), t_start=2, timesteps=3)
            else:
                s.t_start = 2
                getattr(s, loop)(None, (1, 8, 8, 8), timesteps=3)
        for bad in (0, 5, -1, 2.0, True):
            with pytest.raises(ValueError, match="t_start must be an integer in"):
                s.sample(4, 1, (8, 8, 8), None, verbose=False, t_start=bad)
        assert torch.equal(torch.get_rng_state(), state)


def test_t_start_is_a_parameter_of_ddim_and_sampler_state_elsewhere():
    for cls, loop in samplers():
        if loop == "ddim_sampling":
            for name in ("sample", loop):
                p = inspect.signature(getattr(cls, name)).parameters["t_start"]
                assert p.default is None
        else:
            model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
            s = cls(model)
            assert s.t_start is None
            seen = []
            setattr(s, loop, lambda *a, **k: seen.append(s.t_start) or (None, None))
            s.sample(4, 1, (8, 8, 8), None, verbose=False, t_start=3)
            s.sample(4, 1, (8, 8, 8), None, verbose=False)              # a later job without the keyword runs the whole schedule
            assert seen == [3, None]


def test_sample_log_forwards_t_start_to_all_three_samplers(monkeypatch):
    from audioldm2_amd import dpm_solver, plms
    from audioldm2_amd import pipeline as P
    seen = []

    def fake(name):
        class S:
            def __init__(self, model, **kw):
                pass

            def sample(self, S, batch_size, shape, *a, **kw):
                seen.append((name, kw.get("t_start", "absent"), tuple(shape)))
                return torch.zeros(1), None
        return S
    monkeypatch.setattr(P, "DDIMSampler", fake("ddim"))
    monkeypatch.setattr(plms, "PLMSSampler", fake("plms"))
    monkeypatch.setattr(dpm_solver, "DPMSolverSampler", fake("dpmpp"))
    ld = types.SimpleNamespace(channels=8, latent_t_size=256, latent_f_size=16, device="cpu")
    x = torch.zeros(2, 8, 24, 16)
    for how in (dict(), dict(use_plms=True), dict(sampler="dpmpp_2m")):
        P.LatentDiffusion.sample_log(ld, None, 2, ddim=True, ddim_steps=4, x_T=x, t_start=2, **how)
        P.LatentDiffusion.sample_log(ld, None, 2, ddim=True, ddim_steps=4, **how)
    # the start latent sets the shape of a shortened run
    assert seen == [(n, v, sh) for n in ("ddim", "plms", "dpmpp") for v, sh in ((2, (8, 24, 16)), ("absent", (8, 256, 16)))]
    with pytest.raises(ValueError, match="t_start needs ddim_steps"):
        P.LatentDiffusion.sample_log(ld, None, 2, ddim=False, ddim_steps=None, x_T=x, t_start=2)
    with pytest.raises(ValueError, match="t_start needs x_T"):
        P.LatentDiffusion.sample_log(ld, None, 2, ddim=True, ddim_steps=4, t_start=2)


# ---- the pipeline's surface -------------------------------------------------------------------------------------------------------
def test_signatures():
    from audioldm2_amd import pipeline as P
    sig = inspect.signature(P.LatentDiffusion.generate_batch_from_audio)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:-1]] == [
        ("batch", inspect.Parameter.empty), ("strength", inspect.Parameter.empty), ("ddim_steps", 200), ("ddim_eta", 1.0),
        ("n_gen", 1), ("unconditional_guidance_scale", 1.0), ("use_plms", False)]
    assert list(sig.parameters.values())[-1].kind == inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(P.audio_to_audio)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("latent_diffusion", inspect.Parameter.empty), ("text", inspect.Parameter.empty),
        ("original_audio_file_path", inspect.Parameter.empty), ("strength", 0.5), ("transcription", ""), ("seed", 42),
        ("ddim_steps", 200), ("duration", 10), ("batchsize", 1), ("guidance_scale", 3.5), ("n_candidate_gen_per_text", 3),
        ("latent_t_per_second", 25.6), ("negative_prompt", None), ("guidance_rescale", 0.0), ("sampler", None)]


def test_generate_batch_from_audio_refuses_before_any_work():
    from audioldm2_amd import pipeline as P
    stub = types.SimpleNamespace(alphas_cumprod=torch.from_numpy(A.alphas_cumprod_fp64()).float(), num_timesteps=1000)
    gen = P.LatentDiffusion.generate_batch_from_audio
    with pytest.raises(ValueError, match="shard"):
        gen(stub, {}, 0.5, ddim_steps=4, shard=(0, 2))
    with pytest.raises(ValueError, match="needs ddim_steps"):
        gen(stub, {}, 0.5, ddim_steps=None)
    with pytest.raises(ValueError, match="unknown sampler"):
        gen(stub, {}, 0.5, ddim_steps=4, sampler="heun")
    with pytest.raises(ValueError, match="negative_prompt needs unconditional_guidance_scale"):
        gen(stub, {"text": ["a"]}, 0.5, ddim_steps=4, negative_prompt="Low quality.")
    with pytest.raises(ValueError, match="guidance_rescale"):
        gen(stub, {}, 0.5, ddim_steps=4, guidance_rescale=2.0)
    with pytest.raises(ValueError, match=r"strength=0.1 of ddim_steps=4"):
        gen(stub, {}, 0.1, ddim_steps=4)


def test_audio_to_audio_refuses_before_any_work():
    from audioldm2_amd import pipeline as P
    ac = torch.from_numpy(A.alphas_cumprod_fp64()).float()
    enc = lambda n: types.SimpleNamespace(encoder=types.SimpleNamespace(num_resolutions=n))
    ld16 = types.SimpleNamespace(alphas_cumprod=ac, num_timesteps=1000, sampling_rate=16000, latent_f_size=16, first_stage_model=enc(3))
    ld48 = types.SimpleNamespace(alphas_cumprod=ac, num_timesteps=1000, sampling_rate=48000, latent_f_size=32, first_stage_model=enc(4))
    src = np.zeros(16000, dtype=np.float32)
    with pytest.raises(ValueError, match="unknown sampler"):
        P.audio_to_audio(ld16, "a dog", src, sampler="heun")
    with pytest.raises(ValueError, match=r"strength=0.1 of ddim_steps=4"):
        P.audio_to_audio(ld16, "a dog", src, strength=0.1, ddim_steps=4)
    with pytest.raises(ValueError, match="16 kHz / 64-bin"):
        P.audio_to_audio(ld48, "a dog", src, ddim_steps=4)
    with pytest.raises(ValueError, match="latent_t_size must be a positive multiple of 8"):
        P.audio_to_audio(ld16, "a dog", src, ddim_steps=4, duration=3)


# ---- the host-generator contract ------------------------------------------------------------------------------------------------
def test_generate_batch_from_audio_leaves_the_generator_where_the_hand_made_draws_do():
    """Draws 1 to 5 of the contract by hand, here, against generate_batch_from_audio over fakes (encoder, kernel wrapper, decoder,
    vocoder; a conditioner that draws rand(5) per pass; a sample_log that draws DDIM's one randn of the batch per step) and against
    tests/audio2audio.py::expected_rand_after, the helper the GPU test uses.  Also: the launch's operands and what reaches sample_log."""
    from audioldm2_amd import ops
    from audioldm2_amd import pipeline as P
    B0, n_gen, C, h, w = 2, 3, 8, 8, 16
    calls = {}

    class LD:
        generate_batch_from_audio = P.LatentDiffusion.generate_batch_from_audio
        check_latent_t = staticmethod(P.LatentDiffusion.check_latent_t)
        _cfg_dropout_draw = P.LatentDiffusion._cfg_dropout_draw
        first_stage_key, device, scale_factor, num_timesteps = "fbank", "cpu", 0.75, 1000
        alphas_cumprod = torch.from_numpy(A.alphas_cumprod_fp64()).float()
        cond_stage_model_metadata = {"c": {"model_idx": 0}}
        conditional_dry_run_finished = False
        clap = types.SimpleNamespace(cos_similarity=lambda wave, text: torch.arange(len(text)).float())

        def __init__(self):
            self.first_stage_model = types.SimpleNamespace(
                encoder=types.SimpleNamespace(num_resolutions=3),
                encode_moments_cl=lambda x: torch.zeros(x.shape[0], x.shape[2] // 4, x.shape[3] // 4, 2 * C))
            self.cond_stage_models = [types.SimpleNamespace(get_unconditional_condition=lambda b: torch.zeros(b, 2))]
            self.texts = []

        def _check_candidates(self, n_gen, text=None):
            pass

        def get_learned_conditioning_dict(self, batch):
            self.texts.append(list(batch["text"]))
            torch.rand(5)                                  # a conditioner that consumes the host generator
            return {"c": torch.zeros(len(batch["text"]), 2)}

        def sample_log(self, **kw):
            calls["sample_log"] = kw
            for _ in range(kw["t_start"]):                 # DDIM: one draw of the batch per executed step
                torch.randn(tuple(kw["x_T"].shape))
            return kw["x_T"], None

        def decode_first_stage_cl(self, z):
            return torch.zeros(z.shape[0], 32, 64, 1)

        def mel_spectrogram_to_waveform(self, mel, savepath="", bs=None, name=None, save=False):
            return np.zeros((mel.shape[0], 1, 8), dtype=np.float32)

    def fake_kernel(moments, n_post, n_enc, coef):
        calls["kernel"] = (moments, n_post, n_enc, coef)
        return torch.zeros_like(n_post), n_enc.clone()
    orig = ops.posterior_qsample
    ops.posterior_qsample = fake_kernel
    try:
        ld = LD()
        batch = {"text": ["a", "b"], "log_mel_spec": torch.zeros(B0, 4 * h, 4 * w), "fname": ["f"] * B0,
                 "phoneme_idx": torch.zeros(B0, 310, dtype=torch.long)}
        seen = []
        for second, neg in ((False, None), (True, None), (True, "Low quality.")):
            torch.manual_seed(42)
            out = ld.generate_batch_from_audio(batch, 0.5, ddim_steps=4, ddim_eta=0.0, n_gen=n_gen, unconditional_guidance_scale=3.5,
                                               **({} if neg is None else {"negative_prompt": neg}))
            after = float(torch.rand(1))
            assert ld.conditional_dry_run_finished
            torch.manual_seed(42)
            n_post = torch.randn(B0, C, h, w)                 # 1. the posterior noise
            if second:
                torch.rand(1)                                 # 2. R1b: every call but an object's first
            torch.rand(5)                                     # 3. the conditioners' draws ...
            if neg is not None:
                torch.rand(5)                                 #    ... twice with a negative prompt
            n_enc = torch.randn(B0 * n_gen, C, h, w)          # 4. the forward-diffusion noise
            for _ in range(2):                                # 5. the sampler's per-step draws, t_enc = 2 steps
                torch.randn(B0 * n_gen, C, h, w)
            want = float(torch.rand(1))
            assert after == want
            assert want == A.expected_rand_after(42, B0, n_gen, (C, h, w), 2, second_call=second, cond_draws=lambda: torch.rand(5),
                                                 n_neg=0 if neg is None else 1)
            seen.append(want)
            m, got_post, got_enc, coef = calls["kernel"]
            assert m.shape == (B0, h, w, 2 * C) and torch.equal(got_post, n_post) and torch.equal(got_enc, n_enc)
            _, _, sa, so = A.plan_fp64(0.5, 4)
            assert coef.dtype == torch.float32 and np.allclose(coef.numpy(), [0.75, sa, so], rtol=1e-6, atol=0)
            kw = calls["sample_log"]
            assert kw["t_start"] == 2 and kw["ddim_steps"] == 4 and kw["batch_size"] == B0 * n_gen and kw["ddim"] is True
            assert kw["x_T"].shape == (B0 * n_gen, C, h, w) and kw["eta"] == 0.0 and "sampler" not in kw
            assert kw["unconditional_conditioning"]["c"].shape == (B0 * n_gen, 2) and kw["cond"]["c"].shape == (B0 * n_gen, 2)
            assert out.shape == (B0, 1, 8)
        assert len(set(seen)) == 3                            # every draw of the list moves the position
        assert ld.texts[-2:] == [["a", "b"], ["Low quality."] * 2]
        # the helper's other samplers: PLMS draws once more than DDIM, DPM-Solver++(2M) nothing
        kw = dict(second_call=True, cond_draws=lambda: torch.rand(5), n_neg=1)
        assert A.expected_rand_after(42, B0, n_gen, (C, h, w), 2, sampler="plms", **kw) == \
            A.expected_rand_after(42, B0, n_gen, (C, h, w), 3, **kw) != seen[2]
        assert A.expected_rand_after(42, B0, n_gen, (C, h, w), 2, sampler="dpmpp_2m", **kw) == \
            A.expected_rand_after(42, B0, n_gen, (C, h, w), 0, **kw) != seen[2]
    finally:
        ops.posterior_qsample = orig
