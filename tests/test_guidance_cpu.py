"""Host side of negative prompts and guidance rescale (no GPU): what is refused and where, the negative batch and its way through
generate_batch (conditioner pass order, tiling over n_gen, the cut of a 2-rank shard, the host generator), the keywords that
reach sample_log, the public signatures, and columns 5-7 of the samplers' coefficient tables.  The conditioners, sample_log, the
decoder and the vocoder are fakes: generate_batch itself is the code under test."""
import inspect
import types

import numpy as np
import pytest
import torch

from audioldm2_amd import pipeline as P


# ---- fakes ------------------------------------------------------------------------------------------------------------------------
class FakeConditioner:
    """One conditioner under cond_stage_key "all" that returns two keys: a tensor and a [context, mask] list, both encoding each
    row's text (its length) and row index."""

    def __init__(self):
        self.seen = []

    def __call__(self, batch):
        self.seen.append(batch)
        code = torch.tensor([[float(len(t)), float(i)] for i, t in enumerate(batch["text"])])
        return {"film": code, "ctx": [code[:, None, :].clone(), torch.ones(code.shape[0], 1)]}

    def get_unconditional_condition(self, batchsize):
        return torch.full((batchsize, 2), -1.0)


class FakeLD:
    generate_batch = P.LatentDiffusion.generate_batch
    generate_batch_masked = P.LatentDiffusion.generate_batch_masked
    sample_log_real = P.LatentDiffusion.sample_log
    get_learned_conditioning_dict = P.LatentDiffusion.get_learned_conditioning_dict
    check_latent_t = staticmethod(P.LatentDiffusion.check_latent_t)
    first_stage_key = "fbank"
    latent_t_size, latent_f_size, channels = 8, 16, 8

    def __init__(self):
        self.first_stage_model = types.SimpleNamespace(encoder=types.SimpleNamespace(num_resolutions=3), embed_dim=8)
        self.cond = FakeConditioner()
        self.cond_stage_models = [self.cond]
        self.cond_stage_model_metadata = {"film": {"model_idx": 0, "cond_stage_key": "all"},
                                          "ctx": {"model_idx": 0, "cond_stage_key": "all"}}
        self.clap = types.SimpleNamespace(decision_shard=None,
                                          cos_similarity=lambda wave, text: torch.arange(len(text)).float())
        self.calls = []

    def _check_candidates(self, n_gen, text=None):
        pass

    def _cfg_dropout_draw(self):
        pass

    def sample_log(self, **kw):
        self.calls.append(kw)
        return torch.zeros(kw["batch_size"], 8, 8, 16), None

    def decode_first_stage_cl(self, z):
        return torch.zeros(z.shape[0], 32, 64, 1)

    def mel_spectrogram_to_waveform(self, mel, savepath="", bs=None, name=None, save=False):
        return np.zeros((mel.shape[0], 1, 8), dtype=np.float32)


TEXTS = ["a dog barking", "rain", "slow piano melody"]
NEGS = ["Low quality.", "x", "noise, hiss"]


def make_batch(B0=3):
    fb = torch.zeros(B0, 32, 64)
    return {"text": list(TEXTS[:B0]), "fname": ["f"] * B0, "log_mel_spec": fb, "fbank": fb,
            "phoneme_idx": torch.full((B0, 310), 7, dtype=torch.long)}


KW = dict(ddim_steps=4, ddim_eta=0.0, unconditional_guidance_scale=3.5)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [-0.1, 1.5, float("nan"), float("inf"), "a lot"])
def test_guidance_rescale_outside_the_unit_interval_is_refused_everywhere(phi):
    from audioldm2_amd.ddim import DDIMSampler, check_guidance_rescale
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    with pytest.raises(ValueError, match="guidance_rescale"):
        check_guidance_rescale(phi)
    ld = FakeLD()
    for fn in (ld.generate_batch, ld.generate_batch_masked):
        with pytest.raises(ValueError, match="guidance_rescale"):
            fn(make_batch(), guidance_rescale=phi, **KW)
    with pytest.raises(ValueError, match="guidance_rescale"):
        ld.sample_log_real(None, 1, ddim=True, ddim_steps=4, guidance_rescale=phi)
    assert ld.calls == [] and ld.cond.seen == []          # refused before anything was computed
    model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
    for cls, loop in ((DDIMSampler, "ddim_sampling"), (PLMSSampler, "plms_sampling"), (DPMSolverSampler, "dpm_sampling")):
        s = cls(model)
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.sample(4, 1, (8, 8, 8), None, verbose=False, guidance_rescale=phi)
        s.make_schedule(4, ddim_eta=0.0, verbose=False)
        with pytest.raises(ValueError, match="guidance_rescale"):
            if cls is DDIMSampler:
                s.ddim_sampling(None, (1, 8, 8, 8), guidance_rescale=phi)
            else:    # the reference's PLMS signature, which DPMSolverSampler carries too: phi is sampler state there
                s.guidance_rescale = phi
                getattr(s, loop)(None, (1, 8, 8, 8))
    for phi_ok in (0, 0.0, 0.7, 1, 1.0):
        assert check_guidance_rescale(phi_ok) == float(phi_ok)


def test_eager_steps_refuse_a_bad_guidance_rescale_too():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.plms import PLMSSampler
    model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
    x, t = torch.zeros(1, 8, 8, 8), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="guidance_rescale"):
        DDIMSampler(model).p_sample_ddim(x, None, t, 0, guidance_rescale=2.0)
    s = PLMSSampler(model)
    assert s.guidance_rescale == 0.0
    s.guidance_rescale = 2.0
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.p_sample_plms(x, None, t, 0)
    assert "guidance_rescale" in inspect.signature(DDIMSampler.decode).parameters


def test_where_the_argument_is_a_parameter_and_where_sampler_state():
    """DDIMSampler names `guidance_rescale` in `sample`, `ddim_sampling`, `p_sample_ddim` and `decode` (its `sample`'s **kwargs would
    swallow an unknown name).  PLMSSampler's methods keep the reference class's signatures exactly, and DPMSolverSampler carries
    PLMSSampler's parameter lists: their `sample` reads the keyword from **kwargs and sets `self.guidance_rescale` on every call,
    their loop reads the attribute."""
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    for name in ("sample", "ddim_sampling", "p_sample_ddim", "decode"):
        p = inspect.signature(getattr(DDIMSampler, name)).parameters["guidance_rescale"]
        assert p.default == 0.0 and p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
    model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
    for cls, names in ((PLMSSampler, ("sample", "plms_sampling", "p_sample_plms")), (DPMSolverSampler, ("sample", "dpm_sampling"))):
        for name in names:
            assert "guidance_rescale" not in inspect.signature(getattr(cls, name)).parameters
        s = cls(model)
        assert s.guidance_rescale == 0.0
        seen = []
        setattr(s, names[1], lambda *a, **k: seen.append(s.guidance_rescale) or (None, None))
        s.sample(4, 1, (8, 8, 8), None, verbose=False, guidance_rescale=0.7)
        s.sample(4, 1, (8, 8, 8), None, verbose=False)          # a later job without the keyword is plain again
        assert seen == [0.7, 0.0]


def test_negative_prompt_at_scale_one_and_wrong_lists_are_refused():
    ld = FakeLD()
    for fn in (ld.generate_batch, ld.generate_batch_masked):
        with pytest.raises(ValueError, match="negative_prompt needs unconditional_guidance_scale"):
            fn(make_batch(), ddim_steps=4, unconditional_guidance_scale=1.0, negative_prompt="Low quality.")
        with pytest.raises(ValueError, match="list of 3 strings"):
            fn(make_batch(), negative_prompt=["a", "b"], **KW)
        with pytest.raises(ValueError, match="list of 3 strings"):
            fn(make_batch(), negative_prompt=["a", "b", 3], **KW)
    assert ld.calls == [] and ld.cond.seen == []


def test_the_ancestral_sampler_refuses_guidance_rescale():
    ld = FakeLD()
    with pytest.raises(ValueError, match="needs ddim_steps"):
        ld.generate_batch(make_batch(), ddim_steps=None, unconditional_guidance_scale=3.5, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="needs ddim_steps"):
        ld.sample_log_real(None, 1, ddim=False, ddim_steps=None, guidance_rescale=0.7)
    assert ld.calls == [] and ld.cond.seen == []


# ---- the negative batch ----------------------------------------------------------------------------------------------------------
def test_negative_batch_replaces_text_and_transcription_only():
    from audioldm2_amd.phoneme import phoneme_ids
    batch = make_batch()
    for neg, want in (("Low quality.", ["Low quality."] * 3), (NEGS, NEGS), (tuple(NEGS), NEGS)):
        nb = P.negative_batch(batch, neg)
        assert nb["text"] == want and nb["text"] is not batch["text"]
        assert torch.equal(nb["phoneme_idx"], phoneme_ids("", 3)) and nb["phoneme_idx"].shape == (3, 310)
        assert int((nb["phoneme_idx"][0] != 0).sum()) == 1          # the end mark alone
        assert set(nb) == set(batch) and all(nb[k] is batch[k] for k in batch if k not in ("text", "phoneme_idx"))
    assert batch["text"] == TEXTS and bool((batch["phoneme_idx"] == 7).all())   # the caller's batch is not touched


def code_of(texts):
    return torch.tensor([[float(len(t)), float(i)] for i, t in enumerate(texts)])


@pytest.mark.parametrize("n_gen", [1, 2])
def test_negative_conditioning_is_tiled_like_c_and_handed_down(n_gen):
    ld = FakeLD()
    ld.generate_batch(make_batch(), n_gen=n_gen, negative_prompt=NEGS, guidance_rescale=0.7, **KW)
    assert [b["text"] for b in ld.cond.seen] == [TEXTS, NEGS]     # the negative pass runs after the positive one
    (kw,) = ld.calls
    assert kw["batch_size"] == 3 * n_gen and kw["guidance_rescale"] == 0.7 and kw["unconditional_guidance_scale"] == 3.5
    for cond, texts in ((kw["cond"], TEXTS), (kw["unconditional_conditioning"], NEGS)):
        full = torch.cat([code_of(texts)] * n_gen)
        assert sorted(cond) == ["ctx", "film"]
        assert torch.equal(cond["film"], full) and torch.equal(cond["ctx"][0], full[:, None, :])
        assert cond["ctx"][1].shape == (3 * n_gen, 1)


@pytest.mark.parametrize("n_gen", [1, 2])
def test_two_rank_shard_cuts_the_negative_conditioning_with_c(n_gen):
    from audioldm2_amd.dist import candidate_rows
    seen = []
    for rank in (0, 1):
        ld = FakeLD()
        ld.generate_batch(make_batch(), n_gen=n_gen, negative_prompt=NEGS, shard=(rank, 2), **KW)
        (kw,) = ld.calls
        rows = candidate_rows(3, n_gen, rank, 2)
        assert kw["batch_size"] == len(rows)
        for cond, texts in ((kw["cond"], TEXTS), (kw["unconditional_conditioning"], NEGS)):
            full = torch.cat([code_of(texts)] * n_gen)
            assert torch.equal(cond["film"], full[rows]) and torch.equal(cond["ctx"][0], full[rows][:, None, :])
            assert cond["ctx"][1].shape == (len(rows), 1)
        seen += rows.tolist()
    assert sorted(seen) == list(range(3 * n_gen))


def test_without_the_arguments_the_call_is_todays():
    """No negative prompt: the unconditional half is get_unconditional_condition, one conditioner pass, the host generator is
    where it was; no guidance_rescale: the keyword does not reach sample_log."""
    states = []
    for extra in (dict(), dict(negative_prompt=None, guidance_rescale=0.0)):
        ld = FakeLD()
        torch.manual_seed(5)
        ld.generate_batch(make_batch(), **KW, **extra)
        states.append(torch.get_rng_state())
        (kw,) = ld.calls
        assert "guidance_rescale" not in kw and "negative_prompt" not in kw
        assert len(ld.cond.seen) == 1
        assert sorted(kw["unconditional_conditioning"]) == ["ctx", "film"]
        assert torch.equal(kw["unconditional_conditioning"]["film"], torch.full((3, 2), -1.0))
    assert torch.equal(states[0], states[1])


def test_masked_job_takes_both_arguments(monkeypatch):
    ld = FakeLD()
    ld.device = "cpu"
    ld.encode_first_stage = lambda x: x
    ld.get_first_stage_encoding = lambda e: torch.zeros(e.shape[0], 8, 8, 16)
    ld.generate_batch_masked(make_batch(), negative_prompt="Low quality.", guidance_rescale=0.5, **KW)
    (kw,) = ld.calls
    assert kw["guidance_rescale"] == 0.5 and kw["mask"].shape == (3, 1, 8, 16)
    assert torch.equal(kw["unconditional_conditioning"]["film"], code_of(["Low quality."] * 3))
    assert [b["text"] for b in ld.cond.seen] == [TEXTS, ["Low quality."] * 3]


# ---- public interface -----------------------------------------------------------------------------------------------------------
def test_entry_points_gain_the_two_arguments_in_front_of_sampler(monkeypatch):
    for fn in (P.text_to_audio, P.super_resolution_and_inpainting):
        params = list(inspect.signature(fn).parameters.values())
        # `sampler` stays the last parameter; the two new ones sit between the reference's last parameter and it
        assert [p.name for p in params[-4:]] == ["config", "negative_prompt", "guidance_rescale", "sampler"]
        assert params[-3].default is None and params[-2].default == 0.0 and params[-1].default is None
    got = {}

    class LD:
        def generate_batch(self, batch, **kw):
            got.update(kw)
            return "wave"
    assert P.text_to_audio(LD(), "a dog", ddim_steps=4, negative_prompt="Low quality.", guidance_rescale=0.7) == "wave"
    assert got["negative_prompt"] == "Low quality." and got["guidance_rescale"] == 0.7 and "sampler" not in got
    got.clear()
    P.text_to_audio(LD(), "a dog", ddim_steps=4)
    assert "negative_prompt" not in got and "guidance_rescale" not in got


def test_sample_log_forwards_guidance_rescale_to_all_three_samplers(monkeypatch):
    from audioldm2_amd import dpm_solver, plms
    seen = []

    def fake(name):
        class S:
            def __init__(self, model, **kw):
                pass

            def sample(self, *a, **kw):
                seen.append((name, kw.get("guidance_rescale", "absent")))
                return torch.zeros(1), None
        return S
    monkeypatch.setattr(P, "DDIMSampler", fake("ddim"))
    monkeypatch.setattr(plms, "PLMSSampler", fake("plms"))
    monkeypatch.setattr(dpm_solver, "DPMSolverSampler", fake("dpmpp"))
    ld = FakeLD()
    ld.device = "cpu"
    for how in (dict(), dict(use_plms=True), dict(sampler="dpmpp_2m")):
        ld.sample_log_real(None, 1, ddim=True, ddim_steps=4, guidance_rescale=0.7, **how)
        ld.sample_log_real(None, 1, ddim=True, ddim_steps=4, **how)
        ld.sample_log_real(None, 1, ddim=True, ddim_steps=4, guidance_rescale=0.0, **how)
    assert seen == [(n, v) for n in ("ddim", "plms", "dpmpp") for v in (0.7, "absent", "absent")]


# ---- the coefficient tables -------------------------------------------------------------------------------------------------------
def test_sampler_tables_carry_scale_flag_and_phi():
    from audioldm2_amd.ddim import DDIMSampler, guidance_table
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    model = types.SimpleNamespace(num_timesteps=1000, alphas_cumprod=torch.linspace(0.99, 0.01, 1000))
    for cls, attr in ((DDIMSampler, "ddim_coef"), (PLMSSampler, "plms_coef"), (DPMSolverSampler, "dpm_coef")):
        s = cls(model)
        s.make_schedule(4, ddim_eta=0.0, verbose=False)
        rows = getattr(s, attr)
        assert rows.shape == (4, 5)
        for use_cfg, phi, col6, col7 in ((True, 0.7, 0.0, 0.7), (True, 1.0, 0.0, 1.0), (True, 0.0, 1.0, 0.0),
                                         (False, 0.7, 0.0, 0.0), (False, 0.0, 0.0, 0.0)):
            tab = guidance_table(rows, 3.5, use_cfg, phi)
            assert tab.shape == (4, 8) and tab.dtype == torch.float32 and torch.equal(tab[:, :5], rows.float())
            assert bool((tab[:, 5] == 3.5).all()) and bool((tab[:, 6] == col6).all())
            assert bool((tab[:, 7] == torch.tensor(col7)).all())
    src = {cls: inspect.getsource(cls) for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler)}
    assert all("guidance_table(" in v for v in src.values())          # the loops build their tables with it
