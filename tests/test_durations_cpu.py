"""The fifth model (audioldm_16k_crossattn_t5) and the accepted durations, on the host: its config and state-dict keys against the
real reference (tests/golden/reference_config_t5.json, e2et5_statedict_keys.json: tools/make_golden_durations.py), its real
conditioner stack, the latent_t_size check, and the four existing configs unchanged."""
import json
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T5 = "audioldm_16k_crossattn_t5"


def _gold(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def test_t5_model_config_equals_the_reference():
    """default_audioldm_config("audioldm_16k_crossattn_t5"): the reference's unet / first-stage params (utils.py:563-706), one
    context slot of 1024 channels — not the audioldm2-full architecture the name used to fall through to."""
    from audioldm2_amd import pipeline as P
    ref = _gold("reference_config_t5.json")
    mp = P.default_audioldm_config(T5)["model"]["params"]
    assert mp["unet_config"]["params"] == ref["unet_config"]["params"]
    assert mp["unet_config"]["params"]["context_dim"] == [1024]
    fs, rfs = mp["first_stage_config"]["params"], ref["first_stage_config"]["params"]
    assert fs["ddconfig"] == rfs["ddconfig"]
    for k in ("sampling_rate", "embed_dim", "subband", "time_shuffle", "image_key"):
        assert fs[k] == rfs[k], k
    for k in ("latent_t_size", "latent_f_size", "channels", "sampling_rate", "linear_start", "linear_end", "timesteps",
              "parameterization", "first_stage_key", "scale_by_std"):
        assert mp[k] == ref[k], k
    assert list(mp["cond_stage_config"]) == list(ref["cond_stage_config"]) == ["crossattn_flan_t5"]
    c = mp["cond_stage_config"]["crossattn_flan_t5"]
    assert c["params"]["dim"] == 1024 and c["params"]["uncond_length"] == 1 and c["conditioning_key"] == "crossattn"
    # through the reference's own dict as well
    ours = P.retarget_config({"model": {"target": "audioldm2.latent_diffusion.models.ddpm.LatentDiffusion", "params": ref}})
    assert ours["model"]["params"]["unet_config"] == mp["unet_config"]
    assert ours["model"]["params"]["cond_stage_config"] == P.hip_cond_stage_config(T5)


def test_t5_model_state_dict_keys_equal_the_reference():
    from audioldm2_amd.pipeline import build_model
    m = build_model(model_name=T5)
    mine = {k: list(v.shape) for k, v in m.state_dict().items()
            if k.startswith("model.diffusion_model.") or k.startswith("first_stage_model.")}
    assert mine == _gold("e2et5_statedict_keys.json")
    sd = {k: torch.zeros(v.shape) for k, v in m.state_dict().items()}
    sd["cond_stage_models.0.x"] = torch.zeros(1)
    assert "cond_stage_models.0.x" in m.load_reference_state_dict(sd)


def test_t5_model_hip_conditioners_are_flan_t5_alone():
    from audioldm2_amd import pipeline as P
    c = P.hip_cond_stage_config(T5)
    assert list(c) == ["crossattn_flan_t5"] and c["crossattn_flan_t5"]["target"] == "audioldm2_amd.t5.FlanT5HiddenState"
    assert P.default_audioldm_config(T5, conditioners="hip")["model"]["params"]["cond_stage_config"] == c


@pytest.mark.parametrize("latent_t", [100, 92, 4, 0, -8, 96.0])
def test_latent_t_not_a_multiple_of_8_raises_before_sampling(latent_t):
    """The reference's UNet fails in its skip concatenation (openaimodel.py:879) unless latent_t % 8 == 0; generate_batch says so
    before any conditioning or GPU work (this runs without a GPU)."""
    from audioldm2_amd.pipeline import LatentDiffusion, build_model, make_batch_for_text_to_audio
    with pytest.raises(ValueError, match="multiple of 8"):
        LatentDiffusion.check_latent_t(latent_t)
    ld = build_model(model_name="audioldm_48k")
    ld.latent_t_size = latent_t
    with pytest.raises(ValueError, match="multiple of 8"):
        ld.generate_batch(make_batch_for_text_to_audio("a dog", batchsize=1), ddim_steps=2)
    for ok in (8, 64, 96, 192, 256):
        LatentDiffusion.check_latent_t(ok)


def test_the_four_existing_configs_are_unchanged():
    from audioldm2_amd import pipeline as P
    ref = _gold("reference_configs.json")
    for name in ("audioldm2-full", "audioldm2-full-large-1150k", "audioldm2-speech-gigaspeech", "audioldm_48k"):
        mp = P.default_audioldm_config(name)["model"]["params"]
        rp = ref[name]["model"]["params"]
        assert mp["unet_config"]["params"] == rp["unet_config"]["params"], name
        assert mp["first_stage_config"]["params"]["ddconfig"] == rp["first_stage_config"]["params"]["ddconfig"], name
        assert list(P.hip_cond_stage_config(name)) == list(rp["cond_stage_config"]), name
        assert mp["latent_t_size"] == (128 if "48k" in name else 256)
