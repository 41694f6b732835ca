"""The reference-side binding of INTEGRATION.md §2 (VERDICT r1 "what's weak" #1):

 (a) CPU: the schedule and conditioning methods of our LatentDiffusion are bit-equal to the REAL reference class's on the same
     inputs (its results recorded by `oracle/make_golden.py host`).
 (b) GPU: `audioldm2_amd.ddim.DDIMSampler` driven by a model that exposes ONLY what the reference's LatentDiffusion
     offers a sampler (`apply_model`, `num_timesteps`, `alphas_cumprod`; no `apply_model_cfg` / `prepare_cfg`), i.e. the
     two-sequential-pass CFG fallback the reference's own class would hit (ddim.py:293-296), against the reference
     fixture and against the batched path."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


class _ReferenceShapedModel:
    """What ddim.py touches on its model (`:19,42,46-51,188,228,285-296,302,338`): nothing else is exposed."""

    def __init__(self, ld):
        self._ld = ld
        self.num_timesteps = ld.num_timesteps
        self.alphas_cumprod = ld.alphas_cumprod
        self.device = ld.device

    def apply_model(self, x_noisy, t, cond):
        return self._ld.apply_model(x_noisy, t, cond)


@pytest.mark.gpu
def test_ddim_sampler_two_pass_cfg_fallback_matches_reference_fixture_and_batched_path():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.pipeline import build_model, seed_everything
    g = np.load(os.path.join(GOLD, "e2e_full_5step_b2.npz"))
    ld = build_model(model_name="audioldm2-full")
    with open(os.path.join(GOLD, "e2e_statedict_keys.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = weights.make_state_dict(shapes, seed=0)
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    ld.load_state_dict(sd, strict=False)
    ld = ld.cuda()
    ld.latent_t_size = 256
    B, steps = 2, 5
    batch = cases.e2e_batch(B)

    def run(model):
        seed_everything(cases.E2E_SEED)
        torch.randn((B, 8, 256, 16))  # RNG contract R1: the posterior draw of the zero-mel encode (ddpm.py:1500)
        cond = ld.get_learned_conditioning_dict(batch)
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        s = DDIMSampler(model)
        z, _ = s.sample(steps, B, (8, 256, 16), cond, eta=1.0, verbose=False, unconditional_guidance_scale=3.5,
                        unconditional_conditioning=uncond)
        return z
    shim = _ReferenceShapedModel(ld)
    assert not hasattr(shim, "apply_model_cfg") and not hasattr(shim, "prepare_cfg")
    z_two = run(shim).double().cpu().numpy()
    z_bat = run(ld).double().cpu().numpy()
    e_ref = _rms(z_two - g["latent"]) / _rms(g["latent"])
    e_bat = _rms(z_two - z_bat) / _rms(z_bat)
    print(f"two-pass CFG fallback: latent rel rms vs reference {e_ref:.2e}, vs batched path {e_bat:.2e}")
    assert e_ref < 1e-4   # same bar as test_e2e_5step_matches_reference_generate_batch
    assert e_bat < 1e-5


# ---- the conditioner drop-in (VERDICT r2 "missing" #1 / next #4) ------------------------------------------------------------
def _cond_keys():
    with open(os.path.join(GOLD, "e2econd_statedict_keys.json")) as f:
        k = json.load(f)
    return {a: tuple(b) for a, b in k["hot"].items()}, {a: tuple(b) for a, b in k["cond"].items()}


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(GOLD, "e2e_cond_4step_b2.npz")), reason="conditioner e2e fixture absent")
def test_prompts_to_waveform_through_the_hip_conditioner_stack():
    """prompts -> (stub tokenizers) -> CLAP text + FLAN-T5 -> GPT-2 sequence generator -> DDIM -> VAE -> HiFi-GAN as ONE job of
    `default_audioldm_config(conditioners="hip")`, against the same job run by the REAL reference LatentDiffusion over the REAL
    SequenceGenAudioMAECond / FlanT5HiddenState (fixture e2e_cond_4step_b2: two prompts, 4 DDIM steps, CFG 3.5, seed 42;
    random-init weights; T5 with 3 of 24 layers, RoBERTa with 2 of 12)."""
    from audioldm2_amd.pipeline import LatentDiffusion, default_audioldm_config, seed_everything
    g = np.load(os.path.join(GOLD, "e2e_cond_4step_b2.npz"))
    hot, cond = _cond_keys()
    cfg = default_audioldm_config("audioldm2-full", conditioners="hip", t5_config=cases.t5_test_config(),
                                  clap_config=cases.clap_text_test_config())
    cfg["model"]["params"]["build_clap"] = False    # one candidate per prompt: no re-ranker needed
    torch.manual_seed(0)
    ld = LatentDiffusion(**cfg["model"]["params"]).eval()
    sd = weights.make_state_dict(hot, seed=0)
    sd.update(cases.cond_state_dict(cond, seed=0))
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    res = ld.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys[:5]
    ld = ld.cuda()
    seq = ld.cond_stage_models[0]
    seq.cond_stage_models[0].tokenize = cases.StubRobertaTokenizer()
    seq.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    ld.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    rec = {}
    orig_fwd, orig_dec = seq.forward, ld.decode_first_stage_cl

    def fwd(batch):
        ret = orig_fwd(batch)
        rec["tokens"], rec["clap"], rec["t5"] = ret["crossattn_audiomae_generated"][0], ret["film_clap_cond1"], ret["crossattn_flan_t5"][0]
        return ret

    def dec(z):
        rec["latent"] = z.clone()
        return orig_dec(z)
    seq.forward, ld.decode_first_stage_cl = fwd, dec
    seed_everything(cases.E2E_SEED)
    ld.latent_t_size = 256
    wave = ld.generate_batch(cases.e2e_cond_batch(), unconditional_guidance_scale=3.5, ddim_steps=4, n_gen=1, duration=10)
    assert wave.shape == (2, 1, int(g["wave_len"]))
    rel = lambda a, b: _rms(np.asarray(a, dtype=np.float64) - b) / _rms(b)
    e_clap = rel(rec["clap"].double().cpu().numpy(), g["clap"])
    e_t5 = rel(rec["t5"].double().cpu().numpy(), g["t5"])
    e_tok = rel(rec["tokens"].double().cpu().numpy(), g["tokens"])
    e_lat = rel(rec["latent"].double().cpu().numpy(), g["latent"])
    eh = _rms(wave[..., :32768].astype(np.float64) - g["wave_head"])
    ed = _rms(wave[..., ::16].astype(np.float64) - g["wave_dec"])
    print(f"conditioner e2e: clap {e_clap:.2e}  t5 {e_t5:.2e}  generated tokens {e_tok:.2e}  latent {e_lat:.2e}  wave rms_err "
          f"{max(eh, ed):.3e} / between-sample {float(g['wave_between_rms']):.3e}")
    assert e_clap < 2e-4 and e_t5 < 2e-4 and e_tok < 5e-4
    assert e_lat < 2e-4
    assert max(eh, ed) < 1e-3 and max(eh, ed) < 1e-3 * float(g["wave_between_rms"])


def test_schedule_and_conditioning_helpers_equal_the_reference_methods():
    """q_sample / predict_start_from_noise / q_posterior / get_learned_conditioning / filter_useful_cond_dict of OUR
    LatentDiffusion against what the same methods of the REAL reference class (ddpm.py:357-373, 430-436, 804-828, 958-971), built
    with the same config, returned on the same inputs (recorded by `oracle/make_golden.py host`): bit-equal (the tables are the
    same fp32 numbers, the arithmetic the same torch expressions)."""
    from audioldm2_amd import pipeline as P
    ref = np.load(os.path.join(GOLD, "reference_host.npz"))
    want = lambda k: torch.from_numpy(ref[k])
    op = P.default_audioldm_config("audioldm2-full")["model"]["params"]
    op["cond_stage_config"] = cases.e2e_cond_config("cpu")
    op["device"], op["build_clap"] = "cpu", False
    ours = P.LatentDiffusion(**op).eval()
    g = torch.Generator().manual_seed(0)
    x0, xt, eps = (torch.randn(3, 8, 16, 16, generator=g) for _ in range(3))
    t = torch.tensor([0, 417, 999])
    assert torch.equal(ours.q_sample(x0, t, eps), want("q_sample"))
    assert torch.equal(ours.predict_start_from_noise(xt, t, eps), want("predict_start_from_noise"))
    for i, a in enumerate(ours.q_posterior(x0, xt, t)):
        b = want(f"q_posterior{i}")
        assert torch.equal(a.expand_as(b), b)
    torch.manual_seed(7)
    assert torch.equal(ours.q_sample(x0, t), want("q_sample_drawn"))    # the same randn_like draw when no noise is given
    batch = cases.e2e_batch(2)
    keys = json.loads(str(ref["uncond_keys"]))
    assert list(ours.cond_stage_model_metadata) == keys
    for key in keys:
        meta = ours.cond_stage_model_metadata[key]
        xc = batch if meta["cond_stage_key"] == "all" else batch[meta["cond_stage_key"]]
        u_our = ours.get_learned_conditioning(xc, key, unconditional_cfg=True)
        flat = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
        for j, p in enumerate(flat(u_our)):
            assert torch.equal(p, want(f"uncond_{key}_{j}")), key
        assert f"uncond_{key}_{len(flat(u_our))}" not in ref.files, key
    d = {k: torch.zeros(1) for k in keys}
    d["noise"] = torch.ones(1)
    assert list(ours.filter_useful_cond_dict(d).keys()) == json.loads(str(ref["filter_useful_keys"]))
    with pytest.raises(AssertionError):
        ours.filter_useful_cond_dict({"noise": d["noise"]})


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_parity_on_checkpoint_script_hip_stage_meets_the_bars_on_the_committed_reference_cache(tmp_path):
    """tools/parity_on_checkpoint.py end to end, the half the CPU suite cannot run: the hip stage loads a
    reference-format checkpoint through `build_model(ckpt_path=...)`, runs the jobs on the MI355X and compares latent / mel /
    waveform with what the REAL reference produced from the SAME checkpoint on the CPU.  The checkpoint is the deterministic random-init
    one `--make-random-ckpt` writes (oracle.weights seed 3 — reproduced here bit for bit, 1.8 GB, not committed); the reference side is
    `tests/golden/parity_script_ref_s5b2_s20b1.npz`, written in the build container by
        python tools/parity_on_checkpoint.py --ckpt /tmp/rand.pth --make-random-ckpt --steps 5,20 --batch 2,1 --stage reference --cache <that file>
    (5 DDIM steps x 2 prompts, 20 steps x 1).  Exit code 0 = every job inside the per-mode bars of tests/tolerances.py."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cache = os.path.join(GOLD, "parity_script_ref_s5b2_s20b1.npz")
    ckpt = str(tmp_path / "rand.pth")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "parity_on_checkpoint.py"), "--ckpt", ckpt, "--make-random-ckpt",
                        "--model", "audioldm2-full", "--steps", "5,20", "--batch", "2,1", "--stage", "hip", "--cache", cache],
                       capture_output=True, text=True, timeout=850)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["ok"] and [(j["steps"], j["batch"]) for j in rec["jobs"]] == [(5, 2), (20, 1)]
    for j in rec["jobs"]:
        assert j["latent_rel_rms"] < 1e-5 and j["wave_rms_err"] < 1e-5   # measured ~2e-6 / ~4e-7 in the default (fp32-grade) mode
