"""Fixtures of the durations other than 10 s and of the fifth model, audioldm_16k_crossattn_t5, from the REAL reference on the CPU
(tests/test_durations_cpu.py, tests/test_durations_gpu.py):
  tests/golden/reference_config_t5.json   the reference's default_audioldm_config("audioldm_16k_crossattn_t5")["model"]["params"]
  tests/golden/e2et5_statedict_keys.json  names and shapes of its LatentDiffusion's hot-path tensors (model.diffusion_model.*,
                                          first_stage_model.*)
  tests/golden/e2e_dur_<model>_<latent_t>.npz  the reference's generate_batch (B = 2, 5 DDIM steps, CFG 3.5, seed 42, random-init
                                          weights as in oracle/make_golden.py) at latent_t_size != the 10 s value: t5 at 256 / 192
                                          (10 s / 7.5 s), audioldm_48k at 96 / 64 (7.5 s / 5 s).  The waveform is stored as its head
                                          and every 16th sample, like gen_e2e_named.
Usage: python tools/make_golden_durations.py [config | t5_256 | t5_192 | 48k_96 | 48k_64 ...]  (no argument: everything).
Needs the reference checkout (ALDM_REFERENCE_ROOT overrides its location).  Uses the helpers of oracle/make_golden.py,
oracle/refimport.py and oracle/cases.py without modifying them."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import cases, make_golden as mg, refimport  # noqa: E402

T5 = "audioldm_16k_crossattn_t5"
# job -> (model name, keys fixture, latent_t_size, duration in s, batch builder)
E2E = {"t5_256": (T5, "e2et5_statedict_keys.json", 256, 10.0, cases.e2e_batch),
       "t5_192": (T5, "e2et5_statedict_keys.json", 192, 7.5, cases.e2e_batch),
       "48k_96": ("audioldm_48k", "e2e48k_statedict_keys.json", 96, 7.5, cases.e2e_batch_48k),
       "48k_64": ("audioldm_48k", "e2e48k_statedict_keys.json", 64, 5.0, cases.e2e_batch_48k)}
B, STEPS = 2, 5


def fixture_name(job):
    model, _, T, _, _ = E2E[job]
    return f"e2e_dur_{'t5' if model == T5 else '48k'}_{T}"


def gen_config():
    refimport.install()
    import audioldm2.utils as ru
    os.makedirs(mg.OUT, exist_ok=True)
    with open(os.path.join(mg.OUT, "reference_config_t5.json"), "w") as f:
        json.dump(ru.default_audioldm_config(T5)["model"]["params"], f, indent=0)
    mg._ref_latent_diffusion_named(T5, "e2et5_statedict_keys.json")


def gen_e2e(job):
    model, keys_json, T, dur, batch = E2E[job]
    name = fixture_name(job)
    ld = mg._ref_latent_diffusion_named(model, keys_json)
    ld.latent_t_size = T
    rec = {}
    orig = ld.decode_first_stage

    def decode_hook(z):
        rec["latent"] = z.clone()
        return orig(z)
    ld.decode_first_stage = decode_hook
    mg._seed_all()
    t0 = time.time()
    wav = ld.generate_batch(batch(B), unconditional_guidance_scale=3.5, ddim_steps=STEPS, n_gen=1, duration=dur)
    ld.decode_first_stage = orig
    btw = mg.between_sample_rms(ld, wav, rec["latent"])
    print(f"{name}: reference generate_batch({model}, latent_t {T}) B={B} steps={STEPS}: {time.time() - t0:.1f}s wave {wav.shape} "
          f"between-sample rms {btw:.4f} = {btw / mg.rms64(wav):.2f} x wave rms")
    mg.save(name, latent=rec["latent"], wave_head=wav[..., :32768], wave_dec=wav[..., ::16],
            wave_len=np.int64(wav.shape[-1]), wave_rms=np.float64(mg.rms64(wav)), wave_between_rms=np.float64(btw))


def main():
    jobs = sys.argv[1:] or ["config"] + list(E2E)
    for j in jobs:
        gen_config() if j == "config" else gen_e2e(j)


if __name__ == "__main__":
    main()
