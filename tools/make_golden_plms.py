"""Fixtures of the PLMS sampler from the REAL reference on the CPU (tests/test_plms_cpu.py, tests/test_plms_gpu.py):
  tests/golden/e2e_plms_6step_b2.npz         the reference's generate_batch(use_plms=True, ddim_eta=0.0, ddim_steps=6,
                                             unconditional_guidance_scale=1.0) at B = 2, seed 42, the audioldm2-full recipe and
                                             random-init weights of e2e_full_5step_b2 (oracle/make_golden.py).  Six steps reach every
                                             order of plms.py:341-356: improved Euler, 2nd, 3rd, then three 4th-order steps.
  tests/golden/e2e_plms_masked_4step_b1.npz  the same through generate_batch_masked (B = 1, 4 steps).
Each stores the job's inputs (x_T; x0 and mask for the masked job), the final latent, the waveform (B = 2: its head and every 16th
sample, like the batch-8 fixtures, to stay under 1 MiB) and `rand_after` = float(torch.rand(1)) drawn right after the job: the state
the reference leaves the host generator in (RNG contract R).  Guidance is 1.0 because the reference's own p_sample_plms cannot run
under guidance with dict conditioning (plms.py:290).
Usage: python tools/make_golden_plms.py [plain | masked ...]  (no argument: both).
Needs the reference checkout (ALDM_REFERENCE_ROOT overrides its location).  Uses the helpers of oracle/make_golden.py,
oracle/refimport.py and oracle/cases.py without modifying them."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import cases, make_golden as mg, refimport  # noqa: E402

JOBS = {"plain": ("e2e_plms_6step_b2", 2, 6), "masked": ("e2e_plms_masked_4step_b1", 1, 4)}


class _ShapedList(list):
    """A [context, mask] conditioning entry that also answers `.shape`: PLMSSampler.sample reads `.shape[0]` of the first
    conditioning entry for a batch-size warning (plms.py:117-123) and every AudioLDM2 cross-attention entry is a list, so
    as shipped the call ends there with AttributeError.  With this the reference's own code runs on, unmodified."""

    @property
    def shape(self):
        return self[0].shape


def _reference():
    """The reference LatentDiffusion of e2e_full_5step_b2 with a PLMSSampler that runs on the CPU: the class's register_buffer moves
    every table to "cuda" (plms.py:21-25), the one line of it that cannot run here; the tables stay where make_schedule made them."""
    ld = mg._ref_latent_diffusion()
    ld.latent_t_size = 256
    from audioldm2.latent_diffusion.models import plms
    plms.PLMSSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return ld, plms.PLMSSampler


def gen(job):
    name, B, steps = JOBS[job]
    ld, sampler_cls = _reference()
    rec = {}
    orig_decode, orig_sample_log, orig_step = ld.decode_first_stage, ld.sample_log, sampler_cls.p_sample_plms

    def decode_hook(z):
        rec["latent"] = z.clone()
        return orig_decode(z)

    def sample_log_hook(*a, **k):
        if k.get("mask") is not None:
            rec["x0"], rec["mask"] = k["x0"].clone(), k["mask"].clone()
        first = next(iter(k["cond"]))
        if isinstance(k["cond"][first], list):
            k["cond"] = dict(k["cond"], **{first: _ShapedList(k["cond"][first])})
        return orig_sample_log(*a, **k)

    def step_hook(self, x, *a, **k):
        rec.setdefault("x_T", x.clone())
        rec["unet_passes"] = rec.get("unet_passes", 0) + (2 if len(k["old_eps"]) == 0 else 1)
        return orig_step(self, x, *a, **k)
    ld.decode_first_stage, ld.sample_log, sampler_cls.p_sample_plms = decode_hook, sample_log_hook, step_hook
    mg._seed_all()
    t0 = time.time()
    kw = dict(use_plms=True, ddim_eta=0.0, ddim_steps=steps, unconditional_guidance_scale=1.0, n_gen=1, duration=10)
    if job == "masked":
        wav = ld.generate_batch_masked(cases.e2e_masked_batch(B), time_mask_ratio_start_and_end=(0.25, 0.75),
                                       freq_mask_ratio_start_and_end=(0.75, 1.0), **kw)
    else:
        wav = ld.generate_batch(cases.e2e_batch(B), **kw)
    rand_after = float(torch.rand(1))   # the next consumer of the host generator
    ld.decode_first_stage, ld.sample_log, sampler_cls.p_sample_plms = orig_decode, orig_sample_log, orig_step
    btw = mg.between_sample_rms(ld, wav, rec["latent"])
    print(f"{name}: reference PLMS B={B} steps={steps} ({rec['unet_passes']} UNet passes): {time.time() - t0:.1f}s wave {wav.shape} "
          f"rms {mg.rms64(wav):.4f} latent std {rec['latent'].std():.3f} between-sample rms {btw:.4f} rand_after {rand_after!r}")
    arrs = dict(latent=rec["latent"], rand_after=np.float64(rand_after), steps=np.int64(steps),
                wave_len=np.int64(wav.shape[-1]), wave_rms=np.float64(mg.rms64(wav)), wave_between_rms=np.float64(btw))
    if job == "masked":
        arrs.update(x0=rec["x0"], mask=rec["mask"], wave=wav)
    else:
        arrs.update(x_T=rec["x_T"], wave_head=wav[..., :32768], wave_dec=wav[..., ::16])
    mg.save(name, **arrs)
    path = os.path.join(mg.OUT, name + ".npz")
    assert os.path.getsize(path) <= 1 << 20, "a committed fixture stays under 1 MiB"


def main():
    for j in sys.argv[1:] or list(JOBS):
        gen(j)


if __name__ == "__main__":
    main()
