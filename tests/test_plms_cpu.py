"""Host side of the PLMS sampler (audioldm2_amd/plms.py): the schedule refuses eta != 0, the six public methods carry the
reference class's signatures, the fixtures of tools/make_golden_plms.py are complete.  No kernel is launched here."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import refimport

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ("__init__", "register_buffer", "make_schedule", "sample", "plms_sampling", "p_sample_plms")


class _ScheduleOnly:
    """What make_schedule reads on its model."""
    num_timesteps = 1000
    alphas_cumprod = torch.cumprod(1.0 - torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2, 0).float()


def test_make_schedule_refuses_nonzero_eta():
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(_ScheduleOnly())
    with pytest.raises(ValueError, match="ddim_eta must equal 0 for PLMS"):
        s.make_schedule(8, ddim_eta=0.1)
    s.make_schedule(8, ddim_eta=0.0)
    assert s.plms_coef.shape == (8, 5) and float(s.plms_coef[:, 4].abs().max()) == 0.0   # sigma = 0 at every step
    assert float(s.ddim_sigmas.abs().max()) == 0.0


def test_make_schedule_tables_are_ddims_at_eta_zero():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.plms import PLMSSampler
    p, d = PLMSSampler(_ScheduleOnly()), DDIMSampler(_ScheduleOnly(), device="cpu")
    for S in (1, 6, 50):
        p.make_schedule(S, ddim_eta=0.0)
        d.make_schedule(S, ddim_eta=0.0)
        assert np.array_equal(p.ddim_timesteps, d.ddim_timesteps) and torch.equal(p.plms_coef, d.ddim_coef)


@pytest.mark.skipif(not refimport.available(), reason="reference checkout not present")
def test_signatures_equal_the_reference_class():
    refimport.install()
    from audioldm2.latent_diffusion.models.plms import PLMSSampler as Ref
    from audioldm2_amd.plms import PLMSSampler
    for name in METHODS:
        assert inspect.signature(getattr(PLMSSampler, name)) == inspect.signature(getattr(Ref, name)), name


def test_unsupported_options_raise():
    from audioldm2_amd.plms import PLMSSampler
    s = PLMSSampler(_ScheduleOnly())
    s.make_schedule(4)
    for kw in ({"ddim_use_original_steps": True}, {"quantize_denoised": True}, {"score_corrector": object()},
               {"noise_dropout": 0.1}):
        with pytest.raises(NotImplementedError, match=r"PLMSSampler\(HIP\)"):
            s.plms_sampling(None, (1, 8, 4, 4), **kw)


@pytest.mark.parametrize("name,keys,B", [
    ("e2e_plms_6step_b2", ("x_T", "latent", "wave_head", "wave_dec", "wave_len", "wave_rms", "wave_between_rms", "rand_after",
                           "steps"), 2),
    ("e2e_plms_masked_4step_b1", ("x0", "mask", "latent", "wave", "wave_len", "wave_rms", "wave_between_rms", "rand_after",
                                  "steps"), 1)])
def test_fixture_is_complete(name, keys, B):
    path = os.path.join(GOLD, name + ".npz")
    assert os.path.getsize(path) <= 1 << 20
    g = np.load(path)
    assert sorted(g.files) == sorted(keys)
    assert g["latent"].shape == (B, 8, 256, 16) and g["latent"].dtype == np.float32 and np.isfinite(g["latent"]).all()
    assert int(g["wave_len"]) == 163872 and 0.0 < float(g["rand_after"]) < 1.0
    assert float(g["wave_between_rms"]) > 1e-2   # the waveforms depend on the sample
    if B == 1:
        assert g["wave"].shape == (1, 1, 163872) and g["x0"].shape == (1, 8, 256, 16) and g["mask"].shape == (1, 1, 256, 16)
        assert set(np.unique(g["mask"])) == {0.0, 1.0}
    else:
        assert g["wave_head"].shape == (2, 1, 32768) and g["wave_dec"].shape == (2, 1, 10242) and g["x_T"].shape == (2, 8, 256, 16)
