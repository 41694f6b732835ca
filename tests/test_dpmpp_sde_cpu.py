"""Host side of the DPM-Solver++(2M) SDE sampler (audioldm2_amd/dpm_solver.py: dpmpp_2m_sde_coefficients, DPMSolverSDESampler;
DESIGN.md 9l): the coefficient rows against a plain-Python-float restatement and the two identities that tie them to what is already
pinned (eta = 0: DPM-Solver++(2M)'s rows exactly; eta = 1, first order: DDIM's eta = 1 step), the sampler's surface and table, the
`sampler="dpmpp_2m_sde"` keyword through the pipeline, the ABI.  No kernel is launched here."""
import ctypes
import inspect
import math
import types

import numpy as np
import pytest
import torch

import dpmpp_sde as D


def grids():
    return [("S7", *D.project_grid(7)), ("S25", *D.project_grid(25)), ("S200", *D.project_grid(200)), ("uneven", *D.uneven_grid())]


GRIDS = grids()


# ---- coefficients -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,a_t,a_p", GRIDS, ids=[g[0] for g in GRIDS])
@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
def test_rows_match_the_plain_python_restatement(name, a_t, a_p, eta):
    from audioldm2_amd.dpm_solver import dpmpp_2m_sde_coefficients
    tab = dpmpp_2m_sde_coefficients(a_t, a_p, eta)
    n = len(a_t)
    assert tab.shape == (n, 6) and tab.dtype == np.float64
    ref = np.asarray(D.rows_py(a_t, a_p, eta))
    assert np.allclose(tab, ref, rtol=1e-12, atol=1e-300), float(np.abs(tab - ref).max())
    # the w rule: row 0, and the last row of a run under 15 steps
    assert tab[0, 4] == 0.0 and (tab[-1, 4] == 0.0) == (n < 15)
    if n > 2:
        assert (tab[1:-1, 4] > 0).all()


@pytest.mark.parametrize("name,a_t,a_p", GRIDS, ids=[g[0] for g in GRIDS])
def test_eta_zero_is_the_ode_solver_exactly(name, a_t, a_p):
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients, dpmpp_2m_sde_coefficients
    tab = dpmpp_2m_sde_coefficients(a_t, a_p, 0.0)
    assert np.array_equal(tab[:, :5], dpmpp_2m_coefficients(a_t, a_p))
    assert np.array_equal(tab[:, 5], np.zeros(len(a_t)))


@pytest.mark.parametrize("name,a_t,a_p", GRIDS, ids=[g[0] for g in GRIDS])
def test_eta_one_first_order_is_ddims_eta_one_step(name, a_t, a_p):
    """DDIM at eta = 1: sig = sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)), dir = sqrt(1 - a_prev - sig^2),
    x_prev = alpha_prev x0 + dir e + sig z with x0 = (x - sigma_t e) / alpha_t, so the coefficient of x is dir / sigma_t ... with w
    forced to 0 the row {c2, c3, c4} must be {dir / sigma_t, alpha_prev - alpha_t dir / sigma_t, sig}."""
    from audioldm2_amd.dpm_solver import dpmpp_2m_sde_coefficients
    tab = dpmpp_2m_sde_coefficients(a_t, a_p, 1.0)
    worst = 0.0
    for i in range(len(a_t)):
        at, ap = float(a_t[i]), float(a_p[i])
        sig = math.sqrt((1.0 - ap) / (1.0 - at) * (1.0 - at / ap))
        dirc = math.sqrt(1.0 - ap - sig * sig)
        ref = [dirc / math.sqrt(1.0 - at), math.sqrt(ap) - math.sqrt(at) * dirc / math.sqrt(1.0 - at), sig]
        worst = max(worst, max(abs(tab[i, c] - r) for c, r in zip((2, 3, 5), ref)))
    print(f"dpmpp sde eta=1 vs DDIM eta=1 [{name}]: max difference {worst:.1e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name,a_t,a_p", GRIDS, ids=[g[0] for g in GRIDS])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_first_order_step_is_a_member_of_the_ddim_family(name, a_t, a_p, eta):
    """For any eta: the coefficient of x0 sums to alpha_prev, and the coefficient of e and c4 share sigma_prev^2."""
    from audioldm2_amd.dpm_solver import dpmpp_2m_sde_coefficients
    tab = dpmpp_2m_sde_coefficients(a_t, a_p, eta)
    sg_t, al_t, c2, c3, c4 = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 5]
    assert np.abs(c2 * al_t + c3 - np.sqrt(a_p)).max() <= 1e-12
    assert np.abs((c2 * sg_t) ** 2 + c4 ** 2 - (1.0 - a_p)).max() <= 1e-12
    assert (c4 > 0).all() and (c2 > 0).all() and (c3 > 0).all()


def test_coefficients_refuse_bad_arguments():
    from audioldm2_amd.dpm_solver import dpmpp_2m_sde_coefficients
    with pytest.raises(ValueError, match="less noisy"):
        dpmpp_2m_sde_coefficients([0.5, 0.7], [0.6, 0.65], 1.0)
    for eta in (-0.1, 1.5, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="eta must be"):
            dpmpp_2m_sde_coefficients([0.5], [0.6], eta)
    assert dpmpp_2m_sde_coefficients([0.5], [0.6], 0).shape == (1, 6)      # the function accepts 0; the sampler does not


# ---- the sampler's surface ---------------------------------------------------------------------------------------------------------
def test_parameter_lists_are_dpm_solver_samplers():
    from audioldm2_amd.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    for name in ("__init__", "make_schedule", "sample", "dpm_sampling"):
        assert inspect.signature(getattr(DPMSolverSDESampler, name)) == inspect.signature(getattr(DPMSolverSampler, name)), name


@pytest.mark.parametrize("eta", [0, 0.0, -0.1, 1.5, float("nan")])
def test_make_schedule_refuses_eta_outside_its_interval(eta):
    from audioldm2_amd.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    s = DPMSolverSDESampler(D.ScheduleOnly())
    with pytest.raises(ValueError, match=r"DPM-Solver\+\+\(2M\) SDE needs 0 < ddim_eta <= 1; eta = 0 is sampler='dpmpp_2m'"):
        s.make_schedule(8, ddim_eta=eta, verbose=False)
    with pytest.raises(ValueError, match="needs 0 < ddim_eta <= 1"):
        s.sample(8, 1, (8, 4, 4), eta=eta, verbose=False)
    # ... and the deterministic class keeps refusing what is not 0
    with pytest.raises(ValueError, match="ddim_eta must equal 0"):
        DPMSolverSampler(D.ScheduleOnly()).make_schedule(8, ddim_eta=1.0, verbose=False)


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_table_is_guidance_tables_plus_c4_rounded_once(eta):
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler, dpmpp_2m_sde_coefficients
    from audioldm2_amd.sampling import guidance_table
    s = DPMSolverSDESampler(D.ScheduleOnly())
    s.make_schedule(20, ddim_eta=eta, verbose=False)
    a_t, a_p = D.project_grid(20)
    rows64 = dpmpp_2m_sde_coefficients(a_t, a_p, eta)
    assert s.dpm_coef.dtype == torch.float32 and torch.equal(s.dpm_coef, torch.from_numpy(rows64).float())
    for scale, cfg, phi in ((3.5, True, 0.0), (3.5, True, 0.7), (1.0, False, 0.0)):
        tab = s._coef_table(20, scale, cfg, phi)
        assert tab.shape == (20, 9) and tab.dtype == torch.float32 and tab.is_contiguous()
        assert torch.equal(tab[:, :8], guidance_table(torch.from_numpy(rows64[:, :5]).float(), scale, cfg, phi))
        assert torch.equal(tab[:, 8], torch.from_numpy(rows64[:, 5]).float())
    # a t_start sub-range is a run of its own: its own first and last row (first order), rounded once from ITS fp64 rows
    sub = s._coef_table(7, 3.5, True, 0.0)
    sub64 = dpmpp_2m_sde_coefficients(a_t[-7:], a_p[-7:], eta)
    assert sub.shape == (7, 9) and float(sub[0, 4]) == 0.0 and float(sub[-1, 4]) == 0.0
    assert torch.equal(sub[:, :5], torch.from_numpy(sub64[:, :5]).float()) and torch.equal(sub[:, 8], torch.from_numpy(sub64[:, 5]).float())
    assert float(s.dpm_coef[-7, 4]) != 0.0 and float(s.dpm_coef[-1, 4]) != 0.0      # the whole run's rows there are second order


def test_resample_is_refused_before_any_draw():
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    torch.manual_seed(3)
    state = torch.get_rng_state()
    mask, x0 = torch.ones(1, 8, 4, 4), torch.zeros(1, 8, 4, 4)
    with pytest.raises(ValueError, match=r"resample= \(resampled inpainting\) is DDIM's: the multistep history does not survive a jump"):
        DPMSolverSDESampler(D.ScheduleOnly()).sample(6, 1, (8, 4, 4), eta=1.0, verbose=False, mask=mask, x0=x0, resample=(2, 2))
    assert torch.equal(torch.get_rng_state(), state)


def test_unsupported_options_raise():
    from audioldm2_amd.dpm_solver import DPMSolverSDESampler
    s = DPMSolverSDESampler(D.ScheduleOnly())
    s.make_schedule(4, ddim_eta=1.0, verbose=False)
    for kw in ({"ddim_use_original_steps": True}, {"quantize_denoised": True}, {"score_corrector": object()}, {"noise_dropout": 0.1}):
        with pytest.raises(NotImplementedError, match=r"DPMSolverSDESampler\(HIP\)"):
            s.dpm_sampling(None, (1, 8, 4, 4), **kw)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
class FakeLD:
    from audioldm2_amd import pipeline as _P
    sample_log = _P.LatentDiffusion.sample_log
    latent_t_size, latent_f_size, channels, device = 8, 16, 8, "cpu"


def test_name_resolves_and_eta_one_travels_with_it():
    from audioldm2_amd import pipeline as P
    assert P.SAMPLERS == ("dpmpp_2m", "dpmpp_2m_sde")
    assert P.resolve_sampler("dpmpp_2m_sde") == "dpmpp_2m_sde"
    assert P._sampler_kwargs("dpmpp_2m_sde") == {"sampler": "dpmpp_2m_sde", "ddim_eta": 1.0}
    assert P._sampler_kwargs("dpmpp_2m_sde", "hiss", 0.7) == {"sampler": "dpmpp_2m_sde", "ddim_eta": 1.0, "negative_prompt": "hiss",
                                                             "guidance_rescale": 0.7}
    assert P._sampler_kwargs("dpmpp_2m") == {"sampler": "dpmpp_2m", "ddim_eta": 0.0} and P._sampler_kwargs(None) == {}
    with pytest.raises(ValueError, match="use_plms=True"):
        P.resolve_sampler("dpmpp_2m_sde", use_plms=True)
    with pytest.raises(ValueError, match="use_plms=True"):
        FakeLD().sample_log(None, 1, True, 4, use_plms=True, sampler="dpmpp_2m_sde")
    with pytest.raises(ValueError, match="sampler='dpmpp_2m_sde' needs ddim_steps"):
        FakeLD().sample_log(None, 1, False, None, sampler="dpmpp_2m_sde")


def test_sample_log_builds_the_class_and_forwards_the_keywords(monkeypatch):
    from audioldm2_amd import dpm_solver
    seen = []

    class S:
        def __init__(self, model, **kw):
            seen.append(("init", model))

        def sample(self, *a, **kw):
            seen.append((a, kw))
            return torch.zeros(1), None
    monkeypatch.setattr(dpm_solver, "DPMSolverSDESampler", S)     # looked up on the module at call time
    monkeypatch.setattr(dpm_solver, "DPMSolverSampler", None)
    ld = FakeLD()
    plan = types.SimpleNamespace(Tw=8, T=20, x0=None)
    xT = torch.zeros(1, 8, 8, 16)
    ld.sample_log(None, 1, True, 5, sampler="dpmpp_2m_sde", eta=0.5, guidance_rescale=0.7, unconditional_guidance_scale=3.5)
    ld.sample_log(None, 1, True, 5, sampler="dpmpp_2m_sde", eta=1.0, t_start=3, x_T=xT)
    ld.sample_log(None, 1, True, 5, sampler="dpmpp_2m_sde", eta=1.0, windows=plan)
    calls = [c for c in seen if c[0] != "init"]
    assert len(calls) == 3 and [c[0] for c in seen[::2]] == ["init"] * 3 and seen[0][1] is ld
    (a0, k0), (a1, k1), (a2, k2) = calls
    assert a0[:3] == (5, 1, (8, 8, 16)) and k0["eta"] == 0.5 and k0["guidance_rescale"] == 0.7
    assert k0["unconditional_guidance_scale"] == 3.5 and "t_start" not in k0 and "windows" not in k0 and "sampler" not in k0
    assert k1["t_start"] == 3 and k1["x_T"] is xT and "guidance_rescale" not in k1
    assert k2["windows"] is plan and a2[2] == (8, 20, 16)


def test_resample_with_the_name_is_refused_before_any_draw():
    from audioldm2_amd import pipeline as P
    torch.manual_seed(11)
    state = torch.get_rng_state()
    mask = torch.ones(1, 8, 8, 16)
    with pytest.raises(ValueError) as e:
        FakeLD().sample_log(None, 1, True, 6, sampler="dpmpp_2m_sde", eta=1.0, mask=mask, x0=torch.zeros(1, 8, 8, 16), resample=(2, 2))
    assert str(e.value) == P.RESAMPLE_MULTISTEP
    with pytest.raises(ValueError) as e:
        P.check_resample_job((2, 2), 6, "dpmpp_2m_sde", False, FakeLD())
    assert str(e.value) == P.RESAMPLE_MULTISTEP
    assert torch.equal(torch.get_rng_state(), state)


def test_no_signature_changed():
    from audioldm2_amd import pipeline as P
    LD = P.LatentDiffusion
    for f in (LD.sample_log, LD.generate_batch, LD.generate_batch_masked, LD.generate_batch_from_audio):
        assert "sampler" not in inspect.signature(f).parameters
    for f in (P.text_to_audio, P.super_resolution_and_inpainting, P.audio_to_audio):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "sampler" and last.default is None
    for f in (LD.generate_batch_long, LD.generate_batch_long_from_audio, P.text_to_audio_long, P.extend_audio):
        assert inspect.signature(f).parameters["sampler"].default is None


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 26      # the entry point arrived with ABI 26
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    assert "aldm_dpmpp_sde_step_indexed" in lib.EXPORTED_SYMBOLS and hasattr(l, "aldm_dpmpp_sde_step_indexed")


def test_entry_validates_before_launch():
    """aldm_dpmpp_sde_step_indexed refuses null pointers, n <= 0, noise_rows < 1, rows of fewer than nine floats and an x or x0_buf
    inside the noise table before any launch: observable without a GPU (the pointers are never dereferenced)."""
    from audioldm2_amd import lib
    l = lib.load()
    p = lambda a: ctypes.c_void_p(a)
    x, eps, slab, tab, coef, idx = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 29
    n, rows = 64, 3
    good = [p(x), p(eps), p(slab), p(tab), rows, p(coef), p(idx), n, 9]
    for k in (0, 1, 2, 3, 5, 6):
        args = list(good)
        args[k] = None
        assert l.aldm_dpmpp_sde_step_indexed(*args, None) != 0, k
        assert "null pointer" in l.aldm_last_error().decode(), k

    def refused(msg, **kw):
        a = dict(x=p(x), eps=p(eps), slab=p(slab), tab=p(tab), rows=rows, coef=p(coef), idx=p(idx), n=n, ld=9)
        a.update(kw)
        assert l.aldm_dpmpp_sde_step_indexed(a["x"], a["eps"], a["slab"], a["tab"], a["rows"], a["coef"], a["idx"], a["n"], a["ld"],
                                             None) != 0, kw
        assert msg in l.aldm_last_error().decode(), (kw, l.aldm_last_error())
    refused("n=0", n=0)
    refused("n=-4", n=-4)
    refused("noise_rows=0", rows=0)
    refused("noise_rows=-1", rows=-1)
    refused("coef_ld=8", ld=8)
    end = tab + 4 * n * rows      # one past the table's last byte
    for at in (tab, tab + 4 * (n - 1), tab - 4 * (n - 1), tab + 4 * n, end - 4):
        refused("x overlaps noise_tab", x=p(at))
        refused("x0_buf overlaps noise_tab", slab=p(at))
    with pytest.raises(RuntimeError, match="x0_buf overlaps noise_tab"):
        lib.check(1, "dpmpp_sde_step_indexed")
