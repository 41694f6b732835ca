"""Host side of the DPM-Solver++(2M) sampler (audioldm2_amd/dpm_solver.py): the coefficient table against its formulas, the order
of convergence of the table-driven update on an analytic model, the refusals, the `sampler=` keyword, the ABI.  No kernel is
launched here.

The analytic model: data N(0, V) per element with V = 0.25, so eps(x, abar) = sqrt(1 - abar) x / (V abar + 1 - abar) and the
probability-flow solution keeps x / sqrt(V abar + 1 - abar) constant.  Every loop below runs in numpy fp64 on the fp64 table.
Measured (end-point error ratio when the step count doubles, uniform grid in log-SNR from -3 to 3): 2M 3.92 (32 -> 64) and 3.97
(64 -> 128); the same loop with w forced to 0 (first order = DDIM) 1.98 and 1.99.  The bars (>= 3.5, <= 2.2) separate order 2
(ratio -> 4) from order 1 (ratio -> 2)."""
import ctypes
import types

import numpy as np
import pytest
import torch

V = 0.25
EPS32 = 2.0 ** -24


class _ScheduleOnly:
    """What make_schedule reads on its model."""
    num_timesteps = 1000
    alphas_cumprod = torch.cumprod(1.0 - torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2, 0).float()


def formulas(a_t, a_p):
    """The issue's formulas in fp64, step by step (no vector code shared with the builder)."""
    rows, h_last = [], None
    S = len(a_t)
    for i in range(S):
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t[i]), np.sqrt(1 - a_t[i]), np.sqrt(a_p[i]), np.sqrt(1 - a_p[i])
        h = np.log(al_p / sg_p) - np.log(al_t / sg_t)
        first = i == 0 or (i == S - 1 and S < 15)
        w = 0.0 if first else 1.0 / (2.0 * (h_last / h))
        rows.append([sg_t, al_t, sg_p / sg_t, -al_p * np.expm1(-h), w])
        h_last = h
    return np.asarray(rows)


def project_grid(S):
    """abar_t / abar_prev of the project's `uniform` grid in step order (noisiest first), as DPMSolverSampler uses them."""
    from audioldm2_amd.ddim import make_ddim_timesteps
    ac = _ScheduleOnly.alphas_cumprod.double().numpy()
    ts = make_ddim_timesteps("uniform", S, 1000, verbose=False)
    a = ac[ts]
    a_prev = np.concatenate([ac[:1], ac[ts[:-1]]])
    return a[::-1].copy(), a_prev[::-1].copy()


def lambda_grid(S, lo=-3.0, hi=3.0):
    lam = np.linspace(lo, hi, S + 1)
    abar = 1.0 / (1.0 + np.exp(-2.0 * lam))       # lambda = log(alpha / sigma) = 0.5 log(abar / (1 - abar))
    return abar[:-1], abar[1:]


def run_table(tab, a_t, a_p, first_order=False):
    """The update of the kernel, driven by the table, on the analytic model; returns |x_end - exact| / |exact|."""
    x = np.asarray([1.0, -0.7, 2.3])
    exact = x * np.sqrt((V * a_p[-1] + 1 - a_p[-1]) / (V * a_t[0] + 1 - a_t[0]))
    x0_last = np.full_like(x, np.nan)
    for i, (c0, c1, c2, c3, w) in enumerate(tab):
        e = np.sqrt(1 - a_t[i]) * x / (V * a_t[i] + 1 - a_t[i])
        x0 = (x - c0 * e) / c1
        d = x0 if (w == 0 or first_order) else x0 + w * (x0 - x0_last)
        x = c2 * x + c3 * d
        x0_last = x0
    assert np.isfinite(x).all()
    return float(np.abs(x - exact).max() / np.abs(exact).max())


@pytest.mark.parametrize("S", [1, 2, 6, 14, 15, 50])
def test_table_matches_the_formulas(S):
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    a_t, a_p = project_grid(S)
    tab = dpmpp_2m_coefficients(a_t, a_p)
    n = len(a_t)
    assert tab.shape == (n, 5) and tab.dtype == np.float64
    ref = formulas(a_t, a_p)
    assert np.allclose(tab, ref, rtol=1e-12, atol=0.0)
    assert tab[0, 4] == 0.0
    assert (tab[-1, 4] == 0.0) == (n < 15)
    if n > 2:
        assert (tab[1:-1, 4] > 0).all()
    assert (tab[:, 3] > 0).all() and (tab[:, 2] > 0).all() and (tab[:, 2] < 1).all()


def test_last_row_order_switches_at_fifteen_steps():
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    for S in (14, 15):
        tab = dpmpp_2m_coefficients(*lambda_grid(S))
        assert (tab[-1, 4] == 0.0) == (S < 15), S
        assert tab[0, 4] == 0.0
        assert np.allclose(tab[1:S - 1, 4], 0.5)    # uniform in lambda: r = 1


def test_refuses_a_step_towards_more_noise():
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    with pytest.raises(ValueError, match="less noisy"):
        dpmpp_2m_coefficients([0.5, 0.7], [0.6, 0.65])


def test_first_order_rows_are_ddims_eta0_coefficients():
    """x_prev = A x + B e.  DDIM (ddim_coef row {c0..c3}): A = c3 / c1, B = c2 - c3 c0 / c1.  A first-order 2M row {t0..t3}:
    A = t2 + t3 / t1, B = -t3 t0 / t1.  Both from fp32 tables, evaluated here in fp64; every term carries at most four fp32
    roundings on either side (value, square root, quotient or product of rounded values), so the two agree within 8 * 2^-24 of the
    sum of the term magnitudes."""
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    d, s = DDIMSampler(_ScheduleOnly(), device="cpu"), DPMSolverSampler(_ScheduleOnly())
    for S in (1, 2, 6, 12):
        d.make_schedule(S, ddim_eta=0.0, verbose=False)
        s.make_schedule(S, ddim_eta=0.0, verbose=False)
        n = len(s.ddim_timesteps)
        assert s.dpm_coef.shape == (n, 5) and s.dpm_coef.dtype == torch.float32
        first = [i for i in range(n) if float(s.dpm_coef[i, 4]) == 0.0]
        assert first == sorted({0, n - 1})
        for i in first:
            c = d.ddim_coef[n - 1 - i].double().numpy()
            t = s.dpm_coef[i].double().numpy()
            A_d, B_d = c[3] / c[1], c[2] - c[3] * c[0] / c[1]
            A_s, B_s = t[2] + t[3] / t[1], -t[3] * t[0] / t[1]
            assert abs(A_d - A_s) <= 8 * EPS32 * (abs(t[2]) + abs(t[3] / t[1]) + abs(A_d)), (S, i)
            assert abs(B_d - B_s) <= 8 * EPS32 * (abs(c[2]) + abs(c[3] * c[0] / c[1]) + abs(B_s)), (S, i)


def test_table_is_rounded_once_from_fp64():
    from audioldm2_amd.dpm_solver import DPMSolverSampler, dpmpp_2m_coefficients
    s = DPMSolverSampler(_ScheduleOnly())
    s.make_schedule(20, verbose=False)
    a_t, a_p = project_grid(20)
    assert torch.equal(s.dpm_coef, torch.from_numpy(dpmpp_2m_coefficients(a_t, a_p)).float())
    assert torch.equal(s._table(7), torch.from_numpy(dpmpp_2m_coefficients(a_t[-7:], a_p[-7:])).float())   # a `timesteps` sub-range


def test_second_order_convergence_on_the_uniform_lambda_grid():
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    err2, err1 = {}, {}
    for S in (32, 64, 128):
        a_t, a_p = lambda_grid(S)
        tab = dpmpp_2m_coefficients(a_t, a_p)
        err2[S] = run_table(tab, a_t, a_p)
        err1[S] = run_table(tab, a_t, a_p, first_order=True)
    r2 = [err2[32] / err2[64], err2[64] / err2[128]]
    r1 = [err1[32] / err1[64], err1[64] / err1[128]]
    print(f"dpmpp 2M error {err2}  ratios {r2[0]:.2f} {r2[1]:.2f};  first order {err1}  ratios {r1[0]:.2f} {r1[1]:.2f}")
    assert min(r2) >= 3.5
    assert max(r1) <= 2.2


@pytest.mark.parametrize("S", [20, 50, 200])
def test_beats_first_order_on_the_projects_uniform_grid(S):
    from audioldm2_amd.dpm_solver import dpmpp_2m_coefficients
    a_t, a_p = project_grid(S)
    tab = dpmpp_2m_coefficients(a_t, a_p)
    e2, e1 = run_table(tab, a_t, a_p), run_table(tab, a_t, a_p, first_order=True)
    print(f"dpmpp uniform grid S={S}: 2M {e2:.2e}  first order {e1:.2e}")
    assert e2 < e1


def test_make_schedule_refuses_nonzero_eta_and_sample_passes_it_on():
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_ScheduleOnly())
    with pytest.raises(ValueError, match="ddim_eta must equal 0"):
        s.make_schedule(8, ddim_eta=0.5)
    with pytest.raises(ValueError, match="ddim_eta must equal 0"):
        s.sample(8, 1, (8, 4, 4), eta=0.5, verbose=False)
    s.make_schedule(8, ddim_eta=0.0)
    assert float(s.ddim_sigmas.abs().max()) == 0.0


def test_unsupported_options_raise():
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_ScheduleOnly())
    s.make_schedule(4)
    for kw in ({"ddim_use_original_steps": True}, {"quantize_denoised": True}, {"score_corrector": object()},
               {"noise_dropout": 0.1}):
        with pytest.raises(NotImplementedError, match=r"DPMSolverSampler\(HIP\)"):
            s.dpm_sampling(None, (1, 8, 4, 4), **kw)
    with pytest.raises(NotImplementedError, match=r"DPMSolverSampler\(HIP\)"):
        s.sample(4, 1, (8, 4, 4), quantize_x0=True, verbose=False)


def test_parameter_lists_are_plms_samplers():
    import inspect
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    for ours, theirs in (("__init__", "__init__"), ("make_schedule", "make_schedule"), ("sample", "sample"),
                         ("dpm_sampling", "plms_sampling")):
        assert inspect.signature(getattr(DPMSolverSampler, ours)) == inspect.signature(getattr(PLMSSampler, theirs)), ours


def test_sampler_keyword_is_validated_before_any_work():
    """An unknown name and `sampler=` next to use_plms=True raise ValueError at the top of every entry: nothing of `self` or of
    the batch is touched before (an empty namespace stands in for the model)."""
    import inspect
    from audioldm2_amd import pipeline
    LD = pipeline.LatentDiffusion
    stub = types.SimpleNamespace()
    assert pipeline.resolve_sampler(None) is None and pipeline.resolve_sampler(None, use_plms=True) is None
    assert pipeline.resolve_sampler("dpmpp_2m") == "dpmpp_2m"
    for call in (lambda **kw: pipeline.resolve_sampler(kw["sampler"], kw.get("use_plms", False)),
                 lambda **kw: LD.sample_log(stub, None, 1, True, 4, **kw),
                 lambda **kw: LD.generate_batch(stub, {}, ddim_steps=4, ddim_eta=0.0, **kw),
                 lambda **kw: LD.generate_batch_masked(stub, {}, ddim_steps=4, ddim_eta=0.0, **kw)):
        with pytest.raises(ValueError, match="unknown sampler 'heun'"):
            call(sampler="heun")
        with pytest.raises(ValueError, match="use_plms=True"):
            call(sampler="dpmpp_2m", use_plms=True)
    with pytest.raises(ValueError, match="unknown sampler"):
        pipeline.text_to_audio(stub, "a dog", sampler="heun")
    with pytest.raises(ValueError, match="unknown sampler"):
        pipeline.super_resolution_and_inpainting(stub, "a dog", original_audio_file_path=None, duration=10, sampler="heun")
    # the signatures of the three methods are unchanged; the two entry points gain a trailing sampler=None
    for f in (LD.sample_log, LD.generate_batch, LD.generate_batch_masked):
        assert "sampler" not in inspect.signature(f).parameters
    for f in (pipeline.text_to_audio, pipeline.super_resolution_and_inpainting):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "sampler" and last.default is None


def test_abi_version_and_entry_point_validation():
    """aldm_dpmpp_step_indexed refuses null pointers, n <= 0 and rows shorter than 7 floats before any launch."""
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 12   # the entry point arrived with ABI 12
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION and "aldm_dpmpp_step_indexed" in lib.EXPORTED_SYMBOLS
    p = ctypes.c_void_p(4096)   # never dereferenced: validation fails first
    for k in range(5):
        args = [p, p, p, p, p]
        args[k] = None
        assert l.aldm_dpmpp_step_indexed(*args, 1024, 8, None) != 0
        assert "null pointer" in l.aldm_last_error().decode()
    assert l.aldm_dpmpp_step_indexed(p, p, p, p, p, 1024, 6, None) != 0
    assert "coef_ld=6" in l.aldm_last_error().decode()
    with pytest.raises(RuntimeError, match="coef_ld=6"):
        lib.check(1, "dpmpp_step_indexed")
    assert l.aldm_dpmpp_step_indexed(p, p, p, p, p, 0, 8, None) != 0
    assert "n=0" in l.aldm_last_error().decode()
