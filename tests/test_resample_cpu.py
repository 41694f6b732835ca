"""CPU tests of resampled inpainting (RePaint's jumps): the visit schedule against the issue's table, an independent
restatement of the published schedule and position arithmetic; the forward jump's coefficients against a literal fp64 restatement;
every refusal, before any draw; the ABI.  (No kernel is launched here.)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import audio2audio as A
import resample as Rs


# ---- the visit schedule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(Rs.VISIT_TABLE), ids=str)
def test_visits_reproduce_the_table_literally(key):
    from audioldm2_amd.sampling import resample_visits
    v = resample_visits(*key)
    assert isinstance(v, tuple) and Rs.show(v) == Rs.VISIT_TABLE[key] and len(v) == Rs.VISIT_COUNTS[key]
    assert all(e == ("step", e[1]) or e == ("renoise", e[1], e[2]) for e in v)


def test_n_equal_one_has_no_renoise():
    from audioldm2_amd.sampling import resample_visits
    assert resample_visits(6, 1, 2) == tuple(("step", i) for i in range(6))


@pytest.mark.parametrize("key", list(Rs.LARGE_COUNTS), ids=str)
def test_visit_counts_of_the_published_settings(key):
    from audioldm2_amd.sampling import resample_visits
    v = resample_visits(*key)
    assert (sum(e[0] == "step" for e in v), sum(e[0] == "renoise" for e in v)) == Rs.LARGE_COUNTS[key]


def test_visits_on_a_grid_are_position_arithmetic_and_the_published_schedule():
    from audioldm2_amd.sampling import resample_visits
    assert len(Rs.GRID) > 60
    for S, n, jump in Rs.GRID:
        v = resample_visits(S, n, jump)
        points = Rs.jump_points(S, jump)
        pos, used = 0, {}
        for e in v:
            if e[0] == "step":
                assert e[1] == pos and 0 <= e[1] < S, (S, n, jump, e)      # loop step i starts at position i
                pos += 1
            else:
                _, k, k_to = e
                assert k == pos and k in points and k_to == k - jump, (S, n, jump, e)
                used[k] = used.get(k, 0) + 1
                pos = k_to
        assert pos == S, (S, n, jump)
        assert used == ({k: n - 1 for k in points} if n > 1 else {}), (S, n, jump)
        assert sum(e[0] == "step" for e in v) == S + (n - 1) * jump * len(points)
        assert v[0] == ("step", 0) and v[-1] == ("step", S - 1)
        assert v == Rs.published_visits(S, n, jump), (S, n, jump)


@pytest.mark.parametrize("args,msg", [((6, 2.0, 2), "pair of integers"), ((6, 2, 2.0), "pair of integers"), ((6, True, 2), "pair of integers"),
                                      ((6, 2, False), "pair of integers"), ((6, "2", 2), "pair of integers"), ((6, None, 2), "pair of integers"),
                                      ((6, 0, 2), "n .* must be >= 1"), ((6, -1, 2), "n .* must be >= 1"), ((6, 2, 0), "jump must lie in"),
                                      ((6, 2, -2), "jump must lie in"), ((6, 2, 6), r"jump must lie in \[1, 5\]"),
                                      ((6, 2, 7), "no jump point"), ((1, 2, 1), "jump must lie in"), ((6, 1, 6), "jump must lie in")])
def test_visits_refusals(args, msg):
    from audioldm2_amd.sampling import resample_visits
    with pytest.raises(ValueError, match=msg):
        resample_visits(*args)


def test_numpy_integers_are_integers():
    from audioldm2_amd.sampling import resample_visits
    assert resample_visits(np.int64(6), np.int32(2), np.int64(2)) == resample_visits(6, 2, 2)


# ---- the forward jump's coefficients ------------------------------------------------------------------------------------------------
def test_coefficients_match_the_fp64_restatement_within_one_ulp():
    """The restatement starts where the product starts — the model's fp32 schedule — and is literal from there: abar at a position
    from the uniform grid, rho, two square roots, in fp64.  (From the fp64 schedule c1 = sqrt(1 - rho) would differ by the fp32
    rounding of the schedule itself, amplified by 1 / (1 - rho): not the function's error.)"""
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.sampling import renoise_coef, resample_visits
    s = DDIMSampler(Rs.ScheduleModel())
    worst = 0.0
    for ddim_steps, S, n, jump in ((200, 200, 2, 10), (200, 200, 2, 1), (50, 50, 2, 10), (6, 6, 2, 2), (200, 60, 2, 7), (7, 5, 3, 2)):
        s.make_schedule(ddim_steps, verbose=False)
        assert len(s.ddim_timesteps) >= S
        seen_final = False
        for v in resample_visits(S, n, jump):
            if v[0] != "renoise":
                continue
            c0, c1 = renoise_coef(s.ddim_alphas, s.ddim_alphas_prev, S, v[1], v[2])
            assert isinstance(c0, float) and isinstance(c1, float) and 0.0 < c1 < 1.0 and 0.0 < c0 < 1.0
            r0, r1 = Rs.coef_fp64(ddim_steps, S, v[1], v[2])
            worst = max(worst, A.ulps_fp32(c0, r0), A.ulps_fp32(c1, r1))
            f0, f1 = float(np.float32(c0)), float(np.float32(c1))
            assert abs(f0 * f0 + f1 * f1 - 1.0) <= 2.0 ** -22, (ddim_steps, S, v)
            if v[1] == S:
                # the final position is at ddim_alphas_prev[0] = abar[0], not at any entry of ddim_alphas
                rho = float(s.ddim_alphas[jump - 1]) / float(s.ddim_alphas_prev[0])
                assert abs(c0 - np.sqrt(rho)) < 1e-12 and float(s.ddim_alphas_prev[0]) == float(s.alphas_cumprod[0])
                seen_final = True
        assert seen_final
    print(f"renoise_coef vs fp64: worst {worst:.3f} fp32 ulp")
    assert worst <= 1.0
    with pytest.raises(ValueError, match="0 <= k_to < k <= S"):
        renoise_coef(s.ddim_alphas, s.ddim_alphas_prev, 5, 2, 2)
    with pytest.raises(ValueError, match="0 <= k_to < k <= S"):
        renoise_coef(s.ddim_alphas, s.ddim_alphas_prev, 5, 6, 2)


# ---- refusals, before any draw ------------------------------------------------------------------------------------------------------
class _NoGpu:
    """Stands where a LatentDiffusion would: what the entry points read before they touch the GPU; anything else raises."""
    latent_t_size, latent_t_per_second, first_stage_key, num_timesteps = 256, 25.6, "fbank", 1000

    class first_stage_model:
        class encoder:
            num_resolutions = 3

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the arguments were checked")


def _ld_stub():
    from audioldm2_amd.pipeline import LatentDiffusion

    class Stub(_NoGpu):
        pass
    for name in ("long_form_plans", "generate_batch_long_from_audio", "generate_batch_masked", "sample_log", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(Stub, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return Stub()


BAD_PAIRS = [(3, "pair"), ((2,), "pair"), ((2, 2, 2), "pair"), ("22", "pair"), ((2.0, 2), "pair of integers"), ((2, True), "pair of integers"),
             ((0, 2), "must be >= 1"), ((2, 0), "jump must lie in")]


def test_entry_points_refuse_before_any_draw_or_gpu_work():
    from audioldm2_amd.pipeline import extend_audio, make_batch_for_text_to_audio
    ld = _ld_stub()
    wav = np.zeros(16000, dtype=np.float32)
    batch = make_batch_for_text_to_audio("rain")
    torch.manual_seed(5)
    state = torch.get_rng_state()
    jobs = {
        "extend_audio": lambda **kw: extend_audio(ld, "rain", wav, 30, **kw),
        "long_from_audio": lambda **kw: ld.generate_batch_long_from_audio(batch, 768, [(0, 200)], **kw),
        "masked": lambda **kw: ld.generate_batch_masked(batch, **kw),
    }
    for name, job in jobs.items():
        for bad, msg in BAD_PAIRS:
            with pytest.raises(ValueError, match=msg):
                job(resample=bad)
        with pytest.raises(ValueError, match=r"jump must lie in \[1, 199\]"):
            job(resample=(2, 200))                                   # ddim_steps = 200: jump >= the number of steps
        with pytest.raises(ValueError, match=r"jump must lie in \[1, 6\]"):
            job(resample=(2, 7), ddim_steps=6)                       # the uniform grid of "6 steps" has 7 entries: 0, 166, ..., 996
        with pytest.raises(ValueError, match="multistep history .* does not survive a jump"):
            job(resample=(2, 2), sampler="dpmpp_2m")
    for name in ("long_from_audio", "masked"):
        with pytest.raises(ValueError, match="multistep history .* does not survive a jump"):
            jobs[name](resample=(2, 2), use_plms=True)
    with pytest.raises(ValueError, match="resample= needs ddim_steps"):
        ld.generate_batch_masked(batch, ddim_steps=None, resample=(2, 2))
    # sample_log: the keyword goes to DDIM only, and needs a region to keep
    mask = torch.ones(1, 1, 16, 8)
    for kw, msg in ((dict(ddim=True), "something to harmonise with"), (dict(ddim=True, mask=mask, use_plms=True), "multistep history"),
                    (dict(ddim=True, mask=mask, sampler="dpmpp_2m"), "multistep history"),
                    (dict(ddim=False, mask=mask), "resample= needs ddim_steps"), (dict(ddim=True, mask=mask, resample=(2, 0)), "jump must lie in"),
                    (dict(ddim=True, mask=mask, resample=7), "pair")):
        with pytest.raises(ValueError, match=msg):
            ld.sample_log(None, 1, ddim_steps=6, **dict(dict(resample=(2, 2)), **kw))
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn
    assert ld.latent_t_size == 256


def test_samplers_refuse_before_any_draw():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    m = Rs.ScheduleModel()
    mask, x0 = torch.ones(1, 1, 16, 1), torch.zeros(A.TINY_SHAPE)
    torch.manual_seed(6)
    state = torch.get_rng_state()

    def ddim(**kw):
        args = dict(dict(S=5, batch_size=2, shape=A.TINY_SHAPE[1:], verbose=False, mask=mask, x0=x0, resample=(2, 2)), **kw)
        return DDIMSampler(m).sample(**args)
    with pytest.raises(ValueError, match="something to harmonise with"):
        ddim(mask=None, x0=None)
    with pytest.raises(ValueError, match="something to harmonise with"):
        ddim(mask=None, x0=None, resample=(1, 2))
    with pytest.raises(ValueError, match="temperature == 1.0"):
        ddim(temperature=0.5)
    for bad, msg in BAD_PAIRS:
        with pytest.raises(ValueError, match=msg):
            ddim(resample=bad)
    with pytest.raises(ValueError, match=r"jump must lie in \[1, 4\]"):
        ddim(resample=(2, 5))
    with pytest.raises(ValueError, match=r"jump must lie in \[1, 4\]"):
        ddim(resample=(1, 5))                                        # n = 1 is the plain run, but the pair is still checked
    with pytest.raises(ValueError, match=r"jump must lie in \[1, 2\]"):
        ddim(resample=(2, 3), t_start=3, x_T=torch.zeros(A.TINY_SHAPE))      # against the CUT schedule
    s = DDIMSampler(m)
    s.make_schedule(6, verbose=False)
    with pytest.raises(ValueError, match="something to harmonise with"):
        s.ddim_sampling(None, A.TINY_SHAPE, resample=(2, 2))
    with pytest.raises(ValueError, match="temperature == 1.0"):
        s.ddim_sampling(None, A.TINY_SHAPE, mask=mask, x0=x0, temperature=2.0, resample=(2, 2))
    for cls in (PLMSSampler, DPMSolverSampler):
        with pytest.raises(ValueError, match="multistep history does not survive a jump"):
            cls(m).sample(6, 2, A.TINY_SHAPE[1:], verbose=False, mask=mask, x0=x0, resample=(2, 2))
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn


# ---- the ABI and the signatures ----------------------------------------------------------------------------------------------------
def test_abi_version_symbol_and_signatures():
    from audioldm2_amd import lib
    from audioldm2_amd.pipeline import LatentDiffusion, extend_audio
    assert lib.ABI_VERSION >= 23
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    assert "aldm_renoise_indexed" in lib.EXPORTED_SYMBOLS and hasattr(l, "aldm_renoise_indexed")
    for fn in (extend_audio, LatentDiffusion.generate_batch_long_from_audio):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "resample" and last.default is None, fn


def test_entry_validates_before_launch():
    """aldm_renoise_indexed refuses null pointers, n <= 0, rows of fewer than two coefficients and an x inside the noise table's
    first row before any launch: observable without a GPU (the pointers are never dereferenced)."""
    from audioldm2_amd import lib
    l = lib.load()
    p = lambda a: ctypes.c_void_p(a)
    x, tab, coef = 1 << 20, 1 << 24, 1 << 28
    for args, msg in (((None, p(tab), p(coef), None, 64, 8), "null pointer"), ((p(x), None, p(coef), None, 64, 8), "null pointer"),
                      ((p(x), p(tab), None, None, 64, 8), "null pointer"), ((p(x), p(tab), p(coef), None, 0, 8), "bad args"),
                      ((p(x), p(tab), p(coef), None, -4, 8), "bad args"), ((p(x), p(tab), p(coef), None, 64, 1), "bad args"),
                      ((p(tab), p(tab), p(coef), None, 64, 8), "x overlaps noise_tab"),
                      ((p(tab + 4 * 63), p(tab), p(coef), None, 64, 8), "x overlaps noise_tab"),
                      ((p(tab - 4 * 63), p(tab), p(coef), None, 64, 8), "x overlaps noise_tab")):
        assert l.aldm_renoise_indexed(*args, None) != 0, args
        assert msg in l.aldm_last_error().decode(), (args, l.aldm_last_error())
