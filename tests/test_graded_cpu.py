"""CPU tests of graded keep levels (differential diffusion): windows.keep_levels and sampling.keep_thresholds /
hold_steps against the issue's tables and a literal loop; keep_frames with triples; every refusal, before any draw; the ABI.  (No
kernel is launched here.)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import audio2audio as A
import graded as G
import resample as Rs


# ---- levels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,want", G.LEVEL_TABLE, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_keep_levels_reproduce_the_table_exactly(args, want):
    from audioldm2_amd.windows import keep_levels
    T, intervals, feather, ring = args
    lv = keep_levels(T, intervals, feather, ring=ring)
    assert lv.dtype == torch.float32 and tuple(lv.shape) == (T,)
    assert lv.tolist() == [float(v) for v in want]


def test_levels_of_one_without_feather_are_keep_mask():
    from audioldm2_amd.windows import keep_levels, keep_mask
    for T, ivs in ((12, [(2, 5)]), (16, [(0, 5), (5, 9), (12, 16)]), (8, []), (40, [(0, 13), (29, 33)])):
        assert torch.equal(keep_levels(T, ivs), keep_mask(T, ivs))
        assert torch.equal(keep_levels(T, [iv + (1.0,) for iv in ivs], 0, ring=True), keep_mask(T, ivs))
        assert torch.equal(keep_levels(T, [(np.int64(a), np.int32(b), np.float32(1)) for a, b in ivs], np.int64(0)), keep_mask(T, ivs))


def test_feathered_levels_on_a_ring_are_invariant_under_rotation():
    """Round the circle the distances do not know where frame 0 is: rotating the intervals rotates the levels."""
    from audioldm2_amd.windows import keep_levels
    T = 24
    base = keep_levels(T, [(3, 7), (12, 15, .5)], 4, ring=True)
    for shift in (1, 5, 9):
        assert torch.equal(keep_levels(T, [(3 + shift, 7 + shift), (12 + shift, 15 + shift, .5)], 4, ring=True), base.roll(shift))
    # a fade crosses the junction: frame 17 is 3 frames from [20, 24) either way round, frame 3 only round the circle
    wrapped, linear = keep_levels(T, [(20, 24)], 4, ring=True), keep_levels(T, [(20, 24)], 4)
    assert wrapped[17] == linear[17] == np.float32(1 - 3 / 5) and wrapped[3] == np.float32(1 - 4 / 5) and linear[3] == 0.0
    assert wrapped[0] == np.float32(1 - 1 / 5) and torch.equal(wrapped[4:], linear[4:])
    # inside an interval the value is its level, whatever a neighbour's fade would give
    assert keep_levels(T, [(0, 2, .5), (20, 24)], 4, ring=True)[:2].tolist() == [.5, .5]


@pytest.mark.parametrize("args,msg", [
    ((12, [(2, 5, 0.0)]), "level"), ((12, [(2, 5, -.5)]), "level"), ((12, [(2, 5, 1.5)]), "level"), ((12, [(2, 5, float("nan"))]), "level"),
    ((12, [(2, 5, float("inf"))]), "level"), ((12, [(2, 5, True)]), "level"), ((12, [(2, 5, "1")]), "level"), ((12, [(2, 5, None)]), "level"),
    ((12, [(2, 5, .5, 1)]), "interval must be"), ((12, [(2,)]), "interval must be"), ((12, [7]), "interval must be"),
    ((12, [(2.0, 5)]), "integers"), ((12, [(True, 5)]), "integers"), ((12, [(5, 5)]), "empty"), ((12, [(2, 13)]), "leaves"),
    ((12, [(-1, 3)]), "leaves"), ((12, [(2, 6), (5, 8, .5)]), "ordered"), ((12, [(6, 8), (2, 4)]), "ordered"),
    ((12, [(2, 5)], -1), "feather"), ((12, [(2, 5)], 12), "feather"), ((12, [(2, 5)], 1.0), "feather"), ((12, [(2, 5)], True), "feather"),
    ((12, [(2, 5)], None), "feather")])
def test_keep_levels_refusals(args, msg):
    from audioldm2_amd.windows import keep_levels
    with pytest.raises(ValueError, match=msg):
        keep_levels(*args)


# ---- thresholds and what a level means -----------------------------------------------------------------------------------------------
def test_thresholds_are_i_over_S_rounded_once():
    from audioldm2_amd.sampling import keep_thresholds, resample_visits
    for S in (1, 2, 3, 6, 7, 50, 200):
        thr = keep_thresholds(S)
        assert thr.dtype == torch.float32 and tuple(thr.shape) == (S,)
        assert thr.tolist() == [float(np.float32(np.float64(i) / np.float64(S))) for i in range(S)]
        assert thr[0] == 0.0 and float(thr[-1]) < 1.0 and bool((thr[1:] > thr[:-1]).all())
    per_visit = keep_thresholds(6, resample_visits(6, 2, 2))
    assert per_visit.tolist() == [float(np.float32(k / 6.0)) for k in G.THRESHOLD_NUMERATORS_6_2_2]
    assert torch.equal(keep_thresholds(6, resample_visits(6, 1, 2)), keep_thresholds(6))
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="positive integer number of steps"):
            keep_thresholds(bad)


@pytest.mark.parametrize("level,S,want", G.HOLD_TABLE)
def test_hold_steps_table(level, S, want):
    from audioldm2_amd.sampling import hold_steps
    assert hold_steps(level, S) == want


def test_hold_steps_agree_with_the_literal_loop_on_a_grid():
    from audioldm2_amd.sampling import hold_steps, keep_thresholds
    assert len(G.HOLD_GRID) == 54
    for S, level in G.HOLD_GRID:
        got = hold_steps(level, S)
        assert got == G.hold_steps_literal(level, S), (S, level)
        # the held steps are the run's first ones: the per-step masks of a frame are 1 ... 1 0 ... 0
        held = (np.float32(level) > keep_thresholds(S).numpy()).tolist()
        assert held == [True] * got + [False] * (S - got)
    assert all(hold_steps(1.0, S) == S and hold_steps(0.0, S) == 0 for S in (1, 2, 6, 200))


# ---- keep_frames ----------------------------------------------------------------------------------------------------------------------
def test_keep_frames_passes_a_level_through_and_leaves_pairs_pairs():
    from audioldm2_amd.pipeline import keep_frames
    assert keep_frames([(0.0, 6.0)], 25.6, 384) == [(0, 153)]
    assert keep_frames([(0.0, 4.0), (4.0, 6.0, 0.5)], 25.6, 384) == [(0, 102), (103, 153, 0.5)]
    assert keep_frames([[0, 5, 1]], 25.6, 384) == [(0, 128, 1)]
    assert keep_frames([(2.0, 100.0, .25)], 25.6, 384) == [(52, 384, .25)]
    for bad in ([(0.0, 1.0, .5, 2)], [(0.0,)], [3.0], [("a", 1.0, .5)], [(0.0, float("inf"), .5)]):
        with pytest.raises(ValueError, match="keep: "):
            keep_frames(bad, 25.6, 384)


# ---- refusals, before any draw ----------------------------------------------------------------------------------------------------------
class _NoGpu:
    """Stands where a LatentDiffusion would: what the entry points read before they touch the GPU; anything else raises."""
    latent_t_size, latent_t_per_second, first_stage_key, num_timesteps = 256, 25.6, "fbank", 1000
    latent_f_size, sampling_rate = 16, 16000

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


BAD_KEEP_S = [([(0, 4), (4, 6, 0.0)], "level"), ([(0, 4, 1.5)], "level"), ([(0, 4, float("nan"))], "level"), ([(0, 4, .5), (3, 6)], "ordered"),
              ([(0, 4, .5, 1)], "keep: ")]


def test_entry_points_refuse_before_any_draw_or_gpu_work():
    from audioldm2_amd.pipeline import extend_audio, make_batch_for_text_to_audio
    ld = _ld_stub()
    wav = np.zeros(6 * 16000, dtype=np.float32)
    batch = make_batch_for_text_to_audio("rain")
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for keep, msg in BAD_KEEP_S:
        with pytest.raises(ValueError, match=msg):
            extend_audio(ld, "rain", wav, 30, keep=keep)
    for feather, msg in ((-1.0, "feather"), (float("nan"), "feather"), ("1", "feather"), (None, "feather"), (True, "feather"),
                         (30.0, "feather")):
        with pytest.raises(ValueError, match=msg):
            extend_audio(ld, "rain", wav, 30, keep=[(0, 6)], feather=feather)
    with pytest.raises(ValueError, match="feather"):
        extend_audio(ld, "rain", wav, 30, feather=-0.5)                     # the default keep
    long_job = lambda keep, **kw: ld.generate_batch_long_from_audio(batch, 768, keep, **kw)
    for keep, kw, msg in (([(0, 200, 0.0)], {}, "level"), ([(0, 200, 2)], {}, "level"), ([(0, 200, .5), (100, 300)], {}, "ordered"),
                          ([(0, 200)], dict(feather=-1), "feather"), ([(0, 200)], dict(feather=768), "feather"),
                          ([(0, 200)], dict(feather=2.5), "feather"), ([(0, 200, .5)], dict(feather=None), "feather"),
                          ([(0, 200.0, .5)], {}, "integers"), ([(0, 800, .5)], dict(loop=True), "leaves")):
        with pytest.raises(ValueError, match=msg):
            long_job(keep, **kw)
    # generate_batch_masked and sample_log: levels need a DDIM-family sampler, and values in [0, 1]
    ok = torch.full((1, 1, 256, 16), .5)
    for levels, kw, msg in ((ok, dict(ddim_steps=None), "levels= needs ddim_steps"), (ok * 3, {}, r"lie in \[0, 1\]"), (-ok, {}, r"lie in \[0, 1\]"),
                            (ok * float("nan"), {}, "finite"), ([[.5]], {}, "must be a tensor")):
        with pytest.raises(ValueError, match=msg):
            ld.generate_batch_masked(batch, levels=levels, **kw)
    mask = torch.full((1, 1, 16, 8), .5)
    x0 = torch.zeros(1, 8, 16, 8)
    for kw, msg in ((dict(ddim=False, mask=mask, x0=x0), "graded=True needs ddim_steps"), (dict(ddim=True), "needs a mask"),
                    (dict(ddim=True, mask=mask), "needs a mask"), (dict(ddim=True, mask=mask * 4, x0=x0), r"lie in \[0, 1\]"),
                    (dict(ddim=True, use_plms=True, mask=-mask, x0=x0), r"lie in \[0, 1\]"),
                    (dict(ddim=True, sampler="dpmpp_2m", mask=mask * float("inf"), x0=x0), "finite")):
        with pytest.raises(ValueError, match=msg):
            ld.sample_log(None, 1, ddim_steps=6, graded=True, **kw)
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn
    assert ld.latent_t_size == 256


def test_samplers_refuse_before_any_draw():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    from audioldm2_amd.windows import window_plan, with_source
    m = Rs.ScheduleModel()
    level, x0 = torch.full((1, 1, 16, 1), .5), torch.zeros(A.TINY_SHAPE)
    torch.manual_seed(6)
    state = torch.get_rng_state()
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        def run(**kw):
            args = dict(dict(S=5, batch_size=2, shape=A.TINY_SHAPE[1:], verbose=False, mask=level, x0=x0, graded=True), **kw)
            return cls(m).sample(**args)
        for kw, msg in ((dict(mask=None, x0=None), "needs a mask"), (dict(x0=None), "needs a mask"), (dict(mask=level * 2.5), r"lie in \[0, 1\]"),
                        (dict(mask=level - 1), r"lie in \[0, 1\]"), (dict(mask=level * float("nan")), "finite"),
                        (dict(mask=level / 0.0), "finite")):
            with pytest.raises(ValueError, match=msg):
                run(**kw)
        # a source on the plan carries its own flag
        plan = window_plan(16, 16, 8)
        for bad in (torch.full((16,), 1.5), torch.full((16,), float("nan"))):
            with pytest.raises(ValueError, match=r"finite and lie in \[0, 1\]"):
                run(mask=None, x0=None, graded=False, windows=with_source(plan, x0, bad, graded=True))
        with pytest.raises(ValueError, match="needs a mask"):
            run(mask=None, x0=None, windows=plan)
    s = DDIMSampler(m)
    s.make_schedule(6, verbose=False)
    with pytest.raises(ValueError, match="needs a mask"):
        s.ddim_sampling(None, A.TINY_SHAPE, graded=True)
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn


def test_with_source_carries_the_flag_and_keeps_the_plan_key():
    from audioldm2_amd.windows import keep_levels, plan_key, window_plan, with_source
    plan = window_plan(40, 16, 10)
    x0, lv = torch.zeros(1, 2, 40, 4), keep_levels(40, [(0, 11)], 3)
    plain, graded = with_source(plan, x0, lv), with_source(plan, x0, lv, graded=True)
    assert plain.graded is False and graded.graded is True
    assert plan_key(plain) == plan_key(graded) == plan_key(plan)


# ---- the ABI and the signatures ----------------------------------------------------------------------------------------------------
def test_abi_version_symbol_and_signatures():
    from audioldm2_amd import lib
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.pipeline import LatentDiffusion, extend_audio
    assert lib.ABI_VERSION >= 24
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    assert "aldm_keep_threshold_indexed" in lib.EXPORTED_SYMBOLS and hasattr(l, "aldm_keep_threshold_indexed")
    assert inspect.signature(extend_audio).parameters["feather"].default == 0.0
    assert inspect.signature(LatentDiffusion.generate_batch_long_from_audio).parameters["feather"].default == 0
    assert inspect.signature(LatentDiffusion.generate_batch_masked).parameters["levels"].default is None
    for name in ("sample", "ddim_sampling"):
        assert inspect.signature(getattr(DDIMSampler, name)).parameters["graded"].default is False


def test_entry_validates_before_launch():
    """aldm_keep_threshold_indexed refuses null pointers, n <= 0, rows <= 0 and a mask inside the levels before any launch:
    observable without a GPU (the pointers are never dereferenced)."""
    from audioldm2_amd import lib
    l = lib.load()
    p = lambda a: ctypes.c_void_p(a)
    level, thr, mask = 1 << 20, 1 << 24, 1 << 28
    for args, msg in (((None, p(thr), None, 3, p(mask), 64), "null pointer"), ((p(level), None, None, 3, p(mask), 64), "null pointer"),
                      ((p(level), p(thr), None, 3, None, 64), "null pointer"), ((p(level), p(thr), None, 3, p(mask), 0), "bad args"),
                      ((p(level), p(thr), None, 3, p(mask), -4), "bad args"), ((p(level), p(thr), None, 0, p(mask), 64), "bad args"),
                      ((p(level), p(thr), None, -1, p(mask), 64), "bad args"),
                      ((p(level), p(thr), None, 3, p(level), 64), "mask overlaps level"),
                      ((p(level), p(thr), None, 3, p(level + 4 * 63), 64), "mask overlaps level"),
                      ((p(level), p(thr), None, 3, p(level - 4 * 63), 64), "mask overlaps level")):
        assert l.aldm_keep_threshold_indexed(*args, None) != 0, args
        assert msg in l.aldm_last_error().decode(), (args, l.aldm_last_error())
