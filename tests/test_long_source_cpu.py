"""CPU tests of continuation and inpainting of long clips: windows.keep_mask and windows.with_source, the ABI of
aldm_window_blend_gather and its host-side refusals, the argument errors of the entry points — all raised before any draw and any
GPU work — and the self-check of the helpers' fp64 restatement.  (No kernel is launched here.)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import long_source as Ls
import windowed as Wd
from audioldm2_amd.windows import keep_mask, plan_key, window_plan, with_source


# ---- keep_mask ----------------------------------------------------------------------------------------------------------------------
KEEP_GRID = [(40, [], []), (40, [(0, 13)], list(range(13))), (40, [(0, 13), (29, 33)], list(range(13)) + [29, 30, 31, 32]),
             (40, [(0, 13), (13, 20)], list(range(20))),                  # touching intervals
             (40, [(0, 40)], list(range(40))), (16, [(15, 16)], [15]),    # a full cover; the last frame alone
             (40, [(np.int64(3), np.int32(5))], [3, 4])]


@pytest.mark.parametrize("T,intervals,ones", KEEP_GRID, ids=str)
def test_keep_mask_marks_the_half_open_intervals(T, intervals, ones):
    m = keep_mask(T, intervals)
    assert m.dtype == torch.float32 and tuple(m.shape) == (T,)
    assert m.nonzero().view(-1).tolist() == ones and set(m.tolist()) <= {0.0, 1.0}


KEEP_REFUSED = [(40, [(5, 5)], "empty"), (40, [(7, 5)], "empty"), (40, [(10, 20), (0, 5)], "ordered"),
                (40, [(0, 13), (12, 20)], "overlap"), (40, [(-1, 5)], r"leaves \[0, 40\)"), (40, [(30, 41)], r"leaves \[0, 40\)"),
                (40, [(0.0, 5)], "integers"), (40, [(True, 5)], "integers"), (40, [5], "pair"), (40, [(1, 2, 3)], "pair")]


@pytest.mark.parametrize("T,intervals,msg", KEEP_REFUSED, ids=str)
def test_keep_mask_refuses(T, intervals, msg):
    with pytest.raises(ValueError, match=msg):
        keep_mask(T, intervals)


# ---- with_source --------------------------------------------------------------------------------------------------------------------
def test_with_source_keeps_the_plan_and_its_key():
    plan = window_plan(40, 16, 10)
    x0 = torch.zeros(2, 8, 40, 8)
    for mask in (keep_mask(40, Ls.KEEP), torch.ones(2, 1, 40, 8), torch.ones(1, 1, 40, 1), torch.ones(2, 8, 40, 8)):
        src = with_source(plan, x0, mask)
        assert plan_key(src) == plan_key(plan) and (src.T, src.Tw, src.W, src.starts, src.cover) == (40, 16, 4, plan.starts, 3)
        assert src.wn is plan.wn and src.x0 is x0
        assert tuple(torch.broadcast_shapes(tuple(src.mask.shape), tuple(x0.shape))) == tuple(x0.shape)
    assert tuple(with_source(plan, x0, keep_mask(40, Ls.KEEP)).mask.shape) == (1, 1, 40, 1)
    assert not hasattr(plan, "x0") and not hasattr(plan, "mask")          # the plain plan is left as it was


def test_with_source_refuses_wrong_shapes():
    plan = window_plan(40, 16, 10)
    x0 = torch.zeros(2, 8, 40, 8)
    for bad_x0 in (torch.zeros(2, 8, 48, 8), torch.zeros(8, 40, 8), None):
        with pytest.raises(ValueError, match="x0 must be"):
            with_source(plan, bad_x0, torch.ones(40))
    for bad_mask, msg in ((torch.ones(48), "one entry per latent frame"), (torch.ones(2, 1, 48, 8), "does not broadcast"),
                          (torch.ones(3, 1, 40, 8), "does not broadcast"), (torch.ones(2, 2, 8, 40, 8), "does not broadcast"),
                          ([1.0] * 40, "must be a tensor")):
        with pytest.raises(ValueError, match=msg):
            with_source(plan, x0, bad_mask)


def test_plan_run_refuses_a_source_of_another_shape_and_still_refuses_mask_keywords():
    from audioldm2_amd.sampling import SamplerBase

    class M:
        num_timesteps = 1000
        alphas_cumprod = torch.linspace(0.999, 0.01, 1000)
    s = SamplerBase(M())
    s.make_schedule(4, verbose=False)
    plan = window_plan(40, 16, 10)
    table = lambda n, cfg: torch.zeros(n, 8)
    src = with_source(plan, torch.zeros(2, 4, 40, 8), keep_mask(40, Ls.KEEP))
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="source x0"):
        s.plan_run(None, (2, 8, 40, 8), None, None, None, table, 1.0, None, 0.0, None, None, windows=src)
    with pytest.raises(ValueError, match="inpainting over windows"):
        s.plan_run(None, (2, 4, 40, 8), None, None, None, table, 1.0, None, 0.0, torch.ones(2, 1, 40, 8), torch.zeros(2, 4, 40, 8),
                   windows=src)
    assert torch.equal(torch.get_rng_state(), state)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 19
    assert "aldm_window_blend_gather" in lib.EXPORTED_SYMBOLS
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION and hasattr(l, "aldm_window_blend_gather")


def _starts(lib, values, n=None):
    st = lib.WindowStarts()
    st.n = len(values) if n is None else n
    for j, s in enumerate(values):
        st.s[j] = s
    return st


def test_c_entry_refuses_before_any_launch():
    """T = 40, Tw = 16, the starts of the plan (40, 16, 10).  The data pointers are never dereferenced: validation fails first (as
    tests/test_windowed_cpu.py calls the gather and the merge).  x, x0, mask are 2*3*40*5 floats, win 4*2*3*16*5."""
    from audioldm2_amd import lib
    l = lib.load()
    P = lambda v: ctypes.c_void_p(v)
    x, x0, qn, m, coef, win = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20), P(1 << 30)
    st = _starts(lib, [0, 10, 20, 24])
    f = l.aldm_window_blend_gather
    ok_tail = (st, 2, 4, 3, 40, 16, 5, None)
    cases = [(lambda: f(None, x0, qn, m, coef, None, 1, 1, win, *ok_tail), "null pointer"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, None, *ok_tail), "null pointer"),
             (lambda: f(x, x0, None, m, coef, None, 1, 1, win, *ok_tail), "null pointer"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, win, st, 2, 4, 3, 8, 16, 5, None), "bad shape"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, win, st, 2, 4, 0, 40, 16, 5, None), "bad shape"),
             (lambda: f(x, x0, qn, m, coef, None, 0, 1, win, *ok_tail), "q_rows=0"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 0, win, *ok_tail), "coef_rows=0"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, P((1 << 20) + 4 * 100), *ok_tail), "win overlaps"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, P((4 << 20) - 16), *ok_tail), "win overlaps"),
             # the q-noise table's span counts all its rows: 3 rows from qn reach past win placed behind its first row
             (lambda: f(x, x0, qn, m, coef, None, 3, 1, P((3 << 20) + 4 * 1200 * 2), *ok_tail), "win overlaps"),
             (lambda: f(x, x, qn, m, coef, None, 1, 1, win, *ok_tail), "x overlaps"),
             (lambda: f(x, x0, qn, P((1 << 20) + 4 * 1199), coef, None, 1, 1, win, *ok_tail), "x overlaps"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, win, _starts(lib, [0] * 32, 33), 2, 33, 3, 40, 16, 5, None), "windows"),
             (lambda: f(x, x0, qn, m, coef, None, 1, 1, win, _starts(lib, [0, 17, 24]), 2, 3, 3, 40, 16, 5, None), "exceeds Tw")]
    for call, msg in cases:
        assert call() < 0
        assert msg in l.aldm_last_error().decode(), (msg, l.aldm_last_error().decode())


# ---- the entry points' refusals: before any draw and any GPU work ------------------------------------------------------------------
class _NoGpu:
    """Stands where a LatentDiffusion would: what the entry points read before they touch the GPU; anything else raises."""
    latent_t_size, latent_t_per_second, first_stage_key, latent_f_size, sampling_rate = 256, 25.6, "fbank", 16, 16000

    class first_stage_model:
        embed_dim = 8

        class encoder:
            num_resolutions = 3

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the arguments were checked")


def _ld_stub(**over):
    from audioldm2_amd.pipeline import LatentDiffusion

    class Stub(_NoGpu):
        pass
    for k, v in over.items():
        setattr(Stub, k, v)
    for name in ("long_form_plans", "generate_batch_long_from_audio", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(Stub, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return Stub()


def _long_batch(frames=384 * 4):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    batch = make_batch_for_text_to_audio("rain")
    batch["log_mel_spec"] = batch["fbank"] = torch.zeros(1, frames, 64)
    return batch


def test_generate_batch_long_from_audio_refuses_before_any_draw():
    ld = _ld_stub()
    batch = _long_batch()
    torch.manual_seed(5)
    state = torch.get_rng_state()
    G = ld.generate_batch_long_from_audio
    for kw, msg in ((dict(ddim_steps=None), "needs ddim_steps"), (dict(n_gen=3), "n_gen must be 1"), (dict(shard=(0, 2)), "shard"),
                    (dict(sampler="euler"), "unknown sampler"), (dict(guidance_rescale=1.5), "guidance_rescale"),
                    (dict(negative_prompt="noise"), "negative_prompt needs"), (dict(hop=0), "hop"), (dict(hop=257), "hop")):
        with pytest.raises(ValueError, match=msg):
            G(batch, 384, [(0, 100)], **kw)
    for T, msg in ((380, "multiple of 8"), (128, "shorter than the model's window")):
        with pytest.raises(ValueError, match=msg):
            G(batch, T, [(0, 100)])
    for keep, msg in (([(5, 5)], "empty"), ([(10, 20), (0, 5)], "ordered"), ([(0, 13), (12, 20)], "overlap"), ([(300, 385)], "leaves"),
                      ([(0.5, 3)], "integers")):
        with pytest.raises(ValueError, match=msg):
            G(batch, 384, keep)
    with pytest.raises(ValueError, match=r"latent_t_size\*4 = 1536"):
        G(_long_batch(1024), 384, [(0, 100)])
    with pytest.raises(ValueError, match=r"latent_t_size\*4 = 1536"):
        G(_long_batch(1540), 384, [(0, 100)])
    assert torch.equal(torch.get_rng_state(), state) and ld.latent_t_size == 256


def test_extend_audio_refuses_before_any_draw():
    import audioldm2_amd
    from audioldm2_amd.pipeline import extend_audio
    assert audioldm2_amd.extend_audio is extend_audio and "extend_audio" in audioldm2_amd.__all__
    ld = _ld_stub()
    src = np.sin(np.arange(6 * 16000) * 0.05).astype(np.float32)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for args, kw, msg in (((12,), {}, "multiple of 8"),                          # int(12 * 25.6) = 307
                          ((5,), {}, "shorter than the model's window"),
                          ((15,), dict(overlap=10.0), "hop"), ((15,), dict(overlap=-1.0), "hop"),
                          ((600,), dict(overlap=9.7), "more than 32 windows"),
                          ((15,), dict(ddim_steps=None), "needs ddim_steps"),
                          ((15,), dict(sampler="euler"), "unknown sampler"),
                          ((15,), dict(guidance_rescale=2.0), "guidance_rescale"),
                          ((15,), dict(keep=[(4.0, 2.0)]), "empty"), ((15,), dict(keep=[(2.0, 2.01)]), "empty"),
                          ((15,), dict(keep=[(5.0, 8.0), (1.0, 2.0)]), "ordered"),
                          ((15,), dict(keep=[(0.0, 5.0), (4.0, 8.0)]), "overlap"),
                          ((15,), dict(keep=[(-1.0, 5.0)]), "leaves"),
                          ((15,), dict(keep=[(0.0, float("nan"))]), "finite"), ((15,), dict(keep=[3.0]), "pair")):
        with pytest.raises(ValueError, match=msg):
            extend_audio(ld, "rain", src, *args, **kw)
    with pytest.raises(ValueError, match="16 kHz / 64-bin"):
        extend_audio(_ld_stub(sampling_rate=48000), "rain", src, 15)
    with pytest.raises(ValueError, match="16 kHz / 64-bin"):
        extend_audio(_ld_stub(latent_f_size=32), "rain", src, 15)
    assert torch.equal(torch.get_rng_state(), state) and ld.latent_t_size == 256


def test_keep_seconds_become_the_frames_wholly_inside():
    from audioldm2_amd.pipeline import keep_frames
    assert keep_frames([(0.0, 6.0)], 25.6, 384) == [(0, 153)]                 # floor(153.6)
    assert keep_frames([(2.0, 4.0)], 25.6, 384) == [(52, 102)]                # ceil(51.2), floor(102.4)
    assert keep_frames([(0, 12), (19, 40)], 25.6, 1024) == [(0, 307), (487, 1024)]
    assert keep_frames([(0.0, 20.0)], 25.6, 384) == [(0, 384)]                # the end is clipped to the clip


# ---- the helpers' own check ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(40, 16, 10), (24, 16, 1)])
def test_fp64_restatement_of_blend_then_gather(key):
    plan = window_plan(*key)
    x, x0, qn, coef = Ls.blend_inputs(2, plan, 3, 5, S=1)
    sa, so = coef[0].tolist()
    shape = tuple(x.shape)
    masks = Ls.mask_patterns(plan, shape)
    assert len(masks) == 4
    # a zero mask: the gather of x; a mask of ones: the windows of q_sample(x0)
    assert torch.equal(Ls.blend_gather_fp64(x, x0, qn[0], masks["zeros"], sa, so, plan), Wd.gather_ref(x.double(), plan))
    q = sa * x0.double() + so * qn[0].double()
    assert torch.equal(Ls.blend_gather_fp64(x, x0, qn[0], masks["ones"], sa, so, plan), Wd.gather_ref(q, plan))
    # the cut pattern: its two ends lie inside an overlap, on no start, and both values occur in some window
    a, b = Ls.overlap_interval(plan)
    for t in (a, b):
        assert t not in plan.starts and sum(s <= t < s + plan.Tw and s <= t - 1 for s in plan.starts) >= 2
    cut = [m for n, m in masks.items() if n.startswith("keep")][0]
    assert float(cut[0, 0, a - 1, 0]) == 0.0 and float(cut[0, 0, a, 0]) == 1.0 and float(cut[0, 0, b - 1, 0]) == 1.0 \
        and float(cut[0, 0, b, 0]) == 0.0
    ref, den = Ls.blend_fp64(x, x0, qn[0], cut, sa, so)
    assert torch.equal(ref[:, :, a:b], q[:, :, a:b]) and torch.equal(ref[:, :, :a], x.double()[:, :, :a]) and float(den.min()) > 0.0
    # the torch blend of the composition loops is the same expression
    assert torch.allclose(Ls.torch_blend(x, x0, qn[0], cut, sa, so).double(), ref, rtol=0, atol=1e-5)
