"""CPU tests of long-form generation (windowed diffusion): the window plan's properties, the ABI of the two new
entries and their host-side refusals, and the argument errors of the entry points, all raised before any GPU work.  (No kernel is
launched here.)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import windowed as Wd
from audioldm2_amd.windows import tile_cond, window_plan


@pytest.mark.parametrize("T,Tw,hop", sorted(Wd.PLAN_GRID))
def test_window_plan_properties(T, Tw, hop):
    p = window_plan(T, Tw, hop)
    W, cover, last = Wd.PLAN_GRID[(T, Tw, hop)]
    s = list(p.starts)
    assert (p.W, p.cover, s[-1]) == (W, cover, last) and len(s) == W and (p.T, p.Tw, p.hop) == (T, Tw, hop)
    # the starts: s_0 = 0, ascending, j*hop but for the clamped last one, the last window ends at T, no gap wider than a window
    assert s[0] == 0 and s[-1] == T - Tw and s[:-1] == [j * hop for j in range(W - 1)]
    assert all(0 < b - a <= Tw for a, b in zip(s, s[1:]))
    assert W == 1 or s[-2] + Tw < T
    # the weights: fp32 [W, Tw], strictly positive, and per frame they sum to 1 within 2^-23 in fp64
    assert p.wn.dtype == torch.float32 and tuple(p.wn.shape) == (W, Tw) and bool((p.wn > 0).all())
    total = np.zeros(T)
    count = np.zeros(T, dtype=int)
    for j, a in enumerate(s):
        total[a:a + Tw] += p.wn[j].double().numpy()
        count[a:a + Tw] += 1
    assert count.min() >= 1 and count.max() == cover
    assert np.abs(total - 1.0).max() <= 2.0 ** -23
    # exactly 1.0 where one window covers the frame; everywhere with hop == Tw on a whole number of windows, and with T == Tw
    for j, a in enumerate(s):
        assert bool((p.wn[j][torch.from_numpy(count[a:a + Tw] == 1)] == 1.0).all())
    if T == Tw or (hop == Tw and T % Tw == 0):
        assert bool((p.wn == 1.0).all())
    # the raw taper behind the weights, where no normalisation enters (a frame under one window) and where two windows meet
    ramp = Tw - hop
    w = np.minimum(1.0, np.minimum((np.arange(Tw) + 1.0) / (ramp + 1.0), (Tw - np.arange(Tw)) / (ramp + 1.0)))
    if W >= 2 and s[1] == hop < Tw and count[hop] == 2:
        t = hop   # the first frame of window 1: under windows 0 and 1 only
        want = w[0] / (w[0] + w[t])
        assert abs(float(p.wn[1, 0]) - want) <= 2.0 ** -24 * want


@pytest.mark.parametrize("T,Tw,hop", [(40, 16, 10), (768, 256, 192), (384, 256, 128)])
def test_scaled_plan_is_the_plan_of_the_scaled_numbers(T, Tw, hop):
    a, b = window_plan(T, Tw, hop, scale=4), window_plan(4 * T, 4 * Tw, 4 * hop)
    assert a.starts == b.starts == tuple(4 * s for s in window_plan(T, Tw, hop).starts)
    assert (a.T, a.Tw, a.hop, a.W, a.cover) == (b.T, b.Tw, b.hop, b.W, b.cover) and a.scale == 4
    assert torch.equal(a.wn, b.wn)


@pytest.mark.parametrize("args", Wd.PLAN_REFUSED, ids=str)
def test_window_plan_refuses(args):
    with pytest.raises(ValueError, match="window_plan"):
        window_plan(*args)


def test_thirty_two_windows_are_the_most():
    p = window_plan(256 + 31 * 8, 256, 8)
    assert p.W == 32 and p.starts[-1] == 31 * 8
    with pytest.raises(ValueError, match="more than 32 windows"):
        window_plan(256 + 32 * 8, 256, 8)


def test_tile_cond_is_window_major():
    c = {"a": [torch.arange(2.0).view(2, 1), torch.ones(2, 3)], "b": torch.arange(2.0), "c": None}
    t = tile_cond(c, 3)
    assert t["a"][0].view(-1).tolist() == [0, 1, 0, 1, 0, 1] and tuple(t["a"][1].shape) == (6, 3) and t["c"] is None
    assert t["b"].tolist() == [0, 1, 0, 1, 0, 1]
    tup = tile_cond(([torch.zeros(2, 4)], [torch.ones(2, 4)]), 2)
    assert isinstance(tup, tuple) and tuple(tup[0][0].shape) == (4, 4)
    assert tile_cond(None, 4) is None


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbols():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 18
    assert "aldm_window_gather" in lib.EXPORTED_SYMBOLS and "aldm_window_merge" in lib.EXPORTED_SYMBOLS
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    assert hasattr(l, "aldm_window_gather") and hasattr(l, "aldm_window_merge")
    assert ctypes.sizeof(lib.WindowStarts) == 4 * (1 + lib.MAX_WINDOWS) and lib.MAX_WINDOWS == 32


def _starts(lib, values, n=None):
    st = lib.WindowStarts()
    st.n = len(values) if n is None else n
    for j, s in enumerate(values):
        st.s[j] = s
    return st


BAD_STARTS = [([0, 12, 10, 24], None, "ascend"), ([0, 10, 10, 24], None, "ascend"), ([0, 17, 24], None, "exceeds Tw"),
              ([0, 10, 20, 23], None, "last start"), ([0, 10, 20, 24], 3, "starts"), ([2, 10, 20, 24], None, r"starts\[0\]"),
              ([0, 10, 20, 30], None, "last start")]


@pytest.mark.parametrize("values,n,msg", BAD_STARTS, ids=[m + str(i) for i, (_, _, m) in enumerate(BAD_STARTS)])
def test_c_entries_refuse_bad_starts_before_any_launch(values, n, msg):
    """T = 40, Tw = 16: the plan (40, 16, 10) has the starts 0, 10, 20, 24.  The data pointers are never dereferenced: validation
    fails first (as tests/test_abi.py calls the decode entries)."""
    from audioldm2_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(4096)
    q = ctypes.c_void_p(1 << 30)
    W = len(values)
    st = _starts(lib, values, n)
    assert l.aldm_window_gather(p, q, st, 2, W, 3, 40, 16, 5, None) < 0
    with pytest.raises(RuntimeError, match=msg):
        lib.check(-1, "window_gather")
    assert l.aldm_window_merge(q, p, ctypes.c_void_p(1 << 31), st, 2, 2, W, 3, 40, 16, 5, None) < 0
    with pytest.raises(RuntimeError, match=msg):
        lib.check(-1, "window_merge")


def test_c_entries_refuse_bad_shapes_and_overlap():
    from audioldm2_amd import lib
    l = lib.load()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    st = _starts(lib, [0, 10, 20, 24])
    for call, msg in ((lambda: l.aldm_window_gather(None, q, st, 2, 4, 3, 40, 16, 5, None), "null"),
                      (lambda: l.aldm_window_gather(p, q, st, 2, 4, 3, 8, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather(p, q, st, 0, 4, 3, 40, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather(p, p, st, 2, 4, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge(q, p, r, st, 3, 2, 4, 3, 40, 16, 5, None), "H=3"),
                      (lambda: l.aldm_window_merge(q, p, q, st, 2, 2, 4, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge(q, p, r, _starts(lib, [0] * 32, 33), 2, 2, 33, 3, 40, 16, 5, None), "windows")):
        assert call() < 0
        assert msg in l.aldm_last_error().decode()


# ---- the entry points' argument errors: raised before any GPU work ---------------------------------------------------------------
class _NoGpu:
    """Stands where a LatentDiffusion would: what the long-form entry points read before they touch the GPU; anything else raises."""
    latent_t_size, latent_t_per_second, first_stage_key = 256, 25.6, "fbank"

    class first_stage_model:
        class encoder:
            num_resolutions = 3

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the arguments were checked")


def _ld_stub():
    from audioldm2_amd.pipeline import LatentDiffusion
    stub = _NoGpu()
    for name in ("long_form_plans", "generate_batch_long", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(_NoGpu, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return stub


def test_text_to_audio_long_argument_errors():
    from audioldm2_amd.pipeline import text_to_audio_long
    ld = _ld_stub()
    with pytest.raises(ValueError, match="multiple of 8"):
        text_to_audio_long(ld, "rain", 12)              # int(12 * 25.6) = 307
    with pytest.raises(ValueError, match="shorter than the model's window"):
        text_to_audio_long(ld, "rain", 5)               # 128 frames < 256
    with pytest.raises(ValueError, match="hop"):
        text_to_audio_long(ld, "rain", 15, overlap=10.0)   # hop = 0
    with pytest.raises(ValueError, match="hop"):
        text_to_audio_long(ld, "rain", 15, overlap=-1.0)   # hop > Tw
    with pytest.raises(ValueError, match="more than 32 windows"):
        text_to_audio_long(ld, "rain", 600, overlap=9.7)
    with pytest.raises(ValueError, match="needs ddim_steps"):
        text_to_audio_long(ld, "rain", 15, ddim_steps=None)
    with pytest.raises(ValueError, match="unknown sampler"):
        text_to_audio_long(ld, "rain", 15, sampler="euler")
    assert ld.latent_t_size == 256


def test_generate_batch_long_argument_errors():
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    ld = _ld_stub()
    batch = make_batch_for_text_to_audio("rain")
    with pytest.raises(ValueError, match="n_gen must be 1"):
        ld.generate_batch_long(batch, 384, n_gen=3)
    with pytest.raises(ValueError, match="needs ddim_steps"):
        ld.generate_batch_long(batch, 384, ddim_steps=None)
    with pytest.raises(ValueError, match="shard"):
        ld.generate_batch_long(batch, 384, shard=(0, 2))
    with pytest.raises(ValueError, match="multiple of 8"):
        ld.generate_batch_long(batch, 380)
    with pytest.raises(ValueError, match="shorter than the model's window"):
        ld.generate_batch_long(batch, 128)
    with pytest.raises(ValueError, match="negative_prompt needs"):
        ld.generate_batch_long(batch, 384, negative_prompt="noise")
    with pytest.raises(ValueError, match="guidance_rescale"):
        ld.generate_batch_long(batch, 384, guidance_rescale=1.5)


def test_samplers_refuse_a_mask_with_windows():
    """plan_run refuses before its first device tensor; sample_log before it builds a sampler."""
    from audioldm2_amd.pipeline import LatentDiffusion
    from audioldm2_amd.sampling import SamplerBase

    class M:
        num_timesteps = 1000
        alphas_cumprod = torch.linspace(0.999, 0.01, 1000)
    s = SamplerBase(M())
    s.make_schedule(4, verbose=False)
    plan = window_plan(40, 16, 10)
    table = lambda n, cfg: torch.zeros(n, 8)
    with pytest.raises(ValueError, match="inpainting over windows"):
        s.plan_run(None, (2, 8, 40, 8), None, None, None, table, 1.0, None, 0.0, torch.ones(2, 1, 40, 8), torch.zeros(2, 8, 40, 8),
                   windows=plan)
    with pytest.raises(ValueError, match="plan over T=40"):
        s.plan_run(None, (2, 8, 48, 8), None, None, None, table, 1.0, None, 0.0, None, None, windows=plan)
    stub = _NoGpu()
    sample_log = inspect.getattr_static(LatentDiffusion, "sample_log")
    sample_log = getattr(sample_log, "__wrapped__", sample_log)
    with pytest.raises(ValueError, match="inpainting over windows"):
        sample_log(stub, None, 2, True, 4, mask=torch.ones(2, 1, 40, 8), windows=plan)
    with pytest.raises(ValueError, match="needs ddim_steps"):
        sample_log(stub, None, 2, False, None, windows=plan)
    with pytest.raises(ValueError, match="latent_t_size is 256"):
        sample_log(stub, None, 2, True, 4, windows=plan)
