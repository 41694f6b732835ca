"""CPU tests of seamless loops (ring plans): the ring plan's table, refusals and weights, its key and flags, the ABI of
the three wrap-around entries and their host-side refusals, the vocoder's reach, and the argument errors of the loop entry points, all
raised before any draw.  (No kernel is launched here.)"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import looped as Lp
from audioldm2_amd.windows import keep_mask, plan_key, window_plan, with_source


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Tw,hop", sorted(Lp.RING_TABLE))
def test_ring_plan_table_and_weights(T, Tw, hop):
    p = window_plan(T, Tw, hop, ring=True)
    W, starts, cover = Lp.RING_TABLE[(T, Tw, hop)]
    assert (p.W, p.starts, p.cover) == (W, starts, cover) and p.ring is True
    assert (p.T, p.Tw, p.hop, p.scale) == (T, Tw, hop, 1)
    # the definition: W = ceil(T / hop), s_j = (j*T) // W, every gap (the wrap gap included) floor(T/W) or ceil(T/W), hence <= hop
    assert W == math.ceil(T / hop) and list(starts) == [(j * T) // W for j in range(W)]
    gaps = [b - a for a, b in zip(starts, starts[1:] + (T,))]
    assert set(gaps) <= {T // W, -(-T // W)} and max(gaps) <= hop
    # the mel plan's starts are exactly scale x the latent plan's
    m = window_plan(T, Tw, hop, scale=4, ring=True)
    assert m.starts == tuple(4 * s for s in starts) and (m.T, m.Tw, m.hop, m.W, m.cover, m.scale, m.ring) == (4 * T, 4 * Tw, 4 * hop,
                                                                                                              W, cover, 4, True)
    for q in (p, m):
        # the weights: fp32 [W, Tw], strictly positive; per frame their fp64 sum over the covering windows is within cover * 2^-24
        # of 1 (each is the fp32 rounding, at most 2^-24 relative, of an fp64 quotient below 1; the quotients sum to 1)
        assert q.wn.dtype == torch.float32 and tuple(q.wn.shape) == (W, q.Tw) and bool((q.wn > 0).all())
        total, count = np.zeros(q.T), np.zeros(q.T, dtype=int)
        for j, s in enumerate(q.starts):
            frames = (s + np.arange(q.Tw)) % q.T
            assert len(set(frames.tolist())) == q.Tw          # a window covers no frame twice
            total[frames] += q.wn[j].double().numpy()
            count[frames] += 1
        assert count.min() >= 1 and count.max() == cover
        assert np.abs(total - 1.0).max() <= cover * 2.0 ** -24
        # exactly 1.0 where one window covers the frame
        for j, s in enumerate(q.starts):
            one = torch.from_numpy(count[(s + np.arange(q.Tw)) % q.T] == 1)
            assert bool((q.wn[j][one] == 1.0).all())
    # the raw taper: ramp = Tw - (the largest gap); the first frame of window 1 where it lies under windows 0 and 1 only
    ramp = Tw - max(gaps)
    w = np.minimum(1.0, np.minimum((np.arange(Tw) + 1.0) / (ramp + 1.0), (Tw - np.arange(Tw)) / (ramp + 1.0)))
    if cover == 2 and W > 2:
        want = w[0] / (w[0] + w[starts[1]])
        assert abs(float(p.wn[1, 0]) - want) <= 2.0 ** -24 * want


@pytest.mark.parametrize("args", Lp.RING_REFUSED, ids=str)
def test_ring_plan_refuses(args):
    with pytest.raises(ValueError, match="window_plan"):
        window_plan(*args, ring=True)


def test_a_ring_without_overlap_says_why():
    with pytest.raises(ValueError, match="junction"):
        window_plan(40, 16, 16, ring=True)
    with pytest.raises(ValueError, match="more than 32 windows"):
        window_plan(8 * 40, 8, 1, ring=True)
    assert window_plan(32 * 7, 8, 7, ring=True).W == 32         # thirty-two windows are the most
    with pytest.raises(ValueError, match="more than 32 windows"):
        window_plan(32 * 7 + 8, 8, 7, ring=True)


def test_keys_and_flags():
    for key in [(40, 16, 10), (768, 256, 192), (384, 256, 128)]:
        ring, lin = window_plan(*key, ring=True), window_plan(*key)
        assert plan_key(ring) != plan_key(lin) and plan_key(ring) == plan_key(window_plan(*key, ring=True))
        assert lin.ring is False
    # (40, 16, 16): the ring plan of the same starts as a linear plan still has another key
    lin = window_plan(32, 16, 8)
    ring = window_plan(32, 16, 8, ring=True)
    assert (lin.starts, ring.starts) == ((0, 8, 16), (0, 8, 16, 24))
    # ring=False is today's plan, field for field: the linear construction restated (starts j*hop, then T - Tw; ramp = Tw - hop)
    for T, Tw, hop in [(40, 16, 10), (48, 16, 16), (16, 16, 8), (768, 256, 192), (24, 16, 1)]:
        p = window_plan(T, Tw, hop, ring=False)
        starts = [s for s in range(0, T - Tw, hop)] + [T - Tw]
        w = np.minimum(1.0, np.minimum((np.arange(Tw) + 1.0) / (Tw - hop + 1.0), (Tw - np.arange(Tw)) / (Tw - hop + 1.0)))
        norm, count = np.zeros(T), np.zeros(T, dtype=int)
        for s in starts:
            norm[s:s + Tw] += w
            count[s:s + Tw] += 1
        wn = torch.from_numpy(np.stack([w / norm[s:s + Tw] for s in starts]).astype(np.float32))
        assert (p.T, p.Tw, p.hop, p.scale, p.W, p.starts, p.cover, p.ring) == (T, Tw, hop, 1, len(starts), tuple(starts),
                                                                              int(count.max()), False)
        assert torch.equal(p.wn.view(torch.int32), wn.view(torch.int32))
        d = window_plan(T, Tw, hop)
        assert d.ring is False and d.starts == p.starts and torch.equal(d.wn, p.wn)
    # with_source keeps the flag and the key
    ring = window_plan(40, 16, 10, ring=True)
    src = with_source(ring, torch.zeros(1, 2, 40, 4), keep_mask(40, [(0, 13)]))
    assert src.ring is True and plan_key(src) == plan_key(ring) and src.starts == ring.starts and src.wn is ring.wn
    assert with_source(window_plan(40, 16, 10), torch.zeros(1, 2, 40, 4), keep_mask(40, [(0, 13)])).ring is False


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
RING_ENTRIES = ("aldm_window_gather_ring", "aldm_window_merge_ring", "aldm_window_blend_gather_ring")


def test_abi_version_and_symbols():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 20
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    for name in RING_ENTRIES:
        assert name in lib.EXPORTED_SYMBOLS and hasattr(l, name)
        # the argument list of the linear sibling
        assert lib._SIGS[name] == lib._SIGS[name[:-len("_ring")]]


def _starts(lib, values, n=None):
    st = lib.WindowStarts()
    st.n = len(values) if n is None else n
    for j, s in enumerate(values):
        st.s[j] = s
    return st


# T = 40, Tw = 16: the ring plan (40, 16, 10) has the starts 0, 10, 20, 30; the linear one 0, 10, 20, 24 is a legal ring too
BAD_RING_STARTS = [([0, 12, 10, 30], None, "ascend"), ([0, 10, 10, 30], None, "ascend"), ([0, 17, 30], None, "exceeds Tw"),
                   ([0, 10, 20, 23], None, "wrap"), ([0, 10, 20, 30], 3, "starts"), ([2, 10, 20, 30], None, r"starts\[0\]"),
                   ([0, 10, 20, 40], None, "below T"), ([0], None, "2 <= W"), ([0, 16], None, "wrap")]


@pytest.mark.parametrize("values,n,msg", BAD_RING_STARTS, ids=[m + str(i) for i, (_, _, m) in enumerate(BAD_RING_STARTS)])
def test_ring_entries_refuse_bad_starts_before_any_launch(values, n, msg):
    """The data pointers are never dereferenced: validation fails first (as tests/test_windowed_cpu.py calls the linear entries)."""
    from audioldm2_amd import lib
    l = lib.load()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    W = len(values)
    st = _starts(lib, values, n)
    assert l.aldm_window_gather_ring(p, q, st, 2, W, 3, 40, 16, 5, None) < 0
    with pytest.raises(RuntimeError, match=msg):
        lib.check(-1, "window_gather_ring")
    assert l.aldm_window_merge_ring(q, p, r, st, 2, 2, W, 3, 40, 16, 5, None) < 0
    with pytest.raises(RuntimeError, match=msg):
        lib.check(-1, "window_merge_ring")
    assert l.aldm_window_blend_gather_ring(p, r, r, r, r, None, 1, 1, q, st, 2, W, 3, 40, 16, 5, None) < 0
    with pytest.raises(RuntimeError, match=msg):
        lib.check(-1, "window_blend_gather_ring")


def test_ring_entries_refuse_bad_shapes_and_overlap():
    from audioldm2_amd import lib
    l = lib.load()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    st = _starts(lib, [0, 10, 20, 30])
    for call, msg in ((lambda: l.aldm_window_gather_ring(None, q, st, 2, 4, 3, 40, 16, 5, None), "null"),
                      (lambda: l.aldm_window_gather_ring(p, q, st, 2, 4, 3, 8, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather_ring(p, q, st, 0, 4, 3, 40, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather_ring(p, p, st, 2, 4, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge_ring(q, p, r, st, 3, 2, 4, 3, 40, 16, 5, None), "H=3"),
                      (lambda: l.aldm_window_merge_ring(q, p, q, st, 2, 2, 4, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_blend_gather_ring(p, r, r, r, r, None, 0, 1, q, st, 2, 4, 3, 40, 16, 5, None), "q_rows"),
                      (lambda: l.aldm_window_blend_gather_ring(p, p, r, r, r, None, 1, 1, q, st, 2, 4, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge_ring(q, p, r, _starts(lib, [0] * 32, 33), 2, 2, 33, 3, 40, 16, 5, None), "windows")):
        assert call() < 0
        assert msg in l.aldm_last_error().decode()


# ---- the vocoder's reach ------------------------------------------------------------------------------------------------------------
def test_vocoder_reach_is_derived_from_the_config():
    from audioldm2_amd.hifigan import get_vocoder_config, get_vocoder_config_48k, reach_frames
    for cfg in (get_vocoder_config(), get_vocoder_config_48k()):
        P, by_hand = reach_frames(cfg), Lp.reach_by_hand(cfg)
        print(f"vocoder reach, {cfg['num_mels']} mel bins: {P} frames (by hand {by_hand:.4f})")
        assert isinstance(P, int) and P >= by_hand and P < 64
    # the 16 kHz generator: 3 + (15/5 + 15/20 + 7/40 + 3/80 + 3/160) + 60 * (1/5 + 1/20 + 1/40 + 1/80 + 1/160) + 3/160 = 24.625
    assert abs(Lp.reach_by_hand(get_vocoder_config()) - 24.625) < 1e-9 and reach_frames(get_vocoder_config()) == 25


# ---- the entry points' argument errors: raised before any draw ----------------------------------------------------------------------
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
    for name in ("long_form_plans", "generate_batch_long", "generate_batch_long_from_audio", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(_NoGpu, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return stub


def _refused_before_any_draw(call, match):
    torch.manual_seed(123)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=match):
        call()
    assert torch.equal(torch.get_rng_state(), state)


def test_loop_plans_of_the_pipeline():
    ld = _ld_stub()
    plan, mel_plan = ld.long_form_plans(384, 128, ring=True)
    assert (plan.W, plan.starts, mel_plan.starts, mel_plan.Tw, plan.ring, mel_plan.ring) == (3, (0, 128, 256), (0, 512, 1024), 1024,
                                                                                           True, True)
    plan, mel_plan = ld.long_form_plans(256, ring=True)          # the trained length is a legal ring; the default hop 3*Tw//4
    assert (plan.W, plan.starts, plan.hop, mel_plan.starts) == (2, (0, 128), 192, (0, 512))
    lin, _ = ld.long_form_plans(384, 128)
    assert lin.ring is False and lin.starts == (0, 128)


def test_loop_argument_errors_are_raised_before_any_draw():
    from audioldm2_amd.pipeline import extend_audio, make_batch_for_text_to_audio, text_to_audio_long
    ld = _ld_stub()
    batch = make_batch_for_text_to_audio("rain")
    _refused_before_any_draw(lambda: text_to_audio_long(ld, "rain", 15, overlap=0, loop=True), "junction")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 384, hop=256, loop=True), "junction")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 384, n_gen=2, loop=True), "n_gen must be 1")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 384, ddim_steps=None, loop=True), "needs ddim_steps")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 384, shard=(0, 2), loop=True), "shard")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 128, loop=True), "shorter than the model's window")
    _refused_before_any_draw(lambda: ld.generate_batch_long(batch, 380, loop=True), "multiple of 8")
    for kw, match in ((dict(hop=256), "junction"), (dict(n_gen=2), "n_gen must be 1"), (dict(ddim_steps=None), "needs ddim_steps"),
                      (dict(shard=(0, 2)), "shard")):
        _refused_before_any_draw(lambda: ld.generate_batch_long_from_audio(batch, 384, [(0, 128)], loop=True, **kw), match)
    _refused_before_any_draw(lambda: extend_audio(ld, "rain", np.zeros(16000, dtype=np.float32), 15, overlap=0, loop=True), "junction")
    _refused_before_any_draw(lambda: extend_audio(ld, "rain", np.zeros(16000, dtype=np.float32), 15, ddim_steps=None, loop=True),
                             "needs ddim_steps")
    # without loop the same geometry is legal as far as the plans go (hop == Tw is a linear plan)
    assert ld.long_form_plans(512, 256)[0].starts == (0, 256)
    assert ld.latent_t_size == 256
