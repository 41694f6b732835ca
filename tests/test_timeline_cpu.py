"""CPU tests of prompt timelines: the prompt weights and the row plan against the definitions restated frame by frame
(tests/timeline.py) and the row counts worked out from them, the weight properties the merge kernel's bit-exact cases rest on,
every refusal, the per-row conditioning order, the seconds-to-frames mapping of the entry points, and the ABI: version, symbols,
and the host checks of the three row entries (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import timeline as Tl
from audioldm2_amd import windows as Wn
from audioldm2_amd.windows import PerPrompt, prompt_weights, row_plan, rows_cond, window_plan


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,bounds,tau,R,cover", Tl.ROW_GRID, ids=lambda v: str(v).replace(" ", ""))
def test_row_plan_matches_the_definitions(key, bounds, tau, R, cover):
    base, rp = Tl.plans_of(key, bounds, tau)
    m = prompt_weights(key[0], bounds, tau)
    m_ref, rows_ref, wr_ref, starts_ref = Tl.weights_fp64(key, bounds, tau)
    assert m.dtype == np.float64 and m.shape == (len(bounds) + 1, key[0])
    assert np.array_equal(m, np.asarray(m_ref))
    assert float(m.min()) >= 0.0 and np.abs(m.sum(0) - 1.0).max() <= 2.0 ** -52
    assert base.starts == tuple(starts_ref)
    assert rp.R == R == len(rp.rows) and rp.rows == tuple(rows_ref)
    if cover is not None:
        assert rp.cover == cover
    assert rp.W == base.W and rp.starts == base.starts and rp.base.starts == base.starts and not hasattr(rp.base, "rows")
    assert rp.row_starts == tuple(base.starts[j] for j, _ in rp.rows) and rp.row_prompt == tuple(k for _, k in rp.rows)
    assert list(rp.row_starts) == sorted(rp.row_starts) and rp.row_starts[0] == 0 and rp.row_starts[-1] == key[0] - key[1]
    assert rp.wr.dtype == torch.float32 and tuple(rp.wr.shape) == (R, key[1])
    # fp32 roundings of the fp64 weights of the restatement (one ulp of fp64 of slack in front of the rounding: the summation
    # orders of the two normalisations may differ)
    assert np.abs(rp.wr.numpy().astype(np.float64) - np.asarray(wr_ref)).max() <= 2.0 ** -24
    # over every frame the fp32 weights sum to 1 within 2^-23; rows of non-zero weight per frame: the cover
    total, count = np.zeros(key[0]), np.zeros(key[0], dtype=int)
    for r, s in enumerate(rp.row_starts):
        total[s:s + key[1]] += rp.wr[r].numpy().astype(np.float64)
        count[s:s + key[1]] += rp.wr[r].numpy() != 0.0
    print(f"{key} {bounds} tau={tau}: R={rp.R} cover={rp.cover} max |sum wr - 1| = {np.abs(total - 1.0).max():.2e}")
    assert np.abs(total - 1.0).max() <= 2.0 ** -23
    assert int(count.max()) == rp.cover and int(count.min()) >= 1
    for r, (j, k) in enumerate(rp.rows):
        s = rp.row_starts[r]
        w = rp.wr[r].numpy()
        assert np.all(w[count[s:s + key[1]] == 1][w[count[s:s + key[1]] == 1] != 0.0] == 1.0)    # alone on a frame: exactly 1
        assert np.all(w[m[k, s:s + key[1]] == 0.0] == 0.0) and np.all(w[m[k, s:s + key[1]] != 0.0] > 0.0)   # silent: exactly 0


def test_hard_cuts_on_window_edges_give_weights_of_exactly_one():
    _, rp = Tl.plans_of((48, 16, 16), [16, 32], 0)
    assert rp.rows == ((0, 0), (1, 1), (2, 2)) and bool((rp.wr == 1.0).all())


@pytest.mark.parametrize("key", [(40, 16, 10), (24, 16, 1), (16, 16, 8), (768, 256, 192), (48, 16, 16)])
def test_one_prompt_is_the_plan_itself(key):
    base = window_plan(*key)
    rp = row_plan(base, prompt_weights(key[0], [], 7.0))
    assert rp.R == base.W and rp.row_starts == base.starts and rp.row_prompt == (0,) * base.W and rp.cover == base.cover
    assert torch.equal(rp.wr.view(torch.int32), base.wn.view(torch.int32))


def test_plan_key_is_distinct_from_linear_and_ring_keys():
    base = window_plan(40, 16, 10)
    rp = row_plan(base, prompt_weights(40, [], 0))
    rp2 = row_plan(base, prompt_weights(40, [12, 28], 4))
    rp3 = row_plan(base, prompt_weights(40, [12.5, 27.5], 4))
    keys = {Wn.plan_key(base), Wn.plan_key(window_plan(40, 16, 10, ring=True)), Wn.plan_key(rp), Wn.plan_key(rp2)}
    assert len(keys) == 4 and Wn.plan_key(rp2) == (40, 16, rp2.row_starts, "rows")
    # the same row geometry under other weights: the same key (the weights are a buffer of the cache entry, not of the graph)
    assert rp3.rows == rp2.rows and Wn.plan_key(rp3) == Wn.plan_key(rp2) and not torch.equal(rp3.wr, rp2.wr)
    # boundaries [13, 27] do NOT keep the geometry: prompt 2 then starts at frame 25 (25.5 > 27 - 2), inside window 1 = [10, 26)
    rp4 = row_plan(base, prompt_weights(40, [13, 27], 4))
    assert rp4.R == 9 and (1, 2) in rp4.rows and Wn.plan_key(rp4) != Wn.plan_key(rp2)


def test_row_plan_keeps_a_source():
    base = window_plan(40, 16, 10)
    x0, mask = torch.zeros(2, 8, 40, 8), Wn.keep_mask(40, [(0, 8)])
    m = prompt_weights(40, [12, 28], 4)
    a = Wn.with_source(row_plan(base, m), x0, mask)
    b = row_plan(Wn.with_source(base, x0, mask), m)
    for rp in (a, b):
        assert rp.x0 is x0 and rp.R == 8 and Wn.has_rows(rp) and Wn.plan_key(rp) == Wn.plan_key(row_plan(base, m))
        assert not hasattr(rp.base, "x0") and not Wn.has_rows(rp.base)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds,tau,msg", [([28, 12], 4, "ascend"), ([12, 12], 4, "ascend"), ([0], 4, "inside"), ([40], 4, "inside"),
                                            ([-3], 4, "inside"), ([float("nan")], 4, "inside"), ([12], -1, "transition"),
                                            ([12], float("inf"), "transition"), ([12], float("nan"), "transition"),
                                            ([12], "wide", "numbers"), ([12.2, 12.4], 0, "no frame"), ([12.6, 13.4], 0, "no frame")])
def test_prompt_weights_refusals(bounds, tau, msg):
    with pytest.raises(ValueError, match=msg):
        prompt_weights(40, bounds, tau)


def test_row_plan_refusals():
    base = window_plan(40, 16, 10)
    with pytest.raises(ValueError, match="ring"):
        row_plan(window_plan(40, 16, 10, ring=True), prompt_weights(40, [12], 4))
    with pytest.raises(ValueError, match=r"\[K, T=40\]"):
        row_plan(base, prompt_weights(48, [12], 4))
    with pytest.raises(ValueError, match="sum to 1"):
        row_plan(base, 0.5 * prompt_weights(40, [12], 4))
    m = prompt_weights(40, [12], 0)
    with pytest.raises(ValueError, match="no frame"):
        row_plan(base, np.concatenate([m, np.zeros((1, 40))]))
    with pytest.raises(ValueError, match="already has rows"):
        row_plan(row_plan(base, m), m)


def _three_prompts(t0):
    """Two prompts audible at every frame, a third from frame t0 on: over (40, 16, 1), 25 windows one frame apart, the third adds the
    windows with s + 15 >= t0."""
    m = np.zeros((3, 40))
    m[0], m[1] = 0.5, 0.5
    m[2, t0:], m[0, t0:] = 0.25, 0.25
    return m


def test_more_than_64_rows_is_refused():
    base = window_plan(40, 16, 1)
    assert base.W == 25
    assert row_plan(base, _three_prompts(26)).R == 64          # 50 + the 14 windows with s >= 11
    with pytest.raises(ValueError, match="65 rows"):
        row_plan(base, _three_prompts(25))
    with pytest.raises(ValueError, match="75 rows"):
        row_plan(base, prompt_weights(40, [19, 21], 80))       # three prompts audible everywhere


class _M:
    num_timesteps = 1000
    alphas_cumprod = torch.linspace(0.999, 0.01, 1000)


def test_samplers_refuse_every_mismatch_of_row_plan_and_per_prompt():
    """plan_run refuses before its first device tensor."""
    from audioldm2_amd.sampling import SamplerBase
    s = SamplerBase(_M())
    s.make_schedule(4, verbose=False)
    base = window_plan(40, 16, 10)
    rp = row_plan(base, prompt_weights(40, [12, 28], 4))
    table = lambda n, cfg: torch.zeros(n, 8)
    c = (torch.zeros(2, 3),)
    run = lambda cond, plan: s.plan_run(cond, (2, 8, 40, 8), None, None, None, table, 1.0, None, 0.0, None, None, windows=plan)
    with pytest.raises(ValueError, match="go together"):
        run(c, rp)                                   # a row plan with a plain conditioning
    with pytest.raises(ValueError, match="go together"):
        run([c, c, c], rp)                           # ... with a bare list
    with pytest.raises(ValueError, match="go together"):
        run(PerPrompt([c, c, c]), base)              # a PerPrompt with a plain plan
    with pytest.raises(ValueError, match="go together"):
        run(PerPrompt([c, c, c]), None)              # ... without a plan
    with pytest.raises(ValueError, match="3 prompts"):
        run(PerPrompt([c, c]), rp)
    with pytest.raises(ValueError, match="3 prompts"):
        run(PerPrompt([c, c, c, c]), rp)
    with pytest.raises(ValueError, match="at least one"):
        PerPrompt([])
    with pytest.raises(ValueError, match="go together"):
        rows_cond([c, c, c], rp)


def test_model_output_refuses_a_mismatch_too():
    """A caller that drives model_output with a hand-made `win`: refused before any launch (no tensor here lives on a device)."""
    from types import SimpleNamespace
    from audioldm2_amd.sampling import SamplerBase
    s = SamplerBase(_M())
    base = window_plan(40, 16, 10)
    rp = row_plan(base, prompt_weights(40, [12, 28], 4))
    c = (torch.zeros(2, 3),)
    x, t = torch.zeros(2, 8, 40, 8), torch.zeros(32)
    win = lambda plan, **kw: SimpleNamespace(**dict(dict(plan=plan, blend=False, xw=None, merged=None, n=None, wr=None), **kw))
    with pytest.raises(ValueError, match="needs a row plan"):
        s.model_output(x, t, 2, PerPrompt([c, c, c]), None, False, None)
    with pytest.raises(ValueError, match="needs a row plan"):
        s.model_output(x, t, 2, PerPrompt([c, c, c]), None, False, None, win=win(base, n=base.W))
    with pytest.raises(ValueError, match="3 prompts"):
        s.model_output(x, t, 2, PerPrompt([c, c]), None, False, None, win=win(rp, n=rp.R, wr=rp.wr))
    with pytest.raises(ValueError, match="win.n == plan.R and win.wr"):
        s.model_output(x, t, 2, c, None, False, None, win=win(rp, n=rp.R))
    with pytest.raises(ValueError, match="win.n == plan.R and win.wr"):
        s.model_output(x, t, 2, c, None, False, None, win=win(rp, n=base.W, wr=rp.wr))


# ---- the conditioning order -------------------------------------------------------------------------------------------------------
def test_rows_cond_orders_rows_by_window_then_prompt():
    base = window_plan(40, 16, 10)
    rp = row_plan(base, prompt_weights(40, [12, 28], 4))
    assert rp.row_prompt == (0, 1, 0, 1, 1, 2, 1, 2)
    b = 2
    t = [torch.arange(b * 3, dtype=torch.float32).view(b, 3) + 100 * k for k in range(3)]
    want = torch.cat([t[k] for k in rp.row_prompt])
    assert torch.equal(rows_cond(PerPrompt(t), rp), want)
    for r, k in enumerate(rp.row_prompt):
        for i in range(b):
            assert torch.equal(want[r * b + i], t[k][i])        # row r*b + i is prompt k_r's sample i
    tup = rows_cond(PerPrompt([([x, x + 1], [x + 2]) for x in t]), rp)
    assert isinstance(tup, tuple) and isinstance(tup[0], list) and torch.equal(tup[0][1], want + 1) and torch.equal(tup[1][0], want + 2)
    d = rows_cond(PerPrompt([{"a": x, "b": [x, None], "c": None} for x in t]), rp)
    assert torch.equal(d["a"], want) and torch.equal(d["b"][0], want) and d["b"][1] is None and d["c"] is None
    assert torch.equal(Wn.tile_cond(t[0], rp.R), torch.cat([t[0]] * 8))     # the unconditional half: tiled R times


# ---- seconds to frames ------------------------------------------------------------------------------------------------------------
def test_timeline_frames_maps_seconds_to_latent_frames():
    from audioldm2_amd.pipeline import timeline_frames
    prompts, trans, bounds = timeline_frames([(0.0, "rain"), (12.0, "thunder"), (24.0, "birds", "tweet")], 25.6, 768)
    assert prompts == ["rain", "thunder", "birds"] and trans == ["", "", "tweet"]
    assert bounds == [12.0 * 25.6, 24.0 * 25.6] and abs(bounds[0] - 307.2) < 1e-9
    # 5 s and 0.3 s at 25.6 / s: whole frames in exact arithmetic (128 and 7.68 -> not whole); 1.25 s = frame 32 exactly
    assert timeline_frames([(0, "a"), (5.0, "b")], 25.6, 768)[2] == [128.0]
    assert timeline_frames([(0, "a"), (1.25, "b")], 25.6, 768)[2] == [32.0]
    # 0.1 s at 10 / s is 1 frame in exact arithmetic and 1.0000000000000002 or so in floating point: snapped
    b = timeline_frames([(0, "a"), (0.1 * 3, "b")], 10.0, 80)[2]
    assert b == [3.0] and 0.1 * 3 * 10.0 != 3.0
    for bad, msg in (([], "at least one"), ([(1.0, "a")], "start at 0"), ([(0, "a"), (30.0, "b")], "ascend strictly inside"),
                     ([(0, "a"), (9.0, "b"), (9.0, "c")], "ascend strictly inside"), ([(0, "a"), (float("nan"), "b")], "finite"),
                     ([(0, 7)], "an entry is"), ([(0, "a", "b", "c")], "an entry is"), ([(0, "a"), ("x", "b")], "number of seconds")):
        with pytest.raises(ValueError, match=msg):
            timeline_frames(bad, 25.6, 768)


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

    class Stub(_NoGpu):
        pass
    for name in ("long_form_plans", "generate_batch_long", "generate_batch_long_from_audio", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(Stub, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return Stub()


SCENE = [(0.0, "rain"), (12.0, "thunder"), (24.0, "birds after rain")]


def test_entry_points_refuse_a_bad_timeline_before_any_draw_or_gpu_work():
    from audioldm2_amd.pipeline import extend_audio, make_batch_for_text_to_audio, text_to_audio_long
    ld = _ld_stub()
    for kw, msg in ((dict(text="rain"), "pass text=None"), (dict(transcription="hello"), "pass text=None"),
                    (dict(loop=True), "loop=True"), (dict(ddim_steps=None), "text_to_audio_long needs ddim_steps"),
                    (dict(timeline=[(1.0, "a")]), "start at 0"), (dict(timeline=[(0, "a"), (40.0, "b")]), "ascend strictly inside"),
                    (dict(transition=-1.0), "transition"), (dict(timeline=[(0, "a"), (10.0, "b"), (10.01, "c")], transition=0.0), "no frame")):
        args = dict(dict(text=None, timeline=SCENE, transition=2.0), **kw)
        with pytest.raises(ValueError, match=msg):
            text_to_audio_long(ld, args.pop("text"), 30, **args)
    with pytest.raises(ValueError, match="needs a timeline"):
        text_to_audio_long(ld, "rain", 30, transition=2.0)
    with pytest.raises(ValueError, match="pass text=None"):
        extend_audio(ld, "rain", np.zeros(16000, dtype=np.float32), 30, timeline=SCENE)
    batches = [make_batch_for_text_to_audio(p) for _, p in SCENE]
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for kw, msg in ((dict(loop=True), "loop=True"), (dict(n_gen=2), "n_gen must be 1"), (dict(shard=(0, 2)), "shard"),
                    (dict(ddim_steps=None), "needs ddim_steps"), (dict(boundaries=[300.0]), "2 boundaries"),
                    (dict(boundaries=[600.0, 300.0]), "ascend"), (dict(boundaries=[300.0, 800.0]), "inside"),
                    (dict(transition=float("nan")), "transition")):
        with pytest.raises(ValueError, match=msg):
            ld.generate_batch_long(batches, 768, **dict(dict(boundaries=[307.2, 614.4], transition=51.2), **kw))
        with pytest.raises(ValueError, match=msg):
            ld.generate_batch_long_from_audio(batches, 768, [(0, 200)], **dict(dict(boundaries=[307.2, 614.4], transition=51.2), **kw))
    with pytest.raises(ValueError, match="list of batches"):
        ld.generate_batch_long(batches[0], 768, boundaries=[300.0])
    with pytest.raises(ValueError, match="one size"):
        ld.generate_batch_long([batches[0], make_batch_for_text_to_audio("x", batchsize=2)], 768, boundaries=[300.0])
    with pytest.raises(ValueError, match="at least one batch"):
        ld.generate_batch_long([], 768)
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn
    assert ld.latent_t_size == 256


def test_the_thirty_second_scenes_row_counts():
    """30 s, three prompts, overlap 2.5 s: scenes of 10 s cross-faded over 2.5 s (boundaries 256 and 512, transition 64 frames) cost
    R = 8 rows against W = 4 windows; the scene of the entry point's docstring (12 s, 24 s, 2 s) costs 7 — window 0 hears rain only."""
    from audioldm2_amd.pipeline import timeline_frames
    base = window_plan(768, 256, 192)
    _, _, bounds = timeline_frames([(0.0, "rain"), (10.0, "thunder"), (20.0, "birds after rain")], 25.6, 768)
    assert bounds == [256.0, 512.0]
    assert (base.W, row_plan(base, prompt_weights(768, bounds, 2.5 * 25.6)).R) == (4, 8)
    _, _, bounds = timeline_frames(SCENE, 25.6, 768)
    rp = row_plan(base, prompt_weights(768, bounds, 2.0 * 25.6))
    assert rp.R == 7 and rp.rows[0] == (0, 0) and rp.rows[1] == (1, 0)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
ROW_ENTRIES = ("aldm_window_gather_rows", "aldm_window_merge_rows", "aldm_window_blend_gather_rows")


def test_abi_version_and_symbols():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 22
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    for name in ROW_ENTRIES:
        assert name in lib.EXPORTED_SYMBOLS and hasattr(l, name)
    assert ctypes.sizeof(lib.WindowRows) == 4 * (1 + lib.MAX_ROWS) == 260 and lib.MAX_ROWS == 64 == Wn.MAX_ROWS
    assert ctypes.sizeof(lib.WindowStarts) == 4 * 33                    # the window starts are what they were


def _rows(lib, values, n=None):
    st = lib.WindowRows()
    st.n = len(values) if n is None else n
    for j, s in enumerate(values):
        st.s[j] = s
    return st


def _call_all(l, st, T=40, Tw=16):
    """The three row entries on pointers that are never dereferenced -> their return codes and messages."""
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    a, b, c = ctypes.c_void_p(1 << 32), ctypes.c_void_p(1 << 33), ctypes.c_void_p(1 << 34)
    out = []
    for call in (lambda: l.aldm_window_gather_rows(p, q, st, 2, 3, T, Tw, 5, None),
                 lambda: l.aldm_window_merge_rows(q, p, r, st, 2, 2, 3, T, Tw, 5, None),
                 lambda: l.aldm_window_blend_gather_rows(p, a, b, c, ctypes.c_void_p(1 << 35), None, 1, 1, q, st, 2, 3, T, Tw, 5, None)):
        out.append((call(), l.aldm_last_error().decode()))
    return out


BAD_ROWS = [([], 0, "rows"), ([0] * 64, 65, "rows"), ([0, 12, 10, 24], None, "not decrease"), ([0, 17, 24], None, "exceeds Tw"),
            ([0, 10, 20, 23], None, "last row start"), ([0, 10, 20, 30], None, "last row start"), ([2, 10, 20, 24], None, r"rows[0]"),
            ([0, 0, 10, 10], None, "last row start")]


@pytest.mark.parametrize("values,n,msg", BAD_ROWS, ids=[m + str(len(v)) for v, _, m in BAD_ROWS])
def test_row_entries_refuse_bad_rows_without_a_launch(values, n, msg):
    from audioldm2_amd import lib
    for rc, err in _call_all(lib.load(), _rows(lib, values, n)):
        assert rc < 0 and msg in err


def test_row_entries_refuse_bad_shapes_and_overlap_and_the_window_entries_still_refuse_repeated_starts():
    from audioldm2_amd import lib
    l = lib.load()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    st = _rows(lib, [0, 0, 10, 10, 20, 24, 24])
    for call, msg in ((lambda: l.aldm_window_gather_rows(None, q, st, 2, 3, 40, 16, 5, None), "null"),
                      (lambda: l.aldm_window_gather_rows(p, q, st, 2, 3, 8, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather_rows(p, q, st, 0, 3, 40, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather_rows(p, p, st, 2, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge_rows(q, p, r, st, 3, 2, 3, 40, 16, 5, None), "H=3"),
                      (lambda: l.aldm_window_merge_rows(q, p, q, st, 2, 2, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_merge_rows(q, r, r, st, 2, 2, 3, 40, 16, 5, None), "overlaps"),
                      (lambda: l.aldm_window_blend_gather_rows(p, q, q, q, q, None, 0, 1, r, st, 2, 3, 40, 16, 5, None), "q_rows"),
                      (lambda: l.aldm_window_blend_gather_rows(p, p, q, q, q, None, 1, 1, r, st, 2, 3, 40, 16, 5, None), "overlaps")):
        assert call() < 0
        assert msg in l.aldm_last_error().decode()
    ws = lib.WindowStarts()
    ws.n = 4
    for j, s in enumerate([0, 10, 10, 24]):
        ws.s[j] = s
    assert l.aldm_window_gather(p, q, ws, 2, 4, 3, 40, 16, 5, None) < 0 and "ascend" in l.aldm_last_error().decode()
