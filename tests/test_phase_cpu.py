"""CPU tests of moving window phases: the phase table (golden and explicit), what the golden schedule does to the
depth of every frame of a ring, with_phase and the plan key, the ABI of the three phased entries and their host-side refusals, and the
argument errors of the four entry points, all raised before any draw.  (No kernel is launched here.)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import looped as Lp
import phased as Ph
from test_loop_cpu import _ld_stub, _refused_before_any_draw, _starts
from tolerances import log_err
from audioldm2_amd.windows import keep_mask, plan_key, prompt_weights, row_plan, window_plan, with_source

PHASED_ENTRIES = ("aldm_window_gather_ring_phased", "aldm_window_merge_ring_phased", "aldm_window_blend_gather_ring_phased")


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", Ph.EQUAL_GAP_RINGS + [(40, 16, 14), (24, 16, 1), (384, 256, 128)], ids=str)
@pytest.mark.parametrize("steps", [1, 6, 50, 200])
def test_golden_table_is_the_formula(key, steps):
    from audioldm2_amd.windows import phase_table, ring_gap
    plan = Lp.ring_plan(key)
    G = Ph.gap(plan)
    assert ring_gap(plan) == G
    tab = phase_table(plan, steps, "golden")
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (steps,)
    assert tab.tolist() == Ph.golden_by_hand(G, steps)
    assert int(tab[0]) == 0 and int(tab.min()) >= 0 and int(tab.max()) < G
    # deterministic, and no draw from any generator
    torch.manual_seed(5)
    state = torch.get_rng_state()
    assert torch.equal(phase_table(plan, steps, "golden"), tab) and torch.equal(torch.get_rng_state(), state)


def test_the_golden_table_of_the_sampler_tests():
    from audioldm2_amd.windows import phase_table
    assert phase_table(Lp.ring_plan(Ph.LONG_KEY), Ph.STEPS, "golden").tolist() == Ph.GOLDEN_6
    # the end-to-end ring (384, 256, 128), gap 128: an eager step under 0, the capture under 79, replays under 30 and 109
    assert phase_table(Lp.ring_plan((384, 256, 128)), 4, "golden").tolist() == [0, 79, 30, 109]


def test_explicit_phases_are_reduced_mod_T_and_counted():
    from audioldm2_amd.windows import phase_table
    plan = Lp.ring_plan((40, 16, 10))
    tab = phase_table(plan, 5, [0, 39, 40, -1, 87])
    assert tab.dtype == torch.int32 and tab.tolist() == [0, 39, 0, 39, 7]
    assert phase_table(plan, 2, (np.int64(3), np.int32(41))).tolist() == [3, 1]
    for bad, match in (([0, 1, 2], "3 phases for a run of 5"), ([0] * 6, "6 phases"), ([0, 1, 2, 3, 4.0], "integer"),
                       ([0, 1, 2, 3, True], "integer"), ("silver", "unknown phase schedule"), (7, "sequence")):
        with pytest.raises(ValueError, match=match):
            phase_table(plan, 5, bad)
    for steps in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="steps"):
            phase_table(plan, steps, "golden")
    with pytest.raises(ValueError, match="ring plan"):
        phase_table(window_plan(40, 16, 10), 5, "golden")


# ---- equalisation -------------------------------------------------------------------------------------------------------------------
def test_fixed_ring_has_special_frames():
    """The figures of the issue on the production ring: starts 0, 192, 384, 576."""
    plan = Lp.ring_plan((768, 256, 192))
    d = Ph.depth(plan, 0)
    for s in plan.starts:
        assert int(d[s:s + 64].max()) == 63          # 0-63 past a start: never deeper than 63 inside any window
        assert d[s + 127] == 127 and d[s + 128] == 127          # the middle of a window
    count = np.zeros(plan.T, dtype=int)
    for s in plan.starts:
        count[(s + np.arange(plan.Tw)) % plan.T] += 1
    assert (count == 2).sum() * 3 == plan.T and (count == 1).sum() * 3 == 2 * plan.T          # a third under two, two thirds under one
    assert Ph.depth_spread(plan, [0]) == 127 - int(d.min())


@pytest.mark.parametrize("key", Ph.EQUAL_GAP_RINGS, ids=str)
@pytest.mark.parametrize("steps", Ph.EQUALISE_STEPS)
def test_golden_phases_equalise_the_depth(key, steps):
    from audioldm2_amd.windows import phase_table
    plan = Lp.ring_plan(key)
    tab = phase_table(plan, steps, "golden").tolist()
    fixed = Ph.depth_spread(plan, [0])
    assert fixed > 0 and Ph.depth_spread(plan, [0] * steps) == fixed
    whole = Ph.depth_spread(plan, tab) / fixed
    halves = [Ph.depth_spread(plan, tab[:steps // 2]) / fixed, Ph.depth_spread(plan, tab[steps // 2:]) / fixed]
    print(f"ring {key}, {steps} steps: spread of the step-mean depth / the fixed plan's: whole {whole:.4f} (bar {Ph.WHOLE_BAR}), "
          f"halves {halves[0]:.4f} {halves[1]:.4f} (bar {Ph.HALF_BAR})")
    log_err(whole, Ph.WHOLE_BAR, f"phase equalise {key} S={steps} whole")
    log_err(max(halves), Ph.HALF_BAR, f"phase equalise {key} S={steps} halves")
    assert whole <= Ph.WHOLE_BAR
    assert max(halves) <= Ph.HALF_BAR


# ---- with_phase and the key -----------------------------------------------------------------------------------------------------------
def test_with_phase_and_plan_key():
    from audioldm2_amd.windows import has_phase, phase_table, with_phase
    for key in [(40, 16, 10), (768, 256, 192), (16, 16, 8)]:
        ring, lin = window_plan(*key, ring=True), window_plan(*key)
        a, b = with_phase(ring, phase_table(ring, 6, "golden")), with_phase(ring, torch.tensor([5, 4, 3, 2, 1, 0]))
        assert has_phase(a) and not has_phase(ring) and not has_phase(lin)
        assert plan_key(a) == (ring.T, ring.Tw, ring.starts, "phased") == plan_key(b)          # two tables of one length: one key
        assert plan_key(a) == plan_key(with_phase(ring, [0]))                                   # ... the length is the graph key's
        assert plan_key(a) not in (plan_key(ring), plan_key(lin))
        assert plan_key(ring) == (ring.T, ring.Tw, ring.starts, True) and plan_key(lin) == (lin.T, lin.Tw, lin.starts, False)
        assert a.phase.dtype == torch.int32 and a.ring is True and a.starts == ring.starts and a.wn is ring.wn
        assert not hasattr(ring, "phase")                                                        # a copy: the ring is untouched
    lin = window_plan(40, 16, 10)
    rp = row_plan(lin, prompt_weights(40, [20], 4))
    ring = window_plan(40, 16, 10, ring=True)
    assert plan_key(with_phase(ring, [1, 2])) != plan_key(rp)
    # values are reduced mod T on the host: the kernels clamp
    assert with_phase(ring, torch.tensor([40, -1, 87])).phase.tolist() == [0, 39, 7]
    # composes with with_source either way round
    x0, m = torch.zeros(1, 2, 40, 4), keep_mask(40, [(0, 13)])
    tab = phase_table(ring, 6, "golden")
    one, two = with_source(with_phase(ring, tab), x0, m), with_phase(with_source(ring, x0, m, graded=True), tab)
    for q in (one, two):
        assert has_phase(q) and q.x0 is x0 and torch.equal(q.phase, tab) and plan_key(q) == (40, 16, ring.starts, "phased")
    assert one.graded is False and two.graded is True
    # refusals
    with pytest.raises(ValueError, match="ring plan"):
        with_phase(lin, tab)
    with pytest.raises(ValueError, match="row plan"):
        with_phase(rp, tab)
    for bad in (torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4), torch.tensor(3), [0.5, 1.0], "golden", None):
        with pytest.raises(ValueError, match="1-D integer"):
            with_phase(ring, bad)
    for empty in (torch.zeros(0, dtype=torch.int32), []):
        with pytest.raises(ValueError, match="empty|1-D integer"):
            with_phase(ring, empty)
    with pytest.raises(ValueError, match="ring plan"):
        row_plan(with_phase(ring, tab), prompt_weights(40, [20], 4))          # timelines keep refusing rings, phased or not


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbols():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 25
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    for name in PHASED_ENTRIES:
        assert name in lib.EXPORTED_SYMBOLS and hasattr(l, name)
        # the ring sibling's argument list plus the table, its row count and (gather, merge) the counter
        extra = 2 if name == "aldm_window_blend_gather_ring_phased" else 3
        assert len(lib._SIGS[name][1]) == len(lib._SIGS[name[:-len("_phased")]][1]) + extra
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__))), "include", "aldm_hip.h")) as f:
        header = f.read()
    for name in PHASED_ENTRIES:
        assert f"int {name}(" in header


P, Q, R, TAB = (ctypes.c_void_p(v) for v in (4096, 1 << 30, 1 << 31, 1 << 20))


def _calls(l, st, W, tab=TAB, rows=6, T=40, x=P, win=Q, out=R):
    return {"gather": lambda: l.aldm_window_gather_ring_phased(x, win, st, tab, None, rows, 2, W, 3, T, 16, 5, None),
            "merge": lambda: l.aldm_window_merge_ring_phased(win, P, out, st, tab, None, rows, 2, 2, W, 3, T, 16, 5, None),
            "blend": lambda: l.aldm_window_blend_gather_ring_phased(x, R, R, R, R, None, 1, 1, win, st, tab, rows, 2, W, 3, T, 16, 5,
                                                                    None)}


BAD_RING_STARTS = [([0, 12, 10, 30], None, "ascend"), ([0, 17, 30], None, "exceeds Tw"), ([0, 10, 20, 23], None, "wrap"),
                   ([0, 10, 20, 30], 3, "starts"), ([2, 10, 20, 30], None, r"starts\[0\]"), ([0, 10, 20, 40], None, "below T"),
                   ([0], None, "2 <= W")]


@pytest.mark.parametrize("values,n,msg", BAD_RING_STARTS, ids=[m + str(i) for i, (_, _, m) in enumerate(BAD_RING_STARTS)])
def test_phased_entries_refuse_bad_starts_as_the_ring_entries_do(values, n, msg):
    """The data pointers are never dereferenced: validation fails first."""
    import re
    from audioldm2_amd import lib
    l = lib.load()
    st = _starts(lib, values, n)
    for name, call in _calls(l, st, len(values)).items():
        assert call() < 0, name
        err = l.aldm_last_error().decode()
        assert re.search(msg, err) and "_ring_phased" in err, (name, err)


def test_phased_entries_refuse_a_null_table_no_rows_and_overlap():
    from audioldm2_amd import lib
    l = lib.load()
    st = _starts(lib, [0, 10, 20, 30])
    for name, call in _calls(l, st, 4, tab=None).items():
        assert call() < 0 and "null phase table" in l.aldm_last_error().decode(), name
    for rows in (0, -2):
        for name, call in _calls(l, st, 4, rows=rows).items():
            assert call() < 0 and "rows=" in l.aldm_last_error().decode(), name
    # the table inside a written buffer: win (gather, blend), x (blend), out (merge); its last byte counts
    n_win = 4 * 2 * 3 * 16 * 5
    inside_win = ctypes.c_void_p((1 << 30) + 4 * (n_win - 1))
    c = _calls(l, st, 4, tab=inside_win, rows=1)
    for name in ("gather", "blend"):
        assert c[name]() < 0 and "phase_tab" in l.aldm_last_error().decode(), name
    assert _calls(l, st, 4, tab=ctypes.c_void_p(4096 + 8), rows=1)["blend"]() < 0 and "phase_tab" in l.aldm_last_error().decode()
    assert _calls(l, st, 4, tab=ctypes.c_void_p((1 << 31) + 16), rows=2)["merge"]() < 0 and "phase_tab" in l.aldm_last_error().decode()
    # ... and the siblings' own rules still hold
    for call, msg in ((lambda: l.aldm_window_gather_ring_phased(None, Q, st, TAB, None, 6, 2, 4, 3, 40, 16, 5, None), "null pointer"),
                      (lambda: l.aldm_window_gather_ring_phased(P, Q, st, TAB, None, 6, 2, 4, 3, 8, 16, 5, None), "bad shape"),
                      (lambda: l.aldm_window_gather_ring_phased(P, P, st, TAB, None, 6, 2, 4, 3, 40, 16, 5, None), "overlaps x"),
                      (lambda: l.aldm_window_merge_ring_phased(Q, P, R, st, TAB, None, 6, 3, 2, 4, 3, 40, 16, 5, None), "H=3"),
                      (lambda: l.aldm_window_merge_ring_phased(Q, P, Q, st, TAB, None, 6, 2, 2, 4, 3, 40, 16, 5, None), "overlaps win"),
                      (lambda: l.aldm_window_blend_gather_ring_phased(P, R, R, R, R, None, 0, 1, Q, st, TAB, 6, 2, 4, 3, 40, 16, 5, None),
                       "q_rows"),
                      (lambda: l.aldm_window_blend_gather_ring_phased(P, P, R, R, R, None, 1, 1, Q, st, TAB, 6, 2, 4, 3, 40, 16, 5, None),
                       "x overlaps")):
        assert call() < 0
        assert msg in l.aldm_last_error().decode()


# ---- the entry points' argument errors: raised before any draw ------------------------------------------------------------------------
def test_phase_argument_errors_are_raised_before_any_draw():
    from audioldm2_amd.pipeline import LatentDiffusion, extend_audio, make_batch_for_text_to_audio, text_to_audio_long
    for fn in (LatentDiffusion.generate_batch_long, LatentDiffusion.generate_batch_long_from_audio, text_to_audio_long, extend_audio):
        assert inspect.signature(getattr(fn, "__wrapped__", fn)).parameters["phase"].default is None
    ld = _ld_stub()
    batch = make_batch_for_text_to_audio("rain")
    wav = np.zeros(16000, dtype=np.float32)
    entries = {"generate_batch_long": lambda **kw: ld.generate_batch_long(batch, 384, hop=128, **kw),
               "generate_batch_long_from_audio": lambda **kw: ld.generate_batch_long_from_audio(batch, 384, [(0, 128)], hop=128, **kw),
               "text_to_audio_long": lambda **kw: text_to_audio_long(ld, "rain", 15, overlap=5.0, **kw),
               "extend_audio": lambda **kw: extend_audio(ld, "rain", wav, 15, overlap=5.0, **kw)}
    for name, entry in entries.items():
        _refused_before_any_draw(lambda: entry(phase="golden", ddim_steps=4), "needs loop=True")
        _refused_before_any_draw(lambda: entry(phase=[0, 1, 2, 3], ddim_steps=4, loop=False), "needs loop=True")
        _refused_before_any_draw(lambda: entry(phase="silver", ddim_steps=4, loop=True), "unknown phase schedule")
        _refused_before_any_draw(lambda: entry(phase=[0, 1, 2], ddim_steps=4, loop=True), "3 phases for ddim_steps=4")
        _refused_before_any_draw(lambda: entry(phase=[0] * 5, ddim_steps=4, loop=True), "5 phases for ddim_steps=4")
        _refused_before_any_draw(lambda: entry(phase=7, ddim_steps=4, loop=True), "list of integers")
    assert ld.latent_t_size == 256
