"""Composable guidance on the GPU (ops.cfg_compose_indexed, the four samplers, the G-group UNet pass, text_to_audio(compose=...);
DESIGN.md 9m):

 1. the kernel against its fp64 restatement at the four group shapes of tests/composed.py and one n just above a grid pass per
    path, K in {1, 2, 8}, aligned and one float off (the scalar path): |out - ref| <= (K+1) 2^-24 sum_g |c_g eps_g| elementwise; the
    pair's first half bitwise group 0, in place bitwise out of place, pair = 0 writing n floats and no more;
 2. K = 1, w = 1 is bitwise eps[1]; a NaN group under a zero weight is not read; the counter selects the row, clamped; a captured
    [compose ; step_advance] walks the rows and equals the eager launches bitwise;
 3. DDIM, PLMS, DPM-Solver++ 2M and SDE on the tiny UNet under K = 2 against the fp64 composition loop of tests/composed.py — constant
    weights and a per-step schedule — at 4 x (torch fp32 per-step error) x steps; Composed([cond], [1.0]) bitwise the plain job, with
    and without guidance rescale; eager bitwise the graph; other weights move the result;
 4. window plans (linear, ring, phased ring; linear with a source under resample=) against the same loop at the windowed tests' bar;
 5. on a LatentDiffusion at a 64 x 16 latent: the G = 3 group pass with the shared prefix against the repeated-x pass; two composed
    DDIM jobs of one K through one cached graph and a plain job after them; text_to_audio(compose=...) end to end.

Measured on an MI355X (every printed figure: profiles/r25_compose_errors.txt): (1) the largest ratio to the kernel's bound over the 26
calls is 0.77; (3) sampler vs the fp64 loop, max-norm, constant / schedule weights, each under a bar of 3.7e-6 to 8.8e-6: DDIM 2.2e-7 /
8.1e-7, PLMS 3.6e-7 / 5.8e-7, 2M 3.5e-7 / 7.5e-7, SDE 6.3e-7 / 1.1e-6; (4) 4.9e-7 to 9.6e-7 relative rms (bar 1e-5); (5) the G = 3 pass
1.3e-6 (bar 1e-5).
"""
import json
import os

import numpy as np
import pytest
import torch

import audio2audio as A
import composed as Cp
from oracle import cases, weights
from tolerances import log_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GS = Cp.GS
bits = Cp.bits


def counter(v):
    return torch.full((1,), v, device="cuda", dtype=torch.int32)


def place(t, aligned):
    t = t.cuda()
    if aligned:
        assert t.data_ptr() % 16 == 0
        return t
    v = Cp.off_by_one_float(t)
    assert v.data_ptr() % 16 == 4
    return v


def check_against_fp64(eps, tab, out_c, K, what):
    ref, mag = Cp.compose_fp64(eps, tab[0])
    err = (out_c.double() - ref).abs()
    ratio = float((err / (Cp.kernel_bar(K) * mag).clamp_min(1e-300)).max())
    print(f"compose {what}: largest |out - ref| / ((K+1) 2^-24 sum|c_g eps_g|) = {ratio:.3f}")
    assert bool((err <= Cp.kernel_bar(K) * mag).all()), (what, ratio)
    return log_err(ratio, 1.0, f"compose kernel {what}")


# ---- 1. the kernel vs fp64, the pair, in place, the guard -----------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off-by-one-float"])
@pytest.mark.parametrize("K", Cp.KERNEL_KS)
@pytest.mark.parametrize("shape", Cp.KERNEL_SHAPES, ids=["1024", "1003", "3", "4100"])
def test_kernel_matches_fp64_and_the_pair_forms_agree(shape, K, aligned):
    from audioldm2_amd import ops
    eps_h = Cp.kernel_inputs(K, shape)
    tab = Cp.table_by_hand(Cp.kernel_weights(K)[0].tolist()).cuda()
    eps = place(eps_h, aligned)
    n = eps[0].numel()
    keep = eps.clone()
    out = place(torch.full((2,) + tuple(shape), -777.0), aligned)
    assert ops.cfg_compose_indexed(eps, tab, None, pair=True, out=out) is out
    assert torch.equal(bits(eps), bits(keep))                                        # out of place: the operand is untouched
    check_against_fp64(eps, tab, out[1], K, f"{tuple(shape)} K={K} aligned={aligned}")
    assert torch.equal(bits(out[0]), bits(eps[0]))                                   # the first half: group 0, bit for bit
    # pair = 0 writes n floats: the n behind them stay what they were
    single = place(torch.full((2,) + tuple(shape), -777.0), aligned)
    got = ops.cfg_compose_indexed(eps, tab, None, pair=False, out=single[0])
    assert torch.equal(bits(got), bits(out[1])) and bool((single[1] == -777.0).all())
    # in place equals out of place, group 0 is not rewritten and the groups behind the pair are not touched
    work = place(eps_h, aligned)
    res = ops.cfg_compose_indexed(work, tab, None, pair=True)
    assert res.data_ptr() == work.data_ptr() and tuple(res.shape) == (2,) + tuple(shape)
    assert torch.equal(bits(res), bits(out)) and torch.equal(bits(work[2:]), bits(keep[2:]))
    work = place(eps_h, aligned)
    res = ops.cfg_compose_indexed(work, tab, None, pair=False)
    assert res.data_ptr() == work.data_ptr() and torch.equal(bits(res), bits(out[1])) and torch.equal(bits(work[1:]), bits(keep[1:]))
    assert n == int(np.prod(shape))


@pytest.mark.parametrize("path", ["scalar", "vec4"])
def test_one_n_above_a_grid_pass_runs_the_stride_loop_twice(path):
    """The launch caps its grid at 8192 x 256 threads: the elements past one grid pass are the loop's second trip."""
    from audioldm2_amd import ops
    n, K = Cp.STRIDE_N[path], 1
    assert n > Cp.GRID_THREADS * (4 if path == "vec4" else 1) and (n % 4 == 0) == (path == "vec4")
    g = torch.Generator(device="cuda").manual_seed(5)
    eps = torch.randn((K + 1, n), device="cuda", generator=g)
    tab = Cp.table_by_hand([0.75]).cuda()
    out = ops.cfg_compose_indexed(eps, tab, None, pair=True, out=torch.empty((2, n), device="cuda"))
    check_against_fp64(eps, tab, out[1], K, f"n={n} ({path})")
    assert torch.equal(bits(out[0]), bits(eps[0]))
    assert torch.equal(bits(ops.cfg_compose_indexed(eps, tab, None, pair=True)), bits(out))


# ---- 2. identity, the zero-weight skip, the counter, the graph -------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off-by-one-float"])
@pytest.mark.parametrize("shape", Cp.KERNEL_SHAPES, ids=["1024", "1003", "3", "4100"])
def test_one_prompt_of_weight_one_is_bitwise_its_group(shape, aligned):
    from audioldm2_amd import ops
    from audioldm2_amd.sampling import Composed, compose_table
    eps = place(Cp.kernel_inputs(1, shape), aligned)
    tab = compose_table(Composed([None], [1.0]).weights).cuda()
    assert tab.tolist() == [[0.0, 1.0]]
    out = ops.cfg_compose_indexed(eps, tab, None, pair=True, out=torch.empty((2,) + tuple(shape), device="cuda"))
    assert torch.equal(bits(out), bits(eps))
    assert torch.equal(bits(ops.cfg_compose_indexed(eps, tab, None, pair=False, out=torch.empty(shape, device="cuda"))), bits(eps[1]))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off-by-one-float"])
@pytest.mark.parametrize("shape", [Cp.KERNEL_SHAPES[0], Cp.KERNEL_SHAPES[1]], ids=["1024", "1003"])
def test_a_group_under_a_zero_weight_is_not_read(shape, aligned):
    from audioldm2_amd import ops
    K = 3
    eps_h = Cp.kernel_inputs(K, shape)
    w = Cp.kernel_weights(K)[0].tolist()
    # prompt 2 (group 2) gets weight 0 and NaN: the result is the K - 1 call without that group, c_0 being 1 - the same sum
    w0 = [w[0], 0.0, w[2]]
    bad = eps_h.clone()
    bad[2] = float("nan")
    out = ops.cfg_compose_indexed(place(bad, aligned), Cp.table_by_hand(w0).cuda(), None, pair=True,
                                  out=torch.empty((2,) + tuple(shape), device="cuda"))
    less = ops.cfg_compose_indexed(place(eps_h[[0, 1, 3]].contiguous(), aligned), Cp.table_by_hand([w[0], w[2]]).cuda(), None,
                                   pair=True, out=torch.empty((2,) + tuple(shape), device="cuda"))
    assert bool(torch.isfinite(out).all()) and torch.equal(bits(out), bits(less))
    # weights that sum to 1: c_0 == 0, a NaN unconditional group does not reach e_c (the pair's first half is that group, so pair = 0)
    w1 = [1.5, -0.25, -0.25]
    tab1 = Cp.table_by_hand(w1).cuda()
    assert float(tab1[0, 0]) == 0.0
    bad = eps_h.clone()
    bad[0] = float("nan")
    out = ops.cfg_compose_indexed(place(bad, aligned), tab1, None, pair=False, out=torch.empty(shape, device="cuda"))
    clean = ops.cfg_compose_indexed(place(eps_h, aligned), tab1, None, pair=False, out=torch.empty(shape, device="cuda"))
    assert bool(torch.isfinite(out).all()) and torch.equal(bits(out), bits(clean))
    # ... and a NaN under a weight does arrive
    w0[1] = 1e-3
    out = ops.cfg_compose_indexed(place(eps_h.clone().index_fill_(0, torch.tensor([2]), float("nan")), aligned),
                                  Cp.table_by_hand(w0).cuda(), None, pair=False, out=torch.empty(shape, device="cuda"))
    assert bool(torch.isnan(out).all())


def test_the_counter_selects_the_row_clamped_and_is_not_written():
    from audioldm2_amd import ops
    K, shape = 2, Cp.KERNEL_SHAPES[1]
    eps = Cp.kernel_inputs(K, shape).cuda()
    tab = Cp.table_by_hand(Cp.kernel_weights(K, rows=3).tolist()).cuda()
    per_row = [ops.cfg_compose_indexed(eps, tab[r:r + 1].contiguous(), None, pair=True, out=torch.empty((2,) + shape, device="cuda"))
               for r in range(3)]
    assert not torch.equal(per_row[0], per_row[1]) and not torch.equal(per_row[1], per_row[2])
    for value, row in ((-1, 0), (0, 0), (1, 1), (2, 2), (7, 2)):
        idx = counter(value)
        out = ops.cfg_compose_indexed(eps, tab, idx, pair=True, out=torch.empty((2,) + shape, device="cuda"))
        assert torch.equal(bits(out), bits(per_row[row])), (value, row)
        assert int(idx) == value
    out = ops.cfg_compose_indexed(eps, tab, None, pair=True, out=torch.empty((2,) + shape, device="cuda"))      # NULL: row 0
    assert torch.equal(bits(out), bits(per_row[0]))


def test_a_captured_compose_and_advance_walks_the_rows_and_equals_eager():
    from audioldm2_amd import ops
    from audioldm2_amd.sampling import GraphStepper
    K, shape, rows = 2, Cp.KERNEL_SHAPES[0], 3
    eps = Cp.kernel_inputs(K, shape).cuda()
    tab = Cp.table_by_hand(Cp.kernel_weights(K, rows=rows).tolist()).cuda()
    t_tab = torch.arange(rows, dtype=torch.float32, device="cuda").view(rows, 1).contiguous()

    def run(use_graph):
        idx, t_cur, out = counter(0), t_tab[0].clone(), torch.empty((2,) + shape, device="cuda")
        seen = []

        def step():
            ops.cfg_compose_indexed(eps, tab, idx, pair=True, out=out)
            ops.step_advance(idx, t_tab, t_cur)
        stepper = GraphStepper(step, use_graph)
        for _ in range(rows):
            stepper()
            seen.append(out.clone())
        torch.cuda.synchronize()
        graph = stepper.graph is not None
        stepper.release()
        return seen, graph
    eager, g0 = run(False)
    replay, g1 = run(True)
    assert not g0 and g1
    for r in range(rows):
        want = ops.cfg_compose_indexed(eps, tab, counter(r), pair=True, out=torch.empty((2,) + shape, device="cuda"))
        assert torch.equal(bits(eager[r]), bits(want)) and torch.equal(bits(replay[r]), bits(want)), r


def test_the_wrapper_refuses_what_it_cannot_run():
    from audioldm2_amd import ops
    eps = Cp.kernel_inputs(2, Cp.KERNEL_SHAPES[0]).cuda()
    tab = Cp.table_by_hand([1.0, -0.5]).cuda()
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.cfg_compose_indexed(eps.cpu(), tab)
    with pytest.raises(RuntimeError, match="w_tab"):
        ops.cfg_compose_indexed(eps, tab[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.cfg_compose_indexed(eps, tab, counter(0).long())
    with pytest.raises(RuntimeError, match="cfg_compose.out"):
        ops.cfg_compose_indexed(eps, tab, out=torch.empty_like(eps[0]))
    with pytest.raises(RuntimeError, match="overlaps eps"):
        ops.cfg_compose_indexed(eps, tab, out=eps[1:3])
    with pytest.raises(RuntimeError, match="K"):
        ops.cfg_compose_indexed(eps[:1], tab[:, :1].contiguous())


# ---- 3. the samplers on the tiny UNet ---------------------------------------------------------------------------------------------------
KINDS = ["ddim", "plms", "dpmpp", "sde"]
W2 = [1.0, -0.5]
SCHEDULE7 = [[1.0 - 0.05 * i, -0.5 + 0.1 * i] for i in range(7)]


@pytest.fixture(scope="module")
def tiny():
    """The tiny model with a group pass (composed.group_model: one UNet pass over the K+1 groups, for two groups the launches of its
    apply_model_cfg), two prompts' conditionings and the unconditional one."""
    return Cp.group_model(), [Cp.conditioning(1), Cp.conditioning(3)], Cp.conditioning(2)


@pytest.fixture(scope="module")
def tiny_sequential():
    """The same weights on a model WITHOUT apply_model_groups: the samplers make K+1 sequential apply_model calls and stack them."""
    m = A.TinyModel()
    assert not hasattr(m, "apply_model_groups")
    return m


def x_T(seed=3, shape=Cp.TINY_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("weights_", [W2, SCHEDULE7], ids=["constant", "schedule"])
@pytest.mark.parametrize("kind", KINDS)
def test_sampler_matches_the_fp64_composition_loop(tiny, tiny_sequential, kind, weights_):
    """S = 6 makes seven steps: the first runs eagerly, the graph is captured at the next replayable step and replayed after.  The
    constant weights run on the model without a group pass (K+1 sequential calls), the schedule on the one with it."""
    from audioldm2_amd.sampling import Composed, compose_table, make_ddim_timesteps
    m, conds, uncond = tiny
    if weights_ is W2:
        m = tiny_sequential
    ts = make_ddim_timesteps("uniform", 6, 1000, verbose=False)
    steps = len(ts)
    assert steps == 7
    c = Composed(conds, weights_)
    tab = compose_table(c.weights, steps)
    assert tab.shape[0] == (1 if weights_ is W2 else steps)
    _, z = Cp.draws(kind, Cp.TINY_SHAPE, steps, False)
    ref, e32 = Cp.fp64_loop(kind, Cp.Passes(m, conds, uncond, tab), m.alphas_cumprod, ts, x_T(), eta=1.0 if kind == "sde" else 0.0, z=z)
    out = Cp.run_sampler(kind, m, c, uncond, 6, x_T())
    ex, bar = Cp.relmax(out, ref), 4 * e32 * steps
    print(f"composed {kind} sampler, K = 2, {'schedule' if weights_ is not W2 else 'constant'} weights, 7 steps: x {ex:.2e}  "
          f"torch fp32 per step {e32:.2e}  bar {bar:.2e}")
    assert log_err(ex, bar, f"composed {kind} sampler x") <= bar


@pytest.mark.parametrize("kind", KINDS)
def test_one_prompt_of_weight_one_is_bitwise_the_plain_job_and_eager_is_bitwise_the_graph(tiny, kind, monkeypatch):
    from audioldm2_amd.sampling import Composed
    m, conds, uncond = tiny
    for kw in ({}, dict(guidance_rescale=0.7)):
        plain = Cp.run_sampler(kind, m, conds[0], uncond, 6, x_T(), **kw)
        one = Cp.run_sampler(kind, m, Composed([conds[0]], [1.0]), uncond, 6, x_T(), **kw)
        assert torch.equal(bits(one), bits(plain)), kw
    # no guidance (scale 1): pair = 0, the composed prediction alone — K = 1, w = 1 is the unguided job.  That job runs its UNet on b
    # rows and this one on the 2b rows of its two groups (c_0 == 0: the unconditional rows are computed and not read), so the two
    # agree as one computation at two batch sizes does, at the project's bar of a short run's latent, not bitwise
    plain1 = Cp.run_sampler(kind, m, conds[0], uncond, 6, x_T(), gs=1.0)
    one1 = Cp.run_sampler(kind, m, Composed([conds[0]], [1.0]), uncond, 6, x_T(), gs=1.0)
    e1 = A.rel_rms(one1, plain1)
    print(f"composed {kind}, scale 1, K = 1, w = 1 vs the unguided job: {e1:.2e}  bar {A.tstart_bar(7):.1e}")
    assert log_err(e1, A.tstart_bar(7), f"composed {kind} scale 1") <= A.tstart_bar(7) and A.rel_rms(plain1, plain) > 1e-3
    mix = Cp.run_sampler(kind, m, Composed(conds, SCHEDULE7), uncond, 6, x_T(), guidance_rescale=0.7)
    other = Cp.run_sampler(kind, m, Composed(conds, [0.3, 0.9]), uncond, 6, x_T(), guidance_rescale=0.7)
    d = Cp.relmax(other, mix)
    print(f"composed {kind}: other weights move the 7-step latent by {d:.2e} of its maximum")
    assert d > 1e-3 and Cp.relmax(mix, plain) > 1e-3
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    eager = Cp.sampler_class(kind)(m)
    assert not eager.use_graph
    mix_e = Cp.run_sampler(kind, m, Composed(conds, SCHEDULE7), uncond, 6, x_T(), sampler=eager, guidance_rescale=0.7)
    assert torch.equal(bits(mix), bits(mix_e)), "graph replay and eager launches must agree bitwise"


def test_a_composed_run_needs_an_unconditional_conditioning(tiny):
    from audioldm2_amd.sampling import Composed
    m, conds, _ = tiny
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="unconditional conditioning"):
        Cp.sampler_class("ddim")(m).sample(6, 2, Cp.TINY_SHAPE[1:], Composed(conds, W2), verbose=False, eta=0.0,
                                           unconditional_guidance_scale=GS)
    with pytest.raises(ValueError, match="weight schedule has 5 rows"):
        Cp.sampler_class("ddim")(m).sample(6, 2, Cp.TINY_SHAPE[1:], Composed(conds, SCHEDULE7[:5]), verbose=False, eta=0.0,
                                           unconditional_guidance_scale=GS, unconditional_conditioning=conds[0])
    assert torch.equal(torch.get_rng_state(), state)


# ---- 4. window plans ------------------------------------------------------------------------------------------------------------------------
def long_x(seed=3):
    return torch.randn(Cp.LONG_SHAPE, generator=torch.Generator().manual_seed(seed))


def window_case(name):
    """-> (the plan the sampler gets, the plan the loop slices by, the loop's phase table or None, (x0, mask4) or None, resample)."""
    import long_source as Ls
    import looped as Lp
    import phased as Ph
    from audioldm2_amd.windows import keep_mask, phase_table, window_plan, with_phase, with_source
    linear, ring = window_plan(*Cp.LONG_KEY), Lp.ring_plan(Cp.LONG_KEY)
    if name == "linear":
        return linear, linear, None, None, None
    if name == "ring":
        return ring, ring, None, None, None
    if name == "phased ring":
        tab = phase_table(ring, Cp.STEPS, "golden")
        assert tab.tolist() == Ph.GOLDEN_6
        return with_phase(ring, tab), ring, Ph.GOLDEN_6, None, None
    x0 = torch.randn(Cp.LONG_SHAPE, generator=torch.Generator().manual_seed(5)).cuda()
    mask = keep_mask(Cp.LONG_KEY[0], Ls.KEEP)
    return with_source(linear, x0, mask), linear, None, (x0, mask.view(1, 1, -1, 1).expand(Cp.LONG_SHAPE).contiguous()), (2, 2)


WINDOW_CASES = [(k, n) for n in ("linear", "ring", "phased ring") for k in KINDS] + [("ddim", "linear source resample")]


@pytest.mark.parametrize("kind,name", WINDOW_CASES, ids=[f"{k}-{n.replace(' ', '-')}" for k, n in WINDOW_CASES])
def test_windowed_composed_sampler_equals_the_composition_loop(tiny, kind, name):
    from audioldm2_amd.sampling import Composed, compose_table, make_ddim_timesteps, resample_visits
    m, conds, uncond = tiny
    plan, base, phase, source, resample = window_case(name)
    steps = Cp.STEPS
    # the resampled run takes a schedule, so that a visit's row is its loop position's and not the visit's own number
    w = W2 if resample is None else SCHEDULE7[:steps]
    c = Composed(conds, w)
    visits = None if resample is None else resample_visits(steps, *resample)
    kw = {} if resample is None else dict(resample=resample)
    out = Cp.run_sampler(kind, m, c, uncond, steps, long_x(), shape=Cp.LONG_SHAPE, windows=plan, t_start=steps, **kw)
    q, z = Cp.draws(kind, Cp.LONG_SHAPE, steps if visits is None else len(visits), source is not None)
    ts = make_ddim_timesteps("uniform", steps, 1000, verbose=False)[:steps]
    passes = Cp.Passes(m, conds, uncond, compose_table(c.weights, steps), plan=base, phase=phase)
    ref, _ = Cp.fp64_loop(kind, passes, m.alphas_cumprod, ts, long_x(), eta=1.0 if kind == "sde" else 0.0, z=z, q=q, source=source,
                          visits=visits)
    e, bar = A.rel_rms(out, ref), A.tstart_bar(steps)
    print(f"composed {kind} windows [{name}] K = 2, {steps} steps vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert bar == 1e-5 or os.environ.get("ALDM_MMA", "") not in ("", "bf16x6")
    assert tuple(out.shape) == Cp.LONG_SHAPE and bool(torch.isfinite(out).all())
    assert log_err(e, bar, f"composed {kind} windowed [{name}]") <= bar
    assert A.rel_rms(out, long_x().cuda()) > 1e-3


# ---- 5. LatentDiffusion at a small latent --------------------------------------------------------------------------------------------------
LATENT_T = 64


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    ld = build_model(model_name="audioldm2-full")
    with open(os.path.join(GOLD, "e2e_statedict_keys.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = weights.make_state_dict(shapes, seed=0)
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    ld.load_state_dict(sd, strict=False)
    return ld.cuda()


def seeded_conditionings(ld, B, seeds):
    """The model's own conditioning of a B-prompt batch with every context replaced by seeded normals: conditionings that differ as
    much as noise does (the synthetic conditioners of this fixture do not read the text) -> ([one per seed], the unconditional one)."""
    base = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B) for k, m in ld.cond_stage_model_metadata.items()}

    def synth(c, g):
        if torch.is_tensor(c):
            return torch.randn(c.shape, generator=g).to(c.device) if c.dim() == 3 else c       # contexts [B, L, D]; masks stay
        if isinstance(c, dict):
            return {k: synth(v, g) for k, v in c.items()}
        return type(c)(synth(v, g) for v in c)
    return [synth(base, torch.Generator().manual_seed(s)) for s in seeds], uncond


def test_the_group_pass_with_the_shared_prefix_equals_the_repeated_pass(ld):
    """G = 3 groups on audioldm2-full (the smallest shipped config whose _shared_prefix_end is not None — every cross-attention
    config ends its prefix at input block 4, layer 2): the UNet runs its context-free prefix once for all three groups.  Same values
    as the pass over x repeated three times (ALDM_CFG_SHARE=0) within the bar of the two-group test; per-sample timesteps and the
    padded / masked contexts included."""
    import test_model_gpu as M
    B = 2
    conds, uncond = seeded_conditionings(ld, B, (11, 12))
    unet = ld.model.diffusion_model
    assert unet._shared_prefix_end([torch.zeros(1)] * 2) == (4, 2)
    x = cases.latent_input(B, 8, LATENT_T, 16, seed=21).cuda()
    t = torch.tensor([801.0, 401.0]).repeat(3).cuda()
    prepared = ld.prepare_groups(conds, uncond)
    assert prepared["groups"] == 3 and all(c.shape[0] == 3 * B for c in prepared["ctxs"])
    shared = ld.apply_model_groups(x, t, prepared)
    os.environ["ALDM_CFG_SHARE"] = "0"
    try:
        full = ld.apply_model_groups(x, t, prepared)
    finally:
        os.environ.pop("ALDM_CFG_SHARE")
    assert shared.shape == full.shape == (3, B, 8, LATENT_T, 16)
    e = M.rel(shared, full)
    print(f"G = 3 group pass, shared prefix vs repeated x: {e:.2e}  bar {M.batch_tol():.1e}; groups differ by "
          f"{M.rel(shared[0], shared[1]):.2e} / {M.rel(shared[1], shared[2]):.2e}")
    assert log_err(e, M.batch_tol(), "G=3 shared prefix") < M.batch_tol()
    assert M.rel(shared[0], shared[1]) > 1e-3 and M.rel(shared[1], shared[2]) > 1e-3 and M.rel(shared[0], shared[2]) > 1e-3
    # every group is the single pass under its own conditioning
    for g, c in enumerate([uncond] + conds):
        assert M.rel(shared[g], ld.apply_model(x, t[:B].long(), c)) < M.batch_tol(), g
    # two groups through the same door: today's guided pass, bit for bit
    two = ld.apply_model_groups(x, t[:2 * B], ld.prepare_groups(conds[:1], uncond))
    assert torch.equal(bits(two), bits(ld.apply_model_cfg(x, t[:2 * B], conds[0], uncond)))


def test_two_composed_ddim_jobs_share_one_graph_and_plain_jobs_are_untouched(ld):
    """The cache key carries K and the table's row count, the weight VALUES live in the entry's table, refilled per job: a second job
    with other weights on the cached graph equals that job on a model with nothing cached, and a plain job after a composed one equals
    a plain job on a model with nothing cached — all bitwise."""
    from audioldm2_amd.sampling import Composed
    unet = ld.model.diffusion_model
    B = 2
    conds, uncond = seeded_conditionings(ld, B, (11, 12))
    xT = torch.randn((B, ld.channels, LATENT_T, ld.latent_f_size), generator=torch.Generator().manual_seed(7))
    ld.latent_t_size = LATENT_T

    def job(cond):
        torch.manual_seed(9)
        out, _ = ld.sample_log(cond=cond, batch_size=B, x_T=xT, ddim=True, ddim_steps=4, eta=1.0, unconditional_guidance_scale=GS,
                               unconditional_conditioning=uncond)
        return out.clone()
    job_a, job_b, plain = (lambda: job(Composed(conds, [1.0, -0.5]))), (lambda: job(Composed(conds, [0.4, 0.8]))), (lambda: job(conds[0]))
    unet.drop_step_caches()
    a_fresh = job_a()
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and tuple(ent["compose"].shape) == (1, 3)
    b_hit = job_b()
    assert next(iter(unet._graph_cache.values())) is ent
    assert ent["compose"].cpu().tolist() == [[float(np.float32(1.0 - 1.2)), float(np.float32(0.4)), float(np.float32(0.8))]]
    a_hit = job_a()
    assert next(iter(unet._graph_cache.values())) is ent
    plain_after = plain()                     # another launch sequence: its own entry
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is not ent
    unet.drop_step_caches()
    b_fresh = job_b()
    unet.drop_step_caches()
    plain_fresh = plain()
    # K = 1 has a plain guided job's context shapes and another launch sequence: its own entry, and bitwise the plain job
    one = job(Composed(conds[:1], [1.0]))
    assert len(unet._graph_cache) == 1 and "compose" in next(iter(unet._graph_cache.values()))
    unet.drop_step_caches()
    assert torch.equal(a_hit, a_fresh) and torch.equal(b_hit, b_fresh) and torch.equal(plain_after, plain_fresh)
    assert torch.equal(one, plain_fresh)
    assert A.rel_rms(b_fresh, a_fresh) > 1e-3 and A.rel_rms(a_fresh, plain_fresh) > 1e-3
    assert bool(torch.isfinite(a_fresh).all())


@pytest.fixture(scope="module")
def ld_cond():
    """The HIP conditioner stack (prompts that differ give conditionings that differ), as tests/test_guidance_gpu.py builds it."""
    from audioldm2_amd.pipeline import LatentDiffusion, default_audioldm_config
    with open(os.path.join(GOLD, "e2econd_statedict_keys.json")) as f:
        k = json.load(f)
    hot, cond = {a: tuple(b) for a, b in k["hot"].items()}, {a: tuple(b) for a, b in k["cond"].items()}
    cfg = default_audioldm_config("audioldm2-full", conditioners="hip", t5_config=cases.t5_test_config(),
                                  clap_config=cases.clap_text_test_config())
    cfg["model"]["params"]["build_clap"] = False    # one candidate per prompt: no re-ranker needed
    torch.manual_seed(0)
    ld = LatentDiffusion(**cfg["model"]["params"]).eval()
    sd = weights.make_state_dict(hot, seed=0)
    sd.update(cases.cond_state_dict(cond, seed=0))
    sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
    res = ld.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys[:5]
    ld = ld.cuda()
    seq = ld.cond_stage_models[0]
    seq.cond_stage_models[0].tokenize = cases.StubRobertaTokenizer()
    seq.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    ld.cond_stage_models[1].tokenizer = cases.StubT5Tokenizer()
    return ld


MIX = [("rain on a tin roof", 1.0), ("distant thunder", 0.6), ("traffic", -0.4)]


def test_text_to_audio_takes_compose_end_to_end(ld_cond):
    from audioldm2_amd.pipeline import text_to_audio
    ld = ld_cond
    kw = dict(seed=7, ddim_steps=4, duration=2.5, batchsize=1, n_candidate_gen_per_text=1)

    def job(text, **more):
        ld.conditional_dry_run_finished = False   # every call as an object's first (pipeline._cfg_dropout_draw)
        ld.model.diffusion_model.drop_step_caches()
        wave = text_to_audio(ld, text, **kw, **more)
        return wave, float(torch.rand(1))
    mix, _ = job(None, compose=MIX)
    singles = [job(p) for p, _ in MIX]
    assert ld.latent_t_size == LATENT_T
    assert mix.dtype == np.float32 and mix.ndim == 3 and mix.shape == singles[0][0].shape and np.isfinite(mix).all()
    for (wave, _), (p, _) in zip(singles, MIX):
        assert not np.array_equal(mix, wave), p
    assert np.array_equal(job(None, compose=MIX)[0], mix)                       # a second job under the same seed: the first
    # one prompt of weight 1 through the group pass is the plain job, draws included
    one, rand_one = job(None, compose=[(MIX[0][0], 1.0)])
    assert np.array_equal(one, singles[0][0]) and rand_one == singles[0][1]
    # a weight may be a list of ddim_steps numbers; a negative prompt still takes the unconditional group's place
    fade, _ = job(None, compose=[(MIX[0][0], 1.0), (MIX[1][0], [0.0, 0.3, 0.6, 0.9])])
    neg, _ = job(None, compose=MIX, negative_prompt="Low quality.")
    assert np.isfinite(fade).all() and np.isfinite(neg).all() and not np.array_equal(fade, mix) and not np.array_equal(neg, mix)
    ld.model.diffusion_model.drop_step_caches()
