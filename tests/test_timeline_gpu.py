"""GPU tests of prompt timelines: aldm_window_gather_rows against torch slicing (bitwise), aldm_window_merge_rows
against an fp64 overlap-add of the same fp32 inputs (bar: the row cover * 2^-24 of the sum of the terms' magnitudes,
tests/timeline.py), its bit-exact frames, the zero skip (a NaN under a weight of exactly 0 does not reach the output) and bounds;
aldm_window_blend_gather_rows against inpaint_blend followed by the row gather (bitwise); the three samplers over a row plan on the
tiny UNet against the composition loop (slice the rows, run the same model under per-row conditioning, merge in fp64, the sampler's
eager single-step form); one prompt against the run without a timeline (bitwise); generate_batch_long with a timeline end to end,
with the step-graph cache shared by two timelines of one row geometry.

Boundaries [13, 27] at transition 4 do NOT have the row geometry of [12, 28] on the plan (40, 16, 10) — prompt 2 then starts at frame
25, inside window 1 = [10, 26), R = 9 against 8 (tests/test_timeline_cpu.py) — so the job of the same geometry is [12.5, 27.5], and
[13, 27] is run as a job of its own.  The tiny model has no step-graph cache (it is no UNet module): the cache is asserted on
end to end, on the real model."""
import numpy as np
import pytest
import torch

import audio2audio as A
import long_source as Ls
import timeline as Tl
import windowed as Wd
from tolerances import latent_tol, log_err

pytestmark = pytest.mark.gpu

NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


def rows_of(case):
    B, key, bounds, tau, C, F = case
    base, rp = Tl.plans_of(key, bounds, tau)
    return B, base, rp, C, F


# ---- 1. the gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Tl.KERNEL_CASES, ids=Tl.case_id)
def test_gather_rows_is_bitwise_torch_slicing(case):
    from audioldm2_amd import ops
    B, base, rp, C, F = rows_of(case)
    x, _ = Tl.row_inputs(B, rp, C, F)
    x = x.cuda()
    out, buf = A.guarded((rp.R * B, C, rp.Tw, F))
    got = ops.window_gather(x, rp, out=out)
    ref = Wd.gather_ref(x, Tl.as_window_plan(rp))
    assert got is out and torch.equal(bits(out), bits(ref)) and A.guards_intact(buf)
    assert torch.equal(ops.window_gather(x, rp), out)            # the allocating form
    for r, (j, k) in enumerate(rp.rows):                          # the rows of a window are that window of the base plan
        assert torch.equal(out[r * B:(r + 1) * B], x[:, :, base.starts[j]:base.starts[j] + rp.Tw])


# ---- 2. the merge against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [None, 2], ids=["H1", "H2"])
@pytest.mark.parametrize("case", Tl.KERNEL_CASES, ids=Tl.case_id)
def test_merge_rows_matches_fp64(case, H):
    from audioldm2_amd import ops
    B, base, rp, C, F = rows_of(case)
    wp = Tl.as_window_plan(rp)
    _, win = Tl.row_inputs(B, rp, C, F, H=H, seed=1)
    win = win.cuda()
    out, buf = A.guarded(((2,) if H == 2 else ()) + (B, C, rp.T, F))
    got = ops.window_merge(win, rp, out=out)
    assert got is out and A.guards_intact(buf)
    ref, den, _ = Wd.merge_fp64(win, wp)
    assert float(den.min()) > 0.0
    err = float(((out.double() - ref).abs() / den).max())
    bar = Tl.bar(rp)
    print(f"window_merge_rows {Tl.case_id(case)} H={H} R={rp.R} cover={rp.cover}: max |err| / sum |wr e| = {err:.3e}  bar {bar:.3e}")
    assert log_err(err, bar, f"window_merge_rows {Tl.case_id(case)} H={H}") <= bar
    # frames with a single row of weight 1 reproduce that row's input bit for bit
    nz = torch.zeros(rp.T, dtype=torch.int64)
    for r, s in enumerate(rp.row_starts):
        nz[s:s + rp.Tw] += (rp.wr[r] != 0).long()
    assert int(nz.max()) == rp.cover and int(nz.min()) >= 1
    one = (nz == 1).nonzero().view(-1).tolist()
    assert one, "the case has no frame under a single row"
    for t in one[:4] + one[-4:]:
        r = next(r for r, s in enumerate(rp.row_starts) if s <= t < s + rp.Tw and float(rp.wr[r, t - s]) != 0.0)
        assert float(rp.wr[r, t - rp.row_starts[r]]) == 1.0
        assert torch.equal(bits(out[..., t, :]), bits(win[..., r * B:(r + 1) * B, :, t - rp.row_starts[r], :]))
    # two runs are bitwise equal, so is the allocating form, and so is a run that reads the weights from a caller's buffer
    assert torch.equal(ops.window_merge(win, rp), out.clone())
    assert torch.equal(ops.window_merge(win, rp, weights=rp.wr.cuda()), out.clone())


@pytest.mark.parametrize("key,C,F", [((40, 16, 10), 3, 5), ((24, 16, 1), 2, 7), ((768, 256, 192), 8, 16)])
def test_one_prompt_merges_bitwise_like_the_window_merge(key, C, F):
    from audioldm2_amd import ops
    base, rp = Tl.plans_of(key, [], 0)
    assert rp.R == base.W
    x, win = Wd.window_inputs(2, base, C, F, H=2, seed=5)
    x, win = x.cuda(), win.cuda()
    assert torch.equal(bits(ops.window_merge(win, rp)), bits(ops.window_merge(win, base)))
    assert torch.equal(bits(ops.window_gather(x, rp)), bits(ops.window_gather(x, base)))


# ---- 3. the zero skip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 16])
def test_a_nan_under_a_zero_weight_is_not_read_and_one_under_a_weight_reaches_exactly_its_frames(F):
    from audioldm2_amd import ops
    B, C = 2, 3
    _, rp = Tl.plans_of((40, 16, 10), [12, 28], 4)
    _, win = Tl.row_inputs(B, rp, C, F, H=2, seed=4)
    win = win.cuda()
    clean = ops.window_merge(win, rp)
    h, b, c = 1, 1, 2
    r = 2                                   # (window 1, prompt 0): prompt 0 ends at frame 13, the window runs to 25
    assert rp.rows[r] == (1, 0)
    silent = (rp.wr[r] == 0).nonzero().view(-1)
    assert 0 < silent.numel() < rp.Tw
    # (a) NaN wherever the row's weight is exactly 0, in every sample and channel of the row: the output is bitwise the clean one
    w0 = win.clone()
    w0[:, r * B:(r + 1) * B, :, silent.cuda()] = NAN
    out, buf = A.guarded((2, B, C, rp.T, F))
    ops.window_merge(w0, rp, out=out)
    assert bool(torch.isfinite(out).all()) and torch.equal(bits(out), bits(clean)) and A.guards_intact(buf)
    # (b) the whole row NaN: it reaches exactly the frames the row covers with a non-zero weight
    w1 = win.clone()
    w1[h, r * B + b, c] = NAN
    ops.window_merge(w1, rp, out=out)
    want = torch.zeros_like(out, dtype=torch.bool)
    loud = (rp.wr[r] != 0).nonzero().view(-1) + rp.row_starts[r]
    want[h, b, c, loud.cuda()] = True
    assert torch.equal(torch.isnan(out), want) and A.guards_intact(buf)
    assert torch.equal(bits(out)[~want], bits(clean)[~want])


def test_unaligned_pointers_take_the_scalar_path_and_give_the_same_bits():
    """F % 4 == 0 but a tensor starts 4 bytes off a 16-byte boundary: the same results as the aligned launches."""
    from audioldm2_amd import ops
    B, C, F = 1, 3, 16
    _, rp = Tl.plans_of((40, 16, 10), [12, 28], 4)
    x, win = Tl.row_inputs(B, rp, C, F, H=2)

    def off(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        u = buf[1:].view(t.shape).copy_(t)
        assert u.data_ptr() % 16 == 4
        return u
    xu, wu = off(x), off(win)
    assert torch.equal(bits(ops.window_gather(xu, rp)), bits(Wd.gather_ref(x.cuda(), Tl.as_window_plan(rp))))
    assert torch.equal(bits(ops.window_gather(x.cuda(), rp, out=off(torch.empty(rp.R * B, C, rp.Tw, F)))),
                       bits(ops.window_gather(x.cuda(), rp)))
    ref = ops.window_merge(win.cuda(), rp)
    assert torch.equal(bits(ops.window_merge(wu, rp)), bits(ref))
    assert torch.equal(bits(ops.window_merge(win.cuda(), rp, out=off(torch.empty(2, B, C, rp.T, F)))), bits(ref))
    # the blend fused with the row gather: every operand in turn off the boundary
    base = Tl.plans_of((40, 16, 10), [12, 28], 4)[0]
    xb, x0, qn, coef = Ls.blend_inputs(B, base, C, F, S=2, seed=2)
    lo, hi = Ls.overlap_interval(base)
    m = Ls.mask_patterns(base, tuple(xb.shape))[f"keep[{lo},{hi})"].cuda()
    x0d, qnd, coefd = x0.cuda(), qn.cuda(), coef.cuda()
    idx = torch.ones(1, device="cuda", dtype=torch.int32)
    ref_x = xb.cuda()
    ref_win = ops.window_blend_gather(ref_x, x0d, qnd, m, coefd, rp, step_idx=idx)
    plain_x = xb.cuda()
    ops.inpaint_blend(plain_x, x0d, qnd[1], m, coefd[1])
    assert torch.equal(bits(ref_x), bits(plain_x)) and torch.equal(bits(ref_win), bits(ops.window_gather(plain_x, rp)))
    for which in ("x", "x0", "qnoise", "mask", "win"):
        xx = off(xb) if which == "x" else xb.cuda()
        out = off(torch.full(tuple(ref_win.shape), NAN)) if which == "win" else None
        win_u = ops.window_blend_gather(xx, off(x0) if which == "x0" else x0d, off(qn) if which == "qnoise" else qnd,
                                        off(m) if which == "mask" else m, coefd, rp, step_idx=idx, out=out)
        assert torch.equal(bits(win_u), bits(ref_win)) and torch.equal(bits(xx), bits(ref_x)), which


def test_wrappers_refuse_what_they_cannot_run():
    from audioldm2_amd import ops
    B, C, F = 2, 3, 8
    base, rp = Tl.plans_of((40, 16, 10), [12, 28], 4)
    x, win = Tl.row_inputs(B, rp, C, F, H=2)
    with pytest.raises(RuntimeError, match="window_merge: win must be"):
        ops.window_merge(Wd.window_inputs(B, base, C, F, H=2)[1][:, :7].contiguous().cuda(), rp)     # 7 rows, not a multiple of R = 8
    with pytest.raises(RuntimeError, match="window_merge.weights: expected"):
        ops.window_merge(win.cuda(), rp, weights=base.wn.cuda())
    with pytest.raises(RuntimeError, match="only a row plan"):
        ops.window_merge(Wd.window_inputs(B, base, C, F, H=2)[1].cuda(), base, weights=base.wn.cuda())
    with pytest.raises(RuntimeError, match="window_gather.out: expected"):
        ops.window_gather(x.cuda(), rp, out=torch.empty(base.W * B, C, rp.Tw, F, device="cuda"))


# ---- 4. the blend fused with the row gather -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Tl.KERNEL_CASES, ids=Tl.case_id)
def test_blend_gather_rows_is_bitwise_the_blend_then_the_row_gather(case):
    from audioldm2_amd import ops
    B, base, rp, C, F = rows_of(case)
    S = 3
    x, x0, qn, coef = Ls.blend_inputs(B, base, C, F, S=S, seed=3)
    x0d, qnd, coefd = x0.cuda(), qn.cuda(), coef.cuda()
    for name, m in Ls.mask_patterns(base, tuple(x.shape)).items():
        md = m.cuda()
        # the device step counter: step 0, a middle step, and past the tables' end (both saturate at their last row)
        for idx, row in ((0, 0), (1, 1), (7, S - 1)):
            ref_x = x.cuda()
            ops.inpaint_blend(ref_x, x0d, qnd[row], md, coefd[row])
            ref_win = ops.window_gather(ref_x, rp)
            xg, xbuf = A.guarded(tuple(x.shape))
            xg.copy_(x)
            win, wbuf = A.guarded((rp.R * B, C, rp.Tw, F))
            step_idx = torch.full((1,), idx, device="cuda", dtype=torch.int32)
            got = ops.window_blend_gather(xg, x0d, qnd, md, coefd, rp, step_idx=step_idx, out=win)
            assert got is win and int(step_idx) == idx
            assert torch.equal(bits(xg), bits(ref_x)), f"{name} step {idx}: x differs from ops.inpaint_blend"
            assert torch.equal(bits(win), bits(ref_win)), f"{name} step {idx}: win differs from the row gather of the blended x"
            assert A.guards_intact(xbuf) and A.guards_intact(wbuf)
    assert not torch.equal(qnd[0], qnd[1]) and not torch.equal(coefd[1], coefd[2])       # the rows differ: the selection was seen


# ---- 5. the samplers on the tiny UNet -------------------------------------------------------------------------------------------------
LONG_KEY, STEPS, BOUNDS, TAU = (40, 16, 10), 6, [12, 28], 4
LONG_SHAPE = (A.TINY_SHAPE[0], A.TINY_SHAPE[1], LONG_KEY[0], A.TINY_SHAPE[3])
SEED = 9


@pytest.fixture(scope="module")
def tiny():
    """The tiny model, three distinct seeded conditionings (one per prompt) and the unconditional one."""
    from oracle import cases
    m = A.TinyModel()
    B = A.TINY_SHAPE[0]

    def conditioning(seed):
        _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=seed)
        return ([c.cuda() for c in ctxs], [k.cuda() for k in masks])
    return m, [conditioning(s) for s in (1, 3, 4)], conditioning(2)


def x_long(seed=3, shape=LONG_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sampler_class(name):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp_2m": DPMSolverSampler}[name]


CONFIGS = {"ddim": ("ddim", {}), "ddim-rescale": ("ddim", dict(guidance_rescale=0.7)), "plms": ("plms", {}), "dpmpp_2m": ("dpmpp_2m", {})}


def run(name, tiny, plan, conds=None, shape=LONG_SHAPE, steps=STEPS, **kw):
    from audioldm2_amd.windows import PerPrompt, has_rows
    m, prompts, uncond = tiny
    conds = prompts if conds is None else conds
    cond = PerPrompt(conds) if plan is not None and has_rows(plan) else conds[0]
    torch.manual_seed(SEED)
    out, _ = sampler_class(name)(m).sample(steps, shape[0], shape[1:], cond, x_T=x_long(shape=shape), eta=0.0, windows=plan,
                                           t_start=steps, verbose=False, unconditional_guidance_scale=A.GS,
                                           unconditional_conditioning=uncond, **kw)
    return out


def loop(cfg, tiny, rp, conds=None, source=None):
    m, prompts, uncond = tiny
    conds = prompts if conds is None else conds
    name, kw = CONFIGS[cfg]
    torch.manual_seed(SEED)
    if name == "ddim":
        return Tl.ddim_loop(m, rp, x_long(), conds, uncond, STEPS, A.GS, k=STEPS, source=source, **kw)
    assert source is None
    return (Tl.plms_loop if name == "plms" else Tl.dpmpp_loop)(m, rp, x_long(), conds, uncond, STEPS)


@pytest.fixture(scope="module")
def references(tiny):
    """The composition loops of the job [12, 28], each computed once."""
    rp = Tl.plans_of(LONG_KEY, BOUNDS, TAU)[1]
    done = {}

    def get(cfg):
        if cfg not in done:
            done[cfg] = loop(cfg, tiny, rp)
        return done[cfg]
    return get


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_timeline_sampler_equals_the_composition_loop(tiny, references, cfg):
    name, kw = CONFIGS[cfg]
    rp = Tl.plans_of(LONG_KEY, BOUNDS, TAU)[1]
    assert rp.R == 8
    out = run(name, tiny, rp, **kw)
    assert tuple(out.shape) == LONG_SHAPE and bool(torch.isfinite(out).all())
    e, bar = A.rel_rms(out, references(cfg)), A.tstart_bar(STEPS)
    print(f"{cfg} timeline {BOUNDS} tau={TAU} on {LONG_KEY}, {STEPS} steps vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert bar == 1e-5
    assert log_err(e, bar, f"timeline {cfg}") <= bar
    assert A.rel_rms(out, x_long().cuda()) > 1e-3
    assert torch.equal(run(name, tiny, rp, **kw), out)             # a second job under the same seed: bitwise the first


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_one_prompt_is_bitwise_the_windowed_run(tiny, cfg):
    name, kw = CONFIGS[cfg]
    base, rp = Tl.plans_of(LONG_KEY, [], 0)
    m, prompts, uncond = tiny
    assert torch.equal(bits(run(name, tiny, rp, conds=prompts[:1], **kw)), bits(run(name, tiny, base, **kw)))


def test_other_timelines_match_their_own_loops_and_differ(tiny, references):
    from audioldm2_amd.windows import plan_key
    first_plan = Tl.plans_of(LONG_KEY, BOUNDS, TAU)[1]
    first = run("ddim", tiny, first_plan)
    bar = A.tstart_bar(STEPS)
    for bounds, same_geometry in (([12.5, 27.5], True), ([13, 27], False)):
        rp = Tl.plans_of(LONG_KEY, bounds, TAU)[1]
        assert (plan_key(rp) == plan_key(first_plan)) == same_geometry and (rp.R == 8) == same_geometry
        out = run("ddim", tiny, rp)
        e = A.rel_rms(out, loop("ddim", tiny, rp))
        print(f"ddim timeline {bounds} vs its own composition loop: {e:.2e}  bar {bar:.1e}; vs the job {BOUNDS}: "
              f"{A.rel_rms(out, first):.2e}")
        assert log_err(e, bar, f"timeline ddim {bounds}") <= bar
        assert A.rel_rms(out, first) > 1e-3
    # swapping the conditionings of prompts 0 and 2 changes the frames prompt 0 owns
    m, prompts, uncond = tiny
    swapped = run("ddim", tiny, first_plan, conds=[prompts[2], prompts[1], prompts[0]])
    assert A.rel_rms(swapped[:, :, :10], first[:, :, :10]) > 1e-3


def test_a_source_on_the_row_plan_equals_the_composition_loop_with_the_blend(tiny):
    from audioldm2_amd.windows import keep_mask, with_source
    rp = Tl.plans_of(LONG_KEY, BOUNDS, TAU)[1]
    x0 = torch.randn(LONG_SHAPE, generator=torch.Generator().manual_seed(5)).cuda()
    mask = keep_mask(LONG_KEY[0], [(0, 8)])
    out = run("ddim", tiny, with_source(rp, x0, mask))
    after = float(torch.rand(1))
    ref = loop("ddim", tiny, rp, source=(x0, mask.view(1, 1, -1, 1).expand(LONG_SHAPE).contiguous()))
    assert float(torch.rand(1)) == after                           # q-noise then step noise, per step, at the long shape
    e, bar = A.rel_rms(out, ref), A.tstart_bar(STEPS)
    print(f"ddim timeline with a source (keep [0, 8)) vs the composition loop with the blend: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "timeline ddim source") <= bar
    assert A.rel_rms(out, run("ddim", tiny, rp)) > 1e-3            # ... and the source matters


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED, E2E_TAU = 384, 128, 2, 42, 32
PROMPTS = ["rain on a tin roof", "birds after the rain"]


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def timeline_job(ld, boundary, prompts=PROMPTS):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    seed_everything(E2E_SEED)
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = ld.generate_batch_long([make_batch_for_text_to_audio(p) for p in prompts], E2E_T, hop=E2E_HOP, ddim_steps=E2E_STEPS,
                                  unconditional_guidance_scale=A.GS, boundaries=[boundary], transition=E2E_TAU)
    return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), float(torch.rand(1))


def timeline_reference(ld, boundary, prompts=PROMPTS):
    """The job's draws by hand in the stated order — (R1), the conditioners once per prompt in timeline order, x_T, the step draws —
    around the composition loop -> (latent, the rand(1) after)."""
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    from audioldm2_amd.windows import prompt_weights, row_plan
    C, F_ = ld.channels, ld.latent_f_size
    plan, _ = ld.long_form_plans(E2E_T, E2E_HOP)
    rp = row_plan(plan, prompt_weights(E2E_T, [boundary], E2E_TAU))
    seed_everything(E2E_SEED)
    torch.randn((1, C, 256, F_))
    conds = [ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(p)) for p in prompts]
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    ref = Tl.ddim_loop(ld, rp, torch.randn((1, C, E2E_T, F_)), conds, uncond, E2E_STEPS, A.GS, eta=1.0)
    return ref, float(torch.rand(1)), rp


def test_generate_batch_long_with_a_timeline_end_to_end(ld):
    from audioldm2_amd import ops
    from audioldm2_amd.windows import plan_key
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, E2E_HOP)
    wave, latent, mel, rand_after = timeline_job(ld, 192)
    ref, rand_ref, rp = timeline_reference(ld, 192)
    assert (plan.W, rp.R, rp.rows) == (2, 4, ((0, 0), (0, 1), (1, 0), (1, 1)))
    C, F_ = ld.channels, ld.latent_f_size
    assert tuple(latent.shape) == (1, C, E2E_T, F_) and tuple(mel.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.dtype == np.float32 and np.isfinite(wave).all() and wave.shape[:2] == (1, 1)
    # the host generator ends where the RNG contract says
    assert rand_after == rand_ref
    e = A.rel_rms(latent, ref)
    print(f"generate_batch_long timeline latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "timeline long-form latent") <= latent_tol(E2E_STEPS)
    # the mel is the base plan's tail of the job's own latent: prompts do not enter the decode
    mel_w = ld.decode_first_stage_cl(ops.window_gather(latent, plan))
    assert torch.equal(mel, ops.window_merge(mel_w.view(mel_w.shape[0], 1, mel_w.shape[1], mel_w.shape[2]), mel_plan))

    # a second timeline of the same row geometry replays the cached step graph, with its own weights
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and plan_key(ent["win"].plan) == plan_key(rp)
    wave2, latent2, _, rand2 = timeline_job(ld, 200)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    ref2, rand_ref2, rp2 = timeline_reference(ld, 200)
    assert plan_key(rp2) == plan_key(rp) and not torch.equal(rp2.wr, rp.wr) and torch.equal(ent["win"].wr.cpu(), rp2.wr)
    e2 = A.rel_rms(latent2, ref2)
    print(f"... boundary 200 on the cached graph vs its own composition loop: {e2:.2e}; vs the boundary-192 job: "
          f"{A.rel_rms(latent2, latent):.2e}")
    assert log_err(e2, latent_tol(E2E_STEPS), "timeline long-form latent, cached graph") <= latent_tol(E2E_STEPS)
    # (the fixture's synthetic conditioners barely move the random-init model: that the weights of the second job are the ones in
    # force is asserted on the buffer above, and on the latent, under conditionings that differ, in the next test)
    assert rand2 == rand_ref2
    # ... and back: the first timeline on the same graph is bitwise its first run
    wave3, latent3, _, _ = timeline_job(ld, 192)
    assert next(iter(unet._graph_cache.values())) is ent and torch.equal(latent3, latent) and np.array_equal(wave3, wave)
    unet.drop_step_caches()


def test_two_timelines_of_one_row_geometry_share_the_cached_step_graph_and_not_their_weights(ld):
    """The real UNet under two seeded conditionings that differ as much as noise does: the second timeline takes the first one's
    captured graph, matches its own composition loop, and differs from the first."""
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    from audioldm2_amd.windows import PerPrompt, plan_key, prompt_weights, row_plan
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    C, F_ = ld.channels, ld.latent_f_size
    plan, _ = ld.long_form_plans(E2E_T, E2E_HOP)
    base = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(PROMPTS[0]))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}

    def synth(c, g):
        if torch.is_tensor(c):
            return torch.randn(c.shape, generator=g).to(c.device) if c.dim() == 3 else c       # contexts [B, L, D]; masks stay
        if isinstance(c, dict):
            return {k: synth(v, g) for k, v in c.items()}
        return type(c)(synth(v, g) for v in c)
    conds = [synth(base, torch.Generator().manual_seed(s)) for s in (11, 12)]
    x_T = torch.randn((1, C, E2E_T, F_), generator=torch.Generator().manual_seed(7))

    def job(boundary):
        rp = row_plan(plan, prompt_weights(E2E_T, [boundary], E2E_TAU))
        out, _ = ld.sample_log(cond=PerPrompt(conds), batch_size=1, x_T=x_T, ddim=True, ddim_steps=E2E_STEPS, eta=0.0,
                               unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond, windows=rp)
        return out.clone(), rp
    first, rp = job(192)
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and plan_key(ent["win"].plan) == plan_key(rp) and torch.equal(ent["win"].wr.cpu(), rp.wr)
    second, rp2 = job(200)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent          # the cached graph was taken
    assert plan_key(rp2) == plan_key(rp) and torch.equal(ent["win"].wr.cpu(), rp2.wr) and not torch.equal(rp2.wr, rp.wr)
    bar = latent_tol(E2E_STEPS)
    for name, out, p in (("192", first, rp), ("200, cached graph", second, rp2)):
        e = A.rel_rms(out, Tl.ddim_loop(ld, p, x_T, conds, uncond, E2E_STEPS, A.GS, eta=0.0))
        print(f"real UNet, seeded conditionings, boundary {name} vs its own composition loop: {e:.2e}  bar {bar:.1e}")
        assert log_err(e, bar, f"timeline real UNet boundary {name}") <= bar
    d = A.rel_rms(second, first)
    print(f"... boundary 200 vs boundary 192: {d:.2e}")
    assert d > 1e-3
    assert torch.equal(job(192)[0], first) and next(iter(unet._graph_cache.values())) is ent     # and back: bitwise the first run
    unet.drop_step_caches()
