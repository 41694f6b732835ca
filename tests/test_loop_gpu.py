"""GPU tests of seamless loops (ring plans): aldm_window_gather_ring against torch.roll and a slice (bitwise),
aldm_window_merge_ring against a circular fp64 overlap-add of the same fp32 inputs (bar: cover * 2^-24 of the sum of the terms'
magnitudes, tests/looped.py), NaN locality across the wrap, aldm_window_blend_gather_ring against ops.inpaint_blend followed by the
ring gather (bitwise), the wrappers' refusals; the three samplers on a ring plan on the tiny UNet against the composition loop over
looped.RingModel, with and without a source; that no frame of a ring is special (a roll of x_T by one gap rolls the result — and a
linear plan fails that by far); LatentDiffusion.generate_batch_long / text_to_audio_long / generate_batch_long_from_audio with
loop=True end to end, the junction against the vocoder over three periods of the mel."""
import numpy as np
import pytest
import torch

import audio2audio as A
import long_source as Ls
import looped as Lp
import windowed as Wd
from tolerances import latent_tol, log_err, mel_tol, tail_tol

pytestmark = pytest.mark.gpu

NAN = float("nan")


def case_id(c):
    B, key, C, F = c
    return f"B{B}-T{key[0]}w{key[1]}h{key[2]}-C{C}-F{F}"


def bits(t):
    return t.contiguous().view(torch.int32)


def off_by_one_float(t):
    """A copy of `t` that starts 4 bytes off a 16-byte boundary: the launches on it take the scalar path."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    u = buf[1:].view(t.shape).copy_(t)
    assert u.data_ptr() % 16 == 4
    return u


# ---- 1. the gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Lp.KERNEL_CASES, ids=case_id)
def test_ring_gather_is_bitwise_roll_and_slice(case):
    from audioldm2_amd import ops
    B, key, C, F = case
    plan = Lp.ring_plan(key)
    x, _ = Wd.window_inputs(B, plan, C, F)
    x = x.cuda()
    ref = Lp.ring_gather_ref(x, plan)
    out, buf = A.guarded((plan.W * B, C, plan.Tw, F), fill=NAN)
    got = ops.window_gather(x, plan, out=out)
    assert got is out and torch.equal(bits(out), bits(ref))
    assert bool(torch.isnan(buf[:A.GUARD]).all()) and bool(torch.isnan(buf[-A.GUARD:]).all())
    assert torch.equal(ops.window_gather(x, plan), ref)                              # the allocating form
    assert torch.equal(ops.window_gather(off_by_one_float(x), plan), ref)            # the forced scalar path
    # at least one window wraps, and the wrap was seen: the last window differs from the slice that stops at T
    s = plan.starts[-1]
    assert s + plan.Tw > plan.T and torch.equal(out[(plan.W - 1) * B:, :, plan.T - s:], x[:, :, :s + plan.Tw - plan.T])


# ---- 2. the merge against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [None, 2], ids=["H1", "H2"])
@pytest.mark.parametrize("case", Lp.KERNEL_CASES, ids=case_id)
def test_ring_merge_matches_fp64(case, H):
    from audioldm2_amd import ops
    B, key, C, F = case
    plan = Lp.ring_plan(key)
    _, win = Wd.window_inputs(B, plan, C, F, H=H, seed=1)
    win = win.cuda()
    out, buf = A.guarded(((2,) if H == 2 else ()) + (B, C, plan.T, F))
    got = ops.window_merge(win, plan, out=out)
    assert got is out and A.guards_intact(buf)
    ref, den, count = Lp.ring_merge_fp64(win, plan)
    assert int(count.max()) == plan.cover and int(count.min()) >= 1 and float(den.min()) > 0.0
    bar = Wd.bar(plan)
    ratio = (out.double() - ref).abs() / den
    err = float(ratio.max())
    print(f"window_merge_ring {case_id(case)} H={H} cover={plan.cover}: max |err| / sum |wn e| = {err:.3e}  bar {bar:.3e}")
    log_err(err, bar, f"window_merge_ring {case_id(case)}")
    assert bool(((out.double() - ref).abs() <= bar * den).all())
    # frames under ONE window (wn == 1) reproduce their input bit for bit
    one = (count == 1).nonzero().view(-1).tolist()
    for t in one[:4] + one[-4:]:
        (j,) = [i for i, s in enumerate(plan.starts) if (t - s) % plan.T < plan.Tw]
        assert torch.equal(bits(out[..., t, :]), bits(win[..., j * B:(j + 1) * B, :, (t - plan.starts[j]) % plan.T, :]))
    # two runs are bitwise equal, so is the allocating form, and so is the scalar path where the aligned launch took the other one
    assert torch.equal(bits(ops.window_merge(win, plan)), bits(out))
    assert torch.equal(bits(ops.window_merge(off_by_one_float(win), plan)), bits(out))


# ---- 3. NaN locality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 16])
def test_a_nan_at_a_wrapped_position_reaches_its_frame_and_no_other(F):
    from audioldm2_amd import ops
    B, C = 2, 3
    plan = Lp.ring_plan((40, 16, 10))
    _, win = Wd.window_inputs(B, plan, C, F, H=2, seed=4)
    win = win.cuda()
    h, j, b, c, p = 1, 3, 1, 2, 13                       # window 3 starts at 30: p = 13 is frame 43 - 40 = 3
    assert plan.starts[j] + p >= plan.T
    win[h, j * B + b, c, p] = NAN
    out, buf = A.guarded((2, B, C, plan.T, F))
    ops.window_merge(win, plan, out=out)
    want = torch.zeros_like(out, dtype=torch.bool)
    want[h, b, c, plan.starts[j] + p - plan.T] = True
    assert torch.equal(torch.isnan(out), want) and A.guards_intact(buf)
    # the whole window: exactly the frames it covers, on both sides of the junction
    win[h, j * B + b, c] = NAN
    ops.window_merge(win, plan, out=out)
    want[h, b, c, plan.starts[j]:] = True
    want[h, b, c, :plan.starts[j] + plan.Tw - plan.T] = True
    assert torch.equal(torch.isnan(out), want) and int(want.sum()) == plan.Tw * F


# ---- 4. the blend-gather --------------------------------------------------------------------------------------------------------------
def blend_then_ring_gather(x, x0, qn, m, coef_row, plan):
    """The two launches the fused one replaces, on a copy."""
    from audioldm2_amd import ops
    ref_x = x.clone()
    ops.inpaint_blend(ref_x, x0, qn.contiguous(), m, coef_row.contiguous())
    return ref_x, ops.window_gather(ref_x, plan)


@pytest.mark.parametrize("case", [Lp.KERNEL_CASES[0], Lp.KERNEL_CASES[2]], ids=case_id)
def test_ring_blend_gather_is_bitwise_blend_then_ring_gather(case):
    from audioldm2_amd import ops
    B, key, C, F = case
    plan = Lp.ring_plan(key)
    S = 3
    x, x0, qn, coef = Ls.blend_inputs(B, plan, C, F, S=S)
    x0d, qnd, coefd = x0.cuda(), qn.cuda(), coef.cuda()
    masks = {"zeros": torch.zeros(x.shape), "ones": torch.ones(x.shape), "quarter": torch.full(x.shape, 0.25),
             "across the junction": (Wd.window_inputs(B, plan, C, F, seed=9)[0] > 0).float()}
    masks["across the junction"][:, :, -3:] = 1.0
    masks["across the junction"][:, :, :2] = 1.0
    # (step index, q-noise table, coefficient table) -> (q row, coefficient row): step 0, a middle one, beyond the tables' last row
    # (saturation), q_rows == 1 with more coefficient rows, no counter at all
    selections = ((0, qnd, coefd, 0, 0), (1, qnd, coefd, 1, 1), (S + 2, qnd, coefd, S - 1, S - 1),
                  (2, qnd[0].contiguous(), coefd, 0, 2), (S + 2, qnd[:1].contiguous(), coefd, 0, S - 1), (None, qnd, coefd, 0, 0))
    for name, m in masks.items():
        md = m.cuda()
        for idx, q, c, qrow, crow in selections:
            ref_x, ref_win = blend_then_ring_gather(x.cuda(), x0d, qnd[qrow], md, coefd[crow], plan)
            xg, xbuf = A.guarded(tuple(x.shape))
            xg.copy_(x)
            win, wbuf = A.guarded((plan.W * B, C, plan.Tw, F), fill=NAN)
            step_idx = None if idx is None else torch.full((1,), idx, device="cuda", dtype=torch.int32)
            got = ops.window_blend_gather(xg, x0d, q, md, c, plan, step_idx=step_idx, out=win)
            assert got is win
            assert torch.equal(bits(xg), bits(ref_x)), f"{name} step {idx}: x differs from ops.inpaint_blend"
            assert torch.equal(bits(win), bits(ref_win)), f"{name} step {idx}: win differs from the ring gather of the blended x"
            assert torch.equal(bits(win), bits(Lp.ring_gather_ref(ref_x, plan)))
            assert not bool(torch.isnan(win).any()) and A.guards_intact(xbuf)
            assert bool(torch.isnan(wbuf[:A.GUARD]).all()) and bool(torch.isnan(wbuf[-A.GUARD:]).all())
    # the rows differ, so the selection was seen; and the scalar path gives the same bits
    md = masks["quarter"].cuda()
    a = blend_then_ring_gather(x.cuda(), x0d, qnd[0], md, coefd[0], plan)
    assert not torch.equal(a[1], blend_then_ring_gather(x.cuda(), x0d, qnd[2], md, coefd[2], plan)[1])
    xu = off_by_one_float(x.cuda())
    assert torch.equal(bits(ops.window_blend_gather(xu, x0d, qnd[0], md, coefd[0], plan)), bits(a[1]))
    assert torch.equal(bits(xu), bits(a[0]))


# ---- 5. the wrappers' refusals --------------------------------------------------------------------------------------------------------
def test_ring_wrappers_refuse_what_they_cannot_run():
    from types import SimpleNamespace

    from audioldm2_amd import ops
    from audioldm2_amd.windows import window_plan
    B, C, F = 2, 3, 8
    plan = Lp.ring_plan((40, 16, 10))
    x, win = Wd.window_inputs(B, plan, C, F, H=2)
    xd, wd = x.cuda(), win.cuda()
    # a linear plan's starts handed to the ring entries with a gap > Tw: (48, 16, 16) has the starts 0, 16, 32 — as a ring over
    # T = 56 its wrap gap is 24 frames
    lin = window_plan(48, 16, 16)
    bad = SimpleNamespace(**dict(lin.__dict__, T=56, ring=True))
    bad.__dict__.pop("_starts_arg", None)
    with pytest.raises(RuntimeError, match="exceeds Tw"):
        ops.window_gather(torch.zeros(B, C, 56, F, device="cuda"), bad)
    with pytest.raises(RuntimeError, match="exceeds Tw"):
        ops.window_merge(torch.zeros(3 * B, C, 16, F, device="cuda"), bad)
    with pytest.raises(RuntimeError, match="exceeds Tw"):
        z = torch.zeros(B, C, 56, F, device="cuda")
        ops.window_blend_gather(z, z.clone(), z.clone(), z.clone(), torch.ones(2, device="cuda"), bad)
    # W = 1: the one-window linear plan (16, 16, 8) is no ring
    one = SimpleNamespace(**dict(window_plan(16, 16, 8).__dict__, ring=True))
    one.__dict__.pop("_starts_arg", None)
    with pytest.raises(RuntimeError, match="2 <= W"):
        ops.window_gather(torch.zeros(B, C, 16, F, device="cuda"), one)
    with pytest.raises(RuntimeError, match="2 <= W"):
        ops.window_merge(torch.zeros(B, C, 16, F, device="cuda"), one)
    # overlapping buffers
    n_win, n_out = win.numel(), 2 * x.numel()
    buf = torch.zeros(n_win + n_out, device="cuda")
    w = buf[:n_win].view(win.shape).copy_(win)
    with pytest.raises(RuntimeError, match="overlaps win"):
        ops.window_merge(w, plan, out=buf[n_win - 8:n_win - 8 + n_out].view((2,) + tuple(x.shape)))
    with pytest.raises(RuntimeError, match="overlaps x"):
        xs = buf[:x.numel()].view(x.shape)
        ops.window_gather(xs, plan, out=buf[x.numel() - 4:x.numel() - 4 + n_win // 2].view(plan.W * B, C, plan.Tw, F))
    with pytest.raises(RuntimeError, match="x overlaps x0"):
        ops.window_blend_gather(xd, xd, xd.clone(), xd.clone(), torch.ones(2, device="cuda"), plan)
    assert bool((buf[n_win:] == 0).all()) and torch.equal(xd, x.cuda())      # nothing ran
    with pytest.raises(RuntimeError, match="window_gather: x must be"):
        ops.window_gather(xd[:, :, :32].contiguous(), plan)
    with pytest.raises(RuntimeError, match="window_merge: win must be"):
        ops.window_merge(wd[:, :7].contiguous(), plan)


# ---- 6. the samplers on the tiny UNet -------------------------------------------------------------------------------------------------
LONG_KEY, STEPS, LONG_SHAPE, SEED = Lp.LONG_KEY, Lp.STEPS, Lp.LONG_SHAPE, 7


@pytest.fixture(scope="module")
def tiny():
    m = A.TinyModel()
    cond, uncond = A.tiny_conditioning()
    return m, cond, uncond


def x_long(seed=3, shape=LONG_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sampler_class(name):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp_2m": DPMSolverSampler}[name]


def run(name, tiny, plan, x_T=None, steps=STEPS, **kw):
    """One graph-replayed run from a fixed x_T under the seed, eta 0."""
    m, cond, uncond = tiny
    torch.manual_seed(SEED)
    x_T = x_long() if x_T is None else x_T
    out, _ = sampler_class(name)(m).sample(steps, x_T.shape[0], tuple(x_T.shape[1:]), cond, x_T=x_T, eta=0.0, windows=plan,
                                           t_start=steps, verbose=False, unconditional_guidance_scale=A.GS,
                                           unconditional_conditioning=uncond, **kw)
    return out


@pytest.fixture(scope="module")
def references(tiny):
    """The composition loops over RingModel, each computed once on first use."""
    m, cond, uncond = tiny
    plan = Lp.ring_plan(LONG_KEY)
    x0, mask = source()
    mask4 = mask.view(1, 1, -1, 1).expand(LONG_SHAPE).contiguous()
    loops = {"ddim": lambda: Lp.ddim_loop(m, plan, x_long(), cond, uncond, STEPS, A.GS, k=STEPS),
             "plms": lambda: Lp.plms_loop(m, plan, x_long(), cond, uncond, STEPS),
             "dpmpp_2m": lambda: Lp.dpmpp_loop(m, plan, x_long(), cond, uncond, STEPS),
             "ddim-source": lambda: Lp.ddim_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS, A.GS, eta=0.0, k=STEPS),
             "plms-source": lambda: Lp.plms_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS),
             "dpmpp_2m-source": lambda: Lp.dpmpp_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS)}
    done = {}

    def get(name):
        if name not in done:
            torch.manual_seed(SEED)
            done[name] = loops[name]()
        return done[name]
    return get


@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_sampler_on_a_ring_equals_the_composition_loop(tiny, references, name):
    plan = Lp.ring_plan(LONG_KEY)
    out = run(name, tiny, plan)
    assert tuple(out.shape) == LONG_SHAPE and bool(torch.isfinite(out).all())
    e, bar = A.rel_rms(out, references(name)), A.tstart_bar(STEPS)
    print(f"{name} ring={LONG_KEY} {STEPS} steps vs the composition loop over RingModel: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"ring {name}") <= bar
    assert A.rel_rms(out, x_long().cuda()) > 1e-3
    # a second run is bitwise the first
    assert torch.equal(run(name, tiny, plan), out)
    # ... and the ring is not the linear plan of the same numbers
    assert A.rel_rms(out, run(name, tiny, linear_plan(LONG_KEY))) > 1e-3


def linear_plan(key):
    from audioldm2_amd.windows import window_plan
    return window_plan(*key)


# ---- 7. no frame is special -----------------------------------------------------------------------------------------------------------
def test_a_roll_by_one_gap_rolls_the_result_and_a_linear_plan_fails_that_by_far(tiny):
    """DDIM, eta 0.  The ring plan (40, 16, 10) has four gaps of 10 frames: rolling by 10 maps the plan onto itself, window j onto
    window j+1, so only the order in which the merge accumulates its terms differs — hence a bar, not torch.equal.  The control: the
    linear plan of the same numbers (starts 0, 10, 20, 24) has a first and a last frame and must miss the bar by 100x or more."""
    shift = 10
    ring = Lp.ring_plan(LONG_KEY)
    assert all(b - a == shift for a, b in zip(ring.starts, ring.starts[1:] + (ring.T,)))
    bar = A.tstart_bar(STEPS)
    x_T = x_long()
    rolled_in = torch.roll(x_T, shift, dims=2).contiguous()
    out, out_rolled = run("ddim", tiny, ring, x_T=x_T), run("ddim", tiny, ring, x_T=rolled_in)
    e = A.rel_rms(out_rolled, torch.roll(out, shift, dims=2))
    print(f"ring {LONG_KEY}: run(roll(x_T, {shift})) vs roll(run(x_T), {shift}): rel rms {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "ring roll") <= bar
    lin = linear_plan(LONG_KEY)
    lout, lout_rolled = run("ddim", tiny, lin, x_T=x_T), run("ddim", tiny, lin, x_T=rolled_in)
    c = A.rel_rms(lout_rolled, torch.roll(lout, shift, dims=2))
    print(f"control, linear {LONG_KEY}: the same pair of inputs: rel rms {c:.2e}  (100 x bar = {100 * bar:.1e})")
    assert c >= 100 * bar


# ---- 8. a ring with a source ------------------------------------------------------------------------------------------------------------
def source(shape=LONG_SHAPE, keep=Ls.KEEP):
    from audioldm2_amd.windows import keep_mask
    return torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda(), keep_mask(shape[2], keep)


@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_sampler_on_a_ring_with_a_source_equals_the_loop_with_the_blend_in_front_of_each_step(tiny, references, name):
    """The loops of tests/long_source.py over RingModel: per step the q-noise draw, the blend on the long latent (a torch
    restatement of ops.inpaint_blend's expression), then the sampler's eager single step."""
    from audioldm2_amd.windows import with_source
    x0, mask = source()
    plan = with_source(Lp.ring_plan(LONG_KEY), x0, mask)
    assert plan.ring is True
    out = run(name, tiny, plan)
    e, bar = A.rel_rms(out, references(name + "-source")), A.tstart_bar(STEPS)
    print(f"{name} ring={LONG_KEY} keep={Ls.KEEP} vs the composition loop over RingModel: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"ring source {name}") <= bar
    assert torch.equal(run(name, tiny, with_source(Lp.ring_plan(LONG_KEY), x0, mask)), out)
    assert A.rel_rms(out, run(name, tiny, Lp.ring_plan(LONG_KEY))) > 1e-3          # the source matters


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED, E2E_TEXT = 384, 128, 2, 42, "rain on a tin roof"


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def loop_job(ld, T=E2E_T, hop=E2E_HOP, **kw):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    seed_everything(E2E_SEED)
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = ld.generate_batch_long(make_batch_for_text_to_audio(E2E_TEXT), T, hop=hop, ddim_steps=E2E_STEPS,
                                  unconditional_guidance_scale=A.GS, loop=True, **kw)
    return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), float(torch.rand(1))


def conditioning(ld):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    cond = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(E2E_TEXT))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    return cond, uncond


def test_generate_batch_long_loop_end_to_end(ld):
    from audioldm2_amd.pipeline import seed_everything, text_to_audio_long
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, E2E_HOP, ring=True)
    assert (plan.W, plan.starts, mel_plan.starts, mel_plan.Tw) == (3, (0, 128, 256), (0, 512, 1024), 1024)
    wave, latent, mel, rand_after = loop_job(ld)
    C, F_ = ld.channels, ld.latent_f_size
    voc = ld.first_stage_model.vocoder
    h = int(np.prod(voc.h.upsample_rates))
    assert tuple(latent.shape) == (1, C, E2E_T, F_) and tuple(mel.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.shape == (1, 1, E2E_T * 4 * h) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert ld.latent_t_size == 256
    # a loop draws what a linear job draws
    assert rand_after == Wd.expected_rand_after_long(E2E_SEED, 1, (C, 256, F_), (C, E2E_T, F_), E2E_STEPS)

    # the latent: the composition loop — the job's draws by hand, DDIMSampler.decode over the ring model
    seed_everything(E2E_SEED)
    torch.randn((1, C, 256, F_))
    cond, uncond = conditioning(ld)
    ref = Lp.ddim_loop(ld, plan, torch.randn((1, C, E2E_T, F_)), cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"loop latent vs the composition loop over RingModel: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "loop latent") <= latent_tol(E2E_STEPS)

    # the mel: an fp64 ring merge of decode_first_stage on the rolled-and-sliced windows of the job's own latent
    mel_ref = Lp.ring_merge_fp64(ld.decode_first_stage(Lp.ring_gather_ref(latent, plan)), mel_plan)[0]
    e = A.rel_rms(mel, mel_ref)
    print(f"loop mel vs the fp64 ring merge of the windows' decodes: rel rms {e:.2e}  bar {mel_tol(E2E_STEPS):.1e}")
    assert log_err(e, mel_tol(E2E_STEPS), "loop mel") <= mel_tol(E2E_STEPS)

    # the junction: the wave is the middle period of the vocoder over three periods of the mel — a reference that knows nothing of
    # the pad the tail derives from the vocoder's config
    T_mel = mel.shape[-2]
    three = voc.forward_cl(torch.cat([mel[:, 0]] * 3, dim=1).float().contiguous())
    middle = three[..., T_mel * h:2 * T_mel * h].cpu().numpy()
    e = A.rms(wave - middle) / A.rms(middle)
    print(f"loop wave vs the middle period of the vocoder over three periods of the mel: rel rms {e:.2e}  bar {tail_tol():.1e}")
    assert log_err(e, tail_tol(), "loop junction") <= tail_tol()
    # ... which the linear tail's wave (zero padding at both ends) is not: the check can see a junction
    lin = voc.forward_cl(mel[:, 0].float().contiguous())[..., :T_mel * h].cpu().numpy()
    assert A.rms(lin - middle) / A.rms(middle) > 10 * tail_tol()

    # a second job replays the one cached graph and is bitwise the first
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and ent["win"].plan.starts == plan.starts and ent["win"].plan.ring is True
    wave2, latent2, _, rand2 = loop_job(ld)
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent
    assert torch.equal(latent2, latent) and np.array_equal(wave2, wave) and rand2 == rand_after

    # the entry point: 15 s with 5 s of overlap, loop=True, is this very job
    ld.conditional_dry_run_finished = False
    wave3 = text_to_audio_long(ld, E2E_TEXT, duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS, guidance_scale=A.GS,
                               loop=True)
    assert np.array_equal(wave3, wave) and ld.latent_t_size == 256
    unet.drop_step_caches()


# ---- 10. a loop of the trained length ---------------------------------------------------------------------------------------------------
def test_a_loop_of_the_trained_length(ld):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    T = ld.latent_t_size
    plan, mel_plan = ld.long_form_plans(T, ring=True)
    assert (plan.W, plan.starts) == (2, (0, 128))
    wave, latent, mel, rand_after = loop_job(ld, T=T, hop=None)
    C, F_ = ld.channels, ld.latent_f_size
    h = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert bool(torch.isfinite(latent).all()) and np.isfinite(wave).all() and wave.shape == (1, 1, T * 4 * h)
    seed_everything(E2E_SEED)
    torch.randn((1, C, 256, F_))
    cond, uncond = conditioning(ld)
    ref = Lp.ddim_loop(ld, plan, torch.randn((1, C, T, F_)), cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"loop of the trained length, latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "loop T == Tw latent") <= latent_tol(E2E_STEPS)
    # generate_batch under the same seed draws the same x_T and step noise, but its clip has two ends
    seed_everything(E2E_SEED)
    ld.conditional_dry_run_finished = False
    kept = {}
    decode = ld.decode_first_stage_cl

    def decode_and_keep(z):
        kept["z"] = z.clone()
        return decode(z)
    ld.decode_first_stage_cl = decode_and_keep      # the job's tail decodes its final latent: keep it
    try:
        ld.generate_batch(make_batch_for_text_to_audio(E2E_TEXT), ddim_steps=E2E_STEPS, unconditional_guidance_scale=A.GS, n_gen=1)
    finally:
        del ld.decode_first_stage_cl
    d = A.rel_rms(latent, kept["z"])
    print(f"loop of the trained length vs generate_batch under the same seed: rel rms {d:.2e}")
    assert tuple(kept["z"].shape) == tuple(latent.shape) and d > 1e-3
    unet.drop_step_caches()


# ---- 11. a loop round a source ----------------------------------------------------------------------------------------------------------
def source_audio(seconds=5):
    """A seeded synthetic recording at 16 kHz: two tones under a slow envelope, and a little noise."""
    rng = np.random.RandomState(0)
    t = np.arange(seconds * 16000) / 16000.0
    return ((np.sin(2 * np.pi * 220.0 * t) + 0.5 * np.sin(2 * np.pi * 1330.0 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
            + 0.05 * rng.randn(t.shape[0])).astype(np.float32)


def test_generate_batch_long_from_audio_loop(ld):
    from audioldm2_amd import extend_audio
    from audioldm2_amd.pipeline import keep_frames, seed_everything
    from audioldm2_amd.windows import keep_mask
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    ld.conditional_dry_run_finished = False
    wave = extend_audio(ld, E2E_TEXT, source_audio(), duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS,
                        guidance_scale=A.GS, loop=True)
    latent, z, rand_after = ld.last_long_latent.clone(), ld.last_long_source.clone(), float(torch.rand(1))
    C, F_ = ld.channels, ld.latent_f_size
    h = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert wave.shape == (1, 1, E2E_T * 4 * h) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert tuple(latent.shape) == tuple(z.shape) == (1, C, E2E_T, F_)
    # the draws are the linear job's
    assert rand_after == Ls.expected_rand_after_source(E2E_SEED, 1, (C, E2E_T, F_), E2E_STEPS)
    # the ring loop with the blend, from the job's own source latent (encoded on the linear plans); the default keep: [0, 5 s)
    frames = keep_frames([(0.0, 5.0)], ld.latent_t_per_second, E2E_T)
    assert frames == [(0, 128)]
    mask4 = keep_mask(E2E_T, frames).view(1, 1, -1, 1).expand(1, C, E2E_T, F_).contiguous()
    plan, _ = ld.long_form_plans(E2E_T, E2E_HOP, ring=True)
    seed_everything(E2E_SEED)
    torch.randn((1, C, E2E_T, F_))
    cond, uncond = conditioning(ld)
    ref = Lp.ddim_source_loop(ld, plan, torch.randn((1, C, E2E_T, F_)), z, mask4, cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent[:, :, :128], ref[:, :, :128])
    print(f"loop round a source, kept frames of the latent vs the ring loop with the blend: rel rms {e:.2e}  "
          f"bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "loop source latent, kept frames") <= latent_tol(E2E_STEPS)
    e = A.rel_rms(latent, ref)
    print(f"... all frames: rel rms {e:.2e}")
    assert e <= latent_tol(E2E_STEPS)
    unet.drop_step_caches()
