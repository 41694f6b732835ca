"""GPU tests of continuation and inpainting of long clips: aldm_window_blend_gather against ops.inpaint_blend followed
by ops.window_gather (bitwise) and against fp64 (bar: three roundings of the sum of the terms' magnitudes, tests/long_source.py), its
device-side row selection, bounds and refusals; LatentDiffusion.encode_long on the VAE encoder at a small trained shape; the three
samplers with a source on the window plan against the composition loop (torch blend with hand-drawn q-noise, slice, same model, fp64
merge, the sampler's eager single-step form), their degenerate cases (a zero mask, a one-window plan); extend_audio end to end."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import audio2audio as A
import long_source as Ls
import windowed as Wd
from tolerances import latent_tol, log_err, mel_tol

pytestmark = pytest.mark.gpu

NAN = float("nan")


def plan_of(key, scale=1):
    from audioldm2_amd.windows import window_plan
    return window_plan(*key, scale=scale)


def case_id(c):
    B, key, C, F = c
    return f"B{B}-T{key[0]}w{key[1]}h{key[2]}-C{C}-F{F}"


def bits(t):
    return t.contiguous().view(torch.int32)


def nan_guarded(shape):
    """A.guarded with NaN everywhere: the view and GUARD floats on each side."""
    return A.guarded(shape, fill=NAN)


def nan_guards_intact(buf):
    return bool(torch.isnan(buf[:A.GUARD]).all()) and bool(torch.isnan(buf[-A.GUARD:]).all())


def blend_then_gather(x, x0, qn, m, coef_row, plan):
    """The two launches the fused one replaces, on a copy."""
    from audioldm2_amd import ops
    ref_x = x.clone()
    ops.inpaint_blend(ref_x, x0, qn.contiguous(), m, coef_row.contiguous())
    return ref_x, ops.window_gather(ref_x, plan)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Wd.KERNEL_CASES, ids=case_id)
def test_blend_gather_is_bitwise_blend_then_gather_and_within_three_roundings_of_fp64(case):
    from audioldm2_amd import ops
    B, key, C, F = case
    plan = plan_of(key)
    x, x0, qn, coef = Ls.blend_inputs(B, plan, C, F, S=1)
    sa, so = coef[0].tolist()
    x0d, qnd, coefd = x0.cuda(), qn.cuda(), coef.cuda()
    for name, m in Ls.mask_patterns(plan, tuple(x.shape)).items():
        md = m.cuda()
        xg, xbuf = A.guarded(tuple(x.shape))
        xg.copy_(x)
        win, wbuf = nan_guarded((plan.W * B, C, plan.Tw, F))
        ref_x, ref_win = blend_then_gather(x.cuda(), x0d, qnd[0], md, coefd[0], plan)
        got = ops.window_blend_gather(xg, x0d, qnd, md, coefd, plan, out=win)
        assert got is win
        assert torch.equal(bits(xg), bits(ref_x)), f"{name}: x differs from ops.inpaint_blend"
        assert torch.equal(bits(win), bits(ref_win)), f"{name}: win differs from ops.window_gather of the blended x"
        assert not bool(torch.isnan(win).any()) and nan_guards_intact(wbuf) and A.guards_intact(xbuf)
        keep0 = md == 0
        assert torch.equal(bits(xg)[keep0], bits(x.cuda())[keep0])         # where m == 0, x is bitwise its input
        ref, den = Ls.blend_fp64(x, x0, qn[0], m, sa, so)
        err = float(((xg.double().cpu() - ref).abs() / den).max())
        print(f"window_blend_gather {case_id(case)} mask {name}: max |err| / (|sa x0| + |so qn| + |x|) = {err:.3e}  "
              f"bar {Ls.BLEND_BAR:.3e}")
        assert log_err(err, Ls.BLEND_BAR, f"window_blend_gather {case_id(case)} {name}") <= Ls.BLEND_BAR
        # the windows against the fp64 restatement of blend-then-gather: the same figure, seen through the gather
        werr = float(((win.double().cpu() - Ls.blend_gather_fp64(x, x0, qn[0], m, sa, so, plan)).abs()
                      / Wd.gather_ref(den, plan)).max())
        assert werr <= Ls.BLEND_BAR
        # the allocating form, with the q-noise as one row [B, C, T, F]
        x2 = x.cuda()
        assert torch.equal(bits(ops.window_blend_gather(x2, x0d, qnd[0], md, coefd[0], plan)), bits(ref_win))
        assert torch.equal(bits(x2), bits(ref_x))


def test_rows_are_selected_on_the_device_and_saturate():
    from audioldm2_amd import ops
    B, key, C, F = 2, (40, 16, 10), 3, 8
    plan = plan_of(key)
    S = 3
    x, x0, qn, coef = Ls.blend_inputs(B, plan, C, F, S=S, seed=1)
    m = Ls.mask_patterns(plan, tuple(x.shape))["quarter"].cuda()
    xd, x0d, qnd, coefd = x.cuda(), x0.cuda(), qn.cuda(), coef.cuda()
    assert not torch.equal(qnd[0], qnd[2]) and not torch.equal(coefd[0], coefd[2])

    def fused(q, c, idx):
        xx = xd.clone()
        step_idx = None if idx is None else torch.full((1,), idx, device="cuda", dtype=torch.int32)
        win = ops.window_blend_gather(xx, x0d, q, m, c, plan, step_idx=step_idx)
        if step_idx is not None:
            assert int(step_idx) == idx                 # the counter is read, not written
        return xx, win

    def want(qrow, crow):
        return blend_then_gather(xd, x0d, qnd[qrow], m, coefd[crow], plan)
    # (step_idx, q-noise table, coefficient table) -> (q row, coefficient row)
    for idx, q, c, qrow, crow in ((0, qnd, coefd, 0, 0), (1, qnd, coefd, 1, 1), (2, qnd, coefd, 2, 2), (5, qnd, coefd, 2, 2),
                                  (2, qnd[:1].contiguous(), coefd, 0, 2), (2, qnd[0].contiguous(), coefd, 0, 2),
                                  (None, qnd, coefd, 0, 0), (2, qnd, coefd[:2].contiguous(), 2, 1)):
        (gx, gw), (rx, rw) = fused(q, c, idx), want(qrow, crow)
        assert torch.equal(bits(gx), bits(rx)) and torch.equal(bits(gw), bits(rw)), (idx, tuple(q.shape), tuple(c.shape))
    # ... and the rows differ, so the selection was seen
    assert not torch.equal(want(0, 0)[0], want(1, 1)[0]) and not torch.equal(want(0, 2)[0], want(2, 2)[0])


def test_unaligned_pointers_take_the_scalar_path_and_give_the_same_bits():
    """F % 4 == 0 but one tensor starts 4 bytes off a 16-byte boundary: the same results as the aligned launch."""
    from audioldm2_amd import ops
    B, key, C, F = 1, (40, 16, 10), 3, 16
    plan = plan_of(key)
    x, x0, qn, coef = Ls.blend_inputs(B, plan, C, F, S=2, seed=2)
    a, b = Ls.overlap_interval(plan)
    m = Ls.mask_patterns(plan, tuple(x.shape))[f"keep[{a},{b})"].cuda()
    x0d, qnd, coefd = x0.cuda(), qn.cuda(), coef.cuda()
    idx = torch.ones(1, device="cuda", dtype=torch.int32)
    ref_x = x.cuda()
    ref_win = ops.window_blend_gather(ref_x, x0d, qnd, m, coefd, plan, step_idx=idx)

    def off(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        u = buf[1:].view(t.shape).copy_(t)
        assert u.data_ptr() % 16 == 4
        return u
    for which in ("x", "x0", "qnoise", "mask", "win"):
        xu = off(x.cuda()) if which == "x" else x.cuda()
        out = off(torch.full_like(ref_win, NAN)) if which == "win" else None
        win = ops.window_blend_gather(xu, off(x0d) if which == "x0" else x0d, off(qnd) if which == "qnoise" else qnd,
                                      off(m) if which == "mask" else m, coefd, plan, step_idx=idx, out=out)
        assert torch.equal(bits(win), bits(ref_win)) and torch.equal(bits(xu), bits(ref_x)), which


def test_wrapper_refuses_what_it_cannot_run_and_launches_nothing():
    from audioldm2_amd import ops
    B, C, F = 2, 3, 8
    plan = plan_of((40, 16, 10))
    x, x0, qn, coef = Ls.blend_inputs(B, plan, C, F, S=2)
    n_x, n_w = x.numel(), plan.W * B * C * plan.Tw * F
    buf = torch.zeros(n_x + n_w, device="cuda")
    xs = buf[:n_x].view(x.shape)
    x0d, qnd, md, coefd = x0.cuda(), qn.cuda(), torch.ones_like(x).cuda(), coef.cuda()
    wshape = (plan.W * B, C, plan.Tw, F)
    with pytest.raises(RuntimeError, match="out overlaps x"):
        ops.window_blend_gather(xs, x0d, qnd, md, coefd, plan, out=buf[n_x - 4:n_x - 4 + n_w].view(wshape))
    both = torch.zeros(2 * n_x + n_w, device="cuda")                          # a two-row q-noise table, the windows behind it
    with pytest.raises(RuntimeError, match="out overlaps qnoise"):
        ops.window_blend_gather(xs, x0d, both[:2 * n_x].view(qn.shape), md, coefd, plan,
                                out=both[2 * n_x - 4:2 * n_x - 4 + n_w].view(wshape))
    with pytest.raises(RuntimeError, match="x overlaps x0"):
        ops.window_blend_gather(xs, xs, qnd, md, coefd, plan)
    with pytest.raises(RuntimeError, match="x overlaps mask"):
        ops.window_blend_gather(xs, x0d, qnd, xs, coefd, plan)
    assert bool((buf == 0).all()) and bool((both == 0).all())                  # nothing ran
    xd = x.cuda()
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.window_blend_gather(x, x0d, qnd, md, coefd, plan)                  # a host tensor
    with pytest.raises(RuntimeError, match="contiguous fp32 CUDA"):
        ops.window_blend_gather(xd, x0d.double(), qnd, md, coefd, plan)
    with pytest.raises(RuntimeError, match="window_blend_gather: x must be"):
        ops.window_blend_gather(xd[:, :, :32].contiguous(), x0d, qnd, md, coefd, plan)
    with pytest.raises(RuntimeError, match="window_blend_gather.x0: expected"):
        ops.window_blend_gather(xd, x0d[:1].contiguous(), qnd, md, coefd, plan)
    with pytest.raises(RuntimeError, match="window_blend_gather.mask: expected"):
        ops.window_blend_gather(xd, x0d, qnd, md[:, :1].contiguous(), coefd, plan)
    with pytest.raises(RuntimeError, match="window_blend_gather.qnoise: expected"):
        ops.window_blend_gather(xd, x0d, qnd[:, :1].contiguous(), md, coefd, plan)
    with pytest.raises(RuntimeError, match="window_blend_gather.blend_coef: expected"):
        ops.window_blend_gather(xd, x0d, qnd, md, torch.zeros(2, 3, device="cuda"), plan)
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.window_blend_gather(xd, x0d, qnd, md, coefd, plan, step_idx=torch.zeros(1, device="cuda"))
    with pytest.raises(RuntimeError, match="window_blend_gather.out: expected"):
        ops.window_blend_gather(xd, x0d, qnd, md, coefd, plan, out=torch.empty(B, C, plan.Tw, F, device="cuda"))
    assert torch.equal(xd, x.cuda())


# ---- 2. encoding a source longer than the VAE's trained shape ----------------------------------------------------------------------
def test_encode_long_merges_the_window_moments_and_samples_them():
    """The real encoder (the 16 kHz ddconfig, deterministic weights) at a small trained shape: windows of 64 mel frames of a 160-frame
    mel, windowed.MEL_CASE — the latent plan (40, 16, 12), the mel plan its scale by 4."""
    from audioldm2_amd.pipeline import LatentDiffusion
    from audioldm2_amd.vae import AutoencoderKL
    from oracle import cases, weights
    B0, mel_key, _, F_mel = Wd.MEL_CASE
    f = 4
    plan, mel_plan = plan_of(tuple(v // f for v in mel_key)), plan_of(tuple(v // f for v in mel_key), scale=f)
    assert (mel_plan.T, mel_plan.Tw, mel_plan.hop) == mel_key and plan.W == 3 and plan.cover == 2
    ae = AutoencoderKL(ddconfig=cases.DDCONFIG_16K, embed_dim=8, image_key="fbank")
    ae.load_state_dict(weights.make_state_dict(weights.shapes_of(ae), seed=0))
    ae.cuda()
    C, F = 8, F_mel // f
    stub = SimpleNamespace(first_stage_model=ae, scale_factor=A.KERNEL_SCALE, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(4)
    mel = (torch.randn(B0, 1, mel_plan.T, F_mel, generator=g) * 2.0 - 4.0).cuda()
    n_post = torch.randn(B0, C, plan.T, F, generator=g).cuda()
    z = LatentDiffusion.encode_long(stub, mel, plan, mel_plan, n_post)
    moments = stub.last_long_moments
    assert tuple(z.shape) == (B0, C, plan.T, F) and tuple(moments.shape) == (B0, plan.T, F, 2 * C)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(moments).all())
    # the long moments against an fp64 merge of the per-window encodes
    mom_w = ae.encode_moments_cl(Wd.gather_ref(mel, mel_plan))                     # [W*B0, Tw, F, 2C]
    ref, den, count = Wd.merge_fp64(mom_w.view(mom_w.shape[0], 1, plan.Tw, F * 2 * C), plan)
    got = moments.view(B0, 1, plan.T, F * 2 * C)
    err, bar = float(((got.double() - ref).abs() / den).max()), Wd.bar(plan)
    print(f"encode_long moments vs the fp64 merge of the windows' moments: {err:.3e}  bar {bar:.3e}")
    assert log_err(err, bar, "encode_long moments") <= bar
    # frames under one window are that window's moments, bit for bit
    one = (count == 1).nonzero().view(-1).tolist()
    assert len(one) > 0
    for t in one:
        j = max(i for i, s in enumerate(plan.starts) if s <= t < s + plan.Tw)
        assert torch.equal(bits(moments[:, t]), bits(mom_w[j * B0:(j + 1) * B0, t - plan.starts[j]]))
    # z = scale * (mean + exp(0.5 logvar) n_post) in fp64 from the long moments: posterior_qsample's bar
    zr, _, dz, _ = A.kernel_fp64(moments.cpu(), n_post.cpu(), n_post.cpu(), A.KERNEL_SCALE, 1.0, 0.0)
    ez = float(((z.double().cpu() - zr).abs() / dz).max())
    print(f"encode_long z vs fp64 of the long moments: {ez:.3e}  bar {A.KERNEL_BAR:.1e}")
    assert log_err(ez, A.KERNEL_BAR, "encode_long z") <= A.KERNEL_BAR
    with pytest.raises(ValueError, match="do not fit the plans"):
        LatentDiffusion.encode_long(stub, mel[:, :, :128].contiguous(), plan, mel_plan, n_post)


# ---- 3. the samplers on the tiny UNet ------------------------------------------------------------------------------------------------
LONG_KEY, STEPS, LONG_SHAPE, SEED = Ls.LONG_KEY, Ls.STEPS, Ls.LONG_SHAPE, 7


@pytest.fixture(scope="module")
def tiny():
    m = A.TinyModel()
    cond, uncond = A.tiny_conditioning()
    return m, cond, uncond


def x_long(seed=3, shape=LONG_SHAPE):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def source(shape=LONG_SHAPE, keep=Ls.KEEP):
    from audioldm2_amd.windows import keep_mask
    return torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda(), keep_mask(shape[2], keep)


def sampler_class(name):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp_2m": DPMSolverSampler}[name]


def run(name, tiny, plan, shape=LONG_SHAPE, steps=STEPS, eta=0.0, **kw):
    """One graph-replayed run from a fixed x_T under the seed -> (latent, the rand(1) that follows it)."""
    m, cond, uncond = tiny
    torch.manual_seed(SEED)
    out, _ = sampler_class(name)(m).sample(steps, shape[0], shape[1:], cond, x_T=x_long(shape=shape), eta=eta, windows=plan,
                                           t_start=steps, verbose=False, unconditional_guidance_scale=A.GS,
                                           unconditional_conditioning=uncond, **kw)
    return out, float(torch.rand(1))


def src_plan(key=LONG_KEY, shape=LONG_SHAPE, keep=Ls.KEEP, mask=None):
    from audioldm2_amd.windows import with_source
    x0, m = source(shape, keep)
    return with_source(plan_of(key), x0, m if mask is None else mask)


CONFIGS = {"ddim": ("ddim", dict(eta=0.0)), "ddim-eta1": ("ddim", dict(eta=1.0)), "plms": ("plms", {}), "dpmpp_2m": ("dpmpp_2m", {}),
           "ddim-rescale": ("ddim", dict(eta=0.0, guidance_rescale=0.7))}


@pytest.fixture(scope="module")
def references(tiny):
    """The composition loops, each computed once on first use -> (latent, the rand(1) after performing the run's draws by hand)."""
    m, cond, uncond = tiny
    plan = plan_of(LONG_KEY)
    x0, mask = source()
    mask4 = mask.view(1, 1, -1, 1).expand(LONG_SHAPE).contiguous()
    done = {}

    def get(cfg):
        if cfg not in done:
            torch.manual_seed(SEED)
            if cfg.startswith("ddim"):
                kw = CONFIGS[cfg][1]
                ref = Ls.ddim_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS, A.GS, eta=kw["eta"],
                                          guidance_rescale=kw.get("guidance_rescale", 0.0), k=STEPS)
            elif cfg == "plms":
                ref = Ls.plms_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS)
            else:
                ref = Ls.dpmpp_source_loop(m, plan, x_long(), x0, mask4, cond, uncond, STEPS)
            done[cfg] = (ref, float(torch.rand(1)))
        return done[cfg]
    return get


@pytest.mark.parametrize("cfg", ["ddim", "ddim-eta1", "plms", "dpmpp_2m", "ddim-rescale"])
def test_sampler_with_a_source_equals_the_composition_loop(tiny, references, cfg):
    name, kw = CONFIGS[cfg]
    out, rand_after = run(name, tiny, src_plan(), **kw)
    assert tuple(out.shape) == LONG_SHAPE and bool(torch.isfinite(out).all())
    ref, rand_ref = references(cfg)
    e, bar = A.rel_rms(out, ref), A.tstart_bar(STEPS)
    print(f"{cfg} windows={LONG_KEY} keep={Ls.KEEP} {STEPS} steps vs the composition loop: {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, f"long source {cfg}") <= bar
    # the host generator ends where the contract says: after the q-noise and the sampler's own draws of every step
    assert rand_after == rand_ref
    # a second run is bitwise the first
    out2, rand2 = run(name, tiny, src_plan(), **kw)
    assert torch.equal(out2, out) and rand2 == rand_after
    # ... and the source matters
    plain, _ = run(name, tiny, plan_of(LONG_KEY), **kw)
    d = A.rel_rms(out, plain)
    print(f"{cfg}: with a source vs without: rel rms {d:.2e}")
    assert d > 1e-3


@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_a_mask_of_zeros_is_bitwise_the_plain_windowed_run(tiny, name):
    """The blend is exact at m == 0, so only the launch differs (eta 0: the extra q-noise draws shift no value)."""
    zeros, _ = run(name, tiny, src_plan(mask=torch.zeros(LONG_SHAPE[2])))
    plain, _ = run(name, tiny, plan_of(LONG_KEY))
    assert torch.equal(zeros, plain)


@pytest.mark.parametrize("name", ["ddim", "plms", "dpmpp_2m"])
def test_a_one_window_plan_with_a_source_is_bitwise_the_masked_run_without_windows(tiny, name):
    m, cond, uncond = tiny
    shape, steps, keep = A.TINY_SHAPE, 4, [(0, 5), (9, 12)]
    with_plan, rand_plan = run(name, tiny, src_plan((16, 16, 8), shape, keep), shape=shape, steps=steps)
    x0, mask = source(shape, keep)
    torch.manual_seed(SEED)
    masked, _ = sampler_class(name)(m).sample(steps, shape[0], shape[1:], cond, x_T=x_long(shape=shape), eta=0.0, t_start=steps,
                                              mask=mask.view(1, 1, -1, 1), x0=x0, verbose=False,
                                              unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond)
    assert float(torch.rand(1)) == rand_plan
    assert torch.equal(with_plan, masked)


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------
E2E_T, E2E_STEPS, E2E_SEED, E2E_TEXT = 384, 2, 42, "rain on a tin roof"


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def source_audio():
    """A seeded synthetic 6 s recording at 16 kHz: two tones under a slow envelope, and a little noise."""
    rng = np.random.RandomState(0)
    t = np.arange(6 * 16000) / 16000.0
    return ((np.sin(2 * np.pi * 220.0 * t) + 0.5 * np.sin(2 * np.pi * 1330.0 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
            + 0.05 * rng.randn(t.shape[0])).astype(np.float32)


def extend_job(ld, **kw):
    from audioldm2_amd import extend_audio
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = extend_audio(ld, E2E_TEXT, source_audio(), duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS,
                        guidance_scale=A.GS, **kw)
    return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), ld.last_long_source.clone(), float(torch.rand(1))


def test_extend_audio_end_to_end(ld):
    from audioldm2_amd.pipeline import keep_frames, make_batch_for_text_to_audio, seed_everything
    from audioldm2_amd.windows import keep_mask
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, 128)
    wave, latent, mel, z, rand_after = extend_job(ld)
    C, F_ = ld.channels, ld.latent_f_size
    hop_length = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert tuple(latent.shape) == tuple(z.shape) == (1, C, E2E_T, F_) and tuple(mel.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.shape == (1, 1, E2E_T * 4 * hop_length) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert ld.latent_t_size == 256
    assert len(unet._graph_cache) == 0            # like a masked run, a run with a source stays out of the cross-run graph cache
    # the host generator after the job (generate_batch_long_from_audio's docstring)
    assert rand_after == Ls.expected_rand_after_source(E2E_SEED, 1, (C, E2E_T, F_), E2E_STEPS)

    # the latent: the composition loop — the job's draws by hand, the job's own source latent, the default keep: [0, 6 s)
    frames = keep_frames([(0.0, 6.0)], ld.latent_t_per_second, E2E_T)
    assert frames == [(0, 153)]
    mask4 = keep_mask(E2E_T, frames).view(1, 1, -1, 1).expand(1, C, E2E_T, F_).contiguous()
    seed_everything(E2E_SEED)
    torch.randn((1, C, E2E_T, F_))
    cond = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(E2E_TEXT))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    ref = Ls.ddim_source_loop(ld, plan, torch.randn((1, C, E2E_T, F_)), z, mask4, cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"extend_audio latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "long source latent") <= latent_tol(E2E_STEPS)

    # the mel: an fp64 merge of decode_first_stage on the sliced windows of the job's own latent
    mel_ref = Wd.merge_fp64(ld.decode_first_stage(Wd.gather_ref(latent, plan)), mel_plan)[0]
    e = A.rel_rms(mel, mel_ref)
    print(f"extend_audio mel vs the fp64 merge of the windows' decodes: rel rms {e:.2e}  bar {mel_tol(E2E_STEPS):.1e}")
    assert log_err(e, mel_tol(E2E_STEPS), "long source mel") <= mel_tol(E2E_STEPS)

    # the kept frames stay nearer the source than the generated ones (comparative only)
    kept, gen = A.rel_rms(latent[:, :, :153], z[:, :, :153]), A.rel_rms(latent[:, :, 153:], z[:, :, 153:])
    print(f"extend_audio final latent vs the source latent: kept frames {kept:.3e}, generated frames {gen:.3e} (rel rms)")
    assert kept < gen

    # a second identical job is bitwise the first
    wave2, latent2, _, z2, rand2 = extend_job(ld)
    assert torch.equal(latent2, latent) and torch.equal(z2, z) and np.array_equal(wave2, wave) and rand2 == rand_after


def test_extend_audio_keeps_an_interval_inside_the_source(ld):
    default = extend_job(ld)
    wave, latent, _, z, rand_after = extend_job(ld, keep=[(2.0, 4.0)])
    assert np.isfinite(wave).all() and bool(torch.isfinite(latent).all()) and wave.shape == default[0].shape
    assert torch.equal(z, default[3]) and rand_after == default[4]          # the same source, the same draws
    d = A.rel_rms(latent, default[1])
    print(f"extend_audio keep=[(2, 4)] vs the default keep: rel rms {d:.2e}")
    assert d > 1e-3 and not np.array_equal(wave, default[0])
    ld.model.diffusion_model.drop_step_caches()
