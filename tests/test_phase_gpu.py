"""GPU tests of moving window phases: the three `_ring_phased` launches against their bitwise identities — the ring
launch of the rolled problem, restated with torch.roll over tests/looped.py — and the merge against the fp64 ring merge of the rolled
problem; the device-side row selection and its clamps; table values just outside [0, T) inside fenced allocations; NaN locality at a
rotated, wrapped position; the three samplers under the golden table on the tiny UNet against the composition loops of
tests/phased.py (per UNet pass: roll by -phi, looped.RingModel, roll back), with a source, guidance rescale, resample= and graded
levels; a constant table against the rolled ring run; two tables of one length on one cached step graph of the real UNet; and
generate_batch_long / text_to_audio_long / extend_audio with loop=True, phase= end to end.

The end-to-end jobs run FOUR steps where a three-step job would do: the uniform grid of ddim_steps=3 over 1000 timesteps ends on
timestep 1000, outside the schedule (no sampler here or in the reference runs it).  Four steps give the golden phases 0, 79, 30, 109
on the ring (384, 256, 128): the eager step sees 0, the capture 79, and two replays run under phases neither of them saw."""
import numpy as np
import pytest
import torch

import audio2audio as A
import graded as Gd
import long_source as Ls
import looped as Lp
import phased as Ph
import windowed as Wd
from tolerances import latent_tol, log_err, mel_tol, tail_tol

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILL = -777.0


def case_id(c):
    B, key, C, F = c
    return f"B{B}-T{key[0]}w{key[1]}h{key[2]}-C{C}-F{F}"


CASES = [pytest.param(i, c, id=case_id(c)) for i, c in enumerate(Ph.KERNEL_CASES)]


def bits(t):
    return t.contiguous().view(torch.int32)


def off_by_one_float(t):
    """A copy of `t` that starts 4 bytes off a 16-byte boundary: the launches on it take the scalar path."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    u = buf[1:].view(t.shape).copy_(t)
    assert u.data_ptr() % 16 == 4
    return u


def counter(v):
    return torch.full((1,), v, device="cuda", dtype=torch.int32)


def table_plan(plan, phases):
    """`plan` with the phases as its table, the table on the device, and the row of every phase."""
    p = Ph.phased(plan, phases)
    return p, p.phase.cuda(), {int(f): r for r, f in enumerate(phases)}


# ---- 1. the gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", CASES)
def test_phased_gather_is_bitwise_the_ring_gather_of_the_rolled_latent(index, case):
    from audioldm2_amd import ops
    B, key, C, F = case
    ring = Lp.ring_plan(key)
    phases = Ph.phases_of(index, ring)
    plan, tab, row = table_plan(ring, phases)
    x, _ = Wd.window_inputs(B, ring, C, F)
    x = x.cuda()
    out, buf = A.guarded((ring.W * B, C, ring.Tw, F), fill=NAN)
    for phi in phases:
        out.fill_(NAN)
        got = ops.window_gather(x, plan, out=out, phase=tab, step_idx=counter(row[phi]))
        ref = Ph.gather_ref(x, ring, phi)
        assert got is out and torch.equal(bits(out), bits(ref)), f"phi={phi}"
        assert bool(torch.isnan(buf[:A.GUARD]).all()) and bool(torch.isnan(buf[-A.GUARD:]).all())
    # the ring launch on the rolled latent itself, the scalar path, the allocating form reading the plan's own table
    for phi in (phases[1], phases[-1]):
        ref = ops.window_gather(torch.roll(x, -phi, dims=2).contiguous(), ring)
        assert torch.equal(bits(ops.window_gather(x, plan, phase=tab, step_idx=counter(row[phi]))), bits(ref))
        assert torch.equal(bits(ops.window_gather(off_by_one_float(x), plan, phase=tab, step_idx=counter(row[phi]))), bits(ref))
        assert torch.equal(bits(ops.window_gather(x, plan, step_idx=counter(row[phi]))), bits(ref))
    # phi = 0 is the ring sibling, and the phase matters
    assert torch.equal(bits(ops.window_gather(x, plan, phase=tab, step_idx=counter(row[0]))), bits(ops.window_gather(x, ring)))
    assert not torch.equal(ops.window_gather(x, plan, phase=tab, step_idx=counter(row[1])), ops.window_gather(x, ring))


# ---- 2. the merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [None, 2], ids=["H1", "H2"])
@pytest.mark.parametrize("index,case", CASES)
def test_phased_merge_is_bitwise_the_rolled_ring_merge_and_matches_fp64(index, case, H):
    from audioldm2_amd import ops
    B, key, C, F = case
    ring = Lp.ring_plan(key)
    phases = Ph.phases_of(index, ring)
    plan, tab, row = table_plan(ring, phases)
    _, win = Wd.window_inputs(B, ring, C, F, H=H, seed=1)
    win = win.cuda()
    ring_out = ops.window_merge(win, ring)
    ref64, den = Lp.ring_merge_fp64(win, ring)[:2]
    bar = Wd.bar(ring)
    out, buf = A.guarded(((2,) if H == 2 else ()) + (B, C, ring.T, F))
    worst = 0.0
    for phi in phases:
        got = ops.window_merge(win, plan, out=out, phase=tab, step_idx=counter(row[phi]))
        assert got is out and A.guards_intact(buf)
        assert torch.equal(bits(out), bits(torch.roll(ring_out, phi, dims=-2))), f"phi={phi}"
        r, d = torch.roll(ref64, phi, dims=-2), torch.roll(den, phi, dims=-2)
        worst = max(worst, float(((out.double() - r).abs() / d).max()))
        assert bool(((out.double() - r).abs() <= bar * d).all()), f"phi={phi}"
    print(f"window_merge_ring_phased {case_id(case)} H={H} cover={ring.cover}, {len(phases)} phases: max |err| / sum |wn e| = "
          f"{worst:.3e}  bar {bar:.3e}")
    log_err(worst, bar, f"window_merge_ring_phased {case_id(case)}")
    phi = phases[-1]
    assert torch.equal(bits(ops.window_merge(off_by_one_float(win), plan, phase=tab, step_idx=counter(row[phi]))),
                       bits(torch.roll(ring_out, phi, dims=-2)))
    assert torch.equal(bits(ops.window_merge(win, plan, step_idx=counter(row[phi]))), bits(torch.roll(ring_out, phi, dims=-2)))
    assert torch.equal(bits(ops.window_merge(win, plan, phase=tab, step_idx=counter(row[0]))), bits(ring_out))


# ---- 3. the blend-gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", CASES)
def test_phased_blend_gather_leaves_the_ring_blend_and_gathers_the_rolled_result(index, case):
    from audioldm2_amd import ops
    B, key, C, F = case
    ring = Lp.ring_plan(key)
    phases = Ph.phases_of(index, ring)
    plan, tab, row = table_plan(ring, phases)
    x, x0, qn, coef = Ls.blend_inputs(B, ring, C, F, S=1)
    x, x0d, qnd, coefd = x.cuda(), x0.cuda(), qn.cuda()[0].contiguous(), coef.cuda()[0].contiguous()
    m = (Wd.window_inputs(B, ring, C, F, seed=9)[0] > 0).float()
    m[:, :, -3:] = 1.0
    m[:, :, :2] = 1.0
    masks = {"across the junction": m.cuda(), "quarter": torch.full(x.shape, 0.25).cuda()}
    xg, xbuf = A.guarded(tuple(x.shape))
    win, wbuf = A.guarded((ring.W * B, C, ring.Tw, F), fill=NAN)
    for name, md in masks.items():
        ref_x = x.clone()
        ops.inpaint_blend(ref_x, x0d, qnd, md, coefd)
        xr, xrbuf = A.guarded(tuple(x.shape))
        xr.copy_(x)
        ops.window_blend_gather(xr, x0d, qnd, md, coefd, ring)                   # the ring sibling: what it leaves in x
        assert torch.equal(bits(xr), bits(ref_x))
        for phi in phases if name == "across the junction" else phases[:3]:
            xg.copy_(x)
            win.fill_(NAN)
            # q_rows == coef_rows == 1: the counter selects the phase row alone
            got = ops.window_blend_gather(xg, x0d, qnd, md, coefd, plan, step_idx=counter(row[phi]), out=win, phase=tab)
            assert got is win
            assert torch.equal(bits(xg), bits(xr)), f"{name} phi={phi}: x differs from what the ring sibling leaves"
            assert torch.equal(bits(win), bits(Ph.gather_ref(ref_x, ring, phi))), f"{name} phi={phi}: win"
            assert not bool(torch.isnan(win).any()) and A.guards_intact(xbuf)
            assert bool(torch.isnan(wbuf[:A.GUARD]).all()) and bool(torch.isnan(wbuf[-A.GUARD:]).all())
    # the tables' rows and the phase row follow ONE counter: three q-noise and coefficient rows, three phases
    S = 3
    _, _, qn3, coef3 = Ls.blend_inputs(B, ring, C, F, S=S)
    qn3, coef3 = qn3.cuda(), coef3.cuda()
    three = [phases[-1], phases[1], phases[2]]
    p3 = Ph.phased(ring, three)
    md = masks["across the junction"]
    for idx, r in ((0, 0), (1, 1), (2, 2), (S + 2, S - 1), (None, 0)):
        ref_x = x.clone()
        ops.inpaint_blend(ref_x, x0d, qn3[r].contiguous(), md, coef3[r].contiguous())
        xg.copy_(x)
        w = ops.window_blend_gather(xg, x0d, qn3, md, coef3, p3, step_idx=None if idx is None else counter(idx))
        assert torch.equal(bits(xg), bits(ref_x)) and torch.equal(bits(w), bits(Ph.gather_ref(ref_x, ring, three[r]))), f"counter {idx}"
    # the scalar path
    xu = off_by_one_float(x)
    w = ops.window_blend_gather(xu, x0d, qn3, md, coef3, p3, step_idx=counter(1))
    ref_x = x.clone()
    ops.inpaint_blend(ref_x, x0d, qn3[1].contiguous(), md, coef3[1].contiguous())
    assert torch.equal(bits(xu), bits(ref_x)) and torch.equal(bits(w), bits(Ph.gather_ref(ref_x, ring, three[1])))


# ---- 4. row selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [Ph.KERNEL_CASES[0], Ph.KERNEL_CASES[2]], ids=case_id)
def test_the_counter_selects_the_row_and_clamps_and_is_not_written(case):
    from audioldm2_amd import ops
    B, key, C, F = case
    ring = Lp.ring_plan(key)
    table = [3, ring.T - 1, 1, 5, 2]
    rows = len(table)
    plan, tab, _ = table_plan(ring, table)
    x, win = Wd.window_inputs(B, ring, C, F, H=2, seed=2)
    x, win = x.cuda(), win.cuda()
    x0, qn, md = torch.randn_like(x), torch.randn_like(x), (torch.rand_like(x) > 0.5).float()
    coef = torch.tensor([0.8, 0.6], device="cuda")
    ring_out = ops.window_merge(win, ring)
    for idx, r in ((-1, 0), (0, 0), (2, 2), (rows - 1, rows - 1), (rows + 3, rows - 1), (None, 0)):
        phi = table[r]
        c = None if idx is None else counter(idx)
        assert torch.equal(bits(ops.window_gather(x, plan, phase=tab, step_idx=c)), bits(Ph.gather_ref(x, ring, phi))), f"gather {idx}"
        assert torch.equal(bits(ops.window_merge(win, plan, phase=tab, step_idx=c)), bits(torch.roll(ring_out, phi, dims=-2))), idx
        xg, ref_x = x.clone(), x.clone()
        ops.inpaint_blend(ref_x, x0, qn, md, coef)
        w = ops.window_blend_gather(xg, x0, qn, md, coef, plan, step_idx=c, phase=tab)
        assert torch.equal(bits(xg), bits(ref_x)) and torch.equal(bits(w), bits(Ph.gather_ref(ref_x, ring, phi))), f"blend {idx}"
        if c is not None:
            assert int(c) == idx                                        # read, never written
    assert tab.cpu().tolist() == table
    # the wrappers' refusals
    with pytest.raises(RuntimeError, match="carries no phase"):
        ops.window_gather(x, ring, phase=tab)
    with pytest.raises(RuntimeError, match="int32"):
        ops.window_gather(x, plan, phase=tab.long())
    with pytest.raises(RuntimeError, match="int32"):
        ops.window_merge(win, plan, phase=tab.cpu())
    with pytest.raises(RuntimeError, match="step_idx"):
        ops.window_gather(x, plan, phase=tab, step_idx=torch.zeros(1, device="cuda"))


# ---- 5. table values just outside [0, T) ------------------------------------------------------------------------------------------------
def fenced(t, margin, fill=FILL):
    """`t` as a view into an allocation with `margin` sentinel elements on each side -> (view, buffer)."""
    n = t.numel()
    buf = torch.full((n + 2 * margin,), fill, device="cuda", dtype=t.dtype)
    v = buf[margin:margin + n].view(t.shape)
    v.copy_(t)
    return v, buf


def fence_intact(buf, margin, fill=FILL):
    return bool((buf[:margin] == fill).all()) and bool((buf[-margin:] == fill).all())


@pytest.mark.parametrize("case", [Ph.KERNEL_CASES[0], Ph.KERNEL_CASES[2]], ids=case_id)
def test_table_values_just_outside_the_range_clamp_inside_fenced_buffers(case):
    """-3, T and T + 3 behave as 0, T - 1 and T - 1.  Every operand lies inside an allocation of the test's with two planes (T*F
    floats) and more of sentinel on each side, so even a kernel without the clamp would stay in memory the test owns."""
    from audioldm2_amd import ops
    B, key, C, F = case
    ring = Lp.ring_plan(key)
    T = ring.T
    margin = 2 * T * F + (-(2 * T * F) % 4) + 64          # two planes, a multiple of 4 floats: 16-byte alignment is kept
    assert margin % 4 == 0 and margin >= 2 * T * F
    x, win = Wd.window_inputs(B, ring, C, F, H=2, seed=6)
    x0, qn = torch.randn(x.shape), torch.randn(x.shape)
    md = (torch.rand(x.shape) > 0.5).float()
    ops_in = {n: fenced(t.cuda(), margin) for n, t in (("x", x), ("win", win), ("x0", x0), ("qn", qn), ("mask", md))}
    wn, wnbuf = fenced(ring.wn.cuda(), margin)
    coef, cbuf = fenced(torch.tensor([0.8, 0.6]), margin)
    out_of_range, clamped = [-3, T, T + 3], [0, T - 1, T - 1]
    tab, tbuf = fenced(torch.tensor(out_of_range, dtype=torch.int32), 64, fill=0)
    plan = Ph.phased(ring, clamped)          # the plan's own table is not read: `phase=` is
    plan.__dict__.setdefault("_wn_dev", {})[str(wn.device)] = wn          # the merge reads the fenced copy of the weights
    want = Ph.phased(ring, clamped)
    xw, xwbuf = fenced(torch.empty(ring.W * B, C, ring.Tw, F), margin)
    out, obuf = fenced(torch.empty(2, B, C, T, F), margin)
    xg, xgbuf = fenced(torch.empty(x.shape), margin)
    bw, bwbuf = fenced(torch.empty(ring.W * B, C, ring.Tw, F), margin)
    xv, wv, x0v, qnv, mv = (ops_in[n][0] for n in ("x", "win", "x0", "qn", "mask"))
    for r, phi in enumerate(clamped):
        c = counter(r)
        ops.window_gather(xv, plan, out=xw, phase=tab, step_idx=c)
        assert torch.equal(bits(xw), bits(ops.window_gather(xv, want, step_idx=c))), f"gather {out_of_range[r]}"
        assert torch.equal(bits(xw), bits(Ph.gather_ref(xv, ring, phi)))
        ops.window_merge(wv, plan, out=out, phase=tab, step_idx=c)
        assert torch.equal(bits(out), bits(ops.window_merge(wv, want, step_idx=c))), f"merge {out_of_range[r]}"
        xg.copy_(xv)
        ref_x = xv.clone()
        ops.inpaint_blend(ref_x, x0v, qnv, mv, coef)
        ops.window_blend_gather(xg, x0v, qnv, mv, coef, plan, step_idx=c, out=bw, phase=tab)
        assert torch.equal(bits(xg), bits(ref_x)) and torch.equal(bits(bw), bits(Ph.gather_ref(ref_x, ring, phi))), out_of_range[r]
    for name, (_, buf) in ops_in.items():
        assert fence_intact(buf, margin), name
    for name, buf in (("wn", wnbuf), ("coef", cbuf), ("gather out", xwbuf), ("merge out", obuf), ("blend x", xgbuf), ("blend win", bwbuf)):
        assert fence_intact(buf, margin), name
    assert fence_intact(tbuf, 64, fill=0) and tab.cpu().tolist() == out_of_range


# ---- 6. NaN containment -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 16])
def test_a_nan_at_a_rotated_wrapped_position_reaches_its_frame_and_no_other(F):
    from audioldm2_amd import ops
    B, C, phi = 2, 3, 7
    ring = Lp.ring_plan((40, 16, 10))
    plan = Ph.phased(ring, [2, phi])
    idx = counter(1)
    _, win = Wd.window_inputs(B, ring, C, F, H=2, seed=4)
    win = win.cuda()
    h, j, b, c, p = 1, 3, 1, 2, 13                       # window 3 starts at 30 + 7: p = 13 is frame 50 - 40 = 10
    frame = (ring.starts[j] + phi + p) % ring.T
    assert ring.starts[j] + phi + p >= ring.T and frame == 10
    win[h, j * B + b, c, p] = NAN
    out, buf = A.guarded((2, B, C, ring.T, F))
    ops.window_merge(win, plan, out=out, step_idx=idx)
    want = torch.zeros_like(out, dtype=torch.bool)
    want[h, b, c, frame] = True
    assert torch.equal(torch.isnan(out), want) and A.guards_intact(buf)
    # the whole window: exactly the frames it covers under this phase, on both sides of the junction
    win[h, j * B + b, c] = NAN
    ops.window_merge(win, plan, out=out, step_idx=idx)
    for q in range(ring.Tw):
        want[h, b, c, (ring.starts[j] + phi + q) % ring.T] = True
    assert torch.equal(torch.isnan(out), want) and int(want.sum()) == ring.Tw * F
    # ... and the gather carries a NaN frame into exactly the window positions that cover it
    x, _ = Wd.window_inputs(B, ring, C, F, seed=5)
    x = x.cuda()
    x[b, c, frame] = NAN
    xw = ops.window_gather(x, plan, step_idx=idx)
    wantw = torch.zeros_like(xw, dtype=torch.bool)
    for jj, s in enumerate(ring.starts):
        q = (frame - s - phi) % ring.T
        if q < ring.Tw:
            wantw[jj * B + b, c, q] = True
    assert torch.equal(torch.isnan(xw), wantw) and int(wantw.sum()) == 2 * F


# ---- 7. the samplers on the tiny UNet -------------------------------------------------------------------------------------------------
LONG_KEY, STEPS, LONG_SHAPE, SEED = Ph.LONG_KEY, Ph.STEPS, Ph.LONG_SHAPE, 7
SAMPLERS = ["ddim", "plms", "dpmpp_2m"]


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


def golden_plan():
    from audioldm2_amd.windows import phase_table, with_phase
    ring = Lp.ring_plan(LONG_KEY)
    tab = phase_table(ring, STEPS, "golden")
    assert tab.tolist() == Ph.GOLDEN_6
    return with_phase(ring, tab), ring


def source(shape=LONG_SHAPE, keep=Ls.KEEP):
    from audioldm2_amd.windows import keep_mask
    return torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda(), keep_mask(shape[2], keep)


def close_to_its_loop(out, ref, what):
    e, bar = A.rel_rms(out, ref), A.tstart_bar(STEPS)
    print(f"{what}, phases {Ph.GOLDEN_6} vs the composition loop (roll, RingModel, roll back): {e:.2e}  bar {bar:.1e}")
    assert tuple(out.shape) == LONG_SHAPE and bool(torch.isfinite(out).all())
    assert log_err(e, bar, f"phased {what}") <= bar


@pytest.mark.parametrize("name", SAMPLERS)
def test_sampler_under_moving_phases_equals_the_composition_loop(tiny, name):
    m, cond, uncond = tiny
    plan, ring = golden_plan()
    out = run(name, tiny, plan)
    torch.manual_seed(SEED)
    ref = Ph.sampler_loop(name, m, ring, Ph.GOLDEN_6, x_long(), cond, uncond, STEPS, A.GS)
    close_to_its_loop(out, ref, f"{name} ring={LONG_KEY}")
    assert torch.equal(run(name, tiny, golden_plan()[0]), out)                     # a second run is bitwise the first
    d = A.rel_rms(out, run(name, tiny, ring))
    print(f"{name}: moving phases vs the fixed ring: rel rms {d:.2e}")
    assert d > 1e-3


@pytest.mark.parametrize("name", SAMPLERS)
def test_sampler_under_moving_phases_with_a_source_equals_the_loop_with_the_blend(tiny, name):
    from audioldm2_amd.windows import with_source
    m, cond, uncond = tiny
    plan, ring = golden_plan()
    x0, mask = source()
    mask4 = mask.view(1, 1, -1, 1).expand(LONG_SHAPE).contiguous()
    out = run(name, tiny, with_source(plan, x0, mask))
    torch.manual_seed(SEED)
    ref = Ph.source_loop(name, m, ring, Ph.GOLDEN_6, x_long(), x0, mask4, cond, uncond, STEPS, A.GS)
    close_to_its_loop(out, ref, f"{name} ring={LONG_KEY} keep={Ls.KEEP}")
    assert torch.equal(run(name, tiny, with_source(golden_plan()[0], x0, mask)), out)
    d = A.rel_rms(out, run(name, tiny, with_source(ring, x0, mask)))
    print(f"{name} with a source: moving phases vs the fixed ring: rel rms {d:.2e}")
    assert d > 1e-3


def test_ddim_under_moving_phases_with_guidance_rescale_resample_and_graded_levels(tiny):
    import resample as Rs
    from audioldm2_amd.windows import window_plan, with_source
    m, cond, uncond = tiny
    plan, ring = golden_plan()
    x0, mask = source()
    mask4 = mask.view(1, 1, -1, 1).expand(LONG_SHAPE).contiguous()
    # guidance rescale
    out = run("ddim", tiny, plan, guidance_rescale=0.7)
    torch.manual_seed(SEED)
    close_to_its_loop(out, Ph.sampler_loop("ddim", m, ring, Ph.GOLDEN_6, x_long(), cond, uncond, STEPS, A.GS, guidance_rescale=0.7),
                      "ddim guidance_rescale=0.7")
    assert A.rel_rms(out, run("ddim", tiny, ring, guidance_rescale=0.7)) > 1e-3
    # resample=(2, 2): the phase follows the loop position of a visit
    resample = (2, 2)
    visits = Rs.published_visits(STEPS, *resample)
    assert Rs.show(visits) == Rs.VISIT_TABLE[(STEPS,) + resample]
    out = run("ddim", tiny, with_source(plan, x0, mask), resample=resample)
    torch.manual_seed(SEED)
    close_to_its_loop(out, Ph.resample_loop(m, ring, Ph.GOLDEN_6, x_long(), x0, mask4, cond, uncond, STEPS, resample, A.GS),
                      f"ddim resample={resample}, {len(visits)} visits")
    assert A.rel_rms(out, run("ddim", tiny, with_source(ring, x0, mask), resample=resample)) > 1e-3
    # a graded level map
    levels = Gd.long_levels(window_plan(*LONG_KEY), ring=True)
    out = run("ddim", tiny, with_source(plan, x0, levels, graded=True))
    torch.manual_seed(SEED)
    close_to_its_loop(out, Ph.graded_loop(m, ring, Ph.GOLDEN_6, x_long(), x0, Gd.level4(levels, LONG_SHAPE), cond, uncond, STEPS, A.GS),
                      "ddim graded levels")
    assert A.rel_rms(out, run("ddim", tiny, with_source(ring, x0, levels, graded=True))) > 1e-3


def test_a_wrong_table_length_is_refused_before_the_first_draw(tiny):
    ring = Lp.ring_plan(LONG_KEY)
    for name in SAMPLERS:
        torch.manual_seed(SEED)
        state = torch.get_rng_state()
        with pytest.raises(ValueError, match="phase table has 5 entries, the run 6"):
            m, cond, uncond = tiny
            sampler_class(name)(m).sample(STEPS, LONG_SHAPE[0], LONG_SHAPE[1:], cond, eta=0.0, windows=Ph.phased(ring, [0] * 5),
                                          t_start=STEPS, verbose=False, unconditional_guidance_scale=A.GS,
                                          unconditional_conditioning=uncond)
        assert torch.equal(torch.get_rng_state(), state)


# ---- 8. a constant table ----------------------------------------------------------------------------------------------------------------
def test_a_constant_phase_is_the_ring_run_of_the_rolled_start(tiny):
    """phi = 7 at every step — no multiple of the gap of 10: run(x_T) = roll(run_ring(roll(x_T, -7)), +7).  Gather and merge are
    bitwise the ring's on the rolled problem and the step kernels are elementwise, so the measured value is expected to be 0."""
    c = 7
    ring = Lp.ring_plan(LONG_KEY)
    x_T = x_long()
    out = run("ddim", tiny, Ph.phased(ring, [c] * STEPS), x_T=x_T)
    ref = torch.roll(run("ddim", tiny, ring, x_T=torch.roll(x_T, -c, dims=2).contiguous()), c, dims=2)
    e, bar = A.rel_rms(out, ref), A.tstart_bar(STEPS)
    print(f"constant phase {c}: run(x_T) vs roll(run_ring(roll(x_T, -{c})), +{c}): rel rms {e:.2e}  bar {bar:.1e}")
    assert log_err(e, bar, "phased constant table") <= bar
    assert A.rel_rms(out, run("ddim", tiny, ring, x_T=x_T)) > 1e-3


# ---- 9. one cached graph for two tables -------------------------------------------------------------------------------------------------
E2E_T, E2E_HOP, E2E_STEPS, E2E_SEED, E2E_TEXT = 384, 128, 4, 42, "rain on a tin roof"
E2E_GOLDEN = [0, 79, 30, 109]


@pytest.fixture(scope="module")
def ld():
    from audioldm2_amd.pipeline import build_model
    torch.manual_seed(0)
    m = build_model(model_name="audioldm_16k_crossattn_t5")
    assert m.latent_t_size == 256
    return m.cuda()


def conditioning(ld):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    cond = ld.get_learned_conditioning_dict(make_batch_for_text_to_audio(E2E_TEXT))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    return cond, uncond


def test_two_tables_of_one_length_share_the_cached_step_graph(ld):
    from audioldm2_amd.windows import plan_key
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    C, F_ = ld.channels, ld.latent_f_size
    ring, _ = ld.long_form_plans(E2E_T, E2E_HOP, ring=True)
    cond, uncond = conditioning(ld)
    x_T = torch.randn((1, C, E2E_T, F_), generator=torch.Generator().manual_seed(7))
    tables = [E2E_GOLDEN, [5, 200, 131, 64]]

    def job(table):
        plan = Ph.phased(ring, table)
        out, _ = ld.sample_log(cond=cond, batch_size=1, x_T=x_T, ddim=True, ddim_steps=E2E_STEPS, eta=0.0,
                               unconditional_guidance_scale=A.GS, unconditional_conditioning=uncond, windows=plan)
        return out.clone(), plan
    first, p1 = job(tables[0])
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and plan_key(ent["win"].plan) == plan_key(p1) == (E2E_T, 256, ring.starts, "phased")
    assert ent["win"].phase.cpu().tolist() == tables[0] and ent["win"].step_idx is ent["step_idx"]
    second, p2 = job(tables[1])
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent          # the cached graph was taken
    assert ent["win"].phase.cpu().tolist() == tables[1]
    bar = latent_tol(E2E_STEPS)
    for table, out in zip(tables, (first, second)):
        ref = Ph.sampler_loop("ddim", ld, ring, table, x_T, cond, uncond, E2E_STEPS, A.GS, eta=0.0)
        e = A.rel_rms(out, ref)
        print(f"real UNet, phases {table} vs its own composition loop: {e:.2e}  bar {bar:.1e}")
        assert log_err(e, bar, f"phased real UNet {table}") <= bar
    d = A.rel_rms(second, first)
    print(f"... the second table vs the first: {d:.2e}")
    assert d > 1e-3
    assert torch.equal(job(tables[0])[0], first) and next(iter(unet._graph_cache.values())) is ent     # and back: bitwise the first
    unet.drop_step_caches()


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------------
def loop_job(ld, **kw):
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio, seed_everything
    seed_everything(E2E_SEED)
    ld.conditional_dry_run_finished = False      # every job as an object's first (pipeline._cfg_dropout_draw)
    wave = ld.generate_batch_long(make_batch_for_text_to_audio(E2E_TEXT), E2E_T, hop=E2E_HOP, ddim_steps=E2E_STEPS,
                                  unconditional_guidance_scale=A.GS, loop=True, **kw)
    return wave, ld.last_long_latent.clone(), ld.last_long_mel.clone(), float(torch.rand(1))


def test_generate_batch_long_loop_with_moving_phases_end_to_end(ld):
    from audioldm2_amd.pipeline import seed_everything, text_to_audio_long
    from audioldm2_amd.windows import phase_table
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    plan, mel_plan = ld.long_form_plans(E2E_T, E2E_HOP, ring=True)
    assert phase_table(plan, E2E_STEPS, "golden").tolist() == E2E_GOLDEN
    wave, latent, mel, rand_after = loop_job(ld, phase="golden")
    C, F_ = ld.channels, ld.latent_f_size
    voc = ld.first_stage_model.vocoder
    h = int(np.prod(voc.h.upsample_rates))
    assert tuple(latent.shape) == (1, C, E2E_T, F_) and tuple(mel.shape) == (1, 1, 4 * E2E_T, 64)
    assert wave.shape == (1, 1, E2E_T * 4 * h) and wave.dtype == np.float32 and np.isfinite(wave).all()
    # no draw was added: what a loop job — a linear job — draws
    assert rand_after == Wd.expected_rand_after_long(E2E_SEED, 1, (C, 256, F_), (C, E2E_T, F_), E2E_STEPS)
    # the replays ran under the table: the one cached graph's entry holds it, and the counter has walked it (aldm_step_advance
    # saturates at the last row)
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert ent["run_step"].graph is not None and ent["win"].phase.cpu().tolist() == E2E_GOLDEN
    assert int(ent["step_idx"]) == E2E_STEPS - 1 and ent["win"].step_idx is ent["step_idx"]

    # the latent: the composition loop — the job's draws by hand, DDIMSampler.decode over the rolled ring model
    seed_everything(E2E_SEED)
    torch.randn((1, C, 256, F_))
    cond, uncond = conditioning(ld)
    ref = Ph.sampler_loop("ddim", ld, plan, E2E_GOLDEN, torch.randn((1, C, E2E_T, F_)), cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"phased loop latent vs the composition loop: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "phased loop latent") <= latent_tol(E2E_STEPS)

    # the mel: the tail is UNROTATED — an fp64 ring merge of decode_first_stage on the fixed ring's windows of the job's own latent
    mel_ref = Lp.ring_merge_fp64(ld.decode_first_stage(Lp.ring_gather_ref(latent, plan)), mel_plan)[0]
    e = A.rel_rms(mel, mel_ref)
    print(f"phased loop mel vs the fp64 ring merge of the fixed windows' decodes: rel rms {e:.2e}  bar {mel_tol(E2E_STEPS):.1e}")
    assert log_err(e, mel_tol(E2E_STEPS), "phased loop mel") <= mel_tol(E2E_STEPS)

    # the junction: the wave is the middle period of the vocoder over three periods of the mel
    T_mel = mel.shape[-2]
    three = voc.forward_cl(torch.cat([mel[:, 0]] * 3, dim=1).float().contiguous())
    middle = three[..., T_mel * h:2 * T_mel * h].cpu().numpy()
    e = A.rms(wave - middle) / A.rms(middle)
    print(f"phased loop wave vs the middle period of the vocoder over three periods of the mel: rel rms {e:.2e}  bar {tail_tol():.1e}")
    assert log_err(e, tail_tol(), "phased loop junction") <= tail_tol()

    # the entry point: 15 s with 5 s of overlap, loop=True, phase="golden", is this very job
    ld.conditional_dry_run_finished = False
    wave3 = text_to_audio_long(ld, E2E_TEXT, duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS, guidance_scale=A.GS,
                               loop=True, phase="golden")
    assert np.array_equal(wave3, wave) and ld.latent_t_size == 256
    assert len(unet._graph_cache) == 1 and next(iter(unet._graph_cache.values())) is ent

    # phase = [0, 0, 0, 0] is the job without the keyword, bit for bit — and the golden job is another one
    wave0, latent0, _, rand0 = loop_job(ld, phase=[0] * E2E_STEPS)
    wave_plain, latent_plain, _, rand_plain = loop_job(ld)
    assert torch.equal(latent0, latent_plain) and np.array_equal(wave0, wave_plain) and rand0 == rand_plain == rand_after
    d = A.rel_rms(latent, latent_plain)
    print(f"phased loop latent vs the fixed ring's: rel rms {d:.2e}")
    assert d > 1e-3
    unet.drop_step_caches()


def source_audio(seconds=5):
    """A seeded synthetic recording at 16 kHz: two tones under a slow envelope, and a little noise."""
    rng = np.random.RandomState(0)
    t = np.arange(seconds * 16000) / 16000.0
    return ((np.sin(2 * np.pi * 220.0 * t) + 0.5 * np.sin(2 * np.pi * 1330.0 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
            + 0.05 * rng.randn(t.shape[0])).astype(np.float32)


def test_generate_batch_long_from_audio_loop_with_moving_phases(ld):
    from audioldm2_amd import extend_audio
    from audioldm2_amd.pipeline import keep_frames, seed_everything
    from audioldm2_amd.windows import keep_mask
    unet = ld.model.diffusion_model
    unet.drop_step_caches()
    ld.conditional_dry_run_finished = False
    table = [0, 100, 37, 250]
    wave = extend_audio(ld, E2E_TEXT, source_audio(), duration=15, overlap=5.0, seed=E2E_SEED, ddim_steps=E2E_STEPS,
                        guidance_scale=A.GS, loop=True, phase=table)
    latent, z, rand_after = ld.last_long_latent.clone(), ld.last_long_source.clone(), float(torch.rand(1))
    C, F_ = ld.channels, ld.latent_f_size
    h = int(np.prod(ld.first_stage_model.vocoder.h.upsample_rates))
    assert wave.shape == (1, 1, E2E_T * 4 * h) and wave.dtype == np.float32 and np.isfinite(wave).all()
    assert rand_after == Ls.expected_rand_after_source(E2E_SEED, 1, (C, E2E_T, F_), E2E_STEPS)          # the loop job's draws
    frames = keep_frames([(0.0, 5.0)], ld.latent_t_per_second, E2E_T)
    assert frames == [(0, 128)]
    mask4 = keep_mask(E2E_T, frames).view(1, 1, -1, 1).expand(1, C, E2E_T, F_).contiguous()
    plan, _ = ld.long_form_plans(E2E_T, E2E_HOP, ring=True)
    seed_everything(E2E_SEED)
    torch.randn((1, C, E2E_T, F_))
    cond, uncond = conditioning(ld)
    ref = Ph.source_loop("ddim", ld, plan, table, torch.randn((1, C, E2E_T, F_)), z, mask4, cond, uncond, E2E_STEPS, A.GS, eta=1.0)
    assert float(torch.rand(1)) == rand_after
    e = A.rel_rms(latent, ref)
    print(f"phased loop round a source, latent vs the ring loop with the blend: rel rms {e:.2e}  bar {latent_tol(E2E_STEPS):.1e}")
    assert log_err(e, latent_tol(E2E_STEPS), "phased loop source latent") <= latent_tol(E2E_STEPS)
    unet.drop_step_caches()
