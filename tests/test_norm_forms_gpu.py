"""Every launch form of GroupNorm, LayerNorm / RMSNorm and the row softmax (csrc/norm.hip) against fp64 on the same fp32 inputs.

GroupNorm: the cases of tests/norm_forms.py, each asserting through aldm_groupnorm_plan the form it is in the table for BEFORE it
launches (a changed threshold or a pinned $ALDM_GN_* then fails the test instead of moving it to another kernel), on three input
recipes — trend (partials of unequal count differ in mean), large mean, and one spiked element per sample at the positions where the
plan has an edge (chunk ends, the unroll tail, both sides of a pass boundary and of the x1 / x2 seam, the last column).  The GroupNorm
bars are asserted per (sample, group), which is never below the max-norm over the tensor.  Measured errors:
profiles/r13_norm_forms_errors.txt, summarised in tests/tolerances.py."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import norm_forms as nf
from tolerances import log_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The bars this project held for these ops before they were measured form by form — 1e-5 for the normalised GroupNorm output, 5e-5
# output / 1e-5 rstd at large mean, 5e-6 LayerNorm, 2e-6 RMSNorm (tests/test_t5.py), 1e-5 softmax — lowered, by the rule of
# tests/tolerances.py, to at most 5x the worst figure measured on an MI355X (profiles/r13_norm_forms_errors.txt, worst in brackets):
GN_OUT_BAR = {"trend": 1e-6, "spike": 1e-6, "mean1e2": 5e-6, "mean1e3": 5e-6}      # per (sample, group): (2.6e-7), (1.2e-6)
GN_RSTD_BAR = 1e-6                                                                # (2.8e-7)
GN_IMAGE_BAR = {"trend": 9e-7, "spike": 9e-7, "mean1e2": 2e-6, "mean1e3": 2e-6}    # exact 3-part image, max-norm: (1.8e-7), (5.0e-7)
GN_F16_NORM_ALLOWANCE = 5e-7   # of max|ref|, next to the fp16 image's own bound (1e-6 in tests/test_f16x3_gpu.py): (1.1e-7)
LN_BAR = 6e-7                  # (1.8e-7; 1.2e-7 on the $ALDM_LN_R instantiations)
RMS_BAR = 8e-7                 # (1.6e-7)
SOFTMAX_BAR = 9e-7             # (2.2e-7)
SPLIT_MODES = ("bf16x6", "bf16x3", "f16x3")
CHILD_TIMEOUT = 300   # seconds per child process (library load + a handful of launches)


def max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@functools.lru_cache(maxsize=3)
def _gn_data(idx, recipe, rep):
    """(x, gamma, beta, normalised fp64, rstd * gamma fp64) of one launch; shared by the tests of a case, never modified."""
    case = nf.GN_CASES[idx]
    x = nf.gn_input(case, recipe, rep, case.plan())
    ga, be = nf.gn_params(case.C)
    ref, rstd = nf.gn_reference(x, ga, be, case.G)
    return x, ga, be, ref, rstd


def _halves(case, x):
    if not case.C2:
        return x.cuda(), None
    return x[..., :case.C1].contiguous().cuda(), x[..., case.C1:].contiguous().cuda()


def _reps(case, recipe):
    return nf.spike_reps(case, case.plan()) if recipe == "spike" else 1


def _assert_form(case, want_split):
    pl = case.plan(want_split)
    assert pl["form"] == (case.split_form if want_split else case.form), (case.id, pl)
    assert (pl["groups_per_block"], pl["passes"], pl["active_threads"]) == (case.gpb, case.passes, case.active), (case.id, pl)


@pytest.mark.parametrize("recipe", nf.GN_RECIPES)
@pytest.mark.parametrize("idx", range(len(nf.GN_CASES)), ids=[c.id for c in nf.GN_CASES])
def test_groupnorm_stats_on_every_form(idx, recipe):
    """scale / shift of gn_stats against F.group_norm in fp64: the normalised tensor and scale against rstd * gamma, both per
    (sample, group).  The spike recipe launches once per set of B positions until every position of the plan was spiked.  (With the
    first value a thread saw as its pivot, the spike AT that value measured 9.8e-6 on B2-P40-C2048+0-G1 and 4.0e-6 on
    B1-P130-C640+640-G32; with the median of three, 1.1e-7 and 1.9e-7.)"""
    from audioldm2_amd import ops
    case = nf.GN_CASES[idx]
    _assert_form(case, False)
    for rep in range(_reps(case, recipe)):
        x, ga, be, ref, rstd = _gn_data(idx, recipe, rep)
        x1, x2 = _halves(case, x)
        sc, sh = ops.gn_stats(x1, ga.cuda(), be.cuda(), groups=case.G, eps=1e-5, x2=x2)
        sc, sh = sc.cpu().double(), sh.cpu().double()
        assert bool(torch.isfinite(sc).all() and torch.isfinite(sh).all())
        got = torch.addcmul(sh[:, None, :], x.double(), sc[:, None, :])
        e_out = log_err(nf.group_rel_err(got, ref, case.G), GN_OUT_BAR[recipe], f"gn_stats {case.form} {recipe} output, per group")
        log_err(max_rel(got, ref), GN_OUT_BAR[recipe], f"gn_stats {case.form} {recipe} output, max-norm")
        e_sc = log_err(nf.group_rel_err(sc, rstd, case.G), GN_RSTD_BAR, f"gn_stats {case.form} {recipe} rstd*gamma, per group")
        print(f"{case.id} {case.form} {recipe} rep {rep}: output {e_out:.2e} rstd {e_sc:.2e}")
        assert e_out < GN_OUT_BAR[recipe] and e_sc < GN_RSTD_BAR, (case.id, case.why, recipe, rep, e_out, e_sc)


_SPLIT_IDX = [i for i, c in enumerate(nf.GN_CASES) if c.split_form]


@pytest.mark.parametrize("mode", SPLIT_MODES)
@pytest.mark.parametrize("recipe", nf.GN_RECIPES)
@pytest.mark.parametrize("idx", _SPLIT_IDX, ids=[nf.GN_CASES[i].id for i in _SPLIT_IDX])
def test_groupnorm_split_on_every_form(idx, recipe, mode):
    """gn_split: its image is the one gn_stats + split_rows write BIT FOR BIT and matches fp64 — an exact 3-part image ("bf16x6")
    to GN_IMAGE_BAR, a 2-part one ("bf16x3") to that plus the 2^-17 of two roundings to nearest; the fp16 image of "f16x3" stays
    within the element-wise bound of tests/test_f16x3_gpu.py test_images_are_fp16_pairs_of_scaled_values (2^-20 relative + 2^-24 /
    scale + the normalisation's own fp32 rounding).  Until the pivot of gn_partial_kernel became a median of three, the spike at a
    thread's first value missed that bound: excess 5.4e-6 (G = 1, fused), 3.1e-6 and 1.5e-6 (chunked) of max|ref| against 1e-6."""
    from audioldm2_amd import ops
    case = nf.GN_CASES[idx]
    _assert_form(case, True)
    act = ops.ACT_SILU if idx % 2 == 0 else ops.ACT_NONE
    prev = ops.set_mma(mode)
    try:
        for rep in range(_reps(case, recipe)):
            x, ga, be, ref, _ = _gn_data(idx, recipe, rep)
            if act == ops.ACT_SILU:
                ref = torch.nn.functional.silu(ref)
            x1, x2 = _halves(case, x)
            gac, bec = ga.cuda(), be.cuda()
            s_new, r_new = ops.gn_split(x1, gac, bec, groups=case.G, eps=1e-5, x2=x2, act=act, want_raw=True)
            assert r_new.fmt == "bf16"
            if mode == "f16x3":
                assert s_new.fmt == "f16" and s_new.parts == 2 and r_new.parts == 3
                assert torch.equal(r_new.float().cpu(), x)
                bound = math.sqrt((case.C // case.G) * case.P) * float(ga.abs().max()) + float(be.abs().max())
                assert math.log2(s_new.scale) == int(math.log2(s_new.scale)) and 16384.0 < s_new.scale * bound <= 32768.0
                err = (s_new.float().double().cpu() - ref).abs()
                image = ref.abs() * 2.0 ** -20 + 2.0 ** -24 / s_new.scale
                # (what the normalisation itself, fp32, needs next to the image's own rounding)
                need = log_err(float(((err - image).clamp_min(0.0)).max() / ref.abs().max()), GN_F16_NORM_ALLOWANCE,
                               f"gn_split f16 image {case.split_form} {recipe}: excess over the image bound / max|ref|")
                print(f"{case.id} {case.split_form} {recipe} f16x3 rep {rep}: excess {need:.2e}")
                assert bool((err <= image + GN_F16_NORM_ALLOWANCE * ref.abs().max()).all()), (case.id, recipe, rep, need)
                continue
            sc, sh = ops.gn_stats(x1, gac, bec, groups=case.G, eps=1e-5, x2=x2)
            s_old, r_old = ops.split_rows(x1, x2, pre=(sc, sh), act=act, want_raw=True)
            assert s_new.parts == (3 if mode == "bf16x6" else 2)
            assert torch.equal(s_new.data, s_old.data) and torch.equal(r_new.data, r_old.data), (case.id, recipe, rep)
            if mode == "bf16x6":
                assert torch.equal(r_new.float().cpu(), x)
            bar = GN_IMAGE_BAR[recipe] + (0.0 if mode == "bf16x6" else 2.0 ** -17)
            e = log_err(max_rel(s_new.float(), ref), bar, f"gn_split {case.split_form} {recipe} image vs fp64")
            print(f"{case.id} {case.split_form} {recipe} {mode} rep {rep}: image {e:.2e}")
            assert e < bar, (case.id, case.why, recipe, mode, rep, e)
    finally:
        ops.set_mma(prev)


def _child(code, env_extra, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, ALDM_FORMS_DIR=str(tmp_path), **env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("CASE")]


_GN_OVERRIDE_CHILD = r"""
import sys, torch
sys.path.insert(0, "tests")
import norm_forms as nf
from audioldm2_amd import ops
for B, P, C in nf.GN_OVERRIDE_SHAPES:
    case = nf.GnCase(B, P, C, 0, 32, None, None, None, None, None, "")
    pl, ps = case.plan(), case.plan(True)
    x = nf.gn_input(case, "trend")
    ga, be = nf.gn_params(C)
    ref, rstd = nf.gn_reference(x, ga, be, 32)
    xc, gac, bec = x.cuda(), ga.cuda(), be.cuda()
    sc, sh = ops.gn_stats(xc, gac, bec, groups=32, eps=1e-5)
    got = torch.addcmul(sh.cpu().double()[:, None, :], x.double(), sc.cpu().double()[:, None, :])
    s_new = ops.gn_split(xc, gac, bec, groups=32, eps=1e-5, act=ops.ACT_SILU)
    s_old = ops.split_rows(xc, None, pre=(sc, sh), act=ops.ACT_SILU)
    print("CASE", B, P, C, pl["form"], ps["form"], nf.group_rel_err(got, ref, 32), nf.group_rel_err(sc.cpu(), rstd, 32),
          int(torch.equal(s_new.data, s_old.data)))
"""


def test_groupnorm_fused_max_override_runs_large_slabs_fused(tmp_path):
    """$ALDM_GN_FUSED_MAX is read once per process: a fresh one with the value used until round 6 runs the level-1 slabs on the fused
    form (the plan says so there; by the rule they are chunked, tests/test_norm_forms_cpu.py) — 1024 trips of the pixel loop per
    thread, which no default-rule case reaches."""
    lines = _child(_GN_OVERRIDE_CHILD, {"ALDM_GN_FUSED_MAX": str(nf.GN_OVERRIDE_FUSED_MAX), "ALDM_MMA": "bf16x6"}, tmp_path)
    assert len(lines) == len(nf.GN_OVERRIDE_SHAPES)
    for (B, P, C, form, split_form, e_out, e_sc, bitwise), want_split in zip(lines, ("fused_split", "fused")):
        assert (form, split_form) == ("fused", want_split), (B, P, C, form, split_form)
        log_err(float(e_out), GN_OUT_BAR["trend"], "gn_stats fused under ALDM_GN_FUSED_MAX trend output, per group")
        log_err(float(e_sc), GN_RSTD_BAR, "gn_stats fused under ALDM_GN_FUSED_MAX trend rstd*gamma, per group")
        assert float(e_out) < GN_OUT_BAR["trend"] and float(e_sc) < GN_RSTD_BAR and bitwise == "1", (B, P, C, e_out, e_sc, bitwise)


# ---- LayerNorm / RMSNorm -----------------------------------------------------------------------------------------------------
def _ln_ref(x, ga, be, eps=1e-5):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), ga.double(), be.double(), eps)


@pytest.mark.parametrize("C", nf.LN_C)
def test_layernorm_and_rmsnorm_at_ragged_shapes(C):
    from audioldm2_amd import ops
    ga, be = nf.ln_params(C)
    for M in nf.LN_M:
        x = nf.ln_input(M, C)
        y = ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), 1e-5)
        e = log_err(max_rel(y, _ln_ref(x, ga, be)), LN_BAR, "layernorm ragged vs fp64")
        xd = x.double()
        rms_ref = ga.double() * xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-6)
        e_rms = log_err(max_rel(ops.rmsnorm(x.cuda(), ga.cuda(), 1e-6), rms_ref), RMS_BAR, "rmsnorm ragged vs fp64")
        print(f"layernorm M={M} C={C}: {e:.2e}  rmsnorm {e_rms:.2e}")
        assert e < LN_BAR and e_rms < RMS_BAR, (M, C, e, e_rms)


@pytest.mark.parametrize("mode", SPLIT_MODES)
@pytest.mark.parametrize("C", [C for C in nf.LN_C if C % 32 == 0])
def test_layernorm_split_images_equal_the_fp32_output_of_the_same_launch(C, mode):
    """split_out="also": the fp32 output is the plain launch's bit for bit; the 3-part image equals it bitwise, the 2-part one to
    2^-17 relative, the fp16 one within the bound of tests/test_f16x3_gpu.py (2^-21 relative + 2^-24 / scale)."""
    from audioldm2_amd import ops
    ga, be = nf.ln_params(C)
    prev = ops.set_mma(mode)
    try:
        for M in nf.LN_M:
            x = nf.ln_input(M, C).cuda()
            y0 = ops.layernorm(x, ga.cuda(), be.cuda(), 1e-5)
            y, so = ops.layernorm(x, ga.cuda(), be.cuda(), 1e-5, split_out="also")
            only = ops.layernorm(x, ga.cuda(), be.cuda(), 1e-5, split_out="only")
            assert torch.equal(y, y0) and torch.equal(only.data, so.data), (M, C)
            yd = y.double()
            d = (so.float().double() - yd).abs()
            if mode == "bf16x6":
                assert so.fmt == "bf16" and so.parts == 3 and torch.equal(so.float(), y), (M, C)
            elif mode == "bf16x3":
                assert so.fmt == "bf16" and so.parts == 2 and bool((d <= yd.abs() * 2.0 ** -17 + 1e-38).all()), (M, C)
            else:
                assert so.fmt == "f16" and so.parts == 2
                bound = math.sqrt(C) * float(ga.abs().max()) + float(be.abs().max())
                assert 16384.0 < so.scale * bound <= 32768.0
                assert bool((d <= yd.abs() * 2.0 ** -21 + 2.0 ** -24 / so.scale).all()), (M, C)
    finally:
        ops.set_mma(prev)


def test_layernorm_large_mean_against_the_fp32_yardstick():
    """mean / std = 100: with the exact two-pass form the mean is rounded to fp32 at 100 (2^-24 x 100 = 6e-6 of the spread) and
    so are the inputs' differences from it — fp32 itself cannot hold 5e-6 of max|ref| here.  The yardstick is torch's own fp32
    F.layer_norm on the CPU against fp64 on the same input; the bar the larger of 5e-6 and three times that figure."""
    from audioldm2_amd import ops
    M, C = 9, 768     # two rows per wave, odd row count
    x = torch.randn(M, C, generator=nf.gen(1)) + 100.0
    ga, be = nf.ln_params(C)
    ref = _ln_ref(x, ga, be)
    yard = max_rel(torch.nn.functional.layer_norm(x, (C,), ga, be, 1e-5), ref)
    bar = max(LN_BAR, 3.0 * yard)
    e = log_err(max_rel(ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), 1e-5), ref), bar, "layernorm mean/std = 100 vs fp64")
    log_err(yard, bar, "torch fp32 F.layer_norm on the CPU, mean/std = 100, vs fp64 (yardstick)")
    print(f"layernorm large mean: kernel {e:.2e}, torch fp32 on the CPU {yard:.2e}, bar {bar:.2e}")
    assert e < bar, (e, yard, bar)


_LN_R_CHILD = r"""
import os, sys, torch
sys.path.insert(0, "tests")
import norm_forms as nf
from audioldm2_amd import ops
default = torch.load(os.path.join(os.environ["ALDM_FORMS_DIR"], "ln_default.pt"))
for C in nf.LN_ENV_C:
    ga, be = nf.ln_params(C)
    for M in nf.LN_ENV_M:
        x = nf.ln_input(M, C)
        y = ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), 1e-5).cpu()
        ref = torch.nn.functional.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
        d = default[(M, C)]
        print("CASE", M, C, float((y.double() - ref).abs().max() / ref.abs().max()), int(torch.equal(y, d)),
              float((y.double() - d.double()).abs().max()))
"""


@pytest.mark.parametrize("R", nf.LN_ENV_R)
def test_layernorm_rows_per_wave_selected_by_env_agree_with_the_default(R, tmp_path):
    """$ALDM_LN_R (read once per process) selects the 2- / 4-rows-per-wave instantiations for C <= 512, which are compiled and shipped
    but never the default: a fresh process per value, M = 1, 7, 9 (fewer rows than a wave holds; a wave whose last rows are the clamped
    duplicate).  Against fp64 to the LayerNorm bar; and equal to the default's output bit for bit — rows are independent and every
    instantiation evaluates a row with the same operations in the same order (no contraction, no fast-math)."""
    from audioldm2_amd import ops
    assert "ALDM_LN_R" not in os.environ, "ALDM_LN_R pins the instantiation: unset it"
    default = {}
    for C in nf.LN_ENV_C:
        ga, be = nf.ln_params(C)
        for M in nf.LN_ENV_M:
            default[(M, C)] = ops.layernorm(nf.ln_input(M, C).cuda(), ga.cuda(), be.cuda(), 1e-5).cpu()
    torch.save(default, tmp_path / "ln_default.pt")
    lines = _child(_LN_R_CHILD, {"ALDM_LN_R": str(R)}, tmp_path)
    assert len(lines) == len(nf.LN_ENV_C) * len(nf.LN_ENV_M)
    for M, C, e, bitwise, diff in lines:
        log_err(float(e), LN_BAR, f"layernorm ALDM_LN_R={R} vs fp64")
        assert float(e) < LN_BAR and bitwise == "1", (R, M, C, e, diff)


# ---- row softmax -------------------------------------------------------------------------------------------------------------
def _softmax_ref(scores, allowed):
    """fp64 softmax over the allowed keys, excluded keys at weight exactly 0 (every row keeps a key)."""
    return torch.softmax(scores.masked_fill(~allowed, -math.inf), -1)


@pytest.mark.parametrize("kind", ["plain", "masked", "biased"])
@pytest.mark.parametrize("N", nf.SOFTMAX_N)
def test_softmax_rows_at_every_row_length(N, kind):
    from audioldm2_amd import ops
    B, heads, q_rows, scale = 2, 2, 3, 0.7
    x = torch.randn(B, heads, q_rows, N, generator=nf.gen(1)) * 3
    j = torch.arange(N)
    if kind == "plain":
        got = ops.softmax_rows(x.cuda(), scale).cpu()
        e = log_err(max_rel(got, torch.softmax(x.double() * scale, -1)), SOFTMAX_BAR, "softmax_rows plain vs fp64")
        assert e < SOFTMAX_BAR, (N, e)
        return
    km = (torch.rand(B, N, generator=nf.gen(2)) > 0.3).float()
    if kind == "masked":
        km[:, 0] = 1.0                                   # the start token is never masked
        for q_pos0 in sorted({0, max(N - q_rows, 0)}):   # the first row sees exactly one key; the last row sees every key
            allowed = (km[:, None, None, :] != 0) & (j[None, None, None, :] <= q_pos0 + torch.arange(q_rows)[None, None, :, None])
            allowed = allowed.expand(B, heads, q_rows, N)
            got = ops.softmax_rows_masked(x.cuda(), km.cuda(), q_pos0, scale).cpu()
            assert bool((got[~allowed] == 0).all()), (N, q_pos0)
            if q_pos0 == 0:
                assert bool((got[:, :, 0, 0] == 1.0).all())
            e = log_err(max_rel(got, _softmax_ref(x.double() * scale, allowed)), SOFTMAX_BAR, "softmax_rows masked vs fp64")
            assert e < SOFTMAX_BAR, (N, q_pos0, e)
        return
    bias = torch.randn(heads, q_rows, N, generator=nf.gen(3))
    km = torch.ones(B, N)
    for b in range(B):                                   # a padded tail per sample (none at N = 1)
        km[b, N - N // (b + 2):] = 0.0
    allowed = (km[:, None, None, :] != 0).expand(B, heads, q_rows, N)
    got = ops.softmax_rows_bias(x.cuda(), bias.cuda(), km.cuda(), scale).cpu()
    assert bool((got[~allowed] == 0).all()), N
    e = log_err(max_rel(got, _softmax_ref(x.double() * scale + bias.double()[None], allowed)), SOFTMAX_BAR, "softmax_rows biased vs fp64")
    assert e < SOFTMAX_BAR, (N, e)


def test_softmax_rows_refuses_a_row_beyond_the_lds_stage():
    from audioldm2_amd import ops
    x = torch.zeros(1, nf.SOFTMAX_N_REFUSED).cuda()
    with pytest.raises(RuntimeError, match=nf.SOFTMAX_REFUSAL):
        ops.softmax_rows(x)
