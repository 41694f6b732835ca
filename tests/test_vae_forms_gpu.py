"""The VAE's launch forms (audioldm2_amd/vae.py), one by one, against plain torch in fp64 on the same fp32 inputs, in every mode.

The whole-model fixture test (tests/test_model_gpu.py test_vae_matches_reference_fixture: about a hundred launches under tail_tol =
4e-5, default mode only) cannot see a wrong epilogue branch, a tap leaking across the seam between two samples or one lost partial
product in one launch.  Here every launch of a block is asserted on its own, against fp64 of ITS OWN inputs (the references are the
restatements of tests/vae_forms.py, which tests/test_vae_forms_cpu.py holds against oracle.vae), then the block as a whole:

  1. ResnetBlock.run, pre-split path: gn_split (eps 1e-6, SiLU, want_raw) -> the normalised image and the raw image; the 1x1
     nin_shortcut on the raw image; conv1 on the normalised image; the second gn_split; conv2 with res = the skip the other GEMM wrote.
     Register-staged path (set_dma(False), and the only one in "f32"): gn_stats + the SiLU prologue of the consuming conv.
     The 3x3 convs of the pre-split path run on the planner's choice, on a forced non-halo tile and on a forced halo form;
  2. "f16x3" at the real slab: C = 128, P = 262144 (n = 2^20), the fp16 image, its scale, and a 1x1 conv from it;
  3. AttnBlock.run: the qkv projection, gemm_nt on the three column-slice views of the fused [B, L, 3C] buffer (row pitch 3C, alpha =
     C^-0.5; bitwise the result from contiguous copies), softmax_rows, pack_kn of the V slice + gemm_packed_batched (bitwise the
     result from a contiguous V), the out projection + residual; one gemm_nt / gemm_packed_batched pair at K >= LONG_K;
  4. _Down.run / 5. _Up.run on a split operand and unsplit;
  6. the end convs: Decoder.conv_out (N = 1, rows 4 bytes apart, the output only 4-byte aligned), Encoder.conv_out (N = 16 / 32),
     Decoder.conv_in (K = 72 / 144), Encoder.conv_in through Encoder.run's own zero-padding of the single channel (K = 36);
  7. one reduced VAE end to end, pre-split and register-staged, against the fp64 oracle, next to torch's own fp32 evaluation of it.

Every igemm launch is asserted, through ops.TUNE_LOG / ops.PROFILE, to have run the kernel family the case is meant for (a DMA-fed
kernel on the forced tile / halo form and ring depth; a register-staged kernel where the operand is fp32); every conv output is a
view into a NaN-filled buffer whose guards must stay NaN and which must hold no NaN afterwards.  The checks can fail: with the
five-product test hook a conv and a 1x1 skip of the chain miss their bars, and a symmetric-padding downsample, a bilinear upsample
and q / k slices at pitch C are rejected as references.

Shapes: tests/vae_forms.py.  The forced halo form has shapes of its own: the halo-patch kernel runs whole 128-row tiles of one
image, which the other shapes are chosen NOT to be.  Bars: tests/tolerances.py and tests/test_norm_forms_gpu.py, unchanged;
measured figures in profiles/r14_vae_forms_errors.txt and the docstring of tests/tolerances.py."""
import contextlib
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import norm_forms as nf
import tuned_geometry as tg
import vae_forms as vf
from test_dma_gpu import _HALO, _TILES
from test_norm_forms_gpu import GN_F16_NORM_ALLOWANCE, GN_IMAGE_BAR, GN_OUT_BAR, SOFTMAX_BAR
from tolerances import LONG_K, act_act_long_k_tol, fused_tol, gemm_tol, log_err, tail_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096     # floats of NaN on each side of an output view
# forced forms of the 3x3 convs on split operands, by the parts of the operand image (3: "bf16x6", 2: "bf16x3" and the fp16 images):
# a 128-row tile (the planner's own choice at these sizes is a 64-row one) and a halo form that holds W = 16, 32 and 64
TILE = {3: (128, 128, 3), 2: (128, 128, 4)}
HALO = {3: (128, 128, 412), 2: (128, 128, 413)}
assert TILE[3] in _TILES["bf16x6"] and TILE[2] in _TILES["bf16x3"] and HALO[3] in _HALO["bf16x6"] and HALO[2] in _HALO["bf16x3"]
SPLIT_SUFFIX = (",dma", ",dma2")


@pytest.fixture(scope="module", params=vf.MODES)
def ops(request):
    from audioldm2_amd import ops as o
    prev = o.set_mma(request.param)
    prev_dma = o.DMA_MODE
    yield o
    o.set_dma(prev_dma)
    o.set_mma(prev)
    o.igemm_force(0, 0, 0)
    o.TUNE_LOG = o.PROFILE = None


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A fault of the device ends the run: nothing more is started on a GPU that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported a fault, stopping: {e}", returncode=3)


@contextlib.contextmanager
def dma(ops, on):
    prev = ops.set_dma(on)
    try:
        yield
    finally:
        ops.set_dma(prev)


@contextlib.contextmanager
def launches(ops, kinds, force=None):
    """The igemm launches issued inside, one entry of `kinds` each: 3 / 2 = a DMA-fed kernel over a pre-split image of that many parts,
    0 = a register-staged kernel over an fp32 operand.  `force` = (BM, BN, stages code) pins tile, ring depth / halo form and split-K
    1 for them (restored afterwards); each launch is asserted to have run exactly that."""
    ops.TUNE_LOG, ops.PROFILE = [], []
    try:
        if force is not None:
            ops.igemm_force(force[0], force[1], 1, 0, force[2])
        yield
        torch.cuda.synchronize()
        log, prof = ops.TUNE_LOG, ops.PROFILE
    finally:
        ops.igemm_force(0, 0, 0)
        ops.TUNE_LOG = ops.PROFILE = None
    assert len(log) == len(prof) == len(kinds), (kinds, log, [p[7] for p in prof])
    for key, parts, (_what, bm, bn, _fl, _e0, _e1, shape, name) in zip(log, kinds, prof):
        if parts:
            assert key.endswith(",dma" if parts == 3 else ",dma2"), (key, parts)
            assert shape[9] == 1 and shape[12] == parts, (key, shape)
            assert name.startswith("igemm_dma"), (key, name, "fell back to a register-staged kernel")
            if force is not None:
                assert (bm, bn, shape[8] // 10) == (force[0], force[1], 1), (key, force, (bm, bn, shape[8] // 10), name)
                assert tg.ran_dma_kernel(name) == tg.expected_dma_kernel(force[2]), (key, force, name)
        else:
            assert not key.endswith(SPLIT_SUFFIX) and shape[9] == 0 and name.startswith("igemm_kernel<"), (key, shape, name)


def nan_view(shape, offset=0):
    """A view of `shape` into a NaN-filled buffer, `offset` floats past the 16-byte aligned start behind the leading guard."""
    numel = math.prod(shape)
    big = torch.full((numel + 2 * GUARD + offset,), float("nan"), device="cuda", dtype=torch.float32)
    return (big, GUARD + offset, numel), big[GUARD + offset:GUARD + offset + numel].view(shape)


def assert_guarded(buf, what=""):
    big, lo, numel = buf
    bits = big.view(torch.int32)
    assert bool((bits[:lo] == tg.NAN_BITS).all()) and bool((bits[lo + numel:] == tg.NAN_BITS).all()), f"{what}: wrote outside its output"
    assert not bool(torch.isnan(big[lo:lo + numel]).any()), f"{what}: left part of its output unwritten (or wrote a NaN)"


def check(got, ref, bar, what):
    """Log, print, then assert max|got - ref| / max|ref| < bar (vae_forms.assert_close)."""
    from audioldm2_amd import ops
    e = log_err(vf.max_rel(got, ref), bar, what)
    print(f"{what} [{ops.MMA_MODE}]: {e:.3e} (bar {bar:.0e})")
    vf.assert_close(got, ref, bar, what)
    return e


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gpu_cl(x):
    return vf.cl(x).cuda()


def image_parts(ops, normalised):
    """Parts of the image a producer writes in this mode: the fp16 image of a normalised tensor has 2, a raw / GEMM-written one 3."""
    if ops.MMA_MODE == "bf16x3" or (normalised and ops.MMA_MODE == "f16x3"):
        return 2
    return 3


def check_image(ops, img, ref, gamma, beta, n, what):
    """A gn_split image against fp64 GroupNorm (+ SiLU) under the image bars of tests/test_norm_forms_gpu.py: an exact 3-part image
    under GN_IMAGE_BAR, a 2-part one under that + 2^-17, the fp16 image within its format model + GN_F16_NORM_ALLOWANCE of max|ref|
    — and carrying the scale _norm_f16_scale gives for n."""
    got = img.float().double().cpu()
    ref = ref.double()
    assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all()), what
    mode = ops.MMA_MODE
    if mode == "f16x3":
        assert img.fmt == "f16" and img.parts == 2
        assert img.scale == ops._norm_f16_scale(gamma, beta, n) == vf.f16_scale_rule(gamma, beta, n), (what, img.scale)
        err = (got - ref).abs()
        allowed = vf.f16_image_bound(ref, img.scale)
        need = log_err(float((err - allowed).clamp_min(0.0).max() / ref.abs().max()), GN_F16_NORM_ALLOWANCE,
                       f"{what}: fp16 image, excess over the format model / max|ref|")
        print(f"{what} [f16x3] n = {n}: excess {need:.2e} (bar {GN_F16_NORM_ALLOWANCE:.0e}), scale 2^{int(math.log2(img.scale))}")
        assert bool((err <= allowed + GN_F16_NORM_ALLOWANCE * ref.abs().max()).all()), (what, need)
        return need
    assert img.fmt == "bf16" and img.parts == (3 if mode == "bf16x6" else 2)
    bar = GN_IMAGE_BAR["trend"] + (0.0 if mode == "bf16x6" else 2.0 ** -17)
    return check(got, ref, bar, f"{what}: image vs fp64")


def check_raw(ops, raw, x, what):
    """The raw image: x bit for bit under a 3-part split ("bf16x6", "f16x3"), to 2^-17 relative under the 2-part one."""
    assert raw.fmt == "bf16"
    if ops.MMA_MODE == "bf16x3":
        assert raw.parts == 2
        d = (raw.float().double() - x.double()).abs()
        assert bool((d <= x.double().abs() * 2.0 ** -17 + 1e-38).all()), what
    else:
        assert raw.parts == 3 and torch.equal(raw.float(), x), f"{what}: the raw image must equal x exactly"


def check_stats(sc, sh, x_cl, ref_cl, what):
    """scale / shift of gn_stats: x * scale + shift against fp64 GroupNorm, per (sample, group), under GN_OUT_BAR."""
    Bx, C = sc.shape
    xd = x_cl.detach().double().cpu().view(Bx, -1, C)
    got = torch.addcmul(sh.double().cpu()[:, None, :], xd, sc.double().cpu()[:, None, :])
    e = log_err(nf.group_rel_err(got, ref_cl.reshape(Bx, -1, C), vf.GROUPS), GN_OUT_BAR["trend"], f"{what}: gn_stats output, per group")
    assert e < GN_OUT_BAR["trend"], (what, e)
    return e


def assert_plan(P, C, want_split, batch=vf.B):
    form = vf.plan(P, C, want_split, batch)["form"]
    assert form.startswith(vf.expected_form(P)), (P, C, want_split, form)


# ---- 1. the ResnetBlock chain ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def res_case(ci, co, H, W):
    """(state dict, x [B, C, H, W], fp64 restatement from x) of one block; computed once, shared by modes and paths, never modified."""
    from audioldm2_amd.vae import ResnetBlock
    sd = vf._module_state(ResnetBlock(in_channels=ci, out_channels=co), seed=ci + co)
    x = vf.feature_input(ci, H, W)
    return sd, x, vf.resnet_block(sd, x)


def res_block(ci, co, sd):
    from audioldm2_amd.vae import ResnetBlock
    blk = ResnetBlock(in_channels=ci, out_channels=co)
    blk.load_state_dict(sd, strict=True)
    return blk.cuda().eval()


def _conv3(x_nchw, sd, p):
    return vf.conv(x_nchw, sd, p, padding=1)


def run_res_presplit(ops, ci, co, H, W, force_of, tag):
    """The pre-split chain, launch by launch.  force_of(parts) -> the forced form of the 3x3 convs (None: the planner's choice)."""
    sd, x, ref = res_case(ci, co, H, W)
    blk = res_block(ci, co, sd)
    P = H * W
    xg = gpu_cl(x)
    with dma(ops, True):
        assert ops.use_dma()
        with launches(ops, ([image_parts(ops, False)] if ci != co else []) + [image_parts(ops, True)] * 2):
            whole = blk.run(xg)
    pk = blk._pk
    assert_plan(P, ci, True)
    assert_plan(P, co, True)
    # gn_split: the normalised image and the raw image
    if ci != co:
        a1, raw = ops.gn_split(xg, *pk["n1"], groups=32, eps=1e-6, act=ops.ACT_SILU, want_raw=True)
        check_raw(ops, raw, xg, f"resnet {tag}: raw image")
        sbuf, skip = nan_view((vf.B, H, W, co))
        with launches(ops, [raw.parts]):
            ops.conv(raw, pk["nin"], out=skip)
        assert_guarded(sbuf, "1x1 skip")
        check(vf.uncl(skip), ref["skip"], gemm_tol(), f"resnet {tag}: 1x1 skip on the raw image")
        skip_ref = vf.uncl(skip).double()
    else:
        a1 = ops.gn_split(xg, *pk["n1"], groups=32, eps=1e-6, act=ops.ACT_SILU)
        skip, skip_ref = xg, x.double()
    n_in = (ci // vf.GROUPS) * P
    check_image(ops, a1, vf.cl(ref["n1"]), *pk["n1"], n_in, f"resnet {tag}: gn_split 1")
    # conv1 on the normalised image
    hbuf, h = nan_view((vf.B, H, W, co))
    with launches(ops, [a1.parts], force_of(a1.parts)):
        ops.conv(a1, pk["c1"], pad=(1, 1), out=h)
    assert_guarded(hbuf, "conv1")
    hc = vf.uncl(h)
    check(hc, _conv3(vf.uncl(a1.float()), sd, "conv1"), gemm_tol(), f"resnet {tag}: conv1 vs fp64 of its image")
    check(hc, ref["h"], fused_tol(), f"resnet {tag}: conv1 vs fp64 GroupNorm + SiLU + conv")
    # the second gn_split, on the kernel's own h
    a2 = ops.gn_split(h, *pk["n2"], groups=32, eps=1e-6, act=ops.ACT_SILU)
    n2_ref = vf.gn(hc, sd, "norm2", True)
    check_image(ops, a2, vf.cl(n2_ref), *pk["n2"], (co // vf.GROUPS) * P, f"resnet {tag}: gn_split 2")
    # conv2 with the skip the other GEMM produced as its residual
    obuf, out = nan_view((vf.B, H, W, co))
    with launches(ops, [a2.parts], force_of(a2.parts)):
        ops.conv(a2, pk["c2"], pad=(1, 1), res=skip, out=out)
    assert_guarded(obuf, "conv2 + skip")
    oc = vf.uncl(out)
    check(oc, _conv3(vf.uncl(a2.float()), sd, "conv2") + skip_ref, gemm_tol(), f"resnet {tag}: conv2 + skip vs fp64 of its image")
    check(oc, _conv3(n2_ref, sd, "conv2") + skip_ref, fused_tol(), f"resnet {tag}: conv2 + skip vs fp64 GroupNorm + SiLU + conv")
    # the block as a whole
    check(vf.uncl(whole), ref["out"], fused_tol(), f"resnet {tag}: whole block (planner)")
    check(oc, ref["out"], fused_tol(), f"resnet {tag}: whole chain")
    if force_of(3) is None:
        assert same_bits(whole, out), "ResnetBlock.run must be the chain of these launches"


def run_res_staged(ops, ci, co, H, W):
    sd, x, ref = res_case(ci, co, H, W)
    blk = res_block(ci, co, sd)
    P = H * W
    xg = gpu_cl(x)
    with dma(ops, False):
        assert not ops.use_dma()
        with launches(ops, [0] * (2 + (ci != co))):
            whole = blk.run(xg)
    pk = blk._pk
    assert_plan(P, ci, False)
    assert_plan(P, co, False)
    sc, sh = ops.gn_stats(xg, *pk["n1"], groups=32, eps=1e-6)
    check_stats(sc, sh, xg, vf.cl(vf.gn(x, sd, "norm1")), "resnet staged: norm1")
    hbuf, h = nan_view((vf.B, H, W, co))
    with launches(ops, [0]):
        ops.conv(xg, pk["c1"], pad=(1, 1), pre=(sc, sh), pre_act=ops.ACT_SILU, out=h)
    assert_guarded(hbuf, "conv1")
    hc = vf.uncl(h)
    check(hc, ref["h"], fused_tol(), "resnet staged: conv1 behind the GroupNorm + SiLU prologue")
    sc2, sh2 = ops.gn_stats(h, *pk["n2"], groups=32, eps=1e-6)
    check_stats(sc2, sh2, h, vf.cl(vf.gn(hc, sd, "norm2")), "resnet staged: norm2")
    if ci != co:
        sbuf, skip = nan_view((vf.B, H, W, co))
        with launches(ops, [0]):
            ops.conv(xg, pk["nin"], out=skip)
        assert_guarded(sbuf, "1x1 skip")
        check(vf.uncl(skip), ref["skip"], gemm_tol(), "resnet staged: 1x1 skip")
        skip_ref = vf.uncl(skip).double()
    else:
        skip, skip_ref = xg, x.double()
    obuf, out = nan_view((vf.B, H, W, co))
    with launches(ops, [0]):
        ops.conv(h, pk["c2"], pad=(1, 1), pre=(sc2, sh2), pre_act=ops.ACT_SILU, res=skip, out=out)
    assert_guarded(obuf, "conv2 + skip")
    check(vf.uncl(out), _conv3(vf.gn(hc, sd, "norm2", True), sd, "conv2") + skip_ref, fused_tol(),
          "resnet staged: conv2 + skip behind the prologue")
    check(vf.uncl(whole), ref["out"], fused_tol(), "resnet staged: whole block")
    assert same_bits(whole, out), "ResnetBlock.run must be the chain of these launches"


def f32_has_no_presplit_path(ops, run, x):
    """"f32" has no pre-split path: with set_dma(True) the module still issues register-staged launches only, bitwise the
    set_dma(False) result."""
    assert ops.MMA_MODE == "f32"
    outs = []
    for on in (True, False):
        with dma(ops, on):
            assert not ops.use_dma()
            ops.TUNE_LOG = []
            try:
                outs.append(run(x))
                torch.cuda.synchronize()
                assert ops.TUNE_LOG and not any(k.endswith(SPLIT_SUFFIX) for k in ops.TUNE_LOG)
            finally:
                ops.TUNE_LOG = None
    assert same_bits(*outs)


RES_IDS = [f"{ci}to{co}-{h}x{w}" for ci, co, h, w in vf.RES_CASES]


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("ci,co,H,W", vf.RES_CASES, ids=RES_IDS)
def test_resnet_block_chain_launch_by_launch(ops, ci, co, H, W, path):
    if path == "staged":
        return run_res_staged(ops, ci, co, H, W)
    if ops.MMA_MODE == "f32":
        sd, x, _ = res_case(ci, co, H, W)
        return f32_has_no_presplit_path(ops, res_block(ci, co, sd).run, gpu_cl(x))
    if path == "tile":
        # (what the halo-patch kernel cannot run: forced onto these shapes it must refuse, not run something else)
        sd, x, _ = res_case(ci, co, H, W)
        a = ops.split_rows(gpu_cl(x))
        ops.igemm_force(HALO[a.parts][0], HALO[a.parts][1], 1, 0, HALO[a.parts][2])
        try:
            with pytest.raises(RuntimeError, match="halo-patch"):
                ops.conv(a, ops.pack_conv(sd["conv1.weight"], sd["conv1.bias"]), pad=(1, 1))
        finally:
            ops.igemm_force(0, 0, 0)
    run_res_presplit(ops, ci, co, H, W, (lambda parts: TILE[parts]) if path == "tile" else (lambda parts: None), path)


@pytest.mark.parametrize("ci,co,H,W", vf.RES_HALO_CASES, ids=[f"{ci}to{co}-{h}x{w}" for ci, co, h, w in vf.RES_HALO_CASES])
def test_resnet_block_chain_on_a_forced_halo_form(ops, ci, co, H, W):
    if ops.MMA_MODE == "f32":
        sd, x, _ = res_case(ci, co, H, W)
        return f32_has_no_presplit_path(ops, res_block(ci, co, sd).run, gpu_cl(x))
    run_res_presplit(ops, ci, co, H, W, lambda parts: HALO[parts], "halo")


# ---- the checks can fail: one lost partial product ------------------------------------------------------------------------------------
_FIVE_PRODUCT_CHILD = r"""
import sys, torch
sys.path.insert(0, {tests!r})
import vae_forms as vf
from audioldm2_amd import lib, ops
from audioldm2_amd.vae import ResnetBlock
assert lib.LIB_PATH.endswith("libaldm_hip_testhooks.so"), lib.LIB_PATH
ops.set_mma("bf16x6")
ci, co, (H, W) = 128, 256, vf.HW_FUSED
blk = ResnetBlock(in_channels=ci, out_channels=co)
sd = vf._module_state(blk, seed=ci + co)
blk.load_state_dict(sd, strict=True)
blk = blk.cuda().eval()
x = vf.feature_input(ci, H, W)
ref = vf.resnet_block(sd, x)
xg = vf.cl(x).cuda()
blk.run(xg)
pk = blk._pk
a1, raw = ops.gn_split(xg, *pk["n1"], groups=32, eps=1e-6, act=ops.ACT_SILU, want_raw=True)
ref_img = vf.conv(vf.uncl(a1.float()), sd, "conv1", padding=1)
ops.igemm_force(64, 128, 1, 0, 2)          # the one tile that has a five-product form
for drop in (False, True, False):
    ops.debug_drop_product(drop)
    skip = ops.conv(raw, pk["nin"])
    h = ops.conv(a1, pk["c1"], pad=(1, 1))
    print("RESULT", int(drop), vf.max_rel(vf.uncl(skip), ref["skip"]), vf.max_rel(vf.uncl(h), ref_img), vf.max_rel(vf.uncl(h), ref["h"]))
ops.igemm_force(0, 0, 0)
"""


def test_a_lost_partial_product_fails_the_bars_of_the_chain():
    """With ops.debug_drop_product(True) (the five-product hook of libaldm_hip_testhooks.so, a process of its own through
    $ALDM_LIB_PATH) the 1x1 skip and conv1 of the 128 -> 256 chain in "bf16x6" miss the bars they meet with six products: the skip
    gemm_tol, conv1 gemm_tol against fp64 of its image and fused_tol against fp64 from x."""
    from audioldm2_amd import lib
    assert os.path.exists(lib.TESTHOOKS_LIB_PATH), "build() also builds audioldm2_amd/libaldm_hip_testhooks.so"
    env = dict(os.environ, ALDM_LIB_PATH=lib.TESTHOOKS_LIB_PATH, PYTHONPATH=ROOT)
    env.pop("ALDM_ERR_LOG", None)
    out = subprocess.run([sys.executable, "-c", _FIVE_PRODUCT_CHILD.format(tests=os.path.join(ROOT, "tests"))], env=env,
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [[float(v) for v in l.split()[1:]] for l in out.stdout.splitlines() if l.startswith("RESULT")]
    assert [int(r[0]) for r in rows] == [0, 1, 0], out.stdout[-2000:]
    g, f = gemm_tol("bf16x6"), fused_tol("bf16x6")
    for drop, e_skip, e_img, e_chain in rows:
        print(f"five-product hook {'on' if drop else 'off'}: skip {e_skip:.2e} (bar {g:.0e}), conv1 vs its image {e_img:.2e} (bar {g:.0e}), "
              f"conv1 vs fp64 from x {e_chain:.2e} (bar {f:.0e})")
        if drop:
            assert e_skip > g and e_img > g and e_chain > f, "the bars must catch one lost partial product"
        else:
            assert e_skip < g and e_img < g and e_chain < f
    assert rows[0][1:] == rows[2][1:], "the switch must leave nothing behind"


# ---- 2. "f16x3" at the real slab --------------------------------------------------------------------------------------------------
def test_f16x3_image_and_conv_at_the_real_slab():
    """C = 128, P = 262144, one sample: n = (C / 32) P = 2^20, the last level of the 48 kHz decoder at 10 s — five bits more of n
    than any other f16x3 test, so sqrt(n) takes 2.5 more bits out of the fp16 image's scale.  One gn_split (SiLU) and one 1x1 conv
    from its image; the fp64 references are evaluated on the GPU with torch in double (the slab is 128 MiB)."""
    from audioldm2_amd import ops
    C, P = vf.F16_SLAB
    N = 128
    n = (C // vf.GROUPS) * P
    assert n == 1 << 20
    assert_plan(P, C, True, batch=1)
    prev = ops.set_mma("f16x3")
    prev_dma = ops.set_dma(True)
    try:
        g = torch.Generator(device="cuda").manual_seed(14)
        x = torch.randn(1, P, C, generator=g, device="cuda") * nf.GN_SPREAD + 0.5
        x += torch.randn(C, generator=g, device="cuda") * nf.GN_SPREAD
        x += (torch.linspace(-1.0, 1.0, P, device="cuda") * nf.GN_SPREAD * 2)[None, :, None]
        x *= (0.5 + 0.5 * (torch.arange(C, device="cuda") % 4).float()) / 8
        ga, be = (t.cuda() for t in nf.gn_params(C))
        w = torch.randn(N, C, generator=vf.gen(4)) / math.sqrt(C)
        b = torch.randn(N, generator=vf.gen(5))
        pw = ops.pack_conv(w, b)
        img = ops.gn_split(x, ga, be, groups=32, eps=1e-6, act=ops.ACT_SILU)
        assert img.fmt == "f16" and img.parts == 2
        assert img.scale == ops._norm_f16_scale(ga, be, n) == vf.f16_scale_rule(ga, be, n), img.scale
        ref = torch.nn.functional.group_norm(x.double().permute(0, 2, 1), vf.GROUPS, ga.double(), be.double(), vf.EPS).permute(0, 2, 1)
        ref = ref * torch.sigmoid(ref)
        got = img.float().double().view(1, P, C)
        assert bool(torch.isfinite(got).all())
        top = float(ref.abs().max())
        err = (got - ref).abs()
        allowed = vf.f16_image_bound(ref, img.scale)
        need = log_err(float((err - allowed).clamp_min(0.0).max()) / top, GN_F16_NORM_ALLOWANCE,
                       "f16x3 real slab: fp16 image, excess over the format model / max|ref|")
        e_img = log_err(float(err.max()) / top, 0.0, "f16x3 real slab: fp16 image vs fp64, max-norm")
        print(f"f16x3 image at n = 2^20: scale 2^{int(math.log2(img.scale))}, max|ref| {top:.3f}, error {e_img:.2e}, excess over the "
              f"format model {need:.2e} (bar {GN_F16_NORM_ALLOWANCE:.0e})")
        assert bool((err <= allowed + GN_F16_NORM_ALLOWANCE * top).all()), need
        del err, allowed, got
        obuf, out = nan_view((1, 1, P, N))
        with launches(ops, [2]):
            ops.conv(img.view(1, 1, P, C), pw, out=out)
        assert_guarded(obuf, "1x1 conv at the real slab")
        ref_out = ref.view(P, C) @ w.double().cuda().t() + b.double().cuda()
        check(out.view(P, N), ref_out, fused_tol("f16x3"), "f16x3 real slab: 1x1 conv from the fp16 image vs fp64 GroupNorm + SiLU + conv")
    finally:
        ops.set_dma(prev_dma)
        ops.set_mma(prev)


# ---- 3. AttnBlock ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attn_case(C, H, W):
    sd = vf.attn_state(C, seed=C)
    x = vf.feature_input(C, H, W)
    return sd, x, vf.attn_block(sd, x)


@pytest.mark.parametrize("path", ["presplit", "staged"])
@pytest.mark.parametrize("C,H,W", vf.ATTN_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in vf.ATTN_CASES])
def test_attn_block_launch_by_launch(ops, C, H, W, path):
    from audioldm2_amd.vae import AttnBlock
    sd, x, ref = attn_case(C, H, W)
    blk = AttnBlock(C)
    blk.load_state_dict(sd, strict=True)
    blk = blk.cuda().eval()
    xg = gpu_cl(x)
    L = H * W
    if path == "presplit" and ops.MMA_MODE == "f32":
        return f32_has_no_presplit_path(ops, blk.run, xg)
    on = path == "presplit"
    first = image_parts(ops, True) if on else 0
    with dma(ops, on):
        assert ops.use_dma() == on
        with launches(ops, [first, 0, 0, 0]):
            whole = blk.run(xg)
    pk = blk._pk
    # the qkv projection behind gn_split / behind the gn_stats prologue
    qbuf, qkv4 = nan_view((vf.B, H, W, 3 * C))
    if on:
        a = ops.gn_split(xg, *pk["n"], groups=32, eps=1e-6)
        check_image(ops, a, vf.cl(ref["n"]), *pk["n"], (C // vf.GROUPS) * L, "attn: gn_split")
        with launches(ops, [a.parts]):
            ops.conv(a, pk["qkv"], out=qkv4)
    else:
        sc, sh = ops.gn_stats(xg, *pk["n"], groups=32, eps=1e-6)
        check_stats(sc, sh, xg, vf.cl(ref["n"]), "attn staged: norm")
        with launches(ops, [0]):
            ops.conv(xg, pk["qkv"], pre=(sc, sh), out=qkv4)
    assert_guarded(qbuf, "qkv projection")
    qkv = qkv4.view(vf.B, L, 3 * C)
    check(qkv, ref["qkv"], fused_tol(), f"attn {path}: qkv projection behind the GroupNorm")
    # gemm_nt on the column slices exactly as AttnBlock.run passes them
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    assert q.stride() == (L * 3 * C, 3 * C, 1) and not k.is_contiguous()
    alpha = float(int(C) ** (-0.5))
    sbuf, scores = nan_view((vf.B, L, L))
    with launches(ops, [0]):
        ops.gemm_nt(q, k, alpha=alpha, out=scores)
    assert_guarded(sbuf, "gemm_nt")
    qkv_c = qkv.cpu()
    s_ref = vf.attn_scores(qkv_c[:, :, :C], qkv_c[:, :, C:2 * C], C)
    check(scores, s_ref, gemm_tol(), f"attn {path}: gemm_nt on column slices at pitch 3C")
    assert same_bits(scores, ops.gemm_nt(q.contiguous(), k.contiguous(), alpha=alpha)), "a strided view must give the contiguous result"
    with pytest.raises(AssertionError):   # the check can fail: q / k read at pitch C are another product
        vf.assert_close(scores, vf.attn_scores(*vf.slices_at_pitch_c(qkv_c, C), C), gemm_tol(), "gemm_nt vs slices at pitch C")
    # softmax_rows
    probs = ops.softmax_rows(scores, 1.0)
    sc_c = scores.cpu()
    check(probs, torch.softmax(sc_c.double(), -1), SOFTMAX_BAR, f"attn {path}: softmax_rows")
    # pack_kn of the V slice + gemm_packed_batched
    obuf, o = nan_view((vf.B, L, C))
    vp = ops.pack_kn(v)
    with launches(ops, [0]):
        ops.gemm_packed_batched(probs, vp, L, C, out=o)
    assert_guarded(obuf, "gemm_packed_batched")
    check(o, torch.bmm(probs.cpu().double(), qkv_c[:, :, 2 * C:].double()), gemm_tol(), f"attn {path}: pack_kn of the V slice + P V")
    vp_c = ops.pack_kn(v.contiguous())
    assert same_bits(vp, vp_c) and same_bits(o, ops.gemm_packed_batched(probs, vp_c, L, C)), "a strided V must give the contiguous result"
    # the out projection + residual
    rbuf, out = nan_view((vf.B, H, W, C))
    with launches(ops, [0]):
        ops.conv(o.view(vf.B, H, W, C), pk["out"], res=xg, out=out)
    assert_guarded(rbuf, "out projection")
    o_img = o.cpu().double().permute(0, 2, 1).reshape(vf.B, C, H, W)
    check(vf.uncl(out), x.double() + vf.conv(o_img, sd, "proj_out"), gemm_tol(), f"attn {path}: out projection + residual")
    # the block as a whole
    check(vf.uncl(whole), ref["out"], fused_tol(), f"attn {path}: whole block")
    assert same_bits(whole, out), "AttnBlock.run must be the chain of these launches"


@pytest.mark.parametrize("K", vf.ATTN_LONG_K)
def test_attention_products_at_long_k(ops, K):
    """One gemm_nt / gemm_packed_batched pair with a contraction of K >= LONG_K (3104 = 97 k-tiles of 32; 3100: a ragged last k-tile),
    Z = 1, M = 64, operands of non-zero mean, column slices of wider buffers: under act_act_long_k_tol, with torch's own fp32 bmm
    on the same operands logged next to the kernel."""
    assert K >= LONG_K
    M, N = 64, 112
    a = (torch.randn(1, M, K, generator=vf.gen(1)) + 0.3).cuda()
    bw = (torch.randn(1, N, 2 * K, generator=vf.gen(2)) + 0.3).cuda()
    bs = bw[:, :, K:]
    sbuf, s = nan_view((1, M, N))
    with launches(ops, [0]):
        ops.gemm_nt(a, bs, alpha=K ** -0.5, out=s)
    assert_guarded(sbuf, "gemm_nt, long K")
    ref = torch.bmm(a.double(), bs.double().transpose(1, 2)).cpu() * K ** -0.5
    yard = log_err(vf.max_rel(torch.bmm(a, bs.transpose(1, 2)) * K ** -0.5, ref), 0.0, "gemm_nt long K: torch fp32 bmm (yardstick)")
    e = check(s, ref, act_act_long_k_tol(), "gemm_nt long K")
    print(f"gemm_nt K = {K}: kernel {e:.2e}, torch fp32 bmm {yard:.2e}")
    assert same_bits(s, ops.gemm_nt(a, bs.contiguous(), alpha=K ** -0.5))
    Nv = 512
    pr = torch.softmax(torch.randn(1, M, K, generator=vf.gen(3)) * 2, -1).cuda()
    vw = (torch.randn(1, K, 3 * Nv, generator=vf.gen(4)) + 0.3).cuda()
    vs = vw[:, :, 2 * Nv:]
    obuf, o = nan_view((1, M, Nv))
    with launches(ops, [0]):
        ops.gemm_packed_batched(pr, ops.pack_kn(vs), K, Nv, out=o)
    assert_guarded(obuf, "gemm_packed_batched, long K")
    ref = torch.bmm(pr.double(), vs.double()).cpu()
    yard = log_err(vf.max_rel(torch.bmm(pr, vs), ref), 0.0, "gemm_packed_batched long K: torch fp32 bmm (yardstick)")
    e = check(o, ref, act_act_long_k_tol(), "gemm_packed_batched long K")
    print(f"gemm_packed_batched K = {K}: kernel {e:.2e}, torch fp32 bmm {yard:.2e}")


# ---- 4. / 5. Downsample and Upsample ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_case(kind, C, H, W):
    from audioldm2_amd.vae import _Down, _Up
    sd = vf._module_state((_Down if kind == "down" else _Up)(C), seed=C + H)
    x = vf.feature_input(C, H, W)
    right, wrong = (vf.downsample, vf.downsample_symmetric) if kind == "down" else (vf.upsample, vf.upsample_bilinear)
    return sd, x, right(sd, x), wrong(sd, x)


def run_resample(ops, kind, C, H, W, path):
    from audioldm2_amd.vae import _Down, _Up
    sd, x, ref, wrong = resample_case(kind, C, H, W)
    mod = (_Down if kind == "down" else _Up)(C)
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().eval()
    xg = gpu_cl(x)
    if path != "staged" and ops.MMA_MODE == "f32":
        return f32_has_no_presplit_path(ops, mod.run, xg)
    on = path != "staged"
    parts = image_parts(ops, False) if on else 0
    with dma(ops, on):
        assert ops.use_dma() == on
        with launches(ops, [parts]):
            whole = mod.run(xg)
    OH, OW = ((H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1) if kind == "down" else (2 * H, 2 * W)
    assert tuple(whole.shape) == (vf.B, OH, OW, C) == tuple(vf.cl(ref).shape)
    xin = xg
    if on:
        xin = ops.split_rows(xg)
        check_raw(ops, xin, xg, f"{kind}sample: split_rows")
    kw = dict(stride=(2, 2), pad=(0, 0), out_hw=(OH, OW)) if kind == "down" else dict(pad=(1, 1), up=(2, 2))
    force = TILE[parts] if path == "tile" else None
    if path == "tile":   # stride 2 / nearest x2 is outside the halo-patch kernel: forced, it must refuse
        ops.igemm_force(HALO[parts][0], HALO[parts][1], 1, 0, HALO[parts][2])
        try:
            with pytest.raises(RuntimeError, match="halo-patch"):
                ops.conv(xin, mod._pk, **kw)
        finally:
            ops.igemm_force(0, 0, 0)
    buf, out = nan_view((vf.B, OH, OW, C))
    with launches(ops, [parts], force):
        ops.conv(xin, mod._pk, out=out, **kw)
    assert_guarded(buf, f"{kind}sample conv")
    what = "F.pad (0, 1, 0, 1) + conv k3 s2 p0" if kind == "down" else "nearest x2 + conv k3 p1"
    check(vf.uncl(out), ref, gemm_tol(), f"{kind}sample {path}: {what}")
    check(vf.uncl(whole), ref, gemm_tol(), f"{kind}sample {path}: the module's run")
    if force is None:
        assert same_bits(whole, out)
    with pytest.raises(AssertionError):   # the check can fail: symmetric padding / bilinear x2 is another operation
        vf.assert_close(vf.uncl(out), wrong, gemm_tol(), f"{kind}sample vs the wrong reference")


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("C,H,W", vf.DOWN_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in vf.DOWN_CASES])
def test_downsample_with_the_asymmetric_pad(ops, C, H, W, path):
    run_resample(ops, "down", C, H, W, path)


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("C,H,W", vf.UP_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in vf.UP_CASES])
def test_upsample_nearest_x2(ops, C, H, W, path):
    run_resample(ops, "up", C, H, W, path)


# ---- 6. the end convs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def out_conv_case(C, N, H, W):
    x = vf.feature_input(C, H, W, seed=N)
    ga, be = nf.gn_params(C)
    sd = {"norm.weight": ga, "norm.bias": be, "conv.weight": (torch.rand(N, C, 3, 3, generator=vf.gen(N)) * 2 - 1) / math.sqrt(9 * C),
          "conv.bias": torch.randn(N, generator=vf.gen(N + 1)) * 0.05}
    return sd, x, vf.gn(x, sd, "norm"), vf.conv(vf.gn(x, sd, "norm", True), sd, "conv", padding=1)


@pytest.mark.parametrize("C,N,H,W", vf.CONV_OUT_CASES + vf.ENC_OUT_CASES, ids=lambda v: str(v))
def test_out_convs_behind_the_groupnorm_prologue(ops, C, N, H, W):
    """Decoder.conv_out / Encoder.conv_out: gn_stats + conv(pad 1, pre, SiLU).  N = 1: ldo = 1, every output row is 4 bytes; the output
    is a view ONE FLOAT past the aligned start of a NaN-guarded buffer, so its rows are 4-byte aligned only — a vector store or a
    column-tile store not masked per element would land in a neighbouring row or the guards.  Every row is compared with fp64."""
    sd, x, n_ref, ref = out_conv_case(C, N, H, W)
    xg = gpu_cl(x)
    ga, be = sd["norm.weight"].cuda(), sd["norm.bias"].cuda()
    pw = ops.pack_conv(sd["conv.weight"], sd["conv.bias"])
    assert_plan(H * W, C, False)
    sc, sh = ops.gn_stats(xg, ga, be, groups=32, eps=1e-6)
    check_stats(sc, sh, xg, vf.cl(n_ref), f"conv_out N = {N}: norm_out")
    buf, out = nan_view((vf.B, H, W, N), offset=1 if N == 1 else 0)
    assert out.data_ptr() % 16 == (4 if N == 1 else 0)
    with launches(ops, [0]):
        ops.conv(xg, pw, pad=(1, 1), pre=(sc, sh), pre_act=ops.ACT_SILU, out=out)
    assert_guarded(buf, f"conv_out N = {N}")
    got = vf.uncl(out)
    check(got, ref, fused_tol(), f"conv_out N = {N}: conv behind GroupNorm + SiLU")
    rows_err = (got.double() - ref).abs().amax(1).reshape(-1)      # per output row (pixel): the largest error of its N values
    worst = int(rows_err.argmax())
    assert bool((rows_err < fused_tol() * ref.abs().max()).all()), (N, worst, float(rows_err[worst]))


@pytest.mark.parametrize("Cz,N,H,W", vf.DEC_IN_CASES, ids=lambda v: str(v))
def test_decoder_conv_in_from_the_latent_channels(ops, Cz, N, H, W):
    z = torch.randn(vf.B, Cz, H, W, generator=vf.gen(Cz)) + 0.3
    sd = {"conv.weight": (torch.rand(N, Cz, 3, 3, generator=vf.gen(N)) * 2 - 1) / math.sqrt(9 * Cz),
          "conv.bias": torch.randn(N, generator=vf.gen(N + 1)) * 0.05}
    pw = ops.pack_conv(sd["conv.weight"], sd["conv.bias"])
    assert pw.K == 9 * Cz
    buf, out = nan_view((vf.B, H, W, N))
    with launches(ops, [0]):
        ops.conv(gpu_cl(z), pw, pad=(1, 1), out=out)
    assert_guarded(buf, "Decoder.conv_in")
    check(vf.uncl(out), vf.conv(z, sd, "conv", padding=1), gemm_tol(), f"Decoder.conv_in {Cz} -> {N}")


def test_encoder_conv_in_through_the_encoders_own_padding(ops):
    """Encoder.run pads its 1-channel input to 4 channels (and the weight to match) so the 16-byte gather applies: K = 36.  The first
    launch of a one-level Encoder is taken out of the run (its arguments and its result) and held against conv2d of the 1-CHANNEL
    input in fp64."""
    from audioldm2_amd.vae import Encoder
    H, W = vf.ENC_IN_HW
    enc = Encoder(ch=128, out_ch=1, ch_mult=(1,), num_res_blocks=1, in_channels=1, resolution=256, z_channels=8)
    enc, sd = vf.load(enc, seed=9)
    x = torch.randn(vf.B, 1, H, W, generator=vf.gen(9)) * 2 - 4        # log-mel-like values
    calls = []
    real = ops.conv

    def spy(xx, pw, **kw):
        y = real(xx, pw, **kw)
        calls.append((xx, pw, kw, y))
        return y
    ops.conv = spy
    ops.TUNE_LOG = []
    try:
        enc.run(gpu_cl(x))
        torch.cuda.synchronize()
        first_key = ops.TUNE_LOG[0]
    finally:
        ops.conv = real
        ops.TUNE_LOG = None
    xx, pw, kw, y = calls[0]
    assert pw is enc._pk["cin"] and (pw.Cin, pw.K, pw.N) == (4, 36, 128) and kw == dict(pad=(1, 1))
    assert tuple(xx.shape) == (vf.B, H, W, 4) and torch.equal(xx[..., 0].cpu(), x[:, 0]) and not bool(xx[..., 1:].any())
    assert not first_key.endswith(SPLIT_SUFFIX) and tg.parse_key(first_key)[0]["C1"] == 4
    check(vf.uncl(y), vf.conv(x, sd, "conv_in", padding=1), gemm_tol(), "Encoder.conv_in from one channel")


# ---- 7. one reduced VAE end to end -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reduced_case():
    from oracle import vae as ovae
    dd = vf.DD_REDUCED
    sd = vf.vae_state(dd, seed=14)
    z = torch.randn(*vf.LATENT_REDUCED, generator=vf.gen(14))
    mel = vf.mel_for(dd, vf.LATENT_REDUCED, seed=14)
    sd64 = vf.double_state(sd)
    return dd, sd, z, mel, (ovae.vae_decode(sd64, dd, z.double()), ovae.vae_decode(sd, dd, z)), \
        (ovae.vae_encode_moments(sd64, dd, mel.double()), ovae.vae_encode_moments(sd, dd, mel))


def test_reduced_vae_end_to_end_against_the_fp64_oracle(ops):
    """ch = 128, ch_mult [1, 2, 4], z_channels 8: decode a (2, 8, 5, 16) latent, encode the matching (2, 1, 20, 64) mel, pre-split and
    register-staged, against oracle.vae in fp64 under tail_tol; torch's own fp32 evaluation of the oracle on the CPU is logged next
    to them (no bar: what fp32 arithmetic itself gives on this graph).  The launch log shows which path ran: every ResnetBlock conv,
    the qkv projections and the resampling convs over pre-split operands in the first run, none in the second."""
    from audioldm2_amd.vae import ResnetBlock, _Down, _Up
    dd, sd, z, mel, (dec_ref, dec32), (enc_ref, enc32) = reduced_case()
    ae = vf.vae_module(dd)
    ae.load_state_dict(sd, strict=True)
    ae = ae.cuda().eval()

    def presplit_launches(net):
        res = [m for m in net.modules() if isinstance(m, ResnetBlock)]
        return sum(2 + (m.in_channels != m.out_channels) for m in res) + 1 + sum(isinstance(m, (_Down, _Up)) for m in net.modules())
    mode = ops.MMA_MODE
    for name, net, run, ref, ref32 in (("decode", ae.decoder, lambda: ae.decode(z.cuda()), dec_ref, dec32),
                                       ("encode", ae.encoder, lambda: ae.encode(mel.cuda()).parameters, enc_ref, enc32)):
        errs = {}
        for on in (True, False):
            with dma(ops, on):
                ops.TUNE_LOG = []
                try:
                    got = run()
                    torch.cuda.synchronize()
                    log = ops.TUNE_LOG
                finally:
                    ops.TUNE_LOG = None
            n_split = sum(k.endswith(SPLIT_SUFFIX) for k in log)
            assert n_split == (presplit_launches(net) if (on and mode != "f32") else 0), (name, on, n_split, presplit_launches(net))
            what = f"reduced VAE {name}, " + ("pre-split" if on else "register-staged")
            errs[on] = check(got, ref, tail_tol(), what)
        e32 = log_err(vf.max_rel(ref32, ref), 0.0, f"reduced VAE {name}, torch fp32 on the CPU")
        print(f"reduced VAE {name} [{mode}] vs fp64 oracle: pre-split {errs[True]:.3e}, register-staged {errs[False]:.3e}, "
              f"torch fp32 {e32:.3e} (bar {tail_tol():.0e})")


def test_a_vae_of_64_channels_is_refused_not_run(ops):
    """ch = 64 puts two channels into each of the 32 groups; the GroupNorm kernels work on whole float4s of channels per group and
    refuse ((C / G) % 4 == 0) — in every mode, on both paths, for decode and encode, before anything is computed.  Until they take
    narrower groups the reduced VAE above stays at ch = 128; a library that runs ch = 64 fails here, and the case can move down."""
    dd = vf.DD_REFUSED
    ae = vf.vae_module(dd)
    ae.load_state_dict(vf.vae_state(dd, seed=14), strict=True)
    ae = ae.cuda().eval()
    z = torch.randn(*vf.LATENT_REDUCED, generator=vf.gen(14)).cuda()
    mel = vf.mel_for(dd, vf.LATENT_REDUCED, seed=14).cuda()
    for on in (True, False):
        with dma(ops, on):
            with pytest.raises(RuntimeError, match=vf.GN_REFUSAL):
                ae.decode(z)
            with pytest.raises(RuntimeError, match=vf.GN_REFUSAL):
                ae.encode(mel)
