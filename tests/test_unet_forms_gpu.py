"""The UNet's launch forms (audioldm2_amd/unet.py), one by one, against plain torch in fp64 on the same fp32 inputs, in every mode.

The whole-forward fixture tests put a few hundred launches under one max-norm (unet_tol); one lost partial product in one launch, a
wrong row-bias pitch on one ResBlock or a tap leaking across the sample seam at one level can pass them.  Here every launch of a
module is asserted on its own, against fp64 of ITS OWN inputs (the restatements of tests/unet_forms.py, which
tests/test_unet_forms_cpu.py holds against oracle.unet in double), then the module as a whole:

  1. ResBlock.run: gn_split (eps 1e-5, SiLU, the skip concat as x2, want_raw) -> the normalised and the raw image; the 1x1 skip on
     the raw concat image; conv1 + the timestep row bias (always a column-slice view of a wider [B, sum N] buffer at a non-zero
     offset; a contiguous copy must give the same bits); the second gn_split; conv2 + res.  Register-staged twin: gn_stats(x2=) +
     conv(x, x2=, pre=).  The 3x3 convs run on the planner's tile, a forced 128x128 tile and (shapes of its own) a forced halo form;
  2. Downsample (pad 1, stride 2) / Upsample, on split and unsplit operands;
  3. BasicTransformerBlock.run: each LayerNorm image, linear_qkv (q bitwise the plain projection's; K / V^T through the pre-split
     attention bitwise the fp32-K/V attention), attention against fp64 of its own q, k, v, out1 + res; cross-attention folded and
     unfolded on the AudioMAE context, unfolded on a masked T5 context (masked keys weigh exactly 0, an all-masked sample is uniform),
     attn2 as self-attention where no context is routed; GEGLU; ff2 + res;
  4. SpatialTransformer.run as a whole and its two ends (gn_split eps 1e-6 -> proj_in; proj_out from the "also" image);
  5. the embedding path (timestep_embedding, te0, te2, FiLM, emb_all at the real sums of widths, every ResBlock's slice);
  6. conv_in and the out conv;  7. two reduced UNets end to end next to torch's own fp32 evaluation.

Every igemm launch is asserted, through ops.TUNE_LOG / ops.PROFILE, to have run the kernel family the case is meant for; every
GEMM output that takes a buffer is a view into a NaN-filled one whose guards must stay NaN.  The checks can fail: with the
five-product test hook conv1 + row bias and the ff2 projection miss gemm_tol, and every wrong reference of tests/unet_forms.py is
rejected at the bar of its launch.  Bars: tests/tolerances.py and tests/test_norm_forms_gpu.py, unchanged, and one new one for the
timestep embedding (tolerances.timestep_embedding_tol: twice torch's own fp32 error of the same row); measured figures in
profiles/r25_unet_forms_errors.txt and the docstring of tests/tolerances.py."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import unet_forms as uf
from oracle import cases, weights
from oracle import unet as ounet
from test_norm_forms_gpu import LN_BAR
from test_vae_forms_gpu import (HALO, ROOT, SPLIT_SUFFIX, TILE, assert_guarded, check, check_image, check_raw, check_stats, dma,
                                f32_has_no_presplit_path, gpu_cl, image_parts, launches, nan_view, same_bits)
from test_vae_forms_gpu import _stop_after_a_gpu_fault, ops  # noqa: F401  (fixtures: the modes, and the stop after a device fault)
from test_dma_gpu import _HALO
from tolerances import fused_tol, gemm_tol, log_err, timestep_embedding_tol, unet_tol

pytestmark = pytest.mark.gpu

# the halo form that holds two- and four-column images (tests/test_dma_gpu.py test_dma_halo_image_widths) in both split widths
HALO_NARROW = (128, 128, 403)
assert all(HALO_NARROW in _HALO[m] for m in ("bf16x6", "bf16x3"))


def halo_for(W):
    return (lambda parts: HALO_NARROW) if W < 16 else (lambda parts: HALO[parts])


def kind(x):
    """What `launches` expects of a launch over operand x: the parts of a split image, 0 for an fp32 tensor."""
    return 0 if torch.is_tensor(x) else x.parts


def values(x):
    """The fp32 values a launch reads from operand x, on the CPU."""
    return (x if torch.is_tensor(x) else x.float()).detach().cpu()


def check_value_image(ops, img, y, what):
    """A split image a GEMM / attention / LayerNorm launch wrote next to its fp32 output y: 3 parts hold y bit for bit, 2 bf16 parts
    to 2^-17 relative, an fp16 image within its format model (vae_forms.f16_image_bound; it is rounded from the unrounded value, so
    one fp32 ulp more)."""
    got, yd = img.float().double().cpu(), y.detach().double().cpu()
    assert tuple(got.shape) == tuple(yd.shape), (what, got.shape, yd.shape)
    if img.fmt == "f16":
        assert img.parts == 2 and bool(((got - yd).abs() <= uf.f16_image_bound(yd, img.scale) + yd.abs() * 2.0 ** -23).all()), what
    elif img.parts == 3:
        assert torch.equal(img.float(), y), f"{what}: a 3-part image must equal the fp32 output exactly"
    else:
        assert bool(((got - yd).abs() <= yd.abs() * 2.0 ** -17 + 1e-38).all()), what


def rejected(got, wrong, bar, what):
    """The check can fail: `wrong` is a deliberately wrong reference, assert_close at the launch's bar must reject it."""
    with pytest.raises(AssertionError):
        uf.assert_close(got, wrong, bar, what)


def guarded_conv(ops, x, pw, shape, what, force=None, **kw):
    buf, out = nan_view(shape)
    with launches(ops, [kind(x)], force):
        r = ops.conv(x, pw, out=out, **kw)
    assert_guarded(buf, what)
    return r


def guarded_linear(ops, x, pw, shape, what, kinds=None, **kw):
    buf, out = nan_view(shape)
    with launches(ops, [kind(x)]):
        r = ops.linear(x, pw, out=out, **kw)
    assert_guarded(buf, what)
    if kinds is not None:
        kinds.append(kind(x))
    return r


# ---- 1. the ResBlock chain ---------------------------------------------------------------------------------------------------------
def res_block(case, sd):
    from audioldm2_amd.unet import ResBlock
    c1, c2, co = case[:3]
    return uf.load(ResBlock(c1 + c2, uf.EMB, 0, out_channels=co), sd)


def res_inputs(case):
    sd, x, x2, rows, sl, ref = uf.res_case(*case)
    rows_g = rows.cuda()
    e = rows_g[:, sl]
    assert e.data_ptr() != rows_g.data_ptr() and e.stride(0) == rows.shape[1] > e.shape[1] and not e.is_contiguous()
    return sd, x, x2, ref, gpu_cl(x), (None if x2 is None else gpu_cl(x2)), rows_g, sl, e


def run_res_presplit(ops, case, force_of, tag):
    """The pre-split chain, launch by launch.  force_of(parts) -> the forced form of the 3x3 convs (None: the planner's choice)."""
    c1, c2, co, H, W = case
    sd, x, x2, ref, xg, x2g, rows_g, sl, e = res_inputs(case)
    blk = res_block(case, sd)
    pk = blk._prepare()
    P, Cc = H * W, c1 + c2
    has_skip = pk["skip"] is not None
    assert has_skip == (Cc != co) and (c2 == 0 or has_skip)
    tag = f"resblock {c1}+{c2}->{co} {H}x{W} {tag}"
    with dma(ops, True):
        assert ops.use_dma()
        with launches(ops, ([image_parts(ops, False)] if has_skip else []) + [image_parts(ops, True)] * 2):
            whole = blk.run(xg, e, x2g)
        xc = xg if x2g is None else torch.cat([xg, x2g], -1)
        # gn_split: the normalised image and the raw image of the concat
        if has_skip:
            a1, raw = ops.gn_split(xg, *pk["gn1"], groups=32, eps=1e-5, x2=x2g, act=ops.ACT_SILU, want_raw=True)
            check_raw(ops, raw, xc, f"{tag}: raw image")
            skip = guarded_conv(ops, raw, pk["skip"], (uf.B, H, W, co), "1x1 skip")
            check(uf.uncl(skip), ref["skip"], gemm_tol(), f"{tag}: 1x1 skip on the raw image")
            skip_ref = uf.uncl(skip).double()
        else:
            a1 = ops.gn_split(xg, *pk["gn1"], groups=32, eps=1e-5, act=ops.ACT_SILU)
            skip, skip_ref = xg, x.double()
        check_image(ops, a1, uf.cl(ref["n1"]), *pk["gn1"], (Cc // uf.GROUPS) * P, f"{tag}: gn_split 1")
        if c2:   # the concat in the order [x2, x] is another tensor (c1 == c2: the same shapes, so only the values can tell)
            raw_w = uf.concat(x, x2, swapped=True)
            rejected(uf.uncl(a1.float()), uf.gn(raw_w, sd, "in_layers.0", uf.EPS, True), fused_tol(), "gn_split vs the swapped concat")
            rejected(uf.uncl(skip), uf.conv(raw_w, sd, "skip_connection"), gemm_tol(), "1x1 skip vs the swapped concat")
        # conv1 + the row bias, a column-slice view of the wide buffer
        force = force_of(a1.parts)
        h = guarded_conv(ops, a1, pk["conv1"], (uf.B, H, W, co), "conv1", force, pad=(1, 1), rowbias=e)
        hc = uf.uncl(h)
        img1 = uf.conv(uf.uncl(a1.float()), sd, "in_layers.2", padding=1)
        check(hc, img1 + ref["e"][:, :, None, None], gemm_tol(), f"{tag}: conv1 + row bias vs fp64 of its image")
        check(hc, ref["h"], fused_tol(), f"{tag}: conv1 + row bias vs fp64 GroupNorm + SiLU + conv")
        e_next = rows_g[:, uf.shifted(sl, co)].cpu().double()
        rejected(hc, img1 + e_next[:, :, None, None], gemm_tol(), "conv1 vs the next block's row bias")
        h_c = guarded_conv(ops, a1, pk["conv1"], (uf.B, H, W, co), "conv1, contiguous row bias", force, pad=(1, 1), rowbias=e.contiguous())
        assert same_bits(h, h_c), "a strided row-bias view must give the contiguous result"
        # the second gn_split, on the kernel's own h
        a2 = ops.gn_split(h, *pk["gn2"], groups=32, eps=1e-5, act=ops.ACT_SILU)
        n2_ref = uf.gn(hc, sd, "out_layers.0", uf.EPS, True)
        check_image(ops, a2, uf.cl(n2_ref), *pk["gn2"], (co // uf.GROUPS) * P, f"{tag}: gn_split 2")
        # conv2 with the skip as its residual
        out = guarded_conv(ops, a2, pk["conv2"], (uf.B, H, W, co), "conv2 + skip", force_of(a2.parts), pad=(1, 1), res=skip)
        oc = uf.uncl(out)
        check(oc, uf.conv(uf.uncl(a2.float()), sd, "out_layers.3", padding=1) + skip_ref, gemm_tol(), f"{tag}: conv2 + skip vs fp64 of its image")
        check(oc, uf.conv(n2_ref, sd, "out_layers.3", padding=1) + skip_ref, fused_tol(), f"{tag}: conv2 + skip vs fp64 GroupNorm + SiLU + conv")
    check(uf.uncl(whole), ref["out"], fused_tol(), f"{tag}: whole block (planner)")
    check(oc, ref["out"], fused_tol(), f"{tag}: whole chain")
    if force_of(3) is None:
        assert same_bits(whole, out), "ResBlock.run must be the chain of these launches"


def run_res_staged(ops, case):
    c1, c2, co, H, W = case
    sd, x, x2, ref, xg, x2g, rows_g, sl, e = res_inputs(case)
    blk = res_block(case, sd)
    pk = blk._prepare()
    has_skip = pk["skip"] is not None
    tag = f"resblock {c1}+{c2}->{co} {H}x{W} staged"
    with dma(ops, False):
        assert not ops.use_dma()
        with launches(ops, [0] * (2 + has_skip)):
            whole = blk.run(xg, e, x2g)
        xc = xg if x2g is None else torch.cat([xg, x2g], -1)
        sc, sh = ops.gn_stats(xg, *pk["gn1"], groups=32, eps=1e-5, x2=x2g)
        check_stats(sc, sh, xc, uf.cl(uf.gn(ref["raw"], sd, "in_layers.0", uf.EPS)), f"{tag}: norm 1")
        h = guarded_conv(ops, xg, pk["conv1"], (uf.B, H, W, co), "conv1", x2=x2g, pad=(1, 1), pre=(sc, sh), pre_act=ops.ACT_SILU, rowbias=e)
        hc = uf.uncl(h)
        check(hc, ref["h"], fused_tol(), f"{tag}: conv1 + row bias behind the GroupNorm + SiLU prologue")
        e_next = rows_g[:, uf.shifted(sl, co)].cpu().double()
        rejected(hc, ref["h"] - ref["e"][:, :, None, None] + e_next[:, :, None, None], fused_tol(), "conv1 vs the next block's row bias")
        h_c = ops.conv(xg, pk["conv1"], x2=x2g, pad=(1, 1), pre=(sc, sh), pre_act=ops.ACT_SILU, rowbias=e.contiguous())
        assert same_bits(h, h_c), "a strided row-bias view must give the contiguous result"
        if c2:
            wrong = uf.resblock(sd, x, None, x2, swapped=True, e=ref["e"])
            rejected(hc, wrong["h"], fused_tol(), "conv1 vs the swapped concat")
        sc2, sh2 = ops.gn_stats(h, *pk["gn2"], groups=32, eps=1e-5)
        check_stats(sc2, sh2, h, uf.cl(uf.gn(hc, sd, "out_layers.0", uf.EPS)), f"{tag}: norm 2")
        if has_skip:
            skip = guarded_conv(ops, xg, pk["skip"], (uf.B, H, W, co), "1x1 skip", x2=x2g)
            check(uf.uncl(skip), ref["skip"], gemm_tol(), f"{tag}: 1x1 skip on the concat")
            if c2:
                rejected(uf.uncl(skip), wrong["skip"], gemm_tol(), "1x1 skip vs the swapped concat")
            skip_ref = uf.uncl(skip).double()
        else:
            skip, skip_ref = xg, x.double()
        out = guarded_conv(ops, h, pk["conv2"], (uf.B, H, W, co), "conv2 + skip", pad=(1, 1), pre=(sc2, sh2), pre_act=ops.ACT_SILU, res=skip)
        check(uf.uncl(out), uf.conv(uf.gn(hc, sd, "out_layers.0", uf.EPS, True), sd, "out_layers.3", padding=1) + skip_ref, fused_tol(),
              f"{tag}: conv2 + skip behind the prologue")
    check(uf.uncl(whole), ref["out"], fused_tol(), f"{tag}: whole block")
    assert same_bits(whole, out), "ResBlock.run must be the chain of these launches"


def res_f32(ops, case):
    sd, x, x2, ref, xg, x2g, rows_g, sl, e = res_inputs(case)
    blk = res_block(case, sd)
    return f32_has_no_presplit_path(ops, lambda t: blk.run(t, e, x2g), xg)


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("case", uf.RES_CASES + uf.RES_CONCAT_CASES, ids=lambda c: "{}+{}to{}-{}x{}".format(*c))
def test_resblock_chain_launch_by_launch(ops, case, path):
    if path == "staged":
        return run_res_staged(ops, case)
    if ops.MMA_MODE == "f32":
        return res_f32(ops, case)
    run_res_presplit(ops, case, (lambda parts: TILE[parts]) if path == "tile" else (lambda parts: None), path)


@pytest.mark.parametrize("case", uf.RES_HALO_CASES, ids=lambda c: "{}+{}to{}-{}x{}".format(*c))
def test_resblock_chain_on_a_forced_halo_form(ops, case):
    if ops.MMA_MODE == "f32":
        return res_f32(ops, case)
    run_res_presplit(ops, case, halo_for(case[4]), "halo")


# ---- 2. Downsample and Upsample ----------------------------------------------------------------------------------------------------
def run_resample(ops, down, C, H, W, path):
    from audioldm2_amd.unet import Downsample, Upsample
    if down:
        sd, x, ref, wrong = uf.down_case(C, H, W)
    else:
        (sd, x, ref), wrong = uf.up_case(C, H, W), None
    mod = uf.load((Downsample if down else Upsample)(C, True, out_channels=C), sd)
    xg = gpu_cl(x)
    if path != "staged" and ops.MMA_MODE == "f32":
        return f32_has_no_presplit_path(ops, mod.run, xg)
    on = path != "staged"
    parts = image_parts(ops, False) if on else 0
    what = "downsample pad 1 stride 2" if down else "upsample nearest x2"
    with dma(ops, on):
        assert ops.use_dma() == on
        with launches(ops, [parts]):
            whole = mod.run(xg)
        OH, OW = ((H + 1) // 2, (W + 1) // 2) if down else (2 * H, 2 * W)
        assert tuple(whole.shape) == (uf.B, OH, OW, C) == tuple(uf.cl(ref).shape)
        xin = xg
        if on:
            xin = ops.split_rows(xg)
            check_raw(ops, xin, xg, f"{what}: split_rows")
        kw = dict(stride=(2, 2), pad=(1, 1)) if down else dict(pad=(1, 1), up=(2, 2))
        out = guarded_conv(ops, xin, mod._pk, (uf.B, OH, OW, C), what, TILE[parts] if path == "tile" else None, **kw)
    check(uf.uncl(out), ref, gemm_tol(), f"{what} C{C} {H}x{W} {path}")
    check(uf.uncl(whole), ref, gemm_tol(), f"{what} C{C} {H}x{W} {path}: the module's run")
    if path != "tile":
        assert same_bits(whole, out)
    if down:   # the VAE's (0, 1, 0, 1) pad is another operation (another shape where H or W is odd)
        rejected(uf.uncl(out), wrong, gemm_tol(), "downsample vs the asymmetric pad")
        if H % 2 or W % 2:
            rejected(uf.uncl(out)[:, :, :H // 2, :W // 2], wrong, gemm_tol(), "downsample vs the asymmetric pad, the shared outputs")


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("C,H,W", uf.DOWN_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in uf.DOWN_CASES])
def test_downsample_with_the_symmetric_pad(ops, C, H, W, path):
    run_resample(ops, True, C, H, W, path)


@pytest.mark.parametrize("path", ["planner", "tile", "staged"])
@pytest.mark.parametrize("C,H,W", uf.UP_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in uf.UP_CASES])
def test_upsample_nearest_x2(ops, C, H, W, path):
    run_resample(ops, False, C, H, W, path)


# ---- 3. the transformer block -------------------------------------------------------------------------------------------------------
def tr_block(C, heads, ctx, sd):
    from audioldm2_amd.unet import BasicTransformerBlock
    return uf.load(BasicTransformerBlock(C, heads, 32, context_dim=uf.CONTEXT_DIM[ctx]), sd)


def normed(ops, x, gb, on, what):
    """One LayerNorm launch -> (the operand it hands the next GEMM, that operand's values on the CPU)."""
    ref = torch.nn.functional.layer_norm(x.double().cpu(), x.shape[-1:], gb[0].double().cpu(), gb[1].double().cpu(), uf.LN_EPS)
    if not on:
        y = ops.layernorm(x, *gb)
        check(y, ref, LN_BAR, f"{what}: LayerNorm")
        return y, values(y)
    y, img = ops.layernorm(x, *gb, split_out="also")
    check(y, ref, LN_BAR, f"{what}: LayerNorm")
    check_value_image(ops, img, y, f"{what}: LayerNorm image")
    if img.fmt == "f16":
        assert img.scale == ops._norm_f16_scale(*gb, x.shape[-1]) == uf.f16_scale_rule(*gb, x.shape[-1]), (what, img.scale)
    only = ops.layernorm(x, *gb, split_out="only")
    assert same_bits(only.data, img.data) and (only.fmt, only.scale, only.rn, only.rt) == (img.fmt, img.scale, img.rn, img.rt)
    return only, values(only)


def self_attention(ops, nop, nval, pw, w64, heads, pre, on, what, kinds):
    """[q | k | v] = n W^T and the attention over it, as BasicTransformerBlock.run issues them -> (fp32 result, operand for to_out)."""
    Bx, L, C = nval.shape
    qkv = guarded_linear(ops, nop, pw, (Bx, L, 3 * C), f"{what}: qkv projection")
    check(qkv, nval.double() @ w64.t(), gemm_tol(), f"{what}: qkv projection vs fp64 of its operand")
    kinds.append(kind(nop))
    if pre:
        with launches(ops, [nop.parts]):
            q, kimg, vtimg = ops.linear_qkv(nop, pw, heads, L)
        assert same_bits(q, qkv[:, :, :C]), "the QKV epilogue's q must be the plain projection's"
        a, aimg = ops.attention_presplit(q, kimg, vtimg, heads, split_out="also")
        only = ops.attention_presplit(q, kimg, vtimg, heads, split_out="only")
        assert same_bits(only.data, aimg.data)
        if getattr(kimg, "_aldm_f16", None) is None:   # bf16 K / V^T images: the fp32-K/V attention's products in its order
            a_old, s_old = ops.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], heads, split_out="also")
            assert same_bits(a, a_old) and same_bits(aimg.data, s_old.data), "pre-split attention must be bitwise the fp32-K/V one"
        else:
            assert ops.MMA_MODE == "f16x3"
    elif on:
        a, aimg = ops.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], heads, split_out="also")
    else:
        a, aimg = ops.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], heads), None
    qc = qkv.cpu()
    check(a, uf.attention(qc[..., :C], qc[..., C:2 * C], qc[..., 2 * C:], heads), fused_tol(), f"{what}: attention vs fp64 of its own q, k, v")
    if aimg is not None:
        check_value_image(ops, aimg, a, f"{what}: attention image")
    return a, (aimg if on else a)


def run_transformer_block(ops, C, heads, L, ctx, Bx, on, fold):
    """BasicTransformerBlock.run launch by launch (on: pre-split operands; fold: the folded cross-attention switched on), then as a
    whole: the same bits, and the launches `kinds` in the order they were replayed."""
    from audioldm2_amd import unet
    sd, h, context, mask, ref = uf.tr_case(C, heads, L, ctx, Bx)
    blk = tr_block(C, heads, ctx, sd)
    pk = blk._prepare()
    hg = h.cuda()
    cg, mg = (None if context is None else context.cuda()), (None if mask is None else mask.cuda())
    tag = f"transformer C{C} L{L} B{Bx} {ctx} {'pre-split' if on else 'staged'}{' fold' if fold else ''}"
    w = lambda *names: torch.cat([sd[n + ".weight"] for n in names], 0).double()
    lin64 = lambda v, name: uf.lin(v, sd, name)
    kinds = []
    prev_fold = ops.xattn_fold(bool(fold))
    try:
        with dma(ops, on):
            assert ops.use_dma() == on
            pre = on and unet.PRESPLIT_ATTENTION and C % 64 == 0
            assert pre == on, "every width here is a whole number of 64-column tiles: the QKV epilogue applies"
            # attn1
            nop, nval = normed(ops, hg, pk["ln"][0], on, f"{tag}: norm1")
            a, aop = self_attention(ops, nop, nval, pk["qkv1"], w("attn1.to_q", "attn1.to_k", "attn1.to_v"), heads, pre, on, f"{tag}: attn1", kinds)
            h1 = guarded_linear(ops, aop, pk["out1"], (Bx, L, C), "out1 + res", kinds, res=hg)
            check(h1, lin64(values(aop), "attn1.to_out.0") + h.double(), gemm_tol(), f"{tag}: out1 + res vs fp64 of its operand")
            check(h1, ref["h1"], fused_tol(), f"{tag}: h + attn1 vs fp64")
            h1c = h1.cpu()
            # attn2
            folds = context is not None and blk._fold_applies(h1, cg)
            if ctx.startswith("t5"):
                assert not ops.xattn_fold_applies(Bx, L, C, heads, uf.T5_LEN) and not folds, "the T5 context never folds"
            assert folds == (bool(fold) and on and ctx == "mae" and L % 32 == 0 and ops.xattn_fold_plan(Bx, L, C, heads, uf.MAE_LEN)["use"])
            if context is None:
                n2op, n2val = normed(ops, h1, pk["ln"][1], on, f"{tag}: norm2")
                assert pk["qkv2"] is not None
                a2, a2op = self_attention(ops, n2op, n2val, pk["qkv2"], w("attn2.to_q", "attn2.to_k", "attn2.to_v"), heads, pre, on,
                                          f"{tag}: attn2 as self-attention", kinds)
            else:
                with launches(ops, [0]):
                    kv = ops.linear(cg, pk["kv2"])
                check(kv, context.double() @ w("attn2.to_k", "attn2.to_v").t(), gemm_tol(), f"{tag}: K | V projection of the context")
                kvc = kv.cpu()
                n2_64 = uf.ln(h1c, sd, "norm2")
                if folds:
                    kinds.append(0)
                    fold_ops = ops.XattnFold(Bx, C, heads, context.shape[1], hg.device).prepare(kv, pk["wq2"], pk["wout2"])
                    h2 = ops.xattn_folded(h1, *pk["ln"][1], fold_ops, pk["bout2"], mask=mg)
                    a2_64 = uf.attention(uf.F.linear(n2_64, sd["attn2.to_q.weight"]), kvc[..., :C], kvc[..., C:], heads, mask)
                    check(h2, lin64(a2_64, "attn2.to_out.0") + h1c.double(), fused_tol(), f"{tag}: folded cross-attention vs fp64 of its own h, K | V")
                else:
                    n2op, n2val = normed(ops, h1, pk["ln"][1], on, f"{tag}: norm2")
                    q2 = guarded_linear(ops, n2op, pk["q2"], (Bx, L, C), "q2", kinds)
                    check(q2, n2val.double() @ sd["attn2.to_q.weight"].double().t(), gemm_tol(), f"{tag}: q2 vs fp64 of its operand")
                    kinds.append(0)
                    r = ops.attention(q2, kv[:, :, :C], kv[:, :, C:], heads, mask=mg, split_out="also" if on else None)
                    a2, a2img = r if on else (r, None)
                    a2op = a2img if on else a2
                    q2c = q2.cpu()
                    check(a2, uf.attention(q2c, kvc[..., :C], kvc[..., C:], heads, mask), fused_tol(),
                          f"{tag}: cross-attention vs fp64 of its own q, K | V and mask")
                    if a2img is not None:
                        check_value_image(ops, a2img, a2, f"{tag}: cross-attention image")
                    if mask is not None:
                        rejected(a2, uf.attention(q2c, kvc[..., :C], kvc[..., C:], heads, None), fused_tol(), "cross-attention vs one that ignores the mask")
                        # masked keys weigh exactly 0 where a key is real: their values, made huge, leave every bit as it was
                        real = mask.sum(1) > 0
                        kv_big = kv.clone()
                        kv_big[:, :, C:][(mg == 0) & real.cuda()[:, None]] = 1e30
                        a2_big = ops.attention(q2, kv_big[:, :, :C], kv_big[:, :, C:], heads, mask=mg)
                        assert same_bits(a2_big[real.cuda()], a2[real.cuda()]), "a masked key must weigh exactly 0"
                        for b in torch.nonzero(~real).flatten().tolist():   # an all-masked sample: the mean of every value row
                            check(a2[b], kvc[b, :, C:].double().mean(0).expand(L, C), fused_tol(), f"{tag}: all-masked sample is uniform")
            if not folds:
                h2 = guarded_linear(ops, a2op, pk["out2"], (Bx, L, C), "out2 + res", kinds, res=h1)
                check(h2, lin64(values(a2op), "attn2.to_out.0") + h1c.double(), gemm_tol(), f"{tag}: out2 + res vs fp64 of its operand")
            h2c = h2.cpu()
            # GEGLU and ff2
            n3op, n3val = normed(ops, h2, pk["ln"][2], on, f"{tag}: norm3")
            gbuf, gout = nan_view((Bx, L, 4 * C))
            with launches(ops, [kind(n3op)]):
                r = ops.linear_geglu(n3op, pk["ff1"], split_out="also" if on else None, out=gout)
            assert_guarded(gbuf, "GEGLU")
            kinds.append(kind(n3op))
            g, gop = r if on else (r, r)
            check(g, uf.geglu(n3val, sd, ""), fused_tol(), f"{tag}: GEGLU vs fp64 of its operand")
            if on:
                check_value_image(ops, gop, g, f"{tag}: GEGLU image")
                g_only = ops.linear_geglu(n3op, pk["ff1"], split_out="only")
                assert same_bits(g_only.data, gop.data) and g_only.fmt == gop.fmt
            out = guarded_linear(ops, gop, pk["ff2"], (Bx, L, C), "ff2 + res", kinds, res=h2)
            check(out, lin64(values(gop), "ff.net.2") + h2c.double(), gemm_tol(), f"{tag}: ff2 + res vs fp64 of its operand")
            # (the residual is four to six times the product here, so relative to the sum the product's error shows at a fraction of
            #  its size: the projection is also held to the bar on its own)
            plain = guarded_linear(ops, gop, pk["ff2"], (Bx, L, C), "ff2")
            check(plain, lin64(values(gop), "ff.net.2"), gemm_tol(), f"{tag}: ff2 alone vs fp64 of its operand")
            # the block as a whole: the same launches, the same bits
            with launches(ops, kinds):
                whole = blk.run(hg, cg, mg)
        check(whole, ref["out"], fused_tol(), f"{tag}: whole block")
        assert same_bits(whole, out), "BasicTransformerBlock.run must be the chain of these launches"
    finally:
        ops.xattn_fold(prev_fold)


@pytest.mark.parametrize("path", ["presplit", "staged"])
@pytest.mark.parametrize("C,heads,L,ctx,Bx", uf.TR_CASES, ids=lambda v: str(v))
def test_transformer_block_launch_by_launch(ops, C, heads, L, ctx, Bx, path):
    if path == "presplit" and ops.MMA_MODE == "f32":
        sd, h, context, mask, _ = uf.tr_case(C, heads, L, ctx, Bx)
        blk = tr_block(C, heads, ctx, sd)
        cg, mg = (None if context is None else context.cuda()), (None if mask is None else mask.cuda())
        return f32_has_no_presplit_path(ops, lambda t: blk.run(t, cg, mg), h.cuda())
    for fold in ((True, False) if (ctx == "mae" and path == "presplit") else (True,)):
        run_transformer_block(ops, C, heads, L, ctx, Bx, path == "presplit", fold)


def test_a_block_built_for_a_context_refuses_to_run_without_one(ops):
    sd, h, _, _, _ = uf.tr_case(128, 4, 24, "mae")
    blk = tr_block(128, 4, "mae", sd)
    for on in (True, False):
        with dma(ops, on):
            with pytest.raises(RuntimeError, match="context_dim but no context"):
                blk.run(h.cuda())


# ---- 4. SpatialTransformer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["presplit", "staged"])
@pytest.mark.parametrize("C,heads,depth,L,ctx", uf.ST_CASES, ids=lambda v: str(v))
def test_spatial_transformer_and_its_two_ends(ops, C, heads, depth, L, ctx, path):
    from audioldm2_amd.unet import SpatialTransformer
    sd, x, context, mask, ref = uf.st_case(C, heads, depth, L, ctx)
    H, W = uf.TR_TOKENS[L]
    P = H * W
    st = uf.load(SpatialTransformer(C, heads, 32, depth=depth, context_dim=uf.CONTEXT_DIM[ctx]), sd)
    xg = gpu_cl(x)
    cg, mg = (None if context is None else context.cuda()), (None if mask is None else mask.cuda())
    if path == "presplit" and ops.MMA_MODE == "f32":
        return f32_has_no_presplit_path(ops, lambda t: st.run(t, cg, mg), xg)
    on = path == "presplit"
    tag = f"spatial transformer C{C} depth {depth} L{L} {ctx} {path}"
    n_wrong = uf.gn(x, sd, "norm", uf.EPS)
    t_wrong = uf.conv(n_wrong, sd, "proj_in").permute(0, 2, 3, 1).reshape(uf.B, P, C)
    with dma(ops, on):
        assert ops.use_dma() == on
        whole = st.run(xg, cg, mg)
        pk = st._pk
        if on:
            a = ops.gn_split(xg, *pk["gn"], groups=32, eps=1e-6)
            check_image(ops, a, uf.cl(ref["n"]), *pk["gn"], (C // uf.GROUPS) * P, f"{tag}: gn_split (eps 1e-6, no activation)")
            rejected(uf.uncl(a.float()), n_wrong, fused_tol(), "gn_split vs GroupNorm with eps 1e-5")
            tok = guarded_conv(ops, a, pk["pin"], (uf.B, H, W, C), "proj_in")
            check(uf.uncl(tok), uf.conv(uf.uncl(a.float()), sd, "proj_in"), gemm_tol(), f"{tag}: proj_in vs fp64 of its image")
        else:
            sc, sh = ops.gn_stats(xg, *pk["gn"], groups=32, eps=1e-6)
            check_stats(sc, sh, xg, uf.cl(ref["n"]), f"{tag}: norm")
            tok = guarded_conv(ops, xg, pk["pin"], (uf.B, H, W, C), "proj_in", pre=(sc, sh))
        h = tok.view(uf.B, P, C)
        check(h, ref["tokens"], fused_tol(), f"{tag}: proj_in behind the GroupNorm")
        rejected(h, t_wrong, fused_tol(), "proj_in vs GroupNorm with eps 1e-5")
        hs = None
        for i, blk in enumerate(st.transformer_blocks):
            r = blk.run(h, cg, mg, want_split=on and i == depth - 1)
            h, hs = r if isinstance(r, tuple) else (r, None)
        assert (hs is not None) == on
        if on:
            check_value_image(ops, hs, h, f"{tag}: the image ff2 wrote with split_out='also'")
            out = guarded_conv(ops, hs.view(uf.B, H, W, C), pk["pout"], (uf.B, H, W, C), "proj_out", res=xg)
            again = ops.conv(ops.split_rows(h).view(uf.B, H, W, C), pk["pout"], res=xg)
            assert same_bits(out, again), "proj_out from the 'also' image must be proj_out from split_rows of the fp32 result"
            src = values(hs)
        else:
            out = guarded_conv(ops, h.view(uf.B, H, W, C), pk["pout"], (uf.B, H, W, C), "proj_out", res=xg)
            src = values(h)
    src_img = src.double().reshape(uf.B, H, W, C).permute(0, 3, 1, 2)
    check(uf.uncl(out), uf.conv(src_img, sd, "proj_out") + x.double(), gemm_tol(), f"{tag}: proj_out + res vs fp64 of its operand")
    check(uf.uncl(whole), ref["out"], fused_tol(), f"{tag}: whole")
    assert same_bits(whole, out), "SpatialTransformer.run must be the chain of these launches"


# ---- 5. the embedding path ------------------------------------------------------------------------------------------------------------
def emb_state(cfg, film, seed=25):
    """The parameters the embedding path reads, by name: time_embed, film_emb and every ResBlock's emb_layers.1 at the widths of cfg."""
    inp, mid, outb = ounet.unet_layout(cfg)
    widths = [l[2] for blk in inp + [mid] + outb for l in blk if l[0] == "res"]
    names = uf.res_prefixes(cfg)
    emb_ch = uf.EMB * (2 if film else 1)
    shapes = {"time_embed.0.weight": (uf.EMB, 128), "time_embed.0.bias": (uf.EMB,), "time_embed.2.weight": (uf.EMB, uf.EMB),
              "time_embed.2.bias": (uf.EMB,)}
    if film:
        shapes.update({"film_emb.weight": (uf.EMB, uf.FILM_DIM), "film_emb.bias": (uf.EMB,)})
    for rp, n in zip(names, widths):
        shapes.update({rp + "emb_layers.1.weight": (n, emb_ch), rp + "emb_layers.1.bias": (n,)})
    return weights.make_state_dict(shapes, seed=seed), names, widths


@pytest.mark.parametrize("cfg_name,Bx,film", [("tiny", 2, False), ("tiny", 3, True), ("full", 3, False), ("full", 2, True)])
def test_embedding_path_launch_by_launch(ops, cfg_name, Bx, film):
    """timestep_embedding -> te0 (SiLU epilogue) -> te2 -> [FiLM concat] -> emb_all (SiLU prologue, M = B rows, N = the real sum of the
    ResBlocks' widths), packed as UNetModel._prepare packs them; each ResBlock's slice against its own Linear(SiLU(emb))."""
    cfg = cases.UNET_TINY if cfg_name == "tiny" else cases.UNET_FULL
    sd, names, widths = emb_state(cfg, film)
    pack = lambda p: ops.pack_conv(sd[p + ".weight"], sd[p + ".bias"])
    emb_all = ops.pack_conv(torch.cat([sd[rp + "emb_layers.1.weight"] for rp in names], 0), torch.cat([sd[rp + "emb_layers.1.bias"] for rp in names], 0))
    t = torch.tensor(uf.TIMESTEPS[Bx])
    y = None
    if film:
        y = torch.randn(Bx, uf.FILM_DIM, generator=uf.gen(7))
        y = y / y.norm(dim=-1, keepdim=True)
    tag = f"embedding {cfg_name} B{Bx}{' FiLM' if film else ''}"
    t_emb = ops.timestep_embedding(t.float().cuda(), 128)
    t64 = uf.timestep_embedding(t, 128)
    err = (t_emb.double().cpu() - t64).abs().amax(1)
    yard = (ounet.timestep_embedding(t, 128).double() - t64).abs().amax(1)
    bound = timestep_embedding_tol(yard)
    for tb, e_k, e_t in zip(t.tolist(), err.tolist(), yard.tolist()):
        log_err(e_k, 2.0 * e_t, f"{tag}: timestep_embedding, t = {tb}, max |error| of the row")
        log_err(e_t, 0.0, f"{tag}: timestep_embedding, t = {tb}, torch fp32 on the CPU (yardstick)")
    print(f"{tag}: timestep_embedding |err| per row {err.tolist()} (torch fp32 {yard.tolist()}; bar: twice that)")
    assert bool((err <= bound).all()), (err, bound)
    own = uf.embedding(sd, t, y, names, t_emb=t_emb.cpu())
    h0 = guarded_linear(ops, t_emb, pack("time_embed.0"), (Bx, uf.EMB), "te0", act=ops.ACT_SILU)
    check(h0, own["h0"], fused_tol(), f"{tag}: te0 + SiLU vs fp64 of its operand")
    emb = guarded_linear(ops, h0, pack("time_embed.2"), (Bx, uf.EMB), "te2")
    check(emb, uf.lin(h0.cpu(), sd, "time_embed.2"), gemm_tol(), f"{tag}: te2 vs fp64 of its operand")
    if film:
        f = guarded_linear(ops, y.cuda(), pack("film_emb"), (Bx, uf.EMB), "film")
        check(f, uf.lin(y, sd, "film_emb"), gemm_tol(), f"{tag}: film_emb")
        emb = torch.cat([emb, f], dim=-1).contiguous()
        assert torch.equal(emb[:, uf.EMB:], f) and emb.shape == (Bx, 2 * uf.EMB)
    rows = guarded_linear(ops, emb, emb_all, (Bx, sum(widths)), "emb_all", pre_act=ops.ACT_SILU)
    ec = emb.cpu()
    check(rows, torch.cat([uf.row_bias(sd, ec, rp) for rp in names], -1), fused_tol(), f"{tag}: emb_all behind SiLU vs fp64 of its operand")
    off, worst = 0, 0.0
    for rp, n in zip(names, widths):   # each block's slice on its own max-norm
        e = uf.max_rel(rows[:, off:off + n], uf.row_bias(sd, ec, rp))
        assert e < fused_tol(), (rp, off, n, e)
        worst, off = max(worst, e), off + n
    log_err(worst, fused_tol(), f"{tag}: the worst ResBlock slice of emb_all")
    check(rows, own["emb_rows"], fused_tol(), f"{tag}: the whole path from the kernel's timestep embedding")


def test_the_models_own_embedding_is_that_path(ops):
    """UNetModel.forward itself on the reduced UNets: its te0 / te2 / FiLM / emb_all launches are taken out of the run (operands and
    results, through a spy on ops.linear as forward calls it) and held against fp64 of their own operands; every ResBlock.run must
    receive as its row bias the view of emb_all's result at ITS OWN columns (pointer, pitch and shape), never a copy.  The launches
    are register-staged in every mode (fp32 operands).  Their outputs are forward's own allocations, so no guard here: the same
    launches write into guarded buffers in test_embedding_path_launch_by_launch."""
    from audioldm2_amd.unet import ResBlock, UNetModel
    for name in ("tiny", "film_tiny"):
        cfg, latent = {"tiny": (cases.UNET_TINY, uf.LATENT_TINY), "film_tiny": (cases.UNET_FILM_TINY, uf.LATENT_FILM_TINY)}[name]
        model = UNetModel(**cfg)
        sd = uf.module_state(model, seed=25)
        model = uf.load(model, sd)
        x, t, ctxs, masks, y = cases.unet_inputs(cfg, latent[0], latent[2], latent[3], t5_len=uf.T5_LEN, seed=25)
        film = y is not None
        linears, biases = [], []
        real_linear, real_run = ops.linear, ResBlock.run

        def spy_linear(xx, pw, **kw):
            r = real_linear(xx, pw, **kw)
            linears.append((xx, pw, kw, r))
            return r

        def spy_run(self, xx, e, x2=None):
            biases.append((self, e))
            return real_run(self, xx, e, x2)
        ops.linear, ResBlock.run = spy_linear, spy_run
        ops.TUNE_LOG = []
        try:
            model(x.cuda(), t.cuda(), y=None if y is None else y.cuda(), context_list=[c.cuda() for c in ctxs],
                  context_attn_mask_list=[m.cuda() for m in masks])
            torch.cuda.synchronize()
            log = ops.TUNE_LOG
        finally:
            ops.linear, ResBlock.run = real_linear, real_run
            ops.TUNE_LOG = None
        pk = model._pk
        n_emb = 4 if film else 3
        want_pw = [pk["te0"], pk["te2"]] + ([pk["film"]] if film else []) + [pk["emb_all"]]
        assert all(c[1] is pw for c, pw in zip(linears[:n_emb], want_pw)), "forward's first launches are the embedding path"
        assert not any(k.endswith(SPLIT_SUFFIX) for k in log[:n_emb]), "the embedding path runs on fp32 operands"
        assert linears[0][2] == dict(act=ops.ACT_SILU) and linears[1][2] == {} and linears[n_emb - 1][2] == dict(pre_act=ops.ACT_SILU)
        t_emb, emb, rows = linears[0][0], linears[n_emb - 1][0], linears[n_emb - 1][3]
        own = uf.embedding(sd, t, y, uf.res_prefixes(cfg), t_emb=t_emb.cpu())
        tag = f"UNetModel.forward {name}"
        check(linears[0][3], own["h0"], fused_tol(), f"{tag}: te0 + SiLU vs fp64 of its operand")
        check(linears[1][3], uf.lin(linears[1][0].cpu(), sd, "time_embed.2"), gemm_tol(), f"{tag}: te2 vs fp64 of its operand")
        if film:
            assert torch.equal(linears[2][0].cpu(), y)
            check(linears[2][3], uf.lin(y, sd, "film_emb"), gemm_tol(), f"{tag}: film_emb")
            assert torch.equal(emb, torch.cat([linears[1][3], linears[2][3]], -1)) and emb.is_contiguous()
        else:
            assert emb is linears[1][3]
        ec = emb.cpu()
        blocks = [(n, m) for n, m in model.named_modules() if isinstance(m, ResBlock)]
        check(rows, torch.cat([uf.row_bias(sd, ec, n + ".") for n, _ in blocks], -1), fused_tol(), f"{tag}: emb_all vs fp64 of its operand")
        check(rows, own["emb_rows"], fused_tol(), f"{tag}: emb_all from the kernel's timestep embedding")
        # every ResBlock ran once, on the view of `rows` at its own columns
        assert sorted(id(m) for m, _ in biases) == sorted(id(m) for _, m in blocks) and rows.shape == (latent[0], sum(m.out_channels for _, m in blocks))
        off = 0
        for n, m in blocks:
            e = next(e for mm, e in biases if mm is m)
            assert m._emb_slice == slice(off, off + m.out_channels), (n, m._emb_slice, off)
            assert e.data_ptr() == rows.data_ptr() + 4 * off and e.stride() == (rows.shape[1], 1) and tuple(e.shape) == (latent[0], m.out_channels), n
            check(e, uf.row_bias(sd, ec, n + "."), fused_tol(), f"{tag}: the row bias ResBlock.run received vs its own Linear(SiLU(emb))")
            off += m.out_channels


# ---- 6. the ends ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cz,N,H,W", uf.CONV_IN_CASES, ids=lambda v: str(v))
def test_conv_in_from_the_latent_channels(ops, Cz, N, H, W):
    from audioldm2_amd.unet import _ConvIn
    z = torch.randn(uf.B, Cz, H, W, generator=uf.gen(Cz)) + 0.3
    mod = _ConvIn(Cz, N, 3, padding=1)
    sd = uf.module_state(mod, seed=Cz)
    mod = uf.load(mod, sd)
    with launches(ops, [0]):
        whole = mod.run(gpu_cl(z))
    assert mod._pk.K == 9 * Cz
    out = guarded_conv(ops, gpu_cl(z), mod._pk, (uf.B, H, W, N), "conv_in", pad=(1, 1))
    check(uf.uncl(out), uf.F.conv2d(z, sd["weight"], sd["bias"], padding=1), gemm_tol(), f"conv_in {Cz} -> {N}")
    assert same_bits(whole, out)


@functools.lru_cache(maxsize=None)
def out_conv_case(C, N, H, W):
    out = torch.nn.Sequential(torch.nn.GroupNorm(32, C), torch.nn.SiLU(), torch.nn.Conv2d(C, N, 3, padding=1))
    sd = uf.module_state(out, seed=N + H, prefix="out.")
    x = uf.feature_input(C, H, W, seed=N)
    return sd, x, uf.out_conv(sd, x)


@pytest.mark.parametrize("C,N,H,W", uf.CONV_OUT_CASES, ids=lambda v: str(v))
def test_out_conv_behind_the_groupnorm_prologue(ops, C, N, H, W):
    sd, x, ref = out_conv_case(C, N, H, W)
    xg = gpu_cl(x)
    ga, be = sd["out.0.weight"].cuda(), sd["out.0.bias"].cuda()
    pw = ops.pack_conv(sd["out.2.weight"], sd["out.2.bias"])
    sc, sh = ops.gn_stats(xg, ga, be, groups=32, eps=1e-5)
    check_stats(sc, sh, xg, uf.cl(uf.gn(x, sd, "out.0", uf.EPS)), f"out conv N = {N}: norm")
    out = guarded_conv(ops, xg, pw, (uf.B, H, W, N), f"out conv N = {N}", pad=(1, 1), pre=(sc, sh), pre_act=ops.ACT_SILU)
    got = uf.uncl(out)
    check(got, ref["out"], fused_tol(), f"out conv N = {N} {H}x{W}: conv behind GroupNorm + SiLU")
    rows_err = (got.double() - ref["out"]).abs().amax(1).reshape(-1)
    assert bool((rows_err < fused_tol() * ref["out"].abs().max()).all()), (N, int(rows_err.argmax()), float(rows_err.max()))


# ---- 7. the reduced UNets end to end ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reduced_case(name):
    from audioldm2_amd.unet import UNetModel
    cfg, latent = {"tiny": (cases.UNET_TINY, uf.LATENT_TINY), "film_tiny": (cases.UNET_FILM_TINY, uf.LATENT_FILM_TINY)}[name]
    sd = weights.make_state_dict(weights.shapes_of(UNetModel(**cfg)), seed=25)
    Bx, _, H, W = latent
    x, t, ctxs, masks, y = cases.unet_inputs(cfg, Bx, H, W, t5_len=uf.T5_LEN, seed=25)
    assert tuple(x.shape) == latent
    return cfg, sd, (x, t, ctxs, masks, y), uf.unet_forward(sd, cfg, x, t, ctxs, masks, y), ounet.unet_forward(sd, cfg, x, t, ctxs, masks, y=y)


@pytest.mark.parametrize("name", ["tiny", "film_tiny"])
def test_reduced_unet_end_to_end_against_the_fp64_restatement(ops, name):
    """A whole forward at 96 and 24 tokens, pre-split and register-staged, against the fp64 restatement under unet_tol; torch's own
    fp32 evaluation of oracle.unet on the CPU is logged next to them (no bar: what fp32 arithmetic itself gives on this graph)."""
    from audioldm2_amd.unet import UNetModel
    cfg, sd, (x, t, ctxs, masks, y), ref, ref32 = reduced_case(name)
    model = uf.load(UNetModel(**cfg), sd)
    mode = ops.MMA_MODE
    errs = {}
    for on in (True, False):
        with dma(ops, on):
            ops.TUNE_LOG = []
            try:
                got = model(x.cuda(), t.cuda(), y=None if y is None else y.cuda(), context_list=[c.cuda() for c in ctxs],
                            context_attn_mask_list=[m.cuda() for m in masks])
                torch.cuda.synchronize()
                log = ops.TUNE_LOG
            finally:
                ops.TUNE_LOG = None
        model.drop_step_caches()
        n_split = sum(k.endswith(SPLIT_SUFFIX) for k in log)
        assert (n_split > len(log) // 2) if (on and mode != "f32") else n_split == 0, (name, on, n_split, len(log))
        errs[on] = check(got, ref, unet_tol(), f"reduced UNet {name}, " + ("pre-split" if on else "register-staged"))
    e32 = log_err(uf.max_rel(ref32, ref), 0.0, f"reduced UNet {name}, torch fp32 on the CPU (yardstick)")
    print(f"reduced UNet {name} [{mode}] vs fp64: pre-split {errs[True]:.3e}, register-staged {errs[False]:.3e}, torch fp32 {e32:.3e} "
          f"(bar {unet_tol():.0e})")


# ---- the checks can fail: one lost partial product -----------------------------------------------------------------------------------
_FIVE_PRODUCT_CHILD = r"""
import sys, torch
sys.path.insert(0, {tests!r})
import unet_forms as uf
from audioldm2_amd import lib, ops
from audioldm2_amd.unet import BasicTransformerBlock, ResBlock
assert lib.LIB_PATH.endswith("libaldm_hip_testhooks.so"), lib.LIB_PATH
ops.set_mma("bf16x6")
ops.set_dma(True)
case = (128, 0, 256) + uf.HW_FUSED
sd, x, x2, rows, sl, ref = uf.res_case(*case)
blk = uf.load(ResBlock(128, uf.EMB, 0, out_channels=256), sd)
pk = blk._prepare()
e = rows.cuda()[:, sl]
a1 = ops.gn_split(uf.cl(x).cuda(), *pk["gn1"], groups=32, eps=1e-5, act=ops.ACT_SILU)
ref_h = uf.conv(uf.uncl(a1.float()), sd, "in_layers.2", padding=1) + ref["e"][:, :, None, None]
C, heads, L = 256, 8, 208
sdt, h, _, _, reft = uf.tr_case(C, heads, L, "none")
tb = uf.load(BasicTransformerBlock(C, heads, 32), sdt)
pkt = tb._prepare()
h2 = reft["h2"].float().cuda()
g = ops.linear_geglu(ops.layernorm(h2, *pkt["ln"][2], split_out="only"), pkt["ff1"], split_out="only")
assert g.fmt == "bf16" and g.parts == 3
ref_p = uf.lin(g.float().cpu(), sdt, "ff.net.2")
ref_o = ref_p + h2.cpu().double()
ops.igemm_force(64, 128, 1, 0, 2)          # the one tile that has a five-product form
for drop in (False, True, False):
    ops.debug_drop_product(drop)
    hh = ops.conv(a1, pk["conv1"], pad=(1, 1), rowbias=e)
    pp = ops.linear(g, pkt["ff2"])
    oo = ops.linear(g, pkt["ff2"], res=h2)
    print("RESULT", int(drop), uf.max_rel(uf.uncl(hh), ref_h), uf.max_rel(pp, ref_p), uf.max_rel(oo, ref_o))
ops.igemm_force(0, 0, 0)
"""


def test_a_lost_partial_product_fails_the_bars_of_the_chain():
    """With ops.debug_drop_product(True) (the five-product hook of libaldm_hip_testhooks.so, a process of its own through
    $ALDM_LIB_PATH) conv1 + row bias of the 128 -> 256 ResBlock and the ff2 projection of the C = 256 block in "bf16x6" miss gemm_tol
    against fp64 of their own operands, and meet it with six products.  ff2 + res is printed next to them, without an assert: the
    residual is 4.7 times the product there, so relative to the sum a lost product shows at a fifth of its size (measured 1.98e-6 with
    five products, 1.96e-7 with six, against the bar of 2e-6) — which is why the block test holds the projection to the bar on its
    own as well."""
    from audioldm2_amd import lib
    assert os.path.exists(lib.TESTHOOKS_LIB_PATH), "build() also builds audioldm2_amd/libaldm_hip_testhooks.so"
    env = dict(os.environ, ALDM_LIB_PATH=lib.TESTHOOKS_LIB_PATH, PYTHONPATH=ROOT)
    env.pop("ALDM_ERR_LOG", None)
    out = subprocess.run([sys.executable, "-c", _FIVE_PRODUCT_CHILD.format(tests=os.path.join(ROOT, "tests"))], env=env,
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [[float(v) for v in l.split()[1:]] for l in out.stdout.splitlines() if l.startswith("RESULT")]
    assert [int(r[0]) for r in rows] == [0, 1, 0], out.stdout[-2000:]
    g = gemm_tol("bf16x6")
    for drop, e_conv, e_ff, e_sum in rows:
        print(f"five-product hook {'on' if drop else 'off'}: conv1 + row bias {e_conv:.2e}, ff2 {e_ff:.2e} (bar {g:.0e}); ff2 + res {e_sum:.2e}")
        if drop:
            assert e_conv > g and e_ff > g, "the bars must catch one lost partial product"
        else:
            assert e_conv < g and e_ff < g and e_sum < g
    assert rows[0][1:] == rows[2][1:], "the switch must leave nothing behind"
    assert math.isfinite(rows[1][1])
