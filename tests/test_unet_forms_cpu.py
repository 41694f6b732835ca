"""The references of tests/test_unet_forms_gpu.py, validated before any kernel is compared with them (no GPU): the fp64 restatements
of tests/unet_forms.py equal oracle.unet evaluated in double, piece by piece and composed; every deliberately wrong reference lies at
least 100x the loosest bar away from the right one, on the inputs the GPU tests use; and the shape tables reach what they are in the
tables for (the concat seam inside a group, every GroupNorm form, the halo forms that hold two and four columns).

No GPU is needed, but the built library is: the shape-table test asks the library's host-only planners (ops.groupnorm_plan,
ops.xattn_fold_plan) which form a shape takes, as tests/test_vae_forms_cpu.py does, so it passes once build() has run."""
import contextlib

import pytest
import torch

import unet_forms as uf
from oracle import cases
from oracle import unet as ounet
from tolerances import F64

FP64_AGREEMENT = 1e-12     # two fp64 evaluations of the same graph in another operation order
LOOSEST_BAR = 5e-5         # the loosest bar any launch is held to in any mode (gemm_tol / fused_tol of "bf16x3")
SEPARATION = 100 * LOOSEST_BAR


@contextlib.contextmanager
def oracle_in_double():
    """oracle.unet with every torch.nn.functional call promoted to fp64 (tolerances.F64): its einsums, softmax and residual adds then
    run on doubles too.  Only its timestep embedding stays what it is, an fp32 evaluation."""
    prev = ounet.F
    ounet.F = F64
    try:
        yield
    finally:
        ounet.F = prev


def sep(wrong, right):
    return uf.max_rel(wrong, right)


@pytest.mark.parametrize("cfg,Bx,H,W,t5_len,seed", cases.UNET_CROSSCHECK, ids=["tiny", "large_tiny", "film_tiny"])
def test_composed_restatement_equals_the_oracle_in_double(cfg, Bx, H, W, t5_len, seed):
    from audioldm2_amd.unet import UNetModel
    sd = uf.module_state(UNetModel(**cfg), seed=seed)
    x, t, ctxs, masks, y = cases.unet_inputs(cfg, Bx, H, W, t5_len=t5_len, seed=seed)
    with oracle_in_double():
        want = ounet.unet_forward(uf.double_state(sd), cfg, x, t, ctxs, masks, y=y)
    assert want.dtype == torch.float64
    t_emb = ounet.timestep_embedding(t, cfg["model_channels"])
    got = uf.unet_forward(sd, cfg, x, t, ctxs, masks, y, t_emb=t_emb)
    assert got.dtype == torch.float64 and uf.max_rel(got, want) < FP64_AGREEMENT
    # with its own fp64 timestep embedding the restatement is only as far from that as the oracle's fp32 embedding is from fp64
    own = uf.unet_forward(sd, cfg, x, t, ctxs, masks, y)
    assert uf.max_rel(own, want) < 1e-5
    # the ResBlock prefixes are the product's module order (UNetModel._prepare walks self.modules())
    from audioldm2_amd.unet import ResBlock
    assert uf.res_prefixes(cfg) == [n + "." for n, m in UNetModel(**cfg).named_modules() if isinstance(m, ResBlock)]


@pytest.mark.parametrize("c1,c2,co", [(64, 0, 64), (64, 0, 96), (96, 64, 64)])
def test_resblock_restatement_equals_the_oracle(c1, c2, co):
    from audioldm2_amd.unet import ResBlock
    sd = uf.module_state(ResBlock(c1 + c2, uf.EMB, 0, out_channels=co), seed=5, prefix="blk.")
    x, x2 = uf.feature_input(c1, 5, 6), (uf.feature_input(c2, 5, 6, seed=2) if c2 else None)
    emb = uf.emb_input()
    xc = uf.concat(x, x2)
    with oracle_in_double():
        want = ounet.resblock(uf.double_state(sd), "blk", xc, emb.double(), c1 + c2, co)
    got = uf.resblock(sd, x, emb, x2, "blk.")
    assert all(v.dtype == torch.float64 for v in got.values()) and uf.max_rel(got["out"], want) < FP64_AGREEMENT
    assert torch.equal(got["raw"], xc) and (c1 + c2 != co or torch.equal(got["skip"], xc))
    assert uf.max_rel(uf.conv(got["n2"], sd, "blk.out_layers.3", padding=1) + got["skip"], got["out"]) < FP64_AGREEMENT
    assert uf.max_rel(uf.conv(got["n1"], sd, "blk.in_layers.2", padding=1) + got["e"][:, :, None, None], got["h"]) < FP64_AGREEMENT
    # a row bias given from outside replaces the block's own
    assert uf.max_rel(uf.resblock(sd, x, None, x2, "blk.", e=got["e"])["out"], got["out"]) < FP64_AGREEMENT


@pytest.mark.parametrize("ctx", uf.TR_CONTEXTS)
def test_transformer_block_restatement_equals_the_oracle(ctx):
    from audioldm2_amd.unet import BasicTransformerBlock
    C, heads, L = 64, 2, 11
    sd = uf.module_state(BasicTransformerBlock(C, heads, 32, context_dim=uf.CONTEXT_DIM[ctx]), seed=6, prefix="tb.")
    h = uf.token_input(C, L, batch=3)
    context, mask = uf.context_input(ctx, batch=3)
    with oracle_in_double():
        want = ounet.transformer_block(uf.double_state(sd), "tb", h.double(), heads, None if context is None else context.double(), mask)
    got = uf.transformer_block(sd, h, heads, context, mask, "tb.")
    assert uf.max_rel(got["out"], want) < FP64_AGREEMENT
    assert got["qkv"].shape == (3, L, 3 * C) and got["kv"].shape == (3, L if context is None else context.shape[1], 2 * C)
    if mask is not None:
        # an all-masked sample is uniform over EVERY key; elsewhere only the real keys count
        for b, n in enumerate(uf.T5_REAL_KEYS[ctx]):
            v = got["kv"][b, :, C:]
            if n == 0:
                assert uf.max_rel(got["a2"][b], v.mean(0).expand(L, C)) < FP64_AGREEMENT
            else:
                cut = uf.attention(got["q2"][b:b + 1], got["kv"][b:b + 1, :n, :C], v[None, :n], heads)
                assert uf.max_rel(got["a2"][b:b + 1], cut) < FP64_AGREEMENT


@pytest.mark.parametrize("depth,ctx", [(1, "none"), (2, "t5")])
def test_spatial_transformer_restatement_equals_the_oracle(depth, ctx):
    from audioldm2_amd.unet import SpatialTransformer
    C, heads = 64, 2
    sd = uf.module_state(SpatialTransformer(C, heads, 32, depth=depth, context_dim=uf.CONTEXT_DIM[ctx]), seed=7, prefix="st.")
    x = uf.st_input(C, 3, 5)
    context, mask = uf.context_input(ctx)
    with oracle_in_double():
        want = ounet.spatial_transformer(uf.double_state(sd), "st", x.double(), heads, depth, None if context is None else context.double(),
                                         mask)
    got = uf.spatial_transformer(sd, x, heads, depth, context, mask, "st.")
    assert uf.max_rel(got["out"], want) < FP64_AGREEMENT and len(got["blocks"]) == depth
    assert got["tokens"].shape == (uf.B, 15, C)


def test_resampling_restatements_are_the_oracle_lines():
    sd = {"op.weight": torch.randn(32, 32, 3, 3, generator=uf.gen(1)) / 17, "op.bias": torch.randn(32, generator=uf.gen(2))}
    sd["conv.weight"], sd["conv.bias"] = sd["op.weight"], sd["op.bias"]
    for H, W in ((7, 8), (8, 5), (12, 2)):
        x = uf.feature_input(32, H, W)
        with oracle_in_double():
            blk_d = ounet._run_block(uf.double_state({"b.0." + k: v for k, v in sd.items()}), "b", [("down", 32)], x.double(), None, [], [])
            blk_u = ounet._run_block(uf.double_state({"b.0." + k: v for k, v in sd.items()}), "b", [("up", 32)], x.double(), None, [], [])
        assert uf.max_rel(uf.downsample(sd, x), blk_d) < FP64_AGREEMENT and blk_d.shape == (uf.B, 32, (H + 1) // 2, (W + 1) // 2)
        assert uf.max_rel(uf.upsample(sd, x), blk_u) < FP64_AGREEMENT and blk_u.shape == (uf.B, 32, 2 * H, 2 * W)


# ---- the deliberately wrong references, on the inputs of the GPU tests ---------------------------------------------------------------
@pytest.mark.parametrize("c1,c2,co,H,W", [c for c in uf.RES_CONCAT_CASES + uf.RES_HALO_CASES if c[1]], ids=str)
def test_the_swapped_concat_is_far_from_the_right_one(c1, c2, co, H, W):
    sd, x, x2, rows, sl, ref = uf.res_case(c1, c2, co, H, W)
    wrong = uf.resblock(sd, x, None, x2, swapped=True, e=rows[:, sl])
    for k in ("n1", "skip", "h", "out"):
        assert sep(wrong[k], ref[k]) >= SEPARATION, (k, sep(wrong[k], ref[k]))


@pytest.mark.parametrize("c1,c2,co,H,W", uf.RES_CASES + uf.RES_CONCAT_CASES + uf.RES_HALO_CASES, ids=str)
def test_the_next_blocks_row_bias_is_far_from_the_right_one(c1, c2, co, H, W):
    sd, x, x2, rows, sl, ref = uf.res_case(c1, c2, co, H, W)
    assert sl.start == uf.ROW_OFFSET > 0 and rows.shape[1] > sl.stop + co and not rows[:, sl].is_contiguous()
    assert torch.equal(rows[:, sl].double(), ref["e"])
    e_wrong = rows[:, uf.shifted(sl, co)]
    h_wrong = uf.conv(ref["n1"], sd, "in_layers.2", padding=1) + e_wrong.double()[:, :, None, None]
    assert sep(h_wrong, ref["h"]) >= SEPARATION
    # ... and the block's own Linear(SiLU(emb)) is what the slice holds, to fp32 rounding
    assert uf.max_rel(rows[:, sl], uf.row_bias(sd, uf.emb_input())) < 2.0 ** -23


@pytest.mark.parametrize("C,H,W", uf.DOWN_CASES, ids=str)
def test_the_asymmetric_downsample_is_far_from_the_right_one(C, H, W):
    sd, x, ref, wrong = uf.down_case(C, H, W)
    assert ref.shape == (uf.B, C, (H + 1) // 2, (W + 1) // 2) and wrong.shape == (uf.B, C, H // 2, W // 2)
    # (an odd H or W: the asymmetric pad has one output row / column fewer, and the check rejects the shape; what they share differs)
    assert sep(wrong, ref[:, :, :H // 2, :W // 2]) >= SEPARATION


@pytest.mark.parametrize("C,heads,L,ctx,Bx", [c for c in uf.TR_CASES if c[3].startswith("t5")], ids=str)
def test_ignoring_the_mask_is_far_from_the_right_cross_attention(C, heads, L, ctx, Bx):
    sd, h, context, mask, ref = uf.tr_case(C, heads, L, ctx, Bx)
    wrong = uf.attention(ref["q2"], ref["kv"][..., :C], ref["kv"][..., C:], heads, None)
    h2_wrong = uf.lin(wrong, sd, "attn2.to_out.0") + ref["h1"]
    assert sep(wrong, ref["a2"]) >= SEPARATION and sep(h2_wrong, ref["h2"]) >= SEPARATION
    whole = uf.transformer_block(sd, h, heads, context, mask, use_mask=False)
    assert sep(whole["out"], ref["out"]) >= SEPARATION


@pytest.mark.parametrize("C,heads,depth,L,ctx", uf.ST_CASES, ids=str)
def test_eps_1e5_in_the_transformers_norm_is_far_from_the_right_one(C, heads, depth, L, ctx):
    sd, x, context, mask, ref = uf.st_case(C, heads, depth, L, ctx)
    n_wrong = uf.gn(x, sd, "norm", uf.EPS)
    t_wrong = uf.conv(n_wrong, sd, "proj_in").permute(0, 2, 3, 1).reshape(ref["tokens"].shape)
    assert sep(n_wrong, ref["n"]) >= SEPARATION and sep(t_wrong, ref["tokens"]) >= SEPARATION


def test_the_check_rejects_what_is_wrong_and_accepts_what_is_right():
    sd, x, ref, wrong = uf.down_case(*uf.DOWN_CASES[2])
    uf.assert_close(ref.float(), ref, LOOSEST_BAR, "downsample")
    with pytest.raises(AssertionError):
        uf.assert_close(ref.float(), wrong, LOOSEST_BAR, "downsample vs the asymmetric pad")
    with pytest.raises(AssertionError):
        uf.assert_close(torch.full((2, 2), float("nan")), torch.ones(2, 2), LOOSEST_BAR, "NaN")


# ---- the shape tables ----------------------------------------------------------------------------------------------------------------
def test_the_concat_seam_lies_inside_a_group_for_exactly_the_stated_pairs():
    pairs = {t[:2] for t in uf.CONCAT_TRIPLES}
    assert pairs == {(640, 640), (640, 384), (384, 256), (256, 128), (128, 128)}
    for c1, c2 in pairs:
        cg = (c1 + c2) // uf.GROUPS
        assert (c1 + c2) % uf.GROUPS == 0 and cg % 4 == 0          # whole float4s of channels per group: what the kernels take
        assert (c1 % cg != 0) == ((c1, c2) in uf.SEAM_INSIDE_A_GROUP) == uf.seam_inside_a_group(c1, c2), (c1, c2, cg)
    assert (384 + 256) // 32 == 20 and 384 / 20 == 19.2 and (256 + 128) // 32 == 12 and 256 % 12 == 4
    at = lambda hw: {c[:2] for c in uf.RES_CONCAT_CASES if c[3:] == hw}
    assert at(uf.HW_FUSED) == pairs
    assert at(uf.HW_CHUNKED) == set(uf.SEAM_INSIDE_A_GROUP) | {(128, 128)}
    assert at(uf.HW_COL2) == {(640, 640), (640, 384)}
    # every consumer width of a seam-inside pair is there: the decoder's real triples
    assert {c[:3] for c in uf.RES_CONCAT_CASES} == set(uf.CONCAT_TRIPLES)


def test_shape_tables_reach_what_they_are_in_the_tables_for():
    from test_dma_gpu import _HALO
    assert {c[:3:2] for c in uf.RES_CASES} == set(uf.RES_PAIRS) and all(c[1] == 0 for c in uf.RES_CASES)
    for H, W in (uf.HW_FUSED, uf.HW_CHUNKED):
        assert all((H * W) % t and (uf.B * H * W) % t for t in (64, 128, 256))
    # the GroupNorm form depends on the slab (channels per group x pixels), not on the pixels alone: every form is reached, with a
    # second operand and without, for gn_split and for gn_stats
    for table, want in ((uf.RES_CASES, {"fused", "fused_split", "chunked"}), (uf.RES_CONCAT_CASES, {"fused", "fused_split", "chunked"})):
        split = {uf.plan(H * W, c1, c2, True)["form"] for c1, c2, _, H, W in table} | {uf.plan(H * W, co, 0, True)["form"] for _, _, co, H, W in table}
        stats = {uf.plan(H * W, c1, c2, False)["form"] for c1, c2, _, H, W in table}
        assert split == want and stats == {"fused", "chunked"}, (split, stats)
    assert all(uf.plan(H * W, c1, c2, True)["form"] == "chunked" for c1, c2, _, H, W in uf.RES_CONCAT_CASES if (H, W) == uf.HW_CHUNKED)
    # halo cases are whole 128-row tiles of one image; the two- and four-column ones run the (128, 128, 403) form, which
    # tests/test_dma_gpu.py lists for both split widths (test_dma_halo_image_widths runs it at W = 4 and W = 2)
    for _, _, _, H, W in uf.RES_HALO_CASES:
        assert (H * W) % 128 == 0 and 128 % W == 0 and W & (W - 1) == 0
    assert {c[4] for c in uf.RES_HALO_CASES} == {16, 4, 2}
    assert all((128, 128, 403) in _HALO[m] for m in ("bf16x6", "bf16x3"))
    assert any(H % 2 for _, H, _ in uf.DOWN_CASES) and any(H % 2 == 0 for _, H, _ in uf.DOWN_CASES) and any(W % 2 == 0 for *_, W in uf.DOWN_CASES)
    assert {h * w for h, w in uf.TR_TOKENS.values()} == set(uf.TR_TOKENS) == {24, 64, 208} and 24 < 32 and 208 % 32 == 16
    assert all(h * 32 == c for c, h in uf.TR_WIDTHS) and uf.T5_LEN % 32 and uf.MAE_LEN == 8
    assert {n for v in uf.T5_REAL_KEYS.values() for n in v} == {21, 7, 1, 0}
    assert (384, 12, 24, "t5", 3) in uf.TR_CASES
    # the folded cross-attention takes whole 32-row tiles and at most 8 keys: of these shapes the AudioMAE context at L = 64, at every
    # width and batch (the planner's gate keeps it there); never the T5 context
    from audioldm2_amd import ops
    for C, heads, L, ctx, Bx in uf.TR_CASES:
        if ctx == "mae":
            assert ops.xattn_fold_plan(Bx, L, C, heads, uf.MAE_LEN)["use"] == (L == 64), (C, L, Bx)
    assert uf.T5_LEN > ops.XATTN_FOLD_MAX_KEYS >= uf.MAE_LEN
    assert [c * 9 for c, *_ in uf.CONV_IN_CASES] == [72, 144] and {n for _, n, *_ in uf.CONV_OUT_CASES} == {8, 16}
    # emb_all: the real sums of the ResBlocks' widths
    widths = lambda cfg: sum(l[2] for blks in (lambda a, b, c: a + [b] + c)(*ounet.unet_layout(cfg)) for l in blks if l[0] == "res")
    assert widths(cases.UNET_TINY) == 128 + 256 + 256 + 256 + 256 + 256 + 128 + 128
    assert widths(cases.UNET_FULL) == 8320 and len(uf.res_prefixes(cases.UNET_FULL)) == 22
    for cfg, lat in ((cases.UNET_TINY, uf.LATENT_TINY), (cases.UNET_FILM_TINY, uf.LATENT_FILM_TINY)):
        assert lat[1] == cfg["in_channels"] and lat[2] * lat[3] == 96 and (lat[2] // 2) * (lat[3] // 2) == 24
