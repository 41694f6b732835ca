"""The references of tests/test_vae_forms_gpu.py, validated before any kernel is compared with them (no GPU): the fp64 restatements
of tests/vae_forms.py equal the corresponding pieces of oracle.vae evaluated in double on a small state dict; the deliberately wrong
references differ from the right ones by far more than any bar; and the shape tables reach what they are in the tables for —
through the host-only plan query, so a changed GroupNorm threshold fails here instead of moving a GPU case to another kernel."""
import os

import pytest
import torch

import vae_forms as vf
from oracle import vae as ovae
from tolerances import LONG_K

FP64_AGREEMENT = 1e-12     # two fp64 evaluations of the same graph in another operation order


@pytest.fixture(scope="module")
def tiny():
    dd = vf.DD_TINY
    sd = vf.vae_state(dd, seed=3)
    return dd, sd, vf.double_state(sd)


def _x(C, H, W):
    return vf.feature_input(C, H, W)


@pytest.mark.parametrize("cin,cout", [(32, 32), (32, 64), (64, 32)])
def test_resnet_block_restatement_equals_the_oracle(cin, cout):
    from audioldm2_amd.vae import ResnetBlock
    sd = vf._module_state(ResnetBlock(in_channels=cin, out_channels=cout), seed=5, prefix="blk.")
    x = _x(cin, 5, 6)
    want = ovae.resnet_block(vf.double_state(sd), "blk", x.double(), cin, cout)
    got = vf.resnet_block(sd, x, "blk.")
    assert vf.max_rel(got["out"], want) < FP64_AGREEMENT
    assert got["out"].dtype == torch.float64 and all(v.dtype == torch.float64 for v in got.values())
    # the intermediates are the chain's own: out = conv2(n2) + skip, n2 = swish(norm2(h)), h = conv1(n1)
    assert vf.max_rel(vf.conv(got["n2"], sd, "blk.conv2", padding=1) + got["skip"], got["out"]) == 0.0
    assert vf.max_rel(vf.gn(got["h"], sd, "blk.norm2", True), got["n2"]) == 0.0
    if cin == cout:
        assert torch.equal(got["skip"], x.double())


def test_attn_block_restatement_equals_the_oracle():
    from audioldm2_amd.vae import AttnBlock
    C, H, W = 64, 3, 5
    sd = vf._module_state(AttnBlock(C), seed=6, prefix="att.")
    x = _x(C, H, W)
    want = ovae.attn_block(vf.double_state(sd), "att", x.double())
    got = vf.attn_block(sd, x, "att.")
    assert vf.max_rel(got["out"], want) < FP64_AGREEMENT
    L = H * W
    assert got["qkv"].shape == (vf.B, L, 3 * C) and got["scores"].shape == (vf.B, L, L) and got["o"].shape == (vf.B, L, C)
    assert float((got["probs"].sum(-1) - 1).abs().max()) < 1e-14
    q, k = got["qkv"][:, :, :C], got["qkv"][:, :, C:2 * C]
    # (in the memory layout the restatement's own q and k have — [B, C, L] transposed — so that the CPU's BLAS sums the same way)
    as_rows = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    assert vf.max_rel(vf.attn_scores(as_rows(q), as_rows(k), C), got["scores"]) == 0.0


def test_whole_decoder_and_encoder_out_of_the_restatements_equal_the_oracle(tiny):
    """Upsample and Downsample have no function of their own in the oracle: they are lines of decoder_forward / encoder_forward.  The
    whole graphs, built from the restatements, equal oracle.vae.vae_decode / vae_encode_moments in double."""
    dd, sd, sd64 = tiny
    z = torch.randn(2, dd["z_channels"], 3, 8, generator=vf.gen(1))
    assert vf.max_rel(vf.vae_decode(sd, dd, z), ovae.vae_decode(sd64, dd, z.double())) < FP64_AGREEMENT
    mel = vf.mel_for(dd, (2, dd["z_channels"], 3, 8))
    assert mel.shape == (2, 1, 6, 16)
    got = vf.vae_encode_moments(sd, dd, mel)
    assert got.shape == (2, 2 * dd["z_channels"], 3, 8)
    assert vf.max_rel(got, ovae.vae_encode_moments(sd64, dd, mel.double())) < FP64_AGREEMENT


@pytest.mark.parametrize("H,W", [(7, 8), (8, 8), (5, 3)])
def test_up_and_downsample_restatements_are_the_oracle_lines(tiny, H, W):
    """... and one by one, against the oracle's own two lines each (oracle/vae.py decoder_forward / encoder_forward)."""
    import torch.nn.functional as F
    dd, sd, sd64 = tiny
    C = dd["ch"]
    x = _x(C, H, W)
    p = "encoder.down.0.downsample.conv"
    want = ovae._conv(F.pad(x.double(), (0, 1, 0, 1), mode="constant", value=0), sd64, p, stride=2)
    got = vf.downsample(sd, x, p)
    assert got.shape == (vf.B, C, (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1) and vf.max_rel(got, want) == 0.0
    C = dd["ch"] * dd["ch_mult"][-1]
    x = _x(C, H, W)
    p = "decoder.up.1.upsample.conv"
    want = ovae._conv(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), sd64, p, padding=1)
    got = vf.upsample(sd, x, p)
    assert got.shape == (vf.B, C, 2 * H, 2 * W) and vf.max_rel(got, want) == 0.0


def test_wrong_references_fail_the_checks(tiny):
    """The three deliberately wrong references are far from the right ones: the check the GPU tests use (vae_forms.assert_close under
    the loosest bar any mode has, 5e-5) passes on the right reference and fails on the wrong one."""
    dd, sd, _ = tiny
    loosest = 5e-5
    x = _x(dd["ch"], 7, 8)
    p = "encoder.down.0.downsample.conv"
    right = vf.downsample(sd, x, p)
    vf.assert_close(right.float(), right, loosest, "downsample")
    with pytest.raises(AssertionError):
        vf.assert_close(right.float(), vf.downsample_symmetric(sd, x, p), loosest, "downsample vs symmetric padding")
    x = _x(dd["ch"] * dd["ch_mult"][-1], 3, 8)
    p = "decoder.up.1.upsample.conv"
    right = vf.upsample(sd, x, p)
    with pytest.raises(AssertionError):
        vf.assert_close(right.float(), vf.upsample_bilinear(sd, x, p), loosest, "upsample vs bilinear")
    C, L = 64, 15
    qkv = torch.randn(vf.B, L, 3 * C, generator=vf.gen(2)) + 0.3
    right = vf.attn_scores(qkv[:, :, :C], qkv[:, :, C:2 * C], C)
    qw, kw = vf.slices_at_pitch_c(qkv, C)
    assert torch.equal(qw[:, 0], qkv[:, 0, :C]) and torch.equal(kw[:, 0], qkv[:, 0, C:2 * C]) and torch.equal(qw[:, 1], qkv[:, 0, C:2 * C])
    with pytest.raises(AssertionError):
        vf.assert_close(right.float(), vf.attn_scores(qw, kw, C), loosest, "scores vs slices at pitch C")
    with pytest.raises(AssertionError):
        vf.assert_close(torch.full((2, 2), float("nan")), torch.ones(2, 2), loosest, "NaN")


def test_shape_tables_reach_what_they_are_in_the_tables_for():
    assert "ALDM_GN_FUSED_MAX" not in os.environ and "ALDM_GN_SPLIT_FUSED" not in os.environ
    assert {(ci, co) for ci, co, _, _ in vf.RES_CASES} == set(vf.RES_PAIRS)
    for ci, co, H, W in vf.RES_CASES + vf.RES_HALO_CASES:
        P = H * W
        for C in (ci, co):
            for want_split in (False, True):
                form = vf.plan(P, C, want_split)["form"]
                assert form.startswith(vf.expected_form(P)), (ci, co, H, W, C, want_split, form)
    assert vf.expected_form(13 * 16) == "fused" and vf.expected_form(65 * 16) == "chunked"
    # no tile of 64 / 128 / 256 rows divides a sample or the launch, and a row tile straddles the seam between the samples
    for H, W in (vf.HW_FUSED, vf.HW_CHUNKED):
        assert all((H * W) % t and (vf.B * H * W) % t for t in (64, 128, 256))
    assert {W for _, _, H, W in vf.RES_CASES if H == 5} == {32, 64}
    # ... which is exactly what the halo-patch kernel cannot run; its cases are whole 128-row tiles of one image
    for _, _, H, W in vf.RES_HALO_CASES:
        assert (H * W) % 128 == 0 and 128 % W == 0 and W & (W - 1) == 0
    assert {vf.expected_form(H * W) for _, _, H, W in vf.RES_HALO_CASES} == {"fused", "chunked"}
    assert {W for _, _, _, W in vf.RES_HALO_CASES} == {16, 32, 64}
    assert [h * w for _, h, w in vf.ATTN_CASES] == [112, 64] and 112 % 32 != 0
    assert all(K >= LONG_K and K % 4 == 0 for K in vf.ATTN_LONG_K) and any(K % 32 for K in vf.ATTN_LONG_K)
    assert any(H % 2 for _, H, _ in vf.DOWN_CASES) and any(H % 2 == 0 for _, H, _ in vf.DOWN_CASES)
    C, P = vf.F16_SLAB
    assert (C // vf.GROUPS) * P == 1 << 20 and vf.plan(P, C, True, batch=1)["form"] == "chunked"
    assert [c * 9 for c, _, _, _ in vf.DEC_IN_CASES] == [72, 144]
    f = 2 ** (len(vf.DD_REDUCED["ch_mult"]) - 1)
    assert vf.LATENT_REDUCED[3] * f == vf.DD_REDUCED["mel_bins"]
    # whole float4s of channels per group is what the GroupNorm kernels take: the reduced VAE has them at every level, ch = 64 has not
    assert all((vf.DD_REDUCED["ch"] * m // vf.GROUPS) % 4 == 0 for m in vf.DD_REDUCED["ch_mult"])
    assert (vf.DD_REFUSED["ch"] // vf.GROUPS) % 4 != 0


def test_f16_scale_rule_is_the_one_ops_applies():
    """(ops._norm_f16_scale itself reads max|gamma| on the device: the GPU test holds the image's scale against it.)"""
    from audioldm2_amd import ops
    C, P = vf.F16_SLAB
    ga, be = torch.randn(C, generator=vf.gen(2)), torch.randn(C, generator=vf.gen(3))
    for n in (4 * 208, 1 << 15, 1 << 18, 1 << 20):
        s = vf.f16_scale_rule(ga, be, n)
        bound = (n ** 0.5) * float(ga.abs().max()) + float(be.abs().max())
        assert s == ops._pow2_scale(bound)
        assert 16384.0 < s * bound <= 32768.0
    # n is 2^5 times the largest the f16x3 tests had: sqrt(n) takes two to three more bits out of the image's scale
    assert vf.f16_scale_rule(ga, be, 1 << 15) / vf.f16_scale_rule(ga, be, 1 << 20) in (4.0, 8.0)
