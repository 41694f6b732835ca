"""Shapes, input recipes and fp64 restatements of the launch forms the VAE issues (audioldm2_amd/vae.py): the ResnetBlock chain,
the mid attention, the asymmetric-pad downsample, the nearest-x2 upsample and the end convs.  tests/test_vae_forms_cpu.py shows the
restatements equal the corresponding pieces of oracle.vae evaluated in double; tests/test_vae_forms_gpu.py runs the launches
against them.  Importable without a GPU: torch on the CPU only (the plan query is host code).

Every restatement is plain torch in fp64 on fp32 inputs, NCHW like the oracle; `cl` / `uncl` move between that and the engine's
channels-last layout.  They return every intermediate a launch of the module produces, so each launch can be held against fp64 of
ITS OWN inputs."""
import math

import torch

import norm_forms as nf
from tolerances import F64 as F

MODES = ("f32", "bf16x6", "bf16x3", "f16x3")
B = 2
EPS = 1e-6           # every GroupNorm of the VAE (model.py:38-41)
GROUPS = 32
# pixel counts: 208 = 13 x 16 (fused GroupNorm; M = 416: no tile divides it and a row tile straddles the seam between the two samples),
# 1040 = 65 x 16 (above 1024: the chunked GroupNorm form)
HW_FUSED, HW_CHUNKED = (13, 16), (65, 16)
RES_PAIRS = [(128, 128), (128, 256), (256, 128), (512, 256), (512, 512)]
# (Cin, Cout, H, W): every channel pair at both pixel counts, then the decoder's level-0 (W = 64) and level-1 (W = 32) widths at H = 5
RES_CASES = [(ci, co, h, w) for ci, co in RES_PAIRS for h, w in (HW_FUSED, HW_CHUNKED)] + [(256, 128, 5, 64), (512, 256, 5, 32)]
# The halo-patch kernel runs tiles that are whole image rows of ONE image (OH * OW a multiple of the 128-row tile, W a power of two):
# none of the shapes above qualifies — they are chosen so that no tile divides them — so a forced halo form gets shapes of its own,
# the nearest ones that do: 16 x 16 (fused), 80 x 16 (chunked), and the two decoder widths at two tiles per image.
RES_HALO_CASES = [(128, 128, 16, 16), (128, 256, 80, 16), (256, 128, 4, 64), (512, 256, 8, 32)]
ATTN_CASES = [(512, 7, 16), (1024, 2, 32)]            # (C, h, w): L = 112 (no multiple of 32) and L = 64
ATTN_LONG_K = [3104, 3100]                            # >= tolerances.LONG_K; 3104 = 97 x 32 (an odd number of 32-wide k-tiles), 3100 = 96 x 32 + 28
DOWN_CASES = [(128, 7, 64), (128, 8, 64), (256, 7, 32)]   # (C, H, W): odd H puts the padded bottom row into the last output row
UP_CASES = [(512, 3, 16), (256, 5, 32)]
CONV_OUT_CASES = [(128, 1) + HW_FUSED, (128, 1) + HW_CHUNKED]               # Decoder.conv_out: (C, N, H, W)
ENC_OUT_CASES = [(512, 16) + HW_FUSED, (512, 32) + HW_FUSED]                # Encoder.conv_out
DEC_IN_CASES = [(8, 512) + HW_FUSED, (16, 1024) + HW_FUSED]                 # Decoder.conv_in: K = 72 / 144
ENC_IN_HW = HW_FUSED                                                        # Encoder.conv_in: 1 channel padded to 4, K = 36
F16_SLAB = (128, 262144)                                                    # (C, P): n = 4 x 262144 = 2^20, the 48 kHz decoder's last level
# one reduced VAE end to end: three levels, a (2, 8, 5, 16) latent <-> a (2, 1, 20, 64) mel.  ch = 128 is the narrowest the library
# runs: its GroupNorm kernels need whole float4s of channels per group ((C / 32) % 4 == 0, include/aldm_hip.h), so 32 groups need
# 128 channels.  DD_REFUSED (ch = 64: two channels per group) is refused by aldm_groupnorm_stats / _split, loudly.
DD_REDUCED = {"double_z": True, "mel_bins": 64, "z_channels": 8, "resolution": 256, "downsample_time": False, "in_channels": 1,
              "out_ch": 1, "ch": 128, "ch_mult": [1, 2, 4], "num_res_blocks": 2, "attn_resolutions": [], "dropout": 0}
DD_REFUSED = dict(DD_REDUCED, ch=64)
GN_REFUSAL = r"\(C/G\)%4==0"
LATENT_REDUCED = (2, 8, 5, 16)
# the CPU check of the restatements: the same graph at a size fp64 on the CPU evaluates in no time
DD_TINY = dict(DD_REDUCED, ch=32, ch_mult=[1, 2], mel_bins=16, num_res_blocks=1)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cl(x):
    """NCHW (CPU) -> the engine's channels-last layout (still on the CPU)."""
    return x.permute(0, 2, 3, 1).contiguous()


def uncl(y):
    """channels-last (any device) -> NCHW on the CPU."""
    return y.detach().cpu().permute(0, 3, 1, 2).contiguous()


def max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def assert_close(got, ref, bar, what=""):
    """The check every comparison of these tests goes through: max|got - ref| / max|ref| < bar, same shape, nothing non-finite."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values in the result"
    e = max_rel(got, ref)
    assert e < bar, f"{what}: {e:.3e} >= {bar:.1e}"
    return e


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def plan(P, C, want_split=False, batch=B):
    from audioldm2_amd import ops
    return ops.groupnorm_plan(batch, P, C, 0, GROUPS, want_split)


def expected_form(P):
    return "chunked" if P > 1024 else "fused"


def feature_input(C, H, W, seed=0, batch=B):
    """x [B, C, H, W] fp32: the trend recipe of tests/norm_forms.py (Gaussian of spread 2 about 0.5, a per-channel offset, a ramp
    along the pixels) under a per-channel gain of 1/16 .. 1/4 — a non-zero mean, so a padding, halo or seam mistake changes the
    result, and groups whose channels differ in scale.  The gains are powers of two and their multiples by 1.5 and leave max|x| near 4,
    the size of the conv outputs x meets as a residual: neither side of `conv + skip` hides the other's error."""
    case = nf.GnCase(batch, H * W, C, 0, GROUPS, None, None, None, None, None, "")
    x = nf.gn_input(case, "trend")                                   # [B, P, C]
    if seed:
        x = x + torch.randn(x.shape, generator=gen(1000 + seed))
    gain = (0.5 + 0.5 * (torch.arange(C) % 4).float()) / 8
    return (x * gain).view(batch, H, W, C).permute(0, 3, 1, 2).contiguous()


def _module_state(module, seed, prefix=""):
    """Deterministic weights of a module by parameter name (oracle.weights), its GroupNorm gains and shifts replaced by N(0, 1)
    draws as in tests/norm_forms.py gn_params: gains of either sign and of widely different size."""
    from oracle import weights
    sd = weights.make_state_dict({prefix + k: v for k, v in weights.shapes_of(module).items()}, seed=seed)
    for k in list(sd):
        if ".norm" in "." + k and sd[k].dim() == 1:
            sd[k] = torch.randn(sd[k].shape, generator=gen(seed * 7919 + (2 if k.endswith("weight") else 3) + len(k)))
    return sd


def attn_state(C, seed):
    """... of an AttnBlock, with the q and k projections scaled by 1.5: scores of up to +-5 instead of +-2.4, so the softmax is not
    nearly uniform and a wrong score moves the probabilities."""
    from audioldm2_amd.vae import AttnBlock
    sd = _module_state(AttnBlock(C), seed)
    for n in ("q", "k"):
        sd[n + ".weight"] = sd[n + ".weight"] * 1.5
        sd[n + ".bias"] = sd[n + ".bias"] * 1.5
    return sd


def load(module, seed):
    """-> (module on the GPU with deterministic weights, its state dict on the CPU)."""
    sd = _module_state(module, seed)
    module.load_state_dict(sd, strict=True)
    return module.cuda().eval(), sd


# ---- fp64 restatements ---------------------------------------------------------------------------------------------------------
def swish(x):
    return x * torch.sigmoid(x)


def gn(x, sd, p, act=False):
    """GroupNorm(32, eps 1e-6) of NCHW x in fp64 (+ swish)."""
    y = F.group_norm(x, GROUPS, sd[p + ".weight"], sd[p + ".bias"], EPS)
    return swish(y) if act else y


def conv(x, sd, p, stride=1, padding=0):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), stride=stride, padding=padding)


def resnet_block(sd, x, p=""):
    """-> {n1, h, n2, skip, out}: swish(norm1 x), conv1 of it, swish(norm2 h), the (1x1) shortcut, conv2 n2 + skip.  All fp64."""
    r = {"n1": gn(x, sd, p + "norm1", True)}
    r["h"] = conv(r["n1"], sd, p + "conv1", padding=1)
    r["n2"] = gn(r["h"], sd, p + "norm2", True)
    r["skip"] = conv(x, sd, p + "nin_shortcut") if (p + "nin_shortcut.weight") in sd else x.double()
    r["out"] = conv(r["n2"], sd, p + "conv2", padding=1) + r["skip"]
    return r


def attn_scores(q, k, C):
    """q, k [B, L, C] -> bmm(q, k^T) C^-0.5 in fp64."""
    return torch.bmm(q.double(), k.double().transpose(1, 2)) * (int(C) ** (-0.5))


def attn_block(sd, x, p=""):
    """-> {n, qkv [B, L, 3C], scores, probs [B, L, L], o [B, L, C], out [B, C, H, W]}.  All fp64."""
    Bx, C, H, W = x.shape
    L = H * W
    r = {"n": gn(x, sd, p + "norm")}
    rows = lambda t: t.reshape(Bx, C, L).permute(0, 2, 1)
    q, k, v = (rows(conv(r["n"], sd, p + n)) for n in ("q", "k", "v"))
    r["qkv"] = torch.cat([q, k, v], -1)
    r["scores"] = attn_scores(q, k, C)
    r["probs"] = torch.softmax(r["scores"], -1)
    r["o"] = torch.bmm(r["probs"], v)
    o_img = r["o"].permute(0, 2, 1).reshape(Bx, C, H, W)
    r["out"] = x.double() + conv(o_img, sd, p + "proj_out")
    return r


def downsample(sd, x, p="conv"):
    """model.py:88-93: F.pad (0, 1, 0, 1) then conv k3 s2 p0."""
    return conv(F.pad(x.double(), (0, 1, 0, 1), mode="constant", value=0), sd, p, stride=2)


def downsample_symmetric(sd, x, p="conv"):
    """A deliberately WRONG reference: padding 1 on every side (the checks must tell it from the asymmetric one)."""
    return conv(x, sd, p, stride=2, padding=1)


def upsample(sd, x, p="conv"):
    """model.py:53-57: nearest x2 then conv k3 p1."""
    return conv(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), sd, p, padding=1)


def upsample_bilinear(sd, x, p="conv"):
    """A deliberately WRONG reference: bilinear x2."""
    return conv(F.interpolate(x.double(), scale_factor=2.0, mode="bilinear", align_corners=False), sd, p, padding=1)


def slices_at_pitch_c(qkv, C):
    """A deliberately WRONG pair of operands: q and k read out of the fused [B, L, 3C] buffer with row pitch C instead of 3C (what a
    kernel that ignores the pitch of a column slice would read)."""
    Bx, L, _ = qkv.shape
    flat = qkv.reshape(Bx, -1)
    return flat[:, :L * C].reshape(Bx, L, C), flat[:, C:C + L * C].reshape(Bx, L, C)


def decoder(sd, dd, z, p="decoder."):
    """Decoder.forward (model.py:653-686) out of the pieces above, fp64."""
    ch, mult, nrb = dd["ch"], list(dd["ch_mult"]), dd["num_res_blocks"]
    h = conv(z, sd, p + "conv_in", padding=1)
    h = resnet_block(sd, h, p + "mid.block_1.")["out"]
    h = attn_block(sd, h, p + "mid.attn_1.")["out"]
    h = resnet_block(sd, h, p + "mid.block_2.")["out"]
    for lvl in reversed(range(len(mult))):
        for ib in range(nrb + 1):
            h = resnet_block(sd, h, f"{p}up.{lvl}.block.{ib}.")["out"]
        if lvl != 0:
            h = upsample(sd, h, f"{p}up.{lvl}.upsample.conv")
    return conv(gn(h, sd, p + "norm_out", True), sd, p + "conv_out", padding=1)


def encoder(sd, dd, x, p="encoder."):
    """Encoder.forward (model.py:519-543), fp64."""
    mult, nrb = list(dd["ch_mult"]), dd["num_res_blocks"]
    h = conv(x, sd, p + "conv_in", padding=1)
    for lvl in range(len(mult)):
        for ib in range(nrb):
            h = resnet_block(sd, h, f"{p}down.{lvl}.block.{ib}.")["out"]
        if lvl != len(mult) - 1:
            h = downsample(sd, h, f"{p}down.{lvl}.downsample.conv")
    h = resnet_block(sd, h, p + "mid.block_1.")["out"]
    h = attn_block(sd, h, p + "mid.attn_1.")["out"]
    h = resnet_block(sd, h, p + "mid.block_2.")["out"]
    return conv(gn(h, sd, p + "norm_out", True), sd, p + "conv_out", padding=1)


def vae_decode(sd, dd, z):
    return decoder(sd, dd, conv(z, sd, "post_quant_conv"))


def vae_encode_moments(sd, dd, x):
    return conv(encoder(sd, dd, x), sd, "quant_conv")


def vae_module(dd):
    """An AutoencoderKL (audioldm2_amd/vae.py) for ddconfig dd without its vocoder, on the CPU."""
    from audioldm2_amd.vae import AutoencoderKL
    return AutoencoderKL(ddconfig=dd, embed_dim=dd["z_channels"], image_key="stft")


def vae_state(dd, seed=0):
    """{name: fp32 tensor} of that module (oracle.weights: deterministic by parameter name)."""
    from oracle import weights
    return weights.make_state_dict(weights.shapes_of(vae_module(dd)), seed=seed)


def mel_for(dd, latent_shape, seed=0):
    """The mel [B, 1, T, F] whose encoding has the shape of the latent."""
    from oracle import cases
    f = 2 ** (len(dd["ch_mult"]) - 1)
    Bx, _, h, w = latent_shape
    assert w * f == dd["mel_bins"]
    return cases.mel_input(Bx, w * f, h * f, seed=seed).permute(0, 2, 1)[:, None].contiguous()


def double_state(sd):
    return {k: v.double() for k, v in sd.items()}


# ---- the fp16 image's format model ---------------------------------------------------------------------------------------------
def f16_image_bound(ref, scale):
    """|image - v| an fp16 (hi, lo) pair of scale * v allows: 2^-20 |v| + 2^-24 / scale (tests/test_f16x3_gpu.py)."""
    return ref.abs() * 2.0 ** -20 + 2.0 ** -24 / scale


def f16_scale_rule(gamma, beta, n):
    """The scale ops._norm_f16_scale documents: the largest power of two s with s (sqrt(n) max|gamma| + max|beta|) <= 32768."""
    bound = math.sqrt(float(n)) * float(gamma.abs().max()) + float(beta.abs().max())
    return 2.0 ** math.floor(math.log2(32768.0 / bound))
