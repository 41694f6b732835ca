"""Shapes, input recipes, deterministic weights and fp64 restatements of the launch forms the UNet issues (audioldm2_amd/unet.py):
the ResBlock chain with its timestep row bias and its skip concat, the symmetric-pad downsample, the nearest-x2 upsample, the
transformer block (self-attention, cross-attention on a masked context, GEGLU), the SpatialTransformer around it, the embedding
path and the end convs.  tests/test_unet_forms_cpu.py shows the restatements equal oracle.unet evaluated in double;
tests/test_unet_forms_gpu.py runs the launches against them.  Importable without a GPU: torch on the CPU only.

Every restatement is plain torch in fp64 on fp32 inputs, NCHW / [B, L, C] like the oracle, parameter prefixes end in a dot.  They
return every intermediate a launch of the module writes, so each launch can be held against fp64 of ITS OWN inputs.  What
tests/vae_forms.py already has (layout moves, the comparison, the trend input, the fp16 image's format model) is imported from there."""
import functools
import math
import zlib

import torch

import vae_forms as vf
from tolerances import F64 as F
# (re-exported: the tests of the UNet's forms reach these through this module)
from vae_forms import B, GROUPS, assert_close, cl, double_state, f16_image_bound, f16_scale_rule, gen, max_rel, uncl  # noqa: F401

EPS = 1e-5           # the GroupNorms of ResBlock and UNetModel.out (nn.GroupNorm's default)
ST_EPS = 1e-6        # SpatialTransformer.norm
LN_EPS = 1e-5
EMB = 512            # 4 * model_channels: the width of emb without FiLM
# pixel counts: 13 x 16 = 208 (fused GroupNorm; M = 416: no tile divides it, a row tile straddles the sample seam), 65 x 16 = 1040
# (chunked GroupNorm), 12 x 2 and 32 x 2 (the two-column maps of level 3: 12 x 2 = 24 tokens at a ragged duration)
HW_FUSED, HW_CHUNKED, HW_COL2, HW_COL2_LONG = (13, 16), (65, 16), (12, 2), (32, 2)
RES_PAIRS = [(128, 128), (128, 256), (256, 256), (384, 640), (640, 640)]
# (C1, C2, Cout, H, W); C2 = 0: no concat
RES_CASES = [(ci, 0, co) + HW_FUSED for ci, co in RES_PAIRS] + [(128, 0, 128) + HW_CHUNKED, (128, 0, 256) + HW_CHUNKED,
                                                                 (640, 0, 640) + HW_COL2, (384, 0, 640) + HW_COL2_LONG]
CONCAT_TRIPLES = [(640, 640, 640), (640, 384, 640), (640, 384, 384), (384, 256, 384), (384, 256, 256), (256, 128, 256), (256, 128, 128),
                  (128, 128, 128)]
SEAM_INSIDE_A_GROUP = [(384, 256), (256, 128)]     # Cg = 20: the seam at 19.2 groups; Cg = 12: at 21.33


def seam_inside_a_group(c1, c2):
    return c1 % ((c1 + c2) // GROUPS) != 0


RES_CONCAT_CASES = [t + HW_FUSED for t in CONCAT_TRIPLES] + \
    [t + HW_CHUNKED for t in CONCAT_TRIPLES if seam_inside_a_group(t[0], t[1]) or t[:2] == (128, 128)] + \
    [t + HW_COL2 for t in CONCAT_TRIPLES if t[:2] in ((640, 640), (640, 384))]
# the forced halo form runs whole 128-row tiles of one image, W a power of two: shapes of its own (as vae_forms.RES_HALO_CASES), the
# last two at the widths of levels 2 and 3, which tests/test_dma_gpu.py _HALO's (128, 128, 403) holds
RES_HALO_CASES = [(128, 0, 128, 16, 16), (128, 0, 256, 80, 16), (384, 0, 640, 64, 4), (640, 0, 640, 64, 2), (256, 128, 256, 16, 16),
                  (640, 640, 640, 64, 2)]
DOWN_CASES = [(128, 13, 16), (128, 8, 16), (256, 7, 8), (384, 12, 4)]     # (C, H, W): odd H / W: the padded last row / column is read
UP_CASES = [(640, 12, 2), (384, 6, 4), (256, 5, 8)]
TR_WIDTHS = [(128, 4), (256, 8), (384, 12), (640, 20)]                    # (C, heads)
TR_TOKENS = {24: HW_COL2, 64: HW_COL2_LONG, 208: HW_FUSED}                # L: less than one key tile, two, six and a half
# "none": the extra self-attention transformer (a context_dim=None block, attn2 = qkv2, and no context routed to it — the same form
# as the 48 kHz model's context_dim=[None]); "mae": [B, 8, 768]; "t5" / "t5_masked": [B, 21, 1024] under the two mask sets below
TR_CONTEXTS = ("none", "mae", "t5", "t5_masked")
CONTEXT_DIM = {"none": None, "mae": 768, "t5": 1024, "t5_masked": 1024}
T5_LEN, MAE_LEN = 21, 8
T5_REAL_KEYS = {"t5": (21, 7, 1), "t5_masked": (1, 0, 7)}                 # real keys per sample; 0: an all-masked sample
TR_CASES = [(c, h, L, ctx, B) for c, h in TR_WIDTHS for L in TR_TOKENS for ctx in TR_CONTEXTS] + \
    [(384, 12, 24, ctx, 3) for ctx in TR_CONTEXTS]
ST_CASES = [(128, 4, 1, 208, "none"), (256, 8, 2, 64, "mae"), (256, 8, 2, 24, "t5"), (384, 12, 1, 24, "t5_masked"), (640, 20, 1, 64, "mae"),
            (640, 20, 1, 24, "none")]                                     # (C, heads, depth, L, context)
TIMESTEPS = {2: [0, 999], 3: [1, 500, 981]}
FILM_DIM = 512
CONV_IN_CASES = [(8, 128) + HW_FUSED, (16, 128) + HW_FUSED]              # K = 72 / 144
CONV_OUT_CASES = [(128, n) + hw for n in (8, 16) for hw in (HW_FUSED, HW_CHUNKED)]
LATENT_TINY, LATENT_FILM_TINY = (2, 8, 12, 8), (2, 16, 12, 8)           # 96 and 24 tokens


def plan(P, C1, C2=0, want_split=False, batch=B):
    from audioldm2_amd import ops
    return ops.groupnorm_plan(batch, P, C1, C2, GROUPS, want_split)


# ---- weights and inputs ---------------------------------------------------------------------------------------------------------
def module_state(module, seed, prefix=""):
    """Deterministic weights of a product module by parameter name (oracle.weights); the gains and shifts of its GroupNorms and
    LayerNorms redrawn as N(0, 1) (either sign, widely different size: vae_forms._module_state), to_q / to_k scaled by 1.5 (scores of
    several units: the softmax is not near uniform and a wrong score moves the probabilities: vae_forms.attn_state)."""
    from oracle import weights
    sd = weights.make_state_dict(weights.shapes_of(module), seed=seed)
    for name, m in module.named_modules():
        if isinstance(m, (torch.nn.GroupNorm, torch.nn.LayerNorm)):
            for leaf in ("weight", "bias"):
                k = f"{name}.{leaf}" if name else leaf
                sd[k] = torch.randn(sd[k].shape, generator=gen(seed * 7919 + zlib.crc32(k.encode()) % 100003))
    for k in sd:
        if k.endswith(("to_q.weight", "to_k.weight")):
            sd[k] = sd[k] * 1.5
    return {prefix + k: v for k, v in sd.items()}


def load(module, sd):
    module.load_state_dict(sd, strict=True)
    return module.cuda().eval()


feature_input = vf.feature_input


def st_input(C, H, W, batch=B):
    """feature_input with every eighth group scaled by 2^-6: a variance near 1e-4 there, where eps = 1e-6 and eps = 1e-5 give
    different normalised values (about 4 %); at the variances of feature_input alone (0.02 .. 0.5) the two are 2e-4 apart."""
    x = feature_input(C, H, W, seed=3, batch=batch)
    gain = torch.ones(C)
    gain.view(GROUPS, -1)[::8] = 2.0 ** -6
    return x * gain[None, :, None, None]


def token_input(C, L, seed=0, batch=B):
    """h [B, L, C]: the trend recipe as tokens (non-zero mean, per-channel gains, a ramp along the tokens)."""
    return feature_input(C, L, 1, seed=seed, batch=batch).reshape(batch, C, L).permute(0, 2, 1).contiguous()


def emb_input(batch=B, width=EMB, seed=0):
    return torch.randn(batch, width, generator=gen(50 + seed)) * 2


def context_input(kind, batch=B, seed=0):
    """-> (context [B, Lk, D] or None, mask [B, Lk] of 0 / 1 or None)."""
    if kind == "none":
        return None, None
    if kind == "mae":
        return torch.randn(batch, MAE_LEN, 768, generator=gen(60 + seed)), None
    ctx = torch.randn(batch, T5_LEN, 1024, generator=gen(61 + seed))
    mask = torch.zeros(batch, T5_LEN)
    for b, n in enumerate(T5_REAL_KEYS[kind][:batch]):
        mask[b, :n] = 1
    return ctx, mask


def wide_rows(e, off, extra, seed=0):
    """[B, off + N + extra] row-bias buffer with e [B, N] at columns [off, off + N), N(0, 1) / 2 elsewhere: what UNetModel's batched
    emb_all projection looks like to one ResBlock.  -> (buffer, slice)."""
    Bx, N = e.shape
    buf = torch.randn(Bx, off + N + extra, generator=gen(70 + seed)) * 0.5
    buf[:, off:off + N] = e
    return buf, slice(off, off + N)


def shifted(sl, width):
    """The same view `width` columns on: the next ResBlock's slice."""
    return slice(sl.start + width, sl.stop + width)


# ---- fp64 restatements -----------------------------------------------------------------------------------------------------------
def silu(x):
    return x * torch.sigmoid(x)


def gn(x, sd, p, eps, act=False):
    y = F.group_norm(x, GROUPS, sd[p + ".weight"], sd[p + ".bias"], eps)
    return silu(y) if act else y


def ln(x, sd, p):
    return F.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], LN_EPS)


def conv(x, sd, p, stride=1, padding=0):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), stride=stride, padding=padding)


def lin(x, sd, p):
    return F.linear(x, sd[p + ".weight"], sd.get(p + ".bias"))


def concat(x, x2, swapped=False):
    if x2 is None:
        return x.double()
    return torch.cat([x2, x] if swapped else [x, x2], 1).double()


def row_bias(sd, emb, p=""):
    """This block's Linear(SiLU(emb)) [B, out_channels] (openaimodel.py:296)."""
    return lin(silu(emb.double()), sd, p + "emb_layers.1")


def resblock(sd, x, emb, x2=None, p="", swapped=False, e=None):
    """-> {raw, n1, skip, e, h, n2, out}: the concat image, SiLU(GroupNorm) of it, the (1x1) skip on it, the row bias, conv1 + row
    bias, SiLU(GroupNorm h), conv2 + skip.  swapped: the deliberately WRONG concat order [x2, x]; e: a row bias given from outside
    (the deliberately wrong one: another block's slice)."""
    r = {"raw": concat(x, x2, swapped)}
    r["n1"] = gn(r["raw"], sd, p + "in_layers.0", EPS, True)
    r["skip"] = conv(r["raw"], sd, p + "skip_connection") if (p + "skip_connection.weight") in sd else r["raw"]
    r["e"] = row_bias(sd, emb, p) if e is None else e.double()
    r["h"] = conv(r["n1"], sd, p + "in_layers.2", padding=1) + r["e"][:, :, None, None]
    r["n2"] = gn(r["h"], sd, p + "out_layers.0", EPS, True)
    r["out"] = conv(r["n2"], sd, p + "out_layers.3", padding=1) + r["skip"]
    return r


def downsample(sd, x, p="op"):
    """openaimodel.py:172: conv k3 s2 with padding 1 on every side."""
    return conv(x, sd, p, stride=2, padding=1)


def downsample_asymmetric(sd, x, p="op"):
    """A deliberately WRONG reference: the VAE's F.pad (0, 1, 0, 1) + conv k3 s2 p0."""
    return conv(F.pad(x.double(), (0, 1, 0, 1), mode="constant", value=0), sd, p, stride=2)


def upsample(sd, x, p="conv"):
    return conv(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), sd, p, padding=1)


def attention(q, k, v, heads, mask=None):
    """softmax(q k^T d^-0.5 [masked_fill -finfo.max]) v per head in fp64 (oracle/unet.py cross_attention: an all-masked sample is
    uniform over EVERY key).  q [B, L, C]; k, v [B, Lk, C]; mask [B, Lk], 1 = a real key."""
    Bx, L, C = q.shape
    d = C // heads
    sp = lambda t: t.double().reshape(Bx, -1, heads, d).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) * d ** -0.5
    if mask is not None:
        s = s.masked_fill(~(mask.reshape(Bx, 1, 1, -1) == 1), -torch.finfo(s.dtype).max)
    return (s.softmax(-1) @ sp(v)).transpose(1, 2).reshape(Bx, L, C)


def _cat_w(sd, p, names):
    return torch.cat([sd[f"{p}{n}.weight"] for n in names], 0)


def geglu(n3, sd, p):
    a, gate = lin(n3, sd, p + "ff.net.0.proj").chunk(2, dim=-1)
    return a * F.gelu(gate)


def transformer_block(sd, h, heads, context=None, mask=None, p="", use_mask=True):
    """-> {n1, qkv, a1, h1, n2, q2, kv, a2, h2, n3, g, out} (attention.py:400-410).  kv: the K | V projection of the context, or of
    n2 where attn2 runs as self-attention; the mask counts only with a context.  use_mask=False: the deliberately WRONG
    cross-attention that ignores the mask."""
    C = h.shape[-1]
    r = {"n1": ln(h, sd, p + "norm1")}
    r["qkv"] = F.linear(r["n1"], _cat_w(sd, p + "attn1.", ("to_q", "to_k", "to_v")))
    r["a1"] = attention(r["qkv"][..., :C], r["qkv"][..., C:2 * C], r["qkv"][..., 2 * C:], heads)
    r["h1"] = lin(r["a1"], sd, p + "attn1.to_out.0") + h.double()
    r["n2"] = ln(r["h1"], sd, p + "norm2")
    r["q2"] = F.linear(r["n2"], sd[p + "attn2.to_q.weight"])
    r["kv"] = F.linear(r["n2"] if context is None else context, _cat_w(sd, p + "attn2.", ("to_k", "to_v")))
    r["a2"] = attention(r["q2"], r["kv"][..., :C], r["kv"][..., C:], heads, mask if (context is not None and use_mask) else None)
    r["h2"] = lin(r["a2"], sd, p + "attn2.to_out.0") + r["h1"]
    r["n3"] = ln(r["h2"], sd, p + "norm3")
    r["g"] = geglu(r["n3"], sd, p)
    r["out"] = lin(r["g"], sd, p + "ff.net.2") + r["h2"]
    return r


def spatial_transformer(sd, x, heads, depth, context=None, mask=None, p="", eps=ST_EPS, use_mask=True):
    """-> {n, tokens, blocks: [transformer_block dicts], out} (attention.py:456-467).  eps=1e-5: the deliberately WRONG norm."""
    Bx, C, H, W = x.shape
    r = {"n": gn(x, sd, p + "norm", eps)}
    r["tokens"] = conv(r["n"], sd, p + "proj_in").permute(0, 2, 3, 1).reshape(Bx, H * W, -1)
    h, r["blocks"] = r["tokens"], []
    for d in range(depth):
        r["blocks"].append(transformer_block(sd, h, heads, context, mask, f"{p}transformer_blocks.{d}.", use_mask))
        h = r["blocks"][-1]["out"]
    r["out"] = conv(h.reshape(Bx, H, W, -1).permute(0, 3, 1, 2), sd, p + "proj_out") + x.double()
    return r


def timestep_embedding(t, dim, max_period=10000.0):
    """[cos | sin](t f_i), f_i = exp(-ln(max_period) i / half), everything in fp64 (util.py:172-196; dim even)."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], -1)


def embedding(sd, t, y=None, res_prefixes=(), p="", mc=128, t_emb=None):
    """-> {t_emb, h0 (SiLU(te0)), emb, emb_rows}: emb_rows [B, sum N] = every ResBlock's Linear(SiLU(emb)) side by side, in the order
    of res_prefixes (UNetModel._prepare's emb_all)."""
    r = {"t_emb": timestep_embedding(t, mc) if t_emb is None else t_emb.double()}
    r["h0"] = silu(lin(r["t_emb"], sd, p + "time_embed.0"))
    r["emb"] = lin(r["h0"], sd, p + "time_embed.2")
    if y is not None:
        r["emb"] = torch.cat([r["emb"], lin(y, sd, p + "film_emb")], -1)
    if res_prefixes:
        r["emb_rows"] = torch.cat([row_bias(sd, r["emb"], rp) for rp in res_prefixes], -1)
    return r


def out_conv(sd, x, p="out."):
    """-> {n, out}: SiLU(GroupNorm) and the conv of UNetModel.out."""
    n = gn(x, sd, p + "0", EPS, True)
    return {"n": n, "out": conv(n, sd, p + "2", padding=1)}


def res_prefixes(cfg, p=""):
    """The ResBlocks' parameter prefixes in module order: input blocks, middle block, output blocks."""
    from oracle.unet import unet_layout
    inp, mid, outb = unet_layout(cfg)
    names = [(f"{p}input_blocks.{i}.", blk) for i, blk in enumerate(inp)] + [(f"{p}middle_block.", mid)] + \
        [(f"{p}output_blocks.{i}.", blk) for i, blk in enumerate(outb)]
    return [f"{bp}{j}." for bp, blk in names for j, layer in enumerate(blk) if layer[0] == "res"]


def _run_block(sd, bp, blk, h, emb, ctxs, masks, x2=None):
    """TimestepEmbedSequential (openaimodel.py:81-103): the first transformer of a block gets no context, transformer k > 0 gets
    context k - 1, transformers beyond the list none."""
    ctxs, masks = [None] + list(ctxs), [None] + list(masks)
    st = 0
    for j, layer in enumerate(blk):
        lp = f"{bp}{j}."
        if layer[0] == "conv":
            h = conv(h, sd, lp[:-1], padding=1)
        elif layer[0] == "res":
            h, x2 = resblock(sd, h, emb, x2, lp)["out"], None
        elif layer[0] == "st":
            c, m = (ctxs[st], masks[st]) if st < len(ctxs) else (None, None)
            h = spatial_transformer(sd, h, layer[2], layer[5], c, m, lp)["out"]
            st += 1
        elif layer[0] == "down":
            h = downsample(sd, h, lp + "op")
        else:
            h = upsample(sd, h, lp + "conv")
    return h


def unet_forward(sd, cfg, x, t, context_list=None, mask_list=None, y=None, t_emb=None):
    """UNetModel.forward (openaimodel.py:837-885) out of the pieces above, fp64.  t_emb: the timestep embedding given from outside
    (the oracle evaluates it in fp32 whatever the dtype of the rest)."""
    from oracle.unet import unet_layout
    ctxs, masks = list(context_list or []), list(mask_list or [])
    inp, mid, outb = unet_layout(cfg)
    emb = embedding(sd, t, y if cfg.get("extra_film_condition_dim") is not None else None, mc=cfg["model_channels"], t_emb=t_emb)["emb"]
    h, hs = x.double(), []
    for i, blk in enumerate(inp):
        h = _run_block(sd, f"input_blocks.{i}.", blk, h, emb, ctxs, masks)
        hs.append(h)
    h = _run_block(sd, "middle_block.", mid, h, emb, ctxs, masks)
    for i, blk in enumerate(outb):
        h = _run_block(sd, f"output_blocks.{i}.", blk, h, emb, ctxs, masks, x2=hs.pop())
    return out_conv(sd, h)["out"]


# ---- the cases: computed once, shared by modes and paths, never modified --------------------------------------------------------------
ROW_OFFSET = 384     # columns in front of the block's slice of the wide row-bias buffer (three 128-wide blocks before it)


@functools.lru_cache(maxsize=None)
def res_case(c1, c2, co, H, W):
    """-> (state dict, x, x2 or None, wide row-bias buffer [B, 384 + 2 co + 128], the block's slice of it, fp64 restatement).  The
    row bias is Linear(SiLU(emb)) of an N(0, 1) x 2 emb, rounded to fp32: exactly what the kernel reads."""
    from audioldm2_amd.unet import ResBlock
    sd = module_state(ResBlock(c1 + c2, EMB, 0, out_channels=co), seed=c1 + 3 * c2 + co)
    x = feature_input(c1, H, W)
    x2 = feature_input(c2, H, W, seed=2) if c2 else None
    e = row_bias(sd, emb_input()).float()
    rows, sl = wide_rows(e, ROW_OFFSET, co + 128)
    return sd, x, x2, rows, sl, resblock(sd, x, None, x2, e=e)


@functools.lru_cache(maxsize=None)
def down_case(C, H, W):
    from audioldm2_amd.unet import Downsample
    sd = module_state(Downsample(C, True, out_channels=C), seed=C + H)
    x = feature_input(C, H, W)
    return sd, x, downsample(sd, x), downsample_asymmetric(sd, x)


@functools.lru_cache(maxsize=None)
def up_case(C, H, W):
    from audioldm2_amd.unet import Upsample
    sd = module_state(Upsample(C, True, out_channels=C), seed=C + H)
    x = feature_input(C, H, W)
    return sd, x, upsample(sd, x)


@functools.lru_cache(maxsize=None)
def tr_case(C, heads, L, ctx, batch=B):
    """-> (state dict, h [B, L, C], context, mask, fp64 restatement)."""
    from audioldm2_amd.unet import BasicTransformerBlock
    sd = module_state(BasicTransformerBlock(C, heads, 32, context_dim=CONTEXT_DIM[ctx]), seed=C + L)
    h = token_input(C, L, batch=batch)
    context, mask = context_input(ctx, batch)
    return sd, h, context, mask, transformer_block(sd, h, heads, context, mask)


@functools.lru_cache(maxsize=None)
def st_case(C, heads, depth, L, ctx):
    from audioldm2_amd.unet import SpatialTransformer
    H, W = TR_TOKENS[L]
    sd = module_state(SpatialTransformer(C, heads, 32, depth=depth, context_dim=CONTEXT_DIM[ctx]), seed=C + L + depth)
    x = st_input(C, H, W)
    context, mask = context_input(ctx)
    return sd, x, context, mask, spatial_transformer(sd, x, heads, depth, context, mask)
