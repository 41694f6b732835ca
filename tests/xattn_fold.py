"""Shared helpers of the folded cross-attention tests (test_xattn_fold_cpu.py / test_xattn_fold_gpu.py): deterministic inputs of one
cross-attention sublayer, its fp64 reference in the UNFOLDED form the reference model computes (LayerNorm -> to_q -> per-head
masked softmax -> . V -> to_out + bias + residual, attention.py:343-367 / :408), and the fp64 fold (include/aldm_hip.h)."""
import functools
import math

import torch

FLT_MAX = torch.finfo(torch.float32).max
MAX_KEYS = 8


def gen(seed):
    return torch.Generator().manual_seed(7000 + seed)


@functools.lru_cache(maxsize=None)
def case(B, L, C, Lk, seed=0, ctx_scale=1.0, h_mean=0.3, h_std=1.5):
    """Inputs of one sublayer.  A different context per sample; sample 0's context is all zeros (K = V = 0: no projection has a
    bias); sample 1 has its last two keys masked when Lk > 2; sample 2 has EVERY key masked.  kv is the fp32 K | V projection
    [B, Lk, 2C] both paths start from.  The tensors are shared between tests: do not modify them."""
    g = gen(seed)
    Dc = 48
    heads = C // 32
    h = torch.randn(B, L, C, generator=g) * h_std + h_mean
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    wq = torch.randn(C, C, generator=g) / math.sqrt(C)
    wkv = torch.randn(2 * C, Dc, generator=g) / math.sqrt(Dc)
    wout = torch.randn(C, C, generator=g) / math.sqrt(C)
    bout = 0.1 * torch.randn(C, generator=g)
    ctx = torch.randn(B, Lk, Dc, generator=g) * ctx_scale
    ctx[0] = 0.0
    mask = torch.ones(B, Lk)
    if B > 1 and Lk > 2:
        mask[1, -2:] = 0.0
    if B > 2:
        mask[2] = 0.0
    kv = (ctx.double() @ wkv.double().t()).float().contiguous()
    return dict(B=B, L=L, C=C, Lk=Lk, heads=heads, h=h, gamma=gamma, beta=beta, wq=wq, wout=wout, bout=bout, kv=kv, mask=mask)


def layernorm64(h, gamma, beta, eps=1e-5):
    x = h.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ref_unfolded(c, mask=True, normed=None, return_scores=False):
    """fp64, the order of operations of the reference model.  normed: the LayerNorm output to use instead of the fp64 one."""
    B, L, C, Lk, H = c["B"], c["L"], c["C"], c["Lk"], c["heads"]
    n = layernorm64(c["h"], c["gamma"], c["beta"]) if normed is None else normed.double()
    q = (n @ c["wq"].double().t()).view(B, L, H, 32)
    k = c["kv"][..., :C].double().view(B, Lk, H, 32)
    v = c["kv"][..., C:].double().view(B, Lk, H, 32)
    s = torch.einsum("blhd,bjhd->bhlj", q, k) / math.sqrt(32.0)
    smax = float(s.abs().max())
    if mask:
        s = s.masked_fill(~(c["mask"] == 1)[:, None, None, :], -FLT_MAX)
    a = torch.einsum("bhlj,bjhd->blhd", torch.softmax(s, -1), v).reshape(B, L, C)
    out = a @ c["wout"].double().t() + c["bout"].double() + c["h"].double()
    return (out, smax) if return_scores else out


def fold64(c):
    """Mq [B, C, heads * 8] (natural-log units: scale 32^-1/2 only) and Mo [B, heads * 8, C] in fp64; key columns >= Lk are zero."""
    B, C, Lk, H = c["B"], c["C"], c["Lk"], c["heads"]
    k = c["kv"][..., :C].double().view(B, Lk, H, 32)
    v = c["kv"][..., C:].double().view(B, Lk, H, 32)
    wq = c["wq"].double().view(H, 32, C)        # [head, d, c_in]
    wo = c["wout"].double().view(C, H, 32)      # [c_out, head, d]
    mq = torch.zeros(B, C, H, MAX_KEYS, dtype=torch.float64)
    mo = torch.zeros(B, H, MAX_KEYS, C, dtype=torch.float64)
    mq[..., :Lk] = torch.einsum("hdc,bjhd->bchj", wq, k) / math.sqrt(32.0)
    mo[:, :, :Lk] = torch.einsum("bjhd,chd->bhjc", v, wo)
    return mq.reshape(B, C, H * MAX_KEYS), mo.reshape(B, H * MAX_KEYS, C)


def ref_folded(c, mq, mo, mask=True):
    """fp64, the order of operations of the folded kernel: LayerNorm(h) Mq -> 8-wide softmax per head (padded keys weight 0) -> Mo."""
    B, L, C, Lk, H = c["B"], c["L"], c["C"], c["Lk"], c["heads"]
    n = layernorm64(c["h"], c["gamma"], c["beta"])
    s = (n @ mq).view(B, L, H, MAX_KEYS)
    if mask:
        keep = torch.ones(B, MAX_KEYS, dtype=torch.bool)
        keep[:, :Lk] = c["mask"] == 1
        s = s.masked_fill(~keep[:, None, None, :], -FLT_MAX)
    s[..., Lk:] = -math.inf
    p = torch.softmax(s, -1).reshape(B, L, H * MAX_KEYS)
    return p @ mo + c["bout"].double() + c["h"].double()


def max_rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())
