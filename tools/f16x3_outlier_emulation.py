"""CPU model of the "f16x3" operand format on the inputs of tests/test_f16x3_outliers_gpu.py (no GPU needed).

For every op case of that file: the plain fp32 torch evaluation and the image-format model against fp64, whole tensor and
sub-block, as max|err| / max|ref|.  The model is hi = RN_f16(s x), lo = RN_f16(s x - hi), three products with exact (fp64)
accumulation, s from the same bound formulas as audioldm2_amd/ops.py — the guard of the GEGLU image included.  It models the
operand format only, not the kernels' fp32 accumulation: the kernels' real errors are somewhat higher.  The attention cases model
the K / V^T / q images and the output image; the softmax is exact.

  python tools/f16x3_outlier_emulation.py                 the table of model numbers
  python tools/f16x3_outlier_emulation.py --log ERRLOG    ... merged with a $ALDM_ERR_LOG of the GPU run: the rows of
                                                          profiles/r07_f16x3_outlier_errors.txt
"""
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_f16x3_outliers_gpu as T   # noqa: E402  (the input builders)

Fn = torch.nn.functional
from audioldm2_amd.ops import F16_GEGLU_MAX_SLACK_LOG2 as GEGLU_MAX_SLACK_LOG2   # noqa: E402


def pow2(b):
    return 2.0 ** math.floor(math.log2(32768.0 / b))


def split16(x, s):
    v = (x.double() * s).clamp(-65504, 65504)
    h = v.half()
    return h.double(), (v - h.double()).half().double()


def img(x, s):
    h, l = split16(x, s)
    return (h + l) / s


def mm3(a, sa, w, sw):
    """a [.., K] x w [N, K]: hi*hi + hi*lo + lo*hi, exact accumulation."""
    ah, al = split16(a, sa)
    wh, wl = split16(w, sw)
    return (ah @ wh.t() + ah @ wl.t() + al @ wh.t()) / (sa * sw)


def errs(got, ref, cols):
    e = (got.double() - ref).abs()
    return float(e.max() / ref.abs().max()), float(e[..., cols].max() / ref[..., cols].abs().max())


def norm_scale(ga, be, n):
    return pow2(math.sqrt(n) * float(ga.abs().max()) + float(be.abs().max()))


def ln_linear(K, N, M, which, k):
    x, ga, be, w, small = T.ln_linear_inputs(K, N, M, which, k)
    ref = Fn.layer_norm(x.double(), (K,), ga.double(), be.double(), 1e-5) @ w.double().t()
    a32 = Fn.layer_norm(x, (K,), ga, be, 1e-5)
    return errs(a32 @ w.t(), ref, small), errs(mm3(a32, norm_scale(ga, be, K), w, pow2(float(w.abs().max()))), ref, small), "f16"


def gn_conv(B, C1, C2, N, H, W, which, k):
    x, ga, be, w, small = T.gn_conv_inputs(B, C1, C2, N, H, W, which, k)
    C = C1 + C2
    a64 = Fn.silu(Fn.group_norm(x.double(), 32, ga.double(), be.double(), 1e-5))
    ref = Fn.conv2d(a64, w.double(), None, padding=1).permute(0, 2, 3, 1)
    a32 = Fn.silu(Fn.group_norm(x, 32, ga, be, 1e-5))
    y32 = Fn.conv2d(a32, w, None, padding=1).permute(0, 2, 3, 1)
    sa, sw = norm_scale(ga, be, (C // 32) * H * W), pow2(float(w.abs().max()))
    ah, al = split16(a32, sa)
    wh, wl = split16(w, sw)
    y16 = (Fn.conv2d(ah, wh, None, padding=1) + Fn.conv2d(ah, wl, None, padding=1) + Fn.conv2d(al, wh, None, padding=1)) / (sa * sw)
    return errs(y32, ref, small), errs(y16.permute(0, 2, 3, 1), ref, small), "f16"


def geglu_slack(C, ga, be, w, b, squared=False):
    """(bound, log2(bound / typical)) as Packed.geglu_bound computes them (squared: the former (R c + b)^2 of the joint maximum)."""
    rn = math.sqrt(C) * float(ga.abs().max()) + float(be.double().norm())
    rt = math.sqrt(float(ga.double().norm()) ** 2 + float(be.double().norm()) ** 2)
    cn = w.double().norm(dim=1)
    bound, typ = 1.0, 1.0
    for half in (slice(0, 4 * C), slice(4 * C, 8 * C)):
        bound *= rn * float(cn[half].max()) + float(b[half].abs().max())
        typ *= math.sqrt(rt * rt * float(cn[half].median()) ** 2 / C + float(b[half].double().pow(2).mean()))
    if squared:
        bound = (rn * float(cn.max()) + float(b.abs().max())) ** 2
    return bound, math.log2(bound / typ)


def geglu(C, M, which, k, squared=False):
    x, ga, be, w, b, w2, small = T.geglu_inputs(C, M, which, k)
    h = Fn.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5) @ w.double().t() + b.double()
    gg = h[..., :4 * C] * Fn.gelu(h[..., 4 * C:])
    ref = gg @ w2.double().t()
    gg32 = gg.float()
    bound, slack = geglu_slack(C, ga, be, w, b, squared)
    if slack <= GEGLU_MAX_SLACK_LOG2 or squared:
        y16, fmt = mm3(gg32, pow2(bound), w2, pow2(float(w2.abs().max()))), "f16"
    else:
        y16, fmt = gg32.double() @ w2.double().t(), "bf16x3"
    return errs(gg32 @ w2.t(), ref, small), errs(y16, ref, small), f"{fmt} k={slack:.1f}"


def attention(B, L, heads, which, k):
    C = heads * 32
    x, ga, be, wq, wk, wv, wo, bo, small_attn, small_out = T.attention_inputs(B, L, heads, which, k)
    xn = Fn.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    sh = lambda t: t.view(B, L, heads, 32).transpose(1, 2)
    us = lambda t: t.transpose(1, 2).reshape(B, L, C)
    q, kk, v = xn @ wq.double().t(), xn @ wk.double().t(), xn @ wv.double().t()
    ref = us(torch.softmax(sh(q) @ sh(kk).transpose(-1, -2) / math.sqrt(32.0), -1) @ sh(v))
    ref_o = ref @ wo.double().t() + bo.double()
    x32 = Fn.layer_norm(x, (C,), ga, be, 1e-5)
    q32, k32, v32 = x32 @ wq.t(), x32 @ wk.t(), x32 @ wv.t()
    a32 = us(Fn.scaled_dot_product_attention(sh(q32), sh(k32), sh(v32)))
    y32 = a32 @ wo.t() + bo
    rn = math.sqrt(C) * float(ga.abs().max()) + float(be.double().norm())
    bound = rn * float(torch.cat([wq, wk, wv], 0).double().norm(dim=1).max())
    s_kv, s_q = pow2(bound), pow2(bound * 32 ** -0.5 * T.LOG2E)
    sa, sw = norm_scale(ga, be, C), pow2(float(torch.cat([wq, wk, wv], 0).abs().max()))
    q16, k16, v16 = (mm3(x32, sa, w_, sw).float() for w_ in (wq, wk, wv))
    qi = img(q16 * (32 ** -0.5 * T.LOG2E), s_q) / (32 ** -0.5 * T.LOG2E)
    a16 = us(torch.softmax(sh(qi) @ sh(img(k16, s_kv)).transpose(-1, -2) / math.sqrt(32.0), -1) @ sh(img(v16, s_kv)))
    y16 = mm3(a16.float(), s_kv, wo, pow2(float(wo.abs().max()))) + bo.double()
    return (errs(a32, ref, small_attn), errs(y32, ref_o, small_out)), (errs(a16, ref, small_attn), errs(y16, ref_o, small_out)), "f16"


def cases():
    """(test name, pytest id without mode and form, fn, shape / outlier args)"""
    for which, k in [("gamma", 8), ("gamma", 12), ("beta", 8), ("beta", 12)]:
        for K, N, M in sorted({s[:3] for s in T._LN_SHAPES}):
            yield "test_layernorm_linear_with_an_outlier_channel", f"{which}-{k}-{K}-{N}-{M}", ln_linear, (K, N, M, which, k)
        for s in sorted({s[:6] for s in T._GN_SHAPES}):
            yield "test_groupnorm_silu_conv3x3_with_an_outlier_channel", f"{which}-{k}-" + "-".join(map(str, s)), gn_conv, (*s, which, k)
    for which in ("wrow", "wcol"):
        yield "test_linear_weight_with_an_outlier_row_or_column", which, ln_linear, (256, 256, 1024, which, 10)
        yield "test_conv3x3_weight_with_an_outlier_row_or_column", which, gn_conv, (2, 128, 0, 128, 32, 16, which, 10)
    for which, k in T._GEGLU_CASES:
        for C, M in ((256, 1024), (640, 256)):
            yield "test_layernorm_geglu_ff_out_with_an_outlier_row", f"{which}-{k}-{C}-{M}", geglu, (C, M, which, k)
    for which, k in [("wv_col", 10), ("wk_col", 6), ("x_row", 8)]:
        yield "test_layernorm_qkv_attention_to_out_with_an_outlier", f"{which}-{k}", attention, (2, 256, 8, which, k)


def main():
    log = {}
    if "--log" in sys.argv:
        for line in open(sys.argv[sys.argv.index("--log") + 1]):
            tid, what, mode, val, bar = line.rstrip("\n").split("\t")
            log.setdefault(tid.split("::")[-1], []).append((what, mode, float(val), float(bar)))
    if "--former-geglu-bound" in sys.argv:   # the discrimination figure: one gate row x 2^8 under (R c + b)^2
        for k in (4, 8, 12):
            e32, e16, fmt = geglu(256, 1024, "gate", k, squared=True)
            print(f"GEGLU gate x2^{k} C=256, former squared bound ({fmt}): whole {e16[0]:.2e} sub {e16[1]:.2e} (fp32: {e32[0]:.2e} {e32[1]:.2e})")
        return
    print("# test[id]\tmode\twhat\tGPU whole\tGPU sub\tbar\timage\t| model f16 whole\tsub\t| CPU fp32 whole\tsub")
    for name, pid, fn, args in cases():
        torch.manual_seed(0)
        e32, e16, fmt = fn(*args)
        pairs = [("attn", e32[0], e16[0]), ("to_out", e32[1], e16[1])] if fn is attention else \
            [("ff-out" if fn is geglu else "", e32, e16)]
        if not log:
            for what, a, b in pairs:
                print(f"{name}[{pid}]\t{what}\tmodel {fmt}: whole {b[0]:.2e} sub {b[1]:.2e}\t| fp32: whole {a[0]:.2e} sub {a[1]:.2e}")
            continue
        for tid, rows in sorted(log.items()):
            m = re.fullmatch(re.escape(name) + r"\[(f16x3|bf16x6)-(.*)\]", tid)
            if not m or not (m.group(2) == pid or m.group(2).startswith(pid + "-")):
                continue
            image = next((w for w, *_ in rows if w.startswith("image:")), "image:-")[6:]
            for what, a, b in pairs:
                wh = next(r for r in rows if r[0] == (what + " whole").strip())
                su = next(r for r in rows if r[0] == (what + " sub").strip())
                flag = "  MARGINAL" if su[2] * 1.25 > su[3] or wh[2] * 1.25 > wh[3] else ""
                print(f"{tid}\t{wh[1]}\t{what or '-'}\t{wh[2]:.2e}\t{su[2]:.2e}\t{su[3]:.1e}\t{image}\t| {b[0]:.2e}\t{b[1]:.2e}"
                      f"\t| {a[0]:.2e}\t{a[1]:.2e}{flag}")
    if log:
        for tid, rows in sorted(log.items()):
            if tid.startswith("test_unet"):
                for what, mode, val, bar in rows:
                    print(f"{tid}\t{mode}\t{what}\t{val:.2e}\t-\t{bar:.1e}\t-\t|\t\t|")


if __name__ == "__main__":
    main()
