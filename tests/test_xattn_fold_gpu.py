"""Folded cross-attention on the GPU (csrc/xattn_fold.hip): the one-launch kernel against the fp64 reference of the UNFOLDED
sublayer, its launch forms, in-place refresh, and the UNet / DDIM graph cache with the fold on and off."""
import types

import pytest
import torch

import xattn_fold as xf
from oracle import cases, weights
from tolerances import fp32_grade, fused_tol, log_err, unet_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from audioldm2_amd import ops as o
    assert o.use_dma() and o.MMA_MODE != "f32" and o.XATTN_FOLD is True
    return o


def dev(c, *names):
    return [c[n].cuda() for n in names]


def run_folded(ops, c, out=None, fold=None):
    h, gamma, beta, bout, mask = dev(c, "h", "gamma", "beta", "bout", "mask")
    if fold is None:
        fold = ops.XattnFold(c["B"], c["C"], c["heads"], c["Lk"], "cuda").prepare(*dev(c, "kv", "wq", "wout"))
    return ops.xattn_folded(h, gamma, beta, fold, bout, mask=mask, out=out)


def run_unfolded(ops, c):
    """The library path the folded kernel replaces: layernorm -> linear -> attention -> linear (BasicTransformerBlock._attn2_unfolded)."""
    C = c["C"]
    h, gamma, beta, kv, mask = dev(c, "h", "gamma", "beta", "kv", "mask")
    n = ops.layernorm(h, gamma, beta, split_out="only")
    q = ops.linear(n, ops.pack_conv(c["wq"]))
    a = ops.attention(q, kv[:, :, :C], kv[:, :, C:], c["heads"], mask=mask, split_out="only")
    return ops.linear(a, ops.pack_conv(c["wout"], c["bout"]), res=h)


def _score_tol(fp32_grade, smax):
    """tests/test_dma_gpu.py's allowance, restated: what the rounding of a score of magnitude smax (natural units) costs the
    softmax, relative to max |out| — the 6-product form holds a dot product to ~2^-26 of its magnitude, 16-bit operands to ~2^-20."""
    return (2.0 ** -26 if fp32_grade else 2.0 ** -20) * smax * 1.4426950408889634


@pytest.mark.parametrize("Lk", [1, 5, 8])
@pytest.mark.parametrize("L", [32, 64, 96])
@pytest.mark.parametrize("C", [256, 384, 640])
def test_folded_and_unfolded_paths_match_fp64(ops, C, L, Lk):
    """One tile, two tiles and an odd number of 32-row tiles (at C = 256 the 64-row tile's half-empty tail); a zero context, two
    masked keys and an all-masked sample; h with mean 0.3 and std 1.5.  Both paths pass the same bar: they are interchangeable."""
    c = xf.case(3, L, C, Lk)
    ref = xf.ref_unfolded(c)
    bar = fused_tol()
    e_f = log_err(xf.max_rel(run_folded(ops, c), ref), bar, f"xattn_folded C={C} L={L} Lk={Lk} vs fp64 unfolded")
    e_u = log_err(xf.max_rel(run_unfolded(ops, c), ref), bar, f"unfolded library path C={C} L={L} Lk={Lk} vs fp64")
    print(f"xattn fold C={C} L={L} Lk={Lk}: folded {e_f:.2e}  unfolded {e_u:.2e}  bar {bar:.1e}")
    assert e_f < bar and e_u < bar, (e_f, e_u, bar)


def test_all_masked_sample_is_uniform_over_the_real_keys(ops):
    """Sample 2 (every key masked) with Lk = 5: the mean of the five value rows through to_out — padded key columns weigh 0."""
    c = xf.case(3, 32, 256, 5)
    C = c["C"]
    v = c["kv"][2, :, C:].double().mean(0)
    want = v @ c["wout"].double().t() + c["bout"].double() + c["h"][2].double()
    e = log_err(xf.max_rel(run_folded(ops, c)[2], want), fused_tol(), "xattn_folded all-masked row, Lk=5, vs mean of V")
    assert e < fused_tol(), e


@pytest.mark.parametrize("C,L", [(256, 96), (640, 64)])
def test_large_scores(ops, C, L):
    """Context x 8: scores of tens of nats.  Bar: fused_tol() + the score-rounding allowance at the largest |score|."""
    c = xf.case(3, L, C, 8, seed=1, ctx_scale=8.0)
    ref, smax = xf.ref_unfolded(c, return_scores=True)
    bar = fused_tol() + _score_tol(fp32_grade(), smax)
    e = log_err(xf.max_rel(run_folded(ops, c), ref), bar, f"xattn_folded context x 8 C={C} L={L} (max |score| {smax:.0f})")
    print(f"xattn fold large scores C={C}: {e:.2e}  max |score| {smax:.1f}  bar {bar:.2e}")
    assert smax > 20.0 and e < bar, (e, bar, smax)


def test_large_mean_rows(ops):
    """Rows with mean / std = 100: the LayerNorm allowance of tests/test_norm_forms_gpu.py — fp32 cannot hold 5e-6 of the spread
    at 100, so the yardstick is the same sublayer behind torch's own fp32 F.layer_norm on the CPU (everything after it in fp64),
    the bar the larger of fused_tol() and three times that figure."""
    c = xf.case(3, 64, 384, 8, seed=2, h_mean=100.0, h_std=1.0)
    ref = xf.ref_unfolded(c)
    n32 = torch.nn.functional.layer_norm(c["h"], (c["C"],), c["gamma"], c["beta"], 1e-5)
    yard = xf.max_rel(xf.ref_unfolded(c, normed=n32), ref)
    bar = max(fused_tol(), 3.0 * yard)
    e = log_err(xf.max_rel(run_folded(ops, c), ref), bar, "xattn_folded rows with mean/std = 100 vs fp64")
    log_err(yard, bar, "the sublayer behind torch fp32 F.layer_norm on the CPU, mean/std = 100, vs fp64 (yardstick)")
    print(f"xattn fold large mean: kernel {e:.2e}  yardstick {yard:.2e}  bar {bar:.2e}")
    assert e < bar, (e, yard, bar)


@pytest.mark.parametrize("B,L,C,form", [(3, 64, 640, "colsplit"), (2, 1024, 256, "rows64"), (3, 96, 256, "rows64"), (3, 32, 384, "rows32")])
def test_each_form_deterministic_and_inside_its_buffer(ops, B, L, C, form):
    """Each launch form, asserted through the planner: against fp64, two launches bitwise equal, and canary rows on both sides of
    `out` untouched (the 64-row tile of L = 96 has a half-empty tail)."""
    p = ops.xattn_fold_plan(B, L, C, C // 32, 8)
    assert p["supported"]
    if form == "colsplit":
        assert p["col_splits"] > 1 and p["tile_rows"] == 32 and p["waves"] == 8
    elif form == "rows64":
        assert p["tile_rows"] == 64
    else:
        assert p["tile_rows"] == 32 and p["col_splits"] >= 1
    c = xf.case(B, L, C, 8, seed=3)
    guard = 64
    big = torch.full((B * L + 2 * guard, C), 12345.678, device="cuda")
    out = big[guard:guard + B * L].view(B, L, C)
    run_folded(ops, c, out=out)
    first = out.clone()
    big[guard:guard + B * L].fill_(-1.0)
    run_folded(ops, c, out=out)
    assert torch.equal(first, out)
    assert bool((big[:guard] == 12345.678).all()) and bool((big[guard + B * L:] == 12345.678).all())
    e = log_err(xf.max_rel(out, xf.ref_unfolded(c)), fused_tol(), f"xattn_folded form {form} B={B} L={L} C={C} vs fp64")
    assert e < fused_tol(), e


def test_refresh_in_place_equals_a_fresh_prepare(ops):
    """prepare, run, overwrite the projection and the mask IN PLACE, prepare again into the same images, run: bitwise what a fresh
    XattnFold prepared from the new projection gives (what UNetModel.refresh_context_kv relies on)."""
    a, b = xf.case(3, 64, 384, 8, seed=4), xf.case(3, 64, 384, 8, seed=5)
    kv, wq, wout = dev(a, "kv", "wq", "wout")
    h, gamma, beta, bout, mask = dev(a, "h", "gamma", "beta", "bout", "mask")
    fold = ops.XattnFold(3, 384, 12, 8, "cuda").prepare(kv, wq, wout)
    ptrs = (fold.mq.data_ptr(), fold.mo.data_ptr())
    out_a = ops.xattn_folded(h, gamma, beta, fold, bout, mask=mask)
    kv.copy_(b["kv"])
    mask.copy_(torch.flip(a["mask"], (1,)))
    fold.prepare(kv, wq, wout)
    assert ptrs == (fold.mq.data_ptr(), fold.mo.data_ptr())
    out_b = ops.xattn_folded(h, gamma, beta, fold, bout, mask=mask)
    fresh = ops.XattnFold(3, 384, 12, 8, "cuda").prepare(b["kv"].cuda(), wq, wout)
    want = ops.xattn_folded(h, gamma, beta, fresh, bout, mask=torch.flip(a["mask"], (1,)).cuda())
    assert torch.equal(out_b, want) and not torch.equal(out_a, out_b)


def test_wrapper_refuses_what_the_kernel_does_not_support(ops):
    c = xf.case(3, 32, 256, 8)
    fold = ops.XattnFold(3, 256, 8, 8, "cuda").prepare(*dev(c, "kv", "wq", "wout"))
    h, gamma, beta, bout = dev(c, "h", "gamma", "beta", "bout")
    with pytest.raises(AssertionError):
        ops.xattn_folded(h, gamma, beta, fold, bout, out=h)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.xattn_folded(h[:, :24].contiguous(), gamma, beta, fold, bout)


# ---- the UNet and the sampler ---------------------------------------------------------------------------------------------------
# Two levels, attention at both, context_dim [768, 1024], a 16 x 8 latent: C = 128 at 128 tokens (64-row tiles), C = 256 at 32
# tokens (one 32-row tile); contexts of 8 keys (folded) and 32 keys (never folded).  model_channels is 128, the narrowest this
# library runs: its GroupNorm(32) kernels need four channels per group.
UNET_FOLD = dict(cases.UNET_TINY)
SHAPE = (2, 8, 16, 8)
DDIM_S = 4   # "uniform" spacing over 1000 training steps: S = 3 would index step 1000; 4 gives an eager step, the capture, replays


class FoldModel:
    """What a sampler touches on its model, over a two-level UNet reachable as .model.diffusion_model (the graph cache lives there)."""
    num_timesteps = 1000

    def __init__(self):
        from audioldm2_amd.unet import UNetModel
        self.unet = UNetModel(**UNET_FOLD)
        self.unet.load_state_dict(weights.make_state_dict(weights.shapes_of(self.unet), seed=0))
        self.unet.cuda()
        self.model = types.SimpleNamespace(diffusion_model=self.unet)
        betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()

    def apply_model(self, x, t, cond):
        return self.unet(x.contiguous(), t, context_list=cond[0], context_attn_mask_list=cond[1])

    def prepare_cfg(self, cond, uncond):
        return {"ctxs": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[0], cond[0])],
                "masks": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[1], cond[1])], "y": None}

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        p = prepared or self.prepare_cfg(cond, uncond)
        eps = self.unet(x.repeat(2, 1, 1, 1).contiguous(), t2, context_list=p["ctxs"], context_attn_mask_list=p["masks"])
        return eps.view(2, x.shape[0], *eps.shape[1:])


def conditioning(seed):
    _, _, ctxs, masks, _ = cases.unet_inputs(UNET_FOLD, SHAPE[0], 16, 8, 32, seed=seed)
    masks[0][1, -3:] = 0   # the AudioMAE context with masked keys too
    return [c.cuda() for c in ctxs], [m.cuda() for m in masks]


@pytest.fixture(scope="module")
def model():
    return FoldModel()


def folds_of(unet):
    from audioldm2_amd.unet import BasicTransformerBlock
    return [c[3] for m in unet.modules() if isinstance(m, BasicTransformerBlock) for c in (m._kv or ())]


def test_unet_fold_on_equals_fold_off(ops, model):
    """The two-level UNet with contexts of 8 keys (folded at both widths) and 32 keys (never folded): on against off within
    unet_tol(), and the folded images exist exactly when the switch is on."""
    x, t, _, _, _ = cases.unet_inputs(UNET_FOLD, SHAPE[0], 16, 8, 32, seed=1)
    ctxs, masks = conditioning(1)
    assert [c.shape[1] for c in ctxs] == [8, 32]
    unet = model.unet
    unet.drop_step_caches()
    on = unet(x.cuda(), t.cuda(), context_list=ctxs, context_attn_mask_list=masks)
    got = folds_of(unet)
    assert sum(f is not None for f in got) == sum(f is None for f in got) > 0   # every block pair: AudioMAE folded, FLAN-T5 not
    assert {f.C for f in got if f is not None} == {128, 256}
    prev = ops.xattn_fold(False)
    try:
        unet.drop_step_caches()
        off = unet(x.cuda(), t.cuda(), context_list=ctxs, context_attn_mask_list=masks)
        assert all(f is None for f in folds_of(unet))
    finally:
        ops.xattn_fold(prev)
        unet.drop_step_caches()
    e = log_err(xf.max_rel(on, off), unet_tol(), "two-level UNet, folded cross-attention on vs off")
    print(f"xattn fold UNet on vs off: {e:.2e}  bar {unet_tol():.1e}")
    assert 0.0 < e < unet_tol(), e


def test_second_job_on_the_cached_graph_equals_a_fresh_sampler(ops, model):
    """A short DDIM run (DDIM_S steps) through the graph cache, then new conditioning on the cached graph (contexts copied in, K / V and the
    folded images refreshed in place): bitwise the run of a sampler with nothing cached."""
    from audioldm2_amd.ddim import DDIMSampler
    unet = model.unet

    def job(seed):
        cond, uncond = conditioning(seed), conditioning(seed + 10)
        xT = torch.randn(SHAPE, generator=torch.Generator().manual_seed(3))
        return DDIMSampler(model).sample(DDIM_S, SHAPE[0], SHAPE[1:], cond, verbose=False, x_T=xT, eta=0.0,
                                         unconditional_guidance_scale=3.5, unconditional_conditioning=uncond)[0]
    unet.drop_step_caches()
    first = job(1)
    assert len(unet._graph_cache) == 1
    ent = next(iter(unet._graph_cache.values()))
    assert any(e[3] is not None for e in ent["kv"]) and any(e[3] is None for e in ent["kv"])
    second_hit = job(2)
    assert next(iter(unet._graph_cache.values())) is ent
    unet.drop_step_caches()
    second_fresh = job(2)
    unet.drop_step_caches()
    assert torch.equal(second_hit, second_fresh) and not torch.equal(first, second_hit)
    assert bool(torch.isfinite(second_hit).all())
