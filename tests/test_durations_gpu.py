"""Durations other than 10 s on the MI355X: the pre-split self-attention (ALDM_EPI_QKV + aldm_attention_d32_presplit{,_f16}) over
token counts that are not a multiple of 32 — a partial last key tile (ABI v10: attention_d32_presplit2_kernel<..., TAIL> and
aldm_vt_regroup) — from the op up to the UNet and the DDIM sampler of both models that accept other durations (audioldm_48k,
audioldm_16k_crossattn_t5)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, weights
from tolerances import fused_tol, log_err, unet_tol

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LS = [2, 16, 24, 48, 80, 100]


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module", params=["bf16x6", "bf16x3"])
def ops(request):
    from audioldm2_amd import ops as o
    prev = o.set_mma(request.param)
    yield o
    o.set_mma(prev)


# the QKV projection's two epilogue families: igemm_epilogue.h (igemm_dma_kernel, 64 x 128 tile) and the operand-stationary
# kernel's (igemm_dma_os.h); None = whatever the tuner picks
FAMILIES = {"auto": None, "classic": (64, 128, 2), "os": (32, 128, 302)}


def _forced(ops, fam, fn):
    f = FAMILIES[fam]
    if f is not None:
        ops.igemm_force(f[0], f[1], 1, 0, f[2])
    try:
        return fn()
    finally:
        if f is not None:
            ops.igemm_force(0, 0, 0)


@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", LS)
def test_ragged_presplit_attention_is_bitwise_the_fp32_kv_path(ops, L, B, fam):
    """ALDM_EPI_QKV + aldm_attention_d32_presplit at L % 32 != 0 (and the aligned neighbours) against the fp32-K/V path: the fp32
    kernel masks the keys past L of its ragged last tile with -inf and multiplies clamped (finite) V rows by p = 0; the TAIL kernel
    masks the same scores and zeroes those V^T elements — the same products in the same order, so BIT-identical outputs; and
    both within the fp64 bar.  (aldm_vt_regroup zero-fills the last tile's V^T past L, so the kernel's own in-register zeroing of
    those elements is not what these outputs depend on: it guards images written otherwise and is not exercised here.)"""
    heads = 8   # C = 256: the operand-stationary kernel's QKV form needs K = 256 (and qkv_c % 128 == 0)
    C = heads * 32
    x = torch.randn(B, L, C, generator=g(1))
    wq, wk, wv = (torch.randn(C, C, generator=g(2 + i)) / math.sqrt(C) for i in range(3))
    pw = ops.pack_conv(torch.cat([wq, wk, wv], 0))
    xs = ops.split_rows(x.cuda())
    qkv = _forced(ops, fam, lambda: ops.linear(xs, pw))
    a_old, s_old = ops.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], heads, split_out="also")
    q, kimg, vtimg = _forced(ops, fam, lambda: ops.linear_qkv(xs, pw, heads, L))
    assert vtimg.shape[2] == -(-L // 32)
    assert torch.equal(q, qkv[:, :, :C].contiguous())
    assert torch.equal(kimg.reshape(-1), ops.split_rows(qkv[:, :, C:2 * C].contiguous()).data.view(-1))
    a_new, s_new = ops.attention_presplit(q, kimg, vtimg, heads, split_out="also")
    assert torch.isfinite(a_new).all()
    assert torch.equal(a_new, a_old) and torch.equal(s_new.data, s_old.data)
    xd = xs.float().double().cpu()
    sh = lambda t: t.view(B, L, heads, 32).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sh(xd @ wq.double().t()), sh(xd @ wk.double().t()), sh(xd @ wv.double().t()))
    assert rel_err(a_new, ref.transpose(1, 2).reshape(B, L, C)) < fused_tol()


@pytest.fixture(scope="module")
def ops16():
    from audioldm2_amd import ops as o
    prev = o.set_mma("f16x3")
    yield o
    o.set_mma(prev)


@pytest.mark.parametrize("fam", ["auto", "os"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", LS)
def test_ragged_presplit_attention_f16x3(ops16, L, B, fam):
    """The "f16x3" form (fp16 K / V^T images, three products, integer softmax reference) at any L: the keys past L neither enter
    the reference nor the sum (a masked key that moved the reference would still cancel — but one that entered the sum would not);
    LayerNorm-fed like the UNet, within the f16x3 bar of fp64."""
    ops = ops16
    heads = 8   # C = 256: the operand-stationary kernel's QKV form needs K = 256 (and qkv_c % 128 == 0)
    C = heads * 32
    x = torch.randn(B, L, C, generator=g(1))
    ga, be = torch.randn(C, generator=g(2)) * 0.3 + 1.0, torch.randn(C, generator=g(3)) * 0.1
    wq, wk, wv = (torch.randn(C, C, generator=g(4 + i)) / math.sqrt(C) for i in range(3))
    pw = ops.pack_conv(torch.cat([wq, wk, wv], 0))
    n = ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), 1e-5, split_out="only")
    q, kimg, vtimg = _forced(ops, fam, lambda: ops.linear_qkv(n, pw, heads, L))
    assert kimg.shape[2] == 2 and getattr(kimg, "_aldm_f16", None) is not None   # the fp16 images: the F16 TAIL kernel ran
    a = ops.attention_presplit(q, kimg, vtimg, heads)
    xn = F.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    sh = lambda t: t.view(B, L, heads, 32).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sh(xn @ wq.double().t()), sh(xn @ wk.double().t()), sh(xn @ wv.double().t()))
    assert torch.isfinite(a).all()
    assert rel_err(a, ref.transpose(1, 2).reshape(B, L, C)) < fused_tol("f16x3")


def _unet_cfg(model_name):
    from audioldm2_amd.pipeline import default_audioldm_config
    p = default_audioldm_config(model_name)["model"]["params"]
    return p["unet_config"]["params"], p["latent_f_size"]


def test_unet_at_a_ragged_duration_routes_every_self_attention_to_the_presplit_kernel(monkeypatch):
    """audioldm_48k at 7.5 s (latent_t = 96): the deepest transformer sees 12 x 4 = 48 tokens.  Every self-attention (48k has no
    cross-attention context: attn2 runs as self-attention too) goes through ops.attention_presplit, none through the fp32-K/V
    ops.attention fallback."""
    from audioldm2_amd import ops
    from audioldm2_amd.unet import UNetModel
    cfg, F_ = _unet_cfg("audioldm_48k")
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    x, t, ctxs, masks, y = cases.unet_inputs(cfg, 2, 96, F_)
    calls = {"pre": [], "fp32": 0}
    pre, plain = ops.attention_presplit, ops.attention

    def count_pre(q, k_img, vt_img, heads, **kw):
        calls["pre"].append(q.shape[1])
        return pre(q, k_img, vt_img, heads, **kw)

    def count_plain(*a, **kw):
        calls["fp32"] += 1
        return plain(*a, **kw)
    monkeypatch.setattr(ops, "attention_presplit", count_pre)
    monkeypatch.setattr(ops, "attention", count_plain)
    assert not ctxs and y is not None
    out = m(x.cuda(), t.cuda(), y=y.cuda(), context_list=[], context_attn_mask_list=[])
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert calls["fp32"] == 0
    assert 48 in calls["pre"] and len(calls["pre"]) >= 2


@pytest.mark.parametrize("model_name,T", [("audioldm_48k", 64), ("audioldm_48k", 96), ("audioldm_48k", 160),
                                          ("audioldm_16k_crossattn_t5", 64), ("audioldm_16k_crossattn_t5", 96),
                                          ("audioldm_16k_crossattn_t5", 160)])
def test_unet_forward_at_other_durations_matches_the_fp64_oracle(model_name, T):
    """The full-size UNet of both duration-capable models at 5 s / 7.5 s / 12.5 s (48k: 64 / 96 / 160 latent frames; t5: the same
    latent_t at 25.6 frames per second) against oracle/unet.py in fp64."""
    from audioldm2_amd.unet import UNetModel
    from oracle.unet import unet_forward
    cfg, F_ = _unet_cfg(model_name)
    m = UNetModel(**cfg)
    sd = weights.make_state_dict(weights.shapes_of(m), seed=0)
    m.load_state_dict(sd)
    x, t, ctxs, masks, y = cases.unet_inputs(cfg, 1, T, F_, 12)
    out = m(x.cuda(), t.cuda(), y=None if y is None else y.cuda(), context_list=[c.cuda() for c in ctxs],
            context_attn_mask_list=[k.cuda() for k in masks])
    ref = unet_forward(sd, cfg, x, t, ctxs, masks, y=y)
    assert log_err(rel_err(out, ref), unet_tol(), f"{model_name} latent_t {T}") < unet_tol()


@pytest.mark.parametrize("model_name,T", [("audioldm_48k", 96), ("audioldm_16k_crossattn_t5", 192)])
def test_generate_batch_at_a_ragged_duration_replays_a_captured_graph(model_name, T):
    """generate_batch at 7.5 s: the DDIM stepper captures the new geometry into a HIP graph and replays it (no eager fall-back after
    a refused capture), and the waveform has the duration's length."""
    from audioldm2_amd.pipeline import build_model, make_batch_for_text_to_audio, seed_everything
    ld = build_model(model_name=model_name)
    ld.latent_t_size = T
    seed_everything(42)
    w = ld.generate_batch(make_batch_for_text_to_audio("a dog barking", batchsize=2), ddim_steps=4,
                          unconditional_guidance_scale=3.5)
    # (the mel has 4 frames per latent frame, 1024 per 10.24 s: a latent_t of 7.5 s is 7.68 s of audio, as in the reference)
    assert w.shape[0] == 2 and abs(w.shape[-1] - 7.68 * ld.sampling_rate) <= 0.005 * ld.sampling_rate
    assert torch.isfinite(torch.as_tensor(w)).all()
    cache = ld.model.diffusion_model._graph_cache
    ents = [e for e in cache.values() if isinstance(e, dict) and "run_step" in e]
    assert ents and all(e["run_step"].use_graph and e["run_step"].graph is not None for e in ents)
    assert any(k[0][-2] == T for k in cache if isinstance(k, tuple))


# ---- end to end against the REAL reference (tools/make_golden_durations.py) --------------------------------------------------
# job -> (model name, keys fixture, latent_t, duration, fixture, ragged: some self-attention has a partial last key tile)
E2E = {"t5_256": ("audioldm_16k_crossattn_t5", "e2et5_statedict_keys.json", 256, 10.0, "e2e_dur_t5_256", False),
       "t5_192": ("audioldm_16k_crossattn_t5", "e2et5_statedict_keys.json", 192, 7.5, "e2e_dur_t5_192", True),
       "48k_96": ("audioldm_48k", "e2e48k_statedict_keys.json", 96, 7.5, "e2e_dur_48k_96", True),
       "48k_64": ("audioldm_48k", "e2e48k_statedict_keys.json", 64, 5.0, "e2e_dur_48k_64", False)}


def _rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt((a ** 2).mean()))


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3", "f16x3"])
@pytest.mark.parametrize("job", list(E2E))
def test_generate_batch_at_other_durations_matches_the_reference(job, mode):
    """The reference's generate_batch (B = 2, 5 DDIM steps, CFG 3.5, seed 42, random-init weights) of the t5 model at 10 s / 7.5 s
    and of audioldm_48k at 7.5 s / 5 s: latent within the per-mode bar, waveform error below 1e-3 and below 1e-3 of the distance
    between the two samples' waveforms (as tests/test_parity_configs_gpu.py); at a ragged duration the DDIM stepper replayed a
    captured graph."""
    from audioldm2_amd import ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from tolerances import latent_tol
    model_name, keys_json, T, dur, fixture, ragged = E2E[job]
    gd = np.load(os.path.join(GOLD, fixture + ".npz"))
    prev = ops.set_mma(mode)
    try:
        m = build_model(model_name=model_name)
        with open(os.path.join(GOLD, keys_json)) as f:
            shapes = {k: tuple(v) for k, v in json.load(f).items()}
        sd = weights.make_state_dict(shapes, seed=0)
        sd["scale_factor"] = torch.tensor(cases.SCALE_FACTOR)
        m.load_state_dict(sd, strict=False)
        m = m.cuda()
        rec = {}
        orig = m.decode_first_stage_cl

        def hook(z):
            rec["latent"] = z.clone()
            return orig(z)
        m.decode_first_stage_cl = hook
        batch = cases.e2e_batch_48k(2) if "48k" in model_name else cases.e2e_batch(2)
        seed_everything(cases.E2E_SEED)
        m.latent_t_size = T
        wave = m.generate_batch(batch, unconditional_guidance_scale=3.5, ddim_steps=5, n_gen=1, duration=dur)
        assert wave.shape == (2, 1, int(gd["wave_len"]))
        el = _rms(rec["latent"].double().cpu().numpy() - gd["latent"]) / _rms(gd["latent"])
        eh = _rms(wave[..., :32768].astype(np.float64) - gd["wave_head"])
        ed = _rms(wave[..., ::16].astype(np.float64) - gd["wave_dec"])
        between = float(gd["wave_between_rms"])
        print(f"{job} [{mode}]: latent rel rms {el:.2e}  wave rms_err {max(eh, ed):.3e}  between-sample {between:.3e}")
        assert log_err(el, latent_tol(5, mode), f"{job} latent [{mode}]") < latent_tol(5, mode)
        assert between > 1e-2 and max(eh, ed) < 1e-3 and max(eh, ed) < 1e-3 * between
        if ragged:
            ents = [e for e in m.model.diffusion_model._graph_cache.values() if isinstance(e, dict) and "run_step" in e]
            assert ents and all(e["run_step"].use_graph and e["run_step"].graph is not None for e in ents)
        del m
        torch.cuda.empty_cache()
    finally:
        ops.set_mma(prev)


def test_candidate_reranking_at_5_s_picks_what_the_oracle_picks():
    """n_candidate_gen_per_text = 2 on audioldm_48k at 5 s (latent_t 64: 5.12 s of 48 kHz audio, not the 10.24 s the HTSAT front
    end was built around, so its bicubic patchify path, htsat.py:1074-1089, runs): the HIP re-ranker's similarities and chosen
    candidates are the CPU oracle's (oracle HTSAT + CLAP text) on the same candidate waveforms — tests/test_htsat.py's 10 s check
    at another duration."""
    from audioldm2_amd.clap import CLAPAudioEmbeddingClassifierFreev2
    from audioldm2_amd.pipeline import build_model, make_batch_for_text_to_audio, seed_everything
    from oracle import clap_text
    from oracle import htsat as oh
    from test_htsat import _StubTokenizer, _sd, cases_text_sd
    torch.manual_seed(3)
    m = build_model(model_name="audioldm_48k").cuda()
    clap = CLAPAudioEmbeddingClassifierFreev2(embed_mode="audio", unconditional_prob=0.0, sampling_rate=48000,
                                              config=cases.clap_text_test_config(), audio_config=cases.htsat_test_config())
    sd, _ = _sd()
    tsd = cases_text_sd()
    clap.model.load_state_dict({**sd, **tsd}, strict=False)
    clap.tokenize = _StubTokenizer()
    m.clap = clap
    seen = {}
    orig = clap.cos_similarity

    def spy(waveform, text):
        seen["waveform"], seen["text"] = waveform.clone(), list(text)
        return orig(waveform, text)
    clap.cos_similarity = spy
    B0 = 2
    batch = make_batch_for_text_to_audio("a dog barking in the rain", batchsize=B0)
    batch["text"][1] = "a slow piano melody"
    batch["log_mel_spec"] = torch.zeros((B0, 1024, 256))
    seed_everything(7)
    m.latent_t_size = 64
    wav = m.generate_batch(batch, unconditional_guidance_scale=3.5, ddim_steps=2, n_gen=2, duration=5)
    n = wav.shape[-1]
    assert wav.shape[:2] == (B0, 1) and abs(n - 5.12 * 48000) <= 0.005 * 48000 and np.isfinite(wav).all()
    cand = seen["waveform"]
    assert tuple(cand.shape) == (2 * B0, n) and seen["text"] == batch["text"] * 2
    tok = _StubTokenizer()(seen["text"])
    a = oh.audio_embedding(sd, cand.float(), 48000, cases.htsat_test_config())
    t = clap_text.text_embedding(tsd, cases.clap_text_test_config(), tok["input_ids"], tok["attention_mask"])
    want = oh.cos_similarity(a, t)
    assert torch.allclose(m.last_similarity, want, atol=5e-5), (m.last_similarity, want)
    best = [i + int(torch.argmax(want[i::B0])) * B0 for i in range(B0)]
    assert m.last_best_index == best
    assert np.array_equal(wav[:, 0], cand.numpy()[best])
