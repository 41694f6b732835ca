"""The oracle restatement against the REAL reference classes on inputs that are NOT in the other fixtures: other weights,
shapes and seeds.  What the reference computed on them, and the state-dict shapes its classes hold, were recorded by
`python -m oracle.make_golden crosscheck` (tests/golden/crosscheck.npz); the oracle runs live.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, weights
from oracle.unet import unet_forward
from oracle.vae import hifigan_forward, vae_decode, vae_encode_moments

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "crosscheck.npz"))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _shapes(g, key):
    return {k: tuple(v) for k, v in json.loads(g[key + "_shapes"].tobytes().decode()).items()}


@pytest.mark.parametrize("cfg,B,H,W,t5,seed", cases.UNET_CROSSCHECK)
def test_unet_oracle_equals_live_reference(g, cfg, B, H, W, t5, seed):
    """openaimodel.UNetModel.forward (openaimodel.py:837-885) on fresh weights / shapes / seeds."""
    case = cases.UNET_CROSSCHECK.index((cfg, B, H, W, t5, seed))
    sd = weights.make_state_dict(_shapes(g, f"unet{case}"), seed=seed)
    x, t, ctxs, masks, y = cases.unet_inputs(cfg, B, H, W, max(t5, 1), seed=seed)
    with torch.no_grad():
        got = unet_forward(sd, cfg, x, t, ctxs, masks, y=y)
    assert rel(got, g[f"unet{case}"]) < 1e-5


def test_vae_oracle_equals_live_reference(g):
    """AutoencoderKL.decode / .encode (autoencoder.py:103-117) for the 16 kHz ddconfig."""
    dd = cases.DDCONFIG_16K
    sd = weights.make_state_dict(_shapes(g, "vae"), seed=21)
    z = cases.latent_input(1, 8, 12, 16, seed=21)
    x = cases.mel_input(1, 64, 64, seed=22).permute(0, 2, 1)[:, None]
    with torch.no_grad():
        assert rel(vae_decode(sd, dd, z), g["vae_decode"]) < 1e-5
        assert rel(vae_encode_moments(sd, dd, x), g["vae_moments"]) < 1e-5


def test_hifigan_oracle_equals_live_reference(g):
    """hifigan.Generator.forward (hifigan/models.py:149-165), 16 kHz config."""
    sd = weights.make_state_dict(_shapes(g, "hifigan"), seed=31)
    mel = cases.mel_input(2, 64, 12, seed=31)
    with torch.no_grad():
        assert rel(hifigan_forward(sd, cases.HIFIGAN_16K, mel), g["hifigan"]) < 1e-5


def test_audio_front_end_helpers_equal_live_reference(g):
    """pad_wav / normalize_wav / _pad_spec of the inpainting front-end (utilities/audio/tools.py:9-25,71-84)
    — host helpers of audioldm2_amd.pipeline — against the reference's own functions."""
    from audioldm2_amd import pipeline as P
    rng = np.random.default_rng(0)
    w = rng.standard_normal(500).astype(np.float32) * 0.3 + 0.1
    assert np.array_equal(P.normalize_wav(w), g["normalize_wav"])
    for seg in (None, 500, 800):
        assert np.array_equal(P.pad_wav(w[None], seg), g[f"pad_wav_{seg}"])
    fb = torch.randn(20, 65, generator=torch.Generator().manual_seed(0))   # pad to 24, crop to 16, odd bin dropped
    for tl in (24, 16):
        assert torch.equal(P._pad_spec(fb, tl), torch.from_numpy(g[f"pad_spec_{tl}"]))


def test_sequence_generator_oracle_equals_live_reference(g):
    """§8(f) rank 1: Sequence2AudioMAE.generate (sequence_input.py:294-325) on conditioning that is not in the other
    fixtures (other batch, lengths, seed), full re-forward and key/value-cached restatements."""
    from oracle import seqgen
    cfg = dict(cases.SEQGEN_FULL, steps=5)
    sd = weights.make_state_dict(_shapes(g, "seqgen"), seed=3)
    cond = cases.seqgen_cond(cfg, 2, 9, seed=21)
    want = g["seqgen"]
    x, mask = seqgen.input_sequence_and_mask(sd, cond, cfg["keys"], cfg["steps"])
    assert rel(seqgen.generate_full(sd, x, mask, cfg["steps"]), want) < 1e-5
    assert rel(seqgen.generate_cached(sd, x, mask, cfg["steps"]), want) < 1e-5


def test_htsat_oracle_equals_live_reference(g):
    """§8(f) rank 4: HTSAT_Swin_Transformer.forward(...)["embedding"] (clap/open_clip/htsat.py:1092-1127) on audio that is not
    in the other fixtures — other weights, one sample, a 6 s clip (601 frames: the bicubic stretch of reshape_wav2img runs
    at a different ratio) — with depths (1, 2, 1, 2): a stage that ends on an unshifted block and one with a shifted one."""
    from oracle import htsat as oh
    hc = dict(cases.htsat_test_config(), depths=(1, 2, 1, 2))
    ac = dict(oh.AUDIO_CFG)
    sd = cases.htsat_state_dict(_shapes(g, "htsat"), seed=5)
    wav48 = oh.resample(cases.clap_waveform(1, seed=33), 16000, 48000)[:, :288000]
    assert rel(oh.htsat_embedding(sd, wav48, hc, ac), g["htsat"]) < 1e-5


def test_phoneme_and_t5_oracles_equal_live_reference(g):
    """§8(f) ranks 1 (second half) and 2: the REAL PhonemeEncoder and FlanT5HiddenState on inputs, weights and geometries
    that are not in the other fixtures."""
    from oracle import phoneme as oph
    from oracle import t5 as ot5
    # VITS phoneme encoder: other weights, a shorter pad length, other ids / lengths
    pc = cases.PHONEME_CROSSCHECK
    sd = cases.phoneme_state_dict(_shapes(g, "phoneme"), seed=4)
    gen = torch.Generator().manual_seed(17)
    idx = torch.randint(1, pc["vocabs_size"], (3, pc["pad_length"]), generator=gen)
    for b, n in enumerate(cases.PHONEME_CROSSCHECK_LENGTHS):
        idx[b, n:] = pc["pad_token_id"]
    emb, mask = oph.phoneme_encoder_forward(sd, idx, pc["pad_token_id"])
    assert rel(emb, g["phoneme_emb"]) < 1e-5 and torch.equal(mask, torch.from_numpy(g["phoneme_mask"]))
    # FLAN-T5 encoder: other weights, a narrower geometry, other token batch (lengths 9, 17, 2 padded to 17)
    cfg = cases.t5_crosscheck_config()
    L = max(cases.T5_CROSSCHECK_LENGTHS)
    ids = torch.randint(3, cfg["vocab_size"], (3, L), generator=gen)
    am = torch.zeros(3, L, dtype=torch.long)
    for b, n in enumerate(cases.T5_CROSSCHECK_LENGTHS):
        ids[b, n - 1] = 1
        ids[b, n:] = 0
        am[b, :n] = 1
    tsd = cases.t5_state_dict(_shapes(g, "t5"), seed=6)
    h, m2 = ot5.encode_tokens(tsd, cfg, ids, am)
    assert rel(h, g["t5_hidden"]) < 1e-5 and torch.equal(m2.float(), torch.from_numpy(g["t5_mask"]).float())
