"""The tuning tables as test cases, the part that needs no GPU: every key of the four shipped tables maps onto a launch of the
public ops API (tests/tuned_geometry.py), maps back onto itself through ops.tune_key, and the fp64 tap-sum reference the GPU sweep
(tests/test_tuned_geometries_gpu.py) judges the kernels by agrees with torch's own fp64 convolutions on every variant of
operation the tables hold.

No test here touches a GPU.  One of them, test_register_staged_entries_plan_onto_their_hint, asks the library's host planner
(aldm_igemm_plan) and therefore needs the built libaldm_hip.so, as tests/test_abi.py's planner tests do; the others need no library."""
import ctypes

import pytest
import torch
import tuned_geometry as tg
from tolerances import F64 as F

ALL = [(name, key) for name in tg.TABLES for key in tg.load_table(name)]
SIZES = {"mi355x_igemm.json": 145, "mi355x_igemm_bf16x6.json": 97, "mi355x_igemm_dma.json": 163, "mi355x_igemm_dma_bf16x3.json": 173}


def test_every_key_of_every_table_maps_to_a_case():
    assert {n: len(tg.load_table(n)) for n in tg.TABLES} == SIZES and len(ALL) == 578
    for name, key in ALL:
        c = tg.case_from_key(key)
        assert c["op"] in ("linear", "linear_geglu", "conv"), (name, key)     # the tables hold weight GEMMs only
        assert (c["split"] is not None) == ("dma" in name), (name, key)
        assert c["split"] == {"mi355x_igemm_dma.json": "dma", "mi355x_igemm_dma_bf16x3.json": "dma2"}.get(name), (name, key)
        if c["remap"]:
            mul, off, out_len = c["remap"]
            assert off == mul - 1 and out_len >= mul * c["OW"] and 2 <= mul <= 6


def test_out_hw_rederived_from_the_case_is_the_keys():
    explicit = 0
    for name, key in ALL:
        f, _, _ = tg.parse_key(key)
        c = tg.case_from_key(key)
        assert tg.derived_out_hw(c) == (f["OH"], f["OW"]), (name, key)
        if c["out_hw"] is not None:
            # more output positions than the padding gives, never fewer: the extra ones read zeros (asymmetric-pad downsample of
            # the VAE encoder, one spare polyphase position of the vocoder's transposed convolutions)
            explicit += 1
            nat = (tg.natural_out(c["H"], c["up"][0], c["pad"][0], c["dil"][0], c["KH"], c["stride"][0]),
                   tg.natural_out(c["W"], c["up"][1], c["pad"][1], c["dil"][1], c["KW"], c["stride"][1]))
            assert 0 <= f["OH"] - nat[0] <= 1 and 0 <= f["OW"] - nat[1] <= 1, (name, key, nat)
    assert 0 < explicit < 40


def test_every_key_round_trips_through_tune_key():
    from audioldm2_amd import ops
    for name, key in ALL:
        c = tg.case_from_key(key)
        assert ops.tune_key(tg.desc_from_case(c)) == key, (name, key)
        assert tg.shrunk_key(c) == tg.normalise_key(tg.shrunk_key(c))
        assert tg.variant(tg.case_from_key(tg.shrunk_key(c))) == tg.variant(c), (name, key)


def test_no_key_twice_after_normalisation():
    for name in tg.TABLES:
        keys = list(tg.load_table(name))
        norm = [tg.normalise_key(k) for k in keys]
        assert len(set(norm)) == len(keys), name
        assert norm == keys, name                       # and the shipped spelling IS the normal form ops.tune_key produces


def test_register_staged_entries_plan_onto_their_hint():
    """The host planner on every entry of the two register-staged tables (test_abi.py does the two DMA tables): tile, split-K,
    wave groups and the matrix-core path are the entry's — what the GPU sweep then asserts of the launch it records."""
    from audioldm2_amd import lib
    l = lib.load()
    for name in tg.TABLES[:2]:
        for key, v in tg.load_table(name).items():
            d = tg.desc_from_case(tg.case_from_key(key))
            d.x1, d.w, d.out, d.alpha, d.ldo = 0x1000, 0x2000, 1 << 20, 1.0, d.N    # never dereferenced by the planner
            d.x2 = 0x1800 if d.C2 else 0
            d.ws, d.ws_floats = 16, 1 << 40
            if name == "mi355x_igemm_bf16x6.json":
                d.w_split, d.split_parts = 0x4000, 3
                d.hint_mma = v[4]
            d.hint_bm, d.hint_bn, d.hint_splits, d.hint_kgroups = v[:4]
            bm, bn, sp, kg, mma = (ctypes.c_int() for _ in range(5))
            assert l.aldm_igemm_plan(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn), None, ctypes.byref(sp), ctypes.byref(kg),
                                     ctypes.byref(mma)) == 0, (key, l.aldm_last_error())
            assert (bm.value, bn.value, sp.value, max(kg.value, 1)) == (v[0], v[1], v[2], max(v[3], 1)), (name, key, v)
            assert mma.value == (1 if (name == "mi355x_igemm_bf16x6.json" and v[4] == 0) else 0), (name, key, v, mma.value)


def _variants():
    seen = {}
    for name, key in ALL:
        c = tg.case_from_key(key)
        seen.setdefault(tg.variant(c), (name, key))
    return sorted(seen.values())


VARIANTS = _variants()


def test_the_variants_are_the_ones_the_issue_names():
    """Kernel size, stride, dilation, upsampling, out_mul, prologue, concat: about 25 of them by the tables' census; at least the
    classes the sweep exists for must be among them."""
    vs = [tg.variant(tg.case_from_key(k)) for _, k in VARIANTS]
    assert len(vs) >= 25
    assert {v[5] for v in vs} >= {0, 2, 4, 5, 6}                                   # polyphase phases
    assert {(v[1], v[3][1]) for v in vs} >= {(15, 1), (15, 3), (15, 5)}            # dilated 1 x 15 vocoder convs
    assert any(v[4] == (2, 2) for v in vs) and any(v[2] == (2, 2) for v in vs) and any(v[7] for v in vs) and any(v[8] for v in vs)
    assert {v[6] for v in vs} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name,key", VARIANTS, ids=[f"{tg.SHORT[n]}-{i}" for i, (n, _) in enumerate(VARIANTS)])
def test_tap_sum_reference_agrees_with_torch_fp64_convolutions(name, key):
    """reference_fp64 (index arithmetic + one matmul per tap) against F64.conv2d / conv1d / conv_transpose1d on a small key of the
    same variant (2 M N K <= 2 GFLOP): 1e-12."""
    c = tg.case_from_key(tg.shrunk_key(tg.case_from_key(key)))
    assert c["flops"] <= 2e9
    inp = tg.make_inputs(c, torch.device("cpu"), seed=3)
    a = inp["x"] if inp["x2"] is None else torch.cat([inp["x"], inp["x2"]], -1)
    a = tg.prologue_fp64(c, a.double(), inp["scale"], inp["shift"])
    got = tg.reference_fp64(c, a, inp["w"], inp["bias"], inp["res"])
    OH, OW = tg.derived_out_hw(c)
    (SH, SW), (PH, PW), (DH, DW), (UH, UW) = c["stride"], c["pad"], c["dil"], c["up"]
    an = a.permute(0, 3, 1, 2)                                                    # NCHW for torch
    an = an.repeat_interleave(UH, 2).repeat_interleave(UW, 3)                     # nearest upsampling
    w = inp["w"]
    if c["remap"]:
        # a polyphase case IS one output phase of a ConvTranspose1d with stride u = out_mul, kernel T u, no padding:
        # out[q u + ph] = sum_j x[q - j] Wt[:, :, ph + j u], i.e. tap kw = T - 1 - j of a correlation padded by T - 1
        u, ph, out_len = c["remap"]
        T = c["KW"]
        assert PW == T - 1 and c["KH"] == 1 and SW == 1 and DW == 1
        g = torch.Generator().manual_seed(9)
        wt = torch.randn(an.shape[1], c["N"], T * u, generator=g, dtype=torch.float64)   # the other phases: anything
        for kw in range(T):
            wt[:, :, ph + (T - 1 - kw) * u] = w[:, :, 0, kw].double().t()
        full = F.conv_transpose1d(an[:, :, 0], wt, stride=u)                      # [B, N, (W - 1) u + T u]
        Q = c["W"] + T - 1                                                        # positions q whose phase row exists
        want = full[:, :, ph::u][:, :, :Q].permute(0, 2, 1) + inp["bias"].double()
        want = want + inp["res"].double().view(c["B"], out_len, -1)[:, ph::u][:, :Q]
        assert OW in (Q, Q + 1)
        got_q = got[:, 0, :Q]
        if OW > Q:   # the spare position reads only zeros: bias + residual
            spare = inp["bias"].double() + inp["res"].double().view(c["B"], out_len, -1)[:, ph + Q * u]
            assert float((got[:, 0, Q] - spare).abs().max()) < 1e-12
    else:
        # explicit zero padding: PH / PW on the top / left, on the bottom / right whatever the last output position reads
        bot = (OH - 1) * SH + DH * (c["KH"] - 1) + 1 - an.shape[2] - PH
        right = (OW - 1) * SW + DW * (c["KW"] - 1) + 1 - an.shape[3] - PW
        assert 0 <= bot <= PH + SH and 0 <= right <= PW + SW
        ap = F.pad(an, (PW, right, PH, bot))
        if c["H"] == 1 and c["KH"] == 1:
            y = F.conv1d(ap[:, :, 0], w[:, :, 0], inp["bias"], stride=SW, dilation=DW).unsqueeze(2)
        else:
            y = F.conv2d(ap, w, inp["bias"], stride=(SH, SW), dilation=(DH, DW))
        y = y.permute(0, 2, 3, 1)
        if c["geglu"]:
            half = c["N"] // 2
            y = y[..., :half] * F.gelu(y[..., half:])
        want, got_q = (y if inp["res"] is None else y + inp["res"].double()), got
    assert want.shape == got_q.shape
    err = float((got_q - want).abs().max() / want.abs().max())
    assert err < 1e-12, err
