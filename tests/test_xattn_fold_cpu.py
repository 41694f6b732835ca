"""Folded cross-attention, what can be checked without a GPU: the algebra of the fold in fp64, the gate of
BasicTransformerBlock.run, the host planner, the ABI."""
import pytest
import torch

import xattn_fold as xf


@pytest.mark.parametrize("B,L,C,Lk", [(3, 64, 256, 8), (3, 96, 384, 5), (3, 64, 640, 8), (3, 32, 640, 1), (3, 32, 64, 5)])
def test_fp64_fold_equals_the_unfolded_formula(B, L, C, Lk):
    """Re-association only: with masks (two keys of sample 1, every key of sample 2), a zero context (sample 0) and Lk in
    {1, 5, 8} the folded formula equals the unfolded one to 1e-12 of max |out|, masked and unmasked."""
    c = xf.case(B, L, C, Lk)
    mq, mo = xf.fold64(c)
    assert mq.shape == (B, C, C // 4) and mo.shape == (B, C // 4, C)
    assert not mq.view(B, C, -1, 8)[..., Lk:].any() and not mo.view(B, -1, 8, C)[:, :, Lk:].any()
    for mask in (True, False):
        e = xf.max_rel(xf.ref_folded(c, mq, mo, mask=mask), xf.ref_unfolded(c, mask=mask))
        assert e < 1e-12, (mask, e)
    # the all-masked sample is uniform over its Lk real keys: equal to its unmasked output only when Lk == 1
    full, plain = xf.ref_unfolded(c, mask=True), xf.ref_unfolded(c, mask=False)
    assert torch.equal(full[0], plain[0])
    assert (Lk == 1) == bool(torch.allclose(full[2], plain[2], rtol=0, atol=1e-9))


def test_abi_and_symbols():
    from audioldm2_amd import lib
    assert lib.ABI_VERSION >= 21
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    for name in ("aldm_xattn_fold_plan", "aldm_xattn_fold_bytes", "aldm_xattn_fold_prepare", "aldm_xattn_folded"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(l, name), name
    # 3 parts x 2 bytes x B x C x roundup(C / 4, 32): the headline model's 3.1 / 7.1 / 19.7 MB per image pair at batch 16
    assert l.aldm_xattn_fold_bytes(16, 256) == 16 * 256 * 64 * 6
    assert l.aldm_xattn_fold_bytes(2, 64) == 2 * 64 * 32 * 6
    sizes = [2 * l.aldm_xattn_fold_bytes(16, C) / 1e6 for C in (256, 384, 640)]
    assert [round(s, 1) for s in sizes] == [3.1, 7.1, 19.7]


def test_planner_accepts_the_documented_shapes_and_refuses_the_rest():
    from audioldm2_amd import ops
    for B, L, C, Lk in [(16, 1024, 256, 8), (16, 256, 384, 8), (16, 64, 640, 8), (3, 32, 256, 1), (3, 96, 384, 5), (2, 128, 64, 8),
                        (2, 32, 128, 8)]:
        p = ops.xattn_fold_plan(B, L, C, C // 32, Lk)
        assert p["supported"], (B, L, C, Lk)
        assert p["tile_rows"] in (32, 64) and p["waves"] in (4, 8) and (C // 32) % p["col_splits"] == 0
        assert p["blocks"] == B * -(-L // p["tile_rows"]) * p["col_splits"]
        assert p["lds_bytes"] == 6 * p["tile_rows"] * (C + 8) + 6 * p["tile_rows"] * (max(32, -(-C // 128) * 32) + 8) <= 160 * 1024
    for B, L, C, heads, Lk in [(3, 64, 256, 8, 9), (3, 48, 256, 8, 8), (3, 64, 48, 1, 8), (3, 64, 256, 4, 8), (3, 64, 256, 8, 0),
                               (3, 64, 1024, 32, 8), (0, 64, 256, 8, 8)]:
        assert not ops.xattn_fold_plan(B, L, C, heads, Lk)["supported"], (B, L, C, heads, Lk)
    # the three forms the headline model and the GPU tests reach
    lvl1 = ops.xattn_fold_plan(16, 1024, 256, 8, 8)
    assert (lvl1["tile_rows"], lvl1["col_splits"], lvl1["blocks"], lvl1["waves"]) == (64, 1, 256, 4)
    lvl2 = ops.xattn_fold_plan(16, 256, 384, 12, 8)
    assert (lvl2["tile_rows"], lvl2["col_splits"], lvl2["blocks"], lvl2["waves"]) == (32, 2, 256, 4)
    lvl3 = ops.xattn_fold_plan(16, 64, 640, 20, 8)
    assert (lvl3["tile_rows"], lvl3["col_splits"], lvl3["blocks"], lvl3["waves"]) == (32, 5, 160, 8)
    assert all(128 <= p["blocks"] <= 256 for p in (lvl1, lvl2, lvl3))
    assert ops.xattn_fold_plan(3, 64, 640, 20, 8)["col_splits"] == 20
    assert ops.xattn_fold_plan(2, 1024, 256, 8, 8)["tile_rows"] == 64
    assert ops.xattn_fold_plan(3, 96, 256, 8, 8)["tile_rows"] == 64 and ops.xattn_fold_plan(3, 32, 256, 8, 8)["tile_rows"] == 32


def test_gate(monkeypatch):
    """ops.xattn_fold_applies: DMA mode, a mode other than f32, C % 32 == 0, at most 8 keys, L % 32 == 0, the switch, the planner."""
    from audioldm2_amd import ops
    monkeypatch.setattr(ops, "DMA_MODE", True)
    monkeypatch.setattr(ops, "MMA_MODE", "bf16x6")
    monkeypatch.setattr(ops, "XATTN_FOLD", True)
    use = lambda B, L, C, Lk: ops.xattn_fold_plan(B, L, C, C // 32, Lk)["use"]
    for shape in [(16, 1024, 256, 8), (16, 256, 384, 8), (16, 64, 640, 8), (2, 128, 64, 8), (3, 32, 128, 5)]:
        B, L, C, Lk = shape
        assert ops.xattn_fold_applies(B, L, C, C // 32, Lk) == use(B, L, C, Lk), shape
    ok = (2, 128, 128, 4, 8)
    assert ops.xattn_fold_plan(*ok)["use"] and ops.xattn_fold_applies(*ok)
    assert not ops.xattn_fold_applies(2, 128, 128, 4, 9)       # Lk = 9
    assert not ops.xattn_fold_applies(2, 128, 128, 4, 32)      # the FLAN-T5 context
    assert not ops.xattn_fold_applies(2, 48, 128, 4, 8)        # L = 48
    assert not ops.xattn_fold_applies(2, 128, 48, 1, 8)        # C = 48
    for mode in ("bf16x3", "f16x3"):
        monkeypatch.setattr(ops, "MMA_MODE", mode)
        assert ops.xattn_fold_applies(*ok)
    monkeypatch.setattr(ops, "MMA_MODE", "f32")
    assert not ops.xattn_fold_applies(*ok)
    monkeypatch.setattr(ops, "MMA_MODE", "bf16x6")
    monkeypatch.setattr(ops, "DMA_MODE", False)
    assert not ops.xattn_fold_applies(*ok)
    monkeypatch.setattr(ops, "DMA_MODE", True)
    prev = ops.xattn_fold(False)                                # the switch
    try:
        assert prev is True and not ops.xattn_fold_applies(*ok)
        assert ops.xattn_fold([256]) is False
        assert not ops.xattn_fold_applies(*ok) and ops.xattn_fold_applies(2, 64, 256, 8, 8) == use(2, 64, 256, 8)
        ops.xattn_fold(True)
        assert ops.xattn_fold_applies(*ok)
    finally:
        ops.xattn_fold(True)
    assert ops._parse_xattn_fold("0") is False and ops._parse_xattn_fold(None) is True and ops._parse_xattn_fold("1") is True
    assert ops._parse_xattn_fold("256,640") == frozenset({256, 640})
