"""The 64-queries-per-wave attention kernels (QT = 2: a wave owns two 32-query tiles, a block 256 queries) at ragged lengths against
fp64.  Every launcher of csrc/attn.hip takes them when Lq >= 128 and ceil(Lq / 256) * heads * B >= 128
(aldm_attention_query_tiles); each test asserts that its shape does, so a pinned $ALDM_ATTN_QT fails it instead of testing the other
family.  What only QT = 2 has: a wave whose first query tile holds live rows and whose second lies wholly past Lq (every row of it
clamped to Lq - 1, none stored), next to the ragged last key tile, the waves of a block that exit, and the TAIL forms of the
pre-split kernels.  References: attention.py:343-367 restated in fp64 (ref_attention); bars: fused_tol of tests/tolerances.py."""
import functools
import math

import pytest
import torch
from test_dma_gpu import _qkv_images, _score_tol, assert_split_equals, exact_split
from test_ops_gpu import ATTN_MODE_NAME, ref_attention
from tolerances import fused_tol, log_err

pytestmark = pytest.mark.gpu


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b, bar, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return log_err(float((a - b).abs().max() / (b.abs().max() + 1e-30)), bar, what)


@pytest.fixture(scope="module", params=["bf16x6", "bf16x3"])
def ops(request):
    """The engine's two split modes: the pre-split images (and the split image an attention launch writes) have 3 or 2 parts."""
    from audioldm2_amd import ops as o
    prev = o.set_mma(request.param)
    yield o
    o.set_mma(prev)


@pytest.fixture(scope="module")
def ops_any():
    """For tests that pick the attention mode themselves and write no split image: the engine's mode does not matter."""
    from audioldm2_amd import ops as o
    return o


@pytest.fixture(scope="module")
def ops16():
    from audioldm2_amd import ops as o
    prev = o.set_mma("f16x3")
    yield o
    o.set_mma(prev)


# ---- (a) the fp32-K/V kernels: attention_d32_kernel<MASK, 2, BX, NP> and, with whole key tiles, attention_d32_pipe_kernel<MASK, 2, NP>

FP32_KV_CASES = [
    (16, 8, 130, 45, True),     # wave 2's second tile wholly past Lq; ragged key tile
    (16, 8, 161, 8, True),      # 8 keys; one live row in a second tile
    (16, 8, 192, 77, True),     # wave 3 exits; three key tiles, the last ragged
    (16, 8, 200, 33, False),    # one key in the last tile, unmasked
    (16, 8, 256, 1, False),     # a single key
    (16, 8, 255, 64, False),    # pipelined kernel, unmasked, ragged Lq
    (8, 8, 257, 96, True),      # pipelined kernel, masked; the second block holds one row
    (4, 32, 130, 100, False),   # many heads, small batch
]


@functools.lru_cache(maxsize=None)
def _fp32_kv_case(B, heads, Lq, Lk, masked):
    """(q buffer, k | v buffer, mask, fp64 reference) of one case, on the CPU; computed once, shared by the engine modes."""
    Cc = heads * 32
    # fused-QKV style buffers: q / k / v are column slices of wider row-major buffers (row pitch != heads * 32)
    qb = torch.randn(B, Lq, Cc + 64, generator=g(1))
    kvb = torch.randn(B, Lk, 2 * Cc, generator=g(2))
    mask = None
    if masked:
        mask = (torch.rand(B, Lk, generator=g(3)) < 0.7).float()
        mask[:, 0] = 1
        mask[0, :] = 0                      # every key masked: the reference degenerates to uniform weights
        mask[1, :] = 0
        mask[1, 0] = 1                      # only key 0 live
        mask[2, :] = 0
        mask[2, Lk - 1] = 1                 # only the last key live
        if Lk > 32:                         # the whole first key tile masked, later keys live: the running maximum starts at
            mask[3, :32] = 0                # -FLT_MAX and has to be rescaled away
            mask[3, 32] = 1
    q, k, v = qb[:, :, :Cc], kvb[:, :, :Cc], kvb[:, :, Cc:]
    ref = ref_attention(q.double().contiguous(), k.double().contiguous(), v.double().contiguous(), heads, mask)
    return qb, kvb, mask, ref


@pytest.mark.parametrize("B,heads,Lq,Lk,masked", FP32_KV_CASES)
def test_fp32_kv_attention_at_64_queries_per_wave(ops, B, heads, Lq, Lk, masked):
    """ops.attention in the three product modes (fp32 MFMA, bf16x6, bf16x3) on shapes the host rule sends to the QT = 2 kernels:
    finite, within the mode's bar of fp64, and the split image written next to the fp32 output holds the same values."""
    assert ops.attention_query_tiles(B, heads, Lq) == 2
    Cc = heads * 32
    qb, kvb, mask, ref = _fp32_kv_case(B, heads, Lq, Lk, masked)
    qd, kvd = qb.cuda(), kvb.cuda()
    md = None if mask is None else mask.cuda()
    for mode in (1, 2, 3):
        prev = ops.attention_mma(mode)
        try:
            y, s = ops.attention(qd[:, :, :Cc], kvd[:, :, :Cc], kvd[:, :, Cc:], heads, mask=md, split_out="also")
        finally:
            ops.attention_mma(prev)
        name = ATTN_MODE_NAME[mode]
        assert torch.isfinite(y).all(), f"mode {name}"
        assert rel_err(y, ref, fused_tol(name), f"fp32-K/V attention {name} vs fp64") < fused_tol(name), f"mode {name}"
        assert_split_equals(ops, s, y, f"mode {name}")


# ---- (b) nothing past the last row is read: K / V and Q are the leading rows of buffers whose remainder is NaN

@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("Lk", [8, 33, 40, 64, 96, 1])
def test_attention_at_64_queries_per_wave_loads_no_row_past_the_last(ops_any, Lk, masked):
    """test_attention_loads_no_key_past_the_last (tests/test_ops_gpu.py) at QT = 2 and a ragged Lq: a K / V row >= Lk of the last
    sample entering a product shows up as NaN (0 * NaN).  Q is built the same way: the clamped rows of the waves that reach past
    Lq = 200 (rows 200 .. 255 of the block) re-read row Lq - 1, never the row after it."""
    ops = ops_any
    B, heads, Lq = 16, 8, 200
    assert ops.attention_query_tiles(B, heads, Lq) == 2
    Cc = heads * 32
    nq, nkv = B * Lq * Cc, B * Lk * 2 * Cc
    qflat = torch.full((nq + 64 * Cc,), float("nan"))
    qflat[:nq] = torch.randn(nq, generator=g(1))
    qd = qflat.cuda()[:nq].view(B, Lq, Cc)
    flat = torch.full((nkv + 64 * 2 * Cc,), float("nan"))
    flat[:nkv] = torch.randn(nkv, generator=g(2))
    kvd = flat.cuda()[:nkv].view(B, Lk, 2 * Cc)
    mask = None
    if masked:
        mask = torch.ones(B, Lk)
        mask[:, Lk // 2:] = 0
        mask[:, 0] = 1
    ref = ref_attention(qflat[:nq].view(B, Lq, Cc).double(), flat[:nkv].view(B, Lk, 2 * Cc)[:, :, :Cc].double().contiguous(),
                        flat[:nkv].view(B, Lk, 2 * Cc)[:, :, Cc:].double().contiguous(), heads, mask)
    md = None if mask is None else mask.cuda()
    for mode in (1, 2, 3):
        prev = ops.attention_mma(mode)
        try:
            y = ops.attention(qd, kvd[:, :, :Cc], kvd[:, :, Cc:], heads, mask=md)
        finally:
            ops.attention_mma(prev)
        name = ATTN_MODE_NAME[mode]
        assert torch.isfinite(y).all(), f"mode {name}: a row past the last entered the product"
        assert rel_err(y, ref, fused_tol(name), f"NaN-tail attention {name} vs fp64") < fused_tol(name), f"mode {name}"


# ---- (c), (d) the pre-split self-attention's TAIL forms: attention_d32_presplit2_kernel<2, NP, false, F16, true>

TAIL_SHAPES = [(16, 130), (16, 161), (16, 200), (16, 250), (8, 300)]
HEADS = 8   # C = 256: the operand-stationary kernel's QKV form needs K = 256 (and qkv_c % 128 == 0)
# the QKV projection's epilogue families, as in tests/test_durations_gpu.py: None = whatever the tuner picks, "os" = igemm_dma_os.h
FAMILIES = {"auto": None, "os": (32, 128, 302)}


def _forced(ops, fam, fn):
    f = FAMILIES[fam]
    if f is not None:
        ops.igemm_force(f[0], f[1], 1, 0, f[2])
    try:
        return fn()
    finally:
        if f is not None:
            ops.igemm_force(0, 0, 0)


def _self_attention_ref(x, wq, wk, wv, heads):
    """fp64 self-attention of the rows x [B, L, C] (fp64) under the three projections."""
    return ref_attention(x @ wq.double().t(), x @ wk.double().t(), x @ wv.double().t(), heads)


@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize("B,L", TAIL_SHAPES)
def test_ragged_presplit_attention_at_64_queries_per_wave_is_bitwise_the_fp32_kv_path(ops, B, L, fam):
    """test_ragged_presplit_attention_is_bitwise_the_fp32_kv_path (tests/test_durations_gpu.py) at batch 16: ALDM_EPI_QKV +
    aldm_attention_d32_presplit with a partial last key tile AND partial query blocks on the QT = 2 TAIL kernel, against the
    fp32-K/V path's QT = 2 ragged kernel — the same products in the same order, so bit-identical outputs and split images; and
    within the fp64 bar."""
    assert ops.attention_query_tiles(B, HEADS, L) == 2
    C = HEADS * 32
    x = torch.randn(B, L, C, generator=g(1))
    wq, wk, wv = (torch.randn(C, C, generator=g(2 + i)) / math.sqrt(C) for i in range(3))
    pw = ops.pack_conv(torch.cat([wq, wk, wv], 0))
    xs = ops.split_rows(x.cuda())
    qkv = _forced(ops, fam, lambda: ops.linear(xs, pw))
    a_old, s_old = ops.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], HEADS, split_out="also")
    q, kimg, vtimg = _forced(ops, fam, lambda: ops.linear_qkv(xs, pw, HEADS, L))
    assert vtimg.shape[2] == -(-L // 32)
    a_new, s_new = ops.attention_presplit(q, kimg, vtimg, HEADS, split_out="also")
    assert torch.isfinite(a_new).all()
    assert torch.equal(a_new, a_old) and torch.equal(s_new.data, s_old.data)
    ref = _self_attention_ref(xs.float().double().cpu(), wq, wk, wv, HEADS)
    assert rel_err(a_new, ref, fused_tol(), "pre-split TAIL attention vs fp64") < fused_tol()


@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize("B,L", TAIL_SHAPES)
def test_ragged_presplit_attention_f16x3_at_64_queries_per_wave(ops16, B, L, fam):
    """test_ragged_presplit_attention_f16x3 (tests/test_durations_gpu.py) on the QT = 2 F16 TAIL kernel: fp16 K / V^T images, three
    products, LayerNorm-fed like the UNet, within the f16x3 bar of fp64."""
    ops = ops16
    assert ops.attention_query_tiles(B, HEADS, L) == 2
    C = HEADS * 32
    x = torch.randn(B, L, C, generator=g(1))
    ga, be = torch.randn(C, generator=g(2)) * 0.3 + 1.0, torch.randn(C, generator=g(3)) * 0.1
    wq, wk, wv = (torch.randn(C, C, generator=g(4 + i)) / math.sqrt(C) for i in range(3))
    pw = ops.pack_conv(torch.cat([wq, wk, wv], 0))
    n = ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), 1e-5, split_out="only")
    q, kimg, vtimg = _forced(ops, fam, lambda: ops.linear_qkv(n, pw, HEADS, L))
    assert kimg.shape[2] == 2 and getattr(kimg, "_aldm_f16", None) is not None   # the fp16 images: the F16 TAIL kernel ran
    a = ops.attention_presplit(q, kimg, vtimg, HEADS)
    xn = torch.nn.functional.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    ref = _self_attention_ref(xn, wq, wk, wv, HEADS)
    assert torch.isfinite(a).all()
    assert rel_err(a, ref, fused_tol("f16x3"), "pre-split F16 TAIL attention vs fp64") < fused_tol("f16x3")


# ---- (e) schedules 0, 2 and 3 of the pre-split kernel with whole key tiles and partial query blocks (L % 32 == 0, L % 256 != 0)

@pytest.mark.parametrize("B,L", [(16, 160), (16, 224)])
def test_presplit_schedules_at_64_queries_per_wave_and_partial_blocks(ops, B, L):
    """attention_d32_pipe_kernel<false, 2, NP, true> (schedule 0) and schedule 3 — which must fall back to the default kernel, its
    LDS form taking whole blocks only — are bitwise the default schedule; attention_d32_presplit3_kernel<2, NP> (schedule 2, fixed
    softmax reference per row) is held to the fp64 bar tests/test_dma_gpu.py holds it to: the mode's fused bar plus _score_tol."""
    assert ops.attention_query_tiles(B, HEADS, L) == 2 and L % 32 == 0 and L % 256 != 0
    C = HEADS * 32
    q, k, v = (torch.randn(B, L, C, generator=g(i)) for i in (1, 2, 3))
    (qi, kimg, vtimg), qkv = _qkv_images(ops, q, k, v, HEADS)
    out = {}
    prev = ops.attention_sched(1)
    try:
        for sched in (1, 0, 2, 3):
            ops.attention_sched(sched)
            out[sched] = ops.attention_presplit(qi, kimg, vtimg, HEADS)
    finally:
        ops.attention_sched(prev)
    qd, kd, vd = (qkv[..., i * C:(i + 1) * C].double().cpu().contiguous() for i in range(3))
    ref = ref_attention(qd, kd, vd, HEADS)
    smax = float(torch.einsum("bihd,bjhd->bhij", qd.view(B, L, HEADS, 32), kd.view(B, L, HEADS, 32)).abs().max()) / math.sqrt(32.0)
    for sched in (1, 0, 2, 3):
        assert torch.isfinite(out[sched]).all(), f"schedule {sched}"
    assert torch.equal(out[0], out[1]), "schedule 0 is documented as bitwise the default"
    assert torch.equal(out[3], out[1]), "schedule 3 on partial blocks runs the default kernel"
    assert rel_err(out[1], ref, fused_tol(), "pre-split attention schedule 1 vs fp64") < fused_tol()
    bar2 = fused_tol() + _score_tol(exact_split(ops), smax)
    assert rel_err(out[2], ref, bar2, "pre-split attention schedule 2 vs fp64") < bar2
