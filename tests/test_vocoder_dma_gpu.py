"""The vocoder's pre-split stage (audioldm2_amd/hifigan.py Generator._stage_dma), launch form by launch form, against plain torch in
fp64 on the same fp32 inputs.

_stage_dma runs every upsampling stage with at least 128 channels — 87 % of the vocoder's FLOPs — on launch forms no other op
test issues; the whole-generator fixture test (tests/test_model_gpu.py, 60+ launches under tail_tol = 4e-5) would not notice
a wrong slope on an image, an activated fp32 output, a read of `out` on a non-accumulating launch, a dilated tap leaking across
the seam between two samples, or one lost partial product in just these epilogues.  Here:

  1. the producer: split_rows(x, act=ACT_LRELU, slope) is BITWISE the image of torch's own fp32 leaky_relu, planted edge values
     included (split_rows_kernel<ALDM_ACT_LRELU, false>);
  2. conv1 of a ResBlock step: a 1-D dilated conv over that image with a leaky-relu epilogue (act / act_slope), fp32 output and
     image ("also") and image alone ("only");
  3. conv2 with the next conv1's operand: residual, fp32 output NOT activated, image of leaky_relu(output) under its own slope
     (split_act / split_slope: the out_split_act branches);
  4. the closing launch of the three ResBlocks: residual, alpha = 1/3, out = a view into a NaN-filled buffer, accumulate = (j > 0);
  5. the polyphase transposed conv over a pre-split operand with the row remap, phase by phase into a NaN-filled buffer;
  6. one whole two-stage generator (stage 0 on pre-split operands, stage 1 register-staged), with the pre-split form on and off,
     against the fp64 oracle, next to torch's own fp32 evaluation of the same oracle.

2 .. 5 run on whatever the planner picks AND on forced tiles (one 64-row, one 128-row, one 256-row, from test_dma_gpu._TILES),
each without split-K and with split-K 3 (igemm_reduce_kernel's remap / accumulate / leaky-relu-image branches); every launch is
asserted, through ops.TUNE_LOG / ops.PROFILE, to have run a DMA-fed kernel on the forced tile, ring depth and split count.

Shapes: two samples of 203 rows (M = 406: no tile size divides it, a row tile straddles the seam between the samples, and the
padding — up to 35 rows — is needed at both ends of each sample), 128 and 192 channels (192: six channel blocks, a partial
column tile under 128-wide tiles), the ResBlock (kernel, dilation) pairs (3, 1), (7, 3), (11, 5), (15, 5), and the (kernel,
stride) pairs of every shipped upsampler with at least 128 output channels at Cin = 2 N.  The largest K is 15 * 192 = 2880, under
tolerances.LONG_K.  The bars are the existing ones (tests/tolerances.py: gemm_tol, tail_tol); measured figures are in its docstring
and in profiles/r12_vocoder_dma_errors.txt."""
import contextlib
import functools
import math

import pytest
import torch
import tuned_geometry as tg
from test_dma_gpu import _TILES
from tolerances import F64 as F   # references in fp64 (every floating argument promoted)
from tolerances import gemm_tol, log_err, tail_tol

pytestmark = pytest.mark.gpu

B, L = 2, 203
CHANNELS = [128, 192]
PAIRS = [(3, 1), (7, 3), (11, 5), (15, 5)]            # ResBlock (kernel, dilation): the 16 kHz kernels and the 48 kHz config's fourth
# (kernel, stride, N) of the shipped upsamplers with N >= 128 (16 kHz: 16/5, 16/4, 8/2; 48 kHz: 12/6, 10/5, 8/4), Cin = 2 N
UPSAMPLERS = [(16, 5, 128), (16, 4, 192), (8, 2, 128), (12, 6, 192), (10, 5, 128), (8, 4, 192)]
UP_LENGTHS = [41, 100]
GUARD = 4096                                          # floats of NaN on each side of an output view
# (BM, BN, ring depth) per mode — instantiations test_dma_gpu.py walks — x split-K {1, 3}; None: the planner's own choice
FORCED_TILES = {"bf16x6": [(64, 128, 2), (128, 128, 3), (256, 128, 2)], "bf16x3": [(64, 128, 2), (128, 128, 4), (256, 128, 2)]}
assert all(t in _TILES[m] for m, ts in FORCED_TILES.items() for t in ts)
FORCES = [None] + [(i, sp) for i in range(3) for sp in (1, 3)]
FORCE_IDS = ["planner"] + [f"{rows}rows-splitk{sp}" for rows in (64, 128, 256) for sp in (1, 3)]


def rel_err(a, b, bar=0.0, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return log_err(float((a - b).abs().max() / (b.abs().max() + 1e-30)), bar, what)


def g(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module", params=["bf16x6", "bf16x3"])
def ops(request):
    """Both split modes of the DMA-fed kernels ("f16x3" runs the "bf16x6" launches in the vocoder: it has no norms)."""
    from audioldm2_amd import ops as o
    prev = o.set_mma(request.param)
    yield o
    o.set_mma(prev)
    o.igemm_force(0, 0, 0)
    o.TUNE_LOG = o.PROFILE = None


def exact_split(ops):
    return ops.split_parts() == 3


def rows_cl(t):
    """[B, C, L] (torch's conv1d layout, CPU) -> the engine's channels-last [B, 1, L, C] on the GPU."""
    return t.permute(0, 2, 1).contiguous().cuda().view(t.shape[0], 1, t.shape[2], t.shape[1])


def rows_ncl(y):
    """[B, 1, L, C] on the GPU -> [B, C, L] on the CPU."""
    return y.view(y.shape[0], y.shape[2], y.shape[3]).cpu().permute(0, 2, 1)


def _tile(ops, force):
    if force is None:
        return None
    bm, bn, st = FORCED_TILES[ops.MMA_MODE][force[0]]
    return bm, bn, st, force[1]


@contextlib.contextmanager
def launches(ops, force, n):
    """The igemm launches issued inside: under the forced tile / ring depth / split-K (restored afterwards), logged, and each
    asserted to have run a DMA-fed kernel — igemm_dma_kernel on exactly the forced configuration, with igemm_reduce_kernel
    behind it when split-K is forced (the plan's split count is what aldm_igemm launches the reduce on)."""
    tile = _tile(ops, force)
    ops.TUNE_LOG, ops.PROFILE = [], []
    try:
        if tile is not None:
            ops.igemm_force(tile[0], tile[1], tile[3], 0, tile[2])
        yield
        torch.cuda.synchronize()
        log, prof = ops.TUNE_LOG, ops.PROFILE
    finally:
        ops.igemm_force(0, 0, 0)
        ops.TUNE_LOG = ops.PROFILE = None
    assert len(log) == n and len(prof) == n, (n, log, [p[0] for p in prof])
    suffix = ",dma" if exact_split(ops) else ",dma2"
    for key, (_what, bm, bn, _fl, _e0, _e1, shape, name) in zip(log, prof):
        assert key.endswith(suffix), key
        assert shape[9] == 1 and shape[12] == ops.split_parts(), (key, shape)          # a pre-split A operand of this mode
        assert name.startswith("igemm_dma"), (key, name, "fell back to a register-staged kernel")
        if tile is not None:
            assert (bm, bn, shape[8] // 10) == (tile[0], tile[1], tile[3]), (key, tile, (bm, bn, shape[8] // 10), name)
            assert tg.ran_dma_kernel(name) == ("igemm_dma_kernel", tile[2]), (key, tile, name)


def nan_view(shape):
    numel = math.prod(shape)
    big = torch.full((numel + 2 * GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    return big, big[GUARD:GUARD + numel].view(shape)


def guards_intact(big, numel):
    bits = big.view(torch.int32)
    return bool((bits[:GUARD] == tg.NAN_BITS).all()) and bool((bits[GUARD + numel:] == tg.NAN_BITS).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the producer ------------------------------------------------------------------------------------------------------------------
PLANTED = [-0.0, 0.0, 1e-30, -3e38, 65504.0, float("nan")]


@pytest.mark.parametrize("slope", [0.1, 0.01, 0.25])
@pytest.mark.parametrize("C", CHANNELS)
def test_leaky_relu_producer_is_bitwise_the_image_of_torch_leaky_relu(ops, C, slope):
    """ops.split_rows(x, act=ACT_LRELU, slope) against ops.split_rows(F.leaky_relu(x, slope)), the latter torch's own fp32 kernel on
    the GPU (v > 0 ? v : v * slope, one rounding: the same operation): the images are BITWISE equal, on random values (half of
    them negative) and on planted -0.0, +0.0, 1e-30, -3e38, 65504 and a NaN; the 3-part image sums back to leaky_relu(x) bit for
    bit outside the NaN (a zero sums to +0.0: hi + mid of -0.0 is -0.0 + 0.0).  And the image is what a DMA-fed launch reads: its
    product with the identity gives leaky_relu(x) back (exactly with 3 parts, to 2^-16 with 2) in every row but the NaN's."""
    x = torch.randn(B, 1, L, C, generator=g(1))
    flat = x.view(-1)
    where = [0, 7, 8, C - 1, (L - 1) * C + 5, x.numel() - 1]   # first / last of an 8-channel piece, the seam row, the very last value
    for pos, v in zip(where, PLANTED):
        flat[pos] = v
    nan_row = where[-1] // C
    assert 0.4 < float((x < 0).float().mean()) < 0.6
    xg = x.cuda()
    want = torch.nn.functional.leaky_relu(xg, slope)
    img = ops.split_rows(xg, act=ops.ACT_LRELU, slope=slope)
    ref = ops.split_rows(want)
    assert img.parts == ref.parts == ops.split_parts()
    assert torch.equal(img.data, ref.data), "the fused leaky_relu must give the image of torch's leaky_relu bit for bit"
    if slope != 0.25:
        assert not torch.equal(img.data, ops.split_rows(xg, act=ops.ACT_LRELU, slope=0.25).data), "the slope must be applied"
    if exact_split(ops):
        got = img.float()
        ok = ~torch.isnan(want)
        assert int((~ok).sum()) == 1 and bool(torch.isnan(got[~ok]).all())
        nz = ok & (want != 0)
        assert same_bits(got[nz], want[nz]), "hi + mid + lo must reproduce leaky_relu(x) bitwise"
        assert bool((got[ok & (want == 0)] == 0).all())
    eye = ops.pack_conv(torch.eye(C))
    with launches(ops, None, 1):
        back = ops.linear(img.view(1, B * L, C), eye)
    rows = torch.arange(B * L, device="cuda") != nan_row
    got, w2 = back.view(B * L, C)[rows], want.view(B * L, C)[rows]
    if exact_split(ops):
        assert torch.equal(got, w2)
    else:
        assert bool(((got.double() - w2.double()).abs() <= w2.double().abs() * 2.0 ** -16 + 1e-38).all())


# ---- 2 .. 4: the launches of a ResBlock step -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resblock_case(C, k, d):
    """Inputs and fp64 references of one ResBlock step at (C, k, d), computed once and shared (never modified): x [B, C, L], conv1
    (dilation d) and its references at both slopes, the residual r, conv2 (dilation 1) and the three closing launches' operands."""
    s = 100 * k + d
    x = torch.randn(B, C, L, generator=g(s + 1))
    w1 = torch.randn(C, C, k, generator=g(s + 2)) / math.sqrt(C * k)
    b1 = torch.randn(C, generator=g(s + 3))
    pad1 = (k * d - d) // 2
    c1 = F.conv1d(F.leaky_relu(x, 0.1), w1, b1, dilation=d, padding=pad1)
    w2 = torch.randn(C, C, k, generator=g(s + 4)) / math.sqrt(C * k)
    b2 = torch.randn(C, generator=g(s + 5))
    r = torch.randn(B, C, L, generator=g(s + 6))
    close = []
    for j in range(3):
        a = torch.randn(B, C, L, generator=g(s + 10 + j))
        w = torch.randn(C, C, k, generator=g(s + 20 + j)) / math.sqrt(C * k)
        b = torch.randn(C, generator=g(s + 30 + j))
        rj = torch.randn(B, C, L, generator=g(s + 40 + j))
        close.append((a, w, b, rj, F.conv1d(a, w, b, dilation=d, padding=pad1) + rj.double()))
    return dict(x=x, w1=w1, b1=b1, pad1=pad1, ref1={0.1: F.leaky_relu(c1, 0.1), 0.25: F.leaky_relu(c1, 0.25)}, w2=w2, b2=b2,
                pad2=(k - 1) // 2, r=r, close=close, close_ref=sum(c[4] for c in close) / 3)


def _conv1(ops, c, d, force, slope, split_out):
    xl = ops.split_rows(rows_cl(c["x"]), act=ops.ACT_LRELU, slope=0.1)
    pw = ops.pack_conv(c["w1"], c["b1"])
    with launches(ops, force, 1):
        out = ops.conv(xl, pw, pad=(0, c["pad1"]), dil=(1, d), act=ops.ACT_LRELU, act_slope=slope, split_out=split_out)
    return out


@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("k,d", PAIRS)
@pytest.mark.parametrize("C", CHANNELS)
def test_resblock_conv1_on_the_shared_image(ops, C, k, d, force):
    """conv(xl, pw, pad, dil=(1, d), act=ACT_LRELU, act_slope, split_out="also" | "only") with xl = split_rows(x, LRELU, 0.1): the
    fp32 output against leaky_relu(conv1d(leaky_relu(x), w, b, dilation=d, padding=pad)) in fp64 under gemm_tol (leaky relu is
    piecewise linear with slope <= 1: it cannot amplify the contraction's error), the "also" image bitwise split_rows(fp32
    output), the "only" image bitwise the "also" one; at act_slope = 0.25 a different result that matches ITS reference."""
    c = resblock_case(C, k, d)
    y, img = _conv1(ops, c, d, force, 0.1, "also")
    only = _conv1(ops, c, d, force, 0.1, "only")
    e = rel_err(rows_ncl(y), c["ref1"][0.1], gemm_tol(), "conv1 act_slope 0.1")
    print(f"conv1 C={C} k={k} d={d} {FORCE_IDS[FORCES.index(force)]} [{ops.MMA_MODE}]: {e:.3e} (bar {gemm_tol():.0e})")
    assert e < gemm_tol()
    assert torch.equal(img.data, ops.split_rows(y).data), "the image must be the split of the fp32 output"
    assert torch.equal(only.data, img.data), 'split_out="only" must write the image split_out="also" writes'
    y2, img2 = _conv1(ops, c, d, force, 0.25, "also")
    assert not torch.equal(y2, y), "act_slope must be applied"
    e2 = rel_err(rows_ncl(y2), c["ref1"][0.25], gemm_tol(), "conv1 act_slope 0.25")
    assert e2 < gemm_tol()
    assert torch.equal(img2.data, ops.split_rows(y2).data)


_conv2_refs = {}


@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("k,d", PAIRS)
@pytest.mark.parametrize("C", CHANNELS)
def test_resblock_conv2_writes_the_sum_and_the_next_conv1_operand(ops, C, k, d, force):
    """y, img = conv(t1, pw2, pad, res=r, split_out="also", split_act=ACT_LRELU, split_slope=0.25), t1 the image conv1 wrote under
    slope 0.1: y against conv1d(t1, w2, b2) + r in fp64 under gemm_tol and NOT activated (negative where the reference is); the image
    bitwise split_rows(y, act=ACT_LRELU, slope=0.25) — the image's own slope, not conv1's."""
    c = resblock_case(C, k, d)
    s2 = 0.25
    y1, t1 = _conv1(ops, c, d, None, 0.1, "also")          # (planner's tile: the same operand under every forced configuration)
    pw2 = ops.pack_conv(c["w2"], c["b2"])
    rg = rows_cl(c["r"])
    with launches(ops, force, 1):
        y, img = ops.conv(t1, pw2, pad=(0, c["pad2"]), res=rg, split_out="also", split_act=ops.ACT_LRELU, split_slope=s2)
    # the operand as fp32: what the 3-part image holds exactly and what the 2-part image rounds (inside that mode's bar)
    y1c = rows_ncl(y1)
    key = (ops.MMA_MODE, C, k, d)
    if key not in _conv2_refs or not torch.equal(_conv2_refs[key][0], y1c):
        _conv2_refs[key] = (y1c, F.conv1d(y1c, c["w2"], c["b2"], padding=c["pad2"]) + c["r"].double())
    ref = _conv2_refs[key][1]
    got = rows_ncl(y)
    e = rel_err(got, ref, gemm_tol(), "conv2 + res")
    print(f"conv2 C={C} k={k} d={d} {FORCE_IDS[FORCES.index(force)]} [{ops.MMA_MODE}]: {e:.3e} (bar {gemm_tol():.0e})")
    assert e < gemm_tol()
    neg = ref < -1e-3 * ref.abs().max()
    assert int(neg.sum()) > ref.numel() // 4 and bool((got[neg] < 0).all()), "the fp32 output must not be activated"
    assert abs(float(got.min()) - float(ref.min())) < gemm_tol() * float(ref.abs().max())
    assert torch.equal(img.data, ops.split_rows(y, act=ops.ACT_LRELU, slope=s2).data), \
        "the image must be split(leaky_relu(y, split_slope))"
    assert not torch.equal(img.data, ops.split_rows(y, act=ops.ACT_LRELU, slope=0.1).data)
    assert not torch.equal(img.data, ops.split_rows(y).data)


@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("k,d", PAIRS)
@pytest.mark.parametrize("C", CHANNELS)
def test_resblock_closing_launches_accumulate_the_mean(ops, C, k, d, force):
    """For j = 0, 1, 2: conv(t1_j, pw_j, pad, res=r_j, alpha=1/3, out=xs, accumulate=(j > 0)), xs a view into a NaN-filled buffer:
    after j = 0 xs holds no NaN (the non-accumulating launch read nothing), after j = 2 it is sum_j (conv_j + r_j) / 3 in fp64 under
    gemm_tol, and the guards on both sides are bit-for-bit NaN."""
    c = resblock_case(C, k, d)
    big, xs = nan_view((B, 1, L, C))
    for j, (a, w, b, rj, _ref) in enumerate(c["close"]):
        t1 = ops.split_rows(rows_cl(a))
        pw = ops.pack_conv(w, b)
        rg = rows_cl(rj)
        with launches(ops, force, 1):
            ops.conv(t1, pw, pad=(0, c["pad1"]), dil=(1, d), res=rg, alpha=1.0 / 3, out=xs, accumulate=(j > 0))
        if j == 0:
            assert not bool(torch.isnan(xs).any()), "accumulate=False must not read `out` (and must write every element)"
            e0 = rel_err(rows_ncl(xs), c["close"][0][4] / 3, gemm_tol(), "closing launch j=0")
            assert e0 < gemm_tol()
    e = rel_err(rows_ncl(xs), c["close_ref"], gemm_tol(), "closing launches, mean of three")
    print(f"closing C={C} k={k} d={d} {FORCE_IDS[FORCES.index(force)]} [{ops.MMA_MODE}]: {e:.3e} (bar {gemm_tol():.0e})")
    assert e < gemm_tol()
    assert guards_intact(big, xs.numel()), "a launch wrote outside its output"


# ---- 5. the polyphase transposed conv on a pre-split operand ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def upsampler_case(k, u, N, Lin):
    Cin = 2 * N
    s = 1000 * k + 10 * u + Lin
    x = torch.randn(B, Cin, Lin, generator=g(s + 1))
    w = torch.randn(Cin, N, k, generator=g(s + 2)) / math.sqrt(Cin * k / u)
    b = torch.randn(N, generator=g(s + 3))
    return x, w, b, F.conv_transpose1d(F.leaky_relu(x, 0.1), w, b, stride=u, padding=(k - u) // 2)


@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("Lin", UP_LENGTHS)
@pytest.mark.parametrize("k,u,N", UPSAMPLERS)
def test_polyphase_transposed_conv_on_a_presplit_operand(ops, k, u, N, Lin, force):
    """ConvTranspose1d(k, u, padding=(k - u) // 2) as u stride-1 convs over xa = split_rows(x, LRELU, 0.1) with remap = (u, ph - p,
    Lout), out a view into a NaN-filled buffer: after phase ph exactly the rows t = ph - p (mod u) of [0, Lout) of the phases so far
    are written, after all u none is left, the guards stay NaN, and the result matches conv_transpose1d(leaky_relu(x)) in fp64."""
    x, w, b, ref = upsampler_case(k, u, N, Lin)
    p = (k - u) // 2
    Lout = ref.shape[-1]
    assert Lout == (Lin - 1) * u - 2 * p + k
    phases = ops.pack_convtr1d(w, b, u)
    T = phases[0].KW
    xa = ops.split_rows(rows_cl(x), act=ops.ACT_LRELU, slope=0.1)
    big, out = nan_view((B, 1, Lout, N))
    Q = (Lout + p) // u + 2
    t = torch.arange(Lout, device="cuda")
    expect = torch.zeros(Lout, dtype=torch.bool, device="cuda")
    for ph in range(u):
        with launches(ops, force, 1):
            ops.conv(xa, phases[ph], pad=(0, T - 1), out_hw=(1, Q), out=out, remap=(u, ph - p, Lout))
        expect |= (t - (ph - p)) % u == 0
        nan = torch.isnan(out.view(B, Lout, N))
        assert torch.equal(nan.all(-1), nan.any(-1)), "a row was written in part"
        assert torch.equal(~nan.any(-1), expect[None].expand(B, Lout)), f"phase {ph} must write its own rows only"
    assert bool(expect.all()) and not bool(torch.isnan(out).any()), "polyphase left holes"
    assert guards_intact(big, out.numel()), "a launch wrote outside its output"
    e = rel_err(rows_ncl(out), ref, gemm_tol(), "polyphase")
    print(f"polyphase k={k} u={u} N={N} L={Lin} {FORCE_IDS[FORCES.index(force)]} [{ops.MMA_MODE}]: {e:.3e} (bar {gemm_tol():.0e})")
    assert e < gemm_tol()


# ---- 6. one whole stage, both forms, against the oracle ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_stage_case():
    from audioldm2_amd.hifigan import Generator
    from oracle import cases, weights
    from oracle.vae import hifigan_forward
    hc = cases.HIFIGAN_2STAGE
    sd = weights.make_state_dict(weights.shapes_of(Generator(dict(hc))), seed=11)
    mel = cases.mel_input(B, hc["num_mels"], 37, seed=3)
    with torch.no_grad():
        ref = hifigan_forward({k: v.double() for k, v in sd.items()}, hc, mel.double())
        ref32 = hifigan_forward(sd, hc, mel)
    return hc, sd, mel, ref, ref32


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3", "f16x3"])
def test_two_stage_generator_in_both_stage_forms_against_the_fp64_oracle(mode):
    """A two-stage Generator (384 -> 192 -> 96 channels, the 48 kHz ResBlocks, two samples of 37 frames): stage 0 takes _stage_dma,
    stage 1 the register-staged loop; with ops.set_dma(False) both take the latter.  The launch log shows which: 4 polyphase + 4 x 3
    x 2 ResBlock launches over pre-split operands in the first run, none in the second.  Both runs are within tail_tol of
    oracle.vae.hifigan_forward in fp64; torch's own fp32 evaluation of the oracle on the CPU is logged next to them (no bar: the
    figure fp32 arithmetic itself gives on this graph)."""
    from audioldm2_amd import ops
    from audioldm2_amd.hifigan import Generator
    hc, sd, mel, ref, ref32 = two_stage_case()
    nk = len(hc["resblock_kernel_sizes"])
    per_stage = [u + nk * 6 for u in hc["upsample_rates"]]
    prev = ops.set_mma(mode)
    prev_dma = ops.DMA_MODE
    try:
        gen = Generator(dict(hc))
        gen.load_state_dict(sd, strict=True)
        gen = gen.cuda().eval()
        assert gen.DMA_MIN_CHANNELS == 128
        errs = {}
        for dma in (True, False):
            ops.set_dma(dma)
            ops.TUNE_LOG, ops.PROFILE = [], []
            try:
                wave = gen(mel.cuda())
                torch.cuda.synchronize()
                log, prof = ops.TUNE_LOG, ops.PROFILE
            finally:
                ops.TUNE_LOG = ops.PROFILE = None
            assert len(log) == len(prof) == sum(per_stage) + 2
            presplit = [i for i, key in enumerate(log) if key.endswith((",dma", ",dma2"))]
            if dma:
                assert presplit == list(range(1, 1 + per_stage[0])), "stage 0 must run on pre-split operands, stage 1 must not"
                for i in presplit:
                    assert prof[i][6][9] == 1 and prof[i][7].startswith("igemm_dma"), (log[i], prof[i][7])
            else:
                assert not presplit and not any(p[6][9] for p in prof)
            assert tuple(wave.shape) == tuple(ref.shape)
            what = "two-stage generator, " + ("stage 0 pre-split" if dma else "register-staged")
            errs[dma] = rel_err(wave, ref, tail_tol(mode), what)
        e32 = rel_err(ref32, ref, 0.0, "two-stage generator, torch fp32 on the CPU")
        print(f"two-stage generator [{mode}] vs fp64 oracle: pre-split {errs[True]:.3e}, register-staged {errs[False]:.3e}, "
              f"torch fp32 {e32:.3e} (bar {tail_tol(mode):.0e})")
        assert errs[True] < tail_tol(mode) and errs[False] < tail_tol(mode)
    finally:
        ops.set_dma(prev_dma)
        ops.set_mma(prev)
