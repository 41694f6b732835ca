"""Case tables and input recipes of the launch-form tests of csrc/norm.hip (tests/test_norm_forms_cpu.py asserts what the tables
cover, tests/test_norm_forms_gpu.py runs them).  GroupNorm picks between a chunked two-launch form, a fused one-launch form and
the fused form with the operand split inside by batch size, pixel count and channel count (aldm_groupnorm_plan reports which);
LayerNorm between six instantiations by C (and $ALDM_LN_R); the row softmax stages a row of any length up to 60 KiB in LDS with 256
threads.  Importable without a GPU: torch on the CPU only, the plan query is host code."""
import math

import torch

GN_UNROLL = 8        # csrc/norm.hip: pixel loads in flight per thread; a thread's trips beyond a multiple of it run the tail loop
GN_SPREAD = 2.0      # standard deviation of the Gaussian part of the trend / spike recipes


class GnCase:
    """One GroupNorm shape with the form the current rule gives it for gn_stats (`form`) and for gn_split (`split_form`, None
    where aldm_groupnorm_split refuses the shape), the groups per block / column passes / data-holding threads it is in the table
    for, and an id."""

    def __init__(self, B, P, C1, C2, G, form, split_form, gpb, passes, active, why):
        self.B, self.P, self.C1, self.C2, self.G = B, P, C1, C2, G
        self.form, self.split_form, self.gpb, self.passes, self.active, self.why = form, split_form, gpb, passes, active, why

    @property
    def C(self):
        return self.C1 + self.C2

    @property
    def id(self):
        return f"B{self.B}-P{self.P}-C{self.C1}+{self.C2}-G{self.G}"

    def plan(self, want_split=False):
        from audioldm2_amd import ops
        return ops.groupnorm_plan(self.B, self.P, self.C1, self.C2, self.G, want_split)


# (the forms are those of the rule in csrc/norm.hip groupnorm_plan with $ALDM_GN_FUSED_MAX / $ALDM_GN_SPLIT_FUSED unset:
#  tests/test_norm_forms_cpu.py checks every row against the plan query)
GN_CASES = [
    GnCase(16, 16, 640, 0, 32, "fused", "fused_split", 2, 1, 160, "two groups per block, fewer pixels (16) than block rows (25)"),
    GnCase(32, 64, 256, 0, 32, "fused", "fused_split", 4, 1, 256, "four groups per block"),
    GnCase(32, 100, 640, 640, 32, "fused", "fused_split", 4, 1, 240, "four groups per block, 240 of 256 threads, slab of 160 split in the launch"),
    GnCase(32, 48, 1280, 1280, 32, "fused", "fused", 4, 1, 240, "four groups per block, slab of 320 > 256: fused statistics, then split_rows"),
    GnCase(16, 64, 384, 256, 32, "fused", "fused_split", 2, 1, 250, "the x1 / x2 seam inside group 19 and inside a block's slab"),
    GnCase(2, 256, 384, 256, 32, "chunked", "chunked", 1, 1, 160, "chunked, the same seam"),
    GnCase(64, 64, 128, 0, 32, "chunked", "chunked", 8, 1, 256, "B >= 64: eight groups per block fall through to one short chunk"),
    GnCase(1, 130, 640, 640, 32, "chunked", "chunked", 1, 2, 256, "two column passes, group 25 cut at column 256, last chunk of 2 pixels"),
    GnCase(2, 70, 1280, 1280, 32, "chunked", "chunked", 1, 3, 256, "three column passes, two cut groups"),
    GnCase(3, 1031, 128, 0, 32, "chunked", "chunked", 1, 1, 256, "P > 1024; the last chunk's 7 pixels are fewer than the 8 rows"),
    GnCase(2, 50, 132, 124, 32, "fused", None, 1, 1, 100, "statistics only: C1 % 8 != 0, the seam inside group 16"),
    GnCase(1, 300, 256, 0, 64, "fused", "fused", 1, 1, 256, "G = 64: one float4 column per block, 256 pixel rows"),
    GnCase(64, 40, 256, 0, 64, "chunked", "chunked", 16, 1, 256, "G = 64 chunked: 64 merging threads"),
    GnCase(2, 40, 2048, 0, 1, "fused", "fused", 1, 2, 256, "G = 1: a fused block walks two column passes"),
]

# one child process with ALDM_GN_FUSED_MAX=1048576 (the value until round 6): both run fused there, chunked by the default rule
GN_OVERRIDE_FUSED_MAX = 1048576
GN_OVERRIDE_SHAPES = [(16, 1024, 256), (2, 1024, 640)]

GN_RECIPES = ("trend", "mean1e2", "mean1e3", "spike")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_params(C):
    return torch.randn(C, generator=gen(2)), torch.randn(C, generator=gen(3))


def spike_positions(case, plan):
    """(pixel, channel) positions at which a kernel of this plan could lose an element: every pixel of interest with every
    channel of interest."""
    P, C, C1 = case.P, case.C, case.C1
    rows, chunk_px, chunks = plan["rows"], plan["chunk_px"], plan["chunks"]
    px = {0, P - 1}
    if chunks > 1:
        px |= {chunk_px - 1, (chunks - 1) * chunk_px}   # last pixel of a chunk, first pixel of the (ragged) last one
    for p0 in {0, (chunks - 1) * chunk_px}:             # the first tail trip of pixel row 0 in the first and in the last block
        p1 = min(P, p0 + chunk_px)
        trips = (p1 - p0 + rows - 1) // rows
        p = p0 + rows * GN_UNROLL * (trips // GN_UNROLL)
        if p < p1:
            px.add(p)
    ch = {0, C - 1}
    if case.C2:
        ch |= {C1 - 1, C1}
    # pass boundaries: the chunked block starts at column 0, a fused block at its slab
    slab = C if plan["form"] == "chunked" else plan["groups_per_block"] * (C // case.G)
    for lo in range(0, C, slab):
        for k in range(1, plan["passes"]):
            c = lo + 4 * plan["cols"] * k
            if c < min(C, lo + slab):
                ch |= {c - 1, c}
    return [(p, c) for p in sorted(px) for c in sorted(ch)]


def gn_input(case, recipe, rep=0, plan=None):
    """-> x [B, P, C] fp32 (CPU).  trend: Gaussian + per-channel offset + a ramp along the pixels, each about GN_SPREAD — partials
    of unequal count then differ in mean, so a merge with wrong weights misses far beyond the bar.  mean1e2 / mean1e3: the recipe of
    tests/test_ops_gpu.py test_groupnorm_stats_large_mean.  spike: Gaussian, and in sample b ONE element (position b + rep * B of
    spike_positions) raised by sqrt(n) GN_SPREAD, n the group's element count — the group's variance about doubles, a kernel that
    skips the element misses rstd by tens of percent."""
    B, P, C = case.B, case.P, case.C
    if recipe.startswith("mean"):
        ratio = float(recipe[4:])
        return torch.randn(B, P, C, generator=gen(1)) + ratio * (1 + torch.arange(C) % 7).float() / 4
    x = torch.randn(B, P, C, generator=gen(1)) * GN_SPREAD + 0.5
    if recipe == "trend":
        off = torch.randn(C, generator=gen(5)) * GN_SPREAD
        ramp = torch.linspace(-1.0, 1.0, P) * GN_SPREAD * 2 if P > 1 else torch.zeros(P)
        return x + off[None, None, :] + ramp[None, :, None]
    assert recipe == "spike"
    pos = spike_positions(case, plan)
    n = (C // case.G) * P
    for b in range(B):
        p, c = pos[(b + rep * B) % len(pos)]
        x[b, p, c] += math.sqrt(n) * GN_SPREAD
    return x


def spike_reps(case, plan):
    return (len(spike_positions(case, plan)) + case.B - 1) // case.B


def gn_reference(x, gamma, beta, G, eps=1e-5):
    """F.group_norm in fp64 on the fp32 inputs -> (normalised [B, P, C], rstd * gamma [B, C]), both fp64."""
    B, P, C = x.shape
    xd = x.double()
    ref = torch.nn.functional.group_norm(xd.permute(0, 2, 1), G, gamma.double(), beta.double(), eps=eps).permute(0, 2, 1)
    xg = xd.view(B, P, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    rstd = (xg.var(-1, unbiased=False) + eps).rsqrt().repeat_interleave(C // G, 1) * gamma.double()
    return ref, rstd


def group_rel_err(got, ref, G):
    """max over (sample, group) of max|got - ref| / max|ref| within it; got / ref [B, P, C] or [B, C].  Never below the max-norm
    over the whole tensor, and a wrong group cannot hide behind a larger value elsewhere (the spiked element is ~sqrt(n / 2))."""
    got, ref = got.double(), ref.double()
    if got.dim() == 2:
        got, ref = got[:, None, :], ref[:, None, :]
    B, P, C = ref.shape
    e = (got - ref).abs().view(B, P, G, C // G).amax((1, 3))
    r = ref.abs().view(B, P, G, C // G).amax((1, 3))
    return float((e / (r + 1e-30)).max())


# ---- LayerNorm / RMSNorm -----------------------------------------------------------------------------------------------------
# C: 4 and 100 (partly filled lane slots, one value slot), 256 (full), 260 / 512 / 516 (the one- / two-slot instantiations and
# their thresholds), 768 / 1024 (two rows per wave: odd M runs the clamped duplicate row), 1028 / 2048 (eight slots)
LN_C = (4, 100, 256, 260, 512, 516, 768, 1024, 1028, 2048)
LN_M = (1, 3, 7, 9)
LN_ENV_R = (2, 4)             # $ALDM_LN_R: the instantiations that are compiled and shipped but never the default
LN_ENV_C, LN_ENV_M = (128, 512), (1, 7, 9)


def ln_input(M, C, mean=0.3):
    x = torch.randn(M, C, generator=gen(1)) * 2 + mean
    return x + torch.arange(M, dtype=torch.float32)[:, None] * 0.25   # rows differ in mean: a row read twice or swapped shows


def ln_params(C):
    return torch.randn(C, generator=gen(2)), torch.randn(C, generator=gen(3))


# ---- row softmax -------------------------------------------------------------------------------------------------------------
# N: 1, below / at / above the 256 threads, not a multiple of 256, and the largest row the 60 KiB stage holds
SOFTMAX_N = (1, 63, 255, 256, 257, 1000, 15360)
SOFTMAX_N_REFUSED = 15361
SOFTMAX_REFUSAL = "exceeds the 60 KiB LDS stage"
