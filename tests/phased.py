"""Shared by tests/test_phase_cpu.py and tests/test_phase_gpu.py (moving window phases): the golden table restated, the
depth statistics of the equalisation claim, the bitwise identities of the three phased launches restated over tests/looped.py's
ring restatements and torch.roll, and the composition loops — the existing loops of tests/windowed.py, tests/long_source.py,
tests/resample.py and tests/graded.py over a model wrapper that, per UNet pass, rolls the long latent by -phi, runs
looped.RingModel and rolls the result back by +phi.

The identities (all bitwise): gather_phased(x, phi) == gather_ring(roll(x, -phi)); merge_phased(win, phi) == roll(merge_ring(win),
+phi); blend_gather_phased leaves in x what the ring sibling leaves and writes win == gather_ring(roll(x_after, -phi)).  The merge is
also held against the fp64 ring merge of the rolled problem at the project's bar, cover * 2^-24 of the sum of the terms' magnitudes
(tests/windowed.py).
"""
import numpy as np
import torch

import long_source as Ls
import looped as Lp

GOLDEN = 0.6180339887498949

# the rings of the equalisation claim (equal gaps), the schedule lengths, and the two bars of the issue
EQUAL_GAP_RINGS = [(768, 256, 192), (256, 256, 192), (40, 16, 10), (16, 16, 8)]
EQUALISE_STEPS = [10, 20, 50, 200]
WHOLE_BAR, HALF_BAR = 0.10, 0.15

# gather / merge / blend-gather cases (B, (T, Tw, hop), C, F): the scalar path; 24 windows, cover 16; T == Tw on the vector path; the mel
KERNEL_CASES = [(2, (40, 16, 10), 3, 5), (1, (24, 16, 1), 2, 7), (1, (16, 16, 8), 2, 16), (2, (160, 64, 48), 1, 64)]
ALL_PHASES = (0, 2)          # the cases checked at every phi in [0, T)

LONG_KEY, STEPS, LONG_SHAPE = Lp.LONG_KEY, Lp.STEPS, Lp.LONG_SHAPE
GOLDEN_6 = [0, 6, 2, 8, 4, 0]   # the golden table of the ring (40, 16, 10), gap 10, over six steps


def gap(plan):
    """The largest gap between a ring's starts, the wrap gap included — restated."""
    s = list(plan.starts)
    return max(b - a for a, b in zip(s, s[1:] + [plan.T]))


def golden_by_hand(G, steps):
    """phi_i = floor(frac(i * 0.6180339887498949) * G), in Python floats (fp64)."""
    out = []
    for i in range(steps):
        x = i * GOLDEN
        out.append(int(np.floor((x - np.floor(x)) * G)))
    return out


def phases_of(case_index, plan):
    """The phases a kernel case is checked at: every one on the first and third case, else no wrap, wrap by one and the last frame."""
    T, Tw, G = plan.T, plan.Tw, gap(plan)
    if case_index in ALL_PHASES:
        return list(range(T))
    return sorted({0, 1, G - 1, G, T - Tw, T - Tw + 1, T - 1} & set(range(T)))


def depth(plan, phi):
    """[T] the depth of every frame under phase phi: the maximum over its covering windows of min(p, Tw - 1 - p)."""
    T, Tw = plan.T, plan.Tw
    d = np.full(T, -1, dtype=np.int64)
    p = np.arange(Tw)
    inside = np.minimum(p, Tw - 1 - p)
    for s in plan.starts:
        fr = (s + phi + p) % T
        d[fr] = np.maximum(d[fr], inside)
    assert d.min() >= 0
    return d


def depth_spread(plan, phases):
    """max - min over the frames of the mean depth over the steps of `phases`."""
    m = np.mean([depth(plan, int(f)) for f in phases], axis=0)
    return float(m.max() - m.min())


def phased(key_or_plan, table):
    from audioldm2_amd.windows import with_phase
    plan = Lp.ring_plan(key_or_plan) if isinstance(key_or_plan, tuple) else key_or_plan
    return with_phase(plan, torch.as_tensor(table, dtype=torch.int32))


# ---- the identities, restated over the ring restatements ------------------------------------------------------------------------------
def gather_ref(x, plan, phi):
    return Lp.ring_gather_ref(torch.roll(x, -phi, dims=2), plan)


def merge_fp64(win, plan, phi):
    """The fp64 ring merge of the rolled problem -> (out, the sum of the terms' magnitudes), both rolled by +phi."""
    out, den, _ = Lp.ring_merge_fp64(win, plan)
    return torch.roll(out, phi, dims=-2), torch.roll(den, phi, dims=-2)


# ---- the composition loops -------------------------------------------------------------------------------------------------------------
class PhasedRingModel(Lp.RingModel):
    """looped.RingModel under moving phases: UNet pass number n of the run rolls the long latent by -passes[n], runs the ring model
    and rolls its output back by +passes[n].  `passes`: one phase per UNet PASS, in the order the sampler makes them."""

    def __init__(self, inner, plan, passes):
        super().__init__(inner, plan)
        self.passes, self.calls = [int(p) for p in passes], 0

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        phi = self.passes[self.calls]
        self.calls += 1
        eps = super().apply_model_cfg(torch.roll(x, -phi, dims=2).contiguous(), t2, cond, uncond, prepared)
        return torch.roll(eps, phi, dims=-2).contiguous()


def passes_of(name, table, visits=None):
    """The phase of every UNet pass of a run: one per step — per step VISIT with `visits` (resample.published_visits) — and PLMS's
    eager step 0 makes two, both under phase 0's entry."""
    table = [int(v) for v in table]
    if visits is not None:
        return [table[v[1]] for v in visits if v[0] == "step"]
    return ([table[0]] if name == "plms" else []) + table


def _over(model, loop):
    """Run one of the existing composition loops — they build `Wd.WindowedModel(inner, plan)` — with `model` in that place."""
    import windowed as Wd
    real = Wd.WindowedModel
    Wd.WindowedModel = lambda inner, plan: model
    try:
        out = loop()
    finally:
        Wd.WindowedModel = real
    assert model.calls == len(model.passes), "the loop made another number of UNet passes than the table was laid out for"
    return out


def sampler_loop(name, inner, plan, table, x_T, cond, uncond, steps, gs, guidance_rescale=0.0, eta=0.0):
    import windowed as Wd
    model = PhasedRingModel(inner, plan, passes_of(name, table))
    if name == "ddim":
        return _over(model, lambda: Wd.ddim_loop(inner, plan, x_T, cond, uncond, steps, gs, eta=eta,
                                                 guidance_rescale=guidance_rescale, k=len(table)))
    return _over(model, lambda: (Wd.plms_loop if name == "plms" else Wd.dpmpp_loop)(inner, plan, x_T, cond, uncond, steps))


def source_loop(name, inner, plan, table, x_T, x0, mask4, cond, uncond, steps, gs, guidance_rescale=0.0, eta=0.0):
    model = PhasedRingModel(inner, plan, passes_of(name, table))
    if name == "ddim":
        return _over(model, lambda: Ls.ddim_source_loop(inner, plan, x_T, x0, mask4, cond, uncond, steps, gs, eta=eta,
                                                        guidance_rescale=guidance_rescale, k=len(table)))
    return _over(model, lambda: (Ls.plms_source_loop if name == "plms" else Ls.dpmpp_source_loop)(inner, plan, x_T, x0, mask4, cond,
                                                                                                   uncond, steps))


def resample_loop(inner, plan, table, x_T, x0, mask4, cond, uncond, steps, resample, gs):
    import resample as Rs
    visits = Rs.published_visits(len(table), *resample)
    model = PhasedRingModel(inner, plan, passes_of("ddim", table, visits))
    out, n = Rs.resample_loop(model, x_T, x0, mask4, cond, uncond, steps, len(table), *resample, gs)
    assert model.calls == len(model.passes) and n == len(visits)
    return out


def graded_loop(inner, plan, table, x_T, x0, level4, cond, uncond, steps, gs):
    import graded as Gd
    model = PhasedRingModel(inner, plan, passes_of("ddim", table))
    out, _ = Gd.ddim_graded_loop(model, x_T, x0, level4, cond, uncond, steps, len(table), gs)
    assert model.calls == len(model.passes)
    return out
