"""Shared by tests/test_loop_cpu.py and tests/test_loop_gpu.py (seamless loops: ring plans): the ring plan table, the
restatements of the wrap-around gather (torch.roll and a slice) and merge (a circular overlap-add in double precision), the model
wrapper built on the two, and the composition loops — windowed.py's and long_source.py's own, with that wrapper in the place of
windowed.WindowedModel.

The ring merge's bar is the linear merge's (windowed.py): an output element is sum_j wn_j e_j over at most `cover` windows, one
rounding per term, each at most 2^-24 of the sum of the terms' magnitudes: cover * 2^-24 of that sum, elementwise.
"""
from contextlib import contextmanager

import torch

import long_source as Ls
import windowed as Wd

# (T, Tw, hop) -> (W, starts, cover): the table of the ring plan's definition (W = ceil(T / hop), s_j = (j*T) // W)
RING_TABLE = {(16, 16, 8): (2, (0, 8), 2), (16, 16, 12): (2, (0, 8), 2), (40, 16, 10): (4, (0, 10, 20, 30), 2),
              (40, 16, 12): (4, (0, 10, 20, 30), 2), (24, 16, 1): (24, tuple(range(24)), 16), (256, 256, 192): (2, (0, 128), 2),
              (384, 256, 128): (3, (0, 128, 256), 2), (768, 256, 192): (4, (0, 192, 384, 576), 2),
              (320, 128, 96): (4, (0, 80, 160, 240), 2), (160, 64, 48): (4, (0, 40, 80, 120), 2)}
# hop == Tw, hop outside [1, Tw-1], T < Tw, non-multiples of 8, more than 32 windows
RING_REFUSED = [(40, 16, 16), (16, 16, 16), (40, 16, 0), (40, 16, 17), (40, 16, -3), (40, 16, 2.5), (40, 16, None), (8, 16, 4),
                (36, 16, 8), (40, 12, 8), (0, 16, 8), (8 * 40, 8, 1)]

# gather / merge cases (B, (T, Tw, hop), C, F): the scalar path with rows that straddle the waves; 24 windows, cover 16; T == Tw;
# the production plan; the mel
KERNEL_CASES = [(2, (40, 16, 10), 3, 5), (1, (24, 16, 1), 2, 7), (1, (16, 16, 8), 2, 16), (1, (768, 256, 192), 8, 16),
                (2, (160, 64, 48), 1, 64)]

# the sampler tests: the tiny model's long shape, plan and step count of tests/test_windowed_gpu.py and tests/long_source.py
LONG_KEY, STEPS, LONG_SHAPE = Ls.LONG_KEY, Ls.STEPS, Ls.LONG_SHAPE


def ring_plan(key, scale=1):
    from audioldm2_amd.windows import window_plan
    return window_plan(*key, scale=scale, ring=True)


def ring_gather_ref(x, plan):
    """torch.roll and a slice: window-major rows j*B + b, the frames (s_j + p) mod T."""
    return torch.cat([torch.roll(x, -s, dims=2)[:, :, :plan.Tw] for s in plan.starts]).contiguous()


def ring_merge_fp64(win, plan):
    """The circular overlap-add in fp64 on the fp32 inputs: win [..., W*B, C, Tw, F] -> (out [..., B, C, T, F], the sum of the
    magnitudes of the terms, the number of windows over every frame [T])."""
    win = win.double()
    W, Tw, T = plan.W, plan.Tw, plan.T
    B = win.shape[-4] // W
    shape = tuple(win.shape[:-4]) + (B,) + tuple(win.shape[-3:-2]) + (T, win.shape[-1])
    out = torch.zeros(shape, dtype=torch.float64, device=win.device)
    den = torch.zeros_like(out)
    count = torch.zeros(T, dtype=torch.int64)
    wn = plan.wn.double().to(win.device)
    for j, s in enumerate(plan.starts):
        frames = (s + torch.arange(Tw)) % T
        term = wn[j].view(Tw, 1) * win[..., j * B:(j + 1) * B, :, :, :]
        idx = frames.to(win.device)
        out.index_add_(-2, idx, term)
        den.index_add_(-2, idx, term.abs())
        count[frames] += 1
    return out, den, count


class RingModel(Wd.WindowedModel):
    """windowed.WindowedModel on a ring: roll and slice the long latent, run the same model on the W*b windows under the tiled
    conditioning, merge round the circle in fp64, round to fp32."""

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        assert prepared is None and self.plan.ring
        W, b = self.plan.W, x.shape[0]
        xw = ring_gather_ref(x.float(), self.plan)
        eps = self.inner.apply_model_cfg(xw, t2[:1].float().repeat(2 * W * b), Wd.tile(cond, W), Wd.tile(uncond, W))
        return ring_merge_fp64(eps, self.plan)[0].float().contiguous()


@contextmanager
def _ring_model():
    """The composition loops of windowed.py and long_source.py build `Wd.WindowedModel(inner, plan)`: inside this block they build
    a RingModel."""
    linear = Wd.WindowedModel
    Wd.WindowedModel = RingModel
    try:
        yield
    finally:
        Wd.WindowedModel = linear


def _on_ring(loop):
    def run(*args, **kw):
        with _ring_model():
            return loop(*args, **kw)
    run.__doc__ = f"{loop.__module__}.{loop.__name__} over RingModel."
    return run


ddim_loop, plms_loop, dpmpp_loop = _on_ring(Wd.ddim_loop), _on_ring(Wd.plms_loop), _on_ring(Wd.dpmpp_loop)
ddim_source_loop, plms_source_loop, dpmpp_source_loop = (_on_ring(Ls.ddim_source_loop), _on_ring(Ls.plms_source_loop),
                                                         _on_ring(Ls.dpmpp_source_loop))


def reach_by_hand(h):
    """The vocoder's one-sided reach in mel frames, from the formula of hifigan.reach_frames restated in floating point and NOT
    rounded up: conv_pre 3; per stage (k_up - 1) / c and, for the largest ResBlock kernel k, (sum_d d*(k-1)/2 + 3*(k-1)/2) / c, c the
    upsampling accumulated so far; conv_post 3 / c."""
    reach, c = 3.0, 1
    k = max(h["resblock_kernel_sizes"])
    ds = h["resblock_dilation_sizes"][list(h["resblock_kernel_sizes"]).index(k)]
    assert len(ds) == 3
    for u, ku in zip(h["upsample_rates"], h["upsample_kernel_sizes"]):
        c *= u
        reach += (ku - 1) / c + (sum(d * (k - 1) / 2 for d in ds) + 3 * (k - 1) / 2) / c
    return reach + 3 / c
