"""Window plans of long-form generation (windowed diffusion: MultiDiffusion, Bar-Tal et al. 2023).  Pure host code.

A long latent [b, C, T, F] is denoised through W overlapping windows of the UNet's trained length Tw along the time axis: at every
step the windows are gathered (ops.window_gather), the UNet runs on the W*b window rows, and the window-wise outputs are fused by a
tapered, normalised overlap-add (ops.window_merge) before the sampler's update of the long latent.  The plan is everything the two
kernels need: the window starts and the normalised weights.

A plan may carry a source to keep (`with_source`, `keep_mask`): continuation and inpainting of long clips.  The
samplers then blend q_sample(source, t) into the long latent in front of every step's gather (ops.window_blend_gather).  The mask
may be a map of keep LEVELS (`keep_levels`, `with_source(..., graded=True)`): the samplers threshold it per step.

A linear plan may carry a prompt timeline (`prompt_weights`, `row_plan`, `PerPrompt`, `rows_cond`): every prompt has a
weight per latent frame, a window that sees several prompts becomes one ROW per prompt, the UNet runs on the rows — each under its
own prompt's conditioning — and the rows are fused per frame by taper times prompt weight (the `_rows` forms of the three launches).

A ring plan may carry moving window phases (`phase_table`, `with_phase`): at every sampler step all starts of the ring
are rotated by that step's phase, chosen on the device by the samplers' step counter (the `_ring_phased` forms of the three launches).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

MAX_WINDOWS = 32   # the size of `aldm_window_starts` (include/aldm_hip.h): the starts travel as kernel arguments


def _check_int(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"window_plan: {name} must be an integer, got {v!r}")
    return int(v)


def window_plan(T, Tw, hop, scale=1, ring=False):
    """The plan of windows of `Tw` frames, `hop` frames apart, over `T` frames -> an object with

      starts  s_j = j*hop while s_j + Tw < T, then a final T - Tw: s_0 = 0, the last window ends at T, consecutive starts differ
              by at most Tw; W = len(starts)
      wn      [W, Tw] fp32, the normalised weights: the raw taper w[p] = min(1, (p+1)/(ramp+1), (Tw-p)/(ramp+1)), ramp = Tw - hop
              (strictly positive), divided by the sum of the tapers of every window that covers the frame; fp64, rounded to
              fp32 once.  Where one window covers a frame wn is exactly 1.0
      cover   the largest number of windows over one frame
      T, Tw, hop, W, scale   the numbers the plan was built from, after scaling

    `scale` multiplies T, Tw and hop (and so the starts) first: the mel-domain plan of a latent-domain one (x4 for the 16 kHz VAE);
    its taper is the same formula on the scaled numbers.

    `ring=True`: a ring plan (seamless loops).  The T frames are a circle: W = ceil(T / hop) windows start at
    s_j = (j*T) // W — computed on the unscaled numbers, then scaled, so a mel plan's starts are exactly `scale` times the latent
    plan's — and window j covers the frames (s_j + p) mod T, p in [0, Tw): it may wrap from frame T-1 to frame 0, and the junction of
    end and start lies inside a window like every other frame boundary.  The gaps s_{j+1} - s_j (the last one T - s_{W-1}) are
    floor(T/W) or ceil(T/W), hence <= hop; the taper is the same formula with ramp = Tw - (the largest gap) >= 1, normalised by the
    circular sum of the tapers over every frame.  hop must lie in [1, Tw-1]; T == Tw is a legal ring (two half-shifted windows).
    The returned object carries `ring` (False for a linear plan).

    ValueError: T or Tw not a positive multiple of 8 (the UNet's three stride-2 levels), T < Tw, hop not an integer in [1, Tw]
    ([1, Tw-1] for a ring), more than 32 windows."""
    T, Tw, hop, scale = _check_int(T, "T"), _check_int(Tw, "Tw"), _check_int(hop, "hop"), _check_int(scale, "scale")
    for v, name in ((T, "T"), (Tw, "Tw")):
        if v <= 0 or v % 8 != 0:
            raise ValueError(f"window_plan: {name} must be a positive multiple of 8, got {v}")
    if T < Tw:
        raise ValueError(f"window_plan: T={T} is shorter than one window (Tw={Tw})")
    if not 1 <= hop <= Tw:
        raise ValueError(f"window_plan: hop must lie in [1, Tw={Tw}], got {hop}")
    if scale < 1:
        raise ValueError(f"window_plan: scale must be a positive integer, got {scale}")
    if ring:
        return _ring_plan(T, Tw, hop, scale)
    T, Tw, hop = T * scale, Tw * scale, hop * scale
    starts = []
    s = 0
    while s + Tw < T:
        starts.append(s)
        s += hop
        if len(starts) >= MAX_WINDOWS:
            raise ValueError(f"window_plan: T={T}, Tw={Tw}, hop={hop} needs more than {MAX_WINDOWS} windows")
    starts.append(T - Tw)
    W = len(starts)
    ramp = Tw - hop
    p = np.arange(Tw, dtype=np.float64)
    w = np.minimum(1.0, np.minimum((p + 1.0) / (ramp + 1.0), (Tw - p) / (ramp + 1.0)))
    norm = np.zeros(T, dtype=np.float64)
    count = np.zeros(T, dtype=np.int64)
    for s in starts:
        norm[s:s + Tw] += w
        count[s:s + Tw] += 1
    wn = np.stack([w / norm[s:s + Tw] for s in starts])
    # one window over a frame: w / w — exactly 1 in fp64 already; stated here because the kernels' bit-exact cases rest on it
    assert all(np.all(wn[j][count[s:s + Tw] == 1] == 1.0) for j, s in enumerate(starts))
    return SimpleNamespace(T=T, Tw=Tw, hop=hop, scale=scale, W=W, starts=tuple(starts), cover=int(count.max()), ring=False,
                           wn=torch.from_numpy(wn.astype(np.float32)).contiguous())


def _ring_plan(T, Tw, hop, scale):
    """window_plan's ring form, on the checked, unscaled numbers."""
    if hop == Tw:
        raise ValueError(f"window_plan: a ring needs hop < Tw={Tw}: with hop == Tw the windows do not overlap, the junction of the "
                         "clip's end and start lies between two windows and nothing denoises across it")
    W = -(-T // hop)
    if W > MAX_WINDOWS:
        raise ValueError(f"window_plan: a ring of T={T}, Tw={Tw}, hop={hop} needs more than {MAX_WINDOWS} windows")
    starts = [((j * T) // W) * scale for j in range(W)]
    T, Tw, hop = T * scale, Tw * scale, hop * scale
    gaps = [b - a for a, b in zip(starts, starts[1:] + [T])]
    ramp = Tw - max(gaps)
    assert W >= 2 and starts[0] == 0 and min(gaps) >= 1 and max(gaps) <= hop and ramp >= 1
    p = np.arange(Tw, dtype=np.float64)
    w = np.minimum(1.0, np.minimum((p + 1.0) / (ramp + 1.0), (Tw - p) / (ramp + 1.0)))
    frames = [(s + np.arange(Tw)) % T for s in starts]     # Tw <= T: a window covers no frame twice
    norm = np.zeros(T, dtype=np.float64)
    count = np.zeros(T, dtype=np.int64)
    for fr in frames:
        norm[fr] += w
        count[fr] += 1
    wn = np.stack([w / norm[fr] for fr in frames])
    # one window over a frame: w / w, exactly 1 in fp64 already (the merge kernel's bit-exact frames rest on it)
    assert int(count.min()) >= 1 and all(np.all(wn[j][count[fr] == 1] == 1.0) for j, fr in enumerate(frames))
    return SimpleNamespace(T=T, Tw=Tw, hop=hop, scale=scale, W=W, starts=tuple(starts), cover=int(count.max()), ring=True,
                           wn=torch.from_numpy(wn.astype(np.float32)).contiguous())


def plan_key(plan):
    """What identifies a plan's launch sequence (the starts are kernel arguments captured with a step graph; a ring plan launches
    the wrap-around kernels, so a ring and a linear plan never share a step graph).  A row plan (row_plan, prompt timelines) launches
    the row kernels with its row starts: (T, Tw, row_starts, "rows"), distinct from every linear and ring key — its weights are NOT
    part of the key: they live in a static buffer of the step graph's cache entry, refilled per job."""
    if has_rows(plan):
        return (plan.T, plan.Tw, tuple(plan.row_starts), "rows")
    if has_phase(plan):
        # moving window phases (with_phase): the phased ring kernels, distinct from every linear, ring and row key.  The table's
        # VALUES are not part of the key: they live in a static buffer of the step graph's cache entry, refilled per job
        return (plan.T, plan.Tw, tuple(plan.starts), "phased")
    return (plan.T, plan.Tw, tuple(plan.starts), bool(getattr(plan, "ring", False)))


# ---- moving window phases: a ring's starts rotated by a per-step phase ------------------------------------------------
GOLDEN = 0.6180339887498949   # frac of the golden ratio: the additive recurrence with the lowest discrepancy


def has_phase(plan):
    """True for a ring plan that carries a phase table (with_phase): its launches are the `_ring_phased` kernels."""
    return getattr(plan, "phase", None) is not None


def ring_gap(plan):
    """The largest gap between a ring plan's starts, the wrap gap T - s_{W-1} included."""
    if not getattr(plan, "ring", False):
        raise ValueError("ring_gap: not a ring plan (window_plan(..., ring=True))")
    s = list(plan.starts)
    return max(b - a for a, b in zip(s, s[1:] + [plan.T]))


def phase_table(plan, steps, phase="golden"):
    """The per-step window phases of a ring plan -> int32 [steps] (host): at sampler step i every window start is rotated by
    phi_i frames, window j covering the frames (s_j + phi_i + p) mod T.

      phase="golden"   phi_i = floor(frac(i * 0.6180339887498949) * G) in fp64, G = ring_gap(plan): phi_0 = 0, every value in
                       [0, G) — a rotation by a whole gap maps an equal-gap ring onto itself — and neighbouring steps far apart.
                       Deterministic: no draw from any generator.
      phase=[...]      one integer (latent frames) per sampler step, reduced mod T here; the length must be `steps`.

    ValueError: a plan that is not a ring or has rows, steps not a positive integer, an unknown string, entries that are not
    integers, a wrong length."""
    if not getattr(plan, "ring", False) or has_rows(plan):
        raise ValueError("phase_table: moving window phases need a ring plan (window_plan(..., ring=True)): a rotation changes a "
                         "linear plan's gaps and with them its normalisation")
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError(f"phase_table: steps must be a positive integer, got {steps!r}")
    steps = int(steps)
    if isinstance(phase, str):
        if phase != "golden":
            raise ValueError(f"phase_table: unknown phase schedule {phase!r}: 'golden', or a list of one integer per step")
        x = np.arange(steps, dtype=np.float64) * GOLDEN
        vals = np.floor((x - np.floor(x)) * float(ring_gap(plan))).astype(np.int64)
    else:
        try:
            seq = list(phase)
        except TypeError:
            raise ValueError(f"phase_table: phase must be 'golden' or a sequence of integers (latent frames), got {phase!r}")
        for v in seq:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"phase_table: a phase must be an integer number of latent frames, got {v!r}")
        if len(seq) != steps:
            raise ValueError(f"phase_table: {len(seq)} phases for a run of {steps} steps: one per sampler step")
        vals = np.asarray([int(v) % plan.T for v in seq], dtype=np.int64)
    return torch.from_numpy(vals.astype(np.int32))


def with_phase(plan, table):
    """`plan` with moving window phases: a copy of the ring plan that carries `phase`, the int32 [steps] table of
    phase_table — one entry per sampler step of the run it is given to, reduced mod T here (the kernels clamp, they do not wrap).
    Same T, Tw, starts and wn; the plan_key becomes (T, Tw, starts, "phased").  Composes with with_source in either order.
    ValueError: a plan that is not a ring, a row plan, a table that is not a 1-D integer tensor (or sequence), a length of 0."""
    if has_rows(plan):
        raise ValueError("with_phase: a row plan (a prompt timeline) cannot carry a phase: row plans are linear")
    if not getattr(plan, "ring", False):
        raise ValueError("with_phase: moving window phases need a ring plan (window_plan(..., ring=True)): a rotation changes a "
                         "linear plan's gaps and with them its normalisation")
    if not torch.is_tensor(table):
        try:
            table = torch.as_tensor(np.asarray(table))
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"with_phase: the table must be a 1-D integer tensor, got {type(table).__name__}")
    if table.dim() != 1 or table.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"with_phase: the table must be a 1-D integer tensor, got {table.dtype} {tuple(table.shape)}")
    if table.numel() == 0:
        raise ValueError("with_phase: the table is empty: one phase per sampler step")
    table = torch.remainder(table.detach().cpu().to(torch.int64), plan.T).to(torch.int32).contiguous()
    return SimpleNamespace(**dict(plan.__dict__, phase=table))


# ---- prompt timelines: per-frame prompt weights, rows = (window, prompt) pairs -----------------------------------------
MAX_ROWS = 64   # the size of `aldm_window_rows` (include/aldm_hip.h)


def has_rows(plan):
    """True for a row plan (row_plan): its launches are the `_rows` kernels and its UNet pass has plan.R row groups, not plan.W."""
    return getattr(plan, "rows", None) is not None


def prompt_weights(T, boundaries, transition=0.0):
    """The prompt weights m [K, T] (numpy fp64) of a timeline of K = len(boundaries) + 1 prompts over T latent frames: prompt k
    sounds between the boundaries beta_k and beta_{k+1} (latent frames, possibly fractional, ascending, inside (0, T)) and cross-fades
    into its neighbours over `transition` frames centred on the boundary.  With frame centres t + 0.5:

      u_0 = 1, u_K = 0, u_k(t) = clip((t + 0.5 - beta_k) / transition + 0.5, 0, 1)   (transition == 0: 1 if t + 0.5 >= beta_k else 0)
      m_k = u_k - u_{k+1}

    non-negative, summing to 1 over k at every frame, exactly 1.0 or 0.0 outside the transitions.  ValueError: T not a positive
    integer, boundaries not finite, not strictly ascending or outside (0, T), a negative or non-finite transition, a prompt whose
    weight is zero at every frame (two boundaries with no frame centre between them and a transition too short to reach one)."""
    T = _check_int(T, "T")
    if T <= 0:
        raise ValueError(f"prompt_weights: T must be positive, got {T}")
    try:
        beta = [float(b) for b in boundaries]
        tau = float(transition)
    except (TypeError, ValueError):
        raise ValueError(f"prompt_weights: boundaries and transition must be numbers (latent frames), got {boundaries!r}, {transition!r}")
    if not np.isfinite(tau) or tau < 0.0:
        raise ValueError(f"prompt_weights: transition must be finite and >= 0 latent frames, got {transition!r}")
    for i, b in enumerate(beta):
        if not np.isfinite(b) or not 0.0 < b < T:
            raise ValueError(f"prompt_weights: a boundary must lie inside (0, T={T}), got {b!r}")
        if i > 0 and b <= beta[i - 1]:
            raise ValueError(f"prompt_weights: boundaries must ascend strictly, got {beta!r}")
    K = len(beta) + 1
    centre = np.arange(T, dtype=np.float64) + 0.5
    u = np.zeros((K + 1, T), dtype=np.float64)
    u[0] = 1.0
    for k, b in enumerate(beta, start=1):
        u[k] = np.clip((centre - b) / tau + 0.5, 0.0, 1.0) if tau > 0.0 else (centre >= b).astype(np.float64)
    m = u[:-1] - u[1:]
    assert float(m.min()) >= 0.0
    for k in range(K):
        if not np.any(m[k] != 0.0):
            raise ValueError(f"prompt_weights: prompt {k} has no frame: its weight is zero over all T={T} frames (boundaries "
                             f"{beta!r}, transition {tau})")
    return m


def row_plan(plan, m):
    """The row plan of a linear window plan under the prompt weights `m` [K, T] (prompt_weights).  A ROW is a pair
    (window j, prompt k) with m_k != 0 somewhere inside window j, ordered by j, then k: the UNet runs once per row, under the row's
    prompt, and the rows are fused per latent frame.  -> an object with the base plan's fields (T, Tw, hop, scale, W, starts, ring,
    wn — and x0 / mask of a plan with a source) plus

      base        the plan without rows (no prompts enter the window-wise VAE tail, which runs on it); a source stays on the row plan
      rows        ((j, k), ...);  R = len(rows) <= 64
      row_starts  s_j of every row: non-decreasing, equal starts = one window under several prompts
      row_prompt  k of every row
      wr          [R, Tw] fp32: taper_j[p] * m_k[s_j + p] divided by the sum of that product over every row on the frame, in fp64,
                  rounded to fp32 once.  Over every frame the rows' weights sum to 1; where one row alone has weight on a frame wr is
                  exactly 1.0, where the row's prompt is silent exactly 0.0; K == 1: wr == plan.wn bitwise and row_starts == starts
      cover       the largest number of rows with non-zero weight on one frame

    ValueError: a ring plan, m not [K, plan.T], negative or not summing to 1, a prompt with no frame, more than 64 rows."""
    if getattr(plan, "ring", False):
        raise ValueError("row_plan: a ring plan cannot carry a timeline (a loop has no first prompt); use a linear window_plan")
    if has_rows(plan):
        raise ValueError("row_plan: the plan already has rows; build them from its base plan")
    m = np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] != plan.T:
        raise ValueError(f"row_plan: m must be [K, T={plan.T}] prompt weights, got {m.shape}")
    if not np.all(np.isfinite(m)) or float(m.min()) < 0.0 or float(np.abs(m.sum(0) - 1.0).max()) > 1e-9:
        raise ValueError("row_plan: prompt weights must be finite, non-negative and sum to 1 at every frame (prompt_weights)")
    K, T, Tw = m.shape[0], plan.T, plan.Tw
    for k in range(K):
        if not np.any(m[k] != 0.0):
            raise ValueError(f"row_plan: prompt {k} has no frame: its weight is zero over all T={T} frames")
    rows = [(j, k) for j, s in enumerate(plan.starts) for k in range(K) if np.any(m[k, s:s + Tw] != 0.0)]
    if len(rows) > MAX_ROWS:
        raise ValueError(f"row_plan: {len(rows)} rows (windows under prompts), at most {MAX_ROWS}: use fewer prompts, a shorter "
                         "transition or a larger hop")
    # the raw taper of window_plan, on the plan's own (scaled) numbers.  Numerators taper * m, the denominator their sum over the
    # rows in row order: with K == 1 the numerators are the tapers and the sums window_plan's own, term for term, so wr == wn bitwise
    p = np.arange(Tw, dtype=np.float64)
    ramp = Tw - plan.hop
    w = np.minimum(1.0, np.minimum((p + 1.0) / (ramp + 1.0), (Tw - p) / (ramp + 1.0)))
    num = [w * m[k, plan.starts[j]:plan.starts[j] + Tw] for j, k in rows]
    norm = np.zeros(T, dtype=np.float64)
    count = np.zeros(T, dtype=np.int64)
    for (j, k), a in zip(rows, num):
        s = plan.starts[j]
        norm[s:s + Tw] += a
        count[s:s + Tw] += a != 0.0
    assert float(norm.min()) > 0.0 and int(count.min()) >= 1
    wr64 = np.stack([a / norm[plan.starts[j]:plan.starts[j] + Tw] for (j, k), a in zip(rows, num)])
    for r, (j, k) in enumerate(rows):
        s = plan.starts[j]
        # one row alone on a frame: a / a, exactly 1; a silent prompt: 0 / norm, exactly 0 (the merge kernel's skip rests on it)
        assert np.all(wr64[r][(count[s:s + Tw] == 1) & (num[r] != 0.0)] == 1.0) and np.all(wr64[r][num[r] == 0.0] == 0.0)
    wr = torch.from_numpy(wr64.astype(np.float32)).contiguous()
    if K == 1:
        assert torch.equal(wr, plan.wn)
    fields = {k: v for k, v in plan.__dict__.items() if not k.startswith("_")}
    base = SimpleNamespace(**{k: v for k, v in fields.items() if k not in ("x0", "mask")})
    return SimpleNamespace(**dict(fields, base=base, rows=tuple(rows), R=len(rows), row_starts=tuple(plan.starts[j] for j, _ in rows),
                                  row_prompt=tuple(k for _, k in rows), wr=wr, cover=int(count.max())))


class PerPrompt:
    """K conditionings, one per prompt of a timeline, in timeline order: the `cond` of a sampler run over a row plan.  A marker class:
    a conditioning is already a tuple, list or dict of tensors in this code base, so a bare list of them would be ambiguous."""

    def __init__(self, conds):
        conds = list(conds)
        if not conds:
            raise ValueError("PerPrompt: at least one conditioning")
        self.conds = conds

    def __len__(self):
        return len(self.conds)


def _cat_rows(cs):
    c = cs[0]
    if c is None:
        return None
    if torch.is_tensor(c):
        return torch.cat(list(cs), dim=0)
    if isinstance(c, dict):
        return {k: _cat_rows([x[k] for x in cs]) for k in c}
    if isinstance(c, (list, tuple)):
        return type(c)(_cat_rows([x[i] for x in cs]) for i in range(len(c)))
    return c


def check_per_prompt(cond, plan, what="windows="):
    """A row plan wants a PerPrompt of K = max(row_prompt) + 1 conditionings, every other plan (or none) anything else."""
    rows = plan is not None and has_rows(plan)
    if isinstance(cond, PerPrompt) != rows:
        raise ValueError(f"{what}: a row plan (windows.row_plan) and a PerPrompt conditioning go together: got "
                         f"{'a row plan' if rows else 'no row plan'} with {type(cond).__name__}")
    if rows and len(cond) != max(plan.row_prompt) + 1:
        raise ValueError(f"{what}: the row plan has {max(plan.row_prompt) + 1} prompts, the PerPrompt conditioning {len(cond)}")


def rows_cond(per_prompt, plan):
    """The conditioning of a row plan's UNet pass, row-major like ops.window_gather's rows: rows r*b + i, i in [0, b), are prompt
    plan.row_prompt[r]'s conditioning (its b samples).  Tensors inside lists, tuples and dicts, None passing through."""
    check_per_prompt(per_prompt, plan, "rows_cond")
    return _cat_rows([per_prompt.conds[k] for k in plan.row_prompt])


def keep_mask(T, intervals):
    """The [T] fp32 0/1 vector of a source's kept frames: 1 inside the half-open latent-frame intervals [a, b) of `intervals`, 0
    elsewhere (1 = keep the source, 0 = generate).  The intervals must be integer pairs with 0 <= a < b <= T, in ascending order,
    and may touch but not overlap.  ValueError otherwise."""
    T = _check_int(T, "T")
    m = torch.zeros(T, dtype=torch.float32)
    end = 0
    for iv in intervals:
        try:
            a, b = iv
        except (TypeError, ValueError):
            raise ValueError(f"keep_mask: an interval must be a pair (start, end) of latent frames, got {iv!r}")
        for v in (a, b):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"keep_mask: interval bounds must be integers (latent frames), got {iv!r}")
        a, b = int(a), int(b)
        if a >= b:
            raise ValueError(f"keep_mask: the interval [{a}, {b}) is empty")
        if a < 0 or b > T:
            raise ValueError(f"keep_mask: the interval [{a}, {b}) leaves [0, {T})")
        if a < end:
            raise ValueError(f"keep_mask: the interval [{a}, {b}) starts before the previous one ends ({end}): intervals must be "
                             "ordered and may not overlap")
        m[a:b] = 1.0
        end = b
    return m


def keep_levels(T, intervals, feather=0, ring=False):
    """The [T] fp32 vector of a source's keep LEVELS (graded keep, differential diffusion): a frame of level m is
    held on the noised source for about the first m*S of a run's S steps and is free afterwards (sampling.hold_steps) — 1 is
    keep_mask's keep, 0 its generate.  `intervals`: (a, b) or (a, b, level), half-open latent-frame intervals under keep_mask's
    rules (integers, 0 <= a < b <= T, ascending, may touch, may not overlap), level a finite number with 0 < level <= 1, default 1.
    Inside an interval the value is its level.  `feather` (an integer, 0 <= feather < T) fades every interval out over that many
    frames on either side: a frame outside every interval, at distance d from interval I (d = a - t left of it, t - (b - 1) right
    of it; with ring=True the shorter way round the circle of T frames), gets max over I of level_I * max(0, 1 - d / (feather + 1)).
    fp64, rounded to fp32 once.  With every level 1 and feather == 0 the result is keep_mask(T, intervals).  ValueError otherwise."""
    T = _check_int(T, "T")
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)) or not 0 <= feather < T:
        raise ValueError(f"keep_levels: feather must be an integer number of latent frames in [0, T={T}), got {feather!r}")
    ivs = []
    for iv in intervals:
        try:
            n = len(iv)
        except TypeError:
            n = 0
        if n not in (2, 3):
            raise ValueError(f"keep_levels: an interval must be (start, end) or (start, end, level), got {iv!r}")
        level = 1.0
        if n == 3:
            level = iv[2]
            if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, float, np.integer, np.floating)) \
                    or not (np.isfinite(level) and 0.0 < level <= 1.0):
                raise ValueError(f"keep_levels: a level must be a finite number in (0, 1], got {iv!r}")
        ivs.append((iv[0], iv[1], float(level)))
    keep_mask(T, [iv[:2] for iv in ivs])   # the intervals themselves: keep_mask's rules and messages (integer bounds from here on)
    t = np.arange(T, dtype=np.int64)
    out = np.zeros(T, dtype=np.float64)
    for a, b, level in ivs:
        left, right = a - t, t - (b - 1)
        if ring:
            d = np.minimum(left % T, right % T)
        else:
            d = np.where(t < a, left, right)
        inside = (t >= a) & (t < b)
        v = level * np.maximum(0.0, 1.0 - d.astype(np.float64) / (int(feather) + 1.0))
        out = np.maximum(out, np.where(inside, 0.0, v))
    for a, b, level in ivs:
        out[a:b] = level
    return torch.from_numpy(out.astype(np.float32))


def with_source(plan, x0, mask, graded=False):
    """`plan` with a source to keep (continuation and inpainting of long clips): a plan object with the same T, Tw,
    starts, ring flag and wn — and so the same plan_key — that additionally carries `x0` [b, C, T, F] (the source's scaled latent)
    and `mask` (broadcastable to x0's shape; 1 = keep the source, 0 = generate; a [T] vector, as keep_mask returns it, is taken along the time
    axis).  A sampler given such a plan as `windows=` blends q_sample(x0, t) into the long latent in front of every step's gather
    (ops.window_blend_gather).  `graded=True` declares the mask a map of keep LEVELS in [0, 1] (keep_levels): the
    sampler thresholds it per step into the binary mask the blend reads; the flag rides on the plan, the plan_key is unchanged.
    ValueError for shapes that do not fit plan.T."""
    if not torch.is_tensor(x0) or x0.dim() != 4 or x0.shape[2] != plan.T:
        raise ValueError(f"with_source: x0 must be a tensor [b, C, T={plan.T}, F], got "
                         f"{tuple(x0.shape) if torch.is_tensor(x0) else type(x0).__name__}")
    if not torch.is_tensor(mask):
        raise ValueError(f"with_source: mask must be a tensor, got {type(mask).__name__}")
    if mask.dim() == 1:
        if mask.shape[0] != plan.T:
            raise ValueError(f"with_source: a 1-D mask is one entry per latent frame, T={plan.T}, got {tuple(mask.shape)}")
        mask = mask.view(1, 1, plan.T, 1)
    try:
        ok = tuple(torch.broadcast_shapes(tuple(mask.shape), tuple(x0.shape))) == tuple(x0.shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"with_source: mask {tuple(mask.shape)} does not broadcast to x0 {tuple(x0.shape)}")
    return SimpleNamespace(**dict(plan.__dict__, x0=x0, mask=mask, graded=bool(graded)))


def device_weights(plan, device):
    """plan.wn — a row plan's plan.wr — on `device`, uploaded once per plan and device."""
    cache = plan.__dict__.setdefault("_wn_dev", {})
    key = str(device)
    if key not in cache:
        cache[key] = (plan.wr if has_rows(plan) else plan.wn).to(device).contiguous()
    return cache[key]


def tile_cond(c, W):
    """A conditioning (a tensor, or lists / tuples / dicts of them, None passing through) repeated for W windows, window-major:
    row j*b + i is sample i's — the order pipeline._tile_cond gives candidates, and ops.window_gather gives window rows."""
    if c is None:
        return None
    if torch.is_tensor(c):
        return torch.cat([c] * W, dim=0)
    if isinstance(c, dict):
        return {k: tile_cond(v, W) for k, v in c.items()}
    if isinstance(c, (list, tuple)):
        return type(c)(tile_cond(v, W) for v in c)
    return c
