"""What the three samplers share (ddim.DDIMSampler, plms.PLMSSampler, dpm_solver.DPMSolverSampler): the host side of a sampling
run that is the same whichever update rule runs.

  * SamplerBase: the constructor, DDIM's timestep grid and abar tables (`make_schedule`), the run plan (`plan_run`: the cut of the
    schedule, the start latent, the device tables, the inpainting buffers, the batched guidance conditioning) and the UNet pass of
    one step (`model_output`) — with a window plan (`windows=`, windows.py) the pass on the windows of a long latent
    between a window gather and a window merge;
  * ddim_step_rows: the [S, 5] coefficient rows of DDIM's update with the reference's roundings (DDIM and PLMS), guidance_table:
    a sampler's [S, 8] table from its rows;
  * GraphStepper / drop_graph_entries: a fixed launch sequence run eagerly once, captured into a HIP graph, replayed;
  * host_drawer / _NoiseFeed: the host generator's draws in the reference's order (RNG contract);
  * check_guidance_rescale / check_t_start: the two per-run options every sampler takes; log_step: the tail of every step;
  * resample_visits / renoise_coef / check_resample: the visit schedule and the forward-jump coefficients of resampled inpainting
    (RePaint's jumps, `resample=(n, jump)`), which plan_run turns into per-visit tables for DDIM's loop;
  * keep_thresholds / hold_steps / check_levels: the per-step thresholds of graded keep levels (`graded=True`, differential
    diffusion) and what a level means in steps; plan_run keeps the level map and the threshold rows on the device;
  * Composed / compose_table / check_compose_weights: K weighted conditionings on the same frames (composable guidance, DESIGN.md
    9m) and their [V, K+1] coefficient table; model_output reduces the K+1 predictions of the group pass to the pair in one launch.

What differs between the samplers stays in their modules: DDIM's graph cache on the UNet and its threaded noise feed, PLMS's eager
Euler step 0 and its discarded `noise_like` draws, DPM-Solver++'s table per sub-range.  ddim.py re-exports every name that lived
there before this module existed.
"""
from __future__ import annotations

import gc
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    """util.py:55-75"""
    if ddim_discr_method == "uniform":
        c = num_ddpm_timesteps // num_ddim_timesteps
        ddim_timesteps = np.asarray(list(range(0, num_ddpm_timesteps, c)))
    elif ddim_discr_method == "quad":
        ddim_timesteps = ((np.linspace(0, np.sqrt(num_ddpm_timesteps * 0.8), num_ddim_timesteps)) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    return ddim_timesteps + 1


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    """util.py:78-95 — keeps the reference's mixed float32-tensor / float64-ndarray arithmetic:
    (1 - alphas) is a float32 tensor op, the rest float64."""
    alphas = alphacums[ddim_timesteps]
    alphas_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist())
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - alphas) * (1 - alphas / alphas_prev))
    return torch.as_tensor(np.asarray(sigmas, dtype=np.float64)), alphas, alphas_prev


class GraphStepper:
    """Runs a fixed launch sequence repeatedly: eagerly the first time (packs weights, warms the
    allocator, grows the split-K workspace), captured into a HIP graph the second time, replayed after.
    The callable must read its per-step inputs from static device buffers."""

    def __init__(self, fn, use_graph=True):
        self.fn, self.use_graph, self.calls, self.graph = fn, use_graph, 0, None

    def __call__(self):
        if self.use_graph and self.calls >= 1:
            if self.graph is None:
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                # No cyclic garbage collection while the stream is capturing: a collection that happens to run inside the
                # capture can finalise objects of EARLIER jobs (an evicted step graph, a noise feed's side stream and pinned
                # buffers) whose destructors call HIP functions that are illegal during capture — the C++ destructor then
                # throws and the process aborts ("Fatal Python error: Aborted ... Garbage-collecting" a few tests into a
                # long session, at a different place every time).  Collect first, then hold the collector off.
                gc.collect()
                gc_was_on = gc.isenabled()
                gc.disable()
                try:
                    # thread_local: other threads (e.g. the RCCL watchdog of a multi-GPU run) may keep
                    # calling HIP while this thread captures
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        self.fn()
                    self.graph = g
                except RuntimeError as e:  # capture refused: keep sampling eagerly, say so once
                    import sys
                    print(f"[audioldm2_amd] HIP graph capture failed ({e}); continuing without a graph",
                          file=sys.stderr, flush=True)
                    self.use_graph = False
                    torch.cuda.synchronize()
                    if gc_was_on:
                        gc.enable()
                    self.fn()
                    self.calls += 1
                    return
                finally:
                    if gc_was_on:
                        gc.enable()
            self.graph.replay()
        else:
            self.fn()
        self.calls += 1

    def release(self):
        """Break the reference cycle stepper -> step closure -> stepper, so the graph, its private memory pool and its static
        buffers go by reference counting NOW and not with a later cyclic collection, which may run in the middle of the next
        capture (see __call__).  Call it where no stream is capturing and no replay is in flight."""
        self.fn = None
        self.graph = None


def drop_graph_entries(cache: dict) -> None:
    """Evict cached step graphs NOW, by reference counting: an entry is a reference cycle (entry -> stepper -> step closure ->
    entry), so simply forgetting it leaves the HIP graph to the cyclic collector (see GraphStepper.release).  Breaking the cycle
    here frees it at a point where no stream is capturing."""
    for ent in list(cache.values()):
        rs = ent.get("run_step")
        if rs is not None:
            rs.release()
        ent.clear()
    cache.clear()


class _NoiseFeed:
    """Streams the per-step host noise to the GPU in chunks.  A DRAWER THREAD consumes the CPU generator (the reference's RNG
    stream, strictly in its order: only this thread draws while a sampling run is in flight) into pinned staging rows and
    issues the PCIe uploads on a side stream, running up to `len(pin)` chunks ahead of the GPU; the launching thread only
    makes its stream wait for a chunk's upload event (`wait(i)`).  Round 2 drew on the launching thread between graph replays:
    with prompt sharding every rank draws the GLOBAL batch (7 ms per step at 8 ranks x 8 prompts against a 16 ms GPU step,
    profiles/r02_host_noise_cost.txt) — one kernel speed-up away from bounding the job.  `torch.randn` releases the GIL.
    Device buffers hold all steps (`noise_buf` / `qnoise_buf`: write into these — the static inputs of a cached step graph —
    instead of allocating); `close()` joins the thread: after it the generator is where the reference leaves it."""

    def __init__(self, draw, steps, shape, with_mask, temperature, dev, chunk=8, mask_first=True, noise_buf=None,
                 qnoise_buf=None, threaded=None):
        import threading
        self.draw, self.steps, self.with_mask, self.temperature = draw, steps, with_mask, temperature
        self.mask_first = mask_first  # DDIM draws the q_sample noise before the step noise, DDPM after
        # chunk boundaries: the first chunk is ONE step so the GPU starts right away, then `chunk` steps
        self.bounds = [0, min(1, steps)]
        while self.bounds[-1] < steps:
            self.bounds.append(min(steps, self.bounds[-1] + chunk))
        self.chunk = chunk
        self.noise = noise_buf if noise_buf is not None else torch.empty((steps,) + tuple(shape), device=dev,
                                                                         dtype=torch.float32)
        assert self.noise.shape == (steps,) + tuple(shape)
        self.qnoise = (qnoise_buf if qnoise_buf is not None else torch.empty_like(self.noise)) if with_mask else None
        nbuf = 3
        self.pin = [torch.empty((chunk,) + tuple(shape)).pin_memory() for _ in range(nbuf)]
        self.qpin = [torch.empty((chunk,) + tuple(shape)).pin_memory() for _ in range(nbuf)] if with_mask else None
        self.stream = torch.cuda.Stream(device=dev)
        # the device buffers may have been handed out while kernels already queued on the current stream (the previous run's
        # noise copies / step graph) still read them: the upload stream must not start writing before the current stream has
        # reached this point
        self.stream.wait_stream(torch.cuda.current_stream())
        self.noise.record_stream(self.stream)
        if self.qnoise is not None:
            self.qnoise.record_stream(self.stream)
        self.events = {}
        self.produced = 0  # chunks drawn so far
        self.dev_index = torch.cuda.current_device()   # the drawer thread must issue its uploads on THIS device
        self.error = None
        self.cv = threading.Condition()
        self.threaded = (os.environ.get("ALDM_NOISE_THREAD", "1") != "0") if threaded is None else threaded
        self.thread = None
        if self.threaded:
            self.thread = threading.Thread(target=self._run, name="aldm-noise-drawer", daemon=True)
            self.thread.start()

    def _draw_into(self, dst):
        """One reference-ordered draw into a (pinned) staging row."""
        d = self.draw
        if getattr(d, "into", None) is not None:
            d.into(dst)
        else:
            dst.numpy()[...] = d().numpy()   # plain memcpy, no thread pool

    def _produce(self, c):
        lo, hi = self.bounds[c], self.bounds[c + 1]
        slot = c % len(self.pin)
        prev = self.events.get(c - len(self.pin))
        if prev is not None:
            prev.synchronize()  # the upload that last used this pinned slot is done
        # Host side of the RNG contract.  The draws go STRAIGHT into the pinned staging rows (`torch.randn(out=...)`: same
        # generator stream, no intermediate tensor): a 1 MB `Tensor.copy_` through torch's intra-op thread pool costs
        # ~20 ms on a many-core host (measured: 19 ms with 8 threads on 8 busy vCPUs vs 0.02 ms with 4).
        for s in range(lo, hi):  # reference order per step
            if self.with_mask and self.mask_first:
                self._draw_into(self.qpin[slot][s - lo])
            self._draw_into(self.pin[slot][s - lo])
            if self.temperature != 1.0:
                self.pin[slot][s - lo].mul_(self.temperature)
            if self.with_mask and not self.mask_first:
                self._draw_into(self.qpin[slot][s - lo])
        with torch.cuda.stream(self.stream):
            self.noise[lo:hi].copy_(self.pin[slot][:hi - lo], non_blocking=True)
            if self.with_mask:
                self.qnoise[lo:hi].copy_(self.qpin[slot][:hi - lo], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return ev

    def _run(self):   # drawer thread
        try:
            torch.cuda.set_device(self.dev_index)
            for c in range(len(self.bounds) - 1):
                ev = self._produce(c)
                with self.cv:
                    self.events[c] = ev
                    self.produced = c + 1
                    self.cv.notify_all()
        except BaseException as e:  # surfaced by the launching thread's next wait()
            with self.cv:
                self.error = e
                self.cv.notify_all()

    def produce_next(self):
        """Unthreaded mode (ALDM_NOISE_THREAD=0 / tests): draw + upload the next chunk on the calling thread."""
        if self.threaded:
            return
        c = self.produced
        if c + 1 >= len(self.bounds):
            return
        self.events[c] = self._produce(c)
        self.produced = c + 1

    def wait(self, i):
        """Make the current stream wait for step i's noise; returns True when i opens a chunk."""
        c = 0 if i == 0 else 1 + (i - 1) // self.chunk
        if self.threaded:
            with self.cv:
                while self.produced <= c and self.error is None:
                    self.cv.wait(timeout=60.0)
                if self.error is not None:
                    raise RuntimeError(f"noise drawer thread failed: {self.error!r}")
        else:
            while self.produced <= c:
                self.produce_next()
        first = i == self.bounds[c]
        if first:
            torch.cuda.current_stream().wait_event(self.events[c])
        return first

    def close(self):
        """Join the drawer: every draw of the run has been consumed from the generator (callers draw again afterwards)."""
        if self.thread is not None:
            self.thread.join()
            self.thread = None
            if self.error is not None:
                raise RuntimeError(f"noise drawer thread failed: {self.error!r}")


def host_drawer(shape, noise_shard=None):
    """draw() -> one `torch.randn(shape)` from the host default generator, in the reference's order; draw.into(dst) writes
    it into `dst`.  noise_shard = (global_batch, row_offset): a prompt-sharded run draws the GLOBAL batch like the
    single-process reference and keeps rows [offset, offset + shape[0]) (dist.py); with several candidates per prompt
    the second element is the index tensor of the rank's rows (dist.candidate_rows) instead of an offset."""
    shape = tuple(shape)
    if noise_shard is None:
        def draw():
            return torch.randn(shape)

        def into(dst):
            torch.randn(shape, out=dst)
    else:
        gB, off = noise_shard
        gshape = (gB,) + shape[1:]
        if torch.is_tensor(off):
            assert off.numel() == shape[0]
            pick = lambda t: t.index_select(0, off)
        else:
            pick = lambda t: t[off:off + shape[0]]

        def draw():
            return pick(torch.randn(gshape)).contiguous()

        def into(dst):
            dst.numpy()[...] = pick(torch.randn(gshape)).numpy()
    draw.into = into
    return draw


def check_guidance_rescale(phi) -> float:
    """The `guidance_rescale` argument of the samplers and the pipeline as a float: phi of Lin et al. 2023 (section 3.4), in [0, 1];
    0 is off."""
    try:
        phi = float(phi)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_rescale must be a number in [0, 1], got {phi!r}")
    if not (np.isfinite(phi) and 0.0 <= phi <= 1.0):
        raise ValueError(f"guidance_rescale must be finite and in [0, 1], got {phi!r}")
    return phi


def guidance_table(rows, scale, use_cfg, phi=0.0):
    """Pure host function: a sampler's [S, 8] fp32 coefficient table from its [S, 5] rows.  Column 5 = the guidance scale; column
    6 = 1 when the step kernel combines eps[2, n] itself; column 7 = phi.  With guidance rescale on (guidance and phi > 0) the
    combine moves into ops.cfg_rescale_indexed, which reads columns 5 and 7, and the step kernel gets a combined eps[n]: column 6 = 0."""
    rescale = bool(use_cfg) and phi > 0.0
    coef = torch.zeros(rows.shape[0], 8)
    coef[:, :5] = rows
    coef[:, 5] = float(scale)
    coef[:, 6] = 1.0 if use_cfg and not rescale else 0.0
    coef[:, 7] = float(phi) if rescale else 0.0
    return coef


def check_t_start(t_start, timesteps, schedule_len):
    """The `t_start=` keyword of the three samplers (the name of `DDIMSampler.decode`'s parameter): None, or the number k of
    schedule entries to run — indices k-1 ... 0 — from x_T, 1 <= k <= the schedule's length; not together with `timesteps`, whose
    count goes through the reference's float arithmetic."""
    if t_start is None:
        return None
    if timesteps is not None:
        raise ValueError(f"t_start={t_start!r} and timesteps={timesteps!r} both name where to start: pass one")
    if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 1 <= t_start <= schedule_len:
        raise ValueError(f"t_start must be an integer in [1, {schedule_len}] (the schedule's length), got {t_start!r}")
    return int(t_start)


def _integer(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _resample_pair(n, jump):
    """What can be refused of RePaint's (n, jump) before the run's step count is known."""
    if not _integer(n) or not _integer(jump):
        raise ValueError(f"resample=(n, jump) must be a pair of integers, got ({n!r}, {jump!r})")
    if n < 1:
        raise ValueError(f"resample: n (how often each stretch is sampled) must be >= 1, got {n}")
    if jump < 1:
        raise ValueError(f"resample: jump must lie in [1, steps - 1], got {jump}")


def resample_visits(S, n, jump):
    """Pure host function: the visit schedule of resampled inpainting (RePaint, Lugmayr et al. 2022, section 4.2) over
    a run of S sampler steps.  n is RePaint's jump_n_sample — how often every stretch is sampled, 1: off — and jump its jump_length,
    in sampler steps.  Position k in [0, S] counts the net steps completed; loop step i takes the latent from position i to i + 1
    with schedule index S - 1 - i.  A jump point is a position k with (S - k) % jump == 0 and k > jump (the published schedule's
    points: 0, jump, 2*jump, ... steps remaining, strictly below S - jump).  When loop step k - 1 ends on a jump point used fewer
    than n - 1 times, the latent is diffused forward again to position k - jump and the run goes on from loop step k - jump: jump
    points do not nest, and each is used exactly n - 1 times.
    -> a tuple of visits, each ("step", i) or ("renoise", k, k - jump).  ValueError: n or jump no integer (a bool is none), n < 1,
    jump outside [1, S - 1] — with jump >= S there is no jump point and the keyword would be silently ignored."""
    if not _integer(S) or S < 1:
        raise ValueError(f"resample: the run must have a positive integer number of steps, got {S!r}")
    _resample_pair(n, jump)
    if jump > S - 1:
        raise ValueError(f"resample: jump must lie in [1, {S - 1}] for a run of {S} steps, got {jump}: with jump >= the number of "
                         "steps there is no jump point and the keyword would be ignored")
    S, n, jump = int(S), int(n), int(jump)
    used, visits, i = {}, [], 0
    while i < S:
        visits.append(("step", i))
        k = i + 1
        if (S - k) % jump == 0 and k > jump and used.get(k, 0) < n - 1:
            used[k] = used.get(k, 0) + 1
            visits.append(("renoise", k, k - jump))
            k -= jump
        i = k
    return tuple(visits)


def renoise_coef(ddim_alphas, ddim_alphas_prev, S, k, k_to):
    """Pure host function: (c0, c1) of the forward jump from position k down to k_to < k of a run of S steps (resample_visits),
    x <- c0*x + c1*eps: q(x_k_to | x_k) of the DDPM forward process over the whole jump.  The noise level at position p is
    abar(p) = ddim_alphas[S - 1 - p] for p < S — what loop step p takes its input to be at — and abar(S) = ddim_alphas_prev[0], the
    level the last step leaves; rho = abar(k_to) / abar(k) < 1, c0 = sqrt(rho), c1 = sqrt(1 - rho).  Evaluated in fp64 from the
    schedule as given and returned as Python floats (the caller rounds them to fp32 once)."""
    if not 0 <= k_to < k <= S:
        raise ValueError(f"renoise_coef: positions must satisfy 0 <= k_to < k <= S, got k={k!r}, k_to={k_to!r}, S={S!r}")
    a = np.asarray(ddim_alphas.detach().cpu().numpy() if torch.is_tensor(ddim_alphas) else ddim_alphas, dtype=np.float64)
    ap = np.asarray(ddim_alphas_prev.detach().cpu().numpy() if torch.is_tensor(ddim_alphas_prev) else ddim_alphas_prev,
                    dtype=np.float64)

    def abar(p):
        return float(a[S - 1 - p]) if p < S else float(ap[0])
    rho = abar(k_to) / abar(k)
    if not 0.0 < rho < 1.0:
        raise ValueError(f"renoise_coef: abar({k_to}) / abar({k}) = {rho!r} is not in (0, 1): the schedule does not descend")
    return float(np.sqrt(rho)), float(np.sqrt(1.0 - rho))


def check_resample(resample, S=None):
    """The `resample=` keyword of DDIMSampler.sample / ddim_sampling and the pipeline's source-keeping jobs: None, or RePaint's pair
    (n, jump) — see resample_visits, which refuses the values once the run's step count S is known.  -> None, or (n, jump)."""
    if resample is None:
        return None
    if isinstance(resample, (str, bytes)) or not hasattr(resample, "__len__") or len(resample) != 2:
        raise ValueError(f"resample must be None or a pair (n, jump) of integers, got {resample!r}")
    n, jump = resample
    if S is None:
        _resample_pair(n, jump)
    else:
        resample_visits(S, n, jump)
    return int(n), int(jump)


def keep_thresholds(S, visits=None):
    """Pure host function: the threshold table of graded keep levels (differential diffusion, Levin & Fried 2023)
    over a run of S sampler steps -> fp32 [S], entry i = float32(i / S), the quotient taken in fp64.  At loop step i a frame of
    level m is held on q_sample(source, t_i) when float32(m) > entry i, and is free otherwise: level 1 is held at every step, level
    0 at none.  `visits` (resample_visits): one row per visit instead — a step visit takes its loop position's entry, a renoise
    visit the next step visit's, which is not read (plan_run fills blend_coef the same way)."""
    if not _integer(S) or S < 1:
        raise ValueError(f"keep_thresholds: the run must have a positive integer number of steps, got {S!r}")
    pos = np.arange(int(S)) if visits is None else np.asarray([v[1] if v[0] == "step" else v[2] for v in visits])
    return torch.from_numpy((pos.astype(np.float64) / float(int(S))).astype(np.float32))


def hold_steps(level, S):
    """Pure host function: what a keep level MEANS in a run of S steps — the number of loop steps i < S at which a frame of that
    level is held on the noised source, float32(level) > keep_thresholds(S)[i], compared in fp32 (equality releases the frame).
    The thresholds ascend, so these are the run's FIRST hold_steps steps; the frame is free for its last S - hold_steps.  S is
    the number of steps the run really makes (after a t_start / timesteps cut)."""
    return int((np.float32(level) > keep_thresholds(S).numpy()).sum())


def check_levels(mask, x0, who="graded=True"):
    """graded=True declares a sampler's mask a map of keep levels: it needs a mask and a source, and every level finite and in [0, 1].
    ValueError otherwise; host only for a host mask."""
    if mask is None or x0 is None:
        raise ValueError(f"{who} needs a mask of keep levels and a source x0 (or both on the window plan, windows.with_source)")
    if not torch.is_tensor(mask):
        raise ValueError(f"{who}: the levels must be a tensor, got {type(mask).__name__}")
    m = mask.detach().float()
    if m.numel() == 0 or not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
        raise ValueError(f"{who}: keep levels must be finite and lie in [0, 1]")


MAX_COMPOSE = ops.MAX_COMPOSE   # prompts per composed job (ALDM_MAX_COMPOSE)


def check_compose_weights(weights, K, who="Composed"):
    """The weights of a composed job as an fp64 array: [K], or [S, K] — one row per sampler step in loop order, row 0
    the noisiest.  ValueError: a shape that is neither, S == 0, a weight that is no finite number, a row whose weights are all 0
    (the step would run K prompts to read none)."""
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the weights must be numbers, [K] or [steps, K], got {weights!r}")
    if w.ndim not in (1, 2) or w.shape[-1] != K or w.shape[0] == 0:
        raise ValueError(f"{who}: {K} conditionings need weights of shape [{K}] or [steps, {K}], got {tuple(w.shape)}")
    if not np.isfinite(w).all():
        raise ValueError(f"{who}: every weight must be finite")
    if (w.reshape(-1, K) == 0.0).all(axis=1).any():
        raise ValueError(f"{who}: every weight is 0 at some step: the step would read no prompt")
    return w


class Composed:
    """K conditionings under one set of frames with weights w_k (composable-diffusion guidance, Liu et al. 2022): the
    `cond` of a sampler run whose model output is e_u + g * sum_k w_k (e_k - e_u).  A marker class like windows.PerPrompt.  `weights`:
    [K], or [total_steps, K] in loop order (row 0 the noisiest step; a table over the whole schedule is cut with it: a run of its
    last n steps reads the last n rows).  A negative weight steers away from its prompt.  The run needs an unconditional conditioning.
    plan_run binds the run's tiled conditionings, the device table `tab` and — the sampler — the device counter `step_idx` on a copy."""

    def __init__(self, conds, weights):
        conds = list(conds)
        if not 1 <= len(conds) <= MAX_COMPOSE:
            raise ValueError(f"Composed: between 1 and {MAX_COMPOSE} conditionings, got {len(conds)}")
        self.conds = conds
        self.weights = check_compose_weights(weights, len(conds))
        self.tab, self.step_idx = None, None

    def __len__(self):
        return len(self.conds)

    def bound(self, conds, tab):
        """A copy for one run: these (tiled) conditionings and this device table."""
        c = Composed(conds, self.weights)
        c.tab = tab
        return c


def compose_table(weights, total_steps=None, visits=None, schedule_len=None):
    """Pure host function: the [V, K+1] fp32 coefficient table of ops.cfg_compose_indexed from a composed job's weights
    (check_compose_weights' result).  Column 0 = 1 - sum_k w_k, formed in fp64 and rounded to fp32 once; columns 1..K = w_k.
    Weights [K]: one row, whatever the run (the kernel clamps the counter into the table).  Weights [S, K]: S must be the run's
    `total_steps` — or `schedule_len`, the uncut schedule's length, of which the run reads the LAST total_steps rows — and the table has
    one row per step, or with `visits` (resample_visits) one per visit: a step visit at loop position i takes row i, a renoise visit
    — not read — the next step visit's, blend_coef's rule.  ValueError for any other S."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 2:
        if total_steps is None:
            raise ValueError("compose_table: a weight schedule needs the run's step count")
        if w.shape[0] != total_steps:
            if schedule_len is None or w.shape[0] != schedule_len or total_steps > schedule_len:
                raise ValueError(f"Composed: the weight schedule has {w.shape[0]} rows, the run {total_steps} steps"
                                 + ("" if schedule_len is None else f" (of a schedule of {schedule_len})"))
            w = w[schedule_len - total_steps:]
        if visits is not None:
            w = w[np.asarray([v[1] if v[0] == "step" else v[2] for v in visits])]
    else:
        w = w[None]
    tab = np.concatenate([1.0 - w.sum(axis=1, keepdims=True), w], axis=1)
    return torch.from_numpy(np.ascontiguousarray(tab.astype(np.float32)))


def ddim_step_rows(sigmas, alphas, alphas_prev, sqrt_one_minus_alphas):
    """Pure host function: the [S, 5] fp32 rows {sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev - sigma_t^2), sqrt(a_prev), sigma_t} of
    DDIM's update (the row layout of ops.ddim_step), one per schedule index, with the reference's roundings (ddim.py:330-353,
    plms.py:319-338): a_t, a_prev, sigma_t and sqrt(1 - a_t) become fp32 via torch.full; the other square roots are fp32 tensor ops."""
    rows = []
    for i in range(len(alphas)):
        a_t = torch.full((1,), float(alphas[i]))
        ap = torch.full((1,), float(alphas_prev[i]))
        sg = torch.full((1,), float(sigmas[i]))
        som = torch.full((1,), float(sqrt_one_minus_alphas[i]))
        rows.append(torch.cat([som, a_t.sqrt(), (1.0 - ap - sg ** 2).sqrt(), ap.sqrt(), sg]))
    return torch.stack(rows)


def log_step(i, total_steps, log_every_t, x_cur, pred_x0, intermediates, callback=None, img_callback=None):
    """The tail of step i of a sampling loop (ddim.py:244-260): the two callbacks, then the step's state into `intermediates`
    every `log_every_t` schedule indices and at the run's first step."""
    if callback:
        callback(i)
    if img_callback:
        img_callback(pred_x0, i)
    index = total_steps - i - 1
    if index % log_every_t == 0 or index == total_steps - 1:
        intermediates["x_inter"].append(x_cur.clone())
        intermediates["pred_x0"].append(pred_x0.clone())


class SamplerBase(object):
    """Constructor, schedule, run plan and UNet pass of the three samplers.  A subclass adds its coefficient rows in
    `make_schedule`, its `sample` and its loop."""

    # why `ddim_use_original_steps=True` is refused (the tail of _refuse's message)
    ORIGINAL_STEPS = "is not supported"

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = os.environ.get("ALDM_NO_GRAPH", "0") != "1"
        # (global_batch, row_offset) when this process samples one shard of a larger batch (dist.py)
        self.noise_shard = getattr(model, "noise_shard", None)

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """ddim.py:33-91 / plms.py:27-89 (host side, float tables only): the timestep grid, the abar tables, DDIM's sigma and abar
        per grid entry."""
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps, verbose)
        alphas_cumprod = self.model.alphas_cumprod.detach().float().cpu()
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        self.register_buffer("alphas_cumprod", alphas_cumprod)
        self.register_buffer("sqrt_alphas_cumprod", torch.sqrt(alphas_cumprod))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - alphas_cumprod))
        sig, a, a_prev = make_ddim_sampling_parameters(alphas_cumprod, self.ddim_timesteps, ddim_eta, verbose)
        self.register_buffer("ddim_sigmas", sig)
        self.register_buffer("ddim_alphas", a)
        self.register_buffer("ddim_alphas_prev", a_prev)

    def _refuse(self, ddim_use_original_steps, quantize_denoised, score_corrector, noise_dropout):
        name = type(self).__name__
        if ddim_use_original_steps:
            raise NotImplementedError(f"{name}(HIP): ddim_use_original_steps=True {self.ORIGINAL_STEPS}")
        if quantize_denoised or score_corrector is not None or noise_dropout != 0.0:
            raise NotImplementedError(f"{name}(HIP): option not used by the AudioLDM2 pipeline")

    def model_output(self, x, t_row, b, cond, uncond, use_cfg, prepared, win=None, static=True, first_pass=True):
        """The UNet pass of one step: eps [2, b, ...] = [uncond ; cond] under guidance (combined inside the step kernel, or by
        ops.cfg_rescale_indexed), else eps [b, ...].  t_row: the step's timestep as floats, one entry per UNet row.  Guidance is ONE
        pass over 2b samples when the model has `apply_model_cfg` — asked at every call: it may be set on an instance — where the
        reference runs two (ddim.py:293-296).

        `win` (plan_run's `p.win`, a windowed run): x is the long latent; its windows are gathered (ops.window_gather), the pass
        above runs on the W*b window rows — cond, uncond, prepared and t_row are the W-fold tiled ones — and the window outputs
        are merged back to the long shape (ops.window_merge): two launches around an unchanged pass.  `static`: gather and merge
        into win's buffers (a step graph's static tensors); False: into fresh ones (eager calls whose results must coexist).

        A plan with a source (`win.blend`, windows.with_source): at a step's first UNet pass (`first_pass`) the fused
        ops.window_blend_gather takes the gather's place — it blends q_sample(x0, t) into x IN PLACE where the mask is 1, with the
        q-noise row and the coefficient row the device-side `win.step_idx` selects from `win.qnoise` and `win.blend_coef`, and
        writes the windows of the blended latent.  Any further pass of the same step (PLMS's second one in its eager step 0, on the
        provisional x_prev) gathers plainly.  The sampler sets win.qnoise and win.step_idx before its first step.

        A row plan (windows.row_plan, a prompt timeline): the same three launches in their `_rows` forms over
        win.n = plan.R rows — one per (window, prompt) pair, cond holding every row's own prompt (windows.rows_cond), uncond tiled
        R times — and the merge reads the per-row, per-frame weights from win.wr, a static [R, Tw] device buffer (eager passes into
        fresh tensors, `static=False`, read the same buffer).  plan_run is where a row plan and a PerPrompt are matched; here `cond` is
        normally its per-row result.  A PerPrompt that reaches this function is expanded with windows.rows_cond when win.plan has rows
        and refused (ValueError) when it has none or the prompt counts differ; a row plan without win.wr / win.n == R is refused too.

        A phased ring plan (windows.with_phase, moving window phases): the same three launches in their `_ring_phased`
        forms.  All of a pass's launches read the phase of the visit from win.phase — a static int32 device table, one row per visit
        — with the device-side counter win.step_idx, so gather and merge of one pass agree and a replayed step graph moves its
        windows without the host.  The sampler sets win.step_idx before its first step; None reads row 0.

        A Composed conditioning (composable guidance): one pass over the K+1 groups [uncond ; prompt 1 ; ... ; prompt K]
        — the model's apply_model_groups on `prepared` = prepare_groups(...), or K+1 sequential apply_model calls, stacked — and
        ops.cfg_compose_indexed in place behind it, with the row of cond.tab that the device-side counter cond.step_idx selects (None:
        row 0): the result is the first 2n floats of the pass's output, [uncond ; composed cond] — or with use_cfg False the first
        n, the composed prediction.  On a window plan this happens on the window rows, in front of the merge."""
        from .windows import PerPrompt, has_rows, rows_cond
        rows = win is not None and has_rows(win.plan)
        if isinstance(cond, PerPrompt):
            # plan_run hands the per-row conditioning on; a caller with a hand-made `win` may pass the PerPrompt itself
            if not rows:
                raise ValueError("model_output: a PerPrompt conditioning needs a row plan (windows.row_plan) on `win`")
            cond = rows_cond(cond, win.plan)   # refuses a wrong number of prompts
        if rows and (getattr(win, "wr", None) is None or getattr(win, "n", None) != win.plan.R):
            raise ValueError("model_output: a row plan needs win.n == plan.R and win.wr, the [R, Tw] merge weights on the device "
                             "(plan_run builds both)")
        if win is not None:
            phase = getattr(win, "phase", None)
            # moving window phases: gather and merge read the same row of the same table with the same counter
            phased = {} if phase is None else {"phase": phase, "step_idx": win.step_idx}
            if win.blend and first_pass:
                # a plan with a source: the blend of the known region on the long latent, in place, and the gather are one launch
                if getattr(win, "level", None) is not None:
                    # graded keep levels: this step's binary mask from the level map, one launch in front of the
                    # blend, reading the same counter — a node of the captured step like the blend itself
                    ops.keep_threshold_indexed(win.level, win.keep_thr, win.mask, win.step_idx)
                xw = ops.window_blend_gather(x, win.x0, win.qnoise, win.mask, win.blend_coef, win.plan, step_idx=win.step_idx,
                                             out=win.xw if static else None, phase=phase)
            else:
                xw = ops.window_gather(x, win.plan, out=win.xw if static else None, **phased)
            eps_w = self.model_output(xw, t_row, win.n * b, cond, uncond, use_cfg, prepared)
            return ops.window_merge(eps_w.contiguous(), win.plan, out=win.merged if static else None, weights=win.wr, **phased)
        if isinstance(cond, Composed):
            # composable guidance: one pass over the K+1 groups [uncond ; prompt 1 ; ... ; prompt K], then ONE launch
            # that reduces them to the standard pair in place — on a window plan this is the pass on the window rows, in front of
            # the merge.  The row of the weight table is the counter's (None: row 0); the counter is read, never moved
            if uncond is None:
                raise ValueError("model_output: a Composed conditioning needs an unconditional conditioning (its coefficient "
                                 "1 - sum(weights) reads it)")
            if cond.tab is None:
                cond.tab = compose_table(cond.weights).to(x.device)   # a direct caller: constant weights only
            if hasattr(self.model, "apply_model_groups"):
                if prepared is None:
                    prepared = self.model.prepare_groups(cond.conds, uncond)
                eps = self.model.apply_model_groups(x, t_row, prepared)
            else:
                tl = t_row[:b].long()
                eps = torch.stack([self.model.apply_model(x, tl, c) for c in [uncond] + cond.conds]).contiguous()
            return ops.cfg_compose_indexed(eps, cond.tab, cond.step_idx, pair=use_cfg)
        if not use_cfg:
            return self.model.apply_model(x, t_row[:b].long(), cond).contiguous()
        if hasattr(self.model, "apply_model_cfg"):
            return self.model.apply_model_cfg(x, t_row, cond, uncond, prepared=prepared)
        tl = t_row[:b].long()
        return torch.stack([self.model.apply_model(x, tl, uncond), self.model.apply_model(x, tl, cond)]).contiguous()

    def plan_run(self, cond, shape, x_T, t_start, timesteps, table, unconditional_guidance_scale, unconditional_conditioning,
                 guidance_rescale, mask, x0, windows=None, resample=None, graded=False):
        """Everything a sampling loop needs before its first step, as one object.  `table(total_steps, use_cfg)` is the sampler's
        own [total_steps, 8] host coefficient table in loop order (i = 0 is the noisiest step, index = total_steps - 1).

        `windows` (a latent-domain windows.window_plan, or None): a windowed run over the long `shape` [b, C, plan.T, F].  x_T and
        the per-step noise keep the long shape; `p.cond` / `p.uncond` are the conditionings tiled W times (window-major), t_tab
        has W times the columns, prepare_cfg sees the tiled pair, and `p.win` holds the plan and the two static window buffers
        of model_output (xw [W*b, C, Tw, F], merged [2, b, ...] or [b, ...]).  Without a plan p.cond / p.uncond are the arguments
        and p.win is None.  A row plan (windows.row_plan): `cond` must be a windows.PerPrompt of its K conditionings (and a
        PerPrompt needs a row plan; ValueError otherwise); R = plan.R takes W's place for t_tab, xw and the tiled uncond, p.cond is
        windows.rows_cond (row r under its own prompt), and p.win.wr holds the merge weights on the device.
        Not together with mask / x0: a source to keep rides on the plan (windows.with_source) and fills
        p.mask_d / p.x0_d / p.blend_coef as a mask does, with p.win.blend set — the blend then runs inside the step, fused with
        the gather (model_output), not between the steps.

        The cut of the schedule: `t_start=k` keeps exactly its first k entries, as `decode` cuts it (ddim.py:466-467; see
        check_t_start); `timesteps` keeps its first int(min(timesteps / S, 1) * S) - 1 entries (ddim.py:198-206).  `total_steps`
        may be 0 (`timesteps` <= one interval): the reference's loop then runs zero iterations and returns x_T, and nothing past
        `img` is built.

        `resample` (None, or RePaint's pair (n, jump)): resampled inpainting.  The run becomes a sequence of V
        visits (resample_visits over the cut schedule's `total_steps`), `p.visits`, and EVERY table gets V rows in visit order —
        coef, t_tab, blend_coef, and (the sampler's) noise and q-noise tables — so the device-side counter that selects a step's
        rows counts visits.  A step visit at loop position i has the rows position i has without the keyword; a renoise visit's
        coefficient row is (c0, c1, 0, ...) of renoise_coef, its t_tab and blend_coef rows — not read — are the next step visit's.
        Refused (ValueError) before the first draw: a malformed pair or values resample_visits refuses, and a run with nothing to
        harmonise with (no mask / x0 and no source on the plan).  n == 1 is the plain run: p.visits is None, as without the keyword.

        `graded` (or a plan whose source was declared graded, windows.with_source): the mask is a map of keep LEVELS
        in [0, 1].  p.level_d holds the expanded map, p.mask_d becomes a scratch buffer of the same shape — what the blend reads,
        as always — and p.keep_thr the run's threshold rows on the device (keep_thresholds over the cut schedule, one per visit);
        p.win carries `level` and `keep_thr` too.  The sampler issues ops.keep_threshold_indexed directly in front of every blend.
        Refused (ValueError) before the first draw: no mask or source, levels that are not finite or leave [0, 1].  Without it
        p.level_d and p.keep_thr are None and nothing changes.

        A phased ring plan (windows.with_phase): its table must have one entry per step of the cut schedule —
        `total_steps`; ValueError before the first draw otherwise — and p.win.phase holds it on the device as int32 with one row per
        VISIT: a step visit at loop position i has entry i, a renoise visit (not read) the next step visit's, blend_coef's rule.
        The samplers point p.win.step_idx at their step counter.  No draw is added; without a phase p.win.phase is None.

        RNG contract R: x_T is the host generator's first draw of the run, made only when x_T is not given; `draw` makes the
        loop's later ones.  A start latent that already lives on the device (audio-to-audio) stays there.  Host -> device copies,
        in this order: img, coef, t_tab, mask_d, x0_d, blend_coef, keep_thr, (a row plan's wr, a phased plan's phase, a Composed's
        table,) then the model's prepare_cfg / prepare_groups.

        A Composed conditioning (composable guidance): K prompts on the same frames.  It needs an unconditional
        conditioning (ValueError otherwise, and for a weight schedule whose length is neither the run's nor the whole schedule's —
        both before the first draw).  p.compose holds compose_table on the device — one row, or one per visit — t_tab has
        (K+1)*W*b columns, p.cond is a bound copy with every group's conditioning tiled per window, and the model's prepare_groups
        takes prepare_cfg's place.  The samplers point p.cond.step_idx at their step counter.  No draw is added."""
        dev = torch.device("cuda")
        shape = tuple(shape)
        from .windows import check_per_prompt, has_phase, has_rows
        check_per_prompt(cond, windows)   # a row plan and a PerPrompt conditioning go together, or neither
        comp = isinstance(cond, Composed)   # composable guidance: K+1 UNet row groups, reduced to the pair behind the pass
        if comp and unconditional_conditioning is None:
            raise ValueError("a Composed conditioning needs an unconditional conditioning: its coefficient 1 - sum(weights) reads it")
        W, source = 1, None
        if windows is not None:
            if mask is not None or x0 is not None:
                raise ValueError("windows= together with mask / x0: inpainting over windows is not supported")
            if len(shape) != 4 or shape[2] != windows.T:
                raise ValueError(f"windows= is a plan over T={windows.T} frames, the latent shape is {shape}")
            W = windows.R if has_rows(windows) else windows.W   # the UNet's row groups: rows of a timeline, else windows
            if getattr(windows, "x0", None) is not None:
                # a source rides on the plan (windows.with_source): inpainting / continuation over windows
                if tuple(windows.x0.shape) != shape:
                    raise ValueError(f"windows=: the plan's source x0 is {tuple(windows.x0.shape)}, the latent shape is {shape}")
                source = (windows.mask, windows.x0)
                graded = bool(graded) or bool(getattr(windows, "graded", False))
        if graded:
            check_levels(*(source if source is not None else (mask, x0)))
        ts = self.ddim_timesteps
        t_start = check_t_start(t_start, timesteps, ts.shape[0])
        if t_start is not None:
            ts = ts[:t_start]
        if timesteps is not None:
            subset_end = int(min(timesteps / ts.shape[0], 1) * ts.shape[0]) - 1
            ts = ts[:subset_end]
        total_steps = ts.shape[0]
        use_cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
        p = SimpleNamespace(total_steps=total_steps, use_cfg=use_cfg, mask_d=None, x0_d=None, blend_coef=None, prepared=None,
                            cond=cond, uncond=unconditional_conditioning, win=None, visits=None, level_d=None, keep_thr=None,
                            compose=None)
        if resample is not None:
            if mask is None and x0 is None and source is None:
                raise ValueError("resample= needs something to harmonise with: a mask / x0, or a source on the window plan "
                                 "(windows.with_source)")
            if total_steps == 0:
                raise ValueError("resample=: the cut schedule has no step to run")
            if check_resample(resample, total_steps)[0] > 1:
                p.visits = resample_visits(total_steps, *resample)
        phased = windows is not None and has_phase(windows)
        if phased and int(windows.phase.numel()) != total_steps:
            raise ValueError(f"windows=: the plan's phase table has {int(windows.phase.numel())} entries, the run {total_steps} "
                             "steps: one phase per sampler step (windows.phase_table over the cut schedule)")
        # composable guidance: the [V, K+1] coefficient table, refused here — before the first draw — when a weight schedule does not
        # fit the run
        compose = compose_table(cond.weights, total_steps, p.visits, len(self.ddim_timesteps)) if comp and total_steps else None
        p.time_range = np.flip(ts).copy()   # own storage, positive strides: from_numpy refuses the flipped view, even of one entry
        # guidance rescale: the combine and the per-sample rescale run in a launch of their own in front of the step kernel
        p.rescale = use_cfg and guidance_rescale > 0.0
        p.draw = host_drawer(shape, self.noise_shard)
        p.img = (p.draw().to(dev) if x_T is None else x_T.detach().float().to(dev)).contiguous()
        if total_steps == 0:
            return p
        coef = table(total_steps, use_cfg)
        tr = torch.from_numpy(p.time_range)
        if p.visits is not None:
            # one table row per VISIT: a step visit takes its loop position's row, a renoise visit the next step visit's (it reads
            # neither its timestep nor its blend coefficients) — and its own (c0, c1, 0, ...) as the coefficient row
            rows = torch.tensor([v[1] if v[0] == "step" else v[2] for v in p.visits], dtype=torch.long)
            coef = coef[rows].clone()
            for r, v in enumerate(p.visits):
                if v[0] == "renoise":
                    coef[r] = 0.0
                    coef[r, 0], coef[r, 1] = renoise_coef(self.ddim_alphas, self.ddim_alphas_prev, total_steps, v[1], v[2])
            tr = tr[rows]
        p.coef = coef.to(dev)
        groups = len(cond) + 1 if comp else (2 if use_cfg else 1)   # the UNet's conditioning groups
        p.t_tab = tr.float()[:, None].repeat(1, groups * W * shape[0]).to(dev).contiguous()
        if source is not None:
            mask, x0 = source
        if mask is not None:
            assert x0 is not None
            p.mask_d = mask.float().to(dev).expand(shape).contiguous()
            p.x0_d = x0.float().to(dev).contiguous()
            p.blend_coef = torch.stack([self.sqrt_alphas_cumprod[tr], self.sqrt_one_minus_alphas_cumprod[tr]],
                                       1).contiguous().to(dev)  # [S, 2] = {sqrt(abar_t), sqrt(1 - abar_t)}
            if graded:
                # the map of levels stays; the blend's mask is rewritten from it in front of every blend (keep_threshold_indexed)
                p.level_d, p.mask_d = p.mask_d, torch.zeros_like(p.mask_d)
                p.keep_thr = keep_thresholds(total_steps, p.visits).to(dev)
        if windows is not None:
            from .windows import rows_cond, tile_cond
            p.cond = rows_cond(cond, windows) if has_rows(windows) else (cond if comp else tile_cond(cond, W))
            p.uncond = tile_cond(unconditional_conditioning, W)
            b, C, _, F = shape
            # blend: the plan carries a source; the fused blend-and-gather node reads x0 / mask / blend_coef from here and the
            # q-noise table and the step counter the sampler puts next to them (model_output)
            p.win = SimpleNamespace(plan=windows, xw=torch.empty((W * b, C, windows.Tw, F), device=dev, dtype=torch.float32),
                                    merged=torch.empty(((2,) if use_cfg else ()) + shape, device=dev, dtype=torch.float32),
                                    blend=source is not None, x0=p.x0_d, mask=p.mask_d, blend_coef=p.blend_coef, qnoise=None,
                                    step_idx=None, n=W, level=p.level_d, keep_thr=p.keep_thr,
                                    # a row plan: the merge's [R, Tw] weights, a static buffer of the run (of the step graph's
                                    # cache entry, which refills it per job: two timelines of one row geometry share a graph)
                                    wr=windows.wr.to(dev).contiguous() if has_rows(windows) else None, phase=None)
            if phased:
                # moving window phases: one int32 row per visit, selected on the device by the sampler's step counter — a static
                # buffer of the run (of the step graph's cache entry, which refills it per job, as it refills wr)
                pos = torch.arange(total_steps) if p.visits is None else \
                    torch.tensor([v[1] if v[0] == "step" else v[2] for v in p.visits], dtype=torch.long)
                p.win.phase = windows.phase.to(torch.int32)[pos].contiguous().to(dev)
        if comp:
            # the run's own copy: every group's conditioning tiled per window, and the table on the device — a static buffer of the
            # run (of DDIM's step-graph cache entry, which refills it per job, as it refills wr and phase)
            p.compose = compose.to(dev)
            p.cond = cond.bound([tile_cond(c, W) for c in cond.conds] if windows is not None else cond.conds, p.compose)
            if hasattr(self.model, "apply_model_groups") and hasattr(self.model, "prepare_groups"):
                p.prepared = self.model.prepare_groups(p.cond.conds, p.uncond)
        elif use_cfg and hasattr(self.model, "apply_model_cfg") and hasattr(self.model, "prepare_cfg"):
            p.prepared = self.model.prepare_cfg(p.cond, p.uncond)
        return p
