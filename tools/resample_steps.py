"""What resampled inpainting (RePaint's jumps) costs, in one process on cuda:0: audioldm2-full (random-init weights), a
long latent of T = 768 frames (30 s) at batch 1 through windows of the trained 256 frames (--hop 192: four windows) with a source
kept (a random source latent, the first third of the frames), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20),
--jobs jobs per arm, the arms alternating job by job.

 a. the plain source job: the replayed step of generate_batch_long_from_audio — fused blend-and-gather, UNet pass on the window rows,
    merge, DDIM update.  THE YARDSTICK; the spread of its own repeats in this call is reported next to the ratio below.
 b. the same job with resample=(--n, --jump): the same step graph replayed over a longer table of visits.  Its replayed steps are
    timed over the intervals that hold no renoise visit; expect b / a = 1 — read it next to the spread of a's repeats.  Nothing
    is asserted.
 c. a renoise visit alone: ops.renoise_indexed + ops.step_advance, eager and back to back on buffers of the job's shape (GPU time
    per visit from events around --reps visits), and — from the jobs of b — the median interval that holds a renoise visit minus the
    median one that holds none.
 d. the job: the wall time of sample_log (no VAE, no vocoder) of b against V_step / S times that of a.
Per-step GPU time from events recorded by the step callback (step visits only), from the fourth step visit on.  A measurement, not a
bar.  Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--jump", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--hop", type=int, default=192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.sampling import make_ddim_timesteps, resample_visits
    from audioldm2_amd.windows import keep_mask, window_plan, with_source
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    plan = window_plan(args.T, 256, args.hop)
    C, F = ld.channels, ld.latent_f_size
    shape = (1, C, plan.T, F)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    keep = [(0, plan.T // 3)]
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(1))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    S = len(make_ddim_timesteps("uniform", args.steps, ld.num_timesteps, verbose=False))
    visits = resample_visits(S, args.n, args.jump)
    step_visits = [j for j, v in enumerate(visits) if v[0] == "step"]
    # interval k runs from the callback of step visit k to that of step visit k + 1: it holds a renoise visit when the two are not
    # neighbours in the visit list
    jumped = [b - a > 1 for a, b in zip(step_visits, step_visits[1:])]

    def job(resample):
        events = []

        def cb(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
        cb.uses_rng = False   # DDIM keeps its threaded noise feed
        kw = {} if resample is None else {"resample": resample}
        seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.sample_log(cond=cond, batch_size=1, ddim=True, ddim_steps=args.steps, eta=0.0, unconditional_guidance_scale=3.5,
                      unconditional_conditioning=uncond, callback=cb, windows=with_source(plan, x0, keep_mask(plan.T, keep)), **kw)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        gaps = [a.elapsed_time(b) for a, b in zip(events, events[1:])]
        flags = jumped if resample is not None else [False] * len(gaps)
        assert len(flags) == len(gaps)
        per = sorted(g for k, (g, f) in enumerate(zip(gaps, flags)) if k >= 2 and not f)
        out = {"wall_ms": round(wall, 2), "step_ms_median": round(median(per), 4), "step_ms_min": round(per[0], 4),
               "step_visits": len(events)}
        with_jump = sorted(g for g, f in zip(gaps, flags) if f)
        if with_jump:
            out["interval_with_renoise_ms_median"] = round(median(with_jump), 4)
        return out

    def renoise_alone_us():
        V = len(visits)
        x, noise = torch.randn(shape, device="cuda"), torch.randn((V,) + shape, device="cuda")
        coef = torch.zeros(V, 8, device="cuda")
        coef[:, 0], coef[:, 1] = 0.8, 0.6
        t_tab, t_cur = torch.zeros(V, 2 * plan.W, device="cuda"), torch.zeros(2 * plan.W, device="cuda")
        idx = torch.zeros(1, device="cuda", dtype=torch.int32)

        def visit():
            ops.renoise_indexed(x, noise, coef, idx)
            ops.step_advance(idx, t_tab, t_cur)
        for _ in range(10):
            visit()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            visit()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / args.reps, 3)

    v_step = len(step_visits)
    res = {"what": "resampled inpainting (RePaint jumps) on a long-form (windowed) DDIM job at batch 1 with a source kept, next to the "
                   "plain source job of the same call: replayed steps, eta 0; a renoise visit alone; the job's wall time",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "S": S, "resample": [args.n, args.jump], "V": len(visits),
           "V_step": v_step, "V_renoise": len(visits) - v_step, "T": plan.T, "Tw": plan.Tw, "hop": plan.hop, "W": plan.W, "keep": keep,
           "noise_tables_bytes": 2 * len(visits) * 4 * shape[1] * shape[2] * shape[3], "mode": ops.MMA_MODE,
           "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash()}
    plain, resampled = [], []
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
        plain.append(job(None))
        resampled.append(job((args.n, args.jump)))
    a_all = [j["step_ms_median"] for j in plain]
    a, b = median(a_all), median([j["step_ms_median"] for j in resampled])
    wa, wb = median([j["wall_ms"] for j in plain]), median([j["wall_ms"] for j in resampled])
    with_jump = median([j["interval_with_renoise_ms_median"] for j in resampled])
    res.update({"plain_source": plain, "resampled": resampled, "step_ms_plain_source": a, "step_ms_resampled": b,
                "resampled_step_over_plain_step": round(b / a, 4), "plain_repeats_spread": round((max(a_all) - min(a_all)) / a, 4),
                "renoise_visit_alone_us": renoise_alone_us(), "renoise_visit_in_job_us": round((with_jump - b) * 1e3, 1),
                "job_ms_plain_source": wa, "job_ms_resampled": wb, "v_step_over_s": round(v_step / S, 4),
                "job_resampled_over_scaled_plain": round(wb / (wa * v_step / S), 4)})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
