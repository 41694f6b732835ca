"""What graded keep levels (differential diffusion) cost, in one process on cuda:0: audioldm2-full (random-init weights),
a long latent of T = 768 frames (30 s) at batch 1 through windows of the trained 256 frames (--hop 192: four windows) with a source (a
random source latent), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20), --jobs jobs per arm, the arms alternating
job by job.

 a. the plain source job: the replayed step of generate_batch_long_from_audio — fused blend-and-gather, UNet pass on the window rows,
    merge, DDIM update — with the first third of the frames kept.  THE YARDSTICK; the spread of its own repeats in this call is
    reported next to the ratio below.
 b. the graded job: the same frames kept, a half-kept second third and a feather of 26 frames (windows.keep_levels), graded=True on
    the plan: the same step graph with ONE more node, ops.keep_threshold_indexed, in front of the blend.  Expect b / a = 1 + (the
    launch) / (the step) — read it next to the spread of a's repeats.  Nothing is asserted.
 c. the new launch alone: ops.keep_threshold_indexed, eager and back to back on buffers of the job's shape (GPU time per launch from
    events around --reps launches).
Per-step GPU time from events recorded by the step callback, from the fourth step on.  A measurement, not a bar.  Prints one JSON
object; --out also writes it."""
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
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--hop", type=int, default=192)
    ap.add_argument("--feather", type=int, default=26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.sampling import keep_thresholds, make_ddim_timesteps
    from audioldm2_amd.windows import keep_levels, keep_mask, window_plan, with_source
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    plan = window_plan(args.T, 256, args.hop)
    C, F = ld.channels, ld.latent_f_size
    shape = (1, C, plan.T, F)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    third = plan.T // 3
    keep, graded_keep = [(0, third)], [(0, third), (third, 2 * third, 0.5)]
    levels = keep_levels(plan.T, graded_keep, args.feather)
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(1))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}
    S = len(make_ddim_timesteps("uniform", args.steps, ld.num_timesteps, verbose=False))

    def job(graded):
        events = []

        def cb(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
        cb.uses_rng = False   # DDIM keeps its threaded noise feed
        windows = with_source(plan, x0, levels, graded=True) if graded else with_source(plan, x0, keep_mask(plan.T, keep))
        seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.sample_log(cond=cond, batch_size=1, ddim=True, ddim_steps=args.steps, eta=0.0, unconditional_guidance_scale=3.5,
                      unconditional_conditioning=uncond, callback=cb, windows=windows)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = sorted(a.elapsed_time(b) for a, b in list(zip(events, events[1:]))[2:])
        return {"wall_ms": round(wall, 2), "step_ms_median": round(median(per), 4), "step_ms_min": round(per[0], 4), "steps": len(events)}

    def launch_alone_us():
        level, mask = levels.view(1, 1, -1, 1).expand(shape).contiguous().cuda(), torch.empty(shape, device="cuda")
        thr, idx = keep_thresholds(S).cuda(), torch.full((1,), S // 2, device="cuda", dtype=torch.int32)
        for _ in range(10):
            ops.keep_threshold_indexed(level, thr, mask, idx)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            ops.keep_threshold_indexed(level, thr, mask, idx)
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / args.reps, 3)

    res = {"what": "graded keep levels (differential diffusion) on a long-form (windowed) DDIM job at batch 1 with a source, next to the "
                   "plain source job of the same call: replayed steps, eta 0; the threshold launch alone",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "S": S, "T": plan.T, "Tw": plan.Tw, "hop": plan.hop,
           "W": plan.W, "keep": keep, "graded_keep": graded_keep, "feather": args.feather,
           "distinct_levels": len(set(levels.tolist())), "latent_floats": shape[1] * shape[2] * shape[3], "mode": ops.MMA_MODE,
           "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash()}
    plain, graded = [], []
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
        plain.append(job(False))
        graded.append(job(True))
    a_all = [j["step_ms_median"] for j in plain]
    a, b = median(a_all), median([j["step_ms_median"] for j in graded])
    res.update({"plain_source": plain, "graded": graded, "step_ms_plain_source": a, "step_ms_graded": b,
                "graded_step_over_plain_step": round(b / a, 4), "plain_repeats_spread": round((max(a_all) - min(a_all)) / a, 4),
                "threshold_launch_alone_us": launch_alone_us(),
                "job_ms_plain_source": median([j["wall_ms"] for j in plain]), "job_ms_graded": median([j["wall_ms"] for j in graded])})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
