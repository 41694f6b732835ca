"""What keeping a source costs a step of long-form (windowed) generation, in one process on cuda:0: audioldm2-full (random-init
weights), a long latent of T = 768 frames at batch 1 through windows of the trained 256 frames (--hop 256: three windows), DDIM at eta
0, guidance 3.5, --steps schedule steps (default 20), --jobs jobs per arm, the arms alternating job by job.

 a. plain windowed: the replayed step of generate_batch_long — gather, UNet pass on the window rows, merge, DDIM update.  THE
    YARDSTICK; the spread of its own repeats in this call is reported next to the ratio below.
 b. with a source (windows.with_source: a random source latent, the first third of the frames kept): the same step with the fused
    blend-and-gather node (ops.window_blend_gather) in the gather's place, reading the q-noise table with the graph's step counter.
    The figure that matters is b / a of this one call (box-to-box spread is several per cent).
 c. the launches alone, eager and back to back, on the step's buffers (x [1, 8, 768, 16] -> 3 windows, and the default-hop 4-window
    plan): the fused launch against ops.inpaint_blend followed by ops.window_gather — what the fused node replaces if the blend ran
    as a launch of its own.  GPU time per launch from events around --reps launches.
Per-step GPU time from events recorded by the step callback, median over the replayed steps (from the fourth step on) (sample_log
only: no VAE, no vocoder).  A measurement, not a bar.  Prints one JSON object; --out also writes it."""
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
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.windows import keep_mask, window_plan, with_source
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    plan = window_plan(args.T, 256, args.hop)
    C, F = ld.channels, ld.latent_f_size
    x0 = torch.randn(1, C, plan.T, F, generator=torch.Generator().manual_seed(1)).cuda()
    keep = [(0, plan.T // 3)]
    src = with_source(plan, x0, keep_mask(plan.T, keep))
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(1))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(1) for k, m in ld.cond_stage_model_metadata.items()}

    def job(windows):
        events = []

        def cb(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
        cb.uses_rng = False   # DDIM keeps its threaded noise feed
        seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.sample_log(cond=cond, batch_size=1, ddim=True, ddim_steps=args.steps, eta=0.0, unconditional_guidance_scale=3.5,
                      unconditional_conditioning=uncond, callback=cb, windows=windows)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
        return {"wall_ms": round(wall, 2), "step_ms_median": round(median(per), 4), "step_ms_min": round(per[0], 4),
                "steps": len(events)}

    def launch_us(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / args.reps, 3)

    def launches(p):
        shape = (1, C, p.T, F)
        x, z, qn = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda"), torch.randn((4,) + shape, device="cuda")
        m = keep_mask(p.T, [(0, p.T // 3)]).view(1, 1, -1, 1).expand(shape).contiguous().cuda()
        coef = torch.tensor([[0.6, 0.8]] * 4, device="cuda")
        idx = torch.full((1,), 2, device="cuda", dtype=torch.int32)
        xw = torch.empty(p.W, C, p.Tw, F, device="cuda")

        def two():
            ops.inpaint_blend(x, z, qn[2], m, coef[2])
            ops.window_gather(x, p, out=xw)
        fused = launch_us(lambda: ops.window_blend_gather(x, z, qn, m, coef, p, step_idx=idx, out=xw))
        blend = launch_us(lambda: ops.inpaint_blend(x, z, qn[2], m, coef[2]))
        gather = launch_us(lambda: ops.window_gather(x, p, out=xw))
        return {"W": p.W, "hop": p.hop, "cover": p.cover, "fused_us": fused, "blend_then_gather_us": launch_us(two),
                "blend_us": blend, "gather_us": gather}

    res = {"what": "long-form (windowed) DDIM step at batch 1 with a source kept (fused blend-and-gather node) next to the plain "
                   "windowed step: replayed steps, eta 0; and the fused launch alone against inpaint_blend + window_gather",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "T": plan.T, "Tw": plan.Tw, "hop": plan.hop, "W": plan.W,
           "starts": list(plan.starts), "keep": keep, "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0),
           "source_hash": lib.source_hash()}
    plain, source = [], []
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
        plain.append(job(plan))
        source.append(job(src))
    a_all = [j["step_ms_median"] for j in plain]
    a, b = median(a_all), median([j["step_ms_median"] for j in source])
    res.update({"plain_windowed": plain, "with_source": source, "step_ms_plain_windowed": a, "step_ms_with_source": b,
                "with_source_over_plain": round(b / a, 4),
                "plain_repeats_spread": round((max(a_all) - min(a_all)) / a, 4),
                "launches_alone": [launches(plan), launches(window_plan(args.T, 256, 192))]})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
