"""What a step of long-form (windowed) generation costs next to a plain step over as many UNet rows, in one process on cuda:0:
audioldm2-full (random-init weights), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20), --jobs jobs per arm, the arms
alternating job by job.

 1. windowed: a 30 s job at batch 1 — a long latent of T = 768 frames through W = 3 windows of the trained 256 frames (--hop 256:
    the hop at which 768 frames take exactly three windows; the default hop of generate_batch_long, 192, takes four).  The UNet pass
    runs on 3 window rows (6 under guidance); the step adds the window gather and the window merge.
 2. plain: a DDIM job at batch 3 of the same model at the trained length: the same UNet rows, no windows.  THE YARDSTICK: the
    figure that matters is windowed / plain of this one call (box-to-box spread is several per cent).
 3. the two new launches alone, on the step's shapes (x [1, 8, 768, 16] -> 3 windows; eps [2, 3, 8, 256, 16] -> [2, 1, 8, 768, 16]),
    for the 3-window plan and for the default-hop 4-window plan (which overlaps, so its merge does arithmetic): GPU time per launch
    from events around --reps back-to-back launches.
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
    from audioldm2_amd.windows import window_plan
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    plan = window_plan(args.T, 256, args.hop)
    W = plan.W

    def conds(B):
        cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        return cond, uncond

    def job(B, cond, uncond, **kw):
        events = []

        def cb(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
        cb.uses_rng = False   # DDIM keeps its threaded noise feed
        seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=args.steps, eta=0.0, unconditional_guidance_scale=3.5,
                      unconditional_conditioning=uncond, callback=cb, **kw)
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
        x = torch.randn(1, 8, p.T, 16, device="cuda")
        xw = torch.empty(p.W, 8, p.Tw, 16, device="cuda")
        eps = torch.randn(2, p.W, 8, p.Tw, 16, device="cuda")
        out = torch.empty(2, 1, 8, p.T, 16, device="cuda")
        return {"W": p.W, "hop": p.hop, "cover": p.cover, "gather_us": launch_us(lambda: ops.window_gather(x, p, out=xw)),
                "merge_us": launch_us(lambda: ops.window_merge(eps, p, out=out))}

    res = {"what": "long-form (windowed) DDIM step at batch 1 next to a plain step at batch W: replayed steps, eta 0; and the two "
                   "new launches alone",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "T": plan.T, "Tw": plan.Tw, "hop": plan.hop, "W": W,
           "starts": list(plan.starts), "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0),
           "source_hash": lib.source_hash()}
    c1, u1 = conds(1)
    cW, uW = conds(W)
    windowed, plain = [], []
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
        windowed.append(job(1, c1, u1, windows=plan))
        plain.append(job(W, cW, uW))
    w, p = median([j["step_ms_median"] for j in windowed]), median([j["step_ms_median"] for j in plain])
    res.update({"windowed_batch_1": windowed, f"plain_batch_{W}": plain, "step_ms_windowed": w, "step_ms_plain": p,
                "windowed_over_plain": round(w / p, 4),
                "launches_alone": [launches(plan), launches(window_plan(args.T, 256, 192))]})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
