"""What a step of long-form generation under a prompt timeline costs, in one process on cuda:0: audioldm2-full
(random-init weights), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20), --jobs jobs per arm, the arms alternating job
by job.

 1. timeline: a 30 s job at batch 1 — T = 768 frames, windows of the trained 256 frames at the default hop 192 (W = 4), three prompts
    with boundaries at 256 and 512 frames cross-faded over 64 frames: R = 8 rows (every window hears two prompts).  The UNet pass
    runs on 8 rows (16 under guidance); the step adds the row gather and the row merge.
 2. plain: a DDIM job at batch R = 8 of the same model at the trained length: the same UNet rows, no windows.  THE YARDSTICK: the
    figure that matters is timeline / plain of this one call (box-to-box spread is several per cent), next to the spread among the
    plain arm's own repeats.
 3. windowed: the same 30 s job under ONE prompt (W = 4 window rows): timeline / windowed is the price of the timeline.
 4. the three row launches alone, eager and back to back, on the step's shapes (x [1, 8, 768, 16] -> 8 rows; eps [2, 8, 8, 256, 16]
    -> [2, 1, 8, 768, 16]), next to the window launches of the base plan: GPU time per launch from events around --reps launches.
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.windows import PerPrompt, prompt_weights, row_plan, window_plan
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    T, bounds, tau = 768, [256, 512], 64
    plan = window_plan(T, 256, 192)
    rp = row_plan(plan, prompt_weights(T, bounds, tau))
    R, W = rp.R, plan.W

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

    def launches(p, n):
        x = torch.randn(1, 8, p.T, 16, device="cuda")
        x0, qn, m = torch.randn_like(x), torch.randn_like(x), torch.zeros_like(x)
        m[:, :, :200] = 1.0
        coef = torch.tensor([[0.8, 0.6]], device="cuda")
        xw = torch.empty(n, 8, p.Tw, 16, device="cuda")
        eps = torch.randn(2, n, 8, p.Tw, 16, device="cuda")
        out = torch.empty(2, 1, 8, p.T, 16, device="cuda")
        return {"rows": n, "cover": p.cover, "gather_us": launch_us(lambda: ops.window_gather(x, p, out=xw)),
                "merge_us": launch_us(lambda: ops.window_merge(eps, p, out=out)),
                "blend_gather_us": launch_us(lambda: ops.window_blend_gather(x, x0, qn, m, coef, p, out=xw))}

    res = {"what": "DDIM step of a 30 s batch-1 job under a 3-prompt timeline (R rows) next to a plain step at batch R and to the "
                   "one-prompt windowed step (W rows): replayed steps, eta 0; and the three row launches alone",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "T": T, "Tw": plan.Tw, "hop": plan.hop, "W": W, "R": R,
           "boundaries": bounds, "transition": tau, "rows": [list(r) for r in rp.rows], "row_cover": rp.cover,
           "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash()}
    c1, u1 = conds(1)
    cR, uR = conds(R)
    per_prompt = PerPrompt([c1, c1, c1])   # the cost does not depend on what the prompts say
    timeline, plain, windowed = [], [], []
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits all alike
        timeline.append(job(1, per_prompt, u1, windows=rp))
        plain.append(job(R, cR, uR))
        windowed.append(job(1, c1, u1, windows=plan))
    med = lambda jobs: median([j["step_ms_median"] for j in jobs])
    t, p, w = med(timeline), med(plain), med(windowed)
    pm = [j["step_ms_median"] for j in plain]
    res.update({"timeline_batch_1": timeline, f"plain_batch_{R}": plain, "windowed_batch_1": windowed, "step_ms_timeline": t,
                "step_ms_plain": p, "step_ms_windowed": w, "timeline_over_plain": round(t / p, 4),
                "plain_spread": round((max(pm) - min(pm)) / p, 4), "timeline_over_windowed": round(t / w, 4),
                "launches_alone": {"rows": launches(rp, R), "windows": launches(plan, W)}})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
