"""What a step of a seamless loop (windowed diffusion on a ring plan) costs next to the linear windowed step, in one
process on cuda:0: audioldm2-full (random-init weights), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20), --jobs
jobs per arm (default 5), the arms alternating job by job.

 1. ring against linear: a 30 s job at batch 1, T = 768 frames through windows of the trained 256 frames at the default hop 192 —
    four windows either way (ring starts 0, 192, 384, 576; linear 0, 192, 384, 512), the same UNet rows, so the steps differ in the
    gather and merge nodes alone.  THE YARDSTICK: ring / linear of this one call, next to the spread among the linear arm's own
    repeats (box-to-box spread is several per cent).
 2. the loop of the trained length: the ring plan (256, 256, 192) — two half-shifted windows, batch 1 — against a plain DDIM job at
    batch 2: the same UNet rows, no windows.
 3. each ring launch alone next to its linear sibling on the step's shapes (x [1, 8, 768, 16] -> 4 windows; eps [2, 4, 8, 256, 16]
    -> [2, 1, 8, 768, 16]; the blend-gather with a one-row q-noise table): GPU time per launch from events around --reps back-to-back
    launches.
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
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--hop", type=int, default=192)
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
    ring, linear = window_plan(args.T, 256, args.hop, ring=True), window_plan(args.T, 256, args.hop)
    assert ring.W == linear.W, "the arms must run the same UNet rows"
    short = window_plan(256, 256, 192, ring=True)

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
        x0, qn, mask = torch.randn_like(x), torch.randn_like(x), (torch.rand_like(x) > 0.5).float()
        coef = torch.tensor([0.8, 0.6], device="cuda")
        xw = torch.empty(p.W, 8, p.Tw, 16, device="cuda")
        eps = torch.randn(2, p.W, 8, p.Tw, 16, device="cuda")
        out = torch.empty(2, 1, 8, p.T, 16, device="cuda")
        return {"ring": p.ring, "W": p.W, "starts": list(p.starts), "cover": p.cover,
                "gather_us": launch_us(lambda: ops.window_gather(x, p, out=xw)),
                "merge_us": launch_us(lambda: ops.window_merge(eps, p, out=out)),
                "blend_gather_us": launch_us(lambda: ops.window_blend_gather(x, x0, qn, mask, coef, p, out=xw))}

    res = {"what": "DDIM step of a seamless loop (ring plan) at batch 1 next to the linear windowed step of the same numbers, and the "
                   "loop of the trained length next to a plain batch-2 step: replayed steps, eta 0; and each ring launch alone next "
                   "to its linear sibling",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "T": ring.T, "Tw": ring.Tw, "hop": ring.hop, "W": ring.W,
           "ring_starts": list(ring.starts), "linear_starts": list(linear.starts), "mode": ops.MMA_MODE,
           "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash()}
    c1, u1 = conds(1)
    c2, u2 = conds(2)
    arms = {"ring": [], "linear": [], "ring_256": [], "plain_batch_2": []}
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits all arms alike
        arms["ring"].append(job(1, c1, u1, windows=ring))
        arms["linear"].append(job(1, c1, u1, windows=linear))
        arms["ring_256"].append(job(1, c1, u1, windows=short))
        arms["plain_batch_2"].append(job(2, c2, u2))
    med = {k: median([j["step_ms_median"] for j in v]) for k, v in arms.items()}
    lin = [j["step_ms_median"] for j in arms["linear"]]
    res.update({"jobs": arms, "step_ms": med,
                "ring_over_linear": round(med["ring"] / med["linear"], 4),
                # the yardstick of that ratio: how far the linear arm's own repeats lie apart, (max - min) / median
                "linear_repeat_spread": round((max(lin) - min(lin)) / med["linear"], 4),
                "ring_256_over_plain_batch_2": round(med["ring_256"] / med["plain_batch_2"], 4),
                "launches_alone": [launches(ring), launches(linear)]})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
