"""What guidance rescale costs per replayed sampling step, in one process on cuda:0: audioldm2-full (random-init weights), DDIM at eta 0,
guidance 3.5, --steps sampling steps (default 50) through LatentDiffusion.sample_log, the sampler alone (no VAE, no vocoder), at each
batch of --batches (default 8 and 1).  Two arms, guidance_rescale 0.0 and --phi (default 0.7), alternate job by job, --jobs jobs
each.  Per job: wall ms (host clock around the synchronised call) and the per-step GPU time (events recorded by the step callback;
median over the replayed steps, i.e. from the fourth step on).  The two arms are different launch sequences, so each job captures
its step graph anew (the DDIM graph cache holds one geometry at a time): the wall times carry one capture each, alike in both arms.
The expectation to confirm or refute: one more dependent launch moving three slabs of B x 32 768 floats is below 1 % of a step.
A measurement, not a bar.  Prints one JSON object; --out also writes it."""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--phi", type=float, default=0.7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256

    def job(B, cond, uncond, phi):
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
                      unconditional_conditioning=uncond, callback=cb, guidance_rescale=phi)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
        return {"wall_ms": round(wall, 2), "step_ms_median": round(median(per), 4), "step_ms_min": round(per[0], 4),
                "steps": len(events)}

    res = {"what": "replayed DDIM step (eta 0) with guidance_rescale against without (sample_log only)", "model": "audioldm2-full",
           "guidance": 3.5, "phi": args.phi, "steps": args.steps, "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0),
           "source_hash": lib.source_hash(), "batches": {}}
    for B in args.batches:
        cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        plain, rescaled = [], []
        for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
            plain.append(job(B, cond, uncond, 0.0))
            rescaled.append(job(B, cond, uncond, args.phi))
        p, r = median([j["step_ms_median"] for j in plain]), median([j["step_ms_median"] for j in rescaled])
        res["batches"][str(B)] = {"plain": plain, "rescaled": rescaled, "step_ms_plain": p, "step_ms_rescaled": r,
                                  "rescaled_minus_plain_us": round((r - p) * 1e3, 1), "rescaled_over_plain": round(r / p, 4)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
