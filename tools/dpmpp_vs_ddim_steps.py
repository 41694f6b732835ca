"""Wall time of a DPM-Solver++(2M) job against a DDIM job at eta 0, in one process on cuda:0: audioldm2-full (random-init weights), 8
prompts, guidance 3.5, --steps sampling steps (default 25) through LatentDiffusion.sample_log, the sampler alone (no VAE, no vocoder).
Per job: wall ms (host clock around the synchronised call) and the per-step GPU time (events recorded by the step callback; median
over the replayed steps, i.e. from the fourth step on).  Each sampler runs --jobs jobs back to back; the first pays the packing of
the weights and (DDIM) the capture of the graph it then reuses across jobs, where 2M captures its step graph anew in every job.
The expectation to confirm or refute: a 2M step costs a DDIM step, a 2M job about one capture more.  A measurement, not a bar.
Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    B = args.batch
    cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
    uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
              for k, m in ld.cond_stage_model_metadata.items()}

    def job(sampler):
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
                      unconditional_conditioning=uncond, callback=cb, **({} if sampler is None else {"sampler": sampler}))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
        return {"wall_ms": round(wall, 2), "step_ms_median": round(per[len(per) // 2], 3), "step_ms_min": round(per[0], 3),
                "steps": len(events)}

    res = {"what": "sampler wall time, DPM-Solver++(2M) vs DDIM at eta 0 (sample_log only)", "model": "audioldm2-full", "batch": B,
           "guidance": 3.5, "steps": args.steps, "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0),
           "source_hash": lib.source_hash(), "ddim": [], "dpmpp_2m": []}
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
        res["ddim"].append(job(None))
        res["dpmpp_2m"].append(job("dpmpp_2m"))
    d, p = res["ddim"][-1], res["dpmpp_2m"][-1]
    res["last_job"] = {"dpmpp_minus_ddim_wall_ms": round(p["wall_ms"] - d["wall_ms"], 2),
                       "dpmpp_over_ddim_step": round(p["step_ms_median"] / d["step_ms_median"], 4),
                       "extra_wall_in_ddim_steps": round((p["wall_ms"] - d["wall_ms"]) / d["step_ms_median"], 2)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
