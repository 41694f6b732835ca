"""Step cost of the DPM-Solver++(2M) SDE sampler (sampler="dpmpp_2m_sde") against DPM-Solver++(2M) and against DDIM at
eta 1, in one process on cuda:0 with the arms alternating: audioldm2-full (random-init weights), batch 8 and batch 1, --steps sampling
steps (default 25), guidance 3.5, through LatentDiffusion.sample_log — the sampler alone (no VAE, no vocoder).
Per job: the sampling loop's wall ms (host clock around the synchronised call) and the replayed step's GPU time (events recorded by
the step callback, which declares `uses_rng = False` so the stochastic arms keep their threaded noise feed; median over the steps
from the fourth on).  Then the step launch alone at the job's latent shape: ops.dpmpp_sde_step_indexed, ops.dpmpp_step_indexed and
ops.ddim_step_indexed, eager and back to back, --launches of each per repeat, alternating.
The expectation to confirm or refute: ratios near 1 — one more 4-byte read per element in a launch-bound kernel.  Each ratio is quoted
next to the spread among one arm's own repeats.  A measurement, not a bar; what 25 steps of it sound like on a trained model is not
measured here or anywhere in the project.  Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = (("ddim_eta1", None, 1.0), ("dpmpp_2m", "dpmpp_2m", 0.0), ("dpmpp_2m_sde", "dpmpp_2m_sde", 1.0))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v):
    """(max - min) / median of one arm's own repeats."""
    return round((max(v) - min(v)) / median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.sampling import guidance_table
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    res = {"what": "step cost of DPM-Solver++(2M) SDE vs DPM-Solver++(2M) and DDIM at eta 1 (sample_log only; the step launch alone)",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "mode": ops.MMA_MODE,
           "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash(), "batches": {},
           "unmeasured": "audio quality of a short run on a trained model"}

    for B in args.batches:
        cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}

        def job(sampler, eta):
            events = []

            def cb(i):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events.append(e)
            cb.uses_rng = False   # the stochastic arms keep their threaded noise feed
            seed_everything(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ld.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=args.steps, eta=eta, unconditional_guidance_scale=3.5,
                          unconditional_conditioning=uncond, callback=cb, **({} if sampler is None else {"sampler": sampler}))
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
            return {"loop_ms": round(wall, 2), "step_ms_median": round(per[len(per) // 2], 4), "step_ms_min": round(per[0], 4),
                    "steps": len(events)}

        rec = {name: [] for name, _, _ in ARMS}
        for _ in range(args.jobs):   # alternating, so a drift of the clocks hits every arm alike
            for name, sampler, eta in ARMS:
                rec[name].append(job(sampler, eta))
        ld.model.diffusion_model.drop_step_caches()
        # the first job of an arm pays the packing of the weights and a capture: the summary is over the later ones
        summ = {}
        for name, _, _ in ARMS:
            later = rec[name][1:]
            summ[name] = {"step_ms": median([j["step_ms_median"] for j in later]), "loop_ms": median([j["loop_ms"] for j in later]),
                          "step_spread": spread([j["step_ms_median"] for j in later]),
                          "loop_spread": spread([j["loop_ms"] for j in later])}
        sde = summ["dpmpp_2m_sde"]
        ratios = {f"sde_over_{name}": {"step": round(sde["step_ms"] / summ[name]["step_ms"], 4),
                                       "loop": round(sde["loop_ms"] / summ[name]["loop_ms"], 4)} for name in ("dpmpp_2m", "ddim_eta1")}

        # the step launch alone, eager, back to back, on static operands of the job's shape
        shape = (B, ld.channels, ld.latent_t_size, ld.latent_f_size)
        S = 8
        x, eps, slab = torch.randn(shape).cuda(), torch.randn((2,) + shape).cuda(), torch.randn(shape).cuda()
        noise = torch.randn((S,) + shape).cuda()
        tab = torch.cat([guidance_table(torch.tensor([[0.6, 0.8, 0.9, 0.1, 0.4]]).repeat(S, 1), 3.5, True), torch.full((S, 1), 0.3)],
                        1).contiguous().cuda()
        idx = torch.full((1,), 3, device="cuda", dtype=torch.int32)
        launch = {"dpmpp_2m_sde": lambda: ops.dpmpp_sde_step_indexed(x, eps, slab, noise, tab, idx),
                  "dpmpp_2m": lambda: ops.dpmpp_step_indexed(x, eps, slab, tab, idx),
                  "ddim_eta1": lambda: ops.ddim_step_indexed(x, eps, noise, tab, idx, slab)}
        us = {k: [] for k in launch}
        for rep in range(6):
            for k, f in launch.items():
                x.normal_()   # keep the in-place recurrence bounded
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    f()
                b.record()
                torch.cuda.synchronize()
                if rep:   # the first repeat warms up
                    us[k].append(a.elapsed_time(b) * 1e3 / args.launches)
        lsum = {k: {"us_per_launch": round(median(v), 3), "spread": spread(v)} for k, v in us.items()}
        lrat = {f"sde_over_{k}": round(lsum["dpmpp_2m_sde"]["us_per_launch"] / lsum[k]["us_per_launch"], 4) for k in ("dpmpp_2m", "ddim_eta1")}
        res["batches"][str(B)] = {"jobs": rec, "summary": summ, "ratios": ratios,
                                  "step_launch_alone": {"elements": x.numel(), "launches_per_repeat": args.launches, "arms": lsum,
                                                        "ratios": lrat}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
