"""Step cost of composable guidance (`Composed`) against the plain guided step AT THE SAME NUMBER OF UNET ROWS, in one
process on cuda:0 with the arms alternating: audioldm2-full (random-init weights), DDIM at eta 1, --steps sampling steps (default
25), guidance 3.5, through LatentDiffusion.sample_log — the sampler alone (no VAE, no vocoder).
  * composed: batch 4 under K = 3 prompts — 4 groups x 4 samples = 16 UNet rows, the context-free prefix on 4;
  * plain:    batch 8 under one prompt     — 2 groups x 8 samples = 16 UNet rows, the context-free prefix on 8.
So the ratio says what the group pass and the compose launch cost beyond the rows they add; the pass itself grows as (K+1)/2 against
the guided pass at the same batch, which this tool does not re-measure.  Both arms again under ALDM_CFG_SHARE=0 (x repeated, no
shared prefix).  Per job: the replayed step's GPU time (events recorded by the step callback, which declares `uses_rng = False`; median
over the steps from the fourth on).  Then the compose launch alone at the composed job's shape, eager and back to back, next to
ops.ddim_step_indexed on the same latent.
Ratios only: boxes differ by about +-6 %.  Each ratio is quoted next to the spread among the plain arm's own repeats.  A measurement,
not a bar; what composed prompts sound like on a trained model is not measured here or anywhere in the project.  Prints one JSON
object; --out also writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, B_COMPOSED, B_PLAIN = 3, 4, 8
WEIGHTS = [1.0, 0.6, -0.4]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v):
    """(max - min) / median of one arm's own repeats."""
    return round((max(v) - min(v)) / median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.sampling import Composed, compose_table, guidance_table
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    unet = ld.model.diffusion_model
    res = {"what": "replayed DDIM step: K = 3 composed prompts at batch 4 against the plain guided step at batch 8 (16 UNet rows each)",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "mode": ops.MMA_MODE, "K": K,
           "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash(), "ratios_only": "boxes differ by about +-6 %",
           "unmeasured": "what composed prompts sound like on a trained model"}

    def conditioning(B):
        cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        return cond, uncond
    cond4, uncond4 = conditioning(B_COMPOSED)
    cond8, uncond8 = conditioning(B_PLAIN)
    arms = {"composed": (Composed([cond4] * K, WEIGHTS), uncond4, B_COMPOSED), "plain": (cond8, uncond8, B_PLAIN)}

    def job(cond, uncond, B):
        events = []

        def cb(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
        cb.uses_rng = False   # keep the threaded noise feed
        seed_everything(0)
        torch.cuda.synchronize()
        ld.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=args.steps, eta=1.0, unconditional_guidance_scale=3.5,
                      unconditional_conditioning=uncond, callback=cb)
        torch.cuda.synchronize()
        per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
        return per[len(per) // 2]

    def compare():
        rec = {name: [] for name in arms}
        for _ in range(args.jobs):   # alternating, so a drift of the clocks hits both arms alike
            for name, (cond, uncond, B) in arms.items():
                rec[name].append(job(cond, uncond, B))
        unet.drop_step_caches()
        # the first job of an arm pays the packing of the weights: the summary is over the later ones
        later = {name: v[1:] for name, v in rec.items()}
        return {"composed_over_plain_step": round(median(later["composed"]) / median(later["plain"]), 4),
                "spread_among_plain_repeats": spread(later["plain"]), "spread_among_composed_repeats": spread(later["composed"]),
                "jobs_per_arm": args.jobs}

    res["shared_prefix"] = compare()
    os.environ["ALDM_CFG_SHARE"] = "0"
    try:
        res["ALDM_CFG_SHARE=0"] = compare()
    finally:
        os.environ.pop("ALDM_CFG_SHARE")

    # the compose launch alone, eager, back to back, in place on static operands of the composed job's shape — next to the DDIM step
    # launch on the same latent
    shape = (B_COMPOSED, ld.channels, ld.latent_t_size, ld.latent_f_size)
    eps = torch.randn((K + 1,) + shape).cuda()
    tab = compose_table(Composed([None] * K, WEIGHTS).weights).cuda()
    idx = torch.zeros(1, device="cuda", dtype=torch.int32)
    x, noise, slab = torch.randn(shape).cuda(), torch.randn((1,) + shape).cuda(), torch.randn(shape).cuda()
    coef = guidance_table(torch.tensor([[0.6, 0.8, 0.9, 0.1, 0.4]]), 3.5, True).cuda()
    launch = {"compose": lambda: ops.cfg_compose_indexed(eps, tab, idx, pair=True),
              "ddim_step": lambda: ops.ddim_step_indexed(x, eps[:2], noise, coef, idx, slab)}
    us = {k: [] for k in launch}
    for rep in range(6):
        for k, f in launch.items():
            x.normal_()      # keep the in-place recurrences bounded
            eps.normal_()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                f()
            b.record()
            torch.cuda.synchronize()
            if rep:   # the first repeat warms up
                us[k].append(a.elapsed_time(b) * 1e3 / args.launches)
    res["launch_alone"] = {"elements_per_group": x.numel(), "groups": K + 1, "launches_per_repeat": args.launches,
                           "compose_over_ddim_step_launch": round(median(us["compose"]) / median(us["ddim_step"]), 4),
                           "spread_among_ddim_step_repeats": spread(us["ddim_step"]),
                           "spread_among_compose_repeats": spread(us["compose"])}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
