"""What a step of a seamless loop costs under moving window phases next to the same loop on the fixed ring, in one
process on cuda:0: audioldm2-full (random-init weights), DDIM at eta 0, guidance 3.5, --steps schedule steps (default 20), --jobs
jobs per arm (default 5), the arms alternating job by job.

 1. phased against ring: a 30 s job at batch 1, T = 768 frames through four windows of the trained 256 frames (starts 0, 192, 384,
    576), the ring plan against the same plan under windows.phase_table(..., "golden").  The same UNet rows and the same graph
    shape: the steps differ in the gather and merge nodes alone, which read one int32 of a table more.  THE YARDSTICK: phased /
    ring of this one call, next to the spread among the ring arm's own repeats (box-to-box spread is several per cent).  The ring
    arm is the parent's kernels.
 2. the same for the loop of the trained length: the ring plan (256, 256, 192), two half-shifted windows, gap 128.
 3. each phased launch alone next to its ring sibling, reading row 1 of the golden table, on the step's shapes (x [1, 8, 768, 16] -> 4
    windows; eps [2, 4, 8, 256, 16] -> [2, 1, 8, 768, 16]; the blend-gather with a one-row q-noise table) and on the mel case
    (2, (160, 64, 48), 1, 64) — the one shape of the tests where a launch is not launch-bound: GPU time per launch from events around
    --reps back-to-back launches.
Per-step GPU time from events recorded by the step callback, median over the replayed steps (from the fourth step on) (sample_log
only: no VAE, no vocoder).  A measurement, not a bar.  Prints one JSON object; --out also writes it.

--launches-only skips 1 and 2 (no model is built) and times in 3, next to the ring and phased launches, the launches of the linear
plan of the same key and of a row plan over it (three prompts), each from 16-byte aligned tensors and from tensors one float off
(the scalar path): every window kernel of csrc/windows.hip at both access widths.  With $ALDM_LIB_PATH naming another build of the
library, one such process per build compares the two builds launch by launch."""
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
    ap.add_argument("--launches-only", action="store_true")
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.windows import phase_table, prompt_weights, row_plan, window_plan, with_phase
    from oracle import cases
    lib.load()
    ld = None
    if not args.launches_only:
        ld = build_model(model_name="audioldm2-full").cuda()
        ld.latent_t_size = 256
    ring = window_plan(args.T, 256, args.hop, ring=True)
    short = window_plan(256, 256, 192, ring=True)
    phased = with_phase(ring, phase_table(ring, args.steps, "golden"))
    short_phased = with_phase(short, phase_table(short, args.steps, "golden"))

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

    def launches(key, B, C, F, row=1, shift=0, every_plan=False):
        """The three launches of the ring plan `key` and of the same plan under the golden table, read at row `row`; every_plan:
        of the linear plan `key` and of a row plan over it too.  shift = 1: every tensor starts one float off a 16-byte boundary."""
        r = window_plan(*key, ring=True)
        p = with_phase(r, phase_table(r, args.steps, "golden"))
        tab, idx = p.phase.cuda(), torch.full((1,), row, device="cuda", dtype=torch.int32)

        def randn(*shape):
            n = 1
            for d in shape:
                n *= d
            return torch.randn(n + shift, device="cuda")[shift:].view(shape)
        x = randn(B, C, r.T, F)
        x0, qn, mask = randn(*x.shape), randn(*x.shape), randn(*x.shape).gt_(0)
        coef = torch.tensor([0.8, 0.6], device="cuda")

        def three(plan, **kw):
            G = plan.R if getattr(plan, "rows", None) is not None else plan.W
            xw, eps, out = randn(G * B, C, plan.Tw, F), randn(2, G * B, C, plan.Tw, F), randn(2, B, C, plan.T, F)
            return {"gather_us": launch_us(lambda: ops.window_gather(x, plan, out=xw, **kw)),
                    "merge_us": launch_us(lambda: ops.window_merge(eps, plan, out=out, **kw)),
                    "blend_gather_us": launch_us(lambda: ops.window_blend_gather(x, x0, qn, mask, coef, plan, out=xw,
                                                                                 step_idx=kw.get("step_idx"), phase=kw.get("phase")))}
        t = {"ring": three(r), "phased": three(p, phase=tab, step_idx=idx)}
        if every_plan:
            lin = window_plan(*key)
            rows = row_plan(lin, prompt_weights(lin.T, [lin.T // 3, 2 * lin.T // 3], lin.Tw // 4))
            t.update({"linear": three(lin), "rows": three(rows), "R": rows.R})
        return dict(t, key=list(key), B=B, C=C, F=F, W=r.W, starts=list(r.starts), phase=int(p.phase[row]), shift=shift,
                    phased_over_ring={k: round(t["phased"][k] / t["ring"][k], 4) for k in t["ring"]})

    shapes = [((args.T, 256, args.hop), 1, 8, 16), ((160, 64, 48), 2, 1, 64)]
    if args.launches_only:
        res = {"what": "every window launch alone, on the step's shapes and on the mel case, aligned and one float off",
               "device": torch.cuda.get_device_name(0), "lib": lib.LIB_PATH, "reps": args.reps,
               "launches_alone": [launches(*sh, shift=shift, every_plan=True) for shift in (0, 1) for sh in shapes]}
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return

    res = {"what": "DDIM step of a seamless loop under moving window phases (the golden table) next to the same loop on the fixed "
                   "ring, at 30 s and at the trained length: replayed steps, batch 1, eta 0; and each phased launch alone next to "
                   "its ring sibling, on the step's shapes and on the mel case",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "T": ring.T, "Tw": ring.Tw, "hop": ring.hop, "W": ring.W,
           "ring_starts": list(ring.starts), "phases": phased.phase.tolist(), "phases_256": short_phased.phase.tolist(),
           "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash()}
    c1, u1 = conds(1)
    arms = {"ring": [], "phased": [], "ring_256": [], "phased_256": []}
    for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits all arms alike
        arms["ring"].append(job(1, c1, u1, windows=ring))
        arms["phased"].append(job(1, c1, u1, windows=phased))
        arms["ring_256"].append(job(1, c1, u1, windows=short))
        arms["phased_256"].append(job(1, c1, u1, windows=short_phased))
    med = {k: median([j["step_ms_median"] for j in v]) for k, v in arms.items()}
    spread = lambda k: round((max(j["step_ms_median"] for j in arms[k]) - min(j["step_ms_median"] for j in arms[k])) / med[k], 4)
    res.update({"jobs": arms, "step_ms": med,
                "phased_over_ring": round(med["phased"] / med["ring"], 4),
                # the yardstick of that ratio: how far the ring arm's own repeats lie apart, (max - min) / median
                "ring_repeat_spread": spread("ring"),
                "phased_256_over_ring_256": round(med["phased_256"] / med["ring_256"], 4),
                "ring_256_repeat_spread": spread("ring_256"),
                "launches_alone": [launches(*sh) for sh in shapes]})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
