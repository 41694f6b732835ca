"""What audio-to-audio generation costs next to text-to-audio, in one process on cuda:0: audioldm2-full (random-init weights), DDIM at
eta 0, guidance 3.5, --steps schedule steps (default 50), at each batch of --batches (default 8 and 1), --jobs jobs per arm, the arms
alternating job by job.

 1. The replayed DDIM step (sample_log only: no VAE, no vocoder): the text-to-audio run over the whole schedule against the
    audio-to-audio run (`x_T=`, `t_start=int(--strength * steps)`).  Per-step GPU time from events recorded by the step callback,
    median over the replayed steps (from the fourth step on).  The step graph is the same launch sequence in both; the two runs
    differ in the number of steps, which is part of the graph cache's key, so each job of an alternating pair captures anew.
 2. From the mel to the start latent, wall ms around a synchronised call, host draws and uploads included:
      new:  AutoencoderKL.encode_moments_cl -> two host randn -> ops.posterior_qsample (one launch);
      old:  AutoencoderKL.encode -> posterior.sample() * scale_factor -> host randn -> DDIMSampler.stochastic_encode (the layout
            transpose, ~6 element-wise launches, a host round trip for the coefficients).  The DDIM schedule both routes need once
            per job is built before, outside both timed arms.
    ... and the same two routes from the encoder's MOMENTS on (the encoder itself, identical in both, left out; noises already on
    the device): the part the kernel replaces.
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
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.ddim import DDIMSampler, sdedit_plan
    from audioldm2_amd.pipeline import build_model, seed_everything
    from audioldm2_amd.vae import DiagonalGaussianDistribution
    from oracle import cases
    lib.load()
    ld = build_model(model_name="audioldm2-full").cuda()
    ld.latent_t_size = 256
    t_enc, _, sa, so = sdedit_plan(args.strength, args.steps, ld.alphas_cumprod, ld.num_timesteps)
    scale = float(ld.scale_factor)

    def job(B, cond, uncond, x_T=None):
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
                      unconditional_conditioning=uncond, callback=cb,
                      **({} if x_T is None else {"x_T": x_T, "t_start": t_enc}))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = sorted(a.elapsed_time(b) for a, b in zip(events[2:-1], events[3:]))
        return {"wall_ms": round(wall, 2), "step_ms_median": round(median(per), 4), "step_ms_min": round(per[0], 4),
                "steps": len(events)}

    def timed(fn):
        out = []
        for _ in range(args.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        out = out[2:]   # two warm-up calls (weight packing, allocator)
        return {"ms_median": round(median(out), 3), "ms_min": round(min(out), 3), "reps": len(out)}

    res = {"what": "audio-to-audio next to text-to-audio: replayed DDIM step (eta 0), and mel -> start latent by the new kernel / the old route",
           "model": "audioldm2-full", "guidance": 3.5, "steps": args.steps, "strength": args.strength, "t_enc": t_enc,
           "mode": ops.MMA_MODE, "device": torch.cuda.get_device_name(0), "source_hash": lib.source_hash(), "batches": {}}
    sampler = DDIMSampler(ld)
    # the schedule is built once per job on either route (the new one builds it inside sampler.sample()): outside the timed arms
    sampler.make_schedule(args.steps, ddim_eta=0.0, verbose=False)
    for B in args.batches:
        cond = ld.get_learned_conditioning_dict(cases.e2e_batch(B))
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        x = cases.e2e_masked_batch(B)["log_mel_spec"].unsqueeze(1).float().contiguous().cuda()
        coef = torch.tensor([scale, sa, so], dtype=torch.float32).cuda()
        shape = (B, 8, 256, 16)
        idx = torch.full((B,), t_enc - 1, dtype=torch.long)

        def new_route():
            m = ld.first_stage_model.encode_moments_cl(x)
            return ops.posterior_qsample(m, torch.randn(shape).cuda(), torch.randn(shape).cuda(), coef)[1]

        def old_route():
            z = ld.get_first_stage_encoding(ld.encode_first_stage(x))
            return sampler.stochastic_encode(z, idx, noise=torch.randn(shape))
        moments = ld.first_stage_model.encode_moments_cl(x)
        n_post, n_enc = torch.randn(shape).cuda(), torch.randn(shape).cuda()

        def new_tail():
            return ops.posterior_qsample(moments, n_post, n_enc, coef)[1]

        def old_tail():
            post = DiagonalGaussianDistribution(ops.nhwc_to_nchw(moments))
            z = ld.scale_factor * (post.mean + post.std * n_post)
            return sampler.stochastic_encode(z, idx, noise=n_enc)
        enc = {"new": timed(new_route), "old": timed(old_route), "new_from_moments": timed(new_tail),
               "old_from_moments": timed(old_tail)}
        x_T = new_route()
        t2a, a2a = [], []
        for _ in range(args.jobs):   # interleaved, so a drift of the clocks hits both alike
            t2a.append(job(B, cond, uncond))
            a2a.append(job(B, cond, uncond, x_T))
        p, r = median([j["step_ms_median"] for j in t2a]), median([j["step_ms_median"] for j in a2a])
        res["batches"][str(B)] = {"text_to_audio": t2a, "audio_to_audio": a2a, "step_ms_text_to_audio": p, "step_ms_audio_to_audio": r,
                                  "audio_over_text": round(r / p, 4), "mel_to_start_latent_ms": enc,
                                  "old_over_new": round(enc["old"]["ms_median"] / enc["new"]["ms_median"], 3),
                                  "old_over_new_from_moments": round(enc["old_from_moments"]["ms_median"] /
                                                                     enc["new_from_moments"]["ms_median"], 2)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
