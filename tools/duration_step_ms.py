"""UNet step time (ms) per latent length for the two duration-capable models (audioldm_48k, audioldm_16k_crossattn_t5): one
eps prediction of a CFG batch (8 prompts x 2) on cuda:0, median of --iters timed forwards after --warmup, in bf16x6 and f16x3.
latent_t in {64, 96, 128, 160, 192}: 5 / 7.5 / 10 / 12.5 / 15 s of audioldm_48k (12.8 frames per second) and 2.5 .. 7.5 s of the
16 kHz model (25.6 frames per second); 96 and 160 have a deepest self-attention of 48 / 80 tokens (48k) — a ragged last key tile.
Each row also times the same forward with the pre-split self-attention off (ms_fp32_kv_attention).  Prints one JSON object; --out
also writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from audioldm2_amd import lib, ops
    from audioldm2_amd.pipeline import default_audioldm_config
    from audioldm2_amd import unet as unet_mod
    from audioldm2_amd.unet import UNetModel
    from oracle import cases
    lib.load()
    res = {"what": "UNet eps forward of a CFG batch, ms (median)", "batch": args.batch, "source_hash": lib.source_hash(),
           "rows": []}
    for model_name in ("audioldm_48k", "audioldm_16k_crossattn_t5"):
        p = default_audioldm_config(model_name)["model"]["params"]
        cfg, F_ = p["unet_config"]["params"], p["latent_f_size"]
        for mode in ("bf16x6", "f16x3"):
            prev = ops.set_mma(mode)
            torch.manual_seed(0)
            m = UNetModel(**cfg).eval()
            for T in (64, 96, 128, 160, 192):
                x, t, ctxs, masks, y = cases.unet_inputs(cfg, args.batch, T, F_, 32)
                a = dict(y=None if y is None else y.cuda(), context_list=[c.cuda() for c in ctxs],
                         context_attn_mask_list=[k.cuda() for k in masks])
                xc, tc = x.cuda(), t.cuda()

                def timed():
                    with torch.no_grad():
                        for _ in range(args.warmup):
                            m(xc, tc, **a)
                        ts = []
                        for _ in range(args.iters):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            m(xc, tc, **a)
                            e1.record()
                            torch.cuda.synchronize()
                            ts.append(e0.elapsed_time(e1))
                    ts.sort()
                    return ts[len(ts) // 2]
                ms = timed()
                row = {"model": model_name, "mode": mode, "latent_t": T, "ms": round(ms, 3),
                       "ms_per_latent_frame": round(ms / T, 4)}
                # the same forward with every self-attention on the fp32-K/V path (the pre-split path off): what the ragged
                # pre-split path (aldm_vt_regroup + the TAIL kernel) saves or costs against the path it replaces
                unet_mod.PRESPLIT_ATTENTION = False
                try:
                    row["ms_fp32_kv_attention"] = round(timed(), 3)
                finally:
                    unet_mod.PRESPLIT_ATTENTION = True
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del m
            torch.cuda.empty_cache()
            ops.set_mma(prev)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
