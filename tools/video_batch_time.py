#!/usr/bin/env python3
"""Whole videos per GPU with co-batching: the I2VGen-XL network with synthetic FULL weights, 768x448, 16 frames, 50 steps, the
batched video sampler (tweediemix_amd.video.VideoSampler over i2vgen.I2VVideoPlan) at S = 1, 2, 4 videos per UNet call in one
process.  Per S: build, one warm-up video (both graphs recorded), then `--videos` timed videos; seconds per video = host wall time
between device synchronisations / S.  Host clock, not HIP events: events around replays of a two-stream graph are unsafe on
this ROCm (tools/README.md, refine_video.py).  Prints one JSON line per S.

python tools/video_batch_time.py [--S 1,2,4] [--steps 50] [--streams 2] [--res_w 768 --res_h 448] [--frames 16] [--videos 1]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", default="1,2,4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--streams", type=int, default=2, choices=[1, 2])
    ap.add_argument("--res_w", type=int, default=768)
    ap.add_argument("--res_h", type=int, default=448)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--videos", type=int, default=1, help="timed batches per S (after one warm-up batch)")
    a = ap.parse_args()
    from tweediemix_amd import i2vgen as I, video as V
    from tweediemix_amd.weights import synthetic_i2vgen_state_dict
    cfg = I.FULL
    Fr, h, w = a.frames, a.res_h // 8, a.res_w // 8
    Wt = I.I2VWeights(cfg, synthetic_i2vgen_state_dict(cfg))
    acp, kw = V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True, steps_offset=1,
                                                  set_alpha_to_one=False))
    sch = V.VideoSchedule(acp, a.steps, **kw)
    for S in [int(s) for s in a.S.split(",")]:
        g = torch.Generator().manual_seed(S)
        fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0] * 2 * S), torch.randn(2 * S, 4, Fr, h, w, generator=g),
                                      torch.randn(2 * S, cfg.cross_dim, generator=g), torch.randn(2 * S, 77, cfg.cross_dim, generator=g))
        t0 = time.time()
        plan = I.I2VVideoPlan(Wt, S, Fr, h, w, fe, ctx, ilf, streams=a.streams)
        build_s = time.time() - t0
        smp = V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.02), 0.7, clips=2 * S, frames=Fr))
        x = torch.randn(S, 4, Fr, h, w, generator=g).cuda()
        out = smp.sample(x)                               # warm-up video: records the two graphs
        torch.cuda.synchronize()
        times = []
        for _ in range(a.videos):
            torch.cuda.synchronize()
            t0 = time.time()
            out = smp.sample(x)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        best = min(times)
        print(json.dumps(dict(S=S, streams=a.streams, steps=a.steps, frames=Fr, res=[a.res_w, a.res_h], build_s=round(build_s, 2),
                              s_per_batch=round(best, 3), s_per_video=round(best / S, 3), ms_per_step_per_video=round(1000 * best / S / a.steps, 2),
                              finite=bool(torch.isfinite(out).all()), graphs=len(smp.graphs))), flush=True)
        del smp, plan, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
