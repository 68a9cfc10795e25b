#!/usr/bin/env python3
"""cost of the multistep video step entry in the whole step, and whole-video times of few-step sampling (the method of
tools/solver_cost.py).

(1) One captured step of the I2VGen-XL video sampler (synthetic FULL weights, one video, 16 frames) ending in (a) tmix_vpred_step_dev -- the DDIM
step -- and (b) tmix_vpred_step_ms_dev with second-order coefficients -- one more read and write of the state's size; TWO samplers over ONE plan, so
both graphs replay the same launches on the same buffers and differ in their last launch only.  10 replays per round, three interleaved rounds, the
minimum of the rounds, the box's clock beside the numbers.
(2) Whole videos, wall time between device synchronisations, graphs on, the second run of each sampler (the first captures): DDIM 'leading' at
n = 50, the solver on the log-SNR grid at n = 20 and n = 10; a video is n UNet calls, nothing fixed.  No quality claim is attached to these.

    python tools/video_solver_cost.py [--res_w 768 --res_h 448] [--frames 16] [--streams 2] [--no-videos]"""
import argparse
import collections
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res_w", type=int, default=768)
    ap.add_argument("--res_h", type=int, default=448)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2, choices=[1, 2])
    ap.add_argument("--tiny", action="store_true", help="the tiny network (a dry run of the tool)")
    ap.add_argument("--no-videos", action="store_true")
    a = ap.parse_args()
    from tweediemix_amd import i2vgen as I, video as V
    from tweediemix_amd.weights import synthetic_i2vgen_state_dict
    cfg = I.TINY if a.tiny else I.FULL
    Fr, h, w = a.frames, a.res_h // 8, a.res_w // 8
    dev = torch.device("cuda", 0)
    Wt = I.I2VWeights(cfg, synthetic_i2vgen_state_dict(cfg))
    acp, kw = V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True, steps_offset=1,
                                                  set_alpha_to_one=False))
    g = torch.Generator().manual_seed(1)
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0] * 2), torch.randn(2, 4, Fr, h, w, generator=g), torch.randn(2, cfg.cross_dim, generator=g),
                                  torch.randn(2, 77, cfg.cross_dim, generator=g))
    plan = I.I2VVideoPlan(Wt, 1, Fr, h, w, fe, ctx, ilf, streams=a.streams)
    x_T = torch.randn(1, 4, Fr, h, w, generator=g).to(dev)

    def sampler(n, spacing="leading", **skw):
        sch = V.VideoSchedule(acp, n, **kw, spacing=spacing)
        return V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.02), 0.7, clips=2, frames=Fr), **skw)

    ddim, ms = sampler(50), sampler(50, solver="dpmpp2m")
    ts = [int(t) for t in ms.schedule.timesteps]
    i = ts.index(501)

    def ms_step():
        ms.phase.set_previous(ts[i - 1])                  # the step before was the preceding entry: second-order coefficients
        ms.step(501)
    steps = {"a: DDIM step": lambda: ddim.step(501), "b: 2M solver step": ms_step}
    res = collections.defaultdict(list)
    for _rnd in range(3):
        for name, step in steps.items():
            for s in (ddim, ms):
                s.state.copy_(x_T)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 100)
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    assert float(ms.params[5]) != 0.0 and sorted(ddim.graphs) == [False] and sorted(ms.graphs) == [(False, "ms")]
    print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
    print(f"video step, one video, {Fr} frames {a.res_w}x{a.res_h}, streams {a.streams}, ms per replay (three rounds, interleaved):")
    for name, v in res.items():
        print(f"  {name:20s} rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)
    p, q = (min(res[n]) for n in steps)
    print(f"solver step minus DDIM step in the captured step: {1000 * (q - p):+.1f} us ({100 * (q - p) / p:+.2f} % of the step)", flush=True)
    del ddim, ms

    if not a.no_videos:
        print("whole videos (second run of each sampler; wall time between device synchronisations):")
        for name, n, skw in (("DDIM, leading, n = 50", 50, {}), ("2M, logsnr, n = 20", 20, dict(spacing="logsnr", solver="dpmpp2m")),
                             ("2M, logsnr, n = 10", 10, dict(spacing="logsnr", solver="dpmpp2m"))):
            smp = sampler(n, **skw)
            for _run in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = smp.sample(x_T)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            print(f"  {name:22s} {n:3d} UNet calls  {dt:7.3f} s  ({1000 * dt / n:.2f} ms per call)  finite {bool(torch.isfinite(out).all())}", flush=True)
            del smp


if __name__ == "__main__":
    main()
