#!/usr/bin/env python3
"""cost of the guidance rescale in the captured video step (the method of tools/video_solver_cost.py and tools/rescale_cost.py).

(1) One captured step of the I2VGen-XL video sampler (synthetic FULL weights, one video, 16 frames) ending in (a) the parent entry
(tmix_vpred_step_dev, or tmix_vpred_step_ms_dev with --solver dpmpp2m) and (b) tmix_vpred_rescale_factors + the _rs_dev entry: two small launches and
one more read of both halves' predictions.  TWO samplers over ONE plan, so both graphs replay the same launches on the same buffers and differ in
their tail only.  10 replays per round, interleaved rounds, the minimum of the rounds, the rounds' spread and the box's clock beside the numbers.
(2) The launch pair alone on the plan's prediction rows, 200 calls between two synchronisations.
Nothing is asserted about the times: the numbers go into DESIGN.md 7m.

    python tools/video_rescale_cost.py [--res_w 768 --res_h 448] [--frames 16] [--streams 2] [--solver ddim|dpmpp2m] [--phi 0.7] [--rounds 3]"""
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
    ap.add_argument("--solver", default="ddim", choices=["ddim", "dpmpp2m"])
    ap.add_argument("--phi", type=float, default=0.7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tiny network (a dry run of the tool)")
    a = ap.parse_args()
    from tweediemix_amd import i2vgen as I, ops, video as V
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

    def sampler(**skw):
        sch = V.VideoSchedule(acp, 50, **kw)
        return V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.02), 0.7, clips=2, frames=Fr), solver=a.solver, **skw)

    plain, rs = sampler(), sampler(guidance_rescale=a.phi)
    ts = [int(t) for t in plain.schedule.timesteps]
    i = ts.index(501)

    def step_of(s):
        def step():
            if s.ms:
                s.phase.set_previous(ts[i - 1])           # the step before was the preceding entry: second-order coefficients
            s.step(501)
        return step
    steps = {"a: parent entry": step_of(plain), "b: factors + rs entry": step_of(rs)}
    res = collections.defaultdict(list)
    for _rnd in range(a.rounds):
        for name, step in steps.items():
            for s in (plain, rs):
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
    key = (False, "ms") if plain.ms else False
    assert sorted(plain.graphs) == [key] and sorted(rs.graphs) == [(key if plain.ms else (False,)) + ("rs",)]
    print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
    print(f"video step, one video, {Fr} frames {a.res_w}x{a.res_h}, streams {a.streams}, solver {a.solver}, phi {a.phi}, factor {float(rs.rs_factors[0]):.6f}, "
          f"ms per replay ({a.rounds} rounds, interleaved):")
    for name, v in res.items():
        print(f"  {name:24s} rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)
    p, q = (min(res[n]) for n in steps)
    print(f"rescaled step minus parent step in the captured step: {1000 * (q - p):+.1f} us ({100 * (q - p) / p:+.2f} % of the step)", flush=True)

    (_xu, _tu, eu), (_xc, _tc, ec) = plan.halves
    n = rs.state[0].numel()
    pair = lambda: ops.vpred_rescale_factors_dev(eu, ec, 1, n, rs.params, 6 if rs.ms else 5, a.phi, out=rs.rs_factors, ws=rs._rs_ws)
    alone = []
    for _rnd in range(a.rounds):
        for _ in range(20):
            pair()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            pair()
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - t0) * 1e6 / 200)
    print(f"the factors launch pair alone ({n} elements per half, {2 * n * 4 / 1e6:.2f} MB read): us per call {[round(x, 2) for x in alone]} min {min(alone):.2f}", flush=True)


if __name__ == "__main__":
    main()
