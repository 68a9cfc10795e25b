#!/usr/bin/env python3
"""cost of the hold in the captured video step (the method of tools/video_eta_cost.py).

(1) One captured step of the I2VGen-XL video sampler (synthetic FULL weights, one video, 16 frames) ending in (a) the entry the run without a hold
ends in (tmix_vpred_step_dev / tmix_vpred_step_ms_dev at eta = 0, tmix_vpred_step_noise_dev at eta = 1) and (b) tmix_vpred_step_hold_dev with the
same solver and eta: the same launch count, two more reads per element and, where the weight is not 0, one more Philox call.  The held latent is one
image for all frames (Fk = 1), the weight one map (Fw = 1): the left 40 % of the picture held, a ramp of 8 latent pixels, the rest sampled.  EIGHT
samplers over ONE plan, so all graphs replay the same launches on the same buffers and differ in their last launch only.  10 replays per round,
interleaved rounds, the minimum of the rounds, the rounds' spread and the box's clock beside the numbers.
(2) The hold entries against the noise entries alone at the I2VGen-XL state size (4 x 16 x 56 x 96 per video), S = 1 and 4, 200 calls between two
synchronisations: the dense forms (fp32), the forms on plan rows, and the composite entry.
Nothing is asserted about the times: the numbers go into DESIGN.md 7p.

    python tools/video_hold_cost.py [--res_w 768 --res_h 448] [--frames 16] [--streams 2] [--rounds 3] [--no-step]"""
import argparse
import collections
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def report(title, res, unit, scale):
    print(title)
    for name, v in res.items():
        v = [x * scale for x in v]
        print(f"  {name:34s} rounds {[round(x, 3) for x in v]} min {min(v):.3f} {unit} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)


def hold_pair(S, Fr, h, w, gen):
    """(x0 [S, 4, 1, h, w], weight [1, 1, h, w]) on the host: the left 40 % held, 8 columns of ramp, the rest sampled"""
    edge = (4 * w) // 10
    col = ((edge + 8 - torch.arange(w, dtype=torch.float32)) / 8.0).clamp(0.0, 1.0)
    return torch.randn(S, 4, 1, h, w, generator=gen), col.expand(1, 1, h, w).contiguous()


def captured_steps(a, dev):
    from tweediemix_amd import i2vgen as I, video as V
    from tweediemix_amd.weights import synthetic_i2vgen_state_dict
    cfg = I.TINY if a.tiny else I.FULL
    Fr, h, w = a.frames, a.res_h // 8, a.res_w // 8
    Wt = I.I2VWeights(cfg, synthetic_i2vgen_state_dict(cfg))
    acp, kw = V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True, steps_offset=1,
                                                  set_alpha_to_one=False))
    g = torch.Generator().manual_seed(1)
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0] * 2), torch.randn(2, 4, Fr, h, w, generator=g), torch.randn(2, cfg.cross_dim, generator=g),
                                  torch.randn(2, 77, cfg.cross_dim, generator=g))
    plan = I.I2VVideoPlan(Wt, 1, Fr, h, w, fe, ctx, ilf, streams=a.streams)
    x_T = torch.randn(1, 4, Fr, h, w, generator=g).to(dev)
    hold = hold_pair(1, Fr, h, w, g)

    def sampler(**skw):
        sch = V.VideoSchedule(acp, 50, **kw)
        return V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.02), 0.7, clips=2, frames=Fr), **skw)

    smp = {}
    for solver in V.SOLVERS:
        for eta in (0.0, 1.0):
            for held in (False, True):
                skw = dict(solver=solver)
                if eta or held:
                    skw.update(eta=eta, noise_seeds=[6425])
                if held:
                    skw.update(hold=hold)
                smp[(solver, eta, held)] = sampler(**skw)
    ts = [int(t) for t in smp[("ddim", 0.0, False)].schedule.timesteps]
    i = ts.index(501)

    def step_of(s):
        def step():
            if s.ms:
                s.phase.set_previous(ts[i - 1])           # the step before was the preceding entry: second-order coefficients
            s.step(501)
        return step
    name_of = lambda solver, eta, held: f"{solver} eta = {eta:g} {'hold' if held else 'parent'}"
    steps = {name_of(*k): step_of(s) for k, s in smp.items()}
    res = collections.defaultdict(list)
    for _rnd in range(a.rounds):
        for name, step in steps.items():
            for s in smp.values():
                s.state.copy_(x_T)
            res[name].append(timed(step, 10, 3))
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    for (solver, eta, held), s in smp.items():
        tail = (("ms",) if s.ms else ()) + (("eta",) if eta else ()) + (("hold",) if held else ())
        key = (False,) + tail if tail else False
        assert sorted(s.graphs) == [key], (solver, eta, held, sorted(s.graphs))
    print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
    report(f"video step, one video, {Fr} frames {a.res_w}x{a.res_h}, streams {a.streams}, ms per replay ({a.rounds} rounds, interleaved):", res, "ms", 1e3)
    for solver in V.SOLVERS:
        for eta in (0.0, 1.0):
            p, q = min(res[name_of(solver, eta, False)]), min(res[name_of(solver, eta, True)])
            print(f"{solver} eta = {eta:g}: hold step minus parent step in the captured step: {1e6 * (q - p):+.1f} us ({100 * (q - p) / p:+.3f} % of the step)",
                  flush=True)


def entries_alone(a, dev):
    from tweediemix_amd import ops
    C, Fr, h, w = 4, 16, 56, 96
    move = {"ddim": (0.8, 0.45), "dpmpp2m": (0.81, 0.4, -0.08)}
    for S in (1, 4):
        g = torch.Generator(device=dev).manual_seed(S)
        x, v = torch.randn(S, C, Fr, h, w, device=dev, generator=g), torch.randn(2 * S, C, Fr, h, w, device=dev, generator=g)
        eu, ec = torch.randn(S * Fr, C, h, w, device=dev, generator=g), torch.randn(S * Fr, C, h, w, device=dev, generator=g)
        hist, out, keys = torch.zeros_like(x), torch.empty_like(x), ops.noise_keys(range(6425, 6425 + S), dev)
        kx, wt = (t.to(dev) for t in hold_pair(S, Fr, h, w, torch.Generator().manual_seed(S)))
        p12 = {k: ops.video_step_params_noise(501, 9.0, 0.3, m, 0.3, 24).to(dev) for k, m in move.items()}
        ph = {k: ops.video_step_params_hold(501, 9.0, 0.3, m, 0.3, 24, 0.35).to(dev) for k, m in move.items()}
        calls = {
            "dense ddim    noise": lambda: ops.vpred_step_noise(x, v, 9.0, 0.3, move["ddim"], 0.3, keys, 24, out=out),
            "dense ddim    hold": lambda: ops.vpred_step_hold(x, v, 9.0, 0.3, move["ddim"], 0.3, keys, 24, 0.35, kx, wt, out=out),
            "dense dpmpp2m noise": lambda: ops.vpred_step_noise(x, v, 9.0, 0.3, move["dpmpp2m"], 0.3, keys, 24, x0_prev=hist, out=out),
            "dense dpmpp2m hold": lambda: ops.vpred_step_hold(x, v, 9.0, 0.3, move["dpmpp2m"], 0.3, keys, 24, 0.35, kx, wt, x0_prev=hist, out=out),
            "rows  ddim    noise": lambda: ops.vpred_step_noise_dev(x, eu, ec, p12["ddim"], keys),
            "rows  ddim    hold": lambda: ops.vpred_step_hold_dev(x, eu, ec, ph["ddim"], keys, kx, wt),
            "rows  dpmpp2m noise": lambda: ops.vpred_step_noise_dev(x, eu, ec, p12["dpmpp2m"], keys, x0_prev=hist),
            "rows  dpmpp2m hold": lambda: ops.vpred_step_hold_dev(x, eu, ec, ph["dpmpp2m"], keys, kx, wt, x0_prev=hist),
            "composite": lambda: ops.video_hold_composite(out, 0.35, keys, kx, wt),
        }
        res = collections.defaultdict(list)
        for _rnd in range(a.rounds):
            for name, fn in calls.items():
                res[name].append(timed(fn, 200, 20))
        n = x.numel()
        report(f"the entries alone, S = {S} ({n} elements, {n * 4 / 1e6:.2f} MB of state), us per call (200 calls between synchronisations):", res, "us", 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res_w", type=int, default=768)
    ap.add_argument("--res_h", type=int, default=448)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2, choices=[1, 2])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tiny network (a dry run of the tool)")
    ap.add_argument("--no-step", action="store_true", help="part (2) alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if not a.no_step:
        captured_steps(a, dev)
    entries_alone(a, dev)


if __name__ == "__main__":
    main()
