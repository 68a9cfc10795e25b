#!/usr/bin/env python3
"""cost of the unguided video step against the guided one (the method of tools/video_hold_cost.py).

(1) The captured step of the I2VGen-XL video sampler (synthetic FULL weights, 16 frames, 768 x 448) in its guided form -- prologue, the CFG pair's
2S clips, tmix_vpred_step_dev -- and in its unguided form -- tmix_video_step_prologue_cond, the S text clips alone on one stream,
tmix_vpred_step_cond_dev -- as two samplers over ONE plan, at S = 1 and S = 4 videos, for --streams 2 (the unguided step replays the text half's
own chain) and --streams 1 (it replays an S-clip chain built on first use; its extra memory is reported).  10 replays per round, interleaved
rounds, the minimum of the rounds, the rounds' spread and the box's clock beside the numbers.  The yardstick is the guided step of the same call;
the ideal ratio is the row share, 0.5.
(2) The three new launches against their guided parents alone at the I2VGen-XL state size (4 x 16 x 56 x 96 per video), S = 1 and 4, 200 calls
between two synchronisations.
(3) From (1): clips and time per video for the interval (700, 250) at n = 50 'leading' and the clip count at n = 20 'logsnr', counted with the
sampler's own test (guidance.is_guided over the schedule's timesteps).
Nothing is asserted about the times: the numbers go into DESIGN.md 7r and, with --out, into a JSON file.

    python tools/video_interval_cost.py [--videos 1,4] [--streams 2,1] [--rounds 3] [--no-step] [--out profiles/video_interval_cost.json]"""
import argparse
import collections
import json
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INTERVAL = (700, 250)


def timed(fn, calls, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def sclk(dev):
    try:
        return torch.cuda.clock_rate(dev)
    except Exception:
        return None


def table():
    from tweediemix_amd import video as V
    return V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True, steps_offset=1, set_alpha_to_one=False))


def captured_steps(a, dev, Wt, S, streams):
    """-> the record of one (S, streams) cell"""
    from tweediemix_amd import i2vgen as I, video as V
    cfg = Wt.cfg
    Fr, h, w = a.frames, a.res_h // 8, a.res_w // 8
    acp, kw = table()
    g = torch.Generator().manual_seed(S)
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0] * 2 * S), torch.randn(2 * S, 4, Fr, h, w, generator=g), torch.randn(2 * S, cfg.cross_dim, generator=g),
                                  torch.randn(2 * S, 77, cfg.cross_dim, generator=g))
    print(f"S = {S}, streams {streams}: building the plan ...", flush=True)
    plan = I.I2VVideoPlan(Wt, S, Fr, h, w, fe, ctx, ilf, streams=streams)
    x_T = torch.randn(S, 4, Fr, h, w, generator=g).to(dev)

    def sampler(**skw):
        sch = V.VideoSchedule(acp, 50, **kw)
        return V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.02), 0.7, clips=2 * S, frames=Fr), **skw)
    smp = {"guided": sampler(), "unguided": sampler(guidance_interval=(0, 0))}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    plan.cond_plan                                       # streams=1: the S-clip chain is built here, outside the timed rounds
    torch.cuda.synchronize()
    extra = torch.cuda.memory_allocated(dev) - before
    res = collections.defaultdict(list)
    for _rnd in range(a.rounds):
        for name, s in smp.items():
            for o in smp.values():
                o.state.copy_(x_T)
            res[name].append(timed(lambda: s.step(501), 10, 3))
            print(f"  {name:9s} {1e3 * res[name][-1]:.3f} ms", flush=True)
    clk = sclk(dev)                                      # sampled right behind the last timed replays
    assert sorted(smp["guided"].graphs) == [False] and sorted(smp["unguided"].graphs) == [(False, "cond")]
    gd, un = min(res["guided"]), min(res["unguided"])
    rec = dict(videos=S, streams=streams, guided_ms=round(1e3 * gd, 3), unguided_ms=round(1e3 * un, 3), ratio=round(un / gd, 4),
               guided_rounds_ms=[round(1e3 * v, 3) for v in res["guided"]], unguided_rounds_ms=[round(1e3 * v, 3) for v in res["unguided"]],
               guided_spread_pct=round(spread(res["guided"]), 2), unguided_spread_pct=round(spread(res["unguided"]), 2), sclk_mhz=clk,
               launches_guided=len(plan.ops) + 2, launches_unguided=len(plan.cond_plan.ops) + 2, cond_chain_extra_mb=round(extra / 2 ** 20, 1))
    print(f"S = {S}, streams {streams}: guided {rec['guided_ms']} ms, unguided {rec['unguided_ms']} ms, ratio {rec['ratio']} (row share 0.5), "
          f"sclk {clk} MHz, the text chain's own buffers {rec['cond_chain_extra_mb']} MB", flush=True)
    return rec


def entries_alone(a, dev):
    from tweediemix_amd import ops
    C, Fr, h, w, R = 4, 16, 56, 96, 8
    move = {"ddim": (0.8, 0.45), "dpmpp2m": (0.81, 0.4, -0.08)}
    out = {}
    for S in (1, 4):
        g = torch.Generator(device=dev).manual_seed(S)
        x = torch.randn(S, C, Fr, h, w, device=dev, generator=g)
        eu, ec = torch.randn(S * Fr, C, h, w, device=dev, generator=g), torch.randn(S * Fr, C, h, w, device=dev, generator=g)
        xu, xc = torch.zeros(S * Fr, R, h, w, device=dev), torch.zeros(S * Fr, R, h, w, device=dev)
        tu, tc = torch.zeros(S, device=dev), torch.zeros(S, device=dev)
        hist, keys = torch.zeros_like(x), ops.noise_keys(range(6425, 6425 + S), dev)
        p8 = {"ddim": ops.video_step_params(501, 9.0, 0.3, 0.35).to(dev), "dpmpp2m": ops.video_step_params_ms(501, 9.0, 0.3, move["dpmpp2m"]).to(dev)}
        p12 = {k: ops.video_step_params_noise(501, 9.0, 0.3, m, 0.3, 24).to(dev) for k, m in move.items()}
        calls = {
            "prologue            ": lambda: ops.video_step_prologue(x, xu, tu, xc, tc, p8["ddim"]),
            "prologue_cond       ": lambda: ops.video_step_prologue_cond(x, xc, tc, p8["ddim"]),
            "rows ddim    guided ": lambda: ops.vpred_step_dev(x, eu, ec, p8["ddim"]),
            "rows ddim    cond   ": lambda: ops.vpred_step_cond_dev(x, ec, p8["ddim"]),
            "rows dpmpp2m guided ": lambda: ops.vpred_step_ms_dev(x, eu, ec, hist, p8["dpmpp2m"]),
            "rows dpmpp2m cond   ": lambda: ops.vpred_step_cond_dev(x, ec, p8["dpmpp2m"], hist),
            "rows ddim    noise  ": lambda: ops.vpred_step_noise_dev(x, eu, ec, p12["ddim"], keys),
            "rows ddim    noise c": lambda: ops.vpred_step_cond_dev(x, ec, p12["ddim"], None, keys),
        }
        res = collections.defaultdict(list)
        for _rnd in range(a.rounds):
            for name, fn in calls.items():
                res[name].append(timed(fn, 200, 20))
        n = x.numel()
        print(f"the launches alone, S = {S} ({n} elements, {n * 4 / 1e6:.2f} MB of state), us per call (200 calls between synchronisations):")
        for name, v in res.items():
            v = [1e6 * t for t in v]
            print(f"  {name} rounds {[round(t, 2) for t in v]} min {min(v):.2f} us spread {spread(v):.1f} %", flush=True)
        out[f"S{S}"] = {name.strip(): round(1e6 * min(v), 2) for name, v in res.items()}
    return out


def accounting(steps):
    """clips per video under INTERVAL, and the whole-video time at n = 50 as the measured step times multiplied by the counts"""
    from tweediemix_amd import video as V
    from tweediemix_amd.guidance import unguided_count
    acp, kw = table()
    out = {}
    for n, spacing in ((50, "leading"), (20, "logsnr")):
        ts = V.VideoSchedule(acp, n, **kw, spacing=spacing).timesteps
        nu = unguided_count(INTERVAL, ts)
        out[f"n{n}_{spacing}"] = dict(steps=n, unguided=nu, guided=n - nu, clips=2 * n - nu, clips_without=2 * n)
    c = out["n50_leading"]
    for r in steps:
        r["video_n50_ms"] = round(c["guided"] * r["guided_ms"] + c["unguided"] * r["unguided_ms"], 1)
        r["video_n50_without_ms"] = round(50 * r["guided_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res_w", type=int, default=768)
    ap.add_argument("--res_h", type=int, default=448)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--videos", default="1,4")
    ap.add_argument("--streams", default="2,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tiny network (a dry run of the tool)")
    ap.add_argument("--no-step", action="store_true", help="part (2) alone")
    ap.add_argument("--out", default="", help="write the record as JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rec = dict(tool="tools/video_interval_cost.py", box=socket.gethostname(), device=torch.cuda.get_device_name(dev), frames=a.frames,
               resolution=[a.res_w, a.res_h], interval=list(INTERVAL), rounds=a.rounds, replays_per_round=10, steps=[])
    if not a.no_step:
        from tweediemix_amd import i2vgen as I
        from tweediemix_amd.weights import synthetic_i2vgen_state_dict
        cfg = I.TINY if a.tiny else I.FULL
        Wt = I.I2VWeights(cfg, synthetic_i2vgen_state_dict(cfg))
        for S in (int(s) for s in a.videos.split(",")):
            for streams in (int(s) for s in a.streams.split(",")):
                rec["steps"].append(captured_steps(a, dev, Wt, S, streams))
                torch.cuda.empty_cache()
    rec["launches_alone_us"] = entries_alone(a, dev)
    rec["clips"] = accounting(rec["steps"])
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
