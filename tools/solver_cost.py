"""cost of the multistep step entry in the whole step, and whole-image times of few-step sampling.

(1) One captured fusion step of the SDXL sampler at 1024^2 (B = 4) whose fused step is (a) tmix_fused_tweedie_step_dev -- the DDIM step -- and (b)
tmix_fused_tweedie_step_ms_dev with second-order coefficients -- one more 256 KB read and write per seed; ONE sampler, so both graphs replay the same
plan on the same buffers and differ in their last launch only.
10 replays per round, three interleaved rounds, the minimum of the rounds (the method of section 7e), the box's clock beside the numbers.
(2) Whole images, wall time between device synchronisations, graphs on, the second run of each sampler (the first captures): DDIM 'leading' at n = 50,
the solver on the log-SNR grid at n = 20 and n = 10, each beside its counted UNet calls.  No quality claim is attached to these.

    python tools/solver_cost.py [custom|lora] [--no-images]"""
import collections, os, socket, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, sampler as S
from tweediemix_amd.solver import multistep_coeffs

kind = next((a for a in sys.argv[1:] if a in ("custom", "lora")), "custom")
images = "--no-images" not in sys.argv
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num


def sampler(config=None, **kw):
    return S.Tweediemix(config or base.config, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, **kw)


tw = sampler(solver="dpmpp2m")
tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
tw.masks = base.masks
at_prev, at, at_next = (base.alpha(t) for t in (521, 501, 481))
ms = multistep_coeffs(at_prev, at, at_next, True)
assert ms[2] != 0.0
steps = {"a: DDIM step": lambda: tw._run_step("fusion", L.STEP_FUSION, 501, at, at_next),
         "b: 2M solver step": lambda: tw._run_step("fusion", L.STEP_FUSION, 501, at, at_next, ms=ms)}
x0 = torch.randn(1, 4, base.h, base.w, device=dev)
res = collections.defaultdict(list)
for rnd in range(3):
    for name, step in steps.items():
        tw.x_state.copy_(x0)
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
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
print(f"fusion step, {kind}, B = {tw.plan('fusion').B}, ms per replay (three rounds, interleaved):")
for name, v in res.items():
    print(f"  {name:20s} rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)
a, b = (min(res[n]) for n in steps)
print(f"solver step minus DDIM step in the captured step: {1000 * (b - a):+.1f} us ({100 * (b - a) / a:+.2f} % of the step)", flush=True)
assert sorted(tw.graphs, key=len) == [("fusion", L.STEP_FUSION), ("fusion", L.STEP_FUSION, "ms")]
del tw

if images:
    x_T = torch.randn(1, 4, base.h, base.w, generator=torch.Generator().manual_seed(7))
    print("whole images (second run of each sampler; wall time between device synchronisations):")
    for name, n, kw in (("DDIM, leading, n = 50", 50, {}), ("2M, logsnr, n = 20", 20, dict(solver="dpmpp2m", timestep_spacing="logsnr")),
                        ("2M, logsnr, n = 10", 10, dict(solver="dpmpp2m", timestep_spacing="logsnr"))):
        conf = S.make_config(**{**vars(base.config), "n_timesteps": n})
        tw = sampler(conf, **kw)
        for run in range(2):
            del tw.unet_calls[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tw.run_fusion(x_T.clone())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        print(f"  {name:22s} {len(tw.unet_calls):3d} UNet calls  {dt:7.3f} s  ({1000 * dt / len(tw.unet_calls):.2f} ms per call)", flush=True)
        del tw
