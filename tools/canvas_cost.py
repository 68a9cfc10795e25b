"""cost of the window consensus launch in the whole step: graph replays of the fusion step at SDXL 1024^2 windows with three
co-batched row sets (B = 12), (a) as three independent seeds -- no consensus launch -- and (b) as the three windows of one 2048 x 1024 canvas
(overlap 512), whose captured step ends with tmix_window_consensus; same weights, same masks, one process.  Three interleaved rounds of 10 replays,
the minimum of the rounds (the method of section 7e), the box's clock beside the numbers.

    python tools/canvas_cost.py [custom|lora]"""
import collections, os, socket, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, sampler as S

kind = sys.argv[1] if len(sys.argv) > 1 else "custom"
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num
res_px = base.h * 8


def sampler(**kw):
    tw = S.Tweediemix(base.config, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, **kw)
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
    tw.masks = base.masks[None].expand(3, *base.masks.shape).contiguous()          # one mask set per row set, in both variants
    tw.plan("fusion")
    return tw


variants = {"a: three seeds, no consensus": sampler(n_seeds=3),
            "b: three windows of one canvas": sampler(n_seeds=1, canvas=dict(height=res_px, width=2 * res_px, overlap=res_px // 2))}
assert variants["b: three windows of one canvas"].n_seeds == 3
x0 = torch.randn(3, 4, base.h, base.w, device=dev)
res = collections.defaultdict(list)
for rnd in range(3):
    for name, tw in variants.items():
        step = lambda: tw._run_step("fusion", L.STEP_FUSION, 501, tw.alpha(501), tw.alpha(351))
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
print(f"fusion step, {kind}, B = {variants['a: three seeds, no consensus'].plan('fusion').B}, ms per replay (three rounds, interleaved):")
for name, v in res.items():
    print(f"  {name:32s} rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)
a, b = (min(res[n]) for n in variants)
print(f"consensus launch in the captured step: {1000 * (b - a):+.1f} us ({100 * (b - a) / a:+.2f} % of the step)")
