"""cost of the soft-mask launches (tmix_mask_edt + tmix_soft_masks: once per mask acquisition, i.e. once per image) against ONE fusion step
of the SDXL sampler at 1024^2 measured in the same process (bench.py's sampler, K = 3, one graph replay per step): the numbers of
DESIGN.md section 7g.  Two grids: the 128 x 128 latent with K = 4 (three foreground masks) and a 128 x 384 canvas grid with K = 4.  Every
candidate is one captured graph; 10 replays per round, three interleaved rounds, the minimum of the rounds (the method of section 7e), the
box's clock beside the numbers.

    python tools/soft_mask_cost.py"""
import os, socket, sys, time, numpy as np, torch
sys.path.insert(0, os.getcwd())
import bench
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
tw, parts = bench.build_sampler(args, "custom", dev, seed=0)
from tweediemix_amd import lib as L, masks as M, ops
tw.x_state.copy_(torch.randn(1, 4, tw.h, tw.w, device=dev))
t_f = bench.fusion_timesteps(tw)[0]


def fusion_step():
    tw._run_step("fusion", L.STEP_FUSION, t_f, tw.alpha(t_f), tw.alpha(t_f - tw.skip))


def soft_graph(h, w, K=4):
    fg = torch.from_numpy(np.stack([m[::8, ::8] for m in M.random_rectangle_masks(K, h * 8, w * 8, seed=4)])).float().div(255).to(dev).contiguous()
    d_set, d_clear = ops.mask_edt(fg)                           # warm-up outside capture (lazy module load)
    out = ops.soft_masks(d_set.view(1, K - 1, h, w), d_clear.view(1, K - 1, h, w), 4.0, 1.0, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_edt(fg, d_set, d_clear)
        ops.soft_masks(d_set.view(1, K - 1, h, w), d_clear.view(1, K - 1, h, w), 4.0, 1.0, True, out=out)
    return g.replay


cands = {"fusion step (SDXL, 1024^2, B = 4)": fusion_step, "edt + soft masks, 128 x 128, K = 4": soft_graph(128, 128),
         "edt + soft masks, 128 x 384 canvas grid, K = 4": soft_graph(128, 384)}
res = {k: [] for k in cands}
for rnd in range(3):
    for name, run in cands.items():
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) * 100)
try:
    clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
except Exception:
    clk = None
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
step = min(res["fusion step (SDXL, 1024^2, B = 4)"])
for name, v in res.items():
    print(f"{name}: ms per replay per round {[round(x, 4) for x in v]} min {min(v):.4f} = {min(v) / step:.4f} x one fusion step", flush=True)
