"""cost of one propagate round (attention_masks propagate >= 1: the "propagate" plan, the plain B = 2 call plus one
tmix_sattn_propagate launch behind every attn1 of the probed levels) against the plain call it replays: one whole step per graph
replay (prologue + UNet + fused update), SDXL shapes at 1024^2, two foreground tokens, 10 replays each, three interleaved rounds, the
box's clock beside the numbers.  Then the launch alone at the two levels' shapes (B = 2, row 1; events around 20 back-to-back launches
on q / k of the level's width, three rounds): the per-level launch times of DESIGN.md section 7b.

    python tools/propagate_cost.py"""
import os, socket, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
tw, parts = bench.build_sampler(args, "custom", dev, seed=0)
tw.attention_masks = dict(tokens=[[4], [7]], flat=[4, 7], threshold=0.5, levels=None, level_weights=None, propagate=1)
from tweediemix_amd import lib as L, ops, unet as U
tw.x_state.copy_(torch.randn(1, 4, tw.h, tw.w, device=dev))
for src in tw.plan("propagate").prop_src.values():
    src.copy_(torch.rand(src.shape, device=dev))
res = {"plain": [], "propagate": []}
for rnd in range(3):
    for kind in res:
        step = lambda: tw._run_step(kind, L.STEP_PLAIN, 501, tw.alpha(501), tw.alpha(351))
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        res[kind].append((time.perf_counter() - t0) * 100)
try:
    clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
except Exception:
    clk = None
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
names = {k: [getattr(fn, "__name__", "") for fn, _a in tw.plan(k).ops] for k in res}
for k, v in res.items():
    print(f"{k}: B={tw.plan(k).B} launches={len(names[k])} (tmix_sattn_propagate: {names[k].count('tmix_sattn_propagate')}) "
          f"ms/call per round {[round(x, 3) for x in v]} min {min(v):.3f}", flush=True)
lo_p, lo_q = min(res["plain"]), min(res["propagate"])
print(f"propagate - plain: {lo_q - lo_p:.3f} ms per round ({lo_q / lo_p:.2f} x the plain call)", flush=True)

plan = tw.plan("propagate")
cfg = plan.cfg
for lvl, sites in sorted(plan._prop_sites.items()):
    S, C = (tw.h >> lvl) * (tw.w >> lvl), cfg.block_out_channels[lvl]
    H = C // cfg.head_dim
    qk = (torch.randn(2, S, 2 * C, device=dev) * 2).to(torch.bfloat16)
    src, out = torch.rand(1, 2, S, device=dev), torch.zeros(1, 2, S, device=dev)
    run = lambda: ops.sattn_propagate(qk[:, :, :C], qk[:, :, C:], src, H, rows=(1, 2, 1), out=out, accumulate=True, out_scale=1.0 / (H * sites))
    us = []
    for rnd in range(3):
        run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000 / 20)
    flop = 2 * 2 * S * S * 64 * H                         # both products as if the second one were head_dim wide (attention-shaped)
    print(f"level {lvl}: S={S} H={H} n_tok=2, {sites} launches per call: {min(us):.1f} us per launch (rounds {[round(u, 1) for u in us]}), "
          f"{sites * min(us) / 1000:.3f} ms per call, {flop / min(us) * 1e-6:.1f} TFLOP/s attention-shaped", flush=True)
