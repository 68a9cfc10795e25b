"""cost of the free-form attention masks (tmix_attn_shapes: once per seed and image) against ONE fusion step of the SDXL sampler at 1024^2
measured in the same process (bench.py's sampler, K = 3), and against the host time of today's rectangle path on the same scores: the
numbers of DESIGN.md section 7h.  Scores: a few smooth bumps per concept, min / max normalised like attention_scores' output, at the SDXL
attention grid (64 x 64, K = 3 and 4) and at the size limit (128 x 128, K = 4); and the serpentine of the tests at 128 x 128 (one component
whose labels travel the whole path: the worst case of the labelling).  Every GPU candidate is one captured graph; 10 replays per round,
three interleaved rounds, the minimum of the rounds (the method of section 7e), the box's clock beside the numbers.

    python tools/attn_shape_cost.py"""
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


def bump_scores(h, w, km1, seed=0):
    """[km1, h, w] fp64 in [0, 1]: per concept one large and two small Gaussian bumps plus a little noise, min / max normalised"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(km1):
        acc = 0.05 * rng.rand(h, w)
        for amp, rad in ((1.0, 0.22), (0.7, 0.08), (0.6, 0.06)):
            cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
            acc += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (rad * min(h, w)) ** 2))
        out.append((acc - acc.min()) / (acc.max() - acc.min()))
    return np.stack(out)


def serpentine_scores(h, w, km1):
    m = np.zeros((h, w))
    m[0::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    return np.stack([m] * km1)


def shapes_graph(score):
    s = torch.from_numpy(score.astype(np.float32)[None]).to(dev).contiguous()
    out = ops.attn_shapes(s, 0.5, True, True)                   # warm-up outside capture (lazy module load, LDS limit)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], M.attn_shapes_reference(score, 0.5, True, True))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attn_shapes(s, 0.5, True, True, out=out)
    return g.replay


def host_rect_ms(score, H, W, reps=3):
    """today's path on the host: threshold, Python flood fill, expand_masks, nearest upsampling (the score is handed in as one level's maps)"""
    toks = [[k] for k in range(score.shape[0])]
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        M.attention_masks({0: score}, toks, H, W, shape="rect")
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


scores = {"attn_shapes, 64 x 64, K = 3": bump_scores(64, 64, 2), "attn_shapes, 64 x 64, K = 4": bump_scores(64, 64, 3),
          "attn_shapes, 128 x 128, K = 4": bump_scores(128, 128, 3), "attn_shapes, serpentine 128 x 128, K = 4": serpentine_scores(128, 128, 3)}
cands = {"fusion step (SDXL, 1024^2, B = 4)": fusion_step}
cands.update({name: shapes_graph(s) for name, s in scores.items()})
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
for name, s in scores.items():
    side = s.shape[1] * 16                            # the image whose finest attention grid this is (latent / 2)
    print(f"host rectangle path on the scores of '{name}': {host_rect_ms(s, side, side):.2f} ms (attention_masks, shape='rect', best of 3)", flush=True)
