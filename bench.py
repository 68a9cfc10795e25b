#!/usr/bin/env python3
"""bench.py -- denoise steps/sec of the Tweedie-mix fusion phase on MI355X (+ images/sec of whole trajectories).

A "step" = one fusion-phase iteration of `sample_loop` (fusion_sampling.py:493-494 with t <= t_cond_cur): ONE SDXL UNet
forward at batch K+1 (uncond + K concept rows, per-concept weights routed) + the fused CFG/Tweedie/blend/DDIM kernel,
replayed as one hipGraph with the latent resident in HBM.
Workload: SDXL-base shapes, 1024x1024 (latent 128x128), K=3 concepts (2 foreground + background), synthetic random-init
weights / prompt embeddings / rectangle masks (no checkpoints exist offline).  `--kind lora` (default, BASELINE.json
configs[2], the north-star headline: merged per-row LoRA weights, --t_stop 0.8) or `--kind custom` (configs[1]); with the
default `--kind both` the line's `value` is the LoRA figure and `other_configs.custom` carries configs[1].

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
N > 1 without a launcher: the script starts its own N ranks (tweediemix_amd/launch.py; one process per GPU, RCCL); under
`python -m torch.distributed.run` it uses the ranks it is given.  Rank 0 prints ONE JSON line with the contract fields.
A plain run builds the plan, replays the headline step untimed for a few seconds (the chip settles), runs W warm-up and
K timed steps and prints the line: nothing else.
`--full` adds every other measurement and check: `roofline` (timed IN SITU: every GEMM / conv / attention / GroupNorm
launch of the captured step records its own start / end on the device clock while the graph replays), `images_per_s`
(whole 50-step trajectories incl. the VAE decode, all ranks), `parity_check`, the other configs (Custom-Diffusion, fp8,
video) and, at N = 1, `cpu_baseline`; its `value` is the same W + K steps timed again at the end of that run.
`--dump-outputs DIR` writes what the last timed step left on rank 0 (latent.npy, x0.npy, eps.npy; float32).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BF16_DENSE_PEAK_TFLOPS = 2500.0      # MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16 MFMA
METRIC = "denoise steps/sec @ SDXL 1024^2 K=3 concepts (fusion phase); images/sec at 1/2/4/8 GPUs"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: one trajectory's worth of steps behind ten warm-up steps.  ms_per_step falls with the length of the run on these boxes (same box, same
    # library: 33.5 ms at 20 steps / 3 warm-up, 33.1 at 40 / 3, 32.7 at 50 / 10, 32.3 at 100 / 10 -- the clocks are still ramping through the first ~2 s of
    # load; tools/jobs/r3zzx_steps.sh), and a denoising trajectory is 50 steps (75 UNet calls, ~2 s) long
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kind", default="both", choices=["both", "lora", "custom"])
    ap.add_argument("--lora-mode", dest="lora_mode", default="merged", choices=["merged", "lowrank"],
                    help="lowrank: up(down(x)) as the routed projections' last K-tile (tmix_lora_down + shared weights) instead of merged per-concept weight sets")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: the FF / attn1-QKV projections run on e4m3 operands (tmix_gemm_fp8); a separate line, never the headline")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tiny", action="store_true", help="tiny UNet (debug only; not a valid bench line)")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--no-trajectory", action="store_true", help="skip the whole-trajectory / images-per-second part")
    ap.add_argument("--streams", type=int, default=1,
                    help="independent launch chains per UNet call (rows split over HIP streams); 1 = one dependent chain at the full batch, "
                         "which the LDS-staged epilogues made as fast as two half-batch chains (same-box A/B: 37.8 vs 37.6 ms)")
    ap.add_argument("--seeds-per-gpu", type=int, default=1,
                    help="independent trajectories co-batched into every UNet launch (1 = the reference's one image per process)")
    ap.add_argument("--num-seeds", type=int, default=0,
                    help="BASELINE config 4: this many seeds in total, sharded round-robin over the ranks (0: seeds-per-gpu per rank)")
    ap.add_argument("--traj-cobatch", type=int, default=8, help="independent seeds sharing every UNet launch in the images/s measurement (8 = one GPU's share of BASELINE "
                                                                "config 4: 64 seeds over 8 GPUs; 0.626 vs 0.613 images/s with 4, same box)")
    ap.add_argument("--traj-images", type=int, default=8, help="images per rank in the images/s measurement (ignored with --num-seeds)")
    ap.add_argument("--masks", default="partition", choices=["partition", "overlap"],
                    help="synthetic stand-in for the segmentation side-car: 'partition' = rectangles that do not intersect (blend weights sum to 1: the latent keeps its "
                         "scale through the fusion window); 'overlap' = rounds 1-5's intersecting rectangles (the reference does not normalise, fusion_sampling.py:466-469: "
                         "weights sum to 2 on the overlap and that region doubles every fusion step).  The line times BOTH; `value` is this one")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-video", action="store_true", help="skip other_configs.video (BASELINE configs[4], one I2VGen-XL step)")
    ap.add_argument("--cpu-threads", type=int, default=64)
    ap.add_argument("--host-dry-run", action="store_true",
                    help="launcher / collective control flow only, on CPU over gloo with a stand-in step (tests; NOT a bench line)")
    ap.add_argument("--full", action="store_true",
                    help="also run every other measurement and check (parity, in-situ roofline, trajectories, other configs, CPU baseline)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed as DIR/<name>.npy (float32)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------ sampler construction
def build_sampler(args, kind, device, seed, fp8=None):
    from tweediemix_amd import masks as M, sampler as S, unet as U, weights as Wt
    cfg = U.TINY if args.tiny else U.SDXL
    K = 3
    sd = Wt.synthetic_state_dict(cfg, seed=1234, device=device, dtype=torch.bfloat16)
    con = Wt.synthetic_concepts(cfg, kind, K, device=device)
    W = U.UNetWeights(cfg, sd, device, (kind, con), lora_mode=getattr(args, "lora_mode", "merged"))
    g = torch.Generator(device="cpu").manual_seed(42)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g), torch.randn(K, cfg.pooled_dim, generator=g))
    h = w = args.res // 8
    S_ = args.seeds_per_gpu
    conf = S.make_config(guidance_scale=0.8, n_timesteps=50, t_cond=0.2, t_stop=0.8, resampling_steps=10,
                         jumping_steps=5, resolution_h=args.res, resolution_w=args.res, seed=seed)

    def mask_set(i, mask_kind=None):
        return M.build_masks(M.synthetic_masks(mask_kind or getattr(args, "masks", "partition"), K, args.res, args.res, seed=1000 * seed + i), h, w, device)

    turn = [0]

    def provider(x0):                       # the sampler asks once per seed, in seed order
        turn[0] += 1
        return mask_set((turn[0] - 1) % S_)

    tw = S.Tweediemix(conf, W, te, ts, provider, concept_num=K, lora=(kind == "lora"), use_graphs=not args.no_graphs,
                      n_seeds=S_, n_streams=args.streams, fp8=(getattr(args, "dtype", "bf16") == "fp8") if fp8 is None else fp8)
    tw.min_rows_per_stream = int(os.environ.get("TMIX_MIN_ROWS_PER_STREAM", str(tw.min_rows_per_stream)))
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
    tw.mask_sets = lambda mask_kind=None: mask_set(0, mask_kind) if S_ == 1 else torch.stack([mask_set(i, mask_kind) for i in range(S_)]).contiguous()
    tw.masks = tw.mask_sets()
    return tw, (sd, con, te, ts, cfg)


def fusion_timesteps(tw):
    return [t for t in tw.scheduler.timesteps if t <= tw.t_cond_cur and t in tw._window]


SETTLE_S = 5.0      # untimed load ahead of a plain run's window: the chip holds its sustained clock after ~3 s of it


def timed_fusion_steps(tw, args, world, device, x, settle_s=0.0):
    """[settle_s seconds of untimed steps +] W warm-up + K timed fusion steps (barrier + synchronize on both sides).  Returns (seconds, {name: tensor}):
    copies of what the last step left -- the next latent, its Tweedie estimate x0 and the UNet output eps it was built from.
    The steps walk the fusion window's timesteps in order; when the walk wraps around to the window's first timestep the latent is re-seeded from `x`
    (one 4*h*w-float device copy per pass through the window), so every step sees a latent of the scale its timestep has in a trajectory."""
    from tweediemix_amd import lib as L
    ts = fusion_timesteps(tw)
    tw.x_state.copy_(x)

    def step(i):
        if i % len(ts) == 0:
            tw.x_state.copy_(x)
        t = ts[i % len(ts)]
        tw._run_step("fusion", L.STEP_FUSION, t, tw.alpha(t), tw.alpha(t - tw.skip))

    t_end, i = time.perf_counter() + settle_s, 0
    while time.perf_counter() < t_end:          # step(0) below re-seeds the latent: the settling steps leave no trace in the outputs
        step(i)
        i += 1
    for i in range(max(args.warmup, 2)):        # the first call builds the plan, the second captures the graph
        step(i)
    torch.cuda.synchronize()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(tw.x_state).all()
    tw.last_window_max_abs_latent = float(tw.x_state.abs().max())
    return dt, {"latent": tw.x_state.clone(), "x0": tw.x0_state.clone(), "eps": tw.plan("fusion").eps.clone()}


DUMP_CAP_BYTES = 60 << 20          # under 64 MB in decimal units too, .npy headers included


def dump_outputs(outputs, out_dir):
    """--dump-outputs: every array as out_dir/<name>.npy in float32.  Should they exceed DUMP_CAP_BYTES together, each is replaced by
    the same fixed, seeded sample of its flattened elements (a share of it in proportion to the cap), so two runs stay comparable."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: v.detach().float().cpu().numpy() for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_CAP_BYTES:
            idx = np.random.RandomState(0).choice(a.size, int(a.size * DUMP_CAP_BYTES / total), replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def chip_state_under_load(tw, device, x, n_steps=40, samples=4):
    """shader clock / socket power / temperature while the SAME captured step replays (untimed, behind the value window): boxes of the pool differ by up to 8 %
    with identical code, every kernel class moving together -- this says what state the chip held.  None where the SMI library is missing."""
    from tweediemix_amd import lib as L
    ts = fusion_timesteps(tw)
    tw.x_state.copy_(x)
    try:
        for i in range(n_steps):
            t = ts[i % len(ts)]
            tw._run_step("fusion", L.STEP_FUSION, t, tw.alpha(t), tw.alpha(t - tw.skip))
        clk, pw, tc = [], [], []
        for _ in range(samples):
            time.sleep(0.15)
            clk.append(int(torch.cuda.clock_rate(device))); pw.append(int(torch.cuda.power_draw(device))); tc.append(int(torch.cuda.temperature(device)))
        torch.cuda.synchronize()
        return {"sclk_mhz": clk, "power_raw": pw, "temp_c": tc, "what": f"torch.cuda.clock_rate / power_draw (the unit is the SMI library's: W on this image) / temperature, sampled 150 ms apart while {n_steps} more replays of the timed step were in flight (outside every timed window)"}
    except Exception as e:      # noqa: BLE001 -- a diagnostic, never fatal
        torch.cuda.synchronize()
        return {"error": repr(e)[:200]}


def parity_check(tw, args, parts, kind, device):
    """the timed path (hipGraph replay, two launch chains, shipped tile table) against an eager single-chain run of the SAME
    step from the same latent: rel-L2 of the updated latent (the tilings differ, so LayerNorm partial sums are added in a
    different order: equal to bf16 rounding, not bit for bit)."""
    from tweediemix_amd import lib as L, sampler as S
    t = fusion_timesteps(tw)[3]
    g = torch.Generator().manual_seed(99)
    x = torch.randn(tw.n_seeds, 4, tw.h, tw.w, generator=g).to(device)
    tw.x_state.copy_(x)
    tw._run_step("fusion", L.STEP_FUSION, t, tw.alpha(t), tw.alpha(t - tw.skip))
    got = tw.x_state.clone()
    got_eps = tw.plan("fusion").eps.clone()
    ref = S.Tweediemix(tw.config, tw.W, tw.text_embeds, tw.text_embeds_single, tw.mask_provider, concept_num=tw.concept_num,
                       lora=tw.lora, use_graphs=False, n_seeds=tw.n_seeds, n_streams=1)
    ref.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else ref.init_fusion(int(50 * 0.2))
    ref.masks = tw.masks
    ref.x_state.copy_(x)
    ref._run_step("fusion", L.STEP_FUSION, t, ref.alpha(t), ref.alpha(t - ref.skip))
    want = ref.x_state
    rel = float((got - want).norm() / want.norm())
    want_eps = ref.plan("fusion").eps
    rel_eps = float((got_eps - want_eps).norm() / want_eps.norm())
    del ref
    tol = 1e-1 if tw.fp8 else 2e-2
    assert rel < tol and rel_eps < tol, f"timed path differs from the eager single-chain run: rel L2 latent {rel}, eps {rel_eps}"
    return {"vs": "eager single-chain bf16 run of the same step (no graph, one stream)", "rel_l2": rel_eps, "rel_l2_latent": rel, "tol": tol,
            "what": "rel_l2 = UNet output eps [K+1,4,h,w]; rel_l2_latent = the updated latent",
            "kind": "capture sanity check: hipGraph replay vs an eager run of the SAME HIP kernels -- not oracle parity; the timed plan against the "
                    "fp32 oracle is tests/test_unet_gpu.py::test_headline_size_timed_plan_graph_vs_fp32_oracle (rel-L2 4.5e-3, bound 2e-2)"}


# ------------------------------------------------------------------------------------------------ in-situ roofline
def insitu_profile(tw, reps=3, kind="fusion", mode=None):
    """per-launch device-clock timing of the captured fusion step (or of another call kind: tools/step_shapes.py), in the schedule the timed region replays.
    Returns per-class totals of the median replay: launches, sum of launch durations, union busy time, flops."""
    import collections
    from tweediemix_amd import lib as L
    lib = L.load()
    mode = L.STEP_FUSION if mode is None else mode
    plan = tw.plan(kind)
    meta = plan.issued_meta()
    n = len(meta)
    cap = n + 64                                        # spare slots: a launch the plan's meta list does not know would shift every later stamp -- caught below
    slots = torch.zeros(cap, 8, dtype=torch.int64, device=tw.device)
    init = torch.zeros(cap, 8, dtype=torch.int64)
    init[:, 0] = -1                                     # UINT64_MAX
    init = init.to(tw.device)
    L.check(lib.tmix_prof_begin(slots.data_ptr(), cap, 0), "tmix_prof_begin")
    try:
        if tw.use_graphs:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                tw._enqueue_step(kind, mode)
            run = g.replay
        else:
            run = None
    finally:
        used = lib.tmix_prof_end()
    if run is None:                                     # eager mode: instrument every run
        def run():
            lib.tmix_prof_begin(slots.data_ptr(), cap, 0)
            tw._enqueue_step(kind, mode)
            assert lib.tmix_prof_end() == n
    else:
        assert used == n, (used, n)
    plain_ms = None
    if tw.use_graphs and (kind, mode) in tw.graphs:      # the un-instrumented graph the timed region replays, same moment
        ts_ = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()              # (host clock: timing events around replays of a graph captured over two streams corrupt the heap on ROCm 7.0, unet.refine_group)
            t0_ = time.perf_counter()
            tw.graphs[(kind, mode)].replay()
            torch.cuda.synchronize()
            ts_.append(1e3 * (time.perf_counter() - t0_))
        plain_ms = sorted(ts_[1:])[len(ts_[1:]) // 2]
    runs = []
    for _ in range(reps + 1):
        slots.copy_(init)
        torch.cuda.synchronize()
        t0_ = time.perf_counter()
        run()
        torch.cuda.synchronize()
        runs.append((1e3 * (time.perf_counter() - t0_), slots.cpu().numpy().astype("uint64")))
    runs = sorted(runs[1:], key=lambda r: r[0])
    wall_ms, sl = runs[len(runs) // 2]
    tick = 1e-5                                         # ms per tick of the 100 MHz clock
    by = collections.defaultdict(lambda: dict(launches=0, sum_ms=0.0, flops=0.0, iv=[]))
    shapes = collections.defaultdict(lambda: [0, 0.0, 0.0])
    for (cls, fl, key), s in zip(meta, sl):
        d = (int(s[1]) - int(s[0])) * tick
        c = by[cls]
        c["launches"] += 1; c["sum_ms"] += d; c["flops"] += fl; c["iv"].append((int(s[0]), int(s[1])))
        if os.environ.get("TMIX_BENCH_SHAPES"):
            k = key if isinstance(key, tuple) else ((cls, key.batch, key.M, key.N, key.K, key.epilogue, key.tile_cfg) if cls.startswith("gemm")
                                                     else (cls, key.B, key.H, key.W, key.Cin, key.Cout, key.mode, key.tile_cfg))
            shapes[k][0] += 1; shapes[k][1] += d; shapes[k][2] += fl
    for k, (cnt, ms, fl) in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
        print(f"  {str(k):64s} n={cnt:4d} total={ms:7.3f}ms avg={1e3 * ms / cnt:7.1f}us {fl / ms / 1e9 if ms else 0:6.0f}TF", file=sys.stderr)
    if os.environ.get("TMIX_BENCH_SHAPES"):            # kernel boundaries: start of launch i+1 minus end of launch i, by class pair
        gaps = collections.defaultdict(list)
        for i in range(len(meta) - 1):
            gaps[(meta[i][0], meta[i + 1][0])].append((int(sl[i + 1][0]) - int(sl[i][1])) * tick * 1e3)
        tot = sum(sum(v) for v in gaps.values())
        print(f"  boundaries between instrumented launches: {sum(len(v) for v in gaps.values())}, {tot / 1e3:.3f} ms in total", file=sys.stderr)
        for k, v in sorted(gaps.items(), key=lambda kv: -sum(kv[1])):
            v = sorted(v)
            print(f"    {k[0]:5s} -> {k[1]:5s} n={len(v):4d} sum={sum(v) / 1e3:6.3f}ms median={v[len(v) // 2]:6.2f}us p90={v[int(len(v) * 0.9)]:6.2f}us max={v[-1]:7.2f}us", file=sys.stderr)

    def union(iv):
        tot, end = 0, -1
        for a, b in sorted(iv):
            if b <= end:
                continue
            tot += b - max(a, end)
            end = b
        return tot * tick

    out = {"replay_ms": wall_ms, "uninstrumented_replay_ms": plain_ms, "launches_total": len(meta),
           "boundaries_ms": sum((int(sl[i + 1][0]) - int(sl[i][1])) for i in range(len(meta) - 1)) * tick}      # start(i+1) - end(i), summed
    all_iv = []
    for cls, c in by.items():
        all_iv += c["iv"]
        out[cls] = dict(launches=c["launches"], sum_launch_ms=c["sum_ms"], busy_ms=union(c["iv"]),
                        avg_launch_us=1e3 * c["sum_ms"] / max(1, c["launches"]), flops=c["flops"],
                        tflops=c["flops"] / max(1e-9, c["sum_ms"]) / 1e9)
    out["instrumented_busy_ms"] = union(all_iv)
    return out


FP8_DENSE_PEAK_TFLOPS = 5000.0    # MI355X_MICROARCH.md: dense e4m3 MFMA peak (the headline figures with 2:1 sparsity are not used)


def fp8_roofline(prof):
    """the fp8 plan's own roofline block: its tmix_gemm_fp8 launches (attn1 q/k/v, attn2 to_q, FF1, FF2 of every transformer block)
    against the dense fp8 MFMA peak, and what stays bf16 in that plan against the bf16 peak -- same in-situ stamps as the headline."""
    g8, g16 = prof.get("gemm_fp8"), prof.get("gemm")
    if not g8:
        return None
    out = {"bound": "mfma", "kernel": "gemm_conv_kernel<..,PH=2..5> (tmix_gemm_fp8, v_mfma_scale_f32_32x32x64_f8f6f4)",
           "achieved": g8["tflops"], "peak": FP8_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": g8["tflops"] / FP8_DENSE_PEAK_TFLOPS,
           "launches_per_step": g8["launches"], "avg_launch_us": g8["avg_launch_us"], "flops_per_step": g8["flops"],
           "sum_launch_ms": g8["sum_launch_ms"], "graph_replay_ms": prof["replay_ms"],
           "classes": {k: {kk: v[kk] for kk in ("launches", "sum_launch_ms", "busy_ms", "avg_launch_us", "tflops")}
                       for k, v in prof.items() if isinstance(v, dict)}}
    if g16:
        out["bf16_gemms_of_this_plan"] = {"launches": g16["launches"], "tflops": g16["tflops"], "frac_of_bf16_peak": g16["tflops"] / BF16_DENSE_PEAK_TFLOPS}
    return out


def gemm_alg_bytes(plan):
    """algorithmic HBM bytes of the GEMM launches: A and W read once, C written once, residual read once (bf16); GEGLU halves C."""
    from tweediemix_amd import lib as L
    gb = 0
    for d, _f in plan.launches["gemm"]:
        n_out = d.N // 2 if d.epilogue == L.EPI_GEGLU else d.N
        wsets = d.batch if d.strideW else 1
        gb += 2 * (d.batch * d.M * d.K + wsets * d.N * d.K + d.batch * d.M * n_out + (d.batch * d.M * d.N if d.residual else 0))
    return gb / max(1, len(plan.launches["gemm"]))


def conv_alg_bytes(plan):
    """algorithmic HBM bytes of the convolution launches: input (+ shortcut inputs) read once, weights once, output written once, residual once."""
    try:
        tot, n = 0, 0
        for p in ([plan] if hasattr(plan, "launches") else plan.plans):
            for d, _f in p.launches["conv"]:
                half = d.mode in (1, 4)
                ho, wo = (d.H // 2, d.W // 2) if half else ((d.H * 2, d.W * 2) if d.mode == 2 else (d.H, d.W))
                csc = d.S1_channels + d.S2_channels
                tot += 2 * (d.B * d.H * d.W * d.Cin + d.B * ho * wo * csc + d.Cout * (9 * d.Cin + csc) + d.B * ho * wo * d.Cout * (2 if d.residual else 1))
                n += 1
        return tot / max(1, n)
    except Exception:
        return None


def pmc_evidence():
    """the committed rocprofv3 PMC passes this line cites, named by profiles/MANIFEST.json (not "whatever file sorts last"):
    HBM bytes per GEMM launch (FETCH_SIZE / WRITE_SIZE in separate runs, FETCH doubled per MI355X_MICROARCH.md section HBM) and the
    time-weighted MfmaUtil per kernel class; collected by tools/collect_profile.sh with this same workload, since counters cannot be
    read from inside the process.  Returns (traffic bytes or None, {"files": ..., "mfma_util_percent": ...})."""
    man_path = os.path.join(ROOT, "profiles", "MANIFEST.json")
    try:
        man = json.load(open(man_path))
        tr = json.load(open(os.path.join(ROOT, "profiles", man["traffic"])))
        traffic = float(tr["gemm"]["hbm_bytes_per_launch_corrected"])
        mu = json.load(open(os.path.join(ROOT, "profiles", man["mfma_util"])))["per_kernel_class_time_weighted_percent"]
        return traffic, {"files": man, "mfma_util_percent": mu,
                         "traffic_bytes_per_launch_by_class": {k: float(v["hbm_bytes_per_launch_corrected"]) for k, v in tr.items()}}
    except Exception as e:                    # no profile committed (or an unreadable one): say so instead of guessing
        return None, {"files": None, "error": repr(e)}


# ------------------------------------------------------------------------------------------------ trajectories
def run_trajectories(tw, args, rank, world, device):
    """whole sample_loop runs with the reference's default flags (n=50, t_cond=0.2, resampling 10, jumping 5: 75 UNet calls)
    + the final VAE decode.  Two numbers: the latency of ONE image sampled alone (the reference's mode: one seed per process),
    and images/s with `--traj-cobatch` independent seeds sharing every UNet launch (BASELINE config 4: a batch of seeds per GPU;
    --num-seeds T shards T seeds round-robin over the ranks and gathers the latents, else every rank samples --traj-images)."""
    from tweediemix_amd import dist as D, masks as M, sampler as S, vae as V
    K = tw.concept_num
    vcfg = V.TINY if args.tiny else V.FULL
    vae = (vcfg, V.synthetic_state_dict(vcfg, device=device))     # random-init decoder of the SDXL VAE shapes

    def noise(seed_ids, h, w):
        return torch.cat([torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(7000 + s)) for s in seed_ids])

    def sampler(n_seeds):
        turn = [0]

        def provider(x0):                   # one rectangle set per seed, in the order the sampler asks
            turn[0] += 1
            return M.build_masks(M.synthetic_masks(args.masks, K, args.res, args.res, seed=31 * rank + turn[0]), tw.h, tw.w, device)
        t = S.Tweediemix(tw.config, tw.W, tw.text_embeds, tw.text_embeds_single, provider, concept_num=K, lora=tw.lora,
                         use_graphs=tw.use_graphs, n_seeds=n_seeds, n_streams=tw.n_streams, vae=vae, fp8=tw.fp8)
        return t

    out = {}
    # ---- (a) one image alone
    one = sampler(1)
    one.run_fusion(noise([rank], tw.h, tw.w), decode=True)          # builds / captures the start, plain and VAE plans
    n_calls = len(one.unet_calls)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    lat = one.run_fusion(noise([100 + rank], tw.h, tw.w))
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t1
    img = one.decode_final(lat)
    torch.cuda.synchronize()
    t_img = time.perf_counter() - t1
    tv = time.perf_counter()
    for _ in range(3):
        one.decode_final(lat)
    torch.cuda.synchronize()
    vae_ms = 1e3 * (time.perf_counter() - tv) / 3
    assert torch.isfinite(img).all()
    calls = one.unet_calls[n_calls:]
    out["vae_decode_ms"] = vae_ms
    out["trajectory_steps_per_s"] = tw.config.n_timesteps / t_loop      # scheduler steps of one image per second, whole loop
    out["single_image"] = {"seconds_loop": t_loop, "seconds_incl_vae_decode": t_img, "unet_calls": len(calls),
                           "calls_BK1": sum(1 for c in calls if c[1] == K + 1), "calls_B2": sum(1 for c in calls if c[1] == 2)}
    del one
    torch.cuda.empty_cache()
    # ---- (b) throughput: co-batched seeds
    C_ = max(1, args.traj_cobatch)
    if args.num_seeds:
        mine = D.seed_shard(list(range(args.num_seeds)), rank, world)
        total = args.num_seeds
    else:
        mine = [rank * args.traj_images + i for i in range(args.traj_images)]
        total = world * args.traj_images
    co = sampler(C_)
    batches = [mine[i:i + C_] for i in range(0, len(mine), C_)]
    warm = co.run_fusion(noise(((batches[0] if batches else [0]) * C_)[:C_], tw.h, tw.w), decode=True)
    assert torch.isfinite(warm).all()
    torch.cuda.synchronize()
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
    t1 = time.perf_counter()
    lats = []
    for b in batches:
        ids = (b + b * C_)[:C_]                       # a ragged last batch is padded with repeats and trimmed afterwards
        lat = co.run_fusion(noise(ids, tw.h, tw.w))
        img = co.decode_final(lat)
        lats.append(lat[:len(b)])
    local = torch.cat(lats) if lats else torch.zeros(0, 4, tw.h, tw.w, device=device)
    torch.cuda.synchronize()
    assert torch.isfinite(local).all()
    t_local = time.perf_counter() - t1                 # this rank's own seeds, before the gather
    gather_s = 0.0
    if args.num_seeds:                                 # the result gather: the only collective of the path (a one-rank group at N = 1)
        tg = time.perf_counter()
        gathered = D.gather_latents(local.contiguous(), total, rank, world)
        torch.cuda.synchronize()
        gather_s = time.perf_counter() - tg            # (includes waiting for the slowest rank)
        assert gathered.shape[0] == total and torch.isfinite(gathered).all()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    import torch.distributed as dist
    per_rank = [len(mine) / t_local if t_local > 0 else 0.0]
    if dist.is_initialized():
        cdev = torch.device("cpu") if dist.get_backend() == "gloo" else device
        dt = D.max_over_ranks(dt, cdev)
        pr = torch.zeros(world, dtype=torch.float64, device=cdev)
        pr[rank] = per_rank[0]
        dist.all_reduce(pr)
        per_rank = [float(v) for v in pr.cpu()]
    out["per_rank_images_per_s"] = per_rank
    out["gather_s"] = gather_s
    del co
    torch.cuda.empty_cache()
    out.update({"images": total, "seconds": dt, "images_per_s": total / dt if dt > 0 else 0.0, "cobatch": C_,
                "images_per_rank": len(mine),
                "includes": f"50-step sample_loop (start + 10 resampling repeats, plain, 5 jumping look-ahead steps, fusion) + final VAE "
                            f"decode, {C_} independent seeds per UNet launch"
                            + (" + RCCL all_gather of the latents" if world > 1 and args.num_seeds else "")})
    return out


# ------------------------------------------------------------------------------------------------ BASELINE config 5
def video_step_bench(steps=8, warmup=2, res_w=768, res_h=448, frames=16, streams=2):
    """one denoising step of run_video.py's loop (/root/reference/video_gen/pipeline_i2vgen_xl.py:680-722): I2VGen-XL UNet on the
    CFG pair of 16-frame 768x448 clips (2 x 16 x 56 x 96 latents; the two clips as two launch chains, run_video.py's default)
    + the fused CFG / v-prediction / DDIM kernel, synthetic weights, one hipGraph per step.  Returns ms, steps/s, TFLOP/s."""
    import numpy as np
    from tweediemix_amd import i2vgen as I, ops
    from tweediemix_amd.weights import synthetic_i2vgen_state_dict
    h, w, Fr = res_h // 8, res_w // 8, frames
    t0 = time.perf_counter()
    sd = synthetic_i2vgen_state_dict(I.FULL, dtype=torch.bfloat16, device="cuda")        # drawn on the device: plan_build_s 24 -> ~2 s
    Wt = I.I2VWeights(I.FULL, sd)
    del sd
    g = torch.Generator().manual_seed(0)
    il = torch.randn(2, 4, Fr, h, w, generator=g)
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0, 8.0]), il, torch.randn(2, 1024, generator=g), torch.randn(2, 77, 1024, generator=g))
    plan = (I.I2VPlanGroup if streams == 2 else I.I2VPlan)(Wt, 2, Fr, h, w, fe, ctx, ilf)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    x = torch.randn(1, 4, Fr, h, w, generator=g).cuda()
    out = torch.empty_like(x)
    acp = (np.cos((np.arange(1000) / 1000 + 0.008) / 1.008 * np.pi / 2) ** 2).astype(np.float32)
    cin = I.FULL.in_channels

    def step():
        if streams == 2:
            plan.set_input(x, 981)
        else:
            plan.x_in.view(2, Fr, 2 * cin, h, w)[:, :, :cin] = x.permute(0, 2, 1, 3, 4)
            plan.t_dev.fill_(981.0)
        plan.run()
        v = plan.eps.view(2, Fr, I.FULL.out_channels, h, w).permute(0, 2, 1, 3, 4).contiguous()
        ops.vpred_step(x, v, 9.0, acp[981], acp[961], out=out)
        x.copy_(out)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t1) / steps
    assert torch.isfinite(x).all()
    from tweediemix_amd import lib as L_

    def n_kernels(fn, a):
        n = getattr(fn, "__name__", "")
        if n == "tmix_gemm_prefetch_next":
            return 0
        if n == "tmix_groupnorm_nhwc":            # (x1, C1, x2, C2, out, gamma, beta, ws, B, HW, groups, eps, silu): three launches, or one for small images
            return L_.load().tmix_groupnorm_nhwc_launches(a[9], a[1] + a[3], a[10])
        return 2 if n.startswith("tmix_groupnorm_nhwc_pre") else 1
    kernels = sum(n_kernels(fn, a) for fn, a in plan.ops) + 1
    res = {"workload": f"BASELINE configs[4]: I2VGen-XL (1.42 B parameters, synthetic), {frames} frames {res_w}x{res_h}, CFG pair = 2 clips, "
                       f"{streams} launch chain(s), one denoising step = UNet + fused CFG/v-prediction/DDIM kernel, hipGraph replay",
           "value": 1e3 / ms, "unit": "steps/s", "ms_per_step": ms, "unet_tflop_per_step": plan.flops / 1e12,
           "achieved_tflops": plan.flops / ms / 1e9, "seconds_per_50_step_video": 50 * ms / 1e3, "launches_per_step": kernels,
           "launches_what": "GPU kernels per step (a GroupNorm call is three -- statistics, combine, apply --, two on the producers' partials, one for small frames; the weight-prefetch hints in the op list are host-side only)",
           "plan_build_s": build_s, "dtype": "bf16"}
    del plan, Wt
    torch.cuda.empty_cache()
    return res


# ------------------------------------------------------------------------------------------------ CPU baseline
def cpu_baseline(args, parts, K=3):
    """the oracle (fp32 torch-CPU restatement of the same UNet) on the GPU box's host cores.  Measured: BASELINE.json
    config 1 -- one B=K+1 call and one B=2 call at 512x512, combined with that config's 27 / 18 call schedule; and, kept as
    `extrapolated_1024`, one batch row of the 1024x1024 fusion-step call scaled by K+1 (rows are independent)."""
    from oracle import unet_oracle as UO
    sd, con, te, ts, cfg = parts
    ocfg = UO.TINY if args.tiny else UO.SDXL
    t0 = time.time()
    sd_cpu = {k: v.float().cpu() for k, v in sd.items()}
    orc = UO.UNetOracle(ocfg, sd_cpu)        # base weights (the concept deltas do not change the cost)
    cores = min(os.cpu_count() or 1, args.cpu_threads)     # torch-CPU stops scaling (and thrashes) far below 256 threads
    torch.set_num_threads(cores)
    prep = time.time() - t0

    def call(rows, res):
        h = w = res // 8
        torch.manual_seed(0)
        x = torch.randn(rows, 4, h, w)
        tid = torch.tensor([[res, res, 0, 0, res, res]] * rows, dtype=torch.float32)
        t1 = time.time()
        orc.forward(x, 781, te[0][:rows], te[1][:rows], tid)
        return time.time() - t1

    small = 512 if not args.tiny else args.res
    t4 = call(K + 1, small)
    t2 = call(2, small)
    traj = 27 * t4 + 18 * t2                 # config 1 = 27 calls at B=4 + 18 at B=2
    t1row = call(1, args.res)
    return dict(value=1.0 / ((K + 1) * t1row), unit="steps/s", cores=cores, kind="port",
                sample=f"the headline workload ({args.res}x{args.res} fusion-phase step, UNet B={K + 1}): ONE of its {K + 1} batch rows through the fp32 "
                       f"torch-CPU oracle ({t1row:.1f}s on {cores} threads); rows are independent, value = 1 / ({K + 1} x that) steps/s.  Also measured: "
                       f"BASELINE config 1 ({small}x{small}): one B={K + 1} call {t4:.1f}s, one B=2 call {t2:.1f}s (see config1); weight copy {prep:.1f}s not counted",
                config1={"resolution": small, "t_call_B4_s": t4, "t_call_B2_s": t2, "calls": "27 @B=4 + 18 @B=2",
                         "trajectory_s": traj, "trajectory_steps_per_s": 20.0 / traj},
                headline_row={"t_one_row_s": t1row, "rows": K + 1},
                config1_steps_per_s=1.0 / t4)


# ------------------------------------------------------------------------------------------------ dry run (CPU tests)
def host_dry_run(args, rank, world):
    """the N-rank control flow of this script without a GPU: rendezvous, barrier-bracketed timing, MAX over ranks, seed
    sharding and the latent gather, over gloo.  The step is a stand-in; the line says so."""
    import torch.distributed as dist
    from tweediemix_amd import dist as D
    if world > 1:
        dist.init_process_group("gloo")
    x = torch.full((args.seeds_per_gpu, 4, 8, 8), float(rank))
    for _ in range(args.warmup):
        x = x * 0.5 + 1.0
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        x = x * 0.5 + 1.0
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        dt = D.max_over_ranks(dt, torch.device("cpu"))
    total = args.num_seeds or world * args.seeds_per_gpu
    mine = D.seed_shard(list(range(total)), rank, world) if args.num_seeds else [rank * args.seeds_per_gpu + i for i in range(args.seeds_per_gpu)]
    local = torch.stack([torch.full((4, 8, 8), float(s)) for s in mine]) if mine else torch.zeros(0, 4, 8, 8)
    gathered = D.gather_latents(local, total, rank, world) if (world > 1 and args.num_seeds) else local
    ok = (not args.num_seeds) or all(float(gathered[i, 0, 0, 0]) == float(i) for i in range(total))
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": world * args.seeds_per_gpu * args.steps / dt, "unit": "steps/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
                          "data": "DRY RUN: launcher / collective control flow on CPU over gloo, stand-in step, no kernels -- not a measurement",
                          "config": {"workload": "none (host dry run)", "seeds_total": total, "gather_ok": bool(ok)}}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 1


# ------------------------------------------------------------------------------------------------ main
def main(argv=None):
    args = parse(argv)
    from tweediemix_amd import launch as LA
    if args.gpus > 1 and not LA.launched():
        return LA.self_launch(args.gpus)
    rank, local, world = LA.rank_env()
    if args.host_dry_run:
        return host_dry_run(args, rank, world)
    # stdout carries exactly ONE line, the JSON: everything else this process (or a library under it -- RCCL prints a version
    # banner through C stdio when its first communicator comes up) writes to file descriptor 1 goes to stderr instead
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback for the product path)"
    if os.environ.get("TMIX_SINGLE_GPU_DIST_TEST"):     # debug only: all ranks share GPU 0 over gloo (control-flow test)
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import torch.distributed as dist
    from tweediemix_amd import dist as D
    # one process group per job -- ALSO at N = 1: RCCL is loaded, bound to this device, and carries the timing / gather collectives
    backend = D.init(device, world, "gloo" if os.environ.get("TMIX_SINGLE_GPU_DIST_TEST") else None)
    ranks_seen = D.ranks_seen(torch.device("cpu") if backend == "gloo" else device)
    assert ranks_seen == world, (ranks_seen, world)

    primary = "lora" if args.kind in ("both", "lora") else "custom"
    t_start = time.perf_counter()
    tw, parts = build_sampler(args, primary, device, seed=rank)       # each rank owns its own seeds (weak scaling)
    torch.cuda.synchronize()
    startup_s = time.perf_counter() - t_start                         # synthetic weights + per-concept LoRA merges + layout conversion, per rank
    K, S_ = tw.concept_num, args.seeds_per_gpu
    plan = tw.plan("fusion")
    from tweediemix_amd import unet as U
    # the timed plan runs the tilings of the SHIPPED table (nothing re-tuned on this box): the same assertion the oracle parity
    # tests make for the plan they check (tests/test_unet_gpu.py::test_headline_size_timed_plan_graph_vs_fp32_oracle)
    follows, bad = U.tilings_follow_table(plan)
    # a launch whose shape the table HOLDS must run the table's tiling (a deviation means something re-tuned it on this box); a shape the table
    # does not hold (non-default --res / --seeds-per-gpu / --lora-mode lowrank) was timed when the plan was built: reported, not fatal
    deviating = [b for b in bad if b[2] is not None]
    assert not deviating or os.environ.get("TMIX_TUNE_FILE") is not None or args.tiny, f"timed plan deviates from the shipped tile table: {deviating[:5]}"
    tilings = {"used": U.used_tilings(plan), "follow_shipped_table": follows, "shapes_not_in_table": len(bad) - len(deviating),
               "table": os.path.basename(U._TUNE_FILE) if U._TUNE_FILE else None}
    plan_build_s = time.perf_counter() - t_start - startup_s
    x = torch.randn(S_, 4, tw.h, tw.w, generator=torch.Generator().manual_seed(1000 + rank)).to(device)
    cdev = torch.device("cpu") if backend == "gloo" else device
    # the FIRST window: W warm-up + K timed steps right behind the plan build (what rounds 1-4 reported as `value`).  A plain run puts SETTLE_S seconds of untimed
    # replays of the same step in front of it, so that its `value` is the chip's sustained state, as the end-of-run window of --full is (see there).
    dt_first, outputs = timed_fusion_steps(tw, args, world, device, x, settle_s=0.0 if args.full else SETTLE_S)
    dt_first = D.max_over_ranks(dt_first, cdev)                                         # through the group also at N = 1
    dt, max_abs_latent, flops_step = dt_first, tw.last_window_max_abs_latent, plan.flops
    full_line, full_config = {}, {"value_window": f"W + K steps behind {SETTLE_S:g} s of untimed replays of the same step (sustained state)"}
    if args.full:
        # This chip needs ~3 s of load (~100 steps) to reach the state it then holds (tools/step_gap.py, same process, same graph: 31.2 -> 30.4 -> 28.6 -> 28.6 ms per
        # step over consecutive 50-step windows; the 32-byte parameter upload and the replay-to-replay gap cost nothing: upload + replay 28.56, replay only 28.55, one
        # replay behind a synchronize 28.56), and a denoising trajectory is 75 UNet calls = 2 s long.  So --full's `value` is the SAME measurement (W untimed + exactly
        # K timed steps, barrier + synchronize on both sides, MAX over ranks) taken once more at the END of the run, behind the parity check, the in-situ profile and
        # the trajectory measurement -- the sustained state; the first window stays in the line as `first_window`.
        check = parity_check(tw, args, parts, primary, device)
        prof = insitu_profile(tw) if rank == 0 else None
        traj = None if args.no_trajectory else run_trajectories(tw, args, rank, world, device)
        dt, outputs = timed_fusion_steps(tw, args, world, device, x)
        dt = D.max_over_ranks(dt, cdev)
        max_abs_latent = tw.last_window_max_abs_latent
        chip = chip_state_under_load(tw, device, x) if rank == 0 else None
        # the same window once more on the OTHER synthetic mask kind, same process, same graph (the masks live at a fixed address the captured step reads), chip state
        # beside it: rounds 1-5 timed intersecting rectangles, on which the un-normalised blend doubles the overlap region every fusion step
        other_kind = "overlap" if args.masks == "partition" else "partition"
        tw.masks = tw.mask_sets(other_kind)
        dt_o, _xo = timed_fusion_steps(tw, args, world, device, x)
        dt_o = D.max_over_ranks(dt_o, cdev)
        other_masks = {"masks": other_kind, "ms_per_step": 1e3 * dt_o / (args.steps * args.seeds_per_gpu), "value": world * args.seeds_per_gpu * args.steps / dt_o,
                       "max_abs_latent_at_end_of_window": tw.last_window_max_abs_latent,
                       "chip_state_under_load": chip_state_under_load(tw, device, x) if rank == 0 else None,
                       "what": "the same W + K steps, same captured graph, right behind the `value` window, with the other synthetic mask kind"}
        tw.masks = tw.mask_sets()

        alg = gemm_alg_bytes(plan)
        conv_alg = conv_alg_bytes(plan)
        other = {}
        if args.kind == "both" and world == 1:
            del tw, plan
            torch.cuda.empty_cache()
            tw2, _parts2 = build_sampler(args, "custom", device, seed=rank)
            dt2, _ = timed_fusion_steps(tw2, args, world, device, x)
            other["custom"] = {"workload": "BASELINE configs[1]: Custom-Diffusion K/V deltas", "value": S_ * args.steps / dt2, "unit": "steps/s",
                               "ms_per_step": 1e3 * dt2 / (args.steps * S_), "parity_check": parity_check(tw2, args, _parts2, "custom", device)}
            del tw2
            torch.cuda.empty_cache()
            if args.dtype == "bf16" and not args.tiny:
                tw3, _parts3 = build_sampler(args, primary, device, seed=rank, fp8=True)
                dt3, _ = timed_fusion_steps(tw3, args, world, device, x)
                other["fp8"] = {"workload": f"{primary} deltas; every projection of every transformer block (attn1 q/k/v, both attention out-projections, attn2 to_q, FF1, "
                                            "FF2: 420 of the 442 GEMM launches) on e4m3 operands with power-of-two scales (tmix_gemm_fp8); no quantiser launch inside a block: "
                                            "the GEMMs that write the residual stream and the attention kernels (tmix_attn_fwd_f8) leave e4m3 + MX-block copies, FF1 -> FF2 "
                                            "chained through the GEGLU epilogue; the ResnetBlock2D convolutions whose K-tile can be 128 channels of one tap and that carry no shortcut taps "
                                            "(15 of 38) on e4m3 as well (tmix_conv3x3_nhwc_fp8 behind tmix_groupnorm_nhwc_pre_f8); proj_in / proj_out, the other convolutions and the "
                                            "attention inner products stay bf16",
                                "dtype": "fp8", "value": S_ * args.steps / dt3, "unit": "steps/s", "ms_per_step": 1e3 * dt3 / (args.steps * S_),
                                "parity_check": parity_check(tw3, args, _parts3, primary, device)}
                if rank == 0:
                    other["fp8"]["roofline"] = fp8_roofline(insitu_profile(tw3))
                if not args.no_trajectory:                 # the same whole-trajectory / images-per-second measurement on the fp8 plans (every call kind: B = K+1 and B = 2)
                    tr8 = run_trajectories(tw3, args, rank, world, device)
                    other["fp8"].update({"trajectory_steps_per_s": tr8["trajectory_steps_per_s"], "images_per_s": tr8["images_per_s"],
                                         "single_image_seconds_loop": tr8["single_image"]["seconds_loop"], "cobatch": tr8["cobatch"]})
                del tw3
                torch.cuda.empty_cache()
            if not args.tiny and not args.no_video:
                other["video"] = video_step_bench()

        if rank == 0:
            g = prof["gemm"] if args.dtype == "bf16" or "gemm_fp8" not in prof else prof["gemm_fp8"]
            peak_tf = BF16_DENSE_PEAK_TFLOPS if g is prof.get("gemm") else FP8_DENSE_PEAK_TFLOPS
            pmc = pmc_evidence()
            full_config = {"value_window": "end of run (sustained state); first_window_ms_per_step = the same W + K steps right behind the plan build (what rounds 1-4 reported)",
                           "first_window_ms_per_step": 1e3 * dt_first / (args.steps * S_),
                           "other_mask_kind_ms_per_step": other_masks["ms_per_step"]}
            full_line = {
                "first_window": {"ms_per_step": 1e3 * dt_first / (args.steps * S_), "value": world * S_ * args.steps / dt_first,
                                 "what": "the same W + K steps timed right behind the plan build (rounds 1-4 reported this window); `value` is the window at the end of the "
                                         "run, after >= 3 s of load (parity check, in-situ profile, trajectories): the state the chip holds through a 2 s trajectory"},
                "chip_state_under_load": chip,
                "other_mask_kind_window": other_masks,
                "parity_check": check,
                "roofline": {"bound": "mfma", "kernel": "gemm_conv_kernel<..,CONV=0> (tmix_gemm_bf16)" if g is prof.get("gemm") else "gemm_conv_kernel<..,PH=2|3> (tmix_gemm_fp8)",
                             "achieved": g["tflops"], "peak": peak_tf, "unit": "TFLOP/s", "frac": g["tflops"] / peak_tf,
                             "traffic": pmc[0],
                             "traffic_source": "NOT measured in this run: read from the committed rocprofv3 PMC passes named in profiles/MANIFEST.json (the builder's box, same command; "
                                               "counters cannot be read from inside the process) -- see pmc.files",
                             "pmc": pmc[1], "algorithmic_bytes_per_launch": alg,
                             "how": "achieved = sum(2MNK of the step's GEMM launches, plus the 4*M*77*N attention flops of the one-launch attn2 -- tmix_gemm_q_cross_attn -- which that launch performs) / sum(their durations), each launch timed on the device clock "
                                    "INSIDE the captured step while the graph replays (concurrent chains included, so the sum can exceed the wall time)",
                             "launches_per_step": g["launches"], "avg_launch_us": g["avg_launch_us"], "flops_per_step": g["flops"],
                             "launches_per_step_all_classes": prof["launches_total"], "kernel_boundaries_ms": prof["boundaries_ms"],
                             "conv": {"traffic": (pmc[1].get("traffic_bytes_per_launch_by_class") or {}).get("conv"),
                                      "algorithmic_bytes_per_launch": conv_alg, "achieved": (prof.get("conv") or {}).get("tflops")},
                             "graph_replay_ms": prof["replay_ms"], "uninstrumented_graph_replay_ms": prof["uninstrumented_replay_ms"],
                             "instrumented_busy_ms": prof["instrumented_busy_ms"],
                             "classes": {k: {kk: v[kk] for kk in ("launches", "sum_launch_ms", "busy_ms", "avg_launch_us", "tflops")}
                                         for k, v in prof.items() if isinstance(v, dict)}},
            }
            if traj is not None:
                full_line["images_per_s"] = traj["images_per_s"]
                full_line["vae_decode_ms"] = traj["vae_decode_ms"]
                full_line["trajectory_steps_per_s"] = traj["trajectory_steps_per_s"]
                full_line["trajectory"] = traj
            if other:
                full_line["other_configs"] = other
            if world == 1 and not args.no_cpu_baseline:
                full_line["cpu_baseline"] = cpu_baseline(args, parts)

    if rank == 0:
        if args.dump_outputs:
            dump_outputs(outputs, args.dump_outputs)
        line = {
            "metric": METRIC, "value": world * S_ * args.steps / dt, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / (args.steps * S_), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "max_abs_latent_at_end_of_window": max_abs_latent,
            "config": {"workload": f"SDXL-base UNet shapes, {args.res}x{args.res}, K=3 concepts ({primary} deltas"
                                   + (", --t_stop 0.8 window" if primary == "lora" else "") + "), "
                                   f"fusion-phase step = UNet B={K + 1} + fused Tweedie/CFG/blend/DDIM kernel, one hipGraph per step"
                                   + (" [TINY DEBUG CONFIG]" if args.tiny else ""),
                       "masks": f"{args.masks}: synthetic rectangles " + ("that partition the image (fg_1 + fg_2 + bg = 1 on every pixel)" if args.masks == "partition"
                                                                            else "that may intersect (un-normalised blend weights sum to 2 on the overlap)"),
                       **full_config,
                       "seeds_per_gpu": S_, "streams": args.streams, "hip_graph": not args.no_graphs,
                       "parallelism": f"replicas x{world} (seed-sharded, no data-path collective)", "tilings": tilings},
            "dist": {"backend": backend + (" (RCCL)" if backend == "nccl" else ""), "world_size": world, "ranks_seen": ranks_seen,
                     "what": "ranks_seen = all-reduce of ones over the job's process group on the device; the step timing (MAX over ranks) and the "
                             "trajectory latents go through the same group, also at N = 1",
                     "startup_s_per_rank": startup_s, "plan_build_s": plan_build_s,
                     "startup_what": "synthetic weight generation + per-concept LoRA merges + kernel-layout conversion on this rank's GPU (ranks start "
                                     "concurrently, each on its own device: no shared host-side stage)"},
            "unet_tflop_per_step": flops_step / 1e12 / S_,
            "achieved_tflops_whole_step": flops_step / 1e12 / (dt / args.steps),
            **full_line,
        }
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
