"""what an unguided step saves.

(1) The captured step of the SDXL sampler at 1024^2, K = 3, bf16, partition masks, at one seed and at eight co-batched seeds: "fusion" (K + 1 rows per
seed, ending in tmix_fused_tweedie_step_dev) against "fusion_c" (K rows, ending in tmix_fused_tweedie_step_cond_dev), and "plain" (2 rows) against
"plain_c" (1 row).  ONE sampler per seed count and one build: both sides are the same library, weights and buffers.  Replays per round as printed,
three interleaved rounds, the minimum of the rounds (the method of section 7e), the box's clock sampled right behind the timed rounds.  The new batch
sizes have no entry in the tuned tile table: their tilings are whatever the build-time tuner picks when the plan is built.
(2) The UNet rows of a whole image, counted from unet_calls of a run whose launches are skipped (the control flow, the plans and their row counts
are the sampler's own): n = 50 (DDIM, 'leading' grid) and n = 10 (dpmpp2m, 'logsnr' grid) with the CLI's defaults otherwise, with and without the
example interval.

    python tools/guidance_interval_cost.py [custom|lora] [--out FILE.json] [--interval T_HI,T_LO]"""
import collections, json, os, socket, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, sampler as S
from tweediemix_amd.guidance import validate_interval

argv = sys.argv[1:]
kind = next((a for a in argv if a in ("custom", "lora")), "custom")
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
INTERVAL = validate_interval(argv[argv.index("--interval") + 1] if "--interval" in argv else "700,250", "--interval")
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num
conf = S.make_config(**{**vars(base.config), "guidance_scale": 9.0})       # the CLIs' default scale (the cost does not depend on it)
box = socket.gethostname()
print(f"box {box}, {torch.cuda.get_device_name(dev)}; {kind}, K = {K}, g = {conf.guidance_scale}, interval {INTERVAL}")
result = {"tool": "tools/guidance_interval_cost.py", "box": box, "device": torch.cuda.get_device_name(dev), "kind": kind, "K": K, "res": args.res,
          "dtype": "bf16", "masks": args.masks, "interval": list(INTERVAL), "steps": [], "rows_per_image": []}


def init(tw):
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))


plans_one_seed = None
for seeds in (1, 8):
    reps = 10 if seeds == 1 else 5
    tw = S.Tweediemix(conf, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, n_seeds=seeds,
                      guidance_interval=INTERVAL)
    init(tw)
    tw.masks = base.masks
    at, at_next = base.alpha(501), base.alpha(481)
    x0 = torch.randn(seeds, 4, base.h, base.w, device=dev)
    pairs = (("fusion", "fusion_c", L.STEP_FUSION), ("plain", "plain_c", L.STEP_PLAIN))
    res = collections.defaultdict(list)
    for rnd in range(3):
        for a, b, mode in pairs:
            for k in (a, b):
                tw.x_state.copy_(x0)
                for _ in range(3):                    # the first call builds the plan (and tunes its new shapes) and captures the graph
                    tw._run_step(k, mode, 501, at, at_next)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    tw._run_step(k, mode, 501, at, at_next)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / reps)
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    assert sorted(tw.graphs) == sorted((k, m) for a, b, m in pairs for k in (a, b)), sorted(tw.graphs)
    print(f"{seeds} seed(s), ms per replay ({reps} replays per round, three rounds, interleaved), sclk {clk} MHz behind the timed rounds:")
    for a, b, _m in pairs:
        for k in (a, b):
            v = res[k]
            print(f"  {k:9s} B = {tw.plan(k).B:2d}  rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %")
        ga, gb = min(res[a]), min(res[b])
        print(f"  {b} / {a} = {gb / ga:.3f}  ({ga - gb:+.3f} ms saved per step; rows {tw.plan(b).B}/{tw.plan(a).B} = {tw.plan(b).B / tw.plan(a).B:.3f})", flush=True)
        result["steps"].append({"seeds": seeds, "guided": a, "unguided": b, "B_guided": tw.plan(a).B, "B_unguided": tw.plan(b).B, "replays_per_round": reps,
                                "ms_guided_rounds": res[a], "ms_unguided_rounds": res[b], "ms_guided": ga, "ms_unguided": gb, "ratio": gb / ga,
                                "sclk_mhz_after": clk})
    if seeds == 1:
        plans_one_seed = tw.plans
    del tw
    torch.cuda.empty_cache()

# (2) rows per image: the sampler's own loop and plans, the launches skipped
for n, solver, spacing in ((50, "ddim", "leading"), (10, "dpmpp2m", "logsnr")):
    for interval in (None, INTERVAL):
        c = S.make_config(**{**vars(conf), "n_timesteps": n})
        tw = S.Tweediemix(c, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=False, solver=solver, timestep_spacing=spacing,
                          guidance_interval=interval)
        tw.plans = plans_one_seed                         # same weights and shapes: the plans the timing built (others are built lazily)
        tw._enqueue_step = lambda *a, **k: None
        tw.run_fusion(torch.zeros(1, 4, base.h, base.w))
        rows = sum(r for _k, r, _t in tw.unet_calls)
        by_kind = collections.Counter()
        for k, r, _t in tw.unet_calls:
            by_kind[f"{k} x{r}"] += 1
        print(f"n = {n} ({solver}, {spacing}; resampling {c.resampling_steps}, jumping {c.jumping_steps}), interval {interval}: {len(tw.unet_calls)} UNet calls, "
              f"{rows} rows per image; calls by kind and rows {dict(by_kind)}", flush=True)
        result["rows_per_image"].append({"n": n, "solver": solver, "spacing": spacing, "interval": None if interval is None else list(interval),
                                         "calls": len(tw.unet_calls), "rows": rows, "calls_by_kind_and_rows": dict(by_kind)})
        del tw
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {out_path}")
