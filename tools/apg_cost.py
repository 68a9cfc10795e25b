"""cost of adaptive projected guidance in the whole step.

(1) One captured fusion step of the SDXL sampler at 1024^2 with K = 3 (B = 4 rows per seed), at one seed and at eight co-batched seeds, whose tail is
(a) tmix_fused_tweedie_step_dev -- the default, apg = None -- and (b) tmix_apg_coeffs + tmix_fused_tweedie_step_apg_dev: one more read of the state and
the eps rows and two small launches.  ONE sampler per seed count, so both graphs replay the same plan on the same buffers and differ in their tail
only.  10 replays per round, three interleaved rounds in one process; the comparison side is the flag-off step of the same run, and the rounds' spread
is reported beside the difference (the method of section 7e), with the clock sampled behind the timed rounds.
(2) The new launches alone on the plan's eps rows: tmix_apg_coeffs (partials + finalise) and the APG step entry, with the default step entry beside
it; 50 calls captured into one graph, the replay's time / 50.

    python tools/apg_cost.py [custom|lora] [--out profiles/apg_cost.json]"""
import collections, json, os, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, ops, sampler as S

kind = next((a for a in sys.argv[1:] if a in ("custom", "lora")), "custom")
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "apg_cost.json")
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num
APG = dict(eta=0.0, norm_threshold=15.0)
conf = S.make_config(**{**vars(base.config), "guidance_scale": 9.0})       # the CLIs' default scale (the cost does not depend on it)
print(f"{torch.cuda.get_device_name(dev)}; {kind}, K = {K}, g = {conf.guidance_scale}, apg = {APG}")
result = dict(tool="tools/apg_cost.py", device=torch.cuda.get_device_name(dev), kind=kind, K=K, guidance_scale=conf.guidance_scale, apg=APG,
              method="captured fusion step at 1024^2, 10 replays per round, 3 interleaved rounds, minimum of the rounds; alone: 50 captured calls, best of 5 replays",
              seeds={})


def captured_us(call, n=50):
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            call()
    per = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6 / n)
    return min(per)


for seeds in (1, 8):
    tw = S.Tweediemix(conf, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, n_seeds=seeds, apg=APG)
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
    tw.masks = base.masks
    at, at_next = base.alpha(501), base.alpha(481)

    def step(apg):
        tw.apg = apg                                   # None: the default tail and graph key; the buffers of the flag stay allocated either way
        tw._run_step("fusion", L.STEP_FUSION, 501, at, at_next)
    x0 = torch.randn(seeds, 4, base.h, base.w, device=dev)
    res = collections.defaultdict(list)
    for rnd in range(3):
        for name, apg in (("off", None), ("apg", APG)):
            tw.x_state.copy_(x0)
            for _ in range(3):
                step(apg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step(apg)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 100)
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    assert sorted(tw.graphs, key=len) == [("fusion", L.STEP_FUSION), ("fusion", L.STEP_FUSION, "apg")]
    p = tw.plan("fusion")
    print(f"fusion step, {seeds} seed(s), B = {p.B}, ms per replay (three rounds, interleaved), sclk {clk} MHz behind the timed rounds:")
    spread = {}
    for name, v in res.items():
        spread[name] = 100 * (max(v) - min(v)) / min(v)
        print(f"  {name:3s}  rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {spread[name]:.1f} %")
    a, b = min(res["off"]), min(res["apg"])
    print(f"  APG step minus default step: {1000 * (b - a):+.1f} us ({100 * (b - a) / a:+.2f} % of the step)", flush=True)
    # the new launches alone, on this plan's eps rows and the sampler's state
    rows = p.B // seeds
    co, ws = torch.empty(seeds, rows - 1, 2, device=dev), ops.cfg_rescale_ws(rows, seeds, dev)
    xs, o0 = x0.clone(), torch.empty_like(x0)
    us_co = captured_us(lambda: ops.apg_coeffs(xs, p.eps, L.STEP_FUSION, K, tw.step_params, 6, out=co, ws=ws, **APG))
    us_step = captured_us(lambda: ops.fused_tweedie_step_apg_dev(xs, p.eps, tw.masks, L.STEP_FUSION, K, tw.step_params, co, out_x=o0, out_x0=tw.x0_state))
    head = ops._dev_step_head(xs, p.eps, tw.masks, L.STEP_FUSION, K, tw.step_params, o0, tw.x0_state)[5]
    st = lambda: torch.cuda.current_stream().cuda_stream
    us_base = captured_us(lambda: L.check(L.load().tmix_fused_tweedie_step_dev(*head, st()), "tmix_fused_tweedie_step_dev"))
    mb = p.eps.numel() * p.eps.element_size() / 1e6
    print(f"  alone ({mb:.2f} MB of eps rows): tmix_apg_coeffs {us_co:.1f} us, tmix_fused_tweedie_step_apg_dev {us_step:.1f} us, "
          f"tmix_fused_tweedie_step_dev {us_base:.1f} us per call; coefficients of seed 0: {[[round(float(v), 4) for v in r] for r in co[0]]}", flush=True)
    result["seeds"][str(seeds)] = dict(B=p.B, sclk_mhz=clk, step_ms_off_rounds=[round(x, 4) for x in res["off"]], step_ms_apg_rounds=[round(x, 4) for x in res["apg"]],
                                       step_ms_off=round(a, 4), step_ms_apg=round(b, 4), difference_us=round(1000 * (b - a), 1),
                                       difference_percent=round(100 * (b - a) / a, 3), spread_percent_off=round(spread["off"], 2),
                                       spread_percent_apg=round(spread["apg"], 2), eps_mb=round(mb, 2), apg_coeffs_us=round(us_co, 1),
                                       apg_step_us=round(us_step, 1), default_step_us=round(us_base, 1))
    del tw, p
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(f"wrote {out_path}")
