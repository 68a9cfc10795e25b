"""cost of guidance rescale in the whole step.

(1) One captured fusion step of the SDXL sampler at 1024^2 with K = 3 (B = 4 rows per seed), at one seed and at eight co-batched seeds, whose tail is
(a) tmix_fused_tweedie_step_dev -- the default, guidance_rescale = 0 -- and (b) tmix_cfg_rescale_factors + tmix_fused_tweedie_step_rs_dev at phi = 0.7: one
more read of the eps rows and two small launches.  ONE sampler per seed count, so both graphs replay the same plan on the same buffers and differ in
their tail only.  10 replays per round, three interleaved rounds, the minimum of the rounds (the method of section 7e), the box's clock beside the numbers.
(2) The two new launches alone on the plan's eps rows: 50 calls captured into one graph, the replay's time / 50.

    python tools/rescale_cost.py [custom|lora]"""
import collections, os, socket, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, ops, sampler as S

kind = next((a for a in sys.argv[1:] if a in ("custom", "lora")), "custom")
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num
PHI = 0.7
conf = S.make_config(**{**vars(base.config), "guidance_scale": 9.0})       # the CLIs' default scale (the cost does not depend on it)
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; {kind}, K = {K}, g = {conf.guidance_scale}, phi = {PHI}")

for seeds in (1, 8):
    tw = S.Tweediemix(conf, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, n_seeds=seeds, guidance_rescale=PHI)
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
    tw.masks = base.masks
    at, at_next = base.alpha(501), base.alpha(481)

    def step(phi):
        tw.guidance_rescale = phi                      # 0: the default tail and graph key; the buffers of phi > 0 stay allocated either way
        tw._run_step("fusion", L.STEP_FUSION, 501, at, at_next)
    x0 = torch.randn(seeds, 4, base.h, base.w, device=dev)
    res = collections.defaultdict(list)
    for rnd in range(3):
        for phi in (0.0, PHI):
            tw.x_state.copy_(x0)
            for _ in range(3):
                step(phi)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step(phi)
            torch.cuda.synchronize()
            res[phi].append((time.perf_counter() - t0) * 100)
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    assert sorted(tw.graphs, key=len) == [("fusion", L.STEP_FUSION), ("fusion", L.STEP_FUSION, "rs")]
    p = tw.plan("fusion")
    print(f"fusion step, {seeds} seed(s), B = {p.B}, ms per replay (three rounds, interleaved), sclk {clk} MHz behind the timed rounds:")
    for phi, v in res.items():
        print(f"  guidance_rescale {phi:3.1f}  rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %")
    a, b = min(res[0.0]), min(res[PHI])
    print(f"  rescaled step minus default step: {1000 * (b - a):+.1f} us ({100 * (b - a) / a:+.2f} % of the step)", flush=True)
    # the two new launches alone, on this plan's eps rows
    rows = p.B // seeds
    fac, ws = torch.empty(seeds, rows - 1, device=dev), ops.cfg_rescale_ws(rows, seeds, dev)
    call = lambda: ops.cfg_rescale_factors(p.eps, seeds, L.STEP_FUSION, K, tw.step_params, 6, PHI, out=fac, ws=ws)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(50):
            call()
    per = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6 / 50)
    mb = p.eps.numel() * p.eps.element_size() / 1e6
    print(f"  tmix_cfg_rescale_factors alone (partials + finalise, {mb:.2f} MB of eps rows, {mb / seeds:.2f} MB per seed): {min(per):.1f} us per call "
          f"(50 captured calls, best of 5 replays); factors of seed 0: {[round(float(v), 4) for v in fac[0]]}", flush=True)
    del tw, g, p
    torch.cuda.empty_cache()
