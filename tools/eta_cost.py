"""cost of the stochastic step in the whole step.

(1) One captured fusion step of the SDXL sampler at 1024^2 with K = 3 (B = 4 rows per seed), at one seed and at eight co-batched seeds, whose tail is
(a) tmix_fused_tweedie_step_dev -- the deterministic step: the entry, launch and graph key of eta = 0 -- and (b) tmix_fused_tweedie_step_noise_dev at
eta = 1: the same reads and writes plus one Philox4x32-10 call and one Box-Muller per element, and 48 instead of 32 uploaded bytes.  ONE sampler per seed
count, so both graphs replay the same plan on the same buffers and differ in their tail only.  10 replays per round, three interleaved rounds, the
minimum of the rounds (the method of section 7e), the box's clock beside the numbers.
(2) The noise entry against its parent entry alone on the plan's eps rows, and tmix_noise_normal on as many elements: 50 calls captured into one graph,
the replay's time / 50.

    python tools/eta_cost.py [custom|lora]"""
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
ETA = 1.0
conf = S.make_config(**{**vars(base.config), "guidance_scale": 9.0})       # the CLIs' default scale (the cost does not depend on it)
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}; {kind}, K = {K}, g = {conf.guidance_scale}, eta = {ETA}")


def per_call_us(call, n=50):
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
    tw = S.Tweediemix(conf, base.W, te, ts, base.mask_provider, concept_num=K, lora=base.lora, use_graphs=True, n_seeds=seeds, eta=ETA,
                      noise_seeds=list(range(182, 182 + seeds)))
    tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
    tw.masks = base.masks
    at, at_next = base.alpha(501), base.alpha(481)

    def step(noise):
        tw._run_step("fusion", L.STEP_FUSION, 501, at, at_next, **(dict(step_index=25) if noise else {}))
    x0 = torch.randn(seeds, 4, base.h, base.w, device=dev)
    res = collections.defaultdict(list)
    for rnd in range(3):
        for noise in (False, True):
            tw.x_state.copy_(x0)
            for _ in range(3):
                step(noise)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step(noise)
            torch.cuda.synchronize()
            res[noise].append((time.perf_counter() - t0) * 100)
    try:
        clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
    except Exception:
        clk = None
    assert sorted(tw.graphs, key=len) == [("fusion", L.STEP_FUSION), ("fusion", L.STEP_FUSION, "eta")]
    p = tw.plan("fusion")
    print(f"fusion step, {seeds} seed(s), B = {p.B}, ms per replay (three rounds, interleaved), sclk {clk} MHz behind the timed rounds:")
    for noise, v in res.items():
        print(f"  eta {ETA if noise else 0.0:3.1f}  rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %")
    a, b = min(res[False]), min(res[True])
    print(f"  stochastic step minus deterministic step: {1000 * (b - a):+.1f} us ({100 * (b - a) / a:+.2f} % of the step)", flush=True)
    # the entry against its parent alone, out of place on this plan's eps rows, and the generator alone on as many elements
    x, out, out0 = tw.x_state.clone(), torch.empty_like(tw.x_state), torch.empty_like(tw.x_state)
    hw = base.h * base.w
    head = (x.data_ptr(), p.eps.data_ptr(), L.F32, tw.masks.data_ptr(), 0 if tw.masks.dim() == 4 else K * hw, out.data_ptr(), out0.data_ptr(), K, 4, hw,
            L.STEP_FUSION, p.B // seeds, seeds, tw.step_params.data_ptr())
    lib = L.load()
    st = lambda: torch.cuda.current_stream().cuda_stream
    parent = per_call_us(lambda: L.check(lib.tmix_fused_tweedie_step_dev(*head, st()), "tmix_fused_tweedie_step_dev"))
    noisy = per_call_us(lambda: L.check(lib.tmix_fused_tweedie_step_noise_dev(*head, None, None, tw._noise_keys.data_ptr(), base.w, 1, None, 0, 0, st()),
                                        "tmix_fused_tweedie_step_noise_dev"))
    z = torch.empty(x.numel(), device=dev)
    gen = per_call_us(lambda: ops.noise_normal(z.numel(), 0, (182, 0), 25, out=z))
    print(f"  alone, {x.numel()} elements ({seeds} x 4 x {base.h} x {base.w}), us per call (50 captured calls, best of 5 replays): tmix_fused_tweedie_step_dev "
          f"{parent:.1f}, tmix_fused_tweedie_step_noise_dev {noisy:.1f} ({noisy - parent:+.1f}), tmix_noise_normal {gen:.1f}", flush=True)
    del tw, p
    torch.cuda.empty_cache()
