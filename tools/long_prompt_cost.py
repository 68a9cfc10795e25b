"""cost of chunked prompts (--long_prompts) in the whole step: graph replays of the plain (B = 2) and the fusion (B = 4) step at SDXL 1024^2
with (a) 77 keys as shipped, (b) 77 keys with TMIX_NO_QATTN=1 (attn2 as to_q GEMM + tmix_attn_fwd: the form every longer key count takes),
(c) 154 keys, (d) 231 keys; 10 replays each, three interleaved rounds.  Then the in-situ per-launch times of the attn2 attention launches of
(b), (c), (d) (tmix_prof_begin inside the captured step), by level -- the yardstick of DESIGN.md section 7e: is tmix_attn_fwd's general kernel
at 154 / 231 keys slower than 2x / 3x the 77-key small-key kernel by more than the run-to-run spread?

    python tools/long_prompt_cost.py [custom|lora]"""
import collections, os, sys, time, torch
sys.path.insert(0, os.getcwd())
import bench
from tweediemix_amd import lib as L, sampler as S, unet as U

kind = sys.argv[1] if len(sys.argv) > 1 else "custom"
sys.argv = ["bench.py"]
args = bench.parse()
dev = torch.device("cuda", 0)
base, (sd, con, te, ts, cfg) = bench.build_sampler(args, kind, dev, seed=0)
K = base.concept_num


def sampler(chunks, no_qattn=False):
    """a sampler on the shipped one's weights and masks whose prompt rows hold 77 * chunks keys (chunk 0: the shipped embeddings)"""
    g = torch.Generator(device="cpu").manual_seed(43)
    grow = lambda e: torch.cat([e] + [torch.randn(e.shape[0], 77, e.shape[2], generator=g) for _ in range(chunks - 1)], dim=1)
    if no_qattn:
        os.environ["TMIX_NO_QATTN"] = "1"           # read when a plan is built
    try:
        tw = S.Tweediemix(base.config, base.W, (grow(te[0]), te[1]), (grow(ts[0]), ts[1]), base.mask_provider, concept_num=K,
                          lora=base.lora, use_graphs=True)
        tw.init_fusion(int(50 * 0.2), int(50 * 0.8)) if kind == "lora" else tw.init_fusion(int(50 * 0.2))
        tw.masks = base.masks
        for k in ("plain", "fusion"):
            tw.plan(k)
    finally:
        os.environ.pop("TMIX_NO_QATTN", None)
    return tw


variants = {"a: 77 keys": base, "b: 77 keys, TMIX_NO_QATTN=1": sampler(1, True), "c: 154 keys": sampler(2), "d: 231 keys": sampler(3)}
x0 = torch.randn(1, 4, base.h, base.w, device=dev)
MODES = {"plain": L.STEP_PLAIN, "fusion": L.STEP_FUSION}
res = collections.defaultdict(list)
for rnd in range(3):
    for name, tw in variants.items():
        for k, mode in MODES.items():
            step = lambda: tw._run_step(k, mode, 501, tw.alpha(501), tw.alpha(351))
            tw.x_state.copy_(x0)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            res[(name, k)].append((time.perf_counter() - t0) * 100)
import socket
try:
    clk = torch.cuda.clock_rate(dev)                  # sampled right behind the last timed replays
except Exception:
    clk = None
print(f"box {socket.gethostname()}, {torch.cuda.get_device_name(dev)}, sclk {clk} MHz behind the timed rounds")
print(f"whole step, {kind}, ms per replay (three rounds, interleaved):")
for (name, k), v in res.items():
    names = [getattr(fn, "__name__", "") for fn, _a in variants[name].plan(k).ops]
    print(f"  {name:30s} {k:6s} B={variants[name].plan(k).B} launches={len(names)} one-launch attn2={names.count('tmix_gemm_q_cross_attn')} "
          f"rounds {[round(x, 3) for x in v]} min {min(v):.3f} spread {100 * (max(v) - min(v)) / min(v):.1f} %", flush=True)


def attn2_launch_us(tw, k, mode, Lk, reps=5):
    """{(B, H, Sq): [median over the step's launches of that shape, per replay]} of the attn2 tmix_attn_fwd launches in the captured step"""
    lib = L.load()
    meta = tw.plan(k).issued_meta()
    n = len(meta)
    slots = torch.zeros(n + 64, 8, dtype=torch.int64, device=dev)
    L.check(lib.tmix_prof_begin(slots.data_ptr(), n + 64, 0), "tmix_prof_begin")
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tw._enqueue_step(k, mode)
    finally:
        used = lib.tmix_prof_end()
    assert used == n, (used, n)
    out = collections.defaultdict(list)
    for r in range(reps + 1):
        tw.x_state.copy_(x0)
        slots.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if r == 0:
            continue
        sl = slots.cpu().numpy().astype("uint64")
        per = collections.defaultdict(list)
        for (cls, _fl, key), s in zip(meta, sl):
            if cls == "attn" and key[4] == Lk:
                per[key[1:4]].append((int(s[1]) - int(s[0])) * 1e-2)        # 100 MHz ticks -> us
        for shape, v in per.items():
            out[shape].append((sorted(v)[len(v) // 2], len(v)))
    return out


print("attn2 attention launches in situ (us per launch: median of the step's launches of a shape, then min / max over 5 replays):")
table = {}
for name, tw in list(variants.items())[1:]:
    Lk = tw.text_embeds[0].shape[1]
    for k, mode in MODES.items():
        for shape, v in sorted(attn2_launch_us(tw, k, mode, Lk).items()):
            us = [a for a, _n in v]
            table[(Lk, k, shape)] = (min(us), max(us))
            print(f"  {name:30s} {k:6s} (B, H, Sq)={shape} n={v[0][1]:3d}  {min(us):7.2f} .. {max(us):7.2f} us", flush=True)
print("general kernel against the small-key kernel scaled by the key count (ratio > 1: the general kernel costs more than c x 77 keys):")
for (Lk, k, shape), (lo, hi) in table.items():
    if Lk == 77:
        continue
    b = table.get((77, k, shape))
    if b:
        c = Lk // 77
        print(f"  {Lk} keys {k:6s} {shape}: {lo:7.2f} us vs {c} x {b[0]:.2f} = {c * b[0]:7.2f} us  ratio {lo / (c * b[0]):.2f}", flush=True)
