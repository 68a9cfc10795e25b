"""canonical launch log of a plan, with hashes: what a refactor of the plan recorder must leave unchanged.

python tools/plan_log.py [--full] [--dump DIR] [name ...]

For every plan: one line `<name> ops=<n> log=<sha256 of the canonical text> out=<sha256 of the output bytes of one call on a
fixed-seed input>`; --dump writes the canonical texts to DIR/<name>.txt (diff two of them to find the launch that moved).  The text
is made from `plan.ops` alone -- per op the entry point and its arguments; addresses print as p<k>, k = order of first appearance in
the log, descriptors field by field, ctypes arrays by element, everything else by value -- so the same file runs against an older
checkout of the package (PYTHONPATH=<dir holding that tweediemix_amd> TMIX_LIB=<the one built library>).

The default set is the seven small plans of tests/test_plan_gpu.py (autotune=False: no tile timing can differ between two runs).
--full adds the four SDXL-size call kinds bench.py times (synthetic weights, as bench.py builds them) and refuses to print unless
every one of them follows the shipped tile table."""
import argparse
import ctypes as C
import functools
import hashlib
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # behind PYTHONPATH: another checkout's package wins
from tweediemix_amd import lib as L  # noqa: E402


# ------------------------------------------------------------------------------------------------ canonical text
def canonical(ops):
    """the text of an op list [(fn, args)] (PlanGroup.ops / I2VVideoPlan.ops: the chains one after the other)"""
    seen = {}

    def ptr(v):
        v = v.value if isinstance(v, C.c_void_p) else v
        return "null" if not v else f"p{seen.setdefault(int(v), len(seen))}"

    def val(v):
        return "[" + " ".join(repr(x) for x in v) + "]" if isinstance(v, C.Array) else repr(v)

    def struct(d):
        return "{" + " ".join(f"{n}={ptr(getattr(d, n)) if t is L.vp else val(getattr(d, n))}" for n, t in d._fields_) + "}"

    lines = []
    for fn, args in ops:
        name = fn.__name__
        if not args and hasattr(fn, "per_frame"):                  # i2vgen._Inject: a Python op around tmix_frame_inject
            lines.append(f"{name} per_frame={fn.per_frame} hard={fn.hard}")
            continue
        types = L.SIGNATURES[name][1]
        assert len(args) == len(types) - 1, (name, len(args), len(types))          # (the stream is appended when the op runs)
        out = []
        for a, t in zip(args, types):
            if isinstance(a, C.Array):
                out.append(val(a))
            elif hasattr(a, "_obj"):                               # C.byref(descriptor)
                out.append(struct(a._obj))
            elif t is L.vp:
                out.append(ptr(a))
            else:
                out.append(val(a))
        lines.append(name + " " + " ".join(out))
    return "\n".join(lines) + "\n"


def sha(b):
    return hashlib.sha256(b).hexdigest()


def out_hash(t):
    torch.cuda.synchronize()
    return sha(t.detach().contiguous().cpu().numpy().tobytes())


# ------------------------------------------------------------------------------------------------ the small plans
@functools.lru_cache(maxsize=None)
def _unet_weights(lora_mode):
    """tiny UNet with three synthetic LoRA concepts, as tests/test_unet_gpu.py::make builds it"""
    from tweediemix_amd import unet as U, weights as Wt
    sd = Wt.synthetic_state_dict(U.TINY, seed=1234, nontrivial=True)
    return U.UNetWeights(U.TINY, sd, "cuda", ("lora", Wt.synthetic_concepts(U.TINY, "lora", 3)), lora_mode=lora_mode)


def _unet(B, h, w, routed, lora_mode="merged", **kw):
    from tweediemix_amd import unet as U
    W, cfg = _unet_weights(lora_mode), U.TINY
    g = torch.Generator().manual_seed(0)
    ehs = torch.randn(B, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float()
    pooled = torch.randn(B, cfg.pooled_dim, generator=g)
    tid = torch.tensor([[h * 8, w * 8, 0, 0, h * 8, w * 8]] * B, dtype=torch.float32)
    kv = U.KVCache(W, ehs, list(range(B)) if routed else [0] * B)
    plan = U.UNetPlan(W, B, h, w, kv, pooled, tid, routed=routed, autotune=False, **kw)
    x = torch.randn(1, 4, h, w, generator=g).repeat(B, 1, 1, 1).cuda()
    return plan, lambda: plan(x, 500)


def _probe():
    from tweediemix_amd import unet as U
    return _unet(2, 16, 16, False, token_maps=U.TokenMapSpec((1, 4, 7), row0=1, row_step=2, n_rows=1))


def _i2v():
    """i2vgen.TINY as tests/test_i2vgen_gpu.py runs it: 2 clips of 16 frames of 16 x 8"""
    from oracle import i2vgen_oracle as IO
    from tweediemix_amd import i2vgen as I
    B, Fr, H, Wd, Lk = 2, 16, 16, 8, 13
    sd = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v) for k, v in IO.synthetic_state_dict(IO.TINY).items()}
    g = torch.Generator().manual_seed(0)
    il, emb, ehs = torch.randn(B, 4, Fr, H, Wd, generator=g), torch.randn(B, IO.TINY.cross_dim, generator=g), torch.randn(B, Lk, IO.TINY.cross_dim, generator=g)
    sample = torch.randn(B, 4, Fr, H, Wd, generator=g)
    Wt = I.I2VWeights(I.TINY, sd)
    plan = I.I2VPlan(Wt, B, Fr, H, Wd, *I.conditioning(Wt, torch.tensor([8.0] * B), il, emb, ehs), autotune=False)
    return plan, lambda: plan(sample, 981)


def _vae():
    from tweediemix_amd import vae as V
    plan = V.VAEDecoderPlan(V.TINY, V.synthetic_state_dict(V.TINY, nontrivial=True), 1, 16, 16, 1 / 0.13025)
    z = (torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(0)) * 0.13025 * 3).cuda()
    return plan, lambda: plan(z)


# name -> builder of (plan, call): call() runs the plan once on its fixed input and returns the output tensor
SMALL = {
    "unet_lora_routed_16": lambda: _unet(4, 16, 16, True),
    "unet_lora_routed_32": lambda: _unet(4, 32, 32, True),                # both GroupNorm forms occur
    "unet_fp8_16": lambda: _unet(4, 16, 16, True, fp8=True),
    "unet_probe_16": _probe,
    "unet_lowrank_16": lambda: _unet(4, 16, 16, True, lora_mode="lowrank"),
    "i2v_tiny": _i2v,
    "vae_tiny_decoder": _vae,
}


# ------------------------------------------------------------------------------------------------ the SDXL-size call kinds
def full_plans():
    """[(name, plan, call)] of the fusion, fusion_base, start and plain calls of the LoRA sampler at 1024^2, one seed, one chain"""
    import bench
    from tweediemix_amd import unet as U
    tw, _parts = bench.build_sampler(bench.parse(["--no-video"]), "lora", torch.device("cuda", 0), seed=0)
    x = torch.randn(1, 4, tw.h, tw.w, generator=torch.Generator().manual_seed(1000)).cuda()
    out = []
    for kind in ("fusion", "fusion_base", "start", "plain"):
        plan = tw.plan(kind)
        ok, bad = U.tilings_follow_table(plan)
        if not ok:
            raise SystemExit(f"{kind}: the plan does not follow the shipped tile table ({bad[:3]}): its tilings were timed on this box, logs of two runs may differ")
        out.append(("sdxl_" + kind, plan, functools.partial(tw._unet, kind, x, 601)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("names", nargs="*", help=f"small plans to log (default: all of {', '.join(SMALL)})")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--dump", metavar="DIR")
    a = ap.parse_args()
    print("package:", os.path.dirname(os.path.abspath(L.__file__)), file=sys.stderr)
    todo = [(n, *SMALL[n]()) for n in (a.names or SMALL)]
    lines = []
    for name, plan, call in todo + (full_plans() if a.full else []):
        text = canonical(plan.ops)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, name + ".txt"), "w") as f:
                f.write(text)
        lines.append(f"{name} ops={len(plan.ops)} log={sha(text.encode())} out={out_hash(call())}")
    print("\n".join(lines))          # (all at once: --full must not print part of a set it then refuses)


if __name__ == "__main__":
    main()
