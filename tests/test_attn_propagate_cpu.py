"""CPU: token maps through self-attention (tmix_sattn_propagate, --attn_mask_propagate) -- the symbol and its declaration, every
argument error before a launch (the library loads without a GPU), the CLI refusals, the sampler option's validation and host-side
round logic, and that a default plan carries nothing of the feature."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    from tweediemix_amd import lib
    l = lib.load()
    assert "tmix_sattn_propagate" in lib.SIGNATURES and hasattr(l, "tmix_sattn_propagate")
    hdr = open(os.path.join(ROOT, "include", "tmix.h")).read()
    m = re.search(r"int tmix_sattn_propagate\(([^;]*)\);", hdr)
    assert m, "tmix.h does not declare tmix_sattn_propagate"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(lib.SIGNATURES["tmix_sattn_propagate"][1]) == 19
    assert params[6].startswith("const float* src") and params[7].startswith("float* dst") and params[-1] == "void* stream"
    mk = open(os.path.join(ROOT, "tweediemix_amd", "csrc", "Makefile")).read()
    assert "sattn_propagate.o" in mk                     # the shipped library is built from it


def test_sattn_propagate_argument_errors():
    from tweediemix_amd import lib
    l = lib.load()
    q, k, src, dst = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000)
    odd = C.c_void_p(0x10004)

    def call(Q=q, K=k, src=src, dst=dst, ldq=256, ldk=256, B=2, H=4, S=16, row0=1, step=2, n=1, n_tok=2, scale=0.125, out_scale=1.0):
        return l.tmix_sattn_propagate(Q, ldq, S * ldq, K, ldk, S * ldk, src, dst, B, H, S, row0, step, n, n_tok, 1, scale, out_scale, None)

    def msg():
        return l.tmix_last_error_string()
    assert call(Q=None) == lib.EINVAL and b"null" in msg()
    assert call(K=None) == lib.EINVAL and call(src=None) == lib.EINVAL and call(dst=None) == lib.EINVAL
    assert call(n_tok=0) == lib.EINVAL and b"n_tok=0 (1..32)" in msg()
    assert call(n_tok=33) == lib.EINVAL and b"n_tok=33 (1..32)" in msg()
    assert call(S=0) == lib.ESHAPE and b"S=0" in msg()
    assert call(H=0) == lib.ESHAPE and call(B=0) == lib.ESHAPE
    assert call(row0=2) == lib.ESHAPE and b"outside a batch of 2" in msg()                # rows outside the batch
    assert call(n=2) == lib.ESHAPE and call(step=0) == lib.ESHAPE and call(row0=-1) == lib.ESHAPE and call(n=0) == lib.ESHAPE
    assert call(ldq=192) == lib.ESHAPE and b"H*64=256" in msg()                           # narrower than H * 64
    assert call(ldk=192) == lib.ESHAPE
    for name in ("Q", "K", "src", "dst"):                                                 # misaligned pointers
        assert call(**{name: odd}) == lib.EALIGN and b"8-byte" in msg(), name
    assert call(ldq=258) == lib.EALIGN and call(ldk=258) == lib.EALIGN
    assert call(scale=0.0) == lib.EINVAL and b"scale" in msg()
    assert call(scale=-0.125) == lib.EINVAL and call(scale=float("nan")) == lib.EINVAL
    assert call(dst=src) == lib.EINVAL and b"overlap" in msg()                            # every output reads all of src
    assert call(dst=C.c_void_p(0x30000 + 64)) == lib.EINVAL                               # 2 * 16 floats: the ranges intersect


def test_ops_refuses_cpu_tensors():
    import torch
    from tweediemix_amd import ops
    q = torch.zeros(1, 16, 128, dtype=torch.bfloat16)
    with pytest.raises(Exception):
        ops.sattn_propagate(q, q, torch.zeros(1, 1, 16), 2)


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_prop", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def test_cli_refusals_before_the_gpu():
    fs = _cli()
    assert fs.build_parser().parse_args([]).attn_mask_propagate == 0
    base = ["--tiny", "--synthetic", "--mask_token_ids", "4+7", "--seg_concepts", "a cat+a dog"]
    with pytest.raises(SystemExit, match="mask_source attention"):                        # without --mask_source attention
        fs.main(base + ["--attn_mask_propagate", "1"])
    with pytest.raises(SystemExit, match="0..3"):                                         # N = 4
        fs.main(base + ["--mask_source", "attention", "--attn_mask_propagate", "4"])
    with pytest.raises(SystemExit, match="0..3"):
        fs.main(base + ["--mask_source", "attention", "--attn_mask_propagate", "-1"])
    fs.check_propagate_args(fs.build_parser().parse_args(["--mask_source", "attention", "--attn_mask_propagate", "3"]))
    fs.check_propagate_args(fs.build_parser().parse_args([]))                             # the default never refuses


def test_lora_cli_has_the_flag():
    """fusion_sampling_lora.py is this module with LORA switched on: the same parser plus --t_stop, the same refusals"""
    fs = _cli()
    fs.LORA = True
    opt = fs.build_parser().parse_args(["--attn_mask_propagate", "2", "--t_stop", "0.8"])
    assert opt.attn_mask_propagate == 2 and opt.t_stop == 0.8
    with pytest.raises(SystemExit, match="mask_source attention"):
        fs.main(["--tiny", "--synthetic", "--attn_mask_propagate", "2"])


def test_default_plan_carries_nothing_of_the_feature():
    """TokenPropSpec exists, the plan constructors default it to None, and a plan built without it has empty buffers: _prop_level
    then answers None at every site and no launch is added (the launch lists are compared on the GPU)"""
    import inspect
    from types import SimpleNamespace
    from tweediemix_amd import unet as U
    sp = U.TokenPropSpec(3)
    assert (sp.n_tok, sp.row0, sp.row_step, sp.n_rows, sp.levels) == (3, 1, 2, 1, None)
    for cls in (U.BlockPlan, U.UNetPlan):
        assert inspect.signature(cls.__init__).parameters["token_prop"].default is None
    stub = SimpleNamespace(prop_dst={}, h=16)
    assert U.BlockPlan._prop_level(stub, 16) is None and U.BlockPlan._prop_level(stub, 4) is None
    stub = SimpleNamespace(prop_dst={2: None}, h=16)
    assert U.BlockPlan._prop_level(stub, 4) == 2 and U.BlockPlan._prop_level(stub, 8) is None


def test_sampler_option_validation_and_rounds_on_the_host():
    """propagate outside 0..3 is refused; with propagate=0 nothing is built; with propagate=2 the rounds replay the state and timestep
    the LAST look-ahead call read, round 1 from the probe's maps and round 2 from round 1's result, prop_dst zeroed before each, the
    trajectory restored, the raw maps kept in attention_maps and the propagated ones handed to masks.attention_masks"""
    import torch
    from types import SimpleNamespace
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    W = SimpleNamespace(device=torch.device("cpu"), kind="custom")
    cfg = S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, resampling_steps=1, jumping_steps=2,
                        resolution_h=h * 8, resolution_w=w * 8)
    for bad in (4, -1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="propagate"):
            S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]], propagate=bad))
    tw0 = S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]]))
    assert tw0.attention_masks["propagate"] == 0 and tw0._x_look is None and tw0.propagated_maps is None

    tw = S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]], propagate=2, levels=(1,), threshold=0.75))
    maps = {1: torch.zeros(1, 2, 64)}
    tw.plans["probe"] = SimpleNamespace(token_maps=maps, B=2)
    prop = SimpleNamespace(prop_src={1: torch.full((1, 2, 64), 9.0)}, prop_dst={1: torch.full((1, 2, 64), 9.0)}, B=2)
    tw.plans["propagate"] = prop
    calls, seen = [], []

    def run_step(kind, mode, t, *a, **k):
        calls.append((kind, int(t)))
        if kind == "probe":                           # a partial response: one cell of concept 1, one of concept 2
            maps[1][0, 0, 1 * 8 + 2] += 1.0
            maps[1][0, 1, 6 * 8 + 2] += 1.0
        if kind == "propagate":                       # stand-in for P @ src: the cell and its right neighbour
            seen.append((tw.x_state.clone(), prop.prop_src[1].clone(), prop.prop_dst[1].clone()))
            prop.prop_dst[1] += prop.prop_src[1] + torch.roll(prop.prop_src[1], 1, dims=2)
        tw.x_state += 1.0                             # every call moves the state
    tw._run_step = run_step
    tw.init_fusion(2)
    tw.x_state.zero_()
    tw._denoise_inplace(tw.t_cond_prev)
    kinds = [c[0] for c in calls]
    assert kinds == ["plain", "probe", "probe", "propagate", "propagate"]
    assert calls[3][1] == calls[4][1] == calls[2][1]                                      # the last look-ahead call's timestep
    for x, _src, dst in seen:
        assert float(x.min()) == float(x.max()) == 2.0                                    # ... and the state it read (plain + one probe)
        assert float(dst.abs().max()) == 0.0                                              # zeroed before each round
    assert torch.equal(seen[0][1], maps[1]) and float(seen[1][1].sum()) == 2 * float(maps[1].sum())     # round 2 reads round 1's result
    assert float(tw.x_state.min()) == float(tw.x_state.max()) == 1.0                      # the trajectory is where the plain step left it
    assert float(tw.attention_maps[0][1].sum()) == 4.0                                    # raw: two jumps, two cells
    got = tw.propagated_maps[0][1]
    assert got.shape == (2, 8, 8) and float(got[0, 1, 2]) == 2.0 and float(got[0, 1, 3]) == 4.0 and float(got[0, 1, 4]) == 2.0
    want = torch.zeros(2, h, w)
    want[0, 2:4, 6:8] = 1                             # the propagated peak (cell (1, 3)), not the raw one (cell (1, 2))
    want[1, 12:14, 6:8] = 1
    assert torch.equal(tw.masks[:2, 0], want)
