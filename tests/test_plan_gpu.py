"""GPU: a plan's op_meta holds an entry for exactly the launches the library stamps under tmix_prof_begin.  Each case builds one small
plan (the smallest shapes at which every emitter family appears, autotune=False), runs it once eagerly inside a profiler bracket and
compares the number of slots the library dealt out with len(plan.issued_meta()): one stamped launch without its entry -- or one
entry too many -- would shift every later stamp of bench.py's in-situ profile.  The plans are those tools/plan_log.py logs."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("plan_log", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "plan_log.py"))
plan_log = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_log)

# what each case must contain for the count to mean something: entry points that occur in its op list
EXPECT = {
    "unet_lora_routed_16": ("tmix_gemm_bf16", "tmix_conv3x3_nhwc", "tmix_attn_fwd_ws", "tmix_groupnorm_nhwc_pre", "tmix_gemm_prefetch_next"),
    "unet_lora_routed_32": ("tmix_groupnorm_nhwc", "tmix_groupnorm_nhwc_pre"),
    "unet_fp8_16": ("tmix_gemm_fp8", "tmix_conv3x3_nhwc_fp8", "tmix_groupnorm_nhwc_pre_f8", "tmix_attn_fwd_f8_ws"),
    "unet_probe_16": ("tmix_xattn_token_maps", "tmix_attn_fwd_ws"),
    "unet_lowrank_16": ("tmix_lora_down", "tmix_gemm_bf16"),
    "i2v_tiny": ("tmix_temporal_attn", "tmix_frame_inject", "tmix_conv3x3_nhwc", "tmix_groupnorm_nhwc"),
    "vae_tiny_decoder": ("tmix_conv_in_pre", "tmix_softmax_rows", "tmix_gemm_bf16", "tmix_conv3x3_nhwc", "tmix_groupnorm_nhwc"),
}


@pytest.mark.parametrize("name", list(plan_log.SMALL))
def test_profiler_slots_taken_equal_the_plans_issued_meta(name):
    from tweediemix_amd import lib as L, plan as P
    lib = L.load()
    plan, call = plan_log.SMALL[name]()
    names = [fn.__name__ for fn, _a in plan.ops]
    assert all(n in names for n in EXPECT[name]), [n for n in EXPECT[name] if n not in names]
    meta = plan.issued_meta()
    assert len(meta) == sum(n in P.STAMPED for n in names) > 0
    cap = len(meta) + 64                            # spare slots: a launch without an entry shows up as used > len(meta)
    slots = torch.zeros(cap, 8, dtype=torch.int64, device="cuda")
    L.check(lib.tmix_prof_begin(slots.data_ptr(), cap, 0), "tmix_prof_begin")
    try:
        out = call()
    finally:
        used = lib.tmix_prof_end()
    torch.cuda.synchronize()
    assert used == len(meta), (used, len(meta))
    assert torch.isfinite(out).all()
