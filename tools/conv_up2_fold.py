"""hot (back-to-back) launch times of the upsampler convolutions of the UNet calls (B = 4 / 2 / 16 / 32) and of the VAE decoder: the 9-tap TMIX_CONV_UP2 launch
against the folded TMIX_CONV_UP2F launch (ops.fold_up2_weight), per shape and tiling (0 = AUTO, what the VAE plan asks for).  python tools/conv_up2_fold.py"""
import os, sys, ctypes as C, torch
sys.path.insert(0, os.getcwd())
from tweediemix_amd import ops, lib as L
lib = L.load(); BF = torch.bfloat16
st = torch.cuda.current_stream().cuda_stream
def t(d, reps=10):
    for _ in range(3):
        rc = lib.tmix_conv3x3_nhwc(C.byref(d), st)
        assert rc == 0, (rc, lib.tmix_last_error_string())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): lib.tmix_conv3x3_nhwc(C.byref(d), st)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
shapes = [(4, 32, 32, 1280), (4, 64, 64, 640), (2, 32, 32, 1280), (2, 64, 64, 640), (16, 32, 32, 1280), (16, 64, 64, 640), (32, 32, 32, 1280), (32, 64, 64, 640),
          (1, 128, 128, 512), (1, 256, 256, 512), (1, 512, 512, 256)]
for (B, H, W, Cc) in shapes:
    x = torch.randn(B, H, W, Cc, device="cuda").to(BF); w32 = torch.randn(Cc, 3, 3, Cc, device="cuda") * (9 * Cc) ** -0.5
    w = w32.to(BF); wf = ops.fold_up2_weight(w32)
    out = torch.empty(B, 2 * H, 2 * W, Cc, device="cuda", dtype=BF); bias = torch.randn(Cc, device="cuda")
    cs = torch.empty(B * 4 * H * W // 32, 2, Cc, device="cuda", dtype=torch.float32) if 4 * H * W <= ops.COLSTATS_MAX_HW else None
    row = []
    for cfg in (14, 4, 2, 7, 12, 20, 0):
        u9 = t(ops.make_conv_desc(x, w, out, bias, mode=L.CONV_UP2, tile_cfg=cfg, col_stats_out=cs))
        u4 = t(ops.make_conv_desc(x, wf, out, bias, mode=L.CONV_UP2F, tile_cfg=cfg, col_stats_out=cs))
        row.append(f"c{cfg}: {u9:7.1f} -> {u4:7.1f} us")
    print(f"up2 B={B} {H}x{W} C={Cc}: " + " | ".join(row), flush=True)
