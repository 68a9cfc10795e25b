"""GPU: TMIX_CONV_UP2F -- the upsampler convolution as four 2x2 phase convolutions of the source grid -- against the 9-tap TMIX_CONV_UP2 launch it
replaces and against an fp64 CPU reference, on the smallest shapes at which the tiles still meet every edge:

    B  H x W   Cin  Cout   what it exercises
    2  8 x 16   64   160   one 128-row tile per (image, phase), one channel chunk
    1  16 x 16 128   168   a 256-row tile, two chunks, ragged N
    3  16 x 8  192   320   more than one image in a column of tiles

each under every tiling whose tile height divides H * W (a tile must not straddle two phases; the others are refused, see the last test).
References are computed once per shape and shared.  What is asserted, per (shape, tiling):
  (a) weights that are small integers / 64 fold exactly; with inputs that are small integers / 8 every product and every partial sum is an fp32 value, so
      the two launches may differ by the order of an exact sum only: the outputs agree within one bf16 ulp (adjacent values), and nothing outside Y is written;
  (b) random weights, against conv2d(interpolate(x), w) in fp64, elementwise and for every element:
      |err| <= 2^-8 (|x| * |W_folded|) + 2^-8 |y| + 1e-5 (|x| * |W|)   (bf16 rounding of the folded weights, of the stored output, fp32 accumulation);
  (c) col_stats_out, summed per image and channel, equals the sums of the stored output and of its squares to fp32 accumulation accuracy;
  (d) the bias is applied (it is part of (b)'s reference), and a second image poisoned with 1e4 leaves the first image's output bits alone."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from layout_frames import dense_guarded
from test_up2_fold_cpu import folded_conv_reference

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = [(2, 8, 16, 64, 160), (1, 16, 16, 128, 168), (3, 16, 8, 192, 320)]
TILE_ROWS = {1: 128, 2: 256, 3: 128, 4: 256, 5: 256, 7: 128, 12: 128, 13: 64, 14: 256, 15: 32, 20: 128}      # the tilings with a convolution form
CASES = [(s, cfg) for s in SHAPES for cfg in sorted(TILE_ROWS) if (s[1] * s[2]) % TILE_ROWS[cfg] == 0]
_REF = {}


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else f"tile{v}"


def reference(shape):
    """inputs and fp64 references of one shape, made once (CPU) and never modified"""
    if shape not in _REF:
        from tweediemix_amd import ops
        B, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(1000 + H * W + Cin)
        r = {}
        # (a): x = integers / 8, w = integers / 64 -- exact in bf16, and so is every fold
        r["x_int"] = (torch.randint(-16, 17, (B, H, W, Cin), generator=g).float() / 8).to(BF)
        r["w_int"] = (torch.randint(-8, 9, (Cout, 3, 3, Cin), generator=g).float() / 64).to(BF)
        # (b): the checkpoint's fp32 weights, activations as a bf16 tensor
        r["x"] = torch.randn(B, H, W, Cin, generator=g).to(BF)
        r["w"] = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5
        r["bias"] = torch.randn(Cout, generator=g)
        xn, wn = r["x"].double().permute(0, 3, 1, 2), r["w"].double().permute(0, 3, 1, 2)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        r["y"] = (F.conv2d(up(xn), wn, r["bias"].double(), padding=1)).permute(0, 2, 3, 1).contiguous()
        r["abs_xw"] = F.conv2d(up(xn.abs()), wn.abs(), padding=1).permute(0, 2, 3, 1).contiguous()
        r["wf"] = ops.fold_up2_weight(r["w"])                   # bf16 [4][Cout][2][2][Cin], rounded once
        r["abs_xwf"] = folded_conv_reference(xn.abs(), r["wf"].double().abs()).permute(0, 2, 3, 1).contiguous()
        _REF[shape] = r
    return _REF[shape]


def _st():
    return torch.cuda.current_stream().cuda_stream


def launch(x, w, bias, mode, cfg, colstats=False, expect=0):
    """one tmix_conv3x3_nhwc launch into a guarded dense Y; returns (Y frame, col stats or None)"""
    from tweediemix_amd import lib as L, ops
    B, H, W, _ = x.shape
    Cout = w.shape[1] if mode == L.CONV_UP2F else w.shape[0]
    y = dense_guarded((B, 4 * H * W, Cout), BF, device="cuda", name="Y")
    cs = torch.full((B * 4 * H * W // 32, 2, Cout), float("nan"), device="cuda", dtype=F32) if colstats else None
    d = ops.make_conv_desc(x, w, y.view.view(B, 2 * H, 2 * W, Cout), bias, mode=mode, tile_cfg=cfg, col_stats_out=cs)
    rc = L.load().tmix_conv3x3_nhwc(C.byref(d), _st())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.load().tmix_last_error_string())
    return y, cs, d


def ordered(t):
    """bf16 values as integers in which adjacent representable values differ by one"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("shape,cfg", CASES, ids=_ids)
def test_folded_launch_against_the_nine_tap_launch_and_fp64(shape, cfg):
    from tweediemix_amd import lib as L, ops
    B, H, W, Cin, Cout = shape
    r = reference(shape)
    bias = r["bias"].cuda()
    # ---- (a) exactly representable folds, exactly summable inputs
    x, w = r["x_int"].cuda(), r["w_int"].cuda()
    wf = ops.fold_up2_weight(w)
    assert torch.equal(wf.double(), ops.fold_up2_weight(w.double(), dtype=None))
    y9, _, _ = launch(x, w, bias, L.CONV_UP2, cfg)
    y4, _, d = launch(x, wf, bias, L.CONV_UP2F, cfg)
    assert ops.conv_runs_as(d, cfg) == cfg                       # the tiling under test is the kernel that ran
    y4.assert_untouched()
    y4.assert_all_written()
    ulps = (ordered(y4.view) - ordered(y9.view)).abs().max().item()
    print(f"{shape} tile {cfg}: (a) folded vs 9-tap launch: {ulps} bf16 ulp")
    assert ulps <= 1
    # ---- (b) random weights against fp64, every element; (c) column statistics; (d) bias
    x = r["x"].cuda()
    yf, cs, _ = launch(x, r["wf"].cuda(), bias, L.CONV_UP2F, cfg, colstats=True)
    yf.assert_untouched()
    yf.assert_all_written()
    got = yf.view.view(B, 2 * H, 2 * W, Cout).cpu()
    err = (got.double() - r["y"]).abs()
    bound = 2.0 ** -8 * r["abs_xwf"] + 2.0 ** -8 * r["y"].abs() + 1e-5 * r["abs_xw"]
    ratio = (err / bound).max().item()
    print(f"{shape} tile {cfg}: (b) max |err| = {err.max().item():.3e}, max |err| / bound = {ratio:.3f} over {err.numel()} elements")
    assert torch.all(err <= bound)
    # (c): the kernel adds 32 rows per block in fp32 (each partial off by at most 32 u of its sum of magnitudes, u = 2^-24); the blocks of an image are
    # added here in fp64.  The launch's row order is phase-major inside an image, so the blocks of an image are still rows [b * 4HW / 32, (b + 1) * 4HW / 32)
    per_img = cs.view(B, 4 * H * W // 32, 2, Cout).double().sum(1).cpu()
    ys = got.double().reshape(B, -1, Cout)
    s1, s2, sa = ys.sum(1), (ys * ys).sum(1), ys.abs().sum(1)
    e1, e2 = (per_img[:, 0] - s1).abs(), (per_img[:, 1] - s2).abs()
    print(f"{shape} tile {cfg}: (c) column sums off by {e1.max().item():.3e} / squares {e2.max().item():.3e}")
    assert torch.all(e1 <= 32 * 2.0 ** -24 * sa + 1e-30) and torch.all(e2 <= 32 * 2.0 ** -24 * s2 + 1e-30)
    # (d): the second image poisoned
    if B > 1:
        xp = x.clone()
        xp[1] = 1e4
        yp, _, _ = launch(xp, r["wf"].cuda(), bias, L.CONV_UP2F, cfg)
        assert torch.equal(yp.view[0].view(torch.int16), yf.view[0].view(torch.int16))
        assert torch.isfinite(yp.view[1].float()).all() and yp.view[1].float().abs().max() > 1e3


def test_refusals_launch_nothing():
    from tweediemix_amd import lib as L, ops
    lib = L.load()

    def refused(shape, code, tile_cfg, fp8=False, **fields):
        B, H, W, Cin, Cout = shape
        r = reference(shape)
        x, wf, bias = r["x"].cuda(), r["wf"].cuda(), r["bias"].cuda()
        y = dense_guarded((B, 4 * H * W, Cout), BF, device="cuda", name="Y")
        d = ops.make_conv_desc(x, wf, y.view.view(B, 2 * H, 2 * W, Cout), bias, mode=L.CONV_UP2F, tile_cfg=tile_cfg)
        keep = torch.zeros(B, 2 * H, 2 * W, max(Cin, Cout), device="cuda", dtype=BF)      # what a residual / shortcut pointer names
        for k, v in fields.items():
            setattr(d, k, keep.data_ptr() if v is None else v)
        if fp8:
            sc = torch.full((B * H * W * Cin // 32 + Cout,), 127, device="cuda", dtype=torch.uint8)
            rc = lib.tmix_conv3x3_nhwc_fp8(C.byref(d), sc.data_ptr(), sc.data_ptr(), _st())
        else:
            rc = lib.tmix_conv3x3_nhwc(C.byref(d), _st())
        torch.cuda.synchronize()
        assert rc == code, (rc, lib.tmix_last_error_string())
        y.assert_untouched()
        assert bool((y.bits == y.bits[0]).all())                  # nothing inside the view either: the whole allocation still holds the sentinel

    refused(SHAPES[0], L.ESHAPE, 14)                              # H * W = 128 rows per phase under a 256-row tile
    refused(SHAPES[0], L.EINVAL, 12, residual=None)
    refused(SHAPES[0], L.EINVAL, 12, S1=None, S1_channels=64)
    refused(SHAPES[1], L.EINVAL, 12, fp8=True)                    # Cin = 128: an e4m3 convolution of the other modes would accept the shape


def test_tiny_unet_plan_with_and_without_the_fold(monkeypatch):
    """the tiny UNet at B = 4 on a 32 x 32 latent: its second upsampler (128 channels, 16 x 16 -> 32 x 32) folds, the first (8 x 8: 64 pixels, less than the
    tallest tile) keeps the 9-tap launch.  Both plans stay under the bound of every whole-UNet test (rel L2 <= 2e-2 against the fp32 oracle)."""
    from test_unet_gpu import make, rel_l2
    from tweediemix_amd import lib as L
    modes = lambda plan: sorted(d.mode for _i, kind, d in plan._tunable if kind == "conv" and d.mode in (L.CONV_UP2, L.CONV_UP2F))
    monkeypatch.delenv("TMIX_UP2_FOLD", raising=False)
    orc, plan, x, ehs, pooled, time_ids = make("custom", 4, 32, 32, True)
    assert modes(plan) == [L.CONV_UP2, L.CONV_UP2F]
    eps = plan(x.cuda(), 500).float().cpu()
    monkeypatch.setenv("TMIX_UP2_FOLD", "0")
    _orc, plan0, *_ = make("custom", 4, 32, 32, True)
    assert modes(plan0) == [L.CONV_UP2, L.CONV_UP2]
    eps0 = plan0(x.cuda(), 500).float().cpu()
    assert plan.flops < plan0.flops                               # the flops performed
    ref = orc.forward(x, 500, ehs, pooled, time_ids, routed=True)
    r, r0 = rel_l2(eps, ref), rel_l2(eps0, ref)
    print(f"tiny UNet B=4 32x32: rel_l2 vs oracle folded {r:.4g}, 9-tap {r0:.4g}, ratio {r / r0:.4f}; folded vs 9-tap {rel_l2(eps, eps0):.3g}")
    assert torch.isfinite(eps).all() and r <= 2e-2 and r0 <= 2e-2
