"""CPU: the weight fold behind TMIX_CONV_UP2F (ops.fold_up2_weight) and the descriptor checks of the mode.

A 3x3 convolution behind a nearest x2 upsampling is, per output phase (fy, fx) = (row & 1, column & 1), a 2x2 convolution of the SOURCE image whose
weights are sums of 1, 2 or 4 of the 3x3 taps.  The fold is checked here as mathematics (fp64, against conv2d(interpolate(x))), as a layout
([4][Cout][2][2][Cin], phase-major, tap (ky, kx) of phase (fy, fx) reading source pixel (sy - 1 + fy + ky, sx - 1 + fx + kx)) and as bits (sums that bf16
holds exactly come back unchanged); the library's refusals are asked of tmix_conv_resolve_tile, which validates like the launch and launches nothing."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tweediemix_amd import lib as L, ops


def folded_conv_reference(x_nchw, wf, bias=None):
    """what TMIX_CONV_UP2F computes, written out with torch on the folded weights wf [4][Cout][2][2][Cin]: phase (fy, fx) of the output is the 2x2
    correlation of x, zero-padded by one pixel, taken at offsets (fy, fx)"""
    B, Cin, H, W = x_nchw.shape
    Cout = wf.shape[1]
    xp = F.pad(x_nchw, (1, 1, 1, 1))
    y = x_nchw.new_zeros(B, Cout, 2 * H, 2 * W)
    for fy in (0, 1):
        for fx in (0, 1):
            k = wf[2 * fy + fx].permute(0, 3, 1, 2)                       # [Cout][Cin][2][2]
            y[:, :, fy::2, fx::2] = F.conv2d(xp[:, :, fy:fy + H + 1, fx:fx + W + 1], k)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 8, 6, 5, 7), (2, 8, 6, 1, 1)])
def test_fold_equals_conv_of_the_upsampled_image_in_fp64(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    wf = ops.fold_up2_weight(w.permute(0, 2, 3, 1), dtype=None)
    assert wf.dtype == torch.float64 and tuple(wf.shape) == (4, Cout, 2, 2, Cin) and wf.is_contiguous()
    got = folded_conv_reference(x, wf)
    # fp64 rounding, elementwise: either side is a sum of n = 9 Cin products in some order, off its exact value by at most n u (|x| * |w|) with u = 2^-53
    bound = 2 * 9 * Cin * 2.0 ** -53 * F.conv2d(F.interpolate(x.abs(), scale_factor=2, mode="nearest"), w.abs(), padding=1)
    err = (got - want).abs()
    print(f"fold vs conv2d(interpolate): max |diff| = {err.max().item():.3e}, smallest bound = {bound.min().item():.3e}")
    assert torch.all(err <= bound)


def test_folded_layout_is_phase_major_with_the_documented_tap_sets():
    # one weight per tap, 3^(3 ky + kx): a sum of taps names its members
    Cout, Cin = 2, 3
    code = torch.tensor([[3.0 ** (3 * ky + kx) for kx in range(3)] for ky in range(3)], dtype=torch.float64)
    w = code.view(1, 3, 3, 1).expand(Cout, 3, 3, Cin).contiguous()
    wf = ops.fold_up2_weight(w, dtype=None)
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}                           # phase parity -> 3x3 taps merged into 2x2 tap 0 / 1
    for fy in (0, 1):
        for fx in (0, 1):
            for ky in (0, 1):
                for kx in (0, 1):
                    want = sum(3.0 ** (3 * a + b) for a in rows[fy][ky] for b in rows[fx][kx])
                    assert torch.all(wf[2 * fy + fx, :, ky, kx, :] == want), (fy, fx, ky, kx)


def test_fold_sums_in_fp32_and_rounds_once():
    g = torch.Generator().manual_seed(3)
    # small integers / 64: every sum of up to four of them is a bf16 value -> the fold of the bf16 tensor is exact, bit for bit
    w = (torch.randint(-8, 9, (6, 3, 3, 8), generator=g).float() / 64).to(torch.bfloat16)
    wf = ops.fold_up2_weight(w)
    assert wf.dtype == torch.bfloat16
    exact = ops.fold_up2_weight(w.double(), dtype=None)
    assert torch.equal(wf.double(), exact)
    # fp32 weights whose bf16 roundings would add up differently: the sum is taken first, then rounded once
    w32 = torch.randn(6, 3, 3, 8, generator=g)
    once = ops.fold_up2_weight(w32)
    assert torch.equal(once, ops.fold_up2_weight(w32, dtype=None).to(torch.bfloat16))
    assert not torch.equal(once, ops.fold_up2_weight(w32.to(torch.bfloat16)))


def test_conv_out_hw_knows_the_mode():
    assert ops.conv_out_hw(5, 7, L.CONV_UP2F) == ops.conv_out_hw(5, 7, L.CONV_UP2) == (10, 14)


def _desc(B, H, W, Cin, Cout, tile=0, **kw):
    d = L.ConvDesc()
    d.X, d.Wt, d.Y, d.bias = 0x10000, 0x20000, 0x30000, 0x40000
    d.B, d.H, d.W, d.Cin, d.Cout, d.mode, d.tile_cfg = B, H, W, Cin, Cout, L.CONV_UP2F, tile
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _resolve(d, fp8=0):
    return L.load().tmix_conv_resolve_tile(C.byref(d), fp8)


def test_descriptor_checks_of_the_folded_mode():
    # accepted: H * W is a multiple of the tile's rows; the halo tiling falls back as it does for TMIX_CONV_UP2
    assert _resolve(_desc(2, 8, 16, 64, 160, 12)) == 12
    assert _resolve(_desc(1, 16, 16, 128, 168, 14)) == 14
    assert _resolve(_desc(3, 16, 8, 192, 320, 20)) == 20
    assert _resolve(_desc(3, 16, 8, 192, 320, 26)) == 20
    assert _resolve(_desc(1, 16, 16, 128, 160, 12, col_stats_out=0x60000, batch_bias=0x70000, batch_bias_images=1)) == 12
    # H * W % BM != 0: a tile would straddle two phases
    assert _resolve(_desc(2, 8, 16, 64, 160, 14)) == L.ESHAPE            # 128 rows per phase, 256-row tile
    assert _resolve(_desc(2, 8, 12, 64, 160, 12)) == L.ESHAPE            # 96 rows, 128-row tile
    assert _resolve(_desc(2, 96, 1, 64, 160, 15)) == L.ESHAPE            # W = 1
    # no residual, no shortcut taps, no e4m3 operands
    assert _resolve(_desc(2, 8, 16, 64, 160, 12, residual=0x50000)) == L.EINVAL
    assert _resolve(_desc(2, 8, 16, 64, 160, 12, S1=0x80000, S1_channels=64)) == L.EINVAL
    assert _resolve(_desc(2, 8, 16, 128, 160, 12), fp8=1) == L.EINVAL
    # the mode behind it is still no mode
    d = _desc(2, 8, 16, 64, 160, 12); d.mode = 6
    assert _resolve(d) == L.EINVAL


def test_plan_policy_asks_for_whole_tiles_of_every_tiling(monkeypatch):
    monkeypatch.delenv("TMIX_UP2_FOLD", raising=False)
    assert ops.up2_fold_ok(32, 32) and ops.up2_fold_ok(16, 16) and ops.up2_fold_ok(128, 2)
    assert not ops.up2_fold_ok(8, 16) and not ops.up2_fold_ok(14, 24) and not ops.up2_fold_ok(256, 1)
    monkeypatch.setenv("TMIX_UP2_FOLD", "0")
    assert not ops.up2_fold_ok(32, 32)
