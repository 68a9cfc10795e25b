"""Wide canvases: the layout of the overlapping windows a canvas is sampled as, and the torch slicing around them.

A canvas larger than the trained window is sampled as windows of the trained size that share every UNet launch like co-batched
seeds; tmix_window_consensus reconciles them after every step (sampler.Tweediemix(canvas=...)).  Cropping
windows out of a canvas and assembling a canvas from reconciled windows happen outside the step and stay torch slicing.
"""
from __future__ import annotations

import torch


def axis_offsets(c: int, s: int, o: int):
    """window offsets along one axis: canvas size c, window size s, minimum overlap o (all in the same unit, c >= s, 0 <= o < s).
    c == s: one window at 0; otherwise n = ceil((c - o) / (s - o)) windows at off_i = (i * (c - s)) // (n - 1): the first at 0, the
    last flush with the far edge, neighbours overlapping by at least o."""
    c, s, o = int(c), int(s), int(o)
    if not (c >= s >= 1 and 0 <= o < s):
        raise ValueError(f"window layout: canvas {c}, window {s}, overlap {o}: needs canvas >= window >= 1 and 0 <= overlap < window")
    if c == s:
        return [0]
    n = -((c - o) // -(s - o))
    return [(i * (c - s)) // (n - 1) for i in range(n)]


def window_layout(canvas_h: int, canvas_w: int, h: int, w: int, overlap: int):
    """[(oy, ox), ...] of the windows of h x w on a canvas_h x canvas_w canvas, row-major (y outer, x inner).  The overlap is capped
    per axis below the window size only by the caller: it must be smaller than both h and w."""
    ys, xs = axis_offsets(canvas_h, h, overlap), axis_offsets(canvas_w, w, overlap)
    return [(oy, ox) for oy in ys for ox in xs]


def tent_weight(h: int, w: int, device="cpu"):
    """[h, w] fp32 separable tent t(i) = min(i + 1, s - i) per axis: small exact integers, largest in the window's middle"""
    ty = torch.minimum(torch.arange(h) + 1, h - torch.arange(h)).to(torch.float32)
    tx = torch.minimum(torch.arange(w) + 1, w - torch.arange(w)).to(torch.float32)
    return (ty[:, None] * tx[None, :]).contiguous().to(device)


def crop_windows(canvas, offsets, h: int, w: int):
    """canvas [G, ..., ch, cw] -> [G * n_win, ..., h, w], group-major (b = group * n_win + window)"""
    wins = torch.stack([canvas[..., oy:oy + h, ox:ox + w] for oy, ox in offsets], dim=1)
    return wins.reshape(-1, *wins.shape[2:]).contiguous()


def assemble(windows, offsets, canvas_h: int, canvas_w: int):
    """windows [G * n_win, C, h, w] (group-major, reconciled: equal wherever they overlap) -> canvas [G, C, canvas_h, canvas_w];
    a later window overwrites an earlier one on their overlap, which changes nothing once they agree"""
    n = len(offsets)
    G, (C, h, w) = windows.shape[0] // n, windows.shape[1:]
    wins = windows.reshape(G, n, C, h, w)
    out = torch.empty(G, C, canvas_h, canvas_w, device=windows.device, dtype=windows.dtype)
    for i, (oy, ox) in enumerate(offsets):
        out[:, :, oy:oy + h, ox:ox + w] = wins[:, i]
    return out
