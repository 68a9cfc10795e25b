"""Blend-mask preparation (host side, once per image).

preprocess_mask / build_masks follow fusion_generation/fusion_sampling.py:81-89 and :461-469: the
segmentation side-car's '<concept>.jpg' (8-bit grey) -> /255 -> threshold 0.5 -> nearest resize to the
latent grid -> masks = [fg_1..fg_{K-1}, clamp(1 - sum fg, 0)].  random_rectangle_masks is the synthetic
stand-in for the side-car used by the benchmark (run_expand.py:50-51 emits bounding rectangles).  attention_masks is the
in-process mask source: cross-attention token maps of the look-ahead (UNetPlan token_maps) through the side-car's own
post-processing (expand_masks), or, with shape="free", as the object's own outline: largest component, holes filled, overlaps resolved towards the
highest score (tmix_attn_shapes; attn_shapes_reference / mask_label_reference are the numpy restatements the kernels equal).  soft_masks / soft_region turn the {0, 1} masks of any of these sources into blend weights from the distance
to each region's border (dilated, feathered, optionally normalised: tmix_mask_edt + tmix_soft_masks); soft_masks_reference
is their numpy restatement, which the kernels equal bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch


def preprocess_mask(mask, h: int, w: int, device="cuda") -> torch.Tensor:
    """mask: path or uint8 array [H,W]. Returns [1,1,h,w] fp32 {0,1} on `device`."""
    if isinstance(mask, (str, bytes)):
        from PIL import Image
        mask = np.array(Image.open(mask).convert("L"))
    m = np.asarray(mask).astype(np.float32) / np.float32(255.0)
    m = (m >= 0.5).astype(np.float32)
    H, W = m.shape
    ys = np.minimum(np.floor(np.arange(h, dtype=np.float32) * np.float32(H / h)).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(w, dtype=np.float32) * np.float32(W / w)).astype(np.int64), W - 1)
    return torch.from_numpy(np.ascontiguousarray(m[ys][:, xs]))[None, None].to(device)


def build_masks(fg_sources, h: int, w: int, device="cuda") -> torch.Tensor:
    """[K,1,h,w]: foreground masks then background = clamp(1 - sum fg, min 0) (NOT renormalised)."""
    fg = torch.cat([preprocess_mask(s, h, w, device) for s in fg_sources])
    bg = 1 - torch.sum(fg, dim=0, keepdim=True)
    bg[bg < 0] = 0
    return torch.cat([fg, bg]).contiguous()


EDT_NONE = 1 << 30          # TMIX_EDT_NONE (include/tmix.h): squared distance where the mask has no set (clear) pixel at all


def _edt_brute(sel):
    """bool [h,w] -> int32 [h,w]: squared Euclidean distance to the nearest True pixel, by the minimum over all of them (EDT_NONE without one)"""
    h, w = sel.shape
    qy, qx = np.nonzero(sel)
    if qy.size == 0:
        return np.full((h, w), EDT_NONE, np.int32)
    out = np.empty((h, w), np.int32)
    xs = np.arange(w, dtype=np.int64)
    for y in range(h):                                   # row by row: [w, n_set] at a time
        out[y] = ((y - qy)[None, :] ** 2 + (xs[:, None] - qx[None, :]) ** 2).min(axis=1)
    return out


def _edt_separable(sel):
    """the same distances by the two exact passes the kernel makes: along y to the nearest True pixel of the column (capped at 2^14 = none), then
    min over x' of (x - x')^2 + g[x']^2 along the row.  Integer minima: equal to _edt_brute on every mask (tests/test_soft_masks_cpu.py)."""
    h, w = sel.shape
    cap = 1 << 14
    ys = np.arange(h, dtype=np.int64)
    g = np.empty((h, w), np.int64)
    for x in range(w):                                   # column by column: [h, h] at a time
        g[:, x] = np.where(sel[None, :, x], np.abs(ys[:, None] - ys[None, :]), cap).min(axis=1)
    g2 = np.where(g >= cap, EDT_NONE, g * g)
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    out = np.empty((h, w), np.int64)
    for y in range(h):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return np.minimum(out, EDT_NONE).astype(np.int32)


def mask_edt_reference(mask, brute=None):
    """numpy restatement of tmix_mask_edt: mask [..., h, w] (set where >= 0.5) -> (d_set, d_clear) int32 of the same shape.  Brute force up to
    64 x 64, the separable form above (brute=True / False forces one)."""
    m = np.asarray(mask, np.float32) >= np.float32(0.5)
    h, w = m.shape[-2:]
    if brute is None:
        brute = h * w <= 64 * 64
    f = _edt_brute if brute else _edt_separable
    flat = m.reshape(-1, h, w)
    d_set = np.stack([f(b) for b in flat]).reshape(m.shape)
    d_clear = np.stack([f(~b) for b in flat]).reshape(m.shape)
    return d_set, d_clear


def soft_u_reference(d_set, d_clear, feather, dilate):
    """u of DESIGN.md 7g from the squared distances, every op one fp32 op: signed distance to the border (midway between pixel centres),
    moved by the dilation, ramped over the feather width"""
    NF = np.float32
    f, r = NF(feather), NF(dilate)
    if not (np.isfinite(f) and f >= 0 and np.isfinite(r)):
        raise ValueError(f"soft masks: feather={feather} (finite, >= 0) dilate={dilate} (finite)")
    s = np.where(d_set == 0, -(np.sqrt(d_clear.astype(NF)) - NF(0.5)), np.sqrt(d_set.astype(NF)) - NF(0.5)).astype(NF)
    sp = (s - r).astype(NF)
    if f > 0:
        u = np.minimum(np.maximum((NF(0.5) - (sp / f).astype(NF)).astype(NF), NF(0)), NF(1))
    else:
        u = (sp < 0).astype(NF)
    assert u.dtype == NF
    return u


def soft_weights_reference(d_set, d_clear, feather=0.0, dilate=0.0, normalize=False):
    """numpy restatement of tmix_soft_masks: squared distances [n,K-1,h,w] int32 -> the K blend weights [n,K,h,w] fp32 (t summed in ascending
    concept order, every op one fp32 op)"""
    NF = np.float32
    u = soft_u_reference(d_set, d_clear, feather, dilate)
    t = np.zeros(u[:, 0].shape, NF)
    for k in range(u.shape[1]):
        t = (t + u[:, k]).astype(NF)
    if normalize:
        over = t > 1
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(over[:, None], (u / t[:, None]).astype(NF), u)
        bg = np.where(over, NF(0), (NF(1) - t).astype(NF))
    else:
        w, bg = u, np.maximum((NF(1) - t).astype(NF), NF(0))
    return np.concatenate([w, bg[:, None]], axis=1).astype(NF)


def soft_masks_reference(fg, feather=0.0, dilate=0.0, normalize=False, brute=None):
    """numpy restatement of soft_masks (tmix_mask_edt + tmix_soft_masks), compared with the kernels by equality: fg [K-1,h,w] or [n,K-1,h,w]
    -> [K,1,h,w] or [n,K,1,h,w] fp32"""
    fg = np.asarray(fg, np.float32)
    single = fg.ndim == 3
    if single:
        fg = fg[None]
    d_set, d_clear = mask_edt_reference(fg, brute)
    out = soft_weights_reference(d_set, d_clear, feather, dilate, normalize)[:, :, None]
    return out[0] if single else out


def soft_masks(fg, feather=0.0, dilate=0.0, normalize=False, device="cuda"):
    """Soft blend weights of one or several mask sets, through tmix_mask_edt and tmix_soft_masks: fg [K-1,h,w] or [n,K-1,h,w] (tensor or
    array; thresholded at 0.5 like preprocess_mask) -> [K,1,h,w] or [n,K,1,h,w] fp32 on `device`.  Every foreground region is grown by
    `dilate` latent pixels (negative: shrunk) and its edge ramped over `feather` latent pixels around the moved border; normalize=True
    divides the foreground weights by their sum where it exceeds 1, so that the K weights are a partition of unity everywhere.
    dilate = 0 with feather <= 1 and normalize=False returns build_masks' bits."""
    from . import ops
    fg = torch.as_tensor(np.asarray(fg, np.float32) if not torch.is_tensor(fg) else fg).to(device, torch.float32).contiguous()
    if fg.dim() not in (3, 4) or fg.shape[-3] < 1:
        raise ValueError(f"soft_masks: fg is {tuple(fg.shape)}, expected [K-1, h, w] or [n, K-1, h, w]")
    n, km1, h, w = (1,) + tuple(fg.shape) if fg.dim() == 3 else tuple(fg.shape)
    d_set, d_clear = ops.mask_edt(fg.view(n * km1, h, w))
    out = ops.soft_masks(d_set.view(n, km1, h, w), d_clear.view(n, km1, h, w), feather, dilate, normalize).unsqueeze(2)
    return out[0] if fg.dim() == 3 else out


def soft_region(region, feather=0.0, dilate=0.0, device="cuda"):
    """the u of ONE binary region ([..., h, w] with a single map in it, thresholded at 0.5), same shape, fp32 on `device`: what a keep
    region's weight is made of (1 - soft_region(union of the re-rolled regions))"""
    region = torch.as_tensor(np.asarray(region, np.float32) if not torch.is_tensor(region) else region)
    h, w = region.shape[-2:]
    if region.numel() != h * w:
        raise ValueError(f"soft_region: one [h, w] map, got {tuple(region.shape)}")
    return soft_masks(region.reshape(1, h, w), feather, dilate, False, device)[0:1].reshape(region.shape)


def random_rectangle_masks(K: int, H: int, W: int, seed: int = 0):
    """K-1 seeded axis-aligned rectangles (10-30 % area each) on the H x W image grid, uint8 {0,255}."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(K - 1):
        area = rng.uniform(0.10, 0.30) * H * W
        ar = rng.uniform(0.6, 1.6)
        hh = int(min(H, max(8, round((area * ar) ** 0.5))))
        ww = int(min(W, max(8, round(area / hh))))
        y0 = rng.randint(0, H - hh + 1)
        x0 = rng.randint(0, W - ww + 1)
        m = np.zeros((H, W), np.uint8)
        m[y0:y0 + hh, x0:x0 + ww] = 255
        out.append(m)
    return out


def partition_rectangle_masks(K: int, H: int, W: int, seed: int = 0):
    """K-1 seeded rectangles that do NOT overlap: rectangle k loses every pixel an earlier one claimed (what the side-car's
    overlap rule does to its second mask above the 0.8 threshold, text_segment/run_expand.py:78-87), re-drawn while less than
    half of it survives.  With these, fg_1 + ... + fg_{K-1} + bg == 1 on every pixel, i.e. the blend of
    fusion_sampling.py:466-469 is a convex combination and the latent keeps its scale through the fusion window; with
    random_rectangle_masks the weights sum to 2 on the overlap and that region doubles every fusion step (the reference does
    not normalise).  uint8 {0,255}, same conventions as random_rectangle_masks."""
    rng = np.random.RandomState(seed)
    taken = np.zeros((H, W), bool)
    out = []
    for _ in range(K - 1):
        for _try in range(64):
            area = rng.uniform(0.10, 0.30) * H * W
            ar = rng.uniform(0.6, 1.6)
            hh = int(min(H, max(8, round((area * ar) ** 0.5))))
            ww = int(min(W, max(8, round(area / hh))))
            y0 = rng.randint(0, H - hh + 1)
            x0 = rng.randint(0, W - ww + 1)
            m = np.zeros((H, W), bool)
            m[y0:y0 + hh, x0:x0 + ww] = True
            m &= ~taken
            if 2 * int(m.sum()) >= hh * ww:
                break
        taken |= m
        out.append(m.astype(np.uint8) * 255)
    return out


def synthetic_masks(kind: str, K: int, H: int, W: int, seed: int = 0):
    """'partition' (default of bench.py and the trajectory parity test) or 'overlap' (random_rectangle_masks: the reference's
    un-normalised weights on intersecting rectangles, kept as a labelled second case)."""
    if kind == "partition":
        return partition_rectangle_masks(K, H, W, seed)
    if kind == "overlap":
        return random_rectangle_masks(K, H, W, seed)
    raise ValueError(f"mask kind {kind!r}: 'partition' or 'overlap'")


def expand_masks(masks):
    """The side-car's post-processing of the two SAM masks (text_segment/run_expand.py:35-87): every mask becomes its
    bounding rectangle; where the two rectangles overlap, the bounding box of the overlap is re-filled with the
    ORIGINAL masks restricted to the overlap, and mask 1 loses it entirely when more than 80 % of original mask 0
    lies inside the overlap.  Like the reference this handles exactly two foreground masks (:62); for any other
    count only the rectangles are produced.  masks: list of bool arrays [H,W]; returns list of bool arrays."""
    import numpy as np
    orig = [np.asarray(m).astype(bool) for m in masks]
    rect = []
    for m in orig:
        ys, xs = np.nonzero(m)
        r = np.zeros_like(m)
        r[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = True
        rect.append(r)
    if len(rect) == 2:
        ov = rect[0] & rect[1]
        if ov.any():
            ys, xs = np.nonzero(ov)
            y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
            o1 = ov & orig[0]
            o2 = ov & orig[1]
            if o1.sum() / orig[0].sum() > 0.8:
                o2 = np.zeros_like(o2)
            rect[0][y0:y1, x0:x1] = o1[y0:y1, x0:x1]
            rect[1][y0:y1, x0:x1] = o2[y0:y1, x0:x1]
    return rect


def _upsample_bilinear(m, gh: int, gw: int):
    """[h,w] -> [gh,gw], bilinear with half-pixel centres and edge clamping (torch interpolate, align_corners=False)"""
    m = np.asarray(m, np.float64)

    def axis(n_in, n_out):
        x = np.clip((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1)
        i0 = np.floor(x).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, x - i0

    y0, y1, fy = axis(m.shape[0], gh)
    x0, x1, fx = axis(m.shape[1], gw)
    r = m[y0] * (1 - fy)[:, None] + m[y1] * fy[:, None]
    return r[:, x0] * (1 - fx)[None, :] + r[:, x1] * fx[None, :]


def _flood_components(mask):
    """4-connected components of a bool [h,w] mask by a flood fill from every unlabelled set pixel in raster order: (label int32 [h,w], 1, 2, ...
    in the order the components are reached and 0 on clear pixels; first = each component's first pixel as a raster index, which is its
    smallest; size = its pixel count)"""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    label = np.zeros((h, w), np.int32)
    first, size = [], []
    for y0, x0 in zip(*np.nonzero(mask)):
        if label[y0, x0]:
            continue
        n_lab = len(first) + 1
        label[y0, x0] = n_lab
        stack, n = [(y0, x0)], 0
        while stack:
            y, x = stack.pop()
            n += 1
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not label[yy, xx]:
                    label[yy, xx] = n_lab
                    stack.append((yy, xx))
        first.append(int(y0) * w + int(x0))
        size.append(n)
    return label, first, size


def largest_component(mask):
    """the largest 4-connected component of a bool [h,w] mask (ties: the one reached first in raster order); empty stays empty"""
    mask = np.asarray(mask, bool)
    label, _, size = _flood_components(mask)
    best, best_n = 0, 0
    for i, n in enumerate(size):
        if n > best_n:
            best, best_n = i + 1, n
    return label == best if best else np.zeros_like(mask)


def mask_label_reference(map, threshold=0.5, invert=False):
    """numpy restatement of tmix_mask_label: map [..., h, w] -> int32 of the same shape; a pixel is set where fp32(map) >= fp32(threshold);
    every set pixel (invert: every clear pixel) gets the smallest raster index y * w + x of its 4-connected component, the others -1"""
    m = np.asarray(map, np.float32) >= np.float32(threshold)
    if invert:
        m = ~m
    h, w = m.shape[-2:]
    out = np.empty(m.shape, np.int32)
    for b, o in zip(m.reshape(-1, h, w), out.reshape(-1, h, w)):
        label, first, _ = _flood_components(b)
        o[...] = np.array([-1] + first, np.int32)[label]
    return out


def _fill_holes(shape):
    """bool [h,w] plus its holes: the 4-connected components of its complement without a pixel in the first or last row or column"""
    shape = np.asarray(shape, bool)
    label, _, _ = _flood_components(~shape)
    border = np.unique(np.concatenate([label[0], label[-1], label[:, 0], label[:, -1]]))
    return shape | ((label > 0) & ~np.isin(label, border))


def attn_shapes_reference(score, threshold, fill_holes=True, resolve=True):
    """numpy restatement of tmix_attn_shapes, compared with the kernels by equality: score [K-1,h,w] or [n_sets,K-1,h,w]
    (rounded to fp32 here) -> fp32 {0, 1} of the same shape.  Per concept the largest component of fp32(score) >= fp32(threshold)
    (largest_component's tie rule), with its holes filled (fill_holes); with resolve a pixel that several concepts of a set claim stays
    with the highest score there (fp32 >, in ascending k: equal scores go to the smallest k)."""
    score = np.asarray(score, np.float32)
    if score.ndim not in (3, 4):
        raise ValueError(f"attn_shapes_reference: score is {score.shape}, expected [K-1, h, w] or [n_sets, K-1, h, w]")
    sets = score[None] if score.ndim == 3 else score
    out = np.zeros(sets.shape, np.float32)
    for s, o in zip(sets, out):
        f = [largest_component(sk >= np.float32(threshold)) for sk in s]
        if fill_holes:
            f = [_fill_holes(c) for c in f]
        if resolve:
            owner = np.full(s.shape[1:], -1, np.int64)
            top = np.zeros(s.shape[1:], np.float32)
            for k, (c, sk) in enumerate(zip(f, s)):
                with np.errstate(invalid="ignore"):
                    take = c & ((owner < 0) | (sk > top))
                owner[take], top[take] = k, sk[take]
            f = [c & (owner == k) for k, c in enumerate(f)]
        o[...] = np.stack(f).astype(np.float32)
    return out[0] if score.ndim == 3 else out


def attention_scores(maps_per_level, tokens_per_concept, level_weights=None):
    """The per-concept score of attention_masks, fp64 [K-1, gh, gw] on the finest level's grid: mean of the concept's token maps -> bilinear
    upsampling of every level, weighted sum -> min / max normalisation to [0, 1] (a constant map counts as 1 everywhere).  Arguments as
    attention_masks."""
    if isinstance(maps_per_level, dict):
        keys = list(maps_per_level)
        maps = [np.asarray(maps_per_level[k], np.float64) for k in keys]
        wts = [1.0 if level_weights is None else float(level_weights.get(k, 0.0)) for k in keys]
    else:
        maps = [np.asarray(m, np.float64) for m in maps_per_level]
        wts = [1.0] * len(maps) if level_weights is None else [float(x) for x in level_weights]
    if not maps or len(wts) != len(maps):
        raise ValueError("attention_masks: no maps, or level weights that do not match the levels")
    gh = max(m.shape[1] for m in maps)
    gw = max(m.shape[2] for m in maps)
    score = []
    for toks in tokens_per_concept:
        toks = list(toks)
        if not toks:
            raise ValueError("attention_masks: a concept without token maps")
        acc = np.zeros((gh, gw), np.float64)
        for m, wt in zip(maps, wts):
            if wt:
                acc += wt * _upsample_bilinear(m[toks].mean(axis=0), gh, gw)
        lo, hi = acc.min(), acc.max()
        score.append((acc - lo) / (hi - lo) if hi > lo else np.ones_like(acc))
    return np.stack(score) if score else np.zeros((0, gh, gw), np.float64)


def attention_masks(maps_per_level, tokens_per_concept, H: int, W: int, threshold: float = 0.5, level_weights=None, shape="rect",
                    fill_holes=True, device=None):
    """Blend masks from cross-attention token maps (the in-process stand-in for the segmentation side-car).

    maps_per_level  {level: [n_tok, h_l, w_l]} (or a sequence of such arrays): one batch row's summed attn2 probabilities on the
                    token positions (UNetPlan.token_maps of a probe plan, reshaped to the level's grid)
    tokens_per_concept  K-1 lists of indices into n_tok: which maps belong to foreground concept k
    level_weights   {level: weight} (or a sequence in the order of maps_per_level); default 1 for every level -- the maps are SUMS
                    over the level's attn2 modules, so equal weights let every module count once
    Per concept: mean of its token maps -> bilinear upsampling of every level to the finest level's grid, weighted sum -> min / max
    normalisation to [0, 1] (a constant map counts as 1 everywhere): attention_scores.  Then
    shape="rect"  threshold (>=, in fp64) -> largest 4-connected component -> the side-car's expand_masks (bounding rectangles,
                  run_expand.py's overlap rule for two concepts);
    shape="free"  the score rounded once to fp32 -> threshold (>=, in fp32) -> largest 4-connected component -> its holes filled
                  (fill_holes) -> every pixel that several concepts claim goes to the highest score there: the object's own outline, disjoint
                  for any K.  On a GPU `device` through ops.attn_shapes, with device=None or a CPU device through its numpy
                  restatement attn_shapes_reference; the two are equal;
    and a nearest upsampling to H x W.  Returns K-1 uint8 {0,255} [H,W] arrays: what random_rectangle_masks returns and build_masks consumes."""
    if shape not in ("rect", "free"):
        raise ValueError(f"attention_masks: shape={shape!r}: 'rect' or 'free'")
    score = attention_scores(maps_per_level, tokens_per_concept, level_weights)
    gh, gw = score.shape[1:]
    if shape == "rect":
        out = expand_masks([largest_component(s >= threshold) for s in score])
    elif device is not None and torch.device(device).type != "cpu":
        from . import ops
        s32 = torch.from_numpy(score.astype(np.float32)[None]).to(device)
        out = list(ops.attn_shapes(s32, threshold, fill_holes, True)[0].cpu().numpy() != 0)
    else:
        out = list(attn_shapes_reference(score.astype(np.float32), threshold, fill_holes, True) != 0)
    ys = np.minimum((np.arange(H) * gh) // H, gh - 1)
    xs = np.minimum((np.arange(W) * gw) // W, gw - 1)
    return [np.ascontiguousarray(r[ys][:, xs]).astype(np.uint8) * 255 for r in out]


def sidecar_layout(output_path, rank: int, world: int, local_gpu: int, seg_gpu: int):
    """(directory, GPU) the segmentation side-car of rank `rank` uses.  One process (the reference's mode): exactly the reference's
    `{output_path}` and `--seg_gpu`.  Several ranks sample different seeds at the same time, so each gets its OWN directory
    `{output_path}/rank{r}` -- with a shared one, rank A could read the masks the side-car wrote for rank B's preview -- and, when
    `--seg_gpu` names a GPU that one of the ranks samples on (the default 1 does as soon as world > 1), the side-car runs on the
    rank's own GPU instead: that GPU is idle while its rank waits for the masks, whereas another rank's GPU is mid-trajectory."""
    import os
    if world <= 1:
        return output_path, seg_gpu
    gpu = local_gpu if 0 <= seg_gpu < world else seg_gpu
    # the side-car's command line sets CUDA_VISIBLE_DEVICES itself (fusion_sampling.py:458), and the child inherits the parent's environment:
    #   * parent restricted by CUDA_VISIBLE_DEVICES: the child's own value replaces it -> the i-th entry of the parent's list;
    #   * parent restricted by HIP_VISIBLE_DEVICES: the HIP runtime prefers that variable, so a child that inherits it would ignore its own
    #     CUDA_VISIBLE_DEVICES and every side-car would land on the first visible GPU -> the i-th entry of the HIP list, and
    #     SidecarMaskProvider drops HIP_VISIBLE_DEVICES from the child's environment (sidecar_child_env);
    #   * parent restricted by ROCR_VISIBLE_DEVICES only: HIP / CUDA ordinals index the already filtered list -> the rank-local index as is.
    vis = os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("CUDA_VISIBLE_DEVICES")
    if vis and gpu == local_gpu:
        ids = [v.strip() for v in vis.split(",") if v.strip()]
        if 0 <= local_gpu < len(ids) and ids[local_gpu].lstrip("-").isdigit():
            gpu = int(ids[local_gpu])
    return os.path.join(output_path, f"rank{rank}"), gpu


def sidecar_child_env():
    """environment of the side-car process: the parent's without HIP_VISIBLE_DEVICES (see sidecar_layout: the command line's own
    CUDA_VISIBLE_DEVICES must be what selects the GPU; ROCR_VISIBLE_DEVICES, which filters below both, stays)"""
    import os
    env = dict(os.environ)
    env.pop("HIP_VISIBLE_DEVICES", None)
    return env


class SidecarMaskProvider:
    """The reference's segmentation side-car contract (fusion_sampling.py:453-469): decode the Tweedie preview,
    save `{output_path}/tweedie.jpg`, run an external command that writes `{output_path}/{seg_concept}.jpg`
    (8-bit masks; `text_segment/run_expand.py` in the reference), read them back through preprocess_mask.
    cmd_template may use {input_path}, {text_condition}, {output_path}, {seg_gpu}."""

    DEFAULT_CMD = ('CUDA_VISIBLE_DEVICES={seg_gpu} python text_segment/run_expand.py --input_path={input_path} '
                   '--text_condition="{text_condition}" --output_path={output_path}')

    def __init__(self, sampler, output_path, seg_concepts, seg_gpu=1, cmd_template=None):
        self.sampler, self.output_path, self.seg_concepts, self.seg_gpu = sampler, output_path, seg_concepts, seg_gpu
        self.cmd_template = cmd_template or self.DEFAULT_CMD

    def __call__(self, x0_preview):
        import os
        from PIL import Image
        os.makedirs(self.output_path, exist_ok=True)
        assert x0_preview.shape[0] == 1, "one preview per call: the sampler asks once per co-batched seed, in seed order"
        img = self.sampler.decode_latent(x0_preview[:1])[0]                       # [3,H,W] in [0,1]
        arr = (img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()   # ToPILImage semantics (mul 255, byte)
        path = os.path.join(self.output_path, "tweedie.jpg")
        Image.fromarray(arr).save(path)
        cmd = self.cmd_template.format(input_path=path, text_condition=self.seg_concepts, output_path=self.output_path,
                                       seg_gpu=self.seg_gpu)
        import subprocess
        subprocess.call(cmd, shell=True, env=sidecar_child_env())                # (os.system with a cleaned environment; return code ignored, like the reference)
        paths = [os.path.join(self.output_path, sp + ".jpg") for sp in self.seg_concepts.split("+")]
        s = self.sampler
        return build_masks(paths, s.canvas_h, s.canvas_w, s.device)      # (the window's grid unless the sampler has a canvas)
