"""Thin torch-tensor wrappers over the C ABI (include/tmix.h).

PyTorch is plumbing only: device memory (data_ptr) and the current HIP stream.  Every wrapper
validates on the C side and raises TmixError on failure; there is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import lib as L

BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.TmixError("tweediemix_amd ops need device tensors (no CPU fallback exists)")


_EPS_DT = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}


def step_coeffs(at, at_next):
    """fp32 sqrt(at), sqrt(1-at), sqrt(at'), sqrt(1-at') exactly as the fp32 reference computes them."""
    at, an = np.float32(at), np.float32(at_next)
    one = np.float32(1)
    return (float(np.sqrt(at)), float(np.sqrt(one - at)), float(np.sqrt(an)), float(np.sqrt(one - an)))


def fused_tweedie_step(x, eps, masks, mode, K, g, at, at_next, is_last=False, out_x=None, out_x0=None):
    """x [1,C,h,w] fp32; eps [rows,C,h,w] f32|f16|bf16; masks [K,1,h,w] fp32 (FUSION).  Returns out_x."""
    _need_cuda(x, eps, masks)
    lib = L.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    Cc, h, w = x.shape[-3], x.shape[-2], x.shape[-1]
    rows = eps.shape[0]
    need = {L.STEP_FUSION: K + 1, L.STEP_PLAIN: 2, L.STEP_RESAMPLE: K + 1}[mode]
    if rows < need:
        raise L.TmixError(f"tweedie step mode {mode} needs {need} eps rows, got {rows}")
    if mode == L.STEP_FUSION:
        assert masks is not None and masks.dtype == torch.float32 and masks.is_contiguous() and masks.shape[0] == K
        assert masks.numel() == K * h * w
    if out_x is None:
        out_x = torch.empty_like(x)
    sa, s1, san, s1n = step_coeffs(at, at_next)
    L.check(lib.tmix_fused_tweedie_step(_p(x), _p(eps), _EPS_DT[eps.dtype], _p(masks), _p(out_x), _p(out_x0),
                                        K, Cc, h * w, mode, float(g), sa, s1, san, s1n, int(bool(is_last)),
                                        _stream()), "tmix_fused_tweedie_step")
    return out_x


def _seed_stride(t, seeds, extent, what):
    """seed stride of a keep array [1 or seeds, ..., extent floats]: 0 when one array is shared by all seeds"""
    assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] in (1, seeds) and t.numel() == t.shape[0] * extent, (what, tuple(t.shape))
    return 0 if t.shape[0] == 1 else extent


def _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev=None):
    """the shared preparation of the *_dev step wrappers: (S, n, hw, rows, out_x, head), head the 14 arguments every such entry begins with
    (the multistep entries take x0_prev behind the seventh)"""
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous() and params.dtype == torch.float32 and params.numel() >= 8
    if x0_prev is not None:
        assert x0_prev.dtype == torch.float32 and x0_prev.is_contiguous() and x0_prev.shape == x.shape, tuple(x0_prev.shape)
    S, Cc, h, w = x.shape
    hw = h * w
    assert eps.shape[0] % S == 0
    rows = eps.shape[0] // S
    mss = 0
    if mode == L.STEP_FUSION:
        assert masks is not None and masks.dtype == torch.float32 and masks.is_contiguous() and masks.numel() in (K * hw, S * K * hw)
        mss = 0 if masks.numel() == K * hw else K * hw
    if out_x is None:
        out_x = torch.empty_like(x)
    head = (_p(x), _p(eps), _EPS_DT[eps.dtype], _p(masks), mss, _p(out_x), _p(out_x0), K, Cc, hw, mode, rows, S, _p(params))
    return S, Cc * hw, hw, rows, out_x, head


def fused_tweedie_step_keep_dev(x, eps, masks, mode, K, params, keep_x0, keep_eps, keep_w, out_x=None, out_x0=None):
    """tmix_fused_tweedie_step_keep_dev: x [S,C,h,w] fp32, eps [S*rows,C,h,w] f32|f16|bf16, masks [K,1,h,w] or [S,K,1,h,w] (FUSION),
    params the device buffer {t, sa, s1, sa_next, s1_next, is_last, g, -}; keep_x0 [1|S,C,h,w], keep_eps [1|S,C,h,w], keep_w [1|S,1,h,w]
    (first axis 1: shared by all seeds).  out_x may be x itself (in place).  Returns out_x."""
    _need_cuda(x, eps, masks, params, keep_x0, keep_eps, keep_w)
    S, n, hw, _rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0)
    L.check(L.load().tmix_fused_tweedie_step_keep_dev(
        *head, _p(keep_x0), _seed_stride(keep_x0, S, n, "keep_x0"), _p(keep_eps), _seed_stride(keep_eps, S, n, "keep_eps"),
        _p(keep_w), _seed_stride(keep_w, S, hw, "keep_w"), _stream()), "tmix_fused_tweedie_step_keep_dev")
    return out_x


def fused_tweedie_step_ms_dev(x, eps, masks, mode, K, params, x0_prev, out_x=None, out_x0=None):
    """tmix_fused_tweedie_step_ms_dev: x [S,C,h,w] fp32, eps [S*rows,C,h,w] f32|f16|bf16, masks [K,1,h,w] or [S,K,1,h,w] (FUSION), params the
    device buffer {t, sa, s1, cx, c0, c1, is_last, g} (solver.multistep_coeffs), x0_prev [S,C,h,w] fp32 the history buffer, read and
    rewritten with this step's x0.  out_x may be x itself (in place).  Returns out_x."""
    _need_cuda(x, eps, masks, params, x0_prev)
    _S, _n, _hw, _rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev)
    L.check(L.load().tmix_fused_tweedie_step_ms_dev(*head[:7], _p(x0_prev), *head[7:], _stream()), "tmix_fused_tweedie_step_ms_dev")
    return out_x


def cfg_rescale_ws(rows, seeds, device):
    """the fp64 workspace tmix_cfg_rescale_factors needs for `seeds` seeds of `rows` eps rows (contents irrelevant: written before read)"""
    nd = int(L.load().tmix_cfg_rescale_ws_doubles(int(rows), int(seeds)))
    if nd < 1:
        raise L.TmixError(f"cfg_rescale_ws: rows={rows} (2..256) seeds={seeds} (1..65535)")
    return torch.empty(nd, device=device, dtype=torch.float64)


def cfg_rescale_factors(eps, seeds, mode, K, params, g_slot, phi, out=None, ws=None):
    """tmix_cfg_rescale_factors: eps [S*rows,C,h,w] f32|f16|bf16, params the step's device buffer (>= 8 floats) with g in slot g_slot (6: the
    DDIM layout, 7: the multistep layout), phi in [0, 1] -> factors [S, rows-1] fp32 (guidance.rescale_factors_reference per seed)."""
    from .guidance import validate_phi
    _need_cuda(eps, params, out, ws)
    assert eps.is_contiguous() and eps.dim() == 4 and eps.shape[0] % seeds == 0 and params.dtype == torch.float32 and params.numel() >= 8
    rows = eps.shape[0] // seeds
    Cc, h, w = eps.shape[1:]
    if out is None:
        out = torch.empty(seeds, rows - 1, device=eps.device, dtype=torch.float32)
    if ws is None:
        ws = cfg_rescale_ws(rows, seeds, eps.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == seeds * (rows - 1), tuple(out.shape)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= L.load().tmix_cfg_rescale_ws_doubles(rows, seeds)
    L.check(L.load().tmix_cfg_rescale_factors(_p(eps), _EPS_DT[eps.dtype], _p(out), _p(ws), K, Cc, h * w, mode, rows, seeds, _p(params),
                                              int(g_slot), validate_phi(phi, "phi"), _stream()), "tmix_cfg_rescale_factors")
    return out


def fused_tweedie_step_rs_dev(x, eps, masks, mode, K, params, factors, out_x=None, out_x0=None, x0_prev=None):
    """tmix_fused_tweedie_step_rs_dev, or with x0_prev (the history buffer) tmix_fused_tweedie_step_ms_rs_dev: the arguments of
    fused_tweedie_step_ms_dev plus factors [S, rows-1] fp32 (cfg_rescale_factors).  out_x may be x itself (in place).  Returns out_x."""
    _need_cuda(x, eps, masks, params, factors, x0_prev)
    S, _n, _hw, rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev)
    assert factors.dtype == torch.float32 and factors.is_contiguous() and factors.numel() == S * (rows - 1), tuple(factors.shape)
    if x0_prev is None:
        L.check(L.load().tmix_fused_tweedie_step_rs_dev(*head, _p(factors), _stream()), "tmix_fused_tweedie_step_rs_dev")
    else:
        L.check(L.load().tmix_fused_tweedie_step_ms_rs_dev(*head[:7], _p(x0_prev), *head[7:], _p(factors), _stream()), "tmix_fused_tweedie_step_ms_rs_dev")
    return out_x


def noise_normal(n, first_index, key, step, stream_id=0, out=None, device="cuda"):
    """tmix_noise_normal: z [n] fp32, z[i] the normal of index first_index + i under key = (low word, high word) at schedule step `step`
    (noise.normal gives the same bits).  out: a contiguous fp32 device tensor of n elements to write instead of a new one."""
    if out is None:
        out = torch.empty(int(n), device=device, dtype=torch.float32)
    _need_cuda(out)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == int(n), (tuple(out.shape), n)
    L.check(L.load().tmix_noise_normal(_p(out), int(n), int(first_index), int(key[0]), int(key[1]), int(step), int(stream_id), _stream()),
            "tmix_noise_normal")
    return out


def noise_keys(seeds, device):
    """the `keys` array of fused_tweedie_step_noise_dev: int32 [len(seeds), 2] holding the {low, high} words of every trajectory's seed value"""
    from .noise import seed_key
    words = np.array([seed_key(s) for s in seeds], dtype=np.uint32).reshape(-1, 2)
    return torch.from_numpy(words.view(np.int32).copy()).to(device)


def fused_tweedie_step_noise_dev(x, eps, masks, mode, K, params, keys, x0_prev=None, factors=None, windows=None, canvas_hw=None, out_x=None,
                                 out_x0=None):
    """tmix_fused_tweedie_step_noise_dev: the stochastic form of fused_tweedie_step_dev's entry (x0_prev None), of fused_tweedie_step_ms_dev
    (x0_prev the history buffer) and, with factors [S, rows-1], of their rescale forms.  params holds 12 floats: the parent's 8, then
    {cz, step_index, 0, 0}.  keys int32 [S / n_win, 2] (noise_keys).  windows [(oy, ox), ...] with canvas_hw = (canvas_h, canvas_w): the S rows
    are window-major inside a trajectory (window_consensus's layout); None: no canvas.  out_x may be x itself.  Returns out_x."""
    _need_cuda(x, eps, masks, params, keys, x0_prev, factors)
    S, _n, _hw, rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev)
    n_win = 1 if windows is None else len(windows)
    assert params.numel() >= 12, params.numel()
    assert keys.dtype == torch.int32 and keys.is_contiguous() and keys.numel() == 2 * (S // n_win) and S % n_win == 0, (tuple(keys.shape), S, n_win)
    if factors is not None:
        assert factors.dtype == torch.float32 and factors.is_contiguous() and factors.numel() == S * (rows - 1), tuple(factors.shape)
    yx, ch, cw = None, 0, 0
    if windows is not None:
        yx = (C.c_int32 * (2 * n_win))(*[int(v) for o in windows for v in o])
        ch, cw = int(canvas_hw[0]), int(canvas_hw[1])
    L.check(L.load().tmix_fused_tweedie_step_noise_dev(*head, _p(x0_prev), _p(factors), _p(keys), x.shape[-1], n_win, yx, ch, cw, _stream()),
            "tmix_fused_tweedie_step_noise_dev")
    return out_x


def fused_tweedie_step_cond_dev(x, eps, masks, mode, K, params, x0_prev=None, keys=None, windows=None, canvas_hw=None, out_x=None, out_x0=None):
    """tmix_fused_tweedie_step_cond_dev, the unguided step: eps [S*rows,C,h,w] f32|f16|bf16 holds NO unconditional row (FUSION:
    rows >= K, row c concept c's; PLAIN: rows >= 1).  x0_prev None: params {t, sa, s1, sa_next, s1_next, is_last, -, -} and the DDIM move on the
    eps consistent with x0; else the history buffer and {t, sa, s1, cx, c0, c1, is_last, -}.  keys None: no noise; else int32 [S / n_win, 2]
    (noise_keys), params holds 12 floats and windows / canvas_hw are fused_tweedie_step_noise_dev's.  guidance.cond_step_reference gives the
    same bits.  out_x may be x itself.  Returns out_x."""
    _need_cuda(x, eps, masks, params, keys, x0_prev)
    S, _n, _hw, _rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev)
    n_win = 1 if windows is None else len(windows)
    if keys is not None:
        assert params.numel() >= 12, params.numel()
        assert keys.dtype == torch.int32 and keys.is_contiguous() and keys.numel() == 2 * (S // n_win) and S % n_win == 0, (tuple(keys.shape), S, n_win)
    yx, ch, cw = None, 0, 0
    if windows is not None:
        yx = (C.c_int32 * (2 * n_win))(*[int(v) for o in windows for v in o])
        ch, cw = int(canvas_hw[0]), int(canvas_hw[1])
    L.check(L.load().tmix_fused_tweedie_step_cond_dev(*head, _p(x0_prev), _p(keys), x.shape[-1], n_win, yx, ch, cw, _stream()),
            "tmix_fused_tweedie_step_cond_dev")
    return out_x


def apg_coeffs(x, eps, mode, K, params, g_slot, eta=0.0, norm_threshold=0.0, out=None, ws=None):
    """tmix_apg_coeffs, adaptive projected guidance (arXiv:2410.02416): x [S,C,h,w] fp32 the state the step will read, eps
    [S*rows,C,h,w] f32|f16|bf16, params the step's device buffer (>= 8 floats: sa, s1 in slots 1, 2; g in slot g_slot -- 6: the DDIM layout, 7:
    the multistep layout) -> coeffs [S, rows-1, 2] fp32 = {A, B} per conditional row (guidance.apg_coeffs_reference per seed): with d = tc - tu
    of the rows' Tweedie estimates, s = R > 0 and Sdd > R^2 ? R / sqrt(Sdd) : 1, p = Scc > 0 ? s Sdc / Scc : 0, A = 1 - (g-1)(1-eta) p,
    B = (g-1) s; {1, g-1} where a sum is not finite and for rows the mode does not read.  ws: cfg_rescale_ws(rows, S)."""
    from .guidance import validate_apg
    a = validate_apg(dict(eta=eta, norm_threshold=norm_threshold), "apg_coeffs")
    _need_cuda(x, eps, params, out, ws)
    S = x.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and eps.is_contiguous() and eps.dim() == 4 and eps.shape[0] % S == 0
    assert tuple(eps.shape[1:]) == tuple(x.shape[1:]) and params.dtype == torch.float32 and params.numel() >= 8
    rows = eps.shape[0] // S
    Cc, h, w = eps.shape[1:]
    if out is None:
        out = torch.empty(S, rows - 1, 2, device=eps.device, dtype=torch.float32)
    if ws is None:
        ws = cfg_rescale_ws(rows, S, eps.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == S * (rows - 1) * 2, tuple(out.shape)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= L.load().tmix_cfg_rescale_ws_doubles(rows, S)
    L.check(L.load().tmix_apg_coeffs(_p(x), _p(eps), _EPS_DT[eps.dtype], _p(out), _p(ws), K, Cc, h * w, mode, rows, S, _p(params), int(g_slot),
                                     a["eta"], a["norm_threshold"], _stream()), "tmix_apg_coeffs")
    return out


def fused_tweedie_step_apg_dev(x, eps, masks, mode, K, params, coeffs, x0_prev=None, keys=None, windows=None, canvas_hw=None, out_x=None,
                               out_x0=None):
    """tmix_fused_tweedie_step_apg_dev, the APG step: every conditional row's Tweedie estimate is A tc + B (tc - tu) with {A, B} =
    coeffs [S, rows-1, 2] (apg_coeffs); the blend, the move and the noise behind it are the parent's.  x0_prev None: params {t, sa, s1, sa_next,
    s1_next, is_last, g, -} and the DDIM move (FUSION, PLAIN, RESAMPLE); else the history buffer and {t, sa, s1, cx, c0, c1, is_last, g} (FUSION,
    PLAIN).  keys None: no noise; else int32 [S / n_win, 2] (noise_keys), params holds 12 floats and windows / canvas_hw are
    fused_tweedie_step_noise_dev's.  guidance.apg_step_reference / apg_multistep_reference give the same bits.  out_x may be x itself."""
    _need_cuda(x, eps, masks, params, coeffs, keys, x0_prev)
    S, _n, _hw, rows, out_x, head = _dev_step_head(x, eps, masks, mode, K, params, out_x, out_x0, x0_prev)
    assert coeffs.dtype == torch.float32 and coeffs.is_contiguous() and coeffs.numel() == S * (rows - 1) * 2, tuple(coeffs.shape)
    n_win = 1 if windows is None else len(windows)
    if keys is not None:
        assert params.numel() >= 12, params.numel()
        assert keys.dtype == torch.int32 and keys.is_contiguous() and keys.numel() == 2 * (S // n_win) and S % n_win == 0, (tuple(keys.shape), S, n_win)
    yx, ch, cw = None, 0, 0
    if windows is not None:
        yx = (C.c_int32 * (2 * n_win))(*[int(v) for o in windows for v in o])
        ch, cw = int(canvas_hw[0]), int(canvas_hw[1])
    L.check(L.load().tmix_fused_tweedie_step_apg_dev(*head, _p(x0_prev), _p(coeffs), _p(keys), x.shape[-1], n_win, yx, ch, cw, _stream()),
            "tmix_fused_tweedie_step_apg_dev")
    return out_x


def window_consensus(x, groups, offsets, canvas_hw, weight=None):
    """tmix_window_consensus, in place on x [groups * n_win, C, h, w] fp32 (group-major: b = group * n_win + window): every canvas pixel
    that several windows cover becomes their weighted mean in all of them.  offsets [(oy, ox), ...] the windows' corners on the canvas
    of canvas_hw = (canvas_h, canvas_w); weight [h, w] fp32 per window pixel, or None = all ones.  Returns x."""
    _need_cuda(x, weight)
    n_win = len(offsets)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[0] == groups * n_win, (tuple(x.shape), groups, n_win)
    Cc, h, w = x.shape[1:]
    if weight is not None:
        assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == h * w, tuple(weight.shape)
    yx = (C.c_int32 * (2 * n_win))(*[int(v) for o in offsets for v in o])
    L.check(L.load().tmix_window_consensus(_p(x), int(groups), n_win, yx, Cc, h, w, int(canvas_hw[0]), int(canvas_hw[1]), _p(weight),
                                           _stream()), "tmix_window_consensus")
    return x


def mask_edt(mask, d_set=None, d_clear=None):
    """tmix_mask_edt: mask [n, h, w] fp32 (set where >= 0.5) -> (d_set, d_clear) int32 [n, h, w], the exact squared Euclidean distance of
    every pixel to the nearest set / clear pixel (L.EDT_NONE where the mask has none)."""
    _need_cuda(mask, d_set, d_clear)
    assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.dim() == 3, tuple(mask.shape)
    n, h, w = mask.shape
    if d_set is None:
        d_set = torch.empty(n, h, w, dtype=torch.int32, device=mask.device)
    if d_clear is None:
        d_clear = torch.empty(n, h, w, dtype=torch.int32, device=mask.device)
    for d in (d_set, d_clear):
        assert d.dtype == torch.int32 and d.is_contiguous() and tuple(d.shape) == (n, h, w), tuple(d.shape)
    L.check(L.load().tmix_mask_edt(_p(mask), _p(d_set), _p(d_clear), n, h, w, _stream()), "tmix_mask_edt")
    return d_set, d_clear


def soft_masks(d_set, d_clear, feather=0.0, dilate=0.0, normalize=False, out=None):
    """tmix_soft_masks: distances [n_sets, K-1, h, w] int32 (mask_edt) -> blend weights [n_sets, K, h, w] fp32: the K-1 dilated and
    feathered foreground weights, then the background; feather / dilate in pixels of the grid (include/tmix.h has the formula)."""
    _need_cuda(d_set, d_clear, out)
    assert d_set.dtype == torch.int32 and d_set.is_contiguous() and d_set.dim() == 4, tuple(d_set.shape)
    assert d_clear.dtype == torch.int32 and d_clear.is_contiguous() and d_clear.shape == d_set.shape, tuple(d_clear.shape)
    n_sets, km1, h, w = d_set.shape
    if out is None:
        out = torch.empty(n_sets, km1 + 1, h, w, dtype=torch.float32, device=d_set.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_sets, km1 + 1, h, w), tuple(out.shape)
    L.check(L.load().tmix_soft_masks(_p(d_set), _p(d_clear), _p(out), n_sets, km1 + 1, h, w, float(feather), float(dilate),
                                     int(bool(normalize)), _stream()), "tmix_soft_masks")
    return out


def mask_label(map, threshold=0.5, invert=False, out=None):
    """tmix_mask_label: map [n, h, w] fp32 -> int32 [n, h, w]: for every set pixel (map >= threshold; invert=True: every clear pixel) the
    smallest raster index of its 4-connected component, -1 for the pixels of the other kind.  h * w <= L.SHAPE_MAX_PIXELS."""
    _need_cuda(map, out)
    assert map.dtype == torch.float32 and map.is_contiguous() and map.dim() == 3, tuple(map.shape)
    n, h, w = map.shape
    if out is None:
        out = torch.empty(n, h, w, dtype=torch.int32, device=map.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (n, h, w), tuple(out.shape)
    L.check(L.load().tmix_mask_label(_p(map), float(threshold), int(bool(invert)), _p(out), n, h, w, _stream()), "tmix_mask_label")
    return out


def attn_shapes(score, threshold, fill_holes=True, resolve=True, out=None):
    """tmix_attn_shapes: score [n_sets, K-1, h, w] fp32 -> the free-form masks [n_sets, K-1, h, w] fp32 in {0, 1}: per concept the largest
    4-connected component of score >= threshold, with its holes filled (fill_holes) and, within a set, every pixel that several concepts
    claim left to the one with the highest score there (resolve).  include/tmix.h has the definition."""
    _need_cuda(score, out)
    assert score.dtype == torch.float32 and score.is_contiguous() and score.dim() == 4, tuple(score.shape)
    n_sets, km1, h, w = score.shape
    if out is None:
        out = torch.empty(n_sets, km1, h, w, dtype=torch.float32, device=score.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_sets, km1, h, w), tuple(out.shape)
    flags = (L.SHAPE_FILL_HOLES if fill_holes else 0) | (L.SHAPE_RESOLVE if resolve else 0)
    L.check(L.load().tmix_attn_shapes(_p(score), _p(out), n_sets, km1, h, w, float(threshold), flags, _stream()), "tmix_attn_shapes")
    return out


def stats_parts(N, tile_cfg):
    """number of row-statistics partials a GEMM of width N writes with tiling tile_cfg (tmix_gemm_stats_parts)."""
    n = L.load().tmix_gemm_stats_parts(int(N), int(tile_cfg))
    assert n > 0, (N, tile_cfg)
    return n


def f8copy_tile(tile_cfg):
    """the tiling the library runs in place of tile_cfg when a bf16 GEMM also leaves the e4m3 copy of its output (tmix_gemm_f8copy_tile)."""
    n = L.load().tmix_gemm_f8copy_tile(int(tile_cfg))
    return n if n > 0 else tile_cfg              # (AUTO and ids out of range pass through: the launch itself deals with them)


def conv_runs_as(d, tile_cfg):
    """the tiling of the kernel the bf16 convolution d (a ConvDesc) would run if it asked for tile_cfg (tmix_conv_resolve_tile); another id: tile_cfg is an alias."""
    asked, d.tile_cfg = d.tile_cfg, int(tile_cfg)
    n = L.load().tmix_conv_resolve_tile(C.byref(d), 0)
    d.tile_cfg = asked
    if n < 0:
        L.check(n, "tmix_conv_resolve_tile")
    return n


def make_gemm_desc(a, w, out, bias=None, residual=None, rowgroup_bias=None, rows_per_group=0, geglu=False,
                   out_t=None, n_trans_begin=-1, tile_cfg=0, row_stats_out=None, ln_stats=None, ln_colsum=None,
                   ln_eps=1e-5, ln_parts=0, act=None, out_f32=None, ln_k=None, col_stats_out=None):
    """a [batch?,M,K] bf16 (last dim contiguous), w [batch?,N,K] bf16, out [batch?,M,N'] bf16."""
    a3 = a if a.dim() == 3 else a.unsqueeze(0)
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    batch, M, K = a3.shape
    N = w3.shape[1]
    assert a3.dtype == w3.dtype and a3.dtype in (BF16, torch.uint8) and a3.stride(2) == 1 and w3.stride(2) == 1 and w3.shape[2] == K   # uint8 = e4m3 bytes (gemm_fp8)
    d = L.GemmDesc()
    d.A, d.lda, d.strideA = a3.data_ptr(), a3.stride(1), (a3.stride(0) if batch > 1 else 0)
    d.W, d.ldw, d.strideW = w3.data_ptr(), w3.stride(1), (w3.stride(0) if w3.shape[0] > 1 else 0)
    P = w3.shape[0]
    assert P in (1, batch) or batch % P == 0          # P weight sets for a batch of several x P rows: slice b reads set b % P (tmix_gemm_desc.w_period)
    d.w_period = P if 1 < P < batch else 0
    if out is not None:
        o3 = out if out.dim() == 3 else out.unsqueeze(0)
        assert o3.dtype == BF16 and o3.stride(2) == 1
        d.C, d.ldc, d.strideC = o3.data_ptr(), o3.stride(1), (o3.stride(0) if batch > 1 else 0)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.stride(-1) == 1
        d.bias = bias.data_ptr()
        d.strideBias = bias.stride(0) if (bias.dim() == 2 and bias.shape[0] > 1) else 0
        assert bias.dim() == 1 or bias.shape[0] in (1, P)
    if residual is not None:
        r3 = residual if residual.dim() == 3 else residual.unsqueeze(0)
        assert r3.dtype == BF16 and r3.stride(2) == 1
        d.residual, d.ldr, d.strideR = r3.data_ptr(), r3.stride(1), (r3.stride(0) if batch > 1 else 0)
    if rowgroup_bias is not None:
        assert rowgroup_bias.dtype == torch.float32 and rowgroup_bias.is_contiguous()
        d.rowgroup_bias, d.rows_per_group = rowgroup_bias.data_ptr(), rows_per_group
    d.n_trans_begin = -1
    if out_t is not None:
        t3 = out_t if out_t.dim() == 3 else out_t.unsqueeze(0)
        assert t3.dtype == BF16 and t3.stride(2) == 1
        d.Ct, d.ldct, d.strideCt = t3.data_ptr(), t3.stride(1), (t3.stride(0) if batch > 1 else 0)
        d.n_trans_begin = n_trans_begin
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.epilogue = L.EPI_GEGLU if geglu else {None: L.EPI_NONE, "gelu": L.EPI_GELU, "quick_gelu": L.EPI_QUICKGELU}[act]
    if out_f32 is not None:                # fp32 C (attention scores): [batch?, M, ld >= N]
        f3 = out_f32 if out_f32.dim() == 3 else out_f32.unsqueeze(0)
        assert f3.dtype == torch.float32 and f3.stride(2) == 1 and out is None and act is None and not geglu
        d.C, d.ldc, d.strideC, d.epilogue = f3.data_ptr(), f3.stride(1), (f3.stride(0) if batch > 1 else 0), L.EPI_F32OUT
    d.tile_cfg = tile_cfg
    if row_stats_out is not None:          # fp32 [parts, rows, 2] per-column-tile partial sums, rows = batch*M
        st = row_stats_out
        assert st.dtype == torch.float32 and st.is_contiguous() and st.dim() == 3 and st.shape[1:] == (batch * M, 2)
        assert tile_cfg > 0 and st.shape[0] >= stats_parts(N, tile_cfg)
        d.row_stats_out, d.strideStatsOut, d.ldStatsOut = st.data_ptr(), 2 * M, st.shape[1]
    if ln_stats is not None:               # fused LayerNorm on the A rows (see include/tmix.h)
        st = ln_stats
        assert st.dtype == torch.float32 and st.is_contiguous() and st.dim() == 3 and st.shape[1:] == (batch * M, 2)
        assert ln_colsum is not None and ln_colsum.dtype == torch.float32 and ln_colsum.is_contiguous()
        assert ln_colsum.shape in ((N,), (P, N))
        d.ln_stats, d.strideLnStats, d.ldLnStats = st.data_ptr(), 2 * M, st.shape[1]
        d.ln_parts = int(ln_parts) if ln_parts else st.shape[0]
        d.ln_colsum, d.strideLnColsum = ln_colsum.data_ptr(), (N if ln_colsum.dim() == 2 and batch > 1 else 0)
        d.ln_inv_c, d.ln_eps = 1.0 / (ln_k or K), ln_eps       # ln_k: the LayerNorm's width when A carries extra columns behind it (low-rank LoRA pad)
    if col_stats_out is not None:          # GroupNorm partials of the stored rows: fp32 [M/32, 2, N] (colstats_buf)
        cs = col_stats_out
        assert batch == 1 and cs.dtype == torch.float32 and cs.is_contiguous() and tuple(cs.shape) == (M // COLSTATS_ROWS, 2, N) and M % COLSTATS_ROWS == 0
        d.col_stats_out = cs.data_ptr()
    return d


COLSTATS_ROWS = 32          # TMIX_COLSTATS_ROWS
# largest image (pixels) whose GroupNorms take their statistics from the producers: the combine launch walks HW / 32 partials per channel, and beyond
# 128 x 128 that pass loses to the statistics kernel's pass over x itself (VAE decode at 1024^2, all levels on the partials: 15.4 vs 14.7 ms)
COLSTATS_MAX_HW = 16384


def colstats_buf(rows, C, device):
    """receiver of tmix_gemm_desc.col_stats_out / tmix_conv_desc.col_stats_out for an output of `rows` x C: fp32 [rows/32, 2, C],
    plane 0 = column sums, plane 1 = column sums of squares over each 32-row block of the stored bf16 values."""
    assert rows % COLSTATS_ROWS == 0 and C % 8 == 0
    return torch.empty(rows // COLSTATS_ROWS, 2, C, device=device, dtype=torch.float32)


class F8Copy:
    """Receiver of TMIX_F8_COPY_OUT: one byte buffer holding the e4m3 copy [rows, N] of a GEMM's bf16 output and, behind it,
    the MX block scales [N/32, rows] -- the pair tmix_gemm_fp8 takes as a block-scaled A operand."""

    @staticmethod
    def bytes_for(rows, N):
        return (rows * N + 255) // 256 * 256 + (N // 32) * rows

    def __init__(self, rows, N, device, buf=None):
        self.rows, self.N = rows, N
        self.off = (rows * N + 255) // 256 * 256
        self.nbytes = self.off + (N // 32) * rows
        self.buf = buf if buf is not None else torch.empty(self.nbytes, device=device, dtype=torch.uint8)
        assert self.buf.numel() >= self.nbytes and self.buf.dtype == torch.uint8
        self.q = self.buf[:rows * N].view(rows, N)
        self.scales = self.buf[self.off:self.off + (N // 32) * rows].view(N // 32, rows)

    def attach(self, d):
        assert d.batch * d.M == self.rows and d.N == self.N
        d.Ct, d.ldct, d.strideCt = self.buf.data_ptr(), self.N, self.off
        d.reserved0 |= L.F8_COPY_OUT


def gemm(a, w, out=None, f8_copy=None, **kw):
    """out = epi(a @ w^T).  Allocates out ([.., M, N] or [.., M, N/2] for GEGLU) when not given.
    f8_copy: an F8Copy that also receives the e4m3 + MX-block-scale copy of the stored rows."""
    _need_cuda(a, w)
    lib = L.load()
    if out is None and kw.get("out_f32") is None and not (kw.get("out_t") is not None and kw.get("n_trans_begin", -1) == 0):
        N = w.shape[-2]
        No = N // 2 if kw.get("geglu") else N
        if kw.get("out_t") is not None:
            No = kw["n_trans_begin"]
        out = torch.empty(*a.shape[:-1], No, device=a.device, dtype=BF16)
    d = make_gemm_desc(a, w, out, **kw)
    if f8_copy is not None:
        f8_copy.attach(d)
    L.check(lib.tmix_gemm_bf16(C.byref(d), _stream()), "tmix_gemm_bf16")
    return out if out is not None else kw.get("out_f32")


def q_cross_attn_args(k, vt, out, rows_per_image, scale):
    """the arguments of tmix_gemm_q_cross_attn behind its descriptor: cached K [images, Skv, C], V^T [images, C, 80], output [rows, C]"""
    assert k.dtype == BF16 and vt.dtype == BF16 and out.dtype == BF16 and k.stride(2) == 1 and vt.stride(2) == 1 and out.stride(-1) == 1
    o2 = out.reshape(-1, out.shape[-1])
    assert o2.data_ptr() == out.data_ptr()
    return (k.data_ptr(), k.stride(1), k.stride(0), vt.data_ptr(), vt.stride(1), vt.stride(0), o2.data_ptr(), o2.stride(0),
            int(rows_per_image), int(k.shape[1]), float(scale))


def gemm_q_cross_attn(a, w, k, vt, rows_per_image, scale, out=None, **kw):
    """attn2 in one launch (tmix_gemm_q_cross_attn): softmax((a @ w^T [+ bias, folded LayerNorm]) K^T * scale) V per 64-wide head.
    a [batch?, M, C], w [batch?, C, C]; k [images, Skv <= 80, C], vt [images, C, 80]; returns the attention output [batch?, M, C]."""
    _need_cuda(a, w, k, vt)
    if out is None:
        out = torch.empty(*a.shape[:-1], w.shape[-2], device=a.device, dtype=BF16)
    d = make_gemm_desc(a, w, None, **kw)
    L.check(L.load().tmix_gemm_q_cross_attn(C.byref(d), *q_cross_attn_args(k, vt, out, rows_per_image, scale), _stream()), "tmix_gemm_q_cross_attn")
    return out


def quantize_fp8_rows(x, q=None, scale=None):
    """x bf16 [..., K] (rows contiguous in K) -> (q uint8 [..., K] holding OCP e4m3 bytes, scale uint8 [...] E8M0 exponents):
    x[r] ~= e4m3(q[r]) * 2^(scale[r] - 127)."""
    _need_cuda(x)
    assert x.dtype == BF16 and x.stride(-1) == 1
    K = x.shape[-1]
    if K > 8192:                       # rows longer than the kernel keeps in registers (conv weight rows: 9 * Cin): the same arithmetic in torch, once per checkpoint
        xf = x.float()
        amax = xf.abs().amax(dim=-1)
        # e8m0_for_amax (csrc/common.h), bit for bit: the fp32 product amax * fl(1/448), its exponent, + 1 when the mantissa is not zero
        bits = (amax.float() * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=amax.device)).view(torch.int32)
        e = (((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)).clamp(-127, 127)
        e = torch.where(amax > 0, e, torch.zeros_like(e)).float()
        qt = (xf * torch.exp2(-e).unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
        st = (e + 127).to(torch.uint8)
        if q is not None:
            q.copy_(qt); qt = q
        if scale is not None:
            scale.copy_(st); st = scale
        return qt.contiguous(), st.contiguous()
    x2 = x.reshape(-1, K)
    if q is None:
        q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    if scale is None:
        scale = torch.empty(x.shape[:-1], device=x.device, dtype=torch.uint8)
    q2 = q.view(-1, K)
    L.check(L.load().tmix_quantize_fp8_rows(x2.data_ptr(), x2.stride(0), q2.data_ptr(), q2.stride(0), scale.data_ptr(), x2.shape[0], K,
                                            _stream()), "tmix_quantize_fp8_rows")
    return q, scale


def dequantize_fp8_rows(q, scale):
    """fp32 values of (q, scale) as tmix_gemm_fp8 reads them (tests / error measurements)."""
    return q.view(torch.float8_e4m3fn).float() * torch.exp2(scale.float() - 127.0).unsqueeze(-1)


def gemm_fp8(a8, sa, w8, sw, out=None, a_block_scales=False, f8_out=None, f8_copy=None, **kw):
    """gemm() on e4m3 operands with per-row E8M0 scales (tmix_gemm_fp8): a8 [.., M, K] uint8 + sa [.., M]; w8 [.., N, K] + sw [.., N].
    a_block_scales: sa is the MX block form [K/32, rows] (k-block major) instead.
    f8_out=(c8 uint8 [.., M, N/2], scales uint8 [N/64, rows]) with geglu=True: the GEGLU result leaves as e4m3 + block scales."""
    _need_cuda(a8, w8, sa, sw)
    lib = L.load()
    if f8_out is not None:
        c8, cs = f8_out
        assert kw.get("geglu") and c8.dtype == torch.uint8 and cs.dtype == torch.uint8 and cs.is_contiguous() and c8.stride(-1) == 1
        d = make_gemm_desc(a8, w8, None, **kw)
        c3 = c8 if c8.dim() == 3 else c8.unsqueeze(0)
        d.C, d.ldc, d.strideC = c3.data_ptr(), c3.stride(1), (c3.stride(0) if c3.shape[0] > 1 else 0)
        d.Ct, d.ldct = cs.data_ptr(), cs.shape[1]
        d.reserved0 = L.F8_GEGLU_OUT | (L.F8_A_BLOCK_SCALES if a_block_scales else 0)
        L.check(lib.tmix_gemm_fp8(C.byref(d), sa.data_ptr(), sw.data_ptr(), _stream()), "tmix_gemm_fp8")
        return c8, cs
    if out is None and kw.get("out_f32") is None:
        N = w8.shape[-2]
        No = N // 2 if kw.get("geglu") else (kw["n_trans_begin"] if kw.get("out_t") is not None else N)
        out = torch.empty(*a8.shape[:-1], No, device=a8.device, dtype=BF16)
    assert sa.dtype == torch.uint8 and sw.dtype == torch.uint8 and sa.is_contiguous() and sw.is_contiguous()
    d = make_gemm_desc(a8, w8, out, **kw)
    if a_block_scales:
        assert sa.dim() == 2 and sa.shape[0] == a8.shape[-1] // 32
        d.reserved0 = L.F8_A_BLOCK_SCALES
    if f8_copy is not None:
        f8_copy.attach(d)
    L.check(lib.tmix_gemm_fp8(C.byref(d), sa.data_ptr(), sw.data_ptr(), _stream()), "tmix_gemm_fp8")
    return out if out is not None else kw.get("out_f32")


def make_conv_desc(x, w, out, bias=None, batch_bias=None, residual=None, mode=L.CONV_S1, tile_cfg=0, bias_images=1, col_stats_out=None,
                   shortcut=None, _fp8=False):
    """x [B,H,W,Cin] bf16 NHWC contiguous; w [Cout,3,3,Cin] bf16 contiguous ([Cout,3,Cin] for the temporal CONV_T3,
    where x is [clips, frames, h*w, Cin]; [4,Cout,2,2,Cin] for CONV_UP2F: fold_up2_weight).
    shortcut: (s1, s2 or None) -- NHWC tensors whose 1x1 conv_shortcut rides in the same K loop; w is then the 2-d [Cout, 9*Cin + C(s1) + C(s2)]
    matrix [conv taps | shortcut weights] (shortcut_weight) and bias the sum of the two biases."""
    B, H, W, Cin = x.shape
    Cout = w.shape[1] if mode == L.CONV_UP2F else w.shape[0]
    dt = torch.uint8 if _fp8 else BF16                  # (e4m3 bytes: tmix_conv3x3_nhwc_fp8)
    assert x.dtype == dt and w.dtype == dt and x.is_contiguous() and w.is_contiguous() and out.is_contiguous()
    if shortcut is not None:
        s1, s2 = shortcut
        c1, c2 = s1.shape[-1], (0 if s2 is None else s2.shape[-1])
        assert mode == L.CONV_S1 and tuple(w.shape) == (Cout, 9 * Cin + c1 + c2) and residual is None
        assert s1.dtype == BF16 and s1.is_contiguous() and s1.numel() == B * H * W * c1 and (s2 is None or (s2.dtype == BF16 and s2.is_contiguous() and s2.numel() == B * H * W * c2))
    else:
        assert tuple(w.shape) == ((Cout, 3, Cin) if mode == L.CONV_T3 else (4, Cout, 2, 2, Cin) if mode == L.CONV_UP2F else (Cout, 3, 3, Cin))
    d = L.ConvDesc()
    d.X, d.Wt, d.Y = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias, d.batch_bias, d.residual = _p(bias), _p(batch_bias), _p(residual)
    d.B, d.H, d.W, d.Cin, d.Cout, d.mode = B, H, W, Cin, Cout, mode
    d.tile_cfg = tile_cfg
    d.batch_bias_images = bias_images      # consecutive images sharing one batch_bias row (video: frames of a clip)
    if col_stats_out is not None:
        cs = col_stats_out
        assert cs.dtype == torch.float32 and cs.is_contiguous() and tuple(cs.shape) == (out.numel() // Cout // COLSTATS_ROWS, 2, Cout)
        d.col_stats_out = cs.data_ptr()
    if shortcut is not None:
        d.S1, d.S1_channels = s1.data_ptr(), c1
        if s2 is not None:
            d.S2, d.S2_channels = s2.data_ptr(), c2
    return d


def shortcut_weight(w_conv, w_sc):
    """[Cout, 9*Cin + Csc]: the OHWI taps of a 3x3 conv followed by the [Cout, Csc] weights of the 1x1 shortcut that shares its launch"""
    Cout = w_conv.shape[0]
    return torch.cat([w_conv.reshape(Cout, -1), w_sc.reshape(Cout, -1)], dim=1).contiguous()


def conv_out_hw(H, W, mode):
    return (H // 2, W // 2) if mode in (L.CONV_S2, L.CONV_S2A) else ((2 * H, 2 * W) if mode in (L.CONV_UP2, L.CONV_UP2F) else (H, W))


def fold_up2_weight(w_ohwi, dtype=BF16):
    """the weights of TMIX_CONV_UP2F from those of a 3x3 convolution behind a nearest x2 upsampling: w [Cout,3,3,Cin] (OHWI) -> [4,Cout,2,2,Cin],
    phase = 2 fy + fx major.  Output row 2 sy + fy touches source rows sy-1, sy, sy (fy = 0) or sy, sy, sy+1 (fy = 1), so the row taps of phase fy are
    {ky=0}, {ky=1,2} resp. {ky=0,1}, {ky=2}; columns alike.  Summed in fp32 (fp64 input: in fp64) and rounded once to `dtype` (None: not at all)."""
    assert w_ohwi.dim() == 4 and tuple(w_ohwi.shape[1:3]) == (3, 3)
    w = w_ohwi.to(torch.float64 if w_ohwi.dtype == torch.float64 else torch.float32)
    phases = []
    for fy in (0, 1):
        wy = torch.stack([w[:, 0], w[:, 1] + w[:, 2]] if fy == 0 else [w[:, 0] + w[:, 1], w[:, 2]], dim=1)                    # [Cout, 2, 3, Cin]
        for fx in (0, 1):
            phases.append(torch.stack([wy[:, :, 0], wy[:, :, 1] + wy[:, :, 2]] if fx == 0 else [wy[:, :, 0] + wy[:, :, 1], wy[:, :, 2]], dim=2))
    out = torch.stack(phases)                                                                                                    # [4, Cout, 2, 2, Cin]
    return (out if dtype is None else out.to(dtype)).contiguous()


def up2_fold_enabled():
    """the process-wide A/B switch: TMIX_UP2_FOLD=0 makes every plan keep the TMIX_CONV_UP2 launches (9 taps gathered from the upsampled coordinates)"""
    return os.environ.get("TMIX_UP2_FOLD", "1") != "0"


def up2_fold_ok(H, W):
    """do the plan builders run the upsampler conv over an H x W source as TMIX_CONV_UP2F?  The kernel needs H * W to be a multiple of the row count of the
    tile that runs it; the builders ask for a multiple of 256 -- the tallest tile -- so that EVERY tiling the tuner may pick accepts the launch."""
    return up2_fold_enabled() and W >= 2 and (H * W) % 256 == 0


def conv3x3_fp8(x8, sx, w8, sw, bias=None, batch_bias=None, residual=None, mode=L.CONV_S1, out=None, tile_cfg=12, col_stats_out=None, bias_images=1):
    """conv3x3 on e4m3 operands (tmix_conv3x3_nhwc_fp8): x8 uint8 [B,H,W,Cin] + sx uint8 [B*H*W, Cin/32] (row-major MX blocks, as groupnorm(f8_out=) writes);
    w8 uint8 [Cout,3,3,Cin] (or [Cout,3,Cin]) + sw uint8 [Cout] (quantize_fp8_rows over the flattened weight rows)."""
    _need_cuda(x8, w8, sx, sw)
    lib = L.load()
    B, H, W, Cin = x8.shape
    Ho, Wo = conv_out_hw(H, W, mode)
    if out is None:
        out = torch.empty(B, Ho, Wo, w8.shape[0], device=x8.device, dtype=BF16)
    assert x8.dtype == torch.uint8 and w8.dtype == torch.uint8 and sx.dtype == torch.uint8 and sw.dtype == torch.uint8
    assert x8.is_contiguous() and w8.is_contiguous() and sx.is_contiguous() and sw.is_contiguous() and sx.numel() == B * H * W * Cin // 32 and sw.numel() == w8.shape[0]
    d = make_conv_desc(x8, w8, out, bias, batch_bias, residual, mode, tile_cfg, bias_images=bias_images, col_stats_out=col_stats_out, _fp8=True)
    L.check(lib.tmix_conv3x3_nhwc_fp8(C.byref(d), sx.data_ptr(), sw.data_ptr(), _stream()), "tmix_conv3x3_nhwc_fp8")
    return out


def conv3x3(x, w, bias=None, batch_bias=None, residual=None, mode=L.CONV_S1, out=None, tile_cfg=0, col_stats_out=None, shortcut=None):
    _need_cuda(x, w)
    lib = L.load()
    B, H, W, _ = x.shape
    Ho, Wo = conv_out_hw(H, W, mode)
    if out is None:
        out = torch.empty(B, Ho, Wo, w.shape[1] if mode == L.CONV_UP2F else w.shape[0], device=x.device, dtype=BF16)
    d = make_conv_desc(x, w, out, bias, batch_bias, residual, mode, tile_cfg, col_stats_out=col_stats_out, shortcut=shortcut)
    L.check(lib.tmix_conv3x3_nhwc(C.byref(d), _stream()), "tmix_conv3x3_nhwc")
    return out


def conv_in(x_nchw, w_ohwi, bias, out=None, pre_w=None, pre_b=None):
    """fp32 NCHW [B,Cin,H,W] -> bf16 NHWC [B,H,W,Cout]; w fp32 [Cout,3,3,Cin].  pre_w [4,4] (and pre_b [4]), HOST values: tmix_conv_in_pre, the
    per-pixel linear map of a 4-channel latent in front of the convolution (the padding stays zero)."""
    _need_cuda(x_nchw, w_ohwi)
    lib = L.load()
    B, Cin, H, W = x_nchw.shape
    Cout = w_ohwi.shape[0]
    assert x_nchw.dtype == torch.float32 and w_ohwi.dtype == torch.float32 and x_nchw.is_contiguous() and w_ohwi.is_contiguous()
    if out is None:
        out = torch.empty(B, H, W, Cout, device=x_nchw.device, dtype=BF16)
    if pre_w is None:
        assert pre_b is None, "pre_b without pre_w"
        L.check(lib.tmix_conv_in(_p(x_nchw), _p(w_ohwi), _p(bias), _p(out), B, Cin, H, W, Cout, _stream()), "tmix_conv_in")
        return out
    pw = torch.as_tensor(pre_w, dtype=torch.float32, device="cpu").contiguous()          # the entry reads the map on the host
    pb = None if pre_b is None else torch.as_tensor(pre_b, dtype=torch.float32, device="cpu").contiguous()
    assert pw.numel() == 16 and (pb is None or pb.numel() == 4)
    L.check(lib.tmix_conv_in_pre(_p(x_nchw), _p(w_ohwi), _p(bias), _p(out), B, Cin, H, W, Cout, _p(pw), _p(pb), _stream()), "tmix_conv_in_pre")
    return out


def conv_out(x_nhwc, w_ohwi, bias, out=None):
    """bf16 NHWC [B,H,W,Cin] -> fp32 NCHW [B,Cout,H,W]; w bf16 [Cout,3,3,Cin]."""
    _need_cuda(x_nhwc, w_ohwi)
    lib = L.load()
    B, H, W, Cin = x_nhwc.shape
    Cout = w_ohwi.shape[0]
    assert x_nhwc.dtype == BF16 and w_ohwi.dtype == BF16 and x_nhwc.is_contiguous() and w_ohwi.is_contiguous()
    if out is None:
        out = torch.empty(B, Cout, H, W, device=x_nhwc.device, dtype=torch.float32)
    L.check(lib.tmix_conv_out(_p(x_nhwc), _p(w_ohwi), _p(bias), _p(out), B, Cin, H, W, Cout, _stream()), "tmix_conv_out")
    return out


def attention_split_ws(B, H, Sq, Skv, device):
    """zero-filled workspace that lets tmix_attn_fwd_ws cut the items of a partly filled last round into key ranges (None: this shape does not split).
    One per stream that runs attention; the launches leave its ticket counters at zero."""
    n = L.load().tmix_attn_split_ws_bytes(B, H, Sq, Skv)
    return torch.zeros(n, device=device, dtype=torch.uint8) if n > 0 else None


def attention(q, k, vt, H, Skv, scale, out=None, f8_out=None, ws=None):
    """q [B,Sq,>=H*64] bf16 (row stride free), k [B,>=Skv,..] bf16, vt [B,H*64,ldvt] bf16 (V transposed).
    f8_out: an F8Copy(B * Sq, H * 64) that receives the output as e4m3 + MX block scales INSTEAD of the bf16 tensor (tmix_attn_fwd_f8).
    ws: attention_split_ws(...) buffer (at least as large as this shape needs) -> the key-split tail (tmix_attn_fwd_ws / tmix_attn_fwd_f8_ws)."""
    _need_cuda(q, k, vt)
    lib = L.load()
    B, Sq = q.shape[0], q.shape[1]
    assert q.dtype == BF16 and k.dtype == BF16 and vt.dtype == BF16
    assert q.stride(2) == 1 and k.stride(2) == 1 and vt.stride(2) == 1
    wsa = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    if f8_out is not None:
        assert f8_out.rows == B * Sq and f8_out.N == H * 64
        L.check(lib.tmix_attn_fwd_f8_ws(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0), _p(vt), vt.stride(1), vt.stride(0),
                                        f8_out.q.data_ptr(), f8_out.N, f8_out.scales.data_ptr(), f8_out.rows,
                                        B, H, Sq, Skv, float(scale), *wsa, _stream()), "tmix_attn_fwd_f8_ws")
        return f8_out
    if out is None:
        out = torch.empty(B, Sq, H * 64, device=q.device, dtype=BF16)
    L.check(lib.tmix_attn_fwd_ws(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0),
                                 _p(vt), vt.stride(1), vt.stride(0), _p(out), out.stride(1), out.stride(0),
                                 B, H, Sq, Skv, float(scale), *wsa, _stream()), "tmix_attn_fwd_ws")
    return out


def token_array(tokens):
    """the host int32 array tmix_xattn_token_maps reads its positions from (at the call; a plan keeps it with its arguments)"""
    tokens = [int(t) for t in tokens]
    return (C.c_int32 * max(1, len(tokens)))(*tokens)


XATTN_MAPS_SHORT = (80, 8)        # (keys, positions) of tmix_xattn_token_maps; beyond either: tmix_xattn_token_maps_long (240, 32)


def xattn_maps_long(Lk, n_tok):
    """does a token-map launch over Lk keys and n_tok positions need tmix_xattn_token_maps_long?"""
    return Lk > XATTN_MAPS_SHORT[0] or n_tok > XATTN_MAPS_SHORT[1]


def xattn_token_maps(q, k, tokens, H, Lk=None, rows=(0, 1, None), scale=None, out=None, accumulate=False, long=None):
    """maps [n_rows, n_tok, Sq] fp32: softmax(q k^T * scale) of every head at the key positions `tokens` (<= 8), summed over the
    H heads, for batch rows row0 + i * row_step (rows = (row0, row_step, n_rows); n_rows None: every row from row0 on).
    q [B,Sq,>=H*64] bf16 (row stride free), k [B,>=Lk,>=H*64] bf16.  accumulate adds to `out` instead of overwriting it.
    long: call tmix_xattn_token_maps_long (Lk <= 240, <= 32 positions); None = only where the short entry point cannot serve."""
    _need_cuda(q, k)
    assert q.dtype == BF16 and k.dtype == BF16 and q.stride(2) == 1 and k.stride(2) == 1
    B, Sq = q.shape[0], q.shape[1]
    Lk = k.shape[1] if Lk is None else Lk
    row0, step, n = rows
    n = len(range(row0, B, step)) if n is None else n
    if out is None:
        out = torch.zeros(n, len(tokens), Sq, device=q.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, len(tokens), Sq)
    scale = 64 ** -0.5 if scale is None else scale
    long = xattn_maps_long(Lk, len(tokens)) if long is None else long
    fn = L.load().tmix_xattn_token_maps_long if long else L.load().tmix_xattn_token_maps
    L.check(fn(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0), _p(out), B, H, Sq, Lk,
               row0, step, n, token_array(tokens), len(tokens), int(bool(accumulate)), float(scale),
               _stream()), fn.__name__)
    return out


def sattn_propagate(q, k, src, H, rows=(0, 1, None), scale=None, out=None, accumulate=False, out_scale=1.0):
    """out [n_rows, n_tok, S] fp32 (+)= out_scale * sum over the H heads of softmax(q k^T * scale) @ src: the maps `src`
    [n_rows, n_tok <= 32, S] fp32 pushed through the self-attention of batch rows row0 + i * row_step (rows = (row0, row_step, n_rows);
    n_rows None: every row from row0 on).  q, k [B,S,>=H*64] bf16 (row stride free: the two halves of one q/k buffer serve).
    accumulate adds to `out` instead of overwriting it; `out` must not alias `src`."""
    _need_cuda(q, k, src)
    assert q.dtype == BF16 and k.dtype == BF16 and q.stride(2) == 1 and k.stride(2) == 1 and q.shape[:2] == k.shape[:2]
    B, S = q.shape[0], q.shape[1]
    row0, step, n = rows
    n = len(range(row0, B, step)) if n is None else n
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3 and src.shape[0] == n and src.shape[2] == S
    if out is None:
        out = torch.zeros_like(src)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == src.shape
    scale = 64 ** -0.5 if scale is None else scale
    L.check(L.load().tmix_sattn_propagate(_p(q), q.stride(1), q.stride(0), _p(k), k.stride(1), k.stride(0), _p(src), _p(out), B, H, S,
                                          row0, step, n, src.shape[1], int(bool(accumulate)), float(scale), float(out_scale),
                                          _stream()), "tmix_sattn_propagate")
    return out


def groupnorm_ws(B, C, groups, device):
    return torch.empty(L.load().tmix_groupnorm_ws_floats(B, C, groups), device=device, dtype=torch.float32)


def groupnorm(x1, gamma, beta, groups=32, eps=1e-5, silu=False, x2=None, out=None, ws=None, colstats=None, f8_out=None):
    """x1 [B,HW,C1] (+ optional x2 [B,HW,C2], normalised as channel-concat) bf16 NHWC.
    colstats: (cs1, cs2 or None) -- the column partials the tensor's producers left (colstats_buf; their channel counts add up to C1 + C2 but
    need not be C1 and C2): tmix_groupnorm_nhwc_pre, no statistics pass."""
    _need_cuda(x1, gamma, beta)
    lib = L.load()
    B, HW, C1 = x1.shape[0], x1.numel() // (x1.shape[0] * x1.shape[-1]), x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    assert x1.is_contiguous() and (x2 is None or x2.is_contiguous()) and gamma.dtype == torch.float32
    assert f8_out is None or colstats is not None, "the e4m3 output exists for the producer-statistics form (tmix_groupnorm_nhwc_pre_f8)"
    if out is None and f8_out is None:
        out = torch.empty(*x1.shape[:-1], C1 + C2, device=x1.device, dtype=BF16)
    if ws is None:
        ws = groupnorm_ws(B, C1 + C2, groups, x1.device)
    if colstats is not None:
        cs1, cs2 = colstats
        ca, cb = cs1.shape[-1], (0 if cs2 is None else cs2.shape[-1])
        assert cs1.is_contiguous() and cs1.shape[1] == 2 and (cs2 is None or (cs2.is_contiguous() and cs2.shape[:2] == cs1.shape[:2]))
        if HW % COLSTATS_ROWS == 0:
            assert cs1.shape[0] == B * HW // COLSTATS_ROWS
        if f8_out is not None:                             # (y8 uint8 [.., C], s8 uint8 [pixels, C / 32]): e4m3 + row-major MX scales instead of bf16
            y8, s8 = f8_out
            assert y8.dtype == torch.uint8 and s8.dtype == torch.uint8 and y8.is_contiguous() and s8.is_contiguous()
            assert y8.numel() == B * HW * (C1 + C2) and s8.numel() == B * HW * (C1 + C2) // 32
            L.check(lib.tmix_groupnorm_nhwc_pre_f8(_p(x1), C1, _p(x2), C2, _p(y8), _p(s8), _p(gamma), _p(beta), _p(ws), B, HW, groups,
                                                   float(eps), int(bool(silu)), _p(cs1), ca, _p(cs2), cb, _stream()), "tmix_groupnorm_nhwc_pre_f8")
            return f8_out
        L.check(lib.tmix_groupnorm_nhwc_pre(_p(x1), C1, _p(x2), C2, _p(out), _p(gamma), _p(beta), _p(ws), B, HW, groups,
                                            float(eps), int(bool(silu)), _p(cs1), ca, _p(cs2), cb, _stream()), "tmix_groupnorm_nhwc_pre")
        return out
    L.check(lib.tmix_groupnorm_nhwc(_p(x1), C1, _p(x2), C2, _p(out), _p(gamma), _p(beta), _p(ws), B, HW, groups,
                                    float(eps), int(bool(silu)), _stream()), "tmix_groupnorm_nhwc")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _need_cuda(x, gamma, beta)
    lib = L.load()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    assert x.is_contiguous() and x.dtype == BF16 and gamma.dtype == torch.float32
    if out is None:
        out = torch.empty_like(x)
    L.check(lib.tmix_layernorm(_p(x), _p(out), _p(gamma), _p(beta), rows, Cc, float(eps), _stream()), "tmix_layernorm")
    return out


def concat_channels(x1, x2, out=None):
    _need_cuda(x1, x2)
    lib = L.load()
    C1, C2 = x1.shape[-1], x2.shape[-1]
    rows = x1.numel() // C1
    assert x1.is_contiguous() and x2.is_contiguous() and x1.dtype == BF16 and x2.dtype == BF16
    if out is None:
        out = torch.empty(*x1.shape[:-1], C1 + C2, device=x1.device, dtype=BF16)
    L.check(lib.tmix_concat_channels(_p(x1), C1, _p(x2), C2, _p(out), rows, _stream()), "tmix_concat_channels")
    return out


def timestep_embedding(values, dim, out=None):
    _need_cuda(values)
    lib = L.load()
    assert values.dtype == torch.float32 and values.is_contiguous()
    n = values.numel()
    if out is None:
        out = torch.empty(n, dim, device=values.device, dtype=torch.float32)
    L.check(lib.tmix_timestep_embedding(_p(values), _p(out), n, dim, _stream()), "tmix_timestep_embedding")
    return out


def linear_small_sections(x, w, bias, sec_starts, act_in=False, out=None):
    """x [M<=256,K] fp32 against weight matrices stacked along N (w [N,K] bf16, sec_starts int32 device [nsec+1]):
    returns the flat fp32 buffer whose slice [sec_starts[s]*M, sec_starts[s+1]*M) is section s as a dense [M, width_s] matrix."""
    _need_cuda(x, w, sec_starts)
    lib = L.load()
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == BF16 and w.is_contiguous() and w.shape[1] == K
    assert sec_starts.dtype == torch.int32 and sec_starts.is_contiguous()
    if out is None:
        out = torch.empty(M * N, device=x.device, dtype=torch.float32)
    L.check(lib.tmix_linear_small_sections(_p(x), _p(w), _p(bias), _p(out), M, N, K, int(bool(act_in)), _p(sec_starts),
                                           sec_starts.numel() - 1, _stream()), "tmix_linear_small_sections")
    return out


def linear_small(x, w, bias=None, add=None, act_in=False, act_out=False, out=None):
    """x [M<=256,K] fp32, w [N,K] bf16 -> [M,N] fp32."""
    _need_cuda(x, w)
    lib = L.load()
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == BF16 and w.is_contiguous() and w.shape[1] == K
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    L.check(lib.tmix_linear_small(_p(x), _p(w), _p(bias), _p(add), _p(out), M, N, K, int(bool(act_in)),
                                  int(bool(act_out)), _stream()), "tmix_linear_small")
    return out


def _f32c(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "fp32 contiguous tensors"


def conv3x3_f32(x, w, bias=None, stride=1, silu=False):
    """x [B,Cin,H,W] fp32 NCHW, w [Cout,Cin,3,3] fp32 (checkpoint layout), padding 1 -> [B,Cout,OH,OW] fp32 (tmix_conv3x3_f32)."""
    _need_cuda(x, w)
    _f32c(x, w, bias)
    B, Ci, H, W_ = x.shape
    Co = w.shape[0]
    assert tuple(w.shape) == (Co, Ci, 3, 3)
    y = torch.empty(B, Co, (H - 1) // stride + 1, (W_ - 1) // stride + 1, device=x.device, dtype=torch.float32)
    L.check(L.load().tmix_conv3x3_f32(_p(x), _p(w), _p(bias), _p(y), B, Ci, H, W_, Co, int(stride), int(bool(silu)), _stream()), "tmix_conv3x3_f32")
    return y


def adaptive_avgpool_f32(x, oh, ow):
    """torch.nn.AdaptiveAvgPool2d((oh, ow)) on fp32 [..., H, W] (tmix_adaptive_avgpool_f32)."""
    _need_cuda(x)
    _f32c(x)
    H, W_ = x.shape[-2:]
    y = torch.empty(*x.shape[:-2], oh, ow, device=x.device, dtype=torch.float32)
    L.check(L.load().tmix_adaptive_avgpool_f32(_p(x), _p(y), x.numel() // (H * W_), H, W_, int(oh), int(ow), _stream()), "tmix_adaptive_avgpool_f32")
    return y


def linear_f32(x, w, bias=None, act_in=False, act_out=False):
    """x [M<=256,K] fp32, w [N,K] fp32 -> act_out(act_in(x) w^T + bias) [M,N] fp32 (tmix_linear_f32; act = SiLU)."""
    _need_cuda(x, w)
    _f32c(x, w, bias)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    L.check(L.load().tmix_linear_f32(_p(x), _p(w), _p(bias), _p(out), M, N, K, int(bool(act_in)), int(bool(act_out)), _stream()), "tmix_linear_f32")
    return out


def i2v_temporal_encoder(x, clips, frames, p, name):
    """x [clips*frames, 4, H, W] fp32 -> [clips, 4, frames, H, W] fp32: the whole image_latents_temporal_encoder block (tmix_i2v_temporal_encoder);
    p: fp32 state-dict entries under `name` (norm1, attn1.to_q/k/v, attn1.to_out.0, ff.net.0.proj, ff.net.2)."""
    _need_cuda(x)
    BF, Cc, H, W_ = x.shape
    assert BF == clips * frames
    ws = [p[name + k] for k in (".norm1.weight", ".norm1.bias", ".attn1.to_q.weight", ".attn1.to_k.weight", ".attn1.to_v.weight", ".attn1.to_out.0.weight",
                                ".attn1.to_out.0.bias", ".ff.net.0.proj.weight", ".ff.net.0.proj.bias", ".ff.net.2.weight", ".ff.net.2.bias")]
    _f32c(x, *ws)
    want = [(Cc,), (Cc,), (2 * Cc, Cc), (2 * Cc, Cc), (2 * Cc, Cc), (Cc, 2 * Cc), (Cc,), (4 * Cc, Cc), (4 * Cc,), (Cc, 4 * Cc), (Cc,)]
    assert [tuple(w.shape) for w in ws] == want, [tuple(w.shape) for w in ws]
    y = torch.empty(clips, Cc, frames, H, W_, device=x.device, dtype=torch.float32)
    L.check(L.load().tmix_i2v_temporal_encoder(_p(x), _p(y), clips, frames, Cc, H * W_, *[_p(w) for w in ws], _stream()), "tmix_i2v_temporal_encoder")
    return y


def softmax_rows_causal(scores, probs, seq, scale):
    """probs[r, :] = softmax(scale * scores[r, :c<=r%seq]) (bf16), zeros elsewhere; scores fp32 [rows, cols]."""
    _need_cuda(scores, probs)
    rows, cols = scores.shape
    assert scores.dtype == torch.float32 and probs.dtype == BF16 and probs.shape == scores.shape
    L.check(L.load().tmix_softmax_rows_causal(_p(scores), scores.stride(0), _p(probs), probs.stride(0), rows, cols, float(scale),
                                              int(seq), _stream()), "tmix_softmax_rows_causal")
    return probs


def vpred_step(x, v, g, at, at_next, out=None):
    """I2VGen-XL loop update (video_gen/pipeline_i2vgen_xl.py:699-719): x [B,...], v [2B,...] (uncond rows first) of one
    dtype; at / at_next from the un-shifted alpha table.  Returns the next latents (same dtype)."""
    return _vpred_dense(x, v, g, at, step_coeffs(at, at_next)[2:], None, None, out)


def _history(x0_prev, x):
    assert x0_prev.dtype == torch.float32 and x0_prev.is_contiguous() and x0_prev.numel() == x.numel()
    return _p(x0_prev)


def _video_factors(factors, videos):
    assert factors.is_cuda and factors.dtype == torch.float32 and factors.is_contiguous() and factors.numel() == videos, (tuple(factors.shape), videos)
    return _p(factors)


def _vpred_dense(x, v, g, at, move, x0_prev, factors, out):
    """the four dense video step entries: x0_prev None -> the DDIM move, move = (sa_next, s1_next), else the multistep move, move = (cx, c0, c1) and
    tmix_vpred_step_ms*; factors [B] -> the _rs form.  (sa, s1) are formed from `at` in fp32 as step_coeffs forms them."""
    _need_cuda(x, v, x0_prev)
    assert x.is_contiguous() and v.is_contiguous() and v.numel() == 2 * x.numel() and v.dtype == x.dtype
    out = torch.empty_like(x) if out is None else out
    assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
    sa, s1 = step_coeffs(at, at)[:2]
    B = x.shape[0]
    name = "tmix_vpred_step" + ("" if x0_prev is None else "_ms") + ("" if factors is None else "_rs")
    prev = () if x0_prev is None else (_history(x0_prev, x),)
    shape, fac = ((x.numel(),), ()) if factors is None else ((B, x.numel() // B), (_video_factors(factors, B),))
    L.check(getattr(L.load(), name)(_p(x), _p(v), _p(out), *prev, _EPS_DT[x.dtype], *shape, float(g), sa, s1, *(float(c) for c in move), *fac, _stream()), name)
    return out


def _plan_rows(x, u, c, R, clip_stride_u, clip_stride_c):
    """head of the entries on plan rows: x [S,C,F,h,w] fp32 contiguous, u / c the CFG halves' frame rows [(S*F), R, h, w] fp32 with clip s at
    s * clip_stride floats (default: one contiguous clip) -> (S, C, F, h * w, stride_u, stride_c)"""
    assert x.dtype == u.dtype == c.dtype == torch.float32 and x.is_contiguous()
    S, Cc, Fr, h, w = x.shape
    clip = Fr * R * h * w
    su, sc = clip_stride_u or clip, clip_stride_c or clip
    for buf, st in ((u, su), (c, sc)):                          # the kernels reach clip S-1's last frame row
        assert buf.is_contiguous() and buf.numel() >= (S - 1) * st + clip
    return S, Cc, Fr, h * w, su, sc


def _vpred_rows(x, v_u, v_c, params, x0_prev, factors, clip_stride_u, clip_stride_c):
    """the four video step entries on plan rows, in place on x: x0_prev -> tmix_vpred_step_ms*_dev, factors [S] -> the _rs form"""
    _need_cuda(x, v_u, v_c, params, x0_prev)
    S, Cc, Fr, hw, su, sc = _plan_rows(x, v_u, v_c, x.shape[1], clip_stride_u, clip_stride_c)
    assert params.numel() >= (6 if x0_prev is None and factors is None else 8)
    name = "tmix_vpred_step" + ("" if x0_prev is None else "_ms") + ("" if factors is None else "_rs") + "_dev"
    prev = () if x0_prev is None else (_history(x0_prev, x),)
    fac = () if factors is None else (_video_factors(factors, S),)
    L.check(getattr(L.load(), name)(_p(x), _p(v_u), su, _p(v_c), sc, *prev, _p(params), S, Cc, Fr, hw, *fac, _stream()), name)
    return x


def video_step_prologue(x, x_u, t_u, x_c, t_c, params, clip_stride_u=None, clip_stride_c=None):
    """head of the batched video step: x [S,C,F,h,w] fp32 (pipeline layout) -> channels [0, C) of the CFG halves' plan inputs
    x_u / x_c (frame rows [(S*F), R, h, w], R >= C, clip s at s * clip_stride floats: default one contiguous clip), and
    params[0] -> t_u / t_c [S].  Channels [C, R) are not written."""
    _need_cuda(x, x_u, t_u, x_c, t_c, params)
    R = x_u.shape[1]
    S, Cc, Fr, hw, su, sc = _plan_rows(x, x_u, x_c, R, clip_stride_u, clip_stride_c)
    assert x_u.shape[1] == x_c.shape[1] == R and t_u.numel() >= S and t_c.numel() >= S        # the kernel writes S timesteps into each half's input
    L.check(L.load().tmix_video_step_prologue(_p(x), _p(x_u), su, _p(t_u), _p(x_c), sc, _p(t_c), _p(params), S, Cc, Fr, hw, R,
                                              _stream()), "tmix_video_step_prologue")


def vpred_step_dev(x, v_u, v_c, params, clip_stride_u=None, clip_stride_c=None):
    """vpred_step for S videos in place on x [S,C,F,h,w] fp32, the CFG halves' predictions read from the plans' frame rows
    v_u / v_c [(S*F), C, h, w] (clip s at s * clip_stride floats) and the coefficients from params {t, sa, s1, sa', s1', g}."""
    return _vpred_rows(x, v_u, v_c, params, None, None, clip_stride_u, clip_stride_c)


def _fill_params(vals, out):
    if out is None:
        return torch.tensor(vals, dtype=torch.float32)
    for i, v in enumerate(vals):
        out[i] = v
    return out


def video_step_params(t, g, at, at_next, out=None):
    """the 8 floats {t, sa, s1, sa_next, s1_next, g, 0, 0} the batched video step reads (coefficients as vpred_step computes them)."""
    return _fill_params([float(t), *step_coeffs(at, at_next), float(g), 0.0, 0.0], out)


def vpred_step_ms(x, v, g, at, coeffs, x0_prev, out=None):
    """DPM-Solver++(2M) form of vpred_step (tmix_vpred_step_ms): x [B,...], v [2B,...] of one dtype, x0_prev fp32 of x's shape
    (read and rewritten with this step's x0); at from the un-shifted alpha table (sa, s1 formed as vpred_step forms them), coeffs = (cx, c0, c1)
    from solver.video_multistep_coeffs.  out may be x.  Returns the next latents (same dtype)."""
    assert x0_prev is not None
    return _vpred_dense(x, v, g, at, coeffs, x0_prev, None, out)


def vpred_step_ms_dev(x, v_u, v_c, x0_prev, params, clip_stride_u=None, clip_stride_c=None):
    """vpred_step_ms for S videos in place on x [S,C,F,h,w] fp32 (x0_prev: the same shape), the CFG halves' predictions read from the plans'
    frame rows as in vpred_step_dev and the coefficients from params {t, sa, s1, cx, c0, c1, g, 0} (video_step_params_ms)."""
    assert x0_prev is not None
    return _vpred_rows(x, v_u, v_c, params, x0_prev, None, clip_stride_u, clip_stride_c)


def video_step_params_ms(t, g, at, coeffs, out=None):
    """the 8 floats {t, sa, s1, cx, c0, c1, g, 0} the batched solver step reads: sa, s1 as vpred_step computes them, coeffs = (cx, c0, c1)."""
    cx, c0, c1 = coeffs
    return _fill_params([float(t), *step_coeffs(at, at)[:2], *(float(np.float32(c)) for c in (cx, c0, c1)), float(g), 0.0], out)


def vpred_rescale_ws(videos, device):
    """the fp64 workspace tmix_vpred_rescale_factors needs for `videos` videos (contents irrelevant: written before read)"""
    return cfg_rescale_ws(2, videos, device)


def _vpred_rescale(v_u, su, v_c, sc, videos, n, params, g_slot, phi, out, ws):
    from .guidance import validate_phi
    _need_cuda(v_u, v_c, params, out, ws)
    assert v_u.dtype == v_c.dtype and v_u.is_contiguous() and v_c.is_contiguous() and params.dtype == torch.float32 and params.numel() >= 8
    for buf, st in ((v_u, su), (v_c, sc)):
        assert buf.numel() >= (videos - 1) * st + n, (tuple(buf.shape), videos, st, n)
    if out is None:
        out = torch.empty(videos, device=v_u.device, dtype=torch.float32)
    if ws is None:
        ws = vpred_rescale_ws(videos, v_u.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == videos, tuple(out.shape)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= L.load().tmix_cfg_rescale_ws_doubles(2, videos)
    L.check(L.load().tmix_vpred_rescale_factors(_p(v_u), su, _p(v_c), sc, _EPS_DT[v_u.dtype], _p(out), _p(ws), videos, n, _p(params), int(g_slot),
                                                validate_phi(phi, "phi"), _stream()), "tmix_vpred_rescale_factors")
    return out


def vpred_rescale_factors(v, params, g_slot, phi, out=None, ws=None):
    """tmix_vpred_rescale_factors on the host loop's layout: v [2B,...] f32|f16|bf16 (uncond rows first), params a device buffer (>= 8 floats) with g
    in slot g_slot, phi in [0, 1] -> factors [B] fp32 (guidance.vpred_rescale_factors_reference), one per video."""
    assert v.shape[0] % 2 == 0
    B = v.shape[0] // 2
    n = v.numel() // (2 * B)
    return _vpred_rescale(v[:B], n, v[B:], n, B, n, params, g_slot, phi, out, ws)


def vpred_rescale_factors_dev(v_u, v_c, videos, n_per_video, params, g_slot, phi, out=None, ws=None, clip_stride_u=None, clip_stride_c=None):
    """tmix_vpred_rescale_factors on the plans' prediction rows v_u / v_c [(S*F), C, h, w] fp32 (clip s at s * clip_stride floats, as vpred_step_dev
    reads them), g from params[g_slot] (5: video_step_params, 6: video_step_params_ms) -> factors [S] fp32."""
    return _vpred_rescale(v_u, clip_stride_u or n_per_video, v_c, clip_stride_c or n_per_video, int(videos), int(n_per_video), params, g_slot, phi,
                          out, ws)


def vpred_step_rs(x, v, g, at, at_next, factors, out=None):
    """vpred_step with the guided prediction of video b scaled by factors[b] (tmix_vpred_step_rs): x [B,...], v [2B,...]."""
    assert factors is not None
    return _vpred_dense(x, v, g, at, step_coeffs(at, at_next)[2:], None, factors, out)


def vpred_step_ms_rs(x, v, g, at, coeffs, x0_prev, factors, out=None):
    """vpred_step_ms with the guided prediction of video b scaled by factors[b] (tmix_vpred_step_ms_rs)."""
    assert x0_prev is not None and factors is not None
    return _vpred_dense(x, v, g, at, coeffs, x0_prev, factors, out)


def vpred_step_rs_dev(x, v_u, v_c, params, factors, x0_prev=None, clip_stride_u=None, clip_stride_c=None):
    """tmix_vpred_step_rs_dev, or with x0_prev (the history buffer) tmix_vpred_step_ms_rs_dev: the arguments of vpred_step_dev / vpred_step_ms_dev
    plus factors [S] fp32 (vpred_rescale_factors_dev).  In place on x [S,C,F,h,w] fp32; returns x."""
    assert factors is not None
    return _vpred_rows(x, v_u, v_c, params, x0_prev, factors, clip_stride_u, clip_stride_c)


def _video_keys(keys, videos):
    assert keys.is_cuda and keys.dtype == torch.int32 and keys.is_contiguous() and keys.numel() == 2 * videos, (tuple(keys.shape), videos)
    return _p(keys)


def vpred_step_noise(x, v, g, at, move, cz, keys, step, x0_prev=None, factors=None, out=None):
    """tmix_vpred_step_noise: the stochastic form of vpred_step / vpred_step_rs (x0_prev None; move = (sa_next, s1_dir), the third
    and fourth value of solver.ddim_eta_coeffs) and of vpred_step_ms / vpred_step_ms_rs (x0_prev the history buffer; move = (cx, c0, c1) of
    solver.video_multistep_eta_coeffs); cz is the last value of either.  x [B,...], v [2B,...] of one dtype, factors [B] or None, keys int32 [B, 2]
    (noise_keys), step the schedule index.  out may be x.  noise.vpred_step_reference gives the same bits.  Returns the next latents."""
    _need_cuda(x, v, x0_prev, factors, keys)
    assert x.is_contiguous() and v.is_contiguous() and v.numel() == 2 * x.numel() and v.dtype == x.dtype
    out = torch.empty_like(x) if out is None else out
    assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
    sa, s1 = step_coeffs(at, at)[:2]
    B = x.shape[0]
    a, b, c = (float(m) for m in (tuple(move) + (0.0,))[:3])
    prev = None if x0_prev is None else _history(x0_prev, x)
    fac = None if factors is None else _video_factors(factors, B)
    assert 0 <= int(step) < 2 ** 32, step
    L.check(L.load().tmix_vpred_step_noise(_p(x), _p(v), _p(out), prev, _EPS_DT[x.dtype], B, x.numel() // B, float(g), sa, s1, a, b, c, float(cz),
                                           fac, _video_keys(keys, B), int(step), _stream()), "tmix_vpred_step_noise")
    return out


def vpred_step_noise_dev(x, v_u, v_c, params, keys, x0_prev=None, factors=None, clip_stride_u=None, clip_stride_c=None):
    """tmix_vpred_step_noise_dev: the stochastic form of vpred_step_dev / vpred_step_rs_dev (x0_prev None) and of vpred_step_ms_dev / its rescale
    form (x0_prev the history buffer), factors [S] or None, keys int32 [S, 2] (noise_keys); params holds 12 floats (video_step_params_noise).
    In place on x [S,C,F,h,w] fp32; returns x."""
    _need_cuda(x, v_u, v_c, params, x0_prev, factors, keys)
    S, Cc, Fr, hw, su, sc = _plan_rows(x, v_u, v_c, x.shape[1], clip_stride_u, clip_stride_c)
    assert params.dtype == torch.float32 and params.numel() >= 12, params.numel()
    prev = None if x0_prev is None else _history(x0_prev, x)
    fac = None if factors is None else _video_factors(factors, S)
    L.check(L.load().tmix_vpred_step_noise_dev(_p(x), _p(v_u), su, _p(v_c), sc, _p(params), S, Cc, Fr, hw, prev, fac, _video_keys(keys, S), _stream()),
            "tmix_vpred_step_noise_dev")
    return x


def video_step_params_noise(t, g, at, coeffs_or_next, cz, step_index, out=None):
    """the 12 floats tmix_vpred_step_noise_dev reads: the parent's 8, then {cz, step_index, 0, 0}.  coeffs_or_next: (sa_next, s1_dir) -- the DDIM
    layout {t, sa, s1, sa_next, s1_dir, g, 0, 0} -- or (cx, c0, c1) -- the solver's {t, sa, s1, cx, c0, c1, g, 0}; sa, s1 as vpred_step forms them."""
    m = [float(np.float32(c)) for c in coeffs_or_next]
    assert len(m) in (2, 3), m
    assert 0 <= int(step_index) < 2 ** 24, step_index            # exact in fp32
    head = [float(t), *step_coeffs(at, at)[:2], *m, float(g)] + [0.0] * (4 - len(m))
    return _fill_params(head + [float(np.float32(cz)), float(int(step_index)), 0.0, 0.0], out)


def _video_hold(hold_x0, hold_w, S, Cc, Fr, h, w):
    """the six hold arguments of the three hold entries: hold_x0 [S or 1, C, Fk, h, w], hold_w [S or 1, Fw, h, w], fp32 contiguous on the device,
    Fk, Fw in {1, F}; a leading 1 is shared by every video (video stride 0)"""
    for t in (hold_x0, hold_w):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, tuple(t.shape))
    assert hold_x0.dim() == 5 and hold_x0.shape[0] in (1, S) and hold_x0.shape[1] == Cc and hold_x0.shape[2] in (1, Fr), (tuple(hold_x0.shape), (S, Cc, Fr, h, w))
    assert tuple(hold_x0.shape[3:]) == (h, w), (tuple(hold_x0.shape), (S, Cc, Fr, h, w))
    assert hold_w.dim() == 4 and hold_w.shape[0] in (1, S) and hold_w.shape[1] in (1, Fr) and tuple(hold_w.shape[2:]) == (h, w), (tuple(hold_w.shape), (S, Fr, h, w))
    sx = 0 if hold_x0.shape[0] == 1 and S > 1 else hold_x0[0].numel()
    sw = 0 if hold_w.shape[0] == 1 and S > 1 else hold_w[0].numel()
    return _p(hold_x0), sx, int(hold_x0.shape[2]), _p(hold_w), sw, int(hold_w.shape[1])


def vpred_step_hold(x, v, g, at, move, cz, keys, step, at_written, hold_x0, hold_w, x0_prev=None, factors=None, out=None):
    """tmix_vpred_step_hold: vpred_step_noise (cz may be 0: the deterministic step) whose stored value is blended with the held
    latent: x [B,C,F,h,w], hold_x0 fp32 [B or 1, C, 1 or F, h, w], hold_w fp32 [B or 1, 1 or F, h, w] in [0, 1] (1 = held).  at_written: the alpha
    of the state the step writes, None on the last step of a schedule ((ha, hs) = (1, 0): the held part is hold_x0 itself).
    noise.vpred_hold_reference gives the same bits.  out may be x.  Returns the next latents."""
    _need_cuda(x, v, x0_prev, factors, keys, hold_x0, hold_w)
    assert x.dim() == 5 and x.is_contiguous() and v.is_contiguous() and v.numel() == 2 * x.numel() and v.dtype == x.dtype
    out = torch.empty_like(x) if out is None else out
    assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
    sa, s1 = step_coeffs(at, at)[:2]
    ha, hs = hold_coeffs(at_written)
    B, Cc, Fr, h, w = x.shape
    a, b, c = (float(m) for m in (tuple(move) + (0.0,))[:3])
    prev = None if x0_prev is None else _history(x0_prev, x)
    fac = None if factors is None else _video_factors(factors, B)
    assert 0 <= int(step) < 2 ** 32, step
    L.check(L.load().tmix_vpred_step_hold(_p(x), _p(v), _p(out), prev, _EPS_DT[x.dtype], B, Cc, Fr, h * w, float(g), sa, s1, a, b, c, float(cz), fac,
                                          _video_keys(keys, B), int(step), ha, hs, *_video_hold(hold_x0, hold_w, B, Cc, Fr, h, w), _stream()),
            "tmix_vpred_step_hold")
    return out


def vpred_step_hold_dev(x, v_u, v_c, params, keys, hold_x0, hold_w, x0_prev=None, factors=None, clip_stride_u=None, clip_stride_c=None):
    """tmix_vpred_step_hold_dev: vpred_step_noise_dev with the hold; params holds 12 floats (video_step_params_hold).  In place on
    x [S,C,F,h,w] fp32; returns x."""
    _need_cuda(x, v_u, v_c, params, x0_prev, factors, keys, hold_x0, hold_w)
    S, Cc, Fr, hw, su, sc = _plan_rows(x, v_u, v_c, x.shape[1], clip_stride_u, clip_stride_c)
    assert params.dtype == torch.float32 and params.numel() >= 12, params.numel()
    prev = None if x0_prev is None else _history(x0_prev, x)
    fac = None if factors is None else _video_factors(factors, S)
    L.check(L.load().tmix_vpred_step_hold_dev(_p(x), _p(v_u), su, _p(v_c), sc, _p(params), S, Cc, Fr, hw, prev, fac, _video_keys(keys, S),
                                              *_video_hold(hold_x0, hold_w, S, Cc, Fr, x.shape[3], x.shape[4]), _stream()), "tmix_vpred_step_hold_dev")
    return x


def video_hold_composite(x, at_written, keys, hold_x0, hold_w):
    """tmix_video_hold_composite: the hold's blend in place on x [S,C,F,h,w] (any model dtype) with moved = x, at the noise level `at_written` of x
    itself (None: (ha, hs) = (1, 0)): x_T once at the start of a run.  Returns x."""
    _need_cuda(x, keys, hold_x0, hold_w)
    assert x.dim() == 5 and x.is_contiguous()
    S, Cc, Fr, h, w = x.shape
    ha, hs = hold_coeffs(at_written)
    L.check(L.load().tmix_video_hold_composite(_p(x), _EPS_DT[x.dtype], S, Cc, Fr, h * w, ha, hs, _video_keys(keys, S),
                                               *_video_hold(hold_x0, hold_w, S, Cc, Fr, h, w), _stream()), "tmix_video_hold_composite")
    return x


def hold_coeffs(at_written):
    """(ha, hs) of the hold: sqrt(alpha), sqrt(1 - alpha) of the written state as step_coeffs forms (sa, s1); None (the last step): (1, 0)"""
    return (1.0, 0.0) if at_written is None else step_coeffs(at_written, at_written)[:2]


def video_step_params_hold(t, g, at, coeffs_or_next, cz, step_index, at_written, out=None):
    """the 12 floats tmix_vpred_step_hold_dev reads: video_step_params_noise's with slots 10 and 11 = (ha, hs) of the written state (hold_coeffs)"""
    m = [float(np.float32(c)) for c in coeffs_or_next]
    assert len(m) in (2, 3), m
    assert 0 <= int(step_index) < 2 ** 24, step_index            # exact in fp32
    head = [float(t), *step_coeffs(at, at)[:2], *m, float(g)] + [0.0] * (4 - len(m))
    return _fill_params(head + [float(np.float32(cz)), float(int(step_index)), *hold_coeffs(at_written)], out)


def video_step_prologue_cond(x, x_c, t_c, params, clip_stride_c=None):
    """tmix_video_step_prologue_cond, the head of an unguided video step: video_step_prologue for the text half alone -- x
    [S,C,F,h,w] fp32 -> channels [0, C) of x_c's frame rows [(S*F), R, h, w], params[0] -> t_c [S]; nothing else is written."""
    _need_cuda(x, x_c, t_c, params)
    R = x_c.shape[1]
    S, Cc, Fr, hw, _, sc = _plan_rows(x, x_c, x_c, R, clip_stride_c, clip_stride_c)
    assert t_c.numel() >= S
    L.check(L.load().tmix_video_step_prologue_cond(_p(x), _p(x_c), sc, _p(t_c), _p(params), S, Cc, Fr, hw, R, _stream()),
            "tmix_video_step_prologue_cond")


def _cond_hold(hold_x0, hold_w, at_written, S, Cc, Fr, h, w):
    """(ha, hs, the six hold arguments) of the unguided entries; no hold: nulls"""
    if hold_x0 is None and hold_w is None:
        return 0.0, 0.0, None, 0, 1, None, 0, 1
    return (*hold_coeffs(at_written), *_video_hold(hold_x0, hold_w, S, Cc, Fr, h, w))


def vpred_step_cond(x, v_c, at, move, x0_prev=None, cz=0.0, keys=None, step=0, at_written=None, hold_x0=None, hold_w=None, out=None):
    """tmix_vpred_step_cond, the unguided video step on the model dtype: x, v_c [B,C,F,h,w] of one dtype -- v_c is the
    conditional prediction alone, no CFG is applied.  x0_prev None: the DDIM move, move = (sa_next, s1_next or s1_dir); else the fp32 history and
    move = (cx, c0, c1).  keys int32 [B, 2] (noise_keys) with cz and step: the noise of vpred_step_noise; hold_x0 / hold_w with at_written: the hold
    of vpred_step_hold (needs keys).  out may be x.  guidance.vpred_cond_step_reference gives the same bits.  Returns the next latents."""
    _need_cuda(x, v_c, x0_prev, keys, hold_x0, hold_w)
    assert x.dim() == 5 and x.is_contiguous() and v_c.is_contiguous() and v_c.numel() == x.numel() and v_c.dtype == x.dtype
    out = torch.empty_like(x) if out is None else out
    assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
    sa, s1 = step_coeffs(at, at)[:2]
    B, Cc, Fr, h, w = x.shape
    a, b, c = (float(m) for m in (tuple(move) + (0.0,))[:3])
    prev = None if x0_prev is None else _history(x0_prev, x)
    assert 0 <= int(step) < 2 ** 32, step
    ha, hs, *hold = _cond_hold(hold_x0, hold_w, at_written, B, Cc, Fr, h, w)
    L.check(L.load().tmix_vpred_step_cond(_p(x), _p(v_c), _p(out), prev, _EPS_DT[x.dtype], B, Cc, Fr, h * w, sa, s1, a, b, c, float(cz),
                                          None if keys is None else _video_keys(keys, B), int(step), ha, hs, *hold, _stream()), "tmix_vpred_step_cond")
    return out


def vpred_step_cond_dev(x, v_c, params, x0_prev=None, keys=None, hold_x0=None, hold_w=None, clip_stride_c=None):
    """tmix_vpred_step_cond_dev, the unguided video step on plan rows, in place on x [S,C,F,h,w] fp32: v_c the text half's prediction rows
    [(S*F), C, h, w] (clip s at s * clip_stride floats); params the floats of the guided step that would run -- video_step_params[_ms] (8) without
    keys, video_step_params_noise / _hold (12) with -- of which g is not read.  Returns x."""
    _need_cuda(x, v_c, params, x0_prev, keys, hold_x0, hold_w)
    S, Cc, Fr, hw, _, sc = _plan_rows(x, v_c, v_c, x.shape[1], clip_stride_c, clip_stride_c)
    assert params.dtype == torch.float32 and params.numel() >= (8 if keys is None else 12), params.numel()
    prev = None if x0_prev is None else _history(x0_prev, x)
    hold = _cond_hold(hold_x0, hold_w, None, S, Cc, Fr, x.shape[3], x.shape[4])[2:]
    L.check(L.load().tmix_vpred_step_cond_dev(_p(x), _p(v_c), sc, _p(params), S, Cc, Fr, hw, prev, None if keys is None else _video_keys(keys, S),
                                              *hold, _stream()), "tmix_vpred_step_cond_dev")
    return x


def frame_inject(x, clips, frames, interp=None):
    """first-frame feature injection (video_gen/utils_attn.py:433-455), in place on x [(clips*frames), ...] contiguous."""
    _need_cuda(x)
    assert x.is_contiguous() and x.shape[0] == clips * frames
    per = x.numel() // (clips * frames)
    hard = interp is None
    a = 0.0 if hard else float(np.float32(interp))
    b = 0.0 if hard else float(np.float32(1.0 - float(interp)))
    L.check(L.load().tmix_frame_inject(_p(x), _EPS_DT[x.dtype], clips, frames, per, int(hard), a, b, _stream()), "tmix_frame_inject")
    return x


def temporal_attention(qkv, clips, frames, heads, scale=None, out=None):
    """self-attention over the frame axis: qkv [(clips*frames), hw, 3*heads*64] bf16 -> [(clips*frames), hw, heads*64]."""
    _need_cuda(qkv)
    n, hw, ld = qkv.shape
    C3 = 3 * heads * 64
    assert n == clips * frames and qkv.dtype == BF16 and qkv.stride(2) == 1 and qkv.stride(0) == hw * qkv.stride(1) and ld >= C3
    out = torch.empty(n, hw, heads * 64, device=qkv.device, dtype=BF16) if out is None else out
    L.check(L.load().tmix_temporal_attn(_p(qkv), qkv.stride(1), _p(out), out.stride(1), clips, frames, hw, heads,
                                        float(scale if scale is not None else 64 ** -0.5), _stream()), "tmix_temporal_attn")
    return out


def softmax_rows_masked(scores, probs, valid, scale):
    """probs[r, c] = softmax over the first `valid` columns of scale * scores[r] (bf16), zeros in the padding columns."""
    _need_cuda(scores, probs)
    rows, cols = scores.shape
    assert scores.dtype == torch.float32 and probs.dtype == BF16 and probs.shape == scores.shape
    L.check(L.load().tmix_softmax_rows_masked(_p(scores), scores.stride(0), _p(probs), probs.stride(0), rows, cols, int(valid),
                                              float(scale), _stream()), "tmix_softmax_rows_masked")
    return probs


def lora_down(a_pad, K, D, P, nsets, sets, rows_per_set, dcolsum=None, dbias=None, eps=1e-5):
    """fill the 64 pad columns behind the K values of every row of a_pad [rows, K + 64] (bf16, in place) with the rows' LoRA
    down-projections (tmix_lora_down); sets: int32 device tensor, one concept set per block of rows_per_set rows."""
    _need_cuda(a_pad, D, sets)
    assert a_pad.dtype == BF16 and a_pad.dim() == 2 and a_pad.stride(1) == 1 and a_pad.shape[1] >= K + 64 and sets.dtype == torch.int32
    assert D.dtype == BF16 and D.is_contiguous() and D.shape == (nsets * P, K)
    lib = L.load()
    L.check(lib.tmix_lora_down(a_pad.data_ptr(), a_pad.stride(0), K, a_pad.shape[0], D.data_ptr(), P, nsets,
                               None if dcolsum is None else dcolsum.data_ptr(), None if dbias is None else dbias.data_ptr(), eps,
                               sets.data_ptr(), rows_per_set, _stream()), "tmix_lora_down")
    return a_pad

