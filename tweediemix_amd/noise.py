"""Counter-based noise of the stochastic sampler (eta > 0): the numpy restatement of csrc/noise.h.

One Philox4x32-10 call (Salmon et al., SC'11) per element: key = the trajectory's 64-bit seed value {low word, high word}, counter = {index low
word, index high word, schedule step index, stream id}, index = the element's linear index c*H*W + y*W + x on the seed's canvas grid.  Output
words 0 and 1 become one standard normal by Box-Muller; ln, sin and cos are written out in integer operations and single-rounded fp32 add, sub,
mul, div and sqrt, which numpy's float32 has as well: the step kernel is compared with `normal` by equality.  Host code only.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U32, U64 = np.uint32, np.uint64

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM_IMAGE_STEP = 0           # stream id of the image sampler's step
STREAM_VIDEO_STEP = 1           # of the video sampler's step: the same seed draws unrelated noise there
STREAM_VIDEO_HOLD = 2           # of the one fixed noise of the video sampler's hold regions (always step 0); every other value is reserved

# the constants of csrc/noise.h, value for value
SQRT2 = F32(1.41421354)
LN2_HI, LN2_LO = F32(0.693145751953125), F32(1.42860682e-06)        # ln 2 = hi + lo; hi has 12 significant bits, so e * hi is exact for |e| <= 24
LN_C = [F32(1.0 / 3.0), F32(1.0 / 5.0), F32(1.0 / 7.0), F32(1.0 / 9.0)]     # atanh series: ln m = 2 s (1 + s^2/3 + s^4/5 + s^6/7 + s^8/9)
HALF_PI = F32(1.57079637)
SIN_C = [F32(-1.0 / 6.0), F32(1.0 / 120.0), F32(-1.0 / 5040.0), F32(1.0 / 362880.0)]             # sin p = p (1 + p^2 (...)), degree 9
COS_C = [F32(-1.0 / 2.0), F32(1.0 / 24.0), F32(-1.0 / 720.0), F32(1.0 / 40320.0)]                # cos p = 1 + p^2 (...), degree 8


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two -> the four output words as uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, U64)) & U64(0xFFFFFFFF) for v in counter]
    k = [np.atleast_1d(np.asarray(v, U64)) & U64(0xFFFFFFFF) for v in key]
    mask = U64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k = [(k[0] + U64(PHILOX_W0)) & mask, (k[1] + U64(PHILOX_W1)) & mask]
        p0, p1 = U64(PHILOX_M0) * c[0], U64(PHILOX_M1) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & mask]
    return [np.broadcast_to(v, np.broadcast(*c).shape).astype(U32) for v in c]


def _ln(u):
    """ln u for fp32 u in (0, 1): exponent from the bit pattern, mantissa reduced to [sqrt(1/2), sqrt 2), atanh series in (m-1)/(m+1)"""
    bits = u.view(U32)
    e = (bits >> U32(23)).astype(np.int32) - np.int32(127)
    m = ((bits & U32(0x007FFFFF)) | U32(0x3F800000)).view(F32)
    big = m > SQRT2
    m = np.where(big, m * F32(0.5), m).astype(F32)
    e = (e + big.astype(np.int32)).astype(F32)
    s = ((m - F32(1)) / (m + F32(1))).astype(F32)
    s2 = (s * s).astype(F32)
    p = LN_C[3]
    for c in (LN_C[2], LN_C[1], LN_C[0]):
        p = (p * s2 + c).astype(F32)
    p = (p * s2 + F32(1)).astype(F32)
    lnm = ((s + s) * p).astype(F32)
    return (e * LN2_HI + (e * LN2_LO + lnm).astype(F32)).astype(F32)


def normal_from_words(w0, w1):
    """Box-Muller on two uint32 words, operation for operation what csrc/noise.h's noise_normal_words does -> fp32"""
    w0, w1 = np.atleast_1d(np.asarray(w0, U32)), np.atleast_1d(np.asarray(w1, U32))
    u1 = (((w0 >> U32(9)).astype(F32) + F32(0.5)) * F32(2.0 ** -23)).astype(F32)        # >= 2^-24: |z| < 5.8
    r = np.sqrt((F32(-2) * _ln(u1)).astype(F32)).astype(F32)
    a = w1 >> U32(9)                                                                     # 23 angle bits: quadrant, then 21 bits inside it
    q = a >> U32(21)
    t = (((a & U32(0x1FFFFF)).astype(F32) + F32(0.5)) * F32(2.0 ** -21)).astype(F32)     # (0, 1): the angle inside the quadrant / (pi/2)
    fold = t > F32(0.5)
    t = np.where(fold, F32(1) - t, t).astype(F32)
    p = (t * HALF_PI).astype(F32)                                                        # [0, pi/4]
    p2 = (p * p).astype(F32)
    sn, cs = SIN_C[3], COS_C[3]
    for a_s, a_c in ((SIN_C[2], COS_C[2]), (SIN_C[1], COS_C[1]), (SIN_C[0], COS_C[0])):
        sn = (sn * p2 + a_s).astype(F32)
        cs = (cs * p2 + a_c).astype(F32)
    sn = (p * (sn * p2 + F32(1)).astype(F32)).astype(F32)
    cs = (cs * p2 + F32(1)).astype(F32)
    # cos(q pi/2 + theta): cos theta, -sin theta, -cos theta, sin theta; folded, sin and cos of theta trade places
    c = np.where(((q & U32(1)) != 0) != fold, sn, cs).astype(F32)
    c = np.where((q == 1) | (q == 2), -c, c).astype(F32)
    return (r * c).astype(F32)


def normal(index, key_lo, key_hi, step, stream_id=STREAM_IMAGE_STEP):
    """z of the elements `index` (integers below 2^64, any shape) of the trajectory with key {key_lo, key_hi} at schedule step `step` -> fp32"""
    idx = np.asarray(index).astype(U64)
    w = philox4x32_10((idx & U64(0xFFFFFFFF), idx >> U64(32), step, stream_id), (key_lo, key_hi))
    return normal_from_words(w[0], w[1]).reshape(idx.shape)


def seed_key(seed):
    """{low word, high word} of a trajectory's 64-bit seed value"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def canvas_index(channels, h, w, oy=0, ox=0, canvas_h=None, canvas_w=None):
    """[channels, h, w] uint64: the canvas-grid linear index c*H*W + y*W + x of every element of the window at (oy, ox); no canvas: arange"""
    H, W = (h if canvas_h is None else canvas_h), (w if canvas_w is None else canvas_w)
    c = np.arange(channels, dtype=U64)[:, None, None]
    y = np.arange(h, dtype=U64)[None, :, None] + U64(oy)
    x = np.arange(w, dtype=U64)[None, None, :] + U64(ox)
    return c * U64(H * W) + y * U64(W) + x


def step_reference(mode, x, eps, masks, x0_prev, params, key, factors=None, index=None, lowp=None):
    """numpy restatement of tmix_fused_tweedie_step_noise_dev for one row -> (out_x, x0).  params: the 12 floats the entry reads -- the parent's
    8 ({t, sa, s1, sa_next, s1_next, is_last, g, -} when x0_prev is None, else {t, sa, s1, cx, c0, c1, is_last, g}), then {cz, step index, 0, 0};
    key = (low word, high word); factors [rows-1]: the row's rescale factors, or None; index: the canvas index of every element of x
    (canvas_index), None = the element's own linear index.  The parent's restatement (guidance.rescaled_*_reference; a factor of 1.0 gives the
    unscaled parent bit for bit) forms x0 and the move, then one product and one sum add cz * z.  Compared with the kernel by equality."""
    from . import guidance as G
    x = np.asarray(x, F32)
    p = [float(F32(v)) for v in params]
    K = 1 if mode == 1 else np.asarray(masks).shape[0]            # TMIX_STEP_PLAIN reads one guided row
    f = np.ones(K, F32) if factors is None else np.asarray(factors, F32)[:K]
    if x0_prev is None:
        is_last = p[5] != 0.0
        moved, x0 = G.rescaled_step_reference(mode, x, eps, masks, K, f, p[6], p[1], p[2], p[3], p[4], False, lowp)
    else:
        is_last = p[6] != 0.0
        moved, x0 = G.rescaled_multistep_reference(mode, x, eps, masks, x0_prev, f, p[7], p[1], p[2], p[3], p[4], p[5], False, lowp)
    if is_last:
        return x0, x0
    if p[8] != 0.0:
        idx = np.arange(x.size, dtype=U64).reshape(x.shape) if index is None else np.asarray(index, U64).reshape(x.shape)
        z = normal(idx, key[0], key[1], int(p[9]))
        moved = (moved + (F32(p[8]) * z).astype(F32)).astype(F32)
    return moved, x0


def vpred_step_reference(x, v, x0_prev, params_or_coeffs, keys, step=None, factors=None, lowp=None):
    """numpy restatement of tmix_vpred_step_noise and tmix_vpred_step_noise_dev -> (out, x0).  x [B, ...], v [2B, ...] (uncond rows
    first) fp32 copies of values of the model dtype; x0_prev None: the DDIM move, else the fp32 history [B, ...] and the multistep move.
    params_or_coeffs: the 12 floats the _dev entry reads -- the parent's 8 ({t, sa, s1, sa_next, s1_dir, g, 0, 0} when x0_prev is None, else
    {t, sa, s1, cx, c0, c1, g, 0}), then {cz, step index, 0, 0} -- or the dense entry's seven coefficients (g, sa, s1, a, b, c, cz) with
    (a, b) = (sa_next, s1_dir) or (a, b, c) = (cx, c0, c1).  keys [B] of (low word, high word); step: the schedule index (None: params[9]);
    factors [B] or None; lowp as in guidance.vpred_rescaled_step_reference (None, np.float16, "bf16").  The parent's restatement
    (guidance.vpred_rescaled_step_reference / vpred_rescaled_multistep_reference; a factor of 1.0 gives the unscaled parent bit for bit) forms
    x0 and moved; then one product and one sum add cz * z, z = normal(the element's linear index in its video, the video's key, step,
    STREAM_VIDEO_STEP), with the dtype's rounding points: fp16 rounds the product and the sum, bf16 the stored value alone.  Compared with
    both kernels by equality."""
    from . import guidance as G
    from . import solver as SV
    x = np.asarray(x, F32)
    p = [float(F32(c)) for c in params_or_coeffs]
    if len(p) == 12:
        g, sa, s1, a, b, c = (p[5], p[1], p[2], p[3], p[4], 0.0) if x0_prev is None else (p[6], p[1], p[2], p[3], p[4], p[5])
        cz, step = p[8], int(p[9]) if step is None else int(step)
    elif len(p) == 7:
        g, sa, s1, a, b, c, cz = p
        step = int(step)
    else:
        raise ValueError(f"vpred_step_reference: {len(p)} values (12 device parameters or the 7 coefficients g, sa, s1, a, b, c, cz)")
    B = x.shape[0]
    if len(keys) != B:
        raise ValueError(f"vpred_step_reference: {len(keys)} keys for {B} videos")
    f = np.ones(B, F32) if factors is None else np.asarray(factors, F32).reshape(B)
    bf16 = isinstance(lowp, str) and lowp == "bf16"
    lp = None if bf16 else lowp                      # bf16: fp32 arithmetic, ONE rounding at the store -- behind the noise
    if x0_prev is None:
        moved, x0 = G.vpred_rescaled_step_reference(x, v, f, g, sa, s1, a, b, lp)
    else:
        moved, x0 = G.vpred_rescaled_multistep_reference(x, v, x0_prev, f, g, sa, s1, a, b, c, lp)
    if cz != 0.0:
        idx = np.arange(x[0].size, dtype=U64).reshape(x[0].shape)
        z = np.stack([normal(idx, k[0], k[1], step, STREAM_VIDEO_STEP) for k in keys])
        moved = SV._h((moved + SV._h((F32(cz) * z).astype(F32), lp)).astype(F32), lp).astype(F32)
    if bf16:
        moved = SV._bf16_round(moved)
    return moved, x0


def hold_blend_reference(moved, kx, w, ha, hs, keys, lowp=None):
    """the blend of the video hold (csrc/video_step.hip's hold_blend) on fp32 arrays -> fp32, before the store's rounding.
    moved [B, C, F, ...]; kx [B or 1, C, Fk, ...] with Fk in {1, F}; w [B or 1, Fw, ...] with Fw in {1, F}, broadcast over channels; keys [B] of
    (low word, high word); lowp None or np.float16 (every product and sum rounds).
      kept = hs != 0 ? rnd(rnd(ha kx) + rnd(hs zh)) : kx        zh = normal(the element's linear index in its video, the video's key, 0, STREAM_VIDEO_HOLD)
      out  = w == 0 ? moved : w == 1 ? kept : rnd(rnd(w kept) + rnd(rnd(1 - w) moved))
    The selects are np.where on the operands' own arrays: a NaN in moved stays out of w == 1, kx keeps its sign bit at hs == 0."""
    from . import solver as SV
    moved = np.asarray(moved, F32)
    B = moved.shape[0]
    if len(keys) != B:
        raise ValueError(f"hold_blend_reference: {len(keys)} keys for {B} videos")
    kx, w = np.asarray(kx, F32), np.asarray(w, F32)
    if kx.ndim != moved.ndim or w.ndim != moved.ndim - 1:
        raise ValueError(f"hold_blend_reference: kx {kx.shape} / w {w.shape} for a state {moved.shape}")
    kx = np.ascontiguousarray(np.broadcast_to(kx, moved.shape))
    w = np.ascontiguousarray(np.broadcast_to(w[:, None], moved.shape))
    ha, hs = F32(ha), F32(hs)
    kept = kx
    if hs != 0.0:
        idx = np.arange(moved[0].size, dtype=U64).reshape(moved[0].shape)
        zh = np.stack([normal(idx, k[0], k[1], 0, STREAM_VIDEO_HOLD) for k in keys])
        kept = SV._h((SV._h((ha * kx).astype(F32), lowp) + SV._h((hs * zh).astype(F32), lowp)).astype(F32), lowp).astype(F32)
    with np.errstate(invalid="ignore"):
        mix = SV._h((SV._h((w * kept).astype(F32), lowp) + SV._h((SV._h((F32(1) - w).astype(F32), lowp) * moved).astype(F32), lowp)).astype(F32), lowp)
    return np.where(w == 0, moved, np.where(w == 1, kept, mix)).astype(F32)


def vpred_hold_reference(x, v, x0_prev, params_or_coeffs, keys, kx, w, step=None, factors=None, lowp=None):
    """numpy restatement of tmix_vpred_step_hold and tmix_vpred_step_hold_dev -> (out, x0), built on vpred_step_reference: that
    gives moved (before the store's rounding) and x0, hold_blend_reference the stored value.  params_or_coeffs: the 12 floats the _dev entry
    reads, (ha, hs) in slots 10 and 11, or the dense entry's nine (g, sa, s1, a, b, c, cz, ha, hs).  kx, w as in hold_blend_reference; everything
    else as in vpred_step_reference.  Compared with both kernels by equality."""
    from . import solver as SV
    p = [float(F32(c)) for c in params_or_coeffs]
    if len(p) == 12:
        ha, hs, head = p[10], p[11], p
    elif len(p) == 9:
        ha, hs, head = p[7], p[8], p[:7]
    else:
        raise ValueError(f"vpred_hold_reference: {len(p)} values (12 device parameters or the 9 coefficients g, sa, s1, a, b, c, cz, ha, hs)")
    bf16 = isinstance(lowp, str) and lowp == "bf16"
    lp = None if bf16 else lowp                      # bf16: fp32 arithmetic, ONE rounding at the store -- behind the blend
    moved, x0 = vpred_step_reference(x, v, x0_prev, head, keys, step, factors, lp)
    out = hold_blend_reference(moved, kx, w, ha, hs, keys, lp)
    return (SV._bf16_round(out) if bf16 else SV._h(out, lp).astype(F32)), x0


def video_hold_composite_reference(x, kx, w, ha, hs, keys, lowp=None):
    """numpy restatement of tmix_video_hold_composite: the blend with moved = x, then the store's rounding"""
    from . import solver as SV
    bf16 = isinstance(lowp, str) and lowp == "bf16"
    lp = None if bf16 else lowp
    out = hold_blend_reference(x, kx, w, ha, hs, keys, lp)
    return SV._bf16_round(out) if bf16 else SV._h(out, lp).astype(F32)
