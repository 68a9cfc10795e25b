"""Guidance rescale (Lin et al. 2023, arXiv:2305.08891, section 3.4; diffusers' `guidance_rescale`): host-side definition and the numpy
restatements of the kernels that carry it.

Every step forms, per conditional eps row r, the guided prediction e_r = eu + g (ec_r - eu).  At g = 9 its standard deviation is a multiple of the
conditional prediction's.  The rescale scales it back,

    f_r = phi sd(ec_r) / sd(e_r) + (1 - phi),        e'_r = f_r e_r,

with the standard deviations taken over the row's n = C h w elements; phi = 0 switches the feature off (the sampler then launches nothing new),
phi = 0.7 is the paper's value.  Where sd(e_r) is zero or a variance is not finite f_r = 1: OUR choice (diffusers divides and produces inf / nan).

Everything here is host code and loads no library: the kernels (csrc/cfg_rescale.hip; the *_rs_dev step entries) are compared with it.

The video sampler's form (the second half of this file) takes the statistics per video of the guided v-prediction and puts the
rescaled prediction into x0 AND into the move's eps term.
"""
from __future__ import annotations

import math

import numpy as np

from . import solver as SV

F32 = np.float32
STEP_FUSION, STEP_PLAIN, STEP_RESAMPLE = 0, 1, 2      # TMIX_STEP_* (lib.py's values; this module loads no library)


def validate_phi(phi, what="guidance_rescale"):
    """the ONE check of phi (constructor, CLI, wrappers): a real number in [0, 1] -> float"""
    if isinstance(phi, bool) or not isinstance(phi, (int, float, np.floating, np.integer)):
        raise ValueError(f"{what}={phi!r}: a number in [0, 1] (0: off; 0.7: the value of arXiv:2305.08891)")
    phi = float(phi)
    if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
        raise ValueError(f"{what}={phi!r}: a number in [0, 1] (0: off; 0.7: the value of arXiv:2305.08891)")
    return phi


def rows_read(mode, K):
    """how many conditional rows (1 .. this) the step mode reads: they carry a factor, every other row holds 1.0"""
    if mode == STEP_PLAIN:
        return 1
    if mode not in (STEP_FUSION, STEP_RESAMPLE):
        raise ValueError(f"guidance rescale: mode {mode}")
    return int(K)


def guided_rows(eps, g, lowp=None):
    """e_r = cfg(eu, ec_r, g) for r = 1 .. rows-1, fp32 with the kernel's rounding points (lowp = np.float16 for fp16 eps): [rows-1, ...]"""
    eps = np.asarray(eps, F32)
    return SV._cfg(eps[:1], eps[1:], g, lowp)


def rescale_factors_reference(mode, eps, K, g, phi, lowp=None):
    """factors [rows-1] fp32 of ONE seed's eps [rows, C, h, w] (fp32 copies of values of the eps dtype): what tmix_cfg_rescale_factors writes, up to
    the order of the fp64 sums.  e_r elementwise in fp32 as the kernel forms it; mean and variance two-pass in fp64 (denominator n - 1); the factor
    in fp64 from the fp32 value of phi, rounded once."""
    eps = np.asarray(eps, F32)
    used = rows_read(mode, K)
    if eps.shape[0] < used + 1:
        raise ValueError(f"guidance rescale: mode {mode} needs {used + 1} eps rows, got {eps.shape[0]}")
    ph = float(F32(validate_phi(phi, "phi")))
    e = guided_rows(eps, g, lowp)
    out = np.ones(eps.shape[0] - 1, F32)
    for r in range(used):
        c64, e64 = eps[1 + r].astype(np.float64).reshape(-1), e[r].astype(np.float64).reshape(-1)
        n = c64.size
        with np.errstate(all="ignore"):
            vc = float(((c64 - c64.mean()) ** 2).sum() / (n - 1))
            ve = float(((e64 - e64.mean()) ** 2).sum() / (n - 1))
            if math.isfinite(vc) and math.isfinite(ve) and ve > 0.0:
                out[r] = F32(ph * math.sqrt(vc) / math.sqrt(ve) + (1.0 - ph))
    return out


def rescaled_rows(eps, factors, g, lowp=None):
    """e'_r = rnd(f_r e_r) for r = 1 .. rows-1 (rnd: to fp16 when lowp, else nothing): [rows-1, ...] fp32"""
    e = guided_rows(eps, g, lowp)
    f = np.asarray(factors, F32).reshape((-1,) + (1,) * (e.ndim - 1))
    return SV._h((f * e).astype(F32), lowp)


def _as_guided(e):
    """eps rows that the existing restatements turn back into e exactly: cfg(0, e, 1) = 0 + 1 * (e - 0)"""
    return np.concatenate([np.zeros_like(e[:1]), e])


def _rescaled_x0(mode, x, eps, masks, K, factors, g, sa, s1, lowp):
    ep = rescaled_rows(eps, factors, g, lowp)
    if mode != STEP_RESAMPLE:
        return SV.blended_x0_reference(mode, x, _as_guided(ep), masks, 1.0, sa, s1, lowp)
    t = lambda r: SV.blended_x0_reference(STEP_PLAIN, x, _as_guided(ep[r:r + 1]), None, 1.0, sa, s1, lowp)
    x0 = (F32(K - 1) * t(0)).astype(F32)                  # (K-1) x0_multi - sum_{c<K-1} x0_single_c, as tweedie_step_kernel
    for c in range(K - 1):
        x0 = (x0 - t(1 + c)).astype(F32)
    return x0


def rescaled_step_reference(mode, x, eps, masks, K, factors, g, sa, s1, sa_next, s1_next, is_last, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_rs_dev for one seed -> (out_x, x0): the existing x0 restatement (solver.blended_x0_reference;
    the RESAMPLE combination from its PLAIN form) on e'_r, then the DDIM move with the UNCONDITIONAL eu as the noise term.  Compared by equality."""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    x0 = _rescaled_x0(mode, x, eps, masks, K, factors, g, sa, s1, lowp)
    moved = ((F32(sa_next) * x0).astype(F32) + SV._h(F32(s1_next) * eps[:1], lowp)).astype(F32)
    return (x0 if is_last else moved), x0


def rescaled_multistep_reference(mode, x, eps, masks, x0_prev, factors, g, sa, s1, cx, c0, c1, is_last, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_ms_rs_dev for one seed -> (out_x, x0): solver.multistep_step_reference on e'_r (its move
    has no eps term).  Compared by equality."""
    eps = np.asarray(eps, F32)
    K = 1 if mode == STEP_PLAIN else np.asarray(masks).shape[0]
    ep = rescaled_rows(eps[:K + 1], np.asarray(factors, F32)[:K], g, lowp)
    return SV.multistep_step_reference(mode, x, _as_guided(ep), masks, x0_prev, 1.0, sa, s1, cx, c0, c1, is_last, lowp)


# ------------------------------------------------------------------------------------------------ video sampler (v-prediction)
# diffusers' rescale_noise_cfg on the guided v-prediction, per VIDEO: v' = cfg(v_u, v_c, g), f = phi sd(v_c) / sd(v') + (1 - phi) over the video's
# n = C F h w elements, v'' = rnd(f v').  v'' replaces v' in x0 = sa x - s1 v'' AND in eps = sa v'' + s1 x: the video loop hands the scheduler one
# model output and both come from it (the image path above keeps the unconditional row as the move's noise term).
# lowp as in solver.vpred_multistep_reference: None, np.float16 (every operation rounds) or "bf16" (fp32 arithmetic, one rounding at the store).
def _lp(lowp):
    return None if isinstance(lowp, str) and lowp == "bf16" else lowp


def vpred_guided(v_u, v_c, g, lowp=None):
    """v' = cfg(v_u, v_c, g) elementwise, fp32 with the kernel's rounding points"""
    return SV._cfg(np.asarray(v_u, F32), np.asarray(v_c, F32), g, _lp(lowp))


def vpred_rescale_factors_reference(v_u, v_c, g, phi, lowp=None):
    """factors [B] fp32 of v_u, v_c [B, ...] (fp32 copies of values of the model dtype): what tmix_vpred_rescale_factors writes, up to the order
    of the fp64 sums.  Per video: v' elementwise as the kernel forms it; mean and variance two-pass in fp64 (denominator n - 1); the factor in fp64
    from the fp32 value of phi, rounded once; 1 where sd(v') is zero or a variance is not finite."""
    v_u, v_c = np.asarray(v_u, F32), np.asarray(v_c, F32)
    ph = float(F32(validate_phi(phi, "phi")))
    vv = vpred_guided(v_u, v_c, g, lowp)
    out = np.ones(v_c.shape[0], F32)
    for b in range(v_c.shape[0]):
        c64, e64 = v_c[b].astype(np.float64).reshape(-1), vv[b].astype(np.float64).reshape(-1)
        n = c64.size
        with np.errstate(all="ignore"):
            vc = float(((c64 - c64.mean()) ** 2).sum() / (n - 1))
            ve = float(((e64 - e64.mean()) ** 2).sum() / (n - 1))
            if math.isfinite(vc) and math.isfinite(ve) and ve > 0.0:
                out[b] = F32(ph * math.sqrt(vc) / math.sqrt(ve) + (1.0 - ph))
    return out


def vpred_rescaled(v, factors, g, lowp=None):
    """v'' = rnd(f_b v'_b) of v [2B, ...] (uncond rows first) -> [B, ...] fp32"""
    v = np.asarray(v, F32)
    B = v.shape[0] // 2
    vv = vpred_guided(v[:B], v[B:], g, lowp)
    f = np.asarray(factors, F32).reshape((B,) + (1,) * (vv.ndim - 1))
    return SV._h((f * vv).astype(F32), _lp(lowp))


def vpred_rescaled_step_reference(x, v, factors, g, sa, s1, sa_next, s1_next, lowp=None):
    """numpy restatement of tmix_vpred_step_rs (and, with lowp None, of tmix_vpred_step_rs_dev per video) -> (out, x0): the DDIM move of the video
    loop on v'' -- eps = sa v'' + s1 x, x0 = sa x - s1 v'', out = sa' x0 + s1' eps, every product and sum its own fp32 operation
    (oracle.tweedie_oracle.video_vpred_step's operations; tests/test_video_rescale_cpu.py pins the two at factor 1).  Compared by equality."""
    x = np.asarray(x, F32)
    lp = _lp(lowp)
    h = lambda a: SV._h(a, lp)
    vv = vpred_rescaled(v, factors, g, lowp)
    eps = h(h(F32(sa) * vv) + h(F32(s1) * x))
    x0 = h(h(F32(sa) * x) - h(F32(s1) * vv)).astype(F32)
    out = h(h(F32(sa_next) * x0) + h(F32(s1_next) * eps)).astype(F32)
    if lp is not lowp:
        out = SV._bf16_round(out)
    return out, x0


def vpred_rescaled_multistep_reference(x, v, x0_prev, factors, g, sa, s1, cx, c0, c1, lowp=None):
    """numpy restatement of tmix_vpred_step_ms_rs (and, with lowp None, of tmix_vpred_step_ms_rs_dev per video) -> (out, x0):
    solver.vpred_multistep_reference on [0; v''] with g = 1 (cfg(0, e, 1) gives e back exactly).  Compared by equality."""
    vv = vpred_rescaled(v, factors, g, lowp)
    return SV.vpred_multistep_reference(x, np.concatenate([np.zeros_like(vv), vv]), x0_prev, 1.0, sa, s1, cx, c0, c1, lowp)      # _as_guided for B videos
