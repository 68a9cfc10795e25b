"""Guidance rescale (Lin et al. 2023, arXiv:2305.08891, section 3.4; diffusers' `guidance_rescale`): host-side definition and the numpy
restatements of the kernels that carry it.

Every step forms, per conditional eps row r, the guided prediction e_r = eu + g (ec_r - eu).  At g = 9 its standard deviation is a multiple of the
conditional prediction's.  The rescale scales it back,

    f_r = phi sd(ec_r) / sd(e_r) + (1 - phi),        e'_r = f_r e_r,

with the standard deviations taken over the row's n = C h w elements; phi = 0 switches the feature off (the sampler then launches nothing new),
phi = 0.7 is the paper's value.  Where sd(e_r) is zero or a variance is not finite f_r = 1: OUR choice (diffusers divides and produces inf / nan).

Everything here is host code and loads no library: the kernels (csrc/cfg_rescale.hip; the *_rs_dev step entries) are compared with it.
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
