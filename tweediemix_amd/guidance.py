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

The guidance interval (between the two halves) is the other host-side definition about guidance kept here: which timesteps are
guided, and the restatement of the step that runs without the unconditional row (tmix_fused_tweedie_step_cond_dev).  The video sampler's unguided
step (tmix_vpred_step_cond / tmix_vpred_step_cond_dev) is restated in the second half, vpred_cond_step_reference.

Adaptive projected guidance (behind the interval) is the third: the setting's check, the coefficients tmix_apg_coeffs writes and the
step tmix_fused_tweedie_step_apg_dev takes, restated in numpy (apg_coeffs_reference, apg_step_reference, apg_multistep_reference).
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


# ------------------------------------------------------------------------------------------------ guidance interval
# Kynkaanniemi et al. 2024 (arXiv:2404.07724): guidance is applied on a middle range of noise levels only.  Here the range is a pair of TIMESTEP
# values (t_hi, t_lo); a timestep is guided iff t_lo <= t <= t_hi.  An unguided trajectory step runs the UNet without the unconditional row and
# tmix_fused_tweedie_step_cond_dev on what it returns.
def validate_interval(interval, what="guidance_interval"):
    """the ONE check of the interval (constructor, CLI): None, a 'T_HI,T_LO' string or a pair of integers with 1000 >= t_hi >= t_lo >= 0
    -> None or (t_hi, t_lo) as ints"""
    if interval is None:
        return None
    bad = ValueError(f"{what}={interval!r}: two integer timesteps T_HI,T_LO with 1000 >= T_HI >= T_LO >= 0 (a timestep t is guided iff T_LO <= t <= T_HI)")
    if isinstance(interval, str):
        parts = interval.split(",")
        try:
            interval = [int(p.strip()) for p in parts]       # int() refuses '7.5', '', 'a'
        except ValueError:
            raise bad from None
    try:
        vals = list(interval)
    except TypeError:
        raise bad from None
    if len(vals) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise bad
    hi, lo = int(vals[0]), int(vals[1])
    if not 1000 >= hi >= lo >= 0:
        raise bad
    return hi, lo


def is_guided(interval, t):
    """is timestep t inside the interval (None: every timestep is)?"""
    return interval is None or interval[1] <= int(t) <= interval[0]


def unguided_count(interval, timesteps):
    """how many of the schedule's timesteps lie outside the interval (None: 0)"""
    return sum(0 if is_guided(interval, t) else 1 for t in timesteps)


def cond_x0_reference(mode, x, eps, masks, sa, s1, lowp=None):
    """the x0 of an unguided step, solver.blended_x0_reference's operations with e_c = the row itself: eps [rows, C, h, w] holds NO unconditional
    row (FUSION: row c is concept c's, masks [K, 1, h, w]; PLAIN: row 0)"""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    if mode == STEP_PLAIN:
        return SV._tweedie(x, eps[0:1], sa, s1, lowp)
    if mode != STEP_FUSION:
        raise ValueError(f"unguided step: mode {mode} (FUSION or PLAIN)")
    masks = np.asarray(masks, F32)
    x0 = np.zeros_like(x, dtype=F32)
    for c in range(masks.shape[0]):
        x0 = (x0 + masks[c][None] * SV._tweedie(x, eps[c:c + 1], sa, s1, lowp)).astype(F32)
    return x0


def cond_step_reference(mode, x, eps, masks, x0_prev, params, key=None, index=None, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_cond_dev for one row -> (out_x, x0); x0 is also the new history when x0_prev is given.
    x [1, C, h, w]; eps [rows, C, h, w] fp32 copies of values of the eps dtype, no unconditional row; params: the floats the entry reads --
    {t, sa, s1, sa_next, s1_next, is_last, -, -} when x0_prev is None, else {t, sa, s1, cx, c0, c1, is_last, -}, and with key = (low word, high
    word) four more, {cz, step index, 0, 0}; index: the canvas index of every element (noise.canvas_index), None = its own linear index.
    lowp = np.float16 for fp16 eps.  Every product, sum and quotient is a separate fp32 operation.  Compared with the kernel by equality."""
    x = np.asarray(x, F32)
    p = [F32(v) for v in params]
    sa, s1 = p[1], p[2]
    x0 = cond_x0_reference(mode, x, eps, masks, sa, s1, lowp)
    if x0_prev is None:
        is_last = p[5] != 0
        if s1 != 0:
            e0 = ((x - (sa * x0).astype(F32)).astype(F32) / s1).astype(F32)
        else:
            e0 = np.zeros_like(x0)
        moved = ((p[3] * x0).astype(F32) + SV._h((p[4] * e0).astype(F32), lowp)).astype(F32)
    else:
        is_last = p[6] != 0
        m = (p[4] * x0).astype(F32)
        if p[5] != 0:
            m = (m + (p[5] * np.asarray(x0_prev, F32)).astype(F32)).astype(F32)
        moved = ((p[3] * x).astype(F32) + m).astype(F32)
    if is_last:
        return x0, x0
    if key is not None and p[8] != 0:
        from . import noise as NZ
        idx = np.arange(x.size, dtype=np.uint64).reshape(x.shape) if index is None else np.asarray(index, np.uint64).reshape(x.shape)
        z = NZ.normal(idx, key[0], key[1], int(p[9]))
        moved = (moved + (p[8] * z).astype(F32)).astype(F32)
    return moved, x0


# ------------------------------------------------------------------------------------------------ adaptive projected guidance
# Sadat, Hilliges and Weber 2024 (arXiv:2410.02416): guidance on the denoised prediction.  Per conditional row r, with tc / tu the row's conditional
# and the unconditional Tweedie estimate and d = tc - tu, the update d is split into its part parallel to tc and the rest; the parallel part (the one
# that inflates contrast and saturation) is scaled by eta, the whole update's norm is clipped at R (0: no clip):
#     s = R > 0 and Sdd > R^2 ? R / sqrt(Sdd) : 1,   p = Scc > 0 ? s Sdc / Scc : 0,   A = 1 - (g-1)(1-eta) p,   B = (g-1) s,   t_r = A tc + B d
# which is D_c + (g-1)(D_orth + eta D_par) of the clipped update s d.  t_r takes the place of the row's estimate in the blend; the move behind it is
# the parent's (the DDIM move's noise term stays the unconditional row).  OUR choices: {A, B} = {1, g-1} -- CFG in data space -- where a sum is not
# finite, and for rows the mode does not read.  Momentum (the paper's beta) is not implemented.
def validate_apg(apg, what="apg"):
    """the ONE check of the APG setting (constructor, CLI, wrappers): None / False (off), True (the defaults) or a dict with eta in [0, 1]
    (default 0.0: the parallel part is dropped; 1.0: CFG) and norm_threshold >= 0 (default 0.0: no clip), both finite -> None or
    dict(eta=float, norm_threshold=float)"""
    if apg is None or apg is False:
        return None
    if apg is True:
        apg = {}
    bad = ValueError(f"{what}={apg!r}: None or dict(eta=<0..1, the weight of the update's part parallel to the conditional estimate>, "
                     f"norm_threshold=<finite, >= 0: the clip of the update's norm, 0 = none>)")
    if not isinstance(apg, dict) or set(apg) - {"eta", "norm_threshold"}:
        raise bad
    out = {}
    for k in ("eta", "norm_threshold"):
        v = apg.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(float(v)) or float(v) < 0.0:
            raise bad
        out[k] = float(v)
    with np.errstate(over="ignore"):
        if out["eta"] > 1.0 or not math.isfinite(float(F32(out["norm_threshold"]))):     # the kernel takes both as fp32
            raise bad
    return out


def _apg_terms(x, eps, sa, s1, lowp):
    """(tc [rows-1, ...], d [rows-1, ...]) in fp32 with the kernel's rounding points: tc = (x - rnd(s1 ec)) / sa, tu likewise, d = tc - tu"""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    x = x.reshape((1,) + eps.shape[1:])
    with np.errstate(all="ignore"):
        tu = SV._tweedie(x, eps[:1], sa, s1, lowp)
        tc = SV._tweedie(x, eps[1:], sa, s1, lowp)
        return tc, (tc - tu).astype(F32)


def apg_sums_reference(x, eps, sa, s1, lowp=None):
    """[rows-1, 3] fp64 = (Sdd, Sdc, Scc) per conditional row of ONE seed: the fp32 terms of the kernel, products and sums in fp64"""
    tc, d = _apg_terms(x, eps, sa, s1, lowp)
    c64, d64 = tc.astype(np.float64).reshape(tc.shape[0], -1), d.astype(np.float64).reshape(d.shape[0], -1)
    with np.errstate(all="ignore"):
        return np.stack([(d64 * d64).sum(1), (d64 * c64).sum(1), (c64 * c64).sum(1)], axis=1)


def apg_finalise(sums, g, eta, norm_threshold):
    """(A, B, s) as python floats (fp64) from one row's (Sdd, Sdc, Scc): the kernel's operations in the kernel's order, from the fp32 values of g,
    eta and norm_threshold; (1, g-1, 1) where a sum is not finite"""
    dd, dc, cc = (float(v) for v in sums)
    gm1 = float(F32(g)) - 1.0
    if not (math.isfinite(dd) and math.isfinite(dc) and math.isfinite(cc)):
        return 1.0, gm1, 1.0
    R = float(F32(norm_threshold))
    s = R / math.sqrt(dd) if (R > 0.0 and dd > R * R) else 1.0
    p = s * dc / cc if cc > 0.0 else 0.0
    return 1.0 - gm1 * (1.0 - float(F32(eta))) * p, gm1 * s, s


def apg_coeffs_reference(mode, x, eps, K, g, sa, s1, eta, norm_threshold, lowp=None):
    """coeffs [rows-1, 2] fp32 = {A, B} of ONE seed's x [1, C, h, w] and eps [rows, C, h, w] (fp32 copies of values of the eps dtype): what
    tmix_apg_coeffs writes, up to the order of the fp64 sums.  d and tc in fp32 as the kernel forms them, sums in fp64, the coefficients in fp64
    and rounded once; {1, g-1} where a sum is not finite and for the rows the mode does not read."""
    eps = np.asarray(eps, F32)
    used = rows_read(mode, K)
    if eps.shape[0] < used + 1:
        raise ValueError(f"apg: mode {mode} needs {used + 1} eps rows, got {eps.shape[0]}")
    a = validate_apg(dict(eta=eta, norm_threshold=norm_threshold), "apg")
    sums = apg_sums_reference(x, eps, F32(sa), F32(s1), lowp)
    out = np.empty((eps.shape[0] - 1, 2), F32)
    out[:, 0], out[:, 1] = 1.0, F32(float(F32(g)) - 1.0)
    for r in range(used):
        A, B, _s = apg_finalise(sums[r], g, a["eta"], a["norm_threshold"])
        out[r] = F32(A), F32(B)
    return out


def apg_x0_reference(mode, x, eps, masks, K, coeffs, sa, s1, lowp=None):
    """the blended estimate of the APG step, the kernel's operations in the kernel's order: t_r = A_r tc + B_r d (two products, one sum), then the
    mask blend (FUSION), row 1 (PLAIN) or (K-1) t_1 - sum_{c<K-1} t_{2+c} (RESAMPLE).  x [1, C, h, w]; coeffs [rows-1, 2]"""
    tc, d = _apg_terms(x, eps, F32(sa), F32(s1), lowp)
    ab = np.asarray(coeffs, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        t = lambda r: ((ab[r, 0] * tc[r:r + 1]).astype(F32) + (ab[r, 1] * d[r:r + 1]).astype(F32)).astype(F32)
        if mode == STEP_PLAIN:
            return t(0)
        if mode == STEP_FUSION:
            masks = np.asarray(masks, F32)
            x0 = np.zeros_like(t(0))
            for c in range(masks.shape[0]):
                x0 = (x0 + (masks[c][None] * t(c)).astype(F32)).astype(F32)
            return x0
        if mode != STEP_RESAMPLE:
            raise ValueError(f"apg: mode {mode}")
        x0 = (F32(K - 1) * t(0)).astype(F32)
        for c in range(K - 1):
            x0 = (x0 - t(1 + c)).astype(F32)
        return x0


def _apg_noise(moved, p, key, index):
    if key is None or p[8] == 0:
        return moved
    from . import noise as NZ
    idx = np.arange(moved.size, dtype=np.uint64).reshape(moved.shape) if index is None else np.asarray(index, np.uint64).reshape(moved.shape)
    return (moved + (p[8] * NZ.normal(idx, key[0], key[1], int(p[9]))).astype(F32)).astype(F32)


def apg_step_reference(mode, x, eps, masks, K, coeffs, params, key=None, index=None, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_apg_dev WITHOUT a history buffer, for one row -> (out_x, x0).  params: the floats the
    entry reads, {t, sa, s1, sa_next, s1_next, is_last, g, -} and with key = (low word, high word) four more, {cz, step index, 0, 0}; index: the
    canvas index of every element, None = its own linear index.  The DDIM move's noise term is the unconditional row.  Compared by equality."""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    p = [F32(v) for v in params]
    x0 = apg_x0_reference(mode, x, eps, masks, K, coeffs, p[1], p[2], lowp)
    if p[5] != 0:
        return x0, x0
    with np.errstate(all="ignore"):
        moved = ((p[3] * x0).astype(F32) + SV._h((p[4] * eps[:1]).astype(F32), lowp)).astype(F32)
    return _apg_noise(moved, p, key, index), x0


def apg_multistep_reference(mode, x, eps, masks, x0_prev, coeffs, params, key=None, index=None, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_apg_dev WITH the history buffer x0_prev, for one row -> (out_x, x0); x0 is also the new
    history.  params {t, sa, s1, cx, c0, c1, is_last, g} (+ {cz, step index, 0, 0} with key).  x0_prev is used only when c1 != 0."""
    x = np.asarray(x, F32)
    p = [F32(v) for v in params]
    K = 1 if mode == STEP_PLAIN else np.asarray(masks).shape[0]
    x0 = apg_x0_reference(mode, x, eps, masks, K, coeffs, p[1], p[2], lowp)
    if p[6] != 0:
        return x0, x0
    with np.errstate(all="ignore"):
        m = (p[4] * x0).astype(F32)
        if p[5] != 0:
            m = (m + (p[5] * np.asarray(x0_prev, F32)).astype(F32)).astype(F32)
        moved = ((p[3] * x).astype(F32) + m).astype(F32)
    return _apg_noise(moved, p, key, index), x0


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


def vpred_cond_step_reference(x, v_c, x0_prev, sa, s1, move, cz=0.0, keys=None, step=0, hold=None, lowp=None):
    """numpy restatement of tmix_vpred_step_cond and (lowp None) tmix_vpred_step_cond_dev, the UNGUIDED video step -> (out, x0),
    written from the definition: v'' = v_c, the conditional prediction itself -- no CFG, no g, no factor.
      x0    = rnd(rnd(sa x) - rnd(s1 v_c))
      DDIM  (x0_prev None, move = (sa_n, s1_n)):  eps = rnd(rnd(sa v_c) + rnd(s1 x)),  moved = rnd(rnd(sa_n x0) + rnd(s1_n eps))
      2M    (x0_prev the fp32 history, move = (cx, c0, c1)):  m = rnd(c0 x0), c1 != 0: m = rnd(m + rnd(c1 x0_prev)),  moved = rnd(rnd(cx x) + m)
      keys [B] of (low word, high word) and cz != 0:  moved = rnd(moved + rnd(cz z)), z of noise.vpred_step_reference (schedule index `step`)
      hold = (kx, w, ha, hs) (needs keys):  moved = noise.hold_blend_reference(moved, ...)
    x, v_c [B, ...] hold fp32 copies of values of the model dtype.  lowp: None; np.float16 (rnd rounds to fp16 everywhere, x0 included);
    "bf16" (fp32 arithmetic, ONE rounding of out at the store).  Compared with both kernels by equality."""
    from . import noise as NZ
    x, vc = np.asarray(x, F32), np.asarray(v_c, F32)
    if vc.shape != x.shape:
        raise ValueError(f"vpred_cond_step_reference: v_c {vc.shape} for a state {x.shape} (the conditional prediction alone)")
    bf16 = isinstance(lowp, str) and lowp == "bf16"
    lp = _lp(lowp)
    h = lambda a: SV._h(np.asarray(a, F32), lp)
    sa, s1 = F32(sa), F32(s1)
    m_ = [F32(c) for c in move]
    x0 = h(h(sa * x) - h(s1 * vc)).astype(F32)
    if x0_prev is None:
        eps = h(h(sa * vc) + h(s1 * x))
        moved = h(h(m_[0] * x0) + h(m_[1] * eps))
    else:
        m = h(m_[1] * x0)
        if m_[2] != 0:
            m = h(m + h(m_[2] * np.asarray(x0_prev, F32)))
        moved = h(h(m_[0] * x) + m)
    moved = moved.astype(F32)
    if hold is not None and keys is None:
        raise ValueError("vpred_cond_step_reference: a hold without keys")
    if keys is not None and len(keys) != x.shape[0]:
        raise ValueError(f"vpred_cond_step_reference: {len(keys)} keys for {x.shape[0]} videos")
    if keys is not None and F32(cz) != 0:
        idx = np.arange(x[0].size, dtype=np.uint64).reshape(x[0].shape)
        z = np.stack([NZ.normal(idx, k[0], k[1], int(step), NZ.STREAM_VIDEO_STEP) for k in keys])
        moved = h(moved + h(F32(cz) * z)).astype(F32)
    if hold is not None:
        kx, w, ha, hs = hold
        moved = NZ.hold_blend_reference(moved, kx, w, ha, hs, keys, lp)
    return (SV._bf16_round(moved) if bf16 else h(moved).astype(F32)), x0


def vpred_cond_step_from_params(x, v_c, x0_prev, params, keys=None, hold=None):
    """vpred_cond_step_reference on the floats tmix_vpred_step_cond_dev reads: the guided step's 8 ({t, sa, s1, sa_n, s1_n, g, 0, 0} when x0_prev is
    None, else {t, sa, s1, cx, c0, c1, g, 0}) without keys, 12 (then {cz, schedule index, ha, hs}) with; hold = (kx, w).  The g slot is not read."""
    p = [F32(v) for v in params]
    if len(p) < (8 if keys is None else 12):
        raise ValueError(f"vpred_cond_step_from_params: {len(p)} floats")
    move = (p[3], p[4]) if x0_prev is None else (p[3], p[4], p[5])
    cz, step = (p[8], int(p[9])) if keys is not None else (0.0, 0)
    return vpred_cond_step_reference(x, v_c, x0_prev, p[1], p[2], move, cz, keys, step, None if hold is None else (hold[0], hold[1], p[10], p[11]))


def vpred_rescaled_multistep_reference(x, v, x0_prev, factors, g, sa, s1, cx, c0, c1, lowp=None):
    """numpy restatement of tmix_vpred_step_ms_rs (and, with lowp None, of tmix_vpred_step_ms_rs_dev per video) -> (out, x0):
    solver.vpred_multistep_reference on [0; v''] with g = 1 (cfg(0, e, 1) gives e back exactly).  Compared by equality."""
    vv = vpred_rescaled(v, factors, g, lowp)
    return SV.vpred_multistep_reference(x, np.concatenate([np.zeros_like(vv), vv]), x0_prev, 1.0, sa, s1, cx, c0, c1, lowp)      # _as_guided for B videos
