"""DPM-Solver++(2M) on the blended Tweedie estimate: host-side coefficients and the numpy restatement of the step kernel.

The sampler's x0 (in fusion mode the mask blend of the concepts' Tweedie estimates) is the "data prediction" of DPM-Solver++ (Lu et al. 2022,
arXiv:2211.01095, algorithm 2).  With lambda = log(sqrt(a) / sqrt(1 - a)), h = lambda_next - lambda and r = (lambda - lambda_prev) / h the
multistep update is

    x_next = (s1_next / s1) x + sa_next (1 - e^-h) [ (1 + 1/(2r)) x0 - 1/(2r) x0_prev ]  =  cx x + c0 x0 + c1 x0_prev,

first order (c1 = 0) where no usable previous estimate exists.  Everything here is host code: the kernel (csrc/solver_step.hip) sees cx, c0, c1.

The video sampler's v-prediction step takes the same move on x0 = sa x - s1 v': video_multistep_coeffs, vpred_multistep_reference.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
SOLVERS = ("ddim", "dpmpp2m")
STEP_FUSION, STEP_PLAIN = 0, 1        # TMIX_STEP_FUSION / TMIX_STEP_PLAIN (lib.py's values; this module loads no library)


def _sa_s1_lam(a):
    a = float(F32(a))
    sa, s1 = math.sqrt(a), math.sqrt(1.0 - a)
    return sa, s1, math.log(sa / s1)


def multistep_coeffs64(a_prev, a, a_next, second_order):
    """(cx, c0, c1) of the step from alpha a to a_next in fp64 from the fp32 alphas; a_prev (the alpha of the step before, lambda_prev <
    lambda) is read only when second_order"""
    sa, s1, lam = _sa_s1_lam(a)
    san, s1n, lam_n = _sa_s1_lam(a_next)
    h = lam_n - lam
    if not h > 0.0:
        raise ValueError(f"multistep_coeffs: alpha {a} -> {a_next} does not move towards the data (h = {h})")
    E = -math.expm1(-h)
    cx = s1n / s1
    if second_order:
        lam_p = _sa_s1_lam(a_prev)[2]
        r = (lam - lam_p) / h
        if not r > 0.0:
            raise ValueError(f"multistep_coeffs: previous alpha {a_prev} is not noisier than {a}")
        c0, c1 = san * E * (1.0 + 1.0 / (2.0 * r)), -san * E / (2.0 * r)
    else:
        c0, c1 = san * E, 0.0
    return cx, c0, c1


def multistep_coeffs(a_prev, a, a_next, second_order):
    """multistep_coeffs64 rounded ONCE to fp32: what the sampler uploads (Python floats that hold fp32 values)"""
    return tuple(float(F32(v)) for v in multistep_coeffs64(a_prev, a, a_next, second_order))


# ------------------------------------------------------------------------------------------------ stochastic steps (eta)
def validate_eta(eta, name="eta"):
    """eta as a float in [0, 1], or ValueError"""
    try:
        e = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"{name}={eta!r}: a number in [0, 1]") from None
    if not 0.0 <= e <= 1.0:          # NaN fails both comparisons
        raise ValueError(f"{name}={eta!r}: a number in [0, 1] (0: the deterministic sampler, 1: DDPM-like / SDE-DPM-Solver++)")
    return e


def ddim_eta_coeffs64(a, a_next, eta):
    """(sa, s1, sa_next, s1_dir, cz) of the DDIM step with the paper's eta (Song et al. 2020, eq. 12 and 16) in fp64 from the fp32 alphas:
    sigma = eta sqrt((1 - a') / (1 - a)) sqrt(1 - a / a'), s1_dir = sqrt(1 - a' - sigma^2) takes the s1_next slot, cz = sigma"""
    a, an = float(F32(a)), float(F32(a_next))
    if not 0.0 < a <= an <= 1.0:
        raise ValueError(f"ddim_eta_coeffs: alpha {a} -> {an} does not move towards the data")
    sigma = eta * math.sqrt((1.0 - an) / (1.0 - a)) * math.sqrt(1.0 - a / an)
    return math.sqrt(a), math.sqrt(1.0 - a), math.sqrt(an), math.sqrt(max(1.0 - an - sigma * sigma, 0.0)), sigma


def ddim_eta_coeffs(a, a_next, eta):
    """(sa, s1, sa_next, s1_next slot, cz) the sampler uploads for a solver='ddim' step.  sa, s1, sa_next are ops.step_coeffs' fp32 square roots
    (the x0 of a stochastic step is formed with today's coefficients); the s1_next slot and cz are ddim_eta_coeffs64's, rounded ONCE to fp32.
    eta == 0 is today's step: ops.step_coeffs' four values bit for bit (alphas that do not move towards the data included) and cz == 0.0"""
    at, an, one = F32(a), F32(a_next), F32(1)
    sa, s1, san, s1n = float(np.sqrt(at)), float(np.sqrt(one - at)), float(np.sqrt(an)), float(np.sqrt(one - an))
    if eta == 0.0:
        return sa, s1, san, s1n, 0.0
    _, _, _, s1d, cz = ddim_eta_coeffs64(a, a_next, eta)
    return sa, s1, san, float(F32(s1d)), float(F32(cz))


def multistep_eta_coeffs64(a_prev, a, a_next, second_order, eta):
    """(cx, c0, c1, cz) of SDE-DPM-Solver++(2M) in k-diffusion's eta form (sample_dpmpp_2m_sde, midpoint), in fp64: with he = eta h
    cx = (s1'/s1) e^-he,  B = sa' (1 - e^(-h - he)),  c0 = B (1 + 1/(2r)),  c1 = -B / (2r)  (first order: c0 = B, c1 = 0),
    cz = s1' sqrt(1 - e^(-2 he)).  eta == 0 is multistep_coeffs64.  This eta and DDIM's coincide at 0 and 1 and differ in between."""
    cx, c0, c1 = multistep_coeffs64(a_prev, a, a_next, second_order)
    if eta == 0.0:
        return cx, c0, c1, 0.0
    sa, s1, lam = _sa_s1_lam(a)
    san, s1n, lam_n = _sa_s1_lam(a_next)
    h = lam_n - lam
    he = eta * h
    B = -san * math.expm1(-h - he)
    if second_order:
        r = (lam - _sa_s1_lam(a_prev)[2]) / h
        c0, c1 = B * (1.0 + 1.0 / (2.0 * r)), -B / (2.0 * r)
    else:
        c0, c1 = B, 0.0
    return (s1n / s1) * math.exp(-he), c0, c1, s1n * math.sqrt(-math.expm1(-2.0 * he))


def multistep_eta_coeffs(a_prev, a, a_next, second_order, eta):
    """multistep_eta_coeffs64 rounded ONCE to fp32; at eta == 0 multistep_coeffs' values and cz == 0.0"""
    return tuple(float(F32(v)) for v in multistep_eta_coeffs64(a_prev, a, a_next, second_order, eta))


def _h(a, lowp):
    return a.astype(lowp).astype(F32) if lowp is not None else a


def _cfg(eu, ec, g, lowp):
    d = _h(ec - eu, lowp)
    return _h(eu + _h(F32(g) * d, lowp), lowp)


def _tweedie(x, e, sa, s1, lowp):
    return ((x - _h(F32(s1) * e, lowp)) / F32(sa)).astype(F32)


def blended_x0_reference(mode, x, eps, masks, g, sa, s1, lowp=None):
    """the x0 of tweedie_step_kernel (FUSION / PLAIN), operation for operation: x [1,C,h,w], eps [rows,C,h,w] fp32 values of the eps dtype,
    masks [K,1,h,w]; sa, s1 fp32; lowp = np.float16 for fp16 eps (its rounding points), else None"""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    eu = eps[:1]
    if mode == STEP_PLAIN:
        return _tweedie(x, _cfg(eu, eps[1:2], g, lowp), sa, s1, lowp)
    if mode != STEP_FUSION:
        raise ValueError(f"multistep step: mode {mode} (FUSION or PLAIN)")
    masks = np.asarray(masks, F32)
    x0 = np.zeros_like(x, dtype=F32)
    for c in range(masks.shape[0]):
        x0 = (x0 + masks[c][None] * _tweedie(x, _cfg(eu, eps[1 + c:2 + c], g, lowp), sa, s1, lowp)).astype(F32)
    return x0


def multistep_step_reference(mode, x, eps, masks, x0_prev, g, sa, s1, cx, c0, c1, is_last, lowp=None):
    """numpy fp32 restatement of tmix_fused_tweedie_step_ms_dev for one seed -> (out_x, x0); x0 is also the new history.  The kernel is
    compared with this by equality.  Products and sums are separate fp32 operations (the kernel is built with -ffp-contract=off);
    x0_prev is used only when c1 != 0."""
    x = np.asarray(x, F32)
    x0 = blended_x0_reference(mode, x, eps, masks, g, sa, s1, lowp)
    m = (F32(c0) * x0).astype(F32)
    if F32(c1) != 0:
        m = (m + (F32(c1) * np.asarray(x0_prev, F32)).astype(F32)).astype(F32)
    out = x0 if is_last else ((F32(cx) * x).astype(F32) + m).astype(F32)
    return out, x0


# ------------------------------------------------------------------------------------------------ video sampler (v-prediction)
def video_multistep_coeffs(t, a_prev, a, a_next, second_order):
    """(cx, c0, c1) of the video step at timestep t from alpha a to a_next, rounded once to fp32 (multistep_coeffs), on the video table's edge
    cases: a_next == 1 (a checkpoint with set_alpha_to_one behind the last entry; lambda = +inf) is (0, 1, 0), the DDIM result x0, first order by
    definition; a == 0 (the zero-terminal-SNR table's t = 999, or a timestep outside the table) has no lambda and is a ValueError"""
    if not float(F32(a)) > 0.0:
        raise ValueError(f"video solver step: alpha({int(t)}) = {float(a)} has no log-SNR (zero terminal SNR or a timestep outside the table); "
                         f"the grid must start below it")
    if float(F32(a_next)) >= 1.0:
        return 0.0, 1.0, 0.0
    return multistep_coeffs(a_prev, a, a_next, second_order)


def video_multistep_eta_coeffs(t, a_prev, a, a_next, second_order, eta):
    """(cx, c0, c1, cz) of the stochastic video step: multistep_eta_coeffs on video_multistep_coeffs' edge cases -- a_next == 1 is
    (0, 1, 0) with cz = 0 (the step lands on the data; there is no noise level left to add at), a == 0 is refused.  eta == 0: video_multistep_coeffs'
    three values bit for bit and cz == 0.0"""
    cx, c0, c1 = video_multistep_coeffs(t, a_prev, a, a_next, second_order)
    if eta == 0.0 or float(F32(a_next)) >= 1.0:
        return cx, c0, c1, 0.0
    return multistep_eta_coeffs(a_prev, a, a_next, second_order, eta)


def _bf16_round(a):
    """fp32 -> the nearest bf16 value (ties to even), as fp32: the one rounding of a TMIX_BF16 store"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(F32).copy()
    nan = np.isnan(a)
    out[nan] = a[nan]
    return out


def vpred_multistep_reference(x, v, x0_prev, g, sa, s1, cx, c0, c1, lowp=None):
    """numpy restatement of tmix_vpred_step_ms (and, with lowp None, of tmix_vpred_step_ms_dev per video) -> (out, x0); x0 is also the new
    history.  x [B,...], v [2B,...] (uncond rows first) hold fp32 copies of values of the model dtype, x0_prev [B,...] is fp32.  The kernels
    are compared with this by equality: every product and sum is a separate fp32 operation (-ffp-contract=off).  lowp = np.float16: every
    operation's result is rounded to fp16, as the DDIM kernel does for TMIX_F16 (x0 included, so the history holds fp16 values in fp32);
    lowp = "bf16": fp32 arithmetic throughout and ONE rounding of out to bf16 at the store, as the DDIM kernel does for TMIX_BF16 (x0 stays
    fp32).  x0_prev is used only when c1 != 0."""
    x, v = np.asarray(x, F32), np.asarray(v, F32)
    B = x.shape[0]
    lp = None if lowp == "bf16" else lowp
    vv = _cfg(v[:B], v[B:], g, lp)
    x0 = _h(_h(F32(sa) * x, lp) - _h(F32(s1) * vv, lp), lp).astype(F32)
    m = _h(F32(c0) * x0, lp)
    if F32(c1) != 0:
        m = _h(m + _h(F32(c1) * np.asarray(x0_prev, F32), lp), lp)
    out = _h(_h(F32(cx) * x, lp) + m, lp).astype(F32)
    if lowp == "bf16":
        out = _bf16_round(out)
    return out, x0
