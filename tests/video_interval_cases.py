"""Shared by tests/test_video_interval_cpu.py and tests/test_video_interval_gpu.py: inputs of the video sampler's unguided step.

Everything the unguided step computes is compared by equality, so the inputs only have to reach every branch: randn values with no zero (cfg(v, v, g)
gives v back for every g only where v is not -0.0), the hold's weights and held latent of video_hold_cases, small odd shapes -- C = 4, F = 3,
hw = 5 x 7 -- so that video, frame and channel boundaries fall inside one workgroup."""
import numpy as np

import video_hold_cases as VH
from video_hold_cases import C, CZ, F, HA, HH, HS, HW, KEYS, STEP, WW, bits          # noqa: F401  (re-exported)

NF = np.float32
SA, S1 = float(np.sqrt(NF(0.2345))), float(np.sqrt(NF(1) - NF(0.2345)))
DDIM = (float(NF(0.53582)), float(NF(0.78125)))                                    # (sa_next, s1_next or s1_dir)
MOVES = {"ddim": DDIM, "first": tuple(float(NF(v)) for v in (0.8125, 0.3217, 0.0)), "second": tuple(float(NF(v)) for v in (0.8125, 0.4021, -0.0804))}
PACKS = ("plain", "noise", "hold")                                                 # nothing | keys with cz != 0 | keys, cz != 0 and the hold
LOWP = {"f32": None, "f16": np.float16, "bf16": "bf16"}
INTERVAL_N50 = (700, 250)


def rounded(a, dt):
    """fp32 array -> the fp32 copies of its values in the model dtype"""
    from tweediemix_amd import solver as SV
    a = np.asarray(a, NF)
    return a if dt == "f32" else a.astype(np.float16).astype(NF) if dt == "f16" else SV._bf16_round(a)


def case(S, dt, seed, hh=HH, ww=WW, frames=F):
    """-> x, v_c [S, C, F, h, w] (values of the dtype, none of them zero) and an fp32 history of the same shape"""
    rng = np.random.RandomState(seed)
    x, vc, prev = (rng.randn(S, C, frames, hh, ww).astype(NF) for _ in range(3))
    x, vc = rounded(x, dt), rounded(vc, dt)
    assert (x != 0).all() and (vc != 0).all()
    return x, vc, prev


def hold_case(S, seed, hh=HH, ww=WW, frames=F):
    """held latent [S, C, 1, h, w] (one image for every frame) and weight [S, F, h, w] with exact 0, exact 1 and fractions in every frame"""
    return VH.held_latent(S, 1, seed, hh, ww), VH.weight(S, frames, seed + 1, hh, ww)


def reference(kind, pack, x, vc, prev, keys, hold, lowp=None, cz=CZ, step=STEP):
    """the restatement of one unguided step in the form (kind, pack): kind in MOVES, pack in PACKS; hold = (kx, w) -> (out, x0)"""
    from tweediemix_amd import guidance as G
    kz = None if pack == "plain" else keys
    hd = None if pack != "hold" else (hold[0], hold[1], HA, HS)
    return G.vpred_cond_step_reference(x, vc, None if kind == "ddim" else prev, SA, S1, MOVES[kind], cz if kz is not None else 0.0, kz, step, hd, lowp)


def params(kind, pack, g=9.0, cz=CZ, step=STEP, t=501.0):
    """the floats tmix_vpred_step_cond_dev reads, in the guided entries' layouts: 8 without keys, 12 with"""
    m = MOVES[kind]
    head = [t, SA, S1, m[0], m[1], g, 0.0, 0.0] if kind == "ddim" else [t, SA, S1, *m, g, 0.0]
    return head if pack == "plain" else head + [cz, float(step), HA if pack == "hold" else 0.0, HS if pack == "hold" else 0.0]


def interval_orders(ts, interval):
    """is step i second order?  the rule of DESIGN.md 7r restated: the first step and every step whose predecessor had the other guidedness are
    first order"""
    guided = [interval is None or interval[1] <= t <= interval[0] for t in ts]
    return [i > 0 and guided[i] == guided[i - 1] for i in range(len(ts))], guided
