"""Shared by tests/test_video_rescale_cpu.py and tests/test_video_rescale_gpu.py: the (shape, layout, data) sweep of tmix_vpred_rescale_factors
 and its data, so that the CPU test runs the kernel's partition in numpy on exactly the cases the GPU test launches.

One video has n = C F hw elements, C = 4.  (F, hw) -> n = 140 (one workgroup of the 32 gets a partial slice), 280, 2240 (nine workgroups), 16,408 (two full
passes of the 8192-element partition plus a ragged tail of 24), 344,064 (42 full passes: the 16-frame clip of the tiny network's largest test size)."""
import numpy as np

NF = np.float32
C = 4
SHAPES = ((1, 35), (2, 35), (16, 35), (2, 2051), (16, 5376))              # (F, hw)
VIDEOS = (1, 3)
LAYOUTS = [(layout, pad) for layout in ("two", "one") for pad in (False, True)]      # two half buffers | one buffer of 2S clips, dense | padded clip stride
DATA = [(m, s) for m in (0.0, 3.0, -100.0) for s in (1.0, 1e-2)]
GS, PHIS = (1.0, 7.5, 9.0, 30.0), (0.25, 0.7, 1.0)
RS_P, RS_THREADS = 32, 256                                                  # csrc/cfg_rescale.hip


def _combo(k):
    """the k-th of the 72 (data, g, phi) combinations in a stride-7 walk (7 is coprime to 72: the first 72 are distinct)"""
    j = (7 * k) % 72
    return DATA[j % 6], GS[(j // 6) % 4], PHIS[j // 24]


def plan_cases():
    """F32 on plan rows: every layout x shape pair, S in VIDEOS -> dicts (40 launches)"""
    out = []
    for F, hw in SHAPES:
        for layout, pad in LAYOUTS:
            for S in VIDEOS:
                (mean, sd), g, phi = _combo(len(out))
                out.append(dict(dt="f32", S=S, F=F, hw=hw, n=C * F * hw, layout=layout, pad=pad, mean=mean, sd=sd, g=g, phi=phi, seed=5000 + len(out)))
    return out


def scalar_cases():
    """F16 and BF16 on the host loop's [2][B][n] layout (20 launches)"""
    out = []
    for dt in ("f16", "bf16"):
        for F, hw in SHAPES:
            for S in VIDEOS:
                (mean, sd), g, phi = _combo(40 + len(out))
                out.append(dict(dt=dt, S=S, F=F, hw=hw, n=C * F * hw, layout="scalar", pad=False, mean=mean, sd=sd, g=g, phi=phi, seed=6000 + len(out)))
    return out


def all_cases():
    return plan_cases() + scalar_cases()


def make_v(case):
    """-> (v_u, v_c) [S, n] fp32 holding values of the case's dtype: an unconditional prediction of the given mean and standard deviation and a
    conditional one near it"""
    import torch
    rng = np.random.RandomState(case["seed"])
    vu = case["mean"] + case["sd"] * rng.randn(case["S"], case["n"])
    vc = vu + 0.5 * case["sd"] * rng.randn(case["S"], case["n"])
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[case["dt"]]
    q = lambda a: torch.from_numpy(a.astype(NF)).to(tdt).float().numpy()
    return q(vu), q(vc)


def lowp_of(dt):
    return {"f32": None, "f16": np.float16, "bf16": "bf16"}[dt]


def ulps(a, b):
    """distance of two fp32 arrays in units in the last place (same sign assumed: factors are positive)"""
    a, b = np.ascontiguousarray(a, NF).reshape(-1), np.ascontiguousarray(b, NF).reshape(-1)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
