"""Where the constant k of the norm accuracy bound (norm_cases.K, used by test_norm_numerics_gpu.py) comes from: a numpy fp32 model of GroupNorm with
the summation design the bound is derived for -- no sequential fp32 chain longer than 32 terms, fp64 above -- and of the two-pass LayerNorm, run on
every input set of the GPU file.  The model may use at most HALF of the bound (K = 2 x what it needs), so the reference arithmetic provably fits and
the other half is left to what the model does not describe (the order of the device's additions, v_rcp / v_exp in SiLU, rsqrt).  No GPU involved."""
import numpy as np
import pytest
import torch

import norm_cases as N

SHAPES = sorted(set(N.GN_THREE + N.GN_ONE + N.GN_PRE))


def _gn_k(family, r, eps, B, HW, C, silu, seed, groups=N.GROUPS, chain=32):
    x = N.gn_input(family, r, B, HW, C, seed, groups).to(N.BF)
    g, b = N.affine(C, seed)
    R = N.gn_reference(x, g, b, eps, silu, groups)
    y = N.gn_model(x.float().numpy(), g.numpy(), b.numpy(), eps, silu, groups, chain)
    rr = R["r"].expand(B, 1, groups, C // groups).reshape(B, 1, C)
    return N.k_needed(y, R, rr, g.double().view(1, 1, C), silu), R


@pytest.mark.parametrize("fam", N.GN_FAMILIES, ids=N.fam_id)
def test_groupnorm_model_needs_at_most_half_the_bound(fam):
    family, r, eps = fam
    worst = 0.0
    for i, (B, HW, C1, C2, silu) in enumerate(SHAPES):
        k, R = _gn_k(family, r, eps, 1, HW, C1 + C2, silu, 100 + i)           # one image: the groups are independent
        if family in ("offset", "large"):
            N.check_r(R, r, (family, HW, C1 + C2))
        worst = max(worst, k)
    print(f"groupnorm model {N.fam_id(fam)}: k needed {worst:.3f} of K = {N.K}")
    assert worst <= 0.5 * N.K


@pytest.mark.parametrize("r", [3, 30])
def test_groupnorm_model_at_the_vae_size(r):
    """one group of the (1, 1048576, 128) case: 1048576 pixels x 4 channels; in 32-row chains the model stays inside half of the bound.  In the 512-row
    chains gn_stats_kernel ran there before it flushed every 32 rows it needs more than the WHOLE bound at r = 30 (the device missed it 2.9 times)"""
    k, R = _gn_k("offset", r, 1e-6, 1, 1048576, 4, True, 300 + r, groups=1)
    N.check_r(R, r, "vae")
    k512, _ = _gn_k("offset", r, 1e-6, 1, 1048576, 4, True, 300 + r, groups=1, chain=512)
    print(f"groupnorm model at the VAE size, r = {r}: k needed {k:.3f} of K = {N.K} in 32-row chains, {k512:.3f} in 512-row chains")
    assert k <= 0.5 * N.K
    assert r != 30 or k512 > N.K


@pytest.mark.parametrize("r", N.FINAL_R)
@pytest.mark.parametrize("form", ["pre", "three"])
def test_finaliser_models_need_at_most_half_of_ks_final(form, r):
    """the bit-faithful models of the two statistics paths, fp64 finaliser: at most half of KS_FINAL.  With the finaliser's mean, variance and rstd in fp32
    they need more than all of it: the finaliser cases of the GPU file tell an fp32 finaliser"""
    need = N.final_model_rstd_need(form, r, 7000)
    bad = N.final_model_rstd_need(form, r, 7000, fp32_finaliser=True)
    print(f"finaliser model {form} r = {r}: needs {need:.4f} of KS_FINAL = {N.KS_FINAL}; with an fp32 finaliser {bad:.3f}")
    assert need <= 0.5 * N.KS_FINAL
    assert bad > N.KS_FINAL


@pytest.mark.parametrize("fam", N.LN_FAMILIES, ids=N.fam_id)
def test_layernorm_model_needs_at_most_half_the_bound(fam):
    family, r, eps = fam
    worst = 0.0
    for i, (rows, C) in enumerate(N.LN_SHAPES):
        x = N.ln_input(family, r, rows, C, 200 + i).to(N.BF)
        g, b = N.affine(C, 200 + i)
        R = N.ln_reference(x, g, b, eps)
        if family == "offset":
            N.check_r(R, r, (rows, C))
        y = N.ln_model(x.float().numpy(), g.numpy(), b.numpy(), eps)
        worst = max(worst, N.k_needed(y, R, R["r"], g.double().view(1, -1), False, es_power=1))
    print(f"layernorm model {N.fam_id(fam)}: k needed {worst:.3f} of K = {N.K}")
    assert worst <= 0.5 * N.K


def test_bound_tells_a_dropped_eps_and_a_one_pass_layernorm():
    """the bound is tight enough to see the mistakes it is there for (on the model, so this holds without a GPU): eps left out or 1e-5 for 1e-6 at tiny
    variance, and a one-pass E[x^2] - mean^2 LayerNorm at r = 1000"""
    B, HW, C = 1, 256, 320
    x = N.gn_input("tiny", 0, B, HW, C, 7).to(N.BF)
    g, b = N.affine(C, 7)
    for eps_ref, eps_used in ((1e-6, 1e-5), (1e-5, 1e-6), (1e-6, 1e-12)):
        y = torch.from_numpy(N.gn_model(x.float().numpy(), g.numpy(), b.numpy(), eps_used, False)).to(N.BF)
        e, _ = N.gn_err_over_bound(y, x, g, b, eps_ref, False)
        assert float(e.max()) > 10.0, (eps_ref, eps_used, float(e.max()))
    rows, C = 5, 640
    x = N.ln_input("offset", 1000, rows, C, 9).to(N.BF)
    g, b = N.affine(C, 9)
    xf = x.float().numpy()
    mean = xf.sum(1, dtype=np.float32) / np.float32(C)
    var = np.maximum((xf * xf).sum(1, dtype=np.float32) / np.float32(C) - mean * mean, np.float32(0))
    y = (xf - mean[:, None]) * (np.float32(1) / np.sqrt(var + np.float32(1e-5)))[:, None] * g.numpy()[None] + b.numpy()[None]
    e, _ = N.ln_err_over_bound(torch.from_numpy(y).to(N.BF), x, g, b, 1e-5)
    assert float(e.max()) > 1.0, float(e.max())
    e, _ = N.ln_err_over_bound(torch.from_numpy(N.ln_model(xf, g.numpy(), b.numpy(), 1e-5)).to(N.BF), x, g, b, 1e-5)
    assert float(e.max()) <= 1.0, float(e.max())
