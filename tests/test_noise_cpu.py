"""CPU: the counter-based noise of the stochastic sampler without a GPU -- the numpy restatement of csrc/noise.h
(tweediemix_amd/noise.py: Philox4x32-10 known answers, the accuracy of the hand-written Box-Muller, moments and independence of the normals at
fixed keys), the eta coefficients (tweediemix_amd/solver.py) and the variance the two stochastic samplers reach on the scalar Gaussian model
(tests/noise_cases.py: a closed-form covariance recursion), the argument errors of the two ABI entries, the sampler's and the CLI's refusals.
Nothing here opens the GPU; every input is fixed, so every figure is deterministic."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import noise_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = np.float32
N = 1 << 20


# ------------------------------------------------------------------------------------------------ generator
def test_philox_known_answers():
    """{counter; key} -> output: the first and third are Random123's published vectors (kat_vectors, philox4x32 10 rounds)"""
    from tweediemix_amd import noise as NZ
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = NZ.philox4x32_10(ctr, key)
        assert tuple(int(w[0]) for w in got) == want, [hex(int(w[0])) for w in got]
    # vectorised over the counter, and the index's high word is counter word 1
    ctr = np.array([0, 0x243f6a88], np.uint32), np.array([0, 0x85a308d3], np.uint32), np.array([0, 0x13198a2e], np.uint32), np.array([0, 0x03707344], np.uint32)
    assert [int(w[0]) for w in NZ.philox4x32_10(ctr, (0, 0))] == list(kat[0][2])
    idx = np.array([0x85a308d3243f6a88], np.uint64)
    w = NZ.philox4x32_10((idx & np.uint64(0xffffffff), idx >> np.uint64(32), 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert tuple(int(v[0]) for v in w) == kat[2][2]
    assert NZ.normal(idx, 0xa4093822, 0x299f31d0, 0x13198a2e, 0x03707344)[0] == NZ.normal_from_words(kat[2][2][0], kat[2][2][1])[0]
    assert NZ.seed_key(182) == (182, 0) and NZ.seed_key((7 << 32) + 5) == (5, 7) and NZ.seed_key(-1) == (0xffffffff, 0xffffffff)


def test_normal_transform_against_fp64_box_muller():
    """|z - Z| / max(1, |Z|) <= 1e-6 against fp64 Box-Muller on the same uniforms, over 2^20 random word pairs and every pair of the extreme
    words.  Measured: 2.6e-7 (the issue's prototype of this recipe: 2.4e-7); the bound leaves a factor of four for other coefficients."""
    from tweediemix_amd import noise as NZ
    rng = np.random.RandomState(20)
    w = rng.randint(0, 1 << 32, size=(2, N), dtype=np.uint64).astype(np.uint32)
    ex = np.array([0, 0x1ff, 0xffffffff, 0x80000000], np.uint32)
    w0, w1 = np.concatenate([w[0], np.repeat(ex, 4)]), np.concatenate([w[1], np.tile(ex, 4)])
    z = NZ.normal_from_words(w0, w1)
    assert z.dtype == NF and np.isfinite(z).all() and np.abs(z).max() < 5.8
    u1 = ((w0 >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((w1 >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    Z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    err = np.abs(z.astype(np.float64) - Z) / np.maximum(1.0, np.abs(Z))
    print(f"max |z - Z| / max(1, |Z|) = {err.max():.3g}")
    assert err.max() <= 1e-6
    # u1 >= 2^-24: the largest radius is sqrt(2 * 24 ln 2)
    assert abs(float(NZ.normal_from_words(0, 0)[0]) - math.sqrt(48 * math.log(2.0)) * math.cos(math.pi * 2.0 ** -23)) < 1e-5


@pytest.fixture(scope="module")
def normals():
    from tweediemix_amd import noise as NZ
    return NZ.normal(np.arange(N, dtype=np.uint64), 182, 0, 3).astype(np.float64)


def test_moments(normals):
    """over 2^20 normals at fixed key and step every statistic lies within 5 standard errors of its N(0, 1) value"""
    z = normals
    m, v = z.mean(), z.var()
    s = z / math.sqrt(v)
    p2, p3 = math.erfc(2 / math.sqrt(2)), math.erfc(3 / math.sqrt(2))
    stats = [("mean", m, 0.0, 1 / math.sqrt(N)), ("variance", v, 1.0, math.sqrt(2 / N)),
             ("skewness", (s ** 3).mean(), 0.0, math.sqrt(6 / N)), ("excess kurtosis", (s ** 4).mean() - 3.0, 0.0, math.sqrt(24 / N)),
             ("P(|z| > 2)", (np.abs(z) > 2).mean(), p2, math.sqrt(p2 * (1 - p2) / N)),
             ("P(|z| > 3)", (np.abs(z) > 3).mean(), p3, math.sqrt(p3 * (1 - p3) / N))]
    for name, got, want, se in stats:
        print(f"{name}: {got:.6g} (N(0,1): {want:.6g}; {abs(got - want) / se:.2f} standard errors)")
    for name, got, want, se in stats:
        assert abs(got - want) <= 5 * se, name


def test_independence(normals):
    """correlation <= 5 / sqrt(N) between neighbouring indices, neighbouring steps, seeds s and s + 1, and an index against its 2^32 counterpart"""
    from tweediemix_amd import noise as NZ
    idx = np.arange(N, dtype=np.uint64)
    pairs = [("index i, i + 1", normals[:-1], normals[1:]),
             ("step 3, 4", normals, NZ.normal(idx, 182, 0, 4)),
             ("seed 182, 183", normals, NZ.normal(idx, 183, 0, 3)),
             ("key high word 0, 1", normals, NZ.normal(idx, 182, 1, 3)),
             ("index i, i + 2^32", normals, NZ.normal(idx + np.uint64(1 << 32), 182, 0, 3)),
             ("stream 0, 1", normals, NZ.normal(idx, 182, 0, 3, 1))]
    for name, a, b in pairs:
        r = float(np.corrcoef(a, np.asarray(b, np.float64))[0, 1])
        print(f"{name}: correlation {r:.3g} (bound {5 / math.sqrt(N):.3g})")
        assert abs(r) <= 5 / math.sqrt(len(a)), name
        assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ coefficients
def _grid(n, spacing):
    from tweediemix_amd.schedule import Schedule
    s = Schedule(n, spacing=spacing)
    return s, [(s.alpha(s.timesteps[i - 1]), s.alpha(s.timesteps[i]), s.alpha(s.timesteps[i + 1])) for i in range(1, n - 1)]


@pytest.mark.parametrize("spacing,n", [("logsnr", 10), ("leading", 50)])
def test_eta_zero_is_todays_coefficients_and_eta_one_coincides(spacing, n):
    from tweediemix_amd import ops, solver as SV
    for ap, a, an in _grid(n, spacing)[1]:
        assert SV.ddim_eta_coeffs(a, an, 0.0) == ops.step_coeffs(a, an) + (0.0,)
        assert SV.ddim_eta_coeffs(an, a, 0.0) == ops.step_coeffs(an, a) + (0.0,)              # the resampling half's direction too
        for second in (False, True):
            assert SV.multistep_eta_coeffs(ap, a, an, second, 0.0) == SV.multistep_coeffs(ap, a, an, second) + (0.0,)
            assert SV.multistep_eta_coeffs64(ap, a, an, second, 0.0) == SV.multistep_coeffs64(ap, a, an, second) + (0.0,)
        # today's sa, s1, sa_next stay under eta: the x0 of a stochastic step is formed with today's coefficients
        assert SV.ddim_eta_coeffs(a, an, 0.5)[:3] == ops.step_coeffs(a, an)[:3]
        # eta = 1, first order: DDIM in the form cx x + c0 x0 + cz z (eps = (x - sa x0) / s1) is the SDE solver's step, to fp64 rounding
        sa, s1, san, s1d, cz = SV.ddim_eta_coeffs64(a, an, 1.0)
        cx, c0, c1, cz2 = SV.multistep_eta_coeffs64(ap, a, an, False, 1.0)
        assert c1 == 0.0
        assert abs(s1d / s1 - cx) <= 1e-12 * cx and abs(san - s1d * sa / s1 - c0) <= 1e-12 * san and abs(cz - cz2) <= 1e-12 * cz
        # ... and differ in between
        d5, m5 = SV.ddim_eta_coeffs64(a, an, 0.5), SV.multistep_eta_coeffs64(ap, a, an, False, 0.5)
        assert abs(d5[4] - m5[3]) > 1e-3 * m5[3]
        # every step keeps the marginal's noise budget: DDIM s1_dir^2 + cz^2 = 1 - a'; the solver's cx^2 s1^2 + cz^2 = s1'^2
        for eta in (0.3, 1.0):
            d = SV.ddim_eta_coeffs64(a, an, eta)
            assert abs(d[3] ** 2 + d[4] ** 2 - (1 - float(an))) <= 1e-12
            m = SV.multistep_eta_coeffs64(ap, a, an, True, eta)
            assert abs((m[0] * s1) ** 2 + m[3] ** 2 - (1 - float(an))) <= 1e-12
            assert SV.multistep_eta_coeffs(ap, a, an, True, eta) == tuple(float(NF(v)) for v in m)                  # rounded ONCE
            assert SV.ddim_eta_coeffs(a, an, eta)[3:] == (float(NF(d[3])), float(NF(d[4])))
    for bad in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="eta"):
            SV.validate_eta(bad)
    assert SV.validate_eta(1) == 1.0 and SV.validate_eta(0.0) == 0.0


def test_variance_on_the_gaussian_model():
    """data N(0, s^2), eta = 1, closed-form covariance recursion over (x, x0_prev): the relative variance error of dpmpp2m on the log-SNR grid at
    n = 20 is below HALF of DDIM's on 'leading' at n = 40, and every error shrinks from n = 10 to n = 40.  Measured for s = 0.5 / 1 / 2:
    dpmpp2m logsnr n = 10, 20, 40: 6.2e-2 3.1e-2 8.1e-3 / 7.3e-2 3.1e-2 8.0e-3 / 3.5e-2 2.8e-2 7.4e-3;
    ddim leading n = 10, 20, 40: 4.8e-1 3.3e-1 2.1e-1 / 3.5e-1 2.2e-1 1.3e-1 / 3.1e-1 1.8e-1 9.7e-2."""
    def err(c, n, spacing, solver):
        var, sch = NC.predicted_variance(c, n, spacing, solver, 1.0)
        return abs(var - NC.target_variance(c, sch)) / NC.target_variance(c, sch)
    for c in (0.5, 1.0, 2.0):
        ms = {n: err(c, n, "logsnr", "dpmpp2m") for n in (10, 20, 40)}
        dd = {n: err(c, n, "leading", "ddim") for n in (10, 20, 40)}
        print(f"s = {c}: dpmpp2m logsnr {ms}   ddim leading {dd}")
        assert ms[20] < 0.5 * dd[40], c
        assert ms[40] < ms[10] and dd[40] < dd[10], c
    # eta = 0 in the same recursion is the deterministic sampler: no noise enters, the variance is a product of squared gains
    var, _ = NC.predicted_variance(1.0, 10, "logsnr", "dpmpp2m", 0.0)
    assert var > 0


def test_step_restatement_adds_cz_z_to_the_parents_move():
    """noise.step_reference: the parent's restatement bit for bit at cz = 0 and on the last step; cz z added as one product and one sum otherwise"""
    from tweediemix_amd import guidance as G, noise as NZ, solver as SV
    rng = np.random.RandomState(5)
    K, h, w = 3, 4, 6
    x, eps, prev = rng.randn(1, 4, h, w).astype(NF), rng.randn(K + 1, 4, h, w).astype(NF), rng.randn(1, 4, h, w).astype(NF)
    masks = rng.rand(K, 1, h, w).astype(NF)
    f = (0.5 + rng.rand(K)).astype(NF)
    dd = [901.0, 0.6, 0.8, 0.7, 0.71, 0.0, 0.8, 0.0]
    ms = [901.0, 0.6, 0.8, 0.9, 0.3, -0.1, 0.0, 0.8]
    key = (182, 0)
    for mode, m in ((SV.STEP_FUSION, masks), (SV.STEP_PLAIN, None)):
        want = G.rescaled_step_reference(mode, x, eps, m, K if m is not None else 1, np.ones(K, NF), dd[6], *dd[1:5], False)
        got = NZ.step_reference(mode, x, eps, m, None, dd + [0.0, 7.0, 0.0, 0.0], key)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        want = SV.multistep_step_reference(mode, x, eps, m, prev, ms[7], ms[1], ms[2], ms[3], ms[4], ms[5], False)
        got = NZ.step_reference(mode, x, eps, m, prev, ms + [0.0, 7.0, 0.0, 0.0], key)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        z = NZ.normal(np.arange(x.size, dtype=np.uint64).reshape(x.shape), 182, 0, 7)
        got2 = NZ.step_reference(mode, x, eps, m, prev, ms + [0.25, 7.0, 0.0, 0.0], key)
        assert np.array_equal(got2[0], (want[0] + (NF(0.25) * z).astype(NF)).astype(NF)) and np.array_equal(got2[1], want[1])
        want = G.rescaled_multistep_reference(mode, x, eps, m, prev, f, ms[7], ms[1], ms[2], ms[3], ms[4], ms[5], False)
        got3 = NZ.step_reference(mode, x, eps, m, prev, ms + [0.25, 7.0, 0.0, 0.0], key, factors=f)
        assert np.array_equal(got3[0], (want[0] + (NF(0.25) * z).astype(NF)).astype(NF))
        last = list(ms)
        last[6] = 1.0
        got4 = NZ.step_reference(mode, x, eps, m, prev, last + [0.25, 7.0, 0.0, 0.0], key)
        assert np.array_equal(got4[0], got[1]) and np.array_equal(got4[1], got[1])           # the last step writes x0 itself
    # a window's indices are the canvas's: the crop of the canvas-indexed noise
    full = NZ.normal(NZ.canvas_index(4, 16, 24), 5, 0, 2)
    win = NZ.normal(NZ.canvas_index(4, 16, 16, 0, 8, 16, 24), 5, 0, 2)
    assert np.array_equal(win, full[:, :, 8:24])


# ------------------------------------------------------------------------------------------------ ABI
def test_entries_are_declared_and_validate_before_any_launch():
    from tweediemix_amd import lib
    l = lib.load()
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    assert "int tmix_noise_normal(" in src and "int tmix_fused_tweedie_step_noise_dev(" in src
    err = l.tmix_last_error_string
    f = 0x1000                                                  # never dereferenced: validation fails first
    assert l.tmix_noise_normal(None, 4, 0, 1, 2, 3, 0, None) == lib.EINVAL and b"null" in err()
    assert l.tmix_noise_normal(f, 0, 0, 1, 2, 3, 0, None) == lib.ESHAPE
    assert l.tmix_noise_normal(f, 4, -1, 1, 2, 3, 0, None) == lib.ESHAPE
    ok = dict(x=f, eps=f, dt=lib.F32, masks=f, mss=0, out_x=f, out_x0=None, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=4, seeds=2, prm=f,
              prev=None, fac=None, keys=f, w=8, n_win=1, yx=None, ch=0, cw=0)

    def rc(**kw):
        a = dict(ok, **kw)
        yx = a["yx"]
        if yx is not None:
            yx = (C.c_int32 * len(yx))(*yx)
        return l.tmix_fused_tweedie_step_noise_dev(a["x"], a["eps"], a["dt"], a["masks"], a["mss"], a["out_x"], a["out_x0"], a["K"], a["C"], a["hw"],
                                                   a["mode"], a["rows"], a["seeds"], a["prm"], a["prev"], a["fac"], a["keys"], a["w"], a["n_win"],
                                                   yx, a["ch"], a["cw"], None)
    for k in ("x", "eps", "out_x", "prm"):
        assert rc(**{k: None}) == lib.EINVAL and b"null" in err(), k
    assert rc(keys=None) == lib.EINVAL and b"keys" in err()
    assert rc(mode=lib.STEP_RESAMPLE) == lib.EINVAL and b"mode" in err()
    assert rc(mode=lib.STEP_RESAMPLE, prev=f) == lib.EINVAL
    assert rc(masks=None) == lib.EINVAL and b"masks" in err()
    for nw in (0, -1, lib.MAX_WINDOWS + 1):
        assert rc(n_win=nw, yx=[0, 0] * max(nw, 1), ch=8, cw=8) == lib.EINVAL and b"n_win" in err(), nw
    assert rc(n_win=2) == lib.EINVAL                            # two windows need their table
    assert rc(w=7) == lib.ESHAPE and b"w=7" in err()
    assert rc(w=0) == lib.ESHAPE
    assert rc(seeds=3, n_win=2, yx=[0, 0, 0, 4], ch=8, cw=12) == lib.ESHAPE and b"multiple" in err()
    for yx in ([0, 0, 0, 5], [0, 0, 1, 4], [-1, 0, 0, 4], [0, -1, 0, 4]):
        assert rc(n_win=2, yx=yx, ch=8, cw=12) == lib.ESHAPE and b"canvas" in err(), yx
    assert rc(rows=3) == lib.ESHAPE and b"rows" in err()          # the parents' checks
    for bad in (dict(C=0), dict(hw=0), dict(seeds=0), dict(seeds=65536)):
        assert rc(**bad) == lib.ESHAPE, bad
    assert rc(dt=7) == lib.EINVAL and b"dtype" in err()
    assert rc(dt=7, prev=f, fac=f) == lib.EINVAL


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    z = torch.zeros(1, 4, 4, 4)
    with pytest.raises(lib.TmixError):
        ops.fused_tweedie_step_noise_dev(z, torch.zeros(2, 4, 4, 4), None, lib.STEP_PLAIN, 1, torch.zeros(12), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(lib.TmixError):
        ops.noise_normal(4, 0, (1, 2), 3, out=torch.zeros(4))
    k = ops.noise_keys([182, (7 << 32) + 0xfffffffe], "cpu")
    assert k.dtype == torch.int32 and k.tolist() == [[182, 0], [-2, 7]]


# ------------------------------------------------------------------------------------------------ sampler
class NoWeights:
    device = torch.device("cpu")
    kind = "custom"


def _sampler(n=10, **kw):
    from tweediemix_amd import sampler as S
    cfg = S.make_config(n_timesteps=n, resolution_h=128, resolution_w=128, resampling_steps=2, jumping_steps=1, t_cond=0.2, guidance_scale=0.8)
    masks = torch.ones(3, 1, 16, 16) / 3
    return S.Tweediemix(cfg, NoWeights(), None, None, lambda x0: masks, concept_num=3, **kw)


def test_sampler_refusals_and_defaults():
    tw = _sampler()
    assert tw.eta == 0.0 and tw._noise_keys is None and tw.step_params.numel() == 8
    for bad in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            _sampler(eta=bad, noise_seeds=[1])
    with pytest.raises(ValueError, match="noise_seeds"):
        _sampler(eta=0.5)
    with pytest.raises(ValueError, match="2 values for 1 trajectories"):
        _sampler(eta=0.5, noise_seeds=[1, 2])
    tw = _sampler(eta=0.5, noise_seeds=[(9 << 32) + 4])
    assert tw.step_params.numel() == 12 and tw._noise_keys.tolist() == [[4, 9]]
    tw.set_noise_seeds([5])
    assert tw._noise_keys.tolist() == [[5, 0]]
    z = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match=r"set_keep.*eta=0.5"):
        tw.set_keep(z, z[:, :1], z)
    assert _sampler(eta=0.0, noise_seeds=[3]).step_params.numel() == 8       # seeds without eta: today's sampler


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_which_steps_take_noise(solver):
    """host bookkeeping alone: the one advancing move of every schedule entry carries that entry's index; resampling round trips and the look-ahead
    carry none; with eta = 0 no call passes step_index at all (today's calls)"""
    from tweediemix_amd import lib as L, solver as SV
    for eta in (0.0, 0.7):
        tw = _sampler(10, solver=solver, eta=eta, noise_seeds=[11], timestep_spacing="logsnr")
        log = []
        tw._run_step = lambda *a, **k: log.append((a, k))
        tw.run_fusion(torch.zeros(1, 4, 16, 16))
        ts, ic = tw.scheduler.timesteps, tw._window_index(0.2)
        assert len(log) == 10 + 2 * 2 + 1 and ic >= 2
        if eta == 0.0:
            assert all("step_index" not in k for _a, k in log)
            continue
        adv = [(a, k) for a, k in log if "step_index" in k]
        assert [k["step_index"] for _a, k in adv] == list(range(10)) and [a[2] for a, _k in adv] == ts
        rest = [(a, k) for a, k in log if "step_index" not in k]
        assert [(a[0], a[1]) for a, _k in rest[:4]] == [("start", L.STEP_RESAMPLE), ("plain", L.STEP_PLAIN)] * 2       # the round trips
        assert rest[4][0][:3] == ("plain", L.STEP_PLAIN, ts[ic]) and len(rest) == 5                                    # the look-ahead
        assert adv[0][0][:2] == ("start", L.STEP_PLAIN) and adv[0][1].get("ms") is None                                # the start timestep's last step
        for i, (a, k) in enumerate(adv[1:], 1):
            if solver == "ddim":
                assert k.get("ms") is None
            elif i == 9:
                assert k["ms"] == (0.0, 1.0, 0.0, 0.0)
            else:
                second = i not in (1, ic)                        # the first solver step and the first fusion step are first order
                assert k["ms"] == SV.multistep_eta_coeffs(tw.alpha(ts[i - 1]), tw.alpha(ts[i]), tw.alpha(ts[i + 1]), second, eta), i
                assert len(k["ms"]) == 4 and k["ms"][3] > 0.0
    with pytest.raises(ValueError, match="not one of the schedule's timesteps"):
        tw = _sampler(10, eta=0.5, noise_seeds=[1])
        tw._run_step = lambda *a, **k: None
        tw.init_fusion(2)
        tw.denoise_step(torch.zeros(1, 4, 16, 16), 650)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def fs():
    spec = importlib.util.spec_from_file_location("fs_noise_cpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


BASE = ["--synthetic", "--tiny", "--concepts", "a+b+bg", "--seg_concepts", "a cat+a dog", "--resolution_h", "128", "--resolution_w", "128"]


def test_cli_eta_refusals_come_before_the_gpu(fs, tmp_path, monkeypatch):
    opt = fs.build_parser().parse_args([])
    assert opt.eta == 0.0 and fs.check_solver_args(opt) is None
    opt = fs.build_parser().parse_args(["--eta", "0.5", "--solver", "dpmpp2m"])
    assert opt.eta == 0.5 and fs.check_solver_args(opt) is None
    assert "coincide at 0 and 1" in fs.build_parser().format_help()
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "ok.latent.pt")
    keep = ["--mask_paths", "a.png+b.png", "--reroll", "1"]

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match=r"--eta"):
            fs.main(BASE + ["--eta=" + bad])
    with pytest.raises(SystemExit, match=r"--eta 0.5 does not combine with --keep_latents"):
        fs.main(BASE + ["--eta", "0.5", "--keep_latents", str(tmp_path / "ok.latent.pt")] + keep)
    with pytest.raises(SystemExit):
        fs.build_parser().parse_args(["--eta", "much"])
