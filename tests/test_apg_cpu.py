"""CPU: adaptive projected guidance (arXiv:2410.02416) -- the numpy restatements of tweediemix_amd.guidance against hand-computed
elements, their properties in fp64, the kernel's partition order restated in numpy against the restatement's own bound, the declarations and the
argument errors of tmix_apg_coeffs / tmix_fused_tweedie_step_apg_dev (reported on the host before any launch), and the refusals of the sampler and
of both scripts before anything touches the device."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import apg_cases as AC

NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSION, PLAIN, RESAMPLE = 0, 1, 2


# ------------------------------------------------------------------------------------------------ hand-computed elements
def _hand():
    """sa = s1 = 0.5 make t = 2 x - e exact: x = [1, 2], eu = [0, 2], ec = [2, -2] -> tu = [2, 2], tc = [0, 6], d = [-2, 4];
    Sdd = 20, Sdc = 24, Scc = 36"""
    x = np.array([1.0, 2.0], NF).reshape(1, 1, 1, 2)
    eps = np.array([[0.0, 2.0], [2.0, -2.0]], NF).reshape(2, 1, 1, 2)
    return x, eps


def test_restatement_against_hand_computed_elements():
    from tweediemix_amd import guidance as G
    x, eps = _hand()
    tc, d = G._apg_terms(x, eps, NF(0.5), NF(0.5), None)
    assert np.array_equal(tc.reshape(-1), [0.0, 6.0]) and np.array_equal(d.reshape(-1), [-2.0, 4.0])
    assert np.array_equal(G.apg_sums_reference(x, eps, NF(0.5), NF(0.5)), [[20.0, 24.0, 36.0]])
    # g = 3, eta = 0.5, no clip: s = 1, p = 24 / 36, A = 1 - 2 * 0.5 * 2/3 = 1/3, B = 2
    ab = G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 0.5, 0.0)
    assert ab.dtype == NF and ab.shape == (1, 2) and ab[0, 0] == NF(1.0 - 2.0 * 0.5 * (24.0 / 36.0)) and ab[0, 1] == NF(2.0)
    # eta = 1: CFG in data space whatever the sums; eta = 0: A = 1 - 2 * 2/3 = -1/3
    assert np.array_equal(G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 1.0, 0.0), [[1.0, 2.0]])
    assert G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 0.0, 0.0)[0, 0] == NF(1.0 - 2.0 * (24.0 / 36.0))
    # R = 2 < sqrt(20): s = 2 / sqrt(20), p = s * 24 / 36, A = 1 - 2 * 0.5 * p, B = 2 s;  R = 5 > sqrt(20): no clip
    s = 2.0 / math.sqrt(20.0)
    ab = G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 0.5, 2.0)
    assert ab[0, 0] == NF(1.0 - 2.0 * 0.5 * (s * 24.0 / 36.0)) and ab[0, 1] == NF(2.0 * s)
    assert np.array_equal(G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 0.5, 5.0), G.apg_coeffs_reference(PLAIN, x, eps, 1, 3.0, 0.5, 0.5, 0.5, 0.0))
    # the step on exact coefficients: t = A tc + B d = 0.5 * [0, 6] + 2 * [-2, 4] = [-4, 11]; DDIM move 0.25 x0 + 0.5 eu; the last step writes x0
    co = np.array([[0.5, 2.0]], NF)
    prm = [9.0, 0.5, 0.5, 0.25, 0.5, 0.0, 3.0, 0.0]
    out, x0 = G.apg_step_reference(PLAIN, x, eps, None, 1, co, prm)
    assert np.array_equal(x0.reshape(-1), [-4.0, 11.0]) and np.array_equal(out.reshape(-1), [-1.0, 2.75 + 1.0])
    out, x0 = G.apg_step_reference(PLAIN, x, eps, None, 1, co, prm[:5] + [1.0, 3.0, 0.0])
    assert np.array_equal(out, x0) and np.array_equal(x0.reshape(-1), [-4.0, 11.0])
    # 2M move cx x + c0 x0 + c1 prev = 0.5 * [1, 2] + 0.25 * [-4, 11] + 2 * [1, -1]; c1 = 0 never reads the history
    prev = np.array([1.0, -1.0], NF).reshape(x.shape)
    out, x0 = G.apg_multistep_reference(PLAIN, x, eps, None, prev, co, [9.0, 0.5, 0.5, 0.5, 0.25, 2.0, 0.0, 3.0])
    assert np.array_equal(x0.reshape(-1), [-4.0, 11.0]) and np.array_equal(out.reshape(-1), [0.5 - 1.0 + 2.0, 1.0 + 2.75 - 2.0])
    out, _ = G.apg_multistep_reference(PLAIN, x, eps, None, np.full_like(prev, np.nan), co, [9.0, 0.5, 0.5, 0.5, 0.25, 0.0, 0.0, 3.0])
    assert np.array_equal(out.reshape(-1), [0.5 - 1.0, 1.0 + 2.75])
    # FUSION blends the rows' t with the masks; RESAMPLE is (K - 1) t_1 - sum of the single rows' t
    eps3 = np.concatenate([eps, eps[1:] * NF(0.5)])                       # row 2: ec = [1, -1] -> tc = [1, 5], d = [-1, 3]
    co2 = np.array([[0.5, 2.0], [1.0, 1.0]], NF)                         # t_2 = [0, 8]
    masks = np.array([[0.25, 1.0], [0.75, 0.0]], NF).reshape(2, 1, 1, 2)
    assert np.array_equal(G.apg_x0_reference(FUSION, x, eps3, masks, 2, co2, 0.5, 0.5).reshape(-1), [-1.0, 11.0])
    assert np.array_equal(G.apg_x0_reference(RESAMPLE, x, eps3, None, 2, co2, 0.5, 0.5).reshape(-1), [-4.0, 3.0])
    # fp16 eps: s1 * e is rounded to fp16 before it is subtracted
    xh, eh = np.array([1.0], NF).reshape(1, 1, 1, 1), np.array([0.0, 1.0 + 2.0 ** -10], NF).reshape(2, 1, 1, 1)
    tc, _ = G._apg_terms(xh, eh, NF(1.0), NF(1.0 + 2.0 ** -10), np.float16)
    assert tc.reshape(-1)[0] == NF(1.0) - NF(np.float16((1.0 + 2.0 ** -10) ** 2))


def test_fallbacks_and_rows_the_mode_does_not_read():
    from tweediemix_amd import guidance as G
    x, eps = _hand()
    rng = np.random.RandomState(0)
    X, E = rng.randn(1, 4, 3, 5).astype(NF), rng.randn(5, 4, 3, 5).astype(NF)
    gm1 = NF(float(NF(7.5)) - 1.0)
    ab = G.apg_coeffs_reference(PLAIN, X, E, 3, 7.5, 0.6, 0.8, 0.0, 0.0)
    assert ab.shape == (4, 2) and np.array_equal(ab[1:], np.tile([[1.0, gm1]], (3, 1))) and ab[0, 0] != 1.0
    ab = G.apg_coeffs_reference(FUSION, X, E, 3, 7.5, 0.6, 0.8, 0.0, 0.0)
    assert np.array_equal(ab[3], [1.0, gm1]) and np.all(ab[:3, 0] != 1.0)
    with pytest.raises(ValueError, match="eps rows"):
        G.apg_coeffs_reference(FUSION, X, E[:3], 3, 7.5, 0.6, 0.8, 0.0, 0.0)
    # ec == eu: d = 0, every sum with d is zero -> s = 1, p = 0 -> (1, g - 1)
    same = np.concatenate([E[:1], E[:1]])
    assert np.array_equal(G.apg_coeffs_reference(PLAIN, X, same, 1, 7.5, 0.6, 0.8, 0.0, 3.0), [[1.0, gm1]])
    # an all-zero tc (x = s1 ec): Scc = 0 -> p = 0 -> A = 1, B = (g - 1) s
    x0, e0 = np.full((1, 1, 1, 4), 0.5, NF), np.stack([np.zeros(4, NF), np.ones(4, NF)]).reshape(2, 1, 1, 4)
    ab = G.apg_coeffs_reference(PLAIN, x0, e0, 1, 7.5, 0.5, 0.5, 0.0, 0.0)
    assert np.array_equal(ab, [[1.0, gm1]])
    # an inf in eps: a sum is not finite -> (1, g - 1) for that row alone
    bad = E.copy()
    bad[2, 0, 0, 0] = np.inf
    ab = G.apg_coeffs_reference(FUSION, X, bad, 3, 7.5, 0.6, 0.8, 0.0, 0.0)
    assert np.array_equal(ab[1], [1.0, gm1]) and ab[0, 0] != 1.0 and ab[2, 0] != 1.0


def test_validate_apg():
    from tweediemix_amd import guidance as G
    assert G.validate_apg(None) is None and G.validate_apg(False) is None
    assert G.validate_apg(True) == G.validate_apg({}) == dict(eta=0.0, norm_threshold=0.0)
    assert G.validate_apg(dict(eta=1, norm_threshold=np.float32(15))) == dict(eta=1.0, norm_threshold=15.0)
    for bad in (dict(eta=-0.1), dict(eta=1.1), dict(eta=float("nan")), dict(norm_threshold=-1.0), dict(norm_threshold=float("inf")), dict(eta="0"),
                dict(eta=True), dict(beta=0.5), dict(norm_threshold=1e39), 0.5, "on", [0.0, 0.0]):
        with pytest.raises(ValueError, match="apg"):
            G.validate_apg(bad)


# ------------------------------------------------------------------------------------------------ properties in fp64
def _fp64_case(seed, n=4 * 9 * 11):
    from tweediemix_amd import guidance as G
    rng = np.random.RandomState(seed)
    x = rng.randn(1, 4, 9, 11).astype(NF)
    eu = rng.randn(1, 4, 9, 11)
    eps = np.concatenate([eu, eu + 0.5 * rng.randn(1, 4, 9, 11)]).astype(NF)
    sa, s1 = AC.sa_s1(AC.ALPHAS[seed % 3])
    tc, d = G._apg_terms(x, eps, NF(sa), NF(s1), None)
    return tc.astype(np.float64).reshape(-1), d.astype(np.float64).reshape(-1), G.apg_sums_reference(x, eps, NF(sa), NF(s1))[0]


@pytest.mark.parametrize("seed", range(6))
def test_properties_of_the_restatement_in_fp64(seed):
    """on the restatement's own fp32 terms, everything behind them in fp64 (the constants are fp64 round-off margins)"""
    from tweediemix_amd import guidance as G
    tc, d, sums = _fp64_case(seed)
    g = AC.GS[1 + seed % 3]
    nrm = np.linalg.norm
    # eta = 1, R = 0 is CFG's x0
    A, B, s = G.apg_finalise(sums, g, 1.0, 0.0)
    D, cfg = A * tc + B * d, tc + (float(NF(g)) - 1.0) * d
    assert s == 1.0 and nrm(D - cfg) <= 1e-12 * nrm(cfg)
    # eta = 0: the update has no part along D_c -- with and without a clip
    for R in (0.0, 0.5 * math.sqrt(sums[0])):
        A, B, s = G.apg_finalise(sums, g, 0.0, R)
        D = A * tc + B * d
        assert abs(np.dot(D - tc, tc)) <= 1e-10 * nrm(D - tc) * nrm(tc) and nrm(D - tc) > 0
    # 0 < eta < 1: the parallel part is eta times CFG's, the orthogonal part is CFG's
    A, B, s = G.apg_finalise(sums, g, 0.3, 0.0)
    D = A * tc + B * d
    par = lambda v: np.dot(v, tc) / np.dot(tc, tc)
    assert abs(par(D - tc) - float(NF(0.3)) * par(cfg - tc)) <= 1e-10 * abs(par(cfg - tc))
    assert nrm((D - tc) - par(D - tc) * tc - ((cfg - tc) - par(cfg - tc) * tc)) <= 1e-10 * nrm(cfg - tc)
    # the clip: ||s d|| <= R (1 + 1e-12), and s = 1 when ||d|| <= R
    nd = math.sqrt(sums[0])
    for R in (0.1 * nd, 0.999 * nd):
        R = float(NF(R))
        _A, _B, s = G.apg_finalise(sums, g, 0.0, R)
        assert s < 1.0 and s * nrm(d) <= R * (1 + 1e-12)
    for R in (float(NF(1.001 * nd)), 1e4, 0.0):
        assert G.apg_finalise(sums, g, 0.0, R)[2] == 1.0


# ------------------------------------------------------------------------------------------------ the kernel's partition order, in numpy
@pytest.mark.parametrize("dt", AC.DTS)
@pytest.mark.parametrize("mode", AC.MODES)
def test_partition_order_stays_inside_the_bound(mode, dt):
    """the fp64 products summed in the order of the kernels (32 workgroups x 256 threads, wave butterfly, waves, partials) give (A, B) inside the
    bound the GPU test applies, at the GPU test's shapes -- the bound comes from the restatement, not from what a kernel returned"""
    worst = 0
    for c in AC.coeff_cases(mode, dt):
        x, _eps_t, eps, prm = AC.coeff_inputs(c)
        ref, bound = AC.coeffs_reference(c, x, eps, prm)
        got = AC.partition_coeffs(c, x, eps, prm)
        assert AC.ulps(got[..., 1], ref[..., 1]).max() <= 1, c
        assert np.all(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]) <= bound), (c, got[..., 0], ref[..., 0], bound)
        worst = max(worst, int(AC.ulps(got, ref).max()))
    print(f"partition order {mode} {dt}: worst distance {worst} ulp")


def test_partition_sums_of_a_known_row():
    """integers: every order gives the same sums, so the restated partition can be checked against the plain one -- ragged tail and empty workgroups too"""
    for n in (5, 1024, 8212, 16400):
        tc, d = (np.arange(n) % 7 - 3).astype(NF), (np.arange(n) % 5 - 2).astype(NF)
        want = [float((d.astype(np.float64) ** 2).sum()), float((d.astype(np.float64) * tc).sum()), float((tc.astype(np.float64) ** 2).sum())]
        assert AC.partition_sums(tc, d) == want, n


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "double*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int,
          "int64_t": C.c_int64, "float": C.c_float, "const uint32_t*": C.c_void_p, "const int*": C.POINTER(C.c_int32)}


def _prototype(name, res="int", header="tmix.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/{header}"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_header_lists_the_new_symbols_and_ctypes_agrees():
    from tweediemix_amd import lib
    dev, noise = _prototype("tmix_fused_tweedie_step_dev"), _prototype("tmix_fused_tweedie_step_noise_dev")
    apg = _prototype("tmix_fused_tweedie_step_apg_dev", header="tmix_apg.h")      # the extension header: tmix.h keeps its own entries
    assert apg[:14] == dev[:14]                                              # the 14 leading arguments of tmix_fused_tweedie_step_dev
    assert [n for _t, n in apg[14:]] == ["x0_prev", "coeffs", "keys", "w", "n_win", "win_yx", "canvas_h", "canvas_w", "stream"]
    assert apg[14] == noise[14] and apg[15] == ["const float*", "coeffs"] and apg[16:] == noise[16:]      # patterned on the noise entry
    co = _prototype("tmix_apg_coeffs", header="tmix_apg.h")
    assert [n for _t, n in co] == ["x", "eps", "eps_dtype", "coeffs", "ws", "K", "channels", "hw", "mode", "rows", "seeds", "params", "g_slot", "eta",
                                   "norm_threshold", "stream"]
    l = lib.load()
    for name, proto in (("tmix_fused_tweedie_step_apg_dev", apg), ("tmix_apg_coeffs", co)):
        r, args = lib.SIGNATURES_APG[name]
        assert r is C.c_int and args == [_CTYPE[t] for t, _n in proto], name
        assert getattr(l, name).argtypes == args and name not in lib.SIGNATURES
    # the extension header declares exactly the table's entries, and includes tmix.h for the conventions
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix_apg.h")).read(), flags=re.S)
    assert sorted(re.findall(r"\b(tmix_\w+)\s*\(", src)) == sorted(lib.SIGNATURES_APG) and '#include "tmix.h"' in src


def test_entries_validate_before_any_launch():
    """pointers that are never dereferenced: every refusal comes back with its code from the host-side checks"""
    from tweediemix_amd import lib
    l = lib.load()
    p = 0x1000
    err = l.tmix_last_error_string
    ok = dict(x=p, eps=p, dt=lib.F32, co=p, ws=p, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=4, seeds=1, prm=p, slot=6, eta=0.0, R=0.0)

    def rc(**kw):
        a = dict(ok, **kw)
        return l.tmix_apg_coeffs(a["x"], a["eps"], a["dt"], a["co"], a["ws"], a["K"], a["C"], a["hw"], a["mode"], a["rows"], a["seeds"], a["prm"],
                                 a["slot"], a["eta"], a["R"], None)
    for k in ("x", "eps", "co", "ws", "prm"):
        assert rc(**{k: None}) == lib.EINVAL and b"null" in err(), k
    assert rc(dt=3) == lib.EINVAL and b"dtype" in err() and rc(dt=-1) == lib.EINVAL
    assert rc(mode=3) == lib.EINVAL and b"mode" in err() and rc(mode=-1) == lib.EINVAL
    assert rc(K=0) == lib.EINVAL and rc(K=0, mode=lib.STEP_RESAMPLE) == lib.EINVAL
    assert rc(C=0) == lib.ESHAPE and rc(hw=0) == lib.ESHAPE
    assert rc(rows=3) == lib.ESHAPE and b"rows" in err() and rc(mode=lib.STEP_PLAIN, rows=1) == lib.ESHAPE and rc(rows=257) == lib.ESHAPE
    assert rc(mode=lib.STEP_RESAMPLE, rows=3) == lib.ESHAPE
    assert rc(seeds=0) == lib.ESHAPE and rc(seeds=65536) == lib.ESHAPE
    assert rc(slot=-1) == lib.EINVAL and b"g_slot" in err() and rc(slot=8) == lib.EINVAL
    for eta in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert rc(eta=eta) == lib.EINVAL and b"eta" in err(), eta
    for R in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert rc(R=R) == lib.EINVAL and b"norm_threshold" in err(), R

    sok = dict(x=p, eps=p, dt=lib.F32, masks=p, mss=0, out_x=p, out_x0=None, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=4, seeds=1, prm=p, prev=None,
               co=p, keys=None, w=8, n_win=1)

    def step(**kw):
        a = dict(sok, **kw)
        return l.tmix_fused_tweedie_step_apg_dev(a["x"], a["eps"], a["dt"], a["masks"], a["mss"], a["out_x"], a["out_x0"], a["K"], a["C"], a["hw"], a["mode"],
                                                 a["rows"], a["seeds"], a["prm"], a["prev"], a["co"], a["keys"], a["w"], a["n_win"], None, 0, 0, None)
    for prev in (None, p):
        assert step(prev=prev, co=None) == lib.EINVAL and b"coeffs" in err()
        for k in ("x", "eps", "out_x", "prm"):
            assert step(prev=prev, **{k: None}) == lib.EINVAL and b"null" in err(), k
        assert step(prev=prev, mode=3) == lib.EINVAL and step(prev=prev, mode=-1) == lib.EINVAL and step(prev=prev, dt=7) == lib.EINVAL
        assert step(prev=prev, masks=None) == lib.EINVAL and step(prev=prev, K=0) == lib.EINVAL
        assert step(prev=prev, rows=3) == lib.ESHAPE and step(prev=prev, mode=lib.STEP_PLAIN, rows=1) == lib.ESHAPE
        for bad in (dict(C=0), dict(hw=0), dict(seeds=0), dict(seeds=65536)):
            assert step(prev=prev, **bad) == lib.ESHAPE, bad
        # with keys: the noise entry's window checks
        assert step(prev=prev, keys=p, n_win=0) == lib.EINVAL and step(prev=prev, keys=p, n_win=2) == lib.EINVAL
        assert step(prev=prev, keys=p, w=7) == lib.ESHAPE and step(prev=prev, keys=p, w=0) == lib.ESHAPE
    assert step(mode=lib.STEP_RESAMPLE, prev=p) == lib.EINVAL and b"RESAMPLE" in err()
    assert step(mode=lib.STEP_RESAMPLE, keys=p) == lib.EINVAL and b"RESAMPLE" in err()
    assert step(mode=lib.STEP_RESAMPLE, rows=3) == lib.ESHAPE


def test_ops_wrappers_refuse_cpu_tensors_and_bad_settings():
    from tweediemix_amd import lib, ops
    z, e, prm = torch.zeros(1, 4, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(8)
    with pytest.raises(lib.TmixError):
        ops.apg_coeffs(z, e, lib.STEP_PLAIN, 1, prm, 6)
    with pytest.raises(lib.TmixError):
        ops.fused_tweedie_step_apg_dev(z, e, None, lib.STEP_PLAIN, 1, prm, torch.ones(1, 1, 2))
    with pytest.raises(ValueError, match="apg_coeffs"):
        ops.apg_coeffs(z, e, lib.STEP_PLAIN, 1, prm, 6, eta=1.5)


# ------------------------------------------------------------------------------------------------ sampler and CLI
class NoWeights:
    device = torch.device("cpu")
    kind = "custom"


def _sampler(**kw):
    from tweediemix_amd import sampler as S
    cfg = S.make_config(n_timesteps=10, resolution_h=128, resolution_w=128, resampling_steps=2, jumping_steps=1, t_cond=0.4, t_stop=0.9, guidance_scale=9.0)
    masks = torch.ones(3, 1, 16, 16) / 3
    return S.Tweediemix(cfg, NoWeights(), None, None, lambda x0: masks, concept_num=3, **kw)


def test_sampler_default_refusals_and_buffers(monkeypatch):
    tw, off = _sampler(), _sampler(apg=None)
    for t in (tw, off):                                          # flag off: nothing new is allocated
        assert t.apg is None and t._apg_coeffs is None and t._apg_ws is None
    assert sorted(k for k, v in vars(tw).items() if torch.is_tensor(v)) == sorted(k for k, v in vars(off).items() if torch.is_tensor(v))
    z = torch.zeros(1, 4, 16, 16)
    tw.set_keep(z, z[:, :1], z)                                  # the default sampler takes a keep region
    for bad in (dict(eta=-0.1), dict(eta=2.0), dict(norm_threshold=-1.0), dict(norm_threshold=float("nan")), dict(momentum=0.5), 0.5, "on"):
        with pytest.raises(ValueError, match="apg"):
            _sampler(apg=bad)
    on = _sampler(apg=dict(eta=0.25, norm_threshold=15.0), n_seeds=2)
    assert on.apg == dict(eta=0.25, norm_threshold=15.0) and tuple(on._apg_coeffs.shape) == (2 * 3 * 2,) and on._apg_ws.dtype == torch.float64
    assert on._rs_factors is None and on._rs_ws is None
    assert _sampler(apg={}).apg == dict(eta=0.0, norm_threshold=0.0)
    with pytest.raises(ValueError, match=r"set_keep.*apg="):
        on.set_keep(torch.zeros(2, 4, 16, 16), z[:, :1], torch.zeros(2, 4, 16, 16))
    assert on._keep is None
    # the combination with the rescale is refused before a buffer is made (torch.zeros is the first allocation of the constructor)
    def no_alloc(*a, **k):
        raise AssertionError("a buffer was allocated before the refusal")
    monkeypatch.setattr(torch, "zeros", no_alloc)
    with pytest.raises(ValueError, match=r"apg=.*guidance_rescale=0.7"):
        _sampler(apg={}, guidance_rescale=0.7)
    monkeypatch.undo()
    assert _sampler(apg={}, solver="dpmpp2m", timestep_spacing="logsnr")._x0_prev is not None
    assert _sampler(apg={}, eta=0.5, noise_seeds=[3]).step_params.numel() == 12
    assert _sampler(apg={}, guidance_interval=(700, 250)).guidance_interval == (700, 250)


def _load(script, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "fusion_generation", script))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


BASE = ["--synthetic", "--tiny", "--concepts", "a+b+bg", "--seg_concepts", "a cat+a dog", "--resolution_h", "128", "--resolution_w", "128"]


def test_both_scripts_accept_the_flags_and_refuse_before_the_gpu(tmp_path, monkeypatch):
    fs = _load("fusion_sampling.py", "fs_apg_cpu")
    lora = _load("fusion_sampling_lora.py", "fs_lora_apg_cpu")._fs
    assert lora.LORA is True
    for mod in (fs, lora):
        p = mod.build_parser()
        d = p.parse_args([])
        assert d.apg is False and d.apg_eta == 0.0 and d.apg_norm == 0.0
        assert mod.check_solver_args(d) is None and d.apg is None                                   # off: the sampler gets no apg argument
        o = p.parse_args(["--apg", "--apg_eta", "0.25", "--apg_norm", "15", "--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--eta", "0.5",
                          "--guidance_interval", "700,250"])
        assert mod.check_solver_args(o) is None and o.apg == dict(eta=0.25, norm_threshold=15.0)
        o = p.parse_args(["--apg"])
        assert mod.check_solver_args(o) is None and o.apg == dict(eta=0.0, norm_threshold=0.0)      # no paper setting is built in
        with pytest.raises(SystemExit):
            p.parse_args(["--apg_eta", "much"])
        assert "--apg " in mod.__doc__ and "2410.02416" in mod.__doc__
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "ok.latent.pt")
    keep = ["--mask_paths", "a.png+b.png", "--reroll", "1"]

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    from tweediemix_amd import launch as LA
    monkeypatch.setattr(LA, "self_launch", no_gpu)                # ... and no rank was started
    for flags in (["--apg_eta", "0.5"], ["--apg_norm", "15"]):
        with pytest.raises(SystemExit, match=r"give --apg too"):
            fs.main(BASE + flags + ["--gpus", "2"])
    for flags in (["--apg_eta", "1.5"], ["--apg_eta", "-0.2"], ["--apg_eta", "nan"], ["--apg_norm", "-1"], ["--apg_norm", "inf"]):
        with pytest.raises(SystemExit, match=r"--apg_eta .* --apg_norm"):
            fs.main(BASE + ["--apg"] + flags + ["--gpus", "2"])
    with pytest.raises(SystemExit, match=r"--apg does not combine with --guidance_rescale 0.7"):
        fs.main(BASE + ["--apg", "--guidance_rescale", "0.7", "--gpus", "2"])
    with pytest.raises(SystemExit, match=r"--apg does not combine with --keep_latents"):
        fs.main(BASE + ["--apg", "--keep_latents", str(tmp_path / "ok.latent.pt")] + keep)
    from PIL import Image
    Image.fromarray(np.zeros((128, 128, 3), np.uint8)).save(tmp_path / "img.png")
    with pytest.raises(SystemExit, match=r"--apg does not combine with --keep_image"):
        lora.main(BASE + ["--apg", "--keep_image", str(tmp_path / "img.png")] + keep)
