"""CPU: guidance rescale -- the restatements of tweediemix_amd.guidance (properties of the factor, the fp16 rounding points, equality with the oracle
and with solver.multistep_step_reference at factor 1), the one-pass partition sum the kernel uses against the two-pass restatement, phi's validator,
the ABI's prototypes and its refusals (no launch: validation fails first), the sampler's refusals and both CLIs' flag."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = np.float32
FUSION, PLAIN, RESAMPLE = 0, 1, 2


def _eps(rows, shape=(4, 16, 16), mean=0.0, sd=1.0, seed=0, dtype=None):
    rng = np.random.RandomState(seed)
    eu = rng.randn(1, *shape) * sd + mean
    e = np.concatenate([eu] + [eu + 0.3 * sd * rng.randn(1, *shape) for _ in range(rows - 1)]).astype(NF)
    return e.astype(dtype).astype(NF) if dtype is not None else e


def ulps(a, b):
    """distance of two fp32 arrays in units in the last place (same sign assumed: factors are positive)"""
    a, b = np.asarray(a, NF).reshape(-1), np.asarray(b, NF).reshape(-1)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the factor
def test_phi_one_matches_the_conditional_standard_deviation():
    from tweediemix_amd import guidance as G
    for g in (1.0, 7.5, 9.0, 30.0):
        eps = _eps(4, seed=int(g))
        f = G.rescale_factors_reference(FUSION, eps, 3, g, 1.0)
        e = G.guided_rows(eps, g).astype(np.float64)
        for r in range(3):
            sd_c, sd_s = eps[1 + r].astype(np.float64).std(ddof=1), (float(f[r]) * e[r]).std(ddof=1)
            assert abs(sd_s - sd_c) <= 1e-6 * sd_c, (g, r)         # the only error is the fp32 rounding of f (2^-24 relative)


def test_phi_zero_is_exactly_one_and_the_factor_falls_with_g():
    from tweediemix_amd import guidance as G
    eps = _eps(5, mean=3.0, seed=3)
    for mode, K in ((FUSION, 4), (PLAIN, 4), (RESAMPLE, 4)):
        assert np.array_equal(G.rescale_factors_reference(mode, eps, K, 9.0, 0.0), np.ones(4, NF))
    prev = None
    for g in (1.5, 3.0, 7.5, 9.0, 30.0):
        f = G.rescale_factors_reference(FUSION, eps, 4, g, 0.7)
        assert f.dtype == NF and np.all(f > 0.3 - 1e-6) and np.all(f < 1.0)
        assert prev is None or np.all(f < prev), g
        prev = f
    f = G.rescale_factors_reference(PLAIN, eps, 4, 9.0, 0.7)       # rows the mode does not read hold 1.0
    assert f[0] < 1.0 and np.array_equal(f[1:], np.ones(3, NF))


def test_zero_variance_and_non_finite_rule():
    from tweediemix_amd import guidance as G
    eps = np.full((2, 4, 3, 5), 0.1, NF)                              # eu == ec: e_r constant
    assert G.rescale_factors_reference(PLAIN, eps, 1, 9.0, 0.7)[0] == 1.0
    eps = _eps(2, shape=(4, 3, 5))
    eps[1] = eps[0] * NF(0.5)                                         # e = eu + 2 (0.5 eu - eu) = 0 everywhere: sd_e = 0, sd_c > 0
    assert np.all(G.guided_rows(eps, 2.0) == 0) and G.rescale_factors_reference(PLAIN, eps, 1, 2.0, 0.7)[0] == 1.0
    for bad in (np.inf, np.nan):
        eps = _eps(2, shape=(4, 3, 5))
        eps[1, 0, 0, 0] = bad
        assert G.rescale_factors_reference(PLAIN, eps, 1, 9.0, 0.7)[0] == 1.0
    with pytest.raises(ValueError, match="eps rows"):
        G.rescale_factors_reference(FUSION, _eps(3), 3, 9.0, 0.7)


def test_fp16_rounding_points():
    """with lowp every one of cfg's three results and the product f * e is an fp16 value; the statistics are those of the fp16 e_r"""
    from tweediemix_amd import guidance as G
    h = lambda a: a.astype(np.float16).astype(NF)
    eps = _eps(3, dtype=np.float16, seed=5)
    g, f = 7.5, np.array([0.37, 0.81], NF)
    e = G.guided_rows(eps, g, np.float16)
    want = h(eps[:1] + h(NF(g) * h(eps[1:] - eps[:1])))
    assert np.array_equal(e, want) and np.array_equal(e, h(e)) and not np.array_equal(e, G.guided_rows(eps, g))
    ep = G.rescaled_rows(eps, f, g, np.float16)
    assert np.array_equal(ep, h(f.reshape(2, 1, 1, 1) * want)) and np.array_equal(ep, h(ep))
    assert not np.array_equal(ep, (f.reshape(2, 1, 1, 1) * want).astype(NF))
    a, b = G.rescale_factors_reference(FUSION, eps, 2, g, 0.7, np.float16), G.rescale_factors_reference(FUSION, eps, 2, g, 0.7)
    assert not np.array_equal(a, b) and np.all(ulps(a, b) < 1 << 14)


@pytest.mark.parametrize("phi", [None, "0.7", True, -0.1, 1.0001, float("nan"), float("inf")])
def test_validator_refuses(phi):
    from tweediemix_amd import guidance as G
    with pytest.raises(ValueError, match="guidance_rescale"):
        G.validate_phi(phi)


def test_validator_accepts():
    from tweediemix_amd import guidance as G
    assert [G.validate_phi(v) for v in (0, 0.0, 0.7, 1, np.float32(0.5))] == [0.0, 0.0, 0.7, 1.0, 0.5]


# ------------------------------------------------------------------------------------------------ one-pass partition (the kernel's sums) vs two-pass
def kernel_sums_factor(ec, e, phi, P=32, T=256):
    """the kernel's arithmetic in numpy: values minus the row's element 0 in fp64, every thread of the P x T grid adds its strided elements in
    order, a butterfly over each 64 lanes, the waves of a workgroup in order, the P partials in order, then (Q - S*S/n) / (n - 1)"""
    n = ec.size
    out = []
    for v in (ec, e):
        d = v.astype(np.float64).reshape(-1) - float(v.reshape(-1)[0])
        pad = (-n) % (P * T)
        for a in (d, d * d):
            a = np.concatenate([a, np.zeros(pad)]).reshape(-1, P * T)
            acc = np.zeros(P * T)
            for row in a:
                acc = acc + row
            acc = acc.reshape(P, T // 64, 64)
            for m in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[:, :, np.arange(64) ^ m]
            w = acc[:, :, 0]
            part = w[:, 0]
            for k in range(1, T // 64):
                part = part + w[:, k]
            tot = 0.0
            for p in range(P):
                tot = tot + part[p]
            out.append(tot)
    sc, qc, se, qe = out
    vc, ve = (qc - sc * sc / n) / (n - 1.0), (qe - se * se / n) / (n - 1.0)
    if not (np.isfinite(vc) and np.isfinite(ve) and ve > 0.0):
        return NF(1.0)
    ph = float(NF(phi))
    return NF(ph * np.sqrt(max(vc, 0.0)) / np.sqrt(ve) + (1.0 - ph))


def test_one_pass_partition_sums_are_within_one_ulp_of_the_two_pass_restatement():
    """the argument for the GPU test's bound, checked on the issue's data: both sides hold the same fp32 e_r; they differ in the order of the fp64
    sums and in one-pass (shifted by the first element) against two-pass variance -- relative 1e-15 or so, against half an fp32 ulp of 6e-8"""
    from tweediemix_amd import guidance as G
    worst, cases = 0, 0
    for shape in ((4, 5, 7), (4, 16, 16), (4, 64, 64)):
        for mean in (0.0, 3.0, -100.0):
            for sd in (1.0, 1e-2):
                for g in (1.0, 7.5, 9.0, 30.0):
                    for phi in (0.25, 0.7, 1.0):
                        eps = _eps(2, shape, mean, sd, seed=cases)
                        ref = G.rescale_factors_reference(PLAIN, eps, 1, g, phi)[0]
                        got = kernel_sums_factor(eps[1], G.guided_rows(eps, g)[0], phi)
                        worst = max(worst, int(ulps(ref, got)[0]))
                        cases += 1
    assert cases == 216 and worst <= 1, worst


# ------------------------------------------------------------------------------------------------ step restatements
@pytest.mark.parametrize("lowp", [None, np.float16])
def test_restatements_at_factor_one_are_the_existing_ones(lowp):
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import guidance as G, solver as SV
    K, g, at, an = 3, 7.5, NF(0.31), NF(0.36)
    rng = np.random.RandomState(1)
    x = rng.randn(1, 4, 5, 7).astype(NF)
    eps = _eps(K + 1, (4, 5, 7), seed=2, dtype=lowp)
    masks = rng.rand(K, 1, 5, 7).astype(NF)
    sa, s1, san, s1n = np.sqrt(at), np.sqrt(NF(1) - at), np.sqrt(an), np.sqrt(NF(1) - an)
    one = np.ones(K, NF)
    for last in (False, True):
        out, x0 = G.rescaled_step_reference(FUSION, x, eps, masks, K, one, g, sa, s1, san, s1n, last, lowp)
        want, want0 = TO.fused_fusion_step(x, eps, masks, g, at, an, last, lowp)
        assert out.dtype == NF and np.array_equal(out, want) and np.array_equal(x0, want0)
        out, x0 = G.rescaled_step_reference(PLAIN, x, eps, None, K, one, g, sa, s1, san, s1n, last, lowp)
        want, want0 = TO.fused_plain_step(x, eps, g, at, an, last, lowp)
        assert np.array_equal(out, want) and np.array_equal(x0, want0)
    out, _ = G.rescaled_step_reference(RESAMPLE, x, eps, None, K, one, g, sa, s1, san, s1n, False, lowp)
    assert np.array_equal(out, TO.fused_resample_down(x, eps, K, g, at, an, lowp))
    prev = rng.randn(1, 4, 5, 7).astype(NF)
    for mode, m in ((FUSION, masks), (PLAIN, None)):
        got = G.rescaled_multistep_reference(mode, x, eps, m, prev, one, g, sa, s1, 0.8125, 0.4021, -0.0804, False, lowp)
        want = SV.multistep_step_reference(mode, x, eps, m, prev, g, sa, s1, 0.8125, 0.4021, -0.0804, False, lowp)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # and a factor moves exactly the rows it belongs to
    f = np.array([1.0, 0.5, 1.0], NF)
    _, x0 = G.rescaled_step_reference(FUSION, x, eps, masks, K, f, g, sa, s1, san, s1n, False, lowp)
    _, base = G.rescaled_step_reference(FUSION, x, eps, masks, K, one, g, sa, s1, san, s1n, False, lowp)
    only1 = np.broadcast_to(masks[1:2] != 0, x0.shape)
    assert not np.array_equal(x0, base) and np.array_equal(x0[~only1], base[~only1])


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "double*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int,
          "int64_t": C.c_int64, "float": C.c_float}


def _prototype(name, res="int"):
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_header_lists_the_new_symbols_and_ctypes_agrees():
    from tweediemix_amd import lib
    dev, ms = _prototype("tmix_fused_tweedie_step_dev"), _prototype("tmix_fused_tweedie_step_ms_dev")
    fac = [["const float*", "factors"]]
    assert _prototype("tmix_fused_tweedie_step_rs_dev") == dev[:-1] + fac + dev[-1:]        # the parent's arguments, factors behind params
    assert _prototype("tmix_fused_tweedie_step_ms_rs_dev") == ms[:-1] + fac + ms[-1:]
    f = _prototype("tmix_cfg_rescale_factors")
    assert [n for _t, n in f] == ["eps", "eps_dtype", "factors", "ws", "K", "channels", "hw", "mode", "rows", "seeds", "params", "g_slot", "phi", "stream"]
    w = _prototype("tmix_cfg_rescale_ws_doubles", "int64_t")
    assert w == [["int", "rows"], ["int", "seeds"]]
    l = lib.load()
    for name, proto, res in (("tmix_fused_tweedie_step_rs_dev", dev[:-1] + fac + dev[-1:], C.c_int), ("tmix_fused_tweedie_step_ms_rs_dev", ms[:-1] + fac + ms[-1:], C.c_int),
                             ("tmix_cfg_rescale_factors", f, C.c_int), ("tmix_cfg_rescale_ws_doubles", w, C.c_int64)):
        r, args = lib.SIGNATURES[name]
        assert r is res and args == [_CTYPE[t] for t, _n in proto], name
        assert getattr(l, name).argtypes == args
    assert l.tmix_cfg_rescale_ws_doubles(4, 2) == 2 * 3 * l.tmix_cfg_rescale_ws_doubles(2, 1) > 0
    assert [l.tmix_cfg_rescale_ws_doubles(r, s) for r, s in ((1, 1), (257, 1), (2, 0), (2, 65536))] == [0, 0, 0, 0]


def test_entries_validate_before_any_launch():
    """pointers that are never dereferenced: every refusal comes back with its code from the host-side checks"""
    from tweediemix_amd import lib
    l = lib.load()
    p = 0x1000
    err = l.tmix_last_error_string
    ok = dict(eps=p, dt=lib.F32, fac=p, ws=p, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=4, seeds=1, prm=p, slot=6, phi=0.7)

    def rc(**kw):
        a = dict(ok, **kw)
        return l.tmix_cfg_rescale_factors(a["eps"], a["dt"], a["fac"], a["ws"], a["K"], a["C"], a["hw"], a["mode"], a["rows"], a["seeds"], a["prm"],
                                          a["slot"], a["phi"], None)
    for k in ("eps", "fac", "ws", "prm"):
        assert rc(**{k: None}) == lib.EINVAL and b"null" in err(), k
    assert rc(dt=3) == lib.EINVAL and b"dtype" in err() and rc(dt=-1) == lib.EINVAL
    assert rc(mode=3) == lib.EINVAL and b"mode" in err() and rc(mode=-1) == lib.EINVAL
    assert rc(K=0) == lib.EINVAL and rc(K=0, mode=lib.STEP_RESAMPLE) == lib.EINVAL
    assert rc(C=1, hw=1) == lib.ESHAPE and b"n >= 2" in err() and rc(C=0) == lib.ESHAPE and rc(hw=0) == lib.ESHAPE
    assert rc(rows=3) == lib.ESHAPE and b"rows" in err() and rc(mode=lib.STEP_PLAIN, rows=1) == lib.ESHAPE and rc(rows=257) == lib.ESHAPE
    assert rc(mode=lib.STEP_RESAMPLE, rows=3) == lib.ESHAPE
    assert rc(seeds=0) == lib.ESHAPE and rc(seeds=65536) == lib.ESHAPE
    assert rc(slot=-1) == lib.EINVAL and b"g_slot" in err() and rc(slot=8) == lib.EINVAL
    for phi in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert rc(phi=phi) == lib.EINVAL and b"phi" in err(), phi

    sok = dict(x=p, eps=p, dt=lib.F32, masks=p, mss=0, out_x=p, out_x0=None, prev=p, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=4, seeds=1, prm=p, fac=p)

    def step(ms, **kw):
        a = dict(sok, **kw)
        head = (a["x"], a["eps"], a["dt"], a["masks"], a["mss"], a["out_x"], a["out_x0"])
        tail = (a["K"], a["C"], a["hw"], a["mode"], a["rows"], a["seeds"], a["prm"], a["fac"], None)
        if ms:
            return l.tmix_fused_tweedie_step_ms_rs_dev(*head, a["prev"], *tail)
        return l.tmix_fused_tweedie_step_rs_dev(*head, *tail)
    for ms in (False, True):
        assert step(ms, fac=None) == lib.EINVAL and b"factors" in err()
        for k in ("x", "eps", "out_x", "prm"):
            assert step(ms, **{k: None}) == lib.EINVAL and b"null" in err(), k
        assert step(ms, mode=3) == lib.EINVAL and step(ms, mode=-1) == lib.EINVAL and step(ms, dt=7) == lib.EINVAL
        assert step(ms, masks=None) == lib.EINVAL and step(ms, K=0) == lib.EINVAL
        assert step(ms, rows=3) == lib.ESHAPE and step(ms, mode=lib.STEP_PLAIN, rows=1) == lib.ESHAPE
        for bad in (dict(C=0), dict(hw=0), dict(seeds=0), dict(seeds=65536)):
            assert step(ms, **bad) == lib.ESHAPE, bad
    assert step(True, prev=None) == lib.EINVAL and b"x0_prev" in err()
    assert step(True, mode=lib.STEP_RESAMPLE) == lib.EINVAL and b"mode" in err()
    assert step(False, mode=lib.STEP_RESAMPLE, rows=3) == lib.ESHAPE


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    z, e, prm = torch.zeros(1, 4, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(8)
    with pytest.raises(lib.TmixError):
        ops.cfg_rescale_factors(e, 1, lib.STEP_PLAIN, 1, prm, 6, 0.7)
    with pytest.raises(lib.TmixError):
        ops.fused_tweedie_step_rs_dev(z, e, None, lib.STEP_PLAIN, 1, prm, torch.ones(1, 1))


# ------------------------------------------------------------------------------------------------ sampler and CLI
class NoWeights:
    device = torch.device("cpu")
    kind = "custom"


def _sampler(**kw):
    from tweediemix_amd import sampler as S
    cfg = S.make_config(n_timesteps=10, resolution_h=128, resolution_w=128, resampling_steps=2, jumping_steps=1, t_cond=0.4, t_stop=0.9, guidance_scale=9.0)
    masks = torch.ones(3, 1, 16, 16) / 3
    return S.Tweediemix(cfg, NoWeights(), None, None, lambda x0: masks, concept_num=3, **kw)


def test_sampler_default_refusals_and_buffers():
    tw = _sampler()
    assert tw.guidance_rescale == 0.0 and tw._rs_factors is None and tw._rs_ws is None
    z = torch.zeros(1, 4, 16, 16)
    tw.set_keep(z, z[:, :1], z)                                 # the default sampler takes a keep region
    for bad in (-0.1, 1.5, float("nan"), "0.7", None):
        with pytest.raises(ValueError, match="guidance_rescale"):
            _sampler(guidance_rescale=bad)
    rs = _sampler(guidance_rescale=0.7, n_seeds=2)
    assert rs.guidance_rescale == 0.7 and tuple(rs._rs_factors.shape) == (2 * 3,) and rs._rs_ws.dtype == torch.float64
    with pytest.raises(ValueError, match=r"set_keep.*guidance_rescale=0.7"):
        rs.set_keep(torch.zeros(2, 4, 16, 16), z[:, :1], torch.zeros(2, 4, 16, 16))
    assert rs._keep is None
    assert _sampler(guidance_rescale=0.7, solver="dpmpp2m", timestep_spacing="logsnr")._x0_prev is not None


def _load(script, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "fusion_generation", script))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


BASE = ["--synthetic", "--tiny", "--concepts", "a+b+bg", "--seg_concepts", "a cat+a dog", "--resolution_h", "128", "--resolution_w", "128"]


def test_both_scripts_accept_the_flag_and_refuse_before_the_gpu(tmp_path, monkeypatch):
    fs = _load("fusion_sampling.py", "fs_rescale_cpu")
    lora = _load("fusion_sampling_lora.py", "fs_lora_rescale_cpu")._fs
    assert lora.LORA is True
    for mod in (fs, lora):
        p = mod.build_parser()
        assert p.parse_args([]).guidance_rescale == 0.0 and p.parse_args(["--guidance_rescale", "0.7"]).guidance_rescale == 0.7
        assert "0.7" in [a for a in p._actions if a.dest == "guidance_rescale"][0].help
        assert mod.check_solver_args(p.parse_args(["--guidance_rescale", "0.7", "--solver", "dpmpp2m", "--timestep_spacing", "logsnr"])) is None
        with pytest.raises(SystemExit):
            p.parse_args(["--guidance_rescale", "much"])
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "ok.latent.pt")
    keep = ["--mask_paths", "a.png+b.png", "--reroll", "1"]

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    with pytest.raises(SystemExit, match=r"--guidance_rescale 0.7 does not combine with --keep_latents"):
        fs.main(BASE + ["--guidance_rescale", "0.7", "--keep_latents", str(tmp_path / "ok.latent.pt")] + keep)
    for bad in ("1.5", "-0.2", "nan"):
        with pytest.raises(SystemExit, match=r"--guidance_rescale"):
            fs.main(BASE + ["--guidance_rescale", bad])
