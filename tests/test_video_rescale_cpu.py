"""CPU: guidance rescale of the VIDEO sampler -- the restatements of tweediemix_amd.guidance (properties of the per-video factor, the fp16
rounding points, equality with the oracle's DDIM step and with solver.vpred_multistep_reference at factor 1), the kernel's one-pass partition in numpy
against the two-pass restatement on every case of the GPU sweep, the ABI's prototypes and refusals (no launch: validation fails first), and the
refusals of sample_loop, VideoSampler and run_video.py --guidance_rescale."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import video_rescale_cases as VC
from video_rescale_cases import ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = np.float32
LOWPS = [None, np.float16, "bf16"]


def _lp(lowp):
    return None if isinstance(lowp, str) else lowp


def _v(B=2, shape=(4, 3, 5, 7), mean=0.0, sd=1.0, seed=0, lowp=None):
    rng = np.random.RandomState(seed)
    vu = mean + sd * rng.randn(B, *shape)
    v = np.concatenate([vu, vu + 0.3 * sd * rng.randn(B, *shape)]).astype(NF)
    if lowp is not None:
        v = torch.from_numpy(v).to(torch.float16 if lowp is np.float16 else torch.bfloat16).float().numpy()
    return v


# ------------------------------------------------------------------------------------------------ the factor
def test_phi_one_matches_the_conditional_standard_deviation_per_video():
    from tweediemix_amd import guidance as G
    for g in (1.0, 7.5, 9.0, 30.0):
        v = _v(3, seed=int(g))
        f = G.vpred_rescale_factors_reference(v[:3], v[3:], g, 1.0)
        vv = G.vpred_guided(v[:3], v[3:], g).astype(np.float64)
        assert f.shape == (3,) and f.dtype == NF
        for b in range(3):
            sd_c, sd_s = v[3 + b].astype(np.float64).std(ddof=1), (float(f[b]) * vv[b]).std(ddof=1)
            assert abs(sd_s - sd_c) <= 1e-6 * sd_c, (g, b)          # the only error is the fp32 rounding of f (2^-24 relative)


def test_phi_zero_is_exactly_one_and_the_factor_falls_with_g():
    from tweediemix_amd import guidance as G
    v = _v(2, mean=3.0, seed=3)
    assert np.array_equal(G.vpred_rescale_factors_reference(v[:2], v[2:], 9.0, 0.0), np.ones(2, NF))
    prev = None
    for g in (1.5, 3.0, 7.5, 9.0, 30.0):
        f = G.vpred_rescale_factors_reference(v[:2], v[2:], g, 0.7)
        assert np.all(f > 0.3 - 1e-6) and np.all(f < 1.0)
        assert prev is None or np.all(f < prev), g
        prev = f
    # per video: the factor of video 0 does not see video 1
    one = G.vpred_rescale_factors_reference(v[:1], v[2:3], 9.0, 0.7)
    assert np.array_equal(one, G.vpred_rescale_factors_reference(v[:2], v[2:], 9.0, 0.7)[:1])


def test_zero_variance_and_non_finite_rule():
    from tweediemix_amd import guidance as G
    v = np.full((2, 4, 3, 5), 0.1, NF)                                 # v_u == v_c: v' constant
    assert G.vpred_rescale_factors_reference(v[:1], v[1:], 9.0, 0.7)[0] == 1.0
    v = _v(1, shape=(4, 3, 5))
    v[1] = v[0] * NF(0.5)                                              # v' = v_u + 2 (0.5 v_u - v_u) = 0 everywhere: sd_v = 0, sd_c > 0
    assert np.all(G.vpred_guided(v[:1], v[1:], 2.0) == 0) and G.vpred_rescale_factors_reference(v[:1], v[1:], 2.0, 0.7)[0] == 1.0
    for bad in (np.inf, np.nan):
        v = _v(2, shape=(4, 3, 5))
        v[2, 0, 0, 0] = bad                                            # video 0's conditional row; video 1 keeps its factor
        f = G.vpred_rescale_factors_reference(v[:2], v[2:], 9.0, 0.7)
        assert f[0] == 1.0 and 0.3 < f[1] < 1.0
    for phi in (-0.1, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match="phi"):
            G.vpred_rescale_factors_reference(v[:2], v[2:], 9.0, phi)


def test_fp16_rounding_points():
    """with np.float16 every one of cfg's three results and the product f * v' is an fp16 value and the statistics are those of the fp16 v'; with "bf16"
    the arithmetic is fp32 throughout"""
    from tweediemix_amd import guidance as G
    h = lambda a: a.astype(np.float16).astype(NF)
    v = _v(2, seed=5, lowp=np.float16)
    g, f = 7.5, np.array([0.37, 0.81], NF)
    vv = G.vpred_guided(v[:2], v[2:], g, np.float16)
    want = h(v[:2] + h(NF(g) * h(v[2:] - v[:2])))
    assert np.array_equal(vv, want) and np.array_equal(vv, h(vv)) and not np.array_equal(vv, G.vpred_guided(v[:2], v[2:], g))
    r = G.vpred_rescaled(v, f, g, np.float16)
    assert np.array_equal(r, h(f.reshape(2, 1, 1, 1, 1) * want)) and not np.array_equal(r, (f.reshape(2, 1, 1, 1, 1) * want).astype(NF))
    a, b = G.vpred_rescale_factors_reference(v[:2], v[2:], g, 0.7, np.float16), G.vpred_rescale_factors_reference(v[:2], v[2:], g, 0.7)
    assert not np.array_equal(a, b) and np.all(ulps(a, b) < 1 << 14)
    assert np.array_equal(G.vpred_guided(v[:2], v[2:], g, "bf16"), G.vpred_guided(v[:2], v[2:], g))
    assert np.array_equal(G.vpred_rescale_factors_reference(v[:2], v[2:], g, 0.7, "bf16"), b)


# ------------------------------------------------------------------------------------------------ step restatements
@pytest.mark.parametrize("lowp", LOWPS, ids=["f32", "f16", "bf16"])
def test_restatements_at_factor_one_are_the_existing_ones(lowp):
    """factor 1: the DDIM restatement IS oracle.tweedie_oracle.video_vpred_step (for bf16: its fp32 result rounded once at the store, the convention of
    solver.vpred_multistep_reference) and the multistep restatement IS solver.vpred_multistep_reference, by equality; the two x0 agree"""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import guidance as G, solver as SV
    g, at, an = 9.0, NF(0.31), NF(0.36)
    B = 2
    v = _v(B, seed=2, lowp=lowp)
    rng = np.random.RandomState(1)
    x = _v(B, seed=7, lowp=lowp)[:B]
    prev = rng.randn(*x.shape).astype(NF)
    sa, s1, san, s1n = np.sqrt(at), np.sqrt(NF(1) - at), np.sqrt(an), np.sqrt(NF(1) - an)
    one = np.ones(B, NF)
    out, x0 = G.vpred_rescaled_step_reference(x, v, one, g, sa, s1, san, s1n, lowp)
    want = TO.video_vpred_step(x, v, g, at, an, _lp(lowp))
    if lowp == "bf16":
        want = SV._bf16_round(want)
    assert out.dtype == NF and x0.dtype == NF and np.array_equal(out, want)
    for cf in ((0.8125, 0.3217, 0.0), (0.8125, 0.4021, -0.0804)):
        got, got0 = G.vpred_rescaled_multistep_reference(x, v, prev, one, g, sa, s1, *cf, lowp)
        ref, ref0 = SV.vpred_multistep_reference(x, v, prev, g, sa, s1, *cf, lowp)
        assert np.array_equal(got, ref) and np.array_equal(got0, ref0) and np.array_equal(got0, x0)
    # a factor moves exactly its own video, in x0 AND in the move's eps term
    f = np.array([1.0, 0.5], NF)
    out_f, x0_f = G.vpred_rescaled_step_reference(x, v, f, g, sa, s1, san, s1n, lowp)
    assert np.array_equal(out_f[0], out[0]) and np.array_equal(x0_f[0], x0[0]) and not np.array_equal(out_f[1], out[1]) and not np.array_equal(x0_f[1], x0[1])
    if lowp is None:                                                   # eps = sa v'' + s1 x: with x0 given, out - sa' x0 carries the rescaled v''
        vv = G.vpred_rescaled(v, f, g)
        eps = ((sa * vv).astype(NF) + (s1 * x).astype(NF)).astype(NF)
        assert np.array_equal(out_f, ((san * x0_f).astype(NF) + (s1n * eps).astype(NF)).astype(NF))


# ------------------------------------------------------------------------------------------------ one-pass partition (the kernel's sums) vs two-pass
def test_sweep_covers_every_value_and_every_layout_shape_pair():
    cases = VC.all_cases()
    plan = VC.plan_cases()
    assert len(plan) == 40 and len(cases) == 60
    assert {(c["layout"], c["pad"], c["F"], c["hw"]) for c in plan} == {(l, p, F, hw) for l, p in VC.LAYOUTS for F, hw in VC.SHAPES}
    assert sorted({c["n"] for c in cases}) == [140, 280, 2240, 16408, 344064] and 16408 == 2 * 8192 + 24
    assert {c["mean"] for c in cases} == {0.0, 3.0, -100.0} and {c["sd"] for c in cases} == {1.0, 1e-2}
    assert {c["g"] for c in cases} == set(VC.GS) and {c["phi"] for c in cases} == set(VC.PHIS) and {c["S"] for c in cases} == {1, 3}
    assert {c["dt"] for c in cases} == {"f32", "f16", "bf16"}
    assert len({(c["mean"], c["sd"], c["g"], c["phi"]) for c in cases}) == 60


def test_one_pass_partition_sums_are_within_one_ulp_of_the_two_pass_restatement():
    """the argument for the GPU test's bound on the GPU sweep's own data: both sides hold the same fp32 v'; they differ in the order of the fp64 sums
    (32 x 256 strided slices shifted by element 0, a butterfly per wave, waves and partials in index order) and in one-pass against two-pass variance:
    a few 2^-52 n relative (n <= 344,064: under 1e-10) against half an fp32 ulp of 6e-8.  More than one ulp is a bug."""
    from test_guidance_rescale_cpu import kernel_sums_factor
    from tweediemix_amd import guidance as G
    worst, videos = 0, 0
    for case in VC.all_cases():
        vu, vc = VC.make_v(case)
        lowp = VC.lowp_of(case["dt"])
        ref = G.vpred_rescale_factors_reference(vu, vc, case["g"], case["phi"], lowp)
        vv = G.vpred_guided(vu, vc, case["g"], lowp)
        for s in range(case["S"]):
            got = kernel_sums_factor(vc[s], vv[s], case["phi"], VC.RS_P, VC.RS_THREADS)
            d = int(ulps(ref[s], got)[0])
            assert d <= 1, (case, s, ref[s], got)
            worst, videos = max(worst, d), videos + 1
    assert videos == 120
    print(f"partition vs two-pass over {videos} videos: worst {worst} ulp")


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "double*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int,
          "int64_t": C.c_int64, "float": C.c_float}
NEW = ("tmix_vpred_rescale_factors", "tmix_vpred_step_rs", "tmix_vpred_step_rs_dev", "tmix_vpred_step_ms_rs", "tmix_vpred_step_ms_rs_dev")


def _prototype(name, res="int"):
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_header_lists_the_new_symbols_and_ctypes_agrees():
    from tweediemix_amd import lib
    fac = [["const float*", "factors"]]
    dev, ms_dev = _prototype("tmix_vpred_step_dev"), _prototype("tmix_vpred_step_ms_dev")
    assert _prototype("tmix_vpred_step_rs_dev") == dev[:-1] + fac + dev[-1:]              # the parent's arguments, factors in front of the stream
    assert _prototype("tmix_vpred_step_ms_rs_dev") == ms_dev[:-1] + fac + ms_dev[-1:]
    flat = [["int64_t", "n"]]
    per = [["int", "videos"], ["int64_t", "n_per_video"]]
    for parent, child in (("tmix_vpred_step", "tmix_vpred_step_rs"), ("tmix_vpred_step_ms", "tmix_vpred_step_ms_rs")):
        p = _prototype(parent)
        k = p.index(flat[0])
        assert _prototype(child) == p[:k] + per + p[k + 1:-1] + fac + p[-1:], child          # videos, n_per_video in place of the flat n
    f = _prototype("tmix_vpred_rescale_factors")
    assert [n for _t, n in f] == ["v_u", "stride_u", "v_c", "stride_c", "dtype", "factors", "ws", "videos", "n_per_video", "params", "g_slot", "phi", "stream"]
    l = lib.load()
    for name in NEW:
        r, args = lib.SIGNATURES[name]
        assert r is C.c_int and args == [_CTYPE[t] for t, _n in _prototype(name)], name
        assert getattr(l, name).argtypes == args
    readme = open(os.path.join(ROOT, "README.md")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix.h")).read(), flags=re.S)
    count = len(re.findall(r"\btmix_\w+\s*\([^;{]*\)\s*;", src))
    assert count == len(lib.SIGNATURES) and f"{count} entry points" in readme


def test_entries_validate_before_any_launch():
    """pointers that are never dereferenced: every refusal comes back with its code and message from the host-side checks"""
    from tweediemix_amd import lib
    l = lib.load()
    p, err = 0x1000, lib.load().tmix_last_error_string
    ok = dict(vu=p, su=280, vc=p, sc=280, dt=lib.F32, fac=p, ws=p, S=2, n=280, prm=p, slot=5, phi=0.7)

    def rc(**kw):
        a = dict(ok, **kw)
        return l.tmix_vpred_rescale_factors(a["vu"], a["su"], a["vc"], a["sc"], a["dt"], a["fac"], a["ws"], a["S"], a["n"], a["prm"], a["slot"], a["phi"], None)
    for k in ("vu", "vc", "fac", "ws", "prm"):
        assert rc(**{k: None}) == lib.EINVAL and b"vpred_rescale_factors: null" in err(), k
    assert rc(dt=3) == lib.EINVAL and b"dtype" in err() and rc(dt=-1) == lib.EINVAL
    assert rc(slot=-1) == lib.EINVAL and b"g_slot" in err() and rc(slot=8) == lib.EINVAL
    for phi in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert rc(phi=phi) == lib.EINVAL and b"phi" in err(), phi
    assert rc(S=0) == lib.ESHAPE and b"videos" in err() and rc(S=65536) == lib.ESHAPE
    assert rc(n=1, su=1, sc=1) == lib.ESHAPE and b"n >= 2" in err() and rc(n=0) == lib.ESHAPE
    assert rc(su=279) == lib.ESHAPE and b"strides" in err() and rc(sc=279) == lib.ESHAPE

    S, Cc, F, hw = 2, 4, 2, 35
    clip = Cc * F * hw

    def scalar(ms, x=p, v=p, out=p, prev=p, dt=lib.F32, S=S, n=clip, fac=p):
        if ms:
            return l.tmix_vpred_step_ms_rs(x, v, out, prev, dt, S, n, 9.0, 0.6, 0.8, 0.8, 0.4, -0.08, fac, None)
        return l.tmix_vpred_step_rs(x, v, out, dt, S, n, 9.0, 0.6, 0.8, 0.7, 0.7, fac, None)

    def dev(ms, x=p, vu=p, su=clip, vc=p, sc=clip, prev=p, prm=p, shape=(S, Cc, F, hw), fac=p):
        if ms:
            return l.tmix_vpred_step_ms_rs_dev(x, vu, su, vc, sc, prev, prm, *shape, fac, None)
        return l.tmix_vpred_step_rs_dev(x, vu, su, vc, sc, prm, *shape, fac, None)
    for ms, name in ((False, b"vpred_step_rs"), (True, b"vpred_step_ms_rs")):
        assert scalar(ms, fac=None) == lib.EINVAL and name + b": null factors" in err()
        for k in ("x", "v", "out"):
            assert scalar(ms, **{k: None}) == lib.EINVAL and name + b": null pointer" in err(), k
        assert scalar(ms, dt=9) == lib.EINVAL and name + b": bad dtype" in err()
        assert scalar(ms, S=0) == lib.ESHAPE and name + b": videos=0" in err() and scalar(ms, n=0) == lib.ESHAPE
        assert dev(ms, fac=None) == lib.EINVAL and name + b"_dev: null factors" in err()
        for k in ("x", "vu", "vc", "prm"):
            assert dev(ms, **{k: None}) == lib.EINVAL and name + b"_dev: null pointer" in err(), k
        assert dev(ms, su=clip - 1) == lib.ESHAPE and name + b"_dev: clip strides" in err() and dev(ms, sc=clip - 1) == lib.ESHAPE
        for bad in ((0, Cc, F, hw), (S, 0, F, hw), (S, Cc, 0, hw), (S, Cc, F, 0)):
            assert dev(ms, shape=bad) == lib.ESHAPE, bad
    assert scalar(True, prev=None) == lib.EINVAL and b"vpred_step_ms_rs: null x0_prev" in err()
    assert dev(True, prev=None) == lib.EINVAL and b"vpred_step_ms_rs_dev: null x0_prev" in err()


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    x, v, prm, f = torch.zeros(1, 4, 2, 4, 4), torch.zeros(2, 4, 2, 4, 4), torch.zeros(8), torch.ones(1)
    with pytest.raises(lib.TmixError):
        ops.vpred_rescale_factors(v, prm, 0, 0.7)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_rs(x, v, 9.0, 0.3, 0.4, f)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_ms_rs(x, v, 9.0, 0.3, (0.8, 0.4, 0.0), torch.zeros_like(x), f)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_rs_dev(x, v[:1].reshape(2, 4, 4, 4), v[1:].reshape(2, 4, 4, 4), prm, f)


# ------------------------------------------------------------------------------------------------ the two loops and the CLI
BAD = (-0.1, 1.5, float("nan"), "0.7", None, True)


def test_both_loops_refuse_a_bad_phi_before_anything_else():
    from tweediemix_amd import video as V
    sch = V.VideoSchedule(np.linspace(0.9991, 0.0047, 1000).astype(NF), 6)

    def unet(*a):
        raise AssertionError("the network was called before the refusal")
    for bad in BAD:
        with pytest.raises(ValueError, match="guidance_rescale"):
            V.sample_loop(unet, torch.zeros(1, 4, 2, 4, 4), sch, 9.0, guidance_rescale=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            V.VideoSampler(None, sch, 9.0, guidance_rescale=bad)        # refused before the plan is looked at
    with pytest.raises(ValueError, match="solver"):
        V.VideoSampler(None, sch, 9.0, solver="euler", guidance_rescale=0.7)


def _run_video(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "run_video.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_flag_and_refusal_before_the_gpu(monkeypatch):
    rv = _run_video("rv_rescale_cpu")
    p = rv.build_parser()
    assert p.parse_args([]).guidance_rescale == 0.0 and p.parse_args(["--guidance_rescale", "0.7"]).guidance_rescale == 0.7
    assert "0.7" in [a for a in p._actions if a.dest == "guidance_rescale"][0].help and "--guidance_rescale PHI" in rv.__doc__
    assert rv.checked_rescale(p.parse_args(["--guidance_rescale", "1"])) == 1.0
    with pytest.raises(SystemExit):
        p.parse_args(["--guidance_rescale", "much"])

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream", "current_device"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    from tweediemix_amd import launch as LA
    monkeypatch.setattr(LA, "self_launch", no_gpu)                      # ... and before any rank is started
    for bad in ("1.5", "-0.2", "nan", "inf"):
        for more in ([], ["--gpus", "2", "--num_seeds", "2"], ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr"]):
            with pytest.raises(SystemExit, match=r"--guidance_rescale"):
                rv.main(["--synthetic", "--tiny", "--guidance_rescale", bad] + more)
