"""CPU: the guidance interval of the VIDEO sampler -- the numpy restatement of the unguided step against the guided restatements fed
v = [v_c, v_c], the order rule at the interval's borders, the three entries' prototypes and refusals (pointers that are never dereferenced), every
refusal of VideoSampler, sample_loop and run_video.py before the GPU is touched and before any rank starts, and the clip accounting."""
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import video_interval_cases as VI
from video_solver_cases import standin_schedule

NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tmix_video_step_prologue_cond", "tmix_vpred_step_cond", "tmix_vpred_step_cond_dev")
ONES = lambda S: np.ones(S, NF)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("g", [1.0, 9.0, -3.0])
@pytest.mark.parametrize("dt", list(VI.LOWP))
def test_restatement_equals_the_guided_restatements_fed_the_conditional_prediction_twice(dt, g):
    """cfg(v_c, v_c, g) = v_c + g * 0 is v_c for every g where v_c is not -0.0, and no factor (or a factor of 1) leaves it alone: the DDIM
    reference, the multistep reference in both orders, the noise reference and the hold reference, output and x0, by equality"""
    from tweediemix_amd import guidance as G, noise as NZ, solver as SV
    S, lowp = 2, VI.LOWP[dt]
    keys = VI.KEYS[:S]
    x, vc, prev = VI.case(S, dt, 3)
    v = np.concatenate([vc, vc])
    kx, wt = VI.hold_case(S, 5)
    same = lambda a, b: np.array_equal(VI.bits(a[0]), VI.bits(b[0])) and np.array_equal(VI.bits(a[1]), VI.bits(b[1]))
    a, b = VI.MOVES["ddim"]
    assert same(VI.reference("ddim", "plain", x, vc, prev, keys, None, lowp), G.vpred_rescaled_step_reference(x, v, ONES(S), g, VI.SA, VI.S1, a, b, lowp))
    for kind in ("first", "second"):
        got = VI.reference(kind, "plain", x, vc, prev, keys, None, lowp)
        assert same(got, SV.vpred_multistep_reference(x, v, prev, g, VI.SA, VI.S1, *VI.MOVES[kind], lowp)), kind
        assert same(got, G.vpred_rescaled_multistep_reference(x, v, prev, ONES(S), g, VI.SA, VI.S1, *VI.MOVES[kind], lowp)), kind
    for kind in VI.MOVES:
        hist = None if kind == "ddim" else prev
        coef = (g, VI.SA, VI.S1) + (VI.MOVES[kind] + (0.0,))[:3]
        for cz in (0.0, VI.CZ):
            want = NZ.vpred_step_reference(x, v, hist, coef + (cz,), keys, VI.STEP, None, lowp)
            assert same(VI.reference(kind, "noise", x, vc, prev, keys, None, lowp, cz=cz), want), (kind, cz)
            want = NZ.vpred_hold_reference(x, v, hist, coef + (cz, VI.HA, VI.HS), keys, kx, wt, VI.STEP, None, lowp)
            assert same(VI.reference(kind, "hold", x, vc, prev, keys, (kx, wt), lowp, cz=cz), want), (kind, cz)
    # the history did enter the second-order step, and the noise and the hold did change the result
    assert not np.array_equal(VI.reference("second", "plain", x, vc, prev, keys, None, lowp)[0], VI.reference("second", "plain", x, vc, prev + 1, keys, None, lowp)[0])
    plain, noisy, held = (VI.reference("ddim", p, x, vc, prev, keys, (kx, wt), lowp)[0] for p in VI.PACKS)
    assert not np.array_equal(plain, noisy) and not np.array_equal(noisy, held)


def test_a_negative_zero_prediction_keeps_its_sign():
    """x = v_c = -0.0 with sa = s1 = s1_n = 1: eps = rnd(sa v_c) + rnd(s1 x) = -0 + -0 = -0 and x0 = -0 - -0 = +0.  With sa_n = +0 the DDIM result is
    +0 + -0 = +0; with sa_n = -0 it is -0 + -0 = -0: the sign of the prediction is there.  The guided restatement fed [v_c, v_c] loses it:
    cfg(-0, -0, g) = -0 + g * +0 = +0, so eps = +0 + -0 = +0 and the result is -0 + +0 = +0"""
    from tweediemix_amd import guidance as G
    x = np.full((1, 1, 1, 1, 2), NF(-0.0))
    vc = np.full_like(x, NF(-0.0))
    out, x0 = G.vpred_cond_step_reference(x, vc, None, 1.0, 1.0, (0.0, 1.0))
    out2, _ = G.vpred_cond_step_reference(x, vc, None, 1.0, 1.0, (-0.0, 1.0))
    assert not np.signbit(x0).any() and not np.signbit(out).any() and np.signbit(out2).all()
    guided, _ = G.vpred_rescaled_step_reference(x, np.concatenate([vc, vc]), np.ones(1, NF), 9.0, 1.0, 1.0, -0.0, 1.0)
    assert not np.signbit(guided).any()


def test_restatement_refuses_what_it_cannot_read():
    from tweediemix_amd import guidance as G
    x, vc, prev = VI.case(2, "f32", 1)
    kx, wt = VI.hold_case(2, 2)
    with pytest.raises(ValueError, match="conditional prediction alone"):
        G.vpred_cond_step_reference(x, np.concatenate([vc, vc]), None, VI.SA, VI.S1, VI.DDIM)
    with pytest.raises(ValueError, match="hold without keys"):
        G.vpred_cond_step_reference(x, vc, None, VI.SA, VI.S1, VI.DDIM, hold=(kx, wt, 1.0, 0.0))
    with pytest.raises(ValueError, match="keys for 2 videos"):
        G.vpred_cond_step_reference(x, vc, None, VI.SA, VI.S1, VI.DDIM, VI.CZ, VI.KEYS[:1], 0)
    # the device floats: the g slot is not read
    for kind in VI.MOVES:
        for pack in VI.PACKS:
            hist = None if kind == "ddim" else prev
            want = VI.reference(kind, pack, x, vc, prev, VI.KEYS[:2], (kx, wt))
            for g in (9.0, float("nan")):
                got = G.vpred_cond_step_from_params(x, vc, hist, VI.params(kind, pack, g=g), None if pack == "plain" else VI.KEYS[:2],
                                                    (kx, wt) if pack == "hold" else None)
                assert np.array_equal(VI.bits(got[0]), VI.bits(want[0])) and np.array_equal(VI.bits(got[1]), VI.bits(want[1])), (kind, pack, g)


# ------------------------------------------------------------------------------------------------ the order rule
def test_a_step_at_a_border_of_the_interval_is_first_order():
    """6 steps, interval (ts[1], ts[3]): first, first, second, second, first, second; without an interval (no _at_border call, or always guided) the
    sequence is today's: first, then second"""
    from tweediemix_amd import solver as SV, video as V
    from tweediemix_amd.guidance import is_guided
    sch = standin_schedule(6, "logsnr")
    ts = [int(t) for t in sch.timesteps]
    interval = (ts[1], ts[3])
    second, guided = VI.interval_orders(ts, interval)
    assert guided == [False, True, True, True, False, False] and second == [False, False, True, True, False, True]
    want = lambda i, sec: SV.video_multistep_coeffs(ts[i], sch.alpha(ts[i - 1]) if sec else None, sch.alpha(ts[i]), sch.next_alpha(ts[i]), sec)
    ph, plain, always = V.SolverPhase(sch), V.SolverPhase(sch), V.SolverPhase(sch)
    was = True
    for i, t in enumerate(ts):
        was = V._at_border(ph, is_guided(interval, t), was)
        assert V._at_border(always, True, True) is True and V._at_border(None, False, True) is False
        got = ph.coeffs(t)
        assert got == want(i, second[i]) and (got[2] != 0.0) == second[i], i
        assert plain.coeffs(t) == always.coeffs(t) == want(i, i > 0), i
    # the stochastic coefficients follow the same bookkeeping
    ph, was = V.SolverPhase(sch), True
    for i, t in enumerate(ts):
        was = V._at_border(ph, is_guided(interval, t), was)
        assert (ph.coeffs(t, 0.5)[2] != 0.0) == second[i], i
    # an interval that starts unguided and a one-step interval
    ph, was = V.SolverPhase(sch), True
    orders = []
    for t in ts:
        was = V._at_border(ph, is_guided((ts[2], ts[2]), t), was)
        orders.append(ph.coeffs(t)[2] != 0.0)
    assert orders == [False, True, False, False, True, True]


def test_clip_accounting_of_the_issues_interval():
    """(700, 250) at n = 50 'leading' guides the 22 timesteps 681 .. 261: 28 unguided steps, 72 clips per video instead of 100"""
    from tweediemix_amd.guidance import is_guided, unguided_count, validate_interval
    sch = standin_schedule(50, "leading")
    ts = [int(t) for t in sch.timesteps]
    assert ts[0] == 981 and ts[-1] == 1 and len(ts) == 50
    iv = validate_interval("700,250")
    guided = [t for t in ts if is_guided(iv, t)]
    assert iv == VI.INTERVAL_N50 and guided == list(range(681, 260, -20)) and len(guided) == 22
    nu = unguided_count(iv, ts)
    assert nu == 28 and 2 * len(ts) - nu == 72
    assert unguided_count(None, ts) == 0 and unguided_count((1000, 0), ts) == 0 and unguided_count((0, 0), ts) == 50


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "const uint32_t*": C.c_void_p, "int": C.c_int,
          "int64_t": C.c_int64, "float": C.c_float, "uint32_t": C.c_uint32}


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_header_lists_the_three_entries_and_ctypes_agrees():
    from tweediemix_amd import lib
    names = lambda n: [a for _t, a in _prototype(n)]
    hold, hold_dev, pro = names("tmix_vpred_step_hold"), names("tmix_vpred_step_hold_dev"), names("tmix_video_step_prologue")
    drop = lambda args, gone: [a for a in args if a not in gone]
    # the guided entries' arguments without the unconditional half, g and the factors
    assert names("tmix_video_step_prologue_cond") == drop(pro, ("x_u", "clip_stride_u", "t_u"))
    assert names("tmix_vpred_step_cond") == ["x", "v_c"] + drop(hold[2:], ("g", "factors"))
    assert names("tmix_vpred_step_cond_dev") == drop(hold_dev, ("v_u", "clip_stride_u", "factors"))
    l = lib.load()
    for name in NEW:
        r, args = lib.SIGNATURES[name]
        assert r is C.c_int and args == [_CTYPE[t] for t, _n in _prototype(name)], name
        assert getattr(l, name).argtypes == args
    readme = open(os.path.join(ROOT, "README.md")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix.h")).read(), flags=re.S)
    count = len(re.findall(r"\btmix_\w+\s*\([^;{]*\)\s*;", src))
    assert count == 87 == len(lib.SIGNATURES) and "87 entry points" in readme


def test_entries_validate_before_any_launch():
    """pointers that are never dereferenced: every refusal of the three entries with its code and its message; check_vpred_step's answers first, then
    the hold's: without keys, one of the two arrays, frame counts, strides"""
    from tweediemix_amd import lib
    l = lib.load()
    err = l.tmix_last_error_string
    f = 0x1000
    S, Cc, Fr, hw, R = 2, 4, 3, 8, 8
    okp = dict(x=f, xc=f, sc=Fr * R * hw, tc=f, prm=f, S=S, C=Cc, F=Fr, hw=hw, R=R)

    def pro(**kw):
        a = dict(okp, **kw)
        return l.tmix_video_step_prologue_cond(a["x"], a["xc"], a["sc"], a["tc"], a["prm"], a["S"], a["C"], a["F"], a["hw"], a["R"], None)
    for k in ("x", "xc", "tc", "prm"):
        assert pro(**{k: None}) == lib.EINVAL and b"null pointer" in err(), k
    for bad in (dict(S=0), dict(C=0), dict(F=0), dict(hw=0), dict(R=Cc - 1)):
        assert pro(**bad) == lib.ESHAPE and b"row_channels=" in err(), bad
    assert pro(sc=Fr * R * hw - 1) == lib.ESHAPE and b"clip stride" in err()
    assert pro(x=None, S=0) == lib.EINVAL                                                     # pointers first

    ok = dict(x=f, v=f, out=f, prev=None, dt=lib.F32, S=S, C=Cc, F=Fr, hw=hw, keys=f, kx=f, sx=Cc * hw, fk=1, w=f, sw=Fr * hw, fw=Fr)

    def dense(**kw):
        a = dict(ok, **kw)
        return l.tmix_vpred_step_cond(a["x"], a["v"], a["out"], a["prev"], a["dt"], a["S"], a["C"], a["F"], a["hw"], 0.6, 0.8, 0.7, 0.5, 0.0, 0.25,
                                      a["keys"], 7, 0.9, 0.4, a["kx"], a["sx"], a["fk"], a["w"], a["sw"], a["fw"], None)
    okd = dict(ok, vc=f, sc=Cc * Fr * hw, prm=f)

    def rows(**kw):
        a = dict(okd, **kw)
        return l.tmix_vpred_step_cond_dev(a["x"], a["vc"], a["sc"], a["prm"], a["S"], a["C"], a["F"], a["hw"], a["prev"], a["keys"], a["kx"], a["sx"],
                                          a["fk"], a["w"], a["sw"], a["fw"], None)
    nohold = dict(kx=None, w=None)
    for forms in (dict(), dict(prev=f)):
        for k in ("x", "v", "out"):
            assert dense(**forms, **{k: None}) == lib.EINVAL and b"null pointer" in err(), k
        for k in ("x", "vc", "prm"):
            assert rows(**forms, **{k: None}) == lib.EINVAL and b"null pointer" in err(), k
        assert rows(**forms, sc=Cc * Fr * hw - 1) == lib.ESHAPE and b"clip stride" in err()
        assert dense(**forms, dt=7) == lib.EINVAL and b"dtype" in err()
        assert dense(**forms, dt=7, keys=None) == lib.EINVAL and b"dtype" in err()            # the parent's answers come first
        for call in (dense, rows):
            for pack in (dict(), nohold, dict(nohold, keys=None)):
                for bad in (dict(S=0), dict(C=0), dict(F=0), dict(hw=0)):
                    assert call(**forms, **pack, **bad) == lib.ESHAPE and b"videos=" in err(), bad
            assert call(**forms, keys=None) == lib.EINVAL and b"hold without keys" in err()
            assert call(**forms, keys=None, kx=None) == lib.EINVAL and b"hold without keys" in err()
            for k in ("kx", "w"):
                assert call(**forms, **{k: None}) == lib.EINVAL and b"null hold_x0 / hold_w" in err(), k
            for bad in (dict(fk=0), dict(fk=2), dict(fk=Fr + 1), dict(fw=0), dict(fw=2), dict(fw=-1)):
                assert call(**forms, **bad) == lib.ESHAPE and b"hold_x0_frames=" in err(), bad
            for bad in (dict(sx=Cc * hw - 1), dict(sx=-1), dict(sx=1), dict(sw=Fr * hw - 1), dict(sw=-8), dict(fk=Fr, sx=Cc * hw)):
                assert call(**forms, **bad) == lib.ESHAPE and b"hold video strides" in err(), bad
            assert call(**forms, kx=None, fk=2, sx=1) == lib.EINVAL                            # the order of check_hold
            assert call(**forms, S=0, kx=None) == lib.ESHAPE and b"videos=0" in err()


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    x, vc, keys = torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 2, dtype=torch.int32)
    kx, w = torch.zeros(1, 4, 1, 2, 2), torch.zeros(1, 1, 2, 2)
    rows = torch.zeros(2, 4, 2, 2)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_cond(x, vc, 0.3, (0.6, 0.7))
    with pytest.raises(lib.TmixError):
        ops.vpred_step_cond(x, vc, 0.3, (0.8, 0.4, -0.1), torch.zeros_like(x), 0.25, keys, 3, 0.4, kx, w)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_cond_dev(x, rows, torch.zeros(8))
    with pytest.raises(lib.TmixError):
        ops.video_step_prologue_cond(x, torch.zeros(2, 8, 2, 2), torch.zeros(1), torch.zeros(8))


# ------------------------------------------------------------------------------------------------ refusals before the GPU
GPU_ENTRIES = ("vpred_step_cond", "vpred_step_cond_dev", "video_step_prologue_cond", "vpred_step_hold", "vpred_step_hold_dev", "video_hold_composite",
               "vpred_step_noise", "vpred_step_noise_dev", "vpred_step", "vpred_step_dev", "vpred_step_ms", "vpred_step_ms_dev", "video_step_prologue",
               "noise_keys")
MALFORMED = ["700", "700,250,1", "250,700", "1001,0", "7.5,2", "a,b", "", "700,-1"]


def _no_gpu(monkeypatch):
    from tweediemix_amd import ops

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    called = []
    for name in GPU_ENTRIES:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: called.append(_n))
    return called


def test_sampler_and_loop_refusals_come_before_the_gpu(monkeypatch):
    from tweediemix_amd import video as V
    called = _no_gpu(monkeypatch)
    sch = standin_schedule(10, "logsnr")
    S, Cc, Fr, h, w = 2, 4, 3, 5, 7
    plan = types.SimpleNamespace(videos=S, frames=Fr, h=h, w=w, cfg=types.SimpleNamespace(in_channels=Cc))       # what is read before the refusal
    x = torch.zeros(S, Cc, Fr, h, w)
    net = lambda xin, t: (_ for _ in ()).throw(AssertionError("the network ran"))
    for solver in V.SOLVERS:
        for bad in MALFORMED + [(250, 700), (700,), (7.5, 2), (True, 0), 700]:
            with pytest.raises(ValueError, match="guidance_interval"):
                V.VideoSampler(plan, sch, 9.0, solver=solver, guidance_interval=bad)
            with pytest.raises(ValueError, match="guidance_interval"):
                V.sample_loop(net, x, sch, 9.0, solver=solver, guidance_interval=bad, unet_cond=net)
        with pytest.raises(ValueError, match="unet_cond"):                      # unguided timesteps and no network for them
            V.sample_loop(net, x, sch, 9.0, solver=solver, guidance_interval=(700, 250))
    assert called == []


@pytest.fixture(scope="module")
def rv():
    spec = importlib.util.spec_from_file_location("rv_interval_cpu", os.path.join(ROOT, "run_video.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_refusals_come_before_the_gpu(rv, monkeypatch):
    opt = rv.build_parser().parse_args([])
    assert opt.guidance_interval is None and rv.checked_interval(opt) is None
    assert rv.checked_interval(rv.build_parser().parse_args(["--guidance_interval", "700,250"])) == (700, 250)
    assert "--guidance_interval" in rv.__doc__ and "--guidance_interval" in rv.build_parser().format_help()
    called = _no_gpu(monkeypatch)
    started = []
    from tweediemix_amd import launch as LA
    monkeypatch.setattr(LA, "self_launch", lambda n: started.append(n))
    base = ["--synthetic", "--tiny", "--height", "128", "--width", "64"]
    for bad in MALFORMED:
        for more in ([], ["--gpus", "2"], ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_seeds", "2", "--eta", "0.5", "--streams", "1"]):
            with pytest.raises(SystemExit, match="--guidance_interval"):
                rv.main(base + [f"--guidance_interval={bad}"] + more)
    assert started == [] and called == []
