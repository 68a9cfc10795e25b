"""CPU: hold regions of the VIDEO sampler -- the properties of the numpy restatement (the selects on the weight, hs == 0, the stream
id), the three entries' prototypes and refusals (pointers that are never dereferenced), and every refusal of VideoSampler, sample_loop and
run_video.py before the GPU is touched and before any rank starts."""
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import video_hold_cases as VH
from video_solver_cases import standin_schedule

NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWPS = [None, np.float16, "bf16"]
NEW = ("tmix_vpred_step_hold", "tmix_vpred_step_hold_dev", "tmix_video_hold_composite")
COEF = (9.0, float(NF(0.4843)), float(NF(0.8749)), float(NF(0.53582)), float(NF(0.78125)), 0.0)         # g, sa, s1 and a DDIM move
MS = (9.0, float(NF(0.4843)), float(NF(0.8749)), float(NF(0.8125)), float(NF(0.4021)), float(NF(-0.0804)))


def _case(S, Fk, Fw, seed, shared=False):
    rng = np.random.RandomState(seed)
    x = rng.randn(S, VH.C, VH.F, VH.HH, VH.WW).astype(NF)
    v = rng.randn(2 * S, VH.C, VH.F, VH.HH, VH.WW).astype(NF)
    prev = rng.randn(*x.shape).astype(NF)
    return x, v, prev, VH.held_latent(1 if shared else S, Fk, seed + 1), VH.weight(1 if shared else S, Fw, seed + 2)


# ------------------------------------------------------------------------------------------------ the restatement's own properties
@pytest.mark.parametrize("lowp", LOWPS, ids=["f32", "f16", "bf16"])
def test_weight_zero_is_the_noise_step_and_weight_one_ignores_the_prediction(lowp):
    """w == 0 everywhere: vpred_step_reference's output and x0 bit for bit (both moves, with and without noise).  w == 1 everywhere with v all NaN:
    the output is kept -- finite, independent of x and v -- while x0 is the parent's (NaN)."""
    from tweediemix_amd import noise as NZ, solver as SV
    S = 2
    keys = VH.KEYS[:S]
    for coef, ms in ((COEF, False), (MS, True)):
        for cz in (0.0, VH.CZ):
            x, v, prev, kx, _w = _case(S, 1, 1, 5)
            if lowp is not None:
                rd = (lambda a: a.astype(np.float16).astype(NF)) if lowp is np.float16 else SV._bf16_round
                x, v = rd(x), rd(v)
            hist = prev if ms else None
            zero = np.zeros((S, 1, VH.HH, VH.WW), NF)
            got, got0 = NZ.vpred_hold_reference(x, v, hist, coef + (cz, VH.HA, VH.HS), keys, kx, zero, VH.STEP, None, lowp)
            want, want0 = NZ.vpred_step_reference(x, v, hist, coef + (cz,), keys, VH.STEP, None, lowp)
            assert np.array_equal(VH.bits(got), VH.bits(want)) and np.array_equal(VH.bits(got0), VH.bits(want0)), (ms, cz)
            one = np.ones_like(zero)
            nan = np.full_like(v, np.nan)
            with np.errstate(invalid="ignore"):
                held, held0 = NZ.vpred_hold_reference(x, nan, hist, coef + (cz, VH.HA, VH.HS), keys, kx, one, VH.STEP, None, lowp)
                other, _ = NZ.vpred_hold_reference(x + 1, v, hist, coef + (cz, VH.HA, VH.HS), keys, kx, one, VH.STEP, None, lowp)
            assert np.isfinite(held).all() and np.isnan(held0).all() and np.array_equal(VH.bits(held), VH.bits(other)), (ms, cz)
            assert np.array_equal(VH.bits(held), VH.bits(NZ.video_hold_composite_reference(x, kx, one, VH.HA, VH.HS, keys, lowp)))


def test_hs_zero_returns_the_held_latent_with_its_sign_and_calls_no_generator(monkeypatch):
    from tweediemix_amd import noise as NZ
    S = 2
    x, v, _prev, kx, _w = _case(S, VH.F, 1, 8)
    one = np.ones((S, 1, VH.HH, VH.WW), NF)
    at = (slice(None),) + VH.NEG0
    assert np.signbit(kx[at]).all() and (kx[at] == 0).all()
    monkeypatch.setattr(NZ, "normal", lambda *a, **k: (_ for _ in ()).throw(AssertionError("hs == 0 formed a noise")))
    got, _ = NZ.vpred_hold_reference(x, v, None, COEF + (0.0, 1.0, 0.0), VH.KEYS[:S], kx, one, VH.STEP)
    assert np.array_equal(VH.bits(got), VH.bits(kx))
    # with ha * kx formed instead, -0.0 + 0.0 * zh would have lost the sign: the select is what keeps it
    assert np.signbit(got[at]).all()


def test_fractions_blend_and_the_selects_are_per_element():
    """mixed weights: each element follows its own branch; a fraction is rnd(rnd(w kept) + rnd(rnd(1 - w) moved)) of the two pure results"""
    from tweediemix_amd import noise as NZ
    S = 3
    keys = VH.KEYS[:S]
    for Fk in (1, VH.F):
        for Fw in (1, VH.F):
            for shared in (False, True):
                x, v, prev, kx, w = _case(S, Fk, Fw, 11 + Fk + Fw, shared)
                p = COEF + (VH.CZ, VH.HA, VH.HS)
                got, _ = NZ.vpred_hold_reference(x, v, None, p, keys, kx, w, VH.STEP)
                moved, _ = NZ.vpred_step_reference(x, v, None, COEF + (VH.CZ,), keys, VH.STEP)
                kept, _ = NZ.vpred_hold_reference(x, v, None, p, keys, kx, np.ones_like(w), VH.STEP)
                wb = np.broadcast_to(w[:, None], x.shape)
                mix = ((wb * kept).astype(NF) + ((NF(1) - wb).astype(NF) * moved).astype(NF)).astype(NF)
                want = np.where(wb == 0, moved, np.where(wb == 1, kept, mix))
                assert np.array_equal(VH.bits(got), VH.bits(want)), (Fk, Fw, shared)
                assert (wb == 0).any() and (wb == 1).any() and ((wb > 0) & (wb < 1)).any()
                # kept is ha kx + hs zh with zh the video's own fixed noise, the same in every launch shape
                zh = VH.hold_noise(x[0].size, keys).reshape(x.shape)
                kxb = np.broadcast_to(kx, x.shape)
                assert np.array_equal(kept, ((NF(VH.HA) * kxb).astype(NF) + (NF(VH.HS) * zh).astype(NF)).astype(NF))


def test_the_held_noise_has_a_stream_of_its_own_and_no_step():
    from tweediemix_amd import noise as NZ
    assert (NZ.STREAM_IMAGE_STEP, NZ.STREAM_VIDEO_STEP, NZ.STREAM_VIDEO_HOLD) == (0, 1, 2)
    per = VH.C * VH.F * VH.HW
    zh = VH.hold_noise(per, VH.KEYS)
    idx = np.arange(per, dtype=np.uint64)
    for s, (lo, hi) in enumerate(VH.KEYS):
        assert not np.array_equal(zh[s], NZ.normal(idx, lo, hi, 0, NZ.STREAM_VIDEO_STEP))
        assert not np.array_equal(zh[s], NZ.normal(idx, lo, hi, 0, NZ.STREAM_IMAGE_STEP))
    assert not np.array_equal(zh[0], zh[1])
    # kx = 0, hs = 1, w = 1: the output IS zh, at whatever schedule step the launch carries
    x, v, _prev, _kx, _w = _case(3, 1, 1, 2)
    kx, one = np.zeros((1, VH.C, 1, VH.HH, VH.WW), NF), np.ones((1, 1, VH.HH, VH.WW), NF)
    for step in (0, 7):
        got, _ = NZ.vpred_hold_reference(x, v, None, COEF + (VH.CZ, 0.0, 1.0), VH.KEYS, kx, one, step)
        assert np.array_equal(got.reshape(3, per), zh), step


def test_restatement_refuses_what_it_cannot_read():
    from tweediemix_amd import noise as NZ
    x, v, _prev, kx, w = _case(2, 1, 1, 3)
    with pytest.raises(ValueError, match="9 coefficients"):
        NZ.vpred_hold_reference(x, v, None, COEF + (0.0,), VH.KEYS[:2], kx, w, 0)
    with pytest.raises(ValueError, match="keys for 2 videos"):
        NZ.vpred_hold_reference(x, v, None, COEF + (0.0, 1.0, 0.0), VH.KEYS[:1], kx, w, 0)
    with pytest.raises(ValueError, match="kx"):
        NZ.hold_blend_reference(x, kx[0], w, 1.0, 0.0, VH.KEYS[:2])


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "const uint32_t*": C.c_void_p, "int": C.c_int,
          "int64_t": C.c_int64, "float": C.c_float, "uint32_t": C.c_uint32}
HOLD_ARGS = [["const float*", "hold_x0"], ["int64_t", "hold_x0_video_stride"], ["int", "hold_x0_frames"], ["const float*", "hold_w"],
             ["int64_t", "hold_w_video_stride"], ["int", "hold_w_frames"]]


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_header_lists_the_three_entries_and_ctypes_agrees():
    from tweediemix_amd import lib
    noise_dev, noise = _prototype("tmix_vpred_step_noise_dev"), _prototype("tmix_vpred_step_noise")
    assert _prototype("tmix_vpred_step_hold_dev") == noise_dev[:-1] + HOLD_ARGS + noise_dev[-1:]        # the noise entry's arguments, then the hold's
    k = [n for _t, n in noise].index("videos")
    shape = [["int", "videos"], ["int", "channels"], ["int", "frames"], ["int64_t", "hw"]]
    assert _prototype("tmix_vpred_step_hold") == noise[:k] + shape + noise[k + 2:-1] + [["float", "ha"], ["float", "hs"]] + HOLD_ARGS + noise[-1:]
    assert [n for _t, n in _prototype("tmix_video_hold_composite")] == ["x", "dtype", "videos", "channels", "frames", "hw", "ha", "hs", "keys"] + \
        [n for _t, n in HOLD_ARGS] + ["stream"]
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
    """pointers that are never dereferenced: every refusal of the three entries, in all four forms, with its code and its message; the parent's
    answers come first, then the hold's in the order pointers, frame counts, strides"""
    from tweediemix_amd import lib
    l = lib.load()
    err = l.tmix_last_error_string
    f = 0x1000
    S, Cc, Fr, hw = 2, 4, 3, 8
    ok = dict(x=f, v=f, out=f, prev=None, dt=lib.F32, S=S, C=Cc, F=Fr, hw=hw, fac=None, keys=f, kx=f, sx=Cc * hw, fk=1, w=f, sw=Fr * hw, fw=Fr)

    def dense(**kw):
        a = dict(ok, **kw)
        return l.tmix_vpred_step_hold(a["x"], a["v"], a["out"], a["prev"], a["dt"], a["S"], a["C"], a["F"], a["hw"], 9.0, 0.6, 0.8, 0.7, 0.5, 0.0, 0.25,
                                      a["fac"], a["keys"], 7, 0.9, 0.4, a["kx"], a["sx"], a["fk"], a["w"], a["sw"], a["fw"], None)
    okd = dict(ok, vu=f, su=Cc * Fr * hw, vc=f, sc=Cc * Fr * hw, prm=f)

    def rows(**kw):
        a = dict(okd, **kw)
        return l.tmix_vpred_step_hold_dev(a["x"], a["vu"], a["su"], a["vc"], a["sc"], a["prm"], a["S"], a["C"], a["F"], a["hw"], a["prev"], a["fac"],
                                          a["keys"], a["kx"], a["sx"], a["fk"], a["w"], a["sw"], a["fw"], None)

    def comp(**kw):
        a = dict(ok, **kw)
        return l.tmix_video_hold_composite(a["x"], a["dt"], a["S"], a["C"], a["F"], a["hw"], 0.9, 0.4, a["keys"], a["kx"], a["sx"], a["fk"], a["w"],
                                           a["sw"], a["fw"], None)
    for forms in (dict(), dict(prev=f), dict(fac=f), dict(prev=f, fac=f)):
        calls = (dense, rows) if forms else (dense, rows, comp)
        for k in ("x", "v", "out"):
            assert dense(**forms, **{k: None}) == lib.EINVAL and b"null pointer" in err(), k
        for k in ("x", "vu", "vc", "prm"):
            assert rows(**forms, **{k: None}) == lib.EINVAL and b"null pointer" in err(), k
        assert rows(**forms, su=Cc * Fr * hw - 1) == lib.ESHAPE and b"clip stride" in err()
        for call in calls:
            assert call(**forms, keys=None) == lib.EINVAL and b"null keys" in err()
            for bad in (dict(S=0), dict(C=0), dict(F=0), dict(hw=0)):
                assert call(**forms, **bad) == lib.ESHAPE and b"videos=" in err(), bad
            for k in ("kx", "w"):
                assert call(**forms, **{k: None}) == lib.EINVAL and b"null hold_x0 / hold_w" in err(), k
            for bad in (dict(fk=0), dict(fk=2), dict(fk=Fr + 1), dict(fw=0), dict(fw=2), dict(fw=-1)):
                assert call(**forms, **bad) == lib.ESHAPE and b"hold_x0_frames=" in err(), bad
            for bad in (dict(sx=Cc * hw - 1), dict(sx=-1), dict(sx=1), dict(sw=Fr * hw - 1), dict(sw=-8), dict(fk=Fr, sx=Cc * hw)):
                assert call(**forms, **bad) == lib.ESHAPE and b"hold video strides" in err(), bad
            # the order: a null hold pointer is answered in front of a bad frame count, that in front of a bad stride, the parent's in front of all
            assert call(**forms, kx=None, fk=2, sx=1) == lib.EINVAL
            assert call(**forms, fk=2, sx=1) == lib.ESHAPE and b"hold_x0_frames=" in err()
            assert call(**forms, S=0, kx=None) == lib.ESHAPE and b"videos=0" in err()
            assert call(**forms, keys=None, kx=None) == lib.EINVAL and b"null keys" in err()
        for call in (dense, comp) if not forms else (dense,):
            assert call(**forms, dt=7) == lib.EINVAL and b"dtype" in err()
            assert call(**forms, dt=7, kx=None) == lib.EINVAL and b"dtype" in err()


def test_ops_wrappers_refuse_cpu_tensors_and_fill_the_twelve_floats():
    from tweediemix_amd import lib, ops
    x, v, keys = torch.zeros(1, 4, 2, 2, 2), torch.zeros(2, 4, 2, 2, 2), torch.zeros(1, 2, dtype=torch.int32)
    kx, w = torch.zeros(1, 4, 1, 2, 2), torch.zeros(1, 1, 2, 2)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_hold(x, v, 9.0, 0.3, (0.6, 0.7), 0.25, keys, 3, 0.4, kx, w)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_hold_dev(x, torch.zeros(2, 4, 2, 2), torch.zeros(2, 4, 2, 2), torch.zeros(12), keys, kx, w)
    with pytest.raises(lib.TmixError):
        ops.video_hold_composite(x, 0.4, keys, kx, w)
    a, aw = NF(0.2345), NF(0.2871)
    for move in ((0.6, 0.7), (0.8, 0.4, -0.1)):
        base = ops.video_step_params_noise(501, 9.0, a, move, 0.25, 3).tolist()
        p = ops.video_step_params_hold(501, 9.0, a, move, 0.25, 3, aw)
        assert p.dtype == torch.float32 and p.tolist() == base[:10] + [float(np.sqrt(aw)), float(np.sqrt(NF(1) - aw))]
        assert p.tolist()[10:] == list(ops.step_coeffs(aw, aw)[:2]) == list(ops.hold_coeffs(aw))
        last = ops.video_step_params_hold(501, 9.0, a, move, 0.25, 3, None)
        assert last.tolist() == base[:10] + [1.0, 0.0] and ops.hold_coeffs(None) == (1.0, 0.0)
    slot = torch.full((12,), -1.0)
    assert ops.video_step_params_hold(501, 9.0, a, (0.6, 0.7), 0.0, 0, aw, out=slot) is slot and slot[8:10].tolist() == [0.0, 0.0]
    with pytest.raises(AssertionError):
        ops.video_step_params_hold(501, 9.0, a, (0.6, 0.7), 0.25, 2 ** 24, aw)


# ------------------------------------------------------------------------------------------------ refusals before the GPU
GPU_ENTRIES = ("vpred_step_hold", "vpred_step_hold_dev", "video_hold_composite", "vpred_step_noise", "vpred_step_noise_dev", "vpred_step", "vpred_step_dev",
               "vpred_step_ms", "vpred_step_ms_dev", "video_step_prologue", "mask_edt", "soft_masks", "noise_keys")


def _no_gpu(monkeypatch):
    """-> the list that would receive the name of any GPU entry point that is called; torch.cuda's own doors raise"""
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
    kx, wt = torch.zeros(1, Cc, 1, h, w), torch.full((1, 1, h, w), 0.5)
    bad = [((kx, wt), None, "noise_seeds"),                                                   # also at eta = 0
           (kx, [1, 2], "a pair"),
           ((kx[0], wt), [1, 2], "x0 of shape"), ((torch.zeros(3, Cc, 1, h, w), wt), [1, 2], "x0 of shape"),
           ((torch.zeros(1, Cc + 1, 1, h, w), wt), [1, 2], "x0 of shape"), ((torch.zeros(1, Cc, 2, h, w), wt), [1, 2], "x0 of shape"),
           ((torch.zeros(1, Cc, 1, h, w + 1), wt), [1, 2], "x0 of shape"),
           ((kx, wt[0]), [1, 2], "weight of shape"), ((kx, torch.zeros(3, 1, h, w)), [1, 2], "weight of shape"),
           ((kx, torch.zeros(1, 2, h, w)), [1, 2], "weight of shape"), ((kx, torch.zeros(1, 1, h + 1, w)), [1, 2], "weight of shape"),
           ((torch.full_like(kx, float("nan")), wt), [1, 2], "not finite"), ((torch.full_like(kx, float("inf")), wt), [1, 2], "not finite"),
           ((kx, wt + 0.6), [1, 2], r"outside \[0, 1\]"), ((kx, wt - 0.6), [1, 2], r"outside \[0, 1\]"),
           ((kx, torch.full_like(wt, float("nan"))), [1, 2], r"outside \[0, 1\]"),
           ((kx, wt), [1], "1 values for 2 videos")]
    for solver in V.SOLVERS:
        for eta in (0.0, 0.5):
            for hold, seeds, msg in bad:
                if eta > 0.0 and seeds is None:
                    continue                                                                  # eta's own refusal comes first there
                with pytest.raises(ValueError, match=msg):
                    V.VideoSampler(plan, sch, 9.0, solver=solver, eta=eta, noise_seeds=seeds, hold=hold)
                with pytest.raises(ValueError, match=msg):
                    V.sample_loop(net, x, sch, 9.0, solver=solver, eta=eta, noise_seeds=seeds, hold=hold)
    assert called == []
    # what the checks hand on: host tensors, fp32, contiguous, in the entries' layouts; numpy and fp64 inputs are taken
    hx, hw_ = V._check_hold((np.zeros((S, Cc, Fr, h, w)), np.ones((1, Fr, h, w))), [1, 2], S, Cc, Fr, h, w)
    assert hx.dtype == hw_.dtype == torch.float32 and hx.shape == (S, Cc, Fr, h, w) and hw_.shape == (1, Fr, h, w) and not hx.is_cuda
    assert V._check_hold(None, None, S, Cc, Fr, h, w) is None


def test_hold_step_bookkeeping():
    """eta == 0 under a hold uploads the deterministic parent's own coefficients with cz = 0; the written state's alpha is the next entry's, None
    behind the last step; eta > 0 is _noise_step's values"""
    from tweediemix_amd import ops, video as V
    for spacing in V.SPACINGS:
        sch = standin_schedule(10, spacing)
        ts = [int(t) for t in sch.timesteps]
        ph, plain, ph_eta, plain_eta = V.SolverPhase(sch), V.SolverPhase(sch), V.SolverPhase(sch), V.SolverPhase(sch)
        for i, t in enumerate(ts):
            move, cz, k, aw = V._hold_step(sch, t, 0.0, None)
            assert move == ops.step_coeffs(sch.alpha(t), sch.next_alpha(t))[2:] and cz == 0.0 and k == i
            assert (aw is None) == (i == len(ts) - 1) and (aw is None or aw == sch.next_alpha(t))
            move, cz, k, aw2 = V._hold_step(sch, t, 0.0, ph)
            assert move == tuple(plain.coeffs(t)) and cz == 0.0 and k == i and (aw2 is None) == (aw is None)
            assert V._hold_step(sch, t, 0.5, None)[:3] == (tuple(V._noise_step(sch, t, 0.5, None)[0]),) + V._noise_step(sch, t, 0.5, None)[1:]
            m1, c1, k1, _ = V._hold_step(sch, t, 0.5, ph_eta)
            m2, c2, k2 = V._noise_step(sch, t, 0.5, plain_eta)
            assert (m1, c1, k1) == (tuple(m2), c2, k2) and c1 > 0.0


@pytest.fixture(scope="module")
def rv():
    spec = importlib.util.spec_from_file_location("rv_hold_cpu", os.path.join(ROOT, "run_video.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_hold_refusals_come_before_the_gpu(rv, monkeypatch, tmp_path):
    a, b = VH.write_masks(tmp_path, 128, 64)
    opt = rv.build_parser().parse_args([])
    assert rv.checked_hold(opt, ["one.png"]) is None
    for flag in ("--hold_masks", "--animate_masks", "--hold_feather", "--hold_dilate", "--hold_latents"):
        assert flag in rv.__doc__ and flag in rv.build_parser().format_help(), flag
    size = ["--height", "128", "--width", "64"]
    good = torch.zeros(1, 4, 16, 16, 8)
    torch.save(good, tmp_path / "good.latent.pt")
    torch.save(torch.zeros(1, 4, 16, 16, 9), tmp_path / "wide.latent.pt")
    torch.save(torch.zeros(2, 4, 16, 16, 8), tmp_path / "two.latent.pt")
    torch.save({"x": 1}, tmp_path / "dict.latent.pt")
    h = rv.checked_hold(rv.build_parser().parse_args(size + ["--hold_masks", f"{a}+{b}", "--hold_feather", "16", "--hold_dilate", "-8",
                                                             "--hold_latents", str(tmp_path / "good.latent.pt")]), ["one.png"])
    assert h["masks"] == [a, b] and h["animate"] is False and h["soft"] == (2.0, -1.0) and torch.equal(h["latents"], good)
    h = rv.checked_hold(rv.build_parser().parse_args(size + ["--animate_masks", a]), ["one.png"])
    assert h == dict(masks=[a], animate=True, soft=None, latents=None)
    called = _no_gpu(monkeypatch)
    started = []
    from tweediemix_amd import launch as LA
    monkeypatch.setattr(LA, "self_launch", lambda n: started.append(n))
    base = ["--synthetic", "--tiny"] + size
    refused = [(["--hold_masks", a, "--animate_masks", b], "give one of them"),
               (["--hold_masks", str(tmp_path / "none.png")], "no mask file"),
               (["--animate_masks", f"{a}+{tmp_path / 'none.png'}"], "no mask file"),
               (["--hold_feather", "8"], "a hold needs its region"), (["--hold_dilate", "-8"], "a hold needs its region"),
               (["--hold_latents", str(tmp_path / "good.latent.pt")], "a hold needs its region"),
               (["--hold_masks", a, "--hold_latents", str(tmp_path / "wide.latent.pt")], r"holds a latent of shape \(1, 4, 16, 16, 8\)"),
               (["--hold_masks", a, "--hold_latents", str(tmp_path / "two.latent.pt")], "holds a latent of shape"),
               (["--hold_masks", a, "--hold_latents", str(tmp_path / "dict.latent.pt")], "holds a latent of shape"),
               (["--hold_masks", a, "--hold_latents", str(tmp_path / "good.latent.pt"), "--num_frames", "8"], "holds a latent of shape"),
               (["--hold_masks", a, "--hold_latents", str(tmp_path / "none.latent.pt")], "no file"),
               (["--hold_masks", a, "--hold_feather", "-1"], "--hold_feather"), (["--hold_masks", a, "--hold_dilate", "nan"], "--hold_dilate"),
               (["--hold_masks", a, "--image_path", "one.png+two.png"], "ONE image"),
               (["--animate_masks", a, "--image_path", "one.png+two.png", "--num_seeds", "2"], "ONE image")]
    for flags, msg in refused:
        for more in ([], ["--gpus", "2"], ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_seeds", "2", "--eta", "0.5"]):
            with pytest.raises(SystemExit, match=msg):
                rv.main(base + flags + more)
    assert started == [] and called == []                       # ... before any rank starts, and no GPU entry point ran
