"""GPU: guidance rescale of the VIDEO sampler -- tmix_vpred_rescale_factors, tmix_vpred_step_rs / _ms_rs / _rs_dev / _ms_rs_dev,
sample_loop(guidance_rescale=phi), VideoSampler(guidance_rescale=phi), run_video.py --guidance_rescale.

The factors are compared with tweediemix_amd.guidance.vpred_rescale_factors_reference within ONE fp32 ulp: both sides hold the same fp32 v' and differ in
the order of the fp64 sums and in one-pass against two-pass variance (a few 2^-52 n relative, n <= 344,064; half an fp32 ulp is 6e-8;
tests/test_video_rescale_cpu.py runs the kernel's partition in numpy on the same cases).  Everything else -- the scalar step entries against the
restatements, the device forms against the scalar forms, the sampler's states against the step restated with the device's own factors -- is
compared by equality."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import video_rescale_cases as VC
from layout_frames import Frame, _wrap, dense_guarded
from test_video_solver_gpu import AT, DT, FR, G, H, N6, ORDERS, S1, SA, W, _dev_case, _host_loop, _inputs, _pipe, _sampler, _video, _weights, _x
from video_rescale_cases import ulps

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
AN = NF(0.2871)
SAN, S1N = np.sqrt(AN), np.sqrt(NF(1) - AN)
KINDS = ("ddim", "first", "second")                              # the DDIM entry, the multistep entry at a first-order and at a second-order step
RS_ENTRIES = ("tmix_vpred_rescale_factors", "tmix_vpred_step_rs", "tmix_vpred_step_rs_dev", "tmix_vpred_step_ms_rs", "tmix_vpred_step_ms_rs_dev")
ENTRIES = ("tmix_vpred_step", "tmix_vpred_step_dev", "tmix_vpred_step_ms", "tmix_vpred_step_ms_dev", "tmix_video_step_prologue") + RS_ENTRIES


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from tweediemix_amd import lib as L
    return L, L.load()


def _dtc(dt):
    L, _ = _lib()
    return {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[dt]


def _prm_g(g, slot):
    v = [0.0] * 8
    v[slot] = g
    return torch.tensor(v, dtype=F32).cuda()


def _nan_ws(S):
    _, lib = _lib()
    return torch.full((lib.tmix_cfg_rescale_ws_doubles(2, S),), float("nan"), dtype=torch.float64, device="cuda")       # nothing needs zeroing


def _factors(vu, su, vc, sc, dt, S, n, g, phi, slot=5, fac=None, ws=None, prm=None):
    """raw ABI call -> (code, factors [S])"""
    _, lib = _lib()
    prm = _prm_g(g, slot) if prm is None else prm
    fac = torch.full((S,), float("nan"), dtype=F32, device="cuda") if fac is None else fac
    ws = _nan_ws(S) if ws is None else ws
    rc = lib.tmix_vpred_rescale_factors(_p(vu), su, _p(vc), sc, _dtc(dt), _p(fac), _p(ws), S, n, _p(prm), slot, phi, _st())
    torch.cuda.synchronize()
    return rc, fac


def _plan_rows(case, vu, vc):
    """the case's (v_u, v_c) [S, n] as plan prediction rows in sealed frames whose padding holds NaN -> (frames, (v_u, stride, v_c, stride))"""
    S, F, hw, n = case["S"], case["F"], case["hw"], case["n"]
    stride = n + (24 if case["pad"] else 0)
    rows = lambda a: torch.from_numpy(a).cuda().reshape(-1, F * VC.C, hw)
    if case["layout"] == "two":
        fu = Frame.of(rows(vu), batch_stride=stride, name="v_u").seal()
        fc = Frame.of(rows(vc), batch_stride=stride, name="v_c").seal()
        return (fu, fc), (fu.view, stride, fc.view, stride)
    f = Frame.of(torch.cat([rows(vu), rows(vc)]), batch_stride=stride, name="v").seal()
    return (f,), (f.view[:S], stride, f.view[S:], stride)


def _ref(case, vu, vc):
    from tweediemix_amd import guidance as GD
    return GD.vpred_rescale_factors_reference(vu, vc, case["g"], case["phi"], VC.lowp_of(case["dt"]))


# ------------------------------------------------------------------------------------------------ factors == restatement (one ulp)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: f"F{s[0]}hw{s[1]}")
def test_factors_on_plan_rows_equal_the_restatement_to_one_ulp(shape):
    """F32: (two half buffers | one buffer of 2S clips) x (dense | padded clip stride, NaN in the padding) x S in {1, 3}, data / g / phi walking the 72
    combinations, g read from slot 5 or 6; the inputs and their padding stay as they were and no NaN reaches a factor"""
    worst = 0
    for k, case in enumerate(c for c in VC.plan_cases() if (c["F"], c["hw"]) == shape):
        vu, vc = VC.make_v(case)
        frames, (tu, su, tc, sc) = _plan_rows(case, vu, vc)
        rc, fac = _factors(tu, su, tc, sc, "f32", case["S"], case["n"], case["g"], case["phi"], slot=5 + (k & 1))
        assert rc == 0, case
        for f in frames:
            f.assert_unchanged()
        got, ref = fac.cpu().numpy(), _ref(case, vu, vc)
        assert np.isfinite(got).all() and got.shape == ref.shape, (case, got)
        d = ulps(got, ref)
        assert d.max() <= 1, (case, got, ref)
        worst = max(worst, int(d.max()))
    print(f"plan-row factors F, hw = {shape}: worst {worst} ulp")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_factors_on_the_scalar_layout_equal_the_restatement_to_one_ulp(dt):
    """v [2][B][n] of the model dtype, v_c = v + B n, both strides n (what sample_loop hands over), through the raw entry and through the ops wrapper"""
    from tweediemix_amd import ops
    worst = 0
    for case in (c for c in VC.scalar_cases() if c["dt"] == dt):
        vu, vc = VC.make_v(case)
        B, n = case["S"], case["n"]
        v = torch.from_numpy(np.stack([vu, vc])).to(TDT[dt]).cuda().contiguous()
        rc, fac = _factors(v, n, v[1], n, dt, B, n, case["g"], case["phi"], slot=0)
        got, ref = fac.cpu().numpy(), _ref(case, vu, vc)
        assert rc == 0 and np.isfinite(got).all(), case
        d = ulps(got, ref)
        assert d.max() <= 1, (case, got, ref)
        worst = max(worst, int(d.max()))
        w = ops.vpred_rescale_factors(v.view(2 * B, VC.C, case["F"], case["hw"]), _prm_g(case["g"], 3), 3, case["phi"])
        torch.cuda.synchronize()
        assert torch.equal(w, fac), case
    print(f"scalar-layout factors {dt}: worst {worst} ulp")


def test_constant_guided_prediction_gives_one():
    """v_u == v_c (any constant, also one whose square is not exact in fp64 sums): v' is constant, sd_v = 0, the factor is 1.0; a non-finite element too,
    and it costs only its own video its factor"""
    for dt in TDT:
        for c in (0.1, 3.0, -100.3):
            v = torch.full((2, 2, 2240), c, dtype=TDT[dt], device="cuda")
            rc, fac = _factors(v, 2240, v[1], 2240, dt, 2, 2240, 9.0, 0.7)
            assert rc == 0 and torch.equal(fac, torch.ones_like(fac)), (dt, c, fac)
    v = torch.randn(2, 3, 2240, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    v[1, 0, 17] = float("inf")
    v[0, 2, 2239] = float("nan")
    rc, fac = _factors(v, 2240, v[1], 2240, "f32", 3, 2240, 9.0, 0.7)
    assert rc == 0 and fac[0] == 1.0 and fac[2] == 1.0 and 0.3 < float(fac[1]) < 1.0, fac


def test_two_launches_give_identical_bits_and_co_batched_videos_equal_single_ones():
    """the partition per video does not depend on the number of videos: S = 3 gives the three S = 1 factors, by equality, on dense and on padded rows"""
    for case in (c for c in VC.plan_cases() if c["S"] == 3 and c["n"] in (280, 16408, 344064)):
        vu, vc = VC.make_v(case)
        _frames, (tu, su, tc, sc) = _plan_rows(case, vu, vc)
        a = _factors(tu, su, tc, sc, "f32", 3, case["n"], case["g"], case["phi"])[1]
        b = _factors(tu, su, tc, sc, "f32", 3, case["n"], case["g"], case["phi"])[1]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), case
        for s in range(3):
            one = _factors(tu[s:], su, tc[s:], sc, "f32", 1, case["n"], case["g"], case["phi"])[1]
            assert torch.equal(one, a[s:s + 1]), (case, s)


def test_factors_guard_bands_and_untouched_inputs():
    _, lib = _lib()
    case = dict(VC.plan_cases()[0], S=3, F=2, hw=2051, n=16408, layout="one", pad=True, seed=77)
    vu, vc = VC.make_v(case)
    frames, (tu, su, tc, sc) = _plan_rows(case, vu, vc)
    want = _factors(tu, su, tc, sc, "f32", 3, case["n"], 7.5, 0.7, slot=6)[1]
    nd = lib.tmix_cfg_rescale_ws_doubles(2, 3)
    assert nd == 3 * VC.RS_P * 4
    prm = Frame.of(torch.tensor([[0, 0, 0, 0, 0, 0, 7.5, 0]], dtype=F32, device="cuda"), name="params").seal()
    fac = dense_guarded((1, 3), F32, rows=8, device="cuda", name="factors")
    ws = dense_guarded((1, nd), torch.int64, rows=1, device="cuda", name="ws")           # the doubles' bits
    rc, _ = _factors(tu, su, tc, sc, "f32", 3, case["n"], 7.5, 0.7, slot=6, fac=fac.view, ws=ws.view, prm=prm.view)
    assert rc == 0
    for f in (fac, ws):
        f.assert_untouched()
        f.assert_all_written()
    for f in frames:
        f.assert_unchanged()
    prm.assert_unchanged()
    assert torch.equal(fac.view.reshape(-1), want)


# ------------------------------------------------------------------------------------------------ scalar rs forms == restatements
def _scalar_rs(kind, x, v, out, prev, dt, fac, S, n, g=G):
    """raw ABI call of tmix_vpred_step_rs (kind "ddim") or tmix_vpred_step_ms_rs -> the code"""
    _, lib = _lib()
    d = _dtc(dt) if isinstance(dt, str) else dt
    if kind == "ddim":
        return lib.tmix_vpred_step_rs(_p(x), _p(v), _p(out), d, S, n, float(g), float(SA), float(S1), float(SAN), float(S1N), _p(fac), _st())
    return lib.tmix_vpred_step_ms_rs(_p(x), _p(v), _p(out), _p(prev), d, S, n, float(g), float(SA), float(S1), *ORDERS[kind], _p(fac), _st())


def _scalar_parent(kind, x, v, out, prev, dt, g=G):
    _, lib = _lib()
    if kind == "ddim":
        return lib.tmix_vpred_step(_p(x), _p(v), _p(out), _dtc(dt), x.numel(), float(g), float(SA), float(S1), float(SAN), float(S1N), _st())
    return lib.tmix_vpred_step_ms(_p(x), _p(v), _p(out), _p(prev), _dtc(dt), x.numel(), float(g), float(SA), float(S1), *ORDERS[kind], _st())


def _restated(kind, x, v, prev, fac, lowp, g=G):
    """x [B, n], v [2B, n], prev [B, n], fac [B] numpy -> (out, x0)"""
    from tweediemix_amd import guidance as GD
    if kind == "ddim":
        return GD.vpred_rescaled_step_reference(x, v, fac, g, SA, S1, SAN, S1N, lowp)
    return GD.vpred_rescaled_multistep_reference(x, v, prev, fac, g, SA, S1, *ORDERS[kind], lowp)


def _videos(B, n, dt, seed):
    """-> x [B, n], v [2B, n] of the dtype, prev [B, n] fp32, fac [B] in (0.3, 1)"""
    tdt = TDT[dt]
    rng = np.random.RandomState(seed)
    x = torch.from_numpy(rng.randn(B, n).astype(NF)).to(tdt).cuda()
    v = torch.from_numpy(rng.randn(2 * B, n).astype(NF)).to(tdt).cuda()
    prev = torch.from_numpy(rng.randn(B, n).astype(NF)).cuda()
    fac = torch.from_numpy((0.3 + 0.7 * rng.rand(B)).astype(NF)).cuda()
    return x, v, prev, fac


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 4099])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", list(TDT))
def test_scalar_rs_forms_equal_the_restatements(dt, kind, n, B):
    """per-video n = 1, 255 (under one workgroup), 4099 (a ragged last workgroup; with B = 3 a video boundary inside a workgroup): the output and the
    history by equality; every video used its own factor"""
    x, v, prev, fac = _videos(B, n, dt, 10 * n + B + len(kind))
    out, hist = torch.empty_like(x), prev.clone()
    assert _scalar_rs(kind, x, v, out, hist, dt, fac, B, n) == 0
    torch.cuda.synchronize()
    want, want0 = _restated(kind, x.float().cpu().numpy(), v.float().cpu().numpy(), prev.cpu().numpy(), fac.cpu().numpy(), DT[dt][1])
    assert np.array_equal(out.float().cpu().numpy(), want), (dt, kind, n, B)
    if kind != "ddim":
        assert np.array_equal(hist.cpu().numpy(), want0), (dt, kind, n, B)
    if n > 1:                                                    # ... and the factors did enter
        base, _ = _restated(kind, x.float().cpu().numpy(), v.float().cpu().numpy(), prev.cpu().numpy(), np.ones(B, NF), DT[dt][1])
        assert all(not np.array_equal(base[b], want[b]) for b in range(B))


def test_scalar_rs_ops_wrappers_and_guard_bands():
    from tweediemix_amd import ops
    for dt in TDT:
        B, n = 3, 4 * 2 * 35
        x, v, prev, fac = _videos(B, n, dt, 41)
        x5, v5 = x.view(B, 4, 2, 5, 7), v.view(2 * B, 4, 2, 5, 7)
        lowp = DT[dt][1]
        xn, vn, pn, fn = x.float().cpu().numpy(), v.float().cpu().numpy(), prev.cpu().numpy(), fac.cpu().numpy()
        from tweediemix_amd import guidance as GD
        out = ops.vpred_step_rs(x5, v5, G, AT, AN, fac)
        hist = prev.clone().view_as(x5)
        out_ms = ops.vpred_step_ms_rs(x5, v5, G, AT, ORDERS["second"], hist, fac)
        torch.cuda.synchronize()
        assert out.dtype == x.dtype and out.shape == x5.shape
        assert np.array_equal(out.float().cpu().numpy().reshape(B, n), GD.vpred_rescaled_step_reference(xn, vn, fn, G, SA, S1, SAN, S1N, lowp)[0])
        want, want0 = GD.vpred_rescaled_multistep_reference(xn, vn, pn, fn, G, SA, S1, *ORDERS["second"], lowp)
        assert np.array_equal(out_ms.float().cpu().numpy().reshape(B, n), want) and np.array_equal(hist.cpu().numpy().reshape(B, n), want0)
        for kind, ref in (("ddim", out), ("second", out_ms)):      # frames: in place on x, nothing outside, inputs unchanged
            xin, vin = Frame.of(x.reshape(1, -1), name="x"), Frame.of(v.reshape(1, -1), name="v").seal()
            hf, ff = Frame.of(prev.reshape(1, -1), name="x0_prev"), Frame.of(fac.reshape(1, -1), name="factors").seal()
            if kind == "ddim":
                hf.seal()
            assert _scalar_rs(kind, xin.view, vin.view, xin.view, hf.view, dt, ff.view, B, n) == 0
            torch.cuda.synchronize()
            xin.assert_untouched()
            vin.assert_unchanged()
            ff.assert_unchanged()
            hf.assert_unchanged() if kind == "ddim" else hf.assert_untouched()
            assert torch.equal(xin.view.reshape(ref.shape), ref), (dt, kind)


@pytest.mark.parametrize("dt", list(TDT))
def test_factors_of_one_give_the_parent_entries_bit_for_bit(dt):
    """all four: the scalar forms here, the device forms against tmix_vpred_step_dev / _ms_dev"""
    _, lib = _lib()
    B, n = 3, 4099
    x, v, prev, _ = _videos(B, n, dt, 51)
    one = torch.ones(B, device="cuda")
    for kind in KINDS:
        a, ha, b, hb = torch.empty_like(x), prev.clone(), torch.empty_like(x), prev.clone()
        assert _scalar_rs(kind, x, v, a, ha, dt, one, B, n) == 0 and _scalar_parent(kind, x, v, b, hb, dt) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ha, hb), (dt, kind)
    if dt != "f32":
        return
    S, C, F, hw = 3, 4, 2, 2051
    for layout, pad in VC.LAYOUTS:
        xd, pv, _frames, (vu, su, vc, sc), _ = _dev_case(S, F, hw, layout, pad, 52)
        for kind in KINDS:
            a, ha, b, hb = xd.clone(), pv.clone(), xd.clone(), pv.clone()
            if kind == "ddim":
                prm = _ddim_prm()
                assert lib.tmix_vpred_step_rs_dev(_p(a), _p(vu), su, _p(vc), sc, _p(prm), S, C, F, hw, _p(one), _st()) == 0
                assert lib.tmix_vpred_step_dev(_p(b), _p(vu), su, _p(vc), sc, _p(prm), S, C, F, hw, _st()) == 0
            else:
                prm = _ms_prm(kind)
                assert lib.tmix_vpred_step_ms_rs_dev(_p(a), _p(vu), su, _p(vc), sc, _p(ha), _p(prm), S, C, F, hw, _p(one), _st()) == 0
                assert lib.tmix_vpred_step_ms_dev(_p(b), _p(vu), su, _p(vc), sc, _p(hb), _p(prm), S, C, F, hw, _st()) == 0
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(ha, hb) and torch.isfinite(a).all(), (layout, pad, kind)


# ------------------------------------------------------------------------------------------------ device rs forms == scalar rs forms per video
def _ddim_prm(san=SAN, s1n=S1N, t=501.0):
    return torch.tensor([t, SA, S1, san, s1n, G, 0.0, 0.0], dtype=F32).cuda()


def _ms_prm(kind, t=501.0):
    return torch.tensor([t, SA, S1, *ORDERS[kind], G, 0.0], dtype=F32).cuda()


def _dev_rs(kind, x, ptrs, prev, prm, fac, S, C, F, hw):
    _, lib = _lib()
    vu, su, vc, sc = ptrs
    if kind == "ddim":
        return lib.tmix_vpred_step_rs_dev(_p(x), _p(vu), su, _p(vc), sc, _p(prm), S, C, F, hw, _p(fac), _st())
    return lib.tmix_vpred_step_ms_rs_dev(_p(x), _p(vu), su, _p(vc), sc, _p(prev), _p(prm), S, C, F, hw, _p(fac), _st())


def _scalar_rs_per_video(kind, x, eu, ec, prev, fac, S, C, F, hw):
    outs, hists = [], []
    for s in range(S):
        v = torch.stack([_pipe(eu, S, F, C, hw)[s], _pipe(ec, S, F, C, hw)[s]]).contiguous()
        xs, hs = x[s:s + 1].contiguous(), prev[s:s + 1].clone()
        out = torch.empty_like(xs)
        assert _scalar_rs(kind, xs, v, out, hs, "f32", fac[s:s + 1].contiguous(), 1, C * F * hw) == 0
        outs.append(out)
        hists.append(hs)
    return torch.cat(outs), torch.cat(hists)


@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: f"F{s[0]}hw{s[1]}")
@pytest.mark.parametrize("S", [1, 3])
def test_device_rs_forms_equal_the_scalar_rs_forms_per_video(S, shape):
    """every layout (two half buffers | one buffer with the text half at clip `videos`) x (clip stride = a clip | larger, NaN in the padding), the three
    kinds walking over them at the large shapes: state and history equal the scalar rs form's per video; state and history sit in guard-band frames;
    the prediction rows, their padding, the parameters and the factors stay untouched"""
    F, hw = shape
    C = 4
    small = C * F * hw <= 2240
    for i, (layout, pad) in enumerate(VC.LAYOUTS):
        for kind in (KINDS if small else [KINDS[(i + S) % 3]]):
            x, prev, frames, ptrs, (eu, ec) = _dev_case(S, F, hw, layout, pad, 200 * S + F + hw + i)
            fac = torch.from_numpy((0.3 + 0.7 * np.random.RandomState(i + S).rand(S)).astype(NF)).cuda()
            want, want_h = _scalar_rs_per_video(kind, x, eu, ec, prev, fac, S, C, F, hw)
            xf = dense_guarded((S * C * F, hw), F32, rows=8, device="cuda", name="x")
            xf.view.copy_(x.reshape(S * C * F, hw))
            hf = Frame.of(prev.reshape(S * C * F, hw), name="x0_prev")
            ff = Frame.of(fac.reshape(1, S), name="factors").seal()
            prm = Frame.of((_ddim_prm() if kind == "ddim" else _ms_prm(kind)).reshape(1, 8), name="params").seal()
            if kind == "ddim":
                hf.seal()
            assert _dev_rs(kind, xf.view, ptrs, hf.view, prm.view, ff.view, S, C, F, hw) == 0
            torch.cuda.synchronize()
            xf.assert_untouched()
            xf.assert_all_written()
            hf.assert_unchanged() if kind == "ddim" else hf.assert_untouched()
            for f in frames + (ff, prm):
                f.assert_unchanged()
            what = (S, F, hw, layout, pad, kind)
            assert torch.isfinite(xf.view).all(), what
            assert torch.equal(xf.view.reshape(x.shape), want), what
            if kind != "ddim":
                assert torch.equal(hf.view.reshape(x.shape), want_h), what


def test_second_pass_of_the_grid_stride_loop_and_the_ops_wrapper():
    """1 x 4 x 16 x 16385 = 1,048,640 elements > 4096 workgroups x 256 threads: threads of the capped grid take a second element, in all four rs forms;
    the scalar form is tied to the restatement at this size too"""
    from tweediemix_amd import ops
    S, C, F, hw = 1, 4, 16, 16385
    assert 4096 * 256 < S * C * F * hw < 4096 * 256 + 256
    x, prev, _frames, (vu, su, vc, sc), (eu, ec) = _dev_case(S, F, hw, "two", False, 9)
    fac = torch.tensor([0.6180339], device="cuda")
    v = torch.stack([_pipe(eu, S, F, C, hw)[0], _pipe(ec, S, F, C, hw)[0]]).contiguous()
    for kind in ("ddim", "second"):
        want, want_h = _scalar_rs_per_video(kind, x, eu, ec, prev, fac, S, C, F, hw)
        ref, ref_h = _restated(kind, x.reshape(1, -1).cpu().numpy(), v.reshape(2, -1).cpu().numpy(), prev.reshape(1, -1).cpu().numpy(), fac.cpu().numpy(), None)
        assert np.array_equal(want.reshape(1, -1).cpu().numpy(), ref)
        x5, h5 = x.clone().view(S, C, F, 1, hw), prev.clone().view(S, C, F, 1, hw)
        prm = _ddim_prm() if kind == "ddim" else _ms_prm(kind)
        got = ops.vpred_step_rs_dev(x5, eu.view(S * F, C, 1, hw), ec.view(S * F, C, 1, hw), prm, fac, x0_prev=None if kind == "ddim" else h5)
        torch.cuda.synchronize()
        assert got is x5 and torch.equal(x5.reshape(x.shape), want)
        if kind != "ddim":
            assert np.array_equal(want_h.reshape(1, -1).cpu().numpy(), ref_h) and torch.equal(h5.reshape(x.shape), want_h)


def test_multistep_rs_history_is_the_ddim_rs_entrys_x0():
    """tmix_vpred_step_rs_dev with sa_next = 1, s1_next = 0 writes 1 * x0 + 0 * eps = its x0: the multistep rs entry's history holds the same bits, and
    they are not the x0 of the entries without the rescale"""
    S, C, F, hw = 3, 4, 2, 35
    x, prev, _frames, ptrs, _ = _dev_case(S, F, hw, "two", True, 7)
    fac = torch.tensor([0.41, 1.0, 0.77], device="cuda")
    d = x.clone()
    assert _dev_rs("ddim", d, ptrs, None, _ddim_prm(1.0, 0.0), fac, S, C, F, hw) == 0
    h = prev.clone()
    assert _dev_rs("second", x.clone(), ptrs, h, _ms_prm("second"), fac, S, C, F, hw) == 0
    base = x.clone()
    assert _dev_rs("ddim", base, ptrs, None, _ddim_prm(1.0, 0.0), torch.ones(S, device="cuda"), S, C, F, hw) == 0
    torch.cuda.synchronize()
    assert torch.equal(h, d) and torch.isfinite(d).all()
    assert torch.equal(d[1], base[1]) and not torch.equal(d[0], base[0]) and not torch.equal(d[2], base[2])


def test_error_codes_without_a_launch():
    """all five entries: every refusal comes back before a launch -- the outputs still hold the sentinel everywhere"""
    L, lib = _lib()
    S, C, F, hw = 2, 4, 2, 35
    clip = C * F * hw
    n = S * clip
    x = dense_guarded((1, n), F32, rows=8, device="cuda", name="x")
    out = dense_guarded((1, n), F32, rows=8, device="cuda", name="out")
    prev = dense_guarded((1, n), F32, rows=8, device="cuda", name="x0_prev")
    fac = dense_guarded((1, S), F32, rows=8, device="cuda", name="factors")
    ws = dense_guarded((1, lib.tmix_cfg_rescale_ws_doubles(2, S)), torch.int64, rows=1, device="cuda", name="ws")
    v = torch.zeros(2, n, device="cuda")
    err = lib.tmix_last_error_string
    halves = (v[0], clip, v[1], clip)
    for prm, slot, phi, S_, n_, su, code, word in ((None, 5, 0.7, S, clip, clip, L.EINVAL, b"null"), (v, 8, 0.7, S, clip, clip, L.EINVAL, b"g_slot"),
                                                  (v, 5, 1.5, S, clip, clip, L.EINVAL, b"phi"), (v, 5, 0.7, 0, clip, clip, L.ESHAPE, b"videos"),
                                                  (v, 5, 0.7, S, 1, clip, L.ESHAPE, b"n >= 2"), (v, 5, 0.7, S, clip, clip - 1, L.ESHAPE, b"strides")):
        rc = lib.tmix_vpred_rescale_factors(_p(v[0]), su, _p(v[1]), clip, L.F32, _p(fac.view), _p(ws.view), S_, n_, _p(prm), slot, phi, _st())
        assert rc == code and word in err(), (word, rc, err())
    assert lib.tmix_vpred_rescale_factors(_p(v[0]), clip, _p(v[1]), clip, 7, _p(fac.view), _p(ws.view), S, clip, _p(v), 5, 0.7, _st()) == L.EINVAL
    assert lib.tmix_vpred_rescale_factors(_p(v[0]), clip, _p(v[1]), clip, L.F32, None, _p(ws.view), S, clip, _p(v), 5, 0.7, _st()) == L.EINVAL
    one = torch.ones(S, device="cuda")
    for kind in ("ddim", "second"):
        assert _scalar_rs(kind, x.view, v, out.view, prev.view, "f32", None, S, clip) == L.EINVAL and b"null factors" in err()
        assert _scalar_rs(kind, x.view, None, out.view, prev.view, "f32", one, S, clip) == L.EINVAL
        assert _scalar_rs(kind, x.view, v, out.view, prev.view, 9, one, S, clip) == L.EINVAL and b"dtype" in err()
        assert _scalar_rs(kind, x.view, v, out.view, prev.view, "f32", one, 0, clip) == L.ESHAPE
        assert _scalar_rs(kind, x.view, v, out.view, prev.view, "f32", one, S, 0) == L.ESHAPE
        prm = _ddim_prm() if kind == "ddim" else _ms_prm(kind)
        assert _dev_rs(kind, x.view, halves, prev.view, prm, None, S, C, F, hw) == L.EINVAL and b"null factors" in err()
        assert _dev_rs(kind, x.view, (None, clip, v[1], clip), prev.view, prm, one, S, C, F, hw) == L.EINVAL
        assert _dev_rs(kind, x.view, halves, prev.view, None, one, S, C, F, hw) == L.EINVAL
        assert _dev_rs(kind, x.view, (v[0], clip - 1, v[1], clip), prev.view, prm, one, S, C, F, hw) == L.ESHAPE and b"clip stride" in err()
        assert _dev_rs(kind, x.view, (v[0], clip, v[1], clip - 1), prev.view, prm, one, S, C, F, hw) == L.ESHAPE
        for bad in ((0, C, F, hw), (S, 0, F, hw), (S, C, 0, hw), (S, C, F, 0)):
            assert _dev_rs(kind, x.view, halves, prev.view, prm, one, *bad) == L.ESHAPE, bad
    assert _scalar_rs("second", x.view, v, out.view, None, "f32", one, S, clip) == L.EINVAL and b"x0_prev" in err()
    assert _dev_rs("second", x.view, halves, None, _ms_prm("second"), one, S, C, F, hw) == L.EINVAL and b"x0_prev" in err()
    torch.cuda.synchronize()
    for f in (x, out, prev, fac, ws):                             # nothing was launched: every buffer still holds the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ the sampler on the tiny network
PHI = 0.7


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step entry that is called"""
    _, lib = _lib()
    calls = []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("streams", [2, 1])
def test_sampler_every_step_equals_the_restatement_and_graph_equals_eager(streams, solver):
    """n = 6 on the log-SNR grid at g = 9, phi = 0.7: after EVERY step the device factor is within one ulp of the restatement on the plan's own
    prediction rows and the state (and history) equals the step restated with the device's factor; graph replay equals eager, one graph per
    (inject, ["ms",] "rs")"""
    from tweediemix_amd import guidance as GD
    ms = solver != "ddim"
    Wt, vids = _weights(), [_video(3)]
    smp = _sampler(Wt, vids, streams, graphs=False, solver=solver, guidance_rescale=PHI)
    assert smp.guidance_rescale == PHI and smp.rs_factors.shape == (1,) and smp.rs_factors.dtype == F32 and smp._rs_ws.dtype == torch.float64
    rec, real = [], smp._enqueue

    def spy():
        before, hist = smp.state.clone(), (smp.x0_prev.clone() if ms else None)
        real()
        torch.cuda.synchronize()
        (_xu, _tu, eu), (_xc, _tc, ec) = smp.plan.halves
        rec.append((before, hist, eu.clone(), ec.clone(), smp.params.clone(), smp.rs_factors.clone(), smp.state.clone(), smp.x0_prev.clone() if ms else None))
    smp._enqueue = spy
    eager = smp.sample(_x(vids))
    assert len(rec) == N6 and smp.graphs == {}
    pipe = lambda e: e.reshape(1, FR, 4, H, W).permute(0, 2, 1, 3, 4)
    worst = 0
    for i, (before, hist, eu, ec, prm, fac, after, hist_after) in enumerate(rec):
        p = [float(v) for v in prm.cpu()]
        g = p[6] if ms else p[5]
        assert g == 9.0
        vu, vc = pipe(eu).cpu().numpy(), pipe(ec).cpu().numpy()
        d = int(ulps(fac.cpu().numpy(), GD.vpred_rescale_factors_reference(vu, vc, g, PHI))[0])
        assert d <= 1 and float(fac[0]) >= 1.0 - PHI - 1e-6 and float(fac[0]) != 1.0, (i, fac)      # f = phi * ratio + (1 - phi), ratio >= 0
        worst = max(worst, d)
        v = np.concatenate([vu, vc])
        if ms:
            want, want0 = GD.vpred_rescaled_multistep_reference(before.cpu().numpy(), v, hist.cpu().numpy(), fac.cpu().numpy(), g, p[1], p[2], p[3], p[4], p[5])
            assert np.array_equal(hist_after.cpu().numpy(), want0), i
        else:
            want, _ = GD.vpred_rescaled_step_reference(before.cpu().numpy(), v, fac.cpu().numpy(), g, p[1], p[2], p[3], p[4])
        assert np.array_equal(after.cpu().numpy(), want), i
    print(f"sampler factors streams = {streams} {solver}: worst {worst} ulp")
    assert torch.equal(eager, rec[-1][6]) and torch.isfinite(eager).all()
    keys = [(False, "ms", "rs"), (True, "ms", "rs")] if ms else [(False, "rs"), (True, "rs")]
    gs = _sampler(Wt, vids, streams, graphs=True, solver=solver, guidance_rescale=PHI)
    a = gs.sample(_x(vids))
    assert torch.equal(a, eager) and sorted(gs.graphs) == keys
    b = gs.sample(_x(vids))                                     # every step replayed, the first one too
    assert torch.equal(b, eager) and sorted(gs.graphs) == keys


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_two_co_batched_videos_equal_their_single_runs(monkeypatch, solver):
    """S = 2 with different conditioning and seeds: each video equals its own S = 1 run bit for bit (one tiling everywhere, as in
    tests/test_video_batch_gpu.py): the statistics' partition per video does not depend on S"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt = _weights()
    vids = [_video(s) for s in (11, 12)]
    kw = dict(solver=solver, guidance_rescale=PHI)
    many = _sampler(Wt, vids, autotune=True, **kw).sample(_x(vids))
    for i, v in enumerate(vids):
        one = _sampler(Wt, [v], autotune=True, **kw).sample(_x([v]))
        assert torch.equal(many[i:i + 1], one), (i, float((many[i:i + 1] - one).abs().max()))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_sample_loop_with_the_rescale_equals_the_sampler(monkeypatch, solver):
    """one video, F32: the host loop on the scalar rs form gives the device loop's bits; its steps go through the factors entry and the scalar rs entry
    and no other step entry"""
    Wt, vid = _weights(), _video(3)
    kw = dict(solver=solver, guidance_rescale=PHI)
    want = _sampler(Wt, [vid], graphs=False, **kw).sample(_x([vid]))
    calls = _spy_entries(monkeypatch)
    got = _host_loop(Wt, vid, N6, "logsnr", 0.2, **kw)
    assert calls == ["tmix_vpred_rescale_factors", "tmix_vpred_step_rs" if solver == "ddim" else "tmix_vpred_step_ms_rs"] * N6
    assert torch.equal(got, want)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("solver,step,key", [("ddim", "tmix_vpred_step_dev", [False, True]), ("dpmpp2m", "tmix_vpred_step_ms_dev", [(False, "ms"), (True, "ms")])],
                         ids=["ddim", "dpmpp2m"])
def test_phi_zero_is_the_sampler_of_today_and_phi_moves_the_result(monkeypatch, solver, step, key):
    """guidance_rescale=0.0 spelled out equals the call without it: the same bits, the same entry calls, the same graph keys, no factors launch, no
    buffers; and sample_loop likewise.  phi = 0.7 at g = 9 gives another latent, through the rs entries"""
    Wt, vid = _weights(), _video(5)
    calls = _spy_entries(monkeypatch)
    for _ in (0,):
        runs = []
        for graphs in (False, True):
            for kw in ({}, dict(guidance_rescale=0.0)):
                smp = _sampler(Wt, [vid], graphs=graphs, solver=solver, **kw)
                out = smp.sample(_x([vid]))
                runs.append((out, list(calls), smp))
                calls[:] = []
        for (oa, ca, sa), (ob, cb, sb) in ((runs[0], runs[1]), (runs[2], runs[3])):
            assert torch.equal(oa, ob) and ca == cb and sorted(sa.graphs) == sorted(sb.graphs)
            assert sb.rs_factors is None and sb._rs_ws is None and sb.guidance_rescale == 0.0
            assert not any(c in RS_ENTRIES for c in cb)
        assert runs[1][1] == ["tmix_video_step_prologue", step] * N6 and sorted(runs[3][2].graphs) == key
        assert torch.equal(runs[0][0], runs[2][0])
        a = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver)
        scalar = [step[:-4]] * N6
        assert calls == scalar
        calls[:] = []
        b = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver, guidance_rescale=0.0)
        assert calls == scalar and torch.equal(a, b) and torch.equal(a, runs[0][0])
        calls[:] = []
        rs = _sampler(Wt, [vid], graphs=False, solver=solver, guidance_rescale=PHI).sample(_x([vid]))
        assert calls == ["tmix_video_step_prologue", "tmix_vpred_rescale_factors", step[:-4] + "_rs_dev"] * N6
        assert torch.isfinite(rs).all() and not torch.equal(rs, runs[0][0])
        calls[:] = []


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.timeout(120)
def test_cli_run_with_the_flag_writes_its_latent_through_the_rs_entries(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("rv_rescale_gpu", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    calls = _spy_entries(monkeypatch)
    common = ["--synthetic", "--tiny", "--height", "128", "--width", "64", "--num_inference_steps", "6", "--injection_timestep", "0.2", "--seed", "4",
              "--solver", "dpmpp2m", "--timestep_spacing", "logsnr"]
    lat = rv.main(common + ["--guidance_rescale", "0.7", "--output_dir", str(tmp_path / "rs")]).cpu()
    assert set(calls) == {"tmix_video_step_prologue", "tmix_vpred_rescale_factors", "tmix_vpred_step_ms_rs_dev"}
    calls[:] = []
    ref = rv.main(common + ["--output_dir", str(tmp_path / "plain")]).cpu()
    assert set(calls) == {"tmix_video_step_prologue", "tmix_vpred_step_ms_dev"}
    assert lat.shape == (1, 4, 16, 16, 8) and torch.isfinite(lat).all() and not torch.equal(lat, ref)
    assert torch.equal(torch.load(tmp_path / "rs" / "output_i2v_seed_4.latent.pt"), lat)
    two = rv.main(common + ["--guidance_rescale", "0.7", "--num_seeds", "2", "--no_graphs", "--streams", "1", "--output_dir", str(tmp_path / "rs2")]).cpu()
    assert two.shape == (2, 4, 16, 16, 8) and torch.isfinite(two).all()
