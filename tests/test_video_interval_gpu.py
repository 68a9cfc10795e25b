"""GPU: the guidance interval of the VIDEO sampler -- tmix_video_step_prologue_cond / tmix_vpred_step_cond / tmix_vpred_step_cond_dev,
I2VVideoPlan.run_cond, VideoSampler(guidance_interval=...), sample_loop(guidance_interval=..., unet_cond=...), run_video.py --guidance_interval.

Every comparison is an equality (on uint32 views where a sign bit or a NaN matters): the entries against tweediemix_amd.guidance.vpred_cond_step_reference
and against their guided parents called with v_u := v_c, the samplers against the chain of restatements."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import video_interval_cases as VI
from layout_frames import Frame, dense_guarded
from test_video_solver_gpu import DT, FR, H, N6, W, _dev_case, _pipe, _sampler, _schedule, _video, _weights, _x

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, F, HH, WW, HW = VI.C, VI.F, VI.HH, VI.WW, VI.HW
AT, AW = NF(0.2345), NF(0.2871)                               # alpha of the step (VI.SA, VI.S1 are its roots) and of the state it writes
NOHOLD = (None, 0, 1, None, 0, 1)
COND = ("tmix_video_step_prologue_cond", "tmix_vpred_step_cond", "tmix_vpred_step_cond_dev")
ENTRIES = ("tmix_vpred_step", "tmix_vpred_step_dev", "tmix_vpred_step_ms", "tmix_vpred_step_ms_dev", "tmix_vpred_step_rs", "tmix_vpred_step_rs_dev",
           "tmix_vpred_step_ms_rs", "tmix_vpred_step_ms_rs_dev", "tmix_video_step_prologue", "tmix_vpred_rescale_factors", "tmix_vpred_step_noise",
           "tmix_vpred_step_noise_dev", "tmix_vpred_step_hold", "tmix_vpred_step_hold_dev", "tmix_video_hold_composite") + COND
FORMS = [(k, p) for k in VI.MOVES for p in VI.PACKS]


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from tweediemix_amd import lib as L
    return L, L.load()


def _dtc(dt):
    L, _ = _lib()
    return {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[dt] if isinstance(dt, str) else dt


def _keys(keys):
    return torch.from_numpy(np.array(keys, dtype=np.uint32).view(np.int32).reshape(-1, 2).copy()).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _same(a, b):
    return np.array_equal(VI.bits(a), VI.bits(b))


def _t(a, dt="f32"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt][0]).cuda()


def _move3(kind):
    return (VI.MOVES[kind] + (0.0,))[:3]


def _dense(kind, pack, x, vc, out, prev, dt, keys, shape, hold, cz=VI.CZ, step=VI.STEP):
    """raw ABI call of tmix_vpred_step_cond -> the code.  kind "ddim": no history; pack "plain": no keys; pack != "hold": no hold arrays"""
    _, lib = _lib()
    return lib.tmix_vpred_step_cond(_p(x), _p(vc), _p(out), None if kind == "ddim" else _p(prev), _dtc(dt), *shape, VI.SA, VI.S1, *_move3(kind), float(cz),
                                    None if pack == "plain" else _p(keys), step, VI.HA, VI.HS, *(hold if pack == "hold" else NOHOLD), _st())


def _rows(kind, pack, x, vc, sc, prev, prm, keys, shape, hold):
    """raw ABI call of tmix_vpred_step_cond_dev -> the code"""
    _, lib = _lib()
    return lib.tmix_vpred_step_cond_dev(_p(x), _p(vc), sc, _p(prm), *shape, None if kind == "ddim" else _p(prev), None if pack == "plain" else _p(keys),
                                        *(hold if pack == "hold" else NOHOLD), _st())


def _hold_dev(S, seed, hh=HH, ww=WW, frames=F):
    """-> (kx numpy, wt numpy, the six ABI arguments, the device tensors)"""
    kx, wt = VI.hold_case(S, seed, hh, ww, frames)
    tk, tw = _t(kx), _t(wt)
    return kx, wt, (_p(tk), kx[0].size, 1, _p(tw), wt[0].size, frames), (tk, tw)


def _prm(kind, pack, g=9.0):
    return torch.tensor(VI.params(kind, pack, g=g), dtype=F32).cuda()


# ------------------------------------------------------------------------------------------------ 1: the entries == the restatement
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dt", list(DT))
def test_dense_entry_equals_the_restatement(dt, S):
    """{DDIM, first order, second order} x {plain, cz != 0, hold}: output and history by equality; x, v_c, out and x0_prev sit in guard-band frames;
    in the multistep forms a second launch with out aliasing x gives the same bits"""
    tdt, lowp = DT[dt]
    keys = VI.KEYS[:S]
    dk = _keys(keys)
    shape = (S, C, F, HW)
    iv = torch.int32 if dt == "f32" else torch.int16
    for n, (kind, pack) in enumerate(FORMS):
        x, vc, prev = VI.case(S, dt, 100 + n)
        kx, wt, hold, _live = _hold_dev(S, 200 + n)
        want, want0 = VI.reference(kind, pack, x, vc, prev, keys, (kx, wt), lowp)
        xin = Frame.of(_t(x, dt).reshape(S * C * F, HW), name="x").seal()
        vin = Frame.of(_t(vc, dt).reshape(S * C * F, HW), name="v_c").seal()
        out = dense_guarded((S * C * F, HW), tdt, rows=8, device="cuda", name="out")
        hf = Frame.of(_t(prev).reshape(S * C * F, HW), name="x0_prev")
        assert _dense(kind, pack, xin.view, vin.view, out.view, hf.view, dt, dk, shape, hold) == 0
        torch.cuda.synchronize()
        out.assert_untouched()
        out.assert_all_written()
        hf.assert_untouched()
        xin.assert_unchanged()
        vin.assert_unchanged()
        what = (dt, S, kind, pack)
        assert _same(_np(out.view).reshape(x.shape), want), what
        assert _same(_np(hf.view).reshape(x.shape), prev if kind == "ddim" else want0), what
        if kind != "ddim":                                     # out aliasing x
            xi = Frame.of(_t(x, dt).reshape(S * C * F, HW), name="x=out")
            h2 = _t(prev)
            assert _dense(kind, pack, xi.view, vin.view, xi.view, h2, dt, dk, shape, hold) == 0
            torch.cuda.synchronize()
            xi.assert_untouched()
            assert torch.equal(xi.view.view(iv), out.view.view(iv)) and torch.equal(h2.reshape(-1), hf.view.reshape(-1)), what


@pytest.mark.parametrize("S", [1, 3])
def test_rows_entry_equals_the_restatement_and_does_not_read_g(S):
    """the same forms on plan rows: v_c in its own buffer | inside one buffer of 2S clips at clip S, clip stride dense | padded with NaN in the padding;
    state and history in place inside guard-band frames; the prediction rows and their padding stay untouched; with NaN in the g slot the result
    is the same finite bits"""
    keys = VI.KEYS[:S]
    dk = _keys(keys)
    shape = (S, C, F, HW)
    n = 0
    for layout in ("two", "one"):
        for pad in (False, True):
            for kind, pack in FORMS:
                n += 1
                x, prev, frames, (_vu, _su, vc, sc), (_eu, ec) = _dev_case(S, F, HW, layout, pad, 300 + n)
                kx, wt, hold, _live = _hold_dev(S, 400 + n)
                kx4, wt3 = kx.reshape(kx.shape[:3] + (HW,)), wt.reshape(wt.shape[:2] + (HW,))
                want, want0 = VI.reference(kind, pack, _np(x), _np(_pipe(ec, S, F, C, HW)), _np(prev), keys, (kx4, wt3))
                for g in (9.0, float("nan")):
                    xf = Frame.of(x.reshape(S * C * F, HW), name="x")
                    hf = Frame.of(prev.reshape(S * C * F, HW), name="x0_prev")
                    prm = Frame.of(_prm(kind, pack, g).reshape(1, -1), name="params").seal()
                    assert _rows(kind, pack, xf.view, vc, sc, hf.view, prm.view, dk, shape, hold) == 0
                    torch.cuda.synchronize()
                    xf.assert_untouched()
                    hf.assert_untouched()
                    prm.assert_unchanged()
                    for f in frames:
                        f.assert_unchanged()
                    what = (S, layout, pad, kind, pack, g)
                    assert torch.isfinite(xf.view).all(), what
                    assert _same(_np(xf.view).reshape(want.shape), want), what
                    assert _same(_np(hf.view).reshape(want.shape), _np(prev) if kind == "ddim" else want0), what


# ------------------------------------------------------------------------------------------------ 2: == the guided parents with v_u := v_c
@pytest.mark.parametrize("dt", list(DT))
def test_each_entry_equals_its_guided_parents_called_with_the_conditional_prediction_twice(dt):
    """g = 9, inputs without a zero: tmix_vpred_step / _ms, tmix_vpred_step_noise and tmix_vpred_step_hold on v = [v_c, v_c], and on plan rows their
    _dev forms with v_u = v_c, store what the unguided entry stores (through the ops wrappers, which form sa, s1, ha, hs the same way)"""
    from tweediemix_amd import ops
    S = 3
    dk = _keys(VI.KEYS)
    iv = torch.int32 if dt == "f32" else torch.int16
    for n, (kind, pack) in enumerate(FORMS):
        x, vc, prev = VI.case(S, dt, 500 + n)
        kx, wt, _hold, (tk, tw) = _hold_dev(S, 600 + n)
        tx, tv = _t(x, dt), _t(vc, dt)
        v2 = torch.cat([tv, tv])
        move = VI.MOVES[kind]
        ha, hb = (None, None) if kind == "ddim" else (_t(prev), _t(prev))
        if pack == "hold":
            want = ops.vpred_step_hold(tx, v2, 9.0, AT, move, VI.CZ, dk, VI.STEP, AW, tk, tw, x0_prev=ha)
            got = ops.vpred_step_cond(tx, tv, AT, move, hb, VI.CZ, dk, VI.STEP, AW, tk, tw)
        elif pack == "noise":
            want = ops.vpred_step_noise(tx, v2, 9.0, AT, move, VI.CZ, dk, VI.STEP, x0_prev=ha)
            got = ops.vpred_step_cond(tx, tv, AT, move, hb, VI.CZ, dk, VI.STEP)
        else:
            want = ops.vpred_step_ms(tx, v2, 9.0, AT, move, ha) if kind != "ddim" else ops._vpred_dense(tx, v2, 9.0, AT, move, None, None, None)
            got = ops.vpred_step_cond(tx, tv, AT, move, hb)
        torch.cuda.synchronize()
        assert torch.equal(got.view(iv), want.view(iv)) and torch.isfinite(got.float()).all(), (dt, kind, pack)
        assert kind == "ddim" or torch.equal(ha, hb), (dt, kind, pack)
    if dt != "f32":
        return
    for layout, pad in (("two", False), ("one", True)):
        for kind, pack in FORMS:
            x, prev, frames, (_vu, _su, vc, sc), _ = _dev_case(S, F, HW, layout, pad, 700)
            kx, wt, _hold, (tk, tw) = _hold_dev(S, 701)
            x5 = lambda: x.clone().view(S, C, F, HH, WW)
            ha, hb = (None, None) if kind == "ddim" else (prev.clone().view(S, C, F, HH, WW), prev.clone().view(S, C, F, HH, WW))
            # the wrappers take a contiguous buffer from clip 0 of the half on and the clip stride by argument: the frame's own flat storage
            fr = frames[-1]
            first = fr.front + (S * sc if layout == "one" else 0)
            rows = fr.buf[first:first + (S - 1) * sc + F * C * HW]
            assert rows.data_ptr() == vc.data_ptr()
            prm = _prm(kind, pack)
            if pack == "hold":
                want = ops.vpred_step_hold_dev(x5(), rows, rows, prm, dk, tk, tw, x0_prev=ha, clip_stride_u=sc, clip_stride_c=sc)
            elif pack == "noise":
                want = ops.vpred_step_noise_dev(x5(), rows, rows, prm, dk, x0_prev=ha, clip_stride_u=sc, clip_stride_c=sc)
            elif kind != "ddim":
                want = ops.vpred_step_ms_dev(x5(), rows, rows, ha, prm, clip_stride_u=sc, clip_stride_c=sc)
            else:
                want = ops.vpred_step_dev(x5(), rows, rows, prm, clip_stride_u=sc, clip_stride_c=sc)
            got = ops.vpred_step_cond_dev(x5(), rows, prm, hb, None if pack == "plain" else dk, *((tk, tw) if pack == "hold" else (None, None)),
                                          clip_stride_c=sc)
            torch.cuda.synchronize()
            assert torch.equal(got, want) and torch.isfinite(got).all() and (kind == "ddim" or torch.equal(ha, hb)), (layout, pad, kind, pack)


# ------------------------------------------------------------------------------------------------ 3: large, batched
def test_second_pass_of_the_grid_stride_loop():
    """1 x 4 x 16 x 16385 = 1,048,640 elements > 4096 workgroups x 256 threads: threads of the capped grid take a second element; the rows entry and
    the dense f32 entry, in the second-order form with noise, by equality"""
    S, Fb, hw = 1, 16, 16385
    assert 4096 * 256 < S * C * Fb * hw < 4096 * 256 + 256
    keys = VI.KEYS[1:2]
    dk = _keys(keys)
    x, prev, _frames, (_vu, _su, vc, sc), (_eu, ec) = _dev_case(S, Fb, hw, "two", False, 9)
    v = _pipe(ec, S, Fb, C, hw).contiguous()
    want, want0 = VI.reference("second", "noise", _np(x), _np(v), _np(prev), keys, None)
    xd, hd = x.clone(), prev.clone()
    assert _rows("second", "noise", xd, vc, sc, hd, _prm("second", "noise"), dk, (S, C, Fb, hw), None) == 0
    out, h2 = torch.empty_like(x), prev.clone()
    assert _dense("second", "noise", x, v, out, h2, "f32", dk, (S, C, Fb, hw), None) == 0
    torch.cuda.synchronize()
    assert _same(_np(xd), want) and _same(_np(hd), want0) and torch.equal(out, xd) and torch.equal(h2, hd)


def test_co_batched_videos_equal_single_launches_and_keys_belong_to_videos():
    """S = 3 equals three S = 1 launches with the respective keys, held latents and weights (both entries); swapping two videos' keys changes those
    two videos alone"""
    S = 3
    x, prev, _frames, (_vu, _su, vc, sc), (_eu, ec) = _dev_case(S, F, HW, "one", True, 21)
    dv = _pipe(ec, S, F, C, HW).contiguous()
    kx, wt, hold, (tk, tw) = _hold_dev(S, 22)
    shape = (S, C, F, HW)
    for kind in ("ddim", "second"):
        many, hm = x.clone(), prev.clone()
        assert _rows(kind, "hold", many, vc, sc, hm, _prm(kind, "hold"), _keys(VI.KEYS), shape, hold) == 0
        dmany, dh = torch.empty_like(x), prev.clone()
        assert _dense(kind, "hold", x.contiguous(), dv, dmany, dh, "f32", _keys(VI.KEYS), shape, hold) == 0
        torch.cuda.synchronize()
        assert torch.equal(dmany, many) and torch.equal(dh, hm)
        for s in range(S):
            h1 = (_p(tk[s:]), kx[0].size, 1, _p(tw[s:]), wt[0].size, F)
            one, p1 = x[s:s + 1].clone(), prev[s:s + 1].clone()
            assert _rows(kind, "hold", one, vc[s:], sc, p1, _prm(kind, "hold"), _keys(VI.KEYS[s:s + 1]), (1, C, F, HW), h1) == 0
            torch.cuda.synchronize()
            assert torch.equal(one, many[s:s + 1]) and torch.equal(p1, hm[s:s + 1]), (kind, s)
        sw = [VI.KEYS[1], VI.KEYS[0], VI.KEYS[2]]
        swapped, hs_ = x.clone(), prev.clone()
        assert _rows(kind, "hold", swapped, vc, sc, hs_, _prm(kind, "hold"), _keys(sw), shape, hold) == 0
        torch.cuda.synchronize()
        assert torch.equal(swapped[2], many[2]) and torch.equal(hs_, hm)
        assert not torch.equal(swapped[0], many[0]) and not torch.equal(swapped[1], many[1])


# ------------------------------------------------------------------------------------------------ 4: the prologue
@pytest.mark.parametrize("S", [1, 3])
def test_prologue_writes_the_text_half_alone(S):
    """the text half's rows and t_c equal what tmix_video_step_prologue writes there (dense and padded clip stride); the image-latent channels, the
    padding, and a poisoned unconditional buffer (which the entry is not even told about) stay untouched"""
    _, lib = _lib()
    R = 2 * C
    clip = F * R * HW
    g = torch.Generator(device="cuda").manual_seed(5 + S)
    x = torch.randn(S, C, F, HW, device="cuda", generator=g)
    prm = torch.tensor([437.0] + [0.0] * 7, device="cuda")
    for pad in (0, 24):
        init = torch.randn(S, F * R, HW, device="cuda", generator=g)
        xu, xc, xc_ref = (Frame.of(init, batch_stride=clip + pad, name=n) for n in ("x_u", "x_c", "x_c (guided prologue)"))
        xu.seal()
        tu, tc, tc_ref = (Frame.of(torch.full((1, S), -1.0, device="cuda"), name=n) for n in ("t_u", "t_c", "t_c ref"))
        tu.seal()
        assert lib.tmix_video_step_prologue(_p(x), _p(xu.view), clip + pad, _p(tu.view), _p(xc_ref.view), clip + pad, _p(tc_ref.view), _p(prm), S, C, F, HW, R, _st()) == 0
        xu2 = Frame.of(init, batch_stride=clip + pad, name="x_u poisoned").seal()
        assert lib.tmix_video_step_prologue_cond(_p(x), _p(xc.view), clip + pad, _p(tc.view), _p(prm), S, C, F, HW, R, _st()) == 0
        torch.cuda.synchronize()
        xu2.assert_unchanged()
        assert torch.equal(xc.bits, xc_ref.bits) and torch.equal(tc.bits, tc_ref.bits), (S, pad)      # the whole buffers, guards and padding included
        rows = xc.view.reshape(S, F, R, HW)
        assert torch.equal(rows[:, :, :C].permute(0, 2, 1, 3), x) and torch.equal(rows[:, :, C:], init.reshape(S, F, R, HW)[:, :, C:])
        assert tc.view.tolist() == [[437.0] * S]


# ------------------------------------------------------------------------------------------------ 5: the sampler on the tiny network
SEED_A, SEED_B = (9 << 32) + 4, 77
SWEEP = [(s, p, e, False) for s in ("ddim", "dpmpp2m") for p in (0.0, 0.7) for e in (0.0, 0.5)] + [("dpmpp2m", 0.7, 0.5, True)]
SWEEP_IDS = [f"{s}-phi{p}-eta{e}" + ("-hold" if h else "") for s, p, e, h in SWEEP]


def _spy_entries(monkeypatch):
    _, lib = _lib()
    calls = []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _interval(sch):
    ts = [int(t) for t in sch.timesteps]
    return (ts[1], ts[3]), ts


def _tiny_hold(S, seed):
    kx, wt = VI.hold_case(S, seed, H, W, FR)
    return torch.from_numpy(kx), torch.from_numpy(wt[:1])


def _kw(solver, phi, eta, hold, seeds, S=1):
    kw = dict(solver=solver, guidance_rescale=phi, eta=eta)
    if eta > 0.0 or hold:
        kw["noise_seeds"] = list(seeds)
    if hold:
        kw["hold"] = _tiny_hold(S, 50)
    return kw


def _guided_entry(ms, rs, eta, hold):
    if hold:
        return "tmix_vpred_step_hold_dev"
    if eta:
        return "tmix_vpred_step_noise_dev"
    return "tmix_vpred_step" + ("_ms" if ms else "") + ("_rs" if rs else "") + "_dev"


def _expected_calls(guided, ms, rs, eta, hold):
    calls = ["tmix_video_hold_composite"] if hold else []
    for g in guided:
        calls += ["tmix_video_step_prologue"] + (["tmix_vpred_rescale_factors"] if rs else []) + [_guided_entry(ms, rs, eta, hold)] if g else \
            ["tmix_video_step_prologue_cond", "tmix_vpred_step_cond_dev"]
    return calls


def _expected_keys(guided, inject, ms, rs, eta, hold):
    keys = set()
    for g, inj in zip(guided, inject):
        tail = (("ms",) if ms else ()) + (("rs",) if rs and g else ()) + (("eta",) if eta else ()) + (("hold",) if hold else ()) + (() if g else ("cond",))
        keys.add((inj,) + tail if tail else inj)
    return keys


@pytest.mark.timeout(120)
@pytest.mark.parametrize("streams", [2, 1])
@pytest.mark.parametrize("solver,phi,eta,hold", SWEEP, ids=SWEEP_IDS)
def test_sampler_every_step_equals_the_restatement_chain_and_graph_equals_eager(monkeypatch, solver, phi, eta, hold, streams):
    """n = 6 on the log-SNR grid at g = 9, interval (ts[1], ts[3]): after EVERY step the state (and history) equals the restatement -- the guided one
    or the unguided one -- applied to the plan's own prediction rows with the uploaded floats; the solver's orders are first, first, second, second,
    first, second; guided steps go through today's entries, unguided ones through prologue_cond + step_cond_dev and nothing else (no factors
    launch); graph replay equals eager and the graph keys are the guided ones plus (inject, ..., "cond") without "rs" """
    from tweediemix_amd import guidance as GD, noise as NZ
    ms, rs, wide = solver != "ddim", phi > 0.0, eta > 0.0 or hold
    Wt, vids = _weights(), [_video(3)]
    kw = _kw(solver, phi, eta, hold, [SEED_A])
    iv, ts = _interval(_schedule())
    second, guided = VI.interval_orders(ts, iv)
    smp = _sampler(Wt, vids, streams, graphs=False, guidance_interval=iv, **kw)
    assert smp.guidance_interval == iv and smp.params.numel() == (12 if wide else 8)
    rec = []

    def spy(real, is_guided):
        def run():
            before, hist = smp.state.clone(), (smp.x0_prev.clone() if ms else None)
            real()
            torch.cuda.synchronize()
            (_xu, _tu, eu), (_xc, _tc, ec) = smp.plan.halves
            rows = (eu.clone(), ec.clone()) if is_guided else (None, smp.plan.cond_half[2].clone())
            rec.append((is_guided, before, hist, rows, smp.params.clone(), smp.rs_factors.clone() if rs else None, smp.state.clone(),
                        smp.x0_prev.clone() if ms else None, smp.plan.inject))
        return run
    smp._enqueue, smp._enqueue_cond = spy(smp._enqueue, True), spy(smp._enqueue_cond, False)
    calls = _spy_entries(monkeypatch)
    eager = smp.sample(_x(vids))
    assert calls == _expected_calls(guided, ms, rs, eta > 0.0, hold)
    assert [r[0] for r in rec] == guided and smp.graphs == {} and torch.isfinite(eager).all() and torch.equal(eager, rec[-1][6])
    key = [NZ.seed_key(SEED_A)] if wide else None
    hd = tuple(a.numpy() for a in kw["hold"]) if hold else None
    pipe = lambda e: _np(e.reshape(1, FR, 4, H, W).permute(0, 2, 1, 3, 4))
    for i, (is_guided, before, hist, (eu, ec), prm, fac, after, hist_after, _inj) in enumerate(rec):
        p = [float(c) for c in prm.cpu()]
        assert p[0] == float(ts[i]) and (p[6] if ms else p[5]) == 9.0 and (not wide or p[9] == float(i)), (i, p)      # g is still uploaded
        if ms:
            assert (p[5] != 0.0) == second[i], (i, p)
        x, h0 = _np(before), _np(hist) if ms else None
        if not is_guided:
            want, want0 = GD.vpred_cond_step_from_params(x, pipe(ec), h0, p, key, hd)
        else:
            v, f = np.concatenate([pipe(eu), pipe(ec)]), _np(fac) if rs else None
            if hold:
                want, want0 = NZ.vpred_hold_reference(x, v, h0, p, key, hd[0], hd[1], None, f)
            elif wide:
                want, want0 = NZ.vpred_step_reference(x, v, h0, p, key, None, f)
            elif ms:
                want, want0 = GD.vpred_rescaled_multistep_reference(x, v, h0, np.ones(1, NF) if f is None else f, p[6], p[1], p[2], p[3], p[4], p[5])
            else:
                want, want0 = GD.vpred_rescaled_step_reference(x, v, np.ones(1, NF) if f is None else f, p[5], p[1], p[2], p[3], p[4])
        assert _same(_np(after), want), (i, is_guided)
        if ms:
            assert _same(_np(hist_after), want0), (i, is_guided)
    calls[:] = []
    gs = _sampler(Wt, vids, streams, graphs=True, guidance_interval=iv, **kw)
    want_keys = _expected_keys(guided, [r[8] for r in rec], ms, rs, eta > 0.0, hold)
    a = gs.sample(_x(vids))
    assert torch.equal(a, eager) and set(gs.graphs) == want_keys and len(want_keys) == 3
    b = gs.sample(_x(vids))                                     # every step replayed, the first one too
    assert torch.equal(b, eager) and set(gs.graphs) == want_keys
    assert gs.params.numel() == smp.params.numel() and gs._ring.slots.shape[1] == (12 if wide else 8)      # one 32- or 48-byte upload per step
    assert not rs or calls.count("tmix_vpred_rescale_factors") == 2 * 1                                   # warm-up and capture of the one guided graph
    plain = _sampler(Wt, vids, streams, graphs=True, **kw).sample(_x(vids))
    assert not torch.equal(plain, eager)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver,phi,eta,hold", SWEEP, ids=SWEEP_IDS)
def test_two_co_batched_videos_equal_their_single_runs_and_sample_loop_equals_the_sampler(monkeypatch, solver, phi, eta, hold):
    """S = 2 with different conditioning, x_T and seeds: each video equals its own S = 1 run bit for bit; the host loop on the dense entries, with
    unet_cond running the text chain alone, gives the device loop's bits: tmix_vpred_step_cond on the unguided steps, today's entry on the others"""
    from tweediemix_amd import i2vgen as I, video as V
    ms, rs = solver != "ddim", phi > 0.0
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt = _weights()
    vids = [_video(s) for s in (11, 12)]
    iv, ts = _interval(_schedule())
    _second, guided = VI.interval_orders(ts, iv)
    kw2 = _kw(solver, phi, eta, hold, [SEED_A, SEED_B], S=2)
    many = _sampler(Wt, vids, autotune=True, guidance_interval=iv, **kw2).sample(_x(vids))
    for i, (v, seed) in enumerate(zip(vids, (SEED_A, SEED_B))):
        kw1 = dict(kw2)
        if "noise_seeds" in kw1:
            kw1["noise_seeds"] = [seed]
        if hold:
            kw1["hold"] = (kw2["hold"][0][i:i + 1], kw2["hold"][1])
        one = _sampler(Wt, [v], autotune=True, guidance_interval=iv, **kw1).sample(_x([v]))
        assert torch.equal(many[i:i + 1], one), (i, float((many[i:i + 1] - one).abs().max()))
    monkeypatch.delenv("TMIX_FORCE_TILE")
    kw = _kw(solver, phi, eta, hold, [SEED_A])
    want = _sampler(Wt, vids[:1], graphs=False, guidance_interval=iv, **kw).sample(_x(vids[:1]))
    c, x = vids[0]
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0, 8.0]), c["il"], c["ie"], c["pe"])
    plan = I.I2VPlanGroup(Wt, 2, FR, H, W, fe, ctx, ilf, autotune=False)
    sch = _schedule()
    inj = V.FeatureInjector(sch.injection_schedule(0.2), 0.7, clips=2, frames=FR)

    def unet(xin, t):
        plan.inject, plan.interp = V.injection_active(t, inj.schedule), inj.interp
        plan.set_input(xin, t)
        plan.run()
        return plan.eps.view(2, FR, 4, H, W).permute(0, 2, 1, 3, 4).contiguous()

    def unet_cond(xin, t):
        plan.inject, plan.interp = V.injection_active(t, inj.schedule), inj.interp
        xc, tc, ec = plan.cond_half
        xc.view(FR, 8, H, W)[:, :4] = xin[0].to(torch.float32).permute(1, 0, 2, 3)
        tc.fill_(float(t))
        plan.run_cond()
        return ec.view(1, FR, 4, H, W).permute(0, 2, 1, 3, 4).contiguous()
    calls = _spy_entries(monkeypatch)
    got = V.sample_loop(unet, x.cuda(), sch, 9.0, inj, guidance_interval=iv, unet_cond=unet_cond, **kw)
    dense = _guided_entry(ms, rs, eta > 0.0, hold)[:-4]
    per = lambda g: ((["tmix_vpred_rescale_factors"] if rs else []) + [dense]) if g else ["tmix_vpred_step_cond"]
    assert calls == (["tmix_video_hold_composite"] if hold else []) + [n for g in guided for n in per(g)]
    assert torch.equal(got, want)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("streams", [2, 1])
def test_the_unguided_steps_text_rows_are_the_guided_steps_text_rows(monkeypatch, streams):
    """the same state and timestep through a guided and an unguided step: the text half's prediction rows are the same bits -- at streams=2 because
    they are the same recorded launches, at streams=1 (the text clips inside the 2S-clip chain | a chain of their own, built on first use, with
    the injection flags of the moment) under TMIX_FORCE_TILE=1, where both chains take the same tiles"""
    if streams == 1:
        monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt, vids = _weights(), [_video(s) for s in (11, 12)]
    sch = _schedule()
    ts = [int(t) for t in sch.timesteps]
    guided = _sampler(Wt, vids, streams, graphs=False, autotune=streams == 1)
    cond = _sampler(Wt, vids, streams, graphs=False, autotune=streams == 1, guidance_interval=(0, 0))
    assert (cond.plan._cond is None) == (streams == 1) and cond.plan.cond_flops * 2 == cond.plan.flops
    for t in (ts[0], ts[2]):                                    # with the injection and without
        for smp in (guided, cond):
            smp.state.copy_(_x(vids))
            smp.step(t)
        torch.cuda.synchronize()
        assert guided.plan.inject == cond.plan.cond_plan.inject == (t == ts[0])
        assert torch.equal(cond.plan.cond_half[2], guided.plan.halves[1][2]), (streams, t)
        assert not torch.equal(cond.state, guided.state)
    assert cond.plan.cond_plan.flops == cond.plan.cond_flops            # every launch's work is linear in the clip count
    if streams == 2:
        assert cond.plan.cond_plan is cond.plan.plans[1] and cond.plan.cond_half[2] is cond.plan.halves[1][2]
    else:
        assert cond.plan.cond_plan is not cond.plan.plans[0] and cond.plan.cond_plan.clips == 2 and guided.plan._cond is None


# ------------------------------------------------------------------------------------------------ 6: no interval is today's sampler
@pytest.mark.timeout(180)
@pytest.mark.parametrize("solver,step,key", [("ddim", "tmix_vpred_step_dev", [False, True]), ("dpmpp2m", "tmix_vpred_step_ms_dev", [(False, "ms"), (True, "ms")])],
                         ids=["ddim", "dpmpp2m"])
def test_no_interval_and_an_interval_that_holds_every_timestep_are_the_sampler_of_today(monkeypatch, solver, step, key):
    """guidance_interval=None spelled out and (1000, 0) equal the call without the argument: the same bits, entry calls, graph keys and upload sizes,
    eagerly and with graphs; no unguided entry runs and no text chain of its own is built"""
    Wt, vid = _weights(), _video(5)
    calls = _spy_entries(monkeypatch)
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(guidance_interval=None), dict(guidance_interval=(1000, 0)), dict(guidance_interval="1000,1")):
            smp = _sampler(Wt, [vid], graphs=graphs, solver=solver, **kw)
            runs.append((smp.sample(_x([vid])), list(calls), smp))
            calls[:] = []
    for base, others in ((runs[0], runs[1:4]), (runs[4], runs[5:8])):
        for ob, cb, sb in others:
            assert torch.equal(base[0], ob) and base[1] == cb and sorted(base[2].graphs) == sorted(sb.graphs)
            assert sb.params.numel() == 8 and sb._ring.slots.shape[1] == 8 and not any(c in COND for c in cb)
    assert runs[1][1] == ["tmix_video_step_prologue", step] * N6 and sorted(runs[6][2].graphs) == key and torch.equal(runs[0][0], runs[4][0])
    one = _sampler(Wt, [vid], streams=1, graphs=True, solver=solver, guidance_interval=(1000, 0))
    assert torch.isfinite(one.sample(_x([vid]))).all() and one.plan._cond is None and sorted(one.graphs) == key


# ------------------------------------------------------------------------------------------------ 7: CLI
@pytest.mark.timeout(180)
def test_cli_run_with_the_interval(tmp_path, monkeypatch, capsys):
    """run_video.py --tiny --synthetic --guidance_interval 700,250 (n = 6 'leading': 665, 499, 333 are guided): a finite latent that differs from
    the unflagged run's, through the unguided entries on three steps; rank 0 says how many; 1000,0 is the unflagged run bit for bit"""
    spec = importlib.util.spec_from_file_location("rv_interval_gpu", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    calls = _spy_entries(monkeypatch)
    common = ["--synthetic", "--tiny", "--height", "128", "--width", "64", "--num_inference_steps", "6", "--injection_timestep", "0.2", "--seed", "4",
              "--no_graphs"]
    plain = rv.main(common + ["--output_dir", str(tmp_path / "plain")]).cpu()
    assert calls == ["tmix_video_step_prologue", "tmix_vpred_step_dev"] * 6
    calls[:] = []
    capsys.readouterr()
    lat = rv.main(common + ["--guidance_interval", "700,250", "--output_dir", str(tmp_path / "a")]).cpu()
    assert "3 of the schedule's 6 steps are unguided" in capsys.readouterr().out
    un, gd = ["tmix_video_step_prologue_cond", "tmix_vpred_step_cond_dev"], ["tmix_video_step_prologue", "tmix_vpred_step_dev"]
    assert calls == un + gd * 3 + un * 2
    assert lat.shape == (1, 4, 16, 16, 8) and torch.isfinite(lat).all() and not torch.equal(lat, plain)
    assert torch.equal(torch.load(tmp_path / "a" / "output_i2v_seed_4.latent.pt"), lat)
    whole = rv.main(common + ["--guidance_interval", "1000,0", "--output_dir", str(tmp_path / "w")]).cpu()
    assert torch.equal(whole, plain)
