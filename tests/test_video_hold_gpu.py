"""GPU: hold regions of the VIDEO sampler -- tmix_vpred_step_hold / tmix_vpred_step_hold_dev / tmix_video_hold_composite,
sample_loop(hold=...), VideoSampler(hold=...), run_video.py --hold_masks / --animate_masks / --hold_latents.

Every comparison is an equality (on uint32 views where a sign bit or a NaN matters): the three entries against tweediemix_amd.noise.vpred_hold_reference
/ video_hold_composite_reference, the weight-0 launches against the noise entries, the samplers against the chain of restatements."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import video_hold_cases as VH
import video_rescale_cases as VC
from layout_frames import _wrap, dense_guarded
from test_video_solver_gpu import DT, FR, G, H, N6, ORDERS, S1, SA, W, _dev_case, _host_loop, _pipe, _sampler, _video, _weights, _x

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SAN, S1D = float(NF(0.53582)), float(NF(0.78125))
KINDS = ("ddim", "second")
CZ, STEP, HA, HS = VH.CZ, VH.STEP, VH.HA, VH.HS
C, F, HH, WW, HW = VH.C, VH.F, VH.HH, VH.WW, VH.HW
HOLD_ENTRIES = ("tmix_vpred_step_hold", "tmix_vpred_step_hold_dev", "tmix_video_hold_composite")
ENTRIES = ("tmix_vpred_step", "tmix_vpred_step_dev", "tmix_vpred_step_ms", "tmix_vpred_step_ms_dev", "tmix_vpred_step_rs", "tmix_vpred_step_rs_dev",
           "tmix_vpred_step_ms_rs", "tmix_vpred_step_ms_rs_dev", "tmix_video_step_prologue", "tmix_vpred_rescale_factors", "tmix_vpred_step_noise",
           "tmix_vpred_step_noise_dev") + HOLD_ENTRIES
STRIDES = ("shared", "dense", "padded")


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


def _move(kind):
    return (SAN, S1D, 0.0) if kind == "ddim" else ORDERS[kind]


def _hold_arg(a, mode):
    """numpy [S or 1, ...] -> (device tensor, video stride in floats): "shared": the leading 1 serves every video (stride 0); "dense": one video's
    extent; "padded": 24 floats of NaN behind every video"""
    n, ext = a.shape[0], a[0].size
    if mode == "shared":
        assert n == 1
        return torch.from_numpy(a).cuda(), 0
    if mode == "dense":
        return torch.from_numpy(a).cuda(), ext
    buf = np.full((n, ext + 24), np.nan, NF)
    buf[:, :ext] = a.reshape(n, ext)
    return torch.from_numpy(buf).cuda(), ext + 24


def _hold(S, Fk, Fw, mode, seed, hh=HH, ww=WW):
    """-> (kx numpy [S or 1, C, Fk, h, w], w numpy [S or 1, Fw, h, w], the six ABI arguments, the tensors that keep them alive)"""
    n = 1 if mode == "shared" else S
    kx, wt = VH.held_latent(n, Fk, seed, hh, ww), VH.weight(n, Fw, seed + 1, hh, ww)
    (tk, sk), (tw, sw) = _hold_arg(kx, mode), _hold_arg(wt, mode)
    return kx, wt, (_p(tk), sk, Fk, _p(tw), sw, Fw), (tk, tw)


def _dense(kind, x, v, out, prev, dt, fac, keys, shape, hold, cz=CZ, step=STEP, ha=HA, hs=HS):
    """raw ABI call of tmix_vpred_step_hold -> the code; kind "ddim": no history buffer is passed"""
    _, lib = _lib()
    return lib.tmix_vpred_step_hold(_p(x), _p(v), _p(out), None if kind == "ddim" else _p(prev), _dtc(dt), *shape, float(G), float(SA), float(S1),
                                    *_move(kind), float(cz), _p(fac), _p(keys), step, float(ha), float(hs), *hold, _st())


def _noise_dense(kind, x, v, out, prev, dt, fac, keys, S, n, cz=CZ, step=STEP):
    _, lib = _lib()
    return lib.tmix_vpred_step_noise(_p(x), _p(v), _p(out), None if kind == "ddim" else _p(prev), _dtc(dt), S, n, float(G), float(SA), float(S1),
                                     *_move(kind), float(cz), _p(fac), _p(keys), step, _st())


def _prm(kind, cz=CZ, step=STEP, ha=HA, hs=HS, t=501.0):
    head = [t, SA, S1, SAN, S1D, G, 0.0, 0.0] if kind == "ddim" else [t, SA, S1, *ORDERS[kind], G, 0.0]
    return torch.tensor(head + [cz, float(step), ha, hs], dtype=F32).cuda()


def _rows(kind, x, ptrs, prev, prm, fac, keys, shape, hold):
    """raw ABI call of tmix_vpred_step_hold_dev -> the code"""
    _, lib = _lib()
    vu, su, vc, sc = ptrs
    return lib.tmix_vpred_step_hold_dev(_p(x), _p(vu), su, _p(vc), sc, _p(prm), *shape, None if kind == "ddim" else _p(prev), _p(fac), _p(keys), *hold, _st())


def _noise_rows(kind, x, ptrs, prev, prm, fac, keys, shape):
    _, lib = _lib()
    vu, su, vc, sc = ptrs
    return lib.tmix_vpred_step_noise_dev(_p(x), _p(vu), su, _p(vc), sc, _p(prm), *shape, None if kind == "ddim" else _p(prev), _p(fac), _p(keys), _st())


def _comp(x, dt, keys, shape, hold, ha=HA, hs=HS):
    _, lib = _lib()
    return lib.tmix_video_hold_composite(_p(x), _dtc(dt), *shape, float(ha), float(hs), _p(keys), *hold, _st())


def _ref(kind, x, v, prev, fac, keys, kx, wt, lowp, cz=CZ, step=STEP, ha=HA, hs=HS):
    from tweediemix_amd import noise as NZ
    return NZ.vpred_hold_reference(x, v, None if kind == "ddim" else prev, (G, SA, S1, *_move(kind), cz, ha, hs), keys, kx, wt, step, fac, lowp)


def _videos(S, dt, seed, hh=HH, ww=WW, frames=F):
    """-> x [S,C,F,h,w], v [2S,C,F,h,w] of the dtype, prev fp32 of x's shape, fac [S] in (0.3, 1)"""
    rng = np.random.RandomState(seed)
    tdt = TDT[dt]
    x = torch.from_numpy(rng.randn(S, C, frames, hh, ww).astype(NF)).to(tdt).cuda()
    v = torch.from_numpy(rng.randn(2 * S, C, frames, hh, ww).astype(NF)).to(tdt).cuda()
    prev = torch.from_numpy(rng.randn(S, C, frames, hh, ww).astype(NF)).cuda()
    fac = torch.from_numpy((0.3 + 0.7 * rng.rand(S)).astype(NF)).cuda()
    return x, v, prev, fac


def _same(a, b):
    """fp32 numpy arrays equal as bit patterns (a NaN payload and a sign of zero count)"""
    return np.array_equal(VH.bits(a), VH.bits(b))


# ------------------------------------------------------------------------------------------------ 1: both step entries == the restatement
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dt", list(TDT))
def test_dense_entry_equals_the_restatement(dt, S):
    """{DDIM, multistep} x {factors, none} x {cz = 0, cz > 0} x Fk in {1, F} x Fw in {1, F} x {shared, per-video, padded per-video} strides: output and
    history by equality, out of place and in place"""
    keys = VH.KEYS[:S]
    dk = _keys(keys)
    shape = (S, C, F, HW)
    n = 0
    for kind in KINDS:
        for rs in (False, True):
            for cz in (0.0, CZ):
                for Fk in (1, F):
                    for Fw in (1, F):
                        for mode in STRIDES:
                            n += 1
                            x, v, prev, fac = _videos(S, dt, 100 + n)
                            fac = fac if rs else None
                            kx, wt, hold, _live = _hold(S, Fk, Fw, mode, 200 + n)
                            out, hist = torch.empty_like(x), prev.clone()
                            assert _dense(kind, x, v, out, hist, dt, fac, dk, shape, hold, cz=cz) == 0
                            xin, hin = x.clone(), prev.clone()
                            assert _dense(kind, xin, v, xin, hin, dt, fac, dk, shape, hold, cz=cz) == 0
                            torch.cuda.synchronize()
                            want, want0 = _ref(kind, _np(x), _np(v), _np(prev), None if fac is None else _np(fac), keys, kx, wt, DT[dt][1], cz=cz)
                            what = (dt, S, kind, rs, cz, Fk, Fw, mode)
                            assert _same(_np(out), want), what
                            assert _same(_np(hist), _np(prev) if kind == "ddim" else want0), what
                            assert torch.equal(out.view(torch.int16 if dt != "f32" else torch.int32), xin.view(torch.int16 if dt != "f32" else torch.int32)), what
                            assert torch.equal(hist, hin), what


@pytest.mark.parametrize("S", [1, 3])
def test_rows_entry_equals_the_restatement(S):
    """the same sweep on plan rows (two half buffers | one buffer of 2S clips, dense | padded clip stride with NaN in the padding): state and history
    in place; the prediction rows stay untouched"""
    keys = VH.KEYS[:S]
    dk = _keys(keys)
    shape = (S, C, F, HW)
    n = 0
    for kind in KINDS:
        for rs in (False, True):
            for cz in (0.0, CZ):
                for Fk in (1, F):
                    for Fw in (1, F):
                        for mode in STRIDES:
                            n += 1
                            layout, pad = VC.LAYOUTS[n % len(VC.LAYOUTS)]
                            x, prev, frames, ptrs, (eu, ec) = _dev_case(S, F, HW, layout, pad, 300 + n)
                            fac = torch.from_numpy((0.3 + 0.7 * np.random.RandomState(n).rand(S)).astype(NF)).cuda() if rs else None
                            v = torch.cat([_pipe(eu, S, F, C, HW), _pipe(ec, S, F, C, HW)])
                            kx, wt, hold, _live = _hold(S, Fk, Fw, mode, 400 + n)
                            kx4, wt3 = kx.reshape(kx.shape[:3] + (HW,)), wt.reshape(wt.shape[:2] + (HW,))
                            want, want0 = _ref(kind, _np(x), _np(v), _np(prev), None if fac is None else _np(fac), keys, kx4, wt3, None, cz=cz)
                            state, hist = x.clone(), prev.clone()
                            assert _rows(kind, state, ptrs, hist, _prm(kind, cz=cz), fac, dk, shape, hold) == 0
                            torch.cuda.synchronize()
                            for f in frames:
                                f.assert_unchanged()
                            what = (S, kind, rs, cz, Fk, Fw, mode, layout, pad)
                            assert _same(_np(state), want), what
                            assert _same(_np(hist), _np(prev) if kind == "ddim" else want0), what


def test_second_pass_of_the_grid_stride_loop():
    """one video of 4 x 2 x 362 x 363 = 1,051,248 elements > 4096 workgroups x 256 threads: threads of the capped grid take a second element, whose
    held latent, weight and noise index are its own; the rows entry, the dense entry and the composite entry, by equality"""
    from tweediemix_amd import noise as NZ, ops
    Fb, hb, wb = VH.BIG
    S, hw = 1, hb * wb
    assert 4096 * 256 < S * C * Fb * hw
    keys = VH.KEYS[1:2]
    x, prev, _frames, _ptrs, (eu, ec) = _dev_case(S, Fb, hw, "two", False, 9)
    v = torch.cat([_pipe(eu, S, Fb, C, hw), _pipe(ec, S, Fb, C, hw)]).contiguous()
    fac = torch.tensor([0.6180339], device="cuda")
    kx, wt = VH.held_latent(1, 1, 3, hb, wb), VH.weight(1, Fb, 4, hb, wb)
    wt[:, :, -1, :], wt[:, :, -2, :] = 1.0, 0.0                    # the last 2672 elements are the second pass: both selects and fractions in it
    tk, tw = torch.from_numpy(kx).cuda(), torch.from_numpy(wt).cuda()
    x5, v5 = x.view(S, C, Fb, hb, wb), v.view(2 * S, C, Fb, hb, wb)
    want, want0 = _ref("second", _np(x5), _np(v5), _np(prev).reshape(x5.shape), _np(fac), keys, kx, wt, None)
    s5, h5 = x5.clone(), prev.clone().view(x5.shape)
    got = ops.vpred_step_hold_dev(s5, eu.view(S * Fb, C, hb, wb), ec.view(S * Fb, C, hb, wb), _prm("second"), _keys(keys), tk, tw, x0_prev=h5, factors=fac)
    torch.cuda.synchronize()
    assert got is s5 and _same(_np(s5), want) and _same(_np(h5), want0)
    hd, out = prev.clone(), torch.empty_like(x5)
    assert _dense("second", x5, v5, out, hd, "f32", fac, _keys(keys), (S, C, Fb, hw), (_p(tk), kx[0].size, 1, _p(tw), wt[0].size, Fb)) == 0
    torch.cuda.synchronize()
    assert _same(_np(out), want) and _same(_np(hd).reshape(want0.shape), want0)
    wtail = np.broadcast_to(wt[:, None], x5.shape).reshape(-1)[4096 * 256:]
    assert wtail.size == 2672 and (wtail == 1).sum() == wb and (wtail == 0).sum() == wb and ((wtail > 0) & (wtail < 1)).sum() == 2672 - 2 * wb
    c5 = x5.clone()
    assert _comp(c5, "f32", _keys(keys), (S, C, Fb, hw), (_p(tk), kx[0].size, 1, _p(tw), wt[0].size, Fb)) == 0
    torch.cuda.synchronize()
    assert _same(_np(c5), NZ.video_hold_composite_reference(_np(x5), kx, wt, HA, HS, keys))


# ------------------------------------------------------------------------------------------------ 2: w == 0 is the noise entry bit for bit
@pytest.mark.parametrize("dt", list(TDT))
def test_weight_zero_is_the_noise_entry_bit_for_bit(dt):
    """state and x0_prev of tmix_vpred_step_noise / _noise_dev, with cz = 0 and cz > 0, in all four forms; the held latent is NaN everywhere and is
    not looked at"""
    S = 3
    dk = _keys(VH.KEYS)
    nan = torch.full((S, C, F, HH, WW), float("nan"), device="cuda")
    zero = torch.zeros(S, F, HH, WW, device="cuda")
    hold = (_p(nan), nan[0].numel(), F, _p(zero), zero[0].numel(), F)
    iv = torch.int32 if dt == "f32" else torch.int16
    for kind in KINDS:
        for rs in (False, True):
            for cz in (0.0, CZ):
                x, v, prev, fac = _videos(S, dt, 61 + rs)
                fac = fac if rs else None
                a, b, ha_, hb_ = torch.empty_like(x), torch.empty_like(x), prev.clone(), prev.clone()
                assert _dense(kind, x, v, a, ha_, dt, fac, dk, (S, C, F, HW), hold, cz=cz) == 0
                assert _noise_dense(kind, x, v, b, hb_, dt, fac, dk, S, C * F * HW, cz=cz) == 0
                torch.cuda.synchronize()
                assert torch.equal(a.view(iv), b.view(iv)) and torch.equal(ha_, hb_) and torch.isfinite(a).all(), (dt, kind, rs, cz)
    if dt != "f32":
        return
    for layout, pad in VC.LAYOUTS:
        for kind in KINDS:
            for rs in (False, True):
                for cz in (0.0, CZ):
                    xd, pv, _frames, ptrs, _ = _dev_case(S, F, HW, layout, pad, 62)
                    fac = torch.tensor([0.41, 1.0, 0.77], device="cuda") if rs else None
                    a, b, ha_, hb_ = xd.clone(), xd.clone(), pv.clone(), pv.clone()
                    assert _rows(kind, a, ptrs, ha_, _prm(kind, cz=cz), fac, dk, (S, C, F, HW), hold) == 0
                    assert _noise_rows(kind, b, ptrs, hb_, _prm(kind, cz=cz), fac, dk, (S, C, F, HW)) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(a, b) and torch.equal(ha_, hb_) and torch.isfinite(a).all(), (layout, pad, kind, rs, cz)


# ------------------------------------------------------------------------------------------------ 3: w == 1 does not look at the prediction
@pytest.mark.parametrize("dt", list(TDT))
def test_weight_one_gives_the_held_part_whatever_the_prediction(dt):
    """v all NaN, w == 1 everywhere: the output is kept = rnd(rnd(ha kx) + rnd(hs zh)) in every frame; with hs = 0 it is kx's own bit pattern (fp32: the
    -0.0 included; fp16 / bf16: kx rounded once by the store)"""
    from tweediemix_amd import noise as NZ, solver as SV
    S = 3
    keys = VH.KEYS
    dk = _keys(keys)
    for kind in KINDS:
        for Fk in (1, F):
            x, v, prev, _fac = _videos(S, dt, 31)
            v.fill_(float("nan"))
            kx = VH.held_latent(S, Fk, 32)
            tk, one = torch.from_numpy(kx).cuda(), torch.ones(1, 1, HH, WW, device="cuda")
            hold = (_p(tk), kx[0].size, Fk, _p(one), 0, 1)
            kxb = np.ascontiguousarray(np.broadcast_to(kx, (S, C, F, HH, WW)))
            for ha, hs in ((HA, HS), (1.0, 0.0)):
                out, hist = torch.empty_like(x), prev.clone()
                assert _dense(kind, x, v, out, hist, dt, None, dk, (S, C, F, HW), hold, ha=ha, hs=hs) == 0
                torch.cuda.synchronize()
                want = NZ.video_hold_composite_reference(_np(x), kx, np.ones((1, 1, HH, WW), NF), ha, hs, keys, DT[dt][1])
                assert _same(_np(out), want) and torch.isfinite(out).all(), (dt, kind, Fk, ha, hs)
                if hs == 0.0:
                    stored = {"f32": kxb, "f16": kxb.astype(np.float16).astype(NF), "bf16": SV._bf16_round(kxb)}[dt]
                    assert _same(_np(out), stored) and np.signbit(_np(out)[(slice(None),) + VH.NEG0]).all(), (dt, kind, Fk)
                if kind != "ddim":
                    assert torch.isnan(hist).all()                       # the history is the parent's: the element's own x0
    if dt != "f32":
        return
    xd, pv, _frames, ptrs, _ = _dev_case(S, F, HW, "two", True, 33)
    for t in ptrs[0::2]:
        t.fill_(float("nan"))
    kx = VH.held_latent(S, 1, 34)
    tk, one = torch.from_numpy(kx).cuda(), torch.ones(1, 1, HH, WW, device="cuda")
    state, hist = xd.clone(), pv.clone()
    assert _rows("second", state, ptrs, hist, _prm("second", ha=1.0, hs=0.0), None, dk, (S, C, F, HW), (_p(tk), kx[0].size, 1, _p(one), 0, 1)) == 0
    torch.cuda.synchronize()
    assert _same(_np(state).reshape(S, C, F, HH, WW), np.broadcast_to(kx, (S, C, F, HH, WW)))


# ------------------------------------------------------------------------------------------------ 4: the held part's noise
def test_zero_latent_at_hs_one_gives_exactly_the_hold_noise_of_each_videos_key():
    """kx = 0, ha anything, hs = 1, w = 1: the output is noise.normal(arange(per), key_s, 0, STREAM_VIDEO_HOLD), whatever step the launch carries; it
    is not the step noise (stream 1) of the same key"""
    from tweediemix_amd import noise as NZ
    S, per = 3, C * F * HW
    zh = VH.hold_noise(per, VH.KEYS)
    dk = _keys(VH.KEYS)
    kx, one = torch.zeros(1, C, 1, HH, WW, device="cuda"), torch.ones(1, 1, HH, WW, device="cuda")
    hold = (_p(kx), 0, 1, _p(one), 0, 1)
    x, v, prev, _fac = _videos(S, "f32", 41)
    for kind in KINDS:
        for step in (0, STEP):
            out = torch.empty_like(x)
            assert _dense(kind, x, v, out, prev.clone(), "f32", None, dk, (S, C, F, HW), hold, step=step, ha=0.7, hs=1.0) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_np(out).reshape(S, per), zh), (kind, step)
    c = x.clone()
    assert _comp(c, "f32", dk, (S, C, F, HW), hold, ha=0.7, hs=1.0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(c).reshape(S, per), zh)
    idx = np.arange(per, dtype=np.uint64)
    for s, (lo, hi) in enumerate(VH.KEYS):
        assert not np.array_equal(zh[s], NZ.normal(idx, lo, hi, 0, NZ.STREAM_VIDEO_STEP)) and not np.array_equal(zh[s], NZ.normal(idx, lo, hi, STEP, NZ.STREAM_VIDEO_STEP))


# ------------------------------------------------------------------------------------------------ 5: videos, not batch slots
def test_co_batched_videos_equal_single_launches_and_keys_belong_to_videos():
    """S = 3 equals three S = 1 launches with the respective keys, held latents and weights (both entries; shared arrays too); swapping two videos'
    keys changes those two videos alone"""
    S = 3
    per = C * F * HW
    x, prev, _frames, ptrs, (eu, ec) = _dev_case(S, F, HW, "one", True, 21)
    vu, su, vc, sc = ptrs
    fac = torch.tensor([0.41, 1.0, 0.77], device="cuda")
    dv = torch.cat([_pipe(eu, S, F, C, HW), _pipe(ec, S, F, C, HW)]).contiguous()
    for mode in ("dense", "shared"):
        kx, wt, hold, (tk, tw) = _hold(S, F, F, mode, 22)
        for kind in KINDS:
            many, hm = x.clone(), prev.clone()
            assert _rows(kind, many, ptrs, hm, _prm(kind), fac, _keys(VH.KEYS), (S, C, F, HW), hold) == 0
            dmany, dh = torch.empty_like(x), prev.clone()
            assert _dense(kind, x.contiguous(), dv, dmany, dh, "f32", fac, _keys(VH.KEYS), (S, C, F, HW), hold) == 0
            torch.cuda.synchronize()
            assert torch.equal(dmany, many) and torch.equal(dh, hm)
            for s in range(S):
                k = 0 if mode == "shared" else s
                h1 = (_p(tk[k:]), kx[0].size, F, _p(tw[k:]), wt[0].size, F)
                one, p1 = x[s:s + 1].clone(), prev[s:s + 1].clone()
                assert _rows(kind, one, (vu[s:], su, vc[s:], sc), p1, _prm(kind), fac[s:s + 1].contiguous(), _keys(VH.KEYS[s:s + 1]), (1, C, F, HW), h1) == 0
                torch.cuda.synchronize()
                assert torch.equal(one, many[s:s + 1]) and torch.equal(p1, hm[s:s + 1]), (mode, kind, s)
            sw = [VH.KEYS[1], VH.KEYS[0], VH.KEYS[2]]
            swapped, hs_ = x.clone(), prev.clone()
            assert _rows(kind, swapped, ptrs, hs_, _prm(kind), fac, _keys(sw), (S, C, F, HW), hold) == 0
            torch.cuda.synchronize()
            assert torch.equal(swapped[2], many[2]) and torch.equal(hs_, hm)
            assert not torch.equal(swapped[0], many[0]) and not torch.equal(swapped[1], many[1])
            kx4, wt3 = kx.reshape(kx.shape[:3] + (HW,)), wt.reshape(wt.shape[:2] + (HW,))
            assert _same(_np(swapped), _ref(kind, _np(x), _np(dv), _np(prev), _np(fac), sw, kx4, wt3, None)[0])


# ------------------------------------------------------------------------------------------------ 6: the composite entry
@pytest.mark.parametrize("dt", list(TDT))
def test_composite_equals_the_restatement_and_the_steps_held_part(dt):
    """in place on x of the model dtype, Fk x Fw x strides, (ha, hs) of a noise level and (1, 0); where w == 1 it is what a step stores there at the
    same (ha, hs), where w == 0 it leaves x's bits"""
    from tweediemix_amd import noise as NZ
    S = 3
    keys = VH.KEYS
    dk = _keys(keys)
    iv = torch.int32 if dt == "f32" else torch.int16
    n = 0
    for Fk in (1, F):
        for Fw in (1, F):
            for mode in STRIDES:
                for ha, hs in ((HA, HS), (1.0, 0.0)):
                    n += 1
                    x, v, prev, _fac = _videos(S, dt, 500 + n)
                    kx, wt, hold, _live = _hold(S, Fk, Fw, mode, 600 + n)
                    got = x.clone()
                    assert _comp(got, dt, dk, (S, C, F, HW), hold, ha=ha, hs=hs) == 0
                    step = torch.empty_like(x)
                    assert _dense("ddim", x, v, step, None, dt, None, dk, (S, C, F, HW), hold, ha=ha, hs=hs) == 0
                    torch.cuda.synchronize()
                    what = (dt, Fk, Fw, mode, ha, hs)
                    assert _same(_np(got), NZ.video_hold_composite_reference(_np(x), kx, wt, ha, hs, keys, DT[dt][1])), what
                    wb = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(wt[:, None], (S, C, F, HH, WW)))).cuda()
                    held, free = wb == 1, wb == 0
                    assert held.any() and free.any()
                    assert torch.equal(got.view(iv)[held], step.view(iv)[held]) and torch.equal(got.view(iv)[free], x.view(iv)[free]), what


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_error_codes_without_a_launch():
    """every refusal of the three entries comes back before a launch: the outputs still hold the sentinel everywhere"""
    L, lib = _lib()
    S = 2
    per = C * F * HW
    n = S * per
    x = dense_guarded((1, n), F32, rows=8, device="cuda", name="x")
    out = dense_guarded((1, n), F32, rows=8, device="cuda", name="out")
    prev = dense_guarded((1, n), F32, rows=8, device="cuda", name="x0_prev")
    v = torch.zeros(2, n, device="cuda")
    keys, one = _keys(VH.KEYS[:S]), torch.ones(S, device="cuda")
    kx, wt = torch.zeros(S, C, F, HW, device="cuda"), torch.zeros(S, F, HW, device="cuda")
    err = lib.tmix_last_error_string
    halves = (v[0], per, v[1], per)
    shape = (S, C, F, HW)
    good = (_p(kx), C * F * HW, F, _p(wt), F * HW, F)

    def bad_holds():
        yield (None,) + good[1:], L.EINVAL, b"null hold_x0 / hold_w"
        yield good[:3] + (None,) + good[4:], L.EINVAL, b"null hold_x0 / hold_w"
        for fk in (0, 2, F + 1):
            yield good[:2] + (fk,) + good[3:], L.ESHAPE, b"hold_x0_frames="
        for fw in (0, 2, -1):
            yield good[:5] + (fw,), L.ESHAPE, b"hold_w_frames="
        for sx in (C * F * HW - 1, 1, -5):
            yield good[:1] + (sx,) + good[2:], L.ESHAPE, b"hold video strides"
        for sw in (F * HW - 1, 1, -5):
            yield good[:4] + (sw,) + good[5:], L.ESHAPE, b"hold video strides"
    for kind in KINDS:
        for fac in (None, one):
            prm = _prm(kind)
            for hold, code, msg in bad_holds():
                assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, keys, shape, hold) == code and msg in err(), (hold, err())
                assert _rows(kind, x.view, halves, prev.view, prm, fac, keys, shape, hold) == code and msg in err(), (hold, err())
            assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, None, shape, good) == L.EINVAL and b"null keys" in err()
            assert _dense(kind, None, v, out.view, prev.view, "f32", fac, keys, shape, good) == L.EINVAL and b"null" in err()
            assert _dense(kind, x.view, None, out.view, prev.view, "f32", fac, keys, shape, good) == L.EINVAL
            assert _dense(kind, x.view, v, None, prev.view, "f32", fac, keys, shape, good) == L.EINVAL
            assert _dense(kind, x.view, v, out.view, prev.view, 9, fac, keys, shape, good) == L.EINVAL and b"dtype" in err()
            assert _rows(kind, x.view, halves, prev.view, prm, fac, None, shape, good) == L.EINVAL and b"null keys" in err()
            assert _rows(kind, None, halves, prev.view, prm, fac, keys, shape, good) == L.EINVAL
            assert _rows(kind, x.view, (None, per, v[1], per), prev.view, prm, fac, keys, shape, good) == L.EINVAL
            assert _rows(kind, x.view, (v[0], per, None, per), prev.view, prm, fac, keys, shape, good) == L.EINVAL
            assert _rows(kind, x.view, halves, prev.view, None, fac, keys, shape, good) == L.EINVAL
            assert _rows(kind, x.view, (v[0], per - 1, v[1], per), prev.view, prm, fac, keys, shape, good) == L.ESHAPE and b"clip stride" in err()
            for bad in ((0, C, F, HW), (S, 0, F, HW), (S, C, 0, HW), (S, C, F, 0)):
                assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, keys, bad, good) == L.ESHAPE, bad
                assert _rows(kind, x.view, halves, prev.view, prm, fac, keys, bad, good) == L.ESHAPE, bad
    for hold, code, msg in bad_holds():
        assert _comp(x.view, "f32", keys, shape, hold) == code and msg in err(), (hold, err())
    assert _comp(None, "f32", keys, shape, good) == L.EINVAL and b"null pointer" in err()
    assert _comp(x.view, "f32", None, shape, good) == L.EINVAL and b"null keys" in err()
    assert _comp(x.view, 9, keys, shape, good) == L.EINVAL and b"dtype" in err()
    for bad in ((0, C, F, HW), (S, 0, F, HW), (S, C, 0, HW), (S, C, F, 0)):
        assert _comp(x.view, "f32", keys, bad, good) == L.ESHAPE, bad
    torch.cuda.synchronize()
    for f in (x, out, prev):                                      # nothing was launched: every buffer still holds the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ 8: the sampler on the tiny network
SEED_A, SEED_B = (9 << 32) + 4, 77
SWEEP = [(s, p, e) for s in ("ddim", "dpmpp2m") for p in (0.0, 0.7) for e in (0.0, 0.5)]
SWEEP_IDS = [f"{s}-phi{p}-eta{e}" for s, p, e in SWEEP]


def _spy_entries(monkeypatch):
    _, lib = _lib()
    calls = []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _graph_keys(ms, rs, eta, hold=True):
    tail = (("ms",) if ms else ()) + (("rs",) if rs else ()) + (("eta",) if eta else ()) + (("hold",) if hold else ())
    return [(False,) + tail, (True,) + tail]


def _tiny_hold(S, Fk, Fw, seed):
    """(x0, weight) on the tiny network's grid: x0 [S, 4, Fk, 16, 8], weight [1, Fw, 16, 8] shared by the videos"""
    return torch.from_numpy(VH.held_latent(S, Fk, seed, H, W)), torch.from_numpy(VH.weight(1, Fw, seed + 1, H, W))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver,phi,eta", SWEEP, ids=SWEEP_IDS)
def test_sampler_every_step_equals_the_restatement_chain_and_graph_equals_eager(solver, phi, eta):
    """n = 6 on the log-SNR grid at g = 9: x_T is composited at the first timestep's noise level; after EVERY step the state (and history) equals
    the restatement applied to the plan's own prediction rows with the uploaded twelve floats; slots 10 and 11 hold the written state's (ha, hs),
    (1, 0) on the last step; the final latent equals x0 in every frame wherever the weight is 1, bit for bit; graph replay equals eager, one graph
    per (inject, ..., "hold"), a step one 48-byte upload; a weight of 0 everywhere is the run without hold="""
    from tweediemix_amd import noise as NZ, ops
    ms, rs = solver != "ddim", phi > 0.0
    Wt, vids = _weights(), [_video(3)]
    kx, wt = _tiny_hold(1, 1, FR, 50)
    kw = dict(solver=solver, guidance_rescale=phi, eta=eta, noise_seeds=[SEED_A])
    smp = _sampler(Wt, vids, graphs=False, hold=(kx, wt), **kw)
    assert smp.params.numel() == 12 and smp._ring.slots.shape[1] == 12 and smp.noise_keys.dtype == torch.int32 and smp.hold_x0.is_cuda
    rec, real = [], smp._enqueue

    def spy():
        before, hist = smp.state.clone(), (smp.x0_prev.clone() if ms else None)
        real()
        torch.cuda.synchronize()
        (_xu, _tu, eu), (_xc, _tc, ec) = smp.plan.halves
        rec.append((before, hist, eu.clone(), ec.clone(), smp.params.clone(), smp.rs_factors.clone() if rs else None, smp.state.clone(),
                    smp.x0_prev.clone() if ms else None))
    smp._enqueue = spy
    eager = smp.sample(_x(vids))
    assert len(rec) == N6 and smp.graphs == {} and smp.noise_keys.tolist() == [[4, 9]]
    sch = smp.schedule
    ts = [int(t) for t in sch.timesteps]
    key = [NZ.seed_key(SEED_A)]
    first = NZ.video_hold_composite_reference(_np(_x(vids)), kx.numpy(), wt.numpy(), *ops.hold_coeffs(sch.alpha(ts[0])), key)
    assert _same(_np(rec[0][0]), first)
    pipe = lambda e: e.reshape(1, FR, 4, H, W).permute(0, 2, 1, 3, 4)
    for i, (before, hist, eu, ec, prm, fac, after, hist_after) in enumerate(rec):
        p = [float(c) for c in prm.cpu()]
        last = i == N6 - 1
        assert p[0] == float(ts[i]) and p[9] == float(i) and (p[8] > 0.0) == (eta > 0.0) and (p[6] if ms else p[5]) == 9.0, (i, p)
        assert tuple(p[10:]) == ((1.0, 0.0) if last else ops.hold_coeffs(sch.next_alpha(ts[i]))), (i, p)
        v = np.concatenate([_np(pipe(eu)), _np(pipe(ec))])
        want, want0 = NZ.vpred_hold_reference(_np(before), v, _np(hist) if ms else None, p, key, kx.numpy(), wt.numpy(), None, _np(fac) if rs else None)
        assert _same(_np(after), want), i
        if ms:
            assert _same(_np(hist_after), want0), i
    assert torch.equal(eager, rec[-1][6]) and torch.isfinite(eager).all()
    held = (wt == 1)[:, None].expand(1, 4, FR, H, W)
    assert held[0, 0].any(dim=-1).any(dim=-1).all()                          # something is held in every frame
    assert _same(_np(eager)[held.numpy()], kx.expand(1, 4, FR, H, W).numpy()[held.numpy()])
    assert np.signbit(_np(eager)[0, 0, :, 1, 1]).all()                       # the -0.0 of x0 sits in a held row and comes back as -0.0 in every frame
    gs = _sampler(Wt, vids, graphs=True, hold=(kx, wt), **kw)
    a = gs.sample(_x(vids))
    assert torch.equal(a, eager) and sorted(gs.graphs) == _graph_keys(ms, rs, eta > 0.0)
    b = gs.sample(_x(vids))                                     # every step replayed, the first one too
    assert torch.equal(b, eager) and sorted(gs.graphs) == _graph_keys(ms, rs, eta > 0.0)
    # a weight of 0 everywhere, through the same captured steps (the buffers keep their addresses): the run without the hold
    gs.set_hold(kx, torch.zeros_like(wt))
    free = gs.sample(_x(vids))
    plain = _sampler(Wt, vids, graphs=True, **(kw if eta > 0.0 else dict(kw, noise_seeds=None))).sample(_x(vids))
    assert torch.equal(free, plain) and not torch.equal(free, eager) and sorted(gs.graphs) == _graph_keys(ms, rs, eta > 0.0)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver,phi,eta", SWEEP, ids=SWEEP_IDS)
def test_two_co_batched_videos_equal_their_single_runs_and_sample_loop_equals_the_sampler(monkeypatch, solver, phi, eta):
    """S = 2 with different conditioning, x_T, seeds and held latents (a clip each, Fk = F; one weight for all frames): each video equals its own
    S = 1 run bit for bit; the host loop on the dense entry (composite, then tmix_vpred_step_hold per step and no other step entry) gives the
    device loop's bits"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt = _weights()
    vids = [_video(s) for s in (11, 12)]
    kx, wt = _tiny_hold(2, FR, 1, 60)
    kw = dict(solver=solver, guidance_rescale=phi, eta=eta)
    many = _sampler(Wt, vids, autotune=True, noise_seeds=[SEED_A, SEED_B], hold=(kx, wt), **kw).sample(_x(vids))
    held = (wt == 1)[:, None].expand(2, 4, FR, H, W).numpy()
    assert _same(_np(many)[held], kx.numpy()[held])
    for i, (v, seed) in enumerate(zip(vids, (SEED_A, SEED_B))):
        one = _sampler(Wt, [v], autotune=True, noise_seeds=[seed], hold=(kx[i:i + 1], wt), **kw).sample(_x([v]))
        assert torch.equal(many[i:i + 1], one), (i, float((many[i:i + 1] - one).abs().max()))
    monkeypatch.delenv("TMIX_FORCE_TILE")
    want = _sampler(Wt, vids[:1], graphs=False, noise_seeds=[SEED_A], hold=(kx[:1], wt), **kw).sample(_x(vids[:1]))
    calls = _spy_entries(monkeypatch)
    xT = vids[0][1].clone()
    got = _host_loop(Wt, vids[0], N6, "logsnr", 0.2, noise_seeds=[SEED_A], hold=(kx[:1], wt), **kw)
    assert calls == ["tmix_video_hold_composite"] + ((["tmix_vpred_rescale_factors"] if phi > 0.0 else []) + ["tmix_vpred_step_hold"]) * N6
    assert torch.equal(got, want) and torch.equal(vids[0][1], xT)          # the caller's x_T is not composited in place


# ------------------------------------------------------------------------------------------------ 9: hold=None is today's sampler
@pytest.mark.timeout(180)
@pytest.mark.parametrize("solver,step,key", [("ddim", "tmix_vpred_step_dev", [False, True]), ("dpmpp2m", "tmix_vpred_step_ms_dev", [(False, "ms"), (True, "ms")])],
                         ids=["ddim", "dpmpp2m"])
def test_hold_none_is_the_sampler_of_today(monkeypatch, solver, step, key):
    """hold=None spelled out equals the call without it: the same bits, entry calls, graph keys and upload sizes (32 bytes; 48 with eta > 0, slots 10
    and 11 zero), no hold buffers; sample_loop likewise.  With a hold the step goes through the hold entry alone"""
    Wt, vid = _weights(), _video(5)
    calls = _spy_entries(monkeypatch)
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(hold=None), dict(hold=None, noise_seeds=[SEED_A])):
            smp = _sampler(Wt, [vid], graphs=graphs, solver=solver, **kw)
            out = smp.sample(_x([vid]))
            runs.append((out, list(calls), smp))
            calls[:] = []
    for base, others in ((runs[0], runs[1:3]), (runs[3], runs[4:6])):
        for ob, cb, sb in others:
            assert torch.equal(base[0], ob) and base[1] == cb and sorted(base[2].graphs) == sorted(sb.graphs)
            assert sb.hold_x0 is None and sb.hold_w is None and sb.noise_keys is None and sb.params.numel() == 8 and sb._ring.slots.shape[1] == 8
            assert not any(c in HOLD_ENTRIES for c in cb)
    assert runs[1][1] == ["tmix_video_step_prologue", step] * N6 and sorted(runs[4][2].graphs) == key
    a = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver)
    assert calls == [step[:-4]] * N6
    calls[:] = []
    b = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver, hold=None, noise_seeds=[SEED_A])
    assert calls == [step[:-4]] * N6 and torch.equal(a, b) and torch.equal(a, runs[0][0])
    calls[:] = []
    ne = _sampler(Wt, [vid], graphs=True, solver=solver, eta=0.5, noise_seeds=[SEED_A], hold=None)
    ne.sample(_x([vid]))
    tail = (("ms",) if solver != "ddim" else ()) + ("eta",)
    assert sorted(ne.graphs) == [(False,) + tail, (True,) + tail] and ne.params.numel() == 12 and ne.params[10:].tolist() == [0.0, 0.0] and ne.hold_x0 is None
    assert set(calls) == {"tmix_video_step_prologue", "tmix_vpred_step_noise_dev"}
    calls[:] = []
    kx, wt = _tiny_hold(1, 1, 1, 70)
    hd = _sampler(Wt, [vid], graphs=False, solver=solver, noise_seeds=[SEED_A], hold=(kx, wt)).sample(_x([vid]))
    assert calls == ["tmix_video_hold_composite"] + ["tmix_video_step_prologue", "tmix_vpred_step_hold_dev"] * N6
    assert torch.isfinite(hd).all() and not torch.equal(hd, runs[0][0])


# ------------------------------------------------------------------------------------------------ 10: CLI
@pytest.mark.timeout(180)
def test_cli_holds_the_masked_region_in_every_frame(tmp_path, monkeypatch):
    """run_video.py --tiny --synthetic --hold_masks a.png+b.png: inside the masks' union every frame of the latent is the same picture (frame 0 of
    the video's conditional image latents, also for the second seed) and the weight is written as <stem>_hold.png; --animate_masks holds the
    complement; --hold_latents with the first run's clip gives that clip back inside the union, frame by frame, and another result outside"""
    from PIL import Image
    from tweediemix_amd import i2vgen as I
    spec = importlib.util.spec_from_file_location("rv_hold_gpu", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    a, b = VH.write_masks(tmp_path, 128, 64)
    union = torch.from_numpy(VH.latent_union(16, 8))
    calls = _spy_entries(monkeypatch)
    common = ["--synthetic", "--tiny", "--height", "128", "--width", "64", "--num_inference_steps", "6", "--injection_timestep", "0.2", "--seed", "4"]
    lat = rv.main(common + ["--num_seeds", "2", "--hold_masks", f"{a}+{b}", "--output_dir", str(tmp_path / "a")]).cpu()
    assert set(calls) == {"tmix_video_hold_composite", "tmix_video_step_prologue", "tmix_vpred_step_hold_dev"}
    assert lat.shape == (2, 4, 16, 16, 8) and torch.isfinite(lat).all() and not torch.equal(lat[0], lat[1])
    for i, seed in enumerate((4, 5)):
        assert torch.equal(torch.load(tmp_path / "a" / f"output_i2v_seed_{seed}.latent.pt"), lat[i:i + 1])
        png = np.asarray(Image.open(tmp_path / "a" / f"output_i2v_seed_{seed}_hold.png"))
        assert png.shape == (16, 8) and np.array_equal(png == 255, union.numpy()) and np.array_equal(png == 0, ~union.numpy())
        inside, outside = lat[i][:, :, union], lat[i][:, :, ~union]            # [4, 16, pixels]
        assert torch.equal(inside, inside[:, :1].expand_as(inside))             # every frame is frame 0 there ...
        assert not torch.equal(outside, outside[:, :1].expand_as(outside))      # ... and moves elsewhere
        g = torch.Generator().manual_seed(seed)                                 # the synthetic conditioning of that seed: its conditional row, frame 0
        il = rv.synthetic_conditioning(I.TINY, g, 16, 16, 8)["image_latents"]
        assert torch.equal(inside[:, 0], il[1, :, 0][:, union])
    plain = rv.main(common + ["--output_dir", str(tmp_path / "plain")]).cpu()
    assert not torch.equal(plain, lat[:1])
    moved = rv.main(common + ["--animate_masks", f"{a}+{b}", "--output_dir", str(tmp_path / "m")]).cpu()
    out_ = moved[0][:, :, ~union]
    assert torch.equal(out_, out_[:, :1].expand_as(out_)) and not torch.equal(moved[0][:, :, union], moved[0][:, :, union][:, :1].expand(4, 16, -1))
    clip = str(tmp_path / "plain" / "output_i2v_seed_4.latent.pt")
    re_ = rv.main(common + ["--hold_masks", a, "--hold_latents", clip, "--eta", "0.5", "--solver", "dpmpp2m", "--timestep_spacing", "logsnr",
                            "--output_dir", str(tmp_path / "r")]).cpu()
    ua = torch.zeros(16, 8, dtype=torch.bool)
    ua[1:5, 1:3] = True
    assert torch.equal(re_[0][:, :, ua], plain[0][:, :, ua]) and not torch.equal(re_[0][:, :, ~ua], plain[0][:, :, ~ua])
    soft = rv.main(common + ["--hold_masks", a, "--hold_feather", "16", "--hold_dilate", "8", "--output_dir", str(tmp_path / "s")]).cpu()
    png = np.asarray(Image.open(tmp_path / "s" / "output_i2v_seed_4_hold.png"))
    assert ((png > 0) & (png < 255)).any() and (png[ua.numpy()] == 255).all() and torch.isfinite(soft).all()
