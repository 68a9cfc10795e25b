"""GPU: stochastic sampling of the VIDEO sampler -- tmix_vpred_step_noise / tmix_vpred_step_noise_dev, sample_loop(eta=...),
VideoSampler(eta=..., noise_seeds=...), run_video.py --eta.

Both entries are compared with tweediemix_amd.noise.vpred_step_reference by equality: the generator, the parents' moves and the one product and one
sum behind them are the same single-rounded fp32 (fp16) operations on both sides.  The end-to-end variance is compared with the closed-form
recursion of tests/video_noise_cases.py, never with the code under test."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import video_noise_cases as VN
import video_rescale_cases as VC
from layout_frames import Frame, _wrap, dense_guarded
from test_video_solver_gpu import AT, DT, FR, G, H, N6, ORDERS, S1, SA, W, _dev_case, _host_loop, _pipe, _sampler, _video, _weights, _x
from video_solver_cases import standin_schedule, toy_v

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SAN, S1D = float(NF(0.53582)), float(NF(0.78125))                # a DDIM move's (sa_next, s1_dir): s1_dir < sqrt(1 - sa_next^2), the rest went to cz
KINDS = ("ddim", "first", "second")
CZ, STEP = VN.CZ, VN.STEP
PARENTS = ("tmix_vpred_step", "tmix_vpred_step_dev", "tmix_vpred_step_ms", "tmix_vpred_step_ms_dev", "tmix_vpred_step_rs", "tmix_vpred_step_rs_dev",
           "tmix_vpred_step_ms_rs", "tmix_vpred_step_ms_rs_dev")
NOISE_ENTRIES = ("tmix_vpred_step_noise", "tmix_vpred_step_noise_dev")
ENTRIES = PARENTS + ("tmix_video_step_prologue", "tmix_vpred_rescale_factors") + NOISE_ENTRIES


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


def _keys(keys):
    """[(low, high), ...] -> the device array int32 [S, 2]"""
    return torch.from_numpy(np.array(keys, dtype=np.uint32).view(np.int32).reshape(-1, 2).copy()).cuda()


def _move(kind):
    return (SAN, S1D, 0.0) if kind == "ddim" else ORDERS[kind]


def _dense(kind, x, v, out, prev, dt, fac, keys, S, n, cz=CZ, step=STEP, g=G):
    """raw ABI call of tmix_vpred_step_noise -> the code; kind "ddim": no history buffer is passed"""
    _, lib = _lib()
    d = _dtc(dt) if isinstance(dt, str) else dt
    return lib.tmix_vpred_step_noise(_p(x), _p(v), _p(out), None if kind == "ddim" else _p(prev), d, S, n, float(g), float(SA), float(S1), *_move(kind),
                                     float(cz), _p(fac), _p(keys), step, _st())


def _prm(kind, cz=CZ, step=STEP, t=501.0):
    head = [t, SA, S1, SAN, S1D, G, 0.0, 0.0] if kind == "ddim" else [t, SA, S1, *ORDERS[kind], G, 0.0]
    return torch.tensor(head + [cz, float(step), 0.0, 0.0], dtype=F32).cuda()


def _rows(kind, x, ptrs, prev, prm, fac, keys, S, C, F, hw):
    """raw ABI call of tmix_vpred_step_noise_dev -> the code"""
    _, lib = _lib()
    vu, su, vc, sc = ptrs
    return lib.tmix_vpred_step_noise_dev(_p(x), _p(vu), su, _p(vc), sc, _p(prm), S, C, F, hw, None if kind == "ddim" else _p(prev), _p(fac), _p(keys), _st())


def _ref(kind, x, v, prev, fac, keys, lowp, cz=CZ, step=STEP):
    """numpy: x [B, ...], v [2B, ...], prev [B, ...], fac [B] or None -> (out, x0)"""
    from tweediemix_amd import noise as NZ
    return NZ.vpred_step_reference(x, v, None if kind == "ddim" else prev, (G, SA, S1, *_move(kind), cz), keys, step, fac, lowp)


def _videos(B, n, dt, seed):
    """-> x [B, n], v [2B, n] of the dtype, prev [B, n] fp32, fac [B] in (0.3, 1)"""
    tdt = TDT[dt]
    rng = np.random.RandomState(seed)
    x = torch.from_numpy(rng.randn(B, n).astype(NF)).to(tdt).cuda()
    v = torch.from_numpy(rng.randn(2 * B, n).astype(NF)).to(tdt).cuda()
    prev = torch.from_numpy(rng.randn(B, n).astype(NF)).cuda()
    fac = torch.from_numpy((0.3 + 0.7 * rng.rand(B)).astype(NF)).cuda()
    return x, v, prev, fac


def _np(t):
    return t.float().cpu().numpy()


# ------------------------------------------------------------------------------------------------ both entries == the restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 4099])
@pytest.mark.parametrize("dt", list(TDT))
def test_dense_entry_equals_the_restatement(dt, n, B):
    """per-video n = 1, 255 (under one workgroup), 4099 (a ragged last workgroup; with B = 3 a video boundary inside a workgroup) x the DDIM move, a
    first-order and a second-order solver move x with and without factors: output and history by equality; every video drew from its own key"""
    keys = VN.KEYS[:B]
    for kind in KINDS:
        for rs in (False, True):
            x, v, prev, fac = _videos(B, n, dt, 10 * n + B + len(kind) + rs)
            fac = fac if rs else None
            out, hist = torch.empty_like(x), prev.clone()
            assert _dense(kind, x, v, out, hist, dt, fac, _keys(keys), B, n) == 0
            torch.cuda.synchronize()
            want, want0 = _ref(kind, _np(x), _np(v), _np(prev), None if fac is None else _np(fac), keys, DT[dt][1])
            what = (dt, kind, rs, n, B)
            assert np.array_equal(_np(out), want), what
            assert np.array_equal(_np(hist), _np(prev) if kind == "ddim" else want0), what
            base, _ = _ref(kind, _np(x), _np(v), _np(prev), None if fac is None else _np(fac), keys, DT[dt][1], cz=0.0)
            if n > 1:                                            # ... and the noise did enter, in every video
                assert all(not np.array_equal(base[b], want[b]) for b in range(B)), what


@pytest.mark.parametrize("shape", VC.SHAPES[:4], ids=lambda s: f"F{s[0]}hw{s[1]}")
@pytest.mark.parametrize("S", [1, 3])
def test_rows_entry_equals_the_restatement(S, shape):
    """(two half buffers | one buffer of 2S clips) x (dense | padded clip stride, NaN in the padding) x the four parents (DDIM | second-order move,
    with | without factors): state and history equal the restatement on the pipeline layout; state and history sit in guard-band frames; the
    prediction rows, their padding, the parameters, the factors and the keys stay untouched"""
    F, hw = shape
    C = 4
    keys = VN.KEYS[:S]
    for i, (layout, pad) in enumerate(VC.LAYOUTS):
        for kind in ("ddim", "second"):
            for rs in (False, True):
                x, prev, frames, ptrs, (eu, ec) = _dev_case(S, F, hw, layout, pad, 300 * S + F + hw + i)
                fac = torch.from_numpy((0.3 + 0.7 * np.random.RandomState(i + S).rand(S)).astype(NF)).cuda() if rs else None
                v = torch.cat([_pipe(eu, S, F, C, hw), _pipe(ec, S, F, C, hw)])
                want, want0 = _ref(kind, _np(x), _np(v), _np(prev), None if fac is None else _np(fac), keys, None)
                xf = dense_guarded((S * C * F, hw), F32, rows=8, device="cuda", name="x")
                xf.view.copy_(x.reshape(S * C * F, hw))
                hf = Frame.of(prev.reshape(S * C * F, hw), name="x0_prev")
                kf = Frame.of(_keys(keys), name="keys").seal()
                prm = Frame.of(_prm(kind).reshape(1, 12), name="params").seal()
                sealed = frames + (kf, prm)
                if rs:
                    ff = Frame.of(fac.reshape(1, S), name="factors").seal()
                    sealed += (ff,)
                if kind == "ddim":
                    hf.seal()
                assert _rows(kind, xf.view, ptrs, hf.view, prm.view, ff.view if rs else None, kf.view, S, C, F, hw) == 0
                torch.cuda.synchronize()
                xf.assert_untouched()
                xf.assert_all_written()
                hf.assert_unchanged() if kind == "ddim" else hf.assert_untouched()
                for f in sealed:
                    f.assert_unchanged()
                what = (S, F, hw, layout, pad, kind, rs)
                assert np.array_equal(_np(xf.view).reshape(want.shape), want), what
                if kind != "ddim":
                    assert np.array_equal(_np(hf.view).reshape(want0.shape), want0), what


# ------------------------------------------------------------------------------------------------ cz == 0: the eight parents bit for bit
def _parent_dense(kind, rs, x, v, out, prev, dt, fac, B, n):
    _, lib = _lib()
    mv = (SAN, S1D) if kind == "ddim" else ORDERS[kind]
    pv = () if kind == "ddim" else (_p(prev),)
    name = "tmix_vpred_step" + ("" if kind == "ddim" else "_ms") + ("_rs" if rs else "")
    shape, fa = ((B, n), (_p(fac),)) if rs else ((B * n,), ())
    return getattr(lib, name)(_p(x), _p(v), _p(out), *pv, _dtc(dt), *shape, float(G), float(SA), float(S1), *mv, *fa, _st())


def _parent_rows(kind, rs, x, ptrs, prev, prm, fac, S, C, F, hw):
    _, lib = _lib()
    vu, su, vc, sc = ptrs
    pv = () if kind == "ddim" else (_p(prev),)
    name = "tmix_vpred_step" + ("" if kind == "ddim" else "_ms") + ("_rs" if rs else "") + "_dev"
    return getattr(lib, name)(_p(x), _p(vu), su, _p(vc), sc, *pv, _p(prm), S, C, F, hw, *((_p(fac),) if rs else ()), _st())


@pytest.mark.parametrize("dt", list(TDT))
def test_cz_zero_is_the_parent_entry_bit_for_bit(dt):
    """all eight parents: output, history and what lies around them (guard bands, poisoned padding of the plan rows); with cz == 0 no key is read
    for a value (the keys hold a pattern that would show)"""
    B, n = 3, 4099
    keys = _keys(VN.KEYS)
    for kind in KINDS:
        for rs in (False, True):
            x, v, prev, fac = _videos(B, n, dt, 61 + rs)
            a, b = dense_guarded((B, n), TDT[dt], rows=8, device="cuda", name="out"), torch.empty_like(x)
            ha, hb = Frame.of(prev.clone(), name="x0_prev"), prev.clone()
            if kind == "ddim":
                ha.seal()
            assert _dense(kind, x, v, a.view, ha.view, dt, fac if rs else None, keys, B, n, cz=0.0) == 0
            assert _parent_dense(kind, rs, x, v, b, hb, dt, fac, B, n) == 0
            torch.cuda.synchronize()
            a.assert_untouched()
            a.assert_all_written()
            ha.assert_unchanged() if kind == "ddim" else ha.assert_untouched()
            assert torch.equal(a.view, b) and torch.equal(ha.view, hb), (dt, kind, rs)
    if dt != "f32":
        return
    S, C, F, hw = 3, 4, 2, 2051
    for layout, pad in VC.LAYOUTS:
        for kind in KINDS:
            for rs in (False, True):
                xd, pv, frames, ptrs, _ = _dev_case(S, F, hw, layout, pad, 62)
                fac = torch.tensor([0.41, 1.0, 0.77], device="cuda")
                a = dense_guarded((S * C * F, hw), F32, rows=8, device="cuda", name="x")
                a.view.copy_(xd.reshape(S * C * F, hw))
                ha, b, hb = Frame.of(pv.reshape(S * C * F, hw).clone(), name="x0_prev"), xd.clone(), pv.clone()
                if kind == "ddim":
                    ha.seal()
                prm = _prm(kind, cz=0.0)
                assert _rows(kind, a.view, ptrs, ha.view, prm, fac if rs else None, keys, S, C, F, hw) == 0
                assert _parent_rows(kind, rs, b, ptrs, hb, prm, fac, S, C, F, hw) == 0
                torch.cuda.synchronize()
                a.assert_untouched()
                a.assert_all_written()
                ha.assert_unchanged() if kind == "ddim" else ha.assert_untouched()
                for f in frames:
                    f.assert_unchanged()
                what = (layout, pad, kind, rs)
                assert torch.equal(a.view.reshape(b.shape), b) and torch.equal(ha.view.reshape(hb.shape), hb) and torch.isfinite(b).all(), what


# ------------------------------------------------------------------------------------------------ the noise itself
@pytest.mark.parametrize("dt", list(TDT))
def test_zero_input_gives_exactly_cz_z_of_each_videos_key(dt):
    """x = v = 0, history 0: every move is 0 and the output is rnd(cz z), z = noise.normal(arange(per), key_s, step, STREAM_VIDEO_STEP); the rows
    entry too (f32), for every layout"""
    from tweediemix_amd import solver as SV
    B, per = 3, 4 * 2 * 35
    z = VN.video_noise(per, VN.KEYS, STEP)
    prod = (NF(CZ) * z).astype(NF)
    want = {"f32": prod, "f16": prod.astype(np.float16).astype(NF), "bf16": SV._bf16_round(prod)}[dt]
    keys = _keys(VN.KEYS)
    for kind in KINDS:
        x, v, hist = torch.zeros(B, per, dtype=TDT[dt], device="cuda"), torch.zeros(2 * B, per, dtype=TDT[dt], device="cuda"), torch.zeros(B, per, device="cuda")
        out = torch.empty_like(x)
        assert _dense(kind, x, v, out, hist, dt, None, keys, B, per) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_np(out), want) and not hist.any(), (dt, kind)
    if dt != "f32":
        return
    S, C, F, hw = 3, 4, 2, 35
    for layout, pad in VC.LAYOUTS:
        _x0, _pv, _frames, ptrs, (eu, ec) = _dev_case(S, F, hw, layout, pad, 5)
        for t in ptrs[0::2]:
            t.zero_()                                            # the halves' rows (the padding keeps its NaN)
        for kind in ("ddim", "second"):
            x, hist = torch.zeros(S, C, F, hw, device="cuda"), torch.zeros(S, C, F, hw, device="cuda")
            assert _rows(kind, x, ptrs, hist, _prm(kind), None, keys, S, C, F, hw) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_np(x).reshape(S, per), prod) and not hist.any(), (layout, pad, kind)


def test_second_pass_of_the_grid_stride_loop():
    """one video of 4 x 16 x 16400 = 1,049,600 elements > 4096 workgroups x 256 threads: threads of the capped grid take a second element, whose
    noise index is its own; both entries, by equality"""
    from tweediemix_amd import ops
    S, C, F, hw = 1, 4, 16, 16400
    assert 4096 * 256 < S * C * F * hw
    keys = VN.KEYS[1:2]
    x, prev, _frames, _ptrs, (eu, ec) = _dev_case(S, F, hw, "two", False, 9)
    v = torch.cat([_pipe(eu, S, F, C, hw), _pipe(ec, S, F, C, hw)]).contiguous()
    fac = torch.tensor([0.6180339], device="cuda")
    want, want0 = _ref("second", _np(x), _np(v), _np(prev), _np(fac), keys, None)
    x5, h5 = x.clone().view(S, C, F, 1, hw), prev.clone().view(S, C, F, 1, hw)
    got = ops.vpred_step_noise_dev(x5, eu.view(S * F, C, 1, hw), ec.view(S * F, C, 1, hw), _prm("second"), _keys(keys), x0_prev=h5, factors=fac)
    torch.cuda.synchronize()
    assert got is x5 and np.array_equal(_np(x5).reshape(want.shape), want) and np.array_equal(_np(h5).reshape(want0.shape), want0)
    hd = prev.clone()
    out = ops.vpred_step_noise(x, v, G, AT, ORDERS["second"], CZ, _keys(keys), STEP, x0_prev=hd, factors=fac)
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), want) and np.array_equal(_np(hd), want0)
    tail = want[0].reshape(-1)[4096 * 256:] - _ref("second", _np(x), _np(v), _np(prev), _np(fac), keys, None, cz=0.0)[0].reshape(-1)[4096 * 256:]
    assert np.count_nonzero(tail) > 1000                        # the second pass took noise


def test_co_batched_videos_equal_single_launches_and_keys_belong_to_videos():
    """S = 3 equals three S = 1 launches with the respective keys (both entries); swapping two videos' keys swaps only their noise"""
    S, C, F, hw = 3, 4, 2, 2051
    per = C * F * hw
    x, prev, _frames, ptrs, (eu, ec) = _dev_case(S, F, hw, "one", True, 21)
    vu, su, vc, sc = ptrs
    fac = torch.tensor([0.41, 1.0, 0.77], device="cuda")
    for kind in ("ddim", "second"):
        many, hm = x.clone(), prev.clone()
        assert _rows(kind, many, ptrs, hm, _prm(kind), fac, _keys(VN.KEYS), S, C, F, hw) == 0
        dx = x.reshape(S, per).contiguous()
        dv = torch.cat([_pipe(eu, S, F, C, hw), _pipe(ec, S, F, C, hw)]).reshape(2 * S, per).contiguous()
        dmany, dh = torch.empty_like(dx), prev.reshape(S, per).clone()
        assert _dense(kind, dx, dv, dmany, dh, "f32", fac, _keys(VN.KEYS), S, per) == 0
        for s in range(S):
            one, h1 = x[s:s + 1].clone(), prev[s:s + 1].clone()
            assert _rows(kind, one, (vu[s:], su, vc[s:], sc), h1, _prm(kind), fac[s:s + 1].contiguous(), _keys(VN.KEYS[s:s + 1]), 1, C, F, hw) == 0
            torch.cuda.synchronize()
            assert torch.equal(one, many[s:s + 1]) and torch.equal(h1, hm[s:s + 1]), (kind, s)
            d1 = torch.empty(1, per, device="cuda")
            hd1 = prev[s].reshape(1, per).clone()
            v1 = torch.stack([dv[s], dv[S + s]]).contiguous()
            assert _dense(kind, dx[s:s + 1].contiguous(), v1, d1, hd1, "f32", fac[s:s + 1].contiguous(), _keys(VN.KEYS[s:s + 1]), 1, per) == 0
            torch.cuda.synchronize()
            assert torch.equal(d1, dmany[s:s + 1]) and torch.equal(d1.reshape(one.shape), one), (kind, s)
        swapped, hs = x.clone(), prev.clone()
        sw = [VN.KEYS[1], VN.KEYS[0], VN.KEYS[2]]
        assert _rows(kind, swapped, ptrs, hs, _prm(kind), fac, _keys(sw), S, C, F, hw) == 0
        torch.cuda.synchronize()
        assert torch.equal(swapped[2], many[2]) and torch.equal(hs, hm)
        assert not torch.equal(swapped[0], many[0]) and not torch.equal(swapped[1], many[1])
        v = torch.cat([_pipe(eu, S, F, C, hw), _pipe(ec, S, F, C, hw)])
        assert np.array_equal(_np(swapped), _ref(kind, _np(x), _np(v), _np(prev), _np(fac), sw, None)[0])
    # on a zero input the swap is visible as such: video 0 now holds video 1's noise and the other way round
    z0 = torch.zeros(S, per, device="cuda")
    a, b = torch.empty_like(z0), torch.empty_like(z0)
    assert _dense("ddim", z0, torch.zeros(2 * S, per, device="cuda"), a, None, "f32", None, _keys(VN.KEYS), S, per) == 0
    assert _dense("ddim", z0, torch.zeros(2 * S, per, device="cuda"), b, None, "f32", None, _keys(sw), S, per) == 0
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[0], a[1])


@pytest.mark.parametrize("dt", list(TDT))
def test_in_place_equals_out_of_place(dt):
    B, n = 3, 4099
    keys = _keys(VN.KEYS)
    for kind in KINDS:
        x, v, prev, fac = _videos(B, n, dt, 71)
        out, h1, xin, h2 = torch.empty_like(x), prev.clone(), x.clone(), prev.clone()
        assert _dense(kind, x, v, out, h1, dt, fac, keys, B, n) == 0
        assert _dense(kind, xin, v, xin, h2, dt, fac, keys, B, n) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, xin) and torch.equal(h1, h2) and not torch.equal(out, x), (dt, kind)


def test_rows_entry_reads_cz_and_the_step_index_from_the_uploaded_parameters():
    """the graph-replay property at kernel level: the SAME launch (same pointers, same arguments) after another upload into params[8] / params[9]
    gives the other step's noise at the other cz"""
    S, C, F, hw = 3, 4, 2, 35
    x, prev, _frames, ptrs, (eu, ec) = _dev_case(S, F, hw, "two", True, 31)
    v = torch.cat([_pipe(eu, S, F, C, hw), _pipe(ec, S, F, C, hw)])
    keys = _keys(VN.KEYS)
    for kind in ("ddim", "second"):
        prm = _prm(kind)
        state, hist = torch.empty_like(x), torch.empty_like(prev)
        outs = {}
        for cz, step in ((CZ, STEP), (CZ, 19), (0.0625, STEP), (0.0, 3), (CZ, 2 ** 24 - 1)):
            prm.copy_(_prm(kind, cz=cz, step=step))
            state.copy_(x)
            hist.copy_(prev)
            assert _rows(kind, state, ptrs, hist, prm, None, keys, S, C, F, hw) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_np(state), _ref(kind, _np(x), _np(v), _np(prev), None, VN.KEYS, None, cz=cz, step=step)[0]), (kind, cz, step)
            outs[(cz, step)] = state.clone()
        assert len({o.cpu().numpy().tobytes() for o in outs.values()}) == 5


def test_error_codes_without_a_launch():
    """both entries in all four forms: every refusal comes back before a launch -- the outputs still hold the sentinel everywhere"""
    L, lib = _lib()
    S, C, F, hw = 2, 4, 2, 35
    clip = C * F * hw
    n = S * clip
    x = dense_guarded((1, n), F32, rows=8, device="cuda", name="x")
    out = dense_guarded((1, n), F32, rows=8, device="cuda", name="out")
    prev = dense_guarded((1, n), F32, rows=8, device="cuda", name="x0_prev")
    v = torch.zeros(2, n, device="cuda")
    keys, one = _keys(VN.KEYS[:S]), torch.ones(S, device="cuda")
    err = lib.tmix_last_error_string
    halves = (v[0], clip, v[1], clip)
    for kind in ("ddim", "second"):
        for fac in (None, one):
            assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, None, S, clip) == L.EINVAL and b"null keys" in err()
            assert _dense(kind, None, v, out.view, prev.view, "f32", fac, keys, S, clip) == L.EINVAL and b"null" in err()
            assert _dense(kind, x.view, None, out.view, prev.view, "f32", fac, keys, S, clip) == L.EINVAL
            assert _dense(kind, x.view, v, None, prev.view, "f32", fac, keys, S, clip) == L.EINVAL
            assert _dense(kind, x.view, v, out.view, prev.view, 9, fac, keys, S, clip) == L.EINVAL and b"dtype" in err()
            assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, keys, 0, clip) == L.ESHAPE
            assert _dense(kind, x.view, v, out.view, prev.view, "f32", fac, keys, S, 0) == L.ESHAPE
            prm = _prm(kind)
            assert _rows(kind, x.view, halves, prev.view, prm, fac, None, S, C, F, hw) == L.EINVAL and b"null keys" in err()
            assert _rows(kind, None, halves, prev.view, prm, fac, keys, S, C, F, hw) == L.EINVAL
            assert _rows(kind, x.view, (None, clip, v[1], clip), prev.view, prm, fac, keys, S, C, F, hw) == L.EINVAL
            assert _rows(kind, x.view, (v[0], clip, None, clip), prev.view, prm, fac, keys, S, C, F, hw) == L.EINVAL
            assert _rows(kind, x.view, halves, prev.view, None, fac, keys, S, C, F, hw) == L.EINVAL
            assert _rows(kind, x.view, (v[0], clip - 1, v[1], clip), prev.view, prm, fac, keys, S, C, F, hw) == L.ESHAPE and b"clip stride" in err()
            assert _rows(kind, x.view, (v[0], clip, v[1], clip - 1), prev.view, prm, fac, keys, S, C, F, hw) == L.ESHAPE
            for bad in ((0, C, F, hw), (S, 0, F, hw), (S, C, 0, hw), (S, C, F, 0)):
                assert _rows(kind, x.view, halves, prev.view, prm, fac, keys, *bad) == L.ESHAPE, bad
    torch.cuda.synchronize()
    for f in (x, out, prev):                                      # nothing was launched: every buffer still holds the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ the sampler on the tiny network
ETA = 0.6
SEED_A, SEED_B = (9 << 32) + 4, 77


def _spy_entries(monkeypatch):
    """test_video_solver_gpu._spy_entries over every step entry, the rescale's and the two new ones included"""
    _, lib = _lib()
    calls = []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _graph_keys(ms, rs):
    tail = (("ms",) if ms else ()) + (("rs",) if rs else ()) + ("eta",)
    return [(False,) + tail, (True,) + tail]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_sampler_every_step_equals_the_restatement_and_graph_equals_eager(solver, phi):
    """n = 6 on the log-SNR grid at g = 9, eta = 0.6: after EVERY step the state (and history) equals the restatement applied to the plan's own
    prediction rows with the uploaded twelve floats (and the device's own rescale factor); the uploaded step index is the schedule index, cz > 0 at
    every step, the last one included, and under dpmpp2m the first step is a first-order SOLVER step; graph replay equals eager, one graph per
    (inject, ["ms",] ["rs",] "eta"), a step one 48-byte upload"""
    from tweediemix_amd import noise as NZ, solver as SV
    ms, rs = solver != "ddim", phi > 0.0
    Wt, vids = _weights(), [_video(3)]
    smp = _sampler(Wt, vids, graphs=False, solver=solver, guidance_rescale=phi, eta=ETA, noise_seeds=[SEED_A])
    assert smp.eta == ETA and smp.params.numel() == 12 and smp._ring.slots.shape[1] == 12 and smp.noise_keys.dtype == torch.int32
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
    pipe = lambda e: e.reshape(1, FR, 4, H, W).permute(0, 2, 1, 3, 4)
    for i, (before, hist, eu, ec, prm, fac, after, hist_after) in enumerate(rec):
        p = [float(c) for c in prm.cpu()]
        a, an, ap = sch.alpha(ts[i]), sch.next_alpha(ts[i]), sch.alpha(ts[i - 1]) if i else None
        assert p[0] == float(ts[i]) and p[9] == float(i) and p[8] > 0.0 and p[10:] == [0.0, 0.0] and (p[6] if ms else p[5]) == 9.0, (i, p)
        if ms:
            assert tuple(p[3:6]) + (p[8],) == SV.multistep_eta_coeffs(ap, a, an, i > 0, ETA) and (p[5] == 0.0) == (i == 0), (i, p)
        else:
            assert (p[1], p[2], p[3], p[4], p[8]) == SV.ddim_eta_coeffs(a, an, ETA), (i, p)
        v = np.concatenate([_np(pipe(eu)), _np(pipe(ec))])
        want, want0 = NZ.vpred_step_reference(_np(before), v, _np(hist) if ms else None, p, [NZ.seed_key(SEED_A)], None, _np(fac) if rs else None)
        assert np.array_equal(_np(after), want), i
        if ms:
            assert np.array_equal(_np(hist_after), want0), i
        quiet, _ = NZ.vpred_step_reference(_np(before), v, _np(hist) if ms else None, p[:8] + [0.0] * 4, [NZ.seed_key(SEED_A)], None, _np(fac) if rs else None)
        assert not np.array_equal(quiet, want), i
    assert torch.equal(eager, rec[-1][6]) and torch.isfinite(eager).all()
    gs = _sampler(Wt, vids, graphs=True, solver=solver, guidance_rescale=phi, eta=ETA, noise_seeds=[SEED_A])
    a = gs.sample(_x(vids))
    assert torch.equal(a, eager) and sorted(gs.graphs) == _graph_keys(ms, rs)
    b = gs.sample(_x(vids))                                     # every step replayed, the first one too
    assert torch.equal(b, eager) and sorted(gs.graphs) == _graph_keys(ms, rs)
    gs.set_noise_seeds([SEED_B])                                # the captured steps read the keys at their fixed address
    c = gs.sample(_x(vids))
    assert sorted(gs.graphs) == _graph_keys(ms, rs) and gs.noise_keys.tolist() == [[SEED_B, 0]] and not torch.equal(c, eager)
    smp._enqueue = real
    smp.set_noise_seeds([SEED_B])
    assert torch.equal(smp.sample(_x(vids)), c)
    with pytest.raises(ValueError, match="2 values for 1 videos"):
        gs.set_noise_seeds([1, 2])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_two_co_batched_videos_equal_their_single_runs(monkeypatch, solver):
    """S = 2 with different conditioning, x_T and noise seeds: each video equals its own S = 1 run bit for bit (one tiling everywhere, as in
    tests/test_video_batch_gpu.py): a video's noise is a function of its own seed, not of its place in the batch; with the rescale on as well"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt = _weights()
    vids = [_video(s) for s in (11, 12)]
    kw = dict(solver=solver, guidance_rescale=0.7, eta=ETA)
    many = _sampler(Wt, vids, autotune=True, noise_seeds=[SEED_A, SEED_B], **kw).sample(_x(vids))
    for i, (v, seed) in enumerate(zip(vids, (SEED_A, SEED_B))):
        one = _sampler(Wt, [v], autotune=True, noise_seeds=[seed], **kw).sample(_x([v]))
        assert torch.equal(many[i:i + 1], one), (i, float((many[i:i + 1] - one).abs().max()))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_sample_loop_with_eta_equals_the_sampler(monkeypatch, solver, phi):
    """one video, F32: the host loop on the dense entry gives the device loop's bits; its steps go through tmix_vpred_step_noise (behind the factors
    entry with the rescale on) and no other step entry; the same seeds twice give the same bits, another seed another result"""
    Wt, vid = _weights(), _video(3)
    kw = dict(solver=solver, guidance_rescale=phi, eta=ETA)
    want = _sampler(Wt, [vid], graphs=False, noise_seeds=[SEED_A], **kw).sample(_x([vid]))
    calls = _spy_entries(monkeypatch)
    got = _host_loop(Wt, vid, N6, "logsnr", 0.2, noise_seeds=[SEED_A], **kw)
    assert calls == ((["tmix_vpred_rescale_factors"] if phi > 0.0 else []) + ["tmix_vpred_step_noise"]) * N6
    assert torch.equal(got, want)
    again = _host_loop(Wt, vid, N6, "logsnr", 0.2, noise_seeds=[SEED_A], **kw)
    other = _host_loop(Wt, vid, N6, "logsnr", 0.2, noise_seeds=[SEED_A + 1], **kw)
    assert torch.equal(again, got) and torch.isfinite(other).all() and not torch.equal(other, got)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("solver,step,key", [("ddim", "tmix_vpred_step_dev", [False, True]), ("dpmpp2m", "tmix_vpred_step_ms_dev", [(False, "ms"), (True, "ms")])],
                         ids=["ddim", "dpmpp2m"])
def test_eta_zero_is_the_sampler_of_today_and_eta_moves_the_result(monkeypatch, solver, step, key):
    """eta=0.0 spelled out (with or without seeds) equals the call without it: the same bits, the same entry calls, the same graph keys, 32-byte
    uploads, no keys buffer; sample_loop likewise.  eta = 0.6 gives another latent, through the noise entry alone"""
    Wt, vid = _weights(), _video(5)
    calls = _spy_entries(monkeypatch)
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(eta=0.0), dict(eta=0.0, noise_seeds=[SEED_A])):
            smp = _sampler(Wt, [vid], graphs=graphs, solver=solver, **kw)
            out = smp.sample(_x([vid]))
            runs.append((out, list(calls), smp))
            calls[:] = []
    for base, others in ((runs[0], runs[1:3]), (runs[3], runs[4:6])):
        for ob, cb, sb in others:
            assert torch.equal(base[0], ob) and base[1] == cb and sorted(base[2].graphs) == sorted(sb.graphs)
            assert sb.eta == 0.0 and sb.noise_keys is None and sb.params.numel() == 8 and sb._ring.slots.shape[1] == 8
            assert not any(c in NOISE_ENTRIES for c in cb)
    assert runs[1][1] == ["tmix_video_step_prologue", step] * N6 and sorted(runs[4][2].graphs) == key
    assert torch.equal(runs[0][0], runs[3][0])
    a = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver)
    assert calls == [step[:-4]] * N6
    calls[:] = []
    b = _host_loop(Wt, vid, N6, "logsnr", 0.2, solver=solver, eta=0.0, noise_seeds=[SEED_A])
    assert calls == [step[:-4]] * N6 and torch.equal(a, b) and torch.equal(a, runs[0][0])
    calls[:] = []
    nz = _sampler(Wt, [vid], graphs=False, solver=solver, eta=ETA, noise_seeds=[SEED_A]).sample(_x([vid]))
    assert calls == ["tmix_video_step_prologue", "tmix_vpred_step_noise_dev"] * N6
    assert torch.isfinite(nz).all() and not torch.equal(nz, runs[0][0])


# ------------------------------------------------------------------------------------------------ end to end: the variance of the Gaussian model
@pytest.mark.timeout(120)
def test_variance_of_the_gaussian_standin_matches_the_recursion():
    """a callable that returns the EXACT v of scalar Gaussian data N(0, c^2) in both CFG rows, through sample_loop on the device: S = 3 videos of
    4 x 4 x 32 x 32 (49,152 elements), eta = 1, dpmpp2m on the log-SNR grid at n = 20.  The sample variance of the final state lies within five
    standard errors, sqrt(2 / 49152) relative each, of the closed-form recursion's prediction (tests/video_noise_cases.py), for c = 0.5, 1, 2"""
    from tweediemix_amd import video as V
    xT = torch.randn(3, 4, 4, 32, 32, generator=torch.Generator().manual_seed(0))
    se = float(np.sqrt(2.0 / xT.numel()))
    assert xT.numel() == 49152
    for c in VN.CS:
        pred, sch = VN.predicted_variance(c, 20, "logsnr", "dpmpp2m", 1.0)

        def unet(xin, t, sch=sch, c=c):
            return torch.from_numpy(toy_v(xin.cpu().numpy(), float(sch.alpha(t)), 0.0, c).astype(NF)).cuda()
        got = V.sample_loop(unet, xT.cuda(), sch, 9.0, solver="dpmpp2m", eta=1.0, noise_seeds=[101, 102, 103]).cpu().numpy().astype(np.float64)
        var = float((got ** 2).mean())                           # the model's mean is 0
        dist = (var / pred - 1.0) / se
        print(f"Gaussian stand-in c = {c}: sample variance {var:.5f}  recursion {pred:.5f}  target {VN.target_variance(c, sch):.5f}  distance {dist:+.2f} standard errors")
        assert abs(dist) <= 5.0, (c, var, pred, dist)
        per_video = [float((g ** 2).mean()) for g in got]
        assert len({round(p, 9) for p in per_video}) == 3        # three videos, three noises


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.timeout(180)
def test_cli_run_with_eta_writes_its_latents(tmp_path, monkeypatch):
    """run_video.py --eta 1 --solver dpmpp2m --timestep_spacing logsnr --num_seeds 2 writes both latents through the noise entry; a second run gives
    identical files; --seeds_per_batch 1 gives the files of --seeds_per_batch 2 (a video's key is its own seed); without --eta another latent"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")                  # one tiling for the S = 2 and the S = 1 shapes
    spec = importlib.util.spec_from_file_location("rv_noise_gpu", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    calls = _spy_entries(monkeypatch)
    common = ["--synthetic", "--tiny", "--height", "128", "--width", "64", "--num_inference_steps", "6", "--injection_timestep", "0.2", "--seed", "4",
              "--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_seeds", "2"]
    lat = rv.main(common + ["--eta", "1", "--output_dir", str(tmp_path / "a")]).cpu()
    assert set(calls) == {"tmix_video_step_prologue", "tmix_vpred_step_noise_dev"}
    assert lat.shape == (2, 4, 16, 16, 8) and torch.isfinite(lat).all() and not torch.equal(lat[0], lat[1])
    files = ["output_i2v_seed_4.latent.pt", "output_i2v_seed_5.latent.pt"]
    for i, f in enumerate(files):
        assert torch.equal(torch.load(tmp_path / "a" / f), lat[i:i + 1])
    rv.main(common + ["--eta", "1", "--output_dir", str(tmp_path / "b")])
    rv.main(common + ["--eta", "1", "--seeds_per_batch", "1", "--output_dir", str(tmp_path / "c")])
    for f in files:
        assert torch.equal(torch.load(tmp_path / "b" / f), torch.load(tmp_path / "a" / f)), f
        assert torch.equal(torch.load(tmp_path / "c" / f), torch.load(tmp_path / "a" / f)), f
    calls[:] = []
    ref = rv.main(common + ["--output_dir", str(tmp_path / "plain")]).cpu()
    assert set(calls) == {"tmix_video_step_prologue", "tmix_vpred_step_ms_dev"} and not torch.equal(ref, lat)
