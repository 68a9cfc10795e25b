"""GPU: adaptive projected guidance (arXiv:2410.02416) -- tmix_apg_coeffs, tmix_fused_tweedie_step_apg_dev, Tweediemix(apg=...), --apg.

The coefficients are compared with tweediemix_amd.guidance.apg_coeffs_reference inside a bound that comes from the restatement alone (apg_cases.
coeffs_reference): both sides form identical fp32 terms and differ in the order of the fp64 additions; tests/test_apg_cpu.py runs the kernel's
partition in numpy on the same cases.  Everything else -- the step entry against apg_step_reference / apg_multistep_reference, the sampler's states
against the step restated with the device's own coefficients -- is compared by equality."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import apg_cases as AC
from apg_cases import Case, _p
from guidance_interval_cases import mode_id
from layout_frames import Frame, _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(name):
    from tweediemix_amd import lib as L
    return {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[name]


def _coeffs(c, x_t, eps_t, prm_t, co=None, ws=None, seeds=None):
    """raw ABI call -> (code, coeffs [seeds, rows-1, 2]); coeffs and ws pre-filled with NaN: nothing needs zeroing"""
    from tweediemix_amd import lib as L
    lib = L.load()
    S = c["seeds"] if seeds is None else seeds
    if co is None:
        co = torch.full((S, c["rows"] - 1, 2), NAN, dtype=F32, device="cuda")
    if ws is None:
        ws = torch.full((lib.tmix_cfg_rescale_ws_doubles(c["rows"], S),), NAN, dtype=torch.float64, device="cuda")
    rc = lib.tmix_apg_coeffs(_p(x_t), _p(eps_t), _dt(c["dt"]), _p(co), _p(ws), c["K"], 4, c["h"] * c["w"], mode_id(c["mode"]), c["rows"], S, _p(prm_t),
                             c["slot"], c["eta"], c["R"], _st())
    torch.cuda.synchronize()
    return rc, co


def _dev(c):
    x, eps_t, eps, prm = AC.coeff_inputs(c)
    return x, eps, prm, torch.from_numpy(x).cuda(), eps_t.cuda(), torch.tensor(prm, dtype=F32).cuda()


def _one(mode="fusion", dt="f32", h=16, w=16, K=3, spare=0, seeds=3, g=7.5, eta=0.0, R=0.0, alpha=0.2345, slot=6, seed=1):
    return dict(mode=mode, dt=dt, h=h, w=w, K=K, rows=AC.used_rows(mode, K) + 1 + spare, seeds=seeds, g=g, eta=eta, R=R, alpha=alpha, slot=slot, seed=seed)


# ------------------------------------------------------------------------------------------------ coefficients == restatement (derived bound)
@pytest.mark.parametrize("dt", AC.DTS)
@pytest.mark.parametrize("mode", AC.MODES)
def test_coeffs_equal_the_restatement_inside_the_bound(mode, dt):
    """hw in {256, 2053, 4100} x K in {1, 3} x rows in {used + 1, used + 2} x seeds in {1, 3}, cycling g x eta x R x alpha and the slot g is read from:
    B within one fp32 ulp, |A - A_ref| <= ulp32(A_ref) + 4 (g-1)(1-eta) n 2^-53 s sqrt(Sdd / Scc), the spare row (1, g - 1)"""
    worst = 0
    for c in AC.coeff_cases(mode, dt):
        x, eps, prm, x_t, eps_t, prm_t = _dev(c)
        rc, co = _coeffs(c, x_t, eps_t, prm_t)
        assert rc == 0, c
        got = co.cpu().numpy()
        ref, bound = AC.coeffs_reference(c, x, eps, prm)
        assert np.isfinite(got).all() and got.shape == ref.shape, c
        assert AC.ulps(got[..., 1], ref[..., 1]).max() <= 1, (c, got[..., 1], ref[..., 1])
        assert np.all(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]) <= bound), (c, got[..., 0], ref[..., 0], bound)
        used = AC.used_rows(mode, c["K"])
        spare = np.tile(np.array([1.0, NF(float(NF(c["g"])) - 1.0)], NF), (c["seeds"], c["rows"] - 1 - used, 1))
        assert np.array_equal(got[:, used:], spare), c              # rows the mode does not read
        worst = max(worst, int(AC.ulps(got, ref).max()))
    print(f"apg coeffs {mode} {dt}: worst distance {worst} ulp")


def test_two_launches_give_identical_bits():
    c = _one(dt="bf16", h=50, w=82, K=3, eta=0.3, R=15.0)
    _x, _e, _prm, x_t, eps_t, prm_t = _dev(c)
    a = _coeffs(c, x_t, eps_t, prm_t)[1]
    for _ in range(3):
        b = _coeffs(c, x_t, eps_t, prm_t)[1]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_co_batched_seeds_equal_seeds_one_at_a_time():
    for mode, K, spare in (("fusion", 3, 0), ("resample", 3, 0), ("plain", 3, 2), ("plain", 1, 0)):
        c = _one(mode=mode, h=1, w=2053, K=K, spare=spare, R=15.0, seed=8)
        _x, _e, _prm, x_t, eps_t, prm_t = _dev(c)
        all_ = _coeffs(c, x_t, eps_t, prm_t)[1]
        rows = c["rows"]
        for sd in range(3):
            one = _coeffs(c, x_t[sd:sd + 1], eps_t[sd * rows:(sd + 1) * rows], prm_t, seeds=1)[1]
            assert torch.equal(one.view(torch.int32), all_[sd:sd + 1].view(torch.int32)), (mode, sd)


def test_coeffs_guard_bands_and_untouched_inputs():
    from tweediemix_amd import lib as L
    c = _one(dt="f16", h=1, w=2053, K=3, spare=1, eta=0.3, R=15.0, seed=7)
    _x, _e, _prm, x_t, eps_t, prm_t = _dev(c)
    rows, seeds = c["rows"], c["seeds"]
    want = _coeffs(c, x_t, eps_t, prm_t)[1]
    nd = L.load().tmix_cfg_rescale_ws_doubles(rows, seeds)
    assert nd == seeds * (rows - 1) * AC.RS_P * 4
    x = Frame.of(x_t.reshape(1, -1), name="x").seal()
    eps = Frame.of(eps_t.reshape(1, -1), name="eps").seal()
    prm = Frame.of(prm_t.reshape(1, -1), name="params").seal()
    for mode in ("fusion", "plain"):
        co = dense_guarded((seeds, (rows - 1) * 2), F32, rows=8, device="cuda", name="coeffs")
        ws = dense_guarded((1, nd), torch.int64, rows=1, device="cuda", name="ws")           # the doubles' bits
        rc = L.load().tmix_apg_coeffs(_p(x.view), _p(eps.view), L.F16, _p(co.view), _p(ws.view), c["K"], 4, c["h"] * c["w"], mode_id(mode), rows, seeds,
                                      _p(prm.view), c["slot"], c["eta"], c["R"], _st())
        torch.cuda.synchronize()
        assert rc == 0
        co.assert_untouched()
        co.assert_all_written()
        ws.assert_untouched()
        for f in (x, eps, prm):
            f.assert_unchanged()
        got = co.view.reshape(seeds, rows - 1, 2)
        if mode == "fusion":                                            # the three rows the mode reads, then the spare one
            assert torch.equal(got, want)
        else:                                                           # PLAIN: row 1's slots alone are written, every other pair is (1, g - 1)
            assert torch.equal(got[:, 0], want[:, 0]) and torch.equal(got[:, 1:], want[:, 3:].expand(seeds, rows - 2, 2))


def test_degenerate_rows():
    """ec == eu: d = 0 and the pair is (1, g - 1); an all-zero tc: Scc = 0, A = 1; an inf in eps: that row's sums are not finite, (1, g - 1); never a NaN"""
    for dt in AC.DTS:
        c = _one(dt=dt, K=2, seeds=2, R=3.0, seed=5)
        _x, _e, prm, x_t, eps_t, prm_t = _dev(c)
        gm1 = NF(float(NF(c["g"])) - 1.0)
        same = eps_t.clone().reshape(2, 3, 4, 16, 16)
        same[:, 1] = same[:, 0]                                       # row 1 of both seeds equals the unconditional row
        rc, co = _coeffs(c, x_t, same.reshape(6, 4, 16, 16), prm_t)
        got = co.cpu().numpy()
        assert rc == 0 and np.isfinite(got).all() and np.array_equal(got[:, 0], [[1.0, gm1]] * 2) and np.all(got[:, 1, 0] != 1.0), (dt, got)
    # tc == 0 exactly: x = s1 ec with sa = s1 = 0.5 and ec = 1, in every dtype's value set
    c = _one(K=1, seeds=1, mode="plain", R=0.0)
    x_t = torch.full((1, 4, 16, 16), 0.5, device="cuda")
    eps_t = torch.cat([torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)), torch.ones(1, 4, 16, 16)]).cuda()
    prm_t = torch.tensor([0, 0.5, 0.5, 0, 0, 0, c["g"], 0], dtype=F32).cuda()
    rc, co = _coeffs(c, x_t, eps_t, prm_t)
    assert rc == 0 and np.array_equal(co.cpu().numpy(), [[[1.0, NF(float(NF(c["g"])) - 1.0)]]])
    # an inf, and a NaN, in a conditional row
    c = _one(K=3, seeds=1, seed=6)
    x, eps, prm, x_t, eps_t, prm_t = _dev(c)
    eps_t[1, 0, 0, 0] = float("inf")
    eps_t[3, 3, 15, 15] = NAN
    rc, co = _coeffs(c, x_t, eps_t, prm_t)
    got = co.cpu().numpy()
    ref, _b = AC.coeffs_reference(c, x, eps_t.float().cpu().numpy(), prm)
    gm1 = NF(float(NF(c["g"])) - 1.0)
    assert rc == 0 and np.array_equal(got[0, 0], [1.0, gm1]) and np.array_equal(got[0, 2], [1.0, gm1]) and np.array_equal(ref[0, 0], [1.0, gm1])
    assert AC.ulps(got[0, 1], ref[0, 1]).max() <= 1 and got[0, 1, 0] != 1.0


def test_coeffs_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    c = _one(h=3, w=5, K=3, seeds=2)
    _x, _e, _prm, x_t, eps_t, prm_t = _dev(c)
    co = dense_guarded((2, 6), F32, rows=8, device="cuda", name="coeffs")
    ws = dense_guarded((1, lib.tmix_cfg_rescale_ws_doubles(4, 2)), torch.int64, rows=1, device="cuda", name="ws")
    ok = dict(x=_p(x_t), eps=_p(eps_t), dt=L.F32, co=_p(co.view), ws=_p(ws.view), K=3, C=4, hw=15, mode=L.STEP_FUSION, rows=4, seeds=2, prm=_p(prm_t), slot=6,
              eta=0.0, R=0.0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.tmix_apg_coeffs(a["x"], a["eps"], a["dt"], a["co"], a["ws"], a["K"], a["C"], a["hw"], a["mode"], a["rows"], a["seeds"], a["prm"], a["slot"],
                                   a["eta"], a["R"], _st())
    for k in ("x", "eps", "co", "ws", "prm"):
        assert rc(**{k: None}) == L.EINVAL, k
    assert rc(dt=9) == L.EINVAL and rc(mode=7) == L.EINVAL and rc(K=0) == L.EINVAL and rc(slot=8) == L.EINVAL and rc(slot=-1) == L.EINVAL
    assert rc(hw=0) == L.ESHAPE and rc(rows=3) == L.ESHAPE and rc(seeds=0) == L.ESHAPE and rc(seeds=65536) == L.ESHAPE
    for eta in (-0.5, 1.5, NAN, float("inf")):
        assert rc(eta=eta) == L.EINVAL and b"eta" in lib.tmix_last_error_string()
    for R in (-1.0, NAN, float("inf")):
        assert rc(R=R) == L.EINVAL and b"norm_threshold" in lib.tmix_last_error_string()
    torch.cuda.synchronize()
    for f in (co, ws):                                              # nothing was launched: both buffers still hold the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name
    assert rc() == 0
    torch.cuda.synchronize()
    co.assert_all_written()


# ------------------------------------------------------------------------------------------------ step entry == restatement
@pytest.mark.parametrize("dt", AC.DTS)
@pytest.mark.parametrize("form,mode,noise", AC.step_forms())
def test_step_entry_equals_the_restatement_sweep(form, mode, noise, dt):
    """every kernel of the entry: K x seeds x order x shape x (shared | per-seed masks); hw = 1, 5 x 7 (under one workgroup), 17 x 19 (six)"""
    i = 0
    orders = list(AC.ORDERS) if form == "ms" else ["step", "last"]
    for h, w in ((1, 1), (5, 7), (17, 19)):
        for K in (1, 3):
            for seeds in (1, 3):
                for order in orders:
                    Case(form, mode, dt, noise, K, seeds, h, w, order, shared=bool(i & 1), seed=i).cuda().check()
                    i += 1
    # rows the mode does not read lie behind the ones it does: a PLAIN step on a fusion call's rows, a spare row behind FUSION / RESAMPLE
    Case(form, mode, dt, noise, 3, 2, 5, 7, orders[0], rows=5, seed=900).cuda().check()


@pytest.mark.parametrize("mode", AC.MODES[:2])
def test_x0_of_the_2m_form_is_the_ddim_forms_bit_for_bit(mode):
    for dt in AC.DTS:
        for noise in (False, True):
            for order in ("first", "second", "last"):
                m = Case("ms", mode, dt, noise, 3, 3, 17, 19, order, seed=20).cuda()
                d = Case("ddim", mode, dt, noise, 3, 3, 17, 19, "last" if order == "last" else "step", seed=20).cuda()
                assert torch.equal(d.eps_d, m.eps_d) and torch.equal(d.ab_t, m.ab_t) and torch.equal(d.x_t, m.x_t)
                mx, m0, mp = m.run()
                dx, d0, _ = d.run()
                assert torch.equal(m0, d0) and torch.equal(mp, d0), (mode, dt, noise, order)
                if order == "last":                              # the last step writes x0
                    assert torch.equal(mx, d0) and torch.equal(dx, d0)
                else:
                    assert not torch.equal(mx, d0) and not torch.equal(dx, d0)


@pytest.mark.parametrize("form,mode,noise", AC.step_forms())
def test_in_place_guard_bands_and_untouched_inputs(form, mode, noise):
    c = Case(form, mode, "f32", noise, 3, 3, 17, 19, seed=40).cuda()
    ox, o0, pv = c.run()
    S, n = c.seeds, c.n
    flat = lambda t, name: Frame.of(t.reshape(1, -1), name=name).seal()
    eps, masks, prm, ab = flat(c.eps_d, "eps"), flat(c.m_t, "masks"), flat(c.prm, "params"), flat(c.ab_t, "coeffs")
    for in_place in (True, False):
        prev = Frame.of(c.prev_t.reshape(S, n), name="x0_prev")
        out0 = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x0")
        if in_place:
            x = dense_guarded((S, n), F32, rows=8, device="cuda", name="x (in place)")
            x.view.copy_(c.x_t.reshape(S, n))
            outx = x
        else:
            x = Frame.of(c.x_t.reshape(S, n), name="x").seal()
            outx = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x")
        assert c.launch(outx.view, out0.view, prev.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view, ab=ab.view) == 0
        torch.cuda.synchronize()
        for f in (outx, out0):
            f.assert_untouched()
            f.assert_all_written()
        prev.assert_untouched()
        for f in (eps, masks, prm, ab) + (() if in_place else (x,)):
            f.assert_unchanged()
        assert torch.equal(outx.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
        assert torch.equal(prev.view.reshape(o0.shape), pv)          # the history: this step's x0 (2M) or untouched (DDIM)
        x2, prev2 = c.x_t.clone(), c.prev_t.clone()                  # without out_x0, in place
        assert c.launch(x2, None, prev2, x=x2) == 0
        torch.cuda.synchronize()
        assert torch.equal(x2, ox)


def test_shared_and_per_seed_masks():
    """one mask set for all seeds equals the same set repeated per seed; per-seed sets do reach their own seeds"""
    for form in AC.FORMS:
        sh = Case(form, "fusion", "f32", False, 3, 3, 17, 19, shared=True, seed=60).cuda()
        ps = Case(form, "fusion", "f32", False, 3, 3, 17, 19, shared=False, seed=60).cuda()
        a = sh.run()
        rep = sh.m_t.expand(3, 3, 1, 17, 19).contiguous()
        ps.shared = False
        b = ps.run(x=sh.x_t, eps=sh.eps_d, masks=rep, ab=sh.ab_t)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), form
        ps.check()
        sh.check()


def test_second_pass_of_the_grid_stride_loop():
    """hw = 131075 = 175 x 749: n = 524,300 > 2048 workgroups x 256 threads, twelve elements enter the second pass; the coefficients come from the
    coefficient kernels (65 passes of their own loop)"""
    for form, noise in (("ddim", False), ("ms", True)):
        c = Case(form, "fusion", "f32", noise, 3, 1, 175, 749, shared=True, seed=50).cuda()
        assert c.hw == 131075 and c.n > 2048 * 256
        cc = dict(mode="fusion", dt="f32", h=175, w=749, K=3, rows=4, seeds=1, g=7.5, eta=0.0, R=15.0, slot=7 if c.ms else 6)
        rc, co = _coeffs(cc, c.x_t, c.eps_d, c.prm)
        ref, bound = AC.coeffs_reference(cc, c.x, c.eps, c.params)
        got = co.cpu().numpy()
        assert rc == 0 and AC.ulps(got[..., 1], ref[..., 1]).max() <= 1 and np.all(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]) <= bound)
        c.ab_t, c.ab = co, got
        c.check()


def test_a_first_order_step_ignores_a_nan_history():
    for mode in AC.MODES[:2]:
        for noise in (False, True):
            for order in ("first", "last"):
                c = Case("ms", mode, "f32", noise, 3, 2, 17, 19, order, seed=70).cuda()
                ox, o0, pv = c.run()
                nan = torch.full_like(c.prev_t, NAN)
                out_x, out_x0 = torch.empty_like(c.x_t), torch.empty_like(c.x_t)
                assert c.launch(out_x, out_x0, nan) == 0
                torch.cuda.synchronize()
                assert torch.equal(out_x, ox) and torch.equal(out_x0, o0) and torch.equal(nan, o0) and torch.isfinite(out_x).all(), (mode, noise, order)


def test_noise_on_a_two_window_canvas():
    """rows are windows of one trajectory: the noise of an element is that of its canvas coordinate, identical where the windows overlap"""
    from tweediemix_amd import noise as NZ, ops
    from tweediemix_amd import guidance as G
    for form in AC.FORMS:
        c = Case(form, "fusion", "f32", True, 3, 2, 16, 16, seed=80).cuda()
        wins, ch, cw = [(0, 0), (0, 8)], 16, 24
        keys = ops.noise_keys(c.seed_values[:1], "cuda")
        prev = c.prev_t.clone()
        o0 = torch.empty_like(c.x_t)
        ox = ops.fused_tweedie_step_apg_dev(c.x_t, c.eps_d, c.m_t, mode_id("fusion"), 3, c.prm, c.ab_t, x0_prev=prev if c.ms else None, keys=keys, windows=wins,
                                            canvas_hw=(ch, cw), out_x0=o0)
        torch.cuda.synchronize()
        for b, (oy, oxx) in enumerate(wins):
            idx = NZ.canvas_index(4, 16, 16, oy, oxx, ch, cw)
            fn = G.apg_multistep_reference if c.ms else G.apg_step_reference
            args = (c.x[b:b + 1], c.eps[b * 4:(b + 1) * 4], c.masks[b]) + ((c.prev[b:b + 1],) if c.ms else (3,)) + (c.ab[b], c.params, NZ.seed_key(c.seed_values[0]), idx)
            a, z = fn(mode_id("fusion"), *args)
            assert np.array_equal(ox[b:b + 1].cpu().numpy(), a) and np.array_equal(o0[b:b + 1].cpu().numpy(), z), (form, b)


def test_step_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    for form in AC.FORMS:
        c = Case(form, "fusion", "f32", True, 3, 2, 3, 5, seed=71).cuda()
        out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
        out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
        prev = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="x0_prev")
        go = lambda **kw: c.launch(out_x.view, out_x0.view, prev.view, **kw)
        assert go(ab=None) == L.EINVAL and b"coeffs" in lib.tmix_last_error_string()
        assert c.launch(None, out_x0.view, prev.view) == L.EINVAL
        assert go(mode=7) == L.EINVAL and go(K=0) == L.EINVAL and go(dt=9) == L.EINVAL
        assert go(mode=L.STEP_RESAMPLE) == L.EINVAL and b"RESAMPLE" in lib.tmix_last_error_string()       # keys (and, for 2M, x0_prev) are given
        assert go(mode=L.STEP_RESAMPLE, keys=None, ms=True) == L.EINVAL
        assert go(rows=c.K) == L.ESHAPE and go(seeds=0) == L.ESHAPE and go(seeds=65536) == L.ESHAPE
        assert go(w=4) == L.ESHAPE and go(n_win=3) == L.EINVAL and go(n_win=2, yx=[0, 0, 0, 9], canvas=(3, 8)) == L.ESHAPE
        torch.cuda.synchronize()
        for f in (out_x, out_x0, prev):
            assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


def test_ops_wrappers():
    from tweediemix_amd import lib as L, ops
    c = Case("ddim", "fusion", "bf16", False, 3, 3, 17, 19, seed=81).cuda()
    co = ops.apg_coeffs(c.x_t, c.eps_d, L.STEP_FUSION, 3, c.prm, 6, eta=0.25, norm_threshold=15.0)
    torch.cuda.synchronize()
    cc = dict(mode="fusion", dt="bf16", K=3, rows=4, seeds=3, g=7.5, eta=0.25, R=15.0)
    ref, bound = AC.coeffs_reference(cc, c.x, c.eps, c.params)
    got = co.cpu().numpy()
    assert tuple(co.shape) == (3, 3, 2) and AC.ulps(got[..., 1], ref[..., 1]).max() <= 1 and np.all(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]) <= bound)
    c.ab_t, c.ab = co, got
    ref, ref0 = c.reference()
    o0 = torch.empty_like(c.x_t)
    ox = ops.fused_tweedie_step_apg_dev(c.x_t, c.eps_d, c.m_t, L.STEP_FUSION, 3, c.prm, co, out_x0=o0)
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(o0.cpu().numpy(), ref0)
    m = Case("ms", "plain", "f16", True, 3, 2, 17, 19, "second", seed=82).cuda()
    ref, ref0 = m.reference()
    prev = m.prev_t.clone()
    ox = ops.fused_tweedie_step_apg_dev(m.x_t, m.eps_d, None, L.STEP_PLAIN, 3, m.prm, m.ab_t, x0_prev=prev, keys=m.keys_t)
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(prev.cpu().numpy(), ref0)


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


K3, H, W = 3, 16, 16
G_RUN = 7.5
APG = dict(eta=0.25, norm_threshold=15.0)
ROWS = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2, "fusion_c": K3, "fusion_base_c": K3, "plain_c": 1}
OLD_ENTRIES = ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev", "tmix_fused_tweedie_step_ms_dev", "tmix_cfg_rescale_factors",
               "tmix_fused_tweedie_step_rs_dev", "tmix_fused_tweedie_step_ms_rs_dev", "tmix_fused_tweedie_step_noise_dev", "tmix_fused_tweedie_step_cond_dev")
APG_ENTRIES = ("tmix_apg_coeffs", "tmix_fused_tweedie_step_apg_dev")


def _cfg(S, n=10, R=1, J=1, g=G_RUN):
    return S.make_config(guidance_scale=g, n_timesteps=n, t_cond=0.2, t_stop=0.8, resampling_steps=R, jumping_steps=J, resolution_h=H * 8,
                         resolution_w=W * 8)


def _standin_eps(i, rows, seeds, dtype=torch.float32):
    return torch.randn(seeds * rows, 4, H, W, generator=torch.Generator().manual_seed(4000 + i)).to(dtype)


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step / statistics entry the image sampler calls"""
    from tweediemix_amd import lib as L
    lib, calls = L.load(), []
    for name in OLD_ENTRIES + APG_ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _check_coeffs(got, mode, x, eps, prm, ms, lowp, dt="f32"):
    """one seed's device coefficients against the restatement on that step's state and eps, inside the derived bound"""
    c = dict(mode={0: "fusion", 1: "plain", 2: "resample"}[mode], dt="f16" if lowp is not None else dt, K=K3, rows=eps.shape[0], seeds=1, g=G_RUN,
             eta=APG["eta"], R=APG["norm_threshold"])
    assert prm[7 if ms else 6] == NF(G_RUN)
    ref, bound = AC.coeffs_reference(c, x, eps, prm)
    assert AC.ulps(got[:, 1], ref[0, :, 1]).max() <= 1, (got, ref)
    assert np.all(np.abs(got[:, 0].astype(np.float64) - ref[0, :, 0]) <= bound[0]), (got, ref, bound)
    return int(AC.ulps(got, ref[0]).max())


@pytest.mark.parametrize("lora,seeds,dtype,solver,eta", [(False, 1, torch.float32, "ddim", 0.0), (True, 1, torch.float16, "dpmpp2m", 0.0),
                                                         (False, 2, torch.bfloat16, "ddim", 0.0), (False, 2, torch.float32, "dpmpp2m", 0.5),
                                                         (True, 1, torch.bfloat16, "ddim", 0.5)])
def test_sampler_standin_unet_every_step_equals_the_restatement(lora, seeds, dtype, solver, eta, monkeypatch):
    """n = 10, K = 3, partition masks, one resampling and one jumping step, g = 7.5, the stand-in returning fp32 / fp16 / bf16 eps.  A spy copies the
    coefficient buffer at every step: each pair lies inside the bound of the restatement on that step's state and eps, and the step restated with the
    DEVICE's coefficients equals the state by equality -- at all 13 steps (start phase, resampling, look-ahead, plain and fusion steps, both moves,
    with the noise of --eta where the step advances the trajectory)"""
    from tweediemix_amd import guidance as G, lib as L, masks as M, noise as NZ, sampler as S
    n, R, J = 10, 1, 1
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W)
    mk = masks.cpu().numpy()
    lowp = np.float16 if dtype == torch.float16 else None
    kw = dict(solver="dpmpp2m", timestep_spacing="logsnr") if solver != "ddim" else {}
    noise_seeds = [77 + i for i in range(seeds)]
    if eta:
        kw.update(eta=eta, noise_seeds=noise_seeds)
    tw = S.Tweediemix(_cfg(S, n, R, J), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, lora=lora, n_seeds=seeds, apg=APG, **kw)
    log, rec = [], []

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return _standin_eps(len(log) - 1, ROWS[kind], seeds, dtype).cuda()
    tw._unet = unet
    real = tw._fused_step

    def spy(eps_ptr, eps_dt, rows, mode, st, ms=False, nz=False):
        prev = None if tw._x0_prev is None else tw._x0_prev.clone()
        real(eps_ptr, eps_dt, rows, mode, st, ms, **(dict(nz=True) if nz else {}))
        torch.cuda.synchronize()
        rec.append((rows, mode, ms, nz, prev, tw._apg_coeffs[:seeds * (rows - 1) * 2].reshape(seeds, rows - 1, 2).cpu().numpy().copy(),
                    tw.step_params.cpu().numpy().copy(), tw.x_state.cpu().numpy().copy(), tw.x0_state.cpu().numpy().copy()))
    tw._fused_step = spy
    calls = _spy_entries(monkeypatch)
    xT = torch.randn(seeds, 4, H, W, generator=torch.Generator().manual_seed(41 + seeds))
    out = tw.run_fusion(xT.clone())
    assert len(log) == len(rec) == n + 2 * R + J == 13 and torch.isfinite(out).all()
    assert calls == list(APG_ENTRIES) * 13                            # the coefficients, then the APG step: never another entry
    assert sum(r[2] for r in rec) == (9 if solver != "ddim" else 0) and sum(r[3] for r in rec) == (10 if eta else 0)
    worst = 0
    for ci, ((kind, t, x), (rows, mode, ms, nz, prev, co, prm, after, x0s)) in enumerate(zip(log, rec)):
        assert rows == ROWS[kind] and prm[0] == t
        eps = _standin_eps(ci, rows, seeds, dtype).float().numpy()
        xb = x.cpu().numpy()
        p = prm[:12 if nz else 8]
        for sd in range(seeds):
            e = eps[sd * rows:(sd + 1) * rows]
            worst = max(worst, _check_coeffs(co[sd], mode, xb[sd:sd + 1], e, p, ms, lowp))
            used = G.rows_read(mode, K3)
            assert np.all(co[sd, used:] == [1.0, NF(G_RUN - 1)]) and np.all(co[sd, :used, 0] != 1.0)
            key = NZ.seed_key(noise_seeds[sd]) if nz else None
            m = mk if mode == L.STEP_FUSION else None
            if ms:
                a, b = G.apg_multistep_reference(mode, xb[sd:sd + 1], e, m, prev[sd:sd + 1].cpu().numpy(), co[sd], p, key, None, lowp)
            else:
                a, b = G.apg_step_reference(mode, xb[sd:sd + 1], e, m, K3, co[sd], p, key, None, lowp)
            assert np.array_equal(after[sd:sd + 1], a) and np.array_equal(x0s[sd:sd + 1], b), (ci, kind, t, sd)
    assert np.array_equal(out.cpu().numpy(), rec[-1][7])
    print(f"stand-in run lora={lora} seeds={seeds} {dtype} {solver} eta={eta}: worst coefficient distance {worst} ulp")


# ------------------------------------------------------------------------------------------------ sampler on the tiny synthetic UNet (real plans)
class _Tiny:
    K, h, w = 3, 16, 16

    def __init__(self, kind="custom", g=G_RUN):
        from test_keep_region_gpu import _tiny
        from tweediemix_amd import masks as M, sampler as S
        self.S, self.kind = S, kind
        self.W, self.te, self.ts = _tiny(kind, self.K)
        self.cfg = _cfg(S, g=g)
        self.masks = M.build_masks(M.partition_rectangle_masks(self.K, self.h * 8, self.w * 8, seed=3), self.h, self.w)
        self.xT = torch.randn(2, 4, self.h, self.w, generator=torch.Generator().manual_seed(29))

    def sampler(self, graphs=False, seeds=1, masks=None, **kw):
        masks = self.masks if masks is None else masks
        return self.S.Tweediemix(self.cfg, self.W, self.te, self.ts, lambda x0: masks, concept_num=self.K, lora=(self.kind == "lora"),
                                 use_graphs=graphs, n_seeds=seeds, **kw)


MS = dict(solver="dpmpp2m", timestep_spacing="logsnr")


@pytest.mark.parametrize("kind,kw", [("custom", {}), ("lora", dict(MS, eta=0.5, noise_seeds=[5]))])
def test_tiny_unet_graph_replay_equals_eager(kind, kw, monkeypatch):
    """the coefficients are deterministic, so a captured run equals the eager one bit for bit; every captured step has a key of its own ending in "apg" """
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    T = _Tiny(kind)
    eager, graph = T.sampler(False, apg=APG, **kw), T.sampler(True, apg=APG, **kw)
    a, b = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert eager.unet_calls == graph.unet_calls and len(eager.unet_calls) == 13
    keys = sorted(graph.graphs, key=str)
    assert keys and all(k[-1] == "apg" for k in keys)
    if kw:
        assert sorted(keys, key=str) == sorted([("start", L.STEP_RESAMPLE, "apg"), ("plain", L.STEP_PLAIN, "apg"), ("start", L.STEP_PLAIN, "eta", "apg"),
                                                ("fusion", L.STEP_FUSION, "ms", "eta", "apg"), ("fusion_base", L.STEP_FUSION, "ms", "eta", "apg"),
                                                ("plain", L.STEP_PLAIN, "ms", "eta", "apg")], key=str)
    else:
        assert keys == sorted([("start", L.STEP_RESAMPLE, "apg"), ("plain", L.STEP_PLAIN, "apg"), ("start", L.STEP_PLAIN, "apg"),
                               ("fusion", L.STEP_FUSION, "apg")], key=str)
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()             # every captured step replayed from the first one on
    assert torch.equal(again, a) and sorted(graph.graphs, key=str) == keys
    assert not torch.equal(a, T.sampler(False, **kw).run_fusion(T.xT[0:1].clone()).cpu())     # and it is not the run without the flag


def test_flag_off_is_the_sampler_of_today(monkeypatch):
    """apg=None spelled out equals the constructor call without it: the same bits, step entries, UNet calls, plan launch names and graph keys, neither
    APG entry is ever called and nothing is allocated for it"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    names = lambda p: [getattr(fn, "__name__", "") for fn, _a in p.ops]
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(apg=None)):
            tw = T.sampler(graphs, **kw)
            out = tw.run_fusion(T.xT[0:1].clone()).cpu()
            runs.append((out, list(calls), tw))
            calls[:] = []
    for (oa, ca, ta), (ob, cb, tb) in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert torch.equal(oa, ob) and ca == cb and ta.unet_calls == tb.unet_calls and len(ta.unet_calls) == 13
        assert sorted(ta.plans) == sorted(tb.plans) and sorted(ta.graphs) == sorted(tb.graphs)
        for k in ta.plans:
            assert names(ta.plans[k]) == names(tb.plans[k]) and len(names(ta.plans[k])) > 50, k
        assert tb.apg is None and tb._apg_coeffs is None and tb._apg_ws is None
    assert runs[0][1] == [OLD_ENTRIES[0]] * 13
    assert not any(c in APG_ENTRIES for r in runs for c in r[1])
    assert torch.equal(runs[0][0], runs[2][0]) and all(len(k) == 2 for k in runs[3][2].graphs)


def test_tiny_unet_interval_unguided_steps_launch_no_apg_kernel(monkeypatch):
    """guidance_interval (700, 250): the trajectory steps outside it run the unguided entry alone -- neither APG launch -- and keep their graph keys;
    the guided ones run the APG pair; captured equals eager"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    eager = T.sampler(False, apg=APG, guidance_interval=(700, 250))
    a = eager.run_fusion(T.xT[0:1].clone()).cpu()
    got, calls[:] = list(calls), []
    want = []
    for kind, _rows, _t in eager.unet_calls:
        want += ["tmix_fused_tweedie_step_cond_dev"] if kind.endswith("_c") else list(APG_ENTRIES)
    n_c = sum(k.endswith("_c") for k, _r, _t in eager.unet_calls)
    assert got == want and 0 < n_c < 10 and len(eager.unet_calls) == 13
    graph = T.sampler(True, apg=APG, guidance_interval=(700, 250))
    b = graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.equal(a, b) and torch.isfinite(a).all()
    for k in graph.graphs:
        assert (k[-1] == "apg") != k[0].endswith("_c"), k
        assert len(k) == (2 if k[0].endswith("_c") else 3), k


def test_tiny_unet_two_window_canvas_equals_apg_step_plus_consensus(monkeypatch):
    """16 x 24 canvas, two 16 x 16 windows overlapping by 8, the solver run: every step equals the APG step restated per window -- with that window's own
    coefficients, each inside the bound of its restatement on the state and the eps the plan produced -- followed by the consensus restatement of
    tests/test_canvas_gpu.py.  Statistics are per window."""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from test_canvas_gpu import consensus_np
    from tweediemix_amd import guidance as G, lib as L, masks as M
    T = _Tiny("custom")
    ch, cw = 16, 24
    masks = M.build_masks(M.partition_rectangle_masks(T.K, ch * 8, cw * 8, seed=3), ch, cw)
    tw = T.sampler(False, masks=masks, canvas=dict(height=ch * 8, width=cw * 8, overlap=64), apg=APG, **MS)
    assert tw.windows == [(0, 0), (0, 8)] and tw.n_seeds == 2
    rec, real = [], tw._enqueue_step

    def spy(kind, mode, ms=False):
        before, prev = tw.x_state.clone(), tw._x0_prev.clone()
        real(kind, mode, ms)
        torch.cuda.synchronize()
        rows = tw.plan(kind).B // 2
        rec.append((kind, mode, ms, before, prev, tw.plan(kind).eps.clone(), tw.step_params.clone(), tw.x_state.clone(), tw.x0_state.clone(),
                    tw._apg_coeffs[:2 * (rows - 1) * 2].reshape(2, rows - 1, 2).clone()))
    tw._enqueue_step = spy
    xT = torch.randn(1, 4, ch, cw, generator=torch.Generator().manual_seed(31))
    out = tw.run_fusion(xT.clone())
    assert out.shape == (1, 4, ch, cw) and torch.isfinite(out).all() and len(rec) == 13
    assert [r[2] for r in rec] == [False] * 3 + [True] + [False] + [True] * 8
    mw = tw.masks.cpu().numpy()
    differ = False
    for kind, mode, ms, before, prev, eps, prm, after, x0s, co in rec:
        rows = eps.shape[0] // 2
        e, xb, pv, f, p = eps.float().cpu().numpy(), before.cpu().numpy(), prev.cpu().numpy(), co.cpu().numpy(), prm.cpu().numpy()[:8]
        moved, est = [], []
        for b in range(2):
            eb = e[b * rows:(b + 1) * rows]
            _check_coeffs(f[b], mode, xb[b:b + 1], eb, p, ms, None, dt="f32")
            m = mw[b] if mode == L.STEP_FUSION else None
            if ms:
                a, z = G.apg_multistep_reference(mode, xb[b:b + 1], eb, m, pv[b:b + 1], f[b], p)
            else:
                a, z = G.apg_step_reference(mode, xb[b:b + 1], eb, m, T.K, f[b], p)
            moved.append(a)
            est.append(z)
        differ = differ or not np.array_equal(f[0], f[1])
        want = consensus_np(np.concatenate(moved).reshape(1, 2, 4, 16, 16), tw.windows, ch, cw)[0].reshape(2, 4, 16, 16)
        assert np.array_equal(after.cpu().numpy(), want), (kind, p[0])
        assert np.array_equal(x0s.cpu().numpy(), np.concatenate(est)), (kind, p[0])
        assert torch.equal(after[0, :, :, 8:], after[1, :, :, :8])
    assert differ                                                  # the two windows do carry different coefficients


def test_refusals_come_before_any_launch(monkeypatch):
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    tw = T.sampler(False, apg=APG)
    z = torch.zeros(1, 4, T.h, T.w)
    with pytest.raises(ValueError, match=r"set_keep.*apg="):
        tw.set_keep(z, z[:, :1], z)
    assert calls == [] and tw._keep is None and tw.plans == {} and tw.unet_calls == []
    with pytest.raises(ValueError, match=r"apg=.*guidance_rescale=0.7"):
        T.sampler(False, apg=APG, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="apg"):
        T.sampler(False, apg=dict(eta=1.5))
    assert calls == []


# ------------------------------------------------------------------------------------------------ CLI
def _load(script, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "fusion_generation", script))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("script", ["fusion_sampling.py", "fusion_sampling_lora.py"])
def test_cli_run_with_the_flag_writes_its_outputs(script, tmp_path, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from PIL import Image
    fs = _load(script, "fs_apg_gpu_" + script[:-3])
    fs = getattr(fs, "_fs", fs)
    assert fs.LORA == script.endswith("lora.py")
    a, b = np.zeros((128, 128), np.uint8), np.zeros((128, 128), np.uint8)
    a[16:96, 8:56] = 255
    b[32:120, 72:120] = 255
    Image.fromarray(a).save(tmp_path / "a cat.png")
    Image.fromarray(b).save(tmp_path / "a dog.png")
    common = ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--guidance_scale", "7.5",
              "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "1", "--resolution_h", "128", "--resolution_w", "128",
              "--output_path", str(tmp_path), "--mask_paths", f"{tmp_path / 'a cat.png'}+{tmp_path / 'a dog.png'}", "--seed", "5"]
    calls = _spy_entries(monkeypatch)
    lat = fs.main(common + ["--apg", "--apg_eta", "0.25", "--apg_norm", "15", "--output_path_all", str(tmp_path / "apg")]).cpu()
    assert calls and set(calls) == set(APG_ENTRIES)
    calls[:] = []
    ref = fs.main(common + ["--output_path_all", str(tmp_path / "plain")]).cpu()
    assert calls and not set(calls) & set(APG_ENTRIES)
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all() and not torch.equal(lat, ref)
    assert torch.equal(torch.load(tmp_path / "apg" / "p_5.latent.pt"), lat)
    assert Image.open(tmp_path / "apg" / "p_5.png").size == (128, 128)
    with pytest.raises(SystemExit, match=r"--apg does not combine with --keep_latents"):
        fs.main(common + ["--apg", "--keep_latents", str(tmp_path / "apg" / "p_5.latent.pt"), "--reroll", "1", "--output_path_all", str(tmp_path / "keep")])
    with pytest.raises(SystemExit, match=r"give --apg too"):
        fs.main(common + ["--apg_norm", "15", "--output_path_all", str(tmp_path / "x")])
