"""GPU: guidance rescale -- tmix_cfg_rescale_factors, tmix_fused_tweedie_step_rs_dev / _ms_rs_dev, Tweediemix(guidance_rescale=phi), --guidance_rescale.

The factors are compared with tweediemix_amd.guidance.rescale_factors_reference within ONE fp32 ulp: both sides hold the same fp32 e_r and differ in the
order of the fp64 sums and in one-pass against two-pass variance (relative 1e-15 or so; half an fp32 ulp is 6e-8; tests/test_guidance_rescale_cpu.py
runs the kernel's partition in numpy on the same data).  Everything else -- the step entries against rescaled_step_reference /
rescaled_multistep_reference, the sampler's states against the step restated with the device's own factors -- is compared by equality."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from layout_frames import Frame, _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODES = ("fusion", "plain", "resample")
# multistep entry: (cx, c0, c1, is_last) of a first-order step, a second-order step, the last step (whose coefficients are not read)
ORDERS = {"first": (0.8125, 0.3217, 0.0, 0), "second": (0.8125, 0.4021, -0.0804, 0), "last": (0.0, 1.0, 0.0, 1)}
RS_P, RS_THREADS = 32, 256                                          # csrc/cfg_rescale.hip: one pass of the partials grid covers RS_P * RS_THREADS elements
# 4 x 5 x 7 = 140 elements: one workgroup of the 32 gets a partial slice, 31 none; 4 x 16 x 16 = 1024: four get a full slice; 4 x 48 x 48 = 9216 >
# 8192: the first 1024 threads of the grid take a second element; 4 x 64 x 64 = 16384: two full passes
SHAPES = ((5, 7), (16, 16), (48, 48), (64, 64))
DATA = [(m, s) for m in (0.0, 3.0, -100.0) for s in (1.0, 1e-2)]
GS, PHIS = (1.0, 7.5, 9.0, 30.0), (0.25, 0.7, 1.0)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _mode(name):
    from tweediemix_amd import lib as L
    return {"fusion": L.STEP_FUSION, "plain": L.STEP_PLAIN, "resample": L.STEP_RESAMPLE}[name]


def _dt(name):
    from tweediemix_amd import lib as L
    return {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[name]


def ulps(a, b):
    a, b = np.ascontiguousarray(a, NF).reshape(-1), np.ascontiguousarray(b, NF).reshape(-1)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _make_eps(rng, seeds, rows, h, w, mean, sd, dt):
    """[seeds * rows, 4, h, w] of the eps dtype: per seed an unconditional row of the given mean and standard deviation and conditional rows near it"""
    eu = mean + sd * rng.randn(seeds, 1, 4, h, w)
    ec = eu + 0.5 * sd * rng.randn(seeds, rows - 1, 4, h, w)
    e = np.concatenate([eu, ec], axis=1).reshape(seeds * rows, 4, h, w).astype(NF)
    return torch.from_numpy(e).to(DT[dt]).cuda()


def _factors(eps_t, dt, mode, K, rows, seeds, g, phi, slot=6, fac=None, ws=None, prm=None):
    """raw ABI call -> (code, factors [seeds, rows-1], params)"""
    from tweediemix_amd import lib as L
    lib = L.load()
    hw = eps_t.shape[2] * eps_t.shape[3]
    if prm is None:
        v = [0.0] * 8
        v[slot] = g
        prm = torch.tensor(v, dtype=F32).cuda()
    if fac is None:
        fac = torch.full((seeds, rows - 1), float("nan"), dtype=F32, device="cuda")
    if ws is None:
        ws = torch.full((lib.tmix_cfg_rescale_ws_doubles(rows, seeds),), float("nan"), dtype=torch.float64, device="cuda")    # nothing needs zeroing
    rc = lib.tmix_cfg_rescale_factors(_p(eps_t), _dt(dt), _p(fac), _p(ws), K, 4, hw, _mode(mode), rows, seeds, _p(prm), slot, phi, _st())
    torch.cuda.synchronize()
    return rc, fac, prm


def _factors_ref(eps_t, dt, mode, K, rows, seeds, g, phi):
    from tweediemix_amd import guidance as G
    e = eps_t.float().cpu().numpy()
    lowp = np.float16 if dt == "f16" else None
    return np.stack([G.rescale_factors_reference(_mode(mode), e[s * rows:(s + 1) * rows], K, g, phi, lowp) for s in range(seeds)])


# ------------------------------------------------------------------------------------------------ factors == restatement (one ulp)
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
def test_factors_equal_the_restatement_to_one_ulp(mode, dt):
    """shapes x K x seeds, cycling (mean, sd) x g x phi (72 combinations over the 32 launches of each of the 9 parameter sets: 288 launches), the slot g is
    read from, and for PLAIN the row count (2, or K + 1 with K - 1 rows the mode does not read)"""
    i = 7 * MODES.index(mode) + 23 * list(DT).index(dt)
    worst, n_off = 0, 0
    for h, w in SHAPES:
        for K in (1, 2, 3, 4):
            for seeds in (1, 3):
                (mean, sd), g, phi = DATA[i % 6], GS[(i // 6) % 4], PHIS[(i // 24) % 3]
                rows = 2 if (mode == "plain" and i & 1) else K + 1
                eps = _make_eps(np.random.RandomState(1000 + i), seeds, rows, h, w, mean, sd, dt)
                rc, fac, _ = _factors(eps, dt, mode, K, rows, seeds, g, phi, slot=6 + (i & 1))
                assert rc == 0
                got, ref = fac.cpu().numpy(), _factors_ref(eps, dt, mode, K, rows, seeds, g, phi)
                what = (mode, dt, h, w, K, seeds, mean, sd, g, phi, rows)
                assert np.isfinite(got).all() and got.shape == ref.shape, what
                d = ulps(got, ref)
                assert d.max() <= 1, (what, got, ref)
                worst, n_off = max(worst, int(d.max())), n_off + int((d > 0).sum())
                used = 1 if mode == "plain" else K
                assert np.array_equal(got[:, used:], np.ones((seeds, rows - 1 - used), NF)), what     # rows the mode does not read
                i += 5
    print(f"factors {mode} {dt}: worst {worst} ulp, {n_off} factors off by one")


def test_every_data_g_phi_combination_once():
    """the 72 combinations of (mean, sd) x g x phi, each once, at K = 3, two seeds, 4 x 16 x 16, fp32 and fp16"""
    for dt in ("f32", "f16"):
        for j, ((mean, sd), g, phi) in enumerate((d, g, p) for d in DATA for g in GS for p in PHIS):
            eps = _make_eps(np.random.RandomState(3000 + j), 2, 4, 16, 16, mean, sd, dt)
            rc, fac, _ = _factors(eps, dt, "fusion", 3, 4, 2, g, phi)
            ref = _factors_ref(eps, dt, "fusion", 3, 4, 2, g, phi)
            assert rc == 0 and ulps(fac.cpu().numpy(), ref).max() <= 1, (dt, mean, sd, g, phi, fac.cpu().numpy(), ref)


def test_constant_guided_prediction_gives_one():
    """eu == ec (any constant, also one whose square is not exact in fp64 sums): e_r is constant, sd_e = 0, the factor is 1.0; a non-finite element too"""
    for dt in DT:
        for c in (0.1, 3.0, -100.3):
            eps = torch.full((2 * 3, 4, 16, 16), c, dtype=DT[dt], device="cuda")
            rc, fac, _ = _factors(eps, dt, "fusion", 2, 3, 2, 9.0, 0.7)
            assert rc == 0 and torch.equal(fac, torch.ones_like(fac)), (dt, c, fac)
    eps = _make_eps(np.random.RandomState(5), 1, 3, 16, 16, 0.0, 1.0, "f32")
    eps[1, 0, 0, 0] = float("inf")
    eps[2, 3, 15, 15] = float("nan")
    rc, fac, _ = _factors(eps, "f32", "fusion", 2, 3, 1, 9.0, 0.7)
    assert rc == 0 and torch.equal(fac, torch.ones_like(fac))


def test_two_launches_give_identical_bits():
    eps = _make_eps(np.random.RandomState(6), 3, 5, 64, 64, 3.0, 1.0, "bf16")
    a = _factors(eps, "bf16", "fusion", 4, 5, 3, 9.0, 0.7)[1]
    for _ in range(3):
        b = _factors(eps, "bf16", "fusion", 4, 5, 3, 9.0, 0.7)[1]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_factors_guard_bands_and_untouched_inputs():
    from tweediemix_amd import lib as L
    K, rows, seeds = 3, 4, 3
    eps_t = _make_eps(np.random.RandomState(7), seeds, rows, 37, 41, 0.0, 1.0, "f16")
    want = _factors(eps_t, "f16", "fusion", K, rows, seeds, 7.5, 0.7)[1]
    nd = L.load().tmix_cfg_rescale_ws_doubles(rows, seeds)
    assert nd == seeds * (rows - 1) * RS_P * 4
    eps = Frame.of(eps_t.reshape(1, -1), name="eps").seal()
    prm = Frame.of(torch.tensor([[0, 0, 0, 0, 0, 0, 7.5, 0]], dtype=F32, device="cuda"), name="params").seal()
    fac = dense_guarded((seeds, rows - 1), F32, rows=8, device="cuda", name="factors")
    ws = dense_guarded((1, nd), torch.int64, rows=1, device="cuda", name="ws")           # the doubles' bits
    hw = 37 * 41
    rc = L.load().tmix_cfg_rescale_factors(_p(eps.view), L.F16, _p(fac.view), _p(ws.view), K, 4, hw, L.STEP_FUSION, rows, seeds, _p(prm.view), 6, 0.7, _st())
    torch.cuda.synchronize()
    assert rc == 0
    for f in (fac, ws):
        f.assert_untouched()
        f.assert_all_written()
    eps.assert_unchanged()
    prm.assert_unchanged()
    assert torch.equal(fac.view, want)
    # PLAIN on the same rows: only row 1's slots are written, the other factors are 1.0, and still nothing outside
    fac2 = dense_guarded((seeds, rows - 1), F32, rows=8, device="cuda", name="factors")
    ws2 = dense_guarded((1, nd), torch.int64, rows=1, device="cuda", name="ws")
    rc = L.load().tmix_cfg_rescale_factors(_p(eps.view), L.F16, _p(fac2.view), _p(ws2.view), K, 4, hw, L.STEP_PLAIN, rows, seeds, _p(prm.view), 6, 0.7, _st())
    torch.cuda.synchronize()
    assert rc == 0
    fac2.assert_untouched()
    fac2.assert_all_written()
    ws2.assert_untouched()
    assert torch.equal(fac2.view[:, 0], want[:, 0]) and torch.equal(fac2.view[:, 1:], torch.ones(seeds, rows - 2, device="cuda"))


def test_co_batched_seeds_equal_seeds_one_at_a_time():
    for mode, K, rows in (("fusion", 3, 4), ("resample", 3, 4), ("plain", 3, 4), ("plain", 1, 2)):
        eps = _make_eps(np.random.RandomState(8), 3, rows, 37, 41, -100.0, 1.0, "f32")
        all_ = _factors(eps, "f32", mode, K, rows, 3, 9.0, 0.7)[1]
        for sd in range(3):
            one = _factors(eps[sd * rows:(sd + 1) * rows], "f32", mode, K, rows, 1, 9.0, 0.7)[1]
            assert torch.equal(one, all_[sd:sd + 1]), (mode, sd)


def test_factors_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    K, rows, seeds = 3, 4, 2
    eps = _make_eps(np.random.RandomState(9), seeds, rows, 3, 5, 0.0, 1.0, "f32")
    fac = dense_guarded((seeds, rows - 1), F32, rows=8, device="cuda", name="factors")
    ws = dense_guarded((1, lib.tmix_cfg_rescale_ws_doubles(rows, seeds)), torch.int64, rows=1, device="cuda", name="ws")
    prm = torch.tensor([0, 0, 0, 0, 0, 0, 9.0, 0], dtype=F32).cuda()
    ok = dict(eps=_p(eps), dt=L.F32, fac=_p(fac.view), ws=_p(ws.view), K=K, C=4, hw=15, mode=L.STEP_FUSION, rows=rows, seeds=seeds, prm=_p(prm), slot=6, phi=0.7)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.tmix_cfg_rescale_factors(a["eps"], a["dt"], a["fac"], a["ws"], a["K"], a["C"], a["hw"], a["mode"], a["rows"], a["seeds"], a["prm"],
                                            a["slot"], a["phi"], _st())
    for k in ("eps", "fac", "ws", "prm"):
        assert rc(**{k: None}) == L.EINVAL, k
    assert rc(dt=9) == L.EINVAL and rc(mode=7) == L.EINVAL and rc(K=0) == L.EINVAL
    assert rc(C=1, hw=1) == L.ESHAPE and rc(rows=K) == L.ESHAPE and rc(seeds=0) == L.ESHAPE and rc(seeds=65536) == L.ESHAPE
    assert rc(slot=8) == L.EINVAL and rc(slot=-1) == L.EINVAL
    for phi in (-0.5, 1.5, float("nan"), float("inf")):
        assert rc(phi=phi) == L.EINVAL and b"phi" in lib.tmix_last_error_string()
    torch.cuda.synchronize()
    for f in (fac, ws):                                             # nothing was launched: both buffers still hold the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name
    assert rc() == 0
    torch.cuda.synchronize()
    fac.assert_all_written()


def test_ops_wrappers():
    from tweediemix_amd import guidance as G, lib as L, ops
    c = Case("dev", "fusion", "bf16", 3, 3, 37, 41, seed=80, soft=True)
    fac = ops.cfg_rescale_factors(c.eps_t, c.seeds, L.STEP_FUSION, c.K, c.prm, 6, 0.7)
    torch.cuda.synchronize()
    ref = np.stack([G.rescale_factors_reference(L.STEP_FUSION, c.eps[s * c.rows:(s + 1) * c.rows], c.K, c.g, 0.7) for s in range(c.seeds)])
    assert tuple(fac.shape) == (3, 3) and ulps(fac.cpu().numpy(), ref).max() <= 1
    c.fac_t, c.fac = fac, fac.cpu().numpy()
    ref, ref0 = c.reference()
    o0 = torch.empty_like(c.x_t)
    ox = ops.fused_tweedie_step_rs_dev(c.x_t, c.eps_t, c.m_t, L.STEP_FUSION, c.K, c.prm, fac, out_x0=o0)
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(o0.cpu().numpy(), ref0)
    m = Case("ms", "fusion", "f32", 3, 3, 37, 41, "second", seed=81, soft=True)
    ref, ref0 = m.reference()
    prev = m.prev_t.clone()
    ox = ops.fused_tweedie_step_rs_dev(m.x_t, m.eps_t, m.m_t, L.STEP_FUSION, m.K, m.prm, m.fac_t, x0_prev=prev)
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(prev.cpu().numpy(), ref0)


# ------------------------------------------------------------------------------------------------ step entries == restatement
class Case:
    """the inputs of one launch of an rs step entry (numpy fp32 + device tensors): entry "dev" (DDIM move; order: "step" | "last") or "ms" (multistep
    move; order: a key of ORDERS); factors drawn in [0.3, 1.2]; shared: one mask set for all seeds"""

    def __init__(self, entry, mode, dt, K, seeds, h, w, order=None, shared=False, seed=0, soft=False):
        from tweediemix_amd import ops
        rng = np.random.RandomState(seed + 7 * K + 131 * seeds + h)
        order = order or ("second" if entry == "ms" else "step")
        self.entry, self.mode, self.dt, self.K, self.seeds, self.h, self.w, self.order, self.shared = entry, mode, dt, K, seeds, h, w, order, shared
        self.rows = 2 if mode == "plain" else K + 1
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = np.float16 if dt == "f16" else None
        self.g = 7.5
        r = lambda *s: rng.randn(*s).astype(NF)
        self.x, self.prev = r(seeds, 4, h, w), r(seeds, 4, h, w)
        self.eps_t = torch.from_numpy(r(seeds * self.rows, 4, h, w)).to(DT[dt]).cuda()
        self.eps = self.eps_t.float().cpu().numpy()
        ns = 1 if shared else seeds
        self.masks = rng.rand(ns, K, 1, h, w).astype(NF) if soft else (rng.rand(ns, K, 1, h, w) > 0.5).astype(NF)
        self.fac = (0.3 + 0.9 * rng.rand(seeds, self.rows - 1)).astype(NF)
        self.sa, self.s1, self.san, self.s1n = ops.step_coeffs(NF(0.2345), NF(0.3456))
        if entry == "ms":
            self.cx, self.c0, self.c1, self.is_last = ORDERS[order]
            self.prm = torch.tensor([781.0, self.sa, self.s1, self.cx, self.c0, self.c1, float(self.is_last), self.g], dtype=F32).cuda()
            self.cx, self.c0, self.c1 = (float(v) for v in self.prm[3:6].cpu())                # the fp32 values the kernel reads
        else:
            self.is_last = int(order == "last")
            self.prm = torch.tensor([781.0, self.sa, self.s1, self.san, self.s1n, float(self.is_last), self.g, 0.0], dtype=F32).cuda()
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.prev_t, self.fac_t = c(self.x), c(self.masks), c(self.prev), c(self.fac)

    def launch(self, out_x, out_x0, prev=None, x=None, eps=None, masks=None, prm=None, fac="own", seeds=None, rows=None, mode=None, K=None, dt=None,
               parent=False):
        """raw ABI call; every tensor argument defaults to the case's own; parent: the entry without factors.  Returns the code."""
        from tweediemix_amd import lib as L
        lib = L.load()
        mss = 0 if self.shared else self.K * self.hw
        head = [_p(self.x_t if x is None else x), _p(self.eps_t if eps is None else eps), _dt(self.dt) if dt is None else dt,
                _p(self.m_t if masks is None else masks), mss, _p(out_x), _p(out_x0)]
        tail = [self.K if K is None else K, 4, self.hw, _mode(self.mode) if mode is None else mode, self.rows if rows is None else rows,
                self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm)]
        if not parent:
            tail.append(_p(self.fac_t) if isinstance(fac, str) else _p(fac))
        tail.append(_st())
        if self.entry == "ms":
            fn = lib.tmix_fused_tweedie_step_ms_dev if parent else lib.tmix_fused_tweedie_step_ms_rs_dev
            return fn(*head, _p(prev), *tail)
        fn = lib.tmix_fused_tweedie_step_dev if parent else lib.tmix_fused_tweedie_step_rs_dev
        return fn(*head, *tail)

    def run(self, **kw):
        out_x, out_x0 = torch.empty_like(self.x_t), torch.empty_like(self.x_t)
        prev = self.prev_t.clone()
        assert self.launch(out_x, out_x0, prev, **kw) == 0
        torch.cuda.synchronize()
        return out_x, out_x0, prev

    def reference(self):
        from tweediemix_amd import guidance as G
        ox, o0 = [], []
        for sd in range(self.seeds):
            x, e, m, f = self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows], self.masks[0 if self.shared else sd], self.fac[sd]
            if self.entry == "ms":
                a, b = G.rescaled_multistep_reference(_mode(self.mode), x, e, m, self.prev[sd:sd + 1], f, self.g, self.sa, self.s1, self.cx, self.c0,
                                                      self.c1, self.is_last, self.lowp)
            else:
                a, b = G.rescaled_step_reference(_mode(self.mode), x, e, m, self.K, f, self.g, self.sa, self.s1, self.san, self.s1n, self.is_last, self.lowp)
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self):
        out_x, out_x0, prev = self.run()
        ref, ref0 = self.reference()
        what = (self.entry, self.mode, self.dt, self.K, self.seeds, self.h, self.w, self.order, self.shared)
        assert ref.dtype == NF and ref0.dtype == NF
        assert np.array_equal(out_x.cpu().numpy(), ref), what
        assert np.array_equal(out_x0.cpu().numpy(), ref0), what
        if self.entry == "ms":
            assert np.array_equal(prev.cpu().numpy(), ref0), what


def _entry_modes():
    return [("dev", m) for m in MODES] + [("ms", m) for m in MODES[:2]]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("entry,mode", _entry_modes())
def test_step_entries_equal_the_restatement_sweep(entry, mode, dt):
    """K x seeds x (first | second | last, or step | last) x shape x (shared | per-seed masks): hw = 1, 5 x 7 (under one workgroup), 16 x 16 (four)"""
    i = 0
    orders = list(ORDERS) if entry == "ms" else ["step", "last"]
    for h, w in ((1, 1), (5, 7), (16, 16)):
        for K in (1, 2, 3, 4):
            for seeds in (1, 3):
                for order in orders:
                    Case(entry, mode, dt, K, seeds, h, w, order, shared=bool(i & 1), seed=i, soft=bool(i & 2)).check()
                    i += 1
    for shared in (False, True):
        Case(entry, mode, dt, 4, 3, 5, 7, orders[0], shared=shared, seed=900, soft=True).check()


@pytest.mark.parametrize("entry,mode", _entry_modes())
def test_all_factors_one_is_the_parent_entry_bit_for_bit(entry, mode):
    for dt in DT:
        for order in (list(ORDERS) if entry == "ms" else ["step", "last"]):
            c = Case(entry, mode, dt, 3, 3, 37, 41, order, seed=10, soft=True)
            ones = torch.ones_like(c.fac_t)
            ox, o0, pv = c.run(fac=ones)
            px, p0, pp = c.run(parent=True)
            assert torch.equal(ox, px) and torch.equal(o0, p0) and torch.equal(pv, pp), (entry, mode, dt, order)
            qx, q0, _ = c.run()                                 # and the drawn factors do change the result
            assert not torch.equal(q0, p0)


@pytest.mark.parametrize("mode", MODES[:2])
def test_x0_of_the_multistep_rs_entry_is_the_ddim_rs_entrys(mode):
    for dt in DT:
        for order in ("first", "last"):
            m = Case("ms", mode, dt, 3, 3, 37, 41, order, seed=20, soft=True)
            mx, m0, mp = m.run()
            d = Case("dev", mode, dt, 3, 3, 37, 41, "last" if order == "last" else "step", seed=20, soft=True)
            assert torch.equal(d.eps_t, m.eps_t) and torch.equal(d.fac_t, m.fac_t) and torch.equal(d.x_t, m.x_t)
            dx, d0, _ = d.run()
            assert torch.equal(m0, d0) and torch.equal(mp, d0), (mode, dt, order)
            if order == "last":
                assert torch.equal(mx, d0) and torch.equal(dx, d0)


@pytest.mark.parametrize("entry,mode", _entry_modes())
def test_in_place_guard_bands_and_untouched_inputs(entry, mode):
    c = Case(entry, mode, "f32", 3, 3, 37, 41, seed=40, soft=True)
    ox, o0, pv = c.run()
    S, n = c.seeds, c.n
    flat = lambda t, name: Frame.of(t.reshape(1, -1), name=name).seal()
    eps, masks, prm, fac = flat(c.eps_t, "eps"), flat(c.m_t, "masks"), flat(c.prm, "params"), flat(c.fac_t, "factors")
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
        assert c.launch(outx.view, out0.view, prev.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view, fac=fac.view) == 0
        torch.cuda.synchronize()
        for f in (outx, out0):
            f.assert_untouched()
            f.assert_all_written()
        prev.assert_untouched()
        for f in (eps, masks, prm, fac) + (() if in_place else (x,)):
            f.assert_unchanged()
        assert torch.equal(outx.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
        if entry == "ms":
            assert torch.equal(prev.view.reshape(o0.shape), pv)
        # without out_x0, in place
        x2, prev2 = c.x_t.clone(), c.prev_t.clone()
        assert c.launch(x2, None, prev2, x=x2) == 0
        torch.cuda.synchronize()
        assert torch.equal(x2, ox)


def test_second_pass_of_the_step_kernels_grid_stride_loop():
    """hw = 384 x 384: n = 589,824 > 2048 workgroups x 256 threads; the factors come from the factors kernel (72 passes of its own loop)"""
    for entry in ("dev", "ms"):
        c = Case(entry, "fusion", "f32", 3, 1, 384, 384, shared=True, seed=50, soft=True)
        assert c.n > 2048 * 256 and c.n > RS_P * RS_THREADS
        rc, fac, _ = _factors(c.eps_t, "f32", "fusion", 3, 4, 1, c.g, 0.7, prm=c.prm, slot=7 if entry == "ms" else 6)
        ref = _factors_ref(c.eps_t, "f32", "fusion", 3, 4, 1, c.g, 0.7)
        assert rc == 0 and ulps(fac.cpu().numpy(), ref).max() <= 1
        c.fac_t, c.fac = fac, fac.cpu().numpy()
        c.check()


@pytest.mark.parametrize("entry", ["dev", "ms"])
def test_step_error_codes_without_a_launch(entry):
    from tweediemix_amd import lib as L
    lib = L.load()
    c = Case(entry, "fusion", "f32", 3, 2, 3, 5, seed=70)
    out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
    out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
    prev = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="x0_prev")
    go = lambda **kw: c.launch(out_x.view, out_x0.view, prev.view, **kw)
    assert go(fac=None) == L.EINVAL and b"factors" in lib.tmix_last_error_string()
    assert c.launch(None, out_x0.view, prev.view) == L.EINVAL
    if entry == "ms":
        assert c.launch(out_x.view, out_x0.view, None) == L.EINVAL and b"x0_prev" in lib.tmix_last_error_string()
        assert go(mode=L.STEP_RESAMPLE) == L.EINVAL and b"mode" in lib.tmix_last_error_string()
    assert go(mode=7) == L.EINVAL and go(K=0) == L.EINVAL and go(dt=9) == L.EINVAL
    assert go(rows=c.K) == L.ESHAPE and go(seeds=0) == L.ESHAPE and go(seeds=65536) == L.ESHAPE
    torch.cuda.synchronize()
    for f in (out_x, out_x0, prev):
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


K3, H, W = 3, 16, 16
G_RUN, PHI = 7.5, 0.7
ROWS = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2}
PLAIN_ENTRIES = ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev", "tmix_fused_tweedie_step_ms_dev")
RS_ENTRIES = ("tmix_cfg_rescale_factors", "tmix_fused_tweedie_step_rs_dev", "tmix_fused_tweedie_step_ms_rs_dev")


def _cfg(S, n=10, R=1, J=1, g=G_RUN):
    return S.make_config(guidance_scale=g, n_timesteps=n, t_cond=0.2, t_stop=0.8, resampling_steps=R, jumping_steps=J, resolution_h=H * 8,
                         resolution_w=W * 8)


def _standin_eps(i, rows, seeds, dtype=torch.float32):
    return torch.randn(seeds * rows, 4, H, W, generator=torch.Generator().manual_seed(4000 + i)).to(dtype)


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step / factors entry the sampler calls"""
    from tweediemix_amd import lib as L
    lib, calls = L.load(), []
    for name in PLAIN_ENTRIES + RS_ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _restate(mode, ms, x, eps, masks, prev, fac, prm, lowp=None):
    """one seed's step from the uploaded parameters (the DDIM or the multistep layout) and the given factors -> (out, x0)"""
    from tweediemix_amd import guidance as G
    p = [NF(v) for v in prm]
    if ms:
        return G.rescaled_multistep_reference(mode, x, eps, masks, prev, fac, p[7], p[1], p[2], p[3], p[4], p[5], bool(p[6]), lowp)
    return G.rescaled_step_reference(mode, x, eps, masks, K3, fac, p[6], p[1], p[2], p[3], p[4], bool(p[5]), lowp)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("lora,seeds,dtype", [(False, 1, torch.float32), (True, 1, torch.float16), (False, 2, torch.bfloat16)])
def test_sampler_standin_unet_every_step_equals_the_restatement(lora, seeds, dtype, solver, monkeypatch):
    """n = 10, K = 3, partition masks, one resampling and one jumping step, g = 7.5, phi = 0.7, the stand-in returning fp32 / fp16 / bf16 eps.  A spy copies
    the factors buffer at every step: each factor is within one ulp of the restatement on that step's eps, and the step restated with the DEVICE's factors
    equals the state by equality -- at all 13 steps (start phase, resampling, look-ahead, plain and fusion steps, both entries).  A whole-trajectory
    comparison with numpy factors is not made: one ulp in a factor propagates."""
    from tweediemix_amd import guidance as G, lib as L, masks as M, sampler as S
    n, R, J = 10, 1, 1
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W)
    mk = masks.cpu().numpy()
    lowp = np.float16 if dtype == torch.float16 else None
    kw = dict(solver="dpmpp2m", timestep_spacing="logsnr") if solver != "ddim" else {}
    tw = S.Tweediemix(_cfg(S, n, R, J), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, lora=lora, n_seeds=seeds, guidance_rescale=PHI, **kw)
    log, rec = [], []

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return _standin_eps(len(log) - 1, ROWS[kind], seeds, dtype).cuda()
    tw._unet = unet
    real = tw._fused_step

    def spy(eps_ptr, eps_dt, rows, mode, st, ms=False):
        prev = None if tw._x0_prev is None else tw._x0_prev.clone()
        real(eps_ptr, eps_dt, rows, mode, st, ms)
        torch.cuda.synchronize()
        rec.append((rows, mode, ms, prev, tw._rs_factors[:seeds * (rows - 1)].reshape(seeds, rows - 1).cpu().numpy().copy(), tw.step_params.cpu().numpy().copy(),
                    tw.x_state.cpu().numpy().copy(), tw.x0_state.cpu().numpy().copy()))
    tw._fused_step = spy
    calls = _spy_entries(monkeypatch)
    xT = torch.randn(seeds, 4, H, W, generator=torch.Generator().manual_seed(41 + seeds))
    out = tw.run_fusion(xT.clone())
    assert len(log) == len(rec) == n + 2 * R + J == 13 and torch.isfinite(out).all()
    assert calls[0::2] == [RS_ENTRIES[0]] * 13 and set(calls[1::2]) <= set(RS_ENTRIES[1:]) and len(calls) == 26      # factors, then the rs step: never another entry
    n_ms = sum(c == RS_ENTRIES[2] for c in calls)
    assert n_ms == (9 if solver != "ddim" else 0)
    worst = 0
    for ci, ((kind, t, x), (rows, mode, ms, prev, fac, prm, after, x0s)) in enumerate(zip(log, rec)):
        assert rows == ROWS[kind] and prm[0] == t and prm[7 if ms else 6] == NF(G_RUN)
        eps = _standin_eps(ci, rows, seeds, dtype).float().numpy()
        xb = x.cpu().numpy()
        for sd in range(seeds):
            e = eps[sd * rows:(sd + 1) * rows]
            ref = G.rescale_factors_reference(mode, e, K3, G_RUN, PHI, lowp)
            d = ulps(fac[sd], ref)
            assert d.max() <= 1, (ci, kind, t, sd, fac[sd], ref)
            worst = max(worst, int(d.max()))
            used = G.rows_read(mode, K3)
            assert np.all(fac[sd, :used] < 1.0) and np.all(fac[sd, :used] > 1.0 - PHI) and np.all(fac[sd, used:] == 1.0)
            a, b = _restate(mode, ms, xb[sd:sd + 1], e, mk if mode == L.STEP_FUSION else None, None if prev is None else prev[sd:sd + 1].cpu().numpy(), fac[sd], prm, lowp)
            assert np.array_equal(after[sd:sd + 1], a) and np.array_equal(x0s[sd:sd + 1], b), (ci, kind, t, sd)
    assert np.array_equal(out.cpu().numpy(), rec[-1][6])
    print(f"stand-in run lora={lora} seeds={seeds} {dtype} {solver}: worst factor distance {worst} ulp")


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


@pytest.mark.parametrize("kind,kw", [("custom", {}), ("lora", MS)])
def test_tiny_unet_graph_replay_equals_eager(kind, kw, monkeypatch):
    """the factors are deterministic, so a captured run equals the eager one bit for bit; every captured step has a key of its own ending in "rs" """
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    T = _Tiny(kind)
    eager, graph = T.sampler(False, guidance_rescale=PHI, **kw), T.sampler(True, guidance_rescale=PHI, **kw)
    a, b = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert eager.unet_calls == graph.unet_calls and len(eager.unet_calls) == 13
    keys = sorted(graph.graphs)
    assert keys and all(k[-1] == "rs" for k in keys)
    if kw:
        assert sorted(k for k in keys if len(k) == 4) == sorted([("fusion", L.STEP_FUSION, "ms", "rs"), ("fusion_base", L.STEP_FUSION, "ms", "rs"),
                                                                 ("plain", L.STEP_PLAIN, "ms", "rs")])
        assert sorted(k for k in keys if len(k) == 3) == sorted([("start", L.STEP_RESAMPLE, "rs"), ("plain", L.STEP_PLAIN, "rs"), ("start", L.STEP_PLAIN, "rs")])
    else:
        assert keys == sorted([("start", L.STEP_RESAMPLE, "rs"), ("plain", L.STEP_PLAIN, "rs"), ("start", L.STEP_PLAIN, "rs"), ("fusion", L.STEP_FUSION, "rs")])
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()             # every captured step replayed from the first one on
    assert torch.equal(again, a) and sorted(graph.graphs) == keys
    assert not torch.equal(a, T.sampler(False, **kw).run_fusion(T.xT[0:1].clone()).cpu())     # and it is not the run without the rescale


def test_zero_spelled_out_is_the_sampler_of_today(monkeypatch):
    """guidance_rescale=0.0 equals the constructor call without it: the same bits, step entries, UNet calls, plan launch names and graph keys, and neither
    the factors launch nor an rs entry is ever called"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    names = lambda p: [getattr(fn, "__name__", "") for fn, _a in p.ops]
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(guidance_rescale=0.0)):
            tw = T.sampler(graphs, **kw)
            out = tw.run_fusion(T.xT[0:1].clone()).cpu()
            runs.append((out, list(calls), tw))
            calls[:] = []
    for (oa, ca, ta), (ob, cb, tb) in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert torch.equal(oa, ob) and ca == cb and ta.unet_calls == tb.unet_calls and len(ta.unet_calls) == 13
        assert sorted(ta.plans) == sorted(tb.plans) and sorted(ta.graphs) == sorted(tb.graphs)
        for k in ta.plans:
            assert names(ta.plans[k]) == names(tb.plans[k]) and len(names(ta.plans[k])) > 50, k
        assert tb._rs_factors is None and tb._rs_ws is None
    assert runs[0][1] == [PLAIN_ENTRIES[0]] * 13
    assert not any(c in RS_ENTRIES for r in runs for c in r[1])
    assert torch.equal(runs[0][0], runs[2][0]) and all(len(k) == 2 for k in runs[3][2].graphs)


def test_tiny_unet_two_window_canvas_equals_rs_step_plus_consensus(monkeypatch):
    """16 x 24 canvas, two 16 x 16 windows overlapping by 8, the solver run (DDIM entry on the first timestep and the look-ahead, multistep behind): every
    step equals the rs step restated per window -- with that window's own factors, each within one ulp of its restatement on the eps the plan produced --
    followed by the consensus restatement of tests/test_canvas_gpu.py"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from test_canvas_gpu import consensus_np
    from tweediemix_amd import guidance as G, lib as L, masks as M
    T = _Tiny("custom")
    ch, cw = 16, 24
    masks = M.build_masks(M.partition_rectangle_masks(T.K, ch * 8, cw * 8, seed=3), ch, cw)
    tw = T.sampler(False, masks=masks, canvas=dict(height=ch * 8, width=cw * 8, overlap=64), guidance_rescale=PHI, **MS)
    assert tw.windows == [(0, 0), (0, 8)] and tw.n_seeds == 2
    rec, real = [], tw._enqueue_step

    def spy(kind, mode, ms=False):
        before, prev = tw.x_state.clone(), tw._x0_prev.clone()
        real(kind, mode, ms)
        torch.cuda.synchronize()
        rows = tw.plan(kind).B // 2
        rec.append((kind, mode, ms, before, prev, tw.plan(kind).eps.clone(), tw.step_params.clone(), tw.x_state.clone(), tw.x0_state.clone(),
                    tw._rs_factors[:2 * (rows - 1)].reshape(2, rows - 1).clone()))
    tw._enqueue_step = spy
    xT = torch.randn(1, 4, ch, cw, generator=torch.Generator().manual_seed(31))
    out = tw.run_fusion(xT.clone())
    assert out.shape == (1, 4, ch, cw) and torch.isfinite(out).all() and len(rec) == 13
    assert [r[2] for r in rec] == [False] * 3 + [True] + [False] + [True] * 8
    mw = tw.masks.cpu().numpy()
    differ = False
    for kind, mode, ms, before, prev, eps, prm, after, x0s, fac in rec:
        rows = eps.shape[0] // 2
        e, xb, pv, f, p = eps.cpu().numpy(), before.cpu().numpy(), prev.cpu().numpy(), fac.cpu().numpy(), prm.cpu().numpy()
        moved, est = [], []
        for b in range(2):
            eb = e[b * rows:(b + 1) * rows]
            assert ulps(f[b], G.rescale_factors_reference(mode, eb, T.K, G_RUN, PHI)).max() <= 1, (kind, b)
            a, z = _restate(mode, ms, xb[b:b + 1], eb, mw[b] if mode == L.STEP_FUSION else None, pv[b:b + 1], f[b], p)
            moved.append(a)
            est.append(z)
        differ = differ or not np.array_equal(f[0], f[1])
        want = consensus_np(np.concatenate(moved).reshape(1, 2, 4, 16, 16), tw.windows, ch, cw)[0].reshape(2, 4, 16, 16)
        assert np.array_equal(after.cpu().numpy(), want), (kind, p[0])
        assert np.array_equal(x0s.cpu().numpy(), np.concatenate(est)), (kind, p[0])
        assert torch.equal(after[0, :, :, 8:], after[1, :, :, :8])
    assert differ                                                  # statistics are per window: the two windows do carry different factors


def test_set_keep_is_refused_before_any_launch(monkeypatch):
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    tw = T.sampler(False, guidance_rescale=PHI)
    z = torch.zeros(1, 4, T.h, T.w)
    with pytest.raises(ValueError, match=r"set_keep.*guidance_rescale=0.7"):
        tw.set_keep(z, z[:, :1], z)
    assert calls == [] and tw._keep is None and tw.plans == {} and tw.unet_calls == []
    with pytest.raises(ValueError, match="guidance_rescale"):
        T.sampler(False, guidance_rescale=1.5)


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
    fs = _load(script, "fs_rescale_gpu_" + script[:-3])
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
    lat = fs.main(common + ["--guidance_rescale", "0.7", "--output_path_all", str(tmp_path / "rs")]).cpu()
    ref = fs.main(common + ["--output_path_all", str(tmp_path / "plain")]).cpu()
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all() and not torch.equal(lat, ref)
    assert torch.equal(torch.load(tmp_path / "rs" / "p_5.latent.pt"), lat)
    assert Image.open(tmp_path / "rs" / "p_5.png").size == (128, 128)
    with pytest.raises(SystemExit, match=r"--guidance_rescale 0.7 does not combine with --keep_latents"):
        fs.main(common + ["--guidance_rescale", "0.7", "--keep_latents", str(tmp_path / "rs" / "p_5.latent.pt"), "--reroll", "1",
                          "--output_path_all", str(tmp_path / "keep")])
