"""GPU: few-step sampling -- tmix_fused_tweedie_step_ms_dev, Tweediemix(solver="dpmpp2m", timestep_spacing="logsnr"), --solver / --timestep_spacing.

The kernel is compared with the numpy fp32 restatement tweediemix_amd.solver.multistep_step_reference (x0 by the operations of the DDIM step kernel,
then m = c0 x0 [+ c1 x0_prev], out = cx x + m: every product and sum rounded on its own) by np.array_equal / torch.equal, never by a tolerance;
tests/test_solver_cpu.py ties the restatement's x0 to oracle.tweedie_oracle.  The one inequality in this file is the Gaussian toy's (closed form)."""
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
MODES = ("fusion", "plain")
# (cx, c0, c1, is_last): a first-order step, a second-order step, the last step (whose coefficients are not read)
ORDERS = {"first": (0.8125, 0.3217, 0.0, 0), "second": (0.8125, 0.4021, -0.0804, 0), "last": (0.0, 1.0, 0.0, 1)}
SHAPES = ((1, 1), (5, 7), (16, 16))


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _mode(name):
    from tweediemix_amd import lib as L
    return {"fusion": L.STEP_FUSION, "plain": L.STEP_PLAIN, "resample": L.STEP_RESAMPLE}[name]


class Case:
    """the inputs of one launch (numpy fp32 + device tensors): seeds x [C=4,h,w]; shared: one mask set for all seeds"""

    def __init__(self, mode, dt, K, seeds, h, w, order="second", shared=False, seed=0, soft=False):
        from tweediemix_amd import ops
        rng = np.random.RandomState(seed + 7 * K + 131 * seeds + h)
        self.mode, self.dt, self.K, self.seeds, self.h, self.w, self.order, self.shared = mode, dt, K, seeds, h, w, order, shared
        self.rows = 2 if mode == "plain" else K + 1
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = np.float16 if dt == "f16" else None
        self.at, self.g = NF(0.2345), 0.8
        r = lambda *s: rng.randn(*s).astype(NF)
        self.x, self.prev = r(seeds, 4, h, w), r(seeds, 4, h, w)
        self.eps_t = torch.from_numpy(r(seeds * self.rows, 4, h, w)).to(DT[dt]).cuda()
        self.eps = self.eps_t.float().cpu().numpy()
        ns = 1 if shared else seeds
        self.masks = rng.rand(ns, K, 1, h, w).astype(NF) if soft else (rng.rand(ns, K, 1, h, w) > 0.5).astype(NF)
        self.sa, self.s1, _, _ = ops.step_coeffs(self.at, self.at)
        self.cx, self.c0, self.c1, self.is_last = ORDERS[order]
        self.prm = torch.tensor([781.0, self.sa, self.s1, self.cx, self.c0, self.c1, float(self.is_last), self.g], dtype=F32).cuda()
        self.cx, self.c0, self.c1 = (float(v) for v in self.prm[3:6].cpu())                # the fp32 values the kernel reads
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.prev_t = c(self.x), c(self.masks), c(self.prev)

    def launch(self, out_x, out_x0, prev, x=None, eps=None, masks=None, prm=None, seeds=None, mss=None, rows=None, mode=None, entry="ms", K=None,
               dt=None):
        """raw ABI call; every tensor argument defaults to the case's own.  Returns the code."""
        from tweediemix_amd import lib as L
        lib = L.load()
        if mss is None:
            mss = 0 if self.shared else self.K * self.hw
        head = [_p(self.x_t if x is None else x), _p(self.eps_t if eps is None else eps), {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[self.dt] if dt is None else dt,
                _p(self.m_t if masks is None else masks), mss, _p(out_x), _p(out_x0)]
        tail = [self.K if K is None else K, 4, self.hw, _mode(self.mode) if mode is None else mode, self.rows if rows is None else rows,
                self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm), _st()]
        if entry == "dev":
            return lib.tmix_fused_tweedie_step_dev(*head, *tail)
        return lib.tmix_fused_tweedie_step_ms_dev(*head, _p(prev), *tail)

    def run(self, prev=None, **kw):
        out_x, out_x0 = torch.empty_like(self.x_t), torch.empty_like(self.x_t)
        prev = self.prev_t.clone() if prev is None else prev
        assert self.launch(out_x, out_x0, prev, **kw) == 0
        torch.cuda.synchronize()
        return out_x, out_x0, prev

    def reference(self):
        from tweediemix_amd import solver as SV
        ox, o0 = [], []
        for sd in range(self.seeds):
            a, b = SV.multistep_step_reference(_mode(self.mode), self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows],
                                               self.masks[0 if self.shared else sd], self.prev[sd:sd + 1], self.g, self.sa, self.s1, self.cx, self.c0,
                                               self.c1, self.is_last, self.lowp)
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self):
        out_x, out_x0, prev = self.run()
        ref, ref0 = self.reference()
        what = (self.mode, self.dt, self.K, self.seeds, self.h, self.w, self.order, self.shared)
        assert ref.dtype == NF and ref0.dtype == NF
        assert np.array_equal(out_x.cpu().numpy(), ref), what
        assert np.array_equal(out_x0.cpu().numpy(), ref0) and np.array_equal(prev.cpu().numpy(), ref0), what


# ------------------------------------------------------------------------------------------------ kernel == restatement
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_restatement_sweep(mode, dt):
    """K x seeds x order x shape x (shared | per-seed masks): hw = 1 (n = 4), 5 x 7 (n = 140, under one workgroup), 16 x 16 (n = 1024, four workgroups)"""
    i = 0
    for h, w in SHAPES:
        for K in (1, 2, 4):
            for seeds in (1, 3):
                for order in ORDERS:
                    Case(mode, dt, K, seeds, h, w, order, shared=bool(i & 1), seed=i, soft=bool(i & 2)).check()
                    i += 1
    for shared in (False, True):                               # both mask layouts at one fixed point, whatever the cycling above gave it
        Case(mode, dt, 4, 3, 5, 7, "second", shared=shared, seed=900, soft=True).check()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
def test_out_x0_is_the_ddim_entrys_out_x0(mode, dt):
    """tmix_fused_tweedie_step_dev on the same x / eps / masks / sa / s1 / g (its own parameter layout): the same x0, bit for bit"""
    for order in ORDERS:
        c = Case(mode, dt, 3, 3, 37, 41, order, seed=10, soft=True)
        _, o0, prev = c.run()
        dev_prm = torch.tensor([781.0, c.sa, c.s1, 0.6, 0.8, 0.0, c.g, 0.0], dtype=F32).cuda()
        dx, d0 = torch.empty_like(c.x_t), torch.empty_like(c.x_t)
        assert c.launch(dx, d0, None, prm=dev_prm, entry="dev") == 0
        torch.cuda.synchronize()
        assert torch.equal(o0, d0) and torch.equal(prev, d0), (mode, dt, order)
        if order == "last":                                     # ... and the last step's latent is that x0 under both
            ms_x, _, _ = c.run()
            assert torch.equal(ms_x, d0)


@pytest.mark.parametrize("mode", MODES)
def test_nan_history_stays_out_of_a_first_order_step(mode):
    for dt in DT:
        for order in ("first", "last"):
            c = Case(mode, dt, 3, 3, 5, 7, order, seed=20)
            want_x, want_0, _ = c.run()
            prev = torch.full_like(c.prev_t, float("nan"))
            ox, o0, prev = c.run(prev=prev)
            assert torch.isfinite(ox).all() and torch.isfinite(o0).all() and torch.isfinite(prev).all(), (mode, dt, order)
            assert torch.equal(ox, want_x) and torch.equal(o0, want_0) and torch.equal(prev, want_0)
    # a second-order step does read it
    ox, o0, prev = Case(mode, "f32", 3, 1, 5, 7, "second", seed=21).run(prev=torch.full((1, 4, 5, 7), float("nan"), device="cuda"))
    assert torch.isnan(ox).all() and torch.isfinite(o0).all() and torch.equal(prev, o0)


@pytest.mark.parametrize("mode", MODES)
def test_in_place_equals_out_of_place(mode):
    for order in ORDERS:
        c = Case(mode, "f32", 3, 3, 37, 41, order, seed=30, soft=True)
        ox, o0, pv = c.run()
        x, o0b, prev = c.x_t.clone(), torch.empty_like(c.x_t), c.prev_t.clone()
        assert c.launch(x, o0b, prev, x=x) == 0
        torch.cuda.synchronize()
        assert torch.equal(x, ox) and torch.equal(o0b, o0) and torch.equal(prev, pv)
        # without out_x0
        x, prev = c.x_t.clone(), c.prev_t.clone()
        assert c.launch(x, None, prev, x=x) == 0
        torch.cuda.synchronize()
        assert torch.equal(x, ox) and torch.equal(prev, pv)


@pytest.mark.parametrize("mode", MODES)
def test_guard_bands_and_untouched_inputs(mode):
    """every pointer in a guard-band frame (tests/layout_frames.py): nothing outside the views is written, no input changes, the history buffer is
    rewritten inside its view only; in place and out of place"""
    c = Case(mode, "f32", 3, 3, 37, 41, "second", seed=40, soft=True)
    ox, o0, _ = c.run()
    S, n = c.seeds, c.n
    flat = lambda t, name: Frame.of(t.reshape(1, -1), name=name).seal()
    eps, masks, prm = flat(c.eps_t, "eps"), flat(c.m_t, "masks"), flat(c.prm, "params")
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
        assert c.launch(outx.view, out0.view, prev.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view) == 0
        torch.cuda.synchronize()
        for f in (outx, out0):
            f.assert_untouched()
            f.assert_all_written()
        prev.assert_untouched()
        for f in (eps, masks, prm) + (() if in_place else (x,)):
            f.assert_unchanged()
        assert torch.equal(outx.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
        assert torch.equal(prev.view.reshape(o0.shape), o0)


def test_second_pass_of_the_grid_stride_loop():
    """hw = 384 x 384: n = 589,824 > 2048 workgroups x 256 threads, so threads of the capped grid take a second element"""
    c = Case("fusion", "f32", 3, 1, 384, 384, "second", shared=True, seed=50, soft=True)
    assert c.n == 4 * 384 * 384 > 2048 * 256
    c.check()


@pytest.mark.parametrize("mode", MODES)
def test_co_batched_launch_equals_seeds_one_at_a_time(mode):
    c = Case(mode, "f16", 3, 3, 37, 41, "second", seed=60, soft=True)
    ox, o0, pv = c.run()
    for sd in range(c.seeds):
        a, b, p = torch.empty_like(c.x_t[sd:sd + 1]), torch.empty_like(c.x_t[sd:sd + 1]), c.prev_t[sd:sd + 1].clone()
        assert c.launch(a, b, p, x=c.x_t[sd:sd + 1], eps=c.eps_t[sd * c.rows:(sd + 1) * c.rows], masks=c.m_t[sd], seeds=1) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, ox[sd:sd + 1]) and torch.equal(b, o0[sd:sd + 1]) and torch.equal(p, pv[sd:sd + 1]), sd


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    c = Case("fusion", "f32", 3, 2, 3, 5, seed=70)
    out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
    out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
    prev = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="x0_prev")
    go = lambda **kw: c.launch(out_x.view, out_x0.view, prev.view, **kw)
    assert c.launch(out_x.view, out_x0.view, None) == L.EINVAL and b"x0_prev" in lib.tmix_last_error_string()
    assert c.launch(None, out_x0.view, prev.view) == L.EINVAL
    assert go(mode=L.STEP_RESAMPLE) == L.EINVAL and b"mode" in lib.tmix_last_error_string()
    assert go(mode=7) == L.EINVAL and go(K=0) == L.EINVAL and go(dt=9) == L.EINVAL
    assert go(rows=c.K) == L.ESHAPE and go(seeds=0) == L.ESHAPE and go(seeds=65536) == L.ESHAPE
    torch.cuda.synchronize()
    for f in (out_x, out_x0, prev):                            # nothing was launched: every buffer still holds the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


def test_ops_wrapper():
    from tweediemix_amd import lib as L, ops
    for shared in (False, True):
        c = Case("fusion", "bf16", 3, 3, 37, 41, "second", shared=shared, seed=80, soft=True)
        ref, ref0 = c.reference()
        o0, prev = torch.empty_like(c.x_t), c.prev_t.clone()
        ox = ops.fused_tweedie_step_ms_dev(c.x_t, c.eps_t, c.m_t[0] if shared else c.m_t, L.STEP_FUSION, c.K, c.prm, prev, out_x0=o0)
        torch.cuda.synchronize()
        assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(o0.cpu().numpy(), ref0) and np.array_equal(prev.cpu().numpy(), ref0)


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


K3, H, W = 3, 16, 16
ROWS = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2}
ENTRIES = ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev", "tmix_fused_tweedie_step_ms_dev")


def _cfg(S, n=10, R=1, J=1):
    return S.make_config(guidance_scale=0.8, n_timesteps=n, t_cond=0.2, t_stop=0.8, resampling_steps=R, jumping_steps=J, resolution_h=H * 8,
                         resolution_w=W * 8)


def _standin_eps(i, rows, seeds):
    """the stand-in UNet: a fixed seeded function of (call index, row)"""
    return torch.randn(seeds * rows, 4, H, W, generator=torch.Generator().manual_seed(4000 + i))


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step entry the sampler calls"""
    from tweediemix_amd import lib as L
    lib, calls = L.load(), []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


@pytest.mark.parametrize("lora,seeds", [(False, 1), (True, 1), (False, 2)])
def test_sampler_standin_unet_every_trajectory_step_equals_the_restatement(lora, seeds, monkeypatch):
    """n = 10 on the log-SNR grid, K = 3, partition masks, one resampling and one jumping step: the state after EVERY trajectory step behind the first
    timestep (= the state handed to the next call, and the final latent) equals the restatement by equality, with the order of every step from the
    rule restated here; only the first timestep and the look-ahead go through the DDIM entry; the UNet is called n + 2R + J times (2R + 1 on the first
    timestep, n - 1 further steps, J look-ahead calls)"""
    from tweediemix_amd import lib as L, masks as M, sampler as S, solver as SV
    n, R, J, g = 10, 1, 1, 0.8
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W)
    mk = masks.cpu().numpy()
    xT = torch.randn(seeds, 4, H, W, generator=torch.Generator().manual_seed(41 + seeds))
    log = []
    tw = S.Tweediemix(_cfg(S, n, R, J), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, lora=lora, n_seeds=seeds, solver="dpmpp2m",
                      timestep_spacing="logsnr")

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return _standin_eps(len(log) - 1, ROWS[kind], seeds).cuda()
    tw._unet = unet
    calls = _spy_entries(monkeypatch)
    out = tw.run_fusion(xT.clone())
    ts = tw.scheduler.timesteps
    assert ts == [901, 770, 612, 427, 243, 108, 39, 12, 4, 1]
    ic, istop = 2, 6                                              # first index at or below 'leading' t = 701 and t = 101
    assert len(log) == len(calls) == n + 2 * R + J == 13
    dev, ms = ENTRIES[0], ENTRIES[2]
    assert calls == [dev] * (2 * R + 1) + [ms] + [dev] * J + [ms] * (n - 2)
    assert [(k, t) for k, t, _x in log[:5]] == [("start", 901), ("plain", 770), ("start", 901), ("plain", 770), ("plain", 612)]
    assert torch.equal(log[4][2], log[5][2])                      # the look-ahead did not move the trajectory
    traj = [3] + list(range(5, 13))                               # call indices of the trajectory steps i = 1 .. 9
    hist, state, prev_mode = np.zeros((seeds, 4, H, W), NF), log[3][2].cpu().numpy(), None
    for i, ci in enumerate(traj, 1):
        kind, t, x = log[ci]
        assert t == ts[i] and np.array_equal(x.cpu().numpy(), state), (i, t)
        fusion = ic <= i <= istop if lora else i >= ic
        assert kind == (("fusion" if (not lora or i < istop) else "fusion_base") if fusion else "plain"), (i, kind)
        mode = L.STEP_FUSION if fusion else L.STEP_PLAIN
        second = i >= 2 and mode == prev_mode
        assert second == (not (i == 1 or i == ic or (lora and i == istop + 1)))
        last = t == 1
        cf = (0.0, 1.0, 0.0) if last else SV.multistep_coeffs(tw.alpha(ts[i - 1]), tw.alpha(t), tw.alpha(ts[i + 1]), second)
        sa, s1 = np.sqrt(NF(tw.alpha(t))), np.sqrt(NF(1) - NF(tw.alpha(t)))
        eps = _standin_eps(ci, ROWS[kind], seeds).numpy()
        rows = ROWS[kind]
        nxt, x0s = [], []
        for sd in range(seeds):
            a, b = SV.multistep_step_reference(mode, state[sd:sd + 1], eps[sd * rows:(sd + 1) * rows], mk, hist[sd:sd + 1], g, sa, s1, *cf, last)
            nxt.append(a)
            x0s.append(b)
        state, hist, prev_mode = np.concatenate(nxt), np.concatenate(x0s), mode
    assert np.array_equal(out.cpu().numpy(), state) and np.array_equal(tw._x0_prev.cpu().numpy(), hist)
    assert np.array_equal(tw.x0_state.cpu().numpy(), hist) and torch.isfinite(out).all()


def test_sampler_gaussian_eps_2m_at_10_steps_is_closer_than_ddim_at_50():
    """the stand-in returns the EXACT eps of scalar Gaussian data N(m, c^2) for every row (so every concept's estimate and their blend are the exact
    posterior mean); no resampling.  The final latent of 2M on the log-SNR grid at n = 10 is closer to the closed form (the Tweedie estimate at t = 1
    of the exact probability-flow state: tests/test_solver_cpu.py's toy_exact) than DDIM 'leading' at n = 50.  m = 0.7, c = 0.5.  Recorded on an
    MI355X: DDIM 2.86e-2, 2M 3.23e-3, ratio 0.113 (the CPU toy's all-PLAIN run of this draw gives 0.286; with the step at index 2 first order, as
    the phase rule makes the first fusion step, it gives 0.1129)."""
    from test_solver_cpu import toy_exact
    from tweediemix_amd import masks as M, sampler as S
    m, c = 0.7, 0.5
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W)
    xT = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(5))
    err = {}
    for name, n, kw in (("ddim50", 50, {}), ("2m10", 10, dict(solver="dpmpp2m", timestep_spacing="logsnr"))):
        tw = S.Tweediemix(_cfg(S, n, 0, 1), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, **kw)

        n_calls = []

        def unet(kind, x, t, tw=tw, n_calls=n_calls):
            n_calls.append(kind)
            a = float(tw.alpha(t))
            e = (np.sqrt(1 - a) * (x.double() - np.sqrt(a) * m) / (a * c * c + 1 - a)).float()
            return e.repeat_interleave(ROWS[kind], dim=0)
        tw._unet = unet
        got = tw.run_fusion(xT.clone()).cpu().numpy().astype(np.float64).reshape(-1)
        assert len(n_calls) == n + 1                              # n steps and one look-ahead call, also under the solver
        exact = toy_exact(m, c, xT.numpy().reshape(-1), float(tw.alpha(tw.scheduler.timesteps[0])), float(tw.alpha(1)))
        err[name] = float(np.linalg.norm(got - exact) / np.linalg.norm(exact))
    print(f"Gaussian stand-in m = {m} c = {c}: DDIM leading n=50 {err['ddim50']:.3g}   2M logsnr n=10 {err['2m10']:.3g}   ratio {err['2m10'] / err['ddim50']:.3f}")
    assert err["2m10"] < err["ddim50"]


# ------------------------------------------------------------------------------------------------ sampler on the tiny synthetic UNet (real plans)
class _Tiny:
    K, h, w = 3, 16, 16

    def __init__(self, kind="custom"):
        from test_keep_region_gpu import _tiny
        from tweediemix_amd import masks as M, sampler as S
        self.S, self.kind = S, kind
        self.W, self.te, self.ts = _tiny(kind, self.K)
        self.cfg = _cfg(S)
        self.masks = M.build_masks(M.partition_rectangle_masks(self.K, self.h * 8, self.w * 8, seed=3), self.h, self.w)
        self.xT = torch.randn(2, 4, self.h, self.w, generator=torch.Generator().manual_seed(29))

    def sampler(self, graphs=False, seeds=1, masks=None, **kw):
        masks = self.masks if masks is None else masks
        return self.S.Tweediemix(self.cfg, self.W, self.te, self.ts, lambda x0: masks, concept_num=self.K, lora=(self.kind == "lora"),
                                 use_graphs=graphs, n_seeds=seeds, **kw)


MS = dict(solver="dpmpp2m", timestep_spacing="logsnr")


@pytest.mark.parametrize("kind", ["custom", "lora"])
def test_tiny_unet_graph_replay_equals_eager(kind, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    T = _Tiny(kind)
    eager, graph = T.sampler(False, **MS), T.sampler(True, **MS)
    a, b = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)                                  # graph replay == eager execution, bit for bit
    assert eager.unet_calls == graph.unet_calls and len(eager.unet_calls) == 13
    ms_keys = sorted(k for k in graph.graphs if len(k) == 3)
    want = [("fusion", L.STEP_FUSION, "ms"), ("plain", L.STEP_PLAIN, "ms")]
    if kind == "lora":
        want = sorted(want + [("fusion_base", L.STEP_FUSION, "ms")])
    assert ms_keys == want                                                                # one graph per (kind, mode, "ms"): both orders replay it
    assert sorted(k for k in graph.graphs if len(k) == 2) == sorted([("start", L.STEP_RESAMPLE), ("plain", L.STEP_PLAIN), ("start", L.STEP_PLAIN)])
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()                                     # every captured step replayed from the first one on
    assert torch.equal(again, a) and sorted(k for k in graph.graphs if len(k) == 3) == want
    assert not torch.equal(a, T.sampler(False).run_fusion(T.xT[0:1].clone()).cpu())       # and it is not the DDIM run


def test_default_arguments_are_the_sampler_of_today(monkeypatch):
    """solver="ddim", timestep_spacing="leading" spelled out equals the constructor call without them: the same bits, the same step entries, the same
    UNet calls, the same plan launches (names compared as tests/test_keep_region_gpu.py compares them), the same graph keys"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny("custom")
    calls = _spy_entries(monkeypatch)
    names = lambda p: [getattr(fn, "__name__", "") for fn, _a in p.ops]
    runs = []
    for graphs in (False, True):
        for kw in ({}, dict(solver="ddim", timestep_spacing="leading")):
            tw = T.sampler(graphs, **kw)
            out = tw.run_fusion(T.xT[0:1].clone()).cpu()
            runs.append((out, list(calls), tw))
            calls[:] = []
    for (oa, ca, ta), (ob, cb, tb) in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert torch.equal(oa, ob) and ca == cb and ta.unet_calls == tb.unet_calls and len(ta.unet_calls) == 13
        assert sorted(ta.plans) == sorted(tb.plans) and sorted(ta.graphs) == sorted(tb.graphs)
        for k in ta.plans:
            assert names(ta.plans[k]) == names(tb.plans[k]) and len(names(ta.plans[k])) > 50, k
        assert tb._x0_prev is None and tb.skip == 100 and tb.scheduler.timesteps == ta.scheduler.timesteps
    assert runs[0][1] == [ENTRIES[0]] * 13                                                # eager: the DDIM entry for every step, never another
    assert torch.equal(runs[0][0], runs[2][0]) and all(len(k) == 2 for k in runs[3][2].graphs)


def test_tiny_unet_two_window_canvas_equals_step_plus_consensus(monkeypatch):
    """16 x 24 canvas, two 16 x 16 windows overlapping by 8: every solver step of the run equals the restatement of the step per window (on the eps the
    plan produced) followed by the consensus restatement of tests/test_canvas_gpu.py; the history and the estimate stay per window"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from test_canvas_gpu import consensus_np
    from tweediemix_amd import lib as L, masks as M, solver as SV
    T = _Tiny("custom")
    ch, cw = 16, 24
    masks = M.build_masks(M.partition_rectangle_masks(T.K, ch * 8, cw * 8, seed=3), ch, cw)
    tw = T.sampler(False, masks=masks, canvas=dict(height=ch * 8, width=cw * 8, overlap=64), **MS)
    assert tw.windows == [(0, 0), (0, 8)] and tw.n_seeds == 2
    rec, real = [], tw._enqueue_step

    def spy(kind, mode, ms=False):
        before, prev = tw.x_state.clone(), tw._x0_prev.clone()
        real(kind, mode, ms)
        torch.cuda.synchronize()
        rec.append((kind, mode, ms, before, prev, tw.plan(kind).eps.clone(), tw.step_params.clone(), tw.x_state.clone(), tw._x0_prev.clone(),
                    tw.x0_state.clone()))
    tw._enqueue_step = spy
    xT = torch.randn(1, 4, ch, cw, generator=torch.Generator().manual_seed(31))
    out = tw.run_fusion(xT.clone())
    assert out.shape == (1, 4, ch, cw) and torch.isfinite(out).all() and len(rec) == 13
    assert [r[2] for r in rec] == [False] * 3 + [True] + [False] + [True] * 8
    ts, mw = tw.scheduler.timesteps, tw.masks.cpu().numpy()
    n_ms = 0
    for kind, mode, ms, before, prev, eps, prm, after, hist, x0s in rec:
        if not ms:
            continue
        n_ms += 1
        t, sa, s1, cx, c0, c1, is_last, g = (float(v) for v in prm.cpu())
        i = ts.index(int(t))
        second = n_ms > 1 and i != 2                              # the first solver step and the first fusion step are first order
        want_cf = (0.0, 1.0, 0.0) if t == 1 else SV.multistep_coeffs(tw.alpha(ts[i - 1]), tw.alpha(ts[i]), tw.alpha(ts[i + 1]), second)
        assert (cx, c0, c1) == want_cf and is_last == float(t == 1) and g == NF(0.8), (t, i)
        rows = eps.shape[0] // 2
        e, xb, pv = eps.cpu().numpy(), before.cpu().numpy(), prev.cpu().numpy()
        moved, est = [], []
        for b in range(2):
            a, z = SV.multistep_step_reference(mode, xb[b:b + 1], e[b * rows:(b + 1) * rows], mw[b] if mode == L.STEP_FUSION else None, pv[b:b + 1],
                                               g, sa, s1, cx, c0, c1, bool(is_last))
            moved.append(a)
            est.append(z)
        want = consensus_np(np.concatenate(moved).reshape(1, 2, 4, 16, 16), tw.windows, ch, cw)[0].reshape(2, 4, 16, 16)
        assert np.array_equal(after.cpu().numpy(), want), (kind, t)
        assert np.array_equal(hist.cpu().numpy(), np.concatenate(est)) and np.array_equal(x0s.cpu().numpy(), np.concatenate(est)), (kind, t)
        assert torch.equal(after[0, :, :, 8:], after[1, :, :, :8])                        # the windows agree where they overlap
    assert n_ms == 9


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_run_with_both_flags_writes_its_outputs(tmp_path, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("fs_solver_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    a, b = np.zeros((128, 128), np.uint8), np.zeros((128, 128), np.uint8)
    a[16:96, 8:56] = 255
    b[32:120, 72:120] = 255
    Image.fromarray(a).save(tmp_path / "a cat.png")
    Image.fromarray(b).save(tmp_path / "a dog.png")
    common = ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--guidance_scale", "0.8",
              "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "1", "--resolution_h", "128", "--resolution_w", "128",
              "--output_path", str(tmp_path), "--mask_paths", f"{tmp_path / 'a cat.png'}+{tmp_path / 'a dog.png'}", "--seed", "5"]
    lat = fs.main(common + ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--output_path_all", str(tmp_path / "ms")]).cpu()
    ref = fs.main(common + ["--output_path_all", str(tmp_path / "ddim")]).cpu()
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all() and not torch.equal(lat, ref)
    assert torch.equal(torch.load(tmp_path / "ms" / "p_5.latent.pt"), lat)
    img = Image.open(tmp_path / "ms" / "p_5.png")
    assert img.size == (128, 128)
