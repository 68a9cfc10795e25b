"""GPU: stochastic sampling -- tmix_noise_normal, tmix_fused_tweedie_step_noise_dev, Tweediemix(eta=..., noise_seeds=...), --eta.

The generator is compared with the numpy restatement tweediemix_amd.noise.normal and the step with noise.step_reference (the parent's restatement,
then one product and one sum) by np.array_equal / torch.equal, never by a tolerance; with cz = 0 the entry is compared with each of its four parent
ENTRIES bit for bit.  tests/test_noise_cpu.py ties the restatement to the known answers, to fp64 Box-Muller and to N(0, 1).  The one inequality in
this file is the end-to-end variance against the closed-form recursion of tests/noise_cases.py."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import noise_cases as NC
from layout_frames import Frame, _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODES = ("fusion", "plain")
PARENTS = ("dev", "rs", "ms", "ms_rs")
SHAPES = ((8, 8), (24, 40))                 # n = 256: one workgroup; n = 3840: fifteen
SEEDS64 = (182, (0x9E3779B9 << 32) + 7, 0xFFFFFFFFFFFFFFFF)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _mode(name):
    from tweediemix_amd import lib as L
    return {"fusion": L.STEP_FUSION, "plain": L.STEP_PLAIN, "resample": L.STEP_RESAMPLE}[name]


# ------------------------------------------------------------------------------------------------ the generator on its own
@pytest.mark.parametrize("n", [1, 255, 4 * 24 * 40])
def test_noise_normal_equals_the_restatement(n):
    from tweediemix_amd import noise as NZ, ops
    for first in (0, 2 ** 32 - 3):
        for key, step, stream in (((0, 0), 0, 0), ((182, 0), 3, 0), ((0xFFFFFFFF, 0x9E3779B9), 49, 0), ((7, 1), 999, 1), ((182, 0), 2 ** 24 - 1, 0)):
            z = dense_guarded((1, n), F32, rows=8, device="cuda", name="z")
            ops.noise_normal(n, first, key, step, stream, out=z.view.reshape(-1))
            torch.cuda.synchronize()
            z.assert_untouched()
            z.assert_all_written()
            want = NZ.normal(np.arange(n, dtype=np.uint64) + np.uint64(first), key[0], key[1], step, stream)
            assert want.dtype == NF and np.array_equal(z.view.reshape(-1).cpu().numpy(), want), (n, first, key, step)


# ------------------------------------------------------------------------------------------------ the step entry
class Case:
    """the inputs of one launch of the noise entry in the form of one of its four parents: seeds x [4, h, w]; every seed its own key"""

    def __init__(self, parent, mode, dt, K, seeds, h, w, cz=0.3125, is_last=0, step=7, seed=0, zero=False):
        from tweediemix_amd import noise as NZ, ops
        rng = np.random.RandomState(seed + 7 * K + 131 * seeds + h)
        self.parent, self.mode, self.dt, self.K, self.seeds, self.h, self.w = parent, mode, dt, K, seeds, h, w
        self.ms, self.rs = parent.startswith("ms"), parent.endswith("rs")
        self.rows = 2 if mode == "plain" else K + 1
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = np.float16 if dt == "f16" else None
        r = (lambda *s: np.zeros(s, NF)) if zero else (lambda *s: rng.randn(*s).astype(NF))
        self.x, self.prev = r(seeds, 4, h, w), rng.randn(seeds, 4, h, w).astype(NF)
        self.eps_t = torch.from_numpy(r(seeds * self.rows, 4, h, w)).to(DT[dt]).cuda()
        self.eps = self.eps_t.float().cpu().numpy()
        self.masks = rng.rand(seeds, K, 1, h, w).astype(NF)
        self.fac = (0.5 + rng.rand(seeds, self.rows - 1)).astype(NF)
        sa, s1, _, _ = ops.step_coeffs(NF(0.2345), NF(0.2345))
        move = [0.8125, 0.4021, -0.0804, float(is_last), 0.8] if self.ms else [0.7071, 0.6123, float(is_last), 0.8, 0.0]
        self.prm = torch.tensor([781.0, sa, s1] + move + [cz, float(step), 0.0, 0.0], dtype=F32).cuda()
        self.params = [float(v) for v in self.prm.cpu()]              # the fp32 values the kernel reads
        self.keys = [NZ.seed_key(SEEDS64[i % 3] + i // 3) for i in range(seeds)]
        self.keys_t = ops.noise_keys([SEEDS64[i % 3] + i // 3 for i in range(seeds)], "cuda")
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.prev_t, self.fac_t = c(self.x), c(self.masks), c(self.prev), c(self.fac)

    def head(self, out_x, out_x0, x=None, eps=None, masks=None, prm=None, seeds=None, rows=None, mode=None, K=None, dt=None, hw=None):
        from tweediemix_amd import lib as L
        return [_p(self.x_t if x is None else x), _p(self.eps_t if eps is None else eps), {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[self.dt] if dt is None else dt,
                _p(self.m_t if masks is None else masks), self.K * self.hw, _p(out_x), _p(out_x0), self.K if K is None else K, 4,
                self.hw if hw is None else hw, _mode(self.mode) if mode is None else mode, self.rows if rows is None else rows,
                self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm)]

    def launch(self, out_x, out_x0, prev, keys=None, fac=None, w=None, n_win=1, yx=None, canvas=(0, 0), **kw):
        """raw ABI call of the noise entry; every argument defaults to the case's own.  Returns the code."""
        import ctypes as C
        from tweediemix_amd import lib as L
        if yx is not None:
            yx = (C.c_int32 * len(yx))(*yx)
        fac = (self.fac_t if self.rs else None) if fac is None else fac
        return L.load().tmix_fused_tweedie_step_noise_dev(*self.head(out_x, out_x0, **kw), _p(prev) if self.ms else None, _p(fac),
                                                          _p(self.keys_t if keys is None else keys), self.w if w is None else w, n_win, yx,
                                                          canvas[0], canvas[1], _st())

    def launch_parent(self, out_x, out_x0, prev):
        """the parent ENTRY on the same inputs (it reads the first 8 floats of the same params)"""
        from tweediemix_amd import lib as L
        lib, h = L.load(), self.head(out_x, out_x0)
        if self.parent == "dev":
            return lib.tmix_fused_tweedie_step_dev(*h, _st())
        if self.parent == "rs":
            return lib.tmix_fused_tweedie_step_rs_dev(*h, _p(self.fac_t), _st())
        if self.parent == "ms":
            return lib.tmix_fused_tweedie_step_ms_dev(*h[:7], _p(prev), *h[7:], _st())
        return lib.tmix_fused_tweedie_step_ms_rs_dev(*h[:7], _p(prev), *h[7:], _p(self.fac_t), _st())

    def run(self, parent=False, **kw):
        out_x, out_x0, prev = torch.empty_like(self.x_t), torch.empty_like(self.x_t), self.prev_t.clone()
        assert (self.launch_parent(out_x, out_x0, prev) if parent else self.launch(out_x, out_x0, prev, **kw)) == 0
        torch.cuda.synchronize()
        return out_x, out_x0, prev

    def reference(self, index=None):
        from tweediemix_amd import noise as NZ
        ox, o0 = [], []
        for sd in range(self.seeds):
            a, b = NZ.step_reference(_mode(self.mode), self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows], self.masks[sd],
                                     self.prev[sd:sd + 1] if self.ms else None, self.params, self.keys[sd], self.fac[sd] if self.rs else None,
                                     None if index is None else index[sd], self.lowp)
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self):
        out_x, out_x0, prev = self.run()
        ref, ref0 = self.reference()
        what = (self.parent, self.mode, self.dt, self.K, self.seeds, self.h, self.w)
        assert ref.dtype == NF and np.array_equal(out_x.cpu().numpy(), ref), what
        assert np.array_equal(out_x0.cpu().numpy(), ref0), what
        assert np.array_equal(prev.cpu().numpy(), ref0 if self.ms else self.prev), what


def _sweep(parent, mode, dt, **kw):
    i = 0
    for h, w in SHAPES:
        for K in (1, 3):
            for seeds in (1, 3):
                yield Case(parent, mode, dt, K, seeds, h, w, seed=i, **kw)
                i += 1


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("parent", PARENTS)
def test_cz_zero_equals_the_parent_entry_bit_for_bit(parent, mode, dt):
    """cz == 0: out_x, out_x0 and the history are the parent ENTRY's, for K in {1, 3}, 1 and 3 seeds, 8 x 8 and 24 x 40; and so is the last step,
    whatever cz it is handed"""
    for kw in (dict(cz=0.0), dict(cz=0.3125, is_last=1)):
        for c in _sweep(parent, mode, dt, **kw):
            got, want = c.run(), c.run(parent=True)
            for a, b, name in zip(got, want, ("out_x", "out_x0", "x0_prev")):
                assert torch.equal(a, b), (name, parent, mode, dt, c.K, c.seeds, c.h, c.w, kw)
            assert torch.isfinite(got[0]).all()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("parent", PARENTS)
def test_kernel_equals_the_restatement(parent, mode, dt):
    for c in _sweep(parent, mode, dt):
        c.check()
    c = Case(parent, mode, dt, 3, 3, 8, 8, seed=99)
    moved = c.run()[0]
    assert not torch.equal(moved, c.run(parent=True)[0])                                # the noise is there ...
    assert torch.equal(c.run(parent=True)[1], c.run()[1])                               # ... and the estimate does not see it


@pytest.mark.parametrize("parent", ["dev", "ms"])
def test_zero_input_gives_cz_z_exactly(parent):
    """x = 0 and eps = 0: x0 = 0, the parent's move is 0, and out_x is the one product cz * z"""
    from tweediemix_amd import noise as NZ
    for mode in MODES:
        c = Case(parent, mode, "f32", 3, 3, 24, 40, cz=0.4375, step=12, zero=True)
        c.prev_t.zero_()
        out_x, out_x0, _ = c.run()
        assert not out_x0.any()
        idx = np.arange(c.n, dtype=np.uint64).reshape(1, 4, c.h, c.w)
        for sd in range(c.seeds):
            z = NZ.normal(idx, c.keys[sd][0], c.keys[sd][1], 12)
            assert np.array_equal(out_x[sd:sd + 1].cpu().numpy(), (NF(0.4375) * z).astype(NF)), (parent, mode, sd)
        assert not torch.equal(out_x[0], out_x[1])                                      # every seed its own noise


def test_second_pass_of_the_grid_stride_loop():
    """hw = 384 x 384: n = 589,824 > 2048 workgroups x 256 threads, so threads of the capped grid take a second element"""
    c = Case("ms", "fusion", "f32", 3, 1, 384, 384, seed=50)
    assert c.n == 4 * 384 * 384 > 2048 * 256
    c.check()


@pytest.mark.parametrize("parent", PARENTS)
def test_co_batched_launch_equals_seeds_one_at_a_time(parent):
    c = Case(parent, "fusion", "f16", 3, 3, 24, 40, seed=60)
    ox, o0, pv = c.run()
    for sd in range(c.seeds):
        a, b, p = torch.empty_like(c.x_t[sd:sd + 1]), torch.empty_like(c.x_t[sd:sd + 1]), c.prev_t[sd:sd + 1].clone()
        assert c.launch(a, b, p, x=c.x_t[sd:sd + 1], eps=c.eps_t[sd * c.rows:(sd + 1) * c.rows], masks=c.m_t[sd], seeds=1, keys=c.keys_t[sd:sd + 1],
                        fac=c.fac_t[sd:sd + 1] if c.rs else None) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, ox[sd:sd + 1]) and torch.equal(b, o0[sd:sd + 1]) and torch.equal(p, pv[sd:sd + 1]), sd


@pytest.mark.parametrize("parent", ["dev", "ms_rs"])
def test_in_place_equals_out_of_place_inside_guard_bands(parent):
    """x is out_x; every output in a guard-band frame (tests/layout_frames.py): nothing outside the views is written and no input changes"""
    c = Case(parent, "fusion", "f32", 3, 3, 24, 40, seed=30)
    ox, o0, pv = c.run()
    S, n = c.seeds, c.n
    flat = lambda t, name: Frame.of(t.reshape(1, -1), name=name).seal()
    eps, masks, prm, fac = flat(c.eps_t, "eps"), flat(c.m_t, "masks"), flat(c.prm, "params"), flat(c.fac_t, "factors")
    keys = Frame.of(c.keys_t.reshape(1, -1), name="keys").seal()
    prev = Frame.of(c.prev_t.reshape(S, n), name="x0_prev")
    out0 = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x0")
    x = dense_guarded((S, n), F32, rows=8, device="cuda", name="x (in place)")
    x.view.copy_(c.x_t.reshape(S, n))
    assert c.launch(x.view, out0.view, prev.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view, keys=keys.view,
                    fac=fac.view if c.rs else None) == 0
    torch.cuda.synchronize()
    for f in (x, out0):
        f.assert_untouched()
        f.assert_all_written()
    prev.assert_untouched()
    for f in (eps, masks, prm, fac, keys):
        f.assert_unchanged()
    assert torch.equal(x.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
    assert torch.equal(prev.view.reshape(pv.shape), pv)
    # without out_x0
    x2, p2 = c.x_t.clone(), c.prev_t.clone()
    assert c.launch(x2, None, p2, x=x2) == 0
    torch.cuda.synchronize()
    assert torch.equal(x2, ox) and torch.equal(p2, pv)


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    c = Case("ms", "fusion", "f32", 3, 2, 4, 6, seed=70)
    out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
    out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
    prev = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="x0_prev")
    go = lambda **kw: c.launch(out_x.view, out_x0.view, prev.view, **kw)
    err = lib.tmix_last_error_string
    assert go(mode=L.STEP_RESAMPLE) == L.EINVAL and b"mode" in err()
    assert c.launch(None, out_x0.view, prev.view) == L.EINVAL
    lib_keys = lib.tmix_fused_tweedie_step_noise_dev(*c.head(out_x.view, out_x0.view), _p(prev.view), None, None, c.w, 1, None, 0, 0, _st())
    assert lib_keys == L.EINVAL and b"keys" in err()
    assert go(n_win=0) == L.EINVAL and go(n_win=L.MAX_WINDOWS + 1, yx=[0, 0] * (L.MAX_WINDOWS + 1), canvas=(4, 6)) == L.EINVAL
    assert go(n_win=2) == L.EINVAL                                                       # two windows without their table
    assert go(w=5) == L.ESHAPE and b"w=5" in err()
    assert go(n_win=2, yx=[0, 0, 0, 3], canvas=(4, 8)) == L.ESHAPE and b"canvas" in err()        # the second window ends at column 9
    assert go(n_win=2, yx=[0, 0, 1, 2], canvas=(4, 8)) == L.ESHAPE
    assert go(n_win=2, yx=[0, 0, 0, 2], canvas=(4, 8), seeds=1) == L.ESHAPE and b"multiple" in err()
    assert go(mode=7) == L.EINVAL and go(K=0) == L.EINVAL and go(dt=9) == L.EINVAL
    assert go(rows=c.K) == L.ESHAPE and go(seeds=0) == L.ESHAPE and go(seeds=65536) == L.ESHAPE
    assert lib.tmix_noise_normal(None, 4, 0, 1, 2, 3, 0, _st()) == L.EINVAL
    assert lib.tmix_noise_normal(_p(out_x.view), 0, 0, 1, 2, 3, 0, _st()) == L.ESHAPE
    assert lib.tmix_noise_normal(_p(out_x.view), 4, -1, 1, 2, 3, 0, _st()) == L.ESHAPE
    torch.cuda.synchronize()
    for f in (out_x, out_x0, prev):                            # nothing was launched: every buffer still holds the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


@pytest.mark.parametrize("canvas,groups", [((16, 24), 2), ((24, 24), 2)])
def test_canvas_windows_are_crops_of_the_canvas_noise(canvas, groups):
    """two windows of 16 x 16 on a 16 x 24 canvas and four on 24 x 24, x = 0 and eps = 0, two trajectories: every window is cz times the crop of
    the canvas-indexed restatement, so what two windows hold on their overlap is identical before any consensus"""
    from tweediemix_amd import canvas as CV, lib as L, noise as NZ, ops
    ch, cw = canvas
    wins = CV.window_layout(ch, cw, 16, 16, 8)
    assert len(wins) == (2 if ch == 16 else 4)
    S = groups * len(wins)
    x = torch.zeros(S, 4, 16, 16, device="cuda")
    eps = torch.zeros(2 * S, 4, 16, 16, device="cuda")
    cz, step = 0.8125, 5
    seeds = [SEEDS64[1], SEEDS64[0]][:groups]
    keys = ops.noise_keys(seeds, "cuda")
    for ms in (False, True):
        move = [0.8125, 0.4021, -0.0804, 0.0, 0.8] if ms else [0.7071, 0.6123, 0.0, 0.8, 0.0]
        prm = torch.tensor([781.0, 0.6, 0.8] + move + [cz, float(step), 0.0, 0.0], dtype=F32).cuda()
        prev = torch.zeros_like(x) if ms else None
        out = ops.fused_tweedie_step_noise_dev(x, eps, None, L.STEP_PLAIN, 1, prm, keys, x0_prev=prev, windows=wins, canvas_hw=(ch, cw))
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(groups, len(wins), 4, 16, 16)
        for g in range(groups):
            full = (NF(cz) * NZ.normal(NZ.canvas_index(4, ch, cw), *NZ.seed_key(seeds[g]), step)).astype(NF)
            for k, (oy, ox) in enumerate(wins):
                assert np.array_equal(got[g, k], full[:, oy:oy + 16, ox:ox + 16]), (canvas, ms, g, k)
        assert np.array_equal(got[0, 0][:, :, 8:], got[0, 1][:, :, :8]) and not np.array_equal(got[0], got[1])
        # the same rows as windows of NO canvas: every row the latent's own indices, the two trajectories' first rows differ from the canvas's
        one = ops.fused_tweedie_step_noise_dev(x[:groups], eps[:2 * groups], None, L.STEP_PLAIN, 1, prm, keys, x0_prev=None if prev is None else prev[:groups])
        torch.cuda.synchronize()
        assert np.array_equal(one[0].cpu().numpy(), (NF(cz) * NZ.normal(NZ.canvas_index(4, 16, 16), *NZ.seed_key(seeds[0]), step)).astype(NF))


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


K3, H, W = 3, 16, 16
ROWS = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2}
ENTRIES = ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev", "tmix_fused_tweedie_step_ms_dev", "tmix_fused_tweedie_step_rs_dev",
           "tmix_fused_tweedie_step_ms_rs_dev", "tmix_fused_tweedie_step_noise_dev")
DEV, MS_, NOISE = ENTRIES[0], ENTRIES[2], ENTRIES[5]


def _cfg(S, n=10, R=1, J=1, h=H, w=W):
    return S.make_config(guidance_scale=0.8, n_timesteps=n, t_cond=0.2, t_stop=0.8, resampling_steps=R, jumping_steps=J, resolution_h=h * 8,
                         resolution_w=w * 8)


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step entry the sampler calls"""
    from tweediemix_amd import lib as L
    lib, calls = L.load(), []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _standin_eps(kind, x, t):
    """the stand-in UNet: an elementwise function of (row, x, t), so a seed's eps does not depend on what it is co-batched with"""
    rows = ROWS[kind]
    e = torch.stack([torch.sin(x * (1.0 + 0.25 * r) + 0.01 * float(t) + r) for r in range(rows)], dim=1)
    return e.reshape(x.shape[0] * rows, *x.shape[1:]).contiguous()


def _run_standin(solver, seeds, noise_seeds, xT, eta=0.6, log=None):
    from tweediemix_amd import masks as M, sampler as S
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W)
    tw = S.Tweediemix(_cfg(S), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, n_seeds=seeds, solver=solver, timestep_spacing="logsnr",
                      eta=eta, noise_seeds=noise_seeds)

    def unet(kind, x, t):
        e = _standin_eps(kind, x, t)
        if log is not None:
            log.append((kind, int(t), x.clone(), e.clone()))
        return e
    tw._unet = unet
    return tw, masks, tw.run_fusion(xT.clone())


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_sampler_standin_unet_every_trajectory_step_equals_the_restatement(solver, monkeypatch):
    """n = 10 on the log-SNR grid, K = 3, two seeds, one resampling and one jumping step, eta = 0.6: the state after EVERY step that advances the
    trajectory (= the state handed to the next call, and the final latent) equals noise.step_reference on the coefficients of solver.*_eta_coeffs
    with the schedule index as the step; the resampling round trip and the look-ahead go through today's entry and add nothing"""
    from tweediemix_amd import lib as L, noise as NZ, ops, solver as SV
    n, R, J, g, eta, seeds = 10, 1, 1, 0.8, 0.6, 2
    nseeds = [SEEDS64[1], 182]
    xT = torch.randn(seeds, 4, H, W, generator=torch.Generator().manual_seed(43))
    calls, log = _spy_entries(monkeypatch), []
    tw, masks, out = _run_standin(solver, seeds, nseeds, xT, eta, log)
    mk = masks.cpu().numpy()
    ts = tw.scheduler.timesteps
    assert ts == [901, 770, 612, 427, 243, 108, 39, 12, 4, 1] and tw._window_index(0.2) == 2
    assert len(log) == len(calls) == n + 2 * R + J == 13
    assert calls == [DEV] * (2 * R) + [NOISE] * 2 + [DEV] * J + [NOISE] * (n - 2)
    assert [(k, t) for k, t, *_ in log[:5]] == [("start", 901), ("plain", 770), ("start", 901), ("plain", 770), ("plain", 612)]
    assert torch.equal(log[4][2], log[5][2])                      # the look-ahead did not move the trajectory
    traj = [2, 3] + list(range(5, 13))                            # call indices of the advancing steps i = 0 .. 9
    hist, prev_mode = np.zeros((seeds, 4, H, W), NF), None
    for i, ci in enumerate(traj):
        kind, t, x, eps = log[ci]
        assert t == ts[i]
        mode = L.STEP_FUSION if i >= 2 else L.STEP_PLAIN
        assert kind == ("start" if i == 0 else "fusion" if i >= 2 else "plain")
        last = t == 1
        at, an = tw.alpha(t), tw.alpha(tw.scheduler.next_t(t))
        ms = solver == "dpmpp2m" and i > 0
        if ms:
            second = i >= 2 and mode == prev_mode
            cf = (0.0, 1.0, 0.0, 0.0) if last else SV.multistep_eta_coeffs(tw.alpha(ts[i - 1]), at, an, second, eta)
            sa, s1, _, _ = ops.step_coeffs(at, an)
            prm = [t, sa, s1, cf[0], cf[1], cf[2], float(last), g, cf[3], i, 0, 0]
            prev_mode = mode
        else:
            sa, s1, san, s1d, cz = SV.ddim_eta_coeffs(at, an, eta)
            prm = [t, sa, s1, san, s1d, float(last), g, 0, 0.0 if last else cz, i, 0, 0]
        assert last or prm[8] > 0.0
        xs, es = x.cpu().numpy(), eps.cpu().numpy()
        rows = ROWS[kind]
        nxt, x0s = [], []
        for sd in range(seeds):
            a, b = NZ.step_reference(mode, xs[sd:sd + 1], es[sd * rows:(sd + 1) * rows], mk if mode == L.STEP_FUSION else None,
                                     hist[sd:sd + 1] if ms else None, prm, NZ.seed_key(nseeds[sd]))
            nxt.append(a)
            x0s.append(b)
        state = np.concatenate(nxt)
        if ms:
            hist = np.concatenate(x0s)
        after = out if i == n - 1 else log[traj[i + 1]][2]
        assert np.array_equal(after.cpu().numpy(), state), (solver, i, t)
    assert torch.isfinite(out).all()
    # another noise seed is another trajectory; the same seeds are the same bits
    _, _, again = _run_standin(solver, seeds, nseeds, xT, eta)
    _, _, other = _run_standin(solver, seeds, [nseeds[0], 183], xT, eta)
    assert torch.equal(again, out) and torch.equal(other[0], out[0]) and not torch.equal(other[1], out[1])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_seed_of_a_three_seed_run_equals_its_single_run(solver):
    nseeds = [182, 183, SEEDS64[2]]
    xT = torch.randn(3, 4, H, W, generator=torch.Generator().manual_seed(47))
    _, _, all3 = _run_standin(solver, 3, nseeds, xT)
    for sd in range(3):
        _, _, one = _run_standin(solver, 1, nseeds[sd:sd + 1], xT[sd:sd + 1])
        assert torch.equal(one[0], all3[sd]), (solver, sd)


def test_end_to_end_variance_on_the_gaussian_model():
    """the stand-in returns the exact eps of data N(0, c^2), c = 0.5; 3 seeds at 4 x 64 x 64, n = 20, dpmpp2m on the log-SNR grid, eta = 1, no
    resampling: the mean square of the final latent lies within 5 standard errors (sqrt(2 / N), N = 49152: 3.2 %) of the variance the closed-form
    recursion of tests/noise_cases.py predicts for the sampler's own coefficients and phase rule"""
    from tweediemix_amd import masks as M, sampler as S
    c, n, h, w, seeds = 0.5, 20, 64, 64, 3
    masks = M.build_masks(M.partition_rectangle_masks(K3, h * 8, w * 8, seed=3), h, w)
    tw = S.Tweediemix(_cfg(S, n, 0, 1, h, w), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, n_seeds=seeds, solver="dpmpp2m",
                      timestep_spacing="logsnr", eta=1.0, noise_seeds=[182, 183, 184])

    def unet(kind, x, t):
        e = torch.from_numpy(NC.exact_eps(x.cpu().numpy(), tw.alpha(t), c).astype(NF)).cuda()
        return e.repeat_interleave(ROWS[kind], dim=0)
    tw._unet = unet
    xT = torch.randn(seeds, 4, h, w, generator=torch.Generator().manual_seed(53))
    out = tw.run_fusion(xT).double().cpu().numpy().reshape(-1)
    N = out.size
    assert N == 49152
    want, _ = NC.predicted_variance(c, n, "logsnr", "dpmpp2m", 1.0, first_order_at=(tw._window_index(0.2),))
    got = float((out * out).mean())
    print(f"final latent: mean square {got:.6g}, predicted variance {want:.6g}, {abs(got - want) / (want * math.sqrt(2 / N)):.2f} standard errors")
    assert abs(got - want) <= 5 * math.sqrt(2.0 / N) * want
    assert abs(float(out.mean())) <= 5 * math.sqrt(want / N)


def test_canvas_sampler_steps_equal_the_canvas_indexed_restatement():
    """24 x 24 canvas, four 16 x 16 windows overlapping by 8, stand-in UNet, eta = 0.6: every advancing step equals the restatement of the step per
    window with the window's CANVAS indices followed by the consensus restatement of tests/test_canvas_gpu.py -- and the consensus changes nothing:
    where windows overlap they already hold the same bits, noise included"""
    from test_canvas_gpu import consensus_np
    from tweediemix_amd import lib as L, masks as M, noise as NZ, sampler as S, solver as SV
    ch = cw = 24
    eta, g, seed = 0.6, 0.8, SEEDS64[1]
    masks = M.build_masks(M.partition_rectangle_masks(K3, ch * 8, cw * 8, seed=3), ch, cw)
    tw = S.Tweediemix(_cfg(S), _NoWeights(), None, None, lambda x0: masks, concept_num=K3, timestep_spacing="logsnr", eta=eta, noise_seeds=[seed],
                      canvas=dict(height=ch * 8, width=cw * 8, overlap=64))
    assert tw.windows == [(0, 0), (0, 8), (8, 0), (8, 8)] and tw.n_seeds == 4
    log = []

    def unet(kind, x, t):
        e = _standin_eps(kind, x, t)
        log.append((kind, int(t), x.clone(), e.clone()))
        return e
    tw._unet = unet
    xT = torch.randn(1, 4, ch, cw, generator=torch.Generator().manual_seed(59))
    out = tw.run_fusion(xT.clone())
    ts, mw = tw.scheduler.timesteps, tw.masks.cpu().numpy()
    traj = [2, 3] + list(range(5, 13))
    for i, ci in enumerate(traj):
        kind, t, x, eps = log[ci]
        mode = L.STEP_FUSION if i >= 2 else L.STEP_PLAIN
        last = t == 1
        sa, s1, san, s1d, cz = SV.ddim_eta_coeffs(tw.alpha(t), tw.alpha(tw.scheduler.next_t(t)), eta)
        prm = [t, sa, s1, san, s1d, float(last), g, 0, 0.0 if last else cz, i, 0, 0]
        xs, es, rows = x.cpu().numpy(), eps.cpu().numpy(), ROWS[kind]
        moved = [NZ.step_reference(mode, xs[b:b + 1], es[b * rows:(b + 1) * rows], mw[b] if mode == L.STEP_FUSION else None, None, prm, NZ.seed_key(seed),
                                   index=NZ.canvas_index(4, H, W, oy, ox, ch, cw))[0] for b, (oy, ox) in enumerate(tw.windows)]
        moved = np.concatenate(moved)
        want = consensus_np(moved.reshape(1, 4, 4, H, W), tw.windows, ch, cw)[0].reshape(4, 4, H, W)
        assert np.array_equal(want, moved), (i, t)                # equal before the consensus: the mean of equal values
        after = tw.x_state if i == len(traj) - 1 else log[traj[i + 1]][2]
        assert np.array_equal(after.cpu().numpy(), want), (i, t)
    assert out.shape == (1, 4, ch, cw) and torch.isfinite(out).all()
    assert torch.equal(out[0, :, 8:24, 8:24], tw.x_state[3])


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

    def sampler(self, graphs=False, seeds=1, **kw):
        return self.S.Tweediemix(self.cfg, self.W, self.te, self.ts, lambda x0: self.masks, concept_num=self.K, use_graphs=graphs, n_seeds=seeds, **kw)


@pytest.mark.parametrize("kw", [dict(solver="dpmpp2m", timestep_spacing="logsnr"), dict(guidance_rescale=0.7), dict(n_streams=2)],
                         ids=["dpmpp2m", "ddim_rs", "ddim_two_streams"])
def test_tiny_unet_graph_replay_equals_eager(kw, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    T = _Tiny()
    nz = dict(eta=0.5, noise_seeds=[182])
    eager, graph = T.sampler(False, **kw, **nz), T.sampler(True, **kw, **nz)
    a, b = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)                                  # graph replay == eager execution, bit for bit
    assert eager.unet_calls == graph.unet_calls and len(eager.unet_calls) == 13
    tail = ("rs", "eta") if "guidance_rescale" in kw else ("eta",)
    mid = ("ms",) if "solver" in kw else ()
    eta_keys = sorted(k for k in graph.graphs if k[-1] == "eta")
    assert eta_keys == sorted([("start", L.STEP_PLAIN) + tail, ("plain", L.STEP_PLAIN) + mid + tail, ("fusion", L.STEP_FUSION) + mid + tail])
    assert all("eta" not in k for k in graph.graphs if k[-1] != "eta") and len(graph.graphs) == 5
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()                                     # every captured step replayed from the first one on
    assert torch.equal(again, a)
    graph.set_noise_seeds([183])                                                          # the captured steps read the new key
    eager.set_noise_seeds([183])
    c, d = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.equal(c, d) and not torch.equal(c, a)
    assert not torch.equal(a, T.sampler(False, **kw).run_fusion(T.xT[0:1].clone()).cpu())     # and it is not the deterministic run


def test_eta_zero_is_the_sampler_of_today(monkeypatch):
    """eta = 0.0 spelled out, with noise seeds given: the same bits, the same step entries, the same UNet calls, the same graph keys as without"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny()
    calls = _spy_entries(monkeypatch)
    for base in ({}, dict(solver="dpmpp2m", timestep_spacing="logsnr")):
        runs = []
        for graphs in (False, True):
            for kw in ({}, dict(eta=0.0, noise_seeds=[182])):
                tw = T.sampler(graphs, **base, **kw)
                out = tw.run_fusion(T.xT[0:1].clone()).cpu()
                runs.append((out, list(calls), tw))
                calls[:] = []
        for (oa, ca, ta), (ob, cb, tb) in ((runs[0], runs[1]), (runs[2], runs[3])):
            assert torch.equal(oa, ob) and ca == cb and ta.unet_calls == tb.unet_calls and len(ta.unet_calls) == 13
            assert sorted(ta.graphs) == sorted(tb.graphs) and tb.step_params.numel() == 8
        assert NOISE not in runs[1][1] and len(runs[1][1]) == 13 and torch.equal(runs[0][0], runs[2][0])
        assert all("eta" not in k for k in runs[3][2].graphs)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_run_with_eta_writes_its_outputs(tmp_path, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("fs_noise_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
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
    lat = fs.main(common + ["--eta", "0.5", "--output_path_all", str(tmp_path / "eta")]).cpu()
    ref = fs.main(common + ["--output_path_all", str(tmp_path / "ddim")]).cpu()
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all() and not torch.equal(lat, ref)
    assert torch.equal(torch.load(tmp_path / "eta" / "p_5.latent.pt"), lat)
    assert Image.open(tmp_path / "eta" / "p_5.png").size == (128, 128)
    with pytest.raises(SystemExit, match="--eta"):
        fs.main(common + ["--eta", "1.5"])
