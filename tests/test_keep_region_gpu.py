"""GPU: the keep region -- tmix_fused_tweedie_step_keep_dev, Tweediemix.set_keep / clear_keep, --keep_latents / --keep_image / --reroll.

The CPU restatement of the keep term (`restate`) calls oracle.tweedie_oracle unchanged for the mode's x0 / moved and adds, in numpy fp32,
    kept  = is_last ? keep_x0 : sa_next * keep_x0 + s1_next * keep_eps          new = is_last ? x0 : moved
    out_x = w * kept + (1 - w) * new                                            out_x0 = w * keep_x0 + (1 - w) * x0
-- two products and one sum each.  The kernel is compared with it by torch.equal / np.array_equal, never by a tolerance; the one tolerance
in this file (2e-5 per step on the stand-in-UNet trajectories) is tests/test_sampler_gpu.py's bound for its replayed trajectories.
"""
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


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _mode(name):
    from tweediemix_amd import lib as L
    return {"fusion": L.STEP_FUSION, "plain": L.STEP_PLAIN, "resample": L.STEP_RESAMPLE}[name]


# ------------------------------------------------------------------------------------------------ the restatement
def restate(mode, x, eps, masks, K, g, at, an, is_last, lowp, kx, ke, kw):
    """one seed: x, kx, ke [1,C,h,w], eps [rows,C,h,w] (fp32 values of the eps dtype), masks [K,1,h,w], kw [1,1,h,w] -> (out_x, out_x0)"""
    from oracle import tweedie_oracle as TO
    if mode == "fusion":
        new, x0 = TO.fused_fusion_step(x, eps, masks, g, at, an, is_last, lowp)
    elif mode == "plain":
        new, x0 = TO.fused_plain_step(x, eps[:2], g, at, an, is_last, lowp)
    else:       # fused_resample_down returns the moved latent only: its x0 from the same oracle functions, tied to it by the assert
        eu = eps[:1]
        x0 = (NF(K - 1) * TO.tweedie_x0(x, TO.cfg_combine(eu, eps[1:2], g, lowp), at, lowp)).astype(NF)
        for c in range(K - 1):
            x0 = (x0 - TO.tweedie_x0(x, TO.cfg_combine(eu, eps[2 + c:3 + c], g, lowp), at, lowp)).astype(NF)
        moved = TO.ddim_move(x0, eu, an, lowp)
        assert np.array_equal(moved, TO.fused_resample_down(x, eps, K, g, at, an, lowp))
        new = x0 if is_last else moved
    san, s1n = np.sqrt(NF(an)).astype(NF), np.sqrt(NF(1) - NF(an)).astype(NF)
    kept = kx if is_last else (san * kx + s1n * ke).astype(NF)
    out_x = (kw * kept + (NF(1) - kw) * new).astype(NF)
    out_x0 = (kw * kx + (NF(1) - kw) * x0).astype(NF)
    assert out_x.dtype == NF and out_x0.dtype == NF
    return out_x, out_x0


class Case:
    """the inputs of one launch (numpy fp32 + device tensors): seeds x [C=4,h,w]; `shared` = which of keep_x0 / keep_eps / keep_w all seeds share"""

    def __init__(self, mode, dt, K, seeds, h, w, is_last, shared=(False, False, False), frac=False, weight=None, seed=0):
        from tweediemix_amd import ops
        rng = np.random.RandomState(seed + 7 * K + 131 * seeds + h)
        self.mode, self.dt, self.K, self.seeds, self.h, self.w, self.is_last, self.shared = mode, dt, K, seeds, h, w, int(is_last), shared
        self.rows = 2 if mode == "plain" else K + 1
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = np.float16 if dt == "f16" else None
        self.at, self.an, self.g = NF(0.2345), NF(0.3456), 0.8
        r = lambda *s: rng.randn(*s).astype(NF)
        self.x = r(seeds, 4, h, w)
        self.eps_t = torch.from_numpy(r(seeds * self.rows, 4, h, w)).to(DT[dt]).cuda()
        self.eps = self.eps_t.float().cpu().numpy()
        self.masks = (rng.rand(seeds, K, 1, h, w) > 0.5).astype(NF)
        ns = [1 if s else seeds for s in shared]
        self.kx, self.ke = r(ns[0], 4, h, w), r(ns[1], 4, h, w)
        if weight is not None:
            self.kw = np.full((ns[2], 1, h, w), weight, NF)
        elif frac:
            self.kw = rng.rand(ns[2], 1, h, w).astype(NF)
            self.kw.reshape(-1)[::7] = 0.0
            self.kw.reshape(-1)[3::7] = 1.0
        else:
            self.kw = (rng.rand(ns[2], 1, h, w) > 0.5).astype(NF)
        sa, s1, san, s1n = ops.step_coeffs(self.at, self.an)
        self.prm = torch.tensor([781.0, sa, s1, san, s1n, float(self.is_last), self.g, 0.0], dtype=F32).cuda()
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.kx_t, self.ke_t, self.kw_t = c(self.x), c(self.masks), c(self.kx), c(self.ke), c(self.kw)

    def strides(self):
        return tuple(0 if s else ext for s, ext in zip(self.shared, (self.n, self.n, self.hw)))

    def launch(self, out_x, out_x0, x=None, eps=None, masks=None, prm=None, kx=None, ke=None, kw=None, strides=None, seeds=None, entry="keep",
               mss=None, rows=None, **bad):
        """raw ABI call; every tensor argument defaults to the case's own.  Returns the code."""
        from tweediemix_amd import lib as L
        lib = L.load()
        sx, se, sw = self.strides() if strides is None else strides
        head = [_p(self.x_t if x is None else x), _p(self.eps_t if eps is None else eps), {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[self.dt],
                _p(self.m_t if masks is None else masks), self.K * self.hw if mss is None else mss, _p(out_x), _p(out_x0), self.K, 4, self.hw,
                _mode(self.mode), self.rows if rows is None else rows, self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm)]
        if entry == "plain":
            return lib.tmix_fused_tweedie_step_dev(*head, _st())
        keep = dict(kx_ptr=_p(self.kx_t if kx is None else kx), sx=sx, ke_ptr=_p(self.ke_t if ke is None else ke), se=se,
                    kw_ptr=_p(self.kw_t if kw is None else kw), sw=sw)
        assert set(bad) <= set(keep), bad                     # (`bad` overrides raw ABI values: a None pointer, a short stride)
        keep.update(bad)
        return lib.tmix_fused_tweedie_step_keep_dev(*head, keep["kx_ptr"], keep["sx"], keep["ke_ptr"], keep["se"], keep["kw_ptr"], keep["sw"], _st())

    def run(self, **kw):
        out_x, out_x0 = torch.empty_like(self.x_t), torch.empty_like(self.x_t)
        assert self.launch(out_x, out_x0, **kw) == 0
        torch.cuda.synchronize()
        return out_x, out_x0

    def reference(self):
        ox, o0 = [], []
        for sd in range(self.seeds):
            pick = lambda a: a[0:1] if a.shape[0] == 1 else a[sd:sd + 1]
            a, b = restate(self.mode, self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows], self.masks[sd], self.K, self.g, self.at, self.an,
                           self.is_last, self.lowp, pick(self.kx), pick(self.ke), pick(self.kw))
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self, what=""):
        out_x, out_x0 = self.run()
        ref, ref0 = self.reference()
        assert np.array_equal(out_x.cpu().numpy(), ref), (what, self.mode, self.dt, self.K, self.seeds, self.is_last, self.shared)
        assert np.array_equal(out_x0.cpu().numpy(), ref0), (what, self.mode, self.dt, self.K, self.seeds, self.is_last, self.shared)


# ------------------------------------------------------------------------------------------------ kernel == restatement
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_restatement_sweep(mode, dt):
    """every K x seeds x is_last at hw = 3 x 5 (n = 60: less than one workgroup) and 37 x 41 (n = 6068: ragged last workgroup); the sharing pattern of
    the three keep arrays cycles through all eight combinations, binary weights"""
    i = 0
    for h, w in ((3, 5), (37, 41)):
        for K in (1, 3):
            for seeds in (1, 3):
                for is_last in (0, 1):
                    shared = tuple(bool(i >> b & 1) for b in range(3))
                    Case(mode, dt, K, seeds, h, w, is_last, shared=shared, seed=i).check()
                    i += 1


@pytest.mark.parametrize("shared", [tuple(bool(i >> b & 1) for b in range(3)) for i in range(8)])
def test_shared_and_per_seed_strides(shared):
    """shared (stride 0) vs per-seed for each of keep_x0 / keep_eps / keep_w, three seeds, every mode; fractional and binary weights"""
    for mode in MODES:
        Case(mode, "f32", 3, 3, 37, 41, 0, shared=shared, frac=True, seed=50).check("fractional")
        Case(mode, "f16", 3, 3, 3, 5, 1, shared=shared, seed=51).check("binary, last")


@pytest.mark.parametrize("mode,dt,is_last", [("fusion", "f32", 0), ("plain", "f16", 0), ("resample", "bf16", 0), ("fusion", "bf16", 1)])
def test_fractional_weights(mode, dt, is_last):
    Case(mode, dt, 3, 3, 37, 41, is_last, shared=(True, False, True), frac=True, seed=60).check()


def test_second_pass_of_the_grid_stride_loop():
    """hw = 384 x 352: n = 540,672 > 2048 workgroups x 256 threads, so every thread of the capped grid takes a second element"""
    c = Case("fusion", "f32", 3, 1, 384, 352, 0, shared=(True, True, True), frac=True, seed=70)
    assert c.n > 2048 * 256
    c.check()


# ------------------------------------------------------------------------------------------------ boundary and aliasing behaviour
@pytest.mark.parametrize("mode", MODES)
def test_weight_zero_is_the_plain_step_and_weight_one_is_the_kept_latent(mode):
    from tweediemix_amd import ops
    for is_last in (0, 1):
        for dt in DT:
            c = Case(mode, dt, 3, 3, 37, 41, is_last, weight=0.0, seed=80)
            ox, o0 = c.run()
            px, p0 = c.run(entry="plain")
            assert torch.equal(ox, px) and torch.equal(o0, p0), (mode, dt, is_last)
        c = Case(mode, "f32", 3, 3, 37, 41, is_last, weight=1.0, seed=81)
        ox, o0 = c.run()
        _sa, _s1, san, s1n = ops.step_coeffs(c.at, c.an)
        want = c.kx if is_last else (NF(san) * c.kx + NF(s1n) * c.ke).astype(NF)
        assert np.array_equal(ox.cpu().numpy(), want) and np.array_equal(o0.cpu().numpy(), c.kx), (mode, is_last)


@pytest.mark.parametrize("mode", MODES)
def test_in_place_equals_out_of_place(mode):
    c = Case(mode, "f32", 3, 3, 37, 41, 0, frac=True, seed=90)
    ox, o0 = c.run()
    x = c.x_t.clone()
    o0b = torch.empty_like(x)
    assert c.launch(x, o0b, x=x) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, ox) and torch.equal(o0b, o0)


@pytest.mark.parametrize("mode", MODES)
def test_guard_bands_and_untouched_inputs(mode):
    """every pointer in a guard-band frame (tests/layout_frames.py): NaN poison around every input, per-seed keep arrays with seed strides LARGER than
    their extent (poison between the seeds), the latent updated in place; nothing outside the views is written and no input changes"""
    c = Case(mode, "f32", 3, 3, 37, 41, 0, frac=True, seed=100)
    ox, o0 = c.run()
    S, n, hw = c.seeds, c.n, c.hw
    flat = lambda t: Frame.of(t.reshape(1, -1), name="input").seal()
    eps, masks, prm = flat(c.eps_t), flat(c.m_t), flat(c.prm)
    pad = 24
    kx = Frame.of(c.kx_t.reshape(S, n), ld=n + pad, name="keep_x0").seal()
    ke = Frame.of(c.ke_t.reshape(S, n), ld=n + pad + 8, name="keep_eps").seal()
    kw = Frame.of(c.kw_t.reshape(S, hw), ld=hw + pad, name="keep_w").seal()
    x = dense_guarded((S, n), F32, rows=8, device="cuda", name="x (in place)")
    x.view.copy_(c.x_t.reshape(S, n))
    out0 = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x0")
    rc = c.launch(x.view, out0.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view, kx=kx.view, ke=ke.view, kw=kw.view,
                  strides=(n + pad, n + pad + 8, hw + pad))
    assert rc == 0
    torch.cuda.synchronize()
    for f in (x, out0):
        f.assert_untouched()
        f.assert_all_written()
    for f in (eps, masks, prm, kx, ke, kw):
        f.assert_unchanged()
    assert torch.equal(x.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
    # out of place: x is an input like the others
    xin = Frame.of(c.x_t.reshape(S, n), name="x").seal()
    outx = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x")
    out0 = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x0")
    assert c.launch(outx.view, out0.view, x=xin.view, kx=kx.view, ke=ke.view, kw=kw.view, strides=(n + pad, n + pad + 8, hw + pad)) == 0
    torch.cuda.synchronize()
    for f in (outx, out0):
        f.assert_untouched()
        f.assert_all_written()
    xin.assert_unchanged()
    assert torch.equal(outx.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)


@pytest.mark.parametrize("mode", MODES)
def test_co_batched_launch_equals_seeds_one_at_a_time(mode):
    c = Case(mode, "f16", 3, 3, 37, 41, 0, shared=(True, False, False), frac=True, seed=110)
    ox, o0 = c.run()
    for sd in range(c.seeds):
        a, b = torch.empty_like(c.x_t[sd:sd + 1]), torch.empty_like(c.x_t[sd:sd + 1])
        rc = c.launch(a, b, x=c.x_t[sd:sd + 1], eps=c.eps_t[sd * c.rows:(sd + 1) * c.rows], masks=c.m_t[sd], kx=c.kx_t, ke=c.ke_t[sd:sd + 1],
                      kw=c.kw_t[sd:sd + 1], seeds=1)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(a, ox[sd:sd + 1]) and torch.equal(b, o0[sd:sd + 1]), sd


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    c = Case("fusion", "f32", 3, 2, 3, 5, 0, seed=120)
    out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
    out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
    n, hw = c.n, c.hw
    cases = [(dict(kx_ptr=None), L.EINVAL, b"keep pointer"), (dict(ke_ptr=None), L.EINVAL, b"keep pointer"), (dict(kw_ptr=None), L.EINVAL, b"keep pointer"),
             (dict(sx=n - 1), L.ESHAPE, b"stride"), (dict(se=n - 1), L.ESHAPE, b"stride"), (dict(sw=hw - 1), L.ESHAPE, b"stride"),
             (dict(se=1), L.ESHAPE, b"stride"), (dict(sw=-hw), L.ESHAPE, b"stride")]
    for bad, code, word in cases:
        assert c.launch(out_x.view, out_x0.view, **bad) == code and word in lib.tmix_last_error_string(), bad
    # the shape checks it shares with tmix_fused_tweedie_step_dev
    assert c.launch(out_x.view, out_x0.view, rows=c.K) == L.ESHAPE and c.launch(out_x.view, out_x0.view, seeds=0) == L.ESHAPE
    assert c.launch(None, out_x0.view) == L.EINVAL
    torch.cuda.synchronize()
    for f in (out_x, out_x0):                                  # nothing was launched: both outputs still hold the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


def test_ops_wrapper():
    from tweediemix_amd import lib as L, ops
    c = Case("fusion", "bf16", 3, 3, 37, 41, 0, shared=(True, False, True), frac=True, seed=130)
    ref, ref0 = c.reference()
    o0 = torch.empty_like(c.x_t)
    ox = ops.fused_tweedie_step_keep_dev(c.x_t, c.eps_t, c.m_t, L.STEP_FUSION, c.K, c.prm, c.kx_t, c.ke_t, c.kw_t, out_x0=o0)
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), ref) and np.array_equal(o0.cpu().numpy(), ref0)


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


def _standin_cfg(S, h, w):
    return S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=1,
                         resolution_h=h * 8, resolution_w=w * 8)


def _standin_eps(i, rows, seeds, h, w):
    """the stand-in UNet: a fixed seeded function of (call index, row)"""
    return torch.randn(seeds * rows, 4, h, w, generator=torch.Generator().manual_seed(1000 + i))


def _standin_sampler(lora, seeds, masks, log):
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    tw = S.Tweediemix(_standin_cfg(S, h, w), _NoWeights(), None, None, lambda x0: masks, concept_num=K, lora=lora, n_seeds=seeds)
    rows = {"fusion": K + 1, "fusion_base": K + 1, "start": K + 1, "plain": 2}

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return _standin_eps(len(log) - 1, rows[kind], seeds, h, w).cuda()
    tw._unet = unet
    return tw


def _loop_restatement(lora, seeds, xT, masks, keep):
    """numpy fp32 restatement of the sampler's loop with the keep term in every fused step: -> (the state handed to every UNet call, the final latent).
    keep = (kx [1|S,4,h,w], kw [1|S,1,h,w], ke [S,4,h,w]) as numpy."""
    from oracle import tweedie_oracle as TO
    K, n, h, w, g, R, J = 3, 10, 16, 16, NF(0.8), 1, 1
    sch = TO.Schedule(n)
    ts = [int(t) for t in sch.timesteps]
    ic, istop = int(n * 0.2), int(n * 0.8)
    t_cond_prev, t_cond_cur, start_t = ts[ic - 1], ts[ic], ts[0]
    t_stop_cur = ts[istop] if lora else None
    in_fusion = lambda t: (t <= t_cond_cur and t >= t_stop_cur) if lora else t <= t_cond_cur
    kx, kw, ke = keep
    pick = lambda a, sd: a[0:1] if a.shape[0] == 1 else a[sd:sd + 1]
    handed = []
    st = {"x": xT.copy(), "m": None}
    sa0, s10 = np.sqrt(NF(sch.alpha(ts[0]))).astype(NF), np.sqrt(NF(1) - NF(sch.alpha(ts[0]))).astype(NF)
    st["x"] = (kw * (sa0 * kx + s10 * ke) + (NF(1) - kw) * st["x"]).astype(NF)

    def step(mode, t, at, an, last=False):
        rows = 2 if mode == "plain_call" else K + 1
        kind_rows = rows
        handed.append((t, st["x"].copy()))
        eps = _standin_eps(len(handed) - 1, kind_rows, seeds, h, w).numpy()
        md = "plain" if mode in ("plain_call", "plain_on_start") else mode
        out = []
        for sd in range(seeds):
            o, _ = restate(md, st["x"][sd:sd + 1], eps[sd * rows:(sd + 1) * rows], st["m"], K, g, at, an, last, None, pick(kx, sd), pick(ke, sd), pick(kw, sd))
            out.append(o)
        st["x"] = np.concatenate(out)

    for t in ts:
        nt = t - sch.skip
        at, an, last = sch.alpha(t), sch.alpha(nt), t == 1
        if in_fusion(t):
            step("fusion", t, at, an, last)
        elif t == start_t:
            for _ in range(R):
                step("resample", t, at, an)
                step("plain_call", nt, an, at)
            step("plain_on_start", t, at, an, last)
        else:
            step("plain_call", t, at, an, last)
        if t == t_cond_prev:
            backup, tt = st["x"].copy(), nt
            for _ in range(J):
                step("plain_call", tt, sch.alpha(tt), sch.alpha(tt - 150))
                tt -= 150
            st["x"], st["m"] = backup, masks
    return handed, st["x"]


@pytest.mark.parametrize("lora,seeds", [(False, 1), (True, 1), (False, 2)])
def test_sampler_standin_unet_keeps_the_region_at_every_noise_level(lora, seeds):
    """latent 16 x 16, n_timesteps 10, t_cond 0.2, one resampling and one jumping step, K = 3 (LoRA: t_stop 0.8): the state handed to EVERY UNet call --
    the first (the initial composite), the start phase's re-noising calls, the look-ahead -- has its kept region equal to the closed form
    sa(t) keep_x0 + s1(t) keep_eps of that call's timestep; the final latent's kept region is keep_x0; the whole trajectory follows the fp32
    restatement of the loop within 2e-5 per step (tests/test_sampler_gpu.py's bound for its replayed trajectories); weight 0 is the plain sampler"""
    from tweediemix_amd import masks as M, ops
    K, h, w = 3, 16, 16
    masks = M.build_masks(M.partition_rectangle_masks(K, h * 8, w * 8, seed=3), h, w)
    g = torch.Generator().manual_seed(17 + seeds)
    xT, kx, ke = torch.randn(seeds, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g), torch.randn(seeds, 4, h, w, generator=g)
    kw = (1 - masks[1:2]).cpu()                                   # re-roll the second concept's region
    assert 0 < float(kw.sum()) < h * w
    log = []
    tw = _standin_sampler(lora, seeds, masks, log)
    tw.set_keep(kx, kw, ke)
    out = tw.run_fusion(xT.clone()).cpu()
    held = (kw == 1).expand(seeds, 4, h, w)
    assert len(log) == 3 + 1 + 1 + 8                              # start phase, t = 801, look-ahead, eight more timesteps
    for kind, t, x in log:
        sa, s1, _, _ = ops.step_coeffs(tw.alpha(t), tw.alpha(t))
        closed = sa * kx + s1 * ke                                  # (torch fp32: sa, s1 are fp32 values held in Python floats)
        assert torch.equal(x.cpu()[held], closed.expand(seeds, 4, h, w)[held]), (kind, t)
    assert torch.equal(out[held], kx.expand(seeds, 4, h, w)[held])
    assert not torch.equal(out[~held], kx.expand(seeds, 4, h, w)[~held])
    handed, final = _loop_restatement(lora, seeds, xT.numpy(), masks.cpu().numpy(), (kx.numpy(), kw.numpy(), ke.numpy()))
    assert [t for t, _x in handed] == [t for _k, t, _x in log]
    for (t, want), (_k, _t, got) in zip(handed, log):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-5, atol=2e-5, err_msg=f"state handed to the call at t={t}")
    np.testing.assert_allclose(out.numpy(), final, rtol=2e-5, atol=2e-5)
    # weight 0 everywhere: bit for bit the sampler that never heard of a keep region
    log0, logp = [], []
    tw0 = _standin_sampler(lora, seeds, masks, log0)
    tw0.set_keep(kx, torch.zeros_like(kw), ke)
    plain = _standin_sampler(lora, seeds, masks, logp)
    out0, outp = tw0.run_fusion(xT.clone()), plain.run_fusion(xT.clone())
    assert torch.equal(out0, outp) and len(log0) == len(logp)
    for a, b in zip(log0, logp):
        assert a[:2] == b[:2] and torch.equal(a[2], b[2]), a[:2]
    with pytest.raises(ValueError, match="set_keep"):
        tw.set_keep(kx, kw, ke[:, :3])
    with pytest.raises(ValueError, match="set_keep"):
        tw.set_keep(kx, kw.expand(seeds + 1, 1, h, w), ke)


# ------------------------------------------------------------------------------------------------ sampler on the tiny synthetic UNet (real plans)
def _tiny(kind, K=3):
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, kind, K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", (kind, con)), te, ts


class _Tiny:
    K, h, w = 3, 16, 16

    def __init__(self, kind="custom"):
        from tweediemix_amd import masks as M, sampler as S
        self.S, self.kind = S, kind
        self.W, self.te, self.ts = _tiny(kind, self.K)
        self.cfg = _standin_cfg(S, self.h, self.w)
        self.masks = M.build_masks(M.partition_rectangle_masks(self.K, self.h * 8, self.w * 8, seed=3), self.h, self.w)
        g = torch.Generator().manual_seed(23)
        self.xT, self.kx, self.ke = (torch.randn(2, 4, self.h, self.w, generator=g), torch.randn(1, 4, self.h, self.w, generator=g) * 0.5,
                                     torch.randn(2, 4, self.h, self.w, generator=g))
        self.kw = (1 - self.masks[1:2]).cpu()
        self.held = (self.kw == 1).expand(1, 4, self.h, self.w)

    def sampler(self, graphs=False, seeds=1):
        return self.S.Tweediemix(self.cfg, self.W, self.te, self.ts, lambda x0: self.masks, concept_num=self.K, lora=(self.kind == "lora"),
                                 use_graphs=graphs, n_seeds=seeds)


def test_tiny_unet_graph_replay_equals_eager_and_clear_keep_restores_the_plain_sampler(monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny("custom")
    eager, graph = T.sampler(False), T.sampler(True)
    outs = []
    for tw in (eager, graph):
        tw.set_keep(T.kx, T.kw, T.ke[0:1])
        outs.append(tw.run_fusion(T.xT[0:1].clone()).cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])               # graph replay == eager execution, bit for bit
    assert torch.equal(outs[0][T.held], T.kx[T.held]) and not torch.equal(outs[0][~T.held], T.kx[~T.held])
    assert any(len(k) == 3 and k[2] == "keep" for k in graph.graphs) and not any(len(k) == 2 for k in graph.graphs)
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()                                    # the captured keep steps, replayed from the first step on
    assert torch.equal(again, outs[0])
    # after clear_keep the run is the one of a sampler that never had a keep region (and the keep graphs are still there for the next set_keep)
    graph.clear_keep()
    cleared = graph.run_fusion(T.xT[0:1].clone()).cpu()
    fresh = T.sampler(True).run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.equal(cleared, fresh) and not torch.equal(cleared, outs[0])
    assert {len(k) for k in graph.graphs} == {2, 3}
    graph.set_keep(T.kx, T.kw, T.ke[0:1])
    assert torch.equal(graph.run_fusion(T.xT[0:1].clone()).cpu(), outs[0])


@pytest.mark.parametrize("kind", ["custom", "lora"])
def test_tiny_unet_two_co_batched_rerolls_equal_their_single_runs(kind, monkeypatch):
    """two re-rolls of one region share every UNet launch (kept latent and weight shared, stride 0); tiling pinned like tests/test_sampler_gpu.py's
    co-batch test pins it.  The re-rolled region differs between the seeds, the kept region is identical."""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny(kind)
    singles = []
    for i in range(2):
        tw = T.sampler()
        tw.set_keep(T.kx, T.kw, T.ke[i:i + 1])
        singles.append(tw.run_fusion(T.xT[i:i + 1].clone()).cpu())
    tw2 = T.sampler(seeds=2)
    tw2.set_keep(T.kx, T.kw, T.ke)
    both = tw2.run_fusion(T.xT.clone()).cpu()
    assert tw2.plan("fusion").B == 8 and tw2._keep[0].shape[0] == 1 and tw2._keep[1].shape[0] == 1
    for i in range(2):
        d = (both[i:i + 1] - singles[i]).abs().max().item()
        print(f"{kind} seed {i}: co-batched vs single run, max abs diff {d:.3g}")
        assert torch.equal(both[i:i + 1], singles[i]), (kind, i, d)
    assert torch.equal(singles[0][T.held], singles[1][T.held]) and torch.equal(singles[0][T.held], T.kx[T.held])
    assert not torch.equal(singles[0][~T.held], singles[1][~T.held])


def test_launch_list_without_set_keep_is_unchanged(monkeypatch):
    """a sampler that never called set_keep issues what it always issued: the same plan launches (names compared as tests/test_attn_masks_gpu.py compares
    a probe plan's) and tmix_fused_tweedie_step_dev for every step, never the keep entry; one that did issues the same plans and the keep entry only"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    lib = L.load()
    T = _Tiny("custom")
    calls = []
    for name in ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    names = lambda p: [getattr(fn, "__name__", "") for fn, _a in p.ops]
    plain = T.sampler()
    plain.run_fusion(T.xT[0:1].clone())
    n_plain, calls[:] = list(calls), []
    kept = T.sampler()
    kept.set_keep(T.kx, T.kw, T.ke[0:1])
    kept.run_fusion(T.xT[0:1].clone())
    assert n_plain == ["tmix_fused_tweedie_step_dev"] * len(plain.unet_calls) and len(plain.unet_calls) == 13
    assert calls == ["tmix_fused_tweedie_step_keep_dev"] * 13
    assert plain.unet_calls == kept.unet_calls and sorted(plain.plans) == sorted(kept.plans)
    for k in plain.plans:
        assert names(plain.plans[k]) == names(kept.plans[k]) and len(names(plain.plans[k])) > 50, k
        assert not any("tweedie" in n for n in names(plain.plans[k])), k                 # (the step entry is the sampler's, not a plan launch)
    assert plain._keep is None and plain._keep_bufs is None


# ------------------------------------------------------------------------------------------------ CLI
def _cli():
    spec = importlib.util.spec_from_file_location("fs_keep_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def _cli_common(tmp_path):
    from PIL import Image
    a, b = np.zeros((128, 128), np.uint8), np.zeros((128, 128), np.uint8)
    a[16:96, 8:56] = 255
    b[32:120, 72:120] = 255
    Image.fromarray(a).save(tmp_path / "a cat.png")
    Image.fromarray(b).save(tmp_path / "a dog.png")
    region = torch.from_numpy(b[::8, ::8] > 0)[None, None].expand(1, 4, 16, 16)           # the second concept's region on the latent grid
    common = ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--guidance_scale", "0.8",
              "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "1", "--resolution_h", "128", "--resolution_w", "128",
              "--output_path", str(tmp_path), "--mask_paths", f"{tmp_path / 'a cat.png'}+{tmp_path / 'a dog.png'}"]
    return common, region


def test_cli_keep_latents_rerolls_one_concept(tmp_path, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    fs = _cli()
    common, region = _cli_common(tmp_path)
    fs.main(common + ["--seed", "5", "--output_path_all", str(tmp_path / "first")])
    first_file = tmp_path / "first" / "p_5.latent.pt"
    first = torch.load(first_file)
    keep = ["--keep_latents", str(first_file), "--reroll", "1"]
    fs.main(common + keep + ["--seed", "7", "--output_path_all", str(tmp_path / "second")])
    second = torch.load(tmp_path / "second" / "p_7.latent.pt")
    assert second.shape == first.shape == (1, 4, 16, 16) and torch.isfinite(second).all()
    assert torch.equal(second[~region], first[~region])                                  # kept: bit for bit the first run's latent
    assert not torch.equal(second[region], first[region])                                # re-rolled: the second concept's region
    fs.main(common + ["--keep_latents", str(first_file), "--reroll", "a dog", "--seed", "7", "--num_seeds", "2", "--output_path_all", str(tmp_path / "two")])
    two = [torch.load(tmp_path / "two" / f"p_{s}.latent.pt") for s in (7, 8)]
    for lat in two:
        assert lat.shape == (1, 4, 16, 16) and torch.equal(lat[~region], first[~region]) and not torch.equal(lat[region], first[region])
    assert not torch.equal(two[0][region], two[1][region])


def test_cli_keep_image_holds_the_encoders_mean(tmp_path, monkeypatch):
    """--keep_image: the kept region of the final latent is VAEEncoderPlan's mean x the scaling factor decode_final divides by (the plan itself is the
    yardstick: no tolerance)"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from PIL import Image
    from tweediemix_amd import vae as V, video as VI
    fs = _cli()
    common, region = _cli_common(tmp_path)
    rgb = np.random.RandomState(4).randint(0, 256, (128, 128, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "template.png")
    lat = fs.main(common + ["--keep_image", str(tmp_path / "template.png"), "--reroll", "1", "--seed", "9", "--output_path_all", str(tmp_path / "img")]).cpu()
    plan = V.VAEEncoderPlan(V.TINY, V.synthetic_state_dict(V.TINY, encoder=True), 1, 128, 128)
    mean, _ = plan(VI.vae_pixel_values(Image.open(tmp_path / "template.png").convert("RGB")).cuda())
    want = (mean * 0.13025).cpu()                                                        # Tweediemix.vae_scaling_factor of a run without a vae/config.json
    assert torch.isfinite(lat).all() and torch.equal(lat[~region], want[~region]) and not torch.equal(lat[region], want[region])
    assert torch.equal(torch.load(tmp_path / "img" / "p_9.latent.pt"), lat)
