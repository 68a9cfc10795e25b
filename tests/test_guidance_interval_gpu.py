"""GPU: the guidance interval -- tmix_fused_tweedie_step_cond_dev, the plan kinds without the unconditional row, and
Tweediemix(guidance_interval=...) / --guidance_interval.

The kernel is compared with the numpy restatement guidance.cond_step_reference by np.array_equal and with its parent ENTRIES by torch.equal, never
by a tolerance.  The plan kinds are compared with the fp32 oracle within the bounds of tests/test_unet_gpu.py (rel-L2 2e-2, max 5e-2) and with the
rows of their guided twins bit for bit.  The stand-in trajectories are compared step by step with the restatement by equality and, as a whole, with
the fp32 loop restatement of tests/guidance_interval_cases.py within 2e-5 (the bound of tests/test_sampler_gpu.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import guidance_interval_cases as GC
from layout_frames import Frame, _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ("f32", "f16", "bf16")


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the step entry
@pytest.mark.parametrize("form", GC.FORMS)
@pytest.mark.parametrize("mode", GC.MODES)
@pytest.mark.parametrize("dt", DTS)
def test_kernel_equals_the_restatement(dt, mode, form):
    """C = 4, hw = 17 x 19 (n = 1292: six workgroups, the last one ragged), K = 3, two seeds; no noise, cz != 0 and the last step; masks per seed and
    shared; and one more eps row than the mode reads (rows >= K is the contract, not rows == K)"""
    i = 0
    for noise in GC.NOISES:
        for shared in (False, True):
            GC.Case(mode, dt, form, noise, shared_masks=shared, seed=i).cuda().check()
            i += 1
    GC.Case(mode, dt, form, "cz", rows=(2 if mode == "plain" else 4), seed=i).cuda().check()
    GC.Case(mode, dt, form, "none", K=1, seeds=1, h=8, w=8, seed=i + 1).cuda().check()          # one workgroup, one region
    c = GC.Case(mode, dt, form, "cz", seed=i + 2).cuda()
    quiet = GC.Case(mode, dt, form, "none", seed=i + 2).cuda()
    assert not torch.equal(c.run()[0], quiet.run()[0]) and torch.equal(c.run()[1], quiet.run()[1])      # the noise is there; the estimate does not see it


def test_g_slot_is_ignored():
    for form in ("ddim", "ms2"):
        a = GC.Case("fusion", "f32", form, seed=3, g_slot=0.8).cuda().run()
        b = GC.Case("fusion", "f32", form, seed=3, g_slot=float("nan")).cuda().run()
        for u, v in zip(a, b):
            assert torch.equal(u, v) and torch.isfinite(u).all()


@pytest.mark.parametrize("form", ["ddim", "ms2"])
def test_in_place_equals_out_of_place_inside_guard_bands(form):
    """x is out_x; every output in a guard-band frame (tests/layout_frames.py): nothing outside the views is written and no input changes"""
    c = GC.Case("fusion", "f32", form, "cz", seed=30).cuda()
    ox, o0, pv = c.run()
    S, n = c.seeds, c.n
    flat = lambda t, name: Frame.of(t.reshape(1, -1), name=name).seal()
    eps, masks, prm, keys = flat(c.eps_d, "eps"), flat(c.m_t, "masks"), flat(c.prm, "params"), flat(c.keys_t, "keys")
    prev = Frame.of(c.prev_t.reshape(S, n), name="x0_prev")
    if not c.ms:
        prev.seal()
    out0 = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x0")
    x = dense_guarded((S, n), F32, rows=8, device="cuda", name="x (in place)")
    x.view.copy_(c.x_t.reshape(S, n))
    assert c.launch(x.view, out0.view, prev.view, x=x.view, eps=eps.view, masks=masks.view, prm=prm.view, keys=keys.view) == 0
    torch.cuda.synchronize()
    for f in (x, out0):
        f.assert_untouched()
        f.assert_all_written()
    prev.assert_untouched()
    for f in (eps, masks, prm, keys) + (() if c.ms else (prev,)):                    # the DDIM form is not even handed the history
        f.assert_unchanged()
    assert torch.equal(x.view.reshape(ox.shape), ox) and torch.equal(out0.view.reshape(o0.shape), o0)
    assert torch.equal(prev.view.reshape(pv.shape), pv)
    # out of place: x itself is an untouched input; and without out_x0
    xin = flat(c.x_t, "x").seal()
    out = dense_guarded((S, n), F32, rows=8, device="cuda", name="out_x")
    p2 = c.prev_t.clone()
    assert c.launch(out.view, None, p2, x=xin.view) == 0
    torch.cuda.synchronize()
    out.assert_untouched()
    out.assert_all_written()
    xin.assert_unchanged()
    assert torch.equal(out.view.reshape(ox.shape), ox) and torch.equal(p2, pv)


@pytest.mark.parametrize("form", ["ddim", "ms2"])
def test_co_batched_launch_equals_seeds_one_at_a_time(form):
    c = GC.Case("fusion", "f16", form, "cz", seeds=3, seed=60).cuda()
    ox, o0, pv = c.run()
    for sd in range(c.seeds):
        a, b, p = torch.empty_like(c.x_t[sd:sd + 1]), torch.empty_like(c.x_t[sd:sd + 1]), c.prev_t[sd:sd + 1].clone()
        assert c.launch(a, b, p, x=c.x_t[sd:sd + 1], eps=c.eps_d[sd * c.rows:(sd + 1) * c.rows], masks=c.m_t[sd], seeds=1, keys=c.keys_t[sd:sd + 1]) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, ox[sd:sd + 1]) and torch.equal(b, o0[sd:sd + 1]) and torch.equal(p, pv[sd:sd + 1]), sd


def test_second_pass_of_the_grid_stride_loop():
    """hw = 384 x 384: n = 589,824 > 2048 workgroups x 256 threads, so threads of the capped grid take a second element"""
    c = GC.Case("fusion", "f32", "ms2", "none", seeds=1, h=384, w=384, seed=50)
    assert c.n == 4 * 384 * 384 > 2048 * 256
    c.cuda().check()


def test_nan_in_an_unused_history_stays_out_of_a_first_order_step():
    for mode in GC.MODES:
        c = GC.Case(mode, "f32", "ms1", seed=40).cuda()
        want = c.run()
        c.prev_t.fill_(float("nan"))
        got = c.run()
        for a, b in zip(got, want):
            assert torch.equal(a, b) and torch.isfinite(a).all()
        c2 = GC.Case(mode, "f32", "ms2", seed=40).cuda()                      # a second-order step does read it
        c2.prev_t.fill_(float("nan"))
        assert torch.isnan(c2.run()[0]).all()


def test_canvas_windows_index_the_canvas_noise():
    """x = 0, eps = 0: out_x is cz * z; two 16 x 16 windows of a 16 x 24 canvas hold the canvas-indexed noise, identical where they overlap"""
    from tweediemix_amd import canvas as CV, lib as L, noise as NZ, ops
    wins = CV.window_layout(16, 24, 16, 16, 8)
    assert len(wins) == 2
    x, eps = torch.zeros(2, 4, 16, 16, device="cuda"), torch.zeros(2, 4, 16, 16, device="cuda")
    keys = ops.noise_keys([GC.SEEDS64[1]], "cuda")
    for ms in (False, True):
        move = [0.8125, 0.4021, 0.0, 0.0, 0.8] if ms else [0.7071, 0.6123, 0.0, 0.8, 0.0]
        prm = torch.tensor([781.0, 0.6, 0.8] + move + [0.8125, 5.0, 0.0, 0.0], dtype=F32).cuda()
        out = ops.fused_tweedie_step_cond_dev(x, eps, None, L.STEP_PLAIN, 1, prm, x0_prev=torch.zeros_like(x) if ms else None, keys=keys, windows=wins,
                                              canvas_hw=(16, 24))
        torch.cuda.synchronize()
        full = (NF(0.8125) * NZ.normal(NZ.canvas_index(4, 16, 24), *NZ.seed_key(GC.SEEDS64[1]), 5)).astype(NF)
        for k, (oy, ox) in enumerate(wins):
            assert np.array_equal(out[k].cpu().numpy(), full[:, oy:oy + 16, ox:ox + 16]), (ms, k)


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    err = lib.tmix_last_error_string
    for form, noise in (("ms2", "cz"), ("ddim", "none")):
        c = GC.Case("fusion", "f32", form, noise, h=4, w=6, seed=70).cuda()
        out_x = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x")
        out_x0 = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="out_x0")
        prev = dense_guarded((c.seeds, c.n), F32, rows=8, device="cuda", name="x0_prev")
        go = lambda **kw: c.launch(out_x.view, out_x0.view, prev.view, **kw)
        own = b"tweedie_step_cond_dev: "
        assert go(mode=L.STEP_RESAMPLE) == L.EINVAL and err().startswith(own + b"bad mode 2 (FUSION or PLAIN)")
        assert go(mode=7) == L.EINVAL and go(mode=-1) == L.EINVAL
        assert c.launch(None, out_x0.view, prev.view) == L.EINVAL and err().startswith(own + b"null pointer")
        for null in ("x", "eps", "prm"):
            assert lib.tmix_fused_tweedie_step_cond_dev(*[None if i == {"x": 0, "eps": 1, "prm": 13}[null] else v
                                                          for i, v in enumerate(c.head(out_x.view, out_x0.view))], _p(prev.view) if c.ms else None,
                                                        _p(c.keys_t), c.w, 1, None, 0, 0, _st()) == L.EINVAL
        assert go(K=0) == L.EINVAL and err().startswith(own + b"FUSION needs masks and K>=1")
        assert lib.tmix_fused_tweedie_step_cond_dev(*[None if i == 3 else v for i, v in enumerate(c.head(out_x.view, out_x0.view))],
                                                    _p(prev.view) if c.ms else None, _p(c.keys_t), c.w, 1, None, 0, 0, _st()) == L.EINVAL
        assert go(dt=9) == L.EINVAL and err().startswith(own + b"bad eps dtype 9")
        assert go(rows=c.K - 1) == L.ESHAPE and err().startswith(own + b"mode 0 needs 3 eps rows per seed, got 2")
        assert go(mode=L.STEP_PLAIN, rows=0) == L.ESHAPE and err().startswith(own + b"mode 1 needs 1 eps rows per seed, got 0")
        assert go(seeds=0) == L.ESHAPE and go(seeds=65536) == L.ESHAPE and go(hw=0) == L.ESHAPE and go(C=0) == L.ESHAPE
        if c.nz:                                                                 # the window arguments are checked only when there is noise
            assert go(n_win=0) == L.EINVAL and go(n_win=L.MAX_WINDOWS + 1, yx=[0, 0] * (L.MAX_WINDOWS + 1), canvas=(4, 6)) == L.EINVAL
            assert go(n_win=2) == L.EINVAL
            assert go(w=5) == L.ESHAPE and b"w=5" in err()
            assert go(n_win=2, yx=[0, 0, 0, 3], canvas=(4, 8)) == L.ESHAPE and b"canvas" in err()
            assert go(n_win=2, yx=[0, 0, 0, 2], canvas=(4, 8), seeds=1) == L.ESHAPE and b"multiple" in err()
        torch.cuda.synchronize()
        for f in (out_x, out_x0, prev):                            # nothing was launched: every buffer still holds the sentinel everywhere
            assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name
    # without keys the window arguments are not read: nonsense there is no error
    c = GC.Case("plain", "f32", "ddim", "none", h=4, w=6, seed=71).cuda()
    a = c.run()
    b = c.run(w=5, n_win=0)
    assert torch.equal(a[0], b[0])


@pytest.mark.parametrize("dt", DTS)
def test_cross_check_against_the_parent_entries(dt):
    """PLAIN, and FUSION with K = 1, through the parents with the unconditional row a COPY of the conditional one (cfg(e, e, g) = e for any finite g):
    tmix_fused_tweedie_step_ms_dev gives out_x0, the history and out_x bit for bit, tmix_fused_tweedie_step_dev gives out_x0 bit for bit"""
    from tweediemix_amd import lib as L
    lib = L.load()
    for mode in GC.MODES:
        for form in ("ms1", "ms2", "ddim"):
            for g in (9.0, 0.8, -2.5):
                c = GC.Case(mode, dt, form, "none", K=1, seed=80, g_slot=g).cuda()
                got = c.run()
                S = c.seeds
                both = c.eps_d.reshape(S, 1, 4, c.h, c.w).repeat(1, 2, 1, 1, 1).reshape(2 * S, 4, c.h, c.w).contiguous()      # [uncond = cond, cond] per seed
                out_x, out_x0, prev = torch.empty_like(c.x_t), torch.empty_like(c.x_t), c.prev_t.clone()
                h = c.head(out_x, out_x0, eps=both, rows=2)
                if c.ms:
                    assert lib.tmix_fused_tweedie_step_ms_dev(*h[:7], _p(prev), *h[7:], _st()) == 0
                else:
                    assert lib.tmix_fused_tweedie_step_dev(*h, _st()) == 0
                torch.cuda.synchronize()
                what = (dt, mode, form, g)
                assert torch.equal(out_x0, got[1]), what
                if c.ms:
                    assert torch.equal(prev, got[2]) and torch.equal(out_x, got[0]), what
                else:
                    assert torch.isfinite(out_x).all() and torch.equal(prev, got[2])            # the DDIM parent's move uses another eps: x0 alone is compared


# ------------------------------------------------------------------------------------------------ plans (tiny UNet)
def _tiny(kind, K=3):
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, kind, K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", (kind, con)), te, ts, sd, con


def _oracle(kind, sd, con):
    from oracle import unet_oracle as UO
    if kind == "custom":
        oc = UO.Concepts("custom", kv={tb: [(c[f"{tb}.attn2.to_k.weight"], c[f"{tb}.attn2.to_v.weight"]) for c in con]
                                       for tb in UO.attention_prefixes(UO.TINY)})
    else:
        lo = {}
        for tb in UO.attention_prefixes(UO.TINY):
            for a in ("attn1", "attn2"):
                lo[f"{tb}.{a}"] = [{nm: (c[f"{tb}.{a}.processor.to_{nm}_lora.down.weight"], c[f"{tb}.{a}.processor.to_{nm}_lora.up.weight"])
                                    for nm in ("q", "k", "v", "out")} for c in con]
        oc = UO.Concepts("lora", lora=lo)
    return UO.UNetOracle(UO.TINY, sd, oc)


@pytest.mark.parametrize("kind", ["custom", "lora"])
def test_unguided_plans_match_the_oracle_and_the_rows_of_their_twins(kind, monkeypatch):
    """16 x 16 latent, TMIX_FORCE_TILE=1 (one tiling for every batch size, as the co-batch tests pin it).  The plain_c plan (B = 1) and the fusion_c
    plan (B = 3, weight sets 1..3) against the fp32 oracle run at B = 2 and B = 4 (rows 1 and 1..3; rel-L2 2e-2, max 5e-2: the bounds of
    test_unet_plan_matches_oracle); the same rows of the 2-row and the K + 1-row plan are equal bit for bit -- dropping a row does not change the
    others; and a replay gives the same bits"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import sampler as S
    K, h, w, t = 3, 16, 16, 601
    W, te, ts, sd, con = _tiny(kind, K)
    tw = S.Tweediemix(GC.make_cfg(S), W, te, ts, None, concept_num=K, lora=(kind == "lora"), guidance_interval=GC.INTERVAL)
    orc = _oracle(kind, sd, con)
    x = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(7))
    tid = lambda B: torch.tensor([[h * 8, w * 8, 0, 0, h * 8, w * 8]] * B, dtype=torch.float32)
    for kc, kg, rows, ehs, pooled, routed in (("plain_c", "plain", slice(1, 2), te[0][0:2], te[1][0:2], False),
                                              ("fusion_c", "fusion", slice(1, K + 1), torch.cat([te[0][0:1], te[0][2:2 + K]]),
                                               torch.cat([te[1][0:1], te[1][2:2 + K]]), True)):
        B = ehs.shape[0]
        ref = orc.forward(x.repeat(B, 1, 1, 1), t, ehs, pooled, tid(B), routed=routed)[rows]
        eps_c = tw._unet(kc, x.cuda(), t).float().clone()
        eps_g = tw._unet(kg, x.cuda(), t).float().clone()
        torch.cuda.synchronize()
        assert tw.plan(kc).B == B - 1 and tw.plan(kg).B == B and tw.unet_calls[-2:] == [(kc, B - 1, t), (kg, B, t)]
        assert torch.isfinite(eps_c).all()
        got = eps_c.cpu()
        r = ((got - ref).norm() / ref.norm()).item()
        m = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{kind} {kc}: rel_l2={r:.4g} max_rel={m:.4g}")
        assert r <= 2e-2 and m <= 5e-2, (kind, kc, r, m)
        assert torch.equal(eps_c, eps_g[rows]), (kind, kc, (eps_c - eps_g[rows]).abs().max().item())
        assert torch.equal(tw._unet(kc, x.cuda(), t).float(), eps_c), (kind, kc)          # replay is deterministic
    if kind == "lora":                                         # the window's off-by-one step: the same rows on the base weights
        eps_c = tw._unet("fusion_base_c", x.cuda(), t).float().clone()
        eps_g = tw._unet("fusion_base", x.cuda(), t).float().clone()
        assert torch.equal(eps_c, eps_g[1:]) and not torch.equal(eps_c, tw.plan("fusion_c").eps.float())


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
ENTRIES = ("tmix_fused_tweedie_step_dev", "tmix_fused_tweedie_step_keep_dev", "tmix_fused_tweedie_step_ms_dev", "tmix_fused_tweedie_step_rs_dev",
           "tmix_fused_tweedie_step_ms_rs_dev", "tmix_fused_tweedie_step_noise_dev", "tmix_fused_tweedie_step_cond_dev", "tmix_cfg_rescale_factors")
DEV, MS_, NOISE, COND, FACTORS = ENTRIES[0], ENTRIES[2], ENTRIES[5], ENTRIES[6], ENTRIES[7]


def _spy_entries(monkeypatch):
    """-> the list that receives the name of every step entry (and factor launch) the sampler calls"""
    from tweediemix_amd import lib as L
    lib, calls = L.load(), []
    for name in ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _standin_run(xT, seeds=None, log=None, **kw):
    tw, masks = GC.standin_sampler("cuda", seeds=xT.shape[0] if seeds is None else seeds, log=log, **kw)
    return tw, masks, tw.run_fusion(xT.clone())


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_standin_run_with_an_interval(solver, monkeypatch):
    """n = 10 on the leading grid, K = 3, two seeds, one resampling round trip and one look-ahead step, interval (700, 250): the `_c` kinds and
    their row counts sit exactly at the unguided entries; the run equals the run without the flag bit for bit up to the first unguided step;
    every step's result equals the restatement of the entry it went through; the trajectory follows the fp32 loop restatement within 2e-5"""
    from tweediemix_amd import guidance as G, lib as L, ops, solver as SV
    g, seeds = 0.8, 2
    xT = torch.randn(seeds, 4, GC.H, GC.W, generator=torch.Generator().manual_seed(43))
    calls, log = _spy_entries(monkeypatch), []
    tw, masks, out = _standin_run(xT, log=log, solver=solver, guidance_interval=GC.INTERVAL)
    ts = tw.scheduler.timesteps
    assert ts == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    want_calls = [("start", 4, 901), ("plain", 2, 801), ("start", 4, 901), ("plain_c", 1, 801), ("plain", 2, 701), ("fusion_c", 3, 701),
                  ("fusion", 4, 601), ("fusion", 4, 501), ("fusion", 4, 401), ("fusion", 4, 301), ("fusion_c", 3, 201), ("fusion_c", 3, 101),
                  ("fusion_c", 3, 1)]
    assert tw.unet_calls == want_calls
    guided_entry = MS_ if solver == "dpmpp2m" else DEV
    assert calls == [DEV] * 3 + [COND, DEV, COND] + [guided_entry] * 4 + [COND] * 3
    # the loop restatement, written without the sampler: the same calls, and every state within 2e-5
    ref_calls, ref_states = GC.loop_reference(xT.numpy(), masks.cpu().numpy(), GC.INTERVAL, solver=solver, g=g)
    assert ref_calls == want_calls
    traj = [2, 3] + list(range(5, 13))                            # call indices of the steps that advance the trajectory
    for i, ci in enumerate(traj):
        after = out if i == len(traj) - 1 else log[traj[i + 1]][2]
        np.testing.assert_allclose(after.cpu().numpy(), ref_states[i], rtol=2e-5, atol=2e-5, err_msg=f"{solver}: step {i} t={ts[i]}")
    # ... and every unguided step equals the entry's restatement on the eps it was handed, bit for bit
    mk, hist, last_ms = masks.cpu().numpy(), None, None
    for i, ci in enumerate(traj):
        kind, t, x, eps = log[ci]
        mode = L.STEP_FUSION if kind.startswith("fusion") else L.STEP_PLAIN
        cond = kind.endswith("_c")
        at, an = tw.alpha(t), tw.alpha(tw.scheduler.next_t(t))
        sa, s1, san, s1n = ops.step_coeffs(at, an)
        last = t == 1
        ms = solver == "dpmpp2m" and i > 0
        if ms:
            second = last_ms == (i - 1, mode, not cond)
            cf = (0.0, 1.0, 0.0) if last else SV.multistep_coeffs(tw.alpha(ts[i - 1]), at, an, second)
            assert second == (i in (4, 5, 6, 8, 9))               # first order at 801 (first solver step), 701 (mode), 601 and 201 (the borders)
            prm = [t, sa, s1, cf[0], cf[1], cf[2], float(last), g]
            last_ms = (i, mode, not cond)
        else:
            prm = [t, sa, s1, san, s1n, float(last), g, 0.0]
        after = (out if i == len(traj) - 1 else log[traj[i + 1]][2]).cpu().numpy()
        xs, es, rows = x.cpu().numpy(), eps.cpu().numpy(), GC.ROWS[kind]
        if hist is None:
            hist = np.zeros_like(xs)
        new_hist = hist.copy()
        for sd in range(seeds):
            if cond:
                a, b = G.cond_step_reference(mode, xs[sd:sd + 1], es[sd * rows:(sd + 1) * rows], mk if mode == L.STEP_FUSION else None,
                                             hist[sd:sd + 1] if ms else None, prm)
            elif ms:
                a, b = SV.multistep_step_reference(mode, xs[sd:sd + 1], es[sd * rows:(sd + 1) * rows], mk if mode == L.STEP_FUSION else None,
                                                   hist[sd:sd + 1], g, sa, s1, cf[0], cf[1], cf[2], last)
            else:
                K = 1 if mode == L.STEP_PLAIN else GC.K3
                a, b = G.rescaled_step_reference(mode, xs[sd:sd + 1], es[sd * rows:(sd + 1) * rows], mk, K, np.ones(K, NF), g, sa, s1, san, s1n, last)
            assert np.array_equal(after[sd:sd + 1], a), (solver, i, t, sd, kind)
            new_hist[sd:sd + 1] = b
        if ms:
            hist = new_hist
    # the guided prefix is the run without the flag, bit for bit: the states handed to the calls up to and including the first unguided one
    log0 = []
    tw0, _, out0 = _standin_run(xT, log=log0, solver=solver)
    assert [c[0] for c in tw0.unet_calls] == [c[0][:-2] if c[0].endswith("_c") else c[0] for c in want_calls]
    first = next(i for i, c in enumerate(want_calls) if c[0].endswith("_c"))
    assert first == 3
    for i in range(first + 1):
        assert torch.equal(log[i][2], log0[i][2]), i
    assert not torch.equal(log[first + 1][2], log0[first + 1][2]) and not torch.equal(out, out0)
    # a longer prefix: (1000, 250) is guided down to 301
    log1 = []
    tw1, _, out1 = _standin_run(xT, log=log1, solver=solver, guidance_interval=(1000, 250))
    assert [c[0] for c in tw1.unet_calls] == [c[0] for c in tw0.unet_calls[:10]] + ["fusion_c"] * 3
    for i in range(11):                                           # call 10 (fusion_c at 201) is the first unguided one: its input is still the plain run's
        assert torch.equal(log1[i][2], log0[i][2]), i
    assert not torch.equal(out1, out0) and torch.isfinite(out1).all()


@pytest.mark.parametrize("kw", [{}, dict(solver="dpmpp2m", timestep_spacing="logsnr"), dict(guidance_rescale=0.7), dict(eta=0.5, noise_seeds=[1, 2])],
                         ids=["ddim", "dpmpp2m_logsnr", "rescale", "eta"])
def test_full_interval_is_the_plain_run_bit_for_bit(kw, monkeypatch):
    xT = torch.randn(2, 4, GC.H, GC.W, generator=torch.Generator().manual_seed(44))
    calls = _spy_entries(monkeypatch)
    tw0, _, out0 = _standin_run(xT, **kw)
    base = list(calls)
    for interval in ((1000, 0), (901, 1)):
        calls[:] = []
        tw, _, out = _standin_run(xT, guidance_interval=interval, **kw)
        assert torch.equal(out, out0) and calls == base and tw.unet_calls == tw0.unet_calls and len(base) >= 13
        assert COND not in calls and tw.step_params.numel() == tw0.step_params.numel()


def test_standin_seed_of_a_co_batched_run_equals_its_single_run():
    kw = dict(solver="dpmpp2m", guidance_interval=GC.INTERVAL, eta=0.5)
    xT = torch.randn(3, 4, GC.H, GC.W, generator=torch.Generator().manual_seed(47))
    nseeds = [182, 183, GC.SEEDS64[2]]
    _, _, all3 = _standin_run(xT, noise_seeds=nseeds, **kw)
    for sd in range(3):
        _, _, one = _standin_run(xT[sd:sd + 1], noise_seeds=nseeds[sd:sd + 1], **kw)
        assert torch.equal(one[0], all3[sd]), sd


def test_standin_canvas_run_with_an_interval():
    """a 16 x 24 canvas (two windows) with eta: the unguided steps take the canvas-indexed noise, so the windows agree where they overlap before the
    consensus touches them -- the run is finite, deterministic, and differs from the run without the interval"""
    kw = dict(canvas=dict(height=16 * 8, width=24 * 8, overlap=64), eta=0.5, noise_seeds=[182])
    from tweediemix_amd import masks as M, sampler as S
    masks = M.build_masks(M.partition_rectangle_masks(GC.K3, 16 * 8, 24 * 8, seed=3), 16, 24)
    xT = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(48))
    outs = []
    for interval in (GC.INTERVAL, GC.INTERVAL, None):
        tw = S.Tweediemix(GC.make_cfg(S), GC.NoWeights("cuda"), None, None, lambda x0: masks, concept_num=GC.K3, guidance_interval=interval, **kw)
        tw._unet = lambda kind, x, t: GC.standin_eps(kind, x, t)
        outs.append(tw.run_fusion(xT.clone()))
        assert tw.n_seeds == 2 and torch.isfinite(outs[-1]).all() and outs[-1].shape == (1, 4, 16, 24)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ sampler on the tiny synthetic UNet (real plans)
class _Tiny:
    K, h, w = 3, 16, 16

    def __init__(self, kind="custom"):
        from tweediemix_amd import masks as M, sampler as S
        self.S, self.kind = S, kind
        self.W, self.te, self.ts, _sd, _con = _tiny(kind, self.K)
        self.cfg = GC.make_cfg(S)
        self.masks = M.build_masks(M.partition_rectangle_masks(self.K, self.h * 8, self.w * 8, seed=3), self.h, self.w)
        self.xT = torch.randn(2, 4, self.h, self.w, generator=torch.Generator().manual_seed(29))

    def sampler(self, graphs=False, seeds=1, **kw):
        return self.S.Tweediemix(self.cfg, self.W, self.te, self.ts, lambda x0: self.masks, concept_num=self.K, use_graphs=graphs, n_seeds=seeds,
                                 lora=(self.kind == "lora"), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(solver="dpmpp2m", timestep_spacing="logsnr", eta=0.5, noise_seeds=[182]), dict(n_streams=2)],
                         ids=["ddim", "dpmpp2m_eta", "two_streams"])
def test_tiny_unet_graph_replay_equals_eager(kw, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    T = _Tiny()
    eager, graph = T.sampler(False, guidance_interval=GC.INTERVAL, **kw), T.sampler(True, guidance_interval=GC.INTERVAL, **kw)
    a, b = eager.run_fusion(T.xT[0:1].clone()).cpu(), graph.run_fusion(T.xT[0:1].clone()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)                                  # graph replay == eager execution, bit for bit
    assert eager.unet_calls == graph.unet_calls and len(eager.unet_calls) == 13
    assert {k for k, _r, _t in eager.unet_calls} == {"start", "plain", "plain_c", "fusion", "fusion_c"}
    assert all(r == {"plain_c": 1, "fusion_c": 3}.get(k, r) for k, r, _t in eager.unet_calls)
    tail = (("ms",) if "solver" in kw else ()) + (("eta",) if "eta" in kw else ())
    cond_keys = sorted(k for k in graph.graphs if k[0].endswith("_c"))
    assert cond_keys == sorted([("plain_c", L.STEP_PLAIN) + tail, ("fusion_c", L.STEP_FUSION) + tail]), sorted(graph.graphs)
    assert len(graph.graphs) == 6, sorted(graph.graphs)
    again = graph.run_fusion(T.xT[0:1].clone()).cpu()                                     # every captured step replayed from the first one on
    assert torch.equal(again, a)
    assert not torch.equal(a, T.sampler(False, **kw).run_fusion(T.xT[0:1].clone()).cpu())     # and it is not the run without the interval


@pytest.mark.parametrize("kind", ["custom", "lora"])
def test_tiny_unet_two_co_batched_seeds_equal_their_single_runs(kind, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny(kind)
    both = T.sampler(False, seeds=2, guidance_interval=GC.INTERVAL).run_fusion(T.xT.clone())
    for sd in range(2):
        one = T.sampler(False, guidance_interval=GC.INTERVAL).run_fusion(T.xT[sd:sd + 1].clone())
        assert torch.equal(one[0], both[sd]), (kind, sd)


def test_tiny_unet_solver_eta_rescale_with_an_interval_skips_the_factor_launch(monkeypatch):
    """--solver dpmpp2m --eta 0.5 --guidance_rescale 0.7 with an interval: every guided step is a factor launch followed by the noise entry, every
    unguided step the unguided entry alone"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    T = _Tiny()
    calls = _spy_entries(monkeypatch)
    tw = T.sampler(False, solver="dpmpp2m", eta=0.5, noise_seeds=[182], guidance_rescale=0.7, guidance_interval=GC.INTERVAL)
    out = tw.run_fusion(T.xT[0:1].clone())
    assert torch.isfinite(out).all()
    kinds = [k for k, _r, _t in tw.unet_calls]
    assert kinds == ["start", "plain", "start", "plain_c", "plain", "fusion_c"] + ["fusion"] * 4 + ["fusion_c"] * 3
    want = []
    for i, k in enumerate(kinds):
        if k.endswith("_c"):
            want.append(COND)
        else:                                                # round trips and the look-ahead: the deterministic rs entry; trajectory steps: the noise entry
            want += [FACTORS, NOISE if i in (2, 6, 7, 8, 9) else "tmix_fused_tweedie_step_rs_dev"]
    assert calls == want
    tw_g = T.sampler(True, solver="dpmpp2m", eta=0.5, noise_seeds=[182], guidance_rescale=0.7, guidance_interval=GC.INTERVAL)
    assert torch.equal(tw_g.run_fusion(T.xT[0:1].clone()), out)
    assert all("rs" not in k for k in tw_g.graphs if k[0].endswith("_c")) and all("rs" in k for k in tw_g.graphs if not k[0].endswith("_c"))


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_run_with_an_interval_writes_its_outputs(tmp_path, monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("fs_interval_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
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
    lat = fs.main(common + ["--guidance_interval", "700,250", "--output_path_all", str(tmp_path / "gi")]).cpu()
    ref = fs.main(common + ["--output_path_all", str(tmp_path / "all")]).cpu()
    full = fs.main(common + ["--guidance_interval", "1000,0", "--output_path_all", str(tmp_path / "full")]).cpu()
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all() and not torch.equal(lat, ref) and torch.equal(full, ref)
    assert torch.equal(torch.load(tmp_path / "gi" / "p_5.latent.pt"), lat)
    assert Image.open(tmp_path / "gi" / "p_5.png").size == (128, 128)
    with pytest.raises(SystemExit, match="--guidance_interval"):
        fs.main(common + ["--guidance_interval", "250,700"])
