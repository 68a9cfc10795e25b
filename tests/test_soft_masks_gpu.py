"""GPU: soft region masks -- tmix_mask_edt, tmix_soft_masks, masks.soft_masks / soft_region, Tweediemix(mask_soften=...), --mask_feather /
--mask_dilate / --mask_normalize / --reroll_feather / --reroll_dilate.

The yardstick is the numpy restatement of DESIGN.md 7g (masks.mask_edt_reference: brute-force minima up to 64 x 64, the equally exact separable
form above, tied together in tests/test_soft_masks_cpu.py; masks.soft_masks_reference: every fp32 op rounded on its own).  Kernels are compared
with it by equality, never by a tolerance.  The two bounds in this file are derived where they are used: K * 2^-23 on the sum of normalised
weights, and the convex-hull bound on the stand-in trajectory."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from layout_frames import _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 7), (3, 16, 16), (2, 33, 65), (1, 64, 300), (2, 128, 128), (1, 8, 1024)]
KINDS = ("empty", "full", "corner", "rect_two_edges", "two_blobs", "checker", "random_half", "random_sparse")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _mask(kind, i, h, w):
    """one [h, w] fp32 mask; the random kinds hold VALUES in [0, 1) (the kernel thresholds at 0.5), the others {0, 1}"""
    rng = np.random.RandomState(1000 * KINDS.index(kind) + 17 * i + h + 3 * w)
    m = np.zeros((h, w), NF)
    if kind == "full":
        m[:] = 1
    elif kind == "corner":
        m[(h - 1) * (i % 2), (w - 1) * ((i // 2 + 1) % 2)] = 1
    elif kind == "rect_two_edges":
        m[: max(1, h // 2 + i), w - max(1, w // 3):] = 1
    elif kind == "two_blobs":
        ys, xs = np.mgrid[0:h, 0:w]
        for cy, cx, r in ((h * 0.3, w * 0.25, 0.2 * min(h, w) + 1), (h * 0.7, w * 0.75 - i, 0.15 * min(h, w) + 1)):
            m[(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = 1
    elif kind == "checker":
        ys, xs = np.mgrid[0:h, 0:w]
        m[(ys + xs + i) % 2 == 0] = 1
    elif kind == "random_half":
        m = rng.rand(h, w).astype(NF)
    elif kind == "random_sparse":
        m = (rng.rand(h, w).astype(NF) * NF(0.5) + (rng.rand(h, w) < 0.02).astype(NF) * NF(0.5)).astype(NF)
    return m


@functools.lru_cache(maxsize=None)
def _edt_case(shape, kind):
    """(masks [n,h,w], d_set, d_clear) of one shape and mask kind: the reference is computed once and shared"""
    from tweediemix_amd import masks as M
    n, h, w = shape
    masks = np.stack([_mask(kind, i, h, w) for i in range(n)])
    ds, dc = M.mask_edt_reference(masks)
    for a in (masks, ds, dc):
        a.setflags(write=False)
    return masks, ds, dc


# ------------------------------------------------------------------------------------------------ tmix_mask_edt
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_equals_restatement_inside_guard_bands(shape):
    """every mask kind at this shape: both outputs equal the restatement, every element is written, the sentinel around them survives, the mask
    is not written; and all kinds in ONE launch (8 n masks, kinds interleaved: another order and another grid) give the same distances"""
    from tweediemix_amd import lib as L, ops
    lib = L.load()
    n, h, w = shape
    per_kind = {}
    for kind in KINDS:
        masks, ds, dc = _edt_case(shape, kind)
        m = torch.from_numpy(masks.copy()).cuda()
        keep = m.clone()
        f_set = dense_guarded((n, h * w), torch.int32, rows=8, device="cuda", name=f"d_set[{kind}]")
        f_clr = dense_guarded((n, h * w), torch.int32, rows=8, device="cuda", name=f"d_clear[{kind}]")
        assert lib.tmix_mask_edt(m.data_ptr(), f_set.view.data_ptr(), f_clr.view.data_ptr(), n, h, w, _st()) == 0
        torch.cuda.synchronize()
        for f in (f_set, f_clr):
            f.assert_untouched()
            f.assert_all_written()
        assert torch.equal(m, keep)
        got_s, got_c = f_set.view.cpu().numpy().reshape(n, h, w), f_clr.view.cpu().numpy().reshape(n, h, w)
        assert np.array_equal(got_s, ds) and np.array_equal(got_c, dc), (shape, kind)
        per_kind[kind] = (got_s, got_c)
    assert (per_kind["empty"][0] == L.EDT_NONE).all() and (per_kind["full"][1] == L.EDT_NONE).all()
    order = [(kind, i) for i in range(n) for kind in reversed(KINDS)]
    allm = torch.from_numpy(np.stack([_edt_case(shape, kind)[0][i] for kind, i in order])).cuda()
    ds, dc = ops.mask_edt(allm)
    torch.cuda.synchronize()
    ds, dc = ds.cpu().numpy(), dc.cpu().numpy()
    for j, (kind, i) in enumerate(order):
        assert np.array_equal(ds[j], per_kind[kind][0][i]) and np.array_equal(dc[j], per_kind[kind][1][i]), (shape, kind, i)


def test_edt_captured_graph_replay_equals_eager_call():
    from tweediemix_amd import ops
    masks, ds, dc = _edt_case((2, 33, 65), "two_blobs")
    m = torch.from_numpy(masks.copy()).cuda()
    a, b = ops.mask_edt(m)                                         # warm-up outside capture (lazy module load)
    out = torch.empty(1, 3, 33, 65, device="cuda")
    ops.soft_masks(a.view(1, 2, 33, 65), b.view(1, 2, 33, 65), 2.5, 1.5, True, out=out)
    torch.cuda.synchronize()
    want = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_edt(m, a, b)
        ops.soft_masks(a.view(1, 2, 33, 65), b.view(1, 2, 33, 65), 2.5, 1.5, True, out=out)
    for t in (a, b, out):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), ds) and np.array_equal(b.cpu().numpy(), dc) and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ tmix_soft_masks
def _fg_sets(n_sets, K, h, w, seed=0):
    """[n_sets, K-1, h, w] {0, 1}: seeded rectangles that overlap freely; with three sets, one concept of set 1 is empty and one of set 2 full"""
    rng = np.random.RandomState(seed + 100 * n_sets + 10 * K)
    fg = np.zeros((n_sets, K - 1, h, w), NF)
    for s in range(n_sets):
        for k in range(K - 1):
            y0, x0 = rng.randint(0, h - 2), rng.randint(0, w - 2)
            fg[s, k, y0:y0 + rng.randint(2, h), x0:x0 + rng.randint(2, w)] = 1
    if n_sets == 3:
        fg[1, 0] = 0
        fg[2, K - 2] = 1
    return fg


@functools.lru_cache(maxsize=None)
def _soft_case(n_sets, K):
    from tweediemix_amd import masks as M
    h, w = 33, 65                                                  # 2145 pixels per set: several workgroups, a ragged last one
    fg = _fg_sets(n_sets, K, h, w)
    ds, dc = M.mask_edt_reference(fg)
    return fg, ds, dc


def _soft_ref(ds, dc, K, feather, dilate, normalize):
    from tweediemix_amd import masks as M
    assert ds.shape[1] == K - 1
    return M.soft_weights_reference(ds, dc, feather, dilate, normalize)


@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_soft_masks_equal_restatement(K, n_sets):
    """feather x dilate x normalize at this K and n_sets, by equality; the sum of normalised weights is 1 within K * 2^-23 (each of the K-1 quotients
    and each of the K-1 additions is one rounding of a value <= 1: at most 2^-24 each, and 2 (K - 1) * 2^-24 < K * 2^-23)"""
    from tweediemix_amd import masks as M, ops
    fg, ds, dc = _soft_case(n_sets, K)
    d_set, d_clear = ops.mask_edt(torch.from_numpy(fg).cuda().view(-1, 33, 65))
    assert np.array_equal(d_set.cpu().numpy().reshape(ds.shape), ds) and np.array_equal(d_clear.cpu().numpy().reshape(dc.shape), dc)
    d_set, d_clear = d_set.view(n_sets, K - 1, 33, 65), d_clear.view(n_sets, K - 1, 33, 65)
    seen_fraction = seen_scaled = False
    for feather in (0.0, 1.0, 2.5, 16.0):
        for dilate in (-3.0, 0.0, 1.5):
            for normalize in (False, True):
                want = _soft_ref(ds, dc, K, feather, dilate, normalize)
                f = dense_guarded((n_sets * K, 33 * 65), F32, rows=8, device="cuda", name="weights")
                got = ops.soft_masks(d_set, d_clear, feather, dilate, normalize, out=f.view.view(n_sets, K, 33, 65))
                torch.cuda.synchronize()
                f.assert_untouched()
                f.assert_all_written()
                got = got.cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (K, n_sets, feather, dilate, normalize)
                assert got.min() >= 0 and (got[:, :-1].max() <= 1)
                seen_fraction |= bool(((got > 0) & (got < 1)).any())
                if normalize:
                    tot = np.zeros_like(got[:, 0])
                    for k in range(K):
                        tot = (tot + got[:, k]).astype(NF)
                    assert np.abs(tot.astype(np.float64) - 1).max() <= K * 2.0 ** -23 and got.max() <= 1
                    seen_scaled |= bool((got[:, -1] == 0).any() and not np.array_equal(got, _soft_ref(ds, dc, K, feather, dilate, False)))
    assert seen_fraction and (seen_scaled or K == 2)                # (K = 2: one foreground weight never exceeds 1)
    # the front door gives the same: masks.soft_masks == masks.soft_masks_reference, 4-dim and 3-dim input
    a = M.soft_masks(torch.from_numpy(fg), 2.5, 1.5, True).cpu().numpy()
    assert a.shape == (n_sets, K, 1, 33, 65) and np.array_equal(a, M.soft_masks_reference(fg, 2.5, 1.5, True))
    b = M.soft_masks(fg[0], 2.5, 1.5, True).cpu().numpy()
    assert b.shape == (K, 1, 33, 65) and np.array_equal(b, a[0])


def test_identity_against_build_masks_bits_and_soft_region():
    from tweediemix_amd import masks as M
    for K, seed in ((3, 1), (4, 4)):                                # seed 4, K = 4: three mutually overlapping rectangles
        bm = M.build_masks(M.random_rectangle_masks(K, 128, 128, seed=seed), 16, 16)
        for feather in (0.0, 0.5, 1.0):
            got = M.soft_masks(bm[:-1, 0], feather, 0.0, False)
            assert got.shape == bm.shape and torch.equal(got, bm), (K, feather)
        assert not torch.equal(M.soft_masks(bm[:-1, 0], 2.0, 0.0, False), bm)
    region = bm[0:1]                                                # [1, 1, 16, 16]
    u = M.soft_region(region, 2.0, 1.0)
    assert u.shape == region.shape and np.array_equal(u.cpu().numpy()[0, 0], M.soft_masks_reference(region[0].cpu().numpy(), 2.0, 1.0)[0, 0])
    assert torch.equal(M.soft_region(region, 0.0, 0.0), region)


def test_second_pass_of_the_grid_stride_loop():
    """1 set x 768 x 700 = 537,600 pixels > 2048 workgroups x 256 threads: every thread of the capped grid takes a second pixel.  The distances
    come from tmix_mask_edt (compared with the restatement above); the weights from them are compared with the restatement's own steps"""
    from tweediemix_amd import ops
    h, w = 768, 700
    assert h * w > 2048 * 256
    fg = np.zeros((1, 2, h, w), NF)
    fg[0, 0, 100:500, 50:400] = 1
    fg[0, 1, 300:700, 200:650] = 1
    d_set, d_clear = ops.mask_edt(torch.from_numpy(fg).cuda().view(2, h, w))
    got = ops.soft_masks(d_set.view(1, 2, h, w), d_clear.view(1, 2, h, w), 16.0, 1.5, True).cpu().numpy()
    ds, dc = d_set.cpu().numpy().reshape(1, 2, h, w), d_clear.cpu().numpy().reshape(1, 2, h, w)
    assert ds[0, 0, 0, 0] == 100 * 100 + 50 * 50 and dc[0, 0, 300, 200] == 151 * 151      # spot checks of the large grid's distances
    assert np.array_equal(got, _soft_ref(ds, dc, 3, 16.0, 1.5, True))


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    h, w, K = 5, 7, 3
    m = torch.zeros(2, h, w, device="cuda")
    f_set = dense_guarded((2, h * w), torch.int32, rows=8, device="cuda", name="d_set")
    f_clr = dense_guarded((2, h * w), torch.int32, rows=8, device="cuda", name="d_clear")
    f_out = dense_guarded((K, h * w), F32, rows=8, device="cuda", name="weights")
    pm, ps, pc, po = m.data_ptr(), f_set.view.data_ptr(), f_clr.view.data_ptr(), f_out.view.data_ptr()
    edt = lambda mask=pm, a=ps, b=pc, n=2, h_=h, w_=w: lib.tmix_mask_edt(mask, a, b, n, h_, w_, _st())
    assert edt(mask=None) == L.EINVAL and edt(a=None) == L.EINVAL and edt(b=None) == L.EINVAL and b"null" in lib.tmix_last_error_string()
    assert edt(h_=0) == L.ESHAPE and edt(w_=4097) == L.ESHAPE and b"4097" in lib.tmix_last_error_string()
    assert edt(h_=4097) == L.ESHAPE and edt(n=0) == L.ESHAPE and edt(n=65536) == L.ESHAPE and edt(w_=-1) == L.ESHAPE
    soft = lambda a=ps, b=pc, o=po, n=1, K_=K, h_=h, w_=w, f=1.0, r=0.0, nz=0: lib.tmix_soft_masks(a, b, o, n, K_, h_, w_, f, r, nz, _st())
    assert soft(a=None) == L.EINVAL and soft(b=None) == L.EINVAL and soft(o=None) == L.EINVAL
    assert soft(f=-1.0) == L.EINVAL and b"feather=-1" in lib.tmix_last_error_string()
    assert soft(f=float("nan")) == L.EINVAL and b"nan" in lib.tmix_last_error_string().lower()
    assert soft(f=float("inf")) == L.EINVAL and soft(r=float("nan")) == L.EINVAL
    assert soft(K_=1) == L.ESHAPE and b"K=1" in lib.tmix_last_error_string()
    assert soft(h_=0) == L.ESHAPE and soft(w_=4097) == L.ESHAPE and soft(n=0) == L.ESHAPE
    torch.cuda.synchronize()
    for f in (f_set, f_clr, f_out):                                # nothing was launched: the views still hold the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
K4 = 4
ROWS = {"fusion": K4 + 1, "fusion_base": K4 + 1, "start": K4 + 1, "plain": 2}
SOFT = dict(feather=4.0, dilate=1.0, normalize=True)


class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = K4


def _cfg(S, h, w):
    return S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=1,
                         resolution_h=h * 8, resolution_w=w * 8)


def _eps(i, rows, h=16, w=16):
    """the stand-in UNet: a fixed seeded function of (call index, row), independent of the latent"""
    return torch.randn(rows, 4, h, w, generator=torch.Generator().manual_seed(4000 + i))


def _overlap_masks():
    from tweediemix_amd import masks as M
    return M.build_masks(M.random_rectangle_masks(K4, 128, 128, seed=4), 16, 16)


def _standin_run(masks, mask_soften, xT):
    """-> (final latent, [(kind, t, x handed to the call, eps)], [(x_state, x0_state) after every fused step], sampler)"""
    from tweediemix_amd import sampler as S
    tw = S.Tweediemix(_cfg(S, 16, 16), _NoWeights(), None, None, lambda x0: masks, concept_num=K4, mask_soften=mask_soften)
    log, states = [], []

    def unet(kind, x, t):
        e = _eps(len(log), ROWS[kind]).cuda()
        log.append((kind, int(t), x.clone(), e))
        return e
    tw._unet = unet
    real = tw._fused_step

    def fused(*a):
        real(*a)
        states.append((tw.x_state.clone(), tw.x0_state.clone()))
    tw._fused_step = fused
    out = tw.run_fusion(xT.clone())
    return out, log, states, tw


def _loop_np(weights, xT):
    """numpy fp32 restatement of the loop on the stand-in eps (oracle.tweedie_oracle's step functions): the max |x| over every state the loop
    writes, for constant blend weights [K,1,h,w]"""
    from oracle import tweedie_oracle as TO
    n, g = 10, NF(0.8)
    sch = TO.Schedule(n)
    ts = [int(t) for t in sch.timesteps]
    t_cond_prev, t_cond_cur, start_t = ts[1], ts[2], ts[0]
    st = {"x": xT.copy(), "i": 0, "max": float(np.abs(xT).max()), "m": None}

    def step(mode, at, an, last=False):
        rows = 2 if mode == "plain_call" else K4 + 1
        eps = _eps(st["i"], rows).numpy()
        st["i"] += 1
        if mode == "fusion":
            o, _ = TO.fused_fusion_step(st["x"], eps, st["m"], g, at, an, last)
        elif mode == "resample":
            o = TO.fused_resample_down(st["x"], eps, K4, g, at, an)
        else:
            o, _ = TO.fused_plain_step(st["x"], eps[:2], g, at, an, last)
        st["x"] = o
        st["max"] = max(st["max"], float(np.abs(o).max()))

    for t in ts:
        nt = t - sch.skip
        at, an, last = sch.alpha(t), sch.alpha(nt), t == 1
        if t <= t_cond_cur:
            step("fusion", at, an, last)
        elif t == start_t:
            step("resample", at, an)
            step("plain_call", an, at)
            step("plain_on_start", at, an, last)
        else:
            step("plain_call", at, an, last)
        if t == t_cond_prev:
            backup = st["x"].copy()
            step("plain_call", sch.alpha(nt), sch.alpha(nt - 150))
            st["x"], st["m"] = backup, weights
    assert st["i"] == 13
    return st["max"]


def _traj_max(states, xT):
    """max |x| over x_T and every state the loop wrote (what _loop_np tracks)"""
    return max(float(xT.abs().max()), max(float(x.abs().max()) for x, _x0 in states))


def test_sampler_standin_unet_soft_normalised_weights():
    """K = 4 on three mutually overlapping rectangles, mask_soften = feather 4, dilate 1, normalize: the weights the sampler holds are the
    restatement's; EVERY fusion step's x_state and x0_state equal oracle.tweedie_oracle.fused_fusion_step fed those weights and the step's own
    inputs, by equality.

    The bound on the trajectory.  The stand-in eps does not depend on the latent and the blend weights are constant over the fusion steps, so one
    fusion step is, per pixel p, x' = a x + sum_k w_k(p) b_k(p) with a and b_k independent of the weights (x0 = sum_k w_k (x - s1 e_k) / sa and
    sum_k w_k = 1).  By induction the state of a run with convex weights is at every step x(p) = sum_k w_k(p) x^(k)(p), x^(k) being the run that gives
    concept k weight 1 everywhere (the steps before the fusion phase do not read the weights: all runs share them).  Hence
        max |x_convex| <= max_k max |x^(k)| =: H      (the convex hull's extreme; fp32 rounding moves each side by far less than 1e-4 relative)
    for EVERY convex blend, the partition run included -- which picks x^(k(p))(p) per pixel.  The factor on the partition run's own maximum is
    therefore F = H / max |x_partition|, both from the numpy restatement of the loop (oracle step functions on the stand-in eps; nothing from
    the code under test).  The un-normalised weights sum to almost 3 on the triple overlap: that region multiplies at every fusion step and
    leaves the hull."""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import masks as M
    masks = _overlap_masks()
    assert float(masks[:-1].sum(0).max()) == 3.0
    xT = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(77))
    want_w = M.soft_masks_reference(masks[:-1, 0].cpu().numpy(), **SOFT)
    out, log, states, tw = _standin_run(masks, SOFT, xT)
    assert np.array_equal(tw.masks.cpu().numpy(), want_w) and torch.equal(tw.soft_weights, tw.masks)
    assert len(log) == len(states) == 13 and [k for k, *_ in log].count("fusion") == 8
    for (kind, t, x, e), (xs, x0s) in zip(log, states):
        if kind not in ("fusion", "fusion_base"):
            continue
        new, x0 = TO.fused_fusion_step(x.cpu().numpy(), e.cpu().numpy(), want_w, NF(0.8), tw.alpha(t), tw.alpha(t - tw.skip), t == 1)
        assert np.array_equal(xs.cpu().numpy(), new) and np.array_equal(x0s.cpu().numpy(), x0), (kind, t)
    assert torch.equal(out, states[-1][0])
    # the trajectory stays inside the convex hull of the pure-concept runs; the un-normalised run leaves it
    part = M.build_masks(M.partition_rectangle_masks(K4, 128, 128, seed=4), 16, 16)
    assert float(part.sum(0).min()) == float(part.sum(0).max()) == 1.0
    _pout, _plog, pstates, _ = _standin_run(part, None, xT)
    one_hot = lambda k: np.stack([np.full((1, 16, 16), float(j == k), NF) for j in range(K4)])
    hull = max(_loop_np(one_hot(k), xT.numpy()) for k in range(K4))
    part_np = _loop_np(part.cpu().numpy(), xT.numpy())
    factor = hull / part_np
    part_max, soft_max = _traj_max(pstates, xT), _traj_max(states, xT)
    assert abs(part_max - part_np) <= 1e-4 * part_np               # the partition run on the GPU is the restatement's
    _uout, _ulog, ustates, utw = _standin_run(masks, dict(SOFT, normalize=False), xT)
    raw_max = _traj_max(ustates, xT)
    print(f"max |x|: partition {part_max:.4g}, hull {hull:.4g} (factor {factor:.4g}), normalised soft {soft_max:.4g}, un-normalised soft {raw_max:.4g}; "
          f"largest un-normalised weight sum {float(utw.masks.sum(0).max()):.4g}")
    assert 1.0 <= factor and soft_max <= factor * part_max * (1 + 1e-4)
    assert raw_max > factor * part_max * (1 + 1e-4) and float(utw.masks.sum(0).max()) > 2.0


def test_sampler_standin_unet_identity_settings_are_the_plain_sampler():
    """mask_soften = None and feather 1 / dilate 0 / un-normalised: the same handed states and the same final latent, bit for bit, per seed masks
    included (two co-batched seeds with their own mask sets)"""
    from tweediemix_amd import masks as M, sampler as S
    sets = [M.build_masks(M.random_rectangle_masks(K4, 128, 128, seed=s), 16, 16) for s in (4, 8)]
    xT = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(78))
    outs = []
    for soften in (None, dict(feather=1.0, dilate=0.0, normalize=False), dict(feather=0.0)):
        turn = []
        tw = S.Tweediemix(_cfg(S, 16, 16), _NoWeights(), None, None, lambda x0: sets[(len(turn), turn.append(0))[0] % 2], concept_num=K4, n_seeds=2,
                          mask_soften=soften)
        log = []

        def unet(kind, x, t, log=log):
            log.append((kind, int(t), x.clone()))
            return torch.cat([_eps(2 * (len(log) - 1) + s, ROWS[kind]) for s in range(2)]).cuda()
        tw._unet = unet
        outs.append((tw.run_fusion(xT.clone()), log, tw))
    assert outs[0][2].soft_weights is None and outs[1][2].soft_weights is not None
    assert torch.equal(outs[0][2].masks, torch.stack(sets)) and outs[0][2].masks.shape == (2, K4, 1, 16, 16)
    for out, log, tw in outs[1:]:
        assert torch.equal(out, outs[0][0]) and torch.equal(tw.masks, outs[0][2].masks) and len(log) == len(outs[0][1]) == 13
        for a, b in zip(log, outs[0][1]):
            assert a[:2] == b[:2] and torch.equal(a[2], b[2]), a[:2]
    with pytest.raises(ValueError, match="mask_soften"):
        S.Tweediemix(_cfg(S, 16, 16), _NoWeights(), None, None, None, concept_num=K4, mask_soften=dict(feather=-1.0))
    with pytest.raises(ValueError, match="mask_soften"):
        S.Tweediemix(_cfg(S, 16, 16), _NoWeights(), None, None, None, concept_num=K4, mask_soften=dict(feather=1.0, blur=2))


# ------------------------------------------------------------------------------------------------ sampler on the tiny synthetic UNet (real plans)
def _tiny(K=3):
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, "custom", K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", ("custom", con)), te, ts


def test_tiny_unet_launch_list_without_mask_soften_is_unchanged(monkeypatch):
    """a sampler without mask_soften issues no tmix_mask_edt / tmix_soft_masks and the library calls it always issued; one with the identity
    settings issues exactly those calls plus ONE tmix_mask_edt and ONE tmix_soft_masks (the mask acquisition), the same plan launches, and ends in
    the same latent bit for bit; real softening changes the latent"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L, masks as M, sampler as S
    lib = L.load()
    calls = []
    for name in L.SIGNATURES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    K = 3
    W, te, ts = _tiny(K)
    masks = M.build_masks(M.random_rectangle_masks(K, 128, 128, seed=1), 16, 16)
    xT = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(23))
    names = lambda p: [getattr(fn, "__name__", "") for fn, _a in p.ops]
    launches = lambda c: [n for n in c if n not in ("tmix_last_error_string", "tmix_version")]
    runs = []
    for soften in (None, dict(feather=1.0, dilate=0.0, normalize=False), dict(feather=4.0, dilate=1.0, normalize=True)):
        calls[:] = []
        tw = S.Tweediemix(_cfg(S, 16, 16), W, te, ts, lambda x0: masks, concept_num=K, mask_soften=soften)
        out = tw.run_fusion(xT.clone()).cpu()
        runs.append((out, launches(calls), tw))
    new = ("tmix_mask_edt", "tmix_soft_masks")
    plain, ident, soft = runs
    assert not any(n in new for n in plain[1]) and plain[1].count("tmix_fused_tweedie_step_dev") == 13 and len(plain[1]) > 13 * 50
    for out, c, tw in (ident, soft):
        assert [n for n in c if n not in new] == plain[1] and c.count(new[0]) == 1 and c.count(new[1]) == 1
        assert c.index(new[1]) == c.index(new[0]) + 1
        assert tw.unet_calls == plain[2].unet_calls and sorted(tw.plans) == sorted(plain[2].plans)
        for k in tw.plans:
            assert names(tw.plans[k]) == names(plain[2].plans[k]), k
    assert torch.isfinite(plain[0]).all() and torch.equal(ident[0], plain[0]) and not torch.equal(soft[0], plain[0])


# ------------------------------------------------------------------------------------------------ canvas
GEO = dict(h=16, w=16, ch=16, cw=40, overlap=4)        # 1 x 3 windows, up to 2 covers (tests/test_canvas_gpu.py's WIDE)
K3 = 3
ROWS3 = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2}


class _NoWeights3(_NoWeights):
    K = K3


def _field(i, rows, seeds, h, w):
    return torch.randn(seeds * rows, 4, h, w, generator=torch.Generator().manual_seed(5000 + i))


def test_canvas_soft_weights_are_built_on_the_canvas_and_the_run_equals_the_plain_run():
    """1 x 3 windows of 16 x 16 on 16 x 40, overlapping rectangles drawn on the canvas, feather 4 / dilate 1 / normalize: every window's weights are
    the crop of the canvas weights (the restatement's, by equality), so overlapping windows hold identical weights; and with the stand-in UNet
    returning crops of one canvas-sized eps field, the canvas run is the plain run at resolution = canvas with the same mask_soften, bit for bit"""
    from tweediemix_amd import canvas as CV, masks as M, sampler as S
    geo, seeds = GEO, 2
    masks = M.build_masks(M.random_rectangle_masks(K3, geo["ch"] * 8, geo["cw"] * 8, seed=4), geo["ch"], geo["cw"])
    assert float(masks[:-1].sum(0).max()) == 2.0
    xT = torch.randn(seeds, 4, geo["ch"], geo["cw"], generator=torch.Generator().manual_seed(33))
    want_w = M.soft_masks_reference(masks[:-1, 0].cpu().numpy(), **SOFT)                 # [K, 1, 16, 40]
    # the plain run at canvas resolution
    plog = []
    ptw = S.Tweediemix(_cfg(S, geo["ch"], geo["cw"]), _NoWeights3(), None, None, lambda x0: masks, concept_num=K3, n_seeds=seeds, mask_soften=SOFT)

    def punet(kind, x, t):
        plog.append((kind, int(t), x.clone()))
        return _field(len(plog) - 1, ROWS3[kind], seeds, geo["ch"], geo["cw"]).cuda()
    ptw._unet = punet
    want = ptw.run_fusion(xT.clone())
    assert np.array_equal(ptw.masks.cpu().numpy(), np.stack([want_w] * seeds))
    # the canvas run
    log = []
    tw = S.Tweediemix(_cfg(S, geo["h"], geo["w"]), _NoWeights3(), None, None, lambda x0: masks, concept_num=K3, n_seeds=seeds, mask_soften=SOFT,
                      canvas=dict(height=geo["ch"] * 8, width=geo["cw"] * 8, overlap=geo["overlap"] * 8))

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        f = _field(len(log) - 1, ROWS3[kind], seeds, geo["ch"], geo["cw"]).reshape(seeds, ROWS3[kind], 4, geo["ch"], geo["cw"])
        wins = torch.stack([f[..., oy:oy + geo["h"], ox:ox + geo["w"]] for oy, ox in tw.windows], dim=1)
        return wins.reshape(-1, 4, geo["h"], geo["w"]).contiguous().cuda()
    tw._unet = unet
    got = tw.run_fusion(xT.clone())
    assert tw.windows == [(0, 0), (0, 12), (0, 24)] and tw.masks.shape == (3 * seeds, K3, 1, 16, 16)
    assert tw.soft_weights.shape == (seeds, K3, 1, 16, 40) and np.array_equal(tw.soft_weights[1].cpu().numpy(), want_w)
    for sd in range(seeds):
        for i, (oy, ox) in enumerate(tw.windows):
            assert np.array_equal(tw.masks[sd * 3 + i].cpu().numpy(), want_w[:, :, oy:oy + 16, ox:ox + 16]), (sd, i)
    assert ((want_w > 0) & (want_w < 1)).any() and torch.equal(tw.masks[0][..., 12:], tw.masks[1][..., :4])      # soft, and identical on the overlap
    assert got.shape == (seeds, 4, 16, 40) and torch.equal(got, want)
    assert len(log) == len(plog) == 13
    for (kind, t, x), (_k, _t, px) in zip(log, plog):
        assert torch.equal(x, CV.crop_windows(px, tw.windows, 16, 16)), (kind, t)


# ------------------------------------------------------------------------------------------------ CLI
def _cli():
    spec = importlib.util.spec_from_file_location("fs_soft_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """the CLI runs the tests below look at, made once: --synthetic --tiny at 128 x 128 pixels, two mask files, seed 5"""
    from PIL import Image
    mp = pytest.MonkeyPatch()
    mp.setenv("TMIX_FORCE_TILE", "1")
    tmp = tmp_path_factory.mktemp("soft_cli")
    a, b = np.zeros((128, 128), np.uint8), np.zeros((128, 128), np.uint8)
    a[16:96, 8:72] = 255
    b[32:120, 56:120] = 255                                                                  # the two regions overlap on columns 56..71
    Image.fromarray(a).save(tmp / "a cat.png")
    Image.fromarray(b).save(tmp / "a dog.png")
    common = ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--guidance_scale", "0.8",
              "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "1", "--resolution_h", "128", "--resolution_w", "128",
              "--mask_paths", f"{tmp / 'a cat.png'}+{tmp / 'a dog.png'}", "--seed", "5"]
    fs = _cli()
    out = {"tmp": tmp, "fs": fs, "common": common, "a": a, "b": b}
    variants = {"plain": [], "zeros": ["--mask_feather", "0", "--mask_dilate", "0"], "f8": ["--mask_feather", "8"],
                "soft": ["--mask_feather", "32", "--mask_normalize"]}
    try:
        for name, extra in variants.items():
            fs.main(common + extra + ["--output_path", str(tmp / f"side_{name}"), "--output_path_all", str(tmp / name)])
            out[name] = torch.load(tmp / name / "p_5.latent.pt")
    finally:
        mp.undo()
    return out


def test_cli_defaults_and_identity_flags_reproduce_the_run_without_flags(cli_runs):
    plain = cli_runs["plain"]
    assert plain.shape == (1, 4, 16, 16) and torch.isfinite(plain).all()
    assert torch.equal(cli_runs["zeros"], plain) and torch.equal(cli_runs["f8"], plain)
    tmp = cli_runs["tmp"]
    assert not os.path.exists(tmp / "side_plain" / "a cat_soft.png") and not os.path.exists(tmp / "side_zeros" / "a cat_soft.png")


def test_cli_soft_normalised_masks_change_the_latent_and_write_the_weights(cli_runs):
    from PIL import Image
    from tweediemix_amd import masks as M
    tmp = cli_runs["tmp"]
    assert torch.isfinite(cli_runs["soft"]).all() and not torch.equal(cli_runs["soft"], cli_runs["plain"])
    fg = np.stack([M.preprocess_mask(cli_runs[k], 16, 16, "cpu").numpy()[0, 0] for k in ("a", "b")])
    want = M.soft_masks_reference(fg, 4.0, 0.0, True)                                    # 32 image pixels = 4 latent pixels
    for k, name in enumerate(("a cat", "a dog")):
        img = np.array(Image.open(tmp / "side_soft" / f"{name}_soft.png"))
        assert img.shape == (16, 16) and img.dtype == np.uint8 and np.array_equal(img, np.round(want[k, 0] * 255.0).astype(np.uint8))
        assert ((img > 0) & (img < 255)).any()
        hard = np.array(Image.open(tmp / "side_f8" / f"{name}_soft.png"))                # --mask_feather 8: the hard mask itself
        assert np.array_equal(hard, (fg[k] * 255).astype(np.uint8))


def test_cli_feathered_keep_region(cli_runs, monkeypatch):
    """--reroll_feather 16 --reroll_dilate 8 (2 and 1 latent pixels): the final latent is the kept one bit for bit exactly where the kept weight
    1 - soft_region(union) is 1, and differs everywhere in the re-rolled core (weight 0)"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import masks as M
    tmp, fs = cli_runs["tmp"], cli_runs["fs"]
    first = cli_runs["plain"]
    keep = ["--keep_latents", str(tmp / "plain" / "p_5.latent.pt"), "--reroll", "1", "--reroll_feather", "16", "--reroll_dilate", "8", "--seed", "7"]
    fs.main(cli_runs["common"] + keep + ["--output_path", str(tmp / "side_keep"), "--output_path_all", str(tmp / "keep")])
    second = torch.load(tmp / "keep" / "p_7.latent.pt")
    region = M.preprocess_mask(cli_runs["b"], 16, 16, "cpu").numpy()[0]                  # [1, 16, 16]: the second concept's region
    kw = (NF(1) - M.soft_masks_reference(region, 2.0, 1.0)[0, 0]).astype(NF)             # [16, 16]
    held, core = torch.from_numpy(kw == 1)[None, None].expand(1, 4, 16, 16), torch.from_numpy(kw == 0)[None, None].expand(1, 4, 16, 16)
    assert held.any() and core.any() and ((kw > 0) & (kw < 1)).any() and int((kw < 1).sum()) > int(region.sum())       # the ramp reaches outside the region
    assert second.shape == first.shape and torch.isfinite(second).all()
    assert torch.equal(second[held], first[held])
    assert bool((second[core] != first[core]).all())
    ramp = torch.from_numpy((kw > 0) & (kw < 1))[None, None].expand(1, 4, 16, 16)
    assert not torch.equal(second[ramp], first[ramp])
    assert not os.path.exists(tmp / "side_keep" / "a dog_soft.png")                       # (no --mask_* flag: the blend masks stayed hard)
