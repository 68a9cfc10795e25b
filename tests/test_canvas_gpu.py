"""GPU: wide canvases -- tmix_window_consensus, Tweediemix(canvas=...), --canvas_h / --canvas_w / --window_overlap.

The kernel is compared with a numpy fp32 restatement (`consensus_np`: per canvas pixel, over the covering windows in ascending index,
acc = acc + wt * v and ws = ws + wt from 0, r = acc / ws, written to every covering window; a pixel of one window is left alone) by
np.array_equal on the BITS, never by a tolerance.  The one tolerance in this file (rtol = atol = 2e-5 on the stand-in-UNet trajectories)
is tests/test_sampler_gpu.py's bound for its replayed trajectories."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from layout_frames import SENTINEL, Frame, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def consensus_np(x, offs, ch, cw, weight=None):
    """x [G, n, C, h, w] fp32 -> the reconciled copy.  weight [h, w] fp32 or None (all ones)."""
    G, n, C, h, w = x.shape
    wt = np.ones((h, w), NF) if weight is None else weight.astype(NF)
    acc, ws, cnt = np.zeros((G, C, ch, cw), NF), np.zeros((ch, cw), NF), np.zeros((ch, cw), np.int32)
    for i, (oy, ox) in enumerate(offs):                          # ascending window index; separate product and sum, both rounded to fp32
        prod = (wt * x[:, i]).astype(NF)
        acc[:, :, oy:oy + h, ox:ox + w] = (acc[:, :, oy:oy + h, ox:ox + w] + prod).astype(NF)
        ws[oy:oy + h, ox:ox + w] = (ws[oy:oy + h, ox:ox + w] + wt).astype(NF)
        cnt[oy:oy + h, ox:ox + w] += 1
    assert cnt.min() >= 1
    with np.errstate(invalid="ignore"):
        r = (acc / ws).astype(NF)
    out = x.copy()
    for i, (oy, ox) in enumerate(offs):
        many = cnt[oy:oy + h, ox:ox + w] >= 2
        out[:, i] = np.where(many, r[:, :, oy:oy + h, ox:ox + w], x[:, i])
    assert out.dtype == NF
    return out, cnt


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _layouts():
    from tweediemix_amd import canvas as CV
    return {
        "1x3": (16, 16, 16, 40, CV.window_layout(16, 40, 16, 16, 4)),          # up to 2 covers
        "1x4": (16, 16, 16, 28, CV.window_layout(16, 28, 16, 16, 12)),         # up to 4 covers
        "2x2": (16, 16, 24, 24, CV.window_layout(24, 24, 16, 16, 8)),          # the 4-cover corner
        "8": (16, 16, 16, 72, CV.window_layout(16, 72, 16, 16, 8)),            # eight windows
        "odd": (5, 7, 5, 16, CV.window_layout(5, 16, 5, 7, 2)),                # odd window 5 x 7, no alignment anywhere
        "one": (16, 16, 16, 16, CV.window_layout(16, 16, 16, 16, 8)),          # n_win = 1: nothing launched
    }


LAYOUTS = ("1x3", "1x4", "2x2", "8", "odd", "one")


def _case(name, groups, C, tent, seed=0):
    from tweediemix_amd import canvas as CV
    h, w, ch, cw, offs = _layouts()[name]
    rng = np.random.RandomState(seed + 17 * groups + 5 * C + len(offs))
    x = rng.randn(groups, len(offs), C, h, w).astype(NF)
    weight = CV.tent_weight(h, w) if tent else None
    return h, w, ch, cw, offs, x, weight


def _run(x, offs, ch, cw, weight, groups):
    from tweediemix_amd import ops
    G, n, C, h, w = x.shape
    xt = torch.from_numpy(x).reshape(G * n, C, h, w).cuda()
    ops.window_consensus(xt, groups, offs, (ch, cw), None if weight is None else weight.cuda())
    torch.cuda.synchronize()
    return xt.cpu().numpy().reshape(x.shape)


@pytest.mark.parametrize("name", LAYOUTS)
def test_kernel_equals_restatement(name):
    expect_max = {"1x3": 2, "1x4": 4, "2x2": 4, "8": 2, "odd": 2, "one": 1}[name]
    for groups in (1, 2):
        for C in (3, 4):
            for tent in (False, True):
                h, w, ch, cw, offs, x, weight = _case(name, groups, C, tent)
                want, cnt = consensus_np(x, offs, ch, cw, None if weight is None else weight.numpy())
                assert cnt.max() == expect_max and cnt[0, 0] == cnt[-1, -1] == 1, (name, cnt.max())
                got = _run(x, offs, ch, cw, weight, groups)
                assert np.array_equal(bits(got), bits(want)), (name, groups, C, tent)
                if len(offs) > 1:
                    assert not np.array_equal(got, x)
                else:
                    assert np.array_equal(bits(got), bits(x))


def test_layout_sizes_are_the_issues():
    L = _layouts()
    assert [len(L[k][4]) for k in LAYOUTS] == [3, 4, 4, 8, 3, 1]
    assert L["2x2"][4] == [(0, 0), (0, 8), (8, 0), (8, 8)] and L["odd"][4] == [(0, 0), (0, 4), (0, 9)]


@pytest.mark.parametrize("name", ["1x4", "2x2", "odd"])
def test_single_cover_elements_keep_their_bits_and_guard_bands_stay(name):
    """x lives in a guard-band frame (tests/layout_frames.py); every single-cover element holds a NaN of the frame's own sentinel payload, which the
    kernel must neither rewrite (a NaN that went through arithmetic would lose it) nor count as written; the weight is an input frame that stays
    as it is.  Everything outside the view is untouched."""
    from tweediemix_amd import ops
    groups, C = 2, 3
    h, w, ch, cw, offs, x, weight = _case(name, groups, C, True, seed=40)
    _, cnt = consensus_np(x, offs, ch, cw, weight.numpy())
    single = np.zeros(x.shape, bool)
    for i, (oy, ox) in enumerate(offs):
        single[:, i] = (cnt[oy:oy + h, ox:ox + w] == 1)[None, None]
    assert single.any() and not single.all()
    xb = bits(x).copy()
    xb[single] = np.int32(SENTINEL[F32])
    x = xb.view(NF)
    want, _ = consensus_np(x, offs, ch, cw, weight.numpy())
    n = len(offs)
    fx = dense_guarded((groups * n, C * h * w), F32, rows=8, device="cuda", name="x (in place)")
    fx.view.copy_(torch.from_numpy(x).reshape(groups * n, C * h * w))
    fw = Frame.of(weight.cuda().reshape(1, h * w), name="weight").seal()
    ops.window_consensus(fx.view.view(groups * n, C, h, w), groups, offs, (ch, cw), fw.view.view(h, w))
    torch.cuda.synchronize()
    fx.assert_untouched()
    fw.assert_unchanged()
    got = fx.view.cpu().numpy().reshape(x.shape)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got)[single], xb[single]) and (bits(got)[single] == np.int32(SENTINEL[F32])).all()
    assert not np.isnan(got[~single]).any()
    # NULL weight, the same frame discipline
    want1, _ = consensus_np(x, offs, ch, cw, None)
    fx.view.copy_(torch.from_numpy(x).reshape(groups * n, C * h * w))
    ops.window_consensus(fx.view.view(groups * n, C, h, w), groups, offs, (ch, cw))
    torch.cuda.synchronize()
    fx.assert_untouched()
    assert np.array_equal(bits(fx.view.cpu().numpy().reshape(x.shape)), bits(want1))


def test_second_pass_of_the_grid_stride_loop():
    """2 groups x 4 channels x 256 x 384 canvas pixels = 786,432 > 2048 workgroups x 256 threads: every thread of the capped grid takes a second pixel"""
    from tweediemix_amd import canvas as CV
    h = w = 256
    ch, cw = 256, 384
    offs = CV.window_layout(ch, cw, h, w, 64)
    assert offs == [(0, 0), (0, 128)] and 2 * 4 * ch * cw > 2048 * 256
    x = np.random.RandomState(3).randn(2, 2, 4, h, w).astype(NF)
    weight = CV.tent_weight(h, w)
    want, _ = consensus_np(x, offs, ch, cw, weight.numpy())
    assert np.array_equal(bits(_run(x, offs, ch, cw, weight, 2)), bits(want))


def test_error_codes_without_a_launch():
    import ctypes as C
    from tweediemix_amd import lib as L
    lib = L.load()
    h, w, ch, cw, offs, x, _ = _case("1x3", 1, 4, False)
    f = dense_guarded((3, 4 * h * w), F32, rows=8, device="cuda", name="x")
    yx = lambda v: (C.c_int32 * len(v))(*v)
    good = [0, 0, 0, 12, 0, 24]
    st = torch.cuda.current_stream().cuda_stream
    call = lambda p, groups, n, v, c_, h_, w_, ch_, cw_: lib.tmix_window_consensus(p, groups, n, yx(v), c_, h_, w_, ch_, cw_, None, st)
    p = f.view.data_ptr()
    assert call(None, 1, 3, good, 4, h, w, ch, cw) == L.EINVAL
    assert call(p, 1, 9, good * 3, 4, h, w, ch, cw) == L.EINVAL and call(p, 1, 0, good, 4, h, w, ch, cw) == L.EINVAL and call(p, 0, 3, good, 4, h, w, ch, cw) == L.EINVAL
    assert call(p, 1, 3, [0, 0, 0, 12, 0, 25], 4, h, w, ch, cw) == L.ESHAPE and b"outside" in lib.tmix_last_error_string()
    assert call(p, 1, 3, [0, 0, 0, 4, 0, 24], 4, h, w, ch, cw) == L.ESHAPE and b"uncovered" in lib.tmix_last_error_string()
    assert call(p, 1, 3, good, 0, h, w, ch, cw) == L.ESHAPE
    torch.cuda.synchronize()
    f.assert_untouched()
    assert bool((f.bits == f.bits[0]).all())                     # nothing was launched: the view still holds the sentinel too


def test_captured_graph_replay_equals_eager_call():
    """the offsets travel in the kernel arguments: a captured launch carries them by value (the host array is gone by the time of the replay)"""
    from tweediemix_amd import ops
    h, w, ch, cw, offs, x, weight = _case("2x2", 2, 4, True, seed=60)
    wt = weight.cuda()
    src = torch.from_numpy(x).reshape(8, 4, h, w).cuda()
    eager = ops.window_consensus(src.clone(), 2, offs, (ch, cw), wt)
    buf = src.clone()
    ops.window_consensus(buf, 2, offs, (ch, cw), wt)             # warm-up outside capture (lazy module load)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.window_consensus(buf, 2, list(offs), (ch, cw), wt)
    for _ in range(2):
        buf.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, eager)
    want, _ = consensus_np(x, offs, ch, cw, weight.numpy())
    assert np.array_equal(bits(buf.cpu().numpy().reshape(x.shape)), bits(want))


# ------------------------------------------------------------------------------------------------ sampler with a stand-in UNet
class _NoWeights:
    device = torch.device("cuda")
    kind = "custom"
    K = 3


K = 3
ROWS = {"fusion": K + 1, "fusion_base": K + 1, "start": K + 1, "plain": 2}
WIDE = dict(h=16, w=16, ch=16, cw=40, overlap=4)        # 1 x 3 windows, up to 2 covers
SQUARE = dict(h=16, w=16, ch=24, cw=24, overlap=8)      # 2 x 2 windows, the corner covered 4 times


def _cfg(S, h, w):
    return S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=1,
                         resolution_h=h * 8, resolution_w=w * 8)


def _field(i, rows, seeds, h, w):
    """the stand-in UNet: a fixed seeded function of (call index, row) on an h x w grid"""
    return torch.randn(seeds * rows, 4, h, w, generator=torch.Generator().manual_seed(2000 + i))


def _inputs(geo, seeds):
    from tweediemix_amd import masks as M
    masks = M.build_masks(M.partition_rectangle_masks(K, geo["ch"] * 8, geo["cw"] * 8, seed=3), geo["ch"], geo["cw"])
    xT = torch.randn(seeds, 4, geo["ch"], geo["cw"], generator=torch.Generator().manual_seed(31 + seeds))
    return masks, xT


def _plain_run(geo, lora, seeds, masks, xT):
    """a plain Tweediemix at resolution = canvas whose stand-in UNet returns one canvas-sized eps field per call"""
    from tweediemix_amd import sampler as S
    log, previews = [], []

    def provider(x0):
        previews.append(x0.clone())
        return masks
    tw = S.Tweediemix(_cfg(S, geo["ch"], geo["cw"]), _NoWeights(), None, None, provider, concept_num=K, lora=lora, n_seeds=seeds)

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return _field(len(log) - 1, ROWS[kind], seeds, geo["ch"], geo["cw"]).cuda()
    tw._unet = unet
    return tw.run_fusion(xT.clone()), log, previews


def _canvas_sampler(geo, lora, seeds, masks, eps_of_call, log, previews):
    from tweediemix_amd import sampler as S

    def provider(x0):
        previews.append(x0.clone())
        return masks
    tw = S.Tweediemix(_cfg(S, geo["h"], geo["w"]), _NoWeights(), None, None, provider, concept_num=K, lora=lora, n_seeds=seeds,
                      canvas=dict(height=geo["ch"] * 8, width=geo["cw"] * 8, overlap=geo["overlap"] * 8))

    def unet(kind, x, t):
        log.append((kind, int(t), x.clone()))
        return eps_of_call(len(log) - 1, ROWS[kind], tw).cuda()
    tw._unet = unet
    return tw


def _crops_of_field(geo, seeds):
    """eps of the canvas sampler's calls: every window's rows are its crop of the ONE canvas-sized field of that call (row b = (seed * n_win + window) * rows + r)"""
    def eps(i, rows, tw):
        f = _field(i, rows, seeds, geo["ch"], geo["cw"]).reshape(seeds, rows, 4, geo["ch"], geo["cw"])
        wins = torch.stack([f[..., oy:oy + geo["h"], ox:ox + geo["w"]] for oy, ox in tw.windows], dim=1)
        return wins.reshape(-1, 4, geo["h"], geo["w"]).contiguous()
    return eps


def _agree_on_overlaps(tw, x):
    from tweediemix_amd import canvas as CV
    back = CV.crop_windows(CV.assemble(x, tw.windows, tw.canvas_h, tw.canvas_w), tw.windows, tw.h, tw.w)
    return torch.equal(back, x)


@pytest.mark.parametrize("lora,seeds", [(False, 1), (True, 1), (False, 2)])
def test_sampler_wide_canvas_equals_the_plain_sampler_at_canvas_resolution(lora, seeds):
    """1 x 3 windows of 16 x 16 on 16 x 40 (no pixel covered more than twice, and the mean of two equal values is that value): with the stand-in UNet
    returning crops of one canvas-sized eps field, the canvas run IS the plain run at resolution = canvas, bit for bit -- final latent, the state handed
    to every call (cropped), the preview handed to the mask provider.  Checks the crop, mask and noise plumbing."""
    from tweediemix_amd import canvas as CV
    geo = WIDE
    masks, xT = _inputs(geo, seeds)
    want, plog, pprev = _plain_run(geo, lora, seeds, masks, xT)
    log, prev = [], []
    tw = _canvas_sampler(geo, lora, seeds, masks, _crops_of_field(geo, seeds), log, prev)
    assert tw.windows == [(0, 0), (0, 12), (0, 24)] and tw.n_seeds == 3 * seeds
    got = tw.run_fusion(xT.clone())
    assert got.shape == (seeds, 4, 16, 40) and torch.equal(got, want)
    assert len(log) == len(plog) == 13 and [a[:2] for a in log] == [a[:2] for a in plog]
    for (kind, t, x), (_k, _t, px) in zip(log, plog):
        assert x.shape == (3 * seeds, 4, 16, 16) and torch.equal(x, CV.crop_windows(px, tw.windows, 16, 16)), (kind, t)
        assert _agree_on_overlaps(tw, x)
    assert len(prev) == len(pprev) == seeds
    for a, b in zip(prev, pprev):
        assert a.shape == (1, 4, 16, 40) and torch.equal(a, b)
    assert tw.masks.shape == (3 * seeds, K, 1, 16, 16)
    assert torch.equal(tw.masks[1], masks[:, :, :, 12:28].cuda())


@pytest.mark.parametrize("lora", [False, True])
def test_sampler_square_canvas_follows_the_plain_sampler(lora):
    """2 x 2 windows on 24 x 24: the corner is covered four times, and a + a + a is rounded, so the canvas run follows the plain run at resolution =
    canvas within tests/test_sampler_gpu.py's bound instead of bit for bit"""
    geo = SQUARE
    masks, xT = _inputs(geo, 2)
    want, plog, _ = _plain_run(geo, lora, 2, masks, xT)
    log, prev = [], []
    tw = _canvas_sampler(geo, lora, 2, masks, _crops_of_field(geo, 2), log, prev)
    assert tw.windows == [(0, 0), (0, 8), (8, 0), (8, 8)] and tw.n_seeds == 8
    got = tw.run_fusion(xT.clone())
    d = (got - want).abs().max().item()
    print(f"2 x 2 canvas vs plain run at canvas resolution: max abs diff {d:.3g}")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert len(log) == len(plog) and all(_agree_on_overlaps(tw, x) for _k, _t, x in log)


def _loop_restatement(geo, offs, lora, seeds, xT_windows, masks_windows, eps_of_call):
    """numpy fp32 restatement of the canvas sampler's loop: the oracle's step functions per window, then consensus_np.  -> (the state handed to every
    UNet call [S, 4, h, w], the final state)"""
    from oracle import tweedie_oracle as TO
    n, g, R, J = 10, NF(0.8), 1, 1
    sch = TO.Schedule(n)
    ts = [int(t) for t in sch.timesteps]
    ic, istop = int(n * 0.2), int(n * 0.8)
    t_cond_prev, t_cond_cur, start_t = ts[ic - 1], ts[ic], ts[0]
    t_stop_cur = ts[istop] if lora else None
    in_fusion = lambda t: (t <= t_cond_cur and t >= t_stop_cur) if lora else t <= t_cond_cur
    S = seeds * len(offs)
    handed = []
    st = {"x": xT_windows.copy(), "m": None}

    def step(mode, t, at, an, last=False):
        rows = 2 if mode == "plain_call" else K + 1
        handed.append((t, st["x"].copy()))
        eps = eps_of_call(len(handed) - 1, rows)
        out = []
        for b in range(S):
            x, e = st["x"][b:b + 1], eps[b * rows:(b + 1) * rows]
            if mode == "fusion":
                o, _ = TO.fused_fusion_step(x, e, st["m"][b], g, at, an, last)
            elif mode == "resample":
                o = TO.fused_resample_down(x, e, K, g, at, an)
            else:
                o, _ = TO.fused_plain_step(x, e[:2], g, at, an, last)
            out.append(o)
        x = np.concatenate(out).reshape(seeds, len(offs), 4, geo["h"], geo["w"])
        st["x"] = consensus_np(x, offs, geo["ch"], geo["cw"])[0].reshape(S, 4, geo["h"], geo["w"])

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
            st["x"], st["m"] = backup, masks_windows
    return handed, st["x"]


@pytest.mark.parametrize("lora,geo", [(False, WIDE), (True, WIDE), (False, SQUARE)])
def test_sampler_window_dependent_eps_follows_the_loop_restatement(lora, geo):
    """every window gets its OWN eps (what a real UNet does: a window sees only its part of the picture): the windows' steps differ on the overlaps
    and the consensus is what makes the next call's states agree there.  The state handed to every call and the final latent follow the numpy
    restatement within the per-step bound; every handed state agrees exactly across windows on every overlap; the final canvas is their assembly."""
    from tweediemix_amd import canvas as CV
    seeds = 2
    masks, xT = _inputs(geo, seeds)
    offs = CV.window_layout(geo["ch"], geo["cw"], geo["h"], geo["w"], geo["overlap"])
    S = seeds * len(offs)
    own = lambda i, rows: torch.randn(S * rows, 4, geo["h"], geo["w"], generator=torch.Generator().manual_seed(3000 + i))
    log, prev = [], []
    tw = _canvas_sampler(geo, lora, seeds, masks, lambda i, rows, _tw: own(i, rows), log, prev)
    assert tw.windows == offs
    got = tw.run_fusion(xT.clone())
    xw = CV.crop_windows(xT, offs, geo["h"], geo["w"]).numpy()
    mw = CV.crop_windows(masks.cpu().squeeze(1)[None].expand(seeds, K, geo["ch"], geo["cw"]), offs, geo["h"], geo["w"]).unsqueeze(2).numpy()
    assert np.array_equal(tw.masks.cpu().numpy(), mw)
    handed, final = _loop_restatement(geo, offs, lora, seeds, xw, mw, lambda i, rows: own(i, rows).numpy())
    assert [t for t, _x in handed] == [t for _k, t, _x in log] and len(log) == 13
    differs = False
    for (t, want), (_k, _t, x) in zip(handed, log):
        np.testing.assert_allclose(x.cpu().numpy(), want, rtol=2e-5, atol=2e-5, err_msg=f"state handed to the call at t={t}")
        assert _agree_on_overlaps(tw, x), t
    np.testing.assert_allclose(tw.x_state.cpu().numpy(), final, rtol=2e-5, atol=2e-5)
    assert _agree_on_overlaps(tw, tw.x_state) and torch.equal(got, CV.assemble(tw.x_state, offs, geo["ch"], geo["cw"]))
    assert got.shape == (seeds, 4, geo["ch"], geo["cw"]) and torch.isfinite(got).all()
    # the preview is the reconciled, assembled Tweedie estimate, one canvas per seed
    assert len(prev) == seeds and all(p.shape == (1, 4, geo["ch"], geo["cw"]) for p in prev)


# ------------------------------------------------------------------------------------------------ decode
def _decode_restatement(dec, offs, n, Hc, Wc):
    """dec [n * n_win, 3, H, W] decoded windows (CPU) -> [n, 3, Hc, Wc]: the tent blend, in the kernel's order of operations"""
    from tweediemix_amd import canvas as CV
    H, W = dec.shape[-2:]
    wt = CV.tent_weight(H, W)
    v = dec.reshape(n, len(offs), 3, H, W)
    acc, ws, cnt = torch.zeros(n, 3, Hc, Wc), torch.zeros(Hc, Wc), torch.zeros(Hc, Wc, dtype=torch.int32)
    single = torch.zeros(n, 3, Hc, Wc)
    for i, (oy, ox) in enumerate(offs):
        acc[:, :, oy:oy + H, ox:ox + W] = acc[:, :, oy:oy + H, ox:ox + W] + wt * v[:, i]
        ws[oy:oy + H, ox:ox + W] = ws[oy:oy + H, ox:ox + W] + wt
        cnt[oy:oy + H, ox:ox + W] += 1
        single[:, :, oy:oy + H, ox:ox + W] = v[:, i]
    return torch.where(cnt >= 2, acc / ws, single)


def test_canvas_decode_is_the_tent_blend_of_the_decoded_windows():
    from tweediemix_amd import canvas as CV, sampler as S, vae as V
    vae = (V.TINY, V.synthetic_state_dict(V.TINY, nontrivial=True))
    mk = lambda **kw: S.Tweediemix(_cfg(S, 16, 16), _NoWeights(), None, None, None, concept_num=K, vae=vae, **kw)
    tw = mk(n_seeds=2, canvas=dict(height=128, width=320, overlap=32))
    lat = torch.randn(2, 4, 16, 40, generator=torch.Generator().manual_seed(5)).cuda()
    img = tw.decode_final(lat)
    assert img.shape == (2, 3, 128, 320) and img.dtype == F32 and torch.isfinite(img).all()
    plain = mk()
    wins = CV.crop_windows(lat, tw.windows, 16, 16)
    dec = plain.decode_final(wins).cpu()
    assert dec.shape == (6, 3, 128, 128)
    want = _decode_restatement(dec, [(8 * oy, 8 * ox) for oy, ox in tw.windows], 2, 128, 320)
    assert torch.equal(img.cpu(), want)
    assert not torch.equal(dec[0][..., 96:], dec[1][..., :32])                       # (the windows do differ on their overlap: the blend has work to do)
    prev = tw.decode_latent(lat[:1])                                                 # the preview decode: one canvas, the preview's scale
    assert prev.shape == (1, 3, 128, 320)
    want_prev = _decode_restatement(plain.decode_latent(wins[:3]).cpu(), [(8 * oy, 8 * ox) for oy, ox in tw.windows], 1, 128, 320)
    assert torch.equal(prev.cpu(), want_prev)
    # a canvas of the window's size: today's decode, bit for bit
    one = mk(canvas=dict(height=128, width=128, overlap=64))
    assert one.windows is None and torch.equal(one.decode_final(wins[:2]), plain.decode_final(wins[:2]))


# ------------------------------------------------------------------------------------------------ tiny real UNet, through the CLI
def _cli():
    spec = importlib.util.spec_from_file_location("fs_canvas_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def _common(tmp_path):
    return ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--guidance_scale", "0.8",
            "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "1", "--resolution_h", "128", "--resolution_w", "128",
            "--output_path", str(tmp_path)]


CANVAS = ["--canvas_w", "320", "--window_overlap", "32"]


@pytest.fixture(scope="module")
def canvas_runs(tmp_path_factory):
    """the canvas runs several tests look at, made once: seed 5 with graphs, seed 5 without, seed 6 with graphs"""
    mp = pytest.MonkeyPatch()
    mp.setenv("TMIX_FORCE_TILE", "1")
    tmp = tmp_path_factory.mktemp("canvas_cli")
    fs = _cli()
    out = {"tmp": tmp}
    try:
        out["g5"] = fs.main(_common(tmp) + CANVAS + ["--seed", "5", "--output_path_all", str(tmp / "g5")]).cpu()
        out["e5"] = fs.main(_common(tmp) + CANVAS + ["--seed", "5", "--no_graphs", "--output_path_all", str(tmp / "e5")]).cpu()
        out["g6"] = fs.main(_common(tmp) + CANVAS + ["--seed", "6", "--output_path_all", str(tmp / "g6")]).cpu()
    finally:
        mp.undo()
    return out


def test_cli_canvas_graphs_equal_eager_and_files_are_canvas_sized(canvas_runs):
    from PIL import Image
    g5, e5, tmp = canvas_runs["g5"], canvas_runs["e5"], canvas_runs["tmp"]
    assert g5.shape == (1, 4, 16, 40) and torch.isfinite(g5).all()
    assert torch.equal(g5, e5)                                                           # graph replay == eager execution, bit for bit
    assert not torch.equal(g5, canvas_runs["g6"])
    saved = torch.load(tmp / "g5" / "p_5.latent.pt")
    assert saved.shape == (1, 4, 16, 40) and torch.equal(saved, g5)
    assert Image.open(tmp / "g5" / "p_5.png").size == (320, 128)                         # PIL: (width, height)
    assert sorted(os.listdir(tmp / "g5")) == ["p_5.latent.pt", "p_5.png"]


def test_cli_two_seeds_share_the_launches_of_six_row_sets(canvas_runs, monkeypatch):
    """--num_seeds 2 with three windows: 6 co-batched row sets (the default seeds per batch: 8 // 3 = 2), each seed bit for bit its single run"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    tmp = canvas_runs["tmp"]
    both = _cli().main(_common(tmp) + CANVAS + ["--seed", "5", "--num_seeds", "2", "--output_path_all", str(tmp / "two")]).cpu()
    assert both.shape == (2, 4, 16, 40)
    for i, single in enumerate((canvas_runs["g5"], canvas_runs["g6"])):
        d = (both[i:i + 1] - single).abs().max().item()
        print(f"seed {5 + i}: co-batched canvas vs single run, max abs diff {d:.3g}")
        assert torch.equal(both[i:i + 1], single), (i, d)
    assert torch.equal(torch.load(tmp / "two" / "p_6.latent.pt"), canvas_runs["g6"])


def test_cli_canvas_of_the_window_size_is_the_run_without_the_flags(tmp_path, monkeypatch):
    """--canvas_w 128 on 128-pixel windows: one window -- bit for bit today's run, no tmix_window_consensus, the identical list of library calls"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import lib as L
    lib = L.load()
    calls = []
    for name in L.SIGNATURES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    fs = _cli()
    common = _common(tmp_path) + ["--seed", "5", "--no_graphs"]
    plain = fs.main(common + ["--output_path_all", str(tmp_path / "plain")]).cpu()
    n_plain, calls[:] = list(calls), []
    one = fs.main(common + ["--canvas_w", "128", "--canvas_h", "128", "--window_overlap", "32", "--output_path_all", str(tmp_path / "one")]).cpu()
    n_one, calls[:] = list(calls), []
    assert plain.shape == (1, 4, 16, 16) and torch.equal(one, plain)
    launches = lambda names: [n for n in names if n not in ("tmix_last_error_string", "tmix_version")]
    assert launches(n_one) == launches(n_plain) and len(launches(n_plain)) > 13 * 50
    assert "tmix_window_consensus" not in n_one and n_plain.count("tmix_fused_tweedie_step_dev") == 13
    # ... and a real canvas issues one consensus launch behind every fused step, plus one for the preview and one for the pixel-space blend
    fs.main(common + CANVAS + ["--output_path_all", str(tmp_path / "wide")])
    assert calls.count("tmix_fused_tweedie_step_dev") == 13 and calls.count("tmix_window_consensus") == 13 + 1 + 1
    i = [k for k, n in enumerate(calls) if n == "tmix_fused_tweedie_step_dev"]
    assert all(calls[k + 1] == "tmix_window_consensus" for k in i)
