"""GPU: free-form attention masks -- tmix_mask_label, tmix_attn_shapes, masks.attention_masks(shape="free"), Tweediemix(attention_masks=
dict(shape="free")).

The yardstick is the numpy restatement of DESIGN.md 7h (masks.mask_label_reference / attn_shapes_reference: a flood fill per component, tied
to scipy.ndimage in tests/test_attn_shapes_cpu.py).  Everything here is integer work on a grid: kernels are compared with the restatement by
equality, never by a tolerance."""
import functools

import numpy as np
import pytest
import torch

from attn_shape_cases import KINDS, THRESHOLD, equal_score_case, label_case, shapes_case
from layout_frames import _wrap, dense_guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 7), (3, 16, 16), (2, 33, 65), (1, 64, 64), (2, 128, 128), (1, 8, 2048)]
GRIDS = [(5, 7), (33, 65), (64, 64), (128, 128)]


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ tmix_mask_label
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_equal_restatement_inside_guard_bands(shape):
    """every mask kind at this shape, set and clear pixels: the labels equal the restatement, every element is written, the sentinel around
    them survives, the map is not written, a second call gives the same; and all kinds in ONE launch (12 n maps, kinds interleaved in
    another order: other workgroups, another grid) give the same labels"""
    from tweediemix_amd import lib as L, ops
    lib = L.load()
    n, h, w = shape
    for invert in (0, 1):
        per_kind = {}
        for kind in KINDS:
            maps, want = label_case(shape, kind, invert)
            m = torch.from_numpy(maps.copy()).cuda()
            keep = m.clone()
            f = dense_guarded((n, h * w), torch.int32, rows=8, device="cuda", name=f"label[{kind}]")
            assert lib.tmix_mask_label(m.data_ptr(), 0.5, invert, f.view.data_ptr(), n, h, w, _st()) == 0
            torch.cuda.synchronize()
            f.assert_untouched()
            f.assert_all_written()
            assert torch.equal(m, keep)
            got = f.view.cpu().numpy().reshape(n, h, w)
            assert np.array_equal(got, want), (shape, kind, invert)
            again = ops.mask_label(m, 0.5, bool(invert))
            assert again.dtype == torch.int32 and np.array_equal(again.cpu().numpy(), got), (shape, kind, invert)
            per_kind[kind] = got
        if invert == 0:
            assert (per_kind["empty"] == -1).all() and (per_kind["full"] == 0).all()
            idx = np.arange(h * w).reshape(h, w)
            assert all(np.array_equal(lab[lab >= 0], idx[lab >= 0]) for lab in per_kind["checker"])      # every set pixel its own component
            assert all(len(np.unique(lab[lab >= 0])) == 1 for lab in per_kind["serpentine"])              # one component, however long the path
        order = [(kind, i) for i in range(n) for kind in reversed(KINDS)]
        allm = torch.from_numpy(np.stack([label_case(shape, kind, invert)[0][i] for kind, i in order])).cuda()
        lab = ops.mask_label(allm, 0.5, bool(invert)).cpu().numpy()
        for j, (kind, i) in enumerate(order):
            assert np.array_equal(lab[j], per_kind[kind][i]), (shape, kind, i, invert)


def test_label_threshold_is_compared_in_fp32():
    from tweediemix_amd import masks as M, ops
    vals = np.array([[0.1, np.nextafter(NF(0.1), NF(0)), np.nextafter(NF(0.1), NF(1)), 0.0, -0.0, np.nan, np.inf, -np.inf]], NF)
    for thr in (0.1, 0.0, -1.0):                          # the fp64 0.1 is rounded to fp32 on the way in, like the restatement's
        got = ops.mask_label(torch.from_numpy(vals[None]).cuda(), thr).cpu().numpy()
        assert np.array_equal(got, M.mask_label_reference(vals[None], thr)), thr


# ------------------------------------------------------------------------------------------------ tmix_attn_shapes
@pytest.mark.parametrize("n_sets", [1, 2])
@pytest.mark.parametrize("km1", [1, 2, 3])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_shapes_equal_restatement(grid, km1, n_sets):
    """mask kinds times smooth random fields, all four flag combinations, by equality inside guard bands; with RESOLVE the shapes of a set are
    pairwise disjoint, without FILL_HOLES every shape is one component of its thresholded score"""
    from tweediemix_amd import lib as L, ops
    h, w = grid
    seen_overlap = seen_hole = False
    for fill in (False, True):
        for resolve in (False, True):
            score, want = shapes_case(h, w, km1, fill, resolve)
            score, want = score[:n_sets], want[:n_sets]
            s = torch.from_numpy(score.copy()).cuda()
            keep = s.clone()
            f = dense_guarded((n_sets * km1, h * w), F32, rows=8, device="cuda", name="shapes")
            got = ops.attn_shapes(s, THRESHOLD, fill, resolve, out=f.view.view(n_sets, km1, h, w))
            torch.cuda.synchronize()
            f.assert_untouched()
            f.assert_all_written()
            assert torch.equal(s, keep)
            got = got.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (grid, km1, n_sets, fill, resolve)
            assert set(np.unique(got)) <= {0.0, 1.0}
            if resolve:
                assert got.sum(1).max() <= 1
            else:
                seen_overlap |= bool(got.sum(1).max() > 1)
            if not fill and not resolve:
                assert (got <= (score >= NF(THRESHOLD))).all()
                seen_hole |= not np.array_equal(got, shapes_case(h, w, km1, True, False)[1][:n_sets])
    assert seen_hole and (seen_overlap or km1 == 1)                # the cases are what they say: set 0 has holes to fill and overlaps to resolve
    assert L.SHAPE_FILL_HOLES == 1 and L.SHAPE_RESOLVE == 2


@pytest.mark.parametrize("grid", [(33, 65), (128, 128)], ids=lambda g: "x".join(map(str, g)))
def test_exactly_equal_scores_on_the_overlap_go_to_the_smallest_k(grid):
    from tweediemix_amd import masks as M, ops
    score = equal_score_case(*grid)
    raw = M.attn_shapes_reference(score, THRESHOLD, True, False)
    claimed = raw[0] != 0
    ties = (claimed[0] & claimed[1] & (score[0, 0] == score[0, 1])) | (claimed[1] & claimed[2] & (score[0, 1] == score[0, 2]))
    assert ties.sum() > grid[0] * grid[1] // 8                     # the case is what it says: many pixels with exactly equal scores
    want = M.attn_shapes_reference(score, THRESHOLD, True, True)
    got = ops.attn_shapes(torch.from_numpy(score.copy()).cuda(), THRESHOLD, True, True).cpu().numpy()
    assert np.array_equal(got, want) and got.sum(1).max() <= 1
    both = claimed[0] & claimed[1] & (score[0, 0] == score[0, 1]) & ~(claimed[2] & (score[0, 2] > score[0, 0]))
    assert both.any() and (got[0, 0][both] == 1).all() and (got[0, 1][both] == 0).all()


def test_captured_graph_replay_equals_eager_call():
    from tweediemix_amd import ops
    maps, lab = label_case((2, 33, 65), "rings", 0)
    score, want = shapes_case(128, 128, 3, True, True)             # above 64 KB of LDS: the limit is raised by the warm-up call below
    m, s = torch.from_numpy(maps.copy()).cuda(), torch.from_numpy(score.copy()).cuda()
    a = ops.mask_label(m, 0.5)                                     # warm-up outside capture (lazy module load, LDS limit)
    b = ops.attn_shapes(s, THRESHOLD, True, True)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), lab) and np.array_equal(b.cpu().numpy(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_label(m, 0.5, out=a)
        ops.attn_shapes(s, THRESHOLD, True, True, out=b)
    a.fill_(-7)
    b.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), lab) and np.array_equal(b.cpu().numpy(), want)


def test_error_codes_without_a_launch():
    from tweediemix_amd import lib as L
    lib = L.load()
    h, w = 5, 7
    m = torch.zeros(2, h, w, device="cuda")
    f_lab = dense_guarded((2, h * w), torch.int32, rows=8, device="cuda", name="label")
    f_out = dense_guarded((2, h * w), F32, rows=8, device="cuda", name="shapes")
    pm, pl, po = m.data_ptr(), f_lab.view.data_ptr(), f_out.view.data_ptr()
    label = lambda a=pm, o=pl, thr=0.5, n=2, h_=h, w_=w: lib.tmix_mask_label(a, thr, 0, o, n, h_, w_, _st())
    shapes = lambda a=pm, o=po, ns=1, k=2, h_=h, w_=w, thr=0.5, fl=3: lib.tmix_attn_shapes(a, o, ns, k, h_, w_, thr, fl, _st())
    assert label(a=None) == L.EINVAL and label(o=None) == L.EINVAL and label(thr=float("nan")) == L.EINVAL
    assert label(h_=129, w_=128) == L.ESHAPE and label(n=0) == L.ESHAPE and label(n=65536) == L.ESHAPE and label(w_=0) == L.ESHAPE
    assert shapes(a=None) == L.EINVAL and shapes(o=None) == L.EINVAL and shapes(thr=float("inf")) == L.EINVAL and shapes(fl=8) == L.EINVAL
    assert shapes(h_=1, w_=16385) == L.ESHAPE and shapes(k=0) == L.ESHAPE and shapes(ns=0) == L.ESHAPE and shapes(ns=300, k=300) == L.ESHAPE
    torch.cuda.synchronize()
    for f in (f_lab, f_out):                                       # nothing was launched: the views still hold the sentinel everywhere
        assert bool((f.bits == _wrap(f.sentinel, f.bits.dtype)).all()), f.name


# ------------------------------------------------------------------------------------------------ planted localisation
def test_planted_localisation_gives_the_outlines():
    """Q and K built so that token 4 wins inside a disc with an off-centre hole and token 7 inside an L-shape that reaches into the disc's
    bounding box but not into the disc, on a 32 x 32 grid.  shape="free" (the kernels) returns the disc with its hole filled and the L;
    shape="rect" returns the two boxes, whose overlap expand_masks had to cut"""
    from tweediemix_amd import masks as M, ops
    gh = gw = 32
    H, Lk, tok = 4, 77, [4, 7]
    yy, xx = np.mgrid[0:gh, 0:gw]
    disc = (yy - 11) ** 2 + (xx - 11) ** 2 <= 64                   # box [3, 20) x [3, 20)
    holed = disc.copy()
    holed[8:10, 13:15] = False                                     # off-centre, 2 x 2
    ell = np.zeros((gh, gw), bool)
    ell[17:30, 17:21] = True                                       # the bar starts inside the disc's box (rows 17..19, columns 17..19) ...
    ell[27:30, 17:29] = True                                       # ... the foot lies outside it
    assert not (disc & ell).any() and ell[17:20, 17:20].all()
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, gh * gw, H * 64, generator=g) * 0.1
    k = torch.randn(2, 80, H * 64, generator=g) * 0.1
    for j, (t, sel) in enumerate(zip(tok, (holed, ell))):
        k[1, t, [h * 64 + j for h in range(H)]] = 6.0
        for h in range(H):
            q[1, torch.from_numpy(sel.flatten()), h * 64 + j] = 6.0
    maps = ops.xattn_token_maps(q.to(torch.bfloat16).cuda(), k.to(torch.bfloat16).cuda(), tok, H, Lk=Lk, rows=(1, 1, 1))
    per = {2: maps[0].cpu().numpy().reshape(2, gh, gw)}
    as_t = lambda m: torch.from_numpy(m.astype(NF))
    free = M.build_masks(M.attention_masks(per, [[0], [1]], gh * 8, gw * 8, shape="free", device="cuda"), gh, gw, "cpu")
    assert torch.equal(free[0, 0], as_t(disc)) and torch.equal(free[1, 0], as_t(ell))
    assert torch.equal(free[2, 0], 1 - free[0, 0] - free[1, 0])
    kept = M.build_masks(M.attention_masks(per, [[0], [1]], gh * 8, gw * 8, shape="free", fill_holes=False, device="cuda"), gh, gw, "cpu")
    assert torch.equal(kept[0, 0], as_t(holed)) and torch.equal(kept[1, 0], as_t(ell))
    host = M.build_masks(M.attention_masks(per, [[0], [1]], gh * 8, gw * 8, shape="free"), gh, gw, "cpu")       # the restatement's path
    assert torch.equal(host, free)
    rect = M.build_masks(M.attention_masks(per, [[0], [1]], gh * 8, gw * 8, shape="rect", device="cuda"), gh, gw, "cpu")
    want = M.expand_masks([holed, ell])
    assert torch.equal(rect[0, 0], as_t(want[0])) and torch.equal(rect[1, 0], as_t(want[1]))
    box0, box1 = np.zeros((gh, gw), bool), np.zeros((gh, gw), bool)
    box0[3:20, 3:20] = True
    box1[17:30, 17:29] = True
    ov = box0 & box1
    assert np.array_equal(want[0] & ~ov, box0 & ~ov) and np.array_equal(want[1] & ~ov, box1 & ~ov)      # the two boxes ...
    assert not want[0][ov].any() and want[1][ov].all()              # ... and their overlap refilled with the original masks: the L's corner
    assert rect[0, 0].sum() > free[0, 0].sum() and rect[1, 0].sum() > free[1, 0].sum()                    # the boxes claim background


# ------------------------------------------------------------------------------------------------ sampler (tiny UNet)
K, HL, WL = 3, 16, 16
TOKENS = [[4], [7, 9]]
IDX = [[0], [1, 2]]


@functools.lru_cache(maxsize=None)
def _tiny():
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, "custom", K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g).to(torch.bfloat16).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", ("custom", con)), te, ts


def _cfg(S):
    return S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=2,
                         resolution_h=HL * 8, resolution_w=WL * 8)


def _no_provider(x0):
    raise AssertionError("the mask provider must not be called with attention_masks")


def _run(am, xT, **kw):
    from tweediemix_amd import sampler as S
    W, te, ts = _tiny()
    tw = S.Tweediemix(_cfg(S), W, te, ts, _no_provider, concept_num=K, attention_masks=am, **kw)
    lat = tw.run_fusion(xT.clone()).cpu()
    return lat, tw.masks.clone().cpu(), tw


def _xT():
    return torch.randn(2, 4, HL, WL, generator=torch.Generator().manual_seed(7))


def test_sampler_free_masks(monkeypatch):
    """masks in {0, 1}, disjoint foregrounds, the background rule; the kernel path through the whole plumbing equals the restatement path on
    the run's own maps; a second run is bit-identical; the same masks through a fixed provider give the identical latent; co-batched seeds
    get the masks of their single runs"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import masks as M, sampler as S
    am = dict(tokens=TOKENS, threshold=0.5, shape="free")
    xT = _xT()
    singles = [_run(am, xT[i:i + 1]) for i in range(2)]
    lat, ms, tw = singles[0]
    assert ms.shape == (K, 1, HL, WL) and set(torch.unique(ms).tolist()) <= {0.0, 1.0}
    assert (ms[0] + ms[1]).sum() > 0                  # (a score reaches 1 somewhere, and a claimed pixel stays with one of the concepts)
    assert float((ms[0] * ms[1]).sum()) == 0.0                                        # disjoint
    assert torch.equal(ms[K - 1], 1 - ms[0] - ms[1]) and torch.equal(ms.sum(0), torch.ones(1, HL, WL))
    for _lat, m_i, tw_i in singles:                                                  # kernel path == restatement path
        host = M.attention_masks(tw_i.attention_maps[0], IDX, HL * 8, WL * 8, 0.5, None, shape="free", device=None)
        assert all(np.array_equal(a, b) for a, b in zip(tw_i.mask_images[0], host))
        assert torch.equal(m_i, M.build_masks(host, HL, WL, "cpu"))
    lat2, ms2, _tw = _run(am, xT[0:1])
    assert torch.equal(lat2, lat) and torch.equal(ms2, ms)
    W, te, ts = _tiny()
    fixed = S.Tweediemix(_cfg(S), W, te, ts, lambda x0: ms.cuda(), concept_num=K)
    assert torch.equal(fixed.run_fusion(xT[0:1].clone()).cpu(), lat) and "probe" not in fixed.plans
    _both, ms_both, tw2 = _run(am, xT, n_seeds=2, use_graphs=True)
    assert ms_both.shape == (2, K, 1, HL, WL)
    for i in range(2):
        assert torch.equal(ms_both[i], singles[i][1]), i


def test_sampler_rect_key_is_the_run_without_it(monkeypatch):
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    xT = _xT()[0:1]
    lat0, ms0, tw0 = _run(dict(tokens=TOKENS, threshold=0.5), xT)
    lat1, ms1, tw1 = _run(dict(tokens=TOKENS, threshold=0.5, shape="rect", fill_holes=False), xT)
    assert torch.equal(lat1, lat0) and torch.equal(ms1, ms0)
    assert all(np.array_equal(a, b) for a, b in zip(tw0.mask_images[0], tw1.mask_images[0]))
    assert [c[0] for c in tw0.unet_calls] == [c[0] for c in tw1.unet_calls]


def test_sampler_free_masks_softened(monkeypatch):
    """shape="free" with mask_soften: the weights are soft_masks_reference of the free masks (real outlines under the feather)"""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import masks as M
    xT = _xT()[0:1]
    _lat, ws, tw = _run(dict(tokens=TOKENS, threshold=0.5, shape="free"), xT, mask_soften=dict(feather=2, normalize=True))
    free = M.build_masks(tw.mask_images[0], HL, WL, "cpu")
    host = M.attention_masks(tw.attention_maps[0], IDX, HL * 8, WL * 8, 0.5, None, shape="free")
    assert torch.equal(free, M.build_masks(host, HL, WL, "cpu"))
    want = M.soft_masks_reference(free[:-1, 0].numpy(), 2, 0.0, True)
    assert ws.shape == (K, 1, HL, WL) and np.array_equal(ws.numpy(), want) and torch.equal(tw.soft_weights.cpu(), ws)
    assert bool(((ws > 0) & (ws < 1)).any())
