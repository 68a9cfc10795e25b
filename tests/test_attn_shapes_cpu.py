"""CPU: free-form attention masks -- the numpy restatements masks.mask_label_reference / attn_shapes_reference against
scipy.ndimage and against hand-built cases of every rule, masks.attention_masks(shape=...), the argument checks of tmix_mask_label and
tmix_attn_shapes (the library loads without a GPU), the sampler option's validation and the CLI refusals."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from attn_shape_cases import KINDS, mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = np.float32
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


# ------------------------------------------------------------------------------------------------ restatement vs scipy.ndimage
@pytest.mark.parametrize("h,w", [(16, 16), (33, 65)])
def test_restatement_equals_scipy_ndimage(h, w):
    """labels: ndimage.label with the cross element, every label mapped to its component's smallest raster index; hole filling:
    binary_fill_holes with the same element (so the background is 4-connected too), on the largest component of every mask kind"""
    ndi = pytest.importorskip("scipy.ndimage")
    from tweediemix_amd import masks as M
    for kind in KINDS:
        for i in range(2):
            m = mask(kind, i, h, w)
            for invert in (False, True):
                sel = (m >= NF(0.5)) != invert
                lab, n = ndi.label(sel, structure=CROSS)
                idx = np.arange(h * w).reshape(h, w)
                first = np.full(n + 1, -1, np.int64)
                if n:
                    first[1:] = ndi.minimum(idx, lab, np.arange(1, n + 1))
                got = M.mask_label_reference(m, 0.5, invert)
                assert got.dtype == np.int32 and np.array_equal(got, first[lab]), (kind, i, invert)
            c = M.largest_component(m >= NF(0.5))
            want = ndi.binary_fill_holes(c, structure=CROSS)
            got = M.attn_shapes_reference(m[None], 0.5, True, False)[0] != 0
            assert np.array_equal(got, want), (kind, i)
            assert np.array_equal(M.attn_shapes_reference(m[None], 0.5, False, False)[0] != 0, c), (kind, i)


# ------------------------------------------------------------------------------------------------ the rules, one by one
def test_label_reference_shapes_and_threshold_in_fp32():
    from tweediemix_amd import masks as M
    m = np.array([[1, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 1]], NF)
    assert np.array_equal(M.mask_label_reference(m), [[0, -1, 2, 2], [0, -1, -1, 2], [-1, 9, -1, 2]])
    assert np.array_equal(M.mask_label_reference(m, invert=True), [[-1, 1, -1, -1], [-1, 1, 1, -1], [8, -1, 1, -1]])
    assert M.mask_label_reference(np.stack([m, 1 - m])[None]).shape == (1, 2, 3, 4)
    # the comparison is the kernel's: fp32(map) >= fp32(threshold).  0.1 (fp64) is below fp32(0.1), which rounds up
    assert np.float64(0.1) < np.float64(NF(0.1))
    assert M.mask_label_reference(np.array([[0.1]], np.float64), NF(0.1))[0, 0] == 0


def test_tie_rule_the_component_reached_first_wins():
    from tweediemix_amd import masks as M
    m = np.zeros((6, 9), NF)
    m[4:6, 0:3] = 1                                  # six pixels, first pixel at raster index 36
    m[0:3, 6:8] = 1                                  # six pixels, first pixel at raster index 6: the smaller label
    got = M.attn_shapes_reference(m[None], 0.5, False, False)[0]
    assert got[0:3, 6:8].all() and got.sum() == 6
    m[5, 3] = 1                                      # seven pixels now: the larger area beats the smaller label
    got = M.attn_shapes_reference(m[None], 0.5, False, False)[0]
    assert got[4:6, 0:3].all() and got[5, 3] == 1 and got.sum() == 7
    assert M.attn_shapes_reference(np.zeros((1, 4, 5), NF), 0.5).sum() == 0              # an empty map stays empty


def test_hole_rules():
    from tweediemix_amd import masks as M
    shapes = lambda m, fill=True: M.attn_shapes_reference(np.asarray(m, NF)[None], 0.5, fill, False)[0]
    ring = np.zeros((7, 7), NF)
    ring[1:6, 1:6] = 1
    ring[2:5, 2:5] = 0
    assert shapes(ring).sum() == 25 and shapes(ring, False).sum() == 16                   # the 3 x 3 hole is filled
    bay = ring.copy()
    bay[0:2, 3] = 0                                   # the hole now reaches row 0 through a channel: it touches the border
    assert np.array_equal(shapes(bay), bay)
    edge = np.zeros((5, 5), NF)
    edge[0:3, 0:3] = 1
    edge[1, 0] = 0                                    # a clear pixel ON the border column, enclosed on its other three sides
    assert np.array_equal(shapes(edge), edge)
    # a ring of SET pixels closed only diagonally is not one component: 4-connected for set pixels ...
    diamond = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], NF)
    assert shapes(diamond).sum() == 1
    # ... and for clear pixels: a ring with one corner cut out is still one component (the other way round) and still encloses its centre,
    # which touches the outside only through the diagonal (2,2)-(1,1)
    cut = ring.copy()
    cut[1, 1] = 0
    assert shapes(cut, False).sum() == 15 and shapes(cut).sum() == 24 and shapes(cut)[2:5, 2:5].all() and shapes(cut)[1, 1] == 0
    # a discarded smaller blob inside the hole is filled with it: the complement is of c_k, not of b_k
    dot = np.zeros((9, 9), NF)
    dot[1:8, 1:8] = 1
    dot[2:7, 2:7] = 0
    dot[4, 4] = 1
    assert shapes(dot, False).sum() == 24 and shapes(dot, False)[4, 4] == 0 and shapes(dot).sum() == 49


def test_overlap_rule_with_equal_scores():
    from tweediemix_amd import masks as M
    s = np.zeros((3, 4, 6), NF)
    s[0, :, 0:4] = 0.75
    s[1, :, 2:6] = 0.75                              # equal to concept 0 on columns 2..3: the smaller k keeps them
    s[2, 1:3, 1:5] = 1.0                             # higher than both where it lies
    s[1, 0, 2] = 0.875                               # one pixel where concept 1 is strictly higher
    got = M.attn_shapes_reference(s, 0.5, True, True)
    assert got.shape == (3, 4, 6) and got.sum(0).max() == 1
    assert got[2, 1:3, 1:5].all() and got[2].sum() == 8
    assert got[0, 0, 0:2].all() and got[0, 0, 3] == 1 and got[0, 0, 2] == 0 and got[1, 0, 2] == 1
    assert got[0, 3, 0:4].all() and not got[1, 3, 0:4].any() and got[1, 3, 4:6].all()
    raw = M.attn_shapes_reference(s, 0.5, True, False)
    assert raw.sum(0).max() == 3                                                          # without RESOLVE the shapes come back as they are
    # a shape that the resolution cuts in two stays cut: nothing is re-labelled
    t = np.zeros((2, 3, 7), NF)
    t[0, 1, :] = 0.75
    t[1, :, 3] = 1.0
    cut = M.attn_shapes_reference(t, 0.5, True, True)
    assert cut[0, 1, 0:3].all() and cut[0, 1, 4:7].all() and cut[0, 1, 3] == 0 and cut[1, :, 3].all()
    both = M.attn_shapes_reference(np.stack([s[:2], s[1:]]), 0.5, True, True)               # [n_sets, K-1, h, w]: every set on its own
    assert both.shape == (2, 2, 4, 6) and np.array_equal(both[0], M.attn_shapes_reference(s[:2], 0.5, True, True))


# ------------------------------------------------------------------------------------------------ masks.attention_masks
def _blob(h, w, y0, y1, x0, x1, peak=1.0):
    """a smooth bump whose support is exactly [y0, y1) x [x0, x1)"""
    m = np.zeros((h, w))
    yy, xx = np.mgrid[y0:y1, x0:x1]
    cy, cx = (y0 + y1 - 1) / 2, (x0 + x1 - 1) / 2
    m[y0:y1, x0:x1] = peak * (1.2 - ((yy - cy) / (y1 - y0)) ** 2 - ((xx - cx) / (x1 - x0)) ** 2)
    return m


def _rect_cases():
    """(maps_per_level, tokens, H, W, kwargs): the inputs the rectangle path's own tests use -- blobs per concept, two levels with
    weights, overlapping discs, a sub-threshold strip, a constant map, a list instead of a dict"""
    g = 16
    blobs = np.zeros((3, g, g))
    blobs[0] = _blob(g, g, 2, 7, 3, 9)
    blobs[1] = _blob(g, g, 9, 15, 1, 6) * 3
    blobs[2] = _blob(g, g, 9, 15, 1, 6)
    coarse, fine = np.zeros((2, 4, 4)), np.zeros((2, 8, 8))
    coarse[0, 0, 0] = coarse[1, 3, 3] = 1.0
    fine[0, 6:8, 6:8] = fine[1, 0:2, 0:2] = 1.0
    yy, xx = np.mgrid[0:32, 0:32]
    a = np.maximum(0, 64 - (yy - 11) ** 2 - (xx - 11) ** 2).astype(float)
    b = np.maximum(0, 64 - (yy - 20) ** 2 - (xx - 21) ** 2).astype(float)
    strip = np.zeros((1, 20, 20))
    strip[0, 2:10, 2:10] = 1.0
    strip[0, 14:17, 14:17] = 1.0
    strip[0, 2:10, 10:14] = 0.4
    return [({2: blobs}, [[0], [1, 2]], 128, 128, dict(threshold=0.05)),
            ({1: fine, 2: coarse}, [[0], [1]], 8, 8, dict(level_weights={2: 1.0})),
            ({1: fine, 2: coarse}, [[0], [1]], 8, 8, dict(level_weights={1: 1.0, 2: 0.0})),
            ([np.stack([a, b])], [[0], [1]], 32, 32, dict(threshold=1e-9)),
            ({0: strip}, [[0]], 20, 20, {}),
            ({0: strip}, [[0]], 20, 20, dict(threshold=0.3)),
            ({0: np.ones((1, 4, 4))}, [[0]], 8, 8, {})]


def test_rect_mode_is_the_call_without_the_argument(golden_dir):
    from tweediemix_amd import masks as M
    g = np.load(os.path.join(golden_dir, "expand_masks.npz"))                            # the golden SAM masks as maps, as the older test feeds them
    golden = [({0: np.stack([g[f"{case}_in0"], g[f"{case}_in1"]]).astype(np.float64)}, [[0], [1]], 96, 96, {})
              for case in ("disjoint", "overlap", "contained", "touching")]
    for maps, toks, H, W, kw in _rect_cases() + golden:
        plain = M.attention_masks(maps, toks, H, W, **kw)
        rect = M.attention_masks(maps, toks, H, W, shape="rect", fill_holes=False, device="cpu", **kw)
        assert len(plain) == len(rect) == len(toks)
        for p, r in zip(plain, rect):
            assert p.dtype == r.dtype == np.uint8 and np.array_equal(p, r)
        score = M.attention_scores(maps, toks, kw.get("level_weights"))                   # the factored-out score: fp64, normalised
        assert score.dtype == np.float64 and score.shape[0] == len(toks) and score.min() >= 0 and score.max() == 1
        want = M.expand_masks([M.largest_component(s >= kw.get("threshold", 0.5)) for s in score])
        ys, xs = (np.arange(H) * score.shape[1]) // H, (np.arange(W) * score.shape[2]) // W
        for p, r in zip(plain, want):
            assert np.array_equal(p > 0, r[ys][:, xs])
    with pytest.raises(ValueError, match="shape"):
        M.attention_masks(maps, toks, H, W, shape="round")
    with pytest.raises(ValueError):
        M.attention_scores({0: np.ones((1, 4, 4))}, [[]])


def test_planted_l_shape_with_a_hole():
    from tweediemix_amd import masks as M
    g = 12
    ell = np.zeros((g, g), bool)
    ell[2:10, 3:6] = True                            # the bar
    ell[7:10, 3:10] = True                           # the foot
    hole = (4, 4)
    score = np.where(ell, 0.9, 0.1)
    score[hole] = 0.1
    score[0, 11] = 1.0                               # a lone peak elsewhere (the maximum: fixes the normalisation), not part of the L
    score[11, 0] = 0.0
    maps = {0: score[None]}
    up = lambda m: np.kron(m, np.ones((8, 8), bool))
    free = M.attention_masks(maps, [[0]], g * 8, g * 8, shape="free")
    assert free[0].dtype == np.uint8 and set(np.unique(free[0])) == {0, 255} and np.array_equal(free[0] > 0, up(ell))
    holed = ell.copy()
    holed[hole] = False
    kept = M.attention_masks(maps, [[0]], g * 8, g * 8, shape="free", fill_holes=False)
    assert np.array_equal(kept[0] > 0, up(holed))
    assert np.array_equal(M.attention_masks(maps, [[0]], g * 8, g * 8, shape="free", device="cpu")[0], free[0])
    box = np.zeros((g, g), bool)
    box[2:10, 3:10] = True
    rect = M.attention_masks(maps, [[0]], g * 8, g * 8, shape="rect")
    assert np.array_equal(rect[0] > 0, up(box)) and np.array_equal(rect[0], M.attention_masks(maps, [[0]], g * 8, g * 8)[0])


def test_three_overlapping_blobs_free_masks_are_a_partition_rectangles_are_not():
    """K = 4: the property the free mode exists for.  Free: pairwise disjoint, build_masks sums to exactly 1 everywhere.  Rectangles of the
    same scores: expand_masks resolves two masks only, so the weights sum to 2 or more where the three boxes intersect"""
    import torch
    from tweediemix_amd import masks as M
    g = 24
    yy, xx = np.mgrid[0:g, 0:g]
    disc = lambda cy, cx, r: np.maximum(0.0, 1.0 - ((yy - cy) ** 2 + (xx - cx) ** 2) / float(r * r))
    maps = {0: np.stack([disc(9, 9, 8), disc(9, 15, 8), disc(15, 12, 8)])}
    toks = [[0], [1], [2]]
    free = M.attention_masks(maps, toks, g * 8, g * 8, threshold=0.2, shape="free")
    fg = [f > 0 for f in free]
    assert all(f.any() for f in fg)
    raw = M.attn_shapes_reference(M.attention_scores(maps, toks).astype(NF), 0.2, True, False)
    assert (raw.sum(0) >= 2).any() and (raw.sum(0) == 3).any()                            # the three blobs do overlap, all three somewhere
    for a in range(3):
        for b in range(a + 1, 3):
            assert not (fg[a] & fg[b]).any(), (a, b)
    ms = M.build_masks(free, g, g, "cpu")
    assert ms.shape == (4, 1, g, g) and torch.equal(ms.sum(0), torch.ones(1, g, g))
    rect = M.attention_masks(maps, toks, g * 8, g * 8, threshold=0.2, shape="rect")
    mr = M.build_masks(rect, g, g, "cpu")
    assert float(mr.sum(0).max()) >= 2.0


# ------------------------------------------------------------------------------------------------ the C entries without a device
def test_symbols_exported_declared_and_built():
    from tweediemix_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "tmix.h")).read()
    for name, n_args in (("tmix_mask_label", 8), ("tmix_attn_shapes", 9)):
        assert name in lib.SIGNATURES and hasattr(l, name)
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, f"tmix.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(lib.SIGNATURES[name][1]) == n_args and params[-1] == "void* stream"
    for macro, value in (("TMIX_SHAPE_FILL_HOLES", lib.SHAPE_FILL_HOLES), ("TMIX_SHAPE_RESOLVE", lib.SHAPE_RESOLVE),
                         ("TMIX_SHAPE_MAX_PIXELS", lib.SHAPE_MAX_PIXELS)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr), macro
    assert (lib.SHAPE_FILL_HOLES, lib.SHAPE_RESOLVE, lib.SHAPE_MAX_PIXELS) == (1, 2, 16384)
    assert "mask_shape.o" in open(os.path.join(ROOT, "tweediemix_amd", "csrc", "Makefile")).read()


def test_argument_errors_are_reported_before_any_launch():
    from tweediemix_amd import lib
    l = lib.load()
    a, b = C.c_void_p(0x10000), C.c_void_p(0x20000)                  # never dereferenced: validation fails first
    msg = l.tmix_last_error_string

    def label(map=a, thr=0.5, invert=0, out=b, n=2, h=5, w=7):
        return l.tmix_mask_label(map, thr, invert, out, n, h, w, None)

    def shapes(score=a, out=b, n_sets=1, km1=2, h=5, w=7, thr=0.5, flags=3):
        return l.tmix_attn_shapes(score, out, n_sets, km1, h, w, thr, flags, None)

    assert label(map=None) == lib.EINVAL and b"mask_label" in msg() and b"null" in msg()
    assert label(out=None) == lib.EINVAL
    assert label(thr=float("nan")) == lib.EINVAL and b"threshold" in msg() and b"nan" in msg().lower()
    assert label(thr=float("inf")) == lib.EINVAL and label(thr=-float("inf")) == lib.EINVAL
    assert label(h=1, w=16385) == lib.ESHAPE and b"16384" in msg()
    assert label(h=128, w=129) == lib.ESHAPE and label(h=4096, w=4096) == lib.ESHAPE
    assert label(h=0) == lib.ESHAPE and label(w=0) == lib.ESHAPE and label(w=-3) == lib.ESHAPE
    assert label(n=0) == lib.ESHAPE and label(n=65536) == lib.ESHAPE and b"n=65536" in msg()
    assert label(map=None, h=0) == lib.EINVAL                                            # pointers first, then sizes: the order of the other entries

    assert shapes(score=None) == lib.EINVAL and b"attn_shapes" in msg() and b"null" in msg()
    assert shapes(out=None) == lib.EINVAL
    assert shapes(thr=float("nan")) == lib.EINVAL and b"threshold" in msg()
    assert shapes(thr=float("inf")) == lib.EINVAL
    assert shapes(flags=4) == lib.EINVAL and b"flags=0x4" in msg()
    assert shapes(flags=-1) == lib.EINVAL and shapes(flags=7) == lib.EINVAL
    assert shapes(h=127, w=130) == lib.ESHAPE and b"16384" in msg()                       # 16510 pixels
    assert shapes(h=16385, w=1) == lib.ESHAPE
    assert shapes(km1=0) == lib.ESHAPE and b"km1=0" in msg()
    assert shapes(n_sets=0) == lib.ESHAPE and shapes(h=0) == lib.ESHAPE and shapes(w=0) == lib.ESHAPE
    assert shapes(n_sets=256, km1=256) == lib.ESHAPE and shapes(n_sets=70000, km1=70000) == lib.ESHAPE
    assert shapes(flags=4, km1=0) == lib.EINVAL


def test_ops_refuse_cpu_tensors():
    import torch
    from tweediemix_amd import lib, ops
    with pytest.raises(lib.TmixError):
        ops.mask_label(torch.zeros(1, 4, 4))
    with pytest.raises(lib.TmixError):
        ops.attn_shapes(torch.zeros(1, 2, 4, 4), 0.5)


# ------------------------------------------------------------------------------------------------ sampler option and CLI
def test_sampler_option_validation_and_the_host_path():
    """a bad shape is refused; the defaults are the rectangle; on a CPU device the free masks come from the restatement"""
    import torch
    from types import SimpleNamespace
    from tweediemix_amd import masks as M, sampler as S
    K, h, w = 3, 16, 16
    W = SimpleNamespace(device=torch.device("cpu"), kind="custom")
    cfg = S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, resampling_steps=1, jumping_steps=2,
                        resolution_h=h * 8, resolution_w=w * 8)
    for bad in ("round", "", None, 1, "Free"):
        with pytest.raises(ValueError, match="shape"):
            S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]], shape=bad))
    tw = S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]]))
    assert tw.attention_masks["shape"] == "rect" and tw.attention_masks["fill_holes"] is True
    tw = S.Tweediemix(cfg, W, None, None, None, concept_num=K, attention_masks=dict(tokens=[[4], [7]], shape="free", fill_holes=False))
    assert tw.attention_masks["shape"] == "free" and tw.attention_masks["fill_holes"] is False
    maps = torch.zeros(1, 2, 64)
    ring = torch.zeros(8, 8)
    ring[1:6, 1:6] = 1
    ring[2:5, 2:5] = 0
    diag = torch.eye(8).flip(0)                       # a diagonal: eight components of one pixel, the first one wins
    maps[0, 0], maps[0, 1] = ring.flatten(), diag.flatten()
    tw.plans["probe"] = SimpleNamespace(token_maps={1: maps}, B=2)
    got = tw._masks_from_attention()
    assert got.shape == (K, 1, h, w)
    first = torch.zeros(8, 8)
    first[0, 7] = 1                                   # (outside the ring: nothing for the overlap rule to do)
    up = lambda m: m.repeat_interleave(2, 0).repeat_interleave(2, 1)
    assert torch.equal(got[0, 0], up(ring)) and torch.equal(got[1, 0], up(first))         # fill_holes=False: the ring keeps its hole
    assert torch.equal(got[2, 0], 1 - up(ring) - up(first))
    tw.attention_masks["fill_holes"] = True
    filled = torch.zeros(8, 8)
    filled[1:6, 1:6] = 1
    assert torch.equal(tw._masks_from_attention()[0, 0], up(filled))
    imgs = M.attention_masks({1: maps[0].reshape(2, 8, 8).numpy()}, [[0], [1]], h * 8, w * 8, shape="free")
    assert all(np.array_equal(a, b) for a, b in zip(tw.mask_images[0], imgs))


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_shape", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def test_cli_flags_and_refusals_before_the_gpu():
    fs = _cli()
    opt = fs.build_parser().parse_args([])
    assert opt.attn_mask_shape == "rect" and opt.attn_mask_keep_holes is False
    fs.check_shape_args(opt)                                                              # the defaults never refuse
    with pytest.raises(SystemExit):
        fs.build_parser().parse_args(["--attn_mask_shape", "round"])
    base = ["--tiny", "--synthetic", "--mask_token_ids", "4+7", "--seg_concepts", "a cat+a dog"]
    with pytest.raises(SystemExit, match="mask_source attention"):
        fs.main(base + ["--attn_mask_shape", "free"])
    with pytest.raises(SystemExit, match="mask_source attention"):
        fs.main(base + ["--attn_mask_keep_holes"])
    with pytest.raises(SystemExit, match="attn_mask_shape free"):
        fs.main(base + ["--mask_source", "attention", "--attn_mask_keep_holes"])
    with pytest.raises(SystemExit, match="attn_mask_shape free"):
        fs.main(base + ["--mask_source", "attention", "--attn_mask_shape", "rect", "--attn_mask_keep_holes"])
    fs.check_shape_args(fs.build_parser().parse_args(["--mask_source", "attention", "--attn_mask_shape", "free", "--attn_mask_keep_holes"]))
    fs.check_shape_args(fs.build_parser().parse_args(["--mask_source", "attention", "--attn_mask_shape", "free"]))
    fs.LORA = True                                    # fusion_sampling_lora.py is this module with LORA switched on: the same parser
    opt = fs.build_parser().parse_args(["--mask_source", "attention", "--attn_mask_shape", "free", "--t_stop", "0.8"])
    assert opt.attn_mask_shape == "free"
    with pytest.raises(SystemExit, match="mask_source attention"):
        fs.main(["--tiny", "--synthetic", "--attn_mask_shape", "free"])
