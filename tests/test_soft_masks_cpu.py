"""CPU: soft region masks -- the numpy restatement (masks.soft_masks_reference, the yardstick of tests/test_soft_masks_gpu.py) has the
properties DESIGN.md 7g claims for the definition, its separable distances equal brute force, and the CLI parses / refuses the new flags
before anything touches a GPU."""
import importlib.util
import os

import numpy as np
import pytest

NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((1, 1), (1, 7), (5, 7), (16, 16), (33, 65), (64, 64))
DENSITIES = (0.0, 1.0, 0.5, 0.02)


def _mask(h, w, density, seed=0):
    return (np.random.RandomState(seed + 31 * h + w).rand(h, w) < density).astype(NF)


def _overlapping(K=4, h=16, w=16, seed=4):
    """[K-1, h, w] {0, 1}: the seeded rectangles of random_rectangle_masks on the latent grid; seed 4 has pixels that all three cover"""
    from tweediemix_amd import masks as M
    return np.stack([M.preprocess_mask(m, h, w, "cpu").numpy()[0, 0] for m in M.random_rectangle_masks(K, h * 8, w * 8, seed=seed)])


@pytest.mark.parametrize("h,w", GRIDS)
def test_separable_distances_equal_brute_force(h, w):
    from tweediemix_amd import masks as M
    for dens in DENSITIES:
        b = _mask(h, w, dens)[None]
        bs, bc = M.mask_edt_reference(b, brute=True)
        ss, sc = M.mask_edt_reference(b, brute=False)
        assert bs.dtype == np.int32 and np.array_equal(bs, ss) and np.array_equal(bc, sc), (h, w, dens)
        assert ((bs == 0) == (b >= 0.5)).all() and ((bc == 0) == (b < 0.5)).all()
        if dens == 0.0:
            assert (bs == M.EDT_NONE).all() and (bc == 0).all()
        if dens == 1.0:
            assert (bc == M.EDT_NONE).all() and (bs == 0).all()


def test_distances_of_a_known_mask():
    from tweediemix_amd import masks as M
    b = np.zeros((1, 4, 5), NF)
    b[0, 1, 1] = 1
    ds, dc = M.mask_edt_reference(b)
    ys, xs = np.mgrid[0:4, 0:5]
    assert np.array_equal(ds[0], (ys - 1) ** 2 + (xs - 1) ** 2)
    want = np.zeros((4, 5), np.int32)
    want[1, 1] = 1
    assert np.array_equal(dc[0], want)


@pytest.mark.parametrize("h,w", GRIDS[:5])
def test_identity_for_feather_up_to_one_without_dilation(h, w):
    """r = 0, f <= 1: a set pixel has s <= -0.5 and 0.5 - s / f >= 1, a clear pixel s >= 0.5 and 0.5 - s / f <= 0 -> the mask itself, and the
    background is build_masks' clamp(1 - sum, 0)"""
    from tweediemix_amd import masks as M
    for dens in DENSITIES:
        fg = np.stack([_mask(h, w, dens, seed=s) for s in (1, 2)])
        bg = np.maximum(1 - fg.sum(0), 0).astype(NF)
        for f in (0.0, 0.25, 1.0):
            out = M.soft_masks_reference(fg, f, 0.0, False)
            assert out.shape == (3, 1, h, w) and out.dtype == NF
            assert np.array_equal(out[:2, 0], fg) and np.array_equal(out[2, 0], bg), (h, w, dens, f)


def test_dilation_rounds_the_corners_and_weights_grow_with_it():
    from tweediemix_amd import masks as M
    b = np.zeros((1, 20, 20), NF)
    b[0, 7:13, 7:13] = 1
    assert M.soft_masks_reference(b, 0.0, 2.0)[0].sum() == 96           # 6 x 6 grown by 2: 10 x 10 minus the four rounded corners
    assert M.soft_masks_reference(b, 0.0, -1.0)[0].sum() == 16          # eroded by 1: 4 x 4
    fg = _overlapping()[:1]
    for f in (0.0, 1.0, 2.5, 16.0):
        prev = None
        for r in (-3.0, -1.0, 0.0, 0.5, 1.5, 4.0):
            u = M.soft_masks_reference(fg, f, r)[0, 0]
            assert u.min() >= 0 and u.max() <= 1
            if prev is not None:
                assert (u >= prev).all(), (f, r)
            prev = u
    # the ramp: full width f, centred on the border
    u = M.soft_masks_reference(b, 4.0, 0.0)[0, 0][10]                   # a row through the middle of the square; border at x = 6.5 and 12.5
    assert list(u[4:10]) == [0.0, 0.125, 0.375, 0.625, 0.875, 1.0]


def test_normalised_weights_are_a_partition_of_unity_on_three_overlapping_rectangles():
    from tweediemix_amd import masks as M
    fg = _overlapping()
    assert fg.sum(0).max() == 3                                          # all three rectangles cover some pixel
    K = 4
    for f in (0.0, 1.0, 4.0, 16.0):
        for r in (-1.0, 0.0, 1.0):
            raw = M.soft_masks_reference(fg, f, r, False)[:, 0]
            nrm = M.soft_masks_reference(fg, f, r, True)[:, 0]
            assert nrm.min() >= 0 and nrm.max() <= 1
            tot = np.zeros_like(nrm[0])
            for k in range(K):
                tot = (tot + nrm[k]).astype(NF)
            assert np.abs(tot.astype(np.float64) - 1).max() <= K * 2.0 ** -23, (f, r)
            t = raw[:-1].astype(np.float64).sum(0)
            assert np.array_equal(nrm[:, t <= 1], raw[:, t <= 1])       # where the foreground sums to at most 1 nothing changes
            assert (nrm[-1][t > 1] == 0).all()
    assert M.soft_masks_reference(fg, 0.0, 0.0, False)[:-1, 0].sum(0).max() == 3


def test_batched_sets_equal_single_sets_and_bad_numbers_are_refused():
    from tweediemix_amd import masks as M
    a, b = _overlapping(seed=4), _overlapping(seed=8)
    both = M.soft_masks_reference(np.stack([a, b]), 2.5, 1.5, True)
    assert both.shape == (2, 4, 1, 16, 16)
    assert np.array_equal(both[0], M.soft_masks_reference(a, 2.5, 1.5, True)) and np.array_equal(both[1], M.soft_masks_reference(b, 2.5, 1.5, True))
    for f, r in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="feather"):
            M.soft_masks_reference(a, f, r)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def fs():
    spec = importlib.util.spec_from_file_location("fs_soft_cpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_new_flags_default_to_off(fs):
    opt = fs.build_parser().parse_args([])
    assert (opt.mask_feather, opt.mask_dilate, opt.mask_normalize, opt.reroll_feather, opt.reroll_dilate) == (0.0, 0.0, False, 0.0, 0.0)
    assert fs.check_soft_args(opt) == (None, None)
    opt = fs.build_parser().parse_args(["--mask_feather", "0", "--mask_dilate", "0"])
    assert fs.check_soft_args(opt) == (None, None)


def test_flags_are_image_pixels(fs):
    opt = fs.build_parser().parse_args(["--mask_feather", "32", "--mask_dilate", "-12", "--mask_normalize"])
    assert fs.check_soft_args(opt) == (dict(feather=4.0, dilate=-1.5, normalize=True), None)
    opt = fs.build_parser().parse_args(["--mask_normalize"])
    assert fs.check_soft_args(opt) == (dict(feather=0.0, dilate=0.0, normalize=True), None)
    opt = fs.build_parser().parse_args(["--keep_latents", "x.pt", "--reroll_feather", "16", "--reroll_dilate", "8"])
    assert fs.check_soft_args(opt) == (None, (2.0, 1.0))


def test_refusals_name_the_numbers(fs):
    for argv, words in ((["--mask_feather", "-1"], ("--mask_feather", "-1")), (["--mask_feather", "nan"], ("--mask_feather", "nan")),
                        (["--mask_feather", "inf"], ("--mask_feather", "inf")), (["--mask_dilate", "nan"], ("--mask_dilate", "nan")),
                        (["--keep_latents", "x.pt", "--reroll_feather", "-4"], ("--reroll_feather", "-4")),
                        (["--reroll_feather", "16"], ("--reroll_feather 16", "--keep_latents")),
                        (["--reroll_dilate", "-8"], ("--reroll_dilate -8", "--keep_image"))):
        with pytest.raises(SystemExit) as e:
            fs.main(["--synthetic", "--tiny"] + argv)                    # main refuses before it imports the device code
        for word in words:
            assert word in str(e.value), (argv, str(e.value))


def test_keep_weight_without_the_flags_is_todays(fs):
    import torch
    masks = torch.from_numpy(np.concatenate([_overlapping(), np.zeros((1, 16, 16), NF)]))[:, None]
    w = fs.keep_weight(masks, [0, 2])
    assert torch.equal(w, 1.0 - masks[[0, 2]].sum(dim=0, keepdim=True).clamp(max=1.0)) and w.shape == (1, 1, 16, 16)
