"""Inputs shared by tests/test_attn_shapes_cpu.py and tests/test_attn_shapes_gpu.py: the mask kinds of the connected-component tests and the
score sets built from them.  Every generator returns a valid map at every size (a kind that does not fit a tiny grid degenerates, it never
fails), and every reference is computed once per case and handed out read-only."""
import functools

import numpy as np

NF = np.float32
KINDS = ("empty", "full", "corner", "checker", "serpentine", "spiral", "comb", "diag_pair", "rings", "tie", "random_half", "random_dense")


def _spiral(h, w):
    """a one-pixel path that winds inwards from the top-left corner, one clear pixel between its arms"""
    m = np.zeros((h, w), NF)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    for _ in range(h * w):
        for _turn in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy                         # right -> down -> left -> up
        else:
            break
    return m


def mask(kind, i, h, w):
    """one [h, w] fp32 map, set where >= 0.5; the random kinds hold VALUES (the threshold decides), the others {0, 1}; i varies the instance"""
    rng = np.random.RandomState(1000 * KINDS.index(kind) + 17 * i + h + 3 * w)
    m = np.zeros((h, w), NF)
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "full":
        m[:] = 1
    elif kind == "corner":
        m[(h - 1) * (i % 2), (w - 1) * ((i // 2 + 1) % 2)] = 1
    elif kind == "checker":                          # every set pixel its own component
        m[(ys + xs + i) % 2 == 0] = 1
    elif kind == "serpentine":                       # full rows joined at alternating ends: one component, labels travel the whole path
        m[0::2] = 1
        m[1::4, w - 1] = 1
        m[3::4, 0] = 1
    elif kind == "spiral":
        m = _spiral(h, w)
    elif kind == "comb":                             # teeth joined only along the last row: labels travel against raster order
        m[:, i % 2::2] = 1
        m[h - 1] = 1
    elif kind == "diag_pair":                        # two blobs that touch only diagonally: two components
        a, b = max(1, h // 3), max(1, w // 3)
        m[0:a, 0:b] = 1
        m[a:2 * a, b:2 * b] = 1
    elif kind == "rings":                            # ring, gap, ring, ..., centre: holes within holes
        c = np.minimum(np.minimum(ys, h - 1 - ys), np.minimum(xs, w - 1 - xs))
        m[(c + i) % 2 == 1] = 1
    elif kind == "tie":                              # two components of equal area
        a, b = max(1, h // 3), max(1, w // 3)
        m[0:a, 0:b] = 1
        m[h - a:h, w - b:w] = 1
    elif kind == "random_half":                      # below the percolation density: many mid-sized clusters
        m = rng.rand(h, w).astype(NF)
    elif kind == "random_dense":                     # density 0.62, above it: one ragged giant component full of holes
        m = (rng.rand(h, w) + 0.12).astype(NF)
    return m


@functools.lru_cache(maxsize=None)
def label_case(shape, kind, invert):
    """(maps [n,h,w] fp32, labels int32 [n,h,w] of masks.mask_label_reference at threshold 0.5)"""
    from tweediemix_amd import masks as M
    n, h, w = shape
    maps = np.stack([mask(kind, i, h, w) for i in range(n)])
    lab = M.mask_label_reference(maps, 0.5, invert)
    for a in (maps, lab):
        a.setflags(write=False)
    return maps, lab


def smooth_field(rng, h, w, lo=0.55, hi=1.0):
    """a smooth random field in [lo, hi] (a coarse random grid, bilinearly upsampled)"""
    from tweediemix_amd import masks as M
    coarse = rng.rand((h + 7) // 8 + 1, (w + 7) // 8 + 1)
    return (lo + (hi - lo) * M._upsample_bilinear(coarse, h, w)).astype(NF)


SCORE_FIRST = ("rings", "random_dense", "serpentine")          # set 0: large shapes with holes that overlap one another
SCORE_OTHERS = ("full", "comb", "spiral", "checker", "random_half", "tie", "diag_pair", "corner", "empty")
THRESHOLD = 0.5


def score_kinds(h, w, km1):
    """the mask kinds of the two sets: set 0 the first km1 of SCORE_FIRST, set 1 km1 of the others, rotating with the grid so that the four
    grids of the tests cover all of them"""
    first = {(5, 7): 0, (33, 65): 3, (64, 64): 6, (128, 128): 7}.get((h, w), 0)
    return SCORE_FIRST[:km1], tuple(SCORE_OTHERS[(first + k) % len(SCORE_OTHERS)] for k in range(km1))


@functools.lru_cache(maxsize=None)
def score_sets(h, w, km1):
    """score [2, km1, h, w] fp32: thresholded mask kinds times smooth random fields in [0.55, 1], so that a set pixel stays above THRESHOLD
    and the overlap's owner varies from pixel to pixel"""
    rng = np.random.RandomState(h * 131 + w * 7 + km1)
    out = np.zeros((2, km1, h, w), NF)
    for s, kinds in enumerate(score_kinds(h, w, km1)):
        for k, kind in enumerate(kinds):
            out[s, k] = (mask(kind, s + k, h, w) >= NF(0.5)) * smooth_field(rng, h, w)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shapes_case(h, w, km1, fill, resolve):
    """(score [2,km1,h,w], masks.attn_shapes_reference of it): n_sets = 1 is the first set of both"""
    from tweediemix_amd import masks as M
    score = score_sets(h, w, km1)
    want = M.attn_shapes_reference(score, THRESHOLD, fill, resolve)
    want.setflags(write=False)
    return score, want


@functools.lru_cache(maxsize=None)
def equal_score_case(h, w):
    """three concepts whose scores take only the values 0, 0.75 and 1 (all exact in fp32): rings, full and random_dense overlap on many
    pixels with EXACTLY equal scores"""
    rng = np.random.RandomState(99)
    score = np.zeros((1, 3, h, w), NF)
    for k, kind in enumerate(("rings", "full", "random_dense")):
        level = np.where(smooth_field(rng, h, w, 0.0, 1.0) >= 0.5, NF(1.0), NF(0.75))
        score[0, k] = (mask(kind, k, h, w) >= 0.5) * level
    score.setflags(write=False)
    return score
