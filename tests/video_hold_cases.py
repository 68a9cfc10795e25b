"""Shared by tests/test_video_hold_cpu.py and tests/test_video_hold_gpu.py: inputs of the video sampler's hold regions.

Everything the hold computes is compared by equality, so the inputs only have to reach every branch of the blend: the weights hold exact 0, exact 1 and
fractions (in every frame and in every video), the held latent holds a -0.0 (which hs == 0 must give back with its sign), and the shapes are small and
odd -- C = 4, F = 3, hw = 5 x 7 -- so that a video boundary, a frame boundary and a channel boundary all fall inside one workgroup."""
import numpy as np

from video_noise_cases import KEYS, SEEDS                     # three videos' {low word, high word} and the seeds they come from

NF = np.float32
C, F, HH, WW = 4, 3, 5, 7
HW = HH * WW
CZ, STEP = float(NF(0.3125)), 7
HA, HS = float(NF(0.8125)), float(NF(0.5830))                 # (ha, hs) of a written state; not a unit pair on purpose: nothing may assume one
NEG0 = (0, 0, 1, 1)                                           # (channel, frame, y, x) of the -0.0 in every held latent
BIG = (2, 362, 363)                                           # F, h, w: 4 x 2 x 131406 = 1,051,248 elements > 4096 x 256: a second grid-stride pass


def held_latent(S, Fk, seed, h=HH, w=WW, c=C):
    """kx [S, C, Fk, h, w] fp32 with a -0.0 at NEG0 of every video: in row 1, where weight() is exactly 1"""
    kx = np.random.RandomState(seed).randn(S, c, Fk, h, w).astype(NF)
    kx[(slice(None),) + NEG0] = NF(-0.0)
    return kx


def weight(S, Fw, seed, h=HH, w=WW):
    """w [S, Fw, h, w] fp32 in [0, 1]: row 0 of every map exactly 0 and its neighbour exactly 1 (so both selects are taken in every frame of every
    video), row 2 the same two constants swapped per map (so the maps differ between frames and videos), fractions elsewhere"""
    wt = np.random.RandomState(seed).rand(S, Fw, h, w).astype(NF)
    wt = np.clip(wt, NF(0.0625), NF(0.9375))
    wt[:, :, 0, :] = 0.0
    wt[:, :, 1, :] = 1.0
    for s in range(S):
        for f in range(Fw):
            wt[s, f, 2, :] = NF((s + f) % 2)
    assert wt.min() == 0.0 and wt.max() == 1.0 and ((wt > 0) & (wt < 1)).any()
    return wt


def bits(a):
    """fp32 array -> its uint32 view: equality that tells -0.0 from 0.0 and one NaN from another"""
    return np.ascontiguousarray(a, NF).view(np.uint32)


def hold_noise(per, keys):
    """zh [len(keys), per]: element r of video s draws from (r, keys[s], step 0, STREAM_VIDEO_HOLD)"""
    from tweediemix_amd import noise as NZ
    return np.stack([NZ.normal(np.arange(per, dtype=np.uint64), lo, hi, 0, NZ.STREAM_VIDEO_HOLD) for lo, hi in keys])


def write_masks(directory, height, width):
    """two 8-bit mask images on the image grid (white rectangles, disjoint) -> their paths; on the latent grid (/ 8) the union covers rows
    [1, 5) x columns [1, 3) and rows [8, 12) x columns [4, 7)"""
    import os
    from PIL import Image
    out = []
    for name, (y0, y1, x0, x1) in (("a.png", (8, 40, 8, 24)), ("b.png", (64, 96, 32, 56))):
        m = np.zeros((height, width), np.uint8)
        m[y0:y1, x0:x1] = 255
        path = os.path.join(str(directory), name)
        Image.fromarray(m).save(path)
        out.append(path)
    return out


def latent_union(h, w):
    """the union of write_masks' rectangles on the latent grid, bool [h, w]"""
    u = np.zeros((h, w), bool)
    u[1:5, 1:3] = True
    u[8:12, 4:7] = True
    return u
