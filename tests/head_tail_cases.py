"""Inputs, fp64 references, per-element bounds and numpy models of the step's head and tail kernels -- tmix_conv_in, tmix_conv_in_pre, tmix_conv_out (conv_io.hip),
tmix_timestep_embedding, tmix_linear_small, tmix_linear_small_sections (rowwise.hip) -- shared by test_head_tail_numerics_gpu.py (the kernels) and
test_head_tail_cpu.py (the models and their mutations: the checker's teeth, shown without a GPU).  Built on gemm_cases.py; no HIP here.

EXACT family.  Integers in [-8, 8] with power-of-two gains (gemm_cases.ints ...): every product and every partial sum of the kernels' fp32 chains is an fp32 number in
ANY order, so the expected output is the fp64 result (fp32 outputs) or its single RNE rounding (bf16: conv_in).  gemm_cases.expected asserts the precondition
(sum |terms| / unit < 2^24) and, for conv_in, that the rounding is exercised (>= 1 % exact ties, >= 30 % inexact).  Under the pre-map S sums
|pre_b| + |pre_w| |x| through |w|: it bounds the partial sums of the map's own chain as well.

STRUCTURED family.  Values drawn once, reference in fp64 from the values the tensors hold, |out - ref| <= bound for EVERY element.  U = 2^-24 (gemm_cases.U24),
S = the sum of the magnitudes of the terms.  The derivations, from the kernels' operation order:
  conv_in     a sequential fp32 chain of n = 9 Cin products that starts from the bias, then one RNE to bf16.  Any-order summation of n + 1 terms costs n U S; as in
              gemm_cases T = 2 n U S, plus U S because a product of two fp32 numbers is itself rounded (a product of bf16 numbers is not; an fma contracts the
              rounding away, never adds one):                      T = (2 n + 1) U S,     bound = T + half the bf16 spacing at |ref| + T   (gemm_cases.out_term)
              pre-map: u_c = pre_b_c + sum_k pre_w_ck x_k is four products and four adds, eight roundings, (1 + U)^8 - 1 < 9 U:  |u^ - u| <= d_c = 9 U (|pre_b_c| +
              sum_k |pre_w_ck x_k|); carried through the taps E = sum |w| d, and the chain runs on u^:      T = (2 n + 1) U (S + E) + E
  conv_out    MFMA accumulation of n = 9 Cin products of bf16 numbers in fp32, + bias, fp32 output: gemm_cases.gemm_bound(ref, S, 9 Cin + 1, fp32)
              (one term more than the products: the bias is added behind the accumulation)
  linear      lane l multiplies and adds the eight values of the vectors l, l + 64, ...: a chain of 8 ceil(K / 512) terms; a 6-level butterfly (xor 32 .. 1) joins
              the lanes; bias and `add` follow.  A term passes through at most d = 8 ceil(K / 512) + 6 + 2 additions, and its product (fp32 x times bf16 w: 32
              significant bits) is rounded: with the factor 2 of gemm_cases                                  Tv = 2 (d + 1) U S
              act_in: the chain runs on silu_f(x) = silu(x) (1 + e), |e| <= silu_eps(x):  D = sum_k |w_k| silu_eps(x_k) |silu(x_k)|,  Tv = 2 (d + 1) U (S + D) + D
              act_out: out = silu_f(v^), |v^ - v| <= Tv, |silu'| <= SILU_SLOPE = 1.1 (its maximum is 1.0998 at x = 2.3994):
                                                         T = SILU_SLOPE Tv + eps_up (|silu(v)| + SILU_SLOPE Tv),   eps_up = silu_eps over [v - Tv, v + Tv]
              bound = T + U |ref| (out_term, fp32 output)
  silu_eps    common.h: silu_f(x) = x / (1 + __expf(-x)), __expf(y) = v_exp_f32(y log2 e).  y log2 e carries two roundings (the constant's and the product's): a
              relative 2^-23 of the argument, which the exponential turns into |x| 2^-23 of its value; v_exp_f32 is documented to 1 ulp <= 2^-23.  The error of
              e = exp(-x) reaches x / (1 + e) scaled by e / (1 + e) = sigmoid(-x); 1 + e and the division (correctly rounded: the build does not ask for the
              approximate one) are one rounding each:                  silu_eps(x) = ((|x| + 1) sigmoid(-x) + 1) 2^-23
              (relative; plus SILU_FLOOR = 2^-120 absolute: below x = -88.7 exp(-x) overflows fp32 and silu_f returns -0)
              model_silu is the CPU restatement; test_head_tail_cpu.py runs it over a dense grid on [-30, 30], also with the exponential pushed one ulp either way.
  embedding   out = cos / sin(t f), f = expf(u^), u^ = (-ln(10^4)_f32 * j) / half.  Reference cos / sin(t exp(-ln(10^4) j / half)) in fp64, layout [cos | sin].
              The two fp32 roundings of u^ move f by |u| 2^-23 of its value, the exponential (1 ulp) and the product t f by 2 2^-23 more, the sine / cosine itself
              costs 2^-23 absolute:                bound = |t| f (|u| + 2) 2^-23 + 2^-23          (|d sin| <= |d argument|)
              At j = 0 the `+ 2` is dropped: u^ = -0 exactly, expf(-0) = 1 and t * 1 = t exactly, so only the sine's own 2^-23 remains -- there a kernel that reduces
              its argument with a float32 2 pi (159 periods at t = 999: 2.8e-5) or skips the reduction has nowhere to hide.
No constant is fitted to a device.

NUMPY MODELS of the chains as the code has them (model_conv_in, model_conv_out via gemm_cases.model_accumulate, model_linear / model_sections, model_embedding)
and their mutations; test_head_tail_cpu.py holds them against the same checker.  The largest share of the accumulation term (T; for the embedding the bound
itself) a model uses beyond the output's own rounding, over all structured cases there: conv_in 0.041 (with the pre-map 0.022), conv_out 0.011, linear_small 0.069
(activations off) / 0.063 (on), embedding 0.527 (0.528 with expf, cosf and sinf rounded to the other neighbour); model_silu uses up to 0.983 of silu_eps on
[-30, 30].  Full err / bound: 1.0 for conv_in (a bf16 output: some fp32 result lies halfway between two bf16 numbers), 0.012 for conv_out, 0.086 for
linear_small.  The margins asserted there: 0.25 of T for the sums (a model rounds to nearest, which costs half of T = 2 n U S at the very most), 0.7 for the
embedding.
"""
import math

import numpy as np
import torch

import gemm_cases as G
from gemm_cases import BF, U24, check, conv_product, expected, gemm_bound, int_rows, ints, out_term, round_bf16, signs, t_use  # noqa: F401  (check, t_use: for the tests)

f32 = np.float32
F32 = torch.float32
SILU_SLOPE = 1.1
LN1E4 = math.log(10000.0)
FAMILIES = ("gauss", "offset", "quiet_image", "loud_k", "loud_out")
LIN_FAMILIES = FAMILIES + ("tails",)            # linear_small: quiet_image = one quiet row; tails = x with std 8 (both ends of silu_f)

# ------------------------------------------------------------------------------------------------ the case lists
# conv_in  B, Cin, H, W, Cout
CONV_IN_EXACT = [(3, 3, 5, 7, 128),      # <3>; borders inside a 64-pixel tile; 105 pixels: a ragged last tile
                 (2, 4, 5, 7, 32),       # the Cout minimum: one group of 8 channels per wave
                 (2, 4, 12, 20, 320),    # SDXL, 46,080 B of LDS, three workgroups per CU
                 (1, 8, 6, 10, 320),     # video, 92,160 B: the attribute branch, one per CU
                 (1, 4, 6, 10, 512),     # VAE decoder, 73,728 B: two per CU
                 (1, 4, 1, 1, 32),       # one pixel: every tap but the centre is padding
                 (2, 4, 9, 1, 64)]       # a single column
CONV_IN_LOOPED = [(2, 4, 160, 155, 32),  # 49,600 pixels, 775 tiles over a cap of 768
                  (1, 8, 130, 127, 320),  # 16,510 pixels, 258 tiles over 256
                  (1, 4, 182, 181, 512)]  # 32,942 pixels, 515 tiles over 512        (the last two end in a ragged tile; 49,600 pixels are whole tiles)
CONV_IN_PRE = [(2, 4, 5, 7, 64), (1, 4, 6, 10, 512)]
CONV_IN_LDS_WALK = (512, 640, 512, 320)  # Cout in turn on (1, 4, 6, 10): 73,728 B, 92,160 B, back under the largest size set so far, under 64 KB
CONV_IN_LARGEST = (1, 4, 6, 10, 1056)    # 152,064 B: the largest stage the entry carries (1088: 156,672 B, refused)
CONV_IN_STRUCTURED = [(3, 3, 5, 7, 128), (2, 4, 12, 20, 320), (2, 8, 6, 10, 320), (2, 4, 6, 10, 512), (2, 4, 160, 155, 32)]      # (the last one loops)
# conv_out  B, H, W, Cin, Cout
CONV_OUT_EXACT = [(3, 5, 7, 128, 3), (2, 5, 7, 320, 4), (2, 5, 7, 32, 16), (1, 5, 7, 64, 8), (1, 5, 7, 32, 1), (1, 1, 1, 32, 4), (2, 9, 1, 64, 4)]
CONV_OUT_STRUCTURED = [(3, 5, 7, 128, 3), (2, 5, 7, 320, 4), (2, 5, 7, 32, 16), (2, 33, 31, 128, 4)]      # (the last one: 2046 pixels, 32 workgroups, a ragged one)
# linear_small
LINEAR_M = (1, 4, 5, 16, 17, 37)         # <= 4: the <4> kernel; 17, 37: further launches of 16 rows, the last one ragged
LINEAR_NK = [(1280, 320), (1280, 2816), (5, 8), (1, 1280), (37, 64)]     # 2816: 5.5 vectors per lane; 8: one lane works; N % 4 != 0
SECTION_WIDTHS = (5, 320, 3, 1280)       # boundaries at 5, 325, 328 split a workgroup's four columns
SECTION_K = 320
# timestep embedding
EMBED_VALUES = (999.0, 0.0, 0.5, 1.0, 12.75, 500.0, 981.0, 1024.0, -3.0)
EMBED_DIMS = (2, 256, 320, 1280)
EMBED_COUNTS = (1, 5, 33)

# with 32 biases only, the first draw leaves under 30 % of the outputs inexact in bf16 (gemm_cases.expected refuses it): these two take the next seed
_RESEED = {("conv_in", (1, 4, 1, 1, 32)): 1, ("conv_in", (2, 4, 160, 155, 32)): 1}


def _seed(kind, shape):
    """one seed per case, by its place in its list"""
    lists = dict(conv_in=CONV_IN_EXACT + CONV_IN_LOOPED + [CONV_IN_LARGEST] + [(1, 4, 6, 10, c) for c in CONV_IN_LDS_WALK[1:]], conv_in_pre=CONV_IN_PRE,
                 conv_out=CONV_OUT_EXACT, linear=LINEAR_NK)
    return dict(conv_in=3000, conv_in_pre=3400, conv_out=3600, linear=3800)[kind] + 10 * lists[kind].index(tuple(shape)) + _RESEED.get((kind, tuple(shape)), 0)


# ------------------------------------------------------------------------------------------------ launch geometry of conv_in (conv_io.hip, restated)
def conv_in_smem(Cin, Cout):
    return Cout * 9 * Cin * 4


def conv_in_grid_cap(Cin, Cout):
    """256 * per_cu: the largest grid the entry launches; more 64-pixel tiles than that means a second trip of the persistent loop"""
    s = conv_in_smem(Cin, Cout)
    return 256 * (1 if s > 80 * 1024 else 2 if s > 52 * 1024 else 3)


def conv_in_tiles(B, H, W):
    return (B * H * W + 63) // 64


# ------------------------------------------------------------------------------------------------ exact family
def exact_conv_in(shape, pre=False):
    return G.exact_conv_in(*shape, _seed("conv_in_pre" if pre else "conv_in", shape), pre=pre)


def exact_conv_out(shape):
    return G.exact_conv_out(*shape, _seed("conv_out", shape))


def exact_linear(N, K, M=max(LINEAR_M), seed=None):
    """x fp32 [M, K], w bf16 [N, K], bias fp32 [N], add fp32 [M, N], all integers; exp_plain / exp_bias / exp_full fp32 [M, N] without bias and add, with the bias,
    with both.  Rows are independent: a launch of m <= M rows is held against the first m rows"""
    what = f"exact_linear {M}x{N}x{K}"
    seed = _seed("linear", (N, K)) if seed is None else seed
    pos = G.default_pos(K, False)
    x = ints((M, K), seed, pos)
    w = ints((N, K), seed + 1, pos) * signs(N, seed + 2).view(N, 1)
    b, add = int_rows((N,), seed + 5, 600), int_rows((M, N), seed + 7, 256)
    ref, S = x @ w.T, x.abs() @ w.abs().T
    one = torch.ones_like(ref)
    c = dict(x=x.float(), w=G._bf(w, what), bias=b.float(), add=add.float())
    c["exp_plain"] = expected(ref, S, one, what, rounding=False)[1]
    c["exp_bias"] = expected(ref + b, S + b.abs(), one, what, rounding=False)[1]
    c["exp_full"] = expected(ref + b + add, S + b.abs() + add.abs(), one, what, rounding=False)[1]
    return c


def section_starts(widths=SECTION_WIDTHS):
    return [0] + [int(v) for v in np.cumsum(widths)]


def sections_flat(y, starts):
    """[M, N] -> the flat layout of tmix_linear_small_sections: section s a dense [M, width_s] matrix at starts[s] * M"""
    return torch.cat([y[:, a:b].reshape(-1) for a, b in zip(starts[:-1], starts[1:])])


def exact_sections(M):
    c = exact_linear(sum(SECTION_WIDTHS), SECTION_K, M, seed=3900)
    c["starts"] = section_starts()
    return c


# ------------------------------------------------------------------------------------------------ structured family
def _structure(family, x, w, b_axis_x=0, k_axis_x=-1):
    """the in-place part the families share: one image (row) of x times 2^-10, one input channel times 100, three filter rows times 100"""
    if family == "quiet_image":
        assert x.shape[b_axis_x] >= 2, "quiet_image needs a louder neighbour"
        x.select(b_axis_x, x.shape[b_axis_x] - 1).mul_(2.0 ** -10)
    elif family == "loud_k":
        x.select(k_axis_x, 1 % x.shape[k_axis_x]).mul_(100.0)
    elif family == "loud_out":
        for j in G.LOUD_OUT_ROWS:
            w[j % w.shape[0]] *= 100.0


def structured_conv_in(family, shape, seed=4000, pre=False):
    """x fp32 NCHW, w fp32 OHWI, bias fp32 (any fp32 values: nothing here is a bf16 number); ref, T, bound fp64 NHWC"""
    assert family in FAMILIES, family
    B, Cin, H, W, Cout = shape
    g = G._gen(seed + 7 * FAMILIES.index(family) + Cout + Cin)
    if family == "offset" and Cin == 3:
        x = torch.rand(B, H, W, Cin, generator=g) * 2 - 1 + 0.5           # RGB in [-1, 1], off centre
    else:
        x = torch.randn(B, H, W, Cin, generator=g) + (3.0 if family == "offset" else 0.0)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g)
    _structure(family, x, w)
    c = dict(x=x.permute(0, 3, 1, 2).contiguous(), w=w, bias=b)
    xd, wd, n = x.double(), w.double(), 9 * Cin
    u, E = xd, 0.0
    if pre:
        pw = torch.eye(4) + 0.2 * torch.randn(4, 4, generator=g)
        pb = 0.1 * torch.randn(4, generator=g)
        c.update(pre_w=pw, pre_b=pb)
        u = xd @ pw.double().T + pb.double()
        d = 9.0 * U24 * (xd.abs() @ pw.double().abs().T + pb.double().abs())
        E = conv_product(d, wd.abs(), G.S1)
    ref = conv_product(u, wd, G.S1) + b.double()
    S = conv_product(u.abs(), wd.abs(), G.S1) + b.double().abs()
    T = (2 * n + 1) * U24 * (S + E) + E
    c.update(ref=ref, T=T, bound=out_term(ref, T, BF))
    return c


def structured_conv_out(family, shape, seed=4200):
    """x bf16 NHWC, w bf16 OHWI, bias fp32; ref, T, bound fp64 NCHW.  offset: silu(gauss), what a GroupNorm + SiLU feeds conv_out"""
    assert family in FAMILIES, family
    B, H, W, Cin, Cout = shape
    g = G._gen(seed + 7 * FAMILIES.index(family) + Cin + Cout)
    x = torch.randn(B, H, W, Cin, generator=g)
    if family == "offset":
        x = torch.nn.functional.silu(x)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g)
    _structure(family, x, w)
    x, w = x.to(BF), w.to(BF)
    xd, wd, n = x.double(), w.double(), 9 * Cin + 1
    ref = (conv_product(xd, wd, G.S1) + b.double()).permute(0, 3, 1, 2).contiguous()
    S = (conv_product(xd.abs(), wd.abs(), G.S1) + b.double().abs()).permute(0, 3, 1, 2).contiguous()
    return dict(x=x, w=w, bias=b, ref=ref, T=2.0 * n * U24 * S, bound=gemm_bound(ref, S, n, F32))


def silu64(x):
    return x * torch.sigmoid(x)


def silu_eps(x):
    """the relative error of common.h's silu_f at x (fp64 tensor): see the module docstring"""
    return ((x.abs() + 1.0) * torch.sigmoid(-x) + 1.0) * 2.0 ** -23


def linear_depth(K):
    return 8 * ((K + 511) // 512) + 6 + 2


def linear_bound(x, w, bias, add, act_in, act_out):
    """(ref, T, bound) fp64 [M, N] of tmix_linear_small from the values x (fp32), w (bf16), bias, add (fp32 or None) hold"""
    xd, wd = x.double(), w.double()
    K = x.shape[1]
    xs, D = xd, 0.0
    if act_in:
        xs = silu64(xd)
        D = (silu_eps(xd) * xs.abs() + SILU_FLOOR) @ wd.abs().T
    v, S = xs @ wd.T, xs.abs() @ wd.abs().T
    for t in (bias, add):
        if t is not None:
            v, S = v + t.double(), S + t.double().abs()
    T = 2.0 * (linear_depth(K) + 1) * U24 * (S + D) + D
    ref = v
    if act_out:
        ref = silu64(v)
        lo, hi = v - T, v + T
        eps_up = ((torch.maximum(lo.abs(), hi.abs()) + 1.0) * torch.sigmoid(-lo) + 1.0) * 2.0 ** -23
        T = SILU_SLOPE * T + eps_up * (ref.abs() + SILU_SLOPE * T) + SILU_FLOOR
    return ref, T, out_term(ref, T, F32)


def structured_linear(family, M, N, K, seed=4400):
    """x fp32 [M, K], w bf16 [N, K], bias fp32 [N], add fp32 [M, N]"""
    assert family in LIN_FAMILIES, family
    g = G._gen(seed + 7 * LIN_FAMILIES.index(family) + N + K)
    x = torch.randn(M, K, generator=g) * (8.0 if family == "tails" else 1.0) + (3.0 if family == "offset" else 0.0)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    _structure("gauss" if family == "quiet_image" and M < 2 else family, x, w)              # (a single row has no louder neighbour)
    return dict(x=x, w=w.to(BF), bias=torch.randn(N, generator=g), add=torch.randn(M, N, generator=g))


def embed_values(count):
    return torch.tensor(np.resize(np.asarray(EMBED_VALUES, f32), count))


def embed_reference(values, dim):
    """(ref, A, bound) fp64 [count, dim]: A the accumulated term |t| f (|u| + 2 [j > 0]) 2^-23, bound = A + 2^-23"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64)
    u = -LN1E4 * j / half
    f = torch.exp(u)
    t = values.double().view(-1, 1)
    arg = t * f
    A = t.abs() * f * (u.abs() + 2.0 * (j > 0)) * 2.0 ** -23
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1), torch.cat([A, A], 1), torch.cat([A, A], 1) + 2.0 ** -23


def embed_use(out, ref, A):
    """the share of A the error takes beyond the trailing 2^-23 (0 where it stays within it; an element with A = 0 that does not counts as infinite)"""
    over = ((out.double() - ref).abs() - 2.0 ** -23).clamp_min(0.0)
    r = torch.where(A > 0, over / A.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), torch.zeros_like(over)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ numpy models of the chains
def tap_index(B, H, W, col_slack=0):
    """[B H W, 9] flat source pixel of every tap, -1 where it is padding.  col_slack = 1: the mutation `ix <= W` of the border predicate -- the tap at ix = W reads
    the next pixel in memory (the first one of the next row), nothing behind the tensor"""
    p = np.arange(B * H * W)
    b, oy, ox = p // (H * W), (p % (H * W)) // W, p % W
    idx = np.full((p.size, 9), -1, np.int64)
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy + ky - 1, ox + kx - 1
            src = (b * H + iy) * W + ix
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W + col_slack) & (src < p.size)
            idx[:, ky * 3 + kx] = np.where(ok, src, -1)
    return idx


def gather_taps(px, idx, pad=None):
    """px [npix, C] -> [npix, 9 C] tap-major; padding taps read `pad` ([C]; None: zero)"""
    C = px.shape[1]
    ext = np.concatenate([px, (np.zeros((1, C), px.dtype) if pad is None else np.asarray(pad, px.dtype).reshape(1, C))], 0)
    return ext[idx].reshape(idx.shape[0], 9 * C)


def model_conv_in(c, shape, mutate=None):
    """conv_in_kernel on the CPU: fp32 [B, H, W, Cout] holding the bf16 outputs, NaN where nothing was stored.  mutate: 'truncate' | 'bias_bf16' | 'x_bf16' |
    'pre_bias_in_padding' | 'drop_ragged_tile' | 'single_trip'"""
    B, Cin, H, W, Cout = shape
    px = c["x"].permute(0, 2, 3, 1).reshape(-1, Cin).numpy().astype(f32)
    if mutate == "x_bf16":
        px = round_bf16(px)
    pad = None
    if "pre_w" in c:                             # u = b + w0 v0 + w1 v1 + w2 v2 + w3 v3, left to right in fp32
        pw, pb = c["pre_w"].numpy().astype(f32), c["pre_b"].numpy().astype(f32)
        u = np.broadcast_to(pb, px.shape).copy()
        for k in range(4):
            u = u + pw[None, :, k] * px[:, k, None]
        px = u.astype(f32)
        if mutate == "pre_bias_in_padding":
            pad = pb
    patch = gather_taps(px, tap_index(B, H, W), pad)
    w = c["w"].reshape(Cout, -1).numpy().astype(f32)
    bias = c["bias"].numpy().astype(f32)
    acc = np.broadcast_to(round_bf16(bias) if mutate == "bias_bf16" else bias, (patch.shape[0], Cout)).astype(f32)
    for k in range(patch.shape[1]):
        acc = acc + patch[:, k, None] * w[None, :, k]
    assert acc.dtype == f32
    out = round_bf16(acc, truncate=mutate == "truncate")
    npix = patch.shape[0]
    if mutate == "drop_ragged_tile" and npix % 64:
        out[npix // 64 * 64:] = np.nan
    if mutate == "single_trip":
        out[conv_in_grid_cap(Cin, Cout) * 64:] = np.nan
    return out.reshape(B, H, W, Cout)


CONV_OUT_GUARD = 16        # the model's (and the GPU test's) NaN guard behind the output, in planes of H W floats: where lanes fr >= Cout of the last image would store


def model_conv_out(c, shape, mutate=None, order="block32"):
    """conv_out_kernel on the CPU: (fp32 NCHW [B, Cout, H, W], the guard planes behind it).  The MFMA chain is gemm_cases.model_accumulate over the tap-major
    K = 9 Cin in blocks of 32 (one 16x16x32 instruction), then + bias.  mutate: 'padded_rows_stored' (the `fr < Cout` guard of the stores gone: lane fr >= Cout holds
    the replicated last filter row and lands fr - Cout planes into the next image, or behind the tensor) | 'bias_channel0' | 'border_column'"""
    B, H, W, Cin, Cout = shape
    px = c["x"].reshape(-1, Cin).float().numpy()
    a = gather_taps(px, tap_index(B, H, W, 1 if mutate == "border_column" else 0))
    w = c["w"].reshape(Cout, -1).float().numpy()
    bias = c["bias"].numpy().astype(f32)
    acc = G.model_accumulate(a, w, order)                                      # [npix, Cout]
    y = acc + (bias[0] if mutate == "bias_channel0" else bias[None, :])
    assert y.dtype == f32
    hw = H * W
    buf = np.full((B * Cout + CONV_OUT_GUARD) * hw, np.nan, f32)
    buf[:B * Cout * hw] = y.reshape(B, hw, Cout).transpose(0, 2, 1).reshape(-1)
    if mutate == "padded_rows_stored":
        pad = acc[:, Cout - 1].reshape(B, hw)                                  # (+ a bias read behind the array: left out, 0)
        for bb in range(B):
            for fr in range(Cout, 16):
                buf[(bb * Cout + fr) * hw:(bb * Cout + fr + 1) * hw] = pad[bb]
    return buf[:B * Cout * hw].reshape(B, Cout, H, W), buf[B * Cout * hw:]


LOG2E = f32(1.4426950408889634)
SILU_FLOOR = 2.0 ** -120       # below x = -88.7 exp(-x) overflows fp32 and silu_f returns -0, where |silu(x)| < 89 e^-88.7 < 2^-120; denormal results may be flushed as well


def faithful(v, direction):
    """fp64 -> fp32 rounded to nearest (direction 0) or to the fp32 neighbour above (> 0) / below (< 0) the value: the two results a function good to one ulp may
    return.  direction: a number, or an array of them"""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        r = v.astype(f32)
    up = np.where(r.astype(np.float64) < v, np.nextafter(r, f32(np.inf)), r)
    dn = np.where(r.astype(np.float64) > v, np.nextafter(r, f32(-np.inf)), r)
    d = np.broadcast_to(np.asarray(direction), r.shape)
    return np.where(d > 0, up, np.where(d < 0, dn, r)).astype(f32)


def model_silu(x, nudge=0):
    """silu_f on the CPU: x / (1 + 2^(fl(-x log2 e))) in fp32, the exponential correctly rounded (nudge = +-1: the fp32 neighbour above / below the value, what a 1-ulp v_exp_f32 may return)"""
    x = np.asarray(x, f32)
    a = (-x) * LOG2E
    assert a.dtype == f32
    with np.errstate(over="ignore"):
        e = faithful(np.exp2(a.astype(np.float64)), nudge)
    return x / (f32(1.0) + e)


def model_linear(x, w, bias=None, add=None, act_in=False, act_out=False, mutate=None):
    """linear_small_kernel on the CPU -> fp32 [M, N].  Lane l: the vectors l, l + 64, ... of eight values, multiplied and added in turn; the xor butterfly 32 .. 1 is
    the pairwise tree of gemm_cases._tree; then + bias, + add, silu_f.  mutate: 'lane_loop_whole_rounds' (the lane loop stops at K / 512 * 512)"""
    x, w = np.asarray(x, f32), np.asarray(w, f32)
    (M, K), N = x.shape, w.shape[0]
    if act_in:
        x = model_silu(x)
    R = K // 512 if mutate == "lane_loop_whole_rounds" else (K + 511) // 512
    Kp = R * 512
    xp, wp = np.zeros((M, max(Kp, K)), f32), np.zeros((N, max(Kp, K)), f32)             # a zero product leaves an fp32 sum as it is
    xp[:, :K], wp[:, :K] = x, w
    xp, wp = xp[:, :Kp].reshape(M, R, 64, 8), wp[:, :Kp].reshape(N, R, 64, 8)
    acc = np.zeros((M, N, 64), f32)
    for r in range(R):
        for j in range(8):
            acc = acc + xp[:, None, r, :, j] * wp[None, :, r, :, j]
    y = G._tree(acc)
    if bias is not None:
        y = y + np.asarray(bias, f32)[None, :]
    if add is not None:
        y = y + np.asarray(add, f32)
    assert y.dtype == f32
    return model_silu(y) if act_out else y


def model_sections(y0, starts, add=None, guard=64, mutate=None):
    """where the launches of the sections form store y0 [M, N] (the kernel's acc + bias): a flat fp32 buffer of M N + guard floats, NaN where nothing was stored.
    Rows leave 16 per launch.  add [M, N]: the kernel takes it in this form too, though tmix_linear_small_sections passes none -- the model keeps the operand so
    that its indexing is held.  mutate: 'base_launch_rows' (the section base secs[s] * the launch's rows instead of * Mtot) | 'add_section_width' (add read at
    m * width + n)"""
    M, N = y0.shape
    out = np.full(M * N + guard, np.nan, f32)
    addf = None if add is None else np.asarray(add, f32).reshape(-1)
    for m0 in range(0, M, 16):
        rows = min(16, M - m0)
        for s in range(len(starts) - 1):
            ldn = starts[s + 1] - starts[s]
            base = starts[s] * (rows if mutate == "base_launch_rows" else M)
            for m in range(rows):
                v = y0[m0 + m, starts[s]:starts[s + 1]]
                if addf is not None:
                    n = np.arange(starts[s], starts[s + 1])
                    v = v + addf[(m0 + m) * (ldn if mutate == "add_section_width" else N) + n]
                o = base + (m0 + m) * ldn
                out[o:o + ldn] = v
    return out


def model_embedding(values, dim, mutate=None, nudge=0):
    """timestep_embedding_kernel on the CPU, expf / cosf / sinf correctly rounded (nudge = +-1: each rounded to the neighbour on the other side instead, alternating from frequency to frequency)
    -> fp32 [count, dim].  mutate: 'exponent_half_minus_1' | 'sin_cos_order' | 'exp_2^-12' | 'two_pi_f32' (the argument reduced by fp32 multiples of a float32 2 pi)"""
    half = dim // 2
    j = np.arange(half, dtype=f32)
    den = f32(max(half - 1, 1)) if mutate == "exponent_half_minus_1" else f32(half)
    e = f32(-9.210340371976184) * j / den
    assert e.dtype == f32
    alt = np.where(np.arange(half) % 2 == 0, 1, -1) * nudge
    freq = faithful(np.exp(e.astype(np.float64)), alt)
    if mutate == "exp_2^-12":
        freq = np.where(j > 0, freq * f32(1 + 2.0 ** -12), freq)
    a = np.asarray(values, f32).reshape(-1, 1) * freq[None, :]
    assert a.dtype == f32
    if mutate == "two_pi_f32":
        tp = f32(2 * math.pi)
        a = a - np.rint(a / tp) * tp
        assert a.dtype == f32
    co, si = faithful(np.cos(a.astype(np.float64)), alt[None, :]), faithful(np.sin(a.astype(np.float64)), -alt[None, :])
    return np.concatenate([si, co] if mutate == "sin_cos_order" else [co, si], 1)
