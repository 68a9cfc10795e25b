"""Inputs, fp64 reference and per-element bound shared by test_norm_numerics_gpu.py (the kernels) and test_norm_bound_cpu.py (the CPU model the
bound's constant comes from).  See the docstring of test_norm_numerics_gpu.py for the derivation."""
import math

import numpy as np
import torch

BF = torch.bfloat16
GROUPS = 32
U24 = 2.0 ** -24
# k of E_s and E_m: twice the largest value the CPU model (test_norm_bound_cpu.py: no fp32 chain longer than 32 terms, fp64 above) needs over the
# input sets below -- 2.35 for GroupNorm (offset, r = 100), 1.87 for LayerNorm -- rounded up to a whole number.  NOT fitted to the device.
K = 5.0

# (family, target r, eps).  eps 1e-5: the UNets; 1e-6: the VAE and the transformer norms
GN_FAMILIES = [("offset", 0, 1e-5), ("offset", 3, 1e-5), ("offset", 10, 1e-5), ("offset", 30, 1e-5), ("offset", 100, 1e-6),
               ("channel_means", 10, 1e-5), ("channel_means", 100, 1e-6), ("loud_channel", 0, 1e-5),
               ("tiny", 0, 1e-5), ("tiny", 0, 1e-6), ("large", 3, 1e-5), ("constant", 0, 1e-5)]
# (B, HW, C1, C2, silu) per form
GN_THREE = [(2, 1024, 320, 0, True), (1, 4096, 640, 320, True), (2, 2048, 64, 0, False)]
GN_ONE = [(3, 336, 1280, 0, True), (2, 84, 640, 320, False), (1, 100, 64, 0, True)]
GN_PRE = [(2, 256, 320, 0, True), (1, 1024, 1280, 640, True), (2, 32, 32, 0, False)]
CONST_GROUP, CONST_VALUE = 7, 3.0
LOUD_GROUP, LOUD_GAIN = 5, 40.0

LN_SHAPES = [(5, 64), (77, 640), (300, 2048)]
LN_FAMILIES = [("offset", 0, 1e-5), ("offset", 10, 1e-5), ("offset", 100, 1e-6), ("offset", 1000, 1e-5), ("tiny", 0, 1e-6)]


def fam_id(f):
    return f"{f[0]}-r{f[1]}-eps{f[2]:g}"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def gn_input(family, r, B, HW, C, seed, groups=GROUPS):
    """fp32 [B, HW, C] on the CPU, built per group; the caller rounds it to bf16"""
    cpg = C // groups
    z = torch.randn(B, HW, C, generator=_gen(seed), dtype=torch.float32)
    if family in ("offset", "large"):       # standardised per (image, group): a group of 32 values realises the target r too
        zg = z.view(B, HW, groups, cpg)
        zg -= zg.mean(dim=(1, 3), keepdim=True)
        zg /= zg.std(dim=(1, 3), keepdim=True, unbiased=False)
        z += float(r)
        if family == "large":
            z *= 256.0
    elif family == "tiny":
        z *= 2.0 ** -10
    elif family == "channel_means":         # a mean of its own per channel, spread over +-r; within-channel std 1.  Group 0 stays at mean 0
        m = (torch.rand(C, generator=_gen(seed + 1)) * 2 - 1) * float(r)
        m[:cpg] = 0
        z += m
    elif family == "loud_channel":
        z[:, :, LOUD_GROUP % groups * cpg + min(1, cpg - 1)] *= LOUD_GAIN
    elif family == "constant":
        g = CONST_GROUP % groups
        z[:, :, g * cpg:(g + 1) * cpg] = CONST_VALUE
    else:
        raise ValueError(family)
    return z


def affine(C, seed):
    """gamma, beta fp32 [C] on the CPU"""
    return torch.randn(C, generator=_gen(seed + 2)), torch.randn(C, generator=_gen(seed + 3))


def gn_reference(x, gamma, beta, eps, silu, groups=GROUPS):
    """fp64, from the values x (bf16 [B, HW, C]) holds: dict of ref, xhat [B, HW, C] and mu, s, r [B, 1, groups, 1]"""
    B, HW, C = x.shape
    xd = x.double().view(B, HW, groups, C // groups)
    mu = xd.mean(dim=(1, 3), keepdim=True)
    v = ((xd - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    s = torch.sqrt(v + float(np.float32(eps)))
    xh = (xd - mu) / s
    z = gamma.double().view(1, 1, groups, -1) * xh + beta.double().view(1, 1, groups, -1)
    ref = z * torch.sigmoid(z) if silu else z
    return dict(ref=ref.view(B, HW, C), xhat=xh.view(B, HW, C), mu=mu, s=s, r=mu.abs() / s)


def bf16_half_spacing(ref):
    """half the distance between the two bf16 numbers around ref: what ONE round-to-nearest to bf16 can cost.  Between 2^-9 |ref| (just under a power
    of two) and 2^-8 |ref| (at one): bf16 has 8 significant bits"""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def out_round(ref):
    """the output's single rounding to bf16 plus 2^-20 |ref| for the fp32 arithmetic behind the statistics (SiLU's v_exp / v_rcp, the last fma)"""
    return bf16_half_spacing(ref) + 2.0 ** -20 * ref.abs()


def norm_bound(ref, xhat, r, gamma, silu, k=K, es_power=2, ks_final=None):
    """out_round(ref) + S |gamma| (|xhat| E_s + E_m);  r and gamma broadcast against ref.  es_power 2: GroupNorm (E[x^2] - mean^2), 1: LayerNorm.
    ks_final: E_s = 2^-24 + ks_final (1 + r^2) 2^-24 instead (the finaliser cases below)"""
    S = 1.1 if silu else 1.0
    e_s = k * (1 + r ** es_power) * U24 if ks_final is None else (1 + ks_final * (1 + r ** 2)) * U24
    e_m = k * (1 + r) * U24
    return out_round(ref) + S * gamma.abs() * (xhat.abs() * e_s + e_m)


def stat_use(out, ref, xhat, r, gamma, silu, k=K, es_power=2):
    """the share of the STATISTICS term S |gamma| (|xhat| E_s + E_m) that the error beyond the output's rounding takes, largest over the elements.  (The
    full err / bound is about 1.0 on any large tensor whatever the kernel does: some fp32 result lies halfway between two bf16 numbers.)"""
    S = 1.1 if silu else 1.0
    stat = S * gamma.abs() * (xhat.abs() * k * (1 + r ** es_power) + k * (1 + r)) * U24
    return float((((out.double() - ref).abs() - out_round(ref)).clamp_min(0.0) / stat.clamp_min(1e-300)).max())


def gn_err_over_bound(out, x, gamma, beta, eps, silu, k=K, groups=GROUPS):
    """(max |out - ref| / bound over the elements, the reference dict).  The constant group of the `constant` family is NOT treated specially here"""
    R = gn_reference(x, gamma, beta, eps, silu, groups)
    B, HW, C = x.shape
    r = R["r"].expand(B, 1, groups, C // groups).reshape(B, 1, C)
    bound = norm_bound(R["ref"], R["xhat"], r, gamma.double().view(1, 1, C), silu, k)
    assert float(bound.min()) > 0.0
    R["stat_use"] = stat_use(out, R["ref"], R["xhat"], r, gamma.double().view(1, 1, C), silu, k)
    return ((out.double() - R["ref"]).abs() / bound), R


def ln_input(family, r, rows, C, seed):
    """fp32 [rows, C] whose bf16 rounding has row mean / row std = r.  bf16 cannot hold N(1000, 1) (its spacing at 1000 is 4): at r = 1000 a row is one value
    b everywhere but for n = max(1, C / 64) entries at b - 2 and n + 1 at b + 2 (all bf16 numbers; std s ~ 0.4), b = the number nearest 1000 s that is
    twice an odd number, and that +- 4 by row.  The uneven counts matter: with n and n both the mean and E[x^2] are fp32 numbers, and a one-pass
    variance would get away with it"""
    g = _gen(seed)
    if family == "tiny":
        return torch.randn(rows, C, generator=g) * 2.0 ** -10
    if r < 300:                             # standardised per row: 64 values realise the target too
        z = torch.randn(rows, C, generator=g)
        z -= z.mean(dim=1, keepdim=True)
        return z / z.std(dim=1, keepdim=True, unbiased=False) + float(r)
    assert r == 1000
    n = max(1, C // 64)
    s = math.sqrt(4.0 * (2 * n + 1) / C - (2.0 / C) ** 2)
    b0 = 2 * (2 * round((r * s / 2 - 1) / 2) + 1)
    assert 262 <= b0 <= 506
    x = (b0 + 4.0 * (torch.arange(rows) % 3 - 1)).view(rows, 1).repeat(1, C)
    for i in range(rows):
        p = torch.randperm(C, generator=g)
        x[i, p[:n]] -= 2.0
        x[i, p[n:2 * n + 1]] += 2.0
    return x


def ln_reference(x, gamma, beta, eps):
    xd = x.double()
    mu = xd.mean(dim=1, keepdim=True)
    v = ((xd - mu) ** 2).mean(dim=1, keepdim=True)
    s = torch.sqrt(v + float(np.float32(eps)))
    xh = (xd - mu) / s
    return dict(ref=gamma.double() * xh + beta.double(), xhat=xh, mu=mu, s=s, r=mu.abs() / s)


def ln_err_over_bound(out, x, gamma, beta, eps, k=K):
    R = ln_reference(x, gamma, beta, eps)
    bound = norm_bound(R["ref"], R["xhat"], R["r"], gamma.double().view(1, -1), False, k, es_power=1)
    assert float(bound.min()) > 0.0
    R["stat_use"] = stat_use(out, R["ref"], R["xhat"], R["r"], gamma.double().view(1, -1), False, k, es_power=1)
    return ((out.double() - R["ref"]).abs() / bound), R


def check_r(R, target, what):
    """the realised r of what the kernel is given: within 10 % of the target (|r| <= 0.1 for target 0)"""
    r = R["r"]
    lo, hi = (0.0, 0.1) if target == 0 else (0.9 * target, 1.1 * target)
    assert lo <= float(r.min()) and float(r.max()) <= hi, (what, target, float(r.min()), float(r.max()))


# ------------------------------------------------------------------------------------------------ CPU models (numpy fp32)
f32 = np.float32


def gn_model(x, gamma, beta, eps, silu, groups=GROUPS, chain=32, exact_partials=False, stats=False):
    """numpy fp32 model of GroupNorm with the summation design the bound is derived for: per channel, sequential fp32 sums (and sums of squares) over
    runs of `chain` rows -- the producers' 32-row column partials are exactly that --, everything above in fp64, then the finaliser's and the apply
    pass's fp32 arithmetic with every product and sum rounded on its own (the device may fuse them: never worse).  x: bf16 values as fp32 [B, HW, C];
    returns the UNROUNDED fp32 output [B, HW, C] (SiLU taken exactly of the fp32 z).  exact_partials: the per-run sums are fp64 sums rounded once to fp32,
    what the exact-partials tests hand to tmix_groupnorm_nhwc_pre.  stats: also the fp32 mean and rstd [B, groups]"""
    x = np.asarray(x, dtype=f32)
    B, HW, C = x.shape
    cpg = C // groups
    nb = (HW + chain - 1) // chain
    xp = np.zeros((B, nb * chain, C), f32)
    xp[:, :HW] = x
    blk = xp.reshape(B, nb, chain, C)
    a = np.zeros((B, nb, C), f32)
    q = np.zeros((B, nb, C), f32)
    for i in range(chain):
        v = blk[:, :, i]
        a = a + v
        q = q + v * v
    if exact_partials:
        b64 = blk.astype(np.float64)
        a, q = b64.sum(2).astype(f32), (b64 * b64).sum(2).astype(f32)
    n = float(HW * cpg)
    s64 = a.astype(np.float64).sum(1).reshape(B, groups, cpg).sum(2)
    q64 = q.astype(np.float64).sum(1).reshape(B, groups, cpg).sum(2)
    mean = s64 / n
    var = np.maximum(q64 / n - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(f32(eps)))).astype(f32)
    meanf = mean.astype(f32)
    g, b = np.asarray(gamma, f32).reshape(1, groups, cpg), np.asarray(beta, f32).reshape(1, groups, cpg)
    sc = rstd[:, :, None] * g
    sh = b - meanf[:, :, None] * sc
    z = x * sc.reshape(B, 1, C) + sh.reshape(B, 1, C)
    assert z.dtype == f32
    if silu:
        zd = z.astype(np.float64)
        z = (zd / (1.0 + np.exp(-zd))).astype(f32)
    return (z, meanf, rstd) if stats else z


def _lane_tree(p):
    """butterfly sum over the last axis (64 lanes) in fp32"""
    while p.shape[-1] > 1:
        h = p.shape[-1] // 2
        p = p[..., :h] + p[..., h:]
    return p[..., 0]


def ln_model(x, gamma, beta, eps):
    """numpy fp32 model of layernorm_kernel: lane l owns the 8-channel vectors l, 64 + l, ...; sequential fp32 sums per lane, a butterfly over the 64
    lanes, the variance in a second pass over (x - mean).  Unrounded fp32 output"""
    x = np.asarray(x, dtype=f32)
    rows, C = x.shape
    nvec = C // 8
    xp = np.zeros((rows, 4 * 64 * 8), f32)
    xp[:, :C] = x
    lanes = xp.reshape(rows, 4, 64, 8).transpose(0, 2, 1, 3).reshape(rows, 64, 32)
    used = (np.arange(4)[None, :, None] * 64 + np.arange(64)[:, None, None] < nvec) & np.ones((1, 1, 8), bool)
    used = used.reshape(64, 32)

    def lane_sum(v):
        acc = np.zeros((rows, 64), f32)
        for i in range(32):
            acc = acc + v[:, :, i]
        return _lane_tree(acc)
    mean = lane_sum(lanes) / f32(C)
    d = np.where(used[None], lanes - mean[:, None, None], f32(0))
    var = lane_sum(d * d) / f32(C)
    rstd = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
    y = (x - mean[:, None]) * rstd[:, None] * np.asarray(gamma, f32)[None] + np.asarray(beta, f32)[None]
    assert y.dtype == f32
    return y


def k_needed(y, R, r, gamma, silu, es_power=2):
    """the smallest k with |y - ref| <= 2^-20 |ref| + S |gamma| (|xhat| E_s(k) + E_m(k)) on every element (y unrounded: no 2^-9 term)"""
    S = 1.1 if silu else 1.0
    unit = S * gamma.abs() * (R["xhat"].abs() * (1 + r ** es_power) + (1 + r)) * U24
    over = ((torch.from_numpy(y).double() - R["ref"]).abs() - 2.0 ** -20 * R["ref"].abs()).clamp_min(0.0)
    return float((over / unit.clamp_min(1e-300)).max())


def softmax_bound(p, scale_s_absmax):
    """out_round(p) + 2 delta p + 2^-126;  delta = 4 * 2^-24 * ln2 * max_row |scale log2e S|: the fp32 error of the exponent, which hits numerator
    and denominator.  2^-126 is the smallest normal number of fp32 and bf16: exp2 of a smaller probability may flush to zero"""
    delta = 4 * U24 * math.log(2.0) * scale_s_absmax * 1.4426950408889634
    return out_round(p) + 2 * delta * p + 2.0 ** -126


# ------------------------------------------------------------------------------------------------ the finalisers' own precision
# With many partials per group the summation error averages out and what is left of E_s is what the FINALISER adds.  An all-fp32 finaliser
# (var = q / n - mean^2 rounded at every step) costs about (1 + r^2) 2^-24 there and hides under k = 5.  These cases hold the two finalisers to
#     E_s = 2^-24 + KS_FINAL (1 + r^2) 2^-24        (2^-24: rstd's own rounding to fp32; E_m as everywhere)
# with KS_FINAL twice the most that bit-faithful numpy models of the two statistics paths need (test_norm_bound_cpu.py): the fp32 additions in the device's
# order (gn_cs_walk over exact partials; gn_accum8, the LDS reduction and the per-chunk fp32 partial of gn_stats_kernel), fp64 above.
FINAL_R = (10, 30, 100)
FINAL_SHAPES = {"pre": (1, 1024, 1280, 640, True), "three": (1, 4096, 640, 320, True)}
KS_FINAL = 0.13          # the models need 0.063 (three launches, r = 100) and 0.000 (exact partials: bf16 values near r have short mantissas, their sums are exact)


def cs_walk_model(parts, HW, C1, groups=GROUPS):
    """gn_finalize_cs_kernel's sums of one image: parts = (cs1 [nblk, 2, C1], cs2 [nblk, 2, C2] or None) fp32.  Thread (j, c) of 1024 adds blocks j, j + J, ... of
    channel c in fp32, four at a time as (a0 + a1) + (a2 + a3), first over the group's channels in source 1, then in source 2; fp64 above.  -> (sum, sumsq) [groups]"""
    cs1, cs2 = parts
    C = C1 + (0 if cs2 is None else cs2.shape[2])
    cpg, nblk = C // groups, HW // 32
    out = np.zeros((groups, 2))
    for g in range(groups):
        lo, hi = g * cpg, (g + 1) * cpg
        acc = np.zeros((2, 1024), f32)
        for src, a, b in ((cs1, min(lo, C1), min(hi, C1)), (cs2, max(lo, C1) - C1, max(hi, C1) - C1)):
            n = b - a
            if n <= 0:
                continue
            J = 1024 // n
            for j in range(J):
                col = src[j::J, :, a:b]                                   # blocks j, j + J, ...: [m, 2, n]
                m4 = col.shape[0] // 4 * 4                                 # taken four at a time while four are left
                t = acc[:, j * n:(j + 1) * n]
                for i in range(0, m4, 4):
                    t += (col[i] + col[i + 1]) + (col[i + 2] + col[i + 3])
                for i in range(m4, col.shape[0]):
                    t += col[i]
        out[g] = acc.astype(np.float64).sum(1)
    return out[:, 0], out[:, 1]


def stats_kernel_model(x, groups=GROUPS):
    """gn_stats_kernel + gn_finalize_kernel's sums of one image x (fp32 [HW, C]): per chunk, lane pl of a vector column adds rows p0 + pl, p0 + pl + plane, ...
    in fp32 (runs of at most 32 rows: no flush), the group's plane * cpg sums meet in fp64 and leave as ONE fp32 partial per (chunk, group); fp64 over the chunks"""
    HW, C = x.shape
    cpg, nvec = C // groups, C // 8
    chunks = max(1, min(128, HW // 8))
    ppc = HW // chunks
    plane = 256 // nvec if nvec <= 256 else 1
    assert HW % chunks == 0 and ppc % plane == 0 and ppc // plane <= 32
    xc = x.reshape(chunks, ppc // plane, plane, C)
    a = np.zeros((chunks, plane, C), f32)
    q = np.zeros((chunks, plane, C), f32)
    for i in range(ppc // plane):
        v = xc[:, i]
        a = a + v
        q = q + v * v
    red = lambda t: t.astype(np.float64).sum(1).reshape(chunks, groups, cpg).sum(2).astype(f32).astype(np.float64).sum(0)
    return red(a), red(q)


def final_model_rstd_need(form, r, seed, fp32_finaliser=False):
    """what the model of `form` needs of KS_FINAL on the offset input at r: max over the groups of (|rstd_model / rstd_ref - 1| - 2^-24)+ / ((1 + r^2) 2^-24),
    rstd_model = fp32(1 / sqrt(var + eps)) from the model's sums with the finaliser's fp64 arithmetic -- or, fp32_finaliser, with mean, variance and rstd
    taken in fp32 from the fp64 totals: the mistake these cases are there for"""
    B, HW, C1, C2, silu = FINAL_SHAPES[form]
    C, eps = C1 + C2, 1e-5
    cpg = C // GROUPS
    x = gn_input("offset", r, 1, HW, C, seed).to(BF)
    g, b = affine(C, seed)
    R = gn_reference(x, g, b, eps, silu)
    xf = x[0].float().numpy()
    if form == "pre":
        blk = xf.astype(np.float64).reshape(HW // 32, 32, C)
        cs = np.stack([blk.sum(1), (blk * blk).sum(1)], 1).astype(f32)
        s, q = cs_walk_model((np.ascontiguousarray(cs[:, :, :C1]), np.ascontiguousarray(cs[:, :, C1:]) if C2 else None), HW, C1)
    else:
        s, q = stats_kernel_model(xf)
    n = float(HW * cpg)
    if fp32_finaliser:
        s, q, n = s.astype(f32), q.astype(f32), f32(n)
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0)
    rstd = (1 / np.sqrt(var + f32(eps))).astype(f32).astype(np.float64)
    assert var.dtype == (f32 if fp32_finaliser else np.float64)
    sref, rr = R["s"].view(-1).numpy(), R["r"].view(-1).numpy()
    return float(((np.abs(rstd * sref - 1) - U24).clip(0) / ((1 + rr ** 2) * U24)).max())
