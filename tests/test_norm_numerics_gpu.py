"""GroupNorm (all four forms), LayerNorm and the row softmax against an fp64 reference with a derived per-element bound, at non-zero means, tiny
variance and the VAE's sizes.

The other norm tests draw their input from randn (+ 0.5): |mean| / std <= 0.5, variance ~1, eps = 1e-5.  There a kernel that lost accuracy in
var = E[x^2] - mean^2, dropped eps or put it outside the square root passes.  Inputs, reference and bound live in norm_cases.py (shared with
test_norm_bound_cpu.py, which runs the CPU model the bound's constant comes from).

Reference (torch.float64, from the values the bf16 tensors hold), per (image, group) -- per row for LayerNorm:
    mu, v (biased), s = sqrt(v + eps), r = |mu| / s;   per element  xhat = (x - mu) / s,  z = gamma xhat + beta,  ref = z or silu(z).

Bound, per element, no element left out:
    |out - ref| <= h(ref) + 2^-20 |ref| + S |gamma_c| (|xhat| E_s + E_m)
    E_s = k (1 + r^2) 2^-24 (GroupNorm),  k (1 + r) 2^-24 (LayerNorm: two passes)      E_m = k (1 + r) 2^-24      S = 1.1 with SiLU (max |silu'|), else 1
  * h(ref) = half the distance between the two bf16 numbers around ref: the ONE rounding of the output.  It is 2^-9 |ref| just under a power of two
    and 2^-8 |ref| at one (bf16 has 8 significant bits), so a flat 2^-9 |ref| is missed by the correctly rounded exact result itself
    (ref = 2.0859375 lies halfway between 2.078125 and 2.09375: error 2^-7 = 1.92 * 2^-9 |ref|); h is the tightest term a correct kernel meets;
  * E_s: relative error of rstd.  var = E[x^2] - mean^2 loses r^2 times the relative error of the sums;
  * E_m: error of the mean in units of s, the fp32 rounding of shift = beta - mean * scale and of the fma;
  * k = 5 is NOT fitted to the device: the CPU model (numpy fp32, no sequential fp32 chain longer than 32 terms, fp64 above, every product and sum
    of the finaliser and the apply pass rounded on its own) needs at most 2.35 over this file's inputs (offset, r = 100); twice that, rounded up.
    The two-pass LayerNorm model needs 1.87.
The `constant` family holds 3.0 everywhere in one group: v = 0, the clamp decides; there |out - act(beta_c)| <= h + 4 * 2^-24 |mu| |gamma_c| / sqrt(eps).

Softmax: p = softmax(scale S) in fp64 from the fp32 scores over the visible columns;  |P - p| <= h(p) + p (2^-20 + 2 delta) + 2^-126,
delta = 4 * 2^-24 ln2 max_row |scale log2e S| (the fp32 error of the exponent, on numerator and denominator); 2^-126, the smallest normal number of fp32
and bf16, because exp2 of a smaller probability may flush to zero (at a logit std of 30 most of a row is below it).

Measured on an MI355X (every test prints its figures before it asserts).  The full err / bound is 0.99 .. 1.00 in every GroupNorm and LayerNorm case and
says nothing: in a large tensor some fp32 result lies halfway between two bf16 numbers, and h(ref) is exactly that.  The figure that moves is the share
of the STATISTICS term S |gamma| (|xhat| E_s + E_m) that the error beyond h(ref) + 2^-20 |ref| takes (norm_cases.stat_use; largest over a form's shapes),
by family  offset r = 0 / 3 / 10 / 30 / 100 | channel_means 10 / 100 | loud_channel | tiny eps 1e-5 / 1e-6 | large | constant (its group: share of the clamp bound):
    three launches                    0.14 / 0.04 / 0.03 / 0.00 / 0.08 | 0.02 / 0.03 | 0.10 | 0.12 / 0.05 | 0.03 | 0.10 (0.78)
    one launch                        0.05 / 0.08 / 0.09 / 0.06 / 0.08 | 0.05 / 0.00 | 0.03 | 0.02 / 0.05 | 0.05 | 0.03 (0.90)
    from exact partials               0.05 / 0.04 / 0.04 / 0.02 / 0.07 | 0.04 / 0.02 | 0.05 | 0.05 / 0.04 | 0.05 | 0.06 (0.94)
    behind conv3x3 / gemm, r = 10 / 100            0.02 / 0.03 and 0.04 / 0.02
    LayerNorm, r = 0 / 10 / 100 / 1000 | tiny      0.09 / 0.07 / 0.08 / 0.11 | 0.06
    three launches at the VAE size (1, 1048576, 128), r = 3 / 30, full err / bound:
        512-row fp32 chains in gn_stats_kernel (before)                    1.22 / 2.86     -- the CPU model of that order predicted a relative
                                                                                              variance error of 3.3e-3 at r = 30; E_s allows 5.4e-4
        flushed into fp64 every 32 rows (gn_accum8, now)                   1.00 / 0.99, statistics share 0.03 / 0.00
    softmax rows, full err / bound by (std, offset) = (1, 0) / (8, 0) / (30, 0) / (8, 1e4):  plain 1.00 / 1.00 / 1.00 / 0.45, causal 1.00 / 1.00 / 0.99 / 0.44,
        masked 1.00 / 1.00 / 0.99 / 0.45 (again the output's rounding; at offset 1e4 delta dominates the bound and the kernel uses less than half)
    finalisers at many partials (E_s = 2^-24 + 0.13 (1 + r^2) 2^-24, norm_cases.py), share of the rstd term by r = 10 / 30 / 100:
        gn_finalize_cs_kernel, 1920 exact partials per group   0.00 / 0.00 / 0.00     (models: 0.00; the sums of these bf16 values are exact in fp32)
        gn_finalize_kernel, 128 chunk partials per group       0.00 / 0.00 / 0.16     (models: up to half)
The model was pessimistic for the device everywhere but at the VAE size: it needs up to 0.47 of the statistics term, the kernels at most 0.14.
Mutations tried by hand on a scratch build, cases of this file that fail: eps dropped in gn_finalize_cs_kernel 19; the mask limit of softmax_rows_kernel
off by one 24; gn_finalize_kernel's combine, mean and variance in fp32 3; gn_finalize_cs_kernel's in fp32 3.  The last two are seen by the finaliser
cases ONLY (err / bound 1.9 .. 5.3, rstd term used 8 .. 22 times over): under k = 5 an all-fp32 finaliser takes 0.27 of the statistics term and passes.
"""
import math

import pytest
import torch

import norm_cases as N
from test_ops_gpu import BF, _colstats_ref, _mx_quantize, lib_env, ops  # noqa: F401  (lib_env, ops: fixtures)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ GroupNorm
def launches(HW, C):
    from tweediemix_amd import lib as L
    return L.load().tmix_groupnorm_nhwc_launches(HW, C, N.GROUPS)


def gn_case(fam, shape, seed):
    """x (bf16, device, [B, HW, C1 + C2]), its two sources, gamma, beta (fp32, device), eps, silu"""
    family, r, eps = fam
    B, HW, C1, C2, silu = shape
    x = N.gn_input(family, r, B, HW, C1 + C2, seed).to(BF).cuda()
    g, b = [t.cuda() for t in N.affine(C1 + C2, seed)]
    x1 = x[:, :, :C1].contiguous()
    x2 = x[:, :, C1:].contiguous() if C2 else None
    return x, x1, x2, g, b, eps, silu


def gn_check(what, fam, out, x, g, b, eps, silu):
    """print err / bound, then assert it: the realised r for the one-statistic families, the general bound on every element and, for the constant group,
    finiteness and the clamp's own bound"""
    family, r, _ = fam
    assert out.shape == x.shape and torch.isfinite(out.float()).all()
    e, R = N.gn_err_over_bound(out, x, g, b, eps, silu)
    B, HW, C = x.shape
    cpg = C // N.GROUPS
    if family in ("offset", "large"):
        N.check_r(R, r, what)
    const = None
    if family == "constant":
        lo = N.CONST_GROUP * cpg
        assert float(R["s"][:, :, N.CONST_GROUP].max()) == math.sqrt(float(torch.tensor(eps, dtype=torch.float32)))        # v = 0 exactly
        act = R["ref"][:, :, lo:lo + cpg]                                                                                # = act(beta_c): xhat = 0
        cb = N.bf16_half_spacing(act) + 4 * N.U24 * N.CONST_VALUE * g[lo:lo + cpg].double().abs() / math.sqrt(eps)
        const = float(((out[:, :, lo:lo + cpg].double() - act).abs() / cb).max())
        e[:, :, lo:lo + cpg] = 0                                                                                         # the general bound covers the other groups
    worst = float(e.max())
    rr = R["r"].flatten()
    print(f"{what} {N.fam_id(fam)}: err/bound {worst:.3f}, statistics term used {R['stat_use']:.3f}" + (f", constant group {const:.3f}" if const is not None else "")
          + f"  (realised r {float(rr.min()):.3g} .. {float(rr.max()):.3g})")
    assert worst <= 1.0, (what, fam, worst)
    assert const is None or const <= 1.0, (what, fam, const)


@pytest.mark.parametrize("fam", N.GN_FAMILIES, ids=N.fam_id)
@pytest.mark.parametrize("shape", N.GN_THREE, ids=str)
def test_groupnorm_three_launches(ops, lib_env, shape, fam):
    """gn_stats_kernel -> gn_finalize_kernel -> gn_apply_kernel; (2, 1024, 320) would run in one launch and is forced; in (1, 4096, 640 + 320) a group of 30
    channels straddles the two sources"""
    B, HW, C1, C2, _ = shape
    if launches(HW, C1 + C2) == 1:
        lib_env("TMIX_GN_NO_SMALL")
    assert launches(HW, C1 + C2) == 3
    x, x1, x2, g, b, eps, silu = gn_case(fam, shape, 1000)
    gn_check(f"three launches {shape}", fam, ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, x2=x2), x, g, b, eps, silu)


@pytest.mark.parametrize("fam", N.GN_FAMILIES, ids=N.fam_id)
@pytest.mark.parametrize("shape", N.GN_ONE, ids=str)
def test_groupnorm_one_launch(ops, shape, fam):
    """gn_small_kernel"""
    B, HW, C1, C2, _ = shape
    assert launches(HW, C1 + C2) == 1
    x, x1, x2, g, b, eps, silu = gn_case(fam, shape, 2000)
    gn_check(f"one launch {shape}", fam, ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, x2=x2), x, g, b, eps, silu)


def exact_partials(t):
    return None if t is None else _colstats_ref(t).float().contiguous()


@pytest.mark.parametrize("fam", N.GN_FAMILIES, ids=N.fam_id)
@pytest.mark.parametrize("shape", N.GN_PRE, ids=str)
def test_groupnorm_from_exact_partials(ops, shape, fam):
    """tmix_groupnorm_nhwc_pre (gn_finalize_cs_kernel) from exact 32-row column partials: fp64 sums cast to fp32"""
    x, x1, x2, g, b, eps, silu = gn_case(fam, shape, 3000)
    out = ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, x2=x2, colstats=(exact_partials(x1), exact_partials(x2)))
    gn_check(f"from partials {shape}", fam, out, x, g, b, eps, silu)


@pytest.mark.parametrize("r", [10, 100])
@pytest.mark.parametrize("producer", ["conv3x3", "gemm"])
def test_groupnorm_behind_a_producer_whose_bias_carries_the_means(ops, producer, r):
    """the column partials come from a real producer (col_stats_out) whose bias puts every group at mean +-r, output std ~1: the stored bf16 tensor itself
    has r = 10 / 100 (asserted).  The reference is of the stored tensor"""
    C = 320
    sign = torch.tensor([1.0, -1.0]).repeat(N.GROUPS // 2).repeat_interleave(C // N.GROUPS)
    bias = (sign * r).cuda()
    if producer == "conv3x3":
        B, H, W, Cin = 2, 16, 16, 64
        xin = torch.randn(B, H, W, Cin, generator=N._gen(41)).to(BF).cuda()
        w = (torch.randn(C, 3, 3, Cin, generator=N._gen(42)) * (9 * Cin) ** -0.5).to(BF).cuda()
        cs = ops.colstats_buf(B * H * W, C, "cuda")
        h = ops.conv3x3(xin, w, bias=bias, col_stats_out=cs, tile_cfg=12).view(B, H * W, C)
    else:
        B, HW, Kd = 2, 512, 128
        a = torch.randn(B * HW, Kd, generator=N._gen(43)).to(BF).cuda()
        w = (torch.randn(C, Kd, generator=N._gen(44)) * Kd ** -0.5).to(BF).cuda()
        cs = ops.colstats_buf(B * HW, C, "cuda")
        h = ops.gemm(a, w, bias=bias, col_stats_out=cs).view(B, HW, C)
    g, b = [t.cuda() for t in N.affine(C, 45)]
    eps, silu = (1e-5, True) if r == 10 else (1e-6, False)
    out = ops.groupnorm(h, g, b, N.GROUPS, eps, silu, colstats=(cs, None))
    gn_check(f"behind {producer}", ("offset", r, eps), out, h, g, b, eps, silu)


def test_groupnorm_e4m3_output_at_r_30(ops):
    """tmix_groupnorm_nhwc_pre_f8: bytes and scales equal the MX quantiser applied to what the plain form writes (which test_groupnorm_from_exact_partials holds
    to the bound at this r)"""
    fam, shape = ("offset", 30, 1e-5), (2, 256, 640, 0, True)
    x, x1, x2, g, b, eps, silu = gn_case(fam, shape, 3500)
    B, HW, C = x.shape
    cs = (exact_partials(x1), None)
    y = ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, colstats=cs)
    gn_check("from partials, before e4m3", fam, y, x, g, b, eps, silu)
    y8 = torch.full((B, HW, C), 0x5a, device="cuda", dtype=torch.uint8)
    s8 = torch.full((B * HW, C // 32), 0x5a, device="cuda", dtype=torch.uint8)
    ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, colstats=cs, f8_out=(y8, s8))
    torch.cuda.synchronize()
    q, sc, _ = _mx_quantize(y.float().view(B * HW, C))
    assert torch.equal(s8, sc.t().contiguous())
    same = (y8.view(B * HW, C) == q) | (((y8.view(B * HW, C) & 0x7f) == 0) & ((q & 0x7f) == 0))
    assert same.all(), int((~same).sum())


@pytest.mark.parametrize("r", [3, 30])
def test_groupnorm_at_the_vae_size(ops, r):
    """(1, 1048576, 128): the VAE decoder's last level at 1024^2, three launches, eps 1e-6, SiLU.  The smallest shape at which a thread of gn_stats_kernel
    owns 512 rows (HW * C / 262144, whatever the aspect).  Input made on the device; statistics in fp64 and the comparison over 16 slices of 65536 pixels"""
    HW, C, eps, SL = 1048576, 128, 1e-6, 65536
    cpg = C // N.GROUPS
    assert launches(HW, C) == 3
    gen = torch.Generator(device="cuda").manual_seed(500 + r)
    x = torch.empty(1, HW, C, device="cuda", dtype=BF)
    for i in range(0, HW, SL):
        x[0, i:i + SL] = (torch.randn(SL, C, device="cuda", generator=gen) + float(r)).to(BF)
    g, b = [t.cuda() for t in N.affine(C, 500)]
    out = ops.groupnorm(x, g, b, N.GROUPS, eps, True)
    s1 = torch.zeros(N.GROUPS, device="cuda", dtype=torch.float64)
    for i in range(0, HW, SL):
        s1 += x[0, i:i + SL].double().view(SL, N.GROUPS, cpg).sum(dim=(0, 2))
    mu = s1 / (HW * cpg)
    s2 = torch.zeros_like(s1)
    for i in range(0, HW, SL):
        s2 += ((x[0, i:i + SL].double().view(SL, N.GROUPS, cpg) - mu.view(1, -1, 1)) ** 2).sum(dim=(0, 2))
    s = torch.sqrt(s2 / (HW * cpg) + float(torch.tensor(eps, dtype=torch.float32)))
    rr = mu.abs() / s
    assert 0.9 * r <= float(rr.min()) and float(rr.max()) <= 1.1 * r, (float(rr.min()), float(rr.max()))
    gd, bd = g.double().view(1, N.GROUPS, cpg), b.double().view(1, N.GROUPS, cpg)
    worst = used = 0.0
    for i in range(0, HW, SL):
        xh = (x[0, i:i + SL].double().view(SL, N.GROUPS, cpg) - mu.view(1, -1, 1)) / s.view(1, -1, 1)
        z = gd * xh + bd
        ref = z * torch.sigmoid(z)
        bound = N.norm_bound(ref, xh, rr.view(1, -1, 1), gd, True)
        o = out[0, i:i + SL]
        assert torch.isfinite(o.float()).all()
        o = o.view(SL, N.GROUPS, cpg)
        worst = max(worst, float(((o.double() - ref).abs() / bound).max()))
        used = max(used, N.stat_use(o, ref, xh, rr.view(1, -1, 1), gd, True))
    print(f"three launches at the VAE size (1, {HW}, {C}) r = {r}: err/bound {worst:.3f}, statistics term used {used:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("r", N.FINAL_R)
@pytest.mark.parametrize("form", ["pre", "three"])
def test_groupnorm_finalisers_add_nothing_at_many_partials(ops, form, r):
    """gn_finalize_cs_kernel (1920 exact partials per group) and gn_finalize_kernel (128 chunk partials per group) at r = 10 / 30 / 100, held to
    E_s = 2^-24 + KS_FINAL (1 + r^2) 2^-24 (norm_cases.py): with that many partials the summation error averages out and a finaliser that took the mean,
    the variance or the combine in fp32 would stand out -- under k = 5 it hides.  KS_FINAL comes from bit-faithful models of the two paths"""
    shape = N.FINAL_SHAPES[form]
    B, HW, C1, C2, silu = shape
    fam = ("offset", r, 1e-5)
    x, x1, x2, g, b, eps, silu = gn_case(fam, shape, 7000)
    if form == "pre":
        out = ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, x2=x2, colstats=(exact_partials(x1), exact_partials(x2)))
    else:
        assert launches(HW, C1 + C2) == 3
        out = ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, x2=x2)
    assert torch.isfinite(out.float()).all()
    R = N.gn_reference(x, g, b, eps, silu)
    N.check_r(R, r, (form, shape))
    C = C1 + C2
    rr = R["r"].expand(B, 1, N.GROUPS, C // N.GROUPS).reshape(B, 1, C)
    gd = g.double().view(1, 1, C)
    err = (out.double() - R["ref"]).abs()
    bound = N.norm_bound(R["ref"], R["xhat"], rr, gd, silu, ks_final=N.KS_FINAL)
    # the share of the rstd term that the error beyond the output's rounding and E_m takes
    rest = (err - (N.norm_bound(R["ref"], R["xhat"], rr, gd, silu, ks_final=0.0) - 1.1 * gd.abs() * R["xhat"].abs() * N.U24)).clamp_min(0.0)
    used = float((rest / (1.1 * gd.abs() * R["xhat"].abs() * (1 + N.KS_FINAL * (1 + rr ** 2)) * N.U24).clamp_min(1e-300)).max())
    worst = float((err / bound).max())
    print(f"finaliser of {form} {shape} r = {r}: err/bound {worst:.3f}, rstd term used {used:.3f}")
    assert worst <= 1.0, (form, r, worst)


@pytest.mark.parametrize("form", ["three", "one", "pre", "pre_f8"])
def test_groupnorm_image_bits_do_not_depend_on_the_batch(ops, lib_env, form):
    """out[:1] of a batched call is bit-equal to the call on the first image alone, on an offset input (r = 10); for the e4m3 form, bytes and scales"""
    shape = {"three": N.GN_THREE[0], "one": N.GN_ONE[0], "pre": N.GN_PRE[0], "pre_f8": N.GN_PRE[0]}[form]
    B, HW, C1, C2, _ = shape
    assert B > 1
    if form == "three":
        lib_env("TMIX_GN_NO_SMALL")
    assert form in ("pre", "pre_f8") or launches(HW, C1) == (1 if form == "one" else 3)
    x, x1, x2, g, b, eps, silu = gn_case(("offset", 10, 1e-5), shape, 4000)
    if form == "pre_f8":
        def f8(t):
            y8 = torch.full(t.shape, 0x5a, device="cuda", dtype=torch.uint8)
            s8 = torch.full((t.shape[0] * HW, C1 // 32), 0x5a, device="cuda", dtype=torch.uint8)
            ops.groupnorm(t, g, b, N.GROUPS, eps, silu, colstats=(exact_partials(t), None), f8_out=(y8, s8))
            torch.cuda.synchronize()
            return y8, s8
        (y8, s8), (y8a, s8a) = f8(x1), f8(x1[:1].contiguous())
        assert torch.equal(y8[:1], y8a) and torch.equal(s8[:HW], s8a)
        return
    cs = (lambda t: (exact_partials(t), None)) if form == "pre" else (lambda t: None)
    y = ops.groupnorm(x1, g, b, N.GROUPS, eps, silu, colstats=cs(x1))
    first = x1[:1].contiguous()
    assert torch.equal(ops.groupnorm(first, g, b, N.GROUPS, eps, silu, colstats=cs(first)), y[:1])


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("fam", N.LN_FAMILIES, ids=N.fam_id)
@pytest.mark.parametrize("rows,C", N.LN_SHAPES)
def test_layernorm(ops, rows, C, fam):
    """tmix_layernorm keeps the row in registers and takes the variance in a second pass: E_s is LINEAR in r.  A one-pass rewrite misses this at r = 1000
    (test_norm_bound_cpu.py shows it on the model)"""
    family, r, eps = fam
    x = N.ln_input(family, r, rows, C, 5000).to(BF).cuda()
    g, b = [t.cuda() for t in N.affine(C, 5000)]
    out = ops.layernorm(x, g, b, eps)
    assert torch.isfinite(out.float()).all()
    e, R = N.ln_err_over_bound(out, x, g, b, eps)
    if family == "offset":
        N.check_r(R, r, (rows, C))
    print(f"layernorm ({rows}, {C}) {N.fam_id(fam)}: err/bound {float(e.max()):.3f}, statistics term used {R['stat_use']:.3f}  (realised r {float(R['r'].min()):.4g} .. {float(R['r'].max()):.4g})")
    assert float(e.max()) <= 1.0, float(e.max())


# ------------------------------------------------------------------------------------------------ row softmax
SCALE = 0.125
NAN, INF = float("nan"), float("inf")


def scores(rows, cols, std, offset, seed):
    """fp32 [rows, cols] (CPU) with scale * S of per-row std `std` (standardised per row, asserted) about `offset`"""
    z = torch.randn(rows, cols, generator=N._gen(seed), dtype=torch.float64)
    if cols > 1:
        z = (z - z.mean(dim=1, keepdim=True)) / z.std(dim=1, keepdim=True, unbiased=False)
    S = ((z * std + offset) / SCALE).float()
    got = (SCALE * S.double()).std(dim=1, unbiased=False)
    assert cols == 1 or (0.9 * std <= float(got.min()) and float(got.max()) <= 1.1 * std), (std, float(got.min()), float(got.max()))
    return S


def run_softmax(kind, S, arg, ld_s=None, ld_p=None):
    """launch tmix_softmax_rows / _causal / _masked on S (CPU fp32 [rows, cols]) with leading dimensions ld_s, ld_p >= cols: NaN behind the columns of S, the
    guard value 3.0 behind those of P (asserted untouched).  Returns P [rows, cols] (bf16, device)"""
    from tweediemix_amd import lib as L
    lib = L.load()
    rows, cols = S.shape
    ld_s, ld_p = ld_s or cols, ld_p or cols
    Sb = torch.full((rows, ld_s), NAN, device="cuda", dtype=torch.float32)
    Sb[:, :cols] = S.cuda()
    Pb = torch.full((rows, ld_p), 3.0, device="cuda", dtype=BF)
    st = torch.cuda.current_stream().cuda_stream
    if kind == "plain":
        L.check(lib.tmix_softmax_rows(Sb.data_ptr(), ld_s, Pb.data_ptr(), ld_p, rows, cols, SCALE, st), "tmix_softmax_rows")
    elif kind == "causal":
        L.check(lib.tmix_softmax_rows_causal(Sb.data_ptr(), ld_s, Pb.data_ptr(), ld_p, rows, cols, SCALE, arg, st), "tmix_softmax_rows_causal")
    else:
        L.check(lib.tmix_softmax_rows_masked(Sb.data_ptr(), ld_s, Pb.data_ptr(), ld_p, rows, cols, arg, SCALE, st), "tmix_softmax_rows_masked")
    torch.cuda.synchronize()
    assert (Pb[:, cols:] == 3.0).all()
    return Pb[:, :cols]


def softmax_check(what, P, S, visible):
    """visible: bool [rows, cols].  Hidden columns are exactly 0; the visible ones obey the bound"""
    S, visible = S.cuda(), visible.cuda()
    assert torch.isfinite(P.float()).all()
    assert (P[~visible] == 0).all()
    x = torch.where(visible, SCALE * S.double(), torch.full_like(S, -INF, dtype=torch.float64))
    p = torch.softmax(x, dim=1)
    amax = torch.where(visible, SCALE * S.double(), torch.zeros_like(x)).abs().amax(dim=1, keepdim=True)
    e = ((P.double() - p).abs() / N.softmax_bound(p, amax))[visible]
    print(f"{what}: err/bound {float(e.max()):.3f}")
    assert float(e.max()) <= 1.0, (what, float(e.max()))


SM_SETS = [(1, 0.0), (8, 0.0), (30, 0.0), (8, 1e4)]          # (per-row std of scale * S, common offset: the max subtraction)


@pytest.mark.parametrize("std,offset", SM_SETS)
@pytest.mark.parametrize("rows,cols,ld_s,ld_p", [(8, 16384, None, None), (3, 1028, 1032, None), (3, 1028, None, 1040), (5, 4, None, None)])
def test_softmax_rows(ops, rows, cols, ld_s, ld_p, std, offset):
    """tmix_softmax_rows at the VAE's 16384 columns, at one full pass of 1024 columns plus a 4-column tail and at 4 columns"""
    S = scores(rows, cols, std, offset, 6000 + cols)
    P = run_softmax("plain", S, None, ld_s, ld_p)
    softmax_check(f"softmax_rows ({rows}, {cols}) std {std} offset {offset:g}", P, S, torch.ones(rows, cols, dtype=torch.bool))


@pytest.mark.parametrize("std,offset", SM_SETS)
@pytest.mark.parametrize("rows,cols,seq,ld_s,ld_p", [(2 * 77, 80, 77, None, None), (2 * 77, 80, 77, 96, 88), (3 * 8, 8, 8, None, None)])
def test_softmax_rows_causal(ops, rows, cols, seq, ld_s, ld_p, std, offset):
    """row i sees columns <= i % seq; the rest, the padding columns 77..79 included, are exactly 0 and row 0 of every block is exactly [1, 0, ...]"""
    S = scores(rows, cols, std, offset, 6100 + cols)
    P = run_softmax("causal", S, seq, ld_s, ld_p)
    visible = torch.arange(cols).view(1, cols) <= (torch.arange(rows) % seq).view(rows, 1)
    first = P[::seq].float()
    assert (first[:, 0] == 1).all() and (first[:, 1:] == 0).all()
    softmax_check(f"softmax_rows_causal ({rows}, {cols}, seq {seq}) std {std} offset {offset:g}", P, S, visible)


@pytest.mark.parametrize("std,offset", SM_SETS)
@pytest.mark.parametrize("rows,cols,valid,ld_s,ld_p", [(260, 320, 257, None, None), (260, 320, 257, 324, 328), (4, 8, 1, None, None)])
def test_softmax_rows_masked(ops, rows, cols, valid, ld_s, ld_p, std, offset):
    """columns >= valid are exactly 0 although S holds +inf and NaN there"""
    S = scores(rows, cols, std, offset, 6200 + cols)
    S[:, valid::2] = INF
    S[:, valid + 1::2] = NAN
    P = run_softmax("masked", S, valid, ld_s, ld_p)
    visible = (torch.arange(cols) < valid).view(1, cols).expand(rows, cols)
    softmax_check(f"softmax_rows_masked ({rows}, {cols}, valid {valid}) std {std} offset {offset:g}", P, S, visible)


def test_softmax_rows_shape_rules(ops):
    """every TMIX_ESHAPE rule of softmax_entry is refused with TmixError"""
    from tweediemix_amd.lib import TmixError
    S = torch.zeros(16, 16)
    bad = [("plain", S[:, :6], None, {}),                   # cols % 4
           ("plain", S[:, :8], None, {"ld_s": 10}),         # ld_s % 4
           ("plain", S[:, :8], None, {"ld_p": 10}),         # ld_p % 4
           ("causal", S[:, :8], 16, {}),                    # seq > cols
           ("causal", S[:12], 8, {}),                       # rows % seq
           ("causal", S, 0, {}),                            # seq < 1
           ("causal", S[:, :6], 2, {}),                     # cols % 4
           ("masked", S, 0, {}),                            # valid < 1
           ("masked", S, 17, {}),                           # valid > cols
           ("masked", S[:, :6], 2, {})]                     # cols % 4
    for kind, s, arg, ld in bad:
        with pytest.raises(TmixError):
            run_softmax(kind, s.contiguous(), arg, **ld)
    run_softmax("causal", S, 16, ld_s=20, ld_p=24)            # the limits themselves pass: seq == cols, valid == cols, valid == 1
    run_softmax("masked", S, 16)
    run_softmax("masked", S, 1)
