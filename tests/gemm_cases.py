"""Inputs, fp64 references, the per-element bound and the checker shared by test_gemm_numerics_gpu.py (the GEMM / convolution kernels) and
test_gemm_cases_cpu.py (a numpy model of the pipeline and its mutations: the checker's teeth, shown without a GPU).  No HIP here.

EXACT family.  Operands whose every product and every partial sum, in ANY order, is an fp32 number: integers in [-8, 8] (about half of them zero, drawn, so
periodic in nothing), optionally times power-of-two gains 2^[-3, 3] per A row and per W row; integer fp32 bias / row-group bias / time-embedding rows;
integer bf16 residual, |r| <= 256; e4m3 bytes of the same integers with E8M0 scales 2^[-3, 3] per row or, MX form, per 32-block (the e4m3 convolution: 2^[-2, 2] per
block of a pixel, which keeps the share of exact ties above 1 %).  Every builder ASSERTS
the precondition in fp64 -- sum |terms| / unit < 2^24 per output element, unit = the smallest power of two every term is a multiple of -- and that the
expected output exercises the rounding (>= 1 % exact ties, >= 30 % inexact in bf16).  A correct kernel then returns THE bits: the fp64 result for an
fp32 output, the fp64 result rounded once (RNE) for a bf16 one, whatever its tiling, ring depth, split-K or MFMA shape.

STRUCTURED family.  bf16 / e4m3 values drawn once (gauss, loud_k, quiet_rows, offset, loud_out), reference in torch.float64 from the values the tensors
hold, and per element, with S = sum_k |a_ik w_jk| + |bias| + |temb| + |rgb| + |res| (fp64) and n the number of terms:
    T = 2 n 2^-24 S      any-order fp32 summation costs (n - 1) 2^-24 S under RNE; the 2 because an MFMA's internal rounding is not documented as RNE
    bf16 output: |out - ref| <= T + half the bf16 spacing at (|ref| + T)            fp32 output: |out - ref| <= T + 2^-24 |ref|
    GELU / GEGLU, out = v gelu(g) with v, g bounded by Tv, Tg:  |gelu(g)| Tv + GELU_SLOPE (|v| + Tv) Tg + (1e-5 + 2^-24) |v gelu(g)| in place of T
        (1e-5: what test_gelu_epilogue_is_the_exact_erf_form_also_in_the_tail grants the function; GELU_SLOPE = 1.13 >= max |gelu'| = 1.1289; 2^-24: the product)
    folded LayerNorm, out = rstd (acc - mean colsum) + t:  T of the raw accumulation times rstd, plus norm_cases' statistics term carried through the
        product, sum_k |W'_jk| (|xhat_ik| E_s + E_m) with E_s = k (1 + r^2) 2^-24 (one-pass variance, gemm_kernel.h ln_reduce), E_m = k (1 + r) 2^-24, k = norm_cases.K
No global atol, no constant fitted to a device.
"""
import numpy as np
import torch

import norm_cases as NC

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
U24 = 2.0 ** -24
GELU_SLOPE = 1.13
STRUCTURED = ("gauss", "loud_k", "quiet_rows", "offset", "loud_out")
LOUD_OUT_ROWS = (1, 2, 3)          # (taken modulo N) W rows x 100 in `loud_out`
S1, S2, UP2, T3 = 0, 1, 2, 3       # convolution modes (tweediemix_amd.lib.CONV_*)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ references
def conv_taps(x, mode, border="zero"):
    """the taps of a 3x3 (T3: 3x1x1) convolution as a list of tensors [B, Ho, Wo, Cin], tap-major as the OHWI weights are; x [B, H, W, Cin] (T3: [clips, frames,
    hw, Cin]).  border "clamp": the out-of-image taps read the nearest pixel instead of zero (the mutation of test_gemm_cases_cpu.py)"""
    if mode == T3:
        F = x.shape[1]
        xp = torch.cat([x[:, :1] if border == "clamp" else torch.zeros_like(x[:, :1]), x, x[:, -1:] if border == "clamp" else torch.zeros_like(x[:, :1])], 1)
        return [xp[:, k:k + F] for k in range(3)]
    if mode == UP2:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, C = x.shape
    if border == "clamp":
        xp = torch.cat([x[:, :1], x, x[:, -1:]], 1)
        xp = torch.cat([xp[:, :, :1], xp, xp[:, :, -1:]], 2)
    else:
        xp = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype, device=x.device)
        xp[:, 1:-1, 1:-1] = x
    if mode == S2:
        return [xp[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)]
    return [xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]


def conv_product(x, w, mode, border="zero"):
    """sum over taps and channels in the dtype of x (fp64 for references): x as in conv_taps, w [Cout, 3, 3, Cin] (T3: [Cout, 3, Cin]) -> [B, Ho, Wo, Cout]"""
    wt = w.reshape(w.shape[0], -1, w.shape[-1])
    out = None
    for t, xt in enumerate(conv_taps(x, mode, border)):
        y = xt @ wt[:, t].T
        out = y if out is None else out + y
    return out


def im2col(x, mode, border="zero"):
    """[B * Ho * Wo, taps * Cin]: the convolution as the GEMM the kernels run (test_gemm_cases_cpu.py feeds it to the numpy model)"""
    taps = conv_taps(x, mode, border)
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in taps], 1)


def gelu64(x):
    return x * 0.5 * torch.erfc(-x / 2 ** 0.5)


# ------------------------------------------------------------------------------------------------ exact family
def ints(shape, seed, pos=0.8):
    """fp64 integers in [-8, 8]: half of them zero, the others 1 .. 8 with sign + at probability pos (a mean, so that the sums reach the hundreds)"""
    g = _gen(seed)
    mag = torch.randint(1, 9, shape, generator=g)
    keep = torch.rand(shape, generator=g) < 0.5
    sgn = torch.where(torch.rand(shape, generator=g) < pos, 1, -1)
    return (mag * keep * sgn).double()


def signs(n, seed):
    return torch.where(torch.rand(n, generator=_gen(seed)) < 0.5, -1.0, 1.0).double()


def exps(shape, seed):
    """integers in [-3, 3]"""
    return torch.randint(-3, 4, shape, generator=_gen(seed))


def int_rows(shape, seed, amp):
    """integer-valued fp64 in [-amp, amp]"""
    return torch.randint(-amp, amp + 1, shape, generator=_gen(seed)).double()


def rounding_share(ref):
    """(share of exact ties, share of inexact elements) of ref (fp64 holding fp32 numbers) under the rounding to bf16"""
    bits = ref.float().view(torch.int32) & 0xffff
    return float((bits == 0x8000).double().mean()), float((bits != 0).double().mean())


def expected(ref, S, unit, what, rounding=True):
    """the precondition and the expected outputs of an exact case: ref, S = sum |terms|, unit (fp64, same shape).  -> (bf16, fp32)"""
    assert float((S / unit).max()) < 2.0 ** 24, (what, float((S / unit).max()))
    q = ref / unit
    assert bool((q == q.round()).all()), what                 # every result is a multiple of its unit ...
    f32 = ref.float()
    assert bool((f32.double() == ref).all()), what             # ... and so an fp32 number
    if rounding:
        ties, inexact = rounding_share(ref)
        assert ties >= 0.01 and inexact >= 0.30, (what, ties, inexact)
    return f32.to(BF), f32


def _bf(t, what):
    b = t.to(BF)
    assert bool((b.double() == t).all()), what
    return b


def default_pos(K, additive):
    """the share of + signs among the non-zero integers: all of them where a short K alone has to carry the sums past 256 (integers below are bf16 numbers)"""
    return 1.0 if K <= 128 and not additive else 0.8


def exact_gemm(M, N, K, seed, batch=1, wsets=1, gains=False, bias=False, rgb_rows=0, residual=False, pos=None, rounding=True):
    """a bf16 [batch, M, K], w bf16 [wsets, N, K] (slice b reads set b % wsets), bias fp32 [wsets, N], rgb fp32 [ceil(M / rgb_rows), N] (batch 1), res bf16
    [batch, M, N], ref fp64, exp_bf16, exp_f32.  Every W row carries a sign of its own, so the outputs have both"""
    what = f"exact_gemm {M}x{N}x{K} seed {seed}"
    pos = default_pos(K, bias or rgb_rows or residual) if pos is None else pos
    a = ints((batch, M, K), seed, pos)
    w = ints((wsets, N, K), seed + 1, pos) * signs(wsets * N, seed + 2).view(wsets, N, 1)
    unit = torch.ones(batch, M, N, dtype=torch.float64)
    sets = torch.arange(batch) % wsets
    if gains:
        gr, gc = 2.0 ** exps((batch, M, 1), seed + 3).double(), 2.0 ** exps((wsets, N, 1), seed + 4).double()
        a, w = a * gr, w * gc
        unit = gr * gc[sets].transpose(1, 2)
    ws = w[sets]
    ref = a @ ws.transpose(1, 2)
    S = a.abs() @ ws.abs().transpose(1, 2)
    c = dict(a=_bf(a, what), w=_bf(w, what), bias=None, rgb=None, res=None, rgb_rows=rgb_rows)
    if bias:
        b = int_rows((wsets, N), seed + 5, 600)
        ref, S, c["bias"] = ref + b[sets][:, None], S + b[sets][:, None].abs(), b.float()
    if rgb_rows:
        assert batch == 1
        r = int_rows(((M + rgb_rows - 1) // rgb_rows, N), seed + 6, 300)
        rr = r.repeat_interleave(rgb_rows, 0)[:M]
        ref, S, c["rgb"] = ref + rr, S + rr.abs(), r.float()
    if residual:
        r = int_rows((batch, M, N), seed + 7, 256)
        ref, S, c["res"] = ref + r, S + r.abs(), _bf(r, what)
    if bias or rgb_rows or residual:
        unit = unit.clamp_max(1.0)
    c["ref"] = ref
    c["exp_bf16"], c["exp_f32"] = expected(ref, S, unit, what, rounding)
    return c


def e4m3_bytes(v, what):
    q = v.float().to(F8)
    assert bool((q.double() == v).all()), what
    return q.view(torch.uint8)


def mx_exps(K, M):
    """block exponents [K / 32, M] in [-3, 3]: (m + 3 blk) mod 7 - 3, so neighbouring blocks of a row never share one"""
    return (torch.arange(M).view(1, M) + 3 * torch.arange(K // 32).view(-1, 1)) % 7 - 3


def exact_gemm_fp8(M, N, K, seed, mx=False, bias=False, residual=False, pos=0.8):
    """a8 / w8 uint8 e4m3 bytes, sa uint8 [M] ([K / 32, M] with mx), sw uint8 [N]; ad / wd the fp64 values they stand for"""
    what = f"exact_gemm_fp8 {M}x{N}x{K} seed {seed} mx {mx}"
    a = ints((M, K), seed, pos)
    w = ints((N, K), seed + 1, pos) * signs(N, seed + 2).view(N, 1)
    ew = exps((N,), seed + 4)
    if mx:
        ea = mx_exps(K, M)
        ad = (a.view(M, K // 32, 32) * (2.0 ** ea.double()).t().unsqueeze(2)).view(M, K)
        emin = ea.min(0).values
    else:
        ea = exps((M,), seed + 3)
        ad = a * (2.0 ** ea.double()).view(M, 1)
        emin = ea
    wd = w * (2.0 ** ew.double()).view(N, 1)
    unit = 2.0 ** (emin.view(M, 1) + ew.view(1, N)).double()
    ref, S = ad @ wd.T, ad.abs() @ wd.abs().T
    c = dict(a8=e4m3_bytes(a, what), w8=e4m3_bytes(w, what), sa=(ea + 127).to(torch.uint8).contiguous(), sw=(ew + 127).to(torch.uint8), ad=ad, wd=wd,
             bias=None, res=None)
    if bias:
        b = int_rows((N,), seed + 5, 600)
        ref, S, c["bias"] = ref + b, S + b.abs(), b.float()
    if residual:
        r = int_rows((M, N), seed + 7, 256)
        ref, S, c["res"] = ref + r, S + r.abs(), _bf(r, what)
    if bias or residual:
        unit = unit.clamp_max(1.0)
    c["ref"] = ref
    c["exp_bf16"], c["exp_f32"] = expected(ref, S, unit, what)
    return c


def exact_conv(B, H, W, Cin, Cout, mode, seed, bias=True, temb=True, residual=True, gains=True, shortcut=0, pos=0.8, fp8=False):
    """x bf16 [B, H, W, Cin], w bf16 OHWI ([Cout, 3, Cin] for T3, where x is [clips, frames, hw, Cin] = [B, H, W, Cin]), bias fp32 [Cout], temb fp32 [B, Cout], res
    bf16 [B, Ho, Wo, Cout]; shortcut = c1 > 0: s1 bf16 [B, H, W, c1] and wsc bf16 [Cout, c1] ride behind the taps.  fp8: x8 / w8 bytes, sx uint8 [B H W, Cin / 32]
    (row-major MX blocks), sw uint8 [Cout] as tmix_conv3x3_nhwc_fp8 reads them"""
    what = f"exact_conv {(B, H, W, Cin, Cout)} mode {mode} seed {seed}"
    x = ints((B, H, W, Cin), seed, pos)
    w = ints((Cout, 3, Cin) if mode == T3 else (Cout, 3, 3, Cin), seed + 1, pos)
    w = w * signs(Cout, seed + 2).view(Cout, *([1] * (w.dim() - 1)))
    unit = torch.ones(Cout, dtype=torch.float64)
    c = dict(bias=None, temb=None, res=None, s1=None, wsc=None)
    if fp8:
        c["x8"], c["w8"] = e4m3_bytes(x, what), e4m3_bytes(w, what)
        ex = (torch.arange(B * H * W).view(-1, 1) + 2 * torch.arange(Cin // 32).view(1, -1)) % 5 - 2         # [pixels, Cin / 32] in [-2, 2], neighbours differ
        ew = exps((Cout,), seed + 4)
        c["sx"], c["sw"] = (ex + 127).to(torch.uint8).contiguous(), (ew + 127).to(torch.uint8)
        x = (x.view(-1, Cin // 32, 32) * (2.0 ** ex.double()).unsqueeze(2)).view(B, H, W, Cin)
        w = w * (2.0 ** ew.double()).view(Cout, 1, 1, 1)
        unit = 2.0 ** (ew - 2).double()
    elif gains:
        gc = 2.0 ** exps((Cout,), seed + 4).double()
        w = w * gc.view(Cout, *([1] * (w.dim() - 1)))
        unit = gc
    if not fp8:
        c["x"], c["w"] = _bf(x, what), _bf(w, what)
    ref, S = conv_product(x, w, mode), conv_product(x.abs(), w.abs(), mode)
    if shortcut:
        s1 = ints((B, H, W, shortcut), seed + 8, pos)
        wsc = ints((Cout, shortcut), seed + 9, pos) * (signs(Cout, seed + 2) * unit).view(Cout, 1)        # (the sign and gain of its W row)
        ref, S = ref + s1 @ wsc.T, S + s1.abs() @ wsc.abs().T
        c["s1"], c["wsc"] = _bf(s1, what), _bf(wsc, what)
    if bias:
        b = int_rows((Cout,), seed + 5, 600)
        ref, S, c["bias"] = ref + b, S + b.abs(), b.float()
    if temb:
        t = int_rows((B, Cout), seed + 6, 300)
        ref, S, c["temb"] = ref + t[:, None, None], S + t[:, None, None].abs(), t.float()
    if residual:
        r = int_rows(tuple(ref.shape), seed + 7, 256)
        ref, S, c["res"] = ref + r, S + r.abs(), _bf(r, what)
    if bias or temb or residual:
        unit = unit.clamp_max(1.0)
    c["ref"] = ref
    c["exp_bf16"], c["exp_f32"] = expected(ref, S, unit.expand_as(ref), what)
    return c


def exact_conv_in(B, Cin, H, W, Cout, seed, pre=False):
    """conv_in: x fp32 NCHW, w fp32 OHWI, bias fp32, bf16 NHWC output.  fp32 operands: the same integers, a bias in the hundreds carries the sums across 256.
    pre (tmix_conv_in_pre, Cin = 4): an integer 4 x 4 map pre_w in [-2, 2] and a non-zero integer pre_b in +-[1, 3] applied to every pixel of x BEFORE the zero
    padding -- a bias that leaks into the border changes integers --; S then sums |pre_b| + |pre_w| |x| through |w|, which bounds every partial sum of the map's
    own chain too"""
    what = f"exact_conv_in {(B, Cin, H, W, Cout)}{' pre' if pre else ''}"
    x = ints((B, H, W, Cin), seed, 0.8)
    w = ints((Cout, 3, 3, Cin), seed + 1, 0.8) * signs(Cout, seed + 2).view(Cout, 1, 1, 1)
    b = int_rows((Cout,), seed + 5, 600)
    c, u, ua = {}, x, x.abs()
    if pre:
        assert Cin == 4
        pw = int_rows((4, 4), seed + 6, 2)
        pb = int_rows((4,), seed + 7, 3)
        pb = torch.where(pb == 0, signs(4, seed + 8), pb)                      # (no channel without a bias)
        u, ua = x @ pw.T + pb, x.abs() @ pw.abs().T + pb.abs()
        c = dict(pre_w=pw.float(), pre_b=pb.float())
    ref, S = conv_product(u, w, S1) + b, conv_product(ua, w.abs(), S1) + b.abs()
    e, _ = expected(ref, S, torch.ones_like(ref), what)
    return dict(c, x=x.permute(0, 3, 1, 2).contiguous().float(), w=w.float(), bias=b.float(), ref=ref, exp_bf16=e)


def exact_conv_out(B, H, W, Cin, Cout, seed):
    """conv_out: x bf16 NHWC, w bf16 OHWI, bias fp32, fp32 NCHW output (no rounding to exercise: the fp64 result itself)"""
    what = f"exact_conv_out {(B, H, W, Cin, Cout)}"
    x = ints((B, H, W, Cin), seed, 0.8)
    gc = 2.0 ** exps((Cout,), seed + 4).double()
    w = ints((Cout, 3, 3, Cin), seed + 1, 0.8) * (signs(Cout, seed + 2) * gc).view(Cout, 1, 1, 1)
    b = int_rows((Cout,), seed + 5, 600)
    ref, S = conv_product(x, w, S1) + b, conv_product(x.abs(), w.abs(), S1) + b.abs()
    _, e = expected(ref, S, gc.clamp_max(1.0).expand_as(ref), what, rounding=False)
    return dict(x=_bf(x, what), w=_bf(w, what), bias=b.float(), ref=ref, exp_f32=e.permute(0, 3, 1, 2).contiguous())


# ------------------------------------------------------------------------------------------------ structured family
def quantize_rows(x, block=None):
    """fp32 [rows, K] -> (e4m3 bytes [rows, K], E8M0 bytes [rows] or, block = 32: [K / 32, rows] (the MX form), the fp32 values the pair holds).  The scale of a row
    (block) is a power of two that brings its largest magnitude under 448; all-zero ones keep 2^0"""
    rows, K = x.shape
    xb = x.view(rows, 1 if block is None else K // block, -1)
    _, e = torch.frexp(xb.abs().amax(2) / 448.0)
    e = torch.where(xb.abs().amax(2) > 0, e, torch.zeros_like(e)).clamp(-127, 127)
    q = (xb * torch.exp2(-e.float()).unsqueeze(2)).to(F8)
    val = (q.float() * torch.exp2(e.float()).unsqueeze(2)).view(rows, K)
    assert bool(torch.isfinite(val).all())
    sc = (e + 127).to(torch.uint8)
    return q.view(torch.uint8).view(rows, K).contiguous(), (sc[:, 0] if block is None else sc.t()).contiguous(), val


def structured_operands(family, M, N, K, seed, dtype=BF, full=False):
    """(a [M, K], w [N, K]) fp32 values of `dtype`: bf16 numbers, or (F8) what e4m3 bytes with MX block scales on A and one scale per W row hold.
    full (F8): (a8, sa [K / 32, M], a, w8, sw [N], w) instead"""
    assert family in STRUCTURED, family
    a = torch.randn(M, K, generator=_gen(seed))
    w = torch.randn(N, K, generator=_gen(seed + 1)) * K ** -0.5
    if family == "loud_k":
        a[:, 64:96] *= 64.0
    elif family == "quiet_rows":
        a *= (2.0 ** ((torch.arange(M) % 25) - 12).float()).view(M, 1)
    elif family == "offset":                 # columns of W in +- pairs: the offset's share of the product cancels, S >> |ref|
        a += 3.0
        w[:, 1::2] = -w[:, 0::2]
    elif family == "loud_out":
        for j in LOUD_OUT_ROWS:
            w[j % N] *= 100.0
    if dtype == F8:
        a8, sa, av = quantize_rows(a, 32)
        w8, sw, wv = quantize_rows(w)
        return (a8, sa, av, w8, sw, wv) if full else (av, wv)
    return a.to(dtype).float(), w.to(dtype).float()


def half_spacing(v):
    """half the distance between the two bf16 numbers around |v| (norm_cases.bf16_half_spacing): what ONE rounding to bf16 can cost"""
    return NC.bf16_half_spacing(v)


def out_term(ref, T, out_dtype):
    """T plus the output's own rounding"""
    return T + (half_spacing(ref.abs() + T) if out_dtype == BF else U24 * ref.abs())


def gemm_bound(ref, S, n, out_dtype=BF):
    return out_term(ref, 2.0 * n * U24 * S, out_dtype)


def gelu_bound(v, g, Tv, Tg, out_dtype=BF):
    """out = v gelu(g) (GEGLU; act='gelu' is v = 1, Tv = 0)"""
    ref = v * gelu64(g)
    T = gelu64(g).abs() * Tv + GELU_SLOPE * (v.abs() + Tv) * Tg + (1e-5 + U24) * ref.abs()
    return ref, out_term(ref, T, out_dtype)


def ln_fold_reference(h, wp, t, eps):
    """fp64 reference and bound of the folded LayerNorm GEMM from the values h (bf16 [M, K]), W' (bf16 [N, K]) and t (fp32 [N]) hold"""
    R = NC.ln_reference(h, torch.ones(h.shape[1], dtype=torch.float64, device=h.device), torch.zeros(h.shape[1], dtype=torch.float64, device=h.device), eps)
    wd, hd = wp.double(), h.double()
    ref = R["xhat"] @ wd.T + t.double()
    K = h.shape[1]
    rstd = 1.0 / R["s"]
    S = hd.abs() @ wd.abs().T + R["mu"].abs() * wd.sum(1).abs().view(1, -1)            # the raw accumulation and the rank-1 term -mean colsum
    T = 2.0 * (K + 2) * U24 * (rstd * S + t.double().abs())
    e_s, e_m = NC.K * (1 + R["r"] ** 2) * U24, NC.K * (1 + R["r"]) * U24
    T = T + (R["xhat"].abs() @ wd.abs().T) * e_s + wd.abs().sum(1).view(1, -1) * e_m
    return ref, out_term(ref, T, BF)


def check(out, ref, bound):
    """dict(worst = max err / bound, index = where, outside = how many elements exceed their bound).  An element with bound 0 must be exact"""
    err = (out.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(out.double()), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return dict(worst=float(ratio.flatten()[i]), index=tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape))), outside=int((ratio > 1.0).sum()))


def t_use(out, ref, T, out_dtype=BF):
    """the share of T that the error beyond the output's own rounding takes, largest over the elements (the full err / bound is ~1.0 on any large bf16 tensor:
    some fp32 result lies halfway between two bf16 numbers)"""
    own = half_spacing(ref.abs() + T) if out_dtype == BF else U24 * ref.abs()
    return float((((out.double() - ref).abs() - own).clamp_min(0.0) / T.clamp_min(1e-300)).max())


def first_diff(out, exp):
    """where two tensors that should hold the same bits first differ, for the assertion message"""
    ne = (out != exp) | (torch.isnan(out.float()) != torch.isnan(exp.float()))
    n = int(ne.sum())
    if n == 0:
        return "equal"
    i = tuple(int(v) for v in ne.nonzero()[0])
    return f"{n} of {out.numel()} differ, first at {i}: got {float(out[i])!r}, expected {float(exp[i])!r}"


# ------------------------------------------------------------------------------------------------ numpy model of the pipeline (test_gemm_cases_cpu.py)
f32 = np.float32
ORDERS = ("sequential", "block16", "block32", "block64", "reversed", "splitk2")


def _tree(p):
    while p.shape[-1] > 1:
        h = p.shape[-1] // 2
        p = p[..., :h] + p[..., h:]
    return p[..., 0]


def model_accumulate(a, w, order):
    """fp32 accumulator [M, N] of a [M, K] x w [N, K]^T (fp32 arrays holding bf16 / e4m3 values: every product is an fp32 number, so a rounded sum of
    products is what an fma chain or an MFMA with fp32 accumulation leaves) in one of ORDERS"""
    a, w = np.asarray(a, f32), np.asarray(w, f32)
    K = a.shape[1]

    def chain(ks):
        acc = np.zeros((a.shape[0], w.shape[0]), f32)
        for k in ks:
            acc = acc + a[:, k, None] * w[None, :, k]
        return acc
    if order == "sequential":
        return chain(range(K))
    if order == "reversed":
        return chain(range(K - 1, -1, -1))
    if order == "splitk2":
        return chain(range(K // 2)) + chain(range(K // 2, K))
    b = int(order[5:])
    assert order.startswith("block") and K % b == 0
    acc = np.zeros((a.shape[0], w.shape[0]), f32)
    for k0 in range(0, K, b):
        acc = acc + _tree(a[:, None, k0:k0 + b] * w[None, :, k0:k0 + b])
    assert acc.dtype == f32
    return acc


def round_bf16(o, truncate=False):
    """fp32 array -> the fp32 values of its bf16 rounding (RNE; truncate: the low 16 bits dropped)"""
    o = np.ascontiguousarray(o, f32)
    if truncate:
        return (o.view(np.uint32) & np.uint32(0xffff0000)).view(f32)
    return torch.from_numpy(o).to(BF).float().numpy()


def model_epilogue(acc, bias=None, temb=None, res=None, out="bf16", mutate=None):
    """the epilogue as gemm_kernel.h has it: fmaf(acc, 1, bias), + temb (row-group bias / time-embedding row), + residual, all fp32, then ONE RNE to bf16.
    bias [N], temb and res [M, N] or None.  mutate: 'truncate' | 'acc_bf16' (the accumulator rounded to bf16 before the residual add) | 'bias_bf16'"""
    o = np.asarray(acc, f32)
    if bias is not None:
        b = np.asarray(bias, f32)
        o = o + (round_bf16(b) if mutate == "bias_bf16" else b)[None, :]
    if temb is not None:
        o = o + np.asarray(temb, f32)
    if mutate == "acc_bf16":
        o = round_bf16(o)
    if res is not None:
        o = o + np.asarray(res, f32)
    assert o.dtype == f32
    return o if out == "f32" else round_bf16(o, truncate=mutate == "truncate")
