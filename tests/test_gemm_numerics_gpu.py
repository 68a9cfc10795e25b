"""The GEMM / convolution family (gemm_kernel.h, gemm_conv.hip, gemm_convh.hip, gemm_w22.hip, gemm_inst_*.hip, conv_io.hip) held bit for bit on inputs
whose exact result is representable at every step, and per element against an fp64 reference on real-valued ones.  Inputs, references, the bound and
its derivation: gemm_cases.py; the checker's teeth, shown on a CPU model and its mutations: test_gemm_cases_cpu.py.

What close() of test_ops_gpu.py (atol = 2e-3 max|ref|, rtol 2^-7, fp32 torch reference) cannot see and this file does: anything below the global maximum
(a quiet row, image or column block), the rounding itself (truncation, a double rounding, a bias rounded before the add: all 1-ulp effects), and the
reference's own fp32 accumulation error.

EXACT family, torch.equal on the bits, every kernel the resolver reports (tmix_gemm_resolve_tile / tmix_conv_resolve_tile: each RESOLVED kernel runs once per
case, and test_every_live_tiling_is_reached asserts that the kernels reached are the ids that resolve to themselves):
    GEMM M x N x K = 260 x 324 x 384 (a full 256-row tile + 4 ragged rows; N % 8 = 4: the unstaged stores), 260 x 320 x 384 (staged stores; the width tiling 23
    carries), 33 x 4 x 64 and 33 x 320 x 64 (a partly filled tile, the column minimum, a single K-tile: ring prologue and drain with no steady state); K = 384 is
    six K-tiles, three 128-wide rows of the e4m3 lock-step loops.  Forms: plain, power-of-two row / column gains, bias + residual (+ row-group bias), fp32 output,
    transposed region at n_trans_begin 128 and 256, each also under TMIX_NARROW_EPILOGUE=1; batch 4 over 2 weight sets (w_period) with a strided A.
    e4m3 GEMM (ids 0, 12, 16, 17, 19, 20, 21, resolved) x {per-row scales, MX block scales on A} x {plain, bias + residual}.
    conv3x3 S1 / S2 / UP2 (UP2 as the plan builders pick it -- folded into TMIX_CONV_UP2F where up2_fold_ok -- and with TMIX_UP2_FOLD=0) on B, H, W, Cin, Cout =
    2, 5, 7, 64, 68 (S2, which needs even sides: 2, 6, 8), 1, 8, 32, 128, 160 (whole tiles of the halo-patch kernel) and 1, 6, 32, 64, 160 (an image it does not
    carry), bias + time-embedding row + residual; the temporal 3x1x1 form at 9 frames; shortcut taps (tiling 26 included); conv3x3_fp8; conv_in, conv_out at
    5 x 7 and 12 x 20.  Outputs are pre-filled with NaN and the padding columns (ldc > N, ldct > M) must keep it.
STRUCTURED family (gauss, loud_k, quiet_rows, offset, loud_out), |out - ref| <= bound per element (gemm_cases.py), bf16 and fp32 output, every kernel:
    GEMM 260 x 324 x 384 and 260 x 320 x 384, GEGLU (M = 200, C = 128), act = gelu, the folded LayerNorm, the e4m3 GEMMs against the fp64 product of the
    dequantised operands, the conv modes on the two small images.

Found: no defect.  All nineteen kernels return the exact family's bits in every form above and keep the NaN pre-fill of the padding columns.
Measured on an MI355X (every test prints its figures before it asserts), largest over the kernels of a class: full err / bound | share of T = 2 n 2^-24 S used
beyond the output's own rounding (gemm_cases.t_use).  The first is ~1 for any bf16 output whatever the kernel does -- some fp32 result lies halfway between two
bf16 numbers --; the second is the figure that moves (the CPU model of fp32 RNE accumulation in test_gemm_cases_cpu.py uses <= 0.014):
                                              lock-step (1 2 3 4 5 7 12 13 14 15 18 19 20 21)      phase-offset (16 17 22)     own kernels (23; conv: 26)
    bf16 GEMM, bf16 output, five families      0.88 .. 0.99 | <= 0.001                              the same figures            the same figures (23)
    bf16 GEMM, fp32 output (= share of T)      gauss, quiet_rows, loud_out 0.002, loud_k 0.008,     the same                    -- (23 has no fp32 output)
                                               offset 0.000 (split-K tiling 18: 0.001 / 0.006)
    GEGLU / gelu / folded LayerNorm            0.969 / 0.984 / 0.966                                the same                    folded LayerNorm 0.966 (23)
    e4m3 GEMM, per-row and MX scales           0.89 .. 0.99 | gauss, loud_out 0.09, quiet_rows      the same to three digits    --
                                               0.11, offset 0.03, loud_k 0.45
    conv3x3 S1 / S2 / UP2, two images          0.78 .. 0.97 | 0.000                                 -- (GEMM only)              0.85 | 0.000 (26)
The e4m3 rows are the one place where the device is far from the fp32 model (0.003 there): v_mfma_scale_f32_32x32x64_f8f6f4 does not add its 64 products like an
fp32 RNE chain; the figure is the same in all six kernels, so it is the instruction's, not a loop's.  It stays inside T, and the exact family shows that nothing
is lost while the sums fit 24 bits.
Hand mutations of the real kernels on a scratch build, cases of this file that fail: pack_bf2 truncating instead of RNE 103 of 122; the bias rounded to bf16 before
the fmaf of the two staged epilogues 37 of 122 (every launch with a bias on those paths).  close() of test_ops_gpu.py passes both.
"""
import ctypes as C

import pytest
import torch

import gemm_cases as G
from test_ops_gpu import BF, lib_env, ops  # noqa: F401  (lib_env, ops: fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
GEMM_SHAPES = [(260, 324, 384), (260, 320, 384), (33, 4, 64), (33, 320, 64)]
F8_IDS = (0, 12, 16, 17, 19, 20, 21)
CONV_SMALL, CONV_HALO, CONV_NO_HALO = (2, 5, 7, 64, 68), (1, 8, 32, 128, 160), (1, 6, 32, 64, 160)
_cache = {}


def cached(key, build):
    """a case built once per module and moved to the device; nothing mutates it afterwards"""
    if key not in _cache:
        c = build()
        _cache[key] = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()} if isinstance(c, dict) else c
    return _cache[key]


def L():
    from tweediemix_amd import lib
    return lib


# ------------------------------------------------------------------------------------------------ which kernels run a launch
def gemm_kernels(ops, a, w, out, fp8=0, **kw):
    """{kernel that runs: the id to ask for} over every id of a GEMM described as for ops.make_gemm_desc.  fp8: 1 = per-row scales, 2 = MX block scales on A"""
    lib, found = L().load(), {}
    for cfg in (F8_IDS if fp8 else range(1, L().TILE_COUNT + 1)):
        d = ops.make_gemm_desc(a, w, out, tile_cfg=cfg, **kw)
        if fp8 == 2:
            d.reserved0 = L().F8_A_BLOCK_SCALES
        r = lib.tmix_gemm_resolve_tile(C.byref(d), 1 if fp8 else 0)
        if r < 0:
            L().check(r, "tmix_gemm_resolve_tile")
        if r not in found or cfg == r:
            found[r] = cfg
    return found


def conv_kernels(ops, x, w, out, fp8=False, **kw):
    lib, found = L().load(), {}
    for cfg in range(1, L().TILE_COUNT + 1):
        d = ops.make_conv_desc(x, w, out, tile_cfg=cfg, _fp8=fp8, **kw)
        r = lib.tmix_conv_resolve_tile(C.byref(d), 1 if fp8 else 0)
        if r < 0:
            L().check(r, "tmix_conv_resolve_tile")
        if r not in found or cfg == r:
            found[r] = cfg
    return found


def nan_buf(*shape, dtype=BF):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def same(out, exp, what):
    assert out.dtype == exp.dtype and torch.equal(out, exp), f"{what}: {G.first_diff(out, exp)}"


# ------------------------------------------------------------------------------------------------ exact family: GEMM
GEMM_FORMS = ("plain", "gains", "bias+residual", "bias+residual+rgb", "f32", "trans128", "trans256")


def exact_gemm_form(ops, shape, form):
    """(case, kwargs of make_gemm_desc / ops.gemm, output buffers, expected tensors) of one exact GEMM launch form"""
    M, N, K = shape
    seed = 1000 + 7 * GEMM_SHAPES.index(shape)
    if form in ("trans128", "trans256"):
        ntb = int(form[5:])
        assert N > ntb
        c = cached(("gemm", shape, "gains"), lambda: G.exact_gemm(M, N, K, seed, gains=True))
        ldct = (M + 8 + 7) // 8 * 8
        qk, vt = nan_buf(M, ntb + 8), nan_buf(N - ntb, ldct)
        kw = dict(out_t=vt, n_trans_begin=ntb)
        return c, kw, (qk[:, :ntb], None), [(qk[:, :ntb], c["exp_bf16"][0][:, :ntb]), (vt[:, :M], c["exp_bf16"][0][:, ntb:].T), (qk[:, ntb:], None), (vt[:, M:], None)]
    if form == "bias+residual+rgb":
        c = cached(("gemm", shape, form), lambda: G.exact_gemm(M, N, K, seed + 1, bias=True, rgb_rows=104, residual=True))
        kw = dict(bias=c["bias"][0], residual=c["res"][0], rowgroup_bias=c["rgb"], rows_per_group=104)
    elif form == "bias+residual":                     # (without the row-group bias: the form tiling 23 carries)
        c = cached(("gemm", shape, form), lambda: G.exact_gemm(M, N, K, seed + 3, bias=True, residual=True))
        kw = dict(bias=c["bias"][0], residual=c["res"][0])
    else:
        gains = form != "plain"
        c = cached(("gemm", shape, "gains" if gains else "plain"), lambda: G.exact_gemm(M, N, K, seed + (0 if gains else 2), gains=gains))
        kw = {}
    if form == "f32":
        buf = nan_buf(M, N + 4, dtype=torch.float32)
        kw["out_f32"] = buf[:, :N]
        return c, kw, (None, None), [(buf[:, :N], c["exp_f32"][0]), (buf[:, N:], None)]
    buf = nan_buf(M, N + 8)
    return c, kw, (buf[:, :N], None), [(buf[:, :N], c["exp_bf16"][0]), (buf[:, N:], None)]


def run_exact_gemm(ops, shape, form, what):
    c, kw, (out, _), checks = exact_gemm_form(ops, shape, form)
    a, w = c["a"][0], c["w"][0]
    kernels = gemm_kernels(ops, a, w, out, **kw)
    for k, cfg in sorted(kernels.items()):
        for buf, _ in checks:
            buf.fill_(NAN)
        ops.gemm(a, w, out=out, tile_cfg=cfg, **kw)
        for buf, exp in checks:
            if exp is None:
                assert bool(torch.isnan(buf).all()), f"{what}, kernel {k}: padding columns written"
            else:
                same(buf, exp, f"{what}, kernel {k} (asked as {cfg})")
    print(f"{what}: {len(kernels)} kernels {sorted(kernels)} bit-equal")
    return kernels


GEMM_CASES = [(s, f) for s in GEMM_SHAPES for f in GEMM_FORMS if not (f.startswith("trans") and s[1] <= int(f[5:]))]      # (N = 4 has no transposed region)


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "TMIX_NARROW_EPILOGUE"])
@pytest.mark.parametrize("shape,form", GEMM_CASES, ids=lambda v: str(v))
def test_exact_gemm_returns_the_bits(ops, lib_env, shape, form, narrow):
    if narrow:
        lib_env("TMIX_NARROW_EPILOGUE")
    run_exact_gemm(ops, shape, form, f"exact GEMM {shape} {form}{' narrow' if narrow else ''}")


def batched_case():
    return cached("gemm batched", lambda: G.exact_gemm(33, 320, 64, 1100, batch=4, wsets=2, bias=True))


def batched_kernels(ops, run=False):
    """batch 4 over 2 weight sets (slice b reads set b % 2: tmix_gemm_desc.w_period) and bias rows, A a column slice of a wider tensor"""
    c = batched_case()
    big = torch.zeros(4, 33, 128, device="cuda", dtype=BF)
    big[:, :, 64:] = c["a"]
    a = big[:, :, 64:]
    buf = nan_buf(4, 33, 328)
    kernels = gemm_kernels(ops, a, c["w"], buf[:, :, :320], bias=c["bias"])
    for k, cfg in sorted(kernels.items()) if run else ():
        buf.fill_(NAN)
        ops.gemm(a, c["w"], out=buf[:, :, :320], bias=c["bias"], tile_cfg=cfg)
        same(buf[:, :, :320], c["exp_bf16"], f"batched GEMM, kernel {k}")
        assert bool(torch.isnan(buf[:, :, 320:]).all())
    return kernels


def test_exact_gemm_batched_periodic_weight_sets_and_strided_a(ops):
    k = batched_kernels(ops, run=True)
    print(f"exact GEMM batch 4 x 2 weight sets: {len(k)} kernels {sorted(k)} bit-equal")


# ------------------------------------------------------------------------------------------------ exact family: e4m3 GEMM
def f8_case(N, mx, extra):
    return cached(("f8", N, mx, extra), lambda: G.exact_gemm_fp8(260, N, 384, 1200 + N + 2 * mx + extra, mx=mx, bias=bool(extra), residual=bool(extra)))


def f8_kernels(ops, N, mx, extra, run=False):
    c = f8_case(N, mx, extra)
    buf = nan_buf(260, N + 8)
    kw = dict(bias=c["bias"], residual=c["res"]) if extra else {}
    kernels = gemm_kernels(ops, c["a8"], c["w8"], buf[:, :N], fp8=2 if mx else 1, **kw)
    for k, cfg in sorted(kernels.items()) if run else ():
        buf.fill_(NAN)
        ops.gemm_fp8(c["a8"], c["sa"], c["w8"], c["sw"], out=buf[:, :N], a_block_scales=mx, tile_cfg=cfg, **kw)
        same(buf[:, :N], c["exp_bf16"], f"e4m3 GEMM 260 x {N} x 384 mx={mx} extra={extra}, kernel {k} (asked as {cfg})")
        assert bool(torch.isnan(buf[:, N:]).all())
    return kernels


@pytest.mark.parametrize("extra", [0, 1], ids=["plain", "bias+residual"])
@pytest.mark.parametrize("mx", [False, True], ids=["per-row", "mx"])
@pytest.mark.parametrize("N", [324, 320])
def test_exact_gemm_fp8_returns_the_bits(ops, N, mx, extra):
    k = f8_kernels(ops, N, mx, extra, run=True)
    print(f"exact e4m3 GEMM 260 x {N} x 384 {'MX' if mx else 'per-row'} {'bias+residual' if extra else 'plain'}: kernels {sorted(k)} bit-equal")


# ------------------------------------------------------------------------------------------------ exact family: convolutions
def conv_shape(shape, mode):
    B, H, W, Cin, Cout = shape
    return (B, H + H % 2, W + W % 2, Cin, Cout) if mode == G.S2 else shape           # stride 2 takes even sides only


def conv_case(shape, mode, residual=True):
    shape = conv_shape(shape, mode)
    return cached(("conv", shape, mode, residual), lambda: G.exact_conv(*shape, mode, 1300 + 10 * mode + shape[1], residual=residual))


def conv_launch(ops, c, mode, fold):
    """(x, w, kwargs) of the launch: UP2 folded into the four 2x2 phase convolutions where asked (the fold of these integer weights is exact; it takes no residual)"""
    w, kw = c["w"], dict(bias=c["bias"], batch_bias=c["temb"], residual=c["res"], mode=mode)
    if fold:
        w = ops.fold_up2_weight(c["w"])
        assert torch.equal(w.double(), ops.fold_up2_weight(c["w"].double(), dtype=None))
        kw.update(mode=L().CONV_UP2F, residual=None)
    return c["x"], w, kw


def conv_exact_kernels(ops, shape, mode, run=False, what=""):
    B, H, W, _, _ = shape
    fold = mode == G.UP2 and ops.up2_fold_ok(H, W)
    c = conv_case(shape, mode, residual=not fold)
    x, w, kw = conv_launch(ops, c, mode, fold)
    out = nan_buf(*c["exp_bf16"].shape)
    kernels = conv_kernels(ops, x, w, out, **kw)
    for k, cfg in sorted(kernels.items()) if run else ():
        out.fill_(NAN)
        ops.conv3x3(x, w, out=out, tile_cfg=cfg, **kw)
        same(out, c["exp_bf16"], f"{what}, kernel {k} (asked as {cfg})")
    if run:
        print(f"{what}{' (folded: TMIX_CONV_UP2F)' if fold else ''}: {len(kernels)} kernels {sorted(kernels)} bit-equal")
    return kernels


@pytest.mark.parametrize("mode", [G.S1, G.S2, G.UP2], ids=["S1", "S2", "UP2"])
@pytest.mark.parametrize("shape", [CONV_SMALL, CONV_HALO, CONV_NO_HALO], ids=str)
def test_exact_conv3x3_returns_the_bits(ops, shape, mode):
    conv_exact_kernels(ops, shape, mode, run=True, what=f"exact conv3x3 {conv_shape(shape, mode)} mode {mode}")


def test_exact_conv3x3_up2_unfolded_returns_the_bits(ops, lib_env):
    assert ops.up2_fold_ok(8, 32)
    lib_env("TMIX_UP2_FOLD", "0")
    assert not ops.up2_fold_ok(8, 32)
    conv_exact_kernels(ops, CONV_HALO, G.UP2, run=True, what=f"exact conv3x3 {CONV_HALO} UP2 with TMIX_UP2_FOLD=0")


def t3_kernels(ops, run=False):
    """the temporal 3x1x1 form: x [clips, frames, hw, Cin] at 9 frames"""
    c = cached("t3", lambda: G.exact_conv(2, 9, 30, 128, 192, G.T3, 1400, temb=False))
    out = nan_buf(*c["exp_bf16"].shape)
    kw = dict(bias=c["bias"], residual=c["res"], mode=L().CONV_T3)
    kernels = conv_kernels(ops, c["x"], c["w"], out, **kw)
    for k, cfg in sorted(kernels.items()) if run else ():
        out.fill_(NAN)
        ops.conv3x3(c["x"], c["w"], out=out, tile_cfg=cfg, **kw)
        same(out, c["exp_bf16"], f"temporal conv, kernel {k}")
    return kernels


def test_exact_temporal_conv_returns_the_bits(ops):
    k = t3_kernels(ops, run=True)
    print(f"exact temporal 3x1x1 conv, 9 frames: {len(k)} kernels {sorted(k)} bit-equal")


SHORTCUT_SHAPES = [(2, 5, 7, 64, 72), CONV_HALO]


def shortcut_kernels(ops, shape, run=False):
    c = cached(("shortcut", shape), lambda: G.exact_conv(*shape, G.S1, 1500 + shape[1], residual=False, shortcut=64))
    w = ops.shortcut_weight(c["w"], c["wsc"])
    out = nan_buf(*c["exp_bf16"].shape)
    kw = dict(bias=c["bias"], batch_bias=c["temb"], shortcut=(c["s1"], None))
    kernels = conv_kernels(ops, c["x"], w, out, **kw)
    for k, cfg in sorted(kernels.items()) if run else ():
        out.fill_(NAN)
        ops.conv3x3(c["x"], w, out=out, tile_cfg=cfg, **kw)
        same(out, c["exp_bf16"], f"conv with shortcut taps {shape}, kernel {k}")
    return kernels


@pytest.mark.parametrize("shape", SHORTCUT_SHAPES, ids=str)
def test_exact_conv_with_shortcut_taps_returns_the_bits(ops, shape):
    k = shortcut_kernels(ops, shape, run=True)
    assert (L().TILE_CONV_HALO in k) == (shape == CONV_HALO)
    print(f"exact conv3x3 + shortcut taps {shape}: {len(k)} kernels {sorted(k)} bit-equal")


@pytest.mark.parametrize("mode", [G.S1, G.S2, G.UP2], ids=["S1", "S2", "UP2"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 128, 68), CONV_HALO], ids=str)
def test_exact_conv3x3_fp8_returns_the_bits(ops, shape, mode):
    shape = conv_shape(shape, mode)
    c = cached(("conv8", shape, mode), lambda: G.exact_conv(*shape, mode, 1600 + mode, fp8=True))
    out = nan_buf(*c["exp_bf16"].shape)
    kw = dict(bias=c["bias"], batch_bias=c["temb"], residual=c["res"], mode=mode)
    kernels = conv_kernels(ops, c["x8"], c["w8"], out, fp8=True, **kw)
    for k, cfg in sorted(kernels.items()):
        out.fill_(NAN)
        ops.conv3x3_fp8(c["x8"], c["sx"], c["w8"], c["sw"], out=out, tile_cfg=cfg, **kw)
        same(out, c["exp_bf16"], f"conv3x3_fp8 {shape} mode {mode}, kernel {k}")
    print(f"exact conv3x3_fp8 {shape} mode {mode}: kernels {sorted(kernels)} bit-equal")


@pytest.mark.parametrize("H,W", [(5, 7), (12, 20)])
def test_exact_conv_in_and_conv_out_return_the_bits(ops, H, W):
    """their fp32 VALU chain / MFMA accumulation are exact on these inputs as well"""
    ci = cached(("conv_in", H, W), lambda: G.exact_conv_in(2, 4, H, W, 64, 1700))
    y = nan_buf(2, H, W, 64)
    ops.conv_in(ci["x"], ci["w"], ci["bias"], out=y)
    same(y, ci["exp_bf16"], f"conv_in {H} x {W}")
    co = cached(("conv_out", H, W), lambda: G.exact_conv_out(2, H, W, 96, 4, 1710))
    z = nan_buf(2, 4, H, W, dtype=torch.float32)
    ops.conv_out(co["x"], co["w"], co["bias"], out=z)
    same(z, co["exp_f32"], f"conv_out {H} x {W}")


# ------------------------------------------------------------------------------------------------ the kernels reached are the live tilings
def test_every_live_tiling_is_reached(ops):
    """live = the ids that resolve to themselves for some launch (a retired or reserved id never does: gemm_tilings.h runs_as), asked of the resolver on the most
    permissive launches -- a staged plain GEMM 160 columns wide and a stride-1 convolution on whole halo tiles.  reached = what the exact tests above enumerate"""
    a, w = torch.zeros(256, 128, device="cuda", dtype=BF), torch.zeros(320, 128, device="cuda", dtype=BF)
    x, wc = torch.zeros(1, 8, 32, 64, device="cuda", dtype=BF), torch.zeros(160, 3, 3, 64, device="cuda", dtype=BF)
    g = gemm_kernels(ops, a, w, torch.empty(256, 320, device="cuda", dtype=BF))
    c = conv_kernels(ops, x, wc, torch.empty(1, 8, 32, 160, device="cuda", dtype=BF))
    live = {k for k, cfg in g.items() if k == cfg} | {k for k, cfg in c.items() if k == cfg}
    assert all(1 <= k <= L().TILE_COUNT for k in live) and len(live) > 1
    reached_gemm, reached_conv, reached_f8 = set(), set(), set()
    for shape, form in GEMM_CASES:
        cse, kw, (out, _), _ = exact_gemm_form(ops, shape, form)
        reached_gemm |= set(gemm_kernels(ops, cse["a"][0], cse["w"][0], out, **kw))
    reached_gemm |= set(batched_kernels(ops))
    for N in (324, 320):
        for mx in (False, True):
            reached_f8 |= set(f8_kernels(ops, N, mx, 0)) | set(f8_kernels(ops, N, mx, 1))
    for shape in (CONV_SMALL, CONV_HALO, CONV_NO_HALO):
        for mode in (G.S1, G.S2, G.UP2):
            reached_conv |= set(conv_exact_kernels(ops, shape, mode))
    reached_conv |= set(t3_kernels(ops))
    for shape in SHORTCUT_SHAPES:
        reached_conv |= set(shortcut_kernels(ops, shape))
    print(f"live tilings {sorted(live)}; reached by the exact GEMMs {sorted(reached_gemm)}, the exact convolutions {sorted(reached_conv)}, the e4m3 GEMMs {sorted(reached_f8)}")
    assert reached_gemm | reached_conv == live, (sorted(live), sorted(reached_gemm | reached_conv))
    assert reached_gemm == {k for k, cfg in g.items() if k == cfg} and reached_conv == {k for k, cfg in c.items() if k == cfg}
    assert reached_f8 <= live


# ------------------------------------------------------------------------------------------------ structured family
def judge(what, results):
    """results: (kernel, check dict, share of T used).  Print the worst, then assert every element of every kernel inside its bound"""
    k, r, use = max(results, key=lambda t: t[1]["worst"])
    print(f"{what}: {len(results)} kernels, max err/bound {r['worst']:.3f} (kernel {k} at {r['index']}), share of T used {max(t[2] for t in results):.3f};"
          f" by kernel err/bound | share of T: " + ", ".join(f"{k} {r['worst']:.3f}|{u:.3f}" for k, r, u in results))
    for k, r, _ in results:
        assert r["outside"] == 0 and r["worst"] <= 1.0, (what, k, r)


def structured_case(family, N):
    def build():
        M, K = 260, 384
        a, w = G.structured_operands(family, M, N, K, 2000 + N)
        g = G._gen(2001)
        c = dict(a=a.to(BF), w=w.to(BF), bias=torch.randn(N, generator=g), rgb=torch.randn(3, N, generator=g), res=torch.randn(M, N, generator=g).to(BF))
        c = {k: v.cuda() for k, v in c.items()}
        ad, wd = c["a"].double(), c["w"].double()
        add = [c["bias"].double().expand(M, N), c["rgb"].double().repeat_interleave(104, 0)[:M], c["res"].double()]
        c["ref0"], c["S0"] = ad @ wd.T, ad.abs() @ wd.abs().T
        c["ref1"], c["S1"] = c["ref0"] + sum(add), c["S0"] + sum(t.abs() for t in add)
        c["ref2"], c["S2"] = c["ref0"] + add[0] + add[2], c["S0"] + add[0].abs() + add[2].abs()
        return c
    return cached(("structured", family, N), build)


@pytest.mark.parametrize("out_dtype", ["bf16", "f32"])
@pytest.mark.parametrize("N", [324, 320])
@pytest.mark.parametrize("family", G.STRUCTURED)
def test_structured_gemm_inside_the_bound(ops, family, N, out_dtype):
    """bf16: bias + row-group bias + residual ride along (n = K + 3; at N = 320 bias + residual only); fp32 output: the plain product"""
    M, K = 260, 384
    c = structured_case(family, N)
    if out_dtype == "f32":
        buf = nan_buf(M, N, dtype=torch.float32)
        kw, out, ref, S, n, dt = dict(out_f32=buf), None, c["ref0"], c["S0"], K, torch.float32
    else:
        buf = nan_buf(M, N)
        kw, out, ref, S, n, dt = dict(bias=c["bias"], rowgroup_bias=c["rgb"], rows_per_group=104, residual=c["res"]), buf, c["ref1"], c["S1"], K + 3, BF
        if N == 320:            # without the row-group bias (n = K + 2): the launch tiling 23 carries
            kw, ref, S, n = dict(bias=c["bias"], residual=c["res"]), c["ref2"], c["S2"], K + 2
    bound, T = G.gemm_bound(ref, S, n, dt), 2.0 * n * G.U24 * S
    results = []
    for k, cfg in sorted(gemm_kernels(ops, c["a"], c["w"], out, **kw).items()):
        buf.fill_(NAN)
        ops.gemm(c["a"], c["w"], out=out, tile_cfg=cfg, **kw)
        results.append((k, G.check(buf, ref, bound), G.t_use(buf, ref, T, dt)))
    judge(f"structured GEMM {family} 260 x {N} x 384 {out_dtype}", results)


@pytest.mark.parametrize("act", ["geglu", "gelu"])
def test_structured_gelu_epilogues_inside_the_bound(ops, act):
    from tweediemix_amd.weights import interleave_geglu
    M, Cc = 200, 128
    N = 8 * Cc if act == "geglu" else 320

    def build():
        a, w = G.structured_operands("gauss", M, N, Cc, 2100)
        c = dict(a=a.to(BF).cuda(), w=w.to(BF).cuda(), b=torch.randn(N, generator=G._gen(2101)).cuda())
        y = c["a"].double() @ c["w"].double().T + c["b"].double()
        Ty = 2.0 * (Cc + 1) * G.U24 * (c["a"].double().abs() @ c["w"].double().abs().T + c["b"].double().abs())
        if act == "geglu":
            c["ref"], c["bound"] = G.gelu_bound(y[:, :4 * Cc], y[:, 4 * Cc:], Ty[:, :4 * Cc], Ty[:, 4 * Cc:])
            c["wi"], c["bi"] = interleave_geglu(c["w"], c["b"])
        else:
            c["ref"], c["bound"] = G.gelu_bound(torch.ones_like(y), y, torch.zeros_like(y), Ty)
        return c
    c = cached(("gelu", act), build)
    kw = dict(bias=c["bi"], geglu=True) if act == "geglu" else dict(bias=c["b"], act="gelu")
    w = c["wi"] if act == "geglu" else c["w"]
    out = nan_buf(*c["ref"].shape)
    results = []
    for k, cfg in sorted(gemm_kernels(ops, c["a"], w, out, **kw).items()):
        out.fill_(NAN)
        ops.gemm(c["a"], w, out=out, tile_cfg=cfg, **kw)
        results.append((k, G.check(out, c["ref"], c["bound"]), 0.0))
    judge(f"structured {act} M = {M}, C = {Cc}", results)


def test_structured_folded_layernorm_inside_the_bound(ops):
    """Linear(LayerNorm(h)) with the norm folded into the GEMM (ln_stats / ln_colsum): an identity producer stores bf16 rows with mean 0.7 exactly and leaves their
    statistics; every kernel then runs the consumer.  The statistics term is norm_cases' (one-pass variance: E_s = k (1 + r^2) 2^-24), carried through the product"""
    from tweediemix_amd.weights import fold_layernorm
    M, C1, N2 = 260, 256, 320

    def build():
        g = G._gen(2200)
        x = (torch.randn(M, C1, generator=g) + 0.7).to(BF).cuda()
        gamma, beta = (torch.randn(C1, generator=g) * 0.2 + 1).cuda(), (torch.randn(C1, generator=g) * 0.3).cuda()
        w2, b2 = (torch.randn(N2, C1, generator=g) * C1 ** -0.5).to(BF).cuda(), torch.randn(N2, generator=g).cuda()
        stats = torch.full((ops.stats_parts(C1, 1), M, 2), NAN, device="cuda")
        h = ops.gemm(x, torch.eye(C1, device="cuda", dtype=BF), row_stats_out=stats, tile_cfg=1)
        assert torch.equal(h, x)
        wp, cs, t = fold_layernorm(w2, gamma, beta, b2)
        ref, bound = G.ln_fold_reference(h, wp, t, 1e-5)
        return dict(h=h, wp=wp, cs=cs, t=t, stats=stats, ref=ref, bound=bound)
    c = cached("lnfold", build)
    kw = dict(bias=c["t"], ln_stats=c["stats"], ln_colsum=c["cs"])
    out = nan_buf(M, N2)
    results = []
    for k, cfg in sorted(gemm_kernels(ops, c["h"], c["wp"], out, **kw).items()):
        out.fill_(NAN)
        ops.gemm(c["h"], c["wp"], out=out, tile_cfg=cfg, **kw)
        results.append((k, G.check(out, c["ref"], c["bound"]), 0.0))
    judge("structured folded LayerNorm 260 x 320 x 256", results)


@pytest.mark.parametrize("mx", [False, True], ids=["per-row", "mx"])
@pytest.mark.parametrize("family", G.STRUCTURED)
def test_structured_gemm_fp8_inside_the_bound(ops, family, mx):
    """against the fp64 product of the dequantised operands (products of e4m3 values are fp32 numbers: the same T), bias + residual"""
    M, N, K = 260, 320, 384

    def build():
        a8, sa, av, w8, sw, wv = G.structured_operands(family, M, N, K, 2300, G.F8, full=True)
        if not mx:
            a, _ = G.structured_operands(family, M, N, K, 2300, torch.float32)
            a8, sa, av = G.quantize_rows(a)
        g = G._gen(2301)
        c = dict(a8=a8, sa=sa, w8=w8, sw=sw, bias=torch.randn(N, generator=g), res=torch.randn(M, N, generator=g).to(BF))
        c = {k: v.cuda() for k, v in c.items()}
        ad, wd = av.cuda().double(), wv.cuda().double()
        c["ref"] = ad @ wd.T + c["bias"].double() + c["res"].double()
        c["S"] = ad.abs() @ wd.abs().T + c["bias"].double().abs() + c["res"].double().abs()
        return c
    c = cached(("structured8", family, mx), build)
    bound, T = G.gemm_bound(c["ref"], c["S"], K + 2), 2.0 * (K + 2) * G.U24 * c["S"]
    kw = dict(bias=c["bias"], residual=c["res"])
    out = nan_buf(M, N)
    results = []
    for k, cfg in sorted(gemm_kernels(ops, c["a8"], c["w8"], out, fp8=2 if mx else 1, **kw).items()):
        out.fill_(NAN)
        ops.gemm_fp8(c["a8"], c["sa"], c["w8"], c["sw"], out=out, a_block_scales=mx, tile_cfg=cfg, **kw)
        results.append((k, G.check(out, c["ref"], bound), G.t_use(out, c["ref"], T)))
    judge(f"structured e4m3 GEMM {family} {'MX' if mx else 'per-row'} 260 x 320 x 384", results)


@pytest.mark.parametrize("mode", [G.S1, G.S2, G.UP2], ids=["S1", "S2", "UP2"])
@pytest.mark.parametrize("shape", [CONV_SMALL, CONV_HALO], ids=str)
def test_structured_conv3x3_inside_the_bound(ops, shape, mode):
    """unit-Gaussian pixels whose image b is 2^(-6 b) quieter and whose rows fade by 2^-(y mod 5): quiet images and rows next to loud ones.  UP2 runs unfolded
    (the fold rounds the summed weights to bf16: another operand, not another kernel path -- the exact family holds the folded form)"""
    B, H, W, Cin, Cout = shape = conv_shape(shape, mode)

    def build():
        g = G._gen(2400 + mode)
        x = torch.randn(B, H, W, Cin, generator=g) * (2.0 ** (-6.0 * torch.arange(B))).view(B, 1, 1, 1) * (2.0 ** -(torch.arange(H) % 5).float()).view(1, H, 1, 1)
        w = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5
        c = dict(x=x.to(BF).cuda(), w=w.to(BF).cuda(), bias=torch.randn(Cout, generator=g).cuda() * 2.0 ** -6, temb=torch.randn(B, Cout, generator=g).cuda() * 2.0 ** -6)
        ref = G.conv_product(c["x"].double(), c["w"].double(), mode)
        c["res"] = (torch.randn(*ref.shape, generator=g) * 2.0 ** -6).to(BF).cuda()
        add = c["bias"].double() + c["temb"].double()[:, None, None] + c["res"].double()
        c["ref"] = ref + add
        c["S"] = G.conv_product(c["x"].double().abs(), c["w"].double().abs(), mode) + c["bias"].double().abs() + c["temb"].double().abs()[:, None, None] + c["res"].double().abs()
        return c
    c = cached(("sconv", shape, mode), build)
    n = 9 * Cin + 3
    bound, T = G.gemm_bound(c["ref"], c["S"], n), 2.0 * n * G.U24 * c["S"]
    kw = dict(bias=c["bias"], batch_bias=c["temb"], residual=c["res"], mode=mode)
    out = nan_buf(*c["ref"].shape)
    results = []
    for k, cfg in sorted(conv_kernels(ops, c["x"], c["w"], out, **kw).items()):
        out.fill_(NAN)
        ops.conv3x3(c["x"], c["w"], out=out, tile_cfg=cfg, **kw)
        results.append((k, G.check(out, c["ref"], bound), G.t_use(out, c["ref"], T)))
    judge(f"structured conv3x3 {shape} mode {mode}", results)
