"""The first and the last kernels of a UNet / VAE pass -- tmix_conv_in, tmix_conv_in_pre, tmix_conv_out (conv_io.hip), tmix_timestep_embedding, tmix_linear_small,
tmix_linear_small_sections (rowwise.hip) -- held bit for bit on inputs whose exact result is representable at every step, and per element against an fp64
reference on real-valued ones.  Inputs, references, the bounds and their derivations: head_tail_cases.py (built on gemm_cases.py); the checker's teeth, shown on
CPU models of the chains and their mutations: test_head_tail_cpu.py.

What the older tests cannot see and this file does: conv_in had one bit-exact case (Cin 4 -> Cout 64) and close() besides; conv_out one (Cin 96 -> Cout 4); the
embedding an atol of 2e-4 where a correct kernel errs by 5e-8 .. 7e-5; linear_small rtol = atol = 1e-4 on unit Gaussians at K 320 and 1280.  Never reached: the
<3> and <8> instantiations of conv_in, LDS stages beyond 64 KB (the hipFuncSetAttribute branch), the per_cu grid caps, a second trip of the persistent tile loop,
the bits of the pre-map's zero padding, conv_out at Cout 1 / 3 / 8 / 16 and Cin 32 / 128 / 320, K = 2816 (a ragged lane loop), K = 8, N % 4 != 0, section
boundaries inside a workgroup, silu_f's tails, and any structured input (a quiet image, a mean far from zero, a loud channel).

EXACT family, torch.equal on the bits, outputs pre-filled with NaN (head_tail_cases.py holds the lists):
    conv_in B, Cin, H, W, Cout = (3, 3, 5, 7, 128) (2, 4, 5, 7, 32) (2, 4, 12, 20, 320) (1, 8, 6, 10, 320) (1, 4, 6, 10, 512) (1, 4, 1, 1, 32) (2, 4, 9, 1, 64);
    a second trip of the tile loop at (2, 4, 160, 155, 32) (775 tiles over a cap of 768; 49,600 pixels are whole tiles), (1, 8, 130, 127, 320) (258 over 256) and
    (1, 4, 182, 181, 512) (515 over 512), the last two with a ragged last tile; (1, 4, 1, 1, 32) is the one-pixel image (Cin 4: the entry
    takes 3, 4 or 8); Cout 512, 640, 512, 320 in turn in one test (the `largest size so far` static of launch_conv_in); Cout 1056 (152,064 B of LDS, the largest stage carried); refusals on the return code with the output untouched: Cout 1088, Cin 5, Cout 48, a
    pre-map with Cin 8.  conv_in_pre at (2, 4, 5, 7, 64) and (1, 4, 6, 10, 512) with an integer 4 x 4 map and a non-zero integer bias (applied per pixel BEFORE
    the zero padding: a bias that leaks into the border changes integers), and the identity map with zero bias against tmix_conv_in's bits.
    conv_out B, H, W, Cin, Cout = (3, 5, 7, 128, 3) (2, 5, 7, 320, 4) (2, 5, 7, 32, 16) (1, 5, 7, 64, 8) (1, 5, 7, 32, 1) (1, 1, 1, 32, 4) (2, 9, 1, 64, 4), the filter
    rows under distinct power-of-two gains, NaN guards in front of and 16 planes behind the output (where a padded filter row would land); refused: Cout 17, Cin 48.
    linear_small M in {1, 4, 5, 16, 17, 37} x (N, K) in {(1280, 320), (1280, 2816), (5, 8), (1, 1280), (37, 64)}, without and with bias + add.
    linear_small_sections widths [5, 320, 3, 1280] (K = 320) at M = 4 and 37: the bits of the separate launches and of the expectation, the floats in front of and
    behind the sections keep their NaN (the sections themselves are dense, side by side: every float between two of them belongs to one and is compared).
STRUCTURED family (gauss, offset, quiet_image, loud_k, loud_out; linear_small also `tails`: x with std 8), |out - ref| <= bound for every element:
    conv_in at (3, 3, 5, 7, 128) (2, 4, 12, 20, 320) (2, 8, 6, 10, 320) (2, 4, 6, 10, 512) and the looped (2, 4, 160, 155, 32); the pre-map at (2, 4, 12, 20, 320);
    conv_out at (3, 5, 7, 128, 3) (2, 5, 7, 320, 4) (2, 5, 7, 32, 16) and (2, 33, 31, 128, 4) (32 workgroups, the last one ragged);
    linear_small at the five (N, K), M = 4 and 37, activations off and both on; the embedding at t in {999, 0, 0.5, 1, 12.75, 500, 981, 1024, -3},
    dim in {2, 256, 320, 1280}, count in {1, 5, 33} under |t| f (|u| + 2 [j > 0]) 2^-23 + 2^-23 (test_ops_gpu.py keeps its atol = 2e-4 assertion).

launch_conv_in remembers the raised LDS limit per PROCESS, not per device: harmless while every rank is its own process, and nothing a single-GPU test can show.
When the whole suite runs, an earlier file may have raised the limit already; run alone, test_conv_in_lds_limit_walk is the first conv_in launch of the process.

Found: no defect.  All six entries return the exact family's bits at every case above, the refusals come back as return codes with the NaN pre-fill intact, and
no store lands in a guard.  One correction to the case list as it was asked for: (2, 4, 160, 155, 32) has 49,600 = 775 x 64 pixels, so its last tile is whole;
the ragged last tile of a second trip is held by the other two looped cases.
Measured on an MI355X (every test prints its figures before it asserts), largest over the shapes of a family: full err / bound | share of the accumulation term
T used beyond the output's own rounding (gemm_cases.t_use; the first is ~1 for any bf16 output, the second is the figure that moves):
                        gauss            offset           quiet_image      loud_k           loud_out         tails            CPU model (largest share)
    conv_in             0.998 | 0.015    0.998 | 0.030    0.999 | 0.041    0.999 | 0.040    0.999 | 0.023    --               0.041
    conv_in_pre         0.997 | 0.010    0.996 | 0.007    0.998 | 0.011    0.998 | 0.022    0.998 | 0.008    --               0.022
    conv_out (fp32)     0.001 | 0.001    0.001 | 0.001    0.002 | 0.001    0.005 | 0.004    0.001 | 0.001    --               0.011
    linear_small        0.051 | 0.034    0.056 | 0.045    0.062 | 0.035    0.113 | 0.098    0.070 | 0.052    0.065 | 0.040    0.069
      silu in + out     0.035 | 0.028    0.036 | 0.029    0.060 | 0.037    0.119 | 0.102    0.044 | 0.032    0.065 | 0.043    0.063
    timestep embedding  err / bound 0.246 at dim 2 (the sine's rounding alone), 0.369 at 256, 0.482 at 320, 0.527 at 1280 (t = 999, j = 451; the CPU model with
                        correctly rounded expf / cosf / sinf: 0.527); share of |t| f (|u| + 2 [j > 0]) 2^-23 used beyond the trailing 2^-23: 0.000 / 0.355 / 0.445 / 0.490
conv_in's device figures are the CPU model's to three digits (the same sequential chain); conv_out's MFMA chain stays under the model's sequential order; the
linear_small figures above the model's are the 37-row cases (the model runs 5 rows; run on all
37 it gives the device's 0.098 / 0.102).  The whole file takes 4 s on the device.  No hand mutation of the real kernels was run on a device: the mutations are
shown on the CPU models (test_head_tail_cpu.py).
"""
import pytest
import torch

import head_tail_cases as HT
from test_ops_gpu import BF, lib_env, ops  # noqa: F401  (lib_env, ops: fixtures)

pytestmark = pytest.mark.gpu

G = HT.G
F32 = torch.float32
NAN = float("nan")
GUARD = 64                   # floats (bf16: elements) of NaN in front of and behind an output; a multiple of 16 bytes, so the output keeps its alignment
_cache = {}


def cached(key, build):
    """a case built once per module, on the CPU (the references are fp64 there); nothing mutates it afterwards"""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def L():
    from tweediemix_amd import lib
    return lib


def framed(n, dtype, behind=GUARD):
    """(whole buffer, the n elements in its middle), NaN all over"""
    buf = torch.full((GUARD + n + behind,), NAN, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def frame_kept(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def same(out, exp, what):
    out = out.cpu()
    assert out.dtype == exp.dtype and out.shape == exp.shape and torch.equal(out, exp), f"{what}: {G.first_diff(out, exp)}"


def refused(what, code, text, call, *untouched):
    with pytest.raises(L().TmixError) as e:
        call()
    msg = str(e.value)
    print(f"{what}: {msg}")
    assert f"code {code}:" in msg and text in msg, (what, msg)
    assert msg.rstrip().endswith(L().load().tmix_last_error_string().decode("utf-8", "replace").rstrip())
    for t in untouched:
        assert bool(torch.isnan(t).all()), f"{what}: output written"


def judge(what, out, ref, bound, T, out_dtype):
    """print the figures, then assert every element inside its bound"""
    out = out.cpu()
    r = G.check(out, ref, bound)
    use = G.t_use(out, ref, T, out_dtype)
    print(f"{what}: max err/bound {r['worst']:.3f} at {r['index']}, share of T used {use:.3f}")
    assert r["outside"] == 0 and r["worst"] <= 1.0, (what, r)
    return r["worst"], use


# ------------------------------------------------------------------------------------------------ exact family: conv_in
def run_conv_in(ops, c, shape, **kw):
    B, Cin, H, W, Cout = shape
    buf, y = framed(B * H * W * Cout, BF)
    ops.conv_in(c["x"].cuda(), c["w"].cuda(), c["bias"].cuda(), out=y.view(B, H, W, Cout), **kw)
    assert frame_kept(buf, y.numel()), f"conv_in {shape}: stores outside the output"
    return y.view(B, H, W, Cout)


def test_conv_in_lds_limit_walk(ops):
    """Cout 512 (73,728 B: the attribute is raised), 640 (92,160 B: raised again), 512 (under the largest size so far: no call), 320 (under 64 KB) in one process"""
    for Cout in HT.CONV_IN_LDS_WALK:
        shape = (1, 4, 6, 10, Cout)
        c = cached(("conv_in", shape, False), lambda: HT.exact_conv_in(shape))
        same(run_conv_in(ops, c, shape), c["exp_bf16"], f"conv_in {shape}, {HT.conv_in_smem(4, Cout)} B of LDS")


@pytest.mark.parametrize("shape", HT.CONV_IN_EXACT + HT.CONV_IN_LOOPED, ids=str)
def test_exact_conv_in_returns_the_bits(ops, shape):
    B, Cin, H, W, Cout = shape
    tiles, cap = HT.conv_in_tiles(B, H, W), HT.conv_in_grid_cap(Cin, Cout)
    assert (tiles > cap) == (shape in HT.CONV_IN_LOOPED)
    c = cached(("conv_in", shape, False), lambda: HT.exact_conv_in(shape))
    same(run_conv_in(ops, c, shape), c["exp_bf16"], f"conv_in {shape}")
    print(f"exact conv_in {shape}: {HT.conv_in_smem(Cin, Cout)} B of LDS, {tiles} tiles on a grid of {min(tiles, cap)}: bit-equal")


@pytest.mark.parametrize("shape", HT.CONV_IN_PRE, ids=str)
def test_exact_conv_in_pre_returns_the_bits_and_keeps_the_padding_zero(ops, shape):
    c = cached(("conv_in", shape, True), lambda: HT.exact_conv_in(shape, pre=True))
    same(run_conv_in(ops, c, shape, pre_w=c["pre_w"], pre_b=c["pre_b"]), c["exp_bf16"], f"conv_in_pre {shape}")
    plain = run_conv_in(ops, c, shape)
    same(run_conv_in(ops, c, shape, pre_w=torch.eye(4), pre_b=torch.zeros(4)), plain.cpu(), f"conv_in_pre {shape}, identity map against tmix_conv_in")
    same(run_conv_in(ops, c, shape, pre_w=torch.eye(4)), plain.cpu(), f"conv_in_pre {shape}, identity map without a bias against tmix_conv_in")


def test_conv_in_largest_stage_is_carried_and_the_argument_checks_refuse(ops):
    shape = HT.CONV_IN_LARGEST
    c = cached(("conv_in", shape, False), lambda: HT.exact_conv_in(shape))
    same(run_conv_in(ops, c, shape), c["exp_bf16"], f"conv_in {shape}, {HT.conv_in_smem(4, 1056)} B of LDS")
    E = L()

    def attempt(Cin, Cout, **kw):
        x, w, b = torch.zeros(1, Cin, 6, 10, device="cuda"), torch.zeros(Cout, 3, 3, Cin, device="cuda"), torch.zeros(Cout, device="cuda")
        buf = torch.full((6 * 10 * Cout + 2 * GUARD,), NAN, device="cuda", dtype=BF)
        return (lambda: ops.conv_in(x, w, b, out=buf[GUARD:GUARD + 60 * Cout].view(1, 6, 10, Cout), **kw)), buf
    for what, code, text, (call, buf) in [("Cout 1088 (156,672 B)", E.ESHAPE, "too large for the LDS weight stage", attempt(4, 1088)),
                                          ("Cin 5", E.ESHAPE, "Cin=5", attempt(5, 32)),
                                          ("Cout 48", E.ESHAPE, "Cout=48 must be a multiple of 32", attempt(4, 48)),
                                          ("pre-map with Cin 8", E.EINVAL, "pre-map is defined for 4 channels", attempt(8, 32, pre_w=torch.eye(4)))]:
        refused(f"conv_in {what}", code, text, call, buf)


# ------------------------------------------------------------------------------------------------ exact family: conv_out
def run_conv_out(ops, c, shape):
    B, H, W, Cin, Cout = shape
    n = B * Cout * H * W
    buf, y = framed(n, F32, behind=HT.CONV_OUT_GUARD * H * W)
    ops.conv_out(c["x"].cuda(), c["w"].cuda(), c["bias"].cuda(), out=y.view(B, Cout, H, W))
    assert frame_kept(buf, n), f"conv_out {shape}: stores outside the output (a padded filter row?)"
    return y.view(B, Cout, H, W)


@pytest.mark.parametrize("shape", HT.CONV_OUT_EXACT, ids=str)
def test_exact_conv_out_returns_the_bits(ops, shape):
    c = cached(("conv_out", shape), lambda: HT.exact_conv_out(shape))
    same(run_conv_out(ops, c, shape), c["exp_f32"], f"conv_out {shape}")


def test_conv_out_argument_checks_refuse(ops):
    for what, Cin, Cout in (("Cout 17", 32, 17), ("Cin 48", 48, 4)):
        x, w, b = torch.zeros(1, 5, 7, Cin, device="cuda", dtype=BF), torch.zeros(Cout, 3, 3, Cin, device="cuda", dtype=BF), torch.zeros(Cout, device="cuda")
        buf = torch.full((Cout * 35 + 2 * GUARD,), NAN, device="cuda")
        refused(f"conv_out {what}", L().ESHAPE, f"Cin={Cin} (%32) Cout={Cout} (<=16)", lambda: ops.conv_out(x, w, b, out=buf[GUARD:GUARD + Cout * 35].view(1, Cout, 5, 7)), buf)


# ------------------------------------------------------------------------------------------------ exact family: linear_small
def run_linear(ops, x, w, bias, add, M, **kw):
    N = w.shape[0]
    buf, y = framed(M * N, F32)
    ops.linear_small(x[:M], w, bias, None if add is None else add[:M], out=y.view(M, N), **kw)
    assert frame_kept(buf, M * N), f"linear_small M = {M}: stores outside the output"
    return y.view(M, N)


@pytest.mark.parametrize("N,K", HT.LINEAR_NK, ids=str)
def test_exact_linear_small_returns_the_bits(ops, N, K):
    c = cached(("linear", N, K), lambda: HT.exact_linear(N, K))
    x, w, bias, add = (c[k].cuda() for k in ("x", "w", "bias", "add"))
    for M in HT.LINEAR_M:
        same(run_linear(ops, x, w, None, None, M), c["exp_plain"][:M], f"linear_small {M} x {N} x {K}")
        same(run_linear(ops, x, w, bias, add, M), c["exp_full"][:M], f"linear_small {M} x {N} x {K} + bias + add")
    print(f"exact linear_small N = {N}, K = {K}: M in {HT.LINEAR_M}, without and with bias + add: bit-equal")


@pytest.mark.parametrize("M", [4, 37])
def test_exact_linear_small_sections_returns_the_bits(ops, M):
    c = cached(("sections", M), lambda: HT.exact_sections(M))
    x, w, bias = c["x"].cuda(), c["w"].cuda(), c["bias"].cuda()
    N, st = w.shape[0], c["starts"]
    buf, flat = framed(M * N, F32)
    ops.linear_small_sections(x, w, bias, torch.tensor(st, device="cuda", dtype=torch.int32), out=flat)
    assert frame_kept(buf, M * N), "linear_small_sections: stores in front of or behind the sections"
    same(flat, HT.sections_flat(c["exp_bias"], st), f"linear_small_sections M = {M}")
    for a, b in zip(st[:-1], st[1:]):
        sep = run_linear(ops, x, w[a:b], bias[a:b], None, M)
        assert torch.equal(flat[a * M:b * M].view(M, b - a), sep), f"section [{a}, {b}) against its own launch: {G.first_diff(flat[a * M:b * M].view(M, b - a), sep)}"


# ------------------------------------------------------------------------------------------------ structured family
@pytest.mark.parametrize("shape", HT.CONV_IN_STRUCTURED, ids=str)
@pytest.mark.parametrize("family", HT.FAMILIES)
def test_structured_conv_in_inside_the_bound(ops, family, shape):
    c = cached(("sconv_in", family, shape), lambda: HT.structured_conv_in(family, shape))
    judge(f"structured conv_in {family} {shape}", run_conv_in(ops, c, shape), c["ref"], c["bound"], c["T"], BF)


@pytest.mark.parametrize("family", HT.FAMILIES)
def test_structured_conv_in_pre_inside_the_bound(ops, family):
    shape = HT.CONV_IN_STRUCTURED[1]
    c = cached(("sconv_in_pre", family), lambda: HT.structured_conv_in(family, shape, pre=True))
    judge(f"structured conv_in_pre {family} {shape}", run_conv_in(ops, c, shape, pre_w=c["pre_w"], pre_b=c["pre_b"]), c["ref"], c["bound"], c["T"], BF)


@pytest.mark.parametrize("shape", HT.CONV_OUT_STRUCTURED, ids=str)
@pytest.mark.parametrize("family", HT.FAMILIES)
def test_structured_conv_out_inside_the_bound(ops, family, shape):
    c = cached(("sconv_out", family, shape), lambda: HT.structured_conv_out(family, shape))
    judge(f"structured conv_out {family} {shape}", run_conv_out(ops, c, shape), c["ref"], c["bound"], c["T"], F32)


@pytest.mark.parametrize("act", [False, True], ids=["plain", "silu_in+silu_out"])
@pytest.mark.parametrize("N,K", HT.LINEAR_NK, ids=str)
@pytest.mark.parametrize("family", HT.LIN_FAMILIES)
def test_structured_linear_small_inside_the_bound(ops, family, N, K, act):
    c = cached(("slinear", family, N, K), lambda: HT.structured_linear(family, 37, N, K))
    x, w, bias, add = (c[k].cuda() for k in ("x", "w", "bias", "add"))
    for M in (4, 37):
        ref, T, bound = HT.linear_bound(c["x"][:M], c["w"], c["bias"], c["add"][:M], act, act)
        judge(f"structured linear_small {family} {M} x {N} x {K} {'silu in + out' if act else 'plain'}", run_linear(ops, x, w, bias, add, M, act_in=act, act_out=act),
              ref, bound, T, F32)


@pytest.mark.parametrize("count", HT.EMBED_COUNTS)
@pytest.mark.parametrize("dim", HT.EMBED_DIMS)
def test_timestep_embedding_inside_the_bound(ops, dim, count):
    v = HT.embed_values(count)
    ref, A, bound = HT.embed_reference(v, dim)
    buf, e = framed(count * dim, F32)
    ops.timestep_embedding(v.cuda(), dim, out=e.view(count, dim))
    assert frame_kept(buf, count * dim)
    out = e.view(count, dim).cpu()
    r = G.check(out, ref, bound)
    print(f"timestep_embedding dim {dim} count {count}: max err/bound {r['worst']:.3f} at {r['index']}, share of the accumulated term used {HT.embed_use(out, ref, A):.3f}")
    assert r["outside"] == 0 and r["worst"] <= 1.0, (dim, count, r)
