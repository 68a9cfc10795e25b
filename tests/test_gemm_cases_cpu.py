"""The checker of test_gemm_numerics_gpu.py has teeth -- shown without a GPU, on a numpy model of the pipeline as the code has it (gemm_cases.py:
fp32 accumulation, fmaf(acc, 1, bias), + time-embedding / row-group row, + residual in fp32, ONE RNE to bf16) run in six summation orders: sequential,
blocks of 16 / 32 / 64 summed pairwise and then chained, reversed, split-K 2.

  * exact family: every order reproduces the expected bits (GEMM plain / with gains / with bias + row + residual, e4m3 values with per-row and MX block
    scales, the convolution modes through im2col);
  * structured family: every order stays inside the bound.  The full err / bound reaches 1.0 by construction (a correctly rounded result may lie half a
    bf16 spacing from the reference); the figure that moves is the share of T = 2 n 2^-24 S the UNROUNDED fp32 accumulator uses, largest over the
    orders (at most 0.5: the model rounds to nearest), by family  gauss / loud_k / quiet_rows / offset / loud_out:
        bf16 operands 0.002 / 0.014 / 0.002 / 0.000 / 0.002      e4m3 operands with MX block scales 0.001 / 0.003 / 0.002 / 0.000 / 0.001
    (64 x 40 x 384; full err / bound 0.86 .. 0.99).  fp32 rounding errors of random sign add up like sqrt(n), the bound like n: a correct kernel is far inside T
  * every mutation of the model is flagged: truncation instead of RNE; the accumulator rounded to bf16 before the residual add; the bias rounded to bf16
    before the add; the last 32 K values of one 32-row block dropped; one MX block's exponent off by one; a convolution border tap clamped instead of zero;
    output rows m and m + 32 exchanged on `quiet_rows` -- which today's close() of test_ops_gpu.py (atol tied to the largest element of the whole
    output) passes.  That last one is the reason this file and its GPU sibling exist.
"""
import numpy as np
import pytest
import torch

import gemm_cases as G

M, N, K = 64, 40, 384
f32 = np.float32


def np32(t):
    return None if t is None else t.float().numpy()


def run(a, w, order, bias=None, temb=None, res=None, out="bf16", mutate=None):
    return G.model_epilogue(G.model_accumulate(a, w, order), bias, temb, res, out, mutate)


def same_bits(o, e):
    return np.array_equal(np.ascontiguousarray(o, f32).view(np.uint32), np.ascontiguousarray(e, f32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ cases (built once)
def _exact_gemm(**kw):
    c = G.exact_gemm(M, N, K, 10, **kw)
    rgb = None if c["rgb"] is None else np32(c["rgb"].repeat_interleave(c["rgb_rows"], 0)[:M])
    return dict(a=np32(c["a"][0]), w=np32(c["w"][0]), bias=np32(None if c["bias"] is None else c["bias"][0]), temb=rgb, res=np32(None if c["res"] is None else c["res"][0]),
                exp_bf16=np32(c["exp_bf16"][0]), exp_f32=np32(c["exp_f32"][0]))


def _exact_fp8(mx):
    c = G.exact_gemm_fp8(M, N, K, 20, mx=mx, bias=True, residual=True)
    return dict(a=np32(c["ad"]), w=np32(c["wd"]), bias=np32(c["bias"]), temb=None, res=np32(c["res"]), exp_bf16=np32(c["exp_bf16"]), exp_f32=np32(c["exp_f32"]))


def _exact_conv(mode, border="zero"):
    shape = (1, 6, 8, 64, 8) if mode == G.S2 else (1, 5, 7, 64, 8)
    c = G.exact_conv(*shape, mode, 30)
    Cout = shape[-1]
    e = c["exp_bf16"].reshape(-1, Cout)
    rows = e.shape[0]
    return dict(a=np32(G.im2col(c["x"].double(), mode, border)), w=np32(c["w"].reshape(Cout, -1)), bias=np32(c["bias"]),
                temb=np32(c["temb"].repeat_interleave(rows // shape[0], 0)), res=np32(c["res"].reshape(-1, Cout)), exp_bf16=np32(e), exp_f32=np32(c["exp_f32"].reshape(-1, Cout)))


EXACT = {"plain": lambda: _exact_gemm(), "gains": lambda: _exact_gemm(gains=True), "bias+row+residual": lambda: _exact_gemm(bias=True, rgb_rows=24, residual=True),
         "gains+bias+residual": lambda: _exact_gemm(gains=True, bias=True, residual=True), "e4m3 per-row": lambda: _exact_fp8(False), "e4m3 MX": lambda: _exact_fp8(True),
         "conv S1": lambda: _exact_conv(G.S1), "conv S2": lambda: _exact_conv(G.S2), "conv UP2": lambda: _exact_conv(G.UP2)}
_cache = {}


def exact(name):
    if name not in _cache:
        _cache[name] = EXACT[name]()
    return _cache[name]


def structured(family, dtype=G.BF):
    """operands, epilogue terms, fp64 reference, S and n of one structured case"""
    key = (family, dtype)
    if key not in _cache:
        a, w = G.structured_operands(family, M, N, K, 40, dtype)
        g = G._gen(41)
        bias, temb = torch.randn(N, generator=g), torch.randn(M // 16, N, generator=g).repeat_interleave(16, 0)
        res = torch.randn(M, N, generator=g).to(G.BF).float()
        ref = a.double() @ w.double().T + bias.double() + temb.double() + res.double()
        S = a.double().abs() @ w.double().abs().T + bias.double().abs() + temb.double().abs() + res.double().abs()
        _cache[key] = dict(a=a.numpy(), w=w.numpy(), bias=bias.numpy(), temb=temb.numpy(), res=res.numpy(), ref=ref, S=S, n=K + 3)
    return _cache[key]


def structured_conv():
    if "sconv" not in _cache:
        B, H, W, Cin, Cout = 1, 5, 7, 64, 8
        g = G._gen(50)
        x = torch.randn(B, H, W, Cin, generator=g).to(G.BF).double()
        w = (torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5).to(G.BF).double()
        bias = torch.randn(Cout, generator=g)
        ref = G.conv_product(x, w, G.S1).reshape(-1, Cout) + bias.double()
        S = G.conv_product(x.abs(), w.abs(), G.S1).reshape(-1, Cout) + bias.double().abs()
        _cache["sconv"] = dict(x=x, w=np32(w.reshape(Cout, -1)), bias=bias.numpy(), ref=ref, S=S, n=9 * Cin + 1)
    return _cache["sconv"]


def outside(o, c, out_dtype=G.BF):
    return G.check(torch.from_numpy(np.ascontiguousarray(o)), c["ref"], G.gemm_bound(c["ref"], c["S"], c["n"], out_dtype))


# ------------------------------------------------------------------------------------------------ the model itself passes
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_family_is_bit_equal_under_every_summation_order(name):
    c = exact(name)
    for order in G.ORDERS:
        acc = G.model_accumulate(c["a"], c["w"], order)
        assert same_bits(G.model_epilogue(acc, c["bias"], c["temb"], c["res"]), c["exp_bf16"]), (name, order)
        assert same_bits(G.model_epilogue(acc, c["bias"], c["temb"], c["res"], out="f32"), c["exp_f32"]), (name, order, "f32")
    print(f"exact {name}: bit-equal in {len(G.ORDERS)} orders, bf16 and fp32 output")


@pytest.mark.parametrize("dtype", [G.BF, G.F8], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("family", G.STRUCTURED)
def test_structured_family_stays_inside_the_bound_under_every_summation_order(family, dtype):
    c = structured(family, dtype)
    T = 2.0 * c["n"] * G.U24 * c["S"]
    worst, use = 0.0, 0.0
    for order in G.ORDERS:
        acc = G.model_accumulate(c["a"], c["w"], order)
        for out, dt in (("bf16", G.BF), ("f32", torch.float32)):
            r = outside(G.model_epilogue(acc, c["bias"], c["temb"], c["res"], out=out), c, dt)
            assert r["outside"] == 0 and r["worst"] <= 1.0, (family, order, out, r)
            worst = max(worst, r["worst"])
        o32 = torch.from_numpy(G.model_epilogue(acc, c["bias"], c["temb"], c["res"], out="f32")).double()
        use = max(use, float(((o32 - c["ref"]).abs() / T).max()))
    print(f"structured {family} ({'bf16' if dtype == G.BF else 'e4m3'} operands): err/bound {worst:.3f}, share of T the fp32 accumulator uses {use:.3f}")
    assert use <= 0.5              # (n - 1) 2^-24 S is half of T: the model rounds to nearest


# ------------------------------------------------------------------------------------------------ mutations
def flagged_exact(name, o):
    return not same_bits(o, exact(name)["exp_bf16"])


@pytest.mark.parametrize("mutate", ["truncate", "acc_bf16", "bias_bf16"])
def test_rounding_mutations_are_flagged(mutate):
    """truncation instead of RNE; the accumulator rounded to bf16 before the residual add (a double rounding); the bias rounded to bf16 before the add"""
    for name in ("bias+row+residual", "gains+bias+residual", "e4m3 MX", "conv S1"):
        c = exact(name)
        o = run(c["a"], c["w"], "block32", c["bias"], c["temb"], c["res"], mutate=mutate)
        n = int((o != c["exp_bf16"]).sum())
        print(f"{mutate}, exact {name}: {n} of {o.size} elements differ")
        assert n > 0, (mutate, name)
    for family in G.STRUCTURED:
        c = structured(family)
        r = outside(run(c["a"], c["w"], "block32", c["bias"], c["temb"], c["res"], mutate=mutate), c)
        print(f"{mutate}, structured {family}: err/bound {r['worst']:.2f} at {r['index']}, {r['outside']} outside")
        assert r["outside"] > 0, (mutate, family, r)


def test_dropped_k_slice_of_one_row_block_is_flagged():
    """the last 32 K values of rows 32 .. 63 never reach the accumulator"""
    for name in ("plain", "gains", "e4m3 per-row"):
        c = exact(name)
        a = c["a"].copy()
        a[32:64, K - 32:] = 0
        o = run(a, c["w"], "block32", c["bias"], c["temb"], c["res"])
        assert flagged_exact(name, o) and same_bits(o[:32], c["exp_bf16"][:32]), name
    for family in G.STRUCTURED:
        c = structured(family)
        a = c["a"].copy()
        a[32:64, K - 32:] = 0
        r = outside(run(a, c["w"], "block32", c["bias"], c["temb"], c["res"]), c)
        print(f"dropped K slice, structured {family}: err/bound {r['worst']:.1f} at {r['index']}, {r['outside']} outside")
        assert r["outside"] > 0 and 32 <= r["index"][0] < 64, (family, r)


def test_mx_block_exponent_off_by_one_is_flagged():
    """block 2 of row 5 read with the next exponent"""
    c = exact("e4m3 MX")
    a = c["a"].copy()
    a[5, 64:96] *= 2
    o = run(a, c["w"], "block32", c["bias"], c["temb"], c["res"])
    assert flagged_exact("e4m3 MX", o) and same_bits(np.delete(o, 5, 0), np.delete(c["exp_bf16"], 5, 0))
    for family in G.STRUCTURED:
        c = structured(family, G.F8)
        a = c["a"].copy()
        a[5, 64:96] *= 2
        r = outside(run(a, c["w"], "block32", c["bias"], c["temb"], c["res"]), c)
        print(f"MX exponent, structured {family}: err/bound {r['worst']:.1f} at {r['index']}, {r['outside']} outside")
        assert r["outside"] > 0 and r["index"][0] == 5, (family, r)


def test_clamped_border_tap_is_flagged():
    """a border tap that reads the nearest pixel instead of zero"""
    for name, mode in (("conv S1", G.S1), ("conv S2", G.S2), ("conv UP2", G.UP2)):
        c, m = exact(name), _exact_conv(mode, border="clamp")
        o = run(m["a"], c["w"], "block64", c["bias"], c["temb"], c["res"])
        assert flagged_exact(name, o), name
    c = structured_conv()
    ok = outside(run(np32(G.im2col(c["x"], G.S1)), c["w"], "block64", c["bias"]), c)
    assert ok["outside"] == 0, ok
    r = outside(run(np32(G.im2col(c["x"], G.S1, "clamp")), c["w"], "block64", c["bias"]), c)
    print(f"clamped border, structured conv: err/bound {r['worst']:.1f} at {r['index']}, {r['outside']} outside")
    assert r["outside"] > 0, r


def test_rows_exchanged_inside_a_tile_are_flagged_where_todays_close_is_blind():
    """rows 0 and 32 of `quiet_rows` (gains 2^-12 and 2^-5; the loudest rows carry 2^12) change places.  close() of test_ops_gpu.py takes its atol from the
    largest element of the whole output and PASSES the exchanged result; the per-element bound does not"""
    from test_ops_gpu import close
    c = structured("quiet_rows")
    o = run(c["a"], c["w"], "block32", c["bias"], c["temb"], c["res"])
    swapped = o.copy()
    swapped[[0, 32]] = o[[32, 0]]
    a, w = torch.from_numpy(c["a"]), torch.from_numpy(c["w"])
    ref32 = a @ w.T + torch.from_numpy(c["bias"]) + torch.from_numpy(c["temb"]) + torch.from_numpy(c["res"])          # the fp32 reference today's tests form
    close(torch.from_numpy(swapped).to(G.BF), ref32)                                                                        # does not raise
    assert outside(o, c)["outside"] == 0
    r = outside(swapped, c)
    print(f"rows 0 <-> 32 of quiet_rows: close() passes; err/bound {r['worst']:.0f} at {r['index']}, {r['outside']} outside")
    assert r["outside"] > 0 and r["index"][0] in (0, 32), r
    e = exact("gains")
    oe = run(e["a"], e["w"], "block32")
    assert same_bits(oe, e["exp_bf16"])
    oe[[0, 32]] = oe[[32, 0]]
    assert flagged_exact("gains", oe)
