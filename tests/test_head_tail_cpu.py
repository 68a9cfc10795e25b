"""The checker of test_head_tail_numerics_gpu.py has teeth -- shown without a GPU, on numpy models of the kernels' chains as the code has them
(head_tail_cases.py: conv_in's sequential fp32 chain from the bias and its persistent tile loop, conv_out's MFMA chain in blocks of 32 through
gemm_cases.model_accumulate, linear_small's lane chains and butterfly, the sections form's stores, the embedding's fp32 chain).

  * exact family: every builder's precondition holds (gemm_cases.expected: sum |terms| < 2^24 units, so every fp32 partial sum is an integer below 2^24 in any
    order, the pre-map's chain included) and every conv_in case exercises the rounding (>= 30 % inexact, ties present); the models return the expected bits;
  * structured family: the models stay inside every bound; the shares they use are printed and recorded in head_tail_cases.py's docstring;
  * every mutation is flagged.  Cases failed, of the cases of its family this file runs (exact + structured; the counts are asserted):
      conv_in   output truncated instead of RNE 41 of 41 . bias rounded to bf16 before the chain 41 of 41 . input rounded to bf16 before the convolution 30 of 41
                (the structured ones: the exact integers are bf16 numbers) . pre-map bias applied to padding taps 7 of 7 (the pre-map cases) . last ragged tile
                dropped 35 of 41 (every case whose pixels are no multiple of 64) . tiles at or above the grid cap dropped, a single-trip loop, 7 of 41 (the looped ones)
      conv_out  padded filter rows stored 21 of 27 (Cout 16 has none; with one image the stores land in the NaN guard behind the tensor and are flagged there) .
                bias of channel 0 for every channel 26 of 27 (Cout 1 has no other) . a border predicate off by one column 26 of 27 (a single pixel has no next one)
      linear    lane loop stops at K / 512 * 512: 70 of 70 (K = 2816 loses its last 256 values, every K below 512 all of them) . section base from the launch's
                rows 1 of 2 (M = 37; at M = 4 the launch is the whole) . `add` indexed with the section width 2 of 2 (on the model only: the kernel takes the
                operand in the sections form, tmix_linear_small_sections passes none)
      embedding exponent j / (half - 1): 9 of 12 (dim 2 has one frequency) . [sin | cos] order 12 of 12 . a 2^-12-accurate exponential 9 of 12 .
                a float32 2 pi in the argument reduction 12 of 12 (159 periods at t = 999, where j = 0 grants the sine's own 2^-23 only)
"""
import numpy as np
import pytest
import torch

import head_tail_cases as HT

G = HT.G
f32 = np.float32
_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def same_bits(o, e):
    o, e = np.ascontiguousarray(o, f32), np.ascontiguousarray(e.float().numpy() if torch.is_tensor(e) else e, f32)
    return o.shape == e.shape and np.array_equal(o.view(np.uint32), e.view(np.uint32))


def inside(out, ref, bound):
    r = HT.check(torch.from_numpy(np.ascontiguousarray(out)), ref, bound)
    return r["outside"] == 0 and r["worst"] <= 1.0, r


# ------------------------------------------------------------------------------------------------ the cases this file runs
CONV_IN_EXACT_CPU = HT.CONV_IN_EXACT + HT.CONV_IN_LOOPED[:2]          # (the third looped case: its precondition only -- 17 M outputs through a 36-step numpy chain)
CONV_IN_STRUCT_CPU = [(f, s) for s in HT.CONV_IN_STRUCTURED for f in HT.FAMILIES]
CONV_OUT_STRUCT_CPU = [(f, s) for s in HT.CONV_OUT_STRUCTURED for f in HT.FAMILIES]
LINEAR_STRUCT_CPU = [(f, nk, act) for nk in HT.LINEAR_NK for f in HT.LIN_FAMILIES for act in (False, True)]
LINEAR_M_CPU = 5                       # (rows are independent: four rows next to the quiet one)


def conv_in_cases():
    """(name, case, shape, ('exact', expected bf16) or ('bound', None)) of every conv_in case of this file"""
    def build():
        out = [(f"exact {s}", HT.exact_conv_in(s), s, "exact") for s in CONV_IN_EXACT_CPU]
        out += [(f"exact pre {s}", HT.exact_conv_in(s, pre=True), s, "exact") for s in HT.CONV_IN_PRE]
        out += [(f"{f} {s}", HT.structured_conv_in(f, s), s, "bound") for f, s in CONV_IN_STRUCT_CPU]
        out += [(f"{f} pre {HT.CONV_IN_STRUCTURED[1]}", HT.structured_conv_in(f, HT.CONV_IN_STRUCTURED[1], pre=True), HT.CONV_IN_STRUCTURED[1], "bound") for f in HT.FAMILIES]
        return out
    return cached("conv_in", build)


def conv_out_cases():
    def build():
        out = [(f"exact {s}", HT.exact_conv_out(s), s, "exact") for s in HT.CONV_OUT_EXACT]
        return out + [(f"{f} {s}", HT.structured_conv_out(f, s), s, "bound") for f, s in CONV_OUT_STRUCT_CPU]
    return cached("conv_out", build)


def linear_cases():
    """(name, operands, bias, add, acts, kind, expected or (ref, T, bound))"""
    def build():
        out = []
        for N, K in HT.LINEAR_NK:
            c = HT.exact_linear(N, K)
            out.append((f"exact {N}x{K} plain", c, None, None, False, "exact", c["exp_plain"]))
            out.append((f"exact {N}x{K} bias+add", c, c["bias"], c["add"], False, "exact", c["exp_full"]))
        for f, (N, K), act in LINEAR_STRUCT_CPU:
            c = HT.structured_linear(f, LINEAR_M_CPU, N, K)
            out.append((f"{f} {N}x{K} act {act}", c, c["bias"], c["add"], act, "bound", HT.linear_bound(c["x"], c["w"], c["bias"], c["add"], act, act)))
        return out
    return cached("linear", build)


def flagged_conv_in(c, shape, kind, mutate):
    o = HT.model_conv_in(c, shape, mutate)
    if kind == "exact":
        return not same_bits(o, c["exp_bf16"])
    return not inside(o, c["ref"], c["bound"])[0]


def flagged_conv_out(c, shape, kind, mutate):
    o, guard = HT.model_conv_out(c, shape, mutate)
    if not np.isnan(guard).all():
        return True
    if kind == "exact":
        return not same_bits(o, c["exp_f32"])
    return not inside(o, c["ref"], c["bound"])[0]


def flagged_linear(case, mutate):
    _, c, bias, add, act, kind, want = case
    o = HT.model_linear(c["x"].numpy(), c["w"].float().numpy(), None if bias is None else bias.numpy(), None if add is None else add.numpy(), act, act, mutate)
    if kind == "exact":
        return not same_bits(o, want[:o.shape[0]])
    return not inside(o, want[0], want[2])[0]


# ------------------------------------------------------------------------------------------------ exact family: preconditions, rounding shares, the models' bits
def test_exact_preconditions_hold_and_conv_in_exercises_the_rounding():
    """every builder asserts its precondition in gemm_cases.expected; here: all of them build, and the rounding shares of every conv_in case"""
    shapes = [(s, False) for s in HT.CONV_IN_EXACT + HT.CONV_IN_LOOPED + [HT.CONV_IN_LARGEST] + [(1, 4, 6, 10, c) for c in HT.CONV_IN_LDS_WALK]]
    for s, pre in shapes + [(s, True) for s in HT.CONV_IN_PRE]:
        c = HT.exact_conv_in(s, pre=pre)
        ties, inexact = G.rounding_share(c["ref"])
        print(f"conv_in {s}{' pre' if pre else ''}: {c['ref'].numel()} outputs, largest |ref| {float(c['ref'].abs().max()):.0f}, ties {ties:.3f}, inexact {inexact:.3f}")
        assert inexact >= 0.3 and ties > 0, (s, pre, ties, inexact)
        if pre:
            assert bool((c["pre_b"] != 0).all()) and bool((c["pre_w"] == c["pre_w"].round()).all())
    for s in HT.CONV_OUT_EXACT:
        HT.exact_conv_out(s)
    for N, K in HT.LINEAR_NK:
        HT.exact_linear(N, K)
    for M in (4, 37):
        HT.exact_sections(M)


def test_launch_geometry_of_the_cases_is_what_their_comments_say():
    assert [HT.conv_in_smem(s[1], s[4]) for s in HT.CONV_IN_EXACT[2:5]] == [46080, 92160, 73728]
    assert [HT.conv_in_grid_cap(s[1], s[4]) for s in HT.CONV_IN_EXACT[2:5]] == [768, 256, 512]
    for s, tiles, cap in zip(HT.CONV_IN_LOOPED, (775, 258, 515), (768, 256, 512)):
        assert HT.conv_in_tiles(s[0], s[2], s[3]) == tiles and HT.conv_in_grid_cap(s[1], s[4]) == cap
    assert [(s[0] * s[2] * s[3]) % 64 for s in HT.CONV_IN_LOOPED] == [0, 62, 46]            # (49,600 pixels are 775 whole tiles; the other two end ragged)
    assert HT.conv_in_smem(4, 1056) == 152064 <= 150 * 1024 < HT.conv_in_smem(4, 1088) == 156672
    assert HT.conv_in_smem(4, 640) == 92160
    assert HT.section_starts() == [0, 5, 325, 328, 1608]


def test_models_return_the_bits_of_the_exact_family():
    for name, c, s, kind in conv_in_cases():
        if kind == "exact":
            assert same_bits(HT.model_conv_in(c, s), c["exp_bf16"]), name
    for name, c, s, kind in conv_out_cases():
        if kind == "exact":
            for order in ("sequential", "block32", "reversed"):
                o, guard = HT.model_conv_out(c, s, order=order)
                assert same_bits(o, c["exp_f32"]) and np.isnan(guard).all(), (name, order)
    for case in linear_cases():
        if case[5] == "exact":
            assert not flagged_linear(case, None), case[0]
    for M in (4, 37):
        c = HT.exact_sections(M)
        y0 = HT.model_linear(c["x"].numpy(), c["w"].float().numpy(), c["bias"].numpy())
        flat = HT.model_sections(y0, c["starts"])
        assert same_bits(flat[:y0.size], HT.sections_flat(c["exp_bias"], c["starts"])) and np.isnan(flat[y0.size:]).all(), M


# ------------------------------------------------------------------------------------------------ structured family: the models inside the bounds
def test_conv_in_model_stays_inside_the_bound():
    use = {False: 0.0, True: 0.0}
    worst = 0.0
    for name, c, s, kind in conv_in_cases():
        if kind == "bound":
            o = HT.model_conv_in(c, s)
            ok, r = inside(o, c["ref"], c["bound"])
            u = HT.t_use(torch.from_numpy(o), c["ref"], c["T"])
            assert ok, (name, r)
            use["pre_w" in c], worst = max(use["pre_w" in c], u), max(worst, r["worst"])
    print(f"conv_in model: err/bound {worst:.3f}, share of T used {use[False]:.3f} (pre-map {use[True]:.3f})")
    assert max(use.values()) <= 0.25


def test_conv_out_model_stays_inside_the_bound():
    use, worst = 0.0, 0.0
    for name, c, s, kind in conv_out_cases():
        if kind == "bound":
            for order in ("sequential", "block32", "reversed"):
                o, _ = HT.model_conv_out(c, s, order=order)
                ok, r = inside(o, c["ref"], c["bound"])
                assert ok, (name, order, r)
                use, worst = max(use, HT.t_use(torch.from_numpy(o), c["ref"], c["T"], torch.float32)), max(worst, r["worst"])
    print(f"conv_out model: err/bound {worst:.3f}, share of T used {use:.3f}")
    assert use <= 0.25


def test_linear_model_stays_inside_the_bound():
    use, worst = {False: 0.0, True: 0.0}, 0.0
    for case in linear_cases():
        name, c, bias, add, act, kind, want = case
        if kind == "bound":
            o = HT.model_linear(c["x"].numpy(), c["w"].float().numpy(), bias.numpy(), add.numpy(), act, act)
            ok, r = inside(o, want[0], want[2])
            assert ok, (name, r)
            use[act], worst = max(use[act], HT.t_use(torch.from_numpy(o), want[0], want[1], torch.float32)), max(worst, r["worst"])
    print(f"linear_small model: err/bound {worst:.3f}, share of T used {use[False]:.3f} (acts off) {use[True]:.3f} (acts on)")
    assert max(use.values()) <= 0.25


def test_silu_restatement_stays_inside_silu_eps_on_a_dense_grid():
    """the CPU restatement of silu_f over [-30, 30], 2^20 + 1 points, the exponential correctly rounded and one ulp off either way"""
    x = np.linspace(-30.0, 30.0, 2 ** 20 + 1).astype(f32)
    xd = torch.from_numpy(x).double()
    ref, eps = HT.silu64(xd), HT.silu_eps(xd)
    for nudge in (0, 1, -1):
        rel = ((torch.from_numpy(HT.model_silu(x, nudge)).double() - ref).abs() / ref.abs().clamp_min(1e-300))[xd != 0]
        share = float((rel / eps[xd != 0]).max())
        print(f"silu_f restatement, exponential {nudge:+d} ulp: largest relative error {float(rel.max()):.3g}, largest share of silu_eps {share:.3f}")
        assert share <= 1.0
    s = torch.sigmoid(xd)
    slope = float((s * (1.0 + xd * (1.0 - s))).abs().max())                    # silu'
    print(f"largest |silu'| on the grid {slope:.4f}")
    assert slope <= HT.SILU_SLOPE


def embed_cases():
    return [(dim, count) for dim in HT.EMBED_DIMS for count in HT.EMBED_COUNTS]


def test_embedding_model_stays_inside_the_bound():
    use, use1 = 0.0, 0.0
    for dim, count in embed_cases():
        v = HT.embed_values(count)
        ref, A, bound = HT.embed_reference(v, dim)
        o = HT.model_embedding(v.numpy(), dim)
        ok, r = inside(o, ref, bound)
        assert ok, (dim, count, r)
        use = max(use, HT.embed_use(torch.from_numpy(o), ref, A), *([r["worst"]] if dim > 2 else []))
        o1 = [HT.model_embedding(v.numpy(), dim, nudge=s) for s in (1, -1)]
        assert all(inside(t, ref, bound)[0] for t in o1), (dim, count)
        use1 = max(use1, *(HT.check(torch.from_numpy(t), ref, bound)["worst"] for t in o1))
        if dim == 2:
            assert float((torch.from_numpy(o).double() - ref).abs().max()) <= 2.0 ** -24        # one frequency, f = 1: the sine's rounding alone
    print(f"embedding model: largest err/bound {use:.3f} (every function one ulp off: {use1:.3f})")
    assert use <= 0.7


# ------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mutate,count", [("truncate", 41), ("bias_bf16", 41), ("x_bf16", 30), ("pre_bias_in_padding", 7), ("drop_ragged_tile", 35), ("single_trip", 7)])
def test_conv_in_mutations_are_flagged(mutate, count):
    cases = [t for t in conv_in_cases() if mutate != "pre_bias_in_padding" or "pre_w" in t[1]]
    hit = [name for name, c, s, kind in cases if flagged_conv_in(c, s, kind, mutate)]
    print(f"conv_in {mutate}: {len(hit)} of {len(cases)} cases fail: {hit}")
    assert len(hit) == count >= 1, (mutate, len(hit))
    if mutate == "single_trip":
        assert all(any(str(s) in h for s in HT.CONV_IN_LOOPED) for h in hit)
    if mutate == "x_bf16":
        assert all(not h.startswith("exact") for h in hit)


@pytest.mark.parametrize("mutate,count", [("padded_rows_stored", 21), ("bias_channel0", 26), ("border_column", 26)])
def test_conv_out_mutations_are_flagged(mutate, count):
    cases = conv_out_cases()
    hit = [name for name, c, s, kind in cases if flagged_conv_out(c, s, kind, mutate)]
    print(f"conv_out {mutate}: {len(hit)} of {len(cases)} cases fail: {hit}")
    assert len(hit) == count >= 1, (mutate, len(hit))


def test_linear_lane_loop_mutation_is_flagged():
    cases = linear_cases()
    hit = [c[0] for c in cases if flagged_linear(c, "lane_loop_whole_rounds")]
    print(f"linear_small lane loop stops at K / 512 * 512: {len(hit)} of {len(cases)} cases fail")
    assert any("2816" in h for h in hit) and len(hit) == len(cases)


@pytest.mark.parametrize("mutate,fails", [("base_launch_rows", (37,)), ("add_section_width", (4, 37))])
def test_sections_mutations_are_flagged(mutate, fails):
    hit = []
    for M in (4, 37):
        c = HT.exact_sections(M)
        y0 = HT.model_linear(c["x"].numpy(), c["w"].float().numpy(), c["bias"].numpy())
        want = HT.sections_flat(c["exp_full"], c["starts"])
        assert same_bits(HT.model_sections(y0, c["starts"], c["add"].numpy())[:y0.size], want), M         # (the model with the operand, unmutated)
        flat = HT.model_sections(y0, c["starts"], c["add"].numpy(), mutate=mutate)
        if not (same_bits(flat[:y0.size], want) and np.isnan(flat[y0.size:]).all()):
            hit.append(M)
    print(f"sections {mutate}: M in {hit} fail")
    assert tuple(hit) == fails


@pytest.mark.parametrize("mutate,fails", [("exponent_half_minus_1", 9), ("sin_cos_order", 12), ("exp_2^-12", 9), ("two_pi_f32", 12)])
def test_embedding_mutations_are_flagged(mutate, fails):
    hit = []
    for dim, count in embed_cases():
        v = HT.embed_values(count)
        ref, _, bound = HT.embed_reference(v, dim)
        if not inside(HT.model_embedding(v.numpy(), dim, mutate), ref, bound)[0]:
            hit.append((dim, count))
    print(f"embedding {mutate}: {len(hit)} of {len(embed_cases())} cases fail: {hit}")
    assert len(hit) == fails >= 1, (mutate, hit)
