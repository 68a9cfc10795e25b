"""The attention family against an fp64 reference with a derived per-element bound, at the logit scales the models run at.

The other attention tests draw Q, K and V from unit Gaussians: logit std ~1, a nearly flat softmax, where an accuracy loss on the logits is
invisible.  attn1 of SDXL and of the video UNet runs at a logit std of several units with a few dominant keys.  Every input set here is run at Q
gains that realise a logit std of 1, 4, 8 and 16 (asserted), on structured inputs (loud V channels, a sink key, a diagonal band of matching keys).

Reference (torch.float64, from the bf16 input values):  P = softmax(scale * Q K^T),  O = P V,  A = P |V|.

Bound, per element:  |out - O| <= 2^-7 * A + 2^-9 * |O|.   Derivation:
  * P enters the second MFMA rounded to bf16: relative error 2^-9 on every p_j, so at most 2^-9 * sum_j p_j |v_j| = 2^-9 * A on the numerator
    (the row sum is formed from the same rounded values, or differs from them by 2^-9 relative: the same size again at most);
  * the output is rounded once to bf16: 2^-9 * |O|, and |O| <= A;
  * the fp32 score accumulation, exp2 and the key-split merge are orders of magnitude below these (2^-24 relative per operation);
  * a further factor 2 sits on the first term (numerator and denominator both carry the P rounding): 2 * 2 * 2^-9 = 2^-7.
A CPU model of this pipeline with Q rounded once uses at most 0.70 of the bound at every logit scale.  The bound is NOT tuned to the device.

Q rounded once: tmix_attn_fwd* is launched in its negative-scale form (Q already in log2 units, times a power of two: exact in bf16).  The
positive-scale form multiplies Q by scale * log2(e) and rounds it to bf16 a second time; it is kept for outside callers, documented in
include/tmix.h, and checked here at logit std 1 only.  Measured on an MI355X, largest err / bound over the cases of a family
(every test prints its figure before it asserts):

    positive scale (Q rounded twice; the arithmetic every launch had before the negative form existed: the same figures came from the library of
    the commit before it), by logit std 1 / 4 / 8 / 16:
        attn_small_kernel                          0.52 / 2.61 / 6.27 / 13.2
        attn_fwd_pipe_kernel                       0.52 / 2.10 / 4.79 / 12.0
        attn_fwd_pipe_kernel, short key set        0.45 / 2.14 / 4.04 / 7.86
        key-split tail (split launch)              0.68 / 3.08 / 7.71 / 15.0
    negative scale (Q rounded once), by logit std 1 / 4 / 8 / 16:
        attn_small_kernel                          0.39 / 0.60 / 0.61 / 0.57
        attn_fwd_pipe_kernel                       0.40 / 0.55 / 0.57 / 0.55
        attn_fwd_pipe_kernel, short key set        0.39 / 0.50 / 0.54 / 0.52
        key-split tail (split and unsplit)         0.40 / 0.64 / 0.70 / 0.72
    tmix_gemm_q_cross_attn                         0.40 / 0.56 / 0.57 / 0.59
    tmix_temporal_attn (frames 9 and 16)           0.58 / 0.68 / 0.68 / 0.67
"""
import math

import pytest
import torch

from test_ops_gpu import BF, _mx_quantize, lib_env, ops  # noqa: F401  (lib_env, ops: fixtures)

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
SCALE = 0.125                       # head_dim 64
STDS = (1, 4, 8, 16)                # logit standard deviations (per query row, over the keys) every input set is run at
FAMILIES = ("gauss", "loud_v", "sink_first", "sink_last", "band")


# ------------------------------------------------------------------------------------------------ inputs
def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed), dtype=torch.float32)


def _smooth(x, rho, dim=1):
    """AR(1) along `dim` with unit marginal variance: neighbouring rows are similar (correlation rho per step)"""
    out = x.clone()
    rows = out.unbind(dim)
    c = math.sqrt(1 - rho * rho)
    for i in range(1, len(rows)):
        rows[i].copy_(rho * rows[i - 1] + c * rows[i])
    return out


def family_qkv(family, B, H, Sq, Skv, seed):
    """fp32 q [B, Sq, H*64], k, v [B, Skv, H*64] of one input family at unit gain (logit std about 1 before `with_logit_std` sets it)"""
    Cc = H * 64
    q, k, v = _randn(B, Sq, Cc, seed=seed), _randn(B, Skv, Cc, seed=seed + 1), _randn(B, Skv, Cc, seed=seed + 2)
    if family == "loud_v":                      # non-zero mean and loud channels: cancellation in P V, and A >> |O| off the loud channels
        v = v + 0.5
        v[:, :, 5] *= 40.0
        v[:, :, Cc - 27] *= 40.0
    elif family in ("sink_first", "sink_last"):
        # every query carries the same component 6 u (u = the unit vector along (1, ..., 1) of a head), one key is 16 u: its logit is 12 +- 2 at unit
        # gain against a background of std 1.25 -- it dominates every row.  Once in the first 64-key tile, once in the last (and ragged) one
        u = torch.full((64,), 0.125).repeat(H)
        q = q + 6.0 * u
        k[:, 1 if family == "sink_first" else Skv - 2] = 16.0 * u
    elif family == "band":
        # k varies smoothly along the key axis and q_i ~ k_m(i), m(i) = i * Skv / Sq: large positive q.k on a diagonal band that decays over ~50 keys, so
        # for most rows the tile maxima rise tile after tile up to the band (the running maximum of the online softmax moves at every tile)
        k = _smooth(k, 0.98)
        m = (torch.arange(Sq) * Skv) // Sq
        q = k[:, m] + 0.5 * q
    else:
        assert family == "gauss"
    return q, k, v


def heads(t, H):
    return t.reshape(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def row_logit_std(q, k, H, scale):
    """standard deviation of the logits of a query row over its keys, averaged over all rows (fp64)"""
    s = scale * heads(q.double(), H) @ heads(k.double(), H).transpose(2, 3)
    return float(s.std(dim=-1, unbiased=False).mean())


def with_logit_std(q32, k_bf, H, target, unit):
    """q32 (fp32, cuda) times the gain that makes the logit std `target`, times `unit` (log2(e) for the log2-unit form), rounded to bf16 ONCE"""
    gain = target / row_logit_std(q32, k_bf, H, SCALE)
    return (q32 * (gain * unit)).to(BF)


def make_inputs(family, B, H, Sq, Skv, std, log2_units, seed=7000):
    """(q, k, vt, v) bf16 on the device, the scale argument of the launch and the scale of the reference (natural units, for the q handed out).  The
    realised logit std of what the kernel is given is asserted: the inputs cannot drift back to the flat-softmax regime"""
    q32, k32, v32 = [t.cuda() for t in family_qkv(family, B, H, Sq, Skv, seed)]
    k, v = k32.to(BF), v32.to(BF)
    q = with_logit_std(q32, k, H, std, LOG2E if log2_units else 1.0)
    ref_scale = SCALE / LOG2E if log2_units else SCALE
    got = row_logit_std(q, k, H, ref_scale)
    assert 0.9 * std <= got <= 1.1 * std, (family, std, got)
    ld = (Skv + 7) // 8 * 8
    vt = torch.zeros(B, H * 64, ld, device="cuda", dtype=BF)
    vt[:, :, :Skv] = v.transpose(1, 2)
    return q, k, vt, v, (-SCALE if log2_units else SCALE), ref_scale


# ------------------------------------------------------------------------------------------------ reference and bound
def reference(q, k, v, H, scale):
    """(O, A) in fp64, [B, Sq, H*64]: O = softmax(scale q k^T) v, A = softmax(scale q k^T) |v|, from the values the tensors hold"""
    qh, kh, vh = heads(q.double(), H), heads(k.double(), H), heads(v.double(), H)
    p = torch.softmax(scale * qh @ kh.transpose(2, 3), dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(q.shape[0], q.shape[1], H * 64)
    return back(p @ vh), back(p @ vh.abs())


def err_over_bound(out, O, A):
    """max over the elements of |out - O| / (2^-7 A + 2^-9 |O|)"""
    assert out.shape == O.shape and torch.isfinite(out.float()).all()
    bound = 2.0 ** -7 * A + 2.0 ** -9 * O.abs()
    assert float(bound.min()) > 0.0
    return float(((out.double() - O).abs() / bound).max())


def launch_workgroups(fn):
    """run fn (one instrumented launch) inside a tmix_prof_begin / tmix_prof_end bracket with per-workgroup detail: (result, workgroups that ran it)"""
    from tweediemix_amd import lib as L
    lib = L.load()
    slots = torch.zeros(1, 8, dtype=torch.int64, device="cuda")
    slots[:, 0] = -1
    torch.cuda.synchronize()
    L.check(lib.tmix_prof_begin(slots.data_ptr(), 1, 1), "tmix_prof_begin")
    try:
        out = fn()
    finally:
        n = lib.tmix_prof_end()
    torch.cuda.synchronize()
    assert n == 1, n
    return out, int(slots[0, 5])


def small_kernel_workgroups(B, H, Sq):
    waves = (Sq + 63) // 64 * B * H                    # attn_small_kernel: one wave per 64 queries of a (batch, head), four per workgroup while that
    assert (waves + 3) // 4 <= 256                     # is no worse than five -- true while one round of 256 CUs takes them all
    return (waves + 3) // 4


def pipe_kernel_workgroups(B, H, Sq):
    return (Sq + 127) // 128 * B * H                   # attn_fwd_pipe_kernel: one workgroup per 128 queries of a (batch, head)


# kernel, (B, H, Sq, Skv), TMIX_ATTN_GENERAL
ATTN_SHAPES = [("small", (2, 3, 200, 77), False), ("small", (1, 2, 70, 33), False),
               ("pipe", (2, 2, 256, 256), False), ("pipe", (1, 2, 200, 320), False),
               ("pipe", (1, 3, 128, 77), True)]          # the pipelined kernel on a short key set: one full tile + a ragged one of 13 keys


def run_attention(ops, family, shape, std, log2_units, ws=None):
    """one launch of tmix_attn_fwd_ws on an input set -> (out bf16, err / bound)"""
    B, H, Sq, Skv = shape
    q, k, vt, v, scale, ref_scale = make_inputs(family, B, H, Sq, Skv, std, log2_units)
    out = ops.attention(q, k, vt, H, Skv, scale, ws=ws)
    O, A = reference(q, k, v, H, ref_scale)
    return out, err_over_bound(out, O, A), (q, k, vt, scale)


@pytest.mark.parametrize("kernel,shape,general", ATTN_SHAPES)
def test_shapes_select_the_kernel_they_are_meant_for(ops, lib_env, kernel, shape, general):
    """the two kernels cover their queries with different workgroup counts (64 queries per wave / 128 per workgroup): the count the timing hook reports
    for a launch says which one ran.  The negative-scale form changes nothing about the choice"""
    B, H, Sq, Skv = shape
    if general:
        lib_env("TMIX_ATTN_GENERAL")
    q, k, vt, v, scale, _ = make_inputs("gauss", B, H, Sq, Skv, 4, True)
    _, n = launch_workgroups(lambda: ops.attention(q, k, vt, H, Skv, scale))
    want = small_kernel_workgroups(B, H, Sq) if kernel == "small" else pipe_kernel_workgroups(B, H, Sq)
    other = pipe_kernel_workgroups(B, H, Sq) if kernel == "small" else small_kernel_workgroups(B, H, Sq)
    assert want != other and n == want, (n, want, other)


@pytest.mark.parametrize("std", STDS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernel,shape,general", ATTN_SHAPES)
def test_attention_meets_the_fp64_bound_with_q_rounded_once(ops, lib_env, kernel, shape, general, family, std):
    """tmix_attn_fwd_ws, negative-scale form (Q in log2 units): |out - O| <= 2^-7 A + 2^-9 |O| per element against fp64 (module docstring) on both
    kernels, ragged query and key counts, one and several tiles, at logit std 1 .. 16"""
    if general:
        lib_env("TMIX_ATTN_GENERAL")
    _, r, _ = run_attention(ops, family, shape, std, True)
    print(f"{kernel} {shape} {family} std {std}: err / bound = {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernel,shape,general", ATTN_SHAPES)
def test_attention_positive_scale_form_meets_the_bound_at_unit_logits(ops, lib_env, kernel, shape, general, family):
    """the positive-scale form (Q times scale * log2(e), rounded to bf16 a second time) keeps its meaning and its arithmetic; at logit std 1 the second
    rounding stays inside the bound (beyond that it does not: include/tmix.h, and the figures in the module docstring)"""
    if general:
        lib_env("TMIX_ATTN_GENERAL")
    _, r, _ = run_attention(ops, family, shape, 1, False)
    print(f"{kernel} {shape} {family} std 1, positive scale: err / bound = {r:.3f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ key-split tail
SPLIT_SHAPE = (8, 65, 128, 512)      # 520 items of 128 queries: 512 fill the slots, the 8 behind them are cut into 4 key ranges of 2 tiles


def test_key_split_shape_is_the_smallest_that_splits():
    """queried, not assumed: no item count below 520 splits at any key count up to 512, and 520 items do not split below 512 keys"""
    from tweediemix_amd import lib as L
    l = L.load()
    B, H, Sq, Skv = SPLIT_SHAPE
    assert l.tmix_attn_split_ws_bytes(B, H, Sq, Skv) == 4096 + 8 * 4 * 4 * 9 * 64 * 16
    for items in range(1, 520):
        for skv in range(64, 513, 64):
            assert l.tmix_attn_split_ws_bytes(1, items, 128, skv) == 0, (items, skv)
    for skv in range(1, 512):
        assert l.tmix_attn_split_ws_bytes(B, H, Sq, skv) == 0, skv


@pytest.mark.parametrize("std", STDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_key_split_tail_meets_the_fp64_bound(ops, family, std):
    """split and unsplit launches of the same inputs both meet the bound; the split one really split (workgroup count 512 + 8 * 4: with a sink key
    the softmax is one-hot and both forms return the sink's V row bit for bit, so the outputs cannot tell), equals the unsplit one outside the
    tail items, and leaves its tickets at zero"""
    B, H, Sq, Skv = SPLIT_SHAPE
    ws = ops.attention_split_ws(B, H, Sq, Skv, "cuda")
    assert ws is not None
    q, k, vt, v, scale, ref_scale = make_inputs(family, B, H, Sq, Skv, std, True)
    O, A = reference(q, k, v, H, ref_scale)
    base, n_base = launch_workgroups(lambda: ops.attention(q, k, vt, H, Skv, scale))
    out, n_split = launch_workgroups(lambda: ops.attention(q, k, vt, H, Skv, scale, ws=ws))
    assert (n_base, n_split) == (520, 512 + 8 * 4)
    assert int(ws[:4096].view(torch.int32).abs().sum()) == 0
    tail = slice((H - 8) * 64, H * 64)                       # the last 8 heads of the last batch row are the 8 tail items
    assert torch.equal(out[:B - 1], base[:B - 1]) and torch.equal(out[B - 1, :, :tail.start], base[B - 1, :, :tail.start])
    r0, r1 = err_over_bound(base, O, A), err_over_bound(out, O, A)
    r1t = err_over_bound(out[B - 1:, :, tail], O[B - 1:, :, tail], A[B - 1:, :, tail])
    print(f"split {SPLIT_SHAPE} {family} std {std}: err / bound unsplit {r0:.3f}, split {r1:.3f} (tail items alone {r1t:.3f})")
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)


# ------------------------------------------------------------------------------------------------ e4m3 output
@pytest.mark.parametrize("std", STDS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernel,shape", [("small", (2, 3, 200, 77)), ("pipe", (1, 2, 200, 320))])
def test_attention_e4m3_output_equals_the_quantised_bf16_output_at_large_logits(ops, kernel, shape, family, std):
    """tmix_attn_fwd_f8: bytes and scales equal _mx_quantize of the bf16 result of the same launch, one shape per kernel, on the large-logit inputs"""
    B, H, Sq, Skv = shape
    Cc = H * 64
    out, r, (q, k, vt, scale) = run_attention(ops, family, shape, std, True)
    assert r <= 1.0, r
    cp = ops.F8Copy(B * Sq, Cc, "cuda")
    cp.buf.fill_(0x5a)
    ops.attention(q, k, vt, H, Skv, scale, f8_out=cp)
    torch.cuda.synchronize()
    qq, ss, _deq = _mx_quantize(out.float().view(B * Sq, Cc))
    assert torch.equal(cp.scales, ss)
    same = (cp.q == qq) | (((cp.q & 0x7f) == 0) & ((qq & 0x7f) == 0))
    assert same.all(), int((~same).sum())


# ------------------------------------------------------------------------------------------------ attn2 in one launch
def _dyadic(x, step, lim):
    """x rounded to multiples of `step` (a power of two) and clipped to +-lim: sums of products of such values are exact in fp32 in any order"""
    return (torch.round(x / step) * step).clamp(-lim, lim)


def qattn_inputs(family, std, seed=7100):
    """tmix_gemm_q_cross_attn at (B, S, C, Skv) = (2, 128, 640, 77): the input families of the kernels above, with the logit scale produced by
    amplifying the to_q weight (and its bias).  The kernel forms q in registers and rounds (a w^T + bias) * scale * log2(e) to bf16 once; to compare
    against fp64 'from the bf16 values' that rounding has to be reproduced exactly, so the activations, weights and bias are dyadic (multiples of
    1/8, 1/64, 1/64, bounded): the fp32 accumulator then holds a w^T + bias exactly in any summation order (asserted), and one fp32 multiply and
    one bf16 rounding in torch give the very q the kernel uses."""
    B, S, C, Skv = 2, 128, 640, 77
    H = C // 64
    a = _randn(B, S, C, seed=seed)
    if family == "band":
        a = _smooth(a, 0.9)                                           # neighbouring queries are similar
    a = _dyadic(a, 1 / 8, 4.0)
    w1 = _randn(C, C, seed=seed + 1) * C ** -0.5                      # to_q at unit gain
    b1 = torch.zeros(C)
    k, v = _randn(B, Skv, C, seed=seed + 2), _randn(B, Skv, C, seed=seed + 3)
    if family == "loud_v":
        v = v + 0.5
        v[:, :, 5] *= 40.0
        v[:, :, C - 27] *= 40.0
    elif family in ("sink_first", "sink_last"):
        u = torch.full((64,), 0.125).repeat(H)
        b1 = 6.0 * u
        k[:, 1 if family == "sink_first" else Skv - 2] = 16.0 * u
    elif family == "band":
        m = (torch.arange(Skv) * S) // Skv
        k = (a @ w1.t())[:, m] + 0.5 * k                              # k_j ~ q_i(j)
    k = k.to(BF)
    gain = std / row_logit_std(a @ w1.t() + b1, k, H, SCALE)          # the amplification of to_q that realises the logit std
    w, bias = _dyadic(w1 * gain, 1 / 64, 8.0), _dyadic(b1 * gain, 1 / 64, 64.0)
    a, w, bias, k, v = a.to(BF).cuda(), w.to(BF).cuda(), bias.cuda(), k.cuda(), v.to(BF).cuda()
    q64 = a.double() @ w.double().t() + bias.double()
    assert torch.equal(q64.float().double(), q64) and float(q64.abs().max()) * 512 < 2 ** 24          # exact in fp32: multiples of 2^-9, 24 bits at most
    c = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)           # the kernel's fp32 factor scale * LOG2E
    q_used = (q64.float() * c.cuda()).to(BF)                          # log2 units, rounded once
    vt = torch.zeros(B, C, 80, device="cuda", dtype=BF)
    vt[:, :, :Skv] = v.transpose(1, 2)
    return a.view(B * S, C), w, bias, k, vt, v, q_used, H, S, Skv


@pytest.mark.parametrize("std", STDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_q_cross_attn_meets_the_fp64_bound(ops, family, std):
    """tmix_gemm_q_cross_attn rounds q once: the same bound against fp64 from the bf16 values the kernel works on (qattn_inputs)"""
    a, w, bias, k, vt, v, q_used, H, S, Skv = qattn_inputs(family, std)
    ref_scale = math.log(2.0)                                         # q_used is in log2 units with the scale in it: logit = ln 2 * q_used . k
    got_std = row_logit_std(q_used, k, H, ref_scale)
    assert 0.9 * std <= got_std <= 1.1 * std, (family, std, got_std)
    out = ops.gemm_q_cross_attn(a, w, k, vt, S, SCALE, bias=bias).view(q_used.shape)
    O, A = reference(q_used, k, v, H, ref_scale)
    r = err_over_bound(out, O, A)
    print(f"q_cross_attn {family} std {std} (realised {got_std:.2f}): err / bound = {r:.3f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ attention over the frame axis
@pytest.mark.parametrize("std", STDS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("frames", [9, 16])
def test_temporal_attention_meets_the_fp64_bound(ops, frames, family, std):
    """tmix_temporal_attn (frames 9 and 16, hw = 37, 5 heads; it scales fp32 scores): the sequences are the frames of a pixel"""
    clips, hw, heads_ = 2, 37, 5
    C = heads_ * 64
    # family_qkv with batch = pixels and sequence = frames, then to the kernel's layout [(clips * frames), hw, 3 C]
    q32, k32, v32 = [t.cuda() for t in family_qkv(family, clips * hw, heads_, frames, frames, 7200)]
    k, v = k32.to(BF), v32.to(BF)
    q = with_logit_std(q32, k, heads_, std, 1.0)
    got_std = row_logit_std(q, k, heads_, SCALE)
    assert 0.9 * std <= got_std <= 1.1 * std, (family, std, got_std)
    qkv = torch.cat([q, k, v], dim=2).view(clips, hw, frames, 3 * C).transpose(1, 2).reshape(clips * frames, hw, 3 * C).contiguous()
    out = ops.temporal_attention(qkv, clips, frames, heads_)
    out = out.view(clips, frames, hw, C).transpose(1, 2).reshape(clips * hw, frames, C)
    O, A = reference(q, k, v, heads_, SCALE)
    r = err_over_bound(out, O, A)
    print(f"temporal_attn frames {frames} {family} std {std}: err / bound = {r:.3f}")
    assert r <= 1.0, r
