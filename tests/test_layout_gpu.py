"""Guard bands, strided views and poisoned padding for every kernel entry of include/tmix.h.

test_ops_gpu.py compares results with fp32 references on dense, exactly-sized tensors.  Here every case runs its launch twice:
  run D  dense tensors, as there (plus ONE close(D, reference) with that file's constants, so this file stands alone)
  run F  the same values with every output in an output frame (tests/layout_frames.py: NaN-payload sentinel around the logical view), every device input in an
         input frame with NaN poison around it, 64 elements in front, ld = width + 8 (outputs: the width rounded up to the widest tile, + 8), three extra rows
         between batch slices
and asserts: F is bit-equal to D; no guard element of an output changed; every element of an output was written; no input buffer changed.
Nothing here relies on a fault: the frames are sized so that a whole unmasked workgroup tile (256 x 320, the largest tmix_gemm_tile_shape reports) stays inside them.

entry -> case
  tmix_gemm_bf16                    test_gemm_bias_residual, _geglu, _gelu, _f32_output, _transposed_region, _row_statistics_and_folded_layernorm, _column_statistics,
                                    _e4m3_copy, _periodic_weight_sets, test_sensitivity_gemm_extra_row
  tmix_gemm_fp8                     test_gemm_fp8_row_scales, _block_scales, _geglu_e4m3_output
  tmix_gemm_q_cross_attn            test_q_cross_attn
  tmix_quantize_fp8_rows            test_quantize_fp8_rows
  tmix_conv3x3_nhwc                 test_conv3x3_modes, test_conv3x3_halo, test_conv_s2a_against_padded_stride_2_conv, test_sensitivity_conv_extra_channels
  tmix_conv3x3_nhwc_fp8             test_conv3x3_fp8
  tmix_conv_in / _pre / tmix_conv_out   test_conv_in_out
  tmix_attn_fwd[_ws] / _f8[_ws]     test_attention, test_attention_e4m3_output, test_attention_split_workspace, test_sensitivity_attention_extra_query
  tmix_xattn_token_maps             test_xattn_token_maps
  tmix_groupnorm_nhwc / _pre / _pre_f8  test_groupnorm
  tmix_layernorm, tmix_concat_channels, tmix_timestep_embedding, tmix_affine_clamp, tmix_zero      test_layernorm, test_small_dense_entries
  tmix_softmax_rows / _causal / _masked  test_softmax_rows, test_softmax_rows_causal_and_masked_against_torch
  tmix_temporal_attn                test_temporal_attn
  tmix_lora_down                    test_lora_down
  tmix_linear_small / _sections     test_linear_small
  tmix_fused_tweedie_step / _dev, tmix_step_prologue     test_tweedie_step, test_tweedie_step_dev_and_prologue
  tmix_vpred_step / _dev, tmix_video_step_prologue, tmix_frame_inject    test_video_step_entries
  tmix_conv3x3_f32, tmix_adaptive_avgpool_f32, tmix_linear_f32, tmix_i2v_temporal_encoder   test_conditioning_entries
A new entry gets a line here and a case that frames every pointer it takes.

For byte outputs (e4m3, E8M0) "every element written" follows from the bit-equality with run D: 0x5A, the byte sentinel, is also a legitimate e4m3 value.
When this file was added it had been exercised against a CPU emulation of the header's semantics only, not yet on an MI355X: a case that fails on the shipped
kernels is a finding (a missing mask, an ld / stride mix-up, or a contract sentence include/tmix.h still lacks), not a reason to loosen the case.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from layout_frames import Frame, dense_guarded, round_up

pytestmark = pytest.mark.gpu

BF, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
TILE_ROWS, TILE_COLS = 256, 320          # the largest workgroup tile of any tiling (test_frame_tile_bound_covers_every_tiling)


@pytest.fixture
def lib_env():
    """set one of the library's environment switches mid-process (see test_ops_gpu.py).  Restored on teardown."""
    from tweediemix_amd import lib as L
    saved = {}

    def set_(name, value="1"):
        saved.setdefault(name, os.environ.get(name))
        os.environ[name] = value
        L.load().tmix_env_refresh()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    L.load().tmix_env_refresh()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tweediemix_amd import lib, ops as O
    lib.check(lib.load().tmix_check_device(), "tmix_check_device")
    return O


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """a failed comparison is a finding and the file goes on; a device fault is not: nothing more is launched after one (the store is found from the code and the frame
    sizes first)"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001 -- whatever the runtime raises for a faulted queue
        pytest.exit(f"device fault, nothing more is launched: {e}", returncode=3)


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def close(out, ref, rtol=2 ** -7, atol_frac=2e-3):
    out = out.float()
    ref = ref.float()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    atol = atol_frac * ref.abs().max().item() + 1e-6
    err = (out - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    assert not bad.any(), f"max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g}), {int(bad.sum())} bad"


def _mx_quantize(x):
    """torch reference of the MX block form: x fp32 [rows, K] -> (e4m3 bytes [rows, K], E8M0 scales [K/32, rows], dequantised fp32)"""
    rows, K = x.shape
    xb = x.view(rows, K // 32, 32)
    amax = xb.abs().amax(dim=2)
    e = torch.where(amax > 0, torch.ceil(torch.log2(amax.double() / 448.0)).float(), torch.zeros_like(amax))
    q = (xb * torch.exp2(-e).unsqueeze(2)).to(torch.float8_e4m3fn).view(torch.uint8).view(rows, K)
    return q.contiguous(), (e + 127).to(torch.uint8).t().contiguous(), (q.view(torch.float8_e4m3fn).float().view(rows, K // 32, 32)
                                                                        * torch.exp2(e).unsqueeze(2)).view(rows, K)


def _e4m3_same(a, b):
    return bool(((a == b) | (((a & 0x7f) == 0) & ((b & 0x7f) == 0))).all())          # +0 / -0 both fine


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- run D / run F
class Dense:
    """run D: plain contiguous tensors (dense_ld: the row stride an entry fixes by a shape parameter, e.g. row_channels)"""
    framed = False

    def inp(self, data, dense_ld=None, **kw):
        if dense_ld is None:
            return data.contiguous()
        buf = torch.zeros(*data.shape[:-1], dense_ld, dtype=data.dtype, device=data.device)
        buf[..., :data.shape[-1]] = data
        return buf[..., :data.shape[-1]]

    def out(self, shape, dtype, dense_ld=None, **kw):
        if dense_ld is None:
            return torch.zeros(*shape, dtype=dtype, device="cuda")
        return torch.zeros(*shape[:-1], dense_ld, dtype=dtype, device="cuda")[..., :shape[-1]]

    def inout(self, data, dense_ld=None, **kw):
        return self.inp(data, dense_ld).clone() if dense_ld is None else self.inp(data, dense_ld)

    def scratch(self, n, dtype, zero=False):
        return torch.zeros(n, dtype=dtype, device="cuda")

    def check(self):
        torch.cuda.synchronize()


class Framed:
    """run F: every tensor a view into its own guarded allocation"""
    framed = True

    def __init__(self):
        self.ins, self.outs, self.inouts = [], [], []

    @staticmethod
    def _layout(shape, esize, ld, batch_stride, gap_rows, dense, width_to=0):
        """ld = width + 8 elements (16 for bytes: the header's alignment rules stay met), batch stride = three extra rows"""
        if dense or len(shape) == 1 or len(shape) > 3:
            return None, None
        al = 16 // esize
        cols, rows = shape[-1], shape[-2]
        if ld is None:
            ld = round_up(max(cols, round_up(cols, width_to) if width_to else cols) + 8, al)
        if batch_stride is None and len(shape) == 3:
            batch_stride = (rows + gap_rows) * ld
        return ld, batch_stride

    def inp(self, data, ld=None, batch_stride=None, gap_rows=3, dense=False, front=64, tail_rows=32, poison=None, prep=None, name="input", dense_ld=None):
        ld, batch_stride = self._layout(tuple(data.shape), data.element_size(), ld, batch_stride, gap_rows, dense)
        f = Frame.of(data, ld=ld, batch_stride=batch_stride, front=front, tail_rows=tail_rows, poison=poison, name=name)
        if prep is not None:
            prep(f)
        self.ins.append(f.seal())
        return f.view

    def out(self, shape, dtype, ld=None, batch_stride=None, gap_rows=3, dense=False, front=64, tile=(TILE_ROWS, 0), name="output", dense_ld=None, written=True):
        esize = torch.empty(0, dtype=dtype).element_size()
        if dense or len(shape) == 1 or len(shape) > 3:
            f = dense_guarded(shape, dtype, rows=2 * TILE_ROWS + 88 if len(shape) > 1 else 2, front=front, device="cuda", name=name)
        else:
            ld, batch_stride = self._layout(tuple(shape), esize, ld, batch_stride, gap_rows, False, width_to=tile[1])
            f = Frame(shape, dtype, ld=ld, batch_stride=batch_stride, front=front, tail_rows=tile[0] + gap_rows, device="cuda", name=name)
        (self.outs if written else self.inouts).append(f)
        return f.view

    def inout(self, data, ld=None, batch_stride=None, gap_rows=3, dense=False, front=64, tile=(TILE_ROWS, 0), name="in/out", dense_ld=None):
        """a tensor the entry updates in place: the data in the view, the sentinel around it"""
        v = self.out(tuple(data.shape), data.dtype, ld=ld, batch_stride=batch_stride, gap_rows=gap_rows, dense=dense, front=front, tile=tile, name=name, written=False)
        v.copy_(data)
        return v

    def scratch(self, n, dtype, zero=False):
        """a workspace the entry owns between launches: only its surroundings are checked"""
        v = self.out((n,), dtype, name="workspace", written=False)
        if zero:
            v.zero_()
        return v

    def check(self):
        torch.cuda.synchronize()
        for f in self.ins:
            f.assert_unchanged()
        for f in self.outs + self.inouts:
            f.assert_untouched()
        for f in self.outs:
            if f.dtype != U8:       # 0x5A is also a legitimate e4m3 byte (20.0): for byte outputs "all written" follows from the bit-equality with run D instead
                f.assert_all_written()


def pair(fn):
    """run fn(maker) dense and framed; every returned tensor must be bit-equal between the two, every other returned value equal.  Returns run D's results."""
    d = Dense()
    rd = fn(d)
    d.check()
    f = Framed()
    rf = fn(f)
    f.check()
    rd, rf = (rd if isinstance(rd, tuple) else (rd,)), (rf if isinstance(rf, tuple) else (rf,))
    assert len(rd) == len(rf)
    for i, (x, y) in enumerate(zip(rd, rf)):
        if torch.is_tensor(x):
            assert x.shape == y.shape and torch.equal(x, y), f"result {i}: the framed run differs from the dense run in {int((x != y).sum())} of {x.numel()} elements"
        else:
            assert x == y, (i, x, y)
    return rd


def test_frame_tile_bound_covers_every_tiling(ops):
    """the frames' tail guard and row stride come from the largest tile tmix_gemm_tile_shape reports"""
    from tweediemix_amd import lib as L
    lib = L.load()
    for cfg in range(1, L.TILE_COUNT + 1):
        bm, bn = C.c_int(0), C.c_int(0)
        if lib.tmix_gemm_tile_shape(cfg, C.byref(bm), C.byref(bn)) == 0:
            assert 0 < bm.value <= TILE_ROWS and 0 < bn.value <= TILE_COLS, (cfg, bm.value, bn.value)


# --------------------------------------------------------------------------- tmix_gemm_bf16
GEMM_SHAPES = [(77, 200, 128, 1), (129, 320, 192, 3)]        # ragged in M for every tile height; the first ragged in N for every tile width; the second with per-slice weights
ALL_IDS = list(range(1, 24))


def _launch_gemm(d, scales=None):
    """resolve, launch; returns the id of the kernel that ran"""
    from tweediemix_amd import lib as L
    lib = L.load()
    runs = lib.tmix_gemm_resolve_tile(C.byref(d), 0 if scales is None else 1)
    assert runs > 0, (runs, lib.tmix_last_error_string())
    if scales is None:
        L.check(lib.tmix_gemm_bf16(C.byref(d), _st()), "tmix_gemm_bf16")
    else:
        L.check(lib.tmix_gemm_fp8(C.byref(d), _p(scales[0]), _p(scales[1]), _st()), "tmix_gemm_fp8")
    return runs


def _gemm_operands(M, N, K, batch, seed=1, wsets=None):
    shp = (batch, M) if batch > 1 else (M,)
    wsets = batch if wsets is None else wsets
    a = rnd(*shp, K, seed=seed)
    w = rnd(*((wsets,) if wsets > 1 else ()), N, K, seed=seed + 1, scale=K ** -0.5)
    return a, w


def _ref_mm(a, w):
    if w.dim() == 3 and a.dim() == 3 and w.shape[0] != a.shape[0]:
        w = w[torch.arange(a.shape[0], device=w.device) % w.shape[0]]
    return torch.einsum("...mk,...nk->...mn", a.float(), w.float())


def _out_tile():
    return (TILE_ROWS, TILE_COLS)


@pytest.mark.parametrize("cfg", ALL_IDS)
@pytest.mark.parametrize("M,N,K,batch", GEMM_SHAPES)
def test_gemm_bias_residual(ops, cfg, M, N, K, batch):
    """lda / strideA, ldw / strideW, ldc / strideC, ldr / strideR, strideBias: bias + residual on every tiling"""
    a, w = _gemm_operands(M, N, K, batch)
    bias = rnd(*((batch,) if batch > 1 else ()), N, seed=5, dtype=F32)
    res = rnd(*a.shape[:-1], N, seed=6)

    def run(m):
        out = m.out((*a.shape[:-1], N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), residual=m.inp(res), tile_cfg=cfg)
        return out, _launch_gemm(d)
    out, _ = pair(run)
    close(out, _ref_mm(a, w) + (bias[:, None] if batch > 1 else bias) + res.float())


GEGLU_IDS = ALL_IDS[:22] + [24]
GEGLU_CASES = [(c, 77, 192, 128, 1) for c in GEGLU_IDS] + [(c, 129, 320, 192, 3) for c in GEGLU_IDS] + [(24, 256, 320, 128, 1)]


@pytest.mark.parametrize("cfg,M,N,K,batch", GEGLU_CASES)
def test_gemm_geglu(ops, cfg, M, N, K, batch):
    """GEGLU: C is N/2 wide (ragged for every tile width at N = 192); 256 x 320 x 128 is the smallest shape of the persistent path's own test (id 24)"""
    from tweediemix_amd.weights import interleave_geglu
    a, w = _gemm_operands(M, N, K, batch, seed=8, wsets=1)
    b = rnd(N, seed=10, dtype=F32)
    wi, bi = interleave_geglu(w, b)

    def run(m):
        out = m.out((*a.shape[:-1], N // 2), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(wi), out, bias=m.inp(bi), geglu=True, tile_cfg=cfg)
        return out, _launch_gemm(d)
    out, _ = pair(run)
    y = a.float() @ w.float().T + b
    close(out, y[..., :N // 2] * F.gelu(y[..., N // 2:]))


@pytest.mark.parametrize("cfg", [1, 21, 23])
@pytest.mark.parametrize("M,N,K,batch", GEMM_SHAPES)
def test_gemm_gelu(ops, cfg, M, N, K, batch):
    a, w = _gemm_operands(M, N, K, batch, seed=14)
    bias = rnd(N, seed=15, dtype=F32)

    def run(m):
        out = m.out((*a.shape[:-1], N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), act="gelu", tile_cfg=cfg)
        return out, _launch_gemm(d)
    out, _ = pair(run)
    close(out, F.gelu(_ref_mm(a, w) + bias))


@pytest.mark.parametrize("cfg", [1, 2, 4, 6, 7, 13, 14, 16, 17, 18, 21, 22])
@pytest.mark.parametrize("M,N,K,batch", GEMM_SHAPES)
def test_gemm_f32_output(ops, cfg, M, N, K, batch):
    """TMIX_EPI_F32OUT: fp32 C with ld >= N"""
    a, w = _gemm_operands(M, N, K, batch, seed=17)

    def run(m):
        out = m.out((*a.shape[:-1], N), F32, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), None, out_f32=out, tile_cfg=cfg)
        return out, _launch_gemm(d)
    out, _ = pair(run)
    torch.testing.assert_close(out, _ref_mm(a, w), rtol=1e-4, atol=1e-4)          # fp32 accumulation of bf16 products, K <= 192, |values| ~ 1


@pytest.mark.parametrize("cfg", ALL_IDS[:22])
@pytest.mark.parametrize("M,N,K,batch,ntb", [(77, 200, 128, 1, 128), (129, 384, 192, 3, 256)])
def test_gemm_transposed_region(ops, cfg, M, N, K, batch, ntb):
    """columns >= n_trans_begin leave transposed: Ct[b][n - ntb][m] with ldct > M and strideCt.  Columns [M, ldct) of Ct are not the launch's to write."""
    a, w = _gemm_operands(M, N, K, batch, seed=11)

    def run(m):
        out = m.out((*a.shape[:-1], ntb), BF, tile=_out_tile())
        # (run D keeps 16-byte rows too, ldct = M rounded up to 8, so that both runs take the same staged epilogue)
        ct = m.out((*((batch,) if batch > 1 else ()), N - ntb, M), BF, tile=(TILE_COLS, TILE_ROWS), name="Ct", dense_ld=round_up(M, 8))
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, out_t=ct, n_trans_begin=ntb, tile_cfg=cfg)
        return out, ct, _launch_gemm(d)
    out, ct, _ = pair(run)
    ref = _ref_mm(a, w)
    close(out, ref[..., :ntb])
    close(ct, ref[..., ntb:].transpose(-1, -2))


def _stats_frames(m, parts, batch, M, name):
    """fp32 {sum, sumsq} [parts][ld rows][2], slice b `stride` floats in: framed as [parts][batch][2 M] with a slice stride of M + 3 rows and ld > batch * (M + 3);
    an unmasked 256-row tile of the last slice stays inside its own part"""
    stride = 2 * (M + 3)
    ld_rows = (batch - 1) * (M + 3) + TILE_ROWS + 8
    return dict(ld=stride, batch_stride=2 * ld_rows, tile=((2 * (TILE_ROWS + 8)) // stride + 2, 0), name=name)


LN_IDS = [1, 2, 4, 7, 8, 9, 10, 13, 14, 15, 20, 21, 22, 23]
LN_CASES = [(c, 77, 200, 128, 1) for c in LN_IDS] + [(c, 129, 320, 192, 3) for c in LN_IDS] + [(23, 77, 160, 64, 2)]


@pytest.mark.parametrize("cfg,M,N,K,batch", LN_CASES)
def test_gemm_row_statistics_and_folded_layernorm(ops, cfg, M, N, K, batch):
    """producer: row_stats_out with ldStatsOut > batch * M and a non-dense strideStatsOut; consumer: ln_stats / ln_colsum read from that very layout
    ((77, 160, 64, 2): the smallest shape of tiling 23's own test)"""
    from tweediemix_amd.weights import fold_layernorm
    a, w = _gemm_operands(M, N, K, batch, seed=70)
    bias = rnd(N, seed=72, dtype=F32)
    res = rnd(*a.shape[:-1], N, seed=73) * 2 + 0.7
    parts = ops.stats_parts(N, cfg)

    def produce(m):
        out = m.out((*a.shape[:-1], N), BF, tile=_out_tile())
        st = m.out((parts, batch, 2 * M), F32, **_stats_frames(m, parts, batch, M, "row_stats_out"))
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), residual=m.inp(res), tile_cfg=cfg)
        d.row_stats_out, d.strideStatsOut, d.ldStatsOut = st.data_ptr(), st.stride(1), st.stride(0) // 2
        return out, st, _launch_gemm(d)
    h, st, _ = pair(produce)
    hf = h.float().reshape(batch * M, N)
    close(h, _ref_mm(a, w) + bias + res.float())
    s = st.reshape(parts, batch * M, 2).sum(0)
    torch.testing.assert_close(s[:, 0], hf.sum(-1), rtol=1e-5, atol=2e-3)
    torch.testing.assert_close(s[:, 1], (hf ** 2).sum(-1), rtol=1e-5, atol=2e-3)
    if N % 64:
        return
    N2 = 200
    gamma, beta = rnd(N, seed=74, dtype=F32) * 0.2 + 1, rnd(N, seed=75, dtype=F32) * 0.3
    w2 = rnd(*((batch,) if batch > 1 else ()), N2, N, seed=76, scale=N ** -0.5)
    b2 = rnd(*((batch,) if batch > 1 else ()), N2, seed=77, dtype=F32)
    wp, cs, t = fold_layernorm(w2, gamma, beta, b2)

    def consume(m):
        out = m.out((*a.shape[:-1], N2), BF, tile=_out_tile())
        sti = m.inp(st, **{k: v for k, v in _stats_frames(m, parts, batch, M, "ln_stats").items() if k != "tile"})
        d = ops.make_gemm_desc(m.inp(h), m.inp(wp), out, bias=m.inp(t), tile_cfg=cfg)
        csv = m.inp(cs)
        d.ln_stats, d.strideLnStats, d.ldLnStats, d.ln_parts = sti.data_ptr(), sti.stride(1), sti.stride(0) // 2, parts
        d.ln_colsum, d.strideLnColsum = csv.data_ptr(), (csv.stride(0) if batch > 1 else 0)
        d.ln_inv_c, d.ln_eps = 1.0 / N, 1e-5
        return out, _launch_gemm(d)
    y, _ = pair(consume)
    ref = torch.einsum("...mk,...nk->...mn", F.layer_norm(h.float(), (N,), gamma, beta, 1e-5), w2.float()) + (b2[:, None] if batch > 1 else b2)
    close(y, ref, rtol=2 ** -6, atol_frac=4e-3)


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 7, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22])
def test_gemm_column_statistics(ops, cfg):
    """col_stats_out is dense by contract ([M / 32][2][N]): the frame adds the guards"""
    M, N, K = 96, 200, 128
    a, w = _gemm_operands(M, N, K, 1, seed=61)
    bias = rnd(N, seed=63, dtype=F32)

    def run(m):
        out = m.out((M, N), BF, tile=_out_tile())
        cs = m.out((M // 32, 2, N), F32, dense=True, name="col_stats_out")
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), tile_cfg=cfg, col_stats_out=cs)
        return out, cs, _launch_gemm(d)
    out, cs, _ = pair(run)
    close(out, _ref_mm(a, w) + bias)
    blk = out.double().reshape(M // 32, 32, N)
    ref = torch.stack([blk.sum(1), (blk * blk).sum(1)], 1)
    err = (cs.double() - ref).abs()
    assert (err <= 1e-5 * ref.abs() + 1e-5 * ref[:, 1:].sqrt().max() + 1e-6).all(), err.max().item()


@pytest.mark.parametrize("cfg", [1, 4, 7, 12, 13, 17, 18])
@pytest.mark.parametrize("batch", [1, 2])
def test_gemm_e4m3_copy(ops, cfg, batch):
    """TMIX_F8_COPY_OUT with ldct > N (the descriptor by hand: F8Copy.attach fixes ldct = N): bytes [batch * M][ldct] and, strideCt bytes behind them, the scale
    array [N / 32][batch * M] -- two frames in one allocation"""
    from tweediemix_amd import lib as L
    M, N, K = 96, 224, 128
    a, w = _gemm_operands(M, N, K, batch, seed=20)
    bias = rnd(N, seed=22, dtype=F32)
    rows = batch * M

    def run(m):
        out = m.out((*a.shape[:-1], N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), tile_cfg=cfg)
        if m.framed:
            ldct = round_up(round_up(N, TILE_COLS) + 8, 16)
            fq = Frame((rows, N), U8, ld=ldct, front=64, tail_rows=TILE_ROWS + 3, device="cuda", name="e4m3 copy")
            fs = Frame((N // 32, rows), U8, front=64, tail_rows=TILE_COLS // 32 + 8, device="cuda", name="copy scales")     # dense by contract: ld = batch * M
            both = torch.empty(fq.numel + fs.numel, dtype=U8, device="cuda")       # the ABI addresses the scales relative to Ct: one allocation
            fq = Frame((rows, N), U8, ld=ldct, front=64, tail_rows=TILE_ROWS + 3, device="cuda", name="e4m3 copy", storage=both[:fq.numel])
            fs = Frame((N // 32, rows), U8, front=64, tail_rows=TILE_COLS // 32 + 8, device="cuda", name="copy scales", storage=both[fq.numel:])
            m.outs += [fq, fs]
            q, s = fq.view, fs.view
            d.Ct, d.ldct, d.strideCt = q.data_ptr(), ldct, s.data_ptr() - q.data_ptr()
        else:
            cp = ops.F8Copy(rows, N, "cuda")
            cp.attach(d)
            q, s = cp.q, cp.scales
        d.reserved0 |= L.F8_COPY_OUT
        return out, q, s, _launch_gemm(d)
    out, q, s, _ = pair(run)
    close(out, _ref_mm(a, w) + bias)
    qq, ss, _deq = _mx_quantize(out.float().view(rows, N))
    assert torch.equal(s, ss) and _e4m3_same(q, qq)


@pytest.mark.parametrize("cfg", [2, 4, 7, 12, 13, 14, 16, 17, 19, 20, 21, 23])
def test_gemm_periodic_weight_sets(ops, cfg):
    """w_period: four batch slices over two stored weight sets (slice b reads set b % 2), per-set bias, all strides non-dense"""
    M, N, K, batch, P = 129, 320, 192, 4, 2
    a, w = _gemm_operands(M, N, K, batch, seed=301, wsets=P)
    bias = rnd(P, N, seed=303, dtype=F32)
    res = rnd(batch, M, N, seed=304)

    def run(m):
        out = m.out((batch, M, N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a), m.inp(w), out, bias=m.inp(bias), residual=m.inp(res), tile_cfg=cfg)
        assert d.w_period == P
        return out, _launch_gemm(d)
    out, _ = pair(run)
    idx = torch.arange(batch, device="cuda") % P
    close(out, _ref_mm(a, w) + bias[idx][:, None] + res.float())


# --------------------------------------------------------------------------- tmix_gemm_fp8
FP8_IDS = [12, 16, 17, 19, 20, 21]


@pytest.mark.parametrize("cfg", FP8_IDS)
def test_gemm_fp8_row_scales(ops, cfg):
    """e4m3 bytes with lda / ldw multiples of 16, one E8M0 scale per A row and W row: the scale arrays framed too"""
    M, N, K = 300, 264, 128
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    a8, sa = ops.quantize_fp8_rows(a)
    w8, sw = ops.quantize_fp8_rows(w)
    bias = rnd(N, seed=3, dtype=F32)

    def run(m):
        out = m.out((M, N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a8), m.inp(w8), out, bias=m.inp(bias), tile_cfg=cfg)
        return out, _launch_gemm(d, (m.inp(sa), m.inp(sw)))
    out, _ = pair(run)
    close(out, ops.dequantize_fp8_rows(a8, sa) @ ops.dequantize_fp8_rows(w8, sw).t() + bias)


@pytest.mark.parametrize("cfg", FP8_IDS)
@pytest.mark.parametrize("batch", [1, 2])
def test_gemm_fp8_block_scales(ops, cfg, batch):
    """TMIX_F8_A_BLOCK_SCALES: scale_a = [K / 32][batch * M] (dense by contract: guards only), bias + residual"""
    from tweediemix_amd import lib as L
    M, N, K = 300, 264, 128
    a = rnd(batch * M, K, seed=1, dtype=F32)
    a[:, 64:96] *= 37.0
    w = rnd(batch, N, K, seed=2, scale=K ** -0.5)
    a8, sa, ad = _mx_quantize(a)
    w8, sw = ops.quantize_fp8_rows(w.view(batch * N, K))
    wd = ops.dequantize_fp8_rows(w8, sw).view(batch, N, K)
    bias = rnd(N, seed=3, dtype=F32)
    res = rnd(batch, M, N, seed=4)

    def run(m):
        out = m.out((batch, M, N), BF, tile=_out_tile())
        d = ops.make_gemm_desc(m.inp(a8.view(batch, M, K)), m.inp(w8.view(batch, N, K)), out, bias=m.inp(bias), residual=m.inp(res), tile_cfg=cfg)
        d.reserved0 = L.F8_A_BLOCK_SCALES
        return out, _launch_gemm(d, (m.inp(sa, dense=True), m.inp(sw.view(batch, N), dense=True)))
    out, _ = pair(run)
    close(out, torch.einsum("bmk,bnk->bmn", ad.view(batch, M, K), wd) + bias + res.float())


@pytest.mark.parametrize("cfg", [16, 17])
def test_gemm_fp8_geglu_e4m3_output(ops, cfg):
    """TMIX_F8_GEGLU_OUT: C = e4m3 bytes [M][N / 2] with ldc > N / 2, Ct = the scale plane [N / 64][ldct > batch * M]"""
    from tweediemix_amd import lib as L
    from tweediemix_amd.weights import interleave_geglu
    M, N, K = 300, 256, 128
    a = rnd(M, K, seed=8)
    wi, bi = interleave_geglu(rnd(N, K, seed=9, scale=K ** -0.5), rnd(N, seed=10, dtype=F32))
    a8, sa = ops.quantize_fp8_rows(a)
    w8, sw = ops.quantize_fp8_rows(wi.contiguous())
    ref_bf16 = ops.gemm_fp8(a8, sa, w8, sw, bias=bi, geglu=True, tile_cfg=cfg)

    def run(m):
        c8 = m.out((M, N // 2), U8, tile=_out_tile(), name="C (e4m3)")
        cs = m.out((N // 64, M), U8, tile=(TILE_COLS // 64 + 1, TILE_ROWS), name="Ct (scale plane)")
        d = ops.make_gemm_desc(m.inp(a8), m.inp(w8), None, bias=m.inp(bi), geglu=True, tile_cfg=cfg)
        d.C, d.ldc, d.strideC = c8.data_ptr(), c8.stride(0), 0
        d.Ct, d.ldct = cs.data_ptr(), cs.stride(0)
        d.reserved0 = L.F8_GEGLU_OUT
        return c8, cs, _launch_gemm(d, (m.inp(sa), m.inp(sw)))
    c8, cs, _ = pair(run)
    y = ops.dequantize_fp8_rows(a8, sa) @ ops.dequantize_fp8_rows(w8, sw).t() + bi
    v = y.view(M, N // 32, 2, 16)
    close(ref_bf16, (v[:, :, 0] * F.gelu(v[:, :, 1])).reshape(M, N // 2), rtol=2 ** -6)
    q, s, _deq = _mx_quantize(ref_bf16.float())
    assert torch.equal(cs, s) and _e4m3_same(c8, q)


def test_quantize_fp8_rows(ops):
    from tweediemix_amd import lib as L
    rows, K = 37, 64
    x = rnd(rows, K, seed=37, scale=3.0)
    x[1] = 0
    x[2, 5] = 1000.0

    def run(m):
        xv = m.inp(x)
        q = m.out((rows, K), U8, tile=(TILE_ROWS, 0))
        s = m.out((rows,), U8)
        L.check(L.load().tmix_quantize_fp8_rows(_p(xv), xv.stride(0), _p(q), q.stride(0), _p(s), rows, K, _st()), "tmix_quantize_fp8_rows")
        return q, s
    q, s = pair(run)
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    e = torch.where(amax > 0, torch.ceil(torch.log2(amax.double() / 448.0)).float(), torch.zeros_like(amax))
    assert torch.equal(s.float() - 127.0, e)
    assert _e4m3_same(q, (xf * torch.exp2(-e).unsqueeze(1)).to(torch.float8_e4m3fn).view(U8))


# --------------------------------------------------------------------------- tmix_attn_fwd / _f8 / _ws
def _heads(t, H):
    return t.float().reshape(t.shape[0], -1, H, 64).transpose(1, 2)


def _vt_poison(variant, Skv):
    """what lies in V^T columns [Skv, ldvt): (a) zeros, (b) +3e38 / -3e38 alternating -- the header's "finite".  Everything else around Q, K and V^T -- the K rows
    behind Skv of every slice included -- is NaN."""
    def prep(f):
        pad = f.padded[:, :, Skv:]
        if variant == "a":
            pad.zero_()
        else:
            alt = torch.where(torch.arange(pad.shape[-1], device="cuda") % 2 == 0, 3e38, -3e38).to(BF)
            pad.copy_(alt.expand_as(pad))
    return prep


def _attention_case(ops, B, H, Sq, Skv, variant, f8, ws_need=0):
    from tweediemix_amd import lib as L
    lib = L.load()
    Cc = H * 64
    q, k, v = rnd(B, Sq, Cc, seed=40), rnd(B, Skv, Cc, seed=41), rnd(B, Skv, Cc, seed=42)
    vt_data = v.transpose(1, 2).contiguous()
    ld8 = round_up(Skv, 8)

    def run(m):
        qv, kv = m.inp(q, name="Q"), m.inp(k, name="K")
        if m.framed:
            vt = m.inp(vt_data, ld=ld8 + 8, prep=_vt_poison(variant, Skv), name="Vt")
        else:
            vt = torch.zeros(B, Cc, ld8, device="cuda", dtype=BF)
            vt[:, :, :Skv] = vt_data
        ws = None
        if ws_need:
            ws = m.scratch(ws_need + 4096, U8)                    # the bytes past tmix_attn_split_ws_bytes must stay untouched
            ws[:ws_need].zero_()
            if not m.framed:
                ws[ws_need:].fill_(0x5A)
        wsa = (_p(ws), ws_need)
        if f8:
            o8 = m.out((B * Sq, Cc), U8, tile=(TILE_ROWS, 0), name="O8")
            sc = m.out((2 * H, B * Sq), U8, ld=round_up(B * Sq + TILE_ROWS + 8, 16), tile=(4, 0), name="scales")
            L.check(lib.tmix_attn_fwd_f8_ws(_p(qv), qv.stride(1), qv.stride(0), _p(kv), kv.stride(1), kv.stride(0), _p(vt), vt.stride(1), vt.stride(0),
                                            _p(o8), o8.stride(0), _p(sc), sc.stride(0), B, H, Sq, Skv, 0.125, *wsa, _st()), "tmix_attn_fwd_f8_ws")
            res = (o8, sc)
        else:
            o = m.out((B, Sq, Cc), BF, tile=(TILE_ROWS, 0), name="O")
            L.check(lib.tmix_attn_fwd_ws(_p(qv), qv.stride(1), qv.stride(0), _p(kv), kv.stride(1), kv.stride(0), _p(vt), vt.stride(1), vt.stride(0),
                                         _p(o), o.stride(1), o.stride(0), B, H, Sq, Skv, 0.125, *wsa, _st()), "tmix_attn_fwd_ws")
            res = (o,)
        if ws_need:
            torch.cuda.synchronize()
            assert int(ws[:4096].view(torch.int32).abs().sum()) == 0, "ticket counters not back at zero"
            assert bool((ws[ws_need:] == 0x5A).all()), "bytes past tmix_attn_split_ws_bytes were written"
        return res
    return pair(run), (q, k, v)


def _attention_ref(q, k, v, H):
    B, Sq, Cc = q.shape
    outs = []
    for b0 in range(0, B, 2):                                   # (fp32 scores of two batch rows at a time)
        sl = slice(b0, min(B, b0 + 2))
        outs.append(F.scaled_dot_product_attention(_heads(q[sl], H), _heads(k[sl], H), _heads(v[sl], H), scale=0.125).transpose(1, 2).reshape(-1, Sq, Cc))
    return torch.cat(outs)


ATTN_SHAPES = [(2, 3, 70, 96), (2, 2, 300, 33), (2, 1, 200, 80), (1, 2, 200, 200)]      # the last: the general kernel, ragged in both
ATTN_CASES = [(*s, False) for s in ATTN_SHAPES] + [(*s, True) for s in ATTN_SHAPES if s[3] <= 96]      # short-key shapes also under TMIX_ATTN_GENERAL


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("B,H,Sq,Skv,general", ATTN_CASES)
def test_attention(ops, lib_env, B, H, Sq, Skv, variant, general):
    """all eight strides of tmix_attn_fwd non-dense; K rows behind Skv NaN, V^T padding columns zero (a) or huge and finite (b); short-key shapes also on the
    general kernel (TMIX_ATTN_GENERAL)"""
    if general:
        lib_env("TMIX_ATTN_GENERAL")
    (out,), (q, k, v) = _attention_case(ops, B, H, Sq, Skv, variant, False)
    close(out, _attention_ref(q, k, v, H), rtol=2 ** -6, atol_frac=4e-3)


@pytest.mark.parametrize("B,H,Sq,Skv,general", ATTN_CASES)
def test_attention_e4m3_output(ops, lib_env, B, H, Sq, Skv, general):
    """tmix_attn_fwd_f8 with ldo8 > H * 64 and ldScale > B * Sq: the bytes a quantiser makes of the bf16 tensor of the dense bf16 launch"""
    if general:
        lib_env("TMIX_ATTN_GENERAL")
    (o8, sc), (q, k, v) = _attention_case(ops, B, H, Sq, Skv, "a", True)
    ld8 = round_up(Skv, 8)
    vt = torch.zeros(B, H * 64, ld8, device="cuda", dtype=BF)
    vt[:, :, :Skv] = v.transpose(1, 2)
    bf = ops.attention(q, k, vt, H, Skv, 0.125)
    close(bf, _attention_ref(q, k, v, H), rtol=2 ** -6, atol_frac=4e-3)
    qq, ss, _deq = _mx_quantize(bf.float().view(B * Sq, H * 64))
    assert torch.equal(sc, ss) and _e4m3_same(o8, qq)


@pytest.mark.parametrize("f8", [False, True])
def test_attention_split_workspace(ops, f8):
    """(4, 20, 1024, 1024): the smallest shape whose last round splits into key ranges.  Ticket counters zero afterwards, bytes past the workspace untouched."""
    from tweediemix_amd import lib as L
    B, H, S = 4, 20, 1024
    need = L.load().tmix_attn_split_ws_bytes(B, H, S, S)
    assert need > 4096
    res, (q, k, v) = _attention_case(ops, B, H, S, S, "a", f8, ws_need=need)
    if not f8:
        close(res[0], _attention_ref(q, k, v, H), rtol=2 ** -6, atol_frac=4e-3)
    else:
        ws = ops.attention_split_ws(B, H, S, S, "cuda")
        bf = ops.attention(q, k, v.transpose(1, 2).contiguous(), H, S, 0.125, ws=ws)
        qq, ss, _deq = _mx_quantize(bf.float().view(B * S, H * 64))
        assert torch.equal(res[1], ss) and _e4m3_same(res[0], qq)


# --------------------------------------------------------------------------- tmix_gemm_q_cross_attn
@pytest.mark.parametrize("routed", [True, False])
@pytest.mark.parametrize("ln", [True, False])
def test_q_cross_attn(ops, routed, ln):
    """ldk > C, strideK, strideVt, ldo > C, d->C = NULL; K rows behind the 77 keys NaN, V^T columns [77, 80) zero as the header requires"""
    from tweediemix_amd import lib as L
    from tweediemix_amd.weights import fold_layernorm
    B, S, Cc, Skv = 2, 64, 320, 77
    h = rnd(B, S, Cc, seed=501) * 1.5 + 0.3
    P = B if routed else 1
    wq = rnd(P, Cc, Cc, seed=502, scale=Cc ** -0.5)
    bq = rnd(P, Cc, seed=503, dtype=F32) * 0.1
    k = rnd(B, Skv, Cc, seed=504)
    vt_data = rnd(B, Cc, Skv, seed=505)
    scale = 64 ** -0.5
    gamma, beta = rnd(Cc, seed=506, dtype=F32) * 0.2 + 1, rnd(Cc, seed=507, dtype=F32) * 0.3
    if ln:
        fold = [fold_layernorm(wq[i], gamma, beta, bq[i]) for i in range(P)]
        wu, cs, bu = [torch.stack([f[j] for f in fold]).contiguous() for j in range(3)]
        hf = h.float()
        stats = torch.stack([hf.sum(-1), (hf ** 2).sum(-1)], -1).view(1, B * S, 2).contiguous()
    else:
        wu, bu, cs, stats = wq, bq, None, None
    if not routed:
        wu, bu, cs = wu[0], bu[0], (None if cs is None else cs[0])
    a = h if routed else h.view(B * S, Cc)

    def run(m):
        kw = {}
        if ln:
            kw = dict(ln_stats=m.inp(stats, dense=True), ln_colsum=m.inp(cs, dense=True))
        d = ops.make_gemm_desc(m.inp(a), m.inp(wu), None, bias=m.inp(bu, dense=True), **kw)
        assert not d.C
        kv = m.inp(k, name="K")
        if m.framed:
            vt = m.inp(vt_data, ld=80, prep=_vt_poison("a", Skv), name="Vt")
        else:
            vt = torch.zeros(B, Cc, 80, device="cuda", dtype=BF)
            vt[:, :, :Skv] = vt_data
        o = m.out((B * S, Cc), BF, tile=(TILE_ROWS, TILE_COLS), name="O")
        L.check(L.load().tmix_gemm_q_cross_attn(C.byref(d), _p(kv), kv.stride(1), kv.stride(0), _p(vt), vt.stride(1), vt.stride(0), _p(o), o.stride(0),
                                                S, Skv, scale, _st()), "tmix_gemm_q_cross_attn")
        return o
    (got,) = pair(run)
    # fp32 reference as test_ops_gpu.py's: q rounded to bf16 (the two-launch form stores it), softmax(q K^T scale) V per 64-wide head
    af = F.layer_norm(h.float(), (Cc,), gamma, beta, 1e-5) if ln else h.float()
    qf = torch.einsum("bmk,bnk->bmn", af, wq.float().expand(B, -1, -1) if P == 1 else wq.float()) + (bq.expand(B, -1) if P == 1 else bq)[:, None]
    qf = qf.to(BF).float()
    Hh = Cc // 64
    o = F.scaled_dot_product_attention(_heads(qf, Hh), _heads(k, Hh), vt_data.float().reshape(B, Hh, 64, Skv).transpose(2, 3), scale=scale)
    close(got, o.transpose(1, 2).reshape(B * S, Cc), rtol=2 ** -6, atol_frac=6e-3)


# --------------------------------------------------------------------------- tmix_xattn_token_maps
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("align8", [False, True])
def test_xattn_token_maps(ops, accumulate, align8):
    """Q and K framed with NaN behind Lk and behind Sq, rows (1, 2, None) of a batch of four: the map rows of the unselected batch rows do not exist, the output frame
    is exact.  align8: the 8-byte-only alignment the entry allows (4 elements in front, ld % 4 == 0 only)"""
    B, H, Sq, Lk = 4, 3, 70, 77
    tokens = [0, 5, 76]
    q, k = rnd(B, Sq, H * 64, seed=601), rnd(B, Lk, H * 64, seed=602)
    base = rnd(2, len(tokens), Sq, seed=603, dtype=F32)
    lay = dict(front=4, ld=H * 64 + 4) if align8 else {}

    def run(m):
        qv, kv = m.inp(q, name="Q", **lay), m.inp(k, name="K", **lay)
        out = m.inout(base, dense=True, front=2 if align8 else 64) if accumulate else m.out(base.shape, F32, dense=True, front=2 if align8 else 64)
        ops.xattn_token_maps(qv, kv, tokens, H, Lk=Lk, rows=(1, 2, None), out=out, accumulate=accumulate)
        return out
    (maps,) = pair(run)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float().view(B, Sq, H, 64), k.float().view(B, Lk, H, 64)) * 64 ** -0.5
    ref = torch.softmax(s, -1)[1::2][..., tokens].sum(1).transpose(1, 2)            # [rows, tok, Sq]
    err = (maps - (ref + (base if accumulate else 0))).abs().max().item()
    assert err <= 1e-4 * H, err                                                      # test_attn_masks_gpu.py's bound: fp32 summation order and exp2 rounding


# --------------------------------------------------------------------------- tmix_conv3x3_nhwc / _fp8 (dense by contract: the frames add guards only)
def _launch_conv(d, scales=None):
    from tweediemix_amd import lib as L
    lib = L.load()
    runs = lib.tmix_conv_resolve_tile(C.byref(d), 0 if scales is None else 1)
    assert runs > 0, (runs, lib.tmix_last_error_string())
    if scales is None:
        L.check(lib.tmix_conv3x3_nhwc(C.byref(d), _st()), "tmix_conv3x3_nhwc")
    else:
        L.check(lib.tmix_conv3x3_nhwc_fp8(C.byref(d), _p(scales[0]), _p(scales[1]), _st()), "tmix_conv3x3_nhwc_fp8")
    return runs


def _conv_ref(x, w, bias, mode):
    """fp32 torch reference of the five modes (x NHWC; T3: x [clips, frames, hw, Cin], w [Cout, 3, Cin])"""
    from tweediemix_amd import lib as L
    if mode == L.CONV_T3:
        clips, frames, hw, Ci = x.shape
        xt = x.float().view(clips, frames, hw, 1, Ci).permute(0, 4, 1, 2, 3)
        return F.conv3d(xt, w.float().permute(0, 2, 1)[:, :, :, None, None], bias, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(clips, frames, hw, -1)
    xn, wn = x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2)
    if mode == L.CONV_UP2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    if mode == L.CONV_S2A:
        return F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, bias, stride=2).permute(0, 2, 3, 1)
    return F.conv2d(xn, wn, bias, stride=2 if mode == L.CONV_S2 else 1, padding=1).permute(0, 2, 3, 1)


def _conv_case(ops, mode, B, H, W, Cin, Cout, cfg, seed=20, colstats=False):
    from tweediemix_amd import lib as L
    x = rnd(B, H, W, Cin, seed=seed)
    w = rnd(*((Cout, 3, Cin) if mode == L.CONV_T3 else (Cout, 3, 3, Cin)), seed=seed + 1, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=seed + 2, dtype=F32)
    temb = rnd(B, Cout, seed=seed + 3, dtype=F32)
    Ho, Wo = ops.conv_out_hw(H, W, mode)
    res = rnd(B, Ho, Wo, Cout, seed=seed + 4)

    def run(m):
        y = m.out((B, Ho, Wo, Cout), BF, dense=True, name="Y")
        cs = m.out((B * Ho * Wo // 32, 2, Cout), F32, dense=True, name="col_stats_out") if colstats else None
        # NaN directly in front of and behind X: the padding taps must come from the bounds check, not from neighbouring memory
        d = ops.make_conv_desc(m.inp(x, dense=True, name="X"), m.inp(w, dense=True, name="W"), y, m.inp(bias), m.inp(temb, dense=True), m.inp(res, dense=True),
                               mode, cfg, col_stats_out=cs)
        runs = _launch_conv(d)
        return (y, cs, runs) if colstats else (y, runs)
    r = pair(run)
    ref = _conv_ref(x, w, bias, mode)
    tb = temb[:, None, None, :]
    close(r[0], ref + tb + res.float(), **(dict(rtol=2 ** -6, atol_frac=4e-3) if mode == L.CONV_T3 else {}))
    return r


def _colstats_close(cs, out):
    y = out.reshape(-1, out.shape[-1]).double()
    blk = y.reshape(y.shape[0] // 32, 32, y.shape[1])
    ref = torch.stack([blk.sum(1), (blk * blk).sum(1)], 1)
    err = (cs.double() - ref).abs()
    assert cs.shape == ref.shape and (err <= 1e-5 * ref.abs() + 1e-5 * ref[:, 1:].sqrt().max() + 1e-6).all(), err.max().item()


CONV_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 20]


@pytest.mark.parametrize("cfg", CONV_IDS)
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_conv3x3_modes(ops, mode, cfg):
    """S1, S2, UP2, T3 and S2A at (1, 10, 6, 128, 68): 60 / 15 / 240 output pixels and 68 channels, ragged for every tile"""
    _conv_case(ops, mode, 1, 10, 6, 128, 68, cfg)


@pytest.mark.parametrize("shortcut", [False, True])
def test_conv3x3_halo(ops, shortcut):
    """the halo-patch tile 26 at its smallest geometry (one 4 x 32 pixel tile, 160 channels), plain with column statistics and with shortcut taps (S1 / S2)"""
    from tweediemix_amd import lib as L
    B, H, W, Cin, Cout = 1, 4, 32, 64, 160
    if not shortcut:
        y, cs, runs = _conv_case(ops, L.CONV_S1, B, H, W, Cin, Cout, L.TILE_CONV_HALO, seed=500, colstats=True)
        assert runs == L.TILE_CONV_HALO
        _colstats_close(cs, y)
        return
    h = rnd(B, H, W, Cin, seed=520)
    w = rnd(Cout, 3, 3, Cin, seed=521, scale=(9 * Cin) ** -0.5)
    x1, x2 = rnd(B, H, W, 64, seed=522), rnd(B, H, W, 64, seed=523)
    wsc = rnd(Cout, 128, seed=524, scale=128 ** -0.5)
    bias, temb = rnd(Cout, seed=525, dtype=F32), rnd(B, Cout, seed=526, dtype=F32)
    wall = ops.shortcut_weight(w, wsc)

    def run(m):
        y = m.out((B, H, W, Cout), BF, dense=True, name="Y")
        d = ops.make_conv_desc(m.inp(h, dense=True, name="X"), m.inp(wall, dense=True), y, m.inp(bias), m.inp(temb, dense=True), None, L.CONV_S1, L.TILE_CONV_HALO,
                               shortcut=(m.inp(x1, dense=True, name="S1"), m.inp(x2, dense=True, name="S2")))
        return y, _launch_conv(d)
    y, runs = pair(run)
    assert runs == L.TILE_CONV_HALO
    close(y, _conv_ref(h, w, bias, L.CONV_S1) + torch.cat([x1.float(), x2.float()], -1) @ wsc.float().T + temb[:, None, None, :])


@pytest.mark.parametrize("cfg", [12, 20])
def test_conv3x3_fp8(ops, cfg):
    """e4m3 operands at (2, 16, 16, 128, 160): X, W, both scale arrays, Y, the residual and col_stats_out framed"""
    B, H, W, Cin, Cout = 2, 16, 16, 128, 160
    x = rnd(B, H, W, Cin, seed=300, dtype=F32)
    x[..., 40:72] *= 23.0
    w = rnd(Cout, 3, 3, Cin, seed=301, scale=(9 * Cin) ** -0.5)
    q, sc, xd = _mx_quantize(x.view(B * H * W, Cin))
    sx = sc.t().contiguous()
    w8, sw = ops.quantize_fp8_rows(w.view(Cout, 9 * Cin))
    wd = ops.dequantize_fp8_rows(w8, sw).view(Cout, 3, 3, Cin)
    bias, temb, res = rnd(Cout, seed=302, dtype=F32), rnd(B, Cout, seed=303, dtype=F32), rnd(B, H, W, Cout, seed=304)

    def run(m):
        y = m.out((B, H, W, Cout), BF, dense=True, name="Y")
        cs = m.out((B * H * W // 32, 2, Cout), F32, dense=True, name="col_stats_out")
        d = ops.make_conv_desc(m.inp(q.view(B, H, W, Cin), dense=True, name="X"), m.inp(w8.view(Cout, 3, 3, Cin), dense=True), y, m.inp(bias), m.inp(temb, dense=True),
                               m.inp(res, dense=True), 0, cfg, col_stats_out=cs, _fp8=True)
        return y, cs, _launch_conv(d, (m.inp(sx, dense=True, name="scale_x"), m.inp(sw, name="scale_w")))
    y, cs, _ = pair(run)
    ref = F.conv2d(xd.view(B, H, W, Cin).permute(0, 3, 1, 2), wd.permute(0, 3, 1, 2), bias, padding=1).permute(0, 2, 3, 1)
    close(y, ref + temb[:, None, None, :] + res.float(), rtol=2 ** -6, atol_frac=4e-3)
    _colstats_close(cs, y)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 20])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 16, 64, 128), (1, 10, 6, 128, 68), (3, 8, 8, 320, 320)])
def test_conv_s2a_against_padded_stride_2_conv(ops, B, H, W, Cin, Cout, cfg):
    """TMIX_CONV_S2A (zero padding on the right / bottom edge only: the VAE encoder's Downsample2D(padding=0)) against F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2),
    on the shapes, ids and tolerance of test_conv3x3 -- the only other test that reaches this mode goes through an oracle that is not pinned"""
    from tweediemix_amd import lib as L
    x = rnd(B, H, W, Cin, seed=20)
    w = rnd(Cout, 3, 3, Cin, seed=21, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=22, dtype=F32)
    temb = rnd(B, Cout, seed=23, dtype=F32)
    res = rnd(B, H // 2, W // 2, Cout, seed=24)
    out = ops.conv3x3(x, w, bias=bias, batch_bias=temb, residual=res, mode=L.CONV_S2A, tile_cfg=cfg)
    ref = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.float().permute(0, 3, 1, 2), bias, stride=2)
    close(out, (ref + temb[:, :, None, None] + res.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1))
    plain = ops.conv3x3(x, w, mode=L.CONV_S2A, tile_cfg=cfg)                   # and without any epilogue term: the issue's reference as it stands
    close(plain, F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.float().permute(0, 3, 1, 2), stride=2).permute(0, 2, 3, 1))


def test_conv_in_out(ops):
    from tweediemix_amd import lib as L
    B, H, W = 2, 12, 20
    x = rnd(B, 4, H, W, seed=30, dtype=F32)
    w = rnd(64, 3, 3, 4, seed=31, scale=1 / 6, dtype=F32)
    b = rnd(64, seed=32, dtype=F32)
    (y,) = pair(lambda m: ops.conv_in(m.inp(x, dense=True), m.inp(w, dense=True), m.inp(b), out=m.out((B, H, W, 64), BF, dense=True)))
    close(y, F.conv2d(x, w.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1))
    pre_w = torch.tensor([[1.1, 0.2, 0.0, -0.3], [0.1, 0.9, 0.2, 0.0], [0.0, -0.2, 1.2, 0.1], [0.3, 0.0, 0.1, 0.8]])
    pre_b = torch.tensor([0.05, -0.1, 0.2, 0.0])
    pw, pb = (C.c_float * 16)(*pre_w.flatten().tolist()), (C.c_float * 4)(*pre_b.tolist())

    def run_pre(m):
        out = m.out((B, H, W, 64), BF, dense=True)
        L.check(L.load().tmix_conv_in_pre(_p(m.inp(x, dense=True)), _p(m.inp(w, dense=True)), _p(m.inp(b)), _p(out), B, 4, H, W, 64,
                                          C.cast(pw, C.c_void_p), C.cast(pb, C.c_void_p), _st()), "tmix_conv_in_pre")
        return out
    (yp,) = pair(run_pre)
    xm = torch.einsum("oc,bchw->bohw", pre_w.cuda(), x) + pre_b.cuda()[None, :, None, None]
    close(yp, F.conv2d(xm, w.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1))
    xi = rnd(B, H, W, 96, seed=33)
    wo = rnd(4, 3, 3, 96, seed=34, scale=(9 * 96) ** -0.5)
    bo = rnd(4, seed=35, dtype=F32)
    (yo,) = pair(lambda m: ops.conv_out(m.inp(xi, dense=True), m.inp(wo, dense=True), m.inp(bo), out=m.out((B, 4, H, W), F32, dense=True)))
    torch.testing.assert_close(yo, F.conv2d(xi.float().permute(0, 3, 1, 2), wo.float().permute(0, 3, 1, 2), bo, padding=1), rtol=1e-4, atol=1e-4)


# --------------------------------------------------------------------------- normalisation / small ops
@pytest.mark.parametrize("B,HW,C1,C2,silu", [(3, 84, 640, 320, True), (2, 64, 640, 320, True), (1, 100, 64, 0, True)])
def test_groupnorm(ops, B, HW, C1, C2, silu):
    """tmix_groupnorm_nhwc (the first shape: the one-launch small-image path) and, where HW is a multiple of 32, _pre / _pre_f8: x1, x2, y, the workspace and the
    two statistics arrays framed"""
    from tweediemix_amd import lib as L
    lib = L.load()
    x1 = rnd(B, HW, C1, seed=54) * 1.5 + 0.5
    x2 = rnd(B, HW, C2, seed=55) * 2 - 0.25 if C2 else None
    Cc = C1 + C2
    g, b = rnd(Cc, seed=56, dtype=F32), rnd(Cc, seed=57, dtype=F32)
    nws = lib.tmix_groupnorm_ws_floats(B, Cc, 32)

    def run(m):
        y = m.out((B, HW, Cc), BF, dense=True, name="Y")
        ops.groupnorm(m.inp(x1, dense=True, name="X1"), m.inp(g), m.inp(b), 32, 1e-5, silu, x2=None if x2 is None else m.inp(x2, dense=True, name="X2"), out=y,
                      ws=m.scratch(nws, F32))
        return y
    (y,) = pair(run)
    xin = x1.float() if x2 is None else torch.cat([x1.float(), x2.float()], -1)
    ref = F.group_norm(xin.transpose(1, 2), 32, g, b, 1e-5)
    ref = (F.silu(ref) if silu else ref).transpose(1, 2)
    close(y, ref, rtol=2 ** -6, atol_frac=4e-3)
    if HW % 32:
        return

    def colstats(x):
        blk = x.reshape(-1, x.shape[-1]).double().reshape(-1, 32, x.shape[-1])
        return torch.stack([blk.sum(1), (blk * blk).sum(1)], 1).float().contiguous()
    cs1, cs2 = colstats(x1), (colstats(x2) if C2 else None)

    def run_pre(m):
        y = m.out((B, HW, Cc), BF, dense=True, name="Y")
        ops.groupnorm(m.inp(x1, dense=True), m.inp(g), m.inp(b), 32, 1e-5, silu, x2=None if x2 is None else m.inp(x2, dense=True), out=y, ws=m.scratch(nws, F32),
                      colstats=(m.inp(cs1, dense=True, name="cs1"), None if cs2 is None else m.inp(cs2, dense=True, name="cs2")))
        return y
    (yp,) = pair(run_pre)
    close(yp, ref, rtol=2 ** -6, atol_frac=4e-3)

    def run_f8(m):
        y8 = m.out((B, HW, Cc), U8, dense=True, name="Y8")
        s8 = m.out((B * HW, Cc // 32), U8, dense=True, name="scales")
        ops.groupnorm(m.inp(x1, dense=True), m.inp(g), m.inp(b), 32, 1e-5, silu, x2=None if x2 is None else m.inp(x2, dense=True), ws=m.scratch(nws, F32),
                      colstats=(m.inp(cs1, dense=True), None if cs2 is None else m.inp(cs2, dense=True)), f8_out=(y8, s8))
        return y8, s8
    y8, s8 = pair(run_f8)
    q, sc, _deq = _mx_quantize(yp.float().view(B * HW, Cc))
    assert torch.equal(s8, sc.t().contiguous()) and _e4m3_same(y8.view(B * HW, Cc), q)


@pytest.mark.parametrize("rows,Cc", [(5, 64), (3, 2048)])
def test_layernorm(ops, rows, Cc):
    x = rnd(rows, Cc, seed=54) * 3 + 1
    g, b = rnd(Cc, seed=55, dtype=F32), rnd(Cc, seed=56, dtype=F32)
    (y,) = pair(lambda m: ops.layernorm(m.inp(x, dense=True), m.inp(g), m.inp(b), 1e-5, out=m.out((rows, Cc), BF, dense=True)))
    close(y, F.layer_norm(x.float(), (Cc,), g, b, 1e-5))


def test_small_dense_entries(ops):
    """tmix_concat_channels, tmix_timestep_embedding, tmix_affine_clamp, tmix_zero: dense by contract, guards in front and behind"""
    from tweediemix_amd import lib as L
    lib = L.load()
    a, b = rnd(3, 50, 64, seed=57), rnd(3, 50, 128, seed=58)
    (y,) = pair(lambda m: ops.concat_channels(m.inp(a, dense=True), m.inp(b, dense=True), out=m.out((3, 50, 192), BF, dense=True)))
    assert torch.equal(y, torch.cat([a, b], -1))
    vals = torch.tensor([981.0, 1.0, 1024.0, 0.0, 500.0], device="cuda")
    for dim in (320, 256):
        (e,) = pair(lambda m: ops.timestep_embedding(m.inp(vals), dim, out=m.out((5, dim), F32, dense=True)))
        half = dim // 2
        arg = vals[:, None] * torch.exp(-np.log(10000.0) * torch.arange(half, device="cuda", dtype=F32) / half)[None]
        torch.testing.assert_close(e, torch.cat([torch.cos(arg), torch.sin(arg)], -1), rtol=0, atol=2e-4)
    x = rnd(1003, seed=59, dtype=F32)

    def clamp(m):
        out = m.out((1003,), F32)
        L.check(lib.tmix_affine_clamp(_p(m.inp(x)), _p(out), 1003, 0.5, 0.5, 0.0, 1.0, _st()), "tmix_affine_clamp")
        return out
    (yc,) = pair(clamp)
    assert torch.equal(yc, (x * 0.5 + 0.5).clamp(0, 1))

    def zero(m):
        out = m.out((1000,), U8)
        L.check(lib.tmix_zero(_p(out), 1000, _st()), "tmix_zero")
        return out
    (z,) = pair(zero)
    assert int(z.sum()) == 0


def test_softmax_rows(ops):
    """tmix_softmax_rows / _causal / _masked with ld_s, ld_p > cols"""
    from tweediemix_amd import lib as L
    lib = L.load()
    rows, cols = 37, 320
    s = rnd(rows, cols, seed=700, dtype=F32) * 3

    def plain(m):
        sv, p = m.inp(s), m.out((rows, cols), BF, tile=(8, 0))
        L.check(lib.tmix_softmax_rows(_p(sv), sv.stride(0), _p(p), p.stride(0), rows, cols, 0.5, _st()), "tmix_softmax_rows")
        return p
    (p,) = pair(plain)
    close(p, torch.softmax(s * 0.5, -1))
    (pm,) = pair(lambda m: ops.softmax_rows_masked(m.inp(s), m.out((rows, cols), BF, tile=(8, 0)), 257, 0.5))
    close(pm[:, :257], torch.softmax(s[:, :257] * 0.5, -1))
    assert (pm[:, 257:] == 0).all()
    sc = rnd(3 * 77, 128, seed=701, dtype=F32) * 3
    (pc,) = pair(lambda m: ops.softmax_rows_causal(m.inp(sc), m.out((3 * 77, 128), BF, tile=(8, 0)), 77, 0.5))
    close(pc, _causal_ref(sc, 77, 0.5))


def _causal_ref(scores, seq, scale):
    rows, cols = scores.shape
    r = torch.arange(rows, device=scores.device)[:, None] % seq
    c = torch.arange(cols, device=scores.device)[None]
    return torch.softmax((scores * scale).masked_fill(c > r, float("-inf")), -1)


def test_softmax_rows_causal_and_masked_against_torch(ops):
    """the CLIP text towers' causal softmax and the vision tower's padded one against fp32 torch.softmax of the same scores (they are reached otherwise only through
    the towers): the output is one bf16 rounding of a value in [0, 1]; every masked or padding column is exactly 0.0"""
    rows, seq, cols = 3 * 77, 77, 128
    s = rnd(rows, cols, seed=710, dtype=F32) * 4
    p = ops.softmax_rows_causal(s, torch.full((rows, cols), float("nan"), device="cuda", dtype=BF), seq, 0.125)
    close(p, _causal_ref(s, seq, 0.125))
    masked = torch.arange(cols, device="cuda")[None] > (torch.arange(rows, device="cuda")[:, None] % seq)
    assert bool((p[masked] == 0).all()) and bool((p.view(torch.int16)[masked] == 0).all())          # +0.0, bit for bit
    torch.testing.assert_close(p.float().sum(-1), torch.ones(rows, device="cuda"), rtol=0, atol=2 ** -8)       # each term one bf16 rounding (2^-9 relative) of probabilities that sum to 1
    rows, cols, valid = 37, 320, 257
    s = rnd(rows, cols, seed=711, dtype=F32) * 4
    s[:, valid:] = 1e4                                            # padding scores that would dominate if they were read
    p = ops.softmax_rows_masked(s, torch.full((rows, cols), float("nan"), device="cuda", dtype=BF), valid, 0.125)
    ref = torch.zeros(rows, cols, device="cuda")
    ref[:, :valid] = torch.softmax(s[:, :valid] * 0.125, -1)
    close(p, ref)
    assert bool((p.view(torch.int16)[:, valid:] == 0).all())


@pytest.mark.parametrize("frames", [9, 16])
def test_temporal_attn(ops, frames):
    """ld > 3 C, ldo > C, hw = 37"""
    clips, hw, heads = 2, 37, 5
    Cc = heads * 64
    qkv = rnd(clips * frames, hw, 3 * Cc, seed=95)
    (out,) = pair(lambda m: ops.temporal_attention(m.inp(qkv, gap_rows=0), clips, frames, heads, out=m.out((clips * frames, hw, Cc), BF, gap_rows=0)))
    x = qkv.float().view(clips, frames, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)
    ref = F.scaled_dot_product_attention(x[0], x[1], x[2]).permute(0, 3, 1, 2, 4).reshape(clips * frames, hw, Cc)
    close(out, ref, rtol=2 ** -6, atol_frac=4e-3)


@pytest.mark.parametrize("P,ln", [(4, False), (12, True)])
def test_lora_down(ops, P, ln):
    """lda > K + 64: the columns behind the pad stay untouched, the K data columns unchanged, every pad column written (its set's projections, 0 elsewhere)"""
    K, nsets, S, B = 320, 4, 72, 5
    sets = torch.tensor([0, 3, 1, 2, 1], dtype=torch.int32).cuda()
    x = rnd(B * S, K, seed=60) * 1.5 + 0.25
    D = rnd(nsets * P, K, seed=61, scale=0.05)
    gamma, beta = rnd(K, seed=62, dtype=F32) * 0.2 + 1.0, rnd(K, seed=63, dtype=F32) * 0.1
    Dp = (D.float() * gamma).to(BF) if ln else D
    dcs, dbs = (Dp.float().sum(1).contiguous(), (D.float() @ beta).contiguous()) if ln else (None, None)
    a0 = torch.full((B * S, K + 64), 7.0, dtype=BF).cuda()         # stale pad contents must be overwritten
    a0[:, :K] = x

    def run(m):
        a = m.inout(a0, tile=(8, 0), name="A")
        ops.lora_down(a, K, m.inp(Dp, dense=True), P, nsets, m.inp(sets), S, dcolsum=None if dcs is None else m.inp(dcs), dbias=None if dbs is None else m.inp(dbs))
        return a
    (a,) = pair(run)
    assert torch.equal(a[:, :K], x)
    xf = x.float()
    ref = torch.zeros(B * S, 64, device="cuda")
    for bb in range(B):
        s_, rows = int(sets[bb]), slice(bb * S, (bb + 1) * S)
        if ln:
            mean = xf[rows].mean(1, keepdim=True)
            sd = (xf[rows].var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
            ref[rows, s_ * P:(s_ + 1) * P] = (xf[rows] - mean) @ Dp.float()[s_ * P:(s_ + 1) * P].T + (D.float()[s_ * P:(s_ + 1) * P] @ beta) * sd
        else:
            ref[rows, s_ * P:(s_ + 1) * P] = xf[rows] @ D.float()[s_ * P:(s_ + 1) * P].T
    close(a[:, K:], ref)
    assert (a[:, K:].float()[ref == 0] == 0).all()


def test_linear_small(ops):
    """tmix_linear_small / _sections at M = 37 (rows leave 16 per launch: the last launch is ragged)"""
    M, K = 37, 320
    widths = [320, 640, 64]
    x = rnd(M, K, seed=59, dtype=F32)
    ws = [rnd(n, K, seed=70 + i, scale=K ** -0.5) for i, n in enumerate(widths)]
    bs = [rnd(n, seed=80 + i, dtype=F32) for i, n in enumerate(widths)]
    add = rnd(M, widths[0], seed=62, dtype=F32)
    (y,) = pair(lambda m: ops.linear_small(m.inp(x, dense=True), m.inp(ws[0], dense=True), m.inp(bs[0]), m.inp(add, dense=True), act_in=True, act_out=True,
                                           out=m.out((M, widths[0]), F32, dense=True)))
    torch.testing.assert_close(y, F.silu(F.silu(x) @ ws[0].float().T + bs[0] + add), rtol=1e-4, atol=1e-4)
    st = torch.tensor([0] + list(torch.tensor(widths).cumsum(0)), device="cuda", dtype=torch.int32)
    wall, ball, N = torch.cat(ws, 0).contiguous(), torch.cat(bs, 0).contiguous(), sum(widths)
    (flat,) = pair(lambda m: ops.linear_small_sections(m.inp(x, dense=True), m.inp(wall, dense=True), m.inp(ball), m.inp(st), act_in=True, out=m.out((M * N,), F32)))
    off = 0
    for w_, b_ in zip(ws, bs):
        n = w_.shape[0]
        close(flat[off * M:(off + n) * M].view(M, n), F.silu(x) @ w_.float().t() + b_)
        off += n


# --------------------------------------------------------------------------- sampler steps
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("mode", ["fusion", "plain", "resample"])
def test_tweedie_step(ops, dt, mode):
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import lib as L
    K, h, w = 5, 5, 7
    rng = np.random.RandomState(K * 100 + h)
    x = rng.randn(1, 4, h, w).astype(np.float32)
    eps = rng.randn(K + 1, 4, h, w).astype(np.float32)
    masks = (rng.rand(K, 1, h, w) > 0.6).astype(np.float32)
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    eps_t = torch.from_numpy(eps).to(tdt).cuda()
    eps_r = eps_t.float().cpu().numpy()
    at, an, g = np.float32(0.2345), np.float32(0.3456), 0.8
    lowp = np.float16 if dt == "f16" else None
    md = {"fusion": L.STEP_FUSION, "plain": L.STEP_PLAIN, "resample": L.STEP_RESAMPLE}[mode]
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(masks).cuda()

    def run(m):
        ox, o0 = m.out(xt.shape, F32, dense=True, name="out_x"), m.out(xt.shape, F32, dense=True, name="out_x0", written=mode != "resample")
        ops.fused_tweedie_step(m.inp(xt, dense=True), m.inp(eps_t, dense=True), m.inp(mt, dense=True), md, K, g, at, an, False, out_x=ox, out_x0=o0)
        return (ox, o0) if mode != "resample" else (ox,)
    r = pair(run)
    if mode == "fusion":
        ref, ref0 = TO.fused_fusion_step(x, eps_r, masks, g, at, an, False, lowp)
    elif mode == "plain":
        ref, ref0 = TO.fused_plain_step(x, eps_r[:2], g, at, an, False, lowp)
    else:
        ref, ref0 = TO.fused_resample_down(x, eps_r, K, g, at, an, lowp), None
    assert np.array_equal(r[0].cpu().numpy(), ref)
    if ref0 is not None:
        assert np.array_equal(r[1].cpu().numpy(), ref0)


def test_tweedie_step_dev_and_prologue(ops):
    """tmix_fused_tweedie_step_dev (three seeds, per-seed masks, latent updated in place) and tmix_step_prologue"""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import lib as L
    lib = L.load()
    K, h, w, seeds = 5, 5, 7, 3
    rows = K + 1
    rng = np.random.RandomState(11)
    x = rng.randn(seeds, 4, h, w).astype(np.float32)
    eps = rng.randn(seeds * rows, 4, h, w).astype(np.float32)
    masks = (rng.rand(seeds, K, 1, h, w) > 0.5).astype(np.float32)
    at, an, g = np.float32(0.4111), np.float32(0.5222), 0.8
    sa, s1, san, s1n = ops.step_coeffs(at, an)
    prm = torch.tensor([781.0, sa, s1, san, s1n, 0.0, g, 0.0], dtype=F32).cuda()
    xt, et, mt = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda(), torch.from_numpy(masks).cuda()

    def run(m):
        xv = m.inout(xt, dense=True, name="x (in place)")
        o0 = m.out(xt.shape, F32, dense=True, name="out_x0")
        L.check(lib.tmix_fused_tweedie_step_dev(_p(xv), _p(m.inp(et, dense=True)), L.F32, _p(m.inp(mt.view(seeds * K, h * w), dense=True)), K * h * w, _p(xv), _p(o0),
                                                K, 4, h * w, L.STEP_FUSION, rows, seeds, _p(m.inp(prm)), _st()), "tmix_fused_tweedie_step_dev")
        return xv, o0
    xo, x0 = pair(run)
    for sd in range(seeds):
        ref, ref0 = TO.fused_fusion_step(x[sd:sd + 1], eps[sd * rows:(sd + 1) * rows], masks[sd], g, at, an, False, None)
        assert np.array_equal(xo[sd:sd + 1].cpu().numpy(), ref) and np.array_equal(x0[sd:sd + 1].cpu().numpy(), ref0)
    n = 4 * h * w

    def prologue(m):
        lat, td = m.out((seeds * rows, n), F32, dense=True, name="latent"), m.out((seeds * rows,), F32, name="t_dev")
        L.check(lib.tmix_step_prologue(_p(m.inp(xt, dense=True)), _p(lat), _p(td), _p(m.inp(prm)), seeds, rows, n, _st()), "tmix_step_prologue")
        return lat, td
    lat, td = pair(prologue)
    assert torch.equal(lat.view(seeds, rows, n), xt.view(seeds, 1, n).expand(-1, rows, -1)) and torch.equal(td, torch.full_like(td, 781.0))


def test_video_step_entries(ops):
    """tmix_video_step_prologue with clip strides larger than a clip and R > C (channels [C, R) and the gap between clips keep the sentinel), tmix_vpred_step_dev reading
    such plans, tmix_vpred_step and tmix_frame_inject"""
    from tweediemix_amd import lib as L
    lib = L.load()
    S, Cc, Fr, h, w, R = 2, 4, 3, 5, 7, 8
    hw = h * w
    x = rnd(S, Cc, Fr, h, w, seed=800, dtype=F32)
    prm = ops.video_step_params(421.0, 9.0, 0.31, 0.36).cuda()

    def prologue(m):
        xs = []
        for name in ("x_u", "x_c"):          # [clips][frames][C * hw of a row of R * hw]: clip stride = one frame row more than a clip
            xs.append(m.out((S, Fr, Cc * hw), F32, ld=R * hw, batch_stride=(Fr + 1) * R * hw, dense_ld=R * hw, tile=(8, 0), name=name))
        tu, tc = m.out((S,), F32, name="t_u"), m.out((S,), F32, name="t_c")
        L.check(lib.tmix_video_step_prologue(_p(m.inp(x, dense=True)), _p(xs[0]), xs[0].stride(0), _p(tu), _p(xs[1]), xs[1].stride(0), _p(tc), _p(m.inp(prm)),
                                             S, Cc, Fr, hw, R, _st()), "tmix_video_step_prologue")
        return xs[0], xs[1], tu, tc
    xu, xc, tu, tc = pair(prologue)
    want = x.permute(0, 2, 1, 3, 4).reshape(S, Fr, Cc * hw)
    assert torch.equal(xu, want) and torch.equal(xc, want) and torch.equal(tu, torch.full_like(tu, 421.0)) and torch.equal(tc, tu)

    vu, vc = rnd(S, Fr, Cc * hw, seed=801, dtype=F32), rnd(S, Fr, Cc * hw, seed=802, dtype=F32)

    def step_dev(m):
        xv = m.inout(x, dense=True, name="x (in place)")
        a, b = m.inp(vu, ld=Cc * hw, batch_stride=(Fr + 1) * Cc * hw, name="v_u"), m.inp(vc, ld=Cc * hw, batch_stride=(Fr + 2) * Cc * hw, name="v_c")
        L.check(lib.tmix_vpred_step_dev(_p(xv), _p(a), a.stride(0), _p(b), b.stride(0), _p(m.inp(prm)), S, Cc, Fr, hw, _st()), "tmix_vpred_step_dev")
        return xv
    (xn,) = pair(step_dev)
    # the scalar kernel on the same video, element for element (the header's contract), itself framed
    v = torch.cat([vu.view(S, Fr, Cc, hw).permute(0, 2, 1, 3), vc.view(S, Fr, Cc, hw).permute(0, 2, 1, 3)]).contiguous()
    (xs,) = pair(lambda m: ops.vpred_step(m.inp(x.view(S, Cc, Fr, hw), dense=True), m.inp(v, dense=True), 9.0, 0.31, 0.36, out=m.out((S, Cc, Fr, hw), F32, dense=True)))
    assert torch.equal(xn.view(S, Cc, Fr, hw), xs)
    f = np.float32
    sa, s1, san, s1n = [float(t) for t in (np.sqrt(f(0.31)), np.sqrt(f(1) - f(0.31)), np.sqrt(f(0.36)), np.sqrt(f(1) - f(0.36)))]
    vv = v[:S].double() + 9.0 * (v[S:].double() - v[:S].double())
    xd = x.view(S, Cc, Fr, hw).double()
    ref = san * (sa * xd - s1 * vv) + s1n * (sa * vv + s1 * xd)
    torch.testing.assert_close(xs.double(), ref, rtol=1e-5, atol=1e-4)       # fp32 evaluation of |values| up to ~50 (g = 9)

    y = rnd(2 * 4, 6, 40, seed=803)
    for interp in (None, 0.3):
        (yi,) = pair(lambda m: ops.frame_inject(m.inout(y, dense=True), 2, 4, interp))
        yr = y.float().view(2, 4, -1).clone()
        first = yr[:, :1].clone()
        if interp is None:
            yr[:, 1:] = first
        else:
            yr[:, 1:] = float(np.float32(interp)) * first + float(np.float32(1.0 - interp)) * yr[:, 1:]
        close(yi.view(2, 4, -1), yr)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_conditioning_entries(ops):
    """the once-per-video fp32 kernels (csrc/conditioning.hip): dense by contract, every pointer framed"""
    from tweediemix_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    B, Ci, H, W, Co = 1, 5, 7, 11, 3
    x, w, b = torch.randn(B, Ci, H, W, generator=g).cuda(), (torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).cuda(), torch.randn(Co, generator=g).cuda()

    def conv(m):
        y = m.out((B, Co, (H - 1) // 2 + 1, (W - 1) // 2 + 1), F32, dense=True)
        L.check(lib.tmix_conv3x3_f32(_p(m.inp(x, dense=True)), _p(m.inp(w, dense=True)), _p(m.inp(b)), _p(y), B, Ci, H, W, Co, 2, 1, _st()), "tmix_conv3x3_f32")
        return y
    (y,) = pair(conv)
    assert _rel(y, F.silu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))) < 2e-6
    xp = torch.randn(2, 6, 7, 5, generator=g).cuda()

    def pool(m):
        y = m.out((2, 6, 3, 4), F32, dense=True)
        L.check(lib.tmix_adaptive_avgpool_f32(_p(m.inp(xp, dense=True)), _p(y), 12, 7, 5, 3, 4, _st()), "tmix_adaptive_avgpool_f32")
        return y
    (yp,) = pair(pool)
    assert (yp - F.adaptive_avg_pool2d(xp, (3, 4))).abs().max().item() < 1e-6
    M, N, K = 20, 37, 19
    xl, wl, bl = torch.randn(M, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / K ** 0.5).cuda(), torch.randn(N, generator=g).cuda()

    def lin(m):
        y = m.out((M, N), F32, dense=True)
        L.check(lib.tmix_linear_f32(_p(m.inp(xl, dense=True)), _p(m.inp(wl, dense=True)), _p(m.inp(bl)), _p(y), M, N, K, 1, 1, _st()), "tmix_linear_f32")
        return y
    (yl,) = pair(lin)
    assert _rel(yl, F.silu(F.linear(F.silu(xl.double()), wl.double(), bl.double()))) < 2e-6
    clips, frames, Hh, Ww, C_ = 1, 9, 5, 7, 4
    shapes = [(C_,), (C_,), (2 * C_, C_), (2 * C_, C_), (2 * C_, C_), (C_, 2 * C_), (C_,), (4 * C_, C_), (4 * C_,), (C_, 4 * C_), (C_,)]
    ps = [(torch.randn(*s_, generator=g) * (1.0 if len(s_) == 1 else 0.7)).cuda() for s_ in shapes]
    xe = (torch.randn(clips * frames, C_, Hh, Ww, generator=g) * 2 + 0.5).cuda()

    def enc(m):
        y = m.out((clips, C_, frames, Hh, Ww), F32, dense=True)
        L.check(lib.tmix_i2v_temporal_encoder(_p(m.inp(xe, dense=True)), _p(y), clips, frames, C_, Hh * Ww, *[_p(m.inp(t, dense=True)) for t in ps], _st()),
                "tmix_i2v_temporal_encoder")
        return y
    (ye,) = pair(enc)
    d = [t.double() for t in ps]
    t = xe.double().view(clips, frames, C_, Hh, Ww).permute(0, 3, 4, 1, 2).reshape(clips * Hh * Ww, frames, C_)
    h = F.layer_norm(t, (C_,), d[0], d[1], 1e-5)
    q, k, v = [F.linear(h, d[i]).view(-1, frames, 2, C_).transpose(1, 2) for i in (2, 3, 4)]
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(-1, frames, 2 * C_)
    t = t + F.linear(o, d[5], d[6])
    t = t + F.linear(F.gelu(F.linear(t, d[7], d[8])), d[9], d[10])
    assert _rel(ye, t.view(clips, Hh, Ww, frames, C_).permute(0, 4, 3, 1, 2)) < 1e-5


# --------------------------------------------------------------------------- the detector sees what a missing mask would do (no faulty kernel needed)
# Each launch below is a CORRECT one over a slightly larger problem (the bigger operands exist, every write lies inside the allocation); the frame declares the
# smaller extent, so the extra row / query / channels are exactly what an unmasked edge would have stored.
def test_sensitivity_gemm_extra_row(ops):
    M, N, K = 77, 200, 128
    a, w = rnd(M + 1, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    f = Frame((M, N), BF, ld=328, front=64, tail_rows=TILE_ROWS, device="cuda", name="C declared with M rows")
    d = ops.make_gemm_desc(a, w, f.view, tile_cfg=12)
    assert d.M == M + 1 and d.ldc == 328
    _launch_gemm(d)
    torch.cuda.synchronize()
    f.assert_all_written()
    with pytest.raises(AssertionError) as e:
        f.assert_untouched()
    assert e.value.count == N and e.value.positions == [(0, M, c) for c in range(8)]
    assert f.touched_positions() == [(0, M, c) for c in range(N)]
    close(f.padded[0, :, :N], (a.float() @ w.float().T)[:M])


def test_sensitivity_attention_extra_query(ops):
    B, H, Sq, Skv = 1, 2, 70, 96
    Cc = H * 64
    q, k, v = rnd(B, Sq + 1, Cc, seed=40), rnd(B, Skv, Cc, seed=41), rnd(B, Skv, Cc, seed=42)
    f = Frame((B, Sq, Cc), BF, ld=Cc + 8, front=64, tail_rows=TILE_ROWS, device="cuda", name="O declared with Sq queries")
    out = f.buf.as_strided((B, Sq + 1, Cc), (f.batch_stride, f.ld, 1), f.origin)
    ops.attention(q, k, v.transpose(1, 2).contiguous(), H, Skv, 0.125, out=out)
    torch.cuda.synchronize()
    f.assert_all_written()
    with pytest.raises(AssertionError) as e:
        f.assert_untouched()
    assert e.value.count == Cc and f.touched_positions() == [(0, Sq, c) for c in range(Cc)]


def test_sensitivity_conv_extra_channels(ops):
    B, H, W, Cin, Cout = 1, 10, 6, 128, 68
    x, w = rnd(B, H, W, Cin, seed=20), rnd(Cout + 8, 3, 3, Cin, seed=21, scale=(9 * Cin) ** -0.5)
    f = Frame((B * H * W, Cout), BF, ld=Cout + 8, front=64, tail_rows=TILE_ROWS, device="cuda", name="Y declared with Cout channels")
    y = f.buf.as_strided((B, H, W, Cout + 8), (H * W * (Cout + 8), W * (Cout + 8), Cout + 8, 1), f.origin)
    assert y.is_contiguous()
    ops.conv3x3(x, w, out=y, tile_cfg=12)
    torch.cuda.synchronize()
    f.assert_all_written()
    with pytest.raises(AssertionError) as e:
        f.assert_untouched()
    assert e.value.count == 8 * B * H * W
    assert f.touched_positions() == [(0, r, c) for r in range(B * H * W) for c in range(Cout, Cout + 8)]
