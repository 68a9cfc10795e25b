"""CPU: which kernel a GEMM / convolution launch runs for every requested tile_cfg -- tmix_gemm_resolve_tile / tmix_conv_resolve_tile (the resolver
of csrc/gemm_conv.hip over the table in csrc/gemm_tilings.h) against tests/golden/tile_resolution.json.

The fixture was RECORDED from the commit before the table existed: its launch() was patched to return (tiling, fp8 mode) at the three points where
it hands over to a kernel, and tmix_gemm_bf16 / tmix_gemm_fp8 / tmix_conv3x3_nhwc[_fp8] were called with the descriptors of cases() below
(pointers are never dereferenced before the launch).  One array per case over the requested ids 0..28: the tiling that runs, or the negative
TMIX_E* code of a refusal."""
import ctypes as C
import json
import os

import pytest

from tweediemix_amd import lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_resolution.json")
IDS = list(range(29))                      # AUTO, 1..26 (retired and reserved ids included), two ids out of range
RETIRED = (6, 8, 9, 10, 11)

# (M, N, K, batch): tile counts on both sides of AUTO's 192 and the fp8 choice's 160; K % 128 == 0 and != 0; K / 32 on both sides of both f8_block_cap values
GEMM_SHAPES = [(4096, 1280, 1280, 1), (4096, 1280, 1280, 8), (256, 640, 1280, 1), (4096, 1280, 320, 1), (256, 640, 320, 1), (4096, 1280, 5120, 1), (4096, 1280, 2560, 1)]
GEMM_OPERANDS = ("bf16", "f8row", "f8blk")
GEMM_VARIANTS = ("plain", "plain_narrow", "geglu", "geglu_narrow", "geglu_f8out", "trans", "trans_narrow", "f8copy", "f8copy_stats", "f8copy_rgb",
                 "stats", "colstats", "residual", "residual_narrow")


def gemm_desc(operands, M, N, K, batch, variant, n_trans_begin=None):
    d = L.GemmDesc()
    d.A, d.W, d.C = 0x10000, 0x20000, 0x30000
    d.M, d.N, d.K, d.batch, d.lda, d.ldw, d.ldc, d.n_trans_begin = M, N, K, batch, K, K, N, -1
    if variant.startswith("geglu"):
        d.epilogue, d.ldc = L.EPI_GEGLU, N // 2
    if variant.endswith("narrow") and not variant.startswith("trans"):
        d.ldc += 4                                                     # ldc % 8 != 0: the unstaged stores
    if batch > 1:
        d.strideA, d.strideC = M * K, M * d.ldc
    if operands == "f8blk":
        d.reserved0 |= L.F8_A_BLOCK_SCALES
    if variant == "geglu_f8out":
        d.reserved0 |= L.F8_GEGLU_OUT
        d.Ct, d.ldct = 0x40000, batch * M
    if variant.startswith("trans"):
        d.n_trans_begin = n_trans_begin if n_trans_begin is not None else N // 256 * 128     # 1280 -> 640 (off the edge of 256-wide tiles), 640 -> 256 (of 160-wide ones)
        d.Ct, d.ldct = 0x40000, M + (4 if variant == "trans_narrow" else 0)
        d.strideCt = (N - d.n_trans_begin) * d.ldct if batch > 1 else 0
    if variant.startswith("f8copy"):
        d.reserved0 |= L.F8_COPY_OUT
        d.Ct, d.ldct, d.strideCt = 0x40000, N, batch * M * N
    if variant in ("f8copy_stats", "stats"):
        d.row_stats_out, d.ldStatsOut, d.strideStatsOut = 0x50000, batch * M, 2 * M
    if variant == "f8copy_rgb":
        d.rowgroup_bias, d.rows_per_group = 0x60000, 64
    if variant == "colstats":
        d.col_stats_out = 0x70000
    if variant.startswith("residual"):
        d.residual, d.ldr = 0x80000, N + (4 if variant == "residual_narrow" else 0)
        d.strideR = M * d.ldr if batch > 1 else 0
    return d


# (B, H, W, Cin, Cout): a full tile of the halo-patch kernel, a width it cannot run, Cin % 128 != 0, narrow stores (Cout % 8 != 0), enough tiles for AUTO's 256x128
CONV_SHAPES = [(1, 4, 32, 128, 160), (1, 4, 24, 128, 160), (1, 8, 32, 64, 160), (1, 4, 32, 128, 164), (4, 64, 64, 128, 640)]
CONV_VARIANTS = ("plain", "residual", "colstats", "batch_bias", "shortcut1", "shortcut2")


def conv_desc(B, H, W, Cin, Cout, mode, variant):
    d = L.ConvDesc()
    d.X, d.Wt, d.Y, d.bias = 0x10000, 0x20000, 0x30000, 0x40000
    d.B, d.H, d.W, d.Cin, d.Cout, d.mode = B, H, W, Cin, Cout, mode
    if variant == "residual":
        d.residual = 0x50000
    if variant == "colstats":
        d.col_stats_out = 0x60000
    if variant == "batch_bias":
        d.batch_bias, d.batch_bias_images = 0x70000, 1
    if variant.startswith("shortcut"):
        d.S1, d.S1_channels = 0x80000, 64
        if variant == "shortcut2":
            d.S2, d.S2_channels = 0x90000, 128
    return d


def error_cases():
    """launches the validation refuses whatever the tiling: the query must return the same code"""
    out = {}
    d = gemm_desc("bf16", 256, 640, 320, 1, "plain"); d.A = 0
    out["err/gemm/null_A"] = ("gemm", d, 0)
    out["err/gemm/K_100"] = ("gemm", gemm_desc("bf16", 256, 640, 100, 1, "plain"), 0)
    out["err/gemm/N_642"] = ("gemm", gemm_desc("bf16", 256, 642, 320, 1, "plain"), 0)
    d = gemm_desc("bf16", 256, 640, 320, 1, "plain"); d.epilogue = 7
    out["err/gemm/epilogue_7"] = ("gemm", d, 0)
    d = gemm_desc("bf16", 256, 640, 320, 1, "geglu"); d.residual, d.ldr = 0x80000, 640
    out["err/gemm/geglu_residual"] = ("gemm", d, 0)
    d = gemm_desc("bf16", 256, 640, 320, 1, "plain"); d.reserved0 = L.F8_A_BLOCK_SCALES
    out["err/gemm/fp8_flag_on_bf16"] = ("gemm", d, 0)
    out["err/gemm/fp8_block_scales_K_8192"] = ("gemm", gemm_desc("f8blk", 256, 640, 8192, 1, "plain"), 1)
    out["err/gemm/fp8_colstats"] = ("gemm", gemm_desc("f8row", 256, 640, 320, 1, "colstats"), 1)
    out["err/gemm/bf16_geglu_f8out"] = ("gemm", gemm_desc("bf16", 256, 640, 320, 1, "geglu_f8out"), 0)
    out["err/conv/fp8_Cin_64"] = ("conv", conv_desc(1, 8, 32, 64, 160, L.CONV_S1, "plain"), 1)
    out["err/conv/fp8_shortcut"] = ("conv", conv_desc(1, 4, 32, 128, 160, L.CONV_S1, "shortcut1"), 1)
    d = gemm_desc("bf16", 64, 64, 64, 6, "plain"); d.strideW, d.w_period = 64 * 64, 4
    out["err/gemm/w_period"] = ("gemm", d, 0)
    d = conv_desc(1, 4, 32, 128, 160, 9, "plain")
    out["err/conv/mode_9"] = ("conv", d, 0)
    out["err/conv/stride2_odd_H"] = ("conv", conv_desc(1, 5, 32, 128, 160, L.CONV_S2, "plain"), 0)
    out["err/conv/Cin_100"] = ("conv", conv_desc(1, 4, 32, 100, 160, L.CONV_S1, "plain"), 0)
    out["err/conv/shortcut_stride2"] = ("conv", conv_desc(1, 4, 32, 128, 160, L.CONV_S2, "shortcut1"), 0)
    d = conv_desc(1, 4, 32, 128, 160, L.CONV_S1, "plain"); d.Y = 0x30004
    out["err/conv/Y_alignment"] = ("conv", d, 0)
    return out


def cases():
    """name -> (kind, descriptor, fp8_operands): operands x shapes x what the launch asks of its kernel, so that every rule of resolve_tile is reached"""
    out = {}
    for op in GEMM_OPERANDS:
        for n, (M, N, K, b) in enumerate(GEMM_SHAPES):
            # every variant at a large and a small shape (K % 128 == 0 and != 0); the other shapes move tile counts and K only: the variants those rules read
            for v in (GEMM_VARIANTS if n in (0, 4) else ("plain", "f8copy", "stats", "f8copy_stats")):
                if (v == "geglu_f8out") == (op == "bf16") and v in ("geglu_f8out", "colstats"):
                    continue             # (the e4m3 GEGLU output is for e4m3 operands, column statistics for bf16 ones: error_cases records the refusals)
                out[f"gemm/{op}/{M}x{N}x{K}b{b}/{v}"] = ("gemm", gemm_desc(op, M, N, K, b, v), int(op != "bf16"))
        for ntb in (640, 1280):          # a transposed region whose boundary is off an edge of the wider tiles
            for v in ("trans", "trans_narrow"):
                out[f"gemm/{op}/4096x1920x1280b1/{v}@{ntb}"] = ("gemm", gemm_desc(op, 4096, 1920, 1280, 1, v, ntb), int(op != "bf16"))
    for fp8 in (0, 1):
        for shape in CONV_SHAPES:
            for mode, mname in ((L.CONV_S1, "S1"), (L.CONV_S2, "S2"), (L.CONV_UP2, "UP2"), (L.CONV_T3, "T3")):
                for v in (CONV_VARIANTS if mode == L.CONV_S1 else ("plain", "colstats")):      # (shortcut taps: stride 1 only)
                    if fp8 and (shape[3] % 128 or v.startswith("shortcut")):
                        continue         # (refused for e4m3 operands: error_cases)
                    out[f"conv/{'f8' if fp8 else 'bf16'}/{'x'.join(map(str, shape))}/{mname}/{v}"] = ("conv", conv_desc(*shape, mode, v), fp8)
    out.update(error_cases())
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_the_grid(golden):
    assert golden["ids"] == IDS and sorted(golden["cases"]) == sorted(cases())
    seen = {v for row in golden["cases"].values() for v in row}
    # every live tiling runs somewhere, no retired or reserved id ever does, and both kinds of refusal are recorded
    assert {v for v in seen if v > 0} == set(range(1, 27)) - set(RETIRED) - {24, 25}
    assert L.EINVAL in seen and L.ESHAPE in seen and L.EALIGN in seen


def test_queries_resolve_as_the_recorded_launches(golden):
    l = L.load()
    bad = []
    for name, (kind, d, fp8) in cases().items():
        fn = l.tmix_gemm_resolve_tile if kind == "gemm" else l.tmix_conv_resolve_tile
        got = []
        for cfg in IDS:
            d.tile_cfg = cfg
            got.append(fn(C.byref(d), fp8))
        if got != golden["cases"][name]:
            bad.append((name, got, golden["cases"][name]))
    assert not bad, f"{len(bad)} cases differ, first: {bad[0]}"


def test_refusals_keep_their_messages():
    l = L.load()
    d = gemm_desc("bf16", 4096, 1280, 1280, 1, "f8copy_stats")
    d.tile_cfg = 14
    assert l.tmix_gemm_resolve_tile(C.byref(d), 0) == L.EINVAL and b"not compiled into tiling 14" in l.tmix_last_error_string()
    d = gemm_desc("f8blk", 4096, 1280, 5120, 1, "stats")
    d.tile_cfg = 16
    assert l.tmix_gemm_resolve_tile(C.byref(d), 1) == L.EINVAL and b"request tile_cfg 17 explicitly" in l.tmix_last_error_string()
    assert l.tmix_gemm_resolve_tile(None, 0) == L.EINVAL and l.tmix_conv_resolve_tile(None, 0) == L.EINVAL
    assert l.tmix_gemm_f8copy_tile(0) == L.EINVAL and l.tmix_gemm_f8copy_tile(27) == L.EINVAL


def test_python_helpers_reproduce_the_retired_mirrors():
    """the plan builder and the tuners kept copies of two rules; they now ask the library.  For every id that is not retired the answers are the old ones."""
    from tweediemix_amd import ops
    f8copy_tile_alt = {6: 4, 8: 7, 9: 2, 10: 1, 11: 4, 14: 12, 19: 12, 20: 12, 21: 12, 22: 12, 23: 12, 24: 12, 25: 12, 26: 12}      # lib.F8COPY_TILE_ALT
    conv_alias = {16: 4, 17: 2, 18: 12, 19: 12, 21: 12, 22: 14, 23: 12, 24: 14, 25: 12}                                         # UNetPlan.autotune
    conv_skip = (16, 17, 18, 19, 21, 22, 23, 24, 25)                                                                            # refine_group
    halo_ok, halo_no, taps = conv_desc(1, 4, 32, 128, 160, L.CONV_S1, "colstats"), conv_desc(1, 4, 24, 128, 160, L.CONV_S1, "colstats"), conv_desc(1, 4, 32, 128, 160, L.CONV_S1, "shortcut1")
    for cfg in range(1, 27):
        if cfg in RETIRED:
            continue
        assert ops.f8copy_tile(cfg) == f8copy_tile_alt.get(cfg, cfg), cfg
        for d in (halo_ok, halo_no, taps):
            if cfg != L.TILE_CONV_HALO:
                assert ops.conv_runs_as(d, cfg) == conv_alias.get(cfg, cfg), cfg
                assert (ops.conv_runs_as(d, cfg) != cfg) == (cfg in conv_skip), cfg
    # tiling 26: an alias exactly where the old hand copy of its eligibility test said so (W % 32, H % 4, Cout % 160, stride 1)
    assert ops.conv_runs_as(halo_ok, 26) == 26 and ops.conv_runs_as(taps, 26) == 26 and ops.conv_runs_as(halo_no, 26) == 20
    assert ops.conv_runs_as(conv_desc(1, 4, 32, 128, 160, L.CONV_UP2, "plain"), 26) == 20 and ops.conv_runs_as(conv_desc(1, 4, 32, 128, 320 - 8, L.CONV_S1, "plain"), 26) == 20
    assert ops.conv_runs_as(conv_desc(1, 6, 32, 128, 160, L.CONV_S1, "plain"), 26) == 20
    assert halo_ok.tile_cfg == 0                                   # the helper leaves the descriptor as it was
    # the retired ids: the library's answer (8 runs as 19, which the e4m3 copy turns into 12; the old map said 7)
    assert [ops.f8copy_tile(c) for c in RETIRED] == [4, 12, 2, 1, 4]
