// gemm_conv.hip -- host entry points of the bf16 / fp8 MFMA GEMM and the 3x3 NHWC implicit-GEMM convolution: argument
// validation, descriptor -> kernel parameters, the resolver over the tilings of gemm_tilings.h, dispatch.  The kernel lives in gemm_kernel.h and is instantiated per group
// of tilings in gemm_inst_*.hip.
#include "gemm_kernel.h"
#include "gemm_tilings.h"
#include <stdlib.h>

using namespace tmix_gemm;

namespace tmix_gemm {

bool f8_lockstep(int tile_cfg, int K, bool f8out) {
    // rows of 128 K values; not for the e4m3 GEGLU output: its MX blocks of 32 output columns need wave tiles that are multiples of 64 weight rows wide -- the
    // phase-offset tilings' 128 x 64; a 160-wide tile ends in the middle of a block
    return tile_cfg >= 1 && tile_cfg <= NUM_CFG && tile_has(tile_cfg, CAP_F8_LOCKSTEP) && K % 128 == 0 && !f8out;
}

int f8copy_tile(int tile_cfg) {
    if (tile_cfg < 1 || tile_cfg > NUM_CFG) TMIX_FAIL(TMIX_EINVAL, "gemm_f8copy_tile: tile_cfg=%d", tile_cfg);
    // (every substitute keeps the tile width, and with it the number of row-statistics partials, except 256x320 -> 128x160)
    int cfg = TILINGS[tile_cfg].runs_as;
    while (!tile_has(cfg, CAP_F8C)) cfg = TILINGS[cfg].fb;
    return cfg;
}

#define TMIX_REFUSE(code, ...) do { tmix_set_error(__VA_ARGS__); return TileChoice{0, 0, (code)}; } while (0)

// Which kernel runs a launch with traits t that asks for tiling cfg.  The rules run in this order; each sees the id the ones before it left.
TileChoice resolve_tile(const TileTraits& t, int cfg) {
    const bool staged = t.n_trans_begin < 0 && (t.epilogue == TMIX_EPI_GEGLU ? (t.wide & 2) : (t.wide & 1));      // the staged plain / GEGLU epilogue, no transposed region
    if (cfg <= 0 || cfg > NUM_CFG)        // AUTO: 256x128 when it still yields >= 3/4 of a CU wave, else 128x128
        cfg = (int64_t)((t.M + 255) / 256) * ((t.N + 127) / 128) * t.batch >= 192 ? 2 : 1;
    cfg = TILINGS[cfg].runs_as;           // retired and reserved ids
    if (TILINGS[cfg].loop == OWN_KERNEL) {
        if (cfg == 26 ? t.convh_ok : t.w22_ok) return {cfg, 0, TMIX_OK};
        cfg = t.conv ? TILINGS[cfg].fb_conv : TILINGS[cfg].fb;
    }
    if (t.n_trans_begin >= 0) {
        if (t.n_trans_begin % TILINGS[cfg].bn) cfg = 2;                        // the boundary must fall on a tile edge (N = 3 x 320: 640)
        if (!(t.wide & 4) && !tile_has(cfg, CAP_NARROW_T)) cfg = 2;                // narrow (unstaged) transposed stores need square wave tiles
    }
    if (t.f8copy) {
        if (cfg == 14 && t.stats_out) TMIX_REFUSE(TMIX_EINVAL, "gemm: the e4m3 copy is not compiled into tiling 14; with row_stats_out pick another tiling (the partial count depends on it)");
        if (!(t.fp8 && !t.conv && TILINGS[cfg].lw && f8_lockstep(cfg, t.K, t.f8out))) cfg = f8copy_tile(cfg);      // (the loader-wave tilings on e4m3 operands carry the copy themselves)
    }
    int f8 = 0;
    if (!t.conv && t.fp8) {     // fp8 operands (tmix_gemm_fp8): a lock-step loop where asked for and possible, else the phase-offset loop -- 256x128 tiles for narrow N
        f8 = t.fp8;
        const int asked = cfg;
        if (f8_lockstep(cfg, t.K, t.f8out)) {
            f8 += 2;
            // the loader-wave instantiation at the 256-register limit of two waves per SIMD holds the staged plain / GEGLU epilogues only (the transposed and
            // narrow forms spill there, and scratch traffic would break the counted vmcnt): those launches run without loader waves
            if (TILINGS[cfg].lw && !staged) cfg = 12;
            // ... and the e4m3 copy of C in its straight-line form only (epilogue family 4: bf16 output, no activation, no row-group bias)
            if (TILINGS[cfg].lw && t.f8copy && (t.epilogue != TMIX_EPI_NONE || t.rowgroup_bias)) cfg = 12;
        } else
        cfg = (cfg == 17 || (cfg != 16 && (int64_t)((t.M + 255) / 256) * ((t.N + 255) / 256) * t.batch < 160)) ? 17 : 16;
        if (f8 == 2 && cfg == 16 && t.K / 32 > f8_block_cap(256)) cfg = 17;    // the tile's block scales stay in LDS beside the ring
        // the consumers of row_stats_out were told the partial count of the REQUESTED tiling (tmix_gemm_stats_parts): never change the width under them
        if (t.stats_out && TILINGS[asked].bn != TILINGS[cfg].bn)
            TMIX_REFUSE(TMIX_EINVAL, "gemm_fp8: tile_cfg %d cannot run this launch (K / 32 = %d block scales per row exceed the 256x256 tile's LDS budget); "
                                     "with row_stats_out request tile_cfg 17 explicitly", asked, t.K / 32);
    }
    if (t.conv && t.fp8) {      // convolution on e4m3 operands: the 128 x 160 lock-step tilings, with two loader waves (20) or without (12)
        f8 = 4;
        cfg = (tile_has(cfg, CAP_F8_LOCKSTEP) && TILINGS[cfg].lw) ? 20 : 12;
    } else if (t.conv) {
        if (!tile_has(cfg, CAP_CONV)) cfg = TILINGS[cfg].fb_conv;                  // GEMM-only mainloops: the nearest plain tiling
    } else if (cfg == 16 && !f8 && (t.K % 32)) cfg = 4;
    // 256x320 phase-offset: bf16, staged GEGLU / plain epilogues only (the transposed and narrow forms spill at its register count)
    if (!t.conv && cfg == 22 && (f8 || !staged)) cfg = f8 ? 16 : 14;
    // column statistics are compiled for the lock-step tilings only: the phase-offset ones run as their nearest plain tiling
    if (t.cs_out && !tile_has(cfg, CAP_CS)) cfg = TILINGS[cfg].fb;
    return {cfg, f8, TMIX_OK};
}

}  // namespace tmix_gemm

namespace {

TileTraits traits_of(int conv, const Params& p, int batch) {
    TileTraits t = {};
    t.conv = conv; t.fp8 = p.scaleA ? (p.ldScaleA ? 2 : 1) : 0;
    t.n_trans_begin = p.n_trans_begin; t.wide = p.wide; t.epilogue = p.epilogue;
    t.f8copy = p.f8copy; t.f8out = p.f8out; t.stats_out = p.stats_out; t.cs_out = p.cs_out; t.rowgroup_bias = p.rgb;
    t.M = p.M; t.N = p.N; t.K = p.K; t.batch = batch;
    t.w22_ok = w22_eligible(p, conv, 0); t.convh_ok = convh_eligible(p, conv, p.scaleA != nullptr);
    return t;
}

int launch(int conv, Params& p, int batch, int tile_cfg, hipStream_t st) {
    const TileChoice r = resolve_tile(traits_of(conv, p, batch), tile_cfg);
    if (r.err) return r.err;
    switch (r.cfg) {
    case 23: return launch_w22(p, batch, st);
    case 26: return launch_convh(p, st);
    }
    switch (r.f8 >= 3 ? 5 : TILINGS[r.cfg].group) {       // (group 5: the e4m3 lock-step forms of the CAP_F8_LOCKSTEP tilings)
    case 0: return launch_group0(r.cfg, conv, r.f8, p, batch, st);
    case 1: return launch_group1(r.cfg, conv, r.f8, p, batch, st);
    case 2: return launch_group2(r.cfg, conv, r.f8, p, batch, st);
    case 3: return launch_group3(r.cfg, conv, r.f8, p, batch, st);
    case 4: return launch_group4(r.cfg, conv, r.f8, p, batch, st);
    case 5: return launch_group5(r.cfg, conv, r.f8, p, batch, st);
    }
    return no_kernel(r.cfg);
}

}  // namespace

extern "C" int tmix_gemm_tile_shape(int tile_cfg, int* bm, int* bn) {
    if (tile_cfg < 1 || tile_cfg > NUM_CFG || !bm || !bn) TMIX_FAIL(TMIX_EINVAL, "gemm_tile_shape: tile_cfg=%d", tile_cfg);
    *bm = TILINGS[tile_cfg].bm; *bn = TILINGS[tile_cfg].bn;
    return TMIX_OK;
}

extern "C" int tmix_gemm_f8copy_tile(int tile_cfg) { return f8copy_tile(tile_cfg); }

extern "C" int tmix_gemm_stats_parts(int N, int tile_cfg) {
    int bm, bn;
    if (N <= 0 || tmix_gemm_tile_shape(tile_cfg, &bm, &bn) != TMIX_OK) return -1;
    return (N + bn - 1) / bn;
}

// argument validation and descriptor -> kernel parameters, shared by the launch entry points and tmix_gemm_resolve_tile (which passes any aligned non-null
// scale pointers: they are not dereferenced here).  fp8 = true: A / W hold OCP e4m3 bytes with one E8M0 scale per row (tmix_gemm_fp8); everything behind the
// main loop is shared.  qa: the launch is tmix_gemm_q_cross_attn (C may be NULL)
static int gemm_params(const tmix_gemm_desc* d, bool fp8, const uint8_t* scaleA, const uint8_t* scaleW, bool qa, Params& p) {
    if (!d || !d->A || !d->W) TMIX_FAIL(TMIX_EINVAL, "gemm: null descriptor/operand");
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch <= 0) TMIX_FAIL(TMIX_ESHAPE, "gemm: empty problem M=%d N=%d K=%d batch=%d", d->M, d->N, d->K, d->batch);
    if (d->K % BK) TMIX_FAIL(TMIX_ESHAPE, "gemm: K=%d must be a multiple of %d", d->K, BK);
    if (d->N % 4) TMIX_FAIL(TMIX_ESHAPE, "gemm: N=%d must be a multiple of 4", d->N);
    const int el = fp8 ? 1 : 2, al = 16 / el;            // element bytes, elements per 16 bytes
    if (fp8 && (!scaleA || !scaleW)) TMIX_FAIL(TMIX_EINVAL, "gemm_fp8: null scale vector");
    if ((d->lda % al) || (d->ldw % al) || (d->strideA % al) || (d->strideW % al)) TMIX_FAIL(TMIX_EALIGN, "gemm: lda/ldw/strides must be multiples of %d elements", al);
    if (!aligned16(d->A) || !aligned16(d->W)) TMIX_FAIL(TMIX_EALIGN, "gemm: A/W must be 16-byte aligned");
    const bool has_trans = d->n_trans_begin >= 0 && d->n_trans_begin < d->N;
    if (has_trans && (!d->Ct || (d->n_trans_begin % 128))) TMIX_FAIL(TMIX_EINVAL, "gemm: transposed region needs Ct and n_trans_begin %% 128 == 0");
    if ((!has_trans || d->n_trans_begin > 0) && !d->C && !qa) TMIX_FAIL(TMIX_EINVAL, "gemm: null C");
    if (d->C && ((d->ldc % 4) || (((uintptr_t)d->C) & 7) || (d->strideC % 4))) TMIX_FAIL(TMIX_EALIGN, "gemm: C must be 8-byte aligned with ldc %% 4 == 0");
    if (d->residual && ((d->ldr % 4) || (((uintptr_t)d->residual) & 7))) TMIX_FAIL(TMIX_EALIGN, "gemm: residual alignment");
    if (d->bias && (((uintptr_t)d->bias) & 15)) TMIX_FAIL(TMIX_EALIGN, "gemm: bias must be 16-byte aligned");
    if (d->rowgroup_bias && (d->rows_per_group <= 0 || (((uintptr_t)d->rowgroup_bias) & 15))) TMIX_FAIL(TMIX_EINVAL, "gemm: rowgroup_bias needs rows_per_group > 0 and 16-byte alignment");
    if (d->epilogue == TMIX_EPI_GEGLU && ((d->N % 32) || has_trans || d->residual || d->rowgroup_bias)) TMIX_FAIL(TMIX_EINVAL, "gemm: GEGLU needs N %% 32 == 0 and no residual/transposed region");
    if (d->epilogue < TMIX_EPI_NONE || d->epilogue > TMIX_EPI_QUICKGELU) TMIX_FAIL(TMIX_EINVAL, "gemm: bad epilogue %d", d->epilogue);
    if ((d->epilogue == TMIX_EPI_GELU || d->epilogue == TMIX_EPI_QUICKGELU) && (has_trans || d->residual)) TMIX_FAIL(TMIX_EINVAL, "gemm: activation epilogues take no residual/transposed region");
    if (d->epilogue == TMIX_EPI_F32OUT && (has_trans || (((uintptr_t)d->C) & 15))) TMIX_FAIL(TMIX_EINVAL, "gemm: fp32 output needs a 16-byte aligned C and no transposed region");
    if ((int64_t)d->M * d->lda >= (1ll << 31) || (int64_t)d->N * d->ldw >= (1ll << 31)) TMIX_FAIL(TMIX_ESHAPE, "gemm: operand extent exceeds 32-bit element offsets");
    if (d->w_period < 0 || (d->w_period > 0 && (d->batch % d->w_period))) TMIX_FAIL(TMIX_ESHAPE, "gemm: w_period=%d must divide batch=%d", d->w_period, d->batch);
    p = {};
    p.A = (const bf16_t*)d->A; p.lda = d->lda; p.strideA = d->strideA;
    // (w_period == batch is "every slice its own set": the plain strideW walk -- one group would make the magic divisor wrap to 1)
    const int wper = (d->w_period > 0 && d->w_period < d->batch) ? d->w_period : 0;
    p.w_period = wper; p.w_groups = wper ? d->batch / wper : 1;
    p.w_magic = (unsigned)((1ull << 32) / (unsigned)p.w_groups) + 1u;
    if (d->batch > 65535) TMIX_FAIL(TMIX_ESHAPE, "gemm: batch=%d exceeds the grid's 65535 slices", d->batch);
    p.W = (const bf16_t*)d->W; p.ldw = d->ldw; p.strideW = d->strideW;
    p.C = (bf16_t*)d->C; p.ldc = d->ldc; p.strideC = d->strideC;
    p.bias = d->bias; p.strideBias = d->strideBias;
    p.R = (const bf16_t*)d->residual; p.ldr = d->ldr; p.strideR = d->strideR;
    p.rgb = d->rowgroup_bias; p.rows_per_group = d->rows_per_group;
    p.Ct = (bf16_t*)d->Ct; p.ldct = d->ldct; p.strideCt = d->strideCt;
    p.n_trans_begin = has_trans ? d->n_trans_begin : -1;
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.epilogue = d->epilogue;
    p.bytesA = (unsigned)(((int64_t)(d->M - 1) * d->lda + d->K) * el);
    p.bytesW = (unsigned)(((int64_t)(d->N - 1) * d->ldw + d->K) * el);
    if (fp8) {
        const bool lockstep = f8_lockstep(d->tile_cfg, d->K, d->reserved0 & TMIX_F8_GEGLU_OUT);
        if (d->tile_cfg != TMIX_TILE_AUTO && d->tile_cfg != 16 && d->tile_cfg != 17 && !lockstep)
            TMIX_FAIL(TMIX_EINVAL, "gemm_fp8: tile_cfg must be AUTO, 16 (256x256), 17 (256x128) or -- K %% 128 == 0, no e4m3 GEGLU output -- 12 / 19 / 20 / 21 (128x160 without / with one, two, four loader waves)");
        p.scaleA = scaleA; p.scaleW = scaleW; p.strideScaleA = d->strideA ? d->M : 0; p.strideScaleW = d->strideW ? d->N : 0;
        if (d->reserved0 & TMIX_F8_A_BLOCK_SCALES) {
            p.ldScaleA = (int64_t)d->batch * d->M;                                                // [K/32][batch * M], dense
            if ((d->M % 4) || (((uintptr_t)scaleA) & 3)) TMIX_FAIL(TMIX_EALIGN, "gemm_fp8: block-scaled A needs M %% 4 == 0 and a 4-byte aligned scale array");
            if (!lockstep && d->K / 32 > f8_block_cap(128)) TMIX_FAIL(TMIX_ESHAPE, "gemm_fp8: block-scaled A supports K <= %d", 32 * f8_block_cap(128));
            if ((int64_t)(d->K / 32) * p.ldScaleA >= (1ll << 31)) TMIX_FAIL(TMIX_ESHAPE, "gemm_fp8: block scale array exceeds 32-bit offsets");
        }
        if (d->reserved0 & TMIX_F8_GEGLU_OUT) {
            if (d->epilogue != TMIX_EPI_GEGLU || !d->Ct || d->ldct < (int64_t)d->batch * d->M || (d->ldc % 8) || (d->strideC % 8) || (((uintptr_t)d->C) & 7))
                TMIX_FAIL(TMIX_EINVAL, "gemm_fp8: e4m3 GEGLU output needs the GEGLU epilogue, Ct = scale buffer [N/64][ldct >= batch*M] and 8-byte aligned C rows");
            p.f8out = 1; p.scale_out = (unsigned char*)d->Ct; p.ldScaleOut = d->ldct;
        }
    } else if (d->reserved0 & ~TMIX_F8_COPY_OUT) TMIX_FAIL(TMIX_EINVAL, "gemm: the fp8 operand flags in reserved0 belong to tmix_gemm_fp8");
    if (d->reserved0 & TMIX_F8_COPY_OUT) {
        if (has_trans || d->epilogue != TMIX_EPI_NONE || (d->reserved0 & TMIX_F8_GEGLU_OUT) || !d->Ct || (d->M % 32) || (d->N % 32) || (d->ldct % 8) || d->ldct < d->N
            || (((uintptr_t)d->Ct) & 7) || d->strideCt < (int64_t)d->batch * d->M * d->ldct)
            TMIX_FAIL(TMIX_EINVAL, "gemm: the e4m3 copy needs the plain bf16 epilogue, M %% 32 == 0, N %% 32 == 0, Ct = bytes [batch*M][ldct >= N, %% 8 == 0] and strideCt = byte offset of the scale array behind them");
        p.f8copy = (unsigned char*)d->Ct; p.ldF8copy = d->ldct;
        p.scale_out = (unsigned char*)d->Ct + d->strideCt; p.ldScaleOut = (int64_t)d->batch * d->M;
    }
    if (d->row_stats_out && (has_trans || d->epilogue != TMIX_EPI_NONE)) TMIX_FAIL(TMIX_EINVAL, "gemm: row_stats_out needs the plain bf16 epilogue");
    if (d->row_stats_out && (d->tile_cfg < 1 || d->tile_cfg > NUM_CFG || (((uintptr_t)d->row_stats_out) & 7) || (d->strideStatsOut & 1) || d->ldStatsOut < d->M))
        TMIX_FAIL(TMIX_EINVAL, "gemm: row_stats_out needs an explicit tile_cfg (its partial count depends on it) and 8-byte alignment");
    if (d->ln_stats && (!d->ln_colsum || !(d->ln_inv_c > 0.f) || d->ln_parts < 1 || d->ln_parts > 16 || (int64_t)d->ln_parts * d->ldLnStats * 8 >= (1ll << 31) || (((uintptr_t)d->ln_stats) & 7) || (d->strideLnStats & 1) || d->ldLnStats < d->M))
        TMIX_FAIL(TMIX_EINVAL, "gemm: fused LayerNorm needs ln_colsum, ln_inv_c > 0, 1 <= ln_parts <= 16 and 8-byte aligned ln_stats (< 2 GiB)");
    p.stats_out = d->row_stats_out; p.strideStatsOut = d->strideStatsOut; p.ldStatsOut = d->ldStatsOut;
    p.ln_stats = d->ln_stats; p.strideLnStats = d->strideLnStats; p.ldLnStats = d->ldLnStats; p.ln_parts = d->ln_parts;
    p.ln_colsum = d->ln_colsum; p.strideLnColsum = d->strideLnColsum; p.ln_inv_c = d->ln_inv_c; p.ln_eps = d->ln_eps;
    // LDS-staged 16-byte stores need 16-byte aligned rows (the narrow 8-byte form stays as the fallback for odd strides)
    const bool c16 = d->C && aligned16(d->C) && (d->ldc % 8) == 0 && (d->strideC % 8) == 0;
    const bool r16 = !d->residual || (aligned16(d->residual) && (d->ldr % 8) == 0 && (d->strideR % 8) == 0);
    p.wide = 0;
    if (!tmix_env(TMIX_ENV_NARROW_EPILOGUE)) {
        if (d->epilogue == TMIX_EPI_GEGLU) { if (c16 || p.f8out) p.wide |= 2; }
        else if (d->epilogue == TMIX_EPI_F32OUT) { if (aligned16(d->C) && (d->ldc % 4) == 0 && (d->strideC % 4) == 0 && (d->N % 8) == 0) p.wide |= 1; }
        else if (c16 && r16 && (d->N % 8) == 0) p.wide |= 1;
        if (has_trans && aligned16(d->Ct) && (d->ldct % 8) == 0 && (d->strideCt % 8) == 0) p.wide |= 4;
    }
    if (d->col_stats_out) {
        if (fp8) TMIX_FAIL(TMIX_EINVAL, "gemm_fp8: col_stats_out is compiled for the bf16 tilings only (the fp8 loop would be remapped to a bf16 kernel over e4m3 bytes)");
        if (has_trans || d->epilogue != TMIX_EPI_NONE || d->row_stats_out || (d->reserved0 & TMIX_F8_COPY_OUT) || d->batch != 1 || (d->M % TMIX_COLSTATS_ROWS) || (d->N % 8)
            || !aligned16(d->col_stats_out) || !(p.wide & 1))
            TMIX_FAIL(TMIX_EINVAL, "gemm: col_stats_out needs the plain staged bf16 epilogue (16-byte aligned C / residual rows, N %% 8 == 0), batch == 1, M %% 32 == 0, "
                                   "and neither row_stats_out nor the e4m3 copy");
        p.cs_out = d->col_stats_out;
    }
    if (p.f8out && !(p.wide & 2)) TMIX_FAIL(TMIX_EINVAL, "gemm_fp8: e4m3 GEGLU output needs the staged epilogue");
    if (p.f8copy && !(p.wide & 1)) TMIX_FAIL(TMIX_EALIGN, "gemm: the e4m3 copy needs the staged epilogue (16-byte aligned C / residual rows, N %% 8 == 0)");
    if (fp8 && has_trans && !(p.wide & 4)) TMIX_FAIL(TMIX_EALIGN, "gemm_fp8: the transposed region needs a 16-byte aligned Ct with ldct %% 8 == 0");
    return TMIX_OK;
}

static int gemm_entry(const tmix_gemm_desc* d, bool fp8, const uint8_t* scaleA, const uint8_t* scaleW, void* stream, const QAExtra* qa = nullptr) {
    Params p;
    if (const int rc = gemm_params(d, fp8, scaleA, scaleW, qa != nullptr, p)) return rc;
    if (qa) return launch_qattn(p, *qa, d->batch, (hipStream_t)stream);
    return launch(0, p, d->batch, d->tile_cfg, (hipStream_t)stream);
}

// scale arrays of the tile queries: never read
alignas(16) static const uint8_t NO_SCALES[16] = {};

extern "C" int tmix_gemm_resolve_tile(const tmix_gemm_desc* d, int fp8_operands) {
    Params p;
    if (const int rc = gemm_params(d, fp8_operands != 0, fp8_operands ? NO_SCALES : nullptr, fp8_operands ? NO_SCALES : nullptr, false, p)) return rc;
    const TileChoice r = resolve_tile(traits_of(0, p, d->batch), d->tile_cfg);
    return r.err ? r.err : r.cfg;
}

// attn2.to_q (the projection described by d: A = hidden state rows, W = to_q weight, bias / folded LayerNorm as in tmix_gemm_bf16; d->C is not written) and
// the cross-attention of its output against cached K [images][Skv][ldk] / V^T [images][N][ldvt = 80] in one launch: O [batch * M][ldo] receives
// softmax(q K^T * scale) V per 64-wide head.  rows_per_image: consecutive rows of A that share an image's keys (the latent's token count).
extern "C" int tmix_gemm_q_cross_attn(const tmix_gemm_desc* d, const void* K, int64_t ldk, int64_t strideK, const void* Vt, int64_t ldvt, int64_t strideVt,
                                      void* O, int64_t ldo, int rows_per_image, int Skv, float scale, void* stream) {
    if (!d) TMIX_FAIL(TMIX_EINVAL, "gemm_q_cross_attn: null descriptor");
    if (d->reserved0 || d->residual || d->row_stats_out || d->col_stats_out || d->rowgroup_bias || d->epilogue != TMIX_EPI_NONE || (d->n_trans_begin >= 0 && d->n_trans_begin < d->N))
        TMIX_FAIL(TMIX_EINVAL, "gemm_q_cross_attn: the projection takes a bias and a folded LayerNorm only");
    const QAExtra x = {K, ldk, strideK, Vt, ldvt, strideVt, O, ldo, rows_per_image, Skv, scale};
    return gemm_entry(d, false, nullptr, nullptr, stream, &x);
}

extern "C" int tmix_gemm_bf16(const tmix_gemm_desc* d, void* stream) { return gemm_entry(d, false, nullptr, nullptr, stream); }

extern "C" int tmix_gemm_fp8(const tmix_gemm_desc* d, const uint8_t* scale_a, const uint8_t* scale_w, void* stream) {
    return gemm_entry(d, true, scale_a, scale_w, stream);
}

static int conv_params(const tmix_conv_desc* d, const uint8_t* scale_x, const uint8_t* scale_w, Params& p) {
    const bool fp8 = scale_x != nullptr;
    if (!d || !d->X || !d->Wt || !d->Y) TMIX_FAIL(TMIX_EINVAL, "conv3x3: null descriptor/operand");
    if (fp8 && (!scale_w || (d->Cin % 128) || d->S1 || d->S2 || (((uintptr_t)scale_x) & 3)))
        TMIX_FAIL(TMIX_EINVAL, "conv3x3_fp8: needs both scale arrays (scale_x 4-byte aligned), Cin %% 128 == 0 and no shortcut taps");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: empty problem");
    if (d->Cin % BK) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: Cin=%d must be a multiple of %d", d->Cin, BK);
    if (d->Cout % 4) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: Cout=%d must be a multiple of 4", d->Cout);
    if (d->mode < TMIX_CONV_S1 || d->mode > TMIX_CONV_UP2F) TMIX_FAIL(TMIX_EINVAL, "conv3x3: bad mode %d", d->mode);
    const bool fold = d->mode == TMIX_CONV_UP2F;      // nearest x2 folded into four 2x2 phase convolutions: Wt [4][Cout][2][2][Cin], K = 4 Cin
    if (fold && (fp8 || d->residual || d->S1 || d->S2)) TMIX_FAIL(TMIX_EINVAL, "conv3x3: the folded upsampling mode takes bf16 operands, no residual and no shortcut taps");
    if (fold && (d->W < 2 || (int64_t)d->H * d->W * d->W >= (1ll << 32))) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: the folded upsampling mode needs W >= 2 and H * W * W < 2^32");
    if ((d->mode == TMIX_CONV_S2 || d->mode == TMIX_CONV_S2A) && ((d->H | d->W) & 1)) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: stride-2 needs even H,W");
    if (!aligned16(d->X) || !aligned16(d->Wt) || (((uintptr_t)d->Y) & 7)) TMIX_FAIL(TMIX_EALIGN, "conv3x3: pointer alignment");
    if ((d->bias && (((uintptr_t)d->bias) & 15)) || (d->batch_bias && (((uintptr_t)d->batch_bias) & 15))) TMIX_FAIL(TMIX_EALIGN, "conv3x3: bias alignment");
    p = {};
    p.H = d->H; p.Wd = d->W; p.Cin = d->Cin; p.mode = d->mode;
    p.ntaps = d->mode == TMIX_CONV_T3 ? 3 : (fold ? 4 : 9);
    if (fold) { p.up_hw = d->H * d->W; p.up_magic = (unsigned)((1ull << 32) / (unsigned)d->W) + 1u; }
    const bool half = d->mode == TMIX_CONV_S2 || d->mode == TMIX_CONV_S2A;
    const bool up = d->mode == TMIX_CONV_UP2 || fold;
    p.Ho = half ? d->H / 2 : (up ? d->H * 2 : d->H);
    p.Wo = half ? d->W / 2 : (up ? d->W * 2 : d->W);
    const int64_t M = (int64_t)d->B * p.Ho * p.Wo;
    if (M > 0x7fffffff / 4) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: too many output pixels");
    if ((int64_t)d->B * d->H * d->W * d->Cin >= (1ll << 30) || (int64_t)d->Cout * 9 * d->Cin >= (1ll << 30)) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: operand larger than 2 GiB");
    p.A = (const bf16_t*)d->X;
    p.W = (const bf16_t*)d->Wt; p.ldw = p.ntaps * (int64_t)d->Cin;
    p.C = (bf16_t*)d->Y; p.ldc = d->Cout;
    p.bias = d->bias;
    p.R = (const bf16_t*)d->residual; p.ldr = d->Cout;
    p.rgb = d->batch_bias; p.rows_per_group = p.Ho * p.Wo * (d->batch_bias_images > 1 ? d->batch_bias_images : 1);
    p.n_trans_begin = -1;
    p.M = (int)M; p.N = d->Cout; p.K = p.ntaps * d->Cin;
    if (d->S1 || d->S2) {            // shortcut taps behind the nine conv taps
        const int c1 = d->S1_channels, c2 = d->S2 ? d->S2_channels : 0;
        if (!d->S1 || d->mode != TMIX_CONV_S1 || c1 <= 0 || (c1 % BK) || c2 < 0 || (c2 % BK) || (d->S2 && c2 == 0) || !aligned16(d->S1) || (d->S2 && !aligned16(d->S2)) || d->residual)
            TMIX_FAIL(TMIX_EINVAL, "conv3x3: shortcut taps need the stride-1 mode, S1 (S2 only with S1), channel counts that are multiples of %d, 16-byte alignment and no residual", BK);
        if ((int64_t)d->B * d->H * d->W * (c1 > c2 ? c1 : c2) >= (1ll << 30) || (int64_t)d->Cout * (9ll * d->Cin + c1 + c2) >= (1ll << 30)) TMIX_FAIL(TMIX_ESHAPE, "conv3x3: shortcut operand larger than 2 GiB");
        p.S1 = (const bf16_t*)d->S1; p.S2 = (const bf16_t*)d->S2; p.c1s = c1; p.c2s = c2;
        p.bytesS1 = (unsigned)((int64_t)d->B * d->H * d->W * c1 * 2); p.bytesS2 = (unsigned)((int64_t)d->B * d->H * d->W * c2 * 2);
        p.K += c1 + c2;
        p.ldw = p.K;
    }
    p.epilogue = TMIX_EPI_NONE;
    p.bytesA = (unsigned)((int64_t)d->B * d->H * d->W * d->Cin * (fp8 ? 1 : 2));
    p.bytesW = (unsigned)((int64_t)d->Cout * p.K * (fp8 ? 1 : 2));
    if (fp8) { p.scaleA = scale_x; p.scaleW = scale_w; p.ldScaleA = d->Cin / 32; }
    p.wide = (!tmix_env(TMIX_ENV_NARROW_EPILOGUE) && aligned16(d->Y) && (d->Cout % 8) == 0 && (!d->residual || aligned16(d->residual))) ? 1 : 0;
    if (p.S1 && !p.wide) TMIX_FAIL(TMIX_EALIGN, "conv3x3: shortcut taps need the staged epilogue (16-byte aligned Y, Cout %% 8 == 0)");
    if (d->col_stats_out) {
        if ((M % TMIX_COLSTATS_ROWS) || !aligned16(d->col_stats_out) || !p.wide)
            TMIX_FAIL(TMIX_EINVAL, "conv3x3: col_stats_out needs B*Ho*Wo %% 32 == 0, Cout %% 8 == 0 and 16-byte aligned Y / residual");
        p.cs_out = d->col_stats_out;
    }
    return TMIX_OK;
}

// TMIX_CONV_UP2F: a tile of the kernel that runs the launch must lie inside one (image, phase) -- the phase's weight set and the store row are wave-uniform
static int conv_resolve(const Params& p, int tile_cfg, int& cfg) {
    const TileChoice r = resolve_tile(traits_of(1, p, 1), tile_cfg);
    if (r.err) return r.err;
    if (p.mode == TMIX_CONV_UP2F && (p.up_hw % TILINGS[r.cfg].bm))
        TMIX_FAIL(TMIX_ESHAPE, "conv3x3: the folded upsampling mode needs H * W = %d to be a multiple of the %d rows of tiling %d (use TMIX_CONV_UP2)", p.up_hw, TILINGS[r.cfg].bm, r.cfg);
    cfg = r.cfg;
    return TMIX_OK;
}

static int conv_entry(const tmix_conv_desc* d, const uint8_t* scale_x, const uint8_t* scale_w, void* stream) {
    Params p;
    if (const int rc = conv_params(d, scale_x, scale_w, p)) return rc;
    int cfg;
    if (const int rc = conv_resolve(p, d->tile_cfg, cfg)) return rc;
    return launch(1, p, 1, d->tile_cfg, (hipStream_t)stream);
}

extern "C" int tmix_conv_resolve_tile(const tmix_conv_desc* d, int fp8_operands) {
    Params p;
    if (const int rc = conv_params(d, fp8_operands ? NO_SCALES : nullptr, fp8_operands ? NO_SCALES : nullptr, p)) return rc;
    int cfg;
    if (const int rc = conv_resolve(p, d->tile_cfg, cfg)) return rc;
    return cfg;
}

extern "C" int tmix_conv3x3_nhwc(const tmix_conv_desc* d, void* stream) { return conv_entry(d, nullptr, nullptr, stream); }

extern "C" int tmix_conv3x3_nhwc_fp8(const tmix_conv_desc* d, const uint8_t* scale_x, const uint8_t* scale_w, void* stream) {
    if (!scale_x) TMIX_FAIL(TMIX_EINVAL, "conv3x3_fp8: null scale array");
    return conv_entry(d, scale_x, scale_w, stream);
}
