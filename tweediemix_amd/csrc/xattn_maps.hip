// xattn_maps.hip -- cross-attention token maps (tmix_xattn_token_maps): for selected batch rows of an attn2 call, the softmax
// probability every query pixel puts on a few prompt tokens, summed over heads.  The localisation signal of prompt-to-prompt /
// DAAM; masks.attention_masks turns the maps into blend masks.  Runs in the look-ahead only (probe plans), never in a fusion step.
//
// One workgroup of 4 waves per (selected row, 32-query tile).  Wave w takes heads w, w+4, ... in increasing order; per head the
// scores S^T = K . Q^T of the tile are 3 x 4 v_mfma_f32_32x32x16_bf16 (3 key tiles of 32 cover Lk <= 80, 4 k-steps of 16 over the
// head's 64 columns), with the operands loaded straight from global memory (K of one head is 10 KB and stays in the caches).  The
// accumulator has the query on the lane (column = lane & 31) and 16 keys in its registers, the other 16 of the key tile in lane ^ 32,
// so the fp32 row max and exp-sum are an in-lane pass plus one exchange with lane ^ 32.  Only the n_tok probabilities of a head are
// kept.  The 4 waves' partial sums meet in LDS and ONE thread per (token, query) adds them in wave order and stores: no atomics, a
// fixed reduction order, and nothing that depends on the other rows of the batch.
//
// tmix_xattn_token_maps_long (chunked prompts: Lk <= 240 keys, up to 32 positions) is the same workgroup with NKT = 3, 5 or 8 key tiles
// of 32 (Lk <= 96 / 160 / 240).  It KEEPS the scores of all its key tiles in registers -- one pass over K, not a maximum-and-sum
// pass followed by a second one for the selected positions: at NKT = 8 the compiler reports 167 VGPRs + 128 AGPRs (the 8 x 16
// scores) and no scratch for gfx950 (NKT = 5: 112 + 80, NKT = 3: 78 + 48), and a workgroup of 4 waves is one wave per SIMD, which may
// use 512; the two-pass form would load K and run every MFMA twice to save registers nothing else wants.  What changes against the short kernel is the tail: the
// positions are walked in a rolled loop (32 unrolled copies of an 8-way tile select are not worth their code), so a wave adds its
// heads' probabilities into its OWN LDS slice part[w] (same lane, same address, program order: still one fixed order, heads
// ascending) instead of into registers, and the 256 threads then own 8 positions x 32 queries per round of the final store.
// For Lk <= 80 and n_tok <= 8 the long entry point forwards to the short one: the same launch, the same bits.
#include "common.h"

namespace {

constexpr int XM_QT = 32;        // queries per workgroup
constexpr int XM_WAVES = 4;
constexpr int XM_MAXTOK = 8;
constexpr int XM_MAXKEYS = 80;   // 3 key tiles of 32

struct XmTokens { int tok[XM_MAXTOK]; };     // by value in the kernel arguments: a captured graph holds the positions

typedef __attribute__((ext_vector_type(8))) __bf16 xm_frag;

// 8 bf16 at p (8-byte aligned: two 8-byte loads), or zeros
__device__ __forceinline__ xm_frag xm_load8(const bf16_t* p, bool ok) {
    uint2 a = make_uint2(0u, 0u), b = make_uint2(0u, 0u);
    if (ok) {
        a = *(const uint2*)p;
        b = *(const uint2*)(p + 4);
    }
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const u32x4 v = {a.x, a.y, b.x, b.y};
    return __builtin_bit_cast(xm_frag, v);
}

__global__ __launch_bounds__(XM_QT * 2 * XM_WAVES) void xattn_token_maps_kernel(
        const bf16_t* __restrict__ Q, int64_t ldq, int64_t strideQ, const bf16_t* __restrict__ K, int64_t ldk, int64_t strideK,
        float* __restrict__ maps, int H, int Sq, int Lk, int row0, int row_step, XmTokens tp, int n_tok, int accumulate, float scale_log2) {
    __shared__ float part[XM_WAVES][XM_MAXTOK][XM_QT];
    const int i = blockIdx.y;                                   // selected row
    const int64_t b = (int64_t)row0 + (int64_t)i * row_step;    // batch row
    const int s0 = blockIdx.x * XM_QT;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 31, hf = lane >> 5;                    // query column of the tile, lane half
    const bool qok = s0 + c < Sq;
    const bf16_t* qrow = Q + b * strideQ + (int64_t)(qok ? s0 + c : 0) * ldq + hf * 8;
    const bf16_t* kbase = K + b * strideK + hf * 8;

    float acc[XM_MAXTOK];
#pragma unroll
    for (int j = 0; j < XM_MAXTOK; ++j) acc[j] = 0.f;

    for (int h = w; h < H; h += XM_WAVES) {
        f32x16 sc[3];
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[kt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const xm_frag bq = xm_load8(qrow + h * 64 + ks * 16, qok);          // B[k = 8 hf + j][col c] = Q[c][16 ks + 8 hf + j]
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const int key = kt * 32 + c;
                const bool kok = key < Lk;
                const xm_frag ak = xm_load8(kbase + (int64_t)(kok ? key : 0) * ldk + h * 64 + ks * 16, kok);   // A[row key][k]
                sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, bq, sc[kt], 0, 0, 0);
            }
        }
        // sc[kt][r]: key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hf of query c, unscaled.  Softmax in fp32 over the Lk real keys: the lane's
        // valid keys are those below lim, padding keys become -inf (exp2 -> 0)
        int lim = Lk - 4 * hf;
        asm volatile("" : "+v"(lim));                           // (keeps the 48 key tests in the loop: hoisted, their masks spill)
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[kt][r] = kt * 32 + (r & 3) + 8 * (r >> 2) < lim ? sc[kt][r] * scale_log2 : -INFINITY;
                m = fmaxf(m, sc[kt][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) l += exp2f(sc[kt][r] - m);
        l = l + __shfl_xor(l, 32);                              // the same sum in both halves (fp32 addition commutes)
        const float inv_l = 1.0f / l;
#pragma unroll
        for (int j = 0; j < XM_MAXTOK; ++j) {
            if (j >= n_tok) break;
            const int tk = tp.tok[j];                           // wave-uniform: which tile / register / lane half holds it
            const int tkt = tk >> 5, tr = tk & 31;
            const int thf = (tr >> 2) & 1, treg = (tr & 3) + 4 * (tr >> 3);
            const f32x16 st = tkt == 0 ? sc[0] : (tkt == 1 ? sc[1] : sc[2]);
            const float v = st[treg];                           // uniform index: one relative register move
            const float vo = __shfl_xor(v, 32);
            const float t = hf == thf ? v : vo;
            acc[j] += exp2f(t - m) * inv_l;
        }
    }
    if (hf == 0) {
#pragma unroll
        for (int j = 0; j < XM_MAXTOK; ++j)
            if (j < n_tok) part[w][j][c] = acc[j];
    }
    __syncthreads();
    const int j = threadIdx.x / XM_QT, q = threadIdx.x % XM_QT;      // 256 threads = 8 tokens x 32 queries: one owner each
    if (j < n_tok && s0 + q < Sq) {
        float v = part[0][j][q];
#pragma unroll
        for (int ww = 1; ww < XM_WAVES; ++ww) v += part[ww][j][q];
        float* o = maps + ((int64_t)i * n_tok + j) * Sq + s0 + q;
        *o = accumulate ? *o + v : v;
    }
}

constexpr int XL_MAXTOK = 32;
constexpr int XL_MAXKEYS = 240;  // 8 key tiles of 32, V^T / K rows padded to a multiple of 8 keys stay below 256

struct XlTokens { int tok[XL_MAXTOK]; };     // by value, like XmTokens

template <int NKT>
__global__ __launch_bounds__(XM_QT * 2 * XM_WAVES) void xattn_token_maps_long_kernel(
        const bf16_t* __restrict__ Q, int64_t ldq, int64_t strideQ, const bf16_t* __restrict__ K, int64_t ldk, int64_t strideK,
        float* __restrict__ maps, int H, int Sq, int Lk, int row0, int row_step, XlTokens tp, int n_tok, int accumulate, float scale_log2) {
    __shared__ float part[XM_WAVES][XL_MAXTOK][XM_QT];
    const int i = blockIdx.y;                                   // selected row
    const int64_t b = (int64_t)row0 + (int64_t)i * row_step;    // batch row
    const int s0 = blockIdx.x * XM_QT;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 31, hf = lane >> 5;                    // query column of the tile, lane half
    const bool qok = s0 + c < Sq;
    const bf16_t* qrow = Q + b * strideQ + (int64_t)(qok ? s0 + c : 0) * ldq + hf * 8;
    const bf16_t* kbase = K + b * strideK + hf * 8;

    if (hf == 0)                                                // part[w][j][c] belongs to lane c of wave w until the barrier
        for (int j = 0; j < n_tok; ++j) part[w][j][c] = 0.f;

    for (int h = w; h < H; h += XM_WAVES) {
        f32x16 sc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[kt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const xm_frag bq = xm_load8(qrow + h * 64 + ks * 16, qok);          // B[k = 8 hf + j][col c] = Q[c][16 ks + 8 hf + j]
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const int key = kt * 32 + c;
                const bool kok = key < Lk;
                const xm_frag ak = xm_load8(kbase + (int64_t)(kok ? key : 0) * ldk + h * 64 + ks * 16, kok);   // A[row key][k]
                sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, bq, sc[kt], 0, 0, 0);
            }
        }
        // as in the short kernel: sc[kt][r] is key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hf of query c; fp32 softmax over the Lk real keys
        int lim = Lk - 4 * hf;
        asm volatile("" : "+v"(lim));
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[kt][r] = kt * 32 + (r & 3) + 8 * (r >> 2) < lim ? sc[kt][r] * scale_log2 : -INFINITY;
                m = fmaxf(m, sc[kt][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) l += exp2f(sc[kt][r] - m);
        l = l + __shfl_xor(l, 32);
        const float inv_l = 1.0f / l;
        for (int j = 0; j < n_tok; ++j) {
            const int tk = tp.tok[j];                           // wave-uniform: which tile / register / lane half holds it
            const int tkt = tk >> 5, tr = tk & 31;
            const int thf = (tr >> 2) & 1, treg = (tr & 3) + 4 * (tr >> 3);
            float v = 0.f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
                if (tkt == kt) v = sc[kt][treg];                // uniform branch, uniform index into one tile's 16 registers
            const float vo = __shfl_xor(v, 32);
            const float t = hf == thf ? v : vo;
            if (hf == 0) part[w][j][c] += exp2f(t - m) * inv_l;
        }
    }
    __syncthreads();
    const int q = threadIdx.x % XM_QT;
    for (int j = threadIdx.x / XM_QT; j < n_tok; j += 2 * XM_WAVES) {      // 256 threads = 8 positions x 32 queries per round: one owner each
        if (s0 + q < Sq) {
            float v = part[0][j][q];
#pragma unroll
            for (int ww = 1; ww < XM_WAVES; ++ww) v += part[ww][j][q];
            float* o = maps + ((int64_t)i * n_tok + j) * Sq + s0 + q;
            *o = accumulate ? *o + v : v;
        }
    }
}

}  // namespace

extern "C" int tmix_xattn_token_maps(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                                     float* maps, int B, int H, int Sq, int Lk, int row0, int row_step, int n_rows,
                                     const int32_t* tokens, int n_tok, int accumulate, float scale, void* stream) {
    if (!Q || !K || !maps || !tokens) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps: null pointer");
    if (n_tok < 1 || n_tok > XM_MAXTOK) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps: n_tok=%d (1..%d)", n_tok, XM_MAXTOK);
    if (B < 1 || H < 1 || Sq < 1 || Lk < 1 || Lk > XM_MAXKEYS)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps: B=%d H=%d Sq=%d Lk=%d (Lk <= %d)", B, H, Sq, Lk, XM_MAXKEYS);
    if (n_rows < 1 || n_rows > 65535 || row0 < 0 || row_step < 1 || (int64_t)row0 + (int64_t)(n_rows - 1) * row_step >= B)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps: rows row0=%d row_step=%d n_rows=%d outside a batch of %d", row0, row_step, n_rows, B);
    if (ldq < (int64_t)H * 64 || ldk < (int64_t)H * 64 || strideQ < 0 || strideK < 0)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps: ldq=%lld ldk=%lld narrower than H*64=%d", (long long)ldq, (long long)ldk, H * 64);
    if ((((uintptr_t)Q) & 7) || (((uintptr_t)K) & 7) || (((uintptr_t)maps) & 7) || (ldq % 4) || (ldk % 4) || (strideQ % 4) || (strideK % 4))
        TMIX_FAIL(TMIX_EALIGN, "xattn_token_maps: pointers must be 8-byte aligned, ld / stride multiples of 4 elements");
    if (!(scale > 0.f) || scale > 1e30f) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps: scale=%g", (double)scale);
    XmTokens tp;
    for (int j = 0; j < XM_MAXTOK; ++j) {
        tp.tok[j] = j < n_tok ? tokens[j] : 0;
        if (j < n_tok && (tokens[j] < 0 || tokens[j] >= Lk))
            TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps: token position %d outside 0..%d", tokens[j], Lk - 1);
    }
    const dim3 grid((unsigned)((Sq + XM_QT - 1) / XM_QT), (unsigned)n_rows);
    xattn_token_maps_kernel<<<grid, XM_QT * 2 * XM_WAVES, 0, (hipStream_t)stream>>>(
        (const bf16_t*)Q, ldq, strideQ, (const bf16_t*)K, ldk, strideK, maps, H, Sq, Lk, row0, row_step, tp, n_tok, accumulate ? 1 : 0,
        scale * LOG2E);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_xattn_token_maps_long(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                                          float* maps, int B, int H, int Sq, int Lk, int row0, int row_step, int n_rows,
                                          const int32_t* tokens, int n_tok, int accumulate, float scale, void* stream) {
    if (!Q || !K || !maps || !tokens) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps_long: null pointer");
    if (n_tok < 1 || n_tok > XL_MAXTOK) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps_long: n_tok=%d (1..%d)", n_tok, XL_MAXTOK);
    if (B < 1 || H < 1 || Sq < 1 || Lk < 1 || Lk > XL_MAXKEYS)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps_long: B=%d H=%d Sq=%d Lk=%d (Lk <= %d)", B, H, Sq, Lk, XL_MAXKEYS);
    if (Lk <= XM_MAXKEYS && n_tok <= XM_MAXTOK)                 // the short form's launch and bits (it validates the rest)
        return tmix_xattn_token_maps(Q, ldq, strideQ, K, ldk, strideK, maps, B, H, Sq, Lk, row0, row_step, n_rows, tokens, n_tok, accumulate, scale, stream);
    if (n_rows < 1 || n_rows > 65535 || row0 < 0 || row_step < 1 || (int64_t)row0 + (int64_t)(n_rows - 1) * row_step >= B)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps_long: rows row0=%d row_step=%d n_rows=%d outside a batch of %d", row0, row_step, n_rows, B);
    if (ldq < (int64_t)H * 64 || ldk < (int64_t)H * 64 || strideQ < 0 || strideK < 0)
        TMIX_FAIL(TMIX_ESHAPE, "xattn_token_maps_long: ldq=%lld ldk=%lld narrower than H*64=%d", (long long)ldq, (long long)ldk, H * 64);
    if ((((uintptr_t)Q) & 7) || (((uintptr_t)K) & 7) || (((uintptr_t)maps) & 7) || (ldq % 4) || (ldk % 4) || (strideQ % 4) || (strideK % 4))
        TMIX_FAIL(TMIX_EALIGN, "xattn_token_maps_long: pointers must be 8-byte aligned, ld / stride multiples of 4 elements");
    if (!(scale > 0.f) || scale > 1e30f) TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps_long: scale=%g", (double)scale);
    XlTokens tp;
    for (int j = 0; j < XL_MAXTOK; ++j) {
        tp.tok[j] = j < n_tok ? tokens[j] : 0;
        if (j < n_tok && (tokens[j] < 0 || tokens[j] >= Lk))
            TMIX_FAIL(TMIX_EINVAL, "xattn_token_maps_long: token position %d outside 0..%d", tokens[j], Lk - 1);
    }
    const dim3 grid((unsigned)((Sq + XM_QT - 1) / XM_QT), (unsigned)n_rows);
    const auto kern = Lk <= 96 ? xattn_token_maps_long_kernel<3> : (Lk <= 160 ? xattn_token_maps_long_kernel<5> : xattn_token_maps_long_kernel<8>);
    kern<<<grid, XM_QT * 2 * XM_WAVES, 0, (hipStream_t)stream>>>(
        (const bf16_t*)Q, ldq, strideQ, (const bf16_t*)K, ldk, strideK, maps, H, Sq, Lk, row0, row_step, tp, n_tok, accumulate ? 1 : 0,
        scale * LOG2E);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
