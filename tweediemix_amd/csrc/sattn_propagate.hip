// sattn_propagate.hip -- token maps pushed through self-attention (tmix_sattn_propagate): for selected batch rows of an attn1 call,
//   dst[i][j][s] (+)= out_scale * sum_h sum_s' softmax_s'(scale * q[b,s,h,:] . k[b,s',h,:]) * src[i][j][s'],
// the row-stochastic attn1 matrix of every head applied to up to 32 fp32 maps and summed over heads.  Pixels of one object attend to
// each other, so one pass spreads a partial cross-attention response over the object and averages isolated speckle away (the
// refinement step of the DAAM-based segmentation papers).  Runs in the look-ahead's "propagate" plans only, never in a fusion step.
//
// Flash-attention forward whose V is the maps: src^T is [n_tok <= 32] x S and shared by all heads.  One workgroup of 8 waves per
// (selected row, 32-query tile), wave w takes heads w, w+8, ... in increasing order (8, not xattn_maps.hip's 4: the grid is only S / 32 workgroups per
// row -- 32 at the 32^2 level of a 1024^2 image -- so the heads a wave walks one after the other are the launch's length; 4 waves measured 198 us there).
// Per 32-key tile the scores S^T = K . Q^T are 4 v_mfma_f32_32x32x16_bf16 with the operands straight from global memory (as xattn_maps.hip), and a
// tile's K rows and src values are requested a whole tile ahead (unconditional loads on clamped addresses, so that the wait in front of a tile's first MFMA counts only the loads of that tile).  The accumulator has the query on the lane and 16 keys in its registers, the other 16 in lane ^ 32: the
// running max and sum are an in-lane pass plus one exchange.  The exponentials, rounded to bf16 (nearest even), are the B operand of
// the second product directly from those registers: registers 8s .. 8s+7 are k-step s, whose element j of lane half hf is key
// 16 s + 8 (j >> 2) + 4 hf + (j & 3) of the tile -- the A operand (the src tile in bf16, token on the lane row, rows >= n_tok zero)
// is gathered in that same order (the trick of temporal_attn.hip).  The fp32 accumulator [32 tokens x 32 queries] is rescaled when
// the running maximum moves, divided by the head's fp32 sum at the end of the head and added to the wave's total.  The 8 waves'
// totals meet in LDS and ONE thread per output adds them in wave order and stores: no atomics, a fixed reduction order, nothing that
// depends on the other rows of the batch.  Nothing behind row S - 1 of Q, K, src or dst is ever read or written, and keys past S never contribute.
#include "common.h"

namespace {

constexpr int SP_QT = 32;        // queries per workgroup
constexpr int SP_KT = 32;        // keys per tile
constexpr int SP_WAVES = 8;
constexpr int SP_MAXTOK = 32;

typedef __attribute__((ext_vector_type(8))) __bf16 sp_frag;
typedef __attribute__((ext_vector_type(4))) unsigned sp_u32x4;

// Every load of the main loop is UNCONDITIONAL on a clamped address: a load behind a per-lane test becomes a branch around it, and the compiler then
// waits for all outstanding loads (vmcnt(0)) in front of the tile's first MFMA -- the loads just issued for the NEXT tile included.  What a clamped
// load brings in where the real index is out of range never counts: K rows >= S give scores that are masked to -inf, queries >= S are never written,
// and src values at keys >= S or rows >= n_tok are replaced by zero when the fragment is packed, one tile later.

// 8 bf16 at p (8-byte aligned: two 8-byte loads)
__device__ __forceinline__ sp_frag sp_load8(const bf16_t* p) {
    const uint2 a = *(const uint2*)p, b = *(const uint2*)(p + 4);
    const sp_u32x4 v = {a.x, a.y, b.x, b.y};
    return __builtin_bit_cast(sp_frag, v);
}

// The src values of one 32-key tile that this lane's two A fragments of the second product are made of, raw fp32: four runs of 4 keys, run g at
// key + 8 g (key = tile start + 4 hf): runs 0, 1 are k-step 0, runs 2, 3 k-step 1 -- element j of k-step s of lane half hf is key 16 s + 8 (j >> 2) + 4 hf + (j & 3)
// of the tile, the order the accumulator registers of the first product have.  VEC (S % 4 == 0, src 16-byte aligned): a run lies wholly below S or wholly
// behind it, one 16-byte load per run.
template <bool VEC>
__device__ __forceinline__ void sp_load_src(const float* __restrict__ srow, int key, int S, float (&raw)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int k0 = key + 8 * g;
        if (VEC) {
            const float4 v = *(const float4*)(srow + min(k0, S - 4));
            raw[4 * g] = v.x; raw[4 * g + 1] = v.y; raw[4 * g + 2] = v.z; raw[4 * g + 3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[4 * g + j] = srow[min(k0 + j, S - 1)];
        }
    }
}
// the A fragment of k-step s from those values: bf16 (nearest even), zero for rows >= n_tok and keys >= S
__device__ __forceinline__ sp_frag sp_src_frag(const float (&raw)[16], int s, int key, int S, bool tok_ok) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = tok_ok && key + 16 * s + 8 * (j >> 2) + (j & 3) < S ? raw[8 * s + j] : 0.f;
    const sp_u32x4 v = {pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7])};
    return __builtin_bit_cast(sp_frag, v);
}

// the operands of the 32-key tile starting at key0: K rows (lane c: key key0 + c, its half of the 4 k-steps) and the raw src values
template <bool VEC>
__device__ __forceinline__ void sp_load_tile(const bf16_t* __restrict__ kh, int64_t ldk, const float* __restrict__ srow, int key0, int S, int c, int hf,
                                             sp_frag (&ak)[4], float (&raw)[16]) {
    const bf16_t* kr = kh + (int64_t)min(key0 + c, S - 1) * ldk;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ak[ks] = sp_load8(kr + ks * 16);
    sp_load_src<VEC>(srow, key0 + 4 * hf, S, raw);
}

template <bool VEC>
__global__ __launch_bounds__(SP_QT * 2 * SP_WAVES) void sattn_propagate_kernel(
        const bf16_t* __restrict__ Q, int64_t ldq, int64_t strideQ, const bf16_t* __restrict__ K, int64_t ldk, int64_t strideK,
        const float* __restrict__ src, float* __restrict__ dst, int H, int S, int row0, int row_step, int n_tok, int accumulate,
        float scale_log2, float out_scale) {
    __shared__ float part[SP_WAVES][SP_MAXTOK][SP_QT];
    const int i = blockIdx.y;                                   // selected row
    const int64_t b = (int64_t)row0 + (int64_t)i * row_step;    // batch row
    const int s0 = blockIdx.x * SP_QT;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 31, hf = lane >> 5;                    // query column of the tile (first product) / token row (second), lane half
    const bool qok = s0 + c < S;
    const bf16_t* qrow = Q + b * strideQ + (int64_t)(qok ? s0 + c : 0) * ldq + hf * 8;
    const bf16_t* kbase = K + b * strideK + hf * 8;
    const bool tok_ok = c < n_tok;
    const float* srow = src + ((int64_t)i * n_tok + (tok_ok ? c : 0)) * S;
    const int nkt = (S + SP_KT - 1) / SP_KT;

    f32x16 tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.f;

    for (int h = w; h < H; h += SP_WAVES) {
        sp_frag bq[4];                                          // B[k = 8 hf + j][col c] = Q[c][16 ks + 8 hf + j], kept for the whole head
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bq[ks] = sp_load8(qrow + h * 64 + ks * 16);
        const bf16_t* kh = kbase + h * 64;
        sp_frag ak[4];                                          // the current tile: K as A[row key][k] ...
        float raw[16];                                          // ... and the src values of its two A fragments of the second product
        sp_load_tile<VEC>(kh, ldk, srow, 0, S, c, hf, ak, raw);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float m = -INFINITY, l = 0.f;                           // running max (both halves agree), this lane half's share of the sum

        for (int kt = 0; kt < nkt; ++kt) {
            const int key0 = kt * SP_KT;
            // this tile's src fragments from the values loaded during the last tile, then the next tile's operands, requested a whole tile ahead
            // (behind the last tile: row S - 1 and the last keys once more, unused)
            const sp_frag a0 = sp_src_frag(raw, 0, key0 + 4 * hf, S, tok_ok), a1 = sp_src_frag(raw, 1, key0 + 4 * hf, S, tok_ok);
            sp_frag an[4];
            sp_load_tile<VEC>(kh, ldk, srow, key0 + SP_KT, S, c, hf, an, raw);

            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak[ks], bq[ks], sc, 0, 0, 0);
            // sc[r]: key key0 + (r & 3) + 8 (r >> 2) + 4 hf of query c, unscaled; keys >= S become -inf (exp2 -> 0)
            const int lim = S - key0 - 4 * hf;
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[r] = (r & 3) + 8 * (r >> 2) < lim ? sc[r] * scale_log2 : -INFINITY;
                mt = fmaxf(mt, sc[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m, mt);                      // finite: key key0 of every tile is a real key
            const float alpha = __builtin_amdgcn_exp2f(m - mn);    // 0 at the first tile (m = -inf)
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[r] = __builtin_amdgcn_exp2f(sc[r] - mn);
                ls += sc[r];                                    // the fp32 exponentials: the sum is not the rounded operand's
            }
            l = l * alpha + ls;
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= alpha;
            const sp_u32x4 p0 = {pack_bf2(sc[0], sc[1]), pack_bf2(sc[2], sc[3]), pack_bf2(sc[4], sc[5]), pack_bf2(sc[6], sc[7])};
            const sp_u32x4 p1 = {pack_bf2(sc[8], sc[9]), pack_bf2(sc[10], sc[11]), pack_bf2(sc[12], sc[13]), pack_bf2(sc[14], sc[15])};
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, __builtin_bit_cast(sp_frag, p0), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, __builtin_bit_cast(sp_frag, p1), acc, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) ak[ks] = an[ks];
        }
        l = l + __shfl_xor(l, 32);                              // the same sum in both halves (fp32 addition commutes)
        const float inv_l = 1.0f / l;
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] += acc[r] * inv_l;
    }
    // tot[r]: token (r & 3) + 8 (r >> 2) + 4 hf of query c
#pragma unroll
    for (int r = 0; r < 16; ++r) part[w][(r & 3) + 8 * (r >> 2) + 4 * hf][c] = tot[r];
    __syncthreads();
    const int q = threadIdx.x % SP_QT;
    for (int j = threadIdx.x / SP_QT; j < n_tok; j += 2 * SP_WAVES) {      // 512 threads = 16 tokens x 32 queries per round: one owner each
        if (s0 + q < S) {
            float v = part[0][j][q];
#pragma unroll
            for (int ww = 1; ww < SP_WAVES; ++ww) v += part[ww][j][q];
            v *= out_scale;
            float* o = dst + ((int64_t)i * n_tok + j) * S + s0 + q;
            *o = accumulate ? *o + v : v;
        }
    }
}

}  // namespace

extern "C" int tmix_sattn_propagate(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                                    const float* src, float* dst, int B, int H, int S, int row0, int row_step, int n_rows,
                                    int n_tok, int accumulate, float scale, float out_scale, void* stream) {
    if (!Q || !K || !src || !dst) TMIX_FAIL(TMIX_EINVAL, "sattn_propagate: null pointer");
    if (n_tok < 1 || n_tok > SP_MAXTOK) TMIX_FAIL(TMIX_EINVAL, "sattn_propagate: n_tok=%d (1..%d)", n_tok, SP_MAXTOK);
    if (B < 1 || H < 1 || S < 1) TMIX_FAIL(TMIX_ESHAPE, "sattn_propagate: B=%d H=%d S=%d (each >= 1)", B, H, S);
    if (n_rows < 1 || n_rows > 65535 || row0 < 0 || row_step < 1 || (int64_t)row0 + (int64_t)(n_rows - 1) * row_step >= B)
        TMIX_FAIL(TMIX_ESHAPE, "sattn_propagate: rows row0=%d row_step=%d n_rows=%d outside a batch of %d", row0, row_step, n_rows, B);
    if (ldq < (int64_t)H * 64 || ldk < (int64_t)H * 64 || strideQ < 0 || strideK < 0)
        TMIX_FAIL(TMIX_ESHAPE, "sattn_propagate: ldq=%lld ldk=%lld narrower than H*64=%d", (long long)ldq, (long long)ldk, H * 64);
    if ((((uintptr_t)Q) & 7) || (((uintptr_t)K) & 7) || (((uintptr_t)src) & 7) || (((uintptr_t)dst) & 7) || (ldq % 4) || (ldk % 4) ||
        (strideQ % 4) || (strideK % 4))
        TMIX_FAIL(TMIX_EALIGN, "sattn_propagate: pointers must be 8-byte aligned, ld / stride multiples of 4 elements");
    if (!(scale > 0.f) || scale > 1e30f) TMIX_FAIL(TMIX_EINVAL, "sattn_propagate: scale=%g (must be > 0)", (double)scale);
    if (!(out_scale == out_scale) || out_scale > 1e30f || out_scale < -1e30f) TMIX_FAIL(TMIX_EINVAL, "sattn_propagate: out_scale=%g", (double)out_scale);
    const uintptr_t bytes = (uintptr_t)n_rows * (uintptr_t)n_tok * (uintptr_t)S * sizeof(float);
    if ((uintptr_t)src < (uintptr_t)dst + bytes && (uintptr_t)dst < (uintptr_t)src + bytes)
        TMIX_FAIL(TMIX_EINVAL, "sattn_propagate: src and dst overlap (every output reads all of src)");
    const bool vec = (S % 4 == 0) && aligned16(src);            // 16-byte src loads (every run of 4 keys is aligned and wholly below S)
    const dim3 grid((unsigned)((S + SP_QT - 1) / SP_QT), (unsigned)n_rows);
    const auto kern = vec ? sattn_propagate_kernel<true> : sattn_propagate_kernel<false>;
    kern<<<grid, SP_QT * 2 * SP_WAVES, 0, (hipStream_t)stream>>>(
        (const bf16_t*)Q, ldq, strideQ, (const bf16_t*)K, ldk, strideK, src, dst, H, S, row0, row_step, n_tok, accumulate ? 1 : 0,
        scale * LOG2E, out_scale);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
