// lora_down.hip -- the LoRA down-projection of the low-rank form of the concept deltas: fills the 64 pad columns behind every row of a projection's
// A operand, so that the projection GEMM itself adds up(down(x)).  Entry point: tmix_lora_down.
//
// utils_lora.py:65-79,113-119 add `up(down(x))` of concept i to batch row i + 1 of every attention projection (model_lora.py:41-48,
// rank 4).  In the low-rank mode (UNetWeights(lora_mode="lowrank")) the projection runs ONCE on shared weights [W | U | 0] with
// K + 64 input columns: the 64 pad columns behind a row of A hold that row's down-projections -- the P = 4 x (projections fused in the
// GEMM) values of the row's OWN concept at columns K + set * P .., zeros elsewhere -- so the GEMM's last K-tile adds up(down(x)) and no
// merged per-concept weight copies exist.  This kernel fills the pad.  With a LayerNorm folded into the GEMM (ln != 0) the GEMM forms
// rstd * (acc - mean * colsum(W')) + bias with colsum over the first K columns only, so the pad must hold T / rstd where
// T = LN(x) D^T:  (x - mean) D'^T + (D beta) / rstd  with D' = D * gamma; mean / rstd are taken from the row itself (fp32, E[x^2] - mean^2,
// the same definition the GEMM's statistics use).
#include "common.h"

namespace {
// One workgroup = 16 rows of A, its four waves split K: per 32-wide k-step a wave issues v_mfma_f32_16x16x32_bf16 twice --
//   C1[i][j] += sum_k Dx[i][k] X[j][k]   Dx = the concept's P down rows, then one row of ones (row P: the row sum s1), zeros
//   C2[i][j] += sum_k X[i][k] X[j][k]    the Gram matrix of the 16 rows: its diagonal is the sum of squares s2 (exact: bf16 products, fp32 sums)
// -- both operands straight from global memory in MFMA layout (lane = (row, k-quarter): 16 bytes), no cross-lane reduction; the waves'
// partial tiles are added through LDS and wave 0 writes the 64 pad columns of its 16 rows.
template <int P>
__global__ void __launch_bounds__(256) lora_down_kernel(bf16_t* __restrict__ A, int64_t lda, int K, int64_t rows, const bf16_t* __restrict__ D,
                                                        const float* __restrict__ dcolsum, const float* __restrict__ dbias, float eps, int ln,
                                                        const int* __restrict__ sets, int64_t rows_per_set) {
    __shared__ float red[3][2][4][64];                      // waves 1-3: C1 / C2 partials, [reg][lane]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    // blocks of 16 rows never cross a concept boundary: block = (batch row bb, 16-row piece of its rows_per_set rows)
    const int bps = (int)((rows_per_set + 15) >> 4);
    const int64_t bb = blockIdx.x / bps, m0 = bb * rows_per_set + (int64_t)(blockIdx.x - bb * bps) * 16;
    const int64_t mend = (bb + 1) * rows_per_set;           // (rows == batch rows x rows_per_set)
    const int set = sets[bb];
    const int64_t mrow = m0 + j < mend ? m0 + j : mend - 1;
    const bf16_t* xr = A + mrow * lda + kq * 8;
    const bf16_t* dr = D + ((int64_t)set * P + (j < P ? j : 0)) * K + kq * 8;
    frag_ab ones;
#pragma unroll
    for (int k = 0; k < 8; ++k) ones[k] = (__bf16)1.0f;
    frag_ab zero;
#pragma unroll
    for (int k = 0; k < 8; ++k) zero[k] = (__bf16)0.0f;
    f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, c2 = c1;
    const int nks = K >> 5;                                  // 32-wide k-steps; wave w takes every fourth
    for (int ks = w; ks < nks; ks += 4) {
        const frag_ab x = *(const frag_ab*)(xr + ks * 32);
        frag_ab d = j < P ? *(const frag_ab*)(dr + ks * 32) : (j == P ? ones : zero);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d, x, c1, 0, 0, 0);      // lane (column j = data row, rows 4 kq + r = down row)
        c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, x, c2, 0, 0, 0);
    }
    if (w) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { red[w - 1][0][r][lane] = c1[r]; red[w - 1][1][r][lane] = c2[r]; }
    }
    __syncthreads();
    if (w) return;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { c1[r] += red[u][0][r][lane]; c2[r] += red[u][1][r][lane]; }
    // lane (j, kq) holds T[row j][4 kq + r]; s1 of row j sits in lane (j, P / 4) register P % 4, s2 (the Gram diagonal) in lane (j, j / 4) register j % 4
    float mean = 0.f, sd = 1.f;
    if (ln) {
        const float s1c = c1[P & 3];
        const float s2c = (j & 3) == 0 ? c2[0] : (j & 3) == 1 ? c2[1] : (j & 3) == 2 ? c2[2] : c2[3];
        const float s1 = __shfl(s1c, j + 16 * (P >> 2)), s2 = __shfl(s2c, j + 16 * (j >> 2));
        mean = s1 / (float)K;
        sd = sqrtf(fmaxf(s2 / (float)K - mean * mean, 0.f) + eps);            // 1 / rstd
    }
    if (m0 + j >= mend) return;
    // this lane's 4 values go to pad columns set * P + 4 kq .. (when 4 kq < P); every other group of 4 pad columns of the row gets zeros
    bf16_t* prow = A + (m0 + j) * lda + K;
    uint2 v = make_uint2(0u, 0u);
    if (4 * kq < P) {
        float t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 4 * kq + r;
            t[r] = ln ? c1[r] - mean * dcolsum[set * P + q] + dbias[set * P + q] * sd : c1[r];
        }
        v = make_uint2(pack_bf2(t[0], t[1]), pack_bf2(t[2], t[3]));
    }
    // 16 groups of 4 columns per row, 4 lanes (kq) per row: lane kq writes groups kq, kq + 4, kq + 8, kq + 12 -- its own values at group
    // (set * P) / 4 + kq' where kq' < P / 4 ... handled by value: group g holds values iff set * P / 4 <= g < (set * P + P) / 4
    const int g0 = (set * P) >> 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = kq + 4 * u;                            // this lane writes group g; the values for it live in lane kq' = g - g0 of this row
        const int src = g - g0;
        const bool has = src >= 0 && 4 * src < P;
        const unsigned vx = __shfl(v.x, j + 16 * (has ? src : 0)), vy = __shfl(v.y, j + 16 * (has ? src : 0));
        *(uint2*)(prow + 4 * g) = has ? make_uint2(vx, vy) : make_uint2(0u, 0u);
    }
}
}  // namespace

extern "C" int tmix_lora_down(void* A, int64_t lda, int K, int64_t rows, const void* D, int P, int nsets, const float* dcolsum,
                              const float* dbias, float eps, const int* sets, int64_t rows_per_set, void* stream) {
    if (!A || !D || !sets) TMIX_FAIL(TMIX_EINVAL, "lora_down: null pointer");
    if (rows <= 0 || K <= 0 || (K % 8) || lda < K + 64 || (lda % 8)) TMIX_FAIL(TMIX_ESHAPE, "lora_down: rows=%lld K=%d lda=%lld (rows carry 64 pad columns behind their K values)", (long long)rows, K, (long long)lda);
    if ((P != 4 && P != 12) || nsets < 1 || nsets * P > 64) TMIX_FAIL(TMIX_ESHAPE, "lora_down: P=%d (4 or 12) x nsets=%d must fit the 64 pad columns", P, nsets);
    if ((dcolsum == nullptr) != (dbias == nullptr)) TMIX_FAIL(TMIX_EINVAL, "lora_down: the folded-LayerNorm form needs dcolsum and dbias");
    if (!aligned16(A) || !aligned16(D)) TMIX_FAIL(TMIX_EALIGN, "lora_down: A / D must be 16-byte aligned");
    const int ln = dcolsum != nullptr;
    if (rows_per_set <= 0 || (rows % rows_per_set) || (K % 32)) TMIX_FAIL(TMIX_ESHAPE, "lora_down: rows=%lld must be a multiple of rows_per_set=%lld and K=%d of 32", (long long)rows, (long long)rows_per_set, K);
    const unsigned grid = (unsigned)((rows / rows_per_set) * ((rows_per_set + 15) / 16));
    if (P == 12) lora_down_kernel<12><<<grid, 256, 0, (hipStream_t)stream>>>((bf16_t*)A, lda, K, rows, (const bf16_t*)D, dcolsum, dbias, eps, ln, sets, rows_per_set);
    else lora_down_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>((bf16_t*)A, lda, K, rows, (const bf16_t*)D, dcolsum, dbias, eps, ln, sets, rows_per_set);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
