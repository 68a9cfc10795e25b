// groupnorm.hip -- GroupNorm (+ SiLU) on NHWC bf16 tensors of one or two channel-concatenated sources, and nothing else.  Four forms:
//   three launches   gn_stats_kernel (per-chunk partial sums) -> gn_finalize_kernel (scale / shift per channel) -> gn_apply_kernel<0>
//   one launch       gn_small_kernel: small images, one workgroup per (image, a few groups)
//   from partials    gn_finalize_cs_kernel reads the column partials the tensor's producers wrote -> gn_apply_kernel<0>
//   ... as e4m3      the same with gn_apply_kernel<1>: e4m3 bytes + one E8M0 scale per (pixel, 32 channels)
// One accumulate loop (gn_accum8) and one apply body (gn_affine8) serve all of them.  Entry points: tmix_groupnorm_nhwc, tmix_groupnorm_nhwc_pre,
// tmix_groupnorm_nhwc_pre_f8 and the queries tmix_groupnorm_ws_chunks / _ws_floats / tmix_groupnorm_nhwc_launches.  All bf16 traffic is 16 bytes per lane.
#include "common.h"

namespace {

constexpr int GN_MAX_C = 4096;
constexpr int GN_T = 128;                // statistics workgroups per image, at most
constexpr int GN_APPLY_U = 2;            // loads in flight per thread of the apply pass
constexpr int GN_APPLY_ITEMS = 1024;     // 16-byte vectors per apply workgroup ...
constexpr int GN_APPLY_MAXB = 4096;      // ... up to this many workgroups per image

// statistics workgroups per image: up to GN_T, >= 8 pixels each.  A function of the image size ONLY, so the summation order
// -- and with it every output bit -- does not depend on how many images share the launch (co-batched seeds and row-split
// chains reproduce single runs exactly).  Measured (tools/gn_time.py): 32x32 maps want all 128 (18.1 -> 15.1 us against the
// former HW/32 rule); a 32-image video batch would prefer 16-32 per image (-17 %) but that would tie the result to the batch.
__host__ __device__ inline int gn_chunks(int64_t HW) {
    int64_t c = HW / 8;
    if (c > GN_T) c = GN_T;
    if (c < 1) c = 1;
    return (int)c;
}

// sums (a) and sums of squares (q) of 8 channels over rows r0, r0 + step, ... < r1 of src (ld elements per row): four rows in flight per thread
// (the loop is latency-bound), added in row order.  No fp32 sum runs over more than GN_CHAIN rows: before it would, a and q are flushed into fp64
// totals (A, Q) and start again from zero; what leaves is the fp64 total rounded ONCE to fp32.  var = E[x^2] - mean^2 loses (mean / std)^2 times
// the relative error of these sums, and a 512-row fp32 chain -- the VAE decoder's last level at 1024^2, HW * C / 262144 rows per thread of
// gn_stats_kernel -- cost a group at mean / std = 30 three times the error budget of the whole norm (tests/test_norm_numerics_gpu.py).  A run of
// at most GN_CHAIN rows never flushes and leaves exactly the fp32 sums it always did (0.0 + a == a).  FLUSH = false: the caller's runs are no
// longer than GN_CHAIN (gn_small_kernel, by gn_small_gpw; the fp64 totals would cost it 31 VGPRs and three of its seven waves per SIMD).
// I = the caller's row index type: an image of the one-launch form has few rows, and 64-bit row cursors cost that kernel 12 VGPRs.
constexpr int GN_CHAIN = 32;
template <typename I, bool FLUSH>
__device__ __forceinline__ void gn_accum8(const bf16_t* __restrict__ src, int ld, I r0, int step, I r1, float (&a)[8], float (&q)[8]) {
    double A[8] = {0, 0, 0, 0, 0, 0, 0, 0}, Q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n = 0;                                            // rows in a and q since the last flush
    auto count = [&](int rows) {
        if constexpr (FLUSH) {
            if (n + rows > GN_CHAIN) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { A[j] += (double)a[j]; Q[j] += (double)q[j]; a[j] = 0.f; q[j] = 0.f; }
                n = 0;
            }
            n += rows;
        }
    };
    I r = r0;
    for (; r + 3 * step < r1; r += 4 * step) {
        count(4);
        uint4 raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = *(const uint4*)(src + (int64_t)(r + u * step) * ld);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float f[8]; unpack8(raw[u], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] += f[j]; q[j] += f[j] * f[j]; }
        }
    }
    for (; r < r1; r += step) {
        count(1);
        float f[8]; unpack8(*(const uint4*)(src + (int64_t)r * ld), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] += f[j]; q[j] += f[j] * f[j]; }
    }
    if constexpr (FLUSH) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = (float)(A[j] + (double)a[j]); q[j] = (float)(Q[j] + (double)q[j]); }
    }
}

// y = x * scale + shift (+ SiLU) of 8 values; k = the {scale, shift} pairs of their channels
__device__ __forceinline__ void gn_affine8(float (&f)[8], const float2* k, int silu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float y = f[j] * k[j].x + k[j].y;
        if (silu) y = silu_fast(y);
        f[j] = y;
    }
}

// partial sums per (batch, chunk of pixels, group): ws[((b*chunks + ch)*groups + g)*2 + {0,1}]
__global__ void __launch_bounds__(256) gn_stats_kernel(const bf16_t* __restrict__ X1, int C1, const bf16_t* __restrict__ X2, int C2,
                                                       float* __restrict__ ws, int64_t HW, int groups, int chunks,
                                                       unsigned long long* prof) {
    __shared__ float s_sum[GN_MAX_C], s_sq[GN_MAX_C];
    if (prof && threadIdx.x == 0) prof_enter(prof, (blockIdx.x | blockIdx.y) == 0, 0);   // in-situ timing (common.h): the norm's three launches share a slot
    const int C = C1 + C2, nvec = C >> 3, cpg = C / groups;
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int64_t ppc = (HW + chunks - 1) / chunks;
    const int64_t p0 = (int64_t)ch * ppc;
    int64_t p1 = p0 + ppc; if (p1 > HW) p1 = HW;
    // fixed vector column per thread so the 8 per-channel sums stay in registers across pixels;
    // partials land in LDS at [pixel lane][channel] and are reduced in a fixed order (deterministic), in fp64: plane * cpg terms, 60 at 320 channels.
    const int plane = nvec <= 256 ? 256 / nvec : 1;          // pixel lanes per block; plane * C <= 2048
    for (int v0 = 0; v0 < nvec; v0 += 256) {
        const int v = v0 + (nvec <= 256 ? tid % nvec : tid);
        const int pl = nvec <= 256 ? tid / nvec : 0;
        if (v < nvec && pl < plane) {
            float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int c0 = v * 8;
            const bf16_t* src; int cs;
            if (c0 < C1) { src = X1 + (int64_t)b * HW * C1 + c0; cs = C1; }
            else         { src = X2 + (int64_t)b * HW * C2 + (c0 - C1); cs = C2; }
            gn_accum8<int64_t, true>(src, cs, p0 + pl, plane, p1, a, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) { s_sum[pl * C + c0 + j] = a[j]; s_sq[pl * C + c0 + j] = q[j]; }
        }
    }
    __syncthreads();
    if (tid < groups) {
        double s = 0.0, q = 0.0;
        for (int pl = 0; pl < plane; ++pl)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { s += (double)s_sum[pl * C + c]; q += (double)s_sq[pl * C + c]; }
        float* o = ws + (((int64_t)b * chunks + ch) * groups + tid) * 2;
        o[0] = (float)s; o[1] = (float)q;
    }
}

// combine the per-chunk partials (fp64) and fold gamma/beta: ss[b][c] = {scale, shift} with
// y = x*scale + shift.  One tiny launch instead of redoing this in every apply workgroup.
__global__ void __launch_bounds__(64) gn_finalize_kernel(const float* __restrict__ ws, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float2* __restrict__ ss,
                                                         int C, int64_t HW, int groups, int chunks, float eps) {
    // one wave per (group, batch): lanes split the chunks, fp64 tree-combine, then write the group's channels
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, cpg = C / groups;
    double s = 0.0, q = 0.0;
    for (int ch = lane; ch < chunks; ch += 64) {
        const float* o = ws + (((int64_t)b * chunks + ch) * groups + g) * 2;
        s += (double)o[0]; q += (double)o[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
    const double n = (double)HW * cpg;
    const double mean = s / n;
    double var = q / n - mean * mean; if (var < 0.0) var = 0.0;
    const float meanf = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)eps));
    for (int c = g * cpg + lane; c < (g + 1) * cpg; c += 64) {
        const float sc = rstd * gamma[c];
        ss[(int64_t)b * C + c] = make_float2(sc, beta[c] - meanf * sc);
    }
}

// the same from the column partials the tensor's PRODUCERS wrote (tmix_gemm_desc.col_stats_out: [B*HW/32][2][Cs] per source): one
// workgroup of 16 waves per (group, image) adds the group's channels over the image's 32-row blocks -- thread (j, c) walks blocks j, j + J, ...
// of channel c (a fixed order; up to 512 blocks x 80 channels x 2 planes at the 128 x 128 level, where four waves were latency-bound:
// 80 us for the whole norm against 67 with the statistics kernel) in fp32, threads combine in fp64 -- and folds gamma / beta.
// No pass over X: the statistics launch of the three is gone.
constexpr int GN_CS_T = 1024;
__device__ __forceinline__ void gn_cs_walk(const float* __restrict__ base, int Cs, int n, int nblk, int tid, float& s, float& q) {
    if (n <= 0) return;
    const int J = GN_CS_T / n, j = tid / n, c = tid - j * n;       // J >= 4: n <= 256
    if (j >= J) return;
    const float* row = base + (int64_t)j * 2 * Cs + c;
    const int64_t step = (int64_t)J * 2 * Cs;
    int blk = j;
    for (; blk + 3 * J < nblk; blk += 4 * J, row += 4 * step) {     // four blocks in flight per thread
        const float a0 = row[0], b0 = row[Cs], a1 = row[step], b1 = row[step + Cs];
        const float a2 = row[2 * step], b2 = row[2 * step + Cs], a3 = row[3 * step], b3 = row[3 * step + Cs];
        s += (a0 + a1) + (a2 + a3); q += (b0 + b1) + (b2 + b3);
    }
    for (; blk < nblk; blk += J, row += step) { s += row[0]; q += row[Cs]; }
}
__global__ void __launch_bounds__(GN_CS_T) gn_finalize_cs_kernel(const float* __restrict__ cs1, int C1, const float* __restrict__ cs2, int C2,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float2* __restrict__ ss, int64_t HW, int groups, float eps,
                                                                 unsigned long long* prof) {
    __shared__ double s_red[2 * GN_CS_T / 64];
    __shared__ float s_ms[2];
    if (prof && threadIdx.x == 0) prof_enter(prof, (blockIdx.x | blockIdx.y) == 0, 0);
    const int C = C1 + C2, cpg = C / groups;
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nblk = (int)(HW / 32);
    // gamma / beta of the channel this thread will write: requested before the reduction, whose result they do not depend on
    float gm = 0.f, bt = 0.f;
    if (tid < cpg) { gm = gamma[g * cpg + tid]; bt = beta[g * cpg + tid]; }
    // the group's channels that live in source 1 / source 2 (a group may straddle the two)
    const int c_lo = g * cpg, c_hi = c_lo + cpg;
    const int n1 = min(c_hi, C1) - min(c_lo, C1), n2 = cpg - n1;
    float s = 0.f, q = 0.f;
    gn_cs_walk(cs1 + (int64_t)b * nblk * 2 * C1 + c_lo, C1, n1, nblk, tid, s, q);
    if (n2 > 0) gn_cs_walk(cs2 + (int64_t)b * nblk * 2 * C2 + (max(c_lo, C1) - C1), C2, n2, nblk, tid, s, q);
    double sd = (double)s, qd = (double)q;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sd += __shfl_xor(sd, o); qd += __shfl_xor(qd, o); }
    if ((tid & 63) == 0) { s_red[(tid >> 6) * 2] = sd; s_red[(tid >> 6) * 2 + 1] = qd; }
    __syncthreads();
    if (tid == 0) {
        double st = 0.0, qt = 0.0;
#pragma unroll
        for (int w = 0; w < GN_CS_T / 64; ++w) { st += s_red[2 * w]; qt += s_red[2 * w + 1]; }
        const double n = (double)HW * cpg;
        const double mean = st / n;
        double var = qt / n - mean * mean; if (var < 0.0) var = 0.0;
        s_ms[0] = (float)mean; s_ms[1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    if (tid < cpg) {
        const float sc = s_ms[1] * gm;
        ss[(int64_t)b * C + c_lo + tid] = make_float2(sc, bt - s_ms[0] * sc);
    }
}

// F8 = 1 (tmix_groupnorm_nhwc_pre_f8): the normalised (+ SiLU) tensor leaves as OCP e4m3 bytes [B*HW][C] with one E8M0 scale per (pixel, 32 channels) in the
// ROW-major form [B*HW][C / 32] -- the input of tmix_conv3x3_nhwc_fp8 (a tap shift moves a pixel's scales by a multiple of 4 bytes) -- exactly what an MX
// quantiser makes of the bf16 tensor the plain kernel writes.  Work items are dealt out in multiples of four vectors so that a quad of lanes holds one block.
template <int F8>
__global__ void __launch_bounds__(256) gn_apply_kernel(const bf16_t* __restrict__ X1, int C1, const bf16_t* __restrict__ X2, int C2,
                                                       bf16_t* __restrict__ Y, const float2* __restrict__ ss, int64_t HW, int silu,
                                                       unsigned long long* prof, unsigned char* __restrict__ Y8 = nullptr, unsigned char* __restrict__ S8 = nullptr) {
    __shared__ float2 s_ss[GN_MAX_C];
    const unsigned long long pt0 = (prof && threadIdx.x == 0) ? prof_now() : 0;
    const int C = C1 + C2, nvec = C >> 3;
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) s_ss[c] = ss[(int64_t)b * C + c];
    __syncthreads();
    const int64_t total = HW * nvec;
    int64_t per = (total + gridDim.x - 1) / gridDim.x;
    if (F8) per = (per + 3) & ~(int64_t)3;
    const int64_t i0 = (int64_t)blockIdx.x * per;
    int64_t i1 = i0 + per; if (i1 > total) i1 = total;
    int64_t p = i0 / nvec; int v = (int)(i0 - p * nvec) + tid;      // running (pixel, vector) cursor: no 64-bit division per item
    while (v >= nvec) { v -= nvec; ++p; }
    const int step_p = 256 / nvec, step_v = 256 - step_p * nvec;
    constexpr int U = GN_APPLY_U;                        // loads in flight per thread (the pass is latency-bound)
    for (int64_t i = i0 + tid; i < i1; i += 256 * U) {
        uint4 raw[U]; int64_t pp[U]; int cc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pp[u] = p; cc[u] = v * 8;
            if (i + u * 256 < i1) {
                const bf16_t* src = (cc[u] < C1) ? X1 + ((int64_t)b * HW + p) * C1 + cc[u] : X2 + ((int64_t)b * HW + p) * C2 + (cc[u] - C1);
                raw[u] = *(const uint4*)src;
            }
            p += step_p; v += step_v;
            if (v >= nvec) { v -= nvec; ++p; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u * 256 < i1) {
                float f[8]; unpack8(raw[u], f);
                gn_affine8(f, s_ss + cc[u], silu);
                if constexpr (F8) {
                    const uint4 pk = pack8(f);
                    unpack8(pk, f);                       // the bf16-rounded values
                    float am = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(f[j]));
                    const MxPacked mx = mx_pack8(f, quad_max(am));          // the MX block is the 4 adjacent 8-channel vectors of a pixel
                    const int64_t row = (int64_t)b * HW + pp[u];
                    *(uint2*)(Y8 + row * C + cc[u]) = make_uint2(mx.lo, mx.hi);
                    if ((tid & 3) == 0) S8[row * (C >> 5) + (cc[u] >> 5)] = (unsigned char)(mx.e + 127);
                } else
                *(uint4*)(Y + ((int64_t)b * HW + pp[u]) * C + cc[u]) = pack8(f);
            }
        }
    }
    if (prof && threadIdx.x == 0) prof_leave(prof, 0, pt0, pt0, pt0);
}

// GroupNorm (+ SiLU) of a SMALL image in ONE launch (tmix_groupnorm_nhwc picks it by shape): one workgroup owns gpw consecutive groups of one image -- cw = gpw * C / groups
// channels, a multiple of 8 -- reads its HW x cw slice twice (statistics, then apply: <= 128 KB, it stays in L2) and needs nobody else's sums.  The three-launch form costs a
// 336-pixel frame of the video UNet's third level 10 + 5 + 10 us and two kernel boundaries; the slices here are 27 - 80 KB.  Thread t keeps vector t % nv of rows t / nv,
// + rs, ...; the sums meet in LDS and are added in a fixed order (channel sums over row slots, then group sums over channels, both in fp64): every output bit is a function
// of the image alone, as with the other forms.
constexpr int GN_SMALL_MAX_CW = 256, GN_SMALL_MAX_ELEMS = 65536;
__global__ void __launch_bounds__(256) gn_small_kernel(const bf16_t* __restrict__ X1, int C1, const bf16_t* __restrict__ X2, int C2, bf16_t* __restrict__ Y,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, int HW, int groups, int gpw, float eps, int silu,
                                                       unsigned long long* prof) {
    __shared__ float r_s[2048], r_q[2048];
    __shared__ double c_s[GN_SMALL_MAX_CW], c_q[GN_SMALL_MAX_CW];
    __shared__ float g_ms[16];
    __shared__ float2 s_ss[GN_SMALL_MAX_CW];
    const unsigned long long pt0 = (prof && threadIdx.x == 0) ? prof_enter(prof, (blockIdx.x | blockIdx.y) == 0, 0) : 0;      // (the one launch writes both stamps of its slot)
    const int C = C1 + C2, cpg = C / groups, cw = gpw * cpg, nv = cw >> 3, rs = 256 / nv;
    const int b = blockIdx.y, c0 = blockIdx.x * cw, tid = threadIdx.x;
    const int v = tid % nv, slot = tid / nv;
    const bool active = slot < rs;
    const int cg = c0 + v * 8;
    const bf16_t* src; int ld;
    if (cg < C1) { src = X1 + (int64_t)b * HW * C1 + cg; ld = C1; } else { src = X2 + (int64_t)b * HW * C2 + (cg - C1); ld = C2; }
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (active) {
        gn_accum8<int, false>(src, ld, slot, rs, HW, s, q);        // <= GN_CHAIN rows: gn_small_gpw
#pragma unroll
        for (int j = 0; j < 8; ++j) { r_s[slot * cw + v * 8 + j] = s[j]; r_q[slot * cw + v * 8 + j] = q[j]; }
    }
    __syncthreads();
    if (tid < cw) {
        double a = 0.0, d = 0.0;
        for (int k = 0; k < rs; ++k) { a += (double)r_s[k * cw + tid]; d += (double)r_q[k * cw + tid]; }
        c_s[tid] = a; c_q[tid] = d;
    }
    __syncthreads();
    if (tid < gpw) {
        double a = 0.0, d = 0.0;
        for (int k = 0; k < cpg; ++k) { a += c_s[tid * cpg + k]; d += c_q[tid * cpg + k]; }
        const double n = (double)HW * cpg, mean = a / n;
        double var = d / n - mean * mean; if (var < 0.0) var = 0.0;
        g_ms[2 * tid] = (float)mean; g_ms[2 * tid + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    if (tid < cw) {
        const int g = tid / cpg;
        const float sc = g_ms[2 * g + 1] * gamma[c0 + tid];
        s_ss[tid] = make_float2(sc, beta[c0 + tid] - g_ms[2 * g] * sc);
    }
    __syncthreads();
    if (active) {
        float2 k[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = s_ss[v * 8 + j];
        bf16_t* dst = Y + (int64_t)b * HW * C + cg;
        int row = slot;
        for (; row + 3 * rs < HW; row += 4 * rs) {
            uint4 raw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) raw[u] = *(const uint4*)(src + (int64_t)(row + u * rs) * ld);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float f[8]; unpack8(raw[u], f);
                gn_affine8(f, k, silu);
                *(uint4*)(dst + (int64_t)(row + u * rs) * C) = pack8(f);
            }
        }
        for (; row < HW; row += rs) {
            float f[8]; unpack8(*(const uint4*)(src + (int64_t)row * ld), f);
            gn_affine8(f, k, silu);
            *(uint4*)(dst + (int64_t)row * C) = pack8(f);
        }
    }
    if (prof && threadIdx.x == 0) prof_leave(prof, 0, pt0, pt0, pt0);
}
// gpw for the one-launch form, or 0 when the shape does not qualify (the slice must be small).  A function of the image's shape ONLY -- not of the batch: co-batched seeds
// and row-split chains must take the same path as a single run to reproduce it bit for bit.
int gn_small_gpw(int64_t HW, int C, int groups) {
    if (tmix_env(TMIX_ENV_GN_NO_SMALL)) return 0;
    const int cpg = C / groups;
    for (int gpw = 1; gpw <= 8; gpw <<= 1) {
        if (groups % gpw || ((gpw * cpg) & 7)) continue;
        const int cw = gpw * cpg;
        if (cw > GN_SMALL_MAX_CW || HW * cw > GN_SMALL_MAX_ELEMS) return 0;
        const int rs = 256 / (cw >> 3);                   // row slots of gn_small_kernel: a thread adds every rs-th row in fp32
        if ((HW + rs - 1) / rs > GN_CHAIN) return 0;      // (36 at most under the limits above, and only at pixel counts such as 1633 .. 1638 x 40 channels)
        return gpw;
    }
    return 0;
}

// ws layout: [B * GN_T * groups * 2] partial sums (room for the most chunks an image can have) | [B * C] float2 scale / shift
int64_t gn_ws_partial_floats(int B, int groups) { return (int64_t)B * GN_T * groups * 2; }
// workgroups per image of the apply pass
unsigned gn_apply_blocks(int64_t HW, int C) {
    int64_t nb = (HW * (C / 8) + GN_APPLY_ITEMS - 1) / GN_APPLY_ITEMS; if (nb < 1) nb = 1; if (nb > GN_APPLY_MAXB) nb = GN_APPLY_MAXB;
    return (unsigned)nb;
}

// the argument checks every entry shares; `name` is the entry's prefix in the messages
int gn_check(const char* name, const void* X1, int C1, const void* X2, int C2, const void* Y, const float* gamma, const float* beta, const float* ws,
             int B, int64_t HW, int groups) {
    if (!X1 || !Y || !gamma || !beta || !ws) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", name);
    if (C2 > 0 && !X2) TMIX_FAIL(TMIX_EINVAL, "%s: C2 > 0 but X2 is null", name);
    const int C = C1 + C2;
    if (B <= 0 || HW <= 0 || C <= 0) TMIX_FAIL(TMIX_ESHAPE, "%s: empty problem", name);
    if ((C1 % 8) || (C2 % 8) || C > GN_MAX_C || groups <= 0 || groups > 64 || (C % groups)) TMIX_FAIL(TMIX_ESHAPE, "%s: C1=%d C2=%d groups=%d unsupported", name, C1, C2, groups);
    if (!aligned16(X1) || (X2 && !aligned16(X2)) || !aligned16(Y)) TMIX_FAIL(TMIX_EALIGN, "%s: pointers must be 16-byte aligned", name);
    return TMIX_OK;
}

// tmix_groupnorm_nhwc_pre (S8 == nullptr) and tmix_groupnorm_nhwc_pre_f8
int gn_pre_entry(const void* X1, int C1, const void* X2, int C2, void* Y, void* S8, const float* gamma,
                 const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                 const float* cs1, int cs1_channels, const float* cs2, int cs2_channels, void* stream) {
    if (!cs1) TMIX_FAIL(TMIX_EINVAL, "groupnorm_pre: null pointer");
    if (const int rc = gn_check("groupnorm_pre", X1, C1, X2, C2, Y, gamma, beta, ws, B, HW, groups)) return rc;
    const int C = C1 + C2;
    // gn_finalize_cs_kernel: reads source i's partials with cs<i>_channels as their row length
    if (cs1_channels <= 0 || cs2_channels < 0 || cs1_channels + cs2_channels != C || (cs2_channels > 0 && !cs2))
        TMIX_FAIL(TMIX_EINVAL, "groupnorm_pre: the partials cover %d + %d channels, the tensor has %d", cs1_channels, cs2_channels, C);
    // gn_finalize_cs_kernel: one thread per channel of the group writes scale / shift, and gn_cs_walk deals its 1024 threads out over at most 256 channels
    if (C / groups > 256) TMIX_FAIL(TMIX_ESHAPE, "groupnorm_pre: C1=%d C2=%d groups=%d unsupported", C1, C2, groups);
    // gn_finalize_cs_kernel: walks whole 32-row blocks of partials
    if (HW % TMIX_COLSTATS_ROWS) TMIX_FAIL(TMIX_ESHAPE, "groupnorm_pre: HW=%lld must be a multiple of %d (the producers' partials cover 32-row blocks)", (long long)HW, TMIX_COLSTATS_ROWS);
    // gn_apply_kernel<1>: a quad of lanes holds one 32-channel block of one pixel
    if (S8 && (C % 32)) TMIX_FAIL(TMIX_ESHAPE, "groupnorm_pre_f8: C must be a multiple of 32 (MX blocks)");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* prof = tmix_prof_take();
    float2* ss = (float2*)(ws + gn_ws_partial_floats(B, groups));
    gn_finalize_cs_kernel<<<dim3(groups, B), GN_CS_T, 0, st>>>(cs1, cs1_channels, cs2, cs2_channels, gamma, beta, ss, HW, groups, eps, prof);
    TMIX_LAUNCH_CHECK();
    const dim3 grid(gn_apply_blocks(HW, C), B);
    if (S8) gn_apply_kernel<1><<<grid, 256, 0, st>>>((const bf16_t*)X1, C1, (const bf16_t*)X2, C2, nullptr, ss, HW, silu, prof, (unsigned char*)Y, (unsigned char*)S8);
    else gn_apply_kernel<0><<<grid, 256, 0, st>>>((const bf16_t*)X1, C1, (const bf16_t*)X2, C2, (bf16_t*)Y, ss, HW, silu, prof);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

}  // namespace

extern "C" int tmix_groupnorm_ws_chunks(int64_t HW) { return gn_chunks(HW); }
extern "C" int64_t tmix_groupnorm_ws_floats(int B, int C, int groups) { return gn_ws_partial_floats(B, groups) + (int64_t)B * C * 2; }

extern "C" int tmix_groupnorm_nhwc_launches(int64_t HW, int C, int groups) {
    if (HW <= 0 || C <= 0 || groups <= 0 || (C % groups)) return 0;
    return gn_small_gpw(HW, C, groups) ? 1 : 3;
}

extern "C" int tmix_groupnorm_nhwc(const void* X1, int C1, const void* X2, int C2, void* Y, const float* gamma,
                                   const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                                   void* stream) {
    if (const int rc = gn_check("groupnorm", X1, C1, X2, C2, Y, gamma, beta, ws, B, HW, groups)) return rc;
    const int C = C1 + C2;
    const int chunks = gn_chunks(HW);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* prof = tmix_prof_take();
    if (const int gpw = gn_small_gpw(HW, C, groups)) {          // small images: statistics + apply in one launch, one workgroup per (image, gpw groups)
        gn_small_kernel<<<dim3(groups / gpw, B), 256, 0, st>>>((const bf16_t*)X1, C1, (const bf16_t*)X2, C2, (bf16_t*)Y, gamma, beta, (int)HW, groups, gpw, eps, silu, prof);
        TMIX_LAUNCH_CHECK();
        return TMIX_OK;
    }
    gn_stats_kernel<<<dim3(chunks, B), 256, 0, st>>>((const bf16_t*)X1, C1, (const bf16_t*)X2, C2, ws, HW, groups, chunks, prof);
    TMIX_LAUNCH_CHECK();
    float2* ss = (float2*)(ws + gn_ws_partial_floats(B, groups));
    gn_finalize_kernel<<<dim3(groups, B), 64, 0, st>>>(ws, gamma, beta, ss, C, HW, groups, chunks, eps);
    TMIX_LAUNCH_CHECK();
    gn_apply_kernel<0><<<dim3(gn_apply_blocks(HW, C), B), 256, 0, st>>>((const bf16_t*)X1, C1, (const bf16_t*)X2, C2, (bf16_t*)Y, ss, HW, silu, prof);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_groupnorm_nhwc_pre(const void* X1, int C1, const void* X2, int C2, void* Y, const float* gamma,
                                       const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                                       const float* cs1, int cs1_channels, const float* cs2, int cs2_channels, void* stream) {
    return gn_pre_entry(X1, C1, X2, C2, Y, nullptr, gamma, beta, ws, B, HW, groups, eps, silu, cs1, cs1_channels, cs2, cs2_channels, stream);
}

extern "C" int tmix_groupnorm_nhwc_pre_f8(const void* X1, int C1, const void* X2, int C2, void* Y8, void* scales, const float* gamma,
                                          const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                                          const float* cs1, int cs1_channels, const float* cs2, int cs2_channels, void* stream) {
    if (!scales) TMIX_FAIL(TMIX_EINVAL, "groupnorm_pre_f8: null scale array");
    return gn_pre_entry(X1, C1, X2, C2, Y8, scales, gamma, beta, ws, B, HW, groups, eps, silu, cs1, cs1_channels, cs2, cs2_channels, stream);
}
