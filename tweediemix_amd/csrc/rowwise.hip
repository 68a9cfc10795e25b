// rowwise.hip -- the small row-wise and elementwise kernels of the forward passes, HBM- or latency-bound all: LayerNorm, the fp32 -> bf16 row softmax
// (plain, causal, masked), the fp8 row quantiser, channel concat, affine clamp, tmix_zero, the sinusoidal timestep embedding and the small-M linear
// of the time / add-embedding MLPs (plain and sections form).  Kernels first, their entry points below in the same order.
// All bf16 traffic is 16 bytes per lane.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------ LayerNorm
// one wave per row, row kept in registers (exact two-pass variance); C <= 2048, C % 8 == 0
__global__ void __launch_bounds__(256) layernorm_kernel(const bf16_t* __restrict__ X, bf16_t* __restrict__ Y,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = C >> 3;
    float f[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = i * 64 + lane;
        if (v < nvec) {
            const uint4 raw = *(const uint4*)(X + row * C + v * 8);
            unpack8(raw, f[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += f[i][j];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = i * 64 + lane;
        if (v < nvec) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = f[i][j] - mean; q += d * d; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = i * 64 + lane;
        if (v < nvec) {
            const float4 g0 = *(const float4*)(gamma + v * 8), g1 = *(const float4*)(gamma + v * 8 + 4);
            const float4 b0 = *(const float4*)(beta + v * 8), b1 = *(const float4*)(beta + v * 8 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = (f[i][j] - mean) * rstd * gg[j] + bb[j];
            *(uint4*)(Y + row * C + v * 8) = pack8(y);
        }
    }
}

// ------------------------------------------------------------------------------ row softmax (fp32 -> bf16)
// one workgroup per row; the row (<= 64K columns) is streamed three times from L2/HBM (max, sum, write).
// seq > 0: causal rows of a [.., seq, cols] score stack -- row r attends to columns <= r % seq, the rest get P = 0.
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* __restrict__ S, int64_t ld_s, bf16_t* __restrict__ P,
                                                           int64_t ld_p, int cols, float scale_log2e, int seq, int valid) {
    __shared__ float red[4];
    const float* row = S + (int64_t)blockIdx.x * ld_s;
    bf16_t* out = P + (int64_t)blockIdx.x * ld_p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lim = seq > 0 ? (int)(blockIdx.x % (unsigned)seq) + 1 : valid;    // visible columns: [0, lim)
    auto load = [&](int c) {
        float4 v = *(const float4*)(row + c);
        if (c + 0 >= lim) v.x = -INFINITY;
        if (c + 1 >= lim) v.y = -INFINITY;
        if (c + 2 >= lim) v.z = -INFINITY;
        if (c + 3 >= lim) v.w = -INFINITY;
        return v;
    };
    float mx = -INFINITY;
    for (int c = tid * 4; c < cols; c += 1024) {
        const float4 v = load(c);
        mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * scale_log2e;
    __syncthreads();
    float sum = 0.f;
    for (int c = tid * 4; c < cols; c += 1024) {
        const float4 v = load(c);
        sum += exp2f(v.x * scale_log2e - mx) + exp2f(v.y * scale_log2e - mx) + exp2f(v.z * scale_log2e - mx) + exp2f(v.w * scale_log2e - mx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) red[w] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
    for (int c = tid * 4; c < cols; c += 1024) {
        const float4 v = load(c);
        uint2 o;
        o.x = pack_bf2(exp2f(v.x * scale_log2e - mx) * inv, exp2f(v.y * scale_log2e - mx) * inv);
        o.y = pack_bf2(exp2f(v.z * scale_log2e - mx) * inv, exp2f(v.w * scale_log2e - mx) * inv);
        *(uint2*)(out + c) = o;
    }
}

// behind the three tmix_softmax_rows* entries, which differ in their name, in the rules for their own argument (form_ok; shape_fmt prints it: shape_arg)
// and in the (seq, valid) pair the kernel gets
int softmax_entry(const char* name, const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, float scale, int seq, int valid,
                  bool form_ok, const char* shape_fmt, int shape_arg, void* stream) {
    if (!S || !P) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", name);
    if (rows <= 0 || cols <= 0 || !form_ok || (cols % 4) || (ld_s % 4) || (ld_p % 4)) TMIX_FAIL(TMIX_ESHAPE, shape_fmt, name, (long long)rows, cols, shape_arg);
    if (!aligned16(S) || (((uintptr_t)P) & 7)) TMIX_FAIL(TMIX_EALIGN, "%s: pointer alignment", name);
    softmax_rows_kernel<<<(unsigned)rows, 256, 0, (hipStream_t)stream>>>(S, ld_s, (bf16_t*)P, ld_p, cols, scale * LOG2E, seq, valid);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// ------------------------------------------------------------------------------ fp8 row quantiser
// one wave per row: q[r][k] = e4m3(x[r][k] * 2^-(e_r - 127)) with e_r the smallest E8M0 exponent that brings the row's largest
// magnitude under 448 (the e4m3 maximum); an all-zero row gets e = 127 (scale 1).  The row stays in registers between the
// maximum and the conversion (one HBM read, K <= 8192).
__global__ void __launch_bounds__(256) quantize_fp8_rows_kernel(const bf16_t* __restrict__ X, int64_t ld, unsigned char* __restrict__ Q, int64_t ldq,
                                                                unsigned char* __restrict__ scale, int64_t rows, int K) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    constexpr int MAXV = 16;                                  // 16-byte vectors per lane: K <= 64 * 8 * 16 = 8192
    const int nv = K >> 3;
    uint4 v[MAXV];
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int c = u * 64 + lane;
        if (c < nv) {
            v[u] = *(const uint4*)(X + r * ld + (int64_t)c * 8);
            float f[8]; unpack8(v[u], f);
#pragma unroll
            for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(f[k]));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));        // the block is the whole row
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int c = u * 64 + lane;
        if (c < nv) {
            float f[8]; unpack8(v[u], f);
            const MxPacked mx = mx_pack8(f, amax);
            *(uint2*)(Q + r * ldq + (int64_t)c * 8) = make_uint2(mx.lo, mx.hi);
            if (c == 0) scale[r] = (unsigned char)(mx.e + 127);
        }
    }
}

// ------------------------------------------------------------------------------ concat
__global__ void __launch_bounds__(256) concat_kernel(const uint4* __restrict__ X1, int v1, const uint4* __restrict__ X2, int v2,
                                                     uint4* __restrict__ Y, int64_t rows) {
    const int nv = v1 + v2;
    const int64_t total = rows * nv;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / nv; const int v = (int)(i - r * nv);
        Y[i] = v < v1 ? X1[r * v1 + v] : X2[r * v2 + (v - v1)];
    }
}

__global__ void __launch_bounds__(256) affine_clamp_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                           float scale, float shift, float lo, float hi) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        y[i] = fminf(fmaxf(x[i] * scale + shift, lo), hi);
}

// ------------------------------------------------------------------------------ timestep embedding
__global__ void timestep_embedding_kernel(const float* __restrict__ values, float* __restrict__ out, int count, int dim) {
    const int half = dim >> 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * half) return;
    const int r = i / half, j = i - r * half;
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);     // ln(10000)
    const float a = values[r] * freq;
    out[(int64_t)r * dim + j] = cosf(a);                 // flip_sin_to_cos=True: [cos | sin]
    out[(int64_t)r * dim + half + j] = sinf(a);
}

// ------------------------------------------------------------------------------ small-M linear
// one wave per output column; the M (<=16) input rows are tiny and L1/L2 resident
template <int MAXM>
__global__ void __launch_bounds__(256) linear_small_kernel(const float* __restrict__ in, const bf16_t* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ add,
                                                           float* __restrict__ out, int M, int N, int K, int act_in, int act_out,
                                                           const int* __restrict__ secs, int nsec, int Mtot, int mrow0) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc[MAXM];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) acc[m] = 0.f;
    const int nvec = K >> 3;
    for (int v = lane; v < nvec; v += 64) {
        const uint4 raw = *(const uint4*)(W + (int64_t)n * K + v * 8);
        float wf[8]; unpack8(raw, wf);
#pragma unroll
        for (int m = 0; m < MAXM; ++m) {
            if (m < M) {
                const float4 x0 = *(const float4*)(in + (int64_t)m * K + v * 8);
                const float4 x1 = *(const float4*)(in + (int64_t)m * K + v * 8 + 4);
                float xf[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                if (act_in) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xf[j] = silu_f(xf[j]);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[m] += xf[j] * wf[j];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[m] += __shfl_xor(acc[m], o);
    }
    if (lane == 0) {
        // sections: columns [secs[s], secs[s+1]) leave as their own dense [M][width] matrix at out + secs[s] * M
        int64_t base = 0; int ldn = N, col = n;
        if (secs) {
            int sidx = 0;
            while (sidx + 1 < nsec && secs[sidx + 1] <= n) ++sidx;
            base = (int64_t)secs[sidx] * Mtot; ldn = secs[sidx + 1] - secs[sidx]; col = n - secs[sidx];
        }
        for (int m = 0; m < M; ++m) {
            float y = acc[m] + (bias ? bias[n] : 0.f) + (add ? add[(int64_t)m * N + n] : 0.f);
            if (act_out) y = silu_f(y);
            out[base + (int64_t)(secs ? mrow0 + m : m) * ldn + col] = y;
        }
    }
}

// rows beyond 16 go out in further launches of 16 (co-batched seeds: B = 32 rows of time / text embeddings)
int linear_small_launch(const float* in, const void* W, const float* bias, const float* add, float* out, int M, int N, int K,
                        int act_in, int act_out, const int* secs, int nsec, hipStream_t st) {
    for (int m0 = 0; m0 < M; m0 += 16) {
        const int m = M - m0 < 16 ? M - m0 : 16;
        const float* in_c = in + (int64_t)m0 * K;
        const float* add_c = add ? add + (int64_t)m0 * N : nullptr;
        // sections: every section is a dense [M][width] matrix, so a row chunk starts m0 * width into each -- the kernel adds
        // secs[s] * M itself; the plain form is one [M][N] matrix
        float* out_c = secs ? out : out + (int64_t)m0 * N;
        if (m <= 4) linear_small_kernel<4><<<(N + 3) / 4, 256, 0, st>>>(in_c, (const bf16_t*)W, bias, add_c, out_c, m, N, K, act_in, act_out, secs, nsec, M, m0);
        else        linear_small_kernel<16><<<(N + 3) / 4, 256, 0, st>>>(in_c, (const bf16_t*)W, bias, add_c, out_c, m, N, K, act_in, act_out, secs, nsec, M, m0);
        TMIX_LAUNCH_CHECK();
    }
    return TMIX_OK;
}

}  // namespace

extern "C" int tmix_layernorm(const void* X, void* Y, const float* gamma, const float* beta, int64_t rows, int C,
                              float eps, void* stream) {
    if (!X || !Y || !gamma || !beta) TMIX_FAIL(TMIX_EINVAL, "layernorm: null pointer");
    if (rows <= 0 || C <= 0) TMIX_FAIL(TMIX_ESHAPE, "layernorm: empty problem");
    if ((C % 8) || C > 2048) TMIX_FAIL(TMIX_ESHAPE, "layernorm: C=%d must be a multiple of 8 and <= 2048", C);
    if (!aligned16(X) || !aligned16(Y) || !aligned16(gamma) || !aligned16(beta)) TMIX_FAIL(TMIX_EALIGN, "layernorm: pointers must be 16-byte aligned");
    layernorm_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>((const bf16_t*)X, (bf16_t*)Y, gamma, beta, rows, C, eps);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_softmax_rows(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, float scale, void* stream) {
    return softmax_entry("softmax_rows", S, ld_s, P, ld_p, rows, cols, scale, 0, cols, true, "%s: rows=%lld cols=%d (cols, ld %% 4 == 0)", 0, stream);
}

extern "C" int tmix_softmax_rows_causal(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, float scale,
                                        int seq, void* stream) {
    return softmax_entry("softmax_rows_causal", S, ld_s, P, ld_p, rows, cols, scale, seq, cols, seq > 0 && seq <= cols && rows % seq == 0,
                         "%s: rows=%lld cols=%d seq=%d (rows %% seq == 0, seq <= cols, cols/ld %% 4 == 0)", seq, stream);
}

extern "C" int tmix_softmax_rows_masked(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, int valid, float scale,
                                        void* stream) {
    return softmax_entry("softmax_rows_masked", S, ld_s, P, ld_p, rows, cols, scale, 0, valid, valid >= 1 && valid <= cols,
                         "%s: rows=%lld cols=%d valid=%d", valid, stream);
}

extern "C" int tmix_quantize_fp8_rows(const void* X, int64_t ld, void* Q, int64_t ldq, uint8_t* scale_e8m0, int64_t rows, int K, void* stream) {
    if (!X || !Q || !scale_e8m0) TMIX_FAIL(TMIX_EINVAL, "quantize_fp8_rows: null pointer");
    if (rows <= 0 || K <= 0 || (K % 8) || K > 8192) TMIX_FAIL(TMIX_ESHAPE, "quantize_fp8_rows: rows=%lld K=%d (K %% 8 == 0, K <= 8192)", (long long)rows, K);
    if (!aligned16(X) || (ld % 8) || (((uintptr_t)Q) & 7) || (ldq % 8)) TMIX_FAIL(TMIX_EALIGN, "quantize_fp8_rows: X rows must be 16-byte, Q rows 8-byte aligned");
    quantize_fp8_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>((const bf16_t*)X, ld, (unsigned char*)Q, ldq, scale_e8m0, rows, K);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_concat_channels(const void* X1, int C1, const void* X2, int C2, void* Y, int64_t rows, void* stream) {
    if (!X1 || !X2 || !Y) TMIX_FAIL(TMIX_EINVAL, "concat: null pointer");
    if (rows <= 0 || C1 <= 0 || C2 <= 0 || (C1 % 8) || (C2 % 8)) TMIX_FAIL(TMIX_ESHAPE, "concat: rows=%lld C1=%d C2=%d unsupported", (long long)rows, C1, C2);
    if (!aligned16(X1) || !aligned16(X2) || !aligned16(Y)) TMIX_FAIL(TMIX_EALIGN, "concat: pointers must be 16-byte aligned");
    int64_t nb = (rows * ((C1 + C2) / 8) + 255) / 256; if (nb > 4096) nb = 4096;
    concat_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>((const uint4*)X1, C1 / 8, (const uint4*)X2, C2 / 8, (uint4*)Y, rows);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_affine_clamp(const float* x, float* y, int64_t n, float scale, float shift, float lo, float hi, void* stream) {
    if (!x || !y) TMIX_FAIL(TMIX_EINVAL, "affine_clamp: null pointer");
    if (n <= 0) TMIX_FAIL(TMIX_ESHAPE, "affine_clamp: empty");
    int64_t nb = (n + 255) / 256; if (nb > 4096) nb = 4096;
    affine_clamp_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(x, y, n, scale, shift, lo, hi);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_zero(void* ptr, int64_t nbytes, void* stream) {
    if (!ptr || nbytes <= 0) TMIX_FAIL(TMIX_EINVAL, "zero: null pointer / empty range");
    hipError_t e = hipMemsetAsync(ptr, 0, (size_t)nbytes, (hipStream_t)stream);
    if (e != hipSuccess) TMIX_FAIL((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
    return TMIX_OK;
}

extern "C" int tmix_timestep_embedding(const float* values, float* out, int count, int dim, void* stream) {
    if (!values || !out) TMIX_FAIL(TMIX_EINVAL, "timestep_embedding: null pointer");
    if (count <= 0 || dim <= 0 || (dim & 1)) TMIX_FAIL(TMIX_ESHAPE, "timestep_embedding: count=%d dim=%d", count, dim);
    const int n = count * (dim / 2);
    timestep_embedding_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(values, out, count, dim);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_linear_small(const float* in, const void* W, const float* bias, const float* add, float* out,
                                 int M, int N, int K, int act_in, int act_out, void* stream) {
    if (!in || !W || !out) TMIX_FAIL(TMIX_EINVAL, "linear_small: null pointer");
    if (M <= 0 || M > 256 || N <= 0 || K <= 0 || (K % 8)) TMIX_FAIL(TMIX_ESHAPE, "linear_small: M=%d (1..256) N=%d K=%d (K %% 8 == 0)", M, N, K);
    if (!aligned16(in) || !aligned16(W)) TMIX_FAIL(TMIX_EALIGN, "linear_small: in/W must be 16-byte aligned");
    return linear_small_launch(in, W, bias, add, out, M, N, K, act_in, act_out, nullptr, 0, (hipStream_t)stream);
}

extern "C" int tmix_linear_small_sections(const float* in, const void* W, const float* bias, float* out, int M, int N, int K,
                                          int act_in, const int* sec_starts, int nsec, void* stream) {
    if (!in || !W || !out || !sec_starts) TMIX_FAIL(TMIX_EINVAL, "linear_small_sections: null pointer");
    if (M <= 0 || M > 256 || N <= 0 || K <= 0 || (K % 8) || nsec < 1) TMIX_FAIL(TMIX_ESHAPE, "linear_small_sections: M=%d (1..256) N=%d K=%d (K %% 8 == 0) nsec=%d", M, N, K, nsec);
    if (!aligned16(in) || !aligned16(W)) TMIX_FAIL(TMIX_EALIGN, "linear_small_sections: in/W must be 16-byte aligned");
    return linear_small_launch(in, W, bias, nullptr, out, M, N, K, act_in, 0, sec_starts, nsec, (hipStream_t)stream);
}
