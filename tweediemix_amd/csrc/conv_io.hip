// conv_io.hip -- the first and the last convolution of a UNet / VAE pass, where one side is fp32 NCHW and has a handful of channels:
// conv_in (3 / 4 / 8 -> Cout channels, fp32 VALU, bf16 NHWC output; tmix_conv_in_pre adds a per-pixel linear map of the latent, PreMap) and
// conv_out (Cin -> <= 16 channels, MFMA, fp32 NCHW output).  Entry points: tmix_conv_in, tmix_conv_in_pre, tmix_conv_out.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------ conv_in (fp32 VALU)
// workgroup = 64 consecutive output pixels x all Cout; lane = pixel (its 3x3xCIN patch lives in registers), wave q
// owns a quarter of the output channels; the fp32 OHWI weights are staged once per workgroup in LDS and read as
// wave-uniform broadcasts.  fp32 math (the latent is not rounded to bf16 before the first convolution).
struct PreMap { float w[16]; float b[4]; int on; };

template <int CIN>
__global__ void __launch_bounds__(256) conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                      int B, int H, int W, int Cout, const PreMap pm) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];        // [Cout][9*CIN]
    constexpr int KK = 9 * CIN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < Cout * KK / 4; i += 256) ((float4*)s_w)[i] = ((const float4*)w)[i];
    __syncthreads();
    const int64_t npix = (int64_t)B * H * W;
    // persistent over 64-pixel tiles: the weight stage (up to 92 KB) is paid once per workgroup, not once per 64 pixels
    for (int64_t tile = blockIdx.x; tile * 64 < npix; tile += gridDim.x) {
    int64_t pix = tile * 64 + lane;
    const bool live = pix < npix;
    if (!live) pix = npix - 1;
    const int b = (int)(pix / ((int64_t)H * W)); const int rem = (int)(pix - (int64_t)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    float patch[KK];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy + ky - 1, ix = ox + kx - 1;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            float v[CIN];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) v[ci] = ok ? x[(((int64_t)b * CIN + ci) * H + iy) * W + ix] : 0.f;
            if (pm.on && CIN == 4) {          // per-pixel linear map of the latent; padding stays exactly zero
                float u[4];
#pragma unroll
                for (int co = 0; co < 4; ++co)
                    u[co] = ok ? pm.b[co] + pm.w[co * 4 + 0] * v[0] + pm.w[co * 4 + 1] * v[1] + pm.w[co * 4 + 2] * v[2] + pm.w[co * 4 + 3] * v[3] : 0.f;
#pragma unroll
                for (int co = 0; co < 4; ++co) v[co] = u[co];
            }
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) patch[(ky * 3 + kx) * CIN + ci] = v[ci];
        }
    const int cpq = Cout / 4;                      // output channels per wave (multiple of 8)
    for (int c0 = q * cpq; c0 < (q + 1) * cpq; c0 += 8) {
        float o[8];
        // (CIN = 8: 72-tap patches; unrolling all 8 filters at once spills 160 registers to scratch and runs 6x slower per flop)
#pragma unroll 2
        for (int j = 0; j < 8; ++j) {
            const float* wr = s_w + (c0 + j) * KK;
            float a = bias ? bias[c0 + j] : 0.f;
#pragma unroll
            for (int k = 0; k < KK; ++k) a += patch[k] * wr[k];
            o[j] = a;
        }
        if (live) *(uint4*)(y + pix * Cout + c0) = pack8(o);
    }
    }
}

// raises the instantiation's dynamic-LDS limit when this launch needs more than any before it (64 KB need no attribute), then launches
template <int CIN>
int launch_conv_in(unsigned nb, int smem, hipStream_t st, const float* x, const float* w, const float* bias, bf16_t* y, int B, int H, int W, int Cout, const PreMap& pm) {
    static int attr_smem = 0;                      // the largest size set so far
    if (smem > 64 * 1024 && smem > attr_smem) {
        hipError_t e = hipFuncSetAttribute((const void*)conv_in_kernel<CIN>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) TMIX_FAIL((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_smem = smem;
    }
    conv_in_kernel<CIN><<<nb, 256, smem, st>>>(x, w, bias, y, B, H, W, Cout, pm);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// ------------------------------------------------------------------------------ conv_out (MFMA)
// wave = 16 output pixels x (<=16 padded) output channels; K = 9*Cin streamed straight from global
// (A fragment = 16 B of one pixel's channels per lane, W fragment = 16 B of one filter row per lane).
__global__ void __launch_bounds__(256) conv_out_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y,
                                                       int B, int H, int W, int Cin, int Cout) {
    const int lane = threadIdx.x & 63, fr = lane & 15, fg = lane >> 4;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t pbase = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (pbase >= npix) return;
    int64_t pix = pbase + fr; if (pix > npix - 1) pix = npix - 1;
    const int b = (int)(pix / ((int64_t)H * W)); const int rem = (int)(pix - (int64_t)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    const int co = fr < Cout ? fr : Cout - 1;                 // padded filter rows replicate a real one
    const bf16_t* wrow = w + (int64_t)co * 9 * Cin;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const frag_ab zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const bf16_t* src = x + (((int64_t)b * H + (ok ? iy : 0)) * W + (ok ? ix : 0)) * Cin;
        for (int c = 0; c < Cin; c += 32) {
            frag_ab a = *(const frag_ab*)(src + c + fg * 8);
            if (!ok) a = zero;
            const frag_ab wf = *(const frag_ab*)(wrow + tap * Cin + c + fg * 8);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf, acc, 0, 0, 0);   // D[pixel][cout]
        }
    }
    // lane holds pixels pbase + 4*fg + r for output channel fr
    if (fr < Cout) {
        const float bv = bias ? bias[fr] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t pp = pbase + fg * 4 + r;
            if (pp < npix) {
                const int bb = (int)(pp / ((int64_t)H * W)); const int64_t rr = pp - (int64_t)bb * H * W;
                y[((int64_t)bb * Cout + fr) * H * W + rr] = acc[r] + bv;
            }
        }
    }
}

}  // namespace

extern "C" int tmix_conv_in(const float* x_nchw, const float* w_ohwi, const float* bias, void* y_nhwc,
                            int B, int Cin, int H, int W, int Cout, void* stream) {
    return tmix_conv_in_pre(x_nchw, w_ohwi, bias, y_nhwc, B, Cin, H, W, Cout, nullptr, nullptr, stream);
}

extern "C" int tmix_conv_in_pre(const float* x_nchw, const float* w_ohwi, const float* bias, void* y_nhwc,
                                int B, int Cin, int H, int W, int Cout, const float* pre_w, const float* pre_b, void* stream) {
    if (!x_nchw || !w_ohwi || !y_nhwc) TMIX_FAIL(TMIX_EINVAL, "conv_in: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0) TMIX_FAIL(TMIX_ESHAPE, "conv_in: bad shape");
    if (!aligned16(y_nhwc)) TMIX_FAIL(TMIX_EALIGN, "conv_in: output must be 16-byte aligned");
    if (Cout % 32) TMIX_FAIL(TMIX_ESHAPE, "conv_in: Cout=%d must be a multiple of 32", Cout);
    if (Cin != 3 && Cin != 4 && Cin != 8) TMIX_FAIL(TMIX_ESHAPE, "conv_in: Cin=%d (3: RGB image, 4: image latent, 8: video latent + image-latent features)", Cin);
    if (Cin != 4 && pre_w) TMIX_FAIL(TMIX_EINVAL, "conv_in: the latent pre-map is defined for 4 channels");
    if ((Cout * 9 * Cin) % 4) TMIX_FAIL(TMIX_ESHAPE, "conv_in: Cout*9*Cin must be a multiple of 4");
    if (!aligned16(w_ohwi)) TMIX_FAIL(TMIX_EALIGN, "conv_in: weights must be 16-byte aligned");
    const int64_t npix = (int64_t)B * H * W;
    const int64_t ntiles = (npix + 63) / 64;
    const int smem = Cout * 9 * Cin * 4;
    const int per_cu = smem > 80 * 1024 ? 1 : (smem > 52 * 1024 ? 2 : 3);            // resident workgroups per CU (LDS)
    const unsigned nb = (unsigned)(ntiles < 256 * per_cu ? ntiles : 256 * per_cu);
    if (smem > 150 * 1024) TMIX_FAIL(TMIX_ESHAPE, "conv_in: Cout=%d too large for the LDS weight stage", Cout);
    PreMap pm = {};
    if (pre_w) {
        pm.on = 1;
        for (int i = 0; i < 16; ++i) pm.w[i] = pre_w[i];
        for (int i = 0; i < 4; ++i) pm.b[i] = pre_b ? pre_b[i] : 0.f;
    }
    hipStream_t st = (hipStream_t)stream;
    bf16_t* y = (bf16_t*)y_nhwc;
    switch (Cin) {
        case 8:  return launch_conv_in<8>(nb, smem, st, x_nchw, w_ohwi, bias, y, B, H, W, Cout, pm);
        case 3:  return launch_conv_in<3>(nb, smem, st, x_nchw, w_ohwi, bias, y, B, H, W, Cout, pm);
        default: return launch_conv_in<4>(nb, smem, st, x_nchw, w_ohwi, bias, y, B, H, W, Cout, pm);
    }
}

extern "C" int tmix_conv_out(const void* x_nhwc, const void* w_ohwi, const float* bias, float* y_nchw,
                             int B, int Cin, int H, int W, int Cout, void* stream) {
    if (!x_nhwc || !w_ohwi || !y_nchw) TMIX_FAIL(TMIX_EINVAL, "conv_out: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 16 || (Cin % 32)) TMIX_FAIL(TMIX_ESHAPE, "conv_out: Cin=%d (%%32) Cout=%d (<=16)", Cin, Cout);
    if (!aligned16(x_nhwc) || !aligned16(w_ohwi)) TMIX_FAIL(TMIX_EALIGN, "conv_out: pointers must be 16-byte aligned");
    const int64_t npix = (int64_t)B * H * W;
    const unsigned nb = (unsigned)((npix + 63) / 64);
    conv_out_kernel<<<nb, 256, 0, (hipStream_t)stream>>>((const bf16_t*)x_nhwc, (const bf16_t*)w_ohwi, bias, y_nchw, B, H, W, Cin, Cout);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
