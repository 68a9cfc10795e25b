// temporal_attn.hip -- the video UNet's temporal attention: attention over the (<= 16) frames of one pixel.  Entry point: tmix_temporal_attn.
//
// I2VGen-XL's TransformerTemporalModel attends over the FRAMES of one pixel: sequences of 16 tokens, head size 64, one (clip, pixel, head) item per wave,
// on the matrix cores: S^T = K Q^T is two v_mfma_f32_16x16x32_bf16 (operands straight from global memory: a lane's fragment is 16 contiguous bytes of
// its frame's row), the softmax runs over the four scores a lane holds and its three partner lanes (xor 16 / 32), and the exponentials ARE the B operand of
// O^T = V^T P^T (four v_mfma_f32_16x16x16_bf16, one per 16 channels) -- only V has to turn: its rows go through LDS and come back as four 2-byte reads per
// MFMA.  The round-3 form did the 2 x 16 x 16 x 64 multiply-adds of an item on the VALU (~175 us for the 86,016 x 5 items of the first level against
// ~100 us of HBM time for its 440 MB).
#include "common.h"

namespace {
typedef short short4_t __attribute__((ext_vector_type(4)));
constexpr int TA_VLD = 68;                       // LDS row of V: 64 channels + 4 pad (136 B: the four frames a lane group reads sit 8 banks apart)
__global__ void __launch_bounds__(256) temporal_attn_kernel(const bf16_t* __restrict__ QKV, int64_t ld, bf16_t* __restrict__ O, int64_t ldo,
                                                            int frames, int64_t hw, int heads, int64_t items, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) bf16_t sV[4][16][TA_VLD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + w;
    const bool live = item < items;
    const int C = heads * 64;
    const int r = lane & 15, g = lane >> 4;
    const int64_t ph = live ? item : 0;
    const int h = (int)(ph % heads);
    const int64_t cp = ph / heads;                                   // clip * hw + pixel
    const int64_t clip = cp / hw, pix = cp - clip * hw;
    const int64_t row = (clip * frames + (r < frames ? r : 0)) * hw + pix;      // token row of frame r (padding frames re-read frame 0: finite values)
    const bf16_t* q = QKV + row * ld + h * 64;
    // fragments of the score MFMAs: lane (r, g) holds channels [32 kb + 8 g, +8) of frame r -- K as A (rows = key frames), Q as B (columns = query frames)
    const frag_ab k0 = *(const frag_ab*)(q + C + g * 8), k1 = *(const frag_ab*)(q + C + 32 + g * 8);
    const frag_ab q0 = *(const frag_ab*)(q + g * 8), q1 = *(const frag_ab*)(q + 32 + g * 8);
    // V rows -> LDS (lane: frame r, channels [16 g, +16))
    {
        const uint4 va = *(const uint4*)(q + 2 * C + g * 16), vb = *(const uint4*)(q + 2 * C + g * 16 + 8);
        uint2* dst = (uint2*)&sV[w][r][g * 16];
        dst[0] = make_uint2(va.x, va.y); dst[1] = make_uint2(va.z, va.w); dst[2] = make_uint2(vb.x, vb.y); dst[3] = make_uint2(vb.z, vb.w);
    }
    f32x4 st = {0.f, 0.f, 0.f, 0.f};
    st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, q0, st, 0, 0, 0);
    st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, q1, st, 0, 0, 0);          // st[j] = K[4 g + j] . Q[r]
    float sc[4], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) { sc[j] = (4 * g + j) < frames ? st[j] * scale_log2e : -INFINITY; mx = fmaxf(mx, sc[j]); }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { sc[j] = exp2f(sc[j] - mx); sum += sc[j]; }          // 0 for padded frames
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    short4_t pb;                                                                     // P^T as the B operand: column = query r, k = keys 4 g .. 4 g + 3
    {
        const unsigned lo = pack_bf2(sc[0], sc[1]), hi = pack_bf2(sc[2], sc[3]);
        pb = (short4_t){(short)(lo & 0xffff), (short)(lo >> 16), (short)(hi & 0xffff), (short)(hi >> 16)};
    }
    __syncthreads();
    bf16_t* dst = O + row * ldo + h * 64 + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        // V^T as the A operand: row = channel 16 db + r, k = keys 4 g .. 4 g + 3
        short4_t va;
#pragma unroll
        for (int j = 0; j < 4; ++j) va[j] = (short)sV[w][4 * g + j][16 * db + r];
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        o = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(va, pb, o, 0, 0, 0);          // o[j] = O[query r][channel 16 db + 4 g + j] * sum
        if (live && r < frames) *(uint2*)(dst + 16 * db) = make_uint2(pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv));
    }
}
}  // namespace

extern "C" int tmix_temporal_attn(const void* QKV, int64_t ld, void* O, int64_t ldo, int clips, int frames, int64_t hw, int heads,
                                  float scale, void* stream) {
    if (!QKV || !O) TMIX_FAIL(TMIX_EINVAL, "temporal_attn: null pointer");
    if (clips < 1 || frames < 1 || frames > 16 || hw < 1 || heads < 1) TMIX_FAIL(TMIX_ESHAPE, "temporal_attn: clips=%d frames=%d (1..16) hw=%lld heads=%d", clips, frames, (long long)hw, heads);
    if (ld < 3 * heads * 64 || ldo < heads * 64 || (ld % 8) || (ldo % 8)) TMIX_FAIL(TMIX_ESHAPE, "temporal_attn: ld=%lld ldo=%lld for %d heads of 64", (long long)ld, (long long)ldo, heads);
    if (!aligned16(QKV) || !aligned16(O)) TMIX_FAIL(TMIX_EALIGN, "temporal_attn: pointers must be 16-byte aligned");
    const int64_t items = (int64_t)clips * hw * heads;
    const int64_t blocks = (items + 3) / 4;
    if (blocks > 0x7fffffff) TMIX_FAIL(TMIX_ESHAPE, "temporal_attn: grid too large");
    temporal_attn_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const bf16_t*)QKV, ld, (bf16_t*)O, ldo, frames, hw, heads, items, scale * LOG2E);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
