// noise.h -- the counter-based noise of the stochastic sampler: one Philox4x32-10 call (Salmon et al., SC'11) per element and
// Box-Muller on its output words 0 and 1.  The value is a pure function of (key, index, step, stream id): no state, no buffer, the same bits
// from every launch shape.  One call per element wastes two of the four words on purpose: packing four elements into a call would tie an
// element's noise to the alignment of the window it is computed in.
// Stream ids: 0 the image sampler's step (STREAM_IMAGE_STEP in noise.py), 1 the video sampler's step (STREAM_VIDEO_STEP): an image
// run and a video run from one seed draw unrelated noise; 2 the one fixed noise of the video sampler's hold regions (STREAM_VIDEO_HOLD, DESIGN.md 7p;
// always at step 0).  Every other value is reserved.
// ln, sin and cos are written out in integer operations and single-rounded fp32 add, sub, mul, div and sqrt, and every file that includes this
// is compiled with -ffp-contract=off: tweediemix_amd/noise.py restates the same operations in numpy and is compared by equality.  The functions
// are __host__ __device__ so that a host program can make the same comparison without a GPU.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0; c1 = (uint32_t)p1; c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1; c3 = (uint32_t)p0;
    }
    return {{c0, c1, c2, c3}};
}

// ln u for u in (0, 1): exponent from the bit pattern, mantissa reduced to [sqrt(1/2), sqrt 2), atanh series in s = (m-1)/(m+1):
// ln m = 2 s (1 + s^2/3 + s^4/5 + s^6/7 + s^8/9), |s| <= 0.1716 (the next term is below 2e-10 of the sum)
__host__ __device__ __forceinline__ float noise_ln(float u) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, u);
    int e = (int)(bits >> 23) - 127;
    float m = __builtin_bit_cast(float, (bits & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
    const float s = (m - 1.0f) / (m + 1.0f);
    const float s2 = s * s;
    float p = 0.111111112f;                 // 1/9, 1/7, 1/5, 1/3 rounded to fp32
    p = p * s2 + 0.142857149f;
    p = p * s2 + 0.200000003f;
    p = p * s2 + 0.333333343f;
    p = p * s2 + 1.0f;
    const float lnm = (s + s) * p;
    const float ef = (float)e;
    return ef * 0.693145751953125f + (ef * 1.42860682e-06f + lnm);     // ln 2 = hi + lo; hi has 12 significant bits: ef * hi is exact
}

// Box-Muller: u1 = ((w0 >> 9) + 0.5) 2^-23 >= 2^-24, so |z| < 5.8; angle = 2 pi ((w1 >> 9) + 0.5) 2^-23: the quadrant from the two top bits of
// the 23, the rest folded to [0, pi/4], Taylor polynomials of degree 9 (sin) and 8 (cos) there
__host__ __device__ __forceinline__ float noise_normal_words(uint32_t w0, uint32_t w1) {
    const float u1 = ((float)(w0 >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float r = sqrtf(-2.0f * noise_ln(u1));
    const uint32_t a = w1 >> 9, q = a >> 21;
    float t = ((float)(a & 0x1FFFFFu) + 0.5f) * 4.76837158203125e-07f;
    const bool fold = t > 0.5f;
    if (fold) t = 1.0f - t;
    const float p = t * 1.57079637f;
    const float p2 = p * p;
    float sn = 2.75573188e-06f, cs = 2.48015876e-05f;        // 1/9!, 1/8!
    sn = sn * p2 + -1.98412701e-04f; cs = cs * p2 + -1.38888892e-03f;     // -1/7!, -1/6!
    sn = sn * p2 + 8.33333377e-03f;  cs = cs * p2 + 4.16666679e-02f;      // 1/5!, 1/4!
    sn = sn * p2 + -0.166666672f;    cs = cs * p2 + -0.5f;
    sn = p * (sn * p2 + 1.0f);
    cs = cs * p2 + 1.0f;
    // cos(q pi/2 + theta) = cos theta, -sin theta, -cos theta, sin theta; folded, sin and cos of theta trade places
    float c = (((q & 1u) != 0u) != fold) ? sn : cs;
    if (q == 1u || q == 2u) c = -c;
    return r * c;
}

// z of element `index` of the trajectory with key {key_lo, key_hi} at schedule step `step`
__host__ __device__ __forceinline__ float noise_normal(uint64_t index, uint32_t key_lo, uint32_t key_hi, uint32_t step, uint32_t stream_id) {
    const Philox4 o = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), step, stream_id, key_lo, key_hi);
    return noise_normal_words(o.w[0], o.w[1]);
}

}  // namespace
