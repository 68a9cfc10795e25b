// mask_soft.hip -- soft blend weights from binary region masks (no reference counterpart: the reference blends with hard {0, 1} stencils).
//   tmix_mask_edt    exact squared Euclidean distance of every pixel to the nearest set / nearest clear pixel of a mask (int32)
//   tmix_soft_masks  distances -> signed distance to the region border -> dilated, feathered weights u_k -> the K blend weights of a set
// Both run once per image, next to tens of UNet calls; they are written to be exact and simple, not to be at any roofline.
// Compiled with -ffp-contract=off like tweedie_step.hip: every fp32 op below is one correctly rounded op (sqrtf and / compile to the
// correctly rounded sequences), so the weights equal the numpy restatement (masks.soft_masks_reference) bit for bit.  DESIGN.md 7g.
#include "common.h"

namespace {

constexpr int EDT_CAP = 1 << 14;          // column distance of "nothing in this column": above every real distance (h <= 4096)
constexpr int EDT_MAX_SIDE = 4096;

// Column pass: one thread per (mask, column), lanes along x (coalesced).  A down scan writes the distance to the nearest set / clear pixel
// at or above y, an up scan takes the minimum with the nearest at or below.  Plain distances (not squared), capped at EDT_CAP.
__global__ void __launch_bounds__(256)
edt_columns_kernel(const float* __restrict__ mask, int32_t* d_set, int32_t* d_clear, int h, int w) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= w) return;
    const int64_t base = (int64_t)blockIdx.y * h * w + x;
    int ds = EDT_CAP, dc = EDT_CAP;
    for (int y = 0; y < h; ++y) {
        const int64_t i = base + (int64_t)y * w;
        const bool set = mask[i] >= 0.5f;
        ds = set ? 0 : min(ds + 1, EDT_CAP);
        dc = set ? min(dc + 1, EDT_CAP) : 0;
        d_set[i] = ds;
        d_clear[i] = dc;
    }
    ds = EDT_CAP; dc = EDT_CAP;
    for (int y = h - 1; y >= 0; --y) {
        const int64_t i = base + (int64_t)y * w;
        const bool set = mask[i] >= 0.5f;
        ds = set ? 0 : min(ds + 1, EDT_CAP);
        dc = set ? min(dc + 1, EDT_CAP) : 0;
        d_set[i] = min(d_set[i], ds);          // (this thread's own value of the down scan)
        d_clear[i] = min(d_clear[i], dc);
    }
}

// Row pass: one workgroup per (mask, row).  The row's squared column distances g[x']^2 are staged in LDS (a column without a set / clear pixel
// as TMIX_EDT_NONE), then every thread takes, for each of its pixels x = tid, tid + 256, ..., min over x' of (x - x')^2 + g[x']^2 and replaces the
// row in place: the row is read completely before the barrier and no other workgroup touches it.  Integer minima: no order dependence.
//
// Of the two forms of the inner loop this is the PLAIN SWEEP over x': in every iteration all 64 lanes of a wave read the same LDS address,
// which the LDS serves as a broadcast (identical addresses never conflict), four x' per ds_read_b128, and the trip count is uniform, so a
// wave never waits for its slowest lane.  The outward scan from x that stops once (x - x')^2 reaches the best would read per-lane addresses
// (still conflict-free: consecutive lanes, consecutive words) but ends per lane: a wave runs as long as its worst lane, which on the masks that
// occur (rectangles: a long way to the border from the middle, and NONE rows that never stop early) is the full width anyway, for
// two reads and a data-dependent branch per step instead of a quarter of a read.  At w = 128 the sweep is 32 LDS reads per pixel.
__global__ void __launch_bounds__(256)
edt_rows_kernel(int32_t* d_set, int32_t* d_clear, int h, int w) {
    __shared__ __attribute__((aligned(16))) int32_t gs[EDT_MAX_SIDE];
    __shared__ __attribute__((aligned(16))) int32_t gc[EDT_MAX_SIDE];
    const int64_t row = ((int64_t)blockIdx.y * h + blockIdx.x) * w;
    const int w4 = (w + 3) & ~3;
    for (int x = threadIdx.x; x < w4; x += 256) {
        int a = TMIX_EDT_NONE, b = TMIX_EDT_NONE;          // the padding up to a multiple of four never wins a minimum
        if (x < w) {
            const int s = d_set[row + x], c = d_clear[row + x];
            a = s >= EDT_CAP ? TMIX_EDT_NONE : s * s;
            b = c >= EDT_CAP ? TMIX_EDT_NONE : c * c;
        }
        gs[x] = a;
        gc[x] = b;
    }
    __syncthreads();
    const int4* gs4 = reinterpret_cast<const int4*>(gs);
    const int4* gc4 = reinterpret_cast<const int4*>(gc);
    for (int x = threadIdx.x; x < w; x += 256) {
        int bs = TMIX_EDT_NONE, bc = TMIX_EDT_NONE;
        for (int q = 0; q < w4 / 4; ++q) {
            const int4 s = gs4[q], c = gc4[q];
            const int d0 = x - 4 * q, d1 = d0 - 1, d2 = d0 - 2, d3 = d0 - 3;
            const int e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2, e3 = d3 * d3;      // <= 4095^2; + TMIX_EDT_NONE stays below 2^31
            bs = min(min(bs, e0 + s.x), min(e1 + s.y, min(e2 + s.z, e3 + s.w)));
            bc = min(min(bc, e0 + c.x), min(e1 + c.y, min(e2 + c.z, e3 + c.w)));
        }
        d_set[row + x] = bs;               // (bs, bc start at TMIX_EDT_NONE: the clamp)
        d_clear[row + x] = bc;
    }
}

// u of one concept at one pixel (section 1 of DESIGN.md 7g): signed distance to the border midway between pixel centres, moved by the
// dilation, ramped over the feather width
__device__ __forceinline__ float soft_u(int ds, int dc, float feather, float dilate) {
    const float s = ds == 0 ? -(sqrtf((float)dc) - 0.5f) : sqrtf((float)ds) - 0.5f;      // d_set == 0: a set pixel
    const float sp = s - dilate;
    if (feather > 0.0f) {
        const float q = sp / feather;
        return fminf(fmaxf(0.5f - q, 0.0f), 1.0f);
    }
    return sp < 0.0f ? 1.0f : 0.0f;
}

// One thread owns one pixel of one set: the K-1 concepts in ascending order, t in fp32, then the K weights.  u is computed twice (sum, then
// weights) instead of being read back: a handful of flops per pixel, and no thread reads what it wrote.
__global__ void __launch_bounds__(256)
soft_masks_kernel(const int32_t* __restrict__ d_set, const int32_t* __restrict__ d_clear, float* __restrict__ out, int K, int64_t hw,
                  int64_t total, float feather, float dilate, int normalize) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t set = i / hw, p = i % hw;
        const int32_t* ds = d_set + set * (K - 1) * hw + p;
        const int32_t* dc = d_clear + set * (K - 1) * hw + p;
        float* o = out + set * K * hw + p;
        float t = 0.0f;
        for (int k = 0; k < K - 1; ++k)
            t = t + soft_u(ds[k * hw], dc[k * hw], feather, dilate);
        const bool scale = normalize && t > 1.0f;
        for (int k = 0; k < K - 1; ++k) {
            const float u = soft_u(ds[k * hw], dc[k * hw], feather, dilate);
            o[k * hw] = scale ? u / t : u;
        }
        o[(int64_t)(K - 1) * hw] = scale ? 0.0f : (normalize ? 1.0f - t : fmaxf(1.0f - t, 0.0f));
    }
}

}  // namespace

extern "C" int tmix_mask_edt(const float* mask, int32_t* d_set, int32_t* d_clear, int n, int h, int w, void* stream) {
    if (!mask || !d_set || !d_clear) TMIX_FAIL(TMIX_EINVAL, "mask_edt: null pointer");
    if (h < 1 || w < 1 || h > EDT_MAX_SIDE || w > EDT_MAX_SIDE || n < 1 || n > 65535)
        TMIX_FAIL(TMIX_ESHAPE, "mask_edt: n=%d (1..65535) masks of %d x %d (1..%d each side)", n, h, w, EDT_MAX_SIDE);
    edt_columns_kernel<<<dim3((unsigned)((w + 255) / 256), (unsigned)n), 256, 0, (hipStream_t)stream>>>(mask, d_set, d_clear, h, w);
    TMIX_LAUNCH_CHECK();
    edt_rows_kernel<<<dim3((unsigned)h, (unsigned)n), 256, 0, (hipStream_t)stream>>>(d_set, d_clear, h, w);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_soft_masks(const int32_t* d_set, const int32_t* d_clear, float* out, int n_sets, int K, int h, int w, float feather,
                               float dilate, int normalize, void* stream) {
    if (!d_set || !d_clear || !out) TMIX_FAIL(TMIX_EINVAL, "soft_masks: null pointer");
    if (!(feather >= 0.0f) || !(feather <= 3.0e38f))          // (NaN fails both comparisons)
        TMIX_FAIL(TMIX_EINVAL, "soft_masks: feather=%g, a finite ramp width >= 0 in latent pixels", (double)feather);
    if (!(dilate >= -3.0e38f && dilate <= 3.0e38f))
        TMIX_FAIL(TMIX_EINVAL, "soft_masks: dilate=%g, a finite margin in latent pixels", (double)dilate);
    if (K < 2 || n_sets < 1 || h < 1 || w < 1 || h > EDT_MAX_SIDE || w > EDT_MAX_SIDE || (int64_t)n_sets * (K - 1) > 65535)
        TMIX_FAIL(TMIX_ESHAPE, "soft_masks: n_sets=%d (>= 1) K=%d (>= 2, n_sets * (K - 1) <= 65535) grid %d x %d (1..%d each side)", n_sets, K, h, w,
                  EDT_MAX_SIDE);
    const int64_t hw = (int64_t)h * w, total = (int64_t)n_sets * hw;
    int64_t blocks = (total + 255) / 256; if (blocks > 2048) blocks = 2048;
    soft_masks_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(d_set, d_clear, out, K, hw, total, feather, dilate, normalize != 0);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
