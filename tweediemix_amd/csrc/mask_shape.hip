// mask_shape.hip -- free-form attention masks (no reference counterpart: the side-car ends in bounding rectangles).
//   tmix_mask_label   4-connected component labels of the set (or clear) pixels of a thresholded map: the smallest raster index of the component
//   tmix_attn_shapes  per concept the largest component of score >= threshold, its holes filled; overlaps of a set go to the highest score
// Both run once per image on maps of at most 128 x 128, next to tens of UNet calls: written to be exact, bounded and simple.  DESIGN.md 7h.
//
// One workgroup owns one map and keeps its labels in LDS.  The labelling is a union-find forest in which a parent is never larger than its
// child (L[p] <= p always).  It starts from the horizontal runs (every pixel under the first pixel of its run, read off the bit mask), then
// merges runs that touch vertically: a merge writes L by atomicMin alone and the flatten pass replaces a parent by an ancestor, so labels
// only fall, the walk from any pixel towards its root strictly decreases and ends after at most h * w steps whatever other lanes write
// meanwhile, and the root of a finished tree is the component's smallest raster index -- a value that does not depend on the order in which
// lanes ran.  No lane ever waits for a value that another lane has yet to write: every loop is a `for` over a bound computed from the
// arguments, left early by the lane that is done.
// Sizes, the winner and the border flags are integer atomics at the roots (adds, a max, ors): order-independent as well.  No float atomics.
#include "common.h"

namespace {

constexpr int SHAPE_THREADS = 1024;

__device__ __forceinline__ bool bit_of(const uint32_t* bits, int p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// bits[] <- (map[p] >= thr), one word per lane at a time (no atomics: a word has one writer).  Leaves a barrier behind.
__device__ __forceinline__ void threshold_bits(const float* __restrict__ map, float thr, uint32_t* bits, int n) {
    const int words = (n + 31) >> 5;
    for (int wd = threadIdx.x; wd < words; wd += SHAPE_THREADS) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) {
            const int p = wd * 32 + b;
            if (p < n && map[p] >= thr) v |= 1u << b;
        }
        bits[wd] = v;
    }
    __syncthreads();
}

// first pixel of the horizontal run of `want` pixels that holds p (p is one of them; row0 = first pixel of p's row): the highest pixel at or
// below p whose bit differs, plus one.  One bit-mask word per round, at most w / 32 + 2 of them.
__device__ __forceinline__ int run_start(const uint32_t* bits, bool want, int p, int row0, int w) {
    const uint32_t flip = want ? ~0u : 0u;                        // (word ^ flip) has a 1 where the pixel is NOT of the wanted kind
    int wd = p >> 5;
    uint32_t miss = (bits[wd] ^ flip) & ((2u << (p & 31)) - 1u);  // the pixels of this word at or below p (p & 31 == 31: all 32)
    for (int it = 0; it < w / 32 + 2; ++it) {
        if (miss) return max(row0, wd * 32 + 32 - __clz(miss));
        if (wd * 32 <= row0) break;
        --wd;
        miss = bits[wd] ^ flip;
    }
    return row0;
}

// root of p's tree: parents strictly decrease, so at most n steps
__device__ __forceinline__ int find_root(const int32_t* L, int p, int n) {
    for (int it = 0; it < n; ++it) {
        const int q = L[p];
        if (q == p) break;
        p = q;
    }
    return p;
}

// joins the trees of a and b.  Each round walks both to their roots and hooks the larger root under the smaller; if another lane lowered that
// root in between, the round goes on from the parent it was given.  max(a, b) strictly falls from round to round, so at most n rounds.
__device__ __forceinline__ void unite(int32_t* L, int a, int b, int n) {
    for (int it = 0; it < n; ++it) {
        a = find_root(L, a, n);
        b = find_root(L, b, n);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b
        const int old = atomicMin(&L[a], b);
        if (old == a) break;                                     // a was still a root and now hangs under b
        a = old;                                                 // a's new parent (< a) still has to meet b
    }
}

// L[p] <- smallest raster index of p's 4-connected component among the pixels whose bit equals `want`, -1 for the others.
// Called by the whole workgroup; bits[] must be complete (barrier before), L is complete on return (barrier inside).
__device__ void label_bits(const uint32_t* bits, bool want, int32_t* L, int h, int w) {
    const int n = h * w;
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
        L[p] = bit_of(bits, p) == want ? run_start(bits, want, p, p - p % w, w) : -1;
    __syncthreads();
    // vertical merges, one per contact of two runs: where the pair to the left (p - 1 above p - w - 1) is a contact of the same two runs, skip
    for (int p = threadIdx.x + w; p < n; p += SHAPE_THREADS) {
        if (bit_of(bits, p) != want || bit_of(bits, p - w) != want) continue;
        if (p % w > 0 && bit_of(bits, p - 1) == want && bit_of(bits, p - w - 1) == want) continue;
        unite(L, p, p - w, n);
    }
    __syncthreads();
    // flatten: a lane that shortens its own pixel's path only replaces a parent by an ancestor, so concurrent walks stay inside their tree
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
        if (L[p] >= 0) L[p] = find_root(L, p, n);
    __syncthreads();
}

__global__ void __launch_bounds__(SHAPE_THREADS)
mask_label_kernel(const float* __restrict__ map, float thr, int invert, int32_t* __restrict__ label, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    const int n = h * w;
    int32_t* L = lds;
    uint32_t* bits = reinterpret_cast<uint32_t*>(lds + n);
    const int64_t base = (int64_t)blockIdx.x * n;
    threshold_bits(map + base, thr, bits, n);
    label_bits(bits, invert == 0, L, h, w);
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
        label[base + p] = L[p];
}

// One workgroup per (set, concept): threshold -> labels -> sizes -> winner -> (labels of the winner's complement -> border flags -> holes) -> out
__global__ void __launch_bounds__(SHAPE_THREADS)
attn_shape_kernel(const float* __restrict__ score, float* __restrict__ out, int h, int w, float thr, int fill) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    __shared__ int best;
    const int n = h * w, words = (n + 31) >> 5;
    int32_t* L = lds;
    int32_t* aux = lds + n;                                        // component sizes, later border flags, at the roots
    uint32_t* bits = reinterpret_cast<uint32_t*>(lds + 2 * n);     // score >= thr
    uint32_t* shape = bits + words;                                // c_k
    const int64_t base = (int64_t)blockIdx.x * n;
    if (threadIdx.x == 0) best = 0;
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS) aux[p] = 0;
    threshold_bits(score + base, thr, bits, n);
    label_bits(bits, true, L, h, w);
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
        if (L[p] >= 0) atomicAdd(&aux[L[p]], 1);
    __syncthreads();
    // the winner: most pixels, then the smallest root.  count <= 2^14 and root < 2^14: (count << 14) | (2^14 - 1 - root) orders exactly so
    for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
        if (L[p] == p) atomicMax(&best, (aux[p] << 14) | (TMIX_SHAPE_MAX_PIXELS - 1 - p));
    __syncthreads();
    const int key = best;
    const int win = key > 0 ? TMIX_SHAPE_MAX_PIXELS - 1 - (key & (TMIX_SHAPE_MAX_PIXELS - 1)) : -2;      // -2: empty map, matches no label
    for (int wd = threadIdx.x; wd < words; wd += SHAPE_THREADS) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) {
            const int p = wd * 32 + b;
            if (p < n && L[p] == win) v |= 1u << b;
        }
        shape[wd] = v;
    }
    __syncthreads();
    if (fill) {
        for (int p = threadIdx.x; p < n; p += SHAPE_THREADS) aux[p] = 0;
        label_bits(shape, false, L, h, w);                          // (its first barrier also orders the zeroing above)
        for (int p = threadIdx.x; p < n; p += SHAPE_THREADS) {
            const int y = p / w, x = p % w;
            if (L[p] >= 0 && (y == 0 || y == h - 1 || x == 0 || x == w - 1)) atomicOr(&aux[L[p]], 1);
        }
        __syncthreads();
        for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
            out[base + p] = (bit_of(shape, p) || (L[p] >= 0 && aux[L[p]] == 0)) ? 1.0f : 0.0f;
    } else {
        for (int p = threadIdx.x; p < n; p += SHAPE_THREADS)
            out[base + p] = bit_of(shape, p) ? 1.0f : 0.0f;
    }
}

// One thread owns one pixel of one set: of the concepts that claim it, the highest score keeps it (strict >, ascending k: ties to the smallest k)
__global__ void __launch_bounds__(256)
attn_resolve_kernel(const float* __restrict__ score, float* out, int km1, int64_t hw, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t off = (i / hw) * km1 * hw + i % hw;
        int owner = -1, claims = 0;
        float top = 0.0f;
        for (int k = 0; k < km1; ++k) {
            if (out[off + k * hw] == 0.0f) continue;
            const float s = score[off + k * hw];
            if (owner < 0 || s > top) { owner = k; top = s; }
            ++claims;
        }
        if (claims < 2) continue;
        for (int k = 0; k < km1; ++k)
            if (k != owner) out[off + k * hw] = 0.0f;
    }
}

// raises a kernel's dynamic-LDS limit when a launch needs more than any before it (64 KB need no attribute)
int raise_lds_limit(const void* kernel, int* set_so_far, int smem) {
    if (smem > 64 * 1024 && smem > *set_so_far) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) TMIX_FAIL((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        *set_so_far = smem;
    }
    return TMIX_OK;
}

}  // namespace

extern "C" int tmix_mask_label(const float* map, float threshold, int invert, int32_t* label, int n, int h, int w, void* stream) {
    if (!map || !label) TMIX_FAIL(TMIX_EINVAL, "mask_label: null pointer");
    if (!(threshold >= -3.0e38f && threshold <= 3.0e38f))          // (NaN fails both comparisons)
        TMIX_FAIL(TMIX_EINVAL, "mask_label: threshold=%g is not finite", (double)threshold);
    if (h < 1 || w < 1 || n < 1 || n > 65535 || (int64_t)h * w > TMIX_SHAPE_MAX_PIXELS)
        TMIX_FAIL(TMIX_ESHAPE, "mask_label: n=%d (1..65535) maps of %d x %d (each side >= 1, h * w <= %d)", n, h, w, TMIX_SHAPE_MAX_PIXELS);
    const int px = h * w, smem = px * 4 + ((px + 31) / 32) * 4;
    static int attr_smem = 0;
    if (int rc = raise_lds_limit((const void*)mask_label_kernel, &attr_smem, smem)) return rc;
    mask_label_kernel<<<(unsigned)n, SHAPE_THREADS, smem, (hipStream_t)stream>>>(map, threshold, invert, label, h, w);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_attn_shapes(const float* score, float* out, int n_sets, int km1, int h, int w, float threshold, int flags, void* stream) {
    if (!score || !out) TMIX_FAIL(TMIX_EINVAL, "attn_shapes: null pointer");
    if (!(threshold >= -3.0e38f && threshold <= 3.0e38f))
        TMIX_FAIL(TMIX_EINVAL, "attn_shapes: threshold=%g is not finite", (double)threshold);
    if (flags & ~(TMIX_SHAPE_FILL_HOLES | TMIX_SHAPE_RESOLVE))
        TMIX_FAIL(TMIX_EINVAL, "attn_shapes: flags=0x%x, known bits are TMIX_SHAPE_FILL_HOLES | TMIX_SHAPE_RESOLVE", (unsigned)flags);
    if (h < 1 || w < 1 || n_sets < 1 || km1 < 1 || (int64_t)n_sets * km1 > 65535 || (int64_t)h * w > TMIX_SHAPE_MAX_PIXELS)
        TMIX_FAIL(TMIX_ESHAPE, "attn_shapes: n_sets=%d km1=%d (each >= 1, n_sets * km1 <= 65535) grid %d x %d (each side >= 1, h * w <= %d)", n_sets,
                  km1, h, w, TMIX_SHAPE_MAX_PIXELS);
    const int px = h * w, smem = 2 * px * 4 + 2 * ((px + 31) / 32) * 4;
    static int attr_smem = 0;
    if (int rc = raise_lds_limit((const void*)attn_shape_kernel, &attr_smem, smem)) return rc;
    attn_shape_kernel<<<(unsigned)(n_sets * km1), SHAPE_THREADS, smem, (hipStream_t)stream>>>(score, out, h, w, threshold,
                                                                                               (flags & TMIX_SHAPE_FILL_HOLES) != 0);
    TMIX_LAUNCH_CHECK();
    if ((flags & TMIX_SHAPE_RESOLVE) && km1 > 1) {
        const int64_t hw = px, total = (int64_t)n_sets * hw;
        int64_t blocks = (total + 255) / 256; if (blocks > 2048) blocks = 2048;
        attn_resolve_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(score, out, km1, hw, total);
        TMIX_LAUNCH_CHECK();
    }
    return TMIX_OK;
}
