// tweedie_step.hip -- fused CFG + Tweedie x0 + mask blend + DDIM update (one HBM pass).
// Follows fusion_generation/fusion_sampling.py:376-385,392-403,406-412,424-430,471-472.
// HBM-bound: per element it reads (rows) eps values + x + K mask values and writes 1-2 floats.
// Compiled with -ffp-contract=off so fp32 results are bit-identical to the numpy oracle.  The x0 of an element, the fp16 rounding point and the
// argument checks of the *_dev entries are step_core.h's, shared with solver_step.hip.  The image sampler's kernels and entries only: the video
// sampler's step is video_step.hip.
#include "step_core.h"

namespace {

// DEV = 1: the step coefficients come from a device buffer prm = {t, sa, s1, sa_next, s1_next, is_last, g} (so ONE captured
// launch serves every timestep of a hipGraph replay) and blockIdx.y walks co-batched seeds (x / out: [seeds][n], eps:
// [seeds][rows][n], masks: [seeds][K][hw] or shared).  x may alias out_x: element i is read before it is written.
// KEEP (with DEV): a region of the latent is held at a given clean latent kp.x0 re-noised with its own fixed noise kp.eps to the level
// of the state the step writes; kp.w [hw] (broadcast over the channels) is the weight of the held part.  Seed sd reads its arrays at
// sd * stride (0: shared by all seeds).  The mode's x0 / moved are computed exactly as without it.  The flag is the presence of ONE
// trailing KeepArgs kernel argument (the pack KeepT is empty or {KeepArgs}): without it the kernel has the arguments it had before the keep
// region existed.
struct KeepArgs { const float* x0; const float* eps; const float* w; int64_t x0_stride, eps_stride, w_stride; };
__device__ __forceinline__ KeepArgs keep_args(const KeepArgs& k) { return k; }
// RESCALE (with DEV; the same mechanism, the other type of the ONE trailing argument): step_core.h's RescaleArgs.  The move's noise term stays the
// unconditional eu.
template <typename A, typename... T> constexpr bool pack_is = sizeof...(T) == 1 && (__is_same(T, A) && ...);

template <int DT, int MODE, int DEV = 0, typename... KeepT>
__global__ void __launch_bounds__(256)
tweedie_step_kernel(const float* x, const typename EpsT<DT>::T* __restrict__ eps,
                    const float* __restrict__ masks, float* out_x, float* __restrict__ out_x0,
                    int K, int64_t n, int64_t hw, float g, float sa, float s1, float sa_n, float s1_n, int is_last,
                    const float* __restrict__ prm = nullptr, int rows = 0, int64_t mask_seed_stride = 0, KeepT... keep) {
    constexpr bool KEEP = pack_is<KeepArgs, KeepT...>, RS = pack_is<RescaleArgs, KeepT...>;
    static_assert(sizeof...(KeepT) == 0 || ((KEEP || RS) && DEV), "the keep region and the rescale factors exist in the device-parameter form only");
    KeepArgs kp = {};
    if constexpr (KEEP) kp = keep_args(keep...);
    const float* fac = nullptr;
    if constexpr (RS) fac = rescale_args(keep...).fac;
    if constexpr (DEV) {
        sa = prm[1]; s1 = prm[2]; sa_n = prm[3]; s1_n = prm[4]; is_last = prm[5] != 0.0f; g = prm[6];
        const int64_t sd = blockIdx.y;
        x += sd * n; out_x += sd * n; eps += sd * rows * n; masks += sd * mask_seed_stride;
        if (out_x0) out_x0 += sd * n;
        if constexpr (KEEP) { kp.x0 += sd * kp.x0_stride; kp.eps += sd * kp.eps_stride; kp.w += sd * kp.w_stride; }
        if constexpr (RS) fac += sd * (rows - 1);
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = x[i];
        const float eu = EpsT<DT>::ld(eps, i);
        const float x0 = blended_x0<DT, MODE, RS>(eps, masks, fac, K, n, hw, i, xv, eu, g, sa, s1);
        const float moved = sa_n * x0 + rnd<DT>(s1_n * eu);
        if constexpr (KEEP) {   // fp32, two products and one sum each (-ffp-contract=off); w in {0, 1} gives exactly kept or exactly new
            const float kx = kp.x0[i], w = kp.w[i % hw];
            const float kept = is_last ? kx : sa_n * kx + s1_n * kp.eps[i];
            const float nw = is_last ? x0 : moved;
            out_x[i] = w * kept + (1.0f - w) * nw;
            if (out_x0) out_x0[i] = w * kx + (1.0f - w) * x0;
        } else {
            out_x[i] = is_last ? x0 : moved;
            if (out_x0) out_x0[i] = x0;
        }
    }
}

// the coefficients of the scalar form (DEV = 0); the device-parameter forms leave them at these values and the kernel reads prm instead
struct HostCoef { float g = 0.f, sa = 1.f, s1 = 0.f, sa_n = 1.f, s1_n = 0.f; int is_last = 0; };

template <int DT, int DEV, typename... ExtraT>      // ExtraT: empty, or the one trailing kernel argument (KeepArgs or RescaleArgs)
int launch(const float* x, const void* eps, const float* masks, int64_t mss, float* out_x, float* out_x0, int K, int64_t n, int64_t hw, int mode,
           const HostCoef& c, int rows, int seeds, const float* prm, hipStream_t st, const ExtraT&... extra) {
    int64_t bx = (n + 255) / 256; if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, (unsigned)seeds);
    auto go = [&](auto m) {
        tweedie_step_kernel<DT, m(), DEV, ExtraT...><<<grid, 256, 0, st>>>(x, (const typename EpsT<DT>::T*)eps, masks, out_x, out_x0, K, n, hw, c.g, c.sa, c.s1,
                                                                           c.sa_n, c.s1_n, c.is_last, prm, rows, mss, extra...);
    };
    switch (mode) {
    case TMIX_STEP_FUSION: go(std::integral_constant<int, TMIX_STEP_FUSION>()); break;
    case TMIX_STEP_PLAIN:  go(std::integral_constant<int, TMIX_STEP_PLAIN>()); break;
    default:               go(std::integral_constant<int, TMIX_STEP_RESAMPLE>()); break;
    }
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// head of a captured denoising step: every seed's latent is broadcast over its UNet batch rows and the timestep
// (prm[0]) is written to the UNet's per-row timestep input -- fusion_sampling.py:324-327,336 (`latent_model_input`, `t`)
__global__ void __launch_bounds__(256)
step_prologue_kernel(const float* __restrict__ x, float* __restrict__ latent, float* __restrict__ t_dev,
                     const float* __restrict__ prm, int rows, int64_t n) {
    const int64_t sd = blockIdx.y;
    const float4* src = (const float4*)(x + sd * n);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        for (int r = 0; r < rows; ++r) ((float4*)(latent + (sd * rows + r) * n))[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < rows) t_dev[sd * rows + threadIdx.x] = prm[0];
}

}  // namespace

extern "C" int tmix_fused_tweedie_step(const float* x, const void* eps, int eps_dtype, const float* masks,
                                       float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode,
                                       float g, float sa, float s1, float sa_next, float s1_next, int is_last,
                                       void* stream) {
    if (!x || !eps || !out_x) TMIX_FAIL(TMIX_EINVAL, "tweedie_step: null pointer");
    if (mode < TMIX_STEP_FUSION || mode > TMIX_STEP_RESAMPLE) TMIX_FAIL(TMIX_EINVAL, "tweedie_step: bad mode %d", mode);
    if (mode == TMIX_STEP_FUSION && (!masks || K < 1)) TMIX_FAIL(TMIX_EINVAL, "tweedie_step: FUSION needs masks and K>=1");
    if (mode == TMIX_STEP_RESAMPLE && K < 1) TMIX_FAIL(TMIX_EINVAL, "tweedie_step: RESAMPLE needs K>=1");
    if (channels < 1 || hw < 1) TMIX_FAIL(TMIX_ESHAPE, "tweedie_step: empty latent (channels=%d hw=%lld)", channels, (long long)hw);
    if (!(sa > 0.0f)) TMIX_FAIL(TMIX_EINVAL, "tweedie_step: sqrt(alpha) must be > 0");
    const HostCoef c = {g, sa, s1, sa_next, s1_next, is_last};
    return for_dtype(eps_dtype, "tweedie_step", "eps dtype", [&](auto dt) {
        return launch<dt(), 0>(x, eps, masks, 0, out_x, out_x0, K, (int64_t)channels * hw, hw, mode, c, 0, 1, nullptr, (hipStream_t)stream);
    });
}

extern "C" int tmix_fused_tweedie_step_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                           int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                           int64_t hw, int mode, int rows, int seeds, const float* params, void* stream) {
    const char* me = "tweedie_step_dev";
    if (int rc = check_dev_step(me, true, false, x, eps, out_x, params, nullptr, nullptr, masks, K, channels, hw, mode, rows, seeds)) return rc;
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch<dt(), 1>(x, eps, masks, mask_seed_stride, out_x, out_x0, K, (int64_t)channels * hw, hw, mode, HostCoef(), rows, seeds, params, (hipStream_t)stream);
    });
}

extern "C" int tmix_fused_tweedie_step_keep_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                                int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                                int64_t hw, int mode, int rows, int seeds, const float* params,
                                                const float* keep_x0, int64_t keep_x0_seed_stride, const float* keep_eps,
                                                int64_t keep_eps_seed_stride, const float* keep_w, int64_t keep_w_seed_stride, void* stream) {
    const char* me = "tweedie_step_keep_dev";
    const char* missing = keep_x0 && keep_eps && keep_w ? nullptr : "null keep pointer";
    if (int rc = check_dev_step(me, true, false, x, eps, out_x, params, nullptr, missing, masks, K, channels, hw, mode, rows, seeds)) return rc;
    const int64_t n = (int64_t)channels * hw;
    if ((keep_x0_seed_stride != 0 && keep_x0_seed_stride < n) || (keep_eps_seed_stride != 0 && keep_eps_seed_stride < n) ||
        (keep_w_seed_stride != 0 && keep_w_seed_stride < hw))
        TMIX_FAIL(TMIX_ESHAPE, "tweedie_step_keep_dev: keep seed strides %lld / %lld / %lld: 0 (shared) or >= %lld / %lld / %lld floats",
                  (long long)keep_x0_seed_stride, (long long)keep_eps_seed_stride, (long long)keep_w_seed_stride, (long long)n, (long long)n, (long long)hw);
    const KeepArgs kp = {keep_x0, keep_eps, keep_w, keep_x0_seed_stride, keep_eps_seed_stride, keep_w_seed_stride};
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch<dt(), 1>(x, eps, masks, mask_seed_stride, out_x, out_x0, K, n, hw, mode, HostCoef(), rows, seeds, params, (hipStream_t)stream, kp);
    });
}

extern "C" int tmix_fused_tweedie_step_rs_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                              int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                              int64_t hw, int mode, int rows, int seeds, const float* params, const float* factors, void* stream) {
    const char* me = "tweedie_step_rs_dev";
    if (int rc = check_dev_step(me, true, false, x, eps, out_x, params, nullptr, factors ? nullptr : "null factors", masks, K, channels, hw, mode, rows, seeds)) return rc;
    const RescaleArgs rs = {factors};
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch<dt(), 1>(x, eps, masks, mask_seed_stride, out_x, out_x0, K, (int64_t)channels * hw, hw, mode, HostCoef(), rows, seeds, params, (hipStream_t)stream, rs);
    });
}

extern "C" int tmix_step_prologue(const float* x, float* latent, float* t_dev, const float* params, int seeds, int rows,
                                  int64_t n, void* stream) {
    if (!x || !latent || !t_dev || !params) TMIX_FAIL(TMIX_EINVAL, "step_prologue: null pointer");
    if (seeds < 1 || seeds > 65535 || rows < 1 || rows > 256 || n < 4 || (n & 3)) TMIX_FAIL(TMIX_ESHAPE, "step_prologue: seeds=%d rows=%d n=%lld (n %% 4 == 0)", seeds, rows, (long long)n);
    if (!aligned16(x) || !aligned16(latent)) TMIX_FAIL(TMIX_EALIGN, "step_prologue: x / latent must be 16-byte aligned");
    int64_t bx = (n / 4 + 255) / 256; if (bx > 256) bx = 256;
    step_prologue_kernel<<<dim3((unsigned)bx, (unsigned)seeds), 256, 0, (hipStream_t)stream>>>(x, latent, t_dev, params, rows, n);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
