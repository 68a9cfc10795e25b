// solver_step.hip -- fused CFG + Tweedie x0 + mask blend + DPM-Solver++(2M) update on the blended estimate (one HBM pass).
// The x0 part IS tweedie_step.hip's: both kernels call step_core.h's blended_x0, so out_x0 is that kernel's out_x0 bit for bit; the move is the
// data-prediction form x_next = cx x + c0 x0 + c1 x0_prev with the history buffer x0_prev read and rewritten in the same pass.  Per element and
// seed it reads (rows) eps values + x + K mask values + 1 history value and writes 2-3 floats.
// Compiled with -ffp-contract=off so fp32 results are bit-identical to the numpy restatement (solver.multistep_step_reference).
// Second half: the same move for the video sampler's v-prediction step (tmix_vpred_step_ms / _ms_dev; solver.vpred_multistep_reference).
#include "step_core.h"

namespace {

// prm = {t, sa, s1, cx, c0, c1, is_last, g} in device memory (one captured launch serves every timestep and both orders); blockIdx.y walks
// co-batched seeds (x / out_x / out_x0 / x0_prev: [seeds][n], eps: [seeds][rows][n], masks: [seeds][K][hw] or shared).  x may alias out_x:
// every array is read at i before it is written at i.  x0_prev is read AND written, so it carries no __restrict__.
// RESCALE: the presence of ONE trailing RescaleArgs kernel argument (step_core.h; the pack RsT is empty or {RescaleArgs}, tweedie_step.hip's KeepArgs
// mechanism); without it the kernel has the arguments it had before.
template <int DT, int MODE, typename... RsT>
__global__ void __launch_bounds__(256)
solver_step_kernel(const float* x, const typename EpsT<DT>::T* __restrict__ eps, const float* __restrict__ masks, float* out_x,
                   float* __restrict__ out_x0, float* x0_prev, int K, int64_t n, int64_t hw, const float* __restrict__ prm, int rows,
                   int64_t mask_seed_stride, RsT... rs) {
    constexpr bool RS = sizeof...(RsT) != 0;
    const float* fac = nullptr;
    if constexpr (RS) fac = rescale_args(rs...).fac + (int64_t)blockIdx.y * (rows - 1);
    const float sa = prm[1], s1 = prm[2], cx = prm[3], c0 = prm[4], c1 = prm[5], g = prm[7];
    const bool is_last = prm[6] != 0.0f;
    const int64_t sd = blockIdx.y;
    x += sd * n; out_x += sd * n; x0_prev += sd * n; eps += sd * rows * n; masks += sd * mask_seed_stride;
    if (out_x0) out_x0 += sd * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = x[i];
        const float p = x0_prev[i];
        const float eu = EpsT<DT>::ld(eps, i);
        const float x0 = blended_x0<DT, MODE, RS>(eps, masks, fac, K, n, hw, i, xv, eu, g, sa, s1);
        float m = c0 * x0;
        if (c1 != 0.0f) m = m + c1 * p;          // a first-order step never touches the history value: a NaN left there stays out
        out_x[i] = is_last ? x0 : cx * xv + m;
        x0_prev[i] = x0;
        if (out_x0) out_x0[i] = x0;
    }
}

template <int DT, typename... RsT>      // RsT: empty, or {RescaleArgs}
int launch_ms(const float* x, const void* eps, const float* masks, int64_t mss, float* out_x, float* out_x0, float* x0_prev, int K, int64_t n,
              int64_t hw, int mode, int rows, int seeds, const float* prm, hipStream_t st, RsT... rs) {
    typedef typename EpsT<DT>::T T;
    int64_t bx = (n + 255) / 256; if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, (unsigned)seeds);
    const T* e = (const T*)eps;
    if (mode == TMIX_STEP_FUSION)
        solver_step_kernel<DT, TMIX_STEP_FUSION, RsT...><<<grid, 256, 0, st>>>(x, e, masks, out_x, out_x0, x0_prev, K, n, hw, prm, rows, mss, rs...);
    else
        solver_step_kernel<DT, TMIX_STEP_PLAIN, RsT...><<<grid, 256, 0, st>>>(x, e, masks, out_x, out_x0, x0_prev, K, n, hw, prm, rows, mss, rs...);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// ------------------------------------------------------------------ video sampler (I2VGen-XL loop): the same move on the v-prediction
// StT<DT>::st, video_row_offset and the element's x0 (vpred_x0) are step_core.h's, shared with the DDIM forms in tweedie_step.hip

// one element of the v-prediction solver step, shared by the scalar and the device form (so the two agree bit for bit): x0 is vpred_x0's, as in
// tweedie_step.hip's vpred_step_kernel; the history value p is used only when c1 != 0 (a NaN left in an unused history stays out); returns the
// moved state, x0 through the reference
// RS: the guided prediction is rescaled by the video's factor f inside vpred_x0; this move has no eps term
template <int DT, bool RS = false>
__device__ __forceinline__ float vpred_ms_element(float xv, float vu, float vc, float p, float g, float sa, float s1, float cx, float c0, float c1,
                                                  float& x0, float f = 1.0f) {
    x0 = vpred_x0<DT, RS>(xv, vu, vc, g, sa, s1, f).x0;
    float m = rnd<DT>(c0 * x0);
    if (c1 != 0.0f) m = rnd<DT>(m + rnd<DT>(c1 * p));
    return rnd<DT>(rnd<DT>(cx * xv) + m);
}

// x, v [2n] (uncond rows first), out of the model dtype; x0_prev [n] fp32, read and rewritten.  out may alias x: element i of every array is read
// before it is written, so neither carries __restrict__.  RESCALE: ONE trailing RescaleArgs argument (the pack RsT is empty or {RescaleArgs}, as in
// solver_step_kernel); element i then uses fac[i / per], the factor of its video.
template <int DT, typename... RsT>
__global__ void __launch_bounds__(256)
vpred_step_ms_kernel(const typename EpsT<DT>::T* x, const typename EpsT<DT>::T* __restrict__ v, typename EpsT<DT>::T* out, float* __restrict__ x0_prev,
                     int64_t n, float g, float sa, float s1, float cx, float c0, float c1, RsT... rs) {
    constexpr bool RS = sizeof...(RsT) != 0;
    RescaleArgs ra = {};
    if constexpr (RS) ra = rescale_args(rs...);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = EpsT<DT>::ld(x, i);
        const float p = x0_prev[i];
        float x0, f = 1.0f;
        if constexpr (RS) f = ra.fac[i / ra.per];
        const float o = vpred_ms_element<DT, RS>(xv, EpsT<DT>::ld(v, i), EpsT<DT>::ld(v, n + i), p, g, sa, s1, cx, c0, c1, x0, f);
        StT<DT>::st(out, i, o);
        x0_prev[i] = x0;
    }
}

// vpred_step_ms_kernel<TMIX_F32> for S videos, in place on x [S][C][F][hw], with prm = {t, sa, s1, cx, c0, c1, g, 0} in device memory (one captured
// launch serves every timestep and both orders) and v_u / v_c read from the plans' prediction rows.  RsT: as above; the video is the outermost index of i.
template <typename... RsT>
__global__ void __launch_bounds__(256)
vpred_step_ms_dev_kernel(float* __restrict__ x, const float* __restrict__ vu, int64_t su, const float* __restrict__ vc, int64_t sc,
                         float* __restrict__ x0_prev, const float* __restrict__ prm, int C, int F, int64_t hw, int64_t n, RsT... rs) {
    constexpr bool RS = sizeof...(RsT) != 0;
    RescaleArgs ra = {};
    if constexpr (RS) ra = rescale_args(rs...);
    const float sa = prm[1], s1 = prm[2], cx = prm[3], c0 = prm[4], c1 = prm[5], g = prm[6];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = x[i];
        const float p = x0_prev[i];
        float x0, f = 1.0f;
        if constexpr (RS) f = ra.fac[i / ra.per];
        x[i] = vpred_ms_element<TMIX_F32, RS>(xv, vu[video_row_offset(i, C, F, hw, C, su)], vc[video_row_offset(i, C, F, hw, C, sc)], p, g, sa, s1, cx, c0, c1, x0, f);
        x0_prev[i] = x0;
    }
}

template <int DT, typename... RsT>      // RsT: empty, or {RescaleArgs}
int launch_vpred_ms(const void* x, const void* v, void* out, float* x0_prev, int64_t n, float g, float sa, float s1, float cx, float c0, float c1,
                    hipStream_t st, RsT... rs) {
    typedef typename EpsT<DT>::T T;
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    vpred_step_ms_kernel<DT, RsT...><<<(unsigned)blocks, 256, 0, st>>>((const T*)x, (const T*)v, (T*)out, x0_prev, n, g, sa, s1, cx, c0, c1, rs...);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

template <typename... RsT>              // the device-parameter form
int launch_vpred_ms_dev(float* x, const float* vu, int64_t su, const float* vc, int64_t sc, float* x0_prev, const float* prm, int videos, int C, int F,
                        int64_t hw, hipStream_t st, RsT... rs) {
    const int64_t n = (int64_t)videos * F * C * hw;
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    vpred_step_ms_dev_kernel<RsT...><<<(unsigned)blocks, 256, 0, st>>>(x, vu, su, vc, sc, x0_prev, prm, C, F, hw, n, rs...);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

}  // namespace

extern "C" int tmix_vpred_step_ms(const void* x, const void* v, void* out, float* x0_prev, int dtype, int64_t n, float g,
                                  float sa, float s1, float cx, float c0, float c1, void* stream) {
    if (!x || !v || !out) TMIX_FAIL(TMIX_EINVAL, "vpred_step_ms: null pointer");
    if (!x0_prev) TMIX_FAIL(TMIX_EINVAL, "vpred_step_ms: null x0_prev (the history buffer is read and written by every step)");
    if (dtype != TMIX_F32 && dtype != TMIX_F16 && dtype != TMIX_BF16) TMIX_FAIL(TMIX_EINVAL, "vpred_step_ms: bad dtype %d", dtype);
    if (n < 1) TMIX_FAIL(TMIX_ESHAPE, "vpred_step_ms: empty latent");
    return for_dtype(dtype, "vpred_step_ms", "dtype", [&](auto dt) { return launch_vpred_ms<dt()>(x, v, out, x0_prev, n, g, sa, s1, cx, c0, c1, (hipStream_t)stream); });
}

extern "C" int tmix_vpred_step_ms_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                                      const float* params, int videos, int channels, int frames, int64_t hw, void* stream) {
    if (!x || !v_u || !v_c || !params) TMIX_FAIL(TMIX_EINVAL, "vpred_step_ms_dev: null pointer");
    if (!x0_prev) TMIX_FAIL(TMIX_EINVAL, "vpred_step_ms_dev: null x0_prev (the history buffer is read and written by every step)");
    if (int rc = check_video_step("vpred_step_ms_dev", videos, channels, frames, hw, channels, false, clip_stride_u, clip_stride_c)) return rc;
    return launch_vpred_ms_dev(x, v_u, clip_stride_u, v_c, clip_stride_c, x0_prev, params, videos, channels, frames, hw, (hipStream_t)stream);
}

// tmix_vpred_step_ms / tmix_vpred_step_ms_dev with the guided prediction rescaled per video: factors [videos] from tmix_vpred_rescale_factors
extern "C" int tmix_vpred_step_ms_rs(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t n_per_video, float g,
                                     float sa, float s1, float cx, float c0, float c1, const float* factors, void* stream) {
    const char* me = "vpred_step_ms_rs";
    if (!x || !v || !out) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (!x0_prev) TMIX_FAIL(TMIX_EINVAL, "%s: null x0_prev (the history buffer is read and written by every step)", me);
    if (!factors) TMIX_FAIL(TMIX_EINVAL, "%s: null factors", me);
    if (int rc = check_video_step(me, videos, 1, 1, n_per_video, 1, false, n_per_video, n_per_video)) return rc;
    const RescaleArgs rs = {factors, n_per_video};
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        return launch_vpred_ms<dt()>(x, v, out, x0_prev, (int64_t)videos * n_per_video, g, sa, s1, cx, c0, c1, (hipStream_t)stream, rs);
    });
}

extern "C" int tmix_vpred_step_ms_rs_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                                         const float* params, int videos, int channels, int frames, int64_t hw, const float* factors, void* stream) {
    const char* me = "vpred_step_ms_rs_dev";
    if (!x || !v_u || !v_c || !params) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (!x0_prev) TMIX_FAIL(TMIX_EINVAL, "%s: null x0_prev (the history buffer is read and written by every step)", me);
    if (!factors) TMIX_FAIL(TMIX_EINVAL, "%s: null factors", me);
    if (int rc = check_video_step(me, videos, channels, frames, hw, channels, false, clip_stride_u, clip_stride_c)) return rc;
    const RescaleArgs rs = {factors, (int64_t)channels * frames * hw};
    return launch_vpred_ms_dev(x, v_u, clip_stride_u, v_c, clip_stride_c, x0_prev, params, videos, channels, frames, hw, (hipStream_t)stream, rs);
}

extern "C" int tmix_fused_tweedie_step_ms_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                              int64_t mask_seed_stride, float* out_x, float* out_x0, float* x0_prev, int K, int channels,
                                              int64_t hw, int mode, int rows, int seeds, const float* params, void* stream) {
    const char* me = "tweedie_step_ms_dev";
    if (int rc = check_dev_step(me, false, true, x, eps, out_x, params, x0_prev, nullptr, masks, K, channels, hw, mode, rows, seeds)) return rc;
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, (int64_t)channels * hw, hw, mode, rows, seeds, params, (hipStream_t)stream);
    });
}

extern "C" int tmix_fused_tweedie_step_ms_rs_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                                 int64_t mask_seed_stride, float* out_x, float* out_x0, float* x0_prev, int K, int channels,
                                                 int64_t hw, int mode, int rows, int seeds, const float* params, const float* factors, void* stream) {
    const char* me = "tweedie_step_ms_rs_dev";
    if (int rc = check_dev_step(me, false, true, x, eps, out_x, params, x0_prev, factors ? nullptr : "null factors", masks, K, channels, hw, mode, rows, seeds)) return rc;
    const RescaleArgs rs = {factors};
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, (int64_t)channels * hw, hw, mode, rows, seeds, params, (hipStream_t)stream, rs);
    });
}
