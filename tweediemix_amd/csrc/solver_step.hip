// solver_step.hip -- fused CFG + Tweedie x0 + mask blend + DPM-Solver++(2M) update on the blended estimate (one HBM pass).
// The x0 part IS tweedie_step.hip's: both kernels call step_core.h's blended_x0, so out_x0 is that kernel's out_x0 bit for bit; the move is the
// data-prediction form x_next = cx x + c0 x0 + c1 x0_prev with the history buffer x0_prev read and rewritten in the same pass.  Per element and
// seed it reads (rows) eps values + x + K mask values + 1 history value and writes 2-3 floats.
// Compiled with -ffp-contract=off so fp32 results are bit-identical to the numpy restatement (solver.multistep_step_reference).
// The image sampler's kernel and entries only: the same move on the video sampler's v-prediction is video_step.hip's.
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

}  // namespace

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
