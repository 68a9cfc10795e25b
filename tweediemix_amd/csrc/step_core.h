// step_core.h -- the ONE definition of what the sampler's step kernels share (tweedie_step.hip: the image sampler's DDIM forms, solver_step.hip: its
// DPM-Solver++(2M) forms, video_step.hip: the video sampler's step, cfg_rescale.hip: the statistics of the guided prediction).  Device side: element
// types, the fp16 rounding point, CFG, the blended Tweedie x0 of one element, the v-prediction element of the video sampler and its two moves.  Host
// side: the argument checks of the *_dev image entries and of the video entries, and the dtype dispatch.  Every file that includes it is compiled with
// -ffp-contract=off: the kernels that call one function here agree bit for bit because they run the same operations, not because two copies were kept alike.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

template <int DT> struct EpsT;
template <> struct EpsT<TMIX_F32>  { typedef float  T; static __device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; } };
template <> struct EpsT<TMIX_F16>  { typedef __half T; static __device__ __forceinline__ float ld(const __half* p, int64_t i) { return __half2float(p[i]); } };
template <> struct EpsT<TMIX_BF16> { typedef bf16_t T; static __device__ __forceinline__ float ld(const bf16_t* p, int64_t i) { return bf2f(p[i]); } };
// store of an fp32 value as the element type of TMIX_F32 / TMIX_F16 / TMIX_BF16 (one rounding to nearest even)
template <int DT> struct StT;
template <> struct StT<TMIX_F32>  { static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; } };
template <> struct StT<TMIX_F16>  { static __device__ __forceinline__ void st(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); } };
template <> struct StT<TMIX_BF16> { static __device__ __forceinline__ void st(bf16_t* p, int64_t i, float v) { p[i] = f2bf(v); } };

// rounding point of the reference's autocast path (only when eps is fp16)
template <int DT> __device__ __forceinline__ float rnd(float v) {
    if constexpr (DT == TMIX_F16) {
        // torch evaluates fp16 elementwise ops in fp32 and rounds the fp32 RESULT to fp16 (two roundings).
        // The empty asm makes the fp32 value opaque so LLVM cannot fold mul+convert into the single-rounding
        // v_fma_mixlo_f16, which differs from the reference on near-ties.
        asm volatile("" : "+v"(v));
        return __half2float(__float2half_rn(v));
    } else return v;
}

template <int DT> __device__ __forceinline__ float cfg(float eu, float ec, float g) {
    const float d = rnd<DT>(ec - eu);
    const float gd = rnd<DT>(g * d);
    return rnd<DT>(eu + gd);
}

// RESCALE: every guided prediction e_r a step kernel forms becomes rnd<DT>(f_r * e_r) with f_r = fac[seed][r - 1] (layout [seeds][rows - 1];
// tmix_cfg_rescale_factors writes it: DESIGN.md 7k).  f_r = 1.0f gives e_r back bit for bit.  The flag is the presence of ONE trailing
// RescaleArgs kernel argument: without it a kernel has the arguments it had before the rescale existed.
// The video step kernels read fac[i / per]: one factor per video of `per` elements (tmix_vpred_rescale_factors); the image kernels
// leave per at 0 and never read it.
struct RescaleArgs { const float* fac; int64_t per = 0; };
__device__ __forceinline__ RescaleArgs rescale_args(const RescaleArgs& r) { return r; }

// The blended Tweedie estimate of element i, the x0 of EVERY fused step (fusion_sampling.py:376-385,392-403,406-412): CFG per eps row, the rescale
// (RS), x0 per row, then the mask blend (FUSION), the one row (PLAIN) or (K-1)*x0_multi - sum_{c<K-1} x0_single_c (RESAMPLE).  eps / masks / fac are
// the seed's own; xv = x[i], eu = the unconditional row's value at i.
// COND (the unguided step; FUSION and PLAIN): eps has NO unconditional row -- row c is concept c's (PLAIN: row 0 the scene prompt's) -- and
// e_c is the row's prediction itself: no CFG, no factor; eu, g and fac are not read.  Everything behind e_c is the same operations in the same order.
template <int DT, int MODE, bool RS, bool COND = false>
__device__ __forceinline__ float blended_x0(const typename EpsT<DT>::T* eps, const float* masks, const float* fac, int K, int64_t n, int64_t hw,
                                            int64_t i, float xv, float eu, float g, float sa, float s1) {
    float x0;
    if constexpr (MODE == TMIX_STEP_FUSION) {
        const int64_t p = i % hw;
        x0 = 0.0f;
        for (int c = 0; c < K; ++c) {
            float e;
            if constexpr (COND) e = EpsT<DT>::ld(eps, (int64_t)c * n + i);
            else e = cfg<DT>(eu, EpsT<DT>::ld(eps, (int64_t)(1 + c) * n + i), g);
            if constexpr (RS) e = rnd<DT>(fac[c] * e);
            const float t = (xv - rnd<DT>(s1 * e)) / sa;
            x0 = x0 + masks[(int64_t)c * hw + p] * t;
        }
    } else if constexpr (MODE == TMIX_STEP_PLAIN) {
        float e;
        if constexpr (COND) e = EpsT<DT>::ld(eps, i);
        else e = cfg<DT>(eu, EpsT<DT>::ld(eps, n + i), g);
        if constexpr (RS) e = rnd<DT>(fac[0] * e);
        x0 = (xv - rnd<DT>(s1 * e)) / sa;
    } else {
        static_assert(!COND, "the unguided step has no RESAMPLE form");
        float em = cfg<DT>(eu, EpsT<DT>::ld(eps, n + i), g);
        if constexpr (RS) em = rnd<DT>(fac[0] * em);
        x0 = (float)(K - 1) * ((xv - rnd<DT>(s1 * em)) / sa);
        for (int c = 0; c < K - 1; ++c) {
            float e = cfg<DT>(eu, EpsT<DT>::ld(eps, (int64_t)(2 + c) * n + i), g);
            if constexpr (RS) e = rnd<DT>(fac[1 + c] * e);
            x0 = x0 - (xv - rnd<DT>(s1 * e)) / sa;
        }
    }
    return x0;
}

// APG (adaptive projected guidance, arXiv:2410.02416): guidance formed on the rows' Tweedie estimates.  With tc / tu the conditional /
// unconditional estimate of a row's element and d = tc - tu, the row's estimate is t_r = A_r tc + B_r d, {A_r, B_r} = ab[2 (r - 1)], ab[2 (r - 1) + 1]
// (layout [seeds][rows - 1][2]; tmix_apg_coeffs writes it from the row's sums of d d, d tc and tc tc).  {1, g - 1} is plain CFG in data space.
// The flag is the presence of ONE trailing ApgArgs kernel argument (in front of a NoiseArgs; never with a RescaleArgs or a CondArgs).
struct ApgArgs { const float* ab; };
struct ApgTerm { float tc, d; };
// tu, once per element, and {tc, d} of one conditional row: the operations of blended_x0's t on the row's own prediction.  The ONE definition of
// what the statistics (cfg_rescale.hip) sum and the step kernel combines.
template <int DT> __device__ __forceinline__ float apg_tu(float xv, float eu, float sa, float s1) { return (xv - rnd<DT>(s1 * eu)) / sa; }
template <int DT> __device__ __forceinline__ ApgTerm apg_term(float xv, float tu, float ec, float sa, float s1) {
    const float tc = (xv - rnd<DT>(s1 * ec)) / sa;
    return {tc, tc - tu};
}
__device__ __forceinline__ float apg_row(const ApgTerm& t, const float* ab) { return ab[0] * t.tc + ab[1] * t.d; }     // two products, one sum

// blended_x0 with t_r in the place of every row's t: the same blend (FUSION), row (PLAIN) or (K-1) t_1 - sum_{c<K-1} t_{2+c} (RESAMPLE) behind it.
// ab is the seed's own; g is not read here (it is inside B).
template <int DT, int MODE>
__device__ __forceinline__ float blended_x0_apg(const typename EpsT<DT>::T* eps, const float* masks, const float* ab, int K, int64_t n, int64_t hw,
                                                int64_t i, float xv, float eu, float sa, float s1) {
    const float tu = apg_tu<DT>(xv, eu, sa, s1);
    float x0;
    if constexpr (MODE == TMIX_STEP_FUSION) {
        const int64_t p = i % hw;
        x0 = 0.0f;
        for (int c = 0; c < K; ++c) {
            const float t = apg_row(apg_term<DT>(xv, tu, EpsT<DT>::ld(eps, (int64_t)(1 + c) * n + i), sa, s1), ab + 2 * c);
            x0 = x0 + masks[(int64_t)c * hw + p] * t;
        }
    } else if constexpr (MODE == TMIX_STEP_PLAIN) {
        x0 = apg_row(apg_term<DT>(xv, tu, EpsT<DT>::ld(eps, n + i), sa, s1), ab);
    } else {
        x0 = (float)(K - 1) * apg_row(apg_term<DT>(xv, tu, EpsT<DT>::ld(eps, n + i), sa, s1), ab);
        for (int c = 0; c < K - 1; ++c)
            x0 = x0 - apg_row(apg_term<DT>(xv, tu, EpsT<DT>::ld(eps, (int64_t)(2 + c) * n + i), sa, s1), ab + 2 * (1 + c));
    }
    return x0;
}

// ---- video sampler (I2VGen-XL loop): video_gen/pipeline_i2vgen_xl.py:699-719.  Latents and predictions share the model dtype in that loop, so in
// fp16 mode EVERY binary op rounds (rnd<DT>).
// one element's guided v-prediction and the x0 it gives: what the DDIM and the multistep video kernels have in common.  RS: the guided prediction
// is rescaled, v'' = rnd<DT>(f * v'), before ANYTHING uses it -- x0 here and, through VPred::vv, the eps of vpred_ddim_move (in the video loop both
// come from the one model output; the image kernels' move keeps the unconditional row instead).  Without RS f is not read.
struct VPred { float vv, x0; };
template <int DT, bool RS = false> __device__ __forceinline__ VPred vpred_x0(float xv, float vu, float vc, float g, float sa, float s1, float f = 1.0f) {
    float vv = cfg<DT>(vu, vc, g);
    if constexpr (RS) vv = rnd<DT>(f * vv);
    return {vv, rnd<DT>(rnd<DT>(sa * xv) - rnd<DT>(s1 * vv))};
}
// the UNGUIDED element: v'' is the conditional prediction itself -- no CFG, no factor; neither an unconditional value nor g exists
// here, and a -0.0 prediction keeps its sign (cfg(-0, -0, g) gives +0).  Everything behind v'' is the operations above in the same order.
template <int DT> __device__ __forceinline__ VPred vpred_x0(float xv, float vc, float sa, float s1) {
    return {vc, rnd<DT>(rnd<DT>(sa * xv) - rnd<DT>(s1 * vc))};
}
// the DDIM move of that element: eps from (x, v), then sa_n * x0 + s1_n * eps
template <int DT> __device__ __forceinline__ float vpred_ddim_move(float xv, const VPred& p, float sa, float s1, float sa_n, float s1_n) {
    const float eps = rnd<DT>(rnd<DT>(sa * p.vv) + rnd<DT>(s1 * xv));
    return rnd<DT>(rnd<DT>(sa_n * p.x0) + rnd<DT>(s1_n * eps));
}
// the DPM-Solver++(2M) move of that element, x_next = cx x + c0 x0 + c1 x0_prev (no eps term): the history value p is used only when
// c1 != 0, so a NaN left in an unused history stays out of a first-order step
template <int DT> __device__ __forceinline__ float vpred_ms_move(float xv, float x0, float p, float cx, float c0, float c1) {
    float m = rnd<DT>(c0 * x0);
    if (c1 != 0.0f) m = rnd<DT>(m + rnd<DT>(c1 * p));
    return rnd<DT>(rnd<DT>(cx * xv) + m);
}
// index i of the pipeline-layout state [S][C][F][hw] -> offset of (video s, frame f, channel c, pixel p) in a per-row plan buffer
// [(clip*F + f)][row_channels][hw] whose clip s starts at s * clip_stride
__device__ __forceinline__ int64_t video_row_offset(int64_t i, int C, int F, int64_t hw, int row_channels, int64_t clip_stride) {
    const int64_t p = i % hw;
    int64_t r = i / hw;
    const int64_t f = r % F; r /= F;
    const int64_t c = r % C;
    const int64_t s = r / C;
    return s * clip_stride + (f * row_channels + c) * hw + p;
}

// ------------------------------------------------------------------ host side

// f(std::integral_constant<int, DT>()) for dt = TMIX_F32 / TMIX_F16 / TMIX_BF16; any other value: EINVAL, "<me>: bad <word> <dt>"
template <typename F> int for_dtype(int dt, const char* me, const char* word, F&& f) {
    switch (dt) {
    case TMIX_F32:  return f(std::integral_constant<int, TMIX_F32>());
    case TMIX_F16:  return f(std::integral_constant<int, TMIX_F16>());
    case TMIX_BF16: return f(std::integral_constant<int, TMIX_BF16>());
    }
    TMIX_FAIL(TMIX_EINVAL, "%s: bad %s %d", me, word, dt);
}

// The argument checks of the device-parameter step entries (tmix_fused_tweedie_step_dev / _keep_dev / _rs_dev / _ms_dev / _ms_rs_dev / _noise_dev /
// _cond_dev), under the entry's short name `me`.  resample: RESAMPLE is one of the entry's modes (the DDIM forms; the multistep forms take FUSION or PLAIN).
// need_prev: the entry has the history buffer x0_prev, which must not be null.  missing: the entry's complaint about a null pointer of its own
// (factors, the keep arrays), or nullptr when it has none to make; it is reported behind the shared pointers and in front of the mode.
// cond: the entry's eps has no unconditional row (tmix_fused_tweedie_step_cond_dev), so a mode needs one row less.
inline int check_dev_step(const char* me, bool resample, bool need_prev, const void* x, const void* eps, const void* out_x, const void* params,
                          const void* x0_prev, const char* missing, const float* masks, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                          bool cond = false) {
    if (!x || !eps || !out_x || !params) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (need_prev && !x0_prev) TMIX_FAIL(TMIX_EINVAL, "%s: null x0_prev (the history buffer is read and written by every step)", me);
    if (missing) TMIX_FAIL(TMIX_EINVAL, "%s: %s", me, missing);
    if (resample) {
        if (mode < TMIX_STEP_FUSION || mode > TMIX_STEP_RESAMPLE) TMIX_FAIL(TMIX_EINVAL, "%s: bad mode %d", me, mode);
    } else if (mode != TMIX_STEP_FUSION && mode != TMIX_STEP_PLAIN) TMIX_FAIL(TMIX_EINVAL, "%s: bad mode %d (FUSION or PLAIN)", me, mode);
    if (mode == TMIX_STEP_FUSION && (!masks || K < 1)) TMIX_FAIL(TMIX_EINVAL, "%s: FUSION needs masks and K>=1", me);
    if (mode == TMIX_STEP_RESAMPLE && K < 1) TMIX_FAIL(TMIX_EINVAL, "%s: RESAMPLE needs K>=1", me);
    if (channels < 1 || hw < 1 || seeds < 1 || seeds > 65535) TMIX_FAIL(TMIX_ESHAPE, "%s: channels=%d hw=%lld seeds=%d", me, channels, (long long)hw, seeds);
    const int need = (mode == TMIX_STEP_PLAIN ? 2 : K + 1) - (cond ? 1 : 0);
    if (rows < need) TMIX_FAIL(TMIX_ESHAPE, "%s: mode %d needs %d eps rows per seed, got %d", me, mode, need, rows);
    return TMIX_OK;
}

// Shape and clip strides of a batched video entry: the plan rows of a clip hold row_channels >= channels channels (wide_rows: the entry has that
// argument and names it; otherwise the rows hold the state's channels alone) and a clip's stride covers them.
inline int check_video_step(const char* me, int videos, int channels, int frames, int64_t hw, int row_channels, bool wide_rows, int64_t clip_stride_u,
                            int64_t clip_stride_c) {
    if (videos < 1 || channels < 1 || frames < 1 || hw < 1 || row_channels < channels) {
        if (wide_rows) TMIX_FAIL(TMIX_ESHAPE, "%s: videos=%d channels=%d frames=%d hw=%lld row_channels=%d", me, videos, channels, frames, (long long)hw, row_channels);
        TMIX_FAIL(TMIX_ESHAPE, "%s: videos=%d channels=%d frames=%d hw=%lld", me, videos, channels, frames, (long long)hw);
    }
    const int64_t clip = (int64_t)frames * row_channels * hw;
    if (clip_stride_u < clip || clip_stride_c < clip)
        TMIX_FAIL(TMIX_ESHAPE, "%s: clip strides %lld / %lld < one clip's %lld floats", me, (long long)clip_stride_u, (long long)clip_stride_c, (long long)clip);
    return TMIX_OK;
}

// The argument checks of the eight video step entries (tmix_vpred_step[_ms][_rs][_dev]) under the entry's short name `me`.  The codes, the wording
// and the ORDER of the answers are the entries' ABI and differ between them, so the differences are arguments and stay as they are:
// required: none of the entry's own pointers (x, v / v_u, v_c, out / params) is null.  need_prev / need_fac: the entry has x0_prev / factors.
// dtype: the dense forms' element type (the forms on plan rows pass TMIX_F32).  dtype_first: a bad dtype is answered in front of a bad shape
// (tmix_vpred_step_ms alone).  plain_n: the shape is one count n, passed as hw, and its complaint is "empty latent" (the dense forms without the
// rescale); otherwise the shape and the clip strides are check_video_step's (the dense _rs forms pass videos x n_per_video as videos x 1 x 1 x hw).
inline int check_vpred_step(const char* me, bool required, bool need_prev, const void* x0_prev, bool need_fac, const void* factors, int dtype,
                            bool dtype_first, bool plain_n, int videos, int channels, int frames, int64_t hw, int64_t clip_stride_u, int64_t clip_stride_c) {
    if (!required) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (need_prev && !x0_prev) TMIX_FAIL(TMIX_EINVAL, "%s: null x0_prev (the history buffer is read and written by every step)", me);
    if (need_fac && !factors) TMIX_FAIL(TMIX_EINVAL, "%s: null factors", me);
    const bool bad_dtype = dtype != TMIX_F32 && dtype != TMIX_F16 && dtype != TMIX_BF16;
    if (dtype_first && bad_dtype) TMIX_FAIL(TMIX_EINVAL, "%s: bad dtype %d", me, dtype);
    if (plain_n) {
        if (hw < 1) TMIX_FAIL(TMIX_ESHAPE, "%s: empty latent", me);
    } else if (int rc = check_video_step(me, videos, channels, frames, hw, channels, false, clip_stride_u, clip_stride_c)) return rc;
    if (bad_dtype) TMIX_FAIL(TMIX_EINVAL, "%s: bad dtype %d", me, dtype);
    return TMIX_OK;
}

}  // namespace
