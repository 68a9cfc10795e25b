// video_step.hip -- everything the video sampler's step owns (I2VGen-XL loop, video_gen/pipeline_i2vgen_xl.py:699-719): the head of
// the captured step, the first-frame injection, and ONE element kernel behind the eight tmix_vpred_step[_ms][_rs][_dev] entries -- CFG on the
// v-prediction, the optional per-video rescale, x0, then the DDIM move or the DPM-Solver++(2M) move, in one HBM pass.
// The element's operations are step_core.h's (vpred_x0, vpred_ddim_move, vpred_ms_move), so the forms agree bit for bit -- device form with dense form,
// factors of 1.0 with no rescale, the multistep x0 with the DDIM x0 -- because they are one loop.  Compiled with -ffp-contract=off so fp32 results are
// bit-identical to the numpy restatements (guidance.vpred_rescaled_step_reference / vpred_rescaled_multistep_reference).
// The stochastic step (tmix_vpred_step_noise[_dev]) is the same kernel with one trailing VideoNoiseArgs: the move of either solver
// plus cz * z, z from noise.h (noise.vpred_step_reference restates it).
// The hold (tmix_vpred_step_hold[_dev], tmix_video_hold_composite) is the same kernel again with a VideoHoldArgs behind the
// VideoNoiseArgs: the stored value is hold_blend(moved, ...), the held part a clean latent at the written state's noise level under one fixed noise.
// The unguided step of a guidance interval (tmix_video_step_prologue_cond, tmix_vpred_step_cond[_dev]) is the same kernel over a
// COND view: one prediction per element, the conditional one, and no CFG (guidance.vpred_cond_step_reference restates it).
#include "step_core.h"
#include "noise.h"

namespace {

// the coefficients of one step: g, sa, s1 and the move's -- {sa_next, s1_next} (DDIM; c unused) or {cx, c0, c1} (multistep)
struct StepCoef { float g, sa, s1, a, b, c; };

// WHERE the operands of element i live: two views with the same four accessors.
// Dense: x, v [2][n] (uncond rows first, so v_c at n + i) and out of the model dtype, the coefficients by value.  out may alias x in the multistep form
// (element i of every array is read before it is written), so the view both moves share promises nothing about its pointers.
template <int D> struct DenseView {
    static constexpr int DT = D;
    static constexpr bool COND = false;
    typedef typename EpsT<D>::T T;
    const T* x; const T* v; T* out; int64_t n; StepCoef k;
    template <bool MS> __device__ __forceinline__ StepCoef coef() const { return k; }
    __device__ __forceinline__ float xv(int64_t i) const { return EpsT<D>::ld(x, i); }
    __device__ __forceinline__ float vu(int64_t i) const { return EpsT<D>::ld(v, i); }
    __device__ __forceinline__ float vc(int64_t i) const { return EpsT<D>::ld(v, n + i); }
    __device__ __forceinline__ void st(int64_t i, float o) const { StT<D>::st(out, i, o); }
};
// Plan rows: the fp32 state x [S][C][F][hw] updated in place (element i is read before it is written), v_u / v_c read from the plans' prediction rows
// [(clip*F + f)][C][hw] with their clip strides, the coefficients from device memory (one captured launch serves every timestep and both orders):
// prm = {t, sa, s1, sa_next, s1_next, g, 0, 0} for the DDIM move and {t, sa, s1, cx, c0, c1, g, 0} for the multistep move.
struct RowsView {
    static constexpr int DT = TMIX_F32;
    static constexpr bool COND = false;
    float* x; const float* v_u; int64_t su; const float* v_c; int64_t sc; const float* prm; int C, F; int64_t hw;
    template <bool MS> __device__ __forceinline__ StepCoef coef() const { return {prm[MS ? 6 : 5], prm[1], prm[2], prm[3], prm[4], MS ? prm[5] : 0.0f}; }
    __device__ __forceinline__ float xv(int64_t i) const { return x[i]; }
    __device__ __forceinline__ float vu(int64_t i) const { return v_u[video_row_offset(i, C, F, hw, C, su)]; }
    __device__ __forceinline__ float vc(int64_t i) const { return v_c[video_row_offset(i, C, F, hw, C, sc)]; }
    __device__ __forceinline__ void st(int64_t i, float o) const { x[i] = o; }
};
// COND (the unguided step): the same views without an unconditional prediction -- vu does not exist, the kernel takes step_core.h's
// unguided vpred_x0 and reads ONE prediction per element.  Dense: v [videos][per] is the conditional prediction alone; plan rows: the text half's
// prediction rows alone.  The parameter layouts are the parents' (g is still uploaded at slot 5 or 6) and g is not read: coef() leaves it 0.
template <int D> struct DenseCondView {
    static constexpr int DT = D;
    static constexpr bool COND = true;
    typedef typename EpsT<D>::T T;
    const T* x; const T* v; T* out; StepCoef k;
    template <bool MS> __device__ __forceinline__ StepCoef coef() const { return k; }
    __device__ __forceinline__ float xv(int64_t i) const { return EpsT<D>::ld(x, i); }
    __device__ __forceinline__ float vc(int64_t i) const { return EpsT<D>::ld(v, i); }
    __device__ __forceinline__ void st(int64_t i, float o) const { StT<D>::st(out, i, o); }
};
struct RowsCondView {
    static constexpr int DT = TMIX_F32;
    static constexpr bool COND = true;
    float* x; const float* v_c; int64_t sc; const float* prm; int C, F; int64_t hw;
    template <bool MS> __device__ __forceinline__ StepCoef coef() const { return {0.0f, prm[1], prm[2], prm[3], prm[4], MS ? prm[5] : 0.0f}; }
    __device__ __forceinline__ float xv(int64_t i) const { return x[i]; }
    __device__ __forceinline__ float vc(int64_t i) const { return v_c[video_row_offset(i, C, F, hw, C, sc)]; }
    __device__ __forceinline__ void st(int64_t i, float o) const { x[i] = o; }
};

// NOISE: the presence of ONE trailing VideoNoiseArgs kernel argument (the mechanism of solver_step.hip's NoiseArgs); without it a kernel has the
// arguments it had before the noise existed.  Element i of video s = i / per takes z of (index i % per, keys[s], step, NOISE_STREAM_VIDEO_STEP):
// its own linear index in its video's [C][F][hw] layout under its video's key, so nothing of it depends on S, on the batch position or on the
// grid.  prm null (dense): cz and step by value; else (plan rows) cz = prm[8], step = prm[9] of the 12 uploaded floats, so ONE captured launch
// serves every schedule entry.
struct VideoNoiseArgs { const uint32_t* keys; const float* prm; float cz; uint32_t step; };
constexpr uint32_t NOISE_STREAM_VIDEO_STEP = 1u;        // noise.STREAM_VIDEO_STEP; 0 is the image sampler's step
constexpr uint32_t NOISE_STREAM_VIDEO_HOLD = 2u;        // noise.STREAM_VIDEO_HOLD: the held part's one fixed noise (step 0 at every noise level)

// HOLD: the presence of ONE more trailing kernel argument behind VideoNoiseArgs.  kx: the clean latent to hold, fp32 [S or 1][C][kx_f][hw] with
// kx_f in {1, F} (1: one image for every frame) and video s at s * kx_vs (0: one for all videos); w: its weight, fp32 in [0, 1], [S or 1][w_f][hw],
// the same for every channel.  (ha, hs) = sqrt(alpha), sqrt(1 - alpha) of the state the step WRITES: prm null: by value; else prm[10], prm[11] of
// the 12 uploaded floats.  F and hw locate (c, f, p) of an element in its video (rs.per = C F hw gives the video).
struct VideoHoldArgs { const float* kx; int64_t kx_vs; int kx_f; const float* w; int64_t w_vs; int w_f; const float* prm; float ha, hs; int F; int64_t hw; };

// where element r = (c, f, p) of video s reads its held latent and its weight
struct HoldAt { int64_t kx, w; };
__device__ __forceinline__ HoldAt hold_at(const VideoHoldArgs& h, int64_t s, int64_t r) {
    const int64_t p = r % h.hw, cf = r / h.hw;
    const int64_t f = cf % h.F, c = cf / h.F;
    return {s * h.kx_vs + (c * h.kx_f + (h.kx_f == 1 ? 0 : f)) * h.hw + p, s * h.w_vs + (h.w_f == 1 ? 0 : f) * h.hw + p};
}

// THE blend of the hold, for the step entries and the composite entry alike:
//   kept = hs != 0 ? rnd(rnd(ha kx) + rnd(hs zh)) : kx          zh = the normal of (r, the video's key, step 0, NOISE_STREAM_VIDEO_HOLD)
//   out  = w == 0 ? moved : w == 1 ? kept : rnd(rnd(w kept) + rnd(rnd(1 - w) moved))
// The selects are the point: w == 0 keeps the parent's bits, w == 1 does not look at moved (a NaN there stays out), hs == 0 gives kx back with its
// sign bit and calls no generator.  zh is not formed where w == 0 (it would not be used).
template <int DT>
__device__ __forceinline__ float hold_blend(float moved, float kx, float w, float ha, float hs, uint64_t r, uint32_t key_lo, uint32_t key_hi) {
    if (w == 0.0f) return moved;
    float kept = kx;
    if (hs != 0.0f) {
        const float zh = noise_normal(r, key_lo, key_hi, 0u, NOISE_STREAM_VIDEO_HOLD);
        kept = rnd<DT>(rnd<DT>(ha * kx) + rnd<DT>(hs * zh));
    }
    if (w == 1.0f) return kept;
    return rnd<DT>(rnd<DT>(w * kept) + rnd<DT>(rnd<DT>(1.0f - w) * moved));
}

template <typename A, typename... R> __device__ __forceinline__ const A& pack_first(const A& a, const R&...) { return a; }
template <typename A, typename B> __device__ __forceinline__ const B& pack_second(const A&, const B& b) { return b; }

// MS: the multistep move; x0_prev [n] fp32 is then read and rewritten with this step's x0 (no other argument aliases it), and is not touched otherwise.
// RS: element i uses the factor of its video, rs.fac[i / rs.per] (the video is the outermost index of i), for x0 AND for the DDIM move's eps; without
// RS no factor is read and no product is formed, which is what keeps those instantiations' bits the ones they had before the rescale existed.
// NzT: nothing, or {VideoNoiseArgs}: the stored value is then cz != 0 ? rnd(moved + rnd(cz * z)) : moved -- one product and one sum behind the
// parent's operations, and no generator call at cz == 0 (rs.per is read for the video of i, so the launcher always fills it); or
// {VideoNoiseArgs, VideoHoldArgs}: the stored value is then hold_blend of that one.
// View::COND: v'' is the view's one prediction (no vu, no g, no factor; never with RS); the moves, the noise and the hold behind it are the same lines.
template <typename View, bool MS, bool RS, typename... NzT>
__global__ void __launch_bounds__(256)
video_step_kernel(const View vw, float* __restrict__ x0_prev, int64_t n, const RescaleArgs rs, const NzT... nz) {
    constexpr int DT = View::DT;
    constexpr bool NZ = sizeof...(NzT) >= 1, HOLD = sizeof...(NzT) == 2;
    static_assert(sizeof...(NzT) <= 2, "the trailing arguments are nothing, one VideoNoiseArgs, or that and one VideoHoldArgs");
    const StepCoef k = vw.template coef<MS>();
    float cz = 0.0f;
    uint32_t step = 0;
    const uint32_t* keys = nullptr;
    if constexpr (NZ) {
        const VideoNoiseArgs& a = pack_first(nz...);
        cz = a.prm ? a.prm[8] : a.cz;
        step = a.prm ? (uint32_t)a.prm[9] : a.step;
        keys = a.keys;
    }
    float ha = 0.0f, hs = 0.0f;
    if constexpr (HOLD) {
        const VideoHoldArgs& h = pack_second(nz...);
        ha = h.prm ? h.prm[10] : h.ha;
        hs = h.prm ? h.prm[11] : h.hs;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = vw.xv(i);
        float p = 0.0f, f = 1.0f;
        if constexpr (MS) p = x0_prev[i];
        if constexpr (RS) f = rs.fac[i / rs.per];
        VPred e;
        if constexpr (View::COND) {
            static_assert(!RS, "the unguided step has no rescale form: at g = 1 the rescaled prediction is the conditional one");
            e = vpred_x0<DT>(xv, vw.vc(i), k.sa, k.s1);
        } else e = vpred_x0<DT, RS>(xv, vw.vu(i), vw.vc(i), k.g, k.sa, k.s1, f);
        float moved;
        if constexpr (MS) moved = vpred_ms_move<DT>(xv, e.x0, p, k.a, k.b, k.c);
        else moved = vpred_ddim_move<DT>(xv, e, k.sa, k.s1, k.a, k.b);
        if constexpr (NZ) {
            if (cz != 0.0f) {
                const int64_t s = i / rs.per;
                const float z = noise_normal((uint64_t)(i - s * rs.per), keys[2 * s], keys[2 * s + 1], step, NOISE_STREAM_VIDEO_STEP);
                moved = rnd<DT>(moved + rnd<DT>(cz * z));
            }
        }
        if constexpr (HOLD) {
            const VideoHoldArgs& h = pack_second(nz...);
            const int64_t s = i / rs.per, r = i - s * rs.per;
            const HoldAt at = hold_at(h, s, r);
            moved = hold_blend<DT>(moved, h.kx[at.kx], h.w[at.w], ha, hs, (uint64_t)r, keys[2 * s], keys[2 * s + 1]);
        }
        vw.st(i, moved);
        if constexpr (MS) x0_prev[i] = e.x0;
    }
}

template <bool MS, bool RS, typename View, typename... NzT>
int launch_video_step(const View& vw, float* x0_prev, int64_t n, const RescaleArgs& rs, hipStream_t st, const NzT&... nz) {
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    video_step_kernel<View, MS, RS, NzT...><<<(unsigned)blocks, 256, 0, st>>>(vw, x0_prev, n, rs, nz...);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// f(MS, RS as std::bool_constant) for the form a noise entry's nullable x0_prev / factors select
template <typename F> int for_form(bool ms, bool rs, F&& f) {
    if (ms) return rs ? f(std::true_type(), std::true_type()) : f(std::true_type(), std::false_type());
    return rs ? f(std::false_type(), std::true_type()) : f(std::false_type(), std::false_type());
}

// the unguided entries' form: nz null: no trailing argument; hd null: the noise alone; else the noise and the hold.  Never RS; no factor exists.
template <bool MS, typename View>
int launch_cond_step(const View& vw, float* x0_prev, int64_t n, int64_t per, hipStream_t st, const VideoNoiseArgs* nz, const VideoHoldArgs* hd) {
    const RescaleArgs rs = {nullptr, per};
    if (nz && hd) return launch_video_step<MS, false>(vw, x0_prev, n, rs, st, *nz, *hd);
    if (nz) return launch_video_step<MS, false>(vw, x0_prev, n, rs, st, *nz);
    return launch_video_step<MS, false>(vw, x0_prev, n, rs, st);
}

// the four dense entries: videos x per elements (the forms without the rescale: 1 x n, answered as "empty latent")
template <bool MS, bool RS>
int dense_step(const char* me, bool dtype_first, const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t per,
               const StepCoef& k, const float* factors, void* stream) {
    if (int rc = check_vpred_step(me, x && v && out, MS, x0_prev, RS, factors, dtype, dtype_first, !RS, videos, 1, 1, per, per, per)) return rc;
    const int64_t n = (int64_t)videos * per;
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        typedef typename EpsT<dt()>::T T;
        return launch_video_step<MS, RS>(DenseView<dt()>{(const T*)x, (const T*)v, (T*)out, n, k}, x0_prev, n, RescaleArgs{factors, per}, (hipStream_t)stream);
    });
}

// the four entries on plan rows
template <bool MS, bool RS>
int rows_step(const char* me, float* x, const float* v_u, int64_t su, const float* v_c, int64_t sc, float* x0_prev, const float* prm, int videos, int C,
              int F, int64_t hw, const float* factors, void* stream) {
    if (int rc = check_vpred_step(me, x && v_u && v_c && prm, MS, x0_prev, RS, factors, TMIX_F32, false, false, videos, C, F, hw, su, sc)) return rc;
    const int64_t per = (int64_t)C * F * hw;
    return launch_video_step<MS, RS>(RowsView{x, v_u, su, v_c, sc, prm, C, F, hw}, x0_prev, videos * per, RescaleArgs{factors, per}, (hipStream_t)stream);
}

// head of the captured video step: the state goes into channels [0, C) of the frame rows of both CFG halves' inputs (the image-latent
// channels [C, row_channels) are not touched) and prm[0] = t into both halves' per-clip timestep inputs
__global__ void __launch_bounds__(256)
video_prologue_kernel(const float* __restrict__ x, float* __restrict__ xu, int64_t su, float* __restrict__ tu,
                      float* __restrict__ xc, int64_t sc, float* __restrict__ tc, const float* __restrict__ prm,
                      int videos, int C, int F, int64_t hw, int row_channels, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = x[i];
        xu[video_row_offset(i, C, F, hw, row_channels, su)] = v;
        xc[video_row_offset(i, C, F, hw, row_channels, sc)] = v;
    }
    if (blockIdx.x == 0) {
        const float t = prm[0];
        for (int k = threadIdx.x; k < videos; k += blockDim.x) { tu[k] = t; tc[k] = t; }
    }
}

// head of the captured UNGUIDED step: the text half alone -- the unconditional half's inputs are not named, so not touched
__global__ void __launch_bounds__(256)
video_prologue_cond_kernel(const float* __restrict__ x, float* __restrict__ xc, int64_t sc, float* __restrict__ tc, const float* __restrict__ prm,
                           int videos, int C, int F, int64_t hw, int row_channels, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        xc[video_row_offset(i, C, F, hw, row_channels, sc)] = x[i];
    if (blockIdx.x == 0) {
        const float t = prm[0];
        for (int k = threadIdx.x; k < videos; k += blockDim.x) tc[k] = t;
    }
}

// video_gen/utils_attn.py:433-455: frames 1.. of every clip <- first frame (hard) or interp*first + (1-interp)*frame
template <int DT>
__global__ void __launch_bounds__(256)
frame_inject_kernel(typename EpsT<DT>::T* __restrict__ x, int64_t per_frame, int frames, int64_t n, int hard, float a, float b) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t per_clip = (int64_t)(frames - 1) * per_frame;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t clip = i / per_clip, r = i - clip * per_clip;
        const int64_t e = r % per_frame, base = clip * frames * per_frame;
        const float first = EpsT<DT>::ld(x, base + e);
        const int64_t dst = base + per_frame + r;
        const float o = hard ? first : rnd<DT>(rnd<DT>(a * first) + rnd<DT>(b * EpsT<DT>::ld(x, dst)));
        StT<DT>::st(x, dst, o);
    }
}

template <int DT>
int launch_inject(void* x, int64_t per_frame, int frames, int64_t n, int hard, float a, float b, hipStream_t st) {
    typedef typename EpsT<DT>::T T;
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    frame_inject_kernel<DT><<<blocks, 256, 0, st>>>((T*)x, per_frame, frames, n, hard, a, b);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// x_T under the hold, once per run: the blend with moved = x, in place on x [S][C][F][hw] of the model dtype
template <int DT>
__global__ void __launch_bounds__(256)
video_hold_composite_kernel(typename EpsT<DT>::T* __restrict__ x, int64_t n, int64_t per, const uint32_t* __restrict__ keys, const VideoHoldArgs h) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t s = i / per, r = i - s * per;
        const HoldAt at = hold_at(h, s, r);
        StT<DT>::st(x, i, hold_blend<DT>(EpsT<DT>::ld(x, i), h.kx[at.kx], h.w[at.w], h.ha, h.hs, (uint64_t)r, keys[2 * s], keys[2 * s + 1]));
    }
}

// The hold's own arguments, answered behind the parent entry's checks (so channels, frames and hw are at least 1 here): null pointers, then the
// frame counts, then the video strides -- 0 (one array for every video) or at least one video's extent.
inline int check_hold(const char* me, const float* hold_x0, int64_t x0_stride, int x0_frames, const float* hold_w, int64_t w_stride, int w_frames,
                      int channels, int frames, int64_t hw) {
    if (!hold_x0 || !hold_w) TMIX_FAIL(TMIX_EINVAL, "%s: null hold_x0 / hold_w", me);
    if ((x0_frames != 1 && x0_frames != frames) || (w_frames != 1 && w_frames != frames))
        TMIX_FAIL(TMIX_ESHAPE, "%s: hold_x0_frames=%d hold_w_frames=%d (each 1 or frames=%d)", me, x0_frames, w_frames, frames);
    const int64_t ex = (int64_t)channels * x0_frames * hw, ew = (int64_t)w_frames * hw;
    if ((x0_stride != 0 && x0_stride < ex) || (w_stride != 0 && w_stride < ew))
        TMIX_FAIL(TMIX_ESHAPE, "%s: hold video strides %lld / %lld (each 0 or at least one video's %lld / %lld floats)", me, (long long)x0_stride,
                  (long long)w_stride, (long long)ex, (long long)ew);
    return TMIX_OK;
}

}  // namespace

extern "C" int tmix_video_step_prologue(const float* x, float* x_u, int64_t clip_stride_u, float* t_u, float* x_c, int64_t clip_stride_c,
                                        float* t_c, const float* params, int videos, int channels, int frames, int64_t hw,
                                        int row_channels, void* stream) {
    if (!x || !x_u || !t_u || !x_c || !t_c || !params) TMIX_FAIL(TMIX_EINVAL, "video_step_prologue: null pointer");
    if (int rc = check_video_step("video_step_prologue", videos, channels, frames, hw, row_channels, true, clip_stride_u, clip_stride_c)) return rc;
    const int64_t n = (int64_t)videos * channels * frames * hw;
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    video_prologue_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, x_u, clip_stride_u, t_u, x_c, clip_stride_c, t_c, params,
                                                                             videos, channels, frames, hw, row_channels, n);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

extern "C" int tmix_frame_inject(void* x, int dtype, int clips, int frames, int64_t per_frame, int hard, float interp,
                                 float one_minus_interp, void* stream) {
    if (!x) TMIX_FAIL(TMIX_EINVAL, "frame_inject: null pointer");
    if (clips < 1 || frames < 2 || per_frame < 1) TMIX_FAIL(TMIX_ESHAPE, "frame_inject: clips=%d frames=%d per_frame=%lld", clips, frames, (long long)per_frame);
    const int64_t n = (int64_t)clips * (frames - 1) * per_frame;
    return for_dtype(dtype, "frame_inject", "dtype", [&](auto dt) { return launch_inject<dt()>(x, per_frame, frames, n, hard, interp, one_minus_interp, (hipStream_t)stream); });
}

// ---- the eight step entries: [_ms] the multistep move with the history buffer, [_rs] factors [videos] from tmix_vpred_rescale_factors, [_dev] on plan rows
extern "C" int tmix_vpred_step(const void* x, const void* v, void* out, int dtype, int64_t n, float g,
                               float sa, float s1, float sa_next, float s1_next, void* stream) {
    return dense_step<false, false>("vpred_step", false, x, v, out, nullptr, dtype, 1, n, {g, sa, s1, sa_next, s1_next, 0.0f}, nullptr, stream);
}

extern "C" int tmix_vpred_step_ms(const void* x, const void* v, void* out, float* x0_prev, int dtype, int64_t n, float g,
                                  float sa, float s1, float cx, float c0, float c1, void* stream) {
    return dense_step<true, false>("vpred_step_ms", true, x, v, out, x0_prev, dtype, 1, n, {g, sa, s1, cx, c0, c1}, nullptr, stream);
}

extern "C" int tmix_vpred_step_rs(const void* x, const void* v, void* out, int dtype, int videos, int64_t n_per_video, float g,
                                  float sa, float s1, float sa_next, float s1_next, const float* factors, void* stream) {
    return dense_step<false, true>("vpred_step_rs", false, x, v, out, nullptr, dtype, videos, n_per_video, {g, sa, s1, sa_next, s1_next, 0.0f}, factors, stream);
}

extern "C" int tmix_vpred_step_ms_rs(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t n_per_video, float g,
                                     float sa, float s1, float cx, float c0, float c1, const float* factors, void* stream) {
    return dense_step<true, true>("vpred_step_ms_rs", false, x, v, out, x0_prev, dtype, videos, n_per_video, {g, sa, s1, cx, c0, c1}, factors, stream);
}

extern "C" int tmix_vpred_step_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                                   const float* params, int videos, int channels, int frames, int64_t hw, void* stream) {
    return rows_step<false, false>("vpred_step_dev", x, v_u, clip_stride_u, v_c, clip_stride_c, nullptr, params, videos, channels, frames, hw, nullptr, stream);
}

extern "C" int tmix_vpred_step_ms_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                                      const float* params, int videos, int channels, int frames, int64_t hw, void* stream) {
    return rows_step<true, false>("vpred_step_ms_dev", x, v_u, clip_stride_u, v_c, clip_stride_c, x0_prev, params, videos, channels, frames, hw, nullptr, stream);
}

extern "C" int tmix_vpred_step_rs_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                                      const float* params, int videos, int channels, int frames, int64_t hw, const float* factors, void* stream) {
    return rows_step<false, true>("vpred_step_rs_dev", x, v_u, clip_stride_u, v_c, clip_stride_c, nullptr, params, videos, channels, frames, hw, factors, stream);
}

extern "C" int tmix_vpred_step_ms_rs_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                                         const float* params, int videos, int channels, int frames, int64_t hw, const float* factors, void* stream) {
    return rows_step<true, true>("vpred_step_ms_rs_dev", x, v_u, clip_stride_u, v_c, clip_stride_c, x0_prev, params, videos, channels, frames, hw, factors, stream);
}

// ---- the stochastic step: ONE entry per layout for all four parents -- x0_prev null: the DDIM move, (a, b) = (sa_next, s1_dir);
// else the multistep move (cx, c0, c1) and the history buffer; factors null: no rescale
extern "C" int tmix_vpred_step_noise(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t n_per_video, float g,
                                     float sa, float s1, float a, float b, float c, float cz, const float* factors, const uint32_t* keys,
                                     uint32_t step, void* stream) {
    const char* me = "vpred_step_noise";
    if (x && v && out && !keys) TMIX_FAIL(TMIX_EINVAL, "%s: null keys", me);
    if (int rc = check_vpred_step(me, x && v && out, false, nullptr, false, nullptr, dtype, false, false, videos, 1, 1, n_per_video, n_per_video, n_per_video)) return rc;
    const int64_t n = (int64_t)videos * n_per_video;
    const StepCoef k = {g, sa, s1, a, b, x0_prev ? c : 0.0f};
    const VideoNoiseArgs nz = {keys, nullptr, cz, step};
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        typedef typename EpsT<dt()>::T T;
        const DenseView<dt()> vw = {(const T*)x, (const T*)v, (T*)out, n, k};
        return for_form(x0_prev != nullptr, factors != nullptr, [&](auto ms, auto rs) {
            return launch_video_step<ms(), rs()>(vw, x0_prev, n, RescaleArgs{factors, n_per_video}, (hipStream_t)stream, nz);
        });
    });
}

extern "C" int tmix_vpred_step_noise_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                                         const float* params, int videos, int channels, int frames, int64_t hw, float* x0_prev,
                                         const float* factors, const uint32_t* keys, void* stream) {
    const char* me = "vpred_step_noise_dev";
    if (x && v_u && v_c && params && !keys) TMIX_FAIL(TMIX_EINVAL, "%s: null keys", me);
    if (int rc = check_vpred_step(me, x && v_u && v_c && params, false, nullptr, false, nullptr, TMIX_F32, false, false, videos, channels, frames, hw, clip_stride_u, clip_stride_c)) return rc;
    const int64_t per = (int64_t)channels * frames * hw;
    const RowsView vw = {x, v_u, clip_stride_u, v_c, clip_stride_c, params, channels, frames, hw};
    const VideoNoiseArgs nz = {keys, params, 0.0f, 0u};
    return for_form(x0_prev != nullptr, factors != nullptr, [&](auto ms, auto rs) {
        return launch_video_step<ms(), rs()>(vw, x0_prev, videos * per, RescaleArgs{factors, per}, (hipStream_t)stream, nz);
    });
}

// ---- the hold: the noise entries' kernels with one more trailing argument; cz == 0 is the deterministic parent bit for bit
extern "C" int tmix_vpred_step_hold(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int channels, int frames, int64_t hw,
                                    float g, float sa, float s1, float a, float b, float c, float cz, const float* factors, const uint32_t* keys,
                                    uint32_t step, float ha, float hs, const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames,
                                    const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream) {
    const char* me = "vpred_step_hold";
    if (x && v && out && !keys) TMIX_FAIL(TMIX_EINVAL, "%s: null keys", me);
    const int64_t clip = (int64_t)(channels > 0 ? channels : 0) * (frames > 0 ? frames : 0) * (hw > 0 ? hw : 0);
    if (int rc = check_vpred_step(me, x && v && out, false, nullptr, false, nullptr, dtype, false, false, videos, channels, frames, hw, clip, clip)) return rc;
    if (int rc = check_hold(me, hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, channels, frames, hw)) return rc;
    const int64_t per = (int64_t)channels * frames * hw, n = (int64_t)videos * per;
    const StepCoef k = {g, sa, s1, a, b, x0_prev ? c : 0.0f};
    const VideoNoiseArgs nz = {keys, nullptr, cz, step};
    const VideoHoldArgs hd = {hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, nullptr, ha, hs, frames, hw};
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        typedef typename EpsT<dt()>::T T;
        const DenseView<dt()> vw = {(const T*)x, (const T*)v, (T*)out, n, k};
        return for_form(x0_prev != nullptr, factors != nullptr, [&](auto ms, auto rs) {
            return launch_video_step<ms(), rs()>(vw, x0_prev, n, RescaleArgs{factors, per}, (hipStream_t)stream, nz, hd);
        });
    });
}

extern "C" int tmix_vpred_step_hold_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                                        const float* params, int videos, int channels, int frames, int64_t hw, float* x0_prev,
                                        const float* factors, const uint32_t* keys, const float* hold_x0, int64_t hold_x0_video_stride,
                                        int hold_x0_frames, const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream) {
    const char* me = "vpred_step_hold_dev";
    if (x && v_u && v_c && params && !keys) TMIX_FAIL(TMIX_EINVAL, "%s: null keys", me);
    if (int rc = check_vpred_step(me, x && v_u && v_c && params, false, nullptr, false, nullptr, TMIX_F32, false, false, videos, channels, frames, hw, clip_stride_u, clip_stride_c)) return rc;
    if (int rc = check_hold(me, hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, channels, frames, hw)) return rc;
    const int64_t per = (int64_t)channels * frames * hw;
    const RowsView vw = {x, v_u, clip_stride_u, v_c, clip_stride_c, params, channels, frames, hw};
    const VideoNoiseArgs nz = {keys, params, 0.0f, 0u};
    const VideoHoldArgs hd = {hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, params, 0.0f, 0.0f, frames, hw};
    return for_form(x0_prev != nullptr, factors != nullptr, [&](auto ms, auto rs) {
        return launch_video_step<ms(), rs()>(vw, x0_prev, videos * per, RescaleArgs{factors, per}, (hipStream_t)stream, nz, hd);
    });
}

extern "C" int tmix_video_hold_composite(void* x, int dtype, int videos, int channels, int frames, int64_t hw, float ha, float hs, const uint32_t* keys,
                                         const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames, const float* hold_w,
                                         int64_t hold_w_video_stride, int hold_w_frames, void* stream) {
    const char* me = "video_hold_composite";
    if (x && !keys) TMIX_FAIL(TMIX_EINVAL, "%s: null keys", me);
    const int64_t clip = (int64_t)(channels > 0 ? channels : 0) * (frames > 0 ? frames : 0) * (hw > 0 ? hw : 0);
    if (int rc = check_vpred_step(me, x != nullptr, false, nullptr, false, nullptr, dtype, false, false, videos, channels, frames, hw, clip, clip)) return rc;
    if (int rc = check_hold(me, hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, channels, frames, hw)) return rc;
    const int64_t per = (int64_t)channels * frames * hw, n = (int64_t)videos * per;
    const VideoHoldArgs hd = {hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, nullptr, ha, hs, frames, hw};
    return for_dtype(dtype, me, "dtype", [&](auto dt) -> int {
        typedef typename EpsT<dt()>::T T;
        int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
        video_hold_composite_kernel<dt()><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((T*)x, n, per, keys, hd);
        TMIX_LAUNCH_CHECK();
        return TMIX_OK;
    });
}

// ---- the unguided step: the text half alone.  The prologue fills the text half's inputs; ONE step entry per layout serves every
// form -- x0_prev null: the DDIM move (a, b) = (sa_next, s1_next or s1_dir), else the multistep move (a, b, c) and the history buffer; keys null:
// no noise (cz and step are not read) and then no hold either; hold_x0 and hold_w both null: no hold.  No g, no factors: neither is an argument.
extern "C" int tmix_video_step_prologue_cond(const float* x, float* x_c, int64_t clip_stride_c, float* t_c, const float* params, int videos,
                                             int channels, int frames, int64_t hw, int row_channels, void* stream) {
    const char* me = "video_step_prologue_cond";
    if (!x || !x_c || !t_c || !params) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (int rc = check_video_step(me, videos, channels, frames, hw, row_channels, true, clip_stride_c, clip_stride_c)) return rc;
    const int64_t n = (int64_t)videos * channels * frames * hw;
    int64_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    video_prologue_cond_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, x_c, clip_stride_c, t_c, params, videos, channels, frames, hw,
                                                                                  row_channels, n);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

namespace {
// the unguided entries' own answers behind check_vpred_step: a hold needs the videos' keys (its fixed noise is keyed by them), then check_hold
// (one of hold_x0 / hold_w null: EINVAL).  *held: is there a hold?
inline int check_cond_hold(const char* me, const uint32_t* keys, const float* hold_x0, int64_t x0_stride, int x0_frames, const float* hold_w,
                           int64_t w_stride, int w_frames, int channels, int frames, int64_t hw, bool* held) {
    *held = hold_x0 || hold_w;
    if (!*held) return TMIX_OK;
    if (!keys) TMIX_FAIL(TMIX_EINVAL, "%s: a hold without keys (the held part's fixed noise is keyed by the video)", me);
    return check_hold(me, hold_x0, x0_stride, x0_frames, hold_w, w_stride, w_frames, channels, frames, hw);
}
}  // namespace

extern "C" int tmix_vpred_step_cond(const void* x, const void* v_c, void* out, float* x0_prev, int dtype, int videos, int channels, int frames,
                                    int64_t hw, float sa, float s1, float a, float b, float c, float cz, const uint32_t* keys, uint32_t step,
                                    float ha, float hs, const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames,
                                    const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream) {
    const char* me = "vpred_step_cond";
    const int64_t clip = (int64_t)(channels > 0 ? channels : 0) * (frames > 0 ? frames : 0) * (hw > 0 ? hw : 0);
    if (int rc = check_vpred_step(me, x && v_c && out, false, nullptr, false, nullptr, dtype, false, false, videos, channels, frames, hw, clip, clip)) return rc;
    bool held;
    if (int rc = check_cond_hold(me, keys, hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, channels, frames, hw, &held)) return rc;
    const int64_t per = (int64_t)channels * frames * hw, n = (int64_t)videos * per;
    const StepCoef k = {0.0f, sa, s1, a, b, x0_prev ? c : 0.0f};
    const VideoNoiseArgs nz = {keys, nullptr, cz, step};
    const VideoHoldArgs hd = {hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, nullptr, ha, hs, frames, hw};
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        typedef typename EpsT<dt()>::T T;
        const DenseCondView<dt()> vw = {(const T*)x, (const T*)v_c, (T*)out, k};
        if (x0_prev) return launch_cond_step<true>(vw, x0_prev, n, per, (hipStream_t)stream, keys ? &nz : nullptr, held ? &hd : nullptr);
        return launch_cond_step<false>(vw, nullptr, n, per, (hipStream_t)stream, keys ? &nz : nullptr, held ? &hd : nullptr);
    });
}

// params: the parents' layouts -- 8 floats without keys ({t, sa, s1, sa_next, s1_next, g, 0, 0} / {t, sa, s1, cx, c0, c1, g, 0}), 12 with
// (then {cz, schedule index, ha, hs}); the g slot is not read
extern "C" int tmix_vpred_step_cond_dev(float* x, const float* v_c, int64_t clip_stride_c, const float* params, int videos, int channels, int frames,
                                        int64_t hw, float* x0_prev, const uint32_t* keys, const float* hold_x0, int64_t hold_x0_video_stride,
                                        int hold_x0_frames, const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream) {
    const char* me = "vpred_step_cond_dev";
    if (int rc = check_vpred_step(me, x && v_c && params, false, nullptr, false, nullptr, TMIX_F32, false, false, videos, channels, frames, hw, clip_stride_c, clip_stride_c)) return rc;
    bool held;
    if (int rc = check_cond_hold(me, keys, hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, channels, frames, hw, &held)) return rc;
    const int64_t per = (int64_t)channels * frames * hw;
    const RowsCondView vw = {x, v_c, clip_stride_c, params, channels, frames, hw};
    const VideoNoiseArgs nz = {keys, params, 0.0f, 0u};
    const VideoHoldArgs hd = {hold_x0, hold_x0_video_stride, hold_x0_frames, hold_w, hold_w_video_stride, hold_w_frames, params, 0.0f, 0.0f, frames, hw};
    if (x0_prev) return launch_cond_step<true>(vw, x0_prev, videos * per, per, (hipStream_t)stream, keys ? &nz : nullptr, held ? &hd : nullptr);
    return launch_cond_step<false>(vw, nullptr, videos * per, per, (hipStream_t)stream, keys ? &nz : nullptr, held ? &hd : nullptr);
}
