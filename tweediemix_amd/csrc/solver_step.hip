// solver_step.hip -- fused CFG + Tweedie x0 + mask blend + DPM-Solver++(2M) update on the blended estimate (one HBM pass).
// The x0 part IS tweedie_step.hip's: both kernels call step_core.h's blended_x0, so out_x0 is that kernel's out_x0 bit for bit; the move is the
// data-prediction form x_next = cx x + c0 x0 + c1 x0_prev with the history buffer x0_prev read and rewritten in the same pass.  Per element and
// seed it reads (rows) eps values + x + K mask values + 1 history value and writes 2-3 floats.
// Compiled with -ffp-contract=off so fp32 results are bit-identical to the numpy restatement (solver.multistep_step_reference).
// The image sampler's kernel and entries only: the same move on the video sampler's v-prediction is video_step.hip's.
// The stochastic step (tmix_fused_tweedie_step_noise_dev) is this kernel with a trailing NoiseArgs: the move of either solver plus
// cz * z, z from noise.h.  The unguided step (tmix_fused_tweedie_step_cond_dev) is this kernel with a trailing CondArgs: eps rows
// without the unconditional one, each used as it is, and a DDIM move on the eps consistent with the blended estimate.  The APG step
// (tmix_fused_tweedie_step_apg_dev) is this kernel with a trailing ApgArgs: every row's estimate is A tc + B (tc - tu).
#include "step_core.h"
#include "noise.h"
#include "../../include/tmix_apg.h"

namespace {

// NOISE: one trailing NoiseArgs kernel argument (behind the RescaleArgs when both are there).  Row `sd` of the launch is window sd % n_win of
// trajectory sd / n_win (tmix_window_consensus's layout); its element (c, y, x) has the canvas index c*canvas_hw + (oy + y)*canvas_w + ox + x,
// the counter of its noise; keys [rows / n_win][2] are the trajectories' {low, high} key words.  The offsets travel by value, so a captured
// launch carries them.  prm holds 12 floats then: the parent's 8, {cz, step index, 0, 0}.
struct NoiseArgs { const uint32_t* keys; int n_win, w, canvas_w; int64_t canvas_hw; int oy[TMIX_MAX_WINDOWS], ox[TMIX_MAX_WINDOWS]; };
// COND (tmix_fused_tweedie_step_cond_dev): one trailing CondArgs, an empty tag (behind the NoiseArgs when both are there; never with
// a RescaleArgs).  eps holds NO unconditional row and every row's prediction is used as it is (step_core.h's blended_x0<.., COND>); like NOISE it
// may come without a history buffer, and its DDIM move takes the eps that is consistent with the blended estimate in the place of the
// unconditional row: e0 = (x - sa x0) / s1 in fp32 (0 where s1 == 0), moved = sa_next x0 + rnd(s1_next e0).
struct CondArgs {};
template <typename A, typename... T> constexpr bool pack_has = (__is_same(T, A) || ...);
template <typename A, typename T0, typename... T> __device__ __forceinline__ const A& pack_get(const T0& t0, const T&... t) {
    if constexpr (__is_same(T0, A)) return t0; else return pack_get<A>(t...);
}

// prm = {t, sa, s1, cx, c0, c1, is_last, g} in device memory (one captured launch serves every timestep and both orders); blockIdx.y walks
// co-batched seeds (x / out_x / out_x0 / x0_prev: [seeds][n], eps: [seeds][rows][n], masks: [seeds][K][hw] or shared).  x may alias out_x:
// every array is read at i before it is written at i.  x0_prev is read AND written, so it carries no __restrict__.
// RESCALE: the presence of a trailing RescaleArgs kernel argument (step_core.h; tweedie_step.hip's KeepArgs mechanism); without a trailing
// argument the kernel has the arguments it had before.
// APG (step_core.h's ApgArgs and blended_x0_apg): the rows' estimates are combined in data space with the {A, B} pairs of tmix_apg_coeffs; g is
// not read.  Like NOISE and COND it may come without a history buffer, and then has a RESAMPLE form too.
// NOISE (above) alone may come without a history buffer: x0_prev == nullptr selects the DDIM entry's params layout {t, sa, s1, sa_next, s1_next,
// is_last, g, -} and its move sa_next x0 + rnd(s1_next eu), formed as tweedie_step.hip forms it.
template <int DT, int MODE, typename... ExT>
__global__ void __launch_bounds__(256)
solver_step_kernel(const float* x, const typename EpsT<DT>::T* __restrict__ eps, const float* __restrict__ masks, float* out_x,
                   float* __restrict__ out_x0, float* x0_prev, int K, int64_t n, int64_t hw, const float* __restrict__ prm, int rows,
                   int64_t mask_seed_stride, ExT... ex) {
    constexpr bool RS = pack_has<RescaleArgs, ExT...>, NZ = pack_has<NoiseArgs, ExT...>, COND = pack_has<CondArgs, ExT...>;
    constexpr bool APG = pack_has<ApgArgs, ExT...>;
    static_assert(sizeof...(ExT) == (RS ? 1 : 0) + (NZ ? 1 : 0) + (COND ? 1 : 0) + (APG ? 1 : 0) && !(RS && COND) && !(APG && (RS || COND)),
                  "the trailing arguments are a RescaleArgs, a NoiseArgs or both, a CondArgs behind an optional NoiseArgs, or an ApgArgs in front of an optional NoiseArgs");
    const float* fac = nullptr;
    if constexpr (RS) fac = pack_get<RescaleArgs>(ex...).fac + (int64_t)blockIdx.y * (rows - 1);
    if constexpr (APG) fac = pack_get<ApgArgs>(ex...).ab + (int64_t)blockIdx.y * (rows - 1) * 2;      // the seed's {A, B} pairs
    const bool ddim = (NZ || COND || APG) && !x0_prev;
    const float sa = prm[1], s1 = prm[2], cx = prm[3], c0 = prm[4], c1 = prm[5], g = prm[ddim ? 6 : 7];
    const bool is_last = prm[ddim ? 5 : 6] != 0.0f;
    const int64_t sd = blockIdx.y;
    x += sd * n; out_x += sd * n;
    if (!ddim) x0_prev += sd * n;
    eps += sd * rows * n; masks += sd * mask_seed_stride;
    if (out_x0) out_x0 += sd * n;
    float cz = 0.0f;
    uint32_t key_lo = 0, key_hi = 0, step = 0;
    int64_t win_base = 0;                            // the canvas index of the row's element (0, 0, 0)
    if constexpr (NZ) {
        const NoiseArgs& nz = pack_get<NoiseArgs>(ex...);
        const int64_t grp = sd / nz.n_win;
        const int win = (int)(sd % nz.n_win);
        cz = is_last ? 0.0f : prm[8];
        step = (uint32_t)prm[9];
        key_lo = nz.keys[2 * grp]; key_hi = nz.keys[2 * grp + 1];
        win_base = (int64_t)nz.oy[win] * nz.canvas_w + nz.ox[win];
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xv = x[i];
        const float p = ddim ? 0.0f : x0_prev[i];
        float eu = 0.0f;
        if constexpr (!COND) eu = EpsT<DT>::ld(eps, i);
        float x0;
        if constexpr (APG) x0 = blended_x0_apg<DT, MODE>(eps, masks, fac, K, n, hw, i, xv, eu, sa, s1);
        else x0 = blended_x0<DT, MODE, RS, COND>(eps, masks, fac, K, n, hw, i, xv, eu, g, sa, s1);
        float moved;
        if (ddim) {                                  // prm[3], prm[4] hold sa_next, s1_next
            if constexpr (COND) eu = s1 != 0.0f ? (xv - sa * x0) / s1 : 0.0f;       // e0: the eps consistent with x0 stands in for the missing row
            moved = cx * x0 + rnd<DT>(c0 * eu);
        } else {
            float m = c0 * x0;
            if (c1 != 0.0f) m = m + c1 * p;          // a first-order step never touches the history value: a NaN left there stays out
            moved = cx * xv + m;
        }
        if constexpr (NZ) {
            if (cz != 0.0f) {                        // cz == 0 (eta = 0, the last step): the parent entry's bits, no generator call
                const NoiseArgs& nz = pack_get<NoiseArgs>(ex...);
                const int64_t q = i % hw;
                const int64_t idx = (i / hw) * nz.canvas_hw + (q / nz.w) * nz.canvas_w + q % nz.w + win_base;
                moved = moved + cz * noise_normal((uint64_t)idx, key_lo, key_hi, step, 0u);
            }
        }
        out_x[i] = is_last ? x0 : moved;
        if (!ddim) x0_prev[i] = x0;
        if (out_x0) out_x0[i] = x0;
    }
}

template <int DT, typename... RsT>      // RsT: the kernel's trailing arguments -- none, {RescaleArgs}, {NoiseArgs}, {RescaleArgs, NoiseArgs}, {CondArgs}, {NoiseArgs, CondArgs},
                                        // {ApgArgs} or {ApgArgs, NoiseArgs}
int launch_ms(const float* x, const void* eps, const float* masks, int64_t mss, float* out_x, float* out_x0, float* x0_prev, int K, int64_t n,
              int64_t hw, int mode, int rows, int seeds, const float* prm, hipStream_t st, RsT... rs) {
    typedef typename EpsT<DT>::T T;
    int64_t bx = (n + 255) / 256; if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, (unsigned)seeds);
    const T* e = (const T*)eps;
    if constexpr (pack_has<ApgArgs, RsT...> && !pack_has<NoiseArgs, RsT...>) {      // the APG entry alone has a RESAMPLE form (its DDIM layout, no noise)
        if (mode == TMIX_STEP_RESAMPLE) {
            solver_step_kernel<DT, TMIX_STEP_RESAMPLE, RsT...><<<grid, 256, 0, st>>>(x, e, masks, out_x, out_x0, x0_prev, K, n, hw, prm, rows, mss, rs...);
            TMIX_LAUNCH_CHECK();
            return TMIX_OK;
        }
    }
    if (mode == TMIX_STEP_FUSION)
        solver_step_kernel<DT, TMIX_STEP_FUSION, RsT...><<<grid, 256, 0, st>>>(x, e, masks, out_x, out_x0, x0_prev, K, n, hw, prm, rows, mss, rs...);
    else
        solver_step_kernel<DT, TMIX_STEP_PLAIN, RsT...><<<grid, 256, 0, st>>>(x, e, masks, out_x, out_x0, x0_prev, K, n, hw, prm, rows, mss, rs...);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// The checks of a noise entry's window arguments and the NoiseArgs they give (tmix_fused_tweedie_step_noise_dev, tmix_fused_tweedie_step_cond_dev
// with keys).  Without win_yx the latent is its own grid.
int make_noise_args(const char* me, NoiseArgs& nz, const uint32_t* keys, int64_t hw, int seeds, int w, int n_win, const int* win_yx, int canvas_h,
                    int canvas_w) {
    if (n_win < 1 || n_win > TMIX_MAX_WINDOWS || (!win_yx && n_win != 1))
        TMIX_FAIL(TMIX_EINVAL, "%s: n_win=%d (1..%d; without win_yx 1)", me, n_win, TMIX_MAX_WINDOWS);
    if (w < 1 || hw % w != 0) TMIX_FAIL(TMIX_ESHAPE, "%s: hw=%lld is not a multiple of the row width w=%d", me, (long long)hw, w);
    if (seeds % n_win != 0) TMIX_FAIL(TMIX_ESHAPE, "%s: seeds=%d is not a multiple of n_win=%d", me, seeds, n_win);
    const int h = (int)(hw / w);
    nz = {};
    nz.keys = keys; nz.n_win = n_win; nz.w = w;
    if (!win_yx) { canvas_h = h; canvas_w = w; }        // no canvas: the latent is its own grid
    for (int k = 0; win_yx && k < n_win; ++k) {
        const int oy = win_yx[2 * k], ox = win_yx[2 * k + 1];
        if (oy < 0 || ox < 0 || oy > canvas_h - h || ox > canvas_w - w)
            TMIX_FAIL(TMIX_ESHAPE, "%s: window %d at (%d, %d) of %d x %d reaches outside the %d x %d canvas", me, k, oy, ox, h, w, canvas_h, canvas_w);
        nz.oy[k] = oy; nz.ox[k] = ox;
    }
    nz.canvas_w = canvas_w; nz.canvas_hw = (int64_t)canvas_h * canvas_w;
    return TMIX_OK;
}

// the generator on its own: z[i] of index first_index + i
__global__ void __launch_bounds__(256)
noise_normal_kernel(float* __restrict__ z, int64_t n, uint64_t first_index, uint32_t key_lo, uint32_t key_hi, uint32_t step, uint32_t stream_id) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        z[i] = noise_normal(first_index + (uint64_t)i, key_lo, key_hi, step, stream_id);
}

}  // namespace

extern "C" int tmix_noise_normal(float* z, int64_t n, int64_t first_index, uint32_t key_lo, uint32_t key_hi, uint32_t step, uint32_t stream_id,
                                 void* stream) {
    if (!z) TMIX_FAIL(TMIX_EINVAL, "noise_normal: null pointer");
    if (n < 1 || first_index < 0) TMIX_FAIL(TMIX_ESHAPE, "noise_normal: n=%lld (>= 1) first_index=%lld (>= 0)", (long long)n, (long long)first_index);
    int64_t bx = (n + 255) / 256; if (bx > 2048) bx = 2048;
    noise_normal_kernel<<<(unsigned)bx, 256, 0, (hipStream_t)stream>>>(z, n, (uint64_t)first_index, key_lo, key_hi, step, stream_id);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
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

// The stochastic step of both solvers and of both rescale forms: the parent entry's move plus cz * z.
extern "C" int tmix_fused_tweedie_step_noise_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                                 float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                                 const float* params, float* x0_prev, const float* factors, const uint32_t* keys, int w,
                                                 int n_win, const int* win_yx, int canvas_h, int canvas_w, void* stream) {
    const char* me = "tweedie_step_noise_dev";
    if (int rc = check_dev_step(me, false, false, x, eps, out_x, params, nullptr, keys ? nullptr : "null keys", masks, K, channels, hw, mode, rows, seeds)) return rc;
    NoiseArgs nz;
    if (int rc = make_noise_args(me, nz, keys, hw, seeds, w, n_win, win_yx, canvas_h, canvas_w)) return rc;
    const int64_t n = (int64_t)channels * hw;
    const RescaleArgs rs = {factors};
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        if (factors) return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, rs, nz);
        return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, nz);
    });
}

// The unguided step: eps [seeds][rows][n] holds NO unconditional row; every row's prediction is used as it is.  x0_prev NULL: the
// DDIM params layout and the move on the eps consistent with x0; else the multistep layout and move.  keys NULL: no noise (8 floats, the window
// arguments are not read); else the noise entry's 12 floats and canvas indexing.
extern "C" int tmix_fused_tweedie_step_cond_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                                float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                                const float* params, float* x0_prev, const uint32_t* keys, int w, int n_win, const int* win_yx,
                                                int canvas_h, int canvas_w, void* stream) {
    const char* me = "tweedie_step_cond_dev";
    if (int rc = check_dev_step(me, false, false, x, eps, out_x, params, nullptr, nullptr, masks, K, channels, hw, mode, rows, seeds, true)) return rc;
    NoiseArgs nz;
    if (keys) if (int rc = make_noise_args(me, nz, keys, hw, seeds, w, n_win, win_yx, canvas_h, canvas_w)) return rc;
    const int64_t n = (int64_t)channels * hw;
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        if (keys) return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, nz, CondArgs());
        return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, CondArgs());
    });
}

// The APG step: every conditional row's Tweedie estimate becomes A tc + B (tc - tu), {A, B} = coeffs[seed][row - 1] (tmix_apg_coeffs),
// in all three modes; everything behind it -- the blend, the move (the DDIM move's noise term stays the unconditional row), the noise -- is the
// parent's.  x0_prev NULL: the DDIM params layout and move (FUSION, PLAIN, RESAMPLE); else the multistep layout and move (FUSION, PLAIN).
// keys NULL: no noise (8 floats, the window arguments are not read); else the noise entry's 12 floats and canvas indexing (FUSION, PLAIN).
extern "C" int tmix_fused_tweedie_step_apg_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                               float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                               const float* params, float* x0_prev, const float* coeffs, const uint32_t* keys, int w, int n_win,
                                               const int* win_yx, int canvas_h, int canvas_w, void* stream) {
    const char* me = "tweedie_step_apg_dev";
    if (int rc = check_dev_step(me, true, false, x, eps, out_x, params, nullptr, coeffs ? nullptr : "null coeffs", masks, K, channels, hw, mode, rows, seeds)) return rc;
    if (mode == TMIX_STEP_RESAMPLE && (x0_prev || keys))
        TMIX_FAIL(TMIX_EINVAL, "%s: RESAMPLE exists on the DDIM move without noise only (x0_prev and keys must be null)", me);
    NoiseArgs nz;
    if (keys) if (int rc = make_noise_args(me, nz, keys, hw, seeds, w, n_win, win_yx, canvas_h, canvas_w)) return rc;
    const int64_t n = (int64_t)channels * hw;
    const ApgArgs ap = {coeffs};
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        if (keys) return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, ap, nz);
        return launch_ms<dt()>(x, eps, masks, mask_seed_stride, out_x, out_x0, x0_prev, K, n, hw, mode, rows, seeds, params, (hipStream_t)stream, ap);
    });
}
