// cfg_rescale.hip -- guidance rescale (Lin et al., arXiv:2305.08891, section 3.4): per eps row the factor that brings the guided prediction
// e_r = cfg(eu, ec_r, g) back to the standard deviation of the conditional one, f_r = phi sd(ec_r) / sd(e_r) + (1 - phi)  (DESIGN.md 7k).
// Two launches, back to back on the caller's stream: partial sums over a FIXED partition of the row (RS_P workgroups, whatever the data), then one
// lane per (seed, row) adds the partials in index order.  No atomics, no workgroup waits for another, every workspace slot is written before it is
// read, and the summation order is a function of (n, RS_P, RS_THREADS) alone: the factors are the same bits run after run.
// e_r is formed by the step kernels' own cfg<DT> (step_core.h; compiled with -ffp-contract=off like them), so the statistics are those of the
// very values the step kernel will scale.
// Second entry, the same method per VIDEO for the v-prediction step kernels (tmix_vpred_rescale_factors): one accumulation function
// (rescale_partial_sums) and one finalise kernel serve both.
// Third entry, the same method for adaptive projected guidance (tmix_apg_coeffs): three sums of products of the rows' Tweedie
// estimates over the same partition, and per (seed, row) the two coefficients the APG step kernel combines them with.
#include "step_core.h"
#include "../../include/tmix_apg.h"

namespace {

constexpr int RS_P = 32;            // workgroups per (row, seed): fixed, so the partition (and with it the bits of the factors) never depends on the data
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;

__device__ __forceinline__ double wave_sum(double v) {      // wave64 butterfly: every lane ends with the same sum, added in the same order
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// The sums of ONE workgroup's share of one row of n elements (eu: the unconditional values, ec: the conditional ones), shared by the image kernel
// (a row of eps) and the video kernel (a video's clip): workgroup p of RS_P reads elements p * RS_THREADS + tid + k * RS_P * RS_THREADS of eu and ec
// once and writes {S_c, Q_c, S_e, Q_e} to slot[0..4): sum and sum of squares of ec and of e = cfg(eu, ec, g), in fp64, of the values MINUS the row's
// element 0 (the difference of two fp32 values in fp64; the variance does not see the shift).  The shift keeps a constant row at S = Q = 0 exactly
// and takes the mean^2 / variance term out of the one-pass formula's error.  Every loop is bounded by n; the order of the additions is a function
// of (n, RS_P, RS_THREADS) alone.
template <int DT>
__device__ __forceinline__ void rescale_partial_sums(const typename EpsT<DT>::T* __restrict__ eu, const typename EpsT<DT>::T* __restrict__ ec, int64_t n,
                                                     float g, int p, double* __restrict__ slot) {
    const float c0 = EpsT<DT>::ld(ec, 0);
    const float e0 = cfg<DT>(EpsT<DT>::ld(eu, 0), c0, g);
    double sc = 0.0, qc = 0.0, se = 0.0, qe = 0.0;
    for (int64_t i = (int64_t)p * RS_THREADS + threadIdx.x; i < n; i += (int64_t)RS_P * RS_THREADS) {
        const float c = EpsT<DT>::ld(ec, i);
        const float e = cfg<DT>(EpsT<DT>::ld(eu, i), c, g);
        const double dc = (double)c - (double)c0, de = (double)e - (double)e0;
        sc = sc + dc; qc = qc + dc * dc;
        se = se + de; qe = qe + de * de;
    }
    sc = wave_sum(sc); qc = wave_sum(qc); se = wave_sum(se); qe = wave_sum(qe);
    __shared__ double part[RS_WAVES][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = sc; part[wave][1] = qc; part[wave][2] = se; part[wave][3] = qe; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double a = part[0][threadIdx.x];
        for (int w = 1; w < RS_WAVES; ++w) a = a + part[w][threadIdx.x];
        slot[threadIdx.x] = a;
    }
}

// grid (RS_P, rows - 1, seeds).  Workgroup (p, r - 1, s) writes the sums of its share of eps row r of seed s (rescale_partial_sums) to slot
// ws[s][r - 1][p].  Rows the mode does not read (r > used) are left alone: finalise does not read them.
template <int DT>
__global__ void __launch_bounds__(RS_THREADS)
rescale_partials_kernel(const typename EpsT<DT>::T* __restrict__ eps, double* __restrict__ ws, int64_t n, int rows, int used,
                        const float* __restrict__ prm, int g_slot) {
    const int r = blockIdx.y + 1;
    if (r > used) return;
    const int64_t sd = blockIdx.z;
    const typename EpsT<DT>::T* eu = eps + sd * rows * n;
    rescale_partial_sums<DT>(eu, eu + (int64_t)r * n, n, prm[g_slot], blockIdx.x, ws + ((sd * (rows - 1) + (r - 1)) * RS_P + blockIdx.x) * 4);
}

// VIDEO: grid (RS_P, videos).  Video s is the n contiguous elements at vu + s * su and vc + s * sc (strides in elements; a standard
// deviation does not care about the order inside a clip, so plan rows and the pipeline layout are served alike); slot ws[s][p].  The partition of
// a video does not depend on `videos`: co-batched videos get the bits of their single runs.
template <int DT>
__global__ void __launch_bounds__(RS_THREADS)
vpred_rescale_partials_kernel(const typename EpsT<DT>::T* __restrict__ vu, int64_t su, const typename EpsT<DT>::T* __restrict__ vc, int64_t sc,
                              double* __restrict__ ws, int64_t n, const float* __restrict__ prm, int g_slot) {
    const int64_t s = blockIdx.y;
    rescale_partial_sums<DT>(vu + s * su, vc + s * sc, n, prm[g_slot], blockIdx.x, ws + (s * RS_P + blockIdx.x) * 4);
}

// one lane per (seed, row): the RS_P partials in index order, the variances (Q - S*S/n) / (n - 1), the factor in fp64 rounded once to fp32.
// f = 1 where sd_e is zero or a variance is not finite (diffusers would give inf / nan there), and for the rows the mode does not read.
__global__ void __launch_bounds__(RS_THREADS)
rescale_finalise_kernel(const double* __restrict__ ws, float* __restrict__ factors, int64_t n, int rows, int used, int seeds, float phi) {
    const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
    if (idx >= seeds * (rows - 1)) return;
    float f = 1.0f;
    if (idx % (rows - 1) < used) {
        const double* p = ws + (int64_t)idx * RS_P * 4;
        double sc = 0.0, qc = 0.0, se = 0.0, qe = 0.0;
        for (int k = 0; k < RS_P; ++k) { sc = sc + p[4 * k]; qc = qc + p[4 * k + 1]; se = se + p[4 * k + 2]; qe = qe + p[4 * k + 3]; }
        const double dn = (double)n;
        const double vc = (qc - sc * sc / dn) / (dn - 1.0), ve = (qe - se * se / dn) / (dn - 1.0);
        if (isfinite(vc) && isfinite(ve) && ve > 0.0) {
            const double ph = (double)phi;
            f = (float)(ph * sqrt(vc > 0.0 ? vc : 0.0) / sqrt(ve) + (1.0 - ph));
        }
    }
    factors[idx] = f;
}

template <int DT>
int launch_rescale(const void* eps, float* factors, double* ws, int64_t n, int rows, int used, int seeds, const float* prm, int g_slot, float phi,
                   hipStream_t st) {
    typedef typename EpsT<DT>::T T;
    rescale_partials_kernel<DT><<<dim3(RS_P, (unsigned)(rows - 1), (unsigned)seeds), RS_THREADS, 0, st>>>((const T*)eps, ws, n, rows, used, prm, g_slot);
    TMIX_LAUNCH_CHECK();
    const int lanes = seeds * (rows - 1);
    rescale_finalise_kernel<<<(unsigned)((lanes + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, st>>>(ws, factors, n, rows, used, seeds, phi);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// the video pair: the partials per video, then rescale_finalise_kernel with every video as a "seed" of two rows (rows = 2, used = 1)
template <int DT>
int launch_vpred_rescale(const void* vu, int64_t su, const void* vc, int64_t sc, float* factors, double* ws, int videos, int64_t n, const float* prm,
                         int g_slot, float phi, hipStream_t st) {
    typedef typename EpsT<DT>::T T;
    vpred_rescale_partials_kernel<DT><<<dim3(RS_P, (unsigned)videos), RS_THREADS, 0, st>>>((const T*)vu, su, (const T*)vc, sc, ws, n, prm, g_slot);
    TMIX_LAUNCH_CHECK();
    rescale_finalise_kernel<<<(unsigned)((videos + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, st>>>(ws, factors, n, 2, 1, videos, phi);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

// ---- APG (adaptive projected guidance): the same two launches on the rows' Tweedie estimates.
// grid (RS_P, rows - 1, seeds).  Workgroup (p, r - 1, s) writes {Sdd, Sdc, Scc, 0} of its share of eps row r of seed s to slot ws[s][r - 1][p]:
// d and tc are step_core.h's apg_term (the fp32 values the step kernel combines), products and sums in fp64.  A workgroup without elements
// writes zeros.  Rows the mode does not read (r > used) are left alone: finalise does not read them.
template <int DT>
__global__ void __launch_bounds__(RS_THREADS)
apg_partials_kernel(const float* __restrict__ x, const typename EpsT<DT>::T* __restrict__ eps, double* __restrict__ ws, int64_t n, int rows, int used,
                    const float* __restrict__ prm) {
    const int r = blockIdx.y + 1;
    if (r > used) return;
    const int64_t sd = blockIdx.z;
    const float sa = prm[1], s1 = prm[2];
    const float* xs = x + sd * n;
    const typename EpsT<DT>::T* eu = eps + sd * rows * n;
    const typename EpsT<DT>::T* ec = eu + (int64_t)r * n;
    double dd = 0.0, dc = 0.0, cc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += (int64_t)RS_P * RS_THREADS) {
        const float xv = xs[i];
        const ApgTerm t = apg_term<DT>(xv, apg_tu<DT>(xv, EpsT<DT>::ld(eu, i), sa, s1), EpsT<DT>::ld(ec, i), sa, s1);
        const double d = (double)t.d, c = (double)t.tc;
        dd = dd + d * d; dc = dc + d * c; cc = cc + c * c;
    }
    dd = wave_sum(dd); dc = wave_sum(dc); cc = wave_sum(cc);
    __shared__ double part[RS_WAVES][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = dd; part[wave][1] = dc; part[wave][2] = cc; part[wave][3] = 0.0; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double a = part[0][threadIdx.x];
        for (int w = 1; w < RS_WAVES; ++w) a = a + part[w][threadIdx.x];
        ws[((sd * (rows - 1) + (r - 1)) * RS_P + blockIdx.x) * 4 + threadIdx.x] = a;
    }
}

// one lane per (seed, row): the RS_P partials in index order, then in fp64 s = R / sqrt(Sdd) where R > 0 and Sdd > R^2 (else 1),
// p = s Sdc / Scc (0 where Scc is not positive), A = 1 - (g - 1)(1 - eta) p, B = (g - 1) s, each rounded once to fp32.
// {1, g - 1} -- CFG in data space -- where a sum is not finite, and for the rows the mode does not read.
__global__ void __launch_bounds__(RS_THREADS)
apg_finalise_kernel(const double* __restrict__ ws, float* __restrict__ coeffs, int rows, int used, int seeds, const float* __restrict__ prm, int g_slot,
                    float eta, float norm_threshold) {
    const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
    if (idx >= seeds * (rows - 1)) return;
    const double gm1 = (double)prm[g_slot] - 1.0;
    double A = 1.0, B = gm1;
    if (idx % (rows - 1) < used) {
        const double* p = ws + (int64_t)idx * RS_P * 4;
        double dd = 0.0, dc = 0.0, cc = 0.0;
        for (int k = 0; k < RS_P; ++k) { dd = dd + p[4 * k]; dc = dc + p[4 * k + 1]; cc = cc + p[4 * k + 2]; }
        if (isfinite(dd) && isfinite(dc) && isfinite(cc)) {
            const double R = (double)norm_threshold;
            const double s = (R > 0.0 && dd > R * R) ? R / sqrt(dd) : 1.0;
            const double pr = cc > 0.0 ? s * dc / cc : 0.0;
            A = 1.0 - gm1 * (1.0 - (double)eta) * pr;
            B = gm1 * s;
        }
    }
    coeffs[2 * idx] = (float)A;
    coeffs[2 * idx + 1] = (float)B;
}

template <int DT>
int launch_apg(const float* x, const void* eps, float* coeffs, double* ws, int64_t n, int rows, int used, int seeds, const float* prm, int g_slot,
               float eta, float norm_threshold, hipStream_t st) {
    typedef typename EpsT<DT>::T T;
    apg_partials_kernel<DT><<<dim3(RS_P, (unsigned)(rows - 1), (unsigned)seeds), RS_THREADS, 0, st>>>(x, (const T*)eps, ws, n, rows, used, prm);
    TMIX_LAUNCH_CHECK();
    const int lanes = seeds * (rows - 1);
    apg_finalise_kernel<<<(unsigned)((lanes + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, st>>>(ws, coeffs, rows, used, seeds, prm, g_slot, eta,
                                                                                                 norm_threshold);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}

}  // namespace

// APG coefficients: x [seeds][n] fp32 the state the step will read, eps [seeds][rows][n]; coeffs [seeds][rows - 1][2] = {A, B};
// ws: tmix_cfg_rescale_ws_doubles(rows, seeds) doubles (four per slot, three used), written before read.  g = params[g_slot], sa = params[1],
// s1 = params[2] are read on the device.  eta in [0, 1] scales the part of the update parallel to the conditional estimate (1: CFG);
// norm_threshold >= 0 clips the update's norm (0: no clip).
extern "C" int tmix_apg_coeffs(const float* x, const void* eps, int eps_dtype, float* coeffs, double* ws, int K, int channels, int64_t hw, int mode,
                               int rows, int seeds, const float* params, int g_slot, float eta, float norm_threshold, void* stream) {
    const char* me = "apg_coeffs";
    if (!x || !eps || !coeffs || !ws || !params) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (eps_dtype != TMIX_F32 && eps_dtype != TMIX_F16 && eps_dtype != TMIX_BF16) TMIX_FAIL(TMIX_EINVAL, "%s: bad eps dtype %d", me, eps_dtype);
    if (mode < TMIX_STEP_FUSION || mode > TMIX_STEP_RESAMPLE) TMIX_FAIL(TMIX_EINVAL, "%s: bad mode %d", me, mode);
    if (mode != TMIX_STEP_PLAIN && K < 1) TMIX_FAIL(TMIX_EINVAL, "%s: mode %d needs K>=1", me, mode);
    if (g_slot < 0 || g_slot > 7) TMIX_FAIL(TMIX_EINVAL, "%s: g_slot %d outside 0..7", me, g_slot);
    if (!(eta >= 0.0f && eta <= 1.0f)) TMIX_FAIL(TMIX_EINVAL, "%s: eta %g outside [0, 1]", me, (double)eta);
    if (!(norm_threshold >= 0.0f) || __builtin_isinf(norm_threshold)) TMIX_FAIL(TMIX_EINVAL, "%s: norm_threshold %g is not a finite number >= 0", me, (double)norm_threshold);
    if (channels < 1 || hw < 1 || seeds < 1 || seeds > 65535) TMIX_FAIL(TMIX_ESHAPE, "%s: channels=%d hw=%lld seeds=%d", me, channels, (long long)hw, seeds);
    const int used = mode == TMIX_STEP_PLAIN ? 1 : K;
    if (rows < used + 1 || rows > 256) TMIX_FAIL(TMIX_ESHAPE, "%s: mode %d needs %d..256 eps rows per seed, got %d", me, mode, used + 1, rows);
    return for_dtype(eps_dtype, me, "eps dtype", [&](auto dt) {
        return launch_apg<dt()>(x, eps, coeffs, ws, (int64_t)channels * hw, rows, used, seeds, params, g_slot, eta, norm_threshold, (hipStream_t)stream);
    });
}

extern "C" int64_t tmix_cfg_rescale_ws_doubles(int rows, int seeds) {
    if (rows < 2 || rows > 256 || seeds < 1 || seeds > 65535) return 0;
    return (int64_t)seeds * (rows - 1) * RS_P * 4;
}

extern "C" int tmix_cfg_rescale_factors(const void* eps, int eps_dtype, float* factors, double* ws, int K, int channels, int64_t hw, int mode,
                                        int rows, int seeds, const float* params, int g_slot, float phi, void* stream) {
    if (!eps || !factors || !ws || !params) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: null pointer");
    if (eps_dtype != TMIX_F32 && eps_dtype != TMIX_F16 && eps_dtype != TMIX_BF16) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: bad eps dtype %d", eps_dtype);
    if (mode < TMIX_STEP_FUSION || mode > TMIX_STEP_RESAMPLE) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: bad mode %d", mode);
    if (mode != TMIX_STEP_PLAIN && K < 1) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: mode %d needs K>=1", mode);
    if (g_slot < 0 || g_slot > 7) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: g_slot %d outside 0..7", g_slot);
    if (!(phi >= 0.0f && phi <= 1.0f)) TMIX_FAIL(TMIX_EINVAL, "cfg_rescale_factors: phi %g outside [0, 1]", (double)phi);
    if (channels < 1 || hw < 1 || seeds < 1 || seeds > 65535) TMIX_FAIL(TMIX_ESHAPE, "cfg_rescale_factors: channels=%d hw=%lld seeds=%d", channels, (long long)hw, seeds);
    const int64_t n = (int64_t)channels * hw;
    if (n < 2) TMIX_FAIL(TMIX_ESHAPE, "cfg_rescale_factors: a standard deviation needs n >= 2 elements, got %lld", (long long)n);
    const int used = mode == TMIX_STEP_PLAIN ? 1 : K;
    if (rows < used + 1 || rows > 256) TMIX_FAIL(TMIX_ESHAPE, "cfg_rescale_factors: mode %d needs %d..256 eps rows per seed, got %d", mode, used + 1, rows);
    return for_dtype(eps_dtype, "cfg_rescale_factors", "eps dtype", [&](auto dt) {
        return launch_rescale<dt()>(eps, factors, ws, n, rows, used, seeds, params, g_slot, phi, (hipStream_t)stream);
    });
}

extern "C" int tmix_vpred_rescale_factors(const void* v_u, int64_t stride_u, const void* v_c, int64_t stride_c, int dtype, float* factors, double* ws,
                                          int videos, int64_t n_per_video, const float* params, int g_slot, float phi, void* stream) {
    const char* me = "vpred_rescale_factors";
    if (!v_u || !v_c || !factors || !ws || !params) TMIX_FAIL(TMIX_EINVAL, "%s: null pointer", me);
    if (dtype != TMIX_F32 && dtype != TMIX_F16 && dtype != TMIX_BF16) TMIX_FAIL(TMIX_EINVAL, "%s: bad dtype %d", me, dtype);
    if (g_slot < 0 || g_slot > 7) TMIX_FAIL(TMIX_EINVAL, "%s: g_slot %d outside 0..7", me, g_slot);
    if (!(phi >= 0.0f && phi <= 1.0f)) TMIX_FAIL(TMIX_EINVAL, "%s: phi %g outside [0, 1]", me, (double)phi);
    if (videos < 1 || videos > 65535) TMIX_FAIL(TMIX_ESHAPE, "%s: videos=%d (1..65535)", me, videos);
    if (n_per_video < 2) TMIX_FAIL(TMIX_ESHAPE, "%s: a standard deviation needs n >= 2 elements per video, got %lld", me, (long long)n_per_video);
    if (stride_u < n_per_video || stride_c < n_per_video)
        TMIX_FAIL(TMIX_ESHAPE, "%s: strides %lld / %lld < one video's %lld elements", me, (long long)stride_u, (long long)stride_c, (long long)n_per_video);
    return for_dtype(dtype, me, "dtype", [&](auto dt) {
        return launch_vpred_rescale<dt()>(v_u, stride_u, v_c, stride_c, factors, ws, videos, n_per_video, params, g_slot, phi, (hipStream_t)stream);
    });
}
