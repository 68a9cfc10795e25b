/* tmix_apg.h -- extension of the C ABI of libtmix_hip.so (include/tmix.h): adaptive projected guidance for the image sampler's fused step.
 * The conventions, error codes and dtype ids are tmix.h's, which this header includes; tmix.h itself is unchanged and declares none of these.
 * tweediemix_amd/lib.py binds them from SIGNATURES_APG. */
#ifndef TMIX_APG_H
#define TMIX_APG_H

#include "tmix.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ADAPTIVE PROJECTED GUIDANCE (no reference counterpart; Sadat, Hilliges and Weber, arXiv:2410.02416): guidance formed on the rows'
 * Tweedie estimates, with the part of the update parallel to the conditional estimate scaled by eta and the update's norm clipped at R.
 * For eps row r >= 1 of a guided call (row 0 the unconditional eu, row r the conditional ec), element i, state value xv = x[i], sa = params[1],
 * s1 = params[2], every product, sum and quotient its own fp32 operation (rnd: to fp16 and back when eps is fp16, else nothing):
 *   tc = (xv - rnd(s1 ec)) / sa        tu = (xv - rnd(s1 eu)) / sa  (once per element)        d = tc - tu
 *   t_r = A_r tc + B_r d               two products, one sum
 * t_r takes the place of the row's t in the blended estimate of all three modes (FUSION blend, PLAIN, RESAMPLE's (K-1) t_1 - sum t_{2+c});
 * everything behind it is the parent entry's: the mask blend, the DDIM move (its noise term stays eu), the multistep move, the noise.
 * tmix_apg_coeffs writes coeffs [seeds][rows-1][2] = {A_r, B_r} for x [seeds][n], eps [seeds][rows][n] (n = channels*hw):
 *   Sdd = sum d d, Sdc = sum d tc, Scc = sum tc tc over the row's n elements: d and tc the fp32 values above, products and sums in fp64
 *   s = (R > 0 and Sdd > R R) ? R / sqrt(Sdd) : 1          p = Scc > 0 ? s Sdc / Scc : 0          g = params[g_slot], read ON THE DEVICE
 *   A = 1 - (g - 1)(1 - eta) p          B = (g - 1) s          in fp64, each rounded once to fp32
 * which gives D = D_c + (g - 1)(D_orth + eta D_par) on the clipped update s d.  OUR choices: {A, B} = {1, g - 1} (plain CFG in data space) where
 * a sum is not finite, and for the rows the mode does not read (PLAIN reads r = 1; FUSION and RESAMPLE r = 1..K).  {1, g - 1} equals the parent
 * entries mathematically, not bit for bit.  Momentum (the paper's beta) is not implemented.
 *   ws      tmix_cfg_rescale_ws_doubles(rows, seeds) doubles (four per slot, three used); no initial contents required
 * Two launches on `stream`, the method of tmix_cfg_rescale_factors (a fixed partition of 32 workgroups per (row, seed), fp64 sums, no atomics, a
 * workgroup without elements writes zeros): bit-reproducible, and a seed's coefficients do not depend on what it is co-batched with.  Inputs are
 * only read.  TMIX_EINVAL: a null pointer, bad eps_dtype / mode, K < 1 (FUSION, RESAMPLE), g_slot outside 0..7, eta outside [0, 1] or not
 * finite, norm_threshold negative or not finite.  TMIX_ESHAPE: channels / hw / seeds, rows below the mode's need or above 256.  Before any launch.
 * tmix_fused_tweedie_step_apg_dev: the 14 leading arguments of tmix_fused_tweedie_step_dev, then
 *   x0_prev  NULL: params {t, sa, s1, sa_next, s1_next, is_last, g, -} and the DDIM move (FUSION, PLAIN, RESAMPLE); else the history buffer,
 *            params {t, sa, s1, cx, c0, c1, is_last, g} and tmix_fused_tweedie_step_ms_dev's move (FUSION, PLAIN).  g is not read: it is inside B.
 *   coeffs   [seeds][rows-1][2] (tmix_apg_coeffs)
 *   keys     NULL: no noise, 8 floats are read and w, n_win, win_yx, canvas_h, canvas_w are not; else tmix_fused_tweedie_step_noise_dev's keys,
 *            window table and 12 floats {.., cz, step_index, 0, 0} (FUSION, PLAIN)
 * x may alias out_x.  TMIX_EINVAL: null x / eps / out_x / params / coeffs, a bad mode, RESAMPLE with x0_prev or keys, FUSION without masks or
 * K >= 1, a bad eps dtype, with keys the noise entry's n_win check.  TMIX_ESHAPE: channels / hw / seeds, rows below the mode's need, with keys
 * the noise entry's hw % w, seeds % n_win and window checks.  All before any launch; one launch on `stream`, capturable. */
int tmix_apg_coeffs(const float* x, const void* eps, int eps_dtype, float* coeffs, double* ws, int K, int channels, int64_t hw, int mode,
                    int rows, int seeds, const float* params, int g_slot, float eta, float norm_threshold, void* stream);
int tmix_fused_tweedie_step_apg_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                    float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                    const float* params, float* x0_prev, const float* coeffs, const uint32_t* keys, int w, int n_win,
                                    const int* win_yx, int canvas_h, int canvas_w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TMIX_APG_H */
