/* tmix.h -- C ABI of libtmix_hip.so, the MI355X (gfx950) kernels behind the Tweedie-mix
 * denoising loop.
 *
 * The reference (KwonGihyun/TweedieMix) is pure Python and has no FFI of its own: its seams are
 * the Python call sites listed below.  Each entry point here replaces the arithmetic behind one of
 * those call sites; tweediemix_amd/ binds them with ctypes (see INTEGRATION.md for the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes.  Every pointer is a BORROWED device pointer (the caller
 *    -- PyTorch's allocator in our host code -- owns the memory).  Nothing here allocates or frees.
 *  - every launch function takes the hipStream_t to enqueue on (as void*), is asynchronous, never
 *    synchronises, and is capturable into a hipGraph.
 *  - return value: 0 = ok, <0 = TMIX_E* argument error (nothing was launched), >0 = hipError_t.
 *    tmix_last_error_string() gives a thread-local description of the last non-zero return.
 *  - bf16 = raw uint16 storage, row-major.  Activations are NHWC ([B, H*W, C]); Linear weights are
 *    torch layout [N_out, K_in]; conv weights are OHWI [C_out, 3, 3, C_in].
 */
#ifndef TMIX_H
#define TMIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMIX_VERSION 100

enum { TMIX_OK = 0, TMIX_EINVAL = -1, TMIX_ESHAPE = -2, TMIX_EARCH = -3, TMIX_EALIGN = -4 };
enum { TMIX_F32 = 0, TMIX_F16 = 1, TMIX_BF16 = 2 };

int tmix_version(void);
const char* tmix_last_error_string(void);
/* 0 if the current device is gfx950, TMIX_EARCH otherwise, >0 on HIP errors. */
int tmix_check_device(void);
/* The library's debug / A-B environment switches (TMIX_GN_NO_SMALL, TMIX_ATTN_NO_SPLIT, TMIX_ATTN_GENERAL, TMIX_NARROW_EPILOGUE) are read ONCE per process, on first
 * use, so that a launch, the query that accounts for it (tmix_groupnorm_nhwc_launches, tmix_attn_split_ws_bytes) and a captured graph all see one value.  This re-reads
 * them (a test that flips a switch mid-process).  No reference counterpart. */
void tmix_env_refresh(void);

/* In-situ launch timing (measurement only; no reference counterpart).  Between tmix_prof_begin and tmix_prof_end every
 * tmix_gemm_bf16 / tmix_conv3x3_nhwc / tmix_attn_fwd / tmix_groupnorm_nhwc launch issued by THIS host thread -- also while
 * it is being captured into a hipGraph -- takes the next 8-word slot of `slots` (device memory, capacity slots) and records
 * into it, in ticks of the 100 MHz realtime clock: {start, end, sum(first operands landed - start), sum(main loop done -
 * start), sum(workgroup end - start), workgroups, -, -}.  detail = 0: start is stored by the first workgroup, end by every
 * workgroup (the last store wins), nothing else -- negligible cost, accurate to a store latency; detail = 1 (GEMM / conv /
 * attention): exact min / max and the per-workgroup phase sums through atomics (this perturbs launches with thousands of
 * workgroups).  The caller initialises every slot to {UINT64_MAX, 0, 0, 0, 0, 0, 0, 0} before each measured run / replay.
 * tmix_prof_end returns the number of slots handed out.  Launches outside such a bracket carry no instrumentation. */
int tmix_prof_begin(uint64_t* slots, int capacity, int detail);
int tmix_prof_end(void);

/* ---------------------------------------------------------------------------------------------
 * Fused CFG + Tweedie x0 + mask blend + DDIM update.
 * Replaces fusion_generation/fusion_sampling.py:376-385,430,471-472 (fusion branch),
 * :392-403 (resampling, first half), :406-412 / :424-430 / :436-447 (plain CFG / jumping).
 *   x        [n]            fp32 latent (one sample, n = C*h*w)
 *   eps      [rows, n]      UNet output, dtype eps_dtype (row 0 = unconditional)
 *   masks    [K, hw]        fp32 blend weights (FUSION only; broadcast over the C channels)
 *   out_x    [n]            fp32 next latent  (x0 itself when is_last)
 *   out_x0   [n] or NULL    fp32 Tweedie estimate
 * modes: FUSION   rows=K+1 : x0 = sum_c m_c * T(x, cfg(e0,e_{1+c}))
 *        PLAIN    rows=2   : x0 = T(x, cfg(e0,e1))
 *        RESAMPLE rows=K+1 : x0 = (K-1)*T(x,cfg(e0,e1)) - sum_{c<K-1} T(x,cfg(e0,e_{2+c}))
 *   with T(x,e) = (x - s1*e)/sa and out = sa_next*x0 + s1_next*e0.
 * sa=sqrt(at), s1=sqrt(1-at), *_next likewise for the target timestep (computed by the host in fp32).
 * eps_dtype F16 reproduces the reference's autocast rounding points (CFG combine and s1*e in
 * fp16, everything else fp32); BF16/F32 eps are combined in fp32.
 */
enum { TMIX_STEP_FUSION = 0, TMIX_STEP_PLAIN = 1, TMIX_STEP_RESAMPLE = 2 };
int tmix_fused_tweedie_step(const float* x, const void* eps, int eps_dtype, const float* masks,
                            float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode,
                            float g, float sa, float s1, float sa_next, float s1_next, int is_last,
                            void* stream);
/* The same step with its coefficients in DEVICE memory, for hipGraph capture of a whole denoising step (the loop body of
 * fusion_sampling.py:490-494 becomes one graph replay per timestep): params = fp32 {t, sa, s1, sa_next, s1_next,
 * is_last (0/1), g, -}.  `seeds` co-batched trajectories run in one launch: x / out_x / out_x0 are [seeds][n], eps is
 * [seeds][rows][n] (rows = the UNet batch rows per seed), masks [seeds][K][hw] with mask_seed_stride = K*hw (0: one mask
 * set shared by all seeds).  x may alias out_x (in-place update of the latent state).  Bit-identical to the scalar form. */
int tmix_fused_tweedie_step_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                int64_t hw, int mode, int rows, int seeds, const float* params, void* stream);
/* tmix_fused_tweedie_step_dev with a KEEP REGION (no reference counterpart: the reference can only re-sample a whole image): part of the
 * latent is held at a given clean latent while the loop runs on the rest -- re-roll one concept of a finished image, or sample concepts
 * into a template image.  Everything tmix_fused_tweedie_step_dev takes, same order, same meaning, then per seed
 *   keep_x0  [n]   fp32 clean latent to hold        keep_eps [n] fp32 its fixed noise        keep_w [hw] fp32 weight of the kept part in [0, 1]
 *   (broadcast over the channels); seed s reads each array at s * its seed stride, 0 = one array shared by all seeds, otherwise >= n (hw).
 * After x0 and moved = sa_next*x0 + s1_next*e0 of the mode (unchanged), per element i with w = keep_w[i % hw]:
 *   kept   = is_last ? keep_x0[i] : sa_next*keep_x0[i] + s1_next*keep_eps[i]        new = is_last ? x0 : moved
 *   out_x  = w*kept + (1 - w)*new                 out_x0 = w*keep_x0[i] + (1 - w)*x0
 * in fp32, two products and one sum each, not contracted: w = 0 gives exactly new (tmix_fused_tweedie_step_dev's result), w = 1 exactly
 * kept.  The kept part is thus always at the noise level of the state it is written into (sa_next / s1_next come from params: one captured
 * launch serves every timestep).  x may alias out_x; the keep arrays alias no output.  TMIX_EINVAL on a null keep pointer, TMIX_ESHAPE on
 * a non-zero seed stride shorter than its extent; otherwise the checks of tmix_fused_tweedie_step_dev. */
int tmix_fused_tweedie_step_keep_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                     int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                     int64_t hw, int mode, int rows, int seeds, const float* params,
                                     const float* keep_x0, int64_t keep_x0_seed_stride, const float* keep_eps,
                                     int64_t keep_eps_seed_stride, const float* keep_w, int64_t keep_w_seed_stride, void* stream);
/* tmix_fused_tweedie_step_dev with a SECOND-ORDER MULTISTEP move (no reference counterpart: the reference is first-order DDIM): the
 * DPM-Solver++(2M) update in data-prediction form on the mode's x0 -- in FUSION mode the blended estimate -- and the x0 of the step before.
 *   params   fp32 {t, sa, s1, cx, c0, c1, is_last (0/1), g}: sa = sqrt(at), s1 = sqrt(1-at) of the CURRENT timestep (what x0 needs);
 *            cx = s1_next/s1, c0, c1 the solver's coefficients, computed by the host in fp64 and rounded once (solver.multistep_coeffs);
 *            c1 = 0 is a first-order step.  NOT the layout of tmix_fused_tweedie_step_dev's params: g is the last float here.
 *   x0_prev  [seeds][n] fp32, read AND written: the history buffer.  It aliases no other argument.
 * Everything else is tmix_fused_tweedie_step_dev's argument of that name.  x0 is computed by that entry's operations in that order, so
 * out_x0 is bit-identical to its out_x0.  Then per element i, in fp32, every product and sum its own operation (not contracted):
 *   p = x0_prev[i]        m = c0*x0;  if (c1 != 0) m = m + c1*p        out_x[i] = is_last ? x0 : cx*x[i] + m
 *   x0_prev[i] = x0       out_x0[i] = x0 (when given)
 * p is not used when c1 == 0: a first-order step may be run on a history buffer that holds anything, NaN included.  x may alias out_x.
 * modes FUSION and PLAIN; TMIX_EINVAL for RESAMPLE (its re-noising half moves away from the data, which the formula does not cover) and for
 * a null x0_prev; otherwise the checks of tmix_fused_tweedie_step_dev. */
int tmix_fused_tweedie_step_ms_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                   int64_t mask_seed_stride, float* out_x, float* out_x0, float* x0_prev, int K, int channels,
                                   int64_t hw, int mode, int rows, int seeds, const float* params, void* stream);
/* GUIDANCE RESCALE (no reference counterpart; Lin et al., arXiv:2305.08891, section 3.4, diffusers' `guidance_rescale`): every guided prediction
 * e_r = cfg(eps_0, eps_r, g) a step forms is scaled back towards the standard deviation of the conditional prediction eps_r it came from.
 * tmix_cfg_rescale_factors writes, for `seeds` seeds over eps [seeds][rows][n] (n = channels*hw), factors [seeds][rows-1] fp32:
 *   e_r[i]  = the step kernels' cfg (three operations, each rounded to fp16 when eps_dtype is TMIX_F16), g = params[g_slot] read ON THE DEVICE
 *             (g_slot 6: the params of tmix_fused_tweedie_step_dev, 7: of tmix_fused_tweedie_step_ms_dev; params holds >= 8 floats)
 *   sd_c, sd_e  the standard deviations of eps_r and of e_r over the row's n elements (denominator n - 1), in fp64
 *   factors[s][r-1] = fp32( phi*sd_c/sd_e + (1 - phi) ), evaluated in fp64 and rounded once;
 *                     1.0f where sd_e is zero or a variance is not finite (OUR choice: diffusers produces inf / nan there)
 * for the rows the mode reads -- PLAIN: r = 1; FUSION and RESAMPLE: r = 1..K -- and 1.0f for every other r.  Statistics are per UNet row.
 *   ws      device workspace of tmix_cfg_rescale_ws_doubles(rows, seeds) doubles (0: rows outside 2..256 or seeds outside 1..65535), 8-byte
 *           aligned; no initial contents required (every slot is written before it is read)
 * Two launches on `stream`: partial sums over a fixed partition of every row (independent of the data, no atomics), then one lane per
 * (seed, row) adds them in index order -- the factors are bit-reproducible run to run.  eps and params are only read.
 * TMIX_EINVAL: a null pointer, bad eps_dtype / mode, K < 1 (FUSION, RESAMPLE), g_slot outside 0..7, phi outside [0, 1] or not finite.
 * TMIX_ESHAPE: n < 2, rows below the mode's need (PLAIN 2, else K + 1) or above 256, seeds outside 1..65535.  All before any launch.
 * tmix_fused_tweedie_step_rs_dev / _ms_rs_dev: tmix_fused_tweedie_step_dev / _ms_dev with one more argument, `factors` [seeds][rows-1] (behind
 * params): wherever the step uses e_r it uses rnd(factors[s][r-1] * e_r) (rnd: to fp16 for TMIX_F16, else nothing) -- FUSION rows 1..K, PLAIN
 * row 1, RESAMPLE the multi-concept row 1 and the single rows 2..K.  The move's noise term stays eps_0; everything else is the parent entry's.
 * With all factors 1.0f the results are the parent entry's bit for bit.  TMIX_EINVAL on null factors; otherwise the parent's checks. */
int64_t tmix_cfg_rescale_ws_doubles(int rows, int seeds);
int tmix_cfg_rescale_factors(const void* eps, int eps_dtype, float* factors, double* ws, int K, int channels, int64_t hw, int mode,
                             int rows, int seeds, const float* params, int g_slot, float phi, void* stream);
int tmix_fused_tweedie_step_rs_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                   int64_t mask_seed_stride, float* out_x, float* out_x0, int K, int channels,
                                   int64_t hw, int mode, int rows, int seeds, const float* params, const float* factors, void* stream);
int tmix_fused_tweedie_step_ms_rs_dev(const float* x, const void* eps, int eps_dtype, const float* masks,
                                      int64_t mask_seed_stride, float* out_x, float* out_x0, float* x0_prev, int K, int channels,
                                      int64_t hw, int mode, int rows, int seeds, const float* params, const float* factors, void* stream);
/* STOCHASTIC STEPS (no reference counterpart in the hot path: the reference's pipelines carry `eta` to their schedulers).  The
 * noise of an element is a pure function of (trajectory key, canvas index, schedule step, stream id): one Philox4x32-10 call (Salmon et al.,
 * SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) with key = {key_lo, key_hi} and counter = {index low
 * word, index high word, step, stream_id}, then Box-Muller on output words 0 and 1:
 *   u1 = ((w0 >> 9) + 0.5) * 2^-23        angle = 2 pi ((w1 >> 9) + 0.5) * 2^-23        z = sqrt(-2 ln u1) cos(angle),   |z| < 5.8
 * with ln, sin and cos written out in integer operations and single-rounded fp32 add, sub, mul, div and sqrt (csrc/noise.h), so that
 * noise.normal (numpy) gives the same bits.  stream_id 0 is the image sampler's step, 1 the video sampler's, 2 the fixed noise of its hold regions (7p); other values are reserved.
 * tmix_noise_normal: the generator on its own: z[i] = the normal of index first_index + i, i < n.  TMIX_EINVAL: null z.  TMIX_ESHAPE: n < 1,
 * first_index < 0.
 * tmix_fused_tweedie_step_noise_dev: ONE entry for the stochastic form of tmix_fused_tweedie_step_dev / _rs_dev / _ms_dev / _ms_rs_dev.  The
 * arguments of tmix_fused_tweedie_step_dev, then
 *   x0_prev  NULL: the DDIM params layout and move (parent tmix_fused_tweedie_step_dev); else the history buffer: the multistep layout and move
 *   factors  NULL: no guidance rescale; else [seeds][rows-1] with the meaning it has in the parent's _rs_dev form
 *   keys     device array uint32 [seeds / n_win][2]: {low word, high word} of every trajectory's 64-bit seed value
 *   w        the row width of the latent; hw % w == 0
 *   n_win, win_yx, canvas_h, canvas_w   tmix_window_consensus's window table (HOST array, passed by value): the `seeds` rows are window-major
 *            inside a trajectory, row r is window r % n_win of trajectory r / n_win, and element (c, y, x) of that window has the index
 *            c*canvas_h*canvas_w + (oy + y)*canvas_w + (ox + x).  win_yx NULL with n_win 1: no canvas, the index is the element's own
 *            c*hw + y*w + x and canvas_h / canvas_w are not read.
 *   params   12 floats: the parent layout's 8, then {cz, step_index, 0, 0}; step_index an integer below 2^24 (exact in fp32)
 * Per element, with x0 and moved (the parent's out_x value before its is_last selection) formed by the parent's operations in its order:
 *   out_x = is_last ? x0 : (cz != 0 ? moved + cz*z : moved)        one product and one sum, not contracted
 * out_x0 and the history write are the parent's.  With cz == 0 all outputs are the parent entry's bit for bit.  Two windows that cover one
 * canvas pixel add the same value there.  TMIX_EINVAL: RESAMPLE mode, null keys, n_win outside 1..TMIX_MAX_WINDOWS (or not 1 without win_yx).
 * TMIX_ESHAPE: hw % w != 0, seeds % n_win != 0, a window that leaves the canvas.  Otherwise the parents' checks; all before any launch. */
int tmix_noise_normal(float* z, int64_t n, int64_t first_index, uint32_t key_lo, uint32_t key_hi, uint32_t step, uint32_t stream_id, void* stream);
int tmix_fused_tweedie_step_noise_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                      float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                      const float* params, float* x0_prev, const float* factors, const uint32_t* keys, int w,
                                      int n_win, const int* win_yx, int canvas_h, int canvas_w, void* stream);
/* UNGUIDED STEPS (guidance interval, arXiv:2404.07724; no reference counterpart).  The step of a UNet call that ran WITHOUT the
 * unconditional row: eps is [seeds][rows][n] with row c the prediction of concept c (FUSION, rows >= K) or row 0 the scene prompt's (PLAIN,
 * rows >= 1).  The arguments of tmix_fused_tweedie_step_dev, then
 *   x0_prev  NULL: the DDIM params layout {t, sa, s1, sa_next, s1_next, is_last, -, -} and move; else the history buffer, read and rewritten:
 *            the multistep layout {t, sa, s1, cx, c0, c1, is_last, -} and move.  The g slot of either layout is ignored.
 *   keys     NULL: no noise, 8 floats are read and w, n_win, win_yx, canvas_h, canvas_w are not; else tmix_fused_tweedie_step_noise_dev's keys,
 *            window table and 12 floats {.., cz, step_index, 0, 0}
 * Per element, every product, sum and quotient its own fp32 operation (rnd: to fp16 and back when eps is fp16, else nothing):
 *   t_c   = (x - rnd(s1 e_c)) / sa          e_c: row c's value itself -- no CFG, no rescale factor
 *   x0    = 0; x0 = x0 + m_c t_c, c = 0..K-1  (FUSION)          x0 = t_0  (PLAIN)          tmix_fused_tweedie_step_dev's arithmetic and order
 *   DDIM:       e0 = s1 != 0 ? (x - sa x0) / s1 : 0,   moved = sa_next x0 + rnd(s1_next e0)      the eps consistent with the blended estimate
 *   multistep:  moved = cx x + (c1 != 0 ? c0 x0 + c1 x0_prev : c0 x0),   x0_prev = x0            tmix_fused_tweedie_step_ms_dev's move
 *   out_x = is_last ? x0 : (cz != 0 ? moved + cz z : moved),   out_x0 = x0 (optional)
 * x may alias out_x.  With the unconditional row a copy of the conditional one the parents give the same x0 (and the multistep parent the same
 * out_x) bit for bit.  TMIX_EINVAL: null x / eps / out_x / params, a mode other than FUSION / PLAIN, FUSION without masks or K >= 1, a bad eps
 * dtype, with keys the noise entry's n_win check.  TMIX_ESHAPE: channels / hw / seeds, rows < K (FUSION) or < 1 (PLAIN), with keys the noise
 * entry's hw % w, seeds % n_win and window checks.  All before any launch. */
int tmix_fused_tweedie_step_cond_dev(const float* x, const void* eps, int eps_dtype, const float* masks, int64_t mask_seed_stride,
                                     float* out_x, float* out_x0, int K, int channels, int64_t hw, int mode, int rows, int seeds,
                                     const float* params, float* x0_prev, const uint32_t* keys, int w, int n_win, const int* win_yx,
                                     int canvas_h, int canvas_w, void* stream);
/* Head of the captured step (fusion_sampling.py:324-327, `latent_model_input = torch.cat([x] * rows)`, and the timestep
 * argument of the UNet call :340): latent[(s*rows + r)][n] = x[s][n] for every row r, t_dev[s*rows + r] = params[0]. */
int tmix_step_prologue(const float* x, float* latent, float* t_dev, const float* params, int seeds, int rows,
                       int64_t n, void* stream);
/* WIDE CANVASES (no reference counterpart: the reference samples one image of the trained size).  A canvas larger than the trained
 * window is sampled as n_win overlapping windows that share every UNet launch like co-batched seeds; after every step the windows are
 * reconciled: each canvas pixel that several windows cover becomes, in all of them, the weighted mean of their values.
 *   x        [groups][n_win][C][h][w] fp32, dense, updated in place (groups = co-batched seeds; window-major inside a group)
 *   win_yx   HOST array of 2*n_win ints {oy_0, ox_0, oy_1, ...}: the windows' top-left corners on the canvas.  Read at call time and
 *            passed in the kernel arguments, so a captured launch carries them by value (n_win <= TMIX_MAX_WINDOWS)
 *   weight   [h*w] fp32 device array, one weight per WINDOW pixel, or NULL = all ones
 * For every group, channel and canvas pixel, over the windows i that cover it in ascending i, with v_i the window's element and wt_i its weight:
 *   acc = acc + wt_i * v_i     ws = ws + wt_i     (from 0.0f; separate products and sums, not contracted)     r = acc / ws
 * and r is written to that element of every covering window.  A pixel that ONE window covers is not written: its bits stay (NaN payloads
 * included).  One thread owns one canvas pixel and a window element belongs to exactly one canvas pixel: no atomics, results independent
 * of the grid.  No alignment requirement on h or w.  n_win == 1 succeeds and launches nothing.
 * TMIX_EINVAL: null x / win_yx, n_win outside 1..TMIX_MAX_WINDOWS, groups < 1.  TMIX_ESHAPE: a non-positive size, a window that reaches
 * outside the canvas, a canvas pixel that no window covers.  All checked on the host before any launch. */
#define TMIX_MAX_WINDOWS 8
int tmix_window_consensus(float* x, int groups, int n_win, const int* win_yx, int C, int h, int w, int canvas_h, int canvas_w,
                          const float* weight, void* stream);
/* SOFT REGION MASKS (no reference counterpart: the reference blends with hard {0, 1} stencils).  Blend weights from the distance to each
 * region's border, on the grid the masks are built on (DESIGN.md 7g holds the definition).
 * tmix_mask_edt: exact squared Euclidean distances.  mask [n][h][w] fp32, a pixel is SET where the value is >= 0.5;
 *   d_set[p]   = min over set pixels q of |p - q|^2 (int32, 0 on set pixels),  d_clear[p] the same towards clear pixels;
 *   a mask without a set (clear) pixel gives TMIX_EDT_NONE everywhere in d_set (d_clear).  1 <= h, w <= 4096, 1 <= n <= 65535.
 *   Two launches (columns, then rows through LDS); no workspace, no atomics; integer minima, so independent of order and grid.
 * tmix_soft_masks: d_set / d_clear [n_sets][K-1][h][w] -> out [n_sets][K][h][w] fp32.  Per pixel and foreground concept k, in fp32, every
 *   op rounded on its own:   s = d_set == 0 ? -(sqrtf(d_clear) - 0.5f) : sqrtf(d_set) - 0.5f     s' = s - dilate
 *                            u_k = feather > 0 ? min(max(0.5f - s' / feather, 0), 1) : (s' < 0 ? 1 : 0)
 *   t = u_1 + ... + u_{K-1} ascending; normalize == 0: w_k = u_k, bg = max(1 - t, 0); normalize != 0: t > 1 ? (w_k = u_k / t, bg = 0) :
 *   (w_k = u_k, bg = 1 - t).  dilate = 0 with feather <= 1 returns the thresholded mask itself.  feather and dilate in pixels of the grid.
 * Both: TMIX_EINVAL on a null pointer, on feather < 0 or not finite, on a dilate that is not finite; TMIX_ESHAPE on sizes outside the
 * ranges above or K < 2.  All checked on the host before any launch; both run on `stream` and are capturable. */
#define TMIX_EDT_NONE (1 << 30)
int tmix_mask_edt(const float* mask, int32_t* d_set, int32_t* d_clear, int n, int h, int w, void* stream);
int tmix_soft_masks(const int32_t* d_set, const int32_t* d_clear, float* out, int n_sets, int K, int h, int w, float feather,
                    float dilate, int normalize, void* stream);
/* FREE-FORM ATTENTION MASKS (no reference counterpart: the side-car turns every mask into its bounding rectangle).  Connected components on
 * the attention grid, 4-connected for set and for clear pixels, pixels in raster order i = y * w + x (DESIGN.md 7h holds the definition).
 * tmix_mask_label: map [n][h][w] fp32, a pixel is SET where map >= threshold (compared in fp32).  label [n][h][w] int32: for a set pixel
 *   (invert != 0: for a clear pixel) the smallest raster index of its component, -1 for the pixels of the other kind.
 * tmix_attn_shapes: score [n_sets][km1][h][w] fp32 -> out [n_sets][km1][h][w] fp32 in {0, 1}.  Per map k: b_k = score_k >= threshold; c_k = the
 *   component of b_k with the most pixels (equal counts: the smallest label; an empty b_k gives an empty c_k); with TMIX_SHAPE_FILL_HOLES
 *   f_k = c_k plus every component of the complement OF c_k that has no pixel in row 0, row h-1, column 0 or column w-1 (else f_k = c_k); with
 *   TMIX_SHAPE_RESOLVE a pixel in several f_k of a set stays only in the k with the largest score there (fp32 >, equal scores: the smallest k;
 *   nothing is re-labelled afterwards).
 * One workgroup per map with the labels in LDS (a union-find whose merges only lower labels: every loop is bounded by h * w, no workgroup or
 * lane waits for another), integer atomics only: results depend on the input alone, not on launch geometry or execution order.  One launch
 * (tmix_attn_shapes with TMIX_SHAPE_RESOLVE and km1 > 1: two); no workspace.
 * Both: TMIX_EINVAL on a null pointer, on a threshold that is not finite, on unknown flag bits; TMIX_ESHAPE on h, w, n, n_sets or km1 below 1,
 * on h * w > TMIX_SHAPE_MAX_PIXELS, on n or n_sets * km1 above 65535.  All checked on the host before any launch; both run on `stream` and
 * are capturable. */
#define TMIX_SHAPE_FILL_HOLES 1
#define TMIX_SHAPE_RESOLVE    2
#define TMIX_SHAPE_MAX_PIXELS 16384   /* 128 x 128: the attention grid of a 2048^2 image */
int tmix_mask_label(const float* map, float threshold, int invert, int32_t* label, int n, int h, int w, void* stream);
int tmix_attn_shapes(const float* score, float* out, int n_sets, int km1, int h, int w, float threshold, int flags, void* stream);

/* Video sampler (I2VGen-XL loop, BASELINE config #5; replaces video_gen/pipeline_i2vgen_xl.py:699-719):
 *   x [n], v [2n] (uncond rows first), out [n], all of `dtype` (TMIX_F32 / TMIX_F16 / TMIX_BF16); sa = sqrt(alpha(t)) etc. with
 *   the UN-shifted table of that pipeline (:480-482).  v' = v_u + g (v_t - v_u); eps = sa v' + s1 x; x0 = sa x - s1 v';
 *   out = sa_next x0 + s1_next eps.  TMIX_F16 rounds after every binary op like the reference's fp16 tensors. */
int tmix_vpred_step(const void* x, const void* v, void* out, int dtype, int64_t n, float g,
                    float sa, float s1, float sa_next, float s1_next, void* stream);
/* Batched video step (S videos in one UNet call; tweediemix_amd.video.VideoSampler).  Both read the device parameter buffer
 * params = {t, sa, s1, sa_next, s1_next, g, ...} (fp32), so ONE captured launch serves every timestep of a graph replay.
 * The state x is fp32 in the pipeline layout [videos][channels][frames][hw].  A CFG half (u = unconditional, c = text) is a plan
 * buffer of per-frame rows [(clip*frames + f)][row channels][hw] whose clip s starts at s * clip_stride floats: two chains of
 * `videos` clips each, or one plan of 2*videos clips with the text half's base pointer at clip `videos`.
 * tmix_video_step_prologue: x -> channels [0, channels) of both halves' input rows (row_channels per row; the image-latent
 *   channels [channels, row_channels) are never written), t_u[0..videos) = t_c[0..videos) = params[0].
 * tmix_vpred_step_dev: x <- tmix_vpred_step(x, [v_u; v_c]) (TMIX_F32) element for element, in place, with v_u / v_c read from the
 *   halves' prediction rows ([(clip*frames + f)][channels][hw]) -- bit-identical to that kernel on the same video.
 * Both: TMIX_EINVAL on a null pointer, TMIX_ESHAPE on an empty shape or a clip stride shorter than one clip. */
int tmix_video_step_prologue(const float* x, float* x_u, int64_t clip_stride_u, float* t_u, float* x_c, int64_t clip_stride_c,
                             float* t_c, const float* params, int videos, int channels, int frames, int64_t hw, int row_channels,
                             void* stream);
int tmix_vpred_step_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                        const float* params, int videos, int channels, int frames, int64_t hw, void* stream);
/* DPM-Solver++(2M) form of the video step (no reference counterpart).  With v' and x0 = sa x - s1 v' formed exactly as in
 * tmix_vpred_step (the same operations in the same order, so x0 is that kernel's x0 bit for bit), p = x0_prev[i] read first:
 *   m = c0 x0; if (c1 != 0) m = m + c1 p; out[i] = cx x + m; x0_prev[i] = x0
 * -- every binary operation a separate one, rounded as in tmix_vpred_step for TMIX_F16.  cx, c0, c1 come from the host (solver.py); c1 == 0
 * is a first-order step and p then never reaches the output (a NaN-filled history is fine).
 * tmix_vpred_step_ms: x [n], v [2n] (uncond rows first), out [n] of `dtype`; x0_prev [n] is ALWAYS fp32, is read and written and aliases
 *   nothing; out may alias x.
 * tmix_vpred_step_ms_dev: the TMIX_F32 form for `videos` videos, in place on x [videos][channels][frames][hw] with x0_prev of the same layout and
 *   v_u / v_c read from the halves' prediction rows exactly as tmix_vpred_step_dev reads them; params = {t, sa, s1, cx, c0, c1, g, 0} (fp32, device;
 *   NOT tmix_vpred_step_dev's layout; params[0] stays t, so tmix_video_step_prologue is shared).  Bit-identical to the scalar form per element.
 * Both: TMIX_EINVAL on a null pointer (x0_prev included) or a bad dtype, TMIX_ESHAPE on an empty shape or a clip stride shorter than one clip,
 * all checked on the host before any launch; one launch on `stream`, capturable; no workspace. */
int tmix_vpred_step_ms(const void* x, const void* v, void* out, float* x0_prev, int dtype, int64_t n, float g,
                       float sa, float s1, float cx, float c0, float c1, void* stream);
int tmix_vpred_step_ms_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                           const float* params, int videos, int channels, int frames, int64_t hw, void* stream);
/* GUIDANCE RESCALE of the video step (no reference counterpart; arXiv:2305.08891 section 3.4 = diffusers' rescale_noise_cfg on the v-prediction,
 * per video).  One video has n = channels*frames*hw elements.  With v'[i] = the step kernels' cfg(v_u[i], v_c[i], g):
 *   sd_c, sd_v = the standard deviations of v_c and of v' over the video's n elements (denominator n - 1), in fp64
 *   f          = fp32( phi*sd_c/sd_v + (1 - phi) ), evaluated in fp64 from the fp32 phi and rounded once; 1.0f where sd_v is zero or a variance
 *                is not finite (the rule of tmix_cfg_rescale_factors)
 *   v''[i]     = rnd(f * v'[i])   (rnd: to fp16 for TMIX_F16, else nothing)
 * and v'' takes the place of v' EVERYWHERE in the step: in x0 = sa x - s1 v'' and in eps = sa v'' + s1 x (both come from the one model output;
 * unlike tmix_fused_tweedie_step_rs_dev, whose move keeps the unconditional row as its noise term).
 * tmix_vpred_rescale_factors writes factors[videos].  Video s is the n_per_video CONTIGUOUS elements of `dtype` at v_u + s*stride_u and at
 *   v_c + s*stride_c (strides in elements; the order inside a video does not matter to a standard deviation): the plan's two half buffers with their
 *   clip strides, one plan buffer of 2*videos clips with v_c based at clip `videos`, or a dense [2][videos][n] array with v_c = v_u + videos*n.
 *   g = params[g_slot] is read ON THE DEVICE (slot 5: the params of tmix_vpred_step_dev, 6: of tmix_vpred_step_ms_dev; params holds >= 8 floats).
 *   ws: tmix_cfg_rescale_ws_doubles(2, videos) doubles, no initial contents required.  Two launches on `stream`, the method of
 *   tmix_cfg_rescale_factors (a fixed partition of 32 workgroups per video, fp64 sums, no atomics): bit-reproducible, and the factor of a video does
 *   not depend on how many videos share the call.  The inputs are only read.
 *   TMIX_EINVAL: a null pointer, a bad dtype, g_slot outside 0..7, phi outside [0, 1] or not finite.  TMIX_ESHAPE: videos outside 1..65535,
 *   n_per_video < 2, a stride shorter than n_per_video.  All before any launch.
 * tmix_vpred_step_rs / _ms_rs: tmix_vpred_step / _ms on [videos][n_per_video] (v: [2][videos][n_per_video]) with one more argument, factors [videos]:
 *   element i uses factors[i / n_per_video].  tmix_vpred_step_rs_dev / _ms_rs_dev: tmix_vpred_step_dev / _ms_dev with factors [videos] behind hw.
 *   With all factors 1.0f the results are the parent entry's bit for bit.  TMIX_EINVAL on null factors; otherwise the parent's checks. */
int tmix_vpred_rescale_factors(const void* v_u, int64_t stride_u, const void* v_c, int64_t stride_c, int dtype, float* factors, double* ws,
                               int videos, int64_t n_per_video, const float* params, int g_slot, float phi, void* stream);
int tmix_vpred_step_rs(const void* x, const void* v, void* out, int dtype, int videos, int64_t n_per_video, float g,
                       float sa, float s1, float sa_next, float s1_next, const float* factors, void* stream);
int tmix_vpred_step_rs_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c,
                           const float* params, int videos, int channels, int frames, int64_t hw, const float* factors, void* stream);
int tmix_vpred_step_ms_rs(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t n_per_video, float g,
                          float sa, float s1, float cx, float c0, float c1, const float* factors, void* stream);
int tmix_vpred_step_ms_rs_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, float* x0_prev,
                              const float* params, int videos, int channels, int frames, int64_t hw, const float* factors, void* stream);
/* STOCHASTIC VIDEO STEPS (no reference counterpart): the noise of tmix_fused_tweedie_step_noise_dev (above) in the video step, ONE
 * entry per layout for the stochastic form of all four parents.  Element i of video s = i / n_per_video draws
 *   z = the normal of (index i % n_per_video, key {keys[s][0], keys[s][1]}, step, stream_id 1)
 * -- its own linear index in its video's [channels][frames][hw] layout under its video's key, stream id 1 (0 is the image sampler's step, so the
 * same seed draws unrelated noise there) -- one Philox call per element: z does not depend on `videos`, on the video's place in the batch or on
 * the launch.  With x0, the history write and moved (the parent's stored value before the store's rounding) formed by the parent's operations:
 *   out[i] = cz != 0 ? rnd(moved + rnd(cz * z)) : moved        one product and one sum, not contracted; rnd: to fp16 for TMIX_F16, else nothing
 * (TMIX_BF16 rounds once, at the store).  With cz == 0 no generator call runs and every output is the parent entry's bit for bit.
 * tmix_vpred_step_noise: the dense form on [videos][n_per_video] (v: [2][videos][n_per_video]) of `dtype`.
 *   x0_prev  NULL: the DDIM move, (a, b) = (sa_next, s1_dir) with s1_dir = sqrt(1 - alpha' - sigma^2) and c not read (parents tmix_vpred_step /
 *            _rs); else the fp32 history buffer and the multistep move (a, b, c) = (cx, c0, c1) (parents tmix_vpred_step_ms / _ms_rs); out may
 *            alias x in both
 *   factors  NULL: no guidance rescale; else [videos] as in tmix_vpred_step_rs
 *   keys     device array uint32 [videos][2]: {low word, high word} of every video's 64-bit seed value
 *   step     the schedule index of the step
 * tmix_vpred_step_noise_dev: the form on plan rows: the arguments of tmix_vpred_step_dev, then x0_prev, factors, keys with the same meanings.
 *   params   12 floats: the parent layout's 8 ({t, sa, s1, sa_next, s1_dir, g, 0, 0} without x0_prev, {t, sa, s1, cx, c0, c1, g, 0} with it), then
 *            {cz, step_index, 0, 0}; step_index an integer below 2^24 (exact in fp32).  tmix_video_step_prologue and tmix_vpred_rescale_factors
 *            read the first 8 only.
 * Both: TMIX_EINVAL on a null x, v / v_u, v_c, out / params, on null keys and on a bad dtype; TMIX_ESHAPE on videos, n_per_video / channels, frames
 * or hw below 1 or a clip stride shorter than one clip (null pointers are answered first, the dtype last); all before any launch; one launch
 * on `stream`, capturable; no workspace. */
int tmix_vpred_step_noise(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int64_t n_per_video, float g,
                          float sa, float s1, float a, float b, float c, float cz, const float* factors, const uint32_t* keys, uint32_t step,
                          void* stream);
int tmix_vpred_step_noise_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, const float* params,
                              int videos, int channels, int frames, int64_t hw, float* x0_prev, const float* factors, const uint32_t* keys,
                              void* stream);
/* HOLD REGIONS IN THE VIDEO STEP (no reference counterpart): part of every frame is held at a clean latent while the rest is sampled.
 * For element i = (video s, channel c, frame f, pixel p) of the state [videos][channels][frames][hw]:
 *   kx    hold_x0 [videos or 1][channels][hold_x0_frames][hw] fp32, the clean latent to hold; hold_x0_frames 1: one image for every frame, `frames`:
 *         a whole clip; video s starts at s * hold_x0_video_stride floats (0: one array for every video)
 *   w     hold_w [videos or 1][hold_w_frames][hw] fp32 in [0, 1], 1 = held, 0 = sampled, the same for every channel; strides and frames as above
 *   zh    the normal of (index i % (channels frames hw), key {keys[s][0], keys[s][1]}, step 0, stream_id 2): ONE fixed noise per element at every
 *         noise level, so the held part walks the deterministic path sa_t kx + s1_t zh
 *   ha, hs  sqrt(alpha), sqrt(1 - alpha) of the state the step WRITES; (1, 0) on the last step of a schedule
 *   moved what tmix_vpred_step_noise[_dev] stores for the element (x0, the history write and the rescale statistics are the parent's, over the
 *         whole video, held region included)
 *   kept = hs != 0 ? rnd(rnd(ha * kx) + rnd(hs * zh)) : kx            hs == 0: no generator call, no product, kx with its sign bit
 *   out  = w == 0 ? moved : w == 1 ? kept : rnd(rnd(w * kept) + rnd(rnd(1 - w) * moved))
 * w == 0 leaves the noise entry's bits, w == 1 does not depend on the prediction (a NaN in v stays out of a held pixel).  Nothing is contracted.
 * tmix_vpred_step_hold: the dense form: tmix_vpred_step_noise with (videos, channels, frames, hw) in place of (videos, n_per_video), ha and hs by
 *   value behind `step`, then the hold arrays.
 * tmix_vpred_step_hold_dev: the form on plan rows: the arguments of tmix_vpred_step_noise_dev, then the hold arrays.  params holds 12 floats: the
 *   noise entry's {.., cz, step_index} with {ha, hs} in slots 10 and 11.
 * tmix_video_hold_composite: the blend alone, in place on x of `dtype` with moved = x: x_T once, at the first timestep's (ha, hs).
 * All three: the parent's answers first (TMIX_EINVAL on a null x, v / v_u, v_c, out / params, on null keys; TMIX_ESHAPE on a bad shape or clip stride;
 * TMIX_EINVAL on a bad dtype), then TMIX_EINVAL on a null hold_x0 / hold_w, TMIX_ESHAPE on hold_x0_frames / hold_w_frames not in {1, frames} and on
 * a video stride that is neither 0 nor at least one video's extent (channels * hold_x0_frames * hw, hold_w_frames * hw); all before any launch; one
 * launch on `stream`, capturable; no workspace. */
int tmix_vpred_step_hold(const void* x, const void* v, void* out, float* x0_prev, int dtype, int videos, int channels, int frames, int64_t hw,
                         float g, float sa, float s1, float a, float b, float c, float cz, const float* factors, const uint32_t* keys,
                         uint32_t step, float ha, float hs, const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames,
                         const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream);
int tmix_vpred_step_hold_dev(float* x, const float* v_u, int64_t clip_stride_u, const float* v_c, int64_t clip_stride_c, const float* params,
                             int videos, int channels, int frames, int64_t hw, float* x0_prev, const float* factors, const uint32_t* keys,
                             const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames, const float* hold_w,
                             int64_t hold_w_video_stride, int hold_w_frames, void* stream);
int tmix_video_hold_composite(void* x, int dtype, int videos, int channels, int frames, int64_t hw, float ha, float hs, const uint32_t* keys,
                              const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames, const float* hold_w,
                              int64_t hold_w_video_stride, int hold_w_frames, void* stream);
/* The UNGUIDED video step (the guidance interval of arXiv:2404.07724 in the video loop): a step outside the interval runs the text
 * half alone.  Per element the operations are the guided entries' with v'' = v_c, the conditional prediction itself:
 *   x0    = rnd(rnd(sa * x) - rnd(s1 * v_c))
 *   DDIM  : eps = rnd(rnd(sa * v_c) + rnd(s1 * x)),  moved = rnd(rnd(a * x0) + rnd(b * eps))            (a, b) = (sa_next, s1_next or s1_dir)
 *   2M    : moved = the multistep move of tmix_vpred_step_ms on (x, x0, x0_prev) with (a, b, c) = (cx, c0, c1); x0_prev <- x0
 *   then `+ rnd(cz * z)` of tmix_vpred_step_noise and the blend of tmix_vpred_step_hold, exactly as in those entries.
 * No CFG: there is no unconditional prediction, no g and no factors argument, and a -0.0 prediction keeps its sign.  With guidance rescale an
 * unguided step uses these entries as well and no tmix_vpred_rescale_factors runs (at g = 1 the rescaled prediction is the conditional one).
 * tmix_video_step_prologue_cond: tmix_video_step_prologue for the text half alone: x [videos][channels][frames][hw] fp32 -> channels [0, channels)
 *   of x_c's frame rows [(clip*frames + f)][row_channels][hw] (clip s at s * clip_stride_c floats), params[0] -> t_c [videos].  Nothing else is
 *   written.  TMIX_EINVAL on a null pointer, TMIX_ESHAPE on a bad shape or clip stride (tmix_video_step_prologue's checks).
 * tmix_vpred_step_cond: the dense form in the model dtype: x, out [videos][channels][frames][hw] and v_c of the same shape (NOT [2 videos]); out may
 *   alias x.  ONE entry for every form: x0_prev null: the DDIM move, else the multistep move and the fp32 history (read and rewritten); keys null:
 *   no noise (cz and step are not read), else keys [videos][2] and the noise of tmix_vpred_step_noise; hold_x0 and hold_w both null: no hold, else
 *   the hold of tmix_vpred_step_hold with (ha, hs).
 * tmix_vpred_step_cond_dev: the form on plan rows, in place on x fp32: v_c the text half's prediction rows [(clip*frames + f)][channels][hw], clip s at
 *   s * clip_stride_c floats.  params has the guided entries' layouts unchanged -- 8 floats without keys, 12 with ({.., cz, step_index, ha, hs}) -- so
 *   a sampler uploads the same floats on guided and unguided steps; the g slot (5, or 6 in the multistep layout) is not read.
 * Both step entries: TMIX_EINVAL on a null x, v_c, out / params; TMIX_ESHAPE on a bad shape or clip stride; TMIX_EINVAL on a bad dtype; then
 * TMIX_EINVAL on a hold without keys and on exactly one of hold_x0 / hold_w null, TMIX_ESHAPE on the hold's frame counts and video strides as in
 * tmix_vpred_step_hold; all before any launch; one launch on `stream`, capturable; no workspace. */
int tmix_video_step_prologue_cond(const float* x, float* x_c, int64_t clip_stride_c, float* t_c, const float* params, int videos, int channels,
                                  int frames, int64_t hw, int row_channels, void* stream);
int tmix_vpred_step_cond(const void* x, const void* v_c, void* out, float* x0_prev, int dtype, int videos, int channels, int frames, int64_t hw,
                         float sa, float s1, float a, float b, float c, float cz, const uint32_t* keys, uint32_t step, float ha, float hs,
                         const float* hold_x0, int64_t hold_x0_video_stride, int hold_x0_frames, const float* hold_w,
                         int64_t hold_w_video_stride, int hold_w_frames, void* stream);
int tmix_vpred_step_cond_dev(float* x, const float* v_c, int64_t clip_stride_c, const float* params, int videos, int channels, int frames,
                             int64_t hw, float* x0_prev, const uint32_t* keys, const float* hold_x0, int64_t hold_x0_video_stride,
                             int hold_x0_frames, const float* hold_w, int64_t hold_w_video_stride, int hold_w_frames, void* stream);
/* First-frame feature injection of the patched ResnetBlock2D.forward (video_gen/utils_attn.py:433-455), in place on
 * x [clips][frames][per_frame]: frames 1.. <- frame 0 (hard) or interp*frame0 + one_minus_interp*frame. */
int tmix_frame_inject(void* x, int dtype, int clips, int frames, int64_t per_frame, int hard, float interp,
                      float one_minus_interp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogues:  C[b] = epi(A[b] (MxK) * W[b]^T (NxK)).
 * Replaces the Linear layers inside the UNet call at fusion_sampling.py:340/374/406/414/440
 * (diffusers Attention.to_q/to_k/to_v/to_out, FeedForward, proj_in/out, conv_shortcut) and the
 * per-row concept weights of utils_custom.py:64-83 / utils_lora.py:65-79,113-119 (batch with
 * strideW != 0 selects one weight set per batch row).
 * Requirements: K % 64 == 0, lda/ldw % 8 == 0, 16-byte aligned pointers.
 * Rows of A behind M (the next slice's rows, a neighbouring tensor) and the columns [K, lda) / [K, ldw) may hold any bit pattern, NaN included: the loads of
 * a slice are bounded by its own extent ((M - 1) * lda + K elements), and nothing behind it reaches a result.
 */
enum { TMIX_EPI_NONE = 0, TMIX_EPI_GEGLU = 1, TMIX_EPI_F32OUT = 2 /* C is fp32 [M][ldc] (attention scores of the VAE) */,
       TMIX_EPI_GELU = 3 /* gelu(acc + bias), erf form (OpenCLIP-bigG MLP) */,
       TMIX_EPI_QUICKGELU = 4 /* x * sigmoid(1.702 x) (CLIP-L MLP) */ };
/* workgroup tilings of the MFMA mainloop (BM x BN, waves, LDS ring depth); AUTO = built-in heuristic */
enum { TMIX_TILE_AUTO = 0, TMIX_TILE_128x128_S2 = 1, TMIX_TILE_256x128_S3 = 2, TMIX_TILE_128x128_S4 = 3,
       TMIX_TILE_256x256_S2 = 4, TMIX_TILE_256x128_W4 = 5, TMIX_TILE_256x256_W4 = 6, TMIX_TILE_128x160_S2 = 7,
       /* the same tilings with one extra LOADER wave that issues every LDS-DMA (the math waves only read LDS and issue MFMAs) */
       TMIX_TILE_128x160_S2_LW = 8, TMIX_TILE_256x128_S3_LW = 9, TMIX_TILE_128x128_S2_LW = 10, TMIX_TILE_256x256_S2_LW = 11,
       TMIX_TILE_128x160_S4 = 12 /* tiling 7 with a 4-deep LDS ring (one workgroup per CU) */,
       TMIX_TILE_64x160_W5 = 13 /* five waves of 64x32, 4-deep ring: 2048 x 1280 is exactly 256 tiles (one per CU) */,
       TMIX_TILE_256x320_S2 = 14 /* eight waves of 64x160: 2048 x 10240 (GEGLU up-projection) is exactly 256 tiles */,
       TMIX_TILE_32x160_W5 = 15 /* five waves of 32x32: 1024 x 1280 (one batch row per chain) is 256 tiles */,
       TMIX_TILE_256x256_PH = 16 /* eight waves, K slices of 32 through a four-slot ring, the second wave of each SIMD one barrier behind the first */,
       TMIX_TILE_256x128_PH = 17,
       TMIX_TILE_128x160_S4_K2 = 18 /* tiling 12 with in-workgroup split-K: two groups of four waves share the tile (eight waves stage) */,
       TMIX_TILE_128x160_S3_LW = 19 /* 128x160, 3-deep ring, plus ONE loader wave: the four math waves issue no VMEM instruction in the K loop */,
       TMIX_TILE_128x160_S4_LW2 = 20 /* tiling 12 plus TWO loader waves (each issues every other LDS-DMA instruction of a K-tile) */,
       TMIX_TILE_128x160_S4_LW4 = 21 /* tiling 12 plus FOUR loader waves: one per SIMD, nine LDS-DMA instructions of a K-tile each */,
       TMIX_TILE_256x320_PH = 22 /* 256x320 with the phase-offset mainloop (eight waves of 64x160): bf16 GEMM, no transposed region */,
       TMIX_TILE_128x160_W22 = 23 /* 128x160 over 2 x 2 math waves of 64x80 (16x16x32 MFMA) + four loader waves: plain staged bf16 epilogue, other launches run as tiling 21 */,
       /* ids 24 and 25 are reserved; run as 14 / 23 */
       TMIX_TILE_CONV_HALO = 26 /* tmix_conv3x3_nhwc only: stride-1 3x3 convolution with the input halo patch in LDS; launches it cannot run go to tiling 20 (a GEMM: 21) -- tmix_conv_resolve_tile tells */,
       TMIX_TILE_COUNT = 26 };
typedef struct {
    const void* A;  int64_t lda, strideA;        /* bf16 [batch][M][lda]                          */
    const void* W;  int64_t ldw, strideW;        /* bf16 [batch|1][N][ldw]                        */
    void*       C;  int64_t ldc, strideC;        /* bf16 [batch][M][ldc] (N/2 cols when GEGLU)    */
    const float* bias;  int64_t strideBias;      /* fp32 [N] or NULL                              */
    const void* residual; int64_t ldr, strideR;  /* bf16 [batch][M][ldr] or NULL (added in fp32)  */
    const float* rowgroup_bias;                  /* fp32 [M/rows_per_group][N] or NULL            */
    int32_t rows_per_group;
    void*   Ct; int64_t ldct, strideCt;          /* transposed output for columns >= n_trans_begin */
    int32_t n_trans_begin;                       /*   Ct[b][n - n_trans_begin][m]; <0 = none       */
    int32_t M, N, K, batch;
    int32_t epilogue;
    int32_t tile_cfg;                            /* TMIX_TILE_AUTO or a specific tiling (autotuned by the host) */
    /* --- LayerNorm fused across the GEMM pair that surrounds it (diffusers BasicTransformerBlock.norm1/2/3):
     * producer: row_stats_out[b][t][m] = {sum, sum of squares} over the columns of column-tile t of the STORED
     *   (bf16-rounded) output row m: plain stores in a fixed reduction order (no atomics, nothing to zero, replays are
     *   bit-reproducible).  t < tmix_gemm_stats_parts(N, tile_cfg); tile_cfg must be explicit (not TMIX_TILE_AUTO).
     * consumer: A holds the raw (un-normalised) rows and ln_stats the producer's ln_parts partials per row; with
     *   W' = W*gamma (column-scaled), ln_colsum[n] = sum_k W'[n][k] and bias[n] = sum_k W[n][k]*beta[k] (+ the layer's
     *   bias) the kernel forms  rstd[m] * (acc[m][n] - mean[m] * ln_colsum[n]) + bias[n]  ==  Linear(LayerNorm(x)).
     * Statistics live as fp32 {sum, sumsq} pairs [parts][ld rows]; batch b of a batched GEMM starts stride floats in
     * (so a [B*S]-row buffer serves both the flat M = B*S GEMMs and the batched M = S ones: ld = B*S, stride = 2*S). */
    float* row_stats_out; int64_t strideStatsOut, ldStatsOut;     /* NULL or fp32 [parts][ldStatsOut][2] */
    const float* ln_stats; int64_t strideLnStats, ldLnStats;      /* NULL or fp32 [ln_parts][ldLnStats][2] */
    const float* ln_colsum; int64_t strideLnColsum;   /* fp32 [batch?][N] (stride 0: shared) */
    float ln_inv_c, ln_eps;                           /* 1/C and eps of the LayerNorm */
    int32_t ln_parts, reserved0;                      /* partials per row in ln_stats, 1..16 */
    /* --- GroupNorm statistics from the launch that WRITES the normalised tensor (diffusers ResnetBlock2D.norm1/norm2,
     * Transformer2DModel.norm, conv_norm_out read what a conv / proj_out / conv_shortcut launch has just stored): NULL, or fp32
     * [M / TMIX_COLSTATS_ROWS][2][N]: plane 0 the sum, plane 1 the sum of squares of every column over rows [32 r, 32 r + 32) of
     * the STORED (bf16-rounded) output.  Plain stores in a fixed order (nothing to zero, replays are bit-reproducible), the same
     * layout under every tiling; tmix_groupnorm_nhwc_pre consumes it.  Plain bf16 epilogue only (no transposed region, no
     * activation, no row_stats_out / e4m3 copy), batch == 1, M %% 32 == 0, N %% 8 == 0, 16-byte aligned C / residual rows. */
    float* col_stats_out;
    /* --- periodic weight sets (several independent seeds share every UNet launch: batch rows [seed][concept], and row b of the batch wants the
     * weights of concept b %% w_period): 0 = W / bias / ln_colsum (and the fp8 W scales) are indexed by the batch slice as their strides say;
     * P > 0 (batch %% P == 0) = slice b reads set b %% P of P stored sets -- no gathered per-row copies of the merged LoRA weights
     * (utils_lora.py:65-79,113-119 applied per row), and the slices that share a set are issued back to back. */
    int32_t w_period, reserved1;
} tmix_gemm_desc;
int tmix_gemm_bf16(const tmix_gemm_desc* d, void* stream);
/* The tiling (1..TMIX_TILE_COUNT) of the kernel that tmix_gemm_bf16(d) -- fp8_operands != 0: tmix_gemm_fp8(d) with valid scale arrays -- would run: d->tile_cfg
 * after AUTO, the retired / reserved ids and every substitution for what this launch needs (csrc/gemm_tilings.h).  The same validation and the same resolver
 * as the launch itself; negative TMIX_E* where the launch would refuse.  Never touches the device.  tmix_conv_resolve_tile: the same for tmix_conv3x3_nhwc[_fp8]. */
int tmix_gemm_resolve_tile(const tmix_gemm_desc* d, int fp8_operands);
/* the tiling that runs tile_cfg for a bf16 GEMM that leaves an e4m3 copy (TMIX_F8_COPY_OUT), by the id alone; TMIX_EINVAL outside 1..TMIX_TILE_COUNT */
int tmix_gemm_f8copy_tile(int tile_cfg);
/* Hint for the NEXT tmix_gemm_bf16 / tmix_conv3x3_nhwc launch issued by this host thread (consumed and cleared by it): while its
 * workgroups wait for their own first operands they touch [next_weights, next_weights + bytes) -- one 4-byte load per 128-byte line, the
 * range split evenly over the grid -- so that the weights of the launch that FOLLOWS it are in the memory-side (Infinity) cache when that
 * launch starts (a dependent chain of launches otherwise meets every weight cold from HBM: fusion_sampling.py:340 calls the UNet's
 * ~490 Linear / Conv2d layers back to back).  Purely a performance hint: no effect on results; bytes <= 0 or NULL clears it.
 * The touches share the hinting launch's memory queues: from a launch of tens of microseconds name a few MB of a large tensor rather than all of it.
 * `stream` is ignored (present so that the call has the shape of every other launch entry). */
int tmix_gemm_prefetch_next(const void* next_weights, int64_t bytes, void* stream);
/* The same GEMM on OCP fp8 (e4m3) operands -- the reference's precision bar is fp16 autocast (fusion_sampling.py:492); this is
 * the optional lower-precision path for the FF / QKV projections (`--dtype fp8`), never the default.  A and W hold e4m3 BYTES
 * (lda / ldw / strides in elements = bytes, multiples of 16; K %% 64 == 0) and every A row and W row carries one power-of-two
 * scale, an E8M0 exponent byte: A[m][k] = a8[m][k] * 2^(scale_a[m] - 127).  scale_a is [batch][M], scale_w [N] (or [batch][N]
 * when strideW != 0).  v_mfma_scale_f32_32x32x64_f8f6f4 applies both scales in hardware (per-row instead of the MX format's
 * per-32 blocks, so a lane keeps its scales for the whole K loop); accumulation and every epilogue of tmix_gemm_bf16 (bias,
 * fused LayerNorm on A, GEGLU, residual, transposed V, row statistics) are unchanged.  tile_cfg: TMIX_TILE_AUTO,
 * TMIX_TILE_256x256_PH or TMIX_TILE_256x128_PH.
 * Two flags in tmix_gemm_desc.reserved0 chain fp8 GEMMs without a quantiser pass in between (FF up-projection -> down-projection):
 *   TMIX_F8_GEGLU_OUT       with TMIX_EPI_GEGLU: C receives e4m3 BYTES [M][N/2] (ldc in bytes) and Ct (ldct >= batch*M) the E8M0 scales of
 *                           every 32 output columns, k-block major: Ct[(col / 32) * ldct + b*M + m] -- the MX block form;
 *   TMIX_F8_A_BLOCK_SCALES  scale_a is such a block-scale array [K/32][batch*M] instead of one byte per row (the instruction applies
 *                           a lane's scale to exactly its 32 K values); scale_w stays per row.  The K/32 blocks of a tile stay in
 *                           LDS for the whole K loop: K <= 7168 (256x256 tiles up to K = 2816, 256x128 beyond), M %% 4 == 0. */
/*   TMIX_F8_COPY_OUT        (tmix_gemm_bf16 and tmix_gemm_fp8, plain epilogue, no transposed region): besides the bf16 rows in C the launch
 *                           leaves their e4m3 copy with MX block scales -- what a quantiser pass over C would produce -- for the next GEMM
 *                           that reads C as its A operand: Ct = bytes [batch*M][ldct] (ldct >= N), and the scale array [N/32][batch*M]
 *                           starts strideCt BYTES behind Ct.  M %% 32 == 0, N %% 32 == 0. */
enum { TMIX_F8_A_BLOCK_SCALES = 1, TMIX_F8_GEGLU_OUT = 2, TMIX_F8_COPY_OUT = 4 };
#define TMIX_COLSTATS_ROWS 32   /* rows per partial of col_stats_out */
int tmix_gemm_fp8(const tmix_gemm_desc* d, const uint8_t* scale_a, const uint8_t* scale_w, void* stream);
/* attn2 of a BasicTransformerBlock in ONE launch: q = to_q(LayerNorm(h)) and softmax(q K^T * scale) V against the cached prompt keys -- the patched
 * cross-attention forward of utils_custom.py:56-106 / utils_lora.py:65-69,101-111 (per-row concept weights = per-slice weight sets of d) without the q
 * round trip through memory and without the second launch.  d describes the projection exactly as for tmix_gemm_bf16 (A = hidden state rows, W = to_q
 * weight(s), bias, folded LayerNorm via ln_stats / ln_colsum, batch / strideW / w_period; no residual, activation, transposed region or statistics;
 * d->C is not written and may be NULL); N = heads * 64 must be a multiple of 320 (five heads per tile), K %% 64 == 0.  K: cached keys
 * [images][Skv][ldk] (head h at columns h*64..), Vt: cached V^T [images][N][ldvt] with ldvt == 80 (zero behind Skv), Skv <= 80; image of row r of
 * slice b = b * (M / rows_per_image) + r / rows_per_image (rows_per_image %% 64 == 0: the latent's token count).  O [batch * M][ldo] bf16 receives the
 * attention output (head h at columns h*64..), the A operand of attn2.to_out. */
int tmix_gemm_q_cross_attn(const tmix_gemm_desc* d, const void* K, int64_t ldk, int64_t strideK, const void* Vt, int64_t ldvt, int64_t strideVt,
                           void* O, int64_t ldo, int rows_per_image, int Skv, float scale, void* stream);
/* Row quantiser for tmix_gemm_fp8: X bf16 [rows][ld] -> Q e4m3 [rows][ldq] and scale_e8m0[r] = the smallest exponent that brings
 * max|X[r]| under 448 (K %% 8 == 0, K <= 8192).  Used on activations before each fp8 GEMM and once on the weights. */
int tmix_quantize_fp8_rows(const void* X, int64_t ld, void* Q, int64_t ldq, uint8_t* scale_e8m0, int64_t rows, int K, void* stream);
/* workgroup tile of a TMIX_TILE_* id (bm x bn), and the number of row-statistics partials a GEMM of width N writes with it */
int tmix_gemm_tile_shape(int tile_cfg, int* bm, int* bn);
int tmix_gemm_stats_parts(int N, int tile_cfg);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution, NHWC bf16, implicit GEMM on MFMA (pad 1).
 * Replaces diffusers ResnetBlock2D.conv1/conv2, Downsample2D.conv (mode 1) and Upsample2D
 * (nearest x2 + conv, mode 2) inside the same UNet call sites.  Cin % 64 == 0.
 */
/* TMIX_CONV_T3: temporal convolution, kernel (3,1,1) with padding (1,0,0) over the FIRST spatial axis -- X is
 * [clips][frames][h*w][Cin] and Wt [Cout][3][Cin] (diffusers TemporalConvLayer's Conv3d of the I2VGen-XL UNet, config #5). */
/* TMIX_CONV_S2A: stride 2 with the zero padding on the right / bottom edge only (diffusers Downsample2D(padding=0) of the VAE ENCODER:
 * F.pad(x, (0,1,0,1)) then a stride-2 conv), out[y][x] = sum w[ky][kx] in[2y+ky][2x+kx]. */
/* TMIX_CONV_UP2F: TMIX_CONV_UP2 with the nearest x2 upsampling FOLDED into the weights.  The three rows a 3x3 window touches on the upsampled image come
 * from two source rows (output row 2 sy + fy reads source rows sy-1, sy, sy for fy = 0 and sy, sy, sy+1 for fy = 1; columns alike), so each of the four
 * output phases (fy, fx) is a 2x2 convolution of the SOURCE image whose weights are sums of 1, 2 or 4 of the 3x3 taps: K = 4 Cin instead of 9 Cin, and the
 * zero padding is the same (merged taps lie inside the image, lone taps outside exactly where the upsampled coordinate does).  Wt is
 * [4][Cout][2][2][Cin], phase = 2 fy + fx major, tap (ky, kx) of phase (fy, fx) reading source pixel (sy - 1 + fy + ky, sx - 1 + fx + kx): row taps
 * {ky=0}, {ky=1,2} for fy = 0 and {ky=0,1}, {ky=2} for fy = 1 of the 3x3 kernel.  Y is the same dense [B][2H][2W][Cout] tensor; bias, batch_bias and
 * col_stats_out as for the other modes (col_stats_out blocks are 32 rows of the launch's phase-major row order ((b*4 + phase)*H + sy)*W + sx: an image's
 * blocks are still its own and contiguous).  H * W must be a multiple of the row count of the tile that runs the launch (TMIX_ESHAPE otherwise:
 * tmix_conv_resolve_tile says so without launching), W >= 2; no residual, no shortcut taps, bf16 operands only (TMIX_EINVAL). */
enum { TMIX_CONV_S1 = 0, TMIX_CONV_S2 = 1, TMIX_CONV_UP2 = 2, TMIX_CONV_T3 = 3, TMIX_CONV_S2A = 4, TMIX_CONV_UP2F = 5 };
typedef struct {
    const void* X;   /* bf16 [B][H][W][Cin]                                   */
    const void* Wt;  /* bf16 [Cout][3][3][Cin]  ([Cout][3][Cin] for T3, [4][Cout][2][2][Cin] for UP2F) */
    void*       Y;   /* bf16 [B][Ho][Wo][Cout]  Ho = H (S1), H/2 (S2), 2H (UP2, UP2F) */
    const float* bias;           /* fp32 [Cout] or NULL                       */
    const float* batch_bias;     /* fp32 [B][Cout] (time embedding) or NULL   */
    const void* residual;        /* bf16 like Y or NULL                       */
    int32_t B, H, W, Cin, Cout, mode;
    int32_t tile_cfg;            /* TMIX_TILE_*                                */
    int32_t batch_bias_images;   /* consecutive images that share one batch_bias row (0/1: one row per image; the video
                                    UNet folds frames into B and has one time embedding per clip: = frames) */
    float* col_stats_out;        /* NULL or fp32 [B*Ho*Wo / 32][2][Cout]: as in tmix_gemm_desc (B*Ho*Wo %% 32 == 0, Cout %% 8 == 0) */
    /* --- the 1x1 conv_shortcut of a ResnetBlock2D in the same launch (diffusers ResnetBlock2D.forward: conv2(h) + conv_shortcut(x); in the
     * up-blocks x = cat[hidden, skip]): S1 / S2 = NULL or bf16 NHWC [B][H][W][S1_channels] / [..][S2_channels] (TMIX_CONV_S1 geometry only,
     * channels %% 64 == 0, S2 only with S1), and Wt then holds rows [Cout][9*Cin + S1_channels + S2_channels] = [conv2 taps | shortcut
     * weights over S1's channels | over S2's]; bias = conv2.bias + conv_shortcut.bias.  The K loop walks the two tensors' channels at the
     * output pixel behind the nine taps: one accumulator, no shortcut GEMM, no residual round trip, and the concatenation is never written. */
    const void* S1; const void* S2;
    int32_t S1_channels, S2_channels;
} tmix_conv_desc;
int tmix_conv3x3_nhwc(const tmix_conv_desc* d, void* stream);
/* the same convolution (diffusers ResnetBlock2D.conv1 / conv2 behind fusion_sampling.py:340) on OCP e4m3 operands: X = e4m3 bytes [B,H,W,Cin] with one E8M0
 * scale per (pixel, 32 channels) in the ROW-major form scale_x [B*H*W][Cin/32] -- what tmix_groupnorm_nhwc_pre_f8 writes -- Wt = e4m3 bytes [Cout][taps*Cin] with one
 * E8M0 scale per output channel (tmix_quantize_fp8_rows over the weight rows).  Cin %% 128 == 0 (a K-tile is 128 channels of one tap), no shortcut taps;
 * Y, bias, batch_bias, residual, col_stats_out as in tmix_conv3x3_nhwc.  tile_cfg: 12 or 20 (128x160 without / with two loader waves). */
int tmix_conv3x3_nhwc_fp8(const tmix_conv_desc* d, const uint8_t* scale_x, const uint8_t* scale_w, void* stream);
int tmix_conv_resolve_tile(const tmix_conv_desc* d, int fp8_operands);       /* see tmix_gemm_resolve_tile */

/* conv_in: fp32 NCHW latent [B,4,H,W] -> bf16 NHWC [B,H,W,Cout] (Cout % 32 == 0); weights fp32 OHWI. */
int tmix_conv_in(const float* x_nchw, const float* w_ohwi, const float* bias, void* y_nhwc,
                 int B, int Cin, int H, int W, int Cout, void* stream);
/* same with a per-pixel 4x4 linear map applied to the latent first (host pointers: pre_w[16] row-major, pre_b[4]):
 * the VAE's 1/scaling_factor and post_quant_conv (AutoencoderKL.decode), exact at the zero-padded border. */
int tmix_conv_in_pre(const float* x_nchw, const float* w_ohwi, const float* bias, void* y_nhwc,
                     int B, int Cin, int H, int W, int Cout, const float* pre_w, const float* pre_b, void* stream);
/* conv_out: bf16 NHWC [B,H,W,Cin] -> fp32 NCHW [B,Cout<=8,H,W]; weights bf16 OHWI. */
int tmix_conv_out(const void* x_nhwc, const void* w_ohwi, const float* bias, float* y_nchw,
                  int B, int Cin, int H, int W, int Cout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flash attention forward, head dim 64, bf16 in/out, fp32 softmax (never materialises S x S).
 * Replaces the explicit einsum/softmax/einsum of utils_custom.py:93-103 and utils_lora.py:101-111
 * and xformers' memory-efficient attention for attn1 (fusion_sampling.py:120,133,210).
 *   Q  [B][Sq][ldq]   head h at columns h*64..h*64+63
 *   K  [B][Skv][ldk]  same column convention
 *   Vt [B][H*64][ldvt] V TRANSPOSED (row = h*64+d, column = key); ldvt >= Skv rounded up to 8 and
 *                      the padding columns must hold finite values
 *   O  [B][Sq][ldo]
 * Rows of K behind Skv and rows of Q behind Sq of a slice may hold any bit pattern, NaN included: key and query indices past the last real row are clamped to
 * it (or not loaded at all) and what they give is masked by selection (the same holds for tmix_gemm_q_cross_attn and tmix_xattn_token_maps).
 *
 * scale (all four tmix_attn_fwd* entries): the kernels fold the softmax scale into Q while they form its bf16 MFMA fragments, so no multiply sits
 * on the score path.  Two forms:
 *   scale > 0   P = softmax(scale * Q K^T).  Q is multiplied by scale * log2(e) and rounded to bf16 a SECOND time (it arrived rounded once): a
 *               fresh 2^-9 relative error on every element of Q, i.e. a logit error of about 2^-9 * sqrt(sum_d (q_d k_d)^2) * scale, which
 *               grows with the logit and is exponentiated by the softmax (unit-Gaussian inputs: invisible; logit std 4: ~1 % of max|O|).
 *   scale < 0   Q is ALREADY in log2 units -- log2(e) was folded into its producer (weights.q_log2_units: the to_q rows, their bias and
 *               LayerNorm column sums, before the single cast to bf16) -- and P = softmax2(|scale| * Q K^T), softmax2 = the softmax to base 2.
 *               |scale| must be a power of two (TMIX_EINVAL otherwise): that product is exact in bf16, so Q stays rounded once.
 *               The plans launch attn1 of the image UNet and the spatial attn1 of the video UNet with scale = -0.125.
 */
int tmix_attn_fwd(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                  const void* Vt, int64_t ldvt, int64_t strideVt, void* O, int64_t ldo, int64_t strideO,
                  int B, int H, int Sq, int Skv, float scale, void* stream);
/* the same attention with the output as the block-scaled A operand of the out-projection behind it (utils_lora.py:116-119 / utils_custom.py:104-106 on
 * e4m3 operands, tmix_gemm_fp8 + TMIX_F8_A_BLOCK_SCALES): O8 [B*Sq][ldo8] OCP e4m3 bytes (head h at columns h*64..), scales [H*2][ldScale >= B*Sq] one
 * E8M0 byte per (row, 32 columns), k-block major -- bit for bit what an MX quantiser makes of the bf16 tensor tmix_attn_fwd writes; no bf16 output. */
int tmix_attn_fwd_f8(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                     const void* Vt, int64_t ldvt, int64_t strideVt, void* O8, int64_t ldo8, void* scales, int64_t ldScale,
                     int B, int H, int Sq, int Skv, float scale, void* stream);
/* The same two launches with a caller-owned workspace for the KEY-SPLIT TAIL.  B * H * ceil(Sq / 128) work items run on 512 workgroup slots; where a last,
 * partly filled round remains (the reference's attn1 at SDXL 1024^2, utils_lora.py:101-111 at B = 4: 640 items at S = 1024, 1280 at S = 4096) its items
 * are cut into 2 or 4 key ranges, one workgroup each, whose partial (o, maximum, row sum) meet in the workspace; the item's last arriver adds them in range
 * order (a fixed order: results do not depend on arrival) and stores.  tmix_attn_split_ws_bytes: bytes that enable the split for a shape (0: the shape does
 * not split; then, and with ws = NULL, the calls are exactly the two above).  The workspace is zero-filled ONCE by the caller (its first 4 KiB are ticket
 * counters every launch leaves at zero) and belongs to one stream at a time.  Results differ from the unsplit launch by fp32 rounding of the merge only. */
int64_t tmix_attn_split_ws_bytes(int B, int H, int Sq, int Skv);
int tmix_attn_fwd_ws(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                     const void* Vt, int64_t ldvt, int64_t strideVt, void* O, int64_t ldo, int64_t strideO,
                     int B, int H, int Sq, int Skv, float scale, void* ws, int64_t ws_bytes, void* stream);
int tmix_attn_fwd_f8_ws(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                        const void* Vt, int64_t ldvt, int64_t strideVt, void* O8, int64_t ldo8, void* scales, int64_t ldScale,
                        int B, int H, int Sq, int Skv, float scale, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Normalisation / small ops (diffusers GroupNorm(32)+SiLU, LayerNorm, Timesteps, time MLPs).
 */
/* ws: fp32 workspace of >= tmix_groupnorm_ws_floats(B, C1+C2, groups) floats. Two inputs are
 * normalised as one tensor concatenated along C (X2 may be NULL, C2 = 0). */
int64_t tmix_groupnorm_ws_floats(int B, int C, int groups);
int tmix_groupnorm_ws_chunks(int64_t HW);   /* statistics workgroups per image (a function of the image size only) */
int tmix_groupnorm_nhwc(const void* X1, int C1, const void* X2, int C2, void* Y, const float* gamma,
                        const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                        void* stream);
/* kernels one tmix_groupnorm_nhwc call issues for an image of HW pixels and C channels: 3 (statistics, combine, apply) or 1 -- images whose slice of a few groups
 * (HW x 8..256 channels <= 64 K elements: the 336- / 84-pixel frames of video_gen/pipeline_i2vgen_xl.py:680-722's third and fourth levels) is small are normalised by one
 * workgroup per (image, group set) in a single launch.  A function of the image's shape only, never of the batch. */
int tmix_groupnorm_nhwc_launches(int64_t HW, int C, int groups);
/* The same normalisation with the statistics pass replaced by the column partials the PRODUCERS of the tensor left behind
 * (tmix_gemm_desc.col_stats_out / tmix_conv_desc.col_stats_out): cs1 = fp32 [B*HW / 32][2][cs1_channels] covers channels
 * [0, cs1_channels), cs2 (NULL with cs2_channels = 0) the cs2_channels behind them; cs1_channels + cs2_channels = C1 + C2.  The split of
 * the statistics need not be the split of X: the up-blocks normalise ONE concatenated tensor whose halves were written by two launches.
 * HW %% 32 == 0.  Two launches (combine partials -> scale / shift per channel, apply) instead of three, and X is read once instead of
 * twice.  Same ws as tmix_groupnorm_nhwc. */
int tmix_groupnorm_nhwc_pre(const void* X1, int C1, const void* X2, int C2, void* Y, const float* gamma,
                            const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                            const float* cs1, int cs1_channels, const float* cs2, int cs2_channels, void* stream);
/* tmix_groupnorm_nhwc_pre with the normalised (+ SiLU) tensor written as e4m3 bytes Y8 [B*HW][C] + scales [B*HW][C/32] (row-major MX blocks; C %% 32 == 0):
 * the input of tmix_conv3x3_nhwc_fp8; bit for bit what an MX quantiser makes of the bf16 tensor tmix_groupnorm_nhwc_pre writes. */
int tmix_groupnorm_nhwc_pre_f8(const void* X1, int C1, const void* X2, int C2, void* Y8, void* scales, const float* gamma,
                               const float* beta, float* ws, int B, int64_t HW, int groups, float eps, int silu,
                               const float* cs1, int cs1_channels, const float* cs2, int cs2_channels, void* stream);
int tmix_layernorm(const void* X, void* Y, const float* gamma, const float* beta, int64_t rows, int C,
                   float eps, void* stream);
/* hipMemsetAsync(ptr, 0, nbytes) on the stream (graph-capturable): zeroes the LayerNorm statistics accumulators */
int tmix_zero(void* ptr, int64_t nbytes, void* stream);
int tmix_concat_channels(const void* X1, int C1, const void* X2, int C2, void* Y, int64_t rows, void* stream);
/* sinusoidal embedding (flip_sin_to_cos=True, shift 0): out[i] = [cos(v_i f_j) | sin(v_i f_j)], j<dim/2 */
int tmix_timestep_embedding(const float* values, float* out, int count, int dim, void* stream);
/* row softmax: P[r][c] = softmax_c(scale * S[r][c]), S fp32 [rows][ld_s] -> P bf16 [rows][ld_p] (VAE mid-block attention,
 * single head of dim 512: scores come from tmix_gemm_bf16 with TMIX_EPI_F32OUT). */
int tmix_softmax_rows(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, float scale, void* stream);
/* causal variant for the CLIP text encoders (transformers CLIPAttention with the causal mask, fusion_sampling.py:43-68):
 * S is a stack of [seq][cols] score blocks; row r sees columns <= r % seq, every other column (padding included) gets 0. */
int tmix_softmax_rows_causal(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, float scale,
                             int seq, void* stream);
/* padded variant (CLIP vision tower of the video pipeline: 257 tokens in rows padded to a multiple of the GEMM K-tile):
 * columns >= valid get probability 0. */
int tmix_softmax_rows_masked(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int cols, int valid, float scale,
                             void* stream);
/* temporal self-attention over the frame axis (diffusers TransformerTemporalModel of the I2VGen-XL UNet, BASELINE config #5;
 * the reference drives it through video_gen/pipeline_i2vgen_xl.py:688-697): QKV bf16 [(clips*frames)][hw][ld] with columns
 * [0,C) = Q, [C,2C) = K, [2C,3C) = V, C = heads*64; every (clip, pixel, head) attends over its <= 16 frames;
 * O bf16 [(clips*frames)][hw][ldo], columns [0,C). */
int tmix_temporal_attn(const void* QKV, int64_t ld, void* O, int64_t ldo, int clips, int frames, int64_t hw, int heads,
                       float scale, void* stream);
/* LoRA in its low-rank form (utils_lora.py:65-79,113-119: batch row i + 1 gets  proj(x) + up_i(down_i(x)), model_lora.py:41-48, rank 4) without
 * merged per-concept weight copies: the attention projection runs once on shared weights [W | U | 0] over K + 64 input columns, and this
 * launch fills the 64 PAD columns behind every row of A with that row's down-projections: rows [b * rows_per_set, +rows_per_set) belong to
 * concept set sets[b] (0 = base, no delta); the P = 4 x (projections fused in the GEMM: 1, or 3 for q|k|v) values  A[m][0..K) . D[set * P + q][0..K)
 * go to columns K + set * P + q, every other pad column gets 0.  D is bf16 [nsets * P][K], nsets * P <= 64, P in {4, 12}.
 * Folded LayerNorm (dcolsum / dbias non-NULL; the GEMM then reads raw rows with ln_stats): the pad holds
 * (x - mean) D'^T + dbias / rstd  with D' = D * gamma as passed in D, dcolsum[i] = sum_k D'[i][k], dbias[i] = sum_k D[i][k] beta[k], and mean / rstd
 * of the row itself -- so that the GEMM's  rstd * (acc - mean * ln_colsum) + bias  (ln_colsum over the first K columns) adds exactly up(down(LN(x))). */
int tmix_lora_down(void* A, int64_t lda, int K, int64_t rows, const void* D, int P, int nsets, const float* dcolsum, const float* dbias,
                   float eps, const int* sets, int64_t rows_per_set, void* stream);
/* y = clamp(x*scale + shift, lo, hi) on fp32 (image post-processing (img/2+0.5).clamp(0,1), fusion_sampling.py:302) */
int tmix_affine_clamp(const float* x, float* y, int64_t n, float scale, float shift, float lo, float hi, void* stream);
/* out[M,N] = act_out( act_in(in[M,K]) * W[N,K]^T + bias ), fp32 activations, bf16 weights, M <= 256 (16 rows per launch).
 * act: 0 none, 1 SiLU.  add (nullable): fp32 [M,N] added before act_out. */
int tmix_linear_small(const float* in, const void* W, const float* bias, const float* add, float* out,
                      int M, int N, int K, int act_in, int act_out, void* stream);
/* The same for several weight matrices stacked along N that share the input (every ResnetBlock2D's time_emb_proj of one UNet
 * forward: 19 launches -> 1): sec_starts is a DEVICE array of nsec + 1 ascending column offsets (sec_starts[0] = 0,
 * sec_starts[nsec] = N); section s leaves as its own dense fp32 [M][width_s] matrix at out + sec_starts[s] * M. */
int tmix_linear_small_sections(const float* in, const void* W, const float* bias, float* out, int M, int N, int K,
                               int act_in, const int* sec_starts, int nsec, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-independent half of I2VGenXLUNet.forward (BASELINE config #5): the fps embedding, the context tokens and the image-latent
 * features that video_gen/pipeline_i2vgen_xl.py:604-639 prepares and :688-697 passes to the UNet on every step are constant over the
 * loop; tweediemix_amd/i2vgen.py conditioning() evaluates them once per video on these fp32 kernels (layers of 4 .. 64 channels).
 * 3x3 convolution, padding 1, stride 1 or 2: x fp32 NCHW [B,Cin,H,W], w fp32 OIHW [Cout,Cin,3,3] (the checkpoint's layout),
 * y fp32 NCHW [B,Cout,(H-1)/stride+1,(W-1)/stride+1]; silu != 0 applies SiLU to the result. */
int tmix_conv3x3_f32(const float* x_nchw, const float* w_oihw, const float* bias, float* y_nchw, int B, int Cin, int H, int W, int Cout,
                     int stride, int silu, void* stream);
/* torch.nn.AdaptiveAvgPool2d((OH, OW)) over `planes` fp32 [H][W] planes: window i = [floor(i H / OH), ceil((i + 1) H / OH)). */
int tmix_adaptive_avgpool_f32(const float* x, float* y, int64_t planes, int H, int W, int OH, int OW, void* stream);
/* out[M,N] = act_out(act_in(in[M,K]) W[N,K]^T + bias), everything fp32 (act: 0 none, 1 SiLU), M <= 256. */
int tmix_linear_f32(const float* in, const float* W, const float* bias, float* out, int M, int N, int K, int act_in, int act_out, void* stream);
/* image_latents_temporal_encoder (diffusers I2VGenXLTransformerTemporalEncoder, width `channels` = 4): per (clip, pixel) over its <= 16 frames
 *   x1 = x + to_out(attention(LayerNorm(x)))  (two heads of 4, scale 1/2),   y = x1 + W2 gelu(W1 x1 + b1) + b2
 * x fp32 [clips*frames, 4, H, W] (the output of image_latents_proj_in), y fp32 [clips, 4, frames, H, W] (what the UNet concatenates to the
 * sample); weights fp32 in the checkpoint's [out, in] layout: wq / wk / wv [8,4], wo [4,8], w1 [16,4], w2 [4,16]. */
int tmix_i2v_temporal_encoder(const float* x, float* y, int clips, int frames, int channels, int64_t hw, const float* ln_gamma, const float* ln_beta,
                              const float* wq, const float* wk, const float* wv, const float* wo, const float* bo,
                              const float* w1, const float* b1, const float* w2, const float* b2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-attention token maps (the in-process mask source: masks.attention_masks; no reference counterpart -- it replaces the
 * decode + GroundingDINO / SAM side-car of fusion_sampling.py:431-469 with the localisation the attn2 modules already compute).
 * For the selected batch rows b_i = row0 + i * row_step, i < n_rows:
 *   maps[i][j][s] (+)= sum_h softmax_k( scale * Q[b_i][s][h*64..+64) . K[b_i][k][h*64..+64) )[tokens[j]]
 *   Q bf16 [B][Sq][ldq] (row stride strideQ): the attn2 to_q output;  K bf16 [B][Lk][ldk] (strideK): the cached keys (unet.KVCache)
 *   maps fp32 [n_rows][n_tok][Sq]; accumulate != 0 adds to it, 0 overwrites.  Head size 64, H heads (ldq, ldk >= H * 64).
 * n_tok in 1..8 positions (tokens: a HOST array, read at the call and passed by value in the launch, so a captured graph holds
 * it; every position < Lk), Lk <= 80.  Softmax in fp32 over the Lk real keys.  Deterministic: one thread owns every output
 * element, heads are added in a fixed order, no atomics, and a row's maps do not depend on the other rows of the batch.
 * Q, K, maps 8-byte aligned; ldq, strideQ, ldk, strideK multiples of 4. */
int tmix_xattn_token_maps(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, float* maps,
                          int B, int H, int Sq, int Lk, int row0, int row_step, int n_rows, const int32_t* tokens, int n_tok,
                          int accumulate, float scale, void* stream);
/* The same for chunked prompts (text.encode_prompts(long=True): 154 or 231 keys) and longer position lists: same arguments, same
 * meaning and every property above, with Lk <= 240 and n_tok in 1..32 (errors: n_tok outside 1..32 or a position >= Lk TMIX_EINVAL,
 * Lk > 240 TMIX_ESHAPE).  A call with Lk <= 80 and n_tok <= 8 is forwarded to tmix_xattn_token_maps: the same launch, the same bits. */
int tmix_xattn_token_maps_long(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, float* maps,
                               int B, int H, int Sq, int Lk, int row0, int row_step, int n_rows, const int32_t* tokens, int n_tok,
                               int accumulate, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token maps through self-attention (masks.attention_masks with propagate >= 1; no reference counterpart): the row-stochastic attn1
 * matrix of every head applied to a few fp32 maps and summed over heads.  For the selected batch rows b_i = row0 + i * row_step,
 * i < n_rows, every map j < n_tok and query pixel s < S:
 *   dst[i][j][s] (+)= out_scale * sum_h sum_{s' < S} softmax_{s'}( scale * Q[b_i][s][h*64..+64) . K[b_i][s'][h*64..+64) ) * src[i][j][s']
 *   Q, K bf16 [B][S][ld] (row stride stride*): the attn1 to_q / to_k outputs (two column ranges of one buffer in a plan);
 *   src, dst fp32 [n_rows][n_tok][S], the layout of UNetPlan.token_maps; they must not overlap.  accumulate != 0 adds to dst, 0
 *   overwrites.  Head size 64, H heads (ldq, ldk >= H * 64), n_tok in 1..32.
 * Flash-attention forward whose V is the maps: scores, running max and sum in fp32; the probabilities and src enter the second
 * product rounded to bf16 (nearest even), the sum that normalises is the fp32 one: |error| <= 2^-7 * |out_scale| * H * max|src|.
 * Deterministic: one thread owns every output element, heads and waves are added in a fixed order, no atomics, and a row's result
 * does not depend on the other rows of the batch.  Rows behind S of Q, K, src and dst are neither read nor written.
 * Q, K, src, dst 8-byte aligned; ldq, strideQ, ldk, strideK multiples of 4.  Errors (before any launch): n_tok outside 1..32,
 * scale <= 0, a null pointer, overlapping src / dst TMIX_EINVAL; B, H, S < 1, rows outside the batch, ld < H * 64 TMIX_ESHAPE;
 * alignment TMIX_EALIGN. */
int tmix_sattn_propagate(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                         const float* src, float* dst, int B, int H, int S, int row0, int row_step, int n_rows,
                         int n_tok, int accumulate, float scale, float out_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TMIX_H */
