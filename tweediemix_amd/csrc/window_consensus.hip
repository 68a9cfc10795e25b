// window_consensus.hip -- reconcile overlapping windows of a wide canvas: every canvas pixel that several windows cover becomes, in
// all of them, the weighted mean of their values (tmix_window_consensus; no reference counterpart: the reference samples one image of
// the trained size).  Memory-bound: per covered element one read and one write.
// Compiled with -ffp-contract=off like tweedie_step.hip: separate products and sums, so fp32 results equal the numpy restatement.
#include "common.h"

namespace {

// the windows' offsets on the canvas travel in the kernel arguments: a captured launch carries them by value
struct WinArgs { int n; int oy[TMIX_MAX_WINDOWS]; int ox[TMIX_MAX_WINDOWS]; };

// One thread owns one (group, channel, canvas pixel); a window element belongs to exactly one canvas pixel, so nothing is read by one
// thread and written by another: no atomics, in place, independent of the grid size.  x [groups][n][C][h][w].
__global__ void __launch_bounds__(256)
window_consensus_kernel(float* x, WinArgs wa, int C, int h, int w, int canvas_h, int canvas_w, int64_t total,
                        const float* __restrict__ weight) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t hw = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int cx = (int)(i % canvas_w);
        int64_t r = i / canvas_w;
        const int cy = (int)(r % canvas_h); r /= canvas_h;
        const int64_t c = r % C, g = r / C;
        float acc = 0.0f, ws = 0.0f;
        int covers = 0;
#pragma unroll
        for (int k = 0; k < TMIX_MAX_WINDOWS; ++k) {
            if (k >= wa.n) break;
            const int py = cy - wa.oy[k], px = cx - wa.ox[k];
            if (py < 0 || py >= h || px < 0 || px >= w) continue;
            const int64_t p = (int64_t)py * w + px;
            const float wt = weight ? weight[p] : 1.0f;
            const float v = x[((g * wa.n + k) * C + c) * hw + p];
            acc = acc + wt * v;
            ws = ws + wt;
            ++covers;
        }
        if (covers < 2) continue;                 // a pixel of one window keeps its bits (it is not even rewritten)
        const float res = acc / ws;
#pragma unroll
        for (int k = 0; k < TMIX_MAX_WINDOWS; ++k) {
            if (k >= wa.n) break;
            const int py = cy - wa.oy[k], px = cx - wa.ox[k];
            if (py < 0 || py >= h || px < 0 || px >= w) continue;
            x[((g * wa.n + k) * C + c) * hw + (int64_t)py * w + px] = res;
        }
    }
}

// does every canvas pixel lie in some window?  The windows' edges cut the canvas into at most 17 x 17 cells; a cell is covered as a whole or not at all.
bool canvas_covered(const WinArgs& wa, int h, int w, int canvas_h, int canvas_w) {
    int ys[2 * TMIX_MAX_WINDOWS + 1], xs[2 * TMIX_MAX_WINDOWS + 1];
    int ny = 0, nx = 0;
    ys[ny++] = 0; xs[nx++] = 0;
    for (int k = 0; k < wa.n; ++k) {
        ys[ny++] = wa.oy[k]; ys[ny++] = wa.oy[k] + h;
        xs[nx++] = wa.ox[k]; xs[nx++] = wa.ox[k] + w;
    }
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b) {
            const int y = ys[a], x = xs[b];       // the top-left pixel of a cell
            if (y >= canvas_h || x >= canvas_w) continue;
            bool in = false;
            for (int k = 0; k < wa.n && !in; ++k)
                in = y >= wa.oy[k] && y < wa.oy[k] + h && x >= wa.ox[k] && x < wa.ox[k] + w;
            if (!in) return false;
        }
    return true;
}

}  // namespace

extern "C" int tmix_window_consensus(float* x, int groups, int n_win, const int* win_yx, int C, int h, int w, int canvas_h, int canvas_w,
                                     const float* weight, void* stream) {
    if (!x || !win_yx) TMIX_FAIL(TMIX_EINVAL, "window_consensus: null pointer");
    if (n_win < 1 || n_win > TMIX_MAX_WINDOWS || groups < 1)
        TMIX_FAIL(TMIX_EINVAL, "window_consensus: n_win=%d (1..%d) groups=%d (>= 1)", n_win, TMIX_MAX_WINDOWS, groups);
    if (C < 1 || h < 1 || w < 1 || canvas_h < 1 || canvas_w < 1)
        TMIX_FAIL(TMIX_ESHAPE, "window_consensus: non-positive size C=%d window %d x %d canvas %d x %d", C, h, w, canvas_h, canvas_w);
    WinArgs wa = {};
    wa.n = n_win;
    for (int k = 0; k < n_win; ++k) {
        const int oy = win_yx[2 * k], ox = win_yx[2 * k + 1];
        if (oy < 0 || ox < 0 || oy > canvas_h - h || ox > canvas_w - w)
            TMIX_FAIL(TMIX_ESHAPE, "window_consensus: window %d at (%d, %d) of %d x %d reaches outside the %d x %d canvas", k, oy, ox, h, w, canvas_h, canvas_w);
        wa.oy[k] = oy; wa.ox[k] = ox;
    }
    if (!canvas_covered(wa, h, w, canvas_h, canvas_w))
        TMIX_FAIL(TMIX_ESHAPE, "window_consensus: the %d windows of %d x %d leave pixels of the %d x %d canvas uncovered", n_win, h, w, canvas_h, canvas_w);
    if (n_win == 1) return TMIX_OK;               // one window is the canvas: nothing to reconcile, nothing launched
    const int64_t total = (int64_t)groups * C * canvas_h * canvas_w;
    int64_t blocks = (total + 255) / 256; if (blocks > 2048) blocks = 2048;
    window_consensus_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, wa, C, h, w, canvas_h, canvas_w, total, weight);
    TMIX_LAUNCH_CHECK();
    return TMIX_OK;
}
