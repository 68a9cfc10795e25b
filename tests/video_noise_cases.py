"""Shared by tests/test_video_noise_cpu.py and tests/test_video_noise_gpu.py: inputs of the stochastic video step and the scalar
Gaussian data model of tests/noise_cases.py on the VIDEO loop, as a closed-form covariance recursion (no sampling).

Data x0 ~ N(0, c^2): the marginal of x_t = sa x0 + s1 eps is N(0, v), v(a) = a c^2 + (1 - a); the exact x0(x, t) = k x with k = sa c^2 / v and the
exact eps(x, t) = s1 x / v are linear in x (video_solver_cases.toy_v with m = 0 is the v they give), so every step is a linear map of
(x, x0_prev) plus cz z with z ~ N(0, 1) independent of everything before it:

    DDIM entry       x' = (sa' k + s1_dir s1 / v) x + cz z
    multistep entry  x' = (cx + c0 k) x + c1 x0_prev + cz z,   x0_prev' = k x

The trajectory is the video loop's: x_T ~ N(0, 1); EVERY timestep one solver step (no round trips, no last-step selection); under dpmpp2m the first
step is a first-order solver step and every later one second order; the result is the state behind the last step, at final_alpha_cumprod = a_f,
where the true marginal has variance a_f c^2 + 1 - a_f."""
import numpy as np

from noise_cases import model_k_v
from video_solver_cases import standin_schedule

NF = np.float32
CS, NS = (0.5, 1.0, 2.0), (10, 20, 40)
KEYS = [(182, 0), (0xFFFFFFFE, 7), (5, 0x80000000)]                 # {low word, high word} of three videos
SEEDS = [lo + (hi << 32) for lo, hi in KEYS]
CZ, STEP = float(NF(0.3125)), 7


def target_variance(c, sch):
    a = float(sch.final_alpha_cumprod)
    return a * c * c + 1.0 - a


def predicted_variance(c, n, spacing, solver, eta):
    """variance of the video loop's result for data N(0, c^2), from the coefficients the sampler uploads (video.SolverPhase / solver.ddim_eta_coeffs on
    the stand-in table) -> (variance, schedule)"""
    from tweediemix_amd import solver as SV, video as V
    sch = standin_schedule(n, spacing)
    phase = V.SolverPhase(sch)
    cov = np.array([[1.0, 0.0], [0.0, 0.0]])              # of (x, x0_prev): x_T ~ N(0, 1), no history
    for t in sch.timesteps:
        a = sch.alpha(int(t))
        k, v = model_k_v(a, c)
        if solver == "ddim":
            _sa, s1, san, s1d, cz = SV.ddim_eta_coeffs(a, sch.next_alpha(int(t)), eta)
            M = np.array([[san * k + s1d * s1 / v, 0.0], [k, 0.0]])
        else:
            cx, c0, c1, cz = phase.coeffs(int(t), eta)
            M = np.array([[cx + c0 * k, c1], [k, 0.0]])
        cov = M @ cov @ M.T
        cov[0, 0] += cz * cz
    return float(cov[0, 0]), sch


def variance_error(c, n, spacing, solver, eta=1.0):
    var, sch = predicted_variance(c, n, spacing, solver, eta)
    return abs(var - target_variance(c, sch)) / target_variance(c, sch)


def video_noise(per, keys, step, shape=None):
    """z [len(keys), per] (or [len(keys), *shape]) of the video step: element i of video s draws from (i, keys[s], step, STREAM_VIDEO_STEP)"""
    from tweediemix_amd import noise as NZ
    z = np.stack([NZ.normal(np.arange(per, dtype=np.uint64), lo, hi, step, NZ.STREAM_VIDEO_STEP) for lo, hi in keys])
    return z if shape is None else z.reshape((len(keys),) + tuple(shape))
