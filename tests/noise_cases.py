"""Shared by tests/test_noise_cpu.py and tests/test_noise_gpu.py: the scalar Gaussian data model of tests/test_solver_cpu.py under the stochastic
sampler, as a closed-form covariance recursion (no sampling).

Data x0 ~ N(0, c^2): the marginal of x_t = sa x0 + s1 eps is N(0, v), v(a) = a c^2 + (1 - a); the exact eps(x, t) = s1 x / v is linear in x, so
the Tweedie estimate is x0_hat = k x with k = sa c^2 / v, and every step of either solver is a linear map of (x, x0_prev) plus cz z with z ~ N(0, 1)
independent of everything before it.  The covariance of (x, x0_prev) is therefore propagated exactly:

    DDIM entry       x' = (sa' k + s1_dir s1 / v) x + cz z                      (the move's eps term is the exact eps; both CFG rows hold it)
    multistep entry  x' = (cx + c0 k) x + c1 x0_prev + cz z,   x0_prev' = k x
    last step        the result is x0_hat = k x

The trajectory is the sampler's: x_T ~ N(0, 1), the first timestep a DDIM step under either solver, a solver step second order when the step before
it was a solver step.  The exact sampler would return the Tweedie estimate at t = 1 of a draw of the true marginal: variance k_1^2 v_1."""
import math

import numpy as np


def model_k_v(a, c):
    a = float(a)
    v = a * c * c + (1.0 - a)
    return math.sqrt(a) * c * c / v, v


def exact_eps(x, a, c):
    """the model's exact eps(x, t) in fp64 for x of any shape"""
    a = float(a)
    return math.sqrt(1.0 - a) * np.asarray(x, np.float64) / (a * c * c + (1.0 - a))


def target_variance(c, sch):
    k, v = model_k_v(sch.alpha(1), c)
    return k * k * v


def predicted_variance(c, n, spacing, solver, eta, first_order_at=()):
    """variance of the sampler's result for data N(0, c^2), from the coefficients the sampler uploads (the project's own functions and grids).
    first_order_at: schedule indices whose solver step is first order although the step before was a solver step (the sampler's first fusion step)"""
    from tweediemix_amd import solver as SV
    from tweediemix_amd.schedule import Schedule
    sch = Schedule(n, spacing=spacing)
    ts = sch.timesteps
    cov = np.array([[1.0, 0.0], [0.0, 0.0]])              # of (x, x0_prev): x_T ~ N(0, 1), no history
    prev_solver = None
    for i, t in enumerate(ts):
        a, an = sch.alpha(t), sch.alpha(sch.next_t(t))
        k, v = model_k_v(a, c)
        if t == 1:
            return k * k * cov[0, 0], sch
        if solver == "ddim" or i == 0:
            _sa, s1, san, s1d, cz = SV.ddim_eta_coeffs(a, an, eta)
            M = np.array([[san * k + s1d * s1 / v, 0.0], [k, 0.0]])
        else:
            cx, c0, c1, cz = SV.multistep_eta_coeffs(sch.alpha(ts[i - 1]), a, an, prev_solver == i - 1 and i not in first_order_at, eta)
            M = np.array([[cx + c0 * k, c1], [k, 0.0]])
            prev_solver = i
        cov = M @ cov @ M.T
        cov[0, 0] += cz * cz
    raise AssertionError("the grid does not end at t = 1")
