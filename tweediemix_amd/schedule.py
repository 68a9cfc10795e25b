"""DDIM tables of the image sampler, kept on the HOST as plain floats/ints (no device syncs).

Mirrors fusion_generation/fusion_sampling.py:212-218 (scheduler set-up) and :305-307 (alpha):
SDXL's DDIMScheduler is scaled-linear beta 0.00085..0.012 over 1000 steps, 'leading' spacing,
steps_offset=1, set_alpha_to_one=False; the reference prepends 1.0 to alphas_cumprod, so
alpha(t) = alphas_cumprod[t-1], and alpha(t<0) = final_alpha_cumprod = alphas_cumprod[0].

spacing="logsnr" (no reference counterpart) keeps the table and the first timestep of the 'leading' grid and places the n
timesteps uniformly in lambda(t) = log(sqrt(a) / sqrt(1 - a)), the variable a DPM-Solver++ step is exact in.
"""
from __future__ import annotations

import numpy as np
import torch

SPACINGS = ("leading", "logsnr")


class Schedule:
    def __init__(self, n_timesteps: int, num_train_timesteps: int = 1000, beta_start: float = 0.00085,
                 beta_end: float = 0.012, steps_offset: int = 1, spacing: str = "leading"):
        if spacing not in SPACINGS:
            raise ValueError(f"timestep spacing {spacing!r}: one of {SPACINGS}")
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        acp = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.alphas_cumprod = np.concatenate([np.ones(1, np.float32), acp]).astype(np.float32)   # :218
        self.final_alpha_cumprod = np.float32(acp[0])
        self.n = int(n_timesteps)
        self.spacing = spacing
        self.skip = num_train_timesteps // self.n                                                # :216
        ratio = num_train_timesteps // self.n
        self.timesteps = [int(v) for v in (np.arange(self.n)[::-1] * ratio + steps_offset)]
        self.init_noise_sigma = 1.0
        if spacing == "logsnr":
            self.timesteps = self._logsnr_timesteps(self.timesteps[0])
            self.skip = None                       # the grid has no constant stride: next_t(t) is the following entry

    def alpha(self, t: int) -> np.float32:
        return self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod

    def lam(self, t: int) -> float:
        """half log-SNR 0.5 * log(a / (1 - a)) of timestep t >= 1, in fp64 from the fp32 table entry"""
        a = float(self.alphas_cumprod[t])
        return 0.5 * float(np.log(a / (1.0 - a)))

    def _logsnr_timesteps(self, t_hi: int):
        """n strictly decreasing integers from t_hi to 1, each the timestep whose lambda is nearest its uniform target"""
        n = self.n
        if n < 2 or n > t_hi:
            raise ValueError(f"timestep spacing 'logsnr': n = {n} timesteps, 2 .. {t_hi} fit between t = {t_hi} and t = 1")
        a = self.alphas_cumprod[1:t_hi + 1].astype(np.float64)
        lam = 0.5 * np.log(a / (1.0 - a))                          # lam[t - 1] = lambda(t), decreasing in t
        target = lam[-1] + np.arange(n) * (lam[0] - lam[-1]) / (n - 1)
        ts = [int(np.argmin(np.abs(lam - tg))) + 1 for tg in target]    # argmin takes the first minimum: ties go to the smaller t
        ts[0] = t_hi
        for i in range(1, n):
            ts[i] = min(ts[i], ts[i - 1] - 1)
        ts[n - 1] = 1
        for i in range(n - 2, -1, -1):
            ts[i] = max(ts[i], ts[i + 1] + 1)
        return ts

    def next_t(self, t: int) -> int:
        """the timestep a step from t moves to: t - skip on the 'leading' grid (also off the grid: the look-ahead's and the reference's
        arithmetic), the following list entry on the 'logsnr' grid, 0 behind the last entry"""
        t = int(t)
        if self.skip is not None:
            return t - self.skip
        i = self.timesteps.index(t)          # ValueError off the grid: this spacing has no stride to fall back on
        return self.timesteps[i + 1] if i + 1 < self.n else 0

    def index_at_or_below(self, t: int) -> int:
        """the first index i with timesteps[i] <= t (the list is decreasing)"""
        for i, v in enumerate(self.timesteps):
            if v <= t:
                return i
        raise ValueError(f"no timestep at or below {t}")
