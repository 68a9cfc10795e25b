"""Host side of the video sampler's per-step path (BASELINE config #5): the denoising loop of
video_gen/pipeline_i2vgen_xl.py:647-719 and the feature-injection schedule of video_gen/utils_attn.py:14-23,389-474, over
the HIP kernels `tmix_vpred_step` and `tmix_frame_inject`.  The I2VGen-XL UNet itself (diffusers `I2VGenXLUNet`, not in
the reference) is built natively in tweediemix_amd/i2vgen.py.  Two loops: `sample_loop`, the reference-shaped host loop, takes
the network as a callable (any module plugs in; the tests check it against the oracle's loop), and `VideoSampler`, the loop
run_video.py runs for one video or many, keeps the whole step of S videos on the device over an i2vgen.I2VVideoPlan.

Quirks kept: alpha(t) indexes the UN-shifted alphas_cumprod (unlike the image sampler) and falls back to
final_alpha_cumprod below 0 (:480-482); skip = 1000 // n (:647); the injection schedule is the first int(n * ratio)
timesteps, also active when t == 1000 (utils_attn.py:433,444); clips are hard-wired to b=2, t=16 there (:439,449)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .plan import ParamRing


SPACINGS = ("leading", "logsnr")
SOLVERS = ("ddim", "dpmpp2m")


class VideoSchedule:
    """alphas_cumprod [1000] (from the checkpoint's scheduler), leading timesteps with steps_offset (diffusers DDIMScheduler
    set_timesteps as configured for i2vgen-xl), skip = 1000 // n.

    spacing="logsnr" (no reference counterpart) keeps the table and the first timestep of the 'leading' grid and places the n
    timesteps uniformly in lambda(t) = log(sqrt(a) / sqrt(1 - a)) on the UN-shifted table (the construction of
    schedule.Schedule._logsnr_timesteps); skip is then None and next_alpha(t) is the following entry's alpha."""

    def __init__(self, alphas_cumprod, n_steps: int, steps_offset: int = 1, set_alpha_to_one: bool = False, spacing: str = "leading"):
        if spacing not in SPACINGS:
            raise ValueError(f"timestep spacing {spacing!r}: one of {SPACINGS}")
        self.acp = np.asarray(alphas_cumprod, np.float32)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.acp[0]
        self.n = n_steps
        self.spacing = spacing
        self.skip = len(self.acp) // n_steps
        self.timesteps = (np.arange(0, n_steps) * self.skip).round()[::-1].astype(np.int64) + steps_offset
        self._leading = self.timesteps                     # the injection schedule's noise range is defined on this grid
        if spacing == "logsnr":
            self.timesteps = self._logsnr_timesteps(int(self.timesteps[0]))
            self.skip = None                               # the grid has no constant stride
        self._index = {int(t): i for i, t in enumerate(self.timesteps)}

    def index(self, t: int):
        """the position of timestep t on the grid, None off it"""
        return self._index.get(int(t))

    def _logsnr_timesteps(self, t_hi: int):
        """n strictly decreasing integers from t_hi to 1, each the timestep whose lambda is nearest its uniform target (ties: the smaller t)"""
        n = int(self.n)
        if n < 2 or n > t_hi:
            raise ValueError(f"timestep spacing 'logsnr': n = {n} timesteps, 2 .. {t_hi} fit between t = {t_hi} and t = 1")
        if t_hi >= len(self.acp) or not 0.0 < float(self.acp[t_hi]) or not float(self.acp[1]) < 1.0:
            raise ValueError(f"timestep spacing 'logsnr': the alpha table has no finite log-SNR at t = {t_hi} or t = 1")
        a = self.acp[1:t_hi + 1].astype(np.float64)
        lam = 0.5 * np.log(a / (1.0 - a))                          # lam[t - 1] = lambda(t), decreasing in t
        target = lam[-1] + np.arange(n) * (lam[0] - lam[-1]) / (n - 1)
        ts = [int(np.argmin(np.abs(lam - tg))) + 1 for tg in target]    # argmin takes the first minimum
        ts[0] = t_hi
        for i in range(1, n):
            ts[i] = min(ts[i], ts[i - 1] - 1)
        ts[n - 1] = 1
        for i in range(n - 2, -1, -1):
            ts[i] = max(ts[i], ts[i + 1] + 1)
        return np.asarray(ts, np.int64)

    def alpha(self, t: int):
        return self.acp[int(t)] if t >= 0 else self.final_alpha_cumprod

    def next_alpha(self, t: int):
        """the alpha a step from t moves to: alpha(t - skip) on the 'leading' grid (also off the grid), the following entry's alpha on the
        'logsnr' grid, final_alpha_cumprod behind its last entry"""
        t = int(t)
        if self.skip is not None:
            return self.alpha(t - self.skip)
        i = self.index(t)
        if i is None:                                      # this spacing has no stride to fall back on
            raise ValueError(f"timestep {t} is not on the 'logsnr' grid")
        return self.alpha(int(self.timesteps[i + 1])) if i + 1 < len(self.timesteps) else self.final_alpha_cumprod

    def injection_schedule(self, ratio: float):
        k = int(self.n * ratio)
        if self.skip is None:                              # 'logsnr': the NOISE range of the leading grid's first k timesteps
            if k <= 0:
                return set()
            floor = int(self._leading[min(k, len(self._leading)) - 1])
            return set(int(t) for t in self.timesteps if int(t) >= floor)
        return set(int(t) for t in self.timesteps[:k]) if k >= 0 else set()


class SolverPhase:
    """the host's bookkeeping of solver="dpmpp2m": coeffs(t) -> the (cx, c0, c1) of the step at t and remembers it.  A step is second order
    exactly when the previous coeffs() call was for the preceding schedule entry, first order otherwise (the first step, any out-of-order or
    off-grid call); the injection state does not enter.  coeffs(t, eta) -> (cx, c0, c1, cz) of the SDE form of the same step
    (solver.video_multistep_eta_coeffs; eta = 0.0 gives coeffs(t)'s three values bit for bit and cz == 0.0), with the same bookkeeping.
    Under a guidance interval the loops call set_previous(None) in front of a step whose predecessor had the other guidedness
    (_at_border): the data prediction jumps where g goes from 9 to 1, so a border step is first order."""

    def __init__(self, schedule: VideoSchedule):
        self.schedule, self.prev = schedule, None

    def set_previous(self, t):
        """declare the step that ran last: the one for timestep t (its x0 is what the history buffer holds), or None for no usable history.
        For callers that put a state and a history in place themselves (tools/video_solver_cost.py times a second-order step this way)."""
        self.prev = None if t is None else self.schedule.index(t)

    def coeffs(self, t: int, eta=None):
        from .solver import video_multistep_coeffs, video_multistep_eta_coeffs
        sch, t = self.schedule, int(t)
        i = sch.index(t)
        second = i is not None and i > 0 and self.prev == i - 1
        self.prev = None                                   # a refused step leaves no history behind
        a = sch.alpha(t) if 0 <= t < len(sch.acp) else 0.0
        a_prev, a_next = sch.alpha(int(sch.timesteps[i - 1])) if second else None, sch.next_alpha(t) if float(a) > 0 else 0.0
        out = video_multistep_coeffs(t, a_prev, a, a_next, second) if eta is None else video_multistep_eta_coeffs(t, a_prev, a, a_next, second, eta)
        self.prev = i
        return out


def _at_border(phase, guided, prev_guided):
    """the order rule of a guidance interval, in front of the step that is about to ask `phase` (a SolverPhase, or None without the
    solver) for its coefficients: where the step's guidedness differs from its predecessor's the history holds an x0 of the other kind and is not
    usable -- set_previous(None), so the border step is first order.  -> guided, the next call's prev_guided (True in front of the first step)"""
    if phase is not None and bool(guided) != bool(prev_guided):
        phase.set_previous(None)
    return bool(guided)


def alphas_from_scheduler_config(cfg: dict):
    """alphas_cumprod (fp32 [num_train_timesteps]) and the VideoSchedule keyword arguments a diffusers DDIMScheduler built
    from `scheduler/scheduler_config.json` would hold (what `pipe.scheduler.alphas_cumprod` is at pipeline_i2vgen_xl.py:480):
    the beta schedule, `rescale_betas_zero_snr`, `steps_offset` and `set_alpha_to_one` follow the checkpoint, in the
    float32 arithmetic diffusers uses (torch.linspace / cumprod / sqrt on float32 tensors)."""
    import math
    T = int(cfg.get("num_train_timesteps", 1000))
    b0, b1 = float(cfg.get("beta_start", 0.0001)), float(cfg.get("beta_end", 0.02))
    sched = cfg.get("beta_schedule", "linear")
    if cfg.get("trained_betas") is not None:
        betas = torch.tensor(cfg["trained_betas"], dtype=torch.float32)
    elif sched == "linear":
        betas = torch.linspace(b0, b1, T, dtype=torch.float32)
    elif sched == "scaled_linear":
        betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, T, dtype=torch.float32) ** 2
    elif sched == "squaredcos_cap_v2":                       # betas_for_alpha_bar: python floats, then one float32 tensor
        ab = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        betas = torch.tensor([min(1 - ab((i + 1) / T) / ab(i / T), 0.999) for i in range(T)], dtype=torch.float32)
    else:
        raise ValueError(f"beta_schedule {sched!r} is not one of diffusers DDIMScheduler's")
    if cfg.get("rescale_betas_zero_snr", False):             # rescale_zero_terminal_snr
        abs_ = torch.cumprod(1.0 - betas, dim=0).sqrt()
        a0, aT = abs_[0].clone(), abs_[-1].clone()
        abs_ = (abs_ - aT) * (a0 / (a0 - aT))
        bar = abs_ ** 2
        alphas = torch.cat([bar[0:1], bar[1:] / bar[:-1]])
        betas = 1 - alphas
    acp = torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float32)
    return acp, dict(steps_offset=int(cfg.get("steps_offset", 0)), set_alpha_to_one=bool(cfg.get("set_alpha_to_one", True)))


def injection_active(t: int, schedule) -> bool:
    return schedule is not None and (int(t) in schedule or int(t) == 1000)


class FeatureInjector:
    """what `register_conv_control_efficient` + `register_time` do to mid_block.resnets[0,1] (hard copy of the first
    frame's features) and up_blocks[1].resnets[0] (interp blend): call `apply(site, features)` on the resnet OUTPUT
    [(2*16), ...] of those three modules (e.g. from a forward hook)."""

    SITES = {"mid_block.resnets.0": "hard", "mid_block.resnets.1": "hard", "up_blocks.1.resnets.0": "interp"}

    def __init__(self, schedule, interp: float, clips: int = 2, frames: int = 16):
        self.schedule, self.interp, self.clips, self.frames = schedule, interp, clips, frames
        self.t = None

    def register_time(self, t: int):
        self.t = int(t)

    def apply(self, site: str, features: torch.Tensor) -> torch.Tensor:
        if injection_active(self.t, self.schedule):
            ops.frame_inject(features, self.clips, self.frames, None if self.SITES[site] == "hard" else self.interp)
        return features


def _check_solver(solver):
    if solver not in SOLVERS:
        raise ValueError(f"solver={solver!r}: one of {SOLVERS}")
    return solver != "ddim"


def _check_eta(eta, noise_seeds, videos):
    """eta in [0, 1] and, for eta > 0, one integer noise seed per video -> (eta, seeds or None); host only"""
    from .solver import validate_eta
    eta = validate_eta(eta)
    if noise_seeds is None:
        if eta > 0.0:
            raise ValueError(f"eta={eta}: noise_seeds (one integer per video) are what the step's noise is a function of")
        return eta, None
    seeds = [int(s) for s in noise_seeds]
    if len(seeds) != int(videos):
        raise ValueError(f"noise_seeds: {len(seeds)} values for {int(videos)} videos")
    return eta, seeds


def _noise_step(schedule, t, eta, phase):
    """the stochastic step at timestep t (eta > 0) -> (move, cz, schedule index): move = (cx, c0, c1) of the SDE solver step when `phase` is the
    solver's bookkeeping, else the DDIM step's (sa_next, s1_dir).  The noise is indexed by the schedule entry, so t must be on the grid."""
    from .solver import ddim_eta_coeffs
    i = schedule.index(t)
    if i is None:
        raise ValueError(f"eta={eta}: t = {int(t)} is not one of the schedule's timesteps (the noise is indexed by the schedule entry)")
    if phase is not None:
        cx, c0, c1, cz = phase.coeffs(int(t), eta)
        return (cx, c0, c1), cz, i
    _, _, san, s1d, cz = ddim_eta_coeffs(schedule.alpha(int(t)), schedule.next_alpha(int(t)), eta)
    return (san, s1d), cz, i


def _check_hold(hold, noise_seeds, videos, channels, frames, h, w):
    """hold = (x0, weight) of DESIGN.md 7p -> (x0 fp32 [S or 1, C, 1 or F, h, w], weight fp32 [S or 1, 1 or F, h, w]) as contiguous host tensors,
    or None for hold None.  Shapes, finiteness and the weight's range are checked here, on the host, before the GPU is touched; the hold's fixed
    noise is a function of the video's seed, so noise_seeds are needed at eta == 0 too."""
    if hold is None:
        return None
    if noise_seeds is None:
        raise ValueError("hold: noise_seeds (one integer per video) are what the held part's fixed noise is a function of, also at eta = 0")
    if not isinstance(hold, (tuple, list)) or len(hold) != 2:
        raise ValueError("hold: a pair (x0, weight)")
    x0, wt = (torch.as_tensor(a).detach().to("cpu", torch.float32).contiguous() for a in hold)
    S, C, F = int(videos), int(channels), int(frames)
    if x0.dim() != 5 or x0.shape[0] not in (1, S) or x0.shape[1] != C or x0.shape[2] not in (1, F) or tuple(x0.shape[3:]) != (h, w):
        raise ValueError(f"hold: x0 of shape {tuple(x0.shape)}; [{S} or 1, {C}, {F} or 1, {h}, {w}] is what this sampler holds")
    if wt.dim() != 4 or wt.shape[0] not in (1, S) or wt.shape[1] not in (1, F) or tuple(wt.shape[2:]) != (h, w):
        raise ValueError(f"hold: weight of shape {tuple(wt.shape)}; [{S} or 1, {F} or 1, {h}, {w}] is what this sampler holds")
    if not bool(torch.isfinite(x0).all()):
        raise ValueError("hold: x0 has values that are not finite")
    if not bool(((wt >= 0.0) & (wt <= 1.0)).all()):
        raise ValueError("hold: weight outside [0, 1] (1 = held, 0 = sampled)")
    return x0, wt


def _hold_step(schedule, t, eta, phase):
    """the step at timestep t under a hold -> (move, cz, schedule index, the alpha of the state it writes or None on the schedule's last step).
    eta > 0: _noise_step's values; eta == 0: the deterministic parent's own coefficients ((sa_next, s1_next) of ops.step_coeffs, phase.coeffs(t))
    with cz = 0, so that a weight of 0 everywhere is the run without the hold bit for bit."""
    t = int(t)
    if eta > 0.0:
        move, cz, i = _noise_step(schedule, t, eta, phase)
    else:
        i = schedule.index(t)
        move = phase.coeffs(t) if phase is not None else ops.step_coeffs(schedule.alpha(t), schedule.next_alpha(t))[2:]
        cz, i = 0.0, 0 if i is None else i
    last = schedule.index(t) == len(schedule.timesteps) - 1
    return tuple(move), cz, i, None if last else schedule.next_alpha(t)


@torch.no_grad()
def sample_loop(unet, latents: torch.Tensor, schedule: VideoSchedule, guidance_scale: float, injector: FeatureInjector | None = None,
                solver: str = "ddim", guidance_rescale: float = 0.0, eta: float = 0.0, noise_seeds=None, hold=None, guidance_interval=None,
                unet_cond=None):
    """pipeline_i2vgen_xl.py:680-719.  unet(latent_model_input [2B,C,F,H,W], t) -> v-prediction of the same shape (the
    caller closes over prompt/image conditioning; an i2vgen plan behind it needs its `inject` flag set for t, from
    injection_active); latents [B,C,F,H,W] on the GPU in the model dtype.  solver="dpmpp2m": every step is tmix_vpred_step_ms on the
    model dtype with an fp32 history of x0.  guidance_rescale = phi > 0: every step is tmix_vpred_rescale_factors on
    v (one factor per video, g read from a small device tensor) and then the _rs form of the step entry; 0 is the loop without it, launch for launch.
    eta > 0 with noise_seeds, one integer per video: every step is tmix_vpred_step_noise, the same move plus cz * z with z a
    function of (the video's seed, the schedule index, the element's index in its video); 0 is the loop without it, launch for launch.
    hold = (x0, weight) with noise_seeds: x_T is composited once (tmix_video_hold_composite, on a copy) and every step is
    tmix_vpred_step_hold, which keeps x0 under the weight at the noise level of the state it writes; None is the loop without it.
    guidance_interval = (t_hi, t_lo): a timestep outside it is unguided -- unet_cond(latents [B,C,F,H,W], t) -> the conditional
    v-prediction [B,...] alone, then tmix_vpred_step_cond (no factors launch, whatever guidance_rescale is); a solver step next to a border is
    first order.  None, or an interval holding every timestep, is the loop without it, launch for launch."""
    from .guidance import is_guided, validate_interval, validate_phi
    ms = _check_solver(solver)
    phi = validate_phi(guidance_rescale)
    interval = validate_interval(guidance_interval)
    if unet_cond is None and any(not is_guided(interval, t) for t in schedule.timesteps):
        raise ValueError(f"guidance_interval={interval}: the schedule has unguided timesteps and unet_cond, the network on the text half alone, is None")
    eta, seeds = _check_eta(eta, noise_seeds, latents.shape[0])
    hold = _check_hold(hold, seeds, *latents.shape)
    x = latents.contiguous()
    keys = ops.noise_keys(seeds, x.device) if eta > 0.0 or hold is not None else None
    if hold is not None:
        hx, hw_ = (a.to(x.device) for a in hold)
        x = ops.video_hold_composite(x.clone(), schedule.alpha(int(schedule.timesteps[0])), keys, hx, hw_)
    if ms:
        phase, hist = SolverPhase(schedule), torch.zeros_like(x, dtype=torch.float32)
    was_guided = True
    if phi > 0.0:
        B = x.shape[0]
        g_dev = torch.zeros(8, device=x.device, dtype=torch.float32)
        g_dev[0] = float(guidance_scale)
        fac, ws = torch.empty(B, device=x.device, dtype=torch.float32), ops.vpred_rescale_ws(B, x.device)
    for t in schedule.timesteps:
        if injector is not None:
            injector.register_time(t)
        if ms and interval is not None:
            was_guided = _at_border(phase, is_guided(interval, t), was_guided)      # a border step is first order
        if not is_guided(interval, t):                    # the text half alone: no CFG, no factors launch
            v = unet_cond(x, int(t)).contiguous()
            phs = phase if ms else None
            at, hist_ = schedule.alpha(int(t)), hist if ms else None
            if hold is not None:
                move, cz, i, aw = _hold_step(schedule, int(t), eta, phs)
                x = ops.vpred_step_cond(x, v, at, move, hist_, cz, keys, i, aw, hx, hw_)
            elif eta > 0.0:
                move, cz, i = _noise_step(schedule, int(t), eta, phs)
                x = ops.vpred_step_cond(x, v, at, move, hist_, cz, keys, i)
            else:
                move = phase.coeffs(int(t)) if ms else ops.step_coeffs(at, schedule.next_alpha(int(t)))[2:]
                x = ops.vpred_step_cond(x, v, at, move, hist_)
            continue
        v = unet(torch.cat([x, x]), int(t)).contiguous()
        if phi > 0.0:
            ops.vpred_rescale_factors(v, g_dev, 0, phi, out=fac, ws=ws)
        if hold is not None:
            move, cz, i, aw = _hold_step(schedule, int(t), eta, phase if ms else None)
            x = ops.vpred_step_hold(x, v, guidance_scale, schedule.alpha(int(t)), move, cz, keys, i, aw, hx, hw_, x0_prev=hist if ms else None,
                                    factors=fac if phi > 0.0 else None)
        elif eta > 0.0:
            move, cz, i = _noise_step(schedule, int(t), eta, phase if ms else None)
            x = ops.vpred_step_noise(x, v, guidance_scale, schedule.alpha(int(t)), move, cz, keys, i, x0_prev=hist if ms else None,
                                     factors=fac if phi > 0.0 else None)
        elif phi > 0.0:
            if ms:
                x = ops.vpred_step_ms_rs(x, v, guidance_scale, schedule.alpha(int(t)), phase.coeffs(int(t)), hist, fac)
            else:
                x = ops.vpred_step_rs(x, v, guidance_scale, schedule.alpha(int(t)), schedule.next_alpha(int(t)), fac)
        elif ms:
            x = ops.vpred_step_ms(x, v, guidance_scale, schedule.alpha(int(t)), phase.coeffs(int(t)), hist)
        else:
            x = ops.vpred_step(x, v, guidance_scale, schedule.alpha(int(t)), schedule.next_alpha(int(t)))
    return x


class VideoSampler:
    """sample_loop for S videos in one UNet call, with the whole step on the device.  `plan` is an i2vgen.I2VVideoPlan; the state
    [S,4,F,h,w] fp32 is updated in place.  One step = tmix_video_step_prologue (state -> both CFG halves' inputs, t -> their
    timestep inputs) -> the plan's chains -> tmix_vpred_step_dev (CFG + v-prediction + DDIM for every video, coefficients from the
    device parameter buffer).  With graphs (default) that sequence is captured once per injection state (the injection ops are
    decided at record time) and a timestep is one 32-byte upload from a pinned staging ring plus one replay; use_graphs=False issues
    the same launches eagerly.  Video s of a batch is bit for bit what sample_loop gives for it alone (tmix_vpred_step_dev is
    tmix_vpred_step per element).

    solver="dpmpp2m" (DESIGN.md 7j): the step ends in tmix_vpred_step_ms_dev instead, on one fp32 history buffer `x0_prev` of the state's
    shape; params is then {t, sa, s1, cx, c0, c1, g, 0} and the graphs are keyed (inject, "ms").  The order of a step sits in the uploaded
    coefficients (SolverPhase), so one graph serves both orders and a step stays one 32-byte upload and one replay.

    guidance_rescale = phi > 0: behind the plan's chains come tmix_vpred_rescale_factors (two small launches: one factor per video
    into `rs_factors` [S], g read on the device from params) and the _rs_dev form of whichever step entry runs; the graphs are keyed (inject, "rs")
    and (inject, "ms", "rs"); phi is a launch argument fixed at capture, so a step stays one 32-byte upload and one replay.  The statistics'
    partition per video does not depend on S: video s of a batch is still bit for bit its single run.  phi = 0 is the sampler without it: no new
    launch, buffer or graph key.

    eta > 0 with noise_seeds, one integer per video: the step ends in tmix_vpred_step_noise_dev, the stochastic form of whichever
    of the four entries above would run; params and the staging slots are then 12 floats (the parent's 8, then {cz, schedule index, 0, 0}), the
    graphs carry a trailing "eta" in their keys -- (inject, "eta"), (inject, "ms", "eta"), (inject, "rs", "eta"), (inject, "ms", "rs", "eta") --
    and a step stays one (48-byte) upload and one replay.  `noise_keys` int32 [S, 2] holds the videos' key words at a fixed address and is
    written once per sample(); set_noise_seeds replaces the seeds between runs.  A video's noise is a function of its own seed, the schedule
    index and the element's index in the video: video s of a batch is still bit for bit its single run.  eta = 0 is the sampler without it: no
    new launch, buffer, graph key or upload size.

    hold = (x0, weight) with noise_seeds (also at eta = 0: the held part's fixed noise is keyed by the video's seed): x0 fp32
    [S or 1, C, 1 or F, h, w] is the clean latent held where weight fp32 [S or 1, 1 or F, h, w] is 1, sampled where it is 0, blended in between.
    sample() composites x_T once (tmix_video_hold_composite at the first timestep's noise level) and every step ends in tmix_vpred_step_hold_dev,
    the noise entry (cz = 0 at eta = 0) followed by the blend at the noise level of the state it writes ((1, 0) on the last step: the final latent
    IS x0 wherever the weight is 1).  `hold_x0`, `hold_w` and `noise_keys` sit at fixed addresses (set_hold rewrites their contents), params is
    12 floats with (ha, hs) in slots 10 and 11, the graph keys gain a trailing "hold", and a step stays one 48-byte upload and one replay.
    hold = None is the sampler without it: no new launch, buffer, graph key or upload size.

    guidance_interval = (t_hi, t_lo) (guidance.validate_interval): a timestep outside it is unguided and its step is
    tmix_video_step_prologue_cond (state and t into the text half's inputs alone) -> plan.run_cond() (the text half's chain alone, on the current
    stream) -> tmix_vpred_step_cond_dev in the form of whichever step entry would run (history, keys, hold arrays) -- S clips instead of 2S, no
    factors launch whatever guidance_rescale is.  The uploaded floats are the guided step's (g is not read), so a step stays one 32- or 48-byte
    upload and one replay; the graph key is the guided key without "rs" and with a trailing "cond": (inject, "cond"), (inject, "ms", "eta",
    "hold", "cond").  A solver step whose predecessor had the other guidedness is first order (SolverPhase).  None, or an interval that holds
    every timestep of the schedule, is the sampler without it: no new launch, buffer, graph key or upload size."""

    def __init__(self, plan, schedule: VideoSchedule, guidance_scale: float, injector: FeatureInjector | None = None, use_graphs: bool = True,
                 solver: str = "ddim", guidance_rescale: float = 0.0, eta: float = 0.0, noise_seeds=None, hold=None, guidance_interval=None):
        from .guidance import validate_interval, validate_phi
        self.guidance_interval = validate_interval(guidance_interval)                     # host only: refused before the GPU is touched
        self.plan, self.schedule, self.g, self.injector, self.use_graphs = plan, schedule, float(guidance_scale), injector, use_graphs
        self.solver, self.ms = solver, _check_solver(solver)
        self.guidance_rescale = validate_phi(guidance_rescale)
        self.eta, self._noise_seeds = _check_eta(eta, noise_seeds, plan.videos)          # host only: refused before the GPU is touched
        cfg = plan.cfg
        hold = _check_hold(hold, self._noise_seeds, plan.videos, cfg.in_channels, plan.frames, plan.h, plan.w)      # host only, as above
        wide = self.eta > 0.0 or hold is not None         # the 12-float parameter layout and the videos' keys
        dev = plan.plans[0].dev
        self.state = torch.zeros(plan.videos, cfg.in_channels, plan.frames, plan.h, plan.w, device=dev, dtype=torch.float32)
        # {t, sa, s1, sa_next, s1_next, g, -, -}; solver: {t, sa, s1, cx, c0, c1, g, -}; eta > 0 or a hold: four more floats {cz, schedule index, ha, hs}
        self.params = torch.zeros(12 if wide else 8, device=dev, dtype=torch.float32)
        # staging for the asynchronous parameter upload (as the image sampler's step_params)
        self._ring = ParamRing(width=12) if wide else ParamRing()
        self.noise_keys = self._keys_stale = None
        if wide:                                          # int32 [S, 2]: every video's key words at an address the captured steps keep
            self.noise_keys = torch.zeros(plan.videos, 2, device=dev, dtype=torch.int32)
            self._keys_stale = True
        self.hold_x0 = self.hold_w = None
        if hold is not None:                              # at addresses the captured steps keep
            self.hold_x0, self.hold_w = (a.to(dev) for a in hold)
        self.graphs = {}
        self.x0_prev = torch.zeros_like(self.state) if self.ms else None
        self.phase = SolverPhase(schedule) if self.ms else None
        self._was_guided = True                           # the guidedness of the step before (read under a guidance interval only)
        self.rs_factors = self._rs_ws = None
        if self.guidance_rescale > 0.0:                   # allocated once; the workspace needs no initial contents
            self.rs_factors = torch.ones(plan.videos, device=dev, dtype=torch.float32)
            self._rs_ws = ops.vpred_rescale_ws(plan.videos, dev)

    def set_noise_seeds(self, seeds):
        """the integer seed of every video's step noise (eta > 0) for the runs that follow: the next sample() (or step()) writes the key words
        into `noise_keys`, whose address the captured steps keep"""
        _, seeds = _check_eta(self.eta, seeds, self.plan.videos)
        if seeds is None and self.hold_x0 is not None:
            raise ValueError("hold: noise_seeds (one integer per video) are what the held part's fixed noise is a function of, also at eta = 0")
        self._noise_seeds = seeds
        if self.noise_keys is not None:
            self._keys_stale = True

    def set_hold(self, x0, weight):
        """new contents, of the shapes the sampler was built with, for the held latent and its weight in the runs that follow (the addresses stay)"""
        if self.hold_x0 is None:
            raise ValueError("set_hold: this sampler was built without hold=")
        x0, wt = _check_hold((x0, weight), self._noise_seeds, *self.state.shape)
        if x0.shape != self.hold_x0.shape or wt.shape != self.hold_w.shape:
            raise ValueError(f"set_hold: shapes {tuple(x0.shape)} / {tuple(wt.shape)}; the sampler holds {tuple(self.hold_x0.shape)} / {tuple(self.hold_w.shape)}")
        self.hold_x0.copy_(x0)
        self.hold_w.copy_(wt)

    def _write_keys(self):
        self.noise_keys.copy_(ops.noise_keys(self._noise_seeds, self.noise_keys.device))
        self._keys_stale = False

    def _enqueue_cond(self):
        """the unguided step: the text half alone, then the COND form of the step entry that would run; no factors launch"""
        xc, tc, ec = self.plan.cond_half
        ops.video_step_prologue_cond(self.state, xc, tc, self.params)
        self.plan.run_cond()
        ops.vpred_step_cond_dev(self.state, ec, self.params, x0_prev=self.x0_prev, keys=self.noise_keys, hold_x0=self.hold_x0, hold_w=self.hold_w)

    def _enqueue(self):
        (xu, tu, eu), (xc, tc, ec) = self.plan.halves
        ops.video_step_prologue(self.state, xu, tu, xc, tc, self.params)
        self.plan.run()
        if self.guidance_rescale > 0.0:
            ops.vpred_rescale_factors_dev(eu, ec, self.state.shape[0], self.state[0].numel(), self.params, 6 if self.ms else 5,
                                          self.guidance_rescale, out=self.rs_factors, ws=self._rs_ws)
        if self.hold_x0 is not None:
            ops.vpred_step_hold_dev(self.state, eu, ec, self.params, self.noise_keys, self.hold_x0, self.hold_w, x0_prev=self.x0_prev,
                                    factors=self.rs_factors)
        elif self.eta > 0.0:
            ops.vpred_step_noise_dev(self.state, eu, ec, self.params, self.noise_keys, x0_prev=self.x0_prev, factors=self.rs_factors)
        elif self.guidance_rescale > 0.0:
            ops.vpred_step_rs_dev(self.state, eu, ec, self.params, self.rs_factors, x0_prev=self.x0_prev)
        elif self.ms:
            ops.vpred_step_ms_dev(self.state, eu, ec, self.x0_prev, self.params)
        else:
            ops.vpred_step_dev(self.state, eu, ec, self.params)

    def _upload(self, t):
        sch = self.schedule
        if self.hold_x0 is not None:
            move, cz, i, aw = _hold_step(sch, t, self.eta, self.phase)       # first: a refused step rewrites no staging slot
            ops.video_step_params_hold(t, self.g, sch.alpha(int(t)), move, cz, i, aw, out=self._ring.next())
            self._ring.upload(self.params)
            return
        if self.eta > 0.0:
            move, cz, i = _noise_step(sch, t, self.eta, self.phase)          # first: a refused step rewrites no staging slot
            ops.video_step_params_noise(t, self.g, sch.alpha(int(t)), move, cz, i, out=self._ring.next())
            self._ring.upload(self.params)
            return
        coeffs = self.phase.coeffs(t) if self.ms else None          # first: a refused step rewrites no staging slot
        hp = self._ring.next()
        if self.ms:
            ops.video_step_params_ms(t, self.g, sch.alpha(int(t)), coeffs, out=hp)
        else:
            ops.video_step_params(t, self.g, sch.alpha(int(t)), sch.next_alpha(int(t)), out=hp)
        self._ring.upload(self.params)

    def step(self, t):
        inject = False
        if self.injector is not None:
            self.injector.register_time(t)
            inject = injection_active(int(t), self.injector.schedule)
            self.plan.inject, self.plan.interp = inject, self.injector.interp
        if self._keys_stale:                              # a step() outside sample() after new seeds
            self._write_keys()
        guided = True
        if self.guidance_interval is not None:            # without an interval nothing below differs from the sampler without the feature
            from .guidance import is_guided
            guided = is_guided(self.guidance_interval, t)
            self._was_guided = _at_border(self.phase, guided, self._was_guided)      # a border step is first order
        enqueue = self._enqueue if guided else self._enqueue_cond
        self._upload(t)
        if not self.use_graphs:
            enqueue()
            return
        key = (inject, "ms") if self.ms else inject
        if self.guidance_rescale > 0.0:
            key = (key if self.ms else (inject,)) + ("rs",)
        if self.eta > 0.0:
            key = (key if isinstance(key, tuple) else (inject,)) + ("eta",)
        if self.hold_x0 is not None:
            key = (key if isinstance(key, tuple) else (inject,)) + ("hold",)
        if not guided:                                    # the guided key without "rs", then "cond"
            key = tuple(k for k in (key if isinstance(key, tuple) else (inject,)) if k != "rs") + ("cond",)
        g = self.graphs.get(key)
        if g is None:
            enqueue()                                     # warm-up outside capture; it has already performed this step
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            keep = self.state.clone()
            keep_h = self.x0_prev.clone() if self.ms else None
            with torch.cuda.graph(g):
                enqueue()
            self.state.copy_(keep)
            if self.ms:
                self.x0_prev.copy_(keep_h)
            self.graphs[key] = g
            return
        g.replay()

    @torch.no_grad()
    def sample(self, latents: torch.Tensor) -> torch.Tensor:
        """latents [S,4,F,h,w] -> the final latents (a copy of the state)."""
        self.state.copy_(latents)
        if self.noise_keys is not None:
            self._write_keys()
        if self.hold_x0 is not None:                      # x_T under the hold, once, at the first timestep's noise level
            ops.video_hold_composite(self.state, self.schedule.alpha(int(self.schedule.timesteps[0])), self.noise_keys, self.hold_x0, self.hold_w)
        for t in self.schedule.timesteps:
            self.step(int(t))
        return self.state.clone()


# ------------------------------------------------------------------------------------------ image side of the pipeline (host)
def center_crop_wide(image, resolution):
    """video_gen/pipeline_i2vgen_xl.py:772-793: BOX-resize so the image covers `resolution` (w, h), then centre crop (PIL)."""
    import PIL.Image
    scale = min(image.size[0] / resolution[0], image.size[1] / resolution[1])
    image = image.resize((round(image.width // scale), round(image.height // scale)), resample=PIL.Image.BOX)
    x1 = (image.width - resolution[0]) // 2
    y1 = (image.height - resolution[1]) // 2
    return image.crop((x1, y1, x1 + resolution[0], y1 + resolution[1]))


def resize_bilinear(image, resolution):
    """:759-769."""
    import PIL.Image
    return image.resize(resolution, PIL.Image.BILINEAR)


def clip_pixel_values(image, mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711)):
    """`_encode_image` (:300-315): PIL -> [0,1] float -> CLIP normalisation, no further resize / crop.  [1,3,H,W] fp32."""
    a = torch.from_numpy(np.asarray(image, np.float32) / 255.0).permute(2, 0, 1)[None]
    return (a - torch.tensor(mean)[None, :, None, None]) / torch.tensor(std)[None, :, None, None]


def vae_pixel_values(image):
    """VideoProcessor.preprocess: PIL -> [-1,1] float, [1,3,H,W]."""
    return torch.from_numpy(np.asarray(image, np.float32) / 255.0).permute(2, 0, 1)[None] * 2.0 - 1.0


def prepare_image_latents(latent_sample, num_frames, scaling_factor=0.18215, cfg=True):
    """:421-451 after `vae.encode(image).latent_dist.sample()`: scale, add the frame axis, append one constant plane per later
    frame holding its position (frame_idx+1)/(num_frames-1) in all 4 channels, duplicate for classifier-free guidance."""
    il = (latent_sample * scaling_factor).unsqueeze(2)
    masks = [torch.ones_like(il[:, :, :1]) * ((f + 1) / (num_frames - 1)) for f in range(num_frames - 1)]
    if masks:
        il = torch.cat([il, torch.cat(masks, dim=2)], dim=2)
    return torch.cat([il] * 2) if cfg else il
