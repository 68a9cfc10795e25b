"""Tweedie-mix sampler: host-side mirror of the reference's `Tweediemix` hot path.

Same method names, argument meaning and step semantics as fusion_generation/fusion_sampling.py
(`alpha` :305-307, `denoise_step` :309-474, `init_fusion` :476-483, `run_fusion` :485-489,
`sample_loop` :490-530) and fusion_sampling_lora.py (`--t_stop` window :324,378,476-492), with

* phase decisions and alpha tables on the host as plain ints/floats (the reference syncs the device
  several times per step through `.item()` and CPU-tensor indexing),
* one UNet launch plan per call kind (fusion / start / plain), each with its own cross-attention K/V
  cache,
* CFG + Tweedie + blend + DDIM done by ONE kernel (tmix_fused_tweedie_step_dev) that updates the latent
  state in place,
* optionally a KEEP REGION (set_keep / clear_keep): part of the latent held at a given clean latent, re-noised inside the same kernel
  (tmix_fused_tweedie_step_keep_dev) to the level of every state the loop writes,
* optionally (solver="dpmpp2m") a second-order multistep move on the blended estimate behind the first timestep
  (tmix_fused_tweedie_step_ms_dev), on an optional log-SNR timestep grid (timestep_spacing="logsnr"),
* optionally (guidance_rescale=phi > 0) the guided prediction of every concept row scaled back towards the standard deviation of its
  conditional prediction (tmix_cfg_rescale_factors in front of the *_rs_dev form of whichever step entry runs), in every step of every phase,
* optionally (eta > 0) noise added by every step that advances the trajectory, generated inside the step kernel from (seed, schedule index,
  canvas coordinate) (tmix_fused_tweedie_step_noise_dev: one entry for the stochastic form of the DDIM, solver and rescale steps),
* optionally (guidance_interval=(t_hi, t_lo)) trajectory steps at timesteps outside the interval that run the UNet without the unconditional row
  (plan kinds "fusion_c" / "fusion_base_c" / "plain_c") and tmix_fused_tweedie_step_cond_dev on its rows,
* ONE hipGraph per (call kind, step mode) holding the whole step -- latent broadcast + timestep
  (tmix_step_prologue), the UNet launch chains, the fused step for all co-batched seeds: a timestep is one 32-byte
  parameter upload and one graph replay.

The constructor takes prompt embeddings, masks and weights as tensors; `tweediemix_amd/text.py` (tokenizer + text
towers), `vae.py` (final / preview decode) and `masks.py` (side-car contract) produce them from the reference's inputs
-- the CLI `fusion_generation/fusion_sampling.py` wires them together.  The segmentation process itself
(GroundingDINO + SAM) stays an external command.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import lib as L
from . import ops
from .schedule import Schedule
from .guidance import is_guided, validate_apg, validate_interval, validate_phi
from .plan import ParamRing
from .solver import SOLVERS, ddim_eta_coeffs, multistep_coeffs, multistep_eta_coeffs, validate_eta
from .unet import KVCache, PlanGroup, TokenMapSpec, TokenPropSpec, UNetPlan, UNetWeights

F32 = torch.float32


def seed_everything(seed: int):
    """utils_custom.py:10-14"""
    import random

    import numpy as np
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


DEFAULTS = dict(seed=182, guidance_scale=9.0, n_timesteps=50, t_cond=0.4, t_stop=0.9, resampling_steps=10,
                jumping_steps=5, resolution_h=1024, resolution_w=1024, crops_coords_top_left_h=0,
                crops_coords_top_left_w=0)      # argparse defaults of fusion_sampling.py:534-585


def make_config(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return SimpleNamespace(**d)


class Tweediemix:
    """config: namespace with the reference's flag names (guidance_scale, n_timesteps, t_cond,
    [t_stop], resampling_steps, jumping_steps, resolution_h/w, crops_coords_top_left_h/w, seed).

    weights           UNetWeights (base UNet + K concept weight sets, kind 'custom' | 'lora' | 'none')
    text_embeds       ([K+2,77,D], [K+2,P])  rows: 0 uncond, 1 multi-concept prompt, 2.. per-concept prompts
    text_embeds_single([K,77,D],   [K,P])    rows: 0 uncond, 1.. single-concept prompts without modifier tokens
    mask_provider     callable(x0_preview [1,4,h,w]) -> masks [K,1,h,w] fp32 (stands in for decode +
                      run_expand.py + preprocess_mask at fusion_sampling.py:453-469)
    lora              True selects the fusion_sampling_lora.py window semantics (needs config.t_stop)
    strict_reference  keep the hooks' hard-coded `batch == 4` routing test (utils_custom.py:62)
    attention_masks   None (masks come from mask_provider) or dict(tokens=[[positions of concept 1], ...] (<= 32 in all), threshold=0.5,
                      levels=None, level_weights=None): the masks come from the cross-attention maps of the look-ahead's calls
                      on the scene prompt (a "probe" plan: the "plain" rows plus tmix_xattn_token_maps launches) through
                      masks.attention_masks; mask_provider is not called.  Needs jumping_steps >= 1.  propagate=N (0..3, default 0):
                      the maps are pushed N times through the self-attention of the last look-ahead call (a "propagate" plan: the
                      "plain" rows plus tmix_sattn_propagate launches, replayed on that call's input) before they are thresholded.
                      shape="rect" (default: every mask becomes its bounding rectangle, the side-car's rule) or "free": the largest
                      component's own outline, holes filled (fill_holes=True), overlaps of any number of concepts resolved towards the
                      highest score (tmix_attn_shapes, once per seed), so that the foreground masks are disjoint.
    canvas            None, or dict(height, width, overlap) in pixels (multiples of 8): a WIDE CANVAS sampled as overlapping windows of
                      resolution_h x resolution_w (canvas.window_layout) that share every UNet launch like co-batched seeds and are
                      reconciled after every step (tmix_window_consensus behind the fused step, inside the captured graph).  run_fusion /
                      sample_loop / denoise_step then take and return canvas latents [n_seeds, 4, height / 8, width / 8], mask_provider
                      gets the assembled preview [1, 4, height / 8, width / 8] and returns [K, 1, height / 8, width / 8], decode_final /
                      decode_latent return [n, 3, height, width].  n_seeds * windows <= 8; not with attention_masks, set_keep or
                      n_streams > 1.  A canvas of the window's size is one window: today's launches and bits.
    mask_soften       None (the masks of every source are used as they come: no launch, today's bits), or dict(feather=<latent px>,
                      dilate=<latent px>, normalize=bool): the first K-1 masks of every source -- mask_provider (one call or one per seed),
                      attention_masks, the canvas's provider -- are thresholded at 0.5 and become blend weights from the distance to each
                      region's border (masks.soft_masks: tmix_mask_edt + tmix_soft_masks, once per mask acquisition): grown by `dilate`,
                      ramped over `feather`, and with normalize=True a partition of unity where regions overlap.  On a canvas this
                      happens on the canvas grid before the masks are cropped, so overlapping windows hold identical weights.
                      feather <= 1 with dilate = 0 and normalize=False gives the bits of None.  soft_weights holds what the last
                      acquisition produced ([K,1,H,W] or [n,K,1,H,W] on the grid the masks were built on).  The public `masks` setter stays
                      raw: what is assigned there is what the fused step reads.
    solver            "ddim" (the reference's first-order steps: today's launches and bits) or "dpmpp2m": every trajectory step behind the first
                      timestep is a DPM-Solver++(2M) step on the blended Tweedie estimate (tmix_fused_tweedie_step_ms_dev: x' = cx x + c0 x0 +
                      c1 x0_prev, coefficients from solver.multistep_coeffs), second order exactly when the previous call ran a solver step of
                      the same mode on the preceding schedule entry.  The first timestep, the look-ahead and the propagate rounds stay on the
                      DDIM entry.  Not with set_keep.  DESIGN.md 7i.
    timestep_spacing  "leading" (the reference's grid) or "logsnr": n_timesteps uniform in log-SNR from the 'leading' grid's first timestep to
                      t = 1 (schedule.Schedule(spacing="logsnr")); skip is then None, and t_cond / t_stop keep their noise range
                      (_window_index).  Independent of `solver`.
    guidance_rescale  phi in [0, 1], default 0.0 = off (today's entries, launches, graph keys and bits).  phi > 0: in EVERY step -- start phase,
                      resampling, look-ahead, probe, propagate rounds, fusion and plain steps, DDIM and solver entries, eager, captured and
                      with a stand-in UNet -- each guided prediction e_r = eu + g (ec_r - eu) is replaced by f_r e_r with
                      f_r = phi sd(ec_r) / sd(e_r) + (1 - phi) (arXiv:2305.08891 section 3.4; 0.7 is the paper's value): tmix_cfg_rescale_factors
                      (two small launches on the eps rows the plan has just written) and then tmix_fused_tweedie_step_rs_dev / _ms_rs_dev in place
                      of the step, in the same captured graph (keys get "rs" appended).  Statistics are per UNet row: on a canvas per window.
                      Not with set_keep.  DESIGN.md 7k.
    eta               in [0, 1], default 0.0 = the deterministic sampler (today's entries, launches, graph keys and bits).  eta > 0: the one move
                      per schedule entry that advances the trajectory -- the fusion step, the plain step, the last PLAIN step of the start
                      timestep, every solver step -- adds cz * z through tmix_fused_tweedie_step_noise_dev, z a pure function of (the
                      trajectory's noise seed, the entry's index in scheduler.timesteps, the element's canvas coordinate) computed inside the
                      step kernel (graph keys get "eta" appended; 48 bytes uploaded).  solver="ddim": the DDIM paper's eta
                      (solver.ddim_eta_coeffs); solver="dpmpp2m": SDE-DPM-Solver++(2M) in k-diffusion's eta form (solver.multistep_eta_coeffs;
                      the first timestep stays a DDIM step); the two definitions coincide at eta = 0 and 1.  Resampling round trips, the
                      look-ahead, the probe and the propagate rounds stay on today's entries.  Needs noise_seeds.  Not with set_keep.
                      DESIGN.md 7n.
    guidance_interval None (every step is guided: today's entries, plan kinds, launches, graph keys, uploads and bits), or (t_hi, t_lo), integer
                      TIMESTEPS with 1000 >= t_hi >= t_lo >= 0 (arXiv:2404.07724): a timestep t is guided iff t_lo <= t <= t_hi.  The
                      trajectory-advancing fusion / plain step (DDIM or solver) of an unguided timestep behind the first runs the UNet WITHOUT
                      the unconditional row (plan kinds "fusion_c" / "fusion_base_c": K rows, "plain_c": one row) and
                      tmix_fused_tweedie_step_cond_dev on its rows: e_c is the conditional prediction itself, the DDIM move takes the eps
                      consistent with the blended estimate, no rescale factors are computed (the factor of g = 1 is 1), and a solver step is
                      second order only when the step before had the same guidedness.  The whole first timestep, the look-ahead, the probe and
                      the propagate rounds stay guided.  An interval that holds every timestep of the schedule is None's run bit for bit.  Not
                      with set_keep.  DESIGN.md 7q.
    apg               None (off: today's entries, plan kinds, launches, graph keys, uploads and bits), or dict(eta=0.0, norm_threshold=0.0):
                      adaptive projected guidance (arXiv:2410.02416).  Every GUIDED step of every phase -- start, resampling, look-ahead,
                      probe, propagate, plain and fusion, DDIM and solver entries, with or without `eta`, eager, captured and with a stand-in
                      UNet -- forms its guidance on the rows' Tweedie estimates: the update tc - tu is split into the part parallel to the
                      conditional estimate tc, which is scaled by apg["eta"] (0 drops it, 1 is CFG), and the rest, which is kept; its norm is
                      clipped at apg["norm_threshold"] (0: no clip).  tmix_apg_coeffs (two small launches on the state and the eps rows the
                      plan has just written) and then tmix_fused_tweedie_step_apg_dev in place of the step, in the same captured graph (keys
                      get a trailing "apg"); both settings are launch arguments fixed at capture, the upload stays 32 or 48 bytes.  Unguided
                      steps (guidance_interval) launch neither.  Statistics are per UNet row: on a canvas per window.  Not with
                      guidance_rescale > 0, not with set_keep.  No momentum.  DESIGN.md 7s.
    noise_seeds      one integer (a 64-bit seed value) per trajectory the caller sees; set_noise_seeds replaces them between runs.  A
                      trajectory's noise depends on its own seed alone: not on what it is co-batched with, the GPU, graphs or windows.
    """

    def __init__(self, config, weights: UNetWeights, text_embeds, text_embeds_single, mask_provider,
                 concept_num: int, lora: bool = False, strict_reference: bool = True, use_graphs: bool = False,
                 n_seeds: int = 1, n_streams: int = 1, vae=None, fp8: bool = False, attention_masks=None, canvas=None,
                 mask_soften=None, solver: str = "ddim", timestep_spacing: str = "leading", guidance_rescale: float = 0.0,
                 eta: float = 0.0, noise_seeds=None, guidance_interval=None, apg=None):
        self.config = config
        self.guidance_interval = validate_interval(guidance_interval)
        self.guidance_rescale = validate_phi(guidance_rescale)
        self.apg = validate_apg(apg)
        if self.apg is not None and self.guidance_rescale > 0.0:     # both re-shape the same prediction and no order between them is defined
            raise ValueError(f"apg={self.apg}: not with guidance_rescale={self.guidance_rescale} (both re-shape the guided prediction; no order "
                             f"between them is defined)")
        self.eta = validate_eta(eta)
        if self.eta > 0.0 and noise_seeds is None:
            raise ValueError(f"eta={self.eta}: noise_seeds (one integer per trajectory) are what the step's noise is a function of")
        if solver not in SOLVERS:
            raise ValueError(f"solver={solver!r}: one of {SOLVERS}")
        self.solver = solver
        self.timestep_spacing = timestep_spacing
        self.fp8 = bool(fp8)          # optional: FF / QKV projections on e4m3 operands (tmix_gemm_fp8); default bf16 like the reference's fp16
        self.W = weights
        self.device = weights.device
        self.concept_num = int(concept_num)
        self.lora = bool(lora)
        self.strict_reference = strict_reference
        self.use_graphs = use_graphs
        # n_seeds independent trajectories share every UNet launch (rows [seed][uncond, concepts...]); the
        # reference runs one seed per process -- co-batching only raises the GEMM M dimension.
        self.n_seeds = int(n_seeds)
        self.n_canvas = self.n_seeds       # trajectories the caller sees (with a canvas, n_seeds below counts their windows)
        self.windows = None                # canvas: [(oy, ox), ...] of the windows on the latent canvas grid, row-major
        # n_streams > 1 splits the rows of every UNet call into that many independent launch chains (PlanGroup)
        self.n_streams = int(n_streams)
        # optional VAE decoder: (config, state_dict) of tweediemix_amd.vae -- enables decode_latent / decoded outputs
        self.vae = vae
        self.vae_scaling_factor = 0.13025       # SDXL VAE config value; the CLI overrides it from the checkpoint's vae/config.json
        self._vae_plans = {}
        # a call is split into chains only when each keeps >= 2 batch rows: the B = 2 CFG-pair calls run faster as ONE chain
        # with the one-workgroup-per-CU tilings (25.3 ms) than as two single-row chains (27.5 ms)
        self.min_rows_per_stream = 2
        self.text_embeds = text_embeds
        self.text_embeds_single = text_embeds_single
        self.mask_provider = mask_provider
        # in-process masks from the look-ahead's cross-attention (masks.attention_masks): the token positions of every foreground
        # concept, flattened into the <= 32 positions one probe plan records
        self.attention_masks = None
        self.attention_maps = None         # after the look-ahead: per seed {level: [n_tok, h_l, w_l]} (raw sums), when attention_masks is set
        self.mask_images = None            # ... and per seed the K-1 uint8 [H, W] masks they gave
        self.propagated_maps = None        # ... and, with propagate >= 1, per seed {level: [n_tok, h_l, w_l]} after the last round
        if attention_masks is not None:
            am = dict(attention_masks)
            toks = [[int(p) for p in c] for c in am["tokens"]]
            if len(toks) != self.concept_num - 1 or any(not c for c in toks):
                raise ValueError(f"attention_masks: {len(toks)} token lists for {self.concept_num - 1} foreground concepts")
            flat = [p for c in toks for p in c]
            if len(flat) > 32:     # tmix_xattn_token_maps_long's limit (more than 8 positions make the probe plan record it)
                raise ValueError(f"attention_masks: {len(flat)} token positions, at most 32 in all")
            if int(config.jumping_steps) < 1:
                raise ValueError("attention_masks needs the look-ahead (jumping_steps >= 1): its calls are where the maps come from")
            prop = am.get("propagate", 0)
            if isinstance(prop, bool) or not isinstance(prop, int) or not 0 <= prop <= 3:
                raise ValueError(f"attention_masks: propagate={prop!r}, an integer 0..3 (rounds through the self-attention)")
            shape = am.get("shape", "rect")
            if shape not in ("rect", "free"):
                raise ValueError(f"attention_masks: shape={shape!r}: 'rect' (bounding rectangles) or 'free' (the component's own outline)")
            self.attention_masks = dict(tokens=toks, flat=flat, threshold=float(am.get("threshold", 0.5)),
                                        levels=am.get("levels"), level_weights=am.get("level_weights"), propagate=prop,
                                        shape=shape, fill_holes=bool(am.get("fill_holes", True)))
        self.mask_soften = None
        self.soft_weights = None           # after a mask acquisition with mask_soften: the weights it produced, on the masks' own grid
        if mask_soften is not None:
            import math
            ms = dict(mask_soften)
            extra = set(ms) - {"feather", "dilate", "normalize"}
            f, r = float(ms.get("feather", 0.0)), float(ms.get("dilate", 0.0))
            if extra or not (math.isfinite(f) and f >= 0.0 and math.isfinite(r)):
                raise ValueError(f"mask_soften: feather={f} (finite, >= 0) dilate={r} (finite) normalize=bool, in latent pixels"
                                 + (f"; unknown keys {sorted(extra)}" if extra else ""))
            self.mask_soften = dict(feather=f, dilate=r, normalize=bool(ms.get("normalize", False)))
        self._mask_buf = None
        self.scheduler = Schedule(config.n_timesteps, spacing=timestep_spacing)
        self.skip = self.scheduler.skip    # None on the "logsnr" grid: the loop asks scheduler.next_t(t)
        self.final_alpha_cumprod = self.scheduler.final_alpha_cumprod
        self.h, self.w = config.resolution_h // 8, config.resolution_w // 8
        self.canvas_h, self.canvas_w = self.h, self.w
        if canvas is not None:
            self._init_canvas(dict(canvas), attention_masks)
        # compute_time_ids, fusion_sampling.py:70-78
        self.add_time_ids = torch.tensor([[config.resolution_h, config.resolution_w, config.crops_coords_top_left_h,
                                           config.crops_coords_top_left_w, config.resolution_h, config.resolution_w]],
                                         dtype=F32)
        self.plans = {}
        self.graphs = {}
        self.unet_calls = []          # (kind, B, t) trace, for tests / accounting
        self.preview_x0 = None
        S = self.n_seeds
        # latent state of the running trajectories (updated in place by every step), its Tweedie estimate, a backup for
        # the jumping look-ahead (fusion_sampling.py:431-447 does not move the trajectory), and the step parameters
        self.x_state = torch.zeros(S, 4, self.h, self.w, device=self.device, dtype=F32)
        self.x0_state = torch.zeros_like(self.x_state)
        self._x_backup = torch.zeros_like(self.x_state)
        # attention_masks with propagate >= 1: the state the last look-ahead call read, which the propagate rounds replay
        self._x_look = torch.zeros_like(self.x_state) if (self.attention_masks or {}).get("propagate") else None
        # {t, sa, s1, sa_next, s1_next, is_last, g, -}; eta > 0: four more floats {cz, step index, 0, 0}, which the noise entry alone reads
        self._n_params = 12 if self.eta > 0.0 else 8
        self.step_params = torch.zeros(self._n_params, device=self.device, dtype=F32)
        self._noise_keys = None          # eta > 0: int32 [n_canvas, 2], every trajectory's key words at an address the captured steps keep
        if noise_seeds is not None:
            self.set_noise_seeds(noise_seeds)
        # solver="dpmpp2m": the blended estimate of the solver step before (tmix_fused_tweedie_step_ms_dev reads and rewrites it; its steps
        # upload {t, sa, s1, cx, c0, c1, is_last, g} into step_params instead) and which step wrote it: (schedule index, step mode, guided) or None
        self._x0_prev = torch.zeros_like(self.x_state) if solver != "ddim" else None
        self._ms_last = None
        # guidance_rescale > 0: the factors [seeds][rows - 1] of the step being run and the fp64 workspace of their reduction, allocated once for
        # the widest call (K + 1 rows; the two-row calls use the front of both) at addresses the captured steps keep
        self._rs_rows = max(self.concept_num + 1, 2)
        self._rs_factors = self._rs_ws = None
        if self.guidance_rescale > 0.0:
            self._rs_factors = torch.ones(S * (self._rs_rows - 1), device=self.device, dtype=F32)
            self._rs_ws = ops.cfg_rescale_ws(self._rs_rows, S, self.device)
        # apg: the {A, B} pairs [seeds][rows - 1][2] of the step being run and the fp64 workspace of their reduction, sized and kept like the
        # rescale's (which never exists at the same time)
        self._apg_coeffs = self._apg_ws = None
        if self.apg is not None:
            self._apg_coeffs = torch.ones(S * (self._rs_rows - 1) * 2, device=self.device, dtype=F32)
            self._apg_ws = ops.cfg_rescale_ws(self._rs_rows, S, self.device)
        self._keep = self._keep_bufs = None   # keep region (set_keep): (x0, weight, eps) in buffers of fixed address; _keep is None while none is set
        self._ring = ParamRing(cuda=self.device.type == "cuda", width=self._n_params)     # staging for the asynchronous upload of step_params
        self._mask_buf = None            # fixed-address copy of self.masks that the captured fusion step reads

    # ------------------------------------------------------------------ wide canvas
    def _init_canvas(self, cv, attention_masks):
        """the windows of a canvas become co-batched row sets: n_seeds <- n_seeds * windows, group-major (b = seed * windows + window)"""
        from . import canvas as CV
        H, Wd, ov = int(cv["height"]), int(cv["width"]), int(cv.get("overlap", 0))
        rh, rw = self.config.resolution_h, self.config.resolution_w
        if H % 8 or Wd % 8 or ov % 8:
            raise ValueError(f"canvas {Wd} x {H}, overlap {ov}: pixel values must be multiples of 8 (the latent grid)")
        if H < rh or Wd < rw or not 0 <= ov < min(rh, rw):
            raise ValueError(f"canvas {Wd} x {H}, overlap {ov}: the canvas must hold the {rw} x {rh} window and 0 <= overlap < {min(rh, rw)}")
        wins = CV.window_layout(H // 8, Wd // 8, self.h, self.w, ov // 8)
        if len(wins) == 1:                 # the canvas is the window: nothing to reconcile, the sampler is today's
            return
        if self.n_seeds * len(wins) > L.MAX_WINDOWS:
            raise ValueError(f"canvas {Wd} x {H}: {len(wins)} windows x {self.n_seeds} seeds = {self.n_seeds * len(wins)} co-batched row sets, at most {L.MAX_WINDOWS}")
        if attention_masks is not None:
            raise ValueError(f"canvas {Wd} x {H}: attention_masks come per window ({len(wins)} windows) and are not stitched; use a mask_provider")
        if self.n_streams > 1:
            raise ValueError(f"canvas {Wd} x {H}: n_streams = {self.n_streams}, a canvas runs on one launch chain (n_streams = 1)")
        self.windows = wins
        self.canvas_h, self.canvas_w = H // 8, Wd // 8
        self.n_seeds = self.n_canvas * len(wins)
        self._pixel_weight = None          # tent weight of the pixel-space blend (decode), built on first use

    def _consensus(self, x):
        """reconcile the windows of every canvas in x [n_seeds, 4, h, w], in place (on the current stream; capturable); returns x"""
        return ops.window_consensus(x, self.n_canvas, self.windows, (self.canvas_h, self.canvas_w))

    def _to_windows(self, x):
        """canvas latents [n_canvas, C, canvas_h, canvas_w] -> [n_seeds, C, h, w]; without a canvas x itself"""
        if self.windows is None:
            return x
        from . import canvas as CV
        want = (self.n_canvas, self.canvas_h, self.canvas_w)
        if x.dim() != 4 or (x.shape[0], x.shape[2], x.shape[3]) != want:
            raise ValueError(f"canvas latent is {tuple(x.shape)}, expected [{want[0]}, C, {want[1]}, {want[2]}]")
        return CV.crop_windows(x, self.windows, self.h, self.w)

    def _to_canvas(self, x):
        """reconciled windows [n_seeds, C, h, w] -> canvas latents [n_canvas, C, canvas_h, canvas_w]; without a canvas a copy of x"""
        if self.windows is None:
            return x.clone()
        from . import canvas as CV
        return CV.assemble(x, self.windows, self.canvas_h, self.canvas_w)

    # ------------------------------------------------------------------ noise seeds
    def set_noise_seeds(self, seeds):
        """the 64-bit seed value of every trajectory's step noise (eta > 0), copied into a buffer of fixed address: captured steps read it"""
        seeds = [int(v) for v in seeds]
        if len(seeds) != self.n_canvas:
            raise ValueError(f"noise_seeds: {len(seeds)} values for {self.n_canvas} trajectories")
        keys = ops.noise_keys(seeds, self.device)
        if self._noise_keys is None:
            self._noise_keys = keys
        else:
            self._noise_keys.copy_(keys)

    # ------------------------------------------------------------------ keep region
    def set_keep(self, x0, weight, eps):
        """Hold part of the latent while the loop samples the rest (re-roll one concept of a finished image, or sample into a template image).
        x0 [1 or S,4,h,w] the clean latent to hold, weight [1 or S,1,h,w] in [0, 1] the weight of the kept part (1: held, 0: sampled), eps [S,4,h,w]
        the fixed noise of every seed's kept part.  From the next run_fusion / sample_loop on every step writes
        weight * (sa' x0 + s1' eps) + (1 - weight) * (its own result), with sa' / s1' of the state it writes (tmix_fused_tweedie_step_keep_dev),
        x_T is composited the same way once, and the final latent holds x0 itself.  The tensors are copied: captured steps read these buffers."""
        if self.guidance_interval is not None:      # the unguided entry holds no keep region
            raise ValueError(f"set_keep: not with guidance_interval={self.guidance_interval} (the keep region exists on the guided step only)")
        if self.eta > 0.0:               # the kept part is re-noised with ONE fixed eps at every level: fresh noise has no place in it
            raise ValueError(f"set_keep: not with eta={self.eta} (the keep region exists on the deterministic step only)")
        if self.guidance_rescale > 0.0:  # a keep entry that takes factors does not exist (yet)
            raise ValueError(f"set_keep: not with guidance_rescale={self.guidance_rescale} (the keep region exists on the unscaled step only)")
        if self.apg is not None:         # the keep entry has no APG form
            raise ValueError(f"set_keep: not with apg={self.apg} (the keep region exists on the step without adaptive projected guidance only)")
        if self.solver != "ddim":        # the keep term needs sa_next / s1_next, which the multistep entry's eight floats do not carry
            raise ValueError(f"set_keep: not with solver={self.solver!r} (the keep region exists on the solver='ddim' step only)")
        if self.windows is not None:     # the mean of equal values is not always that value bit for bit: the kept region's promise would break
            raise ValueError(f"set_keep: not on a canvas ({len(self.windows)} windows on {self.canvas_w * 8} x {self.canvas_h * 8}): "
                             f"reconciling the windows would change the kept bits")
        S = self.n_seeds
        want = (("x0", x0, 4), ("weight", weight, 1), ("eps", eps, 4))
        for name, t, c in want:
            lead = (S,) if name == "eps" else (1, S)
            if t.dim() != 4 or t.shape[0] not in lead or tuple(t.shape[1:]) != (c, self.h, self.w):
                raise ValueError(f"set_keep: {name} is {tuple(t.shape)}, expected [{' or '.join(map(str, lead))}, {c}, {self.h}, {self.w}]")
        new = [t.to(self.device, F32).contiguous() for _n, t, _c in want]
        if self._keep_bufs is not None and all(a.shape == b.shape for a, b in zip(self._keep_bufs, new)):
            for a, b in zip(self._keep_bufs, new):
                a.copy_(b)
        else:                            # other shapes (shared <-> per seed): new buffers, and the steps captured on the old ones go
            for k in [k for k in self.graphs if len(k) == 3]:
                del self.graphs[k]
            self._keep_bufs = [t.clone() for t in new]
        self._keep = tuple(self._keep_bufs)

    def clear_keep(self):
        """back to plain sampling: the plain steps (and their graphs) are used again; the buffers stay for the next set_keep"""
        self._keep = None

    def _composite_keep(self, t):
        """x_state <- w (sa x0 + s1 eps) + (1 - w) x_state at the noise level of timestep t: once, on x_T"""
        kx, kw, ke = self._keep
        sa, s1, _, _ = ops.step_coeffs(self.alpha(t), self.alpha(t))
        self.x_state.copy_(kw * (sa * kx + s1 * ke) + (1.0 - kw) * self.x_state)

    # ------------------------------------------------------------------ schedule
    def alpha(self, t):
        return self.scheduler.alpha(int(t))

    # ------------------------------------------------------------------ plans
    def _routes(self, B):
        return B == 4 if self.strict_reference else B == self.concept_num + 1

    def _build_plan(self, kind):
        K = self.concept_num
        te, tp = self.text_embeds
        if kind in ("fusion", "fusion_base"):
            ehs = torch.cat([te[0:1], te[2:2 + K]])
            pooled = torch.cat([tp[0:1], tp[2:2 + K]])
            routed = kind == "fusion" and self._routes(K + 1) and self.W.kind != "none"
            wsel = list(range(K + 1)) if routed else [0] * (K + 1)
        elif kind == "start":
            ts_, tps = self.text_embeds_single
            ehs = torch.cat([te[0:1], te[1:2], ts_[1:K]])
            pooled = torch.cat([tp[0:1], tp[1:2], tps[1:K]])
            routed, wsel = False, [0] * (K + 1)
        elif kind in ("plain", "probe", "propagate"):
            ehs, pooled, routed, wsel = te[0:2], tp[0:2], False, [0, 0]
        elif kind in ("fusion_c", "fusion_base_c"):   # the unguided twins (guidance_interval): the same rows without the unconditional one
            ehs, pooled = te[2:2 + K], tp[2:2 + K]
            routed = kind == "fusion_c" and self._routes(K + 1) and self.W.kind != "none"     # routed exactly where the guided twin is
            wsel = list(range(1, K + 1)) if routed else [0] * K
        elif kind == "plain_c":
            ehs, pooled, routed, wsel = te[1:2], tp[1:2], False, [0]
        else:
            raise ValueError(kind)
        S = self.n_seeds
        if S > 1:                                     # seed-major rows: b = seed * rows_per_seed + row
            ehs, pooled, wsel = ehs.repeat(S, 1, 1), pooled.repeat(S, 1), list(wsel) * S
        B = ehs.shape[0]
        if kind == "probe":                           # always one chain; maps of every seed's scene-prompt row (b = 2 seed + 1)
            am = self.attention_masks
            spec = TokenMapSpec(tuple(am["flat"]), row0=1, row_step=2, n_rows=S, levels=am["levels"])
            return UNetPlan(self.W, B, self.h, self.w, KVCache(self.W, ehs, wsel), pooled, self.add_time_ids.repeat(B, 1),
                            fp8=self.fp8, token_maps=spec)
        if kind == "propagate":                       # one chain as well; the same rows' maps through every attn1 of the probed levels
            am = self.attention_masks
            spec = TokenPropSpec(len(am["flat"]), row0=1, row_step=2, n_rows=S, levels=am["levels"])
            return UNetPlan(self.W, B, self.h, self.w, KVCache(self.W, ehs, wsel), pooled, self.add_time_ids.repeat(B, 1),
                            fp8=self.fp8, token_prop=spec)
        if self.n_streams > 1 and B % self.n_streams == 0 and B // self.n_streams >= self.min_rows_per_stream:
            return PlanGroup(self.W, self.h, self.w, ehs, wsel, pooled, self.add_time_ids.repeat(B, 1), routed,
                             self.n_streams, fp8=self.fp8)
        kv = KVCache(self.W, ehs, wsel)
        return UNetPlan(self.W, B, self.h, self.w, kv, pooled, self.add_time_ids.repeat(B, 1), routed=routed,
                        row_sets=wsel if routed else None, fp8=self.fp8)

    def plan(self, kind):
        if kind not in self.plans:
            self.plans[kind] = self._build_plan(kind)
        return self.plans[kind]

    def _unet(self, kind, x, t):
        """eps [n_seeds*rows,4,h,w] fp32 for the call kind's prompt rows; each seed's latent is broadcast over
        its rows.  (UNet call alone, eager: used by tests and tools; the sampler itself runs `_run_step`.)"""
        p = self.plan(kind)
        S = self.n_seeds
        self.unet_calls.append((kind, p.B // S, int(t)))
        p.latent.view(S, p.B // S, *p.latent.shape[1:]).copy_(x.unsqueeze(1))
        p.t_dev.fill_(float(t))
        p.run()
        return p.eps

    # ------------------------------------------------------------------ one whole step = one graph
    def _set_masks(self, masks):
        """masks [K,1,h,w] (one seed) or [n_seeds,K,1,h,w]: kept at a fixed address, because captured steps read it."""
        masks = masks.to(self.device, F32).contiguous()
        # the fused step reads K * h * w floats per seed from this buffer: a tensor of another shape must not get here
        assert masks.dim() in (4, 5) and tuple(masks.shape[-4:]) == (self.concept_num, 1, self.h, self.w), tuple(masks.shape)
        if self._mask_buf is None or self._mask_buf.shape != masks.shape:
            assert not any(k[1] == L.STEP_FUSION for k in self.graphs), "mask shape changed after the fusion step was captured"
            self._mask_buf = torch.empty_like(masks)
        self._mask_buf.copy_(masks)

    def _soften(self, m):
        """masks of a source ([K,1,H,W] or [n,K,1,H,W], on the grid they were built on) -> the blend weights mask_soften asks for; m itself without it"""
        if self.mask_soften is None:
            return m
        from . import masks as M
        fg = m[:-1, 0] if m.dim() == 4 else m[:, :-1, 0]
        self.soft_weights = M.soft_masks(fg, device=self.device, **self.mask_soften)
        return self.soft_weights

    @property
    def masks(self):
        """the blend weights the fused step reads.  Assigning sets them RAW: mask_soften applies to the masks the sampler acquires itself
        (mask_provider, attention_masks), not to what is assigned here."""
        return self._mask_buf

    @masks.setter
    def masks(self, m):
        if m is None:
            self._mask_buf = None
        else:
            self._set_masks(m)

    def _enqueue_step(self, kind, mode, ms=False, nz=False):
        """the launches of one denoising step on the current stream: prologue, UNet chains, fused step (in place; ms: the multistep entry;
        nz: the noise entry in its DDIM or multistep form; a kind without the unconditional row, "*_c": the unguided entry)."""
        p = self.plan(kind)
        S = self.n_seeds
        rows = p.B // S
        n = 4 * self.h * self.w
        lib = L.load()
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.tmix_step_prologue(self.x_state.data_ptr(), p.latent.data_ptr(), p.t_dev.data_ptr(),
                                       self.step_params.data_ptr(), S, rows, n, st), "tmix_step_prologue")
        p.run()
        self._fused_step(p.eps.data_ptr(), L.F32, rows, mode, st, ms, **(dict(nz=True) if nz else {}), **(dict(cond=True) if kind.endswith("_c") else {}))
        if self.windows is not None:
            self._consensus(self.x_state)

    def _fused_step(self, eps_ptr, eps_dt, rows, mode, st, ms=False, nz=False, cond=False):
        """the fused step for every seed, in place on x_state; with a keep region set (set_keep) through the entry that holds it; ms: the
        multistep entry, which also reads and rewrites the history buffer; nz: the noise entry (eta > 0), which is all four forms; cond: the
        eps rows hold no unconditional row (an unguided step): the one entry that is all four forms of it, and no rescale factors"""
        lib = L.load()
        m = self._mask_buf if mode == L.STEP_FUSION else None
        mss = 0 if (m is None or m.dim() == 4) else self.concept_num * self.h * self.w
        hw = self.h * self.w
        head = (self.x_state.data_ptr(), eps_ptr, eps_dt, None if m is None else m.data_ptr(), mss, self.x_state.data_ptr(),
                self.x0_state.data_ptr(), self.concept_num, 4, hw, mode, rows, self.n_seeds, self.step_params.data_ptr())
        if cond:                         # x0_prev / keys present or NULL select the move and the noise; the factor of an unguided row is exactly 1
            yx = None
            if nz and self.windows is not None:
                yx = (C.c_int32 * (2 * len(self.windows)))(*[int(v) for o in self.windows for v in o])
            L.check(lib.tmix_fused_tweedie_step_cond_dev(*head, self._x0_prev.data_ptr() if ms else None, self._noise_keys.data_ptr() if nz else None,
                                                         self.w, 1 if yx is None else len(self.windows), yx, self.canvas_h, self.canvas_w, st),
                    "tmix_fused_tweedie_step_cond_dev")
            return
        if self.apg is not None:         # the {A, B} pairs of these eps rows and this state (g, sa, s1 read on the device), then the one APG entry
            if rows > self._rs_rows:
                raise ValueError(f"apg: {rows} eps rows per seed, the buffers were sized for {self._rs_rows}")
            L.check(lib.tmix_apg_coeffs(self.x_state.data_ptr(), eps_ptr, eps_dt, self._apg_coeffs.data_ptr(), self._apg_ws.data_ptr(),
                                        self.concept_num, 4, hw, mode, rows, self.n_seeds, self.step_params.data_ptr(), 7 if ms else 6,
                                        self.apg["eta"], self.apg["norm_threshold"], st), "tmix_apg_coeffs")
            yx = None
            if nz and self.windows is not None:
                yx = (C.c_int32 * (2 * len(self.windows)))(*[int(v) for o in self.windows for v in o])
            L.check(lib.tmix_fused_tweedie_step_apg_dev(*head, self._x0_prev.data_ptr() if ms else None, self._apg_coeffs.data_ptr(),
                                                        self._noise_keys.data_ptr() if nz else None, self.w, 1 if yx is None else len(self.windows),
                                                        yx, self.canvas_h, self.canvas_w, st), "tmix_fused_tweedie_step_apg_dev")
            return
        if self.guidance_rescale > 0.0:  # the factors of these eps rows (g read on the device from the layout the step uploaded), then the rs form of the step
            if rows > self._rs_rows:
                raise ValueError(f"guidance_rescale: {rows} eps rows per seed, the buffers were sized for {self._rs_rows}")
            L.check(lib.tmix_cfg_rescale_factors(eps_ptr, eps_dt, self._rs_factors.data_ptr(), self._rs_ws.data_ptr(), self.concept_num, 4, hw, mode,
                                                 rows, self.n_seeds, self.step_params.data_ptr(), 7 if ms else 6, self.guidance_rescale, st),
                    "tmix_cfg_rescale_factors")
        if nz:                           # x0_prev / factors present or NULL select the parent whose move and rescale the entry takes
            yx = None
            if self.windows is not None:
                yx = (C.c_int32 * (2 * len(self.windows)))(*[int(v) for o in self.windows for v in o])
            L.check(lib.tmix_fused_tweedie_step_noise_dev(*head, self._x0_prev.data_ptr() if ms else None,
                                                          self._rs_factors.data_ptr() if self.guidance_rescale > 0.0 else None,
                                                          self._noise_keys.data_ptr(), self.w, 1 if yx is None else len(self.windows), yx,
                                                          self.canvas_h, self.canvas_w, st), "tmix_fused_tweedie_step_noise_dev")
            return
        if self.guidance_rescale > 0.0:
            if ms:
                L.check(lib.tmix_fused_tweedie_step_ms_rs_dev(*head[:7], self._x0_prev.data_ptr(), *head[7:], self._rs_factors.data_ptr(), st),
                        "tmix_fused_tweedie_step_ms_rs_dev")
            else:
                L.check(lib.tmix_fused_tweedie_step_rs_dev(*head, self._rs_factors.data_ptr(), st), "tmix_fused_tweedie_step_rs_dev")
            return
        if ms:
            L.check(lib.tmix_fused_tweedie_step_ms_dev(*head[:7], self._x0_prev.data_ptr(), *head[7:], st), "tmix_fused_tweedie_step_ms_dev")
            return
        if self._keep is None:
            L.check(lib.tmix_fused_tweedie_step_dev(*head, st), "tmix_fused_tweedie_step_dev")
            return
        kx, kw, ke = self._keep
        L.check(lib.tmix_fused_tweedie_step_keep_dev(*head, kx.data_ptr(), 0 if kx.shape[0] == 1 else 4 * hw, ke.data_ptr(), 4 * hw,
                                                     kw.data_ptr(), 0 if kw.shape[0] == 1 else hw, st), "tmix_fused_tweedie_step_keep_dev")

    def _run_step(self, kind, mode, t, at, at_next, is_last=False, ms=None, step_index=None):
        """x_state <- step(x_state) for every seed; x0_state <- the Tweedie estimate.  Host work per step: eight floats.
        ms = (cx, c0, c1): a multistep solver step (at_next is then not read: the move is in the coefficients).
        step_index (eta > 0 only): the step advances the trajectory from schedule entry step_index and adds that entry's noise; ms is then
        (cx, c0, c1, cz), and a DDIM step's s1_next slot and cz are solver.ddim_eta_coeffs': twelve floats."""
        if "_unet" not in vars(self):
            self.unet_calls.append((kind, self.plan(kind).B // self.n_seeds, int(t)))
        nz = step_index is not None
        nzk = dict(nz=True) if nz else {}                 # a deterministic step calls _enqueue_step / _fused_step with today's arguments
        cond = kind.endswith("_c")                        # an unguided step: the kind has no unconditional row (guidance_interval)
        sa, s1, san, s1n = ops.step_coeffs(at, at_next)
        cz = 0.0
        if nz:
            if ms is None:
                sa, s1, san, s1n, cz = ddim_eta_coeffs(at, at_next, self.eta)
            else:
                cz = ms[3]
        move =(san, s1n) if ms is None else (ms[0], ms[1], ms[2])        # 7 floats, or 8 for a multistep step: the layouts the step kernels read
        vals = [float(t), sa, s1, *move, 1.0 if is_last else 0.0, float(self.config.guidance_scale)]
        if nz:
            vals = (vals + [0.0])[:8] + [0.0 if is_last else cz, float(step_index), 0.0, 0.0]
        ops._fill_params(vals, self._ring.next())
        self._ring.upload(self.step_params, None if self._n_params == 8 else 12 if nz else 8)      # 32 bytes, or 48 for a step with noise
        if mode == L.STEP_FUSION:
            assert self._mask_buf is not None, "fusion step before the masks were acquired"
        if "_unet" in vars(self):
            # a stand-in UNet was attached to this instance (tests replay recorded eps; a caller may plug the reference's own
            # module in): the same fused step, eagerly, on whatever eps dtype the stand-in returns
            eps = self._unet(kind, self.x_state, t).contiguous()
            self._fused_step(eps.data_ptr(), ops._EPS_DT[eps.dtype], eps.shape[0] // self.n_seeds, mode,
                             torch.cuda.current_stream().cuda_stream, ms is not None, **nzk, **(dict(cond=True) if cond else {}))
            if self.windows is not None:
                self._consensus(self.x_state)
            return
        if not self.use_graphs:
            self._enqueue_step(kind, mode, ms is not None, **nzk)
            return
        # a step captured with a keep region is another graph (another kernel, three more pointers): the ones captured without it stay valid
        # and so is a multistep step (another kernel, one more pointer): one graph serves both orders, the order is in the uploaded coefficients
        gkey = (kind, mode, "ms") if ms is not None else (kind, mode) if self._keep is None else (kind, mode, "keep")
        if self.guidance_rescale > 0.0 and not cond:      # two more launches and another step kernel: graphs of their own (an unguided step has neither)
            gkey = gkey + ("rs",)
        if nz:                                            # another entry, two more pointers and the window table: graphs of their own
            gkey = gkey + ("eta",)
        if self.apg is not None and not cond:             # two more launches and the APG entry (eta and R are launch arguments fixed at capture)
            gkey = gkey + ("apg",)
        g = self.graphs.get(gkey)
        if g is None:
            self._enqueue_step(kind, mode, ms is not None, **nzk)    # warm-up outside capture (kernel attributes, lazy module load);
            torch.cuda.synchronize()                      # it has already performed this step, so no replay now
            g = torch.cuda.CUDAGraph()
            keep = self.x_state.clone()
            with torch.cuda.graph(g):
                self._enqueue_step(kind, mode, ms is not None, **nzk)
            self.x_state.copy_(keep)                      # capture does not execute, but keep the state explicit
            self.graphs[gkey] = g
            return
        g.replay()

    # ------------------------------------------------------------------ VAE
    def _decode(self, latent, inv_scale):
        if self.vae is None:
            raise L.TmixError("no VAE weights were given to Tweediemix(vae=(config, state_dict))")
        from .vae import decode_in_groups
        if self.windows is None:
            return decode_in_groups(self.vae, latent, inv_scale, self._vae_plans, self.device)
        # a canvas is decoded window by window through the same plans (the whole canvas would leave the conv kernel's 32-bit offsets and
        # materialise the mid-block attention's [S, S] scores) and the decoded windows are blended in pixel space: the same kernel,
        # offsets x 8, a separable tent weight
        from . import canvas as CV
        n, ch, cw = latent.shape[0], latent.shape[2], latent.shape[3]
        if (ch, cw) != (self.canvas_h, self.canvas_w):
            raise ValueError(f"canvas latent is {tuple(latent.shape)}, expected [n, 4, {self.canvas_h}, {self.canvas_w}]")
        wins = CV.crop_windows(latent.to(self.device, F32), self.windows, self.h, self.w)
        img = decode_in_groups(self.vae, wins, inv_scale, self._vae_plans, self.device).clone()
        if self._pixel_weight is None:
            self._pixel_weight = CV.tent_weight(8 * self.h, 8 * self.w, self.device)
        px = [(8 * oy, 8 * ox) for oy, ox in self.windows]
        ops.window_consensus(img, n, px, (8 * ch, 8 * cw), self._pixel_weight)
        return CV.assemble(img, px, 8 * ch, 8 * cw)

    @torch.no_grad()
    def decode_latent(self, latent):
        """fusion_sampling.py:297-303: the PREVIEW decode, with the reference's 1/0.18215 scale (not SDXL's 0.13025)."""
        return self._decode(latent, 1 / 0.18215)

    @torch.no_grad()
    def decode_final(self, latent):
        """fusion_sampling.py:496-524: x / vae.config.scaling_factor (0.13025) -> decoder -> (img/2+0.5).clamp(0,1)."""
        return self._decode(latent, 1 / self.vae_scaling_factor)

    # ------------------------------------------------------------------ phases
    def init_fusion(self, t_cond, t_stop=None):
        ts = self.scheduler.timesteps
        if self.lora:
            assert t_stop is not None
            self.t_cond = ts[t_cond:t_stop] if t_cond >= 0 else []       # fusion_sampling_lora.py:477
            self.t_stop_cur = ts[t_stop]
        else:
            self.t_cond = ts[t_cond:] if t_cond >= 0 else []             # fusion_sampling.py:477
            self.t_stop_cur = None
        self._window = set(self.t_cond)
        self.t_cond_prev = ts[t_cond - 1]
        self.t_cond_cur = ts[t_cond]
        self.start_t = ts[0]

    def _in_fusion(self, t):
        if self.lora:
            return t <= self.t_cond_cur and t >= self.t_stop_cur
        return t <= self.t_cond_cur

    def _step(self, x, eps, mode, at, at_next, is_last=False, out=None, out_x0=None):
        """fused CFG/Tweedie/blend/DDIM with host-side coefficients (scalar ABI form; tests and tools)."""
        S = self.n_seeds
        if out is None:
            out = torch.empty_like(x)
        rows = eps.shape[0] // S
        for sd in range(S):
            m = None
            if mode == L.STEP_FUSION:
                m = self.masks if self.masks.dim() == 4 else self.masks[sd]
            ops.fused_tweedie_step(x[sd:sd + 1], eps[sd * rows:(sd + 1) * rows], m, mode, self.concept_num,
                                   self.config.guidance_scale, at, at_next, is_last, out_x=out[sd:sd + 1],
                                   out_x0=None if out_x0 is None else out_x0[sd:sd + 1])
        return out

    def _denoise_inplace(self, t):
        """one scheduler timestep on x_state (fusion_sampling.py:309-474)."""
        t = int(t)
        cfg = self.config
        next_t = self.scheduler.next_t(t)
        at, at_next = self.alpha(t), self.alpha(next_t)
        last = t == 1
        solver_step = self.solver != "ddim" and t != self.start_t
        if not solver_step:
            self._ms_last = None                        # a timestep on the DDIM entry leaves no history for a second-order step to use
        # eta > 0: the ONE move of this schedule entry that advances the trajectory takes the entry's noise (the resampling round trips and
        # the look-ahead below stay deterministic: they return to where they started); eta == 0 passes nothing, today's calls
        adv = {}
        if self.eta > 0.0:
            if t not in self.scheduler.timesteps:
                raise ValueError(f"eta={self.eta}: t = {t} is not one of the schedule's timesteps (the noise is indexed by the schedule entry)")
            adv = dict(step_index=self.scheduler.timesteps.index(t))
        # guidance_interval: the trajectory step of a timestep outside it (behind the first timestep) runs without the unconditional row
        c = "" if (t == self.start_t or is_guided(self.guidance_interval, t)) else "_c"
        if solver_step:
            self._solver_step(t, at, at_next, last)
        elif self._in_fusion(t):
            kind = "fusion" if (t in self._window) else "fusion_base"
            self._run_step(kind + c, L.STEP_FUSION, t, at, at_next, last, **adv)
        elif t == self.start_t:
            for _ in range(cfg.resampling_steps):
                self._run_step("start", L.STEP_RESAMPLE, t, at, at_next)
                self._run_step("plain", L.STEP_PLAIN, next_t, at_next, at)        # Tweedie at next_t, re-noise to t
            self._run_step("start", L.STEP_PLAIN, t, at, at_next, last, **adv)
        else:
            self._run_step("plain" + c, L.STEP_PLAIN, t, at, at_next, last, **adv)

        if t == self.t_cond_prev:                       # fusion_sampling.py:431-469
            self._x_backup.copy_(self.x_state)          # the look-ahead does not move the trajectory
            look = "plain"
            if self.attention_masks is not None:        # the same calls, with the token maps recorded (zeroed once, summed over the jumps)
                look = "probe"
                for buf in self.plan("probe").token_maps.values():
                    buf.zero_()
            tt = next_t
            for _ in range(cfg.jumping_steps):
                a_t = self.alpha(tt)
                if self._x_look is not None:
                    self._x_look.copy_(self.x_state)
                self._run_step(look, L.STEP_PLAIN, tt, a_t, self.alpha(tt - 150))
                tt = tt - 150
            self.preview_x0 = (self.x0_state if cfg.jumping_steps else self._x_backup_x0()).clone()
            if self.windows is not None:              # the step reconciles x_state only: the estimate is reconciled here, where it is read
                self.preview_x0 = self._to_canvas(self._consensus(self.preview_x0))
            if self._x_look is not None:              # after the preview, before the restore: what the rounds write into the state is discarded
                self._propagate_rounds(tt + 150)
            self.x_state.copy_(self._x_backup)
            if self.attention_masks is not None:
                m = self._soften(self._masks_from_attention())
            elif self.windows is not None:            # one canvas mask set per seed, cropped into one set per window (a crop of a partition is a partition)
                m = torch.stack([self.mask_provider(self.preview_x0[i:i + 1]).to(self.device, F32) for i in range(self.n_canvas)])
                if tuple(m.shape[1:]) != (self.concept_num, 1, self.canvas_h, self.canvas_w):
                    raise ValueError(f"canvas masks are {tuple(m.shape[1:])}, expected [{self.concept_num}, 1, {self.canvas_h}, {self.canvas_w}]")
                m = self._to_windows(self._soften(m).squeeze(2)).unsqueeze(2)     # softened on the canvas grid: overlapping windows hold identical weights
            elif self.n_seeds == 1:
                m = self.mask_provider(self.preview_x0).to(self.device, F32).contiguous()
                assert m.shape[0] == self.concept_num
                m = self._soften(m)
            else:                                     # one mask set per seed: [n_seeds, K, 1, h, w]
                m = self._soften(torch.stack([self.mask_provider(self.preview_x0[i:i + 1]).to(self.device, F32)
                                              for i in range(self.n_seeds)]).contiguous())
            self._set_masks(m)

    def _solver_step(self, t, at, at_next, last):
        """one trajectory step behind the first timestep through the multistep entry.  Second order exactly when the previous
        _denoise_inplace call ran a solver step of the same mode and the same guidedness (guidance_interval) on the preceding schedule entry
        -- so the first solver step, the first fusion step, the first plain step behind a LoRA t_stop, the first step on either side of an
        interval border and any step asked for out of order are first order.  The whole first timestep, the
        look-ahead and the propagate rounds run the DDIM entry and leave the history buffer alone."""
        ts = self.scheduler.timesteps
        if t not in ts:
            raise ValueError(f"solver={self.solver!r}: t = {t} is not one of the schedule's timesteps {ts}")
        i = ts.index(t)
        if self._in_fusion(t):
            kind, mode = ("fusion" if (t in self._window) else "fusion_base"), L.STEP_FUSION
        else:
            kind, mode = "plain", L.STEP_PLAIN
        guided = is_guided(self.guidance_interval, t)       # the data prediction jumps where g goes from 9 to 1: no extrapolation across a border
        if not guided:
            kind += "_c"
        second = self._ms_last == (i - 1, mode, guided)
        # the last step writes x0 itself: its move (to alpha = 1, or on the 'leading' grid to the alpha it stands on) has no finite h
        if self.eta > 0.0:
            ms = (0.0, 1.0, 0.0, 0.0) if last else multistep_eta_coeffs(self.alpha(ts[i - 1]), at, at_next, second, self.eta)
            self._run_step(kind, mode, t, at, at_next, last, ms=ms, step_index=i)
        else:
            ms = (0.0, 1.0, 0.0) if last else multistep_coeffs(self.alpha(ts[i - 1]), at, at_next, second)
            self._run_step(kind, mode, t, at, at_next, last, ms=ms)
        self._ms_last = (i, mode, guided)

    def _propagate_rounds(self, t):
        """the token maps pushed propagate times through the self-attention of the last look-ahead call (input _x_look, timestep t): round
        1 reads the probe plan's maps, round r the result of round r - 1; prop_dst is zeroed before each round.  Moves x_state / x0_state."""
        prop, probe = self.plan("propagate"), self.plan("probe")
        for r in range(self.attention_masks["propagate"]):
            for lvl, dst in prop.prop_dst.items():
                prop.prop_src[lvl].copy_(probe.token_maps[lvl] if r == 0 else dst)
                dst.zero_()
            self.x_state.copy_(self._x_look)
            self._run_step("propagate", L.STEP_PLAIN, t, self.alpha(t), self.alpha(t - 150))

    def _masks_from_attention(self):
        """[K,1,h,w] (one seed) or [n_seeds,K,1,h,w] from the probe plan's token maps -- with propagate >= 1 from the propagate plan's
        result, the raw maps stay in attention_maps -- (masks.attention_masks + build_masks)"""
        from . import masks as M
        am, cfg = self.attention_masks, self.config
        maps = {lvl: m.cpu().numpy() for lvl, m in self.plan("probe").token_maps.items()}
        pmaps = {lvl: m.cpu().numpy() for lvl, m in self.plan("propagate").prop_dst.items()} if am["propagate"] else None
        n_tok = len(am["flat"])
        idx, k = [], 0
        for c in am["tokens"]:
            idx.append(list(range(k, k + len(c))))
            k += len(c)
        self.attention_maps, self.mask_images, out = [], [], []
        self.propagated_maps = [] if pmaps is not None else None
        for sd in range(self.n_seeds):
            per = {lvl: m[sd].reshape(n_tok, self.h >> lvl, self.w >> lvl) for lvl, m in maps.items()}
            use = per
            if pmaps is not None:
                use = {lvl: m[sd].reshape(n_tok, self.h >> lvl, self.w >> lvl) for lvl, m in pmaps.items()}
                self.propagated_maps.append(use)
            imgs = M.attention_masks(use, idx, cfg.resolution_h, cfg.resolution_w, am["threshold"], am["level_weights"],
                                     shape=am["shape"], fill_holes=am["fill_holes"], device=self.device)
            self.attention_maps.append(per)
            self.mask_images.append(imgs)
            out.append(M.build_masks(imgs, self.h, self.w, self.device))
        return out[0] if self.n_seeds == 1 else torch.stack(out).contiguous()

    def _x_backup_x0(self):
        return self.x0_state            # jumping_steps == 0: the preview is the Tweedie estimate of the step just taken

    @torch.no_grad()
    def denoise_step(self, x, t):
        """x [n_seeds,4,h,w] fp32 on the device, t python int (or 0-dim tensor). Returns the next latent(s)."""
        self.x_state.copy_(self._to_windows(x))
        self._denoise_inplace(t)
        return self._to_canvas(self.x_state)

    def _window_index(self, frac):
        """schedule index of the window fraction frac (t_cond / t_stop).  The 'logsnr' grid keeps the window's NOISE range, not its index
        range: the index of the first timestep at or below the one the 'leading' grid of the same n has at int(n * frac)."""
        i = int(self.config.n_timesteps * frac)
        if self.timestep_spacing == "leading":
            return i
        return self.scheduler.index_at_or_below(Schedule(self.config.n_timesteps).timesteps[i])

    def run_fusion(self, x=None, decode=False):
        cfg = self.config
        t_cond = self._window_index(cfg.t_cond)
        if self.lora:
            self.init_fusion(t_cond, self._window_index(cfg.t_stop))
        else:
            self.init_fusion(t_cond)
        if x is None:      # drawn on the CPU like the reference (fusion_sampling.py:488): device-independent seeds
            x = torch.randn(self.n_canvas, 4, self.canvas_h, self.canvas_w)
        x = x * self.scheduler.init_noise_sigma          # :488 (1.0 for this scheduler), however x arrived
        return self.sample_loop(x.to(self.device, F32), decode=decode)

    @torch.no_grad()
    def sample_loop(self, x, decode=False):
        """runs every scheduler timestep; returns the final latent, or the decoded image [n,3,H,W] in [0,1] when
        decode=True and VAE weights were given (fusion_sampling.py:496-528)."""
        self.x_state.copy_(self._to_windows(x))
        if self._keep is not None:
            self._composite_keep(self.scheduler.timesteps[0])
        for t in self.scheduler.timesteps:
            self._denoise_inplace(t)
        x = self._to_canvas(self.x_state)
        return self.decode_final(x) if decode else x
