#!/usr/bin/env python3
"""Drop-in for the reference's run_video.py (I2VGen-XL image-to-video from the fused image, BASELINE config #5).

The reference script hard-codes its inputs and pulls `ali-vilab/i2vgen-xl` from the hub; here the same settings are flags
with the reference's values as defaults, and the model comes from local files:

  --i2v_path           diffusers-layout I2VGen-XL folder: unet/, tokenizer/ + text_encoder/, image_encoder/ (+ feature_extractor/),
                       vae/ -- prompt embeddings, the CLIP image embedding and the image latents are computed natively from
                       --prompt / --negative_prompt / --image_path (tweediemix_amd/text.py, vae.py, video.py)
  --conditioning_path  optional torch file with any of {'prompt_embeds': [2,77,1024] (negative row first), 'image_embeddings':
                       [2,1024] (zeros row first), 'image_latents': [2,4,F,h,w]} to use instead of computing them
  --alphas_cumprod     .npy with the checkpoint scheduler's 1000-entry table (else: cosine schedule with zero terminal SNR)
  --synthetic          random-init network and conditioning of the real shapes (no checkpoints exist offline)

Per step: native UNet forward on the CFG pair (tweediemix_amd/i2vgen.py) with the first-frame feature injection of
video_gen/utils_attn.py:389-474 for the first int(steps * injection_timestep) steps, then the fused CFG / v-prediction /
DDIM update.  Output: output_i2v_seed_<seed>.latent.pt, plus output_i2v_seed_<seed>.gif with --vae_path.

Many videos per run (a video is one (image, seed) pair; the videos are the images x seeds, image-major):
  --image_path a.png+b.png  several images ('+'-separated); outputs are then named <image stem>_seed_<seed>.*
  --num_seeds N             seeds seed .. seed+N-1; video (image i, seed s) is exactly the single run `--image_path i --seed s`
  --seeds_per_batch K       videos that share every UNet call (0: all of this rank's videos, at most 4; a ragged last batch is padded)
  --gpus G                  videos sharded round-robin over G GPUs (one process per GPU, started by this script); latents (and
                            decoded frames) are gathered over RCCL and rank 0 writes every file
  --output_dir D            where the files go (default .)
Every run, one video or many, goes through tweediemix_amd.video.VideoSampler: the whole step of S videos on the device
(tmix_video_step_prologue -> both CFG chains -> tmix_vpred_step_dev), one parameter upload and one graph replay per timestep;
frames are decoded in batches (vae.decode_in_groups), so a video's GIF does not depend on whether it ran alone or in a batch.

Few-step sampling (no reference counterpart):
  --solver dpmpp2m          every step is a DPM-Solver++(2M) step on the x0 of the v-prediction (tmix_vpred_step_ms_dev)
  --timestep_spacing logsnr the num_inference_steps timesteps uniform in log-SNR from the leading grid's first timestep to 1
Without them (ddim, leading) the run is the reference's loop; an n the grid or the solver cannot take is refused before the GPU is touched.

Guidance rescale (no reference counterpart; arXiv:2305.08891 section 3.4):
  --guidance_rescale PHI    in [0, 1]; 0 (default): off, the run above launch for launch; 0.7: the paper's value.  Every step scales each video's
                            guided v-prediction back towards the standard deviation of its text-conditional one (tmix_vpred_rescale_factors, then
                            tmix_vpred_step_rs_dev / tmix_vpred_step_ms_rs_dev); meant for exactly this setting: zero terminal SNR, v-prediction,
                            --guidance_scale 9.  Combines with every flag above; a value outside [0, 1] is refused before the GPU is touched.

Stochastic sampling (no reference counterpart: the reference hands `eta` to its scheduler):
  --eta E                   in [0, 1]; 0 (default): off, the run above launch for launch.  Every step adds noise generated inside the step kernel
                            (tmix_vpred_step_noise_dev), a pure function of (the video's seed -- the one its x_T is drawn from --, the schedule
                            step, the element's index in the video): the same bits alone, co-batched, on another GPU, eagerly or from a graph.
                            --solver ddim: the DDIM paper's eta; --solver dpmpp2m: SDE-DPM-Solver++(2M) in k-diffusion's eta form, the variant
                            meant for few steps (`--solver dpmpp2m --timestep_spacing logsnr --eta 1`); the two coincide at 0 and 1.  Combines
                            with every flag above; a value outside [0, 1] is refused before the GPU is touched and before any rank starts.

Hold regions (no reference counterpart: the reference's only controls are --injection_timestep and --interp_ratio):
  --hold_masks a.png+b.png  white is HELD: in every frame the union of the masks stays at the held picture while the rest is sampled ("animate
                            the dog, leave the cat and the mountains as they are").  The masks go to the latent grid like the image CLI's; the
                            `<seg_concept>.jpg` files an image run leaves in its side-car directory work as they are.
  --animate_masks a.png+b.png  white MOVES: the complement of the union is held.  One of the two flags at most.
  --hold_feather PX / --hold_dilate PX  ramp width around, and growth of (negative: shrinking), the white region, in image pixels (divided by 8 for
                            the latent grid; the distance-transform kernels of the image CLI's soft masks).  They need one of the mask flags.
  --hold_latents FILE       what is held: by default frame 0 of the video's own conditional image latents -- what the UNet is conditioned on --
                            in every frame; FILE is the `[1,4,F,h,w]` '.latent.pt' of an earlier run, held frame by frame: re-roll one region of a
                            finished clip.  Needs one of the mask flags.
                            The held part is x0 at the noise level of every state under one fixed noise keyed by the video's seed
                            (tmix_video_hold_composite once on x_T, then tmix_vpred_step_hold_dev); the final latent equals the held latent bit
                            for bit wherever the weight is 1.  Rank 0 writes the weight it used as <stem>_hold.png.  Combines with every flag
                            above and --num_seeds N; one mask set describes one image, so several images are refused, like every misuse above,
                            before the GPU is touched and before any rank starts.

Guidance interval (no reference counterpart; Kynkaanniemi et al., arXiv:2404.07724):
  --guidance_interval T_HI,T_LO  a timestep t is guided iff T_LO <= t <= T_HI (the image CLI's flag and validator).  A step outside the interval
                            runs the S text clips alone instead of the CFG pair's 2S (tmix_video_step_prologue_cond, the text half's chain,
                            tmix_vpred_step_cond_dev): half the step's UNet rows, no CFG, and with --guidance_rescale no factors launch.  On the
                            default grid (50 steps, leading) `700,250` guides 22 timesteps and leaves 28 unguided: 72 clips per video instead of
                            100.  With --solver dpmpp2m a step next to a border of the interval is first order.  Combines with every flag above,
                            --streams 1 (which then builds a second, S-clip chain: extra activation memory) and --gpus N; rank 0 prints how many
                            steps are unguided; a malformed interval is refused before the GPU is touched and before any rank starts.  Without the
                            flag, or with an interval that holds every timestep (`1000,0`), the run is the one above launch for launch."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser()
    # the reference script's constants (run_video.py:7-38)
    p.add_argument("--image_path", default="test_out/photo of a cat and a dog running, mountain background_3821.png")
    p.add_argument("--prompt", default="A cat and a dog running, mountain background")
    p.add_argument("--negative_prompt", default="Distorted, discontinuous, Ugly, blurry, low resolution, motionless, static, disfigured, "
                                                "disconnected limbs, Ugly faces, incomplete arms")
    p.add_argument("--seed", type=int, default=6425)
    p.add_argument("--num_inference_steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=9.0)
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=512)
    p.add_argument("--target_fps", type=int, default=8)
    p.add_argument("--num_frames", type=int, default=16)
    p.add_argument("--injection_timestep", type=float, default=0.02)
    p.add_argument("--interp_ratio", type=float, default=0.7)
    # local inputs
    p.add_argument("--i2v_path", default="")
    p.add_argument("--conditioning_path", default="")
    p.add_argument("--alphas_cumprod", default="")
    p.add_argument("--vae_path", default="")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--tiny", action="store_true", help="tiny network (smoke tests)")
    p.add_argument("--no_graphs", action="store_true")
    p.add_argument("--streams", type=int, default=2, choices=[1, 2], help="2: the two clips of the CFG pair run as two launch chains")
    # many videos per run
    p.add_argument("--num_seeds", type=int, default=1, help="videos per image: seeds seed..seed+n-1")
    p.add_argument("--seeds_per_batch", type=int, default=0, help="videos co-batched into every UNet call (0: all of this rank's videos, at most 4)")
    p.add_argument("--gpus", type=int, default=1, help="shard the videos over this many GPUs (one process per GPU, started by this script; at most 8)")
    p.add_argument("--output_dir", default=".")
    # few-step sampling; the defaults are the reference's loop
    p.add_argument("--solver", default="ddim", choices=["ddim", "dpmpp2m"], help="dpmpp2m: every step is a DPM-Solver++(2M) step on the x0 of the v-prediction")
    p.add_argument("--timestep_spacing", default="leading", choices=["leading", "logsnr"], help="logsnr: timesteps uniform in log-SNR from the leading grid's first timestep to 1")
    # guidance rescale; 0 is the run without it
    p.add_argument("--guidance_rescale", type=float, default=0.0, help="phi in [0, 1]: scale each video's guided v-prediction back towards the standard "
                   "deviation of the conditional one (arXiv:2305.08891 section 3.4; 0: off, 0.7: the paper's value)")
    # stochastic sampling; 0 is the run without it
    p.add_argument("--eta", type=float, default=0.0, help="in [0, 1]: every step adds noise computed inside the step kernel from (the video's seed, the "
                   "schedule step, the element's index); ddim: the DDIM paper's eta, dpmpp2m: SDE-DPM-Solver++(2M)'s; 0: off")
    # hold regions; without a mask flag the run has none
    p.add_argument("--hold_masks", default="", help="'+'-separated mask images: white is held at the picture in every frame, the rest is sampled")
    p.add_argument("--animate_masks", default="", help="'+'-separated mask images: white is sampled, the rest is held (not with --hold_masks)")
    p.add_argument("--hold_feather", type=float, default=0.0, help="ramp width in image pixels around the white region of the mask flag")
    p.add_argument("--hold_dilate", type=float, default=0.0, help="grow the white region of the mask flag by this many image pixels (negative: shrink)")
    p.add_argument("--hold_latents", default="", help="'.latent.pt' [1,4,F,h,w] of an earlier run, held frame by frame (default: frame 0 of the "
                   "video's conditional image latents in every frame)")
    p.add_argument("--guidance_interval", default=None, metavar="T_HI,T_LO", help="a timestep t is guided iff T_LO <= t <= T_HI; the steps outside "
                   "run the text clips alone (half the UNet rows, no CFG); default: every step is guided")
    return p


def video_list(image_paths, seed, num_seeds):
    """the run's videos: (image, seed) pairs, image-major."""
    return [(im, seed + k) for im in image_paths for k in range(num_seeds)]


def padded_batches(items, per):
    """consecutive batches of `per` items; a ragged last batch is padded with repeats of its own items.  -> [(batch, n_real)]"""
    out = []
    for b0 in range(0, len(items), per):
        b = items[b0:b0 + per]
        out.append(((b * per)[:per], len(b)))
    return out


def output_stem(image, seed, several_images):
    """output_i2v_seed_<seed> (one image, the reference's name) or <image stem>_seed_<seed> (several images)."""
    if not several_images:
        return f"output_i2v_seed_{seed}"
    return f"{os.path.splitext(os.path.basename(image))[0]}_seed_{seed}"


def check_args(opt):
    """the run's video list; refuses what a multi-video run cannot do (before anything touches the GPU)."""
    images = [p for p in opt.image_path.split("+") if p]
    if not images:
        raise SystemExit("--image_path: no image given")
    if opt.num_seeds < 1 or opt.seeds_per_batch < 0:
        raise SystemExit("--num_seeds must be >= 1 and --seeds_per_batch >= 0")
    if not 1 <= opt.gpus <= 8:
        raise SystemExit("--gpus must be between 1 and 8")
    videos = video_list(images, opt.seed, opt.num_seeds)
    if len(videos) > 1 and opt.conditioning_path:
        raise SystemExit(f"--conditioning_path holds the conditioning of ONE video; this run has {len(videos)} videos "
                         f"({len(images)} image(s) x {opt.num_seeds} seed(s)): drop it or run one image with one seed")
    return images, videos


def checked_rescale(opt):
    """--guidance_rescale through the one validator of phi, on the host before anything touches the GPU or any rank is started"""
    from tweediemix_amd.guidance import validate_phi
    try:
        return validate_phi(opt.guidance_rescale, "--guidance_rescale")
    except ValueError as e:
        raise SystemExit(str(e))


def checked_interval(opt):
    """--guidance_interval through the one validator of the interval, on the host before anything touches the GPU or any rank is started"""
    from tweediemix_amd.guidance import validate_interval
    try:
        return validate_interval(opt.guidance_interval, "--guidance_interval")
    except ValueError as e:
        raise SystemExit(str(e))


def checked_eta(opt):
    """--eta through the one validator of eta, on the host before anything touches the GPU or any rank is started"""
    from tweediemix_amd.solver import validate_eta
    try:
        return validate_eta(opt.eta, "--eta")
    except ValueError as e:
        raise SystemExit(str(e))


def checked_hold(opt, images):
    """the hold flags, on the host before anything touches the GPU or any rank is started -> None (no hold) or dict(masks=[paths], animate=bool,
    soft=(feather, dilate) in latent pixels or None, latents=[1,4,F,h,w] fp32 or None)"""
    flags = [("--hold_feather", opt.hold_feather), ("--hold_dilate", opt.hold_dilate), ("--hold_latents", opt.hold_latents)]
    if opt.hold_masks and opt.animate_masks:
        raise SystemExit("--hold_masks (white is held) and --animate_masks (white moves) describe the same region twice: give one of them")
    spec = opt.hold_masks or opt.animate_masks
    if not spec:
        used = [f"{f} {v}" for f, v in flags if v]
        if used:
            raise SystemExit(f"{' / '.join(used)}: a hold needs its region: --hold_masks or --animate_masks")
        return None
    if len(images) > 1:
        raise SystemExit(f"--hold_masks / --animate_masks: one mask set describes ONE image; this run has {len(images)} (--num_seeds N is fine)")
    paths = [m for m in spec.split("+") if m]
    for m in paths:
        if not os.path.isfile(m):
            raise SystemExit(f"{'--hold_masks' if opt.hold_masks else '--animate_masks'}: no mask file {m!r}")
    if not np.isfinite(opt.hold_feather) or opt.hold_feather < 0.0 or not np.isfinite(opt.hold_dilate):
        raise SystemExit(f"--hold_feather {opt.hold_feather} / --hold_dilate {opt.hold_dilate}: a width >= 0 and a finite distance, in image pixels")
    lat = None
    if opt.hold_latents:
        want = (1, 4, opt.num_frames, opt.height // 8, opt.width // 8)
        if not os.path.isfile(opt.hold_latents):
            raise SystemExit(f"--hold_latents: no file {opt.hold_latents!r}")
        lat = torch.load(opt.hold_latents, map_location="cpu")
        if not torch.is_tensor(lat) or tuple(lat.shape) != want:
            raise SystemExit(f"--hold_latents {opt.hold_latents!r}: {tuple(lat.shape) if torch.is_tensor(lat) else type(lat).__name__}; this run "
                             f"holds a latent of shape {want}")
        lat = lat.float().contiguous()
    soft = (opt.hold_feather / 8.0, opt.hold_dilate / 8.0) if (opt.hold_feather or opt.hold_dilate) else None
    return dict(masks=paths, animate=bool(opt.animate_masks), soft=soft, latents=lat)


def hold_weight(hold, h, w, device):
    """the weight of the held part [1,1,h,w] fp32 on `device` (1 = held): the union of the masks on the latent grid (masks.build_masks, as the
    image CLI's), softened (masks.soft_region), and its complement under --animate_masks"""
    from tweediemix_amd import masks as M
    white = M.build_masks(hold["masks"], h, w, device)[:-1].sum(dim=0, keepdim=True).clamp(max=1.0)
    if hold["soft"] is not None:
        white = M.soft_region(white, hold["soft"][0], hold["soft"][1], device=device)
    return ((1.0 - white) if hold["animate"] else white).clamp(0.0, 1.0).contiguous()


def batch_noise_seeds(seeds, n_real):
    """the noise seeds of one co-batched launch: a video's key is the seed its x_T is drawn from; the videos padded into a ragged last batch
    (their results are dropped) take the key of the batch's last real video"""
    return list(seeds[:n_real]) + [seeds[n_real - 1]] * (len(seeds) - n_real)


def _vae_config(j):
    return dict(block_out_channels=tuple(j["block_out_channels"]), layers_per_block=j.get("layers_per_block", 2),
                latent_channels=j.get("latent_channels", 4), out_channels=j.get("out_channels", 3), groups=j.get("norm_num_groups", 32))


def encode_prompt(opt):
    """encode_prompt: [negative, prompt] last hidden states [2,77,cross] (negative row first, CFG order)."""
    from tweediemix_amd import text as T
    tok = T.ClipBPETokenizer.from_pretrained(os.path.join(opt.i2v_path, "tokenizer"))
    enc = T.load_text_tower(os.path.join(opt.i2v_path, "text_encoder"))
    return enc.last_hidden_state(tok([opt.negative_prompt, opt.prompt])).float().cpu()


def encode_images(opt, paths, need):
    """the CLIP image embeddings [n,cross] ('image_embeddings' in need) and the VAE encoder's (mean, logvar) [n,4,h,w] plus the
    scaling factor ('image_latents' in need) of the images `paths`, each tower run once, batched over the images."""
    import json
    from PIL import Image
    from fusion_generation.fusion_sampling import find_weights, load_state_dict
    from tweediemix_amd import text as T, vae as VA, video as V
    root = opt.i2v_path
    images = [Image.open(p).convert("RGB") for p in paths]
    out = {}
    if "image_embeddings" in need:                  # :623-628 + _encode_image: crop to (w, w), bilinear to the tower's size, CLIP stats
        icfg = json.load(open(os.path.join(root, "image_encoder", "config.json")))
        fx = os.path.join(root, "feature_extractor", "preprocessor_config.json")
        fcfg = json.load(open(fx)) if os.path.exists(fx) else {}
        size = icfg.get("image_size", 224)
        tower = T.ClipVisionEncoder(load_state_dict(find_weights(os.path.join(root, "image_encoder"), "model")), icfg["num_attention_heads"],
                                    icfg["patch_size"], icfg.get("hidden_act", "gelu"), icfg.get("layer_norm_eps", 1e-5))
        kw = {k: tuple(fcfg[k2]) for k, k2 in (("mean", "image_mean"), ("std", "image_std")) if k2 in fcfg}
        px = torch.cat([V.clip_pixel_values(V.resize_bilinear(V.center_crop_wide(im, (opt.width, opt.width)), (size, size)), **kw) for im in images])
        out["image_embeddings"] = tower(px).float().cpu()
    if "image_latents" in need:                     # :631-639 prepare_image_latents, up to the sample
        vdir = os.path.join(root, "vae")
        j = json.load(open(os.path.join(vdir, "config.json")))
        encp = VA.VAEEncoderPlan(_vae_config(j), load_state_dict(find_weights(vdir, "diffusion_pytorch_model")), len(images), opt.height, opt.width)
        px = torch.cat([V.vae_pixel_values(V.center_crop_wide(im, (opt.width, opt.height))) for im in images])
        mean, logvar = encp(px.cuda())
        out["moments"] = (mean.cpu(), logvar.cpu())
        out["scaling_factor"] = j.get("scaling_factor", 0.18215)
    return out


def image_latents(mean, logvar, gen, num_frames, scaling_factor):
    """latent_dist.sample() of one image ([1,4,h,w] moments; the noise is drawn from the video's generator) -> [2,4,F,h,w]."""
    from tweediemix_amd import video as V
    sample = mean + torch.exp(0.5 * logvar) * torch.randn(mean.shape, generator=gen)
    return V.prepare_image_latents(sample, num_frames, scaling_factor)


def unet_state_dict(opt, cfg):
    if opt.synthetic:
        from tweediemix_amd.weights import synthetic_i2vgen_state_dict
        return synthetic_i2vgen_state_dict(cfg)
    if not opt.i2v_path:
        sys.exit("need --i2v_path (or --synthetic); there is no hub download here")
    from fusion_generation.fusion_sampling import find_weights, load_state_dict
    return load_state_dict(find_weights(os.path.join(opt.i2v_path, "unet"), "diffusion_pytorch_model"))


def synthetic_conditioning(cfg, gen, Fr, h, w):
    return {"prompt_embeds": torch.randn(2, 77, cfg.cross_dim, generator=gen), "image_embeddings": torch.randn(2, cfg.cross_dim, generator=gen),
            "image_latents": torch.randn(2, 4, Fr, h, w, generator=gen)}


def video_schedule(opt):
    from tweediemix_amd import video as V
    sched_json = os.path.join(opt.i2v_path, "scheduler", "scheduler_config.json") if opt.i2v_path else ""
    sch_kw = {}
    if opt.alphas_cumprod:
        acp = np.load(opt.alphas_cumprod).astype(np.float32)
    elif sched_json and os.path.exists(sched_json):      # the checkpoint's own DDIMScheduler settings (pipeline_i2vgen_xl.py:480)
        import json
        acp, sch_kw = V.alphas_from_scheduler_config(json.load(open(sched_json)))
    else:                                   # stand-in: the published i2vgen-xl scheduler settings (squaredcos_cap_v2, zero terminal SNR)
        if not opt.synthetic:
            print("warning: no scheduler/scheduler_config.json under --i2v_path and no --alphas_cumprod: using the published "
                  "i2vgen-xl settings (squaredcos_cap_v2, rescale_betas_zero_snr, steps_offset 1, set_alpha_to_one False)")
        acp, sch_kw = V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True,
                                                          steps_offset=1, set_alpha_to_one=False))
    return V.VideoSchedule(acp, opt.num_inference_steps, **sch_kw, spacing=opt.timestep_spacing)


def checked_schedule(opt):
    """the schedule of a run with --solver / --timestep_spacing, built on the host before anything touches the GPU: an n the grid or the solver
    cannot take is refused here.  A run without the flags never comes here: it builds its schedule where it always did."""
    from tweediemix_amd import video as V
    if opt.num_inference_steps < 1:
        raise SystemExit("--num_inference_steps must be >= 1")
    try:
        sch = video_schedule(opt)
        if opt.solver != "ddim":                           # every step's coefficients exist (a zero alpha has no log-SNR)
            phase = V.SolverPhase(sch)
            for t in sch.timesteps:
                phase.coeffs(int(t))
    except ValueError as e:
        raise SystemExit(f"--solver {opt.solver} --timestep_spacing {opt.timestep_spacing} with --num_inference_steps {opt.num_inference_steps}: {e}")
    return sch


def vae_decoder(opt):
    """(config, state dict) of the --vae_path decoder."""
    import json
    from fusion_generation.fusion_sampling import find_weights, load_state_dict
    from tweediemix_amd import vae as VA
    vcfg = VA.FULL
    if os.path.isdir(opt.vae_path) and os.path.exists(os.path.join(opt.vae_path, "config.json")):
        vcfg = _vae_config(json.load(open(os.path.join(opt.vae_path, "config.json"))))
    return vcfg, load_state_dict(find_weights(opt.vae_path, "diffusion_pytorch_model"))


def save_gif(frames_chw, path, fps):
    """frames [F,3,H,W] in [0,1] -> GIF (the pipeline's uint8 conversion)."""
    from PIL import Image
    frames = [Image.fromarray((img.permute(1, 2, 0).float().cpu().numpy() * 255).round().astype("uint8")) for img in frames_chw]
    frames[0].save(path, save_all=True, append_images=frames[1:], duration=1000 // fps, loop=0)


def main(argv=None):
    """every run, one video or many, one rank or many: conditioning batched over the images, VideoSampler over batches of co-batched
    videos, batched decode, the gather to rank 0, which writes every file."""
    opt = build_parser().parse_args(argv)
    images, videos = check_args(opt)
    phi = checked_rescale(opt)
    eta = checked_eta(opt)
    hold = checked_hold(opt, images)
    interval = checked_interval(opt)
    from tweediemix_amd import dist as D, i2vgen as I, launch as LA, video as V
    few_step = (opt.solver, opt.timestep_spacing) != ("ddim", "leading")
    if opt.gpus > 1 and not LA.launched():
        if few_step:
            checked_schedule(opt)                                        # an impossible n is refused before any rank starts
        return LA.self_launch(opt.gpus)                                  # every rank re-reads the same command line, these flags included
    sch = checked_schedule(opt) if few_step else None                    # host only: refusals come before the GPU is touched
    rank, local, world = LA.rank_env()
    if world > 1:
        single = bool(os.environ.get("TMIX_SINGLE_GPU_DIST_TEST"))      # tests: all ranks on GPU 0, gloo
        device = torch.device("cuda:0" if single else f"cuda:{local}")
        torch.cuda.set_device(device)
        D.init(device, world, backend="gloo" if single else None)
    dev = torch.device("cuda", torch.cuda.current_device())
    say = print if rank == 0 else (lambda *a, **k: None)
    cfg = I.TINY if opt.tiny else I.FULL
    h, w, Fr = opt.height // 8, opt.width // 8, opt.num_frames
    if Fr != 16:
        say("note: the reference's injection hook hard-codes 16 frames (video_gen/utils_attn.py:439)")
    mine = D.seed_shard(videos, rank, world)
    sd = unet_state_dict(opt, cfg)
    # what I2VGenXLPipeline.__call__ computes before its loop (video_gen/pipeline_i2vgen_xl.py:604-639): the --conditioning_path entries
    # (one video only) are used as given, only the missing ones are computed, each tower once, batched over the images
    given = torch.load(opt.conditioning_path, map_location="cpu") if opt.conditioning_path and not opt.synthetic else {}
    if not opt.synthetic and mine:
        pe = given["prompt_embeds"] if "prompt_embeds" in given else encode_prompt(opt)
        distinct = sorted(set(im for im, _s in mine), key=images.index)
        need = [k for k in ("image_embeddings", "image_latents") if k not in given]
        enc = encode_images(opt, distinct, need) if need else {}
    # per video, from its own generator in this order: (synthetic conditioning | latent_dist noise, when image_latents is computed), then x_T
    conds, xs = [], []
    for im, seed in mine:
        gen = torch.Generator().manual_seed(seed)
        if opt.synthetic:
            c = synthetic_conditioning(cfg, gen, Fr, h, w)
        else:
            k = distinct.index(im)
            c = dict(given, prompt_embeds=pe)
            if "image_embeddings" in enc:
                emb = enc["image_embeddings"][k:k + 1]
                c["image_embeddings"] = torch.cat([torch.zeros_like(emb), emb])
            if "moments" in enc:
                mean, logvar = enc["moments"]
                c["image_latents"] = image_latents(mean[k:k + 1], logvar[k:k + 1], gen, Fr, enc["scaling_factor"])
        conds.append(c)
        xs.append(torch.randn(1, 4, Fr, h, w, generator=gen))          # latents * init_noise_sigma (= 1 for DDIM)
    Wt = I.I2VWeights(cfg, sd)
    if sch is None:
        sch = video_schedule(opt)                                        # the defaults: built here, as always
    if interval is not None:
        from tweediemix_amd.guidance import unguided_count
        nu = unguided_count(interval, sch.timesteps)
        say(f"guidance interval {interval[0]},{interval[1]}: {nu} of the schedule's {len(sch.timesteps)} steps are unguided (the text clips alone): "
            f"{2 * len(sch.timesteps) - nu} clips per video instead of {2 * len(sch.timesteps)}")
    per = opt.seeds_per_batch or min(max(len(mine), 1), 4)
    hold_w = hold_weight(hold, h, w, dev) if hold is not None and (mine or rank == 0) else None
    lats = []
    smp = plan = None
    for batch, n_real in padded_batches(list(range(len(mine))), per):
        S = len(batch)
        rows = lambda key: torch.cat([conds[i][key][r:r + 1] for r in (0, 1) for i in batch])     # the S unconditional rows, then the S text rows
        fps = torch.tensor([float(opt.target_fps)] * 2 * S)
        fe, ctx, ilf = I.conditioning(Wt, fps, rows("image_latents"), rows("image_embeddings"), rows("prompt_embeds"))
        smp = plan = None                                            # the previous batch's plan and graphs go before the next are built
        plan = I.I2VVideoPlan(Wt, S, Fr, h, w, fe, ctx, ilf, streams=opt.streams, interp=opt.interp_ratio)
        inj = V.FeatureInjector(sch.injection_schedule(opt.injection_timestep), opt.interp_ratio, clips=2 * S, frames=Fr)
        held = None
        if hold is not None:                                         # frame 0 of every video's own conditional image latents, or the given clip
            kx = hold["latents"] if hold["latents"] is not None else torch.cat([conds[i]["image_latents"][1:2, :, 0:1] for i in batch])
            held = (kx.float().contiguous(), hold_w)
        smp = V.VideoSampler(plan, sch, opt.guidance_scale, inj, use_graphs=not opt.no_graphs, solver=opt.solver, guidance_rescale=phi, eta=eta,
                             noise_seeds=batch_noise_seeds([mine[i][1] for i in batch], n_real) if eta > 0.0 or hold is not None else None, hold=held,
                             guidance_interval=interval)
        lats.append(smp.sample(torch.cat([xs[i] for i in batch]).to(dev))[:n_real])
    smp = plan = None
    lat = torch.cat(lats) if lats else torch.zeros(0, 4, Fr, h, w, device=dev)
    img = None
    if opt.vae_path:                                                 # decode_latents (1 / scaling_factor) in batches of frames
        from tweediemix_amd import vae as VA
        vae, plans = vae_decoder(opt), {}
        img = torch.stack([VA.decode_in_groups(vae, v.permute(1, 0, 2, 3).contiguous(), 1 / 0.18215, plans, dev).float().clamp(0, 1)
                           for v in lat]) if len(lat) else torch.zeros(0, Fr, 3, opt.height, opt.width, device=dev)
    if world > 1:                                                    # the result gather: the only collective of a run
        import torch.distributed as dist
        lat = D.gather_latents(lat.contiguous(), len(videos), rank, world)
        if img is not None:
            img = D.gather_latents(img.contiguous(), len(videos), rank, world)
    if rank == 0:
        os.makedirs(opt.output_dir, exist_ok=True)
        several = len(images) > 1
        for i, (im, seed) in enumerate(videos):
            stem = os.path.join(opt.output_dir, output_stem(im, seed, several))
            torch.save(lat[i:i + 1].cpu(), stem + ".latent.pt")
            print("saved", stem + ".latent.pt")
            if img is not None:
                save_gif(img[i], stem + ".gif", opt.target_fps)
                print("saved", stem + ".gif")
            if hold_w is not None:                                   # the weight this run held with, on the latent grid
                from PIL import Image
                Image.fromarray((hold_w[0, 0].cpu().numpy() * 255.0).round().astype("uint8")).save(stem + "_hold.png")
                print("saved", stem + "_hold.png")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return lat


if __name__ == "__main__":
    rc = main()
    sys.exit(rc if isinstance(rc, int) else 0)
